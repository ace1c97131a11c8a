// vdk_wa_tile.h -- tile helpers shared by the window-attention kernels (window_attention.hip: 49 tokens, dot-product logits; window_attention_cos.hip: 64 tokens, cosine
// logits): one wave per (window, head), the head slices of q / k / v / dO staged as [64][32] 16-bit tiles (64-byte rows), every product computed transposed so that the
// softmax axis lies on registers and the query on the lane (see window_attention.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "vdk_device.h"
#include "vdk_attn_tile.h"

#define WA_HD 32
#define WA_LOG2E 1.4426950408889634f
#define WA_FRAG 4096                                        // floats of one [64 q][64 keys] tile in fragment order: [qt][kt][lane][16]

// A lane moves 16 bytes of row 16 i + (lane >> 2), i = 0..3 (4 lanes per 64-byte head slice of a token row, 16 rows per instruction); rr: the tensor rows of those tokens
__device__ __forceinline__ void wa_dma_rows(unsigned char* tile, const bf16_t* __restrict__ base, long ld, const long (&rr)[4], int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16_t* g = base + rr[i] * ld + 8 * (lane & 3);
    __builtin_amdgcn_global_load_lds(VDK_GLOBAL_PTR(g), VDK_LDS_PTR(tile + i * 1024), 16, 0, 0);
  }
}
// MFMA row fragments of such a tile: lane (row 32 t + l31, hi) -> the 16 bytes at columns 16 ks + 8 hi
__device__ __forceinline__ void wa_row_frags(const unsigned char* tile, int l31, int hi, s16x8 (&f)[2][2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f[t][ks] = *(const s16x8*)(tile + (32 * t + l31) * 64 + 32 * ks + 16 * hi);
}
// transposed fragment of a 64-byte-row tile: lane = column l31, slots 0..3 = rows t1 + 4 hi + {0..3}, slots 4..7 = the same + 8 (the contraction order of a C-layout
// tile packed by as_pack_b).  Rows r .. r+3 cover all 64 banks once, the two hi halves take the two passes a 512-byte read needs anyway: no swizzle required.
__device__ __forceinline__ s16x8 wa_tr32(const unsigned char* tile, int t1, int lane) {
  const int s = lane & 15, chalf = (lane >> 4) & 1, hi = lane >> 5;
  const unsigned char* p1 = tile + (t1 + 4 * hi + (s >> 2)) * 64 + 32 * chalf + 8 * (s & 3);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(p1));
  s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(p1 + 8 * 64));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
  return r;
}
// C-layout tile (kt, qt) as bf16 -> the [64 q][64 keys] LDS tile in the AS layout (128-byte rows, 16-byte chunk ^ as_f(row)); f = the tile's two packed B fragments
__device__ __forceinline__ void wa_put_pt(unsigned char* tile, const s16x8 (&f)[2], int kt, int qt, int l31, int hi) {
  const int row = 32 * qt + l31;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const u32x4 u = *(const u32x4*)&f[s];
    *(u32x2*)(tile + row * AS_ROW + (((4 * kt + 2 * s) ^ as_f(row)) << 4) + 8 * hi) = (u32x2){u[0], u[1]};
    *(u32x2*)(tile + row * AS_ROW + (((4 * kt + 2 * s + 1) ^ as_f(row)) << 4) + 8 * hi) = (u32x2){u[2], u[3]};
  }
}
// Output rows.  A C-layout tile of a transposed product has lane = token row, registers = head-dim columns: stored straight from the registers that is 8 bytes per lane
// into 32 different rows per instruction.  The two tiles of an output go through a [64][32] bf16 staging tile in LDS instead (80-byte pitch: the 8-byte writes of 16
// consecutive rows fall on distinct bank pairs) and leave as 16-byte stores, 4 lanes per 64-byte row.
#define WA_ST_PITCH 80
template <int OF = 0>
__device__ __forceinline__ void wa_stage_t(unsigned char* st, const f32x16& x, float mul, int t, int l31, int hi) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *(u32x2*)(st + (32 * t + l31) * WA_ST_PITCH + (8 * g + 4 * hi) * 2) = (u32x2){pack_op2<OF>(x[4 * g] * mul, x[4 * g + 1] * mul), pack_op2<OF>(x[4 * g + 2] * mul, x[4 * g + 3] * mul)};
}
template <int OF = 0>
__device__ __forceinline__ float wa_dot8(const s16x8& a, const s16x8& b) {
  const u32x4 ua = *(const u32x4*)&a, ub = *(const u32x4*)&b;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { s = fmaf(op_lo<OF>(ua[e]), op_lo<OF>(ub[e]), s); s = fmaf(op_hi<OF>(ua[e]), op_hi<OF>(ub[e]), s); }
  return s;
}

// window_attention_f32.hip -- the attention step of timm's Swin Transformer (WindowAttention inside SwinTransformerBlock, the seam of window_attention.hip) with fp32
// operands on the fp32 MFMA (v_mfma_f32_32x32x2_f32): the PRECISE evaluation path of the Swin engine (vdk_swin_forward_f32).  Per (window, head):
//     S = (q * scale) k^T + bias[head] (+ mask[window mod nW]);   P = softmax(S);   o = P v            N = 49 tokens (7 x 7), head dim 32
// qkv: f32 [W * N, ld] rows in (window, token) order or reached through a row index, q | k | v thirds, head h at columns h * 32; o: f32 rows of the same order.  Products
// and sums are IEEE fp32, softmax with the library expf and a true division like vdk_softmax_rows_f32 (csrc/gemm_f32.hip).  Forward only: nothing is kept for a backward.
//
// One wave per (window, head), tokens padded to 64 = two 32-row MFMA tiles, both products TRANSPOSED as in window_attention.hip so that the softmax axis lies on registers
// and the query on the lane.  The fp32 MFMA takes ONE float per lane and step: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]; which element of the
// contraction a (step, k) pair stands for is free as long as A and B agree.  That freedom removes every LDS round trip:
//     S^T[key][q] = K Q^T    step s of 16, half hi: head-dim column 16 hi + s.  A lane's 16 operands of a row are the 64 contiguous bytes [16 hi, 16 hi + 16) of that row's
//                            head slice: four 16-byte global loads per row, the two halves of the wave cover the 128-byte slice.
//                            C layout: lane = q, register r of tile kt = key 32 kt + (r & 3) + 8 (r >> 2) + 4 hi -- the order of the prepared bias tile of the 16-bit kernel
//                            (wa_prep_bias_kernel, -inf on the padded keys), which is reused unchanged.
//     O^T[d][q]   = V^T P^T  step (kt, r) of 32, half hi: key 32 kt + (r & 3) + 8 (r >> 2) + 4 hi, i.e. B IS register r of the P^T tile as the softmax left it, and
//                            A = V[that key][d = lane & 31]: per step the two wave halves read two whole 128-byte rows of V's head slice.
//                            C layout: lane = q, register r = column (r & 3) + 8 (r >> 2) + 4 hi: four 16-byte stores per output row and lane.
// 128 MFMAs per item (64 + 64), no LDS, no barriers.  Tokens >= 49 read token 48 (finite filler): as keys they meet P = exp(-inf) = 0, as queries they are not stored.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "vdk_device.h"
#include "vdk_host.h"

#define WF_N 49
#define WF_HD 32
#define WF_FRAG 4096                                        // floats of one prepared [64 q][64 keys] bias tile (window_attention.hip: [qt][kt][lane][16])

__global__ __launch_bounds__(256) void window_attn_fwd_f32_kernel(const float* __restrict__ qkv, long ld, float* __restrict__ o, long ldo, const float* __restrict__ bm, int nWm,
                                                                  long items, int H, float scale, const int* __restrict__ rowidx) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int w = (int)(threadIdx.x >> 6);
  const int C = H * WF_HD;
  for (long item = (long)blockIdx.x * 4 + w; item < items; item += (long)gridDim.x * 4) {
    const long win = item / H; const int h = (int)(item - win * H);
    // tensor rows of the lane's two tokens 32 t + l31 (query of tile t in the C layout, key of tile t as the A operand)
    int row[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int tok = 32 * t + l31 < WF_N ? 32 * t + l31 : WF_N - 1;
      const long j = win * WF_N + tok;
      row[t] = rowidx ? rowidx[j] : (int)j;
    }
    const float* base = qkv + h * WF_HD;
    f32x4 qf[2][4], kf[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        qf[t][c] = *(const f32x4*)(base + (long)row[t] * ld + 16 * hi + 4 * c);
        kf[t][c] = *(const f32x4*)(base + C + (long)row[t] * ld + 16 * hi + 4 * c);
      }
    // V operands of the second product, issued now so that they travel under the first: step (kt, r) reads key 32 kt + (r & 3) + 8 (r >> 2) + 4 hi, whose row the lane
    // holding that token as l31 knows
    float vf[2][16];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rk = __shfl(row[kt], (r & 3) + 8 * (r >> 2) + 4 * hi);
        vf[kt][r] = base[2 * C + (long)rk * ld + l31];
      }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) qf[t][c] *= scale;          // timm: q = q * scale in front of q @ k^T
    const float* bmp = bm + ((win % nWm) * H + h) * WF_FRAG + lane * 16;
    f32x16 p[2][2];                                           // [qt][kt]: S^T, then P^T
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f32x16 sa;
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) sa = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[kt][c][e], qf[qt][c][e], sa, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b = *(const f32x4*)(bmp + (qt * 2 + kt) * 1024 + 4 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float a = sa[4 * g + e] + b[e]; sa[4 * g + e] = a; mx = fmaxf(mx, a); }
        }
        p[qt][kt] = sa;
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));                     // (key 0 is never padded nor -inf: mx is finite for every query, padded ones included)
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float e = expf(p[qt][kt][r] - mx); p[qt][kt][r] = e; sum += e; }
      sum += __shfl_xor(sum, 32);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[qt][kt][r] *= inv;
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x16 oa;
#pragma unroll
      for (int r = 0; r < 16; ++r) oa[r] = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oa = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[kt][r], p[qt][kt][r], oa, 0, 0, 0);
      if (32 * qt + l31 < WF_N) {
        float* dst = o + (long)row[qt] * ldo + h * WF_HD + 4 * hi;
#pragma unroll
        for (int g = 0; g < 4; ++g) *(f32x4*)(dst + 8 * g) = (f32x4){oa[4 * g], oa[4 * g + 1], oa[4 * g + 2], oa[4 * g + 3]};
      }
    }
  }
}

// window_attention.hip: the bias (+ mask) tile in the kernels' fragment order
size_t vdk_wa_bm_bytes(int32_t nW, int32_t H);
void vdk_wa_prep_bias(const float* bias, const float* mask, int32_t nW, int32_t H, float* bm, void* stream);

// in-library form for the Swin engine: the tile bm is already prepared (vdk_wa_prep_table_batch)
int vdk_wa_fwd_f32_bm(const float* qkv, int64_t ld, float* o, int64_t ldo, const float* bm, int32_t nWm, int64_t windows, int32_t H, float scale, const int32_t* rowidx, void* stream) {
  if (windows * WF_N > INT_MAX) return vdk_fail(VDK_EINVAL, "window attention (fp32): windows * 49 must fit 31 bits");
  const long items = (long)windows * H;
  long grid = (items + 3) / 4; if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(window_attn_fwd_f32_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, qkv, (long)ld, o, (long)ldo, bm, (int)nWm, items, (int)H, scale,
                     (const int*)rowidx);
  return vdk_check_launch("vdk_window_attention_fwd_f32");
}

extern "C" {

/* vdk_window_attention_fwd with fp32 tensors on the fp32 MFMA (evaluation: no lse): qkv f32 [windows * 49, ld], o f32 [windows * 49, ldo]; ld, ldo % 4 == 0 and 16-byte
 * aligned bases.  ws: vdk_window_attention_fwd_workspace_bytes (the same prepared bias tile) */
int vdk_window_attention_fwd_f32(const float* qkv, int64_t ld, float* o, int64_t ldo, const float* bias, const float* mask, int32_t nW, int64_t windows, int32_t H, int32_t N,
                                 int32_t hd, float scale, const int32_t* rowidx, void* ws, size_t ws_bytes, void* stream) {
  if (!qkv || !o || !bias || windows <= 0 || H <= 0 || N <= 0 || hd <= 0 || (ld & 3) || (ldo & 3) || ld < (int64_t)3 * H * hd || ldo < (int64_t)H * hd || (((size_t)qkv | (size_t)o) & 15))
    return vdk_fail(VDK_EINVAL, "vdk_window_attention_fwd_f32: bad argument");
  if (N != WF_N || hd != WF_HD) return vdk_fail(VDK_EUNSUPPORTED, "window attention: 7 x 7 windows (49 tokens) with head dim 32 (every timm swin_*_window7_224)");
  if (mask && (nW <= 0 || windows % nW)) return vdk_fail(VDK_EINVAL, "vdk_window_attention_fwd_f32: bad argument");
  if (!ws || ws_bytes < vdk_wa_bm_bytes(mask ? nW : 0, H)) return vdk_fail(VDK_EWORKSPACE, "vdk_window_attention_fwd_f32: workspace too small");
  vdk_wa_prep_bias(bias, mask, nW, H, (float*)ws, stream);
  return vdk_wa_fwd_f32_bm(qkv, ld, o, ldo, (const float*)ws, mask ? nW : 1, windows, H, scale, rowidx, stream);
}

}  // extern "C"

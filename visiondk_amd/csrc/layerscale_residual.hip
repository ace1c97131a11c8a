// layerscale_residual.hip -- LayerScale on the residual stream of a transformer block (timm `init_values`, the DINOv2 ViTs): x = x + ls(branch(x)), ls(h) = h * gamma.
// The branch's last GEMM (attn.proj / mlp.fc2) leaves h in the 16-bit operand format, as under the reference's autocast; h * gamma promotes to fp32 and the add is fp32:
//   forward    y[r, c]  = x[r, c] + gamma[c] * float(h[r, c])            one fp32 multiply, one fp32 add (the build passes -ffp-contract=off: no fma); y may alias x
//   backward   dh[r, c] = RNE16(gamma[c] * dy[r, c])                     the gradient of the 16-bit tensor, rounded once
//              dgamma[c] = sum_r dy[r, c] * float(h[r, c])               fp32, in a fixed order: per-workgroup column partials, then vdk_reduce_rows_f32 -- no float atomics
// The shortcut's gradient is dy itself (the caller hands it on, no copy).  gamma is 1e-5 at initialisation: nothing here folds it into a weight (a 16-bit copy of
// gamma (.) W2 at that size is what the ConvNeXt engine's power-of-two branch scale exists for); the multiply happens in fp32 on the stream.
// Both kernels are streaming kernels: 8 columns per thread, 16-byte loads and stores, the grid sized from rows x C.  Forward 10 B / element (4 x + 2 h + 4 y), backward 8 B /
// element (4 dy + 2 h + 2 dh); the backward makes ONE pass over dy and h for both of its results.
#include <hip/hip_runtime.h>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_internal.h"

// forward grid: one 8-column item per thread, like the library's cast kernels; the cap (and the grid stride behind it) only keeps the block count inside 31 bits.  Measured at
// 87 680 x 1024, fp16: caps of 2048 / 4096 / 16384 workgroups 163 / 161 / 155 us, no cap 154 us (overridable for A/B builds, tools/ab_build.py)
#ifndef LS_GRID_MAX
#define LS_GRID_MAX (1 << 30)
#endif
#define LS_TX 32              // backward: a workgroup is 32 column groups of 8 (256 columns, 512-byte row segments of h) ...
#define LS_TY 8               // ... x 8 row lanes
// backward grid (overridable for A/B builds, tools/ab_build.py): about LS_BWD_WGS workgroups, at least LS_SPLIT_ROWS rows and at most LS_SPLITS_MAX partial rows per column.
// Measured at 21 920 / 87 680 x 1024, fp16: (2048, 32, 1024) 38.7 / 148 us, (1024, 64, 256) 33.9 / 143 us, (1024, 128, 128) 31.7 / 142 us -- the partials' second launch
// runs on C / 64 workgroups, so fewer partial rows win as long as the first launch still fills the chip
#ifndef LS_BWD_WGS
#define LS_BWD_WGS 1024
#endif
#ifndef LS_SPLIT_ROWS
#define LS_SPLIT_ROWS 128
#endif
#ifndef LS_SPLITS_MAX
#define LS_SPLITS_MAX 128
#endif

template <int OF> __device__ __forceinline__ void ls_widen8(const u32x4 v, f32x4& lo, f32x4& hi) {
  lo = (f32x4){op_lo<OF>(v[0]), op_hi<OF>(v[0]), op_lo<OF>(v[1]), op_hi<OF>(v[1])};
  hi = (f32x4){op_lo<OF>(v[2]), op_hi<OF>(v[2]), op_lo<OF>(v[3]), op_hi<OF>(v[3])};
}

// (x and y are not __restrict__: y may alias x -- every thread reads its 8 elements of x before it writes the same 8 of y)
template <int OF>
__global__ __launch_bounds__(256) void ls_residual_fwd_kernel(const float* x, long ldx, const bf16_t* __restrict__ h, long ldh, const float* __restrict__ gamma, float* y, long ldy,
                                                              long rows, int C8) {
  const long items = rows * C8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
    const long r = i / C8;
    const int c = (int)(i - r * C8) * 8;
    const u32x4 hv = *(const u32x4*)(h + r * ldh + c);
    const f32x4 x0 = *(const f32x4*)(x + r * ldx + c), x1 = *(const f32x4*)(x + r * ldx + c + 4);
    const f32x4 g0 = *(const f32x4*)(gamma + c), g1 = *(const f32x4*)(gamma + c + 4);
    f32x4 h0, h1;
    ls_widen8<OF>(hv, h0, h1);
    const f32x4 p0 = g0 * h0, p1 = g1 * h1;
    *(f32x4*)(y + r * ldy + c) = x0 + p0;
    *(f32x4*)(y + r * ldy + c + 4) = x1 + p1;
  }
}

// one pass over dy and h: dh, and part[split][c] = the split's share of dgamma[c].  grid = (column blocks of 256, row splits); rows [split * rps, (split + 1) * rps)
template <int OF>
__global__ __launch_bounds__(256) void ls_residual_bwd_kernel(const float* __restrict__ dy, long lddy, const bf16_t* __restrict__ h, long ldh, const float* __restrict__ gamma,
                                                              bf16_t* __restrict__ dh, long lddh, float* __restrict__ part, long rows, int C, long rps) {
  __shared__ float red[LS_TY][LS_TX * 8 + 4];
  const int tx = threadIdx.x & (LS_TX - 1), ty = threadIdx.x / LS_TX;
  const int c = (blockIdx.x * LS_TX + tx) * 8;
  const long r0 = (long)blockIdx.y * rps;
  long r1 = r0 + rps; if (r1 > rows) r1 = rows;
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
  if (c < C) {
    const f32x4 g0 = *(const f32x4*)(gamma + c), g1 = *(const f32x4*)(gamma + c + 4);
    long r = r0 + ty;
    for (; r + LS_TY < r1; r += 2 * LS_TY) {      // two rows in flight per thread
      const long q = r + LS_TY;
      const f32x4 d0 = *(const f32x4*)(dy + r * lddy + c), d1 = *(const f32x4*)(dy + r * lddy + c + 4);
      const f32x4 e0 = *(const f32x4*)(dy + q * lddy + c), e1 = *(const f32x4*)(dy + q * lddy + c + 4);
      const u32x4 hv = *(const u32x4*)(h + r * ldh + c), hw = *(const u32x4*)(h + q * ldh + c);
      f32x4 h0, h1, k0, k1;
      ls_widen8<OF>(hv, h0, h1);
      ls_widen8<OF>(hw, k0, k1);
      const f32x4 s0 = g0 * d0, s1 = g1 * d1, t0 = g0 * e0, t1 = g1 * e1;
      *(u32x4*)(dh + r * lddh + c) = (u32x4){pack_op2<OF>(s0[0], s0[1]), pack_op2<OF>(s0[2], s0[3]), pack_op2<OF>(s1[0], s1[1]), pack_op2<OF>(s1[2], s1[3])};
      *(u32x4*)(dh + q * lddh + c) = (u32x4){pack_op2<OF>(t0[0], t0[1]), pack_op2<OF>(t0[2], t0[3]), pack_op2<OF>(t1[0], t1[1]), pack_op2<OF>(t1[2], t1[3])};
      a0 += d0 * h0; a1 += d1 * h1;
      b0 += e0 * k0; b1 += e1 * k1;
    }
    if (r < r1) {
      const f32x4 d0 = *(const f32x4*)(dy + r * lddy + c), d1 = *(const f32x4*)(dy + r * lddy + c + 4);
      const u32x4 hv = *(const u32x4*)(h + r * ldh + c);
      f32x4 h0, h1;
      ls_widen8<OF>(hv, h0, h1);
      const f32x4 s0 = g0 * d0, s1 = g1 * d1;
      *(u32x4*)(dh + r * lddh + c) = (u32x4){pack_op2<OF>(s0[0], s0[1]), pack_op2<OF>(s0[2], s0[3]), pack_op2<OF>(s1[0], s1[1]), pack_op2<OF>(s1[2], s1[3])};
      a0 += d0 * h0; a1 += d1 * h1;
    }
  }
  a0 += b0; a1 += b1;
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[ty][tx * 8 + e] = a0[e]; red[ty][tx * 8 + 4 + e] = a1[e]; }
  __syncthreads();
  const int cl = threadIdx.x, cg = blockIdx.x * (LS_TX * 8) + cl;      // one column per thread, the 8 row lanes in a fixed order
  if (cg < C)
    part[(long)blockIdx.y * C + cg] = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) + ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]));
}

// row splits of the backward: about LS_BWD_WGS workgroups over the column blocks, at least LS_SPLIT_ROWS rows each; -> rows per split, *splits = the non-empty ones
static long ls_rows_per_split(long rows, int C, int* splits) {
  const int bx = (C + LS_TX * 8 - 1) / (LS_TX * 8);
  long target = LS_BWD_WGS / bx; if (target > LS_SPLITS_MAX) target = LS_SPLITS_MAX; if (target < 1) target = 1;
  long s = (rows + LS_SPLIT_ROWS - 1) / LS_SPLIT_ROWS; if (s > target) s = target;
  const long rps = (rows + s - 1) / s;
  *splits = (int)((rows + rps - 1) / rps);
  return rps;
}
static bool ls_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

extern "C" {

int vdk_reduce_rows_f32(const float*, int64_t, int32_t, int64_t, float*, float, void*);

int vdk_ls_residual_fwd(const float* x, int64_t ldx, const void* h, int64_t ldh, const float* gamma, float* y, int64_t ldy, int64_t rows, int32_t C, int32_t opf, void* stream) {
  if (!x || !h || !gamma || !y || rows < 1 || C <= 0 || (C & 7) || (ldx & 3) || ldx < C || (ldh & 7) || ldh < C || (ldy & 3) || ldy < C || ls_misaligned(x) || ls_misaligned(h) ||
      ls_misaligned(gamma) || ls_misaligned(y))
    return vdk_fail(VDK_EINVAL, "vdk_ls_residual_fwd: bad argument (C % 8 == 0; pitches >= C, multiples of 8 (h) / 4 (f32); 16-byte aligned pointers)");
  if (opf != VDK_OPF_BF16 && opf != VDK_OPF_F16) return vdk_fail(VDK_EUNSUPPORTED, "vdk_ls_residual_fwd: operand format 0 (bf16) or 1 (fp16)");
  const long items = (long)rows * (C / 8);
  long grid = (items + 255) / 256; if (grid > LS_GRID_MAX) grid = LS_GRID_MAX;
  if (opf) hipLaunchKernelGGL(ls_residual_fwd_kernel<VDK_OPF_F16>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, (const bf16_t*)h, (long)ldh, gamma, y,
                              (long)ldy, (long)rows, (int)(C / 8));
  else hipLaunchKernelGGL(ls_residual_fwd_kernel<VDK_OPF_BF16>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, (const bf16_t*)h, (long)ldh, gamma, y,
                          (long)ldy, (long)rows, (int)(C / 8));
  return vdk_check_launch("vdk_ls_residual_fwd");
}

/* workspace of vdk_ls_residual_bwd: one f32 [C] row of column partials per row split */
int vdk_ls_residual_bwd_workspace_bytes(int64_t rows, int32_t C, size_t* bytes) {
  if (!bytes || rows < 1 || C <= 0 || (C & 7)) return vdk_fail(VDK_EINVAL, "vdk_ls_residual_bwd_workspace_bytes: bad argument");
  int S = 0;
  ls_rows_per_split((long)rows, C, &S);
  *bytes = (size_t)S * C * 4;
  return VDK_OK;
}

int vdk_ls_residual_bwd(const float* dy, int64_t lddy, const void* h, int64_t ldh, const float* gamma, void* dh, int64_t lddh, float* dgamma, int64_t rows, int32_t C, int32_t opf,
                        void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !h || !gamma || !dh || !dgamma || rows < 1 || C <= 0 || (C & 7) || (lddy & 3) || lddy < C || (ldh & 7) || ldh < C || (lddh & 7) || lddh < C || ls_misaligned(dy) ||
      ls_misaligned(h) || ls_misaligned(gamma) || ls_misaligned(dh) || ls_misaligned(dgamma) || ls_misaligned(ws))
    return vdk_fail(VDK_EINVAL, "vdk_ls_residual_bwd: bad argument (C % 8 == 0; pitches >= C, multiples of 8 (h, dh) / 4 (f32); 16-byte aligned pointers)");
  if (opf != VDK_OPF_BF16 && opf != VDK_OPF_F16) return vdk_fail(VDK_EUNSUPPORTED, "vdk_ls_residual_bwd: operand format 0 (bf16) or 1 (fp16)");
  int S = 0;
  const long rps = ls_rows_per_split((long)rows, C, &S);
  if (!ws || ws_bytes < (size_t)S * C * 4) return vdk_fail(VDK_EWORKSPACE, "vdk_ls_residual_bwd: workspace too small");
  const dim3 grid((unsigned)((C + LS_TX * 8 - 1) / (LS_TX * 8)), (unsigned)S);
  if (opf) hipLaunchKernelGGL(ls_residual_bwd_kernel<VDK_OPF_F16>, grid, dim3(256), 0, (hipStream_t)stream, dy, (long)lddy, (const bf16_t*)h, (long)ldh, gamma, (bf16_t*)dh,
                              (long)lddh, (float*)ws, (long)rows, (int)C, rps);
  else hipLaunchKernelGGL(ls_residual_bwd_kernel<VDK_OPF_BF16>, grid, dim3(256), 0, (hipStream_t)stream, dy, (long)lddy, (const bf16_t*)h, (long)ldh, gamma, (bf16_t*)dh,
                          (long)lddh, (float*)ws, (long)rows, (int)C, rps);
  const int rc = vdk_check_launch("vdk_ls_residual_bwd");
  if (rc) return rc;
  return vdk_reduce_rows_f32((const float*)ws, (int64_t)C, S, (int64_t)C, dgamma, 1.0f, stream);
}

}  // extern "C"

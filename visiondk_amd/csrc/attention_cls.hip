// attention_cls.hip — attention of ONE query row per image: the class token of a classifier's last block (vit_engine.hip, cls_attn_on()).
// With global_pool='token' the head reads token 0 only, so behind the last block's K and V nothing but that token's query, output and gradients is needed:
//   forward   o[b N] = softmax(q[b N] K^T scale) V,   lse of that row                      (reads K and V of every token once)
//   backward  dK, dV of every token (single products: one query row), dQ of the class row, and the per-image column sums of the stored dq | dk | dv rows
//             (the qkv.bias gradient's partials, as attn_s_bwd5_kernel delivers them)         (reads K and V once, writes dK and dV once)
// Both kernels are bound by that K / V stream, so they are plain HIP: no MFMA, no LDS-DMA.  One wave owns a (batch, head) item and walks over the items; a key row is
// spread over the lanes of a row group (8 lanes x 16 bytes at head dim 64; 16 lanes, 10 of them loading, at head dim 80), so a wave-wide load reads whole rows, and
// the contraction over the head dim is a shuffle reduction inside the group.  Sums run in a fixed order (shuffles, no atomics): the result does not depend on the grid.
//
// Arithmetic and rounding points are those of attention_small.hip (attn_s_fwd_kernel / attn_s_bwd5_kernel), so the class row differs from the full kernels' only by
// the order of fp32 summation:
//   forward   raw scores = fp32 sums of 16-bit products; p = exp2(fma(s, scale log2e, -m scale log2e)) with the exact row maximum m; P = p / l in fp32, rounded ONCE
//             to the operand format; o accumulated in fp32 and rounded once; lse = (m scale log2e + log2 l) ln 2
//   backward  p = exp2(fma(s, scale log2e, -lse log2e)); D = sum dO o in fp32 from the stored 16-bit values; dS = p (dP - D); P and dS rounded to the operand format;
//             dV_j = P16_j dO, dK_j = (dS16_j q) scale, dQ = (sum_j dS16_j k_j) scale, each rounded once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_internal.h"

#define AC_WAVES 4                        /* waves (= items in flight) per workgroup */
#define AC_NMAX 1024                      /* keys per item: the forward keeps one fp32 score per key in LDS */
#define AC_U 4                            /* key passes whose loads are issued together: forward (one 16-byte load per lane and pass) ... */
#define AC_UB 2                           /* ... and backward (two loads, two stores; with 4 the kernel sits at 190 registers) */

template <int HD> struct AcGeo {
  static constexpr int CH = HD / 8;                      // 16-byte chunks per row
  static constexpr int LPR = HD == 64 ? 8 : 16;          // lanes per row group (power of two >= CH)
  static constexpr int RPP = 64 / LPR;                   // rows per wave-wide pass
};

template <int OF> __device__ __forceinline__ void ac_unpack(const u32x4& w, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = op_lo<OF>(w[e]); f[2 * e + 1] = op_hi<OF>(w[e]); }
}
__device__ __forceinline__ u32x4 ac_load(const bf16_t* p, bool on) {
  u32x4 z = {0u, 0u, 0u, 0u};
  if (on) z = *(const u32x4*)p;
  return z;
}
template <int OF> __device__ __forceinline__ float ac_dot(const float (&a)[8], const u32x4& w) {
  float b[8];
  ac_unpack<OF>(w, b);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s = fmaf(a[e], b[e], s);
  return s;
}
// sum over the lanes of a row group / over the row groups (lanes with the same chunk): every lane ends with the same value
template <int LPR> __device__ __forceinline__ float ac_group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
template <int LPR> __device__ __forceinline__ float ac_rows_sum(float v) {
#pragma unroll
  for (int m = LPR; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
template <int OF> __device__ __forceinline__ float ac_round(float x) { return op2f<OF>(f2op<OF>(x)); }
template <int OF> __device__ __forceinline__ u32x4 ac_pack(const float (&f)[8]) {
  return (u32x4){pack_op2<OF>(f[0], f[1]), pack_op2<OF>(f[2], f[3]), pack_op2<OF>(f[4], f[5]), pack_op2<OF>(f[6], f[7])};
}

// =====================================================================================  forward
// q is read at row b N only, k and v at every row; o is written at row b N only, lse at [(b H + h) N + 0] only.
template <int HD, int OF>
__global__ __launch_bounds__(64 * AC_WAVES) void attn_cls_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                                      bf16_t* __restrict__ o, long ldo, float* __restrict__ lse, int N, int H, float scale, int nitems) {
  constexpr int CH = AcGeo<HD>::CH, LPR = AcGeo<HD>::LPR, RPP = AcGeo<HD>::RPP;
  __shared__ float sc_all[AC_WAVES * AC_NMAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* const sc = sc_all + w * AC_NMAX;                // this wave's scores, then its unnormalised probabilities
  const int r = lane / LPR, c = lane % LPR;
  const bool cact = c < CH;
  const float scale2 = scale * VDK_LOG2E;
  const int npass = (N + RPP - 1) / RPP;
  for (int item = blockIdx.x * AC_WAVES + w; item < nitems; item += gridDim.x * AC_WAVES) {
    const int b = item / H, h = item - b * H;
    const long off = (long)b * N * ld + h * HD + c * 8;
    float qf[8];
    ac_unpack<OF>(ac_load(q + off, cact), qf);
    VDK_WAVE_LDS_SYNC();                                 // the previous item's readers of sc are done
    float mx = -INFINITY;
    for (int p0 = 0; p0 < npass; p0 += AC_U) {
      u32x4 kk[AC_U];
#pragma unroll
      for (int u = 0; u < AC_U; ++u) { const int row = (p0 + u) * RPP + r; kk[u] = ac_load(k + off + (long)row * ld, cact && row < N); }
#pragma unroll
      for (int u = 0; u < AC_U; ++u) {
        const int row = (p0 + u) * RPP + r;
        const float s = ac_group_sum<LPR>(ac_dot<OF>(qf, kk[u]));
        if (row < N) { mx = fmaxf(mx, s); if (c == 0) sc[row] = s; }
      }
    }
    VDK_WAVE_LDS_SYNC();
    const float m2 = wave_max(mx) * scale2;
    float lsum = 0.f;
    for (int j = lane; j < N; j += 64) { const float p = fast_exp2(fmaf(sc[j], scale2, -m2)); sc[j] = p; lsum += p; }
    const float l = wave_sum(lsum);
    const float inv = 1.0f / l;
    VDK_WAVE_LDS_SYNC();
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p0 = 0; p0 < npass; p0 += AC_U) {
      u32x4 vv[AC_U];
#pragma unroll
      for (int u = 0; u < AC_U; ++u) { const int row = (p0 + u) * RPP + r; vv[u] = ac_load(v + off + (long)row * ld, cact && row < N); }
#pragma unroll
      for (int u = 0; u < AC_U; ++u) {
        const int row = (p0 + u) * RPP + r;
        const float p16 = row < N ? ac_round<OF>(sc[row] * inv) : 0.f;      // P: normalised in fp32, rounded once
        float vf[8];
        ac_unpack<OF>(vv[u], vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(p16, vf[e], acc[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = ac_rows_sum<LPR>(acc[e]);
    if (r == 0 && cact) *(u32x4*)(o + (long)b * N * ldo + h * HD + c * 8) = ac_pack<OF>(acc);
    if (lse && lane == 0) lse[((long)b * H + h) * N] = (m2 + log2f(l)) * 0.6931471805599453f;
  }
}

// =====================================================================================  backward
// q, o, dout, lse are read at row b N only; dk and dv are written at every row, dq at row b N only.  cspart (optional) f32 [B][3][H][HD]: column sums over the item's
// tokens of the dq | dk | dv rows AS STORED (the q third is the class row's dq: the other rows' dq is zero and is not stored).
template <int HD, int OF>
__global__ __launch_bounds__(64 * AC_WAVES) void attn_cls_bwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                                      const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse,
                                                                      bf16_t* __restrict__ dq, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, long ldd, int N, int H, float scale,
                                                                      int nitems, float* __restrict__ cspart) {
  constexpr int CH = AcGeo<HD>::CH, LPR = AcGeo<HD>::LPR, RPP = AcGeo<HD>::RPP;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane / LPR, c = lane % LPR;
  const bool cact = c < CH;
  const float scale2 = scale * VDK_LOG2E;
  const int npass = (N + RPP - 1) / RPP;
  for (int item = blockIdx.x * AC_WAVES + w; item < nitems; item += gridDim.x * AC_WAVES) {
    const int b = item / H, h = item - b * H;
    const long off = (long)b * N * ld + h * HD + c * 8, offo = (long)b * N * ldo + h * HD + c * 8, offd = (long)b * N * ldd + h * HD + c * 8;
    float qf[8], dof[8];
    ac_unpack<OF>(ac_load(q + off, cact), qf);
    const u32x4 dow = ac_load(dout + offo, cact);
    ac_unpack<OF>(dow, dof);
    float of_[8];
    ac_unpack<OF>(ac_load(o + offo, cact), of_);
    const float Dv = ac_group_sum<LPR>(ac_dot<OF>(of_, dow));                // D = sum_d dO_d o_d
    const float lse2 = lse[((long)b * H + h) * N] * VDK_LOG2E;
    float dqa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, csk[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, csv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p0 = 0; p0 < npass; p0 += AC_UB) {
      u32x4 kk[AC_UB], vv[AC_UB];
#pragma unroll
      for (int u = 0; u < AC_UB; ++u) {
        const int row = (p0 + u) * RPP + r;
        kk[u] = ac_load(k + off + (long)row * ld, cact && row < N);
        vv[u] = ac_load(v + off + (long)row * ld, cact && row < N);
      }
#pragma unroll
      for (int u = 0; u < AC_UB; ++u) {
        const int row = (p0 + u) * RPP + r;
        const bool on = row < N;
        const float s = ac_group_sum<LPR>(ac_dot<OF>(qf, kk[u]));
        const float dp = ac_group_sum<LPR>(ac_dot<OF>(dof, vv[u]));
        const float p = on ? fast_exp2(fmaf(s, scale2, -lse2)) : 0.f;
        const float p16 = ac_round<OF>(p), ds16 = ac_round<OF>(p * (dp - Dv));
        float kf[8], gv[8], gk[8];
        ac_unpack<OF>(kk[u], kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) { gv[e] = p16 * dof[e]; gk[e] = (ds16 * qf[e]) * scale; dqa[e] = fmaf(ds16, kf[e], dqa[e]); }
        const u32x4 wv = ac_pack<OF>(gv), wk = ac_pack<OF>(gk);
        if (on && cact) {
          *(u32x4*)(dv + offd + (long)row * ldd) = wv;
          *(u32x4*)(dk + offd + (long)row * ldd) = wk;
        }
        if (cspart && on) {                             // the sums are taken from the rounded values, as stored
          float a[8];
          ac_unpack<OF>(wv, a);
#pragma unroll
          for (int e = 0; e < 8; ++e) csv[e] += a[e];
          ac_unpack<OF>(wk, a);
#pragma unroll
          for (int e = 0; e < 8; ++e) csk[e] += a[e];
        }
      }
    }
    float gq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gq[e] = ac_rows_sum<LPR>(dqa[e]) * scale;
    const u32x4 wq = ac_pack<OF>(gq);
    if (r == 0 && cact) *(u32x4*)(dq + offd) = wq;
    if (cspart) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { csk[e] = ac_rows_sum<LPR>(csk[e]); csv[e] = ac_rows_sum<LPR>(csv[e]); }
      if (r == 0 && cact) {
        float a[8];
        ac_unpack<OF>(wq, a);
        float* const dst = cspart + ((long)b * 3 * H + h) * HD + c * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) { dst[e] = a[e]; dst[(long)H * HD + e] = csk[e]; dst[(long)2 * H * HD + e] = csv[e]; }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
static int ac_grid(int nitems, int grid) {
  int g = (nitems + AC_WAVES - 1) / AC_WAVES;
  if (g > 2048) g = 2048;                               // eight workgroups per CU walk over the items
  if (grid > 0) g = grid;                               // tests: any grid gives the same bits
  return g;
}
// in-library entry points (vit_engine.hip); VDK_EUNSUPPORTED lets the caller fall back to the full-size kernels
bool vdk_attention_cls_serves(int N, int head_dim) { return (head_dim == 64 || head_dim == 80) && N >= 1 && N <= AC_NMAX; }

int vdk_attention_cls_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int opf, int grid,
                          void* stream) {
  if (!vdk_attention_cls_serves(N, head_dim) || (ld & 7) || (ldo & 7) || B <= 0 || H <= 0) return VDK_EUNSUPPORTED;
  const bf16_t* base = (const bf16_t*)qkv;
  const long D = (long)H * head_dim;
  const int nitems = B * H;
  const dim3 g((unsigned)ac_grid(nitems, grid)), blk(64 * AC_WAVES);
  hipStream_t s = (hipStream_t)stream;
#define FW(hd, of) hipLaunchKernelGGL((attn_cls_fwd_kernel<hd, of>), g, blk, 0, s, base, base + D, base + 2 * D, (long)ld, (bf16_t*)o, (long)ldo, lse, (int)N, (int)H, scale, nitems)
  if (head_dim == 64) { if (opf) FW(64, VDK_OPF_F16); else FW(64, VDK_OPF_BF16); }
  else { if (opf) FW(80, VDK_OPF_F16); else FW(80, VDK_OPF_BF16); }
#undef FW
  return VDK_OK;
}

int vdk_attention_cls_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t ldd, float* cspart, int32_t B, int32_t N,
                          int32_t H, int32_t head_dim, float scale, int opf, int grid, void* stream) {
  if (!vdk_attention_cls_serves(N, head_dim) || (ld & 7) || (ldo & 7) || (ldd & 7) || B <= 0 || H <= 0) return VDK_EUNSUPPORTED;
  const bf16_t* base = (const bf16_t*)qkv;
  bf16_t* dbase = (bf16_t*)dqkv;
  const long D = (long)H * head_dim;
  const int nitems = B * H;
  const dim3 g((unsigned)ac_grid(nitems, grid)), blk(64 * AC_WAVES);
  hipStream_t s = (hipStream_t)stream;
#define BW(hd, of) hipLaunchKernelGGL((attn_cls_bwd_kernel<hd, of>), g, blk, 0, s, base, base + D, base + 2 * D, (long)ld, (const bf16_t*)o, (const bf16_t*)dout, (long)ldo, lse, \
                                      dbase, dbase + D, dbase + 2 * D, (long)ldd, (int)N, (int)H, scale, nitems, cspart)
  if (head_dim == 64) { if (opf) BW(64, VDK_OPF_F16); else BW(64, VDK_OPF_BF16); }
  else { if (opf) BW(80, VDK_OPF_F16); else BW(80, VDK_OPF_BF16); }
#undef BW
  return VDK_OK;
}

extern "C" {

// test hooks (csrc/vdk_internal.h): the two kernels on their own, with the grid as a parameter (0: the default)
int vdk_debug_attention_cls_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype,
                                int32_t grid, void* stream) {
  if (!qkv || !o || (dtype != VDK_BF16 && dtype != VDK_F16)) return vdk_fail(VDK_EINVAL, "vdk_debug_attention_cls_fwd: bad argument");
  const int rc = vdk_attention_cls_fwd(qkv, ld, o, ldo, lse, B, N, H, head_dim, scale, dtype == VDK_F16 ? VDK_OPF_F16 : VDK_OPF_BF16, grid, stream);
  if (rc == VDK_EUNSUPPORTED) return vdk_fail(VDK_EUNSUPPORTED, "vdk_debug_attention_cls_fwd: head_dim 64 or 80, N <= 1024, pitches % 8");
  return rc ? rc : vdk_check_launch("vdk_debug_attention_cls_fwd");
}
int vdk_debug_attention_cls_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t ldd, float* cspart, int32_t B,
                                int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype, int32_t grid, void* stream) {
  if (!qkv || !o || !dout || !lse || !dqkv || (dtype != VDK_BF16 && dtype != VDK_F16)) return vdk_fail(VDK_EINVAL, "vdk_debug_attention_cls_bwd: bad argument");
  const int rc = vdk_attention_cls_bwd(qkv, ld, o, dout, ldo, lse, dqkv, ldd, cspart, B, N, H, head_dim, scale, dtype == VDK_F16 ? VDK_OPF_F16 : VDK_OPF_BF16, grid, stream);
  if (rc == VDK_EUNSUPPORTED) return vdk_fail(VDK_EUNSUPPORTED, "vdk_debug_attention_cls_bwd: head_dim 64 or 80, N <= 1024, pitches % 8");
  return rc ? rc : vdk_check_launch("vdk_debug_attention_cls_bwd");
}

}  // extern "C"

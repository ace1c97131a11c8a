// attn_pool.hip — the attention step of timm's AttentionPoolLatent (global_pool='map': SigLIP ViTs, BASELINE.json configs[4]; timm layers/attention_pool.py;
// reference call site: models/classifier/classify_model.py:49-54 -> timm.create_model, and timm_wrapper.py:16-21 for the faceX / CBIR backbones):
//   out[b, h*HD + d] = sum_n softmax_n(scale * <q[h], k[b, n, h]>) v[b, n, h, d]        ONE latent query, N keys per image
// q is the projected latent (f32 [H*HD], the same for every image), kv the bf16 [B*N, 2*H*HD] output of the kv Linear (k | v halves).  This is HBM-bound
// streaming work (each k / v element is used once): one workgroup per (image, head), 256 threads, scores and probabilities in LDS, no MFMA.
// Algorithmic bytes: forward reads kv once (4 B per token and channel pair) ; backward reads kv once and writes dkv once.
// The head dimension HD is a template parameter: 64 (the public vdk_attn_pool_* entries), 72 (SigLIP SO400M: 1152 / 16) and 80 (ViT-H width) through the _hd entries
// of vdk_internal.h.  The channel phase (P V; dk / dv / dq) runs on 256 / HD groups of HD threads -- 4 x 64, 3 x 72, 3 x 80 --, the remaining threads idle.
#include <hip/hip_runtime.h>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_internal.h"

#define AP_MAXN 4096   // keys per image (probabilities live in LDS)

// sum of the NG key groups' partial results in the fixed order ((0 + 1) + (2 + 3)) resp. ((0 + 1) + 2)
template <int NG, int HD>
__device__ __forceinline__ float ap_group_sum(const float (&acc)[NG][HD], int d) {
  static_assert(NG == 3 || NG == 4, "attn_pool: 3 or 4 key groups");
  if constexpr (NG == 4) return (acc[0][d] + acc[1][d]) + (acc[2][d] + acc[3][d]);
  else return (acc[0][d] + acc[1][d]) + acc[2][d];
}

template <int OF, int HD>
__global__ __launch_bounds__(256) void attn_pool_fwd_kernel(const float* __restrict__ q, const bf16_t* __restrict__ kv, long ldkv, int N, int H, float scale,
                                                            float* __restrict__ out, long ldo, float* __restrict__ probs) {
  __shared__ float p_s[AP_MAXN];
  __shared__ float red[4];
  constexpr int NG = 256 / HD;
  __shared__ float acc_s[NG][HD];
  const int b = blockIdx.x / H, h = blockIdx.x % H, tid = threadIdx.x, D = H * HD;
  const bf16_t* kb = kv + (long)b * N * ldkv + h * HD;
  const bf16_t* vb = kb + D;
  // scores: one key per thread per pass; q[h] in registers (HD floats)
  float qr[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) qr[d] = q[h * HD + d] * scale;
  float mx = -3.0e38f;
  for (int n = tid; n < N; n += 256) {
    const u32x4* kr = (const u32x4*)(kb + (long)n * ldkv);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 8; ++c) {
      const u32x4 u = kr[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) { s = fmaf(qr[c * 8 + 2 * e], op_lo<OF>(u[e]), s); s = fmaf(qr[c * 8 + 2 * e + 1], op_hi<OF>(u[e]), s); }
    }
    p_s[n] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max<4>(mx, red);
  float se = 0.f;
  for (int n = tid; n < N; n += 256) { const float e = expf(p_s[n] - mx); p_s[n] = e; se += e; }
  se = block_sum<4>(se, red);
  const float inv = 1.0f / se;
  for (int n = tid; n < N; n += 256) { const float p = p_s[n] * inv; p_s[n] = p; if (probs) probs[((long)b * H + h) * N + n] = p; }
  __syncthreads();
  // out[d] = sum_n p[n] v[n][d]: NG key groups x HD channels (threads NG * HD .. 255 have no channel)
  const int g = HD == 64 ? tid >> 6 : tid / HD, d = HD == 64 ? tid & 63 : tid - g * HD;
  if (NG * HD == 256 || g < NG) {
    float a = 0.f;
    for (int n = g; n < N; n += NG) a = fmaf(p_s[n], op2f<OF>(vb[(long)n * ldkv + d]), a);
    acc_s[g][d] = a;
  }
  __syncthreads();
  if (tid < HD) out[(long)b * ldo + h * HD + tid] = ap_group_sum<NG, HD>(acc_s, tid);
}

// dout f32 [B, H*HD] -> dkv bf16 [B*N, 2*H*HD] (dk | dv), dq_part f32 [B, H*HD] (sum over images = dL/dq)
//   dp[n] = <dout[h], v[n]>, ds[n] = p[n] (dp[n] - sum_m p[m] dp[m]), dk[n] = scale * ds[n] q[h], dv[n] = p[n] dout[h], dq[h] += scale * sum_n ds[n] k[n]
template <int OF, int HD>
__global__ __launch_bounds__(256) void attn_pool_bwd_kernel(const float* __restrict__ q, const bf16_t* __restrict__ kv, long ldkv, const float* __restrict__ probs,
                                                            const float* __restrict__ dout, long lddo, int N, int H, float scale, bf16_t* __restrict__ dkv,
                                                            long lddkv, float* __restrict__ dq_part) {
  __shared__ float ds_s[AP_MAXN];
  __shared__ float red[4];
  constexpr int NG = 256 / HD;
  __shared__ float acc_s[NG][HD];
  const int b = blockIdx.x / H, h = blockIdx.x % H, tid = threadIdx.x, D = H * HD;
  const bf16_t* kb = kv + (long)b * N * ldkv + h * HD;
  const bf16_t* vb = kb + D;
  bf16_t* dkb = dkv + (long)b * N * lddkv + h * HD;
  bf16_t* dvb = dkb + D;
  const float* pr = probs + ((long)b * H + h) * N;
  float gr[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) gr[d] = dout[(long)b * lddo + h * HD + d];
  float dot = 0.f;
  for (int n = tid; n < N; n += 256) {
    const u32x4* vr = (const u32x4*)(vb + (long)n * ldkv);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 8; ++c) {
      const u32x4 u = vr[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) { s = fmaf(gr[c * 8 + 2 * e], op_lo<OF>(u[e]), s); s = fmaf(gr[c * 8 + 2 * e + 1], op_hi<OF>(u[e]), s); }
    }
    ds_s[n] = s;
    dot = fmaf(pr[n], s, dot);
  }
  dot = block_sum<4>(dot, red);
  for (int n = tid; n < N; n += 256) ds_s[n] = pr[n] * (ds_s[n] - dot);
  __syncthreads();
  const int g = HD == 64 ? tid >> 6 : tid / HD, d = HD == 64 ? tid & 63 : tid - g * HD;
  if (NG * HD == 256 || g < NG) {
    const float qd = q[h * HD + d] * scale, gd = dout[(long)b * lddo + h * HD + d];
    float a = 0.f;
    for (int n = g; n < N; n += NG) {
      const float ds = ds_s[n];
      dkb[(long)n * lddkv + d] = f2op<OF>(ds * qd);
      dvb[(long)n * lddkv + d] = f2op<OF>(pr[n] * gd);
      a = fmaf(ds, op2f<OF>(kb[(long)n * ldkv + d]), a);
    }
    acc_s[g][d] = a;
  }
  __syncthreads();
  if (tid < HD) dq_part[(long)b * D + h * HD + tid] = scale * ap_group_sum<NG, HD>(acc_s, tid);
}

template <int OF, int HD>
static void ap_launch_fwd(const float* q, const void* kv, int64_t ldkv, int32_t B, int32_t N, int32_t H, float scale, float* out, int64_t ldo, float* probs, void* stream) {
  hipLaunchKernelGGL((attn_pool_fwd_kernel<OF, HD>), dim3((unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, q, (const bf16_t*)kv, (long)ldkv, (int)N, (int)H, scale, out,
                     (long)ldo, probs);
}
template <int OF, int HD>
static void ap_launch_bwd(const float* q, const void* kv, int64_t ldkv, const float* probs, const float* dout, int64_t lddo, int32_t B, int32_t N, int32_t H, float scale,
                          void* dkv, int64_t lddkv, float* dq_part, void* stream) {
  hipLaunchKernelGGL((attn_pool_bwd_kernel<OF, HD>), dim3((unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, q, (const bf16_t*)kv, (long)ldkv, probs, dout, (long)lddo,
                     (int)N, (int)H, scale, (bf16_t*)dkv, (long)lddkv, dq_part);
}

extern "C" {

// kv / dkv: 16-bit [B*N, 2*H*64] in the format `dtype` (VDK_BF16 | VDK_F16: the trunk's operand format); head_dim 64 (the HD = 64 instances)
int vdk_attn_pool_fwd_dt(const float* q, const void* kv, int64_t ldkv, int32_t B, int32_t N, int32_t H, float scale, float* out, int64_t ldo, float* probs, int32_t dtype,
                         void* stream) {
  if (!q || !kv || !out || B <= 0 || N <= 0 || H <= 0 || N > AP_MAXN || (ldkv & 7) || ldkv < 2L * H * 64 || (dtype != VDK_BF16 && dtype != VDK_F16))
    return vdk_fail(VDK_EINVAL, "vdk_attn_pool_fwd: bad argument (head_dim 64, N <= 4096, ldkv % 8 == 0)");
  if (dtype == VDK_F16) ap_launch_fwd<VDK_OPF_F16, 64>(q, kv, ldkv, B, N, H, scale, out, ldo, probs, stream);
  else ap_launch_fwd<VDK_OPF_BF16, 64>(q, kv, ldkv, B, N, H, scale, out, ldo, probs, stream);
  return vdk_check_launch("vdk_attn_pool_fwd");
}
int vdk_attn_pool_bwd_dt(const float* q, const void* kv, int64_t ldkv, const float* probs, const float* dout, int64_t lddo, int32_t B, int32_t N, int32_t H, float scale,
                         void* dkv, int64_t lddkv, float* dq_part, int32_t dtype, void* stream) {
  if (!q || !kv || !probs || !dout || !dkv || !dq_part || B <= 0 || N <= 0 || H <= 0 || N > AP_MAXN || (ldkv & 7) || ldkv < 2L * H * 64 || lddkv < 2L * H * 64 ||
      (dtype != VDK_BF16 && dtype != VDK_F16))
    return vdk_fail(VDK_EINVAL, "vdk_attn_pool_bwd: bad argument");
  if (dtype == VDK_F16) ap_launch_bwd<VDK_OPF_F16, 64>(q, kv, ldkv, probs, dout, lddo, B, N, H, scale, dkv, lddkv, dq_part, stream);
  else ap_launch_bwd<VDK_OPF_BF16, 64>(q, kv, ldkv, probs, dout, lddo, B, N, H, scale, dkv, lddkv, dq_part, stream);
  return vdk_check_launch("vdk_attn_pool_bwd");
}
// vdk_internal.h: the same two with the head dimension as an argument, 64 | 72 | 80 (q f32 [H*head_dim], kv / dkv [B*N, 2*H*head_dim], out / dout / dq_part [B, H*head_dim])
int vdk_attn_pool_fwd_hd(const float* q, const void* kv, int64_t ldkv, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, float* out, int64_t ldo, float* probs,
                         int32_t dtype, void* stream) {
  if (head_dim != 64 && head_dim != 72 && head_dim != 80) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attn_pool_fwd_hd: head_dim must be 64, 72 or 80");
  if (!q || !kv || !out || B <= 0 || N <= 0 || H <= 0 || N > AP_MAXN || (ldkv & 7) || ldkv < 2L * H * head_dim || ldo < (long)H * head_dim || (dtype != VDK_BF16 && dtype != VDK_F16))
    return vdk_fail(VDK_EINVAL, "vdk_attn_pool_fwd_hd: bad argument (N <= 4096, ldkv % 8 == 0, ldkv >= 2 * H * head_dim)");
  const bool f16 = dtype == VDK_F16;
#define AP_FWD(OF, HD_) ap_launch_fwd<OF, HD_>(q, kv, ldkv, B, N, H, scale, out, ldo, probs, stream)
  if (head_dim == 64) f16 ? AP_FWD(VDK_OPF_F16, 64) : AP_FWD(VDK_OPF_BF16, 64);
  else if (head_dim == 72) f16 ? AP_FWD(VDK_OPF_F16, 72) : AP_FWD(VDK_OPF_BF16, 72);
  else f16 ? AP_FWD(VDK_OPF_F16, 80) : AP_FWD(VDK_OPF_BF16, 80);
#undef AP_FWD
  return vdk_check_launch("vdk_attn_pool_fwd_hd");
}
int vdk_attn_pool_bwd_hd(const float* q, const void* kv, int64_t ldkv, const float* probs, const float* dout, int64_t lddo, int32_t B, int32_t N, int32_t H, int32_t head_dim,
                         float scale, void* dkv, int64_t lddkv, float* dq_part, int32_t dtype, void* stream) {
  if (head_dim != 64 && head_dim != 72 && head_dim != 80) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attn_pool_bwd_hd: head_dim must be 64, 72 or 80");
  if (!q || !kv || !probs || !dout || !dkv || !dq_part || B <= 0 || N <= 0 || H <= 0 || N > AP_MAXN || (ldkv & 7) || ldkv < 2L * H * head_dim || lddkv < 2L * H * head_dim ||
      lddo < (long)H * head_dim || (dtype != VDK_BF16 && dtype != VDK_F16))
    return vdk_fail(VDK_EINVAL, "vdk_attn_pool_bwd_hd: bad argument (N <= 4096, ldkv % 8 == 0, ldkv and lddkv >= 2 * H * head_dim)");
  const bool f16 = dtype == VDK_F16;
#define AP_BWD(OF, HD_) ap_launch_bwd<OF, HD_>(q, kv, ldkv, probs, dout, lddo, B, N, H, scale, dkv, lddkv, dq_part, stream)
  if (head_dim == 64) f16 ? AP_BWD(VDK_OPF_F16, 64) : AP_BWD(VDK_OPF_BF16, 64);
  else if (head_dim == 72) f16 ? AP_BWD(VDK_OPF_F16, 72) : AP_BWD(VDK_OPF_BF16, 72);
  else f16 ? AP_BWD(VDK_OPF_F16, 80) : AP_BWD(VDK_OPF_BF16, 80);
#undef AP_BWD
  return vdk_check_launch("vdk_attn_pool_bwd_hd");
}
int vdk_attn_pool_fwd(const float* q, const void* kv, int64_t ldkv, int32_t B, int32_t N, int32_t H, float scale, float* out, int64_t ldo, float* probs, void* stream) {
  return vdk_attn_pool_fwd_dt(q, kv, ldkv, B, N, H, scale, out, ldo, probs, VDK_BF16, stream);
}
int vdk_attn_pool_bwd(const float* q, const void* kv, int64_t ldkv, const float* probs, const float* dout, int64_t lddo, int32_t B, int32_t N, int32_t H, float scale,
                      void* dkv, int64_t lddkv, float* dq_part, void* stream) {
  return vdk_attn_pool_bwd_dt(q, kv, ldkv, probs, dout, lddo, B, N, H, scale, dkv, lddkv, dq_part, VDK_BF16, stream);
}

}  // extern "C"

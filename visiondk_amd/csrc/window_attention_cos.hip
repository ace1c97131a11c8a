// window_attention_cos.hip -- the attention step of timm's SwinV2 (WindowAttention of swin_transformer_v2.py inside SwinTransformerV2Block), the `window8_256` family the
// reference's configs list as alternatives (`timm-swinv2_base_window8_256.ms_in1k`).  Per (window, head):
//     qn_i = q_i / max(|q_i|, 1e-12), kn_j likewise;   S = tau_h (qn kn^T) + bias[head] (+ mask[window mod nW]);   P = softmax(S);   o = P v      N = 64 tokens (8 x 8), head dim 32
// qkv: 16-bit [W * N, ld] rows in (window, token) order or reached through a row index, q | k | v thirds, head h at columns h * 32; tau f32 [H] = exp(min(logit_scale, ln 100)),
// formed by the caller; bias f32 [H, N, N] (16 sigmoid of the coordinate MLP, gathered by the caller); mask f32 [nW, N, N] (0 / -100) or NULL.
// Arithmetic as under the reference's autocast: the norms are fp32 sums over the 32 stored 16-bit values, qn and kn are rounded to the operand format (what autocast does to
// the fp32 output of F.normalize ahead of the matmul), fp32 products and sums, softmax in fp32, P rounded once as the left operand of P v, o rounded.
//
// Structure: that of window_attention.hip (one wave per item, [64][32] tiles by LDS-DMA, transposed products, bias + mask prepared once per call in the MFMA C layout); the
// 64 tokens fill the [64 q][64 keys] tile, so nothing is padded.  What is new: the normalisation pass over the staged q and k tiles (in place: 4 lanes per row, the lane layout
// of the DMA), and in the backward its Jacobian on the fp32 d(qn) / d(kn) before their one rounding, and d(tau).
#include <hip/hip_runtime.h>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_attn_tile.h"
#include "vdk_wa_tile.h"
#include "vdk_internal.h"

#define WC_N 64
#define WC_BW 2                                             // waves per workgroup of the backward
#define WC_EPS 1e-12f                                       // F.normalize's eps
#ifndef WC_AB
#define WC_AB 0                                             // timing A/B builds only (tools/ab_build.py; results are WRONG with any bit set): 1 skips the normalisation
#endif                                                      // pass, 2 the Jacobian pass (d(qn) / d(kn) leave as 16-bit rows), 4 the d(tau) accumulation
#define WC_F32_PITCH 144                                    // bytes per row of the fp32 staging tile of d(qn) / d(kn): 32 floats + 16 bytes (row starts 4 banks apart)

// element (qt, kt, lane, r) of the fragment order <-> query 32 qt + (lane & 31), key 32 kt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__global__ __launch_bounds__(256) void wc_prep_bias_kernel(const float* __restrict__ bias, const float* __restrict__ mask, int nWm, int H, float* __restrict__ bm) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nWm * H * WA_FRAG) return;
  const int r = (int)(i & 15), lane = (int)((i >> 4) & 63), kt = (int)((i >> 10) & 1), qt = (int)((i >> 11) & 1);
  const long wh = i >> 12; const int h = (int)(wh % H); const long wm = wh / H;
  const int q = 32 * qt + (lane & 31), key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
  float v = bias[((long)h * WC_N + q) * WC_N + key];
  if (mask) v += mask[(wm * WC_N + q) * WC_N + key];
  bm[i] = v;
}
__global__ __launch_bounds__(256) void wc_unprep_dbias_kernel(const float* __restrict__ red, int H, float* __restrict__ dbias) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * WC_N * WC_N) return;
  const int key = (int)(i & 63), q = (int)((i >> 6) & 63); const long h = i >> 12;
  const int kk = key & 31, hi = (kk >> 2) & 1, r = (kk & 3) + 4 * (kk >> 3), lane = (q & 31) + 32 * hi;
  dbias[i] = red[h * WA_FRAG + ((((q >> 5) * 2 + (key >> 5)) * 64 + lane) << 4) + r];
}

// tensor rows of the tokens 16 i + (lane >> 2) of window `win` (rowidx: token j of window w lives in tensor row rowidx[w * 64 + j])
__device__ __forceinline__ void wc_rows(const int* __restrict__ rowidx, long win, int lane, long (&rr)[4]) {
  long j[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) j[i] = win * WC_N + 16 * i + (lane >> 2);
  if (rowidx) {      // ONE branch around four independent loads
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = rowidx[j[i]];
#pragma unroll
    for (int i = 0; i < 4; ++i) rr[i] = v[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) rr[i] = j[i];
  }
}
// the 64 rows of the 16-bit staging tile -> the tensor rows rr
__device__ __forceinline__ void wc_flush_rows(const unsigned char* st, const long (&rr)[4], bf16_t* __restrict__ base, long ld, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *(u32x4*)(base + rr[i] * ld + 8 * (lane & 3)) = *(const u32x4*)(st + (16 * i + (lane >> 2)) * WA_ST_PITCH + 16 * (lane & 3));
}
template <int OF>
__device__ __forceinline__ void wc_unpack8(const u32x4& u, float (&x)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { x[2 * e] = op_lo<OF>(u[e]); x[2 * e + 1] = op_hi<OF>(u[e]); }
}
// x / max(|x|, eps) over the rows of a staged [64][32] tile, in place, rounded to the operand format.  A lane holds 8 values of row 16 i + (lane >> 2); the four lanes of a
// row add their partial sums of squares in a fixed order.  raw / den: the lane's stored values and its rows' denominators, for the Jacobian of the backward.
template <int OF>
__device__ __forceinline__ void wc_normalize(unsigned char* tile, int lane, u32x4 (&raw)[4], float (&den)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) raw[i] = *(const u32x4*)(tile + i * 1024 + lane * 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (WC_AB & 1) { den[i] = 1.f; continue; }
    float x[8];
    wc_unpack8<OF>(raw[i], x);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(x[e], x[e], ss);
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    den[i] = fmaxf(sqrtf(ss), WC_EPS);
    *(u32x4*)(tile + i * 1024 + lane * 16) = (u32x4){pack_op2<OF>(x[0] / den[i], x[1] / den[i]), pack_op2<OF>(x[2] / den[i], x[3] / den[i]),
                                                     pack_op2<OF>(x[4] / den[i], x[5] / den[i]), pack_op2<OF>(x[6] / den[i], x[7] / den[i])};
  }
  // the backward meets raw again at its very end: keep the 16 packed registers alive until then, not the 64 unpacked values and their 64 quotients
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned a = raw[i][0], b = raw[i][1], c = raw[i][2], d = raw[i][3];
    VDK_PIN2(a, b); VDK_PIN2(c, d);
    raw[i] = (u32x4){a, b, c, d};
  }
}
// C-layout tile t of a transposed product (lane = token row 32 t + l31, registers = head-dim columns) times mul, unrounded, -> rows l31 of the fp32 staging tile
__device__ __forceinline__ void wc_stage_f32(unsigned char* st, const f32x16& x, float mul, int l31, int hi) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *(f32x4*)(st + l31 * WC_F32_PITCH + (8 * g + 4 * hi) * 4) = (f32x4){x[4 * g] * mul, x[4 * g + 1] * mul, x[4 * g + 2] * mul, x[4 * g + 3] * mul};
}
// Jacobian of the normalisation on the 32 staged fp32 rows of tile t, then the one rounding: dx = (dn - u (u . dn)) / max(|x|, eps), u = x / max(|x|, eps) in fp32.
// Lane layout of wc_normalize: rows 16 i + (lane >> 2) with i = 2 t + ii, 8 columns per lane.
template <int OF>
__device__ __forceinline__ void wc_flush_jacobian(const unsigned char* st, int t, const u32x4 (&raw)[4], const float (&den)[4], const long (&rr)[4], bf16_t* __restrict__ base,
                                                  long ld, int lane) {
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int i = 2 * t + ii;
    const unsigned char* p = st + (16 * ii + (lane >> 2)) * WC_F32_PITCH + 32 * (lane & 3);
    const f32x4 d0 = *(const f32x4*)p, d1 = *(const f32x4*)(p + 16);
    const float d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
    float x[8], u[8];
    wc_unpack8<OF>(raw[i], x);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { u[e] = x[e] / den[i]; dot = fmaf(u[e], d[e], dot); }
    dot += __shfl_xor(dot, 1);
    dot += __shfl_xor(dot, 2);
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (d[e] - u[e] * dot) / den[i];
    *(u32x4*)(base + rr[i] * ld + 8 * (lane & 3)) = (u32x4){pack_op2<OF>(y[0], y[1]), pack_op2<OF>(y[2], y[3]), pack_op2<OF>(y[4], y[5]), pack_op2<OF>(y[6], y[7])};
  }
}

template <int OF /* operand format of qkv / o: VDK_OPF_BF16 | VDK_OPF_F16 */>
__global__ __launch_bounds__(256) void window_attn_cos_fwd_kernel(const bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ o, long ldo, float* __restrict__ lse,
                                                                  const float* __restrict__ tau, const float* __restrict__ bm, int nWm, long items, int H,
                                                                  const int* __restrict__ rowidx) {
  __shared__ __attribute__((aligned(16))) unsigned char Qt[4][64 * 64];
  __shared__ __attribute__((aligned(16))) unsigned char Kt[4][64 * 64];
  __shared__ __attribute__((aligned(16))) unsigned char Vt[4][64 * 64];
  __shared__ __attribute__((aligned(16))) unsigned char St[4][64 * WA_ST_PITCH];
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int C = H * WA_HD;
  const long item0 = (long)blockIdx.x * 4 + w, istep = (long)gridDim.x * 4;
  long rr_next[4];
  wc_rows(rowidx, (item0 < items ? item0 : 0) / H, lane, rr_next);
  for (long item = item0; item < items; item += istep) {
    const long win = item / H; const int h = (int)(item - win * H);
    const bf16_t* base = qkv + h * WA_HD;
    long rr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rr[i] = rr_next[i];
    VDK_WAVE_LDS_SYNC();                                  // the previous item's LDS readers are done
    wa_dma_rows(Qt[w], base, ld, rr, lane);
    wa_dma_rows(Kt[w], base + C, ld, rr, lane);
    wa_dma_rows(Vt[w], base + 2 * C, ld, rr, lane);
    const float th = tau[h];
    f32x4 bq[2][2][4];                                    // [qt][kt][4 registers each]
    {
      const float* bmp0 = bm + ((win % nWm) * H + h) * WA_FRAG + lane * 16;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int g = 0; g < 4; ++g) bq[qt][kt][g] = *(const f32x4*)(bmp0 + (qt * 2 + kt) * 1024 + 4 * g);
    }
    { const long nx = item + istep; wc_rows(rowidx, (nx < items ? nx : item) / H, lane, rr_next); }
    __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0): the wave's DMAs have landed
    VDK_WAVE_LDS_SYNC();
    {
      u32x4 raw[4]; float den[4];
      wc_normalize<OF>(Qt[w], lane, raw, den);
      wc_normalize<OF>(Kt[w], lane, raw, den);
    }
    VDK_WAVE_LDS_SYNC();
    s16x8 qf[2][2], kf[2][2];
    wa_row_frags(Qt[w], l31, hi, qf);
    wa_row_frags(Kt[w], l31, hi, kf);
    s16x8 pf[2][2][2];                                    // [kt][qt][k-step]
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x16 sa[2];
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        sa[kt] = as_zero16();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) sa[kt] = vdk_mfma32<OF>(kf[kt][ks], qf[qt][ks], sa[kt]);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b = bq[qt][kt][g];
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float a = fmaf(sa[kt][4 * g + e], th, b[e]); sa[kt][4 * g + e] = a; mx = fmaxf(mx, a); }
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float e = fast_exp2((sa[kt][r] - mx) * WA_LOG2E); sa[kt][r] = e; sum += e; }
      sum += __shfl_xor(sum, 32);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[kt][r] *= inv;
        as_pack_b<OF>(sa[kt], pf[kt][qt]);                     // P rounded once, as the operand of P v
      }
      if (lse && hi == 0) lse[(win * H + h) * WC_N + 32 * qt + l31] = mx + logf(sum);
    }
    s16x8 vt[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) vt[kt][s] = wa_tr32(Vt[w], 32 * kt + 16 * s, lane);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x16 oa = as_zero16();
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) oa = vdk_mfma32<OF>(vt[kt][s], pf[kt][qt][s], oa);
      wa_stage_t<OF>(St[w], oa, 1.0f, qt, l31, hi);
    }
    VDK_WAVE_LDS_SYNC();
    wc_flush_rows(St[w], rr, o + h * WA_HD, ldo, lane);
  }
}

// one wave walks the windows win = slot, slot + nslot, ... of ONE head (h = wave index mod H); dbias_part: f32 [waves][WA_FRAG] in fragment order, dtau_part: f32 [waves]
template <int OF>
__global__ __launch_bounds__(64 * WC_BW, 1) void window_attn_cos_bwd_kernel(const bf16_t* __restrict__ qkv, long ld, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
                                                                            long ldo, const float* __restrict__ lse, const float* __restrict__ tau, const float* __restrict__ bm,
                                                                            int nWm, long nwin, int H, bf16_t* __restrict__ dqkv, long ldd, float* __restrict__ dbias_part,
                                                                            float* __restrict__ dtau_part, const int* __restrict__ rowidx) {
  __shared__ __attribute__((aligned(16))) unsigned char Kt[WC_BW][64 * 64];     // k rows, then kn
  __shared__ __attribute__((aligned(16))) unsigned char Qt[WC_BW][64 * 64];     // q rows, then qn
  __shared__ __attribute__((aligned(16))) unsigned char Gt[WC_BW][64 * 64];     // dO rows
  __shared__ __attribute__((aligned(16))) unsigned char Pt[WC_BW][64 * AS_ROW]; // P [q][key], then dS [q][key]
  __shared__ __attribute__((aligned(16))) unsigned char Vt[WC_BW][64 * 64];
  __shared__ __attribute__((aligned(16))) unsigned char St[WC_BW][64 * WA_ST_PITCH];   // output staging: 64 rows of 16-bit dv, or 32 rows of fp32 d(qn) / d(kn)
  __shared__ float Dl[WC_BW][64];                                                     // rowsum(dO * O)
  static_assert(32 * WC_F32_PITCH <= 64 * WA_ST_PITCH, "the fp32 half tile fits the staging tile");
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int C = H * WA_HD;
  const long wid = (long)blockIdx.x * WC_BW + w, nwave = (long)gridDim.x * WC_BW;
  const int h = (int)(wid % H);
  const long slot = wid / H, nslot = nwave / H;            // (the launcher makes the wave count a multiple of H)
  const float th = tau[h];
  f32x16 dB[2][2];                                         // [kt][qt]
#pragma unroll
  for (int a = 0; a < 2; ++a) { dB[a][0] = as_zero16(); dB[a][1] = as_zero16(); }
  float dT = 0.f;                                          // this lane's share of d(tau_h) = sum dS (qn . kn)
  long rr_next[4];
  wc_rows(rowidx, slot < nwin ? slot : 0, lane, rr_next);
  for (long win = slot; win < nwin; win += nslot) {
    const bf16_t* base = qkv + h * WA_HD;
    long rr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rr[i] = rr_next[i];
    VDK_WAVE_LDS_SYNC();                                  // the previous window's readers are done
    wa_dma_rows(Qt[w], base, ld, rr, lane);
    wa_dma_rows(Kt[w], base + C, ld, rr, lane);
    wa_dma_rows(Vt[w], base + 2 * C, ld, rr, lane);
    wa_dma_rows(Gt[w], dout + h * WA_HD, ldo, rr, lane);
    u32x4 orow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) orow[i] = *(const u32x4*)(o + h * WA_HD + rr[i] * ldo + 8 * (lane & 3));
    float l[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) l[qt] = lse[(win * H + h) * WC_N + 32 * qt + l31];
    f32x4 bq[2][2][4];                                    // bias (+ mask) of this (window mod nWm, head) in the C layout: [qt][kt][4 registers each]
    {
      const float* bmp0 = bm + ((win % nWm) * H + h) * WA_FRAG + lane * 16;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int g = 0; g < 4; ++g) bq[qt][kt][g] = *(const f32x4*)(bmp0 + (qt * 2 + kt) * 1024 + 4 * g);
    }
    { const long nx = win + nslot; wc_rows(rowidx, nx < nwin ? nx : win, lane, rr_next); }
    __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0): the wave's DMAs have landed
    VDK_WAVE_LDS_SYNC();
    u32x4 qraw[4], kraw[4]; float qden[4], kden[4];
    wc_normalize<OF>(Qt[w], lane, qraw, qden);
    wc_normalize<OF>(Kt[w], lane, kraw, kden);
#pragma unroll
    for (int i = 0; i < 4; ++i) {                          // D = rowsum(dO * O) on the rounded tensors: 8 products per lane, 4 lanes per row
      const s16x8 gq = *(const s16x8*)(Gt[w] + i * 1024 + lane * 16);
      float d = wa_dot8<OF>(gq, *(const s16x8*)&orow[i]);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      if ((lane & 3) == 0) Dl[w][16 * i + (lane >> 2)] = d;
    }
    VDK_WAVE_LDS_SYNC();
    s16x8 qf[2][2], kf[2][2], vf[2][2], gf[2][2];
    wa_row_frags(Qt[w], l31, hi, qf);
    wa_row_frags(Kt[w], l31, hi, kf);
    wa_row_frags(Vt[w], l31, hi, vf);
    wa_row_frags(Gt[w], l31, hi, gf);
    const float D[2] = {Dl[w][l31], Dl[w][32 + l31]};
    s16x8 dsf[2][2][2];                                   // dS^T as B fragments [kt][qt][k-step]
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x16 sa = as_zero16(), dp = as_zero16();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) sa = vdk_mfma32<OF>(kf[kt][ks], qf[qt][ks], sa);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) dp = vdk_mfma32<OF>(vf[kt][ks], gf[qt][ks], dp);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b = bq[qt][kt][g];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            const float p = fast_exp2((fmaf(sa[r], th, b[e]) - l[qt]) * WA_LOG2E);
            const float ds = p * (dp[r] - D[qt]);          // d(loss)/dS: also the bias gradient of this (query, key)
            dB[kt][qt][r] += ds;
            if (!(WC_AB & 4)) dT = fmaf(ds, sa[r], dT);                      // sa: the cosine qn_i . kn_j
            sa[r] = p; dp[r] = ds;
          }
        }
        s16x8 pfr[2];
        as_pack_b<OF>(sa, pfr);
        wa_put_pt(Pt[w], pfr, kt, qt, l31, hi);
        as_pack_b<OF>(dp, dsf[kt][qt]);
      }
    VDK_WAVE_LDS_SYNC();
    bf16_t* dbase = dqkv + h * WA_HD;
    // d(qn)^T[d][q] = tau sum_key kn^T[d][key] dS^T[key][q], then the Jacobian of q -> qn, one 32-query half at a time through the fp32 staging tile
    {
      s16x8 ktr[2][2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) ktr[kt][s] = wa_tr32(Kt[w], 32 * kt + 16 * s, lane);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x16 acc = as_zero16();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int s = 0; s < 2; ++s) acc = vdk_mfma32<OF>(ktr[kt][s], dsf[kt][qt][s], acc);
        if (WC_AB & 2) { wa_stage_t<OF>(St[w], acc, th, qt, l31, hi); continue; }
        wc_stage_f32(St[w], acc, th, l31, hi);
        VDK_WAVE_LDS_SYNC();
        wc_flush_jacobian<OF>(St[w], qt, qraw, qden, rr, dbase, ldd, lane);
        VDK_WAVE_LDS_SYNC();                               // the half has left the staging tile
      }
      if (WC_AB & 2) { VDK_WAVE_LDS_SYNC(); wc_flush_rows(St[w], rr, dbase, ldd, lane); VDK_WAVE_LDS_SYNC(); }
    }
    // dV^T[d][key] = sum_q dO^T[d][q] P[q][key]
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16 acc = as_zero16();
#pragma unroll
      for (int qs = 0; qs < 4; ++qs)
        acc = vdk_mfma32<OF>(wa_tr32(Gt[w], 16 * qs, lane), as_tr_frag(Pt[w], 16 * qs, 32 * kt, lane), acc);
      wa_stage_t<OF>(St[w], acc, 1.0f, kt, l31, hi);
    }
    VDK_WAVE_LDS_SYNC();                                  // P has been read: the tile takes dS
    wc_flush_rows(St[w], rr, dbase + 2 * C, ldd, lane);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) wa_put_pt(Pt[w], dsf[kt][qt], kt, qt, l31, hi);
    VDK_WAVE_LDS_SYNC();                                  // dS is in place, dV has left the staging tile
    // d(kn)^T[d][key] = tau sum_q qn^T[d][q] dS[q][key], then the Jacobian of k -> kn
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16 acc = as_zero16();
#pragma unroll
      for (int qs = 0; qs < 4; ++qs)
        acc = vdk_mfma32<OF>(wa_tr32(Qt[w], 16 * qs, lane), as_tr_frag(Pt[w], 16 * qs, 32 * kt, lane), acc);
      if (WC_AB & 2) { wa_stage_t<OF>(St[w], acc, th, kt, l31, hi); continue; }
      wc_stage_f32(St[w], acc, th, l31, hi);
      VDK_WAVE_LDS_SYNC();
      wc_flush_jacobian<OF>(St[w], kt, kraw, kden, rr, dbase + C, ldd, lane);
      VDK_WAVE_LDS_SYNC();
    }
    if (WC_AB & 2) { VDK_WAVE_LDS_SYNC(); wc_flush_rows(St[w], rr, dbase + C, ldd, lane); }
  }
  float* dst = dbias_part + wid * WA_FRAG + lane * 16;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int g = 0; g < 4; ++g) *(f32x4*)(dst + (qt * 2 + kt) * 1024 + 4 * g) = (f32x4){dB[kt][qt][4 * g], dB[kt][qt][4 * g + 1], dB[kt][qt][4 * g + 2], dB[kt][qt][4 * g + 3]};
  dT = wave_sum(dT);                                       // a fixed butterfly: the same bits on every run
  if (lane == 0) dtau_part[wid] = dT;
}

extern "C" {

int vdk_reduce_rows_f32(const float*, int64_t, int32_t, int64_t, float*, float, void*);

static bool wc_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static int wc_check(const void* qkv, int64_t ld, int64_t windows, int32_t H, const float* tau, const float* bias, const float* mask, int32_t nW, int32_t opf, const char* who) {
  if (!qkv || !tau || !bias || windows <= 0 || H <= 0 || (ld & 7) || ld < 3 * H * WA_HD || wc_misaligned(qkv)) return vdk_fail(VDK_EINVAL, who);
  if (opf != VDK_OPF_BF16 && opf != VDK_OPF_F16) return vdk_fail(VDK_EUNSUPPORTED, "cosine window attention: operand format 0 (bf16) or 1 (fp16)");
  if (mask && (nW <= 0 || windows % nW)) return vdk_fail(VDK_EINVAL, who);
  return VDK_OK;
}
static size_t wc_bm_bytes(int32_t nW, int32_t H) { return (size_t)(nW > 0 ? nW : 1) * H * WA_FRAG * 4; }
static long wc_bwd_waves(int64_t windows, int32_t H) {
  long waves = 4096 / H * H; if (waves > windows * H) waves = windows * H; if (waves < H) waves = H;
  return (waves + WC_BW * H - 1) / (WC_BW * H) * (WC_BW * H);             // whole workgroups, whole head groups
}
static void wc_prep(const float* bias, const float* mask, int32_t nW, int32_t H, float* bm, hipStream_t st) {
  const int nWm = mask ? nW : 1;
  const long n = (long)nWm * H * WA_FRAG;
  hipLaunchKernelGGL(wc_prep_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bias, mask, nWm, (int)H, bm);
}

/* workspace of vdk_wa_cos_fwd: the bias (+ mask) in the kernel's fragment order, (nW or 1) * H * 16 KB */
int vdk_wa_cos_fwd_workspace_bytes(int32_t nW, int32_t H, size_t* bytes) {
  if (!bytes || nW < 0 || H <= 0) return vdk_fail(VDK_EINVAL, "vdk_wa_cos_fwd_workspace_bytes: bad argument");
  *bytes = wc_bm_bytes(nW, H);
  return VDK_OK;
}
int vdk_wa_cos_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, const float* tau, const float* bias, const float* mask, int32_t nW, int64_t windows, int32_t H,
                   const int32_t* rowidx, int32_t opf, void* ws, size_t ws_bytes, void* stream) {
  int rc = wc_check(qkv, ld, windows, H, tau, bias, mask, nW, opf, "vdk_wa_cos_fwd: bad argument");
  if (rc) return rc;
  if (!o || (ldo & 7) || ldo < H * WA_HD || wc_misaligned(o)) return vdk_fail(VDK_EINVAL, "vdk_wa_cos_fwd: bad argument");
  if (wc_misaligned(ws)) return vdk_fail(VDK_EINVAL, "vdk_wa_cos_fwd: bad argument");          // (the prepared bias is read back 16 bytes at a time)
  if (!ws || ws_bytes < wc_bm_bytes(mask ? nW : 0, H)) return vdk_fail(VDK_EWORKSPACE, "vdk_wa_cos_fwd: workspace too small");
  const long items = (long)windows * H;
  long grid = (items + 3) / 4; if (grid > 4096) grid = 4096;
  hipStream_t st = (hipStream_t)stream;
  wc_prep(bias, mask, nW, H, (float*)ws, st);
  if (opf) hipLaunchKernelGGL(window_attn_cos_fwd_kernel<VDK_OPF_F16>, dim3((unsigned)grid), dim3(256), 0, st, (const bf16_t*)qkv, (long)ld, (bf16_t*)o, (long)ldo, lse, tau,
                              (const float*)ws, mask ? (int)nW : 1, items, (int)H, (const int*)rowidx);
  else hipLaunchKernelGGL(window_attn_cos_fwd_kernel<VDK_OPF_BF16>, dim3((unsigned)grid), dim3(256), 0, st, (const bf16_t*)qkv, (long)ld, (bf16_t*)o, (long)ldo, lse, tau,
                          (const float*)ws, mask ? (int)nW : 1, items, (int)H, (const int*)rowidx);
  return vdk_check_launch("vdk_wa_cos_fwd");
}

/* workspace of vdk_wa_cos_bwd: the prepared bias, one d(bias) partial per wave and their sum (fragment order), one d(tau) partial per wave */
int vdk_wa_cos_bwd_workspace_bytes(int64_t windows, int32_t nW, int32_t H, size_t* bytes) {
  if (!bytes || windows <= 0 || nW < 0 || H <= 0) return vdk_fail(VDK_EINVAL, "vdk_wa_cos_bwd_workspace_bytes: bad argument");
  const long waves = wc_bwd_waves(windows, H);
  *bytes = wc_bm_bytes(nW, H) + (size_t)(waves + H) * WA_FRAG * 4 + (size_t)waves * 4;
  return VDK_OK;
}
int vdk_wa_cos_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, const float* tau, const float* bias, const float* mask, int32_t nW,
                   int64_t windows, int32_t H, const int32_t* rowidx, void* dqkv, int64_t ldd, float* dbias, float* dtau, int32_t opf, void* ws, size_t ws_bytes, void* stream) {
  int rc = wc_check(qkv, ld, windows, H, tau, bias, mask, nW, opf, "vdk_wa_cos_bwd: bad argument");
  if (rc) return rc;
  if (!o || !dout || !lse || !dqkv || !dbias || !dtau || (ldo & 7) || ldo < H * WA_HD || (ldd & 7) || ldd < 3 * H * WA_HD || wc_misaligned(o) || wc_misaligned(dout) ||
      wc_misaligned(dqkv))
    return vdk_fail(VDK_EINVAL, "vdk_wa_cos_bwd: bad argument");
  size_t need = 0; vdk_wa_cos_bwd_workspace_bytes(windows, mask ? nW : 0, H, &need);
  if (wc_misaligned(ws)) return vdk_fail(VDK_EINVAL, "vdk_wa_cos_bwd: bad argument");
  if (!ws || ws_bytes < need) return vdk_fail(VDK_EWORKSPACE, "vdk_wa_cos_bwd: workspace too small");
  const long waves = wc_bwd_waves(windows, H);
  float* bm = (float*)ws;
  float* part = bm + wc_bm_bytes(mask ? nW : 0, H) / 4;
  float* red = part + waves * WA_FRAG;
  float* tpart = red + (size_t)H * WA_FRAG;
  hipStream_t st = (hipStream_t)stream;
  wc_prep(bias, mask, nW, H, bm, st);
  if (opf) hipLaunchKernelGGL(window_attn_cos_bwd_kernel<VDK_OPF_F16>, dim3((unsigned)(waves / WC_BW)), dim3(64 * WC_BW), 0, st, (const bf16_t*)qkv, (long)ld, (const bf16_t*)o,
                              (const bf16_t*)dout, (long)ldo, lse, tau, (const float*)bm, mask ? (int)nW : 1, (long)windows, (int)H, (bf16_t*)dqkv, (long)ldd, part, tpart,
                              (const int*)rowidx);
  else hipLaunchKernelGGL(window_attn_cos_bwd_kernel<VDK_OPF_BF16>, dim3((unsigned)(waves / WC_BW)), dim3(64 * WC_BW), 0, st, (const bf16_t*)qkv, (long)ld, (const bf16_t*)o,
                          (const bf16_t*)dout, (long)ldo, lse, tau, (const float*)bm, mask ? (int)nW : 1, (long)windows, (int)H, (bf16_t*)dqkv, (long)ldd, part, tpart,
                          (const int*)rowidx);
  // partial row r belongs to head r mod H: a group of H consecutive rows IS one [H, 64 x 64] tensor (one [H] vector of d(tau)); the sum over the groups, in group order
  rc = vdk_reduce_rows_f32(part, (int64_t)H * WA_FRAG, (int32_t)(waves / H), (int64_t)H * WA_FRAG, red, 1.0f, stream);
  if (rc) return rc;
  rc = vdk_reduce_rows_f32(tpart, (int64_t)H, (int32_t)(waves / H), (int64_t)H, dtau, 1.0f, stream);
  if (rc) return rc;
  const long n = (long)H * WC_N * WC_N;
  hipLaunchKernelGGL(wc_unprep_dbias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)red, (int)H, dbias);
  return vdk_check_launch("vdk_wa_cos_bwd");
}

}  // extern "C"

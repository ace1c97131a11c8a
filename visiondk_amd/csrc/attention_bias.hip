// attention_bias.hip -- attention with an additive relative position bias over a whole short sequence (BEiT: 197 tokens, head dim 64):
//     o = softmax(scale q k^T + bias[h]) v,   bias f32 [H, N, N] (head, query, key), shared by every batch item;   the backward also returns d(bias) = sum_b dS.
// Served: 1 <= N <= 256, head dim 64, bf16 | fp16 operands.  Tensor layouts, pitches and dtype are those of vdk_attention_fwd_dt / vdk_attention_bwd_dt.
//
// Arithmetic (tests/beit_ref.py restates it; window_attention.hip's convention moved to the sequence kernels):
//   S = fp32(q . k) * scale + bias in fp32 (16-bit q and k, fp32 accumulator); softmax with the exact row maximum in fp32; P rounded ONCE to the operand format as the left
//   operand of P v; o rounded once; lse = log sum exp S in fp32.  Backward: P = exp(S - lse), dP = dO v^T, D = rowsum(dO o) on the stored tensors, dS = P (dP - D) in fp32;
//   d(bias) += dS in fp32 BEFORE dS is rounded to the operand format for the two gradient GEMMs; dq = scale dS k, dk = scale dS^T q, dv = P^T dO, each rounded once.
//   The kernels work in base-2 exponentials: the prepared bias carries the factor log2 e, the logits scale * log2 e.
//
// Structure: attention_small.hip's two kernels (which see for the LDS layout, the swizzle and the staggered dQ exchange) with the bias added in the MFMA C layout.
//   * A prep kernel lays the bias out once per call in the workspace, in the fragment order of the accumulators it is added to, so a lane fetches the 16 values of a
//     (query tile, key tile) block as four 16-byte loads.  The forward holds S^T (lane = query, registers = keys), the backward S (lane = key, registers = queries):
//     two layouts, [H][query tile][key tile][64 lanes][16] and [H][key tile][query tile][64 lanes][16].  The forward's copy holds -inf at keys >= N (that IS the key masking);
//     out-of-range rows / columns otherwise repeat row / column N - 1, as the operand tiles do.
//   * FORWARD: the bias streams through one tile's 16 registers at a time, loaded ahead of that tile's four MFMAs.
//   * BACKWARD, d(bias): scheme (b) of the two deterministic ones.  A workgroup serves the items of ONE head (h = workgroup mod H, batch items slot, slot + nslot, ...) and adds
//     each dS block into a slab of the workspace it owns alone ([key tile][query tile][64 lanes][16] f32, the accumulators' order): every element is touched by exactly one
//     lane per item, so plain load-add-store suffices (the first item stores).  A second kernel sums the slabs of a head in slot order into dbias [H, N, N].  No atomics, a
//     fixed order: the same bits on every run.  Scheme (a) -- the wave's strip of 16 x nqt <= 128 accumulators kept in registers across its items -- needs one wave per SIMD
//     (512 registers); this kernel runs eight waves of 256 registers as its parent does, and its 7-tile instantiation has none to spare.
//     Cost of (b): 16 transient registers; workspace nt^2 x 4 KB per head (prepared bias) + nt^2 x 4 KB per workgroup (slab), nt = ceil(N / 32): at N = 197, H = 12 and 252
//     workgroups 2.4 MB + 50.6 MB; per item 196 KB read (bias) + 196 KB read + 196 KB written (slab) beside the 150 KB of q, k, v, o, dO, dq, dk, dv.
//     The slab traffic shares the vector-memory counter with the raw LDS-DMA requests of the Q / dO ring, so the tile loop waits vmcnt(0) where the parent counts
//     "all but the newest request": a tile's operands travel one tile ahead, not two.
//   * N in 225..256 (eight key tiles): the backward's dQ staging rows have pitch 136 instead of 144 bytes, which brings its LDS to exactly 160 KB.
//
// Resource report of the cross-compiler (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no hardware involved), registers per lane, both operand
// formats within 8 of each other, NO scratch in any instantiation:
//   key tiles (N <=)      1 (32)  2 (64)  3 (96)  4 (128)  5 (160)  6 (192)  7 (224)  8 (256)
//   forward  VGPRs          112     124     152     160      230      242      256      238 + 32 AGPRs
//            waves / SIMD     4       4       3       3        2        2        2        1   (launch bound: two for <= 7 tiles, one for 8)
//   backward VGPRs          124     212     239     231      255      255      248      248
//            waves / SIMD     4       2       2       2        2        2        2        2   (eight waves per workgroup; LDS allows one workgroup per CU from 3 tiles on)
// The backward holds the wave's K / V row fragments in registers for the whole item up to 6 key tiles; with 7 and 8 it re-reads them from its LDS tiles in every key phase
// (with them held the slab update spilled 32 bytes per lane).  LDS: forward 78 KB at N = 197 (two workgroups per CU), 96 KB at 256; backward 145 KB at 7 tiles, 160 KB at 8.
// Measured on one MI355X (tools/beit_record.py attn; B = 256, H = 12, N = 197, fp16, prep and reduction kernels included): forward 112.5 us against 86.7 us of the unbiased
// kernel in the same process (1.30 x, byte-ratio ceiling 2.5), backward 481.4 against 226.8 us (2.12 x, ceiling 3.3).  The register and LDS figures above are the compiler's.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_attn_tile.h"
#include "vdk_internal.h"

#define AB_FRAG 1024                      /* floats per (query tile, key tile) block in fragment order: 64 lanes x 16 */
#define AB_PITCH 72                       /* bytes per key row of the dS exchange (attention_small.hip's A5_PITCH) */

// forward order: element (h, qt, kt, lane, r) <-> query 32 qt + (lane & 31), key 32 kt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5); keys >= N: -inf
// backward order: element (h, kt, qt, lane, r) <-> key 32 kt + (lane & 31), query 32 qt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__global__ __launch_bounds__(256) void ab_prep_bias_kernel(const float* __restrict__ bias, int N, int H, int nt, int bwd, float* __restrict__ bm) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * nt * nt * AB_FRAG) return;
  const int r = (int)(i & 15), lane = (int)((i >> 4) & 63);
  const long blk = i >> 10;
  const int t1 = (int)(blk % nt), t0 = (int)((blk / nt) % nt), h = (int)(blk / ((long)nt * nt));
  const int a = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), c = lane & 31;
  int q = bwd ? 32 * t1 + a : 32 * t0 + c;
  int key = bwd ? 32 * t0 + c : 32 * t1 + a;
  const bool masked = !bwd && key >= N;
  if (q >= N) q = N - 1;
  if (key >= N) key = N - 1;
  bm[i] = masked ? -INFINITY : bias[((long)h * N + q) * N + key] * VDK_LOG2E;
}
// dbias[h][q][key] = sum over the slots s (in order) of the slab of workgroup s * H + h
__global__ __launch_bounds__(256) void ab_reduce_dbias_kernel(const float* __restrict__ part, int N, int H, int nt, int nslot, float* __restrict__ dbias) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * N * N) return;
  const int key = (int)(i % N), q = (int)((i / N) % N), h = (int)(i / ((long)N * N));
  const int qq = q & 31, hi = (qq >> 2) & 1, r = (qq & 3) + 4 * (qq >> 3), lane = (key & 31) + 32 * hi;
  const long slab = (long)nt * nt * AB_FRAG;
  const float* p = part + (long)h * slab + ((long)((key >> 5) * nt + (q >> 5)) * 64 + lane) * 16 + r;
  float t = 0.f;
  for (int s = 0; s < nslot; ++s) t += p[(long)s * H * slab];
  dbias[i] = t;
}

// =====================================================================================  forward
// attn_s_fwd_kernel (attention_small.hip) with the prepared bias bm added to the scaled logits; LDS: Q [R8 rows] | K [R8] | V [R8] | zero rows up to 32 * NKT of V.
template <int NKT, int OF>
__global__ __launch_bounds__(256, (NKT <= 7 ? 2 : 1)) void ab_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                                          bf16_t* __restrict__ o, long ldo, float* __restrict__ lse, const float* __restrict__ bm, int N, int H,
                                                                          float scale, int nitems) {
  VDK_DYN_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R8 = (N + 7) & ~7;
  unsigned char* const Qs = smem;
  unsigned char* const Ks = smem + R8 * AS_ROW;
  unsigned char* const Vs = smem + 2 * R8 * AS_ROW;
  for (int i = tid * 16; i < (32 * NKT - R8) * AS_ROW; i += 256 * 16) *(u32x4*)(Vs + R8 * AS_ROW + i) = (u32x4){0u, 0u, 0u, 0u};
  const int nqt = (N + 31) >> 5;                       // (= NKT: the launcher instantiates NKT = ceil(N / 32))
  const float scale2 = scale * VDK_LOG2E;
  const AsLane al = as_lane(lane);
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / H, h = item - b * H;
    const long off = (long)b * N * ld + h * 64;
    __syncthreads();                                   // the previous item's readers are done (first pass: the zero rows are written)
    as_dma_rows(Qs, q + off, ld, N, R8, w, 4, lane);
    as_dma_rows(Ks, k + off, ld, N, R8, w, 4, lane);
    as_dma_rows(Vs, v + off, ld, N, R8, w, 4, lane);
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): this wave's DMAs have landed
    __syncthreads();
    for (int qt = w; qt < nqt; qt += 4) {
      const int qrow = qt * 32 + l31;
      const float* const bp = bm + ((long)(h * NKT + qt) * NKT) * AB_FRAG + lane * 16;
      s16x8 qf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[ks] = as_row_frag(Qs, qrow, ks, hi);
      f32x16 st[NKT];
      float m = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 bb[4];                                   // this tile's bias: requested ahead of its MFMAs, 16 registers at a time
#pragma unroll
        for (int g = 0; g < 4; ++g) bb[g] = *(const f32x4*)(bp + kt * AB_FRAG + 4 * g);
        st[kt] = as_zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) st[kt] = vdk_mfma32<OF>(as_row_frag_l(Ks + kt * 32 * AS_ROW, al, ks), qf[ks], st[kt]);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float a = fmaf(st[kt][4 * g + e], scale2, bb[g][e]); st[kt][4 * g + e] = a; m = fmaxf(m, a); }      // keys >= N: -inf
      }
      m = fmaxf(m, __shfl_xor(m, 32));                 // the two half-waves hold the same queries, different keys
      float l = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float p = fast_exp2(st[kt][r] - m); st[kt][r] = p; l += p; }
      l += __shfl_xor(l, 32);
      const float inv = 1.0f / l;
      f32x16 o0 = as_zero16(), o1 = as_zero16();
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x16 pn;
#pragma unroll
        for (int r = 0; r < 16; ++r) pn[r] = st[kt][r] * inv;
        s16x8 pf[2];
        as_pack_b<OF>(pn, pf);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          o0 = vdk_mfma32<OF>(as_tr_frag_l(Vs + (kt * 32 + 16 * s) * AS_ROW, al, 0), pf[s], o0);
          o1 = vdk_mfma32<OF>(as_tr_frag_l(Vs + (kt * 32 + 16 * s) * AS_ROW, al, 1), pf[s], o1);
        }
      }
      as_store_tile<OF>(Qs + qt * 32 * AS_ROW, o0, o1, 1.0f, o + (long)b * N * ldo + h * 64, ldo, qt * 32, N, lane);
      if (lse && hi == 0 && qrow < N) lse[((long)b * H + h) * N + qrow] = (m + log2f(l)) * 0.6931471805599453f;
    }
  }
}

// =====================================================================================  backward
// attn_s_bwd5_kernel (attention_small.hip: a wave owns a key tile and walks the query tiles; dS is exchanged through LDS, the dQ_j^T tile is split by output block) with the
// bias inside the exponent and the wave's dS blocks added into the workgroup's slab.  Workgroup g serves head g mod H, batch items g / H, g / H + nslot, ...
// LDS: 24 KB (Q_j, dO_j x 3) + 2 x NKT x 4 KB (K, V tiles) + 2 x NP x 72 (dS) + NP x QP (dQ rows) + NP x 8 (lse, D), NP = 32 NKT: 145 KB at NKT = 7, 160 KB at NKT = 8.
template <int NKT, int OF>
__global__ __launch_bounds__(512) void ab_bwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                     const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse,
                                                     const float* __restrict__ bm, bf16_t* __restrict__ dq, bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, long ldd,
                                                     float* __restrict__ part, int B, int N, int H, float scale, int nslot) {
  VDK_DYN_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NP = 32 * NKT;
  constexpr int NPC = (NP * 8 + 511) / 512;
  constexpr int DSB = NP * AB_PITCH;                                  // one dS buffer
  constexpr int QP = NKT == 8 ? 136 : 144;                            // bytes per query row of the dQ staging: 64 d x 2 B + 16 (+ 8 where 160 KB would not hold the 16)
  unsigned char* const QO = smem;                                     // [buffer 3][Q | dO][32 rows x 128 B]
  unsigned char* const Kall = smem + 3 * 8192;                        // [NKT][4 KB] K tiles
  unsigned char* const Kt = Kall + w * 4096;
  unsigned char* const Vt = Kall + NKT * 4096 + w * 4096;             // [NKT][4 KB] V tiles
  unsigned char* const Ds = Kall + 2 * NKT * 4096;                    // [2][NP rows x AB_PITCH] dS [key][query]; behind an item's last barrier: the waves' 4 KB store tiles
  unsigned char* const DQs = Ds + 2 * DSB;                            // [NP rows x QP] dQ [query][d], 16-bit, already scaled
  float* const lse2 = (float*)(DQs + NP * QP);
  float* const Dv = lse2 + NP;
  constexpr int nt = NKT;
  constexpr bool KVREG = NKT <= 6;                                    // (with 7 and 8 key tiles the 32 registers of the held fragments are what the slab update needs: scratch otherwise)
  const float scale2 = scale * VDK_LOG2E;
  const bool ragged = (N & 31) != 0;
  const AsLane al = as_lane(lane);
  const bool keyw = w < nt;                                           // (wave-uniform)
  const int h = (int)blockIdx.x % H, slot = (int)blockIdx.x / H;
  const float* const bmw = bm + ((long)(h * NKT + w) * NKT) * AB_FRAG + lane * 16;                      // this wave's strip of the prepared bias (keyw)
  float* const partw = part + ((long)((long)blockIdx.x * NKT + w) * NKT) * AB_FRAG + lane * 16;         // ... and of the workgroup's d(bias) slab
  const int db = w >> 1, qb = w & 1;
  const int a16 = lane & 15, g4 = lane >> 4;
  const int trow = 8 * g4 + (a16 >> 2);                               // key row inside a 32-key step
  const int ds_off = trow * AB_PITCH + qb * 32 + 8 * (a16 & 3);
  int kt_off[2];
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    const int r = trow + 4 * h2, byte = 32 * db + 8 * (a16 & 3);
    kt_off[h2] = r * AS_ROW + (((byte >> 4) ^ as_f(r)) << 4) + (byte & 8);
  }
  auto request_tile = [&](int j, int buf, long off, long offo, int lane_) {
    const int q0 = j * 32, pt = w & 3;
    if (w < 4) as_dma_rows_raw(QO + buf * 8192, q + off + (long)q0 * ld, ld, N - q0, 32, pt, 4, lane_);
    else as_dma_rows_raw(QO + buf * 8192 + 4096, dout + offo + (long)q0 * ldo, ldo, N - q0, 32, pt, 4, lane_);
  };
  auto request_item = [&](long off, long offo, int lane_) {
    request_tile(0, 0, off, offo, lane_);
    if (nt > 1) request_tile(1, 1, off, offo, lane_);
    if (keyw) {
      as_dma_rows_raw(Kt, k + off + (long)(w * 32) * ld, ld, N - w * 32, 32, 0, 1, lane_);
      as_dma_rows_raw(Vt, v + off + (long)(w * 32) * ld, ld, N - w * 32, 32, 0, 1, lane_);
    }
  };
  // D = rowsum(dO * O) on the rounded tensors, straight from global memory: 8 lanes per row
  u32x4 d_a[NPC], d_c[NPC];
  float lse_r = 0.f;
  auto d_issue = [&](long offo, long lrow, int tid_) {
#pragma unroll
    for (int p = 0; p < NPC; ++p) {
      const int id = tid_ + 512 * p, row = id >> 3, cp = id & 7;
      d_a[p] = (u32x4){0u, 0u, 0u, 0u}; d_c[p] = (u32x4){0u, 0u, 0u, 0u};
      if (row < N) { d_a[p] = *(const u32x4*)(dout + offo + (long)row * ldo + cp * 8); d_c[p] = *(const u32x4*)(o + offo + (long)row * ldo + cp * 8); }
    }
    lse_r = tid_ < N ? lse[lrow + tid_] : 0.f;                        // (NP <= 256 < 512 threads)
  };
  auto d_finish = [&]() {
#pragma unroll
    for (int p = 0; p < NPC; ++p) {
      const int id = tid + 512 * p, row = id >> 3, cp = id & 7;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { d = fmaf(op_lo<OF>(d_a[p][e]), op_lo<OF>(d_c[p][e]), d); d = fmaf(op_hi<OF>(d_a[p][e]), op_hi<OF>(d_c[p][e]), d); }
      d += __shfl_xor(d, 1); d += __shfl_xor(d, 2); d += __shfl_xor(d, 4);
      if (row < NP && cp == 0) Dv[row] = row < N ? d : 0.f;
    }
    if (tid < NP) lse2[tid] = lse_r * VDK_LOG2E;
  };
  unsigned char* const St = Ds + w * 4096;                            // this wave's 4 KB store tile at the end of an item
  bool first = true;                                                  // the workgroup's first item stores its dS blocks into the slab, the later ones add
  if (slot < B) {
    request_item((long)slot * N * ld + h * 64, (long)slot * N * ldo + h * 64, lane);
    d_issue((long)slot * N * ldo + h * 64, ((long)slot * H + h) * N, tid);
  }
  for (int b = slot; b < B; b += nslot) {
    const long off = (long)b * N * ld + h * 64, offo = (long)b * N * ldo + h * 64;
    d_finish();                                                       // this item's D and lse rows (requested with the item)
    f32x16 gk0 = as_zero16(), gk1 = as_zero16(), gv0 = as_zero16(), gv1 = as_zero16();
    __builtin_amdgcn_s_waitcnt(0x0F70);                               // vmcnt(0): this item's requests (and the previous item's stores)
    __syncthreads();
    s16x8 kfr[4], vfr[4];                                             // the wave's K / V row fragments: held for the whole item (KVREG) or re-read in every key phase
    if (keyw && KVREG) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) { kfr[ks] = as_row_frag_l(Kt, al, ks); vfr[ks] = as_row_frag_l(Vt, al, ks); }
    }
    auto key_phase = [&](int j) {
      const int q0 = j * 32, buf = j % 3, dbuf = j & 1;
      const unsigned char* Qs = QO + buf * 8192;
      const unsigned char* Os = Qs + 4096;
      unsigned char* const Dsj = Ds + dbuf * DSB;
      f32x4 bb[4];                                                    // bias block (key tile w, query tile j): requested ahead of the tile's MFMAs
      if (keyw) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bb[g] = *(const f32x4*)(bmw + j * AB_FRAG + 4 * g);
      }
      if (j + 2 < nt) request_tile(j + 2, (j + 2) % 3, off, offo, lane);    // (that buffer held tile j - 1: its readers passed the barrier that closed tile j - 1)
      if (keyw) {
        f32x16 st = as_zero16(), dp = as_zero16();
        f32x16 pv, ds;
        s16x8 pf[2], df[2];
        const bool edge = ragged && j == nt - 1;                      // rows of the last query tile beyond N (the DMA filled them with row N - 1): silenced
#define AB_SB() __builtin_amdgcn_sched_barrier(0)
#ifdef VDK_EMU
#define AB_PIN(x) ((void)0)
#else
#define AB_PIN(x) asm volatile("" : "+v"(x))
#endif
        s16x8 qf[4], of_[4], kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { qf[ks] = as_row_frag_l(Qs, al, ks); kf[ks] = KVREG ? kfr[ks] : as_row_frag_l(Kt, al, ks); }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) st = vdk_mfma32<OF>(qf[ks], kf[ks], st);                  // S[q][key]: lane = key, registers = queries
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { of_[ks] = as_row_frag_l(Os, al, ks); vf[ks] = KVREG ? vfr[ks] : as_row_frag_l(Vt, al, ks); }
        AB_SB();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          dp = vdk_mfma32<OF>(of_[g], vf[g], dp);                                                // dP[q][key]
          const f32x4 lv = *(const f32x4*)(lse2 + q0 + 8 * g + 4 * hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) pv[4 * g + e] = fast_exp2(fmaf(st[4 * g + e], scale2, bb[g][e]) - lv[e]);
          AB_SB();
        }
        if (edge) {                                                   // (wave-uniform)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (q0 + 8 * (r >> 2) + 4 * hi + (r & 3) >= N) pv[r] = 0.f;
        }
        as_pack_b<OF>(pv, pf);
        AB_SB();
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dh = 0; dh < 2; ++dh) {
            const s16x8 tf = as_tr_frag_l(Os + 16 * s2 * AS_ROW, al, dh);
            if (dh == 0) gv0 = vdk_mfma32<OF>(tf, pf[s2], gv0); else gv1 = vdk_mfma32<OF>(tf, pf[s2], gv1);      // dV^T[d][key] += dO^T P
            const int g = 2 * s2 + dh;
            const f32x4 dd = *(const f32x4*)(Dv + q0 + 8 * g + 4 * hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) { ds[4 * g + e] = pv[4 * g + e] * (dp[4 * g + e] - dd[e]); AB_PIN(ds[4 * g + e]); }
            AB_SB();
          }
        // d(bias): the fp32 dS block into the workgroup's slab, before its rounding (lanes of keys >= N and rows of queries >= N hold values nobody reads)
        float* const pp = partw + j * AB_FRAG;
        if (first) {                                                  // (wave-uniform)
#pragma unroll
          for (int g = 0; g < 4; ++g) *(f32x4*)(pp + 4 * g) = (f32x4){ds[4 * g], ds[4 * g + 1], ds[4 * g + 2], ds[4 * g + 3]};
        } else {
          f32x4 acc[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = *(const f32x4*)(pp + 4 * g);
#pragma unroll
          for (int g = 0; g < 4; ++g) *(f32x4*)(pp + 4 * g) = (f32x4){acc[g][0] + ds[4 * g], acc[g][1] + ds[4 * g + 1], acc[g][2] + ds[4 * g + 2], acc[g][3] + ds[4 * g + 3]};
        }
        as_pack_b<OF>(ds, df);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          gk0 = vdk_mfma32<OF>(as_tr_frag_l(Qs + 16 * s2 * AS_ROW, al, 0), df[s2], gk0);     // dK^T[d][key] += Q^T dS
          gk1 = vdk_mfma32<OF>(as_tr_frag_l(Qs + 16 * s2 * AS_ROW, al, 1), df[s2], gk1);
        }
#undef AB_SB
#undef AB_PIN
        // dS [q][key] (lane = key, registers = queries) -> the exchange buffer as [key][q] rows.  Lanes of keys beyond N hold dS of a duplicated key row: zero.
        const bool kval = w * 32 + l31 < N;
        unsigned char* const drow = Dsj + (w * 32 + l31) * AB_PITCH + 8 * hi;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          u32x4 u = *(const u32x4*)&df[s2];
          if (!kval) u = (u32x4){0u, 0u, 0u, 0u};
          *(u32x2*)(drow + 32 * s2) = (u32x2){u[0], u[1]};           // queries 16 s2 + 4 hi + 0..3
          *(u32x2*)(drow + 32 * s2 + 16) = (u32x2){u[2], u[3]};      // queries 16 s2 + 8 + 4 hi + 0..3
        }
      }
    };
    auto dq_phase = [&](int j) {
      const int q0 = j * 32, dbuf = j & 1;
      unsigned char* const Dsj = Ds + dbuf * DSB;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const unsigned char* bp = Dsj + t * 32 * AB_PITCH + ds_off;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(bp));
        const s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(bp + 4 * AB_PITCH));
        const s16x8 bfrag = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
        const s16x4 klo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(Kall + t * 4096 + kt_off[0]));
        const s16x4 kup = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(Kall + t * 4096 + kt_off[1]));
        acc = vdk_mfma16<OF>((s16x8){klo[0], klo[1], klo[2], klo[3], kup[0], kup[1], kup[2], kup[3]}, bfrag, acc);
      }
      *(u32x2*)(DQs + (q0 + 16 * qb + a16) * QP + 32 * db + 8 * g4) = (u32x2){pack_op2<OF>(acc[0] * scale, acc[1] * scale), pack_op2<OF>(acc[2] * scale, acc[3] * scale)};
    };
    key_phase(0);
#pragma unroll 1
    for (int j = 0; j < nt; ++j) {
      // tile j + 1 must have landed before the barrier publishes it.  The slab's loads and stores share the counter with the ring's requests and return in no fixed order
      // relative to them, so nothing is counted here: everything this wave has in flight.
      __builtin_amdgcn_s_waitcnt(0x0F70);                             // vmcnt(0)
      __syncthreads();                                                // tile j's dS complete, tile j + 1's operands in place
      const bool keyfirst = w < 4;                                    // (wave-uniform)
      if (keyfirst && j + 1 < nt) key_phase(j + 1);
      dq_phase(j);
      if (!keyfirst && j + 1 < nt) key_phase(j + 1);
    }
    __syncthreads();                                                  // every dQ block is staged; the last tile's dQ phase is done with the K tiles and the dS buffers
    first = false;
    int ln = lane, td = tid;
#ifndef VDK_EMU
    asm volatile("" : "+v"(ln), "+v"(td));                           // (laundered: see attention_small.hip's request_item)
#endif
    const int lane = ln, tid = td;                                    // (shadow the kernel-wide copies for the rest of the item)
    if (b + nslot < B) {
      const int nb = b + nslot;
      request_item((long)nb * N * ld + h * 64, (long)nb * N * ldo + h * 64, lane);
      d_issue((long)nb * N * ldo + h * 64, ((long)nb * H + h) * N, tid);
    }
    if (keyw) {
      as_store_tile<OF>(St, gk0, gk1, scale, dk + (long)b * N * ldd + h * 64, ldd, w * 32, N, lane);
      as_store_tile<OF>(St, gv0, gv1, 1.0f, dv + (long)b * N * ldd + h * 64, ldd, w * 32, N, lane);
    }
    // dQ rows leave as whole 128-byte rows: 8 threads per row (two 8-byte LDS reads per thread: the rows of pitch 136 are 8-byte aligned)
#pragma unroll
    for (int p = 0; p < NPC; ++p) {
      const int id = tid + 512 * p, row = id >> 3, cp = id & 7;
      if (row < N) {
        const u32x2 x0 = *(const u32x2*)(DQs + row * QP + cp * 16), x1 = *(const u32x2*)(DQs + row * QP + cp * 16 + 8);
        *(u32x4*)(dq + (long)b * N * ldd + h * 64 + (long)row * ldd + cp * 8) = (u32x4){x0[0], x0[1], x1[0], x1[1]};
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
template <int NKT, int OF>
static int ab_launch_fwd(const bf16_t* base, long D, long ld, bf16_t* o, long ldo, float* lse, const float* bm, int B, int N, int H, float scale, int grid, hipStream_t s) {
  const int R8 = (N + 7) & ~7;
  const size_t lds = (size_t)(2 * R8 + 32 * NKT) * AS_ROW;
  if (hipFuncSetAttribute((const void*)ab_fwd_kernel<NKT, OF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return vdk_fail(VDK_ELAUNCH, "vdk_attention_bias_fwd: LDS attribute");
  hipLaunchKernelGGL((ab_fwd_kernel<NKT, OF>), dim3((unsigned)grid), dim3(256), lds, s, base, base + D, base + 2 * D, ld, o, ldo, lse, bm, N, H, scale, B * H);
  return VDK_OK;
}
template <int NKT, int OF>
static int ab_launch_bwd(const bf16_t* base, long D, long ld, const bf16_t* o, const bf16_t* dout, long ldo, const float* lse, const float* bm, bf16_t* dbase, long ldd,
                         float* part, int B, int N, int H, float scale, int nslot, hipStream_t s) {
  const size_t lds = 3 * 8192 + 2 * (size_t)NKT * 4096 + 2 * (size_t)(32 * NKT) * AB_PITCH + (size_t)(32 * NKT) * (NKT == 8 ? 136 : 144) + (size_t)NKT * 32 * 8;
  if (hipFuncSetAttribute((const void*)ab_bwd_kernel<NKT, OF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return vdk_fail(VDK_ELAUNCH, "vdk_attention_bias_bwd: LDS attribute");
  hipLaunchKernelGGL((ab_bwd_kernel<NKT, OF>), dim3((unsigned)(nslot * H)), dim3(512), lds, s, base, base + D, base + 2 * D, ld, o, dout, ldo, lse, bm, dbase, dbase + D,
                     dbase + 2 * D, ldd, part, B, N, H, scale, nslot);
  return VDK_OK;
}
static int ab_grid_cap(int dflt) {
  if (const char* e = getenv("VDK_ATTN_GRID")) { const int v = atoi(e); if (v > 0) return v; }   // tests: force several items per workgroup
  return dflt;
}
static int ab_nslot(int B, int H) {      // workgroups per head of the backward: every workgroup has at least one item
  int n = ab_grid_cap(256) / H;
  if (n < 1) n = 1;
  return n < B ? n : B;
}
static bool ab_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static size_t ab_bm_bytes(int N, int H) { const size_t nt = (size_t)(N + 31) / 32; return (size_t)H * nt * nt * AB_FRAG * 4; }
static void ab_prep(const float* bias, int N, int H, int bwd, float* bm, hipStream_t st) {
  const int nt = (N + 31) / 32;
  const long n = (long)H * nt * nt * AB_FRAG;
  hipLaunchKernelGGL(ab_prep_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bias, N, H, nt, bwd, bm);
}

extern "C" {

/* workspace of vdk_attention_bias_fwd: the bias in the forward's fragment order, H * ceil(N / 32)^2 * 4 KB */
int vdk_attention_bias_fwd_workspace_bytes(int32_t N, int32_t H, size_t* bytes) {
  if (!bytes || N <= 0 || H <= 0) return vdk_fail(VDK_EINVAL, "vdk_attention_bias_fwd_workspace_bytes: bad argument");
  if (N > 256) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attention_bias_fwd_workspace_bytes: 1 <= N <= 256");
  *bytes = ab_bm_bytes(N, H);
  return VDK_OK;
}
int vdk_attention_bias_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, const float* bias, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale,
                           int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!qkv || !o || !bias || B <= 0 || N <= 0 || H <= 0 || (dtype != VDK_BF16 && dtype != VDK_F16)) return vdk_fail(VDK_EINVAL, "vdk_attention_bias_fwd: bad argument");
  if (head_dim != 64) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attention_bias_fwd: head_dim must be 64");
  if (N > 256) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attention_bias_fwd: 1 <= N <= 256");
  if ((ld & 7) || (ldo & 7) || ld < 3 * (int64_t)H * 64 || ldo < (int64_t)H * 64) return vdk_fail(VDK_EINVAL, "vdk_attention_bias_fwd: pitches: multiples of 8, ld >= 3 H 64, ldo >= H 64");
  if (ab_misaligned(qkv) || ab_misaligned(o) || ab_misaligned(ws) || ((uintptr_t)bias & 3) || ((uintptr_t)lse & 3))
    return vdk_fail(VDK_EINVAL, "vdk_attention_bias_fwd: misaligned pointer");
  if (!ws || ws_bytes < ab_bm_bytes(N, H)) return vdk_fail(VDK_EWORKSPACE, "vdk_attention_bias_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ab_prep(bias, N, H, 0, (float*)ws, s);
  const bf16_t* base = (const bf16_t*)qkv;
  const long D = (long)H * 64;
  int grid = B * H;
  const int cap = ab_grid_cap(512);
  if (grid > cap) grid = cap;
  int rc = VDK_OK;
  switch ((N + 31) / 32) {
#define FW(n) case n: rc = dtype == VDK_F16 ? ab_launch_fwd<n, VDK_OPF_F16>(base, D, ld, (bf16_t*)o, ldo, lse, (const float*)ws, B, N, H, scale, grid, s) \
                                            : ab_launch_fwd<n, 0>(base, D, ld, (bf16_t*)o, ldo, lse, (const float*)ws, B, N, H, scale, grid, s); break;
    FW(1) FW(2) FW(3) FW(4) FW(5) FW(6) FW(7) FW(8)
#undef FW
  }
  return rc ? rc : vdk_check_launch("vdk_attention_bias_fwd");
}

/* workspace of vdk_attention_bias_bwd: the bias in the backward's fragment order and one d(bias) slab per workgroup (nslot * H workgroups, nslot = min(B, 256 / H)) */
int vdk_attention_bias_bwd_workspace_bytes(int32_t B, int32_t N, int32_t H, size_t* bytes) {
  if (!bytes || B <= 0 || N <= 0 || H <= 0) return vdk_fail(VDK_EINVAL, "vdk_attention_bias_bwd_workspace_bytes: bad argument");
  if (N > 256) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attention_bias_bwd_workspace_bytes: 1 <= N <= 256");
  *bytes = ab_bm_bytes(N, H) * (size_t)(1 + ab_nslot(B, H));
  return VDK_OK;
}
int vdk_attention_bias_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, const float* bias, void* dqkv, int64_t lddqkv,
                           float* dbias, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!qkv || !o || !dout || !lse || !bias || !dqkv || !dbias || B <= 0 || N <= 0 || H <= 0 || (dtype != VDK_BF16 && dtype != VDK_F16))
    return vdk_fail(VDK_EINVAL, "vdk_attention_bias_bwd: bad argument");
  if (head_dim != 64) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attention_bias_bwd: head_dim must be 64");
  if (N > 256) return vdk_fail(VDK_EUNSUPPORTED, "vdk_attention_bias_bwd: 1 <= N <= 256");
  if ((ld & 7) || (ldo & 7) || (lddqkv & 7) || ld < 3 * (int64_t)H * 64 || ldo < (int64_t)H * 64 || lddqkv < 3 * (int64_t)H * 64)
    return vdk_fail(VDK_EINVAL, "vdk_attention_bias_bwd: pitches: multiples of 8, ld and lddqkv >= 3 H 64, ldo >= H 64");
  if (ab_misaligned(qkv) || ab_misaligned(o) || ab_misaligned(dout) || ab_misaligned(dqkv) || ab_misaligned(ws) || ((uintptr_t)bias & 3) || ((uintptr_t)lse & 3) ||
      ((uintptr_t)dbias & 3))
    return vdk_fail(VDK_EINVAL, "vdk_attention_bias_bwd: misaligned pointer");
  const int nslot = ab_nslot(B, H);
  const size_t bmb = ab_bm_bytes(N, H);
  if (!ws || ws_bytes < bmb * (size_t)(1 + nslot)) return vdk_fail(VDK_EWORKSPACE, "vdk_attention_bias_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* const bm = (float*)ws;
  float* const part = bm + bmb / 4;
  ab_prep(bias, N, H, 1, bm, s);
  const bf16_t* base = (const bf16_t*)qkv;
  const long D = (long)H * 64;
  int rc = VDK_OK;
  switch ((N + 31) / 32) {
#define BW(n) case n: rc = dtype == VDK_F16 ? ab_launch_bwd<n, VDK_OPF_F16>(base, D, ld, (const bf16_t*)o, (const bf16_t*)dout, ldo, lse, bm, (bf16_t*)dqkv, lddqkv, part, B, N, \
                                                                             H, scale, nslot, s)                                                                              \
                                            : ab_launch_bwd<n, 0>(base, D, ld, (const bf16_t*)o, (const bf16_t*)dout, ldo, lse, bm, (bf16_t*)dqkv, lddqkv, part, B, N, H, scale, \
                                                                  nslot, s); break;
    BW(1) BW(2) BW(3) BW(4) BW(5) BW(6) BW(7) BW(8)
#undef BW
  }
  if (rc) return rc;
  const long n = (long)H * N * N;
  hipLaunchKernelGGL(ab_reduce_dbias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)part, (int)N, (int)H, (N + 31) / 32, nslot, dbias);
  return vdk_check_launch("vdk_attention_bias_bwd");
}

}  // extern "C"

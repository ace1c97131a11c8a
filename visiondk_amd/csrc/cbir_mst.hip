// cbir_mst.hip — one Boruvka round of the minimum spanning tree of the cosine MUTUAL-REACHABILITY graph (HDBSCAN, the alternative the reference's tools/clustering.py
// names beside its DBSCAN call).  The N x N matrix is never formed: a round is a ROW SCAN that leaves, for every row i, the smallest edge to another component.
//
// Arithmetic contract (DESIGN.md section 3 "HDBSCAN"; rows xn = the library's L2 normalisation; everything fp32, one bit pattern per input):
//   s_ij = the exact score, the k-ordered fmaf chain from +0 (cbir_exact_ip; symmetric in i, j: every product commutes and the order of the sum is that of k);
//   d_ij = max(0, 1.0f - s_ij);   w_ij = max(core_i, core_j, d_ij), i != j;   edges are ordered by the strict, total key (w, min(i, j), max(i, j)).
// For a fixed row i that key orders its partners by (w_ij, j), so "smallest key of row i" = smallest w, then smallest j.
//
// Structure = the range search's (cbir_range.hip): the bf16 MFMA only PROPOSES, the exact chain DECIDES, and what the scan writes has a size known beforehand.
//   1 bound    s' = bf16-MFMA score of every pair; per pair in another component  ub_ij = max(core_i, core_j, 1 - down(s' - e_i))  >= w_ij, and the row minimum U_i of ub
//              over a fixed-owner slice of the columns (a wave owns its queries through its slice: registers, one store), then a reduce over the slices.  No atomics.
//   2 propose  the same scan again: bit (i, j) set iff j is in another component and  lb_ij = max(core_i, core_j, 1 - up(s' + e_i))  <= U_i.  One bit per pair, every word
//              written.
//   3 decide   a thread per (row, chunk of 64 words = 2048 columns) gives every proposed pair its exact chain score, forms w_ij and keeps the smallest (w, j); a per-row
//              reduce over the chunks leaves best_w[i], best_j[i].
//
// Why nothing is lost, rounding included.  e_i = cbir_eps bounds |s - s'| for every partner of row i (the measured rounding-error norms of row i and of the gallery, as in
// the searches).  fl() is monotone, down(x) / up(x) step one float below / above x, so
//     down(fl(s' - e_i)) <= s' - e_i <= s   =>   fl(1 - down(..)) >= fl(1 - s)   =>   ub_ij >= w_ij      (max with 0 and with the cores is monotone too),
//     up(fl(s' + e_i))   >= s' + e_i >= s   =>   fl(1 - up(..))   <= fl(1 - s)   =>   lb_ij <= w_ij.
// Let j* hold the smallest key of row i.  U_i = min_j ub_ij >= min_j w_ij = w_ij*, and every j with w_ij = w_ij* has lb_ij <= w_ij* <= U_i: it is proposed, so the decide
// pass sees every holder of the minimum and the index tie-break is taken on exact values only.  The comparison is written !(lb > U): a NaN proposes.
// The bits of best_w / best_j do not depend on the MFMA's summation order, on the split of the columns or on the order of the chunks: they are a minimum of exact keys.
//
// Both scans form the bounds only where a lane holds a pair near its row's bound; the others are dismissed with one add and one compare (ms_fast below, with its argument).
//
// Rows beyond N of the last 32-row tile: their core is +inf in the padded copy (never a minimum) and their bits are masked out of every word.
#include <hip/hip_runtime.h>
#include <cmath>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_internal.h"
#include "cbir_device.h"

#define MS_NBUF 3        // LDS-DMA ring depth (as cbir_range.hip)
#define MS_CHUNK 64      // 32-column mask words per (row, chunk) thread of the decide kernel: 2048 columns
#define MS_BATCH 16      // mask words a thread loads before it looks at any of them
#define MS_INF __uint_as_float(0x7f800000u)

typedef int ms_i32x4 __attribute__((ext_vector_type(4)));

// one float below / above x (x finite; NaN stays NaN)
__device__ __forceinline__ float ms_down(float x) {
  unsigned u = __float_as_uint(x);
  if (x > 0.f) u -= 1u; else if (x < 0.f) u += 1u; else if (x == 0.f) u = 0x80000001u;
  return __uint_as_float(u);
}
__device__ __forceinline__ float ms_up(float x) {
  unsigned u = __float_as_uint(x);
  if (x > 0.f) u += 1u; else if (x < 0.f) u -= 1u; else if (x == 0.f) u = 0x00000001u;
  return __uint_as_float(u);
}

// MS_FAST: the cut of the scan's fast path for a row whose bound is u (U_i, or the running minimum of ub).  With t = ms_fast(u) = fl(fl(1 - u) - 2e-6) for u <= 4 (the two
// roundings move it by at most 4.8e-7, so t <= 1 - u - 1.5e-6):
//   bound:    a = fl(s' - e) <= t  =>  down(a) < 1 - u - 1.5e-6  =>  fl(1 - down(a)) >= fl(u + 1.5e-6) > u  (ulp(4) = 4.8e-7)  =>  ub > u: the minimum does not move;
//   propose:  b = fl(s' + e) <  t  =>  up(b) <= t                =>  fl(1 - up(b)) > u the same way                          =>  lb > u: the pair is not proposed.
// Everything else, a NaN included on the propose side, takes the path that forms the bounds.  u > 4 or NaN (cores the caller made up): t = -inf, no fast path.
__device__ __forceinline__ float ms_fast(float u) { return u <= 4.0f ? (1.0f - u) - 2e-6f : -MS_INF; }

// ------------------------------------------------------------------------------------ 0 pack
// corep / compp: core and comp padded to whole 32-row tiles (+inf / -1 behind row N - 1), so that the scan loads a tile's 32 values as aligned vectors
__global__ __launch_bounds__(256) void mst_pack_kernel(const float* __restrict__ core, const int* __restrict__ comp, long N, long NP, float* __restrict__ corep,
                                                       int* __restrict__ compp) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= NP) return;
  corep[j] = j < N ? core[j] : MS_INF;
  compp[j] = j < N ? comp[j] : -1;
}

// ------------------------------------------------------------------------------------ 1 bound / 2 propose
// The scan of cbir_range_filter_kernel (ring of 32-row bf16 tiles by LDS-DMA, the bf16 fragments of QT 32-query tiles per wave in registers, 8 waves = 256 QT queries per
// workgroup; grid id -> split = id % nsplit, qblock = id / nsplit) with the rows of the block, q0 .. q0 + nq - 1 of the SAME matrix, as its queries: their bf16 copy and
// norms are rows of Gb / gnorm.  PROPOSE = 0: Upart[split * nqp + q] = min over the slice of ub.  PROPOSE = 1: mask[b * nqp + q] for every 32-row block b of the slice.
template <int NK, int QT, int PROPOSE>
__global__ __launch_bounds__(512) void mst_scan_kernel(const bf16_t* __restrict__ Gb, const float* __restrict__ gnorm, const unsigned* __restrict__ gmax_bits,
                                                       const float* __restrict__ corep, const int* __restrict__ compp, long N, long q0, long nq, long nqp, long rows_per_split,
                                                       int nsplit, const float* __restrict__ U, float* __restrict__ Upart, unsigned* __restrict__ mask) {
  constexpr int RB = NK * 32;           // bytes per bf16 row
  constexpr int CH = RB / 16;           // 16-byte chunks per row
  constexpr int TILEB = 32 * RB;        // one ring slot
  __shared__ __attribute__((aligned(16))) unsigned char Gs[MS_NBUF * TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int split = blockIdx.x % nsplit;
  const long qb0 = (long)(blockIdx.x / nsplit) * (256 * QT);
  const long r_begin = (long)split * rows_per_split;
  long r_end = r_begin + rows_per_split;
  if (r_end > N) r_end = N;

  s16x8 qf[QT][NK];
  float ci[QT], ei[QT], ui[QT], fast[QT];
  int pi[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long q = qb0 + (w * QT + qt) * 32 + l31;
    const bool ok = q < nq;
    const long i = q0 + q;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ok) v = *(const s16x8*)(Gb + i * (long)(RB / 2) + ks * 16 + hi * 8);
      qf[qt][ks] = v;
    }
    ci[qt] = ok ? corep[i] : 0.f;
    pi[qt] = ok ? compp[i] : -2;
    ei[qt] = ok ? cbir_eps(gnorm, i, gmax_bits) : 0.f;
    ui[qt] = PROPOSE ? (ok ? U[q] : 0.f) : MS_INF;      // propose: U_i; bound: the running minimum
    fast[qt] = ms_fast(ui[qt]);
  }
  if (r_begin >= r_end) {   // uniform per workgroup (the host launches no empty slice)
    if (!PROPOSE) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const long q = qb0 + (w * QT + qt) * 32 + l31;
        if (hi == 0 && q < nq) Upart[(long)split * nqp + q] = MS_INF;
      }
    }
    return;
  }
  const long ntile = (r_end - r_begin + 31) / 32;
  // DMA one 32-row tile: NK / 8 instructions per wave; LDS slot (row, cp) holds chunk cp ^ (row & 15) of that row
#define MS_ISSUE(buf, t)                                                                                                  \
  do {                                                                                                                    \
    _Pragma("unroll") for (int j = 0; j < NK / 8; ++j) {                                                                   \
      const int L = j * 512 + w * 64 + lane;                                                                              \
      const int row = L / CH, cp = L % CH, c = cp ^ (row & 15);                                                           \
      long grow = r_begin + (long)(t) * 32 + row;                                                                         \
      if (grow > r_end - 1) grow = r_end - 1;                                                                             \
      const bf16_t* src = Gb + grow * (long)(RB / 2) + c * 8;                                                             \
      unsigned char* dst = Gs + (buf) * TILEB + (j * 512 + w * 64) * 16;                                                  \
      __builtin_amdgcn_global_load_lds(VDK_GLOBAL_PTR(src), VDK_LDS_PTR(dst), 16, 0, 0);                                   \
    }                                                                                                                     \
  } while (0)
  MS_ISSUE(0, 0);
  if (ntile > 1) MS_ISSUE(1, 1);
  if (ntile > 1) __builtin_amdgcn_s_waitcnt(0x0F70 | (NK / 8)); else __builtin_amdgcn_s_waitcnt(0x0F70);   // tile 0 landed
  __syncthreads();
  int cur = 0;
  for (long t = 0; t < ntile; ++t) {
    int nxt2 = cur + 2; if (nxt2 >= MS_NBUF) nxt2 -= MS_NBUF;
    if (t + 2 < ntile) MS_ISSUE(nxt2, t + 2);
    const long row0 = r_begin + t * 32;
    const unsigned char* Gt = Gs + cur * TILEB + l31 * RB;
    f32x16 acc[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[qt][0][r] = 0.f; acc[qt][1][r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < NK; ks += 2) {      // two accumulators per query tile: consecutive MFMAs do not wait for each other
      const s16x8 a0 = *(const s16x8*)(Gt + (((ks * 2 + hi) ^ (l31 & 15)) << 4));
      const s16x8 a1 = *(const s16x8*)(Gt + ((((ks + 1) * 2 + hi) ^ (l31 & 15)) << 4));
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        acc[qt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, qf[qt][ks], acc[qt][0], 0, 0, 0);
        acc[qt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, qf[qt][ks + 1], acc[qt][1], 0, 0, 0);
      }
    }
    const long left = N - row0;                                        // rows of this tile that exist (>= 1)
    const unsigned live = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      // fast path: one add and one compare per pair (MS_FAST); the bounds themselves only where a lane holds a pair that can matter
      unsigned pm = 0;
      float sb[16];
      bool hit = false;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sp = acc[qt][0][r] + acc[qt][1][r];
        sb[r] = PROPOSE ? sp + ei[qt] : sp - ei[qt];
        hit |= PROPOSE ? !(sb[r] < fast[qt]) : (sb[r] > fast[qt]);
      }
      if (hit) {
        // the tile's cores and components: register r of the lane = row (r & 3) + 8 (r >> 2) + 4 hi, so group g = r >> 2 is four consecutive rows (the padded copies
        // reach the end of the last tile).  Loaded only here: a load in the common path would make every tile wait for the DMAs issued before it
        f32x4 cj[4];
        ms_i32x4 pj[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          cj[g] = *(const f32x4*)(corep + row0 + 8 * g + 4 * hi);
          pj[g] = *(const ms_i32x4*)(compp + row0 + 8 * g + 4 * hi);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float cc = fmaxf(ci[qt], cj[r >> 2][r & 3]);
          const bool other = pj[r >> 2][r & 3] != pi[qt];
          if (PROPOSE) {
            const float lb = fmaxf(cc, 1.0f - ms_up(sb[r]));
            pm |= (other && !(lb > ui[qt])) ? (1u << r) : 0u;
          } else {
            const float ub = fmaxf(cc, 1.0f - ms_down(sb[r]));
            ui[qt] = (other && ub < ui[qt]) ? ub : ui[qt];
          }
        }
        if (!PROPOSE) fast[qt] = ms_fast(ui[qt]);
      }
      if (PROPOSE) {
        unsigned word = (pm & 0xfu) | ((pm & 0xf0u) << 4) | ((pm & 0xf00u) << 8) | ((pm & 0xf000u) << 12);   // nibble j -> bits 8 j .. 8 j + 3
        word <<= 4 * hi;
        word |= __shfl_xor(word, 32);                                    // the other half of the rows lives in lane ^ 32
        word &= live;
        const long q = qb0 + (w * QT + qt) * 32 + l31;
        if (hi == 0 && q < nq) mask[(row0 >> 5) * nqp + q] = word;
      }
    }
    if (t + 2 < ntile) __builtin_amdgcn_s_waitcnt(0x0F70 | (NK / 8)); else __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    cur = cur + 1 == MS_NBUF ? 0 : cur + 1;
  }
#undef MS_ISSUE
  if (!PROPOSE) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const float o = __shfl_xor(ui[qt], 32);
      const float m = o < ui[qt] ? o : ui[qt];
      const long q = qb0 + (w * QT + qt) * 32 + l31;
      if (hi == 0 && q < nq) Upart[(long)split * nqp + q] = m;
    }
  }
}

// U[q] = min over the slices (a fixed order; a minimum does not depend on it anyway)
__global__ __launch_bounds__(256) void mst_bound_reduce_kernel(const float* __restrict__ Upart, long nq, long nqp, int nsplit, float* __restrict__ U) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  float m = MS_INF;
  for (int s = 0; s < nsplit; ++s) { const float v = Upart[(long)s * nqp + q]; m = v < m ? v : m; }
  U[q] = m;
}

// ------------------------------------------------------------------------------------ 3 decide
// thread = (row q of the block, chunk c): exact w of every proposed pair of the chunk's words, pw / pj [c * nqp + q] = the smallest (w, j) or (+inf, -1).
// grid: id -> qtile = id % qtiles (256 rows, consecutive threads = consecutive rows: the mask words of a wave are contiguous), chunk = id / qtiles.
__global__ __launch_bounds__(256) void mst_decide_kernel(const float* __restrict__ X, const float* __restrict__ core, long q0, long nq, long nqp, int D, long NB, long qtiles,
                                                         const unsigned* __restrict__ mask, float* __restrict__ pw, int* __restrict__ pj) {
  const long q = (long)(blockIdx.x % qtiles) * 256 + threadIdx.x;
  const long c = (long)(blockIdx.x / qtiles);
  if (q >= nq) return;
  const long i = q0 + q;
  const float* xrow = X + i * (long)D;
  const float ci = core[i];
  long b_end = (c + 1) * MS_CHUNK; if (b_end > NB) b_end = NB;
  float bw = MS_INF;
  int bj = -1;
  for (long b0 = c * MS_CHUNK; b0 < b_end; b0 += MS_BATCH) {
    unsigned wd[MS_BATCH], any = 0;
#pragma unroll
    for (int j = 0; j < MS_BATCH; ++j) { wd[j] = b0 + j < b_end ? mask[(b0 + j) * nqp + q] : 0u; any |= wd[j]; }
    if (!any) continue;
#pragma unroll
    for (int j = 0; j < MS_BATCH; ++j) {
      for (unsigned m = wd[j]; m; m &= m - 1) {                       // ascending column: a strict < keeps the smallest j among equal w
        const long col = (b0 + j) * 32 + (__ffs((int)m) - 1);
        const float s = cbir_exact_ip(xrow, X + col * (long)D, D);
        const float wij = fmaxf(fmaxf(ci, core[col]), fmaxf(0.f, 1.0f - s));
        if (wij < bw || bj < 0) { bw = wij; bj = (int)col; }
      }
    }
  }
  pw[c * nqp + q] = bw;
  pj[c * nqp + q] = bj;
}
// per row: the smallest (w, j) over its chunks, in ascending chunk = ascending column order
__global__ __launch_bounds__(256) void mst_row_reduce_kernel(const float* __restrict__ pw, const int* __restrict__ pj, long q0, long nq, long nqp, long NC,
                                                             float* __restrict__ best_w, int* __restrict__ best_j) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  float bw = MS_INF;
  int bj = -1;
  for (long c = 0; c < NC; ++c) {
    const int j = pj[c * nqp + q];
    const float v = pw[c * nqp + q];
    if (j >= 0 && (bj < 0 || v < bw)) { bw = v; bj = j; }
  }
  best_w[q0 + q] = bw;
  best_j[q0 + q] = bj;
}

// ------------------------------------------------------------------------------------ host side
static inline size_t ms_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int ms_dp(int D) { return (D + 127) / 128 * 128; }   // padded width of the bf16 copy (as vdk_cbir_prepare_gallery built Gb)
struct MsWs { float* corep; int* compp; float* Upart; float* U; unsigned* mask; float* pw; int* pj; long nqp, NB, NC, qblocks, nsplit, rps; size_t bytes; };
static MsWs ms_carve(void* ws, int64_t nq, int64_t N, int32_t D) {
  MsWs c;
  c.nqp = (long)((nq + 63) / 64 * 64);                    // pitch of the per-row arrays: 256-byte multiples
  c.NB = (long)((N + 31) / 32);                           // 32-column mask words per row
  c.NC = (c.NB + MS_CHUNK - 1) / MS_CHUNK;
  // one round of workgroups over the 256 CUs where the shape allows: qblocks * nsplit <= 256, every slice at least 4 tiles long, no empty slice
  const int BQ = ms_dp(D) == 128 ? 512 : 256;
  c.qblocks = (long)((nq + BQ - 1) / BQ);
  long ns = 256 / (c.qblocks > 0 ? c.qblocks : 1);
  if (c.qblocks > 128) {                                  // more query blocks than half the chip: the slice count (<= 4) that fills whole rounds of 256 workgroups best
    double best = 0.0;
    for (long t = 1; t <= 4; ++t) {
      const long wg = c.qblocks * t;
      const double eff = (double)wg / (double)((wg + 255) / 256 * 256);
      if (eff > best + 1e-9) { best = eff; ns = t; }
    }
  }
  if (ns > c.NB / 4) ns = c.NB / 4;
  if (ns < 1) ns = 1;
  const long tiles = (c.NB + ns - 1) / ns;
  c.rps = tiles * 32;
  c.nsplit = tiles > 0 ? (c.NB + tiles - 1) / tiles : 1;
  if (c.nsplit < 1) c.nsplit = 1;
  const size_t o_comp = ms_align((size_t)c.NB * 32 * 4);
  const size_t o_up = o_comp + ms_align((size_t)c.NB * 32 * 4);
  const size_t o_u = o_up + ms_align((size_t)c.nsplit * c.nqp * 4);
  const size_t o_mask = o_u + ms_align((size_t)c.nqp * 4);
  const size_t o_pw = o_mask + ms_align((size_t)c.NB * c.nqp * 4);
  const size_t o_pj = o_pw + ms_align((size_t)c.NC * c.nqp * 4);
  c.bytes = o_pj + ms_align((size_t)c.NC * c.nqp * 4);
  char* p = (char*)ws;                                    // (null: only the sizes are wanted)
  c.corep = (float*)p;
  c.compp = p ? (int*)(p + o_comp) : nullptr;
  c.Upart = p ? (float*)(p + o_up) : nullptr;
  c.U = p ? (float*)(p + o_u) : nullptr;
  c.mask = p ? (unsigned*)(p + o_mask) : nullptr;
  c.pw = p ? (float*)(p + o_pw) : nullptr;
  c.pj = p ? (int*)(p + o_pj) : nullptr;
  return c;
}
static int ms_check_shape(int64_t nq, int64_t N, int32_t D, const char* who) {
  if (nq < 1 || N < 2 || D <= 0 || nq > N) return vdk_fail(VDK_EINVAL, who);
  if (N > 0x7fffffffLL) return vdk_fail(VDK_EINVAL, "vdk_mst: N < 2^31 (components and partners are int32)");
  if (D > 512) return vdk_fail(VDK_EINVAL, "vdk_mst: D <= 512 (the exact-scan form for wider rows is not built)");
  if (D & 3) return vdk_fail(VDK_EINVAL, "vdk_mst: need D % 4 == 0");
  if (((nq + 255) / 256) * (((N + 31) / 32 + MS_CHUNK - 1) / MS_CHUNK) > 0x7fffffffLL) return vdk_fail(VDK_EINVAL, "vdk_mst: too many (row, chunk) pairs for one call: pass fewer rows");
  return VDK_OK;
}
static inline bool ms_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" {

int vdk_mst_scan_workspace_bytes(int64_t nq, int64_t N, int32_t D, size_t* bytes) {
  if (!bytes) return vdk_fail(VDK_EINVAL, "vdk_mst_scan_workspace_bytes: bad argument");
  int rc = ms_check_shape(nq, N, D, "vdk_mst_scan_workspace_bytes: bad argument (1 <= nq <= N, N >= 2)");
  if (rc) return rc;
  *bytes = ms_carve(nullptr, nq, N, D).bytes;
  return VDK_OK;
}

// tools (tools/bench_hdbscan.py counts the proposed pairs): where the last scan of this shape left its one-bit-per-pair matrix inside the workspace: word
// [b * pitch_words + q] at offset_bytes, b < blocks (32 columns each), q < nq
int vdk_mst_scan_mask_layout(int64_t nq, int64_t N, int32_t D, size_t* offset_bytes, int64_t* pitch_words, int64_t* blocks) {
  if (!offset_bytes || !pitch_words || !blocks) return vdk_fail(VDK_EINVAL, "vdk_mst_scan_mask_layout: bad argument");
  int rc = ms_check_shape(nq, N, D, "vdk_mst_scan_mask_layout: bad argument (1 <= nq <= N, N >= 2)");
  if (rc) return rc;
  const MsWs c = ms_carve((void*)256, nq, N, D);
  *offset_bytes = (size_t)((char*)c.mask - (char*)256);
  *pitch_words = c.nqp;
  *blocks = c.NB;
  return VDK_OK;
}

int vdk_mst_scan(const float* X, const void* Gb, const float* gnorm, const uint32_t* gmax_bits, const float* core, const int32_t* comp, int64_t N, int32_t D, int64_t q0,
                 int64_t nq, float* best_w, int32_t* best_j, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ms_check_shape(nq, N, D, "vdk_mst_scan: bad argument (1 <= nq <= N, N >= 2)");
  if (rc) return rc;
  if (q0 < 0 || q0 + nq > N) return vdk_fail(VDK_EINVAL, "vdk_mst_scan: the row block [q0, q0 + nq) must lie inside [0, N)");
  if (!X || !Gb || !gnorm || !gmax_bits || !core || !comp || !best_w || !best_j) return vdk_fail(VDK_EINVAL, "vdk_mst_scan: null pointer");
  if (ms_misaligned(X, 16) || ms_misaligned(Gb, 16) || ms_misaligned(ws, 16) || ms_misaligned(gnorm, 4) || ms_misaligned(gmax_bits, 4) || ms_misaligned(core, 4) ||
      ms_misaligned(comp, 4) || ms_misaligned(best_w, 4) || ms_misaligned(best_j, 4))
    return vdk_fail(VDK_EINVAL, "vdk_mst_scan: misaligned pointer (X, Gb and the workspace 16 bytes, the others 4)");
  if (!ws || ws_bytes < ms_carve(nullptr, nq, N, D).bytes) return vdk_fail(VDK_EWORKSPACE, "vdk_mst_scan: workspace too small");
  const MsWs c = ms_carve(ws, nq, N, D);
  const int DP = ms_dp(D);
  const long NP = c.NB * 32;
  hipLaunchKernelGGL(mst_pack_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, stream, core, (const int*)comp, (long)N, NP, c.corep, c.compp);
  const dim3 grid((unsigned)(c.qblocks * c.nsplit));
#define MS_LAUNCH(NK, QT, P)                                                                                                                                     \
  hipLaunchKernelGGL((mst_scan_kernel<NK, QT, P>), grid, dim3(512), 0, stream, (const bf16_t*)Gb, gnorm, (const unsigned*)gmax_bits, (const float*)c.corep,       \
                     (const int*)c.compp, (long)N, (long)q0, (long)nq, c.nqp, c.rps, (int)c.nsplit, (const float*)c.U, c.Upart, c.mask)
#define MS_PASS(P)                                \
  switch (DP) {                                   \
    case 128: MS_LAUNCH(8, 2, P); break;          \
    case 256: MS_LAUNCH(16, 1, P); break;         \
    case 384: MS_LAUNCH(24, 1, P); break;         \
    default: MS_LAUNCH(32, 1, P); break;          \
  }
  const long qtiles = (long)((nq + 255) / 256);
  MS_PASS(0)
  hipLaunchKernelGGL(mst_bound_reduce_kernel, dim3((unsigned)qtiles), dim3(256), 0, stream, (const float*)c.Upart, (long)nq, c.nqp, (int)c.nsplit, c.U);
  MS_PASS(1)
#undef MS_PASS
#undef MS_LAUNCH
  hipLaunchKernelGGL(mst_decide_kernel, dim3((unsigned)(qtiles * c.NC)), dim3(256), 0, stream, X, core, (long)q0, (long)nq, c.nqp, (int)D, c.NB, qtiles,
                     (const unsigned*)c.mask, c.pw, c.pj);
  hipLaunchKernelGGL(mst_row_reduce_kernel, dim3((unsigned)qtiles), dim3(256), 0, stream, (const float*)c.pw, (const int*)c.pj, (long)q0, (long)nq, c.nqp, c.NC, best_w,
                     (int*)best_j);
  return vdk_check_launch("vdk_mst_scan");
}

}  // extern "C"

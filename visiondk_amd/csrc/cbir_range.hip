// cbir_range.hip — hot path B, the threshold question: every gallery row whose EXACT inner product with a query passes a radius (faiss IndexFlat.range_search), and
// cosine DBSCAN on the neighbourhood lists it returns (the reference's tools/clustering.py: DBSCAN(eps, min_samples, metric="cosine") over the extracted features).
//
// Arithmetic contract = the top-k search's (cbir.hip):
//  * the bf16-MFMA pre-filter only PROPOSES: a pair with exact score s >= r has s' >= r - eps_q (eps_q = cbir_eps: the measured rounding-error norms of the query and of
//    the gallery in gmax_bits), so keeping s' >= r - eps_q never drops a member;
//  * the DECISION is taken on the exact score, the k-ordered fp32 fmaf chain from +0 (cbir_exact_ip / cbir_exact_ip_h = oracle_ip_pair): s > r, or s >= r when inclusive.
//
// Structure: NO candidate lists, hence no capacity, no overflow flag and no repeat.  The result size is decided by the data, so the scan writes what has a size that is
// known beforehand: ONE BIT PER PAIR.
//   vdk_cbir_range_count
//     1 filter   one pass of the pre-filter; a wave's 32 x 32 accumulator block becomes 32 words mask[block][query] (bit i = row 32 block + i proposed), every word
//                written whether it is zero or not (nq N / 8 bytes: 1.25 GB of stores for 10 k x 1 M, against the 2.56 G MFMA multiply-adds per query block);
//     2 decide   a thread per (query, chunk of 64 words = 2048 rows) walks its words, gives every proposed pair its exact score, clears the bits that fail the radius
//                and leaves the chunk's member count;
//     3 offsets  per query: exclusive prefix of its chunk counts (in place) and its total; a one-workgroup scan of the totals gives lims int64 [nq + 1].
//   (the host reads lims[nq] -- the one host read -- and allocates D and I)
//   vdk_cbir_range_fill
//     4 write    the same (query, chunk) threads walk the now exact masks in ascending row order and write I = idx_base + row and D = the exact score (the chain again: the
//                same instructions on the same operands, the same bits) at lims[q] + the chunk's offset.
// Every (query, chunk) owns a fixed slice of the output and walks it in row order, so a query's results are in ASCENDING GALLERY INDEX by construction: no atomics, no
// sort, and the same bits on every run.  A radius below every score returns all nq N pairs through the same path.
//
// DBSCAN (sklearn's dbscan_inner result) on the CSR, gather forms without atomics: core flags from the neighbourhood sizes; components of the core points by
// label[i] <- label[min over core neighbours j of label[j]] in Jacobi rounds (two buffers: the number of rounds is a property of the data, not of the schedule) until a
// device flag stays clear; a core point's cluster = rank of its component's smallest index among the roots, a border point's = the smallest cluster among its core
// neighbours, everything else -1.
#include <hip/hip_runtime.h>
#include <cmath>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_internal.h"
#include "cbir_device.h"

#define CR_NBUF 3        // LDS-DMA ring depth (as the top-k pre-filters: the DMA's latency under load, not its bandwidth, is what has to be covered)
#define CR_CHUNK 64      // 32-row mask words per (query, chunk) thread of the decide / write kernels: 2048 gallery rows
#define CR_BATCH 16      // mask words (chunk counts) a thread loads before it looks at any of them

// ------------------------------------------------------------------------------------ 1 filter
// The wide pre-filter's form (cbir_prefilter_wide_kernel) for every width: a ring slot holds a 32-row gallery tile of NK k-steps (32 x NK x 32 B <= 32 KB, rows past N are
// clamped copies of row N - 1 and masked out), a wave keeps the bf16 fragments of QT 32-query tiles in registers (NK = 8: two tiles, so a tile read from LDS feeds 16 MFMAs;
// NK >= 16: one) and a workgroup of 8 waves covers 256 QT queries.  grid: id -> split = id % nsplit (a slice of rows_per_split rows, a multiple of 32), qblock = id / nsplit.
// Output: mask[b * nqp + q] for every 32-row block b of the slice and every q < nq of the block.
template <int NK, int QT>
__global__ __launch_bounds__(512) void cbir_range_filter_kernel(const bf16_t* __restrict__ Qb, const float* __restrict__ qnorm, long nq, long nqp, const bf16_t* __restrict__ Gb,
                                                                const unsigned* __restrict__ gmax_bits, long N, long rows_per_split, int nsplit, float radius,
                                                                unsigned* __restrict__ mask) {
  constexpr int RB = NK * 32;           // bytes per bf16 row
  constexpr int CH = RB / 16;           // 16-byte chunks per row
  constexpr int TILEB = 32 * RB;        // one ring slot
  __shared__ __attribute__((aligned(16))) unsigned char Gs[CR_NBUF * TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int split = blockIdx.x % nsplit;
  const long q0 = (long)(blockIdx.x / nsplit) * (256 * QT);
  const long r_begin = (long)split * rows_per_split;
  long r_end = r_begin + rows_per_split;
  if (r_end > N) r_end = N;
  if (r_begin >= r_end) return;   // uniform per workgroup

  s16x8 qf[QT][NK];
  float cut[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long q = q0 + (w * QT + qt) * 32 + l31;
    const bool ok = q < nq;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ok) v = *(const s16x8*)(Qb + q * (long)(RB / 2) + ks * 16 + hi * 8);
      qf[qt][ks] = v;
    }
    // proposed <=> s' >= r - eps_q, written !(s' < cut): an approximate score that is NaN (infinite operands) is proposed too, the exact score decides
    cut[qt] = ok ? radius - cbir_eps(qnorm, q, gmax_bits) : __uint_as_float(0x7f800000u);
  }
  const long ntile = (r_end - r_begin + 31) / 32;
  // DMA one 32-row tile: NK / 8 instructions per wave; LDS slot (row, cp) holds chunk cp ^ (row & 15) of that row
#define CR_ISSUE(buf, t)                                                                                                  \
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
  CR_ISSUE(0, 0);
  if (ntile > 1) CR_ISSUE(1, 1);
  if (ntile > 1) __builtin_amdgcn_s_waitcnt(0x0F70 | (NK / 8)); else __builtin_amdgcn_s_waitcnt(0x0F70);   // tile 0 landed
  __syncthreads();
  int cur = 0;
  for (long t = 0; t < ntile; ++t) {
    // ring slot (cur + 2) % 3 was consumed during iteration t - 1 (everybody passed the barrier that ended it)
    int nxt2 = cur + 2; if (nxt2 >= CR_NBUF) nxt2 -= CR_NBUF;
    if (t + 2 < ntile) CR_ISSUE(nxt2, t + 2);
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
    const long row0 = r_begin + t * 32;
    const long left = N - row0;                                        // rows of this tile that exist (>= 1)
    const unsigned live = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      // register r of the lane = row (r & 3) + 8 (r >> 2) + 4 hi of the block, column = the lane's query
      unsigned pm = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) pm |= (acc[qt][0][r] + acc[qt][1][r] < cut[qt]) ? 0u : (1u << r);
      unsigned word = (pm & 0xfu) | ((pm & 0xf0u) << 4) | ((pm & 0xf00u) << 8) | ((pm & 0xf000u) << 12);   // nibble j -> bits 8 j .. 8 j + 3
      word <<= 4 * hi;
      word |= __shfl_xor(word, 32);                                    // the other half of the rows lives in lane ^ 32
      word &= live;
      const long q = q0 + (w * QT + qt) * 32 + l31;
      if (hi == 0 && q < nq) mask[(row0 >> 5) * nqp + q] = word;       // 32 consecutive words per wave and query tile
    }
    // tile t + 1 must have landed: only tile t + 2's DMAs (and this iteration's mask stores, which are younger) may still be in flight
    if (t + 2 < ntile) __builtin_amdgcn_s_waitcnt(0x0F70 | (NK / 8)); else __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    cur = cur + 1 == CR_NBUF ? 0 : cur + 1;
  }
#undef CR_ISSUE
}

// ------------------------------------------------------------------------------------ 2 decide
// thread = (query q, chunk c): exact score of every proposed pair of the chunk's words, bits that fail the radius cleared, cnt[c * nqp + q] = members left.
// grid: id -> qtile = id % qtiles (256 queries, consecutive threads = consecutive queries: the mask words of a wave are contiguous), chunk = id / qtiles.
__global__ __launch_bounds__(256) void cbir_range_decide_kernel(const float* __restrict__ Q, long nq, long nqp, const float* __restrict__ G, int D, int g_half, long NB, long qtiles,
                                                                float radius, int inclusive, unsigned* __restrict__ mask, unsigned* __restrict__ cnt) {
  const long q = (long)(blockIdx.x % qtiles) * 256 + threadIdx.x;
  const long c = (long)(blockIdx.x / qtiles);
  if (q >= nq) return;
  const float* qrow = Q + q * (long)D;
  long b_end = (c + 1) * CR_CHUNK; if (b_end > NB) b_end = NB;
  unsigned n = 0;
  for (long b0 = c * CR_CHUNK; b0 < b_end; b0 += CR_BATCH) {
    // CR_BATCH independent loads, then one test: almost every batch of a selective radius is empty (a word at a time is one exposed memory latency per word)
    unsigned wd[CR_BATCH], any = 0;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) { wd[j] = b0 + j < b_end ? mask[(b0 + j) * nqp + q] : 0u; any |= wd[j]; }
    if (!any) continue;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      const unsigned word = wd[j];
      if (!word) continue;
      const long b = b0 + j;
      unsigned keep = word;
      for (unsigned m = word; m; m &= m - 1) {
        const int bit = __ffs((int)m) - 1;
        const float s = cbir_exact_ip_any(qrow, G, b * 32 + bit, D, g_half);
        if (!(inclusive ? s >= radius : s > radius)) keep &= ~(1u << bit);
      }
      if (keep != word) mask[b * nqp + q] = keep;
      n += (unsigned)__popc(keep);
    }
  }
  cnt[c * nqp + q] = n;
}

// ------------------------------------------------------------------------------------ 3 offsets
// per query: cnt[c][q] <- exclusive prefix over the chunks (in place), tot[q] = the query's result count
__global__ __launch_bounds__(256) void cbir_range_offsets_kernel(long nq, long nqp, long NC, unsigned* __restrict__ cnt, long long* __restrict__ tot) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  unsigned run = 0;             // <= N < 2^32 per query
  for (long c0 = 0; c0 < NC; c0 += CR_BATCH) {
    unsigned t[CR_BATCH];
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) t[j] = c0 + j < NC ? cnt[(c0 + j) * nqp + q] : 0u;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      if (c0 + j < NC) cnt[(c0 + j) * nqp + q] = run;
      run += t[j];
    }
  }
  tot[q] = (long long)run;
}
// lims[0] = 0, lims[i + 1] = tot[0] + ... + tot[i]: one workgroup of 1024 threads, a contiguous segment per thread (tot == nullptr: all zero)
__global__ __launch_bounds__(1024) void cbir_range_scan_kernel(const long long* __restrict__ tot, long nq, long long* __restrict__ lims) {
  __shared__ long long seg[1024];
  const int tid = threadIdx.x;
  const long per = (nq + 1023) / 1024;
  long lo = tid * per, hi = lo + per;
  if (lo > nq) lo = nq;
  if (hi > nq) hi = nq;
  long long s = 0;
  if (tot) for (long i = lo; i < hi; ++i) s += tot[i];
  seg[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < 1024; ++i) { const long long v = seg[i]; seg[i] = run; run += v; }
  }
  __syncthreads();
  long long run = seg[tid];
  if (tid == 0) lims[0] = 0;
  for (long i = lo; i < hi; ++i) { run += tot ? tot[i] : 0; lims[i + 1] = run; }
}

// ------------------------------------------------------------------------------------ 4 write
// thread = (query, chunk) as in the decide kernel: members in ascending row order to out[lims[q] + cnt[c][q] ...]
__global__ __launch_bounds__(256) void cbir_range_write_kernel(const float* __restrict__ Q, long nq, long nqp, const float* __restrict__ G, int D, int g_half, long NB, long NC, long qtiles,
                                                               long idx_base, const unsigned* __restrict__ mask, const unsigned* __restrict__ cnt,
                                                               const long long* __restrict__ lims, float* __restrict__ out_score, long long* __restrict__ out_idx) {
  const long q = (long)(blockIdx.x % qtiles) * 256 + threadIdx.x;
  const long c = (long)(blockIdx.x / qtiles);
  if (q >= nq) return;
  const float* qrow = Q + q * (long)D;
  long b_end = (c + 1) * CR_CHUNK; if (b_end > NB) b_end = NB;
  const unsigned first = cnt[c * nqp + q];
  const long long mine = (c + 1 < NC ? (long long)cnt[(c + 1) * nqp + q] : lims[q + 1] - lims[q]) - (long long)first;     // members of this chunk
  if (mine == 0) return;                      // (most chunks of a selective radius)
  long long pos = lims[q] + (long long)first;
  const long long end = pos + mine;
  for (long b0 = c * CR_CHUNK; b0 < b_end && pos < end; b0 += CR_BATCH) {
    unsigned wd[CR_BATCH], any = 0;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) { wd[j] = b0 + j < b_end ? mask[(b0 + j) * nqp + q] : 0u; any |= wd[j]; }
    if (!any) continue;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      for (unsigned m = wd[j]; m; m &= m - 1) {
        const long row = (b0 + j) * 32 + (__ffs((int)m) - 1);
        out_score[pos] = cbir_exact_ip_any(qrow, G, row, D, g_half);
        out_idx[pos] = (long long)(idx_base + row);
        ++pos;
      }
    }
  }
}

// ------------------------------------------------------------------------------------ DBSCAN on the CSR
// core[i] = |N(i)| >= min_samples (the neighbourhood contains the point itself, as sklearn's does); label[i] = i for a core point, -1 otherwise
__global__ __launch_bounds__(256) void dbscan_core_kernel(const long long* __restrict__ lims, long n, long min_samples, unsigned char* __restrict__ core, int* __restrict__ label) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool c = lims[i + 1] - lims[i] >= (long long)min_samples;
  core[i] = c ? 1 : 0;
  label[i] = c ? (int)i : -1;
}
// wave-wide minimum of non-negative ints
__device__ __forceinline__ int dbscan_wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o < v ? o : v; }
  return v;
}
// one Jacobi round, a wave per point: out[i] = in[min(in[i], min over core neighbours j of in[j])] -- the minimum over the neighbourhood, then one pointer jump (in[m] <= m
// is a core point of the same component).  Labels only decrease and stay inside the component, so the fixed point is the component's smallest core index.
__global__ __launch_bounds__(256) void dbscan_round_kernel(const long long* __restrict__ lims, const long long* __restrict__ nbr, long n, const unsigned char* __restrict__ core,
                                                           const int* __restrict__ in, int* __restrict__ out, unsigned* __restrict__ changed) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                       // wave-uniform
  if (!core[i]) { if (lane == 0) out[i] = -1; return; }
  const int mine = in[i];
  int m = mine;
  for (long long e = lims[i] + lane; e < lims[i + 1]; e += 64) {
    const long long j = nbr[e];
    if (j >= 0 && j < n && core[j]) { const int lj = in[j]; m = lj < m ? lj : m; }
  }
  m = dbscan_wave_min(m);
  m = in[m];
  if (lane == 0) {
    out[i] = m;
    if (m != mine) *changed = 1u;           // (every writer stores the same value)
  }
}
// labels: a core point takes rank[root of its component]; a non-core point the smallest such rank among its core neighbours, or -1.  rank = exclusive prefix sum of the
// "is a root" mask (root: core and label[i] == i), so clusters are numbered by their smallest core index -- sklearn's scan order.
__global__ __launch_bounds__(256) void dbscan_assign_kernel(const long long* __restrict__ lims, const long long* __restrict__ nbr, long n, const unsigned char* __restrict__ core,
                                                            const int* __restrict__ label, const int* __restrict__ rank, long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                       // wave-uniform
  if (core[i]) { if (lane == 0) out[i] = (long long)rank[label[i]]; return; }
  int m = 0x7fffffff;
  for (long long e = lims[i] + lane; e < lims[i + 1]; e += 64) {
    const long long j = nbr[e];
    if (j >= 0 && j < n && core[j]) { const int r = rank[label[j]]; m = r < m ? r : m; }
  }
  m = dbscan_wave_min(m);
  if (lane == 0) out[i] = m == 0x7fffffff ? -1ll : (long long)m;
}

// ------------------------------------------------------------------------------------ host side
static inline size_t cr_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int cr_dp(int D) { return (D + 127) / 128 * 128; }   // padded width of the bf16 copies (as vdk_cbir_prepare_gallery built Gb)
struct CrWs { bf16_t* Qb; float* qnorm; unsigned* mask; unsigned* cnt; long long* tot; long nqp, NB, NC; size_t bytes; };
static CrWs cr_carve(void* ws, int64_t nq, int64_t N, int32_t D) {
  CrWs c;
  c.nqp = (long)((nq + 63) / 64 * 64);                    // pitch of the mask / count rows: 256-byte multiples
  c.NB = (long)((N + 31) / 32);                           // 32-row mask words per query
  c.NC = (c.NB + CR_CHUNK - 1) / CR_CHUNK;
  const size_t o_qn = cr_align((size_t)nq * cr_dp(D) * 2);
  const size_t o_mask = o_qn + cr_align((size_t)nq * 12);
  const size_t o_cnt = o_mask + cr_align((size_t)c.NB * c.nqp * 4);
  const size_t o_tot = o_cnt + cr_align((size_t)c.NC * c.nqp * 4);
  c.bytes = o_tot + cr_align((size_t)nq * 8);
  char* p = (char*)ws;                                    // (null: only the sizes are wanted)
  c.Qb = (bf16_t*)p;
  c.qnorm = p ? (float*)(p + o_qn) : nullptr;
  c.mask = p ? (unsigned*)(p + o_mask) : nullptr;
  c.cnt = p ? (unsigned*)(p + o_cnt) : nullptr;
  c.tot = p ? (long long*)(p + o_tot) : nullptr;
  return c;
}
static int cr_check_shape(int64_t nq, int64_t N, int32_t D, int32_t g_dtype, const char* who) {
  if (nq < 0 || N < 0 || D <= 0) return vdk_fail(VDK_EINVAL, who);
  if (D > 512) return vdk_fail(VDK_EINVAL, "vdk_cbir_range: D <= 512 (the exact-scan form for wider rows is not built)");
  if (g_dtype != VDK_F32 && g_dtype != VDK_F16) return vdk_fail(VDK_EINVAL, "vdk_cbir_range: g_dtype must be VDK_F32 or VDK_F16");
  if (D & 3) return vdk_fail(VDK_EINVAL, "vdk_cbir_range: need D % 4 == 0");
  if (g_dtype == VDK_F16 && (D & 7)) return vdk_fail(VDK_EINVAL, "vdk_cbir_range: fp16 storage needs D % 8 == 0");
  if (((nq + 255) / 256) * (((N + 31) / 32 + CR_CHUNK - 1) / CR_CHUNK) > 0x7fffffffLL) return vdk_fail(VDK_EINVAL, "vdk_cbir_range: too many (query, chunk) pairs for one call: pass fewer queries");
  return VDK_OK;
}

extern "C" {

// workspace of vdk_cbir_range_count / vdk_cbir_range_fill for nq queries against N rows of D columns: the queries' bf16 copy and norms, one bit per pair, one count per
// (query, 2048-row chunk), one total per query.  The same buffer, untouched in between, goes to both calls.
int vdk_cbir_range_workspace_bytes(int64_t nq, int64_t N, int32_t D, size_t* bytes) {
  if (!bytes) return vdk_fail(VDK_EINVAL, "vdk_cbir_range_workspace_bytes: bad argument");
  int rc = cr_check_shape(nq, N, D, VDK_F32, "vdk_cbir_range_workspace_bytes: bad argument");
  if (rc) return rc;
  *bytes = cr_carve(nullptr, nq, N, D).bytes;
  return VDK_OK;
}

int vdk_cbir_range_count(const float* Q, int64_t nq, const void* G, int32_t g_dtype, const void* Gb, const uint32_t* gmax_bits, int64_t N, int32_t D, float radius,
                         int32_t inclusive, int64_t* lims, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = cr_check_shape(nq, N, D, g_dtype, "vdk_cbir_range_count: bad argument");
  if (rc) return rc;
  if (radius != radius) return vdk_fail(VDK_EINVAL, "vdk_cbir_range_count: the radius is NaN");
  if (!lims || (!Q && nq > 0) || ((!G || !Gb) && N > 0) || !gmax_bits) return vdk_fail(VDK_EINVAL, "vdk_cbir_range_count: null pointer");
  if (nq == 0 || N == 0) {   // lims[0 .. nq] = 0
    hipLaunchKernelGGL(cbir_range_scan_kernel, dim3(1), dim3(1024), 0, stream, (const long long*)nullptr, (long)nq, (long long*)lims);
    return vdk_check_launch("vdk_cbir_range_count");
  }
  if (!ws || ws_bytes < cr_carve(nullptr, nq, N, D).bytes) return vdk_fail(VDK_EWORKSPACE, "vdk_cbir_range_count: workspace too small");
  const CrWs c = cr_carve(ws, nq, N, D);
  const int DP = cr_dp(D), g_half = g_dtype == VDK_F16;
  vdk_cbir_cast_rows(Q, (long)nq, (int)D, DP, c.Qb, c.qnorm, stream_);
  // one round of workgroups over the 256 CUs where the shape allows: qblocks * nsplit <= 256, every split at least 4 tiles long (as the top-k scan)
  const int BQ = DP == 128 ? 512 : 256;
  const long qblocks = (long)((nq + BQ - 1) / BQ);
  long nsplit = 256 / qblocks;
  if (nsplit > c.NB / 4) nsplit = c.NB / 4;
  if (nsplit < 1) nsplit = 1;
  const long rps = ((c.NB + nsplit - 1) / nsplit) * 32;
  const dim3 grid((unsigned)(qblocks * nsplit));
#define CR_LAUNCH(NK, QT)                                                                                                                                   \
  hipLaunchKernelGGL((cbir_range_filter_kernel<NK, QT>), grid, dim3(512), 0, stream, (const bf16_t*)c.Qb, (const float*)c.qnorm, (long)nq, c.nqp, (const bf16_t*)Gb, \
                     (const unsigned*)gmax_bits, (long)N, rps, (int)nsplit, radius, c.mask)
  switch (DP) {
    case 128: CR_LAUNCH(8, 2); break;
    case 256: CR_LAUNCH(16, 1); break;
    case 384: CR_LAUNCH(24, 1); break;
    default: CR_LAUNCH(32, 1); break;
  }
#undef CR_LAUNCH
  const long qtiles = (long)((nq + 255) / 256);
  hipLaunchKernelGGL(cbir_range_decide_kernel, dim3((unsigned)(qtiles * c.NC)), dim3(256), 0, stream, Q, (long)nq, c.nqp, (const float*)G, (int)D, g_half, c.NB, qtiles, radius,
                     (int)(inclusive != 0), c.mask, c.cnt);
  hipLaunchKernelGGL(cbir_range_offsets_kernel, dim3((unsigned)qtiles), dim3(256), 0, stream, (long)nq, c.nqp, c.NC, c.cnt, c.tot);
  hipLaunchKernelGGL(cbir_range_scan_kernel, dim3(1), dim3(1024), 0, stream, (const long long*)c.tot, (long)nq, (long long*)lims);
  return vdk_check_launch("vdk_cbir_range_count");
}

int vdk_cbir_range_fill(const float* Q, int64_t nq, const void* G, int32_t g_dtype, int64_t N, int32_t D, int64_t idx_base, const int64_t* lims, int64_t total, float* out_scores,
                        int64_t* out_idx, const void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = cr_check_shape(nq, N, D, g_dtype, "vdk_cbir_range_fill: bad argument");
  if (rc) return rc;
  if (total < 0 || !lims || (!Q && nq > 0) || (!G && N > 0)) return vdk_fail(VDK_EINVAL, "vdk_cbir_range_fill: bad argument");
  if (total > 0 && (!out_scores || !out_idx)) return vdk_fail(VDK_EINVAL, "vdk_cbir_range_fill: null output with a non-zero result count");
  if (nq == 0 || N == 0 || total == 0) return VDK_OK;
  if (!ws || ws_bytes < cr_carve(nullptr, nq, N, D).bytes) return vdk_fail(VDK_EWORKSPACE, "vdk_cbir_range_fill: workspace too small");
  const CrWs c = cr_carve((void*)ws, nq, N, D);
  const long qtiles = (long)((nq + 255) / 256);
  hipLaunchKernelGGL(cbir_range_write_kernel, dim3((unsigned)(qtiles * c.NC)), dim3(256), 0, stream, Q, (long)nq, c.nqp, (const float*)G, (int)D, (int)(g_dtype == VDK_F16), c.NB,
                     c.NC, qtiles, (long)idx_base, (const unsigned*)c.mask, (const unsigned*)c.cnt, (const long long*)lims, out_scores, (long long*)out_idx);
  return vdk_check_launch("vdk_cbir_range_fill");
}

int vdk_dbscan_core(const int64_t* lims, int64_t n, int64_t min_samples, uint8_t* core, int32_t* label, void* stream) {
  if (n < 0 || n > 0x7fffffffLL || min_samples < 1 || (n > 0 && (!lims || !core || !label))) return vdk_fail(VDK_EINVAL, "vdk_dbscan_core: bad argument (0 <= n < 2^31, min_samples >= 1)");
  if (n == 0) return VDK_OK;
  hipLaunchKernelGGL(dbscan_core_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)lims, (long)n, (long)min_samples, core, label);
  return vdk_check_launch("vdk_dbscan_core");
}

int vdk_dbscan_round(const int64_t* lims, const int64_t* nbr, int64_t n, const uint8_t* core, const int32_t* label_in, int32_t* label_out, uint32_t* changed, void* stream) {
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!lims || !core || !label_in || !label_out || !changed)) || label_in == label_out)
    return vdk_fail(VDK_EINVAL, "vdk_dbscan_round: bad argument (two distinct label buffers)");
  if (n == 0) return VDK_OK;
  hipLaunchKernelGGL(dbscan_round_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const long long*)lims, (const long long*)nbr, (long)n, core, label_in,
                     label_out, changed);
  return vdk_check_launch("vdk_dbscan_round");
}

int vdk_dbscan_assign(const int64_t* lims, const int64_t* nbr, int64_t n, const uint8_t* core, const int32_t* label, const int32_t* rank, int64_t* out, void* stream) {
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!lims || !core || !label || !rank || !out))) return vdk_fail(VDK_EINVAL, "vdk_dbscan_assign: bad argument");
  if (n == 0) return VDK_OK;
  hipLaunchKernelGGL(dbscan_assign_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const long long*)lims, (const long long*)nbr, (long)n, core, label, rank,
                     (long long*)out);
  return vdk_check_launch("vdk_dbscan_assign");
}

}  // extern "C"

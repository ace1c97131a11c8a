// attention_hd.hip — K3 forward and backward for head dimensions beyond 64, with the head dimension HD as a template parameter.  Instantiated and dispatched for
// HD = 80 (ViT-H/14 CLIP: 1280 / 16 heads) and HD = 72 (SigLIP SO400M/14: 1152 / 16 heads; the ragged instance, see below).  Same operator and operand contract as attention.hip / attention_small.hip / attention_long.hip:
// softmax(q k^T / sqrt(hd)) v on 16-bit [B, N, 3, H, hd] rows of arbitrary (% 8) pitch, lse and D in fp32, and the same rounding points (scores and statistics in fp32,
// exp2 with scale * log2(e) folded in, P / O / dS rounded once, the backward consumes the forward's own 16-bit o and lse).
//
// One streaming (online-softmax) kernel set covers every N >= 1; the structure is attention_long.hip's:
//   * a work unit is (batch, head, group of 4 query tiles) -- in the kv kernel 4 key tiles --; wave w owns tile 4g + w, its own-row fragments (Q; Q, dO; K, V) come
//     straight from global, the accumulators O^T / dQ^T / dK^T, dV^T (lane = row) stay in registers;
//   * the streamed operands (K, V; K, V; Q, dO) arrive in chunks of 64 rows by LDS-DMA into a double buffer: the chunk after the current one -- of this unit or of the
//     workgroup's next unit -- is requested right after the single barrier of a chunk;
//   * units are numbered so that the groups of one (batch, head) item run at the same time on one XCD (workgroup b lives on XCD b mod 8);
//   * the backward is the recompute form in two kernels (dQ and D by query-tile owner, then dK / dV by key-tile owner): no atomics, fixed summation order.
//
// What differs is the row.  A head's row is HD * 2 = 160 bytes = 10 chunks of 16 bytes, and the power-of-two XOR swizzle over the 8 chunks of a 128-byte row
// (vdk_attn_tile.h) does not apply.  LDS layout here: a staged row takes 12 chunk slots (192 bytes: the 10 chunks and two pad slots); chunk c of row r sits in slot
//     pos(r, c) = (c & ~3) | ((c & 3) ^ ((r >> 2) & 3))                      (an XOR inside each aligned group of 4 chunks -- the pad slots complete the last group)
// Why that is conflict-free for both read patterns (banks: (byte / 4) mod 64, i.e. 16 slots of 16 bytes per bank row; MI355X_MICROARCH.md, LDS):
//   * transposed reads (ds_read_b64_tr_b16, P V / dS K / dO^T P / Q^T dS operands; conflicts count per 32-lane half): a half reads 4 consecutive rows 4m .. 4m + 3, of
//     each the 64 contiguous bytes of ONE aligned group of 4 chunks (the XOR only permutes inside that group).  Row r starts at slot 12 r mod 16 = {0, 12, 8, 4} for
//     r mod 4 = {0, 1, 2, 3}: the four rows cover the four quarters of the bank row, every bank once.
//   * row reads (ds_read_b128, q k^T / dO v^T operands; conflicts count per 16-lane group {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of rows): lane = row, chunk c fixed.
//     r mod 4 picks the quarter of the bank row as above; the four rows of a group that share r mod 4 have (r >> 2) & 3 = {0, 3, 1, 2} resp. {1, 2, 0, 3}, all
//     different, so the XOR puts them in the four different slots of that quarter: 16 lanes, 16 slots.
// The two pad slots of a row are filled by the DMA with copies of real chunks of the same row (an LDS-DMA instruction writes 64 consecutive slots, so every slot gets
// something; the copies keep the source inside the head's columns), which also gives every lane of the third transposed read (columns 64 .. 95) an in-bounds address:
// the MFMAs that produce columns 64 .. 79 of an output produce 16 further rows from the copies, which are never stored.  Cost: 6 instead of 5 MFMA-equivalents for the
// products whose OUTPUT is HD wide (P V, dS K, dO^T P, Q^T dS); q k^T and dO v^T contract over HD in exactly 5 steps.
//
// LDS per workgroup: 2 x 24 KB chunk buffers (+ 2 x 1 KB lse / D in the kv kernel) + 4 wave store tiles of 32 x 176 bytes = 70.5 / 72.5 KB: two workgroups per CU.
//
// HD = 72 is the 80-wide geometry with a ragged last contraction step: 9 chunks per row in the same 12 slots (pad slots 9 .. 11 hold copies of chunks 5 .. 7), KS = 5, and
// step 4 covers columns 64 .. 79 of which 72 .. 79 do not exist.  Every contraction over the head dimension (q k^T, dO v^T, K q^T, V dO^T, and the D = rowsum(dO * O) sum)
// has exactly one own-row operand that comes from global: its upper half-wave does not issue the load of columns 72 .. 79 (they are the next head's, or lie outside the
// operand) and holds an exact zero there (ah_own_frag), so whatever the streamed side's slot 9 holds -- a copy of the row's own finite chunk 5 -- contributes exactly 0.
// The products whose output is HD wide still produce columns 72 .. 95 from copies; ah_store_tile drops everything from column HD on.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "vdk_device.h"
#include "vdk_host.h"
#include "vdk_internal.h"

#define AH_CT 2                            // 32-row tiles per chunk
#define AH_CROWS (32 * AH_CT)              // 64 rows: a multiple of 16, so the swizzle of a chunk-local row equals the one of the global row

template <int HD>
struct AhGeom {
  static_assert(HD % 8 == 0 && HD > 64 && HD <= 96, "attention_hd: head dimensions 72 .. 96 fit this layout");
  static constexpr int KS = (HD + 15) / 16;           // contraction steps of a 32x32x16 MFMA over the head dimension (HD % 16 == 8: the last one is half empty)
  static constexpr int CH = HD / 8;                   // 16-byte chunks of a row
  static constexpr int PCH = (CH + 3) & ~3;           // chunk slots of a staged row
  static constexpr int ROW = PCH * 16;                // bytes per staged row
  static constexpr int NDH = (HD + 31) / 32;          // 32-wide output blocks of a product whose output is HD wide
  static constexpr int ARR = AH_CROWS * ROW;          // one operand of one chunk
  static constexpr int BUF = 2 * ARR;                 // two operands
  static constexpr int BUFKV = BUF + 1024;            // ... | 128 lse values | 128 D values
  static constexpr int TROW = (CH | 1) * 16;          // bytes per row of a wave's store tile (an odd number of chunks)
  static constexpr int TILE = 32 * TROW;
};

__device__ __forceinline__ int ah_pos(int row, int c) { return (c & ~3) | ((c & 3) ^ ((row >> 2) & 3)); }

// rows [r0, r0 + 64) of two [N, HD] operands (row strides lda / ldb) -> buf, rows >= N read row N-1 (finite filler; its contribution is masked)
template <int HD>
__device__ __forceinline__ void ah_dma_chunk2(unsigned char* buf, const bf16_t* __restrict__ a, long lda, const bf16_t* __restrict__ b, long ldb, int N, int r0, int w, int lane) {
  typedef AhGeom<HD> G;
#pragma unroll
  for (int j0 = 0; j0 < G::PCH / 4; ++j0) {
    const int j = w + 4 * j0;                                       // instruction j fills slots [64 j, 64 j + 64) of the array
    const int slot = 64 * j + lane;
    const int lrow = slot / G::PCH, pos = slot - lrow * G::PCH;
    int c = ah_pos(lrow, pos);                                      // (the XOR is its own inverse: the chunk that lives in slot `pos`)
    c = c < G::CH ? c : c - 4;                                      // pad slots: a copy of a real chunk of the same row
    int srow = r0 + lrow;
    srow = srow < N ? srow : N - 1;
    __builtin_amdgcn_global_load_lds(VDK_GLOBAL_PTR(a + (long)srow * lda + c * 8), VDK_LDS_PTR(buf + j * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(VDK_GLOBAL_PTR(b + (long)srow * ldb + c * 8), VDK_LDS_PTR(buf + G::ARR + j * 1024), 16, 0, 0);
  }
}

// Lane-only parts of the fragment addresses (the swizzle looks at bits 2..3 of the row: for a tile that starts at a multiple of 16 rows it depends on the lane alone)
template <int HD>
struct AhLane { int row[AhGeom<HD>::KS]; int tr[AhGeom<HD>::NDH][2]; };
template <int HD>
__device__ __forceinline__ AhLane<HD> ah_lane(int lane) {
  typedef AhGeom<HD> G;
  AhLane<HD> a;
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) a.row[ks] = l31 * G::ROW + (ah_pos(l31, 2 * ks + hi) << 4);
  const int s = lane & 15, chalf = (lane >> 4) & 1;
  const int r1 = 4 * hi + (s >> 2), r2 = r1 + 8;
#pragma unroll
  for (int dh = 0; dh < G::NDH; ++dh) {
    const int byte = 64 * dh + 32 * chalf + 8 * (s & 3);
    a.tr[dh][0] = r1 * G::ROW + (ah_pos(r1, byte >> 4) << 4) + (byte & 8);
    a.tr[dh][1] = r2 * G::ROW + (ah_pos(r2, byte >> 4) << 4) + (byte & 8);
  }
  return a;
}
// own-row fragment from global: the 16 bytes at k = 16 ks + 8 hi of the row at `row`.  HD % 16 == 8: the upper half-wave of the last step takes an exact zero and issues
// no load (those bytes are not the head's)
template <int HD>
__device__ __forceinline__ s16x8 ah_own_frag(const bf16_t* __restrict__ row, int ks, int hi) {
  if (HD % 16 == 0 || ks < AhGeom<HD>::KS - 1 || hi == 0) return *(const s16x8*)(row + ks * 16 + hi * 8);
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return z;
}
// MFMA A/B fragment of the 32-row tile at `tile`: lane (row, hi) -> the 16 bytes at k = 16 ks + 8 hi
template <int HD>
__device__ __forceinline__ s16x8 ah_row_frag(const unsigned char* tile, const AhLane<HD>& a, int ks) { return *(const s16x8*)(tile + a.row[ks]); }
// transposed fragment of the 16 rows at `tile`, columns 32 dh + (lane & 31): rows 4 hi + {0..3} in slots 0..3 and the same + 8 in slots 4..7 (the permuted contraction
// order that makes an MFMA C-layout tile directly usable as the other operand, see attention.hip)
template <int HD>
__device__ __forceinline__ s16x8 ah_tr_frag(const unsigned char* tile, const AhLane<HD>& a, int dh) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(tile + a.tr[dh][0]));
  s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16(VDK_LDS_S16X4(tile + a.tr[dh][1]));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
  return r;
}
__device__ __forceinline__ f32x16 ah_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
// 16 C-layout values -> the two B-operand fragments (k-slot j of step s <-> accumulator register 8*s + j)
template <int OF>
__device__ __forceinline__ void ah_pack_b(const f32x16& p, s16x8 (&f)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    u32x4 u = {pack_op2<OF>(p[8 * s + 0], p[8 * s + 1]), pack_op2<OF>(p[8 * s + 2], p[8 * s + 3]), pack_op2<OF>(p[8 * s + 4], p[8 * s + 5]), pack_op2<OF>(p[8 * s + 6], p[8 * s + 7])};
    f[s] = *(s16x8*)&u;
  }
}
// a wave's 32 x HD output tile (C-layout of a transposed product: lane = row, register 4 g + e of block k = column 32 k + 8 g + 4 hi + e) -> its private LDS tile ->
// coalesced global rows of HD * 2 bytes.  Columns >= HD (the copies) are dropped here.
template <int OF, int HD>
__device__ __forceinline__ void ah_store_tile(unsigned char* tile, const f32x16 (&x)[AhGeom<HD>::NDH], float mul, bf16_t* __restrict__ dst, long ld, int row0, int N, int lane) {
  typedef AhGeom<HD> G;
  const int l31 = lane & 31, hi = lane >> 5;
  if (row0 + l31 < N) {
#pragma unroll
    for (int k = 0; k < G::NDH; ++k)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (32 * k + 8 * g < HD)
          *(u32x2*)(tile + l31 * G::TROW + ((4 * k + g) << 4) + 8 * hi) =
              (u32x2){pack_op2<OF>(x[k][4 * g] * mul, x[k][4 * g + 1] * mul), pack_op2<OF>(x[k][4 * g + 2] * mul, x[k][4 * g + 3] * mul)};
  }
  VDK_WAVE_LDS_SYNC();
#pragma unroll
  for (int p = 0; p < (32 * G::CH + 63) / 64; ++p) {
    const int idx = 64 * p + lane;
    const int r = idx / G::CH, cp = idx - r * G::CH;
    if (idx < 32 * G::CH && row0 + r < N) {
      const u32x4 v = *(const u32x4*)(tile + r * G::TROW + (cp << 4));
      *(u32x4*)(dst + (long)(row0 + r) * ld + cp * 8) = v;
    }
  }
  VDK_WAVE_LDS_SYNC();
}

// LDS (dynamic): chunk buffer 0 | chunk buffer 1 | 4 wave store tiles
template <int OF, int HD>
__global__ __launch_bounds__(256, 2) void attn_h_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                            bf16_t* __restrict__ o, long ldo, float* __restrict__ lse, int N, int H, float scale, int nitems, int G) {
  typedef AhGeom<HD> GE;
  VDK_DYN_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* const Wt = smem + 2 * GE::BUF + w * GE::TILE;
  const int nt = (N + 31) >> 5, nch = (N + AH_CROWS - 1) / AH_CROWS;
  const float scale2 = scale * VDK_LOG2E;
  const AhLane<HD> al = ah_lane<HD>(lane);
  // unit t of XCD x: item (t / G) * 8 + x, query-tile group t % G; this workgroup walks t = blockIdx / 8, + gridDim / 8, ...
  const int x = blockIdx.x & 7, tstride = gridDim.x >> 3;
  int t = blockIdx.x >> 3;
  int item = (t / G) * 8 + x;
  int cc = 0;                                                        // chunks consumed so far: buffer parity runs on across units
  if (item < nitems) {
    const long off0 = (long)(item / H) * N * ld + (item % H) * HD;
    ah_dma_chunk2<HD>(smem, k + off0, ld, v + off0, ld, N, 0, w, lane);
  }
  while (item < nitems) {
    const int g = t % G;
    const int b = item / H, h = item - b * H;
    const long off = (long)b * N * ld + h * HD;
    const int qt = 4 * g + w;
    const bool active = qt < nt;                                     // (wave-uniform) the last group of an item may be short; idle waves still load and meet the barriers
    const int qrow = qt * 32 + l31;
    const int qr = qrow < N ? qrow : N - 1;
    s16x8 qf[GE::KS];
#pragma unroll
    for (int ks = 0; ks < GE::KS; ++ks) qf[ks] = ah_own_frag<HD>(q + off + (long)qr * ld, ks, hi);
    const int tn = t + tstride;
    const int itemn = (tn / G) * 8 + x;
    const long offn = (long)(itemn / H) * N * ld + (itemn % H) * HD;
    float m = -INFINITY, l = 0.f;                                    // running maximum (log2 domain, scaled) and this half-wave's part of the row sum
    f32x16 oa[GE::NDH];
#pragma unroll
    for (int dh = 0; dh < GE::NDH; ++dh) oa[dh] = ah_zero16();
    for (int c = 0; c < nch; ++c, ++cc) {
      __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0): this wave's part of chunk cc has landed (and its Q fragments)
      __syncthreads();                                               // everybody's part has; everybody is done with chunk cc - 1, whose buffer the next request overwrites
      unsigned char* const nb = smem + ((cc + 1) & 1) * GE::BUF;
      if (c + 1 < nch) ah_dma_chunk2<HD>(nb, k + off, ld, v + off, ld, N, (c + 1) * AH_CROWS, w, lane);
      else if (itemn < nitems) ah_dma_chunk2<HD>(nb, k + offn, ld, v + offn, ld, N, 0, w, lane);
      if (!active) continue;
      const unsigned char* const Kb = smem + (cc & 1) * GE::BUF;
      const unsigned char* const Vb = Kb + GE::ARR;
      const int key0 = c * AH_CROWS;
      const int nv = (N - key0 + 31) >> 5;                            // key tiles of this chunk that hold a valid key (wave-uniform; >= AH_CT except in the last chunk)
      f32x16 st[AH_CT];
#pragma unroll
      for (int kt = 0; kt < AH_CT; ++kt) {
        st[kt] = ah_zero16();
        if (kt < nv) {
#pragma unroll
          for (int ks = 0; ks < GE::KS; ++ks) st[kt] = vdk_mfma32<OF>(ah_row_frag<HD>(Kb + kt * 32 * GE::ROW, al, ks), qf[ks], st[kt]);
        }
      }
      if (key0 + AH_CROWS > N) {                                     // the last chunk holds keys beyond N (wave-uniform)
#pragma unroll
        for (int kt = 0; kt < AH_CT; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (key0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= N) st[kt][r] = -INFINITY;
      }
      float mt = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < AH_CT; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, st[kt][r]);
      mt = fmaxf(mt, __shfl_xor(mt, 32));                            // the two half-waves hold the same queries, different keys
      const float mt2 = mt * scale2;
      // deferred rescale: keep the old maximum while the chunk exceeds it by < 2^8; P is then bounded by 2^8 instead of 1 (harmless in 16 bits / fp32).  The first chunk
      // always takes the branch (m = -inf): alpha = 0 on zero accumulators.  Every chunk-0 row has a valid key, so the new maximum is finite.
      if (__any(mt2 > m + 8.0f)) {
        const float mn = fmaxf(m, mt2);
        const float alpha = fast_exp2(m - mn);
        l *= alpha;
        m = mn;
#pragma unroll
        for (int dh = 0; dh < GE::NDH; ++dh)
#pragma unroll
          for (int r = 0; r < 16; ++r) oa[dh][r] *= alpha;
      }
#pragma unroll
      for (int kt = 0; kt < AH_CT; ++kt) {
        if (kt >= nv) break;                                         // nothing but masked keys: P = 0
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float p = fast_exp2(fmaf(st[kt][r], scale2, -m)); st[kt][r] = p; l += p; }
        s16x8 pf[2];
        ah_pack_b<OF>(st[kt], pf);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int dh = 0; dh < GE::NDH; ++dh) oa[dh] = vdk_mfma32<OF>(ah_tr_frag<HD>(Vb + (kt * 32 + 16 * s) * GE::ROW, al, dh), pf[s], oa[dh]);
      }
    }
    if (active) {
      l += __shfl_xor(l, 32);
      ah_store_tile<OF, HD>(Wt, oa, 1.0f / l, o + (long)b * N * ldo + h * HD, ldo, qt * 32, N, lane);
      if (lse && hi == 0 && qrow < N) lse[((long)b * H + h) * N + qrow] = (m + log2f(l)) * 0.6931471805599453f;
    }
    t = tn;
    item = itemn;
  }
}

// =====================================================================================  backward
//   q kernel:  unit = (b, head, group of 4 query tiles); Q / dO / O fragments from global, K / V chunks through the double buffer, dQ^T (lane = query) in registers.  It also
//              computes D = rowsum(dO * O) for its query tile (it holds the dO fragments) and writes it to `dvec` for the kv kernel.
//   kv kernel: unit = (b, head, group of 4 key tiles); K / V fragments from global, Q / dO chunks through the double buffer together with the chunk's lse and D values
//              (staged through one register per thread: loaded under the previous chunk, written to LDS before the chunk's barrier); dK^T, dV^T (lane = key) in registers.
template <int OF, int HD>
__global__ __launch_bounds__(256, 2) void attn_h_bwd_q_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                              const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse,
                                                              float* __restrict__ dvec, bf16_t* __restrict__ dq, long ldd, int N, int H, float scale, int nitems, int G) {
  typedef AhGeom<HD> GE;
  VDK_DYN_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* const Wt = smem + 2 * GE::BUF + w * GE::TILE;
  const int nt = (N + 31) >> 5, nch = (N + AH_CROWS - 1) / AH_CROWS;
  const float scale2 = scale * VDK_LOG2E;
  const AhLane<HD> al = ah_lane<HD>(lane);
  const int x = blockIdx.x & 7, tstride = gridDim.x >> 3;
  int t = blockIdx.x >> 3;
  int item = (t / G) * 8 + x;
  int cc = 0;
  if (item < nitems) {
    const long off0 = (long)(item / H) * N * ld + (item % H) * HD;
    ah_dma_chunk2<HD>(smem, k + off0, ld, v + off0, ld, N, 0, w, lane);
  }
  while (item < nitems) {
    const int g = t % G;
    const int b = item / H, h = item - b * H;
    const long off = (long)b * N * ld + h * HD, offo = (long)b * N * ldo + h * HD;
    const int qt = 4 * g + w;
    const bool active = qt < nt;
    const int qrow = qt * 32 + l31;
    const int qr = qrow < N ? qrow : N - 1;
    s16x8 qf[GE::KS], gf[GE::KS];
    float dsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < GE::KS; ++ks) {
      qf[ks] = ah_own_frag<HD>(q + off + (long)qr * ld, ks, hi);
      gf[ks] = ah_own_frag<HD>(dout + offo + (long)qr * ldo, ks, hi);
      const s16x8 os = ah_own_frag<HD>(o + offo + (long)qr * ldo, ks, hi);
      const u32x4 of = *(const u32x4*)&os;
      const u32x4 gu = *(const u32x4*)&gf[ks];
#pragma unroll
      for (int e = 0; e < 4; ++e) { dsum = fmaf(op_lo<OF>(gu[e]), op_lo<OF>(of[e]), dsum); dsum = fmaf(op_hi<OF>(gu[e]), op_hi<OF>(of[e]), dsum); }
    }
    dsum += __shfl_xor(dsum, 32);                                    // the two half-waves hold the two halves of every 16 channels of a query
    const float lq = lse[((long)b * H + h) * N + qr] * VDK_LOG2E;
    if (active && hi == 0 && qrow < N) dvec[((long)b * H + h) * N + qrow] = dsum;
    const int tn = t + tstride;
    const int itemn = (tn / G) * 8 + x;
    const long offn = (long)(itemn / H) * N * ld + (itemn % H) * HD;
    f32x16 gq[GE::NDH];
#pragma unroll
    for (int dh = 0; dh < GE::NDH; ++dh) gq[dh] = ah_zero16();
    for (int c = 0; c < nch; ++c, ++cc) {
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
      unsigned char* const nb = smem + ((cc + 1) & 1) * GE::BUF;
      if (c + 1 < nch) ah_dma_chunk2<HD>(nb, k + off, ld, v + off, ld, N, (c + 1) * AH_CROWS, w, lane);
      else if (itemn < nitems) ah_dma_chunk2<HD>(nb, k + offn, ld, v + offn, ld, N, 0, w, lane);
      if (!active) continue;
      const unsigned char* const Kb = smem + (cc & 1) * GE::BUF;
      const unsigned char* const Vb = Kb + GE::ARR;
      const int key0 = c * AH_CROWS;
      const bool edge = key0 + AH_CROWS > N;                         // keys beyond N in this chunk (wave-uniform); a lane (= query) beyond N only spoils its own, unstored column
#pragma unroll 1
      for (int kt = 0; kt < AH_CT; ++kt) {
        if (key0 + kt * 32 >= N) break;                              // a tile of nothing but keys beyond N (wave-uniform)
        f32x16 st = ah_zero16(), dp = ah_zero16();
#pragma unroll
        for (int ks = 0; ks < GE::KS; ++ks) {
          st = vdk_mfma32<OF>(ah_row_frag<HD>(Kb + kt * 32 * GE::ROW, al, ks), qf[ks], st);   // S^T[key][q]: lane = query, registers = keys
          dp = vdk_mfma32<OF>(ah_row_frag<HD>(Vb + kt * 32 * GE::ROW, al, ks), gf[ks], dp);   // dP^T[key][q]
        }
        f32x16 ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = fast_exp2(fmaf(st[r], scale2, -lq));
          if (edge && key0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= N) p = 0.f;
          ds[r] = p * (dp[r] - dsum);
        }
        s16x8 df[2];
        ah_pack_b<OF>(ds, df);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dh = 0; dh < GE::NDH; ++dh) gq[dh] = vdk_mfma32<OF>(ah_tr_frag<HD>(Kb + (kt * 32 + 16 * s2) * GE::ROW, al, dh), df[s2], gq[dh]);   // dQ^T[d][q] += K^T dS^T
      }
    }
    if (active) ah_store_tile<OF, HD>(Wt, gq, scale, dq + (long)b * N * ldd + h * HD, ldd, qt * 32, N, lane);
    t = tn;
    item = itemn;
  }
}

template <int OF, int HD>
__global__ __launch_bounds__(256, 2) void attn_h_bwd_kv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld,
                                                               const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse, const float* __restrict__ dvec,
                                                               bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, long ldd, int N, int H, float scale, int nitems, int G) {
  typedef AhGeom<HD> GE;
  VDK_DYN_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* const Wt = smem + 2 * GE::BUFKV + w * GE::TILE;
  const int nt = (N + 31) >> 5, nch = (N + AH_CROWS - 1) / AH_CROWS;
  const float scale2 = scale * VDK_LOG2E;
  const AhLane<HD> al = ah_lane<HD>(lane);
  const int x = blockIdx.x & 7, tstride = gridDim.x >> 3;
  int t = blockIdx.x >> 3;
  int item = (t / G) * 8 + x;
  int cc = 0;
  // thread tid < 128 stages lse value tid of a chunk, thread 128 + i the D value i (64 of each are used)
  const int srow_l = tid & 127;
  float staged = 0.f;
  auto stage_load = [&](int it, int r0) {
    int row = r0 + srow_l;
    row = row < N ? row : N - 1;
    const float* src = tid < 128 ? lse : dvec;
    staged = src[(long)it * N + row];
  };
  if (item < nitems) {
    const long off0 = (long)(item / H) * N * ld + (item % H) * HD, offo0 = (long)(item / H) * N * ldo + (item % H) * HD;
    ah_dma_chunk2<HD>(smem, q + off0, ld, dout + offo0, ldo, N, 0, w, lane);
    stage_load(item, 0);
  }
  while (item < nitems) {
    const int g = t % G;
    const int b = item / H, h = item - b * H;
    const long off = (long)b * N * ld + h * HD, offo = (long)b * N * ldo + h * HD;
    const int kt = 4 * g + w;
    const bool active = kt < nt;
    const int krow = kt * 32 + l31;
    const long kr = (long)(krow < N ? krow : N - 1) * ld;
    s16x8 kf[GE::KS], vf[GE::KS];
#pragma unroll
    for (int ks = 0; ks < GE::KS; ++ks) { kf[ks] = ah_own_frag<HD>(k + off + kr, ks, hi); vf[ks] = ah_own_frag<HD>(v + off + kr, ks, hi); }
    const int tn = t + tstride;
    const int itemn = (tn / G) * 8 + x;
    const long offn = (long)(itemn / H) * N * ld + (itemn % H) * HD, offon = (long)(itemn / H) * N * ldo + (itemn % H) * HD;
    f32x16 gk[GE::NDH], gv[GE::NDH];
#pragma unroll
    for (int dh = 0; dh < GE::NDH; ++dh) { gk[dh] = ah_zero16(); gv[dh] = ah_zero16(); }
    for (int c = 0; c < nch; ++c, ++cc) {
      __builtin_amdgcn_s_waitcnt(0x0F70);                            // this wave's part of chunk cc has landed, and so has its staged lse / D value
      ((float*)(smem + (cc & 1) * GE::BUFKV + GE::BUF))[tid] = staged;  // (buffer cc & 1 was last read in chunk cc - 2: everybody is past that since the previous barrier)
      __syncthreads();
      unsigned char* const nb = smem + ((cc + 1) & 1) * GE::BUFKV;
      if (c + 1 < nch) { ah_dma_chunk2<HD>(nb, q + off, ld, dout + offo, ldo, N, (c + 1) * AH_CROWS, w, lane); stage_load(item, (c + 1) * AH_CROWS); }
      else if (itemn < nitems) { ah_dma_chunk2<HD>(nb, q + offn, ld, dout + offon, ldo, N, 0, w, lane); stage_load(itemn, 0); }
      if (!active) continue;
      const unsigned char* const Qb = smem + (cc & 1) * GE::BUFKV;
      const unsigned char* const Ob = Qb + GE::ARR;
      const float* const lseb = (const float*)(Qb + GE::BUF);
      const float* const Db = lseb + 128;
      const int q0c = c * AH_CROWS;
      const bool edge = q0c + AH_CROWS > N;                          // query rows beyond N in this chunk must be silenced (they would add into valid sums); wave-uniform
#pragma unroll 1
      for (int qt = 0; qt < AH_CT; ++qt) {
        if (q0c + qt * 32 >= N) break;                               // a tile of nothing but query rows beyond N (wave-uniform)
        // S, P and dV first, then dP, dS and dK: P's 16-bit copy and the dP accumulator are never live together (the accumulators already take 96 registers)
        f32x16 pv = ah_zero16();
#pragma unroll
        for (int ks = 0; ks < GE::KS; ++ks) pv = vdk_mfma32<OF>(ah_row_frag<HD>(Qb + qt * 32 * GE::ROW, al, ks), kf[ks], pv);   // S[q][key]: lane = key, registers = queries
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 lv = *(const f32x4*)(lseb + qt * 32 + 8 * g4 + 4 * hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g4 + e;
            float p = fast_exp2(fmaf(pv[r], scale2, -lv[e] * VDK_LOG2E));
            if (edge && q0c + qt * 32 + 8 * g4 + 4 * hi + e >= N) p = 0.f;
            pv[r] = p;
          }
        }
        {
          s16x8 pf[2];
          ah_pack_b<OF>(pv, pf);
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int dh = 0; dh < GE::NDH; ++dh) gv[dh] = vdk_mfma32<OF>(ah_tr_frag<HD>(Ob + (qt * 32 + 16 * s2) * GE::ROW, al, dh), pf[s2], gv[dh]);     // dV^T[d][key] += dO^T P
        }
        f32x16 ds = ah_zero16();
#pragma unroll
        for (int ks = 0; ks < GE::KS; ++ks) ds = vdk_mfma32<OF>(ah_row_frag<HD>(Ob + qt * 32 * GE::ROW, al, ks), vf[ks], ds);   // dP[q][key]
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 dd = *(const f32x4*)(Db + qt * 32 + 8 * g4 + 4 * hi);
#pragma unroll
          for (int e = 0; e < 4; ++e) ds[4 * g4 + e] = pv[4 * g4 + e] * (ds[4 * g4 + e] - dd[e]);
        }
        s16x8 df[2];
        ah_pack_b<OF>(ds, df);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dh = 0; dh < GE::NDH; ++dh) gk[dh] = vdk_mfma32<OF>(ah_tr_frag<HD>(Qb + (qt * 32 + 16 * s2) * GE::ROW, al, dh), df[s2], gk[dh]);     // dK^T[d][key] += Q^T dS
      }
    }
    if (active) {
      ah_store_tile<OF, HD>(Wt, gk, scale, dk + (long)b * N * ldd + h * HD, ldd, kt * 32, N, lane);
      ah_store_tile<OF, HD>(Wt, gv, 1.0f, dv + (long)b * N * ldd + h * HD, ldd, kt * 32, N, lane);
    }
    t = tn;
    item = itemn;
  }
}

static int ah_grid(long units) {
  int cap = 512;                                                     // two workgroups per CU
  if (const char* e = getenv("VDK_ATTN_GRID")) { const int v = atoi(e); if (v > 0) cap = v; }   // tests: force several units per workgroup
  long grid = units < cap ? units : cap;
  return (int)((grid + 7) / 8 * 8);                                  // every XCD residue must be present: items are dealt to XCDs by item mod 8
}

template <int OF, int HD>
static int ah_launch_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, float scale, void* stream) {
  typedef AhGeom<HD> GE;
  const bf16_t* base = (const bf16_t*)qkv;
  const long D = (long)H * HD;
  const int nt = (N + 31) / 32, G = (nt + 3) / 4;
  const int grid = ah_grid((long)B * H * G);
  const size_t lds = 2 * GE::BUF + 4 * GE::TILE;
  if (hipFuncSetAttribute((const void*)attn_h_fwd_kernel<OF, HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return vdk_fail(VDK_ELAUNCH, "vdk_attention_fwd: LDS attribute");
  hipLaunchKernelGGL((attn_h_fwd_kernel<OF, HD>), dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, base, base + D, base + 2 * D, (long)ld, (bf16_t*)o, (long)ldo, lse, (int)N,
                     (int)H, scale, (int)(B * H), G);
  return VDK_OK;
}
// dqkv: [B, N, 3, H, HD] like qkv; dvec: f32 scratch [B, H, N]
template <int OF, int HD>
static int ah_launch_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t ldd, float* dvec, int32_t B, int32_t N,
                         int32_t H, float scale, void* stream) {
  typedef AhGeom<HD> GE;
  const bf16_t* base = (const bf16_t*)qkv;
  bf16_t* dbase = (bf16_t*)dqkv;
  const long D = (long)H * HD;
  const int nt = (N + 31) / 32, G = (nt + 3) / 4;
  const int grid = ah_grid((long)B * H * G);
  const size_t lds_q = 2 * GE::BUF + 4 * GE::TILE, lds_kv = 2 * GE::BUFKV + 4 * GE::TILE;
  if (hipFuncSetAttribute((const void*)attn_h_bwd_q_kernel<OF, HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_q) != hipSuccess ||
      hipFuncSetAttribute((const void*)attn_h_bwd_kv_kernel<OF, HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_kv) != hipSuccess)
    return vdk_fail(VDK_ELAUNCH, "vdk_attention_bwd: LDS attribute");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL((attn_h_bwd_q_kernel<OF, HD>), dim3((unsigned)grid), dim3(256), lds_q, s, base, base + D, base + 2 * D, (long)ld, (const bf16_t*)o, (const bf16_t*)dout, (long)ldo, lse,
                     dvec, dbase, (long)ldd, (int)N, (int)H, scale, (int)(B * H), G);
  hipLaunchKernelGGL((attn_h_bwd_kv_kernel<OF, HD>), dim3((unsigned)grid), dim3(256), lds_kv, s, base, base + D, base + 2 * D, (long)ld, (const bf16_t*)dout, (long)ldo, lse,
                     (const float*)dvec, dbase + D, dbase + 2 * D, (long)ldd, (int)N, (int)H, scale, (int)(B * H), G);
  return VDK_OK;
}

// in-library entry points (attention.hip routes head_dim == 80 here, the ViT engine head_dim == 72 as well); any other head_dim: VDK_EUNSUPPORTED
int vdk_attention_hd_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int opf, void* stream) {
  if (head_dim == 80)
    return opf ? ah_launch_fwd<VDK_OPF_F16, 80>(qkv, ld, o, ldo, lse, B, N, H, scale, stream) : ah_launch_fwd<VDK_OPF_BF16, 80>(qkv, ld, o, ldo, lse, B, N, H, scale, stream);
  if (head_dim == 72)
    return opf ? ah_launch_fwd<VDK_OPF_F16, 72>(qkv, ld, o, ldo, lse, B, N, H, scale, stream) : ah_launch_fwd<VDK_OPF_BF16, 72>(qkv, ld, o, ldo, lse, B, N, H, scale, stream);
  return VDK_EUNSUPPORTED;
}
int vdk_attention_hd_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t ldd, float* dvec, int32_t B, int32_t N,
                         int32_t H, int32_t head_dim, float scale, int opf, void* stream) {
  if (head_dim == 80)
    return opf ? ah_launch_bwd<VDK_OPF_F16, 80>(qkv, ld, o, dout, ldo, lse, dqkv, ldd, dvec, B, N, H, scale, stream)
               : ah_launch_bwd<VDK_OPF_BF16, 80>(qkv, ld, o, dout, ldo, lse, dqkv, ldd, dvec, B, N, H, scale, stream);
  if (head_dim == 72)
    return opf ? ah_launch_bwd<VDK_OPF_F16, 72>(qkv, ld, o, dout, ldo, lse, dqkv, ldd, dvec, B, N, H, scale, stream)
               : ah_launch_bwd<VDK_OPF_BF16, 72>(qkv, ld, o, dout, ldo, lse, dqkv, ldd, dvec, B, N, H, scale, stream);
  return VDK_EUNSUPPORTED;
}

extern "C" {

// vdk_internal.h: the kernels of this file behind the argument lists of vdk_attention_fwd_dt / vdk_attention_bwd_dt, for the kernel-level tests and tools/bench_attention.py
// (the public entries keep refusing head_dim 72; the ViT engine reaches it in-library)
int vdk_debug_attention_hd_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype,
                               void* stream) {
  if (!qkv || !o || B <= 0 || N <= 0 || H <= 0 || (dtype != VDK_BF16 && dtype != VDK_F16)) return vdk_fail(VDK_EINVAL, "vdk_debug_attention_hd_fwd: bad argument");
  if (head_dim != 72 && head_dim != 80) return vdk_fail(VDK_EUNSUPPORTED, "vdk_debug_attention_hd_fwd: head_dim must be 72 or 80");
  if ((ld & 7) || (ldo & 7) || ld < 3L * H * head_dim || ldo < (long)H * head_dim) return vdk_fail(VDK_EINVAL, "vdk_debug_attention_hd_fwd: ld % 8, ld >= 3 * H * head_dim");
  const int rc = vdk_attention_hd_fwd(qkv, ld, o, ldo, lse, B, N, H, head_dim, scale, dtype == VDK_F16 ? VDK_OPF_F16 : VDK_OPF_BF16, stream);
  return rc ? rc : vdk_check_launch("vdk_debug_attention_hd_fwd");
}
int vdk_debug_attention_hd_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t lddqkv, float* dvec, int32_t B,
                               int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype, void* stream) {
  if (!qkv || !o || !dout || !lse || !dqkv || !dvec || B <= 0 || N <= 0 || H <= 0 || (dtype != VDK_BF16 && dtype != VDK_F16))
    return vdk_fail(VDK_EINVAL, "vdk_debug_attention_hd_bwd: bad argument");
  if (head_dim != 72 && head_dim != 80) return vdk_fail(VDK_EUNSUPPORTED, "vdk_debug_attention_hd_bwd: head_dim must be 72 or 80");
  if ((ld & 7) || (ldo & 7) || (lddqkv & 7) || ld < 3L * H * head_dim || lddqkv < 3L * H * head_dim || ldo < (long)H * head_dim)
    return vdk_fail(VDK_EINVAL, "vdk_debug_attention_hd_bwd: ld % 8, ld >= 3 * H * head_dim");
  const int rc = vdk_attention_hd_bwd(qkv, ld, o, dout, ldo, lse, dqkv, lddqkv, dvec, B, N, H, head_dim, scale, dtype == VDK_F16 ? VDK_OPF_F16 : VDK_OPF_BF16, stream);
  return rc ? rc : vdk_check_launch("vdk_debug_attention_hd_bwd");
}

}  // extern "C"

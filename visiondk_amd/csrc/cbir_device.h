// cbir_device.h -- device helpers of hot path B shared by cbir.hip (top-k search) and cbir_range.hip (range search): the exact k-ordered fmaf chain over fp32 and
// fp16 gallery rows, and the pre-filter's error band eps_q.  One definition, so both searches score and bound every pair with the same instructions.
#pragma once
#include "vdk_device.h"

// the oracle's score of one pair: k-ordered fmaf chain from +0 (oracle/cbir_oracle.c oracle_ip_pair), loads batched 8 deep
__device__ __forceinline__ float cbir_exact_ip(const float* __restrict__ qrow, const float* __restrict__ g, int D) {
  float acc = 0.f;
  int c = 0;
  for (; c + 32 <= D; c += 32) {
    f32x4 gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[j] = *(const f32x4*)(g + c + 4 * j);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 qv = *(const f32x4*)(qrow + c + 4 * j);
      acc = fmaf(qv[0], gv[j][0], acc); acc = fmaf(qv[1], gv[j][1], acc); acc = fmaf(qv[2], gv[j][2], acc); acc = fmaf(qv[3], gv[j][3], acc);
    }
  }
  for (; c < D; c += 4) {
    const f32x4 gv = *(const f32x4*)(g + c);
    const f32x4 qv = *(const f32x4*)(qrow + c);
    acc = fmaf(qv[0], gv[0], acc); acc = fmaf(qv[1], gv[1], acc); acc = fmaf(qv[2], gv[2], acc); acc = fmaf(qv[3], gv[3], acc);
  }
  return acc + 0.0f;
}

// the same chain over a gallery row STORED in fp16 (faiss GpuClonerOptions.useFloat16, engine/cbir/evaluation.py:157-162): every element converts exactly to
// fp32, so the score equals cbir_exact_ip on the fp16-rounded row
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float cbir_exact_ip_h(const float* __restrict__ qrow, const _Float16* __restrict__ g, int D) {
  float acc = 0.f;
  int c = 0;
  for (; c + 64 <= D; c += 64) {          // loads batched 8 deep like the fp32 chain (the chain itself is latency-bound, the loads must not be)
    f16x8_t gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[j] = *(const f16x8_t*)(g + c + 8 * j);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 q0 = *(const f32x4*)(qrow + c + 8 * j), q1 = *(const f32x4*)(qrow + c + 8 * j + 4);
      acc = fmaf(q0[0], (float)gv[j][0], acc); acc = fmaf(q0[1], (float)gv[j][1], acc); acc = fmaf(q0[2], (float)gv[j][2], acc); acc = fmaf(q0[3], (float)gv[j][3], acc);
      acc = fmaf(q1[0], (float)gv[j][4], acc); acc = fmaf(q1[1], (float)gv[j][5], acc); acc = fmaf(q1[2], (float)gv[j][6], acc); acc = fmaf(q1[3], (float)gv[j][7], acc);
    }
  }
  for (; c + 8 <= D; c += 8) {
    const f16x8_t gv = *(const f16x8_t*)(g + c);
    const f32x4 q0 = *(const f32x4*)(qrow + c), q1 = *(const f32x4*)(qrow + c + 4);
    acc = fmaf(q0[0], (float)gv[0], acc); acc = fmaf(q0[1], (float)gv[1], acc); acc = fmaf(q0[2], (float)gv[2], acc); acc = fmaf(q0[3], (float)gv[3], acc);
    acc = fmaf(q1[0], (float)gv[4], acc); acc = fmaf(q1[1], (float)gv[5], acc); acc = fmaf(q1[2], (float)gv[6], acc); acc = fmaf(q1[3], (float)gv[7], acc);
  }
  for (; c < D; ++c) acc = fmaf(qrow[c], (float)g[c], acc);
  return acc + 0.0f;
}
// G: fp32 rows, or fp16 rows when g_half
__device__ __forceinline__ float cbir_exact_ip_any(const float* __restrict__ qrow, const float* __restrict__ G, long row, int D, int g_half) {
  return g_half ? cbir_exact_ip_h(qrow, (const _Float16*)G + row * (long)D, D) : cbir_exact_ip(qrow, G + row * (long)D, D);
}

// eps_q of the header comment
// (the accumulation term scales with the contraction length: 4e-5 covers 128 terms with a 5x margin, gstat_bits[3] holds DP / 128)
__device__ __forceinline__ float cbir_eps(const float* __restrict__ qn3, long q, const unsigned* __restrict__ gstat_bits) {
  const float gt = __uint_as_float(gstat_bits[1]), ge = __uint_as_float(gstat_bits[2]);
  const float qn = qn3[q * 3], qt = qn3[q * 3 + 1], qe = qn3[q * 3 + 2];
  const float len = gstat_bits[3] > 1u ? (float)gstat_bits[3] : 1.0f;
  return 1.00001f * (qe * gt + qn * ge) + 4e-5f * len * qt * gt;
}

// in-library (C++ linkage, defined in cbir.hip): xb = bf16 [n, DP] zero-padded copy of x [n, D], norms3[row] = (||x||, ||bf16(x)||, ||bf16(x) - x||) rounded up
// (cbir_cast_rows_kernel, the cast vdk_cbir_search_fast2 applies to its queries)
void vdk_cbir_cast_rows(const float* x, long n, int D, int DP, bf16_t* xb, float* norms3, void* stream);

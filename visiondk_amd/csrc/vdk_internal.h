// vdk_internal.h -- tuning / debug / test knobs of libvisiondk_hip.so.  NOT part of the ABI a host binds (include/visiondk.h): these exist for the repository's own tests, A/B
// tools (tools/) and profiling; they may change between builds.  visiondk_amd/_abi.py binds them from its INTERNAL table.
#pragma once
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
int vdk_gemm_streamk_grid(int32_t workgroups);   /* tests / tuning: persistent workgroups of the stream-K launch (multiple of 8; 0 = one per CU) */
/* tests / A-B benchmarking only: 0 = automatic choice, 1 = 128x128 register-staged kernel, 2 = 256x256 LDS-DMA kernel
 * (the latter still requires K and the split size to be multiples of 64), 3 = stream-K whenever splitk == -1 lends a workspace, 4 = never stream-K. */
int vdk_gemm_force_kernel(int32_t which);
int vdk_gemm_force_band_cw(int32_t cw);   /* tests: tile order of the one-wave-per-SIMD kernels in column bands of cw tile columns (-1: decided by size, the default) */
/* tests / tuning: which structure served the calling thread's last vdk_gemm_bf16_nt / vdk_margin_cos_pass: 1 = 128x128 register-staged, 2 = 256x256 eight waves,
 * 3 = its stream-K form, 5 = 256x256 four waves (one per SIMD, persistent; gemm_w4.hip; the default for big problems; which = 5 forces it wherever it can
 * serve, environment VDK_GEMM_W4=0 disables it), 6 = 256x128 four waves with two workgroups per CU (gemm_w4h_kernel: the default for the long epilogues --
 * GELU, dGELU, fp32 residual; which = 6 forces it; environment VDK_GEMM_W4H = bit mask 1 GELU | 2 dGELU | 4 residual | 8 other NT | 16 TN) */
int vdk_gemm_last_kernel(void);
/* diagnostic: `workgroups` workgroups (256 threads, 32 KB of LDS) that stay resident for `microseconds` on `stream` -- a stand-in for a collective's kernel in flight */
int vdk_debug_occupy_cus(int32_t workgroups, int64_t microseconds, void* stream);
/* profiling aid: when non-NULL, every 256x256 workgroup writes 4 shader-cycle stamps (start, operands landed, main loop done,
 * stores issued) to buf[4 * workgroup]; NULL (default) disables it */
int vdk_gemm_debug_stamps(void* device_u64_buffer);
/* 1: route every attention call of this thread to the flash-style kernels of csrc/attention.hip (bf16 only), 0: never, -1: environment VDK_ATTN_LEGACY (tests, A/B) */
int vdk_attention_force_legacy(int32_t on);
/* tests: one job of the batched row reduction (vdk_reduce_rows_batch) */
int vdk_debug_reduce_rows_job(float* buf, int64_t ld, int32_t S, int64_t n, float* out, float scale, void* stream);
/* TEST-ONLY (tests/test_layernorm_forms.py): the forms of the LayerNorm backward that only the engines reach (csrc/norm_loss.hip, vdk_layernorm_bwd_deferred).  The first 21
 * arguments are those of vdk_layernorm_bwd; then dxb_colsum f32 [C] or NULL (column sums of the stored dxb); the fp8 copy of dxb: out8 [T, ldo8] bytes or NULL (= none), fmt
 * 0 = e4m3 / 1 = e5m2, scale and amax f32 device scalars; opf = format of dxb for an fp32 dy (0 = bf16, 1 = fp16); dy_scale f32 device scalar or NULL; dxb_rs f32
 * [ceil(T / dxb_rps)] or NULL (factor of the 16-bit copy only); dres16 = the residual gradient as fp16 rows (pitch lddres) or NULL; deferred != 0: the dgamma | dbeta reduction
 * is left to the caller's job.  Everything is forwarded unchanged and the jobs that come back run in ONE vdk_reduce_rows_batch; a refusal of the callee is returned as it is.
 * ws: vdk_layernorm_bwd_workspace_bytes(T, C). */
int vdk_debug_layernorm_bwd_forms(const void* dy, int64_t lddy, int32_t dy_dtype, const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                  const float* dres, int64_t lddres, int32_t T, int32_t C, float* dx, int64_t lddx, void* dxb, int64_t lddxb, float* dgamma, float* dbeta,
                                  void* ws, size_t ws_bytes, void* stream, float* dxb_colsum, void* out8, int64_t ldo8, int32_t fmt, const float* scale, float* amax,
                                  int32_t opf, const float* dy_scale, const float* dxb_rs, int32_t dxb_rps, const void* dres16, int32_t deferred);
/* TEST-ONLY: vdk_colsum_bf16_deferred (16-bit `in` [T, ld] of format opf; out f32 [N]; optional fp8 copy out8 [T, ldo8] bytes of a bf16 input with its amax, NULL = none) and
 * its job through vdk_reduce_rows_batch.  ws: vdk_colsum_bf16_workspace_bytes(T, N). */
int vdk_debug_colsum16_q8(const void* in, int64_t ld, int32_t T, int32_t N, float* out, void* ws, size_t ws_bytes, void* out8, int64_t ldo8, int32_t fmt, const float* scale,
                          float* amax, int32_t opf, void* stream);
/* tests: the class-query attention kernels of csrc/attention_cls.hip on their own (the ViT engine reaches them in-library).  Tensors as for vdk_attention_fwd_dt /
 * vdk_attention_bwd_dt, but only row b * N of q, o, dout, dq and lse[(b * H + h) * N] are touched; cspart: f32 [B][3 * H * head_dim] or NULL; grid: workgroups, 0 = default */
int vdk_debug_attention_cls_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype,
                                int32_t grid, void* stream);
int vdk_debug_attention_cls_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t ldd, float* cspart, int32_t B,
                                int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype, int32_t grid, void* stream);
/* tests / tools: the streaming attention kernels of csrc/attention_hd.hip behind the argument lists of vdk_attention_fwd_dt / vdk_attention_bwd_dt.  head_dim 72 or 80, anything
 * else VDK_EUNSUPPORTED.  The public entries keep refusing 72; the ViT engine reaches the 72-wide instance in-library. */
int vdk_debug_attention_hd_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype,
                               void* stream);
int vdk_debug_attention_hd_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, void* dqkv, int64_t lddqkv, float* dvec, int32_t B,
                               int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype, void* stream);
/* vdk_attn_pool_fwd_dt / vdk_attn_pool_bwd_dt with the head dimension as an argument: 64 (the same kernels and bits as the public entries), 72 (SigLIP SO400M) or 80; anything
 * else VDK_EUNSUPPORTED.  q f32 [H*head_dim]; kv / dkv 16-bit [B*N, 2*H*head_dim], ldkv and lddkv >= 2*H*head_dim; out / dout / dq_part f32 [B, H*head_dim]. */
int vdk_attn_pool_fwd_hd(const float* q, const void* kv, int64_t ldkv, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, float* out, int64_t ldo, float* probs,
                         int32_t dtype, void* stream);
int vdk_attn_pool_bwd_hd(const float* q, const void* kv, int64_t ldkv, const float* probs, const float* dout, int64_t lddo, int32_t B, int32_t N, int32_t H, int32_t head_dim,
                         float scale, void* dkv, int64_t lddkv, float* dq_part, int32_t dtype, void* stream);
/* SwinV2 cosine window attention (csrc/window_attention_cos.hip): 64-token windows (8 x 8), head dim 32.  qkv 16-bit [windows * 64, ld] (q | k | v thirds of 3 * H * 32 columns),
 * ld >= 3 * H * 32; o / dout [windows * 64, ldo]; lse f32 [windows, H, 64] (fwd: may be NULL); tau f32 [H] = exp(min(logit_scale, ln 100)), formed by the caller; bias f32
 * [H, 64, 64]; mask f32 [nW, 64, 64] or NULL (window w takes mask[w mod nW], windows % nW == 0); rowidx int32 [windows * 64] or NULL: token j of window w is row
 * rowidx[w * 64 + j] of qkv / o / dout / dqkv; opf 0 = bf16, 1 = fp16.  bwd: dqkv [windows * 64, ldd] (dq | dk | dv), dbias f32 [H, 64, 64] and dtau f32 [H], both summed
 * over every window and overwritten.  Pointers (the workspace included) 16-byte aligned, pitches multiples of 8.  ws: the *_workspace_bytes of the same call. */
int vdk_wa_cos_fwd_workspace_bytes(int32_t nW, int32_t H, size_t* bytes);
int vdk_wa_cos_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, const float* tau, const float* bias, const float* mask, int32_t nW, int64_t windows, int32_t H,
                   const int32_t* rowidx, int32_t opf, void* ws, size_t ws_bytes, void* stream);
int vdk_wa_cos_bwd_workspace_bytes(int64_t windows, int32_t nW, int32_t H, size_t* bytes);
int vdk_wa_cos_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, const float* tau, const float* bias, const float* mask, int32_t nW,
                   int64_t windows, int32_t H, const int32_t* rowidx, void* dqkv, int64_t ldd, float* dbias, float* dtau, int32_t opf, void* ws, size_t ws_bytes, void* stream);
/* LayerScale on the residual stream (csrc/layerscale_residual.hip; the DINOv2 ViTs): x f32 [rows, ldx], h / dh 16-bit [rows, ldh / lddh] (the branch's last GEMM output and its
 * gradient; opf 0 = bf16, 1 = fp16), gamma f32 [C].  fwd: y = x + gamma * float(h) (one fp32 multiply, one fp32 add; y may alias x).  bwd: dh = RNE16(gamma * dy) and
 * dgamma[c] = sum_r dy[r, c] * float(h[r, c]) in fp32, summed in a fixed order through ws and overwritten; the shortcut's gradient is dy itself.  C % 8 == 0, rows >= 1,
 * pitches >= C and multiples of 8 (16-bit) / 4 (f32), every pointer (ws included) 16-byte aligned: else VDK_EINVAL; another opf VDK_EUNSUPPORTED; a short ws VDK_EWORKSPACE. */
int vdk_ls_residual_fwd(const float* x, int64_t ldx, const void* h, int64_t ldh, const float* gamma, float* y, int64_t ldy, int64_t rows, int32_t C, int32_t opf, void* stream);
int vdk_ls_residual_bwd_workspace_bytes(int64_t rows, int32_t C, size_t* bytes);
int vdk_ls_residual_bwd(const float* dy, int64_t lddy, const void* h, int64_t ldh, const float* gamma, void* dh, int64_t lddh, float* dgamma, int64_t rows, int32_t C, int32_t opf,
                        void* ws, size_t ws_bytes, void* stream);
/* Exact range search (csrc/cbir_range.hip; faiss IndexFlat.range_search): every gallery row whose exact score -- the k-ordered fp32 fmaf chain of vdk_cbir_search -- passes
 * `radius` (s > radius, or s >= radius when inclusive), per query in ascending row order.  Q f32 [nq, D]; G f32 or fp16 (g_dtype VDK_F32 / VDK_F16) [N, D]; Gb / gmax_bits from
 * vdk_cbir_prepare_gallery.  Two calls with one host read between them, both on the same workspace (vdk_cbir_range_workspace_bytes(nq, N, D), untouched in between):
 *   vdk_cbir_range_count  -> lims int64 [nq + 1] (device): query i owns entries [lims[i], lims[i + 1]) of the result;
 *   vdk_cbir_range_fill   -> out_scores f32 [total], out_idx int64 [total] = idx_base + row, with total = lims[nq] as the host read it; nothing past `total` is written.
 * No capacity, no overflow, no retry: the workspace holds one bit per pair.  D % 4 (fp16 rows: % 8), D <= 512, a NaN radius, a null output with total > 0: VDK_EINVAL;
 * a short workspace: VDK_EWORKSPACE.  nq == 0 and N == 0 are served (lims all zero) and need no workspace. */
int vdk_cbir_range_workspace_bytes(int64_t nq, int64_t N, int32_t D, size_t* bytes);
int vdk_cbir_range_count(const float* Q, int64_t nq, const void* G, int32_t g_dtype, const void* Gb, const uint32_t* gmax_bits, int64_t N, int32_t D, float radius,
                         int32_t inclusive, int64_t* lims, void* ws, size_t ws_bytes, void* stream);
int vdk_cbir_range_fill(const float* Q, int64_t nq, const void* G, int32_t g_dtype, int64_t N, int32_t D, int64_t idx_base, const int64_t* lims, int64_t total, float* out_scores,
                        int64_t* out_idx, const void* ws, size_t ws_bytes, void* stream);
/* DBSCAN on a neighbourhood CSR (lims int64 [n + 1], nbr int64 [lims[n]] with values in [0, n); the point itself is a member of its neighbourhood), n < 2^31:
 *   vdk_dbscan_core    core[i] = |N(i)| >= min_samples; label[i] = i for a core point, -1 otherwise;
 *   vdk_dbscan_round   one round label_out[i] = label_in[min over i and its core neighbours j of label_in[j]] for the core points (two distinct buffers); *changed (device u32,
 *                      cleared by the caller) is set when any label moved.  Repeated until it stays clear, a core point's label is its component's smallest core index;
 *   vdk_dbscan_assign  out[i] = rank[label[i]] for a core point, the smallest rank[label[j]] among the core neighbours j of any other point, or -1; rank int32 [n] = exclusive
 *                      prefix sum of (core[i] && label[i] == i), formed by the caller. */
int vdk_dbscan_core(const int64_t* lims, int64_t n, int64_t min_samples, uint8_t* core, int32_t* label, void* stream);
int vdk_dbscan_round(const int64_t* lims, const int64_t* nbr, int64_t n, const uint8_t* core, const int32_t* label_in, int32_t* label_out, uint32_t* changed, void* stream);
int vdk_dbscan_assign(const int64_t* lims, const int64_t* nbr, int64_t n, const uint8_t* core, const int32_t* label, const int32_t* rank, int64_t* out, void* stream);
/* One Boruvka round's row scan over the cosine mutual-reachability graph (csrc/cbir_mst.hip; HDBSCAN's minimum spanning tree).  X f32 [N, D] = the unit rows; Gb bf16
 * [N, DP], gnorm f32 [3 N] and gmax_bits = the three outputs of vdk_cbir_prepare_gallery(X, N, D); core f32 [N] (>= 0); comp int32 [N] (>= 0: the component of every row).
 * For every row i of the block [q0, q0 + nq):  best_j[i] = the partner j with comp[j] != comp[i] of the smallest key (w_ij, j), w_ij = max(core_i, core_j, max(0, 1.0f - s_ij))
 * on the exact score s_ij (the k-ordered fp32 fmaf chain of vdk_cbir_search), best_w[i] = that w_ij; (+inf, -1) when every row shares comp[i].  Nothing outside the block is
 * written.  The same bits on every run: a bf16-MFMA bound pass and propose pass (one bit per pair in the workspace) only select the pairs that get the exact chain.
 * D % 4, D > 512, N < 2, N >= 2^31, a block outside [0, N), a null or misaligned pointer (X, Gb, ws: 16 bytes; the others 4): VDK_EINVAL; a short workspace
 * (vdk_mst_scan_workspace_bytes(nq, N, D)): VDK_EWORKSPACE. */
int vdk_mst_scan_workspace_bytes(int64_t nq, int64_t N, int32_t D, size_t* bytes);
/* tools: where a scan of this shape leaves its one-bit-per-pair matrix in the workspace: uint32 word [b * pitch_words + q] at offset_bytes, b < blocks, q < nq */
int vdk_mst_scan_mask_layout(int64_t nq, int64_t N, int32_t D, size_t* offset_bytes, int64_t* pitch_words, int64_t* blocks);
int vdk_mst_scan(const float* X, const void* Gb, const float* gnorm, const uint32_t* gmax_bits, const float* core, const int32_t* comp, int64_t N, int32_t D, int64_t q0,
                 int64_t nq, float* best_w, int32_t* best_j, void* ws, size_t ws_bytes, void* stream);
/* Attention with an additive relative position bias over a whole short sequence (csrc/attention_bias.hip; the BEiT models): o = softmax(scale q k^T + bias[h]) v.
 * qkv, o, dout, dqkv, lse, the pitches and dtype (VDK_BF16 | VDK_F16) as for vdk_attention_fwd_dt / vdk_attention_bwd_dt; bias f32 [H, N, N] (head, query, key), shared by
 * every batch item; lse f32 [B, H, N] (fwd: may be NULL); dbias f32 [H, N, N] = the sum over the batch of dS, overwritten, the same bits on every run.  Served: 1 <= N <= 256
 * and head_dim 64, anything else VDK_EUNSUPPORTED; a null pointer, a pitch that is short or no multiple of 8, a 16-bit tensor or workspace off a 16-byte boundary: VDK_EINVAL;
 * a workspace below the *_workspace_bytes of the same shape: VDK_EWORKSPACE. */
int vdk_attention_bias_fwd_workspace_bytes(int32_t N, int32_t H, size_t* bytes);
int vdk_attention_bias_fwd(const void* qkv, int64_t ld, void* o, int64_t ldo, float* lse, const float* bias, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale,
                           int32_t dtype, void* ws, size_t ws_bytes, void* stream);
int vdk_attention_bias_bwd_workspace_bytes(int32_t B, int32_t N, int32_t H, size_t* bytes);
int vdk_attention_bias_bwd(const void* qkv, int64_t ld, const void* o, const void* dout, int64_t ldo, const float* lse, const float* bias, void* dqkv, int64_t lddqkv,
                           float* dbias, int32_t B, int32_t N, int32_t H, int32_t head_dim, float scale, int32_t dtype, void* ws, size_t ws_bytes, void* stream);
#ifdef __cplusplus
}
#endif

/*
 * stage_hip.h -- C ABI of libstage_hip.so: the MI355X (gfx950) kernels behind model.stage.STAGE's forward/backward.
 *
 * The reference (jayleicn/TVQAplus) is pure Python/PyTorch and has no FFI; the boundary a maintainer binds is the
 * set of fused-op groups that STAGE.forward_main executes.  Every entry point below
 * names the reference lines (relative to the reference repo root) whose arithmetic it replaces.
 *
 * Conventions
 *   - all tensors are dense row-major fp32 device pointers (masks are fp32 0/1 like the reference's); `int*` where said
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous on that stream
 *   - return value: 0 on success, a hipError_t (>0) from a failed launch, or a negative STAGE_ERR_* code
 *   - dropout is counter based: (seed, element index) -> keep/drop, so the backward entry points regenerate the
 *     forward mask from the same seed; p_drop = 0 disables it (eval mode)
 *   - `ws`/`ws_bytes`: caller-provided device scratch, size from the matching *_ws_bytes() query
 *   - reductions are two-stage with a fixed summation order: results are run-to-run deterministic
 */
#ifndef STAGE_HIP_H
#define STAGE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STAGE_ERR_SHAPE (-1)      /* unsupported shape (e.g. width not a multiple of 4 / 16, Lr > 64) */
#define STAGE_ERR_WORKSPACE (-2)  /* workspace too small */

/* ---- library info -------------------------------------------------------------------------------------------- */
#define STAGE_HIP_ABI_VERSION 7  /* what stage_hip_abi_version() of a matching library returns; bumped when an existing symbol's signature or meaning changes (added symbols keep it) */
int stage_hip_abi_version(void);
const char* stage_hip_error_string(int code);
/* Measurement helpers (bench.py; no reference counterpart): events for hosts without a HIP binding, and a one-shot hook that makes the
 * next stage_str_attn_fwd call with `Lr` regions record (start, stop) on its stream around its kernel -- the K1 forward's duration
 * INSIDE a training step.  stage_k1_fwd_timer(NULL, NULL, 0) disarms.  stage_timer_elapsed_ms waits for `stop`; < 0 on error. */
void* stage_timer_create(void);
void stage_timer_destroy(void* event);
float stage_timer_elapsed_ms(void* start, void* stop);
void stage_k1_fwd_timer(void* start, void* stop, int Lr);

/* ---- K1: StructuredAttention (model/context_query_attention.py:35-101, called at model/stage.py:378) ----------
 * Cn      (N, NA, Lqa, D)  L2-normalised (+dropout) QA/context side, produced by stage_l2norm_fwd
 * Q       (N, Li, Lr, D)   raw region / subtitle-word side (normalised + dropped in-kernel for the similarity,
 *                          used raw for the weighted sum, line 81)
 * c_mask  (N, NA, Lqa), q_mask (N, Li, Lr)
 * A       (N, NA, Li, Lqa, D) ; S_raw, S_norm (N, NA, Li, Lqa, Lr)   (raw_s / s_normalized of model/stage.py:378-380)
 * limits: D % 16 == 0, D <= 256, Lr <= 64, NA*Lqa <= 256                                                        */
int stage_str_attn_fwd(const float* Cn, const float* Q, const float* c_mask, const float* q_mask, float* A,
                       float* S_raw, float* S_norm, int N, int NA, int Li, int Lqa, int Lr, int D, float scale,
                       float p_drop, unsigned long long seed, void* stream);
size_t stage_str_attn_bwd_ws_bytes(int N, int NA, int Lqa, int D);
/* dA (like A), dS_raw_ext (like S_raw, may be NULL: gradient arriving on raw_s from the attention loss),
 * Qn = stage_l2norm_fwd(Q) with the forward seed.  Outputs: dS_out (like S_raw; scratch + gradient wrt raw scores),
 * dQraw, dQn (N, Li, Lr, D) (value path / normalised path), dCn (N, NA, Lqa, D).                                 */
int stage_str_attn_bwd(const float* dA, const float* dS_raw_ext, const float* Cn, const float* Q, const float* Qn,
                       const float* S_norm, float* dS_out, float* dQraw, float* dQn, float* dCn, int N, int NA, int Li,
                       int Lqa, int Lr, int D, float scale, void* ws, size_t ws_bytes, void* stream);

/* Fused single-pass backward (D == 128, Lr even <= 64, Lqa >= 4, NA*Lqa <= 256; otherwise STAGE_ERR_SHAPE -> use
 * stage_str_attn_bwd): same mathematics (model/context_query_attention.py:58-61, 81, 95-101), but dA is read from HBM
 * once and dS never leaves the compute unit.  q_mask (N, Li, Lr) lets region tiles / frames without a valid region be
 * skipped: their gradient is exactly zero unless dS_raw_ext is non-zero in the skipped columns, which a scan of those
 * columns detects per frame (such frames are processed in full).  ws sized by stage_str_attn_bwd_fused_ws_bytes.      */
size_t stage_str_attn_bwd_fused_ws_bytes(int N, int NA, int Li, int Lqa, int D);
int stage_str_attn_bwd_fused(const float* dA, const float* dS_raw_ext, const float* Cn, const float* Q, const float* Qn,
                             const float* S_norm, const float* q_mask, float* dQraw, float* dQn, float* dCn, int N,
                             int NA, int Li, int Lqa, int Lr, int D, float scale, void* ws, size_t ws_bytes,
                             void* stream);

/* Long region rows / bf16 storage (BASELINE.json configs[4]: bf16 weights and activations with fp32 softmax accumulation,
 * D = 256, 512 subtitle words per frame): the same StructuredAttention for ANY Lr (16-region blocks, two-pass softmax) and
 * D in {16, 32, 64, 128, 256}.  storage_bf16 != 0: Cn, Q, Qn, A, dA are bf16 (masks, scores, S maps and the gradients
 * dQraw / dQn / dCn stay fp32; every product accumulates in fp32).  Qn = normalised (+dropped) Q in storage precision.
 * Backward (below): A is the forward output (the softmax backward's row term <P, dP> equals <dA, A>); dS_ws is an
 * (N,NA,Li,Lqa,Lr) fp32 scratch that receives the gradient wrt the raw scores.                                        */
int stage_str_attn_long_fwd(const void* Cn, const void* Q, const void* Qn, const float* c_mask, const float* q_mask, void* A,
                            float* S_raw, float* S_norm, int N, int NA, int Li, int Lqa, int Lr, int D, float scale,
                            int storage_bf16, void* stream);

/* The backward with the region mask at hand (round 4): region blocks behind a frame's last valid region are skipped -- there S_ = 0,
 * so dS, their share of dCn and the dQ rows are exact zeros (model/context_query_attention.py:58-61: masked scores are cos - 1e10) --
 * unless dS_raw_ext is non-zero in them (then the frame is processed in full).  The forward skips the same blocks on its own (it has
 * q_mask): raw scores -1e10 and weights 0 are stored as constants.  ws from stage_str_attn_long_bwd_qm_ws_bytes.                   */
size_t stage_str_attn_long_bwd_qm_ws_bytes(int N, int NA, int Li, int Lqa, int D);
int stage_str_attn_long_bwd_qm(const void* dA, const void* A, const float* dS_raw_ext, const void* Cn, const void* Q, const void* Qn,
                               const float* S_norm, const float* q_mask, float* dS_ws, float* dQraw, float* dQn, float* dCn, int N,
                               int NA, int Li, int Lqa, int Lr, int D, float scale, int storage_bf16, void* ws, size_t ws_bytes,
                               void* stream);

/* ---- F.normalize(p=2, eps) (+dropout)  (model/stage.py:256, model/context_query_attention.py:95-96) ----------- */
int stage_l2norm_fwd(const float* x, float* y, float* norm_out /*may be NULL*/, long long rows, int K, float eps,
                     float p_drop, unsigned long long seed, void* stream);
int stage_l2norm_bwd(const float* dy, const float* x, float* dx, long long rows, int K, float eps, float p_drop,
                     unsigned long long seed, int accumulate, void* stream);

/* ---- nn.LayerNorm(K, eps) followed by nn.Dropout(p)  (model/stage.py:85-120,133-138, LinearWrapper :15-32,
 *      model/encoder.py:37-41,47,52).  K % 4 == 0, K <= 1024.  mean/rstd (rows) are saved for the backward.
 * Fused prologue: y = drop(LN(x + res)); res may be NULL.  res_period = 0: res is (rows, K) -- the residual adds of
 * model/encoder.py:44,50 and model/stage.py:478; res_period = L: res is the (>=L, K) position table and row r uses
 * res[r % L] (model/position_encoding.py:38-43).  sum_out (rows, K), if not NULL, receives x + res.
 * In the backward, dx may be NULL when the input needs no gradient (raw features).                            ---- */
int stage_layernorm_fwd(const float* x, const float* res, int res_period, float* sum_out, const float* gamma,
                        const float* beta, float* y, float* mean, float* rstd, long long rows, int K, float eps,
                        float p_drop, unsigned long long seed, void* stream);
size_t stage_ln_bwd_ws_bytes(int K);
/* dx = LN-backward(dy) + dx_add (dx_add may be NULL: gradient that reached the exported sum x + res directly) */
int stage_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        float* dx, const float* dx_add, float* dgamma, float* dbeta, long long rows, int K,
                        float p_drop, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);

/* ---- LayerNorm(3D) over the virtual row cat([a, b, a*b])  (model/stage.py:276-279 concat_fc, :381-385 c2q) -----
 * a may be broadcast over `rep` (the Li frames): a_row = (row / (rep*inner)) * inner + row % inner; rep = 1: none.
 * y (rows, 3D).  Backward returns da_full (rows, D) NOT yet reduced over rep (use stage_reduce_rep) and db (rows, D);
 * ws sized by stage_ln_bwd_ws_bytes(3*D).  D % 4 == 0, D <= 256.                                                  */
int stage_cat3_layernorm_fwd(const float* a, const float* b, const float* gamma, const float* beta, float* y,
                             float* mean, float* rstd, long long rows, int D, int rep, int inner, float eps,
                             float p_drop, unsigned long long seed, void* stream);
int stage_cat3_layernorm_bwd(const float* dy, const float* a, const float* b, const float* mean, const float* rstd,
                             const float* gamma, float* da_full, float* db, float* dgamma, float* dbeta, long long rows,
                             int D, int rep, int inner, float p_drop, unsigned long long seed, void* ws,
                             size_t ws_bytes, void* stream);
/* Same backward with the reduction over `rep` fused in (rep > 1, D/4 a power of two in [4,64], inner <= 64): da is
 * (rows/rep, D), already summed over the frames that share a row of `a` (the `.repeat` gradient of model/stage.py:381).
 * ws sized by stage_cat3_layernorm_bwd_reduced_ws_bytes(rows, D, rep, inner).                                        */
size_t stage_cat3_layernorm_bwd_reduced_ws_bytes(long long rows, int D, int rep, int inner);
int stage_cat3_layernorm_bwd_reduced(const float* dy, const float* a, const float* b, const float* mean,
                                     const float* rstd, const float* gamma, float* da, float* db, float* dgamma,
                                     float* dbeta, long long rows, int D, int rep, int inner, float p_drop,
                                     unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
/* out[g, inner_elems] = sum_{r<rep} in[g, r, inner_elems]  (gradient of a `.repeat`/broadcast, model/stage.py:381) */
int stage_reduce_rep(const float* in, float* out, long long groups, int rep, long long inner_elems, void* stream);

/* ---- fused LayerNorm (+ residual, + dropout) -> depthwise Conv1d of the encoder blocks (model/encoder.py:37-44,
 * model/cnn.py:37-47): h = dwconv(drop(LN(x + res))); the LayerNorm output is never materialised.  x (M*L, D) rows,
 * sequences of L rows; res / res_period / sum_out as in stage_layernorm_fwd; w (D,1,k), k odd <= 9; D/4 a power of two
 * in [4, 64].  Backward: xin = the LayerNorm input (x or the exported sum), dx = d(xin) + dx_add, plus the parameter
 * gradients of both layers; ws sized by stage_ln_dwconv_bwd_ws_bytes(D, k).                                          */
int stage_ln_dwconv_fwd(const float* x, const float* res, int res_period, float* sum_out, const float* gamma,
                        const float* beta, const float* w, const float* bias, float* h, float* mean, float* rstd,
                        long long M, int L, int D, int k, float eps, float p_drop, unsigned long long seed, void* stream);
size_t stage_ln_dwconv_bwd_ws_bytes(int D, int k);
int stage_ln_dwconv_bwd(const float* dh, const float* xin, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, const float* w, float* dx, const float* dx_add, float* dgamma, float* dbeta,
                        float* dw, float* db, long long M, int L, int D, int k, float p_drop, unsigned long long seed,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- nn.Linear / 1x1 Conv1d on the matrix cores (fp32 in, fp32 out, fp32 accumulate) -----------------------------
 * Arithmetic: fp32-faithful products -- a two-way fp16 split with exact power-of-two scaling in the streaming kernels
 * (M >= 4096; error below an fp32 FMA chain's, DESIGN.md finding 20), the exact 3-way bf16 split / the f32 MFMA in the
 * tiled fallbacks.
 * Y[M,N] = epi((X .* [gate>0])[M,K] . W[N,K]^T + bias) ; epi: optional ReLU then optional + residual[M,N].
 * (model/stage.py:88,101,110,117,136; LinearWrapper :23; model/cnn.py:27-28,44-46; model/self_attention.py:32,46,54)
 * `gate` (M,K) fuses a ReLU backward on the input operand (dX = (dY .* [Y>0]) . W with W passed transposed).       */
int stage_gemm_nt(const float* X, const float* gate, const float* W, const float* bias, const float* residual, float* Y,
                  long long M, int N, int K, int relu, void* stream);
/* LayerNorm gain / bias gradients straight from the dX product of the Linear behind it, for a LayerNorm whose INPUT needs no
 * gradient (first layer of the input MLPs: LayerNorm -> Dropout -> Linear -> ReLU, model/stage.py:85-91, 98-104):
 *   dgamma[n] = sum_m G[m,n] x_hat[m,n] , dbeta[n] = sum_m G[m,n] ,  G = ((dY .* relu mask) . Wt^T) .* keep / (1 - p)
 * dY (M, K), gate_mask = the ReLU bit mask of the forward (stage_gemm_nt_mask) or NULL, Wt (N, K) = the weight transposed,
 * x / mean / rstd = the LayerNorm input and statistics, keep_mask = stage_dropout_keepmask of its dropout stream (NULL when
 * p_drop == 0).  The (M, N) gradient is reduced inside the GEMM epilogue and never written.                              */
int stage_gemm_nt_lnparam_supported(long long M, int N, int K);
size_t stage_gemm_nt_lnparam_ws_bytes(long long M, int N);
int stage_gemm_nt_lnparam(const float* dY, const unsigned* gate_mask, const float* Wt, const float* x, const float* mean,
                          const float* rstd, const unsigned* keep_mask, float p_drop, float* dgamma, float* dbeta, long long M,
                          int N, int K, void* ws, size_t ws_bytes, void* stream);
/* keep bits of the dropout stream stage_layernorm_fwd(p_drop, seed) applied to a (rows, K) output: [ceil(K/32)][rows] words */
int stage_dropout_keepmask(float p_drop, unsigned long long seed, unsigned* mask, long long rows, int K, void* stream);
/* dW[N,K] = sum_m (dY .* [gate>0])[m,n] X[m,k] ; db[N] = column sums (db may be NULL)                              */
size_t stage_gemm_tn_ws_bytes(long long M, int N, int K);
int stage_gemm_tn(const float* dY, const float* gate, const float* X, float* dW, float* db, long long M, int N, int K,
                  void* ws, size_t ws_bytes, void* stream);

/* ReLU bit masks (streaming kernels; check stage_gemm_mask_supported first).  The forward GEMM of a Linear + ReLU also
 * emits relu_mask_out[w][m] (uint32, word-major: w < ceil(N/32) rows of M words, bit b <=> Y[m][32w+b] > 0); the two backward GEMMs take that mask
 * instead of the fp32 gate (nn.ReLU backward, model/stage.py:88,101; model/cnn.py:46): 1/32 of the gate bytes.
 * stage_gemm_nt_mask: gate_mask refers to the columns of X (ceil(K/32) word rows of M words).  Returns STAGE_ERR_SHAPE when the
 * shape is not taken by the streaming kernel (fall back to stage_gemm_nt / stage_gemm_tn with the fp32 gate).        */
int stage_gemm_mask_supported(long long M, int N, int K);
int stage_gemm_nt_mask(const float* X, const unsigned* gate_mask, const float* W, const float* bias, float* Y,
                       unsigned* relu_mask_out, long long M, int N, int K, int relu, void* stream);
int stage_gemm_tn_mask(const float* dY, const unsigned* gate_mask, const float* X, float* dW, float* db, long long M,
                       int N, int K, void* ws, size_t ws_bytes, void* stream);

/* ---- encoder block pieces (model/encoder.py:35-44, model/position_encoding.py:38-43, model/cnn.py:23-26,44) ---- */
int stage_dwconv_fwd(const float* in, const float* w /*(D,1,k)*/, const float* bias, float* out, long long M, int L,
                     int D, int k, void* stream);
size_t stage_dwconv_bwd_ws_bytes(int D, int k);
int stage_dwconv_bwd(const float* dout, const float* in, const float* w, float* din, float* dw, float* db, long long M,
                     int L, int D, int k, void* ws, size_t ws_bytes, void* stream);

/* ---- multi-head self-attention core (model/self_attention.py:56-71) with the query-row mask quirk --------------
 * q,k,v,out: (M, L, D) with heads interleaved along D (head h = columns [h*dk, (h+1)*dk)); mask (M, L);
 * probs (M, nh, L, L) saved for the backward (post-softmax, pre-dropout).  L <= 64.
 * stage_mha_core_recomputes(L, D, nh) == 1 (head width D/nh in {8, 16, 32, 64}): the matrix-core kernels run, which
 * recompute the probabilities in the backward -- `probs` is then neither written nor read and may be NULL.            */
int stage_mha_core_recomputes(int L, int D, int nh);
int stage_mha_core_fwd(const float* q, const float* k, const float* v, const float* mask, float* out, float* probs,
                       long long M, int L, int D, int nh, float p_drop, unsigned long long seed, void* stream);
int stage_mha_core_bwd(const float* dout, const float* q, const float* k, const float* v, const float* probs,
                       const float* mask, float* dq, float* dk, float* dv, long long M, int L, int D, int nh,
                       float p_drop, unsigned long long seed, void* stream);

/* ---- mask_logits + max over a sequence axis (model/stage.py:503, 425, 429-432, 456-461, 532-533) ---------------
 * x (R, L, D), mask (R, L), window (R, 2) int [st, ed) or NULL for the whole axis -> out (R, D), argmax (R, D) int */
int stage_masked_max_fwd(const float* x, const float* mask, const int* window, float* out, int* argmax, long long R,
                         int L, int D, void* stream);
int stage_masked_max_bwd(const float* dout, const int* argmax, const float* mask, float* dx, long long R, int L, int D,
                         int accumulate, void* stream);

/* ---- LayerNorm whose output only feeds a masked max over the sequence axis, in one pass ---------------------------
 * The classifier head: final_layer_norm of the cls_encoder (model/encoder.py:52) -> mask_logits + max over the Lqa words
 * (model/stage.py:503).  x, res (optional, added before the norm; sum_out = x + res is written for the backward) are
 * (R, L, K); mask (R, L); out (R, K), argmax (R, K) int; mean / rstd (R * L).  The normalised (R, L, K) tensor and, in the
 * backward, its dense gradient are never materialised.  `stage_ln_masked_max_supported`: K == 128.
 * Backward: xin = the saved sum (or x when res == NULL); dx (R, L, K) is the gradient of x and of res; workspace as
 * stage_ln_bwd_ws_bytes(K).                                                                                          */
int stage_ln_masked_max_supported(int L, int K);
int stage_ln_masked_max_fwd(const float* x, const float* res, float* sum_out, const float* gamma, const float* beta,
                            const float* mask, float* out, int* argmax, float* mean, float* rstd, long long R, int L, int K,
                            float eps, void* stream);
int stage_ln_masked_max_bwd(const float* dout, const int* argmax, const float* mask, const float* xin, const float* mean,
                            const float* rstd, const float* gamma, float* dx, float* dgamma, float* dbeta, long long R, int L,
                            int K, void* ws, size_t ws_bytes, void* stream);

/* ---- bf16 storage mode (BASELINE.json configs[4]: bf16 weights / activations, fp32 softmax and accumulation) ------
 * Same operations and argument meaning as the fp32 entry points of the same name; every pointer typed `void*` is a
 * tensor of bf16 (raw 16-bit words) instead of float.  Statistics, affine parameters, weights, biases, masks, arg-max
 * indices and all parameter gradients stay fp32; a weight is rounded to bf16 while the GEMM stages it.  The
 * attention kernels of this mode: stage_str_attn_fwd_bf16 / stage_str_attn_bwd_fused_bf16 (D == 128, rows <= 64) and
 * stage_str_attn_long_* with storage == 1 (any row length, D up to 256).  The row / conv kernels are the fp32 ones instantiated
 * on 16-bit elements; the GEMMs stream 16-bit operands with one bf16 matrix-core term (gemm_bf16_stream.hip), tiled for the
 * shapes streaming does not pay for.                                                                                   */
/* K1 fast kernels on bf16 Q / A / dA (D == 128, Lr <= 64; STAGE_ERR_SHAPE otherwise -> stage_str_attn_long_*): Cn, the
 * masks, both score maps and the three gradients leaving the backward stay fp32.                                    */
int stage_str_attn_fwd_bf16(const float* Cn, const void* Q, const float* c_mask, const float* q_mask, void* A,
                            float* S_raw, float* S_norm, int N, int NA, int Li, int Lqa, int Lr, int D, float scale,
                            float p_drop, unsigned long long seed, void* stream);
int stage_str_attn_bwd_fused_bf16(const void* dA, const float* dS_raw_ext, const float* Cn, const void* Q, const void* Qn,
                                  const float* S_norm, const float* q_mask, float* dQraw, float* dQn, float* dCn, int N,
                                  int NA, int Li, int Lqa, int Lr, int D, float scale, void* ws, size_t ws_bytes,
                                  void* stream);
int stage_layernorm_fwd_bf16(const void* x, const void* res, int res_period, void* sum_out, const float* gamma,
                             const float* beta, void* y, float* mean, float* rstd, long long rows, int K, float eps,
                             float p_drop, unsigned long long seed, void* stream);
int stage_layernorm_bwd_bf16(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                             void* dx, const void* dx_add, float* dgamma, float* dbeta, long long rows, int K,
                             float p_drop, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
int stage_cat3_layernorm_fwd_bf16(const void* a, const void* b, const float* gamma, const float* beta, void* y,
                                  float* mean, float* rstd, long long rows, int D, int rep, int inner, float eps,
                                  float p_drop, unsigned long long seed, void* stream);
/* da_full (rows, D) stays fp32 (reduce it over `rep` with stage_reduce_rep); db (rows, D) is bf16 */
int stage_cat3_layernorm_bwd_bf16(const void* dy, const void* a, const void* b, const float* mean, const float* rstd,
                                  const float* gamma, float* da_full, void* db, float* dgamma, float* dbeta,
                                  long long rows, int D, int rep, int inner, float p_drop, unsigned long long seed,
                                  void* ws, size_t ws_bytes, void* stream);
/* da (rows / rep, D) fp32 (a sum over the `rep` frames), db (rows, D) bf16; ws as for the fp32 entry point */
int stage_cat3_layernorm_bwd_reduced_bf16(const void* dy, const void* a, const void* b, const float* mean,
                                          const float* rstd, const float* gamma, float* da, void* db, float* dgamma,
                                          float* dbeta, long long rows, int D, int rep, int inner, float p_drop,
                                          unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
int stage_l2norm_fwd_bf16(const void* x, void* y, float* norm_out, long long rows, int K, float eps, float p_drop,
                          unsigned long long seed, void* stream);
int stage_l2norm_bwd_bf16(const void* dy, const void* x, void* dx, long long rows, int K, float eps, float p_drop,
                          unsigned long long seed, int accumulate, void* stream);
/* dx (bf16) = add (fp32, may be NULL) + l2norm backward of (dy fp32, x bf16): folds the attention backward's two fp32
 * gradients (raw path, normalised path) into one bf16 gradient in a single pass                                      */
int stage_l2norm_bwd_mixed_bf16(const float* dy, const void* x, const float* add, void* dx, long long rows, int K, float eps,
                                float p_drop, unsigned long long seed, void* stream);
int stage_gemm_nt_bf16(const void* X, const void* gate, const float* W, const float* bias, const void* residual, void* Y,
                       long long M, int N, int K, int relu, void* stream);
size_t stage_gemm_tn_bf16_ws_bytes(long long M, int N, int K);
int stage_gemm_tn_bf16(const void* dY, const void* gate, const void* X, float* dW, float* db, long long M, int N, int K,
                       void* ws, size_t ws_bytes, void* stream);
int stage_dwconv_fwd_bf16(const void* in, const float* w, const float* bias, void* out, long long M, int L, int D, int k,
                          void* stream);
int stage_dwconv_bwd_bf16(const void* dout, const void* in, const float* w, void* din, float* dw, float* db, long long M,
                          int L, int D, int k, void* ws, size_t ws_bytes, void* stream);
int stage_ln_dwconv_fwd_bf16(const void* x, const void* res, int res_period, void* sum_out, const float* gamma,
                             const float* beta, const float* w, const float* bias, void* h, float* mean, float* rstd,
                             long long M, int L, int D, int k, float eps, float p_drop, unsigned long long seed,
                             void* stream);
int stage_ln_dwconv_bwd_bf16(const void* dh, const void* xin, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, const float* w, void* dx, const void* dx_add, float* dgamma, float* dbeta,
                             float* dw, float* db, long long M, int L, int D, int k, float p_drop, unsigned long long seed,
                             void* ws, size_t ws_bytes, void* stream);
/* self-attention core on bf16 q / k / v / out: the matrix-core kernels only (stage_mha_core_recomputes == 1) */
int stage_mha_core_fwd_bf16(const void* q, const void* k, const void* v, const float* mask, void* out, long long M, int L,
                            int D, int nh, float p_drop, unsigned long long seed, void* stream);
int stage_mha_core_bwd_bf16(const void* dout, const void* q, const void* k, const void* v, const float* mask, void* dq,
                            void* dk, void* dv, long long M, int L, int D, int nh, float p_drop, unsigned long long seed,
                            void* stream);
/* self-attention core on FUSED projections (round 5): qkv (M, L, 3D) = the output of ONE Linear(D -> 3D) with the weight
 * [W_q; W_k; W_v] (model/self_attention.py:35-44: three Linears on the same input), thirds q | k | v of every row; dqkv (M, L, 3D)
 * receives dq | dk | dv and IS that Linear's output gradient.  out / dout (M, L, D).  is_bf16: storage type of all four.  Matrix-core
 * shapes only (stage_mha_core_recomputes == 1), same masking / dropout contract as stage_mha_core_fwd.                          */
int stage_mha_core_qkv_fwd(const void* qkv, const float* mask, void* out, long long M, int L, int D, int nh, float p_drop,
                           unsigned long long seed, int is_bf16, void* stream);
int stage_mha_core_qkv_bwd(const void* dout, const void* qkv, const float* mask, void* dqkv, long long M, int L, int D, int nh,
                           float p_drop, unsigned long long seed, int is_bf16, void* stream);
int stage_masked_max_fwd_bf16(const void* x, const float* mask, const int* window, void* out, int* argmax, long long R,
                              int L, int D, void* stream);
int stage_masked_max_bwd_bf16(const void* dout, const int* argmax, const float* mask, void* dx, long long R, int L, int D,
                              int accumulate, void* stream);
int stage_ln_masked_max_fwd_bf16(const void* x, const void* res, void* sum_out, const float* gamma, const float* beta,
                                 const float* mask, void* out, int* argmax, float* mean, float* rstd, long long R, int L,
                                 int K, float eps, void* stream);
int stage_ln_masked_max_bwd_bf16(const void* dout, const int* argmax, const float* mask, const void* xin, const float* mean,
                                 const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta, long long R,
                                 int L, int K, void* ws, size_t ws_bytes, void* stream);

/* ---- backward of  y = ReLU(drop(LN_3D([a, b, a*b])) W^T + c)  without the 3D-wide gradient (csrc/cat3_fused.hip) -----------------
 * (model/stage.py:381-385 c2q_down_projection, :276-279 concat_fc.)  The Linear's input gradient (dy .* relu') W, 1.47 GB at the
 * full configuration, is neither written nor read back: one workgroup owns complete 3D-wide rows, the product stays in matrix-core
 * accumulators and the LayerNorm backward runs on them.  dy (rows, D) = gradient of the Linear's output BEFORE the ReLU gate;
 * relu_mask = the forward's ReLU bit mask ([D/32][rows], stage_gemm_nt_mask); W (D, 3D); a, b, mean, rstd, gamma, p_drop, seed as
 * for stage_cat3_layernorm_bwd*.  Outputs: rep > 1: da (rows / rep, D) summed over the frames (as ..._bwd_reduced), rep == 1:
 * da (rows, D); db (rows, D); dgamma, dbeta (3D).  D == 128, rows >= 4096 (STAGE_ERR_SHAPE otherwise).                         */
int stage_cat3_dx_ln_bwd_supported(long long rows, int D, int rep, int inner);
size_t stage_cat3_dx_ln_bwd_ws_bytes(long long rows, int D, int rep, int inner);
int stage_cat3_dx_ln_bwd(const float* dy, const unsigned* relu_mask, const float* W, const float* a, const float* b,
                         const float* mean, const float* rstd, const float* gamma, float* da, float* db, float* dgamma,
                         float* dbeta, long long rows, int D, int rep, int inner, float p_drop, unsigned long long seed, void* ws,
                         size_t ws_bytes, void* stream);
/* Forward twin: z = drop(LN_3D([a, b, a*b])) and y = ReLU(z W^T + bias) in one pass over a and b (z is written once for the
 * backward's weight-gradient GEMM, never read back here).  z, mean, rstd are bit-identical to stage_cat3_layernorm_fwd; y and
 * relu_mask_out ([D/32][rows]) as stage_gemm_nt_mask on that z.  D == 128, rows >= 4096; rep > 1 needs inner >= 11 and
 * rep * inner >= 32 (STAGE_ERR_SHAPE otherwise); ws: stage_cat3_ln_gemm_fwd_ws_bytes(). */
int stage_cat3_ln_gemm_fwd_supported(long long rows, int D, int rep, int inner);
size_t stage_cat3_ln_gemm_fwd_ws_bytes(void);
int stage_cat3_ln_gemm_fwd(const float* a, const float* b, const float* gamma, const float* beta, const float* W, const float* bias,
                           float* z, float* mean, float* rstd, float* y, unsigned* relu_mask_out, long long rows, int D, int rep,
                           int inner, float eps, float p_drop, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);

/* ---- the same backward WITH the Linear's own gradients, no saved z (csrc/cat3_bwd_dw.hip) -----------------------------------------
 * (model/stage.py:381-385, :276-279, :107-113, :133-138.)  One persistent 8-wave workgroup per compute unit owns complete rows and
 * the whole (D, 3D) weight gradient in matrix-core accumulators: dz = (dy .* relu') W never exists as a tensor (as above) AND
 * dW[n][k] = sum_rows (dy .* relu')[row][n] z[row][k], dc[n] = sum_rows (dy .* relu')[row][n] are formed from z REBUILT in registers
 * (a, b, the saved row statistics, gamma / beta, the dropout stream) -- the forward passes z = NULL to stage_cat3_ln_gemm_fwd* and
 * no weight-gradient GEMM runs.  Arguments as stage_cat3_dx_ln_bwd plus beta (3D), dW (D, 3D), dc (D).                            */
int stage_cat3_bwd_dw_supported(long long rows, int D, int rep, int inner);
size_t stage_cat3_bwd_dw_ws_bytes(long long rows, int D, int rep, int inner);
int stage_cat3_bwd_dw(const float* dy, const unsigned* relu_mask, const float* W, const float* a, const float* b, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, float* da, float* db, float* dgamma, float* dbeta,
                      float* dW, float* dc, long long rows, int D, int rep, int inner, float p_drop, unsigned long long seed, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- K-groups: launch sequencing on the C side (one forward and one backward symbol per fused-op group) --
 * Each group runs the kernels above in the order tvqaplus_amd/ops.py would, as ONE call (csrc/groups.hip); fp32 storage.
 * Memory protocol: `arena` (stage_grp_*_arena_bytes) = what the forward keeps for the backward, carved deterministically;
 * `tmp` (stage_grp_*_bwd_tmp_bytes) = backward-only scratch; `flags` = host ints written by the forward and handed back to the
 * backward (which optional kernel paths ran; 16 ints are enough for every group); `params` / `grads` = HOST arrays of device
 * pointers in the order each group documents; `seeds` = host array, one entry per dropout site in forward order.
 * STAGE_ERR_SHAPE is returned before anything is launched when a group does not take the shape (use the per-op entry points). */
/* G1 input MLP (model/stage.py:350-362, :85-91, :98-104, :115-120; l2 != 0: F.normalize of :256 first):
 * [l2norm] -> LN(K0)+drop -> Linear(K0->H)+ReLU -> LN(H)+drop -> Linear(H->D)+ReLU -> LN(D).  M rows of x -> out (M, D).
 * params / grads: g0 b0 W1 c1 g1 b1 W2 c2 g2 b2; seeds[2]; flags[2].  The features receive no gradient.
 * One entry point per direction; the forms differ in the first stage only:
 *   dtype     STAGE_DT_F32: x holds fp32 rows.  STAGE_DT_F16 / STAGE_DT_BF16: x holds half-precision rows that the first stage reads
 *             in place (stage_feat16_ln_* below) -- no fp32 image of the features and, with l2, no normalised image is written.
 *   src_rows  NULL: the rows are rows 0..M of x.  Otherwise (M) int32, row r reads x[src_rows[r]]: the live rows of a padded ragged
 *             context stream (stage_rag_ctx_rows) or the rows of a packed one (stage_pack_ctx_rows), read through the table by
 *             stage_layernorm_gather_* / stage_l2norm_gather_fwd / stage_feat16_ln_*.  (NULL is the dense form, never an error.)
 *   arena     carves the normalised image xn only for l2 != 0 with fp32 rows; pass the same M, l2 and dtype to the size query.
 * The backward scratch does not depend on the form.  Refused before a launch with STAGE_ERR_SHAPE: a dtype outside the three;
 * fp32 forward: M <= 0, K0 / H / D not a multiple of 4 or above 1024; half rows, forward and backward: M <= 0 or >= 2^31, H / D not
 * a positive multiple of 4 or above 1024, a K0 that stage_feat16_supported declines, x NULL or not 8-byte aligned.  A buffer smaller
 * than its query names: STAGE_ERR_WORKSPACE.                                                                                    */
size_t stage_grp_input_mlp_arena_bytes(long long M, int K0, int H, int D, int l2, int dtype);
int stage_grp_input_mlp_fwd(const void* x, int dtype, const int* src_rows, const float* const* params, float* out, void* arena,
                            size_t arena_bytes, int* flags, long long M, int K0, int H, int D, int l2, float p_drop,
                            const unsigned long long* seeds, void* stream);
size_t stage_grp_input_mlp_bwd_tmp_bytes(long long M, int K0, int H, int D);
int stage_grp_input_mlp_bwd(const float* dout, const void* x, int dtype, const int* src_rows, const float* const* params,
                            float* const* grads, const void* arena, size_t arena_bytes, const int* flags, void* tmp, size_t tmp_bytes,
                            long long M, int K0, int H, int D, int l2, float p_drop, const unsigned long long* seeds, void* stream);
/* G2 encoder block without self-attention (model/encoder.py:29-52, model/cnn.py:37-47, model/position_encoding.py:38-43):
 * `rows` rows of x that form S sequences of at most L positions, pe (>= L, D).  pool_mask != NULL: out = masked max over each
 * sequence of the block's output (model/stage.py:503); otherwise out (rows, D).  params / grads: per conv i (ln_g ln_b dw_w dw_b
 * pw_w pw_b), then final_g final_b; seeds: one per even conv index; flags[n_conv + 1].  dx (rows, D) may be NULL.
 * One entry point per direction; the forms differ in the LayerNorm -> depthwise-conv launch and in the final stage only:
 *   T == NULL  dense: x (S, L, D); rows = S * L and cap = rows (anything else: STAGE_ERR_SHAPE); pool_mask (S, L); a pooled out is
 *              (S, D) and out_rows is ignored; n_conv 0..8.
 *   T != NULL  ragged ("K-groups on ragged rows" below): x (rows, D) = the U compact rows of the S sequences T[2] = seq names, L = the
 *              longest (Lqa); cap = Ucap >= rows, the row count the arena is sized for; pool_mask = qa_mask (groups, L), a pooled out
 *              is (out_rows, D) dense -- rows no sequence writes come back filled -- and the backward reads T[3] = rowinfo;
 *              unpooled: out (rows, D), out_rows is ignored; n_conv 1..8; pooled needs D = 128.
 * Size queries: cap and out_rows as above (dense: out_rows = S), ragged = (T != NULL), pooled = (pool_mask != NULL).
 * Refused before a launch, forward and backward, with STAGE_ERR_SHAPE: S <= 0, L < 1, rows <= 0, n_conv outside the form's range, a
 * (D, k) the LayerNorm -> depthwise-conv kernels do not take, D > 1024, and the form's conditions above.  A buffer smaller than its
 * query names: STAGE_ERR_WORKSPACE.                                                                                              */
size_t stage_grp_encoder_arena_bytes(long long cap, long long out_rows, int D, int n_conv, int pooled, int ragged);
int stage_grp_encoder_fwd(const float* x, const float* pe, const float* pool_mask, const float* const* params, float* out,
                          const int* const* T, void* arena, size_t arena_bytes, int* flags, long long rows, long long cap, long long S,
                          long long out_rows, int L, int D, int n_conv, int k, float p_drop, const unsigned long long* seeds,
                          void* stream);
size_t stage_grp_encoder_bwd_tmp_bytes(long long cap, int D, int k, int pooled, int ragged);
int stage_grp_encoder_bwd(const float* dout, const float* pool_mask, const float* const* params, float* const* grads, float* dx,
                          const int* const* T, const void* arena, size_t arena_bytes, const int* flags, void* tmp, size_t tmp_bytes,
                          long long rows, long long cap, long long S, long long out_rows, int L, int D, int n_conv, int k,
                          float p_drop, const unsigned long long* seeds, void* stream);
/* G3 QA <-> context attention + down-projection (model/stage.py:365-387): qa (N,NA,Lqa,D), ctx (N,Li,Lr,D) ->
 * mixed (N,NA,Li,Lqa,D), S_raw / S_norm (N,NA,Li,Lqa,Lr).  params / grads: ln_g ln_b W c; seeds[3] = context-side, region-side,
 * LayerNorm dropout.  Backward: dS_ext = gradient on S_raw or NULL; d_qa sums both uses of the QA embedding.              */
size_t stage_grp_qa_ctx_arena_bytes(int N, int NA, int Li, int Lqa, int D);
int stage_grp_qa_ctx_fwd(const float* qa, const float* ctx, const float* qa_mask, const float* ctx_mask,
                         const float* const* params, float* mixed, float* S_raw, float* S_norm, void* arena, size_t arena_bytes,
                         int* flags, int N, int NA, int Li, int Lqa, int Lr, int D, float scale, float p_drop,
                         const unsigned long long* seeds, void* stream);
size_t stage_grp_qa_ctx_bwd_tmp_bytes(int N, int NA, int Li, int Lqa, int Lr, int D);
int stage_grp_qa_ctx_bwd(const float* d_mixed, const float* dS_ext, const float* qa, const float* ctx, const float* ctx_mask,
                         const float* mixed, const float* S_norm, const float* const* params, float* const* grads, float* d_qa,
                         float* d_ctx, const void* arena, size_t arena_bytes, const int* flags, void* tmp, size_t tmp_bytes, int N,
                         int NA, int Li, int Lqa, int Lr, int D, float scale, float p_drop, const unsigned long long* seeds,
                         void* stream);
/* G4 two-stream fusion (model/stage.py:276-279, :106-113): s, v (U, D) -> out (U, D).  params / grads: ln3_g ln3_b W c ln_g ln_b;
 * seeds[1].                                                                                                                */
size_t stage_grp_concat_fc_arena_bytes(long long U, int D);
int stage_grp_concat_fc_fwd(const float* s, const float* v, const float* const* params, float* out, void* arena,
                            size_t arena_bytes, int* flags, long long U, int D, float p_drop, const unsigned long long* seeds,
                            void* stream);
size_t stage_grp_concat_fc_bwd_tmp_bytes(long long U, int D);
int stage_grp_concat_fc_bwd(const float* dout, const float* s, const float* v, const float* const* params, float* const* grads,
                            float* ds, float* dv, const void* arena, size_t arena_bytes, const int* flags, void* tmp,
                            size_t tmp_bytes, long long U, int D, float p_drop, const unsigned long long* seeds, void* stream);
/* G5 temporal head, layer 0 (model/stage.py:469-482, LinearWrapper :15-32): enc (R, D) -> first = enc + h (R, D), t_st, t_ed (R).
 * params / grads: lnp_g lnp_b Wp cp lns_g lns_b Ws cs lne_g lne_b We ce; seeds[3].  d_first may be NULL.                  */
size_t stage_grp_temporal_head_arena_bytes(long long R, int D);
int stage_grp_temporal_head_fwd(const float* enc, const float* const* params, float* first, float* t_st, float* t_ed,
                                void* arena, size_t arena_bytes, int* flags, long long R, int D, float p_drop,
                                const unsigned long long* seeds, void* stream);
size_t stage_grp_temporal_head_bwd_tmp_bytes(long long R, int D);
int stage_grp_temporal_head_bwd(const float* d_first, const float* d_st, const float* d_ed, const float* enc, const float* first,
                                const float* const* params, float* const* grads, float* d_enc, const void* arena,
                                size_t arena_bytes, const int* flags, void* tmp, size_t tmp_bytes, long long R, int D,
                                float p_drop, const unsigned long long* seeds, void* stream);

/* ---- head glue (model/stage.py:389-467, 484-555, 613-746): the small tensor algebra around the temporal scores, the span
 * proposals, the pooling, the classifier and the two auxiliary losses as a handful of kernels (csrc/groups.hip) ----------- */
/* t_scores (N, NA, Li, 2) = mask_logits(cat(t_st, t_ed), frame mask (N, Li))   (model/stage.py:515-521) and its backward */
int stage_tscores_fwd(const float* t_st, const float* t_ed, const float* tm, float* out, int N, int NA, int Li, void* stream);
int stage_tscores_bwd(const float* dout, const float* tm, float* d_st, float* d_ed, int N, int NA, int Li, void* stream);
/* span proposal of the ground-truth candidate (training, model/stage.py:408-418, model/model_utils.py:92-123): softmax over the
 * frames, arg max of the upper-triangular products (first maximal pair).  target / labels: int64 (N).  spans (6, N) float:
 * predicted start, end, confidence, label start, label end, answer index (so that ONE device-to-host copy carries everything
 * the proposal bookkeeping needs).  Li <= 2048.                                                                               */
int stage_gt_spans(const float* t_scores, const long long* target, const long long* lab_st, const long long* lab_ed,
                   float* spans, int N, int NA, int Li, void* stream);
/* Top-K span proposals (csrc/topk_spans.hip; model/model_utils.py:92-123 find_max_triples with topN = K, model/stage.py:389-438
 * get_proposals(max_num_proposal = K)): the K pairs (st <= ed) of a row with the largest p_st[st] * p_ed[ed], value descending, equal
 * values by ascending st * Li + ed (a total order: the list is unique).  One workgroup per row, O(Li) memory, no (Li, Li) product.
 * Ranks that no pair fills (Li (Li + 1) / 2 < K) are st = ed = -1, confidence 0.  The softmax and the product are stage_gt_spans'
 * arithmetic, so rank 0 carries the bits stage_gt_spans / stage_grp_eval_head_fwd report.
 * stage_topk_spans_supported: 1 <= Li <= 2048 and 1 <= K <= STAGE_TOPK_MAX (needs no GPU); elsewhere the other two return
 *   STAGE_ERR_SHAPE before a launch.
 * stage_gt_spans_topk: stage_gt_spans with K ranks.  spans (3K + 3, N) float: rows 3k, 3k + 1, 3k + 2 = start, end, confidence of
 *   rank k, then label start, label end, answer index; K = 1 writes exactly the (6, N) of stage_gt_spans.
 * stage_topk_spans: x (R, Li, 2) [start, end] per frame, 8-byte aligned; is_prob == 0: scores, softmaxed over the frames here (as
 *   the evaluation head reads them); is_prob != 0: probabilities >= 0, used as given (as stage_answer_spans reads them).
 *   span (R, K, 2) int32 [st, ed], conf (R, K).                                                                                  */
#define STAGE_TOPK_MAX 8
int stage_topk_spans_supported(int Li, int K);
int stage_gt_spans_topk(const float* t_scores, const long long* target, const long long* lab_st, const long long* lab_ed,
                        float* spans, int N, int NA, int Li, int K, void* stream);
int stage_topk_spans(const float* x, int is_prob, int* span, float* conf, long long R, int Li, int K, void* stream);
/* temporal loss (model/stage.py:539-555) and d loss / d t_scores in one pass; scratch: N floats; cand_offset: global index of
 * local candidate 0 (candidate-sharded batches: examples whose ground truth is not local contribute nothing); na_total: the
 * model's candidate count over all ranks (a target outside [0, na_total) makes the loss NaN; <= 0: cand_offset + NA)        */
int stage_ts_loss(const float* t_scores, const long long* target, const long long* lab_st, const long long* lab_ed, float* loss,
                  float* grad, float* scratch, int N, int NA, int Li, int cand_offset, int na_total, void* stream);
/* The caller's loss line (main.py:55-60) in one launch: loss[0] = CE_sum(logits (P, C), targets (P)) * scale + att_w * att_loss[0] +
 * ts_w * t_loss[0] (att_loss / t_loss may be NULL), dlogits (P, C) = scale * (softmax - onehot) = the gradient of the first term.
 * scale = scale_dev[0] if scale_dev != NULL (multi-GPU: a device word), else scale_host.  Negative targets are ignored (ignore_index). */
int stage_train_loss(const float* logits, const long long* targets, const float* att_loss, const float* t_loss, const float* scale_dev,
                     float scale_host, float att_w, float ts_w, float* loss, float* dlogits, int P, int C, void* stream);
/* supervised attention loss (model/stage.py:738-745) over M (positive, negative) pairs: flat = 2M int64 indices into scores
 * (positives, then negatives); hinge != 0: max(0, margin + s_neg - s_pos), else log1p(exp(alpha (s_neg - s_pos))).  coef (M) is
 * kept for the backward, which zero-fills dS (n_scores floats) and scatters gout[0] * coef into it.                          */
int stage_att_loss_fwd(const float* scores, const long long* flat, long long M, int hinge, float alpha, float margin, float* coef,
                       float* loss, void* stream);
int stage_att_loss_bwd(const long long* flat, const float* coef, const float* gout, long long M, float* dS, long long n_scores,
                       void* stream);
/* Selected rows of the attention map (csrc/score_rows.hip): K rows of Lr <= 64 scores, row k = scores[row_off[k] .. + Lr), one
 * wavefront per row.  Ties: the lower region index first; +0 == -0.  A row with row_off[k] < 0 or row_off[k] + Lr > n_scores is
 * never read and gets a sentinel (cnt = -1 / flat_neg = -1), as does a pair slot whose position is not below the row's negatives.
 * stage_att_predict (model/stage.py:748-806): the regions with score >= thd (fp32 compare) in ASCENDING score order:
 *   cnt (K) int32, val (K, Lr) the scores, idx (K, Lr) int32 the regions; slots past cnt[k] hold val = 0, idx = -1.
 * stage_att_hard_negatives (model/stage.py:557-611): negbits (K) bit r = region r is a labelled negative of row k; pair slots
 *   [slot_begin[k], slot_begin[k + 1]) belong to row k (slot_begin: K + 1 int32, M slots in all); slot_q (M) = position of the
 *   slot's negative in the DESCENDING score order of the row's negatives (a NaN score sorts last).
 *   flat_neg (M) int64 = row_off[k] + region: the negative half of stage_att_loss_fwd's `flat`.
 * stage_score_rows_supported: 1 for 1 <= Lr <= 64 (needs no GPU); the other two return STAGE_ERR_SHAPE where it says 0.        */
int stage_score_rows_supported(int Lr);
int stage_att_predict(const float* scores, const long long* row_off, int K, int Lr, long long n_scores, float thd, int* cnt,
                      float* val, int* idx, void* stream);
int stage_att_hard_negatives(const float* scores, const long long* row_off, const unsigned long long* negbits,
                             const int* slot_begin, const int* slot_q, int K, int M, int Lr, long long n_scores,
                             long long* flat_neg, void* stream);
/* G6 proposal pooling + answer classifier (model/stage.py:420-467, 526-536): first (N*NA, Li, D), mask (N*NA, Li), glob / idx_g =
 * stage_masked_max_fwd(first, mask) computed ahead; meta (device int32) = src[P] | win[2P] | inv[slots * N] (proposal -> example,
 * frame window [st, ed), example -> its proposals or -1: below).  logits (P*NA).  params / grads: ln_g ln_b W c (2D wide); seeds[1].
 * d_first (N*NA, Li, D) receives both pooling paths.                                                                          */
size_t stage_grp_pool_cls_arena_bytes(long long P, int NA, int D);
int stage_grp_pool_cls_fwd(const float* first, const float* mask, const float* glob, const int* meta, const float* const* params,
                           float* logits, void* arena, size_t arena_bytes, int N, int NA, int Li, int D, long long P, float p_drop,
                           const unsigned long long* seeds, void* stream);
size_t stage_grp_pool_cls_bwd_tmp_bytes(long long P, int NA, int D);
/* The backward, with up to `slots` proposals per example (max_num_proposal = slots - 1 predicted spans + the label's):
 * meta = src[P] | win[2P] | inv[slots * N], inv (N, slots) = the example's proposals in ascending slot order or -1; the sums over
 * an example's proposals run in that order.  1 <= slots <= STAGE_TOPK_MAX + 1 (STAGE_ERR_SHAPE otherwise).  The forward reads src
 * and win only and needs no counterpart.                                                                                         */
int stage_grp_pool_cls_bwd_s(const float* d_logits, const float* mask, const int* idx_g, const int* meta, const float* const* params,
                             float* const* grads, float* d_first, const void* arena, size_t arena_bytes, void* tmp, size_t tmp_bytes,
                             int N, int NA, int Li, int D, long long P, int slots, float p_drop, const unsigned long long* seeds,
                             void* stream);
/* The proposal decision of get_proposals in training (model/stage.py:411-438; model/model_utils.py:37-89) on the device, at a fixed
 * capacity: no read-back of the span table, no data-dependent row count (csrc/proposals.hip).
 *   spans     (3K + 3, N) float, what stage_gt_spans (K = 1) / stage_gt_spans_topk write, used as it is
 *   meta      (5 Pmax) int32 = src[Pmax] | win[2 Pmax] | inv[slots * N] | tgt[Pmax], slots = K + 1, Pmax = slots * N: the layout
 *             of stage_grp_pool_cls_fwd / _bwd_s with P = Pmax
 *   rows [0, P): per example the label's span, then every rank with (double)conf >= ce_prob_thd, start >= 0, union != 0 and
 *             (double)inter / (double)union >= iou_thd (inter / union: integers over end-exclusive spans), in rank order; windows
 *             [max(0, st - extra), ed + 1 + extra), the upper end unclamped; tgt = the example's answer index
 *   rows [P, Pmax): src / win of row 0, tgt = -100 (stage_train_loss ignores a negative target); no inv entry names them
 *   count[0] = P (N <= P <= Pmax), scale[0] = (float)((double)N / (double)P)
 *   thd_host  HOST array {iou_thd, ce_prob_thd} as double (the one host pointer of the call), read before it returns: the
 *             comparisons run in double as the host loop's do (a float 0.01f would keep a confidence of np.float32(0.01))
 * A start / end that is negative, non-finite or >= 2^30 makes its rank absent; no value of the table is used as an index.  One
 * workgroup, plain stores, bitwise repeatable.  STAGE_ERR_SHAPE before any launch: K outside 1 .. STAGE_TOPK_MAX, N <= 0,
 * 5 * (K + 1) * N beyond int, extra outside 0 .. 2^20, a NULL pointer.                                                          */
int stage_proposal_meta(const float* spans, int N, int K, const double* thd_host, int extra, int* meta, int* count, float* scale,
                        void* stream);

/* G7 evaluation head (model/stage.py:440-448, 526-536 outside training; csrc/eval_head.hip): what get_proposals + the classifier do in
 * eval()/inference for R = N * NA independent rows, forward only.  first (R, Li, D), mask (R, Li), t_scores (R, Li, 2).
 *   span (R, 2) int32 [st, ed] = arg max over i <= j of softmax(start)[i] * softmax(end)[j], ties: smallest i * Li + j; conf (R) its
 *   value; both may be NULL.  pooled row = [masked max over [max(0, st - extra), ed + 1 + extra) | masked max over all frames]
 *   (local == 0: the latter only, D wide; t_scores may then be NULL unless span / conf is wanted), then LayerNorm and Linear(-> 1)
 *   through stage_layernorm_fwd / stage_gemm_nt: logits (R).  params: ln_g ln_b W c.  O(Li) memory per row; nothing is kept.
 * stage_eval_head_supported: 1 <= Li <= 2048, D % 4 == 0, 2 D <= 1024 (needs no GPU); elsewhere the group returns STAGE_ERR_SHAPE
 *   before anything is launched.
 * stage_answer_spans (inference.py:13-35 for a batch): answer (N, NA <= 64), t_prob (N, NA, Li <= 2048, 2) ALREADY softmaxed ->
 *   out (N, 3) int32 [st, ed, answer]: answer = first arg max of the row; the span of that candidate by the sweep of
 *   find_max_pair (start = first arg max of p_st[:i + 1], end = first position reaching the best product, (0, 1) when it is <= 0). */
int stage_eval_head_supported(int Li, int D, int local);
size_t stage_grp_eval_head_arena_bytes(long long R, int D, int local);
int stage_grp_eval_head_fwd(const float* first, const float* mask, const float* t_scores, const float* const* params, float* logits,
                            int* span, float* conf, void* arena, size_t arena_bytes, long long R, int Li, int D, int extra, int local,
                            void* stream);
int stage_answer_spans(const float* answer, const float* t_prob, int* out, int N, int NA, int Li, void* stream);


/* ==== Ragged token rows: live-range execution of the (N, 5, Li, Lqa, .) kernels ===================================================
 * The reference computes every padded row of the (N,5,Li,Lqa,D) tensors (model/stage.py:365-387 qa_ctx_attention, :276-279 concat_fc,
 * :484-505 classifier head; no masking inside LayerNorm / Linear / the convolutions of model/encoder.py:35-52, model/cnn.py:42-47).
 * Only this reaches an output or a gradient: frames whose statement mask is not all zero (the others pool to the constant -1e10 at
 * model/stage.py:503 and get the gradient dout * mask = 0), and of those the words below Lc = min(Lqa, last valid word + 1 + halo),
 * halo = (convolution layers of the classifier encoder) * (kernel_size / 2) -- the receptive field through which padded words leak
 * into valid ones.  The entry points below run on exactly those rows ("compact rows": [group g = (n, a)][live frame][word < Lc(g)]);
 * the attention output A and its gradient keep all Lqa words of a live frame ("frame-compact rows":
 * [sequence = first(n) + a * slots(n) + slot][word], slots(n) = live frames of example n + one dump slot that dead frames use).
 * Tables (device int32, built by tvqaplus_amd/ragged.py from the masks):
 *   fmap    [N*Li] slot of each frame (< 0 dead) | [N] slots(n) | [N] first(n)
 *   gdesc   (N*NA, 4)  first compact row, Lc, slots(n), first frame-compact sequence of the group
 *   seq     (S, 4)     first compact row, length, group, dense output row g*Li + i            one per (group, live frame)
 *   seqfc   (S)        frame-compact sequence of each entry of seq
 *   rowinfo (U, 4)     QA row g*Lqa + w, frame-compact row, dense output row, w                 (stage_rag_rowinfo)                 */
int stage_rag_rowinfo(const int* seq, const int* seqfc, long long S, int Lqa, int* rowinfo, void* stream);
/* Ragged CONTEXT rows (the (N, Li, Lw|Lr, .) streams in front of the attention: model/stage.py:235-270): frame f keeps its valid words /
 * regions plus the halo of the input encoder's convolutions, cq[f] = (first compact row, rows); src_rows[r] = row of the padded feature
 * tensor that compact row r reads (stage_rag_ctx_rows).  The *_gather entry points are LayerNorm / L2 normalisation reading those rows
 * in place (model/stage.py:85-91, 98-104, 256); everything behind them runs on the compact rows. */
int stage_rag_ctx_rows(const int* cq, long long frames, int L, int* src_rows, void* stream);
/* Packed context features (csrc/packed.hip, tvqaplus_amd/packed.py): a stream arrives as the rows that exist -- frame-major, frame f
 * owning packed rows ptab[f].x .. ptab[f].x + ptab[f].y - 1 (ptab (frames, 2) int32: first packed row, len <= L) -- followed by ONE zero
 * row, the source of every padded position (the collate zero-fills behind a frame's length: tvqa_dataset.py:515-553).
 * stage_pack_ctx_rows: stage_rag_ctx_rows for such a stream -- src_rows[cq[f].x + l] = l < ptab[f].y ? ptab[f].x + l : zero_row for
 * l < cq[f].y; the input-MLP group then reads the packed buffer through the table.  L < 1 or frames * L >= 2^31:
 * STAGE_ERR_SHAPE, nothing launched.
 * stage_pack_unpack: the padded image for the paths that keep dense tensors.  EVERY row of dense (frames, L, row_bytes) is written in
 * one pass: row l < len is a byte copy of packed row start + l, every other row is zeros (no memset needed, any element type);
 * mask != NULL: the (frames, L) fp32 prefix mask as well; packed == dense == NULL: the mask alone.  row_bytes % 8 == 0,
 * 8 <= row_bytes <= 4096, 8-byte aligned bases (16-byte accesses when row_bytes % 16 == 0 and both bases are 16-byte aligned),
 * frames * L < 2^31 -- anything else is STAGE_ERR_SHAPE before a launch. */
int stage_pack_ctx_rows(const int* cq, const int* ptab, long long frames, int L, int zero_row, int* src_rows, void* stream);
int stage_pack_unpack(const void* packed, const int* ptab, void* dense, float* mask, long long frames, int L, int row_bytes, void* stream);
int stage_layernorm_gather_fwd(const float* x, const int* gather, const float* gamma, const float* beta, float* y, float* mean,
                               float* rstd, long long rows, int K, float eps, float p_drop, unsigned long long seed, void* stream);
int stage_layernorm_gather_bwd(const float* dy, const float* x, const int* gather, const float* mean, const float* rstd,
                               const float* gamma, float* dgamma, float* dbeta, long long rows, int K, float p_drop,
                               unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
int stage_l2norm_gather_fwd(const float* x, const int* gather, float* y, long long rows, int K, float eps, void* stream);
/* HALF-PRECISION FEATURE ROWS in the fp32 model (csrc/feat16.hip).  A loader may store the BERT / region features as fp16 or bf16
 * (half the host -> device bytes); these entry points read such rows in place and convert them in registers -- exactly -- so that no
 * fp32 image of the features (and, with l2, no normalised image) is ever written.  dtype: STAGE_DT_F16 / STAGE_DT_BF16.
 * First stage of the input MLP: [l2 != 0: F.normalize, model/stage.py:256] -> LayerNorm(K0) + inverted dropout (model/stage.py:85-91,
 * 98-104), row r reading x[src_rows ? src_rows[r] : r]; y0 (rows, K0) fp32, mean0 / rstd0 (rows).  The function, the dropout stream
 * (indexed by r) and the order of the floating-point sums are those of stage_l2norm[_gather]_fwd + stage_layernorm[_gather]_fwd on the
 * upcast rows.  The backward gives d gamma / d beta only (features are data), through a deterministic two-stage column reduction.
 * Requirements: K0 % 4 == 0, 4 <= K0 <= 1024 (stage_feat16_supported), x 8-byte aligned with contiguous rows, rows < 2^31; anything
 * else returns STAGE_ERR_SHAPE before a launch. */
#define STAGE_DT_F32 0    /* (stage_grp_input_mlp_* only: the entry points below take half-precision rows) */
#define STAGE_DT_F16 1
#define STAGE_DT_BF16 2
int stage_feat16_supported(int K0, int dtype);
int stage_feat16_ln_fwd(const void* x, int dtype, const int* src_rows, const float* gamma, const float* beta, float* y0, float* mean0,
                        float* rstd0, long long rows, int K0, int l2, float eps_ln, float eps_l2, float p_drop,
                        unsigned long long seed, void* stream);
size_t stage_feat16_ln_bwd_ws_bytes(int K0);
int stage_feat16_ln_bwd(const float* dy0, const void* x, int dtype, const int* src_rows, const float* mean0, const float* rstd0,
                        float* dgamma, float* dbeta, long long rows, int K0, int l2, float eps_l2, float p_drop,
                        unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
int stage_rag_fill_pooled(float* out, int* argmax, long long rows, int D, void* stream);      /* -1e10 / 0: model/stage.py:503 on an all-masked group */
int stage_rag_zero_dump(float* A_fc, const int* fmap, int N, int NA, int Li, int Lqa, int D, void* stream);
/* K1 with a frame-compact A / dA (model/context_query_attention.py:35-101; D == 128, the fast kernels only) */
/* cq (may be NULL): Q / Qn / dQraw / dQn hold compact context rows (above); q_mask stays dense (N, Li, Lr) */
int stage_str_attn_fwd_fc(const float* Cn, const float* Q, const float* c_mask, const float* q_mask, float* A_fc, float* S_raw,
                          float* S_norm, const int* fmap, const int* cq, int N, int NA, int Li, int Lqa, int Lr, int D, float scale,
                          float p_drop, unsigned long long seed, void* stream);
int stage_str_attn_bwd_fused_fc(const float* dA_fc, const float* dS_raw_ext, const float* Cn, const float* Q, const float* Qn,
                                const float* S_norm, const float* q_mask, float* dQraw, float* dQn, float* dCn, const int* fmap,
                                const int* cq, int N, int NA, int Li, int Lqa, int Lr, int D, float scale, void* ws, size_t ws_bytes,
                                void* stream);
/* [a, b, a*b] LayerNorm -> Linear -> ReLU (model/stage.py:381-385) on compact rows: a = QA rows, b = frame-compact rows */
int stage_cat3_ln_gemm_fwd_rag_supported(long long rows, long long a_rows, long long b_rows, int D);
int stage_cat3_ln_gemm_fwd_rag(const float* a, const float* b, const float* gamma, const float* beta, const float* W,
                               const float* bias, float* z, float* mean, float* rstd, float* y, unsigned* relu_mask_out,
                               const int* rowinfo, long long rows, long long a_rows, long long b_rows, int D, float eps,
                               float p_drop, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
int stage_cat3_dx_ln_bwd_rag_supported(long long rows, long long fc_rows, int D, int groups, int max_frames, int Lqa);
size_t stage_cat3_dx_ln_bwd_rag_ws_bytes(int groups, int max_frames, int Lqa);
/* wtab (may be NULL): balanced work table for stage_cat3_rag_work_groups() persistent workgroups (tvqaplus_amd/ragged.py:
 * RaggedTables.work_table -- [first segment of every workgroup, W + 1 ints padded to 4][(first slab, slabs) per group][segments
 * (group, first frame, end frame, workgroup)]): equal tile counts per workgroup; NULL: one workgroup per (group, chunk of max_frames) */
int stage_cat3_rag_work_groups(void);
int stage_cat3_dx_ln_bwd_rag(const float* dy, const unsigned* relu_mask, const float* W, const float* a, const float* b_fc,
                             const float* mean, const float* rstd, const float* gamma, float* da, float* db_fc, float* dgamma,
                             float* dbeta, const int* gdesc, const int* wtab, long long rows, long long fc_rows, int D, int groups,
                             int max_frames, int Lqa, float p_drop, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
/* the ragged backward with the Linear's gradients inside (csrc/cat3_bwd_dw.hip; see stage_cat3_bwd_dw): wtab is REQUIRED and built
 * for stage_cat3_bwd_dw_rag_work_groups() workgroups (= what stage_cat3_rag_work_groups() returns while this path is enabled) */
int stage_cat3_bwd_dw_rag_supported(long long rows, long long fc_rows, int D, int groups, int max_frames, int Lqa);
int stage_cat3_bwd_dw_rag_work_groups(void);
size_t stage_cat3_bwd_dw_rag_ws_bytes(int groups, int Lqa);
int stage_cat3_bwd_dw_rag(const float* dy, const unsigned* relu_mask, const float* W, const float* a, const float* b_fc,
                          const float* mean, const float* rstd, const float* gamma, const float* beta, float* da, float* db_fc,
                          float* dgamma, float* dbeta, float* dW, float* dc, const int* gdesc, const int* wtab, long long rows,
                          long long fc_rows, int D, int groups, int max_frames, int Lqa, float p_drop, unsigned long long seed,
                          void* ws, size_t ws_bytes, void* stream);
/* encoder block pieces on ragged sequences (model/encoder.py:35-52; model/stage.py:503 for the pooled LayerNorm) */
int stage_ln_dwconv_rag_fwd(const float* x, const float* res, const float* pe, float* sum_out, const float* gamma,
                            const float* beta, const float* w, const float* bias, float* h, float* mean, float* rstd,
                            const int* seq, long long S, int Lmax, int D, int k, float eps, float p_drop,
                            unsigned long long seed, void* stream);
int stage_ln_dwconv_rag_bwd(const float* dh, const float* xin, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, const float* w, float* dx, const float* dx_add, float* dgamma, float* dbeta,
                            float* dw, float* db, const int* seq, long long S, int Lmax, int D, int k, float p_drop,
                            unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
int stage_ln_masked_max_rag_fwd(const float* x, const float* res, float* sum_out, const float* gamma, const float* beta,
                                const float* qmask, float* out, int* argmax, float* mean, float* rstd, const int* seq,
                                long long S, int Lq, int K, float eps, void* stream);
int stage_ln_masked_max_rag_bwd(const float* dout, const int* argmax, const float* qmask, const float* xin, const float* mean,
                                const float* rstd, const float* gamma, float* dx, float* dgamma, float* dbeta,
                                const int* rowinfo, long long rows, int K, void* ws, size_t ws_bytes, void* stream);
/* K-groups on ragged rows (csrc/groups.hip "RAGGED TOKEN ROWS"): T = host array of the device tables fmap, gdesc, seq, rowinfo, cq
 * (cq NULL: dense context stream; Uc = rows of ctx / d_ctx) and -- the qa_ctx group, 6 entries -- wtab (the balanced work table of
 * stage_cat3_dx_ln_bwd_rag, or NULL).  The encoder group on these rows: stage_grp_encoder_* above with T != NULL. */
int stage_grp_qa_ctx_rag_supported(int N, int NA, int Li, int Lqa, int Lr, int D, long long U, long long Fc);
size_t stage_grp_qa_ctx_rag_arena_bytes(int N, int NA, int Lqa, int D, long long Ucap, long long Fc);
size_t stage_grp_qa_ctx_rag_bwd_tmp_bytes(int N, int NA, int Li, int Lqa, int Lr, int D, long long Ucap, long long Uc);
int stage_grp_qa_ctx_rag_fwd(const float* qa, const float* ctx, const float* qa_mask, const float* ctx_mask,
                             const float* const* P, float* mixed, float* S_raw, float* S_norm, const int* const* T, void* arena,
                             size_t arena_bytes, int* flags, int N, int NA, int Li, int Lqa, int Lr, int D, long long U,
                             long long Ucap, long long Fc, long long Uc, float scale, float p, const unsigned long long* seeds,
                             void* stream);
int stage_grp_qa_ctx_rag_bwd(const float* d_mixed, const float* dS_ext, const float* qa, const float* ctx, const float* ctx_mask,
                             const float* mixed, const float* S_norm, const float* const* P, float* const* G, float* d_qa,
                             float* d_ctx, const int* const* T, void* arena, size_t arena_bytes, const int* flags, void* tmp,
                             size_t tmp_bytes, int N, int NA, int Li, int Lqa, int Lr, int D, long long U, long long Ucap,
                             long long Fc, long long Uc, float scale, float p, const unsigned long long* seeds, void* stream);

/* ---- Flat Adam (main.py:63-66: clip_grad_norm_(model.parameters(), 10) + optimizer.step() with torch.optim.Adam) ----------------
 * The clip and the Adam update on the packed gradient buffer (csrc/flat_adam.hip; tvqaplus_amd/optim.py: FlatAdam): ONE call, two
 * launches on `stream`, no float atomics (fixed summation order: bitwise repeatable) and no device read-back.
 *   flat, m, v   (total) fp32, 16-byte aligned: the gradients of all parameters back to back, and Adam's two moments in the same layout
 *   seg_table    (n_seg, 3) int64 ON THE DEVICE: address of the parameter's data, its start offset in flat, its numel
 *   chunk_table  (n_chunk, 3) int32 ON THE DEVICE: segment, offset inside the segment, length -- at most 1024 consecutive elements of
 *                one segment per chunk, together tiling every segment (a chunk that does not fit its segment / flat is skipped)
 *   step         (n_seg) fp32: Adam's step count per parameter; active (n_seg) bytes: non-zero = the parameter has a gradient in this
 *                step.  An inactive parameter, its moments and its step are not touched (torch.optim.Adam skips grad = None)
 *   betas_host   HOST array {beta1, beta2} as double (the one host pointer of the call), read before it returns: 1 - beta and the bias corrections 1 - beta^t are formed in
 *                double as torch forms them (from a float beta2 = 0.999 they would be off by 5e-5); lr, eps, weight_decay, max_norm are
 *                used in fp32 and travel by value
 *   max_norm     > 0: flat is scaled by min(1, max_norm / (norm + 1e-6)) before the update and keeps the scaled values (what
 *                clip_grad_norm_ leaves in p.grad); <= 0: no clip, flat is only read.  weight_decay is Adam's L2 form (g + wd * p)
 *   norm_out     one float: the 2-norm of flat as the call found it; ws from stage_flat_adam_ws_bytes(total) (answers without a GPU)
 * STAGE_ERR_SHAPE: a NULL pointer, total <= 0, n_seg <= 0, n_chunk <= 0 (nothing to update), misaligned flat / m / v.               */
size_t stage_flat_adam_ws_bytes(long long total);
int stage_flat_adam_step(float* flat, float* m, float* v, const long long* seg_table, int n_seg, const int* chunk_table,
                         int n_chunk, float* step, const unsigned char* active, long long total, float lr, const double* betas_host,
                         float eps, float weight_decay, float max_norm, void* ws, size_t ws_bytes, float* norm_out, void* stream);

/* ---- Run meter (main.py:69-74, 90-94 training statistics; :173-183 validate(); eval/eval_tvqa_plus.py:14-69 temporal metrics) -----
 * The per-step bookkeeping of the caller's loop, accumulated in device memory (csrc/meter.hip; tvqaplus_amd/meter.py: RunMeter): every
 * call is ONE launch of one 256-thread workgroup, stream-ordered, no atomics, no read-back.  The caller reads the statistics by copying
 * the buffer to the host whenever it logs.  A METER BELONGS TO ONE STREAM: calls on it are ordered by that stream only.
 *
 * The buffer is caller-owned, 8-byte aligned, stage_meter_bytes(ring_cap) bytes, plain arrays (no struct crosses the ABI):
 *   byte   0  double f[8]      0 loss_sum  1 cls_sum  2 att_sum  3 ts_sum  4 grad_norm_sum  5 grad_norm_max  6 iou_sum  7 reserved
 *   byte  64  long long i[24]  0 steps  1 rows  2 correct  3 nonfinite_steps  4 ring_cursor (ring rows written)  5 ring_dropped
 *                              6 span_rows  7 span_right  8 asa (right and IoU >= 0.5)  9..17 recall bins IoU >= 0.1 .. 0.9
 *                              18 grad_norm_steps  19..23 reserved
 *   byte 256  ring: ring_cap rows of 2 bytes in arrival order, one 16-bit word each: bits 0-14 the predicted index, bit 15 the
 *             correct flag
 * Sums: each value is widened to double and added with one IEEE addition per call (bitwise repeatable).
 *
 * stage_meter_bytes needs no GPU (0 for ring_cap < 0).  stage_meter_reset: asynchronous zero fill of the whole buffer.
 * stage_meter_update: every pointer but `meter` may be NULL, its part is then skipped (P = 0 with NULL logits: the grad-norm-only call).
 *   logits (P, C <= 4096) + targets (P) int64: prediction = the first index holding a NaN if the row has one, else the first index of
 *     the maximum (what outputs.max(1)[1] gives on the host); correct = (prediction == target), so a negative or too-large target is
 *     never correct but counts in rows.  Ring rows at or beyond ring_cap are not written and counted in ring_dropped.
 *   loss, cls, att, ts, grad_norm: one device float each; att / ts are multiplied by att_w / ts_w in fp32 first (main.py:55-56).
 *     steps += 1 when any of loss / cls / att / ts is given; nonfinite_steps += !isfinite(loss[0]).
 * stage_train_loss_meter: stage_train_loss (same arguments, the same bits in loss and dlogits) and, in the same launch, the update with
 *   loss = its own loss, cls = ce * scale, att = att_w * att_loss[0], ts = ts_w * t_loss[0] on its own logits / targets.
 * stage_meter_spans: stage_answer_spans' decode (same limits: NA <= 64, Li <= 2048) of answer (N, NA) / t_prob (N, NA, Li, 2), then in
 *   double, with gt (N, 3) ON THE DEVICE = ground-truth start, end (seconds) and the offset (image_indices[0] % 6) / 3: predicted span
 *   [st * 2 + offset, (ed + 1) * 2 + offset] (inference.py:42-72), IoU = intersection / hull, 0 when the hull is 0
 *   (eval/eval_tvqa_plus.py:14-22); adds span_rows, span_right (answer == target), asa, the nine bins iou >= thd_host[k], iou_sum.
 *   thd_host: nine HOST doubles (np.arange(0.1, 1, 0.1) as the evaluation forms them), read before the call returns and passed to
 *   the kernel by value.  rows_out (N, 3) int32, if given, receives what stage_answer_spans would write.
 * STAGE_ERR_SHAPE before any launch: NULL or misaligned meter, negative sizes, C / NA / Li outside the limits, a NULL required pointer. */
size_t stage_meter_bytes(long long ring_cap);
int stage_meter_reset(void* meter, long long ring_cap, void* stream);
int stage_meter_update(void* meter, long long ring_cap, const float* logits, const long long* targets, int P, int C, const float* loss,
                       const float* cls, const float* att, const float* ts, float att_w, float ts_w, const float* grad_norm,
                       void* stream);
int stage_train_loss_meter(const float* logits, const long long* targets, const float* att_loss, const float* t_loss,
                           const float* scale_dev, float scale_host, float att_w, float ts_w, float* loss, float* dlogits, int P, int C,
                           void* stream, void* meter, long long ring_cap);
int stage_meter_spans(void* meter, const float* answer, const float* t_prob, const long long* targets, const double* gt,
                      const double* thd_host, int N, int NA, int Li, int* rows_out, void* stream);

/* ---- Grounding meter (eval/eval_tvqa_plus.py:94-146 + eval/maskrcnn_voc/voc_eval.py as tvqaplus_amd/evaluation.py restates them:
 *      load_predictions :309-329, detection_map :225-282, _pairwise_iou :199-207) ---------------------------------------------------
 * The fourth validation metric next to the run meter's three: the detection records of the grounding mAP, appended to ONE caller-owned
 * device buffer by ONE launch per validation batch (csrc/grounding.hip; tvqaplus_amd/grounding.py: GroundingMeter), one wavefront per
 * task.  The AP is a host-side sort over the records (evaluation.average_precision).  A task is one (example, annotated image, label)
 * triple of the GROUND-TRUTH answer; `tasks` (T, 8) int64 ON THE DEVICE, one row per task:
 *   0 word_off    offset of the statement's Lqa word ids in `words` (qas[b, answer, 0])
 *   1 score_off   offset of scores[b, answer, frame, 0, 0] in `scores`: row w of the task is scores[score_off + w * Lr .. + Lr)
 *   2 label       the word id, 0 .. 2^31 - 1
 *   3 box_first   first region box of the image in `region_boxes`        4 n_boxes  their number (region r < n_boxes has a box)
 *   5 gt_first    first ground-truth box of (image, label) in `gt_boxes`  6 n_gt     their number, >= 1
 *   7 spare (0)
 * region_boxes (n_region_boxes, 4), gt_boxes (n_gt_boxes, 4): float32 x1 y1 x2 y2 (finite), on the device.
 * Per task (load_predictions + the inner loop of detection_map): the positions w (ascending) with words[word_off + w] == label (the
 * comparison runs here, on the device word ids); of each such row the regions r with score >= thd (fp32; a NaN is never kept:
 * stage_att_predict's rule); these detections in descending score order (equal scores: lower w, then lower r) each take the FIRST
 * ground-truth box of the largest IoU -- _pairwise_iou on boxes whose far edges were incremented by 1, the same fp32 operations in the
 * same order, compiled without contraction -- and match when that IoU is not below iou_thd and the box is not taken yet.
 *
 * The buffer is caller-owned, 8-byte aligned, stage_grounding_bytes(capacity) bytes:
 *   byte  0  unsigned long long c[8]   0 cursor (records reserved; the first min(cursor, capacity) slots are written)
 *                                      1 dropped (records that did not fit)  2 tasks  3 detections (of the tasks that emitted)
 *                                      4 overflow  5 bad  6..7 reserved
 *   byte 64  capacity records of 8 bytes: int32 (bits 0-30 the label, bit 31 the match), then the fp32 score.  Order across tasks:
 *            unspecified (one atomic add on the cursor per task; the records are written with plain vector stores).
 * A task writes nothing and is counted in `bad` when its row fails a bound -- label outside 0 .. 2^31 - 1, word_off + Lqa > n_words,
 * a score row outside n_scores, box_first + n_boxes > n_region_boxes, n_gt < 1 or gt_first + n_gt > n_gt_boxes, any of them
 * negative -- or when it has a kept region r >= n_boxes; in `overflow` when the label holds more than 8 positions or n_gt > 32
 * (table bounds are judged first, then the limits, then the rows).  No read is made through an unchecked offset.
 * stage_grounding_supported: 1 for 1 <= Lqa <= 64 and 1 <= Lr <= 64 (needs no GPU); stage_grounding_bytes needs no GPU (0 for
 * capacity < 0).  stage_grounding_reset: asynchronous zero fill.  stage_grounding_update: STAGE_ERR_SHAPE before any launch for an
 * unsupported Lqa / Lr, a NULL or misaligned buffer or table, a negative size; T == 0 launches nothing. */
int stage_grounding_supported(int Lqa, int Lr);
size_t stage_grounding_bytes(long long capacity);
int stage_grounding_reset(void* buf, long long capacity, void* stream);
int stage_grounding_update(void* buf, long long capacity, const float* scores, long long n_scores, const long long* words,
                           long long n_words, const long long* tasks, int T, const float* region_boxes, long long n_region_boxes,
                           const float* gt_boxes, long long n_gt_boxes, int Lqa, int Lr, float thd, float iou_thd, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STAGE_HIP_H */

/*
 * s2t_hip.h -- C ABI of libs2t_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * speech-translation forward/backward hot path of FBK-fairseq-ST (`conv_transformer`).
 *
 * The reference has NO native interface on this path: its boundary is Python (fairseq's
 * register_model / register_task / register_criterion plug-in surface) and every
 * FLOP is an ATen call.  Each entry point below therefore names the reference *call site* whose
 * arithmetic it replaces (file:line under the reference tree).  The Python side of the boundary
 * (fbk_fairseq_st_amd/*.py) mirrors the reference's module interface and binds these symbols with
 * ctypes; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless noted; no ownership
 *     transfer; outputs are caller-allocated; calls are stream-ordered on `stream` (a hipStream_t,
 *     NULL = default stream) and re-entrant per stream; no call synchronises the device.  Internal scratch
 *     (workgroup partial sums of s2t_lsce / s2t_kd_loss / s2t_grad_norm_clip / s2t_conv1_bwd_bn, the cached work
 *     tables of s2t_wgrad_group) is keyed by (current device, stream) under a mutex: concurrent calls of one entry
 *     point on different streams, devices or host threads do not share it.
 *   - dtype: S2T_F32 = 0 (parity path, exact-f32 MFMA), S2T_BF16 = 1 (bf16 storage, f32 accumulate).
 *   - return 0 on success; -22 (EINVAL) bad argument; -95 (ENOTSUP) unsupported shape/dtype;
 *     -(1000 + hipError_t) when the HIP runtime reported an error at launch.
 *   - time-major activations: X[t][b][:] row index t*B + b (the reference's T x B x C).
 */
#ifndef S2T_HIP_H
#define S2T_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S2T_F32 0
#define S2T_BF16 1

/* epilogue selector of s2t_gemm */
#define S2T_ACT_NONE 0
#define S2T_ACT_RELU 1      /* fairseq/utils.py:390-408 ("relu") */
#define S2T_ACT_GELU 2      /* fairseq/modules/gelu.py:24-25 (erf form, computed in f32); pre-activation -> aux_out */
#define S2T_ACT_RELU_BWD 3  /* out = acc * (aux > 0)            (aux = forward post-activation) */
#define S2T_ACT_GELU_BWD 4  /* out = acc * gelu'(aux)           (aux = forward pre-activation)  */
/* ReLU with a 1-bit record instead of a re-read of the activations in the backward pass (the FFN of transformer_layer.py:171-176: the data
 * gradient of fc2 needs only "was the stored, post-dropout activation > 0").  S2T_ACT_RELU_MASK = S2T_ACT_RELU that also writes the
 * record to aux_out; S2T_ACT_RELU_BWD_MASK = S2T_ACT_RELU_BWD with aux = that record.  The record is s2t_gemm_relu_mask_bytes(M, N, K)
 * bytes in the tile / lane order of the 256-wide kernel (opaque: valid only between two products of the same M, N); products that kernel
 * does not take get S2T_ENOTSUP with these codes -- ask s2t_gemm_relu_mask_bytes first (0 = use S2T_ACT_RELU / S2T_ACT_RELU_BWD). */
#define S2T_ACT_RELU_MASK 5
#define S2T_ACT_RELU_BWD_MASK 6

/* ---- library info ------------------------------------------------------------------------- */
/* Weight gradient of the second subsampling convolution (nn.Conv2d(C, C, 3, stride 2, padding 1), conv_transformer.py:348-354), all
 * nine taps in one pass: gw[co][tap*C + ci] += sum_{t4,b,f4} dpre[t4][b][f4][co] * y1n[b][2 t4+kh-1][2 f4+kw-1][ci].
 * bf16, C = 64 (S2T_ENOTSUP otherwise: use the gathered s2t_gemm_gather products). */
int s2t_conv2_wgrad(int dtype, const void* dpre, const void* y1n, float* gw, int B, int T2, int F2, int C, void* stream);
/* Forward of the same convolution as a direct kernel (input rows staged once in LDS, no row maps):
 * z2[t4][b][f4][co] = act(bias[co] + sum y1n[b][2 t4+kh-1][2 f4+kw-1][ci] * w2p[co][(kh*3+kw)*C + ci]), act = S2T_ACT_RELU | S2T_ACT_GELU (GELU also
 * writes the pre-activation to `pre`).  w2p = s2t_permute_conv_w(mode 0).  bf16, C = 64, F2 <= 48 (S2T_ENOTSUP otherwise: s2t_gemm_gather). */
int s2t_conv2_fwd(int dtype, const void* y1n, const void* w2p, const float* bias, void* z2, void* pre, int B, int T2, int F2, int C,
                  int act, void* stream);
/* Data gradient of the same convolution, all four pixel-parity classes in one launch, with the dropout mask of y1n on the way out:
 * dy1n[b][t2][f2][ci] = dropout(sum_{taps reaching (t2, f2)} sum_co dpre[t4][b][f4][co] * w[co][ci][kh][kw], p_drop, seed) (mask indexed by the
 * element's position in dy1n).  w2q = s2t_permute_conv_w(mode 1).  bf16, C = 64, F2 <= 47 (S2T_ENOTSUP otherwise). */
int s2t_conv2_dgrad(int dtype, const void* dpre, const void* w2q, void* dy1n, int B, int T2, int F2, int C, float p_drop,
                    unsigned long long seed, void* stream);
/* The K largest logits of every row, descending, with their columns (scripts/generate_topk.py:64-66: the teacher dump of word-level
 * knowledge distillation).  x [rows][V] with row stride ld; vals f32 [rows][K], idx i32 [rows][K]. */
int s2t_topk(int dtype, const void* x, float* vals, int* idx, long rows, int V, int ld, int K, void* stream);
/* TimeStretch + SpecAugment in one pass (examples/speech_recognition/modules/time_stretch.py:18-57, specaugment.py:44-112; applied by
 * tasks/speech_recognition.py:254-258): out[b][t][:] = x[b][row_map[b][t]][:] (row_map NULL = identity, -1 = zero row), zeroed inside
 * tmask[b][i] = (t0, width) and fmask[b][i] = (f0, width).  x [B][T][F] f32, out [B][To][F] f32 (out != x). */
int s2t_augment(const float* x, float* out, const int* row_map, const int* fmask, const int* tmask, int B, int T, int To, int F,
                int nF, int nT, void* stream);
/* Host: frame-budget batching of utterance indices (fairseq/data/data_utils_fast.pyx:16-68 batch_by_size_fast; caller
 * fairseq/data/data_utils.py:200-234).  lens[idx] = frames of utterance idx; out_flat[n], out_offsets[n + 1]. */
int s2t_host_batch_by_size(const long long* indices, long long n, const long long* lens, long long max_tokens,
                           long long max_sentences, int bsz_mult, long long* out_flat, long long* out_offsets,
                           long long* n_batches);
int s2t_abi_version(void);                       /* bumps when a signature OR a workspace contract changes.  8 (round 5): s2t_ctc_loss's la / lb
                                                  * workspaces are B*T*S2T_CTC_ROW(Lmax) floats holding log2 values with per-step offsets
                                                  * (a phase-1 workspace of a version-7 library is unusable by a version-8 phase 2);
                                                  * the "gemm4w" option of s2t_set_option is gone.  9 (round 6): the s2t_decode_* entry points */
const char* s2t_build_info(void);                /* "gfx950 <date> ..." */

/* ---- GEMM with fused epilogue (MFMA) --------------------------------------------------------
 * C[M,N] = act( alpha * op(A)[M,K] . op(B)[K,N] + bias[N] ) + residual[M,N]      (accumulate: C += ...)
 *   trans_a = 0: A is [M][K];  1: A is [K][M]        trans_b = 0: B is [N][K] (nn.Linear weight);  1: B is [K][N]
 *   in_dtype: A, B.   out_dtype: C, residual, aux, aux_out.   bias is always f32.
 *   splitk > 1: K is split over gridDim.z and partial products are added with f32 atomics into C
 *               (C must be f32 and pre-initialised; no bias/act/residual).
 * Replaces: F.linear at fairseq/modules/multihead_attention.py:190-208,356 (q/k/v/out projections),
 *   fairseq/modules/transformer_layer.py:132-134,358-360 (fc1 + activation, fc2 + residual),
 *   examples/speech_recognition/models/conv_transformer.py:227 (fc3 + activation), :279 (ctc_fc),
 *   fairseq/models/transformer.py:784-788 (output projection), and their autograd backward
 *   (dX = dY W: trans_b = 1;  dW = dY^T X: trans_a = trans_b = 1). */
int s2t_gemm(int in_dtype, int out_dtype, int trans_a, int trans_b, int M, int N, int K,
             const void* A, int lda, const void* B, int ldb, void* C, int ldc,
             const float* bias, const void* residual, int ldr, const void* aux, void* aux_out, int ldaux,
             int act, int accumulate, int splitk, float alpha, void* stream);

/* Same kernel with row gather / scatter, used to run Conv2d(64->64, 3x3, stride 2, pad 1)
 * (conv_transformer.py:203-206, 2nd iteration) and its backward as implicit GEMMs over channels-last
 * activations:  mapA[(k/periodA)*M + r] = source row of A for output row r and k-block (tap) k/periodA
 * (-1 = zero padding);  mapB[k] = source row of a [K][N] B operand;  mapC[r] = destination row.
 * p_drop > 0: dropout (Philox(seed, row*N+col)) on the activated value before the residual add
 * (transformer_layer.py:123-124,133-136: x = residual + dropout(linear(...))). */
int s2t_gemm_gather(int in_dtype, int out_dtype, int trans_a, int trans_b, int M, int N, int K,
                    const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                    const float* bias, const void* residual, int ldr, const void* aux, void* aux_out, int ldaux,
                    int act, int accumulate, int splitk, float alpha,
                    const int* mapA, int periodA, const int* mapB, const int* mapC,
                    float p_drop, unsigned long long seed, void* stream);
/* Size in bytes of the 1-bit ReLU record of an [M][N] bf16 product with reduction length K (S2T_ACT_RELU_MASK / S2T_ACT_RELU_BWD_MASK
 * above), or 0 when products of that shape do not run on the kernel that keeps such records. */
size_t s2t_gemm_relu_mask_bytes(int M, int N, int K);

/* Weight (and bias) gradients of MANY Linears in one launch (bf16 operands, f32 gradients; csrc/wgrad_group.hip):
 *     dW_p[n_out][n_in] += dY_p[tokens][n_out]^T X_p[tokens][n_in]      db_p[n_out] += column sums of dY_p   (db may be NULL)
 * Replaces, for the Transformer blocks, the per-Linear autograd products of F.linear (fairseq/modules/multihead_attention.py:190-208,
 * fairseq/modules/transformer_layer.py:132-134): nothing reads a weight gradient before the optimizer / the gradient all-reduce, so
 * the caller may queue the (dY, X) pairs of several layers during backward and submit them together.  Every 256 x 256 tile of every
 * dW is owned by one workgroup for the whole token range: no split-K, no atomics
 * (when the tile count does not fill the last round of one tile per CU, the tiles of that round are cut along the token range and
 * meet in f32 atomics).  Requirements: ldy, ldx multiples of 8 elements and >= the column count rounded up to 8, 16-byte aligned
 * operand bases; a dW must not appear twice in one call.  `probs` is a HOST array (uploaded stream-ordered with the work list).
 * Refused with S2T_EINVAL, before anything is uploaded or launched (no dW or db of the list is touched): a problem that misses these
 * requirements, has a NULL dY, X or dW or a size below 1; n_out or n_in below 8 (one 16-byte chunk of bf16: such products go to
 * s2t_linear_wgrad); an operand of 4 GiB or more (tokens * ld * 2 bytes: the kernel addresses operands by 32-bit byte offsets);
 * a negative n or, with n > 0, a NULL `probs`.  n = 0 is S2T_OK and does nothing. */
typedef struct S2TWgradProblem {
    const void* dY; const void* X; float* dW; float* db;
    int n_out, n_in, tokens, ldy, ldx, ldw;
} S2TWgradProblem;
int s2t_wgrad_group(int n, const S2TWgradProblem* probs, void* stream);
/* The same for f32 operands (the parity mode; csrc/wgrad_f32.hip): exact-f32 MFMA, every 128 x 128 tile of every dW owned by one workgroup
 * over all its tokens (no atomics: results do not depend on scheduling), all tiles of all products dealt to two workgroups per CU,
 * longest reductions first (when the longest tiles do not fill their last round of 512 workgroups, the tiles of that round are cut along
 * the token range and meet in f32 atomics).  Requirements: ldy, ldx multiples of 4 elements and >= the column count rounded up to 4,
 * 16-byte aligned operand bases; a dW must not appear twice in one call.  Refusals as above, without the minimum width and the 4 GiB
 * limit: S2T_EINVAL for a problem that misses the requirements, a NULL dY, X or dW, a size below 1, a negative n or a NULL `probs`
 * with n > 0; n = 0 is S2T_OK. */
int s2t_wgrad_group_f32(int n, const S2TWgradProblem* probs, void* stream);

/* out[n] += sum_m X[m][n]  (bias gradients of every nn.Linear above; f32 atomics) */
/* Parameter gradients of a Linear in one pass over dY (autograd of F.linear: fairseq/modules/multihead_attention.py:190-208,
 * fairseq/modules/transformer_layer.py:132-134): dW[n_out][n_in] += dY[tokens][n_out]^T X[tokens][n_in] (f32) and, if db is not
 * NULL, db[n_out] += column sums of dY. */
int s2t_linear_wgrad(int in_dtype, int n_out, int n_in, int tokens, const void* dY, int ldy, const void* X, int ldx,
                     float* dW, int ldw, float* db, int splitk, void* stream);
int s2t_colsum(int dtype, const void* X, int ld, int M, int N, float* out, void* stream);

/* ---- fused multi-head attention ---------------------------------------------------------------
 * Replaces fairseq/modules/multihead_attention.py:155-177 (F.multi_head_attention_forward) and
 * :316-355 (own bmm/softmax/bmm path): scores, key-padding (-inf), causal mask
 * (fairseq/models/transformer.py:798-810), fp32 softmax, dropout on P, P.V.  Scores never reach HBM.
 * X[t][b][h][j] = X + t*x_st + b*x_sb + h*head_dim + j (element strides);  head_dim in {32, 64}.
 * klen[b] = number of valid (non-padded) keys of batch b, NULL = all Tk (padding is a suffix on this
 * path: conv_transformer.py:293-300, transformer.py:739-741).  LSE [B][H][Tq] f32 (saved for backward). */
int s2t_attn_fwd(int dtype, int head_dim, int B, int H, int Tq, int Tk,
                 const void* Q, long q_st, long q_sb, const void* K, long k_st, long k_sb,
                 const void* V, long v_st, long v_sb, void* O, long o_st, long o_sb, float* LSE,
                 const int* klen, int causal, int dist_penalty, float scale, float p_drop, unsigned long long seed, void* stream);
/* Head-averaged attention probabilities of ONE layer, recomputed from its q and k (the fused kernels never materialise P):
 * out[b][tq][tk] = mean over the first heads_used heads of softmax_tk(scale * q . k), 0 past klen[b]; f32 [B][Tq][Tk], Tk <= 2048.
 * Replaces the need_attn / need_head_weights return of fairseq/modules/multihead_attention.py:342-355 as consumed by
 * fairseq/models/transformer.py:756-782 (alignment_layer / alignment_heads; generate.py --print-alignment, ensemble averaging). */
int s2t_attn_probs_avg(int dtype, int head_dim, int B, int H, int Tq, int Tk, const void* Q, long q_st, long q_sb,
                       const void* K, long k_st, long k_sb, const int* klen, int heads_used, float scale, float* out, void* stream);
/* Backward of s2t_attn_fwd (flash-style recomputation; Delta [B][H][Tq] f32 is workspace). */
int s2t_attn_bwd(int dtype, int head_dim, int B, int H, int Tq, int Tk,
                 const void* Q, long q_st, long q_sb, const void* K, long k_st, long k_sb,
                 const void* V, long v_st, long v_sb, const void* O, long o_st, long o_sb,
                 const void* dO, long do_st, long do_sb, const float* LSE, float* Delta,
                 void* dQ, long dq_st, long dq_sb, void* dK, long dk_st, long dk_sb, void* dV, long dv_st, long dv_sb,
                 const int* klen, int causal, int dist_penalty, float scale, float p_drop, unsigned long long seed, void* stream);
/* Dropout keep-bit record: the forward writes the keep decision of every (query, key) pair, one bit each, and the backward reads
 * them instead of hashing every pair again in each of its two kernels.  The decisions are the hash's own, so results are bit-equal
 * to s2t_attn_fwd / s2t_attn_bwd.
 * s2t_attn_keep_bytes = size of the record of a bf16 call of this shape, or 0 when the call would not run the second-generation
 * kernels on their plain path: head_dim 64, no causal mask, no distance penalty, p_drop >= 2^-16, B H Tq ((Tk + 3) & ~3) < 2^34,
 * Tq > 64 (not the short-query kernels, which hash once per pair as it is) and Tq >= 128 or (Tq >= "attn_v2_min_tq" and Tk >= 128),
 * "attn_v1" off.  It follows those two options: ask again after s2t_set_option, and keep them fixed between a forward and its backward.
 * Layout, in 32-bit words, with nq = ceil(Tq / 128) query blocks and nk = ceil(Tk / 64) key tiles:
 *     word  (((b * H + h) * nq + bx) * nk + t) * 256 + 64 * w + lane          (w = 0..3, lane = 16 * q + r16, q = 0..3, r16 = 0..15)
 *     bit   16 * qb + 4 * j + r  (qb = 0..1, j = 0..3, r = 0..3)  =  1 when the pair
 *           query 128 * bx + 32 * w + 16 * qb + r16,  key 64 * t + 16 * j + 4 * q + r    is kept.
 * Key tiles at or past klen[b] are not written; bits of queries >= Tq and of keys >= klen[b] mean nothing.
 * s2t_attn_fwd_keep / s2t_attn_bwd_keep = s2t_attn_fwd / s2t_attn_bwd plus the record (4-byte aligned device memory of that size).
 * keep = NULL is s2t_attn_fwd / s2t_attn_bwd exactly.  With a record, a call that s2t_attn_keep_bytes answers with 0, that is not
 * bf16, or whose O / K / V layout leaves the second-generation forward (O strides % 4, O & 7, K / V rows beyond 32-bit offsets)
 * gets S2T_ENOTSUP and launches nothing.  The backward must get the record its forward wrote (same shape, klen, p_drop, seed). */
size_t s2t_attn_keep_bytes(int head_dim, int B, int H, int Tq, int Tk, int causal, int dist_penalty, float p_drop);
int s2t_attn_fwd_keep(int dtype, int head_dim, int B, int H, int Tq, int Tk,
                      const void* Q, long q_st, long q_sb, const void* K, long k_st, long k_sb,
                      const void* V, long v_st, long v_sb, void* O, long o_st, long o_sb, float* LSE,
                      const int* klen, int causal, int dist_penalty, float scale, float p_drop, unsigned long long seed,
                      void* keep, void* stream);
int s2t_attn_bwd_keep(int dtype, int head_dim, int B, int H, int Tq, int Tk,
                      const void* Q, long q_st, long q_sb, const void* K, long k_st, long k_sb,
                      const void* V, long v_st, long v_sb, const void* O, long o_st, long o_sb,
                      const void* dO, long do_st, long do_sb, const float* LSE, float* Delta,
                      void* dQ, long dq_st, long dq_sb, void* dK, long dk_st, long dk_sb, void* dV, long dv_st, long dv_sb,
                      const int* klen, int causal, int dist_penalty, float scale, float p_drop, unsigned long long seed,
                      const void* keep, void* stream);

/* ---- LayerNorm(fairseq/modules/layer_norm.py:29-32; eps 1e-5; rows of D <= 1024) ------------------ */
int s2t_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y,
                      float* mean, float* rstd, int M, int D, float eps, void* stream);
/* dx = LN'(dy) + dres (dres optional: the residual branch of a pre-LN block); dgamma/dbeta += (f32).
 * dx_drop (optional): a second output = s2t_dropout(dx, p_drop, seed), i.e. the gradient that enters the
 * residual-branch dropout of the block that consumes dx, written in the same pass (bit-identical to the
 * separate call). */
int s2t_layernorm_bwd(int dtype, const void* dy, const void* x, const float* mean, const float* rstd,
                      const float* gamma, const void* dres, void* dx, float* dgamma, float* dbeta,
                      int M, int D, void* dx_drop, float p_drop, unsigned long long seed, void* stream);

/* ---- one Transformer layer per call ------------------------------------------------------------------
 * fairseq/modules/transformer_layer.py:87-139 (encoder layer) and :243-377 (decoder layer), pre-LN form, bf16 path: the kernels of
 * a layer in the order the host engine issues them (LayerNorm, projections with fused bias / residual / dropout epilogues, flash
 * attention, FFN with the 1-bit ReLU record or the GELU pre-activation), behind ONE entry point per direction.  Nothing new is
 * computed here -- every launch is one of the entry points above -- but a small batch (8 utterances per GPU: SURVEY.md 8-d) is
 * bound by the HOST's launch rate, and a layer is 7-13 launches forward and 9-20 backward.
 * S2TLayerDesc: shapes, rates and parameter pointers of one layer (fixed per model and batch shape); S2TLayerCall: the operands of
 * one call.  Activations are time-major rows (t*B + b) of D elements; `ws` keeps what the backward needs (s2t_layer_ws_bytes),
 * `tmp` is scratch of the backward (s2t_layer_bwd_tmp_bytes; it holds the dY operands of the layer's weight-gradient products,
 * which s2t_layer_bwd does NOT launch: it appends them to `items` for a later s2t_wgrad_group, so `ws`, `tmp`, `x` and `enc` must
 * stay alive until then).  Dropout seeds are per site, exactly the ones the per-kernel path passes. */
typedef struct S2TLayerDesc {
    int dtype, decoder;                 /* S2T_BF16; 0 = self-attention + FFN, 1 = + encoder attention in between */
    int T, B, D, heads, ffn, Ts;        /* Ts: source positions (decoder) */
    int gelu, causal, dist_penalty;     /* activation (0 ReLU); mask / distance penalty of the self-attention */
    float ln_eps, p_drop, p_attn, p_act;
    const void *w_qkv, *w_o, *w_xq, *w_xkv, *w_xo, *w_fc1, *w_fc2;                  /* [out][in], compute dtype */
    const float *b_qkv, *b_o, *b_xq, *b_xkv, *b_xo, *b_fc1, *b_fc2;
    const float *ln1_g, *ln1_b, *lnx_g, *lnx_b, *ln2_g, *ln2_b;
    float *g_w_qkv, *g_w_o, *g_w_xq, *g_w_xkv, *g_w_xo, *g_w_fc1, *g_w_fc2;         /* f32 gradient slices (backward) */
    float *g_b_qkv, *g_b_o, *g_b_xq, *g_b_xkv, *g_b_xo, *g_b_fc1, *g_b_fc2;
    float *g_ln1_g, *g_ln1_b, *g_lnx_g, *g_lnx_b, *g_ln2_g, *g_ln2_b;
} S2TLayerDesc;
typedef struct S2TLayerCall {
    int training;
    const int* self_klen; const int* enc_klen;            /* key lengths [B] or NULL */
    unsigned long long seed_sa_attn, seed_sa_out, seed_xa_attn, seed_xa_out, seed_ffn_act, seed_ffn_out;
    const void* x; const void* enc; void* y; void* ws;    /* forward: y = layer(x [T*B][D], enc [Ts*B][D]) */
    /* backward: dy = gradient w.r.t. y; dy_drop = dropout(dy) with the FFN's output mask when the producer of dy already wrote it
     * (else NULL); dx, and when nxt_p > 0 also dx_drop = dropout(dx, nxt_p, nxt_seed) for the consumer of dx; the encoder-output
     * gradient is written (denc_accumulate = 0) or added to denc [Ts*B][D] */
    const void* dy; const void* dy_drop; void* dx; void* dx_drop; float nxt_p; unsigned long long nxt_seed;
    void* denc; int denc_accumulate; void* tmp;
    S2TWgradProblem* items; int max_items; int n_items;   /* host array; n_items is advanced by the products appended */
} S2TLayerCall;
size_t s2t_layer_ws_bytes(const S2TLayerDesc* L, int training);
size_t s2t_layer_bwd_tmp_bytes(const S2TLayerDesc* L);
int s2t_layer_fwd(const S2TLayerDesc* L, S2TLayerCall* c, void* stream);
int s2t_layer_bwd(const S2TLayerDesc* L, S2TLayerCall* c, void* stream);

/* ---- convolutional subsampler (conv_transformer.py:202-232) ----------------------------------------
 * conv1: x [B][T][F] f32 -> y [B][T2][F2][C] (channels-last) = act(conv3x3 s2 p1 + bias), act = S2T_ACT_RELU | S2T_ACT_GELU
 * (--activation-fn, conv_transformer.py:140-142,212); with GELU the pre-activation goes to `pre` (same shape, needed by the
 * backward; NULL for ReLU).  Also the BatchNorm sums: sums[c] += y, sums[C+c] += y^2 (double, caller zeroes).  C in {32, 64, 128}. */
int s2t_conv1_fwd(int dtype, const float* x, const float* w, const float* bias, void* y, void* pre, double* sums,
                  int B, int T, int F, int C, int act, void* stream);
/* dw[c][3][3] += , db[c] += from dpre [B][T2][F2][C] (gradient after the ReLU mask) */
int s2t_conv1_bwd(int dtype, const float* x, const void* dpre, float* dw, float* db, int B, int T, int F, int C, void* stream);
/* s2t_bn_bwd_apply + s2t_conv1_bwd in one pass (the gradient w.r.t. the convolution's output is never written): dw / db += as
 * s2t_conv1_bwd would from dpre = act'(.) * BatchNorm'(dyn) (arguments as s2t_bn_bwd_apply: y = BatchNorm input, pre = pre-activation
 * for GELU or NULL, sums from s2t_chan_sums(mode 1)); dgamma / dbeta += */
int s2t_conv1_bwd_bn(int dtype, const float* x, const void* dyn, const void* y, const void* pre, const float* mean, const float* rstd,
                     const float* gamma, const double* sums, float* dw, float* db, float* dgamma, float* dbeta, int B, int T, int F,
                     int C, double count, int training, void* stream);
/* per-channel double sums over a channels-last [P][C] tensor: mode 0 (y, y^2); mode 1 (dyn, dyn*xhat) */
int s2t_chan_sums(int dtype, const void* y, const void* dyn, const float* mean, const float* rstd,
                  double* sums, long P, int C, int mode, void* stream);
/* nn.BatchNorm2d statistics (conv_transformer.py:212,364-368): training -> batch stats from sums, running
 * stats momentum update (unbiased var), num_batches += 1; eval -> running stats.  scale/shift for s2t_bn_apply. */
int s2t_bn_finalize(const double* sums, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    long long* num_batches, float* mean, float* rstd, float* scale, float* shift,
                    double count, int C, int training, float momentum, float eps, void* stream);
/* yn = dropout(y*scale + shift, p_drop, seed): the normalisation and the dropout that follows it (conv_transformer.py:212-214)
 * in one pass; the mask / rounding are those of s2t_dropout on the normalised tensor */
int s2t_bn_apply(int dtype, const void* y, const float* scale, const float* shift, void* yn, long n, int C,
                 float p_drop, unsigned long long seed, void* stream);
/* BatchNorm backward fused with the derivative of the activation in front of it: the ReLU mask (y > 0) when pre == NULL, else
 * gelu'(pre); sums from s2t_chan_sums(mode 1); dgamma/dbeta += */
int s2t_bn_bwd_apply(int dtype, const void* dyn, const void* y, const void* pre, const float* mean, const float* rstd,
                     const float* gamma, const double* sums, void* dpre, float* dgamma, float* dbeta,
                     long n, int C, double count, int training, void* stream);
/* fc3 weight [N][C*F] (k = c*F+f, conv_transformer.py:225-226) <-> channels-last k' = f*C+c */
int s2t_permute_cf(int dst_dtype, const float* src, void* dst, int N, int C, int F, int mode, void* stream);
/* conv2 weight [Co][Ci][3][3] <-> implicit-GEMM operand layouts (see subsample.hip): 0 forward, 1 data gradient by parity
 * class, 2 weight gradient back to the master layout */
int s2t_permute_conv_w(int dst_dtype, const float* src, void* dst, int Co, int Ci, int mode, void* stream);
/* dst[t][b][:] = dropout(src[t][b][:] + sinusoid[(t < len[b]) ? t+1 : 0][:])  (positional_embedding_audio.py:21-27; the add and the
 * F.dropout of conv_transformer.py:229-232 in one pass; src may equal dst; p_drop = 0: no dropout; mask = s2t_dropout's on the flat index) */
int s2t_add_pos(int dtype, const void* src, void* dst, const float* table, const int* len, int T, int B, int D,
                float p_drop, unsigned long long seed, void* stream);

/* ---- CTC compression (conv_transformer.py:278-291, 385-426) -----------------------------------------
 * pred[b][t] = first arg-max of softmax(logits[t][b][:]) (bit-exact integer path), pmax = its probability.
 * Logit rows have a stride of ld >= V elements (here and in the two loss kernels): the producer GEMM pads the
 * row stride to a multiple of 8 so that every GEMM touching the logits can use 16-byte loads. */
/* lse (optional, [T*B] f32): the rows' log-sum-exps, for s2t_ctc_loss over the same logits (phase | 4) */
int s2t_ctc_argmax(int dtype, const void* logits, int* pred, float* pmax, float* lse, int T, int B, int V, int ld, void* stream);
/* run-length collapse inside len[b]; seg/run_start/run_len [B][T] int32, new_len [B] int64, w [B][T] f32
 * strategy 0 avg, 1 weighted, 2 softmax */
int s2t_ctc_rle(const int* pred, const float* pmax, const long long* len, int* seg, int* run_start, int* run_len,
                long long* new_len, float* w, int T, int B, int strategy, void* stream);
/* out[j][b][:] = sum_{t in run j} w[b][t] x[t][b][:]  (zeros for new_len[b] <= j < Tout) */
int s2t_ctc_compress_fwd(int dtype, const void* x, const float* w, const int* run_start, const int* run_len,
                         const long long* new_len, void* out, int T, int B, int D, int Tout, void* stream);
int s2t_ctc_compress_bwd(int dtype, const void* dout, const float* w, const int* seg, void* dx, int T, int B, int D,
                         int accumulate, void* stream);

/* ---- losses ------------------------------------------------------------------------------------
 * F.log_softmax + F.ctc_loss(reduction="sum", zero_infinity=True) (CTC_loss.py:143-151) and its gradient
 * w.r.t. the logits [T][B][V].  Workspaces: lse [T*B], la/lb [B*T*S2T_CTC_ROW(Lmax)], nll [B] (all f32; la/lb rows are padded
 * to the positions of the recursion's wave and hold log2 values shifted per frame: private to the two passes).
 * loss_sum[0] += sum_b nll_b (caller zeroes). grad is multiplied by grad_scale and, if given, by the device scalar
 * grad_scale_dev[0] (the upstream gradient autograd hands to backward).  phase 0: loss and gradient in one call;
 * phase 1: loss only (workspaces kept by the caller); phase 2: the gradient from the workspaces of a phase-1 call;
 * phase | 4: `lse` already holds the row log-sum-exps of these logits (written by s2t_ctc_argmax), skip that pass.
 * Limits of THIS entry point: transcripts of at most S2T_CTC_MAX_TARGET units (Lmax, the padded width of `targets`) and
 * vocabularies of at most S2T_CTC_MAX_VOCAB entries; beyond them the call returns -95 (ENOTSUP).  s2t_ctc_loss_any below has
 * no such limits (the reference's F.ctc_loss has none either); the host side (kernels.py ctc_loss) routes larger batches there. */
#define S2T_CTC_MAX_TARGET 511
#define S2T_CTC_MAX_VOCAB 40704
/* row stride of the la / lb workspaces: the 2*Lmax+1 extended-target positions rounded up to 64 x {1, 2, 4, 8, 16} */
#define S2T_CTC_ROW(Lmax) (2 * (Lmax) + 1 <= 64 ? 64 : 2 * (Lmax) + 1 <= 128 ? 128 : 2 * (Lmax) + 1 <= 256 ? 256 : 2 * (Lmax) + 1 <= 512 ? 512 : 1024)
int s2t_ctc_loss(int dtype, const void* logits, const long long* targets, const long long* tgt_len, const int* in_len,
                 float* lse, float* la, float* lb, float* nll, void* grad, float* loss_sum,
                 int T, int B, int V, int ld, int Lmax, int blank, float grad_scale, int phase, const float* grad_scale_dev,
                 void* stream);
/* The same loss and gradient for any transcript length and any vocabulary size (csrc/ctc.hip: the recursion keeps its state in
 * the workspace, the gradient pass needs no vocabulary-sized LDS row).  Arguments and `phase` as s2t_ctc_loss; la / lb are
 * replaced by ONE workspace `ws` of s2t_ctc_loss_any_workspace(T, B, Lmax, V) bytes:
 *     4 * (2 * B * T * R + B * Q)   with R = 2 * Lmax + 1 and Q = Lmax + 1, each rounded up to a multiple of 64
 * (alpha and beta rows of R floats per frame, then Q ints per utterance).  Private to the two phases of one loss; a phase-2 call
 * must pass the same ws, lse, nll and inputs as its phase-1 call.  V is not part of the size (it is taken for future layouts). */
size_t s2t_ctc_loss_any_workspace(int T, int B, int Lmax, int V);
int s2t_ctc_loss_any(int dtype, const void* logits, const long long* targets, const long long* tgt_len, const int* in_len,
                     float* lse, void* ws, float* nll, void* grad, float* loss_sum,
                     int T, int B, int V, int ld, int Lmax, int blank, float grad_scale, int phase, const float* grad_scale_dev,
                     void* stream);
/* ---- CTC decoding (csrc/ctc_decode.hip): transcripts from CTC logits [T][B][V] (f32 / bf16, row stride ld >= V), frames
 * t >= in_len[b] (int32 [B], clamped to [0, T]) never reach a result, arithmetic in f32.  Per row x with m = max x, a = the FIRST
 * index of that maximum and R = sum_{v != a} exp(x_v - m):   lp_v = (x_v - m) - log1p(R)   (the log-softmax, exact near 0).
 * Common refusals, before anything is launched or written: S2T_OK at once for T*B <= 0; S2T_EINVAL for a NULL pointer, ld < V,
 * V < 2, blank outside [0, V), beam / cand / nbest < 1, nbest > beam; S2T_ENOTSUP for a dtype other than f32 / bf16, beam > 16,
 * cand > 16, cand > V - 1.  No atomics, no host read: a row phase (one wave per row) then one wave per sentence.
 *
 * Greedy (best path): pred_t = a of frame t; runs of equal predictions collapse, blank runs drop (`a _ a` two tokens, `a a` one).
 * tokens [B][T] int32 (the first n_tok[b] written), frames [B][T][2] int32 = (first frame, one past the last frame) of each
 * token's run, tok_score [B][T] f32 = sum of lp_pred over that run, score [B] = the same sum over all in_len[b] frames (blank
 * frames included).  ws: s2t_ctc_greedy_workspace(T, B) = 8*T*B bytes. */
size_t s2t_ctc_greedy_workspace(int T, int B);
int s2t_ctc_greedy(int dtype, const void* logits, const int* in_len, void* ws, int* tokens, int* n_tok, int* frames,
                   float* tok_score, float* score, int T, int B, int V, int ld, int blank, void* stream);
/* Prefix beam search without a language model (Hannun et al. 2014), natural-log space.  State: at most `beam` prefixes (token
 * strings) with pb / pnb = log-probability of the alignments of the frames so far that end in blank / non-blank; start
 * {(): pb 0, pnb -inf}.  Per frame, C = the `cand` non-blank symbols of highest logit (ties: lower index), tot = pb (+) pnb,
 * (+) = logaddexp:   new[p].pb (+)= lp_blank + tot;   c in C, c == last(p): new[p].pnb (+)= lp_c + pnb, new[p+c].pnb (+)= lp_c + pb;
 * c in C, c != last(p): new[p+c].pnb (+)= lp_c + tot.  A prefix is its token STRING (64-bit hash + length): the extension of p and
 * the updates of a live p+c meet in one entry, wherever p came from.  Entries of total -inf are no prefixes; the `beam` highest
 * totals survive.  Output, best first: tokens [B][nbest][T] int32, lens [B][nbest], scores [B][nbest] f32 (lens 0 / scores -inf
 * behind the n_hyp[b] <= nbest hypotheses that exist); in_len[b] == 0: the empty hypothesis, score 0.
 * ws: s2t_ctc_prefix_beam_workspace(T, B, beam, cand, nbest) = 4*T*B*(2*beam + 2*cand + 1) bytes rounded up to 256 (the trie of
 * (parent, token) nodes, then the rows' candidates). */
size_t s2t_ctc_prefix_beam_workspace(int T, int B, int beam, int cand, int nbest);
int s2t_ctc_prefix_beam(int dtype, const void* logits, const int* in_len, void* ws, int* tokens, int* lens, float* scores,
                        int* n_hyp, int T, int B, int V, int ld, int blank, int beam, int cand, int nbest, void* stream);
/* ---- CTC forced alignment (csrc/ctc_align.hip): the most likely CTC path among those that collapse to a GIVEN transcript.
 * logits, in_len, lp_v, blank as in the CTC decoding section above (n = in_len[b] clamped to [0, T]); targets int64 [B][Lmax] and
 * tgt_len int64 [B] as s2t_ctc_loss takes them.  For a sentence of L = tgt_len[b] tokens y the extended sequence has S = 2L + 1
 * states, z_s = blank for even s and y[(s-1)/2] for odd s.  v[0][0] = lp_0[blank], v[0][1] = lp_0[y_0], every other state -inf;
 * for t >= 1   v[t][s] = lp_t[z_s] + max over the allowed predecessors   s;  s-1 if s >= 1;  s-2 if s is odd, s >= 3 and
 * y[(s-1)/2] != y[(s-3)/2].  Among equal values the HIGHER predecessor state wins (stay over advance over skip).  The path ends at
 * frame n-1 in the better of S-1 and S-2, on equal values in S-1; for L = 0 in state 0.  All arithmetic in f32, no atomics; a
 * sentence's result does not depend on B or on its place in the batch.
 * status [B] int32: 0 aligned (n = 0 with L = 0: score 0);  1 infeasible: the best end value is -inf (too few frames for the
 * tokens plus the blanks that repeated tokens force, n = 0 with L > 0, a needed column -inf on every frame);  2 tgt_len[b] outside
 * [0, Lmax], or one of the first L tokens outside [0, V) or equal to the blank (nothing outside the row is read for it).
 * states [B][T] int32: the state of every frame t < n; -1 for t >= n and for the whole row when status != 0.
 * frames [B][Lmax][2] int32: (first frame, one past the last frame) of token i, the convention of s2t_ctc_greedy's frames.
 * tok_score [B][Lmax] f32: the sum of lp over the token's frames.  score [B] f32: the sum over all n frames, blank frames
 * included; -inf when status != 0.  Entries i >= L of frames / tok_score are not written; for status != 0 the first L are
 * (-1, -1) / -inf, and when L itself is out of range nothing is written to the two arrays.
 * NaN logits: the path is unspecified; the call terminates and stays inside its buffers.
 * Refusals, before anything is launched: S2T_OK at once for T*B <= 0; S2T_EINVAL for a NULL pointer, ld < V, V < 2, blank outside
 * [0, V), Lmax < 0, T*B > 2^31 - 1; S2T_ENOTSUP for a dtype other than f32 / bf16 and for Lmax > S2T_CTC_ALIGN_MAX_TARGET.
 * Two launches, no host read: a row phase (one wave per row writes the sentence's L + 1 emissions) and a sentence phase -- one wave
 * per sentence with 1 to 16 states per lane in registers for 2*Lmax + 1 <= 1024, one 256-thread workgroup with two LDS rows above.
 * ws: s2t_ctc_align_workspace(T, B, Lmax) = 4*T*B*(Lmax + 1 + W) bytes rounded up to 256, with W = 64 for 2*Lmax + 1 <= 1024 and
 * ceil((2*Lmax + 1) / 16) above (the emissions [T*B][Lmax + 1] f32, then W dwords of 2-bit back-pointers per sentence and frame);
 * 0 for an empty problem or an Lmax out of range. */
#define S2T_CTC_ALIGN_MAX_TARGET 4095
size_t s2t_ctc_align_workspace(int T, int B, int Lmax);
int s2t_ctc_align(int dtype, const void* logits, const int* in_len, const long long* targets, const long long* tgt_len, void* ws,
                  int* states, int* frames, float* tok_score, float* score, int* status, int T, int B, int V, int ld, int Lmax,
                  int blank, void* stream);
/* ---- CTC segmentation of long recordings (csrc/ctc_segment.hip): s2t_ctc_align's rule with free ends, for transcripts given as a
 * list of utterances, with every utterance's frames and how well it fits.  logits, in_len, targets, tgt_len, lp_v, blank as above.
 * A recording of L = tgt_len[b] tokens is the concatenation of U = n_utt[b] utterances; utt_end int64 [B][Umax] holds their
 * cumulative end offsets (strictly ascending, the first >= 1, the last == L), n_utt int64 [B].
 * Rule: states, z_s, predecessors, tie rule, initialisation and end decision are s2t_ctc_align's.  flags bit 0 (free_start): state 0
 * costs 0 on every frame instead of lp_t[blank], audio before the text is absorbed at no cost; bit 1 (free_end): the same for state
 * S - 1.  With flags = 0 the rule IS s2t_ctc_align's, and states, frames, tok_score and score come out with the same bits.
 * status [B] int32: 0 segmented;  1 no path (the best end value is -inf; n = 0);  2 refused: tgt_len[b] outside [1, Lmax], n_utt[b]
 * outside [1, Umax], offsets that break the rule above, or one of the first L tokens equal to the blank or outside [0, V).  Nothing
 * outside the row is read for a refused recording and, apart from status, none of its outputs is written.
 * states [B][T], frames [B][Lmax][2], tok_score [B][Lmax], score [B]: as s2t_ctc_align gives them, the free frames counting 0 in
 * score; for status 1 states -1, the first L of frames / tok_score (-1, -1) / -inf, score -inf.
 * utt_frames [B][Umax][2] int32: the first frame of the utterance's first token, one past the last frame of its last token (blank
 * frames between two utterances belong to neither).  utt_score [B][Umax] f32: the sum of lp_t[z_{state_t}] over that span, the blanks
 * inside it included.  utt_conf_mean: utt_score / the span's frame count.  utt_conf_min: the lowest mean of lp_t[z_{state_t}] over
 * `window` consecutive frames inside the span, the span's own mean when it is shorter than `window`.  Entries u >= U are not
 * written; for status 1 the first U are (-1, -1) / -inf.
 * A recording's result depends neither on B, nor on its place in the batch, nor on Lmax, Umax or T.  All arithmetic in f32, no atomics,
 * no memset, no host read.  NaN logits: the path is unspecified; the call terminates and stays inside its buffers.
 * Refusals, before anything is launched, in this order: S2T_OK at once for T*B <= 0; S2T_EINVAL for a NULL pointer, V < 2, ld < V,
 * blank outside [0, V), Lmax < 1, Umax < 1, T*B > 2^31 - 1, flags outside [0, 3]; S2T_ENOTSUP for a dtype other than f32 / bf16,
 * Lmax > S2T_CTC_SEGMENT_MAX_TARGET, Umax > S2T_CTC_SEGMENT_MAX_UTT, window outside [1, S2T_CTC_SEGMENT_MAX_WINDOW].
 * Three launches: a row phase (one wave per row writes its maximum and log-sum-exp, 8 bytes), a recording phase (one workgroup of up
 * to 1,024 threads per recording, 2 to 32 states per thread in registers, the logits of a thread's tokens gathered from the frame's
 * row, 2-bit back-pointers, the backward walk staged through LDS in blocks of 64 frames), an utterance phase (one workgroup per
 * utterance).
 * ws: s2t_ctc_segment_workspace(T, B, Lmax, Umax) = 4*T*B*(3 + ceil((2*Lmax + 1) / 16)) bytes rounded up to 256 (per row its maximum
 * and log-sum-exp, per frame the path's emission, then one dword of back-pointers per frame and 16 states); 0 for an empty problem or
 * an Lmax or Umax out of range. */
#define S2T_CTC_SEGMENT_MAX_TARGET 16383
#define S2T_CTC_SEGMENT_MAX_UTT 4096
#define S2T_CTC_SEGMENT_MAX_WINDOW 4096
#define S2T_CTC_SEGMENT_FREE_START 1
#define S2T_CTC_SEGMENT_FREE_END 2
size_t s2t_ctc_segment_workspace(int T, int B, int Lmax, int Umax);
int s2t_ctc_segment(int dtype, const void* logits, const int* in_len, const long long* targets, const long long* tgt_len,
                    const long long* utt_end, const long long* n_utt, void* ws, int* states, int* frames, float* tok_score, float* score,
                    int* utt_frames, float* utt_score, float* utt_conf_mean, float* utt_conf_min, int* status, int T, int B, int V, int ld,
                    int Lmax, int Umax, int blank, int flags, int window, void* stream);
/* ---- Edit-distance alignment of token sequences (csrc/edit_align.hip): cost, step counts and optionally the path, per sentence.
 * One sentence is a pair `a` (n tokens, the rows) and `b` (m tokens, the columns).  The three integer costs `cs`, `ca`, `cb`, each
 * in [1, 255], price a substitution, an `a` token left alone, and a `b` token left alone.
 * Recursion:
 *   - D[0][0] = 0.
 *   - D[0][j] = D[0][j-1] + cb (step B).
 *   - D[i][0] = D[i-1][0] + ca (step A).
 *   - Otherwise best = D[i-1][j-1] + (a[i-1] == b[j-1] ? 0 : cs), which is step M (match) or step S (substitution).
 *   - Then, if D[i][j-1] + cb < best, take step B.
 *   - Then, if D[i-1][j] + ca < best, take step A.
 *   - Both comparisons are strict and are made in that order.
 *   - This is exactly wer_utils.EditDistance(False).align and align_errors in runtime.hip.  The preference is diagonal first,
 *     then left, then up.
 * Path and outputs:
 *   - The path is the one the chosen steps give from (n, m) back to (0, 0).
 *   - counts[b] = (M, S, B, A) are the numbers of each step on that path.
 *   - cost[b] = D[n][m].
 *   - With `a` the decoded transcript, `b` the target and costs (4, 3, 3), S + B + A is the reference's compute_ctc_uer error
 *     count for the sentence.
 *   - Note that a minimum-cost path under (4, 3, 3) is not always a minimum-count path, so the counts must come from this path
 *     and no other.
 * Collapse mode:
 *   - A flag makes a row of `a` a row of per-frame labels with a_len[b] frames.
 *   - Repeats are collapsed, then `blank` is dropped, as s2t_host_ctc_uer does, in the same call.
 *   - n is the number of survivors.
 *   - The call writes n to a_n [B] and, when the pointer is given, the collapsed tokens to a_out [B][Amax].
 * Optional path output:
 *   - With ops != NULL, ops [B][Amax + Bmax] (uint8) gets the step codes in forward order: 0 for M, 1 for S, 2 for B, 3 for A.
 *   - n_ops [B] gets the path's length.
 *   - Entries behind it are not written.
 * Status and limits:
 *   - status [B] is 0 for done and 2 for refused.  A sentence is refused when its length lies outside [0, padded width].  Nothing
 *     else is written for that sentence, counts and cost included.
 *   - A sentence's result does not depend on B or on its place in the batch.
 *   - No atomics and no host read.
 *   - Padded widths are Bmax <= S2T_EDIT_MAX_B = 4095 and Amax <= S2T_EDIT_MAX_A = 32767.
 *   - Tokens are int32 or int64, chosen per side by an element-size argument (a_elem, b_elem: 4 or 8).
 * Operands: a [B][Amax] and a_len [B] have a_elem bytes per element, b [B][Bmax] and b_len [B] have b_elem (what s2t_ctc_greedy and
 * s2t_ctc_argmax give is int32, the criterion's targets are int64); tokens compare as 64-bit integers.  counts [B][4], cost [B],
 * status [B], a_n [B], n_ops [B] are int32; a_out has a's element size.  Without collapse mode `blank` is ignored, a_out is not
 * touched, and a_n (optional) gets a_len[b].  a_n is required in collapse mode, n_ops with ops.
 * One launch: one wave per sentence with 1 to 16 columns per lane in registers and the rows skewed across the lanes for
 * Bmax + 1 <= 1024, one 256-thread workgroup with the same skew above.  A cell carries its cost and the four counts of its path,
 * so no matrix is stored unless ops is asked for.
 * ws: s2t_edit_align_workspace(B, Amax, Bmax, want_ops) = 8*B*Amax bytes rounded up to 256 (room for the collapsed tokens when a_out
 * is NULL in collapse mode) plus, with want_ops, 4*B*(Amax + 1)*ceil((Bmax + 1) / 16) bytes rounded up to 256 (one dword of 2-bit
 * steps per row and 16 columns); 0 for B <= 0 or a width out of range.  ws may be NULL when neither part is used.
 * Refusals, before anything is launched: S2T_OK at once for B <= 0; S2T_EINVAL for a NULL required pointer (a, a_len, b, b_len,
 * counts, cost, status; a_n in collapse mode; n_ops with ops; ws when it is used), a cost outside [1, 255], a negative width, an
 * element size other than 4 or 8; S2T_ENOTSUP for Amax > S2T_EDIT_MAX_A or Bmax > S2T_EDIT_MAX_B. */
#define S2T_EDIT_MAX_A 32767
#define S2T_EDIT_MAX_B 4095
size_t s2t_edit_align_workspace(int B, int Amax, int Bmax, int want_ops);
int s2t_edit_align(const void* a, const void* a_len, int a_elem, const void* b, const void* b_len, int b_elem, int B, int Amax,
                   int Bmax, int cs, int ca, int cb, int collapse, long long blank, void* ws, int* counts, int* cost, int* status,
                   int* a_n, void* a_out, unsigned char* ops, int* n_ops, void* stream);
/* ---- BLEU n-gram statistics of token sequences (csrc/bleu_stats.hip): the ten numbers of the reference's bleu_add
 * (clib/libbleu/libbleu.cpp, called per sentence by fairseq/bleu.py:Scorer.add), per sentence.
 * One sentence is a pair `hyp` (hyp_len tokens) and `ref` (ref_len tokens), with three token ids `pad`, `eos`, `unk`.
 * Trim, each side inside its given length:
 *   - Leading `pad` tokens are dropped.
 *   - Then trailing tokens equal to `eos` or `pad` are dropped, but never the first remaining token: a sentence that is only [eos]
 *     keeps length 1 and its token is eos; [eos, eos, eos] becomes [eos].
 *   - `pad` or `eos` in the interior are ordinary tokens.
 *   - A side that is empty after the left trim has length 0 and all its numbers are 0.  The reference reads out of bounds there;
 *     this is the one deviation.
 * Totals: predlen and reflen are the trimmed lengths; for n = 1 .. 4, count_n = max(predlen - n + 1, 0).
 * Matches:
 *   - match_n = the sum over distinct n-grams g of min(occurrences of g in the trimmed hyp, occurrences of g in the trimmed ref).
 *   - It is 0 when either side is shorter than n.
 *   - A reference token equal to `unk` never matches anything (bleu.py:83-86 rewrites it to -999).  A hypothesis `unk` still
 *     counts in count_n.  unk < 0 switches this off.
 * Comparison: tokens are int32 or int64 per side (hyp_elem, ref_elem: 4 or 8; a side's lengths have its element size) and compare
 * as 64-bit integers.  n-grams are compared token by token, not by hash: apart from a 64-bit FNV collision the result is the
 * reference's.
 * The kernel computes match_n position by position: hypothesis position i matches at order n iff the number of earlier hypothesis
 * positions with the same n-gram is below the number of reference positions with it.  One launch, one sentence per workgroup, no
 * atomics, no host read; a sentence's result does not depend on the batch around it.  One wave per sentence for
 * Hmax <= S2T_BLEU_WAVE_LEN, one 256-thread workgroup up to S2T_BLEU_GROUP_LEN, one of 1,024 threads above; both padded widths
 * up to S2T_BLEU_MAX_LEN.
 * Outputs: stats [B][10] int32 in the order of the reference's BleuStat -- reflen, predlen, match1, count1, ... match4, count4;
 * status [B] int32, 0 for done and 2 for refused.  A sentence is refused when a length lies outside [0, padded width] or its
 * ref_row entry lies outside [0, Rrows); its stats are written as zeros.
 * ref_row: NULL for identity (then Rrows must equal B); otherwise sentence b is scored against row ref_row[b] of ref [Rrows][Rmax]
 * with length ref_len[ref_row[b]], so that an n-best list shares its reference without copies.
 * Refusals, before anything is launched: S2T_OK at once for B <= 0; S2T_EINVAL for a NULL required pointer (hyp, hyp_len, ref,
 * ref_len, stats, status), a negative width, an element size other than 4 or 8, Rrows != B without a map (Rrows < 0 with one),
 * pad == eos, or unk >= 0 equal to pad or eos; S2T_ENOTSUP for a width above S2T_BLEU_MAX_LEN. */
#define S2T_BLEU_MAX_LEN 4095
#define S2T_BLEU_WAVE_LEN 64
#define S2T_BLEU_GROUP_LEN 256
int s2t_bleu_stats(const void* hyp, const void* hyp_len, int hyp_elem, const void* ref, const void* ref_len, int ref_elem,
                   const int* ref_row, int B, int Hmax, int Rmax, int Rrows, long long pad, long long eos, long long unk,
                   int* stats, int* status, void* stream);
/* ---- BLEU statistics of every candidate against every pseudo-reference of its sentence (csrc/bleu_pairs.hip): the pairwise step of
 * minimum-Bayes-risk selection over n-best lists.  The rule of a pair is s2t_bleu_stats's, above, with the candidate as the
 * hypothesis and the pseudo-reference as the reference (trim, clipped matches, a reference-side `unk` matches nothing, an all-pad
 * side has length 0, tokens int32 or int64 per side compared as 64-bit integers); it is not restated here.
 * Operands: cand [Rc][Hmax] with cand_len [Rc] and ref [Rr][Pmax] with ref_len [Rr] (lengths in the dtype of their tokens);
 * cand_sent int32 [Rc], the sentence of each candidate row; ref_off int32 [B + 1], the pseudo-references of sentence b are the rows
 * ref_off[b] .. ref_off[b+1] - 1 of ref.  cand and ref may be the same matrix (hypotheses against themselves): nothing is copied or
 * repeated.  M is the call's widest list; the caller states it (it knows the lists' shapes), the kernel reads no list beyond it.
 * Outputs: stats [Rc][M][10] int32 in the order of s2t_bleu_stats (reflen = the pseudo-reference's trimmed length, predlen = the
 * candidate's), status [Rc][M] int32, 0 for done and 2 for refused.  Every element of both is written: no initialisation is needed.
 * Behind a sentence's list (k >= its length) stats and status are 0.  Refused, with zeros, beside ordinary pairs that are unaffected:
 *   - a pair whose pseudo-reference length lies outside [0, Pmax];
 *   - every pair of a candidate whose length lies outside [0, Hmax];
 *   - all M entries of a candidate whose cand_sent lies outside [0, B), or whose sentence's offsets descend, leave [0, Rr] or span
 *     more than M rows: such a row has no list to be behind of.
 * Kernel: one launch, one candidate position per thread, no atomics, no host read, no memset; a pair's result does not depend on
 * the batch around it.  A workgroup takes one candidate row and a slice of S2T_MBR_SLICE entries of its list (a candidate with one
 * workgroup for its whole list leaves most of the chip idle at the sizes lists have: measured); one wave per candidate
 * for Hmax <= S2T_MBR_WAVE_LEN, 256 threads up to S2T_MBR_GROUP_LEN, 1,024 threads up to S2T_MBR_MAX_LEN.  The candidate is trimmed
 * and staged in LDS once per workgroup and every position counts the earlier positions that hold its n-grams once; the counts stay
 * in registers.  Then the workgroup walks its slice in chunks of S2T_MBR_CHUNK(Pmax, bytes per staged token) pseudo-references --
 * the whole slice unless the rows are wide: a chunk is staged in LDS behind one barrier, every position counts the positions of each
 * staged pseudo-reference that hold its n-grams, and the matches are summed over the workgroup behind a second barrier.  Tokens
 * are staged as 32-bit when both sides are int32 and as 64-bit otherwise.
 * Refusals, before anything is launched: S2T_OK at once for Rc <= 0 or M == 0; S2T_EINVAL for a NULL required pointer (cand,
 * cand_len, ref, ref_len, cand_sent, ref_off, stats, status), a negative width, B, Rr or M, an element size other than 4 or 8,
 * pad == eos, or unk >= 0 equal to pad or eos; S2T_ENOTSUP for a width above S2T_MBR_MAX_LEN or M above S2T_MBR_MAX_LIST.  (The
 * widths cover translation hypotheses; the 4,095 of s2t_bleu_stats serve document-length references, which a list of hypotheses does
 * not have.) */
#define S2T_MBR_MAX_LEN 1024
#define S2T_MBR_MAX_LIST 256
#define S2T_MBR_WAVE_LEN 64
#define S2T_MBR_GROUP_LEN 256
#define S2T_MBR_SLICE 8
#define S2T_MBR_CHUNK_BYTES 32768
#define S2T_MBR_CHUNK(Pmax, elem) \
    (S2T_MBR_CHUNK_BYTES / (((Pmax) + 4) * (elem)) > S2T_MBR_SLICE ? S2T_MBR_SLICE : S2T_MBR_CHUNK_BYTES / (((Pmax) + 4) * (elem)))
int s2t_bleu_pairs(const void* cand, const void* cand_len, int cand_elem, const void* ref, const void* ref_len, int ref_elem,
                   const int* cand_sent, const int* ref_off, int Rc, int B, int Hmax, int Pmax, int Rr, int M, long long pad,
                   long long eos, long long unk, int* stats, int* status, void* stream);
/* ---- chrF / chrF++ statistics of detokenised token rows (csrc/chrf_stats.hip): per pair of rows the character n-gram totals and
 * clipped matches of the orders 1 to 6 and the word n-gram ones of the orders 1 and 2, from which chrF (Popovic 2015, 2017; the
 * rule sacrebleu's CHRF applies to whitespace-split text) follows.  Compatibility is by this restated rule, not by
 * a captured fixture.
 * Text of a row: token id t maps to the piece pieces[piece_off[t] .. piece_off[t + 1]), uint32 code points in which the value
 * S2T_CHRF_SEP marks a word break.  The text is the concatenation of the pieces of the row's first `len` tokens; runs of SEP,
 * leading and trailing ones included, act as one break and no SEP stays in the character stream.  piece_off has V + 2 entries:
 * entry V is what a reference-side token equal to `unk` maps to (unk < 0: no special rendering; the hypothesis side always takes
 * entry unk).  The host builds the table (chrf_scorer.piece_table): pad, eos and bos have empty pieces.
 * Characters: with h and r the two streams, for n = 1 .. char_order: hyp_n = max(|h| - n + 1, 0), ref_n likewise, and
 * match_n = the sum over distinct n-grams g of min(occurrences in h, occurrences in r).
 * Words: the maximal SEP-free runs.  A word of one character stays whole; otherwise, if its last character is one of the 32 ASCII
 * punctuation characters (Python's string.punctuation) it becomes two words, all but the last character and the last; otherwise,
 * if its first character is one of them, the first and the rest; otherwise it stays whole.  Word n-grams for n = 1 .. word_order
 * are counted and clipped the same way; two words are equal iff their code points are.
 * Everything is an exact integer: n-grams and words are compared element by element, never by a hash.
 * Operands: hyp [Hrows][Hmax] and ref [Rrows][Rmax], int32 or int64 tokens per side (hyp_elem, ref_elem: 4 or 8), lengths in the
 * tokens' dtype.  hyp_row / ref_row: int32 [P] or NULL; pair p is row hyp_row[p] against row ref_row[p], NULL means row p (then the
 * side has P rows).  Nothing is copied or repeated; one matrix may serve both sides.  n_pieces: the elements of `pieces`.
 * Outputs: stats [P][24] int32 -- (hyp_n, ref_n, match_n) for the character orders 1 .. 6, then the word orders 1 .. 2; the orders
 * above the configured ones are zeros -- and status [P] int32, 0 done or 2 refused.  A pair is refused, with zeros, beside ordinary
 * pairs that are unaffected, for a map entry outside its matrix, a length outside [0, padded width], a token outside [0, V) inside
 * a length, offsets of a piece that descend or leave [0, n_pieces], or a side of more than S2T_CHRF_MAX_CHARS characters.  Every
 * element of both outputs is written: no initialisation is needed.
 * Kernel: one launch, one pair per workgroup, no atomics, no host read, no memset; a pair's result does not depend on the batch
 * around it.  Piece lengths are prefix-summed over the row, the code points expanded into LDS, and matches counted position by
 * position as in s2t_bleu_stats (position i matches at order n iff the earlier hypothesis positions with its n-gram are fewer than
 * the reference positions with it; one common-prefix length serves all orders).  Words get the index of their first equal
 * occurrence across both sides and are counted over those ids.  256 threads for Hmax <= S2T_CHRF_GROUP_LEN tokens, 1,024 above
 * (the character count is not known to the host; inside, a wave without positions skips the loops).
 * Limits: S2T_CHRF_MAX_LEN tokens of padded width (the width of s2t_bleu_pairs: lists of hypotheses) and S2T_CHRF_MAX_CHARS
 * characters per side (at four bytes per code point both sides take 32.8 KB of LDS, with the words' starts and ids 65.6 KB of the
 * CU's 160 KB: two workgroups per CU with words, four without).
 * Refusals, before anything is launched: S2T_OK at once for P <= 0; S2T_EINVAL for a NULL required pointer (hyp, hyp_len, ref,
 * ref_len, pieces, piece_off, stats, status), a negative width, V or n_pieces, an element size other than 4 or 8, a side without a
 * map whose rows are not P (with one: negative), unk >= V, char_order outside [1, S2T_CHRF_MAX_CHAR_ORDER] or word_order outside
 * [0, S2T_CHRF_MAX_WORD_ORDER]; S2T_ENOTSUP for a width above S2T_CHRF_MAX_LEN. */
#define S2T_CHRF_MAX_LEN 1024
#define S2T_CHRF_MAX_CHARS 4095
#define S2T_CHRF_GROUP_LEN 64
#define S2T_CHRF_MAX_CHAR_ORDER 6
#define S2T_CHRF_MAX_WORD_ORDER 2
#define S2T_CHRF_SEP 0xffffffffu
int s2t_chrf_stats(const void* hyp, const void* hyp_len, int hyp_elem, const void* ref, const void* ref_len, int ref_elem,
                   const int* hyp_row, const int* ref_row, int P, int Hmax, int Rmax, int Hrows, int Rrows,
                   const unsigned int* pieces, const int* piece_off, int n_pieces, int V, long long unk, int char_order,
                   int word_order, int* stats, int* status, void* stream);
/* ---- Unit rows of detokenised token rows (csrc/text_units.hip): per pair of rows the words or the characters of the two texts as
 * int32 rows that s2t_edit_align takes, so that WER and CER of the text come from two launches without a host read.
 * Text of a row: as in s2t_chrf_stats above, unchanged -- the pieces of the row's first `len` tokens concatenated, a run of
 * S2T_CHRF_SEP (leading and trailing runs included) one break, the reference side renders `unk` through table entry V (unk < 0:
 * no special rendering), a token outside [0, V) refuses the pair.  Words are the maximal SEP-free runs; there is no punctuation
 * split here (that is chrF++'s rule).
 * Units, by `mode`:
 *   0  words.  A word's unit is the index of its first equal occurrence in the list "hypothesis words, then reference words"
 *      (lengths and code points compared, no hash): two units of a pair are equal iff the words are.  Units of different pairs do
 *      not compare.
 *   1  characters with spaces: the code points of the text with one U+0020 between consecutive words (no leading or trailing one).
 *   2  characters without spaces: the code points alone.
 * Operands: hyp [Hrows][Hmax] and ref [Rrows][Rmax], int32 or int64 tokens per side (hyp_elem, ref_elem: 4 or 8), lengths in the
 * tokens' dtype.  hyp_row / ref_row: int32 [P] or NULL; pair p is row hyp_row[p] against row ref_row[p], NULL means row p (then the
 * side has P rows).  Nothing is copied or repeated; one matrix may serve both sides.  pieces, piece_off, n_pieces, V, unk: the piece
 * table, as in s2t_chrf_stats.
 * Outputs, all int32: hyp_units [P][Uh], ref_units [P][Ur], hyp_n [P], ref_n [P], status [P] (0 done, 2 refused).  Every element of
 * hyp_n, ref_n and status is written.  hyp_units[p][0 .. hyp_n[p]) and ref_units[p][0 .. ref_n[p]) are written; entries behind them
 * are not.  A pair is refused -- status 2, hyp_n = ref_n = 0 and nothing else written, beside ordinary pairs that are unaffected --
 * for a map entry outside its matrix, a length outside [0, padded width], a token outside [0, V) inside a length, offsets of a piece
 * that descend or leave [0, n_pieces], a side of more than S2T_CHRF_MAX_CHARS characters, or a side with more units than its width
 * (Uh, Ur; the spaces of mode 1 count).
 * Kernel: one launch, one pair per workgroup, no atomics, no host read, no memset; a pair's result does not depend on the batch
 * around it.  The code points are measured, scanned and expanded into LDS by the functions s2t_chrf_stats uses (csrc/text_rows.hpp),
 * the word starts listed, the units written to global memory.  256 threads for max(Hmax, Rmax) <= S2T_CHRF_GROUP_LEN tokens, 1,024
 * above.  LDS: two sides of code points and two start lists, 49.2 KB.
 * Limits: S2T_TEXT_MAX_UNITS units per side (= S2T_EDIT_MAX_B = S2T_CHRF_MAX_CHARS: whatever this call writes, s2t_edit_align
 * takes) and S2T_CHRF_MAX_LEN tokens of padded width.
 * Refusals, before anything is launched: S2T_OK at once for P <= 0; S2T_EINVAL for a NULL required pointer (hyp, hyp_len, ref,
 * ref_len, pieces, piece_off, hyp_units, ref_units, hyp_n, ref_n, status), a negative width, V or n_pieces, an element size other
 * than 4 or 8, a side without a map whose rows are not P (with one: negative), unk >= V, mode outside [0, 2], Uh or Ur outside
 * [0, S2T_TEXT_MAX_UNITS]; S2T_ENOTSUP for a token width above S2T_CHRF_MAX_LEN. */
#define S2T_TEXT_MAX_UNITS 4095
int s2t_text_units(const void* hyp, const void* hyp_len, int hyp_elem, const void* ref, const void* ref_len, int ref_elem,
                   const int* hyp_row, const int* ref_row, int P, int Hmax, int Rmax, int Hrows, int Rrows,
                   const unsigned int* pieces, const int* piece_off, int n_pieces, int V, long long unk, int mode, int Uh, int Ur,
                   int* hyp_units, int* ref_units, int* hyp_n, int* ref_n, int* status, void* stream);
/* ---- Kaldi log-mel filterbanks of waveforms (csrc/fbank.hip): torchaudio.compliance.kaldi.fbank with its defaults, restated.
 * Frames: W samples long, S apart, N the next power of two >= W.  An utterance of n samples has m = 0 frames if n < W, else
 * m = 1 + (n - W) / S (snip-edges); frame t is the samples [t*S, t*S + W).  No sample at or behind n is read into a result.
 * Per frame, in this order:
 *   1. Samples become float: int16 at their integer value, unscaled; float32 as they are.
 *   2. The frame's mean is subtracted (remove_dc).
 *   3. Pre-emphasis with a replicated left edge: y[i] = x[i] - c*x[i-1] for i >= 1, y[0] = x[0] - c*x[0].
 *   4. y is multiplied by `window` (W floats, built by the host: povey, hanning or hamming, symmetric).
 *   5. Zero-padded to N.
 *   6. Real FFT; the power re^2 + im^2 of the bins 0 .. N/2 - 1 (the Nyquist bin has weight 0 in every mel bin).
 *   7. Mel energy e[j] = the sum over i < count_j of weights[offset_j + i] * power[first_j + i]: the bank in sparse form,
 *      bank [F][3] int32 = (first_j, count_j, offset_j), weights [n_weights] float32, made in float64 and rounded once.
 *   8. out[t][j] = log(max(e[j], 2^-23)).
 * Tables: twiddle [N] float64 = cos(2 pi k / N) for k < N/2, then -sin(2 pi k / N) for k < N/2.  The kernel takes a half-size
 * complex FFT of the packed frame (radix-2 Stockham in LDS) and splits it into even and odd parts; it calls no device sin / cos.
 * Steps 2 to 7 run in float64 on the float samples of step 1 (csrc/fbank.hip says why); step 8 is float32.
 * Whatever `bank` holds, a bin's range is cut to the powers and the weights there are.
 * Operands: waves [B] rows of Nmax elements, row_stride elements apart (int16 for wave_elem 2, float32 for 4; no alignment beyond
 * the element's), lengths int64 [B].  out [B][Tmax][F] float32 with Tmax the frames of Nmax samples; out_len [B], status [B] int32.
 * Status: 0 done; 1 no features (0 frames); 2 refused (a length that is negative or above Nmax).  out_len is 0 unless done.  Every
 * row of out at or behind out_len[b] is written as zeros; every row in front of it is written once: out needs no initialisation.
 * One launch, no atomics, no host read.  A workgroup stages the samples of S2T_FBANK_TILE_ELEMS / N consecutive frames in LDS once
 * (S2T_FBANK_FRAME_TILE); a result does not depend on the batch around it or on the tile its frame falls in.
 * Refusals, before anything is launched, in this order: S2T_OK at once for B <= 0; S2T_EINVAL for a NULL pointer (every pointer
 * but stream is required), wave_elem other than 2 or 4, Nmax < 0, row_stride < 0, W < 1, S < 1, F < 1, n_weights < 0, Tmax other
 * than the frames of Nmax, preemph outside [0, 1]; then S2T_ENOTSUP for N other than 256, 512, 1024, W outside (N/2, N],
 * F > S2T_FBANK_MAX_BINS, n_weights > N (a triangular bank has at most two bins over a power), B * tiles >= 2^31. */
#define S2T_FBANK_MAX_BINS 128
#define S2T_FBANK_TILE_ELEMS 8192
#define S2T_FBANK_FRAME_TILE(N) (S2T_FBANK_TILE_ELEMS / (N))
int s2t_fbank(const void* waves, int wave_elem, long long row_stride, const long long* lengths, int B, int Nmax, int W, int S,
              int N, int F, int Tmax, const float* window, const double* twiddle, const int* bank, const float* weights,
              int n_weights, int remove_dc, double preemph, float* out, int* out_len, int* status, void* stream);
/* Per-utterance mean / variance normalisation (examples/speech_recognition/data/data_utils.py:9-25, apply_mv_norm), in place on
 * x [B][Tmax][F] float32 over the first lengths[b] rows (lengths int32 or int64 by len_elem: 4 or 8), per column:
 *   - mean is the column mean, var the unbiased variance;
 *   - inv = 1/(sqrt(var) + 1e-8) for every column of the utterance if any of its columns has var < 1e-8, else 1/sqrt(var);
 *   - x = (x - mean) * inv.
 * The mean is summed over the differences from the utterance's first row and the variance over the differences from that mean,
 * so a constant column has exactly its value as mean, exactly 0 as variance, and normalises to exactly 0.
 * Status [B] int32: 0 done; 1 no features (fewer than 2 rows: one row has no variance, the reference yields NaN); 2 refused (a
 * length that is negative or above Tmax).  out_len [B] int32 is the length if done, else 0; every row at or behind it is written as
 * zeros.  One launch, one workgroup per utterance, no atomics, no host read.
 * Refusals, before anything is launched, in this order: S2T_OK at once for B <= 0; S2T_EINVAL for a NULL pointer (x, lengths,
 * out_len, status), len_elem other than 4 or 8, Tmax < 0, F < 1; then S2T_ENOTSUP for F > S2T_FBANK_MAX_BINS. */
int s2t_cmvn(float* x, const void* lengths, int len_elem, int B, int Tmax, int F, int* out_len, int* status, void* stream);
/* ---- Sinc resampling of waveforms (csrc/resample.hip): Kaldi's LinearResample as torchaudio.compliance.kaldi.resample_waveform
 * restates it, for padded batches; a row picks its resampling from a small table of banks (speed perturbation: one launch).
 * The rule.  A resampling is (orig, new), reduced by its gcd; lowpass_filter_width L = 6, rolloff 0.99 by default.  In float64 on
 * the host: cutoff = rolloff * 0.5 * min(orig, new), ww = L / (2 cutoff), in_unit = orig, out_unit = new; for each phase
 * i < out_unit, t = i / new, first[i] = ceil((t - ww) orig), last[i] = floor((t + ww) orig); tap j = 0 .. last[i] - first[i] has
 * D = (first[i] + j) / orig - t and the weight w[i][j] = [|D| < ww] * 0.5 (1 + cos(2 pi cutoff / L * D)) * s(D) / orig with
 * s(D) = sin(2 pi cutoff D) / (pi D), s(0) = 2 cutoff.  Weights are rounded to float32 once and padded with zeros to `taps`, the
 * widest phase.  Output k of an utterance of n samples, with u = k / out_unit and i = k % out_unit, is
 *   y[k] = the sum over j < taps of w[i][j] * x[first[i] + u * in_unit + j],   x = 0 outside [0, n)
 * (zero, not what lies behind n in the row), summed in float32 from 0 in ascending j with fused multiply-adds.  The utterance
 * yields m = ceil(n * out_unit / in_unit) samples (Kaldi's tick count: every output time is strictly below n / orig).  A bank with
 * in_unit == out_unit copies: y[k] = x[k], int16 at its integer value.
 * The table: `banks` is HOST memory, read during the call only, [n_banks][S2T_RESAMPLE_BANK_INTS] int32 =
 * (in_unit, out_unit, taps, first_off, w_off, lo, extra): first[first_off + i] is first[i]; weights[w_off + j * out_unit + i] is
 * w[i][j] (tap-major); lo = min first[i]; extra = max first[i] - lo + taps.  Of a copying bank only the first two are looked at.
 * `first` (int32 [n_first]) and `weights` (float32 [n_weights]) are device memory.  A first[i] outside [lo, lo + extra - taps] is
 * read as the nearer end: whatever the table holds, no read leaves the staged samples.
 * Operands: waves [B] rows of Nmax elements, row_stride elements apart (int16 for wave_elem 2, float32 for 4; no alignment beyond
 * the element's), lengths [B] int32 or int64 (len_elem 4 or 8), ratio_id [B] int32 or NULL (every row takes bank 0).
 * out [B][Mmax] float32, out_len [B] int64, status [B] int32.  Status: 0 done; 1 no samples (n = 0); 2 refused (a length that is
 * negative or above Nmax, a ratio_id outside [0, n_banks), m > Mmax).  out_len is 0 unless done.  Every element of out at or behind
 * out_len[b] is written as zero, every element in front of it once: out needs no initialisation; nothing else is written.
 * One launch, no atomics, no host read.  A workgroup takes S2T_RESAMPLE_REUSE * G units of a row, G the largest count with
 * G * out_unit <= S2T_RESAMPLE_TILE_ITEMS and (S2T_RESAMPLE_REUSE * G - 1) * in_unit + extra <= S2T_RESAMPLE_MAX_SPAN
 * (G = S2T_RESAMPLE_TILE_ITEMS for a copy); a result does not depend on the batch around it or on the tile it falls in.
 * Refusals, before anything is launched, in this order: S2T_OK at once for B <= 0; S2T_EINVAL for a NULL pointer (all but ratio_id
 * and stream are required), wave_elem other than 2 or 4, len_elem other than 4 or 8, a negative Nmax, Mmax, row_stride, n_first or
 * n_weights, n_banks < 1; S2T_ENOTSUP for n_banks > S2T_RESAMPLE_MAX_BANKS; then bank by bank S2T_EINVAL for in_unit or
 * out_unit < 1, taps < 1, extra < taps, a negative offset, a range of first or weights past n_first or n_weights, |lo| >= 2^30;
 * then S2T_ENOTSUP for a bank with out_unit > S2T_RESAMPLE_MAX_PHASES, taps * out_unit > S2T_RESAMPLE_MAX_BANK or G < 1 (a
 * span of S2T_RESAMPLE_REUSE units that does not fit: (S2T_RESAMPLE_REUSE - 1) * in_unit + extra > S2T_RESAMPLE_MAX_SPAN), and for
 * B * tiles >= 2^31. */
#define S2T_RESAMPLE_MAX_BANKS 8
#define S2T_RESAMPLE_BANK_INTS 7
#define S2T_RESAMPLE_REUSE 4
#define S2T_RESAMPLE_TILE_ITEMS 512
#define S2T_RESAMPLE_MAX_PHASES 512
#define S2T_RESAMPLE_MAX_BANK 8192
#define S2T_RESAMPLE_MAX_SPAN 7672
int s2t_resample(const void* waves, int wave_elem, long long row_stride, const void* lengths, int len_elem, const int* ratio_id,
                 int B, int Nmax, int Mmax, const int* banks, int n_banks, const int* first, int n_first, const float* weights,
                 int n_weights, float* out, long long* out_len, int* status, void* stream);
/* label_smoothed_nll_loss over log_softmax(logits.float()) (label_smoothed_cross_entropy.py:12-29), fused
 * with its gradient: sums2[0] += loss, sums2[1] += nll (caller zeroes); dlogits may be NULL. */
int s2t_lsce(int dtype, const void* logits, const long long* target, void* dlogits, float* sums2,
             long rows, int V, int ld, float eps, int pad, float grad_scale, void* stream);

/* word-level knowledge distillation from stored teacher top-K logits (fairseq/criterions/knowledge_distillation.py:44-96):
 * sum1[0] += sum_rows (1-lambda)*NLL + lambda*KD(tau); teacher_idx [rows][Kt] int64, teacher_logits [rows][Kt] f32, Kt <= 64 */
int s2t_kd_loss(int dtype, const void* logits, const long long* target, const long long* teacher_idx,
                const float* teacher_logits, void* dlogits, float* sum1, long rows, int V, int ld, int Kt,
                float lambda, float tau, int pad, float grad_scale, void* stream);

/* ---- decoder embedding (fairseq/models/transformer.py:720-737) -------------------------------------- */
int s2t_embed_fwd(int dtype, const long long* tokens, const void* W, const float* table, void* out,
                  int B, int L, int D, float scale, int pad, int pos_offset, void* stream);
/* f32 log-probabilities of one decoding step (fairseq/sequence_generator.py:711-768) */
int s2t_log_softmax(int dtype, const void* logits, float* out, long rows, int V, int ld, float inv_temperature, void* stream);
/* The model's get_normalized_probs for criteria that work on (log-)probabilities themselves (fairseq/models/fairseq_decoder.py:58-79,
 * fairseq/models/fairseq_model.py:46-74: utils.log_softmax / utils.softmax of logits.float(); the three criteria of the S2T recipes use
 * the fused loss kernels instead).  s2t_softmax_probs: out = softmax(logits * inv_temperature) in f32.  s2t_softmax_bwd: the gradient of
 * either form w.r.t. the logits, from the saved OUTPUT `out` and its gradient `dout` (both f32 [rows][V], dense):
 *   log_probs = 1:  dlogits = it * (dout - exp(out) * sum_v dout)        log_probs = 0:  dlogits = it * out * (dout - sum_v dout * out)
 * written in `dtype` with row stride ld. */
int s2t_softmax_probs(int dtype, const void* logits, float* out, long rows, int V, int ld, float inv_temperature, void* stream);
int s2t_softmax_bwd(int dtype, const float* out, const float* dout, void* dlogits, long rows, int V, int ld, float inv_temperature,
                    int log_probs, void* stream);
/* ensemble of n <= 8 models (fairseq/sequence_generator.py:757-768 EnsembleModel.forward_decoder): out = logsumexp_j lprobs[j] - log n,
 * element-wise over numel f32 values; `lprobs` is a HOST array of n device pointers */
int s2t_ensemble_lse(int n, const float* const* lprobs, float* out, size_t numel, void* stream);
/* log-probability of the target token at every position of a teacher-forced forward (fairseq/sequence_scorer.py:42-92), for one
 * model or the log of the mean probability of n <= 8 (`logits` and `ld` are HOST arrays of n device pointers / row strides, as
 * s2t_ensemble_lse takes its members).  logits[j]: rows in the engine's time-major order, row r = t*B + b, V columns of `dtype`, row
 * stride ld[j] >= V elements; target (int64) and out (f32): batch-major [B][L].  All arithmetic in f32, per member j and row r with
 * x = logits[j][r][0..V) and c = target[b][t]:
 *     m_j = max_v x_v;  s_j = sum_v exp(x_v - m_j);  lp_j = x_c - (m_j + log s_j)
 *     n == 1: out[b][t] = lp_0;   n > 1: M = max_j lp_j; -inf if M is, else M + log(sum_j exp(lp_j - M)) - log n (members in order:
 *     the combine of s2t_ensemble_lse);   c < 0 or c >= V: NaN, and nothing outside the row is read.
 * No column is special (the pad index is a column like any other); columns [V, ld) never reach a result.  Every logit is read once
 * (running max / sum), in 16-byte loads when every member's base and row stride are multiples of 16 bytes; no [rows, V]
 * intermediate exists and V is limited by int only.  Deterministic: no atomics, a reduction tree fixed by column, identical in both
 * launch forms (a workgroup per row below 4,096 rows, a wave per row from there), so a row's result does not depend on B, L or the grid.
 * S2T_OK at once for B*L == 0; S2T_EINVAL for n < 1, n > 8, a NULL array / member / target / out, V < 1, any ld[j] < V, negative B or
 * L, B*L > 2^31 - 1; S2T_ENOTSUP for a dtype other than bf16 / f32 -- all before anything is launched. */
int s2t_score_targets(int dtype, int n, const void* const* logits, const int* ld, const long long* target, float* out,
                      int B, int L, int V, void* stream);
int s2t_embed_bwd(int dtype, const long long* tokens, const void* dout, float* dW, int B, int L, int D,
                  float scale, int pad, void* stream);
/* out = dropout(dy) * act'(y): act 1 = relu (y = post-activation), act 2 = gelu (y = pre-activation); the dropout (p_drop > 0, mask
 * of s2t_dropout on the flat index) is the backward of one that followed the activation in the forward pass */
int s2t_act_bwd(int dtype, const void* dy, const void* y, void* out, size_t n, int act, float p_drop, unsigned long long seed,
                void* stream);
/* y += x (merging the gradients of two consumers of one activation) */
int s2t_add_inplace(int dtype, const void* x, void* y, size_t n, void* stream);
/* y = x * keep/(1-p) (one rounding to the type; a dropped element is +0), keep a stateless hash of (seed, element index); the backward
 * pass calls it again on the gradient.  The rule every kernel's mask follows (tests/dropout_ref.py restates it; the tests hold to that):
 *   seed key    ks = mix32(lo32(seed) * 0x9E3779B9 + 0x7F4A7C15),  mix32(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16
 *   quad hash   q = index >> 2;  a = lo32(q) ^ ks;  a = bitrev(a + (a mod 2^24) * C) for C = 0x3C6EF2, 0x9E3778, then a += (a mod 2^24) * 0x85EBCA;
 *               a ^= a >> 16;  x = a ^ hwm;  y = bitrev(x + ((x ^ 0x68E31DA4) mod 2^24) * 0xC2B2AE)   (all in 32 bits)
 *   field order element 4q + f draws 16 bits: f0 = y.lo, f1 = y.hi, f2 = x.lo, f3 = x.hi
 *   threshold   kept <=> field >= th16,  th16 = (uint32)min(p * 2^32, 2^32 - 1 as f32) >> 16, in f32: the rate is quantised to 1/65536
 * Index bits >= 34 and seed bits >= 32 enter through one xor only: hw = hi32(q) + hi32(seed), hwm = hw ^ hw << 13 ^ hw >> 7 ^ hw << 27.  Masks
 * that differ only there are correlated (seeds 5 and 2^32 + 5 agree on 79 % of the elements at p = 0.25 where independent masks agree on
 * 62.5 %).  The package issues seeds below 2^32. */
int s2t_dropout(int dtype, const void* x, void* y, size_t n, float p, unsigned long long seed, void* stream);

/* ---- ConvAttention2D blocks of the front end (examples/speech_recognition/modules/conv_attention_2d.py:46-135,
 * conv_transformer.py:216-222).  Channels-last tensors over pixel rows r = (t*B + b)*F + f:
 * x [M][C], qkv [M][16] (q 0-3 | k 4-7 | v 8-11 | 4 zero channels), cat [M][8] (time 0-3 | frequency 4-7).
 * The two 3x3 convolutions are s2t_gemm_gather calls on the packed weights of s2t_a2d_pack_w. ------------------------- */
/* channel moments (mode 0: sum z', z'^2 with z' = prescale[c]*z; mode 1: sum dyn, dyn*xhat with dyn = dy*[BN(z') > 0]),
 * accumulated (double) in groups of Cg channels laid out [Cg | Cg] so that each group feeds s2t_bn_finalize */
int s2t_a2d_chan_stats(int dtype, const void* z, const void* dy, const float* prescale, const float* mean, const float* rstd,
                       const float* scale, const float* shift, double* sums, long M, int C, int ld_z, int ld_dy, int Cg,
                       int mode, void* stream);
/* y = relu(prescale*z*scale + shift) [+ res]   (nn.BatchNorm2d then ReLU, conv_attention_2d.py:92-94,121) */
int s2t_a2d_bn_act(int dtype, const void* z, const float* prescale, const float* scale, const float* shift, const void* res,
                   void* y, long M, int C, int ld_z, int ld_y, void* stream);
/* gradient w.r.t. z of the above given the mode-1 sums (training: batch statistics; eval: running statistics) */
int s2t_a2d_bn_bwd(int dtype, const void* dy, const void* z, const float* prescale, const float* mean, const float* rstd,
                   const float* scale, const float* shift, const double* sums, void* dz, long M, int C, int ld_dy, int ld_z,
                   int Cg, double count, int training, void* stream);
/* dbeta += sums[0..Cg), dgamma += sums[Cg..2Cg) of one group of mode-1 sums */
int s2t_a2d_param_grads(const double* sums, float* dgamma, float* dbeta, int Cg, void* stream);
/* nn.Conv2d weights [Co][Ci][3][3] (f32) <-> gathered-GEMM operands, row stride ld, CP = padded channels per tap:
 * mode 0: dst[co][j*CP+ci] = W[co][ci][j];  mode 1: dst[ci][j*CP+co] = W[co][ci][8-j];  mode 2: grad[co][ci][j] += src[co][j*CP+ci] */
int s2t_a2d_pack_w(int dst_dtype, const float* src, void* dst, float* grad, int Co, int Ci, int CP, int ld, int mode, void* stream);
/* weight gradient of a 3x3 / pad 1 convolution over the pixel rows, all nine taps in one pass, added to the master layout
 * dW [CO][CI][3][3] (f32): (CO <= 16 with ld_dy >= 16, CI = 64) or (CO = 64, CI = 8); other shapes: S2T_ENOTSUP (callers fall
 * back to nine gathered s2t_gemm_gather products).  ws: S2T_A2D_WGRAD_GROUPS x max(CO,16) x CI x 9 floats of workspace
 * (per-workgroup partial sums, reduced by a second kernel: 16 instead of 512 atomics per weight) */
#define S2T_A2D_WGRAD_GROUPS 512
int s2t_a2d_conv_wgrad(int dtype, const void* dY, int ld_dy, const void* X, int ld_x, float* dW, float* ws, int CO, int CI,
                       int B, int T, int F, void* stream);
/* channels-last pixel rows [M][ld] <-> head-major planes [G][T][B][4*32] (plane of head h of group g = channel ch0 + 4g + h,
 * columns 32h .. 32h+F-1, zero padded): dir 0 gathers the planes, dir 1 scatters them back.  The time attention of a block then
 * runs on s2t_attn_fwd / s2t_attn_bwd at head_dim 32 */
int s2t_a2d_planes(int dtype, void* chl, void* planes, int G, int ch0, int ld, int B, int T, int F, int dir, void* stream);
/* time attention of every (batch, head) plane: cat[.., h] = dropout(softmax_t'(q k^T)) v ; lse [B*4][T] for the backward */
int s2t_a2d_time_fwd(int dtype, const void* qkv, void* cat, float* lse, int B, int T, int F, float p_drop,
                     unsigned long long seed, void* stream);
/* writes dq, dk, dv of the time attention into dqkv (delta [B*4][T] is workspace) */
int s2t_a2d_time_bwd(int dtype, const void* qkv, const void* cat, const void* dcat, const float* lse, float* delta, void* dqkv,
                     int B, int T, int F, float p_drop, unsigned long long seed, void* stream);
/* frequency attention: cat[.., 4+h] = (dropout(softmax_f'(q^T k)) v^T)^T ; A [B*4][F][F] = the probabilities before dropout */
int s2t_a2d_freq_fwd(int dtype, const void* qkv, void* cat, float* A, int B, int T, int F, float p_drop,
                     unsigned long long seed, void* stream);
/* ADDS dq, dk, dv of the frequency attention to dqkv */
int s2t_a2d_freq_bwd(int dtype, const void* qkv, const void* dcat, const float* A, void* dqkv, int B, int T, int F,
                     float p_drop, unsigned long long seed, void* stream);

/* ---- optimizer (fairseq/trainer.py:416-443, fairseq/utils.py:253-277, fairseq/optim/adam.py:147-202) ----
 * out2[0] = gnorm = scale*||g||_2 ; out2[1] = scale * min(1, max_norm/(gnorm+1e-6)) (all on device) */
int s2t_grad_norm_clip(const float* g, size_t n, double* acc_ws, float scale, float max_norm, float* out2, void* stream);
/* the same with scale / max(*divisor_dev, 1) in place of scale: divisor_dev = the sample size summed over the data-parallel ranks, still
 * on the device after its all-reduce (fairseq/trainer.py:416-430 reads it on the host; here no host synchronisation precedes Adam) */
int s2t_grad_norm_clip_div(const float* g, size_t n, double* acc_ws, float scale, const double* divisor_dev, float max_norm,
                           float* out2, void* stream);
/* Adam over a flat arena; gradients are multiplied by mult2[1] (NULL = 1); optional bf16 shadow refresh */
int s2t_adam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, size_t n, const float* mult2,
                  float lr, float beta1, float beta2, float eps, float wd, int step, void* stream);
int s2t_cast(int src_dtype, int dst_dtype, const void* src, void* dst, size_t n, void* stream);
int s2t_scale_by_device_scalar(int dtype, void* x, size_t n, const float* scalar, void* stream);

/* ---- incremental decoding + beam search as ONE stream-ordered sequence of launches per step ----------------------------------------
 * Replaces, per decoding step, fairseq/sequence_generator.py:243-447 (the loop body of SequenceGenerator._generate: forward_decoder,
 * log-softmax, the pad / unk / min-len / max-len rules, BeamSearch.step = fairseq/search.py:55-83, EOS finalisation bookkeeping :502-600,
 * next-beam selection :417-446, reorder_incremental_state :430-447 / fairseq/modules/multihead_attention.py:246-283,407-420) and the
 * incremental TransformerDecoder forward (fairseq/models/transformer.py:674-782, transformer_layer.py:243-377).
 *
 * N = B * beam hypothesis slots, slot n = s * beam + j of sentence s.  One step is 3 * layers + 4 launches:
 *   per layer  S: LayerNorm -> q|k|v of one head (k, v written to the cache row of this step) -> attention over the cached rows of the
 *                 hypothesis' ancestors -> this head's share of the output projection           grid (B, heads)
 *              C: LayerNorm -> q of one head -> attention over the sentence's encoder rows -> share of the output projection
 *              F: LayerNorm -> one slice of fc1 + activation -> that slice's share of fc2        grid (B, ffn_slices)
 *   then       final LayerNorm; output projection over all N rows; per row: log-softmax, score rules, + cumulative score, 2*beam best;
 *              per sentence: merge (diverse_groups > 1: the groups' penalised selections instead), finalise EOS candidates, choose the
 *              next beam, record it, embed its tokens for the next step.
 * The shares (per head / per slice, in the compute type T) are summed in f32, in a fixed order, by the launch that consumes them, together with the residual and the
 * bias: no atomics, results do not depend on scheduling.  The K/V cache is never re-ordered: anc[n][p] names the slot whose row at
 * position p belongs to hypothesis n's history (the index indirection that replaces reorder_incremental_state's index_select copies),
 * the encoder-side K/V exist once per sentence.  The step index lives in device memory (steps[s]), so one recorded sequence (a hipGraph
 * captured around s2t_decode_step) serves every step.  Nothing synchronises; the host polls `finished` when it chooses to.
 * Limits (S2T_ENOTSUP otherwise): head size 64, D = 256, 512 or 1024, beam <= 16, B * beam <= 128, ffn / ffn_slices = 64, 128 or 256,
 * max_len + 1 <= 1024 positions, Tsp a multiple of 128, and the LDS plan of every launch within 152 KiB (s2t_decode_lds_bytes).
 * The *_rules calls add, in the per-row launch and in the reference's order after the rules above, prefix tokens
 * (sequence_generator.py:270-280,449-476) and n-gram blocking (:596-650); their limits: n-gram size 0 (off) or >= 2 -- with 1 the reference
 * bans EOS through the <bos> column and the search never finalises (S2T_ENOTSUP); a prefix without EOS -- the reference then copies slot 0
 * over the sentence's other slots, which this path does not do (the CALLER checks: the tokens are device memory).
 * The *_ensemble calls run the search over 2..8 models at once (fairseq/sequence_generator.py:757-768 EnsembleModel.forward_decoder): one
 * descriptor per member, all of them naming ONE search state.  A step is every member's 3 * layers_j + 2 launches up to its logits, one
 * member after the other, then one row launch that takes the log of the members' mean probability (each member's log-softmax as above,
 * combined per column as s2t_ensemble_lse does: m = max_j lp_j; -inf if m is; else m + log(sum_j exp(lp_j - m)) - log n) before the
 * rules, and one sentence launch that also embeds the chosen tokens for every member: sum_j (3 * layers_j + 2) + 2 launches. */
typedef struct S2TDecodeLayer {
    const void *ln1_g, *ln1_b;       /* f32 [D]: self_attn_layer_norm */
    /* every w_* below is the nn.Linear weight in FRAGMENT-MAJOR order (s2t_decode_pack_weight): [rows / 16][K / ks][64 lanes][16 bytes] */
    const void *w_qkv, *b_qkv;       /* T [3D][D] packed, f32 [3D] */
    const void *w_o, *b_o;           /* T [D][D] packed, f32 [D] */
    const void *lnx_g, *lnx_b;       /* encoder_attn_layer_norm */
    const void *w_xq, *b_xq, *w_xo, *b_xo;
    const void *ln2_g, *ln2_b;       /* final_layer_norm */
    const void *w_fc1, *b_fc1;       /* T [ffn][D] packed, f32 [ffn] */
    const void *w_fc2, *b_fc2;       /* T [D][ffn] packed, f32 [D] */
    const void* kv_enc;              /* T [B][heads][Tsp / 16][64 / ks][64][16 B]: this layer's encoder-side keys (static_kv), fragment-major, one
                                      * copy per SENTENCE, zero beyond Ts (s2t_decode_prepare_enc); Tsp % 128 == 0 */
    const void* vt_enc;              /* T [B][heads][4][Tsp / ks][64][16 B]: the values, transposed and fragment-major (same call) */
    void* kv_cache;                  /* T [max_len + 1][N][2D]: k | v rows written by step t at position t */
} S2TDecodeLayer;

typedef struct S2TDecodeDesc {
    int dtype, B, beam, D, heads, ffn, layers, V, ldv, Ts, Tsp, max_len, min_len, ffn_slices, gelu;
    int pad, unk, eos, step0_all_slots;      /* step0_all_slots: HierarchicalBeamSearch (twophase_sequence_generator.py:22-49) */
    float ln_eps, embed_scale, unk_penalty, inv_temperature;
    const S2TDecodeLayer* layer;             /* HOST array [layers] */
    const void *lnf_g, *lnf_b;               /* decoder.layer_norm */
    const void* w_out;                       /* T [V][D] output projection (the embedding when shared), packed like the layers' weights */
    const void* embed;                       /* T [V][D] */
    const float* pos_table;                  /* f32 [>= pad + 2 + max_len][D] sinusoidal table, row `pad` zero */
    const int* enc_klen;                     /* i32 [B] valid encoder rows per sentence, or NULL (no padding) */
    const float* init_scores;                /* f32 [N] starting score of every slot (step0_all_slots), or NULL */
    /* state, all device memory owned by the caller */
    float *x0, *x1;                          /* f32 [N][D] residual stream (ping-pong) */
    void *part0, *part1;                     /* T [max(heads, ffn_slices)][N][D] shares (ping-pong) */
    void* xn;                                /* T [N][D] final LayerNorm output */
    float* logits;                           /* f32 [N][ldv] */
    int* steps;                              /* i32 [B] */
    int* anc;                                /* i32 [N][max_len + 1] */
    float* cand_val; int* cand_idx;          /* [N][2 * beam] per-row candidates */
    int* tok_hist; int* par_hist; float* cum_hist;   /* [max_len + 2][N]: arrangement i = the beam after i selections */
    int* blacklist;                          /* i32 [N] */
    int* nfin; int* finished;                /* i32 [B] */
    int* fin_step; int* fin_row; float* fin_score;   /* [B][beam]: finalised hypotheses in the order the reference appends them */
    /* group-diverse beam search (fairseq/search.py:103-161), appended behind the fields above: a zero-initialised descriptor is the plain
     * search.  diverse_groups G: 0 or 1 = plain (exactly the launches of before); G > 1: the beam is G groups of beam / G slots, group g
     * the slots g, g + G, ...; the groups choose in order, each from its rows' candidates lowered by diverse_strength x (the number of
     * candidates the earlier groups of this step took with that token), and candidate j of group g is overall candidate j G + g.  A form
     * of the per-sentence launch: the number of launches does not change.  Checked by every s2t_decode_* call that takes a descriptor,
     * first of the descriptor's checks (after d == NULL and the rules) and before any launch, in this order: diverse_groups < 0 ->
     * S2T_EINVAL; G > 1 and beam % G != 0 -> S2T_EINVAL (the reference raises ValueError); G > 1 and diverse_strength negative or not
     * finite -> S2T_ENOTSUP (a reward breaks the argument that a row's 2 * beam best are enough); G > 1 with step0_all_slots ->
     * S2T_ENOTSUP.  diverse_strength is not looked at while G <= 1. */
    int diverse_groups; float diverse_strength;
} S2TDecodeDesc;

/* Fragment-major copies for the MFMA B operand: lane l of fragment (tile, step) holds rows 16 tile + (l & 15), columns ks step + per (l >> 4) ..
 * (ks = 32, per = 8 for bf16; 16, 4 for f32), so a wave loads a fragment as one contiguous KiB.
 * s2t_decode_pack_weight: W [N][K] (row stride ldw elements, K % ks == 0) -> Wp [ceil(N / 16)][K / ks][64][per], rows past N zero.
 * s2t_decode_prepare_enc: kv [Ts][B][2D] (K | V rows of the encoder output under one layer's encoder_attn.kv) -> the layer's kv_enc and
 * vt_enc as S2TDecodeLayer describes them. */
int s2t_decode_pack_weight(int dtype, const void* W, int ldw, int N, int K, void* Wp, void* stream);
int s2t_decode_prepare_enc(int dtype, const void* kv, void* kv_enc, void* vt_enc, int Ts, int Tsp, int B, int D, int heads, void* stream);
/* resets the state for a new search: steps, blacklist, nfin, finished = 0; arrangement 0 = `bos` in every slot; x0 = its embedding */
int s2t_decode_begin(const S2TDecodeDesc* d, int bos, void* stream);
/* the launches of one step (see above).  `d` and d->layer are HOST memory read during the call only. */
int s2t_decode_step(const S2TDecodeDesc* d, void* stream);
/* Score rules beyond S2TDecodeDesc's, for the calls below.  prefix: DEVICE i32 [B][prefix_len], the forced token of sentence s at step t
 * or `pad` for none; it must stay where it is while a graph recorded with it is replayed.  At a step t < min(prefix_len, max_len) a row of
 * a sentence with a forced token keeps that column only (its log-probability after the unk penalty), and the min_len rule is skipped for
 * EVERY sentence (the reference's `elif`).  no_repeat_ngram = n >= 2: a hypothesis may not produce a token that completes an n-gram it
 * already contains; applied after the prefix rule (a ban may leave a forced row without any candidate). */
typedef struct S2TDecodeRules { int no_repeat_ngram, prefix_len; const int* prefix; } S2TDecodeRules;
/* s2t_decode_step with rules.  r == NULL, or no_repeat_ngram == 0 and prefix_len == 0: exactly s2t_decode_step (which is this call with
 * NULL).  Checked before any launch: d == NULL, no_repeat_ngram < 0, prefix_len < 0, prefix_len > 0 with prefix == NULL -> S2T_EINVAL;
 * no_repeat_ngram == 1 -> S2T_ENOTSUP; then `d` as s2t_decode_step checks it.  `r` is HOST memory read during the call only. */
int s2t_decode_step_rules(const S2TDecodeDesc* d, const S2TDecodeRules* r, void* stream);
/* dynamic LDS bytes the S / C / F launches of `d` need (0 when `d` is outside the limits): the caller may compare with 160 KiB */
size_t s2t_decode_lds_bytes(const S2TDecodeDesc* d);
/* n_steps (1..64) consecutive steps recorded as ONE hipGraph: `create` captures n_steps x s2t_decode_step(d) on a private stream (nothing
 * executes) and instantiates it, `launch` replays it on `stream` (the kernels read the step index from d->steps, so the same recording
 * serves every step, and every kernel returns at once for a sentence whose step index has passed max_len: replaying past the end is
 * harmless; `d`'s device buffers must stay where they are), `destroy` frees it after the caller has synchronised with the last replay.
 * *graph_exec is HOST. */
int s2t_decode_graph_create(const S2TDecodeDesc* d, int n_steps, void** graph_exec);
/* the same recording of n_steps x s2t_decode_step_rules(d, r); arguments checked as there (and graph_exec, n_steps first: S2T_EINVAL) */
int s2t_decode_graph_create_rules(const S2TDecodeDesc* d, const S2TDecodeRules* r, int n_steps, void** graph_exec);
/* The same three calls for an ensemble.  d: a HOST array of n HOST descriptors (and their HOST layer arrays), read during the call only.
 * Members may differ in D, heads, layers, ffn, ffn_slices, Ts, Tsp, enc_klen, embed_scale, ln_eps, gelu and in every weight and buffer
 * of their own (x0, x1, part0, part1, xn, logits, the layers' caches); they must agree on dtype, B, beam, V, ldv, max_len, min_len, pad,
 * unk, eos, step0_all_slots, unk_penalty, inv_temperature, diverse_groups, diverse_strength and on every state pointer (steps, anc, tok_hist, par_hist, cum_hist, blacklist,
 * nfin, finished, fin_step, fin_row, fin_score, cand_val, cand_idx, init_scores).  Checked before any launch, in this order: d == NULL,
 * n < 1, n > 8 or a NULL d[j] -> S2T_EINVAL; `r` as s2t_decode_step_rules checks it (begin: no rules); members that disagree on a shared
 * field -> S2T_EINVAL; every member as s2t_decode_step checks it (S2T_ENOTSUP outside the limits).  graph_create checks graph_exec and
 * n_steps (1..64) first (S2T_EINVAL) and leaves *graph_exec NULL on every failure.  n == 1 launches exactly what the *_rules calls launch
 * for d[0].  Every recording is one chain on one stream (the members do not overlap); s2t_decode_graph_launch / _destroy serve it. */
int s2t_decode_begin_ensemble(const S2TDecodeDesc* const* d, int n, int bos, void* stream);
int s2t_decode_step_ensemble(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, void* stream);
int s2t_decode_graph_create_ensemble(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, int n_steps, void** graph_exec);
int s2t_decode_graph_launch(void* graph_exec, void* stream);
int s2t_decode_graph_destroy(void* graph_exec);
/* ---- sampling search (fairseq/search.py:164-278 Sampling: unrestricted, top-k, nucleus) --------------------------------------------
 * torch.multinomial's stream cannot be reproduced, so the draw is a stateless function, the same in every call below (csrc/sample.hpp):
 *   uniform   h = hash32(key, step t, slot n, column v) -- 32-bit integer arithmetic only --, u = ((h >> 9) + 0.5) * 2^-23: exact in f32,
 *             never 0 or 1;
 *   kept set  of a row of log-probabilities lp (after all score rules, NOT renormalised), in the order value descending, column
 *             ascending: topp > 0 (takes precedence): a column is kept iff the mass expf(lp) strictly before it is < topp (topp >= the
 *             total mass keeps every finite column); else topk > 0: the first topk columns (topk >= the number of finite columns keeps
 *             them all); else every finite column.  -inf columns are never kept;
 *   token     the arg-max over the kept columns of lp + g, g = -logf(-logf(u)) (Gumbel-max; value descending, column ascending on ties);
 *             its score is lp[token] itself -- the reference returns log(exp(lp)), at most 1 ulp away.  A row without a finite column
 *             gives token 0 with score -inf (the reference raises there).
 * s2t_sample_rows: lprobs f32 [rows][V] with row stride ld; row r, draw j < draws is slot n = r * draws + j: tok / lp_out [rows * draws],
 * n_kept[r] the size of row r's kept set.  Checked before any launch: a NULL pointer, rows < 1, draws < 1, topk < 0, topp NaN, V < 1,
 * ld < V, step < 0 -> S2T_EINVAL; V > 32768 -> S2T_ENOTSUP. */
int s2t_sample_rows(const float* lprobs, long rows, int V, int ld, int draws, int topk, float topp, unsigned long long key, int step,
                    int* tok, float* lp_out, int* n_kept, void* stream);
/* The device-resident search with that draw instead of the merge: a form of the per-row launch (built on the rules form: prefix tokens and
 * n-gram blocking apply before the draw; an ensemble draws from the log of the members' mean probability) and of the per-sentence launch;
 * the number of launches does not change.  Slot n = s * beam + j draws its own token at every step, from its own row -- at step 0 from the
 * sentence's FIRST row (every member's), with parent slot 0 -- and candidate r of a sentence is slot r's draw: exactly `beam` candidates,
 * score = lp[token] + the slot's cumulative score, which enters neither the keys nor the kept set.  EOS finalisation, black-listing, the
 * records and the next input are those of the beam search run with `beam` candidates.  The step index of the hash is steps[s]: one
 * recorded graph serves every step.  topk 0 = off, topp <= 0 = off.  n = 1..8 members; begin, launch and destroy are the calls above.
 * Checked before any launch, in this order: s == NULL, topk < 0 or topp NaN -> S2T_EINVAL; everything s2t_decode_step_ensemble checks, in
 * its order; diverse_groups > 1 or step0_all_slots -> S2T_ENOTSUP.  graph_create checks graph_exec and n_steps first, as above. */
typedef struct S2TDecodeSample { int topk; float topp; unsigned long long key; } S2TDecodeSample;
int s2t_decode_step_sample(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, const S2TDecodeSample* s, void* stream);
int s2t_decode_graph_create_sample(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, const S2TDecodeSample* s, int n_steps,
                                   void** graph_exec);

/* ---- two options of the device-resident search that S2TDecodeDesc (whose size is pinned) has no room for ----------------------------
 * S2TDecodeExtras is HOST memory read during the call only; the pointers in it are DEVICE memory that must stay where it is while a
 * graph recorded with it is replayed.
 *   lne_g[j], lne_b[j]  f32 [D_j]: member j's decoder.layernorm_embedding (--layernorm-embedding, fairseq/models/transformer.py:731-732),
 *                       or both NULL for a member without one.  Every row of a decoder input, embed_scale * embed[token] + position, is
 *                       normalised over D in f32 (biased variance, the member's ln_eps inside the root) before it is stored to x0: the
 *                       <bos> rows by begin, the next step's rows by the per-sentence launch (a wave per row).
 *   attn_part           f32 [heads][N][Tsp]: scratch for the per-head probabilities (one model only).
 *   attn_hist           f32 [max_len + 1][N][Ts]: record t, slot n = the encoder-attention probabilities of the LAST decoder layer,
 *                       averaged over the heads (fixed order, x 1 / heads), of the hypothesis that occupied slot n when step t ran, i.e.
 *                       BEFORE that step's selection (fairseq/sequence_generator.py:286-292 with alignment_layer's default); keys at or
 *                       beyond enc_klen[s] are exactly 0.  A sentence past its last step writes nothing.  Both NULL: nothing is recorded.
 * The last layer's C launch also stores its f32 probabilities to attn_part, and the final LayerNorm launch (per sentence) sums the heads
 * into attn_hist before the per-sentence launch advances steps[s]: the number of launches does not change, and every other launch is the
 * one the calls below make without `x`.
 * The three calls generalise begin / step / graph_create of every form above: n = 1..8 members, r the rules or NULL, s the sampling search
 * or NULL.  x == NULL, or every field of it NULL: exactly the launches of s2t_decode_begin_ensemble / s2t_decode_step_ensemble (s == NULL)
 * or s2t_decode_step_sample (s != NULL) and their graph_create (n == 1: those of the one-model calls).  Checked before any launch, in
 * this order (graph_create: graph_exec and n_steps first, S2T_EINVAL, *graph_exec left NULL on every failure): with x != NULL, one of
 * attn_part / attn_hist without the other, or one of lne_g[j] / lne_b[j] without the other for any j < 8 -> S2T_EINVAL; attn_part with
 * n > 1 -> S2T_ENOTSUP (an ensemble's attention stays with the caller); then, s != NULL: everything s2t_decode_step_sample checks, in its
 * order; s == NULL: everything s2t_decode_step_ensemble checks, in its order; begin_ex then bos as s2t_decode_begin.  Entries lne_g[j],
 * j >= n, are not looked at beyond the pairing check. */
typedef struct S2TDecodeExtras { const float* lne_g[8]; const float* lne_b[8]; float* attn_part; float* attn_hist; } S2TDecodeExtras;
int s2t_decode_begin_ex(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, const S2TDecodeSample* s, const S2TDecodeExtras* x,
                        int bos, void* stream);
int s2t_decode_step_ex(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, const S2TDecodeSample* s, const S2TDecodeExtras* x,
                       void* stream);
int s2t_decode_graph_create_ex(const S2TDecodeDesc* const* d, int n, const S2TDecodeRules* r, const S2TDecodeSample* s,
                               const S2TDecodeExtras* x, int n_steps, void** graph_exec);

/* ---- measurement aid: what a collective costs the kernels beside it, on ONE GPU (bench.py data_parallel.dry_run) --------------------
 * `workgroups` workgroups stay resident on `stream` for the time a ring all-reduce of `bytes` over `ranks` ranks takes at `bus_gbps`
 * (2 (ranks - 1) / ranks * bytes / bus) and copy src -> dst twice meanwhile, evenly paced.  Stands in for RCCL's kernels of
 * fairseq/legacy_distributed_data_parallel.py:96-170's all-reduce as a competitor for CUs and HBM; moves nothing between GPUs. */
int s2t_comm_standin(const void* src, void* dst, size_t bytes, int workgroups, int ranks, float bus_gbps, void* stream);

/* ---- in-library timing of kernel families with HIP events (bench.py roofline) ------------------------
 * While enabled, every launch of the named family on `stream` is bracketed by hipEvents; s2t_prof_read
 * synchronises those events and returns accumulated milliseconds, launches and algorithmic flops/bytes. */
int s2t_prof_enable(int on);
/* ---- kernel-route options (tests cover every route; nothing here changes results beyond rounding) --------------------
 * key = "gemm256": 1 (default) sends the big bf16 NT / NN products to the 256x256x64 LDS-DMA kernel, 0 keeps them on the
 *                  128x128 register-staged kernels;
 *       "attn_v1": 1 forces the first-generation attention kernels (f32 / d 32 / short sequences use them anyway), default 0;
 *       "attn_v2_min_tq": shortest query block taken by the second-generation attention kernels (default 16);
 *       "gemm256_min_tiles": fewest 192 / 256-row output tiles a product must have for the 256-wide kernel (0 = default = 160;
 *                  tools/gemm_gate_probe.py measures both sides of it);
 *       "reserve_cus": 0..128 (default 0): the persistent one-workgroup-per-CU kernels (gemm256, wgrad_group) launch 256 - value
 *                  workgroups and plan their rounds for that many CUs -- what a data-parallel run sets while RCCL's kernels share
 *                  the chip with backward (trainer: --reserve-cus);
 *       "gemm_f32_small_nt" / "gemm_f32_small_kt" (defaults 1024 / 512): f32 products with fewer 128 x 128 tiles than this take the 64 x 64
 *                  form (NT / NN and TN layouts): the exact-f32 MFMA is 1/16 of the bf16 rate, so what counts is that every CU has
 *                  tiles (tools/f32_tile_sweep.py: 22.96 -> 20.03 ms per update of configs[1]); "gemm_f32_narrow" (default 0): below
 *                  that many the 128 x 64 form;
 *       "gemm_small_nt" / "gemm_small_kt" (defaults 192 / 40): the same thresholds for bf16 products (tools/small_m_sweep.py: at M = 3,000 the
 *                  64 x 64 form loses on every NN product and the whole update moves within its noise: the defaults stay);
 *       "gemm_deep" (default 1): the 64 x 64 four-wave bf16 GEMM form requests 8 (NT) / 4 (NN, TN) k-tiles before its first MFMA instead
 *                  of keeping two in flight; bit-identical results (tools/gemm_deep_check.py); 0 restores the two-set loop;
 *       "ln_small" (default 1): the bf16, D = 512 LayerNorm backward of activations below 8,192 rows requests a wave's rows three at a
 *                  time instead of one ahead (same formulas; results agree with the other kernel to bf16 rounding); 0 restores it;
 *       "decode_stop_after": diagnostic, ends s2t_decode_step after that many launches, counted across the members of an ensemble (0 = off);
 * returns the previous value, or S2T_EINVAL (-22) for an unknown key or a value out of range. */
int s2t_set_option(const char* key, int value);
int s2t_prof_read(const char* family, double* ms, long long* launches, double* flops, double* bytes);
int s2t_prof_reset(void);

/* ---- host-side helpers (HOST pointers) -------------------------------------------------------------
 * greedy CTC decode + edit-distance alignment error count (compute_ctc_uer, CTC_loss.py:31-74;
 * examples/speech_recognition/utils/wer_utils.py:71-203) -- the reference runs this in pure Python
 * on the critical path of every step. */
int s2t_host_ctc_uer(const int* pred, const long long* input_len, int B, int T, const long long* targets,
                     const long long* target_len, int L, int blank, double* errors, double* total);

#ifdef __cplusplus
}
#endif
#endif

/* cwlt.h -- C-ABI of libcwlt.so: the MI355X (gfx950) hot path of the compound-word (CW)
 * Linear-Transformer + AIRL / PPO / DQN training path.
 *
 * Every entry point
 *   - is `extern "C"`, takes plain device pointers + sizes (no torch types),
 *   - enqueues on the hipStream_t passed as `stream` (void*; 0 = default stream) and returns
 *     without synchronising, never allocates, never throws, keeps no global mutable state,
 *   - returns 0 on success, a hipError_t value (1..999) if the launch failed, or
 *     CWLT_ERR_ARG (1001) / CWLT_ERR_DTYPE (1002) for arguments it refuses.
 * Workspaces are allocated by the caller and passed in.
 *
 * File:line citations are relative to the reference checkout (/root/reference).
 * `dtype` arguments: CWLT_F32 = 0, CWLT_BF16 = 1 (storage type of activations; all arithmetic
 * and every running state is f32).
 */
#ifndef CWLT_H
#define CWLT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWLT_OK 0
#define CWLT_ERR_ARG 1001
#define CWLT_ERR_DTYPE 1002
#define CWLT_F32 0
#define CWLT_BF16 1

/* ABI version of this header; bumped on any signature change. */
int cwlt_abi_version(void);

/* ---- causal linear attention -------------------------------------------------------------------
 * Replaces fast_transformers (pytorch-fast-transformers==0.4.0, requirements.txt:54)
 * `CausalLinearAttention.forward` incl. its `causal_dot_product` extension, reached from
 * dqn_policy/model.py:128-137,231-232; dqn_policy/agent_pretrain.py:244-253,345-346;
 * ppo_policy/model.py:129-138,233-234,313-321,371-372 (attention_type="causal-linear").
 *
 * q, k, v, out: (N, L, H, head_dim) with token-row stride ld* elements (head h at column
 * h*head_dim, batch stride L*ld*), RAW projections -- the elu(x)+1 feature map is applied inside.
 * zinv: (N, L, H) f32, 1/(phi(q_l).sum_{j<=l} phi(k_j) + eps), written by fwd, read by bwd.
 * head_dim must be 64 (d_model 512 / 8 heads, dqn_policy/config.py:11-15).
 *
 * Few streams: with N * H far below the 256 CUs one workgroup per (sequence, head) leaves the chip idle (the
 * reference's own pretrain batch is 4 sequences: dqn_policy/agent_pretrain.py:48).  `segments` > 1 cuts every
 * sequence into that many runs of whole 64-token chunks, one workgroup each: a first pass reduces each run to its
 * state increment, a prefix pass turns increments into starting states, the scan proper starts every run from its
 * state.  cwlt_scan_segments() is the library's choice (1 once the streams fill the chip; bf16 with row strides % 8
 * == 0 only); seg_ws: cwlt_scan_seg_floats(N, H, segments, backward) floats, NULL when segments == 1.  The backward
 * calls share ONE workspace: dkdv (first) fills it, dq reads it.  A run owns ceil(chunks / segments) chunks, and every
 * run must own at least one: (segments - 1) * ceil(chunks / segments) < chunks, chunks = ceil(L / 64) -- e.g. 9 chunks
 * take 3 segments, not 4 (3 + 3 + 3 + 0); a count that leaves a run empty is CWLT_ERR_ARG.
 *
 * final_state (optional; bf16, row strides % 8 == 0, segments == 1): cwlt_scan_final_state_floats(N, H) floats that
 * receive, per (sequence, head), the scan's state after the last token -- sum_j phi(k_j) v_j^T transposed (64 x 64 f32)
 * followed by sum_j phi(k_j) (64 f32).  It is what cwlt_causal_linear_bwd_sweep needs to run the whole backward in one
 * pass. */
int cwlt_scan_segments(int N, int H, int L, int dtype);
int64_t cwlt_scan_seg_floats(int N, int H, int segments, int backward);
int64_t cwlt_scan_final_state_floats(int N, int H);
int cwlt_causal_linear_fwd(const void* q, const void* k, const void* v, void* out, float* zinv,
                           int N, int H, int L, int head_dim,
                           int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                           float eps, int segments, float* seg_ws, float* final_state, int dtype, void* stream);

/* The whole backward (dq, dk, dv and, optionally, their per-(sequence, head) column sums: colsum_* (N, H*64) f32, all
 * three or none) in ONE reverse sweep: q, k, v, out, dout are each read once -- 8 streams of HBM traffic against the 12
 * of the dkdv + dq pair below.  The dQ scan needs the state of EARLIER tokens while the sweep runs from the last token
 * to the first: it starts from the forward's final_state and removes each chunk's contribution as it passes (f32
 * accumulators).  bf16 with row strides % 8 == 0 only (CWLT_ERR_DTYPE / CWLT_ERR_ARG otherwise); one 8-wave workgroup
 * per (sequence, head), so meant for launches whose N * H fills the chip -- few-stream launches use the segmented pair.
 * Same reference call sites as above (the backward of causal_dot_product). */
int cwlt_causal_linear_bwd_sweep(const void* q, const void* k, const void* v, const void* out, const float* zinv,
                                 const void* dout, const float* final_state, void* dq, void* dk, void* dv,
                                 float* colsum_q, float* colsum_k, float* colsum_v,
                                 int N, int H, int L, int head_dim,
                                 int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                                 int64_t lddq, int64_t lddk, int64_t lddv, int dtype, void* stream);

/* dq, dk, dv are gradients w.r.t. the RAW q, k, v (feature-map derivative applied inside);
 * out / zinv are the forward's outputs, dout the gradient w.r.t. out (row stride lddo). */
int cwlt_causal_linear_bwd(const void* q, const void* k, const void* v, const void* out,
                           const float* zinv, const void* dout, void* dq, void* dk, void* dv,
                           int N, int H, int L, int head_dim,
                           int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                           int64_t lddq, int64_t lddk, int64_t lddv, int dtype, void* stream);

/* The two kernels of the backward, separately launchable (the call above = dkdv then dq):
 * reverse scan producing dk, dv; forward scan producing dq.  colsum_* (each (N, H*head_dim) f32, may be
 * NULL; bf16 tensors with row strides % 8 == 0 only; (N * segments, H*head_dim) when segments > 1): per-sequence
 * (per-segment) column sums of the written gradient,
 * i.e. the partial bias gradients of the key / value / query projections (summed over N by the caller),
 * which saves a separate pass over dQ|dK|dV.
 * dden (N, L, H) f32, may be NULL: dden_l = -(dout_l . out_l) * zinv_l, the gradient through the normaliser.  Both
 * scans need it; when the caller passes one buffer to both calls (dkdv FIRST), dkdv writes it and dq reads it in place
 * of the whole `out` stream (bf16 fast path; `out` may then be NULL for dq).  The f32 kernels ignore it. */
int cwlt_causal_linear_bwd_dkdv(const void* q, const void* k, const void* v, const void* out,
                                const float* zinv, const void* dout, void* dk, void* dv,
                                float* colsum_k, float* colsum_v, float* dden,
                                int N, int H, int L, int head_dim,
                                int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                                int64_t lddk, int64_t lddv, int segments, float* seg_ws, int dtype, void* stream);
int cwlt_causal_linear_bwd_dq(const void* q, const void* k, const void* v, const void* out,
                              const float* zinv, const void* dout, void* dq, float* colsum_q, const float* dden,
                              int N, int H, int L, int head_dim,
                              int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                              int64_t lddq, int segments, const float* seg_ws, int dtype, void* stream);

/* Packed form of the four calls above: songs of different lengths laid end to end in one (rows, H, head_dim) row buffer.
 * cu: n_songs + 1 int32 row offsets ON THE DEVICE, cu[0] = 0, strictly increasing, cu[n_songs] = rows; song s owns rows
 * [cu[s], cu[s + 1]) and is scanned from its own row 0 exactly as the rectangular call scans it alone (N = 1, L = its
 * length, segments = 1): same kernels, instantiated with the offset table in place of (N, L).  One workgroup per
 * (song, head), never segmented.  zinv and dden are (rows, H) by packed row; final_state and colsum_* are per
 * (song, head): cwlt_scan_final_state_floats(n_songs, H) floats / (n_songs, H*64) f32.  The host does not read cu: a
 * table that is not as described is the caller's error.  CWLT_ERR_ARG before any launch for NULL pointers, n_songs < 1,
 * head_dim != 64 and row strides the route cannot take (as above: multiples of 4; final_state, colsum_*, dden and the
 * sweep need bf16 with multiples of 8). */
int cwlt_causal_linear_fwd_packed(const void* q, const void* k, const void* v, void* out, float* zinv, const int* cu,
                                  int n_songs, int H, int head_dim,
                                  int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                                  float eps, float* final_state, int dtype, void* stream);
int cwlt_causal_linear_bwd_sweep_packed(const void* q, const void* k, const void* v, const void* out,
                                        const float* zinv, const void* dout, const float* final_state,
                                        void* dq, void* dk, void* dv,
                                        float* colsum_q, float* colsum_k, float* colsum_v,
                                        const int* cu, int n_songs, int H, int head_dim,
                                        int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                                        int64_t lddq, int64_t lddk, int64_t lddv, int dtype, void* stream);
int cwlt_causal_linear_bwd_dkdv_packed(const void* q, const void* k, const void* v, const void* out,
                                       const float* zinv, const void* dout, void* dk, void* dv,
                                       float* colsum_k, float* colsum_v, float* dden,
                                       const int* cu, int n_songs, int H, int head_dim,
                                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                                       int64_t lddk, int64_t lddv, int dtype, void* stream);
int cwlt_causal_linear_bwd_dq_packed(const void* q, const void* k, const void* v, const void* out,
                                     const float* zinv, const void* dout, void* dq, float* colsum_q, const float* dden,
                                     const int* cu, int n_songs, int H, int head_dim,
                                     int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                                     int64_t lddq, int dtype, void* stream);

/* ---- fused residual + dropout + LayerNorm ------------------------------------------------------
 * s = x + dropout_p(a) ; y = LayerNorm(s) * gamma + beta.  Replaces, inside fast_transformers'
 * TransformerEncoderLayer.forward (built at dqn_policy/model.py:128-137, called :232):
 *   x = x + self.dropout(attn(...)); x = self.norm1(x); ... ; self.norm2(x + self.dropout(ffn));
 * and TransformerEncoder's final self.norm(x) (x == NULL, p == 0).
 * x may be NULL (plain LayerNorm of a); s_out may be NULL; mean/rstd (rows) f32 are saved stats.
 * D % 8 == 0, D <= 1024.  Dropout masks are regenerated from (seed, element index) in backward.
 * seed_base (every entry point that takes a seed): optional device pointer to one uint64 that the kernel adds
 * to `seed` when it runs (NULL = 0).  `seed` is baked into a captured hipGraph; bumping *seed_base between
 * replays (itself a captured device op) gives each replay fresh masks.  Forward and backward of one op must
 * see the same seed + *seed_base. */
int cwlt_ln_blocks(int64_t rows);
int cwlt_add_dropout_layernorm_fwd(const void* x, const void* a, const float* gamma, const float* beta,
                                   void* s_out, void* y, float* mean, float* rstd,
                                   int64_t rows, int D, float eps, float p, uint64_t seed,
                                   const uint64_t* seed_base, int dtype, void* stream);
/* dy2 (optional second upstream gradient, summed with dy), ds = d/ds (also the residual gradient),
 * da = dropout-masked ds (NULL when p == 0: then da == ds).  part: cwlt_ln_blocks(rows)*3*D f32
 * workspace; stats: (3, D) f32 output = dgamma | dbeta | dbias, where dbias = column sum of da,
 * i.e. the bias gradient of the Linear that produced `a`. */
int cwlt_add_dropout_layernorm_bwd(const void* dy, const void* dy2, const void* s, const float* gamma,
                                   const float* mean, const float* rstd, void* ds, void* da,
                                   float* part, float* stats,
                                   int64_t rows, int D, float p, uint64_t seed, const uint64_t* seed_base,
                                   int dtype, void* stream);

/* ---- deterministic column sums (bias gradients) -------------------------------------------------
 * out[c] = sum_r x[r*ld + c]; part: cwlt_colsum_blocks(rows)*ncols f32.  Replaces the reductions
 * autograd runs for nn.Linear bias gradients (dqn_policy/model.py:123,156-161). */
int cwlt_colsum_blocks(int64_t rows);
int cwlt_colsum(const void* x, float* part, float* out, int64_t rows, int ncols, int64_t ld,
                int dtype, void* stream);

/* ---- FFN activation: g = dropout_p(gelu(h + bias)) ----------------------------------------------
 * Replaces `self.dropout(self.activation(self.linear1(y)))` (activation='gelu' = exact erf,
 * dqn_policy/model.py:134) with the Linear run bias-free.  bias may be NULL.  F % 8 == 0.
 * f32 tensors: libm erff / expf (the parity path).  bf16 tensors: Phi(-|x|) = exp(-x^2 / 2) * Q(|x|) with a degree-5
 * minimax Q -- value and derivative within 1.5e-4 (absolute) of the exact-erf forms, under the 2^-9 relative rounding of
 * a bf16 result; the GEMM-epilogue forms below use the same function, bit for bit.
 * gd (rows, F), may be NULL: also write the backward's factor gd = mask * 1/(1-p) * gelu'(h + bias), so that
 * dh = dg * gd is one multiply in the epilogue of the GEMM that produces dg (cwlt_gemm_nt_mul).  gd may be h itself
 * (in place: h is then consumed). */
int cwlt_rowslab_blocks(int64_t rows);
int cwlt_bias_gelu_dropout_fwd(const void* h, const float* bias, void* g, void* gd, int64_t rows, int F,
                               float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);
/* dh = dropout_bwd(dg) * gelu'(h + bias); dbias (F) f32 = column sums of dh (NULL to skip);
 * part: cwlt_rowslab_blocks(rows)*F f32 (needed iff dbias). */
int cwlt_bias_gelu_dropout_bwd(const void* dg, const void* h, const float* bias, void* dh,
                               float* part, float* dbias, int64_t rows, int F, float p,
                               uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);

/* ---- FFN backward: dh = (dy . W2) * gd with the activation gradient in the GEMM epilogue --------
 * Replaces, in the backward of fast_transformers' TransformerEncoderLayer (dqn_policy/model.py:128-137), the input
 * gradient of `linear2` (a GEMM writing dg, rows x d_ff) followed by the backward of dropout(gelu(.)) above: the
 * product never reaches memory.  a = dy (M, K), w = linear2.weight TRANSPOSED, (N, K) row-major, g = gd (M, N) from
 * cwlt_bias_gelu_dropout_fwd, c = dh (M, N); all bf16, f32 accumulation, the product rounded to bf16 before the
 * multiply (the arithmetic of the two-kernel path).  colsum (N) f32 = column sums of c = linear1's bias gradient,
 * through part (cwlt_gemm_nt_tiles(M) * N floats), both or neither NULL.  N % 256 == 0, K % 64 == 0, row strides
 * multiples of 8, 16-byte aligned pointers. */
int64_t cwlt_gemm_nt_tiles(int64_t M);
int cwlt_gemm_nt_mul(const void* a, const void* w, const void* g, void* c, float* part, float* colsum,
                     int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldg, int64_t ldc, void* stream);

/* ---- FFN forward: linear1 + bias + GELU + dropout in the GEMM's epilogue ------------------------
 * x = bf16(a (M, K) . w (N, K)^T) + bias (N, f32);  g = dropout_p(gelu(x)),  gd = mask * 1/(1-p) * gelu'(x):
 * `self.dropout(self.activation(self.linear1(y)))` of fast_transformers' TransformerEncoderLayer
 * (dqn_policy/model.py:128-137, activation='gelu' = exact erf; evaluated as cwlt_bias_gelu_dropout_fwd evaluates it for
 * bf16 tensors) together with the factor cwlt_gemm_nt_mul multiplies the
 * upstream gradient with -- what a plain GEMM followed by cwlt_bias_gelu_dropout_fwd(gd) produces (same arithmetic,
 * the pre-activation rounded to bf16 as the GEMM's output would be, same dropout stream keyed by (seed, element
 * index)), without the (M, N) pre-activation's write and read.  w = linear1.weight as stored, (N, K) row-major.
 * g, gd: dense (M, N) bf16, distinct.  N % 256 == 0, K % 64 == 0, lda / ldw multiples of 8, 16-byte aligned. */
int cwlt_gemm_nt_bias_gelu_dropout(const void* a, const void* w, const float* bias, void* g, void* gd,
                                   int64_t M, int N, int K, int64_t lda, int64_t ldw, float p,
                                   uint64_t seed, const uint64_t* seed_base, void* stream);

/* The post-LN residual block in a GEMM's epilogue:  s = x + dropout(bf16(a (M, K) . w (N, K)^T) + bias);
 * y = LayerNorm(s) * gamma + beta;  mean, rstd per row -- `x = norm1(x + dropout(attention.out_projection(.)))` and
 * `norm2(x + dropout(linear2(.)))` of fast_transformers' post-LN TransformerEncoderLayer reached from
 * /root/reference/dqn_policy/model.py:128-137,231-232; replaces a GEMM with bf16 output followed by
 * cwlt_add_dropout_layernorm_fwd (same dropout stream (seed, row * N + column), same statistics, same rounding points;
 * the bias is added in f32).  The GEMM's output never reaches HBM.  a, w bf16 with row strides lda, ldw (multiples
 * of 8); x, s, y (M, N) bf16 dense; bias, gamma, beta (N) f32; mean, rstd (M) f32.  N == 512 (a workgroup owns whole
 * rows), K % 64 == 0, 16-byte aligned pointers, 0 <= p < 1. */
int cwlt_gemm_nt_bias_dropout_add_layernorm(const void* a, const void* w, const float* bias, const void* x,
                                            const float* gamma, const float* beta, void* s, void* y, float* mean,
                                            float* rstd, int64_t M, int N, int K, int64_t lda, int64_t ldw, float eps,
                                            float p, uint64_t seed, const uint64_t* seed_base, void* stream);

/* ---- the dense projections: C (M, N) [+]= A (M, K) . W (N, K)^T [+ bias] -------------------------
 * The `nn.Linear`s of fast_transformers' AttentionLayer / TransformerEncoderLayer (query / key / value / out projection,
 * linear1, linear2: /root/reference/dqn_policy/model.py:128-137) and the six output heads as one projection
 * (dqn_policy/model.py:156-161,241-249), forward and input-gradient forms -- what `torch.addmm / mm / addmm_` sent to
 * hipBLASLt.  a (M, K), w (N, K), c (M, N) bf16 row-major with row strides lda, ldw, ldc; f32 accumulation; bias (N)
 * f32 or NULL.  Forward: w = the layer's weight as stored.  Input gradient: w = the weight TRANSPOSED (dx = dy . W needs
 * W's columns K-contiguous: pass w = W^T, (in, out) -> rows of length `out`); accumulate != 0 adds the product onto
 * the bf16 values already in c (the residual gradient: `ds.addmm_(dh, W1)`).  256 x 256 tiles, LDS-DMA half-tile
 * ring, v_mfma_f32_16x16x32_bf16 (csrc/gemm_bf16.hip).  N % 8 == 0, K % 64 == 0, K >= 128, strides multiples of 8,
 * 16-byte aligned pointers (N <= 8192 with a bias: the strip is kept in LDS).  Persistent: one workgroup per CU walks the
 * tiles, the next tile's first operand pieces are requested before this tile's stores.
 * cwlt_gemm_bf16_tune(variant, trace): tuning numbers and the diagnostic build (tools/bench_gemm.py); variant < 0: the
 * defaults.  Bits 1-3: start stagger of the workgroups in eighths of a tile period (default: 4 for K <= 1024, else 0);
 * bits 8-15: at most that many x 8 workgroups (0: one per CU).  A variant >= 0 with any other bit set returns
 * CWLT_ERR_ARG and leaves the current state as it was.  trace != NULL (8192 uint32 of device memory): bias-free,
 * non-accumulating launches run the diagnostic build and leave workgroup 0's s_memtime stamps of its second tile there. */
int cwlt_gemm_bf16(const void* a, const void* w, const float* bias, void* c, int64_t M, int N, int K, int64_t lda,
                   int64_t ldw, int64_t ldc, int accumulate, void* stream);
int cwlt_gemm_bf16_tune(int variant, void* trace);

/* ---- positional encoding + dropout --------------------------------------------------------------
 * y = dropout_p(x + pe[r % T]) -- PositionalEncoding.forward, dqn_policy/model.py:90-92.  pe is the
 * registered (max_len, D) f32 buffer; pe == NULL gives plain dropout, which is also this op's
 * backward (dx = dropout with the same seed applied to dy). */
int cwlt_posenc_dropout(const void* x, const float* pe, void* y, int64_t rows, int T, int D,
                        float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);
/* Positions from a table (packed songs): y = dropout_p(x + pe[pos[r]]), pos = `rows` int32 ON THE DEVICE, each inside the
 * pe buffer (the caller's check: the host does not read it); pe and pos must be given.  Row r keeps the dropout stream
 * cwlt_posenc_dropout gives row r for the same seed, so the backward is still cwlt_posenc_dropout(dy, pe = NULL). */
int cwlt_posenc_dropout_pos(const void* x, const float* pe, const int* pos, void* y, int64_t rows, int D,
                            float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);

/* ---- compound-word multi-embedding --------------------------------------------------------------
 * out[r, off_f : off_f+width_f] = table_f[tokens[r, f]] * sqrt(width_f), f = 0..n_attr-1.
 * Replaces Embeddings.forward x6 + torch.cat (dqn_policy/model.py:67-74,206-221;
 * ppo_policy/model.py:69-76,208-223; dqn_policy/AIRL_model.py:34-41,108-115).
 * tables / widths / nrows are HOST arrays (device pointers to f32 tables; widths % 64 == 0).  out: 16-byte aligned,
 * row stride ldo a multiple of 8 elements (bf16) / 4 (f32). */
int cwlt_embed_splits(int64_t rows);
int cwlt_cw_embed_fwd(const int64_t* tokens, const void* const* tables, const int* widths,
                      const int* nrows, int n_attr, void* out, int64_t rows, int64_t ldo,
                      int dtype, void* stream);
/* dtables: one flat f32 buffer, table f's gradient at element offset sum_{g<f} nrows[g]*widths[g];
 * part: cwlt_embed_splits(rows) * (total table elements) f32.  Deterministic (no atomics). */
int cwlt_cw_embed_bwd(const int64_t* tokens, const int* widths, const int* nrows, int n_attr,
                      const void* dout, float* part, float* dtables, int64_t rows, int64_t ldd,
                      int dtype, void* stream);
/* The whole input front in one pass -- embedding x6 + cat + in_linear + PositionalEncoding
 * (dqn_policy/model.py:206-223 and 90-92; ppo_policy/model.py:208-225) -- from PROJECTED tables:
 *   out[r, :] = dropout(sum_f tproj[rowofs_f + tokens[r, f], :] + bias + pe[r % T, :]),  rowofs_f = sum_{g<f} nrows[g],
 *   tproj = cat_f(sqrt(width_f) * table_f . W_in[:, cols_f]^T)   (sum nrows, D), built by the caller per step.
 * The (rows, sum widths) concatenated embeddings and the in_linear GEMM over the token rows do not exist on this path.
 * tproj has out's dtype (bf16 / f32), dense; bias (D), pe (max_len >= T, D) f32 (pe may be NULL); out (rows, D) dense;
 * 16-byte aligned pointers; D % 64 == 0, D <= 2048; ids outside [0, nrows) are clamped; 0 <= p < 1.  The dropout
 * stream is cwlt_posenc_dropout's for the same seed. */
int cwlt_cw_embed_proj_fwd(const int64_t* tokens, const void* tproj, const int* nrows, int n_attr,
                           const float* bias, const float* pe, void* out, int64_t rows, int T, int D,
                           float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);
/* The same with positions from a table (packed songs): pe[pos[r], :] in place of pe[r % T, :]; pos as in
 * cwlt_posenc_dropout_pos, pe must be given.  The backward below never reads pe and serves both. */
int cwlt_cw_embed_proj_fwd_pos(const int64_t* tokens, const void* tproj, const int* nrows, int n_attr,
                               const float* bias, const float* pe, const int* pos, void* out, int64_t rows, int D,
                               float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);
/* dtproj[rowofs_f + id, :] = sum of dpre[r, :] over the token rows with tokens[r, f] == id ((sum nrows, D) f32), dpre =
 * the gradient in front of the dropout (cwlt_posenc_dropout(dout, pe = NULL) with the forward's seed), row stride ldd.
 * The bias gradient is the column sum of any ONE attribute's rows of dtproj.
 * part: cwlt_embed_splits(rows) * (sum nrows) * D f32.  Deterministic (no atomics). */
int cwlt_cw_embed_proj_bwd(const int64_t* tokens, const int* nrows, int n_attr, int D, const void* dpre,
                           float* part, float* dtproj, int64_t rows, int64_t ldd, int dtype, void* stream);

/* ---- per-attribute softmax heads ----------------------------------------------------------------
 * logits (rows, ld), attribute f in columns [sum_{g<f} n_class[g], + n_class[f]) (n_class: HOST
 * array, each <= 256).  Replaces compute_loss x6 (dqn_policy/model.py:163-197: CE(reduction='none')
 * * loss_mask, summed) and Softmax + argmax x6 (dqn_policy/IRL_dqn_train.py:244-250,
 * ppo_policy/ppo_train.py:259-267).  Outputs (each may be NULL): loss_sum (n_attr) =
 * sum_r mask_r * nll_{r,f} [caller divides by sum(mask)]; argmax (rows, n_attr) int64 = first index
 * of the largest softmax value; pmax (rows, n_attr) its probability; probs (rows, ldp) the softmax.
 * loss_part: cwlt_heads_blocks(rows) * n_attr f32. */
int cwlt_heads_blocks(int64_t rows);
/* Which of the two kernel families cwlt_heads_fwd / _ce_bwd / _logp_bwd run these arguments on (the launchers ask
 * this very function): 1 = the tiled kernels (32 rows staged in LDS with 16-byte accesses), 0 = the wave-per-row
 * kernels (n_attr == 8, ld not a multiple of 4 (f32) / 8 (bf16) elements, p0 or p1 not 16-byte aligned, or
 * ld >= 480), negative = -(the CWLT_ERR_* the entry points return for them).  p0 = logits, p1 = dlogits
 * (NULL: the forward, which has none). */
int cwlt_heads_tiled(const int* n_class, int n_attr, int64_t ld, int dtype, const void* p0, const void* p1);
int cwlt_heads_fwd(const void* logits, const int* n_class, int n_attr, const int64_t* target,
                   const float* mask, float* loss_part, float* loss_sum, int64_t* argmax,
                   float* pmax, float* probs, int64_t rows, int64_t ld, int64_t ldp,
                   int dtype, void* stream);
/* dlogits = (softmax - onehot(target)) * mask_r * coef[f]; coef (n_attr) f32 on device. */
int cwlt_heads_ce_bwd(const void* logits, const int* n_class, int n_attr, const int64_t* target,
                      const float* mask, const float* coef, void* dlogits, int64_t rows, int64_t ld,
                      int dtype, void* stream);

/* ---- sliding-window attention of the AIRL discriminator --------------------------------
 * Replaces HF LongformerSelfAttention.forward (banded scores -> fp32 softmax -> probs @ value) as
 * reached from dqn_policy/AIRL_model.py:78-90,117 (attention_window 50) and ppo_policy/model.py:440-451,470
 * (attention_window 512).  q, k, v, out: (B, L, H, 64), row strides ld*; mask (B, L) f32, nonzero =
 * attend (NULL = all); window = one-sided width (attention_window / 2); scale = 1/sqrt(64) applied to q;
 * masked queries produce zero rows; p = dropout on the probabilities. */
int cwlt_band_attn_fwd(const void* q, const void* k, const void* v, const float* mask, void* out, float* lse,
                       int B, int H, int L, int head_dim, int window,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                       float scale, float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);

/* Backward of cwlt_band_attn_fwd -- what torch autograd derives through HF LongformerSelfAttention when the
 * reference trains the discriminator (dqn_policy/AIRL.py:135-170, global_loss.backward()).  lse (B, H, L) f32 =
 * the forward's optional log-sum-exp output (+inf on zeroed query rows; pass NULL to the forward when no
 * backward follows); out = the forward's output; dout its gradient (row stride lddo).  dq, dk, dv: gradients
 * w.r.t. the raw q, k, v, same (B, L, H, 64) layout with row strides lddq / lddk / lddv.  The dropout mask is
 * regenerated from (seed, b, h, i, j). */
int cwlt_band_attn_bwd(const void* q, const void* k, const void* v, const float* mask, const void* out,
                       const float* lse, const void* dout, void* dq, void* dk, void* dv,
                       int B, int H, int L, int head_dim, int window,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                       int64_t lddq, int64_t lddk, int64_t lddv,
                       float scale, float p, uint64_t seed, const uint64_t* seed_base, int dtype, void* stream);

/* Gradient of sum_{r,f} w[r][f] * log softmax_f(logits_r)[target[r][f]] w.r.t. the logits, given as the kernel
 * form dlogits = (softmax - onehot(target)) * w: pass w = -(upstream gradient).  Used for the PPO log pi(a)
 * of the greedy action (ppo_policy/ppo_train.py:320-336).  w (rows, n_attr) f32 on device. */
int cwlt_heads_logp_bwd(const void* logits, const int* n_class, int n_attr, const int64_t* target,
                        const float* w, void* dlogits, int64_t rows, int64_t ld, int dtype, void* stream);

/* ---- RL arithmetic (one launch each; the reference's indexing quirks reproduced) -----------------
 * PRECONDITION (not checked on the device): every ids[r][t][f] given to cwlt_rollout_gather (modes 1, 2, which
 * index probs with it) and every action[j][k][f] given to cwlt_dqn_td_fwd / _bwd lies in [0, n_class[f]).  A value
 * outside its attribute reads (gather, TD forward) or writes (TD backward) outside the attribute's column segment.
 * cwlt_rollout_gather: greedy action rows (+ log-probs) from per-position argmax ids (R, T, A) int64 and
 *   softmax probs (R, T, ldp) f32.  mode 0 = DQN.choose_action (dqn_policy/IRL_dqn_train.py:256-264:
 *   positions [0, T-1, T-2, ...] because -0 == 0); mode 1 = PPO.choose_action (ppo_policy/ppo_train.py:
 *   269-290: rows at -1..-NA, tempo/chord log-prob class taken at position +idx); mode 2 = select_udpate
 *   (ppo_train.py:312-336, no quirk).  action (R, NA, A) int64, logp (R, NA, A) f32 (modes 1, 2). */
int cwlt_rollout_gather(const int64_t* ids, const float* probs, const int* n_class, int n_attr,
                        int64_t* action, float* logp, int R, int T, int NA, int64_t ldp, int mode,
                        void* stream);
/* PPO.calculate_returns + calculate_advantages (ppo_train.py:348-363): forward-order discounted sums,
 * (x - mean) / unbiased std, adv = returns - values, normalised.  E in [2, 8192]. */
int cwlt_ppo_returns_adv(const float* rewards, const float* values, float* returns, float* adv, int E,
                         float gamma, int normalize, void* stream);
/* PPO surrogate (ppo_train.py:388-396): L = -mean(min(0.2*A_e, clamp(exp(new - old), 1-clip, 1+clip)*A_e));
 * new_logp (NA, A) f32, old_logp (E, NA, A) int64 (stored log-probs truncated to integers), adv (E) f32.
 * Outputs loss (1) and grad (NA, A) = dL/dnew_logp. */
int cwlt_ppo_policy_loss(const float* new_logp, const int64_t* old_logp, const float* adv, float* loss,
                         float* grad, int E, int NA, int n_attr, float clip, void* stream);
/* DQN TD loss (dqn_policy/IRL_dqn_train.py:285-330): q gather from batch element 0 (index shape (1, B, NA)),
 * target = reward + gamma (1 - done) topk_NA(max_c target_logits), per-attribute MSE.  y, yt (B, T, ld) f32.
 * mse_part (B, A): sum_k squared error; dq (B, NA, A): d MSEloss / d qval. */
int cwlt_dqn_td_fwd(const float* y, const float* yt, const int* n_class, int n_attr, const int64_t* action,
                    const float* reward, const float* done, float* mse_part, float* dq, int B, int T,
                    int NA, int64_t ld, float gamma, void* stream);
/* scatter dq into the gradient rows of batch element 0 of y (dy zero-filled by the caller), times *gout */
int cwlt_dqn_td_bwd(const float* dq, const int64_t* action, const int* n_class, int n_attr, float* dy,
                    const float* gout, int B, int NA, int64_t ld, void* stream);

/* ---- weight-gradient GEMM of the dense projections ------------------------------------------------
 * out (N1, N2) f32 (+)= A^T B with A = upstream gradient (M, N1), B = layer input (M, N2), bf16 row-major,
 * M = B*T token rows (the reduction).  Replaces the weight-gradient GEMMs autograd runs for the nn.Linear
 * layers of the encoder (dqn_policy/model.py:128-137; FT AttentionLayer / TransformerEncoderLayer).
 * N1, N2 multiples of 256; part: cwlt_wgrad_splits(M, N1, N2) * N1 * N2 f32.  Deterministic. */
int cwlt_wgrad_splits(int64_t M, int N1, int N2);
int cwlt_wgrad_bf16(const void* a, const void* b, float* part, float* out, int64_t M, int N1, int N2,
                    int64_t lda, int64_t ldb, int accumulate, void* stream);

/* Up to four such products over the SAME M token rows in one launch + one reduce launch: the four weight gradients of an
 * encoder layer at few token rows run 20-80 workgroups each, 240 together.  All arrays are HOST arrays of `count` (1..4)
 * entries; widths multiples of 256; part[p]: cwlt_wgrad_splits(M, n1[p], n2[p]) * n1[p] * n2[p] floats, distinct buffers.
 * Results bit-identical to count calls of cwlt_wgrad_bf16 (every product cuts the rows as its own launch would). */
int cwlt_wgrad_bf16_group(const void* const* a, const void* const* b, float* const* part, float* const* out, const int* n1,
                          const int* n2, const int64_t* lda, const int64_t* ldb, int count, int64_t M, int accumulate,
                          void* stream);

/* ---- recurrent (generation) form of the causal linear attention ------------------------------------
 * One token: Zi += phi(k); Si += phi(k) (x) v; out = (phi(q) . Si) / (phi(q) . Zi + eps), state updated in
 * place.  Replaces fast_transformers RecurrentLinearAttention.forward as built by RecurrentEncoderBuilder at
 * dqn_policy/model.py:141-150 and driven by dqn_policy/testing-no-type-cp.py:126-179.
 * q, k, v, out: (N, H*64) rows (row strides ld*); S (N, H, 64, 64) f32; Z (N, H, 64) f32. */
int cwlt_recurrent_cla_step(const void* q, const void* k, const void* v, float* S, float* Z, void* out,
                            int N, int H, int head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                            float eps, int dtype, void* stream);

/* ---- prompt prefill: the chunked scan started from, and handing back, the recurrent state ----------------------
 * The state a prompt of len tokens leaves behind, and its attention rows, in ONE pass per (sequence, head) instead of
 * len calls of cwlt_recurrent_cla_step (same values up to the order of the f32 sums): the generation-time
 * continuation of a prompt (the reference's write_midi(..., prompt_path=...), ppo_policy/utils.py:219,308, and its
 * prompt loop over `init`, dqn_policy/testing-no-type-cp.py:135-152).
 * q, k, v, out: (N, L, H, head_dim) as cwlt_causal_linear_fwd (row strides ld*, multiples of 4, 16-byte aligned q, k,
 * v).  S (N, H, 64, 64) f32 key-feature-major (S[n,h,d,m]) and Z (N, H, 64) f32 -- cwlt_recurrent_cla_step's state --
 * are read as the starting state and overwritten in place with the state after the sequence's last valid token:
 *   out_l = phi(q_l) . (S0 + sum_{j<=l} phi(k_j) (x) v_j) / (phi(q_l) . (Z0 + sum_{j<=l} phi(k_j)) + eps).
 * lengths: DEVICE int32 (N) or NULL (= all L); rows t >= lengths[n] add nothing and their out rows are not written, a
 * length of 0 leaves that sequence's S and Z bit-for-bit unchanged (lengths are clamped to [0, L]).
 * f32 only (CWLT_ERR_DTYPE otherwise); head_dim != 64 is CWLT_ERR_ARG.
 * Few streams (one song is N * H = 8 workgroups on 256 CUs): `segments` > 1 cuts every sequence into runs of whole
 * 32-token chunks, one workgroup each -- a first pass reduces each run to its state increment, a second turns the
 * increments into starting states (S0, Z0 included), the scan proper starts every run from its state and the run
 * holding a sequence's last chunk writes the final state.  cwlt_prefill_segments() is the library's choice (1 once
 * the streams fill the chip); seg_ws: cwlt_prefill_seg_floats(N, H, segments) floats, NULL when segments == 1.  A run
 * owns ceil(chunks / segments) chunks (chunks = ceil(L / 32)) and every run must own at least one
 * ((segments - 1) * ceil(chunks / segments) < chunks), else CWLT_ERR_ARG. */
int cwlt_prefill_segments(int N, int H, int L);
int64_t cwlt_prefill_seg_floats(int N, int H, int segments);
int cwlt_causal_linear_fwd_state(const void* q, const void* k, const void* v, void* out, float* S, float* Z,
                                 const int* lengths, int N, int H, int L, int head_dim, int64_t ldq, int64_t ldk,
                                 int64_t ldv, int64_t ldo, float eps, int segments, float* seg_ws, int dtype,
                                 void* stream);
/* Packed form: songs of different lengths laid end to end in (rows, H, 64) row buffers, as the packed scans above.  cu:
 * n_songs + 1 int32 row offsets ON THE DEVICE (cu[0] = 0, strictly increasing; the host does not read it); song s owns
 * rows [cu[s], cu[s + 1]), starts from S[s], Z[s] ((n_songs, H, 64, 64) / (n_songs, H, 64)) and leaves there the state
 * after its last row.  The same kernel with the offset table in place of (lengths, L): one workgroup per (song, head)
 * runs ceil(len / 32) chunks from the song's own row 0, never segmented, so out rows, S and Z of a song are bitwise
 * those of cwlt_causal_linear_fwd_state on that song alone (N = 1, L = len, segments = 1) and no row outside
 * [0, cu[n_songs]) is read or written.  Refusals as above, plus a NULL cu; n_songs = 0 launches nothing. */
int cwlt_causal_linear_fwd_state_packed(const void* q, const void* k, const void* v, void* out, float* S, float* Z,
                                        const int* cu, int n_songs, int H, int head_dim, int64_t ldq, int64_t ldk,
                                        int64_t ldv, int64_t ldo, float eps, int dtype, void* stream);

/* ---- generation: one CW token through the whole recurrent-form model (f32) --------------------------
 * Replaces the per-token body of the reference's generation loop: `forward_hidden(input_, memory,
 * is_training=False)` (dqn_policy/testing-no-type-cp.py:150,166 -> dqn_policy/model.py:200-238 -> the
 * RecurrentEncoderBuilder product of dqn_policy/model.py:141-150) followed by the six head projections of
 * `forward_output_sampling` (dqn_policy/model.py:273-278); likewise ppo_policy/inference.py:78-160 over
 * ppo_policy/model.py:200-262.  All pointers are device pointers unless marked HOST; the structs themselves
 * are HOST memory, read during the call only.  Per-song state S / Z is updated in place. */
typedef struct cwlt_decode_layer {
    const float *wqkv, *bqkv;     /* (3D, D), (3D): query | key | value projection rows stacked */
    const float *wo, *bo;         /* (D, D), (D): out_projection */
    const float *ln1_w, *ln1_b;   /* norm1 */
    const float *w1, *b1;         /* (F, D), (F): linear1 */
    const float *w2, *b2;         /* (D, F), (D): linear2 */
    const float *ln2_w, *ln2_b;   /* norm2 */
    float *S, *Z;                 /* (n_songs, H, 64, 64), (n_songs, H, 64) f32 recurrent state */
} cwlt_decode_layer;

typedef struct cwlt_decode_model {
    int n_layer, n_head, d_model, d_ff, n_attr, emb_width, n_logits;
    float eps_ln, eps_attn;            /* 1e-5, 1e-6 in the reference */
    const void* const* tables;         /* HOST array of n_attr device pointers (f32 embedding tables) */
    const int* widths;                 /* HOST (n_attr): embedding widths, sum = emb_width */
    const int* nrows;                  /* HOST (n_attr): vocabulary sizes */
    const float *w_in, *b_in;          /* (D, emb_width), (D): in_linear */
    const float* pe0;                  /* (D): row 0 of the positional-encoding buffer (pos_emb.pe) */
    const cwlt_decode_layer* layers;   /* HOST array of n_layer */
    const float *lnf_w, *lnf_b;        /* final encoder norm (NULL: none) */
    const float *w_heads, *b_heads;    /* (n_logits, D), (n_logits): the proj_* heads stacked */
} cwlt_decode_model;

/* floats of workspace PER SONG (-1: unsupported model: needs d_model = 64*n_head <= 2048, d_ff <= 2048,
 * emb_width <= 2048, all multiples of 4) */
int64_t cwlt_decode_workspace_floats(const cwlt_decode_model* m);
/* tokens: (n_songs, n_attr) int64; work: n_songs * cwlt_decode_workspace_floats(m) f32 (16-byte aligned);
 * hidden: (n_songs, D) f32 or NULL -- what forward_hidden returns; logits: (n_songs, n_logits) f32. */
int cwlt_decode_step(const cwlt_decode_model* m, const int64_t* tokens, float* work, float* hidden,
                     float* logits, int n_songs, void* stream);
/* The step's building block: out[n, r] = epi(W[r, :] . pro(xin[n, :]) + bias[r]); pro = optional LayerNorm
 * (ln_w, ln_b) and an optional second one (ln2_w, ln2_b), the normalised vector also stored to x_out when given;
 * epi = exact-erf GELU when act == 1, then + res[n, r] when res != NULL.  K % 4 == 0, K <= 2048. */
int cwlt_decode_gemv(const float* W, const float* bias, const float* xin, const float* ln_w,
                     const float* ln_b, const float* ln2_w, const float* ln2_b, float eps,
                     const float* res, float* out, float* x_out, int n_out, int K, int act, int n_songs,
                     int64_t ld_x, int64_t ld_res, int64_t ld_out, int64_t ld_xo, void* stream);

/* ---- generation: the same token step for many songs at once, projections as f32 MFMA GEMMs (csrc/decode_gemm.hip)
 * cwlt_decode_gemm: cwlt_decode_gemv's product, prologue and epilogue for n_songs rows (1..4096), each weight read
 * once per 64 songs.  Exact f32 (v_mfma_f32_16x16x4_f32) and batch invariant: a row's result is bitwise the same
 * whatever n_songs, its position or the other rows.  K % 16 == 0, 16 <= K <= 2048, n_out <= 4096, ld_x (and ld_xo
 * with a prologue) multiples of 4.  scratch: cwlt_decode_gemm_scratch_floats(n_out, K, n_songs) f32 (16-byte aligned),
 * the split-K partials and, when a prologue has no x_out, the normalised rows; -1 for an unsupported shape. */
int64_t cwlt_decode_gemm_scratch_floats(int n_out, int K, int n_songs);
int cwlt_decode_gemm(const float* W, const float* bias, const float* xin, const float* ln_w,
                     const float* ln_b, const float* ln2_w, const float* ln2_b, float eps,
                     const float* res, float* out, float* x_out, int n_out, int K, int act, int n_songs,
                     int64_t ld_x, int64_t ld_res, int64_t ld_out, int64_t ld_xo, float* scratch, void* stream);
/* cwlt_decode_step's arguments and outputs, its projections on cwlt_decode_gemm.  work: the per-song rows of
 * cwlt_decode_step (n_songs * cwlt_decode_workspace_floats(m)) followed by the GEMMs' scratch,
 * cwlt_decode_rows_workspace_floats(m, n_songs) floats in all (-1: unsupported model or n_songs outside 1..4096;
 * the model also needs d_model, d_ff and emb_width multiples of 16). */
int64_t cwlt_decode_rows_workspace_floats(const cwlt_decode_model* m, int n_songs);
int cwlt_decode_step_rows(const cwlt_decode_model* m, const int64_t* tokens, float* work, float* hidden,
                          float* logits, int n_songs, void* stream);

/* Device-side sampling of the next CW token: for each of `rows` songs and each attribute a, draw from
 * Categorical(softmax(logits[row, off_a : off_a + n_class[a]] / temperature[a])) and store the class id in
 * tokens[row, a] (and in song[counter, row, a] when song != NULL and *counter < song_rows).  Replaces the six
 * `Categorical(softmax(y)).sample()` draws + torch.cat of ppo_policy/inference.py:115-141 (same distribution; the
 * generator is counter-based, keyed by (seed, *counter, row, a), so a captured graph draws fresh numbers per replay
 * as long as the caller advances *counter).  top_p[a] < 1 restricts attribute a to its nucleus first -- the
 * smallest set of most-probable classes whose mass exceeds top_p[a], renormalised: `nucleus` of
 * dqn_policy/model.py:33-47, with temperature[a] its `softmax_with_temperature` (:19-21).
 * n_class / temperature / top_p: HOST arrays (NULL = 1.0); n_class[a] <= 256, n_attr <= 8; counter: device int64
 * (NULL = 0). */
int cwlt_sample_categorical(const float* logits, const int* n_class, const float* temperature,
                            const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                            const int64_t* counter, int64_t* tokens, int64_t* song, int64_t song_rows,
                            void* stream);
/* The same draw keyed by (seed, *counter, song row, attribute) independently of `rows`: song n's tokens are the same
 * whatever the number of songs in the launch (cwlt_sample_categorical mixes `rows` into the key; both give the same
 * keys when rows == 1).  Used by many-song generation, whose songs must not depend on the batch size; *counter < 2^40. */
int cwlt_sample_categorical_slots(const float* logits, const int* n_class, const float* temperature,
                                  const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                  const int64_t* counter, int64_t* tokens, int64_t* song, int64_t song_rows,
                                  void* stream);
/* The slot-keyed draw with per-row keys (DEVICE int64 arrays): row n draws what cwlt_sample_categorical_slots draws for
 * row key[n] at counter step[n] (key[n] < 2^20, step[n] < 2^40).  Continuous batching keys a slot's draw by (song index,
 * position in song), so a song's tokens do not depend on the slot it runs in or on when it started. */
int cwlt_sample_categorical_keyed(const float* logits, const int* n_class, const float* temperature,
                                  const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                  const int64_t* key, const int64_t* step, int64_t* tokens, void* stream);
/* Constrained draw (generation.Constraint): the slot-keyed draw with disallowed classes removed.  Keyed as
 * cwlt_sample_categorical_keyed when key and step are given (song k = key[n]), otherwise as
 * cwlt_sample_categorical_slots at *counter (song k = n).  Row n uses mask row sched[2k] + min(bar[n] - 1,
 * sched[2k + 1] - 1) of `masks` (mask_rows x mask_words uint32, class c of attribute a is bit off[a] + c with off the
 * running sum of n_class); bar (DEVICE int64 x rows) is the song's bar count before this row, sched (DEVICE int64,
 * n_sched x {first row, rows}).  Disallowed classes are -inf logits before the temperature, the max, the softmax and
 * the nucleus (top_p over the renormalised allowed mass).  With every bit set the draw is bitwise the unmasked one.
 * Rows with k < 0 or k >= n_sched, songs with a 0-row schedule, and mask rows outside [0, mask_rows) draw unmasked.
 * Refused: null bar / sched / masks, key without step (or neither key nor counter), mask_words * 32 < sum n_class,
 * rows > 2^20. */
int cwlt_sample_categorical_masked(const float* logits, const int* n_class, const float* temperature,
                                   const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                   const int64_t* counter, const int64_t* key, const int64_t* step, const int64_t* bar,
                                   const int64_t* sched, int64_t n_sched, const uint32_t* masks, int64_t mask_rows,
                                   int mask_words, int64_t* tokens, void* stream);
/* Draw with log-probabilities: the slot-keyed draw at *counter (key = step = NULL), or keyed per row by
 * key / step, as cwlt_sample_categorical_slots / _keyed; masked as cwlt_sample_categorical_masked when bar, sched and
 * masks are given (all three, or none).  Tokens are those entries' tokens, bit for bit.  For the drawn class c of row
 * n, attribute a, it also writes the f32 pair {lp_model, lp_sampler} to logp[((o * rows + n) * n_attr + a) * 2] with
 * o = *out_counter % out_rows (out_counter: DEVICE int64, e.g. the counter the caller advances after the draw; NULL
 * needs out_rows == 1).  lp_model = log_softmax(raw logits)[c]; lp_sampler = log q(c), q the distribution of the draw:
 * tempered logits v, disallowed classes -inf, the nucleus kept set, renormalised: (v_c - m) - log(sum over kept e).
 * Refused: null logp, key without step (or neither key nor counter), a partial mask table, out_rows < 1,
 * rows > 2^20, and what cwlt_sample_categorical refuses. */
int cwlt_sample_categorical_logp(const float* logits, const int* n_class, const float* temperature,
                                 const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                 const int64_t* counter, const int64_t* key, const int64_t* step, const int64_t* bar,
                                 const int64_t* sched, int64_t n_sched, const uint32_t* masks, int64_t mask_rows,
                                 int mask_words, int64_t* tokens, float* logp, const int64_t* out_counter,
                                 int64_t out_rows, void* stream);
/* Score given classes: the pair cwlt_sample_categorical_logp writes, for class targets[n * n_attr + a] (DEVICE int64,
 * rows x n_attr) of row n of logits (rows x ld f32), into logp[(n * n_attr + a) * 2] (rows x n_attr x 2 f32).  The
 * same kernel body as the draw: the logits a draw came from, scored at the class it drew, give its pair bitwise.
 * Masked when bar (the bar count of row n), sched and masks are given, with song key[n] (NULL: n) as in
 * cwlt_sample_categorical_masked.  A negative target (padding) leaves its pair unwritten; a target >= n_class[a]
 * gets {-inf, -inf}.  Refused: null targets / logp, a partial mask table, rows > 2^20, what cwlt_sample_categorical
 * refuses. */
int cwlt_score_categorical(const float* logits, const int* n_class, const float* temperature, const float* top_p,
                           int n_attr, int64_t rows, int64_t ld, const int64_t* targets, const int64_t* key,
                           const int64_t* bar, const int64_t* sched, int64_t n_sched, const uint32_t* masks,
                           int64_t mask_rows, int mask_words, float* logp, void* stream);
/* The batch loop's bar count in constrained mode, enqueued after each draw: bar[n] += 1 (DEVICE int64 x rows) when
 * tokens[n, bar_attr] is a class c < bar_classes with bar_mask[c] != 0 (DEVICE int32).  rows <= 2^20. */
int cwlt_count_bars(const int64_t* tokens, int64_t rows, int n_attr, int bar_attr, const int* bar_mask,
                    int bar_classes, int64_t* bar, void* stream);

/* Row grammar (generation.Grammar): the draw of cwlt_sample_categorical_logp -- slot-keyed at *counter or
 * keyed per row by key / step, masked when bar, sched and masks are given (all three, or none) -- in which the
 * attributes of a row depend on one another.  Attribute bar_attr (bar-beat) is drawn first, under the mask row AND the
 * position rule: with b = beat[n] (DEVICE int64 x rows: -1 after a Bar row, k after Beat_k) and o = order[c] (DEVICE
 * int32 x n_order >= n_class[bar_attr]: -2 the neutral class, -1 a Bar class, k >= 0 Beat_k, -3 never allowed), class
 * c is allowed when o == -1, or o >= 0 and o > b, or o == -2 and b >= 0.  The drawn class fixes the row's kind (o ==
 * -2 NOTE, -1 BAR, >= 0 BEAT) and every other attribute is drawn under the mask row AND row `kind` of gram (DEVICE
 * uint32, 3 x gram_words, rows NOTE / BAR / BEAT, bit layout of `masks`).  Keys, temperature, nucleus and the -inf
 * treatment of removed classes are those of cwlt_sample_categorical_masked; with order all -1 and gram all ones the
 * tokens and pairs are bitwise those of cwlt_sample_categorical_keyed / _masked / _logp.  logp (optional): the pairs of
 * cwlt_sample_categorical_logp, lp_sampler the log q of the distribution each class was drawn from (bar-beat: given
 * the position; the others: given the row's kind).
 * Refused: null beat / order / gram / tokens, bar_attr outside [0, n_attr), n_order < n_class[bar_attr],
 * gram_words * 32 < sum n_class, and what cwlt_sample_categorical_logp refuses (out_rows only with logp). */
int cwlt_sample_categorical_grammar(const float* logits, const int* n_class, const float* temperature,
                                    const float* top_p, int n_attr, int64_t rows, int64_t ld, uint64_t seed,
                                    const int64_t* counter, const int64_t* key, const int64_t* step,
                                    const int64_t* bar, const int64_t* sched, int64_t n_sched, const uint32_t* masks,
                                    int64_t mask_rows, int mask_words, const int64_t* beat, const int* order,
                                    int n_order, const uint32_t* gram, int gram_words, int bar_attr, int64_t* tokens,
                                    float* logp, const int64_t* out_counter, int64_t out_rows, void* stream);
/* cwlt_score_categorical under the row grammar: the kind of row n is that of its target's bar-beat class, beat[n] the
 * position before the row.  An ill-formed target gets -inf in the sampler column of the offending attribute (bar-beat:
 * a class the position rule removes; another attribute: a class outside the kind's gram row, every class when the
 * bar-beat target is -3 or out of range) and a finite model column. */
int cwlt_score_categorical_grammar(const float* logits, const int* n_class, const float* temperature,
                                   const float* top_p, int n_attr, int64_t rows, int64_t ld, const int64_t* targets,
                                   const int64_t* key, const int64_t* bar, const int64_t* sched, int64_t n_sched,
                                   const uint32_t* masks, int64_t mask_rows, int mask_words, const int64_t* beat,
                                   const int* order, int n_order, const uint32_t* gram, int gram_words, int bar_attr,
                                   float* logp, void* stream);
/* The grammar's position after each draw, one thread per row: when fresh[n] != 0 and song[n] >= 0 (the slot was just
 * handed a song) beat[n] = beat0[song[n]] (DEVICE int64 x n_songs, the position each song's prompt leaves); otherwise
 * beat[n] moves by o = order[tokens[n, bar_attr]]: -1 (Bar) and k >= 0 (Beat_k) are stored, anything else leaves it.
 * fresh, song and beat0 are given together or all NULL (the lock-step loop).  rows <= 2^20. */
int cwlt_grammar_track(const int64_t* tokens, int64_t rows, int n_attr, int bar_attr, const int* order, int n_order,
                       const int64_t* fresh, const int64_t* song, const int64_t* beat0, int64_t n_songs,
                       int64_t* beat, void* stream);

/* Policy entropy and KL against a reference model (csrc/policy_stats.hip).  For row n of logits (rows x
 * ld f32) and attribute a: p = softmax of the raw logits, q the distribution cwlt_score_categorical(_grammar) scores
 * row n under -- tempered logits, the mask row of song key[n] (NULL: n) at bar count bar[n], the row grammar, the
 * nucleus kept set, renormalised, the kept set bitwise the sampler's.  Writes f32 nats to out[(n * n_attr + a) * 2]:
 * {H(p), H(q)}; with ref_logits (rows x ref_ld f32, a second model's logits for the same rows) to out[(n * n_attr + a)
 * * 4]: {H(p), H(q), KL(p || p'), KL(q || q')}, p' and q' the same constructions on ref_logits under the same mask,
 * grammar and settings.  KL(q || q') is +inf when a class of q's kept set is outside q''s (a nucleus only).
 * bar_class (DEVICE int64 x rows, nullable): the row's own bar-beat class; negative: a padding row, left unwritten.
 * Under a grammar it fixes the row's kind as the bar-beat target does in cwlt_score_categorical_grammar (attribute
 * bar_attr itself follows the position rule at beat[n]); without one only its sign is read.  A row whose allowed set
 * is empty (an ill-formed row under a grammar) gets NaN in the q columns and finite p columns.
 * bar / sched / masks: all of the constraint table or none of it; beat / order / gram: all of the grammar or none.
 * Refused: what cwlt_score_categorical_grammar refuses of these arguments, ref_ld < sum n_class with ref_logits, a
 * grammar without bar_class, rows > 2^20. */
int cwlt_policy_stats(const float* logits, const int* n_class, const float* temperature, const float* top_p,
                      int n_attr, int64_t rows, int64_t ld, const float* ref_logits, int64_t ref_ld,
                      const int64_t* bar_class, const int64_t* key, const int64_t* bar, const int64_t* sched,
                      int64_t n_sched, const uint32_t* masks, int64_t mask_rows, int mask_words, const int64_t* beat,
                      const int* order, int n_order, const uint32_t* gram, int gram_words, int bar_attr, float* out,
                      void* stream);

/* Blend of a policy with a reference model at sampling time (csrc/blend.hip).  For row n of logits (rows
 * x ld f32) and ref_logits (rows x ref_ld f32, a second model's logits for the same rows) and attribute a with columns
 * [off_a, off_a + n_class[a]): out[n, c] = w logits[n, c] + (1 - w) ref_logits[n, c] (out rows x ld_out f32), so that
 * softmax(out) is softmax(logits)^w softmax(ref_logits)^(1 - w) renormalised.  w = alpha[k * n_attr + a] (DEVICE f32,
 * n_alpha x n_attr): k = 0 when n_alpha == 1, else key[n] (DEVICE int64 x rows; NULL: n); a row with k outside [0,
 * n_alpha) -- an idle (-1) or waiting (-2) stream slot -- is copied from logits.  1 - w is formed once in f32, then two
 * products and a sum (an fma or not), with no special case: w = 1 returns logits and w = 0 ref_logits exactly for
 * finite inputs (a -0 may come back +0).  Columns at or past sum n_class are neither read nor written.  out may be
 * logits itself (ld_out == ld): each element is read, then written, by one thread; otherwise out overlaps neither
 * input.  16-byte accesses when the three bases are 16-byte aligned and the three strides multiples of 4, scalar ones
 * otherwise.  n_class is a HOST array.
 * Refused: a NULL logits, ref_logits, alpha, out or n_class, n_attr outside 1 .. 8, a class count outside 1 .. 256, a
 * stride below sum n_class, n_alpha < 1, rows < 1 or > 2^20, out == ref_logits. */
int cwlt_blend_logits(const float* logits, int64_t ld, const float* ref_logits, int64_t ref_ld, const int* n_class,
                      int n_attr, const float* alpha, int64_t n_alpha, const int64_t* key, float* out, int64_t ld_out,
                      int64_t rows, void* stream);

/* Soft preferences: a logit bias per class and bar and a repetition penalty (csrc/prefer.hip).
 * Tables, all DEVICE: sched (n_songs x 2 int64 {first bias row, rows}) with bias (bias_rows x ld_bias f32), both or
 * neither; pen (n_songs x (2 n_attr + 1) f32: frequency[n_attr], presence[n_attr], decay); seen (one f32 per class in
 * the sampler's column layout, row stride ld_seen).  n_class is a HOST array.  Every product and sum is rounded on its
 * own in f32 (no fused multiply-add): the results are bitwise those of the same formulas in numpy float32.
 *
 * cwlt_prefer_logits: out[n, c] = ((logits[n, c] + b) - f * s) - (s > 0 ? p : 0) for row n of song k = key[n] (DEVICE
 * int64 x rows; NULL: n).  b = bias[first + min(max(bar[n] - 1, 0), rows_k - 1), c] (bar DEVICE int64 x rows, NULL: the
 * first row), the masked sampler's row rule; a song with 0 rows, or no bias table, adds no b.  s = seen[n, c]; f, p =
 * pen[k, a], pen[k, n_attr + a] for the attribute a of c, taken as 0 for the attribute's class 0 and when seen is NULL
 * (then s is 0 too).  A row with k outside [0, n_songs) -- an idle (-1) or waiting (-2) stream slot -- is copied.
 * Layout and aliasing as cwlt_blend_logits: columns at or past sum n_class are neither read nor written, out may be
 * logits itself, 16-byte accesses when every base given is 16-byte aligned and every stride a multiple of 4.
 * Refused: a NULL logits, out or n_class, n_attr outside 1 .. 8, a class count outside 1 .. 256, a stride below sum
 * n_class, n_songs < 1, rows < 1 or > 2^20, bias without sched or the reverse, seen without pen, out == seen or bias.
 *
 * cwlt_prefer_track, after a draw: seen[n, c] = seen[n, c] * decay_k + (tokens[n, a] == c - off_a ? 1 : 0), k =
 * song[n] (NULL: n).  fresh, song (DEVICE int64 x rows) and seen0 (DEVICE f32, n_songs x sum n_class) are given together
 * or all NULL, as in cwlt_grammar_track: a row with fresh[n] != 0 and song[n] >= 0 takes seen0[song[n]] instead (its
 * token belongs to the song that just ended); a row with k outside [0, n_songs) is left alone.  rows <= 2^20.
 *
 * cwlt_prefer_scan, for given songs: tokens (nb * Lb) x n_attr int64, song i in rows [i Lb, (i + 1) Lb); writes
 * seen_rows (nb * Lb x ld f32), row t of a song the state after its rows 0 .. t from a zero state -- what the logits
 * of row t, which predict row t + 1, are penalised by.  The song's decay is that of k = key[i Lb] (DEVICE int64 x nb *
 * Lb, the per-row key of cwlt_prefer_logits; NULL: i); k outside [0, n_songs): decay 0.  One thread per (song, column)
 * walks the rows in order with the step of cwlt_prefer_track.  nb * Lb <= 2^20.
 *
 * cwlt_prefer_scan_packed: the same for n_block songs laid end to end, song i in rows [cu[i], cu[i + 1]) (cu: DEVICE
 * int32 x n_block + 1, as cwlt_causal_linear_fwd_state_packed; not read by the host); its decay is that of k =
 * key[cu[i]] (NULL: i).  The rows of a song are bitwise those of cwlt_prefer_scan.  n_block <= 2^20. */
int cwlt_prefer_logits(const float* logits, int64_t ld, const int* n_class, int n_attr, const int64_t* key,
                       const int64_t* bar, const int64_t* sched, int64_t n_songs, const float* bias,
                       int64_t bias_rows, int64_t ld_bias, const float* pen, const float* seen, int64_t ld_seen,
                       float* out, int64_t ld_out, int64_t rows, void* stream);
int cwlt_prefer_track(const int64_t* tokens, int64_t rows, const int* n_class, int n_attr, const float* pen,
                      int64_t n_songs, const int64_t* fresh, const int64_t* song, const float* seen0, float* seen,
                      int64_t ld_seen, void* stream);
int cwlt_prefer_scan(const int64_t* tokens, int64_t nb, int64_t Lb, const int* n_class, int n_attr, const float* pen,
                     int64_t n_songs, const int64_t* key, float* seen_rows, int64_t ld, void* stream);
int cwlt_prefer_scan_packed(const int64_t* tokens, const int* cu, int64_t n_block, const int* n_class, int n_attr,
                            const float* pen, int64_t n_songs, const int64_t* key, float* seen_rows, int64_t ld,
                            void* stream);

/* ---- continuous batching (csrc/stream.hip) ------------------------------------------------------------------------------
 * A pool of `slots` rows of cwlt_decode_step_rows runs many songs; per token the stream enqueues the decode step,
 * cwlt_stream_refill, cwlt_sample_categorical_keyed and cwlt_stream_advance.
 *
 * cwlt_stream_refill: for every slot s with fresh[s] != 0 (DEVICE int64, `slots` flags), copy the one-slot snapshot
 * into slot s of `state` and snap_logits (n_logits floats) into logits row s (row stride ld_logits).  state holds
 * n_layer blocks, each the S rows of all slots (slots x s_floats) then their Z rows (slots x z_floats); snap_state is
 * the same layout for one slot.  s_floats, z_floats multiples of 4, both state pointers 16-byte aligned.  Other slots'
 * bytes are not written.
 * cwlt_stream_advance (one workgroup): per slot, write (song[s], tokens[s, 0..n_attr), end bit) into row ctl[0] %
 * ring_rows of ring (ring_rows, slots, n_attr + 2) int64; for a slot with song[s] >= 0 advance pos[s] and bar[s] (+1 when
 * bar_mask[tokens[s, bar_attr]], an int array of bar_classes flags) and end the song when bar[s] reaches bar_cond or
 * pos[s] reaches cap.  Ended slots take the next song indices ctl[1], ctl[1] + 1, ... in slot order (song -1 once all
 * n_songs are assigned), get pos 0 and bar bar0, and are flagged fresh; every other slot's flag is cleared.
 * ctl (DEVICE int64 x 3) = {tokens advanced, songs assigned, songs finished}.  n_songs <= 2^20, bar0 < bar_cond. */
int cwlt_stream_refill(float* state, const float* snap_state, int n_layer, int64_t s_floats, int64_t z_floats,
                       float* logits, const float* snap_logits, int64_t n_logits, int64_t ld_logits,
                       const int64_t* fresh, int64_t slots, void* stream);
int cwlt_stream_advance(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr, const int* bar_mask,
                        int bar_classes, int64_t bar_cond, int64_t bar0, int64_t cap, int64_t n_songs, int64_t* song,
                        int64_t* pos, int64_t* bar, int64_t* fresh, int64_t* ctl, int64_t* ring, int64_t ring_rows,
                        void* stream);
/* Per-song prompts: every song starts from its own prefilled state, held in a device bank of `bank` entries (song k in
 * entry k % bank; the host prefills blocks of songs into it while the stream runs).
 * cwlt_stream_refill_bank: cwlt_stream_refill with the source of a fresh slot s the bank entry song[s] % bank (slots
 * with song[s] < 0 are skipped).  bank_state holds n_layer blocks, each the S rows of all entries (bank x s_floats)
 * then their Z rows (bank x z_floats); bank_logits (bank, >= n_logits) with row stride ld_bank_logits.
 * cwlt_stream_advance_bank: cwlt_stream_advance with these changes.  ctl (DEVICE int64 x 4) = {tokens advanced, songs
 * assigned, songs finished, songs ready}: the host raises ctl[3] (with a write enqueued after the prefill) once the
 * entries of songs below it are written.  A slot whose song ended, and a slot already WAITING, is a candidate; the
 * candidates are ranked in slot order and take the next song indices only while they are below min(ready, n_songs).
 * A candidate past that waits (song[s] = -2) while songs remain unassigned and goes idle (-1) once all are; a waiting
 * or idle slot writes song -1 into its ring row, its pos and bar do not move, and it is not counted as finished.  A slot
 * handed song k gets pos 0, bar bank_bar0[k % bank] and cap[s] = bank_cap[k % bank] (its own cap, kept per slot since
 * the entry is reused later) and is flagged fresh; every other slot's flag is cleared.  bar_cond >= 1. */
int cwlt_stream_refill_bank(float* state, const float* bank_state, int64_t bank, int n_layer, int64_t s_floats,
                            int64_t z_floats, float* logits, const float* bank_logits, int64_t n_logits,
                            int64_t ld_logits, int64_t ld_bank_logits, const int64_t* fresh, const int64_t* song,
                            int64_t slots, void* stream);
int cwlt_stream_advance_bank(const int64_t* tokens, int n_attr, int64_t slots, int bar_attr, const int* bar_mask,
                             int bar_classes, int64_t bar_cond, const int64_t* bank_bar0, const int64_t* bank_cap,
                             int64_t bank, int64_t n_songs, int64_t* song, int64_t* pos, int64_t* bar, int64_t* cap,
                             int64_t* fresh, int64_t* ctl, int64_t* ring, int64_t ring_rows, void* stream);

/* ---- particle generation: SMC resampling of lock-step songs (csrc/particles.hip) ---------------------------
 * K consecutive rows of a cwlt_decode_step_rows pool are the particles of one song.  Per token, after the draw of
 * cwlt_sample_categorical_logp / _grammar, cwlt_particle_weigh; every few tokens cwlt_particle_resample and, per family
 * of per-row buffers, cwlt_particle_gather twice (state -> scratch, scratch -> state).  One launch each, no host
 * synchronisation, no allocation.  Every pointer is DEVICE memory.
 *
 * cwlt_particle_weigh (one thread per row): for every row n with done[n] == 0,
 *     lw[n] += sum_a (logp[o, n, a, 0] - logp[o, n, a, 1]),  o = *out_counter % out_rows (NULL: 0, out_rows 1),
 * logp the (out_rows, rows, n_attr, 2) f32 ring of cwlt_sample_categorical_logp and out_counter the counter that draw was
 * given; the attributes' differences are added in order from 0.0f and the row's sum is then added to lw[n], each
 * difference and sum rounded on its own in f32.  Then len[n] += 1 and done[n] = 1 when bar[n] >= bar_cond (bar after
 * cwlt_count_bars) or len[n] >= cap[n], else 0: the row that ends a song counts.  A row with done[n] != 0 is not
 * touched.  lw f32, bar / cap / len / done int64, all x rows.  rows <= 2^20, n_attr 1 .. 8.
 *
 * cwlt_particle_resample (one workgroup per group of `particles` = K consecutive rows, 2 <= K <= 1024): with m = max lw,
 * e_i = expf(lw_i - m), s = sum e_i and ess = s^2 / sum e_i^2 of the group's rows, a group whose rows are all done, or
 * with ess >= ess_frac * K (compared in f32), keeps anc[i] = i (the row's own index in the whole pool) and its lw.  Any
 * other group is resampled systematically: anc[g K + j] = g K + the first i whose inclusive prefix sum of e exceeds
 * (j + u) / K * s, K - 1 when none does; log_z[g] += m + logf(s / K); every lw of the group becomes 0.  u in [0, 1) is
 * the counter-based generator's draw for (seed, event, g): it does not depend on `groups`.  Written for every group:
 * anc (groups * K int64), u and ess (groups f32), resampled (groups int32, 1 where the group was resampled).
 * done int64 x rows, log_z f32 x groups.  0 <= ess_frac <= 1, 0 <= event < 2^32, groups * K <= 2^20.
 *
 * cwlt_particle_gather: dst[b][n] = src[b][anc[n]] for blocks b < n_blocks and rows n < rows with anc[n] != n; row n of
 * block b lies at byte b * block_stride + n * row_bytes of dst and of src alike.  A row with anc[n] == n, or with anc[n]
 * outside [0, rows), is neither read nor written.  row_bytes (and block_stride when n_blocks > 1) multiples of 4, both
 * bases 4-byte aligned; 16-byte accesses when both bases, row_bytes and block_stride are multiples of 16, 8-byte ones
 * when of 8.  dst == src is refused: a permutation in place would read rows it has overwritten (a swap 0 <-> 1), so a
 * caller moves a state through a scratch buffer of the same layout in two calls, moved rows only: state -> scratch with
 * copy_back = 0, then scratch -> state with copy_back = 1, which copies dst[b][n] = src[b][n] for the same rows n (the
 * rows the first call wrote); the launch boundary between the two is the barrier.  rows <= 2^20, block_stride >= rows *
 * row_bytes when n_blocks > 1, copy_back 0 or 1. */
int cwlt_particle_weigh(const float* logp, const int64_t* out_counter, int64_t out_rows, int64_t rows, int n_attr,
                        const int64_t* bar, int64_t bar_cond, const int64_t* cap, float* lw, int64_t* len,
                        int64_t* done, void* stream);
int cwlt_particle_resample(float* lw, const int64_t* done, int64_t groups, int particles, float ess_frac,
                           uint64_t seed, int64_t event, int64_t* anc, float* u, float* ess, int* resampled,
                           float* log_z, void* stream);
int cwlt_particle_gather(void* dst, const void* src, const int64_t* anc, int64_t rows, int64_t row_bytes, int n_blocks,
                         int64_t block_stride, int copy_back, void* stream);

/* ---- particle generation on the stream (csrc/particles.hip, csrc/particles_stream.hip) -------------------
 * A pool of `groups` groups of `particles` = K consecutive rows; group g holds song song[g] (< 0: none), row g K + k its
 * particle k with id[row] = song K + k (-1: none).  pos[row] is the row's clock: tokens since its song started, ticked
 * for every row with a song, done or not.  One launch each, no host synchronisation, no allocation, no atomics.  Every
 * pointer is DEVICE memory; a null pointer or a size out of range is refused with CWLT_ERR_ARG before any launch.
 *
 * cwlt_particle_resample_keyed: cwlt_particle_resample with u drawn for (seed, event, song[g]) where event =
 * pos[g * pos_stride] / every - 1, the song's own event index, instead of (seed, event, g).  A group with song[g] < 0 or
 * event < 0 gets anc[i] = i, u = ess = 0, resampled = 0 and its lw and log_z are neither read nor written; a group whose
 * rows are all done is kept as in cwlt_particle_resample.  With song[g] = g and pos = (e + 1) * every every output is
 * bitwise cwlt_particle_resample's at event e.  song int64 x groups, pos int64, 1 <= pos_stride <= 2^20, every >= 1.
 *
 * cwlt_particle_advance (per token, after cwlt_particle_weigh; one workgroup): row ctl[0] % ring_rows of ring
 * (ring_rows, rows, n_attr + 2) int64 gets, per row, {id (-1 without a song), the n_attr tokens, done != 0 (0 without a
 * song)}; pos += 1 for rows with a song; every fresh flag becomes 0; ctl[0] += 1.  rows <= 2^20, n_attr 1 .. 8.
 *
 * cwlt_particle_release (per event, after the gather; one workgroup, groups <= 4096): a group is a candidate when
 * song[g] < 0 or all its K rows have done != 0.  A candidate with song[g] >= 0 is finished: out_logz[song] = log_z[g],
 * and out_lw[id] = lw, out_len[id] = len for its K rows; ctl[2] += the finished groups.  Candidate number r in group
 * order takes song ctl[1] + r while that is < n_songs: its rows get id = song K + k, pos 0, bar bar0, cap cap0, len 0,
 * done 0, lw 0, fresh 1 and log_z[g] = 0; the others get song -1, id -1, done 1.  ctl[1] = min(ctl[1] + candidates,
 * n_songs).  Nothing of a group that is no candidate is written.  out_lw f32 / out_len int64 x n_songs K, out_logz f32 x
 * n_songs; n_songs K <= 2^20, cap0 >= 1.
 *
 * cwlt_particle_fill: for rows with fresh != 0 and 0 <= id < n_src, row_bytes bytes of dst row n (rows ld_dst bytes
 * apart) = those of src row id (ld_src apart).  row_bytes, ld_dst, ld_src multiples of 4, bases 4-byte aligned, dst !=
 * src. */
int cwlt_particle_resample_keyed(float* lw, const int64_t* done, int64_t groups, int particles, float ess_frac,
                                 uint64_t seed, const int64_t* song, const int64_t* pos, int64_t pos_stride,
                                 int64_t every, int64_t* anc, float* u, float* ess, int* resampled, float* log_z,
                                 void* stream);
int cwlt_particle_advance(const int64_t* tokens, int n_attr, int64_t rows, const int64_t* id, const int64_t* done,
                          int64_t* pos, int64_t* fresh, int64_t* ctl, int64_t* ring, int64_t ring_rows, void* stream);
int cwlt_particle_release(int64_t groups, int particles, int64_t n_songs, int64_t bar0, int64_t cap0, int64_t* song,
                          int64_t* id, int64_t* pos, int64_t* bar, int64_t* cap, int64_t* len, int64_t* done,
                          int64_t* fresh, float* lw, float* log_z, int64_t* ctl, float* out_lw, int64_t* out_len,
                          float* out_logz, void* stream);
int cwlt_particle_fill(void* dst, const void* src, const int64_t* fresh, const int64_t* id, int64_t rows, int64_t n_src,
                       int64_t row_bytes, int64_t ld_dst, int64_t ld_src, void* stream);

/* ---- per-song prompts on the particle stream (csrc/particles_bank.hip) -----------------------------------
 * Every song starts from its own entry, song % bank, of cwlt_stream_refill_bank's bank, and the K particles of a song
 * share that one prefill.  One launch each, no host synchronisation, no allocation, no atomics.  Every pointer is
 * DEVICE memory; a null pointer or a size out of range is refused with CWLT_ERR_ARG before any launch.
 *
 * cwlt_particle_refill_bank (per token, in the place of cwlt_stream_refill): row n of the pool belongs to group
 * n / particles; a row with fresh[n] != 0 and id[n] >= 0 takes the state and the n_logits logits of bank entry
 * e = (id[n] / particles) % bank -- state, bank_state, bank_logits and logits laid out as for cwlt_stream_refill_bank with
 * `rows` slots.  Every other row is not written.  A workgroup that serves a group loads each float4 of the entry once
 * and stores it to every fresh row of the group that takes it.  rows <= 2^20 and a multiple of particles, particles
 * 2 .. 1024, bank >= 1, s_floats and z_floats multiples of 4, state and bank_state 16-byte aligned.
 *
 * cwlt_particle_release_bank (per hand-out boundary, in the place of cwlt_particle_release): ctl (DEVICE int64 x 4) =
 * {tokens advanced, songs assigned, songs finished, songs ready}.  With limit = min(ctl[3], n_songs), candidate number r
 * takes song ctl[1] + r only while that is < limit; a candidate past it is parked (song -1, id -1, done 1) and is a
 * candidate again at the next boundary.  A finished song's out_lw / out_len / out_logz are written whether or not its
 * group gets a new song.  ctl[1] = min(ctl[1] + candidates, max(limit, ctl[1])); ctl[2] += the finished groups.  A row
 * handed song v gets bar bar0_all[v] and cap cap_all[v], two tables of n_songs int64, in the place of bar0 and cap0.
 * With ctl[3] >= n_songs and constant tables every array comes out bitwise as cwlt_particle_release leaves it. */
int cwlt_particle_refill_bank(float* state, const float* bank_state, int64_t bank, int n_layer, int64_t s_floats,
                              int64_t z_floats, float* logits, const float* bank_logits, int64_t n_logits,
                              int64_t ld_logits, int64_t ld_bank_logits, const int64_t* fresh, const int64_t* id,
                              int64_t rows, int particles, void* stream);
int cwlt_particle_release_bank(int64_t groups, int particles, int64_t n_songs, const int64_t* bar0_all,
                               const int64_t* cap_all, int64_t* song, int64_t* id, int64_t* pos, int64_t* bar,
                               int64_t* cap, int64_t* len, int64_t* done, int64_t* fresh, float* lw, float* log_z,
                               int64_t* ctl, float* out_lw, int64_t* out_len, float* out_logz, void* stream);

/* ---- reward terms in the particles' weights (csrc/reward.hip) ----------------------------------------------
 * Each pool row keeps a ring of its particle's last `window` = W drawn rows, recent (rows, W, n_attr) int64, and of
 * whether the particle was alive when each was drawn, live (rows, W) int64.  Both are per-row state: a caller hands them
 * to cwlt_particle_gather with everything else, so a descendant inherits its ancestor's window.  One launch each, no host
 * synchronisation, no allocation, no atomics.  Every pointer is DEVICE memory.  rows 1 .. 2^20, n_attr 1 .. 8,
 * W 1 .. 2^16; anything else, and a null pointer, is refused with CWLT_ERR_ARG before any launch.
 *
 * cwlt_reward_push (per token, after the draw and BEFORE cwlt_particle_weigh): with s = *counter % W,
 *     recent[n, s, :] = tok[n, :],  live[n, s] = (done[n] == 0),
 * tok (rows, n_attr) int64 the token just drawn, done as the previous token's cwlt_particle_weigh left it (so the row
 * that ends a song is live), counter the loop's device int64 row counter.
 *
 * cwlt_reward_window (per reward event; the slots 0 .. filled - 1 of the ring hold the window's rows in time order,
 * 1 <= filled <= W): for slot j of row n, when j < filled and live[n, j] != 0, win[n, j, :] = recent[n, j, :] and
 * mask[n, j] = 1; elsewhere win[n, j, :] = 0 and mask[n, j] = 0.  any[n] = 1 when row n has such a slot, else 0, and
 * then mask[n, 0] = 1 (tokens 0): no consumer sees an empty window.  win (rows, W, n_attr), mask (rows, W), any (rows,)
 * int64.
 *
 * cwlt_reward_apply: for the rows with any[n] != 0, lw[n] = lw[n] + (beta * r[n]), the product rounded to f32 and then
 * the sum (no fma), and h_r[n] = r[n]; for the others lw[n] is not written and h_r[n] = 0 whatever r[n] holds (a
 * select: r[n] may be NaN).  r, lw, h_r f32 x rows.
 *
 * cwlt_reward_apply_keyed: cwlt_reward_apply with a reward weight per song.  Row n belongs to song
 * s = id / particles, id = key[n], or n when key is NULL (the lock-step pool, where the row index is the particle id;
 * the particle stream passes its id array).  A row is on when any[n] != 0, id >= 0 and s < n_beta: it gets
 * lw[n] = lw[n] + (beta[s] * r[n]), by the same two roundings, and h_r[n] = r[n].  Every other row keeps lw[n]
 * unwritten and gets h_r[n] = 0 by a select; beta is not read for it.  beta f32 x n_beta (n_beta >= 1), key int64 x rows
 * or NULL, particles >= 1. */
int cwlt_reward_push(const int64_t* tok, const int64_t* done, const int64_t* counter, int64_t rows, int n_attr,
                     int64_t window, int64_t* recent, int64_t* live, void* stream);
int cwlt_reward_window(const int64_t* recent, const int64_t* live, int64_t rows, int n_attr, int64_t window,
                       int64_t filled, int64_t* win, int64_t* mask, int64_t* any, void* stream);
int cwlt_reward_apply(const float* r, const int64_t* any, float beta, int64_t rows, float* lw, float* h_r,
                      void* stream);
int cwlt_reward_apply_keyed(const float* r, const int64_t* any, const float* beta, int64_t n_beta, const int64_t* key,
                            int particles, int64_t rows, float* lw, float* h_r, void* stream);

/* ---- song metrics and rule-based rewards (csrc/metrics.hip) ------------------------------------------------
 * cwlt_song_metrics: F = 11 measures per song from its token rows, bit for bit sampling.song_metrics_f32.  One launch,
 * no host synchronisation, no allocation, no cross-workgroup communication.  Every pointer is DEVICE memory.
 *
 * tok (N, L, n_attr) int64; mask (N, L) int64 or NULL (nonzero: live); lengths (N) int32 or NULL (rows at or past a
 * song's length are not live).  order (n_order), pitch (n_pitch), chord (n_chord) int32: the tables of the classes of
 * bar_attr, pitch_attr and chord_attr (chord_attr = -1: no chord feature, chord may be NULL).  order: -2 class 0,
 * -1 Bar, k >= 0 Beat_k (k < Q <= 64); pitch: a MIDI pitch 0..127, or -1; chord: -1 keep the current chord, else a 12-bit
 * mask of pitch classes (0: no chord).  xlog2x (n_table >= L + 1) f32: T[c] = float32(c log2 c), T[0] = T[1] = 0.
 *
 * A song is walked in row order from beat = -1, chord mask 0, slot 0.  A row that is not live is nothing.  A live row
 * whose class in one of the (two or three) attributes lies outside its table only counts as a live row.  Otherwise, with
 * o = order[class]: o == -1 opens the next bar slot and sets beat = -1; o >= 0 sets beat = o and, when chord[class] >= 0,
 * the chord mask; o == -2 with pitch[class] in 0..127 is a note at (slot, beat, chord mask); anything else is nothing.
 * Slot s >= 1 is the s-th Bar row's bar; slot 0 exists only if a live row precedes the first Bar row.  B is the number of
 * existing slots, `first` the lowest (0 or 1).  A note in slot s >= max_bars is dropped from every output, and the
 * per-slot measures run over the Bk existing slots below max_bars; bars[n] and n_bars report the true B.
 * Per slot: hist[12] note counts per pitch class (pitch % 12), groove: bit k set when a note sits at beat k (0 <= k < 64;
 * a note at beat -1 sets none), and the note count.
 *
 * ent(c) = (T[n] - (((0 + T[c_0]) + T[c_1]) + ... + T[c_11])) / (float)n with n = sum c, 0 for n = 0; every float
 * operation here and below is rounded to f32 on its own (no fma), in the order written.  feat (N, 11) f32:
 *   0 n_notes   1 n_bars = B
 *   2 h1: over the kept slots in order, for each slot with notes sum += ent(hist), count += 1; sum / count, 0 without
 *   3 h4: the same over every run of 4 consecutive kept slots (the run's histogram the integer sum; runs without notes
 *     skipped)       4 h_all: ent of the integer sum of all kept slots
 *   5 groove: P = Bk (Bk - 1) / 2, S = sum over kept i < j of popcount(g_i ^ g_j); 1 - (float)S / (float)(P Q), 0 for P = 0
 *   6 in_chord: of the notes under a chord mask != 0, the share whose pitch class is in the mask; 0 without such notes
 *   7 pitch_range: max - min pitch   8 distinct_pitches   9 notes_per_bar = n_notes / Bk   10 empty_bars = the share of
 *     kept slots without notes (both 0 for Bk = 0).
 * weights (11) f32 or NULL; reward (N) f32 or NULL: r = 0, then for f = 0..10 m = weights[f] * feat[f], r = r + m.
 * bars (N) int32, hist (N, max_bars, 12) int32, groove (N, max_bars) int64 (indexed by slot, zero outside the kept
 * slots), each or NULL.
 *
 * CWLT_ERR_ARG before any launch: a null tok / order / pitch / xlog2x / feat (chord with chord_attr >= 0), N < 1 or
 * > 2^24, L < 1 or >= 2^24, n_attr outside 1..8, an attribute index outside n_attr (chord_attr below -1), an empty
 * table, Q outside 1..64, max_bars outside 1..512, n_table < L + 1, reward without weights.
 * Songs of at most 128 rows with max_bars <= 64 take a wave each, four to a workgroup; the others 256 threads each. */
#define CWLT_SONG_METRICS 11
int cwlt_song_metrics(const int64_t* tok, const int64_t* mask, const int32_t* lengths, int64_t N, int64_t L, int n_attr,
                      int bar_attr, int pitch_attr, int chord_attr, const int32_t* order, int n_order,
                      const int32_t* pitch, int n_pitch, const int32_t* chord, int n_chord, int Q, const float* xlog2x,
                      int64_t n_table, int max_bars, float* feat, const float* weights, float* reward, int32_t* bars,
                      int32_t* hist, int64_t* groove, void* stream);

/* ---- the dense projections at few token rows, and a whole encoder layer per host call ---------------------------------
 * The reference's own RL setting is 30 windows x 50 tokens = 1 500 token rows per network pass
 * (dqn_policy/IRL_dqn_train.py:267-345 `DQN.update`, ppo_policy/ppo_train.py:365-417 `update_policy`): ~970 launches of
 * ~10 us per update, bound by the HOST when every launch is its own Python-level call.
 *
 * cwlt_gemm_bf16_small: cwlt_gemm_bf16's product on 64 x 64 output tiles (192-768 workgroups at 1 500 rows where 256-row
 * tiles leave 12), operands straight from L2 into MFMA fragments.  N % 8 == 0, K % 32 == 0, row strides multiples of 8,
 * 16-byte aligned pointers; same arithmetic (f32 accumulation, bias in f32, one rounding).
 * cwlt_transpose_bf16_many: dst_i (cols, rows) = src_i (rows, cols)^T for the n dense bf16 matrices of `table` (DEVICE
 * memory, n x 4 int64: element offset from src, element offset from dst, rows, cols) in one launch -- the transposed
 * weight copies the input-gradient products read. */
int cwlt_gemm_bf16_small(const void* a, const void* w, const float* bias, void* c, int64_t M, int N, int K, int64_t lda,
                         int64_t ldw, int64_t ldc, int accumulate, void* stream);
int cwlt_transpose_bf16_many(const void* src, void* dst, const int64_t* table, int n, void* stream);
/* dst_i = bf16(src_i) for the n arrays of `table` (DEVICE memory, n x 3 int64: element offset from src (f32), element
 * offset from dst (bf16), element count) in one launch: the bf16 copies of an encoder's master weights, refreshed once per
 * forward (torch's multi-tensor copy takes four launches and half the bandwidth for the same 84 tensors). */
int cwlt_cast_bf16_many(const float* src, void* dst, const int64_t* table, int n, void* stream);
/* cwlt_gemm_nt_bias_gelu_dropout on the split-K small tiles, for passes of a few hundred rows at most (a 50-token rollout
 * step): g = dropout_p(gelu(bf16(a . w^T) + bias)), and gd = mask / (1 - p) * gelu'(.) when gd != NULL -- what
 * cwlt_gemm_bf16_small followed by cwlt_bias_gelu_dropout_fwd produce, bit for bit (same rounding of the product, same
 * dropout stream keyed by (seed, row * N + column)).  g, gd dense (M, N); K % 128 == 0, N % 8 == 0. */
int cwlt_gemm_bf16_small_gelu(const void* a, const void* w, const float* bias, void* g, void* gd, int64_t M, int N, int K,
                              int64_t lda, int64_t ldw, float p, uint64_t seed, const uint64_t* seed_base, void* stream);

/* One post-LN encoder layer -- fast_transformers' TransformerEncoderLayer(AttentionLayer(CausalLinearAttention)) as
 * built at dqn_policy/model.py:128-137 (ppo_policy/model.py:129-138) and called at :232:
 *     x1 = norm1(x + dropout(out_projection(causal_linear_attention(q, k, v))));
 *     y  = norm2(x1 + dropout(linear2(dropout(gelu(linear1(x1))))))
 * -- enqueued by ONE host call forward (8 launches) and one backward (13-21 launches: 13 with the four weight gradients as one grouped launch), through the entry points above
 * (same kernels, same dropout streams as the per-op path).  bf16 activations; d_model 512, 8 heads of 64, d_ff % 256 == 0.
 * The struct is HOST memory, read during the call only; every pointer in it is a device pointer.
 * forward : reads x and the parameters; writes y and `saved`; uses `scratch` (fwd_scratch_bytes).
 * backward: reads dy, x, `saved` (of the matching forward, same n_seq/len/p_drop/seeds/want_backward = 1), the
 *           TRANSPOSED weight copies and gamma1/gamma2; writes dx and `grads`; uses `scratch` (bwd_scratch_bytes).
 * All buffers 256-byte aligned.  grads (f32, grad_floats): the 12 parameter gradients at grad_off[] (float offsets),
 * in the order CWLT_LAYER_GRAD_* below; the Q / K / V weight (bias) gradients are the three row blocks of wqkv (bqkv). */
#define CWLT_LAYER_NGRADS 12
#define CWLT_LAYER_NSAVED 13
enum { CWLT_LAYER_GRAD_WQKV = 0, CWLT_LAYER_GRAD_BQKV, CWLT_LAYER_GRAD_WO, CWLT_LAYER_GRAD_BO, CWLT_LAYER_GRAD_W1,
       CWLT_LAYER_GRAD_B1, CWLT_LAYER_GRAD_W2, CWLT_LAYER_GRAD_B2, CWLT_LAYER_GRAD_GAMMA1, CWLT_LAYER_GRAD_BETA1,
       CWLT_LAYER_GRAD_GAMMA2, CWLT_LAYER_GRAD_BETA2 };
typedef struct cwlt_encoder_layer {
    int64_t n_seq, len;                /* N sequences x L tokens: R = N L token rows */
    int32_t d_model, d_ff, n_heads;
    int32_t want_backward;             /* forward: also leave the scan's final state for a one-sweep backward */
    float p_drop, ln_eps, attn_eps;    /* dropout probability (0 in eval mode); 1e-5, 1e-6 in the reference */
    int32_t reserved;
    uint64_t seed[3];                  /* dropout streams: residual block 1, FFN, residual block 2 */
    const uint64_t* seed_base;         /* optional device uint64 added to every seed (hipGraph replays), or NULL */
    const void *wqkv, *wo, *w1, *w2;   /* bf16 (3D, D) query|key|value rows stacked, (D, D), (F, D), (D, F) as stored */
    const float *bqkv, *bo, *b1, *b2, *gamma1, *beta1, *gamma2, *beta2;     /* f32 */
    const void *wqkv_t, *wo_t, *w1_t, *w2_t;   /* backward: bf16 transposed copies (D, 3D), (D, D), (D, F), (F, D) */
    const void* x;                     /* (R, D) bf16 layer input */
    void* y;                           /* (R, D) bf16 layer output (forward) */
    void* saved;                       /* saved_bytes: activations kept for the backward */
    void* scratch;
    const void* dy;                    /* (R, D) bf16 gradient of y (backward) */
    void* dx;                          /* (R, D) bf16 gradient of x (backward) */
    float* grads;                      /* grad_floats f32 (backward) */
} cwlt_encoder_layer;
typedef struct cwlt_encoder_layer_plan_t {
    int64_t saved_bytes, fwd_scratch_bytes, bwd_scratch_bytes, grad_floats;
    int64_t grad_off[CWLT_LAYER_NGRADS];
    int64_t saved_off[CWLT_LAYER_NSAVED];  /* byte offsets inside `saved` (tests): qkv, attention out, zinv, final state,
                                            * s1, x1, mean1, rstd1, gd, g, s2, mean2, rstd2 */
} cwlt_encoder_layer_plan_t;
int cwlt_encoder_layer_plan(int64_t n_seq, int64_t len, int d_model, int d_ff, int n_heads, float p_drop,
                            int want_backward, cwlt_encoder_layer_plan_t* plan);
int cwlt_encoder_layer_fwd(const cwlt_encoder_layer* layer, void* stream);
int cwlt_encoder_layer_bwd(const cwlt_encoder_layer* layer, void* stream);
/* The whole stack -- fast_transformers' TransformerEncoder.forward loop over its layers (dqn_policy/model.py:232) -- in one
 * host call: `layers` is a HOST array of n structs wired by the caller (layer i's y is layer i + 1's x; in the backward
 * layer i's dx is layer i - 1's dy); forward runs them in order, backward in reverse. */
int cwlt_encoder_fwd(const cwlt_encoder_layer* layers, int n, void* stream);
int cwlt_encoder_bwd(const cwlt_encoder_layer* layers, int n, void* stream);

/* ---- hipGraph hygiene (no counterpart in the reference, which has no graphs; used by the drop-in RL loops' replayed
 * steps) -------------------------------------------------------------------------------------------
 * Replace every MEMSET node of a captured, not yet instantiated hipGraph_t by a kernel node writing the same bytes (same
 * dependencies, same dependents): on ROCm 7.2 a captured hipMemsetAsync replays a wrong fill pattern from the second
 * replay on, and library code inside a captured step (PyTorch's reduction semaphores, hipBLASLt's split-K workspaces)
 * issues such memsets.  *replaced (may be NULL): nodes replaced.  Child graphs are not entered.  0 or a hipError_t. */
int cwlt_graph_replace_memset_nodes(void* graph, int* replaced);

#ifdef __cplusplus
}
#endif
#endif /* CWLT_H */

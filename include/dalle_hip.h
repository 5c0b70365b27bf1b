/* dalle_hip.h -- C ABI of libdalle_hip.so: the drop-in boundary for the DALL-E train-step hot path
 * on MI355X (gfx950).  SURVEY.md §8(b): the reference (EleutherAI/DALLE-mtf) has NO FFI boundary;
 * its arithmetic lives in mesh_tensorflow / tensorflow ops.  Each entry point below replaces one
 * implicit third-party op of SURVEY.md §2.2 (K-rows) at the reference call site cited.
 *
 * Conventions (all entry points):
 *   - raw DEVICE pointers + explicit sizes; the caller (PyTorch host code) owns every buffer incl.
 *     workspace; nothing is allocated, freed or synchronised inside; everything is enqueued on the
 *     hipStream_t passed last (as void*), so calls are stream-ordered and re-entrant.
 *   - return 0 on success, negative dmi_status otherwise; dmi_last_error_string() is thread-local.
 *   - "bf16" = raw uint16 bfloat16 bits.  Matrices are row-major with explicit leading dimensions.
 *   - weights keep the reference layout [in, out]; the fwd GEMM consumes the
 *     [out, in] bf16 copy produced by dmi_transpose_bf16 / dmi_adam_step.
 */
#ifndef DALLE_HIP_H
#define DALLE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DMI_OK = 0,
  DMI_ERR_INVALID = -1,   /* bad size / alignment / null pointer */
  DMI_ERR_LAUNCH = -2,    /* hipGetLastError() after a launch */
  DMI_ERR_UNSUPPORTED = -3
} dmi_status;

const char* dmi_last_error_string(void);
int dmi_version(void);
/* Test hooks (every setting computes the same results): "nt4" 0/1/2 = never / auto / always use the 256x128 NT tile,
 * "nt8" / "tn8" 0/1/2 = the 256x256 8-wave NT / weight-gradient tiles, "tn_tail" 0/1 = row-split the ragged last residency of
 * unsplit weight gradients, "nt8_min_k" = smallest K at which the auto mode picks the 256x256 NT tile, "skinny" 0/1 = products with M <= 32 rows (the decode step) on the weight-streaming kernel,
 * "attn_xcd" = schedule of the persistent attention blocks (0: one serpentine over all blocks,
 * != 0: per-XCD item lists when the (batch, head) count divides by 8), "attn_mask_force" 0/1 = a causal mask plan runs the masked
 * attention kernels too.  Unknown name -> -1. */
int dmi_get_option(const char* name);
int dmi_set_option(const char* name, int value);
/* Diagnostics (tools/phases.py): u64 device buffer [blocks][5 or 8] that the 256x128 NT kernel and the weight-gradient
 * kernel fill with per-block phase cycle stamps; NULL (default) disables the stamps. */
int dmi_set_debug_buffer(void* device_buffer);

/* ---- K1  embedding: mtf.gather(wte, tokens) + wpe[0..S)   src/dalle_mtf/models.py:186-219 ---- */
/* pos_dev (optional, device int32): every row takes wpe[*pos_dev] (clamped to [0, S)) instead of wpe[row % S] -- the incremental
 * decode step, whose position must not be a by-value argument of a replayed HIP graph. */
int dmi_embed_fwd(const int32_t* tokens, const uint16_t* wte, const uint16_t* wpe, uint16_t* x,
                  int64_t rows /*B*S*/, int S, int d, int vocab, const int* pos_dev, void* stream);
/* stable sort of the n token ids (clamped to [0, vocab)): sorted_tokens ascending, perm[i] = source position of sorted
 * position i.  Index plumbing for dmi_embed_bwd; one-block radix sort, deterministic.
 * workspace: dmi_sort_tokens_workspace_bytes(n). */
int64_t dmi_sort_tokens_workspace_bytes(int64_t n);
int dmi_sort_tokens(const int32_t* tokens, int32_t* sorted_tokens, int32_t* perm, int64_t n, int vocab,
                    void* workspace, void* stream);
/* backward: dwpe[s] = sum_b dx[b,s];  dwte[tok] = sum of dx over the positions holding tok (gradient of mtf.gather =
 * scatter-add), written for every id incl. zeros for absent ones.  Positions are visited in
 * token-id order (dmi_sort_tokens) so equal ids reduce in registers; deterministic, no atomics.
 * workspace: dmi_embed_bwd_workspace_bytes(B, S, d). */
int64_t dmi_embed_bwd_workspace_bytes(int B, int S, int d);
int dmi_embed_bwd(const int32_t* sorted_tokens, const int32_t* perm, const uint16_t* dx, float* dwte,
                  float* dwpe, int B, int S, int d, int vocab, void* workspace, void* stream);

/* ---- Dropout (reference embed_dropout / residual_dropout, src/dalle_mtf/models.py:198-200, 215-217, 312-314, 322-323) ----
 * A dropout SITE is a 64-bit key and a 16-bit threshold thresh in [0, 65535] (= round(rate * 65536), clamped).  Element e of the
 * site's tensor (row-major, e = row * d + col), with g = e >> 2 and j = e & 3, draws r = (splitmix64(key + g) >> 16 j) & 0xffff and
 * is kept iff r >= thresh; drop(v) = kept ? v * scale : +0 with scale = fp32(65536.0 / (65536 - thresh)), the product rounded to
 * fp32 on its own.  thresh 0 keeps everything with scale 1.  The mask is a pure function of (key, e): it is never stored, and the
 * forward, its re-run under recompute_grad and the backward restate it from the key.  All four entry points: stream-ordered, no
 * allocation, DMI_ERR_INVALID with a message before any launch for a null pointer, d % 8 != 0, an empty shape or a thresh
 * outside [0, 65535]; the two dmi_dropout_* also for a buffer that is not 16-byte aligned.
 *
 * dmi_embed_fwd_dropout: x[b,s,:] = bf16(drop_tok(wte[tok]) + drop_pos(wpe[s])); the token mask's element index is
 * (b S + s) d + c, the positional mask's is s d + c (shared over the batch: the reference drops pos_emb as a [seq, embd] tensor).
 * dmi_embed_bwd_dropout: dwte[tok] = sum over the positions holding tok of drop_tok(dx), dwpe[s] = drop_pos(sum_b dx[b,s]);
 * order, workspace and determinism of dmi_embed_bwd. */
int dmi_embed_fwd_dropout(const int32_t* tokens, const uint16_t* wte, const uint16_t* wpe, uint16_t* x, int64_t rows /*B*S*/, int S,
                          int d, int vocab, uint64_t key_tok, uint64_t key_pos, int thresh, void* stream);
int dmi_embed_bwd_dropout(const int32_t* sorted_tokens, const int32_t* perm, const uint16_t* dx, float* dwte, float* dwpe, int B, int S,
                          int d, int vocab, void* workspace, uint64_t key_tok, uint64_t key_pos, int thresh, void* stream);
/* dmi_dropout_add_ln: x_out[m, c] = bf16(float(residual) + drop(float(a))) (one fp32 product, one fp32 sum, one rounding), then
 * y, mean, rstd = what dmi_layernorm_fwd computes from the stored x_out, bit for bit, in the same pass (the row stays in
 * registers; d <= 4096).  gamma == NULL: x_out only -- beta, y, mean, rstd are not touched (a LayerNorm launched elsewhere).
 * dmi_dropout_bwd: dy[m, c] = bf16(drop(float(dx))), the gradient of a dropped branch output; nothing past M * d is touched. */
int dmi_dropout_add_ln(const uint16_t* a, const uint16_t* residual, uint16_t* x_out, const uint16_t* gamma, const uint16_t* beta,
                       uint16_t* y, float* mean, float* rstd, int64_t M, int d, uint64_t key, int thresh, float eps, void* stream);
int dmi_dropout_bwd(const uint16_t* dx, uint16_t* dy, int64_t M, int d, uint64_t key, int thresh, void* stream);

/* ---- Rotary position embeddings (project extension, config key "rotary_emb"; DESIGN.md §4 "Rotary") ----
 * cs = fp32 [S, head_dim / 2, 2]: interleaved (cos, sin) of pair c at sequence position s (dalle_mtf.rotary.rotary_table), shared by
 * every layer, head and batch row.  Pair c of a head is its adjacent elements (2c, 2c + 1); in fp32
 *   y0 = x0 cos - x1 sin,   y1 = x0 sin + x1 cos,   each rounded once to bf16.
 * dmi_rope_qk: rotates, in place, columns [0, 2 H head_dim) (q and k) of every row of a [rows, ld] bf16 buffer in the qkv layout
 * (row = [q | k | v] x [H, head_dim], ld >= 2 H head_dim, ld % 8 == 0); the v columns are neither read nor written.  Row r takes
 * table row r % S; row offsets are 64-bit.  inverse != 0 uses -sin: the transpose of the rotation, i.e. the gradient with respect to
 * the unrotated q, k from the gradient with respect to the rotated ones.
 * dmi_rope_qk_decode: the same rotation of the decode step's [B, 3 H head_dim] staging buffer, every row at table row pos.
 * pos_dev != NULL: the position is read from device memory (one int32; `pos` is then ignored and a position outside [0, S) makes
 * the launch a no-op -- the dmi_attention_decode contract, so one captured graph serves every position).
 * Both: stream-ordered, no allocation.  head_dim other than 64 / 128: DMI_ERR_UNSUPPORTED; a null pointer, an empty shape, a buffer
 * that is not 16-byte aligned, or a by-value pos outside [0, S): DMI_ERR_INVALID -- with a message, before any launch. */
int dmi_rope_qk(uint16_t* qkv, int ld, const float* cs, int64_t rows, int S, int H, int head_dim, int inverse, void* stream);
int dmi_rope_qk_decode(uint16_t* fresh, const float* cs, int B, int S, int H, int head_dim, int pos, const int* pos_dev,
                       void* stream);

/* ---- QK normalisation (project extension, config key "qk_norm"; DESIGN.md §4 "QK norm") ----
 * Every head's query and key vector is RMS-normalised over its head_dim channels, with learned gains gq, gk (bf16 [head_dim], shared
 * by the heads, passed as the LayerNorm gains are) and the constant c = head_dim^(-1/2) for q, 1 for k.  In fp32, eps = 1e-6:
 *   r(x) = rsqrt(mean_j(x_j^2) + eps),   y = x r(x) g c.
 * dmi_qk_norm_fwd: in place on columns [0, 2 H head_dim) of every row of a [rows, ld] bf16 buffer in the qkv layout (ld >= 2 H head_dim,
 * ld % 8 == 0); the v columns are neither read nor written; row offsets are 64-bit.  pre (nullable): the unnormalised q | k of every
 * row are also written there, packed bf16 [rows, 2 H head_dim] -- what the backward reads.  cs (nullable): the table of dmi_rope_qk;
 * the rotation of table row r % S is applied to the fp32 y in the same pass and the result rounded once to bf16 (cs == NULL: S is
 * only checked).  An all-zero head gives zeros.
 * dmi_qk_norm_bwd: in place on the q | k columns of dqkv, the gradient with respect to the forward's output.  With cs it is first
 * rotated back (the transpose, as dmi_rope_qk(inverse = 1)).  With xh = x r(x) recomputed from pre, u = g c and a = u dy:
 *   dx = r (a - xh mean_j(a_j xh_j)),    dg_j = c sum_{rows, heads} dy_j xh_j.
 * dgq, dgk: fp32 [head_dim], written (not accumulated).  The sums are formed in float64 from float64 terms: per-block partial rows in
 * `workspace` (dmi_qk_norm_bwd_workspace_bytes(rows, head_dim), a pure host function), then one fixed-order reduce rounded once to
 * fp32 -- the same inputs give the same bits.
 * dmi_qk_norm_decode: the forward for the decode step's [B, 3 H head_dim] staging buffer.  cs, pos and pos_dev as dmi_rope_qk_decode:
 * every row at table row pos; pos_dev != NULL reads the position from device memory and a position outside [0, S) makes the launch a
 * no-op.  cs == NULL: no rotation and the position is not used.  Bit-equal to the matching rows of dmi_qk_norm_fwd.
 * All: stream-ordered, no allocation, no atomics.  head_dim other than 64 / 128: DMI_ERR_UNSUPPORTED; a null pointer (other than the
 * nullable ones), an empty shape, a buffer that is not 16-byte aligned, ld < 2 H head_dim or ld % 8 != 0, or (with cs) a by-value pos
 * outside [0, S): DMI_ERR_INVALID -- with a message, before any launch. */
int dmi_qk_norm_fwd(uint16_t* qkv, int ld, uint16_t* pre, const uint16_t* gq, const uint16_t* gk, const float* cs, int64_t rows,
                    int S, int H, int head_dim, void* stream);
int64_t dmi_qk_norm_bwd_workspace_bytes(int64_t rows, int head_dim);
int dmi_qk_norm_bwd(uint16_t* dqkv, int ld, const uint16_t* pre, const uint16_t* gq, const uint16_t* gk, const float* cs,
                    float* dgq, float* dgk, void* workspace, int64_t rows, int S, int H, int head_dim, void* stream);
int dmi_qk_norm_decode(uint16_t* fresh, const uint16_t* gq, const uint16_t* gk, const float* cs, int B, int S, int H, int head_dim,
                       int pos, const int* pos_dev, void* stream);

/* ---- Token shift (project extension, config key "token_shift"; DESIGN.md §4 "Token shift") ----
 * A sequence has S = T + G * G positions: p < T is a caption position, p >= T is image token k = p - T of the G x G grid at row
 * r = k / G, column c = k % G.  y = shift(x) over rows of d bf16 channels, d % 32 == 0:
 *   channels       caption position p < T            image position p >= T
 *   [0, d/4)       x[p - 1] if p >= 1 else 0         from above:    x[p - G] if r >= 1 else 0
 *   [d/4, d/2)     x[p - 1] if p >= 1 else 0         from the left: x[p - 1] if c >= 1 else 0
 *   [d/2, d)       x[p]                              x[p]
 * Every read is from an earlier position of the same sequence; values are copied bit for bit, zeros are +0.  The transpose
 * (dx from dy) is again a gather:
 *   [0, d/4)       dy[q + 1] if q + 1 < T else 0     dy[q + G] if r + 1 < G else 0
 *   [d/4, d/2)     dy[q + 1] if q + 1 < T else 0     dy[q + 1] if c + 1 < G else 0
 *   [d/2, d)       dy[q]                             dy[q]
 * dmi_token_shift: out of place over dense [rows, d] buffers, rows a multiple of S (row r is position r % S of sequence r / S);
 * row offsets are 64-bit.  inverse != 0: the transpose.  hist != NULL (forward only): columns [0, d/2) of every input row are also
 * copied to hist[rows, d/2] -- the history the decode step reads.
 * dmi_token_shift_decode: the row of position pos of B sequences.  y[b] = the shift of x[b] ([B, d] each) with the neighbours'
 * halves read from rows pos - 1 and pos - G of hist[B, S, d/2]; then hist[b, pos] <- x[b, :d/2].  pos_dev != NULL: the position is
 * read from device memory (one int32; `pos` is then ignored and a position outside [0, S) makes the launch a no-op -- the
 * dmi_attention_decode contract, so one captured graph serves every position).
 * Both: stream-ordered, no allocation.  A null x, y (decode: hist), an empty shape, S != T + G * G, T < 1 or G < 1, rows % S != 0,
 * d % 32 != 0, a buffer that is not 16-byte aligned, x and y overlapping, hist together with inverse, or a by-value pos outside
 * [0, S): DMI_ERR_INVALID -- with a message, before any launch. */
int dmi_token_shift(const uint16_t* x, uint16_t* y, uint16_t* hist, int64_t rows, int S, int T, int G, int d, int inverse,
                    void* stream);
int dmi_token_shift_decode(const uint16_t* x, uint16_t* hist, uint16_t* y, int B, int S, int T, int G, int d, int pos,
                           const int* pos_dev, void* stream);

/* ---- K2  LayerNorm eps=1e-5 biased variance  models.py:373-389, layers.py:30-33 ---- */
int dmi_layernorm_fwd(const uint16_t* x, const uint16_t* g, const uint16_t* b, uint16_t* y,
                      float* mean, float* rstd, int64_t rows, int d, float eps, void* stream);
/* dx_out = LNbwd(dy) (+ dres if non-null); dg/db fp32 [d] written (not accumulated).
 * workspace: dmi_layernorm_bwd_workspace_bytes(rows, d). */
int64_t dmi_layernorm_bwd_workspace_bytes(int64_t rows, int d);
int dmi_layernorm_bwd(const uint16_t* dy, const uint16_t* x, const uint16_t* g, const float* mean,
                      const float* rstd, const uint16_t* dres, uint16_t* dx, float* dg, float* db,
                      void* workspace, int64_t rows, int d, void* stream);
/* dg == db == NULL defers the reduce of the gain / bias gradients: the per-block partials stay in `workspace` (which the caller
 * then must not reuse) until dmi_layernorm_bwd_finish_batch reduces up to 16 LayerNorms of the same width in one launch (same
 * summation order: bit-identical to the immediate form).  Host arrays of n device pointers / row counts. */
int dmi_layernorm_bwd_finish_batch(const void* const* workspaces, float* const* dgs, float* const* dbs, const int64_t* rows,
                                   int n, int d, void* stream);

/* ---- K3/K5/K6/K7  dense layers: mtf einsum / mtf.layers.dense   models.py:242-244,303-311,320-321,369,393
 * C[M,N] = A[M,K] . Bt[N,K]^T  (both operands K-contiguous), bf16 in, fp32 accumulate on MFMA.
 * flags: DMI_GEMM_*;  bias bf16 [N];  residual bf16 [M,ldc] added;  relu_src bf16 [M,ldc]: C *= (relu_src>0);
 * rowscale fp32 [M]: C[m,:] *= rowscale[m].  K % 64 == 0, N % 8 == 0.  Output bf16 (or fp32 with DMI_GEMM_OUT_F32).
 * GELU: C = bf16(gelu(acc + bias)), the tanh form of mtf.gelu (see dmi_gemm_nt_gelu).
 * Supported flag sets: 0, BIAS, BIAS|RELU, BIAS|GELU, BIAS|RESIDUAL, RESIDUAL, RELU_MASK, ROWSCALE, OUT_F32. */
#define DMI_GEMM_BIAS 1
#define DMI_GEMM_RELU 2
#define DMI_GEMM_RESIDUAL 4
#define DMI_GEMM_RELU_MASK 8
#define DMI_GEMM_OUT_F32 16
#define DMI_GEMM_ROWSCALE 32
#define DMI_GEMM_GELU 512
int dmi_gemm_nt(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, void* C, int ldc,
                int M, int N, int K, int flags, const uint16_t* bias, const uint16_t* residual,
                const uint16_t* relu_src, const float* rowscale, void* stream);
/* LayerNorm (eps, biased variance: K2) fused into the product, for the incremental decode step only (M <= 32 rows, N % 16 == 0,
 * K = the normalised width <= 2048; anything else -> DMI_ERR_UNSUPPORTED): C = LN(X; gamma, beta) . Bt^T (+ bias bf16 [N])(ReLU / GELU).
 * flags: 0, BIAS, BIAS|RELU, BIAS|GELU.  LN(X) is rounded to bf16 before the product, as dmi_layernorm_fwd + dmi_gemm_nt would. */
int dmi_ln_gemm_nt(const uint16_t* X, int ldx, const uint16_t* gamma, const uint16_t* beta, float eps, const uint16_t* Bt, int ldb,
                   uint16_t* C, int ldc, int M, int N, int K, int flags, const uint16_t* bias, void* stream);
/* same product with the K range split over nsplit block groups (fp32 slabs in workspace, deterministic reduction to
 * bf16 C with ldc == N, optionally times rowscale[m]): for long-K GEMMs whose tile count does not fill whole
 * residencies (the head's input gradient: K = vocabulary). */
int64_t dmi_gemm_nt_splitk_workspace_bytes(int M, int N, int nsplit);
int dmi_gemm_nt_splitk(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, uint16_t* C, int M, int N, int K,
                       int nsplit, const float* rowscale, void* workspace, void* stream);
/* weight gradient: dW[I,J] (fp32, ld = J) = sum_m X[m,I] * dY[m,J]; deterministic split over m.
 * dbias (nullable): fp32 [J] = sum_m w[m] * dY[m, :] fused into the same pass (bias gradient of the dense layer), with
 * w = 1, or w = bias_weights (nullable bf16 [M], 4-byte aligned, M even: DMI_ERR_INVALID otherwise) for the fused-softmax head
 * where dY holds unnormalised dlogits.
 * workspace: dmi_gemm_tn_workspace_bytes(M, I, J).
 * Run-to-run bit-identical for every shape.  Unsplit gradients with at least as many 256-column stripes as the chip has gangs
 * of ceil(I / 128) block slots (the vocabulary projection's gradient) run as a gang stream-K on 128 x 256 tiles: a column
 * stripe is cut at most once over m and its two pieces are added onto zeroed elements with fp32 atomics -- a two-addend sum
 * has no order (option "tn_wide" = 0 keeps those shapes on the 128 x 128 tiles). */
int64_t dmi_gemm_tn_workspace_bytes(int M, int I, int J);
/* deferred (nullable, room for 2 items) + n_deferred: when the gradient is split over m, its final slab reduces (dW, dbias)
 * are not launched but described here; the caller runs the reduces of several GEMMs in ONE launch with
 * dmi_reduce_slabs_batch (<= 16 items) -- each deferring GEMM then needs its own workspace, untouched until that call.
 * out[i] = sum_{s < nsplit} slabs[s * 4 n4 + i], i < 4 n4, fixed order: bit-identical to the undeferred call. */
typedef struct dmi_reduce_item { const float* slabs; float* out; int nsplit; int64_t n4; } dmi_reduce_item;
int dmi_gemm_tn(const uint16_t* X, int ldx, const uint16_t* dY, int ldy, float* dW, float* dbias,
                const uint16_t* bias_weights, int M, int I, int J, void* workspace, dmi_reduce_item* deferred,
                int* n_deferred, void* stream);
int dmi_reduce_slabs_batch(const dmi_reduce_item* items, int n, void* stream);
/* Up to 4 weight gradients that contract over the same M rows in ONE launch (the gradients of a block's out-projection and QKV
 * kernels, src/dalle_mtf/models.py:242-244,303-311 under mtf.gradients, src/optimizers.py:34: 16 + 48 tiles fill the chip together,
 * neither does alone).  Per problem: dW[I,J] = X^T dY (+ dbias / bias_weights as dmi_gemm_tn) with its own workspace of
 * dmi_gemm_tn_workspace_bytes(M, I, J) bytes.  The slab reduces (<= 2 per problem) go to `deferred` / *n_deferred, or run here
 * when deferred == NULL.  The row-split plan is the group's, so sums are ordered differently from n single dmi_gemm_tn calls
 * (fp32, deterministic). */
typedef struct dmi_tn_problem { const uint16_t* X; int ldx; const uint16_t* dY; int ldy; float* dW; float* dbias;
                                const uint16_t* bias_weights; int I; int J; void* workspace; } dmi_tn_problem;
int dmi_gemm_tn_group(const dmi_tn_problem* probs, int n, int M, dmi_reduce_item* deferred, int* n_deferred, void* stream);
/* The group's plan for n problems of shapes I[k] x J[k] over M rows: the row-split count (>= 2) when the launch runs on 128 x 256
 * tiles -- the union of those tiles fills the block slots with a split count every problem's own workspace has slabs for: all four
 * gradients of an n_embd = 512 block, 96 tiles x 5 splits --, 0 when it stays on 128 x 128 tiles.  Callers group MORE problems per
 * launch where this is non-zero (the engine: a block's two FFN gradients join the attention pair). */
int dmi_gemm_tn_group_plan(const int* I, const int* J, int n, int M);

/* column sum (bias gradients): out[N] fp32 = sum_m Y[m, 0..N) ; workspace dmi_colsum_workspace_bytes */
int64_t dmi_colsum_workspace_bytes(int64_t M, int N);
int dmi_colsum(const uint16_t* Y, int ldy, float* out, int64_t M, int N, void* workspace, void* stream);
/* batched bf16 transpose: in [batch, R, C] -> out [batch, C, R] */
int dmi_transpose_bf16(const uint16_t* in, uint16_t* out, int batch, int R, int C, void* stream);

/* ---- K4  causal attention, UNSCALED logits, fp32 softmax   models.py:221-227,292-299 (Appendix A.2/A.3)
 * qkv [B*S, 3*H*128] bf16 = the QKV projection output, row = [q | k | v] x [H, 128] (heads-major, A.1);
 * o [B*S, H*128] bf16;  lse [B,H,S] fp32.  These three calls take head dim 128 (README.md:164); the _hd forms below take
 * head dim 64 or 128; S % 8 == 0.
 * Every transposed MFMA operand is a hardware transpose read of the natural tile: no transposed copies. */
int dmi_attention_fwd(const uint16_t* qkv, uint16_t* o, float* lse, int B, int H, int S, void* stream);
/* backward.  d_o [B*S, H*128] bf16; scratch: 3*B*H*S floats (delta | interleaved (lse, delta) pairs);
 * dqkv [B*S, 3*H*128] bf16 in the qkv layout (what the QKV dgrad/wgrad GEMMs consume). */
int dmi_attention_bwd(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, float* scratch,
                      uint16_t* dqkv, int B, int H, int S, void* stream);

/* Incremental decode (the reference's unfinished is_incremental_inference path, src/dalle_mtf/models.py:246-254,281-285):
 * one query position `pos` against the key/value cache.  qkv = the forward pass's projection buffer [B*S, 3*H*128] used as the
 * cache; row b*S + pos must already hold q | k | v of the new position (the caller's QKV GEMM writes it in place with row
 * pitch S*3d).  o[b, h*128 ..] = softmax(q . K[0..pos]^T) V[0..pos], bf16 [B, H*128].  Unscaled logits, keys <= pos only.
 * Graph-replayable form: fresh != NULL = a [B, 3*H*128] staging buffer at a fixed address holding the step's q | k | v (the
 * QKV GEMM writes it instead of the cache row); the kernel copies it into cache row pos and attends.  pos_dev != NULL = the
 * position is read from device memory (one int32; `pos` is then ignored and a position outside [0, S) makes the launch a
 * no-op), so ONE captured HIP graph serves every step of the sampling loop. */
int dmi_attention_decode(uint16_t* qkv, const uint16_t* fresh, uint16_t* o, int B, int H, int S, int pos, const int* pos_dev,
                         void* stream);
/* The same three operations for head_dim = 64 or 128 (any other value: DMI_ERR_UNSUPPORTED): every 128 above becomes head_dim
 * (qkv [B*S, 3*H*head_dim], o / d_o [B*S, H*head_dim]; lse, scratch and the decode contract unchanged).  head_dim = 128 is the
 * call above; head_dim = 64 runs kernels of its own and needs (S + 64) * 3 * H * 64 * 2 < 2^31 (32-bit buffer offsets). */
int dmi_attention_fwd_hd(const uint16_t* qkv, uint16_t* o, float* lse, int B, int H, int S, int head_dim, void* stream);
int dmi_attention_bwd_hd(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, float* scratch,
                         uint16_t* dqkv, int B, int H, int S, int head_dim, void* stream);
int dmi_attention_decode_hd(uint16_t* qkv, const uint16_t* fresh, uint16_t* o, int B, int H, int S, int pos, const int* pos_dev,
                            int head_dim, void* stream);

/* Custom attention masks (the reference's DALLE(attn_mask=...), models.py:221-227,292-299; DESIGN.md §4 "Attention masks").
 * dmi_attn_mask_plan (host only, no GPU): mask = uint8 [S, S] row-major, nonzero = query i may attend to key j.  It must be causal
 * and every row must allow a key (otherwise DMI_ERR_INVALID with a message).  Returns the plan's size in bytes (> 0); fills `plan`
 * (int32 words) when plan != NULL and plan_bytes >= that size.  Copy the filled plan to the device unchanged.
 * dmi_attention_*_masked: the calls above under the mask; `plan` = the device copy, `plan_host` = the host copy (its header is read to
 * route the call).  A causal plan runs the causal kernels above (unless the test option "attn_mask_force" is 1); any other plan runs
 * block-sparse head-dim-128 kernels (head_dim 64: DMI_ERR_UNSUPPORTED).  A plan built for another S is refused.  Decode reads the mask
 * row of the position (pos_dev on the graph-replayable path). */
int64_t dmi_attn_mask_plan(const uint8_t* mask, int S, int32_t* plan, int64_t plan_bytes);
int dmi_attention_fwd_masked(const uint16_t* qkv, uint16_t* o, float* lse, const int32_t* plan, const int32_t* plan_host, int B, int H,
                             int S, int head_dim, void* stream);
int dmi_attention_bwd_masked(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, float* scratch,
                             uint16_t* dqkv, const int32_t* plan, const int32_t* plan_host, int B, int H, int S, int head_dim,
                             void* stream);
int dmi_attention_decode_masked(uint16_t* qkv, const uint16_t* fresh, uint16_t* o, const int32_t* plan, const int32_t* plan_host,
                                int B, int H, int S, int pos, const int* pos_dev, int head_dim, void* stream);

/* ---- FP8 key/value cache for generation ("kv8", project extension; DESIGN.md §4 "Generation: FP8 key/value cache") ----
 * Per layer two buffers: data uint8 [B, S, 2, H, head_dim] (K then V, OCP E4M3FN bytes) and scale fp32 [B, S, 2, H].  For one head's
 * row x of head_dim bf16 values:  amax = max |x_j|,  e = clamp(floor(log2(amax)) - 7, -119, 120) (e = 0 when amax = 0),
 * scale = 2^e,  data_j = e4m3fn(x_j 2^-e) rounded to nearest even -- the byte torch.float8_e4m3fn gives for that fp32 value.  The
 * product is exact in fp32 and below 256 (nothing saturates); data_j 2^e is exact in fp32 and in bf16.
 * dmi_kv8_quantize: rows s0 <= s < s1 of every sequence of a bf16 [B*S, ld] buffer in the qkv layout (its k | v columns, ld >= 3 H
 * head_dim, ld % 8 == 0) go into data / scale; other rows are not touched; offsets are 64-bit.
 * dmi_attention_decode_kv8: the graph-replayable contract of dmi_attention_decode over that cache.  fresh (required: the cache holds
 * no queries) = the step's [B, 3 H head_dim] staging row; the kernel takes q from it, quantises the head's fresh k and v, stores them
 * into cache row pos and attends over the DEQUANTISED keys and values 0 .. pos -- row pos included, so the result does not depend
 * on what the cache row held before.  pos_dev != NULL: the position is read from device memory (`pos` is then ignored and a position
 * outside [0, S) makes the launch a no-op).  o bf16 [B, H head_dim].  Roundings as dmi_attention_decode (fp32 scores, P rounded to
 * bf16 before P V, the row sum over the unrounded P), waves merged in a fixed order: the same inputs give the same bits.
 * dmi_attention_decode_kv8_masked: row pos of a mask plan (plan / plan_host as dmi_attention_decode_masked: a causal plan runs the
 * call above, any other plan needs head_dim 128).
 * All: stream-ordered, no allocation, no atomics.  head_dim other than 64 / 128: DMI_ERR_UNSUPPORTED; a null pointer, an empty
 * shape, data / qkv / fresh not 16-byte aligned, a bad ld, s0 / s1 outside 0 <= s0 < s1 <= S, or a by-value pos outside [0, S):
 * DMI_ERR_INVALID -- with a message, before any launch. */
int dmi_kv8_quantize(const uint16_t* qkv, int ld, uint8_t* data, float* scale, int B, int S, int H, int head_dim, int s0, int s1,
                     void* stream);
int dmi_attention_decode_kv8(uint8_t* data, float* scale, const uint16_t* fresh, uint16_t* o, int B, int H, int S, int pos,
                             const int* pos_dev, int head_dim, void* stream);
int dmi_attention_decode_kv8_masked(uint8_t* data, float* scale, const uint16_t* fresh, uint16_t* o, const int32_t* plan,
                                    const int32_t* plan_host, int B, int H, int S, int pos, const int* pos_dev, int head_dim,
                                    void* stream);

/* ---- K7/K8  to_logits + cross entropy, labels = shift(tokens)   models.py:391-395,348-359,407-410
 * labels[t] = tokens[t+1], last = eos (bit-exact int path). */
int dmi_shift_labels(const int32_t* tokens, int32_t* labels, int B, int S, int eos, void* stream);
/* (a) evaluation / logits-returning path: cross entropy over materialised bf16 logits z [M, ldz] (ldz >= V, pad columns
 * must hold a large negative value).  loss_rows[M] fp32 = lse - z[label]; if dz_scale != 0: z is overwritten IN PLACE by
 * dz = (softmax(z) - onehot(label)) * dz_scale. */
int dmi_cross_entropy(uint16_t* z, int ldz, const int32_t* labels, float* loss_rows, float* lse,
                      int64_t M, int V, float dz_scale, void* stream);
/* (b) training path: the softmax is fused into the vocabulary projection and its row normaliser is deferred, so the
 * logits never make a round trip through HBM:
 *   dmi_label_logit      zl[m] = X[m,:] . Wt[label[m],:] + bias[label[m]] (fp32): the loss needs it; clears flag[0].
 *   dmi_gemm_nt_softmax  E[m,n] = bf16(exp(X[m,:] . Wt[n,:] + bias[n] - rowshift[m])) (rowshift nullable = no shift) and
 *                        rowsum_part[n/64][m] = fp32 sum of those exponentials over the 64-column group
 *                        (dmi_gemm_nt_softmax_partials(N) groups; pad columns need bias << 0 so that they contribute 0).
 *   dmi_softmax_finish   S[m] = sum of the partials; loss_rows[m] = log S[m] + rowshift[m] - label_logit[m] (= logsumexp - label logit);
 *                        rowscale[m] = dz_scale / S[m] (+ its bf16 copy); E[m,label] -= S[m], so dlogits = rowscale[m] * E[m,:];
 *                        Xs[M,K] = bf16(rowscale[m] * X[m,:]).  Consumers: dX = dmi_gemm_nt(E, W, DMI_GEMM_ROWSCALE),
 *                        dW = dmi_gemm_tn(Xs, E, bias_weights = rowscale_bf16).  With dz_scale == 0 only loss_rows is written.
 *                        Rows whose sum overflowed or vanished (a logit beyond +-87 of the shift) are redone exactly with the
 *                        row maximum as the shift (needs X, Wt, bias again); flag[0] != 0 afterwards tells that it happened. */
int dmi_label_logit(const uint16_t* X, int ldx, const uint16_t* Wt, int ldw, const uint16_t* bias,
                    const int32_t* labels, float* zl, int32_t* flag, int64_t M, int K, int V, void* stream);
int64_t dmi_gemm_nt_softmax_partials(int N);
/* Product + bias + residual with the LayerNorm of the result fused into the epilogue (reference src/dalle_mtf/models.py:303-314
 * feeding :333,373-389 -- out-projection + residual -> norm_2; :321-324 feeding the next block's :330 / to_logits' :392 -- FFN-2 +
 * residual -> norm_1 / final norm):  C[M, N] = bf16(A . Bt^T + bias + residual)  (bias, residual nullable),
 * Y[M, N] = bf16((C - mean) * rstd * gamma + beta), mean / rstd fp32 [M] over the ROUNDED row (biased variance, eps inside the
 * rsqrt: what dmi_layernorm_fwd computes from the stored C).  N = 512 only (a block owns whole rows): DMI_ERR_UNSUPPORTED otherwise.
 * K % 32 == 0 (the full-row kernel's k-step; dmi_gemm_nt_lnbwd the same). */
int dmi_gemm_nt_ln(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, uint16_t* C, int ldc, int M, int N, int K,
                   const uint16_t* bias, const uint16_t* residual, const uint16_t* gamma, const uint16_t* beta, float eps,
                   uint16_t* Y, int ldy, float* mean, float* rstd, void* stream);
/* The FFN's ReLU mask as one bit per element (reference src/dalle_mtf/models.py:320-321: h = mtf.relu(dense(x)), and its backward
 * dh = (dx . W2^T) * (h > 0)):  dmi_gemm_nt_relu_bits: C = bf16(relu(A . Bt^T + bias)) and bits = (C > 0), one bit per output;
 * dmi_gemm_nt_mask_bits: C = bf16(A . Bt^T) * bit -- what dmi_gemm_nt(DMI_GEMM_RELU_MASK, relu_src = h) computes, bit for bit,
 * from M*N/8 bytes instead of the 2*M*N bytes of h.  `bits` is an opaque buffer of dmi_relu_bits_bytes(M, N) bytes (8-byte
 * aligned; the layout is private to the two calls).  N % 64 == 0, K % 128 == 0, operands below 2 GiB: DMI_ERR_UNSUPPORTED
 * otherwise.  dmi_relu_bits_auto: 1 where the library's own dispatch would run these shapes on the kernel that has the bit
 * forms (callers keep dmi_gemm_nt elsewhere). */
int64_t dmi_relu_bits_bytes(int M, int N);
int dmi_relu_bits_auto(int M, int N, int K);
int dmi_gemm_nt_relu_bits(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, uint16_t* C, int ldc, int M, int N, int K,
                          const uint16_t* bias, void* bits, void* stream);
int dmi_gemm_nt_mask_bits(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, uint16_t* C, int ldc, int M, int N, int K,
                          const void* bits, void* stream);
/* The FFN's GELU (the DALLE activation_fn "gelu"; reference src/dalle_mtf/models.py:317-324 with mtf.gelu, the tanh form
 * gelu(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) = x * sigmoid(2u), evaluated in fp32):
 *   dmi_gemm_nt_gelu:      a = A . Bt^T + bias (fp32);  C = bf16(gelu(a)),  pre[M, ldpre] = bf16(a)   (the backward's input: GELU
 *                          cannot be inverted from C);
 *   dmi_gemm_nt_gelu_grad: C = bf16((A . Bt^T) * gelu'(pre)), gelu' in fp32 from the bf16 pre.
 * Same shapes as dmi_gemm_nt; pre 16-byte aligned, ldpre % 8 == 0, ldpre >= N. */
int dmi_gemm_nt_gelu(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, uint16_t* C, int ldc, int M, int N, int K,
                     const uint16_t* bias, uint16_t* pre, int ldpre, void* stream);
int dmi_gemm_nt_gelu_grad(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, uint16_t* C, int ldc, int M, int N, int K,
                          const uint16_t* pre, int ldpre, void* stream);
/* The gated FFN (project extension, config key "ff_glu"; DESIGN.md §4 "Gated feed-forward"): FFN-1 is dmi_gemm_nt(BIAS) at N = 2 Hh
 * into pre = [value | gate] (columns [0, Hh) and [Hh, 2 Hh) of a row), then
 *   dmi_glu_fwd:  h[m, j] = bf16(val * act(gate)),  val = pre[m, j], gate = pre[m, Hh + j], read as bf16, computed in fp32;
 *   dmi_glu_bwd:  dpre[m, j] = bf16(dh * act(gate)),  dpre[m, Hh + j] = bf16(dh * val * act'(gate)),  dh = dh[m, j].
 * act = DMI_GEMM_RELU (relu'(0) = 0, the h > 0 convention of DMI_GEMM_RELU_MASK) or DMI_GEMM_GELU (the tanh form and its derivative
 * as dmi_gemm_nt_gelu / _gelu_grad evaluate them).  Streaming kernels over 16-byte pieces with 64-bit addresses: M > 0, Hh % 8 == 0,
 * every pointer 16-byte aligned, every leading dimension a multiple of 8 and at least the row (Hh for h and dh, 2 Hh for pre and
 * dpre); nothing outside those rows and columns is touched.  DMI_ERR_INVALID, naming the argument, otherwise -- and no launch. */
int dmi_glu_fwd(const uint16_t* pre, int ldpre, uint16_t* h, int ldh, int64_t M, int Hh, int act, void* stream);
int dmi_glu_bwd(const uint16_t* dh, int lddh, const uint16_t* pre, int ldpre, uint16_t* dpre, int lddpre, int64_t M, int Hh, int act,
                void* stream);
/* An input-gradient product whose result arrives at a LayerNorm, with that LayerNorm's BACKWARD fused into the epilogue (reference:
 * the backward of src/dalle_mtf/layers.py:30-33 + models.py:387-388 behind models.py:330 / :333 -- norm_1 <- QKV, norm_2 <- FFN-1):
 *   dy = bf16(A . Bt^T) [M, N];  xh = (x - mean) * rstd;  dx[M, N] = bf16(rstd * (dy*gamma - mean_n(dy*gamma) - xh * mean_n(dy*gamma*xh)) + dres)
 * (dres nullable), i.e. what dmi_gemm_nt followed by dmi_layernorm_bwd computes, without writing / re-reading dy; the gain / bias
 * gradients leave as dmi_gemm_nt_lnbwd_parts(M) partial rows [2 N] fp32 in `part` (dgamma | dbeta), summed by
 * dmi_layernorm_bwd_finish_parts (fixed order).  N = 512 only (a block owns whole rows): DMI_ERR_UNSUPPORTED otherwise.  x, dres, dx have
 * row pitch N.  Differs from the two-kernel form only in the summation order of the reductions.
 * B2 / C2 (nullable, both or neither): the product that consumes dx chained in the same launch, C2[M, N] = bf16(dx . B2^T) with
 * B2 [N, ldb2] (K-contiguous) -- norm_2's dx is the gradient of the attention branch's output, and its next consumer is the
 * out-projection's input gradient d_o = dx . Wo^T (the backward of src/dalle_mtf/models.py:303-311): a block owns whole rows of
 * dx, i.e. the whole contraction range of its rows, so it reads them back from L2 as the A operand of a second main loop.
 * Bit-identical to dmi_gemm_nt on the stored dx. */
int dmi_gemm_nt_lnbwd_parts(int M);
/* dmi_gemm_nt_ln_auto: 1 where dmi_gemm_nt_ln / dmi_gemm_nt_lnbwd accept a K-contiguous [M, K] x [N, K]^T product (N = 512, operands
 * inside the kernel's 32-bit offsets) and no CUs are reserved for a concurrent exchange; callers gate the fused forms on it when they
 * size their buffers and keep dmi_gemm_nt + dmi_layernorm_fwd / _bwd elsewhere (same role as dmi_relu_bits_auto). */
int dmi_gemm_nt_ln_auto(int M, int N, int K);
int dmi_gemm_nt_lnbwd(const uint16_t* A, int lda, const uint16_t* Bt, int ldb, int M, int N, int K, const uint16_t* x,
                      const uint16_t* gamma, const float* mean, const float* rstd, const uint16_t* dres, uint16_t* dx,
                      float* part, const uint16_t* B2, int ldb2, uint16_t* C2, void* stream);
int dmi_layernorm_bwd_finish_parts(const float* part, int P, float* dg, float* db, int d, void* stream);
int dmi_gemm_nt_softmax(const uint16_t* X, int ldx, const uint16_t* Wt, int ldw, const uint16_t* bias,
                        const float* rowshift, uint16_t* E, int lde, float* rowsum_part, int M, int N, int K, void* stream);
int dmi_softmax_finish(const float* rowsum_part, int nparts, const float* label_logit, const float* rowshift,
                       const int32_t* labels, const uint16_t* X, int ldx,
                       const uint16_t* Wt, int ldw, const uint16_t* bias, uint16_t* E, int lde, int N,
                       float* loss_rows, float* rowscale, uint16_t* rowscale_bf16, uint16_t* Xs, int32_t* flag,
                       int64_t M, int K, int V, float dz_scale, void* stream);
/* out[0] = scale * sum(x[0..n))  deterministic single-block reduce (loss mean; grad-norm finish) */
int dmi_sum_f32(const float* x, int64_t n, float scale, float* out, void* stream);
/* Text/image loss weights (a project extension: the reference's loss is the plain mean over all positions,
 * src/dalle_mtf/models.py:348-359; position p predicts token p + 1, models.py:407-410).  Every row m carries the static weight
 * w = pos_weight[m % period] (fp32 [period], period = the sequence length):
 *   dmi_softmax_finish_w  dmi_softmax_finish with rowscale[m] = (dz_scale * w) / S[m] (fp32, the product first); rowscale_bf16 and Xs
 *                         derive from that rowscale, in the exact redo of flagged rows too.  loss_rows (the reference's unweighted
 *                         loss_batch), the label patch E[m,label] -= S[m] and the flag logic are those of dmi_softmax_finish, bit for
 *                         bit: the weight reaches both gradient products through rowscale alone.  w == 0 gives rowscale,
 *                         rowscale_bf16 and the Xs row exactly 0.  pos_weight non-null, period > 0; otherwise as dmi_softmax_finish.
 *   dmi_loss_reduce       out3[0] = scale * sum_m pos_weight[m % period] * loss_rows[m] (the weighted loss);
 *                         out3[1] = plain mean of loss_rows over rows with m % period < split (the text positions),
 *                         out3[2] = plain mean over the other rows (the image positions); a mean over no rows is 0.
 *                         Deterministic single-block reduce (fixed order, no atomics), in place of dmi_sum_f32 when weights are set.
 *                         M > 0, period > 0, 0 <= split <= period. */
int dmi_softmax_finish_w(const float* rowsum_part, int nparts, const float* label_logit, const float* rowshift,
                         const int32_t* labels, const uint16_t* X, int ldx,
                         const uint16_t* Wt, int ldw, const uint16_t* bias, uint16_t* E, int lde, int N,
                         float* loss_rows, float* rowscale, uint16_t* rowscale_bf16, uint16_t* Xs, int32_t* flag,
                         int64_t M, int K, int V, float dz_scale, const float* pos_weight, int period, void* stream);
int dmi_loss_reduce(const float* loss_rows, int64_t M, const float* pos_weight, int period, int split, float scale,
                    float* out3, void* stream);
/* Padded caption positions (config key "loss_ignore_padding", a project extension): the weight of a row depends on its label.
 * Row m is a text row when m % period < split (period = the sequence length, split = T - 1) and an image row otherwise; a text row
 * whose label is pad_id is ignored (keep = 0), image rows are always kept.  n_t = the kept text rows, n_i = the image rows.
 *   dmi_loss_mask           counts int32 [2] = (n_t, n_i), exact; row_w fp32 [M] = the weight of every row:
 *                             plain != 0:  keep / (n_t + n_i)
 *                             plain == 0:  keep * ct / max(n_t, 1) on text rows, ci / n_i on image rows
 *                           with ct = wt / (wt + wi), ci = wi / (wt + wi) computed by the host in float64: the numerator in fp32,
 *                           one correctly rounded division by the count converted to float, ignored rows exactly 0.  One launch,
 *                           one block, integer counts (no float atomics): two runs give equal bits.  0 < M < 2^31, period > 0,
 *                           0 <= split <= period.  The gradient path is dmi_softmax_finish_w with pos_weight = row_w, period = M.
 *   dmi_loss_reduce_masked  out4[0] = scale * sum_m row_w[m] * loss_rows[m]  (the masked loss),
 *                           out4[1] = L_t = sum of loss_rows over the kept text rows / max(n_t, 1),
 *                           out4[2] = L_i = mean of loss_rows over the image rows,
 *                           out4[3] = n_t / the number of text rows;  a mean over no rows is 0.
 *                           counts = dmi_loss_mask's, read on the device.  dmi_loss_reduce's single-block tree (fixed order, no
 *                           atomics).  Sizes as dmi_loss_mask. */
int dmi_loss_mask(const int32_t* labels, int64_t M, int period, int split, int pad_id, float ct, float ci, int plain,
                  int32_t* counts, float* row_w, void* stream);
int dmi_loss_reduce_masked(const float* loss_rows, const float* row_w, const int32_t* labels, int64_t M, int period, int split,
                           int pad_id, const int32_t* counts, float scale, float* out4, void* stream);

/* ---- K10  image-token indexing   src/model_fns.py:76-77,118-119 (bit-exact)
 * tokens_out[b, 0:T] = text[b]; tokens_out[b, T + p] = argmax_c logits[b, p, c] (first max) + text_vocab */
int dmi_assemble_tokens(const int32_t* text, const float* vae_logits, int32_t* tokens_out,
                        int B, int T, int P, int C, int text_vocab, void* stream);

/* Sampling of the next image token from head logits (the sampler around the reference's unfinished incremental-inference path,
 * src/dalle_mtf/models.py:246-254,281-285; src/model_fns.py:135-136 raises).  ONE draw, three instances of one kernel body
 * (csrc/elementwise.hip, draw_tokens<NUCLEUS, GUIDED>): dmi_sample_tokens is the plain instance, described here with everything
 * the three share; dmi_sample_tokens_p adds the nucleus filter and logp, dmi_sample_tokens_guided adds the guided logit in front of
 * that -- each states below only what it adds.  The shared checks carry the entry point's own name in front of their message.
 * Per row b of z bf16 [B, ldz] (first nv columns;
 * bias bf16 [nv] optional, added in fp32): v = (z + bias) / temperature; top_k > 0 keeps v >= the k-th largest v (ties kept); the choice is a
 * categorical draw from softmax(v) over the kept entries (Gumbel-max with counter-based noise hash(seed, position, b, i):
 * reproducible, stateless); temperature <= 0: first maximum.  nv <= 8192.
 * next_tok[b] = token_offset + choice (optional: where the next decode step reads its token);
 * out[b, position - out_col0] = choice when that column lies in [0, out_ld) (optional).
 * params_dev (optional, device uint32[4] = {bits of float 1/temperature (0: greedy), top_k, seed low, seed high}) and pos_dev
 * (optional, device int32) override the by-value arguments: decode step + sampling replay as one HIP graph.  advance != 0
 * (needs pos_dev = device int32[2], [1] a zero-initialised scratch counter): the last block to finish stores position + 1. */
int dmi_sample_tokens(const uint16_t* z, int ldz, const uint16_t* bias, int B, int nv, float temperature, int top_k,
                      uint64_t seed, const uint32_t* params_dev, int pos, int32_t* pos_dev, int advance, int token_offset,
                      int32_t* next_tok, int32_t* out, int out_ld, int out_col0, void* stream);

/* The NUCLEUS instance: dmi_sample_tokens's arguments plus top_p and logp.  v and the top-k filter as above; then q = softmax(v) over the top-k survivors, in fixed point: u[i] = floor(exp(v[i] - max v) * 2^31),
 * the mass of a set is the 64-bit integer sum of its u, Z the mass of all survivors, target = ceil(double(top_p) * double(Z)).
 * Nucleus: the shortest prefix of the survivors sorted by q (descending) whose mass reaches top_p; tau = the u of its last entry;
 * EVERY survivor with u >= tau is kept (ties at tau kept, the top-k rule).  Found without a sort: a 32-step bitwise search for the
 * largest tau with mass(u >= tau) >= target.  The draw is Gumbel-max over the kept set with dmi_sample_tokens's noise
 * hash(seed, position, b, i).  top_p = 1: no nucleus step, the tokens equal dmi_sample_tokens's bit for bit.  temperature <= 0:
 * first maximum (top_k and top_p ignored).  0 < top_p <= 1, else DMI_ERR_INVALID (NaN included).
 * logp (nullable, device fp32 [B], zeroed by the caller): logp[b] += (z + bias)[c] - logsumexp_i (z + bias)[i], c the choice --
 * the log-probability of the drawn token at temperature 1, unfiltered, over the nv columns; one call per position accumulates a
 * sample's score.
 * params_dev (optional, device uint32[6] = {bits of 1/temperature (0: greedy), top_k, seed low, seed high, bits of top_p, 0})
 * overrides temperature / top_k / seed / top_p (a device top_p outside (0, 1) skips the nucleus step); pos_dev / advance /
 * next_tok / out as for dmi_sample_tokens.  One 256-thread block per row, nv <= 8192, 64 KB of LDS per block (the plain instance:
 * 32 KB). */
int dmi_sample_tokens_p(const uint16_t* z, int ldz, const uint16_t* bias, int B, int nv, float temperature, int top_k,
                        uint64_t seed, float top_p, const uint32_t* params_dev, int pos, int32_t* pos_dev, int advance,
                        int token_offset, int32_t* next_tok, int32_t* out, int out_ld, int out_col0, float* logp, void* stream);

/* The GUIDED instance, classifier-free guidance: the nucleus draw from l_uncond + scale * (l_cond - l_uncond).  z bf16 [2 * Bc, ldz]: rows 0 .. Bc-1 are
 * the conditional rows, rows Bc .. 2 Bc - 1 the unconditional ones, pair b = rows b and Bc + b; one 256-thread block per pair
 * (grid Bc).  Per column i < nv, in fp32:  zc = z[b, i] + bias[i];  zu = z[Bc + b, i] + bias[i];  d = zc - zu;
 * g = zc + (scale - 1) * d, the difference, the product and the sum each rounded on their own (no fused multiply-add), so that
 * numpy float32 restates g bit for bit; scale - 1 == 0 takes g = zc itself.  v = g * (1/temperature), and from v on the draw is
 * dmi_sample_tokens_p's, the same statements: top-k with ties kept, the fixed-point nucleus, Gumbel-max with the noise hash(seed, position, b, i) (b the
 * pair index), first maximum of g when temperature <= 0.  scale = 1 gives dmi_sample_tokens_p's tokens on the conditional rows bit
 * for bit; scale = 0 draws from the unconditional rows.
 * next_tok[b] = next_tok[Bc + b] = token_offset + choice (both halves of the KV cache are fed the same token; int32 [2 * Bc]);
 * out[b, position - out_col0] = choice, out int32 [Bc, out_ld];  logp (nullable, fp32 [Bc]): logp[b] += log softmax(zc)[choice] --
 * the CONDITIONAL model's own score at temperature 1, unfiltered, so that samples drawn at different scales rank on one measure.
 * params_dev (optional, device uint32[6]): dmi_sample_tokens_p's block with word 5 = bits of scale (the unguided kernels ignore
 * word 5; a device scale is taken as it is).  By value: 0 < top_p <= 1 and scale finite and >= 0, else DMI_ERR_INVALID (NaN
 * included); Bc > 0; nv <= 8192.  pos_dev / advance as for dmi_sample_tokens: the last of the Bc blocks stores position + 1.
 * 64 KB of LDS per block, as the nucleus kernel. */
int dmi_sample_tokens_guided(const uint16_t* z, int ldz, const uint16_t* bias, int Bc, int nv, float temperature, int top_k,
                             uint64_t seed, float top_p, float scale, const uint32_t* params_dev, int pos, int32_t* pos_dev,
                             int advance, int token_offset, int32_t* next_tok, int32_t* out, int out_ld, int out_col0, float* logp,
                             void* stream);

/* "Go to full precision for the logits" (src/dalle_mtf/models.py:394-395) for a slice of the head's output:
 * out[b, i] = float(z[b, i]) + float(bias[i]), z bf16 [B, ldz] (first nv columns), bias bf16 [nv] (nullable), out fp32 [B, nv]. */
int dmi_logits_f32(const uint16_t* z, int ldz, const uint16_t* bias, float* out, int B, int nv, void* stream);

/* ---- K9  clip_by_global_norm + AdamWeightDecayOptimizer   src/optimizers.py:11-16,82-89,154-177
 * sumsq: out[0] = sum g^2 (deterministic two-stage; workspace dmi_sumsq_workspace_bytes(n)).
 * adam: mult = clip>0 ? clip/max(sqrt(*gnorm_sq),clip) : 1;  g*=mult; m=b1 m+(1-b1)g; v=b2 v+(1-b2)g^2;
 *       p -= lr*(m/(sqrt(v)+eps) + wd*p)   (NO bias correction); p_bf16 (optional) = bf16(p).
 * tf_adam=1 switches to tf.train.AdamOptimizer semantics (bias-corrected lr_t passed as lr, eps as given,
 * grad_scale multiplies g first: CrossShardOptimizer mean) -- src/model_fns_tf.py:58-61.
 * lr_dev (nullable): when given, the kernel reads the learning rate from lr_dev[0] (DEVICE memory) and ignores `lr` -- the
 * per-step schedule value (src/optimizers.py:46-76) can then change between replays of a captured HIP graph. */
int64_t dmi_sumsq_workspace_bytes(int64_t n);
int dmi_sumsq(const float* g, int64_t n, float* out, void* workspace, void* stream);
int dmi_adam_step(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n,
                  const float* gnorm_sq, float clip, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float grad_scale, const float* lr_dev, void* stream);

/* Weight EMA over the flat parameter buffer (a project extension: hparams "ema_decay"), once per optimizer step:
 * ema[i] <- ema[i] - (ema[i] - p[i]) * one_minus_decay   (tf.train.ExponentialMovingAverage / assign_moving_average);
 * ema_bf16[i] (nullable) = bf16(new ema[i]), round-to-nearest-even as dmi_cast_f32_bf16.
 * Difference, product and second difference are each rounded to fp32 (no fused multiply-add); NaN / Inf propagate as IEEE gives
 * them.  Nothing at or past index n is touched; no workspace, deterministic.  DMI_ERR_INVALID: null ema or p, n <= 0, a buffer
 * that is not 16-byte aligned, one_minus_decay NaN or outside [0, 1]. */
int dmi_ema_step(float* ema, const float* p, uint16_t* ema_bf16, int64_t n, float one_minus_decay, void* stream);

/* ---- K9b  mtf.optimize.AdafactorOptimizer   src/optimizers.py:91-97 (get_optimizer, "optimizer": "adafactor"), clip :100-103
 * Per variable, with gc = mult * g the clipped gradient (mult as for dmi_adam_step) and w the variable before the step:
 *   g2 = gc^2 + eps1;  scale = lr * max(rms(w), eps2)   (rms over the variable's real elements)
 *   factored:   vr = decay vr + (1-decay) mean_over_d0(g2);  vc = decay vc + (1-decay) mean_over_d1(g2)
 *               x = gc * rsqrt(vr / mean(vr)) * rsqrt(vc)
 *   otherwise:  v = decay v + (1-decay) g2;  x = gc * rsqrt(v)
 *   x /= max(1, rms(x));  u = scale * x;  beta1 != 0: m = beta1 m + (1-beta1) u, u = m;  w -= u;  p_bf16 (optional) = bf16(w)
 * (restated from mesh-tensorflow 0.1.18 optimize.py from memory: no mesh-tensorflow was available to check it against.)
 * The table holds DMI_AF_FIELDS int64 per variable; the caller fills fields 0..8, dmi_adafactor_plan fills 9..16 and writes
 * totals[3] = {tiles, segments, workspace bytes}; copy the planned table to device memory for the step.
 *   0 offset of element [0, 0] in p / g / m    1 rows R (1 for a 1-D variable)   2 cols C   3 leading dimension (>= C)
 *   4 factored (0/1)   5 1: vr is indexed by rows (d0 = the column axis), 0: vr is indexed by columns (d0 = the row axis)
 *   6 / 7 float offsets in `slots` of the row vector [R] / column vector [C] (factored)   8 offset of the dense v [R, C] (otherwise)
 * Elements past C in a row (pad columns) and everything outside the variables are neither read nor written.
 * gnorm_sq (out): sum of g^2 over all variables, computed by the step.  clip <= 0: no clipping.  lr_dev as for dmi_adam_step.
 * m may be NULL when beta1 == 0.  Six launches per step, deterministic (fixed reduction order, no atomics). */
#define DMI_AF_FIELDS 17
int dmi_adafactor_plan(int64_t* table, int nvars, int64_t* totals);
int dmi_adafactor_step(const int64_t* table_dev, int nvars, const int64_t* totals, float* p, const float* g, float* m,
                       float* slots, uint16_t* p_bf16, float* gnorm_sq, float clip, float lr, const float* lr_dev,
                       float decay, float beta1, float eps1, float eps2, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- data-parallel exchange: the all-reduce mtf inserts for `layout: batch_dim:data`   src/model_fns.py:81-82,189,
 * VAE src/model_fns_tf.py:61 (CrossShardOptimizer).  One process per GPU, RCCL over xGMI, bound at run time
 * (dmi_comm_load(path or NULL) -- call it first when the process already maps a specific librccl, e.g. PyTorch's).
 * Rank 0 draws dmi_comm_unique_id (HOST buffer of dmi_comm_unique_id_bytes()), the caller ships the bytes to all ranks
 * out of band, every rank calls dmi_comm_init (blocking collective; the current HIP device is the rank's GPU).
 * dmi_allreduce_bucket: g[0..n) <- sum over ranks (fp32, in place) enqueued on `stream` -- the caller orders it after the
 * bucket's last gradient kernel with an event and joins the stream before clip + Adam. */
int dmi_comm_load(const char* librccl_path);
int dmi_comm_unique_id_bytes(void);
int dmi_comm_unique_id(void* id_out);
int dmi_comm_init(void** comm_out, int nranks, int rank, const void* unique_id);
int dmi_comm_destroy(void* comm);
int dmi_allreduce_bucket(void* comm, float* g, int64_t n, void* stream);
int dmi_comm_broadcast_f32(void* comm, float* buf, int64_t n, int root, void* stream);

/* fp32 -> bf16 cast (initial weight export) */
int dmi_cast_f32_bf16(const float* in, uint16_t* out, int64_t n, void* stream);

/* n independent [R,C] -> [C,R] bf16 transposes between two buffers in one launch: table[i] = {in_off, out_off, R, C,
 * first_tile} (int64, elements / 64x64 tiles, first_tile ascending; R, C multiples of 8); total_tiles = sum of
 * ceil(R/64)*ceil(C/64).  The per-step refresh of the forward GEMMs' [out,in] weight copies (replaces what mtf's
 * einsum lowering does implicitly for y = x W, reference src/dalle_mtf/models.py:361-371). */
int dmi_transpose_bf16_batch(const uint16_t* in_base, uint16_t* out_base, const int64_t* table, int n,
                             int64_t total_tiles, void* stream);

/* in [R_valid, C] -> out [C, R_pitch] with columns [R_valid, R_pitch) zero (K-padding of transposed conv kernels) */
int dmi_transpose_bf16_padded(const uint16_t* in, uint16_t* out, int R_valid, int R_pitch, int C, void* stream);

/* ================= discrete VAE (src/vae_tf/models.py:81-163, src/vae_tf/layers.py:4-25) =================
 * K11 convolutions = implicit-im2col GEMMs (dmi_conv_gemm_nt / dmi_conv_wgrad_tn) for 64-channel-aligned layers; the
 * tap-list dmi_im2col + dmi_gemm_nt / dmi_gemm_tn path serves the 3-channel input layer and is the tested reference.
 * activations NHWC bf16 [B*H*W, C], C % 8 == 0. */
/* Implicit-im2col convolution: dmi_im2col + dmi_gemm_nt in one kernel, no column matrix in HBM, bit-identical results.
 *   out[(b,oy,ox)][n] = sum_t sum_c x[b, oy*stride + dy[t], ox*stride + dx[t], c] * Wt[n][t*C + c]  (+ epilogue flags)
 * x NHWC bf16 [B,H,W,C] with C % 64 == 0 (zero outside the image = TF SAME padding, src/vae_tf/models.py:67-68);
 * Wt [N, ldw] (ldw >= ntaps*C), out [B*Ho*Wo, ldc]; flags/bias/residual/relu_src as dmi_gemm_nt.  A batch whose x reaches
 * 2 GiB runs as launches over whole-image chunks (x is addressed through one buffer descriptor); one image must stay below. */
int dmi_conv_gemm_nt(const uint16_t* x, int B, int H, int W, int C, int Ho, int Wo, int stride, int ntaps,
                     const int* dy, const int* dx, const uint16_t* Wt, int ldw, uint16_t* out, int ldc, int N,
                     int flags, const uint16_t* bias, const uint16_t* residual, const uint16_t* relu_src, void* stream);

/* Implicit-im2col weight gradient: dW[(t*C + c)][n] = sum_{b,oy,ox} x[b, oy*stride+dy[t], ox*stride+dx[t], c] * dY[(b,oy,ox)][n]
 * (+ dbias[n] = column sums of dY, nullable) = dmi_im2col + dmi_gemm_tn without the column matrix; lands in the TF kernel
 * layout [kh*kw*Cin, Cout] of tf.layers.conv2d (src/vae_tf/models.py:67).  C % 64 == 0, Ho and Wo powers of two.
 * workspace >= dmi_conv_wgrad_tn_workspace_bytes(B*Ho*Wo, ntaps*C, N).  deferred / n_deferred as dmi_gemm_tn: the final slab
 * reduces are handed back for one dmi_reduce_slabs_batch launch (the workspace then belongs to this call until that launch).
 * A batch whose x reaches 2 GiB runs in whole-image chunks as dmi_conv_gemm_nt does; the chunks share the single launch's row
 * splits, so each writes its own slabs and the one slab reduce adds them in a fixed order.  That needs at least one split per
 * chunk.  The single launch splits 512 / tiles ways (128x128 output tiles of ntaps*C x N; one split from 257 tiles up), so a
 * batch in n chunks is refused above 512 / n tiles (the vae_coco layers that reach 2 GiB at B = 128 have 9 and 32 tiles). */
int64_t dmi_conv_wgrad_tn_workspace_bytes(int M, int K, int N);
int dmi_conv_wgrad_tn(const uint16_t* x, int B, int H, int W, int C, int Ho, int Wo, int stride, int ntaps,
                      const int* dy, const int* dx, const uint16_t* dY, int ldy, int N, float* dW, float* dbias,
                      void* workspace, dmi_reduce_item* deferred, int* n_deferred, void* stream);

/* out[(b,oy,ox)][t*C + c] = x[b, oy*stride + dy[t], ox*stride + dx[t], c] (0 outside); row pitch ldo, tail zero-filled.
 * dy/dx are HOST arrays (ntaps <= 16). */
int dmi_im2col(const uint16_t* x, uint16_t* out, int B, int H, int W, int C, int Ho, int Wo, int stride,
               int ntaps, const int* dy, const int* dx, int ldo, void* stream);
/* out[a][t*Bn + b] = in[idx[t]][a][b], row pitch ldo (tail zero)  (conv kernel [k][ci][co] -> [ci][(k',co)] for the
 * dgrad / output-parity GEMMs); idx on HOST */
int dmi_weight_gather(const uint16_t* in, uint16_t* out, int A, int Bn, int nsel, const int* idx, int ldo, void* stream);
/* n independent weight gathers between two buffers in ONE launch (the per-step refresh of every dgrad / output-parity weight
 * copy of a model): table[i] = {in_off, out_off, A, Bn, nsel, ldo, first_block, idx[16]} (23 int64 per row, DEVICE memory;
 * offsets in elements, first_block ascending, an item spans ceil(A*ldo / 2048) blocks); total_blocks = their sum. */
int dmi_weight_gather_batch(const uint16_t* in_base, uint16_t* out_base, const int64_t* table, int n, int64_t total_blocks,
                            void* stream);
/* out[b, 2t+py, 2u+px, :] = in4[py*2+px][b, t, u, :]  (assembles a stride-2 transposed convolution) */
int dmi_pixel_interleave(const uint16_t* in4, uint16_t* out, int B, int Ht, int Wt, int C, void* stream);
/* fp32 [N, Cin] <-> bf16 [N, Cp] (zero-padded channels): image in, reconstruction out */
int dmi_pad_channels(const float* in, uint16_t* out, int64_t N, int Cin, int Cp, void* stream);
int dmi_unpad_channels(const uint16_t* in, float* out, int64_t N, int Cin, int Cp, void* stream);
/* fp32 convolution of the TOKENISING encoder (the reference builds the VAE without use_bf16 inside dalle_model_fn,
 * src/model_fns.py:43-51, so image tokens come from fp32 convolutions and an fp32 x @ codebook, src/vae_tf/models.py:81-120):
 *   out[(b,oy,ox)][n] = sum_t sum_c x[b, oy*stride + dy[t], ox*stride + dx[t], c] * Wk[(t*C + c)][n] + bias[n] (ReLU) (+ residual)
 * x NHWC fp32 [B,H,W,C] (C % 8 == 0, zero outside the image = SAME padding), Wk fp32 [(ntaps*C), N] = the TF kernel layout
 * [kh,kw,Cin,Cout], bias / residual nullable, out fp32 [B*Ho*Wo, N], N % 4 == 0.  Exact-fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32).  One tap on a 1x1 image = a plain fp32 matmul (the codebook product). */
int dmi_conv2d_f32(const float* x, int B, int H, int W, int C, int Ho, int Wo, int stride, int ntaps, const int* dy,
                   const int* dx, const float* Wk, const float* bias, const float* residual, float* out, int N, int relu,
                   void* stream);
/* tf.space_to_depth / tf.depth_to_space (NHWC, block s; src/vae_tf/models.py:85-86,158-161) between the image
 * [B, Hs*s, Ws*s, C] and the stacked layout [B, Hs, Ws, Cp] with channel (dy*s + dx)*C + c, Cp >= s*s*C (pad = 0). */
int dmi_space_to_depth_f32(const float* img, float* stacked, int B, int Hs, int Ws, int C, int s, int Cp, void* stream);
int dmi_depth_to_space_f32(const float* stacked, float* img, int B, int Hs, int Ws, int C, int s, int Cp, void* stream);
/* K13 gumbel_softmax (layers.py:4-21) with INJECTED uniforms u in [1e-9, 1): y = softmax((logits - log(-log u))/T);
 * hard: y = one_hot(argmax) (first max), gradient straight-through.  y, y_soft bf16 [M,T]; index int32 [M] (nullable).
 * temperature_dev (nullable): read T from temperature_dev[0] (DEVICE memory) instead of the argument, so the annealed
 * schedule (src/model_fns_tf.py:40-45) can advance between replays of a captured HIP graph. */
int dmi_gumbel_softmax_fwd(const float* logits, const float* u, uint16_t* y, uint16_t* y_soft, int32_t* index,
                           int64_t M, int T, float temperature, int hard, const float* temperature_dev, void* stream);
int dmi_gumbel_softmax_bwd(const uint16_t* dy, const uint16_t* y_soft, uint16_t* dlogits, int64_t M, int T,
                           float temperature, const float* temperature_dev, void* stream);
/* K14 mse_loss (layers.py:24-25): loss[0] = mean((img - out)^2) over N*Cin; dout (nullable) = 2(out-img)*grad_scale/(N*Cin) */
int64_t dmi_mse_workspace_bytes(void);
int dmi_mse_loss(const float* img, const uint16_t* outp, uint16_t* dout, float* loss, int64_t N, int Cin, int Cp,
                 float grad_scale, void* workspace, void* stream);
int dmi_add_f32(float* dst, const float* src, int64_t n, void* stream);
/* KL(q(z|x) || uniform) of the codebook posterior and codebook usage (project extension; DESIGN.md §4 "VAE: KL term and codebook
 * statistics").  Per row m of the fp32 logits [M, T] (no noise, no temperature): lse = logsumexp_k l_k, q_k = exp(l_k - lse),
 * e = sum_k q_k ln q_k (a term with q = 0 contributes 0), KL_m = e + ln T, KL = mean_m KL_m (nats per position).
 * All: stream-ordered, no allocation, no float atomics (every sum has a fixed order: two runs give equal bits), rows indexed in
 * 64 bits.  DMI_ERR_INVALID with a message, before any launch: a null pointer, M <= 0, T % 8 != 0, T > 4096.
 *   dmi_codebook_kl_fwd        rowstat fp32 [M, 2] = (lse_m, e_m); kl[0] = KL.  workspace: dmi_codebook_kl_workspace_bytes(M, T)
 *                              bytes (covers dmi_codebook_usage too), 16-byte aligned.
 *   dmi_gumbel_softmax_bwd_kl  dmi_gumbel_softmax_bwd with the KL gradient added before the one bf16 rounding:
 *                              dlogits = bf16((1/tau) y_soft (dy - sum_j dy_j y_soft_j) + (beta_t / M) q (ln q - e)), q and ln q
 *                              recomputed from logits and rowstat.  kl_weight_dev (nullable): beta_t is read from device memory,
 *                              as temperature_dev is.  beta_t = 0 gives dmi_gumbel_softmax_bwd's bits.  By value: finite, >= 0.
 *   dmi_elbo_loss              loss[0] = recon[0] + beta_t * kl[0] in one rounding (device scalars; beta_t as above).
 *   dmi_codebook_usage         qsum fp32 [T] = sum_m q[m, k] (needs logits, rowstat); counts int32 [T] = #{m : index[m] == k}, exact
 *                              (needs index; values outside [0, T) are not counted).  Either pair may be null, not both. */
int64_t dmi_codebook_kl_workspace_bytes(int64_t M, int T);
int dmi_codebook_kl_fwd(const float* logits, float* rowstat, float* kl, int64_t M, int T, void* workspace, void* stream);
int dmi_gumbel_softmax_bwd_kl(const uint16_t* dy, const uint16_t* y_soft, const float* logits, const float* rowstat,
                              uint16_t* dlogits, int64_t M, int T, float temperature, const float* temperature_dev,
                              float kl_weight, const float* kl_weight_dev, void* stream);
int dmi_elbo_loss(const float* recon, const float* kl, float kl_weight, const float* kl_weight_dev, float* loss, void* stream);
int dmi_codebook_usage(const float* logits, const float* rowstat, const int32_t* index, float* qsum, int32_t* counts,
                       int64_t M, int T, void* workspace, void* stream);
/* Vector-quantised bottleneck (project extension; DESIGN.md §4 "VAE: vector quantisation").  X bf16 [M, ldx] (D channels),
 * codebook_t bf16 [T, ldc] (code k = row k: the transpose of the [D, T] codebook), h fp32 [T] the half-norms:
 *   s[m,k] = sum_j X[m,j] codebook_t[k,j] - h[k] (fp32)   idx[m] = lowest k among the maxima of s[m,:]   xq[m,:] = codebook_t[idx[m],:]
 * All: stream-ordered, no allocation, no float atomics (fixed summation orders: two runs give equal bits), rows indexed in 64 bits,
 * rows >= M never written, operands 16-byte aligned, every ld a multiple of 8 and >= D.  DMI_ERR_INVALID with a message naming
 * the argument, before any launch; DMI_ERR_UNSUPPORTED for a shape outside a kernel's range.
 *   dmi_vq_half_norms     h[k] = 1/2 sum_j c[j,k]^2 in fp32, from exactly one of codebook_t (bf16 [T, ldc], D % 8 == 0, D <= 512) and
 *                         codebook_f32 (the fp32 masters [D, T], for the exact-fp32 tokenising path).
 *   dmi_vq_assign         the scores product on v_mfma_f32_16x16x32_bf16 with the arg-max in its epilogue: idx int32 [M], xq bf16
 *                         [M, ldq] (nullable), score fp32 [M] = the winning s (nullable); nothing of size [M, T] is written.  The fp32
 *                         score of (m, k) depends on row m and column k alone, so equal columns tie and the lower index wins.
 *                         Supported: D % 64 == 0, 64 <= D <= 512, T % 64 == 0, T <= 4096, any M >= 1.
 *   dmi_vq_scores_bias    scores[m,k] -= h[k] on fp32 [M, T] (T % 4 == 0): turns the logits product into s when DALL-E tokenises.
 *   dmi_vq_loss           loss[0] = Lq = (1/(M D)) sum_m ||X[m] - xq[m]||^2; workspace: dmi_vq_loss_workspace_bytes() bytes.
 *   dmi_vq_bwd_x          dx = bf16(d + (2 beta/(M D)) (X - xq)) (difference, product and sum in fp32, one bf16 rounding); beta by
 *                         value, finite and >= 0; beta = 0 gives d's bits.
 *   dmi_vq_codebook_grad  dC fp32 [D, T]: dC[:,k] = (2/(M D)) sum_{m: idx[m]=k} (codebook_t[k,:] - X[m,:]); a code nobody picked gets
 *                         exactly 0; an idx outside [0, T) contributes nothing.  D % 8 == 0, D <= 512, T % 8 == 0, T <= 4096.
 *                         workspace: dmi_vq_codebook_grad_workspace_bytes(M, T, D) bytes (0 today: workspace may then be null).
 *   dmi_vq_gather         out[m,:] = codebook_t[idx[m],:]; an idx outside [0, T) gives a zero row and reads nothing. */
int dmi_vq_half_norms(const uint16_t* codebook_t, int ldc, const float* codebook_f32, float* h, int T, int D, void* stream);
int dmi_vq_assign(const uint16_t* x, int ldx, const uint16_t* codebook_t, int ldc, const float* h, int32_t* idx, uint16_t* xq,
                  int ldq, float* score, int64_t M, int T, int D, void* stream);
int dmi_vq_scores_bias(float* scores, const float* h, int64_t M, int T, void* stream);
int64_t dmi_vq_loss_workspace_bytes(void);
int dmi_vq_loss(const uint16_t* x, int ldx, const uint16_t* xq, int ldq, float* loss, int64_t M, int D, void* workspace,
                void* stream);
int dmi_vq_bwd_x(const uint16_t* d, int ldd, const uint16_t* x, int ldx, const uint16_t* xq, int ldq, uint16_t* dx, int lddx,
                 int64_t M, int D, float beta, void* stream);
int64_t dmi_vq_codebook_grad_workspace_bytes(int64_t M, int T, int D);
int dmi_vq_codebook_grad(const uint16_t* x, int ldx, const int32_t* idx, const uint16_t* codebook_t, int ldc, float* dC,
                         int64_t M, int T, int D, void* workspace, void* stream);
int dmi_vq_gather(const uint16_t* codebook_t, int ldc, const int32_t* idx, uint16_t* out, int ldo, int64_t M, int T, int D,
                  void* stream);
/* EMA codebook updates and dead-code restarts (project extension; DESIGN.md §4 "VAE: EMA codebook and restarts").  State per code k:
 * N fp32 [T], S fp32 [T, D] row-major, idle int32 [T]; one int32 counter restarts.  Initial state: N = 1, S[k] = C[:,k], idle = 0.
 *   dmi_vq_cluster_sums   counts int32 [T]: n[k] = #{m : idx[m] = k}, exact; sums fp32 [T, D]: s[k][c] = sum_{idx[m]=k} X[m][c] in fp32,
 *                         rows added in row order inside a chunk of rows and the chunks' partial sums in chunk order: no float atomics,
 *                         two runs give equal bits; a code nobody picked gets exactly 0; an idx outside [0, T) contributes nothing.
 *                         D % 8 == 0, D <= 512, T % 8 == 0, T <= 4096, 16-byte alignment (DMI_ERR_INVALID / DMI_ERR_UNSUPPORTED as for
 *                         dmi_vq_codebook_grad).  workspace: dmi_vq_cluster_sums_workspace_bytes(M, T, D) bytes (0 for M <= 4096:
 *                         workspace may then be null).
 *   dmi_vq_ema_step       with g = fp32(gamma), w = fp32(1 - gamma) (the difference in double) and every product rounded on its own:
 *                           n[k] > 0:  N' = g N + w float(n), S' = g S + w s, C[:,k] = S' / N', idle = 0
 *                           n[k] = 0:  N' = g N, S' = g S, idle += 1, C[:,k] keeps its bits (no division by a vanishing N)
 *                         then, when restart_after > 0, every k with idle[k] >= restart_after is re-seeded from row
 *                           m_k = splitmix64(splitmix64(splitmix64(seed) ^ step) + k) mod M    (uint64 arithmetic)
 *                         of X: C[:,k] = float(X[m_k]), N = 1, S[k] = C[:,k], idle = 0, restarts += 1.  Two dead codes may draw the
 *                         same row: the arg-max's tie-break (lowest index) then leaves one idle, re-seeded again restart_after steps on.
 *                         Every changed code is written to the fp32 master codebook_f32 [D, T] and, rounded to nearest even, to its
 *                         bf16 copy codebook_bf16 [D, T]; the others keep their bits in both.  step_dev (nullable): the step is read
 *                         from device memory (int64), so that a captured graph serves every step; else step by value.
 *                         0 < gamma < 1, restart_after >= 0 (0 never restarts), step >= 0; shapes as dmi_vq_cluster_sums. */
int64_t dmi_vq_cluster_sums_workspace_bytes(int64_t M, int T, int D);
int dmi_vq_cluster_sums(const uint16_t* x, int ldx, const int32_t* idx, float* sums, int32_t* counts, int64_t M, int T, int D,
                        void* workspace, void* stream);
int dmi_vq_ema_step(float* codebook_f32, uint16_t* codebook_bf16, float* N, float* S, int32_t* idle, int32_t* restarts,
                    const float* sums, const int32_t* counts, const uint16_t* x, int ldx, double gamma, int restart_after,
                    uint64_t seed, int64_t step, const int64_t* step_dev, int64_t M, int T, int D, void* stream);


/* ---- input format (host only): CRC-32C (Castagnoli) of a TFRecord length header / payload, as tf.data.TFRecordDataset
 * verifies them (reference src/input_fns.py:111); the caller applies TFRecord's mask.  No device work, thread-safe. */
uint32_t dmi_crc32c(const void* data, size_t n);

#ifdef __cplusplus
}
#endif
#endif

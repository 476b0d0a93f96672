// Host-side launchers of the miclip CDNA4 kernels (internal interface).
// Every launcher validates the shapes its kernel assumes and returns
// hipErrorInvalidValue instead of launching when they do not hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "miclip.h"

namespace miclip {

// ACT_GELU_TANH: GELU's tanh form, used only where the result is quantised to
// MX-fp8 next (gemm_mx epi 5): its <= 4.8e-4 deviation from the exact GELU is far
// below the e4m3 step (2^-3 relative)
enum Act { ACT_NONE = 0, ACT_QUICKGELU = 1, ACT_GELU = 2, ACT_GELU_TANH = 3 };

// ---- GEMM: C[M,N] = A[M,K] . W[N,K]^T (+ epilogue); A, W in compute dtype ----
// Shapes: N % 128 == 0, K % 64 == 0, any M >= 1; A, W rows K-contiguous.
// Store epilogue: C (compute dtype, ld = N) = act(acc + bias).
// `variant`: 0 = pick by size, 128 / 256 = force that tile (tests, A/B timing).
// skws / sk (the GEMMs of the CLS-only last block): split K into sk deterministic
// slices through an fp32 workspace skws of sk * M * N floats (K % (64 sk) == 0)
hipError_t gemm_store(int dtype, const void* A, const void* W, const float* bias, void* C,
                      int M, int N, int K, int act, hipStream_t s, int variant = 0,
                      float* skws = nullptr, int sk = 1);
// LayerNorm folded into the GEMM (epilogue.h, EpiStoreLN): A = the un-normalised
// rows, W = W diag(gamma) (ln_fold), stats [M] float2 {mean, rstd} (ln_stats);
// C = act(rstd * (acc - mean * colsum) + c).
hipError_t gemm_store_ln(int dtype, const void* A, const void* W, const float* c,
                         const float* colsum, const void* stats, void* C, int M, int N, int K,
                         int act, hipStream_t s, int variant = 0, float* skws = nullptr,
                         int sk = 1);
// Residual epilogue: X (ld = N) += acc + bias; X fp32, or fp16 when resid16
// (fp16 compute only: the reference's fp16 GPU residual stream).
hipError_t gemm_residual(int dtype, const void* A, const void* W, const float* bias, void* X,
                         int M, int N, int K, hipStream_t s, int variant = 0, int resid16 = 0,
                         float* skws = nullptr, int sk = 1);
// Float epilogue: C (fp32, ld = N) = acc + bias (bias may be null).
hipError_t gemm_f32(int dtype, const void* A, const void* W, const float* bias, float* C,
                    int M, int N, int K, hipStream_t s, int variant = 0);
// Diagnostic epilogue that writes nothing (prices the epilogue in A/B timing).
hipError_t gemm_null(int dtype, const void* A, const void* W, float* C, int M, int N, int K,
                     hipStream_t s, int variant = 0);
// Patch-embed epilogue: row m = b*np + p of the patch GEMM goes to token row
// b*(np+1) + 1 + p of X (fp32, or fp16 when resid16; ld = N), plus positional
// embedding row 1 + p. `variant` as gemm_store (the model passes 0; op tests force a tile).
hipError_t gemm_patch(int dtype, const void* A, const void* W, const float* pos, void* X,
                      int M, int N, int K, int np, hipStream_t s, int resid16 = 0,
                      int variant = 0);

// ---- MX-fp8 (OCP e4m3 + E8M0 per 32 k) operands and GEMM (gemm_mx.hip) ----
// Scale plane bytes of a [rows, K] operand (tiled, see mx_scale_index).
size_t mx_scale_bytes(int rows, int K);
// Rows [R, K] (fp32, or fp16 when in_f16; K % 256 == 0) -> data q [R, K] bytes + scales sc.
hipError_t quant_mx(int in_f16, const void* in, int R, int K, void* q, void* sc, hipStream_t s);
// C = A[M,K] . W[N,K]^T with MX-fp8 operands (N % 256 == 0, K % 128 == 0).
// epi 0: C fp16 = act(acc + bias); epi 1: C fp16 residual += acc + bias;
// epi 5: C MX-fp8 data [M, N] + scale plane CS = MX(act(acc + bias)).
// act: epi 0 none / QuickGELU / GELU, epi 1 none, epi 5 those and ACT_GELU_TANH;
// anything else is refused. bias may be null for epi 0 and 5.
// variant: 0 persistent where it applies (K >= 256), 1 one tile per workgroup,
// 2 persistent only (bit-identical kernels; A/B)
hipError_t gemm_mx(const void* A, const void* SA, const void* W, const void* SW, const float* bias,
                   void* C, void* CS, int M, int N, int K, int epi, int act, hipStream_t s,
                   int variant = 0);

// ---- LayerNorm (fp32 statistics, eps 1e-5) over rows of width D ----
// Row r of the input is at in + in_row(r)*D with in_row(r) = rows ? rows[r] : r*in_stride_rows;
// the input is fp32, or fp16 when in16 (fp16 residual stream).
// out_f32 != null -> fp32 output (may alias an fp32 in); else out_t in compute dtype (may
// alias an fp16 in of the same dtype).
// normalize != 0 additionally L2-normalises each output row (F.normalize, eps 1e-12).
// out_q != null: MX-fp8 output instead (data out_q [R, D] bytes + tiled scale plane
// out_s, the fp8 GEMM's A operand).
hipError_t layernorm(int dtype, const void* in, const int32_t* rows, int in_stride_rows,
                     const float* gamma, const float* beta, float* out_f32, void* out_t,
                     int R, int D, int normalize, hipStream_t s, int in16 = 0,
                     void* out_q = nullptr, void* out_s = nullptr);

// Row statistics of the fp16 residual stream for the folded LayerNorm: stats[r] =
// {mean, rstd * *rscale} of row r of in [R, D], mean and rstd exactly as layernorm
// computes them; rscale (device, nullable = 1) is the weight's 1/S from ln_fold.
hipError_t ln_stats(const void* in, float* stats, int R, int D, hipStream_t s,
                    const float* rscale = nullptr);
// Fold LayerNorm (gamma, beta) into the following Linear (W [N, K] compute dtype,
// bias [N] fp32 or null): Wf = W diag(gamma) * S (compute dtype), colsum[j] = sum_k Wf[j,k],
// c[j] = bias[j] + sum_k beta[k] W[j,k] (sums in double, fixed order). S is the power
// of two that puts max|W gamma| S in [2^14, 2^15] (no fp16 subnormals for small
// gamma); inv_scale (device float[2], nullable = no scaling) receives 1/S in [0].
hipError_t ln_fold(int dtype, const void* W, const float* gamma, const float* beta,
                   const float* bias, void* Wf, float* colsum, float* c, int N, int K,
                   hipStream_t s, float* inv_scale = nullptr);

// ---- fused multi-head attention over a packed QKV buffer ----
// qkv: [B*N, 3*H*dh] compute dtype (torch in_proj order q|k|v); out: [B*N, H*dh].
// head dim dh = 64 (OpenAI CLIP) or 80 (open_clip ViT-H/14 vision tower; one head
// per workgroup); causal adds the -inf strictly-upper-triangular mask
// (clip/model.py:323-329). N <= 640 (dh 64) or 416 (dh 80): a head's K and V sit
// in LDS whole; above that every variant is refused. variant (dh 64): 0 = default
// (the two-workgroup x8 kernel for non-causal N in 256..259, else the pipelined
// multi-head kernel while two K/V buffers fit, i.e. N padded to 32 <= 288, one head
// per workgroup above), 1 = one head per workgroup, 2 = pipelined, 4 = pipelined +
// last-chunk split (2 and 4 above N = 288: the one-head kernel, not a refusal),
// 8 = x8 (refused outside non-causal 256..259), 10-16 = one head per workgroup on
// that many waves (probe). variant (dh 80): 0 = default (the pipelined kernel at
// non-causal N in 256..259, else the two-phase kernel where it applies: non-causal
// N in 129..288), 1 = attention_kernel<80>, 2 = two-phase, 6 = pipelined (2 and 6
// are refused where they do not apply).
hipError_t attention(int dtype, const void* qkv, void* out, int B, int N, int H, int causal,
                     hipStream_t s, int variant = 0, int head_dim = 64);

// Attention of token row 0 (CLS) of every image only: out [B, H*dh] compact
// (row b = image b's CLS row), same qkv layout; N <= 768, dh 64 or 80 (0 = 64).
hipError_t attention_q0(int dtype, const void* qkv, void* out, int B, int N, int H,
                        hipStream_t s, int head_dim = 64);

// ---- embeddings / gathers ----
// dst[r, :] = src[r * stride_rows, :], rows of D elements of elt_bytes (2 or 4)
hipError_t gather_rows(const void* src, void* dst, int R, int stride_rows, int D, int elt_bytes,
                       hipStream_t s);
// images [B,3,R,R] (in_dtype: kIn32 fp32, kF16, kBF16) -> patches [B*g*g, Kp] compute
// dtype, col = c*P*P + ky*P + kx, zero-padded up to Kp (multiple of 64). variant 0:
// one workgroup per band of patches (vector loads) where R % 4 == 0, 1: one per patch.
hipError_t im2col(int dtype, int in_dtype, const void* img, void* patches, int B, int R, int P,
                  int Kp, hipStream_t s, int variant = 0);
// Clock probe: n_wg one-wave workgroups each store {HW_REG_XCC_ID, s_memtime,
// s_memrealtime, 0} (4 x u64) to out[4 * blockIdx.x ..].
hipError_t clock_probe(unsigned long long* out, int n_wg, hipStream_t s);
// X[b*ntok + 0, :] = cls + pos[0, :]  (X fp32, or fp16 when resid16)
hipError_t class_token(const float* cls, const float* pos, void* X, int B, int ntok, int D,
                       hipStream_t s, int resid16 = 0);
// X[p*L + t, :] = tok_emb[tokens[p*L + t], :] + pos[t, :]; eot[p] = argmax_t tokens[p*L+t]
// as a row index p*L + argmax (first maximum, like torch.argmax). X fp32 / fp16 (resid16).
hipError_t token_embed(const int64_t* tokens, const float* tok_emb, const float* pos, void* X,
                       int32_t* eot_rows, int P, int L, int D, int vocab, hipStream_t s,
                       int resid16 = 0);
// out[r, :] = in[r, :] @ Wm  (fp32 on the f32 MFMA, Wm [D, E] row-major, D % 16 == 0)
hipError_t rowvec_matmul(const float* in, const float* Wm, float* out, int R, int D, int E,
                         hipStream_t s);
// fp32 [rows, src_cols] -> compute dtype [rows, cols] (cols >= src_cols, zero pad), RNE
hipError_t cast_pad(int dtype, const float* in, void* out, int64_t rows, int src_cols, int cols,
                    hipStream_t s);
// in-place row L2 normalisation (F.normalize, eps 1e-12), fp32 [R, D]
hipError_t row_l2norm(float* x, int R, int D, hipStream_t s);
// zero-shot head: f = normalize(x @ proj) (proj may be null -> f = normalize(x));
// logits = scale * f @ tw ([E, C], E % 16 == 0) on the f32 MFMA with the row norm
// fused (head_logits_kernel); topk indices (sorted, largest first; topk_rows_kernel).
// The top-k order is torch.topk's: NaN ranks above every number (+inf included),
// and among NaNs or equal values the lower index comes first; for k <= C the k
// indices of a row are distinct and lie in [0, C) whatever the logits hold.
// With proj, scratch (fp32 [B, E]) receives the projection, which runs first as
// a chip-wide f32-MFMA kernel (head_proj_kernel, also behind rowvec_matmul).
hipError_t zero_shot(const float* x, const float* proj, const float* tw, float* logits,
                     int32_t* topk, int B, int Din, int E, int C, float scale, int k,
                     hipStream_t s, float* scratch = nullptr);

// ---- cached-feature consumers (outlier scoring), fp32 ----
// norms[r] = ||x[r]||; out = x / max(norms, eps) per row.
hipError_t row_norms(const float* x, int N, int D, float* norms, hipStream_t s);
hipError_t div_rows(const float* x, const float* norms, int N, int D, float eps, float* out,
                    hipStream_t s);
// class k's rows are order[offsets[k] .. offsets[k+1]) (ascending sample order);
// sums [K,D] = per-class sums in that order (a strict left-to-right fp32 sum, bit-
// equal to a CPU loop over the samples); centroids = normalize(sums / count). An
// empty class (offsets[k] == offsets[k+1]) has a sums row and a centroid row of
// exact zeros and changes no other class's rows.
hipError_t class_centroids(const float* x, const int32_t* order, const int32_t* offsets, int K,
                           int D, float eps, float* sums, float* centroids, hipStream_t s);
// sim[s,p] = (x[s] . protos[p]) * inv_nx[s] * inv_np[p] (null -> 1); per sample:
// own_best / own_arg = max / first argmax over p with owner[p] == cls[s],
// other_best = max over the other prototypes (-inf when none).
hipError_t proto_scores(const float* x, const float* protos, const int32_t* owner,
                        const int32_t* cls, const float* inv_nx, const float* inv_np, int N,
                        int P, int D, float* own_best, int32_t* own_arg, float* other_best,
                        hipStream_t s);

// ---- trimmed class centroids (trim.hip), fp32 ----
// Rank by counting costs sum n_k^2 compares, so the class size is bounded: the
// largest supported class has kTrimMaxClassRows rows. The layout is device memory,
// so the bound is enforced through N (no class is larger than N): N above it is
// hipErrorInvalidValue before any launch. kTrimTile: (value, index) pairs staged in
// LDS per step of the rank kernel (8 KiB).
constexpr int kTrimTile = 1024;
constexpr int kTrimMaxClassRows = 65536;
constexpr int kTrimMaxRounds = 8;
// rank_out[i] = #{j in class of i : (values[j], j) < (values[i], i)}, IEEE '<' on the
// fp32 values (-0 and +0 tie), sample order; order / offsets as in class_centroids.
// values must not hold NaN (a NaN ties with everything). K >= 1, 1 <= N <= kTrimMaxClassRows.
hipError_t segment_rank(const float* values, const int32_t* order, const int32_t* offsets, int K,
                        int N, int32_t* rank_out, hipStream_t s);
// rounds (1..kTrimMaxRounds) of {sims = x_i . c[cls[i]]; keep = rank >= drop[class];
// sums / centroids over the kept rows in ascending sample order} from the plain
// centroid, all enqueued on s with no host read. drop [K] is clamped to 0..n_k-1 on the
// device. keep uint8 [N], sims [N] (last round's), changed int32 [rounds] (flags flipped
// per round, keep_0 = all ones), sums / centroids [K, D]. 1 <= K <= 65535, D >= 1.
hipError_t trimmed_centroids(const float* x, const int32_t* order, const int32_t* offsets,
                             const int32_t* cls, const int32_t* drop, int K, int N, int D,
                             int rounds, float eps, float* sums, float* centroids,
                             uint8_t* keep, float* sims, int32_t* changed, hipStream_t s);

// ---- device k-means for the multi-prototype scorer (kmeans.hip), fp32 ----
// Pn problems, one workgroup each: problem p clusters class prob_class[p]'s rows
// (order / offsets as in class_centroids) into prob_k[p] <= k_max clusters; its
// per-row outputs and scratch start at prob_off[p] (floats / int32s). 1 <= D <= 1024,
// 2 <= k_max <= 16, 1 <= Pn <= 65535, max_iter >= 1, else hipErrorInvalidValue.
// kmeans_seed: k-means++ from the uniforms u [Pn, 16] -> picks [Pn, 16] (positions
// inside the class) and centres [Pn, 16, D]; scratch: one float per problem row.
hipError_t kmeans_seed(const float* x, const int32_t* order, const int32_t* offsets, int D,
                       const int32_t* prob_class, const int32_t* prob_k, const int32_t* prob_off,
                       int Pn, int k_max, const float* u, float* scratch, int32_t* picks,
                       float* centres, hipStream_t s);
// kmeans_lloyd: scikit-learn's Lloyd loop from centres (in/out), at most max_iter
// iterations, stop on unchanged labels (strict) or centre shift <= tol[p]; labels
// (per problem row), inertia / n_iter / strict [Pn] (strict may be null), counts [Pn, 16].
hipError_t kmeans_lloyd(const float* x, const int32_t* order, const int32_t* offsets, int D,
                        const int32_t* prob_class, const int32_t* prob_k,
                        const int32_t* prob_off, int Pn, int k_max, const float* tol,
                        int max_iter, float* scratch, float* centres, int32_t* labels,
                        float* inertia, int32_t* n_iter, int32_t* strict, int32_t* counts,
                        hipStream_t s);

// ---- exact t-SNE for the embedding-cache visualiser (tsne.hip), fp32 ----
// 4 <= N <= 16384, 1 <= D <= 4096 (metric 0 cosine, 1 euclidean; 2: x is the [N, N]
// matrix to use as it is and D is ignored), else hipErrorInvalidValue. scratch: 64 N bytes.
// tsne_affinities: dist [N, N] (null: not kept), the perplexity search per row -> beta [N],
// and the joint P [N, N], bit-symmetric with a zero diagonal.
hipError_t tsne_affinities(const float* x, int N, int D, int metric, float perplexity, float* P,
                           float* beta, float* dist, void* scratch, hipStream_t s);
// tsne_run: n_steps iterations of scikit-learn's _gradient_descent on y [N, 2] (in/out, with
// update and gains), two launches each, no host synchronisation. stats [4] = {KL, |grad|_2,
// Z, steps done} is written after every error_every-th step (0: after the last one only).
hipError_t tsne_run(const float* P, int N, float* y, float* update, float* gains, int n_steps,
                    float exaggeration, float momentum, float lr, float min_gain, int error_every,
                    void* scratch, float* stats, hipStream_t s);

// ---- ProLIP projector training on cached features (prolip.hip), fp32 ----
// One optimiser step of G configurations that share x [n, D] (x_dtype kIn32 / kF16 /
// kBF16, 16-B aligned), labels [n] in [0, C), W [E, C] and P0 [D, E] and differ in
// P / m / v [G, D, E], lr [G], lam [G]. D, E % 16 == 0, 16 <= D <= 1280,
// 16 <= E <= 1024, 1 <= C <= 1024, G <= 65535.
// prolip_grad: dZ [G, n, E] = d(mean CE of scale * normalize(x P_g) W) / d(x P_g);
// part [G, ceil(n/16), 2] = per 16-row tile {sum of CE, rows with argmax == label}.
hipError_t prolip_grad(int x_dtype, const void* x, const int64_t* labels, const float* W,
                       const float* P, float* dZ, float* part, int n, int D, int E, int C, int G,
                       float scale, hipStream_t s);
// prolip_adam: dP = x^T dZ_g + 2 (lam_g / lambda_div) (P_g - P0), then torch.optim.Adam's
// step `step` (1-based; betas 0.9 / 0.999, no weight decay) with lr_g * lr_factor on
// P_g, m_g, v_g; mse_part [G, prolip_adam_tiles(D, E)] = per-tile sum((P_g - P0)^2) before
// the update; history [G, 3] = {mean CE, that MSE, correct count} folded from
// grad_part (prolip_grad's part) and mse_part in a fixed order.
int prolip_adam_tiles(int D, int E);
hipError_t prolip_adam(int x_dtype, const void* x, const float* dZ, const float* P0, float* P,
                       float* m, float* v, const float* lr, const float* lam,
                       const float* grad_part, float* mse_part, float* history, int n, int D,
                       int E, int G, float lr_factor, float lambda_div, int step, float eps,
                       hipStream_t s);

// ---- Tip-Adapter cache classifier and (beta, alpha) search (tip.hip), fp32 ----
// Nq query rows, Nk cache keys, E embedding width, C classes, nb betas, na alphas:
// 1 <= Nq <= 2^24, 1 <= Nk <= 65536, E % 16 == 0, 16 <= E <= 1024, 1 <= C <= 1024,
// 1 <= nb, na <= 1024, nb * na <= 65536, else hipErrorInvalidValue. tip_bad_arg is the
// one statement of these limits: the first violated one as "<argument> must ...", or
// null. `which` (kTip* bits) says which arguments the call has; the others are not
// looked at, and every value of a selected argument, negative ones included, is checked.
enum TipArg : unsigned {
  kTipNq = 1, kTipNk = 2, kTipE = 4, kTipC = 8, kTipNb = 16, kTipNa = 32, kTipAll = 63
};
const char* tip_bad_arg(unsigned which, int64_t Nq, int64_t Nk, int64_t E, int64_t C, int64_t nb,
                        int64_t na);
size_t tip_scratch_bytes(int Nq, int Nk, int E, int C, int nb, int na);   // 0 outside the limits
// keys [Nk, E] = mean over the A views of normalize(x_v proj), divided by its row norm
// (a plain division: an all-zero row gives NaN). views: DEVICE array of A device
// pointers to x_v [Nk, Wv] (x_dtype kIn32 / kF16 / kBF16, 16-B aligned); proj [Wv, E].
// 1 <= A <= 1024, Wv % 16 == 0, 16 <= Wv <= 65536.
hipError_t tip_keys(int x_dtype, const void* const* views, int A, const float* proj, float* keys,
                    int Nk, int Wv, int E, hipStream_t s);
// aff [Nq, Nk] = scale * F keys^T; F [Nq, E] (f_dtype kIn32 / kF16 / kBF16), keys [Nk, E].
hipError_t tip_affinity(int f_dtype, const void* F, const float* keys, float* aff, int Nq, int Nk,
                        int E, float scale, hipStream_t s);
// correct [nb, na] = rows whose first argmax of Z + alphas[ia] * s(betas[ib]) is their
// label, s_c(beta) = sum over the keys k of class c of exp(-(beta - beta aff_k)) in
// ascending k. key_labels [Nk] and labels [Nq] int32 in [0, C); Z [Nq, C].
hipError_t tip_grid(const float* aff, const int32_t* key_labels, const float* Z,
                    const int32_t* labels, const float* betas, const float* alphas,
                    int32_t* correct, int Nq, int Nk, int C, int nb, int na, void* scratch,
                    hipStream_t s);
// out [Nq, C] = Z + alpha * s(beta): the numbers tip_grid compares, bit for bit.
hipError_t tip_logits(const float* aff, const int32_t* key_labels, const float* Z, float beta,
                      float alpha, float* out, int Nq, int Nk, int C, void* scratch,
                      hipStream_t s);
// tip_grid's stable counting sort alone: order [Nk] at scratch, offsets [C + 1] at
// scratch + tip_sort_offsets_at(Nk) (the head of tip_scratch_bytes' layout).
size_t tip_sort_offsets_at(int Nk);
hipError_t tip_sort_keys(const int32_t* key_labels, int Nk, int C, void* scratch, hipStream_t s);

// ---- Tip-Adapter-F: training the cache keys (tip_train.hip), fp32 ----
// n cached rows, b batch rows, Nk keys, E width, C classes, G configurations: 1 <= n <=
// 2^24, 1 <= b <= 4096, 1 <= G <= 64, Nk / E / C as tip_bad_arg; tipf_bad_arg names the
// first violated limit or returns null. scratch: tipf_scratch_bytes (0 outside the
// limits), 256-B aligned; tipf_prepare sorts the key labels into its head once per fit.
const char* tipf_bad_arg(int64_t n, int64_t b, int64_t Nk, int64_t E, int64_t C, int64_t G);
size_t tipf_scratch_bytes(int b, int Nk, int E, int C, int G);
hipError_t tipf_prepare(const int32_t* key_labels, int Nk, int C, void* scratch, hipStream_t s);
// One AdamW step of K / m / v [G, Nk, E] on the b rows rows_host (HOST int64, each in
// [0, n), checked before any launch) of F [n, E] (f_dtype kIn32 / kF16 / kBF16), Z [n, C]
// = 100 F W and labels [n] int32: loss = mean CE(Z_b + alpha_g S(beta_g)), step >= 1,
// lr_t = lrs[g] * lr_factor. history [G, 2] = {mean CE, correct rows} before the update;
// grad_out [G, Nk, E] or null.
hipError_t tipf_step(int f_dtype, const void* F, int n, const int64_t* rows_host, int b,
                     const int32_t* labels, const float* Z, const int32_t* key_labels, float* K,
                     float* m, float* v, const float* lrs, const float* betas,
                     const float* alphas, int Nk, int E, int C, int G, float lr_factor,
                     float weight_decay, float eps, int step, float* history, float* grad_out,
                     void* scratch, hipStream_t s);
// counts [>= epoch + 1, G] int32: where counts[epoch, g] is strictly greater than every
// earlier epoch's count and than 0, best_keys[g] = keys[g], best_count[g] = the count,
// best_epoch[g] = epoch.
hipError_t tipf_keep_best(const int32_t* counts, int epoch, const float* keys, float* best_keys,
                          int32_t* best_count, int32_t* best_epoch, int Nk, int E, int G,
                          hipStream_t s);

// ---- last-block fine-tuning of the image tower (finetune.hip) ----
// gemm_tn: G [Nn, K] fp32 = sum_m A[m, Nn] * X[m, K] (A, X compute dtype, row-major,
// 16-B aligned; both contracted along rows), times *out_scale (device, nullable).
// Nn, K % 16 == 0, 16 <= Nn, K <= 65536, M >= 1. M is split into `slices` slices of
// `slice_rows` rows (gemm_tn_plan, a function of the shape only) through the fp32
// workspace ws of gemm_tn_ws_bytes, summed in ascending slice order.
bool gemm_tn_shape_ok(int64_t M, int64_t Nn, int64_t K);
void gemm_tn_plan(int M, int Nn, int K, int* slices, int* slice_rows);
size_t gemm_tn_ws_bytes(int M, int Nn, int K);   // 0 for an unsupported shape
hipError_t gemm_tn(int dtype, const void* A, const void* X, float* G, int M, int Nn, int K,
                   float* ws, const float* out_scale, hipStream_t s);
// torch.optim.Adam's step `step` (1-based; betas 0.9 / 0.999, no weight decay) with the
// rate lr over one contiguous fp32 block of numel elements.
hipError_t ft_adam(float* params, const float* grads, float* m, float* v, int64_t numel, float lr,
                   int step, float eps, hipStream_t s);
// Group 1 (visual.proj) of the tail: y [B, W] fp32 = ln_post of the CLS rows, proj [W, E]
// the fp32 master; loss = mean CE of scale * normalize(y proj) tw against labels.
// dP [W, E] = d loss / d proj (operands y and dZ rounded once to the compute dtype, dZ
// under a power-of-two scale), stats = {sum of row CE, correct count}.
// W % 128 == 0, 128 <= W <= 1280, E % 16 == 0, 16 <= E <= 1024, 1 <= C <= 1024, B >= 1.
bool ft_proj_shape_ok(int64_t B, int64_t W, int64_t E, int64_t C);
size_t ft_proj_scratch_bytes(int B, int W, int E, int C);   // 0 for an unsupported shape
hipError_t ft_proj_grad(int dtype, const float* y, const int64_t* labels, const float* tw,
                        const float* proj, int B, int W, int E, int C, float scale, float* dP,
                        void* scratch, float* stats, hipStream_t s);
// Groups 1 and 2 from the residual stream x [B * N, W] (x_dtype kF16 or kIn32) entering the
// last vision block: forward of the tail, loss, and the gradients of the unlocked groups
// into grads (flat fp32 block laid out by ft_layout: the block's 12 tensors, ln_post's 2,
// proj; offsets [kFtTensors + 1], the last one the total). groups 1 writes dP only. stats =
// {sum of row CE, correct count}; y_out (nullable) [B, W] = ln_post of the CLS rows.
// ft_proj_grad's limits, 1 <= N <= 768, dh 64 or 80 dividing W, act ACT_QUICKGELU / ACT_GELU.
constexpr int kFtTensors = 15;
void ft_layout(int W, int E, int64_t* offsets);
bool ft_shape_ok(int64_t B, int64_t N, int64_t W, int64_t E, int64_t C, int64_t dh);
size_t ft_scratch_bytes(int B, int N, int W, int E, int C, int dh);   // 0 outside the limits
hipError_t ft_grad(int dtype, int x_dtype, const void* x, const int64_t* labels, const float* tw,
                   const float* params, int B, int N, int W, int E, int C, int dh, int act,
                   float scale, int groups, float* grads, void* scratch, float* stats,
                   float* y_out, hipStream_t s);
// ft_grad on the B images whose N-row blocks are x_cache[rows_host[b] * N ..), x_cache
// [cache_images * N, W]: the two reads of x (ln_1 over the token rows, the CLS residual rows)
// go through the row map, no gathered copy is formed, every output is bit-identical to
// ft_grad on a contiguous copy of those blocks. rows_host [B] is a HOST array, checked
// against [0, cache_images) before any launch and staged behind ft_grad's scratch
// (ft_rows_scratch_bytes = ft_scratch_bytes + the index area; 0 outside the limits).
// ft_grad's limits, 1 <= cache_images, cache_images * N * W < 2^47.
bool ft_rows_shape_ok(int64_t cache_images, int64_t B, int64_t N, int64_t W, int64_t E, int64_t C,
                      int64_t dh);
size_t ft_rows_scratch_bytes(int B, int N, int W, int E, int C, int dh);
hipError_t ft_grad_rows(int dtype, int x_dtype, const void* x_cache, int64_t cache_images,
                        const int64_t* rows_host, const int64_t* labels, const float* tw,
                        const float* params, int B, int N, int W, int E, int C, int dh, int act,
                        float scale, int groups, float* grads, void* scratch, float* stats,
                        float* y_out, hipStream_t s);

// ---- validation metrics (evaluate.hip), fp32 ----
// The caller-owned state block, as 8-byte words (include/miclip.h documents it):
// word 0 the float64 sum of batch-mean losses, words 1..7 integer counters, then the
// L3 confusion counts [C, C] and the L2 confusion counts [num_l2, num_l2].
enum EvalWord {
  kEvalLoss = 0, kEvalRows = 1, kEvalBatches = 2, kEvalTop1 = 3, kEvalTop3 = 4, kEvalL2Top1 = 5,
  kEvalL2Top3 = 6, kEvalSkipped = 7, kEvalHeaderWords = 8
};
// l2_mode (MICLIP_EVAL_L2_* in include/miclip.h)
enum EvalL2 { kEvalL2None = 0, kEvalL2Argmax = 1, kEvalL2Sum = 2, kEvalL2Mean = 3,
              kEvalL2LogSumExp = 4 };
size_t eval_state_bytes(int C, int num_l2);   // 0 for an unsupported (C, num_l2)
hipError_t eval_reset(void* state, int C, int num_l2, hipStream_t s);
// One batch: eval_rows_kernel (16 rows per workgroup) + eval_finalise_kernel. f [B, E]
// (f_dtype kIn32 / kF16 / kBF16, 16-B aligned), tw [E, C], labels [B]; with logits_in
// the logits [B, C] are read instead of computed (f, tw, E unused). l3_to_l2_host: HOST
// int32 [C], required exactly when l2_mode != kEvalL2None, entries in [0, num_l2).
// E % 16 == 0, 16 <= E <= 1024, 3 <= C <= 1024, 1 <= num_l2 <= C, B >= 1. row_loss [B]
// is required; every other output may be null.
hipError_t eval_batch(int f_dtype, const void* f, const float* tw, const int64_t* labels, int B,
                      int E, int C, float scale, const int32_t* l3_to_l2_host, int num_l2,
                      int l2_mode, bool logits_in, void* state, float* logits, float* row_loss,
                      int32_t* row_pred, int32_t* row_top3, float* row_top3_prob, int32_t* l2_pred,
                      int32_t* l2_top3, float* l2_logits, hipStream_t s);

// ---- on-device CLIP preprocessing (bicubic resize + center crop + normalise) ----
// PreCache: geometry-table cache + image-array buffers, one per model handle.
// descs: HOST array of B descriptors (validated, copied stream-ordered);
// out_kind 0 = float32 [B,3,n,n] normalised, 1 = uint8 [B,n,n,3]. On error
// fills `err`.
struct PreCache;
PreCache* pre_cache_create();
void pre_cache_destroy(PreCache* c);
hipError_t preprocess(PreCache* c, const uint8_t* pixels, const miclip_image_desc* descs, int B,
                      int n, int out_kind, void* out, hipStream_t s, char* err, int errlen);
// The train transform: per image augs[i] (HOST array) picks the geometry, the
// mirror and the rotation; tables and scratch are per call, owned by the cache.
hipError_t preprocess_aug(PreCache* c, const uint8_t* pixels, const miclip_image_desc* descs,
                          const miclip_aug_desc* augs, int B, int n, int out_kind, void* out,
                          hipStream_t s, char* err, int errlen);

}  // namespace miclip

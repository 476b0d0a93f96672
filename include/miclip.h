/*
 * miclip.h -- C ABI of the MI355X-native CLIP encode path (libmiclip.so).
 *
 * The reference (WhiteGiveFive/aihab-clip) is pure Python and has no FFI; its
 * hot path is the PyTorch call chain behind `clip.load` / `model.encode_image`
 * / `model.encode_text` and the zero-shot head. Each entry point below states
 * the reference interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - Plain pointers and sizes only. Image/token/feature/logit buffers are
 *     caller-owned DEVICE pointers on the handle's device (e.g. torch tensors'
 *     data_ptr()); weights and workspaces are handle-owned.
 *   - Every call is stream-ordered on the caller's `stream` (a hipStream_t;
 *     NULL = the legacy default stream). No call synchronises the device,
 *     except miclip_model_load_weights / miclip_reserve, which allocate.
 *   - Return value: 0 on success, a negative MICLIP_E* code on failure; the
 *     message is available from miclip_last_error() (thread-local).
 *   - A handle is bound to one device and is not safe for concurrent calls
 *     from several host threads.
 */
#ifndef MICLIP_H_
#define MICLIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MICLIP_ABI_VERSION 10

enum miclip_status {
  MICLIP_OK = 0,
  MICLIP_EINVAL = -1,   /* bad argument / shape (reference raises ValueError / RuntimeError) */
  MICLIP_EHIP = -2,     /* HIP runtime error */
  MICLIP_ENOWEIGHTS = -3, /* a tower's weights were not loaded */
  MICLIP_ENOMEM = -4
};

/* MICLIP_MXFP8: the vision tower's QKV, out-proj, c_fc and c_proj on OCP MX-fp8
 * operands (e4m3 + an E8M0 scale per 32 k; weights quantised at load, activations
 * by the producing kernels), the rest -- the whole text tower included -- as
 * MICLIP_FP16. SURVEY §8f row 4 (C5 fp8 weights); parity unpinned. */
/* MICLIP_F32: an input element type only (miclip_encode_image_ex images). */
enum miclip_dtype { MICLIP_FP16 = 0, MICLIP_BF16 = 1, MICLIP_MXFP8 = 2, MICLIP_F32 = 3 };
/* MICLIP_ACT_GELU_TANH: GELU's tanh form, accepted by the op-level MX-fp8 GEMM
 * (miclip_op_gemm_mx epi 5) -- the model's MX c_fc uses it where its output is
 * quantised to e4m3; a model config's act is QUICKGELU or GELU */
enum miclip_act { MICLIP_ACT_QUICKGELU = 1, MICLIP_ACT_GELU = 2, MICLIP_ACT_GELU_TANH = 3 };

/* encode_image flags */
#define MICLIP_FLAG_NORMALIZE 1u  /* F.normalize(feats, dim=-1): aihab_utils/feature_cache.py:126-127 */
#define MICLIP_FLAG_APPLY_PROJ 2u /* feats @ visual.proj:       methods/ProLIP.py:38-41 */
/* miclip_encode_image_ex only: `out` holds fp16 (or bf16) features, the fp32
 * result rounded once (RNE) -- the element type of the reference's GPU path
 * (clip.load on cuda keeps the model fp16, so encode_image returns fp16 and the
 * cached f{v}.pth / embeddings.pt are fp16: aihab_utils/feature_cache.py:126-131,
 * 208-222). The two exclude each other. */
#define MICLIP_FLAG_OUT_FP16 4u
#define MICLIP_FLAG_OUT_BF16 8u

/* Model hyper-parameters; the fields of clip/model.py:240-254 (CLIP.__init__),
 * as inferred by build_model (clip/model.py:396-419). ViT towers only. */
typedef struct miclip_config {
  int32_t embed_dim;
  int32_t image_resolution;
  int32_t vision_layers;
  int32_t vision_width;
  int32_t vision_patch_size;
  int32_t context_length;
  int32_t vocab_size;
  int32_t transformer_width;
  int32_t transformer_heads;
  int32_t transformer_layers;
  int32_t compute_dtype; /* miclip_dtype: GEMM/attention operand type (fp32 accumulate) */
  int32_t act;           /* miclip_act: QuickGELU (clip/model.py:160-162) or exact GELU */
  int32_t vision_head_dim; /* 0 or 64: heads = width // 64 (clip/model.py:268); 80: open_clip
                              ViT-H/14 (16 heads of 80 on width 1280) */
  uint32_t options;        /* MICLIP_OPT_* bits (ABI 7); 0 = the default numerics path */
} miclip_config;

/* Numerics options of a model handle (miclip_config.options). Every path that
 * changes what the kernels compute is chosen here, explicitly -- the library
 * reads no environment variables.
 * RESID_F32: fp32 residual stream (default: fp16 under fp16 AND bf16 compute --
 *   the reference's GPU model keeps its residual stream in half; bf16 compute then
 *   rounds only the GEMM / attention operands to bf16). NO_LN_FOLD: run ln_1 / ln_2
 *   as LayerNorm kernels (default under fp16 compute: folded into the QKV / c_fc
 *   GEMMs on the fp16 stream; bf16 compute never folds: the GEMM would read the fp16
 *   stream as its bf16 operand).
 * MX_OUT_FP16 (MICLIP_MXFP8): keep the vision out-projection fp16 (default MX-fp8).
 * MX_GELU_ERF (MICLIP_MXFP8): exact-erf GELU in the MX c_fc epilogue (default: the
 *   tanh form, <= 4.8e-4 from erf, below the e4m3 step).
 * FULL_LAST_BLOCK: run the last vision block over every token row (default: the
 *   CLS rows only after its QKV GEMM, the only rows ln_post reads, clip/model.py:
 *   226-229); switchable at run time with miclip_model_set_option. */
#define MICLIP_OPT_RESID_F32 1u
#define MICLIP_OPT_NO_LN_FOLD 2u
#define MICLIP_OPT_MX_OUT_FP16 4u
#define MICLIP_OPT_MX_GELU_ERF 8u
#define MICLIP_OPT_FULL_LAST_BLOCK 16u

/* One host fp32 tensor of a CLIP state dict, named as in CLIP.state_dict(). */
typedef struct miclip_tensor {
  const char* name;
  const float* data; /* host, contiguous fp32 */
  int64_t numel;
} miclip_tensor;

typedef struct miclip_model miclip_model;

/* Replaces the construction half of clip.load (clip/clip.py:89-137) /
 * build_model (clip/model.py:396-433): creates an empty model on `device`. */
int miclip_model_create(const miclip_config* cfg, int device, miclip_model** out);

/* Replaces model.load_state_dict + convert_weights (clip/model.py:372-393, 432):
 * copies/repacks the named tensors into handle-owned device memory (GEMM
 * weights in the compute dtype, LayerNorm/bias/embeddings fp32). May be called
 * several times; unknown names are an error, "logit_scale" is accepted and unused. */
int miclip_model_load_weights(miclip_model* m, const miclip_tensor* tensors, int32_t n);
/* Same, with every `data` a DEVICE pointer (fp32, contiguous, on the handle's
 * device): e.g. the model's own torch Parameters after .to(device), so a device
 * move never round-trips the state dict through host memory. Repacking (cast to
 * the compute dtype, conv1 padding, MX quantisation) runs on the device. */
int miclip_model_load_weights_device(miclip_model* m, const miclip_tensor* tensors, int32_t n);

/* Pre-allocates workspaces for up to max_images images / max_prompts prompts,
 * so later encode calls allocate nothing (required before hipGraph capture). */
int miclip_reserve(miclip_model* m, int32_t max_images, int32_t max_prompts);

/* Replaces CLIP.encode_image -> VisionTransformer.forward (clip/model.py:335-336,
 * 216-235). images: device fp32 [B,3,R,R] (CLIP-normalised, clip/clip.py:80).
 * out: device fp32 [B, vision_width] pre-projection features (the modified
 * reference returns ln_post(x[:,0,:]) without @proj, clip/model.py:228-235), or
 * [B, embed_dim] with MICLIP_FLAG_APPLY_PROJ; MICLIP_FLAG_NORMALIZE L2-normalises.
 * fp32 out only (the OUT_FP16 / OUT_BF16 flags are miclip_encode_image_ex's). */
int miclip_encode_image(miclip_model* m, const float* images, int32_t B, float* out,
                        uint32_t flags, void* stream);

/* miclip_encode_image with the input batch's element type named:
 * image_dtype MICLIP_F32, MICLIP_FP16 or MICLIP_BF16 (a device-resident half
 * batch, e.g. the reference's `images.to(device).half()` under clip.load on GPU,
 * clip/model.py:336 `image.type(self.dtype)`, read directly by the patchify:
 * half the input bytes of fp32). Same outputs and flags, plus MICLIP_FLAG_OUT_FP16 /
 * MICLIP_FLAG_OUT_BF16: `out` is then [B, dim] 2-byte elements. Unknown flag
 * bits: MICLIP_EINVAL. */
int miclip_encode_image_ex(miclip_model* m, const void* images, int32_t image_dtype, int32_t B,
                           void* out, uint32_t flags, void* stream);

/* Replaces CLIP.encode_text (clip/model.py:338-353), which returns the tuple
 * (x_before_proj [P, transformer_width], x [P, embed_dim]). tokens: device
 * int64 [P, context_length] as produced by clip.tokenize (clip/clip.py:192-228);
 * EOT row = first argmax of each row. Either output may be NULL. */
int miclip_encode_text(miclip_model* m, const int64_t* tokens, int32_t P, float* x_before,
                       float* x_proj, void* stream);

/* Replaces the zero-shot head of ProLIP eval / compute_image_features_test:
 * f = F.normalize(feats @ visual.proj) (apply_proj != 0) or F.normalize(feats);
 * logits = scale * f @ text_weights  (methods/ProLIP.py:38-41, 288-291;
 * methods/utils.py:181-186; scale 100 in the reference); topk = logits.topk(k)
 * indices, sorted (methods/utils.py:16-21). feats: device fp32 [B, Din];
 * text_weights: device fp32 [embed_dim, C] (clip_classifier output, utils.py:54);
 * logits: device fp32 [B, C]; topk: device int32 [B, k] or NULL. */
int miclip_zero_shot(miclip_model* m, const float* feats, int32_t B, int32_t apply_proj,
                     const float* text_weights, int32_t C, float scale, float* logits,
                     int32_t* topk, int32_t k, void* stream);

/* One decoded image in device memory: interleaved HWC uint8 ('RGB' or 'L'). */
typedef struct miclip_image_desc {
  int64_t offset;     /* byte offset of pixel (0, 0) from the `pixels` base */
  int32_t height;
  int32_t width;
  int32_t channels;   /* 3 (RGB) or 1 (L; replicated to RGB like convert("RGB")) */
  int32_t row_stride; /* bytes between rows; 0 = width * channels */
} miclip_image_desc;

enum miclip_pre_out {
  MICLIP_PRE_F32 = 0, /* float32 [B, 3, R, R], ToTensor + Normalize(CLIP_MEAN, CLIP_STD) */
  MICLIP_PRE_U8 = 1   /* uint8 [B, R, R, 3], the resized + center-cropped RGB pixels */
};

/* On-device CLIP preprocessing, R = the model's image_resolution. Replaces the
 * per-image CPU transform of clip/clip.py:74-81 (`_transform`) and
 * data/clip_transforms.py:50-55 (test split): Resize(R, BICUBIC) of the shorter
 * side -> CenterCrop(R) -> RGB -> ToTensor -> Normalize; bit-exact with
 * Pillow's resize (libImaging/Resample.c) and torchvision's size/anchor rules.
 * pixels: device uint8 base; descs: HOST array [B] (copied, stream-ordered,
 * into a handle-owned device buffer before return); out: device, see
 * miclip_pre_out. Images may differ in size (ragged batch). Errors: EINVAL for
 * a bad descriptor or a downscale beyond 64 taps (about 16x at R = 224). */
int miclip_preprocess(miclip_model* m, const uint8_t* pixels, const miclip_image_desc* descs,
                      int32_t B, void* out, int32_t out_kind, void* stream);

enum miclip_aug_mode {
  MICLIP_AUG_RESIZE_CENTER = 0, /* Resize(R) of the short side + CenterCrop(R), as miclip_preprocess */
  MICLIP_AUG_STRETCH = 1,       /* crop the box, then resize it to R x R (RandomResizedCrop) */
  MICLIP_AUG_CROP = 2           /* crop the R x R box (BottomSquareCrop) */
};

/* One image's train-transform parameters, drawn by the caller. */
typedef struct miclip_aug_desc {
  int32_t mode;                     /* miclip_aug_mode */
  int32_t top, left, height, width; /* box inside the image: STRETCH, CROP */
  int32_t flip;                     /* mirror left-right, after the resize */
  int32_t rotate;                   /* 0: none */
  int32_t affine[6];                /* a0 a1 a2 a3 a4 a5, 16.16, half-pixel folded in */
} miclip_aug_desc;

/* miclip_preprocess with the reference's train transform
 * (data/clip_transforms.py:36-49): per image the geometry of `mode`, then the
 * mirror (transpose(FLIP_LEFT_RIGHT) of the resized image), then
 * RandomRotation's Image.rotate(angle, NEAREST, expand=False, fillcolor=0) as
 * Pillow's 16.16 fixed-point gather over the R x R image:
 *   xin = (a2 + y*a1 + x*a0) >> 16, yin = (a5 + y*a4 + x*a3) >> 16
 * in wrapping 32-bit arithmetic, the source pixel where it lies inside the
 * image and 0 elsewhere; then RGB, ToTensor and Normalize. The random draws and
 * the matrix are the caller's (miclip/augment.py); the result is a deterministic
 * function of them, bit-exact with Pillow, and an image's result does not
 * depend on the rest of the batch. augs: HOST array [B], copied like descs.
 * Coefficient tables and the rotation's input live in handle-owned buffers that
 * are reused from call to call. Errors: EINVAL for a bad descriptor, a box that
 * leaves the image, a CROP box that is not R x R, more than 64 taps in either
 * pass, an unknown mode. */
int miclip_preprocess_aug(miclip_model* m, const uint8_t* pixels, const miclip_image_desc* descs,
                          const miclip_aug_desc* augs, int32_t B, void* out, int32_t out_kind,
                          void* stream);

/* ---- cached-feature consumers: outlier scoring, fp32 ----
 * Replace the torch ops of tools/outlier_cleaning.py's scorers on the
 * embeddings cache; all pointers are device memory, calls stream-ordered.
 * miclip_row_norms: norms[N] = emb.norm(dim=-1) (outlier_cleaning.py:234);
 * with out != NULL also out = emb / max(norms, eps) (:244). */
int miclip_row_norms(const float* x, int32_t N, int32_t D, float* norms, float eps, float* out,
                     void* stream);
/* Per-class normalised centroids (compute_centroids, :266-276): class k's
 * rows are order[offsets[k] .. offsets[k+1]) in ascending sample order (a
 * stable sort of the labels), summed in that order -- bit-identical to the
 * CPU index_add_ -- then means = sums / count, F.normalize(eps).
 * sums: scratch [K, D]; centroids: [K, D]. */
int miclip_class_centroids(const float* x, const int32_t* order, const int32_t* offsets,
                           int32_t K, int32_t D, float eps, float* sums, float* centroids,
                           void* stream);
/* Nearest-prototype scores (score_prototype_distance, :626-673; with inverse
 * norms the cosine of score_centroid_distance, :329): sim = x . proto *
 * inv_nx[s] * inv_np[p] (either may be NULL = 1); own_best / own_arg = best
 * similarity and first best prototype index among owner[p] == cls[s];
 * other_best = best over the other prototypes (-inf when there are none). */
int miclip_proto_scores(const float* x, const float* protos, const int32_t* owner,
                        const int32_t* cls, const float* inv_nx, const float* inv_np, int32_t N,
                        int32_t P, int32_t D, float* own_best, int32_t* own_arg,
                        float* other_best, void* stream);

/* ---- trimmed class centroids, fp32 ----
 * The "trimmed-centroid support" that compute_centroids(trim_frac=...) is reserved
 * for (tools/outlier_cleaning.py:250-257). Mislabelled rows pull the plain mean
 * towards themselves; a trimmed centroid drops the drop[k] rows of class k that
 * are least similar to the class centroid and re-forms it from the rest:
 *   c_0 = the centroid of miclip_class_centroids (same kernels, bit for bit);
 *   round t = 1..rounds:
 *     s_i   = x_i . c_{t-1}[cls[i]]           (fp32, a fixed summation order per row)
 *     r_i   = rank of row i among ALL rows of its class by the key (s ascending,
 *             sample index ascending); IEEE '<' on the fp32 values, so -0 and +0 tie
 *     keep_t[i] = r_i >= drop[class]
 *     c_t   = normalize(sum of the kept rows in ascending sample order / kept count)
 *     changed[t-1] = #{i : keep_t[i] != keep_{t-1}[i]},  keep_0 = all ones.
 * drop[k] = floor(trim_frac * n_k) is the caller's (an integer, computed on the
 * host); the device clamps it to 0 .. n_k - 1, so a non-empty class keeps at least
 * one row. With every drop[k] == 0 the centroids are bit-identical to
 * miclip_class_centroids. There are no float atomics: results are bit-identical run
 * to run. Ranking counts pairs (sum n_k^2 compares), so the largest supported class
 * has MICLIP_TRIM_MAX_CLASS_ROWS rows; the layout is device memory, so the bound is
 * enforced through N (no class is larger than N). All pointers are caller-owned
 * device memory; the calls are stream-ordered, never synchronise and never allocate.
 * Limits: 1 <= K <= 65535, 1 <= N <= MICLIP_TRIM_MAX_CLASS_ROWS, D >= 1,
 * 1 <= rounds <= MICLIP_TRIM_MAX_ROUNDS, no NULL pointer; anything else is
 * MICLIP_EINVAL with the argument named in miclip_last_error, before any launch.
 * values / x must be free of NaN (a NaN ties with every value). */
#define MICLIP_TRIM_MAX_CLASS_ROWS 65536
#define MICLIP_TRIM_MAX_ROUNDS 8
/* miclip_segment_rank (outlier_cleaning.py:250-257, the selection step on its own):
 * rank_out[i] = #{j in the class of i : (values[j], j) < (values[i], i)} for the
 * class layout order / offsets of miclip_class_centroids; values, rank_out: [N] in
 * sample order. Within a class the ranks are a permutation of 0 .. n_k - 1. */
int miclip_segment_rank(const float* values, const int32_t* order, const int32_t* offsets,
                        int32_t K, int32_t N, int32_t* rank_out, void* stream);
/* miclip_trimmed_centroids (outlier_cleaning.py:250-257): all `rounds` rounds in one
 * call, with no host read in between. x [N, D]; cls int32 [N] = class index of each
 * row (the inverse of order / offsets); drop int32 [K]. Outputs: sums [K, D] (the
 * kept rows' sums of the last round), centroids [K, D] = c_rounds, keep uint8 [N] =
 * keep_rounds, sims [N] = the similarities of the last round (against
 * c_{rounds-1}), changed int32 [rounds]. */
int miclip_trimmed_centroids(const float* x, const int32_t* order, const int32_t* offsets,
                             const int32_t* cls, const int32_t* drop, int32_t K, int32_t N,
                             int32_t D, int32_t rounds, float eps, float* sums, float* centroids,
                             uint8_t* keep, float* sims, int32_t* changed, void* stream);

/* ---- device k-means for the multi-prototype scorer, fp32 ----
 * Replace the per-class KMeans(n_init, max_iter).fit of compute_prototypes
 * (tools/outlier_cleaning.py:511-541) by two launches over a problem table: a
 * launch runs Pn problems, one workgroup each. Problem p clusters the rows of
 * class prob_class[p] -- order[offsets[c] .. offsets[c+1]), the class layout of
 * miclip_class_centroids -- into prob_k[p] clusters; the restarts of a class are
 * separate problems naming the same class. prob_off[p] is the problem's offset
 * (in elements) into the per-row buffers `labels` and `scratch`, which hold one
 * element per problem row (scratch: miclip_kmeans_scratch_bytes(total rows)
 * bytes, shared by both calls). Per-problem blocks have 16 slots whatever k is:
 * u / picks / counts [Pn, 16], centres [Pn, 16, D]; slots >= k are not written
 * (counts: 0). Limits: 1 <= D <= 1024, 1 <= Pn <= 65535, 2 <= k_max <= 16 (the
 * caller's bound on prob_k), max_iter >= 1; anything else is MICLIP_EINVAL with
 * the argument named in miclip_last_error, before any launch. The table itself is
 * device memory and is checked on the device: a problem with prob_k outside
 * 2..16 or fewer rows than clusters is skipped (picks = -1, n_iter = -1). All
 * pointers are caller-owned device memory; the calls are stream-ordered, never
 * synchronise and never allocate. A problem's results are bit-identical run to
 * run and do not depend on Pn or on its index.
 *
 * miclip_kmeans_seed (tools/outlier_cleaning.py:511-541, KMeans' init): plain
 * k-means++ with one candidate per step from the uniforms u in [0, 1). Pick 0 is
 * row min(floor(u0 n), n - 1); pick t is the first row whose inclusive prefix of
 * mind[j] = min over the chosen centres of |x_j - c|^2 exceeds u_t * total, or the
 * lowest row not yet chosen when total == 0. picks are positions inside the
 * class; centres receives the chosen rows. */
int64_t miclip_kmeans_scratch_bytes(int64_t total_rows);
int miclip_kmeans_seed(const float* x, const int32_t* order, const int32_t* offsets, int32_t D,
                       const int32_t* prob_class, const int32_t* prob_k, const int32_t* prob_off,
                       int32_t Pn, int32_t k_max, const float* u, float* scratch, int32_t* picks,
                       float* centres, void* stream);
/* miclip_kmeans_lloyd (tools/outlier_cleaning.py:511-541, KMeans.fit's Lloyd
 * loop, rule for rule as scikit-learn runs it): from the initial `centres`
 * (in/out) at most max_iter iterations of {labels = argmin_j |x - c_j|^2, lowest
 * index on a tie; centres = cluster means; an empty cluster, in ascending order,
 * takes the row farthest from its own centre (lowest row among equals), which
 * leaves its old cluster}; stop when the labels repeat (strict[p] = 1) or when
 * sum_j |c_j_new - c_j_old|^2 <= tol[p] (strict[p] = 0, followed by one more
 * labelling so labels match centres). inertia[p] = sum |x - c_label|^2, n_iter[p]
 * the iterations run, counts the final cluster sizes. strict may be NULL. */
int miclip_kmeans_lloyd(const float* x, const int32_t* order, const int32_t* offsets, int32_t D,
                        const int32_t* prob_class, const int32_t* prob_k, const int32_t* prob_off,
                        int32_t Pn, int32_t k_max, const float* tol, int32_t max_iter,
                        float* scratch, float* centres, int32_t* labels, float* inertia,
                        int32_t* n_iter, int32_t* strict, int32_t* counts, void* stream);

/* ---- exact t-SNE for the embedding-cache visualiser, fp32 ----
 * Replace sklearn.manifold.TSNE(n_components=2, perplexity, metric, init).fit_transform
 * of feat_cache_vis/feat_vis.py:150-157 by its exact form on the device: dense P,
 * all-pairs repulsion, no tree and no neighbour truncation, one Student-t degree of
 * freedom. The arithmetic rules are scikit-learn 1.7's (_t_sne.py, _utils.pyx).
 * Limits: 4 <= N <= 16384, 1 <= D <= 4096, 1 <= perplexity < N, n_steps >= 1,
 * error_every >= 0, learning_rate and min_gain finite and > 0, exaggeration finite
 * and > 0, 0 <= momentum < 1, no NULL pointer except `dist`; anything else is
 * MICLIP_EINVAL with the argument named in miclip_last_error, before any launch.
 * All pointers are caller-owned device memory (scratch: miclip_tsne_scratch_bytes(N)
 * bytes, 16-byte aligned, shared by both calls; 0 for an N outside the limits). The
 * calls are stream-ordered, never synchronise and never allocate. There are no float
 * atomics: results are bit-identical run to run.
 *
 * miclip_tsne_affinities (TSNE._fit's pairwise_distances + _joint_probabilities):
 * metric 0 cosine -- clip(1 - cos, 0, 2) with a zero diagonal (cosine_distances), then
 * squared as _t_sne.py:945-946 squares every non-euclidean metric; 1 euclidean --
 * squared distance clamped at 0, zero diagonal; 2 precomputed -- x is the [N, N]
 * matrix the search is fed as it is, D is ignored. dist (may be NULL) receives that
 * matrix. Per row _binary_search_perplexity (beta from 1, at most 100 steps, tolerance
 * 1e-5 on the entropy, sums in fp64) -> beta [N]; then P = max((C + C^T) / max(sum,
 * eps), eps) off the diagonal, 0 on it, eps = 2^-52; P [N, N] is bit-symmetric. */
int64_t miclip_tsne_scratch_bytes(int32_t N);
int miclip_tsne_affinities(const float* x, int32_t N, int32_t D, int32_t metric, float perplexity,
                           float* P, float* beta, float* dist, void* scratch, void* stream);
/* miclip_tsne_run (_gradient_descent over _kl_divergence, _t_sne.py): n_steps
 * iterations on y [N, 2] (in/out) with its `update` and `gains` [N, 2] (in/out).
 * g = 4 (exaggeration * sum_j p w (y_i - y_j) - sum_j w^2 (y_i - y_j) / Z), w = 1 /
 * (1 + |y_i - y_j|^2), Z = sum_{i != j} w; gains += 0.2 where update * g < 0, else
 * *= 0.8, clipped at min_gain; update = momentum * update - learning_rate * gains * g;
 * y += update. stats [4] = {KL error (of exaggeration * P), |gains * g|_2, Z, steps
 * done by this call} is written after every error_every-th step, or after the last
 * step only when error_every is 0. Two launches per step, no host synchronisation. */
int miclip_tsne_run(const float* P, int32_t N, float* y, float* update, float* gains,
                    int32_t n_steps, float exaggeration, float momentum, float learning_rate,
                    float min_gain, int32_t error_every, void* scratch, float* stats,
                    void* stream);

/* ---- ProLIP projector training on the pre-projection feature cache, fp32 ----
 * One optimiser step of G configurations (the (lr, lambda) grid of search_lr,
 * or G = 1) per pair of calls. They share x [n, D] (x_dtype MICLIP_F32,
 * MICLIP_FP16 or MICLIP_BF16, widened in the load; 16-byte aligned), labels
 * [n] int64 in [0, C), text_weights [E, C] and P0 [D, E], and differ in
 * P / m / v [G, D, E], lr [G] and lambda [G]. D % 16 == 0, E % 16 == 0,
 * 16 <= D <= 1280, 16 <= E <= 1024, 1 <= C <= 1024, n >= 1, 1 <= G <= 65535;
 * anything else is MICLIP_EINVAL before any launch. All pointers are device
 * memory owned by the caller; both calls are stream-ordered, never synchronise
 * and never allocate. Results are deterministic and a configuration's result
 * does not depend on G or on its index.
 *
 * miclip_prolip_grad replaces the forward and the autograd backward of
 * methods/ProLIP.py:232-234, 244, 248 (:202-204, 214, 218 chunked; :337-340,
 * 351 in search_init_hp): logits = scale * normalize(x @ P_g) @ text_weights,
 * loss1 = cross_entropy(logits, labels), and dZ [G, n, E] = d loss1 / d(x @
 * P_g). partials [G, ceil(n / 16), 2] receives per 16-row tile {sum of the
 * rows' cross-entropy, number of rows with argmax(logits) == label}. */
int miclip_prolip_grad(const void* x, int32_t x_dtype, const int64_t* labels, int32_t n, int32_t D,
                       int32_t E, int32_t C, const float* text_weights, const float* P,
                       int32_t G, float scale, float* dZ, float* partials, void* stream);
/* miclip_prolip_adam replaces the rest of the step, methods/ProLIP.py:243-256
 * (:213-226 chunked; :350-358) with the optimiser of :165-166 (:316-317):
 * dP = x^T dZ_g + 2 (lambda_g / lambda_div) (P_g - P0), never written, then
 * torch.optim.Adam's update (betas 0.9 / 0.999, eps, bias correction by the
 * 1-based `step`, no weight decay) of P_g, m_g, v_g with the rate lr_g *
 * lr_factor; lr_factor is CosineAnnealingLR's 0.5 (1 + cos(pi epoch / T)),
 * lambda_div the chunk count of :193-195 (1 when not chunked).
 * grad_partials: miclip_prolip_grad's partials of the same step; mse_partials:
 * scratch [G, ceil(D / 32) * ceil(E / 32)]; history [G, 3] receives {loss1,
 * loss2 = sum((P_g - P0)^2) before the update, correct count}: what the
 * reference reads back with .item() at :248-252. */
int miclip_prolip_adam(const void* x, int32_t x_dtype, const float* dZ, int32_t n, int32_t D,
                       int32_t E, int32_t G, const float* P0, float* P, float* m, float* v,
                       const float* lr, const float* lambda, float lr_factor, float lambda_div,
                       int32_t step, float eps, const float* grad_partials, float* mse_partials,
                       float* history, void* stream);

/* ---- Tip-Adapter: training-free cache classifier and its (beta, alpha) search, fp32 ----
 * methods/utils.py:23-62 (build_cache_model) and :64-94 (search_hp_tip) on the device.
 * Nq query rows, Nk cache keys, E embedding width, C classes, nb betas, na alphas, A
 * views of width Wv. Limits: 1 <= Nq <= 2^24, 1 <= Nk <= 65536, E % 16 == 0,
 * 16 <= E <= 1024, 1 <= C <= 1024, 1 <= nb, na <= 1024, nb * na <= 65536,
 * 1 <= A <= 1024, Wv % 16 == 0, 16 <= Wv <= 65536, dtypes MICLIP_F32 / MICLIP_FP16 /
 * MICLIP_BF16 (widened exactly in the load), no NULL pointer; anything else is
 * MICLIP_EINVAL with the argument named in miclip_last_error, before any launch. No
 * model handle is needed. All pointers are caller-owned device memory, F, keys, proj and
 * every view 16-byte aligned (checked, except the view pointers: they live in device
 * memory and are trusted), the `views` array 8-byte aligned; the calls are stream-ordered, never synchronise and
 * never allocate. All arithmetic is fp32; there are no float atomics and every float
 * sum has a fixed shape, so results are bit-identical run to run.
 * key_labels [Nk] and labels [Nq] are int32 in [0, C): host callers check that before
 * the call (miclip/tip.py does); the entries trust device labels, and a label outside
 * the range reads or writes nothing out of bounds (such a key belongs to no class,
 * such a row is never counted correct).
 * scratch: miclip_tip_scratch_bytes(Nq, Nk, E, C, nb, na) bytes (0 outside the limits),
 * 16-byte aligned, used by miclip_tip_grid and miclip_tip_logits. */
int64_t miclip_tip_scratch_bytes(int32_t Nq, int32_t Nk, int32_t E, int32_t C, int32_t nb,
                                 int32_t na);
/* miclip_tip_keys replaces methods/utils.py:37-48: views is a DEVICE array of A device
 * pointers to the cached pre-projection views x_v [Nk, Wv] (f{v}.pth), proj [Wv, E]
 * fp32. Per view f_v = F.normalize(x_v @ proj) (eps 1e-12, :38-39); keys [Nk, E] = the
 * mean over the views, summed in ascending v (:47), divided by its row norm (:48). That
 * last step is a plain division as in the reference: a row whose mean is all zero
 * yields a non-finite key. The permute of :49 is left to the caller. */
int miclip_tip_keys(const void* const* views, int32_t view_dtype, int32_t A, int32_t Nk,
                    int32_t Wv, int32_t E, const float* proj, float* keys, void* stream);
/* miclip_tip_affinity replaces methods/utils.py:79: affinity [Nq, Nk] = scale *
 * F [Nq, E] @ keys [Nk, E]^T (scale 1 for the affinity). With keys = clip_weights^T
 * [C, E] and scale 100 it gives the clip_logits of :82. */
int miclip_tip_affinity(const void* F, int32_t f_dtype, const float* keys, int32_t Nq, int32_t Nk,
                        int32_t E, float scale, float* affinity, void* stream);
/* miclip_tip_grid replaces the double loop of methods/utils.py:74-90 (with cls_acc,
 * :16-21) up to the choice of the best pair: correct [nb, na] (int32, overwritten) =
 * the number of rows whose first argmax over c of clip_logits[c] + alphas[ia] *
 * s_c(betas[ib]) equals their label, where s_c(beta) = sum over the keys k with
 * key_labels[k] == c, in ascending k, of exp(-(beta - beta * affinity[k])) -- :81's
 * product with the one-hot cache_values; a class with no key contributes 0. NaN ranks
 * above every number and the lower index wins ties (torch.topk). affinity [Nq, Nk] is
 * miclip_tip_affinity's or a caller's adapter(features) (:76-77); clip_logits [Nq, C];
 * betas [nb], alphas [na] fp32. One exp per (row, key, beta); nothing of size
 * Nq * nb * C is formed. */
int miclip_tip_grid(const float* affinity, const int32_t* key_labels, const float* clip_logits,
                    const int32_t* labels, const float* betas, const float* alphas, int32_t Nq,
                    int32_t Nk, int32_t C, int32_t nb, int32_t na, int32_t* correct,
                    void* scratch, void* stream);
/* miclip_tip_logits replaces methods/utils.py:81-83 for one pair: logits [Nq, C] =
 * clip_logits + alpha * s(beta), bit for bit the numbers miclip_tip_grid compares. */
int miclip_tip_logits(const float* affinity, const int32_t* key_labels, const float* clip_logits,
                      int32_t Nq, int32_t Nk, int32_t C, float beta, float alpha, float* logits,
                      void* scratch, void* stream);

/* ---- Tip-Adapter-F: training the cache keys on cached features, fp32 ----
 * The fine-tuned variant of the cache classifier: the adapter is a bias-free
 * Linear(E, Nk) initialised to the cache keys, adapter(f) = f keys^T, and only keys
 * [Nk, E] train, by AdamW (betas 0.9 / 0.999, decoupled weight decay) under a cosine
 * schedule that the caller folds into lr_factor. G configurations (lr, beta, alpha)
 * train at once on the same batch; a configuration's result depends neither on G nor on
 * its index. Limits: 1 <= n <= 2^24 cached rows, 1 <= b <= 4096 batch rows, 1 <= Nk <=
 * 65536, E % 16 == 0 in [16, 1024], 1 <= C <= 1024, 1 <= G <= 64; step >= 1; lr_factor,
 * weight_decay >= 0 and eps >= 0 finite. lr / betas / alphas [G] are DEVICE fp32 arrays
 * that the host caller checks to be finite (miclip/tip.py does); labels [n] and key_labels
 * [Nk] are DEVICE int32 in [0, C), checked by the host caller as for miclip_tip_grid.
 * No float atomics and a fixed order for every float sum: bit-identical run to run.
 * Nothing allocates or synchronises.
 * scratch: miclip_tipf_scratch_bytes(b, Nk, E, C, G) bytes (0 outside the limits; b is
 * the largest batch of the fit), 256-byte aligned. miclip_tipf_prepare sorts the key
 * labels into it once per fit, before the first step. */
int64_t miclip_tipf_scratch_bytes(int32_t b, int32_t Nk, int32_t E, int32_t C, int32_t G);
int miclip_tipf_prepare(const int32_t* key_labels, int32_t Nk, int32_t C, void* scratch,
                        void* stream);
/* One step on the rows rows_host [b] (a HOST int64 array, every entry checked against
 * [0, n) before any launch and staged through launch arguments: free on return) of F
 * [n, E] (f_dtype MICLIP_F32 / FP16 / BF16), clip_logits [n, C] = 100 F W and labels [n]:
 *   A = F_b keys_g^T, phi = exp(-(beta_g - beta_g A)), S[r, c] = sum of phi[r, k] over the
 *   keys of class c in ascending k, loss = mean CE(clip_logits_b + alpha_g S, y_b),
 *   dkeys = (alpha_g beta_g phi * gm[:, cls(k)])^T F_b with gm = (softmax - onehot) / b,
 *   lr_t = lr[g] * lr_factor; keys *= 1 - lr_t * weight_decay; m, v as torch.optim.AdamW;
 *   keys -= lr_t / (1 - 0.9^step) * m / (sqrt(v) / sqrt(1 - 0.999^step) + eps).
 * keys / m / v [G, Nk, E] are updated in place. history [G, 2] = {mean CE, number of
 * rows whose first argmax is the label} of the batch before the update. grad_out
 * [G, Nk, E] receives dkeys, or is NULL. */
int miclip_tipf_step(const void* F, int32_t f_dtype, int32_t n, const int64_t* rows_host,
                     int32_t b, const int32_t* labels, const float* clip_logits,
                     const int32_t* key_labels, float* keys, float* m, float* v, const float* lr,
                     const float* betas, const float* alphas, int32_t Nk, int32_t E, int32_t C,
                     int32_t G, float lr_factor, float weight_decay, float eps, int32_t step,
                     float* history, float* grad_out, void* scratch, void* stream);
/* The recipe's `if acc > best_acc` on the device. counts [>= epoch + 1, G] int32 holds
 * the correct counts of the epochs so far (row e: epoch e). Where counts[epoch, g] is
 * strictly greater than every earlier row's and than 0, best_keys[g] = keys[g],
 * best_count[g] = counts[epoch, g], best_epoch[g] = epoch; otherwise nothing is written. */
int miclip_tipf_keep_best(const int32_t* counts, int32_t epoch, const float* keys,
                          float* best_keys, int32_t* best_count, int32_t* best_epoch, int32_t Nk,
                          int32_t E, int32_t G, void* stream);

/* ---- fine-tuning of the image tower's tail ----
 * FTOpenCLIP's training step (methods/PEFT_openclip.py:247-274) for
 * unlocked_groups 1 and 2 of lock_image_tower (:196-197): first the op-level
 * pieces, then the trunk / tail entry points. Except miclip_encode_image_trunk
 * they need no model handle; all are stream-ordered, never synchronise, never
 * allocate after the scratch query and use no atomics: every result is
 * bit-identical run to run. All pointers
 * are device memory owned by the caller. Every limit below is checked before
 * any launch: MICLIP_EINVAL with the argument named in miclip_last_error.
 *
 * miclip_op_gemm_tn: G [Nn, K] (fp32) = sum_m A[m, Nn] * X[m, K], A [M, Nn] and
 * X [M, K] row-major in `dtype` (MICLIP_FP16 / MICLIP_BF16), 16-byte aligned,
 * fp32 accumulation: the weight gradient dW = dY^T X that loss.backward()
 * (:273) forms for every Linear. Nn % 16 == 0, K % 16 == 0, 16 <= Nn, K <=
 * 65536, M >= 1 (the row tail is masked). M is split into `slices` slices of
 * `slice_rows` rows (miclip_gemm_tn_plan; a function of (M, Nn, K) only) that
 * are summed in ascending order through `workspace`, miclip_gemm_tn_ws_bytes
 * bytes (0 for an unsupported shape). */
int64_t miclip_gemm_tn_ws_bytes(int32_t M, int32_t Nn, int32_t K);
int miclip_gemm_tn_plan(int32_t M, int32_t Nn, int32_t K, int32_t* slices, int32_t* slice_rows);
int miclip_op_gemm_tn(int32_t dtype, const void* A, const void* X, float* G, int32_t M, int32_t Nn,
                      int32_t K, void* workspace, void* stream);
/* miclip_ft_adam replaces optimizer.step() (:274) of torch.optim.Adam(lr=lr_v)
 * (:233) over one contiguous fp32 block params / grads / m / v of numel
 * elements: betas 0.9 / 0.999, eps, bias correction by the 1-based `step`, no
 * weight decay. lr is the scheduled rate, lr_v * 0.5 (1 + cos(pi epoch / T))
 * under CosineAnnealingLR (:234). numel >= 1, step >= 1, lr >= 0, eps >= 0. */
int miclip_ft_adam(float* params, const float* grads, float* m, float* v, int64_t numel, float lr,
                   int32_t step, float eps, void* stream);
/* miclip_ft_proj_grad replaces :250-251, :262-266 and the backward (:273) for
 * visual.proj: with y [B, W] fp32 the pre-projection features (ln_post of the
 * CLS rows, miclip_encode_image without MICLIP_FLAG_APPLY_PROJ) and proj [W, E]
 * the fp32 master, logits = scale * normalize(y @ proj) @ text_weights ([E, C]),
 * loss = cross_entropy(logits, labels) (mean), dP [W, E] = d loss / d proj.
 * The forward runs in fp32 (as miclip_prolip_grad); the operands of dP = y^T dZ
 * are rounded once (RNE) to compute_dtype, dZ under a power-of-two scale that
 * is undone in fp32. stats [2] receives {sum of the rows' cross-entropy, number
 * of rows with argmax(logits) == label}. labels [B] int64 in [0, C).
 * W % 128 == 0, 128 <= W <= 1280, E % 16 == 0, 16 <= E <= 1024, 1 <= C <=
 * 1024, 1 <= B <= 2^24, compute_dtype MICLIP_FP16 / MICLIP_BF16; scratch is
 * miclip_ft_proj_scratch_bytes bytes (0 outside the limits), 256-byte aligned. */
int64_t miclip_ft_proj_scratch_bytes(int32_t B, int32_t W, int32_t E, int32_t C);
int miclip_ft_proj_grad(const float* y, const int64_t* labels, const float* text_weights,
                        const float* proj, int32_t B, int32_t W, int32_t E, int32_t C,
                        int32_t compute_dtype, float scale, float* dP, void* scratch, float* stats,
                        void* stream);
/* Groups 1 and 2: visual.proj, and visual.transformer.resblocks.{L-1}.* with
 * visual.ln_post.* (counted from the back as open_clip's VisionTransformer.lock;
 * parity with open_clip unpinned).
 *
 * miclip_encode_image_trunk runs encode_image (clip/model.py:216-226) up to, but
 * not including, the last vision block and copies the residual stream [B * N, W]
 * to x_out in the handle's stream type (fp16, or fp32 under MICLIP_OPT_RESID_F32;
 * miclip_model_flags): the frozen part of :250 when lock_image_tower(
 * unlocked_groups <= 2) (:197) holds. One stream; a row depends on its image alone.
 *
 * miclip_ft_layout: element offsets of the 15 trainable tensors in the flat fp32
 * block, in named_parameters order -- the last block's ln_1.weight, ln_1.bias,
 * attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight, attn.out_proj.bias,
 * ln_2.weight, ln_2.bias, mlp.c_fc.weight, mlp.c_fc.bias, mlp.c_proj.weight,
 * mlp.c_proj.bias, then ln_post.weight, ln_post.bias, then proj [W, E] -- and the
 * total in offsets[15].
 *
 * miclip_ft_grad replaces the rest of :250-266 and loss.backward() (:273): the
 * last block on the CLS rows (clip/model.py:183-186, 226-229), ln_post, proj,
 * normalise, scale * f @ text_weights, mean cross-entropy, and the gradients of
 * the unlocked groups into `grads` (same layout; groups = 1 writes proj's slice
 * only). x [B * N, W] is the trunk's output (x_dtype MICLIP_FP16 or MICLIP_F32)
 * and carries no gradient, so the token-row side of the backward is one TN GEMM
 * dQKV^T . xhat. Master parameters and gradients fp32; GEMM operands rounded
 * once (RNE) to compute_dtype, gradient operands under a power-of-two scale;
 * LayerNorm statistics, softmax, activation derivatives, normalise and loss fp32.
 * stats [2] = {sum of the rows' cross-entropy, correct count}; feats (nullable)
 * [B, W] receives ln_post of the CLS rows (the pre-projection features).
 * Limits: those of miclip_ft_proj_grad, 1 <= N <= 768, head_dim 64 or 80 dividing
 * W, act MICLIP_ACT_QUICKGELU / MICLIP_ACT_GELU, groups 1 or 2; scratch is
 * miclip_ft_scratch_bytes bytes (0 outside the limits), 256-byte aligned. */
int miclip_encode_image_trunk(miclip_model* model, const void* images, int32_t image_dtype,
                              int32_t B, void* x_out, void* stream);
int miclip_ft_layout(int32_t W, int32_t E, int64_t* offsets);
int64_t miclip_ft_scratch_bytes(int32_t B, int32_t N, int32_t W, int32_t E, int32_t C,
                                int32_t head_dim);
int miclip_ft_grad(const void* x, int32_t x_dtype, const int64_t* labels,
                   const float* text_weights, const float* params, int32_t B, int32_t N,
                   int32_t W, int32_t E, int32_t C, int32_t head_dim, int32_t act,
                   int32_t compute_dtype, float scale, int32_t groups, float* grads,
                   void* scratch, float* stats, float* feats, void* stream);
/* miclip_ft_grad_rows is miclip_ft_grad on the B images whose token blocks are
 * x_cache[rows[b] * N .. rows[b] * N + N), x_cache [cache_images * N, W] in
 * x_dtype as miclip_encode_image_trunk wrote it: the frozen trunk encoded once
 * per augmentation view (as ProLIP's cache_preprojection_features does for the
 * projector) and every epoch trained from the cached rows. The two reads of x
 * -- ln_1 over the token rows and the CLS residual rows -- go through the row
 * map; no gathered [B * N, W] copy is formed, and grads, stats and feats are
 * bit-identical to miclip_ft_grad on a contiguous copy of those blocks. An
 * image may appear more than once. rows [B] is a HOST array: every index is
 * checked against [0, cache_images) before any launch (MICLIP_EINVAL names
 * `rows`), then staged into the scratch by the launches' own arguments, so the
 * array is free on return, nothing is allocated and the stream is not waited
 * for. Limits: those of miclip_ft_grad, 1 <= cache_images and cache_images * N
 * * W < 2^47; scratch is miclip_ft_rows_scratch_bytes bytes
 * (miclip_ft_scratch_bytes plus the index area; 0 outside the limits), 256-byte
 * aligned. */
int64_t miclip_ft_rows_scratch_bytes(int32_t B, int32_t N, int32_t W, int32_t E, int32_t C,
                                     int32_t head_dim);
int miclip_ft_grad_rows(const void* x_cache, int32_t x_dtype, int64_t cache_images,
                        const int64_t* rows /* HOST [B] */, const int64_t* labels,
                        const float* text_weights, const float* params, int32_t B, int32_t N,
                        int32_t W, int32_t E, int32_t C, int32_t head_dim, int32_t act,
                        int32_t compute_dtype, float scale, int32_t groups, float* grads,
                        void* scratch, float* stats, float* feats, void* stream);

/* ---- validation metrics on features or logits, fp32 ----
 * Replace the body of _run_validation's batch loop (methods/PEFT_openclip.py:
 * 89-117) and the per-batch work of aihab_utils/evaluation.py (cls_acc top-1 /
 * top-3, CrossEntropyLoss, the confusion-matrix / F1 updates, L2MetricsAccumulator
 * .update :186-221, aggregate_logits_to_l2 :92-142, ClassificationTracker
 * .top3_metrics :261-273). They need no model handle, are stream-ordered, never
 * synchronise and never allocate.
 *
 * The state block is caller-owned device memory of miclip_eval_state_bytes(C,
 * num_l2) bytes, 8-byte aligned, read back with one copy. As 8-byte words:
 *   0                    float64  sum over batches of the batch-mean cross-entropy
 *   1                    int64    rows counted
 *   2                    int64    batches
 *   3, 4                 int64    top-1 hits, top-3 hits
 *   5, 6                 int64    L2 top-1 hits, L2 top-min(3, num_l2) hits
 *   7                    int64    rows skipped (label outside [0, C), or NaN logits)
 *   8 ..                 int64    L3 confusion counts [C, C], row = label, column =
 *                                 prediction
 *   8 + C*C ..           int64    L2 confusion counts [num_l2, num_l2]
 * All integer words are exact and do not depend on the order of the batches.
 * miclip_eval_state_bytes returns 0 unless 3 <= C <= 1024 and 1 <= num_l2 <= C
 * (pass num_l2 = 1 when no L2 map is used). miclip_eval_reset zeroes the block. */
int64_t miclip_eval_state_bytes(int32_t C, int32_t num_l2);
int miclip_eval_reset(void* state, int32_t C, int32_t num_l2, void* stream);

enum miclip_eval_l2 {
  MICLIP_EVAL_L2_NONE = 0,      /* no L2 roll-up; l3_to_l2 must be NULL */
  MICLIP_EVAL_L2_ARGMAX = 1,    /* L2 prediction = l3_to_l2[prediction] (mode "argmax") */
  MICLIP_EVAL_L2_SUM = 2,       /* mode "logits", reduce "sum" */
  MICLIP_EVAL_L2_MEAN = 3,      /* reduce "mean": sum / max(group size, 1) */
  MICLIP_EVAL_L2_LOGSUMEXP = 4  /* reduce "logsumexp": running logaddexp from -inf */
};
#define MICLIP_EVAL_LOGITS_IN 1u /* flags: `logits` is read, not computed */

/* One batch. feats [B, E] (f_dtype MICLIP_F32 / MICLIP_FP16 / MICLIP_BF16, widened
 * in the load, 16-byte aligned), text_weights fp32 [E, C], labels int64 [B]:
 *   logits[b, c] = scale * (feats[b] . text_weights[:, c]) / max(|feats[b]|, 1e-12),
 * bitwise the logits of miclip_zero_shot(apply_proj = 0) on the fp32 features.
 * With MICLIP_EVAL_LOGITS_IN in flags the [B, C] `logits` are an input instead
 * (feats, text_weights, E unused): L2MetricsAccumulator.update's and
 * aggregate_logits_to_l2's form. l3_to_l2: HOST int32 [C] (checked, then passed by
 * value with the launch), NULL exactly when l2_mode is MICLIP_EVAL_L2_NONE.
 * Per-row outputs, device memory: row_loss [B] (required) logsumexp(z) - z[label];
 * row_pred [B], row_top3 [B, 3] class indices by value descending, lower index
 * first among equals (torch.topk for distinct values); row_top3_prob [B, 3] their
 * softmax probabilities; l2_pred [B]; l2_top3 [B, 3] (-1 beyond num_l2, and
 * beyond the first in mode argmax); l2_logits [B, num_l2], the aggregated logits,
 * group by group in ascending L3 id. `logits` [B, C] receives the logits when not
 * an input. Every output but row_loss may be NULL.
 * E % 16 == 0, 16 <= E <= 1024, 3 <= C <= 1024, 1 <= num_l2 <= C, every l3_to_l2
 * entry in [0, num_l2), B >= 1: anything else is MICLIP_EINVAL before any launch.
 * A row whose label is outside [0, C) is skipped by every accumulator (word 7
 * counts it) and its row_loss is 0; nothing is indexed with it. */
int miclip_eval_batch(const void* feats, int32_t f_dtype, const float* text_weights,
                      const int64_t* labels, int32_t B, int32_t E, int32_t C, float scale,
                      const int32_t* l3_to_l2, int32_t num_l2, int32_t l2_mode, uint32_t flags,
                      void* state, float* logits, float* row_loss, int32_t* row_pred,
                      int32_t* row_top3, float* row_top3_prob, int32_t* l2_pred,
                      int32_t* l2_top3, float* l2_logits, void* stream);

/* Batch split of encode_image over the caller's stream and one handle-owned
 * stream (fork/join by events, so the call stays stream-ordered and
 * graph-capturable): 1 = off, 2..4 = that many parts (default 2; a part is
 * never smaller than 16 images). */
int miclip_set_splits(miclip_model* m, int32_t splits);
/* Parts encode_image splits a batch of B images into (>= 1): at most the
 * miclip_set_splits value, no part below 16 images or 16384 token rows. */
int miclip_image_splits(const miclip_model* m, int32_t B);

/* Diagnostics (no reference counterpart; SURVEY §8d measurement): n_wg one-wave
 * workgroups each write {XCD id (HW_REG_XCC_ID), s_memtime (shader-clock
 * counter), s_memrealtime (100 MHz), 0} as 4 uint64 to device out[4*i..].
 * Launched before and after a timed region on its stream, the per-XCD ratio of
 * the two counters' deltas is the core clock the chip held over that region. */
int miclip_clock_probe(uint64_t* out, int32_t n_wg, void* stream);

void miclip_model_destroy(miclip_model* m);
const char* miclip_last_error(void);
int miclip_abi_version(void);
/* Device-memory bytes currently held by the handle (weights + workspaces). */
int64_t miclip_model_bytes(const miclip_model* m);
/* Numerics path the handle runs (from miclip_config.options and the dtype):
 * MICLIP_MODEL_RESID16 fp16 residual stream, MICLIP_MODEL_LNFOLD ln_1 / ln_2 folded
 * into the vision tower's QKV / c_fc GEMMs (MICLIP_MODEL_LNFOLD_TEXT: the text
 * tower's; MX-fp8 models fold the text tower only), MICLIP_MODEL_MXFP8 MX-fp8 GEMM
 * operands (vision tower),
 * MICLIP_MODEL_CLS_LAST last vision block on the CLS rows, MICLIP_MODEL_MX_OUT MX-fp8
 * vision out-projection, MICLIP_MODEL_MX_GELU_TANH tanh-form GELU in the MX c_fc
 * epilogue. 0 for NULL. */
#define MICLIP_MODEL_RESID16 1
#define MICLIP_MODEL_LNFOLD 2
#define MICLIP_MODEL_MXFP8 4
#define MICLIP_MODEL_CLS_LAST 8
#define MICLIP_MODEL_MX_OUT 16
#define MICLIP_MODEL_MX_GELU_TANH 32
#define MICLIP_MODEL_LNFOLD_TEXT 64
int miclip_model_flags(const miclip_model* m);
/* Diagnostics: the GEMM kernel of the block launches (>= 256 rows) --
 * which 0: the folded-LN store GEMMs (QKV, c_fc), 1: the fp16 residual GEMMs
 * (out-proj, c_proj); variant 0 (default) / 259 (the 8-wave persistent kernel);
 * which 2: the MX-fp8 GEMMs (variants of miclip_op_gemm_mx_v). All are
 * bit-identical, so results never change;
 * bench.py --ab-gemm times them in one process. */
int miclip_set_gemm_variant(miclip_model* m, int32_t which, int32_t variant);
/* Switches a run-time option of a handle (only MICLIP_OPT_FULL_LAST_BLOCK; the
 * others fix the weight layout at create and return MICLIP_EINVAL). */
int miclip_model_set_option(miclip_model* m, uint32_t option, int32_t on);

/* ---- diagnostics: per-kernel-class timing with HIP events ---- */

/* Algorithmic totals of one kernel class since the last reset. `flops` counts
 * 2*M*N*K per GEMM and 4*N^2*dh per attention head; `bytes` is the minimum HBM
 * traffic (operands read once, outputs written once). */
typedef struct miclip_kernel_stat {
  const char* name;
  int64_t launches;
  double ms;
  double flops;
  double bytes;
} miclip_kernel_stat;

/* When enabled, every launch of later encode calls is bracketed by hipEvents on
 * the caller's stream (adds a few us per launch: use outside timed regions). */
int miclip_set_profiling(miclip_model* m, int enable);
/* Synchronises on the recorded events, folds them into per-class totals and
 * copies up to n classes into out; returns the number of classes. */
int miclip_profile_read(miclip_model* m, miclip_kernel_stat* out, int32_t n, int32_t reset);

/* ---- op-level entry points (kernel parity tests and micro-benchmarks) ---- */

/* C = A[M,K] . W[N,K]^T + bias, A/W in compute dtype `dtype`.
 * epi 0: C dtype = act(.) with act from `act` (0 none); epi 1: C fp32 += (residual);
 * epi 2: C fp32 = . ; epi 3: no output (diagnostic: prices the epilogue);
 * epi 4: C fp16 += . (fp16 residual stream; dtype MICLIP_FP16 only).
 * N % 128 == 0 and K % 64 == 0 required. variant: 0 = tile
 * chosen by size, 128 / 256 = force the 128x128 / 256x256 kernel (N % 256 for 256);
 * 259 = the persistent 256-row-tile kernel; 192 / 129 / 130 = its 192-row tiles /
 * 128-row tiles / 128-row tiles + row tail (epi 0 and 4 only; N % 256, K >= 128).
 * 259 / 192 / 129 / 130 give bit-identical results (same k order and epilogue per row).
 * Replaces torch Linear (clip/model.py:171-175) and MHA in/out projections. */
int miclip_op_gemm(int32_t dtype, const void* A, const void* W, const float* bias, void* C,
                   int32_t M, int32_t N, int32_t K, int32_t epi, int32_t act, int32_t variant,
                   void* stream);
/* The launch that miclip_op_gemm / _gemm_ln / _gemm_splitk / _gemm_patch would make for
 * this shape, launching nothing (host only; no reference counterpart). epi: the codes
 * above, 5 = the folded-LN store, 6 = the patch-embed epilogue; variant as there; sk <= 1:
 * no split-K; ncu: the CU count to plan for, 0 = this device's (the only case that
 * touches HIP). out = {kernel, grid, block, gm, ntm_dp, wgs, wide, 0}: workgroups,
 * threads per workgroup and the kernel's tile-row group, tile-rows kept in tiles,
 * row-tail tasks and tail flags (0 where the kernel takes none). kernel:
 *   0 split-K pair (grid x sk workgroups, then the reduction)   1 gemm_nt_kernel 128x128
 *   2 / 3 / 4 gemm256_kernel SCHED 0 / 1 / 2   5 gemm256_kernel SCHED 2, register epilogue
 *   6 gemm256p_kernel   7 gemm256s_kernel, 256-row tiles   8 the same with the fp32
 *   row-staging epilogue   9 / 10 gemm256s_kernel, 192- / 128-row tiles
 * MICLIP_EINVAL where the launcher refuses (csrc/gemm_plan.h plan_gemm) or out is NULL. */
int miclip_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t variant, int32_t sk,
                     int32_t ncu, int32_t out[8]);

/* Folded LayerNorm (ln_1 -> QKV, ln_2 -> c_fc of ResidualAttentionBlock,
 * clip/model.py:184-185): LN(x) . W^T + b computed as rs * (x . Wf^T - mean * colsum) + c
 * with rs = rstd / S.
 * miclip_op_ln_fold: Wf = W diag(gamma) * S (dtype), colsum = row sums of Wf, c = bias + W beta
 *   (W [N, K] dtype; gamma, beta [K], bias [N] fp32, bias may be null). S is the power of
 *   two that puts max|W gamma| S in [2^14, 2^15], so a small gamma never rounds W gamma into
 *   the fp16 subnormals; inv_scale: device float[2] ([0] receives 1/S, [1] is scratch), or
 *   NULL for S = 1.
 * miclip_op_ln_stats: stats[r] = {mean, rstd * *rscale} (fp32 pairs) of the fp16 rows
 *   x [R, D]; rscale = the fold's inv_scale (device), or NULL for 1.
 * miclip_op_gemm_ln: C [M, N] (dtype) = act(rs * (A . Wf^T - mean * colsum) + c), A [M, K]
 *   the un-normalised rows (act as miclip_op_gemm; variant as there). */
/* The split-K GEMM of the CLS-only last vision block (gemm_nt_splitk_kernel +
 * splitk_reduce_kernel), op level: sk K slices (K % (64 sk) == 0) summed in
 * ascending order through ws (device fp32, >= sk * M * N floats), then the epilogue.
 * epi 0: C dtype = act(. + bias); 1: C fp32 += . + bias; 4: C fp16 += . + bias (the
 * fp16 residual stream); 5: the folded-LN store of miclip_op_gemm_ln (c, colsum,
 * stats; act). N % 128 == 0. Replaces the CLS rows' Linear calls (clip/model.py:
 * 171-175, 179-181 on ln_post's rows, :226-229). */
int miclip_op_gemm_splitk(int32_t dtype, const void* A, const void* W, const float* bias,
                          const float* c, const float* colsum, const float* stats, void* C,
                          int32_t M, int32_t N, int32_t K, int32_t epi, int32_t act, int32_t sk,
                          float* ws, void* stream);
int miclip_op_ln_stats(const void* x, float* stats, int32_t R, int32_t D, const float* rscale,
                       void* stream);
int miclip_op_ln_fold(int32_t dtype, const void* W, const float* gamma, const float* beta,
                      const float* bias, void* Wf, float* colsum, float* c, int32_t N, int32_t K,
                      float* inv_scale, void* stream);
int miclip_op_gemm_ln(int32_t dtype, const void* A, const void* Wf, const float* c,
                      const float* colsum, const float* stats, void* C, int32_t M, int32_t N,
                      int32_t K, int32_t act, int32_t variant, void* stream);

/* LayerNorm over R rows of width D (eps 1e-5, fp32 statistics); replaces the
 * reference LayerNorm (clip/model.py:151-157). flags bit 0: out fp32 (else compute
 * dtype); bit 1: in fp16 (the fp16 residual stream; dtype MICLIP_FP16 only), else fp32. */
int miclip_op_layernorm(int32_t dtype, const void* in, const float* gamma, const float* beta,
                        void* out, int32_t flags, int32_t R, int32_t D, void* stream);
/* miclip_op_layernorm over gathered rows: output row r normalises input row rows[r]
 * (device int32 [R]; repeats and any order allowed), or row r * in_stride_rows when rows
 * is NULL (in_stride_rows >= 1): ln_post on the CLS rows (stride ntok), ln_final on the
 * EOT rows (clip/model.py:226-229, :349-354). flags bits 0 and 1 as above; bit 2:
 * L2-normalise each output row after the affine (F.normalize, eps 1e-12: the feature
 * cache's fused normalisation). D % 256 == 0, D <= 1536. */
int miclip_op_layernorm_rows(int32_t dtype, const void* in, const int32_t* rows,
                             int32_t in_stride_rows, const float* gamma, const float* beta,
                             void* out, int32_t flags, int32_t R, int32_t D, void* stream);

/* The patch embedding's GEMM (EpiPatch): row m = b * np + p of A[M,K] . W[N,K]^T goes to
 * token row b * (np + 1) + 1 + p of X [B * (np + 1), N] plus positional row pos[1 + p]
 * (pos fp32 [np + 1, N]); X fp32, or fp16 when resid16 (one RNE of the fp32 sum). M % np
 * == 0; shapes as miclip_op_gemm. variant 0 = by size (the model's call), 128 / 256..258,
 * 260 = force the 128x128 / one-tile 256x256 kernels. Replaces conv1 + the positional add
 * (clip/model.py:216-222). Row b * (np + 1) of X is left to miclip_op_class_token. */
int miclip_op_gemm_patch(int32_t dtype, const void* A, const void* W, const float* pos, void* X,
                         int32_t M, int32_t N, int32_t K, int32_t np, int32_t resid16,
                         int32_t variant, void* stream);
/* X[b * ntok, :] = cls + pos[0, :] for b < B (cls, pos fp32 [D]; X fp32, or fp16 when
 * resid16): the class-embedding row (clip/model.py:220-221). */
int miclip_op_class_token(const float* cls, const float* pos, void* X, int32_t B, int32_t ntok,
                          int32_t D, int32_t resid16, void* stream);

/* softmax(Q K^T / sqrt(dh) + mask) V per head over a packed qkv [B*N, 3*H*dh]
 * buffer, out [B*N, H*dh]; replaces F.scaled_dot_product_attention inside
 * nn.MultiheadAttention (clip/model.py:179-181), causal = text mask (323-329).
 * head_dim dh: 64, or 80 (open_clip ViT-H/14 vision tower); 0 means 64.
 * variant (dh 64): 0 = default (two workgroups per CU at N = 256..259, else the
 * pipelined multi-head kernel for N <= 320, else one head per workgroup), 1 = one
 * head per workgroup, 2 = pipelined, 4 = pipelined with the last-chunk split,
 * 8 = two workgroups per CU, 10..16 = one head per workgroup on that many waves.
 * variant (dh 80): 0 = default (6 at N = 256..259, else 2 where it applies, else
 * 1), 1 = one head per workgroup (N <= 416), 2 = two-phase fetch (N = 160..288),
 * 6 = pipelined half-head K/V ring (N = 256..259). A variant outside its range
 * fails (never silently replaced). */
int miclip_op_attention(int32_t dtype, const void* qkv, void* out, int32_t B, int32_t N,
                        int32_t H, int32_t head_dim, int32_t causal, int32_t variant,
                        void* stream);

/* conv1 patchify as the patch GEMM's A operand (clip/model.py:217-219): images
 * [B, 3, R, R] (image_dtype MICLIP_F32 / FP16 / BF16) -> patches [B*(R/P)^2, Kp]
 * (dtype FP16 / BF16), column c*P*P + ky*P + kx, zero up to Kp (>= 3*P*P). variant 0 =
 * default (one workgroup per band of R/P patches -- 16-B vector loads and stores -- where
 * R % 4 == 0, Kp % 4 == 0 and `images` and `patches` are 16-byte aligned, else 1), 1 = one
 * workgroup per patch (element accesses, no alignment requirement). Bit-identical. The
 * encode entry points take any alignment the same way. */
int miclip_op_im2col(int32_t dtype, int32_t image_dtype, const void* images, void* patches,
                     int32_t B, int32_t R, int32_t P, int32_t Kp, int32_t variant, void* stream);

/* Attention of the first query (token row 0, CLS) of every image only, same qkv
 * layout as miclip_op_attention; out [B, H*dh] compact (row b = image b's CLS
 * row). The vision tower's last block (only its CLS rows reach ln_post,
 * clip/model.py:226-229). N <= 768, dh 64 or 80 (0 = 64), non-causal. */
int miclip_op_attention_q0(int32_t dtype, const void* qkv, void* out, int32_t B, int32_t N,
                           int32_t H, int32_t head_dim, void* stream);

/* ---- MX-fp8 operands (MICLIP_MXFP8; no reference counterpart: C5 stretch) ----
 * An MX-fp8 [rows, K] operand is e4m3 bytes [rows, K] plus a tiled E8M0 scale
 * plane of miclip_mx_scale_bytes(rows, K) bytes (one scale per 32 consecutive k). */
int64_t miclip_mx_scale_bytes(int32_t rows, int32_t K);
/* rows [R, K] (in_f16: 0 fp32, 1 fp16, 2 fp16 through the older 8-lane-block
 * kernel -- byte-identical, kept for that test; K % 256 == 0) -> q [R, K] + scales */
int miclip_op_quant_mx(const void* in, int32_t in_f16, int32_t R, int32_t K, void* q, void* scales,
                       void* stream);
/* C = A . W^T on MX-fp8 operands (N % 256 == 0, K % 128 == 0). epi 0: C fp16 =
 * act(. + bias); epi 1: C fp16 += . + bias; epi 5: C MX-fp8 (+ CS scales) = MX(act(. + bias)). */
int miclip_op_gemm_mx(const void* A, const void* SA, const void* W, const void* SW,
                      const float* bias, void* C, void* CS, int32_t M, int32_t N, int32_t K,
                      int32_t epi, int32_t act, void* stream);
/* miclip_op_gemm_mx with the kernel named: variant 0 default (persistent where K >=
 * 256), 1 one 256x256 tile per workgroup, 2 persistent (MICLIP_EINVAL where it does
 * not apply). Bit-identical outputs (A/B and tests). */
int miclip_op_gemm_mx_v(const void* A, const void* SA, const void* W, const void* SW,
                        const float* bias, void* C, void* CS, int32_t M, int32_t N, int32_t K,
                        int32_t epi, int32_t act, int32_t variant, void* stream);
/* LayerNorm (fp32 in, or fp16 if in_f16) -> MX-fp8 rows q [R, D] + scales */
int miclip_op_layernorm_mx(const void* in, int32_t in_f16, const float* gamma, const float* beta,
                           void* q, void* scales, int32_t R, int32_t D, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MICLIP_H_ */

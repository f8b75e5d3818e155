/*
 * skeldiff.h — C ABI of libskeldiff.so, the MI355X (gfx950) sampling engine for the
 * SkeletonDiffusion hot path: NonisotropicGaussianDiffusion.sample().
 *
 * Boundary rules: plain pointers and sizes, no torch types.  Tensors are row-major fp32,
 * contiguous, in device memory (HBM) unless stated; `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Every function returns 0 on success and a negative
 * SD_E* code on error; sd_last_error() returns a thread-local message for the last failure.
 * No C++ exception crosses the ABI.  A plan is immutable after sd_plan_finalize() and may be
 * shared by several streams; a workspace belongs to one stream at a time.
 *
 * Which reference interface each entry point replaces (paths relative to the reference
 * tree, tum-vision/skeletondiffusion):
 *   sd_plan_create / sd_plan_set_tensor / sd_plan_finalize
 *       -> module construction + strict load_state_dict of the diffusion and Denoiser
 *          (src/core/diffusion_manager.py:16-27, src/eval_prepare_model.py:69-72,
 *           src/core/diffusion/nonisotropic.py:72-127, src/core/network/nn/generator.py:8-84).
 *          Tensors are handed over by their reference state_dict key.
 *   sd_denoiser_forward
 *       -> Denoiser.forward (src/core/network/nn/generator.py:86-107) as called by
 *          LatentDiffusion.feed_model (src/core/diffusion/base.py:243-255).
 *   sd_p_sample_update
 *       -> q_posterior + p_combine_mean_var_noise of one reverse step
 *          (src/core/diffusion/base.py:314-341, src/core/diffusion/nonisotropic.py:196-210;
 *           isotropic.py:85-95 for IsotropicGaussianDiffusion), x0 clamp included.
 *   sd_sample_loop
 *       -> LatentDiffusion.p_sample_loop / sample (src/core/diffusion/base.py:343-390,
 *          439-443).
 *   sd_noise_fill
 *       -> the white-noise draws get_noise/randn (src/core/diffusion/base.py:151-158,351),
 *          replaced by counter-based Philox4x32-10 keyed by (seed, global row, step) so that
 *          results do not depend on batch split or GPU count.
 */
#ifndef SKELDIFF_H
#define SKELDIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history: 1 (rounds 1-3); 2 (round 5) -- sd_mahalanobis_loss_forward / _backward take T,
 * sd_set_kernel_variant / sd_set_row_chains / sd_set_update_kernel / sd_set_v5_mix removed
 * (per-plan options instead), sd_test_set_split_route and sd_plan_desc::objective added;
 * 3 (round 6) -- SD_FLAG_NO_CLIP (p_sample's clip_denoised = False), sd_p_sample_update takes
 * flags, the measured-slower kernel forms and option values removed; 4 (round 6) --
 * sd_plan_desc::norm_type (Block LayerNorm over the node axis).  Bindings check it at load. */
#define SD_ABI_VERSION 4

enum {
    SD_OK = 0,
    SD_E_INVALID = -1,   /* bad argument / shape / unsupported configuration */
    SD_E_STATE = -2,     /* plan not finalized, tensor missing, ... */
    SD_E_HIP = -3,       /* HIP runtime error */
    SD_E_NOMEM = -4,
    SD_E_INTERNAL = -5
};

/* flags for sd_sample_loop */
enum {
    SD_FLAG_GRAPH = 1,          /* capture the whole T-step chain in a hipGraph, cache, replay */
    SD_FLAG_DEVICE_START = 2,   /* x_T drawn on device (Philox, step index T) instead of x_T arg */
    SD_FLAG_DEVICE_NOISE = 4,   /* per-step noise drawn on device instead of eps_all */
    SD_FLAG_NO_CLIP = 8         /* x0 is not clamped to [-1, 1] (p_sample / p_mean_variance with
                                   clip_denoised = False, base.py:314-328; the flag also applies to
                                   sd_p_sample_update) */
};

typedef struct sd_plan sd_plan;

typedef struct sd_plan_desc {
    int32_t num_nodes;        /* J = channels = num_nodes (<= 64) */
    int32_t latent_dim;       /* Denoiser `dim` = diffusion latent_size (seq_length) */
    int32_t cond_dim;         /* 0, or latent_dim when diffusion_conditioning */
    int32_t out_dim;          /* Denoiser out_dim (== latent_dim for sampling) */
    int32_t depth;
    int32_t attn_heads;
    int32_t attn_dim_head;
    int32_t use_attention;    /* 1: Attention blocks, 0: Residual(PreNorm(StaticGraphLinear)) */
    int32_t self_condition;   /* must be 0 (no release config uses it) */
    int32_t learn_influence;  /* 1: G-hat = row-L1-normalised G (graph_structural.py:31-32) */
    int32_t num_node_types;   /* 0: shared weights (no node_types); else types in node_types */
    const int64_t* node_types;/* host array[J] (ignored when num_node_types == 0) */
    int32_t timesteps;        /* T */
    int32_t isotropic;        /* 1: IsotropicGaussianDiffusion posterior (scalar coefficients) */
    int32_t activation;       /* diffusion_activation: 0 identity, 1 tanh */
    float sinusoidal_theta;   /* SinusoidalPosEmb theta (10000) */
    int32_t objective;        /* 0 pred_x0 (release configs); isotropic only: 1 pred_noise, 2 pred_v
                                 (x0 = a[t] x_t - b[t] act(model_out): isotropic.py:48-70) */
    int32_t norm_type;        /* ResnetBlock Block.norm (attention.py:49-60): 0 'none' (release configs),
                                 1 'layer' = LayerNorm over the node axis (attention.py:19-28; J = 16, 17
                                 or 21, v4 kernels; tensors "...blockN.norm.norm.weight/bias") -- ABI 4 */
} sd_plan_desc;

int32_t sd_abi_version(void);
const char* sd_last_error(void);
/* How the device code was built: "no-packed-fp32" for the product build (skeletondiffusion_amd/
 * build.py compiles every kernel without packed-FP32 instructions, DESIGN.md §4c, and checks the
 * linked code objects); the Python binding refuses to load a library that says otherwise. */
const char* sd_build_info(void);

int sd_plan_create(sd_plan** out, const sd_plan_desc* desc);
void sd_plan_destroy(sd_plan* plan);

/* The tensors a plan requires, in reference state_dict key order ("model.init_lin.weight",
 * ..., "posterior_mean_coef1_x0", ...). */
int32_t sd_plan_num_tensors(const sd_plan* plan);
const char* sd_plan_tensor_name(const sd_plan* plan, int32_t index);
int64_t sd_plan_tensor_numel(const sd_plan* plan, int32_t index);

/* Copy one tensor (fp32, contiguous, host or device pointer) into the plan. */
int sd_plan_set_tensor(sd_plan* plan, const char* name, const float* data, int64_t numel,
                       void* stream);
/* Pack weights (G-hat, RMSNorm gain folding, time/FiLM tables, posterior tables). */
int sd_plan_finalize(sd_plan* plan, void* stream);

/* dims_out[4] = {J (num_nodes), D (latent_dim), T (timesteps), cond_dim} of the plan (host-side
 * shape validation at the boundary, e.g. the skeldiff::sample_loop torch op). */
int sd_plan_dims(const sd_plan* plan, int32_t* dims_out);

/* Bytes of device workspace needed for `rows` latent rows. */
size_t sd_workspace_bytes(const sd_plan* plan, int64_t rows);

/* x0_out(B,J,out_dim) = Denoiser(x_t(B,J,D), t, x_cond).  x_cond: (B / cond_repeat, J, cond_dim)
 * with row b reading x_cond row b / cond_repeat (the repeat_interleave of base.py:246-248), or
 * NULL when cond_dim == 0. */
int sd_denoiser_forward(const sd_plan* plan, const float* x_t, const float* x_cond,
                        int64_t cond_repeat, int32_t t, float* x0_out, int64_t rows,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Status of the last sd_sample_loop / sd_denoiser_forward / sd_denoiser_trace on `workspace`
 * (synchronises `stream`): flags bit 0 (SD_STATUS_F16_RANGE) = an activation reached |x| >= 65504,
 * outside the f16 range of the split-f16 (v4) products; informational: every f16-product kernel
 * (the split routes' GEMM phases and, since ABI 3, the one-kernel tiles) recomputed the waves'
 * tiles that left the range on exact-f32 MFMA, so f32 mode stays f32-accurate for any finite
 * input.  The word is cleared at the start of each of those calls.  (Bit 1, the round-5 fused
 * layer kernel's timeout, went with that kernel in ABI 3.) */
enum { SD_STATUS_F16_RANGE = 1 };
int sd_workspace_status(const sd_plan* plan, const void* workspace, size_t workspace_bytes, uint32_t* flags,
                        void* stream);

/* sd_denoiser_forward that also copies every block output (rows, J, D + cond_dim), row-major,
 * into acts[0 .. 2 + 4 * depth): init_lin, then per layer i < 2 * depth the ResnetBlock output and
 * the Residual(PreNorm(Attention)) output (nn.Identity for the last layer: a copy of the
 * ResnetBlock output), then final_res_block -- the module outputs of generator.py:94-106 (test
 * hook: the per-layer parity against the reference's forward hooks). */
int sd_denoiser_trace(const sd_plan* plan, const float* x_t, const float* x_cond, int64_t cond_repeat,
                      int32_t t, float* x0_out, int64_t rows, void* workspace, size_t workspace_bytes,
                      float* const* acts, int32_t nacts, void* stream);

/* One reverse step for B rows at time t:
 *   x0 = clamp(act(x0_raw), -1, 1) (no clamp with SD_FLAG_NO_CLIP in flags); mean = C1[t] x0 + C2[t] x_t;
 *   x_prev = mean + U (sigma_t * eps)   (nonisotropic)   |  c1 x0 + c2 x_t + sigma_t eps (iso)
 * eps: (B, J, D) rows `eps_row_stride` floats apart, or NULL for device Philox noise
 * (seed, global row row0 + b, step t).  t == 0 adds no noise.  mean_out / noise_out are
 * optional (NULL) extra outputs with their own row strides (return_sampling_noise). */
int sd_p_sample_update(const sd_plan* plan, const float* x0_raw, const float* x_t,
                       const float* eps, int64_t eps_row_stride, uint64_t seed, int64_t row0,
                       int32_t t, float* x_prev, float* mean_out, int64_t mean_row_stride,
                       float* noise_out, int64_t noise_row_stride, int64_t rows, int32_t flags,
                       void* stream);

/* The full reverse chain t = T-1 .. 0 (base.py:365-367).
 *   x_T     : (B,J,D) start noise, or ignored with SD_FLAG_DEVICE_START
 *   eps_all : (B, T-1, J, D) sampling noise in the reference layout (step t reads
 *             eps_all[:, T-1-t]), or ignored with SD_FLAG_DEVICE_NOISE
 *   out     : (B,J,D) final latents
 *   means_out / noise_out / timages_out : optional (B, T-1, J, D) records of mean_t,
 *             the noise used and x_t for t = T-1..1 (return_sampling_noise / return_timages)
 *   start_out: optional (B,J,D) copy of the start noise used */
int sd_sample_loop(const sd_plan* plan, const float* x_T, const float* x_cond,
                   int64_t cond_repeat, const float* eps_all, uint64_t seed, int64_t row0,
                   float* out, float* means_out, float* noise_out, float* timages_out,
                   float* start_out, int64_t rows, void* workspace, size_t workspace_bytes,
                   int32_t flags, void* stream);

/* Fill out(B, n_per_row) with the device normals of (seed, rows row0.., step). n_per_row % 4 == 0. */
int sd_noise_fill(float* out, int64_t rows, int64_t n_per_row, uint64_t seed, int64_t row0,
                  int32_t step, void* stream);
/* Raw Philox4x32-10 words for tests: out[4*i .. 4*i+3] = philox(ctr = (i % quads, step,
 * row lo, row hi) with row = row0 + i / quads, key = seed). */
int sd_philox_raw(uint32_t* out, int64_t rows, int64_t quads, uint64_t seed, int64_t row0,
                  int32_t step, void* stream);

/* Row-chain boundaries of sd_sample_loop (host arithmetic, no device): the first row of chain i
 * of `nchains` over `rows` rows; i >= nchains gives `rows`.  unit <= 32: cuts on 32-row blocks,
 * chain i starting at ceil(rows / 32) * i / nchains * 32.  A larger unit (a multiple of 32) cuts
 * on that many rows instead where every chain then keeps at least 512 rows, and on 32 otherwise.
 * sd_sample_loop passes sd_chain_tile_unit() -- the tiled GEMM phase's row group -- when the call
 * takes the tiled split route on more than one chain, and 32 everywhere else. */
int64_t sd_chain_start(int64_t rows, int32_t nchains, int64_t unit, int32_t i);
int64_t sd_chain_tile_unit(void);

/* Number of kernel launches one reverse step (denoiser + update) issues. */
int32_t sd_plan_kernels_per_step(const sd_plan* plan);

/* Algorithmic FLOPs of one reverse step over `rows` rows, from the plan's own layer list:
 * flops_out[0] graph-linear GEMMs + G-hat mixing, [1] attention QK^T + PV, [2] posterior update. */
int sd_plan_step_flops(const sd_plan* plan, int64_t rows, double* flops_out);

/* Measurement hook: run one reverse step at time t `reps` times with HIP events recorded on
 * `stream` around every kernel.  ms_out[4] = mean ms per step in graph-linear, attention and
 * update kernels, and first-to-last event of the step; counts_out[3] (nullable) = launches per
 * step per class.  Device noise is used for the update. */
int sd_profile_step(const sd_plan* plan, const float* x_t, const float* x_cond, int64_t cond_repeat,
                    int32_t t, int64_t rows, void* workspace, size_t workspace_bytes, int32_t reps,
                    float* ms_out, int32_t* counts_out, void* stream);

/* Evaluation metrics on device, one workgroup per sequence, deterministic
 * fixed-order reductions, caller-owned device buffers, up to 64 samples per sequence.
 * sd_pairwise_distances: x (nseq, samples, features) -> per sequence the mean over sample pairs
 *   i < j of the L1 distance (l1_mean: the reference's lat_apd, src/metrics/multimodal.py:137-151)
 *   and of the L2 distance (l2_mean: apd, multimodal.py:15-35); either output may be NULL.
 * sd_ade_fde: pred (nseq, samples, frames, features), target (nseq, frames, features) -> per
 *   sequence min over samples of the mean-over-frames L2 distance (ade, multimodal.py:44-57) and
 *   of the last frame's distance (fde, :60-73); per_sample_* (nseq, samples) receive the
 *   distances before the minimum (reduction != 'mean'); any output may be NULL.  The minimum is
 *   torch.min's: NaN if one sample's distance is NaN (a diverged sample is reported, not skipped);
 *   a +Inf distance loses to any number. */
int sd_pairwise_distances(const float* x, int64_t nseq, int32_t samples, int64_t features, float* l1_mean,
                          float* l2_mean, void* stream);
int sd_ade_fde(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames,
               int64_t features, float* ade, float* fde, float* per_sample_ade, float* per_sample_fde, void* stream);
/* Multimodal ADE / FDE (src/metrics/multimodal.py:108-135): sequence i has the ground truths
 * gts[seq_offsets[i] .. seq_offsets[i+1]) (each (frames, features); pair_seq[p] = the sequence
 * of ground truth p, npairs = seq_offsets[nseq]); per pair the min over samples of the ADE /
 * FDE against that ground truth (pair_ade / pair_fde, npairs each), then per sequence their
 * mean (mmade / mmfde, nseq; NaN for a sequence without ground truths, as the reference's
 * mean of an empty tensor).  pred (nseq, samples, frames, features).  seq_offsets and
 * pair_seq are device int64 arrays.  The minimum over samples is sd_ade_fde's (NaN if one
 * sample's distance is NaN), and a sequence's mean is NaN if one of its pairs is. */
int sd_mm_ade_fde(const float* pred, const float* gts, const int64_t* pair_seq, int64_t npairs,
                  const int64_t* seq_offsets, int64_t nseq, int32_t samples, int32_t frames, int64_t features,
                  float* pair_ade, float* pair_fde, float* mmade, float* mmfde, void* stream);

/* Best-of-k training relaxation (reference src/core/trainer.py:182-222,
 * Trainer.loss -> to_comparison_space_train -> get_ksimilarity_loss with train_pick_best_sample_among_k
 * = k): the diffusion loss of nseq sequences x k samples (nseq, k) (p_losses with n_train_samples = k,
 * base.py:262-300) and a similarity (nseq, k) -- the loss itself in the latent space (sim = NULL),
 * sd_pose_loss of the decoded samples in the input space, the per-sample ADE (sd_ade_fde
 * per_sample_ade) in the metric space.
 * sd_best_of_k: idx_out (nseq) int64 = per sequence the index of the smallest similarity
 *   (torch.min(dim).indices: the first minimum; the first NaN if any), loss_out (nseq) = the loss at
 *   that index (torch.gather).  Either output may be NULL.
 * sd_best_of_k_backward: dloss (nseq, k) = dloss_sel at the selected index, 0 elsewhere.
 * sd_pose_loss: AutoEncoder.loss(pred, y, reduction='none') (src/core/network/nn/autoencoder.py:80-98)
 *   per sample: mean over frames and joints of the sum over coordinates of |d| (mse = 0) or d^2 (mse
 *   = 1); pred (nseq, samples, frames, joints, dims), target (nseq, frames, joints, dims) ->
 *   per_sample (nseq, samples). */
int sd_best_of_k(const float* sim, const float* loss, int64_t nseq, int32_t k, int64_t* idx_out, float* loss_out,
                 void* stream);
int sd_best_of_k_backward(const float* dloss_sel, const int64_t* idx, int64_t nseq, int32_t k, float* dloss,
                          void* stream);
int sd_pose_loss(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames,
                 int32_t joints, int32_t dims, int32_t mse, float* per_sample, void* stream);

/* Best-sample selection (reference src/metrics/utils.py:12-30 choose_best_sample / get_best_sample_idx,
 * src/metrics/multimodal.py:37-42 mpjpe, src/eval_utils.py:59-62 the long-term rollout's pick):
 * pred (nseq, samples, frames, joints, coords), target (nseq, frames, joints, coords), f32, dense,
 * 4-byte aligned (16-byte loads are used wherever the addresses allow).
 *   per_sample (nseq, samples)  d[b, s] = mean over frames and joints of the per-joint L2 distance
 *                               ||pred[b, s, t, j, :] - target[b, t, j, :]||; required: the selection
 *                               reads it.  One workgroup per (sequence, sample), pred read once,
 *                               a fixed summation order that does not depend on s or on alignment.
 *   idx_out (nseq) int64        the index of the smallest d[b, :] (torch.min(dim).indices: the first
 *                               minimum; the first NaN if any), as sd_best_of_k
 *   min_out (nseq)              d[b, idx[b]] (mpjpe)
 *   best_out (nseq, frames, joints, coords)       pred[b, idx[b]]
 *   tail_out (nseq, tail_frames, joints, coords)  pred[b, idx[b], frames - tail_frames:] (the next
 *                               observation of the rollout); non-NULL only with tail_frames > 0
 * Every output but per_sample may be NULL.  1 <= samples <= 64, coords == 3, frames, joints >= 1,
 * 0 <= tail_frames <= frames (SD_E_INVALID names the argument); nseq == 0 launches nothing. */
int sd_best_sample(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames,
                   int32_t joints, int32_t coords, int32_t tail_frames, float* per_sample, float* min_out,
                   int64_t* idx_out, float* best_out, float* tail_out, void* stream);

/* Body-realism, limb-angle and motion-profile metrics (reference src/metrics/body_realism.py:109-199
 * limb_stretching_normed_rmse / _mean and limb_jitter_normed_rmse / _mean, src/metrics/multimodal.py:76-102
 * mae, src/metrics/cmd.py:10-12 motion_for_cmd) from one read of pred (nseq, samples, frames, joints, 3);
 * target (nseq, target_frames, joints, 3); f32, dense, 4-byte aligned (16-byte loads where the addresses
 * allow).  limbseq (nlimbs, 2) joint indices and angle_pairs (npairs, 2) limb indices (the consecutive
 * pairs of the reference's limb_angles_idx chains) are HOST int32 arrays, checked and passed to the
 * kernels by value.  All arithmetic on limb lengths and angles is f64, every sum has a fixed order that
 * depends on (frame, limb / pair / joint) only; results are f32.  A ground-truth limb of zero mean length
 * divides by zero, as in the reference.
 * sd_realism_target: the ground-truth pass.
 *   gt_len_mean (nseq, nlimbs) f64   mean over the target's frames of each limb's length; required
 *   gt_cos, gt_ang (nseq, frames, npairs) f64   per frame and pair the cosine between the two limbs
 *                               (limb vectors along the sorted limbseq, denominator clamped at 1e-7) and
 *                               acos of its clamp to [-1, 1]; NULL unless angles are wanted (gt_ang needs gt_cos)
 * sd_realism: the pass over the predictions, then the per-sequence reductions.  Every output may be NULL
 * and is then not computed; q = 0..5 is srmse_std, srmse_var, jrmse_std, jrmse_var, smean, jmean.
 *   none_out (6, nseq, samples, nlimbs)     reduction 'none' of the six quantities
 *   persample_out (6, nseq, samples)        their means over the limbs ('persample')
 *   limb_scratch (6, nseq, samples, nlimbs) f64, workspace of mean_out
 *   mean_out (6, nseq)                      their means over samples and limbs ('mean')
 *   angle_persample, cossim_persample (nseq, samples)  mean over frames and pairs of |acos - acos_gt| and
 *                               of |cos - cos_gt|, both times 180 / pi (mae with if_return_cossim False / True)
 *   angle_min, cossim_min (nseq)            their minima over the samples (NaN if any); each needs its persample
 *   motion_scratch (nseq, samples, frames - 1)  mean over joints of ||pred_t - pred_{t-1}||, workspace of
 *   motion_out (nseq, frames - 1)           its mean over the samples (motion_for_cmd); frames == 1: untouched
 * The float32 jitter quantities of frames == 1 are NaN (0 / 0), as the reference's.  target_frames is the
 * frame count gt_len_mean was taken over (limb_stretching_normed_mean with obs_as_target); angle outputs
 * need target_frames == frames.  1 <= samples, joints, nlimbs <= 64, 0 <= npairs <= 64, frames >= 1, every
 * limbseq entry in [0, joints), every angle_pairs entry in [0, nlimbs) (SD_E_INVALID names the argument,
 * before any device call); nseq == 0 launches nothing.
 * sd_realism_frame_tile: the number of frames the prediction pass stages at a time for `joints` joints. */
int sd_realism_target(const float* target, int64_t nseq, int32_t frames, int32_t joints, const int32_t* limbseq,
                      int32_t nlimbs, const int32_t* angle_pairs, int32_t npairs, double* gt_len_mean, double* gt_cos,
                      double* gt_ang, void* stream);
int sd_realism(const float* pred, int64_t nseq, int32_t samples, int32_t frames, int32_t joints, const int32_t* limbseq,
               int32_t nlimbs, const int32_t* angle_pairs, int32_t npairs, const double* gt_len_mean,
               const double* gt_cos, const double* gt_ang, int32_t target_frames, float* none_out, float* persample_out,
               double* limb_scratch, float* mean_out, float* angle_persample, float* cossim_persample, float* angle_min,
               float* cossim_min, float* motion_scratch, float* motion_out, void* stream);
int32_t sd_realism_frame_tile(int32_t joints);

/* FID on the device (reference src/metrics/fid.py:91-129 MetricStorerFID, src/metrics/fid_classifier.py:38-53
 * ClassifierForFID.get_fid_features).  The classifier is nn.GRU(input_size, 128, 2) over the frames followed
 * by tanh(linear1(h_last)); every pointer of the desc is a DEVICE f32 array in torch's layout: weight_ih_l0
 * (3 * 128, input_size), the other GRU weights (3 * 128, 128), the GRU biases (3 * 128), gate order r, z, n,
 * linear1_weight (feat_size, 128), linear1_bias (feat_size).
 * sd_fid_features (fid_classifier.py:43-53 and the reshape / permute copies of fid.py:111-120): one launch runs
 *   both layers over all frames for tiles of 32 rows and writes feats (rows, feat_size).
 *   motion (rows, frames, input_size) f32, dense: pred (B, S, T, J, 3) and target (B, T, J, 3) as they stand
 *   h0 (2, rows, 128) the initial hidden states, NULL = zeros
 *   workspace   sd_fid_workspace_bytes(desc, rows) bytes (the weights in matrix-instruction order, rewritten
 *               by every call: the desc's arrays may change between calls)
 *   All products are exact f32 (v_mfma_f32_32x32x2_f32); every sum has a fixed order that does not depend on
 *   the row's place in its tile, so a row's features are bitwise independent of the batch.
 *   hidden_size == 128, 1 <= feat_size <= 32, 1 <= input_size <= 64, frames >= 1, rows >= 0, workspace_bytes
 *   large enough (SD_E_INVALID names the argument, before any device call); rows == 0 launches nothing.
 *   sd_fid_workspace_bytes returns 0 for an invalid desc.
 * sd_fid_stats_update (fid.py:7-11 _calculate_activation_statistics, streamed): adds the batch's
 *   (count, sum x, sum x x^T) to state (1 + feat + feat * feat) f64: state[0] the row count, state[1 + a] the
 *   sums, state[1 + feat + a * feat + b] the products.  float64, rows in chunks of 256 (a chunk in row order,
 *   then the chunks in order), no atomics: the same calls give the same bits.  workspace:
 *   sd_fid_stats_workspace_bytes(rows, feat) bytes.  1 <= feat <= 32; rows == 0 launches nothing. */
typedef struct sd_fid_classifier_desc {
    int32_t input_size, hidden_size, feat_size; /* 48, 128, 30 in the release */
    const float *weight_ih_l0, *weight_hh_l0, *bias_ih_l0, *bias_hh_l0;
    const float *weight_ih_l1, *weight_hh_l1, *bias_ih_l1, *bias_hh_l1;
    const float *linear1_weight, *linear1_bias;
} sd_fid_classifier_desc;
size_t sd_fid_workspace_bytes(const sd_fid_classifier_desc* desc, int64_t rows);
int sd_fid_features(const sd_fid_classifier_desc* desc, const float* motion, int64_t rows, int32_t frames,
                    const float* h0, float* feats, void* workspace, size_t workspace_bytes, void* stream);
size_t sd_fid_stats_workspace_bytes(int64_t rows, int32_t feat);
int sd_fid_stats_update(const float* feats, int64_t rows, int32_t feat, double* state, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Multimodal ground truth (reference src/data/loaders/base/math_utils.py:59-110 get_multimodal_gt, whose
 * get_mmgt_idxs (:60-65) is torch.cdist(seq1, seq2, p=2, compute_mode='donot_use_mm_for_euclid_dist'), and the
 * APD of a segment's set of similar futures, src/metrics/multimodal.py:15-35 apd applied to the set: the
 * quantity behind the reference's shipped mmapd_GT.csv, src/metrics/apde.py:9-48).
 * sd_cdist: dist[i, j] = sqrt(sum_k (x1[i,k] - x2[j,k])^2), direct differences, f32;
 *   x1 (m, features), x2 (n, features), dist (m, n) dense; 4-byte aligned, 16-byte accesses where the
 *   addresses allow (an operand whose rows all start on a 16-byte boundary: an aligned base and features % 4
 *   == 0; dist likewise with n % 4 == 0).  m == 0 or n == 0 launches nothing.
 *   The value of dist[i, j] is a function of the two rows' contents and `features` only: the features are
 *   summed in chunks of 32 from feature 0 on, inside a chunk t = fma(d_k, d_k, t) for k ascending from t = 0,
 *   across chunks acc = acc + t in chunk order from acc = 0, then the correctly rounded square root.  So it
 *   does not depend on m, n, the tile, pointer alignment or which operand is x1: sd_cdist(x, x) is bitwise
 *   symmetric with an exactly zero diagonal, and row chunks give the bits of one call.
 * sd_set_mean_distance: out[s] = mean over a < b in [row_ptr[s], row_ptr[s+1]) of dist[col[a] * n + col[b]]
 *   (the reference's apd of the set, multimodal.py:15-35); 0 for a set of one member (multimodal.py:19-20),
 *   NaN for an empty one.  dist (n, n) f32; row_ptr (nsets + 1) and col are DEVICE int64 arrays, every col
 *   entry in [0, n).  float64 accumulation in a fixed order, f32 result.  nsets == 0 launches nothing.
 * Negative sizes, features < 1 and a NULL pointer with a non-empty shape: SD_E_INVALID names the argument,
 * before any launch. */
int sd_cdist(const float* x1, int64_t m, const float* x2, int64_t n, int64_t features, float* dist, void* stream);
int sd_set_mean_distance(const float* dist, int64_t n, const int64_t* row_ptr, const int64_t* col, int64_t nsets,
                         float* out, void* stream);

/* Diversity ranking (reference src/metrics/ranking.py:3-40 greates_minimum_distance / get_highest_diversity /
 * find_samples_maxapd_wrtGT and :42-63 get_closest_and_nfurthest_maxapd: the notebooks' choice of the futures
 * to show; there a batched torch.cdist and a Python loop per sequence with .tolist() / .nonzero() per pick).
 * Per sequence b the points are P_0 = the anchor and P_{1+s} = pred[b, s] (features floats each), and d(i, j)
 * is sd_cdist's value function above: bitwise symmetric, an exactly zero diagonal, independent of tile,
 * alignment and operand order.  Farthest-point greedy: C = {0}, m_i = d(i, 0) for i = 1..samples; for
 * k = 0..n_choose-1 the lowest index c not in C that maximises m_c is picked, idx_out[b, k] = c - 1,
 * score_out[b, k] = m_c, then c joins C and m_i = min(m_i, d(i, c)).  The comparisons are a total order in
 * which NaN ranks below every number (two NaNs: the lower index), and the min keeps a NaN: a NaN sample is
 * picked last.  The reference raises ValueError("No index found") on NaN; a kernel cannot raise.
 *   from_closest == 0: the anchor is target[b] (find_samples_maxapd_wrtGT).
 *   from_closest == 1: closest[b] = the first index of the minimum of d(target[b], pred[b, s]), NaN ranking
 *     above every number, and the anchor is pred[b, closest[b]] (get_closest_and_nfurthest_maxapd); its twin
 *     among the candidates is at distance exactly 0 and is taken last.
 *   pred (nseq, samples, features), target (nseq, features)  f32, dense, 4-byte aligned; 16-byte loads where
 *     both bases are 16-byte aligned and features % 4 == 0
 *   idx_out (nseq, n_choose) int64; required
 *   score_out (nseq, n_choose) f32, closest_out (nseq) int64 (from_closest == 1 only), dist_out (nseq,
 *     samples + 1, samples + 1) f32 = the matrix of [anchor; pred[b]]: each may be NULL
 *   workspace  sd_diverse_rank_workspace_bytes(nseq, samples) bytes (0 for invalid sizes)
 * Two launches: the distance matrices (upper triangle in tiles of 32 x 32, mirrored; never a pair of two
 * sequences), then one workgroup per sequence for the selection (a fixed shuffle tree, no atomics, no host
 * round trip).  1 <= samples <= 255, 1 <= n_choose <= samples, features >= 1, from_closest 0 or 1, nseq *
 * tile pairs <= 2^31 - 1 (SD_E_INVALID names the argument, before any launch); nseq == 0 launches nothing. */
size_t sd_diverse_rank_workspace_bytes(int64_t nseq, int32_t samples);
int sd_diverse_rank(const float* pred, const float* target, int64_t nseq, int32_t samples, int64_t features,
                    int32_t n_choose, int32_t from_closest, int64_t* idx_out, float* score_out, int64_t* closest_out,
                    float* dist_out, void* workspace, size_t workspace_bytes, void* stream);

/* Class-wise CMD accumulation (reference src/metrics/cmd.py:15-31 resolve_cmd and :34-57 CMDMetricStorer, which
 * keep every batch's motion profiles on the host): values (rows, width) f32 the batch's motion profiles
 * (sd_realism's motion_out), cls (rows) int64 DEVICE class indices; the state is updated in place:
 *   sum (classes, width) f64   += per class the rows' values; each (class, column) adds its rows in ascending
 *                              row order from the value it holds, so the state after a dataset is bitwise the
 *                              same however the rows were split into calls
 *   count (classes) int64      += the class's rows
 *   total (1) int64            += rows (a class index outside [0, classes) counts here only, as the
 *                              reference's mask, cmd.py:25-30)
 * One plain kernel, no atomics.  rows >= 0, width, classes >= 1 and non-NULL pointers (SD_E_INVALID names the
 * argument, before any launch); rows == 0 launches nothing. */
int sd_class_sum(const float* values, const int64_t* cls, int64_t rows, int32_t width, int32_t classes, double* sum,
                 int64_t* count, int64_t* total, void* stream);

/* Validation metrics of the training loops (reference src/train_utils.py:56-135 setup_validation_autoencoder /
 * setup_validation_diffusion, which run torch ops per batch and keep every prediction of the split on the host).
 * sd_limb_stats (src/metrics/body_realism.py:4-107 limb_length_variance, limb_length_jitter, limb_length_error,
 *   limb_length_variation_difference_wrtGT; the zero-hip padding of :7-10 is dead behind the assert of :6 and is
 *   not reproduced): one read of pred (nseq, samples, frames, joints, 3); target (nseq, frames, joints, 3) or
 *   NULL; f32, dense, 4-byte aligned (16-byte loads where the addresses allow).  limbseq (nlimbs, 2) is a HOST
 *   int32 array, checked and passed to the kernel by value.  Limb lengths and all arithmetic on them are f64,
 *   results f32.  Every output may be NULL and is then not computed.
 *   limb_out (5, nseq, samples, nlimbs)   per limb, over the frames: 0 the unbiased variance of the length
 *                               (torch.var, correction 1; NaN for frames == 1), 1 / 2 / 3 the mean / maximum /
 *                               minimum of |len_t - len_{t-1}| over the frames - 1 steps (NaN for frames == 1),
 *                               4 the mean of |target_len_t - len_t| (NaN without target)
 *   sample_out (7, nseq, samples)         over the limbs: 0 / 1 / 2 mean / max / min of plane 0, 3 mean of plane 1,
 *                               4 max of plane 2, 5 min of plane 3, 6 mean of plane 4
 *   sample_scratch (7, nseq, samples) f64 the same in f64, workspace of seq_out
 *   seq_out (9, nseq)                     over the samples: rows 0..6 reduce sample rows 0..6 each with its own
 *                               operation (mean / max / min), rows 7 / 8 are the max / min of sample row 6
 *   steps_out (nseq, samples, frames - 1, nlimbs)  |len_t - len_{t-1}| itself (limb_length_jitter mode 'none')
 *   steps_diff_out (same shape)           that minus the target's |target_len_t - target_len_{t-1}|, subtracted in
 *                               f64 (limb_length_variation_difference_wrtGT mode 'none'); needs target
 *   The variance is Chan's combination, over the frame tiles in order, of per-tile sums of squares about the
 *   tile's own mean: never E[x^2] - mean^2.  Maxima and minima keep a NaN, as torch.max / torch.min.  A limb's
 *   sums run over the frames in frame order, a sample's reductions over the limbs in limb order, a sequence's
 *   over the samples in sample order; no atomics.  The frame tile is sd_realism_frame_tile(joints).
 *   1 <= samples, joints, nlimbs <= 64, frames >= 1, every limbseq entry in [0, joints), seq_out needs
 *   sample_scratch (SD_E_INVALID names the argument, before any device call); nseq == 0 launches nothing.
 * sd_frame_error_update (src/metrics/ignite_mpjpe.py MeanPerJointPositionError, src/metrics/ignite_fde.py
 *   FinalDisplacementError: the streaming state of sum over the rows of the per-joint L2 distance):
 *   pred (rows, samples, frames, joints, 3), target (rows, frames, joints, 3) f32, dense, 4-byte aligned;
 *   idx (rows) DEVICE int64, the sample each row takes (sd_best_sample's idx_out: the chosen future is never
 *   gathered), or NULL with samples == 1; the window is frames [frame0, frame0 + nframes) (the FDE: frame0 =
 *   frames - 1, nframes = 1).  The state is updated in place:
 *   sum (nframes, joints) f64   += over the rows ||pred[r, idx[r], frame0 + f, j, :] - target[r, frame0 + f, j, :]||
 *                               (an f64 norm of f64 differences); each (frame, joint) adds its rows in ascending
 *                               row order onto the value it holds, so the state after a dataset is bitwise the
 *                               same however the rows were split into calls
 *   count (1) int64             += rows
 *   A row whose idx is outside [0, samples) adds NaN to all its sums and reads nothing of pred.  A NaN in pred
 *   or target reaches only the (frame, joint) sums it belongs to.  One plain kernel, no atomics.
 *   rows >= 0, 1 <= samples, joints <= 64, frames >= 1, 0 <= frame0 < frames, 1 <= nframes <= frames - frame0,
 *   non-NULL sum and count (SD_E_INVALID names the argument, before any launch); rows == 0 launches nothing. */
int sd_limb_stats(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames, int32_t joints,
                  const int32_t* limbseq, int32_t nlimbs, float* limb_out, float* sample_out, double* sample_scratch,
                  float* seq_out, float* steps_out, float* steps_diff_out, void* stream);
int sd_frame_error_update(const float* pred, const float* target, const int64_t* idx, int64_t rows, int32_t samples,
                          int32_t frames, int32_t joints, int32_t frame0, int32_t nframes, double* sum, int64_t* count,
                          void* stream);

/* Test hooks: one kernel on caller buffers, for the per-kernel numerics tests.
 * sd_test_graph_linear: out(B,J,N) = act(FiLM(ghat @ (s_j W[type j] [x1_j | x2_j] + bias[type j]))) + res,
 *   W (types,N,K1+K2), bias (types,N) or NULL, ghat (J,J), film (2N) or NULL, res (B,J,N) or NULL,
 *   x1 row b read at b / x1_div, s_j = 1/max(||x1_j||,1e-12) when rms (else 1), act 0/1 = none/tanh.
 * sd_test_attention: out(B,J,heads*dh) = softmax(q k^T / sqrt(dh)) v per head, qkv (B,J,3*heads*dh). */
int sd_test_graph_linear(const float* x1, int32_t K1, int64_t x1_div, const float* x2, int32_t K2,
                         const float* W, const float* bias, const int64_t* node_types, const float* ghat,
                         const float* film, int32_t act, const float* res, float* out, int64_t rows,
                         int32_t J, int32_t N, int32_t rms, void* stream);
/* sd_test_graph_linear_layout: as sd_test_graph_linear with operand layouts: bit 0 x1, bit 1 x2,
 *   bit 2 res, bit 3 out in the v4 row-blocked layout (per 32-row block and node, features as
 *   [F/8][2][32 rows][4]; buffers padded to a multiple of 32 rows); needs the v4 kernels. */
int sd_test_graph_linear_layout(const float* x1, int32_t K1, int64_t x1_div, const float* x2, int32_t K2,
                                const float* W, const float* bias, const int64_t* node_types, const float* ghat,
                                const float* film, int32_t act, const float* res, float* out, int64_t rows,
                                int32_t J, int32_t N, int32_t rms, int32_t layout, void* stream);
int sd_test_attention(const float* qkv, float* out, int64_t rows, int32_t J, int32_t heads,
                      int32_t dim_head, void* stream);
/* sd_test_qkv_attention: the fused to_qkv + Attention kernel on caller buffers: qkv = G-hat-mixed
 *   StaticGraphLinear (s_j W[type j] x_j, s_j = RMS scale when rms, no bias) with W (types, 3*heads*32, K),
 *   then out(B,J,heads*32) = softmax(q k^T / sqrt(32)) v per head.  SD_E_INVALID where the fused
 *   kernel does not apply (J > 16).  layout bit 0 / bit 3: x / out row-blocked (as
 *   sd_test_graph_linear_layout).  Replaces to_qkv + Attention, attention.py:105-136. */
int sd_test_qkv_attention(const float* x, int32_t K, const float* W, const int64_t* node_types, const float* ghat,
                          float* out, int64_t rows, int32_t J, int32_t heads, int32_t rms, int32_t layout,
                          void* stream);
/* Test hook: the kernel generation of the sd_test_* entry points ONLY (plans never read it; a
 * plan's generation is its SD_OPT_KERNEL_VARIANT / SD_OPT_GL4_TILE):
 * gl_variant 0 = auto (v4 split-f16 where available, else exact-f32 v3/v2/v5), 2 / 3 = exact-f32
 * generations (1, the removed first generation, runs 2), 4 = v4, 5 = v5; gl4_tile =
 * <waves><row tiles><col tiles> (e.g. 822) or 0 = auto, -1 leaves it.  Returns the previous
 * gl_variant, or -1 for an invalid one (nothing changed); gl_variant = -1 only queries (returns
 * the current value). */
int sd_test_set_kernel_variant(int32_t gl_variant, int32_t gl4_tile);
/* Test hook: the v4 split route of the sd_test_graph_linear* entry points ONLY (as
 * SD_OPT_SPLIT_ROUTE: 0 auto, 1 never, 2 k_gl4y GEMM phase, 3 k_gl4t GEMM phase, 4 k_gl4t except
 * to_qkv + attention; 2 / 3 / 4 allocate the pre-mix scratch per call).  Returns the previous route,
 * or -1 for an invalid one; route = -1 only queries. */
int sd_test_set_split_route(int32_t route);

/* Per-plan kernel options (read by the launches recorded after the call; part of the graph
 * cache key).  There is no process-wide kernel state: a plan starts from the SKELDIFF_*
 * environment read at library load and keeps its own options, so two plans may hold different
 * options and sample concurrently.  SD_E_INVALID for an unknown option or value. */
enum {
    SD_OPT_KERNEL_VARIANT = 1,  /* 0 auto, 2..5 force a graph-linear generation; 1 (the removed
                                   first generation) is an alias of 2 */
    SD_OPT_GL4_TILE = 2,        /* v4 tile <waves><row tiles><col tiles>, 0 = per shape */
    SD_OPT_ROW_CHAINS = 3,      /* 1..8 concurrent row chains in sd_sample_loop; 0 = auto
                                   (3, or 2 at <= 1,200 rows) */
    SD_OPT_PRECISION = 4,       /* as sd_plan_set_precision */
    SD_OPT_GL4_STAGING = 5,     /* v4 weight stages: 0 LDS-DMA (default), 1 register-staged;
                                   2 = 0 (a round-2 diagnostic setting, kept for compatibility) */
    SD_OPT_SPLIT_ROUTE = 6,     /* v4 split route (GEMM phase per (tile, node) + mixing phase,
                                   DESIGN.md §4d'; bitwise identical results): 0 auto (k_gl4y at
                                   <= 1200 rows of the call; k_gl4t for full batches where measured
                                   faster), 1 never (the one-kernel k_gl4 tiles), 2 always (k_gl4y),
                                   3 always with the tiled GEMM phase (k_gl4t: 128 rows x up to 192
                                   columns of one node per workgroup), 4 the tiled GEMM phase except
                                   for to_qkv + attention (one-kernel fused tile).  ABI 3 removed 5
                                   (small-batch fused tile) and 6 (fused layer kernel k_gl4f):
                                   measured slower, DESIGN.md §4i / §4j */
    SD_OPT_LAST_CHAINS = 7,     /* read-only: row chains the plan's last sd_sample_loop ran (the
                                   SD_OPT_ROW_CHAINS value, fewer for batches of fewer than n
                                   32-row units, a ragged last unit counting; auto: 1 at <= 128
                                   rows, 2 at <= 1,200 rows, else 3); 0 before the first
                                   call */
    SD_OPT_LAST_ROUTE = 8,      /* read-only: kernels the plan's last sd_sample_loop launched, bits
                                   1 one-kernel k_gl4, 2 fused to_qkv + attention k_gl4, 4 k_gl4y
                                   GEMM phase, 8 k_gl4t GEMM phase, 16 split-route mixing /
                                   attention phase, 32 v5 mixing (J > 21), 64 exact-f32 kernels,
                                   128 separate k_attention, 1024 k_attention_mix (256 / 512: the
                                   kernels ABI 3 removed) */
    SD_OPT_UPDATE_KERNEL = 9,   /* posterior update: 0 (default) the J x J projections on
                                   v_mfma_f32_16x16x4_f32 where they apply (nonisotropic, J <= 64),
                                   1 the element-per-thread forms; the same bits (ABI 3 removed the
                                   pipelined forms 2 / 3: measured no faster) */
    SD_OPT_V5_MIX = 10,         /* J > 21 mixing pass (v5): 0 (default) G-hat mixing on
                                   v_mfma_f32_16x16x4_f32 (k_gl5_mixm), 1 the VALU form (k_gl5_mix);
                                   the same j-ordered fmaf chains */
    SD_OPT_ATTENTION = 11       /* separate attention kernel at 49 <= J <= 52 (MANO), both forms
                                   the same bits: 0 (default) auto = 2; 2 the to_qkv layer's G-hat
                                   mixing inside the attention kernel, its pre-mix Y in the qkv
                                   buffer (k_attention_mix, 5 % faster); 3 after the mixing pass,
                                   padded to 64 nodes.  ABI 3 removed 1 (the 48-node
                                   tail form, 1 % slower) */
};
int sd_plan_set_option(sd_plan* plan, int32_t option, int64_t value);
int sd_plan_get_option(const sd_plan* plan, int32_t option, int64_t* value);

/* Graph-GRU latent decoder: AutoEncoder.decode -> Decoder.forward
 * (src/core/network/nn/decoder.py:60-104) with the StaticGraphGRU cell
 * (src/core/network/layers/recurrent.py:321-366), recurrent_arch_decoder = StaticGraphGRU, one
 * layer, clockwork off.  Tensors are the reference's `decoder.*` state_dict entries on the device
 * (types = num_node_types, or 1 with shared weights when num_node_types == 0):
 *   init_*  initial_hidden_h: G (J,J), weight (types, H, F+L), bias (types, H) or NULL
 *   G, G_add, weight_ih (types, 3H, F+L), weight_hh (types, 3H, H), bias_ih, bias_hh (types, 3H)
 *           rnn.layers.0 (G_add may be NULL: no additive influence)
 *   fc_*    fc: G (J,J), weight (types, F, H), bias (types, F) or NULL
 * x (rows, 2, J, F) = the last two observed frames (x[:, -2:]), h (rows, J, L) = the sampled
 * latents -> out (rows, ph, J, F).  1 <= J <= 64, 1 <= F <= 16, L and H positive multiples of 16,
 * and the gate kernel's per-row LDS (3 J H + J^2) * 4 bytes must fit in 160 KiB (J = 64: H <= 192):
 * sd_gru_decode / sd_gru_encode refuse anything else with SD_E_INVALID before any device work, and
 * the *_workspace_bytes functions return 0 for it (sd_last_error() names the field). */
typedef struct sd_gru_decoder_desc {
    int32_t num_nodes, feature_size, latent_size, hidden_size, num_node_types;
    const int64_t* node_types; /* host array[J] (ignored when num_node_types == 0) */
    const float *init_G, *init_weight, *init_bias;
    const float *G, *G_add, *weight_ih, *weight_hh, *bias_ih, *bias_hh;
    const float *fc_G, *fc_weight, *fc_bias;
} sd_gru_decoder_desc;
size_t sd_gru_decode_workspace_bytes(const sd_gru_decoder_desc* desc, int64_t rows, int32_t ph);
int sd_gru_decode(const sd_gru_decoder_desc* desc, const float* x, const float* h, int64_t rows, int32_t ph,
                  float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Graph-GRU encoder + z_activation (src/core/network/nn/encoder.py:75-80, autoencoder.py:47-51,
 * encoder_act = z_activation = tanh): x (rows, frames, J, F) observed frames -> z (rows, J, L) =
 * tanh(tanh(fc(GRU over the frames from initial_hidden1(x[:, 0])))).  Same descriptor with the
 * `encoder.*` tensors: init_* = initial_hidden1 (weight (types, H, F)), weight_ih (types, 3H, F),
 * G_add = NULL, fc weight (types, L, H); latent_size = L. */
size_t sd_gru_encode_workspace_bytes(const sd_gru_decoder_desc* desc, int64_t rows, int32_t frames);
int sd_gru_encode(const sd_gru_decoder_desc* desc, const float* x, int64_t rows, int32_t frames, float* z,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Arithmetic of the plan's graph-linear launches.  mode 0 (default):
 * f32-accurate -- 3 split f16 products per f32 product, within the f32-vs-f64 drift.  mode 1:
 * half -- one f16 product (x and W rounded to f16), f32 accumulate, f32 activations in HBM; the
 * latent ADE / APD stay within 1 % of mode 0 (tests/test_precision.py).  Applies to the split-f16
 * (v4) kernels (J in 16, 17, 21); plans on the exact-f32 kernels stay exact.  mode 2: bf16 --
 * "bf16 latents + fp32 Sigma_N projection" (BASELINE config 5): one bf16 product per
 * multiply-add (v_mfma_f32_32x32x16_bf16), f32 accumulate and epilogue; the latents between
 * steps (x_t, x0) and the residual-stream activations are bf16 in HBM; the posterior update
 * (C1 x0 + C2 x_t + U (sigma eps)) computes in f32; start noise, records and the final latents
 * are f32 at the ABI.  J in 16, 17, 21 only (SD_E_INVALID otherwise).  Affects launches recorded
 * after the call; SD_E_INVALID for another mode. */
int sd_plan_set_precision(sd_plan* plan, int32_t mode);

/* Training-side StaticGraphLinear (SURVEY.md §8f "next" #4): replaces GraphLinear.forward
 * (src/core/network/layers/graph_structural.py:30-43, StaticGraphLinear :105-114) and the backward
 * torch autograd derives for it in NonisotropicGaussianDiffusion.forward / p_losses training
 * (src/core/diffusion/base.py:262-307).  Caller-owned device buffers, row-major:
 *   x (rows, J, K), W (types, N, K), bias (types, N) or NULL, node_types device int64 (J) with
 *   values in [0, n_types) (n_types = 0: shared weights, W (1, N, K), node_types ignored),
 *   ghat (J, J) = the mixing matrix actually applied (G, or G / rowsum|G| when learn_influence).
 * sd_gl_train_forward: z = W[type j] x_j + bias[type j] (pre-mix, kept for backward), y = ghat @ z.
 * sd_gl_train_backward: from dy (rows, J, N) and the forward's z: dx (rows, J, K), dW (types, N, K),
 *   dbias (types, N), dghat (J, J); any output may be NULL (not computed).  Deterministic (fixed
 *   reduction order).  workspace >= sd_gl_train_workspace_bytes(rows, J, K, N, n_types).
 *   1 <= J <= 64. */
size_t sd_gl_train_workspace_bytes(int64_t rows, int32_t J, int32_t K, int32_t N, int32_t n_types);
int sd_gl_train_forward(const float* x, const float* W, const float* bias, const int64_t* node_types,
                        int32_t n_types, const float* ghat, int64_t rows, int32_t J, int32_t K, int32_t N,
                        float* z, float* y, void* stream);
int sd_gl_train_backward(const float* x, const float* z, const float* dy, const float* W, const int64_t* node_types,
                         int32_t n_types, const float* ghat, int64_t rows, int32_t J, int32_t K, int32_t N, float* dx,
                         float* dW, float* dbias, float* dghat, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Attention over joints under autograd (training side; reference attention.py:122-136, the part
 * between to_qkv and to_out): qkv (rows, J, 3 * heads * dim_head) as to_qkv writes it.
 * sd_attn_train_forward: out (rows, J, heads * dim_head) = softmax((q scale) k^T) v per head.
 * sd_attn_train_backward: dqkv (rows, J, 3 * heads * dim_head) from dout, P recomputed.
 * 1 <= J <= 64, 1 <= dim_head <= 64; f32; one workgroup per (row, head). */
int sd_attn_train_forward(const float* qkv, float* out, int64_t rows, int32_t J, int32_t heads, int32_t dim_head,
                          float scale, void* stream);
int sd_attn_train_backward(const float* qkv, const float* dout, float* dqkv, int64_t rows, int32_t J, int32_t heads,
                           int32_t dim_head, float scale, void* stream);
/* FiLM + tanh of a ResnetBlock's first Block under autograd (reference attention.py:67-75):
 * y (rows, J, C), ss (rows, 2C) = scale | shift (the time MLP's output, broadcast over the J nodes):
 * out = tanh(y (scale + 1) + shift); backward: dy (rows, J, C) and dss (rows, 2C) from dout.
 * rows <= 65535 for the backward. */
int sd_film_tanh_forward(const float* y, const float* ss, float* out, int64_t rows, int32_t J, int32_t C, void* stream);
int sd_film_tanh_backward(const float* y, const float* ss, const float* out, const float* dout, float* dy, float* dss,
                          int64_t rows, int32_t J, int32_t C, void* stream);

/* Row-wise L1 normalisation of a learnable influence matrix under autograd (reference
 * graph_structural.py:107, F.normalize(G, p=1, dim=1)): ghat[i][j] = G[i][j] / max(sum_k |G[i][k]|, eps);
 * the backward writes dG from dghat.  `count` contiguous J x J row-major matrices (one launch for
 * all of a Denoiser's learnable G), 1 <= J <= 64, f32. */
int sd_l1norm_rows_forward(const float* G, float* ghat, int32_t J, int32_t count, float eps, void* stream);
int sd_l1norm_rows_backward(const float* G, const float* dghat, float* dG, int32_t J, int32_t count, float eps,
                            void* stream);
/* Training-side graph-GRU: the recurrent core of StaticGraphGRUCell.forward unrolled
 * over a sequence by StaticGraphGRU.forward / Decoder.forward (reference
 * src/core/network/layers/recurrent.py:321-366 and :369-391, src/core/network/nn/decoder.py:85-104,
 * clockwork off) and the backward torch autograd derives for it in AutoEncoderTrainer.train_step
 * (src/core/trainer.py:79-96).  Caller-owned device buffers, row-major f32:
 *   a (rows, Ta, J, 3H) = W_ih x + b_ih, unmixed; Ta = T (one projection per frame) or 1 (one
 *   projection reused at every step), h0 (rows, J, H), gx (Tg, J, J) the mixing matrix per step,
 *   Tg = T or 1, W_hh (types, 3H, H), b_hh (types, 3H) or NULL, node_types HOST int64 (J) with
 *   values in [0, n_types) (n_types = 0: shared weights, W_hh (1, 3H, H), node_types ignored).
 * sd_gru_train_forward: hs (rows, T, J, H), the hidden state after each step.  With hprev
 *   (rows, T, J, H), c (rows, T, J, 3H) and gates (rows, T, J, 4H) given (all three or none) it keeps
 *   the state backward reads: h_{t-1}, c_t = W_hh h_{t-1} + b_hh and [r | z | n | (gx c)_n].
 * sd_gru_train_backward: from dhs (rows, T, J, H) and that state: da (rows, Ta, J, 3H) (summed over
 *   the steps when Ta = 1), dh0 (rows, J, H), dgx (Tg, J, J) (per step when Tg = T), dW_hh, db_hh;
 *   any output may be NULL (not computed).  Every reduction over rows and steps runs in a fixed
 *   order (no float atomics): repeated calls give the same bits.
 * Both need workspace >= sd_gru_train_workspace_bytes(rows, T, J, H, n_types).
 * Checked on the host before any device call (SD_E_INVALID names the argument): NULL pointers, J
 * outside 1..64, H not a positive multiple of 16 (at most 256), T < 1, Ta / Tg not in {1, T}, node
 * types out of range, a short workspace, more than 262,140 rows in a backward asked for dgx.
 * rows == 0: SD_OK (the backward zeroes dgx, dW_hh, db_hh). */
size_t sd_gru_train_workspace_bytes(int64_t rows, int32_t T, int32_t J, int32_t H, int32_t n_types);
int sd_gru_train_forward(const float* a, int32_t Ta, const float* h0, const float* gx, int32_t Tg, const float* W_hh,
                         const float* b_hh, const int64_t* node_types, int32_t n_types, int64_t rows, int32_t T,
                         int32_t J, int32_t H, float* hs, float* hprev, float* c, float* gates, void* workspace,
                         size_t workspace_bytes, void* stream);
int sd_gru_train_backward(const float* dhs, const float* a, int32_t Ta, const float* gx, int32_t Tg, const float* W_hh,
                          const int64_t* node_types, int32_t n_types, const float* hprev, const float* c,
                          const float* gates, int64_t rows, int32_t T, int32_t J, int32_t H, float* da, float* dh0,
                          float* dgx, float* dW_hh, float* db_hh, void* workspace, size_t workspace_bytes, void* stream);
/* The cell's mixing matrix per step under autograd (reference recurrent.py:333-334 and :361-364):
 *   gxt[0] = normalize_L1(G) (normalize0 != 0: learn_influence) or G,
 *   gxt[t + 1] = normalize_L1(gxt[t] + G_add), row-wise with F.normalize's eps; G_add NULL = 0.
 * One launch each way, the steps in sequence inside the kernel.  gxt, dgxt (T, J, J); the backward
 * reads the forward's gxt and writes dG and dG_add (NULL: not computed).  1 <= J <= 64, T >= 1. */
int sd_gx_table_forward(const float* G, const float* G_add, int32_t J, int32_t T, int32_t normalize0, float eps,
                        float* gxt, void* stream);
int sd_gx_table_backward(const float* G, const float* G_add, const float* gxt, const float* dgxt, int32_t J, int32_t T,
                         int32_t normalize0, float eps, float* dG, float* dG_add, void* stream);
/* Training-side graph-LSTM: the recurrent core of StaticGraphLSTMCell.forward unrolled
 * over a sequence by StaticGraphLSTM.forward / Decoder.forward (reference
 * src/core/network/layers/recurrent.py:126-167 and :170-196, src/core/network/nn/encoder.py:55-82,
 * src/core/network/nn/decoder.py:47-52 and :75-104, clockwork off) and the backward torch autograd
 * derives for it.  Per step: P_t = a_t + W_hh h_{t-1} + b_hh (unmixed), Q_t = gx_t P_t in the chunk
 * order i | f | g | o, s_t = sigma(Q_f) s_{t-1} + sigma(Q_i) tanh(Q_g), h_t = sigma(Q_o) tanh(s_t)
 * (bias_ih takes no part, as in the reference).  Caller-owned device buffers, row-major f32:
 *   a (rows, Ta, J, 4H) = W_ih x, unmixed, no bias; Ta = T (one projection per frame) or 1 (one
 *   projection reused at every step), h0 and s0 (rows, J, H) the initial hidden and cell state,
 *   gx (Tg, J, J) the mixing matrix per step, Tg = T or 1, W_hh (types, 4H, H), b_hh (types, 4H) or
 *   NULL, node_types HOST int64 (J) with values in [0, n_types) (n_types = 0: shared weights,
 *   W_hh (1, 4H, H), node_types ignored).
 * sd_lstm_train_forward: hs (rows, T, J, H), the hidden state after each step, and s_last
 *   (rows, J, H), the cell state after the last (NULL: not written).  With P (rows, T, J, 4H), gates
 *   (rows, T, J, 4H) and sseq (rows, T, J, H) given (all three or none) it keeps the state backward
 *   reads: P_t, [i | f | g | o] and s_t.
 * sd_lstm_train_backward: from dhs (rows, T, J, H), that state and the forward's h0, s0, hs: da
 *   (rows, Ta, J, 4H) (summed over the steps in order when Ta = 1), dh0, ds0 (rows, J, H), dgx
 *   (Tg, J, J) (per step when Tg = T), dW_hh, db_hh; any output may be NULL (not computed).  Every
 *   reduction over rows and steps runs in a fixed order (no float atomics): repeated calls give the
 *   same bits.
 * The backward needs workspace >= sd_lstm_train_workspace_bytes(rows, T, J, H, n_types); the forward
 * only sd_lstm_train_forward_workspace_bytes(rows, J, H, n_types) (W_hh transposed, one step's P and two
 * cell-state slabs: independent of T), which the former covers.
 * Checked on the host before any device call (SD_E_INVALID names the argument): NULL pointers, J
 * outside 1..64, H not a positive multiple of 16 (at most 256), T < 1, Ta / Tg not in {1, T}, node
 * types out of range, a short workspace, more than 262,140 rows in a backward asked for dgx.
 * rows == 0: SD_OK (the backward zeroes dgx, dW_hh, db_hh). */
size_t sd_lstm_train_workspace_bytes(int64_t rows, int32_t T, int32_t J, int32_t H, int32_t n_types);
size_t sd_lstm_train_forward_workspace_bytes(int64_t rows, int32_t J, int32_t H, int32_t n_types);
int sd_lstm_train_forward(const float* a, int32_t Ta, const float* h0, const float* s0, const float* gx, int32_t Tg,
                          const float* W_hh, const float* b_hh, const int64_t* node_types, int32_t n_types, int64_t rows,
                          int32_t T, int32_t J, int32_t H, float* hs, float* s_last, float* P, float* gates, float* sseq,
                          void* workspace, size_t workspace_bytes, void* stream);
int sd_lstm_train_backward(const float* dhs, int32_t Ta, const float* gx, int32_t Tg, const float* W_hh,
                           const int64_t* node_types, int32_t n_types, const float* h0, const float* s0, const float* hs,
                           const float* P, const float* gates, const float* sseq, int64_t rows, int32_t T, int32_t J,
                           int32_t H, float* da, float* dh0, float* ds0, float* dgx, float* dW_hh, float* db_hh,
                           void* workspace, size_t workspace_bytes, void* stream);
/* PreNorm's RMSNorm under autograd (reference attention.py:30-36): x (R, C), R vectors of C
 * features, out = x / max(||x||, eps) * g * scale (scale = sqrt(C)); the forward also writes
 * dnorm (R) = max(||x||, eps) for the backward, which writes dx (R, C) and dg (C), the latter
 * summed over vectors in a fixed order through a workspace of sd_rmsnorm_workspace_bytes.
 * 1 <= C <= 1024. */
size_t sd_rmsnorm_workspace_bytes(int64_t R, int32_t C);
int sd_rmsnorm_forward(const float* x, const float* g, float* out, float* dnorm, int64_t R, int32_t C, float scale,
                       float eps, void* stream);
int sd_rmsnorm_backward(const float* x, const float* g, const float* dnorm, const float* dy, float* dx, float* dg,
                        int64_t R, int32_t C, float scale, float eps, void* workspace, size_t workspace_bytes,
                        void* stream);
/* Mahalanobis loss of NonisotropicGaussianDiffusion reduced per row (reference
 * nonisotropic.py:177-190 and base.py:297-298): model_out, target (rows, J, F), S =
 * mahalanobis_S_sqrt_recip (T, J, J), t (rows) int64 timesteps (a row whose t is outside [0, T) gets a NaN
 * loss / gradient: no out-of-range table read);
 * loss[r] = mean_{i,f} |(S[t_r] D_r)[i][f]| (mse: squared), D = target - model_out when
 * pred_noise, else model_out - target.  The backward writes d model_out (rows, J, F) from dloss
 * (rows).  1 <= J <= 64, 1 <= F <= 256, f32. */
int sd_mahalanobis_loss_forward(const float* model_out, const float* target, const float* S, const int64_t* t,
                                int32_t T, int64_t rows, int32_t J, int32_t F, int32_t pred_noise, int32_t mse, float* loss,
                                void* stream);
int sd_mahalanobis_loss_backward(const float* model_out, const float* target, const float* S, const int64_t* t,
                                 int32_t T, const float* dloss, int64_t rows, int32_t J, int32_t F, int32_t pred_noise,
                                 int32_t mse, float* dmodel_out, void* stream);

/* Fused optimizer step: what follows backward in the reference's two training loops,
 * src/core/trainer.py:33 (AdamW, amsgrad) and :93-95 (clip_grad_norm_, step) of AutoEncoderTrainer,
 * :153 (Adam), :159 (ema_pytorch.EMA) and :267-275 (clip_grad_norm_, step, ema.update) of
 * TrainerDiffusion.  Each entry works on ALL tensors of a model, f32 and contiguous on one device, in
 * one launch per 40 tensors; the tensor table travels in the launches' arguments, so the host arrays
 * are read before the call returns, nothing is kept between calls and no call synchronises.
 *
 * sd_optim_grad_norm: total_norm = sqrt(sum of g^2 over all tensors) as clip_grad_norm_(norm_type 2,
 *   error_if_nonfinite=False) defines it, summed in float64 through per-chunk partial sums in
 *   `workspace` (>= sd_optim_workspace_bytes(numel, n_tensors)) in a fixed order, and
 *   coef = min(max_norm / (total_norm + 1e-6), 1), NaN kept.  norm_coef (device, 2 floats) receives
 *   { total_norm, coef }.  The gradients are not changed.
 * sd_optim_adam_step: per element, in f32:  g = g coef (coef: device scalar, NULL = 1);
 *   Adam: g' = g + wd p;  AdamW (SD_OPTIM_DECOUPLED_WD): p = p (1 - lr wd), g' = g;
 *   m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;  SD_OPTIM_AMSGRAD: vmax = max(vmax, v);
 *   p = p - lr / (1 - beta1^step) * m / (sqrt(v or vmax) / sqrt(1 - beta2^step) + eps).
 *   `step` is the tensor's own count including this step (>= 1).  With SD_OPTIM_STORE_GRADS the
 *   clipped g is written back to grad (what clip_grad_norm_ leaves there); without it grad is only read.
 * sd_optim_ema_update: ema[i] = lerp(ema[i], params[i], weight) in torch.lerp's two-sided form
 *   (weight = 1 is an exact copy), 0 <= weight <= 1.
 * Checked on the host before any device call (SD_E_INVALID names the argument): NULL arrays and NULL
 * tensors, numel < 0, lr < 0, weight_decay < 0, step < 1, beta1 / beta2 outside [0, 1), eps < 0,
 * max_norm <= 0, a short workspace.  n_tensors == 0 and tensors of no elements: SD_OK, nothing done. */
#define SD_OPTIM_AMSGRAD 1
#define SD_OPTIM_DECOUPLED_WD 2
#define SD_OPTIM_STORE_GRADS 4
typedef struct sd_optim_param {
    float* p;              /* (numel) parameter, updated in place */
    float* grad;           /* (numel) gradient */
    float* exp_avg;        /* (numel) m */
    float* exp_avg_sq;     /* (numel) v */
    float* max_exp_avg_sq; /* (numel) vmax; read only with SD_OPTIM_AMSGRAD (else may be NULL) */
    int64_t numel;
    int64_t step;
    double lr;
    double weight_decay;
} sd_optim_param;
size_t sd_optim_workspace_bytes(const int64_t* numel, int32_t n_tensors);
int sd_optim_grad_norm(const float* const* grads, const int64_t* numel, int32_t n_tensors, float max_norm,
                       float* norm_coef, void* workspace, size_t workspace_bytes, void* stream);
int sd_optim_adam_step(const sd_optim_param* params, int32_t n_tensors, double beta1, double beta2, double eps,
                       int32_t flags, const float* coef, void* stream);
int sd_optim_ema_update(float* const* ema, const float* const* params, const int64_t* numel, int32_t n_tensors,
                        float weight, void* stream);

/* Motion batches from clips resident on the device: the reference's per-item data path for a
 * whole batch in one kernel.  It replaces BaseDataset.__getitem__ / _get_segment
 * (src/data/loaders/base/base_dataset.py:109-133, :164-177), add_noise and MotionDataset.__getitem__ /
 * data_augmentation / tranform2inputspace (src/data/loaders/base/motion_dataset.py:11-19, :129-165, :176-193),
 * Skeleton.tranform_to_input_space with if_consider_hip = False (src/data/skeleton/motion/base.py:35-42,
 * centerpose.py:13-18, rescalepose.py:17-25, utils.py:3-8), default_collate and the host-to-device copy.
 * sd_motion_batch, per sample b (every step in f32, one rounding per operation):
 *   segment = clamp(stride * sample_idx[b] + augmentation (+ offset in [-augmentation, augmentation] when
 *   augmentation != 0), 0, nseg - 1); its obs_len + pred_len frames start at global frame seg_first[segment] of
 *   frames (total_frames, joints, 3); segment_idx[b] = segment.
 *   noisy: joints 1.. of the observation frames: a (frame, joint) pair is hit with probability noise_level and
 *   gets noise_std * a normal per coordinate; in eval mode too, before the augmentation.
 *   train: coordinate m in (0, 1) changes sign with probability da_mirroring each; with probability
 *   da_rotations an integer angle d in [0, 360): x' = c x - s y, y' = s x + c y, c = rot_table[d],
 *   s = rot_table[360 + d] (DEVICE, 720 floats: the f32 roundings of the f64 cosines, then sines).
 *   representation: SD_MOTION_RESCALE_POSE subtracts joint 0 of the same frame and divides by pose_box_size
 *   (a correctly rounded division); SD_MOTION_CENTER_POSE subtracts only; SD_MOTION_VANILLA neither.  Joint 0
 *   is dropped: obs (B, obs_len, joints - 1, 3), pred (B, pred_len, joints - 1, 3).
 *   Draws: with every draw_* pointer NULL they come from the sampler's Philox stream (sd_philox_raw) keyed
 *   (seed, row = sample_idx[b], step = epoch) -- the quad map is in csrc/sd_motion_batch_addr.h --, so a
 *   sample's draws do not depend on its batch.  Otherwise draw_offset (B) i32, draw_mirror (B, 2) u8 and
 *   draw_degrees (B) i32 (-1: no rotation) are read instead, and with noisy draw_noise_mask (B, obs_len,
 *   joints - 1) u8 and draw_noise (B, obs_len, joints - 1, 3) f32 (already times noise_std).
 * sd_motion_draws writes the Philox stream's decisions in exactly that form (noise_mask and noise both NULL:
 *   the per-sample ones only); sd_motion_batch given them returns the bits of its Philox path.
 * sd_motion_batch_frame_tile: frames per workgroup for a joint count (-1 outside [2, 64]).
 * All pointers are DEVICE memory; frames is only read (the resident clips are never written).  Checked on the
 * host before any device call (SD_E_INVALID names the argument): NULL pointers, joints outside [2, 64],
 * obs_len / pred_len < 1, nseg < 1, total_frames < obs_len + pred_len, stride < 1, augmentation < 0,
 * pose_box_size <= 0, probabilities outside [0, 1], noise_std < 0, an unknown representation.  B == 0: SD_OK,
 * nothing launched.  sample_idx cannot be checked on the host: the kernel clamps the segment as above. */
#define SD_MOTION_VANILLA 0
#define SD_MOTION_CENTER_POSE 1
#define SD_MOTION_RESCALE_POSE 2
int sd_motion_batch(const float* frames, int64_t total_frames, const int64_t* seg_first, int64_t nseg,
                    const int64_t* sample_idx, int64_t B, int32_t joints, int32_t obs_len, int32_t pred_len,
                    int64_t stride, int64_t augmentation, int32_t train, int32_t representation, float pose_box_size,
                    float da_mirroring, float da_rotations, int32_t noisy, float noise_level, float noise_std,
                    const float* rot_table, uint64_t seed, int32_t epoch, const int32_t* draw_offset,
                    const uint8_t* draw_mirror, const int32_t* draw_degrees, const uint8_t* draw_noise_mask,
                    const float* draw_noise, float* obs, float* pred, int64_t* segment_idx, void* stream);
int sd_motion_draws(const int64_t* sample_idx, int64_t B, int32_t joints, int32_t obs_len, int64_t augmentation,
                    float da_mirroring, float da_rotations, float noise_level, float noise_std, uint64_t seed,
                    int32_t epoch, int32_t* offset, uint8_t* mirror, int32_t* degrees, uint8_t* noise_mask, float* noise,
                    void* stream);
int32_t sd_motion_batch_frame_tile(int32_t joints);

/* The forward process for k noisy copies of every training sequence: p_losses' repeat_interleave
 * of x_start / t (src/core/diffusion/base.py:262-268), get_white_noise and q_sample (nonisotropic.py:152-159,
 * isotropic.py q_sample) in one kernel.  x0 (nseq, J, D), t (nseq) i64, sqrt_alphas_cumprod (T); either
 * M (T, J, J) = Umm_sqrt_Lambda_bar_t or, with M NULL, sqrt_one_minus_alphas_cumprod (T):
 *   x_t[r, i, d] = sqrt_alphas_cumprod[t_s] x0[s, i, d] + sum_j M[t_s, i, j] eps[r, j, d]
 *   x_t[r, i, d] = sqrt_alphas_cumprod[t_s] x0[s, i, d] + sqrt_one_minus_alphas_cumprod[t_s] eps[r, i, d]
 * in f32, the products summed in this order by fused multiply-adds.
 * Rows: with sel NULL x_t (and noise_out) hold nseq k rows in repeat_interleave order, r = s k + copy; with
 * sel (nseq) i64 they hold nseq rows, the copy sel[s] of each sequence, bit for bit the rows s k + sel[s] of
 * the full launch.
 * Noise: with noise_in NULL, eps of a row comes from the sampler's Philox stream (sd_noise_fill) keyed
 * (seed, row = row0 + s k + copy, step), quad q = elements 4 q .. 4 q + 3 of the row's J D values; otherwise
 * noise_in (nseq k, J, D) is read at row s k + copy.  noise_out (optional, shaped like x_t) receives the eps
 * that was used.
 * All pointers are DEVICE memory, 16-byte aligned.  Checked on the host before any device call (SD_E_INVALID
 * names the argument): NULL pointers, misaligned rows, nseq < 0, k < 1, J outside [1, 64], D outside [4, 256]
 * or not a multiple of 4, T < 1, step outside [0, 2^31), row0 < 0, nseq k > 2^31 - 1, neither or both of M /
 * sqrt_one_minus_alphas_cumprod.  nseq == 0: SD_OK, nothing launched.  t and sel cannot be checked on the
 * host: the kernel clamps t to [0, T - 1] and sel to [0, k - 1], so neither becomes an out-of-bounds read. */
int sd_q_sample_groups(const float* x0, const int64_t* t, const float* sqrt_alphas_cumprod, const float* M,
                       const float* sqrt_one_minus_alphas_cumprod, int32_t T, int64_t nseq, int32_t k, int32_t J,
                       int32_t D, const int64_t* sel, const float* noise_in, uint64_t seed, int64_t step, int64_t row0,
                       float* x_t, float* noise_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SKELDIFF_H */

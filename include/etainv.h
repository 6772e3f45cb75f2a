/* etainv.h -- C ABI of the MI355X-native Eta-Inversion engine (libetainv_hip.so).
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json `north_star`: the
 * forward (DDIM inversion) / backward (eta-sampling) loop of furiosa-ai/eta-inversion's `etainv`
 * with the simple / prompt-to-prompt / MasaCtrl editors on an SD1.x UNet.  Every entry point
 * cites the reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  All tensor pointers are DEVICE pointers
 *     unless the parameter is documented as host.  Tensors are contiguous, NCHW where spatial.
 *   - `stream` is a hipStream_t passed as void* (e.g. torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, no hidden synchronisation, no per-call allocation.
 *   - ownership: the caller owns every buffer it passes; the library never frees or retains it
 *     past the call.  The engine handle owns its weights, workspace and attention-map store.
 *   - errors: every function returns 0 on success, non-zero otherwise; a thread-local message
 *     is available from etainv_last_error().  No C++ exception crosses the ABI.
 *   - threading: a handle is not thread-safe (the reference is single-threaded, one stream).
 *   - batch layout for B image pairs ("n_img"):  latents of the backward pass are 2*B rows
 *     [src_0..src_{B-1}, tgt_0..tgt_{B-1}]; UNet rows / contexts are 4*B rows
 *     [u_src x B, u_tgt x B, c_src x B, c_tgt x B].  With B = 1 this is exactly the reference's
 *     [u_s, u_t, c_s, c_t] (modules/inversion/diffusion_inversion.py:462-479).
 */
#ifndef ETAINV_H
#define ETAINV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ETAINV_ABI_VERSION 1
#define ETAINV_MAX_WORDS 77

enum etainv_dtype { ETAINV_F32 = 0, ETAINV_F16 = 1, ETAINV_BF16 = 2 };

int etainv_abi_version(void);
const char* etainv_last_error(void);

/* ---------------------------------------------------------------- elementwise step kernels
 * (usable without an engine handle; io_dtype is the element type of every tensor argument) */

/* eps = eps_u + g * (eps_c - eps_u).  Replaces the CFG combine of EtaInversion.predict_noise
 * (modules/inversion/eta_inversion.py:328). n = element count. */
int etainv_cfg_combine(const void* eps_u, const void* eps_c, float g, void* out, int64_t n,
                       int io_dtype, void* stream);

/* x' = sqrt(a_to) * (x - sqrt(1-a_from) eps)/sqrt(a_from) + sqrt(1-a_to) eps.
 * Replaces DDIMInverseScheduler.ddim_step (modules/inverse_schedulers/scheduling_ddim_inverse.py:71-100);
 * a_from/a_to are the alphas_cumprod the host looked up (clamp/negative rule :85-92). */
int etainv_ddim_step(const void* x, const void* eps, float a_from, float a_to, void* out, int64_t n,
                     int io_dtype, void* stream);

/* x' = DDIMScheduler.step(eps, t, x, eta, variance_noise) for `rows` latents ([3P] diffusers scheduler as called by
 * DiffusionInversion.step_backward, modules/inversion/diffusion_inversion.py:301-312, and with a per-pixel eta by
 * modules/inversion/eta_inversion.py:245).  eta_px = eta * eta_mask[row % n_mask][pixel] (eta_mask may be NULL);
 * noise [c*hw] is shared by all rows (may be NULL = no noise term). */
int etainv_ddim_eta_step(const void* x, const void* eps, float eta, const void* eta_mask, int n_mask, const void* noise,
                         float a_t, float a_p, float var, int rows, int c, int hw, void* out, int io_dtype, void* stream);

/* Fused backward step of EtaInversion.predict_step_backward (modules/inversion/eta_inversion.py:207-273)
 * for n_img independent (src,tgt) pairs, everything after the UNet call:
 *   CFG combine (:328) -> best-of-n variance noise on the source row (:330-375, argmin on device, NaN counts
 *   as minimal like torch.argmin) -> per-pixel eta = 1[mask_map > thres] * eta (:159-205,:236-243) ->
 *   DDIM-eta update of both rows ([3P] DDIMScheduler.step as called at :245) -> source row replay
 *   x_src += (x_prev_src - x_src) (:247-249; exact assignment when use_mask == 0, :260-261).
 * x        [2*n_img][chw]   current latents (rows src.., tgt..)
 * eps_all  [4*n_img][chw]   UNet output rows [u_s.., u_t.., c_s.., c_t..]
 * x_prev_src [n_img][chw]   stored inversion latent latents[-(k+2)] (:291)
 * noise    [n_cand][chw]    candidates drawn by sample_variance_noise (:145-156), shared by all images
 * mask_map [n_img][hw]      forward-pass mean attention map of the source edit word (may be NULL if !use_mask);
 *                            use_mask == 2: the map IS the per-pixel eta multiplier (non-default mask modes: no threshold,
 *                            `pow`, ground-truth mask -- eta_inversion.py:164-201), mask_thres ignored
 * a_t, a_p, var             alphas_cumprod[t], alphas_cumprod[t-Delta] (or final), _get_variance(t, t-Delta)
 * out_x    [2*n_img][chw]   new latents;  out_eps [2*n_img][chw] guided noise (may be NULL)
 * best_idx [n_img] int32, losses [n_img][n_cand] float (device, may be NULL); scratch: >= n_img*16*64 floats */
int etainv_eta_backward_step(const void* x, const void* eps_all, float g, const void* x_prev_src,
                             const void* noise, int n_cand, float eta, const void* mask_map, float mask_thres,
                             int use_mask, float a_t, float a_p, float var, int n_img, int c, int hw,
                             void* out_x, void* out_eps, int32_t* best_idx, float* losses, float* scratch,
                             int io_dtype, void* stream);
/* same + the reference's `target_dirinv` option (eta_inversion.py:251-256): x_tgt += target_dirinv * dirinv_map * (x_prev_src - x_src_new),
 * dirinv_map [n_img][hw] = 1 - mask_dirinv prepared by the caller (NULL = 1 everywhere); needs use_mask != 0 */
int etainv_eta_backward_step_ex(const void* x, const void* eps_all, float g, const void* x_prev_src, const void* noise, int n_cand, float eta,
                                const void* mask_map, float mask_thres, int use_mask, float a_t, float a_p, float var, int n_img, int c, int hw,
                                void* out_x, void* out_eps, int32_t* best_idx, float* losses, float* scratch, int io_dtype,
                                float target_dirinv, const void* dirinv_map, void* stream);

/* out = a x + b y + c z over n elements (z may be NULL): the latent update of the multistep DPM-Solver++ scheduler pair
 * (reference modules/inverse_schedulers/scheduling_dpmsolver_multistep_inverse.py:83-159 and the [3P] diffusers
 * DPMSolverMultistepScheduler.step behind DiffusionInversion.step_backward, modules/inversion/diffusion_inversion.py:279-312) */
int etainv_lincomb3(const void* x, float a, const void* y, float b, const void* z, float c, void* out, int64_t n, int io_dtype, void* stream);

/* ---- EDICT (coupled latent pair; reference modules/inversion/edict_inversion.py)
 * out = a * base + b * (eps_u + g * (eps_c - eps_u)): classifier-free guidance (DiffusionInversion.predict_noise) and the scheduler step of
 * EdictScheduler.step (:144-179, eta = 0) / EdictSchedulerInverse.step (:194-222) in one pass.  a, b are the host scalars of that step
 * (q = sqrt(abar_t / abar_prev); denoising: a = 1/q, b = sqrt(1-abar_prev) - sqrt(1-abar_t)/q; inversion: a = q,
 * b = sqrt(1-abar_t) - q sqrt(1-abar_prev)).  eps_u == NULL: no guidance, eps = eps_c (the guidance 0 / 1 case of predict_noise).
 * `out` may be `base`. */
int etainv_edict_couple(const void* base, const void* eps_u, const void* eps_c, float g, float a, float b, void* out, int64_t n,
                        int io_dtype, void* stream);
/* sync_latent_pair (:317-338), in place on the pair, in the reference's order.  inverse == 0 (denoising): x <- p x + (1-p) y, then
 * y <- (1-p) x_new + p y.  inverse == 1 (inversion): y <- (y - (1-p) x) / p, then x <- (x - (1-p) y_new) / p.  p in (0, 1]. */
int etainv_edict_mix(void* x, void* y, float p, int inverse, int64_t n, int io_dtype, void* stream);
/* tail of a denoising step (predict_step_backward :408-420): the second half-step's coupled update of x (base_is_y == 0) or y
 * (base_is_y == 1) followed by the mix; bit for bit etainv_edict_couple then etainv_edict_mix(inverse = 0) with fp32 tensors. */
int etainv_edict_couple_mix(void* x, void* y, int base_is_y, const void* eps_u, const void* eps_c, float g, float a, float b, float p,
                            int64_t n, int io_dtype, void* stream);

/* ---- regularised DDIM inversion (pix2pix-zero; reference modules/inversion/regularized_diffusion_inversion.py)
 * Everything of RegularizedDiffusionInversion.predict_step_forward (:116-137) after the UNet call, one launch, for n_img images of
 * [4][l][l] fp32: the CFG combine (eps_u NULL: eps_c already is the guided noise and g is ignored), regularize_noise_pred (:86-114:
 * num_reg_steps rounds of num_ac_rolls gradient steps on auto_corr_loss :42-69, each weighted lambda_ac / num_ac_rolls, and one gradient
 * step on kl_divergence :71-83 weighted lambda_kl -- both gradients in closed form, no autograd), and the DDIM inverse step of
 * etainv_ddim_step on the regularised noise (x NULL: no step; a_from / a_to as there).  eps_out receives the regularised noise and may be
 * eps_c.  shifts_dev, device int32 [num_reg_steps * num_ac_rolls][4][levels]: the roll amount of every autocorrelation step, channel and
 * pyramid level (fine to coarse; the levels are l, l/2, .. while a level is above 8), the reference's torch.randint(0, s // 2) draws in its
 * order; needed only when lambda_ac > 0 and both counts are positive.  8 <= l <= 96.  num_reg_steps == 0 or both lambdas <= 0: the noise
 * passes unchanged.  An image's result does not depend on n_img or on its position and is bit-identical from run to run. */
int etainv_noise_regularize(const float* eps_u, const float* eps_c, float g, float* eps_out, const float* x, float a_from, float a_to,
                            float* x_out, int n_img, int l, const int32_t* shifts_dev, int num_reg_steps, int num_ac_rolls,
                            float lambda_ac, float lambda_kl, void* stream);

/* ---- proximal negative-prompt inversion (reference modules/inversion/proximal_negative_prompt_inversion.py)
 * Everything of ProximalNegativePromptInversion.predict_noise (:130-151) after the UNet call, one launch, all tensors fp32:
 * d = eps_c - eps_u, the threshold, the shrinkage of proximal_guidance (:61-128), eps_out = eps_u + g d', and optionally the DDIM step of
 * etainv_ddim_step on eps_out (x NULL: no step; a_from / a_to as there; x and x_out have the rows of the noise).
 * Rows: n_groups groups of rows_per_group rows of [4][l][l]; row r of group j is tensor row r * n_groups + j (the [src.., tgt..] order of
 * etainv_eta_backward_step).  The n = rows_per_group * 4 * l * l values of a group share one threshold.  1 <= rows_per_group <= 4, 8 <= l <= 96.
 * mode 0: plain CFG (no threshold; bit-equal to mode 1 with a fixed threshold of 0); 1: "l0", d' = d - clamp(d, -thr, thr); 2: "l1", then
 * d' = d' > 0 ? d' - thr : d', then d' = d' < 0 ? d' + thr : d', in that order (:88-90, not symmetric).
 * Threshold, modes 1 and 2: use_rank != 0: torch.quantile of |d| over the group at the rank the host split into rank_lo = k in [0, n - 1]
 * and rank_w = w in [0, 1): thr = lerp(v_k, v_min(k+1, n-1), w) by torch's rule (v_k + w diff below w = 0.5, v_k+1 - diff (1 - w) from there),
 * v the exact order statistics (a radix select over the bit patterns; -0.0 counts as 0, +inf sorts last, a NaN anywhere in a group makes its
 * threshold and its noise NaN).  use_rank == 0: thr = thr_fixed >= 0.
 * eps_out may be eps_c (not eps_u).  thr_out (may be NULL): [n_groups][3] = (thr, v_k, v_k+1); with a fixed threshold all three are thr.
 * A group's result does not depend on n_groups or on its position and is bit-identical from run to run. */
int etainv_prox_guidance(const float* eps_u, const float* eps_c, float g, int mode, int use_rank, int rank_lo, float rank_w, float thr_fixed,
                         float* eps_out, const float* x, float a_from, float a_to, float* x_out, float* thr_out, int n_groups,
                         int rows_per_group, int l, void* stream);

/* ---- edit-friendly DDPM inversion (reference modules/inverse_schedulers/ddpm_inverse_scheduler.py, modules/inversion/ddpm_inversion.py)
 * All tensors fp32, device, 16-byte aligned; a latent is [4][l][l], chw = 4 l l, 8 <= l <= 96.  The schedule coefficients are float64 HOST tables
 * that the call reads before it returns (they travel in the kernel arguments): the caller may free them at once.  An element's result depends
 * on nothing but its own inputs and its step's scalars: not on the step count of the launch, where the chunk starts, n_img or its position.
 *
 * etainv_ddpm_sample_latents replaces DDPMInverseScheduler.sample_latents (ddpm_inverse_scheduler.py:86-129), one launch.
 *   x0 [n_img][chw]; noise [n_steps][n_img][chw] in the reference's draw order (ascending t); ab_host [n_steps][2] = (a, b) per step in that order;
 *   xts [n_steps + 1][n_img][chw] in the reference's index order: xts[n_steps - 1 - s] belongs to draw s (index 0 = the largest t), xts[n_steps] = x0.
 *   markovian == 0 (:118): x_t = x0 * a + r * b, a = sqrt(abar_t), b = sqrt(1 - abar_t).  markovian == 1 (:121-125): cur = cur * a + r * b from
 *   cur = x0, a = sqrt(abar_t / abar_prev), b = sqrt(1 - abar_t / abar_prev); every element walks the steps in its own thread.  Products and sum are
 *   rounded one by one, as torch does.  1 <= n_steps <= ETAINV_DDPM_MAX_STEPS.
 *
 * etainv_ddpm_invert_steps: everything of DDPMInverseScheduler.step (:156-199) after the UNet call for the k consecutive steps
 *   [first, first + k) of n_img images, one launch.  Step j reads x_t = xts[first + j] and x_{t-1} = xts[first + j + 1] (xts as above, n_steps
 *   its step count).  eps_u, eps_c [k][n_img][chw]: eps = eps_u + g (eps_c - eps_u); eps_u NULL: eps_c already is the noise, g is ignored.
 *   coef_host [k][5] = (sqrt(1 - abar_t), sqrt(abar_t), sqrt(abar_prev), sqrt(1 - abar_prev - sigma^2), sigma), sigma = sqrt(get_variance(t)):
 *     x0_pred = (x_t - c0 eps) / c1;  mu = c2 x0_pred + c3 eps;  z = (x_{t-1} - mu) / sigma;  x_out = mu + sigma z   (:178-196, that operation
 *   order, every operation rounded to fp32).  Outputs z, x_out, eps_out (the guided noise; may be NULL), each [k][n_img][chw].
 *   DELIBERATE DEVIATION, sigma == 0: the reference divides by zero there (t = 0 under steps_offset = 0, this pipeline's scheduler): z and the
 *   latent become NaN / inf.  Here z = 0 and x_out = mu.  The reference zeroes that step's z afterwards (ddpm_inversion.py:101) and never reads
 *   its latent.  1 <= k <= ETAINV_DDPM_MAX_CHUNK.
 *
 * etainv_ddpm_backward_step: everything of DDPMInversion.predict_step_backward (ddpm_inversion.py:135-166) after the UNet call, one launch:
 *   classifier-free guidance with one scale per prompt (:154-161; the reference's [guidance_scale_fwd, guidance_scale_bwd] for [source, target]
 *   is n_prompts == 2), then DDIMScheduler.step(eta = 1, variance_noise = z) (:162).  x, eps_u, eps_c, out_x, out_eps (may be NULL):
 *   [n_prompts * n_img][chw], rows [p0 x n_img, p1 x n_img, ..]; g_host [n_prompts] HOST floats, 1 <= n_prompts <= 4; z [n_img][chw] is shared by
 *   the prompt rows of an image; a_t, a_p, var as in etainv_ddim_eta_step.  Bit-equal to etainv_cfg_combine per prompt followed by
 *   etainv_ddim_eta_step(eta = 1, noise = z) per image on fp32 tensors.
 *
 * Refused (etainv_last_error says why): a null pointer other than the optional ones, l outside [8, 96], n_steps / k / n_img < 1, a step range
 * outside the schedule, n_prompts outside [1, 4], a non-finite scale or coefficient, a pointer that is not 16-byte aligned. */
#define ETAINV_DDPM_MAX_STEPS 256
#define ETAINV_DDPM_MAX_CHUNK 128
int etainv_ddpm_sample_latents(const float* x0, const float* noise, const double* ab_host, int markovian, float* xts, int n_steps, int n_img,
                               int l, void* stream);
int etainv_ddpm_invert_steps(const float* xts, int n_steps, int first, int k, const float* eps_u, const float* eps_c, float g,
                             const double* coef_host, float* z, float* x_out, float* eps_out, int n_img, int l, void* stream);
int etainv_ddpm_backward_step(const float* x, const float* eps_u, const float* eps_c, const float* g_host, int n_prompts, const float* z,
                              float a_t, float a_p, float var, float* out_x, float* out_eps, int n_img, int l, void* stream);

/* ---- image metrics of saved edits (reference metrics/, compute_metrics.py)
 * The four metrics of EditMetric that need no pretrained network, for b independent pairs in one call: MSEMetric (metrics/metrics.py:7-17),
 * PSNRMetric (:23-34), MSSSIM (metrics/msssim.py:61-106, :168-247 with data_range 1) and SSIM (metrics/ssim.py:8-30, which is
 * torchmetrics.image.StructuralSimilarityIndexMeasure() with its defaults [3P]: restated from its documented behaviour, not run here).
 * pred, target: fp32 [b][3][h][w] in the range (lo, hi); x' = (x - lo) / (hi - lo) is applied inside the kernels.  out: fp32 [b][4] =
 * (mse, psnr, ssim, msssim) per pair; mask picks the metrics (1 mse, 2 psnr, 4 ssim, 8 msssim), the others' slots receive NaN.
 *   mse    mean of (pred' - target')^2 over the 3 h w elements;  psnr = 10 log10(1 / mse), +inf for identical images
 *   window 11 taps, exp(-(i - 5)^2 / (2 * 1.5^2)) normalised, built in float32; applied along H, then along W, without padding.  With
 *          mu = E[.], sigma = E[..] - mu mu under that window:  cs = (2 sigma12 + C2) / (sigma11 + sigma22 + C2),
 *          ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs,  C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *   msssim R = 1; five levels, between them a 2 x 2 average pool with padding size % 2 whose zeros count in the divisor; per channel the mean
 *          of cs (levels 0-3) and of ssim (level 4), each clamped at 0, raised to 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 and multiplied; the
 *          mean over the channels.  Needs min(h, w) > 160.
 *   ssim   R = max(max pred' - min pred', max target' - min target') of the pair (torchmetrics' data_range=None); reflect padding by 5 and
 *          cropping 5 again is the unpadded window; the mean over all channels and window positions, no clamp.  Needs h, w >= 11.  R = 0 (two
 *          constant images, where torchmetrics divides 0 by 0): the structure term is 1, C1 = 0, and 0 / 0 is 1.
 * Arithmetic is float64 from the normalisation on, rounded to fp32 at the end; sums run in a fixed order without atomics: a pair's results do
 * not depend on b, on its position or on mask, and are bit-identical from run to run.  workspace: a device buffer of at least
 * etainv_image_metrics_workspace_bytes(b, h, w, mask) bytes (-1: refused, see etainv_last_error), 8-byte aligned; its contents mean nothing
 * between calls.  b <= 21845, h, w <= 16384. */
int64_t etainv_image_metrics_workspace_bytes(int b, int h, int w, int mask);
int etainv_image_metrics(const float* pred, const float* target, int b, int h, int w, float lo, float hi, int mask, float* out,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- CLIP metrics (reference metrics/clip_similarity.py): image preprocessing, the ViT's attention, the embedding head and the scores.  The
 * towers' GEMMs, LayerNorms and quick-GELU are the etainv_op_* entry points further down.
 *
 * etainv_clip_preprocess: torch_to_pil (clip_similarity.py:223-239) and clip's transform (:201) for b square images in one launch.
 *   x [b][3][s][s] fp32 in (lo, hi) -> (x - lo) / (hi - lo), * 255, clamped to [0, 255] and TRUNCATED to a byte -> Pillow's bicubic resize s -> r
 *   on bytes (horizontal pass into bytes, then the vertical pass) -> / 255, - mean, / std (the published constants; float64, rounded once) -> the ViT's patch
 *   rows rows_out [b (r / p)^2][Kp] in `dtype`: element k = c p^2 + py p + px (patch_embedding.weight.reshape(d, 3 p^2)), Kp = 3 p^2 rounded up
 *   to 64, zero from 3 p^2 on.  u8_out (optional): the resized bytes [b][3][r][r].
 *   The resampling is integer arithmetic on the caller's tables, built in float64 as Pillow builds them: bounds_* [r][2] = (first tap, taps),
 *   coef_* [r][ksize_*] = the normalised a = -0.5 bicubic weights as int(w 2^22 +- 0.5); a byte is clip8((2^21 + sum w px) >> 22).  s == r:
 *   one tap of weight 2^22 (Pillow does not resample).  max_rows: the most input rows a band of p output rows spans; max_rows (s + r) bytes of
 *   LDS must fit in 65536.  Table values are clamped where they are used: a wrong table gives wrong pixels, never an access out of bounds.
 *   Refused: a null pointer other than u8_out, p outside {14, 16, 32}, r not a multiple of p, a band that does not fit.
 * etainv_clip_assemble_tokens: out [b][1 + g2][d] = (cls | patches [b][g2][d]) + pos [1 + g2][d]  (the ViT's embeddings module).
 * etainv_op_vit_attention: softmax(q k^T / 8) v without a mask, qkv [b][n][3 heads 64] -> out [b][n][heads 64] (the layout of
 *   etainv_op_causal_attention), any n >= 1; rows >= n are never read.  16-bit: MFMA flash kernel, fp32 online softmax, P rounded to the operand
 *   type.  fp32: FMA twin.  Refused: head_dim != 64, a null or not 16-byte aligned pointer.
 * etainv_clip_embed_head: model.encode_image / encode_text's last step and the division by the norm (clip_similarity.py:204-205, :119-120).
 *   Row i of x [b][n][d] (x_dtype) at token index[i] (null: token 0) -> LayerNorm(gamma, beta, eps) when gamma is given -> proj [p][d]
 *   (w_dtype, no bias) -> divided by its L2 norm -> out fp32 [b][p].  fp32 accumulation in a fixed order; a row's result does not depend on b.
 * etainv_clip_similarity: the dot products of CLIPSimilarity.forward (:257-273) and the comparison of CLIPAccuracy.forward (:317-321) for b
 *   pairs.  img_* [b][p], txt_* [b][t][p] unit embeddings; a prompt's t embeddings are averaged and renormalised (:118-125).  mode 0 text_img =
 *   <img_tgt, txt_tgt>; 1 img_img = <img_src, img_tgt>; 2 textdir_imgdir = <img_tgt - img_src, txt_tgt - txt_src> (differences not
 *   renormalised, :263-265); 3 text_img_acc = 1 if <img_tgt, txt_tgt> > <img_tgt, txt_src> else 0.  out fp32 [b]; mode 4: all four of every
 *   pair in one launch, out fp32 [b][4] in that order, each value bit-identical to its own mode's.  float64 arithmetic, fixed
 *   order.  Refused: an unknown mode, t < 1, a null pointer the mode needs. */
int etainv_clip_preprocess(const float* x, int b, int s, int r, int p, float lo, float hi, const int32_t* bounds_h, const int32_t* coef_h,
                           int ksize_h, const int32_t* bounds_v, const int32_t* coef_v, int ksize_v, int max_rows, void* rows_out,
                           uint8_t* u8_out, int dtype, void* stream);
int etainv_clip_assemble_tokens(const void* patches, const void* cls, const void* pos, void* out, int b, int g2, int d, int dtype, void* stream);
int etainv_op_vit_attention(const void* qkv, void* out, int b, int n, int heads, int d, int dtype, void* stream);
int etainv_clip_embed_head(const void* x, int x_dtype, const int32_t* index, int b, int n, int d, const float* gamma, const float* beta, float eps,
                           const void* proj, int w_dtype, int p, float* out, void* stream);
int etainv_clip_similarity(const float* img_src, const float* img_tgt, const float* txt_src, const float* txt_tgt, int b, int t, int p, int mode,
                           float* out, void* stream);

/* ---- dinovitstruct (reference metrics/dino_vit_structure.py): image preprocessing, the erf GELU of the DINO blocks and the fused key
 * self-similarity distance.  The DINO ViT tower runs on etainv_op_gemm / etainv_op_layernorm, etainv_clip_assemble_tokens and etainv_op_vit_attention.
 *
 * etainv_dino_preprocess: SimpleMetric._normalize, Resize(224) on a float tensor and the ImageNet normalisation (dino_vit_structure.py:236-241)
 *   for b square images in one launch.  x [b][3][s][s] fp32 in (lo, hi) -> (x - lo) / (hi - lo) -> the separable resize s -> r in fp32 (horizontal
 *   pass, then vertical; one FMA per tap) -> (v - mean) / std with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225), in float64, rounded
 *   once -> the ViT's patch rows rows_out [b (r / p)^2][3 p^2] in `dtype`: element k = c p^2 + py p + px (patch_embed.proj.weight.reshape(d, 3 p^2)).
 *   Nothing is quantised to bytes.  The tables are the caller's, built in float64: bounds_* [r][2] = (first tap, taps), coef_* [r][ksize_*] fp32
 *   weights that sum to 1 -- torch's antialiased bilinear weights, or the two taps of antialias=False.  max_rows: the most input rows a band of p
 *   output rows spans; max_rows r 4 bytes of LDS must fit in 65536 (512 -> 224 at p = 8 needs 21 rows).  Table values are clamped where they are
 *   used: a wrong table gives wrong pixels, never an access out of bounds.  Refused: a null or misaligned pointer, p outside {8, 16}, r not a
 *   multiple of p, b above 65535, a band that does not fit.
 * etainv_op_gelu_erf: out = x Phi(x), the exact GELU, element-wise (in place allowed); erf to 1.8e-7 (gelu_pair).
 * etainv_dino_selfsim_mse: attn_cosine_sim (:15-20) of the source's and the edit's keys and F.mse_loss between the two (:262), for b pairs.
 *   keys [2 b][n][ld] in `dtype` with d used columns per row: rows 0 .. b-1 the sources' keys, b .. 2 b-1 the edits'.  With
 *   sim[i][j] = <k_i, k_j> / max(|k_i| |k_j|, eps) (the clamp is on the PRODUCT of the norms; a zero key gives 0),
 *   scores_out[pair] = mean over all n^2 (i, j) of (sim_edit - sim_source)^2, float64.  norms_out (optional): the fp32 row norms [2 b][n].
 *   Dots accumulate in fp32 (16-bit: MFMA over 64 x 64 tiles with j-tile >= i-tile, off-diagonal tiles counted twice; fp32: FMA twin), the
 *   cosines are fp32, their difference, its square and every sum float64 in a fixed order without atomics: a pair's score does not depend on
 *   b or on its position and is bit-identical from run to run.  Neither n x n matrix is written.  workspace: a device buffer of at least
 *   etainv_dino_selfsim_workspace_bytes(b, n) bytes (-1: refused), 8-byte aligned; its contents mean nothing between calls.
 *   Refused: a null pointer other than norms_out, keys not 16-byte aligned, d not a multiple of 64, ld < d or ld rows not whole 16-byte
 *   vectors, eps <= 0, b above 32767, n above 16384, a workspace too small. */
int etainv_dino_preprocess(const float* x, int b, int s, int r, int p, float lo, float hi, const int32_t* bounds_h, const float* coef_h,
                           int ksize_h, const int32_t* bounds_v, const float* coef_v, int ksize_v, int max_rows, void* rows_out, int dtype,
                           void* stream);
int etainv_op_gelu_erf(const void* x, void* out, int64_t n, int dtype, void* stream);
int64_t etainv_dino_selfsim_workspace_bytes(int b, int n);
int etainv_dino_selfsim_mse(const void* keys, int b, int n, int d, int64_t ld, float eps, double* scores_out, float* norms_out, void* workspace,
                            int64_t workspace_bytes, int dtype, void* stream);

/* ---- dinovitstruct_v2 (reference metrics/dino_vit_structure.py:32-34, :120-122, :141-160: the same metric on a DINOv2 ViT, patch 14): what the
 * DINOv2 tower needs beyond the dinovitstruct section above.  Its position embeddings are interpolated once per model on the host.
 *
 * etainv_dinov2_preprocess: etainv_dino_preprocess for patch 14.  rows_out [b (r / 14)^2][ETAINV_DINOV2_KP] in `dtype`: element
 *   k = c 196 + py 14 + px for k < 588; columns 588 .. 639 are written as zero (588 is no whole number of GEMM K steps; the patch weight is
 *   padded to match).  Tables, clamping and the LDS need (max_rows * r * 4 bytes, at most 65536) are those of etainv_dino_preprocess.
 *   Refused: a null or misaligned pointer, r not a multiple of 14, b above 65535, hi <= lo, a band that does not fit.
 * etainv_op_layerscale_add_layernorm: DINOv2's residual step x + ls.gamma * branch(x) and the LayerNorm behind it, in one pass.  Per row of c:
 *   x_out = x + ls_gamma * y with one fp32 FMA per element, rounded once to `dtype`; h_out = LayerNorm(x_out AS STORED; ln_gamma, ln_beta, eps),
 *   exact two-pass mean and variance in fp32.  In fp16 and bf16, h_out equals etainv_op_layernorm(x_out) bit for bit.  ls_gamma stays fp32: it is
 *   never folded into 16-bit weights (trained values reach 1e-5 and below).  x_out may be null (h_out alone is written) and may be x (in
 *   place: a wave reads its whole row before it writes); h_out is required and must be a buffer of its own.  One wave per row, fixed summation
 *   order, no atomics: bit-identical from run to run.  Refused: a null y / ls_gamma / x / ln_gamma / ln_beta / h_out, c not a multiple of 8 or
 *   above 1536, y / x / x_out / h_out / ls_gamma not 16-byte aligned. */
#define ETAINV_DINOV2_KP 640
int etainv_dinov2_preprocess(const float* x, int b, int s, int r, float lo, float hi, const int32_t* bounds_h, const float* coef_h, int ksize_h,
                             const int32_t* bounds_v, const float* coef_v, int ksize_v, int max_rows, void* rows_out, int dtype, void* stream);
int etainv_op_layerscale_add_layernorm(const void* y, const float* ls_gamma, const void* x, const float* ln_gamma, const float* ln_beta, float eps,
                                       void* x_out, void* h_out, int rows, int c, int dtype, void* stream);

/* ---- lpips, bglpips (reference metrics/metrics.py:40-61, metrics/bglpips.py:27-52 and :141-148; LPIPS v0.1, net='alex', lpips=True,
 * spatial=False, eval mode): image preprocessing, the AlexNet tower's convolution and pooling, and the per-tap distance.
 *
 * etainv_lpips_preprocess: `_normalize`, `* 2 - 1` (metrics.py:51-60, bglpips.py:142-146), the background mask (bglpips.py:49-51, :91) and
 *   LPIPS's scaling layer for n images in one launch.  x [n][3][h][w] fp32 in (lo, hi) -> v = 2 (x - lo) / (hi - lo) - 1 -> (mask given)
 *   v (1 - mask[i % n_mask]), mask [n_mask][h][w] fp32 with foreground = 1: applied after the map to [-1, 1], so the foreground becomes 0 ->
 *   (v - shift) / scale with shift (-.030, -.088, -.188), scale (.458, .448, .450) -> out [n][h][w][4] NHWC in `dtype`, the fourth channel 0.
 *   The arithmetic is float64, rounded once.  n_mask is read only when mask is given.  h != w is allowed.
 * etainv_op_conv2d_relu: torchvision AlexNet `features` convolutions (conv 11x11 stride 4 pad 2, 5x5 pad 2, 3x3 pad 1) with their ReLU, as one
 *   implicit GEMM over NHWC: x [n][h][w][cin], w [cout][kh kw][cin] (etainv_op_pack_weight mode 1 of the OIHW tensor; conv1: a zero fourth
 *   input channel), bias [cout] fp32 or null, out [n][ho][wo][cout] with ho = (h + 2 pad - kh) / stride + 1 (floor), relu != 0: max(., 0).
 *   kh, kw <= 11, stride 1 or 4, pad <= 2; fp32 accumulation on MFMA (fp32 operands: the f32-input matrix instruction, the parity mode).  The
 *   kernel gathers its own activation tile; nothing is im2col'ed to memory.  Refused before any launch: a null or misaligned pointer (x, w, out
 *   16 bytes), an output smaller than 1 x 1, cin other than 4 or a multiple of 32, cout not a multiple of 4, a stride, pad or kernel size outside
 *   the above.
 * etainv_op_maxpool3s2: MaxPool2d(3, 2) of `features` (floor mode, no pad) over NHWC [n][h][w][c] -> [n][(h - 3) / 2 + 1][(w - 3) / 2 + 1][c];
 *   any sign of input; c a whole number of 16-byte vectors.
 * etainv_lpips_layer_distance: LPIPS's normalize_tensor, `lin` layer and spatial_average for one tap of b pairs.  feats [2 b][pixels][c] in
 *   `dtype`: rows 0 .. b-1 the sources' features, b .. 2 b-1 the edits'; lin_w [c] fp32 (no bias).  Per pixel alpha = sqrt(sum_c a_c^2) + 1e-10
 *   (the epsilon is added to the norm), beta likewise; out[pair] (+)= mean over the pixels of sum_c lin_w[c] (a_c / alpha - b_c / beta)^2,
 *   float64 from the loaded features on, every sum in a fixed order without atomics.  accumulate = 1 adds to out[pair] (the five taps, in the
 *   caller's order), 0 overwrites.  Bit-identical from run to run and for any b; exactly 0.0 for identical features; unchanged when the sides
 *   are swapped.  workspace: at least etainv_lpips_distance_workspace_bytes(b, pixels) bytes (-1: refused), 8-byte aligned. */
int etainv_lpips_preprocess(const float* x, const float* mask, int n, int n_mask, int h, int w, float lo, float hi, void* out, int dtype,
                            void* stream);
int etainv_op_conv2d_relu(const void* x, const void* w, const float* bias, void* out, int n, int h, int wd, int cin, int cout, int kh, int kw,
                          int stride, int pad, int relu, int dtype, void* stream);
int etainv_op_maxpool3s2(const void* x, void* out, int n, int h, int w, int c, int dtype, void* stream);
int64_t etainv_lpips_distance_workspace_bytes(int b, int pixels);
int etainv_lpips_layer_distance(const void* feats, const float* lin_w, int b, int pixels, int c, int accumulate, double* out, void* workspace,
                                int64_t workspace_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------- engine */
typedef struct etainv_engine etainv_engine_t;

typedef struct etainv_engine_config {
  int compute_dtype;      /* ETAINV_F16 / ETAINV_BF16: MFMA operand type (fp32 accumulate); ETAINV_F32: fp32 operands on
                           * v_mfma_f32_32x32x2_f32, fp32 activations -- the reference's default precision (edit_image.py:147),
                           * 1/16 of the 16-bit matrix rate: the parity mode                                              */
  int max_unet_batch;     /* largest number of UNet rows per call (4 * n_img for the backward pass)      */
  int latent_size;        /* L: 64 for 512x512, 96 for 768x768; multiple of 8                           */
  int max_img;            /* largest n_img (attention-map store is sized for it)                        */
  int reserved[4];
} etainv_engine_config;

/* Memory: weights + one activation workspace are allocated here and freed by etainv_engine_destroy; calls never allocate,
 * except two process-wide one-time buffers of the GEMM launcher (a 256-byte zero page for the 3x3 halo and a 64 MiB split-K
 * workspace, created by the first launch that needs them).  One engine per device and process; not thread-safe. */
int etainv_engine_create(const etainv_engine_config* cfg, etainv_engine_t** out);
int etainv_engine_destroy(etainv_engine_t* e);

/* Weights: the engine enumerates the SD1.x UNet parameters under their diffusers state-dict names
 * (what `model.unet` holds in the reference, modules/models/__init__.py:135).  The caller uploads each as a
 * contiguous fp32 DEVICE buffer in diffusers layout; the engine converts / re-lays-out on `stream`. */
int etainv_engine_num_weights(etainv_engine_t* e);
int etainv_engine_weight_info(etainv_engine_t* e, int i, char* name, int name_cap, int64_t shape[4], int* ndim);
int etainv_engine_set_weight(etainv_engine_t* e, const char* name, const float* data, int64_t numel, void* stream);
int etainv_engine_weights_ready(etainv_engine_t* e); /* 1 when every parameter has been set */

/* Declarative attention control for one UNet call: replaces the per-layer Python callbacks installed by
 * register_attention_control (modules/utils/ptp_utils.py:196-302) and register_attention_editor_diffusers
 * (modules/utils/masactrl_utils.py:74-153).  Device pointers; per-image tables have n_img rows. */
enum etainv_attn_mode { ETAINV_ATTN_PLAIN = 0, ETAINV_ATTN_STORE = 1, ETAINV_ATTN_PTP = 2, ETAINV_ATTN_MASA = 3, ETAINV_ATTN_PNP = 4 };

typedef struct etainv_attn_ctrl {
  int mode;
  int n_img;
  /* STORE / PTP: accumulate the cond-half cross-attention probabilities of the layers the store keeps -- the five (L/4)^2-token layers by default,
   * the (L/2)^2 or (L/8)^2 ones after etainv_maps_configure -- (AttentionStore, modules/utils/ptp.py:143-183) into the engine's map store. */
  int store_maps;
  /* PTP cross edit (AttentionControlEdit.forward, modules/utils/ptp.py:205-218; Refine :245-258; Reweight
   * :261-274; Replace :234-242).  cross_alpha is the row of cross_replace_alpha for the current step. */
  const int32_t* mapper;      /* [n_img][77] or NULL */
  const float* alphas;        /* [n_img][77] or NULL */
  const float* replace_mat;   /* [n_img][77][77] or NULL (AttentionReplace) */
  const float* equalizer;     /* [n_img][77] or NULL */
  const float* cross_alpha;   /* [n_img][77] */
  /* PTP self edit: target probabilities := source probabilities when active and N <= self_max_tokens */
  int self_replace_active;
  int self_max_tokens;        /* 32^2 at L = 64 (modules/utils/ptp.py:226) */
  /* MASA: mutual self-attention active for transformer blocks >= masa_first_block (cur_att_layer // 2) */
  int masa_active;
  int masa_first_block;
  /* PTP only: the call carries rows [first_row, 4 n_img) of the [u_s, u_t, c_s, c_t] x n_img layout -- 0 (all rows) or n_img (no uncond source rows:
   * n_rows == 3 n_img, rows [u_t, c_s, c_t]).  A backward step whose eta(t) is 0 does not need eps(uncond source): the source row is replayed from the
   * inversion trajectory (modules/inversion/eta_inversion.py:247-249) and its guided noise only feeds the best-of-n choice of a noise that is then
   * multiplied by eta = 0 (:232, :330-375); the cond source row stays (its attention probabilities are what prompt-to-prompt injects). */
  int first_row;
  /* PTP with first_row = n_img only.  != 0: the 3 n_img rows are ordered [u_t, c_t, c_s] and the cond source rows LEAVE the network after transformer block
   * `src_exit_block` (execution order 0..15): from there on only the first 2 n_img rows are computed and the last n_img rows of `out` are not written.
   * For backward steps with eta == 0 in which nothing is injected from the source any more (cross_replace_alpha row all zero, self-replace over): the
   * cond source row then only feeds the AttentionStore of the five (L/4)^2 cross layers (LocalBlend, modules/utils/ptp.py:37-39), the last of which is
   * block 9 -- its noise prediction is unused (the source latent is replayed).  Needs mapper == replace_mat == NULL; while self_replace_active the exit
   * must lie behind the last (L/2)^2-token self-attention (block 12); with store_maps it must not lie in front of the last layer the store keeps
   * (etainv_maps_configure: res_div 2 -> block 12, 4 -> block 9, 8 -> block 6) -- an earlier exit is an error, not a silent loss of maps. */
  int src_exit_block;
  /* PNP (plug-and-play; register_attention_control_efficient / register_conv_control_efficient, modules/utils/pnp_utils.py, under PnPUnetForward,
   * modules/utils/pnp.py): the call carries n_rows == 3 n_img rows [u_s, u_t, c_t] x n_img over n_lat == n_rows latents [src, tgt, tgt] x n_img -- the
   * reference cuts the cond source row and returns the uncond source noise in its place.  No store, no tables, first_row == src_exit_block == 0.
   * pnp_qk_active: in the self-attention of transformer blocks 8..15 (execution order; up_blocks[1].attentions[1, 2], up_blocks[2, 3].attentions[0..2]) the
   * target rows take Q and K of the u_s row of their image, V stays their own.  pnp_conv_active: in up_blocks[1].resnets[1] the conv2 output (bias
   * included, before the shortcut add) of the target rows is that of the u_s row of their image.  Both 0: the plain call. */
  int pnp_qk_active;
  int pnp_conv_active;
} etainv_attn_ctrl;

/* eps = UNet(latent, t, ctx).  Replaces `self.unet(latent_input, t, encoder_hidden_states=context)["sample"]`
 * (modules/inversion/eta_inversion.py:321).
 * latent  [n_lat][4][L][L]  io_dtype, 1 <= n_lat <= n_rows; UNet row r reads latent row r % n_lat (torch.cat([latent]*2), :320)
 * t_host  [n_rows] int64 HOST timesteps (one per UNet row)
 * ctx     [n_rows][77][768] io_dtype
 * out     [n_rows][4][L][L] io_dtype */
int etainv_unet_forward(etainv_engine_t* e, const void* latent, int n_lat, const int64_t* t_host, const void* ctx,
                        int n_rows, const etainv_attn_ctrl* ctrl, void* out, int io_dtype, void* stream);

/* Attention-map store (AttentionStore.attention_store restricted to what the default path reads:
 * the five (L/4)^2 cross layers; modules/utils/ptp.py:37-39, 288-303). */
int etainv_maps_reset(etainv_engine_t* e, void* stream);

/* Forward-pass word maps (ControllerAttentionStorePerStep.end_step, modules/inversion/eta_inversion.py:44-49;
 * get_attention_map, modules/editing/ptp_editor.py:43-85): for each image and each of n_tok token indices,
 * mean over the 40 head-layers of (store / steps_done), / max, bicubic -> LxL, clamp[0,1].
 * tokens [n_img][n_tok] int32 device.  out [n_img][n_tok][L][L] float: written (accumulate == 0) or
 * accumulated with weight `scale` (accumulate == 1; scale = 1/S gives the "fwd_mean" map, :392-396). */
int etainv_maps_word_maps(etainv_engine_t* e, int n_img, const int32_t* tokens, int n_tok, int steps_done,
                          float* out, int accumulate, float scale, void* stream);
/* same, for one role of the backward-pass store: row_sel 0 = source cond row, 1 = target cond row (the `bwd_source` /
 * `bwd_target` eta-mask sources, reference modules/inversion/eta_inversion.py:176-183 via ptp_editor.py:43-85) */
int etainv_maps_word_maps_role(etainv_engine_t* e, int n_img, const int32_t* tokens, int n_tok, int steps_done, int row_sel, float* out,
                               int accumulate, float scale, void* stream);

/* Which cross-attention layers the store keeps: res_div 4 (default) = the five (L/4)^2 layers [down, down, up, up, up]; 2 = the five (L/2)^2 layers
 * (same order; allocated on first use, 4x the default store); 8 = the mid block's (L/8)^2 layer.  Non-default `attn_res` of the eta mask
 * (modules/inversion/eta_inversion.py:161; aggregate_attention keeps the layers whose token count is res^2, modules/utils/ptp.py:288-303).  Clears the
 * store.  LocalBlend needs res_div 4. */
int etainv_maps_configure(etainv_engine_t* e, int res_div, void* stream);
/* etainv_maps_word_maps_role with `attn_from_where` (eta_inversion.py:162) as a mask over the stored layers: bit l = layer l of the order above
 * ("down" = 0x03, "up" = 0x1c, both = 0x1f; res_div 8: bit 0 = "mid").  A mask that selects no stored layer is an error (the reference fails in
 * torch.cat of an empty list, ptp.py:301). */
int etainv_maps_word_maps_ex(etainv_engine_t* e, int n_img, const int32_t* tokens, int n_tok, int steps_done, int row_sel, unsigned layer_mask,
                             float* out, int accumulate, float scale, void* stream);

/* LocalBlend (modules/utils/ptp.py:18-47) on the backward latents x [2*n_img][4][L][L] (in place, fp32):
 * blend_alpha [n_img][2][77] selects the blend-word tokens of (source, target) prompt. */
int etainv_local_blend(etainv_engine_t* e, float* x, int n_img, const float* blend_alpha, float thres, void* stream);

/* Workspace statistics for DESIGN.md / bench (bytes). */
/* The loops of DiffusionInversion.diffusion_forward / sample (reference modules/inversion/diffusion_inversion.py:388-418, 493-528) pass the SAME context
 * tensor to every UNet call.  enable = 1: etainv_unet_forward reuses the cross-attention K / V projections of the context when the context
 * pointer, row count and dtype equal the previous call's -- the caller promises not to change the buffer's contents in between and switches the
 * cache off (enable = 0) when the loop ends.  Off by default: every call projects the context it is given. */
int etainv_engine_cache_context(etainv_engine_t* e, int enable);
/* Generation of the context buffer: a cached projection is reused only while the generation equals the one it was computed under.  A caller
 * that rewrites the context tensor IN PLACE between two calls (same pointer, rows, dtype) bumps it; the built-in loops pass a fresh value per
 * loop.  The cache entry is recorded only after a forward has succeeded: an error half-way never leaves stale K / V behind. */
int etainv_engine_context_generation(etainv_engine_t* e, uint64_t generation);
/* Default since round 4 (ETAINV_QKV_HM=0 at engine creation switches it off): the fused QKV projection of a transformer block writes
 * three head-major planes [q|k|v][row][head][token][head_dim] where both its GEMM kernel and the self-attention kernel can (head_dim 40 / 80, 16-bit modes,
 * whole 256-row tiles inside one batch row), so that a 64-key tile is one contiguous block.  Same values, same arithmetic: results are bit-identical.
 * `launches` = how many QKV projections took that path since the engine was created. */
int etainv_engine_qkv_head_major_count(etainv_engine_t* e, long long* launches);
/* Read-only activation taps of etainv_unet_forward (per-block parity tests: tests/test_unet_blocks_gpu.py).  The tap points are the blocks of the
 * UNet graph in execution order, each named by the module of the diffusers UNet whose output it is: `time_embedding` (the [rows][1280] MLP output in
 * front of the SiLU), `conv_in`, `down_blocks.{i}.resnets.{j}` / `.attentions.{j}` / `.downsamplers.0`, `mid_block.resnets.0` / `.attentions.0` /
 * `.resnets.1`, `up_blocks.{i}.resnets.{j}` / `.attentions.{j}` / `.upsamplers.0`, `conv_norm_out` (GroupNorm + SiLU: what conv_out reads).
 * etainv_engine_tap_info: name, pixels per side and channels of one point; a tapped tensor is NHWC [rows][side * side][channels] in the compute dtype.
 * etainv_engine_set_tap: `dst` is device memory of at least max_unet_batch rows (refused otherwise, here and not in a forward); NULL clears the tap.
 * A set tap makes every forward enqueue one device-to-device copy of the block's output on the call's stream right after the block (behind the row
 * duplication where the context-independent prefix ran on half the rows); the forward's result does not change, and a forward without taps enqueues
 * nothing more than it did.  etainv_engine_tap_rows: the rows that were live at the point in the last forward (fewer than n_rows behind a
 * src_exit_block), set or not; -1 for a bad argument. */
int etainv_engine_tap_count(etainv_engine_t* e);
int etainv_engine_tap_info(etainv_engine_t* e, int point, char* name, int name_cap, int* side, int* channels);
int etainv_engine_set_tap(etainv_engine_t* e, int point, void* dst, int64_t capacity_bytes);
int etainv_engine_tap_rows(etainv_engine_t* e, int point);
int64_t etainv_engine_workspace_bytes(etainv_engine_t* e);
int64_t etainv_engine_weight_bytes(etainv_engine_t* e);

/* Opt-in per-kernel-class timing (HIP events recorded on the launch stream around every launch of the class).
 * Classes: 0 implicit-GEMM (conv/linear, work = FLOPs), 1 self-attention (FLOPs), 2 cross-attention (FLOPs),
 * 3 GroupNorm (bytes), 4 LayerNorm (bytes).  etainv_prof_read synchronises the device. */
int etainv_prof_enable(int on);
int etainv_prof_reset(void);
int etainv_prof_read(int cls, double* ms, double* work, int64_t* launches);
/* The individual launches of one class since the last reset, in launch order: fills ms[i], work[i] for i < min(n, cap) and
 * returns n through *launches (per-shape breakdown of a UNet call: tools/unet_call.py --shapes). */
int etainv_prof_records(int cls, double* ms, double* work, int64_t cap, int64_t* launches);
/* same + bytes[i] = the algorithmic HBM bytes of launch i (every operand read once, the result written once; 0 where the class records none) */
int etainv_prof_records_ex(int cls, double* ms, double* work, double* bytes, int64_t cap, int64_t* launches);

/* Roofline split of the launches of one class by arithmetic intensity (algorithmic FLOPs / algorithmic HBM bytes of each launch): out6 =
 * {ms, FLOPs, bytes} of the launches at or above `ridge` FLOP/byte (MFMA-bound), then of those below it (HBM-bound); launches2 = their counts.
 * Only the implicit-GEMM class records bytes. */
int etainv_prof_split(int cls, double ridge, double* out6, int64_t* launches2);

/* Per-op entry points used by the parity tests (tests/test_kernels_gpu.py) -- the same launchers the
 * executor uses, exposed so every kernel is checked against a plain fp32 reference in isolation.
 * Activations NHWC in the compute dtype; weights in the engine layouts described in DESIGN.md. */
int etainv_op_gemm(const void* a, const void* w, const void* bias, const void* residual, void* out,
                   int m, int n, int k, int geglu, int dtype, void* stream);
/* LayerNorm folded into the two GEMMs around it (reference: BasicTransformerBlock norm1/2/3 of [3P] diffusers 0.21.1 attention.py, called from
 * Transformer2DModel inside `self.unet(...)`, modules/inversion/eta_inversion.py:321).  The GEMM that writes the LayerNorm's input leaves per-row
 * (mean, M2) partials [m][P][2] in stat_out (*stat_p_out = P, each over n / P columns; 0 = this launch shape emits none: use etainv_op_row_stats);
 * etainv_op_ln_finalize turns them into stat[m] = (mean, rstd); the GEMM that consumes the LayerNorm runs on the RAW rows with the weights of
 * etainv_op_ln_fold: out = rstd (a W'^T - mean s) + c.  stat == NULL: a plain GEMM with bias c_vec. */
int etainv_op_gemm_ln(const void* a, const void* w_folded, const float* c_vec, const float* s_vec, const float* stat,
                      const void* residual, void* out, float* stat_out, int* stat_p_out, int m, int n, int k, int geglu,
                      int dtype, void* stream);
/* The LayerNorm-consumer GEMM above as the fused QKV projection of a transformer block launches it: where the launch shape allows, out is written as
 * three head-major planes [q|k|v][m / tokens][heads][tokens][head_dim] (*wrote_head_major = 1), otherwise row-major [m][n] (0).  n == 3 heads head_dim. */
int etainv_op_gemm_ln_hm(const void* a, const void* w_folded, const float* c_vec, const float* s_vec, const float* stat, void* out,
                         int m, int n, int k, int heads, int head_dim, int tokens, int* wrote_head_major, int dtype, void* stream);
/* W' = gamma . W (packed, compute dtype; geglu: the value / gate row interleave of the GEGLU projection), s = row sums of the rounded W',
 * c = beta W^T + bias (bias in logical row order, may be NULL) */
int etainv_op_ln_fold(const float* w, const float* gamma, const float* beta, const float* bias, int n, int k, int geglu, float scale,
                      void* w_out, float* s_out, float* c_out, int dtype, void* stream);
int etainv_op_row_stats(const void* x, float* stat, int rows, int c, float eps, int dtype, void* stream);
int etainv_op_ln_finalize(const float* partials, int p, int cw, float eps, float* stat, int rows, void* stream);
/* GroupNorm statistics from the producing GEMM's epilogue (reference: the GroupNorms of [3P] diffusers ResnetBlock2D / Transformer2DModel inside the
 * UNet call, eta_inversion.py:321): etainv_op_gemm_gnstat = etainv_op_gemm that also leaves per-channel (sum, sum of squares) partials of its stored
 * output, part[m / wm][2][n] (*wm_out rows per block; 0 = this launch shape emits none); etainv_op_groupnorm_pre = GroupNorm(+SiLU) of cat[x1, x2]
 * from such partials (no statistics pass over x); final_stats: b * (2 * groups + 2 * (c1 + c2)) floats of scratch ((mean, rstd) per group, then the
 * apply pass's per-channel scale / shift planes). */
int etainv_op_gemm_gnstat(const void* a, const void* w, const float* bias, const void* residual, void* out, float* part, int* wm_out, int m,
                          int n, int k, int rows_per_image, int dtype, void* stream);
/* etainv_op_conv3x3 (stride 1, single source, nine taps) that also leaves the GroupNorm partials of its stored output, as etainv_op_gemm_gnstat does for
 * the 1x1 layers: conv1 / conv2 of [3P] diffusers ResnetBlock2D feed the next GroupNorm (inside the UNet call of eta_inversion.py:321). */
int etainv_op_conv3x3_gnstat(const void* x_nhwc, const void* w_okkc, const float* bias, const float* rowvec, const void* residual, void* out,
                             float* part, int* wm_out, int b, int h, int wd, int cin, int cout, int dtype, void* stream);
int etainv_op_groupnorm_pre(const void* x1, const void* x2, int c1, int c2, const float* part1, int wm1, const float* part2, int wm2,
                            const float* gamma, const float* beta, void* out, int b, int hw, int groups, float eps, int silu,
                            float* final_stats, int dtype, void* stream);
/* conv3x3 behind a nearest-2x upsample (diffusers Upsample2D inside the UNet call of eta_inversion.py:321) in PHASE form: the nine taps on the upsampled image
 * are four 2x2 convs on the source image, one per output phase (y & 1, x & 1) -- taps that land on the same source pixel are summed in fp32 and rounded
 * once (4 / 9 of the FLOPs, the same result up to that rounding).  w_oc33 [cout][cin][3][3] fp32 -> dst [4][cout][4][cin] in the compute dtype; run it with
 * etainv_op_conv3x3(..., upsample = 2, taps = 4): the 256 x 160 ring only (h * wd % 256 == 0, enough rows; otherwise an error -- upsample = 1 is the 9-tap form). */
int etainv_op_pack_ups4(const float* w_oc33, void* dst, int cout, int cin, int dtype, void* stream);
int etainv_op_conv3x3(const void* x_nhwc, const void* x2_nhwc, int c1, int c2, const void* w_okkc, const void* bias,
                      const float* rowvec, const void* residual, void* out, int b, int h, int wd, int cout,
                      int stride, int upsample, int taps, int dtype, void* stream);
/* extended conv for the VAE: pad0 = taps start at the output origin (asymmetric (0,1,0,1) padding of its stride-2
 * downsamplers); out_nchw = 1..4: cout must be 4 and the first out_nchw channels are written as io-dtype NCHW */
int etainv_op_conv3x3_ex(const void* x_nhwc, const void* w_okkc, const void* bias, const void* residual, void* out, int b, int h,
                         int wd, int cin, int cout, int stride, int upsample, int pad0, int out_nchw, int out_io_dtype, int dtype,
                         void* stream);
/* VAE / CLIP text-encoder helpers (third-party networks outside the DDIM loop; reference call sites
 * modules/inversion/diffusion_inversion.py:183-247) */
int etainv_op_im2col3x3(const void* x_nchw, int io_dtype, int cin, int h, int w, int rows, const float* premix, void* out,
                        int dtype, void* stream);
int etainv_op_row_softmax(void* x, int rows, int n, float scale, int dtype, void* stream);
int etainv_op_quick_gelu(const void* x, void* out, int64_t n, int dtype, void* stream);
int etainv_op_embed(const int64_t* ids, const void* tok, const void* pos, int b, int n_pos, int d, void* out, int dtype,
                    void* stream);
int etainv_op_causal_attention(const void* qkv, void* out, int b, int n, int heads, int d, int dtype, void* stream);
int etainv_op_groupnorm(const void* x_nhwc, const void* x2_nhwc, int c1, int c2, const float* gamma,
                        const float* beta, void* out, int b, int hw, int groups, float eps, int silu,
                        float* scratch, int dtype, void* stream);
int etainv_op_layernorm(const void* x, const float* gamma, const float* beta, void* out, int rows, int c,
                        float eps, int dtype, void* stream);
/* mode 0 plain, 1 ptp self-replace, 2 masactrl (modes 1/2: b == 4*n_img rows [u_s,u_t,c_s,c_t]), 3 plug-and-play (b == 3*n_img rows [u_s,u_t,c_t]:
 * rows >= n_img take Q and K of row r % n_img, V stays their own).  A row count that does not fit the mode's layout is an error; nothing is launched. */
int etainv_op_self_attention(const void* qkv, void* out, int b, int n, int heads, int d, int mode, int n_img,
                             int dtype, void* stream);
/* The same launch with every argument the UNet passes.  q_prescaled: the queries already carry head_dim^-0.5 * log2(e) (head_dim 40 / 80, 16-bit types);
 * first_row: 0 = all 4 n_img rows (mode 3: all 3 n_img rows, the only value it takes), n_img = rows [u_t, c_s, c_t] (mode 1), < 0 = rows [u_t, c_t, c_s]
 * (mode 1, b == 3 n_img; see etainv_attn_ctrl);
 * head_major: qkv holds three planes [q|k|v][b][heads][n][d] instead of rows [b][n][3 heads d] (head_dim 40 / 80, 16-bit types; else an error). */
int etainv_op_self_attention_ex(const void* qkv, void* out, int b, int n, int heads, int d, int mode, int n_img,
                                int q_prescaled, int first_row, int head_major, int dtype, void* stream);
/* q [b][n][heads d], kv [b][n_ctx][2 heads d] (1 <= n_ctx <= 77), head_dim 40 / 80 / 160.  ctrl as in the UNet call: STORE = rows [u, c] x n_img or [c] x n_img;
 * PTP = rows [first_row, 4 n_img) of [u_s, u_t, c_s, c_t] x n_img, or, with src_exit_block != 0, rows [u_t, c_t, c_s] x n_img / [u_t, c_t] x n_img (store only).
 * mapper or replace_mat asks for the edit (needs cross_alpha); store_maps with map_layer >= 0 accumulates into maps_acc [layers][n_img_cap][2][heads][n][77].
 * A row count that does not fit the layout, an edit without cross_alpha and a store without maps_acc or with n_img > n_img_cap are errors; nothing is launched. */
int etainv_op_cross_attention(const void* q, const void* kv, void* out, int b, int n, int heads, int d,
                              int n_ctx, const etainv_attn_ctrl* ctrl, int map_layer, int n_img_cap,
                              float* maps_acc, int dtype, void* stream);
int etainv_op_word_maps(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, int n_img,
                        const int32_t* tokens, int n_tok, int steps_done, float* out, int accumulate, float scale,
                        void* stream);
int etainv_op_local_blend(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, float* x,
                          int n_img, const float* blend_alpha, float thres, void* stream);

/* etainv_op_word_maps with the two arguments the engine's launches also vary: row_sel (0 = source cond row, 1 = target cond row of the store) and
 * layer_mask (bit l = stored layer l; see etainv_maps_word_maps_ex) */
int etainv_op_word_maps_ex(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, int n_img,
                           const int32_t* tokens, int n_tok, int steps_done, int row_sel, unsigned layer_mask, float* out,
                           int accumulate, float scale, void* stream);
/* The small kernels at the edges of the UNet call (tests/test_small_kernels_gpu.py).
 * etainv_op_time_embedding: sinusoidal timestep embedding [rows][dim] (flip_sin_to_cos, freq_shift 0) of the HOST timesteps t_host [rows],
 *   passed by value in the kernel arguments.
 * etainv_op_silu: out = silu(x) over n elements (out == x allowed).  etainv_op_cast: dst = (dst_dtype) src over n elements.
 * etainv_op_im2col_in: latent NCHW [n_lat][4][l][l] io_dtype -> [rows][l*l][64] dtype, k = tap * 4 + ci, columns 36..63 zero; row r reads
 *   latent r % n_lat.
 * etainv_op_pack_weight: src fp32 [rows][cols] -> dst dtype; mode 0 copy, 1 conv OIHW [rows = O][cols = I * taps] -> [O][tap][I], 2 GEGLU row
 *   interleave, 5 conv_in [O][4][3][3] -> [O][64] (cols must be 36).  Modes 0, 1, 2: every element times `scale`, then (modes 0 / 2 only) times
 *   colscale[column] (may be NULL), in fp32, before the one rounding to dtype.  Mode 5 takes neither: scale must be 1 and colscale NULL.
 *   Refused: any other mode, cols % taps != 0 in mode 1, rows % 64 != 0 in mode 2. */
int etainv_op_time_embedding(const int64_t* t_host, int rows, int dim, void* out, int dtype, void* stream);
int etainv_op_silu(const void* x, void* out, int64_t n, int dtype, void* stream);
int etainv_op_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
int etainv_op_im2col_in(const void* latent, int io_dtype, int n_lat, int rows, int l, void* out, int dtype, void* stream);
int etainv_op_pack_weight(const float* src, void* dst, int64_t rows, int64_t cols, int mode, int taps, float scale, const float* colscale,
                          int dtype, void* stream);
/* Plug-and-play feature injection as resblock() launches it: of the activation x [rows][row_elems] (in place) every row r >= n_src becomes a copy of row
 * r % n_src; rows < n_src are only read.  Refused: null x, rows % n_src != 0, a row whose byte size is not a multiple of 16. */
int etainv_op_rows_broadcast(void* x, int rows, int n_src, int64_t row_elems, int dtype, void* stream);
/* etainv_op_gemm with an fp32 result [m][n]: the one GEMM of all time-embedding projections (ResnetBlock2D.time_emb_proj, n = 20160) */
int etainv_op_gemm_f32out(const void* a, const void* w, const float* bias, float* out_f32, int m, int n, int k, int dtype, void* stream);
/* etainv_op_conv3x3 whose time row is read as the UNet reads it: row i of rowvec starts at rowvec + i * rowvec_stride (a column block of that matrix) */
int etainv_op_conv3x3_rv(const void* x_nhwc, const void* x2_nhwc, int c1, int c2, const void* w_okkc, const void* bias,
                         const float* rowvec, int rowvec_stride, const void* residual, void* out, int b, int h, int wd, int cout,
                         int stride, int upsample, int taps, int dtype, void* stream);
/* GroupNorm (no activation) folded into the 1x1 conv behind it (Transformer2DModel.norm -> proj_in): stats [b][groups] (mean, rstd) pairs ->
 * wb [b][n][k] = W rstd gamma (compute dtype), cb [b][n] = W (beta - mean rstd gamma) + bias; etainv_op_gemm_per_image then multiplies the hw rows
 * of image i by wb[i] and adds cb[i] (hw must be a multiple of the kernel's M tile, else an error). */
int etainv_op_gn_fold(const float* w, const float* gamma, const float* beta, const float* bias, const float* stats, int groups, int b, int n,
                      int k, void* wb_out, float* cb_out, int dtype, void* stream);
int etainv_op_gemm_per_image(const void* a, const void* wb, const float* cb, const void* residual, void* out, int b, int hw, int n, int k,
                             int dtype, void* stream);
/* Which kernel the calling thread's last GEMM / conv launch (any etainv_op_* above that ends in one, or the engine's) took.  Host-side only: touches no
 * device state and launches nothing.  Writes up to n of {route, tile rows, tile columns, K split, form} into out and returns how many there are (5):
 * route indexes etainv_op_igemm_route_name ("ppconv", "dualn", "ring-ups4", "ring-ups9", "ring-patch", "ring", "ring-geglu", "two-slot", "fp32"), -1
 * before the first launch or after a refused one; form = 1 for ppconv's dual-M kernel, the epilogue kind 0..3 of a dual-N launch, else 0. */
int etainv_op_last_igemm_plan(int* out, int n);
const char* etainv_op_igemm_route_name(int route); /* NULL outside the list */

#ifdef __cplusplus
}
#endif
#endif /* ETAINV_H */

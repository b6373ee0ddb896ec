/*
 * vdiff.h -- C-ABI of libvdiff.so, the MI355X (gfx950) kernels behind the
 * video-diffusion denoiser hot path of wdas03/lipreading-video-generation.
 *
 * The reference has no FFI: its boundary is the Python module API of
 * video-generation/diffusion (unet.py, unet_audio.py, utils.py,
 * linear_noise_scheduler.py, noise_scheduler.py).  Every entry point below
 * replaces the ATen op(s) that the reference calls at the cited line; the
 * Python drop-in (lipreading-video-generation_amd/video-generation/diffusion)
 * binds them through ctypes.
 *
 * Conventions
 *  - All tensor arguments are caller-owned DEVICE pointers.  The library never
 *    allocates device memory; kernels that need scratch take a workspace
 *    pointer whose size is returned by the matching *_workspace_size().
 *  - Activations are channels-last: a [B, C, T, H, W] tensor is stored as
 *    [B][T][H][W][C] (C fastest).  2-D tensors use T = 1.
 *  - `stream` is a hipStream_t passed as void* (0 = null stream).  Every call
 *    is asynchronous and stream-ordered; nothing synchronises the host.
 *  - Return 0 on success, otherwise a VD_E* code; vd_last_error() returns a
 *    thread-local message describing the last failure.
 *  - dtype: VD_F32 (parity mode, fp32 storage, exact-fp32 MFMA / VALU math) or
 *    VD_BF16 (throughput mode, bf16 storage, fp32 accumulate/statistics).
 */
#ifndef VDIFF_H
#define VDIFF_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDIFF_ABI_VERSION 1

enum vd_status { VD_OK = 0, VD_EINVAL = 1, VD_EUNSUPPORTED = 2, VD_ELAUNCH = 3 };
enum vd_dtype { VD_F32 = 0, VD_BF16 = 1 };

/* ---- library ---------------------------------------------------------- */
int vd_version(void);
const char* vd_last_error(void);
/* Writes "name;gfx;CUs;HBM bytes" of the current device into buf. */
int vd_device_info(char* buf, int buflen);

/* ---- timestep embedding ------------------------------------------------
 * replaces utils.py:140-158 (timestep_embedding): out[b, i] =
 * cos(t_b * f_i) (i < dim/2), sin(t_b * f_{i-dim/2}) (i >= dim/2),
 * f_i = exp(-ln(max_period) * i / (dim/2)); zero column when dim is odd.
 * t: int64[B]; out: fp32[B, dim]. */
int vd_timestep_embedding(const int64_t* t, int B, int dim, float max_period,
                          float* out, void* stream);
/* Same, with the frequency table f[dim/2] (fp32, device) supplied by the caller -- the
 * reference computes it on the host (utils.py:150-152: torch CPU exp), so a caller that
 * builds it the same way gets the reference's bit-identical arguments t_b * f_i. */
int vd_timestep_embedding_tab(const int64_t* t, int B, int dim, const float* freqs,
                              float* out, void* stream);

/* ---- DDPM / DDIM scheduler math ----------------------------------------
 * Tables are fp32 device arrays of length num_timesteps; t is int64[B];
 * x tensors are [B][per_sample] in `dtype`.  z may be NULL where the
 * formula adds no noise.
 *
 * Alignment of the per-sample kernels -- ONE rule for every entry point of this group:
 * vd_q_sample, vd_p_sample_v1 / _v2 / _cosine, vd_ddim_step / _pred, vd_cfg_stats,
 * vd_cfg_combine, vd_ddim_step_cfg / _cfg_pred, vd_dpm_step / _cfg, vd_x0_abs_quantile,
 * vd_ddim_step_thr, vd_dpm_step_thr, vd_ddim_step_known, vd_dpm_step_known.  A call moves 8
 * elements per lane (16-byte accesses) when per_sample % 8 == 0 AND every non-null tensor
 * pointer it is given (inputs, outputs, the duplicate, the history) is 16-byte aligned; any
 * other call runs one element at a time, so element-aligned pointers are always legal.  Both
 * paths perform the same fp32 operations per element.  Tables, t / t_prev / step and the statistics workspace
 * need their natural alignment only.  (vd_mse_loss / _bwd, below, are stricter: they refuse
 * unaligned tensors with VD_EINVAL.)
 *
 * q_sample: linear_noise_scheduler.py:24-46 (add_noise)
 *   xt = sqrt_acp[t] * x0 + sqrt_1m_acp[t] * eps */
int vd_q_sample(const void* x0, const void* eps, void* xt, const int64_t* t,
                const float* sqrt_acp, const float* sqrt_1m_acp,
                int64_t B, int64_t per_sample, int dtype, void* stream);

/* ---- MSE loss (train.py:103 nn.MSELoss(), :130 loss = criterion(noise_pred, noise)) ----
 * out[0] = mean((pred - target)^2) over n elements of `dtype`, fp32, in a FIXED order:
 * per-block partial sums of fixed ranges into the caller's workspace
 * (vd_mse_loss_workspace_size(n) bytes), then one block sums them in block order.  Two
 * launches, no semaphore and no memset, so the value is identical eager and replayed from
 * a HIP graph.  pred / target 16-B aligned.
 * vd_mse_loss_bwd: grad_pred = 2 (pred - target) / n * grad_loss[0] (grad_loss: device fp32
 * scalar, the autograd seed; MSELoss.backward). */
size_t vd_mse_loss_workspace_size(int64_t n);
int vd_mse_loss(const void* pred, const void* target, int64_t n, int dtype, float* out,
                void* workspace, size_t workspace_bytes, void* stream);
int vd_mse_loss_bwd(const void* pred, const void* target, const float* grad_loss, int64_t n,
                    int dtype, void* grad_pred, void* stream);

/* ---- training objective: v-prediction and Min-SNR weighting (build extension; the reference
 * trains noise prediction with the unweighted MSE above) ----
 * Per sample b, with i = t[b] clamped into [0, T - 1], sa = sqrt_acp[i], s1m = sqrt_1m_acp[i]
 * (the tables vd_q_sample reads) and snr = (sa / s1m)^2:
 *   target  VD_PRED_EPS: eps;  VD_PRED_V: sa eps - s1m x0 (Salimans & Ho 2022), formed in
 *           registers, never written to memory;
 *   w_b     VD_WEIGHT_NONE: 1;  VD_WEIGHT_MIN_SNR (Hang et al. 2023): min(snr, gamma) / snr for
 *           eps, min(snr, gamma) / (snr + 1) for v;
 *   per_sample_mse[b] = 1 / P sum_i (pred - target)^2 (unweighted, fp32 [B]);
 *   loss[0] = 1 / B sum_b w_b per_sample_mse[b] (fp32).
 * pred, x0, eps: [B][per_sample] in `dtype` (x0 is not read for VD_PRED_EPS and may be NULL);
 * t: int64[B] on the device; B <= 65535.  vd_diffusion_loss is a FIXED-order reduction built to
 * the rules of vd_mse_loss / vd_cfg_stats: block k of sample b sums one fixed contiguous range
 * into workspace[b][k] (vd_diffusion_loss_workspace_size bytes), then one block adds each
 * sample's partials in block order and the weighted samples in sample order.  Two launches, no
 * atomics, no memset, no semaphore: the same bits eager and replayed from a HIP graph.
 * vd_diffusion_loss_bwd: grad_pred = grad_loss[0] 2 w_b / (B P) (pred - target) in `dtype`
 * (grad_loss: device fp32 scalar); one launch, target and w_b recomputed. */
enum vd_prediction { VD_PRED_EPS = 0, VD_PRED_V = 1 };
enum vd_loss_weighting { VD_WEIGHT_NONE = 0, VD_WEIGHT_MIN_SNR = 1 };
size_t vd_diffusion_loss_workspace_size(int64_t B, int64_t per_sample);
int vd_diffusion_loss(const void* pred, const void* x0, const void* eps, const int64_t* t,
                      const float* sqrt_acp, const float* sqrt_1m_acp, int64_t T,
                      int prediction, int weighting, float gamma, int64_t B,
                      int64_t per_sample, int dtype, float* loss, float* per_sample_mse,
                      void* workspace, size_t workspace_bytes, void* stream);
int vd_diffusion_loss_bwd(const void* pred, const void* x0, const void* eps, const int64_t* t,
                          const float* sqrt_acp, const float* sqrt_1m_acp, int64_t T,
                          int prediction, int weighting, float gamma, const float* grad_loss,
                          int64_t B, int64_t per_sample, int dtype, void* grad_pred,
                          void* stream);

/* p_sample V1: linear_noise_scheduler.py:48-76 (LinearNoiseScheduler.
 * sample_prev_timestep).  x0 = clamp((xt - s1m[t] eps) / sqrt(acp[t])),
 * mean = (xt - beta[t] eps / s1m[t]) / sqrt(alpha[t]); t == 0 returns mean,
 * else mean + sqrt((1-acp[t-1])/(1-acp[t]) * beta[t]) * z. */
int vd_p_sample_v1(const void* xt, const void* eps, const void* z,
                   void* x_prev, void* x0, const int64_t* t,
                   const float* betas, const float* alphas, const float* acp,
                   const float* sqrt_1m_acp, int64_t B, int64_t per_sample,
                   int dtype, void* stream);

/* p_sample V2: linear_noise_scheduler.py:91-101 (LinearNoiseSchedulerV2).
 * mean = xt - s1m[t] eps / sqrt(alpha[t]); sigma = sqrt((1-acp[t]) beta[t]);
 * x_prev = mean + sigma z (also at t == 0); x0 = clamp((xt - s1m[t] eps)/sa[t]). */
int vd_p_sample_v2(const void* xt, const void* eps, const void* z,
                   void* x_prev, void* x0, const int64_t* t,
                   const float* betas, const float* alphas, const float* acp,
                   const float* sqrt_acp, const float* sqrt_1m_acp,
                   int64_t B, int64_t per_sample, int dtype, void* stream);

/* p_sample cosine: noise_scheduler.py:13-29 (CosineNoiseScheduler).
 * mean = (xt - s1m[t] eps) / sa[t]; t > 0: x_prev = mean + sigma z with
 * sigma = sqrt(acp[t-1] (1-acp[t]) / (1-acp[t-1])); t == 0: x_prev = mean.
 * Second output is `mean` (the reference returns (sampled, mean)). */
int vd_p_sample_cosine(const void* xt, const void* eps, const void* z,
                       void* x_prev, void* mean_out, const int64_t* t,
                       const float* acp, const float* sqrt_acp,
                       const float* sqrt_1m_acp, int64_t B, int64_t per_sample,
                       int dtype, void* stream);

/* DDIM step (build extension, no reference oracle beyond the acp tables):
 * x0 = (xt - sqrt(1-a_t) eps)/sqrt(a_t) [clamped to [-1,1] if clip];
 * sigma = eta sqrt((1-a_p)/(1-a_t) (1 - a_t/a_p));
 * x_prev = sqrt(a_p) x0 + sqrt(1-a_p-sigma^2) eps + sigma z, a_p = acp[t_prev]
 * or 1 when t_prev < 0.  t, t_prev: int64[B].  x0 (the second output) may be NULL, here and
 * in vd_ddim_step_pred: it is then not written.  z may be NULL when eta == 0. */
int vd_ddim_step(const void* xt, const void* eps, const void* z, void* x_prev,
                 void* x0, const int64_t* t, const int64_t* t_prev,
                 const float* acp, float eta, int clip, int64_t B,
                 int64_t per_sample, int dtype, void* stream);
/* The same step for a model output of either parameterisation (enum vd_prediction, above).
 * VD_PRED_EPS: vd_ddim_step (which is this call).  VD_PRED_V: `eps` holds the model's v and,
 * with sa = sqrt(a_t), s1m = sqrt(1 - a_t),
 *   x0 = sa xt - s1m v,  eps = s1m xt + sa v;
 * the clamp, the direction and the noise terms are as above. */
int vd_ddim_step_pred(const void* xt, const void* eps, const void* z, void* x_prev,
                      void* x0, const int64_t* t, const int64_t* t_prev,
                      const float* acp, float eta, int clip, int prediction, int64_t B,
                      int64_t per_sample, int dtype, void* stream);

/* ---- classifier-free audio guidance (build extension; no reference counterpart: the
 * reference samples with one conditional forward per step, test.py:51-83) ----
 * eps_c / eps_u: the denoiser's noise with the audio and with the null audio, [B][per_sample]
 * in `dtype`.  g = eps_u + w (eps_c - eps_u) in fp32; with rescale = phi in (0, 1] the guided
 * noise is f_b g, f_b = phi sqrt(SS(eps_c[b]) / SS(g[b])) + (1 - phi), SS(x) = sum (x_i -
 * mean(x))^2 over the sample (the std-rescale of Lin et al. 2023, diffusers'
 * rescale_noise_cfg; the n - 1 of the unbiased std cancels in the ratio); phi = 0: g itself.
 * vd_cfg_stats: the per-sample statistics in a FIXED order into the caller's workspace
 * (vd_cfg_workspace_size bytes, [B][partials][4] fp32): per-block sums of fixed ranges, then
 * per-block CENTRED sums of squares about the mean of the sums added in a fixed order.  Two
 * launches, no atomics, no semaphore, no memset and no cross-block communication inside a
 * launch, so the bits are identical eager and replayed from a HIP graph (DESIGN section 9.3,
 * as vd_mse_loss; torch.std is the one-launch multi-block reduction that went stale there).
 * vd_ddim_step_cfg: guide, rescale and the vd_ddim_step update in one pass: reads xt, eps_c,
 * eps_u (and z), writes x_prev and x0 (x0 may be NULL) and, when x_prev_dup is non-NULL, the
 * same x_prev values there too (the second half of a doubled-batch denoiser input).  x_prev
 * may alias xt.  rescale > 0 reads the workspace vd_cfg_stats filled for the same eps_c, eps_u
 * and w; every block adds its sample's partials in the same fixed order.  rescale == 0: workspace
 * may be NULL and vd_cfg_stats need not run.
 * vd_cfg_combine: the same guided noise written to eps_out (the eps of vd_p_sample_*). */
size_t vd_cfg_workspace_size(int64_t B, int64_t per_sample);
int vd_cfg_stats(const void* eps_c, const void* eps_u, float w, int64_t B, int64_t per_sample,
                 int dtype, void* workspace, size_t workspace_bytes, void* stream);
int vd_ddim_step_cfg(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                     void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                     const int64_t* t_prev, const float* acp, float w, float rescale,
                     const void* workspace, float eta, int clip, int64_t B, int64_t per_sample,
                     int dtype, void* stream);
int vd_cfg_combine(const void* eps_c, const void* eps_u, void* eps_out, float w, float rescale,
                   const void* workspace, int64_t B, int64_t per_sample, int dtype,
                   void* stream);
/* vd_ddim_step_cfg for either parameterisation: the guide and the std-rescale act on the model
 * output -- with VD_PRED_V on the two v outputs, as Lin et al. define the rescale -- and the
 * guided output enters the step as in vd_ddim_step_pred.  VD_PRED_EPS: vd_ddim_step_cfg (which
 * is this call).
 * Every DDIM and DPM-Solver++ step entry point, plain, guided or thresholded, launches one
 * instantiation of the same step kernel (csrc/elementwise.hip, step_kernel): one block column
 * per sample, the sample's schedule scalars, f_b and threshold taken once per block. */
int vd_ddim_step_cfg_pred(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                          void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                          const int64_t* t_prev, const float* acp, float w, float rescale,
                          const void* workspace, float eta, int clip, int prediction,
                          int64_t B, int64_t per_sample, int dtype, void* stream);

/* DPM-Solver++(2M) step (Lu et al. 2022; build extension, no reference counterpart): a
 * second-order multistep update that reuses the previous step's x0 instead of a second forward.
 * coef: fp32 [n_steps][8], row i = [alpha_t, sigma_t, A, B, C, 0, 0, 0], computed in fp64 on
 * the host (vdiff.schedulers.DPMSolverSampler) and rounded once.
 *   x0 = (xt - sigma_t eps) / alpha_t [clamped to [-1,1] if clip];
 *   x_prev = A xt + B x0 + C x0_last, from the fp32 x0.
 * step: a DEVICE int64 scalar, the row index, clamped into [0, n_steps - 1] by the kernel: the
 * launch arguments are the same at every step, so one captured graph replays for all of them.
 * x0_hist holds x0_last on entry and x0 on return (in place; never NULL).  A row whose C is
 * exactly 0 (the first-order rows and the last one) does NOT read x0_hist, which may then be
 * uninitialised.  x_prev may alias xt.
 * vd_dpm_step_cfg: guide, rescale and the same update in one pass, as vd_ddim_step_cfg: eps =
 * f_b (eps_u + w (eps_c - eps_u)); x_prev_dup (may be NULL) receives x_prev's values too;
 * rescale > 0 reads the vd_cfg_stats workspace, rescale == 0 accepts a NULL one.
 * Plain vector loads and stores: no atomics, no memset, no LDS beyond the f_b sum.
 * v-prediction needs no other kernel: x0 = alpha xt - sigma v = (xt - (sigma / alpha) v) / (1 /
 * alpha), so a table whose columns 0 and 1 hold 1 / alpha_t and sigma_t / alpha_t
 * (DPMSolverSampler(prediction="v")) makes `eps` the model's v, guided or not. */
int vd_dpm_step(const void* xt, const void* eps, void* x_prev, void* x0_hist,
                const float* coef, int64_t n_steps, const int64_t* step, int clip,
                int64_t B, int64_t per_sample, int dtype, void* stream);
int vd_dpm_step_cfg(const void* xt, const void* eps_c, const void* eps_u, void* x_prev,
                    void* x_prev_dup, void* x0_hist, const float* coef, int64_t n_steps,
                    const int64_t* step, float w, float rescale, const void* workspace,
                    int clip, int64_t B, int64_t per_sample, int dtype, void* stream);

/* ---- dynamic thresholding (Saharia et al. 2022, section 2.3; build extension, no reference
 * counterpart: the reference's samplers clamp x0 to [-1, 1]) ----
 * Per sample b over its P = per_sample elements, with x0 in fp32 as the step kernel forms it:
 *   q_b  = the rank-th smallest |x0_i| (0-based; an element of the data, never interpolated:
 *          torch.quantile(..., interpolation="higher") with rank = ceil(p (P - 1)));
 *   s_b  = min(max(q_b, floor), cap)               (sampling: floor = 1, cap = threshold_max);
 *   x0_i = clamp(x0_i, -s_b, s_b) / s_b            (vd_ddim_step_thr / vd_dpm_step_thr).
 * The order is that of the unsigned bit patterns of |x0|: a NaN sorts above +inf, and a NaN q_b
 * becomes the floor (fmaxf).  The rank is the host's: the library never sees p.
 *
 * vd_x0_source says where x0 comes from; it is formed again in every pass and never written:
 *   VD_X0_IDENTITY  x0 = x (eps, eps_u NULL);
 *   VD_X0_DDIM      vd_ddim_step_pred's x0 from x = xt, eps (the model's eps or v, `prediction`),
 *                   t int64[B] and acp;
 *   VD_X0_DPM       vd_dpm_step's x0 from x = xt, eps, coef [n_steps][8] and the device scalar
 *                   `step`, clamped into [0, n_steps - 1] as the step kernel clamps it.
 * eps_u != NULL (the two step rules): eps is eps_c and the model output is guided first, f_b
 * (eps_u + w (eps_c - eps_u)), with rescale > 0 from the vd_cfg_stats workspace `cfg_workspace`
 * (NULL allowed when rescale == 0), exactly as vd_ddim_step_cfg_pred / vd_dpm_step_cfg guide it.
 * Fields a rule does not read are ignored.
 *
 * vd_x0_abs_quantile writes s fp32 [B] (every entry).  Method: a most-significant-digit radix
 * select on the bit pattern of |x0|, four 8-bit digits, EIGHT launches: per digit one histogram
 * launch (block k of sample b counts its fixed range into LDS with integer atomics and stores
 * its row to the workspace with plain stores) and one scan launch (one block per sample adds the
 * rows, finds the bin that holds the rank, hands prefix and remaining rank to the next digit;
 * the last one writes s).  All histogram launches are one kernel, so every pass sees the same
 * bits of x0.  No global atomics, no float atomics, no memset, no cross-block communication
 * inside a launch, and every workspace word read was written earlier in the same call: the
 * workspace (vd_x0_quantile_workspace_size bytes, 4-byte aligned) may be uninitialised, and the
 * bits are the same eager and replayed from a HIP graph.  B <= 65535, per_sample < 2^32, 0 <=
 * rank < per_sample, cap >= floor.  Tensors follow the alignment rule above (x, eps, eps_u).
 *
 * vd_ddim_step_thr: vd_ddim_step_cfg_pred with x0 = clamp(x0, -s_b, s_b) / s_b, s_b = thresh[b]
 * (device fp32 [B], >= 1) in place of the static clamp; x_prev, x_prev_dup and x0 are formed
 * from the thresholded x0, the direction term keeps the model's own (guided) eps.  eps_u == NULL:
 * the unguided step on eps_c (w, rescale and workspace are then not read).  Overwrites x_prev,
 * x_prev_dup and x0 (each of the last two may be NULL); x_prev may alias xt; z may be NULL when
 * eta == 0.
 * vd_dpm_step_thr: vd_dpm_step_cfg the same way: x_prev, x_prev_dup (may be NULL) and the
 * history x0_hist (in place, never NULL) get the thresholded x0; eps_u == NULL is vd_dpm_step's
 * unguided update. */
enum vd_x0_rule { VD_X0_IDENTITY = 0, VD_X0_DDIM = 1, VD_X0_DPM = 2 };
typedef struct {            /* 88 bytes */
  const void* x;            /* the data (identity) or xt */
  const void* eps;          /* the model's output; eps_c when eps_u is given */
  const void* eps_u;        /* NULL: unguided */
  const int64_t* t;         /* DDIM */
  const float* acp;         /* DDIM */
  const float* coef;        /* DPM */
  const int64_t* step;      /* DPM */
  const void* cfg_workspace;
  int64_t n_steps;          /* DPM */
  int32_t rule;             /* enum vd_x0_rule */
  int32_t prediction;       /* DDIM: enum vd_prediction */
  float w;
  float rescale;
} vd_x0_source;
size_t vd_x0_quantile_workspace_size(int64_t B, int64_t per_sample);
int vd_x0_abs_quantile(const vd_x0_source* src, int64_t rank, float floor, float cap, int64_t B,
                       int64_t per_sample, int dtype, float* s, void* workspace,
                       size_t workspace_bytes, void* stream);
int vd_ddim_step_thr(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                     void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                     const int64_t* t_prev, const float* acp, float w, float rescale,
                     const void* workspace, float eta, int prediction, const float* thresh,
                     int64_t B, int64_t per_sample, int dtype, void* stream);
int vd_dpm_step_thr(const void* xt, const void* eps_c, const void* eps_u, void* x_prev,
                    void* x_prev_dup, void* x0_hist, const float* coef, int64_t n_steps,
                    const int64_t* step, float w, float rescale, const void* workspace,
                    const float* thresh, int64_t B, int64_t per_sample, int dtype, void* stream);

/* ---- masked sampling: known pixels and frames kept inside the step (inpainting, clip
 * continuation; build extension, no reference counterpart) ----
 * known: the clip to keep, [B][per_sample] in `dtype` like xt.  keep: fp32 [Bk][S], Bk in {1, B},
 * S > 0 a divisor of per_sample (the product of the spatial dimensions): element i of sample b
 * reads k = keep[Bk == 1 ? 0 : b][i % S], so a row is broadcast over the channels and, Bk == 1,
 * over the batch; k <= 0 is read as 0 and k >= 1 as 1.  Per element, in fp32, with y the x0 the
 * step forms today (rule -> static clamp or dynamic threshold) and e the model's direction term:
 *   k == 0:  x0' = y,                     e' = e         (today's expressions and bits)
 *   k == 1:  x0' = x_k,                   e' = e_k       (selects: a non-finite model output
 *                                                         there reaches no output)
 *   else:    x0' = (1 - k) y + k x_k,     e' = (1 - k) e + k e_k
 *   e_k = (xt - sqrt(a_t) x_k) / sqrt(1 - a_t)           (DDIM; 2M has no direction term)
 *   x_prev = the rule's x_prev on (xt, x0', e', z | x0_last), unchanged.
 * x0' goes to x_prev, x_prev_dup, x0 and the 2M history; x_k is never clamped or divided by the
 * threshold.  With eta = 0 an element with k == 1 therefore stays on the line x_k and xt span,
 * whatever the model says: DDIM x_prev = sqrt(a_p) x_k + dir e_k; 2M x_prev = A xt + (B + C) x_k
 * once the history holds x_k; the last step returns x_k itself.
 * vd_ddim_step_known: vd_ddim_step_pred, _cfg_pred and _thr in one: eps_u == NULL is the
 * unguided step on eps_c (w, rescale, workspace not read; any B), otherwise B <= 65535; thresh
 * != NULL is the thresholded step (clip must be 0).  vd_dpm_step_known: vd_dpm_step, _cfg and
 * _thr the same way.  known == keep == NULL: the unmasked step; one of them alone is refused.
 * Alignment: the rule above over known and keep too, so that a masked step runs 8-wide exactly
 * where the unmasked step on the same tensors does (the k == 0 bits are the unmasked step's at
 * the same width).  The mask index is computed once per vector; with S % 8 == 0 a vector lies
 * inside one channel of the mask and its mask values are one vector load, otherwise they are
 * read one element at a time, so no access straddles the end of a mask row.
 * known and keep are read only and may alias no output; x_prev may alias xt and the
 * history is in place, as in the unmasked steps.  Plain vector loads and stores: no atomics, no
 * workspace, no memset. */
int vd_ddim_step_known(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                       void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                       const int64_t* t_prev, const float* acp, float w, float rescale,
                       const void* workspace, float eta, int clip, int prediction,
                       const float* thresh, const void* known, const float* keep, int64_t Bk,
                       int64_t S, int64_t B, int64_t per_sample, int dtype, void* stream);
int vd_dpm_step_known(const void* xt, const void* eps_c, const void* eps_u, void* x_prev,
                      void* x_prev_dup, void* x0_hist, const float* coef, int64_t n_steps,
                      const int64_t* step, float w, float rescale, const void* workspace,
                      int clip, const float* thresh, const void* known, const float* keep,
                      int64_t Bk, int64_t S, int64_t B, int64_t per_sample, int dtype,
                      void* stream);

/* Long-clip sampling (build extension, no reference counterpart): a latent of L frames is
 * denoised as W overlapping windows of T frames, one batched forward per step, and the windows'
 * predictions are blended back where they overlap (vdiff.engine.sample_long; the tables come
 * from vdiff.schedulers.WindowPlan).  Contiguous NCTHW, fp32 or bf16 (dtype); HW = H * W.
 * vd_window_gather: for x [B][C][L][HW],
 *   win[b * W + w][c][f][hw] = x[b][c][starts[w] + f][hw];
 * win_dup (may be NULL) receives the same values: the null-audio half of a guided forward, as
 * x_prev_dup elsewhere.  starts: DEVICE int32 [W]; an entry is clamped into [0, L - T].
 * vd_window_blend: for win [B * W][C][T][HW],
 *   out[b][c][l][hw] = sum_k cover_wgt[l][k] * win[b * W + w_k][c][l - starts[w_k]][hw],
 *   w_k = cover_win[l][k].
 * cover_win: DEVICE int32 [L][kmax], the windows that cover frame l in ascending order, -1 in
 * the unused slots; cover_wgt: DEVICE fp32 [L][kmax]; kmax <= VD_WINDOW_KMAX.  The first
 * product initialises the accumulator, the rest are one fp32 fma each in ascending k, and the
 * sum is rounded once to dtype.  An entry whose window is outside [0, W) or whose local frame
 * is outside [0, T) is skipped, so no table content reads out of bounds; a frame without a
 * valid entry is written as 0.
 * Both are gathers over output elements -- one element, or one 16-byte vector when HW *
 * sizeof(element) and every pointer are multiples of 16, per thread over a flat grid: no
 * atomics, no memset, no workspace, no cross-block communication, so eager and replayed runs
 * give the same bits.  Null pointers (win_dup excepted), non-positive sizes, T > L, a kmax
 * outside [1, VD_WINDOW_KMAX] and B * W * C or L * HW of 2^31 or more fail with VD_EINVAL
 * before any launch. */
#define VD_WINDOW_KMAX 8
int vd_window_gather(const void* x, void* win, void* win_dup, const int32_t* starts,
                     int64_t B, int64_t C, int64_t L, int64_t T, int64_t W, int64_t HW,
                     int dtype, void* stream);
int vd_window_blend(const void* win, void* out, const int32_t* starts,
                    const int32_t* cover_win, const float* cover_wgt, int kmax, int64_t B,
                    int64_t C, int64_t L, int64_t T, int64_t W, int64_t HW, int dtype,
                    void* stream);

/* ---- GroupNorm (+SiLU) -------------------------------------------------
 * replaces GroupNorm32 (utils.py:54-56, fp32 statistics) followed by nn.SiLU
 * (unet.py:194-198, 218-225, 297, 624-628).  x, y: [B][S][C] channels-last,
 * S = T*H*W; gamma/beta fp32[C]; mean/rstd fp32[B*G] (saved for backward).
 * (The ResBlock emb-add that precedes out_layers' GN is fused into the
 * producing conv's epilogue via vd_conv3d_fwd's chan_add.) */
/* drop_p > 0 also fuses the train-mode nn.Dropout that follows the SiLU in
 * ResBlock.out_layers (unet.py:218-225): element i is kept with probability
 * 1 - drop_p (scaled by 1/(1-drop_p)) by a counter-based hash of (seed, i);
 * the backward regenerates the same mask from the same seed. */
/* counter (device memory, or NULL = off): while set, every GroupNorm launch
 * with drop_p > 0 also takes this pointer and mixes the uint64 it reads at run
 * time into its seed.  A train step captured as a HIP graph (vdiff.engine.
 * Trainer(graph=True)) freezes the host seed in the launch arguments; bumping
 * the counter before each replay gives every step a fresh mask, the forward
 * and backward of one step the same one.  Host-side setting; no GPU call. */
void vd_set_dropout_counter(const uint64_t* counter);
/* Pixel rows whose loads each GroupNorm thread keeps in flight (1, 2 default, 4); the sums are
 * added in the same order for every value (bit-identical).  Process-wide A/B hook; returns the
 * previous value or -2.  No reference counterpart. */
int vd_groupnorm_set_unroll(int u);
size_t vd_groupnorm_workspace_size(int B, int64_t S, int C, int G);
int vd_groupnorm_silu_fwd(const void* x, const float* gamma, const float* beta,
                          void* y, float* mean, float* rstd, int B, int64_t S,
                          int C, int G, float eps, int silu, float drop_p,
                          uint64_t seed, int dtype, void* workspace,
                          void* stream);
/* dx = d/dx of dropout(silu(GN(x))); dgamma/dbeta are fp32[C], OVERWRITTEN. */
int vd_groupnorm_silu_bwd(const void* x, const void* dy, const float* gamma,
                          const float* beta, const float* mean,
                          const float* rstd, void* dx, float* dgamma,
                          float* dbeta, int B, int64_t S, int C, int G,
                          int silu, float drop_p, uint64_t seed, int dtype,
                          void* workspace, void* stream);
/* The same with dx += dadd (dadd in x's layout and dtype, or NULL): x's gradient from its
 * other consumer -- the residual branch of ResBlock (unet.py:268, skip_connection(x) + h) and
 * AttentionBlock (unet.py:317, x + h) -- added in fp32 before dx is rounded, instead of the
 * separate elementwise add autograd would run to accumulate the two gradients. */
int vd_groupnorm_silu_bwd_add(const void* x, const void* dy, const void* dadd,
                              const float* gamma, const float* beta, const float* mean,
                              const float* rstd, void* dx, float* dgamma, float* dbeta,
                              int B, int64_t S, int C, int G, int silu, float drop_p,
                              uint64_t seed, int dtype, void* workspace, void* stream);
/* FiLM-conditioned GroupNorm (reference ResBlock, use_scale_shift_norm):
 *   y = dropout(silu(GN(x) * (1 + scale[b, c]) + shift[b, c]))
 * film is fp32 [B][2C], the scale in [:, :C] and the shift in [:, C:] (the layout of
 * th.chunk(emb_out, 2, dim=1)).  The modulation folds into the per-(sample, channel) affine,
 * so the launches, chunk plan, workspace and activation traffic are those of
 * vd_groupnorm_silu_fwd / _bwd_add; film = 0 returns their bits.  The backward also writes
 * dfilm (fp32 [B][2C], film's layout, every element OVERWRITTEN) in the finalize pass; all sums
 * run in a fixed order (no atomics, no zero fill). */
int vd_groupnorm_film_silu_fwd(const void* x, const float* gamma, const float* beta,
                               const float* film, void* y, float* mean, float* rstd, int B,
                               int64_t S, int C, int G, float eps, int silu, float drop_p,
                               uint64_t seed, int dtype, void* workspace, void* stream);
int vd_groupnorm_film_silu_bwd_add(const void* x, const void* dy, const void* dadd,
                                   const float* gamma, const float* beta, const float* film,
                                   const float* mean, const float* rstd, void* dx,
                                   float* dgamma, float* dbeta, float* dfilm, int B, int64_t S,
                                   int C, int G, int silu, float drop_p, uint64_t seed,
                                   int dtype, void* workspace, void* stream);

/* ---- SiLU on flat tensors (time-embedding MLP, ResBlock.emb_layers:
 * unet.py:483-487, 211-217).  bwd: dx = dy * silu'(x). */
int vd_silu(const void* x, void* y, int64_t n, int dtype, void* stream);
int vd_silu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype,
                void* stream);

/* ---- UNetAudio conditioning concat (unet_audio.py:52-61) -------------
 * out[b][t][y][x][:] = [ image[b][t][y][x][0:Cx] | imc[b][ys][xs][0:Ci] |
 *                        audio[b][t][0:Ca] | zeros up to out_cstride ]
 * with (ys, xs) the torch "nearest" source of (y, x) for an (h, w) -> (H, W)
 * resize (the 1x1 cond conv commutes with it and runs at (h, w)).  imc is
 * broadcast over T (one reference image per clip) and audio over (H, W).
 * bwd: d_imc[b][h][w][Ci] and d_audio[b][T][Ca] (fp32) are OVERWRITTEN, with fixed-order
 * sums (bit-reproducible; d_audio through a caller workspace of
 * vd_cond_concat_bwd_workspace_size bytes). */
int vd_cond_concat(const void* image, const void* imc, const void* audio,
                   void* out, int B, int T, int H, int W, int Cx, int h, int w,
                   int Ci, int Ca, int out_cstride, int dtype, void* stream);
size_t vd_cond_concat_bwd_workspace_size(int B, int T, int H, int W, int Ca);
int vd_cond_concat_bwd(const void* dout, float* d_imc, float* d_audio, int B,
                       int T, int H, int W, int Cx, int h, int w, int Ci,
                       int Ca, int out_cstride, int dtype, void* workspace,
                       void* stream);

/* ---- Upsample (nearest, x2 on H and W) --------------------------------
 * replaces unet.py:112-122 F.interpolate(..., mode="nearest") with the
 * dims=3 size (T, 2H, 2W) (and dims=2 scale_factor=2 with T=1).
 * x: [B][T][H][W][C] -> y: [B][T][2H][2W][C]; bwd sums the 4 children. */
int vd_upsample_nearest_hw(const void* x, void* y, int B, int T, int H, int W,
                           int C, int dtype, void* stream);
int vd_upsample_nearest_hw_bwd(const void* dy, void* dx, int B, int T, int H,
                               int W, int C, int dtype, void* stream);

/* ---- Convolution (implicit GEMM on MFMA) ------------------------------
 * replaces conv_nd (utils.py:59-69) at unet.py:110,143-145,197,223,231,234,
 * 494,627 and the 1x1 Conv1d of AttentionBlock (unet.py:298,306).
 * Weight layouts (packed by the caller from the torch [Co][Ci][kt][kh][kw]):
 *   fwd      : w_fwd [Co][taps][Ci]      (K = taps*Ci contiguous per Co)
 *   bwd_data : w_bwd [Ci][taps][Co]
 *   bwd_wgt  : dw    [Co][taps][Ci] fp32, ACCUMULATED into (zero it first)
 * Epilogue of fwd: y = conv + bias[co] + chan_add[b][co] + residual.
 * Any of bias / chan_add / residual may be NULL.  bias/chan_add are fp32;
 * residual has the activation dtype, y's shape and y's pixel stride (y_cstride).
 * Ci must be a multiple of 8 in both dtypes (the kernels read 16-byte bf16 chunks and the
 * fp32 path keeps the same rule); pad channels otherwise.  x_cstride must be a multiple of 8;
 * y_cstride may be any value >= Co for the forward and must be a multiple of 8, like Co, for
 * bwd_data and bwd_weight, which read dy in 16-byte chunks. */
typedef struct vd_conv_desc {
  int B;
  int Ti, Hi, Wi, Ci;  /* input  */
  int To, Ho, Wo, Co;  /* output */
  int kt, kh, kw;      /* kernel taps */
  int st, sh, sw;      /* stride */
  int pt, ph, pw;      /* zero padding */
  int x_cstride;       /* elements between input pixels (>= Ci), 0 = Ci */
  int y_cstride;       /* elements between output pixels (>= Co), 0 = Co */
  int dtype;
} vd_conv_desc;

int vd_conv3d_fwd(const vd_conv_desc* d, const void* x, const void* w_fwd,
                  const float* bias, const float* chan_add,
                  const void* residual, void* y, void* stream);
/* dx[B][Ti][Hi][Wi][Ci] = conv^T(dy); overwrites dx. */
int vd_conv3d_bwd_data(const vd_conv_desc* d, const void* dy,
                       const void* w_bwd, void* dx, void* stream);
/* dw[Co][taps][Ci] += sum over output pixels of dy (x) x  (fp32) */
int vd_conv3d_bwd_weight(const vd_conv_desc* d, const void* x, const void* dy,
                         float* dw, void* stream);
/* Deterministic weight gradient (the default of the Python ops since round 4): every pixel
 * split writes its fp32 partial dW into its own slice of `workspace`
 * (vd_conv3d_bwd_weight_workspace_size bytes), then one pass adds the slices in a fixed
 * order and WRITES dw in the torch layout [Co_out][Ci_out][taps] (Co_out <= d->Co and
 * Ci_out <= d->Ci drop the channel padding).  Bit-reproducible run to run; no zero fill
 * and no layout permute are needed.  Replaces the weight half of conv_nd's autograd
 * (utils.py:59-69) as vd_conv3d_bwd_weight does. */
size_t vd_conv3d_bwd_weight_workspace_size(const vd_conv_desc* d);
int vd_conv3d_bwd_weight_det(const vd_conv_desc* d, const void* x, const void* dy, float* dw,
                             int Co_out, int Ci_out, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Which 3x3x3 stride-1 bf16 convs (fwd / bwd-data) take the halo-tile kernel: 0 none (the
 * gathered tiles), 1 and 2 (default) every eligible shape (W % 16 == 0, pad 1) on 4-wave
 * 2x4x16 tiles, 3 on 8-wave 2x8x16 tiles, 4 the 4-wave tiles with the compiler's fragment-read
 * placement, 5 the forward without early next-step halo pieces.  Modes 1-5 are bit-identical;
 * 0 agrees up to fp32 summation order.
 * Process-wide; returns the previous mode, or -2 for an invalid one.  Initial value from env
 * VDIFF_CONV_HALO.  No reference counterpart: an A/B and test hook. */
/* Which kernel computes the kw-strip (3x3x3 / 3x3 stride-1 bf16) and 1x1 weight gradients:
 * 1 (default) the round-6 kernel with the ring stages unrolled and early fragment reads, 2 the
 * same with the compiler's read placement, 0 the round-5 kernel; same tiles and summation
 * order (bit-identical results).  Returns the previous mode, or -2 (A/B, tests). */
int vd_conv_set_wgrad(int mode);
int vd_conv_set_halo(int mode);

/* ---- Conv glue ---------------------------------------------------------
 * vd_channel_sums: out[b][c] = sum over the S pixels of x[b][s][c] (fp32; x channels-last
 * with pixel stride cstride, 0 = C; C % 8 == 0; deterministic two-stage reduction through
 * a caller workspace of vd_channel_sums_workspace_size bytes).  One pass gives both the conv bias
 * gradient (sum over b) and the chan_add gradient of the ResBlock emb-add -- the autograd
 * of conv_nd's bias (utils.py:59-69) and of `h = h + emb_out` (unet.py:255-258).
 * vd_conv_pack_weight: torch fp32 weight [Co][Ci][taps] -> the w_fwd [Co][taps][Cip]
 * (transpose 0) or w_bwd [Cip][taps][Cop] (transpose 1) operand above, zero-padded. */
size_t vd_channel_sums_workspace_size(int B, int C);
int vd_channel_sums(const void* x, int B, int64_t S, int C, int cstride, int dtype,
                    float* out, void* workspace, void* stream);
int vd_conv_pack_weight(const float* w, int Co, int Ci, int taps, int Cip, int Cop,
                        int transpose, int dtype, void* out, void* stream);
/* vd_conv_pack_weights: n vd_conv_pack_weight jobs in ONE launch (a training step's conv
 * operands, re-packed once per optimizer step -- the weights that train.py:128-134's
 * optimizer.step() just updated).  `descs` is a DEVICE array of n descriptors with
 * start = the job's first element in the concatenation of all outputs (ascending, start[0]
 * = 0) and `total` the concatenation's length; every output is in `dtype`.  n <= 1024. */
typedef struct {
  const float* w;
  void* out;
  int Co, Ci, taps, Cip, Cop, transpose;
  int64_t start;
} vd_pack_desc;
int vd_conv_pack_weights(const vd_pack_desc* descs, int n, int64_t total, int dtype,
                         void* stream);

/* ---- weight EMA (utils.py:92-102 update_ema, for every tensor and rate in ONE launch) ----
 * For each descriptor, each element i < n and each rate j < k:
 *   dst[j][i] <- dst[j][i] + (1 - d_j) * (src[i] - dst[j][i])          (fp32, src read once)
 * d_j = rates[j], or with `warmup` min(rates[j], (float)(1 + c) / (float)(10 + c)) where
 * c = *num_updates, the updates done before this one (read, never written: the caller
 * increments it).  If skip_if_nonneg is given and *skip_if_nonneg >= 0 nothing is written
 * (Trainer's first-bad-step record).  Both words are read on the device when the kernel runs,
 * so a captured launch replays with their current values.
 * `descs` is a DEVICE array of n_desc descriptors, one per range of a tensor; the caller cuts
 * large tensors into ranges of a fixed size, any number of them (blocks walk the table
 * grid-stride).  A range whose src and k dst pointers are all 16-B aligned moves 8 elements
 * per lane, any other one element at a time.  dst[j] for j >= k is not read.  One kernel, no
 * atomics, no memset, no workspace; the result does not depend on the grid.
 * rates: HOST array of k values in [0, 1). */
typedef struct {            /* 48 bytes */
  const float* src;         /* fp32 parameter range                      */
  float* dst[4];            /* its EMA range per rate; unused slots NULL */
  int64_t n;                /* elements in the range                     */
} vd_ema_desc;
int vd_ema_update(const vd_ema_desc* descs, int n_desc, int k, const float* rates, int warmup,
                  const int64_t* num_updates, const int64_t* skip_if_nonneg, void* stream);

/* ---- gradient clipping by global norm (torch.nn.utils.clip_grad_norm_; no reference
 * counterpart: train.py:102-134 bounds no update) ----
 * `descs` is a DEVICE array of n_desc descriptors, one per range of an fp32 gradient tensor,
 * cut by the caller as for vd_ema_update (any number of ranges; blocks walk the table
 * grid-stride).  A range whose pointer is 16-B aligned moves 8 elements per lane, any other one
 * element at a time.
 * vd_grad_sumsq: workspace[i] (fp32, vd_grad_clip_workspace_size(n_desc) bytes) = the sum of
 * squares of range i in a FIXED order (a lane's fused multiply-add chain, then an LDS tree;
 * csrc/gradclip.hip states the layout), independent of the grid.
 * vd_grad_clip: two launches on the same workspace.  One block adds the n_desc partials in one
 * fixed order (in fp64) and writes
 *   record[0] = norm = sqrt(total),  record[1] = coef = min(1, max_norm / (norm + 1e-6))
 * (torch's formula; fp32).  Then every element becomes g * coef (one fp32 multiply) if
 * coef < 1; with coef == 1 nothing is written.  A non-finite norm records coef = 1 and leaves
 * every gradient as it is.  max_norm > 0; +inf is legal and means "measure only".
 * Overflow is NOT scaled away: gradients whose squares overflow fp32 give a non-finite norm,
 * as torch's do.  No atomics, no memset, no semaphore, no cross-block communication inside a
 * launch, nothing read on the host: the same bits eager and replayed from a HIP graph.
 * record: DEVICE fp32[2].  Null pointers, n_desc <= 0, a max_norm that is not > 0 (NaN
 * included) and a short workspace fail with VD_EINVAL before any launch. */
typedef struct {            /* 16 bytes */
  float* g;                 /* fp32 gradient range  */
  int64_t n;                /* elements in the range */
} vd_grad_desc;
size_t vd_grad_clip_workspace_size(int n_desc);
int vd_grad_sumsq(const vd_grad_desc* descs, int n_desc, void* workspace, size_t workspace_bytes,
                  void* stream);
int vd_grad_clip(const vd_grad_desc* descs, int n_desc, const void* workspace, float max_norm,
                 float* record /* [2]: norm, coef */, void* stream);

/* ---- Adam / AdamW step (torch.optim.Adam / AdamW's update; train.py:102 is Adam at a constant
 * rate) with the learning-rate schedule and the bad-step decision taken ON THE DEVICE ----
 * `descs` is a DEVICE array of n_desc descriptors, one per range of one parameter tensor (cut by
 * the caller as for vd_ema_update; the ranges of one tensor are consecutive rows).  Two launches
 * whatever the number of tensors; no atomics, no memset, no semaphore, nothing read on the host:
 * the same bits eager and replayed from a HIP graph.
 * Launch 1 (grid-stride over the table) updates p, m, v of every range from g.  A range whose
 * four pointers are 16-B aligned moves 8 elements per lane, any other one element at a time.
 * Every block reads the same device words, none of which launch 1 writes:
 *   steps[tensor]             the tensor's own count of applied updates (t = count + 1)
 *   state[0..3]               applied, skipped, run (consecutive skipped), tripped_at (-1: not)
 *   loss, grad_norm           fp32 scalars, either may be NULL
 * The step is SKIPPED -- launch 1 writes nothing -- if max_bad_run > 0 and (loss is non-finite
 * or grad_norm is non-finite or tripped_at >= 0).  Otherwise, with s = applied:
 *   lr_s = lr * warm(s) * decay(s);  warm = min(1, (s + 1) / W) (W = 0: 1);
 *   q = clamp((s - W) / (T - W), 0, 1);  decay = 1 (VD_LR_CONSTANT)
 *     | r + (1 - r) (1 + cos(pi q)) / 2 (VD_LR_COSINE) | r + (1 - r) (1 - q) (VD_LR_LINEAR)
 *   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t          (lr_s, bc1, bc2 in fp64, rounded to fp32 once)
 *   g' = g + wd p (L2 mode);  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g' g';
 *   p *= 1 - lr_s wd (decoupled mode);  p -= (lr_s / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * (csrc/adam.hip states the exact fp32 operation order).
 * Launch 2 (one block) takes the same decision from the same words, then: applied step --
 * steps[tensor] += 1 for every tensor of the table, applied += 1, run = 0; skipped step --
 * skipped += 1, run += 1, and if run > max_bad_run and tripped_at < 0, tripped_at = the global
 * step index (applied + skipped before this step; sticky: every later step is skipped).  It
 * records lr_out[0] = lr_s of this step (at the unchanged s on a skipped step) and
 * skip_flag_out[0] = -1 (applied) or the global step index (skipped), the convention of
 * vd_ema_update's skip_if_nonneg.
 * The hyperparameters are HOST values passed per launch: a captured launch freezes them.
 * Null descs / h / steps / state / lr_out / skip_flag_out, n_desc <= 0, a beta outside [0, 1),
 * eps <= 0, a negative lr or weight_decay, total_steps <= warmup_steps with a non-constant
 * schedule, min_ratio outside [0, 1], an unknown schedule and negative warmup_steps or
 * max_bad_run fail with VD_EINVAL before any launch. */
enum vd_lr_schedule { VD_LR_CONSTANT = 0, VD_LR_COSINE = 1, VD_LR_LINEAR = 2 };
typedef struct {            /* 48 bytes */
  float* p;                 /* fp32 parameter range                          */
  float* m;                 /* its first moment (exp_avg)                    */
  float* v;                 /* its second moment (exp_avg_sq)                */
  const float* g;           /* its gradient                                  */
  int64_t n;                /* elements in the range                         */
  int64_t tensor;           /* the tensor's index into the step-count array  */
} vd_adam_desc;
typedef struct {            /* 80 bytes */
  double lr, beta1, beta2, eps, weight_decay, min_ratio;
  int64_t warmup_steps;     /* W */
  int64_t total_steps;      /* T (ignored by VD_LR_CONSTANT) */
  int32_t schedule;         /* vd_lr_schedule */
  int32_t decoupled;        /* 1: AdamW's decay of p, 0: L2 (wd p added to g) */
  int32_t max_bad_run;      /* K; 0: never skip */
  int32_t reserved;
} vd_adam_hyper;
int vd_adam_step(const vd_adam_desc* descs, int n_desc, const vd_adam_hyper* h, int64_t* steps,
                 int64_t* state /* [4] */, const float* loss, const float* grad_norm,
                 float* lr_out, int64_t* skip_flag_out, void* stream);

/* ---- Flash attention --------------------------------------------------
 * replaces QKVAttentionLegacy.forward (unet.py:349-366) + the fp32 softmax
 * (unet.py:364) and, with heads split by strides, QKVAttention (unet.py:
 * 388-401).  One "sequence" = `seq_len` tokens of one head; sequence i
 * starts at element (i / groups) * batch_stride + (i % groups) * group_stride
 * of q/k/v (and of o with the o_* strides); consecutive tokens are
 * token_stride apart.  joint: groups 1; spatial (per frame): groups T;
 * temporal (per pixel): groups H*W, token_stride H*W*row.
 * softmax(scale * q k^T) v, fp32 softmax statistics; lse fp32[nseq][seq_len]
 * (natural log of the row sum of exp(scale*s)) is saved for backward. */
typedef struct vd_attn_desc {
  int nseq, seq_len, head_dim, groups;
  int64_t batch_stride, group_stride, token_stride;       /* q/k/v */
  int64_t o_batch_stride, o_group_stride, o_token_stride; /* o and dout */
  float scale;
  int dtype;
} vd_attn_desc;

int vd_attention_fwd(const vd_attn_desc* d, const void* q, const void* k,
                     const void* v, void* o, float* lse, void* stream);
/* Same, with a workspace: where the query grid would leave CUs idle (bf16, e.g. head_dim 256
 * at N = 16384) the keys are split over grid.z and the fp32 partials merged by a second
 * kernel (flash-decoding style).  workspace_bytes < vd_attention_fwd_workspace_size(d)
 * (which is 0 for shapes that do not split) falls back to vd_attention_fwd. */
size_t vd_attention_fwd_workspace_size(const vd_attn_desc* d);
int vd_attention_fwd_ws(const vd_attn_desc* d, const void* q, const void* k,
                        const void* v, void* o, float* lse, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Backward workspace: the row constants, plus the KV-split dQ partials for shapes that split. */
size_t vd_attention_bwd_workspace_size(const vd_attn_desc* d);
/* Kernel shape used for bf16 (no effect on results beyond fp32 summation order):
 * -1 per-kernel default, 0 base (4 waves x 32 rows), 1 two 32-row blocks per wave,
 * 2 eight waves, 3 / 4 software-pipelined with 8 / 4 waves, 5 / 6 the deferred-check
 * head_dim-64 forward with / without staggered wave halves, 7 the same with 4 waves and
 * two workgroups per CU, 8 the paired-wave head_dim-128 dK/dV, 9 the pipelined head_dim-64
 * backward with 4 waves x 2 blocks, 10 the role-split head_dim-256 dK/dV, 11 the
 * fragment-pipelined head_dim-64 backward, 12 the hand-scheduled head_dim-64 dQ (one wave
 * per SIMD, asm/gen_attn_asm.py) (shapes a kernel does not take keep their default).
 * Process-wide; returns the previous setting, or -2 for an invalid cfg (vd_last_error says
 * why).  Initial value from env VDIFF_ATTN_CFG
 * (base|nb2|w8|p8|p4|d8|d8n|d4|pair|p4n2|role|sp|asm).  No reference counterpart: an A/B
 * and test hook. */
int vd_attention_set_config(int cfg);
/* Short sequences (bf16, seq_len <= 32, head_dim 32/64/128/256, 16-B aligned rows: the
 * temporal attention of the spatial_temporal mode, T = 16 / 25 frames per pixel, and the
 * ViViT encoder's 9 tokens) run on dedicated kernels, one wave per sequence with 16x16 MFMA
 * tiles: vd_attention_fwd / _fwd_ws, and vd_attention_bwd as ONE fused dQ / dK / dV kernel
 * (no workspace used; it takes delta = rowsum(P dP) from the scores it holds, so its `o`
 * argument is not read there).  vd_attention_short_path(d) says whether d takes that path;
 * vd_attention_set_short(0) (or env VDIFF_ATTN_SHORT=0) routes such shapes to the flash
 * kernels instead (A/B and test hook; returns the previous setting).  No reference
 * counterpart: the reference materialises T x T scores (unet.py:361-365 per regrouped
 * sequence). */
int vd_attention_short_path(const vd_attn_desc* d);
/* The backward's decision on the real buffers: 1 when vd_attention_bwd will run the fused short
 * kernel for these pointers (every buffer 16-B aligned), 0 when it takes the flash dQ + dK/dV
 * kernels, which need the workspace of vd_attention_bwd_workspace_size. */
int vd_attention_bwd_short_path(const vd_attn_desc* d, const void* q, const void* k,
                                const void* v, const void* o, const void* dout, const void* dq,
                                const void* dk, const void* dv);
int vd_attention_set_short(int on);
/* dout uses the o_* strides; dq/dk/dv use the q/k/v strides (so they can be
 * written straight into a d(qkv) buffer) and are OVERWRITTEN. */
int vd_attention_bwd(const vd_attn_desc* d, const void* q, const void* k,
                     const void* v, const void* o, const void* dout,
                     const float* lse, void* dq, void* dk, void* dv,
                     void* workspace, void* stream);
/* The two halves of vd_attention_bwd (same arguments), for per-kernel timing:
 * _dq writes the per-row constants -rowsum(dO * O) and -lse*log2(e) into the
 * workspace and computes dq; _dkdv reads them and computes dk, dv.  Call _dq first. */
int vd_attention_bwd_dq(const vd_attn_desc* d, const void* q, const void* k,
                        const void* v, const void* o, const void* dout,
                        const float* lse, void* dq, void* workspace,
                        void* stream);
int vd_attention_bwd_dkdv(const vd_attn_desc* d, const void* q, const void* k,
                          const void* v, const void* dout, const float* lse,
                          void* dk, void* dv, void* workspace, void* stream);

/* ---- audio cross-attention (north_star build extension; no reference counterpart: the
 * reference conditions on audio by channel concatenation only, unet_audio.py:52-61).
 * Video tokens attend to audio tokens: softmax(scale * q k^T) v with q / o addressed by
 * `q` (as vd_attn_desc: nseq, seq_len = N_q, head_dim, groups, q and o strides, scale,
 * dtype) and k / v rows by the kv_* fields: sequence i's K/V rows start at
 * (i / q.groups) * kv_batch_stride + (i % q.groups) * kv_group_stride, kv_token_stride
 * apart, kv_len of them (N_kv may differ from N_q).  lse fp32 [nseq][N_q] as above.  The
 * backward has the self-attention contract (dq in the q strides, dk / dv in the kv
 * strides, overwritten); where the K/V grid leaves CUs idle (bf16, few audio tokens) the
 * queries are split and the fp32 dK / dV partials summed by a second kernel, inside the
 * workspace. */
typedef struct vd_xattn_desc {
  vd_attn_desc q;
  int kv_len;
  int64_t kv_batch_stride, kv_group_stride, kv_token_stride;
} vd_xattn_desc;

size_t vd_cross_attention_fwd_workspace_size(const vd_xattn_desc* x);
int vd_cross_attention_fwd(const vd_xattn_desc* x, const void* q, const void* k,
                           const void* v, void* o, float* lse, void* workspace,
                           size_t workspace_bytes, void* stream);
size_t vd_cross_attention_bwd_workspace_size(const vd_xattn_desc* x);
int vd_cross_attention_bwd_dq(const vd_xattn_desc* x, const void* q, const void* k,
                              const void* v, const void* o, const void* dout,
                              const float* lse, void* dq, void* workspace, void* stream);
int vd_cross_attention_bwd_dkdv(const vd_xattn_desc* x, const void* q, const void* k,
                                const void* v, const void* dout, const float* lse,
                                void* dk, void* dv, void* workspace, void* stream);

/* ---- data path (video-generation/dataset.py:68-139) ----------------
 * Frames: the reference's ToPILImage -> Resize((S, S)) -> ToTensor -> Normalize(0.5, 0.5)
 * (train.py:70-75, dataset.py:109-111) = PIL's antialiased bilinear resample.
 * vd_resize_plan (HOST, no GPU) computes one axis of PIL's plan (libImaging/Resample.c
 * precompute_coeffs + normalize_coeffs_8bpc): bounds int[out][2] (first tap, taps) and
 * 22-bit fixed-point coefficients int[out][ksize], ksize = 2 * ceil(in / out) + 1 (<= cap).
 * vd_frames_resize_normalize (GPU): uint8 frames [n][H][W][3] -> horizontal pass into tmp
 * (uint8 [n][H][OW][3]) -> vertical pass -> (v / 255 - 0.5) / 0.5 in `dtype`, frame f at
 * out + f * frame_stride as [3][OH][OW] (channels_last = 0) or [OH][OW][3] (channels_last =
 * 1); the uint8 values equal PIL's bit for bit.  frame_stride is in elements of `dtype` and
 * may exceed 3 * OH * OW: the elements between two frames are not written.  OH and OW are
 * independent (PIL's resize to (OW, OH)); tmp is n * H * OW * 3 bytes of scratch.  Both
 * layouts, a padded stride and OH != OW are tested against PIL, bit for bit
 * (tests/test_gpu_guarded_data.py).  Plans are device int arrays. */
int vd_resize_plan(int in_size, int out_size, int* bounds, int* coef, int ksize_cap);
int vd_frames_resize_normalize(const uint8_t* frames, int64_t n, int H, int W, int OH, int OW,
                               const int* xbounds, const int* xcoef, int xksize,
                               const int* ybounds, const int* ycoef, int yksize, uint8_t* tmp,
                               void* out, int dtype, int64_t frame_stride, int channels_last,
                               void* stream);
/* HOST (no GPU): the audio window of one output frame, dataset.py:113-130 -- samples
 * [int(sr * max(0, (out_frame - buffer_frames) / fps)), int(sr * out_frame / fps)) of the
 * track wave fp32 [channels][n]; torchaudio highpass_biquad(300 Hz, Q 0.707) with lfilter's
 * clamp to [-1, 1]; (x - mean) / std (unbiased, all channels); process_audio (:51-66):
 * resample to target_sr (bug_compatible = 1: from orig_freq = channels, as the reference's
 * size(0) comparison does; 0: from sr, identity when sr == target_sr; torchaudio's
 * sinc_interp_hann kernel, width 6, rolloff 0.99), zero-pad / trim to target_len; then the
 * Wav2Vec2 processor's (x - mean) / sqrt(var + 1e-7) per channel.  out fp32
 * [channels][target_len]. */
int vd_audio_window(const float* wave, int channels, int64_t n, int sr, double fps,
                    int out_frame, int buffer_frames, int target_len, int target_sr,
                    int bug_compatible, float* out);

/* ---- ViViT lipreading encoder ops (lipreading/huggingface_vivit_model.py:18-33
 * over transformers' VivitModel: VivitLayer.layernorm_before/_after, final layernorm, VivitMLP
 * with hidden_act "gelu_fast").
 * vd_layernorm_fwd: rows of C contiguous elements (C % 8 == 0, C <= 2048); fp32 affine w, b;
 * writes y and the fp32 per-row mean / rstd the backward reads.
 * vd_layernorm_bwd: dx (overwritten), dw = sum(dy * xhat), db = sum(dy) over rows (fp32,
 * overwritten, deterministic), through a workspace of vd_layernorm_workspace_size bytes.
 * vd_gelu_tanh(_bwd): y = 0.5 x (1 + tanh(0.7978845608 x (1 + 0.044715 x^2))) on n elements
 * (n % 8 == 0); bwd: dx = dy * y'(x). */
size_t vd_layernorm_workspace_size(int rows, int C);
int vd_layernorm_fwd(const void* x, const float* w, const float* b, void* y, float* mean,
                     float* rstd, int rows, int C, float eps, int dtype, void* stream);
int vd_layernorm_bwd(const void* dy, const void* x, const float* w, const float* mean,
                     const float* rstd, void* dx, float* dw, float* db, int rows, int C,
                     int dtype, void* workspace, size_t workspace_bytes, void* stream);
int vd_gelu_tanh(const void* x, void* y, int64_t n, int dtype, void* stream);
int vd_gelu_tanh_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype,
                     void* stream);

/* ---- clip quality metrics: per-frame MSE (PSNR) and SSIM, whole frame or weighted region
 * (build extension, no reference counterpart: the reference scores nothing) ----
 * x, y: two clips, contiguous [B][C][T][H][W] in `dtype` (a 4-D batch of images is T = 1), the
 * layout the samplers return; a frame is the C planes of one (b, t).  weight: fp32 [T][H][W],
 * >= 0, shared by batch and channel (the region; typically 1 - keep of masked sampling), or
 * NULL: a weight of ones, with the same bits as one.
 *   u          = clamp((v - lo) / (hi - lo), 0, 1): the data range is 1 (SSIM assumes
 *                intensities >= 0; sampler outputs are in [-1, 1] and may overshoot).  No 8-bit
 *                quantisation.
 *   mse[b, t]  = sum_c sum_px w[t, px] (ux - uy)^2 / (C sum_px w[t, px]);  PSNR = -10 log10(mse)
 *                is the caller's.
 *   SSIM (Wang et al. 2004): window g (x) g, g the 11-tap Gaussian with sigma 1.5, normalised in
 *   double and then rounded to fp32; VALID positions only, so a plane's map is (H - 10) x (W -
 *   10) and no padding convention enters; K1 = 0.01, K2 = 0.03, L = 1; window-weighted (biased)
 *   variances;
 *     s = (2 mx my + C1) (2 cxy + C2) / ((mx^2 + my^2 + C1) (vx + vy + C2)) per position;
 *   ssim[b, t] = sum_c sum_pos w s / (C sum_pos w), w taken at the window's centre pixel
 *                (y + 5, x + 5).
 *   wsum_px[t] = sum_px w,  wsum_valid[t] = sum_pos w (centres of valid positions).  A frame
 *   whose weight sum is 0 gets NaN in mse resp. ssim; the sums let the caller average over the
 *   frames that count.
 * Outputs (fp32, every element overwritten): mse [B * T], ssim [B * T], wsum_px [T], wsum_valid
 * [T]; ssim_map (may be NULL) [B * C * T][H - 10][W - 10], s before weighting.
 * Method: one workgroup per (plane, 32 x 32 tile of map positions) stages the 42 x 42 patches in
 * LDS as differences from the patch's centre pixel (variances as E[(x - p)^2] - E[x - p]^2, with
 * the exact correction for the fp32 window's sum: E[x^2] - E[x]^2 in fp32 is wrong by ~1e-7
 * against C2 = 9e-4 where frames are smooth), runs the separable window and reduces in a fixed
 * order into one record per (plane, tile) of `workspace` (vd_clip_metrics_workspace_size bytes,
 * 4-byte aligned, may be uninitialised); a second launch, one workgroup per (b, t), adds the
 * records in index order.  No atomics, no memset: the same bits eager and replayed from a HIP
 * graph.  Rows need no alignment.  H < 11 or W < 11, a NULL pointer (weight and ssim_map
 * excepted), hi <= lo, non-positive sizes and an unknown dtype fail before any launch. */
size_t vd_clip_metrics_workspace_size(int B, int C, int T, int H, int W);
int vd_clip_metrics(const void* x, const void* y, const float* weight, float lo, float hi, int B,
                    int C, int T, int H, int W, int dtype, float* mse, float* ssim,
                    float* wsum_px, float* wsum_valid, float* ssim_map, void* workspace,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VDIFF_H */

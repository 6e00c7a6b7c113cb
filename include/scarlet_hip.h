/*
 * scarlet_hip.h -- C ABI of the MI355X (gfx950) proximal-gradient deblending engine.
 *
 * Drop-in boundary for the hot path of scarlet's Blend.fit().
 * The reference's only native boundary is the pybind11 module built from
 * scarlet/operators_pybind11.cc; everything else on the path is numpy called from
 * Python.  This header therefore has three groups:
 *
 *   1. host-pointer drop-ins for the three pybind11 functions (same argument
 *      meaning, caller-owned host buffers mutated in place),
 *   2. batched device-pointer operators -- one call per (reference function x batch
 *      of arrays): these are what scarlet_amd/operator.py, update.py, measurement.py
 *      bind, i.e. what a maintainer would call from the reference's operator.py /
 *      update.py / measurement.py in place of the numpy code,
 *   3. the batched Blend.fit() engine (state struct + iteration driver).
 *
 * Conventions: plain C types only.  Device pointers are HIP device pointers into
 * memory owned by the caller (PyTorch-ROCm tensors in the Python host layer).  All
 * device arrays are C-contiguous float32 unless stated otherwise.  `stream` is a
 * hipStream_t passed as void*; every device entry point is asynchronous on it and
 * allocates nothing.  Return value: 0 = ok, negative = SCARLET_E_* (argument errors
 * are detected on the host before any launch).
 *
 * Threads and global state.  Every entry point may be called from several host threads at once
 * on different batches / streams; scarlet_last_error() is per thread.  The library keeps exactly
 * four process-wide objects, each behind its own mutex or atomic: the constant table of fast
 * FFT lengths (filled once per device), the hipFFT plan cache of the large-frame fallback of the
 * PSF path, the diagnostic switches of scarlet_set_option(), and the event recorder of
 * scarlet_profile_begin/end (one profiled region at a time, whichever batch launches inside it).
 * Per calling thread (and device) it keeps one further stream and three events: with more than eight
 * components per scene the Gram matrix and its eigenvalue run beside the morphology step, forked from and
 * joined back into the caller's stream by events -- to the caller the entry point stays asynchronous on
 * the stream it passed, and a stream capture records both branches.
 * Set-up and host-pointer entry points that need temporary device memory release it on every
 * exit path, error paths included.
 */
#ifndef SCARLET_HIP_H
#define SCARLET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCARLET_OK            0
#define SCARLET_E_ARG        -1   /* bad shape / null pointer / unsupported option  */
#define SCARLET_E_TOO_LARGE  -2   /* frame side larger than SCARLET_MAX_SIDE        */
#define SCARLET_E_HIP        -3   /* a HIP runtime call failed (see scarlet_last_error) */
#define SCARLET_E_NOTIMPL    -4   /* reference raises NotImplementedError here      */

/* largest frame side (H and W, square or not) of the engine, init_extended and the operators */
#define SCARLET_MAX_SIDE     1024
/* most components per scene (K) of the engine and init_extended; more: SCARLET_E_NOTIMPL */
#define SCARLET_MAX_COMPONENTS 256
/* most observations of scarlet_fit_observations / scarlet_fit_multi */
#define SCARLET_MAX_OBSERVATIONS 8
/* most channels of the model frame of a joint fit (scarlet_fit_observations_wide); one observation, and a batch fitted
   on its own, has at most 8 bands */
#define SCARLET_MAX_CHANNELS 32

/* BlendFlag bits -- scarlet/component.py:13-36 */
#define SCARLET_FLAG_SED_NOT_CONVERGED   1
#define SCARLET_FLAG_MORPH_NOT_CONVERGED 2
#define SCARLET_FLAG_EDGE_PIXELS         4
#define SCARLET_FLAG_NO_VALID_PIXELS     8

/* per-scene status bits written by the engine (0 = healthy) */
#define SCARLET_STATUS_CENTER_AT_EDGE    1  /* max_pixel window start < 0: the reference
                                               would raise (measurement.py:24-29)          */
#define SCARLET_STATUS_NONFINITE         2  /* NaN/Inf met in centroid or normalisation   */
#define SCARLET_STATUS_BAD_COUNT         4  /* n_components[s] outside 1..K: the scene is
                                               left untouched and inactive                 */
#define SCARLET_STATUS_BAD_OPTION       32  /* a row of scarlet_update_options of this scene holds an
                                               unknown or out-of-range value: the scene is left
                                               untouched and inactive                      */
#define SCARLET_STATUS_BAD_INIT          8  /* bad input of scarlet_init_sources in this scene:
                                               it is left untouched and inactive           */
#define SCARLET_STATUS_BAD_FRAME        16  /* frame_hw[s] outside 1..H x 1..W: the scene is
                                               left untouched and inactive                 */

/* source types of scarlet_init_sources (scarlet_init_spec::kind) */
#define SCARLET_INIT_EXTENDED 0   /* ExtendedSource (source.py:139-180, 443-492)                */
#define SCARLET_INIT_POINT    1   /* PointSource (source.py:340-400)                            */
/* most members of one multi-component source that scarlet_init_sources layers */
#define SCARLET_MAX_LAYERS    8

/* symmetry algorithms -- scarlet/operator.py:291-350 */
#define SCARLET_SYM_KSPACE 0
#define SCARLET_SYM_SOFT   1
#define SCARLET_SYM_SDSS   2
/* or-ed into `algorithm`: apply the bare operator to the WHOLE array, symmetric about
 * index (H/2, W/2) -- operator.prox_soft/sdss/kspace_symmetry called directly -- instead of
 * going through uncentered_operator's window selection */
#define SCARLET_SYM_FULL_WINDOW 16

/* normalisation types -- scarlet/update.py:35-68 */
#define SCARLET_NORM_SED       0
#define SCARLET_NORM_MORPH     1
#define SCARLET_NORM_MORPH_MAX 2
#define SCARLET_NORM_NONE      3   /* scarlet_update_options only: the update does not normalise */
/* scarlet_update_options::positive -- update.positive_sed / positive_morph / positive (update.py:13-32) */
#define SCARLET_POSITIVE_SED   1
#define SCARLET_POSITIVE_MORPH 2

const char *scarlet_version(void);
const char *scarlet_last_error(void);
/* Diagnostic switches: NO_EXACT, NO_KSCACHE, FUSED_V1, NO_FUSED, FORCE_BLOCK_UPDATE,
 * NO_HYBRID_SWEEP, PAD_LDS, STAMPS, PSF_HIPFFT, NO_BOX, NO_BOX2, NO_PSF3PASS, NO_SIDE_STREAM,
 * NO_GRAM_MFMA, NO_BIGK_FUSED, NO_PIPELINE, NO_PERSIST (one launch per iteration instead of k_fit2x),
 * PERSIST_DBG, NO_PLACE (component k on waves 2k, 2k + 1 of k_fit2x / k_iterate2<4,5,64>, not placed by
 * GEMM cost), NO_LOWRES_MFMA (the GEMMs of a low-resolution observation as plain FMA chains, bit-identical),
 * LOWRES_STREAMED (the *_large low-resolution entry points take the streamed form for shapes that fit LDS as well),
 * LOWRES_CHUNK (planes per chunk of the streamed form, 0 = automatic; it can only lower the chunk; the one switch whose
 * value is a count: scarlet_set_option returns its previous value, negative values are SCARLET_E_ARG).  Each starts from the environment variable SCARLET_<NAME>, read once at first use;
 * afterwards only this call changes it.  Returns the previous value (0 / 1) or SCARLET_E_ARG for an
 * unknown name.  None changes results beyond float32 rounding.
 * PSF_HIPFFT and STAMPS decide the layout of a PSF batch's workspace: they are frozen by the first
 * scarlet_batch_workspace_bytes / scarlet_batch_prepare_psf call of the process on a batch with a
 * PSF; a later call that would change either returns SCARLET_E_ARG and changes nothing. */
int scarlet_set_option(const char *name, int value);
/* Diagnostics: with the STAMPS switch on, kernels that carry phase stamps (k_source_update_box: 16 shader-clock
 * values per component) write them into a buffer owned by the library; this copies up to `capacity` of
 * them to `out` (host) after a device synchronisation and returns the count (0 when the switch is off). */
int64_t scarlet_debug_stamps(int64_t *out, int64_t capacity);
/* 5-smooth fast FFT length (scipy.fftpack.next_fast_len as used by fft.py:99) */
int scarlet_next_fast_len(int n);

/* ------------------------------------------------------------------------------
 * 1. Host-pointer drop-ins for scarlet/operators_pybind11.cc
 * ---------------------------------------------------------------------------- */

/* replaces prox_monotonic (operators_pybind11.cc:11-25): x[d] = min(x[d],
 * x[ref_idx[d]]*(1-thresh)) for d in dist_idx order.  x: n doubles, mutated. */
int scarlet_host_prox_monotonic_f64(double *x, int n, const int *ref_idx,
                                    const int *dist_idx, int n_dist, double thresh);

/* replaces prox_weighted_monotonic<float> / <double> (operators_pybind11.cc:27-50,
 * 82-85).  weights: row-major [8][n] (numpy order), offsets: 8 flat neighbour
 * offsets, dist_idx: radius-sorted pixel indices without the peak.  x mutated. */
int scarlet_host_prox_weighted_monotonic_f32(float *x, int n, const float *weights,
                                             const int *offsets, const int *dist_idx,
                                             int n_dist, float thresh);
int scarlet_host_prox_weighted_monotonic_f64(double *x, int n, const double *weights,
                                             const int *offsets, const int *dist_idx,
                                             int n_dist, double thresh);

/* replaces apply_filter<float> / apply_filter<double> (operators_pybind11.cc:53-70; both overloads are
 * exported, :87-88): result = sum_n values[n] * shifted block of image. */
int scarlet_host_apply_filter_f32(const float *image, int H, int W, const float *values,
                                  const int *y_start, const int *y_end, const int *x_start,
                                  const int *x_end, int n, float *result);
int scarlet_host_apply_filter_f64(const double *image, int H, int W, const double *values,
                                  const int *y_start, const int *y_end, const int *x_start,
                                  const int *x_end, int n, double *result);

/* ------------------------------------------------------------------------------
 * 2. Batched device operators (n arrays of H x W, row stride W, array stride H*W)
 * ---------------------------------------------------------------------------- */

/* update.monotonic default path: operator.prox_strict_monotonic(use_nearest=False)
 * -> operators_pybind11.prox_weighted_monotonic (update.py:106-156, operator.py:81-122,
 * 540-621).  The radial cos-weights and the sweep order are generated on the fly from
 * `centers` (device int32 [n][2] = (y, x)); no weight table, no argsort.  In place. */
int scarlet_prox_weighted_monotonic(float *x, int n, int H, int W, const int32_t *centers,
                                    float thresh, void *stream);

/* operator.prox_strict_monotonic(use_nearest=True) (operator.py:104-113): reference pixel
 * = first neighbour with the largest cos-weight.  thresh must be 0 (ValueError in the
 * reference otherwise -> SCARLET_E_ARG). */
int scarlet_prox_nearest_monotonic(float *x, int n, int H, int W, const int32_t *centers,
                                   float thresh, void *stream);

/* operator.prox_uncentered_symmetry (operator.py:291-350) incl. uncentered_operator
 * window selection (:175-228), prox_soft_symmetry (:242-251), prox_sdss_symmetry
 * (:231-239), prox_kspace_symmetry (:253-288, evaluated as the equivalent real-space
 * Dirichlet-kernel operator).  shifts: device float64 [n][2] = (dy, dx)
 * or NULL; `algorithm` is applied as given (the caller resolves the reference's
 * "kspace -> soft when shift is None/0" rule, operator.py:337-339).  use_fill != 0
 * writes `fill` outside the symmetric window.  In place. */
int scarlet_prox_symmetry(float *x, int n, int H, int W, const int32_t *centers,
                          const double *shifts, int algorithm, float strength,
                          int use_fill, float fill, void *stream);

/* measurement.max_pixel (measurement.py:3-29): 5x5 window argmax, first hit row-major.
 * centers_io updated in place; status (device int32 [n] or NULL) gets
 * SCARLET_STATUS_CENTER_AT_EDGE or-ed in when the reference would have failed. */
int scarlet_max_pixel(const float *x, int n, int H, int W, int32_t *centers_io,
                      int32_t *status, void *stream);

/* measurement.psf_weighted_centroid (measurement.py:32-94).  psf: device float64 [P][P]
 * (P odd).  centers_io updated, shifts_out float64 [n][2]. */
int scarlet_psf_weighted_centroid(const float *x, int n, int H, int W, const double *psf,
                                  int P, int32_t *centers_io, double *shifts_out,
                                  int32_t *status, void *stream);

/* proxmin prox_plus / prox_hard / prox_soft as bound by update.py:13-32,71-82.
 * `count` contiguous floats; step per call (thresh*step is the cut). */
int scarlet_prox_plus(float *x, int64_t count, void *stream);
int scarlet_prox_hard(float *x, int64_t count, float thresh_times_step, void *stream);
int scarlet_prox_soft(float *x, int64_t count, float thresh_times_step, void *stream);

/* update.normalized (update.py:35-68) for n components: sed [n][B], morph [n][H*W]. */
int scarlet_normalize(float *sed, float *morph, int n, int B, int HW, int type, void *stream);

/* measurement.threshold (measurement.py:97-112), device part, for n arrays of `count` floats:
 * scarlet_log_range: out [n][3] float64 = {number of positive pixels, min, max of their log10};
 * scarlet_log_hist: np.histogram of log10(positive pixels) over nbins[i] <= 50 equal bins whose
 * edges [n][51] float64 the caller tabulates (np.linspace, as numpy does); hist [n][50] int32.
 * The caller picks the lower edge of the last empty bin (measurement.py:107-112). */
int scarlet_log_range(const float *x, int n, int64_t count, double *out, void *stream);
int scarlet_log_hist(const float *x, int n, int64_t count, const double *edges,
                     const int32_t *nbins, int32_t *hist, void *stream);
/* update.threshold (update.py:98): x[x < thresh] = 0. */
int scarlet_cut_below(float *x, int64_t count, double thresh, void *stream);
/* bbox.trim (bbox.py:174-193) for n planes [H][W]: box [n][4] int32 = {bottom, top, left, right} of
 * x > min_value (inclusive bounds); {H, -1, W, -1} when no pixel qualifies. */
int scarlet_trim(const float *x, int n, int H, int W, float min_value, int32_t *box, void *stream);
/* interpolation.fft_resample (interpolation.py:408-448) as used by update.translation
 * (update.py:159-167), n planes [H][W], out of place: separable taps [n][2][12] float64 (ky, kx:
 * ny / nx <= 12 of them used), first tap positions win0 [n][2] int32 (the kernels' window[0]). */
int scarlet_resample(const float *in, float *out, int n, int H, int W, const double *taps,
                     const int32_t *win0, int ny, int nx, void *stream);

/* apply_filter on device (operators_pybind11.cc:53-70), one image. */
int scarlet_apply_filter(const float *image, int H, int W, const float *values,
                         const int32_t *y_start, const int32_t *y_end, const int32_t *x_start,
                         const int32_t *x_end, int n, float *result, void *stream);

/* fft.match_psfs (fft.py:282-301) for n PSFs on the device: out[i] = the difference kernel that
   turns psf2[i] (or psf2[0] when n2 == 1) into psf1[i]: ratio of the spectra at the reference's
   FFT shape next_fast_len(P1 + P2 + 3) (last axis even), cropped to psf1's shape.
   psf1 [n][P1y][P1x], psf2 [n2][P2y][P2x], out [n][P1y][P1x], all device float32. */
int scarlet_match_psfs(const float *psf1, int n, int P1y, int P1x, const float *psf2, int n2,
                       int P2y, int P2x, float *out, void *stream);

/* ------------------------------------------------------------------------------
 * 3. Batched Blend.fit() engine (blend.py:65-223, source.py:402-440)
 *
 * Supported shapes: K <= SCARLET_MAX_COMPONENTS (256) components per scene, B <= 8
 * bands, frames up to SCARLET_MAX_SIDE (1024) pixels on either side,
 * with or without a PSF difference kernel.  Which kernels run is an internal choice:
 * one fused launch per iteration when the K morphology tiles fit LDS (H, W <= 64), the
 * four-kernel general path otherwise, chunked gradient passes for K > 8, operators in
 * place in HBM for frames beyond the LDS tile.  Results do not depend on the choice
 * beyond float32 rounding.
 * ---------------------------------------------------------------------------- */

typedef struct scarlet_batch {
    /* shapes: S scenes, K components per scene (at most: see n_components), B bands, H x W pixels (scenes with frames
       of their own inside H x W: struct scarlet_frames and the _frames entry points, below; this struct does not change) */
    int32_t S, K, B, H, W;
    /* data (read only) */
    const float *images;      /* [S][B][H][W]                                          */
    const float *weights;     /* [S][B][H][W] or NULL -> scalar `weight_scalar`
                                 (observation.py:148-151)                              */
    float weight_scalar;
    /* factors, ping-pong: buffer `cur` holds the current values, the other one the
       values of the previous iteration (_last_sed/_last_morph, blend.py:179-182)      */
    float *sed[2];            /* [S][K][B]                                             */
    float *morph[2];          /* [S][K][H][W]                                          */
    int32_t *cur;             /* [S] device: index of each scene's current buffer; a scene's
                                 index flips once per iteration it takes part in        */
    /* per component */
    int32_t *centers;         /* [S][K][2] pixel_center (y, x)                         */
    double *shifts;           /* [S][K][2] sub-pixel shift from the last centroid      */
    int32_t *flags;           /* [S][K]    BlendFlag bits                              */
    const uint8_t *fix_sed;   /* [S][K] or NULL (component.py:111-112)                 */
    const uint8_t *fix_morph; /* [S][K] or NULL                                        */
    /* per scene */
    double *lipschitz;        /* [S][2]  (L_sed, L_morph) of the last iteration        */
    double *mse;              /* [S][mse_capacity] loss before each step (blend.py:138) */
    int32_t mse_capacity;
    int32_t *it;              /* [S] = len(mse)                                        */
    int32_t *active;          /* [S] 1 while the scene has not met e_rel in this fit()  */
    int32_t *status;          /* [S] SCARLET_STATUS_* bits                             */
    /* constraint pipeline of PointSource/ExtendedSource.update (source.py:402-440)    */
    int32_t symmetric, monotonic;
    float l0_thresh, l1_thresh;  /* < 0 -> off; else update.sparse_l0/l1 before positive */
    const double *centroid_psf;  /* [P][P] float64 centroid weight (source.py:483-490) */
    int32_t centroid_P;
    /* PSF difference kernel of Observation.match (observation.py:191-194): NULL (render =
       identity), [B][psf_h][psf_w] shared by all scenes (diff_kernel_per_scene = 0), or one
       set per scene [S][B][psf_h][psf_w] (diff_kernel_per_scene = 1: every scene was observed
       with its own PSFs).  When set, call scarlet_batch_prepare_psf() once before fitting
       (and again if it changes).                                                         */
    const float *diff_kernel;
    int32_t psf_h, psf_w;
    int32_t diff_kernel_per_scene;
    /* workspace owned by the caller: scarlet_batch_workspace_bytes() bytes, ZEROED before
       the first call (it also holds a cache keyed by a magic word)                     */
    void *workspace;
    /* MultiComponentSource (source.py:538-641): [S][K] device int32 or NULL.  -1: the component is a
       source of its own (PointSource / ExtendedSource.update, source.py:402-440); g >= 0: it is a layer of
       multi-component source g of its scene -- the layers of a source share ONE centre, measured on their
       flux-weighted sum (max_pixel, and psf_weighted_centroid every fifth iteration, source.py:613-630),
       and are symmetrised about it with shift = None (update.symmetric falls back to soft symmetry,
       operator.py:337-339).  The members of a source must be adjacent components.             */
    const int32_t *group;
    /* Ragged batches: [S] device int32, or NULL = every scene has K components.  Scene s uses components
       0 .. n_components[s] - 1; components n_components[s] .. K - 1 are ABSENT:
         - their factors must be zero in both buffers (sed[0/1], morph[0/1]) when a call starts; the library
           never reads them and never writes anything non-zero to them, so they stay exactly zero and add
           nothing to the model, the loss, the gradients or the Lipschitz constants;
         - their centers / shifts are not read, and their flags are left at 0 (set them to 0);
         - group[s][k] must be -1 for an absent component;
         - they never enter the constraint pipeline, the initialisation or the convergence test.
       Every entry point that iterates or initialises checks the counts on the device first: a scene whose
       count lies outside 1..K gets SCARLET_STATUS_BAD_COUNT and active = 0 and is not touched again; the
       other scenes go on.  The workspace does not depend on the counts.  scarlet_fit_multi does not take
       them (SCARLET_E_NOTIMPL); scarlet_fit_observations does.                                         */
    const int32_t *n_components;
} scarlet_batch;

/* bytes of device workspace needed for `b`.  Depends on S, K, B, H, W; on diff_kernel (NULL or not), psf_h, psf_w and
   diff_kernel_per_scene; on group (NULL or not: it rules out two pipelines); and on the switches FORCE_HUGEK
   (8 < K <= 32), PSF_HIPFFT and STAMPS (batches with a PSF), which this call fixes for the rest of the process */
int64_t scarlet_batch_workspace_bytes(const scarlet_batch *b);
/* Number of pipelines scarlet_fit() runs `b` as: 2 for a large batch with a PSF (>= 1024 scenes, K <= 8, the
 * LDS-resident transform) -- the two halves of the batch as views with their own workspace regions, the second on the
 * calling thread's second stream, joined back into the caller's stream before scarlet_fit() returns or synchronises,
 * so that one half's convolution (latency-bound) runs beside the other half's streaming passes; results are
 * bit-identical to one pipeline (scenes are independent).  1 otherwise, and with the NO_PIPELINE switch. */
int scarlet_batch_pipelines(const scarlet_batch *b);

/* Run up to `max_iter` proximal-gradient iterations on every active scene
 * (Blend.fit, blend.py:65-102).  Per iteration and scene: loss + analytic gradient
 * (_backward/_loss, :105-139), Lipschitz constants (_set_lipschitz, :186-223, exact or
 * approximate), gradient step (:87-96), per-component constraint pipeline
 * (source.py:402-440), convergence flags (_check_convergence, :141-184).  A scene that
 * converges stops iterating (its `active` becomes 0), exactly like the reference's
 * `break`.  `check_every` > 0: every that many iterations the active flags are copied
 * to the host (one stream sync) to stop early when every scene is done; 0: never sync.
 * Returns the number of iterations launched (>= 0) or an error. */
int scarlet_fit(scarlet_batch *b, int max_iter, double e_rel, int approximate_L,
                int check_every, void *stream);

/* Blend.fit with SEVERAL observations (blend.py:24-43, 120-139, 219-220) for a whole batch, no host synchronisation per
 * iteration.  `state` holds the factors over the model frame's C = state->B channels (its `images` and `weights` are
 * not read: pass any buffer of the right size) and governs everything but the data: counts (n_components), fix_sed /
 * fix_morph, centres, the constraint pipeline and the convergence test.  obs[i] (1 <= n_obs <= SCARLET_MAX_OBSERVATIONS)
 * is a batch over the channels band0[i] .. band0[i] + obs[i]->B - 1 of the model (observations may overlap in
 * channels, e.g. two epochs of the same bands) with its own images / weights / PSF kernel (prepared by
 * scarlet_batch_prepare_psf) / workspace and the same S, K, H, W; its n_components must be NULL (SCARLET_E_ARG), its
 * factor buffers are scratch of this call (sed[0] holds the band slice its PSF chain reads).  Per iteration: the loss
 * summed over the observations, ONE pass over the state's morphologies for all of them (no morphology copies), L_sed =
 * n_obs lambda_max(S S^T), L_morph = n_obs lambda_max(A^T A) over the C channels (or the approximate form of
 * blend.py:189-201 on the summed loss), the step, the constraint pipeline and the convergence test on `state`.
 * Returns the number of iterations launched. */
int scarlet_fit_observations(scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                             int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
/* The same without ragged batches (state->n_components or an observation's: SCARLET_E_NOTIMPL). */
int scarlet_fit_multi(scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                      int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
/* CombinedExtendedSource's SED (source.py:183-240 through get_psf_sed, source.py:41-71) from one observation: for every
 * present component of a scene without SCARLET_STATUS_BAD_INIT, channels band0 .. band0 + B - 1 of buffer cur get the
 * observation's pixel values at the centre (images: device [S][B][H][W]), divided by obs_psf_peak (device [B], or
 * [S][B] when peak_per_scene; NULL: no division) and multiplied by *model_psf_max (device float; NULL: no factor).
 * The morphology is scarlet_init_sources on the batch of observation obs_idx (symmetric, no update). */
int scarlet_init_combined_sed(scarlet_batch *state, const float *images, int B, int band0, const float *obs_psf_peak,
                              int peak_per_scene, const float *model_psf_max, void *stream);

/* Components with a Prior (component.py:39-67, 177-187; blend.py:86-96): a gradient and a Lipschitz constant that
 * are added to ONE component's step.  scarlet_batch does not change; the prior travels in a struct of its own.  Every
 * pointer is device memory owned by the caller, float32 unless stated, indexed like the batch ([S][K] per component);
 * any of the inputs may be NULL.  Per active scene and present component k, on the factors x of buffer cur:
 *     g_prior = given gradient + w (x - target)          L_k = L + given L + w     (float32, as the frame's dtype)
 *     x' = x - (1 / L_k) (g + g_prior)                   unless fix_sed / fix_morph: x' = x and L_k = L
 * with g, L the likelihood's gradient and the scene's constant as scarlet_backward_gradients computes them
 * (`lipschitz` and `mse` keep their meaning: no prior in them).  The constraint pipeline that follows scales the
 * sparse_l0 / sparse_l1 cut with the component's own step 1 / L_morph,k (update.py:71-82).  Absent components,
 * inactive scenes and the rows of L_comp that belong to them are not read and not written. */
typedef struct scarlet_prior {
    /* given values, e.g. what the caller's own code computed from buffer cur for this iteration */
    const float *grad_sed;          /* [S][K][B]     added to d loss / d sed   */
    const float *grad_morph;        /* [S][K][H][W]  added to d loss / d morph */
    const float *L_sed;             /* [S][K]        added to the component's L_sed   */
    const float *L_morph;           /* [S][K]        added to the component's L_morph */
    /* built-in quadratic prior  w/2 |x - target|^2, evaluated by the library on buffer cur:
       gradient w (x - target), Lipschitz constant w; target NULL = 0; a target needs its weight */
    const float *quad_sed_weight;   /* [S][K]        */
    const float *quad_sed_target;   /* [S][K][B]     */
    const float *quad_morph_weight; /* [S][K]        */
    const float *quad_morph_target; /* [S][K][H][W]  */
    /* out, required: the constants each component stepped with, {L_sed, L_morph} */
    double *L_comp;                 /* [S][K][2]     */
} scarlet_prior;

/* scarlet_backward_step with priors: the gradient pass, then one streaming kernel (k_prior_step) that steps the
 * gradients in buffer 1-cur in place and writes L_comp; cur / it are not advanced.  For callers that recompute the
 * given arrays every iteration. */
int scarlet_backward_step_prior(scarlet_batch *b, const scarlet_prior *p, int approximate_L, void *stream);
/* scarlet_source_update for a batch that stepped with priors: the sparsity cut reads p->L_comp (the only field it uses) */
int scarlet_source_update_prior(scarlet_batch *b, const scarlet_prior *p, int in_iteration, void *stream);
/* scarlet_fit with priors whose inputs do not change between iterations (the quadratic form, constant given
 * gradients): gradients, prior step, constraint pipeline, convergence test per iteration, on the general
 * (unfused, one-pipeline) path; no host synchronisation other than the check_every one, no allocation.  Returns the
 * number of iterations launched.  Several observations with priors: scarlet_fit_observations_prior (below). */
int scarlet_fit_prior(scarlet_batch *b, const scarlet_prior *p, int max_iter, double e_rel, int approximate_L,
                      int check_every, void *stream);

/* Components with their own constraint switches (PointSource / ExtendedSource default to symmetric=True,
 * CombinedExtendedSource to symmetric=False, and every constructor takes symmetric= and monotonic=, source.py:340-492):
 * the four settings of the constraint pipeline per component instead of per batch.  scarlet_batch does not change; the
 * settings travel in a struct of their own, device memory owned by the caller, indexed like the batch.
 *   - Rows of absent components and of inactive scenes are not read.
 *   - A given `symmetric` array needs an odd-sized centroid_psf in the batch; otherwise the call returns SCARLET_E_ARG,
 *     found on the host before any launch (as for the scalar b->symmetric).
 *   - c == NULL is SCARLET_E_ARG.
 *   - The members of one multi-component source (group >= 0) must agree on `symmetric` and `monotonic`: the source's
 *     shared centre (k_group_centers) reads the first member's value.
 *   - The workspace layout does not depend on the struct (nor on the batch's four scalars).
 *   - The caller sets b->symmetric and b->monotonic to the OR over its arrays: the library uses those scalars only for
 *     decisions that must err on the side of "some component needs it" (the centroid PSF check, the box kernels of
 *     frames beyond 64 x 64, which serve the monotonic components and leave the others to the full-frame kernel).
 *   - With every pointer NULL the three entry points behave exactly as scarlet_fit / scarlet_fit_prior,
 *     scarlet_source_update / scarlet_source_update_prior and scarlet_fit_observations do.
 * A component without `symmetric` runs no centroid and its `shifts` are not touched; one without `monotonic` is
 * normalised by the maximum over its whole plane.  Batches that take the one-launch iteration (K <= 4, frames up to
 * 64 x 64 with W % 4 == 0, no PSF, exact L, no prior, no group) keep it: the four-wave kernel reads each wave's own
 * component's settings (profile class 4).  So do ragged-frame batches (scarlet_fit_frames, below) of that size class. */
typedef struct scarlet_constraints {
    const uint8_t *symmetric;   /* device [S][K], or NULL = b->symmetric for every component */
    const uint8_t *monotonic;   /* device [S][K], or NULL = b->monotonic                     */
    const float   *l0_thresh;   /* device [S][K], < 0 = off, or NULL = b->l0_thresh          */
    const float   *l1_thresh;   /* device [S][K], < 0 = off, or NULL = b->l1_thresh          */
} scarlet_constraints;          /* 32 bytes */

/* scarlet_fit (p == NULL) or scarlet_fit_prior (p given) with per-component switches */
int scarlet_fit_constrained(scarlet_batch *b, const scarlet_constraints *c, const scarlet_prior *p /* or NULL */,
                            int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
/* scarlet_source_update / scarlet_source_update_prior with per-component switches.  in_iteration = 0 (the constructors'
 * update, which ignores `active`) with any array given leaves scenes with SCARLET_STATUS_BAD_INIT or
 * SCARLET_STATUS_BAD_COUNT untouched. */
int scarlet_source_update_constrained(scarlet_batch *b, const scarlet_constraints *c, const scarlet_prior *p /* or NULL: only L_comp is read */,
                                      int in_iteration, void *stream);
/* scarlet_fit_observations with per-component switches on the state */
int scarlet_fit_observations_constrained(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs,
                                         const int32_t *band0, int n_obs, int max_iter, double e_rel,
                                         int approximate_L, int check_every, void *stream);

/* The stock update functions' other options (update.symmetric(algorithm=, strength=), update.monotonic(use_nearest=,
 * thresh=), update.positive / positive_sed / positive_morph, update.normalized(type=); update.py:13-199): what a user who
 * overrides PointSource / ExtendedSource.update (source.py:402-440, "can be overwritten if a different set of constraints or
 * update functions is desired") changes most often, per component.  scarlet_batch does not change; the options travel in a
 * struct of their own beside scarlet_constraints, device memory owned by the caller, indexed like the batch.  They need no
 * workspace.  The order of the pipeline stays that of source.py:402-440: max_pixel, (symmetric: the centroid every fifth
 * iteration whatever the algorithm, then the symmetry), (monotonic: the sweep), sparse_l0 / sparse_l1, positive, normalized.
 *   - o == NULL is SCARLET_E_ARG.  With every member NULL the three entry points ARE scarlet_fit_constrained (p = NULL),
 *     scarlet_source_update_constrained (p = NULL) and scarlet_fit_observations_constrained, bit for bit; `c` may be NULL.
 *   - Rows of absent components and of inactive scenes are not read.
 *   - Before anything else one thread per scene checks the rows of the scene's present components on the device
 *     (k_check_options): an unknown algorithm, normalisation or positive value, a strength outside [0, 1], a thresh outside
 *     [0, 1), or a thresh != 0 with mono_nearest (the reference raises ValueError, operator.py:107-110) gives the scene
 *     SCARLET_STATUS_BAD_OPTION and active = 0; the scene is left untouched (also by the constructors' update) and the
 *     other scenes go on.
 *   - SCARLET_E_NOTIMPL, found on the host before any launch: a batch with `group` (layers are tied to soft symmetry with
 *     shift = None), a wide state (state->B > 8).  There is no prior, no scarlet_frames and no low-resolution argument.
 *     Groups and ragged frames with options go through scarlet_fit_frames_options /
 *     scarlet_source_update_frames_options (declared after struct scarlet_frames, below): a layer takes its source's shared
 *     centre as given and has no shift, so _KSPACE is soft symmetry with strength 1 for it, _SOFT uses its strength and
 *     _SDSS is sdss; the norms of type _MORPH and _SED sum the pixels of the scene's own frame only.
 *   - A batch with options takes the general path: no one-launch iteration, one pipeline, no box stage beyond 64 pixels; the
 *     full-frame forms of the constraint kernels (their options instances, engine.h) serve every component.
 *   - sym_algorithm: SCARLET_SYM_KSPACE still falls back to soft symmetry with strength 1 while the component has no shift
 *     (NaN); the in-place operators (_SOFT, _SDSS) act on the whole array where the centre is the array's middle, k-space is
 *     a no-op there (uncentered_operator, operator.py:203-204).  sym_strength is read for _SOFT only.
 *   - mono_nearest: the reference pixel is the first neighbour of largest cosine towards the peak (operator.py:591-600):
 *     x = min(x, x_ref), swept ring by ring (the reference pixel lies on the previous Chebyshev ring), exact in any precision.
 *   - positive: bit 0 (SCARLET_POSITIVE_SED) clamps the SED at 0, bit 1 (SCARLET_POSITIVE_MORPH) the morphology.
 *   - normalize: _MORPH_MAX divides the morphology by its maximum and multiplies the SED by it, _MORPH does the same with
 *     morph.sum(), _SED divides the SED by sed.sum() and multiplies the morphology by it, _NONE leaves both.  A norm that is
 *     not positive and finite sets SCARLET_STATUS_NONFINITE.  The convergence sums are taken on what is written. */
typedef struct scarlet_update_options {      /* device [S][K] each, or NULL = the default */
    const uint8_t *sym_algorithm;   /* SCARLET_SYM_KSPACE (default) | _SOFT | _SDSS                                    */
    const float   *sym_strength;    /* soft only; default 0.5 (update.py:170); in [0, 1]                               */
    const uint8_t *mono_nearest;    /* 0 (default): weighted sweep; 1: nearest neighbour                               */
    const float   *mono_thresh;     /* default 0; in [0, 1); must be 0 where mono_nearest                              */
    const uint8_t *positive;        /* bit 0 sed, bit 1 morph; default 3                                               */
    const uint8_t *normalize;       /* SCARLET_NORM_MORPH_MAX (default) | _MORPH | _SED | _NONE                        */
} scarlet_update_options;           /* 48 bytes */

/* scarlet_fit_constrained (p = NULL) with update options; c may be NULL */
int scarlet_fit_options(scarlet_batch *b, const scarlet_constraints *c /* or NULL */, const scarlet_update_options *o,
                        int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
/* scarlet_source_update_constrained (p = NULL) with update options: the constructors' update() (in_iteration = 0) leaves
 * scenes with SCARLET_STATUS_BAD_OPTION, _BAD_INIT or _BAD_COUNT untouched */
int scarlet_source_update_options(scarlet_batch *b, const scarlet_constraints *c /* or NULL */, const scarlet_update_options *o,
                                  int in_iteration, void *stream);
/* scarlet_fit_observations_constrained with update options on the state (same-grid observations, state->B <= 8) */
int scarlet_fit_observations_options(scarlet_batch *state, const scarlet_constraints *c /* or NULL */,
                                     const scarlet_update_options *o, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                                     int max_iter, double e_rel, int approximate_L, int check_every, void *stream);

/* Ragged frames: scenes of different frame sizes in one batch.  scarlet_batch does not change; the shapes travel in a
 * struct of their own.  frame_hw: device [S][2] int32 (h, w), or NULL = every scene is H x W (the _frames entry points then
 * ARE their plain counterparts, bit for bit).  Scene s has its own frame of 1 <= h <= H by 1 <= w <= W pixels in the
 * top-left corner of its padded H x W planes (row stride W).  Its result is what the reference computes for the (B, h, w)
 * scene alone:
 *   - pixels outside the frame do not exist: they are no neighbour, partner or window pixel of any constraint (max_pixel,
 *     centroid, symmetry window and monotonic sweep take the scene's bounds), and the convergence sums run over the
 *     scene's pixels.  After every call they are exactly 0.0f in both morphology buffers (they must be when the first
 *     call starts);
 *   - the gradient kernels are the batch's: the caller passes `weights` that are zero outside each scene's frame, so that
 *     outside pixels add nothing to the loss, the gradients or the Lipschitz constants (the model is zero there because
 *     the morphologies are; what a PSF's adjoint writes there is zeroed by the constraint kernels), and `images` that are
 *     zero there;
 *   - centres are in the scene's own pixel coordinates (= the padded plane's); one outside (h, w) is treated like one
 *     outside (H, W) of a uniform batch;
 *   - every _frames entry point that iterates, updates or initialises checks the entries on the device first: a scene
 *     whose entry lies outside 1..H x 1..W gets SCARLET_STATUS_BAD_FRAME and active = 0 and is not touched again; the
 *     other scenes go on.  No entry beyond the padded plane is ever used as a loop bound;
 *   - the workspace and the launch forms are those of the padded (H, W).  scarlet_fit_frames takes the one-launch
 *     iteration where the padded frame meets the four-wave kernel's conditions (K <= 4, H, W <= 64 with W % 4 == 0,
 *     H >= 3, no PSF, exact L; profile class 4): its ragged-frames instance walks each scene's own pixels only, for
 *     every B and with or without per-component switches.  No eight-wave or persistent kernel takes such a batch; every
 *     other one takes the general path, and none runs a box stage beyond 64 pixels;
 *   - SCARLET_E_NOTIMPL, found on the host before any launch: frame_hw with b->group; scarlet_init_sources_frames with
 *     spec->kind (extended sources only).  Point sources and multi-component sources (b->group) on ragged frames go
 *     through entry points of their own: scarlet_fit_frames_grouped, scarlet_source_update_frames_grouped and
 *     scarlet_init_sources_frames_mixed, below; update options on ragged frames (with or without
 *     b->group) through scarlet_fit_frames_options and scarlet_source_update_frames_options, below.  Priors and
 *     scarlet_fit_multi have no _frames form, and the
 *     joint fits take no group with frame_hw; the joint fit against
 *     same-grid observations has one (scarlet_fit_observations_frames, below), and so has the joint fit against
 *     low-resolution observations, each scene with its own operator (struct scarlet_lowres_frames,
 *     scarlet_fit_observations_frames_lowres, further below).  f == NULL is SCARLET_E_ARG. */
typedef struct scarlet_frames {
    const int32_t *frame_hw;    /* device [S][2] (h, w), or NULL = every scene is H x W */
} scarlet_frames;               /* 8 bytes */

/* scarlet_fit_constrained without a prior (c may be NULL: the batch's scalars) */
int scarlet_fit_frames(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */, int max_iter,
                       double e_rel, int approximate_L, int check_every, void *stream);
/* scarlet_source_update_constrained without a prior */
int scarlet_source_update_frames(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */,
                                 int in_iteration, void *stream);
/* the device check alone, for callers that run an iteration phase by phase: call it before scarlet_backward_step, whose
 * kernels skip the scenes it made inactive */
int scarlet_check_frames(scarlet_batch *b, const scarlet_frames *f, void *stream);
/* scarlet_init_extended / scarlet_init_sources on each scene's own frame: the detection coadd, the sdss symmetry's window,
 * the thresholded sweep and the centre-outside test use the scene's bounds; outside pixels are written as zero */
int scarlet_init_extended_frames(scarlet_batch *b, const scarlet_frames *f, const float *bg_rms_host, float thresh,
                                 const float *sed_scale_host, int init_symmetric, int init_monotonic, int run_update,
                                 void *stream);

/* Ragged frames with multi-component sources (b->group) and point sources.  The four calls above keep refusing frame_hw
 * with b->group, and scarlet_init_sources_frames keeps refusing spec->kind; these three take them.
 *   - scarlet_fit_frames_grouped / scarlet_source_update_frames_grouped follow the contract of scarlet_fit_frames /
 *     scarlet_source_update_frames, and b->group is allowed: the shared centre (and, every fifth iteration, the shift) of
 *     each source is measured on its scene's own frame -- the patch around the previous centre is clipped to h x w, so the
 *     centroid's radius is cut at the scene's own last row and column, as the reference cuts it for the scene alone --
 *     and the update kernels take that centre as given.  They are scarlet_fit_with / scarlet_source_update_with of the
 *     same members (scarlet_fit_request, below), so a NULL group or frame_hw gives the bits of the call without it.
 *     Groups never take a one-launch iteration: such a batch runs the general path.
 *   - scarlet_init_sources_frames_mixed is scarlet_init_sources on each scene's own frame, with spec->kind and b->group
 *     honoured: a point source's centre test and the clipping of the pasted model PSF are the own frame's; the layers of
 *     a multi-component source are cut from the extended start on the own frame, and their least-squares SEDs sum over
 *     the scene's pixels only.  Everything outside a frame is written as zero.  Bad scenes follow scarlet_init_sources
 *     (SCARLET_STATUS_BAD_INIT) and the device check of the frames (SCARLET_STATUS_BAD_FRAME).  With f->frame_hw == NULL
 *     it IS scarlet_init_sources.
 * f == NULL is SCARLET_E_ARG.  The products of such a batch do not depend on the groups: pass scarlet_batch_products_frames
 * a copy of the batch struct with group = NULL; there is no products entry point of its own. */
int scarlet_fit_frames_grouped(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */, int max_iter,
                               double e_rel, int approximate_L, int check_every, void *stream);
int scarlet_source_update_frames_grouped(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */,
                                         int in_iteration, void *stream);
/* (scarlet_init_sources_frames_mixed is declared beside scarlet_init_sources_frames, after struct scarlet_init_spec) */

/* Ragged frames, groups and update options together: a catalogue whose sources carry the stock update functions' options.
 * The contract of the two _grouped calls above with scarlet_update_options beside the constraints:
 *   - b->group is allowed.  f == NULL or o == NULL is SCARLET_E_ARG.  (scarlet_fit_with of the same members: a NULL
 *     frame_hw, group or member of `o` gives the bits of the call without it.)
 *   - A point or extended source runs the options pipeline on its scene's own bounds.  A multi-component source's shared
 *     centre (and, every fifth iteration, if it is symmetric, the centroid) is measured on the flux-weighted sum of its
 *     layers before any option acts; each layer then gets the symmetry (no shift: _KSPACE is soft with strength 1), the
 *     sweep, the positivity variant and the normalisation of its own row.
 *   - The device checks run first, in the order counts, frames, options: a scene may carry SCARLET_STATUS_BAD_FRAME and
 *     _BAD_OPTION together and is then never touched.  The constructors' update (in_iteration = 0) also leaves
 *     _BAD_INIT and _BAD_COUNT scenes untouched.
 *   - Pixels outside a scene's frame are no neighbour, partner, ring pixel or window pixel of any operator and are exactly
 *     0.0f in both morphology buffers after every call.
 *   - Such a batch takes the general path on one pipeline: no one-launch iteration, no box stage, the workspace and the
 *     dynamic LDS of the padded (H, W) forms.  There is no prior and no init entry point of its own: start the sources with
 *     run_update = 0 and call scarlet_source_update_frames_options with in_iteration = 0. */
int scarlet_fit_frames_options(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */,
                               const scarlet_update_options *o, int max_iter, double e_rel, int approximate_L,
                               int check_every, void *stream);
int scarlet_source_update_frames_options(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */,
                                         const scarlet_update_options *o, int in_iteration, void *stream);

/* scarlet_fit_observations_constrained for scenes with their own frames (c may be NULL: the state's scalars).  The state
 * may span up to SCARLET_MAX_CHANNELS channels: with state->B > 8 the call is scarlet_fit_observations_wide without a prior
 * and without low-resolution observations; an observation keeps B <= 8.  With f->frame_hw == NULL it IS
 * scarlet_fit_observations_constrained / _wide, bit for bit.  Otherwise the contract is that of scarlet_fit_frames, for
 * every observation: the caller passes `weights` and `images` in every obs[i] that are zero outside each scene's frame, and
 * state morphologies that are zero there.  The observations' kernels -- PSF planes, the contraction, the Gram and Lipschitz
 * passes -- are those of the padded frame and sum nothing outside; what a PSF's adjoint and the step write outside is zeroed
 * by the constraint kernels, which run on each scene's own frame (no box stage).  The entries are checked on the device
 * first (SCARLET_STATUS_BAD_FRAME, active = 0, the scene is left untouched).  Errors before any launch: those of
 * scarlet_fit_observations_constrained; f == NULL is SCARLET_E_ARG; frame_hw with state->group is SCARLET_E_NOTIMPL.  There
 * is no prior (it has no ragged-frames form) and no `lowres` array: scarlet_fit_observations_frames_lowres takes one. */
int scarlet_fit_observations_frames(scarlet_batch *state, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */,
                                    scarlet_batch *const *obs, const int32_t *band0, int n_obs, int max_iter, double e_rel,
                                    int approximate_L, int check_every, void *stream);

/* A LOW-RESOLUTION observation of the model frame (reference LowResObservation, observation.py:242-599): a second data
 * set with coarser pixels and its own PSFs, fitted jointly with the others.  For frames that are not rotated against
 * each other the reference's resample-and-convolve operator, restricted to the frequencies its sinc cut keeps, is
 *     out_c = Re( Vy . ( Dhat_c o (Uy . model_c . Ux^T) ) . Vx^T )        (o: elementwise product)
 * with five small complex matrices that the caller computes once per geometry (scarlet_amd/resampling.py) and passes as
 * device float32 (re, im) pairs.  The struct travels beside the observation's scarlet_batch; every pointer is device
 * memory owned by the caller.
 * Limit: the four factor matrices, the B band spectra [2][nfy][nfx] and one model plane with its projection stay in
 * LDS: about 4 (2 nfy H + 2 nfx W + 2 h nfy + 2 w nfx + 2 B nfy nfx + 4 nfy nfx + H (W + 2 nfx)) bytes (rows padded to
 * odd lengths) against 159 KiB.  With an 11-pixel model PSF and images of half the model's side: a 64 x 64 model frame
 * (72-point padded plane, nfy = 19, nfx = 37) with 32 x 32 images takes 133 KiB at B = 8 bands; 72 x 72 with 36 x 36
 * (75 x 80-point plane, nfy = 19, nfx = 41) still fits at B = 8 (156 KiB), 76 x 76 with 38 x 38 up to B = 6 (158 KiB),
 * 84 x 84 with 42 x 42 up to B = 2 (158 KiB); beyond: SCARLET_E_NOTIMPL from the LDS-resident entry points, the
 * streamed form from the *_large ones (below). */
typedef struct scarlet_lowres {
    int32_t h, w;               /* the observation's pixel grid: images and weights are [S][B][h][w]                */
    int32_t nfy, nfx;           /* retained frequencies per axis (rows of uy / ux)                                  */
    int32_t B;                  /* bands of the observation = of dhat = of its scarlet_batch                        */
    const float *uy;            /* [nfy][H][2]   model rows    -> frequencies (placement phase included)            */
    const float *ux;            /* [nfx][W][2]   model columns -> frequencies                                       */
    const float *vy;            /* [h][nfy][2], or [S][h][nfy][2] when v_per_scene: frequencies -> observed rows    */
    const float *vx;            /* [w][nfx][2], or [S][w][nfx][2] when v_per_scene                                  */
    const float *dhat;          /* [B][nfy][nfx][2], or [S][B][nfy][nfx][2] when dhat_per_scene: the difference
                                   kernels' spectra times (observed pixel / model pixel)^2                          */
    int32_t v_per_scene;        /* scenes cut at different sub-pixel phases carry their own vy / vx                 */
    int32_t dhat_per_scene;
    void *workspace;            /* scarlet_lowres_workspace_bytes() bytes: the gradient planes [S][B][H][W] and the
                                   per-plane losses [S][B] (float64); scratch of the fit, no need to zero it        */
} scarlet_lowres;               /* 80 bytes */

/* bytes of `lr->workspace` for this state (S, H, W) and observation batch (B); < 0: an error code */
int64_t scarlet_lowres_workspace_bytes(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr);

/* scarlet_fit_observations_constrained where some observations are low-resolution: `lowres` is an array of n_obs pointers,
 * NULL = that observation shares the model's grid and is handled exactly as before; with every entry NULL the call IS
 * scarlet_fit_observations_constrained.  A low-resolution obs[i] has H = lowres[i]->h, W = lowres[i]->w, B = lowres[i]->B,
 * images and weights [S][B][h][w], the state's S and K, and no diff_kernel (SCARLET_E_ARG).  Per iteration and scene one
 * workgroup (k_lowres_planes) projects every present component's morphology once, forms the band spectra from the
 * state's SEDs, renders, takes the weighted residual and its loss (float64 sums) and writes the adjoint as gradient
 * planes over the model frame; the contraction, both Lipschitz constants (n_obs x the eigenvalues as in the reference:
 * the operator's norm is not in them), the step, the constraint pipeline and the convergence test are those of
 * scarlet_fit_observations.  Ragged counts, per-component constraints, fix_sed / fix_morph and approximate_L work as
 * there.  Shapes, null factor pointers and the LDS limit are checked on the host before any launch. */
int scarlet_fit_observations_lowres(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs,
                                    const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs, int max_iter,
                                    double e_rel, int approximate_L, int check_every, void *stream);

/* LowResObservation.render and its adjoint for n planes (also what the tests compare with float64): plane p uses the
 * difference kernel of band[p] (device int32 [n], values in 0 .. lr->B - 1; NULL: band 0) and, with v_per_scene /
 * dhat_per_scene, the factors of scene[p] (device int32 [n]; NULL: scene 0).  render: model [n][H][W] -> out [n][h][w];
 * adjoint: resid [n][h][w] -> out [n][H][W].  lr->workspace is not used. */
int scarlet_lowres_render(const float *model, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                          const int32_t *scene, float *out, void *stream);
int scarlet_lowres_adjoint(const float *resid, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                           const int32_t *scene, float *out, void *stream);

/* The four entry points above are the LDS-RESIDENT form: they end where the factor matrices and one model plane leave
 * LDS (SCARLET_E_NOTIMPL).  The *_large entry points below take every shape those take and every larger one up to
 * SCARLET_MAX_SIDE a side.  Where the shape fits LDS (and the LOWRES_STREAMED switch is off) they launch the same
 * kernels, bit-identical to the calls above; beyond, the STREAMED form (csrc/lowres_stream.h): the same sandwich on the
 * same stacked real operands with the same k-ordered float32 sums as a chain of batched GEMMs over many planes at once
 * (k_lrs_gemm: v_mfma_f32_16x16x4_f32, operands staged through LDS in K-steps, grid = (output tiles, planes)), the
 * intermediates in a scratch area in HBM, planes taken in chunks that keep the scratch below 256 MiB.  A fit projects
 * the B band models sum_k sed[k][c] m_k instead of the K components, so its cost does not depend on K.
 *
 * bytes of `lr->workspace` for scarlet_fit_observations_lowres_large: the gradient planes, the per-plane losses and
 * ALWAYS the scratch of the streamed form (a switch changed between sizing and fitting cannot write past it); < 0: an
 * error code */
int64_t scarlet_lowres_large_workspace_bytes(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr);
/* scarlet_fit_observations_lowres without the LDS limit; every lowres[i]->workspace holds
 * scarlet_lowres_large_workspace_bytes().  Shapes, null pointers, B <= 8 and sides <= SCARLET_MAX_SIDE are checked on
 * the host before any launch. */
int scarlet_fit_observations_lowres_large(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs,
                                          const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs,
                                          int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
/* The joint fit with priors (Blend.fit calls backward_prior for every component however many observations the blend
 * has, blend.py:87-96): scarlet_fit_observations_lowres_large (c given) or its form without per-component switches
 * (c == NULL), with `lowres` NULL or an array of n_obs pointers as there, where every present component of an active
 * scene steps as scarlet_prior describes, L being the scene's constant times n_obs.  No pass is added: the contraction
 * that already reads the morphologies and holds their summed gradient reads the prior's planes where a component has
 * them (k_obs_contract<KS, true>: a weight of 0, no given plane or a fixed morphology reads none), k_obs_head steps the
 * SEDs with the prior's terms and writes p->L_comp, and the sparse_l0 / sparse_l1 cut uses each component's own step.
 * `lipschitz` and `mse` hold no prior.  All gradient paths (K <= 8, <= 32, <= 256; exact and approximate L) are covered.
 * p == NULL, a NULL L_comp or a target without its weight: SCARLET_E_ARG before any launch. */
int scarlet_fit_observations_prior(scarlet_batch *state, const scarlet_constraints *c /* or NULL */, const scarlet_prior *p,
                                   scarlet_batch *const *obs, const scarlet_lowres *const *lowres /* or NULL */,
                                   const int32_t *band0, int n_obs, int max_iter, double e_rel, int approximate_L,
                                   int check_every, void *stream);
/* The joint fit over a model frame of up to SCARLET_MAX_CHANNELS channels: surveys whose bands do not coincide (LSST
 * ugrizy + Euclid VIS/Y/J/H = 10 channels, with Roman's 7 filters 17) exceed the 8 channels of the entry points above.
 * The arguments are those of scarlet_fit_observations_prior, with c, p and lowres each allowed to be NULL.
 *   - state->B <= SCARLET_MAX_CHANNELS; every obs[o]->B <= 8 as before (an instrument with more bands of its own is
 *     split into two observations on the same grid); band0[o] + obs[o]->B <= state->B.  More channels:
 *     SCARLET_E_NOTIMPL.  A single-observation batch keeps B <= 8.
 *   - state->B <= 8: exactly the kernels of scarlet_fit_observations_prior (or _lowres_large / _constrained without a
 *     prior), the same bits.
 *   - state->B > 8: the observations' own chains are unchanged (they take the channel count as a stride); the
 *     contraction over the observations is k_obs_contract_wide (multiobs_wide.h), lambda_max of the SED Gram
 *     (n = min(K, C) <= 32) is k_wide_lmorph, and the morphology Gram comes from the Gram passes for every K.  No atomics:
 *     the loss and d loss / d sed partials are float64 sums in a fixed order, a repeated fit gives the same bits.
 *   - scarlet_batch_workspace_bytes() sizes the state's workspace for any B.  The helpers that check the state's shape
 *     have wide siblings below: the same functions with the state's channel limit at SCARLET_MAX_CHANNELS. */
int scarlet_fit_observations_wide(scarlet_batch *state, const scarlet_constraints *c /* or NULL */,
                                  const scarlet_prior *p /* or NULL */, scarlet_batch *const *obs,
                                  const scarlet_lowres *const *lowres /* or NULL */, const int32_t *band0, int n_obs,
                                  int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
int scarlet_init_combined_sed_wide(scarlet_batch *state, const float *images, int B, int band0, const float *obs_psf_peak,
                                   int peak_per_scene, const float *model_psf_max, void *stream);
int64_t scarlet_lowres_large_workspace_bytes_wide(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr);
/* diagnostics, host-only: the form of the contraction a joint fit of K components over C model channels takes
 * (launch_plan.h contract_plan): {kernel: 1 = k_obs_contract<8>, 2 = k_obs_contract<0>, 3 = k_obs_contract_wide;
 * channels the instance is built for; waves; threads per workgroup; dynamic LDS bytes; the LDS limit of the plans;
 * prior; 0}.  Returns 0, or -1 where there is no form (C > SCARLET_MAX_CHANNELS, K > SCARLET_MAX_COMPONENTS). */
int scarlet_debug_contract_plan(int K, int C, int prior, int32_t *out8);
/* diagnostics, host-only: the one-launch iteration a fit of `b` takes (launch_plan.h fused_plan) with the frames and the
 * constraints scarlet_fit_frames / scarlet_fit_constrained would be given (either may be NULL), under the options in
 * force: {kernel; threads per workgroup; dynamic LDS bytes; 1 = that fits the LDS limit; the LDS limit of the plans;
 * 1 = ragged frames (f->frame_hw given); 0; 0}.  kernel: 0 = none, the general path; 1, 2 = the four-wave kernel's
 * per-component instance for B <= 6, B <= 8; 3 = the persistent eight-wave kernel; 4, 5 = the eight-wave kernel's exact
 * and general instance; 6, 7 = the four-wave kernel for B <= 6, B <= 8; 8, 9 = its ragged-frames instance for B <= 6,
 * B <= 8.  Reads the structs' own fields only: no device call, no device pointer is dereferenced.  Returns 0, or -1 for
 * a NULL b or out8. */
int scarlet_debug_fused_plan(const scarlet_batch *b, const scarlet_frames *f /* or NULL */,
                             const scarlet_constraints *c /* or NULL */, int approximate_L, int n_iter, int32_t *out8);
/* bytes of device scratch scarlet_lowres_render_large / _adjoint_large need for n planes: 0 where the LDS form runs;
 * < 0: an error code */
int64_t scarlet_lowres_op_scratch_bytes(int n, int H, int W, const scarlet_lowres *lr);
/* scarlet_lowres_render / _adjoint without the LDS limit; `scratch` (device, scratch_bytes long; may be NULL when
 * scarlet_lowres_op_scratch_bytes() is 0).  A scratch that is too small is SCARLET_E_ARG before any launch. */
int scarlet_lowres_render_large(const float *model, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                                const int32_t *scene, float *out, void *scratch, int64_t scratch_bytes, void *stream);
int scarlet_lowres_adjoint_large(const float *resid, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                                 const int32_t *scene, float *out, void *scratch, int64_t scratch_bytes, void *stream);

/* Products of a batch's state: what the reference reads off a fitted Blend -- blend.get_model(), observation.render(model),
 * observation.get_loss(model), component.get_flux(), component.get_model() -- for every scene in one READ-ONLY call.
 * Every output pointer is device memory owned by the caller and may be NULL (at least one is not); only the outputs that
 * are given are computed.
 *   - Each scene is read from its own buffer cur[s].  Scenes with active == 0 or with status bits set are evaluated like
 *     the others: the products describe whatever state is there.  NaN in a scene's factors stays in that scene's outputs.
 *   - Absent components (n_components) add nothing; their rows of `flux` and `component_models` are written as zeros.
 *   - The call writes through `out` and `scratch` only.  Of b->workspace it reads the transformed difference kernel that
 *     scarlet_batch_prepare_psf left there (a batch with a diff_kernel and any of rendered / residual / loss wanted must
 *     have been prepared); sed, morph, cur, it, active, status, flags, mse and lipschitz are not touched.
 *   - loss and flux are float64 sums in a fixed order: two calls on the same state give the same bits.
 *   - `scratch`: scarlet_products_scratch_bytes() bytes of device memory, contents irrelevant before and after.  With a
 *     difference kernel and no `model` output the unconvolved planes are staged there, the scenes taken in chunks that
 *     keep the staged planes and the hipFFT chain's buffers within 256 MiB (one scene at the least).
 *   - The planes are convolved by the LDS-resident transform wherever scarlet_debug_psf_plan reports one for the batch,
 *     by the hipFFT chain of scarlet_convolve_same elsewhere (its plans come from the library's cache, as in a fit; a
 *     chunk with another number of planes than the batch creates its plan pair on first use).
 * Errors (SCARLET_E_ARG with a message, before anything is launched): b or out NULL, every output NULL, n_select < 0,
 * component_models without a selection (n_select == 0), a selected index outside 0 .. K - 1, images NULL with residual
 * or loss wanted, a scratch that is too small. */
typedef struct scarlet_products {
    float  *model;            /* [S][B][H][W]: sum_k sed[k][b] morph[k][p]  (ComponentTree.get_model, component.py:321-347) */
    float  *rendered;         /* [S][B][H][W]: model (*) diff_kernel; = model without one (Observation.render,
                                 observation.py:203-220)                                                                     */
    float  *residual;         /* [S][B][H][W]: images - rendered                                                            */
    double *loss;             /* [S][B]: 0.5 sum_p (w (rendered - image))^2 per band; its sum over b is Observation.get_loss
                                 (observation.py:222-239)                                                                    */
    double *flux;             /* [S][K][B]: morph[k].sum() * sed[k][b]  (Component.get_flux, component.py:172-175)            */
    const int32_t *components; /* HOST [n_select] component indices, the same for every scene; NULL: 0 .. n_select - 1        */
    int32_t n_select;
    float  *component_models; /* [S][n_select][B][H][W]: sed[k][b] morph[k][p]  (Component.get_model)                         */
} scarlet_products;           /* 64 bytes */

/* bytes of `scratch` for this batch and these outputs (which pointers of `out` are NULL decides, not their values);
   0 for NULL arguments or a batch whose shape the engine does not take */
int64_t scarlet_products_scratch_bytes(const scarlet_batch *b, const scarlet_products *out);
int scarlet_batch_products(const scarlet_batch *b, const scarlet_products *out, void *scratch, int64_t scratch_bytes,
                           void *stream);
/* scarlet_batch_products of a batch whose scenes have their own frames (scarlet_frames): model, rendered and residual are
 * exactly zero outside each scene's frame -- where a difference kernel's convolution spills, the kernels mask it -- and
 * those pixels add nothing to the loss.  The scratch is that of scarlet_batch_products. */
int scarlet_batch_products_frames(const scarlet_batch *b, const scarlet_frames *f, const scarlet_products *out, void *scratch,
                                  int64_t scratch_bytes, void *stream);
/* The same for a batch fitted against several observations (scarlet_fit_observations): observation i sees the channels
 * band0[i] .. band0[i] + obs[i]->B - 1 of the state's model through its own difference kernel, images and weights, and
 * out[i] takes its rendered / residual / loss ([S][obs[i]->B]...; model, flux and component_models must be NULL there).
 * state_out (or NULL) takes model, flux and component_models over the state's C = state->B channels; they need no
 * observation, and rendered / residual / loss must be NULL there.  An out[i] with every pointer NULL skips that
 * observation.  Every observation here lies on the model's grid; a batch with a low-resolution observation goes
 * through scarlet_observations_products_lowres (below), which renders that one too.
 * `scratch` is shared by the evaluations, which run one after the other: the largest of
 * scarlet_products_scratch_bytes(state, state_out) and scarlet_products_scratch_bytes(obs[i], &out[i]). */
int scarlet_observations_products(const scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                                  const scarlet_products *state_out, const scarlet_products *out, void *scratch,
                                  int64_t scratch_bytes, void *stream);
/* scarlet_observations_products where some observations are low-resolution (LowResObservation.render(blend.get_model()),
 * get_loss(model), reference observation.py:561-599): `lowres` is an array of n_obs pointers, NULL = that observation
 * shares the model's grid and is handled exactly as above; with every entry NULL the call IS
 * scarlet_observations_products.  A low-resolution obs[i] has H = lowres[i]->h, W = lowres[i]->w, B = lowres[i]->B, the
 * state's S and K and no diff_kernel; out[i].rendered and out[i].residual are [S][B][h][w], out[i].loss is [S][B]:
 *   - rendered = the operator of scarlet_lowres applied to channels band0[i] .. band0[i] + B - 1 of the model planes
 *     sum_k sed[k][c] morph[k] (the float32 FMA chain in k order that `model` holds): bit for bit what
 *     scarlet_lowres_render_large makes of those planes; residual = images - rendered; loss as in scarlet_products,
 *     float64 sums in a fixed order, no atomics.
 *   - Every scene is evaluated from its own buffer cur[s], whatever `active` and `status` say; absent components add
 *     nothing; a scene's NaN stays in its own outputs.
 *   - Read-only: the call writes through the outputs and `scratch` only.  lowres[i]->workspace is neither read nor
 *     written (it may be NULL), so a fit's gradient planes, losses and streamed scratch stay as they are, as does the state.
 *   - Where the factor matrices fit LDS (the limit of the LDS-resident entry points above) one workgroup per scene
 *     (k_lowres_products) forms each band's model in LDS, projects, renders and reads the result once; it needs no
 *     scratch.  Beyond, up to SCARLET_MAX_SIDE a side, and everywhere under the LOWRES_STREAMED switch, the streamed
 *     chain of GEMMs runs over the S B band planes in chunks that keep the scratch within 256 MiB (at least one plane;
 *     LOWRES_CHUNK lowers the chunk), on the band models of k_lrs_model -- or, when state_out->model is given, on that
 *     output -- with a finish that only reads the rendered planes.  NO_LOWRES_MFMA gives the same bits in both forms.
 *   - `scratch`: the largest of what scarlet_observations_products asks for the state and the same-grid observations
 *     and scarlet_lowres_products_scratch_bytes() of the low-resolution ones.
 * Errors (SCARLET_E_ARG with a message, before anything is launched): those of scarlet_observations_products; `lowres`
 * NULL; for a low-resolution observation shapes that do not fit the state or its scarlet_lowres, a null factor matrix,
 * B > 8, sides above SCARLET_MAX_SIDE, a diff_kernel, images NULL with residual or loss wanted, a scratch that is too
 * small. */
int scarlet_observations_products_lowres(const scarlet_batch *state, scarlet_batch *const *obs,
                                         const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs,
                                         const scarlet_products *state_out, const scarlet_products *out, void *scratch,
                                         int64_t scratch_bytes, void *stream);
/* bytes of `scratch` that the low-resolution observation `obs` needs there: 0 where the LDS form runs (and for an `out`
 * that is NULL or empty), otherwise a function of the shapes alone; < 0: an error code */
int64_t scarlet_lowres_products_scratch_bytes(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr,
                                              const scarlet_products *out);
/* scarlet_observations_products_lowres for a state of up to SCARLET_MAX_CHANNELS channels (`lowres` may be NULL).  The
 * state's model [S][C][H][W] and flux partials come from k_products in chunks of 8 channels, flux [S][K][C] and
 * component_models [S][n_select][C][H][W] from the kernels that take any channel count; flux stays a float64 sum in a
 * fixed order.  An observation keeps B <= 8.  The scratch sizes come from the _wide functions. */
int scarlet_observations_products_wide(const scarlet_batch *state, scarlet_batch *const *obs,
                                       const scarlet_lowres *const *lowres /* or NULL */, const int32_t *band0, int n_obs,
                                       const scarlet_products *state_out, const scarlet_products *out, void *scratch,
                                       int64_t scratch_bytes, void *stream);
int64_t scarlet_products_scratch_bytes_wide(const scarlet_batch *state, const scarlet_products *out);
int64_t scarlet_lowres_products_scratch_bytes_wide(const scarlet_batch *state, const scarlet_batch *obs,
                                                   const scarlet_lowres *lr, const scarlet_products *out);
/* scarlet_observations_products / _wide (state->B > 8) of a batch fitted by scarlet_fit_observations_frames: every
 * observation's rendered and residual are exactly zero outside each scene's frame (a difference kernel's spill is masked
 * in the kernels) and those pixels add nothing to its loss, as for scarlet_batch_products_frames; the state's model and
 * component_models are zero there because the morphologies are.  With f->frame_hw == NULL the call IS
 * scarlet_observations_products / _wide.  The scratch is theirs (scarlet_products_scratch_bytes / _wide).  f == NULL is
 * SCARLET_E_ARG, frame_hw with state->group SCARLET_E_NOTIMPL; there is no `lowres` array. */
int scarlet_observations_products_frames(const scarlet_batch *state, const scarlet_frames *f, scarlet_batch *const *obs,
                                         const int32_t *band0, int n_obs, const scarlet_products *state_out,
                                         const scarlet_products *out, void *scratch, int64_t scratch_bytes, void *stream);

/* LOW-RESOLUTION observations of scenes with their own frames.  The reference builds the operator from the scene's own
 * frame -- the periodic plane is fast_shape(max(frame, PSF) + 3), the frame sits at pad_start inside it, the shifts are
 * relative to the extent the observation's pixels span -- so a scene fitted on a padded frame is not the scene the
 * reference fits: every scene brings its own H_s, W_s, h_s, w_s, nfy_s, nfx_s and its own five factor matrices.  The
 * caller computes them per scene (scarlet_amd/resampling.py, float64) and ZERO-PADS every table to the per-dimension
 * maxima, which is exact: the padded rows and columns only add products with 0.  This struct travels beside the
 * observation's scarlet_lowres, which then holds the maxima in h, w, nfy, nfx (H, W are the state's), needs
 * v_per_scene = dhat_per_scene = 1 with vy [S][h][nfy][2], vx [S][w][nfx][2] and dhat [S][B][nfy][nfx][2] zero-padded
 * the same way, and whose own uy / ux are not read (they must not be NULL).  Images and weights are the padded
 * [S][B][h][w] blocks, zero outside each scene's own h_s x w_s. */
typedef struct scarlet_lowres_frames {
    const int32_t *dims;   /* device [S][6]: H_s, W_s, h_s, w_s, nfy_s, nfx_s                                  */
    const float *uy, *ux;  /* [S][nfy][H][2], [S][nfx][W][2]: each scene's own matrices, zero-padded to the     */
} scarlet_lowres_frames;   /* maxima that the accompanying scarlet_lowres holds in h, w, nfy, nfx (24 bytes)    */

/* scarlet_fit_observations_lowres_large / scarlet_fit_observations_wide without a prior (the state's channel count
 * decides; c may be NULL) for such scenes: `lowres` and `lowres_frames` are arrays of n_obs pointers, NULL = that
 * observation is on the model's grid / brings no tables of its own.  With every lowres_frames[i] NULL and f->frame_hw NULL
 * the call IS scarlet_fit_observations_lowres_large (or _wide), bit for bit.  Otherwise the contract is that of
 * scarlet_fit_observations_frames, and for a low-resolution observation:
 *   - the call is of the `large` kind: where the maxima fit LDS (the limit at scarlet_lowres, evaluated for the maxima,
 *     which may come from different scenes) one workgroup per scene (k_lowres_planes_frames) reads its row of `dims` and
 *     its own tables and runs every loop and GEMM over the scene's own sizes; it writes the gradient planes over the
 *     whole padded H x W, 0.0f outside the scene's frame, and sums the loss over the scene's own pixels.  Beyond, and
 *     under LOWRES_STREAMED, the streamed form runs on the padded extents of every scene (it streams the padding: the
 *     same sums plus products with 0);
 *   - workspace: scarlet_lowres_large_workspace_bytes() / _wide of the scarlet_lowres that holds the maxima;
 *   - the device check of scarlet_frames extends to `dims`: a row outside 1..max in any column, or whose H_s, W_s
 *     differ from frame_hw[s], gives the scene SCARLET_STATUS_BAD_FRAME and active = 0; it is not touched again, the
 *     others go on.  No entry is a loop bound before it has been tested against the padded blocks.
 * Errors before any launch: those of scarlet_fit_observations_lowres_large / _frames; SCARLET_E_ARG for f, `lowres` or
 * `lowres_frames` NULL, lowres_frames[i] without lowres[i] or without f->frame_hw, a null table, v_per_scene or
 * dhat_per_scene not set; SCARLET_E_NOTIMPL for f->frame_hw with a lowres[i] that has no lowres_frames[i], and for
 * frame_hw with state->group.  There is no prior argument.  Not covered: frames rotated against each other, and batches
 * whose observations are all low-resolution (nothing would carry the model frames). */
int scarlet_fit_observations_frames_lowres(scarlet_batch *state, const scarlet_frames *f, const scarlet_constraints *c /* or NULL */,
                                           scarlet_batch *const *obs, const scarlet_lowres *const *lowres,
                                           const scarlet_lowres_frames *const *lowres_frames, const int32_t *band0, int n_obs,
                                           int max_iter, double e_rel, int approximate_L, int check_every, void *stream);
/* scarlet_observations_products_lowres / _wide for such a batch: rendered and residual of a low-resolution observation
 * are written over the whole padded [S][B][h][w] block, 0.0f outside each scene's own h_s x w_s, and its loss runs over
 * the scene's own pixels; a scene whose `dims` row fails the test above gets zeros in all three (the call is read-only:
 * it marks nothing).  The same-grid observations and the state are evaluated as scarlet_observations_products_frames
 * does.  Scratch: scarlet_lowres_products_scratch_bytes() / _wide of the scarlet_lowres that holds the maxima, and the
 * others' as there.  Errors: those of scarlet_observations_products_lowres and the ones listed above. */
int scarlet_observations_products_frames_lowres(const scarlet_batch *state, const scarlet_frames *f, scarlet_batch *const *obs,
                                                const scarlet_lowres *const *lowres,
                                                const scarlet_lowres_frames *const *lowres_frames, const int32_t *band0,
                                                int n_obs, const scarlet_products *state_out, const scarlet_products *out,
                                                void *scratch, int64_t scratch_bytes, void *stream);

/* ---- A fit in one request.  Every scarlet_fit* and scarlet_source_update* function above is a fixed-shape form of the
 * two calls below: it fills this struct from its arguments and goes through the same check and the same body.
 * A request is accepted iff one of those named functions accepts the same members (the table is in DESIGN.md, 5i):
 *   n_obs = 0 (the batch's own images, at most 8 bands; lowres / lowres_frames must be NULL, SCARLET_E_ARG):
 *     constraints, b->n_components and b->group go with at most one of prior, options, frames->frame_hw -- except that
 *     options and frame_hw go together; a prior with frame_hw or with options is SCARLET_E_NOTIMPL;
 *   n_obs = 1..8 (the `large` kind throughout; up to SCARLET_MAX_CHANNELS model channels):
 *     a prior goes with constraints, lowres, more than 8 channels and b->group, not with frame_hw (E_NOTIMPL);
 *     options go with constraints and b->n_components alone: with a prior, frame_hw, lowres, more than 8 channels or
 *     b->group they are E_NOTIMPL;  frame_hw with b->group is E_NOTIMPL;  frame_hw with a lowres[i] needs its
 *     lowres_frames[i], and lowres_frames[i] needs frame_hw and lowres[i] (scarlet_fit_observations_frames_lowres).
 * `options` counts as given when the pointer is not NULL, `frames` when frame_hw is not NULL, `lowres` and
 * `lowres_frames` when the list is not NULL. */
typedef struct scarlet_fit_request {
    const scarlet_constraints *constraints;              /* NULL or all-NULL members: the batch's scalars     */
    const scarlet_prior *prior;                          /* NULL: none                                        */
    const scarlet_update_options *options;               /* NULL: the stock pipeline                          */
    const scarlet_frames *frames;                        /* NULL or frame_hw = NULL: uniform frames           */
    scarlet_batch *const *obs;                           /* n_obs observation batches, and ...                */
    const int32_t *band0;                                /* ... the first model channel of each               */
    const scarlet_lowres *const *lowres;                 /* NULL, or n_obs pointers (NULL = on the model grid) */
    const scarlet_lowres_frames *const *lowres_frames;   /* NULL, or n_obs pointers (NULL = no own tables)    */
    int32_t n_obs;                                       /* 0: the batch's own images                         */
    int32_t max_iter;
    double e_rel;
    int32_t approximate_L, check_every;
} scarlet_fit_request;          /* 88 bytes */
/* the host-side check of scarlet_fit_with alone: launches nothing, reads no device memory */
int scarlet_fit_request_check(const scarlet_batch *b, const scarlet_fit_request *r);
int scarlet_fit_with(scarlet_batch *b, const scarlet_fit_request *r, void *stream);
/* reads only constraints, prior (its L_comp), options and frames of the request; everything else is ignored */
int scarlet_source_update_with(scarlet_batch *b, const scarlet_fit_request *r, int in_iteration, void *stream);

/* Single phases, exposed for tests and for Python-overridden update() methods:        */
/* _backward + _set_lipschitz + gradient step (blend.py:81-96): reads buffer cur, writes
 * the stepped factors into buffer 1-cur; cur/it are NOT advanced yet                   */
int scarlet_backward_step(scarlet_batch *b, int approximate_L, void *stream);

/* As scarlet_backward_step, but buffer 1-cur receives the GRADIENTS of the loss -- d loss/d sed
   [S][K][B] and d loss/d morph [S][K][H*W] (Blend._backward, blend.py:105-118) -- instead of the
   stepped factors; `lipschitz` and `mse` are written as usual, fix_sed / fix_morph are not applied.
   For callers that combine gradients themselves: several observations per blend (blend.py:136-137,
   219-220) and Prior hooks. */
int scarlet_backward_gradients(scarlet_batch *b, int approximate_L, void *stream);
/* the built-in constraint pipeline (source.py:402-440).  in_iteration=1: on buffer 1-cur
 * (between backward_step and check_convergence); 0: on buffer cur with it=0 semantics,
 * as the source constructors do (source.py:400,492)                                    */
int scarlet_source_update(scarlet_batch *b, int in_iteration, void *stream);
/* _check_convergence (blend.py:141-184) on buffer 1-cur vs cur, then closes the
 * iteration: it += 1, cur flips, active cleared for converged scenes                   */
int scarlet_check_convergence(scarlet_batch *b, double e_rel, void *stream);

/* diagnostics (STAMPS switch on): byte offset inside b->workspace of the convolution kernel's phase stamps
 * ([S][B][32] int64 shader-clock values, written by every k_psf_conv launch), or -1 */
int64_t scarlet_debug_psf_stamps_offset(const scarlet_batch *b);
/* diagnostics: plan of the LDS-resident convolution (fftconv.h) for this batch: {H, W, Fy, Fx, M, RS, R1y, R2y, R1x, R2x,
 * oky, okx, image staged in LDS, exact-shape instance, LDS bytes, 0}; 0, or -1 when the batch takes another path.
 * Host-only: no device call. */
int scarlet_debug_psf_plan(const scarlet_batch *b, int32_t *out16);
/* Per-kernel timing of scarlet_fit with hipEvents recorded on the launch stream (used by
 * bench.py for the roofline line).  begin: allocate events for up to max_iterations
 * iterations and start recording; end: synchronise, return per kernel class
 * {0 k_grad, 1 k_step, 2 k_source_update, 3 k_converge, 4 k_iterate (fused), 5 the PSF convolution chain, 6 k_prior_step, 7 unused}
 * the summed milliseconds and launch counts, and stop recording. */
int scarlet_profile_begin(int max_iterations);
int scarlet_profile_end(double total_ms[8], int64_t launches[8]);
/* the same with both counts: `iterations` = iterations covered by the class's launches (what
 * scarlet_profile_end reports as `launches`: a k_fit2x launch covers several), `launches` = kernel
 * launches actually recorded.  Either array may be NULL. */
int scarlet_profile_end_ex(double total_ms[8], int64_t iterations[8], int64_t launches[8]);

/* ExtendedSource initialisation on device (source.py:139-180, rank f1 of SURVEY 8f):
 * per component: pixel SED (optionally PSF-corrected by the caller through sed_scale
 * [B] or NULL), detection coadd, sdss symmetry, thresh=0.1 weighted monotone sweep,
 * cut at bg_cutoff, divide by the centre pixel.  Writes sed/morph of buffer b->cur,
 * flags (NO_VALID_PIXELS when nothing is above the cut), then runs the constraint
 * pipeline once with it=0 as the constructor does (source.py:492) when run_update != 0.
 * init_symmetric / init_monotonic: the `symmetric` / `monotonic` arguments of
 * init_extended_source (ExtendedSource always passes symmetric=True).  bg_rms: host [B]. */
int scarlet_init_extended(scarlet_batch *b, const float *bg_rms_host, float thresh,
                          const float *sed_scale_host, int init_symmetric, int init_monotonic,
                          int run_update, void *stream);

/* Initialisation of a batch of mixed sources, all inputs on the device (initsrc.h).  Per component:
 *   - group[s][k] >= 0: a layer of MultiComponentSource g (init_multicomponent_source, source.py:242-295).  The n
 *     members of a group (1 <= n <= SCARLET_MAX_LAYERS) start from the extended initialisation at the centre of the
 *     first member (symmetric = b->symmetric); member j >= 1 starts at flux_percentiles[s][k + j] * max / 100
 *     (ascending, inside (0, 100); NULL: 25), each layer is divided by its own max, and the SEDs are the
 *     least-squares fit (M M^T)^-1 M D^T to the scene's images (float64 sums and solve, source.py:74-98);
 *   - kind[s][k] == SCARLET_INIT_POINT: PointSource -- the model PSF pasted with its centre on the pixel and clipped
 *     to the frame (a single 1 without model_psf); SED = pixel / obs PSF peak;
 *   - otherwise ExtendedSource, what scarlet_init_extended does with the scene's own bg_rms row and
 *     sed = pixel / obs PSF peak x max(model PSF) (get_psf_sed, source.py:41-71).
 * Absent components (n_components) are not touched; a centre outside the frame gives an empty component and
 * SCARLET_STATUS_CENTER_AT_EDGE; nothing above the cut gives FLAG_NO_VALID_PIXELS (every member of a group).
 * run_update != 0: the constructors' update() once with it = 0 (the group pipeline for groups).
 * A scene with bad input -- bg_rms <= 0 in a band, a group of more than SCARLET_MAX_LAYERS members, percentiles
 * not ascending or outside (0, 100), an unknown kind -- gets SCARLET_STATUS_BAD_INIT and active = 0 and is left
 * untouched; the bit is cleared on the other scenes.  A layer whose max is <= 0 (the reference divides by zero)
 * or a singular normal matrix is found only while the group is layered: that scene gets BAD_INIT and active = 0
 * too, its other components keep their new start and the update does not run on it.
 * Needs no workspace; allocates a temporary [S] int buffer (and the float64 tiles of frames beyond LDS) and
 * returns after the stream has finished the work. */
typedef struct scarlet_init_spec {
    const float   *bg_rms;               /* device [B], or [S][B] when bg_rms_per_scene                     */
    int32_t        bg_rms_per_scene;
    const float   *obs_psf_peak;         /* device [B] / [S][B]: max of each observed PSF band, or NULL      */
    int32_t        obs_psf_peak_per_scene;
    const float   *model_psf;            /* device [P][P], P odd: the model frame's PSF, or NULL             */
    int32_t        model_psf_P;
    const int32_t *kind;                 /* device [S][K] SCARLET_INIT_*, or NULL = all EXTENDED;
                                            ignored where group[s][k] >= 0                                   */
    const float   *flux_percentiles;     /* device [S][K]: at member j >= 1 of a group, the percentile of
                                            boundary j, ascending; NULL = 25 (groups of 2)                   */
    float          thresh;
    int32_t        init_symmetric, init_monotonic, run_update;
} scarlet_init_spec;

int scarlet_init_sources(scarlet_batch *b, const scarlet_init_spec *spec, void *stream);
/* ... on each scene's own frame (scarlet_frames): extended sources only, spec->kind must be NULL */
int scarlet_init_sources_frames(scarlet_batch *b, const scarlet_frames *f, const scarlet_init_spec *spec, void *stream);
/* ... every stock source type on each scene's own frame: spec->kind and b->group are honoured (see "Ragged frames with
 * multi-component sources" above); with f->frame_hw == NULL it IS scarlet_init_sources */
int scarlet_init_sources_frames_mixed(scarlet_batch *b, const scarlet_frames *f, const scarlet_init_spec *spec, void *stream);

/* Row a3b set-up: FFT the difference kernel into the workspace (K-hat at the reference's FFT
 * shape next_fast_len(N + P + 3), fft.py:68-106) and create the batched hipFFT plans (cached
 * per shape inside the library; the only allocation the library makes). */
int scarlet_batch_prepare_psf(scarlet_batch *b, void *stream);

/* Observation.render / fft.convolve (observation.py:198-220, fft.py:304-317) for n planes:
 * out[p] = crop(model[p] (*) kernel[p or 0]) with the reference's pad / shift / crop
 * conventions.  model, out: device [n][H][W]; kernel: device [nk][Py][Px] with nk == n or 1.
 * Allocates temporary FFT buffers (set-up / test helper, not on the iteration path). */
int scarlet_convolve_same(const float *model, int n, int H, int W, const float *kernel, int nk,
                          int Py, int Px, float *out, void *stream);

/* Convergence sums (blend.py:159-171) of buffer 1-cur vs cur for every component, for
 * callers that ran their own update() between scarlet_backward_step and
 * scarlet_check_convergence (scarlet_source_update computes them itself). */
int scarlet_convergence_sums(scarlet_batch *b, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SCARLET_HIP_H */

/* pnp_hip.h -- C ABI of the MI355X (gfx950) PnP-SVRG/SAGA/SARAH hot path.
 *
 * The reference (vmonardo/pnp-svrg @ v1) is pure Python: it has no FFI of its own.  Its
 * boundary for this path is the duck-typed protocol of its algorithms/, problems/ and
 * denoisers/ packages.  This header is the native side a maintainer binds with
 * ctypes (INTEGRATION.md shows the stub); each entry point names the reference code it
 * replaces.
 *
 * Conventions
 *  - every data pointer is a DEVICE pointer (HBM); `stream` is a hipStream_t passed as void*;
 *  - nothing here allocates, frees or synchronises inside a hot call: plans own their
 *    workspaces (created/destroyed explicitly), so every call may be captured in a hipGraph;
 *  - `dtype`: PNP_F32 (production) or PNP_F64 (parity/debug); complex = interleaved (re,im);
 *  - images are row-major [B][H][W]; B independent problems ("batch") per call;
 *  - return 0 on success, nonzero on error; text via pnp_last_error() (thread-local).
 */
#ifndef PNP_HIP_H
#define PNP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PNP_F32 = 0, PNP_F64 = 1 };
enum { PNP_OK = 0, PNP_ERR_ARG = 1, PNP_ERR_HIP = 2, PNP_ERR_UNSUPPORTED = 3 };

int pnp_version(void);
const char* pnp_last_error(void);

/* ------------------------------------------------------------------ CSMRI masked FFT
 * Replaces problems/CSMRI.py:76-81 (grad_full) and :83-89 (grad_stoch), i.e.
 *   g = Re ifft2( sel o fft2(a - b) - sel o Y )
 * computed with real FFTs on the Hermitian-symmetrised k-space residual.            */
typedef struct pnp_csmri_plan pnp_csmri_plan;

/* H == W in {64, 128, 256}.  The plan owns a [batch][W/2][H] complex workspace + twiddles. */
int pnp_csmri_plan_create(pnp_csmri_plan** plan, int H, int W, int batch, int dtype);
int pnp_csmri_plan_destroy(pnp_csmri_plan* plan);

/* Selector (sampling mask, or mask o minibatch) from flat row-major k-space indices, as
 * np.flatnonzero(mask) / problems/CSMRI.py:66-74 produce them.  idx: [batch][n] int32,
 * selT: [batch][W][H] uint8 (TRANSPOSED: the column pass reads along ky).              */
int pnp_csmri_sel_from_indices(pnp_csmri_plan* plan, const int32_t* idx, int n, uint8_t* selT, void* stream);
/* Bit-packed form of a transposed selector: bitsT [batch][W][H/32] uint32, bit (ky & 31) of word [kx][ky >> 5].
 * The sampling mask is kept in this form (8 KiB per 256 x 256 problem instead of 64 KiB).               */
int pnp_csmri_pack_mask(pnp_csmri_plan* plan, const uint8_t* selT, uint32_t* bitsT, void* stream);

/* Device-side minibatch draw (problems/CSMRI.py:66-74 semantics: `mb` of the problem's sampled locations, uniform
 * without replacement; problems of one batch may have different numbers of sampled locations).  Every sampled
 * location i (flat row-major k-space index, as np.flatnonzero(mask) counts) gets a 32-bit key
 *     state = mix64(mix64(mix64(seed) + step) + problem)                       (mix64 = splitmix64 finaliser)
 *     x = lo32(state) ^ i;  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     key(i) = x ^ hi32(state)
 * and the mb smallest (key, i) pairs win.  Outputs, for steps step0 .. step0 + nsteps - 1 (a whole outer iteration in
 * one launch):
 *   mbd     [nsteps][batch] descriptors {uint64 state; uint32 T; uint32 P} (16 bytes): i is in the minibatch iff
 *           key(i) < T or (key(i) == T and i <= P);
 *   selbits [nsteps][batch][W][H/32] uint32 (may be NULL): mask o minibatch in the bit-packed layout of bitsT, which
 *           pnp_csmri_grad_sel takes as its selector -- 8 KiB per 256 x 256 problem-step instead of a 64 KiB byte
 *           selector.
 * Deterministic in (seed, step); NOT NumPy's legacy stream (reference-identical draws come from the host).
 * step_dev (may be NULL): device-resident counter added to `step0`, so the call can be replayed from a hipGraph.
 * mb >= the number of sampled locations selects them all.                                                */
int pnp_csmri_draw_thresholds(pnp_csmri_plan* plan, const uint32_t* bitsT, int mb, uint64_t seed, uint32_t step0,
                              int nsteps, const uint32_t* step_dev, void* mbd, uint32_t* selbits, void* stream);
/* mask o minibatch of ONE step as an explicit transposed selector (mbd: [batch] descriptors of that step).   */
int pnp_csmri_sel_from_thresholds(pnp_csmri_plan* plan, const uint32_t* bitsT, const void* mbd, uint8_t* selT,
                                  void* stream);
/* pnp_csmri_draw_thresholds for one step followed by pnp_csmri_sel_from_thresholds (plan-owned descriptors).   */
int pnp_csmri_draw_minibatch(pnp_csmri_plan* plan, const uint32_t* bitsT, int mb, uint64_t seed, uint32_t step,
                             const uint32_t* step_dev, uint8_t* selT, void* stream);
/* Same, from a dense row-major 0/1 indicator [batch][H][W] (uint8).                      */
int pnp_csmri_sel_from_dense(pnp_csmri_plan* plan, const uint8_t* sel, uint8_t* selT, void* stream);

/* Data term for a selector: yh = Hermitian part of (sel o Y) in the packed transposed
 * half-spectrum layout [batch][W/2][H] complex (column 0 carries kx=0 and kx=W/2).
 * YT: [batch][W][H] complex = Y transposed (measurements, CSMRI.py:32-33).               */
int pnp_csmri_pack_y(pnp_csmri_plan* plan, const void* YT, const uint8_t* selT, void* yh, void* stream);

/* A batch of problems GENERATED on the device (problems/CSMRI.py:12-59 per problem: Bernoulli mask :43-45, Y0 = mask o fft2(x)
 * :27,53-59, real noise on the support :32-33, Xinit = minmax |ifft2 Y| :35-36) from a counter-based stream, published here so
 * that a caller can restate it.  For an item with 64-bit `seed` and `id`, and a sub-stream tag k (mix64 and the per-position key
 * exactly as in the minibatch draw above):
 *     state_k = mix64(mix64(mix64(seed) + id) + k)
 *     key_k(i) = key(state_k, i)              i = flat row-major k-space index ky*W + kx (np.flatnonzero order)
 *   mask  (k = 0)   : position i is sampled iff (uint64)key_0(i) < T, T = floor(alpha * 2^32) clipped to [0, 2^32] (computed by
 *                     the caller in float64; T = 2^32 samples every position) -- Bernoulli per entry, so M0 differs per item;
 *   data            : Y0 = mask o fft2(x);  sigma = sqrt(||Y0||_2 * snr_fac / H / W), snr_fac = 10^(-snr/10)  (problem.py:58-61:
 *                     the norm, not its square); the sum of squares is taken in double in a fixed order;
 *   noise (k = 1, 2): u1 = (key_1(i) + 1) * 2^-32 in (0, 1], u2 = key_2(i) * 2^-32 in [0, 1), n(i) = sqrt(-2 ln u1) * cos(2 pi u2)
 *                     (Box-Muller in double for both plan dtypes), Y = Y0 + mask * sigma * n, into the REAL part only.  The 32-bit
 *                     uniforms end the tails at sqrt(-2 ln 2^-32) = 6.66 sigma.  An f32 and an f64 plan hold the same problem up to
 *                     the final rounding;
 *   init            : Xinit = minmax(|ifft2(Y)|) (Y is not Hermitian: both the real and the imaginary part of the inverse count).
 * Inputs: images [n_images][H][W] (`dtype`, already normalised to [0, 1]); per item [batch] device arrays image_idx (int32, in
 * [0, n_images)), thresh (uint64 T), snr_fac (double), seed, id (uint64).  Outputs, in the layouts the gradient calls read:
 * xrec [batch][H][W]; bitsT [batch][W][H/32]; maskT [batch][W][H] uint8 (may be NULL); YT [batch][W][H] complex; yh_full = the packed
 * half spectrum pnp_csmri_pack_y makes from this YT and maskT, bit for bit; xinit [batch][H][W]; M0 [batch] int32; inv_m0 [batch]
 * (`dtype`); sigma [batch] double.  Uses the plan's workspace; no allocation, no synchronisation.  An item's outputs do not
 * depend on the batch size or on its index in the batch (fixed-order reductions, no atomics).                                 */
int pnp_csmri_generate(pnp_csmri_plan* plan, const void* images, int n_images, const int32_t* image_idx, const uint64_t* thresh,
                       const double* snr_fac, const uint64_t* seed, const uint64_t* id, void* xrec, uint32_t* bitsT,
                       uint8_t* maskT, void* YT, void* yh_full, void* xinit, int32_t* M0, void* inv_m0, double* sigma,
                       void* stream);

/* out = alpha * Re ifft2( sel o fft2(a - b) - sel o Y ) + beta * c1 + gamma * c2
 *   b, yh, c1, c2 may be NULL (treated as zero).  out may alias a, c1 or c2.
 *   grad_full(z)            : a=z, sel=mask,   yh=pack(mask),    alpha=1/M0
 *   SVRG correction + step  : a=z, b=w, sel=mask o mb, yh=NULL, alpha=-lr/mb, beta=1 (c1=z),
 *                             gamma=-lr (c2=mu), out=z       (pnp_svrg.py:53,57) */
int pnp_csmri_grad(pnp_csmri_plan* plan, const void* a, const void* b, const uint8_t* selT,
                   const void* yh, double alpha, double beta, const void* c1,
                   double gamma, const void* c2, void* out, void* stream);

/* The same gradient with the other selector form and a per-problem scale.  Exactly one of
 *   selT  != NULL     explicit transposed uint8 selector (as pnp_csmri_grad)
 *   bitsT != NULL     bit-packed transposed selector [batch][W][H/32]: the sampling mask itself (grad_full), or one
 *                     step's row of pnp_csmri_draw_thresholds' selbits (mask o device-drawn minibatch)
 * Data term: yh (packed for exactly this selector, pnp_csmri_pack_y) or YT ([batch][W][H] complex = Y transposed:
 * the selector's data term is then formed inside the column pass, which is what a minibatch selector that exists
 * drawn on the device needs -- grad_stoch of pnp_sgd.py:33 / pnp_saga.py:45); at most one of the two.
 * alpha_vec (may be NULL): [batch] values of `dtype`; problem b uses alpha * alpha_vec[b] -- the 1/M0 of
 * problems/CSMRI.py:81 when the masks of a batch have different counts (Bernoulli masks, CSMRI.py:43-45).    */
int pnp_csmri_grad_sel(pnp_csmri_plan* plan, const void* a, const void* b, const uint8_t* selT, const uint32_t* bitsT,
                       const void* yh, const void* YT, double alpha, const void* alpha_vec, double beta,
                       const void* c1, double gamma, const void* c2, void* out, void* stream);

/* One WHOLE inner iteration of pnp_svrg with the TV prox (algorithms/pnp_svrg.py:52-80: minibatch SVRG direction, step,
 * estimate_sigma, TVDenoiser.denoise, Problem.PSNR) in one kernel, one workgroup per problem, the image register-
 * resident from the first load to the last store (f32 plans of 256 x 256):
 *     out = prox_TV( alpha * alpha_vec[b] * Re ifft2( sel o fft2(a - b) ) + beta * c1 + gamma * c2 )
 * bitsT: bit-packed selector as in pnp_csmri_grad_sel (one step's row of pnp_csmri_draw_thresholds' selbits; no data
 * term: the Y terms of the SVRG difference cancel).  sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out as in
 * pnp_prox_tv (the noise estimate is always made in-kernel).  denoise == 0: stop after the noise estimate and store the
 * stepped image (for a prox that is not this one).  out may alias a, c1 or c2.
 * `int denoise` has three values here and in pnp_csmri_svrg_outer_step, pnp_csmri_sarah_step, pnp_csmri_grad_step,
 * pnp_csmri_saga_step and their _pp forms: 0 = store the stepped image; 1 (any value but 0 and 2) = the per-column prox of
 * pnp_prox_tv; 2 = the two-dimensional wavelet prox of pnp_prox_wavelet2d (TVDenoiser(multi=False)) inside the kernel, on the
 * register-resident image: the same 2 x 2 Haar operations in the same order, so the coefficients are those of pnp_prox_wavelet2d
 * bit for bit; the 15 sub-band sums of squares are taken in another order (lane, wave tree, waves 0..7), so the thresholds and
 * the result agree with it to a few ulps, and exactly where every sum is exact.  A problem's result does not depend on the batch.
 * The multi-step forms that carry the argument (pnp_csmri_grad_span, pnp_csmri_saga_span, pnp_csmri_saga_step_hist_pp,
 * pnp_csmri_saga_span_hist) hold the per-column prox only: denoise == 2 is PNP_ERR_ARG there.                        */
int pnp_csmri_svrg_step(pnp_csmri_plan* plan, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                        const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2, void* out,
                        int denoise, double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_out,
                        void* sigma_out, void* stream);

/* The outer-loop refresh of the SVRG loop -- algorithms/pnp_svrg.py:32-38: mu = grad_full(z); w = copy(z) -- folded into the first
 * inner iteration of that outer iteration (:52-80 at j = 0).  There w == z, so the minibatch difference
 * grad_stoch(z, mb) - grad_stoch(w, mb) is exactly zero whatever the minibatch and the iteration is z <- prox(z - lr * mu):
 *     mu_out = alpha_vec[b] * Re ifft2( mask o fft2(z) - Y on the mask )         (= problems/CSMRI.py:76-81, yh packed by
 *                                                                                  pnp_csmri_pack_y for mask_bitsT's mask)
 *     w_out  = z
 *     out    = prox_TV( z + (-lr) * mu_out )              [+ noise estimate, PSNR error: as pnp_csmri_svrg_step]
 * in ONE kernel -- bit for bit what pnp_csmri_grad_sel (bits form, batch >= 192) + a copy + pnp_csmri_svrg_step(a = z,
 * b = w, c1 = z, c2 = mu, beta = 1, gamma = -lr) produce, without the second transform pair and the copy.  w_out and mu_out
 * must not alias z, out or each other; out may alias z.                                                      */
int pnp_csmri_svrg_outer_step(pnp_csmri_plan* plan, const void* z, const uint32_t* mask_bitsT, const void* yh,
                              const void* alpha_vec, double lr, void* w_out, void* mu_out, void* out, int denoise,
                              double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_out,
                              void* sigma_out, void* stream);

/* One whole inner iteration of the SARAH loop -- algorithms/pnp_sarah.py:72-104: the recursive direction, step, estimate_sigma,
 * TVDenoiser.denoise, Problem.PSNR, w_prev = z -- in one kernel -- the SARAH form of pnp_csmri_svrg_step (f32 plans of 256 x 256):
 *     v_out = alpha * alpha_vec[b] * Re ifft2( sel o fft2(a - b) ) + beta * c1        (a = w_next, b = w_prev, c1 = v_prev, beta = 1)
 *     out   = prox_TV( c2 + gamma * v_out )                                          (c2 = z, gamma = -lr)
 *     out2  = out                                                                    (nullable; w_prev)
 * v_out is recursion state: it is stored before c2 is folded in, and equals, bit for bit, what pnp_csmri_grad_sel (bits form,
 * one-kernel route) gives for the same a, b, alpha, beta, c1; the step is one fused multiply-add per element.  No data term:
 * grad_stoch is affine, the Y terms of the difference cancel.  bitsT, alpha_vec, sigma_modifier, fallback_sigma, xrec, sse_out,
 * sigma_out as in pnp_csmri_svrg_step.  denoise == 0: stop after the noise estimate and store c2 + gamma * v_out (for a prox that is
 * not this one); out2 must then be NULL.
 * Aliasing: v_out may alias c1, out may alias c2, out2 may alias b (the engine's in-place form: v, z and w_prev each updated where
 * they lie).  v_out must not alias a, b, c2, out or out2.
 * PNP_ERR_ARG before any device work: a NULL plan, a, b, bitsT, c1, c2, v_out or out; sse_out without xrec; out2 with
 * denoise == 0; a plan that is not f32 256 x 256; v_out aliasing anything but c1.                                  */
int pnp_csmri_sarah_step(pnp_csmri_plan* plan, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                         const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2, void* v_out,
                         void* out, void* out2, int denoise, double sigma_modifier, double fallback_sigma, const void* xrec,
                         double* sse_out, void* sigma_out, void* stream);

/* One whole inner iteration of the GD or the SGD loop -- algorithms/pnp_gd.py:24-70, pnp_sgd.py:24-70: gradient with its data
 * term, step, estimate_sigma, TVDenoiser.denoise, Problem.PSNR -- in one kernel (f32 plans of 256 x 256):
 *     out = prox_TV( alpha * alpha_vec[b] * Re ifft2( sel o fft2(a) - sel o Y ) + beta * c1 )          (a = c1 = z, beta = 1)
 * Exactly one of yh and YT carries the data term.  yh (packed by pnp_csmri_pack_y for the selector bitsT, i.e. for the sampling
 * mask) with bitsT = the mask is the GD step; YT ([batch][W][H] complex f32, Y transposed, as pnp_csmri_grad_sel takes it) with
 * bitsT = one slot of the drawn selbits is the SGD step: the data term of THAT selector is formed inside the kernel's column
 * phase, as the streaming column kernel forms it.  out may alias a and c1.  denoise, sigma_modifier, fallback_sigma, xrec,
 * sse_out, sigma_out as in pnp_csmri_svrg_step.
 * PNP_ERR_ARG before any device work: a NULL plan, a, bitsT, c1 or out; both or neither of yh and YT; sse_out without xrec; a
 * plan that is not f32 256 x 256.                                                                                  */
int pnp_csmri_grad_step(pnp_csmri_plan* plan, const void* a, const uint32_t* bitsT, const void* yh, const void* YT, double alpha,
                        const void* alpha_vec, double beta, const void* c1, void* out, int denoise, double sigma_modifier,
                        double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out, void* stream);

/* One whole inner iteration of the SAGA loop -- algorithms/pnp_saga.py:43-79 -- in one kernel (f32 plans of 256 x 256):
 *     g    = alpha * alpha_vec[b] * Re ifft2( sel o fft2(z) - sel o Y )                  (alpha = 1 / mb, data term from YT)
 *     old  = table[row[b]][b];  pv = table[prev_row[b]][b]
 *     s    = sum + g - old
 *     out  = prox_TV( z - lr * ((g - pv) + s * inv_hist) )
 *     table[row[b]][b] = g;  sum = s
 * Per element the statements and their order are pnp_saga_table_update's.  table: [hist][batch][H][W] f32; row, prev_row: int32
 * [batch] device vectors with entries in [0, hist) (as in pnp_saga_table_update_pp; the kernel cannot check them);
 * row[b] == prev_row[b] is legal (old and pv are loaded before anything is stored); sum: [batch][H][W].  out may alias z.
 * denoise == 0 stores the stepped image for a prox that is not this one.
 * PNP_ERR_ARG before any device work: a NULL plan, z, bitsT, YT, table, row, prev_row, sum or out; hist < 1; sse_out without
 * xrec; a plan that is not f32 256 x 256; table or sum overlapping z, out, xrec or each other.                        */
int pnp_csmri_saga_step(pnp_csmri_plan* plan, const void* z, const uint32_t* bitsT, const void* YT, double alpha,
                        const void* alpha_vec, void* table, const int32_t* row, const int32_t* prev_row, void* sum, double lr,
                        double inv_hist, int hist, void* out, int denoise, double sigma_modifier, double fallback_sigma,
                        const void* xrec, double* sse_out, void* sigma_out, void* stream);

/* A whole OUTER iteration of the SVRG loop with the TV prox -- algorithms/pnp_svrg.py:32-95 for T2 inner iterations: the refresh
 * mu = grad_full(z), w = z, then T2 times { minibatch SVRG direction, step, estimate_sigma, TVDenoiser.denoise, PSNR } -- in ONE
 * launch: the workgroup that owns a problem runs pnp_csmri_svrg_outer_step and then T2 - 1 times pnp_csmri_svrg_step (a = z,
 * b = w, c1 = z, c2 = mu, alpha = -lr / mini_batch_size, beta = 1, gamma = -lr, out = z) on THAT problem back to back; the
 * results are bit for bit those of the T2 separate calls.  z is updated in place, w and mu are outputs.
 *   selbits  [T2][batch][W][H/32]: slot j = the selector of inner iteration j (pnp_csmri_draw_thresholds' layout; slot 0 is
 *            not read: at j = 0 the minibatch difference is exactly zero);
 *   sse_log  [n_log][batch] double: inner iteration j writes row (log_row0 + j) % n_log (sum (xrec - z)^2 after its prox);
 *   sigma_out [batch]: the noise estimate of the last inner iteration.                                        */
int pnp_csmri_svrg_outer_iteration(pnp_csmri_plan* plan, void* z, void* w, void* mu, const uint32_t* mask_bitsT, const void* yh,
                                   const void* alpha_vec, const uint32_t* selbits, int T2, double lr, int mini_batch_size,
                                   double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_log,
                                   int log_row0, int n_log, void* sigma_out, void* stream);

/* ------------------------------------------------------------------ per-problem hyper-parameters: the _pp forms
 * A hyper-parameter grid runs as ONE batch when every problem of the batch carries its own step size, minibatch size and
 * denoiser strength (sweep.grid_search(batch_trials=True)).  ONE naming scheme: an entry point `name_pp` is `name` with,
 * behind each scalar that has a per-problem form, a nullable DEVICE array of [batch] values -- `x_pp` (double) or `mb_vec`
 * (int32).  NULL means "the scalar holds for every problem"; with every such array NULL a _pp call computes what the plain
 * call computes.  The kernels read the arrays with plain loads of wave-uniform values (one workgroup owns one problem) and
 * convert each value exactly as the host converts the scalar of the plain call -- the same order of the 1/N scale, the cast to
 * `dtype` and the product with alpha_vec[b] -- so problem b of a _pp call equals, bit for bit, problem b of the plain call made
 * with that problem's scalars.  The plain entry points and their kernels are unchanged.
 *
 * Draws: problem b takes its own mb_vec[b] smallest keys (at or above its number of candidates: all of them), and its stream
 * absorbs draw_id[b] in place of the batch index b: state = mix64(mix64(mix64(seed) + step) + draw_id[b]).  draw_id == NULL:
 * the batch index.  Keys, fast path and radix fallback are those of the plain draw.  mb_vec is required; the call does not
 * synchronise, so it cannot read mb_vec: entries must be >= 1 (the Python front end checks its host copy and raises; an entry
 * below 1 that reaches the kernel draws as 1, never out of bounds).                                              */
int pnp_csmri_draw_thresholds_pp(pnp_csmri_plan* plan, const uint32_t* bitsT, const int32_t* mb_vec, const uint32_t* draw_id,
                                 uint64_t seed, uint32_t step0, int nsteps, const uint32_t* step_dev, void* mbd,
                                 uint32_t* selbits, void* stream);
int pnp_draw_thresholds_pp(int M, int batch, const int32_t* mb_vec, const uint32_t* draw_id, uint64_t seed, uint32_t step0,
                           int nsteps, const uint32_t* step_dev, void* mbd, void* stream);
/* pnp_csmri_grad_sel with per-problem alpha and gamma: problem b uses (alpha_pp ? alpha_pp[b] : alpha) * alpha_vec[b] and
 * (gamma_pp ? gamma_pp[b] : gamma).  On the one-kernel route (f32 256 x 256 bits form, large batches) a per-problem gamma
 * needs c1 beside c2 (PNP_ERR_ARG otherwise).                                                                     */
int pnp_csmri_grad_sel_pp(pnp_csmri_plan* plan, const void* a, const void* b, const uint8_t* selT, const uint32_t* bitsT,
                          const void* yh, const void* YT, double alpha, const double* alpha_pp, const void* alpha_vec,
                          double beta, const void* c1, double gamma, const double* gamma_pp, const void* c2, void* out,
                          void* stream);
/* The three one-kernel calls.  svrg_step: alpha_pp, gamma_pp, sigma_modifier_pp.  svrg_outer_step: lr_pp (the step uses
 * -lr_pp[b]), sigma_modifier_pp.  svrg_outer_iteration: lr_pp, mb_vec (the inner iterations use -lr_pp[b] / mb_vec[b], the
 * quotient taken in double as the plain call takes it on the host), sigma_modifier_pp.                               */
int pnp_csmri_svrg_step_pp(pnp_csmri_plan* plan, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                           const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, double gamma,
                           const double* gamma_pp, const void* c2, void* out, int denoise, double sigma_modifier,
                           const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_out,
                           void* sigma_out, void* stream);
/* pnp_csmri_sarah_step with alpha_pp, gamma_pp, sigma_modifier_pp: converted as pnp_csmri_svrg_step_pp converts them.         */
int pnp_csmri_sarah_step_pp(pnp_csmri_plan* plan, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                            const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, double gamma,
                            const double* gamma_pp, const void* c2, void* v_out, void* out, void* out2, int denoise,
                            double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                            double* sse_out, void* sigma_out, void* stream);
/* pnp_csmri_grad_step with alpha_pp, sigma_modifier_pp; pnp_csmri_saga_step with alpha_pp, lr_pp (cast as
 * pnp_saga_table_update_pp casts it), sigma_modifier_pp.  Problem b equals problem b of the plain call made with its scalars.     */
int pnp_csmri_grad_step_pp(pnp_csmri_plan* plan, const void* a, const uint32_t* bitsT, const void* yh, const void* YT,
                           double alpha, const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, void* out,
                           int denoise, double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma,
                           const void* xrec, double* sse_out, void* sigma_out, void* stream);
int pnp_csmri_saga_step_pp(pnp_csmri_plan* plan, const void* z, const uint32_t* bitsT, const void* YT, double alpha,
                           const double* alpha_pp, const void* alpha_vec, void* table, const int32_t* row, const int32_t* prev_row,
                           void* sum, double lr, const double* lr_pp, double inv_hist, int hist, void* out, int denoise,
                           double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                           double* sse_out, void* sigma_out, void* stream);
int pnp_csmri_svrg_outer_step_pp(pnp_csmri_plan* plan, const void* z, const uint32_t* mask_bitsT, const void* yh,
                                 const void* alpha_vec, double lr, const double* lr_pp, void* w_out, void* mu_out, void* out,
                                 int denoise, double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma,
                                 const void* xrec, double* sse_out, void* sigma_out, void* stream);
int pnp_csmri_svrg_outer_iteration_pp(pnp_csmri_plan* plan, void* z, void* w, void* mu, const uint32_t* mask_bitsT, const void* yh,
                                      const void* alpha_vec, const uint32_t* selbits, int T2, double lr, const double* lr_pp,
                                      int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                      const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_log,
                                      int log_row0, int n_log, void* sigma_out, void* stream);
/* pnp_csmri_svrg_outer_iteration_pp with the prox kind: denoise == 1 IS that call (the per-column prox, the same kernels, the
 * same bits); denoise == 2 runs pnp_csmri_svrg_outer_step_pp and then T2 - 1 times pnp_csmri_svrg_step_pp with denoise = 2 (the
 * 2-D wavelet prox inside the kernel) on every problem back to back, bit for bit the separate calls.  lr_pp, mb_vec and
 * sigma_modifier_pp are nullable as there.  PNP_ERR_ARG: any other value of denoise; otherwise as the _pp call.          */
int pnp_csmri_svrg_outer_iteration_prox(pnp_csmri_plan* plan, void* z, void* w, void* mu, const uint32_t* mask_bitsT,
                                        const void* yh, const void* alpha_vec, const uint32_t* selbits, int T2, double lr,
                                        const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                        const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                        double* sse_log, int log_row0, int n_log, void* sigma_out, int denoise, void* stream);
/* Per-problem T2: n_steps consecutive inner iterations s = step0 .. step0 + n_steps - 1 of every problem in ONE launch, with the TV
 * prox.  Problem b refreshes (mu = grad_full(z), w = z) at the steps with s % T2_b == 0, T2_b = t2_vec ? t2_vec[b] : T2 -- at its own
 * outer iterations, wherever the span starts or ends inside them (a problem with step0 % T2_b != 0 does not refresh at the span
 * start).  At a refresh step the workgroup that owns b runs pnp_csmri_svrg_outer_step on it, at every other step
 * pnp_csmri_svrg_step (a = z, b = w, c1 = z, c2 = mu, alpha = -lr / mini_batch_size, beta = 1, gamma = -lr, out = z), back to back;
 * the results are bit for bit those of the separate calls.  lr_pp, mb_vec, sigma_modifier_pp: as pnp_csmri_svrg_outer_iteration_pp.
 *   t2_vec   int32 [batch], nullable.  The call does not synchronise, so it cannot read t2_vec: entries must be >= 1 (the Python
 *            front end checks its host copy and raises; an entry below 1 that reaches the kernel counts as 1);
 *   selbits  [n_steps][batch][W][H/32]: slot i = the selector of step step0 + i (drawn with the absolute step id, so a problem
 *            sees the minibatch a scalar-T2 run gives it at that step); the slot of a refresh step is not read;
 *   sse_log  [n_log][batch] double: step s writes row (log_row0 + s - step0) % n_log.
 * PNP_ERR_ARG before any device work: a NULL pointer (t2_vec and the _pp arrays excepted), n_steps <= 0, step0 < 0, T2 <= 0 with a
 * NULL t2_vec, mini_batch_size <= 0 with a NULL mb_vec, a plan that is not f32 256 x 256, z, w, mu not three buffers.        */
int pnp_csmri_svrg_span_pp(pnp_csmri_plan* plan, void* z, void* w, void* mu, const uint32_t* mask_bitsT, const void* yh,
                           const void* alpha_vec, const uint32_t* selbits, int step0, int n_steps, int T2, const int32_t* t2_vec,
                           double lr, const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                           const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_log,
                           int log_row0, int n_log, void* sigma_out, void* stream);
/* Per-problem T2 for the SARAH loop: n_steps consecutive inner iterations s = step0 .. step0 + n_steps - 1 of every problem in ONE
 * launch, with the TV prox.  Problem b takes its outer step (w_prev = z, v_prev = grad_full(z), w_next = prox_TV(z - eta * v_prev); z
 * not written, eta without decay) at the steps with s % T2_b == 0, T2_b = t2_vec ? t2_vec[b] : T2 -- at its own outer iterations,
 * wherever the span starts or ends inside them (a problem with step0 % T2_b != 0 takes none at the span start).  At such a step the
 * workgroup that owns b runs pnp_csmri_svrg_outer_step (out = w_next, w_out = w_prev, mu_out = v_prev) and then, as at every other
 * step, pnp_csmri_sarah_step (a = w_next, b = w_prev, c1 = v_prev, c2 = z, alpha = 1 / mini_batch_size, beta = 1, gamma = -lr, v_out =
 * v_prev, out = z, out2 = w_prev), back to back; the results are bit for bit those of the separate calls.  The span form is for a
 * constant step size: the host passes lr = eta (lr_pp = eta_pp).  eta_pp, lr_pp, mb_vec, sigma_modifier_pp: as
 * pnp_csmri_sarah_outer_iteration_pp.
 *   t2_vec    int32 [batch], nullable; entries must be >= 1 (the Python front end checks its host copy and raises; an entry below 1
 *             that reaches the kernel counts as 1);
 *   selbits   [n_steps][batch][W][H/32]: slot i = the selector of step step0 + i (drawn with the absolute step id); the slot of a
 *             step with an outer step IS read (the outer step is no inner iteration);
 *   sse_log   [n_log][batch] double: inner iteration s writes row (log_row0 + s - step0) % n_log;
 *   outer_log [n_log][batch] double, a ring of its own: the same row gets the squared error of the outer prox problem b made at step
 *             s, NaN where it made none (written by the device: a wrapping ring needs no host fill).
 * PNP_ERR_ARG before any device work: a NULL pointer (t2_vec and the _pp arrays excepted), n_steps <= 0, step0 < 0, T2 <= 0 with a
 * NULL t2_vec, mini_batch_size <= 0 with a NULL mb_vec, n_log < 1, log_row0 < 0, a plan that is not f32 256 x 256, z, w_prev, w_next,
 * v_prev not four distinct buffers, sse_log == outer_log.                                                               */
int pnp_csmri_sarah_span_pp(pnp_csmri_plan* plan, void* z, void* w_prev, void* w_next, void* v_prev, const uint32_t* mask_bitsT,
                            const void* yh, const void* alpha_vec, const uint32_t* selbits, int step0, int n_steps, int T2,
                            const int32_t* t2_vec, double eta, const double* eta_pp, double lr, const double* lr_pp,
                            int mini_batch_size, const int32_t* mb_vec, double sigma_modifier, const double* sigma_modifier_pp,
                            double fallback_sigma, const void* xrec, double* sse_log, double* outer_log, int log_row0, int n_log,
                            void* sigma_out, void* stream);
/* A whole OUTER iteration of the SARAH loop with the TV prox -- algorithms/pnp_sarah.py:28-104 for T2 inner iterations -- in ONE
 * launch: the workgroup that owns a problem runs the outer step, pnp_csmri_svrg_outer_step (w_out = w_prev, mu_out = v_prev,
 * out = w_next, lr = eta: w_prev = z, v_prev = grad_full(z), w_next = prox_TV(z - eta * v_prev); z is NOT written and eta does not
 * decay), and then T2 times pnp_csmri_sarah_step (a = w_next, b = w_prev, alpha = 1 / mini_batch_size, beta = 1,
 * c1 = v_prev, gamma = -lr, c2 = z, v_out = v_prev, out = z, out2 = w_prev) on THAT problem back to back; the results are bit for
 * bit those of the T2 + 1 separate calls.  z, w_prev and v_prev are updated in place, w_next is an output.
 *   selbits  [T2][batch][W][H/32]: slot j = the selector of inner iteration j.  Unlike pnp_csmri_svrg_outer_iteration, slot 0 IS
 *            read: the outer step is no inner iteration, the inner loop runs j = 0 .. T2 - 1 behind it;
 *   sse_log  [n_log][batch] double, T2 + 1 rows per call: the outer prox writes row log_row0 % n_log, inner iteration j row
 *            (log_row0 + 1 + j) % n_log;
 *   sigma_out [batch]: the noise estimate of the last inner iteration.
 * The _pp form: eta_pp, lr_pp, sigma_modifier_pp double [batch], mb_vec int32 [batch], each nullable; converted as
 * pnp_csmri_svrg_outer_step_pp (the outer step: -eta_pp[b]) and pnp_csmri_sarah_step_pp (1 / mb_vec[b] taken in double as the host
 * takes it, -lr_pp[b]) convert them: problem b equals problem b of the plain call made with its scalars.
 * PNP_ERR_ARG before any device work: a NULL plan, z, w_prev, w_next, v_prev, mask_bitsT, yh, alpha_vec, selbits, xrec, sse_log or
 * sigma_out; T2 <= 0; n_log < 1; log_row0 < 0; mini_batch_size <= 0 with a NULL mb_vec; a plan that is not f32 256 x 256; z, w_prev,
 * w_next, v_prev not four distinct buffers.                                                                          */
int pnp_csmri_sarah_outer_iteration(pnp_csmri_plan* plan, void* z, void* w_prev, void* w_next, void* v_prev,
                                    const uint32_t* mask_bitsT, const void* yh, const void* alpha_vec, const uint32_t* selbits,
                                    int T2, double eta, double lr, int mini_batch_size, double sigma_modifier,
                                    double fallback_sigma, const void* xrec, double* sse_log, int log_row0, int n_log,
                                    void* sigma_out, void* stream);
int pnp_csmri_sarah_outer_iteration_pp(pnp_csmri_plan* plan, void* z, void* w_prev, void* w_next, void* v_prev,
                                       const uint32_t* mask_bitsT, const void* yh, const void* alpha_vec, const uint32_t* selbits,
                                       int T2, double eta, const double* eta_pp, double lr, const double* lr_pp,
                                       int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                       const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_log,
                                       int log_row0, int n_log, void* sigma_out, void* stream);
/* n_steps consecutive inner iterations of the GD or the SGD loop -- algorithms/pnp_gd.py:24-70, pnp_sgd.py:24-70 -- with the TV prox
 * in ONE launch, z in place: the workgroup that owns a problem runs n_steps times pnp_csmri_grad_step_pp (a = c1 = out = z) on THAT
 * problem back to back; the results are bit for bit those of the separate calls.  The arguments are those of
 * pnp_csmri_grad_step_pp without out and c1 and with sse_out replaced by the span's log.  Exactly one of yh and YT:
 *   yh (GD):  bitsT [batch][W][H/32] = the mask, the same array at every step;
 *   YT (SGD): bitsT [n_steps][batch][W][H/32] = drawn selbits, slot i = the selector of step i.
 *   sse_log  [n_log][batch] double: step i writes row (log_row0 + i) % n_log;  sigma_out [batch]: the last step's estimate.
 * The kernels hold the per-column prox: denoise must be != 0 and != 2 (the 2-D wavelet prox is not in the span kernels).
 * PNP_ERR_ARG before any device work: a NULL plan, z, bitsT, xrec, sse_log or sigma_out; both or neither of yh and YT;
 * n_steps <= 0; n_log < 1; log_row0 < 0; denoise == 0 or 2; a plan that is not f32 256 x 256.                         */
int pnp_csmri_grad_span(pnp_csmri_plan* plan, void* z, const uint32_t* bitsT, const void* yh, const void* YT, double alpha,
                        const double* alpha_pp, const void* alpha_vec, double beta, int denoise, double sigma_modifier,
                        const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps, double* sse_log,
                        int log_row0, int n_log, void* sigma_out, void* stream);
/* n_steps consecutive inner iterations of the SAGA loop -- algorithms/pnp_saga.py:43-79 -- with the TV prox in ONE launch: the
 * workgroup that owns a problem runs n_steps times pnp_csmri_saga_step_pp (out = z) on THAT problem back to back; the results are bit
 * for bit those of the separate calls.  table, sum and z are updated in place (there is no `out`).  The arguments are those of
 * pnp_csmri_saga_step_pp with
 *   bitsT     [n_steps][batch][W][H/32]: drawn selbits, slot i = the selector of step i;
 *   rows      int32 [n_steps][batch]: step i replaces row rows[i][b] of problem b;
 *   prev_row0 int32 [batch]: the row the step before the span replaced.  Step i takes prev = rows[i - 1][b] (prev_row0[b] at i = 0);
 *             rows[i][b] == prev is legal.  Entries in [0, hist): the kernel cannot check them (the Python front end checks its host
 *             copy and raises);
 *   sse_log, log_row0, n_log, sigma_out as in pnp_csmri_grad_span.  denoise must be != 0 and != 2.
 * PNP_ERR_ARG before any device work: a NULL plan, z, bitsT, YT, table, rows, prev_row0, sum, xrec, sse_log or sigma_out;
 * hist < 1; n_steps <= 0; n_log < 1; log_row0 < 0; denoise == 0 or 2; a plan that is not f32 256 x 256; table or sum overlapping z, xrec
 * or each other.                                                                                                     */
int pnp_csmri_saga_span(pnp_csmri_plan* plan, void* z, const uint32_t* bitsT, const void* YT, double alpha, const double* alpha_pp,
                        const void* alpha_vec, void* table, const int32_t* rows, const int32_t* prev_row0, void* sum, double lr,
                        const double* lr_pp, double inv_hist, int hist, int denoise, double sigma_modifier,
                        const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps, double* sse_log,
                        int log_row0, int n_log, void* sigma_out, void* stream);
/* pnp_csmri_saga_step_pp and pnp_csmri_saga_span with the divisor of the running sum per problem: problem b multiplies its sum by
 * inv_hist_pp ? inv_hist_pp[b] : inv_hist ([batch] doubles on the device, 1 / hist[b], cast to float as the scalar is cast and read
 * once per workgroup).  `hist` is the row count of the table, the largest history length of the batch; problem b names rows below its
 * own history length only (row, prev_row, rows, prev_row0: the caller checks its host copy), so the rows beyond it are never touched.
 * Problem b equals, bit for bit, problem b of the plain call made with its own divisor.  Errors as the calls they extend; both hold
 * the per-column prox only: denoise == 2 is PNP_ERR_ARG (pnp_csmri_saga_step_pp takes the 2-D prox).                          */
int pnp_csmri_saga_step_hist_pp(pnp_csmri_plan* plan, const void* z, const uint32_t* bitsT, const void* YT, double alpha,
                                const double* alpha_pp, const void* alpha_vec, void* table, const int32_t* row,
                                const int32_t* prev_row, void* sum, double lr, const double* lr_pp, double inv_hist,
                                const double* inv_hist_pp, int hist, void* out, int denoise, double sigma_modifier,
                                const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_out,
                                void* sigma_out, void* stream);
int pnp_csmri_saga_span_hist(pnp_csmri_plan* plan, void* z, const uint32_t* bitsT, const void* YT, double alpha,
                             const double* alpha_pp, const void* alpha_vec, void* table, const int32_t* rows,
                             const int32_t* prev_row0, void* sum, double lr, const double* lr_pp, double inv_hist,
                             const double* inv_hist_pp, int hist, int denoise, double sigma_modifier,
                             const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps, double* sse_log,
                             int log_row0, int n_log, void* sigma_out, void* stream);
/* pnp_prox_tv / pnp_prox_wavelet2d with sigma used = sigma_est * (sigma_modifier_pp ? sigma_modifier_pp[b] : sigma_modifier). */
int pnp_prox_tv_pp(const void* z_in, void* z_out, int H, int W, int batch, int dtype, const void* sigma_in,
                   double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                   double* sse_out, void* sigma_out, void* stream);
int pnp_prox_wavelet2d_pp(const void* z_in, void* z_out, int H, int W, int batch, int dtype, const void* sigma_in,
                          double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                          double* sse_out, void* sigma_out, void* stream);

/* ------------------------------------------------------------------ Deblur / super-resolution
 * Replaces problems/DeblurSR.py:119-147: 1-D circular blur of the raveled image via a length-H*W FFT
 * (spectrum of the kernel computed once at plan creation), optional 4-tap bilinear down-sampler
 * (pylops Bilinear semantics; its adjoint as a deterministic CSR gather).  H*W in {64^2, 128^2, 256^2}.
 * Plan-creation arrays are HOST pointers: Bk [H*W] blur kernel (DeblurSR.py:93, already / N, `dtype`);
 * for scale_percent == 100 pass M = H*W and NULL operators; else g_idx/g_w [M][4] (forward taps) and
 * a_rowptr [H*W+1], a_col/a_val [nnz] (CSR of the adjoint: the transpose of the taps entry for entry,
 * nnz = 4 * M).  PNP_ERR_ARG before any allocation or device work: g_idx outside [0, H*W), a_rowptr that
 * does not start at 0, decreases or does not end at 4 * M, a_col outside [0, M).                  */
typedef struct pnp_deblur_plan pnp_deblur_plan;
int pnp_deblur_plan_create(pnp_deblur_plan** plan, int H, int W, int batch, int dtype, const void* Bk, int M,
                           const int32_t* g_idx, const void* g_w, const int32_t* a_rowptr,
                           const int32_t* a_col, const void* a_val);
int pnp_deblur_plan_destroy(pnp_deblur_plan* plan);
/* out = scale * B^T S^T ( sel o (S B z - Y) )   (grad_full: sel = NULL, scale = 1/M; grad_stoch:
 * sel = minibatch indicator uint8 [batch][M], scale = 1).  z, out [batch][H*W]; Y [batch][M].   */
int pnp_deblur_grad(pnp_deblur_plan* plan, const void* z, const void* Y, const uint8_t* sel, double scale,
                    void* out, void* stream);
/* grad_stoch with a device-drawn minibatch: mbd = this step's [batch] threshold descriptors from
 * pnp_draw_thresholds(M, ...); the indicator is re-derived where the residual is masked, never stored.   */
int pnp_deblur_grad_mb(pnp_deblur_plan* plan, const void* z, const void* Y, const void* mbd, double scale,
                       void* out, void* stream);
/* forward model S B x (DeblurSR.py:110-112): out [batch][M]                                     */
int pnp_deblur_forward(pnp_deblur_plan* plan, const void* x, void* out, void* stream);
/* _pp forms of the two gradients (a Deblur grid as one batch): problem b is scaled by scale_pp ? scale_pp[b] : scale.
 * Its output factor is formed as the plain call forms it on the host -- (dtype)(scale_b / sqrt((double)(H*W))), the quotient in
 * double, then the cast -- so problem b equals, bit for bit, problem b of the plain call made with scale_b.  The descriptors of
 * _mb_pp come from pnp_draw_thresholds_pp (per-problem minibatch sizes and stream ids).                              */
int pnp_deblur_grad_pp(pnp_deblur_plan* plan, const void* z, const void* Y, const uint8_t* sel, double scale,
                       const double* scale_pp, void* out, void* stream);
int pnp_deblur_grad_mb_pp(pnp_deblur_plan* plan, const void* z, const void* Y, const void* mbd, double scale,
                          const double* scale_pp, void* out, void* stream);
/* The variance-reduced correction and the step in one gradient pass (pnp_svrg.py:53,57 / pnp_sarah.py:72-75):
 *   out = beta*c1 + gamma_b*c2 + scale_b * B^T S^T ( sel o ( S B (a - b) - Y ) )
 * b    == NULL : a alone.
 * Y    == NULL : no data term (the y terms of a minibatch difference cancel).
 * sel  : uint8 [batch][M]; mbd: one step's threshold descriptors.  Either, neither, never both.
 * scale_b = scale_pp ? scale_pp[b] : scale, the output factor formed as the _pp gradients form it: (dtype)(scale_b / sqrt((double)(H*W)))
 * gamma_b = gamma_pp ? gamma_pp[b] : gamma, cast once to dtype; beta likewise.
 * c1 / c2 == NULL : that addend is absent.
 * The difference a - b is formed where the first FFT pass loads it; the three terms of the result are rounded one by one in the
 * stated order (o = factor*Re; o += beta*c1; o += gamma_b*c2) where the last pass stores it, the addends read at the index that is
 * written: out may alias a, b, c1 or c2.  Problem b of a call with scale_pp / gamma_pp equals, bit for bit, problem b of the scalar
 * call with its values, whatever the batch size and its place in the batch.  Not bit-compatible with two pnp_deblur_grad calls and
 * a combination (one rounding of a - b instead of those of two gradients).  Uniform plans only (a mixed-scale plan: PNP_ERR_ARG).
 * PNP_ERR_ARG before any device work: NULL plan, a or out; sel and mbd together; beta != 0 without c1; gamma != 0 or a gamma_pp
 * without c2.  No allocation, no synchronisation: capturable.                                                              */
int pnp_deblur_grad_step(pnp_deblur_plan* plan, const void* a, const void* b, const void* Y, const uint8_t* sel, const void* mbd,
                         double scale, const double* scale_pp, double beta, const void* c1, double gamma, const double* gamma_pp,
                         const void* c2, void* out, void* stream);
/* Mixed-scale plans (a sampling-ratio sweep as one batch; csrc/deblur_mixed.hip): every problem has a down-sampler and
 * a measurement count M_b of its own.  The plan owns n_sets distinct down-samplers -- the five arrays of pnp_deblur_plan_create
 * concatenated over the sets, all HOST pointers: M_set [n_sets]; the tap rows of set s are rows [g_off[s], g_off[s+1]) of
 * g_idx / g_w (M_set[s] rows, or none for the identity set, M_set[s] == H*W); its CSR entries are [nz_off[s], nz_off[s+1]) of
 * a_col / a_val; a_rowptr holds H*W + 1 entries for every set WITH tables, in set order, each counting from 0.  Problem b works
 * on set set_of[b] and M_vec[b] must be that set's M.  Mmax = max M_b.  Y, sel, the forward output and the plan's scratch are
 * [batch][Mmax]: entries m >= M_b of a row are padding that no call reads into a result; the forward pass and the generator write
 * them as zero.  Destroy with pnp_deblur_plan_destroy.  PNP_ERR_ARG before any device work: a NULL array, set_of out of range,
 * M_vec[b] != M of its set, M_s outside [1, H*W], tables that point outside the image or the set's measurements.  The other
 * pnp_deblur_* calls refuse a mixed plan, and the _mixed calls a plan of pnp_deblur_plan_create (PNP_ERR_ARG).
 * pnp_deblur_generate takes either.
 * The calls below scale problem b by scale_pp ? scale_pp[b] : scale, as the _pp forms do; the blurs are those of the uniform
 * plan over the whole batch and the tap / CSR sums keep the order of the uniform kernels, so a problem WITH a down-sampler equals,
 * bit for bit, the same problem in a uniform batch of its scale, wherever it sits and whatever its neighbours are (an identity
 * problem takes "- Y" behind the blur's rounding instead of inside its epilogue: equal to rounding).  No allocation, no
 * synchronisation: capturable.  pnp_deblur_objective_mixed: f_out[b] = (scale / M_b) * sum over m < M_b of (S_b B z - Y)^2
 * (the host passes scale = 1/2), sums as pnp_deblur_objective's.                                                           */
int pnp_deblur_plan_create_mixed(pnp_deblur_plan** plan, int H, int W, int batch, int dtype, const void* Bk, int n_sets,
                                 const int32_t* M_set, const int32_t* g_off, const int32_t* g_idx, const void* g_w,
                                 const int32_t* nz_off, const int32_t* a_rowptr, const int32_t* a_col, const void* a_val,
                                 const int32_t* set_of, const int32_t* M_vec);
int pnp_deblur_grad_mixed(pnp_deblur_plan* plan, const void* z, const void* Y, const uint8_t* sel, double scale,
                          const double* scale_pp, void* out, void* stream);
int pnp_deblur_grad_mb_mixed(pnp_deblur_plan* plan, const void* z, const void* Y, const void* mbd, double scale,
                             const double* scale_pp, void* out, void* stream);
int pnp_deblur_forward_mixed(pnp_deblur_plan* plan, const void* x, void* out, void* stream);
int pnp_deblur_objective_mixed(pnp_deblur_plan* plan, const void* z, const void* Y, double scale, double* f_out, void* stream);

/* ------------------------------------------------------------------ phase retrieval
 * Replaces problems/PR.py:75-87.  A [M][N] row-major, w [N], y [M] (device, `dtype`).
 * out = scale * A_sel^T ( ((|A_sel w| - y_sel)/|A_sel w|) o A_sel w ); rows int32 [nsel] or NULL (all).
 * workspace: pnp_pr_workspace_elems(M, N) elements of `dtype`.                                  */
size_t pnp_pr_workspace_elems(int M, int N);
int pnp_pr_grad(const void* A, const void* w, const void* y, const int32_t* rows, int nsel, int M, int N,
                int dtype, double scale, void* workspace, void* out, void* stream);
/* B independent problems per call: A [batch][M][N], w [batch][N], y [batch][M], rows [batch][nsel] (NULL = all rows),
 * out [batch][N]; workspace: batch * pnp_pr_workspace_elems(M, N) elements.                                  */
int pnp_pr_grad_batch(const void* A, const void* w, const void* y, const int32_t* rows, int nsel, int M, int N, int batch,
                      int dtype, double scale, void* workspace, void* out, void* stream);
/* One power-iteration step of PhaseRetrieval.spec_init (problems/PR.py:50-63): out = scale * A^T (y o (A v)), i.e.
 * D v for D = A^T diag(y) A / M (scale = 1/M) without forming the N x N matrix.  v, out [N]; same workspace.      */
int pnp_pr_spectral_apply(const void* A, const void* v, const void* y, int M, int N, int dtype, double scale,
                          void* workspace, void* out, void* stream);
/* Gradients of batch = G * items problems that SHARE `items` matrices (a trial-batched grid, csrc/pr_shared.hip): problem
 * b = t * items + i works on A[i] and Y[i].  A [items][M][N], Y [items][M], W [batch][N], W2 [batch][N] or NULL, out [batch][N]:
 *   out[b] = (alpha_b / alpha_div) * (g_b(W[b]) - g_b(W2[b])) + beta * c1[b] + gamma_b * c2[b]
 * with g_b(x) = A_sel^T(((|A_sel x| - y_sel) / |A_sel x|) o A_sel x) over the rows problem b selects; the W2 term is dropped when
 * W2 == NULL; c1, c2 [batch][N] or NULL.  alpha_b = alpha_pp ? alpha_pp[b] : alpha and gamma_b likewise (_pp form; [batch] doubles
 * on the device); the quotient alpha_b / alpha_div is taken in double and rounded to `dtype` as the host rounds a scalar
 * (grad_full: alpha_div = M; else 1).
 * Selection per problem: mbd ([batch] threshold descriptors of pnp_draw_thresholds(M, ...), membership re-derived in the kernel),
 * or ind (uint8 [batch][M]), or neither (all M rows); both is an argument error.  A row that problem b did not select contributes
 * exactly zero to b (its weight is written as 0), whatever the matrix holds there.
 * Both products run on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64; the 16-wide dimension is the problem
 * columns) and A is streamed twice per call and item for up to 64 (W2: 32) problems per item, whatever G is.  Any M, N >= 1
 * (scalar loads where N is not a multiple of 16 bytes or a pointer is not 16-byte aligned).  Deterministic, no atomics: the split
 * of the sums depends on (M, N, dtype) only, so a problem's result is bit-identical whatever G is, wherever it sits in the batch
 * and whatever the other problems select.  out may alias W, c1 or c2 (W and W2 are read before out is written).
 * workspace: pnp_pr_shared_workspace_elems(M, N, batch) elements of `dtype`, 16-byte aligned (enough for any `items`).           */
size_t pnp_pr_shared_workspace_elems(int M, int N, int batch);
int pnp_pr_grad_shared(const void* A, const void* Y, const void* W, const void* W2, const void* mbd, const uint8_t* ind, int M, int N,
                       int batch, int items, int dtype, double alpha, double alpha_div, double beta, const void* c1, double gamma,
                       const void* c2, void* workspace, void* out, void* stream);
int pnp_pr_grad_shared_pp(const void* A, const void* Y, const void* W, const void* W2, const void* mbd, const uint8_t* ind, int M,
                          int N, int batch, int items, int dtype, double alpha, const double* alpha_pp, double alpha_div, double beta,
                          const void* c1, double gamma, const double* gamma_pp, const void* c2, void* workspace, void* out,
                          void* stream);

/* ------------------------------------------------------------------ Deblur / PR sweep batches generated on the device
 * The same stream for the other two problems (tags 0-2 keep the meaning above; state_k and key_k(i) are unchanged), so that a
 * caller can restate a generated Deblur or phase-retrieval batch from this header alone:
 *   measurement noise (k = 1, 2): indexed by the measurement index m: u1 = (key_1(m) + 1) * 2^-32, u2 = key_2(m) * 2^-32,
 *                     n(m) = sqrt(-2 ln u1) * cos(2 pi u2), Box-Muller in double for both dtypes;
 *   PR matrix (k = 3, 4): indexed by the pair index j = (m*N + n) >> 1: r = sqrt(-2 ln u1(key_3(j))), element m*N + n of
 *                     A [M][N] is r * cos(2 pi u2(key_4(j))) when m*N + n is even and r * sin(2 pi u2(key_4(j))) when odd (both
 *                     Box-Muller outputs of one pair, u1 and u2 formed as above), in double, rounded once to `dtype`; M*N <= 2^32,
 *                     otherwise PNP_ERR_ARG;
 *   Deblur Xinit (k = 5): Xinit(i) = key_5(i) * 2^-32 in [0, 1)  (np.random.uniform(0, 1, N), problems/DeblurSR.py:57), rounded
 *                     to `dtype`;
 *   sigma           : sigma = sqrt(||Y0||_2 * snr_fac / H / W) (the norm, not its square), the sum of squares of the stored Y0
 *                     taken in double in a fixed order per item;  Y = Y0 + sigma * n, one more rounding to `dtype`.
 * An f32 and an f64 call hold the same problem up to the final rounding.  Per item [batch] device arrays image_idx (int32),
 * snr_fac (double), seed, id (uint64) and the image set as in pnp_csmri_generate.  No allocation, no synchronisation; an item's
 * outputs do not depend on the batch size or on its index in the batch.
 *
 * pnp_deblur_generate (problems/DeblurSR.py:38-57 per item) on an existing plan (identity or bilinear): xrec [batch][H*W] =
 * images[image_idx[b]]; Y [batch][M] = S B xrec (the plan's forward pass) + sigma * n; xinit [batch][H*W]; sigma [batch] double.
 * On a mixed-scale plan (pnp_deblur_plan_create_mixed) Y is [batch][Mmax]: Y_b = S_b B xrec_b + sigma_b * n over m < M_b with
 * sigma_b from ||Y0_b|| over its M_b entries, zeros in the padding; the noise is keyed by the item's id and m, so an item's
 * Y[:M_b], xinit and sigma equal, bit for bit, those a uniform plan of its scale generates, whatever its neighbours.          */
int pnp_deblur_generate(pnp_deblur_plan* plan, const void* images, int n_images, const int32_t* image_idx,
                        const double* snr_fac, const uint64_t* seed, const uint64_t* id, void* xrec, void* Y, void* xinit,
                        double* sigma, void* stream);
/* pnp_pr_generate (problems/PR.py:26-34 per item) for `batch` items sharing M and N = H*W: A [batch][M][N] from tags 3 and 4;
 * xrec [batch][N]; Y [batch][M] = |A xrec| (row dot products accumulated in double) + sigma * n; sigma [batch] double.        */
int pnp_pr_generate(const void* images, int n_images, const int32_t* image_idx, const double* snr_fac, const uint64_t* seed,
                    const uint64_t* id, int H, int W, int M, int batch, int dtype, void* A, void* xrec, void* Y, double* sigma,
                    void* stream);
/* PhaseRetrieval.spec_init and the normalisation after it (problems/PR.py:50-63, :38) for `batch` items at once: the power
 * iteration v <- A^T (Y o (A v)) / M from v = 2 * ones, lead = max(v), v <- v / lead, until the reference's rule
 * |lead - lead_old| > 1e-5 and ||v - v_old||_2 > 1e-5 fails.  A and Y are read in `dtype`; v, lead, the change norm and every
 * sum are double for both dtypes.  The rule is evaluated per item ON THE DEVICE after every step; an item whose rule has failed
 * is frozen (its v, lead and iteration count are not touched again), so its result does not depend on the batch.  Then
 * xinit [batch][N] = minmax( sqrt(lead) * v / ||v|| * ||xrec|| ), rounded to `dtype`.
 * This is a SETUP call, the one exception to "no synchronisation": steps are launched `check_every` at a time, after which ONE
 * int ("is any item active") is read back with a stream synchronisation; it cannot be captured in a hipGraph.  It stops after
 * max_iters steps at the latest.  iters_out [batch] int32: steps taken per item; active_out [batch] int32: nonzero for an item
 * that had not met its rule when max_iters was reached (the caller decides what that means; xinit is written regardless).
 * workspace: pnp_pr_spectral_workspace_bytes(M, N, batch) bytes, 8-byte aligned.                                              */
size_t pnp_pr_spectral_workspace_bytes(int M, int N, int batch);
int pnp_pr_spectral_init_batch(const void* A, const void* Y, const void* xrec, int M, int N, int batch, int dtype,
                               int max_iters, int check_every, void* workspace, void* xinit, int32_t* iters_out,
                               int32_t* active_out, void* stream);

/* ------------------------------------------------------------------ prox / noise estimate
 * estimate_sigma(z0, multichannel=True, average_sigmas=True) (algorithms/pnp_svrg.py:71):
 * per-column db2 MAD, mean over columns.  sigma_out: [batch] (dtype).                    */
int pnp_sigma_est(const void* z, int H, int W, int batch, int dtype, void* sigma_out, void* stream);

/* TVDenoiser.denoise (denoisers/TV.py:21-26 = per-column Haar BayesShrink) fused with the
 * noise estimate that feeds it and with the squared-error sum of Problem.PSNR
 * (problems/problem.py:33-35).
 *   sigma used = sigma_est*sigma_modifier if sigma_est > 0 else fallback_sigma
 *   sigma_est  = sigma_in[b] if sigma_in != NULL else estimated in-kernel
 *   xrec, sse_out may be NULL; sse_out: [batch] double = sum (xrec - out)^2
 *   sigma_out (may be NULL): [batch] (dtype) the sigma_est that was used.               */
int pnp_prox_tv(const void* z_in, void* z_out, int H, int W, int batch, int dtype,
                const void* sigma_in, double sigma_modifier, double fallback_sigma,
                const void* xrec, double* sse_out, void* sigma_out, void* stream);

/* TVDenoiser(multi=False).denoise (denoisers/TV.py:21-26 with multichannel=False): ONE two-dimensional multi-level
 * Haar decomposition of the image (pywt.wavedecn, L = max(min(log2 H, log2 W) - 3, 1) levels), one BayesShrink
 * threshold per detail sub-band (ad, da, dd of every level, each over the whole image), soft shrinkage,
 * reconstruction -- fused, like pnp_prox_tv, with the noise estimate and the squared-error sum.
 * Argument for argument pnp_prox_tv, same shapes (H in {16, 32, 64, 128, 256}, W a multiple of 16 in [16, 256]),
 * same meaning: the estimate made when sigma_in == NULL is pnp_sigma_est's (per-COLUMN db2 MAD, what the loops pass
 * to every denoiser) bit for bit.  z_out may alias z_in.  An image's result does not depend on the batch.        */
int pnp_prox_wavelet2d(const void* z_in, void* z_out, int H, int W, int batch, int dtype,
                       const void* sigma_in, double sigma_modifier, double fallback_sigma,
                       const void* xrec, double* sse_out, void* sigma_out, void* stream);

/* NLMDenoiser.denoise (denoisers/NLM.py:22-27 -> skimage 0.18 _nl_means_denoising_2d, slow mode,
 * Schraudolph fast_exp).  patch_size as the caller passes it (even sizes are bumped to the
 * next odd one like skimage: 4 -> 5; supported sides 3/5/7), patch_distance in [1, 8].  H and W must be
 * at least side/2 + 1 (2, 3, 4): the border is reflected once, as np.pad(mode='reflect') does down to there.
 *   sigma_in != NULL : h = sigma = sigma_in[b]*sigma_modifier, var = 2 sigma^2   (NLM.py:25)
 *   sigma_in == NULL : h = fixed_h, var = 0                                     (NLM.py:27)
 *   w0 [side*side] (device, double) = exp(-(x^2+y^2)/(2A^2)), A = (side-1)/4, and w0_sum = its sum as
 *   NumPy computes it (the caller builds both once: bit-for-bit the reference's normalisation).
 *   z_out must not alias z_in.  sse_out [batch] double (optional; needs xrec and sse_workspace of
 *   batch*ceil(H/16)*ceil(W/16) doubles).                                                     */
int pnp_nlm2d(const void* z_in, void* z_out, int H, int W, int batch, int dtype, int patch_size,
              int patch_distance, const void* sigma_in, double sigma_modifier, double fixed_h,
              const double* w0, double w0_sum, const void* xrec, double* sse_out, double* sse_workspace,
              void* stream);
/* _pp form: h = sigma = sigma_in[b] * (sigma_modifier_pp ? sigma_modifier_pp[b] : sigma_modifier), the product taken in double
 * and cast as in the plain call ([batch] doubles on the device; without sigma_in the modifier is not read).  Both kernel forms
 * (LDS-streaming and register-strip) have it; image b equals, bit for bit, image b of the plain call made with its modifier. */
int pnp_nlm2d_pp(const void* z_in, void* z_out, int H, int W, int batch, int dtype, int patch_size,
                 int patch_distance, const void* sigma_in, double sigma_modifier, const double* sigma_modifier_pp,
                 double fixed_h, const double* w0, double w0_sum, const void* xrec, double* sse_out,
                 double* sse_workspace, void* stream);

/* sum (xrec - z)^2 per problem (Problem.PSNR, problems/problem.py:33-35). sse_out: [batch] double */
int pnp_sse(const void* z, const void* xrec, int n_per_problem, int batch, int dtype, double* sse_out, void* stream);

/* per-problem min and max (RealSN_DnCNN.py:20-22). out: [batch][2] (dtype)               */
int pnp_minmax(const void* z, int n_per_problem, int batch, int dtype, void* out, void* stream);

/* ------------------------------------------------------------------ DnCNN prox (MFMA)
 * Replaces RealSN_DnCNNDenoiser.denoise (denoisers/RealSN_DnCNN.py:16-42) around the 17-layer
 * network of denoisers/DeepDenoisers/model/models.py:5-22 (realSN_models.py:4-21 at inference:
 * the spectral-norm hook only detaches the stored weight).
 * Weights are HOST pointers (plan creation is setup): BatchNorm already folded by the caller.
 *   w_first [64][3][3]            conv(1->64), no bias
 *   w_mid   [n_mid][64][64][3][3] conv(64->64) x BN scale;  b_mid [n_mid][64] folded BN bias
 *   w_last  [64][3][3]            conv(64->1), no bias
 * H % 8 == 0, W % 32 == 0.  The plan owns two [batch][64][H][W] fp32 activation buffers.   */
typedef struct pnp_dncnn_plan pnp_dncnn_plan;
int pnp_dncnn_plan_create(pnp_dncnn_plan** plan, int n_mid, const float* w_first, const float* w_mid,
                          const float* b_mid, const float* w_last, int H, int W, int batch);
int pnp_dncnn_plan_destroy(pnp_dncnn_plan* plan);
/* Biases of the first / last layer and the activation, for networks of the same 3x3-conv shape that are not
 * bias-free ReLU nets: the MMO `simple_CNN` (denoisers/MMODenoise.py:73-101: every conv has a bias, LeakyReLU(0.01),
 * b_mid goes in through plan_create).  b_first: HOST [64] or NULL (= zeros); negative_slope 0 = ReLU.         */
int pnp_dncnn_set_affine(pnp_dncnn_plan* plan, const float* b_first, float b_last, float negative_slope);
/* Conv kernel choice for the 64->64 layers (0, 1, 5: fp32 on the f32 matrix cores):
 *   5 = Winograd F(4x4,3x3) (default where H % 8 == 0 and W % 64 == 0; executes 1/4 of the direct form's multiply-adds;
 *       accuracy envelope: <= 2e-5 absolute against the reference network on its own weights (measured 8e-7), <= 1e-5
 *       relative against a float64 evaluation on white-noise weights -- about 5x the direct form's rounding error),
 *   1 = Winograd F(2,3) along x (2/3; the default for the other sizes),
 *   0 = direct implicit GEMM (bit-for-bit an fmaf chain; the one-flag way back for parity runs),
 *   6 = opt-in: F(4x4,3x3) on the BF16 matrix cores, every fp32 factor split exactly into three bf16 terms and the six
 *       products above 2^-24 summed in fp32 -- the same error envelope as 5 (measured: equal to 5's against float64),
 *       not the reference's arithmetic operation for operation, and at present SLOWER than 5; H % 8 == 0,
 *       W % 64 == 0.
 * The default comes from the environment variable PNP_DNCNN_WINOGRAD at plan creation (6 as above; unset or any other value = 5,
 * falling back to 1 where the image size does not allow it).  This call rejects any other mode, and 5 / 6 where the image
 * size does not allow them, with PNP_ERR_ARG.                                                                          */
int pnp_dncnn_set_winograd(pnp_dncnn_plan* plan, int enable);
/* raw network: r = net(x), x and r [batch][H][W] fp32 (the predicted noise residual)          */
int pnp_dncnn_forward(pnp_dncnn_plan* plan, const float* x, float* r, void* stream);
/* the whole denoise(): min-max normalise, scale by 1 + sigma_net/255/2, x - net(x), undo both;
 * z_in/z_out/xrec in `dtype` (may alias); sse_out [batch] double = sum (xrec - z_out)^2 or NULL. */
int pnp_dncnn_denoise(pnp_dncnn_plan* plan, const void* z_in, void* z_out, int dtype, double sigma_net,
                      const void* xrec, double* sse_out, void* stream);

/* MMODenoiser.denoise (denoisers/MMODenoise.py:122-128 around apply_model :18-40 and simple_CNN.forward :88-101):
 * z_out = clip(xc + net(xc), 0, 1) with xc = clip(z_in, 0, 1) in fp32.  The reference feeds the TRANSPOSED image
 * (np.moveaxis on a 2-D array); the caller gets the same result by creating the plan with every 3x3 kernel
 * transposed (conv(x^T, w)^T == conv(x, w^T)).  z_in/z_out/xrec in `dtype`; sse_out as in pnp_dncnn_denoise.  */
int pnp_mmo_denoise(pnp_dncnn_plan* plan, const void* z_in, void* z_out, int dtype, const void* xrec,
                    double* sse_out, void* stream);

/* In-band timing of the MFMA conv launches (measurement aid for bench.py): between begin and end
 * every forward/denoise call brackets its n_mid conv launches with hipEvents on the caller's
 * stream (no synchronisation until _end).  _end returns the mean duration of one conv launch.  */
int pnp_dncnn_profile_begin(pnp_dncnn_plan* plan, int max_calls);
int pnp_dncnn_profile_end(pnp_dncnn_plan* plan, double* avg_ms_per_launch, long* launches);
/* Diagnostic (allocates + synchronises; never on the hot path): median in-kernel shader cycles and 100 MHz
 * reference ticks of the conv tile loop after `reps` back-to-back launches -> the clock held under load. */
int pnp_dncnn_debug_clock(pnp_dncnn_plan* plan, int reps, double* cycles, double* ref_ticks, void* stream);
/* Test hooks (never on the hot path): ONE 64->64 layer of the plan's network, kernel as selected by pnp_dncnn_set_winograd, on
 * CALLER-provided activation buffers in/out [batch][64][H][W] fp32 -- so that a test can put guard bands around them
 * (tests/test_gpu_dncnn.py::test_wino44_guard_bands).  w44_override (may be NULL; mode 5 only): packed F(4x4,3x3) weights of
 * the layer in the caller's memory, pnp_dncnn_debug_w44_floats() floats as pnp_dncnn_debug_w44_weights copies them out.
 * w44_rows: 0 = the production choice of region form, 1 / 2 = 4 x 64 / 8 x 64 regions for the whole layer (mode 5 only).
 * pnp_dncnn_debug_w44_weights fails with PNP_ERR_ARG on a plan whose image size rules mode 5 out (no such weights).           */
size_t pnp_dncnn_debug_w44_floats(void);
int pnp_dncnn_debug_w44_weights(pnp_dncnn_plan* plan, int layer, float* dst, void* stream);
int pnp_dncnn_debug_mid_layer(pnp_dncnn_plan* plan, int layer, const float* in, float* out, const float* w44_override,
                              int w44_rows, void* stream);
// the last middle layer with the 64 -> 1 output conv fused in (conv mode 5, ReLU): in [B][64][H][W] -> the 6 x 6 output patch
// of every 4 x 4 block, part [B][H/4][W/4][6][6] (pixel (4 by + py - 1, 4 bx + px - 1)); w44_rows as above
int pnp_dncnn_debug_fused_last(pnp_dncnn_plan* plan, const float* in, float* part, int w44_rows, void* stream);

/* Device-resident step counter and log ring (hipGraph replay of a whole outer iteration: nothing in the graph
 * depends on a host-side step index).  pnp_log_append: log[(*step_dev % n_log)][0..n) = src[0..n).        */
int pnp_counter_add(uint32_t* counter, uint32_t inc, void* stream);
int pnp_log_append(const double* src, int n, double* log, int n_log, const uint32_t* step_dev, void* stream);
/* the same with a log-owned counter that the call also advances: log[(*counter % n_log)] = src; ++*counter          */
int pnp_log_append_inc(const double* src, int n, double* log, int n_log, uint32_t* counter, void* stream);

/* ------------------------------------------------------------------ minibatches over M measurements, SAGA table
 * Problem.select_mb (problems/problem.py:110-117: `np.random.choice(M, size, replace=False)` -> 0/1 indicator) on the
 * device, with the same key / threshold construction as pnp_csmri_draw_thresholds (candidates 0 .. M-1):
 * mbd [nsteps][batch] descriptors; the Deblur gradient consumes a step's descriptors directly (pnp_deblur_grad_mb),
 * or they are expanded to an indicator sel [batch][M] (uint8) / an ascending row list rows [batch][mb] (int32, the
 * form pnp_pr_grad takes).                                                                                */
int pnp_draw_thresholds(int M, int batch, int mb, uint64_t seed, uint32_t step0, int nsteps, const uint32_t* step_dev,
                        void* mbd, void* stream);
int pnp_indicator_from_thresholds(int M, int batch, const void* mbd, uint8_t* sel, void* stream);
/* pnp_draw_thresholds_pp with a population per problem (mixed-scale Deblur batches): the candidates of problem b are
 * 0 .. M_vec[b] - 1 (M_vec: int32 [batch] on the device).  With the same draw_id, mb, seed and step, problem b's descriptor equals,
 * bit for bit, the one pnp_draw_thresholds_pp(M_vec[b], ...) gives.  mb_vec[b] >= M_vec[b] selects every candidate (the front end
 * refuses mb_vec[b] > M_vec[b]); consumers stop at M_b themselves.  seed_vec (uint64 [batch] on the device, or NULL): problem b's
 * stream absorbs seed_vec[b] in place of `seed` -- the items of a sweep keep the streams of the groups they would have run in
 * (sweep.make_runner(mixed_scales=True)).  pnp_indicator_from_thresholds_m: the indicator with row
 * stride Mmax, sel [batch][Mmax], zero for m >= M_vec[b].                                                                   */
int pnp_draw_thresholds_mpp(const int32_t* M_vec, int batch, const int32_t* mb_vec, const uint32_t* draw_id, uint64_t seed,
                            const uint64_t* seed_vec, uint32_t step0, int nsteps, const uint32_t* step_dev, void* mbd, void* stream);
int pnp_indicator_from_thresholds_m(const int32_t* M_vec, int Mmax, int batch, const void* mbd, uint8_t* sel, void* stream);
int pnp_rows_from_thresholds(int M, int batch, int mb, const void* mbd, int32_t* rows, void* stream);
/* indicator from host-drawn index lists (np.random.choice output): idx [batch][n] int32 -> sel [batch][M] uint8   */
int pnp_indicator_from_indices(const int32_t* idx, int n, int M, int batch, uint8_t* sel, void* stream);
/* One SAGA step (algorithms/pnp_saga.py:43-57) in one pass over the vectors (n = batch * N elements):
 *   old = slot; sum += g - old; z -= lr * ((g - prev) + sum * inv_hist); slot = g
 * g = the new minibatch gradient (already / mini_batch_size), slot = the table row being replaced, prev = the row
 * written by the previous step (may be the same row), sum = running sum of the table (== sum(table), :47).   */
int pnp_saga_table_update(void* z, const void* g, void* slot, const void* prev, void* sum, double lr, double inv_hist,
                          size_t n, int dtype, void* stream);
/* The same step for a whole batch in ONE launch when the problems replace different rows or step with different sizes (_pp form):
 * table [hist][batch][N] is the table base, problem b replaces row[b] and its previous step wrote prev_row[b] (int32 [batch] on
 * the device, each in [0, hist); the call does not synchronise and cannot check them: the caller does), and steps with
 * lr_pp ? lr_pp[b] : lr ([batch] doubles on the device, cast to `dtype` as the plain call casts lr).  z, g, sum [batch][N].  Per
 * element the arithmetic and its order are those of pnp_saga_table_update, row[b] == prev_row[b] included (prev is read before the
 * slot is written, by the same thread), so problem b equals, bit for bit, the plain call on its views.  N must be a multiple of 4
 * and the pointers 16-byte aligned (vector loads and stores); PNP_ERR_ARG otherwise.                                  */
int pnp_saga_table_update_pp(void* z, const void* g, void* table, const int32_t* row, const int32_t* prev_row, void* sum,
                             double lr, const double* lr_pp, double inv_hist, int hist, int batch, int N, int dtype,
                             void* stream);
/* pnp_saga_table_update_pp with the divisor per problem: problem b steps with inv_hist_pp ? inv_hist_pp[b] : inv_hist ([batch] doubles
 * on the device, 1 / hist[b], cast to `dtype` as the scalar is cast).  table [hist][batch][N] with hist the LARGEST history length of
 * the batch; row[b], prev_row[b] lie below problem b's own history length (the caller checks them), so rows beyond it are never read
 * or written.  Everything else, the PNP_ERR_ARG cases included, is pnp_saga_table_update_pp's; a NULL inv_hist_pp equals it.      */
int pnp_saga_table_update_hist_pp(void* z, const void* g, void* table, const int32_t* row, const int32_t* prev_row, void* sum,
                                  double lr, const double* lr_pp, double inv_hist, const double* inv_hist_pp, int hist, int batch,
                                  int N, int dtype, void* stream);

/* ------------------------------------------------------------------ elementwise
 * out = a*x + b*y + c*w   (y, w may be NULL); n = total element count.
 * Covers z -= lr*v (pnp_gd.py:35), SAGA/SARAH combines (pnp_saga.py:47, pnp_sarah.py:72). */
int pnp_axpbypcz(double a, const void* x, double b, const void* y, double c, const void* w,
                 void* out, size_t n, int dtype, void* stream);
/* The same combine with per-problem coefficients (_pp form), ONE launch for a batch: n = total element count, problem p owns the
 * elements [p * n / batch, (p + 1) * n / batch) and takes a_pp ? a_pp[p] : a (likewise b, c): [batch] doubles on the device, each
 * cast to `dtype` once, as the plain call casts its scalar.  All three arrays NULL is the plain call.  Per element the arithmetic
 * and its order are those of pnp_axpbypcz (y, w may be NULL), so problem p equals, bit for bit, the plain call on its views.
 * 16 bytes per lane when x, y, w, out are 16-byte aligned and n / batch elements are a multiple of 16 bytes; any other views
 * (offset by one element, odd lengths) take an element-by-element path.  out may alias x, y or w EXACTLY (every thread loads all
 * operands of its elements before it stores them); partially overlapping operands are not supported.
 * PNP_ERR_ARG before any device work: NULL x or out, batch <= 0, n % batch != 0, an unknown dtype.                     */
int pnp_axpbypcz_pp(double a, const double* a_pp, const void* x, double b, const double* b_pp, const void* y,
                    double c, const double* c_pp, const void* w, void* out, size_t n, int batch, int dtype, void* stream);

/* The outer refresh of the SVRG loop -- algorithms/pnp_svrg.py:32-38 -- where every problem has a T2 of its own, ONE launch for a batch of
 * any kind: for every problem p with step % t2_vec[p] == 0:  mu[p] = mu_new[p], w[p] = z[p]; the other problems' mu and w are
 * neither written nor read.  n = total element count, problem p owns [p * n / batch, (p + 1) * n / batch); t2_vec: int32 [batch]
 * on the device (entries >= 1: the front end checks its host copy; an entry below 1 counts as 1); step: the host's step index.
 * 16 bytes per lane when the four arrays are 16-byte aligned and n / batch elements are a multiple of 16 bytes, else element by
 * element.  PNP_ERR_ARG before any device work: a NULL pointer, batch <= 0, n % batch != 0, an unknown dtype, step < 0, mu_new
 * aliasing mu (or w aliasing any of the other three, or z aliasing mu).                                                    */
int pnp_refresh_pp(const void* mu_new, const void* z, void* mu, void* w, const int32_t* t2_vec, int step, size_t n, int batch,
                   int dtype, void* stream);

/* The outer step of the SARAH loop -- algorithms/pnp_sarah.py:40-50 -- where every problem has a T2 of its own, ONE launch for a batch
 * of any kind: the engine makes the outer step for the whole batch into a scratch, and for every problem p with
 * step % t2_vec[p] == 0 this call adopts it: dst[p] = src[p], row_out[p] = row_in[p] (the squared error of that prox).  For every other
 * problem dst[p] is neither read nor written and row_out[p] = NaN ("no outer step here": the device writes it, so a wrapping log ring
 * needs no host fill).  row_in and row_out: double [batch], both or neither NULL.  n = total element count, problem p owns
 * [p * n / batch, (p + 1) * n / batch); t2_vec: int32 [batch] on the device (entries >= 1: the front end checks its host copy; an
 * entry below 1 counts as 1); step: the host's step index.  16 bytes per lane when src and dst are 16-byte aligned and n / batch
 * elements are a multiple of 16 bytes, else element by element.  PNP_ERR_ARG before any device work: NULL src, dst or t2_vec, only
 * one of row_in / row_out NULL, batch <= 0, n % batch != 0, an unknown dtype, step < 0, dst aliasing src.                  */
int pnp_select_pp(const void* src, void* dst, const double* row_in, double* row_out, const int32_t* t2_vec, int step, size_t n,
                  int batch, int dtype, void* stream);

/* ------------------------------------------------------------------ the data-fidelity objective f(z), per problem
 * f = || Y - forward_model(z) ||^2 / 2 / M (problems/CSMRI.py:61-64 with M = N, DeblurSR.py:114-117 with M = lrH * lrW, PR.py:70-73
 * with M = num_meas): the forward passes of the gradients ending in a per-problem reduction -- no inverse / adjoint pass and no
 * image write.  All three write f_out [batch] doubles = scale * (sum of squared residuals); the host passes scale = 1 / (2 M).
 * The sums are taken in double whatever `dtype`, in a fixed order and without atomics: a problem's value depends neither on the
 * batch size nor on its index in the batch.  Nothing is allocated and nothing synchronises (scratch: the plans' own workspaces,
 * the caller's for PR), so the calls may be captured.  PNP_ERR_ARG before any device work: a NULL pointer, batch <= 0, a bad dtype.
 *
 * CSMRI: sum over the FULL spectrum of mask(k) |fft2(z)(k) - Y(k)|^2 (the mask need not be Hermitian, so the packed yh of
 *   pnp_csmri_pack_y is not enough): YT [batch][W][H] complex, bitsT [batch][W][H/32] the bit-packed mask.  Entries of YT outside
 *   the mask are not read into the sum.  Uses the plan's half-spectrum workspace, like pnp_csmri_grad_sel.                       */
int pnp_csmri_objective(pnp_csmri_plan* plan, const void* z, const void* YT, const uint32_t* bitsT, double scale, double* f_out,
                        void* stream);
/* Deblur: sum over the M measurements of (S B z - Y)^2; z [batch][N], Y [batch][M].  Uses the plan's scratch, like pnp_deblur_grad. */
int pnp_deblur_objective(pnp_deblur_plan* plan, const void* z, const void* Y, double scale, double* f_out, void* stream);
/* PR: sum over the M rows of (|A w| - y)^2, A streamed once with 16-byte loads (any M, N; N % (16 / sizeof) != 0 takes scalar
 *   loads).  w [batch][N], y [batch][M]; A [n_mat][M][N] with n_mat == batch (every problem its own matrix) or a divisor of batch
 *   (the tiled batches of pnp_pr_grad_shared: problem b works on A[b % n_mat]).  workspace: pnp_pr_objective_workspace_bytes(M,
 *   batch) bytes, 8-byte aligned.                                                                                              */
size_t pnp_pr_objective_workspace_bytes(int M, int batch);
int pnp_pr_objective(const void* A, const void* w, const void* y, int M, int N, int batch, int n_mat, int dtype, double scale,
                     void* workspace, double* f_out, void* stream);

/* ------------------------------------------------------------------ host: the legacy RNG draw of select_mb
 * np.random.choice(pool, size, replace=False) (problems/CSMRI.py:72, problems/problem.py:114) on the legacy MT19937 stream,
 * restated in C (no device work): out[k] = pool[perm[k]] (pool NULL: perm[k]) for the first `size` entries of
 * permutation(pop).  mt_key [624] / *mt_pos are the stream's state as np.random.get_state() returns it and are advanced
 * exactly as NumPy advances them; work: [pop] scratch.                                                               */
int pnp_legacy_choice(uint32_t* mt_key, int* mt_pos, const int64_t* pool, int pop, int size, int32_t* work, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* PNP_HIP_H */

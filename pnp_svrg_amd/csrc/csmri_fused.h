// csmri_fused.h -- the launchers of csmri_fused.hip (the one-kernel CSMRI iterations) as csmri.hip's entry points call them: the one
// declaration of each, with its default arguments (what each launches: at its definition).  The launchers make the HIP calls; the entry
// points own the argument checks (every answer to a bad argument is given before the first HIP call).
#pragma once
#include <cstdint>

namespace pnp {

// MODE of the one-kernel iteration: 0 = the whole iteration; 1 = stop after the noise estimate and store the stepped image (another
//       prox follows); 2 = the gradient only (phases 1-3: grad_full with its data term, or any other use of pnp_csmri_grad_sel that
//       fits this kernel); 3 = the whole iteration with the 2-D wavelet prox (csmri_fused_w2d.h) in place of the per-column one.
enum { FUSED_FULL = 0, FUSED_NO_DENOISE = 1, FUSED_GRAD = 2, FUSED_FULL_W2D = 3 };

int csmri_fused_launch(int batch, const void* twtab, const void* a, const void* b, const uint32_t* bitsT, const void* yh,
                       double alpha, const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2, void* out,
                       int mode, double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out,
                       void* stream, void* w_out = nullptr, void* mu_out = nullptr, const double* alpha_pp = nullptr,
                       const double* gamma_pp = nullptr, const double* sm_pp = nullptr);
int csmri_fused_outer_launch(int batch, const void* twtab, void* z, void* w, void* mu, const uint32_t* mask_bits, const void* yh,
                             const void* alpha_vec, const uint32_t* selbits, int T2, double lr, int mini_batch_size,
                             double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_log, int log_row0, int n_log,
                             void* sigma_out, void* stream, const double* lr_pp = nullptr, const int32_t* mb_vec = nullptr,
                             const double* sm_pp = nullptr);
int csmri_fused_outer_w2d_launch(int batch, const void* twtab, void* z, void* w, void* mu, const uint32_t* mask_bits, const void* yh,
                                 const void* alpha_vec, const uint32_t* selbits, int T2, double lr, const double* lr_pp,
                                 int mini_batch_size, const int32_t* mb_vec, double sigma_modifier, const double* sm_pp,
                                 double fallback_sigma, const void* xrec, double* sse_log, int log_row0, int n_log, void* sigma_out,
                                 void* stream);
int csmri_fused_span_launch(int batch, const void* twtab, void* z, void* w, void* mu, const uint32_t* mask_bits, const void* yh,
                            const void* alpha_vec, const uint32_t* selbits, int step0, int n_steps, int T2, const int32_t* t2_vec,
                            double lr, const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                            const double* sm_pp, double fallback_sigma, const void* xrec, double* sse_log, int log_row0, int n_log,
                            void* sigma_out, void* stream);
int csmri_sarah_launch(int batch, const void* twtab, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                       const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2, void* v_out, void* out,
                       void* out2, int mode, double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_out,
                       void* sigma_out, void* stream, const double* alpha_pp, const double* gamma_pp, const double* sm_pp);
int csmri_sarah_outer_launch(int batch, const void* twtab, void* z, void* w_prev, void* w_next, void* v_prev, const uint32_t* mask_bits,
                             const void* yh, const void* alpha_vec, const uint32_t* selbits, int T2, double eta, const double* eta_pp,
                             double lr, const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                             const double* sm_pp, double fallback_sigma, const void* xrec, double* sse_log, int log_row0, int n_log,
                             void* sigma_out, void* stream);
int csmri_sarah_span_launch(int batch, const void* twtab, void* z, void* w_prev, void* w_next, void* v_prev, const uint32_t* mask_bits,
                            const void* yh, const void* alpha_vec, const uint32_t* selbits, int step0, int n_steps, int T2,
                            const int32_t* t2_vec, double eta, const double* eta_pp, double lr, const double* lr_pp, int mini_batch_size,
                            const int32_t* mb_vec, double sigma_modifier, const double* sm_pp, double fallback_sigma, const void* xrec,
                            double* sse_log, double* outer_log, int log_row0, int n_log, void* sigma_out, void* stream);
int csmri_step_span_launch(int batch, const void* twtab, void* z, const uint32_t* bits, const void* yh, const void* YT, double alpha,
                           const void* alpha_vec, double beta, void* table, const int32_t* rows, const int32_t* prev_row0, void* sum,
                           double lr, double inv_hist, int n_steps, double sigma_modifier, double fallback_sigma, const void* xrec,
                           double* sse_log, int log_row0, int n_log, void* sigma_out, void* stream, const double* alpha_pp,
                           const double* lr_pp, const double* sm_pp);
int csmri_minibatch_launch(int batch, const void* twtab, const void* a, const uint32_t* bitsT, const void* YT, double alpha,
                           const void* alpha_vec, double beta, const void* c1, void* table, const int32_t* row, const int32_t* prev_row,
                           void* sum, double lr, double inv_hist, void* out, int mode, double sigma_modifier, double fallback_sigma,
                           const void* xrec, double* sse_out, void* sigma_out, void* stream, const double* alpha_pp, const double* lr_pp,
                           const double* sm_pp);
int csmri_saga_hist_launch(int batch, const void* twtab, const void* a, const uint32_t* bitsT, const void* YT, double alpha,
                           const void* alpha_vec, void* table, const int32_t* row, const int32_t* prev_row, void* sum, double lr,
                           double inv_hist, void* out, int mode, double sigma_modifier, double fallback_sigma, const void* xrec,
                           double* sse_out, void* sigma_out, void* stream, const double* alpha_pp, const double* lr_pp, const double* sm_pp,
                           const double* inv_hist_pp, int n_steps, int log_row0, int n_log);

}  // namespace pnp

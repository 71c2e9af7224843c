// deblur_plan.h -- the Deblur plan's state (deblur.hip owns it; setup_generate.hip reads its sizes; deblur_mixed.hip adds the
// mixed-scale state behind it).
#pragma once
#include <cstdint>

// One problem of a mixed-scale plan: its measurement count and where its down-sampler's tables start in the plan's concatenated
// arrays (taps in rows of 4, row pointers and CSR entries in elements).  ident: the identity set (M == N, no tables).
struct pnp_deblur_mixed_prob {
    int32_t M, ident, g_base, rp_base, nz_base;
};

struct pnp_deblur_plan {
    int n, N, NL, batch, dtype, M;            // N = n*n = H*W; M = number of measurements
    void *tw_line, *tw_big, *FB;              // [n], [N], [N] complex
    void *w0, *r0, *r1;                       // complex [batch][N]; real [batch][N] x2
    // optional bilinear operator
    int32_t *g_idx, *a_rowptr, *a_col;
    void *g_w, *a_val, *down;                 // [M][4], [nnz], real [batch][M]
    // mixed-scale plans (pnp_deblur_plan_create_mixed, deblur_mixed.hip): n_sets > 0 distinct down-samplers, problem b works on the
    // tables mx_prob[b] points to; M = Mmax = max M_b, `down` is [batch][Mmax], the five arrays above hold the concatenated sets.
    // A plan of pnp_deblur_plan_create has n_sets == 0 and mx_prob == nullptr.
    int n_sets;
    pnp_deblur_mixed_prob* mx_prob;           // device [batch]
    int32_t* mx_M;                            // device [batch]: M_b (what the draw and indicator kernels take)
};

namespace pnp {
// One blur of all the plan's problems through the FFT passes of deblur.hip (k_colpass -> k_rowpass -> k_colpass), for the callers
// outside that file: out = (dtype)alpha * (x (*) kernel, or its adjoint when conj_kernel), with alpha_pp != nullptr problem b takes
// (dtype)(alpha_pp[b] / alpha_div) instead -- the launches and arguments of the two blurs of a gradient with a down-sampler.
int deblur_blur(pnp_deblur_plan* p, const void* x, bool conj_kernel, double alpha, void* out, void* stream,
                const double* alpha_pp, double alpha_div);
}

// deblur_plan.h -- the Deblur plan's state (deblur.hip owns it; setup_generate.hip reads its sizes).
#pragma once
#include <cstdint>

struct pnp_deblur_plan {
    int n, N, NL, batch, dtype, M;            // N = n*n = H*W; M = number of measurements
    void *tw_line, *tw_big, *FB;              // [n], [N], [N] complex
    void *w0, *r0, *r1;                       // complex [batch][N]; real [batch][N] x2
    // optional bilinear operator
    int32_t *g_idx, *a_rowptr, *a_col;
    void *g_w, *a_val, *down;                 // [M][4], [nnz], real [batch][M]
};

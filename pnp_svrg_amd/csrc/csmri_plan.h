// csmri_plan.h -- the CSMRI plan behind the opaque pnp_csmri_plan of include/pnp_hip.h (created and destroyed in
// csmri.hip; csmri_setup.hip runs the problem generator on it).
#pragma once

struct pnp_csmri_plan {
    int H, W, batch, dtype, NL;              // NL: 16 -> N = 256, 8 -> N = 64, 12 -> N = 128 (8 x 16 split)
    void* work;     // [batch][W/2][H] complex
    void* twtab;    // [N] complex
    void* mbd;      // [batch] MbDesc scratch of pnp_csmri_draw_minibatch
    int fused_min_batch;   // batches at least this large take the one-kernel gradient (env PNP_CSMRI_FUSED_MIN_BATCH)
};

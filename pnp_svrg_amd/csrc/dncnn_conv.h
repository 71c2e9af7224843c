// dncnn_conv.h -- the interface of the 64 -> 64 conv forms of the DnCNN plan (direct.h, wino44.h, wino44b.h): every form exports
// the functions of one ConvMode row of the mode table in dncnn.hip.
#pragma once
#include "common.h"
#include <vector>

namespace pnp {

struct ConvLayerArgs {
    const float* in;                        // [batch][64][H][W]
    float* out;                             // the same
    const void* w;                          // the form's packed weights of all layers (ConvMode::pack) ...
    int layer;                              // ... and which of them
    const float *bias, *zeros;              // [64] of this layer; a zero word (halo padding)
    int H, W, batch, num_cu;
    float slope;                            // LeakyReLU slope, 0 = ReLU
    hipStream_t s;
    // mode 5 only (wino44.h); the other forms reject w44_override and part, and ignore force_rows
    int force_rows = 0;                     // test hook: 1 / 2 = 4 x 64 / 8 x 64 regions for the whole layer
    const float* w44_override = nullptr;    // test hook: this layer's packed weights in the caller's memory
    const float* wlast = nullptr;           // the fused 64 -> 1 output conv: its weights [64][3][3],
    float* part = nullptr;                  // its output patches
};

struct ConvMode {
    int mode;                                                    // pnp_dncnn_set_winograd / PNP_DNCNN_WINOGRAD
    bool (*supports)(int H, int W);                              // image sizes the form runs on
    size_t (*layer_bytes)();                                     // packed weights of one layer
    void (*pack)(const float* w_mid, int n_mid, void* out);      // w_mid [n_mid][64][64][3][3] (BN folded) -> host buffer
    int (*layer)(const ConvLayerArgs& a);
    // diagnostic: `reps` back-to-back launches of a layer, the last one stamped -> per workgroup the shader cycles and 100 MHz
    // ticks of the tile loop; PNP_DEBUG_STAMPS=1 prints the form's own breakdown of them
    int (*debug_clock)(const ConvLayerArgs& a, int reps, std::vector<double>& cycles, std::vector<double>& ticks);
    bool fuses_last;                                             // can run the 64 -> 1 output conv in the last layer's epilogue
};

// ConvMode::layer of a form without the mode 5 extras
inline int check_plain_conv(const ConvLayerArgs& a) {
    PNP_CHECK_ARG(a.w44_override == nullptr, "w44_override needs the F(4x4,3x3) kernel (mode 5)");
    PNP_CHECK_ARG(a.part == nullptr, "the fused last layer needs the F(4x4,3x3) kernel (mode 5) and ReLU");
    return PNP_OK;
}

// ConvMode::debug_clock plumbing: launch(stamps_dev) issues the launches on s, the stamped one writing `per_wg` 64-bit values
// {shader cycles, 100 MHz ticks, ...} for each of `nwg` workgroups -> all of them in h, the first two in cycles / ticks
template <typename F>
int read_stamps(hipStream_t s, int nwg, int per_wg, F&& launch, std::vector<unsigned long long>& h, std::vector<double>& cycles,
                std::vector<double>& ticks) {
    unsigned long long* d = nullptr;
    PNP_CHECK_HIP(hipMalloc(&d, (size_t)nwg * per_wg * sizeof(*d)));
    h.resize((size_t)nwg * per_wg);
    const int rc = launch(d);
    hipError_t e = rc != PNP_OK ? hipSuccess : hipMemcpyAsync(h.data(), d, h.size() * sizeof(*d), hipMemcpyDeviceToHost, s);
    if (rc == PNP_OK && e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (rc != PNP_OK) return rc;
    PNP_CHECK_HIP(e);
    for (int i = 0; i < nwg; ++i) { cycles.push_back((double)h[(size_t)per_wg * i]); ticks.push_back((double)h[(size_t)per_wg * i + 1]); }
    return PNP_OK;
}

}  // namespace pnp

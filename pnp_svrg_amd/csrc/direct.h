// direct.h -- host entry points of the direct (conv mode 0) and Winograd F(2,3) (conv mode 1) conv layers (dncnn_direct.hip),
// used by the DnCNN plan through the interface of dncnn_conv.h.
#pragma once
#include "dncnn_conv.h"

namespace pnp {
bool direct_supports(int H, int W);                                          // H % 8 == 0 and W % 32 == 0: every DnCNN plan
size_t direct_layer_bytes();
void direct_pack(const float* w_mid, int n_mid, void* out);                 // MFMA (16x16x4) register order
int direct_layer(const ConvLayerArgs& a);
int direct_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& cycles, std::vector<double>& ticks);
size_t wino23_layer_bytes();                                                 // (supports: direct_supports)
void wino23_pack(const float* w_mid, int n_mid, void* out);                 // U = G g along x
int wino23_layer(const ConvLayerArgs& a);
int wino23_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& cycles, std::vector<double>& ticks);
}  // namespace pnp

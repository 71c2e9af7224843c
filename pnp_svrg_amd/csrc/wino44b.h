// wino44b.h -- host entry points of the 3 x bf16 split F(4x4,3x3) Winograd conv layer (dncnn_wino44b.hip), used by the DnCNN plan
// through the interface of dncnn_conv.h (conv mode 6: opt-in, fp32-class accuracy on the bf16 matrix cores; not the reference's
// arithmetic operation for operation).
#pragma once
#include "dncnn_conv.h"

namespace pnp {
bool wino44b_supports(int H, int W);                                         // H % 8 == 0 and W % 64 == 0
size_t wino44b_layer_bytes();
void wino44b_pack(const float* w_mid, int n_mid, void* out);                // U = G g G^T, split in three (bf16 bit patterns)
int wino44b_layer(const ConvLayerArgs& a);
int wino44b_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& cycles, std::vector<double>& ticks);
}  // namespace pnp

// wino44.h -- host entry points of the F(4x4,3x3) Winograd conv layer (dncnn_wino44.hip, conv mode 5), used by the DnCNN plan
// through the interface of dncnn_conv.h.
#pragma once
#include "dncnn_conv.h"

namespace pnp {
bool wino44_supports(int H, int W);                                          // H % 8 == 0 and W % 64 == 0
size_t wino44_layer_bytes();
void wino44_pack(const float* w_mid, int n_mid, void* out);                 // U = G g G^T
// a.force_rows 1 / 2 and a.w44_override: test hooks only.  a.part != nullptr (ReLU only): the DnCNN's 64 -> 1 output conv
// (weights a.wlast [64][3][3]) fused into this layer -- `out` is left alone and every 4 x 4 block writes the 6 x 6 patch of
// output partials its activations feed, part[b][by][bx][6][6] (wino44_part_floats), pixel (4 by + py - 1, 4 bx + px - 1)
int wino44_layer(const ConvLayerArgs& a);
inline size_t wino44_part_floats(int H, int W, int batch) { return (size_t)batch * (H / 4) * (W / 4) * 36; }
int wino44_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& cycles, std::vector<double>& ticks);
}  // namespace pnp

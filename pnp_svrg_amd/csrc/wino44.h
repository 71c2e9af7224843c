// wino44.h -- host entry points of the F(4x4,3x3) Winograd conv layer (dncnn_wino44.hip), used by the DnCNN plan.
#pragma once
#include "common.h"

namespace pnp {
bool wino44_supports(int H, int W);                                          // H % 8 == 0 and W % 64 == 0
size_t wino44_weight_floats(int n_mid);
void wino44_pack_weights(const float* w_mid, int n_mid, float* out);         // host -> host buffer (U = G g G^T)
// force_rows 1 / 2: test hook only.  part != nullptr (ReLU only): the DnCNN's 64 -> 1 output conv (weights wlast [64][3][3])
// fused into this layer -- `out` is left alone and every 4 x 4 block writes the 6 x 6 patch of output partials its
// activations feed, part[b][by][bx][6][6] (wino44_part_floats), pixel (4 by + py - 1, 4 bx + px - 1)
int wino44_layer(const float* in, float* out, const float* upack_layer, const float* bias, const float* zeros, int H, int W,
                 int batch, int num_cu, float slope, hipStream_t s, int force_rows = 0, const float* wlast = nullptr,
                 float* part = nullptr);
inline size_t wino44_part_floats(int H, int W, int batch) { return (size_t)batch * (H / 4) * (W / 4) * 36; }
int wino44_debug_clock(const float* in, float* out, const float* upack_layer, const float* bias, int H, int W, int batch,
                       int num_cu, int reps, unsigned long long* stamps_dev, hipStream_t s);   // 4 values per workgroup
}  // namespace pnp

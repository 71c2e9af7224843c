// select_pp.hip -- the outer step of pnp_sarah for a batch whose problems take it at steps of their own (pnp_select_pp):
//
//     for every problem p with step % t2_vec[p] == 0:   dst[p] = src[p];  row_out[p] = row_in[p]
//     for every other problem p:                        row_out[p] = NaN   (dst[p] neither read nor written)
//
// algorithms/pnp_sarah.py:40-50 (w_next = prox(w_prev - eta * v_prev), logged) with T2 per problem: the engine runs the outer step
// for the whole batch into a scratch and this ONE launch adopts it -- the image and its squared error -- where a problem's own outer
// iteration begins.  The NaN marks "no outer step here" in the engine's second log ring; the device writes it, so a wrapping ring
// needs no host fill.  A translation unit of its own, as refresh_pp.hip: no existing kernel is recompiled from other text.  Pure
// copies: the arithmetic of nothing changes.
#include "common.h"

#include <cmath>

namespace pnp {

template <typename T> struct SelectVec;
template <> struct SelectVec<float> { using type = float4; };
template <> struct SelectVec<double> { using type = double2; };

// blockIdx.y strides over the problems, blockIdx.x grid-strides over one problem's elements (refresh_pp.hip's geometry).  Whether
// a problem adopts is wave-uniform: one plain load of t2_vec[p] per workgroup and problem; an entry below 1 counts as 1.  The
// log entry of a problem is written by one lane of its first workgroup.
// VEC: 16 bytes per lane (both pointers 16-byte aligned, len * sizeof(T) a multiple of 16); else element by element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_select_pp(const T* __restrict__ src, T* __restrict__ dst, const double* __restrict__ row_in,
                                                   double* __restrict__ row_out, const int32_t* __restrict__ t2_vec, int step,
                                                   size_t len, int batch) {
    using V = typename SelectVec<T>::type;
    constexpr int NV = (int)(sizeof(V) / sizeof(T));
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (int p = blockIdx.y; p < batch; p += gridDim.y) {
        int t2 = t2_vec[p];
        if (t2 < 1) t2 = 1;
        const bool take = step % t2 == 0;
        if (row_out != nullptr && first == 0) row_out[p] = take ? row_in[p] : (double)NAN;
        if (!take) continue;
        const size_t base = (size_t)p * len;
        if (VEC) {
            const size_t nvec = len / NV;
            for (size_t i = first; i < nvec; i += stride) {
                const size_t e = base + i * NV;
                *(V*)(dst + e) = *(const V*)(src + e);
            }
        } else {
            for (size_t i = first; i < len; i += stride) dst[base + i] = src[base + i];
        }
    }
}

template <typename T>
static void launch_select_pp(const void* src, void* dst, const double* row_in, double* row_out, const int32_t* t2_vec, int step,
                             size_t len, int batch, hipStream_t s) {
    constexpr size_t NV = 16 / sizeof(T);
    const uintptr_t ptrs = (uintptr_t)src | (uintptr_t)dst;
    const bool vec = (ptrs & 15) == 0 && len % NV == 0;
    const size_t units = vec ? len / NV : len;
    // capped grid, as pnp_refresh_pp's: about 4096 workgroups in all, at least one per problem row of the grid (also when len == 0:
    // the log entries are still due)
    const unsigned gy = batch < 65535 ? (unsigned)batch : 65535u;
    const size_t cap = 4096 / gy > 0 ? 4096 / gy : 1, need = units > 0 ? (units + 255) / 256 : 1;
    const dim3 grid((unsigned)(need < cap ? need : cap), gy);
    if (vec)
        k_select_pp<T, true><<<grid, 256, 0, s>>>((const T*)src, (T*)dst, row_in, row_out, t2_vec, step, len, batch);
    else
        k_select_pp<T, false><<<grid, 256, 0, s>>>((const T*)src, (T*)dst, row_in, row_out, t2_vec, step, len, batch);
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_select_pp(const void* src, void* dst, const double* row_in, double* row_out, const int32_t* t2_vec, int step,
                             size_t n, int batch, int dtype, void* stream) {
    PNP_CHECK_ARG(src && dst && t2_vec, "null argument");
    PNP_CHECK_ARG((row_in == nullptr) == (row_out == nullptr), "row_in and row_out: both or neither");
    PNP_CHECK_ARG(batch > 0, "need batch >= 1");
    PNP_CHECK_ARG(n % (size_t)batch == 0, "n must be a multiple of batch");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    PNP_CHECK_ARG(step >= 0, "need step >= 0");
    PNP_CHECK_ARG(src != dst, "dst must not alias src");
    if (n == 0 && row_out == nullptr) return PNP_OK;
    if (dtype == PNP_F32)
        launch_select_pp<float>(src, dst, row_in, row_out, t2_vec, step, n / batch, batch, (hipStream_t)stream);
    else
        launch_select_pp<double>(src, dst, row_in, row_out, t2_vec, step, n / batch, batch, (hipStream_t)stream);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

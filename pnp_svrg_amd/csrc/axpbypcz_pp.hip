// axpbypcz_pp.hip -- the elementwise combine out = a*x + b*y + c*w with per-problem coefficients (pnp_axpbypcz_pp).
//
// A translation unit of its own (built with -ffp-contract=off like prox.hip, where the scalar kernel k_axpbypcz lives): no existing
// kernel is recompiled from other text.  Per element the statements are k_axpbypcz's, in its order, each product and sum rounded on
// its own:  v = a*x[i]; if (y) v += b*y[i]; if (w) v += c*w[i];  -- so problem p equals, bit for bit, the plain call on its views
// with (T)coef[p], the one cast from the double that the plain call applies to its scalar.
#include "common.h"

namespace pnp {

template <typename T> struct CombineVec;
template <> struct CombineVec<float> { using type = float4; };
template <> struct CombineVec<double> { using type = double2; };

// blockIdx.y strides over the problems (a batch may exceed the y limit of a grid), blockIdx.x grid-strides over one problem's
// elements.  A coefficient is wave-uniform: one plain load per workgroup and problem.
// VEC: 16 bytes per lane (every pointer 16-byte aligned, len * sizeof(T) a multiple of 16); else element by element with bounds.
// x, y, w, out carry no __restrict__: out may alias any of them exactly.  A thread loads all operands of its elements before it
// stores them, and no other thread touches those elements.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_axpbypcz_pp(T a, const double* __restrict__ a_pp, const T* x, T b,
                                                     const double* __restrict__ b_pp, const T* y, T c,
                                                     const double* __restrict__ c_pp, const T* w, T* out, size_t len, int batch) {
    using V = typename CombineVec<T>::type;
    constexpr int NV = (int)(sizeof(V) / sizeof(T));
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (int p = blockIdx.y; p < batch; p += gridDim.y) {
        const T ap = a_pp != nullptr ? (T)a_pp[p] : a;
        const T bp = b_pp != nullptr ? (T)b_pp[p] : b;
        const T cp = c_pp != nullptr ? (T)c_pp[p] : c;
        const size_t base = (size_t)p * len;
        if (VEC) {
            const size_t nvec = len / NV;
            for (size_t i = first; i < nvec; i += stride) {
                const size_t e = base + i * NV;
                V xv = *(const V*)(x + e), yv = xv, wv = xv;
                if (y != nullptr) yv = *(const V*)(y + e);
                if (w != nullptr) wv = *(const V*)(w + e);
                T* xa = (T*)&xv; const T* ya = (const T*)&yv; const T* wa = (const T*)&wv;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    T v = ap * xa[k];
                    if (y != nullptr) v += bp * ya[k];
                    if (w != nullptr) v += cp * wa[k];
                    xa[k] = v;
                }
                *(V*)(out + e) = xv;
            }
        } else {
            for (size_t i = first; i < len; i += stride) {
                T v = ap * x[base + i];
                if (y != nullptr) v += bp * y[base + i];
                if (w != nullptr) v += cp * w[base + i];
                out[base + i] = v;
            }
        }
    }
}

template <typename T>
static void launch_axpbypcz_pp(double a, const double* a_pp, const void* x, double b, const double* b_pp, const void* y, double c,
                               const double* c_pp, const void* w, void* out, size_t len, int batch, hipStream_t s) {
    constexpr size_t NV = 16 / sizeof(T);
    const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)y | (uintptr_t)w | (uintptr_t)out;     // (NULL y, w: no bits)
    const bool vec = (ptrs & 15) == 0 && len % NV == 0;
    const size_t units = vec ? len / NV : len;
    // capped grid, as the plain kernel's: about 4096 workgroups in all, at least one per problem row of the grid
    const unsigned gy = batch < 65535 ? (unsigned)batch : 65535u;
    const size_t cap = 4096 / gy > 0 ? 4096 / gy : 1, need = (units + 255) / 256;
    const dim3 grid((unsigned)(need < cap ? need : cap), gy);
    if (vec)
        k_axpbypcz_pp<T, true><<<grid, 256, 0, s>>>((T)a, a_pp, (const T*)x, (T)b, b_pp, (const T*)y, (T)c, c_pp, (const T*)w, (T*)out, len, batch);
    else
        k_axpbypcz_pp<T, false><<<grid, 256, 0, s>>>((T)a, a_pp, (const T*)x, (T)b, b_pp, (const T*)y, (T)c, c_pp, (const T*)w, (T*)out, len, batch);
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_axpbypcz_pp(double a, const double* a_pp, const void* x, double b, const double* b_pp, const void* y,
                               double c, const double* c_pp, const void* w, void* out, size_t n, int batch, int dtype,
                               void* stream) {
    PNP_CHECK_ARG(x && out, "null argument");
    PNP_CHECK_ARG(batch > 0, "need batch >= 1");
    PNP_CHECK_ARG(n % (size_t)batch == 0, "n must be a multiple of batch");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    if (n == 0) return PNP_OK;
    if (dtype == PNP_F32)
        launch_axpbypcz_pp<float>(a, a_pp, x, b, b_pp, y, c, c_pp, w, out, n / batch, batch, (hipStream_t)stream);
    else
        launch_axpbypcz_pp<double>(a, a_pp, x, b, b_pp, y, c, c_pp, w, out, n / batch, batch, (hipStream_t)stream);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

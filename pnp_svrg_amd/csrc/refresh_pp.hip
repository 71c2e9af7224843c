// refresh_pp.hip -- the outer refresh of pnp_svrg for a batch whose problems refresh at steps of their own (pnp_refresh_pp):
//
//     for every problem p with step % t2_vec[p] == 0:   mu[p] = mu_new[p];  w[p] = z[p]
//
// algorithms/pnp_svrg.py:32-38 (mu = grad_full(z); w = copy(z)) with T2 per problem: the engine runs grad_full for the whole batch
// into a scratch mu_new and this ONE launch adopts it where a problem's own outer iteration begins.  The other problems' mu and w
// are neither written nor read.  A translation unit of its own, as axpbypcz_pp.hip: no existing kernel is recompiled from other
// text.  Pure copies: the arithmetic of nothing changes.
#include "common.h"

namespace pnp {

template <typename T> struct RefreshVec;
template <> struct RefreshVec<float> { using type = float4; };
template <> struct RefreshVec<double> { using type = double2; };

// blockIdx.y strides over the problems, blockIdx.x grid-strides over one problem's elements (axpbypcz_pp.hip's geometry).  Whether
// a problem refreshes is wave-uniform: one plain load of t2_vec[p] per workgroup and problem; an entry below 1 counts as 1.
// VEC: 16 bytes per lane (every pointer 16-byte aligned, len * sizeof(T) a multiple of 16); else element by element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_refresh_pp(const T* __restrict__ mu_new, const T* __restrict__ z, T* __restrict__ mu,
                                                    T* __restrict__ w, const int32_t* __restrict__ t2_vec, int step, size_t len,
                                                    int batch) {
    using V = typename RefreshVec<T>::type;
    constexpr int NV = (int)(sizeof(V) / sizeof(T));
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (int p = blockIdx.y; p < batch; p += gridDim.y) {
        int t2 = t2_vec[p];
        if (t2 < 1) t2 = 1;
        if (step % t2 != 0) continue;
        const size_t base = (size_t)p * len;
        if (VEC) {
            const size_t nvec = len / NV;
            for (size_t i = first; i < nvec; i += stride) {
                const size_t e = base + i * NV;
                const V m = *(const V*)(mu_new + e), zv = *(const V*)(z + e);
                *(V*)(mu + e) = m;
                *(V*)(w + e) = zv;
            }
        } else {
            for (size_t i = first; i < len; i += stride) {
                const T m = mu_new[base + i], zv = z[base + i];
                mu[base + i] = m;
                w[base + i] = zv;
            }
        }
    }
}

template <typename T>
static void launch_refresh_pp(const void* mu_new, const void* z, void* mu, void* w, const int32_t* t2_vec, int step, size_t len,
                              int batch, hipStream_t s) {
    constexpr size_t NV = 16 / sizeof(T);
    const uintptr_t ptrs = (uintptr_t)mu_new | (uintptr_t)z | (uintptr_t)mu | (uintptr_t)w;
    const bool vec = (ptrs & 15) == 0 && len % NV == 0;
    const size_t units = vec ? len / NV : len;
    // capped grid, as pnp_axpbypcz_pp's: about 4096 workgroups in all, at least one per problem row of the grid
    const unsigned gy = batch < 65535 ? (unsigned)batch : 65535u;
    const size_t cap = 4096 / gy > 0 ? 4096 / gy : 1, need = (units + 255) / 256;
    const dim3 grid((unsigned)(need < cap ? need : cap), gy);
    if (vec)
        k_refresh_pp<T, true><<<grid, 256, 0, s>>>((const T*)mu_new, (const T*)z, (T*)mu, (T*)w, t2_vec, step, len, batch);
    else
        k_refresh_pp<T, false><<<grid, 256, 0, s>>>((const T*)mu_new, (const T*)z, (T*)mu, (T*)w, t2_vec, step, len, batch);
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_refresh_pp(const void* mu_new, const void* z, void* mu, void* w, const int32_t* t2_vec, int step, size_t n,
                              int batch, int dtype, void* stream) {
    PNP_CHECK_ARG(mu_new && z && mu && w && t2_vec, "null argument");
    PNP_CHECK_ARG(batch > 0, "need batch >= 1");
    PNP_CHECK_ARG(n % (size_t)batch == 0, "n must be a multiple of batch");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    PNP_CHECK_ARG(mu_new != mu, "mu_new must not alias mu");
    PNP_CHECK_ARG(mu != w && z != w && mu_new != w && z != mu, "mu and w must be buffers of their own");
    PNP_CHECK_ARG(step >= 0, "need step >= 0");
    if (n == 0) return PNP_OK;
    if (dtype == PNP_F32)
        launch_refresh_pp<float>(mu_new, z, mu, w, t2_vec, step, n / batch, batch, (hipStream_t)stream);
    else
        launch_refresh_pp<double>(mu_new, z, mu, w, t2_vec, step, n / batch, batch, (hipStream_t)stream);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

// prox_wavelet2d.hip -- noise estimate + 2-D multi-level Haar BayesShrink prox + PSNR error sum.
//
// TVDenoiser(multi=False) of the reference (denoisers/TV.py:21-26): skimage denoise_wavelet(method='BayesShrink',
// multichannel=False) on a float image = pywt.wavedecn('db1', level L) over both axes, one soft threshold per detail
// sub-band (ad, da, dd of every level, each over the WHOLE image), pywt.waverecn.  L = max(min(log2 H, log2 W) - 3, 1).
//
// A level-L 2-D Haar transform is local to aligned 2^L x 2^L tiles (at most 32 x 32); only the 3 L sums of squares are
// image-wide.  One 256-thread workgroup owns one image and walks it twice in 32 x 32 regions, one region per wave and
// turn (pass 1: analysis -> sub-band sums of squares; pass 2: analysis again, shrink, synthesis, store, error sum).  Inside
// a region lane (ly, lx) of the 8 x 8 lane grid holds a 4 x 4 block of pixels: levels 1 and 2 stay in its registers,
// levels 3..5 pair lanes at distance 1, 2, 4 along x and 8, 16, 32 along y (every lane of a group computes the group's
// four coefficients, so synthesis needs no exchange at all).  There is ONE dispatch form: the result of an image cannot
// depend on the batch.  No scratch memory, no atomics; every sum is taken in a fixed order (lane, wave tree, waves 0..3).
// Arithmetic follows pywt product for product (-ffp-contract=off: exact zeros and 0/0 are significant).
//
// With sigma_in == NULL the workgroup first makes the noise estimate of pnp_sigma_est with its code (column_sigma on
// 16 columns x 4 row chunks per wave, column groups summed in order), so the two agree bit for bit.
#include "common.h"
#include "prox_tv.h"
#pragma clang fp contract(off)

namespace pnp {

constexpr int kW2dThreads = 256, kW2dWaves = kW2dThreads / 64;
constexpr int kW2dMaxLevels = 5, kW2dBands = 3 * kW2dMaxLevels;

template <typename T> struct Haar2 { static constexpr T C = (T)0.7071067811865476; };

// one level of pywt.wavedecn on a 2 x 2 quad: axis 0 (rows) first, then axis 1
template <typename T>
__device__ __forceinline__ void haar_quad(T a00, T a01, T a10, T a11, T& aa, T& ad, T& da, T& dd) {
    constexpr T C = Haar2<T>::C;
    const T lo0 = C * a10 + C * a00, lo1 = C * a11 + C * a01;
    const T hi0 = -C * a10 + C * a00, hi1 = -C * a11 + C * a01;
    aa = C * lo1 + C * lo0;
    ad = -C * lo1 + C * lo0;
    da = C * hi1 + C * hi0;
    dd = -C * hi1 + C * hi0;
}

// one level of pywt.waverecn: axis 1 first, then axis 0
template <typename T>
__device__ __forceinline__ void ihaar_quad(T aa, T ad, T da, T dd, T& o00, T& o01, T& o10, T& o11) {
    constexpr T C = Haar2<T>::C;
    const T lo_e = C * aa + C * ad, lo_o = C * aa - C * ad;
    const T hi_e = C * da + C * dd, hi_o = C * da - C * dd;
    o00 = C * lo_e + C * hi_e;
    o10 = C * lo_e - C * hi_e;
    o01 = C * lo_o + C * hi_o;
    o11 = C * lo_o - C * hi_o;
}

template <typename T> __device__ __forceinline__ T soft_shrink(T d, T thr) {
    const T mag = d < 0 ? -d : d;
    T shr = (T)1 - thr / mag;
    shr = shr < (T)0 ? (T)0 : shr;                     // keeps NaN (0/0) like numpy clip
    return d * shr;
}

// The coefficients of one 32 x 32 region as this lane sees them: v[][] holds levels 1 and 2 in place (level 1:
// v[2i][2j] = aa, v[2i][2j+1] = ad, v[2i+1][2j] = da, v[2i+1][2j+1] = dd; level 2 on the four aa: v[0][0] = aa,
// v[0][2] = ad, v[2][0] = da, v[2][2] = dd); up[l-3][] = ad, da, dd of level l >= 3 and top = aa of level L.
template <typename T> struct W2dCoef { T v[4][4]; T up[3][3]; T top; };

template <typename T>
__device__ __forceinline__ void w2d_analysis(W2dCoef<T>& c, int L, int lx, int ly) {
#pragma unroll
    for (int i = 0; i < 4; i += 2)
#pragma unroll
        for (int j = 0; j < 4; j += 2)
            haar_quad(c.v[i][j], c.v[i][j + 1], c.v[i + 1][j], c.v[i + 1][j + 1], c.v[i][j], c.v[i][j + 1], c.v[i + 1][j], c.v[i + 1][j + 1]);
    if (L >= 2) haar_quad(c.v[0][0], c.v[0][2], c.v[2][0], c.v[2][2], c.v[0][0], c.v[0][2], c.v[2][0], c.v[2][2]);
    c.top = c.v[0][0];
#pragma unroll
    for (int l = 3; l <= kW2dMaxLevels; ++l) {
        const int s = 1 << (l - 3);
        if (l <= L) {                                   // uniform over the launch
            const T own = c.top;
            const T xc = __shfl_xor(own, s, 64), xr = __shfl_xor(own, 8 * s, 64), xrc = __shfl_xor(own, 9 * s, 64);
            const bool pc = (lx & s) != 0, pr = (ly & s) != 0;
            const T a00 = pr ? (pc ? xrc : xr) : (pc ? xc : own);
            const T a01 = pr ? (pc ? xr : xrc) : (pc ? own : xc);
            const T a10 = pr ? (pc ? xc : own) : (pc ? xrc : xr);
            const T a11 = pr ? (pc ? own : xc) : (pc ? xr : xrc);
            haar_quad(a00, a01, a10, a11, c.top, c.up[l - 3][0], c.up[l - 3][1], c.up[l - 3][2]);
        }
    }
}

// this lane's share of the sums of squares: acc[3 (l-1) + band] += d * d; a coefficient of level l >= 3 is held by every
// lane of its group and counted by the group's first lane only
template <typename T>
__device__ __forceinline__ void w2d_accumulate(const W2dCoef<T>& c, int L, int lx, int ly, bool inside, T (&acc)[kW2dBands]) {
    if (!inside) return;
    acc[0] += ((c.v[0][1] * c.v[0][1] + c.v[0][3] * c.v[0][3]) + c.v[2][1] * c.v[2][1]) + c.v[2][3] * c.v[2][3];
    acc[1] += ((c.v[1][0] * c.v[1][0] + c.v[1][2] * c.v[1][2]) + c.v[3][0] * c.v[3][0]) + c.v[3][2] * c.v[3][2];
    acc[2] += ((c.v[1][1] * c.v[1][1] + c.v[1][3] * c.v[1][3]) + c.v[3][1] * c.v[3][1]) + c.v[3][3] * c.v[3][3];
    if (L >= 2) {
        acc[3] += c.v[0][2] * c.v[0][2];
        acc[4] += c.v[2][0] * c.v[2][0];
        acc[5] += c.v[2][2] * c.v[2][2];
    }
#pragma unroll
    for (int l = 3; l <= kW2dMaxLevels; ++l) {
        const int m = (2 << (l - 3)) - 1;
        if (l <= L && ((lx | ly) & m) == 0) {
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[3 * (l - 1) + b] += c.up[l - 3][b] * c.up[l - 3][b];
        }
    }
}

template <typename T>
__device__ __forceinline__ void w2d_shrink_synthesis(W2dCoef<T>& c, int L, int lx, int ly, const T (&thr)[kW2dBands]) {
#pragma unroll
    for (int l = kW2dMaxLevels; l >= 3; --l) {
        const int s = 1 << (l - 3);
        if (l <= L) {
            T o00, o01, o10, o11;
            ihaar_quad(c.top, soft_shrink(c.up[l - 3][0], thr[3 * (l - 1)]), soft_shrink(c.up[l - 3][1], thr[3 * (l - 1) + 1]),
                       soft_shrink(c.up[l - 3][2], thr[3 * (l - 1) + 2]), o00, o01, o10, o11);
            const bool pc = (lx & s) != 0, pr = (ly & s) != 0;
            c.top = pr ? (pc ? o11 : o10) : (pc ? o01 : o00);
        }
    }
    c.v[0][0] = c.top;
    if (L >= 2)
        ihaar_quad(c.v[0][0], soft_shrink(c.v[0][2], thr[3]), soft_shrink(c.v[2][0], thr[4]), soft_shrink(c.v[2][2], thr[5]),
                   c.v[0][0], c.v[0][2], c.v[2][0], c.v[2][2]);
#pragma unroll
    for (int i = 0; i < 4; i += 2)
#pragma unroll
        for (int j = 0; j < 4; j += 2)
            ihaar_quad(c.v[i][j], soft_shrink(c.v[i][j + 1], thr[0]), soft_shrink(c.v[i + 1][j], thr[1]),
                       soft_shrink(c.v[i + 1][j + 1], thr[2]), c.v[i][j], c.v[i][j + 1], c.v[i + 1][j], c.v[i + 1][j + 1]);
}

// zin / zout may alias (in-place prox): pass 1 has read the whole image before pass 2 stores anything, and in pass 2 a
// region is read and written by the same lanes.
template <typename T, int H>
__global__ __launch_bounds__(kW2dThreads) void k_prox_wavelet2d(const T* zin, T* zout, int W, int L,
                                                                const T* __restrict__ sigma_in, T sigma_modifier, T fallback_sigma,
                                                                const T* __restrict__ xrec, double* __restrict__ sse_out,
                                                                T* __restrict__ sigma_out) {
#include "prox_wavelet2d_body.h"
}

// sigma_modifier per problem (pnp_prox_wavelet2d_pp): sm_pp is a DOUBLE [batch] array, cast to T as the host casts the scalar
template <typename T, int H>
__global__ __launch_bounds__(kW2dThreads) void k_prox_wavelet2d_pp(const T* zin, T* zout, int W, int L,
                                                                   const T* __restrict__ sigma_in, const double* __restrict__ sm_pp,
                                                                   T fallback_sigma, const T* __restrict__ xrec,
                                                                   double* __restrict__ sse_out, T* __restrict__ sigma_out) {
    const T sigma_modifier = (T)sm_pp[blockIdx.x];
#include "prox_wavelet2d_body.h"
}

template <typename T, int H>
int launch_prox_wavelet2d(const void* zin, void* zout, int W, int batch, const void* sigma_in, double mod, double fb,
                          const void* xrec, double* sse, void* sigma_out, hipStream_t s, const double* sm_pp) {
    int lw = 0;
    while ((2 << lw) <= W) ++lw;                       // floor(log2 W)
    const int lh = HaarLevels<H>::value + 3;           // log2 H
    const int L = (lh < lw ? lh : lw) - 3 > 1 ? (lh < lw ? lh : lw) - 3 : 1;
    if (sm_pp != nullptr)
        k_prox_wavelet2d_pp<T, H><<<batch, kW2dThreads, 0, s>>>((const T*)zin, (T*)zout, W, L, (const T*)sigma_in, sm_pp, (T)fb,
                                                               (const T*)xrec, sse, (T*)sigma_out);
    else
        k_prox_wavelet2d<T, H><<<batch, kW2dThreads, 0, s>>>((const T*)zin, (T*)zout, W, L, (const T*)sigma_in, (T)mod, (T)fb,
                                                            (const T*)xrec, sse, (T*)sigma_out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_prox_wavelet2d(const void* z_in, void* z_out, int H, int W, int batch, int dtype, const void* sigma_in,
                                  double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_out,
                                  void* sigma_out, void* stream) {
    PNP_CHECK_ARG(z_out != nullptr, "null output");
    PNP_CHECK_ARG(z_in != nullptr && batch >= 1, "null input / empty batch");
    PNP_CHECK_ARG(H == 16 || H == 32 || H == 64 || H == 128 || H == 256, "H must be 16, 32, 64, 128 or 256");
    PNP_CHECK_ARG(W % 16 == 0 && W >= 16 && W <= 256, "W must be a multiple of 16 in [16, 256]");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
#define PNP_W2D_CASE(TT, HH) \
    return launch_prox_wavelet2d<TT, HH>(z_in, z_out, W, batch, sigma_in, sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, (hipStream_t)stream, nullptr)
    if (dtype == PNP_F32) {
        if (H == 256) PNP_W2D_CASE(float, 256);
        if (H == 128) PNP_W2D_CASE(float, 128);
        if (H == 64) PNP_W2D_CASE(float, 64);
        if (H == 32) PNP_W2D_CASE(float, 32);
        PNP_W2D_CASE(float, 16);
    }
    if (H == 256) PNP_W2D_CASE(double, 256);
    if (H == 128) PNP_W2D_CASE(double, 128);
    if (H == 64) PNP_W2D_CASE(double, 64);
    if (H == 32) PNP_W2D_CASE(double, 32);
    PNP_W2D_CASE(double, 16);
#undef PNP_W2D_CASE
}

extern "C" int pnp_prox_wavelet2d_pp(const void* z_in, void* z_out, int H, int W, int batch, int dtype, const void* sigma_in,
                                  double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                  double* sse_out, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(z_out != nullptr, "null output");
    PNP_CHECK_ARG(z_in != nullptr && batch >= 1, "null input / empty batch");
    PNP_CHECK_ARG(H == 16 || H == 32 || H == 64 || H == 128 || H == 256, "H must be 16, 32, 64, 128 or 256");
    PNP_CHECK_ARG(W % 16 == 0 && W >= 16 && W <= 256, "W must be a multiple of 16 in [16, 256]");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
#define PNP_W2D_CASE(TT, HH) \
    return launch_prox_wavelet2d<TT, HH>(z_in, z_out, W, batch, sigma_in, sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, (hipStream_t)stream, sigma_modifier_pp)
    if (dtype == PNP_F32) {
        if (H == 256) PNP_W2D_CASE(float, 256);
        if (H == 128) PNP_W2D_CASE(float, 128);
        if (H == 64) PNP_W2D_CASE(float, 64);
        if (H == 32) PNP_W2D_CASE(float, 32);
        PNP_W2D_CASE(float, 16);
    }
    if (H == 256) PNP_W2D_CASE(double, 256);
    if (H == 128) PNP_W2D_CASE(double, 128);
    if (H == 64) PNP_W2D_CASE(double, 64);
    if (H == 32) PNP_W2D_CASE(double, 32);
    PNP_W2D_CASE(double, 16);
#undef PNP_W2D_CASE
}

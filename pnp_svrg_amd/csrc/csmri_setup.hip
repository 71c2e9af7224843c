// csmri_setup.hip -- a batch of CSMRI problems generated on the device (problems/CSMRI.py:12-59 per problem, from the
// counter-based stream published in include/pnp_hip.h): Bernoulli mask, masked spectrum, real noise on the support,
// Xinit = minmax |ifft2 Y| -- written in the layouts the gradient kernels read, so that a sweep's setup never touches
// the host.
//
//   k_gen_mask      key_0(i) < T per k-space position -> bitsT (and the uint8 maskT), one thread per 32-bit word
//   k_gen_gather    xrec[b] = images[image_idx[b]]
//   k_rows_fwd      (csmri_rows.h) row pass of fft2(xrec) into the plan's half-spectrum workspace
//   k_gen_cols_fwd  column FFT, Hermitian expansion to the FULL spectrum, mask -> Y0 in YT
//   k_gen_stats     M0, 1/M0, ||Y0||^2 in double (fixed order) -> sigma
//   k_gen_noise     Y = Y0 + mask * sigma * n, Box-Muller in double from key_1, key_2
//   k_gen_pack_inv  PART 0: Hermitian part of Y, packed (= yh_full, the arithmetic of k_pack_y) -> inverse column FFT
//                   PART 1: the same of -i Y (the anti-Hermitian part of Y times -i)
//   k_rows_inv      (csmri_rows.h) Re ifft2 Y -> xinit, then Im ifft2 Y combined with it: |ifft2 Y|
//   k_gen_minmax    xinit = (m - min m) / (max m - min m)
//
// Y is not Hermitian (the mask is not symmetric), so |ifft2 Y| needs both parts of the inverse: Y = Yh + i Ya with Yh, Ya
// Hermitian, ifft2 Yh = Re ifft2 Y and ifft2 Ya = Im ifft2 Y are real images, and each goes through the real-output
// inverse passes the gradient already has, in the plan's half-spectrum workspace; Yh packed IS yh_full.
//
// Every kernel works on one problem per blockIdx.y (or .x) with reductions in a fixed order and no atomics: an item's
// outputs do not depend on the batch size or on its place in the batch.
#include "csmri_rows.h"
#include "draw.h"
#include "reduce.h"

namespace pnp {

// state_k = mix64(mix64(mix64(seed) + id) + k): sub-stream k of item (seed, id)
__device__ __forceinline__ uint64_t gen_state(uint64_t seed, uint64_t id, uint64_t k) {
    return mix64(mix64(mix64(seed) + id) + k);
}

__device__ __forceinline__ uint32_t mask_bit(const uint32_t* __restrict__ bits, int wpr, int kx, int ky) {
    return (bits[kx * wpr + (ky >> 5)] >> (ky & 31)) & 1u;
}

// ------------------------------------------------------------------------------- mask
__global__ __launch_bounds__(256) void k_gen_mask(const uint64_t* __restrict__ seed, const uint64_t* __restrict__ id,
                                                  const uint64_t* __restrict__ thresh, uint32_t* __restrict__ bitsT,
                                                  uint8_t* __restrict__ maskT, int H, int W) {
    const int prob = blockIdx.y, wpr = H / 32, nwords = W * wpr;
    const int wd = blockIdx.x * blockDim.x + threadIdx.x;
    if (wd >= nwords) return;
    const uint64_t st = gen_state(seed[prob], id[prob], 0), T = thresh[prob];
    const int kx = wd / wpr, kyb = (wd - kx * wpr) * 32;
    uint32_t m = 0;
#pragma unroll 8
    for (int bt = 0; bt < 32; ++bt) {
        const uint32_t i = (uint32_t)((kyb + bt) * W + kx);            // flat row-major k-space index
        m |= ((uint64_t)mb_key(st, i) < T ? 1u : 0u) << bt;
    }
    bitsT[(size_t)prob * nwords + wd] = m;
    if (maskT != nullptr) {
        uint4* dst = reinterpret_cast<uint4*>(maskT + ((size_t)prob * nwords + wd) * 32);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint32_t w4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t nib = (m >> (16 * q + 4 * j)) & 0xFu;      // four mask bits -> four 0/1 bytes
                w4[j] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
            }
            dst[q] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
    }
}

// ------------------------------------------------------------------------------- images
template <typename T>
__global__ __launch_bounds__(256) void k_gen_gather(const T* __restrict__ images, int n_images, const int32_t* __restrict__ image_idx,
                                                    T* __restrict__ xrec, int n4) {
    const int prob = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n4) return;
    int im = image_idx[prob];
    im = im < 0 ? 0 : (im >= n_images ? n_images - 1 : im);            // (the host checks the range; never read outside the set)
    const vec4<T>* src = reinterpret_cast<const vec4<T>*>(images) + (size_t)im * n4;
    reinterpret_cast<vec4<T>*>(xrec)[(size_t)prob * n4 + j] = src[j];
}

// ------------------------------------------------------------------------------- columns forward -> masked full spectrum
// One lane group per PACKED column c of the row pass (csmri_rows.h): c >= 1 carries kx = c, whose transform also gives
// kx = W - c (X[ky][W-c] = conj X[-ky][c], the image is real); c == 0 carries the two real-input columns kx = 0, W/2.
template <typename T, int RA, int LA>
__global__ __launch_bounds__(256) void k_gen_cols_fwd(const cx<T>* __restrict__ S1T, const uint32_t* __restrict__ bitsT,
                                                      cx<T>* __restrict__ YT, const cx<T>* __restrict__ twtab, int W) {
    using S = FftSmem<T, RA, LA>;
    constexpr int N = S::N, G = S::G, LG = S::LG;            // N = H
    constexpr int WPR = N / 32;
    __shared__ cx<T> smem[S::SCR];
    const int t = threadIdx.x, g = t / LG, lane = t % LG;
    const int prob = blockIdx.y, c = blockIdx.x * G + g;
    const cx<T>* col = S1T + ((size_t)prob * (W / 2) + c) * N;
    cx<T>* scr = smem + g * LG * (LG + 1);

    cx<T> v[LG], tw[LG];
    load_twiddles_gen<T, LG>(tw, twtab, lane, N);
#pragma unroll
    for (int r = 0; r < RA; ++r) v[r] = col[(lane < LA ? lane : 0) + LA * r];
    fft_gen<T, RA, LA, false>(v, tw, scr, lane);
    __syncthreads();
    if (lane < RA) {
#pragma unroll
        for (int r = 0; r < LA; ++r) scr[lane + RA * r] = v[r];
    }
    __syncthreads();
    if (lane < RA) {
        const int k1 = c == 0 ? 0 : c, k2 = c == 0 ? W / 2 : W - c;
        const uint32_t* bits = bitsT + (size_t)prob * W * WPR;
        cx<T>* y1 = YT + ((size_t)prob * W + k1) * N;
        cx<T>* y2 = YT + ((size_t)prob * W + k2) * N;
#pragma unroll
        for (int r = 0; r < LA; ++r) {
            const int ky = lane + RA * r, km = (N - ky) & (N - 1);
            const cx<T> pk = v[r], pm = scr[km];
            cx<T> o1, o2;
            if (c == 0) {
                o1 = {(T)0.5 * (pk.x + pm.x), (T)0.5 * (pk.y - pm.y)};
                o2 = {(T)0.5 * (pk.y + pm.y), (T)-0.5 * (pk.x - pm.x)};
            } else {
                o1 = pk;
                o2 = cconj(pm);
            }
            const bool m1 = mask_bit(bits, WPR, k1, ky) != 0, m2 = mask_bit(bits, WPR, k2, ky) != 0;
            y1[ky] = cx<T>{m1 ? o1.x : (T)0, m1 ? o1.y : (T)0};
            y2[ky] = cx<T>{m2 ? o2.x : (T)0, m2 ? o2.y : (T)0};
        }
    }
}

// ------------------------------------------------------------------------------- M0, sigma
// sigma = sqrt(||Y0||_2 * 10^(-snr/10) / H / W)  (problems/problem.py:58-61: the norm, not its square)
template <typename T>
__global__ __launch_bounds__(256) void k_gen_stats(const cx<T>* __restrict__ YT, const uint32_t* __restrict__ bitsT,
                                                   const double* __restrict__ snr_fac, int32_t* __restrict__ M0,
                                                   T* __restrict__ inv_m0, double* __restrict__ sigma, int H, int W) {
    __shared__ double ssum[256];
    __shared__ int scnt[256];
    const int prob = blockIdx.x, t = threadIdx.x, n = H * W, nwords = W * (H / 32);
    const cx<T>* Y = YT + (size_t)prob * n;
    double acc = 0.0;
    for (int j = t; j < n; j += 256) {
        const cx<T> y = Y[j];
        acc = fma_((double)y.x, (double)y.x, acc);
        acc = fma_((double)y.y, (double)y.y, acc);
    }
    int cnt = 0;
    for (int wd = t; wd < nwords; wd += 256) cnt += __builtin_popcount(bitsT[(size_t)prob * nwords + wd]);
    ssum[t] = acc;
    scnt[t] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {                          // fixed tree: the same sum whatever the batch
        if (t < s) { ssum[t] += ssum[t + s]; scnt[t] += scnt[t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        M0[prob] = scnt[0];
        inv_m0[prob] = (T)(1.0 / (double)scnt[0]);
        sigma[prob] = sqrt(sqrt(ssum[0]) * snr_fac[prob] / (double)H / (double)W);
    }
}

// ------------------------------------------------------------------------------- noise
// n(i) = sqrt(-2 ln u1) cos(2 pi u2), u1 = (key_1(i) + 1) 2^-32 in (0, 1], u2 = key_2(i) 2^-32 in [0, 1): in double for
// both plan dtypes, added to the real part on the support, one rounding to T.
template <typename T>
__global__ __launch_bounds__(256) void k_gen_noise(cx<T>* __restrict__ YT, const uint32_t* __restrict__ bitsT,
                                                   const uint64_t* __restrict__ seed, const uint64_t* __restrict__ id,
                                                   const double* __restrict__ sigma, int H, int W) {
    const int prob = blockIdx.y, wpr = H / 32;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;         // transposed flat index kx*H + ky
    if (j >= H * W) return;
    const int kx = j / H, ky = j - kx * H;
    if (!mask_bit(bitsT + (size_t)prob * W * wpr, wpr, kx, ky)) return;
    const uint32_t i = (uint32_t)(ky * W + kx);
    const uint64_t sd = seed[prob], it = id[prob];
    const double u1 = ((double)mb_key(gen_state(sd, it, 1), i) + 1.0) * 0x1p-32;
    const double u2 = (double)mb_key(gen_state(sd, it, 2), i) * 0x1p-32;
    const double nrm = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    cx<T>* y = YT + (size_t)prob * H * W + j;
    y->x = (T)fma_(sigma[prob], nrm, (double)y->x);
}

// ------------------------------------------------------------------------------- Hermitian parts -> inverse columns
// PART 0: P = Y; PART 1: P = -i Y.  Packed column c of the Hermitian part of mask o P, in the arithmetic of k_pack_y
// (csmri.hip; the products by the 0/1 mask are exact, so contraction cannot change a bit) -> yh (PART 0 only) -> inverse
// FFT-H -> the plan's workspace, ready for k_rows_inv.
template <typename T, int RA, int LA, int PART>
__global__ __launch_bounds__(256) void k_gen_pack_inv(const cx<T>* __restrict__ YT, const uint32_t* __restrict__ bitsT,
                                                      cx<T>* __restrict__ yh, cx<T>* __restrict__ S1T,
                                                      const cx<T>* __restrict__ twtab, int W) {
    using S = FftSmem<T, RA, LA>;
    constexpr int N = S::N, G = S::G, LG = S::LG;            // N = H
    constexpr int WPR = N / 32;
    __shared__ cx<T> smem[S::SCR];
    const int t = threadIdx.x, g = t / LG, lane = t % LG;
    const int prob = blockIdx.y, c = blockIdx.x * G + g;
    const int ln = lane < RA ? lane : 0;
    const cx<T>* Y = YT + (size_t)prob * W * N;
    const uint32_t* bits = bitsT + (size_t)prob * W * WPR;

    auto term = [&](int cc, int ky) -> cx<T> {
        const int c2 = (W - cc) % W, k2 = (N - ky) % N;
        const T s1 = (T)mask_bit(bits, WPR, cc, ky), s2 = (T)mask_bit(bits, WPR, c2, k2);
        cx<T> y1 = Y[(size_t)cc * N + ky], y2 = Y[(size_t)c2 * N + k2];
        if (PART == 1) { y1 = {y1.y, -y1.x}; y2 = {y2.y, -y2.x}; }
        return {(T)0.5 * (s1 * y1.x + s2 * y2.x), (T)0.5 * (s1 * y1.y - s2 * y2.y)};
    };

    cx<T> v[LG], tw[LG];
    load_twiddles_gen<T, LG>(tw, twtab, lane, N);
#pragma unroll
    for (int r = 0; r < LA; ++r) {
        const int ky = ln + RA * r;
        if (c == 0) {
            const cx<T> A = term(0, ky), B = term(W / 2, ky);
            v[r] = {A.x - B.y, A.y + B.x};
        } else {
            v[r] = term(c, ky);
        }
        if (PART == 0 && lane < RA) yh[((size_t)prob * (W / 2) + c) * N + ky] = v[r];
    }
    fft_gen<T, LA, RA, true>(v, tw, smem + g * LG * (LG + 1), lane);
    if (lane < LA) {
        cx<T>* col = S1T + ((size_t)prob * (W / 2) + c) * N;
#pragma unroll
        for (int r = 0; r < RA; ++r) col[lane + LA * r] = v[r];
    }
}

// ------------------------------------------------------------------------------- min-max normalisation, in place
template <typename T>
__global__ __launch_bounds__(256) void k_gen_minmax(T* __restrict__ x, int n) {
    __shared__ T rmin[4], rmax[4];
    T* z = x + (size_t)blockIdx.x * n;
    T lo = z[0], hi = lo;
    for (int i = threadIdx.x; i < n; i += 256) {
        const T v = z[i];
        lo = nan_min(v, lo);
        hi = nan_max(v, hi);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = lo; rmax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = rmin[0];
    hi = rmax[0];
    for (int i = 1; i < 4; ++i) { lo = nan_min(rmin[i], lo); hi = nan_max(rmax[i], hi); }
    const T span = hi - lo;
    for (int i = threadIdx.x; i < n; i += 256) z[i] = (z[i] - lo) / span;
}

}  // namespace pnp

using namespace pnp;

namespace {
template <typename T, int RA, int LA>
int run_generate(pnp_csmri_plan* p, const void* images, int n_images, const int32_t* image_idx, const uint64_t* thresh,
                 const double* snr_fac, const uint64_t* seed, const uint64_t* id, void* xrec, uint32_t* bitsT, uint8_t* maskT,
                 void* YT, void* yh_full, void* xinit, int32_t* M0, void* inv_m0, double* sigma, hipStream_t s) {
    constexpr int G = FftSmem<T, RA, LA>::G;
    const int H = p->H, W = p->W, B = p->batch, n = H * W, nwords = W * (H / 32);
    cx<T>* work = (cx<T>*)p->work;
    const cx<T>* tw = (const cx<T>*)p->twtab;
    const dim3 rows(H / (2 * G), B), cols((W / 2) / G, B), flat((n + 255) / 256, B);
    const T scale = (T)(1.0 / ((double)H * (double)W));

    k_gen_mask<<<dim3((nwords + 255) / 256, B), 256, 0, s>>>(seed, id, thresh, bitsT, maskT, H, W);
    PNP_CHECK_LAUNCH();
    k_gen_gather<T><<<dim3((n / 4 + 255) / 256, B), 256, 0, s>>>((const T*)images, n_images, image_idx, (T*)xrec, n / 4);
    PNP_CHECK_LAUNCH();
    k_rows_fwd<T, RA, LA><<<rows, 256, 0, s>>>((const T*)xrec, nullptr, work, tw, H);
    PNP_CHECK_LAUNCH();
    k_gen_cols_fwd<T, RA, LA><<<cols, 256, 0, s>>>(work, bitsT, (cx<T>*)YT, tw, W);
    PNP_CHECK_LAUNCH();
    k_gen_stats<T><<<B, 256, 0, s>>>((const cx<T>*)YT, bitsT, snr_fac, M0, (T*)inv_m0, sigma, H, W);
    PNP_CHECK_LAUNCH();
    k_gen_noise<T><<<flat, 256, 0, s>>>((cx<T>*)YT, bitsT, seed, id, sigma, H, W);
    PNP_CHECK_LAUNCH();
    k_gen_pack_inv<T, RA, LA, 0><<<cols, 256, 0, s>>>((const cx<T>*)YT, bitsT, (cx<T>*)yh_full, work, tw, W);
    PNP_CHECK_LAUNCH();
    k_rows_inv<T, RA, LA><<<rows, 256, 0, s>>>(work, tw, H, scale, nullptr, (T)0, nullptr, (T)0, nullptr, (T*)xinit);
    PNP_CHECK_LAUNCH();
    k_gen_pack_inv<T, RA, LA, 1><<<cols, 256, 0, s>>>((const cx<T>*)YT, bitsT, nullptr, work, tw, W);
    PNP_CHECK_LAUNCH();
    k_rows_inv<T, RA, LA, true><<<rows, 256, 0, s>>>(work, tw, H, scale, nullptr, (T)0, (const T*)xinit, (T)0, nullptr, (T*)xinit);
    PNP_CHECK_LAUNCH();
    k_gen_minmax<T><<<B, 256, 0, s>>>((T*)xinit, n);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}
}  // namespace

extern "C" int pnp_csmri_generate(pnp_csmri_plan* p, const void* images, int n_images, const int32_t* image_idx,
                                  const uint64_t* thresh, const double* snr_fac, const uint64_t* seed, const uint64_t* id,
                                  void* xrec, uint32_t* bitsT, uint8_t* maskT, void* YT, void* yh_full, void* xinit,
                                  int32_t* M0, void* inv_m0, double* sigma, void* stream) {
    PNP_CHECK_ARG(p != nullptr, "null plan");
    PNP_CHECK_ARG(images && image_idx && thresh && snr_fac && seed && id, "null input");
    PNP_CHECK_ARG(xrec && bitsT && YT && yh_full && xinit && M0 && inv_m0 && sigma, "null output (only maskT may be NULL)");
    PNP_CHECK_ARG(n_images >= 1, "n_images must be >= 1");
    hipStream_t s = (hipStream_t)stream;
#define PNP_GEN_ARGS p, images, n_images, image_idx, thresh, snr_fac, seed, id, xrec, bitsT, maskT, YT, yh_full, xinit, M0, inv_m0, sigma, s
    if (p->dtype == PNP_F32) {
        if (p->NL == 16) return run_generate<float, 16, 16>(PNP_GEN_ARGS);
        if (p->NL == 12) return run_generate<float, 8, 16>(PNP_GEN_ARGS);
        return run_generate<float, 8, 8>(PNP_GEN_ARGS);
    }
    if (p->NL == 16) return run_generate<double, 16, 16>(PNP_GEN_ARGS);
    if (p->NL == 12) return run_generate<double, 8, 16>(PNP_GEN_ARGS);
    return run_generate<double, 8, 8>(PNP_GEN_ARGS);
#undef PNP_GEN_ARGS
}

// csmri_rows.h -- the row passes of the CSMRI transforms, shared by the gradient
// (csmri.hip) and the on-device problem generator (csmri_setup.hip).
//
//   k_rows_fwd   two real image rows -> one complex FFT-W -> split -> packed half spectrum,
//                written TRANSPOSED ([kx][h]) through an LDS tile (256-B segments)
//   k_rows_inv   transposed read -> Hermitian re-expansion -> one complex inverse FFT-W gives two
//                real rows -> fused epilogue  out = alpha*g + beta*c1 + gamma*c2
//
// "Packed": column kx=0 stores (X[.,0], X[.,W/2]) as (re,im) -- both are real after the row
// pass -- so the half spectrum is exactly [W/2][H] complex = the bytes of the real image.
#pragma once
#include "fft.h"
#include "csmri_plan.h"

namespace pnp {

template <typename T> struct alignas(4 * sizeof(T)) vec4 { T a, b, c, d; };

// RA x LA = the register x lane split of one length-N transform (fft.h: fft_gen); RA == LA for N = 64, 256,
// <8,16> for N = 128.  A lane group is LG = max(RA, LA) lanes.
template <typename T, int RA, int LA> struct FftSmem {
    static constexpr int N = RA * LA;
    static constexpr int LG = RA > LA ? RA : LA;
    static constexpr int G = 256 / LG;                       // lane groups per 256-thread block
    static constexpr int TILE = G * (N + 1);                 // [group][N+1] complex
    static constexpr int SCR = G * LG * (LG + 1);            // [group][LG][LG+1] complex
    static constexpr int ELEMS = TILE > SCR ? TILE : SCR;
};

// ------------------------------------------------------------------------------- rows forward
template <typename T, int RA, int LA>
__global__ __launch_bounds__(256) void k_rows_fwd(const T* __restrict__ a, const T* __restrict__ b,
                                                  cx<T>* __restrict__ S1T, const cx<T>* __restrict__ twtab, int H) {
    using S = FftSmem<T, RA, LA>;
    constexpr int N = S::N, G = S::G, LG = S::LG;
    __shared__ cx<T> smem[S::ELEMS];
    const int t = threadIdx.x, g = t / LG, lane = t % LG;
    const int prob = blockIdx.y, h0 = blockIdx.x * 2 * G;
    const size_t img = (size_t)prob * H * N;
    const size_t ra = img + (size_t)(h0 + 2 * g) * N, rb = ra + N;

    cx<T> v[LG], tw[LG];
    load_twiddles_gen<T, LG>(tw, twtab, lane, N);
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const int w = (lane < LA ? lane : 0) + LA * r;
        T va = a[ra + w], vb = a[rb + w];
        if (b != nullptr) { va -= b[ra + w]; vb -= b[rb + w]; }
        v[r] = {va, vb};
    }
    fft_gen<T, RA, LA, false>(v, tw, smem + g * LG * (LG + 1), lane);
    __syncthreads();
    if (lane < RA) {
#pragma unroll
        for (int r = 0; r < LA; ++r) smem[g * (N + 1) + lane + RA * r] = v[r];
    }
    __syncthreads();

    // split the two interleaved real transforms and store transposed
    const int p = t % G;
    const cx<T>* zp = smem + p * (N + 1);
    for (int kx = t / G; kx < N / 2; kx += 256 / G) {
        const cx<T> zk = zp[kx], zm = zp[(N - kx) & (N - 1)];
        vec4<T> o;
        if (kx == 0) {
            const cx<T> zn = zp[N / 2];
            o = {zk.x, zn.x, zk.y, zn.y};
        } else {
            o = {(T)0.5 * (zk.x + zm.x), (T)0.5 * (zk.y - zm.y), (T)0.5 * (zk.y + zm.y), (T)-0.5 * (zk.x - zm.x)};
        }
        *reinterpret_cast<vec4<T>*>(S1T + ((size_t)prob * (N / 2) + kx) * H + h0 + 2 * p) = o;
    }
}

// ------------------------------------------------------------------------------- rows inverse + epilogue
// MAG (the generator's |ifft2| of a non-Hermitian spectrum, csmri_setup.hip): out = sqrt((alpha*g)^2 + c1^2) instead;
// c1 (required, not NULL) = the image of the other (Hermitian / anti-Hermitian) part, beta, gamma and c2 are NOT used;
// out may alias c1 (each thread reads an element before it writes it).
template <typename T, int RA, int LA, bool MAG = false>
__global__ __launch_bounds__(256) void k_rows_inv(const cx<T>* __restrict__ S1T, const cx<T>* __restrict__ twtab, int H,
                                                  T alpha, const T* __restrict__ alpha_vec, T beta, const T* c1, T gamma,
                                                  const T* c2, T* out) {
#include "rows_inv_body.h"
}

// Per-problem coefficients (pnp_csmri_grad_sel_pp): alpha_pp / gamma_pp are DOUBLE [batch] arrays (NULL: the scalar), converted
// here exactly as the host converts the scalars of k_rows_inv: alpha -> (T)(alpha * 1/(H W)) (inv_n is a power of two: the
// product is the host's quotient), then the product with alpha_vec[b]; gamma -> (T)gamma.
template <typename T, int RA, int LA>
__global__ __launch_bounds__(256) void k_rows_inv_pp(const cx<T>* __restrict__ S1T, const cx<T>* __restrict__ twtab, int H,
                                                     T alpha, const double* __restrict__ alpha_pp, double inv_n,
                                                     const T* __restrict__ alpha_vec, T beta, const T* c1, T gamma,
                                                     const double* __restrict__ gamma_pp, const T* c2, T* out) {
    constexpr bool MAG = false;
    if (alpha_pp != nullptr) alpha = (T)(alpha_pp[blockIdx.y] * inv_n);
    if (gamma_pp != nullptr) gamma = (T)gamma_pp[blockIdx.y];
#include "rows_inv_body.h"
}

}  // namespace pnp

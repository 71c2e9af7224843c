// csmri.hip -- masked-FFT data-fidelity gradient for CSMRI on gfx950.
//
// Replaces reference problems/CSMRI.py:76-81 (grad_full) and :83-89 (grad_stoch):
//     g = Re ifft2( sel o fft2(x) - sel o Y )
// The real part of an inverse FFT only sees the Hermitian part of its argument, so the
// whole thing runs on the half spectrum with real<->complex transforms:
//
//   k_rows_fwd   (csmri_rows.h) real rows -> packed transposed half spectrum
//   k_cols       per kx column: FFT-H -> symmetrised selector (and data term) -> inverse FFT-H,
//                in one kernel, in place (forward and inverse share the axis)
//   k_rows_inv   (csmri_rows.h) Hermitian re-expansion, inverse row FFT, fused epilogue
#include "csmri_rows.h"
#include "draw.h"
#include "csmri_fused.h"
#include <vector>
#include <cstdlib>
#include <cmath>

namespace pnp {

// ------------------------------------------------------------------------------- columns
// Selector forms of the column pass:
//   SEL_U8   explicit transposed uint8 selector [W][H] (host-drawn minibatches: reference-identical index lists)
//   SEL_BITS a bit-packed transposed selector: word [kx][ky >> 5], bit ky & 31 -- the sampling mask itself (grad_full),
//            or mask o device-drawn minibatch as k_draw_thr emits it (8 KiB per problem instead of a 64 KiB byte
//            selector written by one kernel and read by the next)
enum { SEL_U8 = 0, SEL_BITS = 1 };

template <typename T, int RA, int LA, int SEL>
__global__ __launch_bounds__(256) void k_cols(cx<T>* __restrict__ S1T, const uint8_t* __restrict__ selT,
                                              const uint32_t* __restrict__ bitsT,
                                              const cx<T>* __restrict__ yh, const cx<T>* __restrict__ YT,
                                              const cx<T>* __restrict__ twtab, int W) {
    using S = FftSmem<T, RA, LA>;
    constexpr int N = S::N, G = S::G, LG = S::LG;            // N = H
    constexpr int WPR = N / 32;                              // mask words per k-space column
    __shared__ cx<T> smem[S::SCR];
    __shared__ uint32_t sb[2][G][WPR];                       // mask bits of this block's columns c (slot 0) and W - c (slot 1)
    const int t = threadIdx.x, g = t / LG, lane = t % LG;
    const int prob = blockIdx.y, c = blockIdx.x * G + g;
    cx<T>* col = S1T + ((size_t)prob * (W / 2) + c) * N;
    cx<T>* scr = smem + g * LG * (LG + 1);
    const bool act = lane < RA;                              // lanes that hold spectrum values after the forward pass
    const int ln = act ? lane : 0;

    if (SEL != SEL_U8 && t < 2 * G * WPR) {
        const int slot = t / (G * WPR), gg = (t / WPR) % G, wd = t % WPR, cc = blockIdx.x * G + gg;
        const int kx = cc == 0 ? (slot == 0 ? 0 : W / 2) : (slot == 0 ? cc : W - cc);     // packed column 0 = kx 0 and W/2
        sb[slot][gg][wd] = bitsT[((size_t)prob * W + kx) * WPR + wd];
    }
    // selector value at (kx, ky); slot says in which staged row kx sits
    auto sel_at = [&](int slot, int kx, int ky, const uint8_t* row) -> T {
        if (SEL == SEL_U8) return (T)row[ky];
        return (T)((sb[slot][g][ky >> 5] >> (ky & 31)) & 1u);
    };

    cx<T> v[LG], tw[LG];
    load_twiddles_gen<T, LG>(tw, twtab, lane, N);
#pragma unroll
    for (int r = 0; r < RA; ++r) v[r] = col[(lane < LA ? lane : 0) + LA * r];
    fft_gen<T, RA, LA, false>(v, tw, scr, lane);             // (its barriers also publish sb)

    const uint8_t* sp = SEL == SEL_U8 ? selT + (size_t)prob * W * N : nullptr;
    if (blockIdx.x == 0) {
        // the packed column c == 0 holds two real-input transforms: separate, weight, re-pack
        __syncthreads();
        if (act) {
#pragma unroll
            for (int r = 0; r < LA; ++r) scr[lane + RA * r] = v[r];
        }
        __syncthreads();
        if (g == 0) {
#pragma unroll
            for (int r = 0; r < LA; ++r) {
                const int ky = ln + RA * r, km = (N - ky) & (N - 1);
                const cx<T> pk = v[r], pm = scr[km];
                const cx<T> A = {(T)0.5 * (pk.x + pm.x), (T)0.5 * (pk.y - pm.y)};
                const cx<T> B = {(T)0.5 * (pk.y + pm.y), (T)-0.5 * (pk.x - pm.x)};
                const T a1 = sel_at(0, 0, ky, sp), a2 = sel_at(0, 0, km, sp);
                const T b1 = sel_at(1, W / 2, ky, sp + (size_t)(W / 2) * N), b2 = sel_at(1, W / 2, km, sp + (size_t)(W / 2) * N);
                const T wA = (T)0.5 * (a1 + a2), wB = (T)0.5 * (b1 + b2);
                v[r] = {wA * A.x - wB * B.y, wA * A.y + wB * B.x};
                if (YT != nullptr) {                             // data term of this selector, built on the fly (k_pack_y)
                    const cx<T>* y0 = YT + (size_t)prob * W * N;
                    const cx<T>* yn = y0 + (size_t)(W / 2) * N;
                    const cx<T> p1 = y0[ky], p2 = y0[km], q1 = yn[ky], q2 = yn[km];
                    const cx<T> ya = {(T)0.5 * (a1 * p1.x + a2 * p2.x), (T)0.5 * (a1 * p1.y - a2 * p2.y)};
                    const cx<T> yb = {(T)0.5 * (b1 * q1.x + b2 * q2.x), (T)0.5 * (b1 * q1.y - b2 * q2.y)};
                    v[r] = csub(v[r], cx<T>{ya.x - yb.y, ya.y + yb.x});
                }
            }
        }
    }
    if (c != 0) {
        const uint8_t* s1 = sp + (size_t)c * N;
        const uint8_t* s2 = sp + (size_t)(W - c) * N;
#pragma unroll
        for (int r = 0; r < LA; ++r) {
            const int ky = ln + RA * r, km = (N - ky) & (N - 1);
            const T w1 = sel_at(0, c, ky, s1), w2 = sel_at(1, W - c, km, s2);
            const T wgt = (T)0.5 * (w1 + w2);
            v[r] = {wgt * v[r].x, wgt * v[r].y};
            if (YT != nullptr) {
                const cx<T> y1 = YT[((size_t)prob * W + c) * N + ky], y2 = YT[((size_t)prob * W + (W - c)) * N + km];
                v[r] = csub(v[r], cx<T>{(T)0.5 * (w1 * y1.x + w2 * y2.x), (T)0.5 * (w1 * y1.y - w2 * y2.y)});
            }
        }
    }
    if (yh != nullptr) {
        const cx<T>* yc = yh + ((size_t)prob * (W / 2) + c) * N;
#pragma unroll
        for (int r = 0; r < LA; ++r) v[r] = csub(v[r], yc[ln + RA * r]);
    }
    fft_gen<T, LA, RA, true>(v, tw, scr, lane);
    if (lane < LA) {
#pragma unroll
        for (int r = 0; r < RA; ++r) col[lane + LA * r] = v[r];
    }
}

// ------------------------------------------------------------------------------- data term
template <typename T>
__global__ void k_pack_y(const cx<T>* __restrict__ YT, const uint8_t* __restrict__ selT, cx<T>* __restrict__ yh, int H, int W) {
    const int prob = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (W / 2) * H) return;
    const int c = i / H, ky = i % H;
    const cx<T>* Y = YT + (size_t)prob * W * H;
    const uint8_t* S = selT + (size_t)prob * W * H;
    auto term = [&](int cc) -> cx<T> {
        const size_t i1 = (size_t)cc * H + ky, i2 = (size_t)((W - cc) % W) * H + ((H - ky) % H);
        const T s1 = (T)S[i1], s2 = (T)S[i2];
        const cx<T> y1 = Y[i1], y2 = Y[i2];
        return {(T)0.5 * (s1 * y1.x + s2 * y2.x), (T)0.5 * (s1 * y1.y - s2 * y2.y)};
    };
    cx<T> o;
    if (c == 0) {
        const cx<T> A = term(0), B = term(W / 2);
        o = {A.x - B.y, A.y + B.x};
    } else {
        o = term(c);
    }
    yh[(size_t)prob * (W / 2) * H + i] = o;
}

__global__ void k_sel_scatter(const int32_t* __restrict__ idx, int n, uint8_t* __restrict__ selT, int H, int W) {
    const int prob = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int i = idx[(size_t)prob * n + j];
    if (i < 0 || i >= H * W) return;
    selT[(size_t)prob * H * W + (size_t)(i % W) * H + i / W] = 1;
}

__global__ void k_sel_transpose(const uint8_t* __restrict__ sel, uint8_t* __restrict__ selT, int H, int W) {
    __shared__ uint8_t tile[32][33];
    const int prob = blockIdx.z;
    const uint8_t* s = sel + (size_t)prob * H * W;
    uint8_t* d = selT + (size_t)prob * H * W;
    int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 32 + threadIdx.y;
    for (int j = 0; j < 32; j += 8)
        if (x < W && y + j < H) tile[threadIdx.y + j][threadIdx.x] = s[(size_t)(y + j) * W + x] != 0;
    __syncthreads();
    x = blockIdx.y * 32 + threadIdx.x;
    y = blockIdx.x * 32 + threadIdx.y;
    for (int j = 0; j < 32; j += 8)
        if (x < H && y + j < W) d[(size_t)(y + j) * H + x] = tile[threadIdx.x][threadIdx.y + j];
}

// ------------------------------------------------------------------------------- mask bits
// uint8 transposed selector [W][H] -> bit-packed [W][H/32] (bit ky & 31 of word [kx][ky >> 5])
__global__ void k_pack_bits(const uint8_t* __restrict__ selT, uint32_t* __restrict__ bitsT, int nwords) {
    const int prob = blockIdx.y;
    const int wd = blockIdx.x * blockDim.x + threadIdx.x;
    if (wd >= nwords) return;
    const uint4* src = reinterpret_cast<const uint4*>(selT + ((size_t)prob * nwords + wd) * 32);
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint4 v = src[q];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) m |= (((w4[j] >> (8 * k)) & 0xFFu) != 0 ? 1u : 0u) << (16 * q + 4 * j + k);
    }
    bitsT[(size_t)prob * nwords + wd] = m;
}

// materialise mask o minibatch as a transposed uint8 selector (tests, explicit-selector callers)
__global__ void k_sel_from_thr(const uint32_t* __restrict__ bitsT, const MbDesc* __restrict__ mbd, uint8_t* __restrict__ selT,
                               int H, int W) {
    const int prob = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;         // transposed flat index kx*H + ky
    if (j >= H * W) return;
    const int kx = j / H, ky = j - kx * H;
    const uint32_t bit = (bitsT[((size_t)prob * W + kx) * (H / 32) + (ky >> 5)] >> (ky & 31)) & 1u;
    const MbDesc d = mbd[prob];
    selT[(size_t)prob * H * W + j] = (bit && mb_member(d, (uint32_t)(ky * W + kx))) ? 1 : 0;
}

template <typename T> void fill_twiddles(std::vector<cx<T>>& tab, int N) {
    tab.resize(N);
    for (int j = 0; j < N; ++j) {
        const double ang = -2.0 * 3.14159265358979323846 * j / N;
        tab[j] = {(T)cos(ang), (T)sin(ang)};
    }
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_csmri_plan_create(pnp_csmri_plan** out, int H, int W, int batch, int dtype) {
    PNP_CHECK_ARG(out != nullptr, "null plan pointer");
    PNP_CHECK_ARG(H == W && (H == 64 || H == 128 || H == 256), "supported sizes: H == W in {64, 128, 256}");
    PNP_CHECK_ARG(batch >= 1, "batch must be >= 1");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "dtype must be PNP_F32 or PNP_F64");
    auto* p = new pnp_csmri_plan{H, W, batch, dtype, H == 256 ? 16 : H == 128 ? 12 : 8, nullptr, nullptr, nullptr, 192};
    if (const char* ev = getenv("PNP_CSMRI_FUSED_MIN_BATCH")) p->fused_min_batch = atoi(ev);
    const size_t esz = dtype == PNP_F32 ? 8 : 16;
    hipError_t e = hipMalloc(&p->work, (size_t)batch * (W / 2) * H * esz);
    if (e == hipSuccess) e = hipMalloc(&p->twtab, (size_t)H * esz);
    if (e == hipSuccess) e = hipMalloc(&p->mbd, (size_t)batch * sizeof(MbDesc));
    if (e == hipSuccess) {
        if (dtype == PNP_F32) {
            std::vector<cx<float>> tab; fill_twiddles(tab, H);
            e = hipMemcpy(p->twtab, tab.data(), H * esz, hipMemcpyHostToDevice);
        } else {
            std::vector<cx<double>> tab; fill_twiddles(tab, H);
            e = hipMemcpy(p->twtab, tab.data(), H * esz, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        set_error(std::string("pnp_csmri_plan_create: ") + hipGetErrorString(e));
        if (p->work) (void)hipFree(p->work);
        if (p->twtab) (void)hipFree(p->twtab);
        if (p->mbd) (void)hipFree(p->mbd);
        delete p;
        return PNP_ERR_HIP;
    }
    *out = p;
    return PNP_OK;
}

extern "C" int pnp_csmri_plan_destroy(pnp_csmri_plan* p) {
    if (p == nullptr) return PNP_OK;
    (void)hipFree(p->work);
    (void)hipFree(p->twtab);
    (void)hipFree(p->mbd);
    delete p;
    return PNP_OK;
}

extern "C" int pnp_csmri_sel_from_indices(pnp_csmri_plan* p, const int32_t* idx, int n, uint8_t* selT, void* stream) {
    PNP_CHECK_ARG(p && idx && selT && n >= 0, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PNP_CHECK_HIP(hipMemsetAsync(selT, 0, (size_t)p->batch * p->H * p->W, s));
    if (n > 0) {
        k_sel_scatter<<<dim3((n + 255) / 256, p->batch), 256, 0, s>>>(idx, n, selT, p->H, p->W);
        PNP_CHECK_LAUNCH();
    }
    return PNP_OK;
}

extern "C" int pnp_csmri_pack_mask(pnp_csmri_plan* p, const uint8_t* selT, uint32_t* bitsT, void* stream) {
    PNP_CHECK_ARG(p && selT && bitsT, "null argument");
    const int nwords = p->W * (p->H / 32);
    k_pack_bits<<<dim3((nwords + 255) / 256, p->batch), 256, 0, (hipStream_t)stream>>>(selT, bitsT, nwords);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_csmri_draw_thresholds(pnp_csmri_plan* p, const uint32_t* bitsT, int mb, uint64_t seed, uint32_t step0,
                                         int nsteps, const uint32_t* step_dev, void* mbd, uint32_t* selbits, void* stream) {
    PNP_CHECK_ARG(p && bitsT && mbd, "null argument");
    PNP_CHECK_ARG(mb >= 1 && mb <= p->H * p->W && nsteps >= 1 && nsteps <= 65535, "need 1 <= mb <= H*W, 1 <= nsteps <= 65535");
    k_draw_thr<true><<<dim3(p->batch, nsteps), 256, 0, (hipStream_t)stream>>>(bitsT, p->H, p->W, mb, seed, step0, step_dev, (MbDesc*)mbd, selbits, draw_fast_path());
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_csmri_draw_thresholds_pp(pnp_csmri_plan* p, const uint32_t* bitsT, const int32_t* mb_vec, const uint32_t* draw_id,
                                            uint64_t seed, uint32_t step0, int nsteps, const uint32_t* step_dev, void* mbd,
                                            uint32_t* selbits, void* stream) {
    PNP_CHECK_ARG(p && bitsT && mb_vec && mbd, "null argument");
    PNP_CHECK_ARG(nsteps >= 1 && nsteps <= 65535, "need 1 <= nsteps <= 65535");
    k_draw_thr_pp<true><<<dim3(p->batch, nsteps), 256, 0, (hipStream_t)stream>>>(bitsT, p->H, p->W, mb_vec, draw_id, seed, step0, step_dev,
                                                                                (MbDesc*)mbd, selbits, draw_fast_path());
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_csmri_sel_from_thresholds(pnp_csmri_plan* p, const uint32_t* bitsT, const void* mbd, uint8_t* selT,
                                             void* stream) {
    PNP_CHECK_ARG(p && bitsT && mbd && selT, "null argument");
    k_sel_from_thr<<<dim3((p->H * p->W + 255) / 256, p->batch), 256, 0, (hipStream_t)stream>>>(bitsT, (const MbDesc*)mbd, selT,
                                                                                                p->H, p->W);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_csmri_draw_minibatch(pnp_csmri_plan* p, const uint32_t* bitsT, int mb, uint64_t seed, uint32_t step,
                                        const uint32_t* step_dev, uint8_t* selT, void* stream) {
    int rc = pnp_csmri_draw_thresholds(p, bitsT, mb, seed, step, 1, step_dev, p ? p->mbd : nullptr, nullptr, stream);
    if (rc != PNP_OK) return rc;
    return pnp_csmri_sel_from_thresholds(p, bitsT, p->mbd, selT, stream);
}

extern "C" int pnp_csmri_sel_from_dense(pnp_csmri_plan* p, const uint8_t* sel, uint8_t* selT, void* stream) {
    PNP_CHECK_ARG(p && sel && selT, "null argument");
    k_sel_transpose<<<dim3((p->W + 31) / 32, (p->H + 31) / 32, p->batch), dim3(32, 8), 0, (hipStream_t)stream>>>(
        sel, selT, p->H, p->W);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_csmri_pack_y(pnp_csmri_plan* p, const void* YT, const uint8_t* selT, void* yh, void* stream) {
    PNP_CHECK_ARG(p && YT && selT && yh, "null argument");
    const int n = (p->W / 2) * p->H;
    dim3 grid((n + 255) / 256, p->batch);
    if (p->dtype == PNP_F32)
        k_pack_y<float><<<grid, 256, 0, (hipStream_t)stream>>>((const cx<float>*)YT, selT, (cx<float>*)yh, p->H, p->W);
    else
        k_pack_y<double><<<grid, 256, 0, (hipStream_t)stream>>>((const cx<double>*)YT, selT, (cx<double>*)yh, p->H, p->W);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

namespace {
template <typename T, int RA, int LA>
int run_grad(pnp_csmri_plan* p, const void* a, const void* b, const uint8_t* selT, const uint32_t* bitsT,
             const void* yh, const void* YT, double alpha, const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2,
             void* out, hipStream_t s, const double* alpha_pp, const double* gamma_pp) {
    constexpr int G = FftSmem<T, RA, LA>::G;
    const int H = p->H, W = p->W;
    cx<T>* work = (cx<T>*)p->work;
    const cx<T>* tw = (const cx<T>*)p->twtab;
    const T scale = (T)(alpha / ((double)H * (double)W));
    k_rows_fwd<T, RA, LA><<<dim3(H / (2 * G), p->batch), 256, 0, s>>>((const T*)a, (const T*)b, work, tw, H);
    PNP_CHECK_LAUNCH();
    const dim3 cg((W / 2) / G, p->batch);
    if (selT != nullptr)
        k_cols<T, RA, LA, SEL_U8><<<cg, 256, 0, s>>>(work, selT, nullptr, (const cx<T>*)yh, (const cx<T>*)YT, tw, W);
    else
        k_cols<T, RA, LA, SEL_BITS><<<cg, 256, 0, s>>>(work, nullptr, bitsT, (const cx<T>*)yh, (const cx<T>*)YT, tw, W);
    PNP_CHECK_LAUNCH();
    if (alpha_pp != nullptr || gamma_pp != nullptr)
        k_rows_inv_pp<T, RA, LA><<<dim3(H / (2 * G), p->batch), 256, 0, s>>>(work, tw, H, scale, alpha_pp, 1.0 / ((double)H * (double)W),
                                                                        (const T*)alpha_vec, (T)beta, (const T*)c1, (T)gamma, gamma_pp,
                                                                        (const T*)c2, (T*)out);
    else
        k_rows_inv<T, RA, LA><<<dim3(H / (2 * G), p->batch), 256, 0, s>>>(work, tw, H, scale, (const T*)alpha_vec, (T)beta,
                                                                     (const T*)c1, (T)gamma, (const T*)c2, (T*)out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}
}  // namespace

static int grad_sel_impl(pnp_csmri_plan* p, const void* a, const void* b, const uint8_t* selT, const uint32_t* bitsT,
                         const void* yh, const void* YT, double alpha, const double* alpha_pp, const void* alpha_vec,
                         double beta, const void* c1, double gamma, const double* gamma_pp, const void* c2, void* out, void* stream) {
    PNP_CHECK_ARG(p && a && out, "null argument");
    PNP_CHECK_ARG(!(yh != nullptr && YT != nullptr), "pass the packed data term (yh) or the raw data (YT), not both");
    PNP_CHECK_ARG((selT != nullptr) != (bitsT != nullptr), "pass either an explicit selector (selT) or mask bits (bitsT)");
    // large f32 256 x 256 batches with a bit-packed selector: the three passes in ONE kernel, the spectrum never in HBM
    // (csmri_fused.hip; one workgroup per image, so it needs about a workgroup per CU to pay off)
    if (p->dtype == PNP_F32 && p->H == 256 && bitsT != nullptr && YT == nullptr && p->batch >= p->fused_min_batch)
        return csmri_fused_launch(p->batch, p->twtab, a, b, bitsT, yh, alpha, alpha_vec, beta, c1, gamma, c2, out, FUSED_GRAD, 1.0, 0.0,
                                  nullptr, nullptr, nullptr, stream, nullptr, nullptr, alpha_pp, gamma_pp, nullptr);
    hipStream_t s = (hipStream_t)stream;
#define PNP_CS_ARGS p, a, b, selT, bitsT, yh, YT, alpha, alpha_vec, beta, c1, gamma, c2, out, s, alpha_pp, gamma_pp
    if (p->dtype == PNP_F32) {
        if (p->NL == 16) return run_grad<float, 16, 16>(PNP_CS_ARGS);
        if (p->NL == 12) return run_grad<float, 8, 16>(PNP_CS_ARGS);
        return run_grad<float, 8, 8>(PNP_CS_ARGS);
    }
    if (p->NL == 16) return run_grad<double, 16, 16>(PNP_CS_ARGS);
    if (p->NL == 12) return run_grad<double, 8, 16>(PNP_CS_ARGS);
    return run_grad<double, 8, 8>(PNP_CS_ARGS);
#undef PNP_CS_ARGS
}

extern "C" int pnp_csmri_grad_sel(pnp_csmri_plan* p, const void* a, const void* b, const uint8_t* selT, const uint32_t* bitsT,
                                  const void* yh, const void* YT, double alpha, const void* alpha_vec,
                                  double beta, const void* c1, double gamma, const void* c2, void* out, void* stream) {
    return grad_sel_impl(p, a, b, selT, bitsT, yh, YT, alpha, nullptr, alpha_vec, beta, c1, gamma, nullptr, c2, out, stream);
}

extern "C" int pnp_csmri_grad_sel_pp(pnp_csmri_plan* p, const void* a, const void* b, const uint8_t* selT, const uint32_t* bitsT,
                                     const void* yh, const void* YT, double alpha, const double* alpha_pp, const void* alpha_vec,
                                     double beta, const void* c1, double gamma, const double* gamma_pp, const void* c2, void* out,
                                     void* stream) {
    return grad_sel_impl(p, a, b, selT, bitsT, yh, YT, alpha, alpha_pp, alpha_vec, beta, c1, gamma, gamma_pp, c2, out, stream);
}

extern "C" int pnp_csmri_grad(pnp_csmri_plan* p, const void* a, const void* b, const uint8_t* selT, const void* yh,
                              double alpha, double beta, const void* c1, double gamma, const void* c2, void* out,
                              void* stream) {
    PNP_CHECK_ARG(selT != nullptr, "null selector");
    return pnp_csmri_grad_sel(p, a, b, selT, nullptr, yh, nullptr, alpha, nullptr, beta, c1, gamma, c2, out, stream);
}

// ---- whole inner iteration in one kernel (csmri_fused.hip)
// `int denoise` of the step entry points -> the kernel's MODE: 0 = store the stepped image (FUSED_NO_DENOISE), 2 = the 2-D wavelet prox
// (FUSED_FULL_W2D), any other value = the per-column prox (FUSED_FULL)
static inline int fused_mode(int denoise) { return denoise == 0 ? FUSED_NO_DENOISE : (denoise == 2 ? FUSED_FULL_W2D : FUSED_FULL); }

// The argument checks the entry points below share.  Macros, not functions: a refusal names the function that made it (PNP_CHECK_ARG's
// __func__) and callers see that text, so a check expands inside the function that answers.  The _AS forms are for an _impl that answers
// in the name of the public entry point that called it: it is handed that name (`who`).
#define PNP_CHECK_ARG_AS(who, cond, msg) \
    do { if (!(cond)) { pnp::set_error(std::string(who) + ": " + (msg)); return PNP_ERR_ARG; } } while (0)
#define PNP_CHECK_ONE_KERNEL_PLAN_AS(who, p) \
    PNP_CHECK_ARG_AS(who, (p)->dtype == PNP_F32 && (p)->H == 256 && (p)->W == 256, "the one-kernel iteration exists for f32 plans of 256 x 256")
#define PNP_CHECK_ONE_KERNEL_PLAN(p) PNP_CHECK_ONE_KERNEL_PLAN_AS(__func__, p)
#define PNP_CHECK_SSE_XREC_AS(who, sse, xrec) PNP_CHECK_ARG_AS(who, !((sse) && !(xrec)), "sse_out needs xrec")
#define PNP_CHECK_SSE_XREC(sse, xrec) PNP_CHECK_SSE_XREC_AS(__func__, sse, xrec)
#define PNP_CHECK_OWN_BUFFERS3_AS(who, z, w, mu) \
    PNP_CHECK_ARG_AS(who, (z) != (w) && (z) != (mu) && (w) != (mu), "z, w and mu must be buffers of their own")
#define PNP_CHECK_OWN_BUFFERS3(z, w, mu) PNP_CHECK_OWN_BUFFERS3_AS(__func__, z, w, mu)
#define PNP_CHECK_OWN_BUFFERS4(z, wp, wn, vp)                                                                                      \
    PNP_CHECK_ARG((z) != (wp) && (z) != (wn) && (z) != (vp) && (wp) != (wn) && (wp) != (vp) && (wn) != (vp),                        \
                  "z, w_prev, w_next and v_prev must be buffers of their own")
// the n-step forms: n_steps log rows from log_row0 on (an int in the kernel), and a prox they hold
#define PNP_CHECK_LOG_RANGE(n_steps, n_log, log_row0) \
    PNP_CHECK_ARG((n_steps) >= 1 && (n_log) >= 1 && (log_row0) >= 0 && (log_row0) <= INT32_MAX - (n_steps), "bad n_steps / log")
#define PNP_CHECK_SPAN_DENOISE(denoise) do {                                                                                       \
    PNP_CHECK_ARG((denoise) != 0, "the span kernels hold the TV prox: denoise must be != 0");                                      \
    PNP_CHECK_ARG((denoise) != 2, "the span kernels hold the per-column prox only: denoise = 2 (the 2-D wavelet prox) is not accepted"); \
} while (0)
// the per-problem-T2 spans (pnp_csmri_svrg_span_pp, pnp_csmri_sarah_span_pp)
#define PNP_CHECK_SPAN_RANGE(step0, n_steps, T2, t2_vec, mini_batch_size, mb_vec, n_log, log_row0) do {                            \
    PNP_CHECK_ARG((n_steps) >= 1 && (step0) >= 0 && (step0) <= INT32_MAX - (n_steps), "bad step0 / n_steps");                      \
    PNP_CHECK_ARG((t2_vec) != nullptr || (T2) >= 1, "bad T2: a scalar T2 >= 1 or a t2_vec");                                       \
    PNP_CHECK_ARG(((mb_vec) != nullptr || (mini_batch_size) >= 1) && (n_log) >= 1 && (log_row0) >= 0 &&                            \
                  (log_row0) <= INT32_MAX - (n_steps), "bad mini_batch_size / log");                                               \
} while (0)

// [x, x + nx) and [y, y + ny) share a byte (a NULL buffer shares none)
static bool overlap(const void* x, size_t nx, const void* y, size_t ny) {
    const uintptr_t a0 = (uintptr_t)x, b0 = (uintptr_t)y;
    return x != nullptr && y != nullptr && a0 < b0 + ny && b0 < a0 + nx;
}

static int svrg_step_impl(const char* who, pnp_csmri_plan* p, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                          const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, double gamma,
                          const double* gamma_pp, const void* c2, void* out, int denoise, double sigma_modifier,
                          const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out,
                          void* stream) {
    PNP_CHECK_ARG_AS(who, p && a && bitsT && out, "null argument");
    PNP_CHECK_ONE_KERNEL_PLAN_AS(who, p);
    PNP_CHECK_SSE_XREC_AS(who, sse_out, xrec);
    return csmri_fused_launch(p->batch, p->twtab, a, b, bitsT, nullptr, alpha, alpha_vec, beta, c1, gamma, c2, out, fused_mode(denoise),
                              sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, nullptr, nullptr, alpha_pp, gamma_pp,
                              sigma_modifier_pp);
}

extern "C" int pnp_csmri_svrg_step(pnp_csmri_plan* p, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                                   const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2, void* out,
                                   int denoise, double sigma_modifier, double fallback_sigma, const void* xrec,
                                   double* sse_out, void* sigma_out, void* stream) {
    return svrg_step_impl(__func__, p, a, b, bitsT, alpha, nullptr, alpha_vec, beta, c1, gamma, nullptr, c2, out, denoise, sigma_modifier,
                          nullptr, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

extern "C" int pnp_csmri_svrg_step_pp(pnp_csmri_plan* p, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                                      const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, double gamma,
                                      const double* gamma_pp, const void* c2, void* out, int denoise, double sigma_modifier,
                                      const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_out,
                                      void* sigma_out, void* stream) {
    return svrg_step_impl(__func__, p, a, b, bitsT, alpha, alpha_pp, alpha_vec, beta, c1, gamma, gamma_pp, c2, out, denoise,
                          sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

// ---- the SARAH form of the one-kernel iteration: v_out stored from the epilogue, then out = prox_TV(c2 + gamma * v_out), out2 = out
static int sarah_step_impl(pnp_csmri_plan* p, const void* a, const void* b, const uint32_t* bitsT, double alpha, const double* alpha_pp,
                           const void* alpha_vec, double beta, const void* c1, double gamma, const double* gamma_pp, const void* c2,
                           void* v_out, void* out, void* out2, int denoise, double sigma_modifier, const double* sigma_modifier_pp,
                           double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(p && a && b && bitsT && c1 && c2 && v_out && out, "null argument");
    PNP_CHECK_SSE_XREC(sse_out, xrec);
    PNP_CHECK_ARG(denoise || out2 == nullptr, "out2 needs denoise != 0 (without the prox the stored image is not the iterate)");
    PNP_CHECK_ARG(v_out != a && v_out != b && v_out != c2 && v_out != out && v_out != out2,
                  "v_out may alias c1 only (not a, b, c2, out or out2)");
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    return csmri_sarah_launch(p->batch, p->twtab, a, b, bitsT, alpha, alpha_vec, beta, c1, gamma, c2, v_out, out, out2, fused_mode(denoise),
                              sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, alpha_pp, gamma_pp, sigma_modifier_pp);
}

extern "C" int pnp_csmri_sarah_step(pnp_csmri_plan* p, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                                    const void* alpha_vec, double beta, const void* c1, double gamma, const void* c2, void* v_out,
                                    void* out, void* out2, int denoise, double sigma_modifier, double fallback_sigma, const void* xrec,
                                    double* sse_out, void* sigma_out, void* stream) {
    return sarah_step_impl(p, a, b, bitsT, alpha, nullptr, alpha_vec, beta, c1, gamma, nullptr, c2, v_out, out, out2, denoise,
                           sigma_modifier, nullptr, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

extern "C" int pnp_csmri_sarah_step_pp(pnp_csmri_plan* p, const void* a, const void* b, const uint32_t* bitsT, double alpha,
                                       const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, double gamma,
                                       const double* gamma_pp, const void* c2, void* v_out, void* out, void* out2, int denoise,
                                       double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                       double* sse_out, void* sigma_out, void* stream) {
    return sarah_step_impl(p, a, b, bitsT, alpha, alpha_pp, alpha_vec, beta, c1, gamma, gamma_pp, c2, v_out, out, out2, denoise,
                           sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

// ---- one GD or SGD inner iteration in one kernel: out = prox_TV(alpha * alpha_vec[b] * Re ifft2(sel o fft2(a) - sel o Y) + beta * c1).
// yh (the data term packed for bitsT: the GD step on the mask) takes the existing instantiations with one epilogue operand; YT (the
// raw data, masked by bitsT inside the kernel: the SGD step on a drawn slot) takes k_grad_step.
static int grad_step_impl(pnp_csmri_plan* p, const void* a, const uint32_t* bitsT, const void* yh, const void* YT, double alpha,
                          const double* alpha_pp, const void* alpha_vec, double beta, const void* c1, void* out, int denoise,
                          double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                          double* sse_out, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(p && a && bitsT && c1 && out, "null argument");
    PNP_CHECK_ARG((yh != nullptr) != (YT != nullptr), "pass the packed data term (yh) or the raw data (YT), exactly one of them");
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    PNP_CHECK_SSE_XREC(sse_out, xrec);
    if (yh != nullptr)
        return csmri_fused_launch(p->batch, p->twtab, a, nullptr, bitsT, yh, alpha, alpha_vec, beta, c1, 0.0, nullptr, out,
                                  fused_mode(denoise), sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, nullptr, nullptr,
                                  alpha_pp, nullptr, sigma_modifier_pp);
    return csmri_minibatch_launch(p->batch, p->twtab, a, bitsT, YT, alpha, alpha_vec, beta, c1, nullptr, nullptr, nullptr, nullptr, 0.0,
                                  0.0, out, fused_mode(denoise), sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, alpha_pp,
                                  nullptr, sigma_modifier_pp);
}

extern "C" int pnp_csmri_grad_step(pnp_csmri_plan* p, const void* a, const uint32_t* bitsT, const void* yh, const void* YT, double alpha,
                                   const void* alpha_vec, double beta, const void* c1, void* out, int denoise, double sigma_modifier,
                                   double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out, void* stream) {
    return grad_step_impl(p, a, bitsT, yh, YT, alpha, nullptr, alpha_vec, beta, c1, out, denoise, sigma_modifier, nullptr, fallback_sigma,
                          xrec, sse_out, sigma_out, stream);
}

extern "C" int pnp_csmri_grad_step_pp(pnp_csmri_plan* p, const void* a, const uint32_t* bitsT, const void* yh, const void* YT,
                                      double alpha, const double* alpha_pp, const void* alpha_vec, double beta, const void* c1,
                                      void* out, int denoise, double sigma_modifier, const double* sigma_modifier_pp,
                                      double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out, void* stream) {
    return grad_step_impl(p, a, bitsT, yh, YT, alpha, alpha_pp, alpha_vec, beta, c1, out, denoise, sigma_modifier, sigma_modifier_pp,
                          fallback_sigma, xrec, sse_out, sigma_out, stream);
}

// ---- one whole SAGA inner iteration in one kernel: minibatch gradient with its data term, table update, step, prox
static int saga_step_impl(pnp_csmri_plan* p, const void* z, const uint32_t* bitsT, const void* YT, double alpha, const double* alpha_pp,
                          const void* alpha_vec, void* table, const int32_t* row, const int32_t* prev_row, void* sum, double lr,
                          const double* lr_pp, double inv_hist, int hist, void* out, int denoise, double sigma_modifier,
                          const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out,
                          void* stream, bool hist_form = false, const double* inv_hist_pp = nullptr) {
    PNP_CHECK_ARG(p && z && bitsT && YT && table && row && prev_row && sum && out, "null argument");
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    PNP_CHECK_SSE_XREC(sse_out, xrec);
    PNP_CHECK_ARG(hist >= 1, "need hist >= 1");
    PNP_CHECK_ARG(!(hist_form && denoise == 2), "the per-problem-divisor form holds the per-column prox only: denoise = 2 is not accepted");
    {   // table [hist][batch][H][W] and sum [batch][H][W] are written while z, out and xrec are read or written: no overlap
        const size_t img = (size_t)p->batch * 256 * 256 * sizeof(float);
        const size_t tb = img * (size_t)hist;
        PNP_CHECK_ARG(!overlap(table, tb, z, img) && !overlap(table, tb, out, img) && !overlap(table, tb, xrec, img) &&
                      !overlap(sum, img, z, img) && !overlap(sum, img, out, img) && !overlap(sum, img, xrec, img) &&
                      !overlap(table, tb, sum, img), "table and sum must not alias z, out, xrec or each other");
    }
    if (hist_form)                                              // the kernels that take the divisor per problem (NULL: the scalar)
        return csmri_saga_hist_launch(p->batch, p->twtab, z, bitsT, YT, alpha, alpha_vec, table, row, prev_row, sum, lr, inv_hist, out,
                                      fused_mode(denoise), sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, alpha_pp, lr_pp,
                                      sigma_modifier_pp, inv_hist_pp, 0, 0, 1);
    return csmri_minibatch_launch(p->batch, p->twtab, z, bitsT, YT, alpha, alpha_vec, 0.0, nullptr, table, row, prev_row, sum, lr, inv_hist,
                                  out, fused_mode(denoise), sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, alpha_pp, lr_pp,
                                  sigma_modifier_pp);
}

extern "C" int pnp_csmri_saga_step(pnp_csmri_plan* p, const void* z, const uint32_t* bitsT, const void* YT, double alpha,
                                   const void* alpha_vec, void* table, const int32_t* row, const int32_t* prev_row, void* sum, double lr,
                                   double inv_hist, int hist, void* out, int denoise, double sigma_modifier, double fallback_sigma,
                                   const void* xrec, double* sse_out, void* sigma_out, void* stream) {
    return saga_step_impl(p, z, bitsT, YT, alpha, nullptr, alpha_vec, table, row, prev_row, sum, lr, nullptr, inv_hist, hist, out, denoise,
                          sigma_modifier, nullptr, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

extern "C" int pnp_csmri_saga_step_pp(pnp_csmri_plan* p, const void* z, const uint32_t* bitsT, const void* YT, double alpha,
                                      const double* alpha_pp, const void* alpha_vec, void* table, const int32_t* row,
                                      const int32_t* prev_row, void* sum, double lr, const double* lr_pp, double inv_hist, int hist,
                                      void* out, int denoise, double sigma_modifier, const double* sigma_modifier_pp,
                                      double fallback_sigma, const void* xrec, double* sse_out, void* sigma_out, void* stream) {
    return saga_step_impl(p, z, bitsT, YT, alpha, alpha_pp, alpha_vec, table, row, prev_row, sum, lr, lr_pp, inv_hist, hist, out, denoise,
                          sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

// ---- pnp_csmri_saga_step_pp with the divisor per problem: inv_hist_pp double [batch], NULL = the scalar; hist = the table's row count
extern "C" int pnp_csmri_saga_step_hist_pp(pnp_csmri_plan* p, const void* z, const uint32_t* bitsT, const void* YT, double alpha,
                                           const double* alpha_pp, const void* alpha_vec, void* table, const int32_t* row,
                                           const int32_t* prev_row, void* sum, double lr, const double* lr_pp, double inv_hist,
                                           const double* inv_hist_pp, int hist, void* out, int denoise, double sigma_modifier,
                                           const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_out,
                                           void* sigma_out, void* stream) {
    return saga_step_impl(p, z, bitsT, YT, alpha, alpha_pp, alpha_vec, table, row, prev_row, sum, lr, lr_pp, inv_hist, hist, out, denoise,
                          sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_out, sigma_out, stream, true, inv_hist_pp);
}

// ---- the same with the outer-loop refresh folded in (first inner iteration of an outer iteration); lr_pp, sigma_modifier_pp: double
// [batch], NULL = the scalar
static int svrg_outer_step_impl(const char* who, pnp_csmri_plan* p, const void* z, const uint32_t* mask_bitsT, const void* yh,
                                const void* alpha_vec, double lr, const double* lr_pp, void* w_out, void* mu_out, void* out, int denoise,
                                double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                double* sse_out, void* sigma_out, void* stream) {
    PNP_CHECK_ARG_AS(who, p && z && mask_bitsT && yh && w_out && mu_out && out, "null argument");
    PNP_CHECK_ONE_KERNEL_PLAN_AS(who, p);
    PNP_CHECK_SSE_XREC_AS(who, sse_out, xrec);
    PNP_CHECK_ARG_AS(who, w_out != z && mu_out != z && w_out != mu_out && w_out != out && mu_out != out,
                     "w_out and mu_out must be buffers of their own");
    return csmri_fused_launch(p->batch, p->twtab, z, nullptr, mask_bitsT, yh, 1.0, alpha_vec, 1.0, z, -lr, nullptr, out,
                              fused_mode(denoise), sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream, w_out, mu_out, nullptr,
                              lr_pp, sigma_modifier_pp);
}

extern "C" int pnp_csmri_svrg_outer_step(pnp_csmri_plan* p, const void* z, const uint32_t* mask_bitsT, const void* yh,
                                         const void* alpha_vec, double lr, void* w_out, void* mu_out, void* out, int denoise,
                                         double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_out,
                                         void* sigma_out, void* stream) {
    return svrg_outer_step_impl(__func__, p, z, mask_bitsT, yh, alpha_vec, lr, nullptr, w_out, mu_out, out, denoise, sigma_modifier,
                                nullptr, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

extern "C" int pnp_csmri_svrg_outer_step_pp(pnp_csmri_plan* p, const void* z, const uint32_t* mask_bitsT, const void* yh,
                                            const void* alpha_vec, double lr, const double* lr_pp, void* w_out, void* mu_out, void* out,
                                            int denoise, double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma,
                                            const void* xrec, double* sse_out, void* sigma_out, void* stream) {
    return svrg_outer_step_impl(__func__, p, z, mask_bitsT, yh, alpha_vec, lr, lr_pp, w_out, mu_out, out, denoise, sigma_modifier,
                                sigma_modifier_pp, fallback_sigma, xrec, sse_out, sigma_out, stream);
}

// ---- a whole outer iteration (refresh + T2 inner iterations) in one launch; lr_pp, sigma_modifier_pp: double [batch], mb_vec: int32
// [batch], NULL = the scalar.  w2d: the 2-D wavelet prox in every iteration instead of the per-column one
static int svrg_outer_iteration_impl(const char* who, pnp_csmri_plan* p, void* z, void* w, void* mu, const uint32_t* mask_bitsT,
                                     const void* yh, const void* alpha_vec, const uint32_t* selbits, int T2, double lr,
                                     const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                     const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_log,
                                     int log_row0, int n_log, void* sigma_out, bool w2d, void* stream) {
    PNP_CHECK_ARG_AS(who, p && z && w && mu && mask_bitsT && yh && alpha_vec && xrec && sse_log && sigma_out, "null argument");
    PNP_CHECK_ONE_KERNEL_PLAN_AS(who, p);
    PNP_CHECK_ARG_AS(who, T2 >= 1 && (T2 == 1 || selbits != nullptr) && (mb_vec != nullptr || mini_batch_size >= 1) && n_log >= 1 &&
                     log_row0 >= 0, "bad T2 / selbits / mini_batch_size / log");
    PNP_CHECK_OWN_BUFFERS3_AS(who, z, w, mu);
    if (w2d)
        return csmri_fused_outer_w2d_launch(p->batch, p->twtab, z, w, mu, mask_bitsT, yh, alpha_vec, selbits, T2, lr, lr_pp,
                                            mini_batch_size, mb_vec, sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_log,
                                            log_row0, n_log, sigma_out, stream);
    return csmri_fused_outer_launch(p->batch, p->twtab, z, w, mu, mask_bitsT, yh, alpha_vec, selbits, T2, lr, mini_batch_size,
                                    sigma_modifier, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out, stream, lr_pp, mb_vec,
                                    sigma_modifier_pp);
}

extern "C" int pnp_csmri_svrg_outer_iteration(pnp_csmri_plan* p, void* z, void* w, void* mu, const uint32_t* mask_bitsT, const void* yh,
                                              const void* alpha_vec, const uint32_t* selbits, int T2, double lr, int mini_batch_size,
                                              double sigma_modifier, double fallback_sigma, const void* xrec, double* sse_log,
                                              int log_row0, int n_log, void* sigma_out, void* stream) {
    return svrg_outer_iteration_impl(__func__, p, z, w, mu, mask_bitsT, yh, alpha_vec, selbits, T2, lr, nullptr, mini_batch_size, nullptr,
                                     sigma_modifier, nullptr, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out, false, stream);
}

extern "C" int pnp_csmri_svrg_outer_iteration_pp(pnp_csmri_plan* p, void* z, void* w, void* mu, const uint32_t* mask_bitsT, const void* yh,
                                                 const void* alpha_vec, const uint32_t* selbits, int T2, double lr, const double* lr_pp,
                                                 int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                                 const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                                 double* sse_log, int log_row0, int n_log, void* sigma_out, void* stream) {
    return svrg_outer_iteration_impl(__func__, p, z, w, mu, mask_bitsT, yh, alpha_vec, selbits, T2, lr, lr_pp, mini_batch_size, mb_vec,
                                     sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out, false,
                                     stream);
}

// ---- pnp_csmri_svrg_outer_iteration_pp with the prox kind: denoise = 1 IS that call (the per-column prox; it answers a bad argument
// in that call's name); denoise = 2 runs the 2-D wavelet prox in every iteration -- the outer step and the T2 - 1 inner steps with
// denoise = 2, bit for bit
extern "C" int pnp_csmri_svrg_outer_iteration_prox(pnp_csmri_plan* p, void* z, void* w, void* mu, const uint32_t* mask_bitsT,
                                                   const void* yh, const void* alpha_vec, const uint32_t* selbits, int T2, double lr,
                                                   const double* lr_pp, int mini_batch_size, const int32_t* mb_vec,
                                                   double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma,
                                                   const void* xrec, double* sse_log, int log_row0, int n_log, void* sigma_out,
                                                   int denoise, void* stream) {
    PNP_CHECK_ARG(denoise == 1 || denoise == 2, "denoise must be 1 (the per-column prox) or 2 (the 2-D wavelet prox)");
    return svrg_outer_iteration_impl(denoise == 1 ? "pnp_csmri_svrg_outer_iteration_pp" : __func__, p, z, w, mu, mask_bitsT, yh, alpha_vec,
                                     selbits, T2, lr, lr_pp, mini_batch_size, mb_vec, sigma_modifier, sigma_modifier_pp, fallback_sigma,
                                     xrec, sse_log, log_row0, n_log, sigma_out, denoise == 2, stream);
}

// ---- n_steps inner iterations in one launch, every problem refreshing by its own T2 (t2_vec: int32 [batch]; NULL = the scalar)
extern "C" int pnp_csmri_svrg_span_pp(pnp_csmri_plan* p, void* z, void* w, void* mu, const uint32_t* mask_bitsT, const void* yh,
                                      const void* alpha_vec, const uint32_t* selbits, int step0, int n_steps, int T2,
                                      const int32_t* t2_vec, double lr, const double* lr_pp, int mini_batch_size, const int32_t* mb_vec,
                                      double sigma_modifier, const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                      double* sse_log, int log_row0, int n_log, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(p && z && w && mu && mask_bitsT && yh && alpha_vec && selbits && xrec && sse_log && sigma_out, "null argument");
    PNP_CHECK_SPAN_RANGE(step0, n_steps, T2, t2_vec, mini_batch_size, mb_vec, n_log, log_row0);
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    PNP_CHECK_OWN_BUFFERS3(z, w, mu);
    return csmri_fused_span_launch(p->batch, p->twtab, z, w, mu, mask_bitsT, yh, alpha_vec, selbits, step0, n_steps, T2, t2_vec, lr, lr_pp,
                                   mini_batch_size, mb_vec, sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_log, log_row0,
                                   n_log, sigma_out, stream);
}

// ---- a whole SARAH outer iteration (outer step + T2 inner iterations, TV prox, T2 + 1 log rows) in one launch
static int sarah_outer_impl(pnp_csmri_plan* p, void* z, void* w_prev, void* w_next, void* v_prev, const uint32_t* mask_bitsT,
                            const void* yh, const void* alpha_vec, const uint32_t* selbits, int T2, double eta, const double* eta_pp,
                            double lr, const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                            const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_log, int log_row0,
                            int n_log, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(p && z && w_prev && w_next && v_prev && mask_bitsT && yh && alpha_vec && selbits && xrec && sse_log && sigma_out,
                  "null argument");
    PNP_CHECK_ARG(T2 >= 1 && T2 <= INT32_MAX - 1 && (mb_vec != nullptr || mini_batch_size >= 1) && n_log >= 1 && log_row0 >= 0 &&
                  log_row0 <= INT32_MAX - 1 - T2, "bad T2 / mini_batch_size / log");
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    PNP_CHECK_OWN_BUFFERS4(z, w_prev, w_next, v_prev);
    return csmri_sarah_outer_launch(p->batch, p->twtab, z, w_prev, w_next, v_prev, mask_bitsT, yh, alpha_vec, selbits, T2, eta, eta_pp, lr,
                                    lr_pp, mini_batch_size, mb_vec, sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_log,
                                    log_row0, n_log, sigma_out, stream);
}

extern "C" int pnp_csmri_sarah_outer_iteration(pnp_csmri_plan* p, void* z, void* w_prev, void* w_next, void* v_prev,
                                               const uint32_t* mask_bitsT, const void* yh, const void* alpha_vec, const uint32_t* selbits,
                                               int T2, double eta, double lr, int mini_batch_size, double sigma_modifier,
                                               double fallback_sigma, const void* xrec, double* sse_log, int log_row0, int n_log,
                                               void* sigma_out, void* stream) {
    PNP_CHECK_ARG(mini_batch_size >= 1, "bad T2 / mini_batch_size / log");
    return sarah_outer_impl(p, z, w_prev, w_next, v_prev, mask_bitsT, yh, alpha_vec, selbits, T2, eta, nullptr, lr, nullptr,
                            mini_batch_size, nullptr, sigma_modifier, nullptr, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out,
                            stream);
}

extern "C" int pnp_csmri_sarah_outer_iteration_pp(pnp_csmri_plan* p, void* z, void* w_prev, void* w_next, void* v_prev,
                                                  const uint32_t* mask_bitsT, const void* yh, const void* alpha_vec,
                                                  const uint32_t* selbits, int T2, double eta, const double* eta_pp, double lr,
                                                  const double* lr_pp, int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                                  const double* sigma_modifier_pp, double fallback_sigma, const void* xrec,
                                                  double* sse_log, int log_row0, int n_log, void* sigma_out, void* stream) {
    return sarah_outer_impl(p, z, w_prev, w_next, v_prev, mask_bitsT, yh, alpha_vec, selbits, T2, eta, eta_pp, lr, lr_pp, mini_batch_size,
                            mb_vec, sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out, stream);
}

// ---- n_steps SARAH inner iterations in one launch, every problem taking its outer step by its own T2 (t2_vec: int32 [batch]; NULL =
// the scalar); the outer steps' squared errors go to a ring of their own, NaN where a problem took none
extern "C" int pnp_csmri_sarah_span_pp(pnp_csmri_plan* p, void* z, void* w_prev, void* w_next, void* v_prev, const uint32_t* mask_bitsT,
                                       const void* yh, const void* alpha_vec, const uint32_t* selbits, int step0, int n_steps, int T2,
                                       const int32_t* t2_vec, double eta, const double* eta_pp, double lr, const double* lr_pp,
                                       int mini_batch_size, const int32_t* mb_vec, double sigma_modifier,
                                       const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, double* sse_log,
                                       double* outer_log, int log_row0, int n_log, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(p && z && w_prev && w_next && v_prev && mask_bitsT && yh && alpha_vec && selbits && xrec && sse_log && outer_log &&
                  sigma_out, "null argument");
    PNP_CHECK_SPAN_RANGE(step0, n_steps, T2, t2_vec, mini_batch_size, mb_vec, n_log, log_row0);
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    PNP_CHECK_OWN_BUFFERS4(z, w_prev, w_next, v_prev);
    PNP_CHECK_ARG(sse_log != outer_log, "sse_log and outer_log must be rings of their own");
    return csmri_sarah_span_launch(p->batch, p->twtab, z, w_prev, w_next, v_prev, mask_bitsT, yh, alpha_vec, selbits, step0, n_steps, T2,
                                   t2_vec, eta, eta_pp, lr, lr_pp, mini_batch_size, mb_vec, sigma_modifier, sigma_modifier_pp,
                                   fallback_sigma, xrec, sse_log, outer_log, log_row0, n_log, sigma_out, stream);
}

// ---- n_steps GD or SGD inner iterations in one launch, z in place (yh: the GD form on the mask; YT: the SGD form on n_steps drawn slots)
extern "C" int pnp_csmri_grad_span(pnp_csmri_plan* p, void* z, const uint32_t* bitsT, const void* yh, const void* YT, double alpha,
                                   const double* alpha_pp, const void* alpha_vec, double beta, int denoise, double sigma_modifier,
                                   const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps, double* sse_log,
                                   int log_row0, int n_log, void* sigma_out, void* stream) {
    PNP_CHECK_ARG(p && z && bitsT && xrec && sse_log && sigma_out, "null argument");
    PNP_CHECK_ARG((yh != nullptr) != (YT != nullptr), "pass the packed data term (yh) or the raw data (YT), exactly one of them");
    PNP_CHECK_LOG_RANGE(n_steps, n_log, log_row0);
    PNP_CHECK_SPAN_DENOISE(denoise);
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    return csmri_step_span_launch(p->batch, p->twtab, z, bitsT, yh, YT, alpha, alpha_vec, beta, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0,
                                  n_steps, sigma_modifier, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out, stream, alpha_pp,
                                  nullptr, sigma_modifier_pp);
}

// ---- n_steps SAGA inner iterations in one launch; table, sum and z in place
static int saga_span_impl(pnp_csmri_plan* p, void* z, const uint32_t* bitsT, const void* YT, double alpha, const double* alpha_pp,
                          const void* alpha_vec, void* table, const int32_t* rows, const int32_t* prev_row0, void* sum, double lr,
                          const double* lr_pp, double inv_hist, int hist, int denoise, double sigma_modifier,
                          const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps, double* sse_log,
                          int log_row0, int n_log, void* sigma_out, void* stream, bool hist_form, const double* inv_hist_pp) {
    PNP_CHECK_ARG(p && z && bitsT && YT && table && rows && prev_row0 && sum && xrec && sse_log && sigma_out, "null argument");
    PNP_CHECK_ARG(hist >= 1, "need hist >= 1");
    PNP_CHECK_LOG_RANGE(n_steps, n_log, log_row0);
    PNP_CHECK_SPAN_DENOISE(denoise);
    PNP_CHECK_ONE_KERNEL_PLAN(p);
    {   // as pnp_csmri_saga_step: table [hist][batch][H][W] and sum [batch][H][W] are written while z and xrec are read or written
        const size_t img = (size_t)p->batch * 256 * 256 * sizeof(float);
        const size_t tb = img * (size_t)hist;
        PNP_CHECK_ARG(!overlap(table, tb, z, img) && !overlap(table, tb, xrec, img) && !overlap(sum, img, z, img) &&
                      !overlap(sum, img, xrec, img) && !overlap(table, tb, sum, img), "table and sum must not alias z, xrec or each other");
    }
    if (hist_form)                                              // the kernel that takes the divisor per problem (NULL: the scalar)
        return csmri_saga_hist_launch(p->batch, p->twtab, z, bitsT, YT, alpha, alpha_vec, table, rows, prev_row0, sum, lr, inv_hist, z, 0,
                                      sigma_modifier, fallback_sigma, xrec, sse_log, sigma_out, stream, alpha_pp, lr_pp, sigma_modifier_pp,
                                      inv_hist_pp, n_steps, log_row0, n_log);
    return csmri_step_span_launch(p->batch, p->twtab, z, bitsT, nullptr, YT, alpha, alpha_vec, 0.0, table, rows, prev_row0, sum, lr, inv_hist,
                                  n_steps, sigma_modifier, fallback_sigma, xrec, sse_log, log_row0, n_log, sigma_out, stream, alpha_pp, lr_pp,
                                  sigma_modifier_pp);
}

extern "C" int pnp_csmri_saga_span(pnp_csmri_plan* p, void* z, const uint32_t* bitsT, const void* YT, double alpha, const double* alpha_pp,
                                   const void* alpha_vec, void* table, const int32_t* rows, const int32_t* prev_row0, void* sum, double lr,
                                   const double* lr_pp, double inv_hist, int hist, int denoise, double sigma_modifier,
                                   const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps, double* sse_log,
                                   int log_row0, int n_log, void* sigma_out, void* stream) {
    return saga_span_impl(p, z, bitsT, YT, alpha, alpha_pp, alpha_vec, table, rows, prev_row0, sum, lr, lr_pp, inv_hist, hist, denoise,
                          sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, n_steps, sse_log, log_row0, n_log, sigma_out, stream,
                          false, nullptr);
}

// ---- pnp_csmri_saga_span with the divisor per problem: inv_hist_pp double [batch], NULL = the scalar; hist = the table's row count
extern "C" int pnp_csmri_saga_span_hist(pnp_csmri_plan* p, void* z, const uint32_t* bitsT, const void* YT, double alpha,
                                        const double* alpha_pp, const void* alpha_vec, void* table, const int32_t* rows,
                                        const int32_t* prev_row0, void* sum, double lr, const double* lr_pp, double inv_hist,
                                        const double* inv_hist_pp, int hist, int denoise, double sigma_modifier,
                                        const double* sigma_modifier_pp, double fallback_sigma, const void* xrec, int n_steps,
                                        double* sse_log, int log_row0, int n_log, void* sigma_out, void* stream) {
    return saga_span_impl(p, z, bitsT, YT, alpha, alpha_pp, alpha_vec, table, rows, prev_row0, sum, lr, lr_pp, inv_hist, hist, denoise,
                          sigma_modifier, sigma_modifier_pp, fallback_sigma, xrec, n_steps, sse_log, log_row0, n_log, sigma_out, stream,
                          true, inv_hist_pp);
}

// pr_shared.hip -- phase-retrieval gradients of batch = G * items problems that SHARE `items` dense matrices (a trial-batched grid:
// problem b = t * items + i is trial t of item i and works on A[i], Y[i]).  With the matrix shared the two GEMVs of pr.hip become
// two skinny GEMMs on the matrix cores, and A is streamed twice per call and item whatever G is:
//     T = A [z_1 .. z_G, w_1 .. w_G]       k_prs_rows    (one stream of A; the 16-wide MFMA dimension is the problem columns)
//     U = sel o (wgt(T_z) - wgt(T_w))      k_prs_weight  (wgt(t) = ((|t| - y) / |t|) t; a row a problem did not select is written 0)
//     P = A^T U                            k_prs_cols    (the second stream of A)
//     out = alpha P + beta c1 + gamma c2   k_prs_finish
// v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64: lane l holds a = Aop[i = l & 15][k = l >> 4], b = Bop[k = l >> 4][j = l & 15].
// Every lane loads 16 bytes of A along the row (float4 / double2); element s of the vector feeds k-step s, i.e. the k index is
// permuted the same way for both operands (k_prs_rows), or output sub-tile s (k_prs_cols: a permutation of the n index undone at
// the store).  Columns are padded to multiples of 16 with zero weights.
// Deterministic: the split of N (rows pass) and of M (cols pass) over waves and blocks is a function of (M, N, dtype) alone, the
// partial sums are added in a fixed order, and an MFMA output element is an fma chain over its own row and column only -- so a
// problem's result does not depend on G, on its place in the batch or on what the other problems select.  No float atomics.
#include "common.h"
#include "draw.h"

namespace pnp {

template <typename T> struct Mf;
template <> struct Mf<float> {
    using V = float4;
    using Acc = float __attribute__((ext_vector_type(4)));
    static constexpr int VN = 4;
    static __device__ __forceinline__ Acc mfma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int drow(int lane, int r) { return (lane >> 4) * 4 + r; }      // D: col = lane & 15
    static __device__ __forceinline__ void unpack(const V& v, float* e) { e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
};
template <> struct Mf<double> {
    using V = double2;
    using Acc = double __attribute__((ext_vector_type(4)));
    static constexpr int VN = 2;
    static __device__ __forceinline__ Acc mfma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int drow(int lane, int r) { return (lane >> 4) + 4 * r; }      // (the f64 map differs)
    static __device__ __forceinline__ void unpack(const V& v, double* e) { e[0] = v.x; e[1] = v.y; }
};

// VN consecutive elements p[0 .. VN-1] of which the first `nvalid` exist (the rest read as 0); vec: p is 16-byte aligned and
// nvalid is 0 or VN.
template <typename T> __device__ __forceinline__ void load_vn(const T* p, int nvalid, bool vec, T* e) {
    using M = Mf<T>;
#pragma unroll
    for (int s = 0; s < M::VN; ++s) e[s] = (T)0;
    if (nvalid <= 0) return;
    if (vec) {
        M::unpack(*reinterpret_cast<const typename M::V*>(p), e);
    } else {
#pragma unroll
        for (int s = 0; s < M::VN; ++s) if (s < nvalid) e[s] = p[s];
    }
}

// The fixed partition: rows pass = NS blocks x 4 waves over N (nchunk columns per wave, a multiple of 4 VN), cols pass = MS blocks
// x 4 waves over M (mchunk rows per wave, a multiple of 4 VN).  About 2048 blocks per pass, at most 16 splits.
struct PrsSplit { int Mpad, NS, nchunk, MS, mchunk; };
static PrsSplit prs_split(int M, int N, int VN) {
    PrsSplit p;
    const int K = 4 * VN;
    p.Mpad = (M + 15) / 16 * 16;
    const int row_tiles = p.Mpad / 16, n_blocks = (N + 16 * VN - 1) / (16 * VN);
    auto clamp = [](int v, int hi) { return v < 1 ? 1 : (v > hi ? hi : v); };
    p.NS = clamp((2048 + row_tiles - 1) / row_tiles, clamp((N + 4 * K - 1) / (4 * K), 16));
    p.nchunk = ((N + p.NS * 4 - 1) / (p.NS * 4) + K - 1) / K * K;
    p.MS = clamp((2048 + n_blocks - 1) / n_blocks, clamp((M + 4 * K - 1) / (4 * K), 16));
    p.mchunk = ((M + p.MS * 4 - 1) / (p.MS * 4) + K - 1) / K * K;
    return p;
}

// T partials of columns c0 .. c0 + 16 CT - 1 (column c < G: W of problem c * items + item; G <= c < ncols: W2 of problem c - G;
// beyond: zero weights).  grid (Mpad / 16, NS), 256 threads: wave wv of block (x, y) sums n in [(4 y + wv) nchunk, +nchunk).
// Tp [NS][colsPad][Mpad].
template <typename T, int CT>
__global__ __launch_bounds__(256) void k_prs_rows(const T* __restrict__ A, const T* __restrict__ W, const T* __restrict__ W2,
                                                  int items, int item, int G, int c0, int ncols, int M, int N, int nchunk, int Mpad,
                                                  int colsPad, int vec, T* __restrict__ Tp) {
    using F = Mf<T>;
    constexpr int VN = F::VN;
    __shared__ T red[4][CT * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int m = blockIdx.x * 16 + li;
    const bool mok = m < M;
    const T* ap = A + (size_t)(mok ? m : 0) * N;
    const T* wp[CT];
    bool cok[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int c = c0 + ct * 16 + li;
        cok[ct] = c < ncols;
        const int t = cok[ct] ? (c < G ? c : c - G) : 0;
        wp[ct] = (c < G || !cok[ct] ? W : W2) + ((size_t)t * items + item) * N;
    }
    typename F::Acc acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = (typename F::Acc)(0);
    const int n0 = (blockIdx.y * 4 + wv) * nchunk;
    const int n1 = n0 + nchunk < N ? n0 + nchunk : N;
    for (int nb = n0; nb < n1; nb += 4 * VN) {
        const int n = nb + VN * lk, nv = n1 - n < VN ? n1 - n : VN;
        T av[VN], bv[CT][VN];
        load_vn<T>(ap + n, mok ? nv : 0, vec, av);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) load_vn<T>(wp[ct] + n, cok[ct] ? nv : 0, vec, bv[ct]);
#pragma unroll
        for (int s = 0; s < VN; ++s)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[ct] = F::mfma(av[s], bv[ct][s], acc[ct]);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wv][ct * 256 + r * 64 + lane] = acc[ct][r];
    __syncthreads();
    for (int e = threadIdx.x; e < CT * 256; e += 256) {
        const T sum = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        const int ct = e >> 8, r = (e >> 6) & 3, ln = e & 63;
        const int col = c0 + ct * 16 + (ln & 15), row = blockIdx.x * 16 + F::drow(ln, r);
        Tp[((size_t)blockIdx.y * colsPad + col) * Mpad + row] = sum;
    }
}

template <typename T> __device__ __forceinline__ T prs_wgt(T t, T ym) {      // k_pr_rows' epilogue
    const T mag = t < 0 ? -t : t;
    return ((mag - ym) / mag) * t;
}

// U [GPad][Mpad]: row m of column t = problem t * items + item; 0 where the problem did not select the row and in the padding.
template <typename T>
__global__ __launch_bounds__(256) void k_prs_weight(const T* __restrict__ Tp, int NS, int colsPad, int Mpad, int M, int G, int items,
                                                    int item, const T* __restrict__ Y, int has_w2, const MbDesc* __restrict__ mbd,
                                                    const uint8_t* __restrict__ ind, T* __restrict__ U) {
    const int m = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (m >= Mpad) return;
    T u = (T)0;
    if (t < G && m < M) {
        const size_t b = (size_t)t * items + item;
        const bool sel = mbd != nullptr ? mb_member(mbd[b], (uint32_t)m) : (ind != nullptr ? ind[b * M + m] != 0 : true);
        if (sel) {
            const T ym = Y[(size_t)item * M + m];
            T tz = (T)0;
            for (int ns = 0; ns < NS; ++ns) tz += Tp[((size_t)ns * colsPad + t) * Mpad + m];
            u = prs_wgt(tz, ym);
            if (has_w2) {
                T tw = (T)0;
                for (int ns = 0; ns < NS; ++ns) tw += Tp[((size_t)ns * colsPad + G + t) * Mpad + m];
                u -= prs_wgt(tw, ym);
            }
        }
    }
    U[(size_t)t * Mpad + m] = u;
}

// P partials of columns c0 .. c0 + 16 CT - 1 of U.  grid (ceil(N / (16 VN)), MS), 256 threads: wave wv of block (x, y) sums rows
// [(4 y + wv) mchunk, +mchunk) for the 16 VN matrix columns of block x.  P [MS][GPad][N].
template <typename T, int CT>
__global__ __launch_bounds__(256) void k_prs_cols(const T* __restrict__ A, const T* __restrict__ U, int c0, int M, int N, int mchunk,
                                                  int Mpad, int GPad, int vec, T* __restrict__ P) {
    using F = Mf<T>;
    constexpr int VN = F::VN;
    __shared__ T red[4][VN * CT * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int n = blockIdx.x * 16 * VN + VN * li;
    const int nv = N - n < VN ? N - n : VN;
    typename F::Acc acc[VN][CT];
#pragma unroll
    for (int e = 0; e < VN; ++e)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[e][ct] = (typename F::Acc)(0);
    const int m0 = (blockIdx.y * 4 + wv) * mchunk;
    const int m1 = m0 + mchunk < Mpad ? m0 + mchunk : Mpad;
    for (int mb = m0; mb < m1; mb += 4 * VN) {
        T uv[CT][VN];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
            F::unpack(*reinterpret_cast<const typename F::V*>(U + (size_t)(c0 + ct * 16 + li) * Mpad + mb + VN * lk), uv[ct]);
#pragma unroll
        for (int s = 0; s < VN; ++s) {
            const int row = mb + VN * lk + s;
            T av[VN];
            load_vn<T>(A + (size_t)(row < M ? row : 0) * N + (nv > 0 ? n : 0), row < M ? nv : 0, vec, av);
#pragma unroll
            for (int e = 0; e < VN; ++e)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[e][ct] = F::mfma(av[e], uv[ct][s], acc[e][ct]);
        }
    }
#pragma unroll
    for (int e = 0; e < VN; ++e)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wv][((e * CT + ct) * 4 + r) * 64 + lane] = acc[e][ct][r];
    __syncthreads();
    for (int x = threadIdx.x; x < VN * CT * 256; x += 256) {
        const T sum = ((red[0][x] + red[1][x]) + red[2][x]) + red[3][x];
        const int ln = x & 63, r = (x >> 6) & 3, q = x >> 8, ct = q % CT, e = q / CT;
        const int col = c0 + ct * 16 + (ln & 15), nn = blockIdx.x * 16 * VN + VN * F::drow(ln, r) + e;
        if (nn < N) P[((size_t)blockIdx.y * GPad + col) * N + nn] = sum;
    }
}

// out[b] = alpha_b * sum_ms P + beta * c1[b] + gamma_b * c2[b], b = t * items + item; the coefficients are rounded to T as the
// host rounds a scalar: (T)(alpha / alpha_div), (T)gamma.
template <typename T>
__global__ __launch_bounds__(256) void k_prs_finish(const T* __restrict__ P, int MS, int GPad, int N, int items, int item, double alpha,
                                                    const double* __restrict__ alpha_pp, double alpha_div, T beta, const T* c1,
                                                    double gamma, const double* __restrict__ gamma_pp, const T* c2, T* out) {
    const int n = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (n >= N) return;
    const size_t b = (size_t)t * items + item;
    T acc = (T)0;
    for (int ms = 0; ms < MS; ++ms) acc += P[((size_t)ms * GPad + t) * N + n];
    const T al = (T)((alpha_pp != nullptr ? alpha_pp[b] : alpha) / alpha_div);
    T r = al * acc;
    if (c1 != nullptr) r = fma_(beta, c1[b * N + n], r);
    if (c2 != nullptr) r = fma_((T)(gamma_pp != nullptr ? gamma_pp[b] : gamma), c2[b * N + n], r);
    out[b * N + n] = r;
}

template <typename T>
int run_prs(const T* A, const T* Y, const T* W, const T* W2, const MbDesc* mbd, const uint8_t* ind, int M, int N, int batch, int items,
            double alpha, const double* alpha_pp, double alpha_div, double beta, const T* c1, double gamma, const double* gamma_pp,
            const T* c2, T* ws, T* out, hipStream_t s) {
    constexpr int VN = Mf<T>::VN;
    const PrsSplit p = prs_split(M, N, VN);
    const int G = batch / items, ncols = W2 != nullptr ? 2 * G : G;
    const int colsPad = (ncols + 15) / 16 * 16, GPad = (G + 15) / 16 * 16;
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    const int vec = (N % VN == 0 && al16(A) && al16(W) && (W2 == nullptr || al16(W2))) ? 1 : 0;
    T* Tp = ws;                                              // [NS][colsPad][Mpad]
    T* U = Tp + (size_t)p.NS * colsPad * p.Mpad;             // [GPad][Mpad]
    T* P = U + (size_t)GPad * p.Mpad;                        // [MS][GPad][N]
    for (int item = 0; item < items; ++item) {               // (one workspace: the items follow one another on the stream)
        const T* Ai = A + (size_t)item * M * N;
        const dim3 rg(p.Mpad / 16, p.NS);
        for (int c0 = 0; c0 < colsPad; c0 += 64) {
            const int ct = (colsPad - c0) / 16;
#define PRS_ROWS(CT) k_prs_rows<T, CT><<<rg, 256, 0, s>>>(Ai, W, W2, items, item, G, c0, ncols, M, N, p.nchunk, p.Mpad, colsPad, vec, Tp)
            if (ct >= 4) PRS_ROWS(4); else if (ct == 3) PRS_ROWS(3); else if (ct == 2) PRS_ROWS(2); else PRS_ROWS(1);
#undef PRS_ROWS
            PNP_CHECK_LAUNCH();
        }
        k_prs_weight<T><<<dim3((p.Mpad + 255) / 256, GPad), 256, 0, s>>>(Tp, p.NS, colsPad, p.Mpad, M, G, items, item, Y, W2 != nullptr,
                                                                        mbd, ind, U);
        PNP_CHECK_LAUNCH();
        const dim3 cg((N + 16 * VN - 1) / (16 * VN), p.MS);
        for (int c0 = 0; c0 < GPad; c0 += 32) {
            if (GPad - c0 >= 32) k_prs_cols<T, 2><<<cg, 256, 0, s>>>(Ai, U, c0, M, N, p.mchunk, p.Mpad, GPad, vec, P);
            else k_prs_cols<T, 1><<<cg, 256, 0, s>>>(Ai, U, c0, M, N, p.mchunk, p.Mpad, GPad, vec, P);
            PNP_CHECK_LAUNCH();
        }
        k_prs_finish<T><<<dim3((N + 255) / 256, G), 256, 0, s>>>(P, p.MS, GPad, N, items, item, alpha, alpha_pp, alpha_div, (T)beta, c1,
                                                                gamma, gamma_pp, c2, out);
        PNP_CHECK_LAUNCH();
    }
    return PNP_OK;
}

}  // namespace pnp

using namespace pnp;

// Enough for either dtype and any `items` that divides `batch` (the items of a call run one after the other on one workspace).
extern "C" size_t pnp_pr_shared_workspace_elems(int M, int N, int batch) {
    if (M < 1 || N < 1 || batch < 1) return 0;
    const PrsSplit a = prs_split(M, N, 4), b = prs_split(M, N, 2);
    const size_t c2 = ((size_t)2 * batch + 15) / 16 * 16, cg = ((size_t)batch + 15) / 16 * 16;
    const size_t ns = a.NS > b.NS ? a.NS : b.NS, ms = a.MS > b.MS ? a.MS : b.MS;
    return ns * c2 * a.Mpad + cg * a.Mpad + ms * cg * N;
}

extern "C" int pnp_pr_grad_shared_pp(const void* A, const void* Y, const void* W, const void* W2, const void* mbd, const uint8_t* ind,
                                     int M, int N, int batch, int items, int dtype, double alpha, const double* alpha_pp,
                                     double alpha_div, double beta, const void* c1, double gamma, const double* gamma_pp,
                                     const void* c2, void* workspace, void* out, void* stream) {
    PNP_CHECK_ARG(A, "null A");
    PNP_CHECK_ARG(Y && W && workspace && out, "null argument");
    PNP_CHECK_ARG(M >= 1 && N >= 1 && batch >= 1 && items >= 1 && alpha_div != 0.0, "bad sizes");
    PNP_CHECK_ARG(batch % items == 0, "batch % items != 0");
    PNP_CHECK_ARG(!(mbd && ind), "both selections given (mbd and ind)");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    PNP_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PNP_F32)
        return run_prs<float>((const float*)A, (const float*)Y, (const float*)W, (const float*)W2, (const MbDesc*)mbd, ind, M, N, batch,
                              items, alpha, alpha_pp, alpha_div, beta, (const float*)c1, gamma, gamma_pp, (const float*)c2,
                              (float*)workspace, (float*)out, s);
    if (dtype == PNP_F64)
        return run_prs<double>((const double*)A, (const double*)Y, (const double*)W, (const double*)W2, (const MbDesc*)mbd, ind, M, N,
                               batch, items, alpha, alpha_pp, alpha_div, beta, (const double*)c1, gamma, gamma_pp, (const double*)c2,
                               (double*)workspace, (double*)out, s);
    PNP_CHECK_ARG(false, "bad dtype");
}

extern "C" int pnp_pr_grad_shared(const void* A, const void* Y, const void* W, const void* W2, const void* mbd, const uint8_t* ind,
                                  int M, int N, int batch, int items, int dtype, double alpha, double alpha_div, double beta,
                                  const void* c1, double gamma, const void* c2, void* workspace, void* out, void* stream) {
    return pnp_pr_grad_shared_pp(A, Y, W, W2, mbd, ind, M, N, batch, items, dtype, alpha, nullptr, alpha_div, beta, c1, gamma, nullptr,
                                 c2, workspace, out, stream);
}

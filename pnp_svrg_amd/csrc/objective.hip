// objective.hip -- the data-fidelity objective f(z) = ||Y - forward_model(z)||^2 / 2 / M per problem, on the device
// (reference problems/CSMRI.py:61-64, DeblurSR.py:114-117, PR.py:70-73): forward passes only, ending in a per-problem
// reduction instead of the adjoint / inverse transform and the image write of the gradients.
//
//   CSMRI  : k_rows_fwd (csmri_rows.h, the gradient's row pass) -> k_obj_cols: column FFT on the packed half spectrum,
//            sum of mask(k) |Z(k) - Y(k)|^2 over the FULL spectrum -- the workgroup that owns half-spectrum column kx also
//            accounts for column W - kx through Z(W - kx, (H - ky) mod H) = conj Z(kx, ky); the packed column (kx = 0 and W/2)
//            is unpacked first.  No inverse transform, no k-space write-back.
//   Deblur : pnp_deblur_forward into the plan's residual scratch, then k_obj_sq: sum (forward - Y)^2 over the M measurements.
//   PR     : k_obj_pr_rows: one wavefront per row of A, t = A w as k_pr_rows forms it, then (|t| - y)^2; A is streamed once.
//
// Every sum is taken in double whatever the storage type, in a fixed order and without atomics: lanes by xor-shuffles, the four
// wavefronts of a workgroup in order, the workgroups of a problem by k_obj_final (one workgroup per problem).  A problem's value
// therefore depends neither on the batch size nor on its index in the batch.  The partial sums of the workgroups live in scratch
// the plans already own (CSMRI: the head of each workgroup's own columns of the half-spectrum workspace, once they are consumed;
// Deblur: r1) or in the caller's workspace (PR): nothing is allocated and nothing synchronises.
//
// Compiled with the compiler's default FMA contraction, like csmri.hip, deblur.hip and pr.hip whose transforms and dot products
// these kernels share (the complex products of fft.h spell their FMAs out anyway); only the files that track NumPy / pywt
// product for product (prox*.hip, nlm.hip, axpbypcz_pp.hip) are built with -ffp-contract=off.
#include "csmri_rows.h"
#include "deblur_plan.h"

namespace pnp {

// sum over the 256 threads of a workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum_256(double acc, double* red) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// f_out[b] = scale * sum_i part[b * pstride + i * estride], i < n: one workgroup per problem
__global__ __launch_bounds__(256) void k_obj_final(const double* __restrict__ part, size_t pstride, size_t estride, int n,
                                                   double scale, double* __restrict__ f_out) {
    __shared__ double red[4];
    const double* p = part + (size_t)blockIdx.x * pstride;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += p[(size_t)i * estride];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) f_out[blockIdx.x] = scale * acc;
}

// ------------------------------------------------------------------------------- CSMRI columns
// The column pass of k_cols (csmri.hip) up to the spectrum, then the residual.  S1T: the packed transposed half spectrum of
// k_rows_fwd, [batch][W/2][H].  The workgroup's partial sum (a double) is written over the first bytes of its own first column,
// which all its threads have consumed by then (the transform's first barrier lies behind every load).
template <typename T, int RA, int LA>
__global__ __launch_bounds__(256) void k_obj_cols(cx<T>* S1T, const uint32_t* __restrict__ bitsT, const cx<T>* __restrict__ YT,
                                                  const cx<T>* __restrict__ twtab, int W) {
    using S = FftSmem<T, RA, LA>;
    constexpr int N = S::N, G = S::G, LG = S::LG;            // N = H
    constexpr int WPR = N / 32;                              // mask words per k-space column
    __shared__ cx<T> smem[S::SCR];
    __shared__ uint32_t sb[2][G][WPR];                       // mask bits of this block's columns c (slot 0) and W - c (slot 1)
    __shared__ double red[4];
    const int t = threadIdx.x, g = t / LG, lane = t % LG;
    const int prob = blockIdx.y, c = blockIdx.x * G + g;
    cx<T>* col = S1T + ((size_t)prob * (W / 2) + c) * N;
    cx<T>* scr = smem + g * LG * (LG + 1);
    const bool act = lane < RA;                              // lanes that hold spectrum values after the forward pass
    const int ln = act ? lane : 0;

    if (t < 2 * G * WPR) {
        const int slot = t / (G * WPR), gg = (t / WPR) % G, wd = t % WPR, cc = blockIdx.x * G + gg;
        const int kx = cc == 0 ? (slot == 0 ? 0 : W / 2) : (slot == 0 ? cc : W - cc);     // packed column 0 = kx 0 and W/2
        sb[slot][gg][wd] = bitsT[((size_t)prob * W + kx) * WPR + wd];
    }
    auto bit = [&](int slot, int ky) -> bool { return (sb[slot][g][ky >> 5] >> (ky & 31)) & 1u; };
    // |z - y|^2 with the difference and the squares in double (exact differences of the stored values)
    auto res2 = [](double zx, double zy, cx<T> y) -> double {
        const double dx = zx - (double)y.x, dy = zy - (double)y.y;
        return dx * dx + dy * dy;
    };

    cx<T> v[LG], tw[LG];
    load_twiddles_gen<T, LG>(tw, twtab, lane, N);
#pragma unroll
    for (int r = 0; r < RA; ++r) v[r] = col[(lane < LA ? lane : 0) + LA * r];

    // The data this thread's spectrum entries ky = ln + RA * r meet, loaded BEFORE the transform and whatever the mask says, so
    // that the loads are all in flight together and behind the transform's arithmetic (a load under `if (bit)` would be issued
    // and waited for one at a time); the mask then SELECTS what enters the sum, so values outside it never do.
    //   c != 0: ya = Y(c, ky), yb = Y(W - c, (H - ky) mod H);   the packed column c == 0: ya = Y(0, ky), yb = Y(W/2, ky)
    const cx<T>* Yp = YT + (size_t)prob * W * N;
    const cx<T>* pa = Yp + (size_t)c * N;
    const cx<T>* pb = Yp + (size_t)(c == 0 ? W / 2 : W - c) * N;
    cx<T> ya[LA], yb[LA];
#pragma unroll
    for (int r = 0; r < LA; ++r) {
        const int ky = ln + RA * r;
        ya[r] = pa[ky];
        yb[r] = pb[c == 0 ? ky : (N - ky) & (N - 1)];
    }
    fft_gen<T, RA, LA, false>(v, tw, scr, lane);             // (its barriers also publish sb)

    double acc = 0.0;
    if (blockIdx.x == 0) {
        // the packed column c == 0 holds two real-input transforms P = A + i B: A = Z(0, .), B = Z(W/2, .)
        __syncthreads();
        if (act) {
#pragma unroll
            for (int r = 0; r < LA; ++r) scr[lane + RA * r] = v[r];
        }
        __syncthreads();
        if (g == 0 && act) {
#pragma unroll
            for (int r = 0; r < LA; ++r) {
                const int ky = lane + RA * r, km = (N - ky) & (N - 1);
                const cx<T> pk = v[r], pm = scr[km];
                const cx<T> A = {(T)0.5 * (pk.x + pm.x), (T)0.5 * (pk.y - pm.y)};
                const cx<T> B = {(T)0.5 * (pk.y + pm.y), (T)-0.5 * (pk.x - pm.x)};
                const double dA = res2(A.x, A.y, ya[r]), dB = res2(B.x, B.y, yb[r]);
                acc += bit(0, ky) ? dA : 0.0;
                acc += bit(1, ky) ? dB : 0.0;
            }
        }
    }
    if (c != 0 && act) {
#pragma unroll
        for (int r = 0; r < LA; ++r) {
            const int ky = ln + RA * r, km = (N - ky) & (N - 1);
            const double d1 = res2(v[r].x, v[r].y, ya[r]);               // Z(c, ky)
            const double d2 = res2(v[r].x, -(double)v[r].y, yb[r]);      // Z(W - c, km) = conj Z(c, ky)
            acc += bit(0, ky) ? d1 : 0.0;
            acc += bit(1, km) ? d2 : 0.0;
        }
    }
    acc = block_sum_256(acc, red);
    if (t == 0) *reinterpret_cast<double*>(S1T + ((size_t)prob * (W / 2) + (size_t)blockIdx.x * G) * N) = acc;
}

template <typename T, int RA, int LA>
int run_csmri_objective(pnp_csmri_plan* p, const void* z, const void* YT, const uint32_t* bitsT, double scale, double* f_out,
                        hipStream_t s) {
    constexpr int G = FftSmem<T, RA, LA>::G;
    const int H = p->H, W = p->W, nblk = (W / 2) / G;
    cx<T>* work = (cx<T>*)p->work;
    const cx<T>* tw = (const cx<T>*)p->twtab;
    k_rows_fwd<T, RA, LA><<<dim3(H / (2 * G), p->batch), 256, 0, s>>>((const T*)z, nullptr, work, tw, H);
    PNP_CHECK_LAUNCH();
    k_obj_cols<T, RA, LA><<<dim3(nblk, p->batch), 256, 0, s>>>(work, bitsT, (const cx<T>*)YT, tw, W);
    PNP_CHECK_LAUNCH();
    constexpr size_t DPC = sizeof(cx<T>) / sizeof(double);   // doubles per complex element of the workspace
    k_obj_final<<<p->batch, 256, 0, s>>>((const double*)p->work, (size_t)(W / 2) * H * DPC, (size_t)G * H * DPC, nblk, scale, f_out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

// ------------------------------------------------------------------------------- sum of squared differences, chunked
constexpr int kSqChunk = 4096;                               // elements per workgroup of k_obj_sq

template <typename T>
__global__ __launch_bounds__(256) void k_obj_sq(const T* __restrict__ fwd, const T* __restrict__ Y, int M, int nblk,
                                                double* __restrict__ part) {
    __shared__ double red[4];
    const int prob = blockIdx.y, i0 = blockIdx.x * kSqChunk, i1 = i0 + kSqChunk < M ? i0 + kSqChunk : M;
    const T* f = fwd + (size_t)prob * M;
    const T* y = Y + (size_t)prob * M;
    double acc = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const double d = (double)f[i] - (double)y[i];
        acc += d * d;
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(size_t)prob * nblk + blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------- phase retrieval rows
template <typename T> struct ObjVec16;                       // 16-byte vector of T (pr.hip: Vec16)
template <> struct ObjVec16<float> { using type = float4; static constexpr int n = 4; };
template <> struct ObjVec16<double> { using type = double2; static constexpr int n = 2; };

// One wavefront per row m of problem blockIdx.y, which works on matrix blockIdx.y % n_mat: t = A[m] . w with 16-byte loads when
// N keeps every row 16-byte aligned (scalar loads otherwise), then (|t| - y[m])^2 in double.  Rows past M add nothing.  The
// workgroup's four rows are summed in order into part[prob][blockIdx.x].
template <typename T>
__global__ __launch_bounds__(256) void k_obj_pr_rows(const T* __restrict__ A, const T* __restrict__ w, const T* __restrict__ y,
                                                     int M, int N, int n_mat, int nblk, double* __restrict__ part) {
    using V = typename ObjVec16<T>::type;
    constexpr int VN = ObjVec16<T>::n;
    __shared__ double red[4];
    const int prob = blockIdx.y, mat = prob % n_mat;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double d2 = 0.0;
    if (m < M) {                                             // (wavefront-uniform)
        const T* a = A + ((size_t)mat * M + m) * N;
        const T* wp = w + (size_t)prob * N;
        T acc = 0;
        if (N % VN == 0) {
            const V* a4 = reinterpret_cast<const V*>(a);
            const V* w4 = reinterpret_cast<const V*>(wp);
            for (int n = lane; n < N / VN; n += 64) {
                const V av = a4[n], wq = w4[n];
                if constexpr (VN == 4) acc += (av.x * wq.x + av.y * wq.y) + (av.z * wq.z + av.w * wq.w);
                else acc += av.x * wq.x + av.y * wq.y;
            }
        } else {
            for (int n = lane; n < N; n += 64) acc += a[n] * wp[n];
        }
        acc = wave_sum(acc);
        const double d = (double)(acc < 0 ? -acc : acc) - (double)y[(size_t)prob * M + m];
        d2 = d * d;
    }
    if (lane == 0) red[threadIdx.x >> 6] = d2;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)prob * nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
int run_pr_objective(const void* A, const void* w, const void* y, int M, int N, int batch, int n_mat, double scale, double* part,
                     double* f_out, hipStream_t s) {
    const int nblk = (M + 3) / 4;
    k_obj_pr_rows<T><<<dim3(nblk, batch), 256, 0, s>>>((const T*)A, (const T*)w, (const T*)y, M, N, n_mat, nblk, part);
    PNP_CHECK_LAUNCH();
    k_obj_final<<<batch, 256, 0, s>>>(part, (size_t)nblk, 1, nblk, scale, f_out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_csmri_objective(pnp_csmri_plan* p, const void* z, const void* YT, const uint32_t* bitsT, double scale,
                                   double* f_out, void* stream) {
    PNP_CHECK_ARG(p && z && YT && bitsT && f_out, "null argument");
    PNP_CHECK_ARG(p->batch >= 1 && (p->dtype == PNP_F32 || p->dtype == PNP_F64), "bad plan (batch / dtype)");
    hipStream_t s = (hipStream_t)stream;
#define PNP_OBJ_ARGS p, z, YT, bitsT, scale, f_out, s
    if (p->dtype == PNP_F32) {
        if (p->NL == 16) return run_csmri_objective<float, 16, 16>(PNP_OBJ_ARGS);
        if (p->NL == 12) return run_csmri_objective<float, 8, 16>(PNP_OBJ_ARGS);
        return run_csmri_objective<float, 8, 8>(PNP_OBJ_ARGS);
    }
    if (p->NL == 16) return run_csmri_objective<double, 16, 16>(PNP_OBJ_ARGS);
    if (p->NL == 12) return run_csmri_objective<double, 8, 16>(PNP_OBJ_ARGS);
    return run_csmri_objective<double, 8, 8>(PNP_OBJ_ARGS);
#undef PNP_OBJ_ARGS
}

extern "C" int pnp_deblur_objective(pnp_deblur_plan* p, const void* z, const void* Y, double scale, double* f_out, void* stream) {
    PNP_CHECK_ARG(p && z && Y && f_out, "null argument");
    PNP_CHECK_ARG(p->batch >= 1 && (p->dtype == PNP_F32 || p->dtype == PNP_F64), "bad plan (batch / dtype)");
    hipStream_t s = (hipStream_t)stream;
    // S B z into r0 (with a down-sampler the blurred image passes through r1, which is free again behind the forward call)
    int rc = pnp_deblur_forward(p, z, p->r0, stream);
    if (rc) return rc;
    const int nblk = (p->M + kSqChunk - 1) / kSqChunk;       // <= 16 doubles per problem: r1 holds N >= 4096 elements per problem
    double* part = (double*)p->r1;
    if (p->dtype == PNP_F32)
        k_obj_sq<float><<<dim3(nblk, p->batch), 256, 0, s>>>((const float*)p->r0, (const float*)Y, p->M, nblk, part);
    else
        k_obj_sq<double><<<dim3(nblk, p->batch), 256, 0, s>>>((const double*)p->r0, (const double*)Y, p->M, nblk, part);
    PNP_CHECK_LAUNCH();
    k_obj_final<<<p->batch, 256, 0, s>>>(part, (size_t)nblk, 1, nblk, scale, f_out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" size_t pnp_pr_objective_workspace_bytes(int M, int batch) {
    return M < 1 || batch < 1 ? 0 : (size_t)batch * (size_t)((M + 3) / 4) * sizeof(double);
}

extern "C" int pnp_pr_objective(const void* A, const void* w, const void* y, int M, int N, int batch, int n_mat, int dtype,
                                double scale, void* workspace, double* f_out, void* stream) {
    PNP_CHECK_ARG(A && w && y && workspace && f_out, "null argument");
    PNP_CHECK_ARG(batch >= 1 && M >= 1 && N >= 1, "bad sizes (batch, M, N must be >= 1)");
    PNP_CHECK_ARG(n_mat >= 1 && n_mat <= batch && batch % n_mat == 0, "n_mat must be batch or a divisor of it");
    PNP_CHECK_ARG(batch <= 65535, "batch must be <= 65535 (grid y)");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "dtype must be PNP_F32 or PNP_F64");
    PNP_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PNP_F32) return run_pr_objective<float>(A, w, y, M, N, batch, n_mat, scale, (double*)workspace, f_out, s);
    return run_pr_objective<double>(A, w, y, M, N, batch, n_mat, scale, (double*)workspace, f_out, s);
}

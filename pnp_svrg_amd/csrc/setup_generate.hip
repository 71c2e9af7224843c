// setup_generate.hip -- Deblur and phase-retrieval sweep batches generated on the device from the counter-based stream
// published in include/pnp_hip.h (problems/DeblurSR.py:38-57, problems/PR.py:26-63, problems/problem.py:58-61 per item), and
// the batched spectral initialisation of PR with its stopping rule evaluated per item on the device.
//
//   k_sg_gather      xrec[b] = images[image_idx[b]]
//   k_sg_sigma       sigma = sqrt(||Y0||_2 * snr_fac / H / W): one workgroup per item, sum of squares in double, fixed tree
//   k_sg_noise       Y = Y0 + sigma * n(m), Box-Muller in double from key_1, key_2
//   k_sg_uniform     Deblur Xinit(i) = key_5(i) * 2^-32
//   k_pr_gen_A       A[m][n] from key_3, key_4: one Box-Muller pair = two adjacent elements, 16-byte stores
//   k_pr_gen_rows    Y0[m] = |A[m] . x|, one wavefront per row, products and sums in double
//   k_si_init / k_si_rows / k_si_cols / k_si_reduce / k_si_epilogue / k_si_any / k_si_final
//                    the power iteration v <- A^T (Y o (A v)) / M of PR.py:50-63 for all items at once: A and Y in the plan
//                    dtype, everything else in double; an item whose stopping rule has fired is frozen (every kernel returns at
//                    once for it), so its result does not depend on what else is in the batch.
//
// Every reduction is per item, in a fixed order, without atomics, and there is one dispatch form for every batch size.
#include "common.h"
#include "draw.h"
#include "reduce.h"
#include "deblur_plan.h"

namespace pnp {

namespace {

constexpr int SI_CHUNKS = 64;                 // row chunks of the column pass (the partial sums are reduced in chunk order)
constexpr double SI_TOL = 1e-5;               // PR.py:56

__device__ __forceinline__ uint64_t sg_state(uint64_t seed, uint64_t id, uint64_t k) {
    return mix64(mix64(mix64(seed) + id) + k);
}

__device__ __forceinline__ double sg_u1(uint32_t key) { return ((double)key + 1.0) * 0x1p-32; }      // (0, 1]
__device__ __forceinline__ double sg_u2(uint32_t key) { return (double)key * 0x1p-32; }              // [0, 1)

template <typename T> struct V16;                                  // 16 bytes of T
template <> struct V16<float> { using type = float4; static constexpr int n = 4; };
template <> struct V16<double> { using type = double2; static constexpr int n = 2; };

// fixed-order sum of one double per thread over a 256-thread workgroup; the result is valid in every thread
__device__ __forceinline__ double block_sum256(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double block_max256(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] = nan_max(sh[t + s], sh[t]);
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double block_min256(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] = nan_min(sh[t + s], sh[t]);
        __syncthreads();
    }
    return sh[0];
}

// ------------------------------------------------------------------------------- shared by Deblur and PR
template <typename T>
__global__ __launch_bounds__(256) void k_sg_gather(const T* __restrict__ images, int n_images, const int32_t* __restrict__ image_idx,
                                                   T* __restrict__ xrec, int n) {
    const int prob = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int im = image_idx[prob];
    im = im < 0 ? 0 : (im >= n_images ? n_images - 1 : im);            // (the host checks the range; never read outside the set)
    xrec[(size_t)prob * n + j] = images[(size_t)im * n + j];
}

template <typename T>
__global__ __launch_bounds__(256) void k_sg_sigma(const T* __restrict__ Y0, int M, const double* __restrict__ snr_fac, double H,
                                                  double W, double* __restrict__ sigma) {
    __shared__ double sh[256];
    const int prob = blockIdx.x;
    const T* y = Y0 + (size_t)prob * M;
    double acc = 0.0;
    for (int m = threadIdx.x; m < M; m += 256) {
        const double v = (double)y[m];
        acc = fma_(v, v, acc);
    }
    const double ss = block_sum256(acc, sh);
    if (threadIdx.x == 0) sigma[prob] = sqrt(sqrt(ss) * snr_fac[prob] / H / W);      // the norm, not its square
}

template <typename T>
__global__ __launch_bounds__(256) void k_sg_noise(T* __restrict__ Y, int M, const uint64_t* __restrict__ seed,
                                                  const uint64_t* __restrict__ id, const double* __restrict__ sigma) {
    const int prob = blockIdx.y;
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const uint64_t sd = seed[prob], it = id[prob];
    const double u1 = sg_u1(mb_key(sg_state(sd, it, 1), (uint32_t)m));
    const double u2 = sg_u2(mb_key(sg_state(sd, it, 2), (uint32_t)m));
    const double nrm = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    T* y = Y + (size_t)prob * M + m;
    *y = (T)fma_(sigma[prob], nrm, (double)*y);
}

// The two kernels above for a mixed-scale Deblur plan: item b has M_vec[b] measurements in a row of Mmax.  The same statements over
// m < M_b, so an item's sigma and Y[:M_b] are those of a uniform plan of its scale; the padding is neither read nor written.
template <typename T>
__global__ __launch_bounds__(256) void k_sg_sigma_m(const T* __restrict__ Y0, const int32_t* __restrict__ M_vec, int Mmax,
                                                    const double* __restrict__ snr_fac, double H, double W,
                                                    double* __restrict__ sigma) {
    __shared__ double sh[256];
    const int prob = blockIdx.x, M = M_vec[prob];
    const T* y = Y0 + (size_t)prob * Mmax;
    double acc = 0.0;
    for (int m = threadIdx.x; m < M; m += 256) {
        const double v = (double)y[m];
        acc = fma_(v, v, acc);
    }
    const double ss = block_sum256(acc, sh);
    if (threadIdx.x == 0) sigma[prob] = sqrt(sqrt(ss) * snr_fac[prob] / H / W);
}

template <typename T>
__global__ __launch_bounds__(256) void k_sg_noise_m(T* __restrict__ Y, const int32_t* __restrict__ M_vec, int Mmax,
                                                    const uint64_t* __restrict__ seed, const uint64_t* __restrict__ id,
                                                    const double* __restrict__ sigma) {
    const int prob = blockIdx.y;
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M_vec[prob]) return;
    const uint64_t sd = seed[prob], it = id[prob];
    const double u1 = sg_u1(mb_key(sg_state(sd, it, 1), (uint32_t)m));
    const double u2 = sg_u2(mb_key(sg_state(sd, it, 2), (uint32_t)m));
    const double nrm = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    T* y = Y + (size_t)prob * Mmax + m;
    *y = (T)fma_(sigma[prob], nrm, (double)*y);
}

template <typename T>
__global__ __launch_bounds__(256) void k_sg_uniform(T* __restrict__ xinit, int n, const uint64_t* __restrict__ seed,
                                                    const uint64_t* __restrict__ id) {
    const int prob = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    xinit[(size_t)prob * n + i] = (T)sg_u2(mb_key(sg_state(seed[prob], id[prob], 5), (uint32_t)i));
}

// ------------------------------------------------------------------------------- PR: the matrix
// Element e = m*N + n of an item comes from pair j = e >> 1: r = sqrt(-2 ln u1(key_3(j))), cos for even e, sin for odd e.
// One thread makes 16 bytes (two pairs in f32, one in f64) and stores them at once when the item's element count keeps every
// item 16-byte aligned; otherwise element by element.
template <typename T>
__global__ __launch_bounds__(256) void k_pr_gen_A(T* __restrict__ A, uint64_t MN, const uint64_t* __restrict__ seed,
                                                  const uint64_t* __restrict__ id) {
    using V = typename V16<T>::type;
    constexpr int VN = V16<T>::n;
    const int prob = blockIdx.y;
    const uint64_t e0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * VN;
    if (e0 >= MN) return;
    const uint64_t sd = seed[prob], it = id[prob];
    const uint64_t s3 = sg_state(sd, it, 3), s4 = sg_state(sd, it, 4);
    T out[VN];
#pragma unroll
    for (int q = 0; q < VN / 2; ++q) {
        const uint32_t j = (uint32_t)((e0 >> 1) + q);
        const double r = sqrt(-2.0 * log(sg_u1(mb_key(s3, j))));
        double sn, cs;
        sincospi(2.0 * sg_u2(mb_key(s4, j)), &sn, &cs);
        out[2 * q] = (T)(r * cs);
        out[2 * q + 1] = (T)(r * sn);
    }
    T* dst = A + (size_t)prob * MN + e0;
    if (MN % VN == 0) {
        V v;
        if constexpr (VN == 4) v = V{out[0], out[1], out[2], out[3]};
        else v = V{out[0], out[1]};
        *reinterpret_cast<V*>(dst) = v;
    } else {
#pragma unroll
        for (int q = 0; q < VN; ++q)
            if (e0 + q < MN) dst[q] = out[q];
    }
}

// dot product of row `a` (plan dtype) with `x` (XT: plan dtype or double) over a wavefront, products and sums in double
template <typename T, typename XT>
__device__ __forceinline__ double row_dot(const T* __restrict__ a, const XT* __restrict__ x, int N, int lane) {
    using V = typename V16<T>::type;
    constexpr int VN = V16<T>::n;
    double acc = 0.0;
    if (N % VN == 0) {
        const V* a4 = reinterpret_cast<const V*>(a);
        for (int n = lane; n < N / VN; n += 64) {
            const V av = a4[n];
            const XT* xp = x + (size_t)n * VN;
            acc = fma_((double)av.x, (double)xp[0], acc);
            acc = fma_((double)av.y, (double)xp[1], acc);
            if constexpr (VN == 4) {
                acc = fma_((double)av.z, (double)xp[2], acc);
                acc = fma_((double)av.w, (double)xp[3], acc);
            }
        }
    } else {
        for (int n = lane; n < N; n += 64) acc = fma_((double)a[n], (double)x[n], acc);
    }
    return wave_sum(acc);
}

template <typename T>
__global__ __launch_bounds__(256) void k_pr_gen_rows(const T* __restrict__ A, const T* __restrict__ x, int M, int N,
                                                     T* __restrict__ Y0) {
    const int prob = blockIdx.y;
    const int m = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (m >= M) return;
    const double d = row_dot<T, T>(A + ((size_t)prob * M + m) * N, x + (size_t)prob * N, N, lane);
    if (lane == 0) Y0[(size_t)prob * M + m] = (T)fabs(d);
}

// ------------------------------------------------------------------------------- PR: batched spectral initialisation
// Workspace (doubles): v [B][N], vraw [B][N], u [B][M], part [B][SI_CHUNKS][N], lead [B], then one int32 "any active".
struct SiWs {
    double *v, *vraw, *u, *part, *lead;
    int32_t* any;
};

__host__ inline SiWs si_carve(void* ws, int M, int N, int B) {
    SiWs w;
    w.v = (double*)ws;
    w.vraw = w.v + (size_t)B * N;
    w.u = w.vraw + (size_t)B * N;
    w.part = w.u + (size_t)B * M;
    w.lead = w.part + (size_t)B * SI_CHUNKS * N;
    w.any = (int32_t*)(w.lead + B);
    return w;
}

// PR.py:54-55: m, mold = 1, 2; y_final = 2 * ones, y_old = ones -- the rule holds before the first step (|1 - 2| > tol and
// ||2 - 1|| = sqrt(N) > tol), so every item starts active
__global__ __launch_bounds__(256) void k_si_init(double* __restrict__ v, double* __restrict__ lead, int32_t* __restrict__ active,
                                                 int32_t* __restrict__ iters, int N) {
    const int prob = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < N) v[(size_t)prob * N + n] = 2.0;
    if (n == 0) { lead[prob] = 1.0; active[prob] = 1; iters[prob] = 0; }
}

template <typename T>
__global__ __launch_bounds__(256) void k_si_rows(const T* __restrict__ A, const T* __restrict__ Y, const double* __restrict__ v,
                                                 const int32_t* __restrict__ active, int M, int N, double* __restrict__ u) {
    const int prob = blockIdx.y;
    if (!active[prob]) return;
    const int m = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (m >= M) return;
    const double d = row_dot<T, double>(A + ((size_t)prob * M + m) * N, v + (size_t)prob * N, N, lane);
    if (lane == 0) u[(size_t)prob * M + m] = (double)Y[(size_t)prob * M + m] * d;
}

// part[c][n] = sum over the rows m of chunk c of A[m][n] * u[m]; a thread owns VN adjacent columns (VN = 1: any N)
template <typename T, int VN>
__global__ __launch_bounds__(256) void k_si_cols(const T* __restrict__ A, const double* __restrict__ u,
                                                 const int32_t* __restrict__ active, int M, int N, int rows_per_chunk,
                                                 double* __restrict__ part) {
    const int prob = blockIdx.z;
    if (!active[prob]) return;
    const int n0 = (blockIdx.x * 256 + threadIdx.x) * VN;
    if (n0 >= N) return;
    const int m0 = blockIdx.y * rows_per_chunk, m1 = m0 + rows_per_chunk < M ? m0 + rows_per_chunk : M;
    const T* Ap = A + (size_t)prob * M * N + n0;
    const double* up = u + (size_t)prob * M;
    double acc[VN];
#pragma unroll
    for (int q = 0; q < VN; ++q) acc[q] = 0.0;
    for (int m = m0; m < m1; ++m) {
        const double um = up[m];
        if constexpr (VN == 1) {
            acc[0] = fma_((double)Ap[(size_t)m * N], um, acc[0]);
        } else {
            using V = typename V16<T>::type;
            const V av = *reinterpret_cast<const V*>(Ap + (size_t)m * N);
            acc[0] = fma_((double)av.x, um, acc[0]);
            acc[1] = fma_((double)av.y, um, acc[1]);
            if constexpr (VN == 4) {
                acc[2] = fma_((double)av.z, um, acc[2]);
                acc[3] = fma_((double)av.w, um, acc[3]);
            }
        }
    }
    double* dst = part + ((size_t)prob * SI_CHUNKS + blockIdx.y) * N + n0;
#pragma unroll
    for (int q = 0; q < VN; ++q) dst[q] = acc[q];
}

__global__ __launch_bounds__(256) void k_si_reduce(const double* __restrict__ part, const int32_t* __restrict__ active, int M, int N,
                                                   double* __restrict__ vraw) {
    const int prob = blockIdx.y;
    if (!active[prob]) return;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double acc = 0.0;
    for (int c = 0; c < SI_CHUNKS; ++c) acc += part[((size_t)prob * SI_CHUNKS + c) * N + n];
    vraw[(size_t)prob * N + n] = acc / (double)M;
}

// PR.py:58-62 and the rule of :57 for the NEXT step: lead = max(vraw); v_new = vraw / lead; the item stays active iff
// |lead - lead_old| > tol and ||v_new - v|| > tol.  One workgroup per item.
__global__ __launch_bounds__(256) void k_si_epilogue(const double* __restrict__ vraw, double* __restrict__ v, double* __restrict__ lead,
                                                     int32_t* __restrict__ active, int32_t* __restrict__ iters, int N) {
    __shared__ double sh[256];
    const int prob = blockIdx.x;
    if (!active[prob]) return;
    const double* r = vraw + (size_t)prob * N;
    double* vp = v + (size_t)prob * N;
    double mx = r[0];
    for (int n = threadIdx.x; n < N; n += 256) mx = nan_max(r[n], mx);
    mx = block_max256(mx, sh);
    double acc = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const double nv = r[n] / mx, d = nv - vp[n];
        acc = fma_(d, d, acc);
        vp[n] = nv;
    }
    const double change = sqrt(block_sum256(acc, sh));
    if (threadIdx.x == 0) {
        const double old = lead[prob];
        lead[prob] = mx;
        iters[prob] += 1;
        active[prob] = (fabs(mx - old) > SI_TOL && change > SI_TOL) ? 1 : 0;
    }
}

__global__ void k_si_any(const int32_t* __restrict__ active, int B, int32_t* __restrict__ any) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int a = 0;
        for (int b = 0; b < B; ++b) a |= active[b];
        *any = a;
    }
}

// PR.py:63 and :38: x0 = sqrt(lead) * v / ||v|| * ||x||, Xinit = (x0 - min x0) / (max x0 - min x0); norms in double
template <typename T>
__global__ __launch_bounds__(256) void k_si_final(const double* __restrict__ v, const double* __restrict__ lead,
                                                  const T* __restrict__ xrec, int N, T* __restrict__ xinit) {
    __shared__ double sh[256];
    const int prob = blockIdx.x;
    const double* vp = v + (size_t)prob * N;
    const T* x = xrec + (size_t)prob * N;
    double av = 0.0, ax = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        av = fma_(vp[n], vp[n], av);
        ax = fma_((double)x[n], (double)x[n], ax);
    }
    const double nv = sqrt(block_sum256(av, sh)), nx = sqrt(block_sum256(ax, sh));
    const double sl = sqrt(lead[prob]);
    auto x0 = [&](int n) { return sl * vp[n] / nv * nx; };
    double lo = x0(0), hi = lo;
    for (int n = threadIdx.x; n < N; n += 256) {
        const double q = x0(n);
        lo = nan_min(q, lo);
        hi = nan_max(q, hi);
    }
    lo = block_min256(lo, sh);
    hi = block_max256(hi, sh);
    const double span = hi - lo;
    for (int n = threadIdx.x; n < N; n += 256) xinit[(size_t)prob * N + n] = (T)((x0(n) - lo) / span);
}

// ------------------------------------------------------------------------------- launch sequences
template <typename T>
int run_noise_tail(T* Y, int M, int B, const double* snr_fac, const uint64_t* seed, const uint64_t* id, double H, double W,
                   double* sigma, hipStream_t s) {
    k_sg_sigma<T><<<B, 256, 0, s>>>(Y, M, snr_fac, H, W, sigma);
    PNP_CHECK_LAUNCH();
    k_sg_noise<T><<<dim3((M + 255) / 256, B), 256, 0, s>>>(Y, M, seed, id, sigma);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

template <typename T>
int run_deblur_generate(pnp_deblur_plan* p, const void* images, int n_images, const int32_t* image_idx, const double* snr_fac,
                        const uint64_t* seed, const uint64_t* id, void* xrec, void* Y, void* xinit, double* sigma, hipStream_t s) {
    const int N = p->N, B = p->batch, M = p->M;
    k_sg_gather<T><<<dim3((N + 255) / 256, B), 256, 0, s>>>((const T*)images, n_images, image_idx, (T*)xrec, N);
    PNP_CHECK_LAUNCH();
    if (p->n_sets > 0) {
        // a mixed-scale plan: Y [batch][Mmax], Y0_b = S_b B x_b with zeros in the padding; sigma and noise over m < M_b
        int rc = pnp_deblur_forward_mixed(p, xrec, Y, s);
        if (rc) return rc;
        k_sg_sigma_m<T><<<B, 256, 0, s>>>((const T*)Y, p->mx_M, M, snr_fac, (double)p->n, (double)(N / p->n), sigma);
        PNP_CHECK_LAUNCH();
        k_sg_noise_m<T><<<dim3((M + 255) / 256, B), 256, 0, s>>>((T*)Y, p->mx_M, M, seed, id, sigma);
        PNP_CHECK_LAUNCH();
        k_sg_uniform<T><<<dim3((N + 255) / 256, B), 256, 0, s>>>((T*)xinit, N, seed, id);
        PNP_CHECK_LAUNCH();
        return PNP_OK;
    }
    int rc = pnp_deblur_forward(p, xrec, Y, s);                            // Y0 = S B x through the plan's own forward pass
    if (rc) return rc;
    // H * W = N with H and W powers of two: the two divisions of the sigma formula are exact, so (n, N / n) stands for (H, W)
    rc = run_noise_tail<T>((T*)Y, M, B, snr_fac, seed, id, (double)p->n, (double)(N / p->n), sigma, s);
    if (rc) return rc;
    k_sg_uniform<T><<<dim3((N + 255) / 256, B), 256, 0, s>>>((T*)xinit, N, seed, id);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

template <typename T>
int run_pr_generate(const void* images, int n_images, const int32_t* image_idx, const double* snr_fac, const uint64_t* seed,
                    const uint64_t* id, int H, int W, int M, int B, void* A, void* xrec, void* Y, double* sigma, hipStream_t s) {
    constexpr int VN = V16<T>::n;
    const int N = H * W;
    const uint64_t MN = (uint64_t)M * (uint64_t)N;
    const uint64_t nthreads = (MN + VN - 1) / VN;
    k_pr_gen_A<T><<<dim3((unsigned)((nthreads + 255) / 256), B), 256, 0, s>>>((T*)A, MN, seed, id);
    PNP_CHECK_LAUNCH();
    k_sg_gather<T><<<dim3((N + 255) / 256, B), 256, 0, s>>>((const T*)images, n_images, image_idx, (T*)xrec, N);
    PNP_CHECK_LAUNCH();
    k_pr_gen_rows<T><<<dim3((M + 3) / 4, B), 256, 0, s>>>((const T*)A, (const T*)xrec, M, N, (T*)Y);
    PNP_CHECK_LAUNCH();
    return run_noise_tail<T>((T*)Y, M, B, snr_fac, seed, id, (double)H, (double)W, sigma, s);
}

template <typename T>
int run_spectral_init(const void* A_, const void* Y_, const void* xrec, int M, int N, int B, int max_iters, int check_every,
                      void* ws, void* xinit, int32_t* iters, int32_t* active, hipStream_t s) {
    constexpr int VN = V16<T>::n;
    const T* A = (const T*)A_;
    const T* Y = (const T*)Y_;
    const SiWs w = si_carve(ws, M, N, B);
    const int rpc = (M + SI_CHUNKS - 1) / SI_CHUNKS;
    k_si_init<<<dim3((N + 255) / 256, B), 256, 0, s>>>(w.v, w.lead, active, iters, N);
    PNP_CHECK_LAUNCH();
    for (int done = 0; done < max_iters;) {
        const int chunk = check_every < max_iters - done ? check_every : max_iters - done;
        for (int k = 0; k < chunk; ++k) {
            k_si_rows<T><<<dim3((M + 3) / 4, B), 256, 0, s>>>(A, Y, w.v, active, M, N, w.u);
            PNP_CHECK_LAUNCH();
            if (N % VN == 0)
                k_si_cols<T, VN><<<dim3((N / VN + 255) / 256, SI_CHUNKS, B), 256, 0, s>>>(A, w.u, active, M, N, rpc, w.part);
            else
                k_si_cols<T, 1><<<dim3((N + 255) / 256, SI_CHUNKS, B), 256, 0, s>>>(A, w.u, active, M, N, rpc, w.part);
            PNP_CHECK_LAUNCH();
            k_si_reduce<<<dim3((N + 255) / 256, B), 256, 0, s>>>(w.part, active, M, N, w.vraw);
            PNP_CHECK_LAUNCH();
            k_si_epilogue<<<B, 256, 0, s>>>(w.vraw, w.v, w.lead, active, iters, N);
            PNP_CHECK_LAUNCH();
        }
        done += chunk;
        k_si_any<<<1, 64, 0, s>>>(active, B, w.any);
        PNP_CHECK_LAUNCH();
        int32_t any = 0;                                                   // the one read-back of the chunk
        PNP_CHECK_HIP(hipMemcpyAsync(&any, w.any, sizeof(any), hipMemcpyDeviceToHost, s));
        PNP_CHECK_HIP(hipStreamSynchronize(s));
        if (!any) break;
    }
    k_si_final<T><<<B, 256, 0, s>>>(w.v, w.lead, (const T*)xrec, N, (T*)xinit);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

}  // namespace
}  // namespace pnp

using namespace pnp;

extern "C" int pnp_deblur_generate(pnp_deblur_plan* p, const void* images, int n_images, const int32_t* image_idx,
                                   const double* snr_fac, const uint64_t* seed, const uint64_t* id, void* xrec, void* Y,
                                   void* xinit, double* sigma, void* stream) {
    PNP_CHECK_ARG(p != nullptr, "null plan");
    PNP_CHECK_ARG(images && image_idx && snr_fac && seed && id, "null input");
    PNP_CHECK_ARG(xrec && Y && xinit && sigma, "null output");
    PNP_CHECK_ARG(n_images >= 1, "n_images must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    if (p->dtype == PNP_F32) return run_deblur_generate<float>(p, images, n_images, image_idx, snr_fac, seed, id, xrec, Y, xinit, sigma, s);
    return run_deblur_generate<double>(p, images, n_images, image_idx, snr_fac, seed, id, xrec, Y, xinit, sigma, s);
}

extern "C" int pnp_pr_generate(const void* images, int n_images, const int32_t* image_idx, const double* snr_fac,
                               const uint64_t* seed, const uint64_t* id, int H, int W, int M, int batch, int dtype, void* A,
                               void* xrec, void* Y, double* sigma, void* stream) {
    PNP_CHECK_ARG(A != nullptr, "null A");
    PNP_CHECK_ARG(images && image_idx && snr_fac && seed && id, "null input");
    PNP_CHECK_ARG(xrec && Y && sigma, "null output");
    PNP_CHECK_ARG(n_images >= 1 && H >= 1 && W >= 1 && M >= 1 && batch >= 1 && batch <= 65535, "bad sizes");
    PNP_CHECK_ARG((uint64_t)H * (uint64_t)W <= (1ull << 31) - 1, "H * W too large");
    PNP_CHECK_ARG((uint64_t)M * (uint64_t)H * (uint64_t)W <= (1ull << 32), "M * N must be <= 2^32 (32-bit pair index of the matrix stream)");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PNP_F32) return run_pr_generate<float>(images, n_images, image_idx, snr_fac, seed, id, H, W, M, batch, A, xrec, Y, sigma, s);
    if (dtype == PNP_F64) return run_pr_generate<double>(images, n_images, image_idx, snr_fac, seed, id, H, W, M, batch, A, xrec, Y, sigma, s);
    PNP_CHECK_ARG(false, "bad dtype");
}

extern "C" size_t pnp_pr_spectral_workspace_bytes(int M, int N, int batch) {
    if (M < 1 || N < 1 || batch < 1) return 0;
    const size_t B = (size_t)batch;
    return (B * ((size_t)2 * N + (size_t)M + (size_t)SI_CHUNKS * N + 1) + 1) * sizeof(double);
}

extern "C" int pnp_pr_spectral_init_batch(const void* A, const void* Y, const void* xrec, int M, int N, int batch, int dtype,
                                          int max_iters, int check_every, void* workspace, void* xinit, int32_t* iters_out,
                                          int32_t* active_out, void* stream) {
    PNP_CHECK_ARG(A != nullptr, "null A");
    PNP_CHECK_ARG(Y && xrec && workspace && xinit && iters_out && active_out, "null argument");
    PNP_CHECK_ARG(M >= 1 && N >= 1 && batch >= 1 && batch <= 65535, "bad sizes");
    PNP_CHECK_ARG(max_iters >= 1 && check_every >= 1, "max_iters and check_every must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PNP_F32) return run_spectral_init<float>(A, Y, xrec, M, N, batch, max_iters, check_every, workspace, xinit, iters_out, active_out, s);
    if (dtype == PNP_F64) return run_spectral_init<double>(A, Y, xrec, M, N, batch, max_iters, check_every, workspace, xinit, iters_out, active_out, s);
    PNP_CHECK_ARG(false, "bad dtype");
}

// deblur_mixed.hip -- Deblur batches whose problems each have a down-sampler and a measurement count M_b of their own (a
// sampling-ratio sweep, scale_percent = 10 .. 100, as ONE batch).
//
// A mixed plan (pnp_deblur_plan_create_mixed) is a plan of deblur.hip without a down-sampler of its own -- twiddles, kernel
// spectrum and FFT scratch for `batch` problems -- plus n_sets distinct down-samplers, concatenated: forward taps g_idx / g_w
// (rows of 4), adjoint CSR (row pointers of N + 1 entries per set with tables, entries a_col / a_val).  Problem b works on the set
// mx_prob[b] points to; the identity set (scale_percent == 100: M = N) has no tables.  Y and the plan's `down` scratch are
// [batch][Mmax], Mmax = max M_b: entries m >= M_b of a row are padding that no kernel here reads.
//
//   gradient : blur (deblur.hip, whole batch) -> k_mx_forward: down_b = sel o (S_b blurred_b + beta * Y_b) -> k_mx_adjoint:
//              res_b = S_b^T down_b -> adjoint blur with the factor scale_b (the scale_pp path of pnp_deblur_grad_pp)
//   objective: blur -> k_mx_forward -> k_mx_obj_sq / k_mx_obj_final: (scale / M_b) * sum over m < M_b of (S_b B z - Y)^2
//   draws    : k_draw_thr_mpp, the statements of k_draw_thr_pp (draw_thr_body.h) over the candidates 0 .. M_b - 1
//
// The tap sum and the CSR sum are written as k_gather4 / k_csr of deblur.hip write them (o = 0 first, the terms in table order)
// and this file is compiled with the same FMA contraction (the compiler's default), so a problem with a down-sampler equals, bit
// for bit, the same problem in a uniform batch of its scale.  An identity problem passes through the same two kernels as copies
// (a uniform identity batch fuses "- Y" into the blur's epilogue instead: equal up to the rounding of the blurred value).
// The objective's sums are those of objective.hip: in double, chunks of 4096 in a fixed order, no atomics.
#include "common.h"
#include "draw.h"
#include "deblur_plan.h"
#include <vector>
#include <cmath>

namespace pnp {
namespace {

using MxProb = pnp_deblur_mixed_prob;

// down[b][m] = sel o (S_b x_b + beta * c[b][m]) for m < M_b, 0 in the padding M_b <= m < Mmax.  x [batch][N]; c, sel, out
// [batch][Mmax].  c / sel / mbd may be NULL (sel and mbd never both).
template <typename T>
__global__ __launch_bounds__(256) void k_mx_forward(const T* __restrict__ x, const MxProb* __restrict__ probs,
                                                    const int32_t* __restrict__ g_idx, const T* __restrict__ g_w, int N, int Mmax,
                                                    T beta, const T* __restrict__ c, const uint8_t* __restrict__ sel,
                                                    const MbDesc* __restrict__ mbd, T* __restrict__ out) {
    const int prob = blockIdx.y;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Mmax) return;
    const MxProb pd = probs[prob];
    const size_t i = (size_t)prob * Mmax + m;
    if (m >= pd.M) {
        out[i] = (T)0;
        return;
    }
    const T* xp = x + (size_t)prob * N;
    T o = 0;
    if (pd.ident) {
        o = xp[m];
    } else {
        const int32_t* idx = g_idx + (size_t)pd.g_base * 4;
        const T* w = g_w + (size_t)pd.g_base * 4;
#pragma unroll
        for (int t = 0; t < 4; ++t) o += w[(size_t)m * 4 + t] * xp[idx[(size_t)m * 4 + t]];
    }
    if (c != nullptr) o += beta * c[i];
    if (sel != nullptr && sel[i] == 0) o = (T)0;
    if (mbd != nullptr && !mb_member(mbd[prob], (uint32_t)m)) o = (T)0;
    out[i] = o;
}

// res[b][n] = (S_b^T down_b)[n]: y [batch][Mmax], out [batch][N]
template <typename T>
__global__ __launch_bounds__(256) void k_mx_adjoint(const T* __restrict__ y, const MxProb* __restrict__ probs,
                                                    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const T* __restrict__ val, int N, int Mmax, T* __restrict__ out) {
    const int prob = blockIdx.y;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const MxProb pd = probs[prob];
    const T* yp = y + (size_t)prob * Mmax;
    T o = 0;
    if (pd.ident) {
        o = yp[n];                                               // (M_b == N == Mmax)
    } else {
        const int32_t* rp = rowptr + pd.rp_base;
        const int32_t* cl = col + pd.nz_base;
        const T* vl = val + pd.nz_base;
        for (int e = rp[n]; e < rp[n + 1]; ++e) o += vl[e] * yp[cl[e]];
    }
    out[(size_t)prob * N + n] = o;
}

// ------------------------------------------------------------------------------- objective (the sums of objective.hip)
constexpr int kSqChunk = 4096;

__device__ __forceinline__ double block_sum_256(double acc, double* red) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// part[b][blk] = sum over the chunk's m < M_b of (fwd - Y)^2; a chunk past M_b holds 0.  fwd, Y [batch][Mmax].
template <typename T>
__global__ __launch_bounds__(256) void k_mx_obj_sq(const T* __restrict__ fwd, const T* __restrict__ Y,
                                                   const MxProb* __restrict__ probs, int Mmax, int nblk, double* __restrict__ part) {
    __shared__ double red[4];
    const int prob = blockIdx.y, M = probs[prob].M;
    const int i0 = blockIdx.x * kSqChunk, i1 = i0 + kSqChunk < M ? i0 + kSqChunk : M;
    const T* f = fwd + (size_t)prob * Mmax;
    const T* y = Y + (size_t)prob * Mmax;
    double acc = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const double d = (double)f[i] - (double)y[i];
        acc += d * d;
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(size_t)prob * nblk + blockIdx.x] = acc;
}

// f_out[b] = (scale / M_b) * sum of problem b's parts: one workgroup per problem
__global__ __launch_bounds__(256) void k_mx_obj_final(const double* __restrict__ part, const MxProb* __restrict__ probs, int nblk,
                                                      double scale, double* __restrict__ f_out) {
    __shared__ double red[4];
    const double* p = part + (size_t)blockIdx.x * nblk;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += p[i];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) f_out[blockIdx.x] = (scale / (double)probs[blockIdx.x].M) * acc;
}

// ------------------------------------------------------------------------------- draws
// k_draw_thr_pp (draw.h) with a population per problem: the candidates of problem b are 0 .. M_vec[b] - 1.  The statements are
// the shared ones, so with the same id, mb, seed and step problem b's descriptor is the one pnp_draw_thresholds_pp(M_b) gives.
// An mb_vec[b] >= M_b selects every candidate: the descriptor then admits EVERY index, consumers stop at M_b themselves.
__global__ __launch_bounds__(256) void k_draw_thr_mpp(const int32_t* __restrict__ M_vec, const int32_t* __restrict__ mb_vec,
                                                      const uint32_t* __restrict__ draw_id, uint64_t seed,
                                                      const uint64_t* __restrict__ seed_vec, uint32_t step0,
                                                      const uint32_t* __restrict__ step_dev, MbDesc* __restrict__ mbd, int fast) {
    constexpr bool MASKED = false;
    if (seed_vec != nullptr) seed = seed_vec[blockIdx.x];      // a seed per problem: its stream is that of a batch drawn with it
    const uint32_t* bitsT = nullptr;
    uint32_t* selbits = nullptr;
    const int H = 1, W = M_vec[blockIdx.x] < 0 ? 0 : M_vec[blockIdx.x];
    const int mb = mb_vec[blockIdx.x] < 1 ? 1 : mb_vec[blockIdx.x];
    const uint64_t id = draw_id != nullptr ? (uint64_t)draw_id[blockIdx.x] : (uint64_t)(int)blockIdx.x;
#define PNP_DRAW_ID id
#include "draw_thr_body.h"
#undef PNP_DRAW_ID
}

// sel[b][m] = m < M_b and m is in problem b's minibatch; row stride Mmax, the padding is 0
__global__ void k_mx_indicator(const MbDesc* __restrict__ mbd, const int32_t* __restrict__ M_vec, uint8_t* __restrict__ sel, int Mmax) {
    const int prob = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mmax) return;
    sel[(size_t)prob * Mmax + i] = (i < M_vec[prob] && mb_member(mbd[prob], (uint32_t)i)) ? 1 : 0;
}

// ------------------------------------------------------------------------------- launch sequences
template <typename T>
int mx_forward(pnp_deblur_plan* p, const void* blurred, T beta, const void* c, const uint8_t* sel, const MbDesc* mbd, void* out,
               hipStream_t s) {
    k_mx_forward<T><<<dim3((p->M + 255) / 256, p->batch), 256, 0, s>>>((const T*)blurred, p->mx_prob, p->g_idx, (const T*)p->g_w, p->N,
                                                                     p->M, beta, (const T*)c, sel, mbd, (T*)out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

template <typename T>
int run_grad_mixed(pnp_deblur_plan* p, const void* z, const void* Y, const uint8_t* sel, const MbDesc* mbd, double scale,
                   const double* scale_pp, void* out, hipStream_t s) {
    const double sqrtN = std::sqrt((double)p->N);
    int rc = deblur_blur(p, z, false, 1.0 / sqrtN, p->r1, s, nullptr, 1.0);
    if (rc) return rc;
    rc = mx_forward<T>(p, p->r1, (T)-1, Y, sel, mbd, p->down, s);               // sel o (S_b B z - Y)
    if (rc) return rc;
    k_mx_adjoint<T><<<dim3((p->N + 255) / 256, p->batch), 256, 0, s>>>((const T*)p->down, p->mx_prob, p->a_rowptr, p->a_col,
                                                                       (const T*)p->a_val, p->N, p->M, (T*)p->r0);
    PNP_CHECK_LAUNCH();
    return deblur_blur(p, p->r0, true, scale / sqrtN, out, s, scale_pp, sqrtN);
}

int grad_mixed(pnp_deblur_plan* p, const void* z, const void* Y, const uint8_t* sel, const MbDesc* mbd, double scale,
               const double* scale_pp, void* out, hipStream_t s) {
    if (p->dtype == PNP_F32) return run_grad_mixed<float>(p, z, Y, sel, mbd, scale, scale_pp, out, s);
    return run_grad_mixed<double>(p, z, Y, sel, mbd, scale, scale_pp, out, s);
}

int forward_mixed(pnp_deblur_plan* p, const void* x, void* out, hipStream_t s) {
    int rc = deblur_blur(p, x, false, 1.0 / std::sqrt((double)p->N), p->r1, s, nullptr, 1.0);
    if (rc) return rc;
    if (p->dtype == PNP_F32) return mx_forward<float>(p, p->r1, 0.f, nullptr, nullptr, nullptr, out, s);
    return mx_forward<double>(p, p->r1, 0.0, nullptr, nullptr, nullptr, out, s);
}

}  // namespace
}  // namespace pnp

using namespace pnp;

#define PNP_MX_PLAN(p) PNP_CHECK_ARG((p)->n_sets > 0 && (p)->mx_prob != nullptr, "not a mixed-scale plan (pnp_deblur_plan_create_mixed)")

// n_sets down-samplers, all HOST arrays: M_set [n_sets]; g_off [n_sets + 1] tap rows of set s = [g_off[s], g_off[s + 1]) of
// g_idx / g_w (M_set[s] rows, or none: the identity set, M_set[s] == H*W); nz_off [n_sets + 1] likewise for a_col / a_val;
// a_rowptr: N + 1 entries per set WITH tables, in set order, each counting from 0.  set_of, M_vec [batch].
extern "C" int pnp_deblur_plan_create_mixed(pnp_deblur_plan** out, int H, int W, int batch, int dtype, const void* Bk, int n_sets,
                                            const int32_t* M_set, const int32_t* g_off, const int32_t* g_idx, const void* g_w,
                                            const int32_t* nz_off, const int32_t* a_rowptr, const int32_t* a_col, const void* a_val,
                                            const int32_t* set_of, const int32_t* M_vec) {
    PNP_CHECK_ARG(out && Bk && M_set && g_off && nz_off && set_of && M_vec, "null argument");
    const long long N = (long long)H * W;
    PNP_CHECK_ARG(H > 0 && W > 0 && (N == 65536 || N == 16384 || N == 4096), "H*W must be 65536 (256x256), 16384 (128x128) or 4096 (64x64)");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    PNP_CHECK_ARG(batch >= 1 && batch <= 65535 && n_sets >= 1 && n_sets <= batch, "need 1 <= n_sets <= batch <= 65535");
    PNP_CHECK_ARG(g_off[0] == 0 && nz_off[0] == 0, "g_off and nz_off start at 0");
    std::vector<int32_t> rp_base(n_sets, 0);
    int n_tab = 0;
    for (int s = 0; s < n_sets; ++s) {
        const int M = M_set[s];
        PNP_CHECK_ARG(M >= 1 && M <= N, "M_s outside [1, H*W]");
        const long long rows = (long long)g_off[s + 1] - g_off[s], nnz = (long long)nz_off[s + 1] - nz_off[s];
        PNP_CHECK_ARG(rows >= 0 && nnz >= 0, "g_off and nz_off must not decrease");
        if (rows == 0) {
            PNP_CHECK_ARG(M == N && nnz == 0, "a set without tables is the identity: M_s == H*W");
            continue;
        }
        PNP_CHECK_ARG(g_idx && g_w && a_rowptr && a_col && a_val, "bilinear operator needs all five arrays");
        PNP_CHECK_ARG(rows == M, "a set's tap rows must number M_s");
        PNP_CHECK_ARG((long long)g_off[s + 1] * 4 < (1ll << 31), "tap tables too large");
        for (long long i = (long long)g_off[s] * 4; i < (long long)g_off[s + 1] * 4; ++i)
            PNP_CHECK_ARG(g_idx[i] >= 0 && g_idx[i] < N, "g_idx outside [0, H*W)");
        const int32_t* rp = a_rowptr + (size_t)n_tab * (N + 1);
        PNP_CHECK_ARG(rp[0] == 0 && rp[N] == nnz, "a_rowptr of a set must run from 0 to its number of entries");
        for (long long n = 0; n < N; ++n) PNP_CHECK_ARG(rp[n] <= rp[n + 1], "a_rowptr must not decrease");
        for (long long e = nz_off[s]; e < nz_off[s + 1]; ++e) PNP_CHECK_ARG(a_col[e] >= 0 && a_col[e] < M, "a_col outside [0, M_s)");
        rp_base[s] = (int32_t)(n_tab * (N + 1));
        ++n_tab;
    }
    int Mmax = 0;
    std::vector<pnp_deblur_mixed_prob> probs(batch);
    for (int b = 0; b < batch; ++b) {
        const int s = set_of[b];
        PNP_CHECK_ARG(s >= 0 && s < n_sets, "set_of out of range");
        PNP_CHECK_ARG(M_vec[b] == M_set[s], "M_vec[b] must be the M of problem b's set");
        const bool ident = g_off[s + 1] == g_off[s];
        probs[b] = {M_set[s], ident ? 1 : 0, g_off[s], rp_base[s], nz_off[s]};
        Mmax = M_set[s] > Mmax ? M_set[s] : Mmax;
    }
    pnp_deblur_plan* p = nullptr;
    int rc = pnp_deblur_plan_create(&p, H, W, batch, dtype, Bk, (int)N, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const size_t rs = dtype == PNP_F32 ? 4 : 8, rows = (size_t)g_off[n_sets], nnz = (size_t)nz_off[n_sets];
    p->M = Mmax;
    p->n_sets = n_sets;
    hipError_t e = hipMalloc((void**)&p->mx_prob, (size_t)batch * sizeof(pnp_deblur_mixed_prob));
    if (e == hipSuccess) e = hipMemcpy(p->mx_prob, probs.data(), (size_t)batch * sizeof(pnp_deblur_mixed_prob), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&p->mx_M, (size_t)batch * 4);
    if (e == hipSuccess) e = hipMemcpy(p->mx_M, M_vec, (size_t)batch * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->down, (size_t)batch * Mmax * rs);
    if (e == hipSuccess && rows > 0) {
        e = hipMalloc((void**)&p->g_idx, rows * 16);
        if (e == hipSuccess) e = hipMemcpy(p->g_idx, g_idx, rows * 16, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&p->g_w, rows * 4 * rs);
        if (e == hipSuccess) e = hipMemcpy(p->g_w, g_w, rows * 4 * rs, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&p->a_rowptr, (size_t)n_tab * (N + 1) * 4);
        if (e == hipSuccess) e = hipMemcpy(p->a_rowptr, a_rowptr, (size_t)n_tab * (N + 1) * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&p->a_col, nnz * 4);
        if (e == hipSuccess) e = hipMemcpy(p->a_col, a_col, nnz * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&p->a_val, nnz * rs);
        if (e == hipSuccess) e = hipMemcpy(p->a_val, a_val, nnz * rs, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        set_error(std::string("pnp_deblur_plan_create_mixed: ") + hipGetErrorString(e));
        pnp_deblur_plan_destroy(p);
        return PNP_ERR_HIP;
    }
    *out = p;
    return PNP_OK;
}

// out = scale_b * B^T S_b^T ( sel o (S_b B z - Y) ), scale_b = scale_pp ? scale_pp[b] : scale; z, out [batch][H*W]; Y, sel
// [batch][Mmax]
extern "C" int pnp_deblur_grad_mixed(pnp_deblur_plan* p, const void* z, const void* Y, const uint8_t* sel, double scale,
                                     const double* scale_pp, void* out, void* stream) {
    PNP_CHECK_ARG(p && z && Y && out, "null argument");
    PNP_MX_PLAN(p);
    return grad_mixed(p, z, Y, sel, nullptr, scale, scale_pp, out, (hipStream_t)stream);
}

extern "C" int pnp_deblur_grad_mb_mixed(pnp_deblur_plan* p, const void* z, const void* Y, const void* mbd, double scale,
                                        const double* scale_pp, void* out, void* stream) {
    PNP_CHECK_ARG(p && z && Y && mbd && out, "null argument");
    PNP_MX_PLAN(p);
    return grad_mixed(p, z, Y, nullptr, (const MbDesc*)mbd, scale, scale_pp, out, (hipStream_t)stream);
}

// out [batch][Mmax] = S_b B x_b, zero in the padding
extern "C" int pnp_deblur_forward_mixed(pnp_deblur_plan* p, const void* x, void* out, void* stream) {
    PNP_CHECK_ARG(p && x && out, "null argument");
    PNP_MX_PLAN(p);
    return forward_mixed(p, x, out, (hipStream_t)stream);
}

extern "C" int pnp_deblur_objective_mixed(pnp_deblur_plan* p, const void* z, const void* Y, double scale, double* f_out,
                                          void* stream) {
    PNP_CHECK_ARG(p && z && Y && f_out, "null argument");
    PNP_MX_PLAN(p);
    hipStream_t s = (hipStream_t)stream;
    int rc = forward_mixed(p, z, p->r0, s);                  // [batch][Mmax] inside r0's [batch][N]; r1 is free again behind it
    if (rc) return rc;
    const int nblk = (p->M + kSqChunk - 1) / kSqChunk;       // <= 16 doubles per problem: r1 holds N >= 4096 elements per problem
    double* part = (double*)p->r1;
    if (p->dtype == PNP_F32)
        k_mx_obj_sq<float><<<dim3(nblk, p->batch), 256, 0, s>>>((const float*)p->r0, (const float*)Y, p->mx_prob, p->M, nblk, part);
    else
        k_mx_obj_sq<double><<<dim3(nblk, p->batch), 256, 0, s>>>((const double*)p->r0, (const double*)Y, p->mx_prob, p->M, nblk, part);
    PNP_CHECK_LAUNCH();
    k_mx_obj_final<<<p->batch, 256, 0, s>>>(part, p->mx_prob, nblk, scale, f_out);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_draw_thresholds_mpp(const int32_t* M_vec, int batch, const int32_t* mb_vec, const uint32_t* draw_id, uint64_t seed,
                                       const uint64_t* seed_vec, uint32_t step0, int nsteps, const uint32_t* step_dev, void* mbd,
                                       void* stream) {
    PNP_CHECK_ARG(mbd != nullptr && mb_vec != nullptr && M_vec != nullptr, "null argument");
    PNP_CHECK_ARG(batch >= 1 && nsteps >= 1 && nsteps <= 65535, "need batch >= 1 and 1 <= nsteps <= 65535");
    k_draw_thr_mpp<<<dim3(batch, nsteps), 256, 0, (hipStream_t)stream>>>(M_vec, mb_vec, draw_id, seed, seed_vec, step0, step_dev, (MbDesc*)mbd,
                                                                         draw_fast_path());
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_indicator_from_thresholds_m(const int32_t* M_vec, int Mmax, int batch, const void* mbd, uint8_t* sel, void* stream) {
    PNP_CHECK_ARG(M_vec && mbd && sel && Mmax >= 1 && batch >= 1, "bad argument");
    k_mx_indicator<<<dim3((Mmax + 255) / 256, batch), 256, 0, (hipStream_t)stream>>>((const MbDesc*)mbd, M_vec, sel, Mmax);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

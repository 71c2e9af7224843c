// vr.hip -- problem-independent pieces of the variance-reduced loops on gfx950:
//   * minibatch draws over a length-M measurement vector (problems/problem.py:110-117: `np.random.choice(M, size,
//     replace=False)` -> 0/1 indicator), as thresholds (draw.h) and, when a caller needs them, as an indicator
//     (Deblur) or an ascending row list (PhaseRetrieval);
//   * the SAGA gradient-table update (algorithms/pnp_saga.py:43-57) as ONE pass over the vectors.
#include "draw.h"

namespace pnp {

__global__ void k_indicator_from_thr(const MbDesc* __restrict__ mbd, uint8_t* __restrict__ sel, int M) {
    const int prob = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    sel[(size_t)prob * M + i] = mb_member(mbd[prob], (uint32_t)i) ? 1 : 0;
}

__global__ void k_indicator_scatter(const int32_t* __restrict__ idx, int n, uint8_t* __restrict__ sel, int M) {
    const int prob = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int i = idx[(size_t)prob * n + j];
    if (i >= 0 && i < M) sel[(size_t)prob * M + i] = 1;
}

// ascending list of the minibatch members of one problem (deterministic: block-wide prefix sum, no atomics)
__global__ __launch_bounds__(256) void k_rows_from_thr(const MbDesc* __restrict__ mbd, int32_t* __restrict__ rows, int M, int mb) {
    __shared__ int wtot[4];
    const int prob = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const MbDesc d = mbd[prob];
    const int per = (M + 255) / 256, i0 = tid * per, i1 = i0 + per < M ? i0 + per : M;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += mb_member(d, (uint32_t)i) ? 1 : 0;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    int pos = incl - cnt;
    for (int q = 0; q < wv; ++q) pos += wtot[q];
    int32_t* out = rows + (size_t)prob * mb;
    for (int i = i0; i < i1; ++i)
        if (mb_member(d, (uint32_t)i)) { if (pos < mb) out[pos] = i; ++pos; }
}

// SAGA step (pnp_saga.py:45-57 with the table sum kept incrementally, which is algebraically sum(table)):
//   old = slot; sum += g - old; v = g - prev + sum / hist; z -= lr * v; slot = g
// `prev` is the slot written by the previous step (it may be this very slot: read before write, same thread).
template <typename T>
__global__ void k_saga_update(T* z, const T* __restrict__ g, T* slot, const T* prev, T* sum, T lr, T inv_hist, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const T gi = g[i], old = slot[i], pv = prev[i];
        const T s = sum[i] + gi - old;
        z[i] -= lr * ((gi - pv) + s * inv_hist);
        slot[i] = gi;
        sum[i] = s;
    }
}

// The same step for a whole batch whose problems replace different rows and step with different sizes (pnp_saga_table_update_pp):
// blockIdx.y = problem, V elements (16 bytes) per thread and pass.  Per element the statements are k_saga_update's, in its order;
// row == prev_row makes `slot` and `prev` the same memory: both are loaded before anything is stored, by the thread that stores.
template <typename T> struct SagaVec;
template <> struct SagaVec<float> { using type = float4; };
template <> struct SagaVec<double> { using type = double2; };

template <typename T>
__global__ __launch_bounds__(256) void k_saga_update_pp(T* z, const T* __restrict__ g, T* table, const int32_t* __restrict__ row,
                                                        const int32_t* __restrict__ prev_row, T* sum, T lr,
                                                        const double* __restrict__ lr_pp, T inv_hist, int batch, int N) {
    using V = typename SagaVec<T>::type;
    constexpr int NV = (int)(sizeof(V) / sizeof(T));
    const int b = blockIdx.y;
    if (lr_pp != nullptr) lr = (T)lr_pp[b];
    const size_t pb = (size_t)b * N;
    T* slot = table + ((size_t)row[b] * batch + b) * N;
    const T* prev = table + ((size_t)prev_row[b] * batch + b) * N;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * NV; i < N; i += gridDim.x * blockDim.x * NV) {
        const V gv = *(const V*)(g + pb + i), ov = *(const V*)(slot + i), pv = *(const V*)(prev + i);
        V sv = *(const V*)(sum + pb + i), zv = *(const V*)(z + pb + i);
        const T* ga = (const T*)&gv; const T* oa = (const T*)&ov; const T* pa = (const T*)&pv;
        T* sa = (T*)&sv; T* za = (T*)&zv;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const T gi = ga[k], old = oa[k], pvk = pa[k];
            const T s = sa[k] + gi - old;
            za[k] -= lr * ((gi - pvk) + s * inv_hist);
            sa[k] = s;
        }
        *(V*)(z + pb + i) = zv;
        *(V*)(slot + i) = gv;
        *(V*)(sum + pb + i) = sv;
    }
}

// k_saga_update_pp with the divisor per problem as well (pnp_saga_table_update_hist_pp): problem b divides its running sum by its OWN
// history length, inv_hist_pp[b] = 1 / hist[b] in double, cast as the scalar is cast and loaded once per workgroup; a problem only names
// rows below its own hist[b] (row[b], prev_row[b]: the caller checks them), so the rows of the dense table beyond them are never
// touched.  Everything else is k_saga_update_pp's, statement for statement, row[b] == prev_row[b] included.
template <typename T>
__global__ __launch_bounds__(256) void k_saga_update_hist_pp(T* z, const T* __restrict__ g, T* table, const int32_t* __restrict__ row,
                                                             const int32_t* __restrict__ prev_row, T* sum, T lr,
                                                             const double* __restrict__ lr_pp, T inv_hist,
                                                             const double* __restrict__ inv_hist_pp, int batch, int N) {
    using V = typename SagaVec<T>::type;
    constexpr int NV = (int)(sizeof(V) / sizeof(T));
    const int b = blockIdx.y;
    if (lr_pp != nullptr) lr = (T)lr_pp[b];
    if (inv_hist_pp != nullptr) inv_hist = (T)inv_hist_pp[b];
    const size_t pb = (size_t)b * N;
    T* slot = table + ((size_t)row[b] * batch + b) * N;
    const T* prev = table + ((size_t)prev_row[b] * batch + b) * N;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * NV; i < N; i += gridDim.x * blockDim.x * NV) {
        const V gv = *(const V*)(g + pb + i), ov = *(const V*)(slot + i), pv = *(const V*)(prev + i);
        V sv = *(const V*)(sum + pb + i), zv = *(const V*)(z + pb + i);
        const T* ga = (const T*)&gv; const T* oa = (const T*)&ov; const T* pa = (const T*)&pv;
        T* sa = (T*)&sv; T* za = (T*)&zv;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const T gi = ga[k], old = oa[k], pvk = pa[k];
            const T s = sa[k] + gi - old;
            za[k] -= lr * ((gi - pvk) + s * inv_hist);
            sa[k] = s;
        }
        *(V*)(z + pb + i) = zv;
        *(V*)(slot + i) = gv;
        *(V*)(sum + pb + i) = sv;
    }
}

}  // namespace pnp

using namespace pnp;

extern "C" int pnp_draw_thresholds(int M, int batch, int mb, uint64_t seed, uint32_t step0, int nsteps,
                                   const uint32_t* step_dev, void* mbd, void* stream) {
    PNP_CHECK_ARG(mbd != nullptr, "null argument");
    PNP_CHECK_ARG(M >= 1 && batch >= 1 && mb >= 1 && nsteps >= 1 && nsteps <= 65535, "need M, batch, mb >= 1 and 1 <= nsteps <= 65535");
    k_draw_thr<false><<<dim3(batch, nsteps), 256, 0, (hipStream_t)stream>>>(nullptr, 1, M, mb, seed, step0, step_dev, (MbDesc*)mbd, nullptr, draw_fast_path());
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_draw_thresholds_pp(int M, int batch, const int32_t* mb_vec, const uint32_t* draw_id, uint64_t seed, uint32_t step0,
                                      int nsteps, const uint32_t* step_dev, void* mbd, void* stream) {
    PNP_CHECK_ARG(mbd != nullptr && mb_vec != nullptr, "null argument");
    PNP_CHECK_ARG(M >= 1 && batch >= 1 && nsteps >= 1 && nsteps <= 65535, "need M, batch >= 1 and 1 <= nsteps <= 65535");
    k_draw_thr_pp<false><<<dim3(batch, nsteps), 256, 0, (hipStream_t)stream>>>(nullptr, 1, M, mb_vec, draw_id, seed, step0, step_dev,
                                                                              (MbDesc*)mbd, nullptr, draw_fast_path());
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_indicator_from_thresholds(int M, int batch, const void* mbd, uint8_t* sel, void* stream) {
    PNP_CHECK_ARG(mbd && sel && M >= 1 && batch >= 1, "bad argument");
    k_indicator_from_thr<<<dim3((M + 255) / 256, batch), 256, 0, (hipStream_t)stream>>>((const MbDesc*)mbd, sel, M);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_indicator_from_indices(const int32_t* idx, int n, int M, int batch, uint8_t* sel, void* stream) {
    PNP_CHECK_ARG(idx && sel && n >= 0 && M >= 1 && batch >= 1, "bad argument");
    PNP_CHECK_HIP(hipMemsetAsync(sel, 0, (size_t)batch * M, (hipStream_t)stream));
    if (n > 0) {
        k_indicator_scatter<<<dim3((n + 255) / 256, batch), 256, 0, (hipStream_t)stream>>>(idx, n, sel, M);
        PNP_CHECK_LAUNCH();
    }
    return PNP_OK;
}

extern "C" int pnp_rows_from_thresholds(int M, int batch, int mb, const void* mbd, int32_t* rows, void* stream) {
    PNP_CHECK_ARG(mbd && rows && M >= 1 && batch >= 1 && mb >= 1 && mb <= M, "bad argument");
    k_rows_from_thr<<<batch, 256, 0, (hipStream_t)stream>>>((const MbDesc*)mbd, rows, M, mb);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_saga_table_update(void* z, const void* g, void* slot, const void* prev, void* sum, double lr,
                                     double inv_hist, size_t n, int dtype, void* stream) {
    PNP_CHECK_ARG(z && g && slot && prev && sum, "null argument");
    if (n == 0) return PNP_OK;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    if (dtype == PNP_F32)
        k_saga_update<float><<<grid, 256, 0, (hipStream_t)stream>>>((float*)z, (const float*)g, (float*)slot, (const float*)prev,
                                                                      (float*)sum, (float)lr, (float)inv_hist, n);
    else if (dtype == PNP_F64)
        k_saga_update<double><<<grid, 256, 0, (hipStream_t)stream>>>((double*)z, (const double*)g, (double*)slot, (const double*)prev,
                                                                       (double*)sum, lr, inv_hist, n);
    else PNP_CHECK_ARG(false, "bad dtype");
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_saga_table_update_pp(void* z, const void* g, void* table, const int32_t* row, const int32_t* prev_row, void* sum,
                                        double lr, const double* lr_pp, double inv_hist, int hist, int batch, int N, int dtype,
                                        void* stream) {
    PNP_CHECK_ARG(z && g && table && row && prev_row && sum, "null argument");
    PNP_CHECK_ARG(hist >= 1 && batch >= 1 && batch <= 65535 && N >= 4 && N % 4 == 0, "need hist >= 1, 1 <= batch <= 65535 and N a multiple of 4");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    PNP_CHECK_ARG((((uintptr_t)z | (uintptr_t)g | (uintptr_t)table | (uintptr_t)sum) & 15) == 0, "z, g, table and sum must be 16-byte aligned");
    const int nv = dtype == PNP_F32 ? 4 : 2, per = (N / nv + 255) / 256;
    const dim3 grid(per < 256 ? per : 256, batch);
    if (dtype == PNP_F32)
        k_saga_update_pp<float><<<grid, 256, 0, (hipStream_t)stream>>>((float*)z, (const float*)g, (float*)table, row, prev_row, (float*)sum,
                                                                         (float)lr, lr_pp, (float)inv_hist, batch, N);
    else
        k_saga_update_pp<double><<<grid, 256, 0, (hipStream_t)stream>>>((double*)z, (const double*)g, (double*)table, row, prev_row,
                                                                          (double*)sum, lr, lr_pp, inv_hist, batch, N);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

extern "C" int pnp_saga_table_update_hist_pp(void* z, const void* g, void* table, const int32_t* row, const int32_t* prev_row, void* sum,
                                             double lr, const double* lr_pp, double inv_hist, const double* inv_hist_pp, int hist,
                                             int batch, int N, int dtype, void* stream) {
    PNP_CHECK_ARG(z && g && table && row && prev_row && sum, "null argument");
    PNP_CHECK_ARG(hist >= 1 && batch >= 1 && batch <= 65535 && N >= 4 && N % 4 == 0, "need hist >= 1, 1 <= batch <= 65535 and N a multiple of 4");
    PNP_CHECK_ARG(dtype == PNP_F32 || dtype == PNP_F64, "bad dtype");
    PNP_CHECK_ARG((((uintptr_t)z | (uintptr_t)g | (uintptr_t)table | (uintptr_t)sum) & 15) == 0, "z, g, table and sum must be 16-byte aligned");
    const int nv = dtype == PNP_F32 ? 4 : 2, per = (N / nv + 255) / 256;
    const dim3 grid(per < 256 ? per : 256, batch);
    if (dtype == PNP_F32)
        k_saga_update_hist_pp<float><<<grid, 256, 0, (hipStream_t)stream>>>((float*)z, (const float*)g, (float*)table, row, prev_row,
                                                                              (float*)sum, (float)lr, lr_pp, (float)inv_hist, inv_hist_pp,
                                                                              batch, N);
    else
        k_saga_update_hist_pp<double><<<grid, 256, 0, (hipStream_t)stream>>>((double*)z, (const double*)g, (double*)table, row, prev_row,
                                                                               (double*)sum, lr, lr_pp, inv_hist, inv_hist_pp, batch, N);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}

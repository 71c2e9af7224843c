// dncnn.hip -- DnCNN-17 prox (reference denoisers/RealSN_DnCNN.py:16-42 around the network of
// denoisers/DeepDenoisers/model/models.py:5-22 / realSN_models.py:4-21) on gfx950: the network around its middle layers.
//
//   k_first   1 -> 64 channels, 3x3, ReLU; fused with the min-max normalisation and the
//             "1 + sigma/255/2" range scaling of the wrapper (RealSN_DnCNN.py:19-29)
//   middle    64 -> 64 channels, 3x3, BatchNorm folded into weights + bias, ReLU; x15 per forward = 99.8 % of the FLOPs.
//             One of four conv forms on the matrix cores, the conv modes of the table below: 0 = direct, 1 = Winograd F(2,3)
//             along x (dncnn_direct.hip), 5 = Winograd F(4x4,3x3) (dncnn_wino44.hip), 6 = the same on 3 x bf16 splits
//             (dncnn_wino44b.hip)
//   k_last    64 -> 1 channel, 3x3; fused with x = xtilde - r, the inverse scaling and the squared
//             error of Problem.PSNR (RealSN_DnCNN.py:36-40, problems/problem.py:33-35)
#include "direct.h"
#include "wino44.h"
#include "wino44b.h"
#include "reduce.h"
#include <vector>
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace pnp {

constexpr int C = 64;             // feature channels

// ------------------------------------------------------------------------------- first layer
// xt = ((z - lo) / (hi - lo)) * srange + sshift ; act[c] = relu(sum_t w[c][t] * xt[tap t])
// MMO form (clamp01): xt = clamp(z, 0, 1); act[c] = leaky_relu(b[c] + sum_t ..., slope)   (MMODenoise.py:30,90-91)
template <typename T>
__global__ __launch_bounds__(256) void k_first(const T* __restrict__ z, const T* __restrict__ mm,
                                               const float* __restrict__ w, const float* __restrict__ bfirst,
                                               float* __restrict__ out, int H, int W, double srange, double sshift,
                                               int clamp01, float slope) {
    __shared__ float ws[C * 9];
    __shared__ float bs[C];
    for (int i = threadIdx.x; i < C * 9; i += 256) ws[i] = w[i];
    if (threadIdx.x < C) bs[threadIdx.x] = bfirst[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const T lo = mm ? mm[2 * b] : (T)0, hi = mm ? mm[2 * b + 1] : (T)1;
    const T* zi = z + (size_t)b * H * W;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        float q = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            T u = zi[yy * W + xx];
            if (clamp01) {
                u = u < (T)0 ? (T)0 : (u > (T)1 ? (T)1 : u);
            } else {
                u = (u - lo) / (hi - lo);
                u = u * (T)srange + (T)sshift;
            }
            q = (float)u;
        }
        v[t] = q;
    }
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) a = fmaf(ws[c * 9 + t], v[t], a);
        a += bs[c];                                             // 0 for the DnCNN family (bias-free first layer)
        out[((size_t)b * C + c) * H * W + p] = a > 0.f ? a : slope * a + 0.f;
    }
}

// ------------------------------------------------------------------------------- last layer
// r = sum_{c,t} w[c][t] * act[c][tap t];  x = xt - r;  x = (x - sshift)/srange;  z = x*(hi-lo)+lo
// HBM/L2-bound (reads the 64-channel activation once): 16 x 64 output tile per workgroup, 4 channels
// at a time staged in LDS as [4][18][72] (columns tx0-4 .. tx0+67, 16-byte aligned rows; 21 KB, so a whole
// B = 16 grid of 1024 workgroups is resident at once), the next slab's loads in flight during the current one, every
// thread owns a 1 x 4 pixel strip: one ds_read_b128 + two ds_read_b32 per row and channel.
constexpr int LT_R = 16, LT_C = 64, LT_CK = 4, LT_PR = LT_R + 2, LT_PC = LT_C + 8;

template <typename T>
__global__ __launch_bounds__(256) void k_last(const float* __restrict__ act, const float* __restrict__ w,
                                              const T* zin, const T* __restrict__ mm,      // zin may alias zout (in-place prox): no __restrict__
                                              T* zout, float* __restrict__ r_out,
                                              const T* __restrict__ xrec, double* __restrict__ sse_part, int H, int W,
                                              double srange, double sshift, int skip01, float blast) {
    __shared__ float ws[C * 9];
    __shared__ __attribute__((aligned(16))) float tile[LT_CK * LT_PR * LT_PC];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < C * 9; i += 256) ws[i] = w[i];
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * LT_R, tx0 = blockIdx.x * LT_C;
    const int py = tid >> 4, px = (tid & 15) * 4;               // this thread's strip inside the tile
    const float* ab = act + (size_t)b * C * H * W;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    // software pipeline over the 8-channel slabs: the global loads of slab k+1 are in flight (in registers) while
    // slab k is consumed out of LDS, so a workgroup never sits on an exposed HBM round trip per slab
    constexpr int SLAB = LT_CK * LT_PR * (LT_PC / 4);          // float4 elements of one slab (2592)
    constexpr int PER_T = (SLAB + 255) / 256;                  // 11 per thread
    float4 pre[PER_T];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int k = 0; k < PER_T; ++k) {
            const int i = tid + 256 * k;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < SLAB) {
                const int ch = i / (LT_PR * (LT_PC / 4)), rem = i - ch * (LT_PR * (LT_PC / 4));
                const int ry = rem / (LT_PC / 4), cx = rem - ry * (LT_PC / 4);
                const int y = ty0 - 1 + ry, x = tx0 - 4 + 4 * cx;
                if (y >= 0 && y < H && x >= 0 && x < W)
                    v = *reinterpret_cast<const float4*>(ab + ((size_t)(c0 + ch) * H + y) * W + x);
            }
            pre[k] = v;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < C; c0 += LT_CK) {
        __syncthreads();                                        // the previous slab has been consumed
#pragma unroll
        for (int k = 0; k < PER_T; ++k) {
            const int i = tid + 256 * k;
            if (i < SLAB) reinterpret_cast<float4*>(tile)[i] = pre[k];   // slab layout == linear float4 index
        }
        __syncthreads();
        if (c0 + LT_CK < C) fetch(c0 + LT_CK);
#pragma unroll
        for (int ch = 0; ch < LT_CK; ++ch) {
            const float* wc = ws + (c0 + ch) * 9;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const float* row = tile + (ch * LT_PR + py + dy) * LT_PC + px + 4;     // LDS col of pixel px
                const float4 m = *reinterpret_cast<const float4*>(row);
                const float l = row[-1], rr = row[4];
                const float w0 = wc[dy * 3], w1 = wc[dy * 3 + 1], w2 = wc[dy * 3 + 2];
                r[0] = fmaf(w0, l, fmaf(w1, m.x, fmaf(w2, m.y, r[0])));
                r[1] = fmaf(w0, m.x, fmaf(w1, m.y, fmaf(w2, m.z, r[1])));
                r[2] = fmaf(w0, m.y, fmaf(w1, m.z, fmaf(w2, m.w, r[2])));
                r[3] = fmaf(w0, m.z, fmaf(w1, m.w, fmaf(w2, rr, r[3])));
            }
        }
    }
    double err = 0.0;
    const int y = ty0 + py;
    if (y < H) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = tx0 + px + j;
            if (x >= W) continue;
            const size_t p = (size_t)b * H * W + (size_t)y * W + x;
            r[j] += blast;                                      // 0 for the DnCNN family (bias-free last layer)
            if (r_out != nullptr) r_out[p] = r[j];
            if (zout != nullptr && skip01) {
                // MMO form: out = clip(clamp(x,0,1) + net(clamp(x,0,1)), 0, 1), fp32 like the reference's tensors
                // (MMODenoise.py:30-32,98, then the float64 np.clip of :128 which is a no-op after the clamp)
                const float xin = (float)zin[p];
                float v = (xin < 0.f ? 0.f : (xin > 1.f ? 1.f : xin)) + r[j];
                v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
                zout[p] = (T)v;
                if (xrec != nullptr) {
                    const double d = (double)xrec[p] - (double)(T)v;
                    err += d * d;
                }
            } else if (zout != nullptr) {
                const T lo = mm[2 * b], hi = mm[2 * b + 1];
                T v = (zin[p] - lo) / (hi - lo);
                v = v * (T)srange + (T)sshift;                  // xtilde, kept in T (f64 in the reference wrapper)
                v = v - (T)r[j];                                // f64 - f32 in the reference wrapper
                v = (v - (T)sshift) / (T)srange;
                v = v * (hi - lo) + lo;
                zout[p] = v;
                if (xrec != nullptr) {
                    const double d = (double)xrec[p] - (double)v;
                    err += d * d;
                }
            }
        }
    }
    if (sse_part != nullptr) {
        err = wave_sum(err);
        if ((tid & 63) == 0) red[tid >> 6] = err;
        __syncthreads();
        if (tid == 0)
            sse_part[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    }
}

// the rest of k_last behind the fused last layer (conv mode 5, ReLU net; wino44.h): r = the sum of the up to four 6 x 6
// patches part[b][by][bx] that cover a pixel (own block, the vertical, the horizontal, the diagonal neighbour: one fixed
// order), then the same epilogue.  Workgroup = 4 x 64 pixels (16 blocks of one block row), one pixel per thread.
template <typename T>
__global__ __launch_bounds__(256) void k_last_patches(const float* __restrict__ part, const T* zin, const T* __restrict__ mm,
                                                      T* zout, float* __restrict__ r_out, const T* __restrict__ xrec,
                                                      double* __restrict__ sse_part, int H, int W, double srange, double sshift,
                                                      float blast) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int iy = tid >> 6, ix = tid & 3, bx = blockIdx.x * 16 + ((tid >> 2) & 15), by = blockIdx.y;
    const int y = 4 * by + iy, x = 4 * bx + ix;
    const int NBX = W / 4, NBY = H / 4;
    const float* pb = part + (size_t)b * NBY * NBX * 36;
    auto at = [&](int qy, int qx, int py, int px) { return pb[((size_t)qy * NBX + qx) * 36 + py * 6 + px]; };
    const int vy = iy == 0 ? -1 : iy == 3 ? 1 : 0, vx = ix == 0 ? -1 : ix == 3 ? 1 : 0;     // neighbour whose spill-over reaches here
    const bool hv = vy != 0 && by + vy >= 0 && by + vy < NBY, hh = vx != 0 && bx + vx >= 0 && bx + vx < NBX;
    const int py = iy + 1, px = ix + 1, pyn = py - 4 * vy, pxn = px - 4 * vx;              // position in own / neighbour patch
    float r = at(by, bx, py, px);
    if (hv) r += at(by + vy, bx, pyn, px);
    if (hh) r += at(by, bx + vx, py, pxn);
    if (hv && hh) r += at(by + vy, bx + vx, pyn, pxn);
    r += blast;                                                 // 0 for the DnCNN family (bias-free last layer)
    const size_t p = (size_t)b * H * W + (size_t)y * W + x;
    if (r_out != nullptr) r_out[p] = r;
    double err = 0.0;
    if (zout != nullptr) {
        const T lo = mm ? mm[2 * b] : (T)0, hi = mm ? mm[2 * b + 1] : (T)1;
        T v = (zin[p] - lo) / (hi - lo);
        v = v * (T)srange + (T)sshift;
        v = v - (T)r;
        v = (v - (T)sshift) / (T)srange;
        v = v * (hi - lo) + lo;
        zout[p] = v;
        if (xrec != nullptr) {
            const double d = (double)xrec[p] - (double)v;
            err = d * d;
        }
    }
    if (sse_part != nullptr) {
        err = wave_sum(err);
        if ((tid & 63) == 0) red[tid >> 6] = err;
        __syncthreads();
        if (tid == 0)
            sse_part[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    }
}

__global__ void k_sum_parts(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    double s = 0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += part[(size_t)blockIdx.x * nparts + i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace pnp
using namespace pnp;

// the conv forms of the middle layers (dncnn_conv.h), one row per conv mode
static const ConvMode kModes[] = {
    {0, direct_supports, direct_layer_bytes, direct_pack, direct_layer, direct_debug_clock, false},
    {1, direct_supports, wino23_layer_bytes, wino23_pack, wino23_layer, wino23_debug_clock, false},
    {5, wino44_supports, wino44_layer_bytes, wino44_pack, wino44_layer, wino44_debug_clock, true},
    {6, wino44b_supports, wino44b_layer_bytes, wino44b_pack, wino44b_layer, wino44b_debug_clock, false},
};
constexpr int NMODES = sizeof(kModes) / sizeof(kModes[0]);

static const ConvMode* find_mode(int mode) {
    for (const ConvMode& m : kModes)
        if (m.mode == mode) return &m;
    return nullptr;
}

// The conv form a plan of H x W runs for the mode `requested`.  strict (pnp_dncnn_set_winograd): an unknown mode, or a mode the
// image size rules out, is an error.  Not strict (PNP_DNCNN_WINOGRAD at plan creation): an unknown value means the default 5, and
// a mode the image size rules out falls back to 1 (5 and 6 need H % 8 == 0 and W % 64 == 0; 0 and 1 run on every plan).
static int resolve_conv_mode(int requested, int H, int W, bool strict, const ConvMode** out) {
    const ConvMode* m = find_mode(requested);
    PNP_CHECK_ARG(m || !strict,
                  "mode must be 0 (direct), 1 (Winograd F(2,3) along x), 5 (Winograd F(4x4,3x3)) or 6 (the same on 3 x bf16 splits)");
    if (!m) m = find_mode(5);
    PNP_CHECK_ARG(m->supports(H, W) || !strict, "Winograd F(4x4,3x3) needs H % 8 == 0 and W % 64 == 0");
    *out = m->supports(H, W) ? m : find_mode(1);
    return PNP_OK;
}

struct pnp_dncnn_plan {
    int n_mid, H, W, batch, num_cu;
    float *w_first, *w_last, *bias;              // device
    void* wconv[NMODES];                         // packed middle-layer weights per row of kModes; null where the size rules it out
    const ConvMode* conv;                        // the conv form of the middle layers
    float* b_first;                              // [64] device, zeros unless pnp_dncnn_set_affine
    float b_last, slope;                         // last-layer bias, LeakyReLU slope (0 = ReLU)
    bool edge_fusion;                            // conv mode 5, ReLU, float: the last layer inside the last middle layer
    float* part;                                 // its output patches [B][H/4][W/4][36] (wino44.h); null without F(4x4,3x3)
    float *act0, *act1, *zeros;                  // [B][64][H][W] x2; a zero word for halo padding
    double* mm;                                  // [B][2] (as double or float depending on call)
    double* sse_part;                            // [B][H*W/256]
    // optional in-band timing of the MFMA layers (hipEvents on the caller's stream, no sync)
    bool profile;
    std::vector<hipEvent_t> ev;                  // pairs: [2i] before, [2i+1] after the n_mid launches
    size_t ev_used;
    double prof_ms;
    long prof_launches;
};

static void plan_free(pnp_dncnn_plan* p) {
    for (void* q : p->wconv) (void)hipFree(q);
    for (void* q : {(void*)p->bias, (void*)p->w_first, (void*)p->w_last, (void*)p->act0, (void*)p->act1, (void*)p->zeros,
                    (void*)p->mm, (void*)p->sse_part, (void*)p->b_first, (void*)p->part})
        (void)hipFree(q);
    for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
    delete p;
}

// one middle layer of the plan's network in its conv form; bias and weights of layer `l`
static ConvLayerArgs conv_args(const pnp_dncnn_plan* p, int l, const float* in, float* out, hipStream_t s) {
    return {in, out, p->wconv[p->conv - kModes], l, p->bias + (size_t)l * C, p->zeros, p->H, p->W, p->batch, p->num_cu, p->slope, s};
}

extern "C" int pnp_dncnn_plan_create(pnp_dncnn_plan** out, int n_mid, const float* w_first, const float* w_mid,
                                     const float* b_mid, const float* w_last, int H, int W, int batch) {
    PNP_CHECK_ARG(out && w_first && w_mid && b_mid && w_last, "null argument");
    PNP_CHECK_ARG(n_mid >= 1 && batch >= 1, "n_mid and batch must be >= 1");
    PNP_CHECK_ARG(H % 8 == 0 && W % 32 == 0 && (H * W) % 256 == 0, "H must be a multiple of 8, W of 32");
    auto* p = new pnp_dncnn_plan{};
    p->n_mid = n_mid; p->H = H; p->W = W; p->batch = batch;
    hipDeviceProp_t prop;
    int dev = 0;
    PNP_CHECK_HIP(hipGetDevice(&dev));
    PNP_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    p->num_cu = prop.multiProcessorCount;
    const char* ev = getenv("PNP_DNCNN_WINOGRAD");
    (void)resolve_conv_mode(ev ? atoi(ev) : 5, H, W, false, &p->conv);
    // PNP_DNCNN_EDGE_FUSION=0: the separate last-layer kernel everywhere (A/B runs and tests; read once per plan)
    const char* ef = getenv("PNP_DNCNN_EDGE_FUSION");
    p->edge_fusion = !(ef && atoi(ef) == 0);
    const size_t act_bytes = (size_t)batch * C * H * W * sizeof(float);
    hipError_t e = hipSuccess;
    auto alloc = [&](auto** dst, size_t bytes, const void* src = nullptr) {     // device buffer, uploaded from the host if src
        if (e == hipSuccess) e = hipMalloc(dst, bytes);
        if (e == hipSuccess && src) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    };
    for (int i = 0; i < NMODES; ++i) {                          // the weights of every conv form the image size allows
        if (!kModes[i].supports(H, W)) continue;
        std::vector<char> w(kModes[i].layer_bytes() * n_mid);
        kModes[i].pack(w_mid, n_mid, w.data());
        alloc(&p->wconv[i], w.size(), w.data());
    }
    alloc(&p->bias, (size_t)n_mid * C * sizeof(float), b_mid);
    alloc(&p->w_first, C * 9 * sizeof(float), w_first);
    alloc(&p->w_last, C * 9 * sizeof(float), w_last);
    alloc(&p->b_first, C * sizeof(float));
    if (e == hipSuccess) e = hipMemset(p->b_first, 0, C * sizeof(float));
    alloc(&p->act0, act_bytes);
    alloc(&p->act1, act_bytes);
    alloc(&p->zeros, 256);
    if (e == hipSuccess) e = hipMemset(p->zeros, 0, 256);
    alloc(&p->mm, (size_t)batch * 2 * sizeof(double));
    alloc(&p->sse_part, (size_t)batch * (H * W / 256) * sizeof(double));
    if (wino44_supports(H, W)) alloc(&p->part, wino44_part_floats(H, W, batch) * sizeof(float));
    if (e != hipSuccess) {
        set_error(std::string("pnp_dncnn_plan_create: ") + hipGetErrorString(e));
        plan_free(p);
        return PNP_ERR_HIP;
    }
    *out = p;
    return PNP_OK;
}

extern "C" int pnp_dncnn_plan_destroy(pnp_dncnn_plan* p) {
    if (p) plan_free(p);
    return PNP_OK;
}

namespace {
template <typename T>
int run_dncnn(pnp_dncnn_plan* p, const T* z_in, bool normalise, double sigma_net, T* z_out, float* r_out,
              const T* xrec, double* sse_out, hipStream_t s, bool mmo = false) {
    const int H = p->H, W = p->W, B = p->batch, HW = H * W;
    T* mm = normalise ? (T*)p->mm : nullptr;             // raw network (no wrapper scaling): lo = 0, hi = 1
    double srange = 1.0, sshift = 0.0;
    if (normalise) {
        k_minmax<T><<<B, 256, 0, s>>>(z_in, HW, mm);
        PNP_CHECK_LAUNCH();
        srange = 1.0 + sigma_net / 255.0 / 2.0;
        sshift = (1.0 - srange) / 2.0;
    }
    dim3 pg(HW / 256, B);
    k_first<T><<<pg, 256, 0, s>>>(z_in, mm, p->w_first, p->b_first, p->act0, H, W, srange, sshift, mmo ? 1 : 0, p->slope);
    PNP_CHECK_LAUNCH();
    float *src = p->act0, *dst = p->act1;
    // the DnCNN family on the F(4x4,3x3) kernel: the 64 -> 1 output conv runs in the last middle layer's epilogue
    const bool fuse_last = p->edge_fusion && p->conv->fuses_last && p->slope == 0.f && !mmo && std::is_same<T, float>::value &&
                           p->part != nullptr;
    const bool prof = p->profile && p->ev_used + 2 <= p->ev.size();
    if (prof) PNP_CHECK_HIP(hipEventRecord(p->ev[p->ev_used], s));
    for (int l = 0; l < p->n_mid; ++l) {
        ConvLayerArgs a = conv_args(p, l, src, dst, s);
        if (fuse_last && l == p->n_mid - 1) { a.wlast = p->w_last; a.part = p->part; }
        const int rc = p->conv->layer(a);
        if (rc != PNP_OK) return rc;
        std::swap(src, dst);
    }
    if (prof) { PNP_CHECK_HIP(hipEventRecord(p->ev[p->ev_used + 1], s)); p->ev_used += 2; }
    if (fuse_last) {
        const dim3 fg(W / 64, H / 4, B);
        k_last_patches<T><<<fg, 256, 0, s>>>(p->part, z_in, mm, z_out, r_out, xrec, sse_out ? p->sse_part : nullptr, H, W, srange,
                                             sshift, p->b_last);
        PNP_CHECK_LAUNCH();
        if (sse_out) {
            k_sum_parts<<<B, 64, 0, s>>>(p->sse_part, (int)(fg.x * fg.y), sse_out);
            PNP_CHECK_LAUNCH();
        }
        return PNP_OK;
    }
    dim3 lg((W + LT_C - 1) / LT_C, (H + LT_R - 1) / LT_R, B);
    k_last<T><<<lg, 256, 0, s>>>(src, p->w_last, z_in, mm, z_out, r_out, xrec, sse_out ? p->sse_part : nullptr, H, W,
                                 srange, sshift, mmo ? 1 : 0, p->b_last);
    PNP_CHECK_LAUNCH();
    if (sse_out) {
        k_sum_parts<<<B, 64, 0, s>>>(p->sse_part, (int)(lg.x * lg.y), sse_out);
        PNP_CHECK_LAUNCH();
    }
    return PNP_OK;
}
}  // namespace

// ---- test hooks: one middle layer on caller-provided buffers (guard-band tests)
extern "C" size_t pnp_dncnn_debug_w44_floats(void) { return wino44_layer_bytes() / sizeof(float); }

extern "C" int pnp_dncnn_debug_w44_weights(pnp_dncnn_plan* p, int layer, float* dst, void* stream) {
    PNP_CHECK_ARG(p && dst && layer >= 0 && layer < p->n_mid, "bad argument");
    const char* w = (const char*)p->wconv[find_mode(5) - kModes];
    PNP_CHECK_ARG(w != nullptr, "the plan's image size rules out the F(4x4,3x3) kernel (mode 5): no such weights");
    PNP_CHECK_HIP(hipMemcpyAsync(dst, w + (size_t)layer * wino44_layer_bytes(), wino44_layer_bytes(), hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream));
    return PNP_OK;
}

extern "C" int pnp_dncnn_debug_mid_layer(pnp_dncnn_plan* p, int layer, const float* in, float* out, const float* w44_override,
                                         int w44_rows, void* stream) {
    PNP_CHECK_ARG(p && in && out && layer >= 0 && layer < p->n_mid && w44_rows >= 0 && w44_rows <= 2, "bad argument");
    ConvLayerArgs a = conv_args(p, layer, in, out, (hipStream_t)stream);
    a.force_rows = w44_rows;
    a.w44_override = w44_override;
    return p->conv->layer(a);
}

extern "C" int pnp_dncnn_debug_fused_last(pnp_dncnn_plan* p, const float* in, float* part, int w44_rows, void* stream) {
    PNP_CHECK_ARG(p && in && part && w44_rows >= 0 && w44_rows <= 2, "bad argument");
    ConvLayerArgs a = conv_args(p, p->n_mid - 1, in, nullptr, (hipStream_t)stream);
    a.force_rows = w44_rows;
    a.wlast = p->w_last;
    a.part = part;
    return p->conv->layer(a);
}

extern "C" int pnp_dncnn_set_affine(pnp_dncnn_plan* p, const float* b_first, float b_last, float negative_slope) {
    PNP_CHECK_ARG(p != nullptr, "null plan");
    PNP_CHECK_ARG(negative_slope >= 0.f && negative_slope < 1.f, "negative_slope must be in [0, 1)");
    if (b_first) PNP_CHECK_HIP(hipMemcpy(p->b_first, b_first, C * sizeof(float), hipMemcpyHostToDevice));
    else PNP_CHECK_HIP(hipMemset(p->b_first, 0, C * sizeof(float)));
    p->b_last = b_last;
    p->slope = negative_slope;
    return PNP_OK;
}

extern "C" int pnp_dncnn_set_winograd(pnp_dncnn_plan* p, int enable) {
    PNP_CHECK_ARG(p != nullptr, "null plan");
    return resolve_conv_mode(enable, p->H, p->W, true, &p->conv);
}

extern "C" int pnp_dncnn_profile_begin(pnp_dncnn_plan* p, int max_calls) {
    PNP_CHECK_ARG(p && max_calls > 0, "bad argument");
    while (p->ev.size() < (size_t)2 * max_calls) {
        hipEvent_t e;
        PNP_CHECK_HIP(hipEventCreate(&e));
        p->ev.push_back(e);
    }
    p->profile = true; p->ev_used = 0; p->prof_ms = 0; p->prof_launches = 0;
    return PNP_OK;
}

extern "C" int pnp_dncnn_profile_end(pnp_dncnn_plan* p, double* avg_ms_per_launch, long* launches) {
    PNP_CHECK_ARG(p && avg_ms_per_launch && launches, "null argument");
    p->profile = false;
    for (size_t i = 0; i + 1 < p->ev_used; i += 2) {
        PNP_CHECK_HIP(hipEventSynchronize(p->ev[i + 1]));
        float ms = 0;
        PNP_CHECK_HIP(hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]));
        p->prof_ms += ms;
        p->prof_launches += p->n_mid;
    }
    *launches = p->prof_launches;
    *avg_ms_per_launch = p->prof_launches ? p->prof_ms / (double)p->prof_launches : 0.0;
    return PNP_OK;
}

// Diagnostic: in-kernel shader clock and phase shares of the conv kernel under load.  Runs `reps` back-to-back
// conv launches on the plan's activation buffers (contents arbitrary), the last one stamped; returns the median
// over workgroups of (shader cycles, 100 MHz reference ticks) spent in the tile loop.  PNP_DEBUG_STAMPS=1 prints
// the conv form's phase split; PNP_DEBUG_ABL (direct form) and PNP_W44_VAR (modes 5, 6) select an ablation build.
extern "C" int pnp_dncnn_debug_clock(pnp_dncnn_plan* p, int reps, double* cycles, double* ref_ticks, void* stream) {
    PNP_CHECK_ARG(p && cycles && ref_ticks && reps >= 1, "bad argument");
    std::vector<double> c, r;
    const int rc = p->conv->debug_clock(conv_args(p, 0, p->act0, p->act1, (hipStream_t)stream), reps, c, r);
    if (rc != PNP_OK) return rc;
    std::sort(c.begin(), c.end());
    std::sort(r.begin(), r.end());
    *cycles = c[c.size() / 2];
    *ref_ticks = r[r.size() / 2];
    return PNP_OK;
}

extern "C" int pnp_dncnn_forward(pnp_dncnn_plan* p, const float* x, float* r, void* stream) {
    PNP_CHECK_ARG(p && x && r, "null argument");
    return run_dncnn<float>(p, x, false, 0.0, nullptr, r, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int pnp_mmo_denoise(pnp_dncnn_plan* p, const void* z_in, void* z_out, int dtype, const void* xrec,
                               double* sse_out, void* stream) {
    PNP_CHECK_ARG(p && z_in && z_out, "null argument");
    PNP_CHECK_ARG(!(sse_out && !xrec), "sse_out needs xrec");
    if (dtype == PNP_F32)
        return run_dncnn<float>(p, (const float*)z_in, false, 0.0, (float*)z_out, nullptr, (const float*)xrec, sse_out,
                                (hipStream_t)stream, true);
    if (dtype == PNP_F64)
        return run_dncnn<double>(p, (const double*)z_in, false, 0.0, (double*)z_out, nullptr, (const double*)xrec, sse_out,
                                 (hipStream_t)stream, true);
    PNP_CHECK_ARG(false, "bad dtype");
}

extern "C" int pnp_dncnn_denoise(pnp_dncnn_plan* p, const void* z_in, void* z_out, int dtype, double sigma_net,
                                 const void* xrec, double* sse_out, void* stream) {
    PNP_CHECK_ARG(p && z_in && z_out, "null argument");
    PNP_CHECK_ARG(!(sse_out && !xrec), "sse_out needs xrec");
    if (dtype == PNP_F32)
        return run_dncnn<float>(p, (const float*)z_in, true, sigma_net, (float*)z_out, nullptr, (const float*)xrec, sse_out,
                                (hipStream_t)stream);
    if (dtype == PNP_F64)
        return run_dncnn<double>(p, (const double*)z_in, true, sigma_net, (double*)z_out, nullptr, (const double*)xrec,
                                 sse_out, (hipStream_t)stream);
    PNP_CHECK_ARG(false, "bad dtype");
}

// wino44_common.h -- what the two F(4x4,3x3) Winograd conv kernels share: dncnn_wino44.hip (fp32, conv mode 5) and
// dncnn_wino44b.hip (3 x bf16 split, conv mode 6) differ in their matrix-core steps, V images and epilogues; the transform
// arithmetic, the LDS-DMA front end that brings a region's halo planes in, the patch in flight, the weight cursor and the
// host-side U = G g G^T are the same and live here once.
#pragma once
#include "common.h"
#include <vector>
#include <cstdio>

namespace pnp {
namespace w44c {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) float lds_f;
typedef __attribute__((address_space(3))) f32x2 lds_f2;
typedef __attribute__((address_space(3))) f32x4 lds_f4;

constexpr int C = 64;
constexpr int TC = 64;                                // region width: 16 blocks of 4 x 4
constexpr int PC = 72;                                // LDS row: image columns [tx0 - 4, tx0 + 68) = eighteen 16-byte chunks
constexpr int KC = 8;                                 // input channels per chunk
constexpr int NCH = C / KC;
constexpr unsigned DUMMY = 1u << 27;                  // descriptor flag: padding chunk of a plane
// the halo planes of a region of NG block rows (the fp32 kernel: 2 or 1; the bf16 kernel: 2)
template <int NG> struct HaloGeo {
    static constexpr int TR = 4 * NG, PR = TR + 2;                 // output rows, halo rows
    static constexpr int PLANE = NG == 2 ? 768 : 512;              // PR x 72 payload + pad: 0 mod 64 dwords (ds_read_b128 lane groups mix two planes)
    static constexpr int DBUF = KC * PLANE;                        // floats per input buffer: 24 / 16 DMA pieces of 1 KiB
    static constexpr int PPW = DBUF / 256 / 4;                     // 6 / 4 pieces per wave
};

// ---- Winograd arithmetic ------------------------------------------------------------------------------------------------------
// B^T of F(4,3) applied to six values
__device__ __forceinline__ void bt6(float d0, float d1, float d2, float d3, float d4, float d5, float (&v)[6]) {
    const float t1 = __builtin_fmaf(-4.f, d2, d4), t2 = __builtin_fmaf(-4.f, d1, d3);
    const float t3 = d4 - d2, sd = d3 - d1;
    v[0] = __builtin_fmaf(4.f, d0, __builtin_fmaf(-5.f, d2, d4));
    v[1] = t1 + t2;
    v[2] = t1 - t2;
    v[3] = __builtin_fmaf(2.f, sd, t3);
    v[4] = __builtin_fmaf(-2.f, sd, t3);
    v[5] = __builtin_fmaf(4.f, d1, __builtin_fmaf(-5.f, d3, d5));
}
// A^T of F(4,3) applied to six values
template <typename T> __device__ __forceinline__ void at6(T m0, T m1, T m2, T m3, T m4, T m5, T (&y)[4]) {
    const T s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
    y[0] = (m0 + s12) + s34;
    y[1] = 2.f * d34 + d12;                                 // contracted to (packed) fma
    y[2] = 4.f * s34 + s12;
    y[3] = (8.f * d34 + d12) + m5;
}
// The transform on the packed-f32 ALU (a v_pk_* beside f32 MFMAs costs what one plain instruction does).  Row pass of
// B^T d B: the loaded row holds (d1, d2) and (d3, d4) as aligned register pairs, so
//     (t2, t1) = (d3, d4) - 4 (d1, d2)      (sd, t3) = (d3, d4) - (d1, d2)
//     (V1, V2) = (t1 + t2, t1 - t2)         (V3, V4) = (t3 + 2 sd, t3 - 2 sd)        [half-selects: op_sel, hand-written]
// and V0, V5 (their inputs straddle the pairs) stay scalar: 8 instructions instead of 12.  The results are kept as the
// pairs (V0, V5), (V1, V2), (V3, V4), so the column pass runs on whole pairs: 12 packed instructions for two columns.
__device__ __forceinline__ f32x2 pk_sum_diff(f32x2 a) {             // (a.lo + a.hi, a.hi - a.lo)
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a));
    return r;
}
__device__ __forceinline__ f32x2 pk_hi_pm_2lo(f32x2 a) {            // (a.hi + 2 a.lo, a.hi - 2 a.lo)
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, 2.0, %1 op_sel:[0,0,1] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(r) : "v"(a));
    return r;
}
// B^T of F(4,3) on six pairs
__device__ __forceinline__ void bt6_pk(f32x2 q0, f32x2 q1, f32x2 q2, f32x2 q3, f32x2 q4, f32x2 q5, f32x2 (&v)[6]) {
    const f32x2 t1 = q4 - 4.f * q2, t2 = q3 - 4.f * q1;
    const f32x2 t3 = q4 - q2, sd = q3 - q1;
    v[0] = 4.f * q0 + (q4 - 5.f * q2);
    v[1] = t1 + t2;
    v[2] = t1 - t2;
    v[3] = 2.f * sd + t3;
    v[4] = t3 - 2.f * sd;
    v[5] = 4.f * q1 + (q5 - 5.f * q3);
}

// ---- the patch a thread transforms, and the weight stream of a wave -----------------------------------------------------------
struct Patch {
    f32x2 a; f32x4 m; f32x2 e;                                 // one patch row in flight: LDS columns 4tc + 2..3, 4..7, 8..9
    f32x2 t[6][3];                                             // row transforms as register pairs: (V0, V5), (V1, V2), (V3, V4) of row r
    f32x2 v[6];                                                // one transformed pair of columns on its way to the V image
};
// patch row R of d buffer DPAR (c.dsrc[DPAR]: this lane's patch) into c.P, in two halves; all ten floats are "used"
// (slice_valu) so that the reads stay one conflict-free ds_read_b128 and two ds_read_b64 (narrowed to the six needed values
// they become three 4-way bank-conflicting ds_read2_b32)
template <int DPAR, int R, int HALF, typename CT> __device__ __forceinline__ void patch_load(CT& c) {
    const lds_f* row = c.dsrc[DPAR] + R * PC;                    // 16-byte aligned
    if (HALF == 0) { c.P.a = *(const lds_f2*)(row + 2); c.P.e = *(const lds_f2*)(row + 8); }
    else c.P.m = *(const lds_f4*)(row + 4);
}
// weight stream of a wave (base of both kernels' Ctx): a scalar cursor (1 KiB per load; advanced on the scalar ALU,
// re-defined through an empty asm so that it stays ONE register pair instead of 144 hoisted addresses) + the lane's 16
// bytes as a 32-bit vector offset.  The ring the loads go to (URING deep) is the kernel's own.
struct WeightCursor {
    const __attribute__((address_space(1))) char* ucur;
    unsigned ulane;
    __device__ __forceinline__ f32x4 uload_next() {
        const f32x4 u = *(const __attribute__((address_space(1))) f32x4*)(ucur + ulane);
        ucur += 1024;
        asm volatile("" : "+s"(ucur));
        return u;
    }
};

// ---- halo front end: a region's (8 + 2 rows) x 72 columns of 8 channels, global -> LDS by LDS-DMA -------------------------------
// The DMA is inline asm, invisible to the compiler's s_waitcnt insertion -- visible, it makes every LDS read after a DMA
// wait for vmcnt(0), which drains the weight ring at every step.  The kernels wait for it with one hand-counted vmcnt per
// chunk (vector-memory operations leave the queue in issue order).
// one 1-KiB piece global -> LDS: lane's 16 bytes from rsrc.base + voff (an offset beyond num_records reads zeros)
__device__ __forceinline__ void dma_piece_asm(unsigned voff, i32x4 rsrc, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" :: "v"(voff), "s"(rsrc), "s"(lds_byte_addr) : "memory");
}

// Regions are numbered in units of 8 x 64 pixels (`tile0` + ...) whatever the form: a 4 x 64 region u (NG = 1) is sub-row
// u & 1 of unit tile0 + (u >> 1), so that a launch of the one-row form can take over the units a two-row launch left.
template <int NG> struct Regions {
    int tile0, tiles_x, units_per_img;
    __device__ __forceinline__ Regions(int H, int W, int tile0_) : tile0(tile0_), tiles_x(W / TC), units_per_img(tiles_x * (H / 8)) {}
    // region u of the launch: image b, first output row / column
    __device__ __forceinline__ void operator()(int u, int& b, int& ty0, int& tx0) const {
        const int t = tile0 + (NG == 2 ? u : u >> 1);
        b = t / units_per_img;
        const int t2 = t - b * units_per_img;
        ty0 = (t2 / tiles_x) * 8 + (NG == 2 ? 0 : 4 * (u & 1));
        tx0 = (t2 % tiles_x) * TC;
    }
};
// DMA piece descriptor of piece i of wave wv (pieces wv, wv + 4, ... of a chunk's DBUF / 256 are its own): bits 0..26 = element
// offset of the lane's 16-byte chunk inside the chunk's 8 channel planes, bit 27 = padding, bits 28..31 = which image edge
// would put the chunk outside
template <int NG> __device__ __forceinline__ unsigned piece_desc(int wv, int i, int lane, int H, int W) {
    using G = HaloGeo<NG>;
    const int q = (wv + 4 * i) * 64 + lane;
    const int c = q / (G::PLANE / 4), r = q - c * (G::PLANE / 4);
    const int ry = r / 18, cx4 = 4 * (r - ry * 18);
    const unsigned edge = (ry == 0 ? 1u : 0u) | (ry == G::PR - 1 ? 2u : 0u) | (cx4 == 0 ? 4u : 0u) | (cx4 == TC + 4 ? 8u : 0u);
    return r < G::PR * 18 ? ((unsigned)((c * H + ry) * W + cx4) | (edge << 28)) : DUMMY;
}
// DMA state of a tile: the buffer base of its chunk 0 and, per piece, the lane's byte offset (or an offset beyond
// num_records) -- the same for all chunks of the tile, whose bases are chunk_bytes = 8 planes apart
template <int NG> struct TileDma { size_t base; unsigned voff[HaloGeo<NG>::PPW]; };
// The one guard of the halo loads, in two halves (the kernels' tile_dma puts them together for a tile t).  A lane whose chunk
// lies outside the image (edge bits) or is padding carries an offset beyond num_records, and the descriptor's range check
// returns zeros without touching memory.  t == ntiles is "none": the prefetch behind a workgroup's last region, whose base
// would be one image beyond the buffer -- every lane out of range.
// the descriptor bits that rule a piece out for the tile t at (ty0, tx0)
template <int NG> __device__ __forceinline__ unsigned bad_mask(int t, int ntiles, int ty0, int tx0, int H, int W) {
    return t < ntiles ? ((((ty0 == 0 ? 1u : 0u) | (ty0 + HaloGeo<NG>::TR == H ? 2u : 0u) | (tx0 == 0 ? 4u : 0u) | (tx0 + TC == W ? 8u : 0u)) << 28) | DUMMY)
                      : 0xFFFFFFFFu;
}
// the lane's byte offset for a piece, or an offset beyond num_records
__device__ __forceinline__ unsigned piece_voff(unsigned pdesc, unsigned bad) { return (pdesc & bad) == 0u ? 4u * (pdesc & 0x07FFFFFFu) : 0x80000000u; }
// buffer descriptor of chunk k of a tile: 48-bit base, stride 0, num_records = 2 GiB, 32-bit data format
template <int NG> __device__ __forceinline__ i32x4 chunk_rsrc(const TileDma<NG>& td, int k, size_t chunk_bytes) {
    const size_t base = td.base + (size_t)k * chunk_bytes;
    i32x4 rs;
    rs.x = (int)(unsigned)base; rs.y = (int)(unsigned)(base >> 32) & 0xFFFF; rs.z = (int)0x80000000u; rs.w = 0x00020000;
    return rs;
}
// piece i of a chunk -> d buffer `buf` (the two d buffers stand at the start of the workgroup's LDS, byte address lds0)
template <int NG> __device__ __forceinline__ void dma_piece(const TileDma<NG>& td, i32x4 rs, unsigned lds0, int wv, int buf, int i) {
    dma_piece_asm(td.voff[i], rs, lds0 + 4u * (unsigned)(buf * HaloGeo<NG>::DBUF + (wv + 4 * i) * 256));
}
// (tile_dma as ONE shared function, the two-chunk prologue and the "chunk K + 2 of this tile, or chunk 0 / 1 of the next"
//  selector stay in the kernels, as a few lines over the functions above: moved here, each of them changed the generated code
//  of k_mid_wino44 -- DESIGN 3.1)

// ---- host side ------------------------------------------------------------------------------------------------------------
// U = G g G^T of one (cout, cin) filter g [3][3]: u[6 xi_y + xi_x], evaluated in float64 and rounded to fp32
inline void filter_u(const float* g, float (&u)[36]) {
    static const double G[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    for (int xy = 0; xy < 6; ++xy)
        for (int xx = 0; xx < 6; ++xx) {
            double s = 0;
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) s += G[xy][dy] * G[xx][dx] * (double)g[dy * 3 + dx];
            u[6 * xy + xx] = (float)s;
        }
}
// PNP_DEBUG_STAMPS summary of a stamped launch: h = {cycles, ticks, chunk-end waits (+ steps 0..5 of the chunks << 32: the bf16
// kernel only), epilogue} per workgroup
inline void print_stamp_summary(const char* kernel, const std::vector<unsigned long long>& h, int grid) {
    double wsum = 0, esum = 0, rsum = 0;
    for (int i = 0; i < grid; ++i) { wsum += (double)(h[4 * i + 2] & 0xFFFFFFFFull); rsum += (double)(h[4 * i + 2] >> 32); esum += h[4 * i + 3]; }
    fprintf(stderr, "[%s stamps] mean cycles per WG: chunk-end wait + barrier %.0f  epilogue %.0f  (mode 6: steps 0..5 of the chunks %.0f)\n",
            kernel, wsum / grid, esum / grid, rsum / grid);
}

}  // namespace w44c
}  // namespace pnp

// dncnn_wino44.hip -- the 64 -> 64 channel 3x3 layer of the DnCNN prox (reference denoisers/DeepDenoisers/model/models.py:
// 13-17: conv + BatchNorm + ReLU, BN folded by the caller) as the TWO-dimensional Winograd minimal-filtering algorithm
// F(4x4, 3x3): per 4x4 output block and (cout, cin)
//     V = B^T d B  (d = the 6x6 input patch)      U = G g G^T  (6x6 per (cout, cin), pre-transformed at plan creation)
//     M_xi = sum_cin U_xi V_xi  (36 multiply-adds per cin for 16 outputs)          Y = A^T M A
// i.e. ONE QUARTER of the direct form's matrix-core work (F(4,3) along x alone: one half); fp32 throughout.
//
// Organisation (one workgroup = 4 waves = one per SIMD, persistent over 8 x 64 output regions in the XCD-aware order; 4 x 64
// regions with half the accumulators for launches that would leave CUs idle -- Geo<NG> below):
//   * the 36 transformed-domain products are 36 independent [64 cout] x [64 cin] x [32 blocks] GEMMs; wave wv owns output
//     channels [16 wv, 16 wv + 16) and keeps ALL 36 x 2 accumulator quads (288 registers) for the region's 2 x 16 blocks;
//   * input channels go by in chunks of 8: the chunk's (8+2) x 72 halo planes arrive by LDS-DMA, every thread transforms
//     ONE (channel, block) patch -- the transform is shared by the four waves, i.e. by all 64 output channels -- and
//     writes its 36 values to the V image [xi][k-row][block][row of blocks][k-step], from which a wave's B operands of
//     one xi (both block rows) are a single conflict-free ds_read_b128 (one block row: ds_read_b64);
//   * transformed weights do not fit registers (36 x 64 x 64): they stream from L2 in MFMA operand order, one 16-byte
//     load per lane and xi pair and chunk through a ring of 18 loads in flight, each value used by two MFMAs (the two
//     block rows);
//   * software pipeline over chunks: while the MFMAs of chunk k run, the same wave transforms chunk k + 1 and the DMA of
//     chunk k + 2 is in flight; one barrier per chunk.
#include "common.h"
#include "wino44.h"
#include "wino44_common.h"
#include "tilewalk.h"
#include <vector>
#include <utility>
#include <cstdlib>

namespace pnp {
namespace w44 {

using namespace w44c;              // transform arithmetic, halo front end, Patch, weight cursor, C / TC / PC / KC / NCH

// NG = block rows per region: 2 (8 x 64 outputs, 72 accumulator quads per wave; the throughput form) or 1 (4 x 64, 36 quads:
// twice the regions for launches that would otherwise leave CUs idle -- a single 256 x 256 image is 128 regions of 8 x 64)
template <int NG_> struct Geo : HaloGeo<NG_> {                     // TR, PR, PLANE, DBUF, PPW: wino44_common.h
    static constexpr int NG = NG_;
    static constexpr int VPL = 128 * NG;                           // floats per xi plane of V: [4 k-rows][16 blocks][NG block rows][2 k-steps]
    static constexpr int VBUF = 36 * VPL;
    static constexpr int LDS_FLOATS = 2 * HaloGeo<NG_>::DBUF + 2 * VBUF;         // 120 KiB / 68 KiB
    static constexpr int NQ_AGPR = NG == 2 ? 64 : 36;              // accumulator quads kept in AGPRs (of 72: block row 0 and xi < 28 of row 1; of 36: all)
    static constexpr bool in_agpr(int g, int xi) { return g * 36 + xi < NQ_AGPR; }
};
constexpr int URING = 18;                              // weight loads in flight per lane

// hand-issued MFMAs: the accumulator quad lives in AGPRs (AG) or VGPRs; the first product of a tile takes the constant-zero
// SrcC form.  (Left to the compiler, all 72 quads are sent to the 256 AGPRs and the overflow is shuffled around.)
// hipcc does not look inside inline asm, so its hazard recognizer protects nothing here: if register pressure makes it
// split an accumulator's live range, the copy it puts next to the MFMA reads the 4th register (written by the last pass)
// stale.  Wait states inside every statement cost 30 cycles per MFMA, so instead the kernel keeps the pressure low enough
// that no accumulator is ever moved (all 256 AGPRs are accumulators, the epilogue reads them in small batches) and
// tests/test_cpu_host.py::test_w44_accumulators_untouched checks the generated code for it.
#define PNP_MFMA_PRE ""
#define PNP_MFMA_POST ""
template <bool AG> __device__ __forceinline__ void mfma(f32x4& acc, float w, float v) {
    if (AG) asm volatile(PNP_MFMA_PRE "v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" PNP_MFMA_POST : "+a"(acc) : "v"(w), "v"(v));
    else asm volatile(PNP_MFMA_PRE "v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" PNP_MFMA_POST : "+v"(acc) : "v"(w), "v"(v));
}
template <bool AG> __device__ __forceinline__ void mfma_first(f32x4& acc, float w, float v) {
    if (AG) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" PNP_MFMA_POST : "=&a"(acc) : "v"(w), "v"(v));
    else asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" PNP_MFMA_POST : "=&v"(acc) : "v"(w), "v"(v));
}

// ---- memory streams of the main loop ------------------------------------------------------------------------------------------
// * LDS-DMA (activations): the halo front end of wino44_common.h, inline asm the compiler does not count.  One hand-counted
//   vmcnt wait per chunk (sched_barriers pin the order of everything else around it).
// * weights: plain loads, a ring of URING 16-byte values per lane; the compiler waits for them itself (its counts do not
//   include the DMA pieces, so its waits are stricter than needed while pieces are in flight, never weaker).
// * LDS: plain reads / writes, software-pipelined in the source (B operands one xi ahead, patch rows one slice ahead).
template <int NG_> struct Ctx : WeightCursor {              // + the weight stream of this wave (ucur, ulane, uload_next)
    static constexpr int NG = NG_;
    using G = Geo<NG_>;
    f32x4 acc[NG_][36];
    f32x4 ur[URING];
    Patch P;
    f32x2 b[2][NG_];                                           // B operands of the current / next xi: [parity][block row]
    const lds_f* dsrc[2];                                      // this lane's patch in the two d buffers
    lds_f* vdst[2];                                            // its V item in the two V buffers
    const lds_f* vsrc0[2];                                     // its B operands (both block rows: 16 bytes) in the two V buffers
};
// One memory instruction beside an f32 MFMA is free, two per gap kept up cost up to an MFMA (tools/microbench/
// mfma_f32_fillers.hip; an isolated pair costs far less: DESIGN 3.1), and vector-ALU work is cheapest in blocks; so a step (two xi = 8 MFMAs) has fixed slots, pinned by
// sched_barriers.  Two block rows (step2): every memory instruction of a chunk has a gap of its own and the vector-ALU
// blocks stand alone (tools/check_w44_gaps.py, tests/test_cpu_w44_gaps.py hold the generated code to it) --
//     M1 | B(xi1) | M2 | a | M3 | VALU block | M4 | b | M5 | B(xi0') | M6 | c | M7 | d | M8 | ring reload
//     step 0:          a, b = reads of patch row 0   (no VALU: reload of step 17)  d = DMA piece 0
//     step p = 1..6:   a = DMA piece p (p < 6)   VALU = row transform p - 1        b, c = reads of patch row p (p < 6)
//     step 7 / 9 / 11: VALU = column transform 0 / 1 / 2                           b, c, d = its V writes 0..2
//     step 8 / 10 / 12: a, b, c = its V writes 3..5                                steps 13..17: B reads and reloads only
// (the gap behind M8 of step 17 belongs to the B read of the next chunk's first xi, behind the barrier: that step's ring
//  reload waits for the free VALU gap of the next chunk's step 0.)
// One block row (step; half the gaps for nearly the same memory instructions: they share) --
//     M1 | B(xi1) | M3 | VALU block of transform slice p, slice LDS op 1 | M5 | B(xi0') | M7 | DMA piece p, slice LDS ops 2, 3, ring reload
#define PNP_SLOT() __builtin_amdgcn_sched_barrier(0)

// transform slice SL of the patch (d buffer DPAR -> V buffer DPAR): 0..5 = row transforms, 6 / 8 / 10 = column transforms of
// the column pairs (0, 5) / (1, 2) / (3, 4); the six value pairs wait in P.v for their write slots
constexpr int col_pair(int sl) { return (sl - 6) / 2; }
constexpr bool is_col_slice(int sl) { return sl == 6 || sl == 8 || sl == 10; }
template <int SL, typename CT> __device__ __forceinline__ void slice_valu(CT& c) {
    Patch& P = c.P;
    if constexpr (SL < 6) {
        asm volatile("" :: "v"(P.a.x), "v"(P.e.y));
        const f32x2 p12 = {P.m.x, P.m.y}, p34 = {P.m.z, P.m.w};
        const f32x2 A = p34 - 4.f * p12;                          // (t2, t1)
        const f32x2 Bv = p34 - p12;                               // (sd, t3)
        P.t[SL][1] = pk_sum_diff(A);
        P.t[SL][2] = pk_hi_pm_2lo(Bv);
        // (the last FMA of each as asm with its own destination: hipcc picks the two-address v_fmac_f32 and then moves the
        //  result into the pair)
        float v0, v5;
        asm("v_fma_f32 %0, 4.0, %1, %2" : "=v"(v0) : "v"(P.a.y), "v"(__builtin_fmaf(-5.f, P.m.y, P.m.w)));
        asm("v_fma_f32 %0, 4.0, %1, %2" : "=v"(v5) : "v"(P.m.x), "v"(__builtin_fmaf(-5.f, P.m.z, P.e.x)));
        P.t[SL][0] = f32x2{v0, v5};
    } else if constexpr (is_col_slice(SL)) {
        constexpr int cp = col_pair(SL);
        bt6_pk(P.t[0][cp], P.t[1][cp], P.t[2][cp], P.t[3][cp], P.t[4][cp], P.t[5][cp], P.v);
    }
}
// pair Y (0..5) of the V writes of column slice SL: one ds_write2st64_b32
template <int DPAR, int SL, int Y, typename CT> __device__ __forceinline__ void v_write(CT& c) {
    constexpr int VPL = CT::G::VPL;
    constexpr int cp = col_pair(SL), xa = cp == 0 ? 0 : cp == 1 ? 1 : 3, xb = cp == 0 ? 5 : cp == 1 ? 2 : 4;
    c.vdst[DPAR][(Y * 6 + xa) * VPL] = c.P.v[Y].x;
    c.vdst[DPAR][(Y * 6 + xb) * VPL] = c.P.v[Y].y;
}
// LDS operation N (0..2) of slice SL: the next patch row's reads (SL < 5) or two of the six pairs of V writes (column slices)
template <int DPAR, int SL, int N, typename CT> __device__ __forceinline__ void slice_lds(CT& c) {
    if constexpr (SL < 5) {
        if constexpr (N < 2) patch_load<DPAR, SL + 1, N>(c);
    } else if constexpr (is_col_slice(SL)) {
        v_write<DPAR, SL, 2 * N>(c);
        v_write<DPAR, SL, 2 * N + 1>(c);
    }
}
// B operands of xi: one ds_read_b64 (one block row) / one ds_read_b128 (both block rows)
template <int VPAR, int XI, typename CT> __device__ __forceinline__ void b_load(CT& c) {
    if constexpr (CT::NG == 1) c.b[XI & 1][0] = *(const lds_f2*)(c.vsrc0[VPAR] + XI * CT::G::VPL);
    else {
        const f32x4 q = *(const lds_f4*)(c.vsrc0[VPAR] + XI * CT::G::VPL);
        c.b[XI & 1][0] = f32x2{q.x, q.y};
        c.b[XI & 1][CT::NG - 1] = f32x2{q.z, q.w};
    }
}
// MFMA of block row GR (nothing for a block row the region does not have): first k-step of a xi (constant-zero SrcC in
// chunk 0) / second k-step
template <int K, int XI, int GR, typename CT> __device__ __forceinline__ void mfma_j0(CT& c, float u, f32x2 (&b)[CT::NG]) {
    if constexpr (GR < CT::NG) {
        if constexpr (K == 0) mfma_first<CT::G::in_agpr(GR, XI)>(c.acc[GR][XI], u, b[GR].x);
        else mfma<CT::G::in_agpr(GR, XI)>(c.acc[GR][XI], u, b[GR].x);
    }
}
template <int XI, int GR, typename CT> __device__ __forceinline__ void mfma_j1(CT& c, float u, f32x2 (&b)[CT::NG]) {
    if constexpr (GR < CT::NG) mfma<CT::G::in_agpr(GR, XI)>(c.acc[GR][XI], u, b[GR].y);
}

// step (K, P) of the main loop, one block row: xi = 2P, 2P + 1; dma(piece) issues DMA piece `piece` of chunk K + 2.
// VAR (ablation builds, timing only): 10 = no transform arithmetic, 11 = no DMA, 12 = no weight reloads, 13 = no B reads,
// 14 = no transform LDS traffic, 15 = bare MFMAs
template <int K, int P, int VAR, typename CT, typename DMA> __device__ __forceinline__ void step(CT& c, DMA&& dma) {
    static_assert(CT::NG == 1, "two block rows: step2");
    constexpr int X0 = 2 * P, X1 = 2 * P + 1, SQ = K * 18 + P;
    constexpr int VPAR = K & 1, DPAR = (K + 1) & 1;
    const f32x4 u = c.ur[SQ % URING];
    f32x2 b0[1] = {c.b[0][0]}, b1[1];
    mfma_j0<K, X0, 0>(c, u.x, b0);                   PNP_SLOT();          // M1
    if constexpr (VAR != 13 && VAR != 15) b_load<VPAR, X1>(c);
    PNP_SLOT();
    mfma_j1<X0, 0>(c, u.y, b0);                      PNP_SLOT();          // M3
    if constexpr (VAR != 10 && VAR != 15) slice_valu<P>(c);
    PNP_SLOT();
    if constexpr (VAR != 14 && VAR != 15) slice_lds<DPAR, P, 0>(c);
    PNP_SLOT();
    b1[0] = c.b[1][0];
    mfma_j0<K, X1, 0>(c, u.z, b1);                   PNP_SLOT();          // M5
    if constexpr (X1 + 1 < 36 && VAR != 13 && VAR != 15) b_load<VPAR, X1 + 1>(c);
    PNP_SLOT();
    mfma_j1<X1, 0>(c, u.w, b1);                      PNP_SLOT();          // M7
    if constexpr (P < CT::G::PPW && VAR != 11 && VAR != 15) dma(P);
    if constexpr (VAR != 14 && VAR != 15) slice_lds<DPAR, P, 1>(c);
    PNP_SLOT();
    if constexpr (VAR != 14 && VAR != 15) slice_lds<DPAR, P, 2>(c);
    if constexpr (VAR != 12 && VAR != 15 && SQ + URING < NCH * 18) c.ur[SQ % URING] = c.uload_next();
    PNP_SLOT();
}
// two block rows: what stands in slot S (0..3 = a..d of the table above PNP_SLOT) of step P, and the step's VALU block
template <int DPAR, int P, int S, int VAR, typename CT, typename DMA> __device__ __forceinline__ void slot2(CT& c, DMA&& dma) {
    constexpr bool LDS = VAR != 14 && VAR != 15, DM = VAR != 11 && VAR != 15;
    if constexpr (P == 0) {
        if constexpr (S < 2 && LDS) patch_load<DPAR, 0, S>(c);
        if constexpr (S == 3 && DM) dma(0);
    } else if constexpr (P < 6) {
        if constexpr (S == 0 && DM) dma(P);
        if constexpr ((S == 1 || S == 2) && LDS) patch_load<DPAR, P, S - 1>(c);
    } else if constexpr (P >= 7 && P <= 12 && LDS) {
        constexpr int SL = 6 + 2 * ((P - 7) / 2), Y = (P & 1) ? S - 1 : S + 3;       // odd step: b, c, d = 0..2; even step: a, b, c = 3..5
        if constexpr (Y >= 0 && Y < 6) v_write<DPAR, SL, Y>(c);
    }
}
template <int P, typename CT> __device__ __forceinline__ void valu2(CT& c) {
    if constexpr (P >= 1 && P <= 6) slice_valu<P - 1>(c);
    else if constexpr (P == 7 || P == 9 || P == 11) slice_valu<P - 1>(c);              // column slices 6, 8, 10
}
template <int K, int P, int VAR, typename CT, typename DMA> __device__ __forceinline__ void step2(CT& c, DMA&& dma) {
    static_assert(CT::NG == 2 && CT::G::PPW == 6, "one DMA piece in each of the steps 0..5");
    constexpr int X0 = 2 * P, X1 = 2 * P + 1, SQ = K * 18 + P;
    constexpr int VPAR = K & 1, DPAR = (K + 1) & 1;
    const f32x4 u = c.ur[SQ % URING];
    f32x2 b0[2] = {c.b[0][0], c.b[0][1]}, b1[2];
    mfma_j0<K, X0, 0>(c, u.x, b0);                   PNP_SLOT();          // M1
    if constexpr (VAR != 13 && VAR != 15) b_load<VPAR, X1>(c);
    PNP_SLOT();
    mfma_j0<K, X0, 1>(c, u.x, b0);                   PNP_SLOT();          // M2
    slot2<DPAR, P, 0, VAR>(c, dma);
    PNP_SLOT();
    mfma_j1<X0, 0>(c, u.y, b0);                      PNP_SLOT();          // M3
    if constexpr (VAR != 10 && VAR != 15) valu2<P>(c);
    if constexpr (P == 0 && K > 0 && VAR != 12 && VAR != 15 && SQ - 1 + URING < NCH * 18) c.ur[(SQ - 1) % URING] = c.uload_next();
    PNP_SLOT();
    mfma_j1<X0, 1>(c, u.y, b0);                      PNP_SLOT();          // M4
    slot2<DPAR, P, 1, VAR>(c, dma);
    PNP_SLOT();
    b1[0] = c.b[1][0]; b1[1] = c.b[1][1];
    mfma_j0<K, X1, 0>(c, u.z, b1);                   PNP_SLOT();          // M5
    if constexpr (X1 + 1 < 36 && VAR != 13 && VAR != 15) b_load<VPAR, X1 + 1>(c);
    PNP_SLOT();
    mfma_j0<K, X1, 1>(c, u.z, b1);                   PNP_SLOT();          // M6
    slot2<DPAR, P, 2, VAR>(c, dma);
    PNP_SLOT();
    mfma_j1<X1, 0>(c, u.w, b1);                      PNP_SLOT();          // M7
    slot2<DPAR, P, 3, VAR>(c, dma);
    PNP_SLOT();
    mfma_j1<X1, 1>(c, u.w, b1);                      PNP_SLOT();          // M8
    if constexpr (P < 17 && VAR != 12 && VAR != 15 && SQ + URING < NCH * 18) c.ur[SQ % URING] = c.uload_next();
    PNP_SLOT();
}
template <int K, int VAR, typename CT, typename DMA, int... P> __device__ __forceinline__ void chunk_steps(CT& c, DMA&& dma, std::integer_sequence<int, P...>) {
    if constexpr (CT::NG == 2) (step2<K, P, VAR>(c, dma), ...);
    else (step<K, P, VAR>(c, dma), ...);
}
// weight reloads of steps p0 .. p1 of chunk K
template <int K> constexpr int reloads_of(int p0, int p1) {
    int n = 0;
    for (int p = p0; p <= p1; ++p) n += (K * 18 + p + URING < NCH * 18) ? 1 : 0;
    return n;
}
// chunk K of a tile: MFMAs on V buffer K & 1, transform of chunk K + 1, DMA of chunk K + 2
template <int K, bool STAMP, int VAR, typename CT, typename DMA> __device__ __forceinline__ void chunk(CT& c, DMA&& dma, unsigned long long& t_wait) {
    if constexpr (CT::NG == 1) {                             // (two block rows: patch row 0 is read in step 0)
        patch_load<(K + 1) & 1, 0, 0>(c);
        patch_load<(K + 1) & 1, 0, 1>(c);
    }
    b_load<K & 1, 0>(c);
    PNP_SLOT();
    chunk_steps<K, VAR>(c, dma, std::make_integer_sequence<int, 18>{});
    unsigned long long ta = 0;
    if (STAMP) ta = __builtin_amdgcn_s_memtime();
    // this chunk's DMA pieces have landed: vector-memory operations leave the queue in issue order, and piece p was issued
    // in step p < PPW before that step's weight reload and behind every older reload, so only reloads are younger than
    // the last piece.  Two block rows: those of steps PPW - 1 .. 16 (step 17's is issued behind this wait).  One block
    // row: those of steps PPW - 1 .. 17; the count leaves out step PPW - 1 (one stricter than needed, never weaker).
    // The last chunk of a tile reloads nothing: see step()
    constexpr int PPW = CT::G::PPW, younger = CT::NG == 2 ? reloads_of<K>(PPW - 1, 16) : reloads_of<K>(PPW, 17);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(younger) : "memory");
    __syncthreads();
    if (STAMP) t_wait += __builtin_amdgcn_s_memtime() - ta;
}
template <bool STAMP, int VAR, typename CT, typename MK, int... K> __device__ __forceinline__ void all_chunks(CT& c, MK&& mk, unsigned long long& t_wait, std::integer_sequence<int, K...>) {
    (chunk<K, STAMP, VAR>(c, mk(std::integral_constant<int, K>{}), t_wait), ...);
}

// the first chunk of a workgroup's first tile, outside the pipeline
template <int VPL> __device__ __forceinline__ void transform0(const float* dsrc, float* vdst) {
    float t[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const float* row = dsrc + r * PC;                         // LDS column 4 tc of patch row r
        bt6(row[3], row[4], row[5], row[6], row[7], row[8], t[r]);
    }
#pragma unroll
    for (int x = 0; x < 6; ++x) {
        float v[6];
        bt6(t[0][x], t[1][x], t[2][x], t[3][x], t[4][x], t[5][x], v);
#pragma unroll
        for (int y = 0; y < 6; ++y) vdst[(y * 6 + x) * VPL] = v[y];
    }
}

// Last-layer fusion (FL): the DnCNN's 64 -> 1 output conv folded into the epilogue of the last middle layer.  Instead of its
// 64 channels, a 4 x 4 block leaves the 6 x 6 patch of output partials it feeds,
//     part[b][by][bx][py][px] = sum_c sum_(dy,dx) w_last[c][dy][dx] a[c][4 by + py + dy - 2][4 bx + px + dx - 2]
// restricted to the block's own activations (patch row / column 0 and 5 are the one-pixel spill-over into the neighbouring
// blocks); finish_last_layer (dncnn.hip) adds the up to four patches that cover a pixel.  36 floats per 16 pixels instead
// of 64 x 16.  The sums: within a lane (its 4 channels) in registers, across its wave's four channel groups by a
// reduce-scatter over lanes, across the four waves through LDS -- one fixed order per block, whatever the region form.
constexpr int FL_PATCH = 36;
constexpr int FL_BLK = 16 * FL_PATCH;                 // one block row of a region: 16 blocks x 36
template <int NG, bool FL> constexpr int fl_lds_floats() { return FL ? C * 9 + NG * 4 * FL_BLK : 0; }   // w_last + [NG][wave][576]

// STAMP: diagnostic build only (wino44_debug_clock): s_memtime / s_memrealtime around the tile loop, the chunk-end waits and
// the epilogue; the stamps go to their own buffer
template <bool LEAKY, int NG = 2, bool STAMP = false, int VAR = 0, bool FL = false>
__global__ __launch_bounds__(256, 1) void k_mid_wino44(const float* __restrict__ in, float* __restrict__ out,
                                                       const float4* __restrict__ upack, const float* __restrict__ bias,
                                                       int H, int W, int ntiles, float slope,
                                                       unsigned long long* __restrict__ stamps = nullptr, int tile0 = 0,
                                                       const float* __restrict__ wlast = nullptr, float* __restrict__ part = nullptr) {
    using G = Geo<NG>;
    constexpr int PLANE = G::PLANE, DBUF = G::DBUF, PPW = G::PPW, VPL = G::VPL, VBUF = G::VBUF;
    static_assert(!(FL && LEAKY), "the fused last layer is built for the ReLU net");
    __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS + fl_lds_floats<NG, FL>()];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // regions are numbered in units of 8 x 64 pixels from `tile0`, so that a launch of the one-row form can take over the units
    // a two-row launch left (the last, partly filled wave of workgroups: wino44_layer)
    const Regions<NG> region(H, W, tile0);

    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[16 * wv + 4 * (lane >> 4) + r];

    // transform item of this thread: block (g, tc), chunk channel 2 wv + j  (k-row wv, k-step j of the MFMA B operand)
    // (with one block row the upper half-wave repeats the lower half's items: same values to the same addresses)
    const int tc = lane & 15, j = (lane >> 4) & 1, g = NG == 2 ? lane >> 5 : 0;
    const int d_off = 4 * ((2 * wv + j) * (PLANE / 4) + g * PC + tc);               // 16-byte aligned
    const ptrdiff_t hw4 = (ptrdiff_t)4 * H * W, w4 = (ptrdiff_t)4 * W;
    const unsigned st_off = 4u * (unsigned)(4 * (lane >> 4) * H * W + 4 * tc);      // output: channel 4 (lane >> 4) of the wave's 16, column 4 tc
    // V item: [k-row wv][block tc][block row g][k-step j] -- the 64 lanes of a wave write 64 consecutive dwords per point
    const int v_off = NG == 2 ? wv * 64 + tc * 4 + g * 2 + j : wv * 32 + tc * 2 + j;

    // halo front end (wino44_common.h): this wave's DMA pieces, and the DMA state of tile t (t == ntiles: "none", zeros)
    unsigned pdesc[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) pdesc[i] = piece_desc<NG>(wv, i, lane, H, W);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;
    const size_t chunk_bytes = (size_t)KC * H * W * 4;
    auto tile_dma = [&](int t) {
        TileDma<NG> td;
        int b, ty0, tx0;
        region(t, b, ty0, tx0);
        td.base = (size_t)in + 4 * ((((size_t)b * C) * H + ty0 - 1) * (size_t)W + tx0 - 4);
        const unsigned bad = bad_mask<NG>(t, ntiles, ty0, tx0, H, W);
#pragma unroll
        for (int i = 0; i < PPW; ++i) td.voff[i] = piece_voff(pdesc[i], bad);
        return td;
    };

    float* const dbuf = lds;
    float* const vbuf = lds + 2 * DBUF;

    Ctx<NG> c;
    lds_f* const ldsp = (lds_f*)lds;
    c.dsrc[0] = ldsp + d_off;                     c.dsrc[1] = ldsp + DBUF + d_off;
    c.vdst[0] = ldsp + 2 * DBUF + v_off;          c.vdst[1] = ldsp + 2 * DBUF + VBUF + v_off;
    // (laundered: folded into the instructions' offsets, the buffers' constant bases push some pairs of a ds_write2st64_b32
    //  beyond its 8-bit offsets and the pair becomes two ds_write_b32)
    asm volatile("" : "+v"(c.vdst[0]), "+v"(c.vdst[1]));
    c.vsrc0[0] = ldsp + 2 * DBUF + 2 * NG * lane; c.vsrc0[1] = ldsp + 2 * DBUF + VBUF + 2 * NG * lane;
    // transformed weights: the same stream of NCH x 18 16-byte loads per lane for every tile, kept URING loads ahead
    const __attribute__((address_space(1))) char* const ubase = (const __attribute__((address_space(1))) char*)upack + (size_t)(wv * NCH * 18) * 1024;
    c.ucur = ubase;
    c.ulane = 16u * lane;

    const TileWalk tw_ = tile_walk(ntiles);
    int tile = tw_.first;
    const int limit = tw_.limit < ntiles ? tw_.limit : ntiles;
    float* const flw = lds + G::LDS_FLOATS;                // FL: w_last [64][9], then the cross-wave exchange [NG][4][576]
    float* const flx = flw + C * 9;
    if constexpr (FL)
        for (int i = tid; i < C * 9; i += 256) flw[i] = wlast[i];
    {
        const TileDma<NG> td0 = tile_dma(tile < limit ? tile : ntiles);
#pragma unroll
        for (int i = 0; i < PPW; ++i) dma_piece(td0, chunk_rsrc(td0, 0, chunk_bytes), lds0, wv, 0, i);
#pragma unroll
        for (int i = 0; i < PPW; ++i) dma_piece(td0, chunk_rsrc(td0, 1, chunk_bytes), lds0, wv, 1, i);
#pragma unroll
        for (int i = 0; i < URING; ++i) c.ur[i] = c.uload_next();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        transform0<VPL>(dbuf + d_off, vbuf + v_off);
        __syncthreads();
    }

    unsigned long long t0 = 0, r0 = 0, t_wait = 0, t_epi = 0;
    if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    for (; tile < limit; tile += tw_.step) {
        asm volatile("" : "+v"(c.ulane));                                        // the weight loads stay inside the tile loop
        int b, ty0, tx0;
        region(tile, b, ty0, tx0);
        const int ntile = tile + tw_.step < limit ? tile + tw_.step : ntiles;      // ntiles = "none": zeros

        const TileDma<NG> cur = tile_dma(tile), nxt = tile_dma(ntile);
        all_chunks<STAMP, VAR>(c, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            // chunk K + 2 (of this tile, or chunk 0 / 1 of the next) -> the d buffer chunk K was transformed from
            const TileDma<NG>& td = K + 2 < NCH ? cur : nxt;
            const i32x4 rs = chunk_rsrc(td, (K + 2) % NCH, chunk_bytes);
            return [&, rs](int piece) { dma_piece(td, rs, lds0, wv, K & 1, piece); };
        }, t_wait, std::make_integer_sequence<int, NCH>{});

        unsigned long long te = 0;
        if (STAMP) te = __builtin_amdgcn_s_memtime();
        asm volatile("; W44_EPILOGUE_BEGIN\n\ts_nop 15\n\ts_nop 7" ::: "memory");      // MFMA write -> VALU read distance
        // ... which only holds if no read of an accumulator is scheduled above it: to hipcc the MFMA results are ready where
        // the asm statements stand, and it hoists the epilogue's v_accvgpr_reads right behind them.  Every accumulator is
        // therefore re-defined here by an empty asm (ordered behind the wait states; no code).
#pragma unroll
        for (int g2 = 0; g2 < NG; ++g2)
#pragma unroll
            for (int xi = 0; xi < 36; xi += 4) {
                if (G::in_agpr(g2, xi)) asm volatile("" : "+a"(c.acc[g2][xi]), "+a"(c.acc[g2][xi + 1]), "+a"(c.acc[g2][xi + 2]), "+a"(c.acc[g2][xi + 3]));
                else asm volatile("" : "+v"(c.acc[g2][xi]), "+v"(c.acc[g2][xi + 1]), "+v"(c.acc[g2][xi + 2]), "+v"(c.acc[g2][xi + 3]));
            }
        // epilogue: Y = A^T M A, bias, ReLU; a lane holds block (g2, tc) of channels 16 wv + 4 (lane >> 4) + i.  Two
        // channels at a time on the packed-f32 ALU (the halves of an accumulator quad are register pairs), two columns /
        // rows per scheduling region so that at most two dozen accumulator copies are in flight; the bias enters through
        // M[1][1], whose weight is 1 in all sixteen outputs.
        // stores: scalar base (tile, wave, channel pair, row: scalar ALU) + the lane's 32-bit byte offset
        unsigned so = st_off;                 // (re-defined inside the loop: its zero-extension must sit next to the stores for
        asm volatile("" : "+v"(so));          //  instruction selection to fold it into the scalar-base addressing mode)
        __attribute__((address_space(1))) char* const ob = (__attribute__((address_space(1))) char*)out + 4 * ((((size_t)b * C + 16 * wv) * H + ty0) * (size_t)W + tx0);
        float q[FL_PATCH];                                      // FL: this lane's output patch of the current block, its 4 channels
#pragma unroll
        for (int blk = 0; blk < 2 * NG; ++blk) {
            {
                const int g2 = NG == 2 ? 1 - (blk >> 1) : 0, pi = blk & 1;   // block row 1 first: it frees the eight VGPR accumulator quads
                float wr[2][9];                                 // FL: w_last of channels 2 pi, 2 pi + 1 of the lane's four
                if constexpr (FL) {
                    if (pi == 0)
#pragma unroll
                        for (int i = 0; i < FL_PATCH; ++i) q[i] = 0.f;
                    const float* wc = flw + (16 * wv + 4 * (lane >> 4) + 2 * pi) * 9;
#pragma unroll
                    for (int t = 0; t < 9; ++t) { wr[0][t] = wc[t]; wr[1][t] = wc[9 + t]; }
                }
                // no weight load is in flight across the epilogue (a spilled in-flight load costs its whole latency); the
                // ring's first entries of the next tile go out before the last block
                if (blk == 2 * NG - 1) {
                    c.ucur = ubase;
#pragma unroll
                    for (int i = 0; i < URING; ++i) c.ur[i] = c.uload_next();
                    __builtin_amdgcn_sched_barrier(0);
                }
                const f32x2 bias2 = {bv[2 * pi], bv[2 * pi + 1]};
                // store cursor: one scalar register pair walked over the block's eight rows (re-defined through empty asms: left
                // alone, hipcc keeps all 32 store bases in scalar registers and spills them)
                __attribute__((address_space(1))) char* oc = ob + (ptrdiff_t)(2 * pi) * hw4 + (ptrdiff_t)(4 * g2) * w4;
                asm volatile("" : "+s"(oc));
                f32x2 s[6][4];                                  // s[x][r]: A^T along y of column x
#pragma unroll
                for (int x = 0; x < 6; ++x) {
                    f32x2 m[6];
#pragma unroll
                    for (int y = 0; y < 6; ++y) {
                        const f32x4 q = c.acc[g2][6 * y + x];
                        m[y] = pi ? f32x2{q.z, q.w} : f32x2{q.x, q.y};
                    }
                    if (x == 1) m[1] += bias2;
                    at6(m[0], m[1], m[2], m[3], m[4], m[5], s[x]);
                    if (x & 1) __builtin_amdgcn_sched_barrier(0);          // (two columns / rows per scheduling region: -0.35 % against one)
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    f32x2 y[4];
                    at6(s[0][r], s[1][r], s[2][r], s[3][r], s[4][r], s[5][r], y);
                    f32x4 v0, v1;
                    if (LEAKY) {
                        v0.x = fmaxf(y[0].x, slope * y[0].x); v0.y = fmaxf(y[1].x, slope * y[1].x);
                        v0.z = fmaxf(y[2].x, slope * y[2].x); v0.w = fmaxf(y[3].x, slope * y[3].x);
                        v1.x = fmaxf(y[0].y, slope * y[0].y); v1.y = fmaxf(y[1].y, slope * y[1].y);
                        v1.z = fmaxf(y[2].y, slope * y[2].y); v1.w = fmaxf(y[3].y, slope * y[3].y);
                    } else {
                        v0.x = fmaxf(y[0].x, 0.f); v0.y = fmaxf(y[1].x, 0.f); v0.z = fmaxf(y[2].x, 0.f); v0.w = fmaxf(y[3].x, 0.f);
                        v1.x = fmaxf(y[0].y, 0.f); v1.y = fmaxf(y[1].y, 0.f); v1.z = fmaxf(y[2].y, 0.f); v1.w = fmaxf(y[3].y, 0.f);
                    }
                    if constexpr (FL) {
                        // activation (r, k) of the block feeds patch position (r + 2 - dy, k + 2 - dx) through tap (dy, dx)
                        const float a0[4] = {v0.x, v0.y, v0.z, v0.w}, a1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    float& d = q[(r + 2 - dy) * 6 + k + 2 - dx];
                                    d = __builtin_fmaf(wr[0][dy * 3 + dx], a0[k], d);
                                    d = __builtin_fmaf(wr[1][dy * 3 + dx], a1[k], d);
                                }
                    } else {
                        *(__attribute__((address_space(1))) f32x4*)(oc + so) = v0;          // channel 2 pi, row 4 g2 + r
                        oc += hw4;
                        asm volatile("" : "+s"(oc));
                        *(__attribute__((address_space(1))) f32x4*)(oc + so) = v1;          // channel 2 pi + 1
                        oc += w4 - hw4;
                        asm volatile("" : "+s"(oc));
                    }
                    if (r & 1) __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (FL) {
                    if (pi == 1) {
                        // reduce-scatter over the four channel groups (lanes tc + 16 cg): lane keeps patch entries 9 cg .. 9 cg + 8
                        const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0;
                        float k1[18], k2[9];
#pragma unroll
                        for (int i = 0; i < 18; ++i) {
                            const float mine = h32 ? q[18 + i] : q[i], give = h32 ? q[i] : q[18 + i];
                            k1[i] = mine + __shfl_xor(give, 32);
                        }
#pragma unroll
                        for (int i = 0; i < 9; ++i) {
                            const float mine = h16 ? k1[9 + i] : k1[i], give = h16 ? k1[i] : k1[9 + i];
                            k2[i] = mine + __shfl_xor(give, 16);
                        }
                        float* const xd = flx + (g2 * 4 + wv) * FL_BLK + tc * FL_PATCH + 9 * (lane >> 4);
#pragma unroll
                        for (int i = 0; i < 9; ++i) xd[i] = k2[i];
                    }
                }
            }
        }
        if constexpr (FL) {
            // the four waves' patches of every block, summed in wave order; one region's NG x 16 patches are contiguous
            // per block row of `part` ([B][H/4][W/4][36])
            __syncthreads();
            float* const pb = part + (((size_t)b * (H / 4) + ty0 / 4) * (size_t)(W / 4) + tx0 / 4) * FL_PATCH;
            for (int e = tid; e < NG * FL_BLK; e += 256) {
                const int g2 = e >= FL_BLK ? 1 : 0, rem = e - g2 * FL_BLK;
                const float* xs = flx + g2 * 4 * FL_BLK + rem;
                pb[(size_t)g2 * (W / 4) * FL_PATCH + rem] = ((xs[0] + xs[FL_BLK]) + xs[2 * FL_BLK]) + xs[3 * FL_BLK];
            }
        }
        asm volatile("; W44_EPILOGUE_END" ::: "memory");
        if (STAMP) t_epi += __builtin_amdgcn_s_memtime() - te;
    }
    if (STAMP && tid == 0) {
        stamps[4 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t0;
        stamps[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - r0;
        stamps[4 * blockIdx.x + 2] = t_wait;
        stamps[4 * blockIdx.x + 3] = t_epi;
    }
}

}  // namespace w44

bool wino44_supports(int H, int W) { return H % 8 == 0 && W % w44::TC == 0; }

size_t wino44_layer_bytes() { return (size_t)4 * w44::NCH * 18 * 64 * 4 * sizeof(float); }

// w_mid [n_mid][64][64][3][3] (BN folded) -> upack[l][wv][chunk k][xi pair p][lane][e]:  xi = 2 p + (e >> 1), k-step j = e & 1,
// U_xi[cout = 16 wv + (lane & 15)][cin = 8 k + 2 (lane >> 4) + j],  U = G g G^T,  xi = 6 xi_y + xi_x
void wino44_pack(const float* w_mid, int n_mid, void* out_) {
    float* out = (float*)out_;
    for (int l = 0; l < n_mid; ++l)
        for (int wv = 0; wv < 4; ++wv)
            for (int k = 0; k < w44::NCH; ++k)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 2; ++j) {
                        const int cout = 16 * wv + (lane & 15), cin = w44::KC * k + 2 * (lane >> 4) + j;
                        const float* g = w_mid + (((size_t)l * w44::C + cout) * w44::C + cin) * 9;
                        float u[36];
                        w44c::filter_u(g, u);
                        for (int xi = 0; xi < 36; ++xi) {
                            const int p = xi >> 1, e = 2 * (xi & 1) + j;
                            out[((((size_t)(l * 4 + wv) * w44::NCH + k) * 18 + p) * 64 + lane) * 4 + e] = u[xi];
                        }
                    }
}

int wino44_layer(const ConvLayerArgs& a) {
    // 8 x 64 regions (72 accumulator quads per wave) in full waves of one region per CU; what is left -- a launch smaller than
    // the chip, or the last, partly filled wave -- goes through the 4 x 64 form, twice as many regions of half the work (one
    // 256 x 256 image: 256 regions instead of 128; three images: 256 + 256 instead of 384 in two waves).  Same bits either way.
    // force = 1 / 2 (test hook pnp_dncnn_debug_mid_layer only) takes one form for the whole layer.
    // part != nullptr: the fused last layer (ReLU only): `out` is not written, the output patches go to `part` (wino44.h).
    PNP_CHECK_ARG(a.part == nullptr || (a.slope == 0.f && a.wlast != nullptr), "the fused last layer needs ReLU and w_last");
    const float *in = a.in, *bias = a.bias, *wlast = a.wlast;
    float *out = a.out, *part = a.part;
    const int H = a.H, W = a.W, num_cu = a.num_cu, force = a.force_rows, batch = a.batch;
    const float slope = a.slope;
    const hipStream_t s = a.s;
    const int units = batch * (H / 8) * (W / w44::TC);
    int full = force == 1 ? 0 : force == 2 ? units : (units / num_cu) * num_cu;              // units done as 8 x 64 regions
    if (force == 0 && 2 * (units - full) > num_cu) full = units;      // (more than half a wave left: one more 8 x 64 wave is cheaper than two 4 x 64 waves)
    const float4* up = (const float4*)(a.w44_override ? a.w44_override : (const float*)a.w + a.layer * wino44_layer_bytes() / sizeof(float));
    if (full > 0) {
        const int grid = full < num_cu ? full : num_cu;
        if (part) w44::k_mid_wino44<false, 2, false, 0, true><<<grid, 256, 0, s>>>(in, out, up, bias, H, W, full, 0.f, nullptr, 0, wlast, part);
        else if (slope != 0.f) w44::k_mid_wino44<true, 2><<<grid, 256, 0, s>>>(in, out, up, bias, H, W, full, slope, nullptr, 0);
        else w44::k_mid_wino44<false, 2><<<grid, 256, 0, s>>>(in, out, up, bias, H, W, full, 0.f, nullptr, 0);
        PNP_CHECK_LAUNCH();
    }
    if (full < units) {
        const int n1 = 2 * (units - full), grid = n1 < num_cu ? n1 : num_cu;
        if (part) w44::k_mid_wino44<false, 1, false, 0, true><<<grid, 256, 0, s>>>(in, out, up, bias, H, W, n1, 0.f, nullptr, full, wlast, part);
        else if (slope != 0.f) w44::k_mid_wino44<true, 1><<<grid, 256, 0, s>>>(in, out, up, bias, H, W, n1, slope, nullptr, full);
        else w44::k_mid_wino44<false, 1><<<grid, 256, 0, s>>>(in, out, up, bias, H, W, n1, 0.f, nullptr, full);
        PNP_CHECK_LAUNCH();
    }
    return PNP_OK;
}

// per workgroup {shader cycles, 100 MHz ticks, cycles in the chunk-end waits + barriers, cycles in the epilogue} of the tile loop
int wino44_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& cycles, std::vector<double>& ticks) {
    const int ntiles = a.batch * (a.H / 8) * (a.W / w44::TC);
    const int grid = ntiles < a.num_cu ? ntiles : a.num_cu;
    const float *in = a.in, *bias = a.bias;
    float* out = a.out;
    const int H = a.H, W = a.W;
    const hipStream_t s = a.s;
    const float* upack_layer = (const float*)a.w + a.layer * wino44_layer_bytes() / sizeof(float);
    std::vector<unsigned long long> h;
    const int rc = read_stamps(s, grid, 4, [&](unsigned long long* stamps_dev) {
        for (int i = 0; i < reps - 1; ++i)
            w44::k_mid_wino44<false, 2><<<grid, 256, 0, s>>>(in, out, (const float4*)upack_layer, bias, H, W, ntiles, 0.f);
        const int var = getenv("PNP_W44_VAR") ? atoi(getenv("PNP_W44_VAR")) : 0;
        if (var == 0) w44::k_mid_wino44<false, 2, true><<<grid, 256, 0, s>>>(in, out, (const float4*)upack_layer, bias, H, W, ntiles, 0.f, stamps_dev);
#ifdef PNP_W44_ABLATIONS   // timing-only builds (wrong results): 10 = no transform
                           // arithmetic, 11 = no DMA, 12 = no weight reloads, 13 = no B reads, 14 = no transform LDS traffic, 15 = bare MFMAs
#define PNP_W44_ABL(V) else if (var == V) w44::k_mid_wino44<false, 2, true, V><<<grid, 256, 0, s>>>(in, out, (const float4*)upack_layer, bias, H, W, ntiles, 0.f, stamps_dev);
        PNP_W44_ABL(10) PNP_W44_ABL(11) PNP_W44_ABL(12) PNP_W44_ABL(13) PNP_W44_ABL(14) PNP_W44_ABL(15)
#undef PNP_W44_ABL
#endif
        else PNP_CHECK_ARG(false, "PNP_W44_VAR: this library was built without -DPNP_W44_ABLATIONS");
        PNP_CHECK_LAUNCH();
        return PNP_OK;
    }, h, cycles, ticks);
    if (rc != PNP_OK) return rc;
    if (getenv("PNP_DEBUG_STAMPS")) w44c::print_stamp_summary("k_mid_wino44", h, grid);
    return PNP_OK;
}

}  // namespace pnp

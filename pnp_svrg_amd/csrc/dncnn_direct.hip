// dncnn_direct.hip -- the 64 -> 64 channel 3x3 layer of the DnCNN prox (reference denoisers/DeepDenoisers/model/models.py:13-17:
// conv + BatchNorm + ReLU, BN folded into weights + bias by the caller) as an implicit GEMM on the f32 matrix cores
// (v_mfma_f32_16x16x4f32: exact fp32, the reference network's own precision), in two forms: k_mid, the direct form (conv
// mode 0), and k_mid_wino, Winograd F(2,3) along x (conv mode 1).
//
// k_mid design (one workgroup = 4 waves = one wave per SIMD, persistent over output tiles):
//   * output tile: 8 rows x 32 columns x 64 channels.  D[cout][pixel] = sum_k W[cout][k] X[k][pixel]
//     with K = 9 taps x 64 channels = 576: A operand = weights (rows = cout), B operand =
//     activations (columns = 16 adjacent pixels of one row) so that every accumulator register
//     holds 16 adjacent pixels of one channel -> coalesced stores into NCHW.
//   * WEIGHT-STATIONARY: wave wv owns couts [16wv, 16wv+16) of the whole tile.  Its 16 x 576
//     weight slice sits in 144 VGPRs for the life of the kernel -- weights are fetched from
//     L2 once per launch, never per tile, and never go through LDS.
//   * activations: the (8+2) x (32+2) halo tile of 32 input channels (one K-half) lives in LDS as
//     channel planes [cin][10][40] -> the B operand of an MFMA is ONE conflict-free ds_read_b32
//     (16 adjacent pixels per k-row).  Two K-halves = two LDS buffers = a natural double buffer:
//     while the MFMAs chew on one half, the next half (or the next tile's first half) is in flight
//     global -> LDS, by LDS-DMA.
//   * per wave and K-half: 1152 MFMAs vs 480 ds_read_b32 + 13 DMA pieces: the matrix pipe is the
//     only busy resource by a wide margin.
#include "direct.h"
#include "tilewalk.h"
#include <cstdlib>

namespace pnp {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int C = 64;             // feature channels
constexpr int TR = 8, TC = 32;    // output tile rows / cols
constexpr int PR = TR + 2;        // halo rows
constexpr int PC = 40;            // halo row stride in LDS: columns [tx0-4, tx0+36) = ten 16-byte chunks,
                                  // so every global->LDS piece is an aligned dwordx4 (the 3x3 halo needs
                                  // only tx0-1 .. tx0+32; the 6 extra floats buy 4x fewer DMA instructions)
constexpr int XOFF = 3;           // LDS column of image column tx0-1
constexpr int PLANE = PR * PC;    // 400 floats per channel; 400 % 32 == 16 -> the 4 k-rows of a B operand
                                  // (lanes 0-15 / 16-31 of a half-wave) fall on disjoint LDS banks
constexpr int HALF_C = 32;        // channels per K-half
constexpr int HALF_PAYLOAD = HALF_C * PLANE;          // 12800 floats = 50 KB of halo tile per K-half
constexpr int HALF_LDS = 52 * 256;                    // LDS buffer rounded up to 13 DMA pieces per wave (52 KB):
                                                      // every wave issues the same, branch-free piece sequence
constexpr int CHUNKS = HALF_PAYLOAD / 4;              // 3200 16-byte chunks = 50 wave-pieces per half
constexpr int KSTEPS_HALF = 9 * (HALF_C / 4);         // 72 MFMA K-steps (K=4 each) per half
constexpr int MT = 16;                                // 16-pixel M-tiles per output tile (8 rows x 2)

// Stage one K-half of an input halo tile global (NCHW) -> LDS by LDS-DMA (global_load_lds_dwordx4):
// no staging registers, no ds_write.  The LDS image [cin][10][40] is linear in the chunk index
// q = cin*100 + row*10 + chunk, so one wave-instruction (64 lanes x 16 B) fills 64 consecutive
// chunks; the SOURCE address is per lane; chunks outside the image read a zero line instead.
__device__ __forceinline__ void dma_piece(int pc, const float* __restrict__ in, const float* __restrict__ zeros,
                                          float* ldsbuf, int H, int W, int b, int ty0, int tx0, int half, int lane,
                                          bool valid_tile) {
    const int q = pc * 64 + lane;
    const int cin = q / 100, r = q - cin * 100;
    const int ry = r / 10, cx = r - ry * 10;
    const int y = ty0 - 1 + ry, x = tx0 - 4 + 4 * cx;
    const float* src = zeros;
    if (valid_tile && y >= 0 && y < H && x >= 0 && x < W)
        src = in + (((size_t)b * C + half * HALF_C + cin) * H + y) * W + x;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)(ldsbuf + pc * 256), 16, 0, 0);
}

constexpr int PIECES = CHUNKS / 64;                   // 50 wave-pieces per half
constexpr int PIECES_PER_WAVE = (PIECES + 3) / 4;     // 13 (the last one only for waves 0,1)

__device__ __forceinline__ void dma_half(const float* __restrict__ in, const float* __restrict__ zeros,
                                         float* ldsbuf, int H, int W, int b, int ty0, int tx0, int half, int tid,
                                         bool valid_tile) {
    const int wv = tid >> 6, lane = tid & 63;
#pragma unroll 1
    for (int pc = wv; pc < PIECES; pc += 4) dma_piece(pc, in, zeros, ldsbuf, H, W, b, ty0, tx0, half, lane, valid_tile);
}

// STAMP / ABL: diagnostic builds only (pnp_dncnn_debug_clock): s_memtime / s_memrealtime around the tile
// loop and its phases; ABL bit 0 replaces the LDS reads by register values, bit 1 drops the DMA.
// LEAKY: the activation is LeakyReLU(slope) instead of ReLU (the MMO network, reference denoisers/MMODenoise.py:84).
template <bool RELU, bool STAMP = false, int ABL = 0, bool LEAKY = false>
__global__ __launch_bounds__(256, 1) void k_mid(const float* __restrict__ in, float* __restrict__ out,
                                                const float* __restrict__ wpack, const float* __restrict__ bias,
                                                const float* __restrict__ zeros, int H, int W, int ntiles,
                                                unsigned long long* __restrict__ stamps = nullptr, float slope = 0.f) {
    __shared__ float lds[2 * HALF_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = W / TC, tiles_per_img = tiles_x * (H / TR);

    // weight slice of this wave (16 couts x 576): wreg[s] = W'[16wv + (lane&15)][k = 4s + (lane>>4)]
    float wreg[2 * KSTEPS_HALF];
#pragma unroll
    for (int s = 0; s < 2 * KSTEPS_HALF; ++s) wreg[s] = wpack[((size_t)wv * 2 * KSTEPS_HALF + s) * 64 + lane];
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[16 * wv + 4 * (lane >> 4) + r];

    const int lbase = (lane >> 4) * PLANE + (lane & 15) + XOFF;     // lane part of the B-operand LDS address
    int loff[4];                                               // lane part of the output offsets (per register)
#pragma unroll
    for (int r = 0; r < 4; ++r) loff[r] = (16 * wv + 4 * (lane >> 4) + r) * H * W + (lane & 15);

    // Per-lane descriptors of this wave's DMA pieces (tile independent): element offset of the chunk relative
    // to the tile origin ((b*64 + half*32)*H + ty0 - 1)*W + tx0 - 4, and its (halo row, 4*chunk column).
    int poff[PIECES_PER_WAVE], pry[PIECES_PER_WAVE], pcx4[PIECES_PER_WAVE];
#pragma unroll
    for (int i = 0; i < PIECES_PER_WAVE; ++i) {
        const int q = (wv + 4 * i) * 64 + lane;
        const int cin = q / 100, r = q - cin * 100;
        pry[i] = r / 10;
        pcx4[i] = 4 * (r - pry[i] * 10);
        poff[i] = (cin * H + pry[i]) * W + pcx4[i];
    }

    const TileWalk tw_ = tile_walk(ntiles);
    int tile = tw_.first;
    {
        const int b = tile / tiles_per_img, t2 = tile - b * tiles_per_img;
        dma_half(in, zeros, lds, H, W, b, (t2 / tiles_x) * TR, (t2 % tiles_x) * TC, 0, tid, tile < tw_.limit);
    }
    __syncthreads();                                        // (drains the DMA: vmcnt(0) + barrier)
    unsigned long long t0 = 0, r0 = 0, acc_compute = 0, acc_barrier = 0, acc_epi = 0, tp = 0;
    if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }

    for (; tile < tw_.limit; tile += tw_.step) {
        const int b = tile / tiles_per_img, t2 = tile - b * tiles_per_img;
        const int ty0 = (t2 / tiles_x) * TR, tx0 = (t2 % tiles_x) * TC;
        f32x4 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
        for (int half = 0; half < 2; ++half) {
            // prefetch target: the other K-half of this tile, or the first K-half of the next tile
            float* nbuf = lds + (half ^ 1) * HALF_LDS;
            const int nt = tile + tw_.step;
            const int nb = half == 0 ? b : nt / tiles_per_img;
            const int n2 = nt - nb * tiles_per_img;
            const int nty0 = half == 0 ? ty0 : (n2 / tiles_x) * TR, ntx0 = half == 0 ? tx0 : (n2 % tiles_x) * TC;
            const bool nvalid = half == 0 ? true : nt < tw_.limit;
            const float* nsrc0 = in + (((size_t)nb * C + (half ^ 1) * HALF_C) * H + nty0 - 1) * (size_t)W + ntx0 - 4;

            // keep the buffer base in a register of its own: every B-operand address is then base +
            // a 16-bit immediate (< 48 KB) instead of one v_add per LDS read
            int xb_off = half * HALF_LDS + lbase;
            asm volatile("" : "+v"(xb_off));
            const float* xb = lds + xb_off;
            if (STAMP) tp = __builtin_amdgcn_s_memtime();
            // B operands of one (channel quad c4, dx) group: the 10 halo rows x 2 column halves; each
            // value feeds up to three taps (dy): 20 LDS reads per 48 MFMAs.  Software pipeline: the reads
            // of group g+1 and one DMA piece of the next buffer are issued underneath the MFMAs of group g.
            float xr[2][PR][2];
            constexpr int NG = (HALF_C / 4) * 3;           // 24 groups per half
#pragma unroll
            for (int ry = 0; ry < PR; ++ry)
#pragma unroll
                for (int h = 0; h < 2; ++h) xr[0][ry][h] = (ABL & 1) ? (float)(lane + ry + h) : xb[ry * PC + 16 * h];
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int c4 = g / 3, dx = g % 3;
                if (g + 1 < NG) {
                    const int c4n = (g + 1) / 3, dxn = (g + 1) % 3;
#pragma unroll
                    for (int ry = 0; ry < PR; ++ry)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            xr[(g + 1) & 1][ry][h] = (ABL & 1) ? xr[g & 1][ry][h] : xb[(4 * c4n) * PLANE + ry * PC + 16 * h + dxn];
                }
                if (g < PIECES_PER_WAVE && !(ABL & 2)) {
                    // branch-free and identical in every wave (a branch here would split the MFMA scheduling
                    // region): pieces 50/51 and the pieces of a non-existent next tile just move zeros
                    const int pc = wv + 4 * g;
                    const int y = nty0 - 1 + pry[g], x = ntx0 - 4 + pcx4[g];
                    const bool ok = nvalid & (pc < PIECES) & ((unsigned)y < (unsigned)H) & ((unsigned)x < (unsigned)W);
                    const float* src = ok ? nsrc0 + poff[g] : zeros;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(nbuf + pc * 256), 16, 0, 0);
                }
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int s = half * KSTEPS_HALF + (dy * 3 + dx) * (HALF_C / 4) + c4;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[s], xr[g & 1][(m >> 1) + dy][m & 1], acc[m], 0, 0, 0);
                }
                // interleave: 2 MFMA, then 1 LDS read (ds_read2 pairs count once), ... rest MFMA
#pragma unroll
                for (int i = 0; i < 20; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (STAMP) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc_compute += t - tp; tp = t; }
            __syncthreads();                                // next buffer landed (vmcnt(0)) + everyone done reading
            if (STAMP) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc_barrier += t - tp; tp = t; }
        }

        // epilogue: bias (+ReLU); each accumulator register = 16 adjacent pixels of one channel.
        // 32-bit in-image offsets off a per-tile scalar base: one v_add per store, no 64-bit multiplies.
        // (The transposed operand order -- 4 adjacent pixels per lane, one float4 store per M-tile -- was
        // measured SLOWER: each store instruction then touches 16 channel planes instead of 4.)
        float* ob = out + (size_t)b * C * H * W + ty0 * W + tx0;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int so = (m >> 1) * W + 16 * (m & 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[m][r] + bv[r];
                if (RELU) v = v > 0.f ? v : (LEAKY ? slope * v : 0.f);
                ob[loff[r] + so] = v;
            }
        }
        if (STAMP) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc_epi += t - tp; }
    }
    if (STAMP && tid == 0) {
        stamps[5 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t0;
        stamps[5 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - r0;
        stamps[5 * blockIdx.x + 2] = acc_compute;
        stamps[5 * blockIdx.x + 3] = acc_barrier;
        stamps[5 * blockIdx.x + 4] = acc_epi;
    }
}

// ------------------------------------------------------------------------------- Winograd F(2,3) variant
// Same tile / LDS image / DMA pipeline as k_mid, but the 3 horizontal taps go through the 1-D Winograd
// minimal-filtering transform F(2,3): per output PAIR (x, x+1) and input row,
//     V = B^T d  (d = inputs x-1 .. x+2):  V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3
//     U = G g    (g = the 3 horizontal weights): U0 = g0, U1 = (g0+g1+g2)/2, U2 = (g0-g1+g2)/2, U3 = g2
//     m_xi = sum_{dy,cin} U_xi V_xi ;   y(x) = m0 + m1 + m2 ,  y(x+1) = m1 - m2 - m3
// i.e. 4 x 3 x 64 multiply-adds per output pair instead of 2 x 9 x 64: 2/3 of the matrix-core work of the
// direct form for the same (exact-arithmetic) result; fp32 throughout, rounding differs from the fmaf chain
// at the 1e-7 level.  An M-tile is the 16 pixel pairs of one 32-pixel output row; a wave keeps
// 8 rows x 4 xi accumulators (128 regs) and its 4 x 3 x 16 = 192 transformed weights in registers.
// The B-operand transform (4 LDS values -> 4 V values, 4 VALU ops) feeds up to 12 MFMAs.
constexpr int WINO_U = 2 * (HALF_C / 4) * 3 * 4;      // 192 transformed-weight registers per wave
struct __attribute__((packed, aligned(4))) f2u { float a, b; };   // 4-byte-aligned float pair
typedef float f32x2v __attribute__((ext_vector_type(2)));

// The raw Winograd inputs of one group -- 5 halo rows x (d0,d1),(d2,d3) -- as ten hand-issued ds_read2_b32 off ONE
// base register with immediate offsets (row stride PC = 40 dwords).  hipcc pairs these loads as (d0,d3),(d1,d2)
// with a second base register and an extra v_add per row, and every VALU instruction here costs matrix-pipe issue.
// The results are asynchronous: the caller waits lgkmcnt(0) (wino_lds_wait) before the first use.
__device__ __forceinline__ void wino_lds_load(f32x2v (&dd)[5][2], unsigned lds_byte_addr) {
    f32x2v r0, r1, r2, r3, r4, r5, r6, r7, r8, r9;
    asm volatile(
        "ds_read2_b32 %0, %10 offset0:0 offset1:1\n"
        "ds_read2_b32 %1, %10 offset0:2 offset1:3\n"
        "ds_read2_b32 %2, %10 offset0:40 offset1:41\n"
        "ds_read2_b32 %3, %10 offset0:42 offset1:43\n"
        "ds_read2_b32 %4, %10 offset0:80 offset1:81\n"
        "ds_read2_b32 %5, %10 offset0:82 offset1:83\n"
        "ds_read2_b32 %6, %10 offset0:120 offset1:121\n"
        "ds_read2_b32 %7, %10 offset0:122 offset1:123\n"
        "ds_read2_b32 %8, %10 offset0:160 offset1:161\n"
        "ds_read2_b32 %9, %10 offset0:162 offset1:163\n"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7), "=&v"(r8), "=&v"(r9)
        : "v"(lds_byte_addr)
        : "memory");
    dd[0][0] = r0; dd[0][1] = r1; dd[1][0] = r2; dd[1][1] = r3; dd[2][0] = r4; dd[2][1] = r5;
    dd[3][0] = r6; dd[3][1] = r7; dd[4][0] = r8; dd[4][1] = r9;
}
// The wait takes the ten register pairs as in/out operands, so every consumer is data-dependent on it and no pass
// can move a use of the (still in flight) load results above the s_waitcnt.
// B^T d of one halo row as two packed-f32 adds: (d0-d2, -d1-d2) and (d1-d2, d1-d3).  The middle two components are
// the NEGATED textbook ones (d1+d2, d2-d1); the inverse transform in the epilogue flips their signs back.  hipcc
// lowers the first shuffle+negate to movs + two adds, so both are spelled out.  NO wait states inside: the caller
// must put >= 2 instructions between this and the first MFMA that reads the results.
__device__ __forceinline__ void wino_bt(f32x2v& v01, f32x2v& v23, f32x2v A, f32x2v Bq) {
    asm volatile("v_pk_add_f32 %0, %2, %3 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,1]\n\t"
                 "v_pk_add_f32 %1, %2, %3 op_sel:[1,0] neg_lo:[0,1] neg_hi:[0,1]"
                 : "=&v"(v01), "=&v"(v23) : "v"(A), "v"(Bq));
}
// The Winograd kernel's MFMAs are hand-issued so that the REGISTER FILES are split the other way round from what
// hipcc picks: accumulators in VGPRs (the epilogue's VALU reads them in place), the 192 tile-invariant transformed
// weights in AGPRs (gfx90a+ MFMAs read SrcA from either file).  hipcc keeps accumulators in AGPRs, copies ~60
// weights through v_accvgpr_read every tile and reads all 128 accumulators back for the epilogue.  The first MFMA
// of an accumulator in a tile uses the constant-zero SrcC form, so accumulators are never cleared.
// Hazards are the caller's: >= 2 instructions between a VALU write of `v` and the MFMA, and wait states between the
// last MFMA and a VALU read of an accumulator (the hazard recognizer does not look inside inline asm).
__device__ __forceinline__ void mfma_wa(f32x4& acc, float w_agpr, float v) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "a"(w_agpr), "v"(v));
}
__device__ __forceinline__ void mfma_wa_first(f32x4& acc, float w_agpr, float v) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=&v"(acc) : "a"(w_agpr), "v"(v));
}
__device__ __forceinline__ void wino_lds_wait(f32x2v (&dd)[5][2]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(dd[0][0]), "+v"(dd[0][1]), "+v"(dd[1][0]), "+v"(dd[1][1]), "+v"(dd[2][0]), "+v"(dd[2][1]),
                   "+v"(dd[3][0]), "+v"(dd[3][1]), "+v"(dd[4][0]), "+v"(dd[4][1])
                 :: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
static_assert(PC == 40, "wino_lds_load hard-codes the 40-dword LDS row stride");

template <bool RELU, bool STAMP = false, bool LEAKY = false>
__global__ __launch_bounds__(256, 1) void k_mid_wino(const float* __restrict__ in, float* __restrict__ out,
                                                     const float* __restrict__ upack, const float* __restrict__ bias,
                                                     const float* __restrict__ zeros, int H, int W, int ntiles,
                                                     unsigned long long* __restrict__ stamps = nullptr, float slope = 0.f) {
    __shared__ float lds[2 * HALF_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = W / TC, tiles_per_img = tiles_x * (H / TR);

    // ureg[((half*8 + c4)*3 + dy)*4 + xi] = U_xi[cout = 16wv + (lane&15)][cin = 32half + 4c4 + (lane>>4)][dy]
    float ureg[WINO_U];
#pragma unroll
    for (int s = 0; s < WINO_U; ++s) ureg[s] = upack[((size_t)wv * WINO_U + s) * 64 + lane];
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = bias[16 * wv + 4 * (lane >> 4) + r];

    // lane (k-row kq = lane>>4, pair j = lane&15) reads d0..d3 at LDS columns XOFF + 2j + {0,1,2,3}
    const int lbase = (lane >> 4) * PLANE + 2 * (lane & 15) + XOFF;
    int loff[4];                                               // output offsets: pixel pair 2j of channel ...
#pragma unroll
    for (int r = 0; r < 4; ++r) loff[r] = (16 * wv + 4 * (lane >> 4) + r) * H * W + 2 * (lane & 15);

    // DMA piece descriptors, ONE register each: bits 0..27 = element offset of the lane's 16-byte chunk inside the
    // half's 32 channel planes, bits 28..31 = which image edge would put the chunk outside (top row of the halo,
    // bottom row, left chunk, right chunk).  A tile's own edge mask (scalar) then decides validity with one AND.
    unsigned pdesc[PIECES_PER_WAVE];
#pragma unroll
    for (int i = 0; i < PIECES_PER_WAVE; ++i) {
        const int q = (wv + 4 * i) * 64 + lane;
        const int cin = q / 100, r = q - cin * 100;
        const int ry = r / 10, cx4 = 4 * (r - ry * 10);
        const unsigned edge = (ry == 0 ? 1u : 0u) | (ry == TR + 1 ? 2u : 0u) | (cx4 == 0 ? 4u : 0u) | (cx4 == TC + 4 ? 8u : 0u);
        pdesc[i] = (unsigned)((cin * H + ry) * W + cx4) | (edge << 28);
    }

    const TileWalk tw_ = tile_walk(ntiles);
    int tile = tw_.first;
    {
        const int b = tile / tiles_per_img, t2 = tile - b * tiles_per_img;
        dma_half(in, zeros, lds, H, W, b, (t2 / tiles_x) * TR, (t2 % tiles_x) * TC, 0, tid, tile < tw_.limit);
    }
    __syncthreads();
    unsigned long long t0 = 0, r0 = 0, acc_compute = 0, acc_barrier = 0, acc_epi = 0, tp = 0;
    if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }

    for (; tile < tw_.limit; tile += tw_.step) {
        const int b = tile / tiles_per_img, t2 = tile - b * tiles_per_img;
        const int ty0 = (t2 / tiles_x) * TR, tx0 = (t2 % tiles_x) * TC;
        f32x4 acc[TR][4];                                       // written first by mfma_wa_first (half 0, channel quad 0, dy 0)

#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float* nbuf = lds + (half ^ 1) * HALF_LDS;
            const int nt = tile + tw_.step;
            const int nb = half == 0 ? b : nt / tiles_per_img;
            const int n2 = nt - nb * tiles_per_img;
            const int nty0 = half == 0 ? ty0 : (n2 / tiles_x) * TR, ntx0 = half == 0 ? tx0 : (n2 % tiles_x) * TC;
            const bool nvalid = half == 0 ? true : nt < tw_.limit;
            const float* nsrc0 = in + (((size_t)nb * C + (half ^ 1) * HALF_C) * H + nty0 - 1) * (size_t)W + ntx0 - 4;
            const unsigned nedge = ((nty0 == 0 ? 1u : 0u) | (nty0 + TR == H ? 2u : 0u) | (ntx0 == 0 ? 4u : 0u) | (ntx0 + TC == W ? 8u : 0u)) << 28;

            int xb_off = half * HALF_LDS + lbase;
            asm volatile("" : "+v"(xb_off));
            if (STAMP) tp = __builtin_amdgcn_s_memtime();

            // group = (channel quad c4, block of 5 halo rows): 10 ds_read2 + 20 transform ops + 48 MFMAs
            constexpr int NG = (HALF_C / 4) * 2;               // 16 groups per half
            f32x2v d[2][5][2];
            const unsigned xb_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds + 4u * (unsigned)xb_off;
            wino_lds_load(d[0], xb_addr);
            // All non-MFMA work of a group -- retire the group's LDS reads, issue the next group's, one DMA piece, the ten
            // packed adds of B^T d for the group's five halo rows -- is issued as ONE block in front of the group's 48
            // MFMAs.  On gfx950 every excursion from the MFMA stream to the vector ALU and back costs ~10 cycles on top
            // of ~4.3 per instruction (tools/microbench/mfma_f32_valu.hip: one v_pk_add_f32 between two fp32 MFMAs takes
            // them from 32.3 to 46.8 cycles), so the number of excursions counts, not only the instruction count.  It
            // also puts >= 2 instructions between every transform and the MFMA that reads it (VALU -> MFMA wait
            // states; the hazard recognizer does not see inside the asm).
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int c4 = g / 2, rb = g % 2;
                wino_lds_wait(d[g & 1]);                        // issued a whole group ago (or just above for g = 0)
                if (g + 1 < NG) {
                    const int c4n = (g + 1) / 2, rbn = (g + 1) % 2;
                    wino_lds_load(d[(g + 1) & 1], xb_addr + 4u * ((4 * c4n) * PLANE + (5 * rbn) * PC));
                }
                if (g < PIECES_PER_WAVE) {
                    const int pc = wv + 4 * g;
                    const bool ok = (nvalid & (pc < PIECES)) & ((pdesc[g] & nedge) == 0u);
                    const float* src = ok ? nsrc0 + (pdesc[g] & 0x0FFFFFFFu) : zeros;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(nbuf + pc * 256), 16, 0, 0);
                }
                f32x2v v01[5], v23[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) wino_bt(v01[i], v23[i], d[g & 1][i][0], d[g & 1][i][1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int ry = 5 * rb + i;
                    const float V[4] = {v01[i].x, v01[i].y, v23[i].x, v23[i].y};
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const int r = ry - dy;
                        if (r >= 0 && r < TR) {
#pragma unroll
                            for (int xi = 0; xi < 4; ++xi) {
                                const float wgt = ureg[((half * (HALF_C / 4) + c4) * 3 + dy) * 4 + xi];
                                if (half == 0 && c4 == 0 && dy == 0) mfma_wa_first(acc[r][xi], wgt, V[xi]);
                                else mfma_wa(acc[r][xi], wgt, V[xi]);
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (STAMP) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc_compute += t - tp; tp = t; }
            __syncthreads();
            if (STAMP) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc_barrier += t - tp; tp = t; }
        }

        // epilogue: inverse transform, bias (+ReLU); a lane holds pixel pair (2j, 2j+1) of 4 channels per row
        // (the barrier above sits between the last MFMA and these VALU reads; the explicit wait states make the
        // MFMA-write -> VALU-read distance independent of what the barrier costs)
        asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
        float* ob = out + (size_t)b * C * H * W + ty0 * W + tx0;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float m0 = acc[r][0][q], m1 = acc[r][1][q], m2 = acc[r][2][q], m3 = acc[r][3][q];
                float2 v;
                v.x = (m0 - m1 - m2) + bv[q];                   // m1, m2 carry the flipped signs of the packed transform
                v.y = (m2 - m1 - m3) + bv[q];
                if (RELU) { v.x = v.x > 0.f ? v.x : (LEAKY ? slope * v.x : 0.f); v.y = v.y > 0.f ? v.y : (LEAKY ? slope * v.y : 0.f); }
                *reinterpret_cast<float2*>(ob + loff[q] + r * W) = v;
            }
        }
        if (STAMP) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc_epi += t - tp; }
    }
    if (STAMP && tid == 0) {
        stamps[5 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t0;
        stamps[5 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - r0;
        stamps[5 * blockIdx.x + 2] = acc_compute;
        stamps[5 * blockIdx.x + 3] = acc_barrier;
        stamps[5 * blockIdx.x + 4] = acc_epi;
    }
}

// ------------------------------------------------------------------------------- host side
bool direct_supports(int H, int W) { return H % TR == 0 && W % TC == 0; }

size_t direct_layer_bytes() { return (size_t)4 * 2 * KSTEPS_HALF * 64 * sizeof(float); }
size_t wino23_layer_bytes() { return (size_t)4 * WINO_U * 64 * sizeof(float); }

// wpack[l][wv][s][lane] = W[l][cout = 16wv + (lane&15)][cin][tap], k-step s = half*72 + tap*8 + c4, cin = 32*half + 4*c4 + (lane>>4)
void direct_pack(const float* w_mid, int n_mid, void* out) {
    float* pack = (float*)out;
    for (int l = 0; l < n_mid; ++l)
        for (int wv = 0; wv < 4; ++wv)
            for (int s = 0; s < 2 * KSTEPS_HALF; ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int half = s / KSTEPS_HALF, rs = s % KSTEPS_HALF, tap = rs / (HALF_C / 4), c4 = rs % (HALF_C / 4);
                    const int cout = 16 * wv + (lane & 15), cin = HALF_C * half + 4 * c4 + (lane >> 4);
                    pack[(((size_t)l * 4 + wv) * 2 * KSTEPS_HALF + s) * 64 + lane] =
                        w_mid[(((size_t)l * C + cout) * C + cin) * 9 + tap];
                }
}

// Winograd F(2,3)-transformed weights (along dx): upack[l][wv][s][lane], s = ((half*8 + c4)*3 + dy)*4 + xi
void wino23_pack(const float* w_mid, int n_mid, void* out) {
    float* upk = (float*)out;
    for (int l = 0; l < n_mid; ++l)
        for (int wv = 0; wv < 4; ++wv)
            for (int s = 0; s < WINO_U; ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int xi = s % 4, dy = (s / 4) % 3, c4 = (s / 12) % (HALF_C / 4), half = s / (12 * (HALF_C / 4));
                    const int cout = 16 * wv + (lane & 15), cin = HALF_C * half + 4 * c4 + (lane >> 4);
                    const float* g = w_mid + (((size_t)l * C + cout) * C + cin) * 9 + dy * 3;
                    const double g0 = g[0], g1 = g[1], g2 = g[2];
                    const double u = xi == 0 ? g0 : xi == 1 ? 0.5 * (g0 + g1 + g2) : xi == 2 ? 0.5 * (g0 - g1 + g2) : g2;
                    upk[(((size_t)l * 4 + wv) * WINO_U + s) * 64 + lane] = (float)u;
                }
}

// the ReLU / LeakyReLU builds of k_mid (wino = false) and k_mid_wino (wino = true) on one layer; stamps != nullptr: the
// diagnostic build (ReLU), abl 2 = k_mid without its DMA
static void launch(const ConvLayerArgs& a, bool wino, unsigned long long* stamps = nullptr, int abl = 0) {
    const int ntiles = a.batch * (a.H / TR) * (a.W / TC), grid = ntiles < a.num_cu ? ntiles : a.num_cu;
    const float* w = (const float*)a.w + (size_t)a.layer * (wino ? wino23_layer_bytes() : direct_layer_bytes()) / sizeof(float);
    const bool leaky = a.slope != 0.f && !stamps;
    if (wino && stamps) k_mid_wino<true, true><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles, stamps);
    else if (wino && leaky) k_mid_wino<true, false, true><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles, nullptr, a.slope);
    else if (wino) k_mid_wino<true><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles);
    else if (stamps && abl == 2) k_mid<true, true, 2><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles, stamps);
    else if (stamps) k_mid<true, true><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles, stamps);
    else if (leaky) k_mid<true, false, 0, true><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles, nullptr, a.slope);
    else k_mid<true><<<grid, 256, 0, a.s>>>(a.in, a.out, w, a.bias, a.zeros, a.H, a.W, ntiles);
}

static int layer(const ConvLayerArgs& a, bool wino) {
    if (const int rc = check_plain_conv(a)) return rc;
    launch(a, wino);
    PNP_CHECK_LAUNCH();
    return PNP_OK;
}
int direct_layer(const ConvLayerArgs& a) { return layer(a, false); }
int wino23_layer(const ConvLayerArgs& a) { return layer(a, true); }

// per workgroup {shader cycles, 100 MHz ticks, cycles in the MFMA phases, in the barriers, in the epilogue} of the ReLU build
static int debug_clock(const ConvLayerArgs& a, bool wino, int reps, std::vector<double>& cycles, std::vector<double>& ticks) {
    const int ntiles = a.batch * (a.H / TR) * (a.W / TC), grid = ntiles < a.num_cu ? ntiles : a.num_cu;
    std::vector<unsigned long long> h;
    const int rc = read_stamps(a.s, grid, 5, [&](unsigned long long* d) {
        ConvLayerArgs relu = a;
        relu.slope = 0.f;
        for (int i = 0; i < reps - 1; ++i) launch(relu, wino);
        launch(a, wino, d, getenv("PNP_DEBUG_ABL") ? atoi(getenv("PNP_DEBUG_ABL")) : 0);
        return PNP_OK;
    }, h, cycles, ticks);
    if (rc != PNP_OK) return rc;
    if (getenv("PNP_DEBUG_STAMPS")) {
        double c = 0, b = 0, ep = 0;
        for (int i = 0; i < grid; ++i) { c += h[5 * i + 2]; b += h[5 * i + 3]; ep += h[5 * i + 4]; }
        fprintf(stderr, "[k_mid stamps] mean cycles per WG: compute %.0f  barrier %.0f  epilogue %.0f\n", c / grid, b / grid, ep / grid);
    }
    return PNP_OK;
}
int direct_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& c, std::vector<double>& t) { return debug_clock(a, false, reps, c, t); }
int wino23_debug_clock(const ConvLayerArgs& a, int reps, std::vector<double>& c, std::vector<double>& t) { return debug_clock(a, true, reps, c, t); }

}  // namespace pnp

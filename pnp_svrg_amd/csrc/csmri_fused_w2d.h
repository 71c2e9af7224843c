// csmri_fused_w2d.h -- the 2-D Haar BayesShrink prox (TVDenoiser(multi=False); prox_wavelet2d.hip) in the C layout of the one-kernel
// CSMRI iteration (csmri_fused.hip, phase 5; f32, 256 x 256, L = 5 levels in aligned 32 x 32 tiles).  Included behind
// `#pragma clang fp contract(off)`: every 2 x 2 quad goes through the operations of haar_quad / ihaar_quad in their order (rows
// first, then columns), so the coefficients are those of pnp_prox_wavelet2d bit for bit; only the order of the 15 sums differs.
//
// C layout: wave wv owns image columns [16 wv, 16 wv + 16) and 128 + the same (h2 = 0, 1); lane cl + 16 q keeps rows
// [64 q, 64 q + 64) of both columns in x[h2][0..63].  Level l (s = 2^(l-1)) works in place:
//   rows     : positions p and p + s of a lane, p a multiple of 2 s -- lane-local for all five levels;
//   columns  : lanes cl and cl ^ s, for the lanes with cl a multiple of s (the others hold details of lower levels and keep them).
//              Levels 1..4 stay inside the 16 lanes of a DPP row; level 5 pairs wave wv with wave wv ^ 1.
//   after it : the lane with (cl & s) == 0 holds aa at p and da at p + s, its partner ad at p and dd at p + s.
// Level 5: the level-4 approximation (16 x 16 floats) crosses through the hand-over buffer, both waves of a pair compute the quad, and
// the synthesis needs no second exchange.  Sums of squares: per lane in a fixed order, wave_sum, waves 0..7 in order; a level-5
// coefficient is counted by the even wave of its pair.  No global memory instruction, no atomics.
#pragma once

namespace pnp {

constexpr float kFw2dC = 0.7071067811865476f;              // Haar2<float>::C of prox_wavelet2d.hip
constexpr int kFw2dBands = 15;
// float offsets in the hand-over buffer (idle between phase 4 and `finish`)
constexpr int kFw2dL4 = 0;                                  // [16 level-4 rows][16 level-4 columns]
constexpr int kFw2dBandSum = 256;                           // [8 waves][16]
constexpr int kFw2dThr = 384;                               // [16]

// value of lane ^ S inside a row of 16 lanes
template <int S> __device__ __forceinline__ float fw2d_xor(float v) {
    static_assert(S == 1 || S == 2 || S == 4 || S == 8, "lane distance inside a DPP row");
    if constexpr (S == 1) return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));        // quad_perm [1,0,3,2]
    else if constexpr (S == 2) return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    else if constexpr (S == 8) return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));  // row_ror:8
    else return __shfl_xor(v, 4, 64);
}

__device__ __forceinline__ float fw2d_soft_shrink(float d, float thr) {          // soft_shrink of prox_wavelet2d.hip
    const float mag = d < 0 ? -d : d;
    float shr = 1.0f - thr / mag;
    shr = shr < 0.0f ? 0.0f : shr;                          // keeps NaN (0/0) like numpy clip
    return d * shr;
}

// analysis of level LV <= 4 in place + this lane's share of the level's three sums of squares
template <int LV>
__device__ __forceinline__ void fw2d_analysis_level(float (&x)[2][64], int cl, float* bsum_w, int lane64) {
    constexpr int S = 1 << (LV - 1);
    constexpr float C = kFw2dC;
    const bool part = (cl & (S - 1)) == 0, odd = (cl & S) != 0;
    float sp = 0.f, sq = 0.f;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int p = 0; p < 64; p += 2 * S) {
            const float a0 = x[h2][p], a1 = x[h2][p + S];
            const float lo = C * a1 + C * a0, hi = -C * a1 + C * a0;                // haar_quad: rows first -- this lane's column
            const float plo = fw2d_xor<S>(lo), phi = fw2d_xor<S>(hi);
            const float lo0 = odd ? plo : lo, lo1 = odd ? lo : plo, hi0 = odd ? phi : hi, hi1 = odd ? hi : phi;
            const float n0 = odd ? -C * lo1 + C * lo0 : C * lo1 + C * lo0;          // ad : aa
            const float n1 = odd ? -C * hi1 + C * hi0 : C * hi1 + C * hi0;          // dd : da
            x[h2][p] = part ? n0 : a0;
            x[h2][p + S] = part ? n1 : a1;
            sp += n0 * n0;
            sq += n1 * n1;
            asm volatile("" : "+v"(x[h2][p]), "+v"(x[h2][p + S]));          // one quad at a time: see fused_wavelet2d
            __builtin_amdgcn_sched_barrier(0);
        }
    // the level's three sums leave the registers at once: wave tree, then this wave's row of the table in the hand-over buffer
    const float s_ad = wave_sum(part && odd ? sp : 0.f), s_da = wave_sum(part && !odd ? sq : 0.f), s_dd = wave_sum(part && odd ? sq : 0.f);
    if (lane64 == 0) {
        bsum_w[3 * (LV - 1)] = s_ad;
        bsum_w[3 * (LV - 1) + 1] = s_da;
        bsum_w[3 * (LV - 1) + 2] = s_dd;
    }
}

// shrink + synthesis of level LV <= 4 in place
template <int LV>
__device__ __forceinline__ void fw2d_synthesis_level(float (&x)[2][64], int cl, const float (&thr)[kFw2dBands]) {
    constexpr int S = 1 << (LV - 1);
    constexpr float C = kFw2dC;
    const bool part = (cl & (S - 1)) == 0, odd = (cl & S) != 0;
    const float t1 = odd ? thr[3 * (LV - 1) + 2] : thr[3 * (LV - 1) + 1];
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int p = 0; p < 64; p += 2 * S) {
            const float c0 = x[h2][p], c1 = x[h2][p + S];
            const float u = odd ? fw2d_soft_shrink(c0, thr[3 * (LV - 1)]) : c0;    // shrunk ad : aa
            const float v = fw2d_soft_shrink(c1, t1);                               // shrunk dd : shrunk da
            const float pu = fw2d_xor<S>(u), pv = fw2d_xor<S>(v);
            const float aa = odd ? pu : u, ad = odd ? u : pu, da = odd ? pv : v, dd = odd ? v : pv;
            const float lo = odd ? C * aa - C * ad : C * aa + C * ad;               // ihaar_quad: columns first -- lo_o : lo_e
            const float hi = odd ? C * da - C * dd : C * da + C * dd;               // hi_o : hi_e
            x[h2][p] = part ? C * lo + C * hi : c0;
            x[h2][p + S] = part ? C * lo - C * hi : c1;
            asm volatile("" : "+v"(x[h2][p]), "+v"(x[h2][p + S]));          // one quad at a time: see fused_wavelet2d
            __builtin_amdgcn_sched_barrier(0);
        }
}

// haar_quad / ihaar_quad of prox_wavelet2d.hip, operation for operation
__device__ __forceinline__ void fw2d_haar_quad(float a00, float a01, float a10, float a11, float& aa, float& ad, float& da, float& dd) {
    constexpr float C = kFw2dC;
    const float lo0 = C * a10 + C * a00, lo1 = C * a11 + C * a01;
    const float hi0 = -C * a10 + C * a00, hi1 = -C * a11 + C * a01;
    aa = C * lo1 + C * lo0;
    ad = -C * lo1 + C * lo0;
    da = C * hi1 + C * hi0;
    dd = -C * hi1 + C * hi0;
}
__device__ __forceinline__ void fw2d_ihaar_quad(float aa, float ad, float da, float dd, float& o00, float& o01, float& o10, float& o11) {
    constexpr float C = kFw2dC;
    const float lo_e = C * aa + C * ad, lo_o = C * aa - C * ad;
    const float hi_e = C * da + C * dd, hi_o = C * da - C * dd;
    o00 = C * lo_e + C * hi_e;
    o10 = C * lo_e - C * hi_e;
    o01 = C * lo_o + C * hi_o;
    o11 = C * lo_o - C * hi_o;
}

// Registers: the image is 128 of the lane's 256 registers, and every quad is written so that it needs a handful more.  Left alone
// hipcc does not keep it that way -- it runs the soft thresholds of a whole level (an IEEE division each) side by side and keeps the
// old and the new coefficients of a level alive together: one synthesis level alone then took all 256 registers and spilled 142, the
// whole prox 282.  So every quad hands its two results to an empty asm (they are final before the next quad starts) and a scheduling
// barrier closes it, and the band sums leave for the hand-over buffer level by level: 181 registers in a stand-alone build, no spill.
// The whole prox on x in place.  Whole-workgroup collective (three barriers); on entry no wave reads the hand-over buffer any more
// (the barriers of the noise estimate lie behind phase 4's reads), on exit the caller's next barrier (`finish`) frees it again.
__device__ __forceinline__ void fused_wavelet2d(float (&x)[2][64], float* ldf, float var, int t) {
    const int lane64 = t & 63, wv = t >> 6, cl = lane64 & 15, q = lane64 >> 4;
    float* bsum = ldf + kFw2dBandSum;
    float* thr_sh = ldf + kFw2dThr;
    fw2d_analysis_level<1>(x, cl, bsum + wv * 16, lane64);
    fw2d_analysis_level<2>(x, cl, bsum + wv * 16, lane64);
    fw2d_analysis_level<3>(x, cl, bsum + wv * 16, lane64);
    fw2d_analysis_level<4>(x, cl, bsum + wv * 16, lane64);
    // ---- level 5: the level-4 approximation of column 16 (wv + 8 h2), rows 16 (4 q + k), sits on lane cl == 0 at x[h2][16 k]
    float* l4 = ldf + kFw2dL4;
    if (cl == 0) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int k = 0; k < 4; ++k) l4[(4 * q + k) * 16 + wv + 8 * h2] = x[h2][16 * k];
    }
    __syncthreads();
    const bool oddw = (wv & 1) != 0;
    // one level-5 quad from this wave's column (x) and the partner wave's (the hand-over buffer, the same rows): the same operands
    // in the same operations before and after the thresholds are known, so nothing of it has to stay in registers in between
    auto quad5 = [&](int h2, int m, float& aa, float& ad, float& da, float& dd) {
        const float o0 = x[h2][32 * m], o1 = x[h2][32 * m + 16];
        const float p0 = l4[(4 * q + 2 * m) * 16 + (wv ^ 1) + 8 * h2], p1 = l4[(4 * q + 2 * m + 1) * 16 + (wv ^ 1) + 8 * h2];
        fw2d_haar_quad(oddw ? p0 : o0, oddw ? o0 : p0, oddw ? p1 : o1, oddw ? o1 : p1, aa, ad, da, dd);
    };
    {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float aa, ad, da, dd;
                quad5(h2, m, aa, ad, da, dd);
                s0 += ad * ad;
                s1 += da * da;
                s2 += dd * dd;
            }
        const bool count = cl == 0 && !oddw;                // held by two waves, counted once
        s0 = wave_sum(count ? s0 : 0.f);
        s1 = wave_sum(count ? s1 : 0.f);
        s2 = wave_sum(count ? s2 : 0.f);
        if (lane64 == 0) {
            bsum[wv * 16 + 12] = s0;
            bsum[wv * 16 + 13] = s1;
            bsum[wv * 16 + 14] = s2;
        }
    }
    // ---- the 15 sums: lane, wave tree (above), waves 0..7 in order; thresholds as prox_wavelet2d_body.h
    __syncthreads();
    if (t < kFw2dBands) {
        const int l = t / 3 + 1;
        float ss = bsum[t];
        for (int w = 1; w < 8; ++w) ss += bsum[w * 16 + t];
        const float dvar = ss / (float)((FN >> l) * (FN >> l));
        float den = dvar - var;
        den = (den > 2.220446049250313e-16f || den != den) ? den : 2.220446049250313e-16f;   // max(NaN, eps) is NaN
        thr_sh[t] = var / sqrtf(den);
    }
    __syncthreads();
    float thr[kFw2dBands];
#pragma unroll
    for (int k = 0; k < kFw2dBands; ++k)                   // uniform: kept in scalar registers
        thr[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, thr_sh[k])));
    // ---- shrink + synthesis, level 5 first (each wave of a pair takes its own column of the quad)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float aa, ad, da, dd, o00, o01, o10, o11;
            quad5(h2, m, aa, ad, da, dd);
            fw2d_ihaar_quad(aa, fw2d_soft_shrink(ad, thr[12]), fw2d_soft_shrink(da, thr[13]), fw2d_soft_shrink(dd, thr[14]), o00, o01,
                            o10, o11);
            if (cl == 0) {
                x[h2][32 * m] = oddw ? o01 : o00;
                x[h2][32 * m + 16] = oddw ? o11 : o10;
            }
        }
    fw2d_synthesis_level<4>(x, cl, thr);
    fw2d_synthesis_level<3>(x, cl, thr);
    fw2d_synthesis_level<2>(x, cl, thr);
    fw2d_synthesis_level<1>(x, cl, thr);
}

}  // namespace pnp

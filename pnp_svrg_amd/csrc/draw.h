// draw.h -- device-side minibatch draws (problems/problem.py:110-117, problems/CSMRI.py:66-74:
// `np.random.choice(candidates, size, replace=False)`) as counter-based keys + a threshold.
//
// Every candidate position i gets the 32-bit key  mb_key(state, i),  state = mix64(mix64(mix64(seed) + step) +
// problem); the `mb` smallest (key, i) pairs are the minibatch (uniform without replacement; the pairs are distinct,
// so a draw is deterministic).  Only the THRESHOLD pair (T, P) of each (problem, step) is computed (k_draw_thr);
// consumers re-derive membership (mb_member) where they need it, so a minibatch never exists as an array unless a
// caller asks for one.  The fields are absorbed one at a time, so streams of different seeds / steps / problems are
// unrelated (no XOR-aliasing between the fields).  NOT the NumPy legacy stream: reference-identical draws come from
// the host.
#pragma once
#include "common.h"
#include <cstdlib>

namespace pnp {

inline int draw_fast_path() { return getenv("PNP_DRAW_NO_FAST") == nullptr ? 1 : 0; }

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {      // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
struct MbDesc { uint64_t state; uint32_t T, P; };
// Per-position key: a 32-bit mixer (two 32-bit multiplies; 64-bit multiplies are several quarter-rate instructions each
// on gfx950 and this runs once per k-space position) of the position XOR the stream's low word, XOR the stream's high
// word.  For a fixed stream it is a BIJECTION of the position, so keys never tie inside one draw.
__host__ __device__ __forceinline__ uint32_t mb_key(uint64_t state, uint32_t i) {
    uint32_t x = (uint32_t)state ^ i;
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x ^ (uint32_t)(state >> 32);
}
__device__ __forceinline__ bool mb_member(const MbDesc& d, uint32_t i) {
    const uint32_t key = mb_key(d.state, i);
    return key < d.T || (key == d.T && i <= d.P);
}

// One workgroup per (problem, step): a whole outer iteration's draws are one launch.
// Radix select, 12 + 12 + 8 bits: histogram of the current digit in LDS, pick the bucket that holds rank `mb`; as
// soon as that bucket has at most DRAW_LIST keys they are collected and ranked by brute force.
// MASKED: candidates are the set bits of a transposed bit-packed H x W mask (word [kx][ky >> 5], bit ky & 31),
//         position i = ky*W + kx (the flat row-major index np.flatnonzero counts);
// else  : candidates are all of 0 .. H*W-1 (pass H = 1, W = M for a length-M measurement vector).
constexpr int DRAW_BINS = 4096, DRAW_LIST = 1024;

template <bool MASKED>
__global__ __launch_bounds__(256) void k_draw_thr(const uint32_t* __restrict__ bitsT, int H, int W, int mb, uint64_t seed,
                                                  uint32_t step0, const uint32_t* __restrict__ step_dev,
                                                  MbDesc* __restrict__ mbd, uint32_t* __restrict__ selbits, int fast) {
#define PNP_DRAW_ID (uint64_t)prob
#include "draw_thr_body.h"
#undef PNP_DRAW_ID
}

// Per-problem form (the _pp entry points): problem b takes its own mb_vec[b] smallest keys, and its stream absorbs
// draw_id[b] in place of the batch index (NULL: the batch index) -- a problem's minibatches then follow its id, not its
// place in the batch.  The host cannot see mb_vec without a synchronisation; an entry below 1 draws as 1 (never out of bounds).
template <bool MASKED>
__global__ __launch_bounds__(256) void k_draw_thr_pp(const uint32_t* __restrict__ bitsT, int H, int W,
                                                     const int32_t* __restrict__ mb_vec, const uint32_t* __restrict__ draw_id,
                                                     uint64_t seed, uint32_t step0, const uint32_t* __restrict__ step_dev,
                                                     MbDesc* __restrict__ mbd, uint32_t* __restrict__ selbits, int fast) {
    const int mb = mb_vec[blockIdx.x] < 1 ? 1 : mb_vec[blockIdx.x];
    const uint64_t id = draw_id != nullptr ? (uint64_t)draw_id[blockIdx.x] : (uint64_t)(int)blockIdx.x;
#define PNP_DRAW_ID id
#include "draw_thr_body.h"
#undef PNP_DRAW_ID
}

}  // namespace pnp

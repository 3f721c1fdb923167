// gsr_select.h -- the pieces of the exact radix selection that gsr_points.hip (Regr3D's quantiles) and gsr_outputs.hip (depth range,
// PLY normaliser) share: the ranks torch.quantile reads, torch's lerp, the grouped LDS histogram bump and the one-wavefront pick of a
// digit.  Selection runs over 32-bit keys in four 8-bit digit passes; what a key is and which elements are counted is the caller's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int SEL_BINS = 256, SEL_RANKS = 4, SEL_PASSES = 4;

// selected values are compared with the data they were selected from: no contraction may change a bit between two users
#pragma clang fp contract(off)

// the two ranks torch.quantile reads for one q over n elements: floor / ceil of float32(q) * float32(n - 1), and the lerp weight
__device__ inline void sel_rank_pair(float q, long long n, uint32_t *k, float *w)
{
    const float pos = q * (float)(n - 1);
    const float lo = floorf(pos);
    k[0] = (uint32_t)lo;
    k[1] = (uint32_t)ceilf(pos);
    *w = pos - lo;
}
// torch's lerp(a, b, w)
__device__ inline float sel_lerp(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w); }

// every valid lane bumps h[digit]: one LDS atomic per DISTINCT digit of the wavefront (pass 0 sees the exponent byte: two or three values)
__device__ inline void hist_bump_grouped(uint32_t *h, uint32_t digit, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)digit, leader);
        const unsigned long long m = __ballot(valid && digit == dl);
        if (lane == leader) atomicAdd(h + dl, (uint32_t)__popcll(m));
        todo &= ~m;
    }
}

// one digit of one rank, by ONE wavefront: the bin of `h[256]` that holds rank k (0-based among the counted keys); returns the digit and
// leaves in k the rank inside that bin.  Same result in every lane.
__device__ inline uint32_t sel_pick(const uint32_t *h, uint32_t &k)
{
    const int lane = threadIdx.x & 63;
    const uint32_t c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
    const uint32_t s = c0 + c1 + c2 + c3;
    uint32_t incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
    }
    const uint32_t excl = incl - s;
    const unsigned long long hit = __ballot(excl <= k && k < incl);
    const int src = hit ? __ffsll((long long)hit) - 1 : 63;          // (no hit: k beyond the count, cannot happen with every key counted)
    uint32_t r = k - excl, d = 4 * lane;
    if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
    k = (uint32_t)__shfl((int)r, src, 64);
    return (uint32_t)__shfl((int)d, src, 64);
}

#pragma clang fp contract(fast)

}  // namespace gsr

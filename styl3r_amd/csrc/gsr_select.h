// gsr_select.h -- the exact radix selection that stands in for torch.quantile / torch.median: gsr_points.hip (Regr3D's quantiles of |gt|)
// and gsr_outputs.hip (depth range, PLY normaliser) run it.  Selection goes over the order-preserving 32-bit image of the fp32 values in
// four 8-bit digit passes: a map is cut into chunks over many workgroups that add LDS histograms into a global integer histogram
// (k_digit_hist), and one workgroup per map picks a digit of every followed rank between the passes (k_digit_pick); sel_run issues the
// eight launches.  No host sync, no float atomics, two runs give the same bits.
//
// A caller states WHAT is selected with a source object, a trivially copyable struct passed to the kernels by value:
//   long long n                       elements per map
//   SelPlan plan()                    at most two rank pairs (floor / ceil rank of a quantile, or the lower median), each over its own
//                                     subset of the elements (all, or the positive ones); ranks come from the subset's count
//   float value(m, i, pass)           element i of map m (pass 0 may compute and store it, later passes read it back)
//   void finish(m, vals, w, nan)      called by one thread of the last pick: the four selected values, the two lerp weights, the NaN flag
// Everything else -- chunk walk, histograms, prefixes, ranks, NaN flag, scratch, launch loop -- is here, once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_common.h"

namespace gsr {

constexpr int SEL_BINS = 256, SEL_RANKS = 4, SEL_PASSES = 4, SEL_BLOCK = 256;
enum { SEL_ALL = 0, SEL_POSITIVE = 1 };                  // a pair's subset: every element / those with v > 0
constexpr float SEL_MEDIAN = -1.0f, SEL_UNUSED = -2.0f;    // a pair's q: the lower median instead of a quantile / the pair is not followed

struct SelPlan {
    float q[2];
    int subset[2];
};
__host__ __device__ inline bool sel_two(const SelPlan &p) { return p.q[1] >= -1.5f; }
// pass 0 counts one histogram row per DISTINCT subset; pair g's count is in row sel_row0(p, g)
__host__ __device__ inline int sel_rows0(const SelPlan &p) { return sel_two(p) && p.subset[1] != p.subset[0] ? 2 : 1; }
__host__ __device__ inline int sel_row0(const SelPlan &p, int g) { return g ? sel_rows0(p) - 1 : 0; }

// per-map selection state
struct SelScratch {
    uint32_t *hist;      // [maps][SEL_RANKS][SEL_BINS]
    uint32_t *nanflag;   // [maps]
    uint32_t *sel;       // [maps][SEL_RANKS][2]: key prefix found so far, rank left inside it
    uint32_t *cnt;       // [maps][2]: elements counted by each pair's subset
    float *w;            // [maps][2]: lerp weight of each pair
    float *vals;         // [maps][SEL_RANKS]: the selected values
};
inline SelScratch sel_carve(Carver &c, size_t maps)
{
    SelScratch s;
    s.hist = c.take<uint32_t>(maps * SEL_RANKS * SEL_BINS);
    s.nanflag = c.take<uint32_t>(maps);
    s.sel = c.take<uint32_t>(maps * SEL_RANKS * 2);
    s.cnt = c.take<uint32_t>(maps * 2);
    s.w = c.take<float>(maps * 2);
    s.vals = c.take<float>(maps * SEL_RANKS);
    return s;
}
// the words that must be zero before sel_run: histograms and NaN flags (the picks leave the histograms at zero again)
inline size_t sel_zero_bytes(const SelScratch &s) { return reinterpret_cast<char *>(s.sel) - reinterpret_cast<char *>(s.hist); }

// selected values are compared with the data they were selected from: no contraction may change a bit between two users
#pragma clang fp contract(off)

// order-preserving: a < b as floats <=> key(a) < key(b) as unsigned.  A NaN sorts at an end and shifts the ranks of its subset; the
// map's flag overrides whatever was selected then.  On |gt| = sqrtf(sum of squares), which is never negative and never -0, the key is
// bits | 0x80000000: the order of the bare bits, and sel_unkey gives the bits back.
__device__ inline uint32_t sel_key(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float sel_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ inline bool sel_in(int subset, float v) { return subset == SEL_ALL || v > 0.f; }

// the two ranks torch.quantile reads for one q over n elements: floor / ceil of float32(q) * float32(n - 1), and the lerp weight
__device__ inline void sel_rank_pair(float q, long long n, uint32_t *k, float *w)
{
    const float pos = q * (float)(n - 1);
    const float lo = floorf(pos);
    k[0] = (uint32_t)lo;
    k[1] = (uint32_t)ceilf(pos);
    *w = pos - lo;
}
// rank j (0: floor, 1: ceil) of a pair over its c counted elements, and the pair's lerp weight (an empty subset or an unused pair: 0, 0)
__device__ inline uint32_t sel_rank(float q, uint32_t c, int j, float *w)
{
    uint32_t k[2] = {0u, 0u};
    *w = 0.f;
    if (c > 0u && q >= 0.f) sel_rank_pair(q, (long long)c, k, w);
    else if (c > 0u && q >= -1.5f) k[0] = k[1] = (c - 1u) >> 1;              // torch.median: the lower of the two middle elements
    return j ? k[1] : k[0];
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

// passes 1..3: the upper bits of the four followed ranks' prefixes (prefix[r * stride]), and the bump of one key under them: row r of
// h gets the key's next digit if the key continues rank r's prefix; in0 / in1: the key is in the subset of pair 0 / 1 (ranks 0, 1 / 2, 3)
struct SelPrefixes { uint32_t p0, p1, p2, p3; int shift; };
__device__ inline SelPrefixes sel_prefixes(const uint32_t *prefix, int stride, int pass)
{
    const int shift = 24 - 8 * pass;
    return {prefix[0] >> (shift + 8), prefix[stride] >> (shift + 8), prefix[2 * stride] >> (shift + 8), prefix[3 * stride] >> (shift + 8), shift};
}
__device__ inline void sel_bump_ranks(uint32_t *h, uint32_t key, const SelPrefixes &p, bool in0, bool in1)
{
    const uint32_t top = key >> (p.shift + 8), dg = (key >> p.shift) & 255u;
    if (in0) {
        if (top == p.p0) atomicAdd(h + dg, 1u);
        if (top == p.p1) atomicAdd(h + SEL_BINS + dg, 1u);
    }
    if (in1) {
        if (top == p.p2) atomicAdd(h + 2 * SEL_BINS + dg, 1u);
        if (top == p.p3) atomicAdd(h + 3 * SEL_BINS + dg, 1u);
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
    const int src = hit ? __ffsll((long long)hit) - 1 : 63;          // (no hit: an empty subset; its values are never read)
    uint32_t r = k - excl, d = 4 * lane;
    if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
    k = (uint32_t)__shfl((int)r, src, 64);
    return (uint32_t)__shfl((int)d, src, 64);
}

// one digit pass over (chunk, map) workgroups.  Pass 0 counts the top byte per SUBSET, the later passes the next byte of the keys
// under each RANK's prefix (two rows per followed pair).
template <class Src>
__global__ void __launch_bounds__(SEL_BLOCK) k_digit_hist(Src s, int pass, SelScratch sc)
{
    __shared__ uint32_t h[SEL_RANKS * SEL_BINS];
    const SelPlan pl = s.plan();
    const int m = blockIdx.y, tid = threadIdx.x;
    const long long per = (s.n + gridDim.x - 1) / gridDim.x, i0 = (long long)blockIdx.x * per, i1 = min(s.n, i0 + per);
    const bool two = sel_two(pl);
    const int rows = pass == 0 ? sel_rows0(pl) : (two ? SEL_RANKS : 2);
    for (int t = tid; t < rows * SEL_BINS; t += SEL_BLOCK) h[t] = 0u;
    __syncthreads();
    if (pass == 0) {
        bool nan = false;
        for (long long base = i0; base < i1; base += SEL_BLOCK) {       // (uniform trip count: the grouped bump is a wave-wide operation)
            const long long i = base + tid;
            const bool ok = i < i1;
            float v = 0.f;
            if (ok) { v = s.value(m, i, 0); nan |= v != v; }
            const uint32_t dg = sel_key(v) >> 24;
            hist_bump_grouped(h, dg, ok && sel_in(pl.subset[0], v));
            if (rows == 2) hist_bump_grouped(h + SEL_BINS, dg, ok && sel_in(pl.subset[1], v));
        }
        if (nan) atomicOr(sc.nanflag + m, 1u);
    } else {
        const SelPrefixes p = sel_prefixes(sc.sel + (size_t)m * SEL_RANKS * 2, 2, pass);
        for (long long i = i0 + tid; i < i1; i += SEL_BLOCK) {
            const float v = s.value(m, i, pass);
            sel_bump_ranks(h, sel_key(v), p, sel_in(pl.subset[0], v), two && sel_in(pl.subset[1], v));
        }
    }
    __syncthreads();
    uint32_t *hg = sc.hist + (size_t)m * SEL_RANKS * SEL_BINS;
    for (int t = tid; t < rows * SEL_BINS; t += SEL_BLOCK)
        if (h[t]) atomicAdd(hg + t, h[t]);
}

// one workgroup per map, wave r follows rank r (pair r / 2).  Pass 0 also turns the pair's count into its two ranks; the last pass
// un-keys the four prefixes and hands them to the source's finish.  Every pass re-arms the histogram.
template <class Src>
__global__ void __launch_bounds__(SEL_BLOCK) k_digit_pick(Src s, int pass, SelScratch sc)
{
    __shared__ float picked[SEL_RANKS];
    const SelPlan pl = s.plan();
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = wave >> 1, shift = 24 - 8 * pass;
    uint32_t *hg = sc.hist + (size_t)m * SEL_RANKS * SEL_BINS, *sp = sc.sel + (size_t)m * SEL_RANKS * 2;
    const uint32_t *row = hg + (pass == 0 ? sel_row0(pl, grp) : wave) * SEL_BINS;
    uint32_t k, before = 0u;
    if (pass == 0) {
        uint32_t c = row[4 * lane] + row[4 * lane + 1] + row[4 * lane + 2] + row[4 * lane + 3];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
        float wt;
        k = sel_rank(grp ? pl.q[1] : pl.q[0], c, wave & 1, &wt);
        if (lane == 0 && !(wave & 1)) { sc.cnt[2 * m + grp] = c; sc.w[2 * m + grp] = wt; }
    } else {
        k = sp[2 * wave + 1];
        before = sp[2 * wave];
    }
    const uint32_t now = before | (sel_pick(row, k) << shift);
    if (lane == 0) {
        sp[2 * wave] = now; sp[2 * wave + 1] = k;
        if (pass == SEL_PASSES - 1) sc.vals[SEL_RANKS * m + wave] = picked[wave] = sel_unkey(now);
    }
    __syncthreads();
    for (int t = tid; t < SEL_RANKS * SEL_BINS; t += SEL_BLOCK) hg[t] = 0u;      // re-armed for the next pass (and the next selection)
    if (pass == SEL_PASSES - 1 && tid == 0) {
        const float w[2] = {sc.w[2 * m], sc.w[2 * m + 1]};
        s.finish(m, picked, w, sc.nanflag[m] != 0u);
    }
}

#pragma clang fp contract(fast)

// the eight launches of one selection over `maps` maps of `chunks` chunks each; sel_zero_bytes(sc) must be zero on entry
template <class Src>
inline void sel_run(const Src &s, int maps, int chunks, const SelScratch &sc, hipStream_t st)
{
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        hipLaunchKernelGGL(k_digit_hist<Src>, dim3(chunks, maps), dim3(SEL_BLOCK), 0, st, s, pass, sc);
        hipLaunchKernelGGL(k_digit_pick<Src>, dim3(maps), dim3(SEL_BLOCK), 0, st, s, pass, sc);
    }
}

}  // namespace gsr

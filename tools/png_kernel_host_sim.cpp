// png_kernel_host_sim.cpp -- the kernels of styl3r_amd/csrc/gsr_png.hip run on the CPU for the host sanitizers: the file is compiled as
// plain C++17 (GSR_PNG_HOST_SIM) with stand-ins for the HIP built-ins it uses, one workgroup = 256 OS threads, __syncthreads = a barrier,
// the wave shuffle through memory, LDS atomics = host atomics.  It proves nothing about the GPU's memory model; it shows that no index
// leaves the LDS tables, the scratch slots or the output (AddressSanitizer), that no arithmetic overflows (UBSan), and that the streams
// are valid: for a set of built-in pictures -- 1 x 1, noise (stored blocks, also at the full 16 384-byte chunk), flat, long runs with
// remainders of 1 and 2, one run over a whole chunk, a smooth picture over several chunks in both source forms -- every stream is
// inflated by zlib (which checks the Adler-32), un-filtered by the rules of the PNG specification and compared with the source picture.
// The scratch and the output are heap blocks of exactly the sizes the size queries report.  Exit code 0 and "clean" when all agree.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/png_kernel_host_sim.cpp -lz -o png_sim && ./png_sim
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <thread>
#include <vector>

using std::max;
using std::min;
#define GSR_PNG_HOST_SIM 1
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __constant__ static const
struct SimIdx {
    unsigned x, y, z;
};
static thread_local SimIdx threadIdx, blockIdx;
static pthread_barrier_t g_block_barrier, g_wave_barrier[4];
static uint32_t g_shfl[4][64];
static inline void __syncthreads() { pthread_barrier_wait(&g_block_barrier); }
static inline uint32_t __shfl_xor(uint32_t v, int d, int)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_shfl[w][l] = v;
    pthread_barrier_wait(&g_wave_barrier[w]);
    const uint32_t r = g_shfl[w][l ^ d];
    pthread_barrier_wait(&g_wave_barrier[w]);
    return r;
}
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline uint32_t __brev(uint32_t v)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}

#include "../styl3r_amd/csrc/gsr_png.hip"

template <class F>
static void run_block(unsigned bx, F f)
{
    pthread_barrier_init(&g_block_barrier, nullptr, 256);
    for (auto &b : g_wave_barrier) pthread_barrier_init(&b, nullptr, 64);
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < 256; ++t)
        threads.emplace_back([=] {
            threadIdx = {t, 0, 0};
            blockIdx = {bx, 0, 0};
            f();
        });
    for (auto &t : threads) t.join();
    pthread_barrier_destroy(&g_block_barrier);
    for (auto &b : g_wave_barrier) pthread_barrier_destroy(&b);
}

static int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

static long g_chunks = 0, g_images = 0;

// bytes: N * H * W * C interleaved; as_float: hand the kernels the same picture as planar fp32 (byte / 255, which converts back exactly)
static bool run_case(const char *name, const std::vector<uint8_t> &bytes, int N, int H, int W, int C, int filter_mode, bool as_float)
{
    gsr::PngPlan p;
    if (gsr::png_plan(N, H, W, C, p) != GSR_OK) {
        printf("%s: png_plan refused\n", name);
        return false;
    }
    std::vector<float> planar;
    if (as_float) {
        planar.resize(bytes.size());
        for (int n = 0; n < N; ++n)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    for (int c = 0; c < C; ++c)
                        planar[(((size_t)n * C + c) * H + y) * W + x] = (float)bytes[(((size_t)n * H + y) * W + x) * C + c] / 255.0f + 1e-4f;
    }
    const void *src = as_float ? (const void *)planar.data() : (const void *)bytes.data();
    uint8_t *scratch = (uint8_t *)malloc(p.scratch_bytes), *out = (uint8_t *)malloc((size_t)N * p.bound);
    int32_t *lengths = (int32_t *)malloc(sizeof(int32_t) * N);
    memset(scratch, 0xA5, p.scratch_bytes);
    memset(out, 0xA5, (size_t)N * p.bound);
    int32_t *meta = (int32_t *)scratch;
    uint8_t *slots = scratch + p.meta_bytes;
    for (long long b = 0; b < p.chunks; ++b)
        run_block((unsigned)b, [=] {
            if (as_float) gsr::k_png_chunks<GSR_PNG_SRC_F32_PLANAR>(src, H, W, C, filter_mode, p.rows, p.chunks_per_image, meta, slots);
            else gsr::k_png_chunks<GSR_PNG_SRC_U8>(src, H, W, C, filter_mode, p.rows, p.chunks_per_image, meta, slots);
        });
    for (long long b = 0; b < p.chunks; ++b)
        run_block((unsigned)b, [=] { gsr::k_png_assemble(meta, slots, p.chunks_per_image, out, (long long)p.bound, lengths); });
    g_chunks += p.chunks;
    bool ok = true;
    const size_t row = 1 + (size_t)W * C;
    std::vector<uint8_t> filt(row * H), img((size_t)H * W * C);
    for (int n = 0; n < N && ok; ++n, ++g_images) {
        uLongf got = filt.size();
        const int rc = uncompress(filt.data(), &got, out + (size_t)n * p.bound, (uLong)lengths[n]);
        if (rc != Z_OK || got != filt.size() || lengths[n] > (int32_t)p.bound) {
            printf("%s: image %d: zlib says %d, %lu of %zu bytes, stream %d of at most %zu\n", name, n, rc, (unsigned long)got, filt.size(), lengths[n], p.bound);
            ok = false;
            break;
        }
        for (int y = 0; y < H; ++y) {
            const int f = filt[y * row];
            if (f > 4 || (filter_mode == 1 && f != 0)) ok = false;
            for (int j = 0; j < W * C; ++j) {
                const int a = j >= C ? img[(size_t)y * W * C + j - C] : 0, b = y ? img[(size_t)(y - 1) * W * C + j] : 0;
                const int c = (y && j >= C) ? img[(size_t)(y - 1) * W * C + j - C] : 0;
                const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) / 2 : paeth(a, b, c);
                img[(size_t)y * W * C + j] = (uint8_t)(filt[y * row + 1 + j] + pred);
            }
        }
        if (memcmp(img.data(), bytes.data() + (size_t)n * img.size(), img.size()) != 0) ok = false;
        if (!ok) printf("%s: image %d does not decode to the source picture\n", name, n);
    }
    free(scratch), free(out), free(lengths);
    printf("%-28s %s\n", name, ok ? "ok" : "FAILED");
    return ok;
}

int main()
{
    uint32_t state = 12345u;
    auto rnd = [&] { return (state = state * 1664525u + 1013904223u) >> 24; };
    auto picture = [&](int N, int H, int W, int C, int kind) {
        std::vector<uint8_t> v((size_t)N * H * W * C);
        for (int n = 0; n < N; ++n)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    for (int c = 0; c < C; ++c) {
                        int b = 0;
                        if (kind == 0) b = (int)rnd();                                                        // noise
                        if (kind == 1) b = 77;                                                                // flat
                        if (kind == 2) b = (x * 200 / (W > 1 ? W - 1 : 1) + y * 55 / (H > 1 ? H - 1 : 1) + 9 * c + 30 * n + (int)(rnd() & 7)) & 255;   // smooth
                        if (kind == 3) b = ((x - W / 2) * (x - W / 2) + (y - H / 2) * (y - H / 2) < H * W / 16) ? 200 - 3 * c : 0;   // disc on black
                        v[(((size_t)n * H + y) * W + x) * C + c] = (uint8_t)b;
                    }
        return v;
    };
    bool ok = true;
    for (int C = 3; C <= 4; ++C) {
        ok &= run_case("1 x 1", picture(1, 1, 1, C, 0), 1, 1, 1, C, 0, false);
        ok &= run_case("3 x 5 noise, 2 images", picture(2, 5, 3, C, 0), 2, 5, 3, C, 0, false);
        ok &= run_case("smooth, three chunks", picture(2, 120, 100, C, 2), 2, 120, 100, C, 0, false);
        ok &= run_case("smooth, fp32 planar", picture(1, 60, 100, C, 2), 1, 60, 100, C, 0, true);
    }
    ok &= run_case("noise, two chunks", picture(1, 70, 90, 3, 0), 1, 70, 90, 3, 0, false);
    ok &= run_case("noise, a full chunk", picture(1, 1, 5461, 3, 0), 1, 1, 5461, 3, 1, false);
    ok &= run_case("one run over a full chunk", std::vector<uint8_t>(5461 * 3, 0), 1, 1, 5461, 3, 1, false);
    ok &= run_case("flat", picture(1, 120, 100, 3, 1), 1, 120, 100, 3, 0, false);
    ok &= run_case("flat, filter none", picture(1, 120, 100, 3, 1), 1, 120, 100, 3, 1, false);
    ok &= run_case("disc on black", picture(1, 96, 96, 3, 3), 1, 96, 96, 3, 0, false);
    ok &= run_case("wide rows", picture(1, 3, 1920, 3, 2), 1, 3, 1920, 3, 0, false);
    {
        std::vector<uint8_t> runs;
        const int lens[] = {300, 260, 261, 259, 1000, 3, 4, 2};
        for (int k = 0; k < 8; ++k) runs.insert(runs.end(), lens[k], (uint8_t)(k ? 4 + k : 0));
        for (int k = 30; k < 60; ++k) runs.push_back((uint8_t)k);
        while (runs.size() % 3) runs.push_back(99);
        ok &= run_case("run remainders", runs, 1, 1, (int)runs.size() / 3, 3, 1, false);
    }
    {   // a Fibonacci histogram over 16 byte values, the filter byte and the end of block: the 15-bit limit must repair a 17-bit code
        std::vector<uint8_t> vals;
        int f0 = 1, f1 = 1;
        for (int k = 16; k >= 1; --k) {
            const int f = f0 + f1;
            f0 = f1, f1 = f;
            vals.insert(vals.begin(), f, (uint8_t)(7 * (17 - k)));
        }
        std::vector<uint8_t> rowv(vals.size());
        const size_t half = (vals.size() + 1) / 2;
        for (size_t i = 0; i < vals.size(); ++i) rowv[i] = (i & 1) ? vals[half + i / 2] : vals[i / 2];
        ok &= run_case("fibonacci histogram", rowv, 1, 1, (int)rowv.size() / 3, 3, 1, false);
    }
    printf("%ld images, %ld chunks: %s\n", g_images, g_chunks, ok ? "clean" : "FAILED");
    return ok ? 0 : 1;
}

// jpeg_enc_host_sim.cpp -- the kernels of styl3r_amd/csrc/gsr_jpeg_enc.hip run on the CPU, for the host sanitizers and for comparing the
// scan with libjpeg's where there is no GPU: the file is compiled as plain C++17 (GSR_JPEG_ENC_HOST_SIM) with stand-ins for the HIP
// built-ins it uses, one workgroup = as many OS threads, __syncthreads = a barrier, LDS atomics = host atomics.  It proves nothing about
// the GPU's memory model; it shows that no index leaves the LDS tables, the scratch or the output (AddressSanitizer: the scratch and the
// output are heap blocks of exactly the sizes the size queries report, the output stride is the bound), that no arithmetic overflows
// (UBSan), and it writes the scans so that a script can hold them against Pillow's.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_enc_host_sim.cpp -o jpeg_enc_sim
//   ./jpeg_enc_sim case.bin scans.bin
// case.bin: int32 N, H, W, sampling (GSR_JPEG_444 / 422 / 420), src_kind; uint16 quant[128] (natural order); the pictures, uint8 (N,H,W,3)
// or fp32 (N,3,H,W).  scans.bin: per picture int32 length, then the bytes.  Exit code 0 when every byte behind a scan kept its fill value.
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

using std::max;
using std::min;
#define GSR_JPEG_ENC_HOST_SIM 1
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
static pthread_barrier_t g_block_barrier;
static inline void __syncthreads() { pthread_barrier_wait(&g_block_barrier); }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }

#include "../styl3r_amd/csrc/gsr_jpeg_enc.hip"

template <class F>
static void run_block(unsigned bx, unsigned nthreads, F f)
{
    pthread_barrier_init(&g_block_barrier, nullptr, nthreads);
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < nthreads; ++t)
        threads.emplace_back([=] {
            threadIdx = {t, 0, 0};
            blockIdx = {bx, 0, 0};
            f();
        });
    for (auto &t : threads) t.join();
    pthread_barrier_destroy(&g_block_barrier);
}

int main(int argc, char **argv)
{
    using namespace gsr;
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    JeQuant q;
    if (fread(head, 4, 5, f) != 5 || fread(q.q, 2, 128, f) != 128) return 2;
    const int N = head[0], H = head[1], W = head[2], sampling = head[3], kind = head[4];
    const size_t pixels = (size_t)N * H * W * 3 * (kind == GSR_JPEG_ENC_SRC_U8 ? 1 : 4);
    uint8_t *src = (uint8_t *)malloc(pixels);
    if (fread(src, 1, pixels, f) != pixels) return 2;
    fclose(f);
    JePlan p;
    if (je_plan(N, H, W, sampling, p) != GSR_OK) {
        printf("je_plan refused\n");
        return 2;
    }
    uint8_t *base = (uint8_t *)malloc(p.scratch_bytes), *out = (uint8_t *)malloc((size_t)N * p.bound);
    int32_t *lengths = (int32_t *)malloc(sizeof(int32_t) * N);
    memset(base, 0xA5, p.scratch_bytes);
    memset(out, 0xA5, (size_t)N * p.bound);
    int16_t *coef = reinterpret_cast<int16_t *>(base);
    uint16_t *bits = reinterpret_cast<uint16_t *>(base + p.off_bits);
    uint32_t *seg_bits = reinterpret_cast<uint32_t *>(base + p.off_seg_bits), *seg_off = reinterpret_cast<uint32_t *>(base + p.off_seg_off);
    uint32_t *seg_ff = reinterpret_cast<uint32_t *>(base + p.off_seg_ff), *image_bits = reinterpret_cast<uint32_t *>(base + p.off_image_bits);
    int16_t *seg_dc = reinterpret_cast<int16_t *>(base + p.off_seg_dc);
    uint8_t *raw = base + p.off_raw;
    const unsigned groups = (unsigned)(N * p.g.segs);
    for (unsigned b = 0; b < groups; ++b)
        run_block(b, JE_THREADS, [=] {
            if (kind == GSR_JPEG_ENC_SRC_U8) k_jpeg_enc_transform<GSR_JPEG_ENC_SRC_U8>(src, p.g, q, coef, bits, seg_bits, seg_dc);
            else k_jpeg_enc_transform<GSR_JPEG_ENC_SRC_F32_PLANAR>(src, p.g, q, coef, bits, seg_bits, seg_dc);
        });
    for (unsigned b = 0; b < (unsigned)N; ++b) run_block(b, JE_THREADS, [=] { k_jpeg_enc_scan(p.g, coef, bits, seg_bits, seg_dc, seg_off, image_bits); });
    for (unsigned b = 0; b < groups; ++b)
        run_block(b, JE_CODE_THREADS, [=] { k_jpeg_enc_code(p.g, coef, bits, seg_off, image_bits, raw, p.raw_stride, seg_ff); });
    for (unsigned b = 0; b < groups; ++b)
        run_block(b, JE_THREADS, [=] { k_jpeg_enc_assemble(p.g, seg_off, image_bits, seg_ff, raw, p.raw_stride, out, p.bound, lengths); });
    bool ok = true;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int n = 0; n < N; ++n) {
        if (lengths[n] < 2 || (size_t)lengths[n] > p.bound) {
            printf("picture %d: length %d outside [2, %zu]\n", n, lengths[n], p.bound);
            return 1;
        }
        for (size_t i = (size_t)lengths[n]; i < p.bound; ++i) ok &= out[n * p.bound + i] == 0xA5;
        fwrite(&lengths[n], 4, 1, o);
        fwrite(out + n * p.bound, 1, (size_t)lengths[n], o);
    }
    fclose(o);
    free(src), free(base), free(out), free(lengths);
    printf("%d pictures, %u segments: %s\n", N, groups, ok ? "clean" : "WROTE BEHIND A SCAN");
    return ok ? 0 : 1;
}

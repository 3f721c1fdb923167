// Baseline JPEG encoding on the device (include/gsr.h, "JPEG frames out"): N pictures of one size -> N entropy-coded scans that are
// libjpeg's bytes.  The arithmetic is libjpeg's integer path: 16-bit fixed-point colour conversion, box chroma downsampling with the
// alternating bias, the "islow" forward DCT of jfdctint.c (CONST_BITS 13, PASS1_BITS 2), division by (q << 3) with rounding half away
// from zero, the Annex K Huffman tables K.3 - K.6.  Edges: columns and rows are repeated up to the sampling factor, below that the last
// DOWNSAMPLED row is repeated; a luminance block of an MCU beyond ceil(W / 8) or ceil(H / 8) is a dummy -- zero AC and the DC of the
// block before it in the MCU, so it codes as "difference 0, end of block".
//
// Four launches, no atomics on global memory.  The coding order of a picture (MCU after MCU; in an MCU the Y blocks row-major, Cb, Cr)
// is cut into segments of JE_SEG_MCUS MCUs.
//   k_jpeg_enc_transform  one workgroup per segment: colour, downsampling, DCT, quantisation; zig-zag int16 coefficients with the DC
//                         already a difference (the first MCU of a segment keeps its DC: its predecessor is another workgroup's),
//                         bits per block, bits per segment, the DC of the segment's last MCU
//   k_jpeg_enc_scan       one workgroup per picture: the three open DC differences of every segment, then the bit offset of every segment
//   k_jpeg_enc_code       one workgroup per segment, one thread per block: an intra-workgroup scan places the blocks, the codes are ORed
//                         into LDS.  Segment joins are not byte-aligned, so a segment also codes the two blocks in front of it (>= 8 bits)
//                         and owns the bytes from the one its first bit lies in up to the one the next segment begins in: every byte it
//                         writes, and every 0xFF it counts, is a finished byte of the stream.
//   k_jpeg_enc_assemble   one workgroup per segment: its bytes to their final place with 0x00 after every 0xFF; the last adds the EOI.
#include <stdint.h>

#include "../../include/gsr.h"
#ifndef GSR_JPEG_ENC_HOST_SIM   // tools/jpeg_enc_host_sim.cpp compiles the kernels as plain C++ threads, with stand-ins for the HIP built-ins
#include <hip/hip_runtime.h>

#include "gsr_common.h"
#endif

namespace gsr {

constexpr int JE_SEG_MCUS = 16;
constexpr int JE_SEG_BLOCKS = 6 * JE_SEG_MCUS;                  // 4:2:0: four Y, Cb, Cr
constexpr int JE_BLOCK_BITS = 22 + 63 * 26;                     // DC: 11-bit code + 11 bits; AC: 16-bit code + 10 bits
constexpr int JE_THREADS = 256;
constexpr int JE_CODE_THREADS = 128;                            // >= JE_SEG_BLOCKS + 2
constexpr int JE_WORK = 72;                                     // ints of LDS per block in the DCT: 64 + 8, columns of 8 blocks on 64 banks
constexpr int JE_ZZ = 66;                                       // int16 of LDS per block of coefficients: 33 words, one thread per block
constexpr int JE_CODE_WORDS = ((JE_SEG_BLOCKS + 2) * JE_BLOCK_BITS + 7 + 31) / 32 + 2;
constexpr long long JE_MAX_BLOCKS = 2500000;                    // per picture: worst-case bits below 2^32, stream bound below 2^31

constexpr uint8_t je_dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t je_ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t je_dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t je_ac_vals[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};
constexpr uint8_t je_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// code << 5 | length per symbol, table 0 luminance, 1 chrominance; where: natural index -> zig-zag position
struct JeTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t where[64];
};

constexpr JeTables je_make_tables()
{
    JeTables t{};
    for (int tab = 0; tab < 2; ++tab)
        for (int kind = 0; kind < 2; ++kind) {
            const uint8_t *bits = kind ? je_ac_bits[tab] : je_dc_bits[tab];
            const uint8_t *vals = kind ? je_ac_vals[tab] : je_dc_vals;
            uint32_t *out = kind ? t.ac[tab] : t.dc[tab];
            uint32_t code = 0;
            int k = 0;
            for (int l = 1; l <= 16; ++l) {
                for (int i = 0; i < bits[l - 1]; ++i) out[vals[k++]] = (code++ << 5) | (uint32_t)l;
                code <<= 1;
            }
        }
    for (int k = 0; k < 64; ++k) t.where[je_zigzag[k]] = (uint8_t)k;
    return t;
}

__constant__ JeTables c_je = je_make_tables();

struct JeGeom {
    int H, W, hs, vs, ny, bpm;      // sampling factors of Y, Y blocks per MCU, blocks per MCU
    int mx, bw, bh;                 // MCUs per row; real Y blocks per row and per column
    uint32_t mcus, blocks, segs;    // per picture
};

struct JeQuant {
    uint16_t q[2][64];              // natural order, 1 .. 255
};

// block `k` of MCU `m`: its component (0 Y, 1 Cb, 2 Cr), its place in the component's block grid; true for a dummy luminance block
__device__ __forceinline__ bool je_block(const JeGeom &g, uint32_t m, int k, int &comp, int &by, int &bx)
{
    const int my = (int)(m / (uint32_t)g.mx), mxi = (int)(m - (uint32_t)my * (uint32_t)g.mx);
    if (k >= g.ny) {
        comp = 1 + k - g.ny, by = my, bx = mxi;
        return false;
    }
    const int v = k / g.hs, u = k - v * g.hs;
    comp = 0, by = my * g.vs + v, bx = mxi * g.hs + u;
    return by >= g.bh || bx >= g.bw;
}

template <int KIND>
__device__ __forceinline__ void je_rgb(const void *__restrict__ src, long long n, int y, int x, int H, int W, int &r, int &g, int &b)
{
    if (KIND == GSR_JPEG_ENC_SRC_U8) {
        const uint8_t *p = static_cast<const uint8_t *>(src) + ((n * H + y) * (long long)W + x) * 3;
        r = p[0], g = p[1], b = p[2];
    } else {
        const float *p = static_cast<const float *>(src) + (n * 3 * H + y) * (long long)W + x;
        const long long plane = (long long)H * W;
        const float v[3] = {p[0], p[plane], p[2 * plane]};
        int o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = v[c] != v[c] ? 0 : (int)(fminf(fmaxf(v[c], 0.0f), 1.0f) * 255.0f);   // export._rgb_bytes_host
        r = o[0], g = o[1], b = o[2];
    }
}

// one sample of a component's plane (for chroma: the downsampled plane), level-shifted
template <int KIND>
__device__ int je_sample(const void *__restrict__ src, long long n, const JeGeom &g, int comp, int y, int x)
{
    int r, gg, b;
    if (comp == 0) {
        je_rgb<KIND>(src, n, min(y, g.H - 1), min(x, g.W - 1), g.H, g.W, r, gg, b);
        return ((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) - 128;
    }
    y = min(y, (g.H + g.vs - 1) / g.vs - 1);                      // below the last downsampled row: that row again
    int sum = 0;
    for (int i = 0; i < g.vs; ++i)
        for (int j = 0; j < g.hs; ++j) {
            je_rgb<KIND>(src, n, min(g.vs * y + i, g.H - 1), min(g.hs * x + j, g.W - 1), g.H, g.W, r, gg, b);
            sum += comp == 1 ? (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16
                             : (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
        }
    if (g.hs == 2 && g.vs == 1) sum = (sum + (x & 1)) >> 1;       // bias 0, 1, 0, 1 ...
    if (g.hs == 2 && g.vs == 2) sum = (sum + 1 + (x & 1)) >> 2;   // bias 1, 2, 1, 2 ...
    return sum - 128;
}

// jfdctint.c, one pass over eight values: PASS 1 leaves the results scaled up by 4, PASS 2 removes that and the constants' 2^13
template <int PASS>
__device__ __forceinline__ void je_fdct8(int d[8])
{
    auto descale = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    constexpr int n = PASS == 1 ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (PASS == 1) d[0] = (t10 + t11) * 4, d[4] = (t10 - t11) * 4;
    else d[0] = descale(t10 + t11, 2), d[4] = descale(t10 - t11, 2);
    const int z = (t12 + t13) * 4433;
    d[2] = descale(z + t13 * 6270, n);
    d[6] = descale(z - t12 * 15137, n);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = -(t4 + t7) * 7373, z2 = -(t5 + t6) * 20995, z3 = -(t4 + t6) * 16069 + z5, z4 = -(t5 + t7) * 3196 + z5;
    d[7] = descale(t4 * 2446 + z1 + z3, n);
    d[5] = descale(t5 * 16819 + z2 + z4, n);
    d[3] = descale(t6 * 25172 + z2 + z3, n);
    d[1] = descale(t7 * 12299 + z1 + z4, n);
}

__device__ __forceinline__ int je_bit_length(int v) { return 32 - __clz(v < 0 ? -v : v); }   // 0 for 0

// exclusive sum of `v` over the workgroup's `n` threads (a power of two); `total` = the sum of all
__device__ __forceinline__ uint32_t je_scan(uint32_t v, uint32_t *sh, int n, uint32_t &total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < n; d <<= 1) {
        const uint32_t add = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[n - 1];
    const uint32_t r = sh[t] - v;
    __syncthreads();
    return r;
}

template <int KIND>
__global__ void __launch_bounds__(JE_THREADS) k_jpeg_enc_transform(const void *__restrict__ src, JeGeom g, JeQuant quant, int16_t *__restrict__ coef,
                                                                   uint16_t *__restrict__ bits, uint32_t *__restrict__ seg_bits,
                                                                   int16_t *__restrict__ seg_dc)
{
    __shared__ int work[JE_SEG_BLOCKS * JE_WORK];
    __shared__ uint32_t zz32[JE_SEG_BLOCKS * JE_ZZ / 2];
    __shared__ uint8_t ac_len[2][256], dc_len[2][16];
    __shared__ uint32_t total;
    int16_t *zz = reinterpret_cast<int16_t *>(zz32);
    const int t = threadIdx.x;
    const long long image = blockIdx.x / g.segs;
    const uint32_t seg = (uint32_t)(blockIdx.x - image * g.segs), m0 = seg * JE_SEG_MCUS;
    const int nm = (int)min((uint32_t)JE_SEG_MCUS, g.mcus - m0), nb = nm * g.bpm;

    for (int i = t; i < 512; i += JE_THREADS) ac_len[i >> 8][i & 255] = (uint8_t)(c_je.ac[i >> 8][i & 255] & 31u);
    if (t < 32) dc_len[t >> 4][t & 15] = (uint8_t)(c_je.dc[t >> 4][t & 15] & 31u);
    if (t == 0) total = 0u;

    // rows: one thread per row of a block
    for (int task = t; task < nb * 8; task += JE_THREADS) {
        const int b = task >> 3, r = task & 7, j = b / g.bpm, k = b - j * g.bpm;
        int comp, by, bx;
        if (je_block(g, m0 + j, k, comp, by, bx)) continue;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = je_sample<KIND>(src, image, g, comp, by * 8 + r, bx * 8 + i);
        je_fdct8<1>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) work[b * JE_WORK + r * 8 + i] = d[i];
    }
    __syncthreads();
    // columns, quantisation, zig-zag
    for (int task = t; task < nb * 8; task += JE_THREADS) {
        const int b = task >> 3, c = task & 7, j = b / g.bpm, k = b - j * g.bpm;
        int comp, by, bx;
        if (je_block(g, m0 + j, k, comp, by, bx)) {
#pragma unroll
            for (int i = 0; i < 8; ++i) zz[b * JE_ZZ + c * 8 + i] = 0;
            continue;
        }
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = work[b * JE_WORK + i * 8 + c];
        je_fdct8<2>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int div = (int)quant.q[comp ? 1 : 0][i * 8 + c] << 3, a = d[i] < 0 ? -d[i] : d[i];
            const int v = (a + (div >> 1)) / div;
            zz[b * JE_ZZ + c_je.where[i * 8 + c]] = (int16_t)(d[i] < 0 ? -v : v);
        }
    }
    __syncthreads();
    // a dummy block takes the DC of the block before it in the MCU (the first block of an MCU is never one)
    if (t < nm)
        for (int k = 1; k < g.ny; ++k) {
            int comp, by, bx;
            if (je_block(g, m0 + t, k, comp, by, bx)) zz[(t * g.bpm + k) * JE_ZZ] = zz[(t * g.bpm + k - 1) * JE_ZZ];
        }
    __syncthreads();
    // one thread per block: the bits of its code, the DC as a difference
    int dc = 0, pred = 0;
    bool open = false;
    uint32_t nbits = 0;
    const int j = t / g.bpm, k = t - j * g.bpm, tab = k >= g.ny ? 1 : 0;
    if (t < nb) {
        dc = zz[t * JE_ZZ];
        open = j == 0 && (k == 0 || k >= g.ny);                  // the predecessor is in the segment before
        if (!open) pred = (k > 0 && k < g.ny) ? zz[(t - 1) * JE_ZZ] : (k == 0 ? zz[((j - 1) * g.bpm + g.ny - 1) * JE_ZZ] : zz[(t - g.bpm) * JE_ZZ]);
        int run = 0;
        for (int i = 1; i < 64; ++i) {
            const int v = zz[t * JE_ZZ + i];
            if (v == 0) {
                ++run;
                continue;
            }
            const int n = je_bit_length(v) & 15;
            nbits += (uint32_t)(run >> 4) * ac_len[tab][0xF0] + ac_len[tab][((run & 15) << 4) | n] + n;
            run = 0;
        }
        if (run) nbits += ac_len[tab][0];
        if (!open) {
            const int n = je_bit_length(dc - pred) & 15;
            nbits += dc_len[tab][n] + n;
        }
    }
    __syncthreads();
    if (t < nb) {
        if (!open) zz[t * JE_ZZ] = (int16_t)(dc - pred);
        bits[(size_t)image * g.blocks + (size_t)m0 * g.bpm + t] = (uint16_t)nbits;
        atomicAdd(&total, nbits);
        if (j == nm - 1 && k >= g.ny - 1) seg_dc[((size_t)image * g.segs + seg) * 4 + (k - (g.ny - 1))] = (int16_t)dc;
    }
    __syncthreads();
    if (t == 0) seg_bits[(size_t)image * g.segs + seg] = total;
    uint32_t *__restrict__ out = reinterpret_cast<uint32_t *>(coef) + ((size_t)image * g.blocks + (size_t)m0 * g.bpm) * 32;
    for (int w = t; w < nb * 32; w += JE_THREADS) out[w] = zz32[(w >> 5) * (JE_ZZ / 2) + (w & 31)];
}

// one workgroup per picture: close the three open DC differences of every segment, then the bit offset of every segment
__global__ void __launch_bounds__(JE_THREADS) k_jpeg_enc_scan(JeGeom g, int16_t *__restrict__ coef, uint16_t *__restrict__ bits,
                                                              const uint32_t *__restrict__ seg_bits, const int16_t *__restrict__ seg_dc,
                                                              uint32_t *__restrict__ seg_off, uint32_t *__restrict__ image_bits)
{
    __shared__ uint32_t sh[JE_THREADS];
    const int t = threadIdx.x;
    const size_t image = blockIdx.x, s0 = image * g.segs, b0 = image * g.blocks;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < g.segs; base += JE_THREADS) {
        const uint32_t s = base + t;
        uint32_t v = 0;
        if (s < g.segs) {
            v = seg_bits[s0 + s];
            for (int c = 0; c < 3; ++c) {
                const size_t blk = b0 + (size_t)s * JE_SEG_MCUS * g.bpm + (c ? g.ny + c - 1 : 0);
                const int dc = coef[blk * 64], pred = s ? seg_dc[(s0 + s - 1) * 4 + c] : 0;
                const int n = je_bit_length(dc - pred) & 15;
                const uint32_t len = (c_je.dc[c ? 1 : 0][n] & 31u) + (uint32_t)n;
                coef[blk * 64] = (int16_t)(dc - pred);
                bits[blk] = (uint16_t)(bits[blk] + len);
                v += len;
            }
        }
        uint32_t total;
        const uint32_t before = je_scan(v, sh, JE_THREADS, total);
        if (s < g.segs) seg_off[s0 + s] = carry + before;
        carry += total;
    }
    if (t == 0) image_bits[image] = carry;
}

// `n` bits of `val` behind the `used` bits held at the top of `acc`; full words leave for the LDS string (most significant bit first)
__device__ __forceinline__ void je_put(uint32_t *buf, uint64_t &acc, int &used, uint32_t &word, uint32_t val, int n)
{
    if (n <= 0) return;
    acc |= (uint64_t)val << (64 - used - n);                      // used <= 31, n <= 26
    used += n;
    if (used >= 32) {
        if (word < (uint32_t)JE_CODE_WORDS) atomicOr(&buf[word], (uint32_t)(acc >> 32));
        ++word;
        acc <<= 32;
        used -= 32;
    }
}

__global__ void __launch_bounds__(JE_CODE_THREADS) k_jpeg_enc_code(JeGeom g, const int16_t *__restrict__ coef, const uint16_t *__restrict__ bits,
                                                                   const uint32_t *__restrict__ seg_off, const uint32_t *__restrict__ image_bits,
                                                                   uint8_t *__restrict__ raw, size_t raw_stride, uint32_t *__restrict__ seg_ff)
{
    __shared__ uint32_t buf[JE_CODE_WORDS];
    __shared__ uint32_t zz32[(JE_SEG_BLOCKS + 2) * JE_ZZ / 2];
    __shared__ uint32_t sh[JE_CODE_THREADS];
    __shared__ uint32_t dc_code[2][16], ac_code[2][256];
    __shared__ uint32_t ff;
    const int16_t *zz = reinterpret_cast<const int16_t *>(zz32);
    const int t = threadIdx.x;
    const size_t image = blockIdx.x / g.segs;
    const uint32_t seg = (uint32_t)(blockIdx.x - image * g.segs), m0 = seg * JE_SEG_MCUS;
    const int nm = (int)min((uint32_t)JE_SEG_MCUS, g.mcus - m0), lead = seg ? 2 : 0, nb = nm * g.bpm + lead;   // the Cb and Cr in front
    const uint32_t first = m0 * (uint32_t)g.bpm - (uint32_t)lead;                                               // first block coded, in the picture
    const bool last = seg == g.segs - 1;

    for (int i = t; i < 512; i += JE_CODE_THREADS) ac_code[i >> 8][i & 255] = c_je.ac[i >> 8][i & 255];
    if (t < 32) dc_code[t >> 4][t & 15] = c_je.dc[t >> 4][t & 15];
    for (int i = t; i < JE_CODE_WORDS; i += JE_CODE_THREADS) buf[i] = 0u;
    if (t == 0) ff = 0u;
    const uint32_t *__restrict__ from = reinterpret_cast<const uint32_t *>(coef) + (image * g.blocks + first) * 32;
    for (int w = t; w < nb * 32; w += JE_CODE_THREADS) zz32[(w >> 5) * (JE_ZZ / 2) + (w & 31)] = from[w];
    const uint32_t mine = t < nb ? bits[image * g.blocks + first + t] : 0u;
    uint32_t total;
    const uint32_t before = je_scan(mine, sh, JE_CODE_THREADS, total);   // (its barriers also publish the tables, the zeros and zz32)
    sh[t] = mine;
    __syncthreads();
    const uint32_t in_front = lead ? sh[0] + sh[1] : 0u;
    const uint32_t start = seg_off[image * g.segs + seg], end = last ? image_bits[image] : seg_off[image * g.segs + seg + 1];
    const uint32_t origin = (start - in_front) >> 3;              // byte of the stream that buf begins with
    if (t < nb) {
        const uint32_t at = ((start - in_front) & 7u) + before;
        uint64_t acc = 0;
        int used = (int)(at & 31u);
        uint32_t word = at >> 5;
        const int k = (int)((first + t) % (uint32_t)g.bpm), tab = k >= g.ny ? 1 : 0;
        const int diff = zz[t * JE_ZZ], n = je_bit_length(diff) & 15;
        je_put(buf, acc, used, word, dc_code[tab][n] >> 5, (int)(dc_code[tab][n] & 31u));
        je_put(buf, acc, used, word, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
        int run = 0;
        for (int i = 1; i < 64; ++i) {
            const int v = zz[t * JE_ZZ + i];
            if (v == 0) {
                ++run;
                continue;
            }
            for (; run > 15; run -= 16) je_put(buf, acc, used, word, ac_code[tab][0xF0] >> 5, (int)(ac_code[tab][0xF0] & 31u));
            const int m = je_bit_length(v) & 15;
            const uint32_t c = ac_code[tab][(run << 4) | m];
            je_put(buf, acc, used, word, c >> 5, (int)(c & 31u));
            je_put(buf, acc, used, word, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << m) - 1u), m);
            run = 0;
        }
        if (run) je_put(buf, acc, used, word, ac_code[tab][0] >> 5, (int)(ac_code[tab][0] & 31u));
        if (last && t == nb - 1) {                                // the last byte of the scan is filled with 1-bits
            const int pad = (int)((8u - (end & 7u)) & 7u);
            je_put(buf, acc, used, word, (1u << pad) - 1u, pad);
        }
        if (used && word < (uint32_t)JE_CODE_WORDS) atomicOr(&buf[word], (uint32_t)(acc >> 32));
    }
    __syncthreads();
    const uint32_t lo = (start >> 3) - origin, hi = (last ? (end + 7u) >> 3 : end >> 3) - origin;
    uint8_t *__restrict__ dst = raw + image * raw_stride + origin;
    uint32_t count = 0;
    for (uint32_t i = lo + t; i < hi; i += JE_CODE_THREADS) {
        const uint32_t byte = (buf[i >> 2] >> (24u - 8u * (i & 3u))) & 255u;
        dst[i] = (uint8_t)byte;
        count += byte == 255u ? 1u : 0u;
    }
    if (count) atomicAdd(&ff, count);
    __syncthreads();
    if (t == 0) seg_ff[image * g.segs + seg] = ff;
}

// one workgroup per segment: its bytes behind those of the segments before it, 0x00 after every 0xFF; the last one ends the scan
__global__ void __launch_bounds__(JE_THREADS) k_jpeg_enc_assemble(JeGeom g, const uint32_t *__restrict__ seg_off, const uint32_t *__restrict__ image_bits,
                                                                  const uint32_t *__restrict__ seg_ff, const uint8_t *__restrict__ raw, size_t raw_stride,
                                                                  uint8_t *__restrict__ out, size_t out_stride, int32_t *__restrict__ lengths)
{
    __shared__ uint32_t sh[JE_THREADS];
    __shared__ uint32_t before;
    const int t = threadIdx.x;
    const size_t image = blockIdx.x / g.segs;
    const uint32_t seg = (uint32_t)(blockIdx.x - image * g.segs);
    const bool last = seg == g.segs - 1;
    if (t == 0) before = 0u;
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t u = t; u < seg; u += JE_THREADS) sum += seg_ff[image * g.segs + u];
    if (sum) atomicAdd(&before, sum);
    __syncthreads();
    const uint32_t lo = seg_off[image * g.segs + seg] >> 3;
    const uint32_t hi = last ? (image_bits[image] + 7u) >> 3 : seg_off[image * g.segs + seg + 1] >> 3;
    const uint8_t *__restrict__ from = raw + image * raw_stride;
    uint8_t *__restrict__ dst = out + image * out_stride;
    uint32_t stuffed = before;
    for (uint32_t base = lo; base < hi; base += JE_THREADS * 8) {
        const uint32_t i0 = base + (uint32_t)t * 8u;
        uint32_t byte[8], count = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            byte[q] = i0 + q < hi ? from[i0 + q] : 0u;
            count += byte[q] == 255u ? 1u : 0u;
        }
        uint32_t total;
        uint32_t at = i0 + stuffed + je_scan(count, sh, JE_THREADS, total);
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q)
            if (i0 + q < hi) {
                dst[at++] = (uint8_t)byte[q];
                if (byte[q] == 255u) dst[at++] = 0u;
            }
        stuffed += total;
    }
    if (last && t == 0) {
        dst[hi + stuffed] = 0xff, dst[hi + stuffed + 1] = 0xd9;
        lengths[image] = (int32_t)(hi + stuffed + 2u);
    }
}

struct JePlan {
    JeGeom g;
    size_t off_bits, off_seg_bits, off_seg_off, off_seg_ff, off_seg_dc, off_image_bits, off_raw, raw_stride, scratch_bytes, bound;
};

// 0: fine, GSR_JPEG_ENC_TOO_LARGE, or GSR_EINVAL
inline int je_plan(int64_t N, int H, int W, int sampling, JePlan &p)
{
    if (N < 1 || N > (1LL << 24) || H < 1 || W < 1 || H > 65535 || W > 65535) return GSR_EINVAL;
    if (sampling != GSR_JPEG_444 && sampling != GSR_JPEG_422 && sampling != GSR_JPEG_420) return GSR_EINVAL;
    JeGeom &g = p.g;
    g.H = H, g.W = W;
    g.hs = sampling == GSR_JPEG_444 ? 1 : 2, g.vs = sampling == GSR_JPEG_420 ? 2 : 1;
    g.ny = g.hs * g.vs, g.bpm = g.ny + 2;
    g.mx = (W + 8 * g.hs - 1) / (8 * g.hs);
    const long long my = (H + 8 * g.vs - 1) / (8 * g.vs), mcus = (long long)g.mx * my, blocks = mcus * g.bpm;
    g.bw = (W + 7) / 8, g.bh = (H + 7) / 8;
    if (blocks > JE_MAX_BLOCKS) return GSR_JPEG_ENC_TOO_LARGE;
    const long long segs = (mcus + JE_SEG_MCUS - 1) / JE_SEG_MCUS;
    if (N * segs > 0x7fffffffLL) return GSR_JPEG_ENC_TOO_LARGE;
    g.mcus = (uint32_t)mcus, g.blocks = (uint32_t)blocks, g.segs = (uint32_t)segs;
    const size_t raw = ((size_t)blocks * JE_BLOCK_BITS + 7) / 8;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    p.bound = 2 * raw + 2;
    p.raw_stride = up(raw);
    p.off_bits = up((size_t)N * blocks * 64 * sizeof(int16_t));
    p.off_seg_bits = p.off_bits + up((size_t)N * blocks * sizeof(uint16_t));
    p.off_seg_off = p.off_seg_bits + up((size_t)N * segs * sizeof(uint32_t));
    p.off_seg_ff = p.off_seg_off + up((size_t)N * segs * sizeof(uint32_t));
    p.off_seg_dc = p.off_seg_ff + up((size_t)N * segs * sizeof(uint32_t));
    p.off_image_bits = p.off_seg_dc + up((size_t)N * segs * 4 * sizeof(int16_t));
    p.off_raw = p.off_image_bits + up((size_t)N * sizeof(uint32_t));
    p.scratch_bytes = p.off_raw + (size_t)N * p.raw_stride;
    return GSR_OK;
}

}  // namespace gsr

#ifndef GSR_JPEG_ENC_HOST_SIM
extern "C" {

__attribute__((visibility("default"))) size_t gsr_jpeg_enc_scratch_bytes(int64_t N, int H, int W, int sampling)
{
    gsr::JePlan p;
    return gsr::je_plan(N, H, W, sampling, p) == GSR_OK ? p.scratch_bytes : 0;
}

__attribute__((visibility("default"))) size_t gsr_jpeg_enc_stream_bound(int H, int W, int sampling)
{
    gsr::JePlan p;
    return gsr::je_plan(1, H, W, sampling, p) == GSR_OK ? p.bound : 0;
}

__attribute__((visibility("default"))) int gsr_jpeg_enc_scans(const void *src, int src_kind, int64_t N, int H, int W, int sampling, const uint16_t *quant,
                                                              void *scratch, size_t scratch_bytes, uint8_t *out, size_t out_stride, int32_t *lengths,
                                                              void *stream)
{
    using namespace gsr;
    JePlan p;
    if (!src || !quant || !scratch || !out || !lengths) return GSR_EINVAL;
    if (src_kind != GSR_JPEG_ENC_SRC_U8 && src_kind != GSR_JPEG_ENC_SRC_F32_PLANAR) return GSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) || (reinterpret_cast<uintptr_t>(lengths) & 3)) return GSR_EINVAL;
    if (src_kind == GSR_JPEG_ENC_SRC_F32_PLANAR && (reinterpret_cast<uintptr_t>(src) & 3)) return GSR_EINVAL;
    JeQuant q;
    for (int i = 0; i < 128; ++i) {
        if (quant[i] < 1 || quant[i] > 255) return GSR_EINVAL;
        q.q[i >> 6][i & 63] = quant[i];
    }
    const int rc = je_plan(N, H, W, sampling, p);
    if (rc != GSR_OK) return rc;
    if (scratch_bytes < p.scratch_bytes) return GSR_ENOSPACE;
    if (out_stride < p.bound || out_stride > 0x7fffffffULL) return GSR_EINVAL;
    uint8_t *base = static_cast<uint8_t *>(scratch);
    int16_t *coef = reinterpret_cast<int16_t *>(base);
    uint16_t *bits = reinterpret_cast<uint16_t *>(base + p.off_bits);
    uint32_t *seg_bits = reinterpret_cast<uint32_t *>(base + p.off_seg_bits), *seg_off = reinterpret_cast<uint32_t *>(base + p.off_seg_off);
    uint32_t *seg_ff = reinterpret_cast<uint32_t *>(base + p.off_seg_ff), *image_bits = reinterpret_cast<uint32_t *>(base + p.off_image_bits);
    int16_t *seg_dc = reinterpret_cast<int16_t *>(base + p.off_seg_dc);
    uint8_t *raw = base + p.off_raw;
    const unsigned groups = (unsigned)(N * p.g.segs);
    hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (src_kind == GSR_JPEG_ENC_SRC_U8)
        hipLaunchKernelGGL(k_jpeg_enc_transform<GSR_JPEG_ENC_SRC_U8>, dim3(groups), dim3(JE_THREADS), 0, s, src, p.g, q, coef, bits, seg_bits, seg_dc);
    else
        hipLaunchKernelGGL(k_jpeg_enc_transform<GSR_JPEG_ENC_SRC_F32_PLANAR>, dim3(groups), dim3(JE_THREADS), 0, s, src, p.g, q, coef, bits, seg_bits,
                           seg_dc);
    hipLaunchKernelGGL(k_jpeg_enc_scan, dim3((unsigned)N), dim3(JE_THREADS), 0, s, p.g, coef, bits, seg_bits, seg_dc, seg_off, image_bits);
    hipLaunchKernelGGL(k_jpeg_enc_code, dim3(groups), dim3(JE_CODE_THREADS), 0, s, p.g, coef, bits, seg_off, image_bits, raw, p.raw_stride, seg_ff);
    hipLaunchKernelGGL(k_jpeg_enc_assemble, dim3(groups), dim3(JE_THREADS), 0, s, p.g, seg_off, image_bits, seg_ff, raw, p.raw_stride, out, out_stride,
                       lengths);
    return launch_status();
}

}  // extern "C"
#endif

// gsr_jpeg.hip -- JPEG frames: the C ABI of the host entropy stage (gsr_jpeg_entropy.h) and the device stage that turns its
// coefficient blocks into the interleaved RGB bytes gsr_resample_crop reads.  All arithmetic is integer and exact; the oracle is the
// bytes of libjpeg-turbo (JDCT_ISLOW, fancy upsampling), which the reference's loader gets from PIL (include/gsr.h has the rules).
//
// Two launches:
//   k_jpeg_idct    dequantise + 8 x 8 "islow" IDCT + range limit -> byte planes of the components, in their whole-MCU block grids.
//                  Eight lanes own one block, a wave eight blocks, a 256-thread group 32 consecutive blocks of one image.  A lane
//                  loads ROW r of the block as one 16-byte load (a wave reads 1 KiB contiguous), multiplies by the table row and
//                  parks the eight products in LDS; it then owns COLUMN c for pass 1, writes the column back in place, and owns ROW r
//                  again for pass 2, whose eight bytes leave as one 8-byte store.  The block's LDS tile is 8 rows of 9 dwords: the
//                  pad makes the column walk conflict-free (4 blocks of a half-wave sit 72 dwords apart: banks 0, 8, 16, 24 + c).
//                  The two transposes go through LDS, not cross-lane moves: 8 ds_bpermute per pass, each with a per-lane choice of
//                  the register to send and to fill, cost more than 8 ds_write + 8 ds_read, and the kernel is bound by its
//                  2-byte-in / 1-byte-out traffic anyway.
//   k_jpeg_colour  chroma upsampling + YCbCr -> RGB.  The output (N,H,W,3) is walked FLAT, four pixels = twelve bytes per thread (the
//                  scheme of gsr_undistort.hip), so that stores are dense across the wave whatever W is; only the call's last group
//                  can be partial.  Every pixel gathers its luma byte and the two or four chroma bytes its filter taps from the planes,
//                  which the first launch left in L2.
// No atomics, no host sync, vector stores only; every output byte is written exactly once.  The descriptors come from the caller:
// each image's class, grids and offsets are checked on the device (jp_image) before an address is formed from them, and an image
// that fails -- or that the entropy stage marked as not decoded -- is written as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"
#include "gsr_jpeg_entropy.h"

namespace gsr {

constexpr int JP_THREADS = 256;
constexpr int JP_GROUP_BLOCKS = JP_THREADS / 8;   // 8 x 8 blocks per thread group
constexpr int JP_TILE = 72;                       // dwords of LDS per block: 8 rows of 8 + 1
constexpr int JP_MAX_GROUPS = 4096;               // k_jpeg_colour: grid-stride above this

struct JpImage {
    bool valid;
    int sampling;
    int32_t bw[3], bh[3];
    long long plane[3];   // first value / byte of each component, from the start of the buffers
    long long blocks;     // all components
};

// the descriptor of image n, believed only as far as it agrees with (H, W) and stays inside `capacity` values
__device__ __forceinline__ JpImage jp_image(const gsr_jpeg_desc *__restrict__ desc, long long n, int H, int W, long long capacity)
{
    const gsr_jpeg_desc *__restrict__ d = desc + n;
    JpImage g;
    g.sampling = d->sampling;
    g.valid = g.sampling >= GSR_JPEG_GRAY && g.sampling <= GSR_JPEG_420;
    g.blocks = gsr_jpeg::block_grids(g.valid ? g.sampling : GSR_JPEG_GRAY, H, W, g.bw, g.bh) / 64;
    const long long off = d->coef_offset;
    g.valid = g.valid && off >= 0 && (off & 63) == 0 && off <= capacity - 64 * g.blocks && d->coef_count == 64 * g.blocks;
#pragma unroll
    for (int c = 0; c < 3; ++c) g.valid = g.valid && d->bw[c] == g.bw[c] && d->bh[c] == g.bh[c];
    g.plane[0] = off;
    g.plane[1] = off + 64LL * g.bw[0] * g.bh[0];
    g.plane[2] = g.plane[1] + 64LL * g.bw[1] * g.bh[1];
    return g;
}

// one 8-point pass of the "islow" IDCT (13-bit constants), outputs descaled by `shift` with rounding.  Inside the coefficient gate no
// intermediate leaves 32 bits.
template <int SHIFT>
__device__ __forceinline__ void jp_idct8(const int in[8], int out[8])
{
    int z1 = (in[2] + in[6]) * 4433;
    int tmp2 = z1 + in[6] * -15137;
    int tmp3 = z1 + in[2] * 6270;
    int tmp0 = (in[0] + in[4]) * 8192;
    int tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    int z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    out[0] = (tmp10 + tmp3 + R) >> SHIFT;
    out[7] = (tmp10 - tmp3 + R) >> SHIFT;
    out[1] = (tmp11 + tmp2 + R) >> SHIFT;
    out[6] = (tmp11 - tmp2 + R) >> SHIFT;
    out[2] = (tmp12 + tmp1 + R) >> SHIFT;
    out[5] = (tmp12 - tmp1 + R) >> SHIFT;
    out[3] = (tmp13 + tmp0 + R) >> SHIFT;
    out[4] = (tmp13 - tmp0 + R) >> SHIFT;
}

__device__ __forceinline__ uint32_t jp_range_limit(int v)
{
    int s = v & 1023;
    s = s >= 512 ? s - 1024 : s;
    s += 128;
    return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

struct __attribute__((aligned(16))) JpRow16 {
    int16_t v[8];
};
struct __attribute__((aligned(16))) JpRowU16 {
    uint16_t v[8];
};

// grid: N * groups_per_image thread groups; group g of image n takes blocks [32 g, 32 g + 32) of the image's block list (component after
// component).  groups_per_image covers the largest class, so the groups behind a smaller image's list have nothing to do.
__global__ void __launch_bounds__(JP_THREADS) k_jpeg_idct(const int16_t *__restrict__ coefs, const gsr_jpeg_desc *__restrict__ desc, int H, int W,
                                                           int groups_per_image, long long capacity, uint8_t *__restrict__ planes)
{
    __shared__ int tile[JP_GROUP_BLOCKS * JP_TILE];
    const long long n = blockIdx.x / groups_per_image;
    const int group = (int)(blockIdx.x - n * groups_per_image);
    const JpImage img = jp_image(desc, n, H, W, capacity);
    const int local = threadIdx.x >> 3, k = threadIdx.x & 7;   // k: the row of the load and of pass 2, the column of pass 1
    const long long blk = (long long)group * JP_GROUP_BLOCKS + local;
    const bool live = img.valid && blk < img.blocks;
    const long long n0 = (long long)img.bw[0] * img.bh[0], n1 = (long long)img.bw[1] * img.bh[1];
    const int comp = blk < n0 ? 0 : (blk < n0 + n1 ? 1 : 2);
    const long long in_comp = blk - (comp == 0 ? 0 : (comp == 1 ? n0 : n0 + n1));
    // selects, not indexed reads: an array of the descriptor indexed by `comp` would live in scratch memory
    const long long plane = comp == 0 ? img.plane[0] : (comp == 1 ? img.plane[1] : img.plane[2]);
    const int bwc = comp == 0 ? img.bw[0] : img.bw[1];
    int *__restrict__ t = tile + local * JP_TILE;
    if (live) {
        const JpRow16 c = *reinterpret_cast<const JpRow16 *>(coefs + plane + 64 * in_comp + 8 * k);
        const JpRowU16 q = *reinterpret_cast<const JpRowU16 *>(&desc[n].quant[comp][8 * k]);
#pragma unroll
        for (int j = 0; j < 8; ++j) t[9 * k + j] = (int)c.v[j] * (int)q.v[j];
    }
    __syncthreads();
    if (live) {
        int col[8], ws[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) col[r] = t[9 * r + k];
        jp_idct8<11>(col, ws);
#pragma unroll
        for (int r = 0; r < 8; ++r) t[9 * r + k] = ws[r];   // its own column: no other lane reads or writes these
    }
    __syncthreads();
    if (live) {
        int row[8], px[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = t[9 * k + j];
        jp_idct8<18>(row, px);
        uint2 bytes;
        bytes.x = jp_range_limit(px[0]) | (jp_range_limit(px[1]) << 8) | (jp_range_limit(px[2]) << 16) | (jp_range_limit(px[3]) << 24);
        bytes.y = jp_range_limit(px[4]) | (jp_range_limit(px[5]) << 8) | (jp_range_limit(px[6]) << 16) | (jp_range_limit(px[7]) << 24);
        const long long by = in_comp / bwc, bx = in_comp - by * bwc;
        // plane row by * 8 + k, byte bx * 8: inside the plane because in_comp < bw * bh; 8-byte aligned because planes start on 64
        *reinterpret_cast<uint2 *>(planes + plane + ((by * 8 + k) * bwc + bx) * 8) = bytes;
    }
}

struct JpPlanes {
    bool valid;
    int sampling, pitch0, pitchc, cw, ch;
    const uint8_t *y, *cb, *cr;
};

__device__ __forceinline__ JpPlanes jp_planes(const gsr_jpeg_desc *__restrict__ desc, long long n, int H, int W, long long capacity,
                                              const uint8_t *__restrict__ planes)
{
    const JpImage img = jp_image(desc, n, H, W, capacity);
    JpPlanes p;
    p.valid = img.valid;
    p.sampling = img.sampling;
    p.pitch0 = img.bw[0] * 8;
    p.pitchc = img.bw[1] * 8;
    p.cw = img.sampling == GSR_JPEG_444 ? W : (W + 1) >> 1;
    p.ch = img.sampling == GSR_JPEG_420 ? (H + 1) >> 1 : H;
    p.y = planes + img.plane[0];
    p.cb = planes + img.plane[1];
    p.cr = planes + img.plane[2];
    return p;
}

// one chroma sample at full resolution.  x < W and y < H keep every tap inside the plane: the plane holds at least cw columns and ch rows.
__device__ __forceinline__ int jp_chroma(const uint8_t *__restrict__ c, const JpPlanes &p, int x, int y)
{
    if (p.sampling == GSR_JPEG_444) return c[(long long)y * p.pitchc + x];
    const int i = x >> 1, odd = x & 1, last = p.cw - 1;
    if (p.sampling == GSR_JPEG_422) {
        const uint8_t *__restrict__ row = c + (long long)y * p.pitchc;
        if (p.cw <= 2) return row[i];
        if (odd) return i == last ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
        return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const uint8_t *__restrict__ row = c + (long long)r * p.pitchc;
    if (p.cw <= 2) return row[i];
    int nr = (y & 1) ? r + 1 : r - 1;
    nr = nr < 0 ? 0 : (nr > p.ch - 1 ? p.ch - 1 : nr);
    const uint8_t *__restrict__ near = c + (long long)nr * p.pitchc;
    const int cs = 3 * row[i] + near[i];
    if (odd) return i == last ? (4 * cs + 7) >> 4 : (3 * cs + 3 * row[i + 1] + near[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * row[i - 1] + near[i - 1] + 8) >> 4;
}

__device__ __forceinline__ uint32_t jp_byte(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// one output pixel -> R | G << 8 | B << 16
__device__ __forceinline__ uint32_t jp_pixel(const JpPlanes &p, int x, int y)
{
    if (!p.valid) return 0u;
    const int Y = p.y[(long long)y * p.pitch0 + x];
    if (p.sampling == GSR_JPEG_GRAY) return (uint32_t)Y * 0x010101u;
    const int cb = jp_chroma(p.cb, p, x, y) - 128, cr = jp_chroma(p.cr, p, x, y) - 128;
    const int R = Y + ((91881 * cr + 32768) >> 16);
    const int G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int B = Y + ((116130 * cb + 32768) >> 16);
    return jp_byte(R) | (jp_byte(G) << 8) | (jp_byte(B) << 16);
}

struct __attribute__((aligned(4))) JpWords {
    uint32_t w[3];
};

__global__ void __launch_bounds__(JP_THREADS) k_jpeg_colour(const uint8_t *__restrict__ planes, const gsr_jpeg_desc *__restrict__ desc, long long N,
                                                             int H, int W, long long capacity, uint8_t *__restrict__ out)
{
    const long long per_image = (long long)H * W, n_pixels = per_image * N, n_groups = (n_pixels + 3) >> 2;
    for (long long g = (long long)blockIdx.x * JP_THREADS + threadIdx.x; g < n_groups; g += (long long)gridDim.x * JP_THREADS) {
        const long long first = g * 4;
        long long n = first / per_image;
        const int rem = (int)(first - n * per_image);
        int y = rem / W, x = rem - y * W;
        JpPlanes p = jp_planes(desc, n, H, W, capacity, planes);
        const int live = n_pixels - first >= 4 ? 4 : (int)(n_pixels - first);
        uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < live) {
                px[q] = jp_pixel(p, x, y);
                if (++x == W) {
                    x = 0;
                    if (++y == H) {
                        y = 0;
                        if (++n < N) p = jp_planes(desc, n, H, W, capacity, planes);
                    }
                }
            }
        }
        uint8_t *__restrict__ o = out + first * 3;
        if (live == 4) {
            JpWords w;
            w.w[0] = px[0] | (px[1] << 24);
            w.w[1] = (px[1] >> 8) | (px[2] << 16);
            w.w[2] = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<JpWords *>(o) = w;
        } else {
            for (int q = 0; q < live; ++q) {
                o[3 * q] = (uint8_t)px[q];
                o[3 * q + 1] = (uint8_t)(px[q] >> 8);
                o[3 * q + 2] = (uint8_t)(px[q] >> 16);
            }
        }
    }
}

inline bool jp_dims_ok(int64_t N, int H, int W) { return N >= 1 && N <= (1LL << 24) && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) int gsr_jpeg_probe(const uint8_t *data, size_t len, gsr_jpeg_info *info)
{
    return gsr_jpeg::probe(data, len, info);
}

__attribute__((visibility("default"))) size_t gsr_jpeg_coef_bytes(int64_t N, int H, int W)
{
    if (!gsr::jp_dims_ok(N, H, W)) return 0;
    return (size_t)N * (size_t)gsr_jpeg::max_image_coefs(H, W) * sizeof(int16_t);
}

__attribute__((visibility("default"))) int gsr_jpeg_entropy(const uint8_t *const *data, const size_t *len, int64_t N, int H, int W, int16_t *coefs,
                                                            gsr_jpeg_desc *desc, int32_t *status, int threads)
{
    return gsr_jpeg::entropy(data, len, N, H, W, coefs, desc, status, threads);
}

__attribute__((visibility("default"))) size_t gsr_jpeg_scratch_bytes(int64_t N, int H, int W)
{
    if (!gsr::jp_dims_ok(N, H, W)) return 0;
    return (size_t)N * (size_t)gsr_jpeg::max_image_coefs(H, W);   // one byte per coefficient
}

__attribute__((visibility("default"))) int gsr_jpeg_pixels(const int16_t *coefs_dev, const gsr_jpeg_desc *desc_dev, int64_t N, int H, int W,
                                                           void *scratch, size_t scratch_bytes, uint8_t *out, void *stream)
{
    using namespace gsr;
    if (!coefs_dev || !desc_dev || !scratch || !out || !jp_dims_ok(N, H, W)) return GSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(coefs_dev) & 15) || (reinterpret_cast<uintptr_t>(desc_dev) & 15) || (reinterpret_cast<uintptr_t>(scratch) & 15) ||
        (reinterpret_cast<uintptr_t>(out) & 3))
        return GSR_EINVAL;
    const long long max_blocks = gsr_jpeg::max_image_coefs(H, W) / 64, capacity = (long long)N * max_blocks * 64;
    if (scratch_bytes < (size_t)capacity) return GSR_ENOSPACE;
    const long long groups_per_image = (max_blocks + JP_GROUP_BLOCKS - 1) / JP_GROUP_BLOCKS;
    if (groups_per_image * N > 0x7fffffffLL) return GSR_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)(groups_per_image * N)), dim3(JP_THREADS), 0, s, coefs_dev, desc_dev, H, W, (int)groups_per_image,
                       capacity, static_cast<uint8_t *>(scratch));
    const long long groups = ((long long)N * H * W + 3) >> 2, blocks = (groups + JP_THREADS - 1) / JP_THREADS;
    hipLaunchKernelGGL(k_jpeg_colour, dim3((unsigned)(blocks < JP_MAX_GROUPS ? blocks : JP_MAX_GROUPS)), dim3(JP_THREADS), 0, s,
                       static_cast<const uint8_t *>(scratch), desc_dev, (long long)N, H, W, capacity, out);
    return launch_status();
}

}  // extern "C"

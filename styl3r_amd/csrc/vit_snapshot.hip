// vit_snapshot.hip -- the device half of a checkpoint (styl3r_amd/checkpointing.py): every tensor of the training state (1 806 at full size,
// 4.4 GB of weights, 13.2 GB with the two AdamW moments) leaves the train stream in ONE launch.  A device table of chunks {src, byte offset
// in the staging buffer, nbytes <= 64 KiB of ONE tensor, flags} -- the layout idea of VitAdamChunk in vit_optim.hip -- gives each workgroup
// one chunk: it copies the bytes exactly into `staging` and writes one partial record {s1, s2, nonfinite} for them.  After the launch the
// train step may overwrite the sources; one device-to-host copy of `staging` on a side stream and a writer thread do the rest.
//
//   s1 = sum w_i, s2 = sum (i + 1) w_i   (mod 2^64) over the chunk's little-endian 32-bit words w_i, i local to the chunk, a final partial word
//   zero-extended; nonfinite = words whose fp32 exponent field is all ones, counted only for a chunk flagged VIT_SNAP_FP32.
// The host folds the partials of a tensor: S1 = sum s1_c, S2 = sum (s2_c + base_c s1_c) with base_c the word index of the chunk's start.  Integer
// sums only, no atomics: the record of a chunk does not depend on the order the lanes are reduced in, so two runs agree bit for bit.
//
// HBM-bound: one read and one write per byte (measured: 1.64 ms for 4.4 GB, 5.4 TB/s read + write; DESIGN R27).  Lane shape as in k_adamw: 16-byte loads and stores when the source is 16-byte aligned (the
// destination always is: tensors start at multiples of 64 bytes in `staging`, chunks at multiples of the chunk size behind that), four
// independent loads per lane in flight before the first store; 4-byte words for a source that is only word aligned (the 0-dim step
// counters of the optimizer, views that start inside a storage), bytes for the rest.  The bytes between the end of one tensor and the start
// of the next are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_common.h"
#include "vit_internal.h"

namespace vit {
namespace {
constexpr uint32_t kChunkBytes = 64u << 10;
constexpr int kThreads = 256;
// the sources come out of the table as generic pointers; they are device memory, and saying so turns the flat loads into global ones
template <class T> using global_ptr = const T __attribute__((address_space(1))) *;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));          // 16 bytes, one load / store

struct Acc {
    uint64_t s1 = 0, s2 = 0;
    uint32_t bad = 0;
    bool fp32;
    __device__ inline void word(uint32_t w, uint32_t index)          // index: the word's position inside the chunk
    {
        s1 += w;
        s2 += (uint64_t)(index + 1u) * w;
        if (fp32) bad += (w & 0x7f800000u) == 0x7f800000u;
    }
    __device__ inline void quad(const u32x4 &q, uint32_t v)          // v: index of the 16-byte vector
    {
        word(q.x, 4u * v); word(q.y, 4u * v + 1u); word(q.z, 4u * v + 2u); word(q.w, 4u * v + 3u);
    }
};

__global__ void __launch_bounds__(kThreads) k_snapshot_pack(const VitSnapChunk *__restrict__ chunks, uint8_t *__restrict__ staging,
                                                            VitSnapPartial *__restrict__ partials)
{
    const VitSnapChunk ch = chunks[blockIdx.x];
    const global_ptr<uint8_t> src = (global_ptr<uint8_t>)ch.src;
    uint8_t *dst = staging + ch.dst_off;
    const uint32_t nbytes = ch.nbytes, nwords = nbytes >> 2, tid = threadIdx.x;
    Acc a;
    a.fp32 = (ch.flags & VIT_SNAP_FP32) != 0;
    uint32_t done = 0;                                               // words copied by the wide paths
    if (ch.flags & VIT_SNAP_VEC16) {
        const global_ptr<u32x4> s4 = (global_ptr<u32x4>)ch.src;
        u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
        const uint32_t n4 = nbytes >> 4;
        uint32_t i = tid;
        for (; i + 3 * kThreads < n4; i += 4 * kThreads) {          // four 16-byte loads in flight per lane
            const u32x4 q0 = s4[i], q1 = s4[i + kThreads], q2 = s4[i + 2 * kThreads], q3 = s4[i + 3 * kThreads];
            d4[i] = q0; d4[i + kThreads] = q1; d4[i + 2 * kThreads] = q2; d4[i + 3 * kThreads] = q3;
            a.quad(q0, i); a.quad(q1, i + kThreads); a.quad(q2, i + 2 * kThreads); a.quad(q3, i + 3 * kThreads);
        }
        for (; i < n4; i += kThreads) {
            const u32x4 q = s4[i];
            d4[i] = q;
            a.quad(q, i);
        }
        done = n4 << 2;
    }
    if (ch.flags & (VIT_SNAP_VEC16 | VIT_SNAP_WORD)) {               // whole words (all of them, or what the vectors left)
        const global_ptr<uint32_t> sw = (global_ptr<uint32_t>)ch.src;
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst);
        for (uint32_t j = done + tid; j < nwords; j += kThreads) {
            const uint32_t w = sw[j];
            dw[j] = w;
            a.word(w, j);
        }
        const uint32_t tail = nbytes & 3u;                           // the final partial word, byte by byte, zero-extended
        if (tail && tid == 0) {
            uint32_t w = 0;
            for (uint32_t b = 0; b < tail; ++b) {
                const uint8_t x = src[4u * nwords + b];
                dst[4u * nwords + b] = x;
                w |= (uint32_t)x << (8u * b);
            }
            a.word(w, nwords);
        }
    } else {                                                         // a source that is not even word aligned: bytes
        const uint32_t nw = (nbytes + 3u) >> 2;
        for (uint32_t j = tid; j < nw; j += kThreads) {
            uint32_t w = 0;
            for (uint32_t b = 0; b < 4u && 4u * j + b < nbytes; ++b) {
                const uint8_t x = src[4u * j + b];
                dst[4u * j + b] = x;
                w |= (uint32_t)x << (8u * b);
            }
            a.word(w, j);
        }
    }
    // workgroup sums (integers: any order gives the same bits)
    for (int off = 32; off > 0; off >>= 1) {
        a.s1 += __shfl_down((unsigned long long)a.s1, off, 64);
        a.s2 += __shfl_down((unsigned long long)a.s2, off, 64);
        a.bad += __shfl_down(a.bad, off, 64);
    }
    __shared__ uint64_t l1[kThreads / 64], l2[kThreads / 64];
    __shared__ uint32_t lb[kThreads / 64];
    if ((tid & 63u) == 0) { l1[tid >> 6] = a.s1; l2[tid >> 6] = a.s2; lb[tid >> 6] = a.bad; }
    __syncthreads();
    if (tid == 0) {
        VitSnapPartial out;
        out.s1 = l1[0] + l1[1] + l1[2] + l1[3];
        out.s2 = l2[0] + l2[1] + l2[2] + l2[3];
        out.nonfinite = lb[0] + lb[1] + lb[2] + lb[3];
        out.reserved = 0;
        partials[blockIdx.x] = out;
    }
}
}  // namespace

size_t snapshot_chunk_bytes() { return kChunkBytes; }

int snapshot_pack(const VitSnapChunk *chunks, int n_chunks, void *staging, VitSnapPartial *partials, hipStream_t stream)
{
    if (n_chunks == 0) return VIT_OK;
    if (!chunks || n_chunks < 0 || !staging || !partials) return VIT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(staging) & 63u) || (reinterpret_cast<uintptr_t>(partials) & 7u)) return VIT_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_snapshot_pack, dim3(n_chunks), dim3(kThreads), 0, stream, chunks, static_cast<uint8_t *>(staging), partials);
    return launch_status();
}
}  // namespace vit

// PNG encoding on the device (include/gsr.h, "PNG frames"): k_png_chunks codes one chunk of whole rows per workgroup -- filter, byte-run
// tokens, length-limited Huffman codes, one dynamic deflate block or one stored block -- and k_png_assemble strings the chunks of every
// image into its zlib stream.  styl3r_amd/image_io.py restates every step in integers on the host; the two give the same bytes.
//
// The Huffman construction, stated exactly (image_io.code_lengths is the same text in Python):
//   1. the used symbols (count > 0) in ascending order of (count, symbol) are the leaves 0 .. m-1; one used symbol gets length 1;
//   2. m - 1 times: take the two smallest of (next unmerged leaf, next unmerged node) -- a leaf wins against a node of equal weight --
//      and make them children of a new node whose weight is their sum; nodes are created, and consumed, in order;
//   3. num[d] = how many leaves are d edges below the root, depths above the limit counted at the limit (then the limit "acted");
//   4. if it acted, with total = sum(num[d] << (limit - d)): until total == 1 << limit: num[limit] -= 1; the largest d < limit with
//      num[d] > 0 gives num[d] -= 1, num[d + 1] += 2; total -= 1;
//   5. lengths are handed out by rank: the num[1] leaves of largest (count, symbol) get length 1, the next num[2] get 2, ...
// Codes are deflate's canonical codes.  Every bit of the output is placed with LDS atomics and leaves the workgroup in vector stores.
#include <stdint.h>

#include "../../include/gsr.h"
#ifndef GSR_PNG_HOST_SIM   // tools/png_kernel_host_sim.cpp compiles the kernels as plain C++ threads, with stand-ins for the HIP built-ins
#include <hip/hip_runtime.h>

#include "gsr_common.h"
#endif

namespace gsr {

constexpr int PNG_THREADS = 256;
constexpr int PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_LL = 286;              // literal / length symbols sent (HLIT = 29)
constexpr int PNG_SEQ = PNG_LL + 1;      // code lengths sent: 286 literal / length + 1 distance
constexpr int PNG_CL = 19;
constexpr int PNG_SYMS = 288;            // room per symbol table
constexpr int PNG_BIT_WORDS = GSR_PNG_SLOT_BYTES / 4;
constexpr uint32_t PNG_ADLER = 65521u;
constexpr int PNG_META = 4;              // int32 per chunk: payload bytes, Adler s1, s2, filtered bytes

struct PngShared {
    uint32_t bits[PNG_BIT_WORDS];        // the coded block, bit by bit
    uint8_t filt[GSR_PNG_CHUNK_BYTES];   // the chunk's filtered bytes
    uint32_t hist[PNG_SYMS];             // counts of the literal / length symbols; [286]: matches (= uses of distance code 0)
    uint32_t weight[2 * PNG_SYMS];       // leaves in sorted order, then the nodes
    uint16_t parent[2 * PNG_SYMS];
    uint16_t order[PNG_SYMS];            // sorted position -> symbol
    uint16_t code[PNG_SYMS];             // bit-reversed canonical codes
    uint8_t len[PNG_SYMS];               // [0, 286): literal / length code lengths, [286]: the distance code's
    uint16_t cl_tok[PNG_SYMS];           // code-length tokens: symbol | extra value << 5
    uint32_t cl_hist[PNG_CL + 1];
    uint16_t cl_code[PNG_CL + 1];
    uint8_t cl_len[PNG_CL + 1];
    uint32_t num[16], cum[16], next_code[16];
    int16_t first_start[PNG_THREADS], last_start[PNG_THREADS];   // n <= 16384
    int used, acted, n_cl_tok, hclen;
    uint32_t header_bits, s1, s2;
};

__constant__ uint8_t c_png_cl_order[PNG_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one raw byte of the picture: j in [0, W * C) along row y of image n
template <int KIND>
__device__ __forceinline__ int png_raw(const void *__restrict__ src, long long n, int y, int j, int H, int W, int Cn)
{
    if (KIND == GSR_PNG_SRC_U8) return static_cast<const uint8_t *>(src)[((n * H + y) * W) * Cn + j];
    const int x = j / Cn, c = j - x * Cn;
    const float v = static_cast<const float *>(src)[((n * Cn + c) * H + y) * (long long)W + x];
    if (v != v) return 0;                                         // NaN -> 0 (export._rgb_bytes_host)
    return (int)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);          // (x.clip(0, 1) * 255) truncated
}

__device__ __forceinline__ int png_paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int png_cost(int v) { return v < 256 - v ? v : 256 - v; }

// the five filtered values of one byte
__device__ __forceinline__ void png_filters(int x, int a, int b, int c, int f[5])
{
    f[0] = x;
    f[1] = (x - a) & 255;
    f[2] = (x - b) & 255;
    f[3] = (x - ((a + b) >> 1)) & 255;
    f[4] = (x - png_paeth(a, b, c)) & 255;
}

// step 1 + 2: rows [y0, y0 + rows) of image n, filtered, into sh.filt; one wave per row
template <int KIND>
__device__ void png_filter_chunk(PngShared &sh, const void *__restrict__ src, long long n, int y0, int rows, int H, int W, int Cn, int filter_mode)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, WC = W * Cn;
    for (int r = wave; r < rows; r += PNG_WAVES) {
        const int y = y0 + r;
        int best = 0;
        if (filter_mode == 0) {
            uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
            for (int j = lane; j < WC; j += 64) {
                const int x = png_raw<KIND>(src, n, y, j, H, W, Cn);
                const int a = j >= Cn ? png_raw<KIND>(src, n, y, j - Cn, H, W, Cn) : 0;
                const int b = y > 0 ? png_raw<KIND>(src, n, y - 1, j, H, W, Cn) : 0;
                const int c = (y > 0 && j >= Cn) ? png_raw<KIND>(src, n, y - 1, j - Cn, H, W, Cn) : 0;
                int f[5];
                png_filters(x, a, b, c, f);
#pragma unroll
                for (int k = 0; k < 5; ++k) cost[k] += (uint32_t)png_cost(f[k]);
            }
#pragma unroll
            for (int k = 0; k < 5; ++k)
                for (int d = 32; d >= 1; d >>= 1) cost[k] += __shfl_xor(cost[k], d, 64);
#pragma unroll
            for (int k = 1; k < 5; ++k)
                if (cost[k] < cost[best]) best = k;               // ties to the lowest filter number
        }
        uint8_t *__restrict__ out = sh.filt + (size_t)r * (WC + 1);
        if (lane == 0) out[0] = (uint8_t)best;
        for (int j = lane; j < WC; j += 64) {
            const int x = png_raw<KIND>(src, n, y, j, H, W, Cn);
            int v = x;
            if (best != 0) {
                const int a = j >= Cn ? png_raw<KIND>(src, n, y, j - Cn, H, W, Cn) : 0;
                const int b = y > 0 ? png_raw<KIND>(src, n, y - 1, j, H, W, Cn) : 0;
                const int c = (y > 0 && j >= Cn) ? png_raw<KIND>(src, n, y - 1, j - Cn, H, W, Cn) : 0;
                int f[5];
                png_filters(x, a, b, c, f);
                v = f[best];
            }
            out[1 + j] = (uint8_t)v;
        }
    }
}

// deflate's length code of a match of m = 3 .. 258 bytes
__device__ __forceinline__ void png_length_symbol(int m, int &sym, int &ebits, int &extra)
{
    const int v = m - 3;
    if (m == 258) {
        sym = 285, ebits = 0, extra = 0;
    } else if (v < 8) {
        sym = 257 + v, ebits = 0, extra = 0;
    } else {
        const int e = 29 - __clz(v);                              // floor(log2 v) - 2
        sym = 261 + 4 * e + ((v >> e) & 3), ebits = e, extra = v & ((1 << e) - 1);
    }
}

// OR `nbits` bits of `val` into the bit string at `at` (LDS atomics: neighbours share words)
__device__ __forceinline__ void png_put(PngShared &sh, uint32_t at, uint32_t val, int nbits)
{
    if (nbits <= 0) return;
    const uint64_t v = (uint64_t)val << (at & 31);
    const uint32_t w = at >> 5, lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (lo && w < PNG_BIT_WORDS) atomicOr(&sh.bits[w], lo);
    if (hi && w + 1 < PNG_BIT_WORDS) atomicOr(&sh.bits[w + 1], hi);
}

// The tokens whose first byte lies in [a, b) of the n filtered bytes, in order.  A run of L equal bytes starting at s is the literal at s,
// then the other R = L - 1 bytes in pieces of 258 from s + 1: a piece of 3 or more is one match (distance 1), a last piece of 1 or 2
// bytes is literals.  MODE 0 counts symbols, MODE 1 returns the bits of the tokens, MODE 2 writes them from bit `at` on.
template <int MODE>
__device__ uint32_t png_walk(PngShared &sh, int n, int a, int b, int prev_start, int next_start, uint32_t at)
{
    uint32_t bits = 0;
    auto literal = [&](int v) {
        if (MODE == 0) atomicAdd(&sh.hist[v], 1u);
        if (MODE == 1) bits += sh.len[v];
        if (MODE == 2) {
            png_put(sh, at, sh.code[v], sh.len[v]);
            at += sh.len[v];
        }
    };
    auto match = [&](int m) {
        int sym, ebits, extra;
        png_length_symbol(m, sym, ebits, extra);
        if (MODE == 0) {
            atomicAdd(&sh.hist[sym], 1u);
            atomicAdd(&sh.hist[PNG_LL], 1u);
        }
        const int nb = sh.len[sym] + ebits;
        if (MODE == 1) bits += nb + sh.len[PNG_LL];
        if (MODE == 2) {
            png_put(sh, at, (uint32_t)sh.code[sym] | ((uint32_t)extra << sh.len[sym]), nb);
            at += nb + sh.len[PNG_LL];                             // distance code 0 is the single bit 0
        }
    };
    int i = a;
    if (i >= b) return 0;
    int s = (i == 0 || sh.filt[i] != sh.filt[i - 1]) ? i : prev_start;
    while (i < b) {
        const int v = sh.filt[i];
        int e = i + 1;
        while (e < b && sh.filt[e] == v) ++e;
        if (e == b) e = next_start;                               // no start in the rest of this range: the run ends where the next one begins
        const int stop = e < b ? e : b;
        if (i == s) literal(v);
        const int R = e - s - 1, first = s + 1;
        for (int j = i > first ? (i - first) / 258 : 0;; ++j) {
            const int p = first + 258 * j;
            if (p >= stop || 258 * j >= R) break;
            const int plen = R - 258 * j < 258 ? R - 258 * j : 258;
            if (plen >= 3) {
                if (p >= i) match(plen);
            } else {
                for (int q = 0; q < plen; ++q)
                    if (p + q >= i && p + q < stop) literal(v);
            }
        }
        i = stop;
        s = e;
    }
    return bits;
}

// steps 1-5 of the construction above for `n` symbols with counts `cnt`: lengths into `len`, sh.num[d] = codes of length d; all threads
__device__ void png_code_lengths(PngShared &sh, const uint32_t *cnt, int n, int limit, uint8_t *len)
{
    const int t = threadIdx.x;
    if (t == 0) sh.used = 0, sh.acted = 0;
    if (t < 16) sh.num[t] = 0;
    __syncthreads();
    for (int s = t; s < n; s += PNG_THREADS) {
        const uint32_t c = cnt[s];
        len[s] = 0;
        if (c) {
            int rank = 0;
            for (int u = 0; u < n; ++u) {
                const uint32_t cu = cnt[u];
                rank += (cu != 0 && (cu < c || (cu == c && u < s))) ? 1 : 0;
            }
            sh.order[rank] = (uint16_t)s;
            sh.weight[rank] = c;
            atomicAdd(&sh.used, 1);
        }
    }
    __syncthreads();
    const int m = sh.used;
    if (m == 1) {
        if (t == 0) len[sh.order[0]] = 1, sh.num[1] = 1;
        __syncthreads();
        return;
    }
    if (t == 0) {
        int leaf = 0, node = m;
        for (int nw = m; nw < 2 * m - 1; ++nw) {
            uint32_t sum = 0;
            for (int k = 0; k < 2; ++k) {
                int pick;
                if (leaf < m && (node >= nw || sh.weight[leaf] <= sh.weight[node])) pick = leaf++;
                else pick = node++;
                sh.parent[pick] = (uint16_t)nw;
                sum += sh.weight[pick];
            }
            sh.weight[nw] = sum;
        }
    }
    __syncthreads();
    for (int i = t; i < m; i += PNG_THREADS) {
        int d = 0;
        for (int p = i; p != 2 * m - 2; p = sh.parent[p]) ++d;
        if (d > limit) {
            d = limit;
            sh.acted = 1;
        }
        atomicAdd(&sh.num[d], 1u);
    }
    __syncthreads();
    if (t == 0) {
        if (sh.acted) {
            uint32_t total = 0;
            for (int d = 1; d <= limit; ++d) total += sh.num[d] << (limit - d);
            while (total != (1u << limit)) {
                sh.num[limit] -= 1;
                for (int d = limit - 1; d >= 1; --d)
                    if (sh.num[d]) {
                        sh.num[d] -= 1;
                        sh.num[d + 1] += 2;
                        break;
                    }
                total -= 1;
            }
        }
        uint32_t c = 0;
        for (int d = 1; d <= limit; ++d) {
            c += sh.num[d];
            sh.cum[d] = c;
        }
    }
    __syncthreads();
    for (int i = t; i < m; i += PNG_THREADS) {
        const uint32_t from_top = (uint32_t)(m - 1 - i);
        int d = 1;
        while (d < limit && sh.cum[d] <= from_top) ++d;
        len[sh.order[i]] = (uint8_t)d;
    }
    __syncthreads();
}

// deflate's canonical codes from the lengths and sh.num, bit-reversed; all threads
__device__ void png_codes(PngShared &sh, const uint8_t *len, int n, int limit, uint16_t *code)
{
    const int t = threadIdx.x;
    if (t == 0) {
        uint32_t c = 0;
        sh.next_code[0] = 0;
        for (int d = 1; d <= limit; ++d) {
            c = (c + (d > 1 ? sh.num[d - 1] : 0u)) << 1;
            sh.next_code[d] = c;
        }
    }
    __syncthreads();
    for (int s = t; s < n; s += PNG_THREADS) {
        const int d = len[s];
        uint32_t c = 0;
        if (d) {
            c = sh.next_code[d];
            for (int u = 0; u < s; ++u) c += len[u] == d ? 1u : 0u;
            c = __brev(c) >> (32 - d);
        }
        code[s] = (uint16_t)c;
    }
    __syncthreads();
}

// The 287 code lengths in the code-length alphabet, greedy: a run of r zeros is 18 (11..138) while r >= 11, then 17 (3..10) while r >= 3,
// then single zeros; a run of r equal lengths v > 0 is v, then 16 (3..6 repeats) while r >= 3 remain, then single v.  Thread 0.
__device__ void png_code_length_tokens(PngShared &sh)
{
    int count = 0, i = 0;
    auto emit = [&](int sym, int extra) {
        sh.cl_tok[count++] = (uint16_t)(sym | (extra << 5));
        sh.cl_hist[sym] += 1;
    };
    while (i < PNG_SEQ) {
        const int v = sh.len[i];
        int r = 1;
        while (i + r < PNG_SEQ && sh.len[i + r] == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) {
                const int m = r < 138 ? r : 138;
                emit(18, m - 11);
                r -= m;
            }
            while (r >= 3) {
                const int m = r < 10 ? r : 10;
                emit(17, m - 3);
                r -= m;
            }
        } else {
            emit(v, 0);
            r -= 1;
            while (r >= 3) {
                const int m = r < 6 ? r : 6;
                emit(16, m - 3);
                r -= m;
            }
        }
        for (; r > 0; --r) emit(v, 0);
    }
    sh.n_cl_tok = count;
}

__device__ __forceinline__ int png_cl_extra_bits(int sym) { return sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)); }

template <int KIND>
__global__ void __launch_bounds__(PNG_THREADS) k_png_chunks(const void *__restrict__ src, int H, int W, int Cn, int filter_mode, int rows_per_chunk,
                                                            int chunks_per_image, int32_t *__restrict__ meta, uint8_t *__restrict__ slots)
{
    __shared__ PngShared sh;
    const int t = threadIdx.x;
    const long long chunk = blockIdx.x, image = chunk / chunks_per_image;
    const int k = (int)(chunk - image * chunks_per_image), y0 = k * rows_per_chunk;
    const int rows = H - y0 < rows_per_chunk ? H - y0 : rows_per_chunk;
    const int n = rows * (1 + W * Cn);                            // <= GSR_PNG_CHUNK_BYTES by the host's choice of rows_per_chunk

    for (int i = t; i < PNG_BIT_WORDS; i += PNG_THREADS) sh.bits[i] = 0u;
    for (int i = t; i < PNG_SYMS; i += PNG_THREADS) sh.hist[i] = 0u;
    if (t <= PNG_CL) sh.cl_hist[t] = 0u;
    if (t == 0) sh.header_bits = 0u, sh.s1 = 0u, sh.s2 = 0u;
    png_filter_chunk<KIND>(sh, src, image, y0, rows, H, W, Cn, filter_mode);
    __syncthreads();

    // every thread owns the tokens that begin in [a, b); where runs begin, for the ranges before and after
    const int per = (n + PNG_THREADS - 1) / PNG_THREADS, a = min(t * per, n), b = min(a + per, n);
    {
        int first = -1, last = -1;
        uint32_t s1 = 0, s2 = 0;
        for (int i = a; i < b; ++i) {
            const uint32_t d = sh.filt[i];
            if (i == 0 || sh.filt[i - 1] != d) {
                if (first < 0) first = i;
                last = i;
            }
            s1 += d;
            s2 += (uint32_t)(n - i) * d;                           // per <= 64: below 64 * 16384 * 255
        }
        sh.first_start[t] = (int16_t)first;
        sh.last_start[t] = (int16_t)last;
        atomicAdd(&sh.s1, s1);                                     // below 16384 * 255
        atomicAdd(&sh.s2, s2 % PNG_ADLER);
    }
    __syncthreads();
    int prev_start = 0, next_start = n;
    for (int u = t - 1; u >= 0; --u)
        if (sh.last_start[u] >= 0) {
            prev_start = sh.last_start[u];
            break;
        }
    for (int u = t + 1; u < PNG_THREADS; ++u)
        if (sh.first_start[u] >= 0) {
            next_start = sh.first_start[u];
            break;
        }

    // steps 3-5: tokens, histogram, codes
    png_walk<0>(sh, n, a, b, prev_start, next_start, 0u);
    if (t == 0) sh.hist[256] = 1u;                                // end of block, once
    __syncthreads();
    const uint32_t matches = sh.hist[PNG_LL];
    __syncthreads();
    if (t == 0) sh.hist[PNG_LL] = 0u;                             // (not a literal / length symbol)
    png_code_lengths(sh, sh.hist, PNG_LL, 15, sh.len);
    png_codes(sh, sh.len, PNG_LL, 15, sh.code);
    if (t == 0) {
        sh.len[PNG_LL] = matches ? 1 : 0;                         // only distance code 0: length 1; no match at all: HDIST 1 with a zero length
        png_code_length_tokens(sh);
    }
    __syncthreads();
    png_code_lengths(sh, sh.cl_hist, PNG_CL, 7, sh.cl_len);
    png_codes(sh, sh.cl_len, PNG_CL, 7, sh.cl_code);

    // sizes: header, tokens, end of block
    if (t == 0) {
        int hclen = 4;
        for (int i = 4; i < PNG_CL; ++i)
            if (sh.cl_len[c_png_cl_order[i]]) hclen = i + 1;
        sh.hclen = hclen;
        atomicAdd(&sh.header_bits, 17u + 3u * hclen);
    }
    for (int i = t; i < sh.n_cl_tok; i += PNG_THREADS) {
        const int sym = sh.cl_tok[i] & 31;
        atomicAdd(&sh.header_bits, (uint32_t)sh.cl_len[sym] + png_cl_extra_bits(sym));
    }
    const uint32_t mine = png_walk<1>(sh, n, a, b, prev_start, next_start, 0u);
    uint32_t *scan = sh.weight;                                   // (the tree is done with it)
    scan[t] = mine;
    __syncthreads();
    for (int d = 1; d < PNG_THREADS; d <<= 1) {                   // inclusive sum over the threads
        const uint32_t add = t >= d ? scan[t - d] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const uint32_t header_bits = sh.header_bits, token_bits = scan[PNG_THREADS - 1];
    const uint32_t total_bits = header_bits + token_bits + sh.len[256];
    const uint32_t coded_bytes = (total_bits + 3u + 7u) / 8u + 4u;
    uint8_t *__restrict__ slot = slots + (size_t)chunk * GSR_PNG_SLOT_BYTES;
    uint32_t *__restrict__ slot_w = reinterpret_cast<uint32_t *>(slot);
    uint32_t payload;
    if (coded_bytes >= (uint32_t)n + 5u) {
        // step 7: one stored block, 00 LEN NLEN and the bytes
        payload = (uint32_t)n + 5u;
        const uint32_t nlen = (uint32_t)n ^ 0xffffu;
        for (uint32_t w = t; w < (payload + 3u) / 4u; w += PNG_THREADS) {
            uint32_t word = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t at = 4u * w + q;
                uint32_t byte = 0;
                if (at == 1) byte = (uint32_t)n & 255u;
                else if (at == 2) byte = ((uint32_t)n >> 8) & 255u;
                else if (at == 3) byte = nlen & 255u;
                else if (at == 4) byte = (nlen >> 8) & 255u;
                else if (at >= 5 && at < payload) byte = sh.filt[at - 5];
                word |= byte << (8 * q);
            }
            slot_w[w] = word;
        }
    } else {
        // step 6: BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN, the code-length code, the code lengths; the tokens; end of block
        payload = coded_bytes;
        if (t == 0) {
            uint32_t at = 0;
            png_put(sh, at, 4u, 3), at += 3;
            png_put(sh, at, 29u, 5), at += 5;
            png_put(sh, at, 0u, 5), at += 5;
            png_put(sh, at, (uint32_t)(sh.hclen - 4), 4), at += 4;
            for (int i = 0; i < sh.hclen; ++i) png_put(sh, at, sh.cl_len[c_png_cl_order[i]], 3), at += 3;
            for (int i = 0; i < sh.n_cl_tok; ++i) {
                const int sym = sh.cl_tok[i] & 31, extra = sh.cl_tok[i] >> 5, nb = sh.cl_len[sym];
                png_put(sh, at, (uint32_t)sh.cl_code[sym] | ((uint32_t)extra << nb), nb + png_cl_extra_bits(sym));
                at += nb + png_cl_extra_bits(sym);
            }
            png_put(sh, header_bits + token_bits, sh.code[256], sh.len[256]);
            // the empty stored block: 000, padding to the byte, 00 00 FF FF
            png_put(sh, (coded_bytes - 2u) * 8u, 0xffffu, 16);
        }
        png_walk<2>(sh, n, a, b, prev_start, next_start, header_bits + scan[t] - mine);
        __syncthreads();
        for (uint32_t w = t; w < (payload + 3u) / 4u; w += PNG_THREADS) slot_w[w] = sh.bits[w];
    }
    if (t == 0) {
        int32_t *__restrict__ mrow = meta + chunk * PNG_META;
        mrow[0] = (int32_t)payload;
        mrow[1] = (int32_t)(sh.s1 % PNG_ADLER);
        mrow[2] = (int32_t)(sh.s2 % PNG_ADLER);
        mrow[3] = n;
    }
}

// one workgroup per chunk: its payload to its place in the image's stream; the first writes the zlib header, the last the final block,
// the Adler-32 and the length
__global__ void __launch_bounds__(PNG_THREADS) k_png_assemble(const int32_t *__restrict__ meta, const uint8_t *__restrict__ slots, int chunks_per_image,
                                                              uint8_t *__restrict__ out, long long out_stride, int32_t *__restrict__ lengths)
{
    __shared__ uint32_t before;
    const int t = threadIdx.x;
    const long long image = blockIdx.x / chunks_per_image, c0 = image * chunks_per_image;
    const int k = (int)(blockIdx.x - c0);
    if (t == 0) before = 0u;
    __syncthreads();
    uint32_t sum = 0;
    for (int u = t; u < k; u += PNG_THREADS) sum += (uint32_t)meta[(c0 + u) * PNG_META];
    if (sum) atomicAdd(&before, sum);
    __syncthreads();
    const uint32_t at = 2u + before, bytes = (uint32_t)meta[(c0 + k) * PNG_META];
    uint8_t *__restrict__ dst = out + image * out_stride;
    const uint8_t *__restrict__ from = slots + (size_t)(c0 + k) * GSR_PNG_SLOT_BYTES;
    for (uint32_t i = t; i < bytes; i += PNG_THREADS) dst[at + i] = from[i];
    if (k == 0 && t == 0) dst[0] = 0x78, dst[1] = 0x01;
    if (k == chunks_per_image - 1 && t == 0) {
        uint32_t A = 1u, B = 0u;
        for (int u = 0; u < chunks_per_image; ++u) {
            const int32_t *__restrict__ m = meta + (c0 + u) * PNG_META;
            B = (B + (uint32_t)m[3] * A + (uint32_t)m[2]) % PNG_ADLER;      // m[3] <= 16384, A < 65521: below 2^31
            A = (A + (uint32_t)m[1]) % PNG_ADLER;
        }
        uint8_t *__restrict__ e = dst + at + bytes;
        e[0] = 0x01, e[1] = 0x00, e[2] = 0x00, e[3] = 0xff, e[4] = 0xff;
        e[5] = (uint8_t)(B >> 8), e[6] = (uint8_t)B, e[7] = (uint8_t)(A >> 8), e[8] = (uint8_t)A;
        lengths[image] = (int32_t)(at + bytes + 9u);
    }
}

struct PngPlan {
    int rows, chunks_per_image;
    long long chunks;
    size_t meta_bytes, scratch_bytes, bound;
};

// 0: fine, GSR_PNG_ROW_TOO_WIDE, or GSR_EINVAL
inline int png_plan(int64_t N, int H, int W, int Cn, PngPlan &p)
{
    if (N < 1 || N > (1LL << 24) || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20) || (Cn != 3 && Cn != 4)) return GSR_EINVAL;
    const long long row = 1 + (long long)W * Cn;
    if (row > GSR_PNG_CHUNK_BYTES) return GSR_PNG_ROW_TOO_WIDE;
    p.rows = (int)(GSR_PNG_CHUNK_BYTES / row);
    if (p.rows > H) p.rows = H;
    p.chunks_per_image = (H + p.rows - 1) / p.rows;
    p.chunks = (long long)N * p.chunks_per_image;
    const long long bound = 2 + (long long)H * row + 5LL * p.chunks_per_image + 5 + 4;
    if (p.chunks > 0x7fffffffLL || bound > 0x7fffffffLL || p.chunks_per_image > 65535) return GSR_EINVAL;
    p.bound = (size_t)bound;
    p.meta_bytes = ((size_t)p.chunks * PNG_META * sizeof(int32_t) + 15) & ~(size_t)15;
    p.scratch_bytes = p.meta_bytes + (size_t)p.chunks * GSR_PNG_SLOT_BYTES;
    return GSR_OK;
}

}  // namespace gsr

#ifndef GSR_PNG_HOST_SIM
extern "C" {

__attribute__((visibility("default"))) size_t gsr_png_scratch_bytes(int64_t N, int H, int W, int C)
{
    gsr::PngPlan p;
    return gsr::png_plan(N, H, W, C, p) == GSR_OK ? p.scratch_bytes : 0;
}

__attribute__((visibility("default"))) size_t gsr_png_stream_bound(int H, int W, int C)
{
    gsr::PngPlan p;
    return gsr::png_plan(1, H, W, C, p) == GSR_OK ? p.bound : 0;
}

__attribute__((visibility("default"))) int gsr_png_chunks(const void *src, int src_kind, int64_t N, int H, int W, int C, int filter_mode, void *scratch,
                                                          size_t scratch_bytes, void *stream)
{
    using namespace gsr;
    PngPlan p;
    if (!src || !scratch || (src_kind != GSR_PNG_SRC_U8 && src_kind != GSR_PNG_SRC_F32_PLANAR) || (filter_mode != 0 && filter_mode != 1)) return GSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) || (src_kind == GSR_PNG_SRC_F32_PLANAR && (reinterpret_cast<uintptr_t>(src) & 3))) return GSR_EINVAL;
    const int rc = png_plan(N, H, W, C, p);
    if (rc != GSR_OK) return rc;
    if (scratch_bytes < p.scratch_bytes) return GSR_ENOSPACE;
    int32_t *meta = static_cast<int32_t *>(scratch);
    uint8_t *slots = static_cast<uint8_t *>(scratch) + p.meta_bytes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (src_kind == GSR_PNG_SRC_U8)
        hipLaunchKernelGGL(k_png_chunks<GSR_PNG_SRC_U8>, dim3((unsigned)p.chunks), dim3(PNG_THREADS), 0, s, src, H, W, C, filter_mode, p.rows,
                           p.chunks_per_image, meta, slots);
    else
        hipLaunchKernelGGL(k_png_chunks<GSR_PNG_SRC_F32_PLANAR>, dim3((unsigned)p.chunks), dim3(PNG_THREADS), 0, s, src, H, W, C, filter_mode, p.rows,
                           p.chunks_per_image, meta, slots);
    return launch_status();
}

__attribute__((visibility("default"))) int gsr_png_assemble(const void *scratch, size_t scratch_bytes, int64_t N, int H, int W, int C, uint8_t *out,
                                                            size_t out_stride, int32_t *lengths, void *stream)
{
    using namespace gsr;
    PngPlan p;
    if (!scratch || !out || !lengths || (reinterpret_cast<uintptr_t>(scratch) & 15) || (reinterpret_cast<uintptr_t>(lengths) & 3)) return GSR_EINVAL;
    const int rc = png_plan(N, H, W, C, p);
    if (rc != GSR_OK) return rc;
    if (scratch_bytes < p.scratch_bytes) return GSR_ENOSPACE;
    if (out_stride < p.bound || out_stride > 0x7fffffffULL) return GSR_EINVAL;
    const int32_t *meta = static_cast<const int32_t *>(scratch);
    const uint8_t *slots = static_cast<const uint8_t *>(scratch) + p.meta_bytes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_png_assemble, dim3((unsigned)p.chunks), dim3(PNG_THREADS), 0, s, meta, slots, p.chunks_per_image, out,
                       (long long)out_stride, lengths);
    return launch_status();
}

}  // extern "C"
#endif

// gsr_jpeg_entropy.h -- the host half of the JPEG decoder (include/gsr.h: gsr_jpeg_probe, gsr_jpeg_entropy): marker parsing and the
// Huffman stage of baseline / extended-sequential streams, into de-zigzagged int16 coefficient blocks that csrc/gsr_jpeg.hip turns
// into pixels.  Plain C++17, no HIP include: it compiles alone (tools/jpeg_entropy_sweep.cpp builds it with the host sanitizers).
//
// This code parses UNTRUSTED bytes.  The rules it keeps:
//   * every byte of the stream is read through Reader / BitReader, which know the length and never index past it;
//   * every table index is formed from a value that was range-checked on the line that produced it (table ids 0..3, component
//     ids by search, Huffman symbols by construction of the tables, zigzag positions 1..63);
//   * every coefficient write goes through a block index that was computed from the block grid of its component and is checked
//     against the image's coefficient count once more before the store;
//   * anything that is not a complete, valid stream of the fast path ends as GSR_JPEG_CORRUPT or GSR_JPEG_UNSUPPORTED; the caller
//     hands both to the reference decoder, so a wrong verdict between the two costs time, never a wrong picture.
//
// Fast path: SOF0 / SOF1, 8-bit samples, Huffman, ONE interleaved scan; one component, or three (YCbCr) with luma sampled 1x1, 2x1 or
// 2x2 and chroma 1x1; any restart interval; any Huffman tables.  The coefficient gate sends an image whose
// dequantised blocks leave the range in which the device kernel's 32-bit arithmetic (and the reference's 16-bit SIMD lanes) cannot
// overflow to GSR_JPEG_UNSUPPORTED.
#ifndef GSR_JPEG_ENTROPY_H
#define GSR_JPEG_ENTROPY_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/gsr.h"

// the two size rules below are also the device stage's (csrc/gsr_jpeg.hip checks every descriptor against them): compiled for both
// sides there, for the host alone everywhere else
#ifdef __HIPCC__
#define GSR_JPEG_HD __host__ __device__
#else
#define GSR_JPEG_HD
#endif

namespace gsr_jpeg {

constexpr int LOOK = 9;   // bits of the Huffman look-ahead table

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined = false;
    uint16_t look[1 << LOOK];   // (length << 8) | symbol for codes of at most LOOK bits, 0: longer (or no such code)
    int32_t maxcode[18];        // largest code of each length, -1: none; [17] is a sentinel
    int32_t valoff[17];         // index of the first symbol of a length minus its first code
    uint8_t vals[256];
    int nvals = 0;
};

struct Component {
    int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
};

struct Header {
    int width = 0, height = 0, ncomp = 0, sampling = -1, restart = 0, sof = -1;
    Component comp[3];
    uint16_t quant[4][64];   // natural order
    bool quant_defined[4] = {false, false, false, false};
    bool quant16 = false;
    Huff dc[4], ac[4];
    size_t scan = 0;   // offset of the first entropy-coded byte
};

// bounds-checked big-endian reads of the marker segments
struct Reader {
    const uint8_t *p;
    size_t n, at;
    bool ok = true;
    Reader(const uint8_t *data, size_t len) : p(data), n(len), at(0) {}
    int u8()
    {
        if (at >= n) { ok = false; return 0; }
        return p[at++];
    }
    int u16()
    {
        const int hi = u8();
        return (hi << 8) | u8();
    }
};

inline int build_huff(Huff &t, const uint8_t counts[16], const uint8_t *vals, int nvals)
{
    int code = 0, k = 0;
    memset(t.look, 0, sizeof(t.look));
    for (int len = 1; len <= 16; ++len) {
        const int cnt = counts[len - 1];
        t.valoff[len] = k - code;
        if (cnt) {
            if (code + cnt > (1 << len)) return GSR_JPEG_CORRUPT;   // more codes than the length has
            for (int i = 0; i < cnt; ++i, ++k, ++code) {
                if (len <= LOOK) {
                    const int first = code << (LOOK - len), span = 1 << (LOOK - len);
                    for (int j = 0; j < span; ++j) t.look[first + j] = (uint16_t)((len << 8) | vals[k]);
                }
            }
            t.maxcode[len] = code - 1;
        } else {
            t.maxcode[len] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    memcpy(t.vals, vals, (size_t)nvals);
    t.nvals = nvals;
    t.defined = true;
    return GSR_OK;
}

// Markers up to and including SOS.  GSR_OK: `h` describes a stream of the fast path and h.scan points at its entropy-coded bytes.
// width / height / ncomp are filled as soon as a frame header was read, also for an unsupported stream.
inline int parse_header(const uint8_t *data, size_t len, Header &h)
{
    Reader r(data, len);
    if (r.u8() != 0xFF || r.u8() != 0xD8 || !r.ok) return GSR_JPEG_CORRUPT;
    bool jfif = false, adobe = false;
    int adobe_transform = 0;
    for (;;) {
        int b = r.u8();
        if (!r.ok) return GSR_JPEG_CORRUPT;
        if (b != 0xFF) return GSR_JPEG_CORRUPT;   // the reference decoder resynchronises here; it keeps such streams
        int m = r.u8();
        while (m == 0xFF && r.ok) m = r.u8();     // fill bytes
        if (!r.ok) return GSR_JPEG_CORRUPT;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, RSTn: no segment
        if (m == 0xD8 || m == 0xD9 || m == 0x00) return GSR_JPEG_CORRUPT;
        const size_t seg = r.at;
        const int L = r.u16();
        if (!r.ok || L < 2 || seg + (size_t)L > len) return GSR_JPEG_CORRUPT;
        const size_t end = seg + (size_t)L;
        if (m == 0xC0 || m == 0xC1) {
            if (h.sof >= 0) return GSR_JPEG_CORRUPT;
            if (L < 8) return GSR_JPEG_CORRUPT;
            const int prec = r.u8();
            h.height = r.u16();
            h.width = r.u16();
            h.ncomp = r.u8();
            h.sof = m - 0xC0;
            if (L != 8 + 3 * h.ncomp) return GSR_JPEG_CORRUPT;
            if (h.width < 1) return GSR_JPEG_CORRUPT;
            if (prec != 8 || h.height < 1) return GSR_JPEG_UNSUPPORTED;   // 12-bit samples; a height given later by DNL
            if (h.ncomp != 1 && h.ncomp != 3) return h.ncomp < 1 ? GSR_JPEG_CORRUPT : GSR_JPEG_UNSUPPORTED;
            for (int c = 0; c < h.ncomp; ++c) {
                Component &k = h.comp[c];
                k.id = r.u8();
                const int hv = r.u8();
                k.h = hv >> 4;
                k.v = hv & 15;
                k.tq = r.u8();
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) return GSR_JPEG_CORRUPT;
            }
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            // progressive, lossless, differential, arithmetic frames: read the size for the caller, then leave
            if (L >= 8) {
                (void)r.u8();
                h.height = r.u16();
                h.width = r.u16();
                h.ncomp = r.u8();
            }
            return GSR_JPEG_UNSUPPORTED;
        } else if (m == 0xCC) {
            return GSR_JPEG_UNSUPPORTED;   // arithmetic conditioning
        } else if (m == 0xC4) {
            while (r.at < end) {
                const int tc_th = r.u8();
                const int tc = tc_th >> 4, th = tc_th & 15;
                if (tc > 1 || th > 3) return GSR_JPEG_CORRUPT;
                uint8_t counts[16], vals[256];
                int total = 0;
                for (int i = 0; i < 16; ++i) {
                    counts[i] = (uint8_t)r.u8();
                    total += counts[i];
                }
                if (!r.ok || total > 256 || r.at + (size_t)total > end) return GSR_JPEG_CORRUPT;
                for (int i = 0; i < total; ++i) vals[i] = (uint8_t)r.u8();
                const int rc = build_huff(tc ? h.ac[th] : h.dc[th], counts, vals, total);
                if (rc != GSR_OK) return rc;
            }
        } else if (m == 0xDB) {
            while (r.at < end) {
                const int pq_tq = r.u8();
                const int pq = pq_tq >> 4, tq = pq_tq & 15;
                if (pq > 1 || tq > 3) return GSR_JPEG_CORRUPT;
                if (r.at + (size_t)(64 << pq) > end) return GSR_JPEG_CORRUPT;
                for (int i = 0; i < 64; ++i) h.quant[tq][ZIGZAG[i]] = (uint16_t)(pq ? r.u16() : r.u8());
                h.quant_defined[tq] = true;
                if (pq) h.quant16 = true;
            }
        } else if (m == 0xDD) {
            if (L != 4) return GSR_JPEG_CORRUPT;
            h.restart = r.u16();
        } else if (m == 0xE0) {
            if (L >= 7 && data[seg + 2] == 'J' && data[seg + 3] == 'F' && data[seg + 4] == 'I' && data[seg + 5] == 'F' && data[seg + 6] == 0) jfif = true;
        } else if (m == 0xEE) {
            if (L >= 14 && data[seg + 2] == 'A' && data[seg + 3] == 'd' && data[seg + 4] == 'o' && data[seg + 5] == 'b' && data[seg + 6] == 'e') {
                adobe = true;
                adobe_transform = data[seg + 13];
            }
        } else if (m == 0xDA) {
            if (h.sof < 0) return GSR_JPEG_CORRUPT;
            const int ns = r.u8();
            if (!r.ok || ns < 1 || ns > 4 || L != 6 + 2 * ns) return GSR_JPEG_CORRUPT;
            if (ns != h.ncomp) return GSR_JPEG_UNSUPPORTED;   // several scans
            for (int i = 0; i < ns; ++i) {
                const int cid = r.u8(), tt = r.u8();
                if (cid != h.comp[i].id) return GSR_JPEG_UNSUPPORTED;   // another component order
                h.comp[i].td = tt >> 4;
                h.comp[i].ta = tt & 15;
                if (h.comp[i].td > 3 || h.comp[i].ta > 3) return GSR_JPEG_CORRUPT;
                if (!h.dc[h.comp[i].td].defined || !h.ac[h.comp[i].ta].defined || !h.quant_defined[h.comp[i].tq]) return GSR_JPEG_CORRUPT;
            }
            const int ss = r.u8(), se = r.u8(), ahal = r.u8();
            if (!r.ok) return GSR_JPEG_CORRUPT;
            if (ss != 0 || se != 63 || ahal != 0) return GSR_JPEG_UNSUPPORTED;
            if (h.quant16 && h.sof == 0) return GSR_JPEG_UNSUPPORTED;
            if (h.ncomp == 1) {
                h.sampling = GSR_JPEG_GRAY;
            } else {
                // the colour space as the reference decoder guesses it: JFIF says YCbCr; else the Adobe transform; else the component ids
                if (!jfif && adobe && adobe_transform != 1) return GSR_JPEG_UNSUPPORTED;
                if (!jfif && !adobe && h.comp[0].id == 'R' && h.comp[1].id == 'G' && h.comp[2].id == 'B') return GSR_JPEG_UNSUPPORTED;
                if (h.comp[1].h != 1 || h.comp[1].v != 1 || h.comp[2].h != 1 || h.comp[2].v != 1) return GSR_JPEG_UNSUPPORTED;
                const int lh = h.comp[0].h, lv = h.comp[0].v;
                if (lh == 1 && lv == 1) h.sampling = GSR_JPEG_444;
                else if (lh == 2 && lv == 1) h.sampling = GSR_JPEG_422;
                else if (lh == 2 && lv == 2) h.sampling = GSR_JPEG_420;
                else return GSR_JPEG_UNSUPPORTED;
            }
            h.scan = end;
            return GSR_OK;
        }
        r.at = end;
    }
}

// block grids of a sampling class for an H x W picture, in whole MCUs; returns the int16 count of all components
GSR_JPEG_HD inline int64_t block_grids(int sampling, int H, int W, int32_t bw[3], int32_t bh[3])
{
    const int mw = sampling == GSR_JPEG_422 || sampling == GSR_JPEG_420 ? 16 : 8, mh = sampling == GSR_JPEG_420 ? 16 : 8;
    const int mx = (W + mw - 1) / mw, my = (H + mh - 1) / mh;
    bw[0] = mx * (mw / 8);
    bh[0] = my * (mh / 8);
    const int nc = sampling == GSR_JPEG_GRAY ? 1 : 3;
    for (int c = 1; c < 3; ++c) {
        bw[c] = nc == 3 ? mx : 0;
        bh[c] = nc == 3 ? my : 0;
    }
    return 64 * ((int64_t)bw[0] * bh[0] + (int64_t)bw[1] * bh[1] + (int64_t)bw[2] * bh[2]);
}

// the largest coefficient count any sampling class needs for an H x W picture: the per-image stride of the byte planes and the bound of
// the coefficient buffer
GSR_JPEG_HD inline int64_t max_image_coefs(int H, int W)
{
    int32_t bw[3], bh[3];
    int64_t best = 0;
    for (int s = GSR_JPEG_GRAY; s <= GSR_JPEG_420; ++s) {
        const int64_t n = block_grids(s, H, W, bw, bh);
        best = n > best ? n : best;
    }
    return best;
}

// The entropy-coded segment as a bit stream.  0xFF 0x00 is a stuffed 0xFF; any other marker ends the data: the reader then feeds zero
// bits and counts them, and a caller that CONSUMED one of them has run past the data (`overrun`).
struct BitReader {
    const uint8_t *p;
    size_t n, at;
    uint64_t acc = 0;
    int bits = 0;       // valid bits in acc (the low `bits` bits)
    int pad = 0;        // how many of them, at the bottom, are padding
    bool at_marker = false;
    BitReader(const uint8_t *data, size_t len, size_t start) : p(data), n(len), at(start) {}
    void fill()
    {
        while (bits <= 56) {
            int byte = 0;
            if (!at_marker && at < n) {
                byte = p[at];
                if (byte == 0xFF) {
                    if (at + 1 < n && p[at + 1] == 0x00) {
                        at += 2;
                    } else {
                        at_marker = true;   // a marker, or the stream's last byte: `at` stays on the 0xFF
                        byte = 0;
                    }
                } else {
                    ++at;
                }
            } else {
                at_marker = true;
            }
            if (at_marker) pad += 8;
            acc = (acc << 8) | (uint64_t)byte;
            bits += 8;
        }
    }
    bool overrun() const { return pad > bits; }   // more padding was fed than is still unread: some of it was consumed
    // peek / skip need 1 <= k <= 16 and a fill() since the last 40 consumed bits
    uint32_t peek(int k) const { return (uint32_t)(acc >> (bits - k)) & ((1u << k) - 1u); }
    void skip(int k) { bits -= k; }
    // the marker that must follow the data read so far (RSTn after an interval, EOI after the last one): drop the bits of the last
    // byte, step over the marker
    bool marker(int code)
    {
        if (overrun()) return false;
        if (bits - pad >= 8) return false;   // whole unread data bytes in front of the marker
        acc = 0;
        bits = 0;
        pad = 0;
        at_marker = false;
        while (at + 1 < n && p[at] == 0xFF && p[at + 1] == 0xFF) ++at;
        if (at + 1 >= n || p[at] != 0xFF || p[at + 1] != code) return false;
        at += 2;
        return true;
    }
};

inline int decode_symbol(BitReader &br, const Huff &t)
{
    const uint32_t look = t.look[br.peek(LOOK)];
    if (look) {
        br.skip((int)(look >> 8));
        return (int)(look & 255u);
    }
    int len = LOOK + 1;
    int32_t code = (int32_t)br.peek(len);
    while (len <= 16 && code > t.maxcode[len]) {
        ++len;
        if (len <= 16) code = (int32_t)br.peek(len);
    }
    if (len > 16) return -1;
    const int idx = t.valoff[len] + code;
    if (idx < 0 || idx >= t.nvals) return -1;
    br.skip(len);
    return t.vals[idx];
}

inline int receive_extend(BitReader &br, int s)
{
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// GSR_JPEG_MAX_COLUMN_L1 / GSR_JPEG_MAX_BLOCK_L1 (include/gsr.h): the coefficient gate of DESIGN.md R23
struct Gate {
    int64_t col[8];
    void reset() { memset(col, 0, sizeof(col)); }
    void add(int natural, int value, int q)
    {
        const int64_t d = (int64_t)value * q;
        col[natural & 7] += d < 0 ? -d : d;
    }
    bool pass() const
    {
        int64_t sum = 0;
        for (int c = 0; c < 8; ++c) {
            if (col[c] > GSR_JPEG_MAX_COLUMN_L1) return false;
            sum += col[c];
        }
        return sum <= GSR_JPEG_MAX_BLOCK_L1;
    }
};

// one stream -> its coefficient blocks at coefs[0 .. capacity) and its descriptor.  `coefs` is the image's own region.
inline int decode_image(const uint8_t *data, size_t len, int H, int W, int16_t *coefs, int64_t capacity, gsr_jpeg_desc *desc)
{
    const int64_t offset = desc->coef_offset;
    memset(desc, 0, sizeof(*desc));
    desc->coef_offset = offset;
    desc->sampling = -1;
    if (!data) return GSR_JPEG_CORRUPT;
    // a Header is 10 KB of tables: thread-local storage of the worker, not its stack
    static thread_local Header h;
    h = Header();
    const int rc = parse_header(data, len, h);
    if (rc != GSR_OK) return rc;
    if (h.width != W || h.height != H) return GSR_JPEG_UNSUPPORTED;   // not a picture of this call's size
    int32_t bw[3], bh[3];
    const int64_t count = block_grids(h.sampling, H, W, bw, bh);
    if (count > capacity) return GSR_JPEG_UNSUPPORTED;
    memset(coefs, 0, (size_t)count * sizeof(int16_t));
    int64_t plane[3];
    plane[0] = 0;
    plane[1] = 64 * (int64_t)bw[0] * bh[0];
    plane[2] = plane[1] + 64 * (int64_t)bw[1] * bh[1];
    const int nc = h.ncomp;
    const int hs = nc == 1 ? 1 : h.comp[0].h, vs = nc == 1 ? 1 : h.comp[0].v;
    const int mcus_x = bw[0] / hs, mcus_y = bh[0] / vs;
    BitReader br(data, len, h.scan);
    int pred[3] = {0, 0, 0};
    int until_restart = h.restart, next_rst = 0;
    Gate gate;
    bool gated = false;
    for (int my = 0; my < mcus_y; ++my) {
        for (int mx = 0; mx < mcus_x; ++mx) {
            if (h.restart && until_restart == 0) {
                if (!br.marker(0xD0 + next_rst)) return GSR_JPEG_CORRUPT;
                next_rst = (next_rst + 1) & 7;
                until_restart = h.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < nc; ++c) {
                const Component &k = h.comp[c];
                const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
                const Huff &dc = h.dc[k.td], &ac = h.ac[k.ta];
                const uint16_t *q = h.quant[k.tq];
                for (int by = 0; by < cv; ++by) {
                    for (int bx = 0; bx < ch; ++bx) {
                        const int64_t block = (int64_t)(my * cv + by) * bw[c] + (mx * ch + bx);
                        const int64_t base = plane[c] + 64 * block;
                        if (block < 0 || block >= (int64_t)bw[c] * bh[c] || base + 64 > count) return GSR_JPEG_CORRUPT;
                        int16_t *out = coefs + base;
                        gate.reset();
                        br.fill();
                        int s = decode_symbol(br, dc);
                        if (s < 0 || s > 15) return GSR_JPEG_CORRUPT;
                        if (s) {
                            br.fill();
                            pred[c] += receive_extend(br, s);
                        }
                        if (pred[c] < -32768 || pred[c] > 32767) return GSR_JPEG_CORRUPT;
                        out[0] = (int16_t)pred[c];
                        gate.add(0, pred[c], q[0]);
                        for (int kk = 1; kk < 64;) {
                            br.fill();
                            const int rs = decode_symbol(br, ac);
                            if (rs < 0) return GSR_JPEG_CORRUPT;
                            const int run = rs >> 4, size = rs & 15;
                            if (size == 0) {
                                if (run != 15) break;   // end of block
                                kk += 16;
                                continue;
                            }
                            kk += run;
                            if (kk > 63) return GSR_JPEG_CORRUPT;
                            const int v = receive_extend(br, size);   // |v| < 2^15: fits the int16
                            const int nat = ZIGZAG[kk];
                            out[nat] = (int16_t)v;
                            gate.add(nat, v, q[nat]);
                            ++kk;
                        }
                        if (br.overrun()) return GSR_JPEG_CORRUPT;
                        if (!gate.pass()) gated = true;
                    }
                }
            }
            if (h.restart) --until_restart;
        }
    }
    // the reference decoder refuses a stream whose EOI is missing: such a stream is left to it
    if (!br.marker(0xD9)) return GSR_JPEG_CORRUPT;
    if (gated) return GSR_JPEG_UNSUPPORTED;
    desc->sampling = h.sampling;
    desc->ncomp = nc;
    for (int c = 0; c < 3; ++c) {
        desc->bw[c] = bw[c];
        desc->bh[c] = bh[c];
        for (int i = 0; i < 64; ++i) desc->quant[c][i] = c < nc ? h.quant[h.comp[c].tq][i] : (uint16_t)0;
    }
    desc->coef_count = count;
    return GSR_OK;
}

inline int probe(const uint8_t *data, size_t len, gsr_jpeg_info *info)
{
    if (!info) return GSR_EINVAL;
    memset(info, 0, sizeof(*info));
    info->sampling = -1;
    if (!data) return GSR_EINVAL;
    static thread_local Header h;
    h = Header();
    const int rc = parse_header(data, len, h);
    info->width = h.width;
    info->height = h.height;
    info->components = h.ncomp;
    info->restart_interval = h.restart;
    info->sampling = rc == GSR_OK ? h.sampling : -1;
    return rc;
}

inline int clamp_threads(int threads, int64_t N)
{
    int t = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    return (int64_t)t > N ? (int)N : t;
}

// N streams of one picture size.  A first, serial pass over the headers gives every image its region of `coefs`, one behind the other
// (a 4:2:0 picture takes half of what a 4:4:4 one does, and the caller uploads only what is used); the workers then decode whole
// images into their own regions.  An image that does not decode keeps its region: nothing moves after the first pass.
inline int entropy(const uint8_t *const *data, const size_t *len, int64_t N, int H, int W, int16_t *coefs, gsr_jpeg_desc *desc,
                   int32_t *status, int threads)
{
    if (!data || !len || !coefs || !desc || !status) return GSR_EINVAL;
    if (N < 1 || N > (1LL << 24) || H < 1 || W < 1 || H > 65535 || W > 65535) return GSR_EINVAL;
    std::vector<int64_t> room((size_t)N);
    {
        static thread_local Header h;
        int64_t offset = 0;
        for (int64_t n = 0; n < N; ++n) {
            int32_t bw[3], bh[3];
            h = Header();
            const bool ok = data[n] && parse_header(data[n], len[n], h) == GSR_OK && h.width == W && h.height == H;
            room[(size_t)n] = ok ? block_grids(h.sampling, H, W, bw, bh) : 0;
            desc[n].coef_offset = offset;
            offset += room[(size_t)n];
        }
    }
    auto work = [&](int64_t n) {
        status[n] = decode_image(data[n], len[n], H, W, coefs + desc[n].coef_offset, room[(size_t)n], &desc[n]);
    };
    const int T = clamp_threads(threads, N);
    if (T == 1) {
        for (int64_t n = 0; n < N; ++n) work(n);
        return GSR_OK;
    }
    std::atomic<int64_t> next(0);
    auto loop = [&]() {
        for (int64_t n = next.fetch_add(1); n < N; n = next.fetch_add(1)) work(n);
    };
    std::vector<std::thread> pool;
    pool.reserve((size_t)T - 1);
    for (int t = 1; t < T; ++t) pool.emplace_back(loop);
    loop();
    for (auto &th : pool) th.join();
    return GSR_OK;
}

}  // namespace gsr_jpeg

#endif /* GSR_JPEG_ENTROPY_H */

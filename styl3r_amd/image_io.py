"""Writing pictures and videos: the reference's src/misc/image_io.py (`prep_image`, `save_image`, `load_image`, `save_video`) with the PNG
and the baseline-JPEG encoder on the device.

`encode_png` turns N frames of one size into N complete PNG files.  Device tensors go through csrc/gsr_png.hip: `gsr_png_chunks` (one
workgroup per chunk of whole rows: filter, byte-run tokens, Huffman code, dynamic deflate block) and `gsr_png_assemble` (the zlib stream
of each image from its chunks), two launches per call whatever N is, and two read-backs: the stream lengths, then the used bytes.  CPU
tensors take `_deflate_host`, an integer restatement of exactly the same algorithm -- the two are equal byte for byte, which is what the
tests hold them to.  The container (signature, IHDR, one IDAT, IEND, CRC-32 through zlib.crc32) is host work.

The stream of one image: `78 01`, then per chunk either one dynamic-Huffman block followed by an empty stored block
(the byte-alignment marker of Z_SYNC_FLUSH) or, when that is not smaller, one stored block; then the final empty stored block
`01 00 00 FF FF` and the Adler-32 of the filtered bytes.  A chunk is the largest number of whole rows whose filtered bytes
rows * (1 + W * C) fit GSR_PNG_CHUNK_BYTES; an image whose single row does not fit goes to Pillow and is counted in
CALLS["png_fallback"].  Only 8-bit RGB / RGBA, no interlace, no ancillary chunks.

`encode_jpeg` turns N frames of one size into N baseline JPEG files that are Pillow's (libjpeg's) bytes: csrc/gsr_jpeg_enc.hip writes the
entropy-coded scans, `jpeg_header` the markers in front of them.  CPU tensors go to Pillow itself.  `save_video` puts the
files of one `encode_jpeg` call into a Motion-JPEG AVI (the reference writes H.264 .mp4 through ffmpeg, which this build does not have);
`read_avi` is its inverse.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from io import BytesIO
from pathlib import Path
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import GSR_PNG_CHUNK_BYTES as CHUNK_BYTES

# images encoded on the device / by the restatement / by Pillow; JPEG: on the device / by Pillow for CPU tensors / by Pillow for a refused size
CALLS = {"png_hip": 0, "png_host": 0, "png_fallback": 0, "jpeg_enc_hip": 0, "jpeg_enc_host": 0, "jpeg_enc_fallback": 0}
DEBUG_FILL: Optional[int] = None    # tests: a byte value the device buffers are filled with before the launches (an unwritten byte shows)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTERS = {"adaptive": 0, "none": 1}
LL_SYMBOLS, CL_SYMBOLS, LL_LIMIT, CL_LIMIT = 286, 19, 15, 7
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
ADLER = 65521


# ---- the reference's three functions -------------------------------------------------------------------------------------------------
def prep_image(image: Tensor) -> Tensor:
    """image_io.py:38-54: (H,W), (C,H,W) with C in {1,3,4} (1 repeated to 3) or (B,C,H,W) laid side by side as `c h (b w)` ->
    uint8 (H,W,C), `(x.clip(0, 1) * 255)` truncated.  Returned as a tensor on the input's device (the reference returns numpy);
    a NaN becomes 0, the rule of export.pack_frames (the reference's cast is undefined there)."""
    image = image.detach()
    if image.ndim == 4:
        image = image.permute(1, 2, 0, 3).reshape(image.shape[1], image.shape[2], -1)
    if image.ndim == 2:
        image = image[None]
    if image.ndim != 3:
        raise ValueError(f"prep_image: an image is (H,W), (C,H,W) or (B,C,H,W), not {tuple(image.shape)}")
    if image.shape[0] == 1:
        image = image.expand(3, -1, -1)
    if image.shape[0] not in (3, 4):
        raise ValueError(f"prep_image: {image.shape[0]} channels; an image has 1, 3 or 4")
    image = torch.where(image.isnan(), torch.zeros_like(image), image)
    return (image.clip(min=0, max=1) * 255).type(torch.uint8).permute(1, 2, 0).contiguous()


def load_image(path) -> Tensor:
    """image_io.py:71-74 (host only): the file through Pillow as fp32 (3,H,W) in [0, 1] (ToTensor's byte / 255, first three channels)"""
    from PIL import Image
    a = np.asarray(Image.open(path))
    if a.dtype != np.uint8:
        raise ValueError(f"load_image: {path} is not an 8-bit picture")
    a = a[:, :, None] if a.ndim == 2 else a
    return (torch.from_numpy(a.copy()).permute(2, 0, 1).float() / 255)[:3]


def save_image(image: Tensor, path) -> None:
    """image_io.py:57-68: save an image in range 0-1, the parent directory created.  A `.png` path takes `encode_png`; a `.jpg` / `.jpeg`
    path with a three-channel device tensor takes `encode_jpeg` at Pillow's defaults (quality 75, 4:2:0), so the file is the one Pillow
    writes; any other suffix, and CPU tensors under .jpg, go to Pillow (the drivers save the style image under its own name, often .jpg)."""
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    if path.suffix.lower() in (".jpg", ".jpeg") and image.is_cuda:
        planar = image.ndim == 3 and image.shape[0] == 3 and image.dtype == torch.float32
        frames = image.detach()[None] if planar else prep_image(image)[None]
        if planar or frames.shape[-1] == 3:                      # (four channels: Pillow refuses them below, as it always did)
            path.write_bytes(encode_jpeg(frames, quality=75, subsampling="4:2:0")[0])
            return
    if path.suffix.lower() != ".png":
        from PIL import Image
        Image.fromarray(prep_image(image).cpu().numpy()).save(path)
        return
    if image.ndim == 3 and image.shape[0] in (3, 4) and image.dtype == torch.float32:
        data = encode_png(image.detach()[None])[0]              # converted in the kernel's load, no byte image in between
    else:
        data = encode_png(prep_image(image)[None])[0]
    path.write_bytes(data)


def save_images(frames: Tensor, paths: Sequence, filter: str = "adaptive") -> None:
    """N frames of one size (as `encode_png` takes them) in ONE encoder call, written to `paths` in order"""
    paths = [Path(p) for p in paths]
    if len(paths) != frames.shape[0]:
        raise ValueError(f"save_images: {frames.shape[0]} frames for {len(paths)} paths")
    for p in paths:
        if p.suffix.lower() != ".png":
            raise ValueError(f"save_images writes PNG files, not {p.name}")
    if not paths:
        return
    files = encode_png(frames, filter)
    made = set()
    for p, data in zip(paths, files):
        if p.parent not in made:
            p.parent.mkdir(exist_ok=True, parents=True)
            made.add(p.parent)
        p.write_bytes(data)


# ---- the container ---------------------------------------------------------------------------------------------------------------------
def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def wrap_png(stream: bytes, H: int, W: int, channels: int) -> bytes:
    """signature, IHDR (8-bit, colour type 2 or 6, no interlace), one IDAT holding `stream`, IEND"""
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if channels == 3 else 6, 0, 0, 0)
    return SIGNATURE + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", stream) + _png_chunk(b"IEND", b"")


def idat_payload(png: bytes) -> bytes:
    """the concatenated IDAT data of a PNG file (tests, benchmark)"""
    at, out = 8, b""
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        if kind == b"IDAT":
            out += png[at + 8:at + 8 + n]
        at += 12 + n
    return out


def chunk_rows(H: int, W: int, channels: int) -> int:
    """rows per chunk: the most whole rows whose filtered bytes fit GSR_PNG_CHUNK_BYTES (0: one row does not fit)"""
    return min(H, CHUNK_BYTES // (1 + W * channels))


def stream_bound(H: int, W: int, channels: int) -> int:
    """most bytes of one image's zlib stream: every chunk stored"""
    rows = chunk_rows(H, W, channels)
    return 2 + H * (1 + W * channels) + 5 * (-(-H // rows)) + 5 + 4


# ---- the restatement of csrc/gsr_png.hip -----------------------------------------------------------------------------------------------
def filter_rows(raw: np.ndarray, channels: int, mode: int) -> np.ndarray:
    """raw uint8 (H, W*C) -> filtered uint8 (H, 1 + W*C).  mode 0: per row the filter 0..4 (None, Sub, Up, Average, Paeth) with the
    smallest sum of min(b, 256 - b) over the filtered bytes, ties to the lowest number; the row above the first is zeros.  mode 1: None."""
    H, WC = raw.shape
    out = np.zeros((H, 1 + WC), np.uint8)
    if mode == 1:
        out[:, 1:] = raw
        return out
    x = raw.astype(np.int32)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, channels:] = x[:, :WC - channels]
    b[1:] = x[:-1]
    c[1:, channels:] = x[:-1, :WC - channels]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255
    cost = np.minimum(cand, 256 - cand).sum(axis=2)             # (5, H)
    choice = cost.argmin(axis=0)                                # the first of equal minima
    out[:, 0] = choice
    out[:, 1:] = np.take_along_axis(cand, choice[None, :, None], axis=0)[0]
    return out


def length_symbol(m):
    """deflate's length code of a match of m = 3 .. 258 bytes: (symbol, extra bits, extra value); numpy arrays or ints"""
    m = np.asarray(m, np.int64)
    v = m - 3
    e = np.maximum(np.floor(np.log2(np.maximum(v, 1))).astype(np.int64) - 2, 0)
    sym = np.where(v < 8, 257 + v, 261 + 4 * e + ((v >> e) & 3))
    extra = np.where(v < 8, 0, v & ((1 << e) - 1))
    e = np.where(v < 8, 0, e)
    full = m == 258
    return np.where(full, 285, sym), np.where(full, 0, e), np.where(full, 0, extra)


def tokenise(f: np.ndarray):
    """Byte runs of a chunk as deflate tokens with distance-1 matches only.  A run of L equal bytes is one literal, then the other
    R = L - 1 bytes longest first: matches of 258 while at least 258 remain, then one match of the rest if it is 3 or more,
    else the rest (1 or 2 bytes) as literals.  Returns (position, value) of the literals and (position, length) of the matches."""
    n = f.shape[0]
    starts = np.flatnonzero(np.concatenate([[True], f[1:] != f[:-1]]))
    R = np.diff(np.concatenate([starts, [n]])) - 1
    full, rem = R // 258, R % 258
    first = starts + 1
    m_pos = [np.repeat(first, full) + 258 * (np.arange(full.sum()) - np.repeat(np.cumsum(full) - full, full))]
    m_len = [np.full(int(full.sum()), 258, np.int64)]
    tail = rem >= 3
    m_pos.append((first + 258 * full)[tail])
    m_len.append(rem[tail])
    l_pos = [starts]
    for k in (0, 1):                                            # a rest of 1 or 2 bytes
        short = (rem < 3) & (rem > k)
        l_pos.append((first + 258 * full)[short] + k)
    l_pos = np.sort(np.concatenate(l_pos))
    m_pos, m_len = np.concatenate(m_pos), np.concatenate(m_len)
    order = np.argsort(m_pos, kind="stable")
    return l_pos, f[l_pos].astype(np.int64), m_pos[order], m_len[order]


def code_lengths(counts, limit: int):
    """The length-limited Huffman code both implementations build, stated exactly:
      1. the used symbols (count > 0) in ascending order of (count, symbol) are the leaves 0 .. m-1; one used symbol gets length 1;
      2. m - 1 times: take the two smallest of (next unmerged leaf, next unmerged node) -- a leaf wins against a node of equal weight --
         and make them children of a new node whose weight is their sum; nodes are created, and consumed, in order;
      3. num[d] = how many leaves are d edges below the root, depths above `limit` counted at `limit` (then the limit "acted");
      4. if it acted, with total = sum(num[d] << (limit - d)): until total == 1 << limit: num[limit] -= 1; the largest d < limit with
         num[d] > 0 gives num[d] -= 1, num[d + 1] += 2; total -= 1;
      5. lengths are handed out by rank: the num[1] leaves of largest (count, symbol) get length 1, the next num[2] get 2, ...
    Returns (lengths per symbol, num, acted)."""
    counts = [int(c) for c in counts]
    lens = [0] * len(counts)
    num = [0] * (limit + 1)
    order = sorted((s for s in range(len(counts)) if counts[s]), key=lambda s: (counts[s], s))
    m = len(order)
    if m == 1:
        lens[order[0]], num[1] = 1, 1
        return lens, num, False
    w = [counts[s] for s in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    leaf, node = 0, m
    for new in range(m, 2 * m - 1):
        for _ in (0, 1):
            if leaf < m and (node >= new or w[leaf] <= w[node]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, node = node, node + 1
            parent[pick] = new
            w[new] += w[pick]
    acted = False
    for i in range(m):
        d, p = 0, i
        while p != 2 * m - 2:
            p, d = parent[p], d + 1
        if d > limit:
            d, acted = limit, True
        num[d] += 1
    if acted:
        total = sum(num[d] << (limit - d) for d in range(1, limit + 1))
        while total != 1 << limit:
            num[limit] -= 1
            for d in range(limit - 1, 0, -1):
                if num[d]:
                    num[d] -= 1
                    num[d + 1] += 2
                    break
            total -= 1
    j = m
    for d in range(1, limit + 1):
        for _ in range(num[d]):
            j -= 1
            lens[order[j]] = d
    return lens, num, acted


def canonical_codes(lens, num, limit: int):
    """deflate's canonical codes, bit-reversed (the stream takes Huffman codes most significant bit first, everything else least)"""
    nxt, code = [0] * (limit + 2), 0
    for d in range(1, limit + 1):
        code = (code + num[d - 1]) << 1
        nxt[d] = code
    out = [0] * len(lens)
    for s, d in enumerate(lens):
        if d:
            out[s] = int(format(nxt[d], f"0{d}b")[::-1], 2)
            nxt[d] += 1
    return out


def code_length_tokens(seq):
    """The 287 code lengths (286 literal/length, 1 distance) in the code-length alphabet, greedy: a run of r zeros is coded 18 (11..138)
    while r >= 11, then 17 (3..10) while r >= 3, then single zeros; a run of r equal lengths v > 0 is v, then 16 (3..6 repeats) while
    r >= 3 remain, then single v.  Returns [(symbol, extra bits, extra value)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                m = min(r, 138)
                out.append((18, 7, m - 11))
                r -= m
            while r >= 3:
                m = min(r, 10)
                out.append((17, 3, m - 3))
                r -= m
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                m = min(r, 6)
                out.append((16, 2, m - 3))
                r -= m
        out.extend([(v, 0, 0)] * r)
    return out


def _pack(pos, val, nbytes: int) -> np.ndarray:
    """OR `val` (below 2^24) into a little-endian bit string at bit offsets `pos` (the pieces do not overlap, so adding is ORing)"""
    buf = np.zeros(nbytes + 4, np.int64)
    shifted = val << (pos & 7)
    for k in range(4):
        buf += np.bincount((pos >> 3) + k, weights=((shifted >> (8 * k)) & 255).astype(np.float64), minlength=nbytes + 4).astype(np.int64)
    return buf[:nbytes].astype(np.uint8)


def deflate_chunk(f: np.ndarray, details: Optional[dict] = None) -> bytes:
    """one chunk of filtered bytes -> its deflate blocks (csrc/gsr_png.hip k_png_chunks, steps 3-7)"""
    n = f.shape[0]
    l_pos, l_val, m_pos, m_len = tokenise(f)
    m_sym, m_ebits, m_extra = length_symbol(m_len)
    hist = np.bincount(l_val, minlength=LL_SYMBOLS) + np.bincount(m_sym, minlength=LL_SYMBOLS)
    hist[256] = 1
    lens, num, acted = code_lengths(hist, LL_LIMIT)
    codes = canonical_codes(lens, num, LL_LIMIT)
    dist_len = 1 if len(m_pos) else 0                           # only distance code 0: length 1 (its code is the bit 0); none: HDIST 1, length 0
    cl_tok = code_length_tokens(lens + [dist_len])
    cl_hist = np.bincount([t[0] for t in cl_tok], minlength=CL_SYMBOLS)
    cl_lens, cl_num, cl_acted = code_lengths(cl_hist, CL_LIMIT)
    cl_codes = canonical_codes(cl_lens, cl_num, CL_LIMIT)
    hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    lens_a, codes_a = np.array(lens, np.int64), np.array(codes, np.int64)
    header_bits = 17 + 3 * hclen + sum(cl_lens[s] + e for s, e, _ in cl_tok)
    l_bits = lens_a[l_val]
    m_bits = lens_a[m_sym] + m_ebits + dist_len
    total = header_bits + int(l_bits.sum()) + int(m_bits.sum()) + lens[256]
    coded_bytes = (total + 3 + 7) // 8 + 4
    if details is not None:
        details["chunks"] = details.get("chunks", 0) + 1
        details["limit_acted"] = details.get("limit_acted", 0) + int(acted)
        details["cl_limit_acted"] = details.get("cl_limit_acted", 0) + int(cl_acted)
        details["matches"] = details.get("matches", 0) + len(m_pos)
        details["max_length"] = max(details.get("max_length", 0), max(lens))
    if coded_bytes >= n + 5:
        if details is not None:
            details["stored"] = details.get("stored", 0) + 1
        return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + f.tobytes()
    # header: BFINAL 0, BTYPE 2, HLIT 29 (286 codes), HDIST 0 (1 code), HCLEN
    pos, val, at = [], [], 0

    def put(v, nbits):
        nonlocal at
        pos.append(at)
        val.append(v)
        at += nbits
    put(0 | (2 << 1), 3)
    put(29, 5)
    put(0, 5)
    put(hclen - 4, 4)
    for k in range(hclen):
        put(cl_lens[CL_ORDER[k]], 3)
    for s, e, x in cl_tok:
        put(cl_codes[s] | (x << cl_lens[s]), cl_lens[s] + e)
    assert at == header_bits
    # tokens in stream order
    t_pos = np.concatenate([l_pos, m_pos])
    t_val = np.concatenate([codes_a[l_val], codes_a[m_sym] | (m_extra << lens_a[m_sym])])
    t_bits = np.concatenate([l_bits, m_bits])
    order = np.argsort(t_pos, kind="stable")
    t_val, t_bits = t_val[order], t_bits[order]
    t_at = header_bits + np.cumsum(t_bits) - t_bits
    put_pos = np.concatenate([np.array(pos, np.int64), t_at, [total - lens[256]]])
    put_val = np.concatenate([np.array(val, np.int64), t_val, [codes[256]]])
    out = _pack(put_pos, put_val, coded_bytes)
    out[-2:] = 255                                              # the empty stored block: 000, padding, 00 00 FF FF
    return out.tobytes()


def adler_partial(f: np.ndarray):
    """(sum d_i, sum (n - i) d_i) mod 65521 over a chunk: what the Adler-32 of the whole is combined from"""
    n = f.shape[0]
    d = f.astype(np.int64)
    return int(d.sum() % ADLER), int((d * (n - np.arange(n))).sum() % ADLER)


def _deflate_host(frames: np.ndarray, mode: int, details: Optional[dict] = None) -> list:
    """uint8 (N,H,W,C) -> the zlib stream of every image, as the two kernels write it"""
    N, H, W, ch = frames.shape
    rows = chunk_rows(H, W, ch)
    out = []
    for img in frames:
        filt = filter_rows(img.reshape(H, W * ch), ch, mode)
        parts, A, B = [b"\x78\x01"], 1, 0
        for r0 in range(0, H, rows):
            f = filt[r0:r0 + rows].reshape(-1)
            parts.append(deflate_chunk(f, details))
            a, b = adler_partial(f)
            B = (B + f.shape[0] * A + b) % ADLER
            A = (A + a) % ADLER
        parts.append(b"\x01\x00\x00\xff\xff" + struct.pack(">I", (B << 16) | A))
        out.append(b"".join(parts))
    return out


# ---- the encoder -----------------------------------------------------------------------------------------------------------------------
def _bytes_host(frames: Tensor) -> np.ndarray:
    if frames.dtype == torch.uint8:
        return frames.cpu().numpy()
    from .export import _rgb_bytes_host
    return _rgb_bytes_host(frames.cpu()).contiguous().numpy()


def _pillow(frames: np.ndarray) -> list:
    from PIL import Image
    out = []
    for img in frames:
        buf = BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        out.append(buf.getvalue())
    return out


def encode_png(frames: Tensor, filter: str = "adaptive", details: Optional[dict] = None) -> list:
    """N frames of one size -> N PNG files as bytes.  `frames`: uint8 (N,H,W,C) or fp32 (N,C,H,W), C in {3, 4}; fp32 values are
    converted as `prep_image` does, in the kernel's load.  Device tensors take the kernels (and raise if the library is missing), CPU
    tensors the restatement; the bytes are the same.  filter: "adaptive" (per row, smallest sum of min(b, 256 - b)) or "none".
    `details` (CPU path): a dict that receives counts over the chunks -- `chunks`, `stored`, `matches`, `limit_acted`, `max_length`."""
    if filter not in FILTERS:
        raise ValueError(f"encode_png: filter is 'adaptive' or 'none', not {filter!r}")
    if not isinstance(frames, Tensor) or frames.ndim != 4 or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError("encode_png takes uint8 (N,H,W,C) or float32 (N,C,H,W) frames")
    planar = frames.dtype == torch.float32
    N, (H, W, ch) = frames.shape[0], ((frames.shape[2], frames.shape[3], frames.shape[1]) if planar else frames.shape[1:])
    if ch not in (3, 4) or N < 1 or H < 1 or W < 1:
        raise ValueError(f"encode_png: {N} frames of {H} x {W} with {ch} channels; frames are RGB or RGBA and not empty")
    frames = frames.detach().contiguous()
    if chunk_rows(H, W, ch) == 0:                               # one row is wider than a chunk: Pillow, counted
        CALLS["png_fallback"] += N
        return _pillow(_bytes_host(frames))
    if not frames.is_cuda:
        CALLS["png_host"] += N
        return [wrap_png(s, H, W, ch) for s in _deflate_host(_bytes_host(frames), FILTERS[filter], details)]
    lib, dev = _lib.load(), frames.device
    bound = lib.gsr_png_stream_bound(H, W, ch)
    nbytes = lib.gsr_png_scratch_bytes(N, H, W, ch)
    if not bound or not nbytes:
        raise RuntimeError(f"encode_png: gsr_png_scratch_bytes refuses {N} frames of {H} x {W} x {ch}")
    stride = (bound + 15) & ~15
    make = (lambda n: torch.empty(n, dtype=torch.uint8, device=dev)) if DEBUG_FILL is None else \
        (lambda n: torch.full((n,), DEBUG_FILL, dtype=torch.uint8, device=dev))
    scratch, out, lengths = make(nbytes), make(N * stride), make(4 * N).view(torch.int32)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.gsr_png_chunks(frames.data_ptr(), _lib.GSR_PNG_SRC_F32_PLANAR if planar else _lib.GSR_PNG_SRC_U8, N, H, W, ch,
                                  FILTERS[filter], scratch.data_ptr(), nbytes, stream), "gsr_png_chunks")
    _lib.check(lib.gsr_png_assemble(scratch.data_ptr(), nbytes, N, H, W, ch, out.data_ptr(), stride, lengths.data_ptr(), stream),
               "gsr_png_assemble")
    sizes = lengths.cpu().tolist()                              # read-back 1
    if min(sizes) < 11 or max(sizes) > bound:
        raise RuntimeError(f"encode_png: stream lengths {min(sizes)} .. {max(sizes)} outside [11, {bound}]")
    used = out.view(N, stride)[:, :max(sizes)].cpu().numpy()    # read-back 2
    CALLS["png_hip"] += N
    return [wrap_png(used[i, :n].tobytes(), H, W, ch) for i, n in enumerate(sizes)]


# ---- baseline JPEG ---------------------------------------------------------------------------------------------------------------------
JPEG_SAMPLING = {"4:4:4": (_lib.GSR_JPEG_444, 1, 1, 0), "4:2:2": (_lib.GSR_JPEG_422, 2, 1, 1), "4:2:0": (_lib.GSR_JPEG_420, 2, 2, 2)}   # library's code, Y factors, Pillow's number
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
QUANT_BASE = (      # ITU-T T.81 Annex K tables K.1 (luminance) and K.2 (chrominance), row-major
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99)
    + (99,) * 32)
HUFF_BITS = {   # Annex K tables K.3 - K.6: codes per length 1 .. 16, keyed (class: 0 DC / 1 AC, table: 0 luminance / 1 chrominance)
    (0, 0): (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 0): (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
    (0, 1): (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), (1, 1): (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)}
HUFF_VALS = {
    (0, 0): tuple(range(12)), (0, 1): tuple(range(12)),
    (1, 0): (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51,
             98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84,
             85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136,
             137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183,
             184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229,
             230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250),
    (1, 1): (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98,
             114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
             83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133,
             134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
             181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227,
             228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250)}
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10
JPEG_BATCH_BYTES = 1 << 31          # encode_jpeg: most device memory (scratch + worst-case output) of one library call; more frames go in batches
AVI_LIMIT = 1 << 31                 # AVI 1.0: one RIFF chunk; OpenDML is not written


def _jpeg_args(quality, subsampling, who: str):
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"{who}: quality is an integer in 1 .. 100, not {quality!r}")
    if subsampling not in JPEG_SAMPLING:
        raise ValueError(f"{who}: subsampling is '4:4:4', '4:2:2' or '4:2:0', not {subsampling!r}")


def jpeg_quant_tables(quality: int) -> np.ndarray:
    """libjpeg's jpeg_set_quality: uint16 (2, 64), luminance and chrominance in natural order.  scale = 5000 / quality below 50, else
    200 - 2 quality; an entry is (base * scale + 50) / 100 in integers, clamped to 1 .. 255."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(QUANT_BASE, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16)


def jpeg_header(H: int, W: int, quality: int = 90, subsampling: str = "4:2:0") -> bytes:
    """Everything a baseline JPEG file holds in front of its scan, as Pillow / libjpeg write it: SOI, APP0 (JFIF 1.1, no units, density
    1 x 1, no thumbnail), the two quantisation tables (8-bit, zig-zag), SOF0 (components 1, 2, 3; tables 0, 1, 1), the four Annex K
    Huffman tables in the order DC0, AC0, DC1, AC1, and SOS (Ss 0, Se 63, Ah / Al 0)."""
    _jpeg_args(quality, subsampling, "jpeg_header")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"jpeg_header: a JPEG picture is 1 .. 65535 pixels on a side, not {H} x {W}")
    _, hs, vs, _ = JPEG_SAMPLING[subsampling]
    seg = lambda marker, data: bytes((0xFF, marker)) + struct.pack(">H", len(data) + 2) + data
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00" + struct.pack(">HHBB", 1, 1, 0, 0))
    for t, table in enumerate(jpeg_quant_tables(quality)):
        out += seg(0xDB, bytes((t,)) + bytes(int(table[ZIGZAG[k]]) for k in range(64)))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes((1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for table in (0, 1):
        for cls in (0, 1):
            out += seg(0xC4, bytes((cls << 4 | table,)) + bytes(HUFF_BITS[cls, table]) + bytes(HUFF_VALS[cls, table]))
    return out + seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def _pillow_jpeg(frames: np.ndarray, quality: int, subsampling: str) -> list:
    from PIL import Image
    out = []
    for img in frames:
        buf = BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=JPEG_SAMPLING[subsampling][3])
        out.append(buf.getvalue())
    return out


def encode_jpeg(frames: Tensor, quality: int = 90, subsampling: str = "4:2:0") -> list:
    """N frames of one size -> N baseline JPEG files as bytes, the ones Pillow's `save(format="JPEG", quality=, subsampling=)` writes.
    `frames`: uint8 (N,H,W,3) or fp32 (N,3,H,W); fp32 values are converted as `prep_image` does, in the kernel's load.  Device tensors
    take the kernels -- four launches and two read-backs (the scan lengths, then the used bytes) for as many frames as fit
    JPEG_BATCH_BYTES of scratch and worst-case output, 58 frames of 1080 x 1920 or 1 800 of 256 x 256 at 4:2:0 -- and raise if the
    library is missing; CPU tensors take Pillow.  A picture the kernels refuse (more than 2.5 million blocks) goes to Pillow and is
    counted in CALLS["jpeg_enc_fallback"]."""
    _jpeg_args(quality, subsampling, "encode_jpeg")
    if not isinstance(frames, Tensor) or frames.ndim != 4 or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError("encode_jpeg takes uint8 (N,H,W,3) or float32 (N,3,H,W) frames")
    planar = frames.dtype == torch.float32
    N, (H, W, ch) = frames.shape[0], ((frames.shape[2], frames.shape[3], frames.shape[1]) if planar else frames.shape[1:])
    if ch != 3 or N < 1 or H < 1 or W < 1:
        raise ValueError(f"encode_jpeg: {N} frames of {H} x {W} with {ch} channels; frames are RGB and not empty")
    frames = frames.detach().contiguous()
    if not frames.is_cuda:
        CALLS["jpeg_enc_host"] += N
        return _pillow_jpeg(_bytes_host(frames), quality, subsampling)
    lib, dev, code = _lib.load(), frames.device, JPEG_SAMPLING[subsampling][0]
    bound = lib.gsr_jpeg_enc_stream_bound(H, W, code)
    if not bound or not lib.gsr_jpeg_enc_scratch_bytes(1, H, W, code):
        CALLS["jpeg_enc_fallback"] += N
        return _pillow_jpeg(_bytes_host(frames), quality, subsampling)
    stride = (bound + 15) & ~15
    per = max(1, JPEG_BATCH_BYTES // (stride + lib.gsr_jpeg_enc_scratch_bytes(1, H, W, code)))      # frames per library call
    make = (lambda n: torch.empty(n, dtype=torch.uint8, device=dev)) if DEBUG_FILL is None else \
        (lambda n: torch.full((n,), DEBUG_FILL, dtype=torch.uint8, device=dev))
    quant = np.ascontiguousarray(jpeg_quant_tables(quality))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    header, files = jpeg_header(H, W, quality, subsampling), []
    for at in range(0, N, per):
        part = frames[at:at + per]
        n = part.shape[0]
        nbytes = lib.gsr_jpeg_enc_scratch_bytes(n, H, W, code)
        scratch, out, lengths = make(nbytes), make(n * stride), make(4 * n).view(torch.int32)
        _lib.check(lib.gsr_jpeg_enc_scans(part.data_ptr(), _lib.GSR_JPEG_ENC_SRC_F32_PLANAR if planar else _lib.GSR_JPEG_ENC_SRC_U8, n, H, W, code,
                                          quant.ctypes.data, scratch.data_ptr(), nbytes, out.data_ptr(), stride, lengths.data_ptr(), stream),
                   "gsr_jpeg_enc_scans")
        sizes = lengths.cpu().tolist()                              # read-back 1
        if min(sizes) < 2 or max(sizes) > bound:
            raise RuntimeError(f"encode_jpeg: scan lengths {min(sizes)} .. {max(sizes)} outside [2, {bound}]")
        used = out.view(n, stride)[:, :max(sizes)].cpu().numpy()    # read-back 2
        files += [header + used[i, :k].tobytes() for i, k in enumerate(sizes)]
    CALLS["jpeg_enc_hip"] += N
    return files


# ---- Motion-JPEG AVI -------------------------------------------------------------------------------------------------------------------
def _riff(kind: bytes, data: bytes) -> bytes:
    return kind + struct.pack("<I", len(data)) + data + b"\x00" * (len(data) & 1)


def wrap_avi(files: Sequence, H: int, W: int, fps: float) -> bytes:
    """JPEG files of one size -> an AVI 1.0 file: RIFF AVI, LIST hdrl (avih with AVIF_HASINDEX; one LIST strl: strh vids / MJPG with
    dwRate / dwScale = fps, scale 1 for an integer fps and 1000 otherwise; strf: a 40-byte BITMAPINFOHEADER, MJPG, 24 bits, 1 plane),
    LIST movi of `00dc` chunks padded to even length, idx1 (every frame a key frame, offsets from the `movi` fourcc)."""
    if not fps > 0:
        raise ValueError(f"save_video: fps is positive, not {fps!r}")
    scale = 1 if float(fps).is_integer() else 1000
    rate, n = int(round(fps * scale)), len(files)
    largest = max((len(f) for f in files), default=0)
    total = 12 + (12 + 64 + 12 + 64 + 48) + 12 + sum(8 + len(f) + (len(f) & 1) for f in files) + 8 + 16 * n
    if total >= AVI_LIMIT:
        raise ValueError(f"save_video: the file would hold {total} bytes; this build writes AVI 1.0, below 2 GiB -- save fewer frames per file")
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), 0, 0, AVIF_HASINDEX, n, 0, 1, largest, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, scale, rate, 0, n, largest, -1, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _riff(b"avih", avih) + _riff(b"LIST", b"strl" + _riff(b"strh", strh) + _riff(b"strf", strf))
    movi, index, at = [b"movi"], [], 4
    for f in files:
        index.append(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, at, len(f)))
        movi.append(_riff(b"00dc", f))
        at += len(movi[-1])
    body = b"AVI " + _riff(b"LIST", hdrl) + _riff(b"LIST", b"".join(movi)) + _riff(b"idx1", b"".join(index))
    out = _riff(b"RIFF", body)
    assert len(out) == total, (len(out), total)
    return out


def save_video(images, path, fps: float = 30, quality: int = 90, subsampling: str = "4:2:0") -> None:
    """image_io.py's save_video: the frames as a video file, the parent directory created.  `images`: the reference's list of fp32
    (3,H,W) images in 0 .. 1, an fp32 (F,3,H,W) tensor, or the uint8 (F,H,W,3) tensor `inference.render_flythrough` returns.  One
    `encode_jpeg` call for all frames.  The file is Motion-JPEG in an AVI container, so the suffix must be `.avi` (the reference writes
    H.264 into .mp4 through ffmpeg)."""
    path = Path(path)
    if path.suffix.lower() != ".avi":
        raise ValueError(f"save_video: this build writes Motion-JPEG AVI; name the file .avi, not {path.name!r}")
    if not isinstance(images, Tensor):
        images = list(images)
        if not images or any(not isinstance(i, Tensor) or i.ndim != 3 for i in images):
            raise ValueError("save_video takes a non-empty list of (3,H,W) images, an (F,3,H,W) tensor or a uint8 (F,H,W,3) tensor")
        images = torch.stack([i.detach().float() for i in images])
    files = encode_jpeg(images, quality, subsampling)
    H, W = (images.shape[2], images.shape[3]) if images.dtype == torch.float32 else (images.shape[1], images.shape[2])
    data = wrap_avi(files, H, W, fps)
    path.parent.mkdir(exist_ok=True, parents=True)
    path.write_bytes(data)


def read_avi(path) -> tuple:
    """(fps, [the JPEG file of every frame]) of a Motion-JPEG AVI as `save_video` writes it: the `00dc` chunks of LIST movi in order,
    fps = dwRate / dwScale of the stream header"""
    data = Path(path).read_bytes()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"read_avi: {path} is not a RIFF AVI file")
    fps, frames = None, []

    def walk(at: int, end: int):
        nonlocal fps
        while at + 8 <= end:
            kind, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
            if kind == b"LIST":
                if data[at + 8:at + 12] in (b"hdrl", b"strl", b"movi"):
                    walk(at + 12, at + 8 + n)
            elif kind == b"strh" and data[at + 8:at + 12] == b"vids":
                scale, rate = struct.unpack("<II", data[at + 28:at + 36])
                fps = rate / scale
            elif kind == b"00dc":
                frames.append(data[at + 8:at + 8 + n])
            at += 8 + n + (n & 1)
    walk(12, min(len(data), 8 + struct.unpack("<I", data[4:8])[0]))
    if fps is None:
        raise ValueError(f"read_avi: {path} has no video stream header")
    return fps, frames

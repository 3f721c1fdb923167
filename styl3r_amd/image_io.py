"""Writing pictures: the reference's src/misc/image_io.py (`prep_image`, `save_image`, `load_image`) with the PNG encoder on the device.

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

CALLS = {"png_hip": 0, "png_host": 0, "png_fallback": 0}     # images encoded on the device / by the restatement / by Pillow
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
    """image_io.py:57-68: save an image in range 0-1, the parent directory created.  A `.png` path takes `encode_png`; any other
    suffix goes to Pillow (the drivers save the style image under its own name, often .jpg)."""
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
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

"""The bytes of a packed weight image, restated in torch with no HIP code (test_weight_image_host.py, test_gpu_weight_images.py, test_gpu_vit.py).

Every Linear and convolution on the split-arithmetic path reads its weight as an image: the pieces of an (R, Kc) fp32 matrix -- R output rows, Kc
the contraction length, Kc % 8 == 0 -- in groups of eight consecutive k, three 16-byte slots per group, and the weight's 8 KiB |max| word right
behind the pieces (csrc/vit_weight_image.h).  `values` is always the matrix AS THE GEMM READS IT: a caller that tests a transposed or a
convolution image transposes or rearranges the weight first.

  modes    "bf16x6", "bf16x3": three bf16 pieces, each the round-to-nearest-even bf16 of what the pieces before it left over;
           "f16x3": two fp16 pieces of values * s, s the power of two of `f16_scale_of` (csrc/vit_common.h) from the largest of the |max|
           word's 64 slots; slot 2 of every group belongs to nobody in this mode: kernels neither write nor read it, `compared` leaves it out
  layouts  row   [row][k / 8][piece][8]
           block [row / 64][k / 8][piece][row % 64][8], rows padded to a multiple of 64 with zero pieces"""
import torch

MODES = ("bf16x6", "bf16x3", "f16x3")
PRODUCTS = {"bf16x6": 6, "bf16x3": 3, "f16x3": 2}      # vit_x6_set_products
WORD_BYTES, WORD_SLOTS, WORD_STRIDE = 8192, 64, 32       # the |max| word: 64 uint32 slots, one per 128-byte line


def padded_rows(rows, block):
    return (rows + 63) // 64 * 64 if block else rows


def word_slots(word):
    """the 64 slots of a |max| word given as 8192 bytes or 2048 32-bit words (bit patterns of non-negative floats: int32 orders them)"""
    return word.contiguous().view(torch.int32).reshape(-1)[::WORD_STRIDE].cpu()


def f16_scale_of(amax_bits):
    """csrc/vit_common.h f16_scale_of: the power of two that puts the tensor's |max| into [2^14, 2^15), clamped to 2^+-100; 1 for a zero /
    denormal / non-finite maximum"""
    e = (int(amax_bits) >> 23) & 0xFF
    if e == 0 or e == 255:
        return 1.0
    return 2.0 ** (min(max(127 + 14 - (e - 127), 27), 227) - 127)


def _pieces(values, mode, amax_word):
    """(rows, Kc) fp32 -> (rows, Kc, 3) int16 bit patterns of the pieces (slot 2 zero in f16x3)"""
    v = values.detach().cpu().float()
    if mode == "f16x3":
        x = v * f16_scale_of(word_slots(amax_word).max())       # a power of two: exact
        h = x.half()
        l = (x - h.float()).half()                              # x - h is exact in fp32
        return torch.stack([h.view(torch.int16), l.view(torch.int16), torch.zeros_like(h).view(torch.int16)], -1)
    p0 = v.bfloat16()
    r1 = v - p0.float()
    p1 = r1.bfloat16()
    r2 = r1 - p1.float()
    p2 = r2.bfloat16()
    return torch.stack([p0.view(torch.int16), p1.view(torch.int16), p2.view(torch.int16)], -1)


def piece_planes(values, mode, amax_word=None):
    """the pieces of `_pieces` as float64 planes of the shape of `values`, in the units of `values` (f16x3: two planes, divided by the exact
    power-of-two scale again; bf16: three) -- for ANY operand of a split-arithmetic product: an activation's pieces are made by the same
    rule from the |max| word announced for it (csrc/vit_common.h), so `amax_word` is whatever word the launch would be handed"""
    p = _pieces(values, mode, amax_word)
    if mode == "f16x3":
        s = f16_scale_of(word_slots(amax_word).max())
        return [p[..., i].contiguous().view(torch.float16).double() / s for i in range(2)]
    return [(p[..., i].to(torch.int32) << 16).view(torch.float32).double() for i in range(3)]


def expected_image(values, block, mode, amax_word=None):
    """the exact uint8 body (the piece bytes, without the |max| word) of the image of `values` (R, Kc)"""
    assert mode in MODES and values.dim() == 2 and values.shape[1] % 8 == 0
    R, Kc = values.shape
    p = _pieces(values, mode, amax_word)
    if block:
        p = torch.cat([p, p.new_zeros(padded_rows(R, True) - R, Kc, 3)])
        p = p.view(-1, 64, Kc // 8, 8, 3).permute(0, 2, 4, 1, 3)          # [row block][k group][piece][row in block][8]
    else:
        p = p.view(R, Kc // 8, 8, 3).permute(0, 1, 3, 2)                  # [row][k group][piece][8]
    return p.contiguous().view(torch.uint8).reshape(-1)


def slots(body, block):
    """the body as (groups, 3 pieces, ...) 16-byte slots: what `compared` indexes"""
    b = body.cpu().view(-1, 16)
    return b.view(-1, 3, 64, 16) if block else b.view(-1, 3, 16)


def compared(body, block, mode):
    """the bytes of a body that belong to the expectation: all three slots of every group, two in f16x3"""
    return slots(body, block)[:, : 2 if mode == "f16x3" else 3]


def unpack_image(body, rows, kcols, block=False, mode="bf16x6", amax_word=None):
    """the inverse of `expected_image`: the pieces as fp64 planes (padded_rows(rows, block), kcols) in the units of `values` (f16x3: divided by
    the scale again) -- three planes, two in f16x3.  `body` may carry the |max| word behind the pieces."""
    Rp = padded_rows(rows, block)
    raw = body[: Rp * kcols * 6].cpu().view(torch.int16)
    if block:
        raw = raw.view(Rp // 64, kcols // 8, 3, 64, 8).permute(2, 0, 3, 1, 4)
    else:
        raw = raw.view(Rp, kcols // 8, 3, 8).permute(2, 0, 1, 3)
    raw = raw.reshape(3, Rp, kcols)
    if mode == "f16x3":
        s = f16_scale_of(word_slots(amax_word).max())
        return [raw[p].contiguous().view(torch.float16).double() / s for p in range(2)]
    return [(raw[p].to(torch.int32) << 16).view(torch.float32).double() for p in range(3)]


def ramp_matrix(rows, cols, seed):
    """randn times a column ramp over nine decades: every exponent a weight can have, fp16 subnormals of the scaled value included"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g) * torch.logspace(-6, 3, cols)[None]


def word_of(values):
    """a |max| word of `values` (2048 int32) as a producer leaves it: 64 partial maxima, the true maximum's bit pattern the largest"""
    bits = values.detach().cpu().float().abs().reshape(-1).view(torch.int32)
    word = torch.zeros(WORD_SLOTS * WORD_STRIDE, dtype=torch.int32)
    for j in range(WORD_SLOTS):
        part = bits[j::WORD_SLOTS]
        word[j * WORD_STRIDE] = int(part.max()) if part.numel() else 0
    return word

"""-m gpu: every call site of the fused Linear (vit_ops._linear_cfg routes it, vit_ops._launch_linear launches it) against the EXPLICIT C-ABI
sequence written out here -- weight image (split_weight / split_weight_block), vit_x6_set_operand_amax, vit_x6_set_output_amax, the raw entry
point -- on the same seeded inputs: the autograd forward, the input-gradient GEMM with and without a GeluLink, the serving path; every cfg a
site can reach (0: vit_linear_x6_fwd on the row image; 1 / 3 / 5: vit_linear_x6r_fwd on the block image); bf16x6 and f16x3.  Equal bits, equal
|max| words, equal CALLS counters, nothing left pending on the thread.  Shapes: the smallest at which each route is taken (the ring tables are
keyed on production widths; no launch here splits its contraction, so every kernel has one summation order)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTERS = ("linear_x6r", "linear_sm", "split_pair", "amax_pass", "amax_published")


@pytest.fixture(params=["bf16x6", "f16x3"])
def vo(request, monkeypatch):
    from styl3r_amd import vit_ops
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", request.param)
    assert vit_ops._x6() and vit_ops.PUBLISH_AMAX and vit_ops.PAIR_SPLIT and vit_ops.RING_DISPATCH
    yield vit_ops
    monkeypatch.undo()
    vit_ops._x6()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _raw(vo, a, w, cols, cfg, transposed=False, bias=None, res=None, act=0, want_pre=False, operand=None, want_word=False):
    """ONE Linear launch as the library wants it: the image of `cfg`'s kernel, the activation's |max| word (f16x3), the output word, the entry point"""
    lib = vo.load()
    M, K = a.shape
    out = torch.empty(M, cols, device=a.device)
    pre = torch.empty_like(out) if want_pre else None
    wp = (vo.split_weight_block if cfg else vo.split_weight)(w, transposed)
    if vo._f16():
        vo._announce(operand)
    word = vo._output_amax_word(a.device) if want_word else None
    args = (a.data_ptr(), wp.data_ptr(), _ptr(bias), _ptr(res), out.data_ptr(), _ptr(pre), M, cols, K, act)
    rc = lib.vit_linear_x6r_fwd(*args, cfg, vo._stream(a.device)) if cfg else lib.vit_linear_x6_fwd(*args, vo._stream(a.device))
    assert rc == 0, (rc, cfg, M, cols, K, act)
    return out, pre, word


class _Probe:
    """a tiny raw launch WITHOUT an announcement: in f16x3 the library refuses it (VIT_EINVAL) unless a product call left operand words pending"""

    def __init__(self, vo):
        self.vo, self.x, self.out = vo, torch.ones(64, 64, device=DEV), torch.empty(64, 64, device=DEV)
        self.wp = vo.split_weight(torch.ones(64, 64, device=DEV))          # (split now: a lazy split announces and consumes words of its own)

    def nothing_pending(self):
        if self.vo._f16():
            rc = self.vo.load().vit_linear_x6_fwd(self.x.data_ptr(), self.wp.data_ptr(), None, None, self.out.data_ptr(), None, 64, 64, 64, 0,
                                                  self.vo._stream(self.x.device))
            assert rc == -1, rc


def _counted(vo, fn):
    before = {k: vo.CALLS.get(k, 0) for k in COUNTERS}
    got = fn()
    return got, {k: vo.CALLS.get(k, 0) - before[k] for k in COUNTERS}


def _same_word(vo, got, want, stored):
    """f16x3: the product's |max| word against the explicit sequence's, as values; both are the exact |max| of what the epilogue stored"""
    if not vo._f16():
        assert got is None and want is None
        return
    assert got is not None and want is not None
    assert int(got.max()) == int(want.max()) == int(stored.abs().max().view(torch.int32))


def _cached(vo, w, layout):
    return vo._SPLIT_CACHE.get(vo._image_key(w, layout), w) is not None


def _inputs(M, N, K, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return r(M, K), r(N, K) / K ** 0.5, r(N), r(M, N), r(M, N), r(M, K)       # x, w, bias, residual, dY, the pre-activation of a GELU in front


# (M, N, K, cfg of the forward / of the input-gradient GEMM in bf16x6, the same in f16x3)
AUTOGRAD_SHAPES = [(64, 64, 64, (0, 0), (0, 0)),
                   (130, 80, 80, (0, 0), (0, 0)),            # cfg 0, ragged in M and N; K = 80: five 16-deep slabs (every x6 entry point refuses K % 16 != 0, so not 72)
                   (1040, 64, 512, (5, 0), (5, 0)),          # narrow output above SMALL_M_ROWS; vit_linear_sm_ok declines its dX (contraction 64 < 128) ...
                   (1040, 256, 256, (5, 5), (5, 5)),         # ... and this is the smallest layer it accepts both ways
                   (2048, 2304, 768, (0, 5), (1, 5)),        # ring cfg 1 (mid-M table; its dX is 768 wide: narrow)
                   (2048, 4096, 1024, (3, 0), (3, 1))]       # ring cfg 3; six products: dX forced to the row image


@pytest.mark.parametrize("fc2_like", [False, True])
@pytest.mark.parametrize("M,N,K,cfg6,cfg3", AUTOGRAD_SHAPES)
def test_autograd_forward_and_input_gradient_equal_the_explicit_sequence(M, N, K, cfg6, cfg3, fc2_like, vo):
    """fc2_like = False: GELU layer with a link (its epilogue stores `pre` and fills link.ax), plain dX whose |max| is published (amax_dx);
    fc2_like = True: residual layer behind a GELU (output |max| published: amax_out; dX runs GELU'(pre) in its epilogue and fills link.adx)"""
    f16 = vo._f16()
    cfg_f, cfg_d = cfg3 if f16 else cfg6
    assert (vo._linear_cfg(M, N, K), vo._linear_cfg(M, N, K, dx=True, mode=vo.LINEAR_MODE)) == (cfg_f, cfg_d)
    x0, w0, b, res, gy, pre_in = _inputs(M, N, K, M + N + K)
    probe = _Probe(vo)
    w = w0.clone().requires_grad_(True)                    # a trainable weight with no image yet: the forward builds both in one pair split
    lk = vo.GeluLink()
    if fc2_like:
        lk.pre = pre_in
    x = x0.clone().requires_grad_(True)

    def product_forward():
        if fc2_like:
            return vo.fused_linear(x, w, b, residual=res, link_in=lk, amax_out=True)
        return vo.fused_linear(x, w, b, gelu=True, link=lk, amax_dx=True)
    y, took_f = _counted(vo, product_forward)
    probe.nothing_pending()
    # the pair split built the image each of the two launches reads, and no other
    assert _cached(vo, w, "block" if cfg_f else "row") and not _cached(vo, w, "row" if cfg_f else "block")
    assert _cached(vo, w, "block_t" if cfg_d else "row_t") and not _cached(vo, w, "row_t" if cfg_d else "block_t")
    (dx,), took_b = _counted(vo, lambda: torch.autograd.grad(y, x, gy))
    probe.nothing_pending()

    wr = w0.clone()                                        # (its own images: the single-image splits)
    def explicit():
        ax = vo._amax_of(x0) if f16 else None
        if fc2_like:
            out, pre, word = _raw(vo, x0, wr, N, cfg_f, bias=b, res=res, operand=ax, want_word=f16)
            ag = vo._amax_of(gy) if f16 else None
            d, _, dword = _raw(vo, gy, wr, K, cfg_d, transposed=True, res=pre_in, act=2, operand=ag, want_word=f16)
        else:
            out, pre, word = _raw(vo, x0, wr, N, cfg_f, bias=b, act=1, want_pre=True, operand=ax, want_word=f16)
            g2 = torch.ops.aten.gelu_backward(gy, pre, approximate="none")
            ag = vo._amax_of(g2) if f16 else None
            d, _, dword = _raw(vo, g2, wr, K, cfg_d, transposed=True, operand=ag, want_word=f16)
        return out, pre, word, d, dword
    (out, pre, word, d, dword), took_e = _counted(vo, explicit)

    assert torch.equal(y.detach(), out) and torch.equal(dx, d)
    if fc2_like:
        assert lk.fused
        _same_word(vo, vo._known_amax(y.detach()) if f16 else None, word, out)
        _same_word(vo, lk.adx, dword, d)
    else:
        assert torch.equal(lk.pre, pre) and not lk.fused
        _same_word(vo, lk.ax, word, out)
        _same_word(vo, vo._known_amax(dx) if f16 else None, dword, d)
    took = {k: took_f[k] + took_b[k] for k in COUNTERS}
    assert took["linear_x6r"] == (cfg_f != 0) + (cfg_d != 0) and took_f["linear_x6r"] == (cfg_f != 0), (took_f, took_b)
    assert took["linear_sm"] == 0 and took["split_pair"] == 1 and took_b["split_pair"] == 0, (took_f, took_b)
    assert (took["amax_pass"], took["amax_published"]) == (took_e["amax_pass"], took_e["amax_published"]), (took, took_e)
    assert took["amax_pass"] == (2 if f16 else 0)


@pytest.mark.parametrize("ring", [False, True])
def test_mlp_pair_with_a_gelu_link_equals_the_explicit_sequence(ring, vo, monkeypatch):
    """fc1 -> GELU -> fc2 (1024 -> 4096 -> 1024 at M = 2048) tied by a GeluLink, as vit.Mlp runs it: GELU' (act = 2) in fc2's dX epilogue once on
    the row-image kernel (RING_DISPATCH off) and once on a ring; the link's two words feed fc2's forward and fc1's dX without a vit_amax pass"""
    monkeypatch.setattr(vo, "RING_DISPATCH", ring)
    f16 = vo._f16()
    M, C, Hd = 2048, 1024, 4096
    # cfg of: fc1 forward, fc2 forward, fc2 dX, fc1 dX
    cfgs = ((3, 1, 3, 1) if f16 else (3, 0, 0, 0)) if ring else (0, 0, 0, 0)
    mode = vo.LINEAR_MODE
    assert cfgs == (vo._linear_cfg(M, Hd, C), vo._linear_cfg(M, C, Hd), vo._linear_cfg(M, C, Hd, dx=True, mode=mode), vo._linear_cfg(M, Hd, C, dx=True, mode=mode))
    g = torch.Generator(DEV).manual_seed(17)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x0, w1, b1, w2, b2, gy = r(M, C), r(Hd, C) / C ** 0.5, r(Hd), r(C, Hd) / Hd ** 0.5, r(C), r(M, C)
    probe = _Probe(vo)
    p1, p2 = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    x = x0.clone().requires_grad_(True)
    lk = vo.GeluLink()

    def product():
        y = vo.fused_linear(vo.fused_linear(x, p1, b1, gelu=True, link=lk), p2, b2, residual=x, link_in=lk)
        probe.nothing_pending()
        (dx,) = torch.autograd.grad(y, x, gy)
        probe.nothing_pending()
        return y.detach(), dx
    (y, dx), took = _counted(vo, product)

    def explicit():
        h, pre, ax = _raw(vo, x0, w1, Hd, cfgs[0], bias=b1, act=1, want_pre=True, operand=vo._amax_of(x0) if f16 else None, want_word=f16)
        out, _, _ = _raw(vo, h, w2, C, cfgs[1], bias=b2, res=x0, operand=ax)
        dh, _, adx = _raw(vo, gy, w2, Hd, cfgs[2], transposed=True, res=pre, act=2, operand=vo._amax_of(gy) if f16 else None, want_word=f16)
        d, _, _ = _raw(vo, dh, w1, C, cfgs[3], transposed=True, operand=adx)
        return h, pre, ax, out, dh, adx, d
    (h, pre, ax, out, dh, adx, d), took_e = _counted(vo, explicit)

    assert torch.equal(y, out) and torch.equal(lk.pre, pre) and lk.fused
    assert torch.equal(dx, d + gy)                          # (the residual branch hands dY through to x; one fp32 add in the engine)
    _same_word(vo, lk.ax, ax, h)
    _same_word(vo, lk.adx, adx, dh)
    assert took["linear_x6r"] == sum(c != 0 for c in cfgs) and took["linear_sm"] == 0 and took["split_pair"] == 2, took
    assert (took["amax_pass"], took["amax_published"]) == (took_e["amax_pass"], took_e["amax_published"]) == ((2, 0) if f16 else (0, 0)), (took, took_e)


@pytest.mark.parametrize("M,N,K,cfg", [(64, 64, 64, 0), (130, 80, 80, 0), (257, 768, 768, 5)])
def test_serving_path_equals_the_explicit_sequence(M, N, K, cfg, vo):
    """fused_linear under no_grad: the small-M kernel where it serves the shape, else the row-image kernel; GELU, residual and the |max| word
    each site publishes (small-M: every output; 128-row kernel: un-activated outputs on request)"""
    f16 = vo._f16()
    assert vo._linear_cfg(M, N, K, serving=True) == cfg
    x, w, b, res, _, _ = _inputs(M, N, K, 3 * M + N + K)
    probe = _Probe(vo)
    with torch.no_grad():
        for gelu, use_res, amax_out in ((True, False, False), (False, True, True), (False, False, False)):
            r = res if use_res else None
            got, took = _counted(vo, lambda: vo.fused_linear(x, w, b, r, gelu=gelu, amax_out=amax_out))
            probe.nothing_pending()
            wants = f16 and ((amax_out and not gelu) or cfg != 0)
            (out, _, word), took_e = _counted(vo, lambda: _raw(vo, x, w, N, cfg, bias=b, res=r, act=1 if gelu else 0,
                                                                operand=vo._amax_of(x) if f16 else None, want_word=wants))
            assert torch.equal(got, out), (gelu, use_res)
            if wants:
                _same_word(vo, vo._known_amax(got), word, out)
            else:
                assert vo._known_amax(got) is None
            assert took["linear_sm"] == (cfg != 0) and took["linear_x6r"] == 0 and took["split_pair"] == 0, took
            assert (took["amax_pass"], took["amax_published"]) == (took_e["amax_pass"], took_e["amax_published"]) == ((1, 0) if f16 else (0, 0)), (took, took_e)

"""-m gpu: the tile scan (K2) on many workgroups (round 15: three launches of one workgroup per 256 counters instead of one workgroup).

gsr_forward is driven through the C ABI with a workspace of its own (non-persistent counters, so tile_count still holds what K1 counted)
and the scan's products are checked against a numpy scan of those counts:
  * tile_offset is the exact exclusive scan, saturated at 2^32 - 1, with R in [n];
  * the status words: R (low / high), overflow, longest list, unit count (0 after an overflow);
  * tile_order is a permutation of [0, V*T) in non-increasing length class;
  * unit_order holds every (tile, segment) exactly once: the full units first, then the last units in non-increasing class.
The order inside a class is arbitrary and is not checked."""
import ctypes as C

import numpy as np
import pytest
import torch

from styl3r_amd import _lib

pytestmark = pytest.mark.gpu


def _seg_len(flags, vt):
    """include/gsr.h GSR_FLAG_SEG_SHIFT"""
    sel = (flags >> _lib.GSR_FLAG_SEG_SHIFT) & 7
    return {1: 64, 2: 128, 3: 192, 4: 256, 5: 384, 7: 1 << 30}.get(sel, 256 if vt >= 4096 else (128 if vt >= 1024 else 64))


def _forward(n_views, image_hw, grid_hw, cap, flags=0, seed=21, cov_scale=1.0):
    from styl3r_amd.decoder import build_views_hip
    from styl3r_amd.scenes import make_scene
    lib = _lib.load()
    dev = torch.device("cuda:0")
    H, W = image_hw
    sc = make_scene(n_ctx=1, grid_hw=grid_hw, n_views=n_views, image_hw=image_hw, seed=seed)
    means, cov, har, op = (t.to(dev)[None].contiguous() for t in (sc.means, sc.covariances * cov_scale, sc.harmonics, sc.opacities))
    views = build_views_hip(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev), torch.zeros(3, device=dev), False)
    shs = har.permute(0, 1, 3, 2).contiguous()
    V, G = n_views, means.shape[1]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    n = V * T
    flags |= _lib.GSR_FLAG_COV9
    dims = _lib.GsrDims(1, V, G, H, W, shs.shape[2], 0, flags, None)
    L = _lib.workspace_layout(dims, cap)
    ws = torch.zeros(L.total, dtype=torch.uint8, device=dev)
    img = torch.empty((V, 3, H, W), device=dev); dep = torch.empty((V, H, W), device=dev); opa = torch.empty((V, H, W), device=dev)
    radii = torch.empty((V, G), dtype=torch.int32, device=dev); status = torch.zeros(8, dtype=torch.int32, device=dev)
    rc = lib.gsr_forward(C.byref(dims), views.data_ptr(), means.data_ptr(), cov.data_ptr(), op.data_ptr(), shs.data_ptr(),
                         cap, ws.data_ptr(), L.total, img.data_ptr(), dep.data_ptr(), opa.data_ptr(), radii.data_ptr(),
                         None, status.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    seg = _seg_len(flags, n)
    umax = n + cap // seg
    view = lambda off, count, dt: ws[off:off + count * np.dtype(dt).itemsize].cpu().numpy().view(dt)
    st = status.cpu().numpy()
    assert np.array_equal(st, view(L.status, 8, np.int32)), "caller's status words != the workspace copy"
    return dict(n=n, cap=cap, seg=seg, status=st, count=view(L.tile_count, n, np.uint32), offset=view(L.tile_offset, n + 1, np.uint32),
                cursor=view(L.tile_cursor, n, np.uint32), order=view(L.tile_order, n, np.uint32),
                units=view(L.unit_order, umax * 2, np.uint32).reshape(umax, 2))


def _class(length, longest):
    sh = 0
    while (int(longest) >> sh) > 255:
        sh += 1
    return np.minimum(length >> sh, 255)


def _check(r):
    n, seg, count = r["n"], r["seg"], r["count"].astype(np.int64)
    R = int(count.sum())
    m = int(count.max())
    exact = np.concatenate([[0], np.cumsum(count)])
    assert np.array_equal(r["offset"].astype(np.int64), np.minimum(exact, 0xFFFFFFFF)), "tile_offset != exclusive scan of tile_count"
    overflow = int(R > r["cap"] or R > 0xFFFFFFFF)
    st = r["status"].astype(np.int64) & 0xFFFFFFFF
    assert (int(st[0]), int(st[3])) == (R & 0xFFFFFFFF, R >> 32), "pair count"
    assert int(st[1]) == overflow and int(st[2]) == m, "overflow flag / longest list"
    order = r["order"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "tile_order is not a permutation of [0, V*T)"
    cls = _class(count, m)[order]
    assert (np.diff(cls) <= 0).all(), "tile_order: length classes must not increase"
    if overflow:
        assert int(st[4]) == 0, "no unit table after an overflow"
        return
    assert np.array_equal(r["cursor"].astype(np.int64), count), "cursors: zeroed by the scan, then advanced once per pair"
    nfull = np.where(count > 0, (count - 1) // seg, 0)
    F, U = int(nfull.sum()), int(nfull.sum() + (count > 0).sum())
    assert int(st[4]) == U, "unit count"
    units = r["units"][:U].astype(np.int64)
    want = sorted((t, s) for t in np.nonzero(count)[0] for s in range(int(nfull[t]) + 1))
    assert sorted(map(tuple, units)) == want, "unit_order must hold every (tile, segment) exactly once"
    assert (units[:F, 1] < nfull[units[:F, 0]]).all(), "the full units come first"
    last = units[F:]
    assert (last[:, 1] == nfull[last[:, 0]]).all()
    ucls = _class(count[last[:, 0]] - nfull[last[:, 0]] * seg, min(m, seg))
    assert (np.diff(ucls) <= 0).all(), "last units: length classes must not increase"


@pytest.mark.parametrize("n_views,image_hw,grid_hw,n,cov_scale", [
    (1, (16, 16), (12, 12), 1, 1.0),            # one counter
    (3, (16, 16), (12, 12), 3, 1.0),
    (5, (80, 656), (24, 96), 1025, 1.0),        # 5 views of 41 x 5 tiles: crosses a chunk of 1 024 counters (and four of 256)
    (4, (1040, 1040), (16, 16), 16900, 1e-4),   # 4 views of 65 x 65 tiles, 256 pixel-sized Gaussians: > 16 384 counters, most tiles empty, ballot binning
    (3, (64, 96), (3, 4), 72, 1e-4),            # 12 pixel-sized Gaussians: empty tiles in the middle of the range
], ids=["n1", "n3", "n1025", "n16900", "gaps"])
def test_scan_products_match_a_numpy_scan(n_views, image_hw, grid_hw, n, cov_scale):
    r = _forward(n_views, image_hw, grid_hw, cap=1 << 20, cov_scale=cov_scale)
    assert r["n"] == n
    assert r["status"][1] == 0 and r["count"].any()
    if cov_scale < 1.0:
        z = np.nonzero(r["count"])[0]
        assert len(z) > 1 and (r["count"][z[0]:z[-1]] == 0).any(), "the scene must leave empty tiles between non-empty ones"
    _check(r)


def test_forced_segment_length_and_a_list_of_more_than_three_segments():
    r = _forward(2, (16, 16), (40, 40), cap=1 << 16, flags=1 << _lib.GSR_FLAG_SEG_SHIFT)
    assert r["seg"] == 64 and r["count"].max() > 3 * 64
    _check(r)


def test_capacity_below_the_pair_count_reports_overflow_and_the_retry_succeeds():
    r = _forward(2, (48, 64), (32, 32), cap=256)
    R = int(r["count"].sum())
    assert R > 256 and r["status"][1] == 1 and r["status"][4] == 0
    _check(r)
    r = _forward(2, (48, 64), (32, 32), cap=R + 1024)
    assert r["status"][1] == 0 and int(r["status"][0]) == R and r["status"][4] > 0
    _check(r)

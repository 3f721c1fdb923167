"""Helpers for the -m gpu parity tests: run the HIP path through the C ABI and
the CPU oracle on identical bytes."""
import os

import numpy as np
import torch

from oracle.gsr_oracle import Oracle
from styl3r_amd import rasterizer as rz


def ws_view(name, dtype, count):
    """typed view into the workspace of the last forward (rasterizer.KEEP_DEBUG must be on)."""
    dbg = rz.LAST_DEBUG
    off = getattr(dbg["layout"], name)
    nbytes = count * np.dtype(dtype).itemsize
    raw = dbg["ws"][off:off + nbytes].cpu().numpy()
    return raw.view(dtype)


def hip_single_view(means, cov6, opac, cam, shs=None, colors=None, bg=(0, 0, 0), sh_degree=0, theta=None, rho=None,
                    requires_grad=False):
    """One view through the drop-in GaussianRasterizer; inputs are numpy, returns dict of tensors."""
    dev = torch.device("cuda:0")
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    t = dict(means=f(means), cov6=f(cov6), opac=f(opac).reshape(-1, 1))
    t["colors"] = f(shs if shs is not None else colors)
    means2D = torch.zeros_like(t["means"])
    if requires_grad:
        for k in t:
            t[k].requires_grad_(True)
        means2D.requires_grad_(True)
    settings = rz.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=f(bg),
        scale_modifier=1.0, viewmatrix=f(cam["view"]), projmatrix=f(cam["proj"]), projmatrix_raw=f(cam["proj_raw"]),
        sh_degree=sh_degree, campos=f(cam["campos"]), prefiltered=False, debug=False)
    rast = rz.GaussianRasterizer(settings)
    image, radii, depth, opacity, n_touched = rast(
        means3D=t["means"], means2D=means2D, shs=t["colors"] if shs is not None else None,
        colors_precomp=None if shs is not None else t["colors"], opacities=t["opac"], cov3D_precomp=t["cov6"],
        theta=theta, rho=rho)
    return dict(image=image, radii=radii, depth=depth, opacity=opacity, n_touched=n_touched, inputs=t, means2D=means2D)


def oracle_single_view(precision, means, cov6, opac, cam, shs=None, colors=None, bg=(0, 0, 0), sh_degree=0, nthreads=8):
    orc = Oracle(precision)
    # feed the oracle the exact fp32 values the GPU sees
    r = lambda a: None if a is None else np.asarray(a, dtype=np.float32)
    st, ctx = orc.forward(r(means), r(cov6), r(opac), shs=r(shs), colors=r(colors), H=cam["H"], W=cam["W"],
                          tanfovx=np.float32(cam["tanfovx"]), tanfovy=np.float32(cam["tanfovy"]), bg=bg,
                          view=r(cam["view"]), proj=r(cam["proj"]), proj_raw=r(cam["proj_raw"]), campos=r(cam["campos"]),
                          sh_degree=sh_degree, nthreads=nthreads)
    return orc, st, ctx


def assert_close_rel(actual, expected, rel=1e-4, what="", atol=0.0):
    """max |a-e| <= rel * max|e| (+ tiny absolute floor): the 1e-4-rel bar of BASELINE.json's north_star."""
    a = np.asarray(actual, dtype=np.float64); e = np.asarray(expected, dtype=np.float64)
    scale = max(np.abs(e).max(), 1e-12)
    err = np.abs(a - e).max()
    if os.environ.get("PARITY_VERBOSE"):      # bar calibration runs: `PARITY_VERBOSE=1 pytest -s` lists every observed distance beside its bar
        print(f"    [parity] {what}: rel {err / scale:.3e} (bar {rel:.1e})")
    assert err <= rel * scale + atol, f"{what}: max abs err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})"


def worst_row_rel(actual, expected, floor=1e-300):
    """per-ROW error of a (B, N, H, D) attention tensor: a row is one (b, h, n) -- (b, h, query) for out / dq, (b, h, key) for dk / dv.
    Error of a row = max |a - e| over the row / max |e| over the row, so a row far below the tensor's maximum is judged at its own scale;
    rows whose reference max is below `floor` (a number, or one value per row: shape (B, N, H)) -- exactly zero ones in particular -- are
    divided by `floor` instead.  A NaN / Inf counts as an
    infinite error.  Returns (worst error, (b, h, n) of that row)."""
    a = np.asarray(actual, dtype=np.float64); e = np.asarray(expected, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(a - e).max(-1)
    err = np.where(np.isfinite(err), err, np.inf)
    den = np.maximum(np.abs(e).max(-1), floor)
    rel = err / den
    i = np.unravel_index(int(np.argmax(rel)), rel.shape)
    return float(rel[i]), (int(i[0]), int(i[2]), int(i[1]))


CANCEL_FLOOR = 2.0 ** -8        # the two floors of tests/test_gpu_attention_ranges.py, for the 2-D row metric below
RANGE_FLOOR = 2.0 ** -24


def row_scales(expected, terms=None, tensor_max=None):
    """what each row of a 2-D tensor is judged against: its own max |e|, but at least CANCEL_FLOOR x the row max of `terms` (the product
    |a| . |b|^T of the contraction that made it: a row that is a near-complete cancellation) and at least RANGE_FLOOR x the tensor's maximum
    (`tensor_max`, default max |expected|: a row far below anything the output's fp32 consumer can see).  Returns (scale per row, rows that
    sit on a floor)."""
    e = np.abs(np.asarray(expected, dtype=np.float64))
    own = e.max(-1)
    floor = np.full(own.shape, RANGE_FLOOR * (float(e.max()) if tensor_max is None else float(tensor_max)))
    if terms is not None:
        floor = np.maximum(floor, CANCEL_FLOOR * np.abs(np.asarray(terms, dtype=np.float64)).max(-1))
    floor = np.maximum(floor, 1e-300)
    return np.maximum(own, floor), own < floor


def worst_row_rel_2d(actual, expected, terms=None, tensor_max=None, rows=None):
    """per-ROW error of a 2-D (rows, columns) tensor: error of a row = max |a - e| over the row / max |e| over the row, with the two floors of
    `row_scales`.  rows: judge only these (an index array or slice; the floors still come from the whole tensor).  A NaN / Inf counts as an
    infinite error.  Returns (worst error, index of that row in the whole tensor)."""
    a = np.asarray(actual, dtype=np.float64); e = np.asarray(expected, dtype=np.float64)
    assert a.shape == e.shape and e.ndim == 2, (a.shape, e.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(a - e).max(-1)
    err = np.where(np.isfinite(err), err, np.inf)
    rel = err / row_scales(e, terms, tensor_max)[0]
    idx = np.arange(e.shape[0])[rows] if rows is not None else np.arange(e.shape[0])
    i = int(idx[int(np.argmax(rel[idx]))])
    return float(rel[i]), i

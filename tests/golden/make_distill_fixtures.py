"""Generates tests/golden/distill_ref.npz from the REFERENCE:
  * `Regr3D` (src/loss/loss_point.py:188-254) values and input gradients in float64 for B = 2, N = 32 x 48, in the modes None, 'avg_dis',
    dist_clip = 4.0 and disable_view1 (inputs stored as float32);
  * a tiny `Dust3R` (src/model/distiller/dust3d_backbone.py) under tests.helpers.deterministic_init_, the confidence bias of both heads
    shifted so that the confidence straddles 3 (at plain init it is ~2 and nothing would be valid): its state-dict keys, parameter count
    and pts3d / conf on a seeded 2 x 2 x 3 x 32 x 48 batch.  No weights are stored.
    python tests/golden/make_distill_fixtures.py
"""
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests.golden.ref_stubs import REF, install
from tests.helpers import deterministic_init_

TINY = dict(enc_depth=1, dec_depth=12, enc_embed_dim=128, dec_embed_dim=128, enc_num_heads=2, dec_num_heads=2, pos_embed="RoPE100",
            img_size=(512, 512))
CONF_BIAS_SHIFT = 0.7          # conf = 1 + exp(x): x ~ 0 at init gives ~2; + 0.7 gives ~3
inf = float("inf")


def regr3d_inputs(B=2, H=32, W=48, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt1 = torch.randn(B, H, W, 3, generator=g) * 2
    gt2 = torch.randn(B, H, W, 3, generator=g) * 2 + 0.5
    pr1 = gt1 + 0.1 * torch.randn(B, H, W, 3, generator=g)
    pr2 = gt2 + 0.1 * torch.randn(B, H, W, 3, generator=g)
    c1 = 1 + torch.exp(torch.randn(B, H, W, generator=g) + 1)
    c2 = 1 + torch.exp(torch.randn(B, H, W, generator=g) + 1)
    return gt1, gt2, pr1, pr2, c1, c2


MODES = {"none": dict(norm_mode=None), "avg_dis": dict(norm_mode="avg_dis"), "clip": dict(norm_mode="avg_dis", dist_clip=4.0),
         "no_view1": dict(norm_mode=None, disable_view1=True)}


def main():
    install()
    m = types.ModuleType("src.model.distiller"); m.__path__ = [REF + "/src/model/distiller"]; sys.modules["src.model.distiller"] = m
    lp = importlib.import_module("src.loss.loss_point")
    d3 = importlib.import_module("src.model.distiller.dust3d_backbone")
    out = {}
    ins = regr3d_inputs()
    for k, t in zip(("gt1", "gt2", "pr1", "pr2", "conf1", "conf2"), ins):
        out["regr_" + k] = t.numpy()
    torch.set_default_dtype(torch.float64)          # the reference builds its quantile tensor in the default dtype
    for name, kw in MODES.items():
        gt1, gt2, pr1, pr2, c1, c2 = (t.double() for t in ins)
        pr1.requires_grad_(True); pr2.requires_grad_(True)
        kw = dict(kw)
        loss = lp.Regr3D(norm_mode=kw.pop("norm_mode"))(gt1, gt2, pr1, pr2, c1, c2, **kw)
        loss.backward()
        out[f"regr_{name}_loss"] = loss.detach().numpy()
        out[f"regr_{name}_g1"] = (pr1.grad if pr1.grad is not None else torch.zeros_like(pr1)).numpy()      # (no_view1: view 1 is unused)
        out[f"regr_{name}_g2"] = pr2.grad.numpy()
    torch.set_default_dtype(torch.float32)
    teacher = d3.Dust3R(patch_embed_cls="PatchEmbedDust3R", head_type="dpt", output_mode="pts3d", depth_mode=("exp", -inf, inf),
                        conf_mode=("exp", 1, inf), **TINY).eval()
    deterministic_init_(teacher)
    with torch.no_grad():
        for head in (teacher.downstream_head1, teacher.downstream_head2):
            head.dpt.head[4].bias[3] += CONF_BIAS_SHIFT
    g = torch.Generator().manual_seed(7)
    image = torch.rand(2, 2, 3, 32, 48, generator=g) * 2 - 1
    r1, r2 = teacher({"image": image}, False)
    out.update(t_image=image.numpy(), t_pts1=r1["pts3d"].numpy(), t_conf1=r1["conf"].numpy(), t_pts2=r2["pts3d"].numpy(),
               t_conf2=r2["conf"].numpy(), t_keys=np.array(sorted(teacher.state_dict().keys())),
               t_nparams=np.array(sum(p.numel() for p in teacher.parameters())), t_conf_bias_shift=np.array(CONF_BIAS_SHIFT))
    path = ROOT / "tests/golden/distill_ref.npz"
    np.savez_compressed(path, **out)
    print("Regr3D", {k: float(out[f"regr_{k}_loss"]) for k in MODES}, "| teacher keys", len(out["t_keys"]), "params", int(out["t_nparams"]),
          "conf range", float(r1["conf"].min()), float(r1["conf"].max()), "share >= 3", float((r1["conf"] >= 3).float().mean()),
          "| bytes", path.stat().st_size)


if __name__ == "__main__":
    main()

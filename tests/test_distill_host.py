"""Point-map distillation, host side: `regr3d_expression` and the `Dust3R` teacher against the reference's own outputs
(tests/golden/make_distill_fixtures.py -> distill_ref.npz), the distillation branch of `select_trainable`, and one CPU
`TrainStep(distill_only=True)`."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.helpers import deterministic_init_

F = np.load(Path(__file__).resolve().parent / "golden" / "distill_ref.npz")
TEACHER_TINY = dict(enc_depth=1, dec_depth=12, enc_embed_dim=128, dec_embed_dim=128, enc_num_heads=2, dec_num_heads=2, pos_embed="RoPE100",
                    img_size=(512, 512))
STUDENT_TINY = dict(enc_depth=1, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=128, enc_num_heads=16, dec_num_heads=2, pos_embed="RoPE100",
                    img_size=(512, 512))            # (the intrinsics token of the student is 1024 wide)
MODES = {"none": dict(norm_mode=None), "avg_dis": dict(norm_mode="avg_dis"), "clip": dict(norm_mode="avg_dis", dist_clip=4.0),
         "no_view1": dict(norm_mode=None, disable_view1=True)}


def tiny_teacher():
    from styl3r_amd.distiller import Dust3R
    m = deterministic_init_(Dust3R(**TEACHER_TINY))
    with torch.no_grad():
        for head in (m.downstream_head1, m.downstream_head2):
            head.dpt.head[4].bias[3] += float(F["t_conf_bias_shift"])
    return m


def tiny_student(device="cpu"):
    from styl3r_amd.encoder import EncoderNoPoSplatTokenStyle, EncoderNoPoSplatTokenStyleCfg
    cfg = EncoderNoPoSplatTokenStyleCfg(name="noposplat_token_style", stylized=False)
    return deterministic_init_(EncoderNoPoSplatTokenStyle(cfg, trunk_params=STUDENT_TINY).eval()).to(device)


def distill_batch(device="cpu", b=2):
    image = torch.tensor(F["t_image"], device=device)[:b]
    K = torch.tensor([[0.86, 0, 0.5], [0, 0.86, 0.5], [0, 0, 1.0]], device=device).expand(b, 2, 3, 3).contiguous()
    return dict(context=dict(image=image, intrinsics=K))


def regr_inputs(dtype, device="cpu"):
    return [torch.tensor(F["regr_" + k], dtype=dtype, device=device) for k in ("gt1", "gt2", "pr1", "pr2", "conf1", "conf2")]


@pytest.mark.parametrize("mode", list(MODES))
def test_expression_in_float64_reproduces_the_reference(mode):
    """the same formula in the same precision: value and both input gradients to 1e-12 relative"""
    from styl3r_amd.losses import regr3d_expression
    gt1, gt2, pr1, pr2, c1, c2 = regr_inputs(torch.float64)
    pr1.requires_grad_(True); pr2.requires_grad_(True)
    loss = regr3d_expression(gt1, gt2, pr1, pr2, c1, c2, **MODES[mode])
    loss.backward()
    want = float(F[f"regr_{mode}_loss"])
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)
    for got, key in ((pr1.grad, "g1"), (pr2.grad, "g2")):
        ref = F[f"regr_{mode}_{key}"]
        got = np.zeros_like(ref) if got is None else got.numpy()
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), (mode, key)


def test_regr3d_module_takes_the_expression_on_the_cpu_and_an_empty_view_counts_zero():
    from styl3r_amd.losses import Regr3D, regr3d_expression
    gt1, gt2, pr1, pr2, c1, c2 = regr_inputs(torch.float32)
    a = Regr3D(norm_mode=None)(gt1, gt2, pr1, pr2, c1, c2)
    assert torch.equal(a, regr3d_expression(gt1, gt2, pr1, pr2, c1, c2, norm_mode=None))
    assert abs(float(a) - float(F["regr_none_loss"])) <= 1e-5 * float(F["regr_none_loss"])
    assert Regr3D().norm_mode == "avg_dis" and Regr3D().alpha == 0.2 and Regr3D().gt_scale is False
    # the deliberate deviation: no confident point in view 1 -> its term is 0 (the reference: NaN)
    pr1 = pr1.clone().requires_grad_(True)
    lone = Regr3D()(gt1, gt2, pr1, pr2, torch.ones_like(c1), c2)
    assert torch.isfinite(lone) and float(lone.detach()) > 0
    lone.backward()
    assert torch.isfinite(pr1.grad).all()
    for other in ("avg_log1p", "median_dis"):              # the modes no wrapper uses stay available through the expression
        assert torch.isfinite(Regr3D(norm_mode=other)(gt1, gt2, pr1, pr2, c1, c2))


def test_teacher_keys_and_parameter_count_match_the_reference():
    m = tiny_teacher()
    assert sorted(m.state_dict().keys()) == list(F["t_keys"])
    assert sum(p.numel() for p in m.parameters()) == int(F["t_nparams"])
    assert not m.training and not m.train().training          # always in eval mode


def test_teacher_load_state_dict_fills_the_second_decoder():
    from styl3r_amd.distiller import Dust3R
    src = tiny_teacher()
    sd = {k: v for k, v in src.state_dict().items() if not k.startswith("dec_blocks2")}
    assert len(sd) < len(src.state_dict())
    dst = Dust3R(**TEACHER_TINY)
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in dst.state_dict().items():
        if k.startswith("dec_blocks2"):
            assert torch.equal(v, sd[k.replace("dec_blocks2", "dec_blocks")]), k


def test_teacher_cpu_forward_matches_the_reference():
    from oracle.encoder_cpu import cpu_attention          # (the attention kernels have no CPU path: plain-torch restatement, tests only)
    from tests.gpu_utils import assert_close_rel
    m = tiny_teacher()
    with cpu_attention():
        r1, r2 = m({"image": torch.tensor(F["t_image"])}, False)
    assert r1["pts3d"].shape == (2, 32, 48, 3) and r1["conf"].shape == (2, 32, 48) and not r1["pts3d"].requires_grad
    for r, k in ((r1, "1"), (r2, "2")):
        assert_close_rel(r["pts3d"].numpy(), F["t_pts" + k], 1e-4, "pts3d " + k)
        assert_close_rel(r["conf"].numpy(), F["t_conf" + k], 1e-4, "conf " + k)
    assert float(r1["conf"].min()) < 3 < float(r1["conf"].max())
    with pytest.raises(NotImplementedError):
        m({"image": torch.tensor(F["t_image"])}, True)
    with pytest.raises(NotImplementedError):
        m.estimate_pose({"image": torch.tensor(F["t_image"])})


def test_head_factory_confidence_channel_is_the_dpt_point_head_only():
    from styl3r_amd.encoder import StructureBuilder, head_factory
    net = StructureBuilder(TEACHER_TINY)
    assert head_factory("dpt", "pts3d", net, has_conf=True).dpt.head[4].out_channels == 4
    assert head_factory("dpt", "pts3d", net).dpt.head[4].out_channels == 3
    with pytest.raises(AssertionError):
        head_factory("linear", "pts3d", net, has_conf=True)


def test_get_distiller_names():
    from styl3r_amd.distiller import get_distiller
    with pytest.raises(AssertionError):
        get_distiller("croco")


def test_distillation_stage_selection_partitions_by_the_three_name_rules():
    from styl3r_amd.encoder import EncoderNoPoSplatTokenStyle, EncoderNoPoSplatTokenStyleCfg
    from styl3r_amd.train import select_trainable
    with torch.device("meta"):
        m = EncoderNoPoSplatTokenStyle(EncoderNoPoSplatTokenStyleCfg(name="noposplat_token_style", stylized=False))
    new, pre, frozen = select_trainable(m, distill_only=True)
    names = {id(p): n for n, p in m.named_parameters()}
    assert new and pre and not frozen
    assert all("structure_builder" in names[id(p)] or "downstream_head" in names[id(p)] for p in new)
    assert all("backbone" in names[id(p)] for p in pre)
    chosen = {id(p) for p in new + pre}
    left = [n for n, p in m.named_parameters() if id(p) not in chosen]
    assert left and all(n.startswith(("token_stylizer.", "gaussian_structure_head.", "gaussian_appearance_head.")) for n in left)
    assert len(chosen) == len(new) + len(pre) and len(chosen) + len(left) == sum(1 for _ in m.parameters())
    # the default is the NVS-stage selection, untouched
    with torch.device("meta"):
        m2 = EncoderNoPoSplatTokenStyle(EncoderNoPoSplatTokenStyleCfg(name="noposplat_token_style", stylized=False))
    n2, p2, f2 = select_trainable(m2)
    assert len(n2) + len(p2) == sum(1 for _ in m2.parameters()) and not f2


def test_cpu_train_step_distill_only_updates_only_the_distilled_parts():
    from oracle.encoder_cpu import cpu_attention
    with cpu_attention():
        _cpu_train_step_distill_only()


def _cpu_train_step_distill_only():
    from styl3r_amd.losses import regr3d_expression
    from styl3r_amd.train import TrainStep
    enc, teacher = tiny_student(), tiny_teacher()
    batch = distill_batch()
    style = {"image": batch["context"]["image"][:, 0]}
    with torch.no_grad():
        dump = {}
        assert enc(batch["context"], style, 0, visualization_dump=dump, distill_only=True) is None
        assert set(dump) == {"means"} and dump["means"].shape == (2, 2, 32, 48, 1, 3)
        gt1, gt2 = teacher(batch["context"], False)
        want = regr3d_expression(gt1["pts3d"], gt2["pts3d"], dump["means"][:, 0].squeeze(-2), dump["means"][:, 1].squeeze(-2),
                                 gt1["conf"], gt2["conf"], norm_mode=None)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    step = TrainStep(enc, None, distiller=teacher, distill_only=True, lr=1e-3)
    assert step.distiller_loss.norm_mode is None            # an encoder that takes a style: Regr3D(norm_mode=None)
    loss = step(batch)
    assert torch.isfinite(loss) and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    moved = {n for n, p in enc.named_parameters() if not torch.equal(p.detach(), before[n])}
    assert moved and all(n.startswith(("structure_builder.", "downstream_head1.", "backbone.")) for n in moved), sorted(moved)[:5]
    assert any(n.startswith("structure_builder.") for n in moved) and any(n.startswith("downstream_head1.") for n in moved)
    assert any(n.startswith("backbone.enc_blocks.") for n in moved)
    assert all(p.grad is None for p in teacher.parameters()) and step.global_step == 1
    with pytest.raises(ValueError):
        from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg
        with torch.device("meta"):
            other = EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg(stylized=False))
        TrainStep(other, None, distiller=teacher, distill_only=True)

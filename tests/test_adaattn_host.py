"""CPU tests (-m "not gpu") of the AdaAttN loss: losses.LossAdaAttN / adaattn_expression in float64 against the golden vectors of the
reference's own VGGContentLoss + VGGStyleLoss on its NormalizedVGG (tests/golden/make_adaattn_fixtures.py), the registry, the VGG's
state-dict layout, the C ABI's argument checks and the routes CPU tensors take."""
import ctypes as C
import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from styl3r_amd import losses, vit_ops
from tests import adaattn_inputs as ai

ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests/golden/adaattn_ref.npz")


@functools.lru_cache(maxsize=None)
def vgg(depth=5, dtype=torch.float64):
    net = losses.NormalizedVGG(depth=depth)
    net.load_normalised_vgg(ai.vgg_state_dict())
    return net.to(dtype)


def batch_of(dtype):
    target, pred, style = (t.to(dtype) for t in ai.images(**ai.FIXTURE_SHAPE))
    return SimpleNamespace(color=pred.requires_grad_(True)), {"target": {"image": target}, "style": {"image": style}}


@pytest.mark.parametrize("tag", list(ai.CONFIGS))
def test_float64_loss_reproduces_the_reference(tag):
    cfg = losses.LossAdaAttNCfg(**ai.CONFIGS[tag])
    prediction, batch = batch_of(torch.float64)
    n0 = dict(losses.CALLS)
    details = {}
    loss = losses.LossAdaAttN(cfg, vgg(max(*cfg.content_loss_layers, *cfg.style_loss_layers)))(prediction, batch, None, 0, details=details)
    loss.backward()
    assert losses.CALLS["adaattn_hip_stats"] == n0["adaattn_hip_stats"] and losses.CALLS["adaattn_hip_l1"] == n0["adaattn_hip_l1"]
    loss = loss.detach()
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    grad, ref = prediction.color.grad.numpy(), GOLD[f"{tag}_grad"]
    gerr = np.abs(grad - ref).max() / np.abs(ref).max()
    print(f"{tag}: value {rel(loss, GOLD[tag + '_value']):.2e} content {rel(details['content'], GOLD[tag + '_content']):.2e} "
          f"style {rel(details['style'], GOLD[tag + '_style']):.2e} gradient {gerr:.2e}")
    assert rel(loss, GOLD[f"{tag}_value"]) <= 1e-12
    assert rel(details["content"], GOLD[f"{tag}_content"]) <= 1e-12
    assert rel(details["style"], GOLD[f"{tag}_style"]) <= 1e-12
    assert gerr <= 1e-10
    for l in cfg.content_loss_layers:
        p_shape = (4, (64, 128, 256)[l - 1], (32 >> (l - 1)) ** 2)
        assert details[f"cs{l}"].shape == p_shape and details[f"feature_grad{l}"].shape == p_shape


def test_fp32_expression_is_the_reference_op_sequence():
    """the fp32 run of the same chain lands where the reference's own fp32 run does (conv summation order aside)"""
    cfg = losses.LossAdaAttNCfg(**ai.CONFIGS["yaml"])
    prediction, batch = batch_of(torch.float32)
    with torch.no_grad():
        loss = losses.LossAdaAttN(cfg, vgg(3, torch.float32))(prediction, batch)
    assert abs(float(loss) - float(GOLD["yaml_value32"])) <= 1e-5 * float(GOLD["yaml_value32"])


def test_get_losses_round_trip():
    cfgs = [losses.LossMseCfg(), losses.LossAdaAttNCfg()]
    built = losses.get_losses(cfgs)
    assert [type(m) for m in built] == [losses.LossMse, losses.LossAdaAttN] and built[1].cfg is cfgs[1]
    assert built[1].vgg.depth == 3 and not any(p.requires_grad for p in built[1].parameters())
    assert (built[1].cfg.lam, tuple(built[1].cfg.content_loss_layers), tuple(built[1].cfg.style_loss_layers), tuple(built[1].cfg.style_loss_stats)) \
        == (0.3, (3,), (2, 3), ("mean", "std"))
    with pytest.raises(NotImplementedError, match="adaattn") as e:
        losses.get_losses([losses.LossMseCfg(), {"adaattn": {"weight": 1.0}}])
    assert repr({"adaattn": {"weight": 1.0}}) in str(e.value)
    with pytest.raises(NotImplementedError, match="'nope'"):
        losses.get_losses(["nope"])
    with pytest.raises(ValueError):
        losses.LossAdaAttN(losses.LossAdaAttNCfg(content_loss_layers=(6,)))
    with pytest.raises(ValueError):
        losses.LossAdaAttN(losses.LossAdaAttNCfg(content_loss_layers=(4,)), losses.NormalizedVGG(depth=3))


def test_normalized_vgg_layout():
    net = losses.NormalizedVGG()
    assert list(net.state_dict().keys()) == [str(k) for k in GOLD["vgg_keys"]]
    assert [ai.slice_key(k) for k in net.all_keys] == list(net.state_dict().keys())
    sd = ai.vgg_state_dict()
    res = net.load_normalised_vgg(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.slice2[0].weight, sd["5.weight"]) and torch.equal(net.slice5[3].bias, sd["42.bias"])
    assert not any(p.requires_grad for p in net.parameters())
    shallow = losses.NormalizedVGG(depth=3)
    assert list(shallow.state_dict().keys()) == [str(k) for k in GOLD["vgg_keys"] if int(str(k)[5]) <= 3]
    shallow.load_normalised_vgg(sd)                                   # the whole file is accepted, the deeper slices are not kept
    with pytest.raises(KeyError):
        shallow.load_normalised_vgg({k: v for k, v in sd.items() if k != "42.bias"})
    with pytest.raises(KeyError):
        net.load_normalised_vgg({**sd, "44.weight": sd["42.weight"]})
    with pytest.raises(RuntimeError):
        net.load_normalised_vgg({**sd, "5.weight": sd["2.weight"]})
    x = torch.rand(1, 3, 8, 12)                                       # a shallow VGG takes images the reference's five slices refuse
    feats = shallow(x)
    assert [tuple(f.shape) for f in feats] == [(1, 64, 8, 12), (1, 128, 4, 6), (1, 256, 2, 3)]


def test_nothing_of_the_vgg_enters_a_train_step_state_dict():
    from styl3r_amd.train import TrainStep
    enc = torch.nn.Sequential(torch.nn.Linear(4, 4))
    enc.forward = lambda context, global_step: None                   # (only its signature is looked at)
    loss = losses.LossAdaAttN()
    step = TrainStep(enc, torch.nn.Identity(), extra_losses=[loss])
    sd = step.state_dict()
    assert set(sd["encoder"]) == {"0.weight", "0.bias"}
    ids = {id(p) for p in loss.parameters()}
    assert not any(id(p) in ids for g in step.optimizer.param_groups for p in g["params"])


def test_symbols_and_argument_checks_without_a_device():
    vit_ops.build_library()
    lib = vit_ops.load()
    header = (ROOT / "include/vit_ops.h").read_text()
    for name in ("vit_adaattn_stats", "vit_adaattn_l1_scratch_bytes", "vit_adaattn_l1"):
        assert name in vit_ops.EXPORTS and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", header)
    one = C.c_void_p(64)                                              # (validation only: nothing is dereferenced but the host index)
    idx = (C.c_int32 * 3)(0, 0, 1)
    ip = C.cast(idx, C.c_void_p)
    ok = dict(Bq=3, Bs=2, D=448, C=256, Nq=200, M=150)
    call = lambda ptrs=(one, one, one, ip, one), outs=(one, one), **kw: lib.vit_adaattn_stats(
        *ptrs, *[{**ok, **kw}[k] for k in ("Bq", "Bs", "D", "C", "Nq", "M")], *outs, None)
    for i in range(5):
        assert call(ptrs=tuple(None if j == i else p for j, p in enumerate((one, one, one, ip, one)))) == -1
    assert call(outs=(None, one)) == -1 and call(outs=(one, None)) == -1
    assert call(D=100) == -1 and call(D=0) == -1 and call(C=96) == -1 and call(C=0) == -1 and call(M=0) == -1 and call(Nq=0) == -1
    assert call(D=512) == -1 and call(C=320) == -1                    # beyond the kernel's fast path: the caller routes to the expression
    assert call(Bs=1) == -1                                           # index 1 outside [0, 1)
    idx[1] = -1
    assert call() == -1
    assert lib.vit_adaattn_l1_scratch_bytes(3, 64) == 3 * 64 * 8 and lib.vit_adaattn_l1_scratch_bytes(0, 64) == 0
    l1 = lambda *a: lib.vit_adaattn_l1(*a, None)
    assert l1(None, one, one, one, 1, 1, 1, one, one, one, None) == -1 and l1(one, one, one, None, 1, 1, 1, one, one, one, None) == -1
    assert l1(one, one, one, one, 1, 1, 1, None, one, one, None) == -1 and l1(one, one, one, one, 1, 1, 1, one, None, one, None) == -1
    assert l1(one, one, one, one, 1, 1, 1, one, one, None, None) == -1
    assert l1(one, one, one, one, 0, 1, 1, one, one, one, None) == -1 and l1(one, one, one, one, 1, 1, 0, one, one, one, None) == -1


def test_cpu_tensors_take_the_expression_route():
    q_hat, k_hat, s, index = ai.stats_inputs("diffuse")
    n0 = dict(losses.CALLS)
    mean, std = losses.adaattn_stats(q_hat, k_hat, s, index)
    assert losses.CALLS["adaattn_expr_stats"] == n0["adaattn_expr_stats"] + 1 and losses.CALLS["adaattn_hip_stats"] == n0["adaattn_hip_stats"]
    assert mean.shape == std.shape == (3, 64, 70)
    m64, s64 = losses.adaattn_stats_expression(q_hat.double(), k_hat.double(), s.double(), index)
    assert (mean - m64).abs().max() < 1e-4 and (std.double() ** 2 - s64 ** 2).abs().max() < 1e-3
    assert torch.equal(mean[0], mean[1]) is False and std.min() >= 0
    with pytest.raises(ValueError, match="style_index"):
        losses.adaattn_stats(q_hat, k_hat, s)                         # three images, two styles, no map
    with pytest.raises(ValueError, match="k_hat"):
        losses.adaattn_stats(q_hat, k_hat, s[:, :, :149], index)
    p, c, mu, sd, ties = ai.tail_inputs((3, 64, 70))
    details = {}
    loss = losses.adaattn_l1(p.requires_grad_(True), c, mu, sd, details)
    loss.backward()
    assert losses.CALLS["adaattn_hip_l1"] == n0["adaattn_hip_l1"]
    assert torch.equal(p.grad, details["feature_grad"]) and (p.grad.view(-1)[ties] == 0).all()

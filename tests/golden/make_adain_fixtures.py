"""Generates tests/golden/adain_ref.npz from the REFERENCE's own modules:
  * `AdaIN2D.generate`, `adain`, `calc_mean_std`, `VGGEncoder`, `Decoder`   src/test/vgg_model.py:19-159
  * `vgg_denorm`                                                           src/model/model_wrapper_style.py:51-55
  * the two wrapper sites' calling code (:281-285, :538-542): normalise, repeat the style per view, generate(.., 1), vgg_denorm
torchvision is not installed here: the stub below supplies `torchvision.models.vgg19` (the stock `features` layout; the weights are then
loaded from tests/adain_inputs.reference_state_dict, closed forms under the reference's own keys) and `transforms.Normalize`
((x - mean) / std per channel with the constants in the tensor's dtype, its documented definition).  model_wrapper_style.py cannot be
imported (it pulls in the training stack), so `vgg_denorm` is compiled from its source text, the function alone.  Everything runs in float64.
The fixture holds no weights: the key list and shapes of the reference's state dict, the images, relu4_1 of content and style, the AdaIN
output, the decoder's raw output and the pre-clamp and final pictures of scenes A and B (tests/adain_inputs.SCENES).
    python tests/golden/make_adain_fixtures.py
"""
import ast
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import torch
from torch import nn

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import adain_inputs as ai
from tests.golden.ref_stubs import REF, install

install()
# ---- torchvision stub -------------------------------------------------------------------------------------------
tv = types.ModuleType("torchvision"); tvm = types.ModuleType("torchvision.models"); tvt = types.ModuleType("torchvision.transforms")
_CFG_E = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


def vgg19(pretrained=False, **kw):
    layers, c = [], 3
    for v in _CFG_E:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(c, v, 3, padding=1), nn.ReLU(inplace=True)]; c = v
    return types.SimpleNamespace(features=nn.Sequential(*layers))


class Normalize(nn.Module):
    def __init__(self, mean, std):
        super().__init__()
        self.mean, self.std = list(mean), list(std)

    def forward(self, x):
        m = torch.tensor(self.mean, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        s = torch.tensor(self.std, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        return (x - m) / s


tvm.vgg19 = vgg19; tvt.Normalize = Normalize; tv.models = tvm; tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.transforms": tvt})
vm = importlib.import_module("src.test.vgg_model")

# ---- vgg_denorm, compiled from the wrapper's source ----------------------------------------------------------------
tree = ast.parse((Path(REF) / "src/model/model_wrapper_style.py").read_text())
fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "vgg_denorm")
scope = {"torch": torch}
exec(compile(ast.Module(body=[fn], type_ignores=[]), "model_wrapper_style.py", "exec"), scope)
vgg_denorm = scope["vgg_denorm"]

# ---- the model ------------------------------------------------------------------------------------------------------
model = vm.AdaIN2D()
keys = list(model.state_dict().keys())
print(model.load_state_dict(ai.reference_state_dict(), strict=True))
model = model.double()
vgg_normalize = Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
out = {"keys": np.array(keys), "shapes": np.array([";".join(map(str, model.state_dict()[k].shape)) for k in keys])}

for scene in ai.SCENES:
    target32, style32 = ai.images(scene)
    views = target32.shape[0]
    with torch.no_grad():
        # what the wrapper's two sites do: normalised targets, the normalised style once per view, generate at alpha 1, vgg_denorm
        content = vgg_normalize(target32.double())
        style_rows = vgg_normalize(style32.double())[None].expand(views, -1, -1, -1).contiguous()
        raw = model.generate(content, style_rows, 1)
        final = vgg_denorm(raw)
        # the intermediates, from the same modules
        fc = model.vgg_encoder(content, output_last_feature=True)
        fs_views = model.vgg_encoder(style_rows, output_last_feature=True)
        fs = fs_views[:1]
        t = vm.adain(fc, fs_views)
        assert torch.equal(model.decoder(t), raw)
        raw03 = model.generate(content, style_rows, 0.3)
    # the picture before the clamp: ImageNet constants as fp32 values (vgg_denorm builds them as fp32 tensors), arithmetic in float64
    scale = torch.tensor(ai.IMAGENET_STD, dtype=torch.float32).double().view(3, 1, 1)
    shift = torch.tensor(ai.IMAGENET_MEAN, dtype=torch.float32).double().view(3, 1, 1)
    preclamp = raw * scale + shift
    assert torch.equal(preclamp.clamp(0, 1), final)
    # conditioning: AdaIN divides by the content std; a near-dead channel would turn a 1e-7 feature difference into an O(1) output difference
    ratio = float(fc.flatten(2).std(-1).min() / fc.abs().max())
    assert ratio >= 1e-3, f"scene {scene}: a content channel's std at relu4_1 is {ratio:.2e} of the tensor's |max|"
    # clamp coverage: the clamp must not hide an error
    inside = float(((preclamp > 0) & (preclamp < 1)).double().mean())
    assert inside >= 0.25, f"scene {scene}: only {inside:.2%} of the pre-clamp values lie inside (0, 1)"
    per_channel = ((preclamp > 0) & (preclamp < 1)).double().mean(dim=(0, 2, 3)).tolist()
    print(f"scene {scene}: relu4_1 {tuple(fc.shape)} min std / |max| {ratio:.2e}; inside (0, 1): {inside:.2%} (per channel {per_channel}); "
          f"raw |max| {float(raw.abs().max()):.3f}")
    out.update({f"{scene}_images": target32.numpy(), f"{scene}_style": style32.numpy(), f"{scene}_relu41_content": fc.numpy(),
                f"{scene}_relu41_style": fs.numpy(), f"{scene}_adain": t.numpy(), f"{scene}_raw": raw.numpy(),
                f"{scene}_raw_alpha03": raw03.numpy(), f"{scene}_preclamp": preclamp.numpy(), f"{scene}_final": final.numpy()})

path = ROOT / "tests/golden/adain_ref.npz"
np.savez_compressed(path, **out)
print("adain fixture:", len(keys), "keys,", path.stat().st_size, "bytes")

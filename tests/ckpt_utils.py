"""Shared by the checkpoint tests: a hand-made "encoder" of a dozen tensors that `train.TrainStep` can drive on the CPU and on the GPU
(two learning-rate groups by the NVS-stage name rules, a frozen buffer, odd sizes), a decoder stand-in and a loss."""
from types import SimpleNamespace

import torch
from torch import nn


class HandEncoder(nn.Module):
    """forward(context, global_step) -> (B, 24) "gaussians" from the 64 values of each context image.  `backbone.*` is the pretrained group,
    `gaussian_param_head.*` the new one; on a GPU the three wide layers go through vit_ops.fused_linear, so the pre-split weight cache is
    in play."""
    stylized = False

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.backbone = nn.Sequential(nn.Linear(64, 128), nn.Linear(128, 64))
        self.gaussian_param_head = nn.Sequential(nn.Linear(64, 64), nn.Linear(64, 24))
        self.odd = nn.Parameter(torch.zeros(5, 3))
        self.register_buffer("table", torch.arange(7, dtype=torch.int64))
        self.register_buffer("scale", torch.full((3,), 0.5))
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)

    def _linear(self, layer, x):
        if x.is_cuda:
            from styl3r_amd import vit_ops
            return vit_ops.fused_linear(x, layer.weight, layer.bias)
        return nn.functional.linear(x, layer.weight, layer.bias)

    def forward(self, context, global_step):
        x = context["image"].reshape(context["image"].shape[0], -1)
        h = torch.tanh(self._linear(self.backbone[0], x))
        h = torch.tanh(self._linear(self.backbone[1], h))
        h = torch.tanh(self._linear(self.gaussian_param_head[0], h))
        return self.gaussian_param_head[1](h) + self.odd.sum() * self.scale.sum()


class HandDecoder:
    def forward(self, g, extrinsics, intrinsics, near, far, image_shape, **kw):
        return SimpleNamespace(color=g)


def hand_loss(out, batch, g, global_step):
    return (out.color - batch["target"]["image"].reshape(out.color.shape[0], -1)[:, :24]).pow(2).mean()


def hand_batch(device="cpu", seed=0, b=128):
    g = torch.Generator().manual_seed(100 + seed)
    z = torch.zeros(b, 1, device=device)
    return dict(context=dict(image=torch.randn(b, 1, 4, 4, 4, generator=g).to(device)),
                target=dict(image=torch.randn(b, 1, 3, 4, 4, generator=g).to(device), extrinsics=z, intrinsics=z, near=z, far=z))


def hand_train_step(device="cpu", **kw):
    from styl3r_amd.train import TrainStep
    enc = HandEncoder().to(device)
    kw.setdefault("warm_up_steps", 3)
    kw.setdefault("max_steps", 20)
    kw.setdefault("lr", 1e-2)
    return TrainStep(enc, HandDecoder(), losses=[hand_loss], **kw)

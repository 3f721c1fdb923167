"""The frozen point-map teacher of the distillation stage (src/model/distiller/__init__.py, dust3d_backbone.py): a DUSt3R / MASt3R
network -- the CroCo trunk this package already runs, two cross-attending decoders and two 4-channel DPT heads -- that turns the first
two context views into `pts3d` (b,h,w,3), both in view 1's frame, plus a confidence (b,h,w).

Same state-dict keys as the reference class (`patch_embed.*`, `enc_blocks.*`, `enc_norm.*`, `mask_token`, `decoder_embed.*`,
`dec_blocks.*`, `dec_blocks2.*`, `dec_norm.*`, `downstream_head1/2.dpt.*`), so the published checkpoints load unchanged.  On the device
everything runs on the package's kernels: the encoder / decoder blocks (both views as one batch; at serving shapes the two decoders as
two-problem launches), the DPT heads, and the head post-processing in one pass (gsr_pointmap_post).  The derived weight images come from
the versioned weak cache of vit_ops: a frozen teacher builds them once."""
from __future__ import annotations

from typing import Optional

import torch

from .encoder import AsymmetricCroCoMulti, BackboneCrocoCfg, head_factory

inf = float("inf")

DISTILLER_PARAMS = dict(enc_depth=24, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=768, enc_num_heads=16, dec_num_heads=12,
                        pos_embed="RoPE100", img_size=(512, 512))
DISTILLER_WEIGHTS = {"dust3r": "./pretrained_weights/DUSt3R_ViTLarge_BaseDecoder_512_dpt.pth",
                     "mast3r": "./ckpts/MASt3R_ViTLarge_BaseDecoder_512_catmlpdpt_metric.pth"}


class Dust3R(AsymmetricCroCoMulti):
    """`Dust3R(CroCoNet)` (dust3d_backbone.py:20-208).  Built on the trunk of the student's backbone without an intrinsics embedding;
    `load_state_dict` (inherited) copies `dec_blocks.*` into `dec_blocks2.*` for a checkpoint that lacks the second decoder."""

    def __init__(self, output_mode="pts3d", head_type="dpt", depth_mode=("exp", -inf, inf), conf_mode=("exp", 1, inf), freeze="none",
                 landscape_only=True, patch_embed_cls="PatchEmbedDust3R", **croco_kwargs):
        assert patch_embed_cls == "PatchEmbedDust3R" and landscape_only
        assert (output_mode, head_type) == ("pts3d", "dpt") and tuple(depth_mode) == ("exp", -inf, inf) and tuple(conf_mode) == ("exp", 1, inf), \
            "the teacher is the DPT point head with the ('exp', -inf, inf) depth and ('exp', 1, inf) confidence modes"
        cfg = BackboneCrocoCfg(name="croco_multi", asymmetry_decoder=True, intrinsics_embed_loc="none", intrinsics_embed_type="pixelwise")
        super().__init__(cfg, 3, dict(croco_kwargs))
        self.depth_mode, self.conf_mode = tuple(depth_mode), tuple(conf_mode)
        self.output_mode, self.head_type = output_mode, head_type
        self.downstream_head1 = head_factory(head_type, output_mode, self, has_conf=True)
        self.downstream_head2 = head_factory(head_type, output_mode, self, has_conf=True)
        self.set_freeze(freeze)
        self.eval()

    def set_freeze(self, freeze: str) -> None:
        self.freeze = freeze
        frozen = {"none": [], "mask": [self.mask_token], "encoder": [self.mask_token, self.patch_embed, self.enc_blocks]}[freeze]
        for m in frozen:
            for p in ([m] if isinstance(m, torch.nn.Parameter) else m.parameters()):
                p.requires_grad = False

    def train(self, mode: bool = True):
        return super().train(False)            # a teacher: always in eval mode

    @torch.no_grad()
    def forward(self, context: dict, symmetrize_batch: bool = False, return_views: bool = False, normalize: bool = False):
        """context["image"] (b, v >= 2, 3, h, w) in [-1, 1] (`normalize`: in [0, 1]); views 0 and 1 are used.  -> (res1, res2), each
        {"pts3d" (b,h,w,3), "conf" (b,h,w)}; res2's points are view 2's in view 1's frame."""
        if symmetrize_batch:
            raise NotImplementedError("symmetrize_batch: no training wrapper passes it")
        image = context["image"]
        b, v, _, h, w = image.shape
        assert v >= 2
        pair = image[:, :2]
        if normalize:
            pair = (pair - 0.5) / 0.5
        feat, pos = self._encode_image(pair.reshape(b * 2, 3, h, w), None)          # both views as one batch
        outs = self._decoder_split(feat.view(b, 2, feat.shape[1], -1), pos.view(b, 2, pos.shape[1], 2))
        with torch.autocast("cuda", enabled=False):
            res1 = self.downstream_head1([a.float() for a, _ in outs], (h, w))
            res2 = self.downstream_head2([r.float() for _, r in outs], (h, w))
        if h > w:        # transpose_to_landscape on a portrait batch (see encoder.landscape_mean_head)
            res1, res2 = ({k: t.swapaxes(1, 2) for k, t in r.items()} for r in (res1, res2))
        if return_views:
            return res1, res2, {"img": pair[:, 0]}, {"img": pair[:, 1]}
        return res1, res2

    def estimate_pose(self, context, normalize=False):
        raise NotImplementedError("estimate_pose needs the global aligner, which the reference itself never imports")


def get_distiller(name: str, weight_path: Optional[str] = None) -> Dust3R:
    """`get_distiller` (distiller/__init__.py:9-23): the full-size teacher, in eval mode, with the checkpoint's 'model' state dict loaded
    (strictly for DUSt3R; MASt3R carries a descriptor head the point teacher does not have).  weight_path: default = the reference's."""
    assert name in ("dust3r", "mast3r"), f"unexpected name={name}"
    distiller = Dust3R(head_type="dpt", output_mode="pts3d", depth_mode=("exp", -inf, inf), conf_mode=("exp", 1, inf),
                       patch_embed_cls="PatchEmbedDust3R", **DISTILLER_PARAMS).eval()
    ckpt = torch.load(weight_path or DISTILLER_WEIGHTS[name], map_location="cpu", weights_only=False)["model"]
    distiller.load_state_dict(ckpt, strict=name != "mast3r")
    for p in distiller.parameters():          # convert_to_buffer(distiller) of the wrappers: nothing of the teacher is trained
        p.requires_grad = False
    return distiller

"""Shared by tests/test_vis_host.py and tests/test_gpu_vis.py: the fixture tests/golden/validation_vis.npz (the reference's drawing run in
float64, tests/golden/make_validation_vis_fixtures.py) and the comparisons both files make -- on the host for the float64 restatement, on
the device for the kernel.

Tolerances.  Coverage is an integer (alpha * 64) and is compared exactly.  A picture is compared with the golden float64 picture rounded to
fp32, within 2^-22 absolute: one fp32 rounding of a value in [0, 1] (2^-24) plus the golden value's own rounding (2^-24), doubled; the
float64 sums of at most 64 terms contribute nothing at that scale.  The same bar holds between the device and the host restatement.  No
pixel is set aside."""
import json
from pathlib import Path

import numpy as np
import torch

from styl3r_amd import visualization as vis

T = np.load(Path(__file__).resolve().parent / "golden" / "validation_vis.npz", allow_pickle=False)
DRAW_CASES = [str(x) for x in T["draw_cases"]]
CAM_CASES = [str(x) for x in T["cam_cases"]]
TOL = 2.0 ** -22


def draw_case(name):
    """-> (kind, image (3,h,w) fp32, [keyword dicts of the draw calls, arrays as fp32 tensors])"""
    calls = []
    for call in json.loads(str(T[f"draw_{name}_calls"])):
        calls.append({k: (torch.tensor(np.asarray(v, dtype=np.float32)) if isinstance(v, list) and k not in ("x_range", "y_range") else v)
                      for k, v in call.items()})
    return str(T[f"draw_{name}_kind"]), torch.from_numpy(T[f"draw_{name}_image"]), calls


def case_layers(name):
    kind, image, calls = draw_case(name)
    layers = []
    for call in calls:
        call = dict(call)
        make = {"lines": vis.line_layer, "points": vis.point_layer}[call.pop("fn", kind)]
        layers.append(make(image.shape[1:], **call))
    return image, layers


def golden32(key):
    return torch.from_numpy(T[key]).to(torch.float32)


def max_diff(a, b):
    return float((a.double() - b.double()).abs().max())


def coverage64(layer, shape, device):
    """alpha * 64 of one layer from two drawings, over black and over white: white - black = 1 - alpha in every channel, whatever the
    colours; each picture is within 2^-24 of its value, so 64 alpha is recovered to 2^-17 and must be an integer"""
    h, w = shape
    base = torch.stack([torch.zeros((3, h, w)), torch.ones((3, h, w))]).to(device)
    black, white = vis.draw_layers(base, [[layer], [layer]]).cpu().double()
    a64 = 64 * (1 - (white - black))
    assert float((a64 - a64.round()).abs().max()) < 1e-3, "alpha * 64 is not an integer"
    assert torch.equal(a64[0].round(), a64[1].round()) and torch.equal(a64[0].round(), a64[2].round())
    return a64[0].round()


def check_draw_case(name, device):
    """one fixture case through `draw_layers` on `device`: the picture and every layer's coverage"""
    image, layers = case_layers(name)
    got = vis.draw_layers(image[None].to(device), [layers])[0].cpu()
    assert got.dtype == torch.float32
    d = max_diff(got, golden32(f"draw_{name}_gold"))
    print(f"{name} on {device}: max |picture - golden| = {d:.3g}")
    alphas = torch.from_numpy(T[f"draw_{name}_alpha"])
    for layer, alpha in zip(layers, alphas):
        assert torch.equal(coverage64(layer, image.shape[1:], device), alpha * 64), f"{name}: coverage differs"
    assert d <= TOL, (name, d)


def camera_inputs():
    return (torch.from_numpy(T["cam_E"]), torch.from_numpy(T["cam_K"]), torch.from_numpy(T["cam_color"]),
            torch.from_numpy(T["cam_near"]), torch.from_numpy(T["cam_far"]))


def camera_kwargs(name):
    return {k: (torch.tensor(np.asarray(v, dtype=np.float32)) if isinstance(v, list) else v) for k, v in json.loads(str(T[f"cam_{name}_kwargs"])).items()}


def check_camera_case(name, device):
    E, K, color, _, _ = camera_inputs()
    got = vis.draw_cameras(48, E.to(device), K.to(device), color, **camera_kwargs(name)).cpu()
    assert got.shape == (3, 3, 48, 48) and got.dtype == torch.float32
    d = max_diff(got, golden32(f"cam_{name}_gold"))
    print(f"cameras {name} on {device}: max |picture - golden| = {d:.3g}")
    stacks = vis.camera_layers(48, E, K, color, **camera_kwargs(name))
    alphas = iter(torch.from_numpy(T[f"cam_{name}_alpha"]))
    for stack in stacks:
        for layer in stack:
            assert torch.equal(coverage64(layer, (48, 48), device), next(alphas) * 64), f"cameras {name}: coverage differs"
    assert d <= TOL, (name, d)

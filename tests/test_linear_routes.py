"""CPU test: vit_ops._linear_cfg -- the one route of every fused-Linear launch -- reproduces the table recorded from the functions it replaced
(tests/golden/linear_routes.json: the commit, the grid and the cell order are inside the file; it is never regenerated from the code under test).
Needs only the cross-compiled library: vit_linear_sm_ok / vit_linear_sm_set are host functions."""
import json
from pathlib import Path

import pytest

GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "linear_routes.json").read_text())


@pytest.fixture
def vo():
    from styl3r_amd import vit_ops
    vit_ops.build_library()
    yield vit_ops
    vit_ops._SMALL_M_SET.clear()           # (the next user of this thread re-states SMALL_M_ROWS to the library)
    if vit_ops.LINEAR_MODE != "f32":
        vit_ops._x6()


@pytest.mark.parametrize("switch", list(GOLD["switches"]))
@pytest.mark.parametrize("mode", GOLD["modes"])
def test_one_route_function_reproduces_the_recorded_routes_and_layouts(mode, switch, vo, monkeypatch):
    assert GOLD["modes"] == ["bf16x6", "bf16x3", "f16x3", "f32"] and len(GOLD["M"]) == 12 and len(GOLD["NK"]) == 17
    monkeypatch.setattr(vo, "LINEAR_MODE", mode)
    for name, value in GOLD["switches"][switch].items():
        monkeypatch.setattr(vo, name, value)
    if mode != "f32":
        vo._x6()                                                    # (what every call site does first: the library's products per launch follow the mode)
    other = "bf16x6" if mode != "bf16x6" else "f16x3"
    cells = GOLD["routes"][mode][switch]
    shapes = [(M, N, K) for M in GOLD["M"] for N, K in GOLD["NK"]]
    assert len(cells) == 4 * len(shapes)
    seen = set()
    for i, (M, N, K) in enumerate(shapes):
        want = tuple(int(c) for c in cells[4 * i:4 * i + 4])
        fwd, dx = vo._linear_cfg(M, N, K), vo._linear_cfg(M, N, K, dx=True, mode=mode)
        got = (fwd, dx, vo._linear_cfg(M, N, K, serving=True), vo._linear_cfg(M, N, K, dx=True, mode=other))
        assert got == want, (mode, switch, M, N, K, got, want)
        assert vo._linear_cfg(M, N, K, dx=True) == dx               # (the forward's spelling of the same question, for the pair split)
        # the layout rule: the block flags the forward hands to split_weight_pair are those of the two launches' routes
        assert (bool(want[0]), bool(want[1])) == (fwd != 0, dx != 0)
        seen.update(got)
    assert seen <= {0, 1, 3, 5}                                       # cfg 2 is no route
    if mode != "f32" and switch == "default":
        assert seen == ({0, 1, 3, 5})
    if mode == "f32":
        assert seen == {0}

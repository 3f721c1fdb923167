"""No GPU: the cases, the yardstick and the backward closed form of the Gaussian-adapter tests (tests/adapter_cases.py).

The kernel test (test_gpu_adapter.py) holds csrc/vit_adapter.hip against the float64 expression per regime and per gradient group.  What
can be settled without a device is settled here: every Gaussian of a case lies in its regime, the float64 expression is finite there, the
recorded float32 yardstick is what this machine measures, and the kernel's hand-derived backward -- restated on whole tensors in
`closed_form_backward` -- is the derivative of the expression in every regime."""
import math

import pytest
import torch

from tests import adapter_cases as ac

CASES = [(r, l) for r in ac.REGIMES for l in ac.LAYOUTS]


@pytest.mark.parametrize("regime,layout", CASES)
def test_every_gaussian_lies_in_its_regime(regime, layout):
    case = ac.case_of(regime, layout)
    ok = ac.regime_predicate(case)
    assert ok.shape == (case.b, case.v * case.H * case.W)
    assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} Gaussians outside {regime}"
    for t in case.ins:
        if t is not None:
            assert t.dtype == torch.float64 and bool((t.float().double() == t).all()), "inputs must be float32 values"
    xyz, dens, _, _ = ac.raw_values(case)
    if regime == "tiny_xyz":
        zero = (xyz == 0).all(-1)
        assert 3 <= int(zero.sum()) <= 8 and bool(zero.flatten()[0]) and bool(zero.flatten()[-1])       # first and last thread included
    if regime == "dens_sat":
        assert bool((dens > 0).any()) and bool((dens < 0).any())


def test_layouts_cover_the_shapes():
    rows = list(ac.LAYOUTS.values())
    assert {r[0] for r in rows} == {1, 2} and {r[1] for r in rows} == {1, 3} and {r[2:4] for r in rows} == {(8, 16), (5, 7)}
    assert {r[4] for r in rows} == {0, 2} and {r[5] for r in rows} == {True, False}
    assert any(r[0] * r[1] * r[2] * r[3] % 256 for r in rows) and any(r[0] * r[1] * r[2] * r[3] > 256 for r in rows)


@pytest.mark.parametrize("regime,layout", CASES)
def test_float64_expression_is_finite(regime, layout):
    for e in ac.EXPONENTS:
        for name, t in ac.reference(regime, layout, e).items():
            assert bool(torch.isfinite(t).all()), (e, name)


@pytest.mark.parametrize("regime", ac.REGIMES)
def test_reference_zeros_are_exact(regime):
    """what the kernel tests demand bit for bit is what the float64 autograd gives: no gradient above the clamp, none at q = 0"""
    for layout in ac.LAYOUTS:
        for e in ac.EXPONENTS:
            ac.assert_exact_zeros(ac.reference(regime, layout, e), regime, f"float64 {layout} {e}")
    if regime in ("clamp_all", "iso"):                      # the quaternion gradient is cancellation residue, far below its terms
        for layout in ac.LAYOUTS:
            want = ac.reference(regime, layout, 1.0)["d_quaternion"]
            assert float(want.abs().max()) <= 1e-6 * ac.conditioning_scale(ac.case_of(regime, layout))


@pytest.mark.parametrize("regime", ac.REGIMES)
def test_recorded_yardstick_is_what_the_float32_expression_gives(regime):
    """YARDSTICK[regime][group] = error of the float32 element-wise expression against float64, max over layouts and exponents.  The bars
    use the record, not this machine's measurement; a fresh measurement stays within a factor 2 of it (another libm's or vector width's
    last bits move a maximum of rounding errors by that much): never above twice the record unless the floor governs anyway, and
    never below half of a record that moves a bar."""
    live = ac.measured_yardstick(regime)
    print()
    for n in ac.FORWARD + ac.GRADIENT:
        rec = ac.YARDSTICK[regime][n]
        print(f"    [yardstick] {regime:16s} {n:13s} measured {live[n]:.2e} recorded {rec:.2e} bar {ac.bar(regime, n):.2e}")
        assert live[n] <= max(2 * rec, ac.FLOOR[n] / ac.YARDSTICK_FACTOR), (n, live[n], rec)
        if ac.YARDSTICK_FACTOR * rec > ac.FLOOR[n]:
            assert live[n] >= rec / 2, (n, live[n], rec)


def test_only_known_entries_rise_above_the_floor():
    above = {(r, n) for r in ac.REGIMES for n in ac.FORWARD + ac.GRADIENT if ac.bar(r, n) > ac.FLOOR[n]}
    # Sigma of a clamped axis is 0.09 against s^2 <= 4e-5 of the others: the maximum is one product of rounded R entries; the opacity map
    # and p (1 - p) are formed from a rounded p within 3e-4 of 0 or 1
    assert above == {("clamp_all", "cov"), ("clamp_one", "cov"), ("dens_sat", "opac"), ("dens_sat", "d_density")}


@pytest.mark.parametrize("regime,layout", CASES)
def test_closed_form_backward_is_the_gradient_of_the_expression(regime, layout):
    case = ac.case_of(regime, layout)
    print()
    for e in ac.EXPONENTS:
        want = {n: t for n, t in ac.reference(regime, layout, e).items() if n in ac.GRADIENT}
        got = ac.closed_form_backward(case, e)
        errs = ac.group_errors(got, want, case)
        print(f"    [closed form] {regime:16s} {layout:22s} e={e}: " + " ".join(f"{n} {x:.1e}" for n, x in errs.items()))
        ac.assert_within_bars(errs, regime, f"{regime} {layout} exponent {e}")
        ac.assert_exact_zeros(got, regime, f"{regime} {layout} exponent {e}")


@pytest.mark.parametrize("layout", list(ac.LAYOUTS))
def test_closed_form_in_float64_leaves_only_rounding(layout):
    """the same formulas in float64: 1e-12 of every group -- the float32 bars above are not what makes the closed form pass"""
    for regime in ac.REGIMES:
        case = ac.case_of(regime, layout)
        want = {n: t for n, t in ac.reference(regime, layout, 1.7).items() if n in ac.GRADIENT}
        errs = ac.group_errors(ac.closed_form_backward(case, 1.7, torch.float64), want, case)
        assert max(errs.values()) < 1e-12, (regime, errs)


@pytest.mark.parametrize("layout", list(ac.LAYOUTS))
def test_a_missing_radial_term_below_the_clip_is_caught(layout):
    """for 0 < |xyz| < 1e-8 the forward is xyz / 1e-8 * expm1(d), whose derivative keeps xyz xyz^T (f + 1) / (1e-8 d) -- as large as the
    f / 1e-8 term.  The kernel's earlier closed form set that coefficient to 0: tiny_xyz rejects it, by five orders of magnitude over
    the bar, and no other regime and no other group notices."""
    case = ac.case_of("tiny_xyz", layout)
    want = {n: t for n, t in ac.reference("tiny_xyz", layout, 1.0).items() if n in ac.GRADIENT}
    errs = ac.group_errors(ac.closed_form_backward(case, 1.0, radial_below_clip=False), want, case)
    assert errs["d_pts"] > 0.1, errs
    with pytest.raises(AssertionError):
        ac.assert_within_bars(errs, "tiny_xyz", "earlier closed form")
    del errs["d_pts"]
    ac.assert_within_bars(errs, "tiny_xyz", "earlier closed form, other groups")
    normal = ac.case_of("normal", layout)
    want = {n: t for n, t in ac.reference("normal", layout, 1.0).items() if n in ac.GRADIENT}
    ac.assert_within_bars(ac.group_errors(ac.closed_form_backward(normal, 1.0, radial_below_clip=False), want, normal), "normal", "earlier form")


def test_the_issue_example_below_the_clip():
    """xyz = (3e-9, 0, 0), upstream (1, 2, 3): autograd gives (0.6, 0.6, 0.9); without the radial term the first entry is 0.3"""
    from styl3r_amd.encoder import reg_dense_depth_exp
    for dtype in (torch.float32, torch.float64):
        x = torch.tensor([3e-9, 0.0, 0.0], dtype=dtype, requires_grad=True)
        (reg_dense_depth_exp(x) * torch.tensor([1.0, 2.0, 3.0], dtype=dtype)).sum().backward()
        assert torch.allclose(x.grad, torch.tensor([0.6, 0.6, 0.9], dtype=dtype), rtol=1e-6)


def test_group_errors_counts_nonfinite_and_nonzero_against_an_exact_zero():
    case = ac.case_of("clamp_all", "packed_b2_v1_5x7_sh0")
    want = ac.reference("clamp_all", "packed_b2_v1_5x7_sh0", 1.0)
    got = {n: t.clone() for n, t in want.items()}
    assert max(ac.group_errors(got, want, case).values()) == 0
    got["d_scale"][0, 0, 0] = 1e-30
    got["means"][0, 0, 0] = math.nan
    errs = ac.group_errors(got, want, case)
    assert errs["d_scale"] == math.inf and errs["means"] == math.inf and errs["cov"] == 0
    with pytest.raises(AssertionError):
        ac.assert_exact_zeros(got, "clamp_all", "planted")

"""-m gpu: the kernels of csrc/gsr_views.hip (k_view_tables, k_view_overlap behind gsr_view_overlap) through styl3r_amd/views.py, against
the reference's counts (tests/golden/view_selection.npz) and against the float64 host path of the same module (which
tests/test_views_host.py holds to the same fixture).  Every comparison is of integers: there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import views as vw
from tests.views_common import DEGENERATE_CASES, OVERLAP_CASES, T, check_index, check_overlap_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def cameras(n, seed, spread=0.25):
    """n seeded views around the origin looking roughly the same way, with unequal focal lengths and off-centre principal points"""
    g = torch.Generator().manual_seed(seed)
    E = torch.eye(4).repeat(n, 1, 1)
    for v in range(n):
        a, b, c = ((torch.rand(3, generator=g) - 0.5) * 2 * spread).tolist()
        ry = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = torch.tensor([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        rz = torch.tensor([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        E[v, :3, :3] = (ry @ rx @ rz).float()
        E[v, :3, 3] = (torch.rand(3, generator=g) - 0.5) * 2 * spread
    K = torch.eye(3).repeat(n, 1, 1)
    K[:, 0, 0] = torch.rand(n, generator=g) * 0.4 + 0.7
    K[:, 1, 1] = torch.rand(n, generator=g) * 0.4 + 1.0
    K[:, 0, 2] = torch.rand(n, generator=g) * 0.1 + 0.45
    K[:, 1, 2] = torch.rand(n, generator=g) * 0.1 + 0.45
    return E, K


def device_and_host(E, K, pairs, shape):
    got, _ = vw.view_overlap(E.to(DEV), K.to(DEV), pairs, shape)
    want, _ = vw.view_overlap(E, K, pairs, shape)
    return got.cpu(), want


@pytest.mark.parametrize("key", OVERLAP_CASES + DEGENERATE_CASES)
def test_every_fixture_case_on_the_device(key):
    check_overlap_case(key, DEV)


# one ray, one short of a wave, a wave, one more; a row that is no multiple of anything with three blocks' worth of rays split unevenly
@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (8, 8), (5, 13), (3, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_on_small_and_odd_shapes(shape):
    E, K = cameras(5, 31)
    pairs = [(0, 1), (1, 2), (3, 4), (4, 0), (2, 2)]
    got, want = device_and_host(E, K, pairs, shape)
    assert torch.equal(got, want), (shape, got.tolist(), want.tolist())
    assert 0 < int(want.sum()) and int(want.max()) <= shape[0] * shape[1]


def test_device_equals_host_on_one_256x256_pair():
    E, K = cameras(2, 32, 0.4)
    got, want = device_and_host(E, K, [(0, 1)], (256, 256))
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert 0 < int(want.min()) and int(want.max()) < 256 * 256            # partly overlapping: the count is not a trivial one


def test_device_equals_host_on_300_pairs_with_repeats():
    E, K = cameras(9, 33, 0.5)
    g = torch.Generator().manual_seed(34)
    pairs = torch.randint(0, 9, (300, 2), generator=g)
    pairs[7] = pairs[3]
    pairs[11] = torch.tensor([4, 4])
    assert (pairs[:, 0] == pairs[:, 1]).sum() >= 2
    got, want = device_and_host(E, K, pairs, (16, 16))
    assert torch.equal(got, want), (got - want).nonzero().tolist()
    assert torch.equal(got[7], got[3]) and got[11].tolist() == [256, 256]
    assert len(set(got.reshape(-1).tolist())) > 20                        # many different counts, not one value


def test_device_equals_host_with_a_single_view():
    E, K = cameras(1, 35)
    got, want = device_and_host(E, K, [(0, 0), (0, 0)], (9, 11))
    assert torch.equal(got, want) and got.tolist() == [[99, 99], [99, 99]]


def test_same_scratch_twice_and_pairs_outside_the_views():
    """gsr_view_overlap directly: two calls on ONE scratch and ONE counts buffer give the same counts (the prologue re-arms them), and
    a pair that names a view outside [0, V) gets -1, -1 while its neighbours keep their counts"""
    lib = _lib.load()
    E, K = cameras(4, 36)
    Ed, Kd = E.to(DEV), K.to(DEV)
    good = torch.tensor([[0, 1], [1, 2], [2, 3], [3, 0], [1, 3]], dtype=torch.int32)
    want, _ = vw.view_overlap(E, K, good, (12, 20))
    bad = good.clone()
    bad[1] = torch.tensor([1, 4])
    bad[3] = torch.tensor([-1, 0])
    scratch = torch.empty(lib.gsr_view_overlap_scratch_bytes(4, 5) // 8, dtype=torch.float64, device=DEV)
    counts = torch.full((5, 2), 12345, dtype=torch.int32, device=DEV)
    stream = vw._stream(DEV)

    def run(pairs):
        p = pairs.to(DEV)
        _lib.check(lib.gsr_view_overlap(Ed.data_ptr(), Kd.data_ptr(), 4, p.data_ptr(), 5, 12, 20, scratch.data_ptr(), scratch.numel() * 8,
                                        counts.data_ptr(), stream), "gsr_view_overlap")
        return counts.cpu()
    first = run(good)
    assert torch.equal(first, want)
    assert torch.equal(run(good), first)                                   # not doubled: the counters were re-armed
    marked = run(bad)
    assert marked[1].tolist() == [-1, -1] and marked[3].tolist() == [-1, -1]
    assert torch.equal(marked[[0, 2, 4]], want[[0, 2, 4]])
    assert torch.equal(run(good), first)
    assert torch.equal(vw.view_overlap_device(Ed, Kd, bad.to(DEV), (12, 20)).cpu(), marked)


def test_restatement_on_the_device_equals_the_host_at_360x640():
    """the float64 torch restatement gives the same counts wherever it runs: its fp32 pixel coordinates are formed on the host, since
    the device's own fp32 division is not correctly rounded and W = 640 is no power of two (at 256 the quotients are exact)"""
    E, K = cameras(3, 37, 0.4)
    pairs = torch.tensor([[0, 1], [2, 0]])
    host = vw.overlap_counts_torch(E, K, pairs, (360, 640))
    assert torch.equal(vw.overlap_counts_torch(E.to(DEV), K.to(DEV), pairs, (360, 640)).cpu(), host)
    assert torch.equal(vw.view_overlap_device(E.to(DEV), K.to(DEV), pairs.to(DEV, torch.int32), (360, 640)).cpu(), host)
    assert 0 < int(host.min()) and int(host.max()) < 360 * 640
    for on_device, on_host in zip(vw.pixel_coordinates(360, 640, DEV), vw.pixel_coordinates(360, 640, "cpu")):
        assert torch.equal(on_device.cpu().view(torch.int64), on_host.view(torch.int64))    # the coordinates themselves, bit for bit
    assert torch.equal(vw.overlap_ratio(host.to(DEV), (360, 640)).cpu().view(torch.int32),
                       (host.to(torch.float32) / float(360 * 640)).view(torch.int32))       # the CPU's fp32 division rounds correctly


def test_index_generator_with_device_cameras_reproduces_the_recorded_entries():
    check_index(DEV)

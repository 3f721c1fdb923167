"""CPU tests of the composite backward's LDS reduction (gsr_common.h wave_reduce9_lds, DESIGN R17).

The depth-free K6 sums its nine per-splat partials over the wave through an LDS transpose: eight planes of 64 floats written by plain
stores, read back as two float4 per lane, three adds each, then the packed DPP row sums of the swap form.  Here: the generated gfx950
code of that instantiation (what the change is for: no swap, no scratch, the LDS and register budget of eight waves per SIMD, six DS
instructions and no vector-memory wait in the reduction), and a numpy restatement of the layout against plain sums."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from styl3r_amd import _lib

LDS_KERNEL = "_ZN3gsr15k_composite_bwdILb0ELb1EEE"      # k_composite_bwd<false, true>


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    src = Path(_lib.__file__).resolve().parent / "csrc" / "gsr_backward.hip"
    out = tmp_path_factory.mktemp("k6lds") / "gsr_backward.s"
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", str(src), "-o", str(out)], check=True, capture_output=True)
    return out.read_text()


def _body(text):
    start = re.search(rf"^{LDS_KERNEL}\w*:", text, flags=re.M)
    assert start, "the LDS instantiation of k_composite_bwd is not in gsr_backward.hip's code object"
    return text[start.start():text.index(".Lfunc_end", start.start())]


def _metadata(text):
    """the kernel's entry in the code object's metadata (amdhsa.kernels)"""
    entries = [e for e in text[text.index("amdhsa.kernels:"):].split("\n  - ") if re.search(rf"^\s*\.name:\s+{LDS_KERNEL}\w*$", e, flags=re.M)]
    assert len(entries) == 1, len(entries)
    return entries[0]


def test_lds_instantiation_has_no_swap_no_scratch_and_the_budget_of_eight_waves(asm):
    body = _body(asm)
    assert "v_permlane" not in body
    assert "scratch_" not in body
    meta = _metadata(asm)
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1)) == 5120        # 3 072 (entry records) + 2 048 (eight planes)
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64                          # 512 / 64: eight waves per SIMD


def test_reduction_is_six_ds_instructions_and_waits_for_no_vector_memory(asm):
    """between the evaluation (its last v_exp_f32 in program order) and the gradient atomic: the eight stores, the two 16-byte loads, and no
    s_waitcnt vmcnt(0) -- that would wait for every gradient atomic the wave still has in flight"""
    body = _body(asm)
    atomics = [m.start() for m in re.finditer(r"global_atomic_add_f32", body)]
    assert len(atomics) == 1, len(atomics)
    evals = [m.start() for m in re.finditer(r"v_exp_f32", body[:atomics[0]])]
    assert evals
    red = body[evals[-1]:atomics[0]]
    assert len(re.findall(r"\bds_read_b128\b", red)) == 2
    assert len(re.findall(r"\bds_read", red)) == 2
    dwords = {"ds_write_b32": 1, "ds_write2_b32": 2, "ds_write2st64_b32": 2, "ds_write_b64": 2, "ds_write2_b64": 4, "ds_write2st64_b64": 4,
              "ds_write_b96": 3, "ds_write_b128": 4}
    writes = re.findall(r"\b(ds_write\w*)", red)
    assert writes and sum(dwords[w] for w in writes) <= 8, writes
    assert not re.search(r"s_waitcnt[^\n]*vmcnt\(0\)", red)
    assert "s_barrier" not in red


# ---- the layout, restated ----
def _slot_lds(lane):
    r, s = lane >> 4, lane & 15
    return r if s == 0 else (4 + r if s == 8 else (8 if lane == 63 else -1))


def _row_sum(x):
    """what rows_packed_sum leaves of a row-level register: every 16-lane row summed"""
    return x.reshape(4, 16).sum(1)


def _reduce9_lds_model(v):
    """v: (9, 64) values per lane -> {lane: total} as wave_reduce9_lds leaves them"""
    red = np.zeros(8 * 64, v.dtype)
    for i in range(8):
        red[i * 64:(i + 1) * 64] = v[i]                       # lane l stores red[i][l]
    f4 = red.reshape(128, 4)
    x = f4[0:64].sum(1)                                       # lane l: float4 #l
    y = f4[64:128].sum(1)                                     # lane l: float4 #(64 + l)
    xs, ys = _row_sum(x), _row_sum(y)
    out = {}
    for r in range(4):
        out[16 * r] = xs[r]                                   # bank 0 of row r
        out[16 * r + 8] = ys[r]                               # bank 2 of row r
    out[63] = v[8].sum()
    return out


def test_numpy_model_of_the_layout_gives_the_plain_sums():
    rng = np.random.default_rng(17)
    v = rng.integers(-1000, 1000, size=(9, 64)).astype(np.float64)
    got = _reduce9_lds_model(v)
    lanes = [l for l in range(64) if _slot_lds(l) >= 0]
    assert sorted(got) == lanes and sorted(_slot_lds(l) for l in lanes) == list(range(9))
    for l in lanes:
        assert got[l] == v[_slot_lds(l)].sum(), l
    # float4 #l holds value l >> 4 of lanes 4 (l & 15) .. + 3
    idx = np.arange(8 * 64).reshape(128, 4)
    for l in range(64):
        assert (idx[l] // 64 == l >> 4).all() and (idx[l] % 64 == 4 * (l & 15) + np.arange(4)).all()
        assert (idx[64 + l] // 64 == 4 + (l >> 4)).all() and (idx[64 + l] % 64 == 4 * (l & 15) + np.arange(4)).all()


def test_flag_and_exports_are_declared():
    header = (Path(__file__).resolve().parents[1] / "include/gsr.h").read_text()
    assert f"#define GSR_FLAG_K6_SWAP_SUM {_lib.GSR_FLAG_K6_SWAP_SUM} " in header and _lib.GSR_FLAG_K6_SWAP_SUM == 64
    used = [_lib.GSR_FLAG_NTOUCHED, _lib.GSR_FLAG_COV9, _lib.GSR_FLAG_PHASE_BIN, _lib.GSR_FLAG_PHASE_RENDER, _lib.GSR_FLAG_PREZERO_GRADS,
            _lib.GSR_FLAG_BIN_BALLOT, 3 << _lib.GSR_FLAG_SORT_KEYS_SHIFT, 7 << _lib.GSR_FLAG_SEG_SHIFT, 7 << _lib.GSR_FLAG_STYLES_CHUNK_SHIFT]
    assert all(not (_lib.GSR_FLAG_K6_SWAP_SUM & u) for u in used)
    assert "gsr_k6_blocks_per_cu" in _lib.EXPORTS and "gsr_test_reduce9" in _lib.EXPORTS

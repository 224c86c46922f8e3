"""CPU: the uniform-drive path of the register-resident split-operator kernels (profiles/uniform_drive.md).

  * The rule that lets a handle take k_split_reg_uni (ryd_desc_uniform: the function ryd_set_qubit_desc applies to its table)
    over hand-made descriptor tables: equal rows, every field off in turn, ``extra > 0``, a gauged handle.
  * The cross-compiled listings of the six new kernels - k_split_reg_uni and k_split_reg_seg_uni at <14, 5>, <13, 5> and
    <12, 4> - next to the general kernels of the same part unit: no scratch instruction in the stage loop, at most 256 vector
    registers, 4 barriers, the DPP moves of the general kernel (384 at <14, 5>, 192 at <12, 4>), ONE load of the coefficient
    record (s_load_dwordx8) and one touch of the next one where the general kernel has 2 N loads and 7 - 8 touches, the FMAs
    and roundings of the general kernel, N - 2 multiplications fewer (N - 1 of the cosine product, one more for Delta x n_t),
    none of its 8 - 9 additions, and at least 14 fewer v_cndmask.  The general kernels' own counts are pinned to what
    profiles/uniform_drive.md records for them (tests/test_split_reg_waits.py and tests/test_check_segments_host.py pin them
    to profiles/ychain.md as before).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from pulser_amd import _lib
from pulser_amd.terms import DESC_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- the rule ----
def _table(b, n):
    d = np.zeros((b, n), dtype=DESC_DTYPE)
    for q in range(b):  # every sequence its own series and scales, the same for all of its atoms
        d[q]["drive_series"], d[q]["det_series"], d[q]["off_series"] = 3 * q, 3 * q + 1, -1
        d[q]["drive_scale"], d[q]["det_scale"], d[q]["off_scale"] = 1.0 + 0.1 * q, 0.9 - 0.2 * q, 0.0
    return d


def _uniform(desc, gauged=0):
    lib = _lib.load()
    desc = np.ascontiguousarray(desc)
    out = C.c_int32(-1)
    _lib.check(lib.ryd_desc_uniform(desc.ctypes.data, desc.shape[0], desc.shape[1], gauged, C.byref(out)))
    return out.value


def test_equal_rows_are_uniform_whatever_the_sequences_do():
    assert _uniform(_table(3, 14)) == 1
    assert _uniform(_table(1, 12)) == 1
    d = _table(2, 13)
    d["drive_series"] = d["det_series"] = -1  # no drive and no detuning at all is uniform too
    assert _uniform(d) == 1


@pytest.mark.parametrize("field, value", [("drive_series", 7), ("det_series", 8), ("off_series", 2), ("drive_scale", 1.0 + 1e-15),
                                          ("det_scale", 0.9 * (1 + 1e-3)), ("off_scale", 1e-300)])
@pytest.mark.parametrize("where", [(0, 0), (2, 13), (1, 6)])
def test_one_field_of_one_atom_off_is_not_uniform(field, value, where):
    d = _table(3, 14)
    assert d[field][where] != value
    d[field][where] = value
    assert _uniform(d) == 0


def test_detuning_term_lists_and_gauged_handles_are_not_uniform():
    d = _table(3, 14)
    d["extra"][2, 9] = 1
    assert _uniform(d) == 0
    d = _table(3, 14)
    d["extra"][:] = 1  # every atom the SAME list: still the general path (the wave-per-atom coefficient launch sums them)
    assert _uniform(d) == 0
    assert _uniform(_table(3, 14), gauged=1) == 0
    assert _uniform(_table(3, 14), gauged=0) == 1


# ---- the compiled stage loops ----
KERNELS = {"general": r"_Z\d+k_split_regILi%dELi%dELb0ELb0ELb0ELb0E\w*", "general_seg": r"_Z\d+k_split_reg_segILi%dELi%dEE\w*",
           "uni": r"_Z\d+k_split_reg_uniILi%dELi%dEE\w*", "uni_seg": r"_Z\d+k_split_reg_seg_uniILi%dELi%dEE\w*"}
SHAPES = [(14, 5), (13, 5), (12, 4)]


def _stage_loop(text, name):
    """Counts of the stage loop of one kernel: the innermost loop that holds the four barriers of the LDS pass."""
    body = re.search(r"^(%s):(.*?)s_endpgm" % name, text, re.S | re.M).group(2).split("\n")
    best = None
    for hdr in [i for i, l in enumerate(body) if "Loop Header: Depth=" in l]:
        j = hdr
        while not re.match(r"\.LBB\d+_\d+:", body[j]):
            j -= 1
        lab = body[j].split(":")[0]
        backs = [i for i, l in enumerate(body) if i > j and re.search(r"s_c?branch\w*\s+%s\b" % re.escape(lab), l)]
        if backs and sum("s_barrier" in l for l in body[j:backs[-1] + 1]) >= 4 and (best is None or backs[-1] - j < best[1] - best[0]):
            best = (j, backs[-1])
    assert best, "no loop with the barriers of the LDS pass"
    reg = body[best[0]:best[1] + 1]
    c = lambda pat: sum(1 for l in reg if re.search(pat, l))
    meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % name, text, re.S).group(1)
    return {"valu": sum(1 for l in reg if re.match(r"\s+v_", l)), "fma": c(r"\sv_fmac?_f64"), "mul": c(r"\sv_mul_f64"), "add": c(r"\sv_add_f64"),
            "rndne": c(r"v_rndne_f64"), "dpp": c(r"v_mov_b32_dpp"), "cndmask": c(r"v_cndmask"), "load_x8": c(r"s_load_dwordx8"),
            "load_x4": c(r"s_load_dwordx4"), "load_x2": c(r"s_load_dwordx2\b"), "load_x1": c(r"s_load_dword\s"), "barriers": c("s_barrier"),
            "scratch": c("scratch_"), "vgpr": int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))}


@pytest.fixture(scope="module")
def listings():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "pulser_amd", "csrc", "rydemu_splitreg.hip")

    def counts(shape):
        n, nr = shape
        with tempfile.TemporaryDirectory() as d:
            asm = os.path.join(d, "r.s")
            subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                            "-Wno-unused-function", f"-DRYD_SPLITR_N={n}", src, "-o", asm], check=True, stderr=subprocess.DEVNULL, timeout=1200)
            text = open(asm).read()
        return {k: _stage_loop(text, pat % (n, nr)) for k, pat in KERNELS.items()}

    with ThreadPoolExecutor(3) as pool:
        return dict(zip(SHAPES, pool.map(counts, SHAPES)))


def _recorded(n, nr, kernel):
    """(valu, fma, mul, add, rndne, dpp, cndmask) of a row of the table of profiles/uniform_drive.md."""
    text = open(os.path.join(ROOT, "profiles", "uniform_drive.md")).read()
    m = re.search(r"^\| `<%d, %d>` \| `%s` \| (\d+) \| (\d+) / (\d+) / (\d+) / (\d+) \| (\d+) \| (\d+) \|" % (n, nr, kernel), text, re.M)
    assert m, f"profiles/uniform_drive.md: no row for {kernel}<{n}, {nr}>"
    return tuple(int(g) for g in m.groups())


@pytest.mark.parametrize("seg", [False, True])
@pytest.mark.parametrize("n, nr", SHAPES)
def test_the_uniform_stage_loop_is_the_general_one_minus_the_per_atom_work(listings, n, nr, seg):
    gen, uni = listings[(n, nr)]["general_seg" if seg else "general"], listings[(n, nr)]["uni_seg" if seg else "uni"]
    print(f"<{n}, {nr}>{' seg' if seg else ''}: general {gen}\n{' ' * 12}uniform {uni}")
    assert uni["scratch"] == 0 and uni["barriers"] == 4 and uni["vgpr"] <= 256
    assert uni["dpp"] == gen["dpp"] and (uni["dpp"] == {14: 384, 12: 192}[n] if n != 13 else True)
    # one load of the 32-byte record, one touch of the next one - and nothing else from the scalar cache
    assert (uni["load_x8"], uni["load_x4"], uni["load_x2"], uni["load_x1"]) == (1, 0, 0, 1)
    assert gen["load_x4"] == n and gen["load_x2"] == n  # (the general kernel: (C, T) and Delta of every atom)
    assert uni["fma"] == gen["fma"] and uni["rndne"] == gen["rndne"]
    assert gen["mul"] - uni["mul"] == n - 2
    assert uni["add"] == 0 and gen["add"] in (8, 9)
    assert gen["cndmask"] - uni["cndmask"] >= 14
    assert uni["valu"] < gen["valu"]
    # ... by the amounts the note records, and the general kernels where the note has them
    keys = ("valu", "fma", "mul", "add", "rndne", "dpp", "cndmask")
    assert tuple(gen[k] for k in keys) == _recorded(n, nr, "k_split_reg_seg" if seg else "k_split_reg")
    assert tuple(uni[k] for k in keys) == _recorded(n, nr, "k_split_reg_seg_uni" if seg else "k_split_reg_uni")


def test_the_general_kernel_of_the_headline_counts_what_it_counted(listings):
    g = listings[(14, 5)]["general"]
    assert (g["valu"], g["fma"], g["mul"], g["add"], g["rndne"], g["dpp"], g["cndmask"]) == (1903, 1162, 241, 9, 7, 384, 34)
    assert g["load_x4"] + g["load_x2"] + g["load_x1"] == 36 and g["scratch"] == 0 and g["vgpr"] <= 256

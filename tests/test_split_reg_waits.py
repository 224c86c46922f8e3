"""CPU: where the stage loop of k_split_reg waits for memory (SPLITR_KWARM, SPLITR_GAHEAD; profiles/stage_waits.md), read off
the cross-compiled listing by tools/stage_waits.py - one compilation per shape, <14, 5> and <12, 4>:

  (a) between the last warm-up load of the next stage's coefficient record and the first following s_waitcnt that names
      lgkmcnt lie at least 200 vector instructions (one chunk's rotations alone are 112 FMAs + 96 moves at <14, 5>; with the
      loads folded on the spot there were 2);
  (b) every read of the G table (the 2^NR ds_read_b128 on one address register) has at least 32 fp64 instructions between
      itself and the wait that releases its value (a group's phase work and rotations are ~80; read just in time: 4 - 8);
  (c) nothing else moved: the fp64 instructions, DPP moves and swaps profiles/ychain.md records, 4 barriers, no scratch, at
      most 256 vector registers.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SHAPES = [(14, 5), (12, 4)]
COLS = ("warm_loads", "warm_kind", "warm_valu", "g_reads", "g_min", "g_median", "g_max", "trig_reads", "trig_min", "fma", "mul", "add",
        "rndne", "dpp", "swap", "barriers", "scratch", "vgpr")


@pytest.fixture(scope="module")
def tables():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")

    def table(shape):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stage_waits.py"), str(shape[0]), str(shape[1])],
                             check=True, capture_output=True, text=True, timeout=900).stdout
        row = [l for l in out.splitlines() if re.match(r"^\| \d+ \|", l)][0]
        cells = dict(zip(COLS, (c.strip() for c in row.strip("|").split("|"))))
        per_read = [l for l in out.splitlines() if l.startswith("G(r) by register r:")][0].split(":", 1)[1].split()
        cells["g"] = {int(a.split(":")[0]): int(a.split(":")[1]) for a in per_read}
        return cells

    with ThreadPoolExecutor(2) as pool:
        return dict(zip(SHAPES, pool.map(table, SHAPES)))


def _recorded(n, nr):
    """fp64 / DPP / swap counts of the default row of profiles/ychain.md: (fma, mul, add, rndne, dpp, swaps)."""
    text = open(os.path.join(ROOT, "profiles", "ychain.md")).read()
    m = re.search(r"^\| `<%d, %d>` \| \d \(default\) \| (\d+) \| (\d+) / (\d+) / (\d+) / (\d+) \| [\d.]+ \| (\d+) \|" % (n, nr), text, re.M)
    assert m, f"profiles/ychain.md: no default row for <{n}, {nr}>"
    dpp, fma, mul, add, rnd, swaps = (int(g) for g in m.groups())
    return fma, mul, add, rnd, dpp, swaps


@pytest.mark.parametrize("n, nr", SHAPES)
def test_the_warm_up_is_not_waited_for_where_it_is_issued(tables, n, nr):
    t = tables[(n, nr)]
    print(f"<{n}, {nr}>: {t['warm_loads']} x {t['warm_kind']}, {t['warm_valu']} vector instructions to the next lgkmcnt wait")
    assert int(t["warm_loads"]) >= n * 32 // 64  # one touch per 64-byte line of the record (4 doubles per atom)
    assert t["warm_kind"] == "s_load_dword"  # plain scalar loads, as before
    assert int(t["warm_valu"]) >= 200, t


@pytest.mark.parametrize("n, nr", SHAPES)
def test_every_g_value_is_read_a_group_ahead(tables, n, nr):
    t = tables[(n, nr)]
    print(f"<{n}, {nr}>: fp64 instructions between a G read and its wait: {t['g']}")
    assert sorted(t["g"]) == list(range(1 << nr))  # the 2^NR reads, offsets 16 k on one address register
    assert min(t["g"].values()) >= 32, t["g"]


@pytest.mark.parametrize("n, nr", SHAPES)
def test_the_work_of_a_stage_is_what_it_was(tables, n, nr):
    t = tables[(n, nr)]
    got = tuple(int(t[k]) for k in ("fma", "mul", "add", "rndne", "dpp", "swap"))
    print(f"<{n}, {nr}>: fma / mul / add / rndne / dpp / swaps {got}, barriers {t['barriers']}, scratch {t['scratch']}, vgpr {t['vgpr']}")
    assert got == _recorded(n, nr), (got, _recorded(n, nr))
    assert int(t["barriers"]) == 4 and int(t["scratch"]) == 0
    assert int(t["vgpr"]) <= 256

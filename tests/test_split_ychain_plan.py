"""CPU: the y chain of k_split_reg (SPLITR_YCHAIN; pulser_amd/csrc/split_ychain.hpp, profiles/ychain.md).

For a real drive only the imaginary parts travel over the DPP crossbar, as a chain of hops from one lane direction to the
next.  The hop plan is data, replayed at compile time as permutations of the 16 lanes of a row; here
  * a translation unit that includes the header compiles (its static_asserts are the proof of the plans), and the checker
    names the rule a broken plan breaks (bits in the wrong order, a pattern that is none of the six involutions, a final
    shift the store does not expect, a plan that saves nothing);
  * the compiled stage loops of <14, 5> and <12, 4> hold fewer v_mov_b32_dpp than the partner fetches took (512 / 256), exactly
    what profiles/ychain.md records for the default of the switch, no scratch, and the fp64 work bench.py's roofline uses;
  * tools/lane_layout_check.py replays the bank rules of the pass, the split 8-byte stores included.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pulser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PARENT_DPP = {(14, 5): 512, (12, 4): 256}  # the partner fetches: 4 moves per amplitude and DPP bit

CHECKS = r"""
#include "split_ychain.hpp"
// the shipped plans are asserted by the header itself; the checker must also REFUSE broken ones, each by its own rule
struct WrongOrder {  // bit 3 and bit 2 rotated in each other's place: the shift before the third rotation is 8, not 7
  static constexpr int order[4] = {0, 1, 2, 3};
  static constexpr int dir[4] = {1, 2, 7, 8};
  static constexpr SplitYHop hops[5] = {{1, {0xB1, 0}}, {1, {0x1B, 0}}, {2, {0x4E, 0x128}}, {1, {0x140, 0}}, {1, {0x141, 0}}};
  static constexpr int final_shift = 0;
  static constexpr int fetch_moves = 16;
};
static_assert(splity_check<WrongOrder, 4>() == 2, "a plan whose shifts do not meet the directions must be refused");
struct WrongPattern : SplitYPlan<4, 0> {  // row_shr:1 is no involution
  static constexpr SplitYHop hops[5] = {{1, {0x111, 0}}, {1, {0x1B, 0}}, {2, {0x4E, 0x128}}, {1, {0x140, 0}}, {1, {0x141, 0}}};
};
static_assert(splity_check<WrongPattern, 4>() == 1, "a pattern outside the six involutions must be refused");
struct WrongHome : SplitYPlan<4, 0> {  // y left at shift 7 although the store expects it at home
  static constexpr SplitYHop hops[5] = {{1, {0xB1, 0}}, {1, {0x1B, 0}}, {2, {0x4E, 0x128}}, {1, {0x140, 0}}, {0, {0, 0}}};
};
static_assert(splity_check<WrongHome, 4>() == 3, "a final shift the store does not expect must be refused");
struct NoGain : SplitYPlan<4, 0> {  // xor 1 as xor 2 after xor 3, home as xor 15 after xor 8: sound, but 16 moves
  static constexpr SplitYHop hops[5] = {{2, {0x1B, 0x4E}}, {1, {0x1B, 0}}, {2, {0x4E, 0x128}}, {1, {0x140, 0}}, {2, {0x128, 0x140}}};
};
static_assert(splity_check<NoGain, 4>() == 5, "a plan that saves no moves must be refused");
struct TwiceTheSameBit : SplitYPlan<2, 0> {
  static constexpr int order[2] = {0, 0};
};
static_assert(splity_check<TwiceTheSameBit, 2>() == 4, "every DPP bit is rotated exactly once");
int main() { return 0; }
"""


def test_the_hop_plans_are_proven_at_compile_time_and_broken_plans_are_refused():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "ychain_checks.hip")
        with open(src, "w") as f:
            f.write(CHECKS)
        res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, src],
                             capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]


def test_the_kernel_takes_its_hops_from_the_table_alone():
    """Inside chain_step every DPP move is splitr_dpp<h.ctrl[..]> of a table entry: no literal control word, no
    splitr_partner."""
    text = open(os.path.join(CSRC, "k_split_reg.hpp")).read()
    m = re.search(r"auto chain_step = \[&\]\(auto Cc, auto Ic\) \{(.*?)\n    \};\n", text, re.S)
    assert m, "chain_step"
    body = m.group(1)
    assert "SplitYPlan<ND" in body and "splitr_partner" not in body
    assert set(re.findall(r"splitr_dpp<([^>]*)>", body)) == {"h.ctrl[0]", "h.ctrl[1]"}


def _default_switch():
    text = open(os.path.join(CSRC, "k_split_reg.hpp")).read()
    return int(re.search(r"#ifndef SPLITR_YCHAIN\n#define SPLITR_YCHAIN (\d)\n", text).group(1))


def _recorded(n, nr):
    """The ISA row profiles/ychain.md records for the default of the switch: (switch value, v_mov_b32_dpp)."""
    text = open(os.path.join(ROOT, "profiles", "ychain.md")).read()
    m = re.search(r"^\| `<%d, %d>` \| (\d) \(default\) \| (\d+) \|" % (n, nr), text, re.M)
    assert m, f"profiles/ychain.md: no default row for <{n}, {nr}>"
    return int(m.group(1)), int(m.group(2))


@pytest.fixture(scope="module")
def isa_rows():
    """tools/count_isa.py on both shapes, the two compilations side by side."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")

    def count(shape):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_isa.py"), "splitreg", str(shape[0]), str(shape[1])],
                             check=True, capture_output=True, text=True, timeout=900).stdout
        row = [l for l in out.splitlines() if re.match(r"^\| \d+ \|", l)][0]
        return [c.strip() for c in row.strip("|").split("|")]

    with ThreadPoolExecutor(2) as pool:
        return dict(zip(PARENT_DPP, pool.map(count, PARENT_DPP)))


@pytest.mark.parametrize("n, nr", list(PARENT_DPP))
def test_stage_loop_moves_fewer_dwords_over_the_crossbar_for_the_same_fp64_work(isa_rows, n, nr):
    cells = isa_rows[(n, nr)]
    dpp, scratch, flops = int(cells[4]), int(cells[8]), float(cells[10])
    switch, recorded = _recorded(n, nr)
    print(f"<{n}, {nr}>: v_mov_b32_dpp {dpp} (partner fetches: {PARENT_DPP[(n, nr)]}), scratch {scratch}, flops / amplitude / stage {flops}")
    assert switch == _default_switch()
    assert dpp < PARENT_DPP[(n, nr)] and dpp == recorded, cells
    assert scratch == 0, cells
    # the fp64 work is what it was: the constants of bench.py's roofline (pinned to the ISA by tests/test_host_logic.py)
    src = open(os.path.join(ROOT, "bench.py")).read()
    ns = {}
    exec(re.search(r"^KSPLITREG_FLOPS_PER_AMP_STAGE = .*$", src, re.M).group(0), ns)
    exec(re.search(r"^KSPLITREG_SHAPES = .*?\n\n", src, re.M | re.S).group(0), ns)
    want = ns["KSPLITREG_FLOPS_PER_AMP_STAGE"] if n == 14 else ns["KSPLITREG_SHAPES"][12][1]
    assert abs(flops - want) < 0.005, (flops, want)
    assert int(cells[9]) == 4  # barriers per stage


def test_bank_rules_of_the_pass_with_the_split_stores():
    """The 16-byte stores and loads of the pass and of the transposition stay conflict-free (exit status); the split 8-byte
    stores of SPLITR_YCHAIN 2 are 2-way by the rule for ds_write_b64 (16 lanes on 16-byte slots meet every bank pair twice),
    x and y alike - the figure profiles/ychain.md sets against the measured counter."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lane_layout_check.py")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-2000:]
    split = [l for l in res.stdout.splitlines() if "SPLITR_YCHAIN 2" in l]
    assert len(split) == 2 * 5 and all("8 cycles (conflict-free 4)" in l for l in split), split

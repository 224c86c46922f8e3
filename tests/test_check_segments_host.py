"""CPU: the segments of a split-operator run (SplitRun.nseg, split_types.hpp; profiles/check_segments.md).

  * A Python restatement of the stage numbering and the E0 weights: for random cuts of a run into up to three segments,
    compositions of 10 and 6 stages mixed by `alt` flags, every segment's (sub-step, stage, weight) list and the place of its
    records equal those of the same sub-steps described as a run of their own (split_types.hpp asserts the same on one
    case at compile time).
  * The cross-compiled listing of k_split_reg_seg<14, 5> and <12, 4>: the stage loop - now inside the segment loop - holds
    the fp64 instructions, DPP moves and swaps profiles/ychain.md records for the plain kernel (what
    tests/test_split_reg_waits.py pins for k_split_reg itself), 4 barriers, no scratch instruction, and the kernel stays
    within 256 vector registers.
"""
from __future__ import annotations

import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- split_types.hpp, restated ----
class Run:
    def __init__(self, S, S2, a, a2, tau, alt, seg_end=()):
        self.S, self.S2, self.a, self.a2, self.tau, self.alt = S, S2, a, a2, list(tau), list(alt)
        self.nsub = len(self.tau)
        self.first = np.concatenate([[0], np.cumsum([S2 if f else S for f in self.alt])]).astype(int)
        self.seg_end = list(seg_end)  # empty: one closed run

    def S_of(self, s):
        return self.S2 if self.alt[s] else self.S

    def a_of(self, s, i):
        return (self.a2 if self.alt[s] else self.a)[i]

    def seg(self, q):
        if not self.seg_end:
            return 0, self.nsub, 0
        s0 = self.seg_end[q - 1] if q else 0
        return s0, self.seg_end[q], int(self.first[s0]) + q

    def nseg(self):
        return max(1, len(self.seg_end))

    def records(self):
        return int(self.first[self.nsub]) + self.nseg()

    def seg_of(self, rec):
        q = 0
        while q + 1 < len(self.seg_end) and rec >= int(self.first[self.seg_end[q]]) + q + 1:
            q += 1
        return q

    def locate(self, j):
        s = int(np.searchsorted(self.first, j, side="right")) - 1
        return s, j - int(self.first[s])

    def stage_list(self, q):
        """[(sub-step relative to the segment's first, stage, weight)] of segment q, the closing D last"""
        s0, s1, _ = self.seg(q)
        total = int(self.first[s1] - self.first[s0])
        out = []
        for jl in range(total):
            s, st = self.locate(int(self.first[s0]) + jl)
            w = self.a_of(s, st) * self.tau[s]
            if st == 0 and s > s0:
                w += self.a_of(s - 1, self.S_of(s - 1)) * self.tau[s - 1]
            out.append((s - s0, st, w))
        out.append((s1 - 1 - s0, self.S_of(s1 - 1), self.a_of(s1 - 1, self.S_of(s1 - 1)) * self.tau[s1 - 1]))
        return out


@pytest.mark.parametrize("seed", range(40))
def test_every_segment_is_the_same_sub_steps_as_a_run_of_their_own(seed):
    rng = np.random.default_rng(seed)
    a, a2 = rng.uniform(-0.3, 0.5, 11), rng.uniform(-0.3, 0.5, 7)
    nsub = int(rng.integers(3, 30))
    tau = rng.uniform(1e-4, 1e-2, nsub)
    alt = rng.integers(0, 2, nsub) if seed % 4 else np.full(nsub, seed // 4 % 2)  # (every fourth: one composition only)
    nseg = 1 + seed % 3
    ends = sorted(rng.choice(np.arange(1, nsub), nseg - 1, replace=False).tolist()) + [nsub]
    R = Run(10, 6, a, a2, tau, alt, ends)
    assert R.records() == int(R.first[nsub]) + nseg
    rec = 0
    for q in range(nseg):
        s0, s1, rec0 = R.seg(q)
        own = Run(10, 6, a, a2, tau[s0:s1], alt[s0:s1])
        mine, theirs = R.stage_list(q), own.stage_list(0)
        assert rec0 == rec and len(mine) == own.records()
        assert mine == theirs  # sub-step, stage AND the weight, bit for bit: the same products in the same order
        assert all(R.seg_of(rec + j) == q for j in range(len(mine)))
        # a sub-step at the head of a segment carries no D of the one before it
        assert mine[0][2] == R.a_of(s0, 0) * tau[s0]
        rec += len(mine)
    assert rec == R.records()
    # ... and n_applications counts n_stages - 1 of every closed segment: the stages of the compositions, whatever the cut
    assert sum(len(R.stage_list(q)) - 1 for q in range(nseg)) == int(R.first[nsub])


# ---- the compiled stage loop of the segment kernel ----
def _recorded(n, nr):
    """fp64 / DPP / swap counts of the default row of profiles/ychain.md: (fma, mul, add, rndne, dpp, swaps)."""
    text = open(os.path.join(ROOT, "profiles", "ychain.md")).read()
    m = re.search(r"^\| `<%d, %d>` \| \d \(default\) \| (\d+) \| (\d+) / (\d+) / (\d+) / (\d+) \| [\d.]+ \| (\d+) \|" % (n, nr), text, re.M)
    assert m, f"profiles/ychain.md: no default row for <{n}, {nr}>"
    dpp, fma, mul, add, rnd, swaps = (int(g) for g in m.groups())
    return fma, mul, add, rnd, dpp, swaps


def _seg_stage_loop(n, nr):
    """(lines of the stage loop of k_split_reg_seg<n, nr>, vector registers of the kernel): the loop is the innermost one
    that holds the four barriers of the LDS pass (counting as tools/count_isa.py does for the plain kernel, where the stage
    loop is the longest loop of depth 1; here it sits inside the segment loop)."""
    src = os.path.join(ROOT, "pulser_amd", "csrc", "rydemu_splitreg.hip")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "r.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                        "-Wno-unused-function", f"-DRYD_SPLITR_N={n}", src, "-o", asm], check=True, stderr=subprocess.DEVNULL, timeout=900)
        text = open(asm).read()
    name = r"_Z\d+k_split_reg_segILi%dELi%dEE\w*" % (n, nr)
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
    meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % name, text, re.S).group(1)
    return body[best[0]:best[1] + 1], int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))


@pytest.fixture(scope="module")
def loops():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    shapes = [(14, 5), (12, 4)]
    with ThreadPoolExecutor(2) as pool:
        return dict(zip(shapes, pool.map(lambda s: _seg_stage_loop(*s), shapes)))


@pytest.mark.parametrize("n, nr", [(14, 5), (12, 4)])
def test_the_stage_loop_of_the_segment_kernel_is_the_plain_one(loops, n, nr):
    reg, vgpr = loops[(n, nr)]
    c = lambda pat: sum(1 for l in reg if re.search(pat, l))
    got = (c(r"\sv_fmac?_f64"), c(r"\sv_mul_f64"), c(r"\sv_add_f64"), c(r"v_rndne_f64"), c(r"v_mov_b32_dpp"), c(r"v_permlane\d+_swap"))
    print(f"k_split_reg_seg<{n}, {nr}>: fma / mul / add / rndne / dpp / swaps {got}, barriers {c('s_barrier')}, scratch {c('scratch_')}, vgpr {vgpr}")
    assert got == _recorded(n, nr), (got, _recorded(n, nr))
    assert c("s_barrier") == 4 and c("scratch_") == 0
    assert vgpr <= 256

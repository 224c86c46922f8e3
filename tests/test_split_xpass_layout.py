"""CPU: the layout convention of SPLITR_XPASS (pulser_amd/csrc/k_split_reg.hpp, profiles/xpass.md), replayed in Python for
<14, 5> and <12, 4>.

In these kernels lane bits 4, 5 change places with the two T register bits inside the LDS pass: a register NAMED with T bits
(s0, s1) holds, on a lane with bits (l4, l5), the amplitude whose T-position index bits are (s0 ^ l4, s1 ^ l5), and reader lane
l fills its registers named (s0, s1) from the registers of the same name of lane l ^ (s0 << 4 | s1 << 5).  Here

  * index_x(odd, t, r) - SplitRegLayout::index_x restated - is a bijection onto the 2^N amplitudes for both parities;
  * one pass with the chunk XORs maps the even layout onto the odd one, and a second one maps it back;
  * the bookkeeping of the phase factors in named bits (et', ev', the selects of the lane's detuning sum, the sign of Dr, the
    four permuted copies of the G table) gives E0(index) minus the detuning sum of the excited atoms for every lane and
    register, on a random pairwise-additive E0;
  * the compiled stage loops hold no v_permlane*_swap at the fp64 counts they had (tools/count_isa.py).
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SHAPES = [(14, 5), (12, 4)]
FP64 = {(14, 5): (1162, 241, 9, 7), (12, 4): (543, 138, 8, 6)}  # fma, mul, add, rndne of the stage loop before the change


class Layout:
    """SplitRegLayout<N, NR> (positions of the index bits at the start of an even / odd stage)."""

    def __init__(self, n, nr):
        self.n, self.nr = n, nr
        self.nw = n - 6 - nr
        self.ntb = nr - self.nw
        self.nd = 6 - self.ntb
        assert self.ntb == 2 and self.nw > 0
        self.nt, self.na = 64 << self.nw, 1 << nr

    def regbit(self, odd, j):
        if not odd:
            return 6 + self.nw + j
        return 6 + j if j < self.nw else self.nd + (j - self.nw)

    def lanebit(self, odd, j):
        return j if (j < self.nd or not odd) else 6 + 2 * self.nw + (j - self.nd)

    def wavebit(self, odd, j):
        return 6 + self.nw + j if odd else 6 + j

    def index(self, odd, t, r):
        i = 0
        for j in range(6):
            i |= ((t >> j) & 1) << self.lanebit(odd, j)
        for j in range(self.nw):
            i |= ((t >> (6 + j)) & 1) << self.wavebit(odd, j)
        for j in range(self.nr):
            i |= ((r >> j) & 1) << self.regbit(odd, j)
        return i

    def index_x(self, odd, t, r):
        i = self.index(odd, t, r)
        for m in range(self.ntb):
            i ^= ((t >> (self.nd + m)) & 1) << self.regbit(odd, self.nw + m)
        return i

    def held(self, odd):
        """[t][r] -> the amplitude a register holds under the convention"""
        return np.array([[self.index_x(odd, t, r) for r in range(self.na)] for t in range(self.nt)])

    def the_pass(self, old):
        """The LDS pass: writer slot (lane, A = wave, B = pass bits, chunk); reader A = its pass bits, B = its wave, the lane of
        the chunk named (s0, s1) = l ^ (s0 << 4 | s1 << 5)."""
        nw, pw = self.nw, (1 << self.nw) - 1
        new = np.empty_like(old)
        for t in range(self.nt):
            l, w = t & 63, t >> 6
            for r in range(self.na):
                kp, c = r & pw, r >> nw
                src_t = (l ^ (c << self.nd)) | (kp << 6)
                new[t, r] = old[src_t, w | (c << nw)]
        return new


@pytest.mark.parametrize("n, nr", SHAPES)
def test_index_is_a_bijection_for_both_parities(n, nr):
    lay = Layout(n, nr)
    for odd in (False, True):
        held = lay.held(odd)
        assert sorted(held.ravel().tolist()) == list(range(1 << n))
        # chunk (0, 0) on a lane with l4 = l5 = 0 is the plain map
        assert all(lay.index_x(odd, t, r) == lay.index(odd, t, r) for t in range(0, lay.nt, 64) for r in range(lay.na))


@pytest.mark.parametrize("n, nr", SHAPES)
def test_one_pass_maps_the_even_layout_onto_the_odd_one_and_back(n, nr):
    lay = Layout(n, nr)
    even, odd = lay.held(False), lay.held(True)
    assert np.array_equal(lay.the_pass(even), odd)
    assert np.array_equal(lay.the_pass(odd), even)
    # without the chunk XORs the convention is NOT reproduced (the check can fail)
    plain = Layout(n, nr)
    plain.the_pass = lambda old: np.array([[old[(t & 63) | ((r & ((1 << lay.nw) - 1)) << 6), (t >> 6) | ((r >> lay.nw) << lay.nw)]
                                            for r in range(lay.na)] for t in range(lay.nt)])
    assert not np.array_equal(plain.the_pass(even), odd)


@pytest.mark.parametrize("n, nr", SHAPES)
@pytest.mark.parametrize("odd", [False, True])
def test_named_bit_bookkeeping_reproduces_the_phase_of_every_amplitude(n, nr, odd):
    lay = Layout(n, nr)
    nw, nd, na, nt = lay.nw, lay.nd, lay.na, lay.nt
    rng = np.random.default_rng(17 * n + odd)
    u = np.triu(rng.uniform(0.1, 3.0, (n, n)), 1)  # pair energies by index bit; an atom is excited where its bit is 0
    det = rng.uniform(-2.0, 2.0, n)                # detuning integrals by index bit
    w_e = 0.37

    def excited(i):
        return np.array([((i >> p) & 1) == 0 for p in range(n)])

    def e0(i):
        x = excited(i).astype(float)
        return float(x @ u @ x)

    e0_of = np.array([e0(i) for i in range(1 << n)])
    exact = lambda i: w_e * e0_of[i] - float(det[excited(i)].sum())
    # coefficients by POSITION, as the stage loads them
    d_l = [det[lay.lanebit(odd, j)] for j in range(6)]
    d_w = [det[lay.wavebit(odd, j)] for j in range(nw)]
    d_r = [det[lay.regbit(odd, j)] for j in range(nr)]
    # the uniform table in ACTUAL register bits, and its four permuted copies: copy c holds G[r ^ (c << NW)] at slot r
    g = np.array([e0_of[lay.index(odd, nt - 1, r)] for r in range(na)])
    copies = np.empty((4, na))
    for lane in range(64):  # the writers: lane & (NA - 1) holds G(lane & (NA - 1)); 64 / NA replicas share the four copies
        ra = lane & (na - 1)
        for cpy in ([lane >> 4] if na == 16 else [k | ((lane >> 5) << 1) for k in range(2)]):
            copies[cpy, ra ^ (cpy << nw)] = g[ra]
    worst = 0.0
    for t in range(nt):
        flip = [(t >> (nd + m)) & 1 for m in range(2)]
        # prologue: the pieces in actual bits (plain map), then the per-lane constants of the flipped T bits
        et = e0_of[lay.index(odd, t, na - 1)]
        ev = [e0_of[lay.index(odd, t, (na - 1) ^ (1 << j))] - et for j in range(nr)]
        for m in range(2):
            if flip[m]:
                et += ev[nw + m]
                ev[nw + m] = -ev[nw + m]
        # the lane's detuning sum: lane bits 4, 5 select between two scalars
        dthr = 0.0
        for j in range(6):
            bit = (t >> j) & 1
            if j >= nd:
                dthr += d_r[nw + j - nd] if bit else d_l[j]
            else:
                dthr += 0.0 if bit else d_l[j]
        for j in range(nw):
            dthr += 0.0 if (t >> (6 + j)) & 1 else d_w[j]
        b_arg = w_e * et - dthr
        f_arg = [w_e * ev[j] - (-d_r[j] if (j >= nw and flip[j - nw]) else d_r[j]) for j in range(nr)]
        cpy = (t >> nd) & 3
        for r in range(na):
            phi = b_arg + sum(f_arg[j] for j in range(nr) if not (r >> j) & 1) + w_e * copies[cpy, r]
            worst = max(worst, abs(phi - exact(lay.index_x(odd, t, r))))
    # sums of at most 14 + 91 terms of size <= 3: rounding alone
    assert worst < 1e-11, worst


@pytest.fixture(scope="module")
def isa_rows():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")

    def count(shape):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_isa.py"), "splitreg", str(shape[0]), str(shape[1])],
                             check=True, capture_output=True, text=True, timeout=900).stdout
        row = [l for l in out.splitlines() if re.match(r"^\| \d+ \|", l)][0]
        return [c.strip() for c in row.strip("|").split("|")]

    with ThreadPoolExecutor(2) as pool:
        return dict(zip(SHAPES, pool.map(count, SHAPES)))


@pytest.mark.parametrize("n, nr", SHAPES)
def test_compiled_stage_loop_has_no_swaps_at_unchanged_fp64_counts(isa_rows, n, nr):
    cells = isa_rows[(n, nr)]
    fp64, swaps, scratch, barriers = tuple(int(c) for c in cells[:4]), int(cells[5]), int(cells[8]), int(cells[9])
    print(f"<{n}, {nr}>: fma / mul / add / rndne {fp64}, swaps {swaps}, scratch {scratch}, barriers {barriers}")
    assert swaps == 0
    assert fp64 == FP64[(n, nr)]
    assert scratch == 0 and barriers == 4

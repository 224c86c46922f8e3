"""Extra detuning terms (``ryd_set_detuning_terms``) for the tests: device tables with term lists and the plain problems
that mean the same thing (tests/test_dterm_ref.py, tests/test_gpu_detuning_terms.py).

Plain NumPy / SciPy, no GPU and no ``HamiltonianData.device_tables``: the tables are ``lower(problems)`` with the series,
the term table and the ``extra`` indices added by hand.  A spline is linear in its samples, so atom k of problem b with
the list ``[(series, scale), ...]`` has the detuning of the problem whose ``det`` samples are
``det + sum scale * samples[series]`` - the *folded* problem, which the oracle can build and integrate.
"""
from __future__ import annotations

import copy
from dataclasses import replace

import numpy as np
from scipy.interpolate import CubicSpline

from pulser_amd.terms import DTERM_DTYPE, adapt_to_sampling_rate, lower

# the lengths every kernel family sums: below, at and above one wave (64 lanes), two waves and a tail
LENGTHS = (1, 2, 63, 64, 65, 130)
N_FREQ = 65          # noise frequencies: 65 x (cos, sin) = 130 series, so the longest list names each series once
SCALE_LO, SCALE_HI = 0.05, 0.5  # rad/us


def noise_series(duration, n_freq=N_FREQ, mhz=None):
    """``[2 n_freq, duration]``: m cos(w_f t), m sin(w_f t) on the 1-ns grid, w_f / 2 pi = 1 ... 40 MHz (or the
    frequencies ``mhz``), interleaved as the device lowering interleaves them; the slot mask m is zero on an eighth of
    the window (past its middle), so every series has two kinks the not-a-knot spline rings next to."""
    t_us = np.arange(duration) * 1e-3
    mask = np.ones(duration)
    mask[duration // 2:duration // 2 + max(2, duration // 8)] = 0.0
    freqs = np.linspace(1.0, 40.0, n_freq) if mhz is None else np.atleast_1d(np.asarray(mhz, dtype=float))
    out = np.empty((2 * len(freqs), duration))
    for f, fm in enumerate(freqs):
        w = 2.0 * np.pi * fm
        out[2 * f] = mask * np.cos(w * t_us)
        out[2 * f + 1] = mask * np.sin(w * t_us)
    return out


def make_list(rng, length, n_series):
    """One list: ``length`` (series, scale) pairs, scales distinct and of either sign, |scale| in [0.05, 0.5] rad/us.
    Dropping the last entry is the defect the tests must see, so it is the term that does not average out over a
    window of a few periods - series 0, the lowest-frequency cosine - at the upper end of the range (lists of 65 and
    more entries: at the end itself)."""
    ser = rng.permutation(np.arange(1, n_series))[:length - 1] if length <= n_series else rng.integers(1, n_series, length - 1)
    ser = np.append(ser, 0)
    mag = rng.uniform(SCALE_LO, SCALE_HI, length)
    mag[-1] = SCALE_HI if length >= 65 else rng.uniform(0.6 * SCALE_HI, SCALE_HI)
    sign = rng.choice([-1.0, 1.0], length)
    scale = mag * sign
    assert len(np.unique(scale)) == length
    return [(int(s), float(c)) for s, c in zip(ser, scale)]


# what the slots of a batch get, in this order (0 = no list: ``extra`` = 0 between atoms that have one; "share" = the
# list of the slot before, once more); a batch with more slots starts over with new lists, one with fewer takes a prefix
_PLAN = (130, 1, 0, 65, 64, 63, 2, "share")


def standard_lists(n, entries, n_series=2 * N_FREQ, seed=0, plan=_PLAN):
    """``lists[b][k]`` for ``entries`` batch entries of ``n`` atoms: every (b, k) slot in turn takes the next item of the
    plan (130, 1, none, 65, 64, 63, 2, shared).  The caller adds ``[None] * n`` for an entry without any list."""
    rng = np.random.default_rng(1000 + seed)
    lists, prev, i = [], None, 0
    for _ in range(entries):
        row = []
        for _ in range(n):
            item = plan[i % len(plan)]
            i += 1
            if item == 0:
                row.append(None)
                continue
            if item != "share" or prev is None:
                prev = make_list(rng, 65 if item == "share" else item, n_series)
            row.append(prev)
        lists.append(row)
    return lists


def _key(lst):
    return (np.array([s for s, _ in lst], dtype=np.int64).tobytes(), np.array([c for _, c in lst], dtype=np.float64).tobytes())


def unique_lists(lists):
    """The distinct non-empty lists in (b, k) order: one table block each."""
    seen, out = set(), []
    for row in lists:
        for lst in row:
            if lst and _key(lst) not in seen:
                seen.add(_key(lst))
                out.append(lst)
    return out


def fold(problems, lists, series):
    """Problem b with ``sum scale * series`` added to the ``det`` samples of every atom that has a list."""
    series = np.asarray(series, dtype=float)
    out = []
    for p, row in zip(problems, lists):
        q = dict(p)
        q["samples"] = copy.deepcopy(p["samples"])
        basis = p["basis_name"]
        for k, lst in enumerate(row):
            if not lst:
                continue
            add = sum(c * series[s] for s, c in lst)
            loc = q["samples"].setdefault("Local", {}).setdefault(basis, {})
            if k in loc:
                loc[k]["det"] = np.asarray(loc[k]["det"], dtype=float) + add
            else:  # a channel of its own on this atom: the terms of one atom add up
                loc[k] = {"amp": np.zeros_like(add), "det": add, "phase": np.zeros_like(add)}
        out.append(q)
    return out


def with_term_lists(problems, lists, series):
    """``(tables, folded_problems)``: ``lower(problems)`` with the M real ``series`` [M, duration] appended to the spline
    tables, one ``DTERM_DTYPE`` block per distinct list and ``desc["extra"]`` per (b, k); and the folded problems."""
    series = np.asarray(series, dtype=float)
    assert len(lists) == len(problems) and all(len(row) == int(problems[0]["n_qudits"]) for row in lists)
    tables = lower(problems)
    duration, rate = int(problems[0]["duration"]), float(problems[0].get("sampling_rate", 1.0))
    base = tables.pp.shape[0]
    knots = [np.ascontiguousarray(adapt_to_sampling_rate(s, rate, duration), dtype=np.complex128) for s in series]
    pp_new = np.empty((len(knots), len(tables.tknots) - 1, 4), dtype=np.complex128)
    for i, kn in enumerate(knots):
        pp_new[i] = np.transpose(CubicSpline(tables.tknots, kn, bc_type="not-a-knot").c, (1, 0))
    blocks, start = [], {}
    n_terms = 0
    for lst in unique_lists(lists):
        block = np.zeros(len(lst), dtype=DTERM_DTYPE)
        block["series"] = [base + s for s, _ in lst]
        block["scale"] = [c for _, c in lst]
        block["remaining"] = np.arange(len(lst) - 1, -1, -1)
        start[_key(lst)] = n_terms + 1  # 1-based
        n_terms += len(lst)
        blocks.append(block)
    desc = tables.desc.copy()
    for b, row in enumerate(lists):
        for k, lst in enumerate(row):
            desc["extra"][b, k] = start[_key(lst)] if lst else 0
    tables = replace(tables, pp=np.ascontiguousarray(np.concatenate([tables.pp, pp_new])),
                     series_knots=list(tables.series_knots) + knots, desc=desc,
                     dterms=np.concatenate(blocks) if blocks else None)
    return tables, fold(problems, lists, series)


def without_last(lists):
    """``lists`` with the last entry of the longest list removed (for every atom that shares it)."""
    longest = max(unique_lists(lists), key=len)
    cut = longest[:-1]
    return [[(cut if lst and _key(lst) == _key(longest) else lst) for lst in row] for row in lists]


def ref_without_last(problems, lists, series):
    """The folded problems of the same lists with the last entry of the longest one dropped: a kernel that loses the
    tail of its list computes THIS.  The tests assert that it lies 1000 tolerances from the true reference."""
    return fold(problems, without_last(lists), series)


def check_remaining(dterms):
    """The rule ``ryd_set_detuning_terms`` checks (host_handle.hpp): every count stays inside the table and counts down."""
    n = len(dterms)
    for i in range(n):
        r = int(dterms["remaining"][i])
        if r < 0 or i + r >= n or (r > 0 and int(dterms["remaining"][i + 1]) != r - 1):
            return False
    return True

"""The helper behind tests/test_gpu_detuning_terms.py (tests/dterm_ref.py), checked on the host: the tables it builds
and the folded problems it hands to the oracle must mean the same detuning."""
import numpy as np
import pytest

import dterm_ref as dr
from helpers import chain_problem, local_problem
from pulser_amd.terms import lower


def _case(n=5, batch=3, duration=41, seed=0):
    probs = [local_problem(n, seed=s, duration=duration) for s in range(batch)]
    lists = dr.standard_lists(n, batch - 1, seed=seed)
    lists.insert(1, [None] * n)
    return probs, lists, dr.noise_series(duration)


def _detuning_pp(tables, b, k):
    """The cubic pieces [n_int, 4] of delta_k(t) of entry b as the device sums them (include/rydemu.h)."""
    d = tables.desc[b, k]
    q = np.zeros(tables.pp.shape[1:], dtype=float)
    if d["det_series"] >= 0:
        q += d["det_scale"] * tables.pp[d["det_series"]].real
    if d["off_series"] >= 0:
        q += d["off_scale"] * tables.pp[d["off_series"]].real
    if d["extra"] > 0:
        e = d["extra"] - 1
        while True:
            t = tables.dterms[e]
            q += t["scale"] * tables.pp[t["series"]].real
            if t["remaining"] == 0:
                break
            e += 1
    return q


@pytest.mark.parametrize("kind", ["local", "global"])
def test_folded_samples_spline_equals_the_sum_of_the_table_pieces(kind):
    if kind == "local":
        probs, lists, series = _case()
    else:  # a global channel: the folded problem gets a channel of its own on the atoms with a list
        probs = [chain_problem(4)]
        probs[0] = dict(probs[0], duration=61, samples={"Global": {"ground-rydberg": {
            k: np.asarray(v)[1000:1061].copy() for k, v in probs[0]["samples"]["Global"]["ground-rydberg"].items()}}, "Local": {}})
        lists, series = dr.standard_lists(4, 1, seed=3), dr.noise_series(61)
    tables, folded = dr.with_term_lists(probs, lists, series)
    plain = lower(probs)
    assert np.array_equal(tables.pp[:plain.pp.shape[0]], plain.pp) and tables.pp.shape[0] == plain.pp.shape[0] + len(series)
    assert len(tables.series_knots) == tables.pp.shape[0]
    assert not np.any(tables.pp[plain.pp.shape[0]:].imag)
    worst = 0.0
    for b, p in enumerate(folded):
        ref = lower([p])
        for k in range(tables.n_qubits):
            want = _detuning_pp(ref, 0, k)
            got = _detuning_pp(tables, b, k)
            scale = np.max(np.abs(want), axis=0)  # per power of (t - t_i)
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300))))
            # the drive is untouched
            a, c = tables.desc[b, k], ref.desc[0, k]
            if a["drive_series"] >= 0:
                assert np.array_equal(tables.pp[a["drive_series"]] * a["drive_scale"], ref.pp[c["drive_series"]] * c["drive_scale"])
            else:
                assert c["drive_series"] < 0
    assert worst <= 1e-13, worst


def test_remaining_counts_and_extra_indices_follow_the_abi_rule():
    probs, lists, series = _case()
    tables, _ = dr.with_term_lists(probs, lists, series)
    dt = tables.dterms
    assert dt.dtype == dr.DTERM_DTYPE and dr.check_remaining(dt)
    bad = dt.copy()
    bad["remaining"][0] += 1
    assert not dr.check_remaining(bad)
    bad = dt.copy()
    bad["remaining"][-1] = 1  # runs past the table
    assert not dr.check_remaining(bad)
    n_series = tables.pp.shape[0]
    assert dt["series"].min() >= lower(probs).pp.shape[0] and dt["series"].max() < n_series
    # every extra points at the head of a list whose length is the list's, and the last list ends the table
    for b, row in enumerate(lists):
        for k, lst in enumerate(row):
            e = int(tables.desc["extra"][b, k])
            if not lst:
                assert e == 0
                continue
            assert 1 <= e <= len(dt) and dt["remaining"][e - 1] == len(lst) - 1
            assert np.array_equal(dt["scale"][e - 1:e - 1 + len(lst)], [c for _, c in lst])
    assert np.all(tables.desc["extra"][1] == 0)  # the entry without any list
    last = dr.unique_lists(lists)[-1]
    assert np.max(tables.desc["extra"]) - 1 + len(last) == len(dt)
    # the shapes every family sums, a gap between atoms with lists, distinct scales of either sign in range
    assert {len(l) for l in dr.unique_lists(lists)} >= set(dr.LENGTHS)
    ex0 = tables.desc["extra"][0]
    assert any(ex0[k] == 0 and ex0[k - 1] > 0 and ex0[k + 1] > 0 for k in range(1, len(ex0) - 1))
    for l in dr.unique_lists(lists):
        sc = np.array([c for _, c in l])
        assert len(np.unique(sc)) == len(sc) and np.all(np.abs(sc) >= dr.SCALE_LO) and np.all(np.abs(sc) <= dr.SCALE_HI)
        assert len(l) < 2 or (sc.min() < 0 < sc.max()) or len(l) == 2


def test_shared_lists_get_one_table_block():
    probs, lists, series = _case()
    shared = [(b, k) for b, row in enumerate(lists) for k in range(1, len(row)) if row[k] is not None and row[k] is row[k - 1]]
    assert shared
    tables, _ = dr.with_term_lists(probs, lists, series)
    for b, k in shared:
        assert tables.desc["extra"][b, k] == tables.desc["extra"][b, k - 1] > 0
    assert len(tables.dterms) == sum(len(l) for l in dr.unique_lists(lists))
    assert len(dr.unique_lists(lists)) < sum(1 for row in lists for l in row if l)


def test_reference_without_the_last_term_differs_only_on_the_atoms_of_the_longest_list():
    probs, lists, series = _case()
    _, folded = dr.with_term_lists(probs, lists, series)
    cut = dr.ref_without_last(probs, lists, series)
    longest = max(dr.unique_lists(lists), key=len)
    assert len(longest) == 130
    s, c = longest[-1]
    hit = 0
    for b, row in enumerate(lists):
        for k, lst in enumerate(row):
            a = folded[b]["samples"]["Local"]["ground-rydberg"][k]["det"]
            d = cut[b]["samples"]["Local"]["ground-rydberg"][k]["det"]
            if lst is longest:
                hit += 1
                assert np.allclose(a - d, c * series[s], rtol=0, atol=1e-13) and np.max(np.abs(a - d)) > 0.4
            else:
                assert np.array_equal(a, d)
    assert hit >= 1
    # the inputs are left as they were
    assert all(np.array_equal(p["samples"]["Local"]["ground-rydberg"][0]["det"],
                              local_problem(5, seed=i, duration=41)["samples"]["Local"]["ground-rydberg"][0]["det"])
               for i, p in enumerate(probs))

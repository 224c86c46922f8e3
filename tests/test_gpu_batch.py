"""-m gpu: many sequences of different durations in one solve (pulser_amd.batch: solve_many / run_batch) and the
per-entry snapshot map behind it (ryd_set_snapshot_map) on every store path."""
from __future__ import annotations

import dataclasses
import os
import sys
import warnings

import numpy as np
import pytest

from helpers import blockade_radius, fuzz_case, load_fixture, with_anneal_samples

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _oracle_kets(name):
    """(problem, t_end, tight-oracle ket) of every stored ket of a fuzz fixture, the inputs checked against the fixture's
    digests first (tests/golden/make_fuzz_fixtures.py)."""
    sys.path.insert(0, GOLDEN)
    from make_fuzz_fixtures import digest

    fx = np.load(os.path.join(GOLDEN, name))
    out = []
    for r in range(len(fx["state_owner"])):
        k, b = (int(v) for v in fx["state_owner"][r])
        over = int(fx["n_override"][k])
        probs, desc = fuzz_case(int(fx["seeds"][k]), None if over < 0 else over)
        assert digest(probs[b]) == str(fx["input_sha256"][r]), f"fuzz_case({fx['seeds'][k]}) has drifted from the fixture"
        out.append((probs[b], float(fx["state_t_end"][r]), fx["states"][r][: 2 ** int(fx["state_atoms"][r])], desc))
    return out


def _solve_fixture(name, n_solves):
    from pulser_amd.batch import solve_many

    cases = _oracle_kets(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = solve_many([c[0] for c in cases], [[0.0, c[1]] for c in cases])
    assert len(res.chunks) == n_solves
    worst = 0.0
    for (prob, t_end, ref, desc), psi in zip(cases, res.states):
        got = psi.cpu().numpy()
        assert got.shape == (1, ref.size)
        e = float(np.max(np.abs(got[0] - ref)))
        worst = max(worst, e)
        assert e < 1e-7, (desc, t_end, e)
    return cases, res, worst


def test_fuzz_oracle_12_in_one_ragged_solve():
    """All 34 kets of fuzz_oracle_12 (24 seeds, 117 - 3 700 ns, different registers and waveforms) in ONE solve on
    k_split_reg<12, 4>, every final ket within 1e-7 of the tight oracle."""
    cases, res, _ = _solve_fixture("fuzz_oracle_12.npz", 1)
    assert len(cases) == 34 and res.stats[0]["batch"] == 34
    assert len({int(c[0]["duration"]) for c in cases}) > 10


def test_fuzz_oracle_14_in_one_ragged_solve():
    cases, res, _ = _solve_fixture("fuzz_oracle_14.npz", 1)
    assert len(cases) == 8


def test_fuzz_oracle_small_grouped_by_atom_count():
    """fuzz_oracle_small: 8 - 11 atoms, one solve per register size (k_traj)."""
    cases, res, _ = _solve_fixture("fuzz_oracle_small.npz", 4)
    assert sorted(len(c) for c in res.chunks) == sorted(
        np.unique([int(c[0]["n_qudits"]) for c in cases], return_counts=True)[1].tolist())


# -- the map on every store path -------------------------------------------------------------------------------------
def _ragged_problems(n):
    from pulser_amd import problem as P

    coords = P.register_coords(P.square_rect(1, n), blockade_radius())
    out = []
    for k, dur in enumerate((180, 260, 221)):
        t = np.arange(dur + 1) / 1000.0
        T = t[-1]
        s = {"amp": (6.0 + k) * np.sin(np.pi * t / T) ** 2, "det": -8.0 + 16.0 * t / T + k, "phase": np.zeros(dur + 1)}
        out.append(P.make_ising_problem(coords, s))
    return out


PATHS = [
    (9, "k_traj", {}, {}),
    (9, "tiled passes", {"force_generic": True}, {}),
    (9, "Taylor", {"force_generic": True}, {"method": "taylor"}),
    (9, "Lanczos", {"force_generic": True}, {"method": "krylov"}),
    (12, "k_ket", {"force_ket": True}, {}),
    (12, "k_split_reg in-run snapshots", {}, {}),
    (12, "k_split_reg snaps_outside", {"snaps_outside": True}, {}),
    (15, "split-operator passes", {}, {}),
    (15, "Taylor", {"no_split": True}, {"method": "taylor"}),
]


@pytest.mark.parametrize("n, label, path, kw", PATHS, ids=[f"{p[0]}-{p[1]}" for p in PATHS])
def test_snapshot_map_is_bit_for_bit_on_every_store_path(n, label, path, kw):
    """The same solve with and without a map: every mapped slot equals the dense snapshot bit for bit (the times, and so
    the schedule, are the same); every row nothing maps to keeps its NaN."""
    import torch

    from pulser_amd.engine import Engine
    from pulser_amd.terms import lower_ragged

    probs = _ragged_problems(n)
    tables = lower_ragged(probs)
    times = np.array([0.0, 0.05, 0.1, 0.1, 0.181, 0.222, 0.261])
    S, B, D = len(times) - 1, len(probs), 2**n
    rng = np.random.default_rng(n)
    offsets = np.full((B, S), -1, dtype=np.int64)
    rows = rng.permutation(3 * S)  # scattered, some slots unmapped, spare rows
    k = 0
    for b in range(B):
        for s in range(S):
            if rng.random() < 0.7:
                offsets[b, s] = rows[k]
                k += 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with Engine(tables, mode="sesolve") as eng:
            eng.set_path(**{"force_generic": False, **path})
            st = eng.new_state()
            dense = eng.solve(st, times, **kw).cpu().numpy()
            dense_stats = eng.stats()
        with Engine(tables, mode="sesolve") as eng:
            eng.set_path(**{"force_generic": False, **path})
            eng.set_snapshot_map(offsets)
            out = torch.full((3 * S + 2, D), complex(np.nan, np.nan), dtype=torch.complex128, device=eng.device)
            st = eng.new_state()
            eng.solve(st, times, out=out, **kw)
            mapped = out.cpu().numpy()
            assert eng.stats()["n_steps"] == dense_stats["n_steps"], label
    used = set()
    for b in range(B):
        for s in range(S):
            if offsets[b, s] >= 0:
                assert np.array_equal(mapped[offsets[b, s]], dense[s, b]), (label, b, s)
                used.add(int(offsets[b, s]))
    for r in range(len(mapped)):
        if r not in used:
            assert np.all(np.isnan(mapped[r].real)) and np.all(np.isnan(mapped[r].imag)), (label, r)


def test_snapshot_map_arguments():
    from pulser_amd._lib import RydError
    from pulser_amd.engine import Engine
    from pulser_amd.terms import lower_ragged

    probs = _ragged_problems(9)
    with Engine(lower_ragged(probs), mode="sesolve") as eng:
        eng.set_snapshot_map(np.zeros((3, 2), dtype=np.int64) - 1)
        with pytest.raises(ValueError, match="2 slots"):
            eng.solve(eng.new_state(), [0.0, 0.1])
        eng.set_snapshot_map(None)
        assert eng.solve(eng.new_state(), [0.0, 0.1]).shape == (1, 3, 512)
    prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
    with Engine.from_problems([with_anneal_samples(prob)], mode="mesolve") as eng:
        with pytest.raises(RydError, match="two-level sesolve"):
            eng.set_snapshot_map(np.zeros((1, 1), dtype=np.int64))


# -- the public call ---------------------------------------------------------------------------------------------------
def _emulator(n, dur, k, evaluation_times, xy=False, noise=None, n_traj=None):
    from pulser_amd import QutipEmulator
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import single_global_channel

    coords = P.register_coords(P.square_rect(2, n // 2) if n > 3 else P.square_rect(1, n), blockade_radius())
    t = np.arange(dur) / dur
    s = {"amp": (5.0 + 0.5 * k) * np.sin(np.pi * t) ** 2, "det": -10.0 + (20.0 - k) * t, "phase": np.zeros(dur)}
    inputs = single_global_channel(coords, s, 3700.0 if xy else P.C6_LEVEL70, basis="XY" if xy else "ground-rydberg",
                                   extended=False)
    if xy:  # (C3 = 3700, field along z)
        inputs = dataclasses.replace(inputs, interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))
    kw = {}
    if noise is not None:
        kw = dict(noise_model=noise, n_trajectories=n_traj)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return QutipEmulator(inputs, evaluation_times=evaluation_times, **kw)


def _runs(emus, **options):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return [e.run(**options) for e in emus]


def test_run_batch_matches_solo_runs():
    """Six 12-atom sequences of 400 - 1 200 ns, evaluation times "Minimal", 0.5, an explicit list and "Full", some with
    their own initial state: every result has its solo run()'s evaluation times, and every state lies within 2e-7."""
    from pulser_amd import run_batch

    specs = [(400, "Minimal"), (560, 0.5), (720, [0.0, 0.1, 0.25, 0.4]), (880, "Full"), (1040, 0.5), (1200, "Minimal")]
    make = lambda: [_emulator(12, d, k, ev) for k, (d, ev) in enumerate(specs)]
    emus, solo_emus = make(), make()
    rng = np.random.default_rng(3)
    for i in (1, 4):
        psi = rng.normal(size=4096) + 1j * rng.normal(size=4096)
        psi /= np.linalg.norm(psi)
        emus[i].set_initial_state(psi)
        solo_emus[i].set_initial_state(psi)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = run_batch(emus)
        solo = _runs(solo_emus)
    for i, (g, s) in enumerate(zip(got, solo)):
        assert type(g) is type(s)
        assert np.array_equal(np.asarray(g._sim_times), np.asarray(s._sim_times)), i
        gs, ss = g.states, s.states
        assert len(gs) == len(ss)
        for a, b in zip(gs, ss):
            e = float(np.max(np.abs(np.asarray(a.full()) - np.asarray(b.full()))))
            assert e < 2e-7, (i, e)
        assert emus[i].last_engine_stats["batch"] == 6


def test_run_batch_runs_the_rest_on_their_own():
    """A noisy and an XY emulator among batched ones: their results equal their solo run()'s (Counters under the same
    np.random seed)."""
    from pulser_amd import NoiseModel, run_batch

    def make():
        return [_emulator(12, 500, 0, "Minimal"),
                _emulator(4, 300, 1, "Minimal", noise=NoiseModel(samples_per_run=1, temperature=20000), n_traj=6),
                _emulator(3, 300, 2, "Minimal", xy=True),
                _emulator(12, 700, 3, 0.5)]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        np.random.seed(21)
        got = run_batch(make())
        np.random.seed(21)
        solo = _runs(make())
    g, s = got[1], solo[1]
    assert type(g) is type(s) and len(g.results) == len(s.results) and g.results == s.results
    a, b = got[2].get_final_state(), solo[2].get_final_state()
    assert np.array_equal(np.asarray(a.full()), np.asarray(b.full()))
    for i in (0, 3):
        assert np.max(np.abs(np.asarray(got[i].get_final_state().full())
                             - np.asarray(solo[i].get_final_state().full()))) < 2e-7


def test_256_distinct_anneals_headline_register():
    """256 distinct 14-atom anneals (amplitude and detuning spread +-1 %, sequence 0 nominal) in one solve: sequence 0's
    final ket within 1e-7 of the tight headline fixture."""
    from pulser_amd.batch import solve_many

    prob, extra = load_fixture("ns_tri14_anneal.npz")
    prob = with_anneal_samples(prob)
    t_end = float(np.asarray(extra["eval_times"])[-1])
    rng = np.random.default_rng(7)
    probs = []
    for b in range(256):
        fa, fd = (1.0, 1.0) if b == 0 else tuple(1.0 + 0.01 * (2.0 * rng.random(2) - 1.0))
        s = prob["samples"]["Global"]["ground-rydberg"]
        p = dict(prob)
        p["samples"] = {"Global": {"ground-rydberg": dict(s, amp=fa * np.asarray(s["amp"]), det=fd * np.asarray(s["det"]))},
                        "Local": {}}
        probs.append(p)
    res = solve_many(probs, [[0.0, t_end]] * 256)
    assert len(res.chunks) == 1
    e = float(np.max(np.abs(res.states[0].cpu().numpy()[0] - np.asarray(extra["oracle_states_tight"])[-1])))
    assert e < 1e-7, e
    assert float(np.max(np.abs(res.states[200].cpu().numpy()[0] - res.states[0].cpu().numpy()[0]))) > 1e-4

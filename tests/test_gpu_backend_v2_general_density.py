"""GPU: ``QutipBackendV2.general_density_one_call`` - the built-in observables, ``Fidelity`` and ``Expectation`` of a
multi-level or XY master-equation run from device calls over the run's density matrices, which never leave the GPU
(``QutipEmulator.run(general_density_snapshots=True)``, ``GeneralEngine.observe_density_many``, ``overlap_many``,
``expect_sparse``), against the same run with the attribute False - the per-time path, unchanged.

Two runs: the ``noisy_xy_0`` inputs (XY, 4 atoms, D = 16) with ``NoiseModel(dephasing_rate=0.05)`` and the inputs behind
``general_oracle_all4_me`` (3-level "all" basis on a 2 x 2 square, D = 81) with relaxation and both dephasing channels,
each at 130 evaluation times.

Bounds.  The two paths divide by different numbers, on purpose: the per-time path normalises the matrix on the host by
its trace norm (an SVD), the one-call path divides the device sums by the device trace.  In exact arithmetic
``on = off * ||rho||_1 / Tr rho``, and that factor is read off a third run that stores the normalised matrices
``rho^ = rho / ||rho||_1``: ``scale = 1 / Re Tr rho^``.  Each value of the one-call run is compared with ``off * scale``
within the SUM of the two paths' bounds on ``rho^`` - ``observe_ref.tol_sum`` for the pair sums, ``tol_energy_dm_general``
for the energy moments (both paths are held to them in tests/test_gpu_general_observe*.py), ``tol_sum(D^2, S_abs)`` for
``<phi|rho|phi>`` and ``Tr(A rho)`` (D^2 products in some order, S_abs the sum of their moduli) - plus ``(D + 12) u |v|``
for the two normalisations and the D-term sum behind ``scale``.  Nothing is fitted to what either path gives.  Worst ratios
seen on an MI355X: pair sums 0.079, energy moments 3.2e-05, variance 7.3e-06, fidelity 0.0084, expectation 0.011.
"""
import os
import sys

import numpy as np
import pytest

from helpers import load_fixture
from general_observe_ref import ref_pairs_d, tol_energy_dm_general
from observe_ref import U53, ref_energy_dm, tol_sum
from test_gpu_general_observe_many import _Reads, _count_calls

pytestmark = pytest.mark.gpu

N_TIMES = 130


def _xy_case():
    from pulser_amd import NoiseModel
    from pulser_amd.hamiltonian_data import SequenceInputs

    prob, _ = load_fixture("noisy_xy_0.npz")
    return SequenceInputs.from_dict(prob["inputs"]), NoiseModel(dephasing_rate=0.05), ("d", "u"), {"dddd": 0.6, "uddd": 0.8j}


def _all4_case():
    from pulser_amd import NoiseModel
    from pulser_amd import problem as P
    from test_host_logic import _inputs_from_problem

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_general_fixtures as G

    prob = G.multilevel_problem(P.register_coords(P.square_rect(2, 2), 6.0), 161, 10, local=(1,))
    nm = NoiseModel(relaxation_rate=0.5, dephasing_rate=0.7, hyperfine_dephasing_rate=0.3)
    return _inputs_from_problem(prob), nm, ("r", "h"), {"gggg": 0.6, "rggh": 0.8j}


CASES = {"xy": _xy_case, "all4": _all4_case}


def _observables(eigenstates, ones, amplitudes, D):
    from pulser_amd.backend import (CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance, Expectation, Fidelity,
                                    Occupation, RydState)

    one, other = ones
    rng = np.random.default_rng(31)
    a = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    target = RydState.from_state_amplitudes(eigenstates=eigenstates, amplitudes=amplitudes)
    return [Occupation(one_state=one), CorrelationMatrix(one_state=one), Energy(), EnergySecondMoment(), EnergyVariance(),
            Occupation(one_state=other, tag_suffix="other"), Fidelity(target), Expectation(a + a.conj().T)]


def _run(inputs, cfg, attribute, min_times=128):
    from pulser_amd.backend import QutipBackendV2

    backend = QutipBackendV2(inputs, config=cfg)
    backend.observe_many_min_times = min_times
    if attribute:
        backend.general_density_one_call = True
    res = backend.run()
    assert QutipBackendV2.general_density_one_call is False
    return res, QutipBackendV2.last_observable_engine_stats, backend._sim_obj


def _count_density_calls(monkeypatch):
    """The (shape, digit, energy) of every ``GeneralEngine.observe_density_many`` call, and the (shape, density) of every
    ``overlap_many`` / ``expect_sparse`` call."""
    from pulser_amd import engine

    dens, overlaps, expects = [], [], []
    real_d, real_o, real_e = engine.GeneralEngine.observe_density_many, engine.overlap_many, engine.expect_sparse

    def counted_d(self, states, times, one=0, **kw):
        dens.append((tuple(states.shape), one, kw.get("energy", True)))
        return real_d(self, states, times, one=one, **kw)

    def counted_o(states, targets, **kw):
        overlaps.append((tuple(states.shape), kw.get("density")))
        return real_o(states, targets, **kw)

    def counted_e(states, op, **kw):
        expects.append((tuple(states.shape), kw.get("density")))
        return real_e(states, op, **kw)

    monkeypatch.setattr(engine.GeneralEngine, "observe_density_many", counted_d)
    monkeypatch.setattr(engine, "overlap_many", counted_o)
    monkeypatch.setattr(engine, "expect_sparse", counted_e)
    return dens, overlaps, expects


def _setup(which):
    from pulser_amd.backend import QutipConfig, StateResult

    inputs, nm, ones, amplitudes = CASES[which]()
    eigenstates = ("u", "d") if which == "xy" else ("r", "g", "h")
    d, n = len(eigenstates), 4
    D = d**n
    times = np.linspace(0.01, 1.0, N_TIMES).tolist()
    obs = _observables(eigenstates, ones, amplitudes, D)
    cfg = QutipConfig(default_evaluation_times=times, observables=obs, noise_model=nm)
    # the third run: the normalised matrices of every time
    sr = StateResult()
    res, _, sim = _run(inputs, QutipConfig(default_evaluation_times=times, observables=[sr], noise_model=nm), False)
    assert tuple(sim._hamiltonian_data.eigenbasis) == eigenstates
    states = {t: np.asarray(res.get_result(sr, t).to_qobj()) for t in res.get_result_times(sr)}
    assert len(states) == N_TIMES and all(s.shape == (D, D) for s in states.values())
    return inputs, cfg, obs, times, states, eigenstates, ones, D


def _compare(on, off, obs, states, sim, eigenstates, ones):
    """Every tagged result of the one-call run against the per-time run, as the module docstring derives."""
    from oracle import qutip_path as qp

    ham = qp.build_hamiltonian(dict(sim._noiseless_problem))
    T_us = sim.total_duration_ns / 1000
    d, n = len(eigenstates), 4
    D = d**n
    # (the XY fixture's drive has phase 0; the 3-level drives do not: there H is not real and rows are not columns)
    assert d == 2 or np.max(np.abs(ham.matrix(0.5 * T_us).toarray().imag)) > 1e-3
    phi = np.asarray(obs[6].state.to_qobj()).reshape(-1)
    A = np.asarray(obs[7].operator)
    assert on.get_tagged_results().keys() == off.get_tagged_results().keys()
    ok, worst = True, {}
    for t in off.get_result_times(obs[0]):
        rho = states[t]
        scale = 1.0 / float(np.real(np.trace(rho)))
        norm_u = (D + 12) * U53
        e1_ref, e2_ref, s_abs = ref_energy_dm(ham, t * T_us, rho)
        t1, t2 = tol_energy_dm_general(ham, t * T_us, rho, s_abs)
        tols = {}
        for o, one in ((obs[0], ones[0]), (obs[1], ones[0]), (obs[5], ones[1])):
            _, _, _, (_, s_occ, s_corr) = ref_pairs_d(np.real(np.diag(rho)), n, d, eigenstates.index(one))
            tols[o.uuid] = 2 * tol_sum(D, s_corr if o is obs[1] else s_occ)
        tols[obs[2].uuid], tols[obs[3].uuid] = 2 * t1, 2 * t2
        tols[obs[6].uuid] = 2 * tol_sum(D * D, float(np.abs(phi) @ np.abs(rho) @ np.abs(phi)))
        tols[obs[7].uuid] = 2 * tol_sum(D * D, float(np.sum(np.abs(A) * np.abs(rho.T))))
        for o in obs:
            if o is obs[4]:
                continue
            want = np.asarray(off.get_result(o, t)) * scale
            err = np.abs(np.asarray(on.get_result(o, t)) - want)
            tol = np.asarray(tols[o.uuid], dtype=float) + norm_u * np.abs(want)
            ok &= bool(np.all(err <= tol))
            worst[o.tag] = max(worst.get(o.tag, 0.0), float(np.max(err / tol)))
        # the variance e2 - e1^2 from the scaled moments of the per-time run
        e1, e2 = off.get_result(obs[2], t) * scale, off.get_result(obs[3], t) * scale
        tv = 2 * t2 + norm_u * abs(e2) + 2 * abs(e1) * (2 * t1 + norm_u * abs(e1)) + (2 * t1 + norm_u * abs(e1)) ** 2
        ev = abs(on.get_result(obs[4], t) - (e2 - e1 * e1))
        ok &= ev <= tv
        worst[obs[4].tag] = max(worst.get(obs[4].tag, 0.0), ev / tv)
    print("RATIO backend one-call vs per-time:", " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    return ok


@pytest.mark.parametrize("which", ["xy", "all4"])
def test_one_call_per_digit_no_state_read_and_the_values_of_the_per_time_path(which, monkeypatch):
    inputs, cfg, obs, times, states, eigenstates, ones, D = _setup(which)
    off, stats_off, _ = _run(inputs, cfg, False)
    assert stats_off["n_applications"] >= N_TIMES, stats_off  # the per-time path: generator applications at every time
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    dens, overlaps, expects = _count_density_calls(monkeypatch)
    on, stats, sim = _run(inputs, cfg, True)
    assert reads.stores == 1 and reads.gets == [] and reads.bulk == 0, (reads.stores, reads.gets, reads.bulk)
    assert [c[0] for c in dens] == [(N_TIMES, 1, D, D)] * 2 and [c[2] for c in dens] == [True, False], dens
    assert {c[1] for c in dens} == {eigenstates.index(o) for o in ones}
    assert many == [] and single == [], (many, single)
    # Fidelity and Expectation: the overlap route on the same 4-axis store, one call each
    assert overlaps == [((N_TIMES, D, D), True)] and expects == [((N_TIMES, D, D), True)], (overlaps, expects)
    assert stats["n_applications"] == 0 and stats["n_launches"] == 3 + 1, stats
    assert _compare(on, off, obs, states, sim, eigenstates, ones)


@pytest.mark.parametrize("which", ["xy", "all4"])
def test_below_the_floor_the_route_stays_shut(which, monkeypatch):
    """127 evaluation times with the attribute set and a threshold of 1: host states, per-time calls, the launches of the
    default route."""
    from pulser_amd.backend import QutipConfig

    inputs, nm, ones, amplitudes = CASES[which]()
    eigenstates = ("u", "d") if which == "xy" else ("r", "g", "h")
    D = len(eigenstates) ** 4
    obs = _observables(eigenstates, ones, amplitudes, D)
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, 127).tolist(), observables=obs, noise_model=nm)
    off, stats_off, _ = _run(inputs, cfg, False)
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    dens, overlaps, expects = _count_density_calls(monkeypatch)
    for threshold in (128, 1):
        on, stats, _ = _run(inputs, cfg, True, min_times=threshold)
        assert dens == [] and many == [] and overlaps == [] and expects == [] and reads.stores == 0
        for key in ("apply_path", "n_launches", "n_applications"):
            assert stats[key] == stats_off[key], (key, stats, stats_off)
        assert on.get_tagged_results().keys() == off.get_tagged_results().keys()
    assert len(single) > 0


def test_a_callback_that_reads_the_state_sees_the_states_of_the_default_route(monkeypatch):
    """A callback reads ``state`` at three times: exactly those snapshots are copied, and they are bitwise the matrices
    the default route hands over (``_DeferredRydState`` divides by the trace norm as the eager construction does)."""
    from pulser_amd.backend import QutipConfig

    inputs, nm, ones, amplitudes = CASES["all4"]()
    eigenstates = ("r", "g", "h")
    D = 81
    obs = _observables(eigenstates, ones, amplitudes, D)
    times = np.linspace(0.01, 1.0, N_TIMES).tolist()
    seen = {}

    def callback(config, t, state, hamiltonian, result):  # (callbacks see every time of the 1-ns grid: 160 ns)
        ns = t * 160
        if any(abs(ns - p) < 1e-6 for p in (20, 81, 160)):
            seen[int(round(ns))] = np.array(state.to_qobj())

    cfg = QutipConfig(default_evaluation_times=times, observables=obs, callbacks=[callback], noise_model=nm)
    _run(inputs, cfg, False)
    kept = dict(seen)
    seen.clear()
    assert len(kept) == 3 and all(v.shape == (D, D) for v in kept.values())
    reads = _Reads(monkeypatch)
    dens, _, _ = _count_density_calls(monkeypatch)
    _run(inputs, cfg, True)
    assert len(dens) == 2 and len(reads.gets) == 3 and reads.bulk == 0, (dens, reads.gets, reads.bulk)
    assert seen.keys() == kept.keys()
    for k in kept:
        assert np.array_equal(seen[k], kept[k]), k

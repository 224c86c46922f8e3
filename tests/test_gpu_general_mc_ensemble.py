"""GPU: quantum-jump ensembles of multi-level and XY registers without the density matrix -
``QutipEmulator.run(general_jumps=True, mc_ensemble=True)`` against the default general-jump route on the SAME
trajectories (d = 2, 3, 4; every digit), two chunks, the runs the default route refuses (14 XY atoms, 9 three-level
atoms) against a longdouble reduction of their kets, and ``QutipBackendV2.general_jumps`` with ``mc_ensemble``.

Bounds (none fitted to what the kernels give; those of tests/test_gpu_mc_ensemble.py with the d-level references):
 * two routes, same trajectories: the ensemble diagonal against ``diag`` of the averaged matrix within
   2 (ntraj + 8) u; pair sums of every digit within ``tol_sum(D + ntraj, S_abs)`` once per route of
   ``general_observe_ref.ref_pairs_d``; energy moments within ``tol_energy_dm_general`` of the averaged matrix plus the
   mean over the trajectories of the per-ket ``tol_energy_ket``, H(t) the oracle's of the noiseless problem.
 * capability runs: ``tol_diag`` / ``tol_sum`` against the trajectory sum of |psi_b|^2 in longdouble.
 * sampling: the Counters are EQUAL when no drawn uniform lies within 1e-12 of a boundary of the reference route's
   cumulative weights; the seed is advanced until the reference route says so.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

from ensemble_ref import ref_diag, tol_diag
from general_observe_ref import ref_pairs_d, tol_energy_dm_general
from observe_ref import LD, U53, ket_probabilities, ref_energy_dm, ref_energy_ket, tol_energy_ket, tol_sum

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd import problem as P
from pulser_amd.results import EnsembleState

pytestmark = pytest.mark.gpu

NTRAJ = 300
NONDIAG = np.array([[1.0, 1.0], [0.0, 0.0]], dtype=complex)


def _xy_inputs(rows, cols, spacing, dur, amp):
    """A global microwave pulse amp sin^2(pi t / dur) on a rows x cols XY register (C3 = 3700, field along z)."""
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    n = rows * cols
    coords = P.register_coords(P.square_rect(rows, cols), spacing)
    t = np.arange(dur)
    ch = ChannelInput("mw", "Global", "XY", amp * np.sin(np.pi * t / dur) ** 2, np.full(dur, -2.0), np.zeros(dur),
                      [Slot(0, dur, tuple(range(n)))])
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), [ch], 5420158.53,
                          interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))


def _all_inputs(rows, cols, spacing, dur, amp=9.0):
    """A Rydberg and a Raman pulse, both global, on a rows x cols register: the 3-level "all" basis."""
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    n = rows * cols
    coords = P.register_coords(P.square_rect(rows, cols), spacing)
    t = np.arange(dur)
    slot = [Slot(0, dur, tuple(range(n)))]
    chans = [ChannelInput("ryd", "Global", "ground-rydberg", amp * np.sin(np.pi * t / dur) ** 2, np.full(dur, -1.0),
                          np.zeros(dur), list(slot)),
             ChannelInput("ram", "Global", "digital", 6.0 * np.sin(np.pi * t / dur) ** 2, np.full(dur, 0.5),
                          np.full(dur, 0.3), list(slot))]
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), chans, P.C6_LEVEL70)


def _all3_inputs():
    from helpers import load_fixture
    from test_host_logic import _inputs_from_problem

    prob, extra = load_fixture("noises_all_0.npz")
    meas = extra["aux"]["meas_basis"]
    return _inputs_from_problem(prob, measurement=meas if meas != "digital" else None)


def _tri4_inputs():
    from helpers import load_fixture, with_anneal_samples
    from test_host_logic import _inputs_from_problem

    prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
    return _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")


def _leak_ops():
    """|x><r| and |x><g| in the eigenbasis (r, g, h, x) of the "all" basis with leakage."""
    a, b = np.zeros((4, 4), dtype=complex), np.zeros((4, 4), dtype=complex)
    a[3, 0] = b[3, 1] = 1.0
    return [a, b]


# kind -> (inputs, noise model, sampling rate, local dimension, atoms)
CASES = {
    "xy4": lambda: (_xy_inputs(2, 2, 8.0, 500, 8.0), NoiseModel(dephasing_rate=3.0), 0.1, 2, 4),
    "all3": lambda: (_all3_inputs(), NoiseModel(relaxation_rate=1.0, dephasing_rate=0.5, hyperfine_dephasing_rate=0.3),
                     0.01, 3, 3),
    "leak2": lambda: (_all_inputs(1, 2, 7.0, 400), NoiseModel(eff_noise_opers=_leak_ops(), eff_noise_rates=[2.0, 1.0],
                                                             with_leakage=True), 1.0, 4, 2),
    "nondiag4": lambda: (_tri4_inputs(), NoiseModel(eff_noise_opers=[NONDIAG], eff_noise_rates=[0.3]), 1.0, 2, 4),
}


def _emulator(kind, ntraj=NTRAJ, inner=(0.3, 0.55, 0.8)):
    inputs, nm, rate, d, n = CASES[kind]()
    dur_us = max(len(ch.amp) for ch in inputs.channels) / 1000
    emu = QutipEmulator(inputs, sampling_rate=rate, noise_model=nm, solver=Solver.MCSOLVER, n_trajectories=ntraj,
                        evaluation_times=[round(f * dur_us, 3) for f in inner])
    prob = emu._current_problem
    assert emu._solver_mode(prob) == "mcsolve" and not emu._mc_fast_ok(prob)
    assert len(prob["eigenbasis"]) == d and prob["n_qudits"] == n
    return emu, d, n


def _oracle_hamiltonian(emu):
    from oracle import qutip_path as qp

    noiseless = dict(emu._current_problem)
    noiseless["collapse_ops"] = []
    return qp.build_hamiltonian(noiseless)


def _capture_kets(monkeypatch):
    """Host copies of what every ``GeneralEngine.mc_solve`` call stored: [T - 1, B, D] per chunk."""
    from pulser_amd.engine import GeneralEngine

    kept = []
    real = GeneralEngine.mc_solve

    def capturing(self, state, times, seeds, **kw):
        out = real(self, state, times, seeds, **kw)
        kept.append(out.cpu().numpy())
        return out

    monkeypatch.setattr(GeneralEngine, "mc_solve", capturing)
    return kept


def _ratio(err, bound):
    """max err / bound for the printed report (0 / 0 counts as 0)."""
    err, bound = np.asarray(err, dtype=float), np.asarray(bound, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(err > 0, err / bound, 0.0)))


def _safe_seed(cumulative, n_draws, margin=1e-12):
    """The first seed whose ``n_draws`` uniforms all keep ``margin`` away from every boundary of ``cumulative`` (the
    reference route's cumulative weights: it alone decides)."""
    for seed in range(100):
        np.random.seed(seed)
        u = np.random.rand(n_draws)
        if np.min(np.abs(u[:, None] - cumulative[None, :])) > margin:
            return seed
    raise AssertionError("no seed keeps the draws away from the boundaries")


def _pair_bounds(rho, n, d, digits, ntraj):
    """digit -> (occupation, correlation, their bounds) of the averaged matrix ``rho``: ``tol_sum(D + ntraj, S_abs)``
    once per route."""
    out = {}
    for digit in digits:
        _, occ, corr, (_, s_occ, s_corr) = ref_pairs_d(np.real(np.diag(rho)), n, d, digit)
        out[digit] = (occ, corr, 2 * tol_sum(d**n + ntraj, s_occ), 2 * tol_sum(d**n + ntraj, s_corr))
    return out


def _energy_bounds(ham, t_us, rho, kets):
    """(<H>, <H^2>, their bounds): ``tol_energy_dm_general`` of ``rho`` plus the mean over the trajectories ``kets``
    [B, D] of the per-ket ``tol_energy_ket``."""
    e1, e2, s_abs = ref_energy_dm(ham, t_us, rho)
    d1, d2 = tol_energy_dm_general(ham, t_us, rho, s_abs)
    k1 = k2 = 0.0
    for x in kets:
        _, _, s_ket, w = ref_energy_ket(ham, t_us, x)
        a, b = tol_energy_ket(x, w, s_ket)
        k1, k2 = k1 + a / len(kets), k2 + b / len(kets)
    return e1, e2, d1 + k1, d2 + k2


# ---------------------------------------------------------------------------------------------------------------------
# 1. the same trajectories on two routes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(CASES))
def test_same_trajectories_two_routes(kind, monkeypatch):
    kets = _capture_kets(monkeypatch)
    runs = []
    for ensemble in (False, True):
        emu, d, n = _emulator(kind)
        option = {"mc_ensemble": True, "mc_ensemble_digits": range(d)} if ensemble else {}
        with pytest.warns(DeprecationWarning):
            runs.append((emu, emu.run(seeds=1, general_jumps=True, **option)))
    (emu_a, avg), (emu_e, ens) = runs
    D = d**n
    times = emu_a._eval_times_array
    assert len(times) == 5 and len(avg) == len(ens) == 5
    assert len(kets) == 2 and kets[0].shape == (4, NTRAJ, D) and np.array_equal(kets[0], kets[1])
    assert np.array_equal(emu_a.last_mc_jumps, emu_e.last_mc_jumps) and emu_e.last_mc_jumps.sum() > 0
    assert emu_e.last_engine_stats["n_launches"] == emu_a.last_engine_stats["n_launches"]
    ham = _oracle_hamiltonian(emu_a)
    init = np.asarray(emu_a._initial_state, dtype=complex).reshape(1, -1)
    digits = list(range(d))
    worst = np.zeros(5)
    apart = 0.0  # the largest gap between the reference occupations of two digits, in bounds
    for i, t in enumerate(times):
        st = ens.states[i]
        assert isinstance(st, EnsembleState) and st.n_trajectories == NTRAJ and st.shape == (D, D)
        assert list(st.by_digit) == digits
        rho = np.asarray(avg.states[i])
        err = np.abs(st.diag() - np.diag(rho))
        bound = 2 * (NTRAJ + 8) * U53
        worst[0] = max(worst[0], err.max() / bound)
        assert np.all(err <= bound)
        refs = _pair_bounds(rho, n, d, digits, NTRAJ)
        for a in digits:
            for b in digits[a + 1:]:
                apart = max(apart, _ratio(np.abs(refs[a][0] - refs[b][0]), np.maximum(refs[a][2], refs[b][2])))
    assert apart > 100, apart  # swapped digits cannot pass
    for i, t in enumerate(times):
        st = ens.states[i]
        rho = np.asarray(avg.states[i])
        for digit, (occ, corr, b_occ, b_cor) in _pair_bounds(rho, n, d, digits, NTRAJ).items():
            got = st.by_digit[digit]
            for j, (v, want, b) in enumerate(((got["occupation"], occ, b_occ), (got["correlation"], corr, b_cor)), start=1):
                e = np.abs(np.asarray(v, dtype=LD) - want)
                worst[j] = max(worst[j], _ratio(e, b))
                assert np.all(e <= b), (i, digit, j)
            se = got["occupation_stderr"]
            assert np.all(np.isfinite(se)) and np.all(se >= 0) and np.all(se <= 0.5 / np.sqrt(NTRAJ - 1) + 1e-12)
            assert i > 0 or np.all(se == 0)  # every trajectory starts in the same ket
        assert np.array_equal(st.occupation, st.by_digit[0]["occupation"])
        assert np.array_equal(st.correlation, st.by_digit[0]["correlation"])
        assert np.array_equal(st.occupation_stderr, st.by_digit[0]["occupation_stderr"])
        e1, e2, b_e1, b_e2 = _energy_bounds(ham, t, rho, kets[0][i - 1] if i else init)
        for j, (v, want, b) in enumerate(((st.energy, e1, b_e1), (st.energy2, e2, b_e2)), start=3):
            e = np.abs(np.asarray(v, dtype=LD) - want)
            worst[j] = max(worst[j], _ratio(e, b))
            assert e <= b, (i, j)
        assert abs(st.norm2 - 1) < 1e-12 and abs(st.tr() - 1) < 1e-12
    print(f"RATIO general two routes {kind} (diag, occupation, correlation, <H>, <H^2>):",
          " ".join(f"{v:.3e}" for v in worst))
    # sampling: the same Counter under the same seed
    cum = np.cumsum(avg[-1]._weights())
    assert np.max(np.abs(cum - np.cumsum(ens[-1]._weights()))) < 1e-12
    seed = _safe_seed(cum, 500)
    np.random.seed(seed)
    ca = avg.sample_final_state(500)
    np.random.seed(seed)
    ce = ens.sample_final_state(500)
    assert ca == ce and list(ca) == list(ce) and sum(ce.values()) == 500


# ---------------------------------------------------------------------------------------------------------------------
# 2. chunks accumulate
# ---------------------------------------------------------------------------------------------------------------------
def test_two_chunks_accumulate(monkeypatch):
    ntraj = 1100
    kets = _capture_kets(monkeypatch)
    runs = []
    for option in ({}, {"mc_ensemble": True, "mc_ensemble_digits": [0]}):
        emu, d, n = _emulator("xy4", ntraj=ntraj)
        with pytest.warns(DeprecationWarning):
            runs.append((emu, emu.run(seeds=1, general_jumps=True, **option)))
    (emu_a, avg), (emu_e, ens) = runs
    assert [k.shape[1] for k in kets] == [1024, 76, 1024, 76]  # two kets tensors per route
    assert np.array_equal(kets[0], kets[2]) and np.array_equal(kets[1], kets[3])
    assert len(emu_e.last_mc_jumps) == ntraj and np.array_equal(emu_a.last_mc_jumps, emu_e.last_mc_jumps)
    worst = np.zeros(3)
    for i in range(len(emu_a._eval_times_array)):
        st = ens.states[i]
        assert isinstance(st, EnsembleState) and st.n_trajectories == ntraj and list(st.by_digit) == [0]
        rho = np.asarray(avg.states[i])
        err = np.abs(st.diag() - np.diag(rho))
        bound = 2 * (ntraj + 8) * U53
        worst[0] = max(worst[0], err.max() / bound)
        assert np.all(err <= bound)
        occ, corr, b_occ, b_cor = _pair_bounds(rho, n, d, [0], ntraj)[0]
        for j, (v, want, b) in enumerate(((st.occupation, occ, b_occ), (st.correlation, corr, b_cor)), start=1):
            e = np.abs(np.asarray(v, dtype=LD) - want)
            worst[j] = max(worst[j], _ratio(e, b))
            assert np.all(e <= b), (i, j)
        assert abs(st.norm2 - 1) < 1e-12 and abs(st.tr() - 1) < 1e-12
    print("RATIO general two chunks (diag, occupation, correlation):", " ".join(f"{v:.3e}" for v in worst))


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. the capability: runs whose averaged density matrices do not fit
# ---------------------------------------------------------------------------------------------------------------------
def _capability(emu, d, n, ntraj, n_times, seed, digits, label, monkeypatch, **option):
    import time

    D = d**n
    assert n_times * D * D * 16 > (16 << 30)
    assert len(emu._eval_times_array) == n_times and not emu._mc_fast_ok(emu._current_problem)
    with pytest.warns(DeprecationWarning), pytest.raises(MemoryError, match="do not fit"):
        emu.run(seeds=seed, general_jumps=True)  # (a host check: nothing is launched)
    kets = _capture_kets(monkeypatch)
    tic = time.perf_counter()
    with pytest.warns(DeprecationWarning):
        res = emu.run(seeds=seed, general_jumps=True, mc_ensemble=True, **option)
    print(f"TIME {label}: ensemble run {time.perf_counter() - tic:.2f} s, jumps {emu.last_mc_jumps.tolist()}")
    assert len(res) == n_times and all(isinstance(s, EnsembleState) for s in res.states)
    assert len(kets) == 1 and kets[0].shape == (n_times - 1, ntraj, D) and len(emu.last_mc_jumps) == ntraj
    assert emu.last_mc_jumps.sum() > 0  # jumps, not only decay
    for st in res.states:
        assert st.shape == (D, D) and st.n_trajectories == ntraj and list(st.by_digit) == digits
        assert abs(st.tr() - 1) < 1e-12 and abs(st.norm2 - 1) < 1e-12
    assert sum(res.sample_final_state(100).values()) == 100
    worst = np.zeros(3)
    for i in (1, n_times // 2, n_times - 1):
        st = res.states[i]
        p = ket_probabilities(kets[0][i - 1]).sum(axis=0, dtype=LD)  # the trajectory sum of |psi_b|^2
        _, s_abs = ref_diag(kets[0][i - 1][None], np.zeros((1, D)))
        e = np.abs(st.diag().real.astype(LD) - p / ntraj)
        b = (tol_diag(ntraj, s_abs)[0] + U53 * p) / ntraj
        worst[0] = max(worst[0], _ratio(e, b))
        assert np.all(e <= b)
        for digit in digits:
            _, occ, corr, (_, s_occ, s_corr) = ref_pairs_d(p, n, d, digit)
            got = st.by_digit[digit]
            for j, (v, want, s) in enumerate(((got["occupation"], occ, s_occ), (got["correlation"], corr, s_corr)), start=1):
                e = np.abs(v.astype(LD) - want / ntraj)
                b = tol_sum(D + ntraj, s) / ntraj
                worst[j] = max(worst[j], _ratio(e, b))
                assert np.all(e <= b), (i, digit, j)
    print(f"RATIO general capability {label} (diag, occupation, correlation):", " ".join(f"{v:.3e}" for v in worst))


def test_fourteen_xy_atoms_run_only_as_an_ensemble(monkeypatch):
    n, ntraj = 14, 4
    emu = QutipEmulator(_xy_inputs(2, 7, 9.0, 120, 30.0), noise_model=NoiseModel(dephasing_rate=6.0),
                        solver=Solver.MCSOLVER, n_trajectories=ntraj, evaluation_times=[0.024, 0.048, 0.072, 0.096])
    # (the default digit: the one-state "d" of the XY basis (u, d))
    _capability(emu, 2, n, ntraj, 6, 3, [1], "xy 14 atoms", monkeypatch)


def test_nine_three_level_atoms_run_only_as_an_ensemble(monkeypatch):
    """D = 3^9 = 19 683: not a power of two, beyond the persistent kernel (the multi-launch path)."""
    n, ntraj = 9, 3
    emu = QutipEmulator(_all_inputs(3, 3, 6.5, 100, amp=40.0),
                        noise_model=NoiseModel(relaxation_rate=5.0, dephasing_rate=10.0),
                        solver=Solver.MCSOLVER, n_trajectories=ntraj, evaluation_times=[0.03, 0.07])
    assert len(emu._current_problem["eigenbasis"]) == 3
    _capability(emu, 3, n, ntraj, 4, 3, [0, 2], "all 9 atoms", monkeypatch, mc_ensemble_digits=[0, 2])


def test_digits_outside_the_local_dimension_are_refused():
    emu, d, _ = _emulator("all3", ntraj=4)
    with pytest.warns(DeprecationWarning), pytest.raises(ValueError, match="mc_ensemble_digits"):
        emu.run(seeds=1, general_jumps=True, mc_ensemble=True, mc_ensemble_digits=[0, d])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
V2_CASES = {"xy4": ("u", "d"), "all3": ("r", "g", "h"), "nondiag4": ("r", "g")}
NTRAJ_V2 = 100  # (the bounds are those of case 1 at this count)


def _backend_run(kind, cfg_kw, observables, seed, general_jumps, mc_ensemble):
    from pulser_amd.backend import QutipBackendV2, QutipConfig

    inputs, nm, rate, _, _ = CASES[kind]()
    cfg = QutipConfig(observables=observables, noise_model=nm, sampling_rate=rate, **cfg_kw)
    backend = QutipBackendV2(inputs, config=cfg)
    backend._options["seeds"] = 1  # the jump seeds (QutipEmulator.run(seeds=...)): the same trajectories on every run
    if kind == "all3":
        # 9 us sampled every 100 ns: one step per sample interval on every route instead of the default 1-ns cap (9 000
        # steps per run, five runs per case); which kets the routes share does not matter to what is compared
        backend._options["max_step"] = 0.1
    backend.general_jumps, backend.mc_ensemble = general_jumps, mc_ensemble
    np.random.seed(seed)
    return backend, backend.run()


@pytest.mark.parametrize("kind", list(V2_CASES))
def test_backend_serves_the_built_in_observables_from_the_general_ensemble(kind, monkeypatch):
    from pulser_amd.backend import (BitStrings, CorrelationMatrix, Energy, EnergyVariance, Occupation, QutipBackendV2,
                                    QutipConfig, RydState, StateResult)

    assert QutipBackendV2.general_jumps is False and QutipBackendV2.mc_ensemble is False
    ones = V2_CASES[kind]
    _, _, _, d, n = CASES[kind]()
    shots = 200
    bit_one = "r" if d == 3 else None  # (nothing to infer from three eigenstates)
    bits = BitStrings(evaluation_times=[1.0], num_shots=shots, one_state=bit_one)
    occs = [Occupation(one_state=s, tag_suffix=s) for s in ones]
    cors = [CorrelationMatrix(one_state=s, tag_suffix=s) for s in ones]
    energy, variance = Energy(), EnergyVariance()
    obs = [bits] + occs + cors + [energy, variance]
    rel = [0.25, 0.5, 1.0]
    kw = dict(default_evaluation_times=rel, solver=Solver.MCSOLVER, n_trajectories=NTRAJ_V2)
    calls = []
    real_ens, real_jumps = QutipEmulator._solve_general_jumps_ensemble, QutipEmulator._solve_general_jumps
    monkeypatch.setattr(QutipEmulator, "_solve_general_jumps_ensemble",
                        lambda self, *a: calls.append("ensemble") or real_ens(self, *a))
    monkeypatch.setattr(QutipEmulator, "_solve_general_jumps",
                        lambda self, *a: calls.append("jumps") or real_jumps(self, *a))
    # with a StateResult mc_ensemble is without effect: identical results, and the averaged matrices for the bounds
    sr = StateResult()
    (_, ref_on), (b_off, ref_off) = (_backend_run(kind, kw, obs + [sr], 0, True, flag) for flag in (True, False))
    assert calls == ["jumps", "jumps"]
    for tag, values in ref_off.get_tagged_results().items():
        got = ref_on.get_tagged_results()[tag]
        assert len(got) == len(values)
        for a, b in zip(got, values):
            if isinstance(b, RydState):
                assert np.array_equal(np.asarray(a.to_qobj()), np.asarray(b.to_qobj()))
            else:
                assert a == b, tag
    sim = b_off._sim_obj
    eig = tuple(sim._hamiltonian_data.eigenbasis)
    assert eig == ones and len(eig) == d
    T = sim.total_duration_ns
    ham = _oracle_hamiltonian(sim)
    rhos = {t: np.asarray(ref_off.get_result(sr, t).to_qobj()) for t in ref_off.get_result_times(sr)}
    probs = RydState(rhos[1.0], eigenstates=eig).bitstring_probabilities(one_state=bit_one, cutoff=1 / (1000 * shots))
    seed = _safe_seed(np.cumsum(np.array(list(probs.values()))), shots)
    kets = _capture_kets(monkeypatch)
    calls.clear()
    (_, on), (_, off) = (_backend_run(kind, kw, obs, seed, True, flag) for flag in (True, False))
    assert calls == ["ensemble", "jumps"]
    assert len(kets) == 2 and np.array_equal(kets[0], kets[1])
    assert on.get_result(bits, 1.0) == off.get_result(bits, 1.0)
    assert isinstance(on.get_result(bits, 1.0), Counter) and sum(on.get_result(bits, 1.0).values()) == shots
    worst = np.zeros(4)
    for i, t in enumerate(rel):
        rho = rhos[t]
        pairs = _pair_bounds(rho, n, d, list(range(d)), NTRAJ_V2)
        for digit, (o, c) in enumerate(zip(occs, cors)):
            assert on.get_result_times(o) == off.get_result_times(o) == rel
            _, _, b_occ, b_cor = pairs[digit]
            for j, (ob, b) in enumerate(((o, b_occ), (c, b_cor))):
                v_on, v_off = (np.array(r.get_result(ob, t), dtype=float) for r in (on, off))
                # (+ 4 u |value|: each route divides by its norm / trace once, the default route the matrix and the sums)
                tol = b + 4 * U53 * np.abs(v_off)
                e = np.abs(v_on - v_off)
                worst[j] = max(worst[j], _ratio(e, tol))
                assert np.all(e <= tol), (t, digit, j)
        _, _, b_e1, b_e2 = _energy_bounds(ham, t * T / 1000, rho, kets[0][i])
        e_on, e_off = float(on.get_result(energy, t)), float(off.get_result(energy, t))
        var_on, var_off = float(on.get_result(variance, t)), float(off.get_result(variance, t))
        e2_off = var_off + e_off ** 2  # <H^2> of the default route: its scale carries the normalisation term
        tol_e = b_e1 + 4 * U53 * abs(e_off)
        tol_var = (b_e2 + 4 * U53 * abs(e2_off)) + 2 * abs(e_off) * tol_e
        for j, (a, b, tol) in enumerate(((e_on, e_off, tol_e), (var_on, var_off, tol_var)), start=2):
            worst[j] = max(worst[j], _ratio(abs(a - b), tol))
            assert abs(a - b) <= tol, (t, j)
    print(f"RATIO backend general ensemble vs default {kind} (occupation, correlation, <H>, variance):",
          " ".join(f"{v:.3e}" for v in worst))
    # both attributes off: the master-equation fallback, as before
    calls.clear()
    _backend_run(kind, kw, obs, seed, False, False)
    assert calls == [] and QutipBackendV2.general_jumps is False

"""GPU: quantum-jump ensembles without the density matrix - ``ryd_ensemble_diag`` (k_ensemble_diag) against the
longdouble reference of tests/ensemble_ref.py, ``QutipEmulator.run(mc_ensemble=True)`` against the default route on
the SAME trajectories, the run the default route refuses, and ``QutipBackendV2.mc_ensemble``.

Bounds (none fitted to what the kernels give):
 * the kernel: ``tol_diag(n_batch, S_abs)`` per entry, n_batch the trajectories summed onto the value found.
 * two routes, same trajectories: the ensemble diagonal against ``diag`` of the averaged matrix within
   2 (ntraj + 8) u (each route sums ntraj squares <= 1 onto its accumulator and divides once); pair sums within
   ``tol_sum(D + ntraj, S_abs)`` of tests/observe_ref.py once per route; energy moments within ``tol_energy_dm`` of the
   averaged matrix plus the mean over the trajectories of the per-ket ``tol_energy_ket``.
 * sampling: the Counters are EQUAL when no drawn uniform lies within 1e-12 of a boundary of the reference route's
   cumulative weights (the two diagonals differ by ~1e-14); the seed is advanced until the reference route says so.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

from ensemble_ref import ref_diag, tol_diag
from helpers import load_fixture, local_problem, with_anneal_samples
from observe_ref import LD, U53, ket_probabilities, ref_energy_dm, ref_energy_ket, ref_pairs, tol_energy_dm, \
    tol_energy_ket, tol_sum
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd import _lib
from pulser_amd.results import EnsembleState

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _rand(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _check(got, states, start, n_batch):
    """Entry by entry against the reference; prints the worst error over its bound."""
    ref, s_abs = ref_diag(states, start)
    tol = tol_diag(n_batch, s_abs)
    err = np.abs(got.astype(LD) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err > 0, err / tol.astype(LD), 0)
    print(f"RATIO ensemble_diag {states.shape}: {float(np.max(ratio)):.3e}")
    assert np.all(err <= tol)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("dim", [1, 2, 3, 243, 256, 257, 4096 + 1])
def test_kernel_matches_the_reference(dim, B, T):
    from pulser_amd.engine import ensemble_diag

    torch = _torch()
    rng = np.random.default_rng(7 * dim + 3 * B + T)
    x = _rand(rng, T, B, dim)
    dev = torch.from_numpy(x).cuda()
    diag = torch.zeros((T, dim), dtype=torch.float64, device="cuda")
    ensemble_diag(dev, diag)
    _check(diag.cpu().numpy(), x, np.zeros((T, dim)), B)


def test_strided_view_and_a_diag_that_starts_non_zero():
    from pulser_amd.engine import ensemble_diag

    torch = _torch()
    rng = np.random.default_rng(1)
    T, B, dim = 3, 5, 257
    big = _rand(rng, T + 1, B + 2, dim + 31)  # stride_b = dim + 31 > dim, stride_t = (B + 2) (dim + 31): a gap
    dev = torch.from_numpy(big).cuda()
    view = dev[1:, 1:B + 1, 7:7 + dim]
    assert view.stride(1) > dim and view.stride(0) > B * view.stride(1) and not view.is_contiguous()
    start = rng.normal(size=(T, dim))  # either sign: S_abs carries |start|
    diag = torch.from_numpy(start.copy()).cuda()
    ensemble_diag(view, diag)
    _check(diag.cpu().numpy(), big[1:, 1:B + 1, 7:7 + dim], start, B)
    assert np.array_equal(dev.cpu().numpy(), big)  # the states are only read


def test_two_chunks_accumulate_against_one_reference_over_both():
    from pulser_amd.engine import ensemble_diag

    torch = _torch()
    rng = np.random.default_rng(2)
    T, dim = 2, 300
    x = _rand(rng, T, 65 + 19, dim)
    diag = torch.zeros((T, dim), dtype=torch.float64, device="cuda")
    for part in (x[:, :65], x[:, 65:]):
        ensemble_diag(torch.from_numpy(np.ascontiguousarray(part)).cuda(), diag)
    _check(diag.cpu().numpy(), x, np.zeros((T, dim)), x.shape[1])


def test_amplitudes_spanning_1e_minus_160_to_1_in_one_ket():
    """Squares down to 1e-320, far below the smallest normal float64: the bound is relative, so the amplitudes of the
    first case are powers of two (their squares and the sums of a few of them are exact, subnormal or not; what rounds is
    what the bound covers).  The second case has full mantissas over 1e-140 .. 1, where every square is normal."""
    from pulser_amd.engine import ensemble_diag

    torch = _torch()
    rng = np.random.default_rng(3)
    T, B, dim = 2, 3, 533
    expo = -np.arange(dim)  # 2^0 .. 2^-532 = 7.1e-161
    mag = np.ldexp(1.0, expo)
    assert mag[-1] < 1e-160 and mag[-1] ** 2 > 0 and mag[0] == 1.0
    x = mag * rng.choice([-1.0, 1.0], size=(T, B, dim)) + 1j * mag * rng.choice([-1.0, 1.0], size=(T, B, dim))
    x = np.ascontiguousarray(x[:, :, rng.permutation(dim)])
    rich = _rand(rng, T, B, dim) * 10.0 ** rng.uniform(-140, 0, size=(T, B, dim))
    for states in (x, rich):
        diag = torch.zeros((T, dim), dtype=torch.float64, device="cuda")
        ensemble_diag(torch.from_numpy(states).cuda(), diag)
        got = diag.cpu().numpy()
        assert np.all(got > 0)
        _check(got, states, np.zeros((T, dim)), B)


def test_no_times_launches_nothing_and_invalid_arguments_are_refused():
    from pulser_amd.engine import ensemble_diag

    torch = _torch()
    lib = _lib.load()
    x = torch.ones((2, 3, 8), dtype=torch.complex128, device="cuda")
    d = torch.full((2, 8), 5.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    px, pd = x.data_ptr(), d.data_ptr()
    assert lib.ryd_ensemble_diag(px, 0, 3, 24, 8, 8, pd, 0, stream) == 0
    ensemble_diag(x[:0], d[:0])
    for args in ((None, 2, 3, 24, 8, 8, pd), (px, 2, 3, 24, 8, 8, None), (px, 2, 0, 24, 8, 8, pd),
                 (px, 2, -1, 24, 8, 8, pd), (px, 2, 3, 24, 8, 0, pd), (px, 2, 3, 24, 7, 8, pd), (px, 2, 3, 7, 8, 8, pd),
                 (px, -1, 3, 24, 8, 8, pd)):
        assert lib.ryd_ensemble_diag(*args, 0, stream) == -1, args
    torch.cuda.synchronize()
    assert torch.all(d == 5.0)  # nothing was launched
    # the wrapper's own checks
    with pytest.raises(TypeError):
        ensemble_diag(x.to(torch.complex64), d)
    with pytest.raises(TypeError):
        ensemble_diag(x, d.to(torch.float32))
    with pytest.raises(ValueError):
        ensemble_diag(x, d[:, :7])
    with pytest.raises(ValueError):
        ensemble_diag(x, d.t().contiguous().t())
    with pytest.raises(ValueError):
        ensemble_diag(x.cpu(), d)
    with pytest.raises(ValueError):
        ensemble_diag(x[:, :1].expand(2, 3, 8), d)  # stride_b = 0: not [T, B, D] states
    with pytest.raises(ValueError):
        ensemble_diag(x.transpose(1, 2).contiguous().transpose(1, 2), d)  # last axis not contiguous


def test_two_calls_on_the_same_input_are_bitwise_equal():
    from pulser_amd.engine import ensemble_diag

    torch = _torch()
    rng = np.random.default_rng(4)
    dev = torch.from_numpy(_rand(rng, 3, 67, 1000)).cuda()
    start = torch.from_numpy(rng.normal(size=(3, 1000))).cuda()
    outs = []
    for _ in range(2):
        diag = start.clone()
        ensemble_diag(dev, diag)
        outs.append(diag.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the same trajectories on two routes
# ---------------------------------------------------------------------------------------------------------------------
NTRAJ = 300
NOISE = dict(dephasing_rate=0.3, relaxation_rate=0.2)
N4 = 4


def _tri4():
    if "v" not in _tri4.__dict__:
        from oracle import qutip_path as qp

        prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
        prob = with_anneal_samples(prob)
        noiseless = dict(prob)
        noiseless["collapse_ops"] = []
        _tri4.v = (_inputs_from_problem(prob, "ground-rydberg"), qp.build_hamiltonian(noiseless))
    return _tri4.v


def _capture_kets(monkeypatch):
    """Host copies of what every ``Engine.mc_solve`` call stored: [T - 1, B, D] per chunk."""
    from pulser_amd.engine import Engine

    kept = []
    real = Engine.mc_solve

    def capturing(self, state, times, seeds, **kw):
        out = real(self, state, times, seeds, **kw)
        kept.append(out.cpu().numpy())
        return out

    monkeypatch.setattr(Engine, "mc_solve", capturing)
    return kept


def _bounds(ham, n, t_us, rho, kets):
    """(occupation, correlation, <H>, <H^2>) bounds of the ensemble route against the averaged matrix ``rho`` at one
    time, and the reference values: pair sums ``tol_sum(D + ntraj, S_abs)`` once per route; moments ``tol_energy_dm`` of
    ``rho`` plus the mean over the trajectories ``kets`` [B, D] of the per-ket ``tol_energy_ket``."""
    D, ntraj = 2**n, len(kets)
    _, occ, corr, (_, s_occ, s_corr) = ref_pairs(np.real(np.diag(rho)), n)
    e1, e2, s_abs = ref_energy_dm(ham, t_us, rho)
    d1, d2 = tol_energy_dm(n, s_abs)
    k1 = k2 = 0.0
    for x in kets:
        _, _, s_ket, w = ref_energy_ket(ham, t_us, x)
        a, b = tol_energy_ket(x, w, s_ket)
        k1, k2 = k1 + a / ntraj, k2 + b / ntraj
    return (2 * tol_sum(D + ntraj, s_occ), 2 * tol_sum(D + ntraj, s_corr), d1 + k1, d2 + k2), (occ, corr, e1, e2)


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


def _two_routes(monkeypatch):
    inputs, ham = _tri4()
    out = []
    kets = _capture_kets(monkeypatch)
    for option in ({}, {"mc_ensemble": True}):
        emu = QutipEmulator(inputs, noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=NTRAJ,
                            evaluation_times=[0.5, 1.2, 2.0])
        with pytest.warns(DeprecationWarning):
            res = emu.run(seeds=1, **option)
        out.append((emu, res))
    assert len(kets) == 2 and np.array_equal(kets[0], kets[1])  # one chunk each, the same kets bit for bit
    return out[0], out[1], kets[1], ham


def test_same_trajectories_two_routes(monkeypatch):
    (emu_a, avg), (emu_e, ens), kets, ham = _two_routes(monkeypatch)
    times = emu_a._eval_times_array
    assert len(times) == 5 and len(avg) == len(ens) == 5 and kets.shape == (4, NTRAJ, 16)
    assert np.array_equal(emu_a.last_mc_jumps, emu_e.last_mc_jumps) and emu_e.last_mc_jumps.sum() > 0
    assert emu_e.last_engine_stats["n_launches"] == emu_a.last_engine_stats["n_launches"]
    init = np.asarray(emu_a._initial_state, dtype=complex).reshape(1, -1)
    worst = np.zeros(5)
    for i, t in enumerate(times):
        st = ens.states[i]
        assert isinstance(st, EnsembleState) and st.n_trajectories == NTRAJ and st.shape == (16, 16)
        rho = np.asarray(avg.states[i])
        err = np.abs(st.diag() - np.diag(rho))
        bound = 2 * (NTRAJ + 8) * U53
        worst[0] = max(worst[0], err.max() / bound)
        assert np.all(err <= bound)
        x = kets[i - 1] if i else init  # every trajectory starts in the initial ket
        (b_occ, b_cor, b_e1, b_e2), (occ, corr, e1, e2) = _bounds(ham, N4, t, rho, x)
        for j, (got, want, b) in enumerate(((st.occupation, occ, b_occ), (st.correlation, corr, b_cor),
                                            (st.energy, e1, b_e1), (st.energy2, e2, b_e2)), start=1):
            e = np.abs(np.asarray(got, dtype=LD) - want)
            worst[j] = max(worst[j], _ratio(e, b))
            assert np.all(e <= b), (i, j)
        assert abs(st.norm2 - 1) < 1e-12 and abs(st.tr() - 1) < 1e-12
        assert np.all(np.isfinite(st.occupation_stderr)) and np.all(st.occupation_stderr >= 0)
        assert np.all(st.occupation_stderr <= 0.5 / np.sqrt(NTRAJ - 1) + 1e-12)  # a variable in [0, 1]
    assert np.all(ens.states[0].occupation_stderr == 0)  # every trajectory starts in the same ket
    print("RATIO two routes (diag, occupation, correlation, <H>, <H^2>):", " ".join(f"{v:.3e}" for v in worst))
    # sampling: the same Counter under the same seed
    cum = np.cumsum(avg[-1]._weights())
    assert np.max(np.abs(cum - np.cumsum(ens[-1]._weights()))) < 1e-12
    seed = _safe_seed(cum, 500)
    np.random.seed(seed)
    ca = avg.sample_final_state(500)
    np.random.seed(seed)
    ce = ens.sample_final_state(500)
    assert ca == ce and list(ca) == list(ce) and sum(ce.values()) == 500
    assert set(ens[-1].sampling_dist) == set(avg[-1].sampling_dist)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the capability: a run the averaged density matrices do not fit
# ---------------------------------------------------------------------------------------------------------------------
def test_twelve_atoms_seventy_times_run_only_as_an_ensemble(monkeypatch):
    n, ntraj, n_times = 12, 32, 70
    D = 2**n
    assert n_times * D * D * 16 > (16 << 30)
    inputs = _inputs_from_problem(local_problem(n, seed=1, duration=141), "ground-rydberg")
    times = np.linspace(0.0, 0.14, n_times)
    emu = QutipEmulator(inputs, noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=ntraj,
                        evaluation_times=times)
    assert len(emu._eval_times_array) == n_times
    with pytest.warns(DeprecationWarning), pytest.raises(MemoryError, match="do not fit"):
        emu.run(seeds=3)  # (a host check: nothing is launched)
    kets = _capture_kets(monkeypatch)
    with pytest.warns(DeprecationWarning):
        res = emu.run(seeds=3, mc_ensemble=True)
    assert len(res) == n_times and all(isinstance(s, EnsembleState) for s in res.states)
    assert len(kets) == 1 and kets[0].shape == (n_times - 1, ntraj, D) and len(emu.last_mc_jumps) == ntraj
    for st in res.states:
        assert st.shape == (D, D) and st.n_trajectories == ntraj
        assert abs(st.tr() - 1) < 1e-12 and abs(st.norm2 - 1) < 1e-12
        assert np.all(st.occupation >= 0) and np.all(st.occupation <= 1)
        assert np.all(np.isfinite(st.occupation_stderr))
    assert sum(res.sample_final_state(100).values()) == 100
    for i in (1, 35, n_times - 1):
        p = ket_probabilities(kets[0][i - 1]).sum(axis=0, dtype=LD)  # the trajectory sum of |psi_b|^2
        _, occ, corr, (_, s_occ, s_corr) = ref_pairs(p, n)
        st = res.states[i]
        assert np.all(np.abs(st.occupation.astype(LD) - occ / ntraj) <= tol_sum(D + ntraj, s_occ) / ntraj)
        assert np.all(np.abs(st.correlation.astype(LD) - corr / ntraj) <= tol_sum(D + ntraj, s_corr) / ntraj)
        _, s_abs = ref_diag(kets[0][i - 1][None], np.zeros((1, D)))
        assert np.all(np.abs(st.diag().real.astype(LD) - p / ntraj) <= (tol_diag(ntraj, s_abs)[0] + U53 * p) / ntraj)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
def _backend_run(cfg, attribute, seed):
    from pulser_amd.backend import QutipBackendV2

    backend = QutipBackendV2(_tri4()[0], config=cfg)
    backend._options["seeds"] = 1  # the jump seeds (QutipEmulator.run(seeds=...)): the same trajectories on every run
    if attribute:
        backend.mc_ensemble = True
    np.random.seed(seed)
    return backend.run()


def test_backend_serves_the_built_in_observables_from_the_ensemble(monkeypatch):
    from pulser_amd.backend import (BitStrings, CorrelationMatrix, Energy, EnergyVariance, Occupation, QutipBackendV2,
                                    QutipConfig, RydState, StateResult)

    _, ham = _tri4()
    shots = 200
    bits = BitStrings(evaluation_times=[1.0], num_shots=shots)
    obs = [bits, Occupation(), CorrelationMatrix(), Energy(), EnergyVariance()]
    rel = [0.25, 0.5, 1.0]
    kw = dict(default_evaluation_times=rel, noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=NTRAJ)
    # with a StateResult the attribute is without effect: identical results, and the averaged matrices for the bounds
    sr = StateResult()
    with_state = QutipConfig(observables=obs + [sr], **kw)
    ref_on, ref_off = _backend_run(with_state, True, 0), _backend_run(with_state, False, 0)
    for tag, values in ref_off.get_tagged_results().items():
        got = ref_on.get_tagged_results()[tag]
        assert len(got) == len(values)
        for a, b in zip(got, values):
            if isinstance(b, RydState):
                assert np.array_equal(np.asarray(a.to_qobj()), np.asarray(b.to_qobj()))
            else:
                assert a == b, tag
    rhos = {t: np.asarray(ref_off.get_result(sr, t).to_qobj()) for t in ref_off.get_result_times(sr)}
    cutoff = 1 / (1000 * shots)
    probs = RydState(rhos[1.0], eigenstates=("r", "g")).bitstring_probabilities(cutoff=cutoff)
    seed = _safe_seed(np.cumsum(np.array(list(probs.values()))), shots)
    kets = _capture_kets(monkeypatch)
    cfg = QutipConfig(observables=obs, **kw)
    seen = []
    real = QutipEmulator._solve_mc_ensemble
    monkeypatch.setattr(QutipEmulator, "_solve_mc_ensemble",
                        lambda self, *a: seen.append("ensemble") or real(self, *a))
    on, off = _backend_run(cfg, True, seed), _backend_run(cfg, False, seed)
    assert seen == ["ensemble"] and QutipBackendV2.mc_ensemble is False
    assert len(kets) == 2 and np.array_equal(kets[0], kets[1])
    assert on.get_result(bits, 1.0) == off.get_result(bits, 1.0)
    assert isinstance(on.get_result(bits, 1.0), Counter) and sum(on.get_result(bits, 1.0).values()) == shots
    worst = np.zeros(4)
    for i, t in enumerate(rel):
        assert on.get_result_times(obs[1]) == off.get_result_times(obs[1]) == rel
        (b_occ, b_cor, b_e1, b_e2), _ = _bounds(ham, N4, t * 3.1, rhos[t], kets[0][i])
        v_on = [np.array(on.get_result(o, t), dtype=float) for o in obs[1:]]
        v_off = [np.array(off.get_result(o, t), dtype=float) for o in obs[1:]]
        e2_off = v_off[3] + v_off[2] ** 2  # <H^2> of the default route: its scale carries the normalisation term
        # (+ 4 u |value|: each route divides by its norm / trace once, the default route the matrix and the sums)
        tols = [b_occ + 4 * U53 * np.abs(v_off[0]), b_cor + 4 * U53 * np.abs(v_off[1]), b_e1 + 4 * U53 * abs(v_off[2]),
                (b_e2 + 4 * U53 * abs(e2_off)) + 2 * abs(v_off[2]) * (b_e1 + 4 * U53 * abs(v_off[2]))]
        for j in range(4):
            e = np.abs(v_on[j] - v_off[j])
            worst[j] = max(worst[j], _ratio(e, tols[j]))
            assert np.all(e <= tols[j]), (t, j)
    print("RATIO backend ensemble vs default (occupation, correlation, <H>, variance):", " ".join(f"{v:.3e}" for v in worst))

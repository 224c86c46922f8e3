"""GPU: fidelities and expectation values of quantum-jump ensembles from the kets -
``QutipEmulator.run(mc_ensemble=True, mc_ensemble_targets=..., mc_ensemble_operators=...)`` on the two-level and on the
general route, and ``Fidelity`` / ``Expectation`` under ``QutipBackendV2.mc_ensemble``.

References: the longdouble helpers of tests/overlap_ref.py and tests/expect_ref.py on the kets the solver stored
(captured around ``Engine.mc_solve`` / ``GeneralEngine.mc_solve``), and the averaged matrix of the default route on the
SAME trajectories.

Bounds (none fitted to what the code gives), u = 2^-53, n trajectories, per ket b of dimension D:
 * fidelity, the mean of v_b = |z_b|^2 with z_b = <phi|psi_b> from ``overlap_many``: either part of z_b errs by at
   most dz_b = ``tol_z(D, S_abs_b)``, so |delta z_b| <= sqrt(2) dz_b and v_b by dv_b = 2 sqrt(2) |z_b| dz_b + 2 dz_b^2;
   forming v_b in float64 (2 u), summing n of them in any order ((n - 1) u) and dividing once (u) adds (n + 2) u F:

       (1 / n) sum_b dv_b + (n + 2) u F

 * expectation, per real and imaginary part, e_b from ``expect_sparse``: ``tol_expect(nnz, S_abs_b)`` per ket, the
   sum and the division as above:

       (1 / n) sum_b tol_expect(nnz, S_abs_b) + (n + 2) u (1 / n) sum_b |e_b|

 * against the averaged matrix rho of the default route (float64, every entry a sum of n products divided once):
   <phi|rho|phi> and Tr(O rho) in longdouble from it, the bounds above plus the per-entry error (n + 8) u of rho
   weighted by the moduli it is multiplied with: (n + 8) u (sum_i |phi_i|)^2 and (n + 8) u sum_j |v_j|.
 * standard errors, as variances against ``np.var(ddof=1)`` of the longdouble per-ket values.  The code uses
   (sum v^2 - n mean^2) / (n - 1): the rounding of sum v^2 and of n mean^2 at (n + 8) u sum v_b^2, plus
   sum_b 2 |v_b| dv_b for what the values themselves carry, all over n - 1; for an operator v runs over both parts of
   e_b with dv_b = ``tol_expect``.  Every case asserts that at least one reference variance it checks exceeds 1e-6.
 * the V2 backend divides by ``norm2`` where the default route divides rho by its trace: the bounds against rho over
   ``norm2``.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest
import scipy.sparse as sp

from expect_ref import ref_expect, ref_expect_dm, tol_expect, triplets
from helpers import local_problem
from overlap_ref import CLD, LD, U53, ref_overlap, tol_z
from test_gpu_general_mc_ensemble import _capture_kets as _capture_general_kets, _emulator as _general_emulator
from test_gpu_mc_ensemble import NOISE, NTRAJ, _capture_kets, _ratio, _tri4
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd.results import EnsembleState

pytestmark = pytest.mark.gpu

SQRT2 = np.sqrt(LD(2))


def _embed(local, site, n, d=2):
    """``local`` [d, d] on ``site`` of ``n`` qudits (site 0 is the most significant digit), identities elsewhere."""
    return sp.kron(sp.kron(sp.identity(d**site), sp.csr_matrix(local)), sp.identity(d**(n - site - 1))).tocsr()


def _sigma_x_sum(n):
    return sum((_embed(np.array([[0.0, 1.0], [1.0, 0.0]]), q, n) for q in range(n)), sp.csr_matrix((2**n, 2**n))).tocsr()


def _hop(n, d=2):
    """|0><1| on site 0 times |1><0| on site 1: two sites, not Hermitian."""
    up = np.zeros((d, d))
    up[0, 1] = 1.0
    return (_embed(up, 0, n, d) @ _embed(up.T, 1, n, d)).tocsr()


def _random_ket(D, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=D) + 1j * rng.normal(size=D)
    return x / np.linalg.norm(x)


def _reference(kets, targets, operators):
    """Per ket of ``kets`` [B, D], in longdouble: v = |<phi_f|psi>|^2 [B, F] with its bound dv, e = <psi|O_k|psi> [B, K]
    with the bound de of either part."""
    B, D = kets.shape
    z, s_abs = ref_overlap(kets, np.array([np.asarray(t).reshape(-1) for t in targets], dtype=complex).reshape(-1, D))
    dz = tol_z(D, s_abs).astype(LD)
    v = z.real ** 2 + z.imag ** 2
    dv = 2 * SQRT2 * np.abs(z) * dz + 2 * dz ** 2
    e, de = np.zeros((B, len(operators)), dtype=CLD), np.zeros((B, len(operators)), dtype=LD)
    for k, op in enumerate(operators):
        e[:, k], s = ref_expect(op, kets)
        de[:, k] = tol_expect(len(triplets(op)[2]), s)
    return v, dv, e, de


def _check_means(st, n, ref, worst, where):
    """The means of one ``EnsembleState`` against the per-ket reference ``ref`` (over n kets, or over the one every
    trajectory starts in); returns the bounds (fidelity [F], expectation [K]) for the comparison with rho."""
    v, dv, e, de = ref
    fid = v.mean(axis=0, dtype=LD)
    b_fid = dv.mean(axis=0, dtype=LD) + (n + 2) * U53 * fid
    err = np.abs(st.fidelity.astype(LD) - fid)
    worst[0] = max(worst[0], _ratio(err, b_fid))
    assert np.all(err <= b_fid), (where, "fidelity", err, b_fid)
    b_exp = de.mean(axis=0, dtype=LD) + (n + 2) * U53 * np.abs(e).mean(axis=0, dtype=LD)
    mean = e.mean(axis=0, dtype=CLD)
    for got, want in ((st.expectation.real, mean.real), (st.expectation.imag, mean.imag)):
        err = np.abs(got.astype(LD) - want)
        worst[1] = max(worst[1], _ratio(err, b_exp))
        assert np.all(err <= b_exp), (where, "expectation", err, b_exp)
    return b_fid, b_exp


def _check_variances(st, n, ref, worst, where):
    """n stderr^2 of one ``EnsembleState`` against ``np.var(ddof=1)`` of the n per-ket values; returns the largest
    reference variance checked."""
    v, dv, e, de = ref
    assert len(v) == n > 1
    ref_var = np.var(v, axis=0, ddof=1)
    b = ((n + 8) * U53 * (v ** 2).sum(axis=0, dtype=LD) + (2 * v * dv).sum(axis=0, dtype=LD)) / (n - 1)
    err = np.abs(st.fidelity_stderr.astype(LD) ** 2 * n - ref_var)
    worst[2] = max(worst[2], _ratio(err, b))
    assert np.all(err <= b), (where, "fidelity variance", err, b)
    re, im = e.real, e.imag
    ref_exp = np.var(re, axis=0, ddof=1) + np.var(im, axis=0, ddof=1)
    b = ((n + 8) * U53 * ((re ** 2).sum(axis=0, dtype=LD) + (im ** 2).sum(axis=0, dtype=LD))
         + (2 * (np.abs(re) + np.abs(im)) * de).sum(axis=0, dtype=LD)) / (n - 1)
    err = np.abs(st.expectation_stderr.astype(LD) ** 2 * n - ref_exp)
    worst[3] = max(worst[3], _ratio(err, b))
    assert np.all(err <= b), (where, "expectation variance", err, b)
    return max([float(x) for x in ref_var] + [float(x) for x in ref_exp] + [0.0])


def _from_rho(rho, targets, operators):
    """(<phi_f|rho|phi_f> [F], Tr(O_k rho) [K]) in longdouble and the terms the rounding of rho adds per unit (n + 8) u:
    (sum_i |phi_i|)^2 [F] and sum_j |v_j| [K]."""
    r = np.asarray(rho).astype(CLD)
    fid, w_fid = [], []
    for phi in targets:
        phi = np.asarray(phi).reshape(-1).astype(CLD)
        fid.append((np.conj(phi)[:, None] * r * phi[None, :]).sum(dtype=CLD))
        w_fid.append(np.abs(phi).sum(dtype=LD) ** 2)
    exp = [ref_expect_dm(op, rho)[0] for op in operators]
    w_exp = [np.abs(triplets(op)[2]).astype(LD).sum(dtype=LD) for op in operators]
    return np.array(fid, dtype=CLD), np.array(w_fid, dtype=LD), np.array(exp, dtype=CLD), np.array(w_exp, dtype=LD)


def _check_rho(st, n, rho, targets, operators, bounds, worst, where, scale=1.0):
    """One ``EnsembleState`` (its values divided by ``scale``) against the averaged matrix ``rho`` of the default route."""
    fid, w_fid, exp, w_exp = _from_rho(rho, targets, operators)
    b_fid = (bounds[0] + (n + 8) * U53 * w_fid) / scale
    assert np.all(np.abs(fid.imag) <= b_fid)  # (rho is Hermitian as stored or within its rounding)
    err = np.abs(st.fidelity.astype(LD) / scale - fid.real)
    worst[4] = max(worst[4], _ratio(err, b_fid))
    assert np.all(err <= b_fid), (where, "fidelity against rho", err, b_fid)
    b_exp = (bounds[1] + (n + 8) * U53 * w_exp) / scale
    for got, want in ((st.expectation.real, exp.real), (st.expectation.imag, exp.imag)):
        err = np.abs(got.astype(LD) / scale - want)
        worst[5] = max(worst[5], _ratio(err, b_exp))
        assert np.all(err <= b_exp), (where, "expectation against rho", err, b_exp)


def _report(label, worst):
    print(f"RATIO {label} (fidelity, expectation, their variances, fidelity and expectation against rho):",
          " ".join(f"{v:.3e}" for v in worst))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the same trajectories on two routes
# ---------------------------------------------------------------------------------------------------------------------
N4, D4 = 4, 16
TIMES4 = [0.5, 1.2, 2.0]


def _tri4_emulator(ntraj=NTRAJ):
    return QutipEmulator(_tri4()[0], noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=ntraj,
                         evaluation_times=TIMES4)


def test_same_trajectories_two_routes(monkeypatch):
    kets = _capture_kets(monkeypatch)
    init = np.asarray(_tri4_emulator()._initial_state, dtype=complex).reshape(-1)
    basis = np.zeros(D4, dtype=complex)
    basis[0b0101] = 1.0
    targets = [init, _random_ket(D4, 11), basis.reshape(D4, 1)]
    projector = sp.diags((np.arange(D4) % 4 == 1).astype(float)).tocsr()
    operators = [_sigma_x_sum(N4), _hop(N4), projector, sp.csr_matrix((D4, D4))]
    assert operators[3].nnz == 0 and (operators[1] != operators[1].conj().T).nnz > 0
    registered = dict(mc_ensemble_targets=targets, mc_ensemble_operators=operators)
    runs = []
    for option in ({}, {"mc_ensemble": True}):  # (the default route ignores what is registered)
        emu = _tri4_emulator()
        with pytest.warns(DeprecationWarning):
            runs.append((emu, emu.run(seeds=1, **option, **registered)))
    (emu_a, avg), (emu_e, ens) = runs
    assert len(kets) == 2 and kets[0].shape == (4, NTRAJ, D4) and np.array_equal(kets[0], kets[1])
    assert np.array_equal(emu_a.last_mc_jumps, emu_e.last_mc_jumps) and emu_e.last_mc_jumps.sum() > 0
    worst, largest = np.zeros(6), 0.0
    for i in range(5):
        st = ens.states[i]
        assert isinstance(st, EnsembleState) and not isinstance(avg.states[i], EnsembleState)
        assert st.fidelity.shape == st.fidelity_stderr.shape == (3,) and st.fidelity.dtype == np.float64
        assert st.expectation.shape == st.expectation_stderr.shape == (4,) and st.expectation.dtype == np.complex128
        ref = _reference(kets[1][i - 1] if i else init[None], targets, operators)
        bounds = _check_means(st, NTRAJ, ref, worst, i)
        if i:
            largest = max(largest, _check_variances(st, NTRAJ, ref, worst, i))
            assert np.all(np.isfinite(st.fidelity_stderr)) and np.all(np.isfinite(st.expectation_stderr))
        else:  # the initial ket as its own target: a basis ket, so the reference is 1 exactly
            assert ref[0][0, 0] == 1 and abs(st.fidelity[0] - 1) <= bounds[0][0]
        _check_rho(st, NTRAJ, np.asarray(avg.states[i]), targets, operators, bounds, worst, i)
        assert st.expectation[3] == 0 and st.expectation_stderr[3] == 0  # no stored non-zero
    first = ens.states[0]
    assert np.all(first.fidelity_stderr == 0) and np.all(first.expectation_stderr == 0)
    assert largest > 1e-6, largest
    _report("two routes", worst)
    # results.expect serves what was registered, by its non-zeros; the diagonal as before; nothing else
    got = ens.expect([_sigma_x_sum(N4).toarray(), _hop(N4), projector])
    assert got[0].dtype == np.float64 and np.array_equal(got[0], [st.expectation[0].real for st in ens.states])
    assert got[1].dtype == np.complex128 and np.array_equal(got[1], [st.expectation[1] for st in ens.states])
    assert np.array_equal(got[2], [np.sum(projector.diagonal() * st.diag()).real for st in ens.states])
    with pytest.raises(NotImplementedError, match="mc_ensemble_operators"):
        ens.expect([_hop(N4).T.tocsr()])
    with pytest.raises(NotImplementedError, match="mc_ensemble_targets"):
        ens.states[-1].overlap(init)


# ---------------------------------------------------------------------------------------------------------------------
# 2. chunks accumulate
# ---------------------------------------------------------------------------------------------------------------------
def test_two_chunks_accumulate(monkeypatch):
    ntraj = 1027
    kets = _capture_kets(monkeypatch)
    targets, operators = [_random_ket(D4, 12)], [_hop(N4)]
    emu = _tri4_emulator(ntraj)
    with pytest.warns(DeprecationWarning):
        ens = emu.run(seeds=1, mc_ensemble=True, mc_ensemble_targets=targets, mc_ensemble_operators=operators)
    assert [k.shape[1] for k in kets] == [1024, 3] and len(emu.last_mc_jumps) == ntraj
    both = np.concatenate(kets, axis=1)
    worst, largest = np.zeros(6), 0.0
    for i in range(1, 5):
        st = ens.states[i]
        assert st.n_trajectories == ntraj
        ref = _reference(both[i - 1], targets, operators)
        _check_means(st, ntraj, ref, worst, i)
        largest = max(largest, _check_variances(st, ntraj, ref, worst, i))
    assert largest > 1e-6, largest
    _report("two chunks", worst[:4])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the general route: a three-level and an XY register
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all3", "xy4"])
def test_general_route(kind, monkeypatch):
    ntraj = 64
    kets = _capture_general_kets(monkeypatch)
    # (all3: 9 us sampled every 100 ns - one step per sample interval instead of the default 1-ns cap on both routes;
    # which kets the routes share does not matter to what is compared)
    extra = {"max_step": 0.1} if kind == "all3" else {}
    runs = []
    for option in ({}, {"mc_ensemble": True}):
        emu, d, n = _general_emulator(kind, ntraj=ntraj)
        D = d**n
        targets, operators = [_random_ket(D, 13)], [_hop(n, d)]
        with pytest.warns(DeprecationWarning):
            runs.append((emu, emu.run(seeds=1, general_jumps=True, mc_ensemble_targets=targets,
                                      mc_ensemble_operators=operators, **option, **extra)))
    (emu_a, avg), (emu_e, ens) = runs
    assert D == {"all3": 27, "xy4": 16}[kind]
    assert len(kets) == 2 and kets[0].shape == (4, ntraj, D) and np.array_equal(kets[0], kets[1])
    assert np.array_equal(emu_a.last_mc_jumps, emu_e.last_mc_jumps) and emu_e.last_mc_jumps.sum() > 0
    init = np.asarray(emu_a._initial_state, dtype=complex).reshape(-1)
    worst, largest = np.zeros(6), 0.0
    for i in range(5):
        st = ens.states[i]
        assert isinstance(st, EnsembleState) and st.by_digit is not None
        assert st.fidelity.shape == (1,) and st.expectation.shape == (1,)
        ref = _reference(kets[1][i - 1] if i else init[None], targets, operators)
        bounds = _check_means(st, ntraj, ref, worst, i)
        if i:
            largest = max(largest, _check_variances(st, ntraj, ref, worst, i))
        _check_rho(st, ntraj, np.asarray(avg.states[i]), targets, operators, bounds, worst, i)
    assert np.all(ens.states[0].fidelity_stderr == 0) and np.all(ens.states[0].expectation_stderr == 0)
    assert largest > 1e-6, largest
    _report(f"general route {kind}", worst)
    assert np.array_equal(ens.expect([_hop(n, d).toarray()])[0], [st.expectation[0] for st in ens.states])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the capability: a run the averaged density matrices do not fit
# ---------------------------------------------------------------------------------------------------------------------
def test_twelve_atoms_seventy_times_with_a_target_and_an_operator(monkeypatch):
    n, ntraj, n_times = 12, 32, 70
    D = 2**n
    inputs = _inputs_from_problem(local_problem(n, seed=1, duration=141), "ground-rydberg")
    emu = QutipEmulator(inputs, noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=ntraj,
                        evaluation_times=np.linspace(0.0, 0.14, n_times))
    assert len(emu._eval_times_array) == n_times and n_times * D * D * 16 > (16 << 30)
    antiferro = np.zeros(D, dtype=complex)
    antiferro[int("01" * (n // 2), 2)] = 1.0  # |rgrg...> in the eigenbasis (r, g)
    targets, operators = [antiferro], [_sigma_x_sum(n)]
    registered = dict(mc_ensemble_targets=targets, mc_ensemble_operators=operators)
    with pytest.warns(DeprecationWarning), pytest.raises(MemoryError, match="do not fit"):
        emu.run(seeds=3, **registered)  # (a host check: nothing is launched)
    kets = _capture_kets(monkeypatch)
    with pytest.warns(DeprecationWarning):
        res = emu.run(seeds=3, mc_ensemble=True, **registered)
    assert len(res) == n_times and all(isinstance(s, EnsembleState) for s in res.states)
    assert len(kets) == 1 and kets[0].shape == (n_times - 1, ntraj, D)
    worst, largest = np.zeros(6), 0.0
    for i in (1, 35, n_times - 1):
        ref = _reference(kets[0][i - 1], targets, operators)
        _check_means(res.states[i], ntraj, ref, worst, i)
        largest = max(largest, _check_variances(res.states[i], ntraj, ref, worst, i))
    assert largest > 1e-6, largest
    _report("capability 12 atoms", worst[:4])
    sx = res.expect([_sigma_x_sum(n)])[0]
    assert sx.shape == (n_times,) and sx.dtype == np.float64 and sx[35] == res.states[35].expectation[0].real


# ---------------------------------------------------------------------------------------------------------------------
# 5. the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
def _backend(cfg, attribute, seed):
    from pulser_amd.backend import QutipBackendV2

    backend = QutipBackendV2(_tri4()[0], config=cfg)
    backend._options["seeds"] = 1  # the jump seeds (QutipEmulator.run(seeds=...)): the same trajectories on every run
    backend.mc_ensemble = attribute
    np.random.seed(seed)
    return backend.run()


def test_backend_serves_fidelity_and_expectation_from_the_ensemble(monkeypatch):
    from pulser_amd import engine
    from pulser_amd.backend import (BitStrings, Expectation, Fidelity, Occupation, QutipConfig, RydOperator, RydState,
                                    StateResult)

    eig = ("r", "g")
    phi = _random_ket(D4, 14)
    dense = _hop(N4).toarray() + np.diag(np.arange(D4, dtype=float))
    fid = Fidelity(RydState(phi, eigenstates=eig))
    exp_op = Expectation(RydOperator(_sigma_x_sum(N4), eigenstates=eig))
    exp_dense = Expectation(dense, tag_suffix="dense")
    occ, bits = Occupation(), BitStrings(evaluation_times=[1.0], num_shots=100)
    obs = [fid, exp_op, exp_dense, occ, bits]
    rel = [0.25, 0.5, 1.0]
    kw = dict(default_evaluation_times=rel, noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=NTRAJ)
    cfg = QutipConfig(observables=obs, **kw)
    kets = _capture_kets(monkeypatch)
    # the default route first: its averaged matrices are the reference (a StateResult keeps the route and shows them)
    sr = StateResult()
    off = _backend(QutipConfig(observables=obs + [sr], **kw), False, 0)
    rhos = {t: np.asarray(off.get_result(sr, t).to_qobj()) for t in rel}
    # ... then the ensemble route, which must never form an outer product
    states = []
    real = QutipEmulator._solve_mc_ensemble

    def solve(self, *a):
        out = real(self, *a)
        states.extend(out.states)
        return out

    def never(*a, **k):
        raise AssertionError("the ensemble route formed an outer product")

    with monkeypatch.context() as m:
        m.setattr(QutipEmulator, "_solve_mc_ensemble", solve)
        m.setattr(engine.Engine, "outer_accumulate", never)
        m.setattr(engine, "outer_accumulate", never)
        on = _backend(cfg, True, 0)
    assert len(kets) == 2 and np.array_equal(kets[0], kets[1])
    assert len(states) == len(rel) + 1 and all(isinstance(s, EnsembleState) for s in states)
    assert states[-1].fidelity.shape == (1,) and states[-1].expectation.shape == (2,)
    assert isinstance(on.get_result(bits, 1.0), Counter) and sum(on.get_result(bits, 1.0).values()) == 100
    assert len(on.get_result(occ, 1.0)) == N4
    operators = [_sigma_x_sum(N4), dense]
    worst = np.zeros(6)
    for i, t in enumerate(rel):
        st = states[i + 1]
        ref = _reference(kets[1][i], [phi], operators)
        bounds = _check_means(st, NTRAJ, ref, worst, t)
        v_fid, v_op, v_dense = on.get_result(fid, t), on.get_result(exp_op, t), on.get_result(exp_dense, t)
        assert isinstance(v_fid, float) and v_fid == st.fidelity[0] / st.norm2
        assert complex(v_op) == st.expectation[0] / st.norm2 and complex(v_dense) == st.expectation[1] / st.norm2
        # the default route hands out rho over its trace norm: the ensemble's values over norm2 against it ...
        rho = rhos[t]
        _check_rho(st, NTRAJ, rho, [phi], operators, bounds, worst, t, scale=st.norm2)
        # ... and the two backends' results against each other
        fid_rho, w_fid, exp_rho, w_exp = _from_rho(rho, [phi], operators)
        b_fid = (bounds[0] + (NTRAJ + 8) * U53 * w_fid) / st.norm2
        b_exp = (bounds[1] + (NTRAJ + 8) * U53 * w_exp) / st.norm2
        err = abs(v_fid - float(off.get_result(fid, t)))
        worst[4] = max(worst[4], _ratio(err, b_fid[0]))
        assert err <= b_fid[0], (t, err, b_fid)
        for k, o in enumerate((exp_op, exp_dense)):
            d = complex(on.get_result(o, t)) - complex(off.get_result(o, t))
            err = max(abs(d.real), abs(d.imag))
            worst[5] = max(worst[5], _ratio(err, b_exp[k]))
            assert err <= b_exp[k], (t, k, err, b_exp)
    _report("backend ensemble vs default", worst)
    # a density-matrix target: the default route, as before
    calls = []
    real_avg = QutipEmulator._solve_mc_average
    monkeypatch.setattr(QutipEmulator, "_solve_mc_average", lambda self, *a: calls.append("average") or real_avg(self, *a))
    monkeypatch.setattr(QutipEmulator, "_solve_mc_ensemble", lambda self, *a: calls.append("ensemble") or real(self, *a))
    mixed = Fidelity(RydState(np.outer(phi, phi.conj()) * 0.5 + np.eye(D4) / (2 * D4), eigenstates=eig))
    res = _backend(QutipConfig(observables=[mixed, exp_op, occ], **kw), True, 0)
    assert calls == ["average"]
    assert all(0 < float(res.get_result(mixed, t)) <= 1 for t in rel)
    for t in rel:  # (the same matrices as the first run: the same values)
        assert complex(res.get_result(exp_op, t)) == complex(off.get_result(exp_op, t))

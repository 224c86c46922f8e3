"""CPU: the host side of quantum-jump ensembles without the density matrix (``run(mc_ensemble=True)``) - the
``ryd_ensemble_diag`` declaration, binding and export; ``EnsembleState`` built from arrays (sampling equal to that of a
density matrix with the same diagonal, the refusals, ``expect``); the emulator's routing with and without the option;
the predicate and the option hand-over of ``QutipBackendV2.mc_ensemble``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import load_fixture, with_anneal_samples
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd import _lib
from pulser_amd.backend import (BitStrings, CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance, Expectation,
                                Fidelity, Occupation, QutipBackendV2, QutipConfig, RydState, StateResult as StateObservable,
                                _mc_ensemble_route)
from pulser_amd.results import CoherentResults, DeviceState, EnsembleState, QState, StateResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["const void* states_dev", "int32_t n_times", "int32_t n_batch", "int64_t stride_t", "int64_t stride_b",
             "int64_t dim", "double* diag_dev", "int32_t device", "void* stream"]


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_ensemble_diag\(([^;]*)\);", header)
    assert m, "ryd_ensemble_diag is not declared in include/rydemu.h"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split(",")]
    assert args == PROTOTYPE, args
    restype, argtypes = _lib.SYMBOLS["ryd_ensemble_diag"]
    want = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want
    # (loading the library needs no device)
    assert hasattr(_lib.load(), "ryd_ensemble_diag")
    assert _lib.RYD_ABI_VERSION == 1 and re.search(r"#define\s+RYD_ABI_VERSION\s+1\b", header)


def test_abi_rejects_bad_arguments_without_a_device():
    """Every RYD_ERR_INVALID case is decided before the device is touched (test_gpu_mc_ensemble repeats them with real
    pointers)."""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data
    for args in ((None, 1, 1, 4, 4, 4, p), (p, 1, 1, 4, 4, 4, None), (p, 1, 0, 4, 4, 4, p), (p, 1, -3, 4, 4, 4, p),
                 (p, 1, 1, 4, 4, 0, p), (p, 1, 1, 4, 4, -1, p), (p, 1, 2, 4, 3, 4, p), (p, 2, 1, 3, 4, 4, p),
                 (p, -1, 1, 4, 4, 4, p), (None, 0, 1, 4, 4, 4, p)):
        assert lib.ryd_ensemble_diag(*args, 0, None) == -1, args  # RYD_ERR_INVALID
        assert "ensemble_diag" in lib.ryd_last_error().decode()
    assert lib.ryd_ensemble_diag(p, 0, 1, 4, 4, 4, p, 0, None) == 0  # n_times = 0: nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------------------------------
# EnsembleState from arrays
# ---------------------------------------------------------------------------------------------------------------------
N = 4
QIDS = tuple(f"q{k}" for k in range(N))
NTRAJ = 7


def _ensemble(seed=0, n=N, ntraj=NTRAJ):
    rng = np.random.default_rng(seed)
    kets = rng.normal(size=(ntraj, 2**n)) + 1j * rng.normal(size=(ntraj, 2**n))
    kets /= np.linalg.norm(kets, axis=1)[:, None]
    diag_sum = (np.abs(kets) ** 2).sum(axis=0)
    rho = np.einsum("bi,bj->ij", kets, kets.conj()) / ntraj
    np.fill_diagonal(rho, diag_sum / ntraj)  # the same diagonal, bit for bit
    st = EnsembleState(diag_sum, ntraj, occupation=np.full(n, 0.5), correlation=np.full((n, n), 0.25), energy=1.5,
                       energy2=4.0, norm2=1.0, occupation_stderr=np.full(n, 0.1))
    return st, rho


def test_ensemble_state_is_a_diagonal_only_density_matrix():
    st, rho = _ensemble()
    assert isinstance(st, DeviceState) and st.isket is False and st.isoper is True and st.shape == (16, 16)
    assert st.n_trajectories == NTRAJ and st.device_tensor is None
    assert st.diag().dtype == np.complex128 and np.array_equal(st.diag(), np.diag(rho))
    assert st.tr() == complex(np.sum(np.diag(rho))) and abs(st.tr() - 1) < 1e-14
    assert st.occupation.shape == (N,) and st.correlation.shape == (N, N) and st.occupation_stderr.shape == (N,)
    assert (st.energy, st.energy2, st.norm2) == (1.5, 4.0, 1.0)
    assert "n_trajectories=7" in repr(st)


@pytest.mark.parametrize("call", [lambda s: s.full(), lambda s: np.asarray(s), lambda s: s.copy(), lambda s: s.dag(),
                                  lambda s: s.norm(), lambda s: s.unit(), lambda s: s.overlap(np.ones(16))],
                         ids=["full", "asarray", "copy", "dag", "norm", "unit", "overlap"])
def test_whatever_needs_the_matrix_is_refused(call):
    st, _ = _ensemble()
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        call(st)


@pytest.mark.parametrize("basis,matching", [("ground-rydberg", True), ("digital", True), ("ground-rydberg", False)])
def test_weights_and_samples_equal_those_of_the_density_matrix(basis, matching):
    st, rho = _ensemble(1)
    a = StateResult(QIDS, basis, st, matching)
    b = StateResult(QIDS, basis, QState(rho), matching)
    assert np.array_equal(a._weights(), b._weights())
    assert a.sampling_dist == b.sampling_dist
    np.random.seed(5)
    sa = a.get_samples(400)
    np.random.seed(5)
    sb = b.get_samples(400)
    assert sa == sb and list(sa) == list(sb) and sum(sa.values()) == 400


def _coherent(states, meas_errors=None):
    rs = [StateResult(QIDS, "ground-rydberg", s, True, evaluation_time=t) for s, t in zip(states, (0.0, 1.0))]
    return CoherentResults(rs, N, "ground-rydberg", np.array([0.0, 0.1]), "ground-rydberg", meas_errors)


@pytest.mark.parametrize("errors", [None, {"epsilon": 0.05, "epsilon_prime": 0.1}])
def test_sample_state_with_spam_errors_equals_the_density_matrix_route(errors):
    pairs = [_ensemble(2), _ensemble(3)]
    ens = _coherent([p[0] for p in pairs], errors)
    dms = _coherent([QState(p[1]) for p in pairs], errors)
    for draw in (lambda r: r.sample_final_state(300), lambda r: r.sample_state(0.0, 200), lambda r: r[1].get_samples(50)):
        np.random.seed(11)
        got = draw(ens)
        np.random.seed(11)
        want = draw(dms)
        assert got == want and list(got) == list(want)
    assert ens[1].sampling_dist == dms[1].sampling_dist


def test_ryd_state_samples_from_the_diagonal():
    st, rho = _ensemble(4)
    a = RydState(st, eigenstates=("r", "g"))
    b = RydState(QState(rho), eigenstates=("r", "g"))
    assert a.n_qudits == b.n_qudits == N and a.probabilities() == b.probabilities()
    for kw in ({}, {"p_false_pos": 0.02, "p_false_neg": 0.07}):
        np.random.seed(3)
        sa = a.sample(num_shots=250, **kw)
        np.random.seed(3)
        sb = b.sample(num_shots=250, **kw)
        assert sa == sb and list(sa) == list(sb)


def test_expect_serves_diagonal_operators_and_refuses_the_rest():
    import scipy.sparse as sp

    pairs = [_ensemble(5), _ensemble(6)]
    ens = _coherent([p[0] for p in pairs])
    dms = _coherent([QState(p[1]) for p in pairs])
    d = np.arange(16, dtype=float)
    for op in (np.diag(d), sp.diags(d).tocsr(), np.diag(d + 0.5j)):
        got, want = ens.expect([op])[0], dms.expect([op])[0]
        assert got.dtype == want.dtype and np.allclose(got, want, rtol=0, atol=1e-13)
    off = np.diag(d)
    off[0, 1] = off[1, 0] = 1e-300  # (exactly diagonal or not at all)
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        ens.expect([off])
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        ens.states[0].full()


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
def _tri4_inputs():
    prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
    return _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")


class _EngineReached(Exception):
    pass


def _routes(emu, monkeypatch, prob=None, **solve_kw):
    """Where ``_solve_batch`` goes for each option dict: "average", "ensemble", "general" or ("engine", mode)."""
    from pulser_amd import engine

    calls = []
    monkeypatch.setattr(emu, "_solve_mc_average", lambda p, ntraj, options: calls.append(("average", ntraj)) or "avg")
    monkeypatch.setattr(emu, "_solve_mc_ensemble", lambda p, ntraj, options: calls.append(("ensemble", ntraj)) or "ens")
    monkeypatch.setattr(emu, "_solve_general", lambda probs, mode, options: calls.append(("general", mode)) or ["gen"])

    def no_engine(tables, mode="sesolve", **kw):
        calls.append(("engine", mode))
        raise _EngineReached

    monkeypatch.setattr(engine, "Engine", no_engine)
    prob = prob or emu._current_problem
    out = {}
    for name, options in (("none", {}), ("off", {"mc_ensemble": False}), ("on", {"mc_ensemble": True})):
        calls.clear()
        try:
            emu._solve_batch([prob], False, dict(options), **solve_kw)
        except _EngineReached:
            pass
        assert len(calls) == 1, calls
        out[name] = calls[0]
    return out


@pytest.mark.parametrize("solver", [Solver.MCSOLVER, Solver.DEFAULT, Solver.MESOLVER])
def test_option_reaches_the_ensemble_solve_only_for_the_deterministic_jump_run(solver, monkeypatch):
    emu = QutipEmulator(_tri4_inputs(), noise_model=NoiseModel(dephasing_rate=0.3, relaxation_rate=0.2), solver=solver,
                        n_trajectories=12, evaluation_times="Minimal")
    got = _routes(emu, monkeypatch, mc_ntraj=12)
    if solver == Solver.MCSOLVER:
        assert emu._mc_fast_ok(emu._current_problem)
        assert got == {"none": ("average", 12), "off": ("average", 12), "on": ("ensemble", 12)}
    else:  # deterministic noise without the jump solver: the master equation, with or without the option
        assert got == {k: ("engine", "mesolve") for k in ("none", "off", "on")}


def test_option_changes_nothing_for_one_trajectory_per_noise_draw(monkeypatch):
    emu = QutipEmulator(_tri4_inputs(), noise_model=NoiseModel(dephasing_rate=0.3, relaxation_rate=0.2),
                        solver=Solver.MCSOLVER, n_trajectories=12, evaluation_times="Minimal")
    got = _routes(emu, monkeypatch, mc_ntraj=None)  # what the noisy runs pass: kets, one per batch entry
    assert got == {k: ("engine", "mcsolve") for k in ("none", "off", "on")}


def test_option_changes_nothing_without_collapse_operators_or_off_the_tuned_path(monkeypatch):
    emu = QutipEmulator(_tri4_inputs(), solver=Solver.MCSOLVER, evaluation_times="Minimal")
    assert _routes(emu, monkeypatch, mc_ntraj=1) == {k: ("engine", "sesolve") for k in ("none", "off", "on")}
    from pulser_amd.hamiltonian_data import SequenceInputs

    prob, _ = load_fixture("noisy_xy_0.npz")
    xy = QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), sampling_rate=0.1,
                       noise_model=NoiseModel(dephasing_rate=0.5), solver=Solver.MCSOLVER, n_trajectories=4)
    assert not xy._mc_fast_ok(xy._current_problem)
    assert _routes(xy, monkeypatch, mc_ntraj=4) == {k: ("general", "mesolve") for k in ("none", "off", "on")}


def test_run_docstring_documents_the_option():
    assert "mc_ensemble=True" in QutipEmulator.run.__doc__ and "EnsembleState" in QutipEmulator.run.__doc__


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
DETERMINISTIC = dict(noise_model=NoiseModel(dephasing_rate=0.3, relaxation_rate=0.2), solver=Solver.MCSOLVER,
                     n_trajectories=12)
SERVED = lambda: [BitStrings(num_shots=10), Occupation(), CorrelationMatrix(), Energy(), EnergySecondMoment(),  # noqa: E731
                  EnergyVariance()]


def _sim(cfg, inputs=None):
    return QutipBackendV2(inputs or _tri4_inputs(), config=cfg)._sim_obj


def test_attribute_is_off_on_the_class_and_the_config_has_no_key_for_it():
    assert QutipBackendV2.mc_ensemble is False
    assert "mc_ensemble" not in QutipConfig._expected_kwargs()


def test_predicate_opens_for_the_deterministic_jump_run_with_served_observables():
    cfg = QutipConfig(observables=SERVED(), **DETERMINISTIC)
    assert _mc_ensemble_route(_sim(cfg), cfg) is True
    for one in SERVED():
        cfg = QutipConfig(observables=[one], **DETERMINISTIC)
        assert _mc_ensemble_route(_sim(cfg), cfg) is True


def test_predicate_turns_the_route_down_for_each_disqualifier():
    target = RydState.from_state_amplitudes(eigenstates=("r", "g"), amplitudes={"gggg": 1.0})
    for extra in (StateObservable(), Fidelity(target), Expectation(np.eye(16))):
        cfg = QutipConfig(observables=SERVED() + [extra], **DETERMINISTIC)
        assert _mc_ensemble_route(_sim(cfg), cfg) is False, extra

    class MyOccupation(Occupation):  # a subclass may read anything of the state
        pass

    cfg = QutipConfig(observables=[MyOccupation()], **DETERMINISTIC)
    assert _mc_ensemble_route(_sim(cfg), cfg) is False
    cfg = QutipConfig(observables=SERVED(), callbacks=[lambda **kw: None], **DETERMINISTIC)
    assert _mc_ensemble_route(_sim(cfg), cfg) is False
    # the solver: deterministic noise takes the master equation unless the jump solver is asked for; no noise, no jumps
    for kw in (dict(DETERMINISTIC, solver=Solver.DEFAULT), dict(DETERMINISTIC, solver=Solver.MESOLVER),
               dict(solver=Solver.MCSOLVER)):
        cfg = QutipConfig(observables=SERVED(), **kw)
        assert _mc_ensemble_route(_sim(cfg), cfg) is False, kw
    # stochastic noise: one jump trajectory per noise draw, already kets
    np.random.seed(0)
    cfg = QutipConfig(observables=SERVED(), noise_model=NoiseModel(dephasing_rate=0.3, amp_sigma=0.05),
                      n_trajectories=3)
    sim = _sim(cfg)
    assert sim._solver_mode(sim._current_problem) == "mcsolve" and _mc_ensemble_route(sim, cfg) is False
    # a problem the tuned jump kernels do not take
    cfg = QutipConfig(observables=SERVED(), **DETERMINISTIC)
    sim = _sim(cfg)
    sim._mc_fast_ok = lambda problem: False
    assert _mc_ensemble_route(sim, cfg) is False


class _StubEngine:
    def stats(self):
        return {}

    def close(self):
        pass


@pytest.mark.parametrize("attribute,extra,expected", [(False, [], False), (True, [], True), (True, ["state"], False)])
def test_backend_hands_the_option_and_its_own_observer_to_the_solve(attribute, extra, expected, monkeypatch):
    from pulser_amd import engine

    stub = _StubEngine()
    monkeypatch.setattr(engine.Engine, "from_problems", classmethod(lambda cls, problems, mode=None, **kw: stub))
    seen = {}

    class _Solved(Exception):
        pass

    def run(self, progress_bar=False, print_progress=False, **options):
        seen.update(options)
        raise _Solved

    monkeypatch.setattr(QutipEmulator, "run", run)
    cfg = QutipConfig(observables=SERVED() + [StateObservable() for _ in extra], **DETERMINISTIC)
    backend = QutipBackendV2(_tri4_inputs(), config=cfg)
    if attribute:
        backend.mc_ensemble = True
    with pytest.raises(_Solved):
        backend.run()
    assert QutipBackendV2.mc_ensemble is False  # (set on the instance only)
    if expected:
        assert seen.get("mc_ensemble") is True and seen.get("mc_ensemble_observer") is stub
    else:
        assert "mc_ensemble" not in seen and "mc_ensemble_observer" not in seen

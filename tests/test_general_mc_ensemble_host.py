"""CPU: the host side of quantum-jump ensembles of multi-level and XY registers (``run(general_jumps=True,
mc_ensemble=True)``) - ``EnsembleState(by_digit=...)``, the sampling weights of d = 3 and d = 4 ensembles, the
emulator's routing and its ``mc_ensemble_digits`` check, the predicate and the option hand-over of
``QutipBackendV2.general_jumps``."""
import numpy as np
import pytest

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd import problem as P
from pulser_amd.backend import (BitStrings, CorrelationMatrix, Energy, EnergyVariance, Occupation, QutipBackendV2,
                                QutipConfig, StateResult as StateObservable, _mc_ensemble_route)
from pulser_amd.results import EnsembleState, QState, StateResult


def _xy_inputs(rows=2, cols=2, spacing=8.0, dur=500, amp=8.0):
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    n = rows * cols
    coords = P.register_coords(P.square_rect(rows, cols), spacing)
    t = np.arange(dur)
    ch = ChannelInput("mw", "Global", "XY", amp * np.sin(np.pi * t / dur) ** 2, np.full(dur, -2.0), np.zeros(dur),
                      [Slot(0, dur, tuple(range(n)))])
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), [ch], 5420158.53,
                          interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))


# ---------------------------------------------------------------------------------------------------------------------
# EnsembleState(by_digit=...)
# ---------------------------------------------------------------------------------------------------------------------
def _pairs(n, value):
    return {"occupation": np.full(n, value), "correlation": np.full((n, n), value / 2),
            "occupation_stderr": np.full(n, value / 10)}


def test_by_digit_exposes_every_digit_and_the_first_one_as_the_plain_attributes():
    n = 2
    by = {2: _pairs(n, 0.25), 0: _pairs(n, 0.5)}
    st = EnsembleState(np.full(9, 5.0 / 9), 5, energy=1.5, energy2=4.0, norm2=1.0, by_digit=by)
    assert list(st.by_digit) == [2, 0]  # the order asked for: the first digit leads
    for name in ("occupation", "correlation", "occupation_stderr"):
        assert np.array_equal(getattr(st, name), by[2][name]) and getattr(st, name).dtype == np.float64
        assert np.array_equal(st.by_digit[0][name], by[0][name])
    assert set(st.by_digit[0]) == {"occupation", "correlation", "occupation_stderr"}
    assert st.shape == (9, 9) and st.n_trajectories == 5 and abs(st.tr() - 1) < 1e-15
    assert (st.energy, st.energy2, st.norm2) == (1.5, 4.0, 1.0)
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        st.full()
    with pytest.raises(ValueError):
        EnsembleState(np.ones(9), 5, energy=0.0, energy2=0.0, norm2=1.0, by_digit={})


def test_without_by_digit_the_object_is_unchanged():
    n = 3
    p = _pairs(n, 0.5)
    st = EnsembleState(np.ones(8), 8, energy=1.0, energy2=2.0, norm2=1.0, **p)
    assert st.by_digit is None
    for name, v in p.items():
        assert np.array_equal(getattr(st, name), v)
    assert np.array_equal(st.diag(), np.full(8, 0.125 + 0j)) and st.shape == (8, 8)
    with pytest.raises(TypeError):  # the pair sums come from somewhere: by_digit or the three keywords
        EnsembleState(np.ones(8), 8, energy=1.0, energy2=2.0, norm2=1.0, occupation=p["occupation"])


@pytest.mark.parametrize("d,basis,matching", [(3, "ground-rydberg", False), (3, "digital", False),
                                              (3, "ground-rydberg", True), (4, "ground-rydberg", False),
                                              (4, "digital", True), (3, "XY", True)])
def test_weights_of_multi_level_ensembles_equal_those_of_a_density_matrix_with_the_same_diagonal(d, basis, matching):
    n, ntraj = 3, 7
    rng = np.random.default_rng(10 * d + len(basis))
    kets = rng.normal(size=(ntraj, d**n)) + 1j * rng.normal(size=(ntraj, d**n))
    kets /= np.linalg.norm(kets, axis=1)[:, None]
    diag_sum = (np.abs(kets) ** 2).sum(axis=0)
    rho = np.einsum("bi,bj->ij", kets, kets.conj()) / ntraj
    np.fill_diagonal(rho, diag_sum / ntraj)
    st = EnsembleState(diag_sum, ntraj, energy=0.0, energy2=0.0, norm2=1.0, by_digit={0: _pairs(n, 0.5)})
    qids = tuple(f"q{k}" for k in range(n))
    a = StateResult(qids, basis, st, matching)._weights()
    b = StateResult(qids, basis, QState(rho), matching)._weights()
    assert a.shape == b.shape == (2**n,) and abs(a.sum() - 1) < 1e-15
    assert np.max(np.abs(a - b)) <= 4 * np.spacing(np.max(b))


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
def _xy_emulator(**kw):
    return QutipEmulator(_xy_inputs(), sampling_rate=0.1, noise_model=NoiseModel(dephasing_rate=3.0),
                         solver=Solver.MCSOLVER, n_trajectories=12, evaluation_times="Minimal", **kw)


def test_both_options_and_a_trajectory_count_reach_the_general_ensemble_solve(monkeypatch):
    emu = _xy_emulator()
    prob = emu._current_problem
    assert emu._solver_mode(prob) == "mcsolve" and not emu._mc_fast_ok(prob)
    calls = []
    monkeypatch.setattr(emu, "_solve_general_jumps_ensemble", lambda p, ntraj, o: calls.append(("ensemble", ntraj)) or "e")
    monkeypatch.setattr(emu, "_solve_general_jumps", lambda ps, o, ntraj: calls.append(("jumps", ntraj)) or ["j"])
    monkeypatch.setattr(emu, "_solve_general", lambda ps, mode, o: calls.append(("general", mode)) or ["g"])
    monkeypatch.setattr(emu, "_solve_mc_ensemble", lambda p, ntraj, o: calls.append(("two-level", ntraj)) or "t")
    want = [({"general_jumps": True, "mc_ensemble": True}, 12, ("ensemble", 12)),
            ({"general_jumps": True, "mc_ensemble": True}, None, ("jumps", None)),  # the noisy runs: already kets
            ({"general_jumps": True, "mc_ensemble": False}, 12, ("jumps", 12)),
            ({"general_jumps": True}, 12, ("jumps", 12)),
            ({"mc_ensemble": True}, 12, ("general", "mesolve")),
            ({}, 12, ("general", "mesolve"))]
    for options, ntraj, route in want:
        calls.clear()
        emu._solve_batch([prob], False, dict(options), mc_ntraj=ntraj)
        assert calls == [route], (options, ntraj)


@pytest.mark.parametrize("digits", [[2], [0, -1], [], range(1, 3)])
def test_digits_outside_the_local_dimension_are_refused_before_anything_is_launched(digits):
    emu = _xy_emulator()
    with pytest.warns(DeprecationWarning), pytest.raises(ValueError, match="mc_ensemble_digits"):
        emu.run(seeds=1, general_jumps=True, mc_ensemble=True, mc_ensemble_digits=digits)


def test_run_docstring_documents_the_general_route():
    doc = QutipEmulator.run.__doc__
    assert "mc_ensemble_digits" in doc and "by_digit" in doc and "nan" in doc


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
DETERMINISTIC = dict(noise_model=NoiseModel(dephasing_rate=3.0), solver=Solver.MCSOLVER, n_trajectories=12,
                     sampling_rate=0.1)
SERVED = lambda: [BitStrings(num_shots=10), Occupation(one_state="u"), CorrelationMatrix(), Energy(),  # noqa: E731
                  EnergyVariance()]


def test_attribute_is_off_on_the_class_and_the_config_has_no_key_for_it():
    assert QutipBackendV2.general_jumps is False
    assert "general_jumps" not in QutipConfig._expected_kwargs()


def test_predicate_opens_for_the_general_route_only_with_the_attribute_and_resolvable_one_states():
    cfg = QutipConfig(observables=SERVED(), **DETERMINISTIC)
    sim = QutipBackendV2(_xy_inputs(), config=cfg)._sim_obj
    assert _mc_ensemble_route(sim, cfg) is False  # (as before: the tuned kernels do not take an XY register)
    assert _mc_ensemble_route(sim, cfg, False) is False
    assert _mc_ensemble_route(sim, cfg, True) is True
    for extra in ([StateObservable()], [Occupation(one_state="r", tag_suffix="r")]):  # reads the matrix / not an eigenstate of (u, d)
        cfg = QutipConfig(observables=SERVED() + extra, **DETERMINISTIC)
        assert _mc_ensemble_route(QutipBackendV2(_xy_inputs(), config=cfg)._sim_obj, cfg, True) is False
    cfg = QutipConfig(observables=SERVED(), **dict(DETERMINISTIC, solver=Solver.MESOLVER))
    assert _mc_ensemble_route(QutipBackendV2(_xy_inputs(), config=cfg)._sim_obj, cfg, True) is False


class _StubGeneralEngine:
    built = []

    def __init__(self, tables, device=None, batch=1):
        self.tables, self.batch = tables, batch
        _StubGeneralEngine.built.append(self)

    def stats(self):
        return {}

    def close(self):
        pass


@pytest.mark.parametrize("jumps,ensemble,extra", [(False, False, []), (False, True, []), (True, False, []),
                                                  (True, True, []), (True, True, ["state"])])
def test_backend_hands_the_options_the_digits_and_a_matrix_free_observer_to_the_solve(jumps, ensemble, extra, monkeypatch):
    from pulser_amd import engine

    _StubGeneralEngine.built.clear()
    monkeypatch.setattr(engine, "GeneralEngine", _StubGeneralEngine)
    seen = {}

    class _Solved(Exception):
        pass

    def run(self, progress_bar=False, print_progress=False, **options):
        seen.update(options)
        raise _Solved

    monkeypatch.setattr(QutipEmulator, "run", run)
    cfg = QutipConfig(observables=SERVED() + [StateObservable() for _ in extra], **DETERMINISTIC)
    backend = QutipBackendV2(_xy_inputs(), config=cfg)
    backend.general_jumps, backend.mc_ensemble = jumps, ensemble
    state = np.random.get_state()
    with pytest.raises(_Solved):
        backend.run()
    assert QutipBackendV2.general_jumps is False and QutipBackendV2.mc_ensemble is False  # (instance attributes)
    assert ("general_jumps" in seen) == jumps and (not jumps or seen["general_jumps"] is True)
    if jumps and ensemble and not extra:
        assert seen["mc_ensemble"] is True and seen["mc_ensemble_digits"] == [0, 1]  # "u" named, "d" inferred
        assert len(_StubGeneralEngine.built) == 1 and seen["mc_ensemble_observer"] is _StubGeneralEngine.built[0]
        tables = seen["mc_ensemble_observer"].tables  # lowered matrix-free although the register is tiny, no collapse
        assert getattr(tables, "free", None) is not None and not tables.is_density and tables.dim == 16
    else:
        assert not {"mc_ensemble", "mc_ensemble_digits", "mc_ensemble_observer"} & set(seen)
        assert not _StubGeneralEngine.built
    # (building the observer before the solve drew nothing from the global stream)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]

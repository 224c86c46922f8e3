"""CPU: the host side of the one-call observable path for multi-level and XY master-equation runs - the
``ryd_general_observe_density_many`` declaration, binding and export, the routing predicate of ``QutipBackendV2``
(``_general_density_many_route``) on stand-in engines and stores, the emulator's ``general_density_snapshots`` option
with the engine replaced by a host stand-in, and the option hand-over of ``QutipBackendV2.general_density_one_call``."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import load_fixture

from pulser_amd import NoiseModel, QutipEmulator
from pulser_amd import _lib
from pulser_amd.backend import (CorrelationMatrix, Energy, Expectation, Occupation, QutipBackendV2, QutipConfig,
                                _observe_density_many_route, _observe_many_route)
from pulser_amd.hamiltonian_data import SequenceInputs
from pulser_amd.results import LazyState, QState, SnapshotStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["ryd_handle* h", "const void* states_dev", "int32_t n_times", "int32_t n_batch", "int64_t stride_t",
             "int64_t stride_b", "const double* times", "int32_t what", "int32_t local_dim", "int32_t n_atoms",
             "int32_t one_digit", "double* out_dev", "void* stream"]
FLOOR = 128


def _route(*a, **kw):
    from pulser_amd.backend import _general_density_many_route

    return _general_density_many_route(*a, **kw)


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_general_observe_density_many\(([^;]*)\);", header)
    assert m, "ryd_general_observe_density_many is not declared in include/rydemu.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == PROTOTYPE
    restype, argtypes = _lib.SYMBOLS["ryd_general_observe_density_many"]
    want = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
            C.c_int32, C.c_void_p, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want
    assert list(argtypes) == list(_lib.SYMBOLS["ryd_general_observe_many"][1])  # (the signature of its ket sibling)
    assert hasattr(_lib.load(), "ryd_general_observe_density_many")  # (loading the library needs no device)
    assert _lib.RYD_ABI_VERSION == 1 and re.search(r"#define\s+RYD_ABI_VERSION\s+1\b", header)


def test_null_handle_is_refused_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data
    for args in ((None, p, 1, 1, 16, 16, p, 7, 2, 2, 0, p, None), (None, None, -1, 0, 0, 0, None, 7, 9, 99, 9, None, None)):
        assert lib.ryd_general_observe_density_many(*args) == -1  # RYD_ERR_INVALID
        msg = lib.ryd_last_error().decode()
        assert "observe_density_many" in msg and "null handle" in msg, msg


def test_floor_and_attribute_are_class_constants_and_the_config_has_no_key():
    assert QutipBackendV2._GENERAL_DENSITY_OBSERVE_MANY_FLOOR == FLOOR
    assert QutipBackendV2.general_density_one_call is False
    assert "general_density_one_call" not in QutipConfig._expected_kwargs()


# ---------------------------------------------------------------------------------------------------------------------
# the predicate
# ---------------------------------------------------------------------------------------------------------------------
class _Tensor:
    """What the predicate asks of a store's device tensor (no torch, no GPU)."""

    def __init__(self, shape, is_cuda=True):
        self.shape, self.is_cuda = tuple(shape), is_cuda
        self.nbytes = 0

    def dim(self):
        return len(self.shape)


def _general(n=2, d=3, path="fused_lds", **kw):
    """Stand-in for the noiseless ket ``GeneralEngine``: one problem, ``d`` levels, ``n`` atoms."""
    base = dict(observe_many=lambda *a, **k: None, observe_density_many=lambda *a, **k: None, local_dim=d, n=n, dim=d**n,
                batch=1, is_density=False, n_collapse=0, apply_path=lambda: path)
    base.update(kw)
    return SimpleNamespace(**base)


def _matrices(store, n_times, D, b=0):
    return [LazyState(store, i, b, (D, D)) for i in range(n_times)]


def test_route_takes_a_four_axis_store():
    T, D = FLOOR + 2, 9
    store = SnapshotStore(_Tensor((T, 1, D, D)))
    states = [QState(np.eye(D, dtype=complex))] + _matrices(store, T, D)  # (the initial state is a host state)
    fires = [True] * (T + 1)
    fires[5] = False                                                      # (no observable fires there)
    route = _route(states, fires, _general(), 3, 1)
    assert route is not None and route[0] is store and route[1] == 0
    assert route[2] == [p for p in range(1, T + 1) if p != 5]
    for path in ("fused", "fused_lds"):
        assert _route(states, fires, _general(path=path), 3, 1, True) is not None
    # pairs only: neither the application kernel nor collapse operators matter
    for kw in (dict(path="sites"), dict(path="terms"), dict(n_collapse=2)):
        assert _route(states, fires, _general(**kw), 3, 1, False) is not None, kw
    # XY: two levels on a general engine
    xy = SnapshotStore(_Tensor((T, 1, 8, 8)))
    assert _route(_matrices(xy, T, 8), [True] * T, _general(n=3, d=2), 2, 1) is not None
    # the existing predicates answer for these engines and states as they always did
    assert _observe_many_route(states, fires, _general(), 3, 1) is None
    assert _observe_density_many_route(states, fires, _general(), 3, 1) is None
    assert _observe_density_many_route(states, fires, _general(is_density=True, dim=81), 3, 1) is None
    kets = [LazyState(SnapshotStore(_Tensor((T, 1, D))), i, 0, (D, 1)) for i in range(T)]
    assert _observe_many_route(kets, [True] * T, _general(), 3, 1) is not None
    assert _observe_many_route(kets, [True] * T, _general(is_density=True, dim=81), 3, 1) is None
    assert _route(kets, [True] * T, _general(), 3, 1) is None


def test_route_opens_exactly_at_the_floor_and_refuses_a_spilled_store():
    D = 9
    for T, min_times, want in ((FLOOR, 1, True), (FLOOR, FLOOR, True), (FLOOR - 1, 1, False), (FLOOR + 5, FLOOR + 5, True),
                               (FLOOR + 5, FLOOR + 6, False)):
        store = SnapshotStore(_Tensor((T, 1, D, D)))
        got = _route(_matrices(store, T, D), [True] * T, _general(), 3, min_times)
        assert (got is not None) == want, (T, min_times)
    store = SnapshotStore(_Tensor((FLOOR, 1, D, D)))
    states = _matrices(store, FLOOR, D)
    assert _route(states, [True] * FLOOR, _general(), 3, 1) is not None
    store._dev, store._host = None, [None] * FLOOR  # (spilled: SnapshotStore.fetch_all leaves it like this)
    assert _route(states, [True] * FLOOR, _general(), 3, 1) is None


def test_route_skips_states_already_read():
    T, D = FLOOR + 1, 9
    store = SnapshotStore(_Tensor((T, 1, D, D)))
    states = _matrices(store, T, D)
    states[3]._store, states[3]._q = None, object()  # (what a materialised LazyState looks like)
    route = _route(states, [True] * T, _general(), 3, 1)
    assert route is not None and 3 not in route[2] and len(route[2]) == T - 1
    states[4]._store = None                          # one more: below the floor now
    assert _route(states, [True] * T, _general(), 3, 1) is None


@pytest.mark.parametrize("why,shape,state_shape,engine,n_eig,min_times,energy", [
    ("a density engine", (200, 1, 9, 9), (9, 9), dict(is_density=True, dim=81), 3, 1, True),
    ("batch 2", (200, 1, 9, 9), (9, 9), dict(batch=2), 3, 1, True),
    ("local_dim 5", (200, 1, 25, 25), (25, 25), dict(d=5), 5, 1, True),
    ("local_dim != n_eigenstates", (200, 1, 9, 9), (9, 9), dict(), 4, 1, True),
    ("dim != d**n", (200, 1, 10, 10), (10, 10), dict(dim=10), 3, 1, True),
    ("energy with collapse operators", (200, 1, 9, 9), (9, 9), dict(n_collapse=1), 3, 1, True),
    ("energy on the site kernel", (200, 1, 9, 9), (9, 9), dict(path="sites"), 3, 1, True),
    ("energy on the term kernel", (200, 1, 9, 9), (9, 9), dict(path="terms"), 3, 1, True),
    ("a 3-axis store", (200, 1, 81), (9, 9), dict(), 3, 1, True),
    ("wrong D in the store", (200, 1, 8, 8), (8, 8), dict(), 3, 1, True),
    ("wrong D in the states", (200, 1, 9, 9), (8, 8), dict(), 3, 1, True),
    ("a host tensor", (200, 1, 9, 9), (9, 9), dict(), 3, 1, True),
    ("an engine without the call", (200, 1, 9, 9), (9, 9), dict(observe_density_many=None), 3, 1, True),
    ("a two-level Ising engine", (200, 1, 4, 4), (4, 4), dict(local_dim=None), 2, 1, True),
    ("fewer than the floor, whatever min_times says", (FLOOR - 1, 1, 9, 9), (9, 9), dict(), 3, 1, True),
    ("fewer than min_times above the floor", (200, 1, 9, 9), (9, 9), dict(), 3, 201, True),
    ("min_times=None", (200, 1, 9, 9), (9, 9), dict(), 3, None, True),
])
def test_route_refuses(why, shape, state_shape, engine, n_eig, min_times, energy):
    store = SnapshotStore(_Tensor(shape, is_cuda=why != "a host tensor"))
    n_times = shape[0]
    states = [LazyState(store, i, 0, state_shape) for i in range(n_times)]
    fires = [True] * n_times
    eng = _general(**{k: v for k, v in engine.items() if v is not None})
    for k, v in engine.items():
        if v is None:
            delattr(eng, k)
    assert _route(states, fires, eng, n_eig, min_times, energy) is None, why


# ---------------------------------------------------------------------------------------------------------------------
# the emulator: run(general_density_snapshots=True)
# ---------------------------------------------------------------------------------------------------------------------
class _FakeTensor:
    """A numpy array behind the few tensor calls ``_solve_general`` and ``SnapshotStore`` make."""

    is_cuda = True

    def __init__(self, a):
        self.a = np.asarray(a)

    shape = property(lambda self: self.a.shape)
    nbytes = property(lambda self: self.a.nbytes)

    def dim(self):
        return self.a.ndim

    def reshape(self, *shape):
        return _FakeTensor(self.a.reshape(*shape))

    def __getitem__(self, key):
        return _FakeTensor(self.a[key])

    def cpu(self):
        return self

    def numpy(self):
        return self.a

    def element_size(self):
        return self.a.itemsize

    def numel(self):
        return self.a.size


def _xy_emulator(noise=True):
    prob, _ = load_fixture("noisy_xy_0.npz")
    emu = QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), sampling_rate=0.1,
                        noise_model=NoiseModel(dephasing_rate=0.5) if noise else None)
    return emu


def _solve_with_stand_ins(emu, mode, options, monkeypatch):
    """``_solve_general`` with ``GeneralEngine``, ``lower_general`` and the budget check (it asks the device for its free
    memory) replaced: (results, the solved stand-in tensors, D, the budget checks made)."""
    from pulser_amd import engine, general

    D = 2 ** emu._hamiltonian_data.n_qudits
    made, budget = [], []
    monkeypatch.setattr(QutipEmulator, "_check_snapshot_budget",
                        staticmethod(lambda n, per, what="": budget.append((n, per, what))))

    class Stub:
        def __init__(self, tables):
            self.dim = tables.dim

        def new_state(self, ket):
            psi = np.asarray(ket, dtype=complex).reshape(-1)
            first = np.outer(psi, psi.conj()).reshape(-1) if self.dim == D * D else psi
            return _FakeTensor(first[None])

        def solve(self, state, times, **kw):
            rng = np.random.default_rng(len(made))
            snap = _FakeTensor(rng.normal(size=(len(times) - 1, 1, self.dim)) + 0j)
            made.append(snap)
            return snap

        def stats(self):
            return {}

        def close(self):
            pass

    monkeypatch.setattr(engine, "GeneralEngine", Stub)
    monkeypatch.setattr(general, "lower_general", lambda prob, mesolve=False, **kw: SimpleNamespace(dim=D * D if mesolve else D))
    options = dict(options)
    emu._validate_options(options)
    return emu._solve_general([emu._current_problem], mode, options), made, D, budget


@pytest.mark.parametrize("options,mode,kept", [
    ({}, "mesolve", False),
    ({"general_density_snapshots": False}, "mesolve", False),
    ({"general_density_snapshots": True}, "mesolve", True),
    ({"general_device_snapshots": True}, "mesolve", False),   # (its meaning stays: sesolve kets only)
    ({"general_density_snapshots": True}, "sesolve", False),  # (and this one is for matrices only)
])
def test_option_keeps_the_matrices_on_the_device_for_mesolve_only(options, mode, kept, monkeypatch):
    emu = _xy_emulator()
    (res,), made, D, budget = _solve_with_stand_ins(emu, mode, options, monkeypatch)
    assert bool(budget) == kept
    states = list(res.states)
    T = len(emu._eval_times_array)
    assert len(states) == T and len(made) == 1
    shape = (D, D) if mode == "mesolve" else (D, 1)
    assert type(states[0]) is QState and tuple(states[0].shape) == shape
    if kept:
        assert all(type(st) is LazyState for st in states[1:])
        stores = {id(st._store) for st in states[1:]}
        assert len(stores) == 1
        dev = states[1]._store.device_tensor
        assert tuple(dev.shape) == (T - 1, 1, D, D)
        assert np.shares_memory(dev.a, made[0].a)  # the solved tensor itself, viewed as matrices
        assert [(st._i, st._b, tuple(st.shape)) for st in states[1:]] == [(i, 0, (D, D)) for i in range(T - 1)]
        assert np.array_equal(np.asarray(states[3]), made[0].a[2, 0].reshape(D, D))
    else:
        assert all(type(st) is QState and tuple(st.shape) == shape for st in states)
        assert np.array_equal(np.asarray(states[3]), made[0].a[2, 0].reshape(shape))


def test_option_checks_the_budget_of_all_trajectories_first(monkeypatch):
    emu = _xy_emulator()
    _, made, D, seen = _solve_with_stand_ins(emu, "mesolve", {"general_density_snapshots": True}, monkeypatch)
    assert seen == [(len(emu._eval_times_array) - 1, 16 * D * D, seen[0][2])] and "density matrices" in seen[0][2]
    assert _solve_with_stand_ins(emu, "mesolve", {}, monkeypatch)[3] == []


def test_run_docstring_documents_the_option():
    doc = QutipEmulator.run.__doc__
    assert "general_density_snapshots=True" in doc and "general_device_snapshots=True" in doc


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend hands the option over
# ---------------------------------------------------------------------------------------------------------------------
def _observables():
    return [Occupation(one_state="d"), CorrelationMatrix(one_state="d"), Energy()]


@pytest.mark.parametrize("attribute,noise,n_times,observables,expected", [
    (False, True, 130, "builtin", False),
    (True, True, 130, "builtin", True),
    (True, True, 127, "builtin", False),       # below the floor
    (True, False, 130, "builtin", False),      # no collapse operators: the ket route's business
    (True, True, 130, "expectation", True),    # Fidelity / Expectation alone keep the matrices there too
    (True, True, 130, "none", False),
])
def test_backend_hands_the_option_to_the_solve(attribute, noise, n_times, observables, expected, monkeypatch):
    seen = {}

    class _Solved(Exception):
        pass

    def run(self, progress_bar=False, print_progress=False, **options):
        seen.update(options)
        raise _Solved

    monkeypatch.setattr(QutipEmulator, "run", run)
    prob, _ = load_fixture("noisy_xy_0.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    from pulser_amd.backend import BitStrings

    obs = {"builtin": _observables(), "expectation": [Expectation(np.eye(16))], "none": [BitStrings(num_shots=5)]}[observables]
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, n_times).tolist(), observables=obs,
                      noise_model=NoiseModel(dephasing_rate=0.05) if noise else NoiseModel())
    backend = QutipBackendV2(inputs, config=cfg)
    if attribute:
        backend.general_density_one_call = True
    with pytest.raises(_Solved):
        backend.run()
    assert QutipBackendV2.general_density_one_call is False  # (set on the instance only)
    assert (seen.get("general_density_snapshots") is True) == expected, seen
    if not expected:
        assert "general_density_snapshots" not in seen
    if attribute and noise:
        assert "general_device_snapshots" not in seen  # (the ket option is not this run's)


def test_backend_threshold_none_switches_the_route_off(monkeypatch):
    seen = {}

    class _Solved(Exception):
        pass

    def run(self, progress_bar=False, print_progress=False, **options):
        seen.update(options)
        raise _Solved

    monkeypatch.setattr(QutipEmulator, "run", run)
    prob, _ = load_fixture("noisy_xy_0.npz")
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, 130).tolist(), observables=_observables(),
                      noise_model=NoiseModel(dephasing_rate=0.05))
    backend = QutipBackendV2(SequenceInputs.from_dict(prob["inputs"]), config=cfg)
    backend.general_density_one_call = True
    backend.observe_many_min_times = None
    with pytest.raises(_Solved):
        backend.run()
    assert "general_density_snapshots" not in seen

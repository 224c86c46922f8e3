"""CPU: the host side of the one-call observable path for two-level master-equation runs - the
``ryd_observe_density_many`` declaration, binding and export, the routing predicate of ``QutipBackendV2``
(``_observe_density_many_route``) on stand-in engines and stores, and ``_DeferredRydState`` on a density matrix."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from pulser_amd import _lib
from pulser_amd.backend import QutipBackendV2, RydState, _DeferredRydState, _observe_density_many_route, _observe_many_route
from pulser_amd.results import LazyState, SnapshotStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["ryd_handle* h", "const void* states_dev", "int32_t n_times", "int32_t n_batch", "int64_t stride_t",
             "int64_t stride_b", "const double* times", "int32_t what", "double* out_dev", "void* stream"]
FLOOR = 128


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_observe_density_many\(([^;]*)\);", header)
    assert m, "ryd_observe_density_many is not declared in include/rydemu.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == PROTOTYPE
    restype, argtypes = _lib.SYMBOLS["ryd_observe_density_many"]
    want = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want
    assert list(argtypes) == list(_lib.SYMBOLS["ryd_observe_many"][1])  # (the signature of its ket sibling)
    assert hasattr(_lib.load(), "ryd_observe_density_many")  # (loading the library needs no device)
    assert re.search(r"#define RYD_ABI_VERSION 1\b", header)


def test_floor_is_a_class_constant():
    assert QutipBackendV2._DENSITY_OBSERVE_MANY_FLOOR == FLOOR


class _Tensor:
    """What the predicate asks of a store's device tensor (no torch, no GPU)."""

    def __init__(self, shape, is_cuda=True):
        self.shape, self.is_cuda = tuple(shape), is_cuda
        self.nbytes = 0

    def dim(self):
        return len(self.shape)


def _ising(n=3, **kw):
    """Stand-in for the noiseless two-level ``Engine``: one problem, sesolve mode, no jumps, no detuning terms."""
    base = dict(observe_many=lambda *a, **k: None, observe_density_many=lambda *a, **k: None, n=n, dim=2**n, batch=1,
                mode=0, monte_carlo=False, tables=SimpleNamespace(dterms=None))
    base.update(kw)
    return SimpleNamespace(**base)


def _matrices(store, n_times, D, b=0):
    return [LazyState(store, i, b, (D, D)) for i in range(n_times)]


def test_route_takes_a_four_axis_store():
    T, D = FLOOR + 2, 8
    store = SnapshotStore(_Tensor((T, 2, D, D)))
    states = [np.eye(D, dtype=complex)] + _matrices(store, T, D, b=1)  # (the initial state is a host array)
    fires = [True] * (T + 1)
    fires[5] = False                                                   # (no built-in observable fires there)
    route = _observe_density_many_route(states, fires, _ising(), 2, 1)
    assert route is not None and route[0] is store and route[1] == 1
    assert route[2] == [p for p in range(1, T + 1) if p != 5]
    # the ket route leaves these states alone, and the density route leaves kets alone
    assert _observe_many_route(states, fires, _ising(), 2, 1) is None
    kets = [LazyState(SnapshotStore(_Tensor((T, 1, D))), i, 0, (D, 1)) for i in range(T)]
    assert _observe_many_route(kets, [True] * T, _ising(), 2, 1) is not None
    assert _observe_density_many_route(kets, [True] * T, _ising(), 2, 1) is None


def test_route_skips_states_already_read():
    T, D = FLOOR + 1, 4
    store = SnapshotStore(_Tensor((T, 1, D, D)))
    states = _matrices(store, T, D)
    states[3]._store, states[3]._q = None, object()  # (what a materialised LazyState looks like)
    route = _observe_density_many_route(states, [True] * T, _ising(n=2), 2, 1)
    assert route is not None and 3 not in route[2] and len(route[2]) == T - 1
    states[4]._store = None                          # one more: below the floor now
    assert _observe_density_many_route(states, [True] * T, _ising(n=2), 2, 1) is None


@pytest.mark.parametrize("why,shape,state_shape,engine,n_eig,n_times,min_times", [
    ("a 3-axis store with non-ket states", (200, 1, 64), (8, 8), dict(), 2, 200, 1),
    ("wrong D in the store", (200, 1, 4, 4), (4, 4), dict(), 2, 200, 1),
    ("wrong D in the states", (200, 1, 8, 8), (4, 4), dict(), 2, 200, 1),
    ("engine batch != 1", (200, 1, 8, 8), (8, 8), dict(batch=2), 2, 200, 1),
    ("a mesolve engine", (200, 1, 8, 8), (8, 8), dict(mode=1), 2, 200, 1),
    ("a Monte-Carlo engine", (200, 1, 8, 8), (8, 8), dict(monte_carlo=True), 2, 200, 1),
    ("extra detuning terms", (200, 1, 8, 8), (8, 8), dict(tables=SimpleNamespace(dterms=np.zeros(1))), 2, 200, 1),
    ("a general engine", (200, 1, 8, 8), (8, 8), dict(local_dim=2), 2, 200, 1),
    ("an engine without the call", (200, 1, 8, 8), (8, 8), dict(observe_density_many=None), 2, 200, 1),
    ("three eigenstates", (200, 1, 8, 8), (8, 8), dict(), 3, 200, 1),
    ("fewer than the floor, whatever min_times says", (FLOOR - 1, 1, 8, 8), (8, 8), dict(), 2, FLOOR - 1, 1),
    ("fewer than min_times above the floor", (200, 1, 8, 8), (8, 8), dict(), 2, 200, 201),
    ("min_times=None", (200, 1, 8, 8), (8, 8), dict(), 2, 200, None),
    ("a host tensor", (200, 1, 8, 8), (8, 8), dict(), 2, 200, 1),
])
def test_route_refuses(why, shape, state_shape, engine, n_eig, n_times, min_times):
    store = SnapshotStore(_Tensor(shape, is_cuda=why != "a host tensor"))
    states = [LazyState(store, i, 0, state_shape) for i in range(n_times)]
    fires = [True] * n_times
    if engine.get("observe_density_many", 1) is None:
        eng = _ising()
        del eng.observe_density_many
    else:
        eng = _ising(**engine)
    assert _observe_density_many_route(states, fires, eng, n_eig, min_times) is None, why


def test_route_opens_exactly_at_the_floor_and_refuses_a_spilled_store():
    D = 8
    for T, min_times, want in ((FLOOR, 1, True), (FLOOR, FLOOR, True), (FLOOR - 1, 1, False), (FLOOR + 5, FLOOR + 5, True),
                               (FLOOR + 5, FLOOR + 6, False)):
        store = SnapshotStore(_Tensor((T, 1, D, D)))
        got = _observe_density_many_route(_matrices(store, T, D), [True] * T, _ising(), 2, min_times)
        assert (got is not None) == want, (T, min_times)
    store = SnapshotStore(_Tensor((FLOOR, 1, D, D)))
    states = _matrices(store, FLOOR, D)
    assert _observe_density_many_route(states, [True] * FLOOR, _ising(), 2, 1) is not None
    store._dev, store._host = None, [None] * FLOOR  # (spilled: SnapshotStore.fetch_all leaves it like this)
    assert _observe_density_many_route(states, [True] * FLOOR, _ising(), 2, 1) is None


def test_deferred_state_of_a_density_matrix_is_the_eager_one():
    """``_DeferredRydState`` costs nothing until it is read, and then is ``RydState(lazy.unit())``: a matrix divided by
    its trace norm, as the per-time path builds it."""
    D = 4
    rng = np.random.default_rng(5)
    a = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    rho = 1.7 * (a @ a.conj().T)

    class Host:
        """A store that counts its reads."""
        reads = 0

        def get(self, i, b):
            Host.reads += 1
            return rho.copy()

    lazy = LazyState(Host(), 0, 0, (D, D))
    deferred = _DeferredRydState(lazy, eigenstates=("r", "g"))
    assert deferred.n_qudits == 2 and deferred.qudit_dim == 2 and deferred.infer_one_state() == "r" and Host.reads == 0
    eager = RydState(LazyState(Host(), 0, 0, (D, D)).unit(), eigenstates=("r", "g"))
    got = np.asarray(deferred.to_qobj())
    assert Host.reads == 2 and got.shape == (D, D) and not deferred.to_qobj().isket
    assert np.array_equal(got, np.asarray(eager.to_qobj()))
    assert abs(np.trace(got).real - 1.0) < 1e-14  # (positive matrix: the trace norm is the trace)

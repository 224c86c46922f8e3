"""CPU: the host side of the one-call ``Fidelity`` / ``Expectation`` path - the ``ryd_overlap_many`` declaration, binding
and export, the routing predicate of ``QutipBackendV2`` (``_overlap_many_route``) on stand-in stores, and what a seeded
and an unseeded ``_DeferredRydState`` hand to the two observables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pulser_amd import _lib
from pulser_amd.backend import (Expectation, Fidelity, QutipBackendV2, RydOperator, RydState, _DeferredRydState,
                                _overlap_many_route)
from pulser_amd.results import LazyState, SnapshotStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["const void* states_dev", "int64_t n_states", "int64_t stride", "int64_t dim", "int32_t density",
             "const void* targets_dev", "int32_t n_targets", "int32_t target_form", "void* out_dev", "double* norm_dev",
             "int32_t device", "void* stream"]
FLOOR = 128


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_overlap_many\(([^;]*)\);", header)
    assert m, "ryd_overlap_many is not declared in include/rydemu.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == PROTOTYPE, args
    restype, argtypes = _lib.SYMBOLS["ryd_overlap_many"]
    want = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
            C.c_void_p, C.c_int32, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want and len(argtypes) == 12
    # (loading the library needs no device)
    assert hasattr(_lib.load(), "ryd_overlap_many")
    assert _lib.RYD_ABI_VERSION == 1


class _Tensor:
    """What the predicate asks of a store's device tensor (no torch, no GPU)."""

    def __init__(self, shape, is_cuda=True):
        self.shape, self.is_cuda = tuple(shape), is_cuda
        self.nbytes = 0

    def dim(self):
        return len(self.shape)


def _states(store, n_times, D, density=False, b=0):
    return [LazyState(store, i, b, (D, D) if density else (D, 1)) for i in range(n_times)]


@pytest.mark.parametrize("density", [False, True])
def test_route_opens_at_the_threshold_and_not_one_below(density):
    assert QutipBackendV2._OVERLAP_MANY_FLOOR == FLOOR
    D = 8
    tail = (D, D) if density else (D,)
    for T, min_times, opens in ((FLOOR, FLOOR, True), (FLOOR - 1, FLOOR, False), (150, 150, True), (149, 150, False),
                                (FLOOR, 1, True), (FLOOR - 1, 1, False),   # the floor holds below the threshold
                                (400, None, False)):                        # None switches the route off
        store = SnapshotStore(_Tensor((T, 2, *tail)))
        route = _overlap_many_route(_states(store, T, D, density, b=1), [True] * T, min_times)
        assert (route is not None) == opens, (T, min_times)
        if opens:
            assert route[0] is store and route[1] == 1 and route[2] == list(range(T)) and route[3] is density


def test_route_counts_only_firing_unread_snapshots_of_one_store():
    T, D = FLOOR + 2, 4
    store = SnapshotStore(_Tensor((T, 1, D)))
    lazy = _states(store, T, D)
    states = [np.ones((D, 1), complex)] + lazy  # the initial state is a host array
    fires = [True] * (T + 1)
    route = _overlap_many_route(states, fires, FLOOR)
    assert route is not None and route[2] == list(range(1, T + 1)) and route[3] is False
    # two positions where nothing fires: exactly the floor is left
    quiet = list(fires)
    quiet[3] = quiet[7] = False
    assert _overlap_many_route(states, quiet, FLOOR)[2] == [p for p in range(1, T + 1) if p not in (3, 7)]
    quiet[9] = False
    assert _overlap_many_route(states, quiet, FLOOR) is None
    # a state that has been read holds its host data and has let go of the store
    lazy[0]._q, lazy[0]._store = np.ones((D, 1), complex), None
    lazy[5]._q, lazy[5]._store = np.ones((D, 1), complex), None
    assert _overlap_many_route(states, fires, FLOOR)[2] == [p for p in range(2, T + 1) if p != 6]
    lazy[6]._q, lazy[6]._store = np.ones((D, 1), complex), None
    assert _overlap_many_route(states, fires, FLOOR) is None
    # the states of another store do not count
    other = SnapshotStore(_Tensor((T, 1, D)))
    mixed = _states(store, FLOOR - 1, D) + _states(other, 3, D)
    assert _overlap_many_route(mixed, [True] * len(mixed), FLOOR) is None


@pytest.mark.parametrize("why,shape,lazy_shape", [
    ("a rectangular tail", (FLOOR, 1, 4, 5), (4, 5)),
    ("three state axes", (FLOOR, 1, 4, 4, 4), (4, 4)),
    ("no sequence axis", (FLOOR, 4), (4, 1)),
    ("a tensor of another dimension than its states", (FLOOR, 1, 8), (4, 1)),
    ("kets in a store of matrices", (FLOOR, 1, 4, 4), (4, 1)),
])
def test_route_refuses_a_tail_of_the_wrong_shape(why, shape, lazy_shape):
    store = SnapshotStore(_Tensor(shape))
    states = [LazyState(store, i, 0, lazy_shape) for i in range(FLOOR)]
    assert _overlap_many_route(states, [True] * FLOOR, FLOOR) is None, why


def test_route_refuses_spilled_and_host_stores():
    D = 4
    store = SnapshotStore(_Tensor((FLOOR, 1, D)))
    states = _states(store, FLOOR, D)
    assert _overlap_many_route(states, [True] * FLOOR, FLOOR) is not None
    store._host, store._dev = [np.zeros((1, D), complex)] * FLOOR, None  # what fetch_all leaves behind
    assert _overlap_many_route(states, [True] * FLOOR, FLOOR) is None
    host = SnapshotStore(_Tensor((FLOOR, 1, D), is_cuda=False))
    assert _overlap_many_route(_states(host, FLOOR, D), [True] * FLOOR, FLOOR) is None


class _CountedStore(SnapshotStore):
    def __init__(self, tensor):
        super().__init__(tensor)
        self.gets = []

    def get(self, i, b):
        self.gets.append((i, b))
        return super().get(i, b)


def _snapshots(density):
    import torch

    D = 4
    rng = np.random.default_rng(5 + density)
    shape = (3, 1, D, D) if density else (3, 1, D)
    host = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    if density:
        host = host @ host.conj().transpose(0, 1, 3, 2)  # positive: the trace norm of the eager path is the trace
    return D, host, _CountedStore(torch.from_numpy(host.copy()))


def _observables(D):
    eig = ("r", "g")
    target = RydState(np.arange(1, D + 1) * (1 + 0.5j), eigenstates=eig)
    op = RydOperator.from_operator_repr(eigenstates=eig, n_qudits=2, operations=[(1.0, [({"rg": 1.0, "gr": 1.0}, {0})])])
    dense = np.arange(D * D, dtype=complex).reshape(D, D)
    return eig, [Fidelity(target), Expectation(op), Expectation(dense)]


@pytest.mark.parametrize("density", [False, True])
def test_seeded_deferred_state_is_not_read(density):
    D, _, store = _snapshots(density)
    eig, obs = _observables(D)
    state = _DeferredRydState(LazyState(store, 1, 0, (D, D) if density else (D, 1)), eigenstates=eig)
    seeds = [0.25, 0.5 - 2j, 3 + 1j]
    for o, v in zip(obs, seeds):
        state.seed(o, v)
    for o, v in zip(obs, seeds):
        got = o.apply(state=state, config=None, hamiltonian=None)
        assert got == v and type(got) is type(v)
    assert store.gets == []
    # another observable of the same kind has no seed: it reads the state (once) and gives the eager value
    other = Fidelity(obs[0].state)
    eager = RydState(LazyState(store, 1, 0, (D, D) if density else (D, 1)).unit(), eigenstates=eig)
    store.gets.clear()
    assert other.apply(state=state) == other.apply(state=eager)
    assert store.gets == [(1, 0)]


@pytest.mark.parametrize("density", [False, True])
def test_unseeded_deferred_state_is_read_once_and_equals_the_eager_result(density):
    D, host, store = _snapshots(density)
    eig, obs = _observables(D)
    shape = (D, D) if density else (D, 1)
    state = _DeferredRydState(LazyState(store, 2, 0, shape), eigenstates=eig)
    got = [o.apply(state=state) for o in obs]
    assert store.gets == [(2, 0)]
    eager = RydState(LazyState(store, 2, 0, shape).unit(), eigenstates=eig)
    want = [o.apply(state=eager) for o in obs]
    assert got == want and all(type(g) is type(w) for g, w in zip(got, want))
    assert np.array_equal(np.asarray(state.to_qobj()), np.asarray(eager.to_qobj()))
    # a plain RydState carries no seeds: ``apply`` is what it was
    x = host[2, 0] if not density else host[2, 0] / np.trace(host[2, 0]).real
    plain = RydState(x, eigenstates=eig)
    assert obs[0].apply(state=plain) == obs[0].state.overlap(plain)

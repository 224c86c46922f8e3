"""CPU: the host side of the one-call observable path for multi-level and XY registers - the
``ryd_general_observe_many`` declaration, binding and export, the routing predicate of ``QutipBackendV2``
(``_observe_many_route``) on stand-in general engines, and ``HamiltonianOperator.seed`` with the digit counted."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from pulser_amd import _lib
from pulser_amd.backend import HamiltonianOperator, RydState, _observe_many_route
from pulser_amd.results import LazyState, SnapshotStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["ryd_handle* h", "const void* states_dev", "int32_t n_times", "int32_t n_batch", "int64_t stride_t",
             "int64_t stride_b", "const double* times", "int32_t what", "int32_t local_dim", "int32_t n_atoms",
             "int32_t one_digit", "double* out_dev", "void* stream"]


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_general_observe_many\(([^;]*)\);", header)
    assert m, "ryd_general_observe_many is not declared in include/rydemu.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == PROTOTYPE, args
    restype, argtypes = _lib.SYMBOLS["ryd_general_observe_many"]
    want = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want
    # (loading the library needs no device)
    assert hasattr(_lib.load(), "ryd_general_observe_many")


def test_apply_path_query_is_declared_bound_and_exported():
    """``ryd_general_apply_path``: the kernel of the next application, asked before the first one (``ryd_get_stats``
    stays a pure read), so it takes a handle it may build tables on - not a const one."""
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_general_apply_path\(([^;]*)\);", header)
    assert m, "ryd_general_apply_path is not declared in include/rydemu.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ["ryd_handle* h", "int32_t* path"]
    assert re.search(r"int ryd_get_stats\(const ryd_handle\* h, ryd_stats\* out\);", header)
    restype, argtypes = _lib.SYMBOLS["ryd_general_apply_path"]
    assert restype is C.c_int and list(argtypes) == [C.c_void_p, C.POINTER(C.c_int32)]
    assert hasattr(_lib.load(), "ryd_general_apply_path")


class _Tensor:
    """What the predicate asks of a store's device tensor (no torch, no GPU)."""

    def __init__(self, shape, is_cuda=True):
        self.shape, self.is_cuda = tuple(shape), is_cuda
        self.nbytes = 0

    def dim(self):
        return len(self.shape)


def _general(n=3, d=3, path="fused_lds", **kw):
    """Stand-in for a ``GeneralEngine``: a ket engine of one problem, ``d`` levels, ``n`` atoms."""
    base = dict(observe_many=lambda *a, **k: None, local_dim=d, n=n, dim=d**n, batch=1, is_density=False, n_collapse=0,
                apply_path=lambda: path)
    base.update(kw)
    return SimpleNamespace(**base)


def _states(store, n_times, D):
    return [LazyState(store, i, 0, (D, 1)) for i in range(n_times)]


def test_route_takes_a_qualifying_general_engine():
    T, D = 6, 27
    store = SnapshotStore(_Tensor((T, 1, D)))
    states = [np.ones((D, 1), complex)] + _states(store, T, D)  # (the initial state is a host array)
    fires = [True] * (T + 1)
    route = _observe_many_route(states, fires, _general(), 3, 6)
    assert route is not None and route[0] is store and route[1] == 0 and route[2] == [1, 2, 3, 4, 5, 6]
    for path in ("fused", "fused_lds"):
        assert _observe_many_route(states, fires, _general(path=path), 3, 6, True) is not None
    # XY: two levels on a general engine
    xy = SnapshotStore(_Tensor((T, 1, 8)))
    assert _observe_many_route(_states(xy, T, 8), [True] * T, _general(d=2), 2, T) is not None
    # pairs only: the application kernel does not matter
    for path in ("sites", "terms"):
        assert _observe_many_route(states, fires, _general(path=path), 3, 6, False) is not None


@pytest.mark.parametrize("why,engine,n_eig,min_times,energy", [
    ("a density engine", dict(is_density=True, dim=27 * 27), 3, 6, True),
    ("batch != 1", dict(batch=2), 3, 6, True),
    ("local_dim != number of eigenstates", dict(), 4, 6, True),
    ("dim is not local_dim ** n", dict(dim=28), 3, 6, True),
    ("the round-3 site kernel with energy wanted", dict(path="sites"), 3, 6, True),
    ("the term-by-term kernel with energy wanted", dict(path="terms"), 3, 6, True),
    ("collapse operators with energy wanted", dict(n_collapse=2), 3, 6, True),
    ("fewer than min_times qualifying positions", dict(), 3, 7, True),
    ("min_times=None", dict(), 3, None, True),
])
def test_route_refuses(why, engine, n_eig, min_times, energy):
    T, D = 6, 27
    states = _states(SnapshotStore(_Tensor((T, 1, D))), T, D)
    fires = [True] * T
    assert _observe_many_route(states, fires, _general(), 3, 6) is not None  # (the same states on a qualifying engine)
    assert _observe_many_route(states, fires, _general(**engine), n_eig, min_times, energy) is None, why


def test_seed_takes_the_digit_and_costs_no_engine_call():
    n, d = 2, 3
    eig = ("r", "g", "h")

    class Untouchable:
        """A general engine that ``observe`` may look at but must not call."""
        dim, local_dim, batch, is_density, device = d**n, d, 1, False, "cpu"

        def __init__(self):
            self.n = n

        def observe(self, *a, **k):
            raise AssertionError("a seeded state went to the device")

    x = np.zeros(d**n, complex)
    x[0] = 1.0
    state = RydState(x, eigenstates=eig)
    ham = HamiltonianOperator(Untouchable(), 0.1, eig)
    occ = {0: np.array([0.5, 1.0]), 1: np.array([1.5, 0.25])}
    corr = {k: np.outer(v, v) for k, v in occ.items()}
    ham.seed(state, 2.0, occ[0], corr[0], 3.0, 8.0, digit=0)   # the first call of a run carries the energies
    ham.seed(state, 2.0, occ[1], corr[1], digit=1)
    for one, k in (("r", 0), ("g", 1)):
        got = ham.observe(state, one)
        assert got["digit"] == k
        assert np.array_equal(got["occupation"], occ[k] / 2.0) and np.array_equal(got["correlation"], corr[k] / 2.0)
        assert got["energy"] == 1.5 and got["energy2"] == 4.0
    got = ham.observe(state, pairs=False)  # the energies need no digit
    assert got["energy"] == 1.5 and got["energy2"] == 4.0
    with pytest.raises(AssertionError):  # a digit nobody seeded is a device call
        ham.observe(state, "h")

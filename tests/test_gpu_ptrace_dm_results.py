"""GPU: the partial trace of master-equation runs at the level of results - ``SimulationResults.reduced_states`` /
``entanglement_entropy``, ``LazyState.ptrace`` and ``DeviceState.ptrace`` over density matrices that are still on the
device (``engine.reduced_density_dm``) against the host formula on the same matrices.

Bounds (none fitted to what the code gives).  The device route and the host route read the SAME stored numbers (a state
on the host is a copy of its snapshot), so they differ by their own rounding only: each sums the R = D / dA elements
``rho[idx(a, r)][idx(a', r)]`` of an entry in some order, S the sum of the absolute values of the summands.  Against the
longdouble reference each route is held to ITS OWN bound - the host formula to ``tol_reduced_dm(R, S)``, the device route
to ``tol_reduced_dm(R + n_split, S)``, where ``n_split`` is the number of partials the library may have added when it
chose a split (``engine.reduced_density_dm_splits``; nothing is added when that is 1) - and the two routes are compared
WITH EACH OTHER within the sum of the two bounds.  Real and imaginary parts are compared apart.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from helpers import load_fixture, with_anneal_samples
from observe_ref import LD
from ptrace_dm_ref import ref_reduced_dm, tol_reduced_dm
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QState, QutipEmulator, Solver, entropy_vn
from pulser_amd.results import CoherentResults, DeviceState, LazyState, SnapshotStore, StateResult, _ptrace_host

pytestmark = pytest.mark.gpu


class _Counters:
    """``SnapshotStore.get`` / ``fetch_all`` calls and the shapes handed to ``engine.reduced_density_dm`` (and to the
    ket call, which a master-equation run must never make)."""

    def __init__(self, monkeypatch):
        from pulser_amd import engine

        self.gets, self.bulk, self.calls, self.ket_calls = [], 0, [], []
        get, fetch_all, real, real_ket = (SnapshotStore.get, SnapshotStore.fetch_all, engine.reduced_density_dm,
                                          engine.reduced_density)

        def counted_get(store, i, b):
            self.gets.append((i, b))
            return get(store, i, b)

        def counted_fetch_all(store):
            self.bulk += 1
            return fetch_all(store)

        def counted(states, keep, local_dim=2, out=None, n_split=0):
            self.calls.append((tuple(states.shape), tuple(keep), local_dim))
            return real(states, keep, local_dim, out, n_split)

        def counted_ket(states, keep, local_dim=2, out=None, n_split=0):
            self.ket_calls.append((tuple(states.shape), tuple(keep), local_dim))
            return real_ket(states, keep, local_dim, out, n_split)

        monkeypatch.setattr(SnapshotStore, "get", counted_get)
        monkeypatch.setattr(SnapshotStore, "fetch_all", counted_fetch_all)
        monkeypatch.setattr(engine, "reduced_density_dm", counted)
        monkeypatch.setattr(engine, "reduced_density", counted_ket)


N6 = 6
N_TIMES = 12


def _tri6(n_times=N_TIMES):
    """The 6-atom dephasing fixture as a master-equation run at a dozen evaluation times."""
    prob, _ = load_fixture("cfg3_tri6_dephasing.npz")
    inputs = _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")
    emu = QutipEmulator(inputs, noise_model=NoiseModel(dephasing_rate=0.05), solver=Solver.MESOLVER,
                        evaluation_times=list(np.linspace(0.25, 3.0, n_times)))
    with pytest.warns(DeprecationWarning):
        res = emu.run()
    assert len(res) >= n_times and tuple(res.states[-1].shape) == (2**N6, 2**N6)
    return res


def _assert_routes_agree(got, mats, keep, d, n_split, what, host=None):
    """``got`` [T, dA, dA] from the device route and ``host`` (the host formula on the host copies ``mats`` [T, D, D];
    computed here when not given) against the reference, each within its own bound, and against each other within the
    sum of the two."""
    mats = np.asarray(mats)
    d_a = d ** len(keep)
    r = mats.shape[1] // d_a
    if host is None:
        host = np.array([_ptrace_host(m, False, keep, d) for m in mats])
    (re, im), s_re, s_im = ref_reduced_dm(mats[:, None], np.zeros((len(mats), d_a, d_a), dtype=complex), keep, d)
    worst = [0.0, 0.0, 0.0]
    for g, h, want, s in ((got.real, host.real, re, s_re), (got.imag, host.imag, im, s_im)):
        tol_dev = tol_reduced_dm(r + (n_split if n_split > 1 else 0), s)
        tol_host = tol_reduced_dm(r, s)
        errs = (np.abs(g.astype(LD) - want), np.abs(h.astype(LD) - want), np.abs(g.astype(LD) - h.astype(LD)))
        for k, (err, tol) in enumerate(zip(errs, (tol_dev, tol_host, tol_dev + tol_host))):
            with np.errstate(invalid="ignore", divide="ignore"):
                worst[k] = max(worst[k], float(np.max(np.where(err > 0, err / tol.astype(LD), 0))))
        print(f"RATIO reduced_states (density) {what}: device {worst[0]:.3e}, host {worst[1]:.3e}, "
              f"device - host {worst[2]:.3e}")
        assert np.all(errs[0] <= tol_dev), (what, "device route against the reference")
        assert np.all(errs[1] <= tol_host), (what, "host route against the reference")
        assert np.all(errs[2] <= tol_dev + tol_host), (what, "device route against host route")


def _cap(n_t, dim, d_a, d=2):
    from pulser_amd.engine import reduced_density_dm_splits

    return reduced_density_dm_splits(n_t, dim, d_a, d)


# ---------------------------------------------------------------------------------------------------------------------
# a two-level dephasing run
# ---------------------------------------------------------------------------------------------------------------------
def test_two_level_dephasing_run_is_traced_on_the_device_without_a_read(monkeypatch):
    res = _tri6()
    states = res.states
    lazy = [st for st in states if isinstance(st, LazyState)]
    assert len(lazy) == len(states) - 1 and not isinstance(states[0], LazyState)  # (the initial state is on the host)
    assert len({id(st._store) for st in lazy}) == 1 and all(not st.isket for st in lazy)
    count = _Counters(monkeypatch)
    keep = [1, 2]
    got = res.reduced_states(keep)
    assert got.shape == (len(res), 4, 4) and got.dtype == np.complex128
    assert count.gets == [] and count.bulk == 0  # nothing was read
    assert count.calls == [((len(lazy), 1, 2**N6, 2**N6), (1, 2), 2)]  # one call over the store's tensor
    assert count.ket_calls == []
    assert all(st._q is None and st._store is not None for st in lazy)  # and every state is still a snapshot
    assert lazy[0]._store.device_tensor is not None
    # the entropy is entropy_vn of these very matrices: the same function on the same numbers
    ent = res.entanglement_entropy(keep)
    assert len(count.calls) == 2 and count.calls[1] == count.calls[0] and count.gets == [] and count.bulk == 0
    assert np.array_equal(ent, np.array([entropy_vn(r) for r in got]))
    assert np.array_equal(res.reduced_states(keep), got)  # (and the call is repeatable bit for bit)
    norm = res.reduced_states(keep, normalize=True)
    assert np.max(np.abs(np.trace(norm, axis1=1, axis2=2) - 1.0)) <= 4 * 2.0**-52
    n_calls = len(count.calls)
    # after to_host(): the same values through the host route, no further device call
    res.to_host()
    assert count.bulk == 1
    host = res.reduced_states(keep)
    assert len(count.calls) == n_calls and count.ket_calls == []
    mats = np.array([np.asarray(st) for st in states])
    assert np.array_equal(host, np.array([_ptrace_host(m, False, keep, 2) for m in mats]))
    # 16 summands per entry and a single step of the walk: there is nothing to split (the issue's bound, tol(R, S) each)
    assert _cap(len(lazy), 2**N6, 4) == 1
    _assert_routes_agree(got, mats, keep, 2, 1, "6 atoms, device route and host route after to_host()", host=host)
    # dephasing mixes: the subsystem of a pure product start is pure, later ones are not
    assert ent[0] == 0.0 and np.max(ent) > 1e-3
    assert np.array_equal(res.entanglement_entropy(keep), np.array([entropy_vn(r) for r in host]))


def test_a_state_read_before_the_call_is_served_from_the_host(monkeypatch):
    res = _tri6()
    states = res.states
    read = [3, 7]
    copies = {i: np.asarray(states[i]).copy() for i in read}  # materialises these two
    count = _Counters(monkeypatch)
    got = res.reduced_states([0, 5])
    live = [i for i, st in enumerate(states) if isinstance(st, LazyState) and st._q is None]
    assert not set(read) & set(live) and len(live) == len(states) - 1 - len(read)
    assert count.gets == [] and count.bulk == 0
    assert count.calls == [((len(live), 1, 2**N6, 2**N6), (0, 5), 2)]  # a gathered copy: the live times are not equidistant
    for i in read:
        assert np.array_equal(got[i], _ptrace_host(copies[i], False, [0, 5], 2))
    mats = np.array([np.asarray(st) for st in states])
    _assert_routes_agree(got, mats, [0, 5], 2, _cap(len(live), 2**N6, 4), "6 atoms, two states on the host")
    # every 2nd state read: the rest is a strided view of the store
    res2 = _tri6()
    st2 = res2.states
    for i in range(2, len(st2), 2):
        np.asarray(st2[i])
    got2 = res2.reduced_states([2, 3, 4])
    assert len(count.calls) == 2 and count.calls[1][0][0] == len(st2) // 2
    _assert_routes_agree(got2, np.array([np.asarray(s) for s in st2]), [2, 3, 4], 2, _cap(len(st2) // 2, 2**N6, 8),
                         "every 2nd time")


def test_lazy_state_ptrace_stays_on_the_device(monkeypatch):
    res = _tri6(4)
    st = res.states[-1]
    assert isinstance(st, LazyState) and not st.isket
    count = _Counters(monkeypatch)
    rho = st.ptrace([5, 0])
    assert isinstance(rho, QState) and rho.shape == (4, 4)
    assert count.gets == [] and count.bulk == 0 and st._q is None and st._store is not None
    assert count.calls == [((1, 1, 2**N6, 2**N6), (0, 5), 2)] and count.ket_calls == []
    full = st.ptrace(range(N6))  # dA = D: the matrix itself, still from the device
    assert len(count.calls) == 2 and st._q is None and count.gets == []
    mat = np.asarray(st)  # reads the state
    assert len(count.gets) + count.bulk == 1
    assert np.array_equal(np.asarray(full), mat)
    _assert_routes_agree(np.asarray(rho)[None], mat[None], [0, 5], 2, _cap(1, 2**N6, 4), "LazyState.ptrace")
    # materialised now: the host formula, no device call
    assert np.array_equal(st.ptrace([0, 5]), _ptrace_host(mat, False, [0, 5], 2)) and len(count.calls) == 2
    with pytest.raises(ValueError):
        res.states[-2].ptrace([0, 0])
    assert res.states[-2]._q is None


# ---------------------------------------------------------------------------------------------------------------------
# DeviceState with a device tensor
# ---------------------------------------------------------------------------------------------------------------------
def test_device_state_with_a_device_tensor_is_traced_without_a_copy(monkeypatch):
    import torch

    rng = np.random.default_rng(80)
    a = rng.normal(size=(16, 16)) + 1j * rng.normal(size=(16, 16))  # no symmetry: both triangles are read as they are
    st = DeviceState(tensor=torch.from_numpy(a).cuda())

    def no_copy(self):
        raise AssertionError("full() was called")

    count = _Counters(monkeypatch)
    monkeypatch.setattr(DeviceState, "full", no_copy)
    for keep in ([0], [3, 1], [0, 1, 2], [0, 1, 2, 3]):
        got = st.ptrace(keep)
        sites = sorted(keep)
        assert isinstance(got, QState) and got.shape == (2 ** len(keep),) * 2
        assert count.calls[-1] == ((1, 1, 16, 16), tuple(sites), 2)
        _assert_routes_agree(np.asarray(got)[None], a[None], sites, 2, _cap(1, 16, 2 ** len(keep)), f"DeviceState {keep}")
    assert np.array_equal(np.asarray(st.ptrace(range(4))), a)  # dA = D: served, and exact
    got4 = DeviceState(tensor=torch.from_numpy(a).cuda()).ptrace([0], local_dim=4)  # two four-level atoms
    _assert_routes_agree(np.asarray(got4)[None], a[None], [0], 4, _cap(1, 16, 4, 4), "DeviceState local_dim=4")
    with pytest.raises(ValueError):
        st.ptrace([4])
    assert count.gets == [] and count.bulk == 0 and count.ket_calls == []


def test_device_state_falls_back_to_full_beyond_64_rows(monkeypatch):
    import torch

    rng = np.random.default_rng(81)
    a = rng.normal(size=(256, 256)) + 1j * rng.normal(size=(256, 256))
    st = DeviceState(tensor=torch.from_numpy(a).cuda())
    count = _Counters(monkeypatch)
    fulls = []
    real_full = DeviceState.full

    def counted_full(self):
        fulls.append(1)
        return real_full(self)

    monkeypatch.setattr(DeviceState, "full", counted_full)
    keep = list(range(1, 8))  # dA = 128
    got = st.ptrace(keep)
    assert got.shape == (128, 128) and fulls == [1] and count.calls == []
    assert np.array_equal(np.asarray(got), _ptrace_host(a, False, keep, 2))
    small = st.ptrace([0, 7])  # 4 rows: back on the device
    assert fulls == [1] and len(count.calls) == 1
    _assert_routes_agree(np.asarray(small)[None], a[None], [0, 7], 2, _cap(1, 256, 4), "DeviceState 256, 4 rows")
    # the ket form is traced as a ket, as before
    psi = rng.normal(size=16) + 1j * rng.normal(size=16)
    assert np.array_equal(np.asarray(DeviceState(ket=psi).ptrace([1, 2])), _ptrace_host(psi.reshape(-1, 1), True, [1, 2], 2))
    assert len(count.calls) == 1 and count.ket_calls == []


# ---------------------------------------------------------------------------------------------------------------------
# the general path: multi-level and XY master-equation runs with general_density_snapshots=True
# ---------------------------------------------------------------------------------------------------------------------
def _all4_run():
    """The inputs behind tests/golden/general_oracle_all4_me.npz (3-level "all" basis on a 2 x 2 square, D = 81) with the
    noise model that makes its collapse operators: relaxation and both dephasing channels."""
    from pulser_amd import problem as P

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_general_fixtures as G

    fx = np.load(os.path.join(os.path.dirname(G.__file__), "general_oracle_all4_me.npz"))
    assert str(fx["input_sha256"]) == G.digest_case("all4_me"), "generator drifted from the committed fixture"
    prob = G.multilevel_problem(P.register_coords(P.square_rect(2, 2), 6.0), 161, 10, local=(1,))
    nm = NoiseModel(relaxation_rate=0.5, dephasing_rate=0.7, hyperfine_dephasing_rate=0.3)
    return QutipEmulator(_inputs_from_problem(prob), sampling_rate=1.0, noise_model=nm), 3, 4, [3, 0]


def _xy_run():
    """An XY master-equation run: the ``noisy_xy_0`` inputs (4 atoms, D = 16) with dephasing."""
    from pulser_amd.hamiltonian_data import SequenceInputs

    prob, _ = load_fixture("noisy_xy_0.npz")
    return (QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), noise_model=NoiseModel(dephasing_rate=0.05)), 2, 4,
            [1, 2])


@pytest.mark.parametrize("case", ["all4", "xy"])
def test_general_path_run_with_density_snapshots_takes_the_device_route(case, monkeypatch):
    emu, d, n, keep = {"all4": _all4_run, "xy": _xy_run}[case]()
    emu.set_evaluation_times(list(np.linspace(0.0, emu._tot_duration / 1000, 11)))
    with pytest.warns(DeprecationWarning):
        plain = emu.run()
    with pytest.warns(DeprecationWarning):
        kept = emu.run(general_density_snapshots=True)
    dim = d**n
    assert kept._dim == d and all(isinstance(st, LazyState) and st.shape == (dim, dim) for st in kept.states[1:])
    assert all(not isinstance(st, LazyState) for st in plain.states)
    count = _Counters(monkeypatch)
    sites = tuple(sorted(keep))
    got = kept.reduced_states(keep)
    d_a = d ** len(keep)
    assert got.shape == (len(kept), d_a, d_a)
    n_dev = len(kept) - 1
    assert count.gets == [] and count.bulk == 0 and count.ket_calls == []
    assert count.calls == [((n_dev, 1, dim, dim), sites, d)]
    assert all(st._q is None for st in kept.states[1:])
    host = plain.reduced_states(keep)  # QState states: the host formula
    assert len(count.calls) == 1
    # the host formula on the fetched matrices of the SAME run
    mats = np.array([np.asarray(st) for st in kept.states])
    assert count.bulk + len(count.gets) > 0
    fetched = np.array([_ptrace_host(m, False, sites, d) for m in mats])
    _assert_routes_agree(got, mats, sites, d, _cap(n_dev, dim, d_a, d), f"{case}: device route and the host formula on "
                         "the fetched matrices", host=fetched)
    assert np.array_equal(kept.reduced_states(keep), fetched) and len(count.calls) == 1  # read now: the host route
    assert host.shape == got.shape
    assert np.array_equal(kept.entanglement_entropy(keep), np.array([entropy_vn(r) for r in fetched]))


# ---------------------------------------------------------------------------------------------------------------------
# the matrices of the committed general-path master-equation fixtures, behind a store as a run holds them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,keep", [("all4_me", [0, 2]), ("xy5_me", [1, 4])])
def test_fixture_matrices_behind_a_store_take_the_device_route(name, keep, monkeypatch):
    """tests/golden/general_oracle_all4_me.npz / general_oracle_xy5_me.npz are problems of the general engine (no
    sequence inputs to build an emulator from): they are solved by ``GeneralEngine`` and held the way
    ``run(general_density_snapshots=True)`` holds its matrices - ``LazyState``s of shape (D, D) over a ``[T, 1, D, D]``
    view of the solved tensor."""
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_general_fixtures as G

    fx = np.load(os.path.join(os.path.dirname(G.__file__), f"general_oracle_{name}.npz"))
    assert str(fx["input_sha256"]) == G.digest_case(name), f"{name}: generator drifted from the committed fixture"
    probs, mesolve, psi, times = G.build(name)
    assert mesolve
    prob = probs[0]
    d, n = len(prob["eigenbasis"]), int(prob["n_qudits"])
    dim = d**n
    with GeneralEngine(lower_general(prob, mesolve=True)) as eng:
        snaps = eng.solve(eng.new_state(psi), times)
    n_dev = len(times) - 1
    assert tuple(snaps.shape) == (n_dev, 1, dim * dim)
    oracle = np.asarray(fx["states"])[0]
    assert float(np.max(np.abs(snaps.cpu().numpy()[:len(oracle), 0] - oracle))) < 1e-7  # the fixture's matrices
    store = SnapshotStore(snaps.reshape(n_dev, 1, dim, dim))
    qids = tuple(f"q{k}" for k in range(n))
    basis = "XY" if d == 2 else "all"
    first = QState(np.outer(psi, np.conj(psi)))
    results = [StateResult(qids, "XY" if d == 2 else "ground-rydberg", first if i == 0 else LazyState(store, i - 1, 0, (dim, dim)),
                           d == 2, evaluation_time=float(i) / n_dev) for i in range(len(times))]
    res = CoherentResults(results, n, basis, np.asarray(times), "XY" if d == 2 else "ground-rydberg", None)
    assert res._dim == d
    count = _Counters(monkeypatch)
    sites = tuple(sorted(keep))
    d_a = d ** len(keep)
    got = res.reduced_states(keep)
    assert count.calls == [((n_dev, 1, dim, dim), sites, d)] and count.gets == [] and count.bulk == 0
    assert all(st._q is None for st in res.states[1:])
    mats = np.array([np.asarray(st) for st in res.states])
    fetched = np.array([_ptrace_host(m, False, sites, d) for m in mats])
    _assert_routes_agree(got, mats, sites, d, _cap(n_dev, dim, d_a, d), f"{name}: device route and host formula",
                         host=fetched)
    assert np.array_equal(res.reduced_states(keep), fetched) and len(count.calls) == 1

"""GPU: the partial trace at the level of results - ``SimulationResults.reduced_states`` / ``entanglement_entropy`` and
``LazyState.ptrace`` over device snapshots against the host route on the same states, and
``run(mc_ensemble=True, mc_ensemble_subsystems=...)`` against the reference over the very kets the run integrated.

Bounds (none fitted to what the code gives).  The device route and the host route read the SAME amplitudes (a state on
the host is a copy of its snapshot), so they differ by their own rounding only: ``tol_reduced(R + n_split, S)`` of
tests/ptrace_ref.py for the kernel - with the engine's cap ``min(1024 // T, D // 512)`` (at least 1) standing in for
the split the library chose - plus the same rule for the host's matmul, ``tol_reduced(R, S)``: it sums the same 2 R
products per part in some order.  Real and imaginary parts are compared apart.
"""
from __future__ import annotations

import numpy as np
import pytest

from helpers import load_fixture, with_anneal_samples
from observe_ref import LD
from ptrace_ref import ref_reduced, tol_reduced
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QState, QutipEmulator, Solver, entropy_vn
from pulser_amd.results import EnsembleState, LazyState, SnapshotStore

pytestmark = pytest.mark.gpu

N8 = 8


class _Counters:
    """``SnapshotStore.get`` / ``fetch_all`` calls and the shapes handed to ``engine.reduced_density``."""

    def __init__(self, monkeypatch):
        from pulser_amd import engine

        self.gets, self.bulk, self.calls = [], 0, []
        get, fetch_all, real = SnapshotStore.get, SnapshotStore.fetch_all, engine.reduced_density

        def counted_get(store, i, b):
            self.gets.append((i, b))
            return get(store, i, b)

        def counted_fetch_all(store):
            self.bulk += 1
            return fetch_all(store)

        def counted(states, keep, local_dim=2, out=None, n_split=0):
            self.calls.append((tuple(states.shape), tuple(keep), local_dim))
            return real(states, keep, local_dim, out, n_split)

        monkeypatch.setattr(SnapshotStore, "get", counted_get)
        monkeypatch.setattr(SnapshotStore, "fetch_all", counted_fetch_all)
        monkeypatch.setattr(engine, "reduced_density", counted)


def _chain8(n_times=40):
    prob, _ = load_fixture("cfg2_chain8_anneal.npz")
    inputs = _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")
    emu = QutipEmulator(inputs, sampling_rate=1.0)
    emu.set_evaluation_times(list(np.linspace(0.0, emu._tot_duration / 1000, n_times)))
    with pytest.warns(DeprecationWarning):
        res = emu.run()
    assert len(res) >= n_times
    return res


def _assert_routes_agree(got, kets, keep, d, split_cap, what):
    """``got`` [T, dA, dA] against the reference over the host copies ``kets`` [T, D], within the kernel's bound plus
    the host formula's."""
    kets = np.asarray(kets)
    d_a = d ** len(keep)
    r = kets.shape[1] // d_a
    (re, im), s_re, s_im = ref_reduced(kets[:, None, :], np.zeros((len(kets), d_a, d_a), dtype=complex), keep, d)
    worst = 0.0
    for g, want, s in ((got.real, re, s_re), (got.imag, im, s_im)):
        tol = tol_reduced(r + split_cap, s) + tol_reduced(r, s)
        err = np.abs(g.astype(LD) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.max(np.where(err > 0, err / tol.astype(LD), 0))))
        assert np.all(err <= tol), what
    print(f"RATIO reduced_states {what}: {worst:.3e}")


def test_two_level_run_is_traced_on_the_device_without_a_read(monkeypatch):
    res = _chain8()
    states = res.states
    assert all(isinstance(st, LazyState) for st in states[1:]) and len({id(st._store) for st in states[1:]}) == 1
    count = _Counters(monkeypatch)
    keep = [0, 1, 2, 3]
    got = res.reduced_states(keep)
    assert got.shape == (len(res), 16, 16) and got.dtype == np.complex128
    n_dev = sum(isinstance(st, LazyState) for st in states)
    assert count.gets == [] and count.bulk == 0  # nothing was read
    assert count.calls == [((n_dev, 1, 2**N8), (0, 1, 2, 3), 2)]  # one call over the store's tensor
    assert all(st._q is None for st in states if isinstance(st, LazyState))  # and every state is still a snapshot
    norm = res.reduced_states(keep, normalize=True)
    assert np.max(np.abs(np.trace(norm, axis1=1, axis2=2) - 1.0)) <= 16 * 2.0**-52
    ent = res.entanglement_entropy(keep)
    comp = res.entanglement_entropy([4, 5, 6, 7])
    one = res.entanglement_entropy([0])
    assert count.calls[-1][1] == (0,) and len(count.calls) == 5 and count.gets == [] and count.bulk == 0
    # after to_host(): the same values through the host route, no device call
    res.to_host()
    assert count.bulk == 1
    host = res.reduced_states(keep)
    assert len(count.calls) == 5
    # the per-state host formula on the same states
    kets = np.array([np.asarray(st).reshape(-1) for st in states])
    per_state = np.array([QState(k).ptrace(keep) for k in kets])
    assert np.array_equal(host, per_state)
    cap = max(1, min(1024 // n_dev, 2**N8 // 512))
    _assert_routes_agree(got, kets, keep, 2, cap, "8 atoms, device against the reference")
    _assert_routes_agree(host, kets, keep, 2, cap, "8 atoms, host route against the reference")
    # entropies: 0 for the all-ground initial state; a pure state's two halves agree
    assert ent.shape == (len(res),) and ent[0] == 0.0
    assert np.max(ent) > 0.1  # (the anneal entangles the chain)
    assert np.allclose(ent, comp, rtol=0, atol=1e-10)
    big = res.entanglement_entropy(range(1, 8))  # dA = 128: beyond the device route, still answered
    assert len(count.calls) == 5 and big.shape == ent.shape and big[0] == 0.0
    assert np.allclose(big, one, rtol=0, atol=1e-10)  # 7 atoms against the remaining one


def test_a_state_read_before_the_call_is_served_from_the_host(monkeypatch):
    res = _chain8(12)
    states = res.states
    read = [3, 7]
    copies = {i: np.asarray(states[i]).copy() for i in read}  # materialises these two
    count = _Counters(monkeypatch)
    got = res.reduced_states([1, 6])
    live = [i for i, st in enumerate(states) if isinstance(st, LazyState) and st._q is None]
    assert not set(read) & set(live) and len(live) == len(states) - 1 - len(read)
    assert count.gets == [] and count.bulk == 0
    assert count.calls == [((len(live), 1, 2**N8), (1, 6), 2)]  # a gathered copy: the live times are not equidistant
    for i in read:
        assert np.array_equal(got[i], QState(copies[i]).ptrace([1, 6]))
    kets = np.array([np.asarray(st).reshape(-1) for st in states])
    _assert_routes_agree(got, kets, [1, 6], 2, 1, "8 atoms, two states on the host")
    # every 2nd state read: the rest is a strided view of the store
    res2 = _chain8(12)
    st2 = res2.states
    for i in range(2, len(st2), 2):
        np.asarray(st2[i])
    got2 = res2.reduced_states([0, 7])
    _assert_routes_agree(got2, np.array([np.asarray(s).reshape(-1) for s in st2]), [0, 7], 2, 1, "every 2nd time")


def test_lazy_state_ptrace_stays_on_the_device(monkeypatch):
    res = _chain8(6)
    st = res.states[-1]
    assert isinstance(st, LazyState)
    count = _Counters(monkeypatch)
    rho = st.ptrace([7, 0])
    assert isinstance(rho, QState) and rho.shape == (4, 4)
    assert count.gets == [] and count.bulk == 0 and st._q is None and len(count.calls) == 1
    ket = np.asarray(st).reshape(-1)
    _assert_routes_agree(np.asarray(rho)[None], ket[None], [0, 7], 2, 1, "LazyState.ptrace")
    assert np.array_equal(st.ptrace([0, 7]), QState(ket).ptrace([0, 7]))  # materialised now: the host formula
    with pytest.raises(ValueError):
        res.states[-2].ptrace([0, 0])
    # 7 atoms (dA = 128) over live snapshots: no device call, the states are read and the host formula answers
    calls = len(count.calls)
    big = res.entanglement_entropy(range(1, 8))
    assert len(count.calls) == calls and len(count.gets) + count.bulk > 0
    assert np.allclose(big, res.entanglement_entropy([0]), rtol=0, atol=1e-10)


def test_general_path_run_with_device_snapshots_takes_the_device_route(monkeypatch):
    import os
    import sys

    from pulser_amd import problem as P

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_general_fixtures as G

    inputs = _inputs_from_problem(G.multilevel_problem(P.register_coords(P.square_rect(1, 3), 6.0), 121, 78, local=(0,)))
    emu = QutipEmulator(inputs, sampling_rate=1.0)
    emu.set_evaluation_times(list(np.linspace(0.0, 0.12, 13)))
    with pytest.warns(DeprecationWarning):
        plain = emu.run()
    with pytest.warns(DeprecationWarning):
        kept = emu.run(general_device_snapshots=True)
    assert kept._dim == 3 and all(isinstance(st, LazyState) for st in kept.states[1:])
    count = _Counters(monkeypatch)
    got = kept.reduced_states([2, 0])
    assert got.shape == (len(kept), 9, 9)
    assert count.gets == [] and count.bulk == 0 and len(count.calls) == 1 and count.calls[0][1:] == ((0, 2), 3)
    host = plain.reduced_states([0, 2])  # QState states: the host formula
    assert len(count.calls) == 1
    kets = np.array([np.asarray(st).reshape(-1) for st in plain.states])
    _assert_routes_agree(got, kets, [0, 2], 3, 1, "3 three-level atoms, device")
    _assert_routes_agree(host, kets, [0, 2], 3, 1, "3 three-level atoms, host")
    assert np.allclose(kept.entanglement_entropy([1]), plain.entanglement_entropy([0, 2]), rtol=0, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# quantum-jump ensembles
# ---------------------------------------------------------------------------------------------------------------------
NTRAJ = 60
NOISE = dict(dephasing_rate=0.3, relaxation_rate=0.2)
SUBSYSTEMS = [(0, 1), (3, 1, 2), (2,)]


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


def test_ensemble_run_reduces_the_registered_subsystems_from_its_kets(monkeypatch):
    prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
    inputs = _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")
    kets = _capture_kets(monkeypatch)
    runs = []
    for option in ({}, {"mc_ensemble_subsystems": SUBSYSTEMS}):
        emu = QutipEmulator(inputs, noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=NTRAJ,
                            evaluation_times=[0.5, 1.2, 2.0])
        with pytest.warns(DeprecationWarning):
            runs.append(emu.run(seeds=1, mc_ensemble=True, **option))
    without, res = runs
    assert len(kets) == 2 and np.array_equal(kets[0], kets[1])  # the same trajectories, bit for bit
    x = kets[1]  # [T - 1, NTRAJ, 16]
    assert all(isinstance(st, EnsembleState) for st in res.states) and len(res) == x.shape[0] + 1
    # every existing field is unchanged, bit for bit
    for a, b in zip(without.states, res.states):
        assert a.subsystems == () and b.subsystems == ((0, 1), (1, 2, 3), (2,))
        assert np.array_equal(a.diag(), b.diag()) and np.array_equal(a.occupation, b.occupation)
        assert np.array_equal(a.correlation, b.correlation) and (a.energy, a.energy2, a.norm2) == (b.energy, b.energy2, b.norm2)
    init = np.zeros(16, dtype=complex)
    init[np.argmax(np.abs(res.states[0].diag()))] = 1.0  # (the run starts in a basis state)
    for keep in SUBSYSTEMS:
        keep = tuple(sorted(keep))
        d_a, r = 2 ** len(keep), 16 // 2 ** len(keep)
        got = res.reduced_states(keep)
        assert got.shape == (len(res), d_a, d_a)
        # time 0: the initial ket, summed NTRAJ times and divided again - exact for a basis state
        assert np.array_equal(got[0], QState(init).ptrace(keep))
        (re, im), s_re, s_im = ref_reduced(x, np.zeros((x.shape[0], d_a, d_a), dtype=complex), keep, 2)
        for g, want, s in ((got[1:].real, re, s_re), (got[1:].imag, im, s_im)):
            # the sums within the kernel's bound (no split at 16 amplitudes), then one division by NTRAJ: one rounding
            tol = tol_reduced(NTRAJ * r, s) / NTRAJ + 2.0**-53 * np.abs(want.astype(np.float64)) / NTRAJ
            assert np.all(np.abs(g.astype(LD) - want / NTRAJ) <= tol), keep
        for i, st in enumerate(res.states):
            assert np.array_equal(st.ptrace(keep), got[i])
            assert np.array_equal(got[i], got[i].conj().T)  # exactly Hermitian
            # the diagonal of rho_A is the marginal of the ensemble diagonal
            marg = np.asarray(QState(np.diag(st.diag())).ptrace(keep)).diagonal()
            assert np.allclose(got[i].diagonal(), marg, rtol=0, atol=1e-14)
    ent = res.entanglement_entropy((0, 1))
    assert ent[0] == 0.0 and np.all(ent[1:] > 0) and ent[-1] == entropy_vn(res.states[-1].ptrace((1, 0)))
    with pytest.raises(NotImplementedError, match="mc_ensemble_subsystems"):
        res.reduced_states((0, 2))
    with pytest.raises(NotImplementedError, match="mc_ensemble_subsystems"):
        without.reduced_states((0, 1))

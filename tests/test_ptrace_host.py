"""CPU: the host side of the partial trace - the ``ryd_reduced_density`` declaration, binding and export, its argument
checks (decided before the device is touched), ``QState.ptrace`` against tests/ptrace_ref.py, ``entropy_vn``,
``EnsembleState.ptrace`` built from arrays, and the validation of ``run(mc_ensemble_subsystems=...)``."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from helpers import load_fixture, with_anneal_samples
from ptrace_ref import ref_reduced
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QState, QutipEmulator, Solver, entropy_vn
from pulser_amd import _lib
from pulser_amd.results import CoherentResults, DeviceState, EnsembleState, StateResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["const void* states_dev", "int32_t n_times", "int32_t n_batch", "int64_t stride_t", "int64_t stride_b",
             "int64_t dim", "int32_t local_dim", "int32_t n_sites", "const int32_t* keep", "int32_t n_keep",
             "void* out_dev", "int32_t n_split", "void* scratch_dev", "int64_t scratch_bytes", "int32_t device",
             "void* stream"]


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_reduced_density\(([^;]*)\);", header)
    assert m, "ryd_reduced_density is not declared in include/rydemu.h"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split(",")]
    assert args == PROTOTYPE, args
    restype, argtypes = _lib.SYMBOLS["ryd_reduced_density"]
    want = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want
    # (loading the library needs no device)
    assert hasattr(_lib.load(), "ryd_reduced_density")
    assert _lib.RYD_ABI_VERSION == 1 and re.search(r"#define\s+RYD_ABI_VERSION\s+1\b", header)


def test_abi_rejects_bad_arguments_without_a_device():
    """Every RYD_ERR_INVALID case is decided before the device is touched (test_gpu_reduced_density repeats them with
    real pointers).  Arguments: states, n_times, n_batch, stride_t, stride_b, dim, local_dim, n_sites, keep, n_keep, out,
    n_split, scratch, scratch_bytes."""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data

    def keep(*sites):
        a = np.array(sites, dtype=np.int32)
        return a, a.ctypes.data, len(sites)

    k1, pk1, _ = keep(1)
    good = (p, 1, 1, 8, 8, 8, 2, 3, pk1, 1, p, 1, None, 0)
    bad = {
        "states null": (None,) + good[1:],
        "out null": good[:10] + (None,) + good[11:],
        "keep null": good[:8] + (None,) + good[9:],
        "n_times < 0": (p, -1) + good[2:],
        "n_batch = 0": (p, 1, 0) + good[3:],
        "n_batch < 0": (p, 1, -2) + good[3:],
        "dim != d^n": good[:5] + (9,) + good[6:],
        "dim != d^n (n)": good[:7] + (4,) + good[8:],
        "local_dim 1": good[:6] + (1,) + good[7:],
        "local_dim 5": good[:6] + (5,) + good[7:],
        "stride_t < dim": (p, 2, 1, 7) + good[4:],
        "stride_b < dim": (p, 1, 2, 8, 7) + good[5:],
        "n_keep = 0": good[:9] + (0,) + good[10:],
        "n_keep < 0": good[:9] + (-1,) + good[10:],
        "n_split < 0": good[:11] + (-1,) + good[12:],
        "split without scratch": good[:11] + (2, None, 0),
        "scratch too small": good[:11] + (2, p, 2 * 4 * 16 - 1),
        "null states, no times": (None, 0) + good[2:],
    }
    for sites in ((3,), (-1,), (1, 1), (2, 1), (0, 1, 2, 3)):  # out of range, repeated, descending, more than n_sites
        arr, ptr, cnt = keep(*sites)
        bad[f"keep {sites}"] = good[:8] + (ptr, cnt) + good[10:]
        bad[f"keep {sites}"] += (arr,)  # (keeps the array alive; cut off below)
    for name, args in bad.items():
        assert lib.ryd_reduced_density(*args[:14], 0, None) == -1, name  # RYD_ERR_INVALID
        assert "reduced_density" in lib.ryd_last_error().decode(), name
    # dA > 64: seven of eight qubits, four of five qutrits, four four-level atoms
    for d, n, cnt in ((2, 8, 7), (3, 5, 4), (4, 4, 4)):
        arr, ptr, _ = keep(*range(cnt))
        assert lib.ryd_reduced_density(p, 1, 1, d**n, d**n, d**n, d, n, ptr, cnt, p, 1, None, 0, 0, None) == -1
        assert "64" in lib.ryd_last_error().decode()
    # n_times = 0: nothing to do, nothing launched - with or without a split
    assert lib.ryd_reduced_density(p, 0, 1, 8, 8, 8, 2, 3, pk1, 1, p, 1, None, 0, 0, None) == 0
    assert lib.ryd_reduced_density(p, 0, 1, 8, 8, 8, 2, 3, pk1, 1, p, 0, None, 0, 0, None) == 0
    assert lib.ryd_reduced_density(p, 0, 1, 8, 8, 8, 2, 3, pk1, 1, p, 3, p, 0, 0, None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# QState.ptrace, DeviceState.ptrace
# ---------------------------------------------------------------------------------------------------------------------
def _rand(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _ref(psi, keep, d):
    d_a = d ** len(keep)
    (re, im), _, _ = ref_reduced(psi.reshape(1, 1, -1), np.zeros((1, d_a, d_a), dtype=complex), keep, d)
    return (re.astype(np.float64) + 1j * im.astype(np.float64))[0]


@pytest.mark.parametrize("d,n,keep", [(2, 5, [3, 0]), (2, 5, [4]), (2, 6, [5, 2, 3, 0, 1, 4]), (3, 4, [2, 1]),
                                      (3, 3, [0]), (4, 3, [2, 0]), (4, 2, [1])])
def test_qstate_ptrace_matches_the_reference_for_kets_and_density_matrices(d, n, keep):
    rng = np.random.default_rng(d * 100 + n)
    psi = _rand(rng, d**n)
    want = _ref(psi, keep, d)
    scale = np.vdot(psi, psi).real
    got = QState(psi).ptrace(keep, d)
    assert isinstance(got, QState) and got.isoper and got.shape == (d ** len(keep),) * 2
    assert np.allclose(got, want, rtol=0, atol=1e-13 * scale)
    assert np.allclose(QState(np.outer(psi, psi.conj())).ptrace(keep, d), want, rtol=0, atol=1e-13 * scale)
    # a mixture: the partial trace is linear
    phi = _rand(rng, d**n)
    mix = 0.25 * np.outer(psi, psi.conj()) + 0.75 * np.outer(phi, phi.conj())
    assert np.allclose(QState(mix).ptrace(keep, d), 0.25 * want + 0.75 * _ref(phi, keep, d), rtol=0,
                       atol=1e-13 * (scale + np.vdot(phi, phi).real))
    # the same through the other order of the sites and through any iterable
    assert np.array_equal(QState(psi).ptrace(tuple(sorted(keep)), d), got)
    assert np.array_equal(QState(psi).ptrace(iter(keep), d), got)
    if d == 2:
        assert np.array_equal(QState(psi).ptrace(keep), got)  # local_dim defaults to 2
        assert np.allclose(DeviceState(ket=psi).ptrace(keep), want, rtol=0, atol=1e-13 * scale)


def test_qstate_ptrace_refuses_bad_arguments():
    st = QState(np.ones(8))
    for keep in ([0, 0], [3], [-1], [], [0.5], 1):
        with pytest.raises(ValueError):
            st.ptrace(keep)
    with pytest.raises(ValueError, match="power"):
        st.ptrace([0], local_dim=3)
    with pytest.raises(ValueError, match="power"):
        QState(np.eye(6)).ptrace([0])
    assert QState(np.ones(9)).ptrace([1], local_dim=3).shape == (3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# entropy_vn
# ---------------------------------------------------------------------------------------------------------------------
def test_entropy_edge_cases():
    pure = np.zeros((4, 4))
    pure[2, 2] = 1.0
    s = entropy_vn(pure)
    assert s == 0.0 and np.signbit(s) == False and isinstance(s, float)  # noqa: E712
    assert entropy_vn(np.diag([1.0, -1e-18])) == 0.0  # the negative eigenvalue is clipped, 0 log 0 = 0
    assert entropy_vn(np.diag([0.5, 0.5, -1e-18])) == pytest.approx(1.0, abs=1e-15)
    rng = np.random.default_rng(0)
    a = _rand(rng, 5, 5)
    rho = a @ a.conj().T
    s = entropy_vn(rho)
    assert 0 < s < np.log2(5)
    for scale in (3.0, 1e-9, 2.0**40):
        assert entropy_vn(scale * rho) == pytest.approx(s, rel=1e-12)
    assert entropy_vn(rho, base=np.e) == pytest.approx(s * np.log(2), rel=1e-13)
    assert entropy_vn(np.eye(8)) == pytest.approx(3.0, abs=1e-14)
    with pytest.raises(ValueError):
        entropy_vn(np.ones((2, 3)))


# ---------------------------------------------------------------------------------------------------------------------
# EnsembleState from arrays
# ---------------------------------------------------------------------------------------------------------------------
N, NTRAJ = 4, 7
QIDS = tuple(f"q{k}" for k in range(N))


def _ensemble(seed=0, subsystems=((0, 1), (1, 3))):
    rng = np.random.default_rng(seed)
    kets = _rand(rng, NTRAJ, 2**N)
    kets /= np.linalg.norm(kets, axis=1)[:, None]
    sums = [sum(np.asarray(QState(k).ptrace(sub)) for k in kets) for sub in subsystems]
    kw = dict(occupation=np.full(N, 0.5), correlation=np.full((N, N), 0.25), energy=1.5, energy2=4.0, norm2=1.0,
              occupation_stderr=np.full(N, 0.1))
    st = EnsembleState((np.abs(kets) ** 2).sum(axis=0), NTRAJ, subsystems=subsystems, reduced=sums, **kw)
    return st, kets, sums, kw


def test_ensemble_state_serves_registered_subsystems_and_refuses_the_rest():
    st, kets, sums, kw = _ensemble()
    assert st.subsystems == ((0, 1), (1, 3))
    for keep, total in (((0, 1), sums[0]), ([1, 0], sums[0]), ((3, 1), sums[1])):
        got = st.ptrace(keep)
        assert isinstance(got, QState) and got.isoper and got.shape == (4, 4)
        assert np.array_equal(got, total / NTRAJ)  # the sums, divided by n_trajectories - not by norm2
        assert abs(got.tr() - 1) < 1e-14
    rho = np.einsum("bi,bj->ij", kets, kets.conj()) / NTRAJ
    assert np.allclose(st.ptrace((1, 3)), QState(rho).ptrace((1, 3)), rtol=0, atol=1e-14)
    for keep in ((0,), (0, 1, 3), (2, 3), ()):
        with pytest.raises(NotImplementedError, match="mc_ensemble_subsystems"):
            st.ptrace(keep)
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        st.full()
    with pytest.raises(ValueError):
        EnsembleState(np.ones(16), NTRAJ, subsystems=[(0,)], reduced=[], **kw)
    # without the new arguments: as before
    plain = EnsembleState(np.ones(16), NTRAJ, **kw)
    assert plain.subsystems == () and plain.reduced == ()
    with pytest.raises(NotImplementedError, match="mc_ensemble_subsystems"):
        plain.ptrace((0,))


def test_results_of_an_ensemble_serve_registered_subsystems_only():
    pairs = [_ensemble(1), _ensemble(2)]
    rs = [StateResult(QIDS, "ground-rydberg", p[0], True, evaluation_time=t) for p, t in zip(pairs, (0.0, 1.0))]
    res = CoherentResults(rs, N, "ground-rydberg", np.array([0.0, 0.1]), "ground-rydberg", None)
    got = res.reduced_states([3, 1])
    assert got.shape == (2, 4, 4)
    for k, p in enumerate(pairs):
        assert np.array_equal(got[k], p[2][1] / NTRAJ)
    ent = res.entanglement_entropy((0, 1))
    assert ent.shape == (2,) and np.all(ent > 0) and np.all(ent <= 2.0)
    assert ent[0] == pytest.approx(entropy_vn(pairs[0][2][0]), rel=1e-12)  # (entropy_vn normalises: the sum serves too)
    norm = res.reduced_states((0, 1), normalize=True)
    assert np.allclose(np.trace(norm, axis1=1, axis2=2), 1.0, rtol=0, atol=1e-15)
    with pytest.raises(NotImplementedError, match="mc_ensemble_subsystems"):
        res.reduced_states((2,))
    with pytest.raises(NotImplementedError, match="mc_ensemble_subsystems"):
        res.entanglement_entropy((0, 2))


def test_results_on_the_host_use_the_host_formula():
    rng = np.random.default_rng(3)
    kets = _rand(rng, 3, 2**N)
    rs = [StateResult(QIDS, "ground-rydberg", QState(k), True, evaluation_time=t) for k, t in zip(kets, (0.0, 0.5, 1.0))]
    res = CoherentResults(rs, N, "ground-rydberg", np.array([0.0, 0.05, 0.1]), "ground-rydberg", None)
    got = res.reduced_states((2, 0))
    for k in range(3):
        assert np.array_equal(got[k], QState(kets[k]).ptrace((0, 2)))
    a, b = res.entanglement_entropy((0, 2)), res.entanglement_entropy((1, 3))
    assert np.allclose(a, b, rtol=0, atol=1e-10)  # a pure state: the two halves agree
    for keep in ([], [0, 0], [4]):
        with pytest.raises(ValueError):
            res.reduced_states(keep)


# ---------------------------------------------------------------------------------------------------------------------
# run(mc_ensemble_subsystems=...): refused before anything is solved
# ---------------------------------------------------------------------------------------------------------------------
class _SolveStarted(Exception):
    pass


def _emulator(monkeypatch):
    prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
    inputs = _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")
    emu = QutipEmulator(inputs, noise_model=NoiseModel(dephasing_rate=0.3, relaxation_rate=0.2), solver=Solver.MCSOLVER,
                        n_trajectories=12, evaluation_times="Minimal")

    def no_solve(*args, **kw):
        raise _SolveStarted

    monkeypatch.setattr(emu, "_solve_batch", no_solve)
    return emu


@pytest.mark.parametrize("subsystems", [[(0, 0)], [(0, 1), (4,)], [(-1,)], [()], [(0.5,)], [("a",)], [3],
                                        [(0, 1), (1, True)]])
def test_run_refuses_bad_subsystems_before_any_solve(subsystems, monkeypatch):
    emu = _emulator(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        with pytest.raises(ValueError, match="mc_ensemble_subsystems"):
            emu.run(mc_ensemble=True, mc_ensemble_subsystems=subsystems)


def test_run_accepts_good_subsystems_and_limits_their_size(monkeypatch):
    emu = _emulator(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        with pytest.raises(_SolveStarted):  # valid: the (stand-in) solve is reached
            emu.run(mc_ensemble=True, mc_ensemble_subsystems=[(1, 0), [2], range(4)])
    assert emu._ensemble_subsystems({"mc_ensemble_subsystems": [(1, 0), [2], range(4)]}) == [(0, 1), (2,), (0, 1, 2, 3)]
    assert emu._ensemble_subsystems({}) == []
    # 2^k <= 64: seven sites are refused whatever the register (the size check of a 7-atom register)
    emu._hamiltonian_data = type("H", (), {"n_qudits": 8})()
    assert emu._ensemble_subsystems({"mc_ensemble_subsystems": [range(6)]}) == [tuple(range(6))]
    with pytest.raises(ValueError, match="64"):
        emu._ensemble_subsystems({"mc_ensemble_subsystems": [range(7)]})
    assert "mc_ensemble_subsystems" in QutipEmulator.run.__doc__

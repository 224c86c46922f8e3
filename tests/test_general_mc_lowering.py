"""Host side of quantum jumps on the general path (``run(..., general_jumps=True)``), no GPU needed: the argument
checks of ``ryd_general_set_collapse`` and of ``GeneralEngine.set_collapse``, the local collapse operators of
``lower_general(..., with_collapse=True)`` against the oracle's placed operators, and the emulator's routing with
and without the option."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from helpers import load_fixture
from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd import _lib
from pulser_amd._lib import RydError
from pulser_amd.engine import check_collapse_args
from pulser_amd.general import lower_general

DEPOL = np.array([[0.3, 0.5 - 0.2j, 0.0], [0.1j, -0.3, 0.2], [0.0, 0.0, 0.4]])


def _set_collapse(h, local_dim, n_atoms, ops):
    m = np.ascontiguousarray(np.asarray(ops, dtype=np.complex128))
    _lib.check(_lib.load().ryd_general_set_collapse(h, local_dim, n_atoms, len(m), m.ctypes.data if len(m) else None))


@pytest.mark.parametrize("local_dim,n_ops,match", [(1, 1, "local_dim=1"), (5, 1, "local_dim=5"), (9, 2, "local_dim=9"),
                                                   (3, 17, "n_ops=17"), (2, -1, "n_ops=-1")])
def test_abi_rejects_bad_arguments_before_touching_the_handle(local_dim, n_ops, match):
    ops = np.zeros((max(n_ops, 1), local_dim, local_dim), dtype=complex)
    lib = _lib.load()
    rc = lib.ryd_general_set_collapse(None, local_dim, 3, n_ops, ops.ctypes.data)
    assert rc == -1  # RYD_ERR_INVALID
    assert match in lib.ryd_last_error().decode()


def test_abi_rejects_a_handle_that_is_not_general():
    with pytest.raises(RydError, match="not a general-path handle"):
        _set_collapse(None, 3, 2, [np.eye(3)])
    with pytest.raises(RydError, match="n_ops=1 out of range"):  # ops missing for n_ops > 0
        _lib.check(_lib.load().ryd_general_set_collapse(None, 3, 2, 1, None))


def test_engine_checks_collapse_arguments():
    m = check_collapse_args(3, 2, [DEPOL, np.eye(3)], 9, False)
    assert m.shape == (2, 3, 3) and m.dtype == np.complex128 and m.flags.c_contiguous
    assert check_collapse_args(2, 4, [], 16, False).shape == (0, 2, 2)
    with pytest.raises(ValueError, match="ket engine"):
        check_collapse_args(3, 2, [DEPOL], 81, True)  # a Liouvillian engine
    with pytest.raises(ValueError, match="local dimensions 2 - 4"):
        check_collapse_args(5, 2, [np.eye(5)], 25, False)
    with pytest.raises(ValueError, match="at most 16"):
        check_collapse_args(2, 2, [np.eye(2)] * 17, 4, False)
    with pytest.raises(ValueError, match="is not 3"):
        check_collapse_args(3, 3, [DEPOL], 81, False)


def _embed(local, a, n, d):
    out = np.ones((1, 1))
    for k in range(n):
        out = np.kron(out, local if k == a else np.eye(d))
    return out


@pytest.mark.parametrize("fixture", ["noises_all_0.npz", "noises_digital_6.npz"])
@pytest.mark.parametrize("matrix_free", [False, True])
def test_lowered_collapse_operators_follow_the_reference_order(fixture, matrix_free):
    """hamiltonian.py:97-124: one local operator per collapse spec, placed on every atom; the oracle holds the placed
    ones operator-major (index k * n + a) - string operators, depolarizing Pauli sums and explicit matrices."""
    from oracle import qutip_path as qp

    prob, _ = load_fixture(fixture)
    prob = dict(prob)
    d, n = len(prob["eigenbasis"]), prob["n_qudits"]
    extra_op = DEPOL[:d, :d] if d <= 3 else np.pad(DEPOL, ((0, 1), (0, 1)))
    eb = prob["eigenbasis"]
    prob["collapse_ops"] = list(prob.get("collapse_ops", [])) + [(0.7, extra_op), (0.4, f"sigma_{eb[1]}{eb[0]}")]
    tables, ops = lower_general(prob, mesolve=False, matrix_free=matrix_free, with_collapse=True)
    assert not tables.is_density and tables.dim == d**n
    ham = qp.build_hamiltonian(prob)
    assert len(ops) == len(prob["collapse_ops"]) and len(ham.collapse) == n * len(ops)
    for k, local in enumerate(ops):
        assert local.shape == (d, d)
        for a in range(n):
            np.testing.assert_allclose(_embed(local, a, n, d), ham.collapse[k * n + a].toarray(), atol=1e-15)
    # the tables themselves are the ket tables of the plain call
    plain = lower_general(prob, mesolve=False, matrix_free=matrix_free)
    assert plain.dim == tables.dim and len(plain.series) == len(tables.series)


def _xy_emulator(solver):
    from pulser_amd.hamiltonian_data import SequenceInputs

    prob, _ = load_fixture("noisy_xy_0.npz")
    return QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), sampling_rate=0.1,
                         noise_model=NoiseModel(dephasing_rate=0.5), solver=solver, n_trajectories=4)


@pytest.mark.parametrize("solver", [Solver.MCSOLVER, Solver.DEFAULT, Solver.MESOLVER])
def test_general_jumps_only_changes_the_routing_it_is_asked_to(solver, monkeypatch):
    emu = _xy_emulator(solver)
    calls = []
    monkeypatch.setattr(emu, "_solve_general", lambda probs, mode, options: calls.append(("me", mode)) or ["me"])
    monkeypatch.setattr(emu, "_solve_general_jumps",
                        lambda probs, options, ntraj: calls.append(("jumps", ntraj)) or ["jumps"])
    prob = emu._current_problem
    mode = emu._solver_mode(prob)
    assert not emu._mc_fast_ok(prob)
    for options in ({}, {"general_jumps": False}, {"general_jumps": True}):
        calls.clear()
        out = emu._solve_batch([prob], False, dict(options), mc_ntraj=4)
        if mode == "mcsolve" and options.get("general_jumps"):
            assert calls == [("jumps", 4)] and out == ["jumps"]
        else:  # as without the option: the master-equation fallback
            assert calls == [("me", "mesolve")] and out == ["me"]
    assert mode == ("mcsolve" if solver == Solver.MCSOLVER else "mesolve")


def test_run_docstring_documents_the_option():
    assert "general_jumps=True" in QutipEmulator.run.__doc__
    assert C.sizeof(_lib.RydGeneralConfig) == 24 and _lib.RYD_GENERAL_DENSITY == 1

"""The host reference of the Lanczos exponential tests (tests/lanczos_ref.py) against SciPy and the oracle: no GPU.

tests/test_gpu_lanczos.py judges the device against exp(-i H t) of a constant Hamiltonian; this file shows that the
reference deserves it - the problems are time independent, the two exact propagators agree with ``scipy.linalg.expm``,
with each other and with the oracle's integrator, and a plain float64 Lanczos process with the library's Krylov dimension
keeps the bar of the device tests."""
from __future__ import annotations

import numpy as np
import pytest

import lanczos_ref as L
from helpers import rand_state


def _problems():
    out = [(f"plan{n}", L.plan_problem(n)) for n in (3, 8, 9)]
    out += [(f"batch{i}", p) for i, p in enumerate(L.batch_problems())]
    out += [("diagonal", L.diagonal_problem()), ("symmetric", L.symmetric_problem()), ("dense", L.dense_chain_problem()),
            ("tiny", L.tiny_step_problem()), ("weak", L.weak_drive_problem())]
    return out


def _assert_time_independent(prob, name):
    """matrix(0), matrix(t / 3) and matrix(t_end) of the oracle's Hamiltonian differ by at most 1e-13 max|H|."""
    from oracle import qutip_path as qp

    ham = qp.build_hamiltonian(prob)
    H0 = ham.matrix(0.0)
    for t in (L.T1 / 3, (int(prob["duration"]) - 1) * 1e-3):
        assert abs(ham.matrix(t) - H0).max() <= 1e-13 * abs(H0).max(), (name, t)


@pytest.mark.parametrize("name, prob", _problems(), ids=[n for n, _ in _problems()])
def test_constant_problems_are_time_independent(name, prob):
    _assert_time_independent(prob, name)


def test_constant_problems_13_and_14_atoms_are_time_independent():
    for prob in (L.plan_problem(13), L.plan_problem(13, 1), L.plan_problem(14)):
        _assert_time_independent(prob, int(prob["n_qudits"]))


def test_exact_propagate_against_expm_6_atoms():
    from scipy.linalg import expm

    for prob in L.batch_problems():
        psi = 3.0 * rand_state(64, 1)
        ref = expm(-1j * L.T1 * L.hamiltonian(prob).toarray()) @ psi
        assert np.linalg.norm(L.exact_propagate(prob, L.T1, psi) - ref) <= 1e-13 * np.linalg.norm(psi)


def test_exact_propagate_against_the_oracle_integrator_6_atoms():
    """zvode at rtol 1e-13 (the tight oracle is good to 2e-10 on amplitudes)."""
    from oracle import qutip_path as qp

    prob = L.batch_problems()[0]
    psi = rand_state(64, 2)
    got = qp.sesolve(qp.build_hamiltonian(prob), psi, np.array([0.0, L.T1]), max_step=1e-3, **qp.TIGHT)[-1]
    assert np.linalg.norm(got - L.exact_propagate(prob, L.T1, psi)) <= 2e-10


def test_sparse_propagate_against_exact_propagate_10_atoms():
    prob = L.plan_problem(10)
    psi = 0.5 * rand_state(1024, 3)
    diff = np.linalg.norm(L.sparse_propagate(prob, L.T1, psi) - L.exact_propagate(prob, L.T1, psi))
    assert diff <= 1e-13 * np.linalg.norm(psi)


@pytest.mark.parametrize("tol", [1e-8, 1e-10, 1e-12, 1e-13])
@pytest.mark.parametrize("rho", [1e-4, 0.1, 1.0, 3.0, 6.0])
def test_lanczos_model_with_the_library_dimension_keeps_the_bar(rho, tol):
    """The reference alone keeps the bar: one exponential of argument rho (against the same bound the library forms: half
    the range of the diagonal plus the drives) with m = krylov_dim(rho, tol) ends within 3 tol + FLOOR of the exact one."""
    worst = 0.0
    for prob in (L.plan_problem(8), L.dense_chain_problem()):
        H = L.hamiltonian(prob)
        sigma, radius = L.spectral_bound(H)
        h = rho / radius
        psi = 2.0 * rand_state(H.shape[0], 4)
        got = L.lanczos_model(H, sigma, h, psi, L.krylov_dim(rho, tol))
        err = np.linalg.norm(got - L.exact_propagate(prob, h, psi)) / np.linalg.norm(psi)
        worst = max(worst, err / (3 * tol + L.FLOOR))
    print(f"rho {rho:g} tol {tol:g}: error / (3 tol + floor) = {worst:.2e}")
    assert worst <= 1.0


def test_lanczos_model_ends_at_an_invariant_subspace():
    """4 atoms without interaction under a global drive, from all-ground: the Krylov space is the 5-dimensional symmetric
    subspace, the process breaks down there and the answer is the product of single-atom propagators."""
    prob = L.symmetric_problem()
    H = L.hamiltonian(prob)
    sigma, radius = L.spectral_bound(H)
    psi = np.zeros(16, complex)
    psi[-1] = 1.0
    got = L.lanczos_model(H, sigma, 0.002, psi, 12)
    assert np.linalg.norm(got - L.single_atom_product(prob, 0.002, 4)) <= L.FLOOR
    assert np.linalg.norm(L.exact_propagate(prob, 0.002, psi) - L.single_atom_product(prob, 0.002, 4)) <= 1e-14


def test_krylov_dim_edges():
    assert L.krylov_dim(0.0, 1e-12) == 2 and L.krylov_dim(1e-9, 1e-12) == 2  # never below two basis vectors
    assert L.krylov_dim(2e-6, 1e-12) == 2 and L.krylov_dim(2.1e-6, 1e-12) == 3  # 2 (rho / 2)^2 / 2! = tol at rho = 2e-6
    # the tiny-argument case of the device tests (a step of 0.1 ps) stays at two vectors with a margin of two in rho
    _, radius = L.spectral_bound(L.hamiltonian(L.tiny_step_problem()))
    assert L.krylov_dim(2 * radius * 0.5e-7, 1e-12) == 2
    rhos = [1e-6, 1e-4, 1e-2, 0.1, 0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 10.0, 30.0, 100.0]
    for tol in (1e-6, 1e-8, 1e-10, 1e-12, 1e-14):
        ms = [L.krylov_dim(r, tol) for r in rhos]
        assert all(a <= b for a, b in zip(ms, ms[1:])), (tol, ms)  # monotone in rho
        assert ms[-1] == L.KRY_MAX_M  # capped
    for r in rhos:
        ms = [L.krylov_dim(r, tol) for tol in (1e-4, 1e-6, 1e-8, 1e-10, 1e-12, 1e-14)]
        assert all(a <= b for a, b in zip(ms, ms[1:])), (r, ms)  # monotone in 1 / tol
    for r, tol in ((0.1, 1e-12), (1.0, 1e-10), (5.4, 1e-12), (6.0, 1e-8)):  # the defining inequality, and minimality
        m = L.krylov_dim(r, tol)
        term = lambda k: 2.0 * (r / 2) ** k / np.prod(np.arange(1, k + 1, dtype=float))
        assert term(m) <= tol and (m == 2 or term(m - 1) > tol)
    assert L.krylov_dim(5.4, 1e-12) >= 16 and L.krylov_dim(5.4, 1e-8) < L.krylov_dim(5.4, 1e-12)


def test_bar_formula():
    assert L.FLOOR == 8.0 * L.MEASURED_FLOOR
    assert L.bar(2.0, 16, 1e-12, 1e-13) == pytest.approx(2.0 * 16 * (3e-12 + 1e-13), rel=1e-15)

"""Host reference of the Lanczos exponential tests (tests/test_lanczos_ref.py, tests/test_gpu_lanczos.py): NumPy / SciPy only.

For a Hamiltonian that does not depend on time both exponentials of a CF4 step are exp(-i h H / 2) exactly, so a whole
``method="krylov"`` run is exp(-i H t) and the only errors left are the truncation of the Lanczos process and rounding.
This module builds such problems (:func:`constant_problem`), the exact propagators (:func:`exact_propagate`,
:func:`sparse_propagate`), a restatement of the library's choice of the Krylov dimension (:func:`krylov_dim`), a plain
float64 Lanczos exponential (:func:`lanczos_model`, used only to measure the rounding floor) and the bar of the device
tests (:func:`bar`).

``python tests/lanczos_ref.py`` measures the rounding floor on the problems of the device tests (see :data:`FLOOR`).
"""
from __future__ import annotations

import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root holds ``oracle`` and ``pulser_amd``
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulser_amd import problem as P

KRY_MAX_M = 40  # k_krylov.hpp

# Rounding allowance per exponential (2-norm, relative to the norm of the ket).  MEASURED_FLOOR is the worst error of
# lanczos_model against the exact propagator per exponential with tol = 1e-30 (no truncation left) over the problems of
# the device tests, printed by `python tests/lanczos_ref.py`: 6.8e-14 on the 9-atom chain at 4.5 um from a random ket
# (rho = 5.4, 40 basis vectors), 1.2e-15 .. 1.6e-14 on the others.  The device reduces in another order (block sums and
# atomics), hence the factor 8.
MEASURED_FLOOR = 6.8e-14
FLOOR_FACTOR = 8.0
FLOOR = FLOOR_FACTOR * MEASURED_FLOOR


def constant_problem(n, spacing, seed, global_only=False, zero_interaction=False, amp_scale=1.0, duration=61):
    """An n-atom Ising chain whose samples are constant in time: per-atom amplitude, detuning and non-zero phase through
    ``samples["Local"]`` (the layout of ``helpers.local_problem``), or one global real drive (``global_only``).
    ``zero_interaction`` zeroes ``problem["interaction_matrix"]``; ``amp_scale`` multiplies every amplitude (0: a diagonal
    Hamiltonian)."""
    rng = np.random.default_rng(seed)
    coords = P.register_coords(P.square_rect(1, n), float(spacing))
    zero = np.zeros(duration)
    prob = P.make_ising_problem(coords, {"amp": zero, "det": zero, "phase": zero})
    if global_only:
        a, b = rng.uniform(6, 12), rng.uniform(2, 6)
        prob["samples"] = {"Global": {"ground-rydberg": {"amp": np.full(duration, a * amp_scale), "det": np.full(duration, -b),
                                                         "phase": zero.copy()}}, "Local": {}}
    else:
        loc = {}
        for q in range(n):
            a, b, c = rng.uniform(2, 12, 3)
            loc[q] = {"amp": np.full(duration, a * amp_scale), "det": np.full(duration, b - c - 0.5),
                      "phase": np.full(duration, 0.3 * (q + 1))}
        prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": loc}}
    if zero_interaction:
        prob["interaction_matrix"] = np.zeros_like(prob["interaction_matrix"])
    return prob


def hamiltonian(problem, t=0.0):
    """The oracle's H(t) as CSR."""
    from oracle import qutip_path as qp

    return qp.build_hamiltonian(problem).matrix(float(t)).tocsr()


_EIG = {}  # id(problem) -> (problem, w, V): the decomposition is shared by the calls on one problem


def exact_propagate(problem, t, psi):
    """exp(-i H t) psi by a dense eigendecomposition of the oracle's H (evaluated at t / 2; it is constant).  n <= 10."""
    if id(problem) not in _EIG:
        _EIG[id(problem)] = (problem,) + tuple(np.linalg.eigh(hamiltonian(problem, 0.5 * t).toarray()))
    _, w, V = _EIG[id(problem)]
    return V @ (np.exp(-1j * w * t) * (V.conj().T @ np.asarray(psi, dtype=complex)))


def sparse_propagate(problem, t, psi):
    """exp(-i H t) psi by scipy's expm_multiply on the sparse H (13 and 14 atoms)."""
    from scipy.sparse.linalg import expm_multiply

    return expm_multiply(-1j * t * hamiltonian(problem, 0.5 * t).tocsc(), np.asarray(psi, dtype=complex))


def krylov_dim(rho, tol):
    """host_krylov.hpp: the smallest m >= 2 with 2 (rho / 2)^m / m! <= tol, capped at KRY_MAX_M."""
    term, m = 2.0, 0
    while m < KRY_MAX_M:
        m += 1
        term *= 0.5 * rho / m
        if m >= 2 and term <= tol:
            break
    return min(m, KRY_MAX_M)


def spectral_bound(H):
    """(sigma, radius): centre of the diagonal of H and a Gershgorin bound of ||H - sigma|| (the library's bound has the
    same two parts: half the range of the diagonal plus the sum of the drives)."""
    import scipy.sparse as sp

    H = sp.csr_matrix(H)
    d = H.diagonal().real
    off = abs(H - sp.diags(H.diagonal()))
    sigma = 0.5 * (d.min() + d.max())
    return float(sigma), float(0.5 * (d.max() - d.min()) + off.sum(axis=1).max())


def lanczos_model(H, sigma, h, psi, m):
    """exp(-i h H) psi by an m-dimensional Lanczos process on H - sigma in float64, no reorthogonalisation: the recurrence
    of k_krylov.hpp in plain NumPy (beta at or below 1e-14 ends the process: the subspace is invariant)."""
    from scipy.linalg import eigh_tridiagonal

    psi = np.asarray(psi, dtype=complex)
    n0 = np.linalg.norm(psi)
    if n0 == 0.0:
        return np.zeros_like(psi)
    V = [psi / n0]
    alpha, beta = [], []
    for j in range(m):
        w = H @ V[j] - sigma * V[j]
        a = np.vdot(V[j], w).real
        u = w - a * V[j] - (beta[j - 1] * V[j - 1] if j > 0 else 0.0)
        b = np.linalg.norm(u)
        alpha.append(a)
        if j == m - 1:
            break
        if b <= 1e-14:
            break
        beta.append(b)
        V.append(u / b)
    k = len(alpha)
    if k == 1:
        c = np.array([np.exp(-1j * h * alpha[0])])
    else:
        w, Q = eigh_tridiagonal(np.array(alpha), np.array(beta[: k - 1]))
        c = Q @ (np.exp(-1j * h * w) * Q[0])
    out = np.zeros_like(psi)
    for j in range(k):
        out += c[j] * V[j]
    return n0 * np.exp(-1j * h * sigma) * out


def bar(norm0, n_exp, tol, floor=FLOOR):
    """Bound of the 2-norm error of one ket after ``n_exp`` Lanczos exponentials at tolerance ``tol``:
    ``norm0 * n_exp * (3 * tol + floor)``.

    Each exponential is unitary up to its own error, so the errors of the exponentials add.  Truncation per exponential
    (relative to the norm of the ket):
      1. the Lanczos approximation of exp(-i h H) v is within twice the best approximation of e^{-ix} by a polynomial of
         degree m - 1 on the spectral interval (half-width rho, after the shift);
      2. that is at most the Chebyshev tail  2 sum_{k >= m} |J_k(rho)| <= 2 (rho / 2)^m / m! * 1 / (1 - rho / (2 (m + 1)));
      3. krylov_dim picks m so that the first factor is <= tol, and for rho <= 6 (the scheduler's r_max; the device tests
         assert that their arguments stay below it) and the m it picks the second factor is <= 1.15 at tol <= 1e-10
         (m >= 22 at rho = 6) and 1.167 at tol = 1e-8 (m = 20); it falls with rho.
    The chain: 2 x 1.15 <= 3 (2 x 1.167 <= 3 at the loosest tol the tests use).
    ``floor`` is the rounding allowance per exponential (FLOOR: measured, see the module)."""
    return float(norm0) * int(n_exp) * (3.0 * float(tol) + float(floor))


# ---------------------------------------------------------------------------------------------------------------------
# The problems of the device tests (tests/test_gpu_lanczos.py builds its cases from these, and so does the measurement
# of the floor below)
# ---------------------------------------------------------------------------------------------------------------------
T1 = 0.03  # us: the run of most cases


def plan_problem(n, seed=0):
    """A: interacting chain at 7 um, per-atom complex constant drives."""
    return constant_problem(n, 7.0, 100 + n + seed)


def batch_problems():
    """B: three distinct 6-atom problems cycled over the batch."""
    return [constant_problem(6, s, 200 + i) for i, s in enumerate((7.0, 6.0, 8.5))]


def diagonal_problem(n=6):
    """C: amplitude 0, constant non-zero detunings, interacting: every basis state is an eigenvector."""
    return constant_problem(n, 6.0, 300, amp_scale=0.0)


def symmetric_problem():
    """C: 4 atoms without interaction under one global real drive: from all-ground the Krylov space is the 5-dimensional
    symmetric subspace."""
    return constant_problem(4, 7.0, 301, global_only=True, zero_interaction=True, amp_scale=3.0)


def dense_chain_problem():
    """D: 9 atoms at 4.5 um (about 650 rad/us between neighbours): a four-knot step has an argument of about 5."""
    return constant_problem(9, 4.5, 302)


def weak_drive_problem():
    """C: the 9-atom chain at 4.5 um with drives of 0.01 - 0.05 rad/us.  From all-ground |u|^2 / |w|^2 of the first iteration
    is (sum |Omega_k / 2|^2) / (E - sigma)^2 = 2e-10: below the 1e-8 at which k_kry_update_fused gives up the cancelling
    formula for its provisional scale, so the next stored basis vector has a norm of 1e-5 instead of about 1."""
    return constant_problem(9, 4.5, 304, amp_scale=0.004)


def edge_superposition(n, phase=0.9):
    """e^{i phase} (|g...g> + e^{0.7 i} |r...r>): weight on both ends of the spectrum of a diagonal-dominated H (the
    polynomial must hold over the whole interval) and a global phase that is not real."""
    psi = np.zeros(2**n, complex)
    psi[-1] = np.exp(1j * phase)
    psi[0] = np.exp(1j * (phase + 0.7))
    return psi


def tiny_step_problem():
    """D: 3 atoms at 10 um: ||H|| is small enough (about 20 rad/us against the library's bound) for an exponential over
    0.05 ps to need the minimum of two basis vectors at tol = 1e-12 (2 (rho / 2)^2 / 2! <= 1e-12 from rho = 2e-6 down)."""
    return constant_problem(3, 10.0, 303, amp_scale=0.5)


def single_atom_product(problem, t, n):
    """exp(-i H t) |g...g> of ``symmetric_problem`` as a product of exact single-atom 2 x 2 propagators."""
    g = problem["samples"]["Global"]["ground-rydberg"]
    om, de = float(g["amp"][0]), float(g["det"][0])
    h1 = np.array([[-de, om / 2], [om / 2, 0.0]])  # (r, g): -delta n_r + (Omega / 2) sigma_x
    w, v = np.linalg.eigh(h1)
    a1 = (v @ np.diag(np.exp(-1j * w * t)) @ v.conj().T) @ np.array([0.0, 1.0])
    out = np.array([1.0 + 0j])
    for _ in range(n):
        out = np.kron(out, a1)
    return out


def measure_floor(verbose=True):
    """Worst error per exponential of lanczos_model (tol = 1e-30: no truncation left) against the exact propagator on
    the constant problems of the device tests, from a seeded random ket, over four exponentials of a four-knot step
    (h / 2 = 2 ns) each."""
    cases = [(f"A n={n}", plan_problem(n)) for n in (3, 8, 9, 14)]
    cases += [(f"A n=13 entry {s}", plan_problem(13, s)) for s in (0, 1)]
    cases += [(f"B problem {i}", p) for i, p in enumerate(batch_problems())]
    cases += [("C diagonal", diagonal_problem()), ("C symmetric", symmetric_problem()), ("C weak drive", weak_drive_problem()),
              ("D 4.5 um", dense_chain_problem()), ("D 4.5 um, edges", dense_chain_problem()), ("D tiny step", tiny_step_problem())]
    worst = 0.0
    for name, prob in cases:
        n = int(prob["n_qudits"])
        H = hamiltonian(prob)
        sigma, radius = spectral_bound(H)
        h = 0.002
        m = krylov_dim(h * radius, 1e-30)
        rng = np.random.default_rng(7)
        psi = rng.normal(size=2**n) + 1j * rng.normal(size=2**n)
        if name in ("C symmetric", "C weak drive"):
            psi = np.zeros(2**n, complex)
            psi[-1] = 1.0
        if name == "D 4.5 um, edges":
            psi = edge_superposition(n)
        err = 0.0
        for _ in range(4):
            got = lanczos_model(H, sigma, h, psi, m)
            ref = (exact_propagate if n <= 10 else sparse_propagate)(prob, h, psi)
            err = max(err, float(np.linalg.norm(got - ref) / np.linalg.norm(psi)))
            psi = ref
        worst = max(worst, err)
        if verbose:
            print(f"{name:18s} rho = {h * radius:8.3g}  m = {m:2d}  error per exponential {err:.2e}")
    if verbose:
        print(f"measured floor {worst:.2e}; FLOOR = {FLOOR_FACTOR:g} x {MEASURED_FLOOR:.1e} = {FLOOR:.1e}")
    return worst


if __name__ == "__main__":
    measure_floor()

"""CPU: the longdouble reference of tests/overlap_ref.py against the plain ``np.vdot`` / ``np.trace`` formulas on small
random inputs, and its bounds against their definitions."""
import numpy as np
import pytest

from overlap_ref import (U53, part_errors, ref_norm, ref_overlap, tol_fidelity_ket, tol_norm, tol_ratio, tol_trace,
                         tol_z)


def _rand(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


@pytest.mark.parametrize("D", [1, 2, 5, 27])
def test_kets_against_vdot(D):
    rng = np.random.default_rng(D)
    x, a = _rand(rng, 6, D), _rand(rng, 3, D)
    z, s_abs = ref_overlap(x, a)
    n, n_abs = ref_norm(x)
    assert z.shape == s_abs.shape == (6, 3) and n.shape == (6,)
    for s in range(6):
        assert abs(float(n[s]) - np.vdot(x[s], x[s]).real) <= 1e-13 * float(n[s]) and n_abs[s] == n[s]
        for f in range(3):
            assert part_errors(z[s, f], np.vdot(a[f], x[s])) <= 1e-13 * float(s_abs[s, f])
            assert abs(float(s_abs[s, f]) - np.sum(np.abs(a[f]) * np.abs(x[s]))) <= 1e-13 * float(s_abs[s, f])


@pytest.mark.parametrize("D", [1, 2, 4, 9])
def test_density_matrices_against_trace_formulas(D):
    rng = np.random.default_rng(10 + D)
    rho, A, phi = _rand(rng, 5, D, D), _rand(rng, 2, D, D), _rand(rng, 3, D)  # no symmetry: read as stored
    z0, s0 = ref_overlap(rho, A, density=True)
    z0_flat, _ = ref_overlap(rho, A.reshape(2, D * D), density=True)
    z1, s1 = ref_overlap(rho, phi, density=True, outer=True)
    tr, tr_abs = ref_norm(rho, density=True)
    assert np.array_equal(z0, z0_flat)
    for s in range(5):
        assert abs(float(tr[s]) - np.trace(rho[s]).real) <= 1e-13 * float(tr_abs[s])
        assert abs(float(tr_abs[s]) - np.sum(np.abs(np.diag(rho[s]).real))) <= 1e-13 * float(tr_abs[s])
        for f in range(2):
            assert part_errors(z0[s, f], np.trace(A[f].conj().T @ rho[s])) <= 1e-13 * float(s0[s, f])
        for f in range(3):
            assert part_errors(z1[s, f], np.vdot(phi[f], rho[s] @ phi[f])) <= 1e-13 * float(s1[s, f])
            big = np.outer(phi[f], phi[f].conj())  # A = |phi><phi| materialised: the same number as target form 0
            assert part_errors(z1[s, f], ref_overlap(rho[s:s + 1], big[None], density=True)[0][0, 0]) <= 1e-13 * float(s1[s, f])
            assert abs(float(s1[s, f]) - np.sum(np.abs(big) * np.abs(rho[s]))) <= 1e-13 * float(s1[s, f])


def test_bounds_are_the_documented_expressions():
    assert tol_z(100, 2.0) == 116 * U53 * 2.0
    assert tol_norm(8, 3.0) == 10 * U53 * 3.0
    assert tol_trace(8, 3.0) == 10 * U53 * 3.0
    z, n, dz, dn = 0.3 - 0.4j, 2.0, 1e-9, 3e-9
    assert np.isclose(tol_fidelity_ket(z, n, dz, dn), 2 * 0.5 * np.sqrt(2) * dz / n + 0.25 * dn / n**2, rtol=1e-14)
    assert np.isclose(tol_ratio(-0.3, n, dz, dn), dz / n + 0.3 * dn / n**2, rtol=1e-14)
    # a perturbation of the size of the bounds stays inside the propagated bound (first order, 1 % slack for the second)
    for sz, sn in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        zp, np_ = z + sz * np.sqrt(2) * dz * z / abs(z), n + sn * dn  # radial: the worst direction for |z|
        assert abs(abs(zp)**2 / np_ - abs(z)**2 / n) <= 1.01 * tol_fidelity_ket(z, n, dz, dn)

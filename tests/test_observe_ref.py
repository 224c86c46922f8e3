"""CPU: the longdouble host reference of the device observables (tests/observe_ref.py) checked on its own, on the
kind of input tests/test_gpu_observe.py feeds it: per-atom drives with a non-zero phase, unnormalised random states."""
import numpy as np
import pytest

from helpers import local_problem, rand_state
from observe_ref import LD, U53, ket_probabilities, ref_energy_dm, ref_energy_ket, ref_pairs

T_INTERIOR = 0.12345


def _ham(n, seed):
    from oracle import qutip_path as qp

    prob = local_problem(n, seed=seed)
    return prob, qp.build_hamiltonian(prob)


@pytest.mark.parametrize("n", [1, 2, 4, 7])
@pytest.mark.parametrize("t", [0.0, T_INTERIOR, 0.2, 0.4])
def test_ket_and_density_matrix_formulas_agree_on_a_pure_state(n, t):
    _, ham = _ham(n, seed=n)
    x = 1.7 * rand_state(2**n, 40 + n)
    e1, e2, _, _ = ref_energy_ket(ham, t, x)
    d1, d2, (s1, s2) = ref_energy_dm(ham, t, np.outer(x, x.conj()))
    # the ket path applies H in float64: every (H x)_i carries at most ~(n + 2) u sum_j |H_ij||x_j|
    assert abs(e1 - d1) <= 8 * (n + 2) * U53 * s1
    assert abs(e2 - d2) <= 8 * (n + 2) * U53 * s2


@pytest.mark.parametrize("n", [1, 3, 5])
def test_basis_states_give_the_closed_forms(n):
    """<a|H|a> = E(a) and <a|H^2|a> = E(a)^2 + sum_k |c_k|^2 (the comment above k_obs_energy_dm), with
    E(a) = sum_{i<j} U_ij n_i n_j - sum_k delta_k(t) n_k and c_k = Omega_k(t) exp(-i phi_k(t)) / 2."""
    prob, ham = _ham(n, seed=11 + n)
    dyn = [term for term in ham.terms if term.knots is not None]
    U = np.asarray(prob["interaction_matrix"], dtype=float)[-1]
    D = 2**n
    for t in (0.0, T_INTERIOR, 0.4):
        coef = dict(zip((term.label for term in dyn), ham.coefficients(t)))
        drive = np.array([coef[f"L:ground-rydberg:{k}:sigma_gr"] for k in range(n)])
        det = np.array([-2.0 * coef[f"L:ground-rydberg:{k}:sigma_rr"].real for k in range(n)])
        assert np.all(np.abs(drive.imag) > 1e-3) or t == 0.0  # the phase is exercised
        c2 = float(np.sum(np.abs(drive) ** 2))
        for a in range(D):
            nk = np.array([1 - ((a >> (n - 1 - k)) & 1) for k in range(n)], dtype=float)
            E = sum(U[i, j] * nk[i] * nk[j] for i in range(n) for j in range(i + 1, n)) - float(det @ nk)
            x = np.zeros(D, complex)
            x[a] = 1.0
            scale = max(1.0, abs(E)) ** 2 + c2
            e1, e2, _, _ = ref_energy_ket(ham, t, x)
            assert abs(e1 - E) <= 1e-13 * scale and abs(e2 - (E * E + c2)) <= 1e-13 * scale
            d1, d2, _ = ref_energy_dm(ham, t, np.outer(x, x))
            assert abs(d1 - E) <= 1e-13 * scale and abs(d2 - (E * E + c2)) <= 1e-13 * scale


@pytest.mark.parametrize("n", [1, 2, 3, 6, 10])
def test_ref_pairs_equals_the_dense_product(n):
    D = 2**n
    x = 0.6 * rand_state(D, 7 + n)
    p = ket_probabilities(x)
    norm, occ, corr, (s_norm, s_occ, s_corr) = ref_pairs(p, n)
    idx = np.arange(D)
    nk = np.stack([1 - ((idx >> (n - 1 - k)) & 1) for k in range(n)], axis=1).astype(float)
    p64 = p.astype(float)
    assert abs(norm - p64.sum()) <= D * U53 * s_norm
    assert np.all(np.abs(occ - p64 @ nk) <= D * U53 * s_occ)
    assert np.all(np.abs(corr - (nk * p64[:, None]).T @ nk) <= D * U53 * s_corr)
    assert np.array_equal(corr, corr.T) and np.array_equal(np.diag(corr), occ)
    assert norm.dtype == LD and abs(float(norm) - 0.36) < 1e-15
    # p >= 0: the sums of absolute values are the sums themselves
    assert s_norm == norm and np.array_equal(s_corr, corr)


def test_ref_pairs_on_basis_states_is_exact():
    n = 5
    for a in range(2**n):
        p = np.zeros(2**n)
        p[a] = 1.0
        norm, occ, corr, _ = ref_pairs(p, n)
        bits = np.array([1 - ((a >> (n - 1 - k)) & 1) for k in range(n)], dtype=float)
        assert norm == 1.0 and np.array_equal(occ, bits) and np.array_equal(corr, np.outer(bits, bits))

"""CPU: the longdouble host reference of ``engine.expect_sparse`` (tests/expect_ref.py) pinned to the dense formulas
x^dag O x and trace(O rho) on 2 - 4 atoms, on the kind of input tests/test_gpu_expect.py feeds it: random complex
non-Hermitian operators (sparse and dense), unnormalised random states, random non-Hermitian "density" matrices."""
import numpy as np
import pytest
import scipy.sparse as sp

from expect_ref import CLD, LD, U53, part_errors, ref_expect, ref_expect_dm, ref_expect_ket, tol_expect, triplets
from helpers import rand_state


def _operator(D, density, seed):
    rng = np.random.default_rng(seed)
    m = sp.random(D, D, density=density, random_state=rng, format="csr", dtype=np.float64)
    m.data = rng.normal(size=m.nnz) + 1j * rng.normal(size=m.nnz)
    return m


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("fill", [0.2, 1.0])
def test_reference_equals_the_dense_formulas(n, fill):
    D = 2**n
    O = _operator(D, fill, seed=10 * n + int(fill * 10))
    dense = O.toarray()
    r, c, v = triplets(O)
    assert len(v) == O.nnz and np.all(np.diff(r * D + c) > 0)  # sorted by (row, col), no duplicates
    for s in range(3):
        x = 1.7 * rand_state(D, 40 + n + s)
        val, s_abs = ref_expect_ket(O, x)
        assert val.dtype == CLD and s_abs.dtype == LD
        # the float64 dense product carries at most ~(D + 2) u sum |O_ij||x_i||x_j| per part; S_abs is that sum
        assert part_errors(np.vdot(x, dense @ x), val) <= 4 * (D + 2) * U53 * float(s_abs)
        assert abs(float(s_abs) - float(np.abs(x) @ (np.abs(dense) @ np.abs(x)))) <= 1e-13 * float(s_abs)
        rho = rand_state(D * D, 70 + n + s).reshape(D, D) * 2.5  # not Hermitian, trace not 1
        val, s_abs = ref_expect_dm(O, rho)
        assert part_errors(np.trace(dense @ rho), val) <= 4 * (D + 2) * U53 * float(s_abs)
        assert abs(float(s_abs) - float(np.sum(np.abs(dense) * np.abs(rho).T))) <= 1e-13 * float(s_abs)
        # a pure state: both formulas give one number
        pure, s_pure = ref_expect_dm(O, np.outer(x, x.conj()))
        assert part_errors(pure, ref_expect_ket(O, x)[0]) <= 8 * U53 * float(s_pure)


def test_reference_on_basis_states_duplicates_and_the_empty_operator():
    D = 8
    O = _operator(D, 0.5, seed=3)
    dense = O.toarray()
    for a in range(D):
        x = np.zeros(D, complex)
        x[a] = 1.0
        val, s_abs = ref_expect_ket(O, x)
        assert complex(val) == dense[a, a] and float(s_abs) == abs(dense[a, a])
    # duplicates in coordinate form are summed before anything else; explicit entries that cancel stay harmless
    coo = sp.coo_matrix((np.array([1.0, 2.0, 1j, -1j]), (np.array([1, 1, 2, 2]), np.array([3, 3, 0, 0]))), shape=(D, D))
    x = rand_state(D, 5)
    val, _ = ref_expect_ket(coo, x)
    assert abs(complex(val) - 3.0 * np.conj(x[1]) * x[3]) < 1e-15
    vals, s_abs = ref_expect(sp.csr_matrix((D, D), dtype=complex), np.stack([x, 2 * x]))
    assert np.all(vals == 0) and np.all(s_abs == 0) and np.all(tol_expect(0, s_abs) == 0)


def test_tolerance_is_the_documented_bound():
    assert tol_expect(5, 2.0) == 21 * 2.0 ** -53 * 2.0
    assert np.array_equal(tol_expect(0, np.array([1.0, 0.0], dtype=LD)), np.array([16 * 2.0 ** -53, 0.0]))
    assert part_errors(1 + 2j, 1.5 + 2.25j) == 0.5

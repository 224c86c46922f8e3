"""CPU: the longdouble reference of ``ryd_ensemble_diag`` (tests/ensemble_ref.py) against a float64 NumPy sum, within its
own bound - the reference and the bound are what tests/test_gpu_mc_ensemble.py holds the kernel to."""
import numpy as np
import pytest

from ensemble_ref import ref_diag, tol_diag
from observe_ref import LD, U53


def _states(rng, T, B, D, scale=1.0):
    return (rng.normal(size=(T, B, D)) + 1j * rng.normal(size=(T, B, D))) * scale


@pytest.mark.parametrize("T,B,D", [(1, 1, 1), (3, 2, 3), (2, 65, 243), (1, 300, 16)])
def test_reference_matches_a_float64_sum_within_its_bound(T, B, D):
    rng = np.random.default_rng(1000 * T + 10 * B + D)
    x = _states(rng, T, B, D)
    start = rng.normal(size=(T, D))
    ref, s_abs = ref_diag(x, start)
    assert ref.dtype == LD and ref.shape == s_abs.shape == (T, D)
    assert np.all(s_abs >= np.abs(ref))
    got = start.copy()
    for b in range(B):  # the order of the kernel: onto the value found, b ascending
        got += x[:, b].real ** 2 + x[:, b].imag ** 2
    tol = tol_diag(B, s_abs)
    assert np.all(np.abs(got.astype(LD) - ref) <= tol)
    # another order of the same summands stays inside the bound too (it does not depend on the order)
    other = (x.real ** 2 + x.imag ** 2)[:, ::-1].sum(axis=1) + start
    assert np.all(np.abs(other.astype(LD) - ref) <= tol)


def test_bound_is_the_projects_sum_rule():
    s = np.array([[1.0, 2.0], [0.0, 4.0]])
    assert np.array_equal(tol_diag(5, s), 13 * U53 * s)
    assert tol_diag(1, LD(3)).dtype == np.float64


def test_reference_resolves_what_float64_loses():
    # 1 + 2^-60 per trajectory: float64 keeps 1.0 for every partial sum, the longdouble reference does not
    x = np.full((1, 4, 1), np.sqrt(2.0 ** -60), dtype=complex)
    ref, s_abs = ref_diag(x, np.ones((1, 1)))
    assert ref[0, 0] > 1 and float(ref[0, 0]) == 1.0
    assert abs(ref[0, 0] - 1 - 4 * LD(2.0) ** -60) < LD(2.0) ** -100
    assert abs(1.0 - ref[0, 0]) <= tol_diag(4, s_abs)[0, 0]

"""CPU: the longdouble reference of ``ryd_reduced_density_dm`` (tests/ptrace_dm_ref.py) against the package's host
formula (``_ptrace_host``) and against an independent one - the partial trace written out with explicit loops over the
digits - on NON-Hermitian random matrices, for local dimensions 2, 3 and 4."""
import itertools

import numpy as np
import pytest

from observe_ref import LD, U53
from ptrace_dm_ref import kept_first_dm, ref_reduced_dm, tol_reduced_dm
from ptrace_ref import ref_reduced

from pulser_amd.results import _ptrace_host


def _rand(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _reduced(rho, keep, d):
    """One matrix, no start value: the complex128 rounding of the reference."""
    d_a = d ** len(keep)
    (re, im), _, _ = ref_reduced_dm(np.asarray(rho)[None, None], np.zeros((1, d_a, d_a), dtype=complex), keep, d)
    return (re.astype(np.float64) + 1j * im.astype(np.float64))[0]


def _subsets(n):
    return [list(c) for k in range(1, n + 1) for c in itertools.combinations(range(n), k)]


def _loops(rho, keep, d, n):
    """out[a][a'] = sum_r rho[idx(a, r)][idx(a', r)] with every index built digit by digit."""
    rest = [k for k in range(n) if k not in keep]
    d_a = d ** len(keep)
    out = np.zeros((d_a, d_a), dtype=complex)

    def idx(a_digits, r_digits):
        i = 0
        for k in range(n):
            dg = a_digits[keep.index(k)] if k in keep else r_digits[rest.index(k)]
            i = i * d + dg
        return i

    for a, ad in enumerate(itertools.product(range(d), repeat=len(keep))):
        for c, cd in enumerate(itertools.product(range(d), repeat=len(keep))):
            for rd in itertools.product(range(d), repeat=len(rest)):
                out[a, c] += rho[idx(ad, rd), idx(cd, rd)]
    return out


@pytest.mark.parametrize("d,n", [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (4, 1), (4, 2)])
def test_reference_equals_explicit_loops_for_every_subset(d, n):
    rng = np.random.default_rng(10 * d + n)
    rho = _rand(rng, d**n, d**n)  # no symmetry of any kind
    scale = np.abs(rho).sum()
    for keep in _subsets(n):
        got = _reduced(rho, keep, d)
        want = _loops(rho, keep, d, n)
        assert got.shape == want.shape
        assert np.allclose(got, want, rtol=0, atol=1e-14 * scale), keep


@pytest.mark.parametrize("d,n", [(2, 5), (3, 3), (4, 3)])
def test_reference_equals_the_host_formula_on_non_hermitian_matrices(d, n):
    rng = np.random.default_rng(d + n)
    rho = _rand(rng, d**n, d**n) * np.exp(rng.normal(size=(d**n, d**n)))  # mixed signs and magnitudes
    scale = np.abs(rho).sum()
    for keep in _subsets(n):
        got = _reduced(rho, keep, d)
        host = _ptrace_host(rho, False, keep, d)
        assert np.allclose(got, host, rtol=0, atol=1e-14 * scale), keep
        # the reference reads rho[i][j], not rho[j][i]: the transposed input gives the transposed answer, another matrix
        assert not np.allclose(got, got.T, rtol=0, atol=1e-6 * np.abs(got).max())
        assert np.allclose(_reduced(rho.T, keep, d), got.T, rtol=0, atol=1e-14 * scale)
        assert abs(np.trace(got) - np.trace(rho)) <= 1e-14 * scale


def test_scales_bound_the_entries_and_the_start_value_is_added():
    rng = np.random.default_rng(3)
    x = _rand(rng, 2, 3, 27, 27)
    start = _rand(rng, 2, 9, 9)
    (re, im), s_re, s_im = ref_reduced_dm(x, start, [0, 2], 3)
    (re0, im0), s_re0, s_im0 = ref_reduced_dm(x, np.zeros_like(start), [0, 2], 3)
    assert re.dtype == LD and s_re.dtype == LD and re.shape == (2, 9, 9)
    assert np.all(np.abs(re) <= s_re) and np.all(np.abs(im) <= s_im)
    assert np.allclose((re - re0).astype(float), start.real) and np.allclose((im - im0).astype(float), start.imag)
    assert np.allclose((s_re - s_re0).astype(float), np.abs(start.real))
    assert np.allclose((s_im - s_im0).astype(float), np.abs(start.imag))
    # the trajectory axis is a plain sum
    parts = [ref_reduced_dm(x[:, b:b + 1], np.zeros_like(start), [0, 2], 3)[0] for b in range(3)]
    assert np.allclose(sum(p[0] for p in parts).astype(float), re0.astype(float))
    assert np.allclose(sum(p[1] for p in parts).astype(float), im0.astype(float))
    # a float64 NumPy evaluation lies within the bound of the reference
    f64 = kept_first_dm(x, [0, 2], 3).sum(axis=(1, 4))
    assert np.all(np.abs(f64.real - re0) <= tol_reduced_dm(3 * 3, s_re0))
    assert np.all(np.abs(f64.imag - im0) <= tol_reduced_dm(3 * 3, s_im0))
    assert tol_reduced_dm(5, 2.0) == 13 * U53 * 2.0


def test_projector_of_a_ket_gives_the_ket_reference():
    rng = np.random.default_rng(4)
    psi = _rand(rng, 3**3)
    rho = np.outer(psi, psi.conj())
    for keep in _subsets(3):
        d_a = 3 ** len(keep)
        (re, im), _, _ = ref_reduced(psi.reshape(1, 1, -1), np.zeros((1, d_a, d_a), dtype=complex), keep, 3)
        want = (re.astype(np.float64) + 1j * im.astype(np.float64))[0]
        assert np.allclose(_reduced(rho, keep, 3), want, rtol=0, atol=1e-13 * np.vdot(psi, psi).real), keep


@pytest.mark.parametrize("d,n", [(2, 4), (3, 3), (4, 2)])
def test_keeping_every_site_returns_the_matrix(d, n):
    rng = np.random.default_rng(7)
    rho = _rand(rng, d**n, d**n)
    assert np.array_equal(_reduced(rho, range(n), d), rho)

"""CPU: the longdouble reference of ``ryd_reduced_density`` (tests/ptrace_ref.py) against independent formulas - the
partial trace written out with Kronecker products, traces, marginals, ranks and the entropies of states whose answer is
known."""
import itertools

import numpy as np
import pytest

from observe_ref import LD
from general_observe_ref import digits_of
from ptrace_ref import kept_first, ref_reduced, tol_reduced

from pulser_amd import entropy_vn


def _rand(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _rho(ref):
    re, im = ref
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def _reduced(psi, keep, d):
    """One ket, no start value: the complex128 rounding of the reference."""
    d_a = d ** len(keep)
    ref, _, _ = ref_reduced(np.asarray(psi).reshape(1, 1, -1), np.zeros((1, d_a, d_a), dtype=complex), keep, d)
    return _rho(ref)[0]


def _subsets(n):
    return [list(c) for k in range(1, n + 1) for c in itertools.combinations(range(n), k)]


def _kron_partial_trace(psi, keep, d, n):
    """sum_r (1 (x) <r|) |psi><psi| (1 (x) |r>) with the bra on the sites outside ``keep``, as explicit matrices."""
    rest = [k for k in range(n) if k not in keep]
    rho = np.outer(psi, psi.conj())
    eye = np.eye(d)
    out = np.zeros((d ** len(keep),) * 2, dtype=complex)
    for r in itertools.product(range(d), repeat=len(rest)):
        op = np.ones((1, 1))
        for k in range(n):
            op = np.kron(op, eye if k in keep else eye[[r[rest.index(k)]]])  # identity, or the row vector <r_k|
        out += op @ rho @ op.conj().T
    return out


@pytest.mark.parametrize("d,n", [(2, 1), (2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4)])
def test_reference_equals_the_explicit_partial_trace_for_every_subset(d, n):
    rng = np.random.default_rng(10 * d + n)
    psi = _rand(rng, d**n)
    for keep in _subsets(n):
        got = _reduced(psi, keep, d)
        want = _kron_partial_trace(psi, keep, d, n)
        assert got.shape == want.shape
        assert np.allclose(got, want, rtol=0, atol=1e-13 * np.vdot(psi, psi).real), keep


@pytest.mark.parametrize("d,n", [(2, 5), (3, 3), (4, 3)])
def test_trace_hermiticity_and_marginals(d, n):
    rng = np.random.default_rng(d + n)
    psi = _rand(rng, d**n)
    p = np.abs(psi) ** 2
    dig = digits_of(n, d)
    for keep in _subsets(n):
        rho = _reduced(psi, keep, d)
        assert abs(np.trace(rho) - p.sum()) <= 1e-13 * p.sum()
        assert np.allclose(rho, rho.conj().T, rtol=0, atol=1e-14 * p.sum())
        row = np.zeros(d**n, dtype=np.int64)  # the row index of every basis state: kept digits, ascending site order
        for k in keep:
            row = row * d + dig[:, k]
        marginal = np.bincount(row, weights=p, minlength=d ** len(keep))
        assert np.allclose(np.diag(rho).real, marginal, rtol=0, atol=1e-13 * p.sum())
        assert np.all(np.abs(np.diag(rho).imag) == 0)


def test_scales_bound_the_entries_and_the_start_value_is_added():
    rng = np.random.default_rng(3)
    x = _rand(rng, 2, 3, 3**3)
    start = _rand(rng, 2, 9, 9)
    (re, im), s_re, s_im = ref_reduced(x, start, [0, 2], 3)
    (re0, im0), s_re0, s_im0 = ref_reduced(x, np.zeros_like(start), [0, 2], 3)
    assert re.dtype == LD and s_re.dtype == LD
    assert np.all(np.abs(re) <= s_re) and np.all(np.abs(im) <= s_im)
    assert np.allclose((re - re0).astype(float), start.real) and np.allclose((im - im0).astype(float), start.imag)
    assert np.allclose((s_re - s_re0).astype(float), np.abs(start.real))
    assert np.allclose((s_im - s_im0).astype(float), np.abs(start.imag))
    # the trajectory axis is a plain sum
    parts = [ref_reduced(x[:, b:b + 1], np.zeros_like(start), [0, 2], 3)[0] for b in range(3)]
    assert np.allclose(sum(p[0] for p in parts).astype(float), re0.astype(float))
    assert np.allclose(sum(p[1] for p in parts).astype(float), im0.astype(float))
    # a float64 NumPy evaluation lies within the bound of the reference
    m = kept_first(x, [0, 2], 3)
    f64 = np.einsum("tbar,tbcr->tac", m, m.conj())
    assert np.all(np.abs(f64.real - re0) <= tol_reduced(3 * 3, s_re0))
    assert np.all(np.abs(f64.imag - im0) <= tol_reduced(3 * 3, s_im0))
    assert tol_reduced(5, 2.0) == 18 * 2.0**-53 * 2.0


def test_product_ket_gives_rank_one():
    rng = np.random.default_rng(4)
    single = _rand(rng, 4, 3)
    psi = np.array([1.0 + 0j])
    for k in range(4):
        psi = np.kron(psi, single[k])
    for keep in _subsets(4):
        rho = _reduced(psi, keep, 3)
        sv = np.linalg.svd(rho, compute_uv=False)
        assert sv[0] > 0 and np.all(sv[1:] <= 1e-13 * sv[0]), keep
        assert abs(entropy_vn(rho)) < 1e-10


def test_ghz_bell_and_maximally_mixed_entropies():
    ghz = np.zeros(16, dtype=complex)
    ghz[0] = ghz[15] = np.sqrt(0.5)
    for keep in _subsets(4):
        s = entropy_vn(_reduced(ghz, keep, 2))
        assert abs(s - (1.0 if len(keep) < 4 else 0.0)) < 1e-12, keep
    bell = np.array([0, 1, -1, 0], dtype=complex) / np.sqrt(2)
    for keep in ([0], [1]):
        assert abs(entropy_vn(_reduced(bell, keep, 2)) - 1.0) < 1e-12
    # k qubits each half of a Bell pair with a partner outside: rho_A is the maximally mixed state, k bits
    for k in (1, 2, 3):
        pairs = np.array([1.0 + 0j])
        for _ in range(k):
            pairs = np.kron(pairs, np.array([1, 0, 0, 1]) / np.sqrt(2))  # sites (0, 1), (2, 3), ...
        keep = list(range(0, 2 * k, 2))
        rho = _reduced(pairs, keep, 2)
        assert np.allclose(rho, np.eye(2**k) / 2**k, rtol=0, atol=1e-15)
        assert abs(entropy_vn(rho) - k) < 1e-12
    assert abs(entropy_vn(np.eye(27), base=3.0) - 3.0) < 1e-12


@pytest.mark.parametrize("d,n", [(2, 4), (3, 3), (4, 2)])
def test_keeping_every_site_returns_the_projector(d, n):
    rng = np.random.default_rng(7)
    psi = _rand(rng, d**n)
    rho = _reduced(psi, range(n), d)
    assert np.allclose(rho, np.outer(psi, psi.conj()), rtol=0, atol=1e-14 * np.vdot(psi, psi).real)

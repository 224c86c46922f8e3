"""Host reference of the device observables (tests/test_gpu_observe.py), in ``np.longdouble``.

Plain NumPy on the oracle's Hamiltonian; nothing here calls into ``pulser_amd.engine``.  Every function returns, next
to its value, ``S_abs`` = the sum of the absolute values of the summands it added up: the scale of the rounding-error
bounds of the tests (any summation order of m terms errs by at most (m - 1) u S_abs).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U53 = 2.0 ** -53  # unit roundoff of the device's float64 arithmetic


def ket_probabilities(x):
    """|x_i|^2 in longdouble."""
    x = np.asarray(x)
    re, im = x.real.astype(LD), x.imag.astype(LD)
    return re * re + im * im


def ref_pairs(p, n):
    """(norm, <n_k> [n], <n_k n_l> [n, n], S_abs) of a probability vector ``p`` [2^n], n_k(i) = 1 - bit_{n-1-k}(i).

    One longdouble sum per pair k <= l over the indices whose bits n-1-k and n-1-l are both 0; no D x n matrix.
    ``S_abs`` (norm, [n], [n, n]) holds the same sums of |p_i| (p may be the diagonal of any Hermitian matrix)."""
    p = np.asarray(p).astype(LD)
    D = 1 << n
    assert p.shape == (D,)
    a = np.abs(p)
    idx = np.arange(D, dtype=np.uint32)
    occ, corr = np.zeros(n, LD), np.zeros((n, n), LD)
    occ_abs, corr_abs = np.zeros(n, LD), np.zeros((n, n), LD)
    for k in range(n):
        keep = (idx & np.uint32(1 << (n - 1 - k))) == 0
        pk, ak, ik = p[keep], a[keep], idx[keep]
        for l in range(k, n):
            sel = (ik & np.uint32(1 << (n - 1 - l))) == 0
            corr[k, l] = corr[l, k] = pk[sel].sum(dtype=LD)
            corr_abs[k, l] = corr_abs[l, k] = ak[sel].sum(dtype=LD)
        occ[k], occ_abs[k] = corr[k, k], corr_abs[k, k]
    return p.sum(dtype=LD), occ, corr, (a.sum(dtype=LD), occ_abs, corr_abs)


def ref_energy_ket(ham, t, x):
    """(<x|H|x>, <Hx|Hx>, S_abs = (sum |x_i||w_i|, sum |w_i|^2), w = H(t) x) with the oracle's matrix-free ``apply``
    and the two dot products accumulated in longdouble."""
    x = np.asarray(x, dtype=np.complex128)
    w = np.asarray(ham.apply(float(t), x))
    xr, xi, wr, wi = (v.astype(LD) for v in (x.real, x.imag, w.real, w.imag))
    e1 = (xr * wr + xi * wi).sum(dtype=LD)  # Re <x|w>; the imaginary part vanishes for a Hermitian H
    w2 = wr * wr + wi * wi
    e2 = w2.sum(dtype=LD)
    s1 = (np.sqrt(xr * xr + xi * xi) * np.sqrt(w2)).sum(dtype=LD)
    return e1, e2, (s1, e2), w


def ref_energy_dm(ham, t, rho):
    """(Tr(H rho), Tr(H^2 rho), S_abs = (sum |H_ab||rho_ba|, sum |H_ab||H_bc||rho_ca|)) from the dense H(t), every
    product and sum in (complex) longdouble.  Only the non-zero elements of H are visited: D (N + 1) terms for the first
    moment, D (N + 1)^2 for the second."""
    H = np.asarray(ham.matrix(float(t)).toarray())
    rho = np.asarray(rho)
    D = H.shape[0]
    assert H.shape == rho.shape == (D, D)
    r, c = np.nonzero(H)  # row-major order: sorted by r
    v = H[r, c].astype(CLD)
    rl = rho.astype(CLD)
    t1 = v * rl[c, r]
    # second moment: join the non-zeros (a, b) with the non-zeros (b, c') of row b
    cnt = np.bincount(r, minlength=D)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rep = cnt[c]                                   # partners of every first factor
    first = np.repeat(np.arange(len(r)), rep)
    offs = np.arange(rep.sum()) - np.repeat(np.cumsum(rep) - rep, rep)
    second = start[c[first]] + offs
    assert np.array_equal(r[second], c[first])
    t2 = v[first] * v[second] * rl[c[second], r[first]]
    s1 = (np.abs(v) * np.abs(rl[c, r])).sum(dtype=LD)
    s2 = (np.abs(v[first]) * np.abs(v[second]) * np.abs(rl[c[second], r[first]])).sum(dtype=LD)
    return t1.sum(dtype=CLD).real, t2.sum(dtype=CLD).real, (s1, s2)


# ---------------------------------------------------------------------------------------------------------------------
# Tolerances of tests/test_gpu_observe.py, derived (never fitted to what the kernels give):
#  * a sum of m float64 terms in any order, atomics included, errs by at most (m - 1) u S_abs, u = 2^-53; forming
#    x^2 + y^2 or a two-product term costs a few u more per term: (m + 8) u S_abs.
#  * one generator application is held to 1e-11 max(1, max|Hx|) per entry (tests/test_gpu_parity.py header);
#    through <x|w> that is 1e-11 ||x||_1 max(1, max|Hx|), through <w|w> 2e-11 ||Hx||_1 max(1, max|Hx|).
#  * density matrices: H enters through its coefficients, held to the same 1e-11 relative: 1e-11 S_abs on top of the
#    summation bound over the D (1 + N + N (N - 1) / 2) elements gathered.
# ---------------------------------------------------------------------------------------------------------------------
def tol_sum(m, s_abs):
    return (m + 8) * U53 * np.asarray(s_abs, dtype=np.float64)


def tol_energy_ket(x, w, s_abs):
    D = len(x)
    top = max(1.0, float(np.max(np.abs(w))))
    return (float(tol_sum(D, s_abs[0])) + 1e-11 * float(np.sum(np.abs(x))) * top,
            float(tol_sum(D, s_abs[1])) + 2e-11 * float(np.sum(np.abs(w))) * top)


def tol_energy_dm(n, s_abs):
    m = (1 << n) * (1 + n + n * (n - 1) // 2)
    return tuple(float(tol_sum(m, s)) + 1e-11 * float(s) for s in s_abs)


def ulp(v):
    """Spacing of float64 at |v| (elementwise)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)))

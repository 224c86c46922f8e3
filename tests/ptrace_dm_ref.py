"""Host reference of ``ryd_reduced_density_dm`` (tests/test_gpu_reduced_density_dm.py), in ``np.longdouble``.

Plain NumPy in the style of tests/ptrace_ref.py, with ``LD`` and ``U53`` of tests/observe_ref.py; nothing here calls into
``pulser_amd``.  Atom k is the digit at stride d^(n-1-k) (atom 0 most significant); the row index of the reduced matrix
is the number formed by the kept digits in ascending site order.  Nothing is assumed Hermitian: entry (a, a') is the
sum over r of the stored elements rho[idx(a, r)][idx(a', r)], both triangles read as they are.
"""
from __future__ import annotations

import numpy as np

from observe_ref import LD, U53
from ptrace_ref import sites_of


def kept_first_dm(rho, keep, d):
    """``rho`` [..., D, D] as [..., dA, dA, R]: the elements (idx(a, r), idx(a', r)), the rest digits of row and
    column equal."""
    rho = np.asarray(rho)
    n = sites_of(rho.shape[-1], d)
    assert rho.shape[-2] == rho.shape[-1]
    keep = tuple(sorted(int(k) for k in keep))
    assert len(set(keep)) == len(keep) and keep and 0 <= keep[0] and keep[-1] < n
    rest = tuple(k for k in range(n) if k not in keep)
    lead = rho.ndim - 2
    d_a, r = d ** len(keep), d ** len(rest)
    x = rho.reshape(rho.shape[:-2] + (d,) * (2 * n))
    x = x.transpose(tuple(range(lead)) + tuple(lead + k for k in keep) + tuple(lead + n + k for k in keep)
                    + tuple(lead + k for k in rest) + tuple(lead + n + k for k in rest))
    x = x.reshape(rho.shape[:-2] + (d_a, d_a, r, r))
    return np.diagonal(x, axis1=-2, axis2=-1)  # [..., dA, dA, R]


def ref_reduced_dm(states, start, keep, d):
    """((re, im), S_re, S_im) for ``states`` [T, B, D, D] and ``start`` [T, dA, dA] (complex):
    ``rho_A[t] = start[t] + sum_b sum_r rho(t, b)[idx(a, r)][idx(a', r)]``, real and imaginary parts summed apart in
    longdouble.  The scales of the rounding bound are the sums of the absolute values of the summands:
      S_re[a, a'] = |Re start| + sum |Re rho_ij|,   S_im[a, a'] = |Im start| + sum |Im rho_ij|."""
    start = np.asarray(start)
    m = kept_first_dm(states, keep, d)  # [T, B, dA, dA, R]
    t, b, d_a, _, r = m.shape
    assert start.shape == (t, d_a, d_a)
    x = m.real.astype(LD)
    y = m.imag.astype(LD)
    re = start.real.astype(LD) + x.sum(axis=(1, 4))
    im = start.imag.astype(LD) + y.sum(axis=(1, 4))
    s_re = np.abs(start.real).astype(LD) + np.abs(x).sum(axis=(1, 4))
    s_im = np.abs(start.imag).astype(LD) + np.abs(y).sum(axis=(1, 4))
    return (re, im), s_re, s_im


# ---------------------------------------------------------------------------------------------------------------------
# The project's tol_sum rule (tests/observe_ref.py), derived, not measured.  The real (imaginary) part of an entry is a
# sum, in some order, of the B R stored float64 numbers Re rho_ij (Im rho_ij) and the value found in `out`: there are no
# products, so nothing is rounded before it is added.  Whatever the order - a chain, slots added through LDS, partials of
# splits - the sum is made with B R additions, each of which errs by at most u = 2^-53 of the absolute value of its
# result, itself at most (1 + B R u) S with S the sum of the absolute values of the summands: (B R) u S to first
# order.  The second-order term is (B R)^2 u^2 S / 2 < u S for B R < 2^26; the 8 covers it with room to spare at every
# size used here.  n_terms = B R; when the call splits the r range over n_split workgroups the second kernel makes
# n_split more additions per part: the caller adds n_split to n_terms.
# ---------------------------------------------------------------------------------------------------------------------
def tol_reduced_dm(n_terms, s):
    return (n_terms + 8) * U53 * np.asarray(s, dtype=np.float64)

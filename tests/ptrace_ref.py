"""Host reference of ``ryd_reduced_density`` (tests/test_gpu_reduced_density.py), in ``np.longdouble``.

Plain NumPy in the style of tests/ensemble_ref.py, with ``LD`` and ``U53`` of tests/observe_ref.py; nothing here calls
into ``pulser_amd.engine``.  Atom k is the digit at stride d^(n-1-k) (atom 0 most significant, as
tests/general_observe_ref.py:16 has it); the row index of the reduced matrix is the number formed by the kept digits in
ascending site order.
"""
from __future__ import annotations

import numpy as np

from observe_ref import LD, U53


def sites_of(dim, d):
    n = int(round(np.log(dim) / np.log(d)))
    assert d**n == dim, (dim, d)
    return n


def kept_first(states, keep, d):
    """``states`` [..., d^n] with the digits permuted so that the kept ones lead: [..., dA, R]."""
    states = np.asarray(states)
    n = sites_of(states.shape[-1], d)
    keep = tuple(sorted(int(k) for k in keep))
    assert len(set(keep)) == len(keep) and keep and 0 <= keep[0] and keep[-1] < n
    rest = tuple(k for k in range(n) if k not in keep)
    lead = states.ndim - 1
    x = states.reshape(states.shape[:-1] + (d,) * n)
    x = x.transpose(tuple(range(lead)) + tuple(lead + k for k in keep + rest))
    return x.reshape(states.shape[:-1] + (d ** len(keep), d ** len(rest)))


def ref_reduced(states, start, keep, d):
    """(rho, S_re, S_im) for ``states`` [T, B, D] and ``start`` [T, dA, dA] (complex):
    ``rho[t] = start[t] + sum_b M M^dagger`` with M the ket (t, b) as a dA x R matrix, every product and sum in
    longdouble (real and imaginary parts apart: NumPy has no use for a complex longdouble here).  The scales of the
    rounding bound are the sums of the absolute values of the summands:
      S_re[a, a'] = |Re start| + sum (|x_a x_a'| + |y_a y_a'|),   S_im[a, a'] = |Im start| + sum (|y_a x_a'| + |x_a y_a'|)."""
    start = np.asarray(start)
    m = kept_first(states, keep, d)  # [T, B, dA, R]
    t, b, d_a, r = m.shape
    assert start.shape == (t, d_a, d_a)
    x = m.real.astype(LD).transpose(0, 2, 1, 3).reshape(t, d_a, b * r)  # (the sum over b and r is one sum)
    y = m.imag.astype(LD).transpose(0, 2, 1, 3).reshape(t, d_a, b * r)
    xt, yt = x.transpose(0, 2, 1), y.transpose(0, 2, 1)
    ax, ay, axt, ayt = np.abs(x), np.abs(y), np.abs(xt), np.abs(yt)
    re = start.real.astype(LD) + x @ xt + y @ yt
    im = start.imag.astype(LD) + y @ xt - x @ yt
    s_re = np.abs(start.real).astype(LD) + ax @ axt + ay @ ayt
    s_im = np.abs(start.imag).astype(LD) + ay @ axt + ax @ ayt
    return (re, im), s_re, s_im


# ---------------------------------------------------------------------------------------------------------------------
# The project's tol_sum rule (tests/observe_ref.py).  The real (imaginary) part of an entry is a sum, in some order, of
# 2 B R float64 products - x_a x_a' and y_a y_a' (y_a x_a' and -x_a y_a') for each of the B R columns - and the value
# found: 2 B R additions, each at most u = 2^-53 of the running sum of absolute values, so at most 2 B R u S.  A product
# is rounded once unless it is fused into the addition (one rounding then covers both): eight u more, as tol_diag
# (tests/ensemble_ref.py) allows for forming the terms, cover that and the few extra additions of partial sums that an
# order which is not a single chain makes.  n_terms = B R; when the call splits the r range over n_split workgroups the
# second kernel makes n_split more additions per part: the caller adds n_split to n_terms (2 u each, more than the one
# they cost).
# ---------------------------------------------------------------------------------------------------------------------
def tol_reduced(n_terms, s):
    return (2 * n_terms + 8) * U53 * np.asarray(s, dtype=np.float64)

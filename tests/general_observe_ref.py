"""Host reference of the general-path device observables (tests/test_gpu_general_observe.py), in ``np.longdouble``.

The d-level companion of tests/observe_ref.py: pair sums for any local dimension and any ``one`` digit.  Energies need no
new reference - ``observe_ref.ref_energy_ket`` / ``ref_energy_dm`` take any oracle Hamiltonian - only a tolerance for
the density case, whose two-level version hard-codes the term count of an Ising register.  Nothing here calls into
``pulser_amd.engine``.
"""
from __future__ import annotations

import numpy as np

from observe_ref import LD, tol_sum


def digits_of(n, d):
    """int[d^n, n]: digit k of index i, atom k at stride d^(n-1-k) (atom 0 most significant)."""
    idx = np.arange(d**n, dtype=np.int64)
    return np.stack([(idx // d ** (n - 1 - k)) % d for k in range(n)], axis=1)


def ref_pairs_d(p, n, d, one):
    """(norm, <n_k> [n], <n_k n_l> [n, n], S_abs) of a probability vector ``p`` [d^n], n_k(i) = (digit_k(i) == one).

    One longdouble sum per pair k <= l over the selected indices; ``S_abs`` (norm, [n], [n, n]) holds the same sums
    of |p_i| (p may be the diagonal of any Hermitian matrix)."""
    p = np.asarray(p).astype(LD)
    assert p.shape == (d**n,) and 0 <= one < d
    a = np.abs(p)
    is_one = digits_of(n, d) == one
    occ, corr = np.zeros(n, LD), np.zeros((n, n), LD)
    occ_abs, corr_abs = np.zeros(n, LD), np.zeros((n, n), LD)
    for k in range(n):
        keep = is_one[:, k]
        pk, ak, sk = p[keep], a[keep], is_one[keep]
        for l in range(k, n):
            sel = sk[:, l]
            corr[k, l] = corr[l, k] = pk[sel].sum(dtype=LD)
            corr_abs[k, l] = corr_abs[l, k] = ak[sel].sum(dtype=LD)
        occ[k], occ_abs[k] = corr[k, k], corr_abs[k, k]
    return p.sum(dtype=LD), occ, corr, (a.sum(dtype=LD), occ_abs, corr_abs)


# ---------------------------------------------------------------------------------------------------------------------
# Tolerance of Tr(H rho), Tr(H^2 rho) of the general path, derived (never fitted to what the kernels give).  The device
# applies H to the D columns of rho (W = H X, one entry of W per row and column), applies it again (W2 = H W) and sums
# the D diagonal entries of W and of W2.
#  * summation: the reference adds m1 = nnz(H) products H_ab rho_ba for the first moment and m2 = the number of
#    non-zero triples H_ab H_bc rho_ca for the second; the device adds the same products grouped by row, then D trace
#    terms.  Any order of m terms errs by at most (m - 1) u S_abs; a few u more per term for the complex products:
#    (m + D + 8) u S_abs with observe_ref.ref_energy_dm's S_abs (sums of |H_ab||rho_ba| and |H_ab||H_bc||rho_ca|).
#  * one generator application is held to 1e-11 max(1, max|Hx|) per entry (tests/test_gpu_parity.py header, SURVEY 8d;
#    it covers the coefficients of H(t) evaluated on the device).  First application, column c:
#        |dW_ac| <= 1e-11 top1_c,   top1_c = max(1, max_a |(H rho)_ac|),
#    and the trace adds the D entries dW_cc:  1e-11 sum_c top1_c.
#  * second application: W2 + dW2 = H (W + dW) + e, |e_ac| <= 1e-11 top2_c with top2_c = max(1, max_a |(H^2 rho)_ac|),
#    so |dW2_cc| <= sum_a |H_ca| |dW_ac| + |e_cc| <= 1e-11 (r_c top1_c + top2_c), r_c = sum_a |H_ca| (row c of H),
#    and the trace adds them:  1e-11 sum_c (r_c top1_c + top2_c).
# ---------------------------------------------------------------------------------------------------------------------
def tol_energy_dm_general(ham, t, rho, s_abs):
    """(tolerance of Tr(H rho), tolerance of Tr(H^2 rho)); ``s_abs`` from ``observe_ref.ref_energy_dm``."""
    H = ham.matrix(float(t)).tocsr()
    rho = np.asarray(rho, dtype=np.complex128)
    D = H.shape[0]
    nnz_row = np.diff(H.indptr)
    m1 = int(H.nnz)
    m2 = int(nnz_row[H.indices].sum())  # partners (b, c) of every non-zero (a, b)
    w1 = H @ rho
    w2 = H @ w1
    top1 = np.maximum(1.0, np.max(np.abs(w1), axis=0))
    top2 = np.maximum(1.0, np.max(np.abs(w2), axis=0))
    rows = np.asarray(abs(H).sum(axis=1)).ravel()
    tol1 = float(tol_sum(m1 + D, s_abs[0])) + 1e-11 * float(top1.sum())
    tol2 = float(tol_sum(m2 + D, s_abs[1])) + 1e-11 * float((rows * top1 + top2).sum())
    return tol1, tol2

"""Host reference of ``engine.expect_sparse`` (tests/test_gpu_expect.py), in ``np.clongdouble``.

Plain NumPy / SciPy on the operator's stored non-zeros; nothing here calls into ``pulser_amd.engine``.  Next to its
value every function returns ``S_abs`` = the sum of the absolute values of the terms it added up, the scale of the
rounding-error bound below.

Tolerance (derived, never fitted to what the kernel gives), per real and per imaginary part, u = 2^-53:

 * the value is a sum of nnz complex terms.  A float64 sum of m terms in ANY order - lanes, shuffles, the LDS step and
   the atomics of different workgroups included - errs by at most (m - 1) u sum |term| (to first order in u): with
   |Re t|, |Im t| <= |t| that is (nnz - 1) u S_abs for either part.
 * a term is two complex products, conj(x_r) (v x_c).  One complex product formed from four real products and two
   additions has a relative error of at most sqrt(5) u < 3 u of the product's modulus in either part (Brent, Percival,
   Zimmermann 2007; fused multiply-adds only lower it); two products in a row, to first order, less than 6 u.  The
   density form v rho_cr has one product.  Either way below the 17 u the bound leaves for it.

   tol = (nnz + 16) u S_abs,   S_abs = sum_j |v_j| |x_r(j)| |x_c(j)|   (kets),   sum_j |v_j| |rho_c(j) r(j)|   (density)

The reference's own error, (nnz + 6) 2^-64 S_abs with x86's 80-bit longdouble, is 2^-11 of that and is not added.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
CLD = np.clongdouble
U53 = 2.0 ** -53  # unit roundoff of the device's float64 arithmetic


def triplets(operator):
    """(rows, cols, vals) of the stored non-zeros, duplicates summed, sorted by (row, col) - the list the wrapper uploads."""
    m = sp.csr_matrix(operator).astype(np.complex128)
    m.sum_duplicates()
    m.sort_indices()
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    return rows, np.asarray(m.indices), np.asarray(m.data)


def ref_expect_ket(operator, x):
    """(<x| O |x>, S_abs) of one ket x [D]: sum_j conj(x_r) v_j x_c, every product and the sum in clongdouble."""
    r, c, v = triplets(operator)
    x = np.asarray(x).reshape(-1).astype(CLD)
    assert x.shape == (sp.csr_matrix(operator).shape[0],)
    terms = np.conj(x[r]) * (v.astype(CLD) * x[c])
    s_abs = (np.abs(v).astype(LD) * np.abs(x[r]) * np.abs(x[c])).sum(dtype=LD)
    return terms.sum(dtype=CLD), s_abs


def ref_expect_dm(operator, rho):
    """(Tr(O rho), S_abs) of one density matrix rho [D, D]: sum_j v_j rho[c_j, r_j] in clongdouble."""
    r, c, v = triplets(operator)
    rho = np.asarray(rho).astype(CLD)
    assert rho.shape == sp.csr_matrix(operator).shape
    g = rho[c, r]
    return (v.astype(CLD) * g).sum(dtype=CLD), (np.abs(v).astype(LD) * np.abs(g)).sum(dtype=LD)


def ref_expect(operator, states, density=False):
    """Values [S] (clongdouble) and S_abs [S] (longdouble) over a stack of states."""
    one = ref_expect_dm if density else ref_expect_ket
    out = [one(operator, s) for s in states]
    return np.array([o[0] for o in out], dtype=CLD), np.array([o[1] for o in out], dtype=LD)


def tol_expect(nnz, s_abs):
    """(nnz + 16) u S_abs, for the real and for the imaginary part."""
    return (nnz + 16) * U53 * np.asarray(s_abs, dtype=np.float64)


def part_errors(got, ref):
    """max(|Re(got - ref)|, |Im(got - ref)|) elementwise, the difference taken in clongdouble."""
    d = np.asarray(got).astype(CLD) - np.asarray(ref).astype(CLD)
    return np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)

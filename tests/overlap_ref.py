"""Host reference of ``engine.overlap_many`` (tests/test_gpu_overlap_many.py), in ``np.clongdouble``.

Plain NumPy; nothing here calls into ``pulser_amd.engine``.  Next to its value every function returns ``S_abs`` = the
sum of the absolute values of the terms it added up, the scale of the rounding-error bound below.

Tolerances (derived, never fitted to what the kernel gives), per real and per imaginary part, u = 2^-53:

 * ``z = sum_e w_e x_e`` over the L stored elements of a state (L = dim for kets, dim^2 for density matrices).  A
   float64 sum of m terms in ANY order - lanes, shuffles, the LDS step and the atomics of different workgroups
   included - errs by at most (m - 1) u sum |term| (to first order in u): with |Re t|, |Im t| <= |t| that is
   (L - 1) u S_abs for either part.
 * a term of target form 0 is one complex product conj(a_e) x_e (the conjugation is exact): formed from four real
   products and two additions it has a relative error of at most sqrt(5) u < 3 u of the product's modulus in either
   part (Brent, Percival, Zimmermann 2007; fused multiply-adds only lower it).  A term of target form 1 multiplies
   three complex factors, (conj(phi_i) phi_j) rho_ij - two products in a row: to first order less than 6 u, and less
   than 9 u even if each of the three factors' handling is charged a full product.  Either way below the 17 u the bound
   leaves for it.

       tol_z = (L + 16) u S_abs,   S_abs = sum_e |a_e| |x_e|  (form 0),   sum_ij |phi_i| |phi_j| |rho_ij|  (form 1)

 * the norm of a ket, sum_e |x_e|^2, is a sum of L = dim non-negative terms, each (Re x_e)^2 + (Im x_e)^2 formed with
   at most two roundings (one when fused): (L - 1) u for the sum in any order, 2 u for a term, of the norm, and one u
   to spare.  (Where the compiler fuses both squares into the running sum, a lane adds 2 numbers per element; no
   chain of additions through a lane's 8 elements, the 6 shuffle steps, the LDS step and the atomics of the chunks is
   then longer than 16 + 6 + 3 + dim / 2048, and with fewer than 64 elements only log2(dim) shuffle steps add two
   non-zero numbers: 2 + 1 at dim = 2, 2 + 3 at dim = 8 - inside (L + 2) u at every size.)

       tol_norm = (L + 2) u norm,   L = dim summed terms

 * the trace, sum_i Re rho_ii, adds dim stored numbers as they are:

       tol_trace = (dim + 2) u sum_i |Re rho_ii|

The finished values follow to first order, with dz the bound of either part of z (|delta z| <= sqrt(2) dz) and dn that
of the norm or trace n:

       |z|^2 / n:   2 |z| sqrt(2) dz / n  +  |z|^2 dn / n^2            (``tol_fidelity_ket``)
       Re z / n:    dz / |n|  +  |Re z| dn / n^2                         (``tol_ratio``, also either part of e / n)

The reference's own error, about (L + 6) 2^-64 S_abs with x86's 80-bit longdouble, is 2^-11 of that and is not added.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U53 = 2.0 ** -53  # unit roundoff of the device's float64 arithmetic


def ref_overlap(states, targets, density=False, outer=False):
    """(z [S, F] clongdouble, S_abs [S, F] longdouble).  ``states`` [S, D] or, with ``density``, [S, D, D] read as stored;
    ``targets`` [F, D] / [F, D * D] / [F, D, D], or with ``outer`` [F, D] used as A = |phi><phi|."""
    states = np.asarray(states)
    S = states.shape[0]
    x = states.reshape(S, -1).astype(CLD)
    targets = np.asarray(targets)
    F = targets.shape[0]
    if outer:
        assert density
        phi = targets.reshape(F, -1).astype(CLD)
        w = (np.conj(phi)[:, :, None] * phi[:, None, :]).reshape(F, -1)            # conj(phi_i) phi_j at e = i D + j
        w_abs = (np.abs(phi)[:, :, None] * np.abs(phi)[:, None, :]).reshape(F, -1)
    else:
        w = np.conj(targets.reshape(F, -1).astype(CLD))
        w_abs = np.abs(w)
    assert w.shape == (F, x.shape[1]), (w.shape, x.shape)
    z = np.empty((S, F), dtype=CLD)
    s_abs = np.empty((S, F), dtype=LD)
    ax = np.abs(x)
    for s in range(S):
        for f in range(F):
            z[s, f] = (w[f] * x[s]).sum(dtype=CLD)
            s_abs[s, f] = (w_abs[f] * ax[s]).sum(dtype=LD)
    return z, s_abs


def ref_norm(states, density=False):
    """(norm [S] longdouble, S_abs [S] longdouble): sum |x_e|^2 for kets (S_abs = the norm itself), sum_i Re rho_ii for
    density matrices (S_abs = sum_i |Re rho_ii|)."""
    states = np.asarray(states)
    if density:
        d = np.real(np.diagonal(states, axis1=1, axis2=2)).astype(LD)
        return d.sum(axis=1, dtype=LD), np.abs(d).sum(axis=1, dtype=LD)
    x = states.reshape(states.shape[0], -1)
    n = (x.real.astype(LD) ** 2 + x.imag.astype(LD) ** 2).sum(axis=1, dtype=LD)
    return n, n


def tol_z(n_terms, s_abs):
    """(L + 16) u S_abs, for the real and for the imaginary part."""
    return (n_terms + 16) * U53 * np.asarray(s_abs, dtype=np.float64)


def tol_norm(dim, norm):
    """(L + 2) u norm with L = dim summed terms."""
    return (dim + 2) * U53 * np.asarray(norm, dtype=np.float64)


def tol_trace(dim, s_abs):
    """(dim + 2) u sum |Re rho_ii|."""
    return (dim + 2) * U53 * np.asarray(s_abs, dtype=np.float64)


def tol_fidelity_ket(z, n, dz, dn):
    """First-order bound of |z|^2 / n."""
    z, n = np.abs(np.asarray(z).astype(np.complex128)), np.asarray(n, dtype=np.float64)
    return 2 * z * np.sqrt(2.0) * dz / n + z ** 2 * dn / n ** 2


def tol_ratio(v, n, dv, dn):
    """First-order bound of v / n for one real part v with bound dv."""
    v, n = np.abs(np.asarray(v, dtype=np.float64)), np.asarray(n, dtype=np.float64)
    return dv / np.abs(n) + v * dn / n ** 2


def part_errors(got, ref):
    """max(|Re(got - ref)|, |Im(got - ref)|) elementwise, the difference taken in clongdouble."""
    d = np.asarray(got).astype(CLD) - np.asarray(ref).astype(CLD)
    return np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)

"""GPU: ``ryd_reduced_density`` (k_ptrace, k_ptrace_sum) through ``ctypes`` and through ``engine.reduced_density``
against the longdouble reference of tests/ptrace_ref.py, entry by entry.

Bounds (none fitted to what the kernels give): ``tol_reduced(B R + n_split, S)`` of tests/ptrace_ref.py for the real and
the imaginary part of every entry, S the sum of the absolute values of the summands of that part (the value found in
``out`` among them); ``n_split`` is added only where a split is forced or may have been chosen (``n_split = 0`` on a
large ket: the engine's own cap, ``min(1024 // T, D // 512)``, stands in for the number the library chose - no test
asserts that number).  Two chunk calls: the sum of the two calls' bounds.  Exact structure (Hermiticity bit for bit, an
untouched imaginary diagonal, bitwise repeatability) is asserted with ``array_equal``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from observe_ref import LD
from ptrace_ref import ref_reduced, tol_reduced

from pulser_amd import _lib, entropy_vn

pytestmark = pytest.mark.gpu

SENTINEL = complex(-7.25, 3.5)


def _torch():
    import torch

    return torch


def _rand(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _hermitian(rng, t, d_a):
    a = _rand(rng, t, d_a, d_a)
    return a + a.conj().transpose(0, 2, 1)


def _within(got, ref, s_re, s_im, n_terms, what):
    """Entry by entry, real and imaginary parts apart; prints the worst error over its bound."""
    (re, im) = ref
    worst = 0.0
    for g, r, s in ((got.real, re, s_re), (got.imag, im, s_im)):
        tol = tol_reduced(n_terms, s)
        err = np.abs(g.astype(LD) - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.max(np.where(err > 0, err / tol.astype(LD), 0))))
        assert np.all(err <= tol), (what, float(np.max(err)), float(np.min(tol)))
    print(f"RATIO reduced_density {what}: {worst:.3e}")


def _engine_call(x_dev, keep, d, start, n_split=0):
    """``engine.reduced_density`` into a buffer that sits inside a larger tensor prefilled with a sentinel; returns the
    result after checking that the surroundings are untouched."""
    from pulser_amd.engine import reduced_density

    torch = _torch()
    t, d_a = start.shape[0], start.shape[1]
    big = torch.full((t + 2, d_a, d_a), SENTINEL, dtype=torch.complex128, device="cuda")
    out = big[1:t + 1]
    out.copy_(torch.from_numpy(start))
    assert reduced_density(x_dev, keep, d, out=out, n_split=n_split) is out
    host = big.cpu().numpy()
    assert np.all(host[0] == SENTINEL) and np.all(host[-1] == SENTINEL)
    return host[1:t + 1]


def _ctypes_call(x_dev, keep, d, start, n_split=1, scratch_bytes=None):
    """The C entry point itself on a contiguous [T, B, D] tensor; returns (status, out)."""
    torch = _torch()
    t, b, dim = (int(v) for v in x_dev.shape)
    d_a = start.shape[1]
    n = int(round(np.log(dim) / np.log(d)))
    out = torch.from_numpy(start.copy()).cuda()
    keep_arr = np.ascontiguousarray(sorted(keep), dtype=np.int32)
    need = t * max(n_split, 1) * d_a * d_a * 16
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") if n_split != 1 else None
    rc = _lib.load().ryd_reduced_density(
        x_dev.data_ptr(), t, b, b * dim, dim, dim, d, n, keep_arr.ctypes.data, len(keep_arr), out.data_ptr(), n_split,
        None if scratch is None else scratch.data_ptr(), 0 if scratch is None else (need if scratch_bytes is None else scratch_bytes),
        0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check_both_ways(x, keep, d, start, what):
    torch = _torch()
    dev = torch.from_numpy(x).cuda()
    ref, s_re, s_im = ref_reduced(x, start, keep, d)
    n_terms = x.shape[1] * (x.shape[2] // start.shape[1])
    got = _engine_call(dev, keep, d, start, n_split=1)
    _within(got, ref, s_re, s_im, n_terms, f"{what} engine")
    rc, got_c = _ctypes_call(dev, keep, d, start, n_split=1)
    assert rc == 0, _lib.load().ryd_last_error()
    assert np.array_equal(got, got_c)  # the same call: bitwise
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes: the smallest at which each mechanism can go wrong
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [
    (2, 1, [0]), (2, 2, [0]), (2, 2, [1]), (2, 2, [0, 1]),
    (2, 7, [0]), (2, 7, [6]), (2, 7, [0, 6]), (2, 7, [2, 3]), (2, 7, [1, 3, 5]), (2, 7, [0, 1, 2, 3]),
    (2, 7, [2, 3, 4, 5, 6]), (2, 7, [0, 1, 2, 4, 5, 6]),
    (2, 6, [0, 1, 2, 3, 4, 5]), (2, 10, [4, 5, 6, 7, 8, 9]), (2, 10, [0, 1, 2, 3, 4, 5]),
    (3, 4, [1]), (3, 4, [0, 3]), (3, 4, [1, 2, 3]), (3, 5, [0, 2, 4]),
    (4, 4, [3]), (4, 4, [0, 2]), (4, 4, [0, 1, 3]),
]


@pytest.mark.parametrize("d,n,keep", SHAPES, ids=[f"d{d}n{n}k{''.join(map(str, k))}" for d, n, k in SHAPES])
def test_kernel_matches_the_reference(d, n, keep):
    rng = np.random.default_rng(1000 * d + 10 * n + sum(keep))
    t, b = 2, 2
    x = _rand(rng, t, b, d**n)
    d_a = d ** len(keep)
    start = _hermitian(rng, t, d_a)
    got = _check_both_ways(x, keep, d, start, f"d={d} n={n} keep={keep}")
    # Hermitian start, Hermitian sum: bit for bit
    assert np.array_equal(got, got.conj().transpose(0, 2, 1))


def test_an_unsorted_keep_is_sorted_by_the_wrapper():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    x = _rand(np.random.default_rng(5), 1, 1, 2**5)
    dev = torch.from_numpy(x).cuda()
    a = reduced_density(dev, [3, 0, 2]).cpu().numpy()
    b = reduced_density(dev, (0, 2, 3)).cpu().numpy()
    assert np.array_equal(a, b) and a.shape == (1, 8, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 2. accumulation and strides
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 8, 9])
def test_trajectory_axis_is_summed_onto_what_out_holds(B):
    rng = np.random.default_rng(20 + B)
    x = _rand(rng, 3, B, 2**6)
    start = _rand(rng, 3, 4, 4)  # any values, Hermitian or not: S carries their absolute values
    _check_both_ways(x, [1, 4], 2, start, f"B={B}")


def test_one_time_with_several_trajectories():
    rng = np.random.default_rng(31)
    x = _rand(rng, 1, 5, 3**4)
    _check_both_ways(x, [0, 2], 3, np.zeros((1, 9, 9), dtype=complex), "T=1 B=5 qutrits")


def test_two_chunk_calls_against_one_reference_over_both():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    rng = np.random.default_rng(32)
    x = _rand(rng, 2, 7 + 4, 2**7)
    keep = [0, 3, 6]
    out = torch.zeros((2, 8, 8), dtype=torch.complex128, device="cuda")
    for part in (x[:, :7], x[:, 7:]):
        reduced_density(torch.from_numpy(np.ascontiguousarray(part)).cuda(), keep, out=out, n_split=1)
    ref, s_re, s_im = ref_reduced(x, np.zeros((2, 8, 8), dtype=complex), keep, 2)
    # the sum of the two calls' bounds: (2 * 7 R + 8) + (2 * 4 R + 8) = 2 * 11 R + 16 units, on scales no larger than S
    _within(out.cpu().numpy(), ref, s_re, s_im, 11 * 16 + 4, "two chunks")


def test_every_third_time_and_a_padded_trajectory_stride():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    rng = np.random.default_rng(33)
    big = _rand(rng, 10, 5, 2**6 + 24)
    dev = torch.from_numpy(big).cuda()
    view = dev[1::3, 1:4, 8:8 + 64]  # times 1, 4, 7; stride_b = 88 > 64; a gap after every time
    assert tuple(view.shape) == (3, 3, 64) and view.stride(1) == 88 and view.stride(0) == 3 * 5 * 88
    got = reduced_density(view, [0, 5], n_split=1).cpu().numpy()
    sub = big[1::3, 1:4, 8:8 + 64]
    ref, s_re, s_im = ref_reduced(sub, np.zeros((3, 4, 4), dtype=complex), [0, 5], 2)
    _within(got, ref, s_re, s_im, 3 * 16, "strided view")
    assert np.array_equal(dev.cpu().numpy(), big)  # the states are only read
    # one matrix per (t, b): the caller's reshape
    each = reduced_density(dev[:, :, :64].reshape(50, 1, 64) if dev[:, :, :64].is_contiguous()
                           else dev[:, :, :64].contiguous().reshape(50, 1, 64), [0, 5], n_split=1).cpu().numpy()
    ref, s_re, s_im = ref_reduced(big[:, :, :64].reshape(50, 1, 64), np.zeros((50, 4, 4), dtype=complex), [0, 5], 2)
    _within(each, ref, s_re, s_im, 16, "one matrix per (t, b)")


def test_66000_times_walk_the_grid_stride():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    rng = np.random.default_rng(34)
    x = _rand(rng, 66000, 1, 4)
    got = reduced_density(torch.from_numpy(x).cuda(), [1]).cpu().numpy()
    ref, s_re, s_im = ref_reduced(x, np.zeros((66000, 2, 2), dtype=complex), [1], 2)
    _within(got, ref, s_re, s_im, 2, "66 000 times")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the split of one ket over workgroups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,keep", [(8, [0, 7]), (14, [0, 13]), (14, [3, 4, 5, 6, 7])])
@pytest.mark.parametrize("n_split", [1, 2, 3, 7])
def test_forced_split_is_within_its_bound_and_repeatable(n_split, n, keep):
    """(8 atoms: the issue's case, one tile per ket - all but one partial are zeros; 14 atoms: 8 tiles per ket, which 3 and 7
    divide unevenly.)"""
    torch = _torch()
    rng = np.random.default_rng(40 + n_split + n)
    x = _rand(rng, 2, 2, 2**n)
    d_a = 2 ** len(keep)
    start = _hermitian(rng, 2, d_a)
    dev = torch.from_numpy(x).cuda()
    ref, s_re, s_im = ref_reduced(x, start, keep, 2)
    n_terms = 2 * (2**n // d_a) + (n_split if n_split > 1 else 0)
    got = _engine_call(dev, keep, 2, start, n_split=n_split)
    _within(got, ref, s_re, s_im, n_terms, f"n={n} keep={keep} n_split={n_split}")
    again = _engine_call(dev, keep, 2, start, n_split=n_split)
    assert np.array_equal(got, again)
    rc, got_c = _ctypes_call(dev, keep, 2, start, n_split=n_split)
    assert rc == 0 and np.array_equal(got, got_c)
    assert np.array_equal(got, got.conj().transpose(0, 2, 1))


def test_a_scratch_one_byte_too_small_is_refused():
    torch = _torch()
    x = torch.ones((2, 1, 2**8), dtype=torch.complex128, device="cuda")
    start = np.full((2, 4, 4), 5.0 + 0j)
    need = 2 * 2 * 16 * 16
    rc, out = _ctypes_call(x, [0, 7], 2, start, n_split=2, scratch_bytes=need - 1)
    assert rc == -1 and "scratch" in _lib.load().ryd_last_error().decode()
    assert np.array_equal(out, start)  # nothing was launched
    rc, _ = _ctypes_call(x, [0, 7], 2, start, n_split=2, scratch_bytes=need)
    assert rc == 0


def test_library_chosen_split_on_one_large_ket():
    torch = _torch()
    rng = np.random.default_rng(45)
    n, keep = 18, [0, 1, 2, 17]
    x = _rand(rng, 1, 1, 2**n)
    start = np.zeros((1, 16, 16), dtype=complex)
    dev = torch.from_numpy(x).cuda()
    ref, s_re, s_im = ref_reduced(x, start, keep, 2)
    got = _engine_call(dev, keep, 2, start, n_split=0)
    _within(got, ref, s_re, s_im, 2**n // 16 + min(1024, 2**n // 512), "n=18 n_split=0")
    assert np.array_equal(got, _engine_call(dev, keep, 2, start, n_split=0))


# ---------------------------------------------------------------------------------------------------------------------
# 4. exact structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,keep,n_split", [(2, 9, [1, 8], 1), (2, 9, [0, 2, 4, 6, 8], 1), (3, 5, [1, 2, 4], 1),
                                              (2, 13, [0, 1, 2, 3, 4, 12], 3)])
def test_lower_triangle_is_the_conjugate_and_the_imaginary_diagonal_is_untouched(d, n, keep, n_split):
    torch = _torch()
    rng = np.random.default_rng(50 + n)
    x = _rand(rng, 2, 3, d**n)
    d_a = d ** len(keep)
    start = _hermitian(rng, 2, d_a)
    k = np.arange(d_a)
    start[:, k, k] += 1j * 0.3125  # a value the kernel must leave alone
    got = _engine_call(torch.from_numpy(x).cuda(), keep, d, start, n_split=n_split)
    assert np.all(got.imag[:, k, k] == 0.3125)
    off = got.copy()
    off[:, k, k] = off[:, k, k].real
    assert np.array_equal(off, off.conj().transpose(0, 2, 1))
    assert np.all(got.real[:, k, k] > start.real[:, k, k])  # (and something was added)


# ---------------------------------------------------------------------------------------------------------------------
# 5. known answers
# ---------------------------------------------------------------------------------------------------------------------
def test_product_ket_of_14_atoms_gives_rank_one():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    rng = np.random.default_rng(60)
    single = _rand(rng, 14, 2)
    single /= np.linalg.norm(single, axis=1)[:, None]
    psi = np.array([1.0 + 0j])
    for k in range(14):
        psi = np.kron(psi, single[k])
    for keep in ([0], [13], [2, 5, 11], [0, 1, 2, 3, 4, 5]):
        rho = reduced_density(torch.from_numpy(psi.reshape(1, 1, -1)).cuda(), keep).cpu().numpy()[0]
        want = np.array([1.0 + 0j])
        for k in keep:
            want = np.kron(want, single[k])
        d_a, r = len(want), 2**14 // len(want)
        # The kernel: every part of every entry has S <= 1 (Cauchy-Schwarz on unit vectors) -> tol_reduced(R + n_split, 1)
        # with the engine's cap min(1024, D // 512) for n_split.  The inputs: an amplitude of |psi> is a product of 14
        # rounded complex factors (13 products, relative error <= sqrt(5) u each: 30 u), an entry is bilinear in them
        # (60 u), the 14 - |keep| traced factors have squared norms 1 +- 3 u (42 u), `want` has its own few products
        # (2 * 5 * sqrt(5) u < 23 u): 125 u on entries of modulus <= 1, sqrt(2) of it for the complex modulus.
        tol = np.sqrt(2) * (float(tol_reduced(r + min(1024, 2**14 // 512), 1.0)) + 125 * 2.0**-53)
        assert np.max(np.abs(rho - np.outer(want, want.conj()))) <= tol
        # purity Tr rho^2 = 1: rho = P + delta with P = |w><w|, |delta_ij| <= tol, sum |P_ij| = (sum |w_i|)^2 <= d_a and
        # sum |P_ij|^2 = |w|^4 = 1 +- 12 u
        assert abs(np.sum(np.abs(rho) ** 2) - 1.0) <= 2 * d_a * tol + d_a * d_a * tol * tol + 12 * 2.0**-53


def test_ghz_of_10_qubits_has_one_bit_everywhere():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    psi = np.zeros(2**10, dtype=complex)
    psi[0] = psi[-1] = np.sqrt(0.5)
    dev = torch.from_numpy(psi.reshape(1, 1, -1)).cuda()
    for keep in ([0], [0, 9], [3, 4, 5, 6, 7, 8]):
        rho = reduced_density(dev, keep).cpu().numpy()[0]
        assert abs(entropy_vn(rho) - 1.0) < 1e-12
        assert abs(np.trace(rho) - 1.0) < 1e-15


# ---------------------------------------------------------------------------------------------------------------------
# 6. nothing to do, and what is refused
# ---------------------------------------------------------------------------------------------------------------------
def test_no_times_launches_nothing_and_invalid_arguments_are_refused():
    from pulser_amd.engine import reduced_density

    torch = _torch()
    lib = _lib.load()
    x = torch.ones((2, 3, 8), dtype=torch.complex128, device="cuda")
    o = torch.full((2, 2, 2), 5.0, dtype=torch.complex128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    px, po = x.data_ptr(), o.data_ptr()
    keep = np.array([1], dtype=np.int32)
    bad = np.array([2, 1], dtype=np.int32)
    pk = keep.ctypes.data
    tail = (1, None, 0, 0, stream)
    assert lib.ryd_reduced_density(px, 0, 3, 24, 8, 8, 2, 3, pk, 1, po, *tail) == 0
    assert tuple(reduced_density(x[:0], [1]).shape) == (0, 2, 2)
    for args in ((None, 2, 3, 24, 8, 8, 2, 3, pk, 1, po), (px, 2, 3, 24, 8, 8, 2, 3, pk, 1, None),
                 (px, 2, 3, 24, 8, 8, 2, 3, None, 1, po), (px, 2, 0, 24, 8, 8, 2, 3, pk, 1, po),
                 (px, -1, 3, 24, 8, 8, 2, 3, pk, 1, po), (px, 2, 3, 24, 8, 8, 2, 4, pk, 1, po),
                 (px, 2, 3, 24, 7, 8, 2, 3, pk, 1, po), (px, 2, 3, 7, 8, 8, 2, 3, pk, 1, po),
                 (px, 2, 3, 24, 8, 8, 2, 3, bad.ctypes.data, 2, po), (px, 2, 3, 24, 8, 8, 2, 3, pk, 0, po),
                 (px, 2, 3, 24, 8, 8, 5, 3, pk, 1, po)):
        assert lib.ryd_reduced_density(*args, *tail) == -1, args
        assert "reduced_density" in lib.ryd_last_error().decode()
    assert lib.ryd_reduced_density(px, 2, 3, 24, 8, 8, 2, 3, pk, 1, po, 2, None, 0, 0, stream) == -1  # a split, no scratch
    torch.cuda.synchronize()
    assert torch.all(o == 5.0)  # nothing was launched
    # the wrapper's own checks
    with pytest.raises(TypeError):
        reduced_density(x.to(torch.complex64), [1])
    with pytest.raises(ValueError):
        reduced_density(x.cpu(), [1])
    with pytest.raises(ValueError):
        reduced_density(x, [])
    with pytest.raises(ValueError):
        reduced_density(x, [1, 1])
    with pytest.raises(ValueError):
        reduced_density(x, [3])
    with pytest.raises(ValueError):
        reduced_density(x, [0], local_dim=3)  # 8 is no power of 3
    with pytest.raises(ValueError):
        reduced_density(x, [1], out=o[:, :1])
    with pytest.raises(TypeError):
        reduced_density(x, [1], out=o.to(torch.complex64))
    with pytest.raises(ValueError):
        reduced_density(x[:, :1].expand(2, 3, 8), [1])  # stride_b = 0
    with pytest.raises(ValueError):
        reduced_density(x.transpose(1, 2).contiguous().transpose(1, 2), [1])  # last axis not contiguous
    with pytest.raises(ValueError, match="64"):
        reduced_density(torch.ones((1, 1, 2**7), dtype=torch.complex128, device="cuda"), range(7))

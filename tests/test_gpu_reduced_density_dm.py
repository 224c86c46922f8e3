"""GPU: ``ryd_reduced_density_dm`` (k_ptrace_dm, k_ptrace_dm_sum) through ``ctypes`` and through
``engine.reduced_density_dm`` against the longdouble reference of tests/ptrace_dm_ref.py, entry by entry.

Inputs are seeded NON-Hermitian complex matrices of mixed signs and magnitudes: a kernel that reads rho[j][i], mirrors a
triangle or conjugates fails on them.  Bounds (none fitted to what the kernels give): ``tol_reduced_dm(B R + n_split,
S)`` of tests/ptrace_dm_ref.py for the real and the imaginary part of every entry, S the sum of the absolute values of
the summands of that part (the value found in ``out`` among them); ``n_split`` is added only where a split is forced or
may have been chosen (``n_split = 0``: ``engine.reduced_density_dm_splits``, the most partials the library takes, stands
in for the number it chose - no test asserts that number).  Two chunk calls: the sum of the two calls' bounds.  Known answers
whose summands are equal powers of two, and bitwise repeatability, are asserted with ``array_equal``.
"""
from __future__ import annotations

import numpy as np
import pytest

from observe_ref import LD
from ptrace_dm_ref import ref_reduced_dm, tol_reduced_dm

from pulser_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = complex(-7.25, 3.5)


def _torch():
    import torch

    return torch


def _rand(rng, *shape):
    """No symmetry, both signs, magnitudes over six decades (powers of two: the scaling itself is exact)."""
    z = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return z * np.exp2(rng.integers(-10, 11, size=shape))


def _within(got, ref, s_re, s_im, n_terms, what):
    """Entry by entry, real and imaginary parts apart; prints the worst error over its bound."""
    (re, im) = ref
    worst = 0.0
    assert not np.any(np.isnan(got)), what
    for g, r, s in ((got.real, re, s_re), (got.imag, im, s_im)):
        tol = tol_reduced_dm(n_terms, s)
        err = np.abs(g.astype(LD) - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.max(np.where(err > 0, err / tol.astype(LD), 0))))
        assert np.all(err <= tol), (what, float(np.max(err)), float(np.min(tol)))
    print(f"RATIO reduced_density_dm {what}: {worst:.3e}")


def _engine_call(x_dev, keep, d, start, n_split=0):
    """``engine.reduced_density_dm`` into a buffer that sits inside a larger tensor prefilled with a sentinel; returns
    the result after checking that the surroundings are untouched."""
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    t, d_a = start.shape[0], start.shape[1]
    big = torch.full((t + 2, d_a, d_a), SENTINEL, dtype=torch.complex128, device="cuda")
    out = big[1:t + 1]
    out.copy_(torch.from_numpy(start))
    assert reduced_density_dm(x_dev, keep, d, out=out, n_split=n_split) is out
    host = big.cpu().numpy()
    assert np.all(host[0] == SENTINEL) and np.all(host[-1] == SENTINEL)
    return host[1:t + 1]


def _ctypes_call(x_dev, keep, d, start, n_split=1, scratch_bytes=None):
    """The C entry point itself on a contiguous [T, B, D, D] tensor; returns (status, out)."""
    torch = _torch()
    t, b, dim = (int(v) for v in x_dev.shape[:3])
    d_a = start.shape[1]
    n = int(round(np.log(dim) / np.log(d)))
    out = torch.from_numpy(start.copy()).cuda()
    keep_arr = np.ascontiguousarray(sorted(keep), dtype=np.int32)
    need = t * max(n_split, 1) * d_a * d_a * 16
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") if n_split != 1 else None
    rc = _lib.load().ryd_reduced_density_dm(
        x_dev.data_ptr(), t, b, b * dim * dim, dim * dim, dim, d, n, keep_arr.ctypes.data, len(keep_arr), out.data_ptr(),
        n_split, None if scratch is None else scratch.data_ptr(),
        0 if scratch is None else (need if scratch_bytes is None else scratch_bytes),
        0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes: the smallest at which the index arithmetic, the entry blocking and the padding can go wrong
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [
    (2, 1, [0]), (2, 2, [0]), (2, 2, [1]), (2, 2, [0, 1]),
    (2, 5, [0, 4]), (2, 5, [1, 2, 3]),
    (2, 6, [0, 1, 2, 3, 4, 5]),
    (2, 7, [0, 1, 2, 3, 4, 5]), (2, 7, [1, 2, 3, 4, 5, 6]),
    (2, 8, [0, 2, 3, 5, 6, 7]),
    (2, 10, [4]), (2, 10, [0, 9]),
    (3, 1, [0]), (3, 3, [1]), (3, 4, [0, 3]), (3, 4, [0, 1, 2]), (3, 5, [1, 2, 4]),
    (4, 2, [1]), (4, 3, [0, 2]), (4, 4, [0, 1, 3]),
]


@pytest.mark.parametrize("d,n,keep", SHAPES, ids=[f"d{d}n{n}k{''.join(map(str, k))}" for d, n, k in SHAPES])
def test_kernel_matches_the_reference(d, n, keep):
    torch = _torch()
    rng = np.random.default_rng(1000 * d + 10 * n + sum(keep))
    dim, d_a = d**n, d ** len(keep)
    full = _rand(rng, 3, 3, dim, dim)
    for t in (1, 3):
        for b in (1, 3):
            x = np.ascontiguousarray(full[:t, :b])
            start = _rand(rng, t, d_a, d_a)  # `out` pre-filled with random numbers
            dev = torch.from_numpy(x).cuda()
            ref, s_re, s_im = ref_reduced_dm(x, start, keep, d)
            what = f"d={d} n={n} keep={keep} T={t} B={b}"
            got = _engine_call(dev, keep, d, start, n_split=1)
            _within(got, ref, s_re, s_im, b * (dim // d_a), f"{what} engine")
            rc, got_c = _ctypes_call(dev, keep, d, start, n_split=1)
            assert rc == 0, _lib.load().ryd_last_error()
            assert np.array_equal(got, got_c)  # the same call: bitwise
            assert np.array_equal(dev.cpu().numpy(), x)  # the matrices are only read


def test_an_unsorted_keep_is_sorted_by_the_wrapper():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    x = _rand(np.random.default_rng(5), 1, 1, 32, 32)
    dev = torch.from_numpy(x).cuda()
    a = reduced_density_dm(dev, [3, 0, 2]).cpu().numpy()
    b = reduced_density_dm(dev, (0, 2, 3)).cpu().numpy()
    assert np.array_equal(a, b) and a.shape == (1, 8, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the split of one matrix over workgroups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,keep", [(8, [0, 7]), (10, [3, 4, 5, 6, 7])])
@pytest.mark.parametrize("n_split", [1, 2, 3, 7])
def test_forced_split_is_within_its_bound_and_repeatable(n_split, n, keep):
    """(8 atoms, dA = 4: 16 slots of 4 steps each, which 3 and 7 divide unevenly or leave empty; 10 atoms, dA = 32: four
    entries per thread, 32 steps.)"""
    torch = _torch()
    rng = np.random.default_rng(40 + n_split + n)
    x = _rand(rng, 2, 2, 2**n, 2**n)
    d_a = 2 ** len(keep)
    start = _rand(rng, 2, d_a, d_a)
    dev = torch.from_numpy(x).cuda()
    ref, s_re, s_im = ref_reduced_dm(x, start, keep, 2)
    n_terms = 2 * (2**n // d_a) + n_split
    got = _engine_call(dev, keep, 2, start, n_split=n_split)
    _within(got, ref, s_re, s_im, n_terms, f"n={n} keep={keep} n_split={n_split}")
    again = _engine_call(dev, keep, 2, start, n_split=n_split)
    assert np.array_equal(got, again)  # bitwise on a second call
    rc, got_c = _ctypes_call(dev, keep, 2, start, n_split=n_split)
    assert rc == 0 and np.array_equal(got, got_c)


def test_a_scratch_one_byte_too_small_is_refused():
    torch = _torch()
    x = torch.ones((2, 1, 2**8, 2**8), dtype=torch.complex128, device="cuda")
    start = np.full((2, 4, 4), 5.0 + 0j)
    need = 2 * 2 * 16 * 16
    rc, out = _ctypes_call(x, [0, 7], 2, start, n_split=2, scratch_bytes=need - 1)
    assert rc == -1 and "scratch" in _lib.load().ryd_last_error().decode()
    assert np.array_equal(out, start)  # nothing was launched
    rc, out = _ctypes_call(x, [0, 7], 2, start, n_split=2, scratch_bytes=need)
    assert rc == 0 and np.array_equal(out, start + 64.0)  # 64 ones per entry: exact


def test_library_chosen_split():
    torch = _torch()
    rng = np.random.default_rng(45)
    n, keep = 10, [0, 9]
    x = _rand(rng, 1, 1, 2**n, 2**n)
    start = np.zeros((1, 4, 4), dtype=complex)
    dev = torch.from_numpy(x).cuda()
    ref, s_re, s_im = ref_reduced_dm(x, start, keep, 2)
    got = _engine_call(dev, keep, 2, start, n_split=0)
    from pulser_amd.engine import reduced_density_dm_splits

    _within(got, ref, s_re, s_im, 2**n // 4 + reduced_density_dm_splits(1, 2**n, 4), "n=10 n_split=0")
    assert np.array_equal(got, _engine_call(dev, keep, 2, start, n_split=0))


# ---------------------------------------------------------------------------------------------------------------------
# 3. accumulation and strides
# ---------------------------------------------------------------------------------------------------------------------
def test_two_chunk_calls_against_one_reference_over_both():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    rng = np.random.default_rng(32)
    x = _rand(rng, 2, 2 + 3, 2**6, 2**6)
    keep = [0, 3, 5]
    out = torch.zeros((2, 8, 8), dtype=torch.complex128, device="cuda")
    for part in (x[:, :2], x[:, 2:]):
        reduced_density_dm(torch.from_numpy(np.ascontiguousarray(part)).cuda(), keep, out=out, n_split=1)
    ref, s_re, s_im = ref_reduced_dm(x, np.zeros((2, 8, 8), dtype=complex), keep, 2)
    # the sum of the two calls' bounds: (2 R + 8) + (3 R + 8) = 5 R + 16 units, on scales no larger than S
    _within(out.cpu().numpy(), ref, s_re, s_im, 5 * 8 + 8, "two chunks")


def test_every_third_time_and_a_padded_trajectory_stride_with_nan_in_the_gaps():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    rng = np.random.default_rng(33)
    dim = 2**5
    big = torch.full((10, 5, dim * dim + 24), float("nan"), dtype=torch.complex128, device="cuda")
    view = big[1::3, 1:4, 8:8 + dim * dim].unflatten(2, (dim, dim))  # times 1, 4, 7; a gap after every matrix
    assert tuple(view.shape) == (3, 3, dim, dim) and view.stride(1) == dim * dim + 24
    assert view.stride(0) == 3 * 5 * (dim * dim + 24) and view.data_ptr() != big.data_ptr()
    sub = _rand(rng, 3, 3, dim, dim)
    view.copy_(torch.from_numpy(sub))
    before = big.cpu().numpy()
    assert np.isnan(before).sum() == before.size - sub.size  # everything else is NaN
    for keep, n_split in (([0, 4], 1), ([1, 2], 1), ([2], 3)):
        d_a = 2 ** len(keep)
        got = reduced_density_dm(view, keep, n_split=n_split).cpu().numpy()
        ref, s_re, s_im = ref_reduced_dm(sub, np.zeros((3, d_a, d_a), dtype=complex), keep, 2)
        _within(got, ref, s_re, s_im, 3 * (dim // d_a) + n_split, f"strided view keep={keep}")  # (no NaN: _within)
    assert np.array_equal(big.cpu().numpy(), before, equal_nan=True)  # the states are only read


def test_66000_times_walk_the_grid_stride():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    rng = np.random.default_rng(34)
    x = _rand(rng, 66000, 1, 2, 2)
    got = reduced_density_dm(torch.from_numpy(x).cuda(), [0]).cpu().numpy()
    assert np.array_equal(got, x[:, 0])  # one summand onto zero: the matrices themselves
    start = _rand(rng, 66000, 2, 2)
    out = torch.from_numpy(start).cuda()
    reduced_density_dm(torch.from_numpy(x).cuda(), [0], out=out)
    ref, s_re, s_im = ref_reduced_dm(x, start, [0], 2)
    _within(out.cpu().numpy(), ref, s_re, s_im, 1, "66 000 times")


# ---------------------------------------------------------------------------------------------------------------------
# 4. offsets beyond 32 bits
# ---------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    return int(_torch().cuda.mem_get_info()[0])


def test_two_matrices_more_than_4_gib_apart():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    stride_t = 2**28 + 1000  # complex128 elements: 2^32 bytes and a little
    n_elems = stride_t + 64 * 64
    if _free_bytes() < 2 * 16 * n_elems:
        pytest.skip(f"needs {2 * 16 * n_elems / 2**30:.1f} GiB of free device memory (twice the 4.3-GB allocation)")
    base = torch.empty(n_elems, dtype=torch.complex128, device="cuda")  # uninitialised but for the two matrices
    view = torch.as_strided(base, (2, 1, 64, 64), (stride_t, 64 * 64, 64, 1))
    x = _rand(np.random.default_rng(70), 2, 1, 64, 64)
    view.copy_(torch.from_numpy(x))
    assert view[1].data_ptr() - view[0].data_ptr() > 2**32
    for keep in ([1, 4], [0, 1, 2, 3, 4, 5]):
        d_a = 2 ** len(keep)
        got = reduced_density_dm(view, keep, n_split=1).cpu().numpy()
        ref, s_re, s_im = ref_reduced_dm(x, np.zeros((2, d_a, d_a), dtype=complex), keep, 2)
        _within(got, ref, s_re, s_im, 64 // d_a, f"4 GiB apart keep={keep}")
    del view, base
    torch.cuda.empty_cache()


def test_one_13_atom_matrix():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    n, keep = 13, [0, 12]
    dim = 2**n
    if _free_bytes() < 2 * 16 * dim * dim:
        pytest.skip("needs 2 GiB of free device memory (twice the 1-GiB matrix)")
    gen = torch.Generator(device="cuda").manual_seed(71)
    rho = torch.empty((dim, dim), dtype=torch.complex128, device="cuda")
    torch.view_as_real(rho).normal_(generator=gen)  # filled on the device: no symmetry, both signs
    # the dA * D elements the formula names, fetched with plain indexing
    r = np.arange(dim // 4)
    rows = np.array([(a >> 1) * (dim // 2) + (a & 1) + 2 * r for a in range(4)])  # idx(a, r): site 0 and site 12 from a
    ri = torch.from_numpy(rows).cuda()
    picked = rho[ri[:, None, :], ri[None, :, :]].cpu().numpy()  # [4, 4, R]
    re = picked.real.astype(LD).sum(axis=2)
    im = picked.imag.astype(LD).sum(axis=2)
    s_re = np.abs(picked.real).astype(LD).sum(axis=2)
    s_im = np.abs(picked.imag).astype(LD).sum(axis=2)
    from pulser_amd.engine import reduced_density_dm_splits

    for n_split, extra in ((1, 0), (0, reduced_density_dm_splits(1, dim, 4))):
        got = reduced_density_dm(rho[None, None], keep, n_split=n_split).cpu().numpy()[0]
        _within(got, (re, im), s_re, s_im, dim // 4 + extra, f"13 atoms n_split={n_split}")
    del rho, picked
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 5. exact known answers: bitwise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [[0], [3, 9], [1, 2, 4, 5, 7, 8]])
def test_maximally_mixed_state_of_10_qubits(keep):
    """rho = 1 / D: every summand of a diagonal entry is 2^-10 and there are R = 2^(10 - |keep|) of them - exact in any
    order; every summand of another entry is 0."""
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    dim, d_a = 2**10, 2 ** len(keep)
    rho = torch.zeros((dim, dim), dtype=torch.complex128, device="cuda")
    rho.diagonal().fill_(1.0 / dim)
    for n_split in (1, 0, 5):
        got = reduced_density_dm(rho[None, None], keep, n_split=n_split).cpu().numpy()[0]
        assert np.array_equal(got, np.eye(d_a) / d_a), (keep, n_split)


@pytest.mark.parametrize("keep", [[0], [9], [0, 9], [2, 5, 6], [3, 4, 5, 6, 7, 8]])
def test_ghz_projector_of_10_qubits(keep):
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    dim, d_a = 2**10, 2 ** len(keep)
    rho = torch.zeros((dim, dim), dtype=torch.complex128, device="cuda")
    for i in (0, dim - 1):
        for j in (0, dim - 1):
            rho[i, j] = 0.5
    want = np.zeros((d_a, d_a), dtype=complex)
    want[0, 0] = want[-1, -1] = 0.5  # (the coherences sit where the free digits of row and column differ)
    for n_split in (1, 0):
        got = reduced_density_dm(rho[None, None], keep, n_split=n_split).cpu().numpy()[0]
        assert np.array_equal(got, want), (keep, n_split)


@pytest.mark.parametrize("i,j", [(0, 0), (5, 5), (5, 36), (36, 5), (37, 36), (63, 0), (21, 53), (53, 21), (6, 7)])
def test_a_single_element_lands_in_the_entry_the_formula_names(i, j):
    """Six qubits, keep = [0, 3, 5] (digits 32, 4 and 1 of the index; free: 16, 8, 2).  rho[i][j] belongs to entry
    (a(i), a(j)) when the free digits of i and j agree, and to none otherwise."""
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    keep, free_mask = [0, 3, 5], 16 + 8 + 2
    value = complex(-1.25, 0.375)
    rho = torch.zeros((64, 64), dtype=torch.complex128, device="cuda")
    rho[i, j] = value

    def row(x):
        return ((x >> 5) & 1) * 4 + ((x >> 2) & 1) * 2 + (x & 1)

    want = np.zeros((8, 8), dtype=complex)
    if (i & free_mask) == (j & free_mask):
        want[row(i), row(j)] = value
    for n_split in (1, 2):
        got = reduced_density_dm(rho[None, None], keep, n_split=n_split).cpu().numpy()[0]
        assert np.array_equal(got, want), (i, j, n_split)


# ---------------------------------------------------------------------------------------------------------------------
# 6. nothing to do, and what is refused
# ---------------------------------------------------------------------------------------------------------------------
def test_no_times_launches_nothing_and_invalid_arguments_are_refused():
    from pulser_amd.engine import reduced_density_dm

    torch = _torch()
    lib = _lib.load()
    x = torch.ones((2, 3, 8, 8), dtype=torch.complex128, device="cuda")
    o = torch.full((2, 2, 2), 5.0, dtype=torch.complex128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    px, po = x.data_ptr(), o.data_ptr()
    keep = np.array([1], dtype=np.int32)
    bad = np.array([2, 1], dtype=np.int32)
    pk = keep.ctypes.data
    tail = (1, None, 0, 0, stream)
    assert lib.ryd_reduced_density_dm(px, 0, 3, 192, 64, 8, 2, 3, pk, 1, po, *tail) == 0
    assert tuple(reduced_density_dm(x[:0], [1]).shape) == (0, 2, 2)
    for args in ((None, 2, 3, 192, 64, 8, 2, 3, pk, 1, po), (px, 2, 3, 192, 64, 8, 2, 3, pk, 1, None),
                 (px, 2, 3, 192, 64, 8, 2, 3, None, 1, po), (px, 2, 0, 192, 64, 8, 2, 3, pk, 1, po),
                 (px, -1, 3, 192, 64, 8, 2, 3, pk, 1, po), (px, 2, 3, 192, 64, 8, 2, 4, pk, 1, po),
                 (px, 2, 3, 192, 63, 8, 2, 3, pk, 1, po), (px, 2, 3, 63, 64, 8, 2, 3, pk, 1, po),
                 (px, 2, 3, 192, 8, 8, 2, 3, pk, 1, po), (px, 2, 3, 8, 64, 8, 2, 3, pk, 1, po),
                 (px, 2, 3, 192, 64, 8, 2, 3, bad.ctypes.data, 2, po), (px, 2, 3, 192, 64, 8, 2, 3, pk, 0, po),
                 (px, 2, 3, 192, 64, 8, 5, 3, pk, 1, po)):
        assert lib.ryd_reduced_density_dm(*args, *tail) == -1, args
        assert "reduced_density_dm" in lib.ryd_last_error().decode()
    assert lib.ryd_reduced_density_dm(px, 2, 3, 192, 64, 8, 2, 3, pk, 1, po, 2, None, 0, 0, stream) == -1  # no scratch
    torch.cuda.synchronize()
    assert torch.all(o == 5.0)  # nothing was launched
    # the wrapper's own checks
    with pytest.raises(TypeError):
        reduced_density_dm(x.to(torch.complex64), [1])
    with pytest.raises(ValueError):
        reduced_density_dm(x.cpu(), [1])
    with pytest.raises(ValueError):
        reduced_density_dm(x.reshape(2, 3, 64), [1])
    with pytest.raises(ValueError):
        reduced_density_dm(x, [])
    with pytest.raises(ValueError):
        reduced_density_dm(x, [1, 1])
    with pytest.raises(ValueError):
        reduced_density_dm(x, [3])
    with pytest.raises(ValueError):
        reduced_density_dm(x, [0], local_dim=3)  # 8 is no power of 3
    with pytest.raises(ValueError):
        reduced_density_dm(x, [1], out=o[:, :1])
    with pytest.raises(TypeError):
        reduced_density_dm(x, [1], out=o.to(torch.complex64))
    with pytest.raises(ValueError):
        reduced_density_dm(x[:, :1].expand(2, 3, 8, 8), [1])  # stride_b = 0
    with pytest.raises(ValueError):
        reduced_density_dm(x.transpose(2, 3), [1])  # the matrix axes are not contiguous
    with pytest.raises(ValueError, match="64"):
        reduced_density_dm(torch.ones((1, 1, 2**7, 2**7), dtype=torch.complex128, device="cuda"), range(7))
    torch.cuda.synchronize()
    assert torch.all(o == 5.0)

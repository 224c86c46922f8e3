"""GPU: ``ryd_general_observe_density_many`` (k_gen_obs_pairs on the diagonals, k_gen_coefs_fused_many,
k_gen_obs_energy_dm_many) - the occupations, correlations and energy moments of the density matrices of every evaluation
time of a multi-level or XY master-equation run in one call - called through ``GeneralEngine.observe_density_many`` and
pinned to the longdouble host references ``observe_ref.ref_energy_dm`` and ``general_observe_ref.ref_pairs_d``.

Matrices are random, complex and NOT Hermitian (a Hermitian rho or a real H would hide a row / column mix-up), different
per (time, entry) and scaled by entry; every problem's drive carries a non-zero phase, asserted on H at the interior knot.

Tolerances are ``observe_ref.tol_sum`` and ``general_observe_ref.tol_energy_dm_general``, imported and unchanged.  That
derivation was written for the per-time path (H applied to all columns, then the diagonal summed) and carries over: the
kernel here adds the same m1 = nnz(H) products H_ab rho_ba and the same m2 triples H_ab H_bc rho_ca, grouped by row r of
the trace (so the (m + D + 8) u S_abs summation bound holds for it as for any order of those terms), and the 1e-11 terms
bound what one row evaluation of G on a column of rho may deviate by - the device's evaluation of the coefficients of
H(t) included - which is the same row evaluation (``gen_fused_row``) here, used once for (G rho)_rr and nested for
(G G rho)_rr exactly as W2 = H (W + dW) + e in the derivation.  Nothing is fitted to what the kernel gives; every case
prints ``RATIO kernel what err tol ratio`` before it asserts.

The kernel has no size-dependent path (the matrix never enters LDS; only the tables do), so no extra shape is added.
Worst ratios seen on an MI355X:

    k_gen_obs_pairs (diagonals)   0.099     (the trace of a 2-atom XY matrix; occupation / correlation 0.067)
    k_gen_obs_energy_dm_many      9.6e-06   (Tr(H rho); Tr(H^2 rho) 4.0e-06; the trace of an energy-only request 0.074)
    against observe(density=True) pair sums identical; Tr(H rho) 1.2e-05, Tr(H^2 rho) 2.2e-06 of both bounds
    5 times per chunk             identical to one chunk
"""
import itertools

import numpy as np
import pytest

from helpers import local_problem
from general_observe_ref import ref_pairs_d, tol_energy_dm_general
from observe_ref import ref_energy_dm, tol_sum
from test_gpu_general_observe import _engine, _problem

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.6, 1.9)
INVALID, UNSUPPORTED = -1, -3  # RYD_ERR_* of include/rydemu.h
KNOT, T_END = 0.06, 0.12       # the "_me" and "leak" problems have 121 samples: 1-ns knots up to 0.12 us

# (kind, atoms): D = 4, 256 (pair sites, 4 row blocks), 1024 (16 row blocks, 2 workgroups in x), 9 and 27 (partial row
# block), 243, 729 (12 row blocks, the last workgroup short), 64 (exactly one block), 256
CASES = [("xy_me", 2), ("xy_me", 8), ("xy_me", 10), ("l3_me", 2), ("l3_me", 3), ("l3_me", 5), ("l3_me", 6),
         ("leak", 3), ("leak", 4)]


def _times(T):
    """Unsorted, one repeated, one on a knot, one on the last knot; from T = 5 on also off the knots."""
    return {3: [KNOT, T_END, KNOT],
            5: [0.0444, T_END, KNOT, 0.0444, 0.1013],
            12: [0.0444, T_END, KNOT, 0.0444, 0.1013, 0.0, 0.0137, 0.09, 0.0781, 0.0302, T_END, 0.0555]}[T]


def _report(kernel, what, err, tol):
    err, tol = np.asarray(err, dtype=float), np.asarray(tol, dtype=float)
    ok = bool(np.all(err <= tol))
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0, tol, np.finfo(float).tiny))))
    print(f"RATIO {kernel:24s} {what:48s} err {float(np.max(err)):.3e} tol {float(np.max(tol)):.3e} ratio {ratio:.3e}")
    return ok


def _matrices(D, T, B, seed):
    """[T, B, D, D]: a different random complex non-Hermitian matrix for every (time, entry), scaled by entry."""
    rng = np.random.default_rng(8800 + seed)
    m = (rng.normal(size=(T, B, D, D)) + 1j * rng.normal(size=(T, B, D, D))) / np.sqrt(D)
    m += 0.4 * np.eye(D)  # (a trace that is not a sum of noise alone)
    for b in range(B):
        m[:, b] *= SCALES[b % 3]
    return m


def _dev(eng, host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).to(eng.device)


_REFS = {}


def _refs(kind, n, T, B=2):
    """(matrices [T, B, D, D], times, pair references by (i, b, one) for one in (0, d - 1), (e1, e2, tol1, tol2) by
    (i, b)): computed once per shape, shared by the tests that use it and never changed."""
    key = (kind, n, T, B)
    if key not in _REFS:
        _, ham, d, _ = _problem(kind, n)
        D = d**n
        assert np.max(np.abs(ham.matrix(KNOT).toarray().imag)) > 1e-2  # H is not real
        ms, times = _matrices(D, T, B, 10 * n + d), _times(T)
        assert np.max(np.abs(ms[0, 0] - ms[0, 0].conj().T)) > 0.1  # rho is not Hermitian
        pairs = {(i, b, one): ref_pairs_d(np.real(np.diag(ms[i, b])), n, d, one)
                 for i in range(T) for b in range(B) for one in (0, d - 1)}
        energy = {}
        for i, b in itertools.product(range(T), range(B)):
            e1, e2, s_abs = ref_energy_dm(ham, times[i], ms[i, b])
            energy[(i, b)] = (e1, e2) + tuple(tol_energy_dm_general(ham, times[i], ms[i, b], s_abs))
        _REFS[key] = (ms, times, pairs, energy)
    return _REFS[key]


def _check(got, D, pair_ref, e_ref, tag, r, c, occupation=True, correlation=True, energy=True):
    """Every output at [r, c] of ``got``: what was asked for against the longdouble reference, the rest exactly 0."""
    norm, occ, corr, (s_norm, s_occ, s_corr) = pair_ref
    pairs = occupation or correlation or not energy
    ok = _report("k_gen_obs_pairs" if pairs else "k_gen_obs_energy_dm_many", f"{tag} trace",
                 abs(got["norm2"][r, c] - norm), tol_sum(D, s_norm))
    if occupation:
        ok &= _report("k_gen_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][r, c] - occ), tol_sum(D, s_occ))
    else:
        ok &= bool(np.all(got["occupation"][r, c] == 0.0))
    if correlation:
        ok &= _report("k_gen_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][r, c] - corr), tol_sum(D, s_corr))
    else:
        ok &= bool(np.all(got["correlation"][r, c] == 0.0))
    if energy:
        e1, e2, tol1, tol2 = e_ref
        ok &= _report("k_gen_obs_energy_dm_many", f"{tag} Tr(H rho)", abs(got["energy"][r, c] - e1), tol1)
        ok &= _report("k_gen_obs_energy_dm_many", f"{tag} Tr(H^2 rho)", abs(got["energy2"][r, c] - e2), tol2)
    else:
        ok &= bool(got["energy"][r, c] == 0.0 and got["energy2"][r, c] == 0.0)
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# 1. every shape: one-state digits 0 and d - 1, four requests, launch counts, agreement with the per-time call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", CASES)
def test_observe_density_many_against_the_references(kind, n):
    prob, _, d, _ = _problem(kind, n)
    D, T, B = d**n, 3, 2
    ms, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    with _engine(prob) as eng:
        assert eng.dim == D and eng.local_dim == d and eng.n == n and eng.batch == 1
        assert eng.apply_path() in ("fused", "fused_lds")
        dev = _dev(eng, ms)
        for one in (0, d - 1):
            for occ, cor, en in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
                eng.reset_stats()
                got = eng.observe_density_many(dev, times, one=one, occupation=occ, correlation=cor, energy=en)
                stats = eng.stats()
                assert stats["n_launches"] == (1 if occ or cor else 0) + (2 if en else 0), stats
                assert stats["n_applications"] == 0
                assert got["norm2"].shape == (T, B) and got["occupation"].shape == (T, B, n)
                assert got["correlation"].shape == (T, B, n, n) and got["energy"].shape == got["energy2"].shape == (T, B)
                for i, b in itertools.product(range(T), range(B)):
                    ok &= _check(got, D, pair_ref[(i, b, one)], e_ref[(i, b)],
                                 f"{kind}{n} i={i} b={b} one={one} [{int(occ)}{int(cor)}{int(en)}]", i, b, occ, cor, en)
        # the per-time path on the same matrices: within the sum of the two calls' bounds
        one = d - 1
        for i, b in itertools.product(range(T), range(B)):
            single = eng.observe(dev[i, b:b + 1], float(times[i]), one=one, density=True)
            _, _, _, (s_norm, s_occ, s_corr) = pair_ref[(i, b, one)]
            _, _, tol1, tol2 = e_ref[(i, b)]
            tag = f"{kind}{n} i={i} b={b} vs observe(density=True)"
            ok &= _report("both paths", f"{tag} trace", abs(got["norm2"][i, b] - single["norm2"][0]), 2 * tol_sum(D, s_norm))
            ok &= _report("both paths", f"{tag} occupation", np.abs(got["occupation"][i, b] - single["occupation"][0]), 2 * tol_sum(D, s_occ))
            ok &= _report("both paths", f"{tag} correlation", np.abs(got["correlation"][i, b] - single["correlation"][0]), 2 * tol_sum(D, s_corr))
            ok &= _report("both paths", f"{tag} Tr(H rho)", abs(got["energy"][i, b] - single["energy"][0]), 2 * tol1)
            ok &= _report("both paths", f"{tag} Tr(H^2 rho)", abs(got["energy2"][i, b] - single["energy2"][0]), 2 * tol2)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 2. strides
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("l3_me", 3), ("xy_me", 8)])
def test_views_are_observed_in_place(kind, n):
    """``dev[:, 1:2]`` of a [T, 2, D, D] tensor, every second time of a [2 T, 1, D, D] tensor, and both strides padded
    beyond D * D go through with their strides; last axes that are not contiguous are refused."""
    import torch

    prob, _, d, _ = _problem(kind, n)
    D, T = d**n, 5
    ms, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    with _engine(prob) as eng:
        dev = _dev(eng, ms)
        view = dev[:, 1:2]
        assert view.data_ptr() == dev.data_ptr() + 16 * D * D and not view.is_contiguous()
        got = eng.observe_density_many(view, times, one=d - 1)
        for i in range(T):
            ok &= _check(got, D, pair_ref[(i, 1, d - 1)], e_ref[(i, 1)], f"{kind}{n} column 1 i={i}", i, 0)
        wide = torch.zeros((2 * T, 1, D, D), dtype=torch.complex128, device=eng.device)
        wide[::2] = dev[:, 0:1]
        wide[1::2] = 7.0  # (what a dropped stride would read)
        got = eng.observe_density_many(wide[::2], times, one=0)
        for i in range(T):
            ok &= _check(got, D, pair_ref[(i, 0, 0)], e_ref[(i, 0)], f"{kind}{n} every second i={i}", i, 0)
        pad = torch.full((T, 2, D * D + 24), 7.0, dtype=torch.complex128, device=eng.device)
        pad[:, :, :D * D] = dev.reshape(T, 2, D * D)
        padded = pad[:, :, :D * D].unflatten(2, (D, D))
        assert padded.stride(0) == 2 * (D * D + 24) and padded.stride(1) == D * D + 24 and padded.stride(2) == D
        got = eng.observe_density_many(padded, times, one=0)
        for i, b in itertools.product(range(T), range(2)):
            ok &= _check(got, D, pair_ref[(i, b, 0)], e_ref[(i, b)], f"{kind}{n} padded strides i={i} b={b}", i, b)
        with pytest.raises(ValueError, match="two axes"):
            eng.observe_density_many(torch.zeros((T, 1, D, 2 * D), dtype=torch.complex128, device=eng.device)[..., ::2], times)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 3. more states than the second grid axis holds
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_stride_over_states():
    """70 000 matrices of a 2-atom XY register (17.9 MB, the 3 x 2 pattern tiled): the kernels stride over the states
    beyond the 65 535 workgroups of the second grid axis.  The last rows against the reference; every row equals its
    pattern row within twice the bound (two evaluations of one matrix)."""
    kind, n, T3, T, B = "xy_me", 2, 3, 35000, 2
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    ms, times, pair_ref, e_ref = _refs(kind, n, T3)
    reps = -(-T // T3)
    big = np.tile(ms, (reps, 1, 1, 1))[:T]
    tt = np.tile(np.asarray(times), reps)[:T]
    with _engine(prob) as eng:
        eng.reset_stats()
        got = eng.observe_density_many(_dev(eng, big), tt, one=1)
        stats = eng.stats()
    assert stats["n_launches"] == 3 and stats["n_applications"] == 0, stats
    ok = True
    for r, b in itertools.product(range(T - 6, T), range(B)):
        i = r % T3
        ok &= _check(got, D, pair_ref[(i, b, 1)], e_ref[(i, b)], f"{kind}{n} row {r} b={b}", r, b)
    rows = np.arange(T) % T3
    for i, b in itertools.product(range(T3), range(B)):
        _, _, _, (s_norm, s_occ, s_corr) = pair_ref[(i, b, 1)]
        _, _, tol1, tol2 = e_ref[(i, b)]
        sel = rows == i
        tag = f"rows = {i} mod 3, b={b}:"
        ok &= _report("k_gen_obs_pairs", f"{tag} trace", np.abs(got["norm2"][sel, b] - got["norm2"][i, b]), 2 * tol_sum(D, s_norm))
        ok &= _report("k_gen_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][sel, b] - got["occupation"][i, b]), 2 * tol_sum(D, s_occ))
        ok &= _report("k_gen_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][sel, b] - got["correlation"][i, b]), 2 * tol_sum(D, s_corr))
        ok &= _report("k_gen_obs_energy_dm_many", f"{tag} Tr(H rho)", np.abs(got["energy"][sel, b] - got["energy"][i, b]), 2 * tol1)
        ok &= _report("k_gen_obs_energy_dm_many", f"{tag} Tr(H^2 rho)", np.abs(got["energy2"][sel, b] - got["energy2"][i, b]), 2 * tol2)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 4. time chunks
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_in_chunks_of_five_times():
    """The chunked path (tables of all times beyond the scratch cap) on D = 27: with the 5-per-chunk hook 12 times take
    three chunks - one pair launch and two launches per chunk - and give what one chunk gives within twice the bound."""
    kind, n, T, B = "l3_me", 3, 12, 2
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    ms, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    with _engine(prob) as eng:
        dev = _dev(eng, ms)
        eng.reset_stats()
        whole = eng.observe_density_many(dev, times, one=2)
        assert eng.stats()["n_launches"] == 3
        eng.set_path(False, observe_small_chunks=True)
        eng.reset_stats()
        got = eng.observe_density_many(dev, times, one=2)
        assert eng.stats()["n_launches"] == 1 + 2 * 3 and eng.stats()["n_applications"] == 0, eng.stats()
        eng.reset_stats()
        energy_only = eng.observe_density_many(dev, times, one=2, occupation=False, correlation=False)
        assert eng.stats()["n_launches"] == 2 * 3, eng.stats()
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check(got, D, pair_ref[(i, b, 2)], e_ref[(i, b)], f"{kind}{n} chunks i={i} b={b}", i, b)
        ok &= _check(energy_only, D, pair_ref[(i, b, 2)], e_ref[(i, b)], f"{kind}{n} chunks, energy only i={i} b={b}", i, b,
                     occupation=False, correlation=False)
        _, _, tol1, tol2 = e_ref[(i, b)]
        ok &= _report("chunked vs whole", f"i={i} b={b} Tr(H rho)", abs(got["energy"][i, b] - whole["energy"][i, b]), 2 * tol1)
        ok &= _report("chunked vs whole", f"i={i} b={b} Tr(H^2 rho)", abs(got["energy2"][i, b] - whole["energy2"][i, b]), 2 * tol2)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 5. the handle is left as it was
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi_launch", [False, True])
def test_handle_state_is_untouched(multi_launch):
    """A 20-ns ``solve``, a ket ``observe`` and a per-time density ``observe`` after an ``observe_density_many`` call at
    other times are bitwise those of a fresh engine (the handle's coefficients, site matrices, work vector and column
    scratch are not the call's).  D = 27: one wave carries every sum of the per-time kernels, so their order is fixed."""
    from helpers import rand_state

    kind, n, T = "l3_me", 3, 12
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    ms, times, _, _ = _refs(kind, n, T)
    t = 0.0731
    init = rand_state(D, 4242)
    init /= np.linalg.norm(init)
    x = rand_state(D, 77)[None]

    def after(eng):
        solved = eng.solve(eng.new_state(init), [0.0, 0.02]).cpu().numpy()
        ket = eng.observe(_dev(eng, x), t, one=1)
        dm = eng.observe(_dev(eng, ms[2, :1]), t, one=1, density=True)
        return solved, ket, dm

    with _engine(prob) as eng:
        if multi_launch:
            eng.set_path(True)
        fresh = after(eng)
    with _engine(prob) as eng:
        if multi_launch:
            eng.set_path(True)
        eng.observe_density_many(_dev(eng, ms), times, one=0)
        used = after(eng)
    assert np.array_equal(fresh[0], used[0])
    for a, b in zip(fresh[1:], used[1:]):
        for k in ("norm2", "occupation", "correlation", "energy", "energy2"):
            assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raw(eng, states, n_t, n_b, stride_t, stride_b, times, what, d, n, one, out, h="own"):
    tt = np.ascontiguousarray(times, dtype=np.float64)
    rc = eng.lib.ryd_general_observe_density_many(eng._h if h == "own" else h, states if isinstance(states, int) else states.data_ptr(),
                                                  n_t, n_b, stride_t, stride_b, tt.ctypes.data if times is not None else None,
                                                  what, d, n, one, out if isinstance(out, int) or out is None else out.data_ptr(),
                                                  eng._stream())
    return rc, eng.lib.ryd_last_error().decode()


def test_refusals():
    import torch
    from pulser_amd._lib import RydError
    from pulser_amd.engine import Engine

    kind, n, T, B = "l3_me", 3, 3, 2
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    DD = D * D
    ms, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    # a RYD_GENERAL_DENSITY handle
    with _engine(_problem("xy_me", 2)[0], mesolve=True) as eng:
        rho = torch.zeros((T, 1, 4, 4), dtype=torch.complex128, device=eng.device)
        with pytest.raises(ValueError, match="ket engines"):
            eng.observe_density_many(rho, times, energy=False)
        out = torch.zeros((T, 1, 9), dtype=torch.float64, device=eng.device)
        rc, msg = _raw(eng, rho, T, 1, 16, 16, times, 3, 2, 2, 0, out)
        assert rc == UNSUPPORTED and "ryd_general_observe" in msg, (rc, msg)
    # collapse operators: no energy moments, the pair sums are served
    with _engine(prob) as eng:
        jump = np.zeros((d, d), complex)
        jump[1, 0] = 0.3
        eng.set_collapse([jump])
        dev = _dev(eng, ms)
        with pytest.raises(RydError, match="collapse operators") as exc:
            eng.observe_density_many(dev, times, one=2)
        assert exc.value.code == UNSUPPORTED and "pair sums" in str(exc.value)
        got = eng.observe_density_many(dev, times, one=2, energy=False)
        for i, b in itertools.product(range(T), range(B)):
            ok &= _check(got, D, pair_ref[(i, b, 2)], None, f"collapse handle i={i} b={b}", i, b, energy=False)
    with _engine(prob) as eng:
        # no padded site tables: no energy moments, the pair sums are served
        eng.set_path(False, no_fused=True)
        dev = _dev(eng, ms)
        with pytest.raises(RydError, match="padded site tables") as exc:
            eng.observe_density_many(dev, times, one=2)
        assert exc.value.code == UNSUPPORTED
        got = eng.observe_density_many(dev, times, one=2, energy=False)
        for i, b in itertools.product(range(T), range(B)):
            ok &= _check(got, D, pair_ref[(i, b, 2)], None, f"no_fused handle i={i} b={b}", i, b, energy=False)
        with pytest.raises(ValueError, match="digit"):
            eng.observe_density_many(dev, times, one=d)
        eng.set_path(False)
        # a set RYD_OBS_DENSITY bit is ignored
        out = torch.full((T, B, n * n + n + 3), 7.0, dtype=torch.float64, device=eng.device)
        want = eng.observe_density_many(dev, times, one=0, correlation=False, energy=False)
        rc, msg = _raw(eng, dev, T, B, B * DD, DD, times, 1 | 8, d, n, 0, out)
        assert rc == 0, (rc, msg)
        assert np.array_equal(out.cpu().numpy()[..., :n], want["occupation"])
        out.fill_(7.0)
        # ranges, the dimension, strides, counts, null pointers
        for dd, nn, one in ((5, n, 0), (1, n, 0), (d, 0, 0), (d, 27, 0), (d, n, d), (d, n, -1)):
            rc, msg = _raw(eng, dev, T, B, B * DD, DD, times, 3, dd, nn, one, out)
            assert rc == INVALID and "out of range" in msg, (rc, msg)
        rc, msg = _raw(eng, dev, T, B, B * DD, DD, times, 3, d, n - 1, 0, out)
        assert rc == INVALID and "is not 3^2" in msg, (rc, msg)
        rc, msg = _raw(eng, dev, T, B, B * DD, DD, times, 3, d, 9, 0, out)  # 3^9 > 2^13
        assert rc == INVALID and "2^26 entries" in msg, (rc, msg)
        for st_t, st_b in ((DD - 1, DD), (B * DD, DD - 1)):
            rc, msg = _raw(eng, dev, T, B, st_t, st_b, times, 3, d, n, 0, out)
            assert rc == INVALID and "smaller than a density matrix" in msg, (rc, msg)
        for n_t, n_b in ((T, 0), (-1, B)):
            rc, msg = _raw(eng, dev, n_t, n_b, B * DD, DD, times, 3, d, n, 0, out)
            assert rc == INVALID and "general observe_density_many" in msg, (rc, msg)
        for states, tt, o in ((0, times, out), (dev, None, out), (dev, times, None)):
            rc, msg = _raw(eng, states, T, B, B * DD, DD, tt, 3, d, n, 0, o)
            assert rc == INVALID and "null argument" in msg, (rc, msg)
        rc, msg = _raw(eng, dev, T, B, B * DD, DD, times, 3, d, n, 0, out, h=None)
        assert rc == INVALID and "general observe_density_many" in msg and "null handle" in msg, (rc, msg)
        # no times at all: nothing is zeroed, nothing is written (null pointers are fine then)
        rc, msg = _raw(eng, 0, 0, B, B * DD, DD, None, 7, d, n, 0, out)
        assert rc == 0, (rc, msg)
        torch.cuda.synchronize()
        assert bool(torch.all(out == 7.0))
    # a two-level handle
    with Engine.from_problems([local_problem(2, seed=5)], mode="sesolve") as two:
        x2 = torch.zeros((T, 1, 4, 4), dtype=torch.complex128, device=two.device)
        out = torch.zeros((T, 1, 9), dtype=torch.float64, device=two.device)
        rc, msg = _raw(two, x2, T, 1, 16, 16, times, 3, 2, 2, 0, out)
        assert rc == INVALID and "ryd_observe_density_many" in msg, (rc, msg)
    assert ok

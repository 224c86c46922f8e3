"""GPU: ``ryd_general_observe_many`` (k_gen_obs_pairs with many-state addressing, k_gen_coefs_fused_many,
k_gen_obs_energy_many) - the occupations, correlations and energy moments of the kets of every evaluation time of a
multi-level or XY run in one call - called directly through ``GeneralEngine.observe_many`` and pinned to the longdouble
host references of tests/observe_ref.py and tests/general_observe_ref.py, and its use by ``QutipBackendV2``.

States are random, unnormalised and different per batch entry (scales 1.0 / 0.6 / 1.9); drives are complex.  Shapes are
the smallest at which each path of the energy kernel can go wrong: less than one wave (XY on 2 atoms), less than one
64-row block (XY on 4), one full and one partial row block with d = 3 digit words (3 levels on 4), the ket staged in LDS
(3 levels on 6, 4 levels on 5, XY on 12: 66 exchange pairs, 64 KiB), and the ket gathered from L2 (3 levels on 9, XY on
14).  Times: 0, interior, exactly a knot, the last knot, repeated, unsorted.

Tolerances are the derived ones of tests/observe_ref.py (``tol_sum``: worst-case summation bound; ``tol_energy_ket``:
that plus the project's 1e-11 bar of one generator application, which the fused w = -i H x is held to as well); nothing
is fitted.  The backend cases compare the one-call path with the per-time path within the sum of the two paths' bounds,
written for a normalised state without reading it (``_backend_bounds``).  Every case prints ``RATIO kernel what err
tol ratio`` before it asserts.  Worst ratios seen on an MI355X:

    k_gen_obs_pairs          0.13      (the 4-term norm of a 2-atom XY ket; occupation / correlation 0.11 on 4 atoms)
    k_gen_obs_energy_many    1.0e-05   (<H^2>; <H> 9.6e-06; the norm of an energy-only request 0.14 on 2 atoms)
    300 times, 3^6           pair sums identical to per-time ``GeneralEngine.observe``; <H> 1.7e-06, <H^2> 3.4e-06 of both bounds
    backend, both paths      occupation 0.0072, other pair sums 0.068, <H> 1.1e-05, <H^2> 6.0e-06
"""
import itertools

import numpy as np
import pytest

from helpers import load_fixture, local_problem, rand_state
from general_observe_ref import ref_pairs_d
from observe_ref import U53, ket_probabilities, ref_energy_ket, tol_energy_ket, tol_sum
from test_gpu_general_observe import _engine, _problem

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.6, 1.9)
INVALID, UNSUPPORTED = -1, -3  # RYD_ERR_* of include/rydemu.h

# (kind, atoms, kernel of the application: the vector staged in LDS, or gathered from L2)
CASES = [("xy", 2, "fused_lds"), ("xy", 4, "fused_lds"), ("l3", 4, "fused_lds"), ("l3", 6, "fused_lds"),
         ("leak", 5, "fused_lds"), ("xy", 12, "fused_lds"), ("l3", 9, "fused"), ("xy", 14, "fused")]


def _times(t_end, T):
    """The patterns of ``TIMES`` of tests/test_gpu_observe_many.py on a sequence that ends at ``t_end`` (1-ns knots)."""
    inner, knot = round(0.37 * t_end, 3) + 0.0004, round(0.5 * t_end, 3)
    return {1: [inner], 2: [knot, 0.0],
            7: [t_end, 0.0, inner, knot, inner, round(0.75 * t_end, 3) + 0.0002, round(0.12 * t_end, 3) + 0.0003]}[T]


def _report(kernel, what, err, tol):
    err, tol = np.asarray(err, dtype=float), np.asarray(tol, dtype=float)
    ok = bool(np.all(err <= tol))
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0, tol, np.finfo(float).tiny))))
    print(f"RATIO {kernel:22s} {what:44s} err {float(np.max(err)):.3e} tol {float(np.max(tol)):.3e} ratio {ratio:.3e}")
    return ok


def _kets(D, T, B, seed):
    """[T, B, D]: a different random ket for every (time, entry), scaled by entry."""
    return np.stack([np.stack([SCALES[(i + b) % 3] * rand_state(D, 5000 + 97 * seed + 10 * i + b) for b in range(B)])
                     for i in range(T)])


def _dev(eng, host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).to(eng.device)


_REFS = {}


def _refs(kind, n, T, B=3):
    """(kets [T, B, D], times, pair references by (i, b, one), energy references by (i, b)): computed once per shape and
    shared by the tests that use it; B = 1 cases take entry 0."""
    key = (kind, n, T)
    if key not in _REFS:
        _, ham, d, t_end = _problem(kind, n)
        D = d**n
        xs, times = _kets(D, T, B, n), _times(t_end, T)
        pairs = {(i, b, one): ref_pairs_d(ket_probabilities(xs[i, b]), n, d, one)
                 for i in range(T) for b in range(B) for one in range(d)}
        energy = {(i, b): ref_energy_ket(ham, times[i], xs[i, b]) for i in range(T) for b in range(B)}
        _REFS[key] = (xs, times, pairs, energy)
    return _REFS[key]


def _check(got, i, b, x, pair_ref, e_ref, tag, occupation=True, correlation=True, energy=True, row=None, col=None):
    """Every output of state (i, b) - at [row, col] of ``got`` when that is not [i, b]: what was asked for against the
    longdouble reference, the rest exactly 0."""
    D = len(x)
    r = i if row is None else row
    b = b if col is None else col
    norm, occ, corr, (s_norm, s_occ, s_corr) = pair_ref
    ok = _report("k_gen_obs_pairs" if occupation or correlation or not energy else "k_gen_obs_energy_many",
                 f"{tag} norm2", abs(got["norm2"][r, b] - norm), tol_sum(D, s_norm))
    if occupation:
        ok &= _report("k_gen_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][r, b] - occ), tol_sum(D, s_occ))
    else:
        ok &= bool(np.all(got["occupation"][r, b] == 0.0))
    if correlation:
        ok &= _report("k_gen_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][r, b] - corr), tol_sum(D, s_corr))
    else:
        ok &= bool(np.all(got["correlation"][r, b] == 0.0))
    if energy:
        e1, e2, s_abs, w = e_ref
        tol1, tol2 = tol_energy_ket(x, w, s_abs)
        ok &= _report("k_gen_obs_energy_many", f"{tag} <H>", abs(got["energy"][r, b] - e1), tol1)
        ok &= _report("k_gen_obs_energy_many", f"{tag} <H^2>", abs(got["energy2"][r, b] - e2), tol2)
    else:
        ok &= got["energy"][r, b] == 0.0 and got["energy2"][r, b] == 0.0
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# 1. direct: every shape x times x batch x digit, every subset of the request
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("kind,n,kernel", CASES)
def test_observe_many_against_the_references(kind, n, kernel, T):
    """B = 1 and B = 3 on a handle of batch 1 (its one problem serves every entry), every ``one`` digit with everything
    asked for, then every other subset of occupation / correlation / energy for the last digit: slots not asked for are
    exactly 0 and ``norm2`` is right even for an energy-only request.  With B = 3 ``observe_many`` is the first call
    on a fresh handle."""
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    xs, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    for B in (1, 3):
        with _engine(prob) as eng:
            assert eng.dim == D and eng.local_dim == d and eng.n == n and eng.batch == 1
            if B == 1:  # (LDS or L2: what the case is named for - asked before any call here, after the calls below)
                assert eng.apply_path() == kernel
            dev = _dev(eng, xs[:, :B])
            for one in range(d):
                got = eng.observe_many(dev, times, one=one)
                assert got["norm2"].shape == (T, B) and got["occupation"].shape == (T, B, n)
                assert got["correlation"].shape == (T, B, n, n) and got["energy"].shape == got["energy2"].shape == (T, B)
                for i, b in itertools.product(range(T), range(B)):
                    ok &= _check(got, i, b, xs[i, b], pair_ref[(i, b, one)], e_ref[(i, b)],
                                 f"{kind}{n} T={T} B={B} i={i} b={b} one={one}")
            one = d - 1
            for occ, cor, en in itertools.product((False, True), repeat=3):
                if occ and cor and en:
                    continue
                eng.reset_stats()
                got = eng.observe_many(dev, times, one=one, occupation=occ, correlation=cor, energy=en)
                stats = eng.stats()
                assert stats["n_launches"] == (1 if occ or cor or not en else 0) + (2 if en else 0), stats
                assert stats["n_applications"] == 0
                for i, b in itertools.product(range(T), range(B)):
                    ok &= _check(got, i, b, xs[i, b], pair_ref[(i, b, one)], e_ref[(i, b)],
                                 f"{kind}{n} T={T} B={B} i={i} b={b} [{int(occ)}{int(cor)}{int(en)}]", occ, cor, en)
            assert eng.apply_path() == kernel
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 2. views
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("l3", 4), ("xy", 12)])
def test_views_are_observed_in_place(kind, n):
    """``dev[:, b:b + 1]`` of a [T, 3, D] tensor and ``dev[::3]`` of a [21, 1, D] tensor go through with their strides;
    a last axis that is not contiguous is refused."""
    import torch

    prob, _, d, _ = _problem(kind, n)
    D, T = d**n, 7
    xs, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    with _engine(prob) as eng:
        dev = _dev(eng, xs)
        for b in range(3):
            view = dev[:, b:b + 1]
            assert view.data_ptr() == dev.data_ptr() + 16 * b * D and not view.is_contiguous()
            got = eng.observe_many(view, times, one=1)
            for i in range(T):
                ok &= _check(got, i, b, xs[i, b], pair_ref[(i, b, 1)], e_ref[(i, b)], f"{kind}{n} column b={b} i={i}", col=0)
        wide = torch.zeros((21, 1, D), dtype=torch.complex128, device=eng.device)
        wide[::3] = dev[:, 1:2]
        wide[1::3] = 7.0  # (what a dropped stride would read)
        got = eng.observe_many(wide[::3], times, one=0)
        for i in range(T):
            ok &= _check(got, i, 0, xs[i, 1], pair_ref[(i, 1, 0)], e_ref[(i, 1)], f"{kind}{n} every third i={i}")
        with pytest.raises(ValueError, match="last axis"):
            eng.observe_many(torch.zeros((T, 1, 2 * D), dtype=torch.complex128, device=eng.device)[:, :, ::2], times)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 3. more states than the second grid axis holds
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_stride_over_states():
    """65 540 states of a 4-atom XY register (16.8 MB, the 7-state pattern tiled): the kernels stride over the states
    beyond the 65 535 workgroups of the second grid axis.  The last 16 rows against the reference; every row equals row
    ``i mod 7`` within twice the bound (two evaluations of one state)."""
    kind, n, T7, T = "xy", 4, 7, 65540
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    xs, times, pair_ref, e_ref = _refs(kind, n, T7)
    reps = -(-T // T7)
    big = np.tile(xs[:, :1], (reps, 1, 1))[:T]
    tt = np.tile(np.asarray(times), reps)[:T]
    with _engine(prob) as eng:
        got = eng.observe_many(_dev(eng, big), tt, one=1)
        stats = eng.stats()
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    ok = True
    for r in range(T - 16, T):
        i = r % T7
        ok &= _check(got, i, 0, xs[i, 0], pair_ref[(i, 0, 1)], e_ref[(i, 0)], f"{kind}{n} row {r}", row=r)
    rows = np.arange(T) % T7
    for i in range(T7):
        norm, occ, corr, (s_norm, s_occ, s_corr) = pair_ref[(i, 0, 1)]
        e1, e2, s_abs, w = e_ref[(i, 0)]
        tol1, tol2 = tol_energy_ket(xs[i, 0], w, s_abs)
        sel = rows == i
        ok &= _report("k_gen_obs_pairs", f"rows = {i} mod 7: norm2", np.abs(got["norm2"][sel, 0] - got["norm2"][i, 0]), 2 * tol_sum(D, s_norm))
        ok &= _report("k_gen_obs_pairs", f"rows = {i} mod 7: occupation", np.abs(got["occupation"][sel, 0] - got["occupation"][i, 0]), 2 * tol_sum(D, s_occ))
        ok &= _report("k_gen_obs_pairs", f"rows = {i} mod 7: correlation", np.abs(got["correlation"][sel, 0] - got["correlation"][i, 0]), 2 * tol_sum(D, s_corr))
        ok &= _report("k_gen_obs_energy_many", f"rows = {i} mod 7: <H>", np.abs(got["energy"][sel, 0] - got["energy"][i, 0]), 2 * tol1)
        ok &= _report("k_gen_obs_energy_many", f"rows = {i} mod 7: <H^2>", np.abs(got["energy2"][sel, 0] - got["energy2"][i, 0]), 2 * tol2)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 4. the launch contract, and agreement with the per-time call
# ---------------------------------------------------------------------------------------------------------------------
def test_three_hundred_times_cost_three_launches():
    kind, n, T = "l3", 6, 300
    prob, ham, d, t_end = _problem(kind, n)
    D = d**n
    times = np.linspace(0.0, t_end, T)
    xs = _kets(D, T, 1, 61)
    with _engine(prob) as eng:
        dev = _dev(eng, xs)
        eng.reset_stats()
        got = eng.observe_many(dev, times, one=0)
        stats = eng.stats()
        single = [eng.observe(dev[i], float(times[i]), one=0) for i in range(T)]
        assert eng.stats()["n_applications"] == T
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    worst = np.zeros(5)
    for i in range(T):
        _, _, _, (s_norm, s_occ, s_corr) = ref_pairs_d(ket_probabilities(xs[i, 0]), n, d, 0)
        _, _, s_abs, w = ref_energy_ket(ham, times[i], xs[i, 0])
        tol1, tol2 = tol_energy_ket(xs[i, 0], w, s_abs)
        errs = [abs(got["norm2"][i, 0] - single[i]["norm2"][0]) / (2 * tol_sum(D, s_norm)),
                np.max(np.abs(got["occupation"][i, 0] - single[i]["occupation"][0]) / (2 * tol_sum(D, s_occ))),
                np.max(np.abs(got["correlation"][i, 0] - single[i]["correlation"][0]) / (2 * tol_sum(D, s_corr))),
                abs(got["energy"][i, 0] - single[i]["energy"][0]) / (2 * tol1),
                abs(got["energy2"][i, 0] - single[i]["energy2"][0]) / (2 * tol2)]
        worst = np.maximum(worst, errs)
    print("RATIO observe_many vs observe (norm2, occupation, correlation, <H>, <H^2>) of the sum of both bounds:",
          " ".join(f"{v:.3e}" for v in worst))
    assert np.all(worst <= 1.0)


def test_tables_in_chunks_of_five_times():
    """The chunked path (tables of all times beyond the scratch cap) on a small state: with the 5-per-chunk hook 7 times
    take two chunks, two more launches, and give what one chunk gives within twice the bound."""
    kind, n, T = "l3", 6, 7
    prob, _, d, _ = _problem(kind, n)
    xs, times, pair_ref, e_ref = _refs(kind, n, T)
    ok = True
    with _engine(prob) as eng:
        eng.set_path(False, observe_small_chunks=True)
        dev = _dev(eng, xs)
        eng.reset_stats()
        got = eng.observe_many(dev, times, one=2)
        assert eng.stats()["n_launches"] == 5 and eng.stats()["n_applications"] == 0
    for i, b in itertools.product(range(T), range(3)):
        ok &= _check(got, i, b, xs[i, b], pair_ref[(i, b, 2)], e_ref[(i, b)], f"{kind}{n} chunks i={i} b={b}")
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 5. the handle is left as it was
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi_launch", [False, True])
def test_handle_state_is_untouched(multi_launch):
    """``observe`` and a 20-ns ``solve`` give the same before and after an ``observe_many`` call at other times (the
    handle's coefficients, site matrices and work vector are not the call's).  ``multi_launch``: the solve applies the
    generator launch by launch, through the handle's own tables."""
    kind, n, T = "l3", 6, 7
    prob, ham, d, t_end = _problem(kind, n)
    D = d**n
    xs, times, _, _ = _refs(kind, n, T)
    x, t = xs[2, :1], round(0.61 * t_end, 3) + 0.0001
    init = rand_state(D, 4242)
    init /= np.linalg.norm(init)
    with _engine(prob) as eng:
        if multi_launch:
            eng.set_path(True)
        dx = _dev(eng, x)
        before = eng.observe(dx, t, one=1)
        solved_before = eng.solve(eng.new_state(init), [0.0, 0.02]).cpu().numpy()
        eng.observe_many(_dev(eng, xs), times, one=0)
        after = eng.observe(dx, t, one=1)
        solved_after = eng.solve(eng.new_state(init), [0.0, 0.02]).cpu().numpy()
    for k in ("norm2", "occupation", "correlation"):
        assert np.array_equal(before[k], after[k]), k  # (729 amplitudes are one block of the pair reduction: one order)
    _, _, s_abs, w = ref_energy_ket(ham, t, x[0])
    tol1, tol2 = tol_energy_ket(x[0], w, s_abs)
    ok = _report("k_obs_energy", "<H> before / after observe_many", abs(before["energy"][0] - after["energy"][0]), 2 * tol1)
    ok &= _report("k_obs_energy", "<H^2> before / after observe_many", abs(before["energy2"][0] - after["energy2"][0]), 2 * tol2)
    assert ok and np.array_equal(solved_before, solved_after)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raw(eng, states, n_t, n_b, stride_t, stride_b, times, what, d, n, one, out):
    tt = np.ascontiguousarray(times, dtype=np.float64)
    rc = eng.lib.ryd_general_observe_many(eng._h, states.data_ptr(), n_t, n_b, stride_t, stride_b, tt.ctypes.data, what,
                                          d, n, one, out.data_ptr(), eng._stream())
    return rc, eng.lib.ryd_last_error().decode()


def test_refusals_name_the_alternative():
    import torch
    from pulser_amd._lib import RydError
    from pulser_amd.engine import Engine

    kind, n, T = "l3", 4, 2
    prob, _, d, _ = _problem(kind, n)
    D = d**n
    xs, times, pair_ref, _ = _refs(kind, n, T)
    # a RYD_GENERAL_DENSITY handle
    with _engine(_problem("xy", 2)[0], mesolve=True) as eng:
        rho = torch.zeros((T, 1, eng.dim), dtype=torch.complex128, device=eng.device)
        with pytest.raises(RydError, match="ryd_general_observe") as exc:
            eng.observe_many(rho, times, energy=False)
        assert exc.value.code == UNSUPPORTED
    # collapse operators: no energy moments, the pair sums are served
    ok = True
    with _engine(prob) as eng:
        jump = np.zeros((d, d), complex)
        jump[1, 0] = 0.3
        eng.set_collapse([jump])
        dev = _dev(eng, xs)
        with pytest.raises(RydError, match="collapse operators") as exc:
            eng.observe_many(dev, times, one=1)
        assert exc.value.code == UNSUPPORTED and "pair sums" in str(exc.value)
        got = eng.observe_many(dev, times, one=1, energy=False)
        for i, b in itertools.product(range(T), range(3)):
            ok &= _check(got, i, b, xs[i, b], pair_ref[(i, b, 1)], None, f"collapse handle i={i} b={b}", energy=False)
    # no padded site tables: no energy moments, the pair sums are served
    with _engine(prob) as eng:
        eng.set_path(False, no_fused=True)
        dev = _dev(eng, xs)
        with pytest.raises(RydError, match="ryd_general_observe per time") as exc:
            eng.observe_many(dev, times, one=1)
        assert exc.value.code == UNSUPPORTED
        got = eng.observe_many(dev, times, one=1, energy=False)
        for i, b in itertools.product(range(T), range(3)):
            ok &= _check(got, i, b, xs[i, b], pair_ref[(i, b, 1)], None, f"no_fused handle i={i} b={b}", energy=False)
        # RYD_OBS_DENSITY, strides below D, no times at all
        out = torch.full((T, 3, n * n + n + 3), 7.0, dtype=torch.float64, device=eng.device)
        rc, msg = _raw(eng, dev, T, 3, 3 * D, D, times, 1 | 8, d, n, 0, out)
        assert rc == UNSUPPORTED and "ryd_general_observe" in msg, (rc, msg)
        for st_t, st_b in ((D - 1, D), (3 * D, D - 1)):
            rc, msg = _raw(eng, dev, T, 3, st_t, st_b, times, 3, d, n, 0, out)
            assert rc == INVALID and "smaller than a ket" in msg, (rc, msg)
        rc, msg = _raw(eng, dev, 0, 3, 3 * D, D, [], 3, d, n, 0, out)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool(torch.all(out == 7.0))  # nothing was zeroed, nothing was written
    # a two-level handle
    with Engine.from_problems([local_problem(2, seed=5)], mode="sesolve") as two:
        x2 = torch.zeros((T, 1, 4), dtype=torch.complex128, device=two.device)
        out = torch.zeros((T, 1, 9), dtype=torch.float64, device=two.device)
        rc = two.lib.ryd_general_observe_many(two._h, x2.data_ptr(), T, 1, 4, 4, np.zeros(T).ctypes.data, 3, 2, 2, 0,
                                              out.data_ptr(), two._stream())
        assert rc == INVALID and "ryd_observe_many" in two.lib.ryd_last_error().decode()
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
def _l3_inputs():
    """A 5-atom chain in the 3-level "all" basis: global ground-rydberg drive with a phase jump, local raman drives with
    complex phases on the two end atoms, 400 ns."""
    import os
    import sys

    from pulser_amd import problem as P
    from test_host_logic import _inputs_from_problem

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_general_fixtures as G

    return _inputs_from_problem(G.multilevel_problem(P.register_coords(P.square_rect(1, 5), 6.0), 401, 77, local=(0, 4)))


def _xy_inputs():
    from test_gpu_backend_v2_general import _xy_inputs as xy

    return xy(2, 3)  # 6 atoms, 400 ns, a drive with a non-zero phase


SEQUENCES = {"l3": (_l3_inputs, 3**5, "r", "h"), "xy": (_xy_inputs, 2**6, "d", "u")}


def _observables(one, other=None, variance=True):
    from pulser_amd.backend import CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance, Occupation

    obs = [Occupation(one_state=one), CorrelationMatrix(one_state=one), Energy(), EnergySecondMoment()]
    obs += [EnergyVariance()] if variance else []
    return obs + ([Occupation(one_state=other, tag_suffix="other")] if other else [])


def _backend_bounds(D, e2):
    """Sum of the bounds of the two paths on (pair sums, <H>, <H^2>) for a NORMALISED ket that the test does not read.
    Both paths are held to tests/observe_ref.py: ``tol_sum(D, S_abs)`` with S_abs <= sum p = 1 for every pair sum, and
    ``tol_energy_ket`` with, by Cauchy-Schwarz on ||x||_2 = 1 and ||w||_2 = sqrt(<H^2>) =: h: sum |x_i||w_i| <= h,
    sum |x_i| <= sqrt(D), sum |w_i| <= sqrt(D) h, max |w_i| <= h, and max(1, h) <= 1 + h, h max(1, h) <= 1 + h^2 - so
    every bound is linear or concave in <H^2> and the mean of the bounds of several trajectories is at most the bound
    at their mean <H^2> (the noisy case compares aggregated values).  <H^2> is the per-time path's value (a scale, not a
    fit); |<H>| <= h.  On top, 4 u |value| for the two divisions by the norm (the per-time path normalises the state on
    the host and divides again, the one-call path divides once)."""
    h = np.sqrt(np.abs(e2))
    pair = 2 * tol_sum(D, 1.0) + 4 * U53
    t1 = 2 * (tol_sum(D, h) + 1e-11 * np.sqrt(D) * (1 + h)) + 4 * U53 * h
    t2 = 2 * (tol_sum(D, np.abs(e2)) + 2e-11 * np.sqrt(D) * (1 + np.abs(e2))) + 4 * U53 * np.abs(e2)
    return pair, t1, t2


_WORST = np.zeros(4)


def _compare_paths(D, on, off, obs, variance=True):
    """Every result of the one-call run against the per-time run within ``_backend_bounds``."""
    global _WORST
    ok = True
    times = off.get_result_times(obs[0])
    assert on.get_result_times(obs[0]) == times
    pairs = [o for o in obs if o._base_tag in ("occupation", "correlation_matrix")]
    for t in times:
        e1, e2 = off.get_result(obs[2], t), off.get_result(obs[3], t)
        pair, t1, t2 = _backend_bounds(D, e2)
        d_pair = [float(np.max(np.abs(np.array(on.get_result(o, t)) - np.array(off.get_result(o, t))))) for o in pairs]
        d1, d2 = abs(on.get_result(obs[2], t) - e1), abs(on.get_result(obs[3], t) - e2)
        ok &= all(v <= pair for v in d_pair) and d1 <= t1 and d2 <= t2
        _WORST = np.maximum(_WORST, [d_pair[0] / pair, max(d_pair[1:]) / pair, d1 / t1, d2 / t2])
        if variance:
            ok &= abs(on.get_result(obs[4], t) - off.get_result(obs[4], t)) <= t2 + 2 * abs(e1) * t1 + t1 * t1
    print("RATIO backend one-call vs per-time (occupation, other pair sums, <H>, <H^2>):", " ".join(f"{v:.3e}" for v in _WORST))
    return ok


class _Reads:
    """Counts ``SnapshotStore.get`` (with its arguments), ``fetch_all`` and the stores made."""

    def __init__(self, monkeypatch):
        from pulser_amd.results import SnapshotStore

        self.gets, self.bulk, self.stores = [], 0, 0
        get, fetch_all, init = SnapshotStore.get, SnapshotStore.fetch_all, SnapshotStore.__init__

        def counted_get(store, i, b):
            self.gets.append((i, b))
            return get(store, i, b)

        def counted_fetch_all(store):
            self.bulk += 1
            return fetch_all(store)

        def counted_init(store, *a, **kw):
            self.stores += 1
            init(store, *a, **kw)

        monkeypatch.setattr(SnapshotStore, "get", counted_get)
        monkeypatch.setattr(SnapshotStore, "fetch_all", counted_fetch_all)
        monkeypatch.setattr(SnapshotStore, "__init__", counted_init)


def _count_calls(monkeypatch):
    """The (shape, digit, energy) of every ``GeneralEngine.observe_many`` call and the number of ``observe`` calls."""
    from pulser_amd.engine import GeneralEngine

    many, single = [], []
    real_many, real_single = GeneralEngine.observe_many, GeneralEngine.observe

    def counted_many(self, states, times, one=0, **kw):
        many.append((tuple(states.shape), one, kw.get("energy", True)))
        return real_many(self, states, times, one=one, **kw)

    def counted_single(self, *a, **kw):
        single.append(1)
        return real_single(self, *a, **kw)

    monkeypatch.setattr(GeneralEngine, "observe_many", counted_many)
    monkeypatch.setattr(GeneralEngine, "observe", counted_single)
    return many, single


def _run(inputs, cfg, min_times, seed=None):
    from pulser_amd.backend import QutipBackendV2

    if seed is not None:
        np.random.seed(seed)  # (the noise trajectories are drawn when the backend is built)
    backend = QutipBackendV2(inputs, config=cfg)
    backend.observe_many_min_times = min_times
    res = backend.run()
    return res, QutipBackendV2.last_observable_engine_stats


@pytest.mark.parametrize("which", ["l3", "xy"])
def test_backend_one_call_per_one_state_and_no_state_read(which, monkeypatch):
    """130 evaluation times at the path's floor of 128: every stored value agrees with the per-time path's within the
    sum of both bounds; the one-call run made one ``observe_many`` call per distinct one-state (the first with the
    energies), no ``ryd_general_observe`` call and no generator application, and read no snapshot."""
    from pulser_amd.backend import QutipConfig

    make, D, one, other = SEQUENCES[which]
    inputs = make()
    times = np.linspace(0.01, 1.0, 130).tolist()
    obs = _observables(one, other)
    cfg = QutipConfig(default_evaluation_times=times, observables=obs)
    off, stats_off = _run(inputs, cfg, None)
    assert stats_off["n_applications"] == len(times)
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 128)
    assert [c[0] for c in many] == [(130, 1, D)] * 2 and [c[2] for c in many] == [True, False], many
    assert len({c[1] for c in many}) == 2 and single == []
    assert stats["n_applications"] == 0 and stats["n_launches"] == 3 + 1, stats
    assert reads.stores == 1 and reads.gets == [] and reads.bulk == 0, (reads.stores, reads.gets, reads.bulk)
    assert _compare_paths(D, on, off, obs)


@pytest.mark.parametrize("which", ["l3", "xy"])
def test_backend_below_the_floor_keeps_the_per_time_path(which, monkeypatch):
    """127 evaluation times: the per-time path, whatever the threshold says, with the launches of the path switched off."""
    from pulser_amd.backend import QutipConfig

    make, D, one, other = SEQUENCES[which]
    inputs = make()
    obs = _observables(one, other)
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, 127).tolist(), observables=obs)
    off, stats_off = _run(inputs, cfg, None)
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    for threshold in (128, 1):
        on, stats = _run(inputs, cfg, threshold)
        assert many == [] and reads.stores == 0
        assert stats["n_launches"] == stats_off["n_launches"] and stats["n_applications"] == stats_off["n_applications"] == 127
        assert on.get_tagged_results().keys() == off.get_tagged_results().keys()
        assert _compare_paths(D, on, off, obs)  # (two per-time runs: the atomic sums of k_obs_energy may move the last bits)


@pytest.mark.parametrize("which", ["l3", "xy"])
def test_backend_states_that_are_read_are_the_same_states(which, monkeypatch):
    """``StateResult`` at two times next to the observables: exactly those two snapshots are copied, and they equal the
    per-time run's bit for bit."""
    from pulser_amd.backend import QutipConfig, StateResult

    make, D, one, other = SEQUENCES[which]
    inputs = make()
    times = np.linspace(0.01, 1.0, 130).tolist()
    sr = StateResult(evaluation_times=[times[64], 1.0])
    obs = _observables(one)
    cfg = QutipConfig(default_evaluation_times=times, observables=obs + [sr])
    off, _ = _run(inputs, cfg, None)
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 128)
    assert len(many) == 1 and single == [] and stats["n_applications"] == 0, (many, single, stats)
    for t in (times[64], 1.0):
        assert np.array_equal(np.array(on.get_result(sr, t).to_qobj()), np.array(off.get_result(sr, t).to_qobj()))
    assert len(reads.gets) == 2 and reads.bulk == 0, (reads.gets, reads.bulk)
    assert _compare_paths(D, on, off, obs)


def test_backend_noisy_xy_one_call_per_trajectory_store(monkeypatch):
    """The seeded SPAM trajectories (state-preparation errors: bad atoms) of the XY fixture, solved together in one
    launch (``solve_many``): one store and one ``observe_many`` call per trajectory, no per-time call, and the
    aggregated results of both paths agree within the bounds under the same seed."""
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipConfig
    from pulser_amd.hamiltonian_data import SequenceInputs

    prob, extra = load_fixture("noisy_xy_0.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    D = 2**4
    obs = _observables("d", variance=False)
    nm = NoiseModel(state_prep_error=0.4, p_false_pos=0.01, p_false_neg=0.05)
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, 130).tolist(), observables=obs, noise_model=nm,
                      n_trajectories=6)
    seed = int(extra["seed"])
    off, _ = _run(inputs, cfg, None, seed=seed)
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 128, seed=seed)
    assert reads.stores >= 2 and len(many) == reads.stores and single == [], (many, reads.stores, single)
    assert all(c[0] == (130, 1, D) and c[2] for c in many) and len({c[1] for c in many}) == 1, many
    assert stats["n_applications"] == 0 and stats["n_launches"] == 3 * len(many), stats
    assert reads.gets == [] and reads.bulk == 0
    assert _compare_paths(D, on, off, obs, variance=False)


def test_backend_master_equation_run_is_left_alone(monkeypatch):
    """A dephasing XY run (master equation, density-matrix results) at 130 evaluation times: no store, no one-call, and
    the noiseless engine is the one the run gets with the path switched off - same application kernel (explicit terms
    for so small a register, not the matrix-free lowering of the one-call route), same launches and applications."""
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipConfig
    from pulser_amd.hamiltonian_data import SequenceInputs

    prob, _ = load_fixture("noisy_xy_0.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    obs = _observables("d", variance=False)
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, 130).tolist(), observables=obs,
                      noise_model=NoiseModel(dephasing_rate=0.05))
    off, stats_off = _run(inputs, cfg, None)
    reads = _Reads(monkeypatch)
    many, single = _count_calls(monkeypatch)
    import pulser_amd.general as general

    lowered, real_lower = [], general.lower_general

    def counted_lower(*a, **kw):
        lowered.append(kw.get("matrix_free"))
        return real_lower(*a, **kw)

    monkeypatch.setattr(general, "lower_general", counted_lower)
    on, stats = _run(inputs, cfg, 128)
    assert many == [] and reads.stores == 0 and len(single) > 0, (many, reads.stores, len(single))
    assert lowered and all(m is None for m in lowered), lowered  # (the default lowering: by register size)
    for key in ("apply_path", "n_launches", "n_applications"):
        assert stats[key] == stats_off[key], (key, stats, stats_off)
    assert on.get_tagged_results().keys() == off.get_tagged_results().keys()


def test_emulator_default_is_unchanged():
    """``QutipEmulator.run()`` on a 3-level problem without the keyword: host ``QState`` states, and ``expect`` of a
    non-diagonal operator is the host formula bit for bit; with ``general_device_snapshots=True`` the same states are
    ``LazyState`` snapshots of one store."""
    import os
    import sys

    from pulser_amd import QutipEmulator
    from pulser_amd import problem as P
    from pulser_amd.results import LazyState, QState
    from test_host_logic import _inputs_from_problem

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_general_fixtures as G

    inputs = _inputs_from_problem(G.multilevel_problem(P.register_coords(P.square_rect(1, 3), 6.0), 121, 78, local=(0,)))
    emu = QutipEmulator(inputs, sampling_rate=1.0)
    emu.set_evaluation_times(list(np.linspace(0.0, 0.12, 13)))
    with pytest.warns(DeprecationWarning):
        res = emu.run()
    assert len(res.states) >= 13 and all(type(st) is QState for st in res.states)
    rng = np.random.default_rng(8)
    m = rng.normal(size=(27, 27)) + 1j * rng.normal(size=(27, 27))
    m = m + m.conj().T
    want = np.array([np.vdot(np.asarray(st), m @ np.asarray(st)).real for st in res.states])
    assert np.array_equal(res.expect([m])[0], want)
    with pytest.warns(DeprecationWarning):
        kept = emu.run(general_device_snapshots=True)
    assert type(kept.states[0]) is QState and all(isinstance(st, LazyState) for st in kept.states[1:])
    assert len({id(st._store) for st in kept.states[1:]}) == 1
    for a, b in zip(kept.states, res.states):
        assert np.array_equal(np.asarray(a), np.asarray(b))

"""GPU: ``ryd_observe_many`` (k_eval_coefs_many, k_obs_pairs, k_obs_energy_many) - the occupations, correlations and
energy moments of the kets of every evaluation time in one call - called directly through ``Engine.observe_many`` and
pinned to the longdouble host reference of tests/observe_ref.py, and its use by ``QutipBackendV2``.

States are random, unnormalised and without symmetry, problems have per-atom amplitude, detuning and a non-zero phase,
every entry of a batched handle has its own problem (entry 1 with a bad atom), and the atom counts sit on the edges of
the 2^11-amplitude tile of k_obs_energy_many: registers smaller than a tile, exactly one tile, 2 .. 32 tiles with 1 .. 5
partner bits served from global memory.  Times: 0, interior, exactly a knot, the last knot, repeated, unsorted.

Tolerances are the derived ones of tests/observe_ref.py (``tol_sum``: worst-case summation bound; ``tol_energy_ket``:
that plus the project's 1e-11 bar of one generator application, which the fused w = H x is held to as well); nothing is
fitted.  The backend cases compare the one-call path with the per-time path within the sum of the two paths' bounds,
written for a normalised state without reading it (``_backend_bounds``).  Every case prints ``error / tolerance``
before it asserts.  Worst ratios seen on an MI355X:

    k_obs_pairs           0.19      (the 4-term norm of a 2-atom ket; below 0.02 from 10 atoms on)
    k_obs_energy_many     3.0e-05
    300 times, 10 atoms   pair sums identical to per-time ``Engine.observe``; <H> 5.3e-06, <H^2> 3.0e-06 of both bounds
    backend, both paths   occupation 0.015, correlation 0.005, <H> 7.2e-06, <H^2> 3.7e-06
"""
import itertools

import numpy as np
import pytest

from helpers import blockade_radius, local_problem, rand_state
from observe_ref import U53, ket_probabilities, ref_energy_ket, ref_pairs, tol_energy_ket, tol_sum

pytestmark = pytest.mark.gpu

TB = 11                                   # kObsManyTB of k_observe.hpp
T_KNOT, T_LAST = 0.2, 0.4                 # knots 200 and 400 of the 401 of local_problem (1-ns grid)
TIMES = {1: [0.12345], 2: [T_KNOT, 0.0], 7: [T_LAST, 0.0, 0.12345, T_KNOT, 0.12345, 0.3, 0.05]}
SCALES = (1.0, 0.6, 1.9)


def _report(kernel, what, err, tol):
    err, tol = np.asarray(err, dtype=float), np.asarray(tol, dtype=float)
    ok = bool(np.all(err <= tol))
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0, tol, np.finfo(float).tiny))))
    print(f"RATIO {kernel:18s} {what:40s} err {float(np.max(err)):.3e} tol {float(np.max(tol)):.3e} ratio {ratio:.3e}")
    return ok


def _problems(n, B):
    """One problem per batch entry (own register, drives, detunings, phases); entry 1 has a bad atom."""
    from pulser_amd.problem import C6_LEVEL70, interaction_matrix

    probs = [local_problem(n, seed=100 * n + s) for s in range(B)]
    if B > 1 and n >= 2:
        probs[1]["bad_atoms"][1] = True
        for k in ("amp", "det", "phase"):
            probs[1]["samples"]["Local"]["ground-rydberg"][1][k] *= 0.0
        probs[1]["interaction_matrix"] = interaction_matrix(probs[1]["coords"], C6_LEVEL70, probs[1]["bad_atoms"])
    return probs


_HAMS = {}


def _ham(n, B, b):
    """Oracle Hamiltonian of entry b of ``_problems(n, B)``; those of one atom number at a time."""
    from oracle import qutip_path as qp

    if _HAMS.get("n") != n:
        _HAMS.clear()
        _HAMS["n"] = n
    key = (b, B > 1 and n >= 2 and b == 1)
    if key not in _HAMS:
        _HAMS[key] = qp.build_hamiltonian(_problems(n, B)[b])
    return _HAMS[key]


def _kets(n, T, B):
    """[T, B, 2^n]: a different random ket for every (time, entry), scaled by entry."""
    return np.stack([np.stack([SCALES[(i + b) % 3] * rand_state(2**n, 1000 * n + 10 * i + b) for b in range(B)])
                     for i in range(T)])


def _engine(problems, mode="sesolve"):
    from pulser_amd.engine import Engine

    return Engine.from_problems(problems, mode=mode)


def _dev(eng, host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).to(eng.device)


def _check_state(got, i, b, x, ham, t, n, tag, occupation=True, correlation=True, energy=True):
    """Every requested output of state (i, b) against the longdouble reference."""
    D = 2**n
    norm, occ, corr, (s_norm, s_occ, s_corr) = ref_pairs(ket_probabilities(x), n)
    ok = _report("k_obs_pairs", f"{tag} norm2", abs(got["norm2"][i, b] - norm), tol_sum(D, s_norm))
    if occupation:
        ok &= _report("k_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][i, b] - occ), tol_sum(D, s_occ))
    if correlation:
        ok &= _report("k_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][i, b] - corr), tol_sum(D, s_corr))
    if energy:
        e1, e2, s_abs, w = ref_energy_ket(ham, t, x)
        tol1, tol2 = tol_energy_ket(x, w, s_abs)
        ok &= _report("k_obs_energy_many", f"{tag} <H>", abs(got["energy"][i, b] - e1), tol1)
        ok &= _report("k_obs_energy_many", f"{tag} <H^2>", abs(got["energy2"][i, b] - e2), tol2)
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# direct: atom counts on the tile's edges x times x batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 2, 3, TB - 1, TB, TB + 1, TB + 2, 14, 16])
def test_observe_many_batched_handle(n, T):
    """B = 3 on a handle of batch 3: a dropped batch offset in the coefficient table or in e0 shows (entry 1 has a bad
    atom, every entry its own register).  First call on a fresh handle."""
    B, times = 3, TIMES[T]
    xs = _kets(n, T, B)
    with _engine(_problems(n, B)) as eng:
        got = eng.observe_many(_dev(eng, xs), times)
        stats = eng.stats()
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    assert got["norm2"].shape == (T, B) and got["occupation"].shape == (T, B, n)
    assert got["correlation"].shape == (T, B, n, n) and got["energy"].shape == got["energy2"].shape == (T, B)
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check_state(got, i, b, xs[i, b], _ham(n, B, b), times[i], n, f"n={n} T={T} i={i} b={b} t={times[i]}")
    assert ok


@pytest.mark.parametrize("n", [3, TB + 1, 14])
def test_observe_many_one_problem_serves_every_entry(n):
    """B = 3 states per time on a handle of batch 1."""
    B, T = 3, 2
    times = TIMES[T]
    xs = _kets(n, T, B)
    with _engine(_problems(n, 1)) as eng:
        got = eng.observe_many(_dev(eng, xs), times)
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check_state(got, i, b, xs[i, b], _ham(n, 1, 0), times[i], n, f"shared n={n} i={i} b={b}")
    assert ok


def test_observe_many_batch_mismatch_is_invalid():
    from pulser_amd._lib import RydError

    n = 3
    with _engine(_problems(n, 2)) as eng:
        with pytest.raises(RydError) as err:
            eng.observe_many(_dev(eng, _kets(n, 2, 3)), TIMES[2])
    assert err.value.code == -1, err.value  # RYD_ERR_INVALID


def test_observe_many_300_times_against_per_time_observe():
    """10 atoms, 300 unsorted times (knots, the last knot and repeats among them), one state each: every time against
    per-time ``Engine.observe`` within the sum of both bounds, 8 sampled times against the longdouble reference; three
    launches whatever T is."""
    n, T = 10, 300
    D = 2**n
    rng = np.random.default_rng(7)
    times = rng.uniform(0.0, T_LAST, T)
    times[[0, 17, 150, 151, 299]] = [T_LAST, T_KNOT, 0.0, 0.0, 0.123]
    times[40:44] = 0.123  # repeated
    xs = _kets(n, T, 1)
    ham = _ham(n, 1, 0)
    with _engine(_problems(n, 1)) as eng:
        dev = _dev(eng, xs)
        got = eng.observe_many(dev, times)
        stats = eng.stats()
        single = [eng.observe(dev[i], float(times[i])) for i in range(T)]
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    ok = True
    worst = np.zeros(5)
    for i in range(T):
        x = xs[i, 0]
        _, _, _, (s_norm, s_occ, s_corr) = ref_pairs(ket_probabilities(x), n)
        _, _, s_abs, w = ref_energy_ket(ham, times[i], x)
        tol1, tol2 = tol_energy_ket(x, w, s_abs)
        pairs = [(abs(got["norm2"][i, 0] - single[i]["norm2"][0]), 2 * tol_sum(D, s_norm)),
                 (np.abs(got["occupation"][i, 0] - single[i]["occupation"][0]), 2 * tol_sum(D, s_occ)),
                 (np.abs(got["correlation"][i, 0] - single[i]["correlation"][0]), 2 * tol_sum(D, s_corr)),
                 (abs(got["energy"][i, 0] - single[i]["energy"][0]), 2 * tol1),
                 (abs(got["energy2"][i, 0] - single[i]["energy2"][0]), 2 * tol2)]
        for j, (err, tol) in enumerate(pairs):
            worst[j] = max(worst[j], float(np.max(np.asarray(err, dtype=float) / np.asarray(tol, dtype=float))))
            ok &= bool(np.all(err <= tol))
    print("RATIO many vs per-time (norm2, occupation, correlation, <H>, <H^2>):", " ".join(f"{v:.3e}" for v in worst))
    for i in (0, 17, 40, 43, 150, 151, 222, 299):
        ok &= _check_state(got, i, 0, xs[i, 0], ham, times[i], n, f"n={n} T=300 i={i} t={times[i]:.5f}")
    assert ok


@pytest.mark.parametrize("what", [dict(), dict(correlation=False, energy=False)], ids=["all", "occupation"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 11])
def test_observe_many_pair_sums_equal_per_time_observe_to_the_bit(n, B, what):
    """``ryd_observe`` and ``ryd_observe_many`` launch ONE pair kernel (k_obs_pairs).  Up to 11 atoms a state is one chunk
    of 2 048 probabilities (11 atoms fill it, 1 atom is one pair and padding), so every output slot receives exactly
    one atomicAdd, the result is deterministic, and the two callers must agree bit for bit."""
    T = 4
    times = TIMES[7][:T]
    with _engine(_problems(n, B)) as eng:
        dev = _dev(eng, _kets(n, T, B))
        got = eng.observe_many(dev, times, **what)
        single = [eng.observe(dev[i], times[i], **what) for i in range(T)]
    for i, key in itertools.product(range(T), ("occupation", "correlation", "norm2")):
        assert np.array_equal(got[key][i], single[i][key]), (i, key, got[key][i], single[i][key])
    if what:
        assert np.all(got["correlation"] == 0.0) and np.any(got["occupation"] != 0.0)


def test_observe_many_pair_sums_against_per_time_observe_two_chunks():
    """12 atoms: two chunks add into every slot, in either order, so the two callers agree within the sum of their
    bounds (``tol_sum`` of tests/observe_ref.py) and no bit equality is asserted."""
    n, B, T = 12, 3, 4
    D = 2**n
    times = TIMES[7][:T]
    xs = _kets(n, T, B)
    with _engine(_problems(n, B)) as eng:
        dev = _dev(eng, xs)
        got = eng.observe_many(dev, times, energy=False)
        single = [eng.observe(dev[i], times[i], energy=False) for i in range(T)]
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        _, _, _, sums = ref_pairs(ket_probabilities(xs[i, b]), n)
        for key, s_abs in zip(("norm2", "occupation", "correlation"), sums):
            ok &= _report("k_obs_pairs", f"n=12 i={i} b={b} {key} many vs per-time",
                          np.abs(got[key][i, b] - single[i][key][b]), 2 * tol_sum(D, s_abs))
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# strides
# ---------------------------------------------------------------------------------------------------------------------
def test_observe_many_views_and_padded_strides():
    """``dev[:, 1:2]`` of a [T, 3, D] tensor observed in place, and a first axis padded by 37 amplitudes."""
    import torch

    n, T = 10, 7
    D = 2**n
    times = TIMES[T]
    xs = _kets(n, T, 3)
    ham = _ham(n, 1, 0)
    ok = True
    with _engine(_problems(n, 1)) as eng:
        dev = _dev(eng, xs)
        got = eng.observe_many(dev[:, 1:2], times)
        assert got["norm2"].shape == (T, 1)
        for i in range(T):
            ok &= _check_state(got, i, 0, xs[i, 1], ham, times[i], n, f"view [:, 1:2] i={i}")
        pad = torch.full((T * (3 * D + 37),), complex("nan"), dtype=torch.complex128, device=eng.device)
        view = pad.as_strided((T, 3, D), (3 * D + 37, D, 1))
        view.copy_(dev)
        got = eng.observe_many(view, times)
        for i, b in itertools.product(range(T), range(3)):
            ok &= _check_state(got, i, b, xs[i, b], ham, times[i], n, f"padded stride_t i={i} b={b}")
    assert ok


def test_observe_many_second_state_beyond_4_gib():
    """Two 10-atom states in one ``torch.empty`` allocation, the second one more than 2^32 bytes after the first:
    the state offset is 64-bit.  Only the two states are written; nothing else of the allocation is read."""
    import torch

    n = 10
    D = 2**n
    gap = 2**28 + 4099  # complex128 elements: 2^32 bytes and a bit
    times = [0.12345, T_KNOT]
    xs = _kets(n, 2, 1)
    ham = _ham(n, 1, 0)
    with _engine(_problems(n, 1)) as eng:
        big = torch.empty(gap + D, dtype=torch.complex128, device=eng.device)
        view = big.as_strided((2, 1, D), (gap, D, 1))
        view.copy_(_dev(eng, xs))
        got = eng.observe_many(view, times)
        del view, big
    ok = True
    for i in range(2):
        ok &= _check_state(got, i, 0, xs[i, 0], ham, times[i], n, f"offset {i * gap * 16} bytes")
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# `what` subsets, closed forms, refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occupation,correlation,energy",
                         [w for w in itertools.product([False, True], repeat=3) if any(w)])
def test_observe_many_what_subsets(occupation, correlation, energy):
    """What was not asked for is exactly 0; the norm is always there."""
    n, B, T = 5, 3, 2
    times = TIMES[T]
    xs = _kets(n, T, B)
    with _engine(_problems(n, B)) as eng:
        got = eng.observe_many(_dev(eng, xs), times, occupation=occupation, correlation=correlation, energy=energy)
        launches = eng.stats()["n_launches"]
    assert launches == (1 if occupation or correlation else 0) + (2 if energy else 0)
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check_state(got, i, b, xs[i, b], _ham(n, B, b), times[i], n,
                           f"what={occupation:d}{correlation:d}{energy:d} i={i} b={b}", occupation=occupation,
                           correlation=correlation, energy=energy)
    if not occupation:
        assert np.all(got["occupation"] == 0.0)
    if not correlation:
        assert np.all(got["correlation"] == 0.0)
    if not energy:
        assert np.all(got["energy"] == 0.0) and np.all(got["energy2"] == 0.0)
    assert ok


def test_observe_many_basis_states_closed_forms():
    """Every basis state |a> of 3 atoms (amplitude exactly 1): occupations, correlations and the norm are exact, <H> is
    H_aa and <H^2> is sum_b |H_ba|^2 of the oracle's dense H(t) (within the bound of the one-term reference)."""
    n, t = 3, 0.12345
    D = 2**n
    xs = np.eye(D, dtype=complex)[:, None, :]
    ham = _ham(n, 1, 0)
    H = np.asarray(ham.matrix(t).toarray())
    with _engine(_problems(n, 1)) as eng:
        got = eng.observe_many(_dev(eng, xs), [t] * D)
    ok = True
    for a in range(D):
        bits = np.array([1 - ((a >> (n - 1 - k)) & 1) for k in range(n)], dtype=float)
        assert got["norm2"][a, 0] == 1.0
        assert np.array_equal(got["occupation"][a, 0], bits), (a, got["occupation"][a, 0])
        assert np.array_equal(got["correlation"][a, 0], np.outer(bits, bits)), (a, got["correlation"][a, 0])
        _, _, s_abs, w = ref_energy_ket(ham, t, xs[a, 0])
        tol1, tol2 = tol_energy_ket(xs[a, 0], w, s_abs)
        ok &= _report("k_obs_energy_many", f"|{a}> H_aa", abs(got["energy"][a, 0] - H[a, a].real), tol1)
        ok &= _report("k_obs_energy_many", f"|{a}> sum_b |H_ba|^2", abs(got["energy2"][a, 0] - np.sum(np.abs(H[:, a]) ** 2)), tol2)
    assert ok


def test_observe_many_refusals():
    """A mesolve handle, a general handle, RYD_OBS_DENSITY, a handle with detuning terms and a stride below 2^N return
    their error code and leave ``ryd_last_error`` set; ``n_times = 0`` is RYD_OK."""
    import torch
    from helpers import three_level_problem
    from pulser_amd import _lib
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general
    from pulser_amd.terms import lower

    n = 3
    D = 2**n
    lib = _lib.load()
    times = np.array([0.1, 0.2])

    def call(eng, x, n_times=2, what=7, stride_t=D, stride_b=D):
        out = torch.zeros((2, 1, n * n + n + 3), dtype=torch.float64, device=x.device)
        rc = lib.ryd_observe_many(eng._h, x.data_ptr(), n_times, 1, stride_t, stride_b, times.ctypes.data, what,
                                  out.data_ptr(), eng._stream())
        torch.cuda.synchronize()
        return rc, lib.ryd_last_error().decode()

    with _engine(_problems(n, 1)) as eng:
        x = _dev(eng, _kets(n, 2, 1))
        assert call(eng, x)[0] == 0
        assert call(eng, x, n_times=0)[0] == 0
        rc, msg = call(eng, x, what=7 | 8)
        assert rc == -3 and "DENSITY" in msg, (rc, msg)
        rc, msg = call(eng, x, stride_t=D - 1)
        assert rc == -1 and "stride" in msg, (rc, msg)
        rc, msg = call(eng, x, stride_b=D - 1)
        assert rc == -1 and "stride" in msg, (rc, msg)
        with pytest.raises(ValueError):
            eng.observe_many(x.to(torch.complex64), times)
        with pytest.raises(ValueError):
            eng.observe_many(x.cpu(), times)
        with pytest.raises(ValueError):
            eng.observe_many(torch.zeros((2, 1, 2 * D), dtype=torch.complex128, device=eng.device)[..., ::2], times)
        with _engine(_problems(n, 1), mode="mesolve") as me:
            rc, msg = call(me, x)
            assert rc == -3 and "sesolve" in msg, (rc, msg)
        # extra detuning terms: the table of the same problem with one (zero-scale) term on atom 0
        tables = lower(_problems(n, 1))
        from pulser_amd.terms import DTERM_DTYPE

        dt = np.zeros(1, dtype=DTERM_DTYPE)
        desc = np.array(tables.desc, copy=True)
        desc["extra"][0, 0] = 1
        from dataclasses import replace

        from pulser_amd.engine import Engine

        with Engine(replace(tables, desc=desc, dterms=dt)) as de:
            rc, msg = call(de, x)
            assert rc == -3 and "detuning" in msg, (rc, msg)
    prob, _, _ = three_level_problem(4)
    with GeneralEngine(lower_general(prob, mesolve=False)) as ge:
        xg = torch.zeros((2, 1, ge.dim), dtype=torch.complex128, device=ge.device)
        rc = lib.ryd_observe_many(ge._h, xg.data_ptr(), 2, 1, ge.dim, ge.dim, times.ctypes.data, 7, xg.data_ptr(), 0)
        assert rc == -1 and "general" in lib.ryd_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(n):
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import single_global_channel

    coords = P.register_coords(P.square_rect(1, n), blockade_radius())
    smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
    return single_global_channel(coords, smp, P.C6_LEVEL70, extended=False)


def _observables(variance=True, one_state=None):
    from pulser_amd.backend import CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance, Occupation

    return [Occupation(one_state=one_state), CorrelationMatrix(one_state=one_state), Energy(),
            EnergySecondMoment()] + ([EnergyVariance()] if variance else [])


def _backend_bounds(n, e1, e2):
    """Sum of the bounds of the two paths on (pair sums, <H>, <H^2>) for a NORMALISED ket that the test does not read.
    Both paths are held to tests/observe_ref.py: ``tol_sum(D, S_abs)`` with S_abs <= sum p = 1 for every pair sum, and
    ``tol_energy_ket`` with, by Cauchy-Schwarz on ||x||_2 = 1 and ||w||_2 = sqrt(<H^2>): sum |x_i||w_i| <= ||w||_2,
    sum |x_i| <= sqrt(D), sum |w_i| <= sqrt(D) ||w||_2, max |w_i| <= ||w||_2.  <H^2> is the per-time path's value (a
    scale, not a fit).  On top, 4 u |value| for the two divisions by the norm (the per-time path normalises the state on
    the host and divides again, the one-call path divides once)."""
    D = 2.0**n
    w2 = np.sqrt(np.abs(e2))
    top = np.maximum(1.0, w2)
    pair = 2 * tol_sum(D, 1.0) + 4 * U53
    t1 = 2 * (tol_sum(D, w2) + 1e-11 * np.sqrt(D) * top) + 4 * U53 * np.abs(e1)
    t2 = 2 * (tol_sum(D, np.abs(e2)) + 2e-11 * np.sqrt(D) * w2 * top) + 4 * U53 * np.abs(e2)
    return pair, t1, t2


def _compare_paths(n, on, off, obs, variance=True):
    """Every result of the one-call run against the per-time run within ``_backend_bounds``."""
    ok = True
    times = off.get_result_times(obs[0])
    assert on.get_result_times(obs[0]) == times
    for t in times:
        e1, e2 = off.get_result(obs[2], t), off.get_result(obs[3], t)
        pair, t1, t2 = _backend_bounds(n, e1, e2)
        d_occ = np.abs(np.array(on.get_result(obs[0], t)) - np.array(off.get_result(obs[0], t)))
        d_cor = np.abs(np.array(on.get_result(obs[1], t)) - np.array(off.get_result(obs[1], t)))
        ok &= bool(np.all(d_occ <= pair)) and bool(np.all(d_cor <= 3 * pair))  # (complemented: 1 - o_i - o_j + c_ij)
        ok &= abs(on.get_result(obs[2], t) - e1) <= t1 and abs(on.get_result(obs[3], t) - e2) <= t2
        _compare_paths.worst = np.maximum(_compare_paths.worst, [np.max(d_occ) / pair, np.max(d_cor) / (3 * pair),
                                                                 abs(on.get_result(obs[2], t) - e1) / t1,
                                                                 abs(on.get_result(obs[3], t) - e2) / t2])
        if variance:
            ok &= abs(on.get_result(obs[4], t) - off.get_result(obs[4], t)) <= t2 + 2 * abs(e1) * t1
    print("RATIO backend one-call vs per-time (occupation, correlation, <H>, <H^2>):",
          " ".join(f"{v:.3e}" for v in _compare_paths.worst))
    return ok


_compare_paths.worst = np.zeros(4)


class _Reads:
    """Counts ``SnapshotStore.get`` (with its arguments) and ``fetch_all``."""

    def __init__(self, monkeypatch):
        from pulser_amd.results import SnapshotStore

        self.gets, self.bulk = [], 0
        get, fetch_all = SnapshotStore.get, SnapshotStore.fetch_all

        def counted_get(store, i, b):
            self.gets.append((i, b))
            return get(store, i, b)

        def counted_fetch_all(store):
            self.bulk += 1
            return fetch_all(store)

        monkeypatch.setattr(SnapshotStore, "get", counted_get)
        monkeypatch.setattr(SnapshotStore, "fetch_all", counted_fetch_all)


def _count_observe_many(monkeypatch):
    from pulser_amd.engine import Engine

    calls = []
    real = Engine.observe_many

    def counted(self, states, times, **kw):
        calls.append(tuple(states.shape))
        return real(self, states, times, **kw)

    monkeypatch.setattr(Engine, "observe_many", counted)
    return calls


def _run(inputs, cfg, min_times, monkeypatch, seed=None):
    from pulser_amd.backend import QutipBackendV2

    monkeypatch.setattr(QutipBackendV2, "observe_many_min_times", min_times)
    if seed is not None:
        np.random.seed(seed)
    res = QutipBackendV2(inputs, config=cfg).run()
    return res, QutipBackendV2.last_observable_engine_stats


def test_backend_one_call_serves_every_time_and_reads_no_state(monkeypatch):
    from pulser_amd.backend import QutipConfig

    n = 10
    inputs = _inputs(n)
    times = np.linspace(0.01, 1.0, 150).tolist()
    obs = _observables()
    cfg = QutipConfig(default_evaluation_times=times, observables=obs)
    off, stats_off = _run(inputs, cfg, None, monkeypatch)
    assert stats_off["n_applications"] == len(times)
    reads = _Reads(monkeypatch)
    calls = _count_observe_many(monkeypatch)
    on, stats = _run(inputs, cfg, 128, monkeypatch)
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    assert calls == [(150, 1, 2**n)] and reads.gets == [] and reads.bulk == 0, (calls, reads.gets, reads.bulk)
    assert _compare_paths(n, on, off, obs)


def test_backend_states_that_are_read_are_the_same_states(monkeypatch):
    """``StateResult`` at two times and a callback that reads the state at a third (one where no observable fires):
    exactly those three snapshots are copied, and they equal the per-time run's bit for bit.  The 150 times of the
    observables are not equally spaced among the 3 101 a callback makes the solver keep: the call takes a gathered copy."""
    from pulser_amd.backend import QutipConfig, StateResult

    n = 10
    inputs = _inputs(n)
    times = np.linspace(0.01, 1.0, 150)
    seen = {}

    def callback(config, t, state, hamiltonian, result):  # (callbacks see all 3 101 times of the 1-ns grid)
        if abs(t * 3100 - 650) < 1e-6:
            seen["state"] = np.array(state.to_qobj())

    sr = StateResult(evaluation_times=[0.5, 1.0])
    obs = _observables()
    cfg = QutipConfig(default_evaluation_times=times.tolist(), observables=obs + [sr], callbacks=[callback])
    off, _ = _run(inputs, cfg, None, monkeypatch)
    kept = {"cb": seen.pop("state"), 0.5: np.array(off.get_result(sr, 0.5).to_qobj()), 1.0: np.array(off.get_result(sr, 1.0).to_qobj())}
    reads = _Reads(monkeypatch)
    calls = _count_observe_many(monkeypatch)
    on, stats = _run(inputs, cfg, 128, monkeypatch)
    assert len(calls) == 1 and stats["n_applications"] == 0 and stats["n_launches"] <= 3, (calls, stats)
    assert np.array_equal(seen["state"], kept["cb"])
    for t in (0.5, 1.0):
        assert np.array_equal(np.array(on.get_result(sr, t).to_qobj()), kept[t])
    # snapshot i is the state after i + 1 ns (the initial state is not in the store): the callback's 650 ns, then the two
    # times of StateResult, 1 550 ns and 3 100 ns, in the order fill() reaches them
    assert reads.gets == [(649, 0), (1549, 0), (3099, 0)] and reads.bulk == 0, (reads.gets, reads.bulk)
    assert _compare_paths(n, on, off, obs)


def test_backend_noisy_run_shares_one_call_per_solve(monkeypatch):
    """Amplitude noise, 3 trajectories, 8 atoms, 140 times: the sequences of one batched solve (and their repetitions)
    share one ``observe_many`` call over the store; the aggregated results equal the per-time run's."""
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipConfig
    from pulser_amd.results import SnapshotStore

    n = 8
    inputs = _inputs(n)
    times = np.linspace(0.01, 1.0, 140).tolist()
    obs = _observables(variance=False)
    cfg = QutipConfig(default_evaluation_times=times, observables=obs, noise_model=NoiseModel(amp_sigma=0.05), n_trajectories=3)
    off, _ = _run(inputs, cfg, None, monkeypatch, seed=11)
    stores = []
    init = SnapshotStore.__init__

    def counted_init(self, *a, **kw):
        stores.append(1)
        init(self, *a, **kw)

    monkeypatch.setattr(SnapshotStore, "__init__", counted_init)
    calls = _count_observe_many(monkeypatch)
    on, stats = _run(inputs, cfg, 128, monkeypatch, seed=11)
    assert len(stores) >= 1 and len(calls) == len(stores), (calls, stores)
    assert sum(c[1] for c in calls) == 3 and all(c[0] == 140 for c in calls), calls
    assert stats["n_applications"] == 0 and stats["n_launches"] <= 3 * len(calls), stats
    assert _compare_paths(n, on, off, obs, variance=False)


def _tagged(res):
    return {k: v for k, v in res.get_tagged_results().items()}


@pytest.mark.parametrize("which", ["dephasing", "three_level", "below_threshold"])
def test_backend_other_runs_keep_the_per_time_path(which, monkeypatch):
    """Master-equation runs, multi-level registers and runs below the threshold never call ``observe_many`` and give
    what they give with the path switched off."""
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipConfig

    obs = _observables()
    min_times = 1
    if which == "dephasing":
        inputs = _inputs(4)
        cfg = QutipConfig(default_evaluation_times=np.linspace(0.1, 1.0, 10).tolist(), observables=obs,
                          noise_model=NoiseModel(dephasing_rate=0.3))
    elif which == "three_level":
        from helpers import load_fixture
        from test_host_logic import _inputs_from_problem

        prob, extra = load_fixture("noises_all_0.npz")
        meas = extra["aux"]["meas_basis"]
        inputs = _inputs_from_problem(prob, measurement=meas if meas != "digital" else None)
        cfg = QutipConfig(default_evaluation_times=np.linspace(0.1, 1.0, 10).tolist(), sampling_rate=0.1,
                          observables=_observables(one_state="r"))
    else:
        inputs = _inputs(4)
        cfg = QutipConfig(default_evaluation_times=np.linspace(0.05, 1.0, 20).tolist(), observables=obs)
        min_times = 21
    off, stats_off = _run(inputs, cfg, None, monkeypatch, seed=3)
    calls = _count_observe_many(monkeypatch)
    on, stats = _run(inputs, cfg, min_times, monkeypatch, seed=3)
    assert calls == []
    assert stats["n_launches"] == stats_off["n_launches"] and stats["n_applications"] == stats_off["n_applications"]
    a, b = _tagged(on), _tagged(off)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k], dtype=float), np.asarray(b[k], dtype=float)), k

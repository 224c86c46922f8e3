"""GPU: ``ryd_general_observe`` (k_gen_observe.hpp: k_gen_obs_pairs, k_obs_energy, k_gen_obs_stage_cols,
k_gen_obs_trace) called directly through ``GeneralEngine.observe`` and pinned to the longdouble host references of
tests/observe_ref.py and tests/general_observe_ref.py, on XY registers (d = 2), the 3-level "all" basis and a 4-level
leakage register, with complex drives.

States are random and unphysical on purpose (kets not normalised, a different one per batch entry; density matrices
exactly Hermitian random mixtures with trace != 1).  Covered: every ``one`` digit, every ``what`` subset (slots not
asked for exactly 0), t = 0 / interior / on a knot / last knot, every application kernel (k_gen_apply_fused with and
without the vector in LDS, k_gen_apply_sites, k_gen_apply, CSR terms), a fresh handle whose first call is ``observe``,
density matrices on a ket handle (D = 16 .. 243, one chunk and many), ``vec(rho)`` on a RYD_GENERAL_DENSITY handle, exact
basis-state sweeps, and the refusals of the two-level entry points on a general handle.

Tolerances are derived in the reference files (worst-case summation bounds in the unit roundoff 2^-53 plus the
project's 1e-11 bar of one generator application); nothing is fitted to what the kernels give.  Every case prints
``error / tolerance`` before it asserts.  Worst ratios seen on an MI355X, per kernel:

    k_gen_obs_pairs        0.082     (the 16-term bound of a 4-atom XY register; below 0.02 from 3^6 amplitudes on)
    k_obs_energy           1.0e-5    (<H>; <H^2> 8.0e-6)
    k_gen_obs_trace        1.0e-5    (Tr(H rho); Tr(H^2 rho) 1.1e-5; both on a basis state |1><1|)
    apply_generator        3.2e-5    (batched GeneralEngine.apply_generator against the 1e-11 bar)
"""
import os
import sys

import numpy as np
import pytest

from helpers import rand_state, three_level_problem, xy_problem
from general_observe_ref import digits_of, ref_pairs_d, tol_energy_dm_general
from observe_ref import ket_probabilities, ref_energy_dm, ref_energy_ket, tol_energy_ket, tol_sum

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_general_fixtures as G  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.6, 1.9)  # batch entries 1 and 2 are not normalised


def _report(kernel, what, err, tol):
    """Print error / tolerance of one output (max over its elements), then say whether it holds."""
    err, tol = np.asarray(err, dtype=float), np.asarray(tol, dtype=float)
    ok = bool(np.all(err <= tol))
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0, tol, np.finfo(float).tiny))))
    print(f"RATIO {kernel:16s} {what:44s} err {float(np.max(err)):.3e} tol {float(np.max(tol)):.3e} ratio {ratio:.3e}")
    return ok


_PROBLEMS = {}


def _problem(kind, n):
    """(problem, oracle Hamiltonian, local dimension, last knot in us) - built once per module run."""
    from oracle import qutip_path as qp
    from pulser_amd import problem as P

    key = (kind, n)
    if key not in _PROBLEMS:
        if kind == "xy":
            prob, _, t_end = xy_problem(n)
        elif kind == "l3":
            prob, _, t_end = three_level_problem(n)
        elif kind == "leak":  # 4-level: the builder of the leak6 fixture on a chain
            prob = G.multilevel_problem(P.register_coords(P.square_rect(1, n), 6.0), 121, 6, leakage=True, local=(1, n - 1))
            t_end = 0.12
        elif kind == "xy_me":  # density cases: any atom number
            prob = G.xy_problem(P.register_coords(P.square_rect(1, n), 5.0), 121, 50 + n)
            t_end = 0.12
        else:  # "l3_me"
            prob = G.multilevel_problem(P.register_coords(P.square_rect(1, n), 6.0), 121, 60 + n, local=(0, n - 1))
            t_end = 0.12
        _PROBLEMS[key] = (prob, qp.build_hamiltonian(prob), len(prob["eigenbasis"]), float(t_end))
    return _PROBLEMS[key]


def _times(t_end):
    """t = 0, between two knots, on a knot, the last knot."""
    return [0.0, round(0.37 * t_end, 3) + 0.0004, round(0.5 * t_end, 3), t_end]


def _engine(prob, batch=1, mesolve=False, matrix_free=True):
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general

    tables = lower_general(prob, mesolve=mesolve, matrix_free=matrix_free)
    assert (tables.free is not None) == matrix_free
    return GeneralEngine(tables, batch=batch)


def _dev(eng, host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).to(eng.device)


def _ket(D, b, seed=0):
    return SCALES[b % 3] * rand_state(D, 7000 + 13 * seed + b)


def _mixture(D, b):
    """Random Hermitian mixture sum_j w_j |x_j><x_j| of 3 random kets, exactly Hermitian, trace != 1."""
    rho = np.zeros((D, D), complex)
    for j, w in enumerate((0.5, 0.3, 0.45 * SCALES[b % 3])):
        x = rand_state(D, 9000 + 10 * b + j + D)
        rho += w * np.outer(x, x.conj())
    return 0.5 * (rho + rho.conj().T)


def _check_pairs(got, b, ref, D, tag, occupation=True, correlation=True):
    norm, occ, corr, (s_norm, s_occ, s_corr) = ref
    ok = _report("k_gen_obs_pairs", f"{tag} norm2", abs(got["norm2"][b] - norm), tol_sum(D, s_norm))
    if occupation:
        ok &= _report("k_gen_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][b] - occ), tol_sum(D, s_occ))
    if correlation:
        ok &= _report("k_gen_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][b] - corr), tol_sum(D, s_corr))
    return ok


def _check_ket_energy(got, b, ref, x, tag):
    e1, e2, s_abs, w = ref
    tol1, tol2 = tol_energy_ket(x, w, s_abs)
    ok = _report("k_obs_energy", f"{tag} <H>", abs(got["energy"][b] - e1), tol1)
    return ok & _report("k_obs_energy", f"{tag} <H^2>", abs(got["energy2"][b] - e2), tol2)


def _check_dm_energy(got, b, ham, t, rho, tag):
    e1, e2, s_abs = ref_energy_dm(ham, t, rho)
    tol1, tol2 = tol_energy_dm_general(ham, t, rho, s_abs)
    ok = _report("k_gen_obs_trace", f"{tag} Tr(H rho)", abs(got["energy"][b] - e1), tol1)
    return ok & _report("k_gen_obs_trace", f"{tag} Tr(H^2 rho)", abs(got["energy2"][b] - e2), tol2)


KET_CASES = [("xy", 4), ("xy", 8), ("xy", 12), ("xy", 14), ("l3", 4), ("l3", 6), ("l3", 8), ("l3", 9), ("leak", 5)]


# ---------------------------------------------------------------------------------------------------------------------
# kets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind,n", KET_CASES)
def test_observe_kets(kind, n, B):
    """All five outputs of every batch entry, every ``one`` digit, four times; ``observe`` is the first call on a fresh
    handle (no solve before it).  Up to 3^8 amplitudes k_gen_apply_fused stages the vector in LDS, XY on 14 atoms and
    3-level on 9 gather from L2: the kernel of the application is asserted (``stats()["apply_path"]``)."""
    prob, ham, d, t_end = _problem(kind, n)
    D = d**n
    xs = np.stack([_ket(D, b, seed=n) for b in range(B)])
    pair_ref = {(b, one): ref_pairs_d(ket_probabilities(xs[b]), n, d, one) for b in range(B) for one in range(d)}
    ok = True
    with _engine(prob, batch=B) as eng:
        assert eng.dim == D and eng.local_dim == d and eng.n == n
        state = _dev(eng, xs)
        for t in _times(t_end):
            e_ref = [ref_energy_ket(ham, t, xs[b]) for b in range(B)]
            for one in range(d):
                got = eng.observe(state, t, one=one)
                path = eng.stats()["apply_path"]
                # (host_general.hpp: the vector is staged when the site tables + 16 B per amplitude fit 150 KiB; the
                # tables of these registers are a few KiB, so 3^8 = 6561 amplitudes - 103 KiB - still fit)
                assert path == ("fused" if 16 * D > 150 * 1024 else "fused_lds"), path
                for b in range(B):
                    tag = f"{kind}{n} B={B} b={b} one={one} t={t:.4f}"
                    ok &= _check_pairs(got, b, pair_ref[(b, one)], D, tag)
                    ok &= _check_ket_energy(got, b, e_ref[b], xs[b], tag)
    assert ok


@pytest.mark.parametrize("kind,n", [("xy", 8), ("l3", 6), ("leak", 5), ("l3", 9)])
def test_observe_kets_on_every_application_path(kind, n):
    """The energy moments go through whichever generator application is active: the padded site tables (default), the
    round-3 site kernel, the term-by-term kernel, each also with the multi-launch hook set, and explicit CSR terms; which
    kernel served the application is read back from the handle's statistics."""
    prob, ham, d, t_end = _problem(kind, n)
    D, B = d**n, 3
    t = _times(t_end)[1]
    xs = np.stack([_ket(D, b, seed=n + 1) for b in range(B)])
    e_ref = [ref_energy_ket(ham, t, xs[b]) for b in range(B)]
    p_ref = [ref_pairs_d(ket_probabilities(xs[b]), n, d, 1) for b in range(B)]
    ok = True
    fused = "fused_lds" if D <= 4096 else "fused"  # (the vector of 3^9 amplitudes does not fit the LDS)
    legs = [("fused", True, {}, fused), ("fused multi", True, {"force_multi_launch": True}, fused),
            ("sites", True, {"force_multi_launch": True, "no_fused": True}, "sites"),
            ("terms", True, {"force_multi_launch": False, "no_sites": True}, "terms"),
            ("terms multi", True, {"force_multi_launch": True, "no_sites": True}, "terms")]
    if D <= 4096:
        legs.append(("csr", False, {}, "terms"))
    for name, free, path, kernel in legs:
        with _engine(prob, batch=B, matrix_free=free) as eng:
            if path:
                eng.set_path(**{"force_multi_launch": False, **path})
            got = eng.observe(_dev(eng, xs), t, one=1)
            assert eng.stats()["n_applications"] == 1
            assert eng.stats()["apply_path"] == kernel, (name, eng.stats()["apply_path"])  # the kernel that ran
        for b in range(B):
            ok &= _check_pairs(got, b, p_ref[b], D, f"{kind}{n} [{name}] b={b}")
            ok &= _check_ket_energy(got, b, e_ref[b], xs[b], f"{kind}{n} [{name}] b={b}")
    assert ok


def test_apply_generator_takes_the_batch():
    """``GeneralEngine.apply_generator`` on (batch, dim) and on (1, dim) of a batched engine: -i H x per entry at the
    project's 1e-11 bar of one application."""
    prob, ham, d, t_end = _problem("l3", 4)
    D, B, t = d**4, 3, 0.0617
    xs = np.stack([_ket(D, b) for b in range(B)])
    with _engine(prob, batch=B) as eng:
        full = eng.apply_generator(_dev(eng, xs), t).cpu().numpy()
        one = eng.apply_generator(_dev(eng, xs[2:3]), t).cpu().numpy()
        with pytest.raises(ValueError):
            eng.apply_generator(_dev(eng, xs[:2]), t)
    assert full.shape == (B, D) and one.shape == (1, D)
    ok = True
    for b in range(B):
        want = -1j * np.asarray(ham.apply(t, xs[b]))
        ok &= _report("k_gen_apply_fused", f"apply_generator b={b}", np.max(np.abs(full[b] - want)),
                      1e-11 * max(1.0, np.max(np.abs(want))))
    assert ok and np.array_equal(one[0], full[2])


# ---------------------------------------------------------------------------------------------------------------------
# density matrices on a ket handle (RYD_OBS_DENSITY)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind,n", [("xy_me", 4), ("xy_me", 5), ("xy_me", 6), ("l3_me", 3), ("l3_me", 4), ("l3_me", 5)])
def test_observe_density_matrices_on_a_ket_handle(kind, n, B):
    """Tr(H rho), Tr(H^2 rho) through H on the columns of rho in one chunk (two applications per call); D = 243 is not
    a multiple of the 32 x 32 staging tile.  The default lowering at these sizes is CSR: both term kinds are run."""
    prob, ham, d, t_end = _problem(kind, n)
    D = d**n
    rhos = np.stack([_mixture(D, b) for b in range(B)])
    pair_ref = {(b, one): ref_pairs_d(np.real(np.diag(rhos[b])), n, d, one) for b in range(B) for one in range(d)}
    ok = True
    for free in (True, False):
        with _engine(prob, batch=B, matrix_free=free) as eng:
            state = _dev(eng, rhos)
            for t in _times(t_end):
                for one in range(d):
                    before = eng.stats()["n_applications"]
                    got = eng.observe(state, t, one=one, density=True)
                    assert eng.stats()["n_applications"] - before == 2
                    for b in range(B):
                        tag = f"dm {kind}{n} free={free} B={B} b={b} one={one} t={t:.4f}"
                        ok &= _check_pairs(got, b, pair_ref[(b, one)], D, tag)
                        ok &= _check_dm_energy(got, b, ham, t, rhos[b], tag)
    assert ok


@pytest.mark.parametrize("kind,n", [("l3_me", 4), ("xy_me", 5)])
def test_observe_density_matrices_in_column_chunks(kind, n):
    """The chunked path (``observe_small_chunks``: 5 columns per chunk, the last chunk partly filled) gives the values
    of the one-chunk path within the same tolerance, with two applications per chunk."""
    prob, ham, d, t_end = _problem(kind, n)
    D, B = d**n, 2
    t = _times(t_end)[1]
    rhos = np.stack([_mixture(D, b) for b in range(B)])
    n_chunks = -(-D // 5)
    assert D % 5 != 0 and n_chunks > 1
    ok = True
    with _engine(prob, batch=B) as eng:
        eng.set_path(False, observe_small_chunks=True)
        got = eng.observe(_dev(eng, rhos), t, one=1, density=True)
        assert eng.stats()["n_applications"] == 2 * n_chunks
        eng.set_path(False)
        whole = eng.observe(_dev(eng, rhos), t, one=1, density=True)
        assert eng.stats()["n_applications"] == 2 * n_chunks + 2
    for b in range(B):
        tag = f"dm chunks {kind}{n} b={b}"
        ok &= _check_pairs(got, b, ref_pairs_d(np.real(np.diag(rhos[b])), n, d, 1), D, tag)
        ok &= _check_dm_energy(got, b, ham, t, rhos[b], tag)
        ok &= _check_dm_energy(whole, b, ham, t, rhos[b], tag + " (one chunk)")
    assert ok


def test_observe_density_matrix_is_read_as_stored():
    """rho is not assumed Hermitian and its columns (not its rows) meet H: for a non-Hermitian ``rho = |x><y|`` the
    reference Tr(H rho) = <y|H|x> is matched, and it differs from the row version Tr(H^T rho) by far more than the bar."""
    prob, ham, d, t_end = _problem("l3_me", 3)
    D, t = d**3, _times(t_end)[1]
    x, y = rand_state(D, 1), rand_state(D, 2)
    rho = np.outer(x, y.conj())[None]
    with _engine(prob) as eng:
        got = eng.observe(_dev(eng, rho), t, density=True)
    e1, e2, s_abs = ref_energy_dm(ham, t, rho[0])
    tol1, tol2 = tol_energy_dm_general(ham, t, rho[0], s_abs)
    H = ham.matrix(t).toarray()
    assert abs(np.sum(H * rho[0]).real - float(e1)) > 1e3 * tol1
    assert _check_dm_energy(got, 0, ham, t, rho[0], "non-Hermitian |x><y|")


# ---------------------------------------------------------------------------------------------------------------------
# RYD_GENERAL_DENSITY handles: vec(rho)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("xy_me", 5), ("l3_me", 4)])
def test_observe_on_a_density_handle(kind, n):
    from pulser_amd._lib import RydError

    prob, ham, d, t_end = _problem(kind, n)
    D, B = d**n, 2
    rhos = np.stack([_mixture(D, b) for b in range(B)])
    ok = True
    with _engine(prob, batch=B, mesolve=True) as eng:
        assert eng.is_density and eng.dim == D * D
        state = _dev(eng, rhos.reshape(B, D * D))
        for one in range(d):
            got = eng.observe(state, 0.03, one=one, energy=False)
            for b in range(B):
                ok &= _check_pairs(got, b, ref_pairs_d(np.real(np.diag(rhos[b])), n, d, one), D,
                                   f"vec(rho) {kind}{n} b={b} one={one}")
                assert got["energy"][b] == 0.0 and got["energy2"][b] == 0.0
        with pytest.raises(RydError) as exc:
            eng.observe(state, 0.03)
        assert exc.value.code == -3 and "Liouvillian" in str(exc.value)  # RYD_ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            eng.observe(_dev(eng, rhos), 0.03, energy=False, density=True)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# `what` subsets: what was not asked for is exactly 0, the norm comes with either pair output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ket", "dm"])
@pytest.mark.parametrize("mask", range(8))
def test_observe_what_subsets(mask, kind):
    occ, cor, en = bool(mask & 1), bool(mask & 2), bool(mask & 4)
    prob, ham, d, t_end = _problem("l3", 4) if kind == "ket" else _problem("l3_me", 3)
    n = 4 if kind == "ket" else 3
    D, B, t = d**n, 3, _times(t_end)[1]
    states = np.stack([(_ket if kind == "ket" else _mixture)(D, b) for b in range(B)])
    with _engine(prob, batch=B) as eng:
        got = eng.observe(_dev(eng, states), t, one=2, occupation=occ, correlation=cor, energy=en, density=kind == "dm")
    ok = True
    for b in range(B):
        tag = f"{kind} b={b} what={mask}"
        p = ket_probabilities(states[b]) if kind == "ket" else np.real(np.diag(states[b]))
        if occ or cor:
            ok &= _check_pairs(got, b, ref_pairs_d(p, n, d, 2), D, tag, occupation=occ, correlation=cor)
            assert got["norm2"][b] != 0.0
        else:
            assert got["norm2"][b] == 0.0
        if not occ:
            assert np.all(got["occupation"][b] == 0.0), got["occupation"][b]
        if not cor:
            assert np.all(got["correlation"][b] == 0.0), got["correlation"][b]
        if not en:
            assert got["energy"][b] == 0.0 and got["energy2"][b] == 0.0
        elif kind == "ket":
            ok &= _check_ket_energy(got, b, ref_energy_ket(ham, t, states[b]), states[b], tag)
        else:
            ok &= _check_dm_energy(got, b, ham, t, states[b], tag)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# exact basis-state sweeps: single-term sums, equality
# ---------------------------------------------------------------------------------------------------------------------
def _assert_basis_outputs(got, b, a, dg, one):
    bits = (dg[a] == one).astype(float)
    assert got["norm2"][b] == 1.0, (a, got["norm2"][b])
    assert np.array_equal(got["occupation"][b], bits), (a, one, got["occupation"][b])
    assert np.array_equal(got["correlation"][b], np.outer(bits, bits)), (a, one, got["correlation"][b])


@pytest.mark.parametrize("kind,n", [("xy", 4), ("l3", 4), ("leak", 5), ("l3", 9)])
def test_observe_basis_kets_exactly(kind, n):
    """|a> with amplitude exactly 1, batches of 3 different basis states per call, every ``one``: a mirrored digit order,
    an ignored ``one`` or a dropped batch offset cannot hide under a tolerance.  3^9: indices around the 2048-entry
    chunks of k_gen_obs_pairs and the last one."""
    prob, _, d, _ = _problem(kind, n)
    D, B = d**n, 3
    dg = digits_of(n, d)
    pick = [0, 1, 2, 2047, 2048, 2049, 4095, 4096, 4097, D // 3, D // 2, D - 3, D - 2, D - 1]
    idx = list(range(D)) if D <= 256 else sorted({a for a in pick if a < D})
    idx = idx[len(idx) % B:]  # (keeps the last indices)
    with _engine(prob, batch=B) as eng:
        for i in range(0, len(idx), B):
            xs = np.zeros((B, D), complex)
            for b, a in enumerate(idx[i:i + B]):
                xs[b, a] = 1.0
            state = _dev(eng, xs)
            for one in range(d):
                got = eng.observe(state, 0.0, one=one, energy=False)
                for b, a in enumerate(idx[i:i + B]):
                    _assert_basis_outputs(got, b, a, dg, one)


def test_observe_basis_density_matrices_exactly():
    """rho = |a><a| for every a of a 3-level register of 3 atoms: pair sums exact, the energy moments are H_aa and
    (H^2)_aa alone."""
    n = 3
    prob, ham, d, t_end = _problem("l3_me", n)
    D, B, t = d**n, 3, _times(t_end)[2]
    dg = digits_of(n, d)
    ok = True
    with _engine(prob, batch=B) as eng:
        for i in range(0, D, B):
            rhos = np.zeros((B, D, D), complex)
            for b in range(B):
                rhos[b, i + b, i + b] = 1.0
            for one in range(d):
                got = eng.observe(_dev(eng, rhos), t, one=one, density=True)
                for b in range(B):
                    _assert_basis_outputs(got, b, i + b, dg, one)
                    if one == 1:
                        ok &= _check_dm_energy(got, b, ham, t, rhos[b], f"|{i + b}><{i + b}|")
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# argument checks and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_observe_checks_its_arguments():
    import torch
    from pulser_amd import _lib

    prob, _, d, _ = _problem("l3", 4)
    D = d**4
    with _engine(prob, batch=2) as eng:
        good = _dev(eng, np.stack([_ket(D, 0), _ket(D, 1)]))
        for bad in (good[:1], good.to(torch.complex64), good.cpu(), good[:, :-1], good.t().contiguous().t()):
            with pytest.raises(ValueError):
                eng.observe(bad, 0.0)
        with pytest.raises(ValueError):
            eng.observe(good, 0.0, one=3)
        with pytest.raises(ValueError):
            eng.observe(good, 0.0, density=True)  # a ket where a [B, D, D] matrix is expected
        out = torch.empty((2, 4 * 4 + 4 + 3), dtype=torch.float64, device=eng.device)
        lib = eng.lib
        for args in ((3, 5, 0), (2, 4, 0), (5, 4, 0), (3, 4, 3), (3, 4, -1)):  # local_dim, n_atoms, one_digit
            rc = lib.ryd_general_observe(eng._h, good.data_ptr(), 0.0, 3, *args, out.data_ptr(), eng._stream())
            assert rc == -1, (args, rc)  # RYD_ERR_INVALID
        assert eng.observe(good, 0.0)["norm2"][1] == pytest.approx(0.36, rel=1e-12)
        del _lib


def test_two_level_entry_points_refuse_a_general_handle():
    """``ryd_observe`` keeps its refusal; ``ryd_probabilities``, ``ryd_occupations``, ``ryd_ket_to_dm`` and
    ``ryd_outer_accumulate`` (which read the atom number of a two-level handle) gained the same one."""
    import torch

    prob, _, d, _ = _problem("xy", 4)
    D = d**4
    with _engine(prob) as eng:
        lib, h, st = eng.lib, eng._h, eng._stream()
        x = _dev(eng, _ket(D, 0)[None])
        big = torch.zeros((D, D), dtype=torch.complex128, device=eng.device)
        w = torch.zeros((1, D * D), dtype=torch.float64, device=eng.device)
        calls = {
            "ryd_observe": lambda: lib.ryd_observe(h, x.data_ptr(), 0.0, 7, w.data_ptr(), st),
            "ryd_probabilities": lambda: lib.ryd_probabilities(h, x.data_ptr(), w.data_ptr(), 0, st),
            "ryd_occupations": lambda: lib.ryd_occupations(h, x.data_ptr(), w.data_ptr(), st),
            "ryd_ket_to_dm": lambda: lib.ryd_ket_to_dm(h, x.data_ptr(), big.data_ptr(), st),
            "ryd_outer_accumulate": lambda: lib.ryd_outer_accumulate(h, x.data_ptr(), None, big.data_ptr(), st),
        }
        for name, call in calls.items():
            assert call() == -1, name  # RYD_ERR_INVALID
            assert "not available on a general-path handle" in lib.ryd_last_error().decode(), name
        torch.cuda.synchronize()
        assert float(w.abs().sum()) == 0.0 and float(big.abs().sum()) == 0.0  # nothing was launched

"""GPU: ``ryd_observe_density_many`` (k_obs_pairs on the diagonals, k_eval_coefs_many, k_obs_energy_dm_many) - the
occupations, correlations and energy moments of the density matrices of every evaluation time in one call - called
directly through ``Engine.observe_density_many`` and pinned to the longdouble host reference of tests/observe_ref.py
(``ref_pairs``, ``ref_energy_dm``), and its use by ``QutipBackendV2`` for two-level master-equation runs.

Matrices are seeded random complex matrices WITHOUT any symmetry (rho is read as stored, so a kernel that read the
transposed element or assumed a Hermitian matrix fails) with a random positive trace; problems have per-atom amplitude,
detuning and a non-zero phase, every entry of a batched handle has its own problem (entry 1 with a bad atom).  The
atom counts sit on the edges of the row pieces of k_obs_energy_dm_many: rows shorter than one 128-byte piece (1, 2
atoms), one piece and no higher bit (3), the first higher bit (4), the first pair of higher bits (5: 32 rows, one
per 8-lane group of the workgroup), a second and an eighth sweep of the workgroup over the rows (6, 8), and 11 atoms:
37 pieces and 67 masks per row, 8 workgroups per state, 64 MiB per matrix.  Times: 0, interior, exactly a knot, the
last knot, repeated, unsorted.

Tolerances are the derived ones of tests/observe_ref.py, unchanged: ``tol_sum(D, S_abs)`` for the pair sums and
``tol_energy_dm(n, S_abs)`` for the moments (its m = D (1 + N + N (N - 1) / 2) is exactly the number of elements this
kernel adds); nothing is fitted.  The backend cases compare the one-call path with the per-time path within the sum
of the two paths' bounds, evaluated on the normalised matrices of a third run that carries a ``StateResult`` (for the
noisy run: on the trajectory mean that run aggregates), plus 4 u |value| for the two normalisations.  Every case
prints ``error / tolerance`` before it asserts.  Worst ratios seen on an MI355X:

    k_obs_pairs             0.10      (the 2-term trace of a 1-atom matrix)
    k_obs_energy_dm_many    6.2e-05
    against per-time ``Engine.observe(density=True)``   pair sums identical; <H> 1.1e-05, <H^2> 8.4e-06 of both bounds
    backend, both paths     occupation 0.074, correlation 0.074, <H> 2.7e-05, <H^2> 2.4e-05
"""
import itertools

import numpy as np
import pytest

from observe_ref import U53, ref_energy_dm, ref_pairs, tol_energy_dm, tol_sum
from test_gpu_observe_many import (SCALES, T_KNOT, TIMES, _dev, _engine, _ham, _observables, _problems, _Reads,
                                   _report, _run, _tagged)

pytestmark = pytest.mark.gpu


def _rhos(n, T, B, seed=0):
    """[T, B, D, D]: a different random complex matrix for every (time, entry) - no symmetry, complex diagonal, one
    negative diagonal element from 2 atoms on - with a random positive trace of about SCALES[(i + b) % 3]."""
    D = 2**n
    rng = np.random.default_rng(7000 * n + 10 * T + B + seed)
    out = (rng.normal(size=(T, B, D, D)) + 1j * rng.normal(size=(T, B, D, D))) / D
    for i, b in itertools.product(range(T), range(B)):
        w = SCALES[(i + b) % 3] * rng.uniform(0.5, 1.5, D) / D
        if D >= 4:
            w[1] *= -0.1
        out[i, b][np.diag_indices(D)] = w + 1j * out[i, b][np.diag_indices(D)].imag
    return out


def _check_state(got, i, b, rho, ham, t, n, tag, occupation=True, correlation=True, energy=True):
    """Every requested output of matrix (i, b) against the longdouble reference; the trace is always checked."""
    D = 2**n
    norm, occ, corr, (s_norm, s_occ, s_corr) = ref_pairs(np.real(np.diag(rho)), n)
    assert norm > 0
    ok = _report("k_obs_pairs", f"{tag} trace", abs(got["norm2"][i, b] - norm), tol_sum(D, s_norm))
    if occupation:
        ok &= _report("k_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][i, b] - occ), tol_sum(D, s_occ))
    if correlation:
        ok &= _report("k_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][i, b] - corr), tol_sum(D, s_corr))
    if energy:
        e1, e2, s_abs = ref_energy_dm(ham, t, rho)
        tol1, tol2 = tol_energy_dm(n, s_abs)
        ok &= _report("k_obs_energy_dm_many", f"{tag} Tr(H rho)", abs(got["energy"][i, b] - e1), tol1)
        ok &= _report("k_obs_energy_dm_many", f"{tag} Tr(H^2 rho)", abs(got["energy2"][i, b] - e2), tol2)
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# direct: atom counts on the edges of the row pieces x times x batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 8])
def test_observe_density_many_batched_handle(n, T, B):
    """A handle of batch B, entry b with problem b: a dropped batch offset in the coefficient table or in e0 shows (entry
    1 has a bad atom, every entry its own register).  First call on a fresh handle."""
    times = TIMES[T]
    rhos = _rhos(n, T, B)
    with _engine(_problems(n, B)) as eng:
        got = eng.observe_density_many(_dev(eng, rhos), times)
        stats = eng.stats()
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    assert got["norm2"].shape == (T, B) and got["occupation"].shape == (T, B, n)
    assert got["correlation"].shape == (T, B, n, n) and got["energy"].shape == got["energy2"].shape == (T, B)
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check_state(got, i, b, rhos[i, b], _ham(n, B, b), times[i], n, f"n={n} T={T} i={i} b={b} t={times[i]}")
    assert ok


def test_observe_density_many_11_atoms():
    """D^2 is 64 MiB per matrix; 1 + 11 + 55 = 67 masks per row (more than the lanes of a wave) in 1 + 8 + 28 = 37
    pieces; 8 workgroups per state."""
    n, T = 11, 2
    times = TIMES[T]
    rhos = _rhos(n, T, 1)
    with _engine(_problems(n, 1)) as eng:
        got = eng.observe_density_many(_dev(eng, rhos), times)
        stats = eng.stats()
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    ok = True
    for i in range(T):
        ok &= _check_state(got, i, 0, rhos[i, 0], _ham(n, 1, 0), times[i], n, f"n={n} i={i} t={times[i]}")
    assert ok


@pytest.mark.parametrize("mode", ["sesolve", "mesolve"])
def test_observe_density_many_one_problem_serves_every_entry(mode):
    """B = 3 matrices per time on a handle of batch 1 - a sesolve handle and a mesolve handle of the same problem: both
    within the bounds, and the same kernels on the same tables give the same pair sums bit for bit."""
    n, B, T = 4, 3, 2
    times = TIMES[T]
    rhos = _rhos(n, T, B)
    with _engine(_problems(n, 1), mode=mode) as eng:
        got = eng.observe_density_many(_dev(eng, rhos), times)
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check_state(got, i, b, rhos[i, b], _ham(n, 1, 0), times[i], n, f"shared [{mode}] i={i} b={b}")
    assert ok
    if mode == "mesolve":
        with _engine(_problems(n, 1)) as eng:
            ket = eng.observe_density_many(_dev(eng, rhos), times)
        for key in ("norm2", "occupation", "correlation"):
            assert np.array_equal(got[key], ket[key]), key
        for i, b in itertools.product(range(T), range(B)):
            _, _, s_abs = ref_energy_dm(_ham(n, 1, 0), times[i], rhos[i, b])
            tol1, tol2 = tol_energy_dm(n, s_abs)
            assert abs(got["energy"][i, b] - ket["energy"][i, b]) <= 2 * tol1
            assert abs(got["energy2"][i, b] - ket["energy2"][i, b]) <= 2 * tol2


def test_observe_density_many_batch_mismatch_is_invalid():
    from pulser_amd._lib import RydError

    n = 3
    with _engine(_problems(n, 2)) as eng:
        with pytest.raises(RydError) as err:
            eng.observe_density_many(_dev(eng, _rhos(n, 2, 3)), TIMES[2])
    assert err.value.code == -1, err.value  # RYD_ERR_INVALID


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [1, 3, 5, 8])
def test_observe_density_many_against_per_time_observe(n, B):
    """State by state against ``ryd_observe(..., RYD_OBS_DENSITY)``: one workgroup per state runs the same pair kernel
    (a matrix of up to 11 atoms is one chunk of diagonal elements: every slot receives one atomicAdd), so the pair sums
    agree bit for bit; the energy moments come from another kernel with another summation order and agree within the
    sum of the two calls' ``tol_energy_dm``."""
    T = 4
    times = TIMES[7][:T]
    rhos = _rhos(n, T, B)
    with _engine(_problems(n, B)) as eng:
        dev = _dev(eng, rhos)
        got = eng.observe_density_many(dev, times)
        single = [eng.observe(dev[i], times[i], density=True) for i in range(T)]
    ok = True
    for i, key in itertools.product(range(T), ("occupation", "correlation", "norm2")):
        assert np.array_equal(got[key][i], single[i][key]), (i, key, got[key][i], single[i][key])
    for i, b in itertools.product(range(T), range(B)):
        _, _, s_abs = ref_energy_dm(_ham(n, B, b), times[i], rhos[i, b])
        tol1, tol2 = tol_energy_dm(n, s_abs)
        ok &= _report("many vs per-time", f"n={n} i={i} b={b} Tr(H rho)",
                      abs(got["energy"][i, b] - single[i]["energy"][b]), 2 * tol1)
        ok &= _report("many vs per-time", f"n={n} i={i} b={b} Tr(H^2 rho)",
                      abs(got["energy2"][i, b] - single[i]["energy2"][b]), 2 * tol2)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# views and strides
# ---------------------------------------------------------------------------------------------------------------------
def test_observe_density_many_views_and_padded_strides():
    """``dev[:, 1:2]`` and ``dev[1::2]`` of a [T, 3, D, D] tensor observed in place, and both outer axes padded."""
    import torch

    n, T = 6, 7
    D = 2**n
    times = TIMES[T]
    rhos = _rhos(n, T, 3)
    ham = _ham(n, 1, 0)
    ok = True
    with _engine(_problems(n, 1)) as eng:
        dev = _dev(eng, rhos)
        got = eng.observe_density_many(dev[:, 1:2], times)
        assert got["norm2"].shape == (T, 1)
        for i in range(T):
            ok &= _check_state(got, i, 0, rhos[i, 1], ham, times[i], n, f"view [:, 1:2] i={i}")
        got = eng.observe_density_many(dev[1::2], times[1::2])
        assert got["norm2"].shape == (3, 3)
        for j, b in itertools.product(range(3), range(3)):
            ok &= _check_state(got, j, b, rhos[1 + 2 * j, b], ham, times[1 + 2 * j], n, f"view [1::2] j={j} b={b}")
        sb, st = D * D + 5, 3 * (D * D + 5) + 37
        pad = torch.full((T * st,), complex("nan"), dtype=torch.complex128, device=eng.device)
        view = pad.as_strided((T, 3, D, D), (st, sb, D, 1))
        view.copy_(dev)
        got = eng.observe_density_many(view, times)
        for i, b in itertools.product(range(T), range(3)):
            ok &= _check_state(got, i, b, rhos[i, b], ham, times[i], n, f"padded strides i={i} b={b}")
    assert ok


def test_observe_density_many_second_matrix_beyond_4_gib():
    """Two 5-atom matrices in one ``torch.empty`` allocation of 4 GiB + 16 KiB, the second one 2^28 elements = 2^32
    bytes after the first: the state offset is 64-bit.  Only the two matrices are written; nothing else is read."""
    import torch

    n = 5
    D = 2**n
    gap = 2**28
    times = [0.12345, T_KNOT]
    rhos = _rhos(n, 2, 1)
    ham = _ham(n, 1, 0)
    with _engine(_problems(n, 1)) as eng:
        big = torch.empty(gap + D * D, dtype=torch.complex128, device=eng.device)
        view = big.as_strided((2, 1, D, D), (gap, D * D, D, 1))
        view.copy_(_dev(eng, rhos))
        got = eng.observe_density_many(view, times)
        del view, big
    ok = True
    for i in range(2):
        ok &= _check_state(got, i, 0, rhos[i, 0], ham, times[i], n, f"offset {i * gap * 16} bytes")
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# `what` subsets, closed forms, refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occupation,correlation,energy", list(itertools.product([False, True], repeat=3)))
def test_observe_density_many_what_subsets(occupation, correlation, energy):
    """What was not asked for is exactly 0; the trace is always there (from the pair launch, or from the energy kernel
    of an energy-only call); at most 1 launch for pairs only, 2 for energy only, 3 for all."""
    n, B, T = 5, 3, 2
    times = TIMES[T]
    rhos = _rhos(n, T, B)
    with _engine(_problems(n, B)) as eng:
        got = eng.observe_density_many(_dev(eng, rhos), times, occupation=occupation, correlation=correlation,
                                       energy=energy)
        stats = eng.stats()
    assert stats["n_launches"] == (1 if occupation or correlation or not energy else 0) + (2 if energy else 0), stats
    assert stats["n_applications"] == 0, stats
    ok = True
    for i, b in itertools.product(range(T), range(B)):
        ok &= _check_state(got, i, b, rhos[i, b], _ham(n, B, b), times[i], n,
                           f"what={occupation:d}{correlation:d}{energy:d} i={i} b={b}", occupation=occupation,
                           correlation=correlation, energy=energy)
    if not occupation:
        assert np.all(got["occupation"] == 0.0)
    if not correlation:
        assert np.all(got["correlation"] == 0.0)
    if not energy:
        assert np.all(got["energy"] == 0.0) and np.all(got["energy2"] == 0.0)
    assert ok


def test_observe_density_many_basis_states_closed_forms():
    """rho = |a><a| for basis states of 4 atoms (element exactly 1): occupations, correlations and the trace are exact,
    <H> = E(a) = H_aa and <H^2> = E(a)^2 + sum_k |c_k|^2 = sum_b |H_ba|^2 of the oracle's dense H(t)."""
    n, t = 4, 0.12345
    D = 2**n
    idx = [0, 1, 5, 8, 10, D - 1]
    rhos = np.zeros((len(idx), 1, D, D), complex)
    for i, a in enumerate(idx):
        rhos[i, 0, a, a] = 1.0
    ham = _ham(n, 1, 0)
    H = np.asarray(ham.matrix(t).toarray())
    with _engine(_problems(n, 1)) as eng:
        got = eng.observe_density_many(_dev(eng, rhos), [t] * len(idx))
    ok = True
    for i, a in enumerate(idx):
        bits = np.array([1 - ((a >> (n - 1 - k)) & 1) for k in range(n)], dtype=float)
        assert got["norm2"][i, 0] == 1.0
        assert np.array_equal(got["occupation"][i, 0], bits), (a, got["occupation"][i, 0])
        assert np.array_equal(got["correlation"][i, 0], np.outer(bits, bits)), (a, got["correlation"][i, 0])
        _, _, s_abs = ref_energy_dm(ham, t, rhos[i, 0])
        tol1, tol2 = tol_energy_dm(n, s_abs)
        ok &= _report("k_obs_energy_dm_many", f"|{a}><{a}| E(a)", abs(got["energy"][i, 0] - H[a, a].real), tol1)
        ok &= _report("k_obs_energy_dm_many", f"|{a}><{a}| E(a)^2 + sum |c_k|^2",
                      abs(got["energy2"][i, 0] - np.sum(np.abs(H[:, a]) ** 2)), tol2)
    assert ok


def test_observe_density_many_single_elements_are_read_as_stored():
    """One stored element rho[r][c] = 1 at a time (3 atoms, every (r, c)): the call returns Re(H_cr) and Re((H^2)_cr) of
    the oracle's dense H(t) - the transposed element, a doubled or a dropped one cannot hide under a tolerance."""
    n, t = 3, 0.3
    D = 2**n
    rhos = np.zeros((D * D, 1, D, D), complex)
    for r, c in itertools.product(range(D), range(D)):
        rhos[r * D + c, 0, r, c] = 1.0
    ham = _ham(n, 1, 0)
    H = np.asarray(ham.matrix(t).toarray())
    H2 = H @ H
    with _engine(_problems(n, 1)) as eng:
        got = eng.observe_density_many(_dev(eng, rhos), [t] * (D * D))
    ok = True
    for r, c in itertools.product(range(D), range(D)):
        _, _, s_abs = ref_energy_dm(ham, t, rhos[r * D + c, 0])
        tol1, tol2 = tol_energy_dm(n, s_abs)
        assert got["norm2"][r * D + c, 0] == (1.0 if r == c else 0.0)
        ok &= bool(abs(got["energy"][r * D + c, 0] - H[c, r].real) <= tol1)
        ok &= bool(abs(got["energy2"][r * D + c, 0] - H2[c, r].real) <= tol2)
        if bin(r ^ c).count("1") > 2:
            assert got["energy"][r * D + c, 0] == 0.0 and got["energy2"][r * D + c, 0] == 0.0
    assert ok


def test_observe_density_many_refusals():
    """A general handle and strides below D^2 are RYD_ERR_INVALID, a Monte-Carlo handle and a handle with detuning
    terms RYD_ERR_UNSUPPORTED with a message naming ryd_observe; a set RYD_OBS_DENSITY bit is ignored; ``n_times = 0``
    is RYD_OK; the Python wrapper raises ``ValueError`` for what it can see."""
    import torch
    from dataclasses import replace

    from helpers import DEPOL_PAULIS, local_problem, three_level_problem
    from pulser_amd import _lib
    from pulser_amd.engine import Engine, GeneralEngine
    from pulser_amd.general import lower_general
    from pulser_amd.terms import DTERM_DTYPE, lower

    n = 3
    D = 2**n
    lib = _lib.load()
    times = np.array([0.1, 0.2])

    def call(eng, x, n_times=2, what=7, stride_t=D * D, stride_b=D * D):
        out = torch.full((2, 1, n * n + n + 3), 5.0, dtype=torch.float64, device=x.device)
        rc = lib.ryd_observe_density_many(eng._h, x.data_ptr(), n_times, 1, stride_t, stride_b, times.ctypes.data, what,
                                          out.data_ptr(), eng._stream())
        torch.cuda.synchronize()
        return rc, lib.ryd_last_error().decode(), out.cpu().numpy()

    with _engine(_problems(n, 1)) as eng:
        x = _dev(eng, _rhos(n, 2, 1))
        rc, _, plain = call(eng, x)
        assert rc == 0
        rc, _, flagged = call(eng, x, what=7 | 8)  # RYD_OBS_DENSITY is ignored
        assert rc == 0 and np.array_equal(flagged[..., :n * n + n + 1], plain[..., :n * n + n + 1])
        rc, _, untouched = call(eng, x, n_times=0)
        assert rc == 0 and np.all(untouched == 5.0)
        for kw in (dict(stride_t=D * D - 1), dict(stride_b=D * D - 1)):
            rc, msg, _ = call(eng, x, **kw)
            assert rc == -1 and "stride" in msg, (rc, msg)
        with pytest.raises(ValueError):
            eng.observe_density_many(x.to(torch.complex64), times)
        with pytest.raises(ValueError):
            eng.observe_density_many(x.cpu(), times)
        with pytest.raises(ValueError):
            eng.observe_density_many(x.reshape(2, 1, D * D), times)  # kets where matrices are expected
        with pytest.raises(ValueError):
            eng.observe_density_many(x.transpose(2, 3), times)       # the matrices must be row-major
        with pytest.raises(ValueError):
            eng.observe_density_many(torch.zeros((2, 1, D, 2 * D), dtype=torch.complex128, device=eng.device)[..., ::2], times)
        with pytest.raises(ValueError):
            eng.observe_density_many(x, times[:1])
        # extra detuning terms: the table of the same problem with one (zero-scale) term on atom 0
        tables = lower(_problems(n, 1))
        desc = np.array(tables.desc, copy=True)
        desc["extra"][0, 0] = 1
        with Engine(replace(tables, desc=desc, dterms=np.zeros(1, dtype=DTERM_DTYPE))) as de:
            rc, msg, _ = call(de, x)
            assert rc == -3 and "detuning" in msg and "ryd_observe" in msg, (rc, msg)
        ops = [(np.sqrt(3.0), "sigma_gr"), (np.sqrt(1.8), "sigma_rr")]
        with Engine(lower([local_problem(n, seed=3, collapse_ops=ops, paulis=DEPOL_PAULIS)]), mode="mcsolve") as mc:
            rc, msg, _ = call(mc, x)
            assert rc == -3 and "ryd_observe" in msg, (rc, msg)
    prob, _, _ = three_level_problem(4)
    with GeneralEngine(lower_general(prob, mesolve=False)) as ge:
        xg = torch.zeros((2, 1, ge.dim), dtype=torch.complex128, device=ge.device)
        rc = lib.ryd_observe_density_many(ge._h, xg.data_ptr(), 2, 1, ge.dim, ge.dim, times.ctypes.data, 7, xg.data_ptr(), 0)
        assert rc == -1 and "general" in lib.ryd_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend: two-level master-equation runs
# ---------------------------------------------------------------------------------------------------------------------
N_BACKEND = 5
FLOOR = 128


def _setup():
    """(inputs, oracle Hamiltonian) of the 5-atom anneal (the register and samples of
    test_gpu_backend_v2.test_device_side_observables_of_density_matrices, one row of atoms)."""
    from oracle import qutip_path as qp
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import single_global_channel

    if "v" not in _setup.__dict__:
        coords = P.register_coords(P.square_rect(1, N_BACKEND), _blockade())
        smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
        inputs = single_global_channel(coords, smp, P.C6_LEVEL70, extended=False)
        _setup.v = (inputs, qp.build_hamiltonian(P.make_ising_problem(coords, P.anneal_samples())))
    return _setup.v


def _blockade():
    from helpers import blockade_radius

    return blockade_radius()


def _count_calls(monkeypatch):
    """Shapes of the states handed to ``Engine.observe_density_many`` and to ``Engine.observe_many``."""
    from pulser_amd.engine import Engine

    dens, kets = [], []
    real_d, real_k = Engine.observe_density_many, Engine.observe_many

    def counted_d(self, states, times, **kw):
        dens.append(tuple(states.shape))
        return real_d(self, states, times, **kw)

    def counted_k(self, states, times, **kw):
        kets.append(tuple(states.shape))
        return real_k(self, states, times, **kw)

    monkeypatch.setattr(Engine, "observe_density_many", counted_d)
    monkeypatch.setattr(Engine, "observe_many", counted_k)
    return dens, kets


def _bounds(ham, n, t_us, rho):
    """Sum of the bounds of the two paths for the NORMALISED matrix ``rho`` (from a run that carries a StateResult):
    twice ``tol_sum`` / ``tol_energy_dm`` of tests/observe_ref.py on this state.  The caller adds 4 u |value| for the
    two normalisations (the per-time path divides the matrix on the host and the sums again, the one-call path once)."""
    D = 2**n
    _, occ, corr, (_, s_occ, s_corr) = ref_pairs(np.real(np.diag(rho)), n)
    e1, e2, s_abs = ref_energy_dm(ham, t_us, rho)
    tol1, tol2 = tol_energy_dm(n, s_abs)
    return 2 * tol_sum(D, s_occ), 2 * tol_sum(D, s_corr), 2 * tol1, 2 * tol2, (occ, corr, e1, e2)


def _compare_paths(on, off, obs, states, variance=True):
    """Every result of the one-call run against the per-time run within ``_bounds`` + 4 u |value|; ``states``: time ->
    normalised density matrix of the third run."""
    _, ham = _setup()
    n = N_BACKEND
    ok = True
    worst = np.zeros(4)
    times = off.get_result_times(obs[0])
    assert on.get_result_times(obs[0]) == times and len(times) == len(states)
    for t in times:
        b_occ, b_cor, t1, t2, _ = _bounds(ham, n, t * 3.1, states[t])
        v = [np.array(r.get_result(o, t), dtype=float) for r in (on, off) for o in obs[:4]]
        errs = [np.abs(v[j] - v[4 + j]) for j in range(4)]
        tols = [b + 4 * U53 * np.abs(v[4 + j]) for j, b in enumerate((b_occ, b_cor, t1, t2))]
        for j in range(4):
            ok &= bool(np.all(errs[j] <= tols[j]))
            worst[j] = max(worst[j], float(np.max(errs[j] / tols[j])))
        if variance:
            e1 = float(v[6])
            ok &= abs(on.get_result(obs[4], t) - off.get_result(obs[4], t)) <= float(tols[3]) + 2 * abs(e1) * float(tols[2])
    print("RATIO backend one-call vs per-time (occupation, correlation, <H>, <H^2>):", " ".join(f"{x:.3e}" for x in worst))
    return ok


def _third_run_states(inputs, cfg_kw, times, monkeypatch, seed=None):
    """time -> normalised density matrix, from a per-time run of the same configuration that carries a StateResult."""
    from pulser_amd.backend import QutipConfig, StateResult

    sr = StateResult()
    res, _ = _run(inputs, QutipConfig(default_evaluation_times=times, observables=[sr], **cfg_kw), None, monkeypatch, seed=seed)
    return {t: np.asarray(res.get_result(sr, t).to_qobj()) for t in res.get_result_times(sr)}


def test_backend_one_call_serves_a_master_equation_run_and_reads_no_state(monkeypatch):
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipConfig

    inputs, _ = _setup()
    D = 2**N_BACKEND
    times = np.linspace(0.01, 1.0, 140).tolist()
    obs = _observables()
    kw = dict(noise_model=NoiseModel(dephasing_rate=0.3))
    cfg = QutipConfig(default_evaluation_times=times, observables=obs, **kw)
    states = _third_run_states(inputs, kw, times, monkeypatch)
    assert all(s.shape == (D, D) for s in states.values())
    off, stats_off = _run(inputs, cfg, None, monkeypatch)
    assert stats_off["n_launches"] == 2 * len(times), stats_off
    reads = _Reads(monkeypatch)
    dens, kets = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 128, monkeypatch)
    assert stats["n_launches"] <= 3 and stats["n_applications"] == 0, stats
    assert dens == [(140, 1, D, D)] and kets == [] and reads.gets == [] and reads.bulk == 0, (dens, kets, reads.gets, reads.bulk)
    assert _compare_paths(on, off, obs, states)


def test_backend_states_that_are_read_are_the_same_states(monkeypatch):
    """``StateResult`` at two times and a callback that reads the state at a third: exactly those three snapshots are
    copied, and they equal the per-time run's bit for bit (``_DeferredRydState`` divides by the trace norm as the
    eager construction does)."""
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipConfig, StateResult

    inputs, _ = _setup()
    times = np.linspace(0.01, 1.0, 140)
    seen = {}

    def callback(config, t, state, hamiltonian, result):  # (callbacks see all 3 101 times of the 1-ns grid)
        if abs(t * 3100 - 650) < 1e-6:
            seen["state"] = np.array(state.to_qobj())

    sr = StateResult(evaluation_times=[0.5, 1.0])
    obs = _observables()
    kw = dict(noise_model=NoiseModel(dephasing_rate=0.3))
    cfg = QutipConfig(default_evaluation_times=times.tolist(), observables=obs + [sr], callbacks=[callback], **kw)
    off, _ = _run(inputs, cfg, None, monkeypatch)
    kept = {"cb": seen.pop("state"), **{t: np.array(off.get_result(sr, t).to_qobj()) for t in off.get_result_times(sr)}}
    assert len(kept) == 3
    reads = _Reads(monkeypatch)
    dens, kets = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 128, monkeypatch)
    assert len(dens) == 1 and kets == [] and stats["n_applications"] == 0 and stats["n_launches"] <= 3, (dens, stats)
    assert seen["state"].shape == (32, 32) and np.array_equal(seen["state"], kept["cb"])
    for t in off.get_result_times(sr):
        assert np.array_equal(np.array(on.get_result(sr, t).to_qobj()), kept[t])
    # snapshot i is the state after i + 1 ns (the initial state is not in the store): the callback's 650 ns, then the two
    # times of StateResult, 1 550 ns and 3 100 ns, in the order fill() reaches them
    assert reads.gets == [(649, 0), (1549, 0), (3099, 0)] and reads.bulk == 0, (reads.gets, reads.bulk)
    assert _tagged(on).keys() == _tagged(off).keys()


def test_backend_noisy_master_equation_run_shares_one_call_per_store(monkeypatch):
    """Amplitude noise on top of dephasing, 3 trajectories, each solved with the master equation (the default solver
    would pick quantum jumps for a stochastic noise model): the sequences of one batched solve share one
    ``observe_density_many`` call over their store, and the aggregated results are within the bounds."""
    from pulser_amd import NoiseModel, Solver
    from pulser_amd.backend import QutipConfig
    from pulser_amd.results import SnapshotStore

    inputs, _ = _setup()
    D = 2**N_BACKEND
    times = np.linspace(0.01, 1.0, 140).tolist()
    obs = _observables(variance=False)
    kw = dict(noise_model=NoiseModel(amp_sigma=0.05, dephasing_rate=0.3), n_trajectories=3, solver=Solver.MESOLVER)
    cfg = QutipConfig(default_evaluation_times=times, observables=obs, **kw)
    states = _third_run_states(inputs, kw, times, monkeypatch, seed=11)  # (the trajectory mean: a scale for the bounds)
    off, _ = _run(inputs, cfg, None, monkeypatch, seed=11)
    stores = []
    init = SnapshotStore.__init__

    def counted_init(self, *a, **k):
        stores.append(1)
        init(self, *a, **k)

    monkeypatch.setattr(SnapshotStore, "__init__", counted_init)
    dens, kets = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 128, monkeypatch, seed=11)
    assert len(stores) >= 1 and len(dens) == len(stores) and kets == [], (dens, kets, stores)
    assert sum(c[1] for c in dens) == 3 and all(c[0] == 140 and c[2:] == (D, D) for c in dens), dens
    assert stats["n_applications"] == 0 and stats["n_launches"] <= 3 * len(dens), stats
    assert _compare_paths(on, off, obs, states, variance=False)


def test_backend_below_the_floor_keeps_the_per_time_path(monkeypatch):
    """100 evaluation times with ``observe_many_min_times = 1``: the floor of 128 holds, no call is made, and launch
    counts and results are those of the run with the path switched off."""
    from pulser_amd import NoiseModel
    from pulser_amd.backend import QutipBackendV2, QutipConfig

    assert QutipBackendV2._DENSITY_OBSERVE_MANY_FLOOR == FLOOR
    inputs, _ = _setup()
    cfg = QutipConfig(default_evaluation_times=np.linspace(0.01, 1.0, 100).tolist(), observables=_observables(),
                      noise_model=NoiseModel(dephasing_rate=0.3))
    off, stats_off = _run(inputs, cfg, None, monkeypatch)
    dens, kets = _count_calls(monkeypatch)
    on, stats = _run(inputs, cfg, 1, monkeypatch)
    assert dens == [] and kets == []
    assert stats["n_launches"] == stats_off["n_launches"] and stats["n_applications"] == stats_off["n_applications"]
    a, b = _tagged(on), _tagged(off)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k], dtype=float), np.asarray(b[k], dtype=float)), k

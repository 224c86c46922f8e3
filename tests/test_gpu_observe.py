"""GPU: the kernels that turn a finished state into the numbers a user reads - ``ryd_observe`` (k_obs_pairs,
k_obs_energy, k_obs_energy_dm), ``ryd_occupations``, ``ryd_probabilities``, ``ryd_ket_to_dm``,
``ryd_outer_accumulate_dim`` (k_outer_acc, k_outer_mfma) and ``ryd_accumulate`` (k_axpy) - called directly through
``Engine.observe`` and the other wrappers and pinned to the longdouble host reference of tests/observe_ref.py.

States are random and unphysical on purpose (no mirror symmetry, some batch entries not normalised, density matrices
random Hermitian mixtures), problems have per-atom amplitude, detuning and a non-zero phase, every batch entry has its
own problem (one with a bad atom), and the shapes sit on the kernels' edges: a partly filled and an exactly filled LDS
chunk of k_obs_pairs, more pairs than threads (23 atoms), the tail block and the grid-stride loop of k_obs_energy_dm,
the block caps of k_occupations and k_axpy, dimensions that are a multiple of 64 without being a power of two and
batches around the KT = 16 chunk of k_outer_mfma.

Tolerances are derived in tests/observe_ref.py (worst-case summation bounds in the unit roundoff 2^-53 plus the
project's 1e-11 bar of one generator application); nothing is fitted to what the kernels give.  Every case prints
``error / tolerance`` before it asserts.  Worst ratios seen on an MI355X, per kernel:

    k_obs_pairs        0.091     (the 16-term bound of a 3-atom diagonal; below 0.02 for kets of 10+ atoms)
    k_obs_energy       2.8e-5
    k_obs_energy_dm    5.4e-5
    k_occupations      0.061
    k_probabilities    1.0       (kets differ from the unfused NumPy expression by exactly 1 ulp in places; 1 ulp is
                                  the bar; density matrices are exact)
    k_ket_to_dm        0.50      (1 ulp of the 2 allowed)
    k_outer_acc        0.32
    k_outer_mfma       0.26
    k_axpy             0.50      (half an ulp of the 1 allowed)

What the module found: ``ryd_observe`` filled the correlation slots when only occupations were asked for and the
other way round, against the header's "entries that were not requested are 0" (test_observe_what_subsets); fixed in
k_obs_pairs.
"""
import numpy as np
import pytest

from helpers import local_problem, rand_state
from observe_ref import (CLD, LD, ket_probabilities, ref_energy_dm, ref_energy_ket, ref_pairs, tol_energy_dm,
                         tol_energy_ket, tol_sum, ulp)

pytestmark = pytest.mark.gpu

T_KNOT, T_LAST = 0.2, 0.4           # knots 200 and 400 of the 401 of local_problem (1-ns grid)
TIMES = [0.0, 0.12345, T_KNOT, T_LAST]
SCALES = (1.0, 0.6, 1.9)            # batch entries 1 and 2 are not normalised


def _report(kernel, what, err, tol):
    """Print error / tolerance of one output (max over its elements), then say whether it holds."""
    err, tol = np.asarray(err, dtype=float), np.asarray(tol, dtype=float)
    ok = bool(np.all(err <= tol))
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0, tol, np.finfo(float).tiny))))
    print(f"RATIO {kernel:16s} {what:34s} err {float(np.max(err)):.3e} tol {float(np.max(tol)):.3e} ratio {ratio:.3e}")
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


_CACHE = {"n": None}


def _cached(n, key, make):
    """Oracle Hamiltonians and pair references of the current atom number only (a 20-atom Hamiltonian is 0.5 GB)."""
    if _CACHE["n"] != n:
        _CACHE.clear()
        _CACHE["n"] = n
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ham(n, B, b):
    from oracle import qutip_path as qp

    bad = B > 1 and n >= 2 and b == 1
    return _cached(n, ("ham", b, bad), lambda: qp.build_hamiltonian(_problems(n, B)[b]))


def _ket(n, b):
    return SCALES[b % 3] * rand_state(2**n, 1000 * n + b)


def _mixture(n, b):
    """Random Hermitian positive mixture sum_j w_j |x_j><x_j| of 3 random kets, exactly Hermitian, trace != 1."""
    D = 2**n
    rho = np.zeros((D, D), complex)
    for j, w in enumerate((0.5, 0.3, 0.45 * SCALES[b % 3])):
        x = rand_state(D, 5000 * n + 10 * b + j)
        rho += w * np.outer(x, x.conj())
    return 0.5 * (rho + rho.conj().T)


def _engine(problems, mode="sesolve"):
    from pulser_amd.engine import Engine

    return Engine.from_problems(problems, mode=mode)


def _dev(eng, host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).to(eng.device)


def _check_pairs(got, b, p, n, tag, occupation=True, correlation=True):
    norm, occ, corr, (s_norm, s_occ, s_corr) = _cached(n, ("pairs", tag), lambda: ref_pairs(p, n))
    D = 2**n
    ok = _report("k_obs_pairs", f"{tag} norm2", abs(got["norm2"][b] - norm), tol_sum(D, s_norm))
    if occupation:
        ok &= _report("k_obs_pairs", f"{tag} occupation", np.abs(got["occupation"][b] - occ), tol_sum(D, s_occ))
    if correlation:
        ok &= _report("k_obs_pairs", f"{tag} correlation", np.abs(got["correlation"][b] - corr), tol_sum(D, s_corr))
    return ok


def _check_ket_energy(got, b, ham, t, x, tag):
    e1, e2, s_abs, w = ref_energy_ket(ham, t, x)
    tol1, tol2 = tol_energy_ket(x, w, s_abs)
    ok = _report("k_obs_energy", f"{tag} <H>", abs(got["energy"][b] - e1), tol1)
    return ok & _report("k_obs_energy", f"{tag} <H^2>", abs(got["energy2"][b] - e2), tol2)


def _check_dm_energy(got, b, ham, t, rho, n, tag):
    e1, e2, s_abs = ref_energy_dm(ham, t, rho)
    tol1, tol2 = tol_energy_dm(n, s_abs)
    ok = _report("k_obs_energy_dm", f"{tag} Tr(H rho)", abs(got["energy"][b] - e1), tol1)
    return ok & _report("k_obs_energy_dm", f"{tag} Tr(H^2 rho)", abs(got["energy2"][b] - e2), tol2)


# ---------------------------------------------------------------------------------------------------------------------
# ryd_observe on kets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 10, 11, 12, 14, 17, 20])
def test_observe_kets(n, B, t):
    """All five outputs of every batch entry; ``observe`` is the first call on a fresh handle (no solve before it: the
    work vector that takes H x and the coefficient bounds must be there already)."""
    xs = np.stack([_ket(n, b) for b in range(B)])
    with _engine(_problems(n, B)) as eng:
        got = eng.observe(_dev(eng, xs), t)
    ok = True
    for b in range(B):
        ok &= _check_pairs(got, b, ket_probabilities(xs[b]), n, f"ket n={n} b={b}")
        ok &= _check_ket_energy(got, b, _ham(n, B, b), t, xs[b], f"ket n={n} B={B} b={b} t={t}")
    assert ok


def test_observe_kets_23_atoms_pairs_only():
    """N (N + 1) / 2 + 1 = 277 > 256: a thread of k_obs_pairs takes more than one pair.  ``energy=False``: no 2^23 oracle
    matvec is needed, and the energy slots stay 0."""
    n = 23
    x = _ket(n, 1)[None, :]
    with _engine(_problems(n, 1)) as eng:
        got = eng.observe(_dev(eng, x), 0.12345, energy=False)
    assert _check_pairs(got, 0, ket_probabilities(x[0]), n, f"ket n={n}")
    assert got["energy"][0] == 0.0 and got["energy2"][0] == 0.0


def test_observe_kets_forced_generator_paths():
    """The energy moments go through whichever ``apply_generator`` plan is active: the default one, then the generic
    tiled passes without the 2^14 register tiles."""
    n, B, t = 14, 3, 0.12345
    xs = np.stack([_ket(n, b) for b in range(B)])
    ok = True
    with _engine(_problems(n, B)) as eng:
        state = _dev(eng, xs)
        for name, forced in (("default", False), ("generic", True)):
            if forced:
                eng.set_path(True, no_tile14=True)
            got = eng.observe(state, t)
            for b in range(B):
                ok &= _check_pairs(got, b, ket_probabilities(xs[b]), n, f"ket n={n} b={b}")
                ok &= _check_ket_energy(got, b, _ham(n, B, b), t, xs[b], f"ket n={n} b={b} {name}")
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# ryd_observe on density matrices
# ---------------------------------------------------------------------------------------------------------------------
def _observe_dm_case(n, B, mode):
    rhos = np.stack([_mixture(n, b) for b in range(B)])
    ok = True
    with _engine(_problems(n, B), mode=mode) as eng:
        state = _dev(eng, rhos)
        for t in TIMES:
            got = eng.observe(state, t, density=(mode == "sesolve"))
            for b in range(B):
                tag = f"dm[{mode}] n={n} B={B} b={b}"
                ok &= _check_pairs(got, b, np.real(np.diag(rhos[b])), n, tag)
                ok &= _check_dm_energy(got, b, _ham(n, B, b), t, rhos[b], n, f"{tag} t={t}")
    return ok


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 4, 6, 7, 8, 9, 10])
def test_observe_density_matrices_mesolve_handle(n, B):
    """N < 8: the tail of a partly filled block of k_obs_energy_dm; N >= 9: several blocks."""
    assert _observe_dm_case(n, B, "mesolve")


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [3, 6, 9])
def test_observe_density_matrices_on_a_ket_handle(n, B):
    """RYD_OBS_DENSITY: a ket (sesolve) handle observing density matrices with its Hamiltonian."""
    assert _observe_dm_case(n, B, "sesolve")


# ---------------------------------------------------------------------------------------------------------------------
# `what` subsets: what was not asked for is exactly 0, the norm comes with either pair output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ket", "dm"])
@pytest.mark.parametrize("which", ["occupation", "correlation", "energy"])
def test_observe_what_subsets(which, kind):
    n, B, t = (5, 3, 0.12345) if kind == "ket" else (4, 2, 0.12345)
    states = np.stack([(_ket if kind == "ket" else _mixture)(n, b) for b in range(B)])
    with _engine(_problems(n, B), mode="sesolve" if kind == "ket" else "mesolve") as eng:
        got = eng.observe(_dev(eng, states), t, occupation=which == "occupation", correlation=which == "correlation",
                          energy=which == "energy")
    ok = True
    for b in range(B):
        tag = f"{kind} n={n} b={b} only {which}"
        p = ket_probabilities(states[b]) if kind == "ket" else np.real(np.diag(states[b]))
        if which == "energy":
            assert got["norm2"][b] == 0.0
            if kind == "ket":
                ok &= _check_ket_energy(got, b, _ham(n, B, b), t, states[b], tag)
            else:
                ok &= _check_dm_energy(got, b, _ham(n, B, b), t, states[b], n, tag)
        else:
            ok &= _check_pairs(got, b, p, n, tag, occupation=which == "occupation", correlation=which == "correlation")
            assert got["norm2"][b] != 0.0
            assert got["energy"][b] == 0.0 and got["energy2"][b] == 0.0
        if which != "occupation":
            assert np.all(got["occupation"][b] == 0.0), got["occupation"][b]
        if which != "correlation":
            assert np.all(got["correlation"][b] == 0.0), got["correlation"][b]
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# exact basis-state sweep: single-term sums, equality
# ---------------------------------------------------------------------------------------------------------------------
def _basis_indices(n):
    D = 2**n
    return list(range(D)) if n == 4 else [0, 1, 2047, 2048, 2049, D // 2, D - 2, D - 1]


def _assert_basis_outputs(got, b, a, n):
    bits = np.array([1 - ((a >> (n - 1 - k)) & 1) for k in range(n)], dtype=float)
    assert got["norm2"][b] == 1.0, (a, got["norm2"][b])
    assert np.array_equal(got["occupation"][b], bits), (a, got["occupation"][b])
    assert np.array_equal(got["correlation"][b], np.outer(bits, bits)), (a, got["correlation"][b])


@pytest.mark.parametrize("n", [4, 12, 20])
def test_observe_basis_kets_exactly(n):
    """|a> with amplitude exactly 1: a dropped or doubled element cannot hide under a tolerance.  Batches of 4
    different basis states per call (the batch offsets are part of what is swept)."""
    B = 4
    idx = _basis_indices(n)
    assert len(idx) % B == 0
    with _engine([local_problem(n, seed=3)] * B) as eng:
        for i in range(0, len(idx), B):
            xs = np.zeros((B, 2**n), complex)
            for b, a in enumerate(idx[i:i + B]):
                xs[b, a] = 1.0
            got = eng.observe(_dev(eng, xs), 0.0, energy=False)
            for b, a in enumerate(idx[i:i + B]):
                _assert_basis_outputs(got, b, a, n)


def test_observe_basis_density_matrices_exactly():
    """rho = |a><a| for every a of 4 atoms, on a mesolve handle and on a ket handle with ``density=True``; the energy
    moments are then H_aa and (H^2)_aa alone (the closed forms of the comment above k_obs_energy_dm, which
    tests/test_observe_ref.py checks the reference against)."""
    n, B, t = 4, 4, 0.12345
    D = 2**n
    probs = [local_problem(n, seed=3)] * B
    from oracle import qutip_path as qp

    ham = qp.build_hamiltonian(probs[0])
    ok = True
    for mode in ("mesolve", "sesolve"):
        with _engine(probs, mode=mode) as eng:
            for i in range(0, D, B):
                rhos = np.zeros((B, D, D), complex)
                for b in range(B):
                    rhos[b, i + b, i + b] = 1.0
                got = eng.observe(_dev(eng, rhos), t, density=(mode == "sesolve"))
                for b in range(B):
                    _assert_basis_outputs(got, b, i + b, n)
                    ok &= _check_dm_energy(got, b, ham, t, rhos[b], n, f"|{i + b}><{i + b}| [{mode}]")
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# ryd_occupations / ryd_probabilities / ryd_ket_to_dm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(1, "ket"), (10, "ket"), (19, "ket"), (20, "ket"), (1, "dm"), (5, "dm"), (9, "dm")])
def test_occupations_and_probabilities(n, kind):
    """Kets up to the 1024-block cap of k_occupations (19 atoms: the first grid-stride size) and density matrices; both
    ``reverse`` values.  A probability is one rounded expression per entry: 1 ulp for a ket (fma contraction may
    differ), exact for a density matrix."""
    B, D = 2, 2**n
    if kind == "ket":
        states = np.stack([_ket(n, b + 1) for b in range(B)])
        p64 = states.real**2 + states.imag**2
        plong = [ket_probabilities(s) for s in states]
    else:
        states = np.stack([_mixture(n, b + 1) for b in range(B)])
        p64 = np.real(np.einsum("bii->bi", states)).copy()
        plong = [p.astype(LD) for p in p64]
    with _engine(_problems(n, B), mode="sesolve" if kind == "ket" else "mesolve") as eng:
        state = _dev(eng, states)
        occ = eng.occupations(state).cpu().numpy()
        probs = {rev: eng.probabilities(state, reverse=rev).cpu().numpy() for rev in (False, True)}
    ok = True
    for b in range(B):
        norm, ref_occ, _, (s_norm, s_occ, _) = ref_pairs(plong[b], n)
        ok &= _report("k_occupations", f"{kind} n={n} b={b} occupations", np.abs(occ[b, :n] - ref_occ), tol_sum(D, s_occ))
        ok &= _report("k_occupations", f"{kind} n={n} b={b} norm", abs(occ[b, n] - norm), tol_sum(D, s_norm))
    for rev, got in probs.items():
        assert got.shape == (B, D)
        want = p64[:, ::-1] if rev else p64
        if kind == "dm":
            assert np.array_equal(got, want)
        else:
            ok &= _report("k_probabilities", f"ket n={n} reverse={rev} (in ulp)", np.abs(got - want) / ulp(want), 1.0)
    assert ok


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9])
def test_new_state_ket_to_dm(n):
    """``Engine.new_state`` of a mesolve engine (ryd_ket_to_dm): one product per entry, at most 2 ulp of |x_a||x_b| on
    either component."""
    B = 2
    xs = np.stack([_ket(n, b + 1) for b in range(B)])
    with _engine(_problems(n, B), mode="mesolve") as eng:
        got = eng.new_state(xs).cpu().numpy()
    assert got.shape == (B, 2**n, 2**n)
    ok = True
    for b in range(B):
        want = np.outer(xs[b].astype(CLD), xs[b].conj().astype(CLD))  # the same product, rounded once at the end
        mag = np.outer(np.abs(xs[b]).astype(LD), np.abs(xs[b]).astype(LD)).astype(float)
        err = np.maximum(np.abs(got[b].real - want.real), np.abs(got[b].imag - want.imag)).astype(float)
        ok &= _report("k_ket_to_dm", f"n={n} b={b} (in ulp of |x_a||x_b|)", err / ulp(mag), 2.0)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# handle-free accumulators
# ---------------------------------------------------------------------------------------------------------------------
def _hermitian_start(D, seed):
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    return 0.5 * (m + m.conj().T)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("D", [9, 27, 243, 64, 192, 256])
def test_module_outer_accumulate(D, B, weighted):
    """``engine.outer_accumulate`` (ryd_outer_accumulate_dim): the plain kernel at 3^N, the matrix-core kernel at
    multiples of 64 (192 is not a power of two), batches around its chunk of 16 states.  An entry is a sum of 2 B
    products on top of the start value: (2 B + 8) u S_abs per component, S_abs = |start| + sum_t |w_t| (|.||.| + |.||.|).
    The increment is Hermitian to the same bound (not bit for bit: the weight is folded into one of the two operands)."""
    import torch
    from pulser_amd import engine as E

    rng = np.random.default_rng(31 * D + B)
    psi = rng.normal(size=(B, D)) + 1j * rng.normal(size=(B, D))
    w = rng.uniform(-0.5, 1.5, B) if weighted else None
    start = _hermitian_start(D, D + B)
    dev = torch.device("cuda", torch.cuda.current_device())
    acc = torch.from_numpy(start.copy()).to(dev)
    E.outer_accumulate(torch.from_numpy(psi).to(dev), acc, w)
    got = acc.cpu().numpy()
    wl = (np.ones(B) if w is None else w).astype(LD)
    xr, xi = psi.real.astype(LD), psi.imag.astype(LD)
    inc_re = np.einsum("t,ta,tb->ab", wl, xr, xr) + np.einsum("t,ta,tb->ab", wl, xi, xi)
    inc_im = np.einsum("t,ta,tb->ab", wl, xi, xr) - np.einsum("t,ta,tb->ab", wl, xr, xi)
    aw, ar, ai = np.abs(wl), np.abs(xr), np.abs(xi)
    s_re = np.abs(start.real) + np.einsum("t,ta,tb->ab", aw, ar, ar) + np.einsum("t,ta,tb->ab", aw, ai, ai)
    s_im = np.abs(start.imag) + np.einsum("t,ta,tb->ab", aw, ai, ar) + np.einsum("t,ta,tb->ab", aw, ar, ai)
    tol_re, tol_im = tol_sum(2 * B, s_re), tol_sum(2 * B, s_im)
    kernel = "k_outer_mfma" if D % 64 == 0 else "k_outer_acc"
    tag = f"D={D} B={B} weighted={weighted}"
    ok = _report(kernel, f"{tag} re", np.abs(got.real - (start.real + inc_re)), tol_re)
    ok &= _report(kernel, f"{tag} im", np.abs(got.imag - (start.imag + inc_im)), tol_im)
    d_re, d_im = got.real.astype(LD) - start.real, got.imag.astype(LD) - start.imag
    ok &= _report(kernel, f"{tag} increment Hermitian re", np.abs(d_re - d_re.T), tol_re + tol_re.T)
    ok &= _report(kernel, f"{tag} increment Hermitian im", np.abs(d_im + d_im.T), tol_im + tol_im.T)
    assert ok


@pytest.mark.parametrize("weight", [1.0, -0.37])
@pytest.mark.parametrize("count", [1, 255, 4**6, 4**11 + 3])
def test_module_accumulate(count, weight):
    """``engine.accumulate`` (ryd_accumulate, k_axpy) below, at and beyond its 8192 x 256 grid, count not a multiple of
    256: one fused or unfused multiply-add per component, at most 1 ulp of |acc| + |w||x|."""
    import torch
    from pulser_amd import engine as E

    rng = np.random.default_rng(count % 1000 + 5)
    x = rng.normal(size=count) + 1j * rng.normal(size=count)
    a0 = rng.normal(size=count) + 1j * rng.normal(size=count)
    dev = torch.device("cuda", torch.cuda.current_device())
    acc = torch.from_numpy(a0.copy()).to(dev)
    E.accumulate(torch.from_numpy(x).to(dev), acc, weight)
    got = acc.cpu().numpy()
    wl = LD(weight)
    err_re = np.abs(got.real - (a0.real.astype(LD) + wl * x.real)).astype(float)
    err_im = np.abs(got.imag - (a0.imag.astype(LD) + wl * x.imag)).astype(float)
    ok = _report("k_axpy", f"count={count} w={weight} re (in ulp)", err_re / ulp(np.abs(a0.real) + abs(weight) * np.abs(x.real)), 1.0)
    ok &= _report("k_axpy", f"count={count} w={weight} im (in ulp)", err_im / ulp(np.abs(a0.imag) + abs(weight) * np.abs(x.imag)), 1.0)
    assert ok

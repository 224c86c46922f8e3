"""-m gpu: the extra detuning terms (``ryd_set_detuning_terms``: high-frequency detuning noise) on every kernel that sums
them - k_eval_coefs, k_split_coefs, k_traj, k_ket, k_traj_dm - and on the host's step schedule.

The device gets ``lower(problems)`` plus term lists (tests/dterm_ref.py: lists of 1, 2, 63, 64, 65 and 130 entries, an
atom without a list between atoms with one, a shared list, a batch entry without any list, a list that ends the
table); the oracle gets the *folded* problems, whose detuning samples carry the same sum (a spline is linear in its
samples).  Bars: 1e-11 max(1, max|ref|) for one generator application, 1e-7 against the tight oracle, the bounds of
tests/observe_ref.py for the energy moments - the project's own, nothing new.

Sensitivity: next to every reference the same reference WITHOUT the last entry of the longest list is computed (what a
kernel that drops the tail of its list would give), and the two must lie 1000 tolerances apart - no test here can pass
with that term missing.  Hilbert dimensions above 2^10 assert it on one generator application instead of a second
solve.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import dterm_ref as dr
from helpers import DEPOL_PAULIS, SPLIT_BUDGET, local_problem, rand_state
from observe_ref import CLD, LD, tol_energy_ket
from pulser_amd import problem as P
from test_gpu_ket import PHASES, _with_phases, real_local_problem
from test_gpu_parity import ME_CASES

pytestmark = pytest.mark.gpu

AMP_TOL = 1e-7   # amplitudes / rho entries against the tight oracle (tests/test_gpu_parity.py)
GEN_TOL = 1e-11  # one generator application, relative to max(1, max|ref|)
SENS = 1000.0    # the reference without the last term lies at least this many tolerances away

MC_OPS = [(np.sqrt(3.0), "sigma_gr"), (np.sqrt(2 * 0.9), "sigma_rr")] + [(np.sqrt(1.2 / 4), p) for p in "xyz"]


def _make_problem(kind, n, seed, duration):
    if kind == "local":  # per-atom complex drives (time-dependent phases) and detunings
        return local_problem(n, seed=seed, duration=duration)
    if kind == "real":   # per-atom real drives
        return real_local_problem(n, seed=seed, duration=duration)
    if kind == "phase":  # ... with one of the complex-phase families of tests/test_gpu_ket.py (KET_GAUGE)
        return _with_phases(real_local_problem(n, seed=seed, duration=duration), PHASES["time-dependent"])
    if kind == "mc":
        return local_problem(n, seed=seed, duration=duration, collapse_ops=MC_OPS, paulis=DEPOL_PAULIS)
    if kind in ME_CASES:
        ops, paulis = ME_CASES[kind]
        return local_problem(n, seed=seed, duration=duration, collapse_ops=ops, paulis=paulis)
    if kind == "constant":  # constant global drive, no detuning: the lists are the only time dependence
        coords = P.register_coords(P.square_rect(1, n), 7.0)
        z = np.zeros(duration)
        return P.make_ising_problem(coords, {"amp": np.full(duration, 6.0), "det": z, "phase": z})
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _case(kind, n, distinct, duration, layout=None, plan=None, mhz=None):
    """``distinct`` different problems of ``n`` atoms; the second one (when there are two or more) has no list at all.
    ``layout``: the batch as indices into them (entries that share a problem share its lists, too)."""
    probs = [_make_problem(kind, n, 3 + s, duration) for s in range(distinct)]
    series = dr.noise_series(duration, mhz=mhz)
    with_lists = distinct - 1 if distinct >= 2 else distinct
    lists = dr.standard_lists(n, with_lists, n_series=len(series), seed=n, **({"plan": plan} if plan else {}))
    if distinct >= 2:
        lists.insert(1, [None] * n)
    idx = list(layout) if layout is not None else list(range(distinct))
    probs, lists = [probs[i] for i in idx], [lists[i] for i in idx]
    tables, folded = dr.with_term_lists(probs, lists, series)
    assert dr.check_remaining(tables.dterms)
    cut = dr.ref_without_last(probs, lists, series)
    # the batch entries (and atoms) whose list loses its last term in `cut`
    longest = max(dr.unique_lists(lists), key=len)
    hit = [(b, k) for b, row in enumerate(lists) for k, l in enumerate(row) if l is longest]
    return SimpleNamespace(n=n, problems=probs, lists=lists, series=series, tables=tables, folded=folded, cut=cut, hit=hit,
                           t_end=(duration - 1) * 1e-3)


def _canon(key, b):
    """(key, entry) without the layout: the references are cached per problem, whatever batch it sits in."""
    key = tuple(key) + (None,) * (7 - len(key))
    if key[4] is None:
        return key, b
    return key[:4] + (None,) + key[5:], key[4][b]


def _ham(key, b, which="folded"):
    return _ham_cached(*_canon(key, b), which)


@functools.lru_cache(maxsize=None)
def _ham_cached(key, b, which):
    from oracle import qutip_path as qp

    return qp.build_hamiltonian(getattr(_case(*key), which)[b])


def _sesolve_ref(key, b, times, which="folded"):
    """Tight oracle of entry b from the random ket ``_psi0(key, b)`` (computed once, shared, read-only)."""
    return _sesolve_cached(*_canon(key, b), tuple(float(t) for t in times), which)


@functools.lru_cache(maxsize=None)
def _sesolve_cached(key, b, times, which):
    from oracle import qutip_path as qp

    out = np.array(qp.sesolve(_ham_cached(key, b, which), _psi0(key, b), np.array(times), max_step=1e-3, **qp.TIGHT))
    out.setflags(write=False)
    return out


def _psi0(key, b):
    """The random start ket of entry b; entries of a ``layout`` that share a problem share it, too."""
    layout = key[4] if len(key) > 4 and key[4] is not None else None
    return rand_state(2 ** key[1], 40 + (layout[b] if layout else b))


def _engine(tables, mode="sesolve"):
    from pulser_amd.engine import Engine

    return Engine(tables, mode=mode)


def _to_dev(eng, host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).to(eng.device)


def _assert_generator_sensitive(key, t, tol):
    """G(t) x of the folded problem and of the one without the last term of the longest list, on an entry that has it."""
    c = _case(*key)
    b = c.hit[0][0]
    x = _psi0(key, b)
    d = np.max(np.abs(_ham(key, b).apply(t, x) - _ham(key, b, "cut").apply(t, x)))
    assert d >= SENS * tol, (d, tol)


def _check_kets(key, got, times, entries, worst):
    """``got`` [len(times) - 1, B, D] against the tight oracle of the folded problems; the sensitivity condition on the
    entries whose list loses its last term."""
    c = _case(*key)
    hit = {b for b, _ in c.hit}
    for b in entries:
        ref = _sesolve_ref(key, b, tuple(times))
        for i in range(1, len(times)):
            worst.append(float(np.max(np.abs(got[i - 1][b] - ref[i]))))
        if b in hit:
            if 2 ** c.n <= 1024:
                ref_cut = _sesolve_ref(key, b, tuple(times), "cut")
                gap = min(np.max(np.abs(ref[i] - ref_cut[i])) for i in range(1, len(times)))
                assert gap >= SENS * AMP_TOL, gap
            else:
                _assert_generator_sensitive(key, 0.4 * c.t_end, AMP_TOL)
    assert hit & set(entries)
    print(f"worst |hip - oracle| = {max(worst):.2e}")
    assert max(worst) < AMP_TOL, worst


# ---------------------------------------------------------------------------------------------- a. k_eval_coefs
GEN_SHAPES = {"n3_b5": ("local", 3, 5, 41), "n9_b1": ("local", 9, 1, 41)}


def _gen_times(c):
    # on a knot, inside the first interval, inside the last interval, the last knot
    return (0.005, 0.0003, c.t_end - 0.0003, c.t_end)


@pytest.mark.parametrize("shape", list(GEN_SHAPES))
def test_generator_application_sums_every_list(shape):
    """``ryd_apply_generator`` (k_eval_coefs: a wave per (trajectory, atom), four per block).  15 items: the last block
    has three live waves and one that leaves; 9 items: one live wave in the last block."""
    key = GEN_SHAPES[shape]
    c = _case(*key)
    B = len(c.problems)
    xs = np.stack([_psi0(key, b) for b in range(B)])
    worst = 0.0
    with _engine(c.tables) as eng:
        for t in _gen_times(c):
            got = eng.apply_generator(_to_dev(eng, xs), t).cpu().numpy()
            for b in range(B):
                ref = -1j * _ham(key, b).apply(t, xs[b])
                scale = max(1.0, float(np.max(np.abs(ref))))
                err = float(np.max(np.abs(got[b] - ref)))
                worst = max(worst, err / scale)
                assert err <= GEN_TOL * scale, (t, b, err)
                if b in {bb for bb, _ in c.hit}:
                    cut = -1j * _ham(key, b, "cut").apply(t, xs[b])
                    assert np.max(np.abs(ref - cut)) >= SENS * GEN_TOL * scale, t
    print(f"worst |hip - oracle| / max(1, max|ref|) = {worst:.2e}")


# ---------------------------------------------------------------------------------------------- b. ryd_observe
def _energy_longdouble(ham, t, x):
    """<x|H|x>, <Hx|Hx> and the bound's scales from the DENSE folded H(t) applied in longdouble."""
    H = np.asarray(ham.matrix(float(t)).toarray()).astype(CLD)
    xl = np.asarray(x).astype(CLD)
    w = H @ xl
    e1 = np.sum(np.conj(xl) * w).real
    w2 = (w.real * w.real + w.imag * w.imag).astype(LD)
    e2 = w2.sum(dtype=LD)
    s1 = (np.abs(xl) * np.sqrt(w2)).sum(dtype=LD)
    return e1, e2, (s1, e2), np.asarray(w, dtype=np.complex128)


@pytest.mark.parametrize("shape", list(GEN_SHAPES))
def test_observe_energy_on_a_handle_with_term_lists(shape):
    """``ryd_observe`` with RYD_OBS_ENERGY: <H> and <H^2> of a handle that has a table, every batch entry at once."""
    key = GEN_SHAPES[shape]
    c = _case(*key)
    B = len(c.problems)
    xs = np.stack([_psi0(key, b) for b in range(B)])
    worst = [0.0, 0.0]
    with _engine(c.tables) as eng:
        for t in _gen_times(c)[1:3]:
            obs = eng.observe(_to_dev(eng, xs), t, occupation=False, correlation=False, energy=True)
            for b in range(B):
                e1, e2, s_abs, w = _energy_longdouble(_ham(key, b), t, xs[b])
                tol1, tol2 = tol_energy_ket(xs[b], w, s_abs)
                d1, d2 = abs(float(obs["energy"][b] - e1)), abs(float(obs["energy2"][b] - e2))
                worst = [max(worst[0], d1 / tol1), max(worst[1], d2 / tol2)]
                assert d1 <= tol1 and d2 <= tol2, (t, b, d1, tol1, d2, tol2)
                if b in {bb for bb, _ in c.hit}:
                    c1, c2, _, _ = _energy_longdouble(_ham(key, b, "cut"), t, xs[b])
                    assert abs(float(e1 - c1)) >= SENS * tol1 and abs(float(e2 - c2)) >= SENS * tol2, (t, b)
    print(f"worst error / bound: <H> {worst[0]:.2e}, <H^2> {worst[1]:.2e}")


# ---------------------------------------------------------------------------------------------- c. k_traj
KET13 = ("real", 13, 3, 21, (0, 2, 1, 1, 0, 2, 0, 2))


@pytest.mark.parametrize("n", [3, 6, 7, 9, 11, 13])
def test_one_launch_trajectory_kernel(n):
    """k_traj, the one-launch path of kets up to 13 atoms: wave w sums the lists of atoms w, w + NW, ... into LDS.
    3 atoms: lanes without an amplitude still sum; 6: one wave; 7: two; 9: eight waves, atom 8 is wave 0's second
    round; 11: sixteen; 13: the single-buffer LDS layout (k_traj itself: 12 - 13 atoms default to k_split_reg)."""
    # (13 atoms: the first problem of the k_ket batch below, alone - one oracle run serves both tests)
    key = ("local", n, 3, 41 if n <= 9 else 21) if n <= 11 else KET13[:4] + ((0,),)
    c = _case(*key)
    times = (0.0, 0.37 * c.t_end, c.t_end)
    with _engine(c.tables) as eng:
        if n >= 12:
            eng.set_path(False, no_split14=True)
        st = _to_dev(eng, np.stack([_psi0(key, b) for b in range(len(c.problems))]))
        got = eng.solve(st, times).cpu().numpy()
        assert eng.stats()["n_launches"] == 1
    _check_kets(key, got, times, range(len(c.problems)), [])


# ---------------------------------------------------------------------------------------------- d. k_ket
@pytest.mark.parametrize("kind", ["real", "phase"])
def test_register_resident_ket_kernel_10_atoms(kind):
    """k_ket<10> (forced from 10 atoms on), real drives and - KET_GAUGE - per-atom complex phases; entry 1 has no list."""
    key = (kind, 10, 2, 41)
    c = _case(*key)
    times = (0.0, 0.017, c.t_end)
    with _engine(c.tables) as eng:
        eng.set_path(False, force_ket=True)
        st = _to_dev(eng, np.stack([_psi0(key, b) for b in range(2)]))
        got = eng.solve(st, times).cpu().numpy()
        assert eng.stats()["n_launches"] == 1, "k_ket did not take the solve"
    _check_kets(key, got, times, range(2), [])


def test_register_resident_ket_kernel_13_atoms_batch_of_8():
    """k_ket<13> on a batch of eight (the polynomial kernel kept: not k_split_reg): three different problems, one
    of them without a list; two entries against the oracle, the other six equal the entries that share their problem."""
    key, layout = KET13, KET13[4]
    c = _case(*key)
    times = (0.0, 0.37 * c.t_end, c.t_end)
    with _engine(c.tables) as eng:
        eng.set_path(False, no_split14=True)
        st = _to_dev(eng, np.stack([_psi0(key, b) for b in range(8)]))
        got = eng.solve(st, times).cpu().numpy()
        assert eng.stats()["n_launches"] == 1, "k_ket did not take the solve"
    for b in range(2, 8):
        assert np.array_equal(got[:, b], got[:, layout.index(layout[b])]), b
    assert np.max(np.abs(got[-1, 0] - got[-1, 1])) > 1e-3 and np.max(np.abs(got[-1, 0] - got[-1, 2])) > 1e-3
    _check_kets(key, got, times, (0, 1), [])


# ---------------------------------------------------------------------------------------------- e. k_split_coefs
def _split_runs(key, path, method, entries):
    """Once from t = 0 in one piece (the drive is on at t = 0: the pre-kick record), once with three evaluation times
    strictly inside the run (the records that close a snapshot)."""
    c = _case(*key)
    B = len(c.problems)
    inside = (0.0, 0.183 * c.t_end, 0.47 * c.t_end, 0.81 * c.t_end, c.t_end)
    x0 = np.stack([_psi0(key, b) for b in range(B)])
    with _engine(c.tables) as eng:
        eng.set_path(False, **path)
        st = _to_dev(eng, x0)
        eng.evolve(st, 0.0, c.t_end, method=method)
        whole = st.cpu().numpy()
        s0 = eng.stats()
        st = _to_dev(eng, x0)
        snaps = eng.solve(st, inside, method=method).cpu().numpy()
        s1 = eng.stats()
        assert np.array_equal(snaps[-1], st.cpu().numpy())
    for s in (s0, s1):
        assert 0 < s["reserved"][0] <= SPLIT_BUDGET, s  # the split-operator path ran and kept its error budget
    worst = []
    for b in entries:
        worst.append(float(np.max(np.abs(whole[b] - _sesolve_ref(key, b, inside)[-1]))))
    _check_kets(key, snaps, inside, entries, worst)
    return s0, s1


def test_split_operator_passes_forced_at_8_atoms():
    """k_split_coefs in front of the tiled split-operator passes (``method="split"``), 24 items in wave-per-item form."""
    _split_runs(("local", 8, 3, 41), {}, "split", range(3))


def test_split_operator_register_kernel_12_atoms_default_route():
    """The default route of 12 atoms (k_split_reg): its coefficient records - pre-kick, stages, snapshot closings - with a
    table; 24 items.  Snapshots are stored from inside the run (the round-4 hook ``snaps_outside`` is not set)."""
    s0, s1 = _split_runs(("local", 12, 2, 21), {}, "auto", range(2))
    assert s1["n_launches"] < s1["n_applications"]  # closed runs, not a launch per stage


# ---------------------------------------------------------------------------------------------- f. k_traj_dm
DM_PLAN = (1, 65, 0, "share", 1, 65)


@functools.lru_cache(maxsize=None)
def _mesolve_ref(key, b, times, which="folded"):
    from oracle import qutip_path as qp

    out = np.array(qp.mesolve(_ham(key, b, which), _psi0(key, b), np.array(times), max_step=1e-3, **qp.TIGHT))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("case", ["dephasing", "all"])
@pytest.mark.parametrize("n", [2, 5, 6])
def test_one_launch_density_matrix_kernel(case, n):
    """k_traj_dm: one lane per atom walks its list until ``remaining == 0`` - lists of 1 and 65 entries, a shared one,
    an atom without, an entry without."""
    key = (case, n, 2, 31 if n < 5 else 21, None, DM_PLAN)
    c = _case(*key)
    times = (0.0, 0.011, c.t_end)
    with _engine(c.tables, mode="mesolve") as eng:
        st = eng.new_state(np.stack([_psi0(key, b) for b in range(2)]))
        got = eng.solve(st, times).cpu().numpy()
        assert eng.stats()["n_launches"] == 1
    worst = 0.0
    for b in range(2):
        ref = _mesolve_ref(key, b, times)
        for i in (1, 2):
            worst = max(worst, float(np.max(np.abs(got[i - 1][b] - ref[i]))))
    assert c.hit[0][0] == 0
    if 4 ** n <= 1024:
        ref, cut = _mesolve_ref(key, 0, times), _mesolve_ref(key, 0, times, "cut")
        assert min(np.max(np.abs(ref[i] - cut[i])) for i in (1, 2)) >= SENS * AMP_TOL
    else:  # 4096 entries: one application of the Lindbladian instead of a second solve
        from oracle import qutip_path as qp

        rho = np.outer(_psi0(key, 0), _psi0(key, 0).conj()).ravel()
        gap = np.max(np.abs(qp.lindblad_rhs(_ham(key, 0))(0.4 * c.t_end, rho) - qp.lindblad_rhs(_ham(key, 0, "cut"))(0.4 * c.t_end, rho)))
        assert gap >= SENS * AMP_TOL, gap
    print(f"worst |hip - oracle| = {worst:.2e}")
    assert worst < AMP_TOL, worst


# ---------------------------------------------------------------------------------------------- g. Monte Carlo
MC_KEY = ("mc", 5, 4, 41)
MC_EVAL = (0.0, 0.02, 0.04)
MC_SUB = 8  # steps per knot interval of the jump test


def test_monte_carlo_instantiation_no_jump_evolution():
    """k_traj<.., MC = true> under H_eff, no jumps, against the tight integration of the folded effective generator."""
    from oracle import mcwf, qutip_path as qp

    c = _case(*MC_KEY)
    x0 = np.stack([_psi0(MC_KEY, b) for b in range(4)])
    with _engine(c.tables, mode="mcsolve") as eng:
        st = _to_dev(eng, x0)
        got = eng.solve(st, MC_EVAL).cpu().numpy()
        assert eng.stats()["n_launches"] == 1
    worst, gap = 0.0, np.inf
    for b in range(4):
        ref = qp._zvode(mcwf.effective_rhs(_ham(MC_KEY, b)), x0[b], np.array(MC_EVAL), dict(qp.TIGHT, max_step=1e-3))
        for i in (1, 2):
            worst = max(worst, float(np.max(np.abs(got[i - 1][b] - ref[i]))))
        if b == c.hit[0][0]:
            cut = qp._zvode(mcwf.effective_rhs(_ham(MC_KEY, b, "cut")), x0[b], np.array(MC_EVAL), dict(qp.TIGHT, max_step=1e-3))
            gap = min(np.max(np.abs(ref[i] - cut[i])) for i in (1, 2))
    assert gap >= SENS * 1e-8, gap
    print(f"worst |hip - oracle| = {worst:.2e}")
    assert worst < 1e-8, worst


def test_monte_carlo_instantiation_jump_trajectories():
    """Four seeds, four different problems (one without a list): the jumps and the kets of the CPU restatement.

    The norm threshold is tested at the end of every CF4 step (include/rydemu.h), and next to the kinks of the slot mask
    the host cuts a knot interval into sub-steps of its own (host_sched.hpp: the curvature estimate), so the restatement
    must walk the device's grid: ``max_step`` = 1/8 ns puts both on eight equal steps per interval - as long as no
    interval asks for more, which ``n_steps`` shows."""
    from oracle import mcwf

    c = _case(*MC_KEY)
    n_int = len(c.tables.tknots) - 1
    grid = np.arange(MC_SUB * n_int + 1) * (1e-3 / MC_SUB)
    seeds = np.array([1, 2 ** 40 + 17, 123456789012345, 2 ** 64 - 1], dtype=np.uint64)
    x0 = np.stack([_psi0(MC_KEY, b) for b in range(4)])
    with _engine(c.tables, mode="mcsolve") as eng:
        st = _to_dev(eng, x0)
        got = eng.mc_solve(st, MC_EVAL, seeds, max_step=1e-3 / MC_SUB).cpu().numpy()
        counts = eng.mc_jumps()
        assert eng.stats()["n_steps"] == MC_SUB * n_int, eng.stats()
    worst, total, gap = 0.0, 0, 0.0
    for b, seed in enumerate(seeds):
        ref, jumps = mcwf.mcwf_trajectory(_ham(MC_KEY, b), x0[b], grid, np.array(MC_EVAL), int(seed))
        assert counts[b] == len(jumps), (b, counts[b], jumps)
        total += len(jumps)
        for i in (1, 2):
            worst = max(worst, float(np.max(np.abs(got[i - 1][b] - ref[i]))))
        if b == c.hit[0][0]:
            cut, _ = mcwf.mcwf_trajectory(_ham(MC_KEY, b, "cut"), x0[b], grid, np.array(MC_EVAL), int(seed))
            gap = min(np.max(np.abs(ref[i] - cut[i])) for i in (1, 2))
    assert total >= 1  # jumps happen
    assert gap >= SENS * AMP_TOL, gap
    print(f"worst |hip - oracle| = {worst:.2e}, {total} jumps")
    assert worst < AMP_TOL, worst


# ---------------------------------------------------------------------------------------------- h. step schedule
def test_step_schedule_sees_a_waveform_that_lives_in_the_lists_only():
    """Constant drive, ``det_series = -1``: only the lists (40 MHz) depend on time.  Every knot interval gets a step of
    its own - a multi-knot step would cross a waveform that is not one polynomial - and the result meets the bar."""
    key = ("constant", 8, 1, 41, None, None, 40.0)
    c = _case(*key)
    assert np.all(c.tables.desc["det_series"] == -1) and len(c.series) == 2
    times = (0.0, c.t_end)
    with _engine(c.tables) as eng:
        st = _to_dev(eng, _psi0(key, 0)[None, :])
        got = eng.solve(st, times).cpu().numpy()
        s = eng.stats()
    assert s["n_steps"] >= len(c.tables.tknots) - 1, s
    _check_kets(key, got, times, (0,), [])


# ---------------------------------------------------------------------------------------------- i. the table at the ABI
def test_table_handling_at_the_abi():
    from pulser_amd._lib import RydError
    from pulser_amd.terms import lower

    key = GEN_SHAPES["n3_b5"]
    c = _case(*key)
    dt = np.ascontiguousarray(c.tables.dterms)
    xs = np.stack([_psi0(key, b) for b in range(5)])
    INVALID = -1  # RYD_ERR_INVALID
    with _engine(c.tables) as eng:
        lib, h = eng.lib, eng._h
        x = _to_dev(eng, xs)
        good = eng.apply_generator(x, 0.0123).cpu().numpy()
        # an inconsistent `remaining`: refused, the table stays
        for i, v in ((0, dt["remaining"][0] + 1), (len(dt) - 1, 1), (3, -1)):
            bad = dt.copy()
            bad["remaining"][i] = v
            assert lib.ryd_set_detuning_terms(h, len(bad), bad.ctypes.data) == INVALID
            assert "remaining" in lib.ryd_last_error().decode()
        assert np.array_equal(eng.apply_generator(x, 0.0123).cpu().numpy(), good)
        # an `extra` past the table, desc set after the terms: refused when an apply / a solve starts
        desc = np.ascontiguousarray(c.tables.desc.copy())
        desc["extra"][4, 2] = len(dt) + 1
        assert lib.ryd_set_qubit_desc(h, desc.ctypes.data) == 0
        for call in (lambda: eng.apply_generator(x, 0.0123), lambda: eng.evolve(x.clone(), 0.0, 0.01)):
            with pytest.raises(RydError) as err:
                call()
            assert err.value.code == INVALID and "extra" in str(err.value)
        # ... and terms set after the desc: a shorter table leaves the old indices outside
        good_desc = np.ascontiguousarray(c.tables.desc)
        assert lib.ryd_set_qubit_desc(h, good_desc.ctypes.data) == 0
        assert np.array_equal(eng.apply_generator(x, 0.0123).cpu().numpy(), good)
        short = np.ascontiguousarray(dt[:130])  # the first list alone
        assert dr.check_remaining(short) and int(good_desc["extra"].max()) > 130
        assert lib.ryd_set_detuning_terms(h, len(short), short.ctypes.data) == 0
        for call in (lambda: eng.apply_generator(x, 0.0123), lambda: eng.evolve(x.clone(), 0.0, 0.01)):
            with pytest.raises(RydError) as err:
                call()
            assert err.value.code == INVALID
        # n_terms = 0 removes the table: indices into it are refused; with the plain descriptors the handle is the
        # un-noised one, bit for bit (the extra series stay in the spline table, unused)
        assert lib.ryd_set_detuning_terms(h, 0, None) == 0
        with pytest.raises(RydError) as err:
            eng.apply_generator(x, 0.0123)
        assert err.value.code == INVALID
        plain = lower(c.problems)
        pdesc = np.ascontiguousarray(plain.desc)
        assert np.all(pdesc["extra"] == 0) and lib.ryd_set_qubit_desc(h, pdesc.ctypes.data) == 0
        bare = eng.apply_generator(x, 0.0123).cpu().numpy()
        with _engine(plain) as ref:
            assert np.array_equal(bare, ref.apply_generator(_to_dev(ref, xs), 0.0123).cpu().numpy())
        assert np.max(np.abs(bare - good)) > 1e-3  # the table did something

"""The quantum-jump kernels of the general path (multi-level and XY registers) against exact trajectories on every route.

Every case of the table in tests/mcwf_general_ref.py is run on every route that serves it and compared, trajectory by
trajectory, with the cluster-product reference of that file (interaction block-diagonal over scattered clusters of 1 - 3
atoms, every atom driven; tests/test_mcwf_general_ref.py pins it on the full-space restatement of ``oracle/mcwf.py`` and
checks the table):

* ``many``: ``GeneralEngine.mc_solve_many``, one engine per trajectory - the persistent kernel ``k_gen_traj_mc`` with
  its in-register copy of the bookkeeping (``mcg_traj_norm``, ``mcg_traj_step``) at 2, 3, 4 amplitudes, 729 (row set
  j = 0 partly filled), 1 024 (full), 2 048 (two row sets), 2 187 (j = 2 holds 139 rows) and 4 096 (the cap: six
  four-level atoms fill the ``rho`` scratch, twelve XY atoms make the longest atom loop), and one call over engines of
  243, 729 and 2 187 amplitudes;
* ``batched``: ``mc_solve`` of a batched engine on the persistent kernel (the sizes that pass
  ``use_persistent_general_mc``), batches of 1, 12 and 130, the evaluation times (the first one repeated) cutting the
  run into two launches that hand the jump state over (``init = 0``, ``refnorm <- ref / n2``);
* ``chain``: the multi-launch kernels of k_mc_general.hpp (``set_path(True)``) on the same cases, and at their natural
  sizes of 6, 8, 16, 19 and 128 blocks.

Both lowerings (explicit CSR terms: the digit layout comes from ``set_collapse``; matrix-free terms) up to 4 096
amplitudes.  Per trajectory: the number of jumps is the reference's; every stored ket and the final state are within the
parity bar of 1e-7 (``test_trajectories_match_cpu_restatement``) - a jump on another step, atom or operator is off by
O(0.1) - and have norm 1 to 1e-12.  The route is asserted from the statistics, ``n_steps`` against the grid.

What this does and does not detect: as for the two-level kernels (tests/test_gpu_mcwf_edges.py) the weights are never
read out, an error in them shows only as a flipped selection; the reference never entangles two clusters.
"""
import functools

import numpy as np
import pytest

import mcwf_general_ref as R

from pulser_amd.engine import GeneralEngine
from pulser_amd.general import lower_general

pytestmark = pytest.mark.gpu

PARITY = 1e-7
N_STEPS = len(R.GRID) - 1
# A solve on the persistent kernel is one launch whatever its evaluation times; only a repeated time ends a launch
# (host_step.hpp: flush, copy the snapshot, continue).  The batched route repeats the first evaluation time, so that
# the run is two launches and the jump state is handed over between them at a time that trajectories of the table
# cross decayed and without a jump (tests/test_mcwf_general_ref.py).
EVAL_CUT = np.array([R.EVAL[0], R.EVAL[1], R.EVAL[1], R.EVAL[2]])


def _lowerings(case, route):
    if case.dim > 4096:
        return (True,)
    return (False,) if route == "batched" else (False, True)


PARAMS = [pytest.param(c, r, f, id=f"{c.name}-{r}-{'free' if f else 'csr'}")
          for c in R.CASES for r in c.routes for f in _lowerings(c, r)]


@functools.lru_cache(maxsize=None)
def _lowered(ops, n, parts, lean, free):
    tables, cops = lower_general(R._problem(ops, n, parts, lean), mesolve=False, matrix_free=free, with_collapse=True)
    assert (tables.free is not None) == free  # no fall-back between the lowerings
    return tables, cops


def _tables(case, free):
    return _lowered(case.ops, case.n, case.parts, case.lean, free)


def _solve_many(cases_and_rows, free):
    """One ``mc_solve_many`` call over one engine per (case, trajectory): (snapshots, finals, counts, stats) per engine."""
    engines, states, seeds = [], [], []
    try:
        for case, b in cases_and_rows:
            d = R.case_data(case)
            tables, cops = _tables(case, free)
            eng = GeneralEngine(tables)
            engines.append(eng)
            eng.set_collapse(cops)
            states.append(eng.torch.from_numpy(np.ascontiguousarray(d.psi0()[b:b + 1])).to(eng.device))
            seeds.append(int(d.seeds[b]))
        outs = GeneralEngine.mc_solve_many(engines, states, R.EVAL, np.array(seeds, dtype=np.uint64))
        return ([o.cpu().numpy()[:, 0] for o in outs], [s.cpu().numpy()[0] for s in states],
                [int(e.mc_jumps()[0]) for e in engines], [e.stats() for e in engines])
    finally:
        for e in engines:
            e.close()


@functools.lru_cache(maxsize=None)
def _run(case, route, free):
    """(snapshots [len(EVAL) - 1, batch, dim], finals [batch, dim], jump counts, statistics) of a case on a route."""
    d = R.case_data(case)
    if route == "many":
        snaps, finals, counts, stats = _solve_many([(case, b) for b in range(case.batch)], free)
        assert all(s["n_steps"] == N_STEPS for s in stats)
        assert sum(s["n_launches"] for s in stats) == 1  # counted on the first engine
        return np.stack(snaps, axis=1), np.stack(finals), counts, stats[0]
    tables, cops = _tables(case, free)
    with GeneralEngine(tables, batch=case.batch) as eng:
        eng.set_collapse(cops)
        eng.set_path(route == "chain")
        state = eng.torch.from_numpy(np.ascontiguousarray(d.psi0())).to(eng.device)
        if route == "chain":
            snaps = eng.mc_solve(state, R.EVAL, d.seeds).cpu().numpy()
        else:
            cut = eng.mc_solve(state, EVAL_CUT, d.seeds).cpu().numpy()
            assert np.max(np.abs(cut[1] - cut[0])) < 1e-14  # the repeated time stores the handed-over state
            snaps = cut[[0, 2]]
        return snaps, state.cpu().numpy(), eng.mc_jumps().tolist(), eng.stats()


def _compare(snaps, finals, kets):
    """(worst |hip - ref|, worst norm defect) over the stored kets and the final state of one trajectory."""
    worst, defect = 0.0, 0.0
    for i in range(1, len(R.EVAL)):
        worst = max(worst, float(np.max(np.abs(snaps[i - 1] - kets[i]))))
        defect = max(defect, abs(float(np.linalg.norm(snaps[i - 1])) - 1.0))
    worst = max(worst, float(np.max(np.abs(finals - kets[-1]))))
    return worst, max(defect, abs(float(np.linalg.norm(finals)) - 1.0))


@pytest.mark.parametrize("case,route,free", PARAMS)
def test_trajectories_match_the_exact_reference(case, route, free):
    d = R.case_data(case)
    snaps, finals, counts, stats = _run(case, route, free)
    worst, defect = 0.0, 0.0
    for b in range(case.batch):
        w, e = _compare(snaps[:, b], finals[b], d.kets[b])
        worst, defect = max(worst, w), max(defect, e)
    want = [len(j) for j in d.jumps]
    shown = counts if len(counts) <= 12 else f"{counts[:12]}..."
    print(f"mcwf-general-edges {case.name} {route} {'free' if free else 'csr'}: worst |hip - ref| = {worst:.2e}, "
          f"norm defect {defect:.1e}, {case.batch} trajectories, {sum(want)} jumps, device counts {shown}, "
          f"skipped seeds {len(d.skipped)}, n_steps {stats['n_steps']}, launches {stats['n_launches']}, "
          f"reference {d.cpu_seconds:.1f} s")
    assert list(counts) == want, (counts, want, d.jumps)
    assert worst < PARITY, worst
    assert defect < 1e-12, defect
    assert stats["n_steps"] == N_STEPS, stats  # one step per sample interval: the grid of the reference
    if route == "many":
        assert stats["n_launches"] == 1
    elif route == "batched":
        # the persistent kernel: at most one launch per interval, and the hand-over between launches is reached
        assert 2 <= stats["n_launches"] <= len(EVAL_CUT) - 1, stats
    else:
        assert stats["n_launches"] > 4 * stats["n_steps"], stats


@pytest.mark.parametrize("case", [c for c in R.CASES if len(c.routes) > 1], ids=lambda c: c.name)
def test_routes_agree_with_each_other(case):
    """The two persistent entry points and the chain on the cases they share: 1e-10, the bar of
    ``test_trajectories_match_cpu_restatement``."""
    runs = {(r, f): _run(case, r, f) for r in case.routes for f in _lowerings(case, r)}
    (key0, first), *rest = runs.items()
    worst = 0.0
    for key, other in rest:
        assert list(other[2]) == list(first[2]), (key0, key)
        worst = max(worst, float(np.max(np.abs(other[0] - first[0]))), float(np.max(np.abs(other[1] - first[1]))))
    print(f"mcwf-general-edges {case.name}: {len(runs)} runs agree to {worst:.2e}")
    assert worst < 1e-10, worst


@pytest.mark.parametrize("free", [False, True], ids=["csr", "free"])
def test_one_call_over_engines_of_three_sizes(free):
    """``ryd_general_mc_solve_many`` carries a ``dim`` and an atom count of its own in every workgroup: four trajectories
    each of the 243-, 729- and 2 187-amplitude cases in one launch."""
    cases = [next(c for c in R.CASES if c.name == name) for name in ("all-n5", "all-n6", "all-n7")]
    rows = [(c, b) for b in range(4) for c in cases]  # sizes interleaved over the workgroups
    snaps, finals, counts, stats = _solve_many(rows, free)
    assert sum(s["n_launches"] for s in stats) == 1 and all(s["n_steps"] == N_STEPS for s in stats)
    worst = 0.0
    for (c, b), s, f, n in zip(rows, snaps, finals, counts):
        d = R.case_data(c)
        assert n == len(d.jumps[b]), (c.name, b, n, d.jumps[b])
        w, e = _compare(s, f, d.kets[b])
        assert e < 1e-12, e
        worst = max(worst, w)
    print(f"mcwf-general-edges mixed sizes {'free' if free else 'csr'}: worst |hip - ref| = {worst:.2e}, counts {counts}")
    assert worst < PARITY, worst
    assert sum(counts) >= len(rows)

"""The cluster-product quantum-jump reference of tests/mcwf_general_ref.py against the full-space restatement
(``oracle/mcwf.py``) where that is affordable, and the conditions on the case table that drives
tests/test_gpu_mcwf_general_edges.py - all on the CPU, so that the device test cannot pass vacuously."""
import numpy as np
import pytest

import mcwf_general_ref as R
import mcwf_ref

from pulser_amd.general import lower_general

ROUTES = ("many", "batched", "chain")
T_FIRST = float(R.EVAL[1])  # the first evaluation time: where a batched persistent run hands over between launches


def _data(case):
    return R.case_data(case, False)  # (the d^n kets are formed by the device tests only)


# ---------------------------------------------------------------------------------------------------------------------
# The reference against the full-space restatement
# ---------------------------------------------------------------------------------------------------------------------
PINS = {
    "xy-3+2+1": R.Case("xy", 6, (3, 2, 1), 3, ()),
    "all-2+2+1": R.Case("all", 5, (2, 2, 1), 3, ()),
    "leak-2+1": R.Case("leak", 3, (2, 1), 3, ()),
    "nondiag3-2+1+1": R.Case("nondiag3", 4, (2, 1, 1), 3, ()),
}
PIN_SEEDS = (1, 2 ** 40 + 17, 2 ** 64 - 1)  # those of tests/test_mcwf_ref.py


@pytest.mark.parametrize("name", list(PINS))
def test_cluster_reference_equals_the_full_space_restatement(name):
    """Driven and interacting clusters with scattered members, every local drive the table takes, kets of squared norm
    1 and 0.6: the same jumps, kets to 1e-9 (the bar of tests/test_mcwf_ref.py), both margins above 1e-9."""
    from oracle import mcwf, qutip_path as qp

    case = PINS[name]
    prob = R.problem_of(case)
    ham = qp.build_hamiltonian(prob)
    clusters, cops, props = R.case_parts(case)
    assert any(len(c) > 1 and c[-1] - c[0] >= len(c) for c in clusters) or case.n <= 4  # members not contiguous
    total = 0
    for b, seed in enumerate(PIN_SEEDS):
        f0 = R.initial_factors(case, b)
        if b == 1:
            f0[-1] = f0[-1] * np.sqrt(0.6)
        psi0 = R.product_ket(case.d, case.n, clusters, f0)
        want, wj = mcwf.mcwf_trajectory(ham, psi0, R.GRID, R.EVAL, seed)
        got, gj, margins = R.cluster_trajectory(case.d, case.n, clusters, cops, props, f0, R.GRID, R.EVAL, seed)
        assert gj == wj, (seed, gj, wj)
        assert min(margins) > 1e-9, margins
        for g, w in zip(got, want):
            assert np.max(np.abs(g - w)) < 1e-9, (seed, np.max(np.abs(g - w)))
        total += len(gj)
    assert total >= len(PIN_SEEDS)


def test_shared_constants_are_those_of_the_two_level_table():
    assert R.MARGIN is mcwf_ref.MARGIN and R.MARGIN == 1e-6
    assert R.seed_list is mcwf_ref.seed_list and R.GRID is mcwf_ref.GRID and R.EVAL is mcwf_ref.EVAL
    assert set(mcwf_ref.SPECIAL_SEEDS) == {0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1}


# ---------------------------------------------------------------------------------------------------------------------
# The problems
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_interaction_is_block_diagonal_over_scattered_clusters(case):
    prob = R.problem_of(case)
    clusters = R.clusters_of(case)
    assert sorted(a for c in clusters for a in c) == list(range(case.n))
    assert tuple(len(c) for c in clusters) == case.parts
    member = {a: i for i, c in enumerate(clusters) for a in c}
    imat = np.asarray(prob["interaction_matrix"])
    inside = []
    for i in range(case.n):
        for j in range(case.n):
            if i == j:
                continue
            if member[i] != member[j]:
                assert np.all(imat[:, i, j] == 0.0)
            else:
                inside.append(np.abs(imat[:, i, j]).min())
    if case.n > 1:
        assert inside and min(inside) > 1.0, inside  # rad/us: every in-cluster pair interacts (on every layer)
        assert len(set(np.round(inside, 12))) == len(inside) // 2  # no two pairs alike
    if case.n >= 5:  # strides mix: some cluster's members are not a contiguous run
        assert any(c[-1] - c[0] >= len(c) for c in clusters), clusters
    # drives: a global one; local ones on atoms 0 and N - 1 always, on every atom where the term table allows
    local = [q for per in prob["samples"]["Local"].values() for q in per]
    assert 0 in local and case.n - 1 in local
    assert len(local) == (min(case.n, 2) if case.lean else case.n)
    waves = [s["amp"] for per in prob["samples"]["Local"].values() for s in per.values()]
    assert len({w.tobytes() for w in waves}) == len(waves)
    # nothing starts in the leakage state, every cluster ket is entangled (no product of one-atom kets)
    f0 = R.initial_factors(case, 0)
    if case.basis == "leak":
        psi = R.product_ket(case.d, case.n, clusters, f0)
        digits = (np.arange(case.dim)[:, None] // case.d ** np.arange(case.n)) % case.d
        assert np.all(psi[(digits == 3).any(axis=1)] == 0.0)
    for f, c in zip(f0, clusters):
        if len(c) > 1:
            sv = np.linalg.svd(np.asarray(f).reshape(case.d, -1), compute_uv=False)
            assert sv[1] / sv[0] > 0.05


def _lowerings(case):
    return ((False, True) if case.dim <= 4096 else (True,))


@pytest.mark.parametrize("case", [c for c in R.CASES if c.batch != 130 and c.batch != 1 and c.norm2 == 1.0],
                         ids=lambda c: c.name)
def test_one_cf4_step_per_sample_interval_by_the_rule_of_the_scheduler(case):
    """The waveforms are slow enough for build_schedule (host_sched.hpp) to take one CF4 step per sample interval -
    its two estimates, restated on the lowered tables, stay below their bounds - and the matrix-free lowering holds
    every term (no fall-back to CSR).  The device test asserts n_steps itself."""
    prob = R.problem_of(case)
    cops = R.local_collapse(prob)
    s = sum(c.conj().T @ c for c in cops)
    decay = case.n * float(np.abs(0.5 * s).sum(axis=1).max())
    for free in _lowerings(case):
        tables = lower_general(prob, mesolve=False, matrix_free=free)
        assert (tables.free is not None) == free
        curv, step = R.schedule_estimates(tables, decay)
        assert curv < 0.5 and step < 0.5, (case.name, free, curv, step)
        if free:
            assert len(tables.series) + 1 <= R.MAX_GEN_TERMS


# ---------------------------------------------------------------------------------------------------------------------
# The case table: conditions on the inputs of the device tests, checked with the reference alone
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_holds_the_matrix_of_the_device_tests():
    by = {(c.ops, c.n): c for c in R.CASES if not c.lean and c.norm2 == 1.0}
    # the persistent kernel's rows through mc_solve_many, and the chain on the same cases
    for key, dim in ((("xy", 1), 2), (("all", 1), 3), (("leak+", 1), 4), (("all", 6), 729), (("leak", 5), 1024),
                     (("xy", 10), 1024), (("xy", 11), 2048), (("all", 7), 2187), (("leak", 6), 4096), (("xy", 12), 4096),
                     (("all", 5), 243)):
        assert by[key].dim == dim and {"many", "chain"} <= set(by[key].routes), key
    # the chain's natural sizes: blocks = min(max(dim >> 10, 1), 128)
    for key, dim, blocks, batch in ((("all", 8), 6561, 6, 4), (("all", 9), 19683, 19, 4), (("leak", 7), 16384, 16, 4),
                                    (("xy", 13), 8192, 8, 4), (("xy", 14), 16384, 16, 4), (("xy", 18), 262144, 128, 2)):
        c = by[key]
        assert c.dim == dim and min(max(dim >> 10, 1), 128) == blocks and c.batch == batch and c.routes == ("chain",)
    assert 2187 - 2 * 1024 == 139  # rows of j = 2 at 3^7
    assert 6 * 4 * 4 == 96        # N D^2 at the cap with four levels: the stated limit of the rho scratch
    # batched persistent runs: batches of 1, 12 and 130, the last at 64 amplitudes
    batched = [c for c in R.CASES if "batched" in c.routes]
    assert {c.batch for c in batched} == {1, 12, 130}
    assert all(c.dim == 64 for c in batched if c.batch == 130)
    assert {c.d for c in batched} == {2, 3, 4}
    # operators: 16, a single one, non-diagonal sums at d = 2 and d = 3, the leakage pair; start norms
    assert len(R.OPERATORS["ops16"]) == R.MC_MAX_OPS and len(R.OPERATORS["xy"]) == 1
    for ops in ("nondiag2", "nondiag3"):
        case = next(c for c in R.CASES if c.ops == ops)
        s = sum(m.conj().T @ m for m in R.local_collapse(R.problem_of(case)))
        assert np.abs(s - np.diag(np.diag(s))).max() > 0.1
    assert {c.ops for c in R.CASES} == set(R.OPERATORS)
    assert sorted(c.norm2 for c in R.CASES if c.norm2 != 1.0) == [0.37, 2.5]
    assert len({c.name for c in R.CASES}) == len(R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_margins_seeds_and_jump_counts(case):
    d = _data(case)
    assert len(d.seeds) == case.batch
    assert len(d.skipped) <= case.batch // 12, d.skipped  # at most 1 seed in 12
    for m in d.margins:
        assert min(m) >= R.MARGIN, m
    used = [int(s) for s in d.seeds]
    for s in mcwf_ref.SPECIAL_SEEDS[:case.batch]:
        assert s in used or s in d.skipped
    counts = [len(j) for j in d.jumps]
    assert sum(counts) >= case.batch, counts
    if case.batch >= 4:
        assert max(counts) >= 2 and min(counts) == 0, counts
    for f0 in d.factors0:
        n2 = float(np.prod([np.vdot(f, f).real for f in f0]))
        assert abs(n2 - case.norm2) < 1e-12
    if case.batch > 1:  # a step in which one entry jumps and another does not
        steps = [{t for t, _, _ in j} for j in d.jumps]
        assert any(t not in other for s in steps for t in s for other in steps if other is not s)


@pytest.mark.parametrize("route", ROUTES)
def test_route_coverage(route):
    cases = [c for c in R.CASES if route in c.routes]
    first, last, kinds, zero_before, high = False, False, set(), 0, False
    for c in cases:
        d = _data(c)
        for j, tr in zip(d.jumps, d.traces):
            for _, a, k in j:
                first |= a == 0 and c.n > 1
                last |= a == c.n - 1 and c.n > 1
                kinds.add((c.ops, k))
                high |= c.ops == "ops16" and k >= 8
            zero_before += sum(1 for e in tr if e[0] == "select" and e[1] > 0)
    assert first and last
    want = {(c.ops, k) for c in cases for k in range(len(R.OPERATORS[c.ops])) if c.ops != "ops16"}
    assert want <= kinds, sorted(want - kinds)
    assert zero_before >= 1
    if route != "batched":
        assert high  # the 16-operator case selects an operator of index >= 8
    if route == "many":  # rows j >= 1 of the persistent kernel: jumps on both ends of the register there too
        for c in cases:
            if c.dim > 2048 and c.ops != "xy":
                atoms = {a for j in _data(c).jumps for _, a, _ in j}
                assert 0 in atoms and c.n - 1 in atoms, (c.name, atoms)


def test_batched_persistent_cases_cross_the_first_evaluation_time_both_ways():
    """The hand-over between the launches of a batched persistent run (refnorm <- ref / n2): some trajectory reaches the
    first evaluation time without a jump and with a squared norm below 0.99, another has jumped by then."""
    step = int(round(T_FIRST / (R.GRID[1] - R.GRID[0]))) - 1
    for c in (c for c in R.CASES if "batched" in c.routes and c.batch >= 12):
        d = _data(c)
        decayed = jumped = 0
        for j, tr in zip(d.jumps, d.traces):
            early = [t for t, _, _ in j if t <= T_FIRST + 1e-12]
            ratio = next(e[1] for e in tr if e[0] == step)
            decayed += (not early) and ratio < 0.99
            jumped += bool(early)
        assert decayed >= 1 and jumped >= 1, (c.name, decayed, jumped)
        # ... and jumps again after it: the threshold of the next jump crosses the launches too
        assert any(len(j) >= 2 and j[0][0] <= T_FIRST < j[-1][0] for j in d.jumps) or c.n == 1, c.name


# ---------------------------------------------------------------------------------------------------------------------
# What the device test can detect
# ---------------------------------------------------------------------------------------------------------------------
def _rerun(case, b, **kw):
    d = _data(case)
    clusters, cops, props = R.case_parts(case)
    return R.cluster_trajectory(case.d, case.n, clusters, cops, props, d.factors0[b], R.GRID, R.EVAL, int(d.seeds[b]), **kw)


@pytest.mark.parametrize("name", ["all-n6", "leak-n5", "xy-n11", "nondiag3-n7", "ops16-n6"])
def test_a_jump_moved_to_the_neighbour_changes_a_stored_ket(name):
    """Moving one jump of the reference to the neighbouring atom, or to the neighbouring operator, changes a stored ket
    by more than 0.01 (the device test's bar is 1e-7)."""
    case = next(c for c in R.CASES if c.name == name)
    d = _data(case)
    b = next(i for i, j in enumerate(d.jumps) if j and j[0][0] < R.EVAL[-1] - 0.01)
    base = _rerun(case, b)[0]
    n_ops = len(R.OPERATORS[case.ops])
    moves = [lambda a, k: ((a + 1) % case.n, k)] + ([lambda a, k: (a, (k + 1) % n_ops)] if n_ops > 1 else [])
    for move in moves:
        kets = _rerun(case, b, override=lambda j, a, k, move=move: move(a, k) if j == 0 else (a, k))[0]
        diff = max(float(np.max(np.abs(x - y))) for x, y in zip(kets, base))
        assert np.isfinite(diff) and diff > 0.01, diff


def test_the_table_sees_weight_errors_from_about_one_percent():
    """The weights are never read out: a wrong weight shows only as a flipped selection.  Weights off by +-1 %
    (alternating over the candidates) change the jump list of some trajectory of the table, weights off by +-1e-6
    change none: the margins keep rounding differences between the device and the reference from flipping anything."""
    changed = {0.01: 0, 1e-6: 0}
    for eps in changed:
        for case in R.CASES:
            d = _data(case)
            for b in range(min(case.batch, 12)):
                jumps = _rerun(case, b, form_kets=False,
                               perturb=lambda a, k, w, eps=eps: w * (1 + eps * (1 if (a + k) % 2 else -1)))[1]
                changed[eps] += jumps != d.jumps[b]
    print(f"trajectories whose jump list changes: {changed}")
    assert changed[0.01] >= 1 and changed[1e-6] == 0, changed

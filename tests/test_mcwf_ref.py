"""The two exact quantum-jump references of tests/mcwf_ref.py against the full-space restatement (``oracle/mcwf.py``)
where that is cheap, the Philox generator against published vectors, and the conditions on the case table that drives
tests/test_gpu_mcwf_edges.py - all on the CPU."""
import numpy as np
import pytest

import mcwf_ref as R
from helpers import DEPOL_PAULIS, local_problem

# the operators, step grid and evaluation times of tests/test_gpu_mcwf.py (restated: importing that module needs the
# device library); test_the_restated_constants_are_those_of_the_device_tests compares them where it can be imported
OPS = [(np.sqrt(3.0), "sigma_gr"), (np.sqrt(2 * 0.9), "sigma_rr")] + [(np.sqrt(1.2 / 4), p) for p in "xyz"]
GRID = np.arange(401) / 1000.0
EVAL = np.array([0.0, 0.1, 0.25, 0.4])
SEEDS = (1, 2 ** 40 + 17, 2 ** 64 - 1)


def test_the_restated_constants_are_those_of_the_device_tests():
    import ast
    import os

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_mcwf.py")).read()
    found = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) in ("GRID", "EVAL", "OPS"):
            found[node.targets[0].id] = eval(compile(ast.Expression(node.value), "test_gpu_mcwf.py", "eval"), {"np": np})
    assert np.array_equal(found["GRID"], GRID) and np.array_equal(found["EVAL"], EVAL)
    assert [(float(c), k) for c, k in found["OPS"]] == [(float(c), k) for c, k in OPS]
    assert R.PAULIS == DEPOL_PAULIS


def _driven(n, model):
    prob = local_problem(n, seed=5, collapse_ops=OPS, paulis=DEPOL_PAULIS)
    if model == 1:
        t = GRID
        prob["samples"] = {"Global": {"ground-rydberg": {"amp": 7.0 * (1 + 0.5 * np.sin(2 * np.pi * t / t[-1])),
                                                         "det": 5.0 * np.cos(3 * t) - 4.0, "phase": np.zeros(len(t))}},
                           "Local": {}}
    prob["interaction_matrix"] = np.zeros_like(prob["interaction_matrix"])
    return prob


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("model", [0, 1])
def test_product_reference_equals_the_full_space_restatement(n, model):
    """Reference A: no interaction, local complex drives (model 0) / one global real drive (model 1), product kets of
    squared norm 1 and 0.6: the same jumps, kets to 1e-9."""
    from oracle import mcwf, qutip_path as qp

    prob = _driven(n, model)
    ham = qp.build_hamiltonian(prob)
    props = R.one_atom_propagators(prob, GRID)
    rng = np.random.default_rng(n + 10 * model)
    total = 0
    for i, seed in enumerate(SEEDS):
        f0 = rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))
        f0 /= np.linalg.norm(f0, axis=1)[:, None]
        if i == 1:
            f0[-1] *= np.sqrt(0.6)
        want, wj = mcwf.mcwf_trajectory(ham, R.kron_chain(f0), GRID, EVAL, seed)
        got, gj, margins = R.product_trajectory(prob, f0, GRID, EVAL, seed, props=props)
        assert gj == wj, (seed, gj, wj)
        assert min(margins) > 1e-9, margins
        for g, w in zip(got, want):
            assert np.max(np.abs(g - w)) < 1e-9, (seed, np.max(np.abs(g - w)))
        total += len(gj)
    assert total >= len(SEEDS)


@pytest.mark.parametrize("n", [3, 4])
def test_diagonal_reference_equals_the_full_space_restatement(n):
    """Reference B: zero amplitudes, time-dependent detunings, the real interaction matrix, random entangled unnormalised
    kets: the same jumps, kets to 1e-9."""
    from oracle import mcwf, qutip_path as qp

    prob = R.problem_b(n, 5.0, 77 + n)
    assert np.abs(prob["interaction_matrix"]).max() > 10.0
    ham = qp.build_hamiltonian(prob)
    factors = R.diagonal_factors(prob, R.GRID)
    rng = np.random.default_rng(n)
    total = 0
    for seed in SEEDS + (4242,):
        psi0 = (rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)) * rng.uniform(0.2, 0.8)
        want, wj = mcwf.mcwf_trajectory(ham, psi0, R.GRID, R.EVAL, seed)
        got, gj, margins = R.diagonal_trajectory(prob, psi0, R.GRID, R.EVAL, seed, factors=factors)
        assert gj == wj, (seed, gj, wj)
        assert min(margins) > 1e-9, margins
        for g, w in zip(got, want):
            assert np.max(np.abs(g - w)) < 1e-9, (seed, np.max(np.abs(g - w)))
        total += len(gj)
    assert total >= 4


def test_philox4x32_10_known_answers():
    """The three known-answer vectors of philox4x32-10 in the Random123 distribution (D. E. Shaw Research,
    ``examples/kat_vectors``: zero counter and key, all-ones counter and key, counter and key from the digits of pi)."""
    from oracle.mcwf import philox4x32_10

    ones = 0xFFFFFFFF
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
        ([ones] * 4, [ones] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
         [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
    ]
    for counter, key, want in kat:
        assert philox4x32_10(counter, key) == want, [hex(x) for x in philox4x32_10(counter, key)]


# ---------------------------------------------------------------------------------------------------------------------
# The case table: conditions on the inputs of the device tests, checked with the references alone
# ---------------------------------------------------------------------------------------------------------------------
def _data(case):
    return R.case_data(case, case.kind != "A")  # (the 2^N kets of reference A are formed by the device tests only)


def test_case_table_holds_the_matrix_of_the_device_tests():
    by = {}
    for c in R.CASES:
        if c.norm2 in (0.0, 1.0):
            by.setdefault(c.n, set()).add((c.kind, c.model, c.batch))
    for n in (1, 4, 5, 6, 9, 10, 11, 12, 13):
        assert by[n] == {("A", 0, 12), ("A", 1, 12), ("B", -1, 12)}
    assert by[14] == {("A", 0, 8), ("A", 1, 8), ("B", -1, 8)}
    assert by[16] == {("A", 0, 4), ("A", 1, 4)} and by[20] == {("A", 0, 2), ("A", 1, 2)}
    odd = sorted((c.n, c.norm2) for c in R.CASES if c.norm2 not in (0.0, 1.0))
    assert odd == [(6, 0.37), (6, 2.5), (12, 0.37), (12, 2.5)]
    assert len({c.name for c in R.CASES}) == len(R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_margins_seeds_and_jump_counts(case):
    d = _data(case)
    assert len(d.seeds) == case.batch
    assert len(d.skipped) <= case.batch // 12, d.skipped  # at most 1 seed in 12
    for m in d.margins:
        assert min(m) >= R.MARGIN, m
    # the seeds that split differently into the key's words are used (as many of them as the batch has room for)
    used = [int(s) for s in d.seeds]
    for s in R.SPECIAL_SEEDS[:case.batch]:
        assert s in used or s in d.skipped
    counts = [len(j) for j in d.jumps]
    assert sum(counts) >= case.batch and max(counts) >= 2 and min(counts) == 0, counts
    # initial kets: the squared norm of the case; reference B never starts from a normalised ket
    for b in range(case.batch):
        n2 = float(np.prod(np.sum(np.abs(d.psi0[b]) ** 2, axis=-1))) if case.kind == "A" else float(np.vdot(d.psi0[b], d.psi0[b]).real)
        if case.kind == "A":
            assert abs(n2 - case.norm2) < 1e-12
        else:
            assert abs(n2 - 1.0) > 0.01


def test_every_operator_kind_is_selected():
    kinds = {R.KINDS[k] for c in R.CASES for j in _data(c).jumps for _, _, k in j}
    assert kinds == set(R.KINDS)


@pytest.mark.parametrize("n", sorted({c.n for c in R.CASES if c.n >= 10}))
def test_jumps_reach_both_ends_of_the_register(n):
    """From 10 atoms on: jumps on atom 0, on atom N - 1, on one of the top three bits (the register index of k_traj) and
    on one of the lowest six (the lane index)."""
    atoms = {a for c in R.CASES if c.n == n for j in _data(c).jumps for _, a, _ in j}
    assert 0 in atoms and n - 1 in atoms
    assert atoms & {0, 1, 2} and atoms & set(range(n - 6, n))


def _rerun(case, perturb):
    """The jump lists of the case's trajectories with every weight of the selection passed through ``perturb``."""
    d = _data(case)
    prob, steps = R._problem_and_steps(case.kind, case.n, case.model, case.scale)
    out = []
    for b, seed in enumerate(d.seeds):
        if case.kind == "A":
            out.append(R.product_trajectory(prob, d.psi0[b], R.GRID, R.EVAL, int(seed), props=steps, form_kets=False,
                                            perturb=perturb)[1])
        else:
            out.append(R.diagonal_trajectory(prob, d.psi0[b], R.GRID, R.EVAL, int(seed), factors=steps, perturb=perturb)[1])
    return d, out


def test_the_table_sees_weight_errors_from_about_one_percent():
    """What the device tests can detect, measured on the references: the weights are never read out, a wrong weight
    shows only as a flipped selection.  Weights off by +-1 % (alternating over the candidates) change the jump list of
    some trajectory of the table - the device tests would fail on it -, weights off by +-1e-6 change none: the margins
    of the table keep rounding differences between the device and the references from flipping anything."""
    changed = {0.01: 0, 1e-6: 0}
    for eps in changed:
        for case in R.CASES:
            d, jumps = _rerun(case, lambda a, k, w, eps=eps: w * (1 + eps * (1 if (a + k) % 2 else -1)))
            changed[eps] += sum(j != want for j, want in zip(jumps, d.jumps))
    print(f"trajectories whose jump list changes: {changed}")
    assert changed[0.01] >= 1 and changed[1e-6] == 0, changed


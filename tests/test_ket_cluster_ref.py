"""CPU checks of the cluster-product ket reference (tests/ket_cluster_ref.py) and of the case table that
tests/test_gpu_ket_clusters.py runs: no GPU.  Every test prints the figure it asserts."""
import numpy as np
import pytest

import ket_cluster_ref as R


def _plans(s):
    return R.PLANS.get(s.n, ("split",))


# ---------------------------------------------------------------------------------------------------------------------
# the reference against the full-space oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_cluster_product_equals_the_full_space_oracle_to_the_floor_of_two_tight_solves():
    """8 to 12 atoms, 20 ns, clusters interleaved over the atom indices: every family, both initial states, clusters of up
    to 6 atoms, both pitches, every evaluation time.  No two atoms are alike, so this is also the check that atom 0 is
    the highest bit."""
    setups = R.floor_setups()
    assert {s.family for s in setups} == set(R.FAMILIES) and {s.init for s in setups} == {"ket", "ground"}
    assert {s.pitch for s in setups} == {"blockade", "tight"} and {s.n for s in setups} == {8, 9, 10, 11, 12}
    assert all(s.ns == 20 for s in setups) and any(len(atoms) == 6 for s in setups for _, atoms in s.layout)
    for n in (8, 9):  # the whole cross of (family, initial state)
        assert len({(s.family, s.init) for s in setups if s.n == n}) == 6
    errs = [R.floor_error(s) for s in setups]
    amp, nrm = max(e[0] for e in errs), max(e[1] for e in errs)
    print(f"floor over {len(errs)} comparisons: max |cluster product - full space| = {amp:.2e}, 2-norm {nrm:.2e}")
    assert amp <= R.FLOOR_FACTOR * R.FLOOR_MEASURED[0] and nrm <= R.FLOOR_FACTOR * R.FLOOR_MEASURED[1], (amp, nrm)
    assert R.FLOOR_FACTOR * R.FLOOR_MEASURED[1] < 1e-3 * R.NORM_BAR  # far below what the device tests resolve


def test_a_bit_order_mistake_would_not_pass_the_floor():
    """The same comparison with atom 0 taken for the LOWEST bit is off by O(0.1): the floor test does check the order."""
    s = R.floor_setups()[0]
    times = R.eval_times(s.ns)[:2]
    full = R.full_space_solution(s, times)[-1]
    kets = [c[-1] for c in R.cluster_solutions(s, times)]
    wrong = tuple((name, tuple(s.n - 1 - a for a in atoms)) for name, atoms in s.layout)
    assert np.max(np.abs(R.product(wrong, kets, s.n).numpy() - full)) > 1e-2
    assert np.max(np.abs(R.product(s.layout, kets, s.n).numpy() - full)) < 1e-10


# ---------------------------------------------------------------------------------------------------------------------
# separation
# ---------------------------------------------------------------------------------------------------------------------
def test_cross_cluster_interaction_times_duration_is_negligible_in_every_case():
    worst = 0.0
    for (s, _), name in R.all_setups().items():
        sep = R.separation(s)
        worst = max(worst, sep)
        assert sep <= R.SEPARATION_BAR, (name, sep)
    print(f"separation: largest sum of cross-cluster U x duration = {worst:.2e} (bar {R.SEPARATION_BAR:g})")


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 10, 11, 12])
def test_product_by_index_arithmetic_equals_the_explicit_product(n):
    """Against an explicit Kronecker product + axis permutation, on a scrambled layout, with random (unnormalised)
    cluster kets."""
    rng = np.random.default_rng(n)
    layout = R.layout_of(n, R.PARTS[n], R.FLOOR_PERMS[n])
    flat = [a for _, atoms in layout for a in atoms]
    assert flat != sorted(flat)  # scrambled
    kets = [rng.normal(size=1 << len(atoms)) + 1j * rng.normal(size=1 << len(atoms)) for _, atoms in layout]
    got = R.product(layout, kets, n).numpy()
    # kron in cluster order, then an index map to the register's bit order
    k = np.ones(1, dtype=complex)
    for v in kets:
        k = np.kron(k, v)
    idx = np.arange(1 << n)
    f = np.zeros_like(idx)
    for p, a in enumerate(flat):
        f |= ((idx >> (n - 1 - a)) & 1) << (n - 1 - p)
    want = k[f]
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"evaluator n = {n}: largest relative deviation from the explicit product {rel:.1e}")
    assert rel <= 1e-15
    assert np.array_equal(want, R.product_numpy(R.Setup(n, layout), kets))  # (the outer-product route of the floor's psi(0))


def test_distances_from_cluster_kets_equal_the_full_space_distances():
    """:func:`product_distance` and :func:`exchange_distance` (what the motion and sensitivity figures are made of)."""
    n = 9
    s = R.Setup(n, R.layout_of(n, R.PARTS[n], R.FLOOR_PERMS[n]), seed=3)
    rng = np.random.default_rng(5)
    a = R.initial_kets(s)
    b = [v + 0.01 * (rng.normal(size=v.shape) + 1j * rng.normal(size=v.shape)) for v in a]
    pa, pb = R.product(s.layout, a, n).numpy(), R.product(s.layout, b, n).numpy()
    assert abs(R.product_distance(a, b) - np.linalg.norm(pa - pb)) < 1e-12
    x, y = s.layout[0][1][1], s.layout[1][1][2]
    moved = tuple((name, tuple(y if q == x else x if q == y else q for q in atoms)) for name, atoms in s.layout)
    assert abs(R.exchange_distance(s, a, x, y) - np.linalg.norm(pa - R.product(moved, a, n).numpy())) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# plans and coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_restated_from_the_host_code():
    """split_tile_bits / split_plan (host_split.hpp) and the ket plan of plan_passes (host_handle.hpp)."""
    assert [R.split_tile_bits(n) for n in (10, 15, 20, 21, 22, 23, 25)] == [10, 12, 12, 13, 13, 12, 12]
    assert [R.split_tile_bits(n, True) for n in (21, 22)] == [12, 12]
    assert {n: R.high_groups(n) for n in (15, 17, 20, 21, 22)} == \
        {15: [(12, 3)], 17: [(12, 5)], 20: [(12, 8)], 21: [(13, 8)], 22: [(13, 9)]}
    assert {n: R.high_groups(n) for n in (23, 24, 25)} == \
        {23: [(12, 5), (17, 6)], 24: [(12, 6), (18, 6)], 25: [(12, 6), (18, 7)]}
    assert R.high_groups(21, True) == [(12, 4), (16, 5)] and R.high_groups(22, True) == [(12, 5), (17, 5)]
    for n in range(13, 26):
        for small in (False, True):
            t = R.split_tile_bits(n, small)
            for til in R.split_plan(n, small)[1:]:  # every tiling keeps the low T - n_high bits, at least 4 of them, and fills a tile
                nh = sum(1 for b in til if b >= t)
                assert len(til) == t and til[:t - nh] == list(range(t - nh)) and t - nh >= 4, (n, small, til)
            assert sorted({b for til in R.split_plan(n, small) for b in til}) == list(range(n))
    # ryd_stats.passes: 1 up to 20 atoms and at 21 - 22, 2 at 23 - 25 atoms and with split_small_tiles at 21 - 22
    assert [R.split_passes(n) for n in range(10, 26)] == [1] * 13 + [2] * 3
    assert [R.split_passes(n, True) for n in (20, 21, 22, 23)] == [1, 2, 2, 2]
    assert R.bit_classes(R.split_plan(25), 25) == [[0, 1, 2, 3], [4, 5], list(range(6, 12)), list(range(12, 18)), list(range(18, 25))]
    assert R.bit_classes(R.split_plan(21), 21) == [[0, 1, 2, 3], [4], list(range(5, 13)), list(range(13, 21))]
    # k_apply: one launch (tile + outer bits) up to 128 MiB, 2^14 tiles + two passes of 5 high bits at 24 atoms
    assert R.apply_plan(17) == ([list(range(9)), list(range(9, 17))], 1)
    assert R.apply_plan(21) == ([list(range(12)), list(range(12, 21))], 1)
    assert R.apply_plan(24) == ([list(range(14)), list(range(7)) + list(range(14, 19)), list(range(7)) + list(range(19, 24))], 3)


def test_interacting_pairs_straddle_every_pair_of_bit_classes_of_every_plan():
    """For every register of the table and every plan it runs on: every pair of bit classes is straddled by an
    interacting pair, every class of two or more bits holds both members of one, every atom index is used once."""
    checked = 0
    for (s, _), name in R.all_setups().items():
        assert sorted(a for _, atoms in s.layout for a in atoms) == list(range(s.n)), name
        assert all(np.linalg.norm(np.subtract(R.SHAPES[nm][i], R.SHAPES[nm][j])) <= R.NEIGHBOUR + 1e-9
                   for nm, _ in s.layout for i, j in R.shape_pairs(nm))
        for plan, classes in R.plans_of(s.n, _plans(s)).items():
            assert sorted(b for c in classes for b in c) == list(range(s.n))
            assert R.coverage_gaps(s.n, s.pairs, classes) == [], (name, plan)
            checked += 1
    plans_run = {(c.n, c.plan) for c in R.CASES}
    assert all(p in R.PLANS[n] for n, p in plans_run), plans_run  # every plan a case runs is one its layout was built for
    print(f"coverage: {checked} (register, plan) combinations")
    # the condition is not empty: the unscattered 25-atom register misses most of it
    plain = R.Setup(25, R.layout_of(25, R.PARTS[25]))
    assert len(R.coverage_gaps(25, plain.pairs, R.bit_classes(R.split_plan(25), 25))) >= 5


def test_no_two_atoms_of_a_register_are_alike():
    for (s, _), name in R.all_setups().items():
        if s.family != "global":
            amps = [R.atom_waveform(s, c, k)["amp"] for c, (_, atoms) in enumerate(s.layout) for k in range(len(atoms))]
            assert len({a.tobytes() for a in amps}) == s.n, name
        if s.init == "ket":
            kets = [R.cluster_ket(s, c) for c in range(len(s.layout))]
            assert len({k.tobytes() for k in kets}) == len(kets), name


def test_the_table_holds_every_plan_of_the_issue():
    have = {(c.plan, c.n, c.setups[0].family) for c in R.CASES}
    for n in (15, 17, 20):
        assert {("split", n, "complex"), ("split", n, "real")} <= have
    assert ("split", 17, "global") in have
    for n in (21, 22):
        for family in ("real", "complex"):
            assert {("split", n, family), ("split-small", n, family)} <= have
    assert {("split", 23, "complex"), ("split", 25, "complex"), ("split", 10, "complex"), ("split", 13, "complex"),
            ("split", 14, "complex"), ("taylor", 17, "complex"), ("taylor", 21, "complex"), ("taylor", 24, "complex")} <= have
    assert any(len(c.setups) == 2 and c.n == 17 and c.setups[0].layout != c.setups[1].layout for c in R.CASES)
    assert any(dict(c.path).get("split_fixed") for c in R.CASES)
    assert {c.n for c in R.CASES if c.setups[0].init == "ground"} == {15, 21, 23}  # one per size class
    # one case with two evaluation times inside one knot interval
    assert any(any(int(a * 1e3) == int(b * 1e3) for a, b in zip(c.times, c.times[1:])) for c in R.CASES)
    # durations: 20 ns up to 20 atoms, 6 - 8 ns from 21 atoms on
    assert all(s.ns == 20 if s.n <= 20 else 6 <= s.ns <= 8 for s, _ in R.all_setups())
    # the registers are shared where a size is shared between plans
    for n in (17, 21):
        assert len({c.setups[0].layout for c in R.CASES if c.n == n and len(c.setups) == 1}) == 1
    assert len({c.name for c in R.CASES}) == len(R.CASES)


# ---------------------------------------------------------------------------------------------------------------------
# motion and sensitivity, from cluster solves alone
# ---------------------------------------------------------------------------------------------------------------------
def test_every_case_moves_and_its_interaction_matters():
    """|psi(T) - psi(0)|_2 >= 1e-2 and |psi(T) - psi(T) with the interaction matrix zeroed|_2 >= 1e-3: otherwise the 1e-7
    bars would not see a wrong drive or a wrong E0 entry."""
    mv = {name: R.motion(s, times) for (s, times), name in R.all_setups().items()}
    a, b = min(mv, key=lambda k: mv[k][0]), min(mv, key=lambda k: mv[k][1])
    print(f"motion: smallest |psi(T) - psi(0)|_2 = {mv[a][0]:.2e} ({a}); smallest effect of the interaction = {mv[b][1]:.2e} ({b})")
    assert mv[a][0] >= 1e-2 and mv[b][1] >= 1e-3


def test_sensitivity_to_exchanged_waveforms_and_to_an_atom_on_the_wrong_bit():
    """What the 2-norm bar of the device tests resolves, from the reference alone, at every size of the table (the short
    large-ket cases included): the waveforms of two atoms of different clusters exchanged, and an atom of one cluster
    placed on the bit of an atom of another cluster in another bit class, each change psi(T) by at least 100 bars."""
    worst_swap, worst_move = (np.inf, ""), (np.inf, "")
    for (s, times), name in R.all_setups().items():
        d_swap, d_move = R.sensitivity(s, times, _plans(s))
        if d_swap is not None:
            worst_swap = min(worst_swap, (d_swap, name))
        worst_move = min(worst_move, (d_move, name))
    print(f"sensitivity: exchanged waveforms >= {worst_swap[0]:.3g} bars ({worst_swap[1]}); "
          f"moved atom >= {worst_move[0]:.3g} bars ({worst_move[1]})")
    assert worst_swap[0] >= 100.0 and worst_move[0] >= 100.0

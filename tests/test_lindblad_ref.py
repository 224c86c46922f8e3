"""CPU checks of the cluster-product reference (tests/lindblad_ref.py) and of the case table that
tests/test_gpu_lindblad_edges.py runs: no GPU.  Every test prints the figure it asserts."""
import numpy as np
import pytest

import lindblad_ref as R

from pulser_amd import problem as P


def _all_setups():
    seen = {}
    for case in R.CASES:
        for s in case.setups:
            seen.setdefault((s, case.times), case.name)
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# the reference against the full-space oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_cluster_product_equals_the_full_space_oracle_to_the_floor_of_two_tight_solves():
    """4 atoms (2 + 2 interleaved), 5 (3 + 2), 6 (3 + 3 and 2 + 2 + 2 interleaved); every dissipator case, per-atom
    complex and real drives and the global drive, both initial states, every evaluation time.  The registers have no two
    atoms alike, so this is also the check that atom 0 is the highest bit."""
    setups = R.floor_setups()
    assert {s.diss for s in setups} == set(R.DISS_CASES) and {s.init for s in setups} == {"ket", "ground"}
    assert {s.family for s in setups} == set(R.FAMILIES) and {s.n for s in setups} == {4, 5, 6}
    for n in (4, 5):  # the whole cross of (dissipator, family, initial state)
        assert len({(s.diss, s.family, s.init) for s in setups if s.n == n and s.family != "global"}) == 24
    six = [s for s in setups if s.n == 6]  # every dissipator case with both families and both initial states, on both layouts
    assert {(s.diss, s.family) for s in six} == {(d, f) for d in R.DISS_CASES for f in ("complex", "real")}
    assert {(s.diss, s.init) for s in six} == {(d, i) for d in R.DISS_CASES for i in ("ket", "ground")}
    assert len({s.layout for s in six}) == 2
    errs = [R.floor_error(s) for s in setups]
    worst = int(np.argmax(errs))
    print(f"floor: max |cluster product - full space| over {len(errs)} comparisons = {errs[worst]:.2e} ({setups[worst]})")
    assert errs[worst] <= R.FLOOR_FACTOR * R.FLOOR_MEASURED, errs[worst]


def test_a_bit_order_mistake_would_not_pass_the_floor():
    """The same comparison with atom 0 taken for the LOWEST bit is off by O(0.1): the floor test does check the order."""
    n, parts, perm = R.FLOOR_LAYOUTS[1]
    s = R.Setup(n, R.layout_of(n, parts, perm), "all", "complex", "ket")
    full = R.full_space_solution(s, R.EVAL[:2])[-1]
    wrong = R.Setup(n, tuple((name, tuple(n - 1 - a for a in atoms)) for name, atoms in s.layout), "all", "complex", "ket")
    ref = R.references(wrong, R.EVAL[:2])[-1].full()
    assert np.max(np.abs(ref - full)) > 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# separation
# ---------------------------------------------------------------------------------------------------------------------
def test_cross_cluster_interaction_times_duration_is_negligible_in_every_case():
    worst = 0.0
    for (s, _), name in _all_setups().items():
        sep = R.separation(s)
        worst = max(worst, sep)
        assert sep <= R.SEPARATION_BAR, (name, sep)
        # the cached cluster solves use the cluster alone at the origin: same interaction, bit for bit
        u = np.asarray(R.assemble(s)["interaction_matrix"])
        for c_name, atoms in s.layout:
            bad_local = tuple(k for k, a in enumerate(atoms) if a in s.bad)
            one = R.Setup(len(atoms), ((c_name, tuple(range(len(atoms)))),), s.diss, s.family, s.init, s.pitch, bad_local)
            assert np.array_equal(u[:, list(atoms)][:, :, list(atoms)], R.assemble(one)["interaction_matrix"]), name
    one_pair = P.C6_LEVEL70 / R.CENTRE_PITCH ** 6
    print(f"separation: largest sum of cross-cluster U x duration = {worst:.2e} (bar {R.SEPARATION_BAR:g}); one pair at "
          f"{R.CENTRE_PITCH:g} um: {one_pair:.2e} rad/us")
    assert 5e-12 < one_pair < 6e-12


def test_60_um_between_clusters_is_not_non_interacting():
    """Why the clusters are 1000 um apart: two interleaved 3-atom clusters, per-atom drives, all five collapse
    operators, 40 ns.  With the centres 60 um apart - the spacing the older product-state tests call non-interacting
    (there: 8 ns, identical atoms) - the product of the cluster solutions is off the full solution by 5.4e-6 (sum of the
    cross-cluster U x 40 ns: 1.0e-4), fifty times the 1e-7 bar; at 300 um by 1.4e-10 (3.0e-9).  The deviation is bounded by
    the summed phase, which is what the separation condition of the table (<= 1e-10) rests on."""
    n, parts, perm = R.FLOOR_LAYOUTS[2]
    out = {}
    for pitch in (60.0, 300.0):
        s = R.Setup(n, R.layout_of(n, parts, perm), "all", "complex", "ket", centre_pitch=pitch)
        out[pitch] = (R.floor_error(s, (0.0, 0.04)), R.separation(s))
    print(f"60 um: |product - full| = {out[60.0][0]:.2e} (sum U x T = {out[60.0][1]:.2e}); "
          f"300 um: {out[300.0][0]:.2e} ({out[300.0][1]:.2e})")
    assert out[60.0][0] > R.BAR
    for pitch in out:
        assert out[pitch][0] <= out[pitch][1] + R.FLOOR_FACTOR * R.FLOOR_MEASURED


# ---------------------------------------------------------------------------------------------------------------------
# structured evaluators
# ---------------------------------------------------------------------------------------------------------------------
def _explicit_product(n, layout, mats):
    """kron of the cluster matrices in cluster order, then an index map to the register's bit order."""
    k = np.ones((1, 1), dtype=complex)
    for m in mats:
        k = np.kron(k, m)
    flat = [a for _, atoms in layout for a in atoms]
    idx = np.arange(1 << n)
    f = np.zeros_like(idx)
    for p, a in enumerate(flat):
        f |= ((idx >> (n - 1 - a)) & 1) << (n - 1 - p)
    return k[np.ix_(f, f)]


@pytest.mark.parametrize("n", [6, 7, 8])
def test_structured_evaluators_equal_the_explicit_product(n):
    rng = np.random.default_rng(n)
    layout = R.default_layout(n)
    assert [a for _, atoms in layout for a in atoms] != list(range(n))  # scrambled
    mats = []
    for name, atoms in layout:
        d = 1 << len(atoms)
        mats.append(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))  # not Hermitian, trace not 1
    ref = R.Reference(n, layout, mats)
    rho = _explicit_product(n, layout, mats)
    scale = np.max(np.abs(rho))
    D = 1 << n
    worst = {}
    worst["full"] = np.max(np.abs(ref.full() - rho)) / scale
    r, c = rng.integers(0, D, 500), rng.integers(0, D, 500)
    worst["entries"] = np.max(np.abs(ref.entries(r, c) - rho[r, c])) / scale
    rows = rng.choice(D, 7, replace=False)
    worst["rows"] = np.max(np.abs(ref.rows(rows) - rho[rows])) / scale
    worst["diagonal"] = np.max(np.abs(ref.diagonal() - np.diagonal(rho))) / scale
    worst["trace"] = abs(ref.trace() - np.trace(rho)) / abs(np.trace(rho))
    idx = np.arange(D)
    herm = R.Reference(n, layout, [m @ m.conj().T for m in mats])  # (occupations are reported as real numbers)
    rho_h = _explicit_product(n, layout, herm.mats)
    occ_h = np.array([np.sum(np.diagonal(rho_h)[((idx >> (n - 1 - a)) & 1) == 0]).real for a in range(n)])
    worst["occupations"] = np.max(np.abs(herm.occupations() - occ_h)) / np.max(np.abs(occ_h))
    v = R.probe_vectors(n)
    assert np.allclose(np.linalg.norm(v, axis=0), 1.0, atol=1e-15)
    worst["matmul"] = np.max(np.abs(ref.matmul(v) - rho @ v)) / np.max(np.abs(rho @ v))
    print(f"evaluators n = {n}: " + ", ".join(f"{k} {e:.1e}" for k, e in worst.items()))
    assert max(worst.values()) <= 1e-14, worst


def test_product_ket_is_the_explicit_product():
    for n in (5, 8):
        s = R.Setup(n, R.default_layout(n))
        psi = R.product_ket(s)
        mats = [np.outer(R.species_ket(R.SPECIES[name], "ket"), R.species_ket(R.SPECIES[name], "ket").conj())
                for name, _ in s.layout]
        assert np.max(np.abs(np.outer(psi, psi.conj()) - _explicit_product(n, s.layout, mats))) < 1e-15
        assert abs(np.linalg.norm(psi) - 1.0) < 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_no_two_atoms_of_a_register_are_alike():
    for (s, _), name in _all_setups().items():
        kinds = [(c_name, k) for c_name, atoms in s.layout for k in range(len(atoms))]
        assert sorted(a for _, atoms in s.layout for a in atoms) == list(range(s.n)), name
        if s.family != "global":  # (one global drive: the atoms differ by their geometry and initial ket only)
            assert len(set(kinds)) == len(kinds), name
        assert len({c_name for c_name, _ in s.layout}) == len(s.layout), name  # distinct species: every size allows it


def test_pair_pass_grouping_restated_from_the_host_code():
    """plan_passes (host_handle.hpp) at the sizes of the table: tile sizes and atoms per pass."""
    assert [R.auto_tile_bits(2 * n) for n in (8, 9, 10, 11, 12, 13, 14)] == [10, 11, 12, 12, 12, 12, 12]
    assert [[len(g) for g in R.pair_pass_groups(n)] for n in (8, 9, 10, 11, 12, 13, 14)] == \
        [[5, 3], [5, 3, 1], [6, 4], [6, 4, 1], [6, 4, 2], [6, 4, 3], [6, 4, 4]]
    assert R.pair_pass_groups(10)[0] == [9, 8, 7, 6, 5, 4]  # from the low-bit end: atom N - 1 first
    assert [len(g) for g in R.pair_pass_groups(11, batch=2)] == [6, 4, 1]
    assert [len(g) for g in R.pair_pass_groups(5, tile_bits=6)] == [3, 1, 1]
    assert [len(g) for g in R.pair_pass_groups(7, tile_bits=7)] == [3, 2, 1, 1]


def test_clusters_straddle_every_pair_pass_boundary_and_join_both_ends():
    """At 8 to 14 atoms: for each boundary between two pair passes at least TWO clusters have atoms on both sides (the
    cluster that holds atoms 0 and N - 1 always has; a second one makes the interacting pairs cross it elsewhere too),
    and atoms 0 and N - 1 share a cluster at every size."""
    sizes = {}
    for (s, _), name in _all_setups().items():
        both_ends = any(0 in atoms and s.n - 1 in atoms for _, atoms in s.layout)
        sizes[s.n] = sizes.get(s.n, False) or both_ends
        if s.n < 8:
            continue
        groups = R.pair_pass_groups(s.n)
        for k in range(1, len(groups)):
            low = {a for g in groups[:k] for a in g}
            n_straddle = sum(1 for _, atoms in s.layout if 0 < len(low & set(atoms)) < len(atoms))
            want = 2 if min(len(low), s.n - len(low)) >= 2 else 1  # (one atom alone beyond the boundary: its cluster only)
            assert n_straddle >= want, (name, k, groups, s.layout)
    assert all(sizes.values()) and set(sizes) == set(range(4, 15)), sizes


def test_every_plan_of_the_issue_appears_at_every_size_named():
    have = {(c.plan, c.n) for c in R.CASES}
    want = {("persistent", 4), ("persistent", 5), ("persistent", 6), ("tiled", 5), ("tiled", 7), ("tiled", 8), ("tiled", 9),
            ("tiled-single-launch", 7), ("hermitian", 7), ("hermitian", 8), ("hermitian", 9), ("hermitian", 10),
            ("rows-ket", 10), ("rows-ket", 11), ("rows-ket", 12), ("rows-ket", 13), ("rows-ket", 14),
            ("rows-ket-by-estimate", 12), ("rows-split", 12), ("rows-split", 13), ("rows-split", 14),
            ("rows-local-exp", 10), ("rows-local-exp", 11), ("rows-local-exp", 12), ("rows-local-exp", 13),
            ("rows-local-exp", 14), ("pair-passes", 10), ("pair-passes", 11)}
    assert have == want, have ^ want
    for n in (10, 11, 12, 13):
        assert {c.setups[0].diss for c in R.CASES if c.plan == "rows-local-exp" and c.n == n} == set(R.DOUBLE_FLIP)
    assert len({c.name for c in R.CASES}) == len(R.CASES)


def test_every_case_moves_and_its_dissipator_matters():
    """|rho(t_end) - rho(0)| > 1e-3 and |rho(t_end) - rho(t_end) without collapse operators| > 1e-5 (max-abs over what the
    device test compares): otherwise the 1e-7 bar would not see a wrong drive or a wrong rate."""
    moved, diss = {}, {}
    for (s, times), name in _all_setups().items():
        moved[name], diss[name] = R.motion(s, times)
    a, b = min(moved, key=moved.get), min(diss, key=diss.get)
    print(f"motion: smallest |rho(T) - rho(0)| = {moved[a]:.2e} ({a}); smallest effect of the dissipator = {diss[b]:.2e} ({b})")
    assert moved[a] > 1e-3 and diss[b] > 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------------------------------------
def _compared_values(s, refs):
    if s.n <= 9:
        return refs.full().ravel()
    r, c = R.compared_entries(s)
    return np.concatenate([refs.entries(r, c), refs.rows(R.compared_rows(s.n)).ravel(), refs.diagonal()])


@pytest.mark.parametrize("n", [6, 10, 14])
def test_sensitivity_to_a_swapped_waveform_and_to_a_wrong_rate(n):
    """What the 1e-7 bar of the device tests resolves, from the reference alone ("all", real drives):

    * the waveforms of two atoms of different clusters exchanged: more than 100 bars at every size (measured 6 / 10 /
      14 atoms: 2.6e5 / 3.8e4 / 3.6e3 bars);
    * the relaxation RATE scaled by 1 + 1e-3.  The change is bounded by 1e-3 x rate x time x |rho_ij| = 1e-3 x 0.07 /us x
      0.04 us x |rho_ij| <= 2.8e-6 |rho_ij| (the fastest rate of the table, dephasing at 0.2 / us over four flipped atoms of
      an entry of size 1/4, gives 8e-6): a thousandth of a rate can never move an entry by 100 bars = 1e-5 in 40 ns, so
      the figure is recorded, not held to that: 6 atoms 6.5 bars, 10 atoms 2.1 bars, 14 atoms (20 ns) 0.37 bars.  A rate
      error is seen by the device tests from 1e-3 x (1 bar / that figure) relative on: 0.015 % at 6 atoms, 0.05 % at 10,
      0.27 % at 14 - the small registers carry the rates, the large ones the indexing.  Asserted: the change is linear in
      the rate error and at least RATE_FLOOR bars at each size, i.e. the figures above do not silently shrink."""
    times = R.EVAL if n <= 12 else R.EVAL_BIG
    s = R.Setup(n, R.default_layout(n), "all", "real", "ket")
    base = _compared_values(s, R.references(s, times)[-1])

    def edited(edit):
        prob = R.assemble(s)
        edit(prob)
        sols = R.solve_problem_clusters(prob, s, times)
        return _compared_values(s, R.Reference(n, s.layout, [m[-1] for m in sols]))

    # self-check of the route: the unedited problem through the same function is the cached reference, bit for bit
    assert np.array_equal(edited(lambda prob: None), base)

    def swap(prob):
        a, b = s.layout[0][1][0], s.layout[1][1][0]
        loc = prob["samples"]["Local"]["ground-rydberg"]
        loc[a], loc[b] = loc[b], loc[a]

    def rate(eps):
        def edit(prob):
            prob["collapse_ops"] = [(c * np.sqrt(1 + eps) if k == "sigma_gr" else c, k) for c, k in prob["collapse_ops"]]
        return edit

    d_swap = float(np.max(np.abs(edited(swap) - base))) / R.BAR
    d_rate = float(np.max(np.abs(edited(rate(1e-3)) - base))) / R.BAR
    d_rate10 = float(np.max(np.abs(edited(rate(1e-2)) - base))) / R.BAR
    print(f"sensitivity n = {n}: swapped waveforms {d_swap:.3g} bars; relaxation rate x (1 + 1e-3): {d_rate:.3g} bars, "
          f"x (1 + 1e-2): {d_rate10:.3g} bars")
    assert d_swap > 100.0
    assert 9.0 < d_rate10 / d_rate < 11.0
    assert d_rate > RATE_FLOOR[n]


# half of what `python -m pytest -s tests/test_lindblad_ref.py` printed when the table was written
RATE_FLOOR = {6: 3.0, 10: 1.0, 14: 0.18}

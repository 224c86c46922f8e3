"""The two-level quantum-jump kernels (``ryd_mc_solve``) against exact trajectories on every plan.

Every case of the table in tests/mcwf_ref.py is run on every plan that serves its size and compared, trajectory by
trajectory, with one of two references that use a structure the kernels know nothing about (tests/mcwf_ref.py;
tests/test_mcwf_ref.py pins both on the full-space restatement of ``oracle/mcwf.py`` and checks the table):

* A, product reference: driven atoms without interaction from a product ket - per-atom complex drives (``k_traj<.., MODEL
  0, true>``) and one global real drive (``MODEL 1``);
* B, diagonal reference: interacting, undriven atoms with time-dependent detunings from a random entangled ket that is
  not normalised.

Plans: the persistent kernel and the multi-launch chain at 1, 4, 5, 6, 9 - 13 atoms (idle lanes below 6 atoms, one
amplitude per thread at 6 - 9, two at 10 and 11, four at 12, eight at 13); the 2^14 register-tile plan, the tiled one- and
two-pass plans and the register-resident split-operator kernel at 14; the split-operator passes at 16 and 20 (reference A
only).  Batches of 12 / 8 / 4 / 2 trajectories over 60 one-nanosecond steps, stored at 0.02 and 0.06 us; the seeds include
0, 2^32 - 1, 2^32 and 2^64 - 1; four cases start from kets of squared norm 0.37 and 2.5.

Per trajectory: the number of jumps is the reference's; every stored ket and the final state are within the parity bar
of 1e-7 (``test_trajectories_match_cpu_restatement``) of the reference - a trajectory that jumps at another step, atom
or operator is off by O(0.1) - and have norm 1 to 1e-12.

What this does and does not detect: the weights are never read out, so an error in them shows only as a flipped
selection.  A relative error eps flips about eps x (number of candidates) of the jumps; sign and index errors in
``mc_weight`` and the coherence sums are O(1) on these inputs (random product kets and entangled kets carry a large
rho_rg).  The table holds several hundred jumps per plan family, so errors from about 1 % up are caught and smaller ones
are not.
"""
import numpy as np
import pytest

import mcwf_ref as R

from pulser_amd.engine import Engine
from pulser_amd.terms import lower

pytestmark = pytest.mark.gpu

PARITY = 1e-7
# plan -> (set_path arguments, method); the 14-atom Taylor plans are those of
# test_quantum_jumps_on_register_tile_and_tiled_kernels_agree
PLANS = {
    "persistent": (dict(force_generic=False), "auto"),
    "multi-launch": (dict(force_generic=True), "auto"),
    "tile14": (dict(force_generic=False, no_tile14=False, no_single_pass=False), "taylor"),
    "tiled-one-pass": (dict(force_generic=False, no_tile14=True, no_single_pass=False), "taylor"),
    "tiled-two-pass": (dict(force_generic=False, no_tile14=True, no_single_pass=True), "taylor"),
    "split": (dict(force_generic=False), "auto"),
}


def _plans_of(n):
    if n <= 13:
        return ["persistent", "multi-launch"]
    if n == 14:
        return ["tile14", "tiled-one-pass", "tiled-two-pass", "split"]
    return ["split"]


PARAMS = [pytest.param(c, p, id=f"{c.name}-{p}") for c in R.CASES for p in _plans_of(c.n)]


@pytest.mark.parametrize("case,plan", PARAMS)
def test_trajectories_match_the_exact_reference(case, plan):
    d = R.case_data(case)
    path, method = PLANS[plan]
    with Engine(lower([d.problem] * case.batch), mode="mcsolve") as eng:
        eng.set_path(**path)
        state = eng.new_state(d.psi0)
        snaps = eng.mc_solve(state, R.EVAL, d.seeds, method=method).cpu().numpy()
        counts = eng.mc_jumps()
        final = state.cpu().numpy()
        stats = eng.stats()
    worst, defect = 0.0, 0.0
    for b in range(case.batch):
        for i in (1, 2):
            worst = max(worst, float(np.max(np.abs(snaps[i - 1][b] - d.kets[b][i]))))
            defect = max(defect, abs(float(np.linalg.norm(snaps[i - 1][b])) - 1.0))
        worst = max(worst, float(np.max(np.abs(final[b] - d.kets[b][-1]))))
        defect = max(defect, abs(float(np.linalg.norm(final[b])) - 1.0))
    want = [len(j) for j in d.jumps]
    print(f"mcwf-edges {case.name} {plan}: worst |hip - ref| = {worst:.2e}, norm defect {defect:.1e}, "
          f"{case.batch} trajectories, {sum(want)} jumps, device counts {counts.tolist()}, skipped seeds {len(d.skipped)}, "
          f"n_steps {stats['n_steps']}, launches {stats['n_launches']}, passes {stats['passes']}, "
          f"reference {d.cpu_seconds:.1f} s")
    assert counts.tolist() == want, (counts.tolist(), want, d.jumps)
    assert worst < PARITY, worst
    assert defect < 1e-12, defect
    if plan == "persistent":
        assert stats["n_launches"] == 1
    elif plan == "multi-launch":
        assert stats["n_launches"] > 100
    elif plan != "split":
        assert stats["passes"] == (2 if plan == "tiled-two-pass" else 1)
    else:
        assert stats["passes"] in (1, 2)
    # one step per sample interval, never a merged one (the split-operator passes count their schedule steps, after
    # each of which the threshold is tested, in the same field)
    assert stats["n_steps"] == 60, stats

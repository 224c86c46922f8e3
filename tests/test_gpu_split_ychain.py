"""-m gpu: the y chain of k_split_reg (SPLITR_YCHAIN; pulser_amd/csrc/split_ychain.hpp) on per-atom REAL drives.

With a real drive only the imaginary parts travel over the DPP crossbar, hop by hop from one lane direction to the next,
and the last hop rides on the stores of the LDS pass.  A global drive has the same tan T on every index bit and cannot see
bits rotated in the wrong order or with each other's coefficient, so the drives here are local: every atom its own amplitude
and detuning (`local_problem` of tests/test_gpu_split.py with the phases set to 0 - a phase would be gauged into the D
factors and is beside the point).  12 atoms run <12, 4> (four DPP bits, 16 amplitudes per lane), 13 atoms <13, 5> (three DPP
bits, the LDS transposition), 14 atoms <14, 5> (four DPP bits, 32 amplitudes per lane).

Checkers, with the bounds of the sibling tests of tests/test_gpu_split.py: the same stages launched pass by pass
(`split_no_loop`: the tile kernels, no DPP chain at all) to rounding, 1e-12, and CF4 + Taylor at tol 1e-13 on the
generator kernels (`no_ket`) to 5e-9.

Two end times per size.  The compositions have 6 and 10 stages, so a closed ket run always ends after an EVEN number of
full stages (the odd closing layout and its store map are reached only by the density-matrix rows that open with a kick:
tests/test_gpu_ket.py); inside a run the layouts alternate stage by stage, and both are met from the first sub-step on.
The two end times give runs of different lengths and different cuts by the step-size controller (measured at 14 atoms:
1 080 stages in 30 launches for 21 ns, 1 548 in 42 for 30 ns; 12 atoms 996 / 1 428, 13 atoms 1 032 / 1 464), far beyond 3
sub-steps of 6 stages per run; the stage counts are printed and the lower bound asserted."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_split import local_problem

pytestmark = pytest.mark.gpu

END_TIMES = (0.021, 0.030)


def _engine(probs):
    from pulser_amd.engine import Engine

    return Engine.from_problems(probs, mode="sesolve")


def real_local_problem(n, seed):
    prob = local_problem(n, seed=seed, duration=41, spacing=6.5)
    for drive in prob["samples"]["Local"]["ground-rydberg"].values():
        drive["phase"] = np.zeros_like(drive["phase"])
    return prob


@pytest.fixture(scope="module")
def problems():
    return {n: [real_local_problem(n, seed=3 + 10 * b + n) for b in range(2)] for n in (12, 13, 14)}


@pytest.mark.parametrize("t_end", END_TIMES)
@pytest.mark.parametrize("n", [12, 13, 14])
def test_y_chain_on_per_atom_real_drives_against_the_passes_and_taylor(problems, n, t_end):
    probs = problems[n]
    outs, stats = {}, {}
    for name, kw, method, opts in (("loop", {}, "split", {}), ("passes", {"split_no_loop": True}, "split", {}),
                                   ("taylor", {"no_ket": True}, "taylor", {"tol": 1e-13})):
        with _engine(probs) as eng:
            eng.set_path(False, **kw)
            st = eng.new_state()
            eng.evolve(st, 0.0, t_end, method=method, **opts)
            outs[name], stats[name] = st.cpu().numpy(), eng.stats()
    gap_passes = float(np.max(np.abs(outs["loop"] - outs["passes"])))
    gap_taylor = float(np.max(np.abs(outs["loop"] - outs["taylor"])))
    print(f"n={n} t_end={t_end}: stages {stats['loop']['n_applications']} in {stats['loop']['n_launches']} launches "
          f"(passes: {stats['passes']['n_applications']} in {stats['passes']['n_launches']}); "
          f"|loop - passes| = {gap_passes:.2e}, |loop - taylor| = {gap_taylor:.2e}")
    # the register-resident kernel ran, whole runs per launch, the same stages as the passes; >= 3 sub-steps of 6 stages
    assert stats["loop"]["n_applications"] == stats["passes"]["n_applications"] >= 18
    assert stats["loop"]["n_applications"] % 2 == 0
    assert stats["loop"]["n_launches"] < stats["passes"]["n_launches"] / 15
    assert gap_passes < 1e-12
    assert gap_taylor < 5e-9
    assert np.max(np.abs(outs["loop"][0] - outs["loop"][1])) > 1e-3  # the sequences really differ
    assert np.max(np.abs(np.linalg.norm(outs["loop"], axis=1) - 1.0)) < 1e-11


def test_y_chain_snapshots_inside_a_run_equal_a_closed_run_per_evaluation_time(problems):
    """14 atoms, four evaluation times inside the sequence (k_split_reg<14, 5, .., SNAP>: the registers are stored after
    the stage that ends a sub-step - every y must be home there) against a run that closes at every evaluation time, to
    rounding as in test_snapshots_stored_inside_a_run_equal_a_closed_run_per_evaluation_time."""
    probs = problems[14]
    times = np.array([0.0, 0.004, 0.009, 0.015, 0.022, 0.03])
    outs, stats = {}, {}
    for name, kw, opts in (("inside", {}, {}), ("outside", {"snaps_outside": True}, {"method": "split"})):
        with _engine(probs) as eng:
            eng.set_path(False, **kw)
            outs[name] = eng.solve(eng.new_state(), times, **opts).cpu().numpy()
            stats[name] = eng.stats()
    gap = float(np.max(np.abs(outs["inside"] - outs["outside"])))
    print(f"snapshots: inside {stats['inside']['n_applications']} stages in {stats['inside']['n_launches']} launches, outside "
          f"{stats['outside']['n_applications']} in {stats['outside']['n_launches']}; |inside - outside| = {gap:.2e}")
    assert outs["inside"].shape == (5, 2, 1 << 14)
    assert stats["inside"]["reserved"][0] > 0  # the split-operator path ran
    assert stats["inside"]["n_launches"] < stats["outside"]["n_launches"]  # runs, not a run per evaluation time
    assert gap < 1e-12

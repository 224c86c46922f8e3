"""GPU: k_split_reg with lane bits 4, 5 exchanged inside the LDS pass (SPLITR_XPASS; profiles/xpass.md) computes what the
pass-by-pass launches compute - 12 and 14 atoms take the new layout (the snapshot kernel at 12 atoms only: at 14 it keeps
the swaps), 13 atoms (three T bits: the LDS transposition) are the untouched control.  Triangular register, per-atom different amplitudes and detunings (a wrong select of the detuning sum, a
wrong sign of a flipped T atom or a wrong copy of the G table changes the ket), three sequences per launch.

  * runs of several lengths (one short sub-step up to the whole ramp: different numbers of S6 / S10 sub-steps per run)
    against the pass-by-pass launches with the same stages, to 1e-12 (the bound tests/test_gpu_split_reg_waits.py uses);
  * an evaluation time inside a run (the snapshot store from the registers) against a closed run per evaluation time, 1e-12;
  * the controller's check through the fused epilogue (out-of-place store, second store, comparison): state and booked
    estimate against the pass-by-pass path's.

The compositions have 6 or 10 stages, so a plain run closes after an even number of full stages: on the device every load,
store and snapshot of these kernels happens in the even layout; the odd one lives between two stages only and is covered by
the comparison of whole runs (every second stage runs in it) and by the replay of tests/test_split_xpass_layout.py."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import blockade_radius
from pulser_amd import problem as P
from pulser_amd.engine import Engine

pytestmark = pytest.mark.gpu

T = 81  # samples: 80 ns
LENGTHS = (0.004, 0.023, 0.05, 0.08)  # us


def _ramp_problem(n, seed):
    """Per-atom REAL drives (phase 0) ramping up from zero, per-atom detunings ramping through resonance."""
    rng = np.random.default_rng(seed)
    s = np.arange(T) / (T - 1.0)
    coords = P.register_coords(P.triangular_rect(2, 7)[:n], blockade_radius())
    z = np.zeros(T)
    prob = P.make_ising_problem(coords, {"amp": z, "det": z, "phase": z})
    loc = {}
    for q in range(n):
        a, d0, d1 = rng.uniform(4, 12), rng.uniform(-14, -6), rng.uniform(2, 10)
        loc[q] = {"amp": a * s, "det": d0 + (d1 - d0) * s, "phase": z}
    prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": loc}}
    prob["collapse_ops"] = []
    prob["depolarizing_pauli_2ds"] = {}
    return prob


def _probs(n):
    return [_ramp_problem(n, seed=1000 + 100 * n + b) for b in range(3)]


@pytest.fixture(scope="module")
def runs():
    """{n: {path: [(state, stats) per length]}}: every length from t = 0 on a fresh state, one engine per path."""
    out = {}
    for n in (12, 13, 14):
        out[n] = {}
        for name, kw in (("loop", {}), ("passes", {"split_no_loop": True})):
            with Engine.from_problems(_probs(n), mode="sesolve") as eng:
                eng.set_path(False, **kw)
                res = []
                for t1 in LENGTHS:
                    eng.reset_stats()
                    st = eng.new_state()
                    eng.evolve(st, 0.0, t1, method="split")
                    res.append((st.cpu().numpy(), eng.stats()))
                out[n][name] = res
    return out


@pytest.mark.parametrize("n", [12, 13, 14])
@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_default_kernel_equals_the_pass_by_pass_launches(runs, n, k):
    (loop, s_loop), (passes, s_pass) = runs[n]["loop"][k], runs[n]["passes"][k]
    diff = float(np.max(np.abs(loop - passes)))
    print(f"n = {n}, {LENGTHS[k] * 1e3:.0f} ns: max |loop - passes| = {diff:.3e}; stages {s_loop['n_applications']} / "
          f"{s_pass['n_applications']}; launches {s_loop['n_launches']} / {s_pass['n_launches']}")
    assert diff < 1e-12
    assert s_loop["n_applications"] == s_pass["n_applications"]
    assert s_loop["n_launches"] < s_pass["n_launches"]  # the register-resident kernel ran
    assert np.allclose(np.linalg.norm(loop, axis=-1), 1.0, atol=1e-12)
    if LENGTHS[k] >= 0.02:
        assert np.max(np.abs(loop[0] - loop[1])) > 1e-3  # the sequences really differ


@pytest.mark.parametrize("n", [12, 13, 14])
def test_controller_check_through_the_fused_epilogue_books_what_the_passes_book(runs, n):
    """The whole ramp takes at least two runs and a step-size check: the check's launch stores out of place, stores a
    second copy and compares on the way out.  The estimate is a norm of differences of kets that agree to 1e-12."""
    (loop, s_loop), (passes, s_pass) = runs[n]["loop"][-1], runs[n]["passes"][-1]
    est, est_p = s_loop["reserved"][0], s_pass["reserved"][0]
    print(f"n = {n}: booked estimate {est:.6e} / {est_p:.6e}; steps {s_loop['n_steps']} / {s_pass['n_steps']}")
    assert est > 0 and est_p > 0  # the controller checked and booked
    assert abs(est - est_p) < 1e-12
    assert s_loop["n_steps"] == s_pass["n_steps"]
    assert float(np.max(np.abs(loop - passes))) < 1e-12


@pytest.mark.parametrize("n", [12, 13, 14])
def test_a_snapshot_inside_a_run_equals_a_closed_run_per_evaluation_time(n):
    times = np.array([0.0, 0.011, 0.03, 0.08])
    outs, stats = {}, {}
    for name, kw, opts in (("inside", {}, {}), ("outside", {"snaps_outside": True}, {"method": "split"})):
        with Engine.from_problems(_probs(n), mode="sesolve") as eng:
            eng.set_path(False, **kw)
            outs[name] = eng.solve(eng.new_state(), times, **opts).cpu().numpy()
            stats[name] = eng.stats()
    diff = float(np.max(np.abs(outs["inside"] - outs["outside"])))
    print(f"n = {n}: max |inside - outside| = {diff:.3e}; launches {stats['inside']['n_launches']} / {stats['outside']['n_launches']}")
    assert stats["inside"]["reserved"][0] > 0  # the split-operator path ran
    assert diff < 1e-12

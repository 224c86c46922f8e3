"""GPU: the stage loop of k_split_reg with its memory waits moved (SPLITR_KWARM 2, SPLITR_GAHEAD; profiles/stage_waits.md)
computes what it computed - every instantiation of the one stage body against a path that does not run it:

  * the default kernel against the pass-by-pass launches (12, 13, 14 atoms), same stage count;
  * an evaluation time inside a run (SNAP) against a closed run per evaluation time;
  * a dephasing row pass (ROWS) against the k_ket rows;
  * a quantum-jump solve (DECAY) against the CF4 + Taylor path: same jumps, unit norms.

Small on purpose: 3 sequences with per-atom real drives over 80 ns of a ramp (at least two runs and a controller check)."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import DEPOL_PAULIS, blockade_radius
from pulser_amd import problem as P
from pulser_amd.engine import Engine
from pulser_amd.terms import lower

pytestmark = pytest.mark.gpu

T = 81  # samples: 80 ns


def _ramp_problem(n, seed, collapse_ops=None, paulis=None):
    """Per-atom REAL drives (phase 0) ramping up from zero, per-atom detunings ramping through resonance."""
    rng = np.random.default_rng(seed)
    s = np.arange(T) / (T - 1.0)
    coords = P.register_coords(P.triangular_rect(2, 7) if n == 14 else P.square_rect(1, n), blockade_radius())
    z = np.zeros(T)
    prob = P.make_ising_problem(coords, {"amp": z, "det": z, "phase": z})
    loc = {}
    for q in range(n):
        a, d0, d1 = rng.uniform(4, 12), rng.uniform(-14, -6), rng.uniform(2, 10)
        loc[q] = {"amp": a * s, "det": d0 + (d1 - d0) * s, "phase": z}
    prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": loc}}
    prob["collapse_ops"] = list(collapse_ops or [])
    prob["depolarizing_pauli_2ds"] = dict(paulis or {})
    return prob


def _probs(n):
    return [_ramp_problem(n, seed=100 * n + b) for b in range(3)]


@pytest.mark.parametrize("n", [12, 13, 14])
def test_default_kernel_equals_the_pass_by_pass_launches(n):
    outs, stats = {}, {}
    for name, kw in (("loop", {}), ("passes", {"split_no_loop": True})):
        with Engine.from_problems(_probs(n), mode="sesolve") as eng:
            eng.set_path(False, **kw)
            st = eng.new_state()
            eng.evolve(st, 0.0, (T - 1) * 1e-3, method="split")
            outs[name], stats[name] = st.cpu().numpy(), eng.stats()
    diff = float(np.max(np.abs(outs["loop"] - outs["passes"])))
    print(f"n = {n}: max |loop - passes| = {diff:.3e}; stages {stats['loop']['n_applications']} / {stats['passes']['n_applications']}; "
          f"launches {stats['loop']['n_launches']} / {stats['passes']['n_launches']}")
    assert diff < 1e-12
    assert stats["loop"]["n_applications"] == stats["passes"]["n_applications"]
    assert stats["loop"]["n_launches"] < stats["passes"]["n_launches"]  # the register-resident kernel ran
    assert np.max(np.abs(outs["loop"][0] - outs["loop"][1])) > 1e-3  # the sequences really differ


@pytest.mark.parametrize("n", [12, 13, 14])
def test_an_evaluation_time_inside_a_run_equals_a_closed_run_per_evaluation_time(n):
    times = np.array([0.0, 0.03, 0.08])
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


def test_dephasing_row_pass_equals_the_k_ket_rows():
    ops = [(float(np.sqrt(2 * 0.05)), "sigma_rr")]
    prob = P.make_ising_problem(P.register_coords(P.triangular_rect(2, 6), blockade_radius()), P.anneal_samples(), collapse_ops=ops)
    outs, stats = {}, {}
    for rows_ket in (False, True):
        with Engine.from_problems([prob], mode="mesolve") as eng:
            eng.set_path(False, rows_ket=rows_ket)
            st = eng.new_state()
            eng.evolve(st, 0.0, 0.008)
            outs[rows_ket], stats[rows_ket] = st.cpu().numpy()[0], eng.stats()
    diff = float(np.max(np.abs(outs[False] - outs[True])))
    print(f"rows: max |split rows - k_ket rows| = {diff:.3e}; last_order {stats[False]['last_order']}")
    assert stats[False]["last_order"] in (6, 10) and stats[False]["reserved"][3] == 0  # the split-operator rows ran
    assert diff < 2e-9  # (tests/test_gpu_ket.py: the bound of this comparison on this problem)
    assert abs(np.trace(outs[False]).real - 1.0) < 1e-10


def test_quantum_jump_solve_keeps_its_jumps_and_norms():
    strong = [(np.sqrt(6.0), "sigma_gr"), (np.sqrt(2 * 1.5), "sigma_rr")] + [(np.sqrt(2.0 / 4), p) for p in "xyz"]
    prob = _ramp_problem(14, seed=7, collapse_ops=strong, paulis=DEPOL_PAULIS)
    batch = 8
    seeds = np.arange(batch, dtype=np.uint64) * np.uint64(7919) + np.uint64(11)
    times = np.array([0.0, 0.03, 0.08])
    out = {}
    for method in ("auto", "taylor"):
        with Engine(lower([prob] * batch), mode="mcsolve") as eng:
            state = eng.new_state()
            snaps = eng.mc_solve(state, times, seeds, method=method, tol=0.0 if method == "auto" else 1e-12).cpu().numpy()
            out[method] = (snaps, eng.mc_jumps(), eng.stats())
    diff = float(np.max(np.abs(out["auto"][0] - out["taylor"][0])))
    print(f"jumps {out['auto'][1]} / {out['taylor'][1]}; max |split - taylor| = {diff:.3e}; stages {out['auto'][2]['n_applications']} / "
          f"{out['taylor'][2]['n_applications']}")
    assert out["auto"][2]["n_applications"] < out["taylor"][2]["n_applications"]  # the split-operator stages ran
    assert np.array_equal(out["auto"][1], out["taylor"][1]) and out["auto"][1].sum() >= batch // 2
    assert diff < 1e-7
    assert np.allclose(np.linalg.norm(out["auto"][0], axis=-1), 1.0, atol=1e-12)

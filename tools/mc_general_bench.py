#!/usr/bin/env python
"""Quantum-jump trajectories on the general path against the master equation of the same problem.

    python tools/mc_general_bench.py [--ntraj 1024] [--t-end US] [--json]

Legs (the problems of tools/general_bench.py, with noise):
  xy12   XY, 12 atoms (kets of 4 096 amplitudes; the Liouvillian has 4^12 = 16.8 M entries), dephasing;
  all9   3-level "all" basis, 9 atoms (kets of 19 683; the Liouvillian would need 3^18 = 387 M entries, beyond the
         2^26 of a general handle: its mesolve leg reports the refusal).
Per leg: wall time of `ntraj` trajectories in one batched ryd_general_mc_solve (warm), jumps per trajectory, and the
wall time of one ryd_solve of the Liouvillian over the same sequence."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import three_level_problem, xy_problem  # noqa: E402


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    tic = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - tic, out


def run_leg(label, prob, init, t_end, ntraj):
    from pulser_amd._lib import RydError
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general

    d, n = len(prob["eigenbasis"]), prob["n_qudits"]
    rec = {"leg": label, "n_atoms": n, "local_dim": d, "t_end_us": t_end, "ntraj": ntraj}
    tables, cops = lower_general(prob, mesolve=False, matrix_free=True, with_collapse=True)
    seeds = np.random.default_rng(0).integers(0, 2**64, size=ntraj, dtype=np.uint64)
    with GeneralEngine(tables, batch=ntraj) as eng:
        eng.set_collapse(cops)
        eng.mc_solve(eng.new_state(init), [0.0, min(0.002, t_end)], seeds)  # warm-up: code objects, work buffers
        best = np.inf
        for _ in range(2):
            st = eng.new_state(init)
            dt, _ = _timed(lambda: eng.mc_solve(st, [0.0, t_end], seeds))
            best = min(best, dt)
        rec["jumps_per_traj"] = float(eng.mc_jumps().mean())
        rec["norm_err"] = float(abs(np.linalg.norm(st.cpu().numpy(), axis=1) - 1).max())
    rec["mc_s"] = best
    try:
        me = lower_general(prob, mesolve=True, matrix_free=True)
    except NotImplementedError as exc:
        rec["mesolve"] = f"refused: {exc}"
        return rec
    try:
        with GeneralEngine(me) as eng:
            eng.solve(eng.new_state(init), [0.0, min(0.002, t_end)])
            st = eng.new_state(init)
            dt, _ = _timed(lambda: eng.solve(st, [0.0, t_end]))
        rec["mesolve_s"] = dt
        rec["mc_over_mesolve"] = best / dt
    except RydError as exc:
        rec["mesolve"] = f"refused: {exc}"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntraj", type=int, default=1024)
    ap.add_argument("--t-end", type=float, default=0.0, help="us of each sequence to run (0: all of it)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    xy, xy_init, xy_t = xy_problem(12)
    xy = dict(xy, collapse_ops=[(np.sqrt(2 * 0.5), "sigma_dd")])
    al, al_init, al_t = three_level_problem(9)
    al = dict(al, collapse_ops=[(np.sqrt(1.0), "sigma_gr"), (np.sqrt(2 * 0.5), "sigma_rr")],
              depolarizing_pauli_2ds={})
    cut = (lambda t: min(t, a.t_end)) if a.t_end > 0 else (lambda t: t)
    out = [run_leg("xy12", xy, xy_init, cut(xy_t), a.ntraj), run_leg("all9", al, al_init, cut(al_t), a.ntraj)]
    for r in out:
        print(json.dumps(r) if a.json else r)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What the V2 backend's observable loop costs on general-path runs (multi-level bases, XY): wall-clock split of
``QutipBackendV2.last_timing`` (``solve_s``, ``observables_s``) and the launches of the noiseless-H engine
(``last_observable_engine_stats``) for three workloads, all five device-served observables (Occupation,
CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance):

  a  3-level "all" register of 6 atoms under mesolve (rho 729 x 729), 20 evaluation times
  b  XY register of 12 atoms, 64 noise trajectories as quantum jumps (general_jumps=True), 10 evaluation times
  c  3-level register of 9 atoms (19 683 amplitudes), noiseless, 50 evaluation times
  d  workload a with Occupation alone (no energy observable: the device route then applies no generator)

    python tools/general_observe_bench.py [--workloads a b c d] [--reps 5] [--out file.json]

Every workload runs in a child process of its own under a time limit; nothing is started after one that failed.  Per
workload: one warm-up run, then the median of `reps` runs and their spread (max - min).  Uses only the public backend, so
the same file measures a build without the device route (the host formulas)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"a": 420, "b": 300, "c": 300, "d": 300}  # seconds per child


def _level3_inputs(n, dur):
    import numpy as np
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    lay = P.square_rect(3, 3) if n == 9 else P.square_rect(2, n // 2)
    coords = P.register_coords(lay, 6.5)
    t = np.arange(dur)
    everyone = [Slot(0, dur, tuple(range(n)))]
    ryd = ChannelInput("ryd", "Global", "ground-rydberg", 6.0 + 2.0 * np.sin(0.04 * t), -3.0 + 0.05 * t, np.full(dur, 0.4), everyone)
    ram = ChannelInput("raman", "Global", "digital", 4.0 * np.sin(np.pi * t / dur) ** 2, np.full(dur, 1.5), np.full(dur, 0.7), everyone)
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), [ryd, ram], P.C6_LEVEL70)


def _xy_inputs(n, dur):
    import numpy as np
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    coords = P.register_coords(P.square_rect(2, n // 2), 8.0)
    t = np.arange(dur)
    ch = ChannelInput("mw", "Global", "XY", 8.0 * np.sin(np.pi * t / dur) ** 2, -2.0 + 3.0 * t / dur, np.full(dur, 0.4),
                      [Slot(0, dur, tuple(range(n)))])
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), [ch], P.C6_LEVEL70, interaction_coeff_xy=3700.0,
                          magnetic_field=(0.0, 0.0, 30.0))


def _observables(one):
    from pulser_amd.backend import CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance, Occupation

    return [Occupation(one_state=one), CorrelationMatrix(one_state=one), Energy(), EnergySecondMoment(), EnergyVariance()]


def _backend(which):
    import numpy as np
    from pulser_amd import NoiseModel, Solver
    from pulser_amd.backend import QutipBackendV2, QutipConfig

    if which in ("a", "d"):
        cfg = QutipConfig(default_evaluation_times=list(np.linspace(0.0, 1.0, 20)),
                          observables=_observables("r")[:1 if which == "d" else None],
                          noise_model=NoiseModel(dephasing_rate=0.5, hyperfine_dephasing_rate=0.2), solver=Solver.MESOLVER)
        return QutipBackendV2(_level3_inputs(6, 60), config=cfg), 20
    if which == "b":
        cfg = QutipConfig(default_evaluation_times=list(np.linspace(0.1, 1.0, 10)), observables=_observables("d"),
                          noise_model=NoiseModel(dephasing_rate=3.0, state_prep_error=0.05), n_trajectories=64)
        backend = QutipBackendV2(_xy_inputs(12, 120), config=cfg)
        # general_jumps is a run option of QutipEmulator.run; QutipConfig has no field for it (its keyword set is the
        # reference's), so it goes into the options the backend hands to its emulator
        backend._options["general_jumps"] = True
        return backend, 10
    cfg = QutipConfig(default_evaluation_times=list(np.linspace(0.0, 1.0, 50)), observables=_observables("r"))
    return QutipBackendV2(_level3_inputs(9, 100), config=cfg), 50


def child(which, reps):
    import numpy as np
    import torch
    from pulser_amd.backend import QutipBackendV2

    rows = []
    for rep in range(reps + 1):  # run 0 warms up (library load, first allocations, lowering caches)
        np.random.seed(11)
        backend, n_times = _backend(which)
        tic = time.perf_counter()
        res = backend.run()
        torch.cuda.synchronize()
        wall = time.perf_counter() - tic
        stats = QutipBackendV2.last_observable_engine_stats or {}
        row = dict(QutipBackendV2.last_timing or {}, wall_s=wall, n_applications=stats.get("n_applications"),
                   n_launches=stats.get("n_launches"), n_times=n_times, occupation_last=float(np.sum(res.occupation[-1])))
        print(f"workload {which} run {rep}{' (warm-up)' if rep == 0 else ''}: {json.dumps(row)}", flush=True)
        if rep:
            rows.append(row)
    out = {"workload": which, "reps": reps, "n_times": rows[0]["n_times"], "n_applications": rows[0]["n_applications"],
           "n_launches": rows[0]["n_launches"], "occupation_last": rows[0]["occupation_last"]}
    for key in ("solve_s", "observables_s", "wall_s"):
        v = np.array([r[key] for r in rows])
        out[key] = {"median": float(np.median(v)), "spread": float(v.max() - v.min()), "runs": [float(x) for x in v]}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["a", "b", "c", "d"], choices=["a", "b", "c", "d"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results (a JSON list) here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if args.child:
        child(args.child, args.reps)
        return 0
    results = []
    for w in args.workloads:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", w, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=LIMITS[w], cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"workload {w}: no result within {LIMITS[w]} s; stopping", flush=True)
            return 124
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stdout.write(p.stderr[-4000:])
            print(f"workload {w}: exit status {p.returncode}; stopping", flush=True)
            return p.returncode if p.returncode > 0 else 1
        results += [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")]
    for r in results:
        print(f"{r['workload']}: observables {r['observables_s']['median'] * 1e3:9.2f} ms (spread "
              f"{r['observables_s']['spread'] * 1e3:.2f}), solve {r['solve_s']['median'] * 1e3:9.2f} ms (spread "
              f"{r['solve_s']['spread'] * 1e3:.2f}), {r['n_applications']} applications / {r['n_launches']} launches of the "
              f"noiseless-H engine over {r['n_times']} evaluation times")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

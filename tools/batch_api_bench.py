"""run_batch against the serial run() loop.

Three workloads: 256 distinct 14-atom anneals (amplitude and detuning spread +-1 % as in bench.py's spread_tables,
evaluation_times="Minimal"); a 64-point duration scan, 500 - 3 100 ns, on 12 atoms; one "Full" group of 32 x 12 atoms.
For each: the wall time of run_batch, its GPU solve and host lowering parts (solve_many's own clocks, the solve waits
for the device), and the serial loop of run() over 8 of the emulators, extrapolated to all of them.  One JSON line each.

    python tools/batch_api_bench.py [--serial 8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _emulators(n, durations, amp_f, det_f, evaluation_times):
    from pulser_amd import QutipEmulator
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import single_global_channel

    lay = P.triangular_rect(2, 7) if n == 14 else P.square_rect(2, n // 2)
    coords = P.register_coords(lay, 7.0)
    out = []
    for d, fa, fd in zip(durations, amp_f, det_f):
        s = P.anneal_samples()
        if d != len(s["amp"]) - 1:  # a duration scan: the anneal's shape stretched to d ns
            x = np.linspace(0.0, 1.0, d + 1)
            xs = np.linspace(0.0, 1.0, len(s["amp"]))
            s = {k: np.interp(x, xs, v) for k, v in s.items()}
        s = {"amp": fa * s["amp"][:-1], "det": fd * s["det"][:-1], "phase": s["phase"][:-1]}
        inputs = single_global_channel(coords, s, P.C6_LEVEL70, extended=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            out.append(QutipEmulator(inputs, evaluation_times=evaluation_times))
    return out


def _measure(name, emus, n_serial):
    import torch

    import pulser_amd.batch as B

    clocks = {}
    orig = B.solve_many

    def timed(*a, **k):
        r = orig(*a, **k)
        clocks["lower_s"] = clocks.get("lower_s", 0.0) + r.lower_s
        clocks["solve_s"] = clocks.get("solve_s", 0.0) + r.solve_s
        clocks["n_solves"] = clocks.get("n_solves", 0) + len(r.chunks)
        return r

    B.solve_many = timed
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            B.run_batch(emus[:2])  # warm-up: library, kernels, allocator
            clocks.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = B.run_batch(emus)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            final = res[0].states[-1].full()  # (forces one read back)
            t0 = time.perf_counter()
            for e in emus[:n_serial]:
                e.run()
            torch.cuda.synchronize()
            serial = (time.perf_counter() - t0) / n_serial * len(emus)
    finally:
        B.solve_many = orig
    line = {"workload": name, "n_sequences": len(emus), "run_batch_ms": 1e3 * wall,
            "gpu_solve_ms": 1e3 * clocks["solve_s"], "host_lowering_ms": 1e3 * clocks["lower_s"],
            "n_solves": clocks["n_solves"], "serial_run_ms_extrapolated": 1e3 * serial,
            "serial_measured_on": n_serial, "speedup": serial / wall, "final_norm_0": float(np.linalg.norm(final))}
    print(json.dumps(line), flush=True)
    return line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--serial", type=int, default=8)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    if a.only in ("", "anneal"):
        amp = 1.0 + 0.01 * (2.0 * rng.random(256) - 1.0)
        det = 1.0 + 0.01 * (2.0 * rng.random(256) - 1.0)
        amp[0] = det[0] = 1.0
        _measure("anneal14_x256_minimal", _emulators(14, [3100] * 256, amp, det, "Minimal"), a.serial)
    if a.only in ("", "scan"):
        durs = np.linspace(500, 3100, 64).astype(int).tolist()
        _measure("duration_scan12_x64_minimal", _emulators(12, durs, [1.0] * 64, [1.0] * 64, "Minimal"), a.serial)
    if a.only in ("", "full"):
        amp = 1.0 + 0.01 * (2.0 * rng.random(32) - 1.0)
        _measure("anneal12_x32_full", _emulators(12, [3100] * 32, amp, [1.0] * 32, "Full"), a.serial)


if __name__ == "__main__":
    main()

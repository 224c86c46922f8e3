"""Observable phase of a two-level master-equation run of the V2 backend (``QutipBackendV2.last_timing["observables_s"]``)
with ``NoiseModel(dephasing_rate=0.05)`` and Occupation, CorrelationMatrix, Energy, EnergyVariance and
EnergySecondMoment configured: the per-time path (per evaluation time one download, host normalisation, upload,
``ryd_observe`` and read-back) against the one-call path (``ryd_observe_density_many`` over the device snapshots), for
8 and 10 atoms and a list of evaluation-time counts of the 3.1-us anneal.  Each cell is the median of ``--repeats``
runs after one warm-up run of each path, the two paths alternating.  Prints a markdown table (the source of
profiles/observe_density_many.md) and the smallest of the counts from which the one-call path is faster at every size.

On a commit without the route both columns are the per-time path: that run is the baseline the table is compared with.
A count whose snapshots ([count, 1, D, D] complex128) do not fit ``--max-gib`` of device memory is skipped.

    python tools/observe_density_many_bench.py [--atoms 8 10] [--times 128 512 3101] [--repeats 3] [--max-gib 64]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, nargs="+", default=[8, 10])
    ap.add_argument("--times", type=int, nargs="+", default=[128, 512, 3101])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-gib", type=float, default=64.0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("observe_density_many_bench needs the GPU: nothing is timed without one")

    from helpers import blockade_radius
    from pulser_amd import NoiseModel
    from pulser_amd import problem as P
    from pulser_amd.backend import (CorrelationMatrix, Energy, EnergySecondMoment, EnergyVariance, Occupation,
                                    QutipBackendV2, QutipConfig)
    from pulser_amd.hamiltonian_data import single_global_channel

    has_route = hasattr(QutipBackendV2, "_DENSITY_OBSERVE_MANY_FLOOR")
    print(f"# one-call route for density matrices: {'present' if has_route else 'ABSENT (both columns are the per-time path)'}")

    def run(inputs, cfg, min_times):
        QutipBackendV2.observe_many_min_times = min_times
        QutipBackendV2(inputs, config=cfg).run()
        torch.cuda.synchronize()
        t = QutipBackendV2.last_timing
        return t["observables_s"], t["solve_s"], QutipBackendV2.last_observable_engine_stats["n_launches"]

    rows = []
    for n in args.atoms:
        coords = P.register_coords(P.square_rect(1, n), blockade_radius())
        smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
        inputs = single_global_channel(coords, smp, P.C6_LEVEL70, extended=False)
        for count in args.times:
            gib = count * 16.0 * 4.0**n / 2**30
            if gib > args.max_gib:
                print(f"# {n} atoms, {count} times: {gib:.1f} GiB of snapshots exceed --max-gib {args.max_gib}: skipped", flush=True)
                continue
            times = "Full" if count == 3101 else np.linspace(1.0 / count, 1.0, count).tolist()
            cfg = QutipConfig(default_evaluation_times=times, noise_model=NoiseModel(dephasing_rate=0.05), observables=[
                Occupation(), CorrelationMatrix(), Energy(), EnergyVariance(), EnergySecondMoment()])
            run(inputs, cfg, None), run(inputs, cfg, 1)  # warm-up of both paths
            per, one, solve, launches = [], [], [], (0, 0)
            for _ in range(args.repeats):
                a, s1, la = run(inputs, cfg, None)
                b, s2, lb = run(inputs, cfg, 1)
                per.append(a), one.append(b), solve.extend([s1, s2])
                launches = (la, lb)
            rows.append((n, count, statistics.median(per), statistics.median(one), statistics.median(solve), launches,
                         (min(per), max(per)), (min(one), max(one))))
            print(f"# {n} atoms, {count} times: per-time {rows[-1][2]:.4f} s, one call {rows[-1][3]:.4f} s", flush=True)
    print("| atoms | evaluation times | per-time path (s) [min, max] | one call (s) [min, max] | ratio | solve (s) | launches per-time / one call |")
    print("|---|---|---|---|---|---|---|")
    for n, count, a, b, s, (la, lb), (a0, a1), (b0, b1) in rows:
        print(f"| {n} | {count} | {a:.4f} [{a0:.4f}, {a1:.4f}] | {b:.4f} [{b0:.4f}, {b1:.4f}] | {a / b:.1f} | {s:.4f} | {la} / {lb} |")
    counts = sorted({r[1] for r in rows})
    faster = [c for c in counts if all(r[3] < r[2] for r in rows if r[1] >= c)]
    print(f"one call faster at every size from {faster[0] if faster else 'no count'} evaluation times on")


if __name__ == "__main__":
    main()

"""Observable phase of a V2-backend run (``QutipBackendV2.last_timing["observables_s"]``) of multi-level and XY
sequences on the per-time path (``ryd_general_observe`` per evaluation time) and on the one-call path
(``ryd_general_observe_many`` over the device snapshots): a 12-atom XY sequence, a 9-atom and a 10-atom 3-level ("all"
basis) sequence at 128, 256, 1 024 and all ("Full") evaluation times, with Occupation, CorrelationMatrix and Energy
configured.  Each cell is the median of ``--repeats`` runs after one warm-up run, the two paths alternating, with the
spread (min .. max).  Prints a markdown table (the source of profiles/general_observe_many.md) and the smallest of those
counts from which the one-call path is faster on every workload.

    python tools/general_observe_many_bench.py [--workloads xy12 l3_9 l3_10] [--times 128 256 1024 0] [--repeats 5]
                                               [--duration 2000] [--paths per-time one-call]

``--times 0`` is "Full" (one time per ns: ``--duration`` + 1 of them).  ``--paths per-time`` alone also runs on a tree
that has no one-call path for these registers (the threshold attribute is then without effect)."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def xy_inputs(rows: int, cols: int, dur: int):
    """An XY register with a global microwave drive of non-zero phase (a complex H)."""
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    n = rows * cols
    coords = P.register_coords(P.square_rect(rows, cols), 8.0)
    t = np.arange(dur)
    ch = ChannelInput("mw", "Global", "XY", 8.0 * np.sin(np.pi * t / dur) ** 2, -2.0 + 3.0 * t / dur, np.full(dur, 0.4),
                      [Slot(0, dur, tuple(range(n)))])
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), [ch], 5420158.53,
                          interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))


def three_level_inputs(rows: int, cols: int, dur: int):
    """The "all" basis (r, g, h): a global ground-rydberg drive and local raman drives with complex phases on three atoms."""
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    n = rows * cols
    coords = P.register_coords(P.square_rect(rows, cols), 6.5)
    t = np.arange(dur) / 1000.0
    rng = np.random.default_rng(5)
    chans = [ChannelInput("ryd", "Global", "ground-rydberg", 6.0 + 2.0 * np.sin(40 * t), -3.0 + 5.0 * t, np.full(dur, 0.4),
                          [Slot(0, dur, tuple(range(n)))])]
    for q in (0, n // 2, n - 2):
        chans.append(ChannelInput(f"raman{q}", "Local", "digital", np.full(dur, rng.uniform(2, 8)),
                                  np.full(dur, rng.uniform(-3, 3)), np.full(dur, rng.uniform(0, 1)), [Slot(0, dur, (q,))]))
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), chans, P.C6_LEVEL70)


WORKLOADS = {"xy12": (lambda dur: xy_inputs(2, 6, dur), "d"), "l3_9": (lambda dur: three_level_inputs(3, 3, dur), "r"),
             "l3_10": (lambda dur: three_level_inputs(2, 5, dur), "r")}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--times", type=int, nargs="+", default=[128, 256, 1024, 0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--duration", type=int, default=2000)
    ap.add_argument("--paths", nargs="+", default=["per-time", "one-call"], choices=["per-time", "one-call"])
    args = ap.parse_args()

    from pulser_amd.backend import CorrelationMatrix, Energy, Occupation, QutipBackendV2, QutipConfig

    threshold = {"per-time": None, "one-call": 128}

    def run(inputs, cfg, path):
        backend = QutipBackendV2(inputs, config=cfg)
        backend.observe_many_min_times = threshold[path]
        backend.run()
        t = QutipBackendV2.last_timing
        n_eval.append(len(backend._sim_obj._eval_times_array))
        return t["observables_s"], t["solve_s"], QutipBackendV2.last_observable_engine_stats["n_launches"]

    rows = []
    n_eval: list[int] = []  # evaluation times of the last run (the solver's list: the configured ones and t = 0)
    for name in args.workloads:
        make, one = WORKLOADS[name]
        inputs = make(args.duration)
        for count in args.times:
            times = "Full" if count == 0 else np.linspace(1.0 / count, 1.0, count).tolist()
            cfg = QutipConfig(default_evaluation_times=times, observables=[
                Occupation(one_state=one), CorrelationMatrix(one_state=one), Energy()])
            for path in args.paths:
                run(inputs, cfg, path)  # warm-up
            obs = {p: [] for p in args.paths}
            solve, launches = [], {}
            for _ in range(args.repeats):
                for path in args.paths:
                    o, s, launches[path] = run(inputs, cfg, path)
                    obs[path].append(o)
                    solve.append(s)
            n_times = n_eval[-1]
            rows.append((name, n_times, obs, statistics.median(solve), dict(launches)))
            print(f"# {name}, {n_times} times: " + ", ".join(
                f"{p} {statistics.median(v):.4f} s ({min(v):.4f} .. {max(v):.4f})" for p, v in obs.items()), flush=True)
    cell = lambda v: f"{statistics.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"  # noqa: E731
    print("| workload | evaluation times | " + " | ".join(f"{p} path: observables_s, median (min .. max)" for p in args.paths)
          + " | ratio | solve (s) | launches " + " / ".join(args.paths) + " |")
    print("|---|---|" + "---|" * (len(args.paths) + 3))
    for name, n_times, obs, solve, launches in rows:
        ratio = (f"{statistics.median(obs['per-time']) / statistics.median(obs['one-call']):.1f}"
                 if len(args.paths) == 2 else "-")
        print(f"| {name} | {n_times} | " + " | ".join(cell(obs[p]) for p in args.paths)
              + f" | {ratio} | {solve:.4f} | " + " / ".join(str(launches[p]) for p in args.paths) + " |")
    if len(args.paths) == 2:
        counts = sorted({r[1] for r in rows})
        faster = [c for c in counts if all(statistics.median(o["one-call"]) < statistics.median(o["per-time"])
                                           for _, cc, o, _, _ in rows if cc >= c)]
        print(f"one call faster on every workload from {faster[0] if faster else 'no count'} evaluation times on")


if __name__ == "__main__":
    main()

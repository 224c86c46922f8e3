"""Quantum-jump ensembles of multi-level and XY registers from their kets (``QutipEmulator.run(general_jumps=True,
mc_ensemble=True)``): the numbers of profiles/general_mc_ensemble.md.

 1. The two runs the default general-jump route refuses (those of tests/test_gpu_general_mc_ensemble.py): 14 XY
    atoms at 6 evaluation times and 4 trajectories, 9 three-level atoms at 4 evaluation times and 3 trajectories -
    wall time and ``torch.cuda.max_memory_allocated`` of the ensemble run, after one warm-up run.
 2. A 12-atom XY register (D = 4096) at 32 evaluation times and 256 trajectories on both routes, alternating after one
    warm-up run of each, the same ``seeds=``: wall time and ``torch.cuda.max_memory_allocated`` per route.

    python tools/general_mc_ensemble_bench.py [--skip-capability] [--skip-both]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--times", type=int, default=32)
    ap.add_argument("--trajectories", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-capability", action="store_true")
    ap.add_argument("--skip-both", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("general_mc_ensemble_bench needs the GPU: nothing is timed without one")

    from pulser_amd import NoiseModel, QutipEmulator, Solver
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    def xy_inputs(rows, cols, spacing, dur, amp):
        n = rows * cols
        t = np.arange(dur)
        ch = ChannelInput("mw", "Global", "XY", amp * np.sin(np.pi * t / dur) ** 2, np.full(dur, -2.0), np.zeros(dur),
                          [Slot(0, dur, tuple(range(n)))])
        return SequenceInputs(P.register_coords(P.square_rect(rows, cols), spacing), tuple(f"q{i}" for i in range(n)),
                              [ch], 5420158.53, interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))

    def all_inputs(rows, cols, spacing, dur, amp):
        n = rows * cols
        t = np.arange(dur)
        slot = [Slot(0, dur, tuple(range(n)))]
        chans = [ChannelInput("ryd", "Global", "ground-rydberg", amp * np.sin(np.pi * t / dur) ** 2,
                              np.full(dur, -1.0), np.zeros(dur), list(slot)),
                 ChannelInput("ram", "Global", "digital", 6.0 * np.sin(np.pi * t / dur) ** 2, np.full(dur, 0.5),
                              np.full(dur, 0.3), list(slot))]
        return SequenceInputs(P.register_coords(P.square_rect(rows, cols), spacing), tuple(f"q{i}" for i in range(n)),
                              chans, P.C6_LEVEL70)

    def timed(emu, **options):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        tic = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            res = emu.run(seeds=1, general_jumps=True, **options)
        torch.cuda.synchronize()
        return time.perf_counter() - tic, torch.cuda.max_memory_allocated() / 2**20, res

    if not args.skip_capability:
        cases = [
            ("XY 2 x 7", QutipEmulator(xy_inputs(2, 7, 9.0, 120, 30.0), noise_model=NoiseModel(dephasing_rate=6.0),
                                       solver=Solver.MCSOLVER, n_trajectories=4,
                                       evaluation_times=[0.024, 0.048, 0.072, 0.096]), {}),
            ("all 3 x 3", QutipEmulator(all_inputs(3, 3, 6.5, 100, 40.0),
                                        noise_model=NoiseModel(relaxation_rate=5.0, dephasing_rate=10.0),
                                        solver=Solver.MCSOLVER, n_trajectories=3, evaluation_times=[0.03, 0.07]),
             {"mc_ensemble_digits": [0, 2]}),
        ]
        print("| register | D | evaluation times | trajectories | wall (s) [min, max] | torch tensors peak (MiB) | jumps | "
              "energy served |")
        print("|---|---|---|---|---|---|---|---|")
        for name, emu, options in cases:
            timed(emu, mc_ensemble=True, **options)  # warm-up
            runs = [timed(emu, mc_ensemble=True, **options) for _ in range(args.repeats)]
            secs = [r[0] for r in runs]
            res = runs[-1][2]
            print(f"| {name} | {res.states[-1].shape[0]} | {len(res)} | {emu.n_trajectories} | {statistics.median(secs):.3f} "
                  f"[{min(secs):.3f}, {max(secs):.3f}] | {max(r[1] for r in runs):.1f} | {int(emu.last_mc_jumps.sum())} | "
                  f"{bool(np.isfinite(res.states[-1].energy))} |", flush=True)
            del emu, res, runs
            torch.cuda.empty_cache()

    if not args.skip_both:
        dur = 500
        emu = QutipEmulator(xy_inputs(3, 4, 9.0, dur, 12.0), sampling_rate=0.1, noise_model=NoiseModel(dephasing_rate=3.0),
                            solver=Solver.MCSOLVER, n_trajectories=args.trajectories,
                            evaluation_times=np.linspace(0.0, dur / 1000, args.times))
        timed(emu), timed(emu, mc_ensemble=True)  # warm-up of both routes
        a, b = [], []
        for _ in range(args.repeats):
            a.append(timed(emu)[:2])
            b.append(timed(emu, mc_ensemble=True)[:2])
        print("| register | D | evaluation times | trajectories | general_jumps (s) [min, max] | peak (MiB) | "
              "+ mc_ensemble (s) [min, max] | peak (MiB) |")
        print("|---|---|---|---|---|---|---|---|")
        sa, sb = [r[0] for r in a], [r[0] for r in b]
        print(f"| XY 3 x 4 | 4096 | {len(emu._eval_times_array)} | {args.trajectories} | {statistics.median(sa):.3f} "
              f"[{min(sa):.3f}, {max(sa):.3f}] | {max(r[1] for r in a):.1f} | {statistics.median(sb):.3f} "
              f"[{min(sb):.3f}, {max(sb):.3f}] | {max(r[1] for r in b):.1f} |", flush=True)


if __name__ == "__main__":
    main()

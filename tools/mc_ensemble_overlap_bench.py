"""Fidelities and expectation values of quantum-jump ensembles from the kets (``QutipEmulator.run(mc_ensemble=True,
mc_ensemble_targets=..., mc_ensemble_operators=...)``): the numbers of profiles/mc_ensemble_overlap.md.

Wall time of an ensemble run without anything registered against the same run with one target (the antiferromagnetic
basis state) and one operator (sum of sigma_x over the atoms) registered, the two alternating after one warm-up run of
each, the same ``seeds=``:

 1. the 14-atom / 100 evaluation times / 256 trajectories run of profiles/mc_ensemble.md (the tuned two-level route,
    four chunks);
 2. 12 atoms / 32 evaluation times / 256 trajectories (one chunk) on both ensemble routes: the chain of
    tools/mc_ensemble_bench.py on the two-level route, the 3 x 4 XY register of tools/general_mc_ensemble_bench.py on
    the general route (``general_jumps=True``).

    python tools/mc_ensemble_overlap_bench.py [--skip-big] [--skip-both]
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
    ap.add_argument("--atoms", type=int, default=12)
    ap.add_argument("--times", type=int, default=32)
    ap.add_argument("--trajectories", type=int, default=256)
    ap.add_argument("--big-atoms", type=int, default=14)
    ap.add_argument("--big-times", type=int, default=100)
    ap.add_argument("--big-trajectories", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--skip-both", action="store_true")
    args = ap.parse_args()

    import scipy.sparse as sp
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mc_ensemble_overlap_bench needs the GPU: nothing is timed without one")

    from helpers import blockade_radius
    from pulser_amd import NoiseModel, QutipEmulator, Solver
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot, single_global_channel

    def chain(n, n_times, ntraj):
        coords = P.register_coords(P.square_rect(1, n), blockade_radius())
        smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
        inputs = single_global_channel(coords, smp, P.C6_LEVEL70, extended=False)
        return QutipEmulator(inputs, noise_model=NoiseModel(dephasing_rate=0.3, relaxation_rate=0.2),
                             solver=Solver.MCSOLVER, n_trajectories=ntraj, evaluation_times=np.linspace(0.0, 3.1, n_times))

    def xy(rows, cols, n_times, ntraj, spacing=9.0, dur=500, amp=12.0):
        n = rows * cols
        t = np.arange(dur)
        ch = ChannelInput("mw", "Global", "XY", amp * np.sin(np.pi * t / dur) ** 2, np.full(dur, -2.0), np.zeros(dur),
                          [Slot(0, dur, tuple(range(n)))])
        inputs = SequenceInputs(P.register_coords(P.square_rect(rows, cols), spacing), tuple(f"q{i}" for i in range(n)),
                                [ch], 5420158.53, interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))
        return QutipEmulator(inputs, sampling_rate=0.1, noise_model=NoiseModel(dephasing_rate=3.0), solver=Solver.MCSOLVER,
                             n_trajectories=ntraj, evaluation_times=np.linspace(0.0, dur / 1000, n_times))

    def registered(n):
        """The antiferromagnetic basis state and the sum of sigma_x over ``n`` two-level atoms."""
        target = np.zeros(2**n, dtype=complex)
        target[int("01" * (n // 2) + "0" * (n % 2), 2)] = 1.0
        sx = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
        op = sp.csr_matrix((2**n, 2**n))
        for q in range(n):
            op = op + sp.kron(sp.kron(sp.identity(2**q), sx), sp.identity(2**(n - q - 1)))
        return dict(mc_ensemble_targets=[target], mc_ensemble_operators=[op.tocsr()])

    def timed(emu, **options):
        torch.cuda.synchronize()
        tic = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            res = emu.run(seeds=1, mc_ensemble=True, **options)
        torch.cuda.synchronize()
        return time.perf_counter() - tic, res

    def row(name, emu, n, **options):
        extra = registered(n)
        timed(emu, **options), timed(emu, **options, **extra)  # warm-up of both
        a, b = [], []
        for _ in range(args.repeats):
            a.append(timed(emu, **options)[0])
            secs, res = timed(emu, **options, **extra)
            b.append(secs)
        st = res.states[-1]
        print(f"| {name} | {st.shape[0]} | {len(res)} | {emu.n_trajectories} | {statistics.median(a):.3f} "
              f"[{min(a):.3f}, {max(a):.3f}] | {statistics.median(b):.3f} [{min(b):.3f}, {max(b):.3f}] | "
              f"{st.fidelity[0]:.3e} +- {st.fidelity_stderr[0]:.1e} | {st.expectation[0].real:.4f} +- "
              f"{st.expectation_stderr[0]:.4f} |", flush=True)
        del res
        torch.cuda.empty_cache()

    print("| run | D | evaluation times | trajectories | nothing registered (s) [min, max] | one target, one operator (s) "
          "[min, max] | final fidelity | final sum sigma_x |")
    print("|---|---|---|---|---|---|---|---|")
    if not args.skip_big:
        n = args.big_atoms
        row(f"chain of {n}, two-level route", chain(n, args.big_times, args.big_trajectories), n)
    if not args.skip_both:
        n = args.atoms
        row(f"chain of {n}, two-level route", chain(n, args.times, args.trajectories), n)
        row("XY 3 x 4, general route", xy(3, 4, args.times, args.trajectories), 12, general_jumps=True)


if __name__ == "__main__":
    main()

"""Quantum-jump ensembles without the density matrix (``QutipEmulator.run(mc_ensemble=True)``): the numbers of
profiles/mc_ensemble.md.

 1. ``ryd_ensemble_diag`` alone over snapshot tensors ``[T, B, D]`` (``--kernel-shapes``): warm-up launches, then timed
    launches between HIP events on the stream; the bytes it has to move (16 per amplitude and trajectory, and the
    diagonal read and written once) against ``--hbm-tbs``.
 2. Wall time of the deterministic-noise jump run of one register (``--atoms``, ``--times`` evaluation times,
    ``--trajectories``) on the default route (``run()``: the averaged density matrices, the code of every earlier
    commit) and with ``mc_ensemble=True``, the two alternating after one warm-up run of each, the same ``seeds=``.
 3. One run only the ensemble route can do (``--big-atoms``, ``--big-times``, ``--big-trajectories``): wall time and
    peak device memory (the drop of ``torch.cuda.mem_get_info`` free memory sampled around the solve by a thread, which
    counts the library's own allocations too, next to torch's peak for its tensors).

    python tools/mc_ensemble_bench.py [--skip-kernel] [--skip-run] [--skip-big]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import threading
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-shapes", type=str, nargs="+", default=["32x256x4096", "100x81x16384"])
    ap.add_argument("--atoms", type=int, default=12)
    ap.add_argument("--times", type=int, default=32)
    ap.add_argument("--trajectories", type=int, default=256)
    ap.add_argument("--big-atoms", type=int, default=14)
    ap.add_argument("--big-times", type=int, default=100)
    ap.add_argument("--big-trajectories", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the kernel is compared with, TB/s")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-run", action="store_true")
    ap.add_argument("--skip-big", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mc_ensemble_bench needs the GPU: nothing is timed without one")

    from helpers import blockade_radius
    from pulser_amd import NoiseModel, QutipEmulator, Solver, _lib
    from pulser_amd import problem as P
    from pulser_amd.hamiltonian_data import single_global_channel

    if not args.skip_kernel:
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        print("| T | B | D | bytes (MB) | call (us) [min, max] | at the HBM rate (us) | fraction |")
        print("|---|---|---|---|---|---|---|")
        for shape in args.kernel_shapes:
            T, B, D = (int(v) for v in shape.split("x"))
            x = torch.randn((T, B, D), dtype=torch.complex128, device="cuda:0")
            diag = torch.zeros((T, D), dtype=torch.float64, device="cuda:0")

            def call():
                _lib.check(lib.ryd_ensemble_diag(x.data_ptr(), T, B, B * D, D, D, diag.data_ptr(), 0, stream))

            for _ in range(3):
                call()
            torch.cuda.synchronize()
            us = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1))
            nbytes = 16.0 * T * B * D + 16.0 * T * D
            roof = nbytes / (args.hbm_tbs * 1e12) * 1e6
            med = statistics.median(us)
            print(f"| {T} | {B} | {D} | {nbytes / 1e6:.1f} | {med:.1f} [{min(us):.1f}, {max(us):.1f}] | {roof:.1f} | "
                  f"{roof / med:.2f} |", flush=True)
            del x, diag

    def emulator(n, n_times, ntraj):
        coords = P.register_coords(P.square_rect(1, n), blockade_radius())
        smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
        inputs = single_global_channel(coords, smp, P.C6_LEVEL70, extended=False)
        return QutipEmulator(inputs, noise_model=NoiseModel(dephasing_rate=0.3, relaxation_rate=0.2),
                             solver=Solver.MCSOLVER, n_trajectories=ntraj,
                             evaluation_times=np.linspace(0.0, 3.1, n_times))

    def timed(emu, **options):
        torch.cuda.synchronize()
        tic = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            res = emu.run(seeds=1, **options)
        torch.cuda.synchronize()
        return time.perf_counter() - tic, res

    if not args.skip_run:
        emu = emulator(args.atoms, args.times, args.trajectories)
        timed(emu), timed(emu, mc_ensemble=True)  # warm-up of both routes
        a, b = [], []
        for _ in range(args.repeats):
            a.append(timed(emu)[0])
            b.append(timed(emu, mc_ensemble=True)[0])
        print("| atoms | evaluation times | trajectories | run() (s) [min, max] | run(mc_ensemble=True) (s) [min, max] |")
        print("|---|---|---|---|---|")
        print(f"| {args.atoms} | {len(emu._eval_times_array)} | {args.trajectories} | {statistics.median(a):.3f} "
              f"[{min(a):.3f}, {max(a):.3f}] | {statistics.median(b):.3f} [{min(b):.3f}, {max(b):.3f}] |", flush=True)
        del emu
        torch.cuda.empty_cache()

    if not args.skip_big:
        emu = emulator(args.big_atoms, args.big_times, args.big_trajectories)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        free0 = torch.cuda.mem_get_info()[0]
        low = [free0]
        stop = threading.Event()

        def sample():
            while not stop.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info()[0])
                time.sleep(0.005)

        th = threading.Thread(target=sample, daemon=True)
        th.start()
        secs, res = timed(emu, mc_ensemble=True)
        stop.set()
        th.join()
        st = res.states[-1]
        print("| atoms | evaluation times | trajectories | wall (s) | peak device memory (GiB, free-memory drop) | "
              "torch tensors peak (GiB) | jumps | trace | max occupation stderr |")
        print("|---|---|---|---|---|---|---|---|---|")
        print(f"| {args.big_atoms} | {len(res)} | {args.big_trajectories} | {secs:.2f} | {(free0 - low[0]) / 2**30:.2f} | "
              f"{torch.cuda.max_memory_allocated() / 2**30:.2f} | {int(emu.last_mc_jumps.sum())} | {st.tr().real:.15f} | "
              f"{float(st.occupation_stderr.max()):.4f} |", flush=True)


if __name__ == "__main__":
    main()

"""Reduced density matrices from the device snapshots (``ryd_reduced_density``, ``results.entanglement_entropy``): the
numbers of profiles/reduced_density.md.

 (a) ``ryd_reduced_density`` alone over snapshot tensors ``[T, 1, 2^14]`` (``--times``) for kept sets of 1, 2, 4 and 6
     qubits at the top, at the bottom and interleaved, and over one 20-atom ket with the library's split against
     ``n_split = 1``: warm-up launches, then timed launches between HIP events on the stream (median, min, max); the
     bytes it has to read (16 per amplitude) against ``--hbm-tbs`` (the figure bench.py uses) and, for 6 qubits, the
     flops of the MFMAs it issues against ``--f64-tflops`` (the peak quoted in k_small.hpp).
 (b) ``entanglement_entropy`` of the half chain of a ``--atoms``-atom ``evaluation_times="Full"`` run through the
     device route (the states stay snapshots) against the host route on results of the same run: every state fetched
     with ``np.asarray``, then ``QState.ptrace`` and ``entropy_vn`` per time.  Every repeat solves anew, so that the
     host route pays its copies every time; the solve itself is outside the timed region.

    python tools/reduced_density_bench.py [--skip-kernel] [--skip-run]
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
    ap.add_argument("--times", type=int, default=3101)
    ap.add_argument("--atoms", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate the call is compared with, TB/s (bench.py: HBM_PEAK)")
    ap.add_argument("--f64-tflops", type=float, default=78.6, help="f64 matrix peak the 6-qubit call is compared with")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-run", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("reduced_density_bench needs the GPU: nothing is timed without one")

    from pulser_amd import QState, QutipEmulator, entropy_vn
    from pulser_amd.engine import reduced_density

    def time_call(x, keep, n_split):
        d_a = 2 ** len(keep)
        out = torch.zeros((x.shape[0], d_a, d_a), dtype=torch.complex128, device=x.device)
        for _ in range(3):
            reduced_density(x, keep, out=out, n_split=n_split)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            reduced_density(x, keep, out=out, n_split=n_split)
            e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        return us

    def row(label, x, keep, n_split):
        us = time_call(x, keep, n_split)
        t, _, dim = (int(v) for v in x.shape)
        d_a = 2 ** len(keep)
        nbytes = 16.0 * t * dim
        med = statistics.median(us)
        nt = (d_a + 15) // 16
        # per pair of columns: nt (nt + 1) / 2 blocks, a real and an imaginary MFMA of 16 x 16 x 4 x 2 flops each
        flops = t * (dim // d_a + 1) // 2 * nt * (nt + 1) * 2048.0
        frac_f = f"{flops / (med * 1e-6) / 1e12:.1f} ({flops / (med * 1e-6) / 1e12 / args.f64_tflops:.2f})" if d_a == 64 else "-"
        print(f"| {label} | {list(keep)} | {d_a} | {n_split} | {nbytes / 1e6:.1f} | {med:.1f} [{min(us):.1f}, {max(us):.1f}] | "
              f"{nbytes / (med * 1e-6) / 1e12:.2f} ({nbytes / (med * 1e-6) / 1e12 / args.hbm_tbs:.2f}) | {frac_f} |", flush=True)

    if not args.skip_kernel:
        n = 14
        x = torch.randn((args.times, 1, 2**n), dtype=torch.complex128, device="cuda:0")
        print(f"(the call includes the wrapper: argument checks and, with a split, the scratch allocation; "
              f"{args.launches} timed launches after 3 warm-up ones)")
        print("| states | keep | dA | n_split (0: library) | bytes read (MB) | call (us) [min, max] | TB/s (of the HBM figure) | "
              "MFMA TFLOP/s (of the f64 peak) |")
        print("|---|---|---|---|---|---|---|---|")
        label = f"{args.times} x 2^{n}"
        for keep in ([0], [13], [7], [0, 1], [12, 13], [3, 10], [0, 1, 2, 3], [10, 11, 12, 13], [1, 5, 9, 13],
                     [0, 1, 2, 3, 4, 5], [8, 9, 10, 11, 12, 13], [0, 3, 5, 8, 10, 13]):
            row(label, x, keep, 0)
        del x
        torch.cuda.empty_cache()
        x = torch.randn((1, 1, 2**20), dtype=torch.complex128, device="cuda:0")
        for keep in ([0], [0, 19], [4, 9, 14, 19], [0, 1, 2, 17, 18, 19]):
            for n_split in (0, 1):
                row("1 x 2^20", x, keep, n_split)
        del x
        torch.cuda.empty_cache()

    if not args.skip_run:
        from helpers import blockade_radius
        from pulser_amd import problem as P
        from pulser_amd.hamiltonian_data import single_global_channel

        n = args.atoms
        coords = P.register_coords(P.square_rect(1, n), blockade_radius())
        smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
        emu = QutipEmulator(single_global_channel(coords, smp, P.C6_LEVEL70, extended=False))  # evaluation_times="Full"
        keep = list(range(n // 2))

        def solve():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                res = emu.run()
            torch.cuda.synchronize()
            return res

        def device_route(res):
            return res.entanglement_entropy(keep)

        def host_route(res):
            return np.array([entropy_vn(QState(np.asarray(st)).ptrace(keep)) for st in res.states])

        device_route(solve()), host_route(solve())  # warm-up of both routes
        dev, host, diff = [], [], 0.0
        for _ in range(args.repeats):
            res = solve()
            tic = time.perf_counter()
            a = device_route(res)
            dev.append(time.perf_counter() - tic)
            res = solve()
            tic = time.perf_counter()
            b = host_route(res)
            host.append(time.perf_counter() - tic)
            diff = max(diff, float(np.max(np.abs(a - b))))
        print("| atoms | evaluation times | kept | device route (ms) [min, max] | host route (ms) [min, max] | max difference (bits) | "
              "largest entropy (bits) |")
        print("|---|---|---|---|---|---|---|")
        print(f"| {n} | {len(a)} | {keep} | {1e3 * statistics.median(dev):.1f} [{1e3 * min(dev):.1f}, {1e3 * max(dev):.1f}] | "
              f"{1e3 * statistics.median(host):.1f} [{1e3 * min(host):.1f}, {1e3 * max(host):.1f}] | {diff:.1e} | "
              f"{float(np.max(a)):.4f} |", flush=True)


if __name__ == "__main__":
    main()

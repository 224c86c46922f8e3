"""Reduced density matrices of master-equation runs from the device (``ryd_reduced_density_dm``,
``results.reduced_states`` / ``entanglement_entropy`` over density-matrix snapshots): the numbers of
profiles/reduced_density_dm.md.

 (a) ``engine.reduced_density_dm`` alone over random matrices ``[T, 1, 2^N, 2^N]`` - N = 10 with T = 128, N = 13 and
     N = 14 with T = 1 (a size is skipped, and named, when less than twice its bytes are free) - for dA = 2, 16 and 64
     with the kept sites lowest, highest and spread: warm-up calls, then ``--launches`` timed calls between HIP events on
     the stream (median, min, max).  Beside each time: the cache lines the call touches at most (dA D per matrix, fewer
     where the kept sites are the lowest ones and the dA columns of a row share lines of 128 bytes) and the bytes it
     uses (16 dA D).  Against it the route of the commit before this one on the SAME tensor: ``.cpu().numpy()`` of every
     matrix (timed once per size: it does not depend on ``keep``) followed by ``_ptrace_host`` (timed per ``keep``).
 (b) wall time of ``reduced_states`` and ``entanglement_entropy`` on a ``--run-atoms``-atom dephasing run at
     ``--run-times`` evaluation times through the device route (the states stay snapshots; repeated) and then through
     the host route on the same results (every state read with ``np.asarray``, then ``_ptrace_host`` - what
     ``reduced_states`` did before; once, since it ends the store's life on the device).

    python tools/reduced_density_dm_bench.py [--skip-kernel] [--skip-run] [--sizes 10:128,13:1,14:1]
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


def keeps_of(n: int, k: int) -> dict[str, list[int]]:
    spread = sorted({round(j * (n - 1) / max(k - 1, 1)) for j in range(k)}) if k > 1 else [n // 2]
    return {"lowest": list(range(n - k, n)), "highest": list(range(k)), "spread": spread}


def lines_touched(n: int, keep: list[int], n_mats: int) -> int:
    """An estimate from the geometry, not a counter.  A line of 128 bytes holds 8 complex128.  Each of the D rows
    idx(a, r) of a matrix is read at dA columns; when the l lowest sites are all kept these come in aligned runs of 2^l
    adjacent columns, dA / min(2^l, 8) lines per row, else dA lines."""
    d_a = 2 ** len(keep)
    low = 0
    while low < len(keep) and (n - 1 - low) in keep:
        low += 1
    per_line = min(2**low, 8)
    return n_mats * (2**n) * d_a // per_line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10:128,13:1,14:1", help="N:T pairs")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--run-atoms", type=int, default=10)
    ap.add_argument("--run-times", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-host", action="store_true", help="do not time the host route of part (a)")
    ap.add_argument("--skip-run", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("reduced_density_dm_bench needs the GPU: nothing is timed without one")

    from pulser_amd import NoiseModel, QutipEmulator, Solver, entropy_vn
    from pulser_amd.engine import reduced_density_dm
    from pulser_amd.results import _ptrace_host

    def time_call(x, keep):
        d_a = 2 ** len(keep)
        out = torch.zeros((x.shape[0], d_a, d_a), dtype=torch.complex128, device=x.device)
        for _ in range(3):
            reduced_density_dm(x, keep, out=out)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            reduced_density_dm(x, keep, out=out)
            e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        return us, out

    if not args.skip_kernel:
        print(f"(the call includes the wrapper: argument checks and, with a split, the scratch allocation; n_split = 0; "
              f"{args.launches} timed calls after 3 warm-up ones)")
        print("| matrices | keep | dA | lines touched at most | MB used | device call (us) [min, max] | host: copy (ms) | "
              "host: _ptrace_host (ms) | host route / device call | max abs difference |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for item in args.sizes.split(","):
            n, t = (int(v) for v in item.split(":"))
            dim = 2**n
            nbytes = 16 * t * dim * dim
            free = int(torch.cuda.mem_get_info()[0])
            if free < 2 * nbytes:
                print(f"NOT RUN: N = {n}, T = {t} ({nbytes / 2**30:.2f} GiB; {free / 2**30:.1f} GiB free)", flush=True)
                continue
            x = torch.empty((t, 1, dim, dim), dtype=torch.complex128, device="cuda:0")
            torch.view_as_real(x).normal_()
            host, copy_ms = None, float("nan")
            if not args.skip_host:
                torch.cuda.synchronize()
                tic = time.perf_counter()
                host = x.cpu().numpy()
                copy_ms = 1e3 * (time.perf_counter() - tic)
            for k in (1, 4, 6):
                for where, keep in keeps_of(n, k).items():
                    us, out = time_call(x, keep)
                    med = statistics.median(us)
                    d_a = 2 ** len(keep)
                    host_ms, diff = float("nan"), float("nan")
                    if host is not None:
                        tic = time.perf_counter()
                        ref = np.array([_ptrace_host(host[i, 0], False, keep, 2) for i in range(t)])
                        host_ms = 1e3 * (time.perf_counter() - tic)
                        # (`out` was accumulated into by every call: 3 + launches of them)
                        diff = float(np.max(np.abs(out.cpu().numpy() / (3 + args.launches) - ref)))
                    print(f"| {t} x 2^{n} x 2^{n} | {where} {keep} | {d_a} | {lines_touched(n, keep, t)} | "
                          f"{16e-6 * t * dim * d_a:.2f} | {med:.1f} [{min(us):.1f}, {max(us):.1f}] | {copy_ms:.0f} | "
                          f"{host_ms:.0f} | {(copy_ms + host_ms) * 1e3 / med:.0f} | {diff:.1e} |", flush=True)
            del x, host
            torch.cuda.empty_cache()

    if not args.skip_run:
        from helpers import blockade_radius
        from pulser_amd import problem as P
        from pulser_amd.hamiltonian_data import single_global_channel

        n = args.run_atoms
        coords = P.register_coords(P.square_rect(1, n), blockade_radius())
        smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
        emu = QutipEmulator(single_global_channel(coords, smp, P.C6_LEVEL70, extended=False),
                            noise_model=NoiseModel(dephasing_rate=0.05), solver=Solver.MESOLVER)
        emu.set_evaluation_times(list(np.linspace(0.0, emu._tot_duration / 1000, args.run_times)))
        tic = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            res = emu.run()
        torch.cuda.synchronize()
        print(f"(solve of {n} atoms at {len(res)} evaluation times: {time.perf_counter() - tic:.1f} s, not part of any "
              f"time below)")
        print("| atoms | evaluation times | kept | call | device route (ms) [min, max] | host route, first use (ms) | "
              "max abs difference |")
        print("|---|---|---|---|---|---|---|")
        for keep in ([n // 2], list(range(n // 2 - 2, n // 2 + 2)), list(range(6))):
            res.reduced_states(keep)  # warm-up
            dev_rs, dev_ee = [], []
            for _ in range(args.repeats):
                tic = time.perf_counter()
                a = res.reduced_states(keep)
                dev_rs.append(time.perf_counter() - tic)
                tic = time.perf_counter()
                ea = res.entanglement_entropy(keep)
                dev_ee.append(time.perf_counter() - tic)
            rows = (("reduced_states", dev_rs), ("entanglement_entropy", dev_ee))
            if keep != list(range(6)):  # (the host route ends the store's life on the device: on the last subsystem only)
                for name, ts in rows:
                    print(f"| {n} | {len(res)} | {keep} | {name} | {1e3 * statistics.median(ts):.1f} "
                          f"[{1e3 * min(ts):.1f}, {1e3 * max(ts):.1f}] | - | - |", flush=True)
                continue
            tic = time.perf_counter()
            b = np.array([_ptrace_host(np.asarray(st), False, keep, 2) for st in res.states])
            host_rs = time.perf_counter() - tic
            tic = time.perf_counter()  # (the states are on the host now: the second host call pays no copy)
            eb = np.array([entropy_vn(_ptrace_host(np.asarray(st), False, keep, 2)) for st in res.states])
            host_ee = time.perf_counter() - tic
            print(f"| {n} | {len(res)} | {keep} | reduced_states | {1e3 * statistics.median(dev_rs):.1f} "
                  f"[{1e3 * min(dev_rs):.1f}, {1e3 * max(dev_rs):.1f}] | {1e3 * host_rs:.0f} (with the copies) | "
                  f"{float(np.max(np.abs(a - b))):.1e} |", flush=True)
            print(f"| {n} | {len(res)} | {keep} | entanglement_entropy | {1e3 * statistics.median(dev_ee):.1f} "
                  f"[{1e3 * min(dev_ee):.1f}, {1e3 * max(dev_ee):.1f}] | {1e3 * host_ee:.0f} (states already on the host) | "
                  f"{float(np.max(np.abs(ea - eb))):.1e} |", flush=True)


if __name__ == "__main__":
    main()

"""Observable phase of a V2 backend run (``QutipBackendV2.last_timing["observables_s"]``) whose only observable is one
``Fidelity``: the per-time path (``observe_many_min_times = None`` - per evaluation time one download, one host
normalisation and one ``vdot``; for density matrices the normalisation is an SVD) against the one-call path
(``ryd_overlap_many`` over the device snapshots), for a two-level ket run and a two-level dephasing run of the 3.1-us
anneal at a list of evaluation-time counts.  Each cell is the median of ``--repeats`` runs after one warm-up run of each
path, the two paths alternating.  Then ``ryd_overlap_many`` alone (its two memsets and its launch, HIP events on the
stream, device-resident targets) over snapshot tensors of the same shapes, against the time to read those bytes once at
``--hbm-tbs``.  Prints markdown tables (the source of profiles/overlap_many.md).

On a commit without the route both columns are the per-time path (a run with one ``Fidelity`` never deferred its
states there): ``observe_many_min_times = None`` on this commit runs that same code.

    python tools/overlap_many_bench.py [--ket-atoms 12] [--dm-atoms 8] [--ket-times 128 3101] [--dm-times 128 512]
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
    ap.add_argument("--ket-atoms", type=int, nargs="+", default=[12])
    ap.add_argument("--dm-atoms", type=int, nargs="+", default=[8])
    ap.add_argument("--ket-times", type=int, nargs="+", default=[128, 3101])
    ap.add_argument("--dm-times", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--kernel-shapes", type=str, nargs="+", default=["3100x4096", "3100x16384", "512x256x256"],
                    help="states x dim (kets) or states x dim x dim (density matrices) of the kernel-only timing")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the kernel is compared with, TB/s")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("overlap_many_bench needs the GPU: nothing is timed without one")

    from helpers import blockade_radius
    from pulser_amd import NoiseModel, _lib
    from pulser_amd import problem as P
    from pulser_amd.backend import Fidelity, QutipBackendV2, QutipConfig, RydState
    from pulser_amd.hamiltonian_data import single_global_channel

    has_route = hasattr(QutipBackendV2, "_OVERLAP_MANY_FLOOR")
    print(f"# one-call route for Fidelity: {'present' if has_route else 'ABSENT (both columns are the per-time path)'}")

    def run(inputs, cfg, min_times):
        backend = QutipBackendV2(inputs, config=cfg)
        backend.observe_many_min_times = min_times
        backend.run()
        torch.cuda.synchronize()
        t = QutipBackendV2.last_timing
        return t["observables_s"], t["solve_s"]

    rows = []
    for kind, atoms, counts in (("kets", args.ket_atoms, args.ket_times), ("dephasing", args.dm_atoms, args.dm_times)):
        for n in atoms:
            coords = P.register_coords(P.square_rect(1, n), blockade_radius())
            smp = {k: v[:-1] for k, v in P.anneal_samples().items()}
            inputs = single_global_channel(coords, smp, P.C6_LEVEL70, extended=False)
            rng = np.random.default_rng(n)
            v = rng.normal(size=2**n) + 1j * rng.normal(size=2**n)
            target = RydState(v / np.linalg.norm(v), eigenstates=("r", "g"))
            for count in counts:
                times = "Full" if count == 3101 else np.linspace(1.0 / count, 1.0, count).tolist()
                kw = dict(noise_model=NoiseModel(dephasing_rate=0.05)) if kind == "dephasing" else {}
                cfg = QutipConfig(default_evaluation_times=times, observables=[Fidelity(target)], **kw)
                run(inputs, cfg, None), run(inputs, cfg, 128)  # warm-up of both paths
                per, one, solve = [], [], []
                for _ in range(args.repeats):
                    a, s1 = run(inputs, cfg, None)
                    b, s2 = run(inputs, cfg, 128)
                    per.append(a), one.append(b), solve.extend([s1, s2])
                rows.append((kind, n, count, statistics.median(per), statistics.median(one), statistics.median(solve),
                             (min(per), max(per)), (min(one), max(one))))
                print(f"# {kind}, {n} atoms, {count} times: per-time {rows[-1][3]:.4f} s, one call {rows[-1][4]:.4f} s", flush=True)
    print("| run | atoms | evaluation times | per-time path (s) [min, max] | one call (s) [min, max] | ratio | solve (s) |")
    print("|---|---|---|---|---|---|---|")
    for kind, n, count, a, b, s, (a0, a1), (b0, b1) in rows:
        print(f"| {kind} | {n} | {count} | {a:.4f} [{a0:.4f}, {a1:.4f}] | {b:.4f} [{b0:.4f}, {b1:.4f}] | {a / b:.1f} | {s:.4f} |")

    lib = _lib.load()
    if not hasattr(lib, "ryd_overlap_many"):
        print("# ryd_overlap_many: ABSENT from this library, the call alone is not timed")
        return
    stream = torch.cuda.current_stream().cuda_stream
    print("| states | shape of a state | targets | form | bytes of states (MB) | call (us) [min, max] | at the HBM rate (us) | fraction |")
    print("|---|---|---|---|---|---|---|---|")
    for shape in args.kernel_shapes:
        dims = [int(v) for v in shape.split("x")]
        n_states, dim, density = dims[0], dims[1], len(dims) == 3
        elems = dim * dim if density else dim
        x = torch.randn((n_states, elems), dtype=torch.complex128, device="cuda:0")
        for n_targets, form in ((1, 0), (4, 0)) + (((1, 1),) if density else ()):
            tg = torch.randn((n_targets, dim if form else elems), dtype=torch.complex128, device="cuda:0")
            out = torch.empty((n_states, n_targets), dtype=torch.complex128, device="cuda:0")
            norm = torch.empty(n_states, dtype=torch.float64, device="cuda:0")

            def call():
                _lib.check(lib.ryd_overlap_many(x.data_ptr(), n_states, elems, dim, int(density), tg.data_ptr(), n_targets,
                                                form, out.data_ptr(), norm.data_ptr(), 0, stream))

            for _ in range(3):
                call()
            torch.cuda.synchronize()
            us = []
            for _ in range(max(args.repeats, 5)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1))
            nbytes = 16.0 * n_states * elems
            roof = nbytes / (args.hbm_tbs * 1e12) * 1e6
            med = statistics.median(us)
            print(f"| {n_states} | {'x'.join(map(str, dims[1:]))} | {n_targets} | {form} | {nbytes / 1e6:.1f} | {med:.1f} "
                  f"[{min(us):.1f}, {max(us):.1f}] | {roof:.1f} | {roof / med:.2f} |")
        del x


if __name__ == "__main__":
    main()

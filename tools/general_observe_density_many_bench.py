"""The one-call observable path of multi-level and XY master-equation runs against the per-time path (the source of
profiles/general_observe_density_many.md).

1. Observable phase of a V2-backend run (``QutipBackendV2.last_timing["observables_s"]``) with
   ``general_density_one_call`` on and off - off is the default route: one host copy, an SVD, one upload and one
   ``ryd_general_observe + RYD_OBS_DENSITY`` call per evaluation time - for a 10-atom XY dephasing run (D = 1 024) and a
   6-atom 3-level run with relaxation and dephasing (D = 729), each at 128 evaluation times, with Occupation,
   CorrelationMatrix, Energy and EnergySecondMoment configured.  Median of ``--repeats`` runs after one warm-up run, the
   two routes alternating, with the spread.
2. The kernels alone: device time per matrix (events on the engine's stream around the C calls, no read-back inside the
   bracket) of ``ryd_general_observe_density_many`` over 128 random matrices against 128 calls of
   ``ryd_general_observe + RYD_OBS_DENSITY``, on the noiseless engines of the same two registers.

    python tools/general_observe_density_many_bench.py [--workloads xy10 l3_6] [--repeats 3] [--duration 128]
                                                       [--parts backend kernel]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from general_observe_many_bench import three_level_inputs, xy_inputs  # noqa: E402

N_TIMES = 128


def workloads():
    from pulser_amd import NoiseModel

    return {"xy10": (lambda dur: xy_inputs(2, 5, dur), "d", NoiseModel(dephasing_rate=0.05), 2, 10),
            "l3_6": (lambda dur: three_level_inputs(2, 3, dur), "r",
                     NoiseModel(relaxation_rate=0.5, dephasing_rate=0.7, hyperfine_dephasing_rate=0.3), 3, 6)}


def backend_part(names, repeats, duration):
    import torch

    from pulser_amd.backend import CorrelationMatrix, Energy, EnergySecondMoment, Occupation, QutipBackendV2, QutipConfig

    print("| workload | D | evaluation times | per-time route: observables_s, median (min .. max) | one-call route | ratio "
          "| solve (s) | launches per-time / one-call | device memory held by the snapshots |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in names:
        make, one, nm, d, n = workloads()[name]
        inputs = make(duration)
        times = np.linspace(1.0 / N_TIMES, 1.0, N_TIMES).tolist()
        cfg = QutipConfig(default_evaluation_times=times, noise_model=nm, observables=[
            Occupation(one_state=one), CorrelationMatrix(one_state=one), Energy(), EnergySecondMoment()])

        def run(on):
            backend = QutipBackendV2(inputs, config=cfg)
            backend.general_density_one_call = on
            torch.cuda.reset_peak_memory_stats()
            backend.run()
            t = QutipBackendV2.last_timing
            print(f"# {name}, {'one-call' if on else 'per-time'}: observables {t['observables_s']:.4f} s, solve {t['solve_s']:.3f} s",
                  flush=True)
            return (t["observables_s"], t["solve_s"], QutipBackendV2.last_observable_engine_stats["n_launches"],
                    torch.cuda.max_memory_allocated())

        obs, solve, launches, peak = {False: [], True: []}, [], {}, {}
        for on in (False, True):
            run(on)  # warm-up
        for _ in range(repeats):
            for on in (False, True):
                o, s, launches[on], peak[on] = run(on)
                obs[on].append(o)
                solve.append(s)
        cell = lambda v: f"{statistics.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"  # noqa: E731
        D = d**n
        print(f"| {name} | {D} | {N_TIMES} | {cell(obs[False])} | {cell(obs[True])} | "
              f"{statistics.median(obs[False]) / statistics.median(obs[True]):.1f} | {statistics.median(solve):.3f} | "
              f"{launches[False]} / {launches[True]} | {N_TIMES * 16 * D * D / 2**20:.0f} MiB "
              f"(torch peak {peak[False] / 2**20:.0f} / {peak[True] / 2**20:.0f} MiB) |", flush=True)


def kernel_part(names, repeats, duration):
    import torch

    from pulser_amd.backend import QutipBackendV2, QutipConfig
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general

    print("| register | D | what | one call over 128 matrices: us per matrix, median (min .. max) "
          "| 128 per-time calls: us per matrix | ratio |")
    print("|---|---|---|---|---|---|")
    for name in names:
        make, one, nm, d, n = workloads()[name]
        sim = QutipBackendV2(make(duration), config=QutipConfig(observables=[]))._sim_obj
        hd = sim._get_noiseless_data(False)
        noiseless = dict(hd.problem(hd.noise_trajectories[0], sim._sampling_rate))
        noiseless["collapse_ops"] = []
        D = d**n
        with GeneralEngine(lower_general(noiseless, mesolve=False, matrix_free=True)) as eng:
            assert eng.apply_path() in ("fused", "fused_lds")
            rng = np.random.default_rng(1)
            x = torch.from_numpy(rng.normal(size=(N_TIMES, 1, D, D)) + 1j * rng.normal(size=(N_TIMES, 1, D, D))).to(eng.device)
            tt = np.ascontiguousarray(np.linspace(0.001, duration / 1000, N_TIMES))
            out = torch.empty((N_TIMES, 1, n * n + n + 3), dtype=torch.float64, device=eng.device)
            lib, h, st = eng.lib, eng._h, eng._stream()

            def many(what):
                rc = lib.ryd_general_observe_density_many(h, x.data_ptr(), N_TIMES, 1, D * D, D * D, tt.ctypes.data, what, d, n,
                                                          1, out.data_ptr(), st)
                assert rc == 0, lib.ryd_last_error()

            def single(what):
                for i in range(N_TIMES):
                    rc = lib.ryd_general_observe(h, x[i].data_ptr(), float(tt[i]), what | 8, d, n, 1, out[i].data_ptr(), st)
                    assert rc == 0, lib.ryd_last_error()

            for label, what in (("pair sums", 3), ("energy moments", 4), ("all", 7)):
                res = {}
                for fn in (many, single):
                    fn(what)  # warm-up (scratch grows here)
                    torch.cuda.synchronize()
                    us = []
                    for _ in range(repeats):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn(what)
                        b.record()
                        torch.cuda.synchronize()
                        us.append(a.elapsed_time(b) * 1000 / N_TIMES)
                    res[fn.__name__] = us
                cell = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"  # noqa: E731
                print(f"| {name} | {D} | {label} | {cell(res['many'])} | {cell(res['single'])} | "
                      f"{statistics.median(res['single']) / statistics.median(res['many']):.1f} |", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["xy10", "l3_6"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--duration", type=int, default=128)
    ap.add_argument("--parts", nargs="+", default=["backend", "kernel"], choices=["backend", "kernel"])
    args = ap.parse_args()
    tic = time.perf_counter()
    if "kernel" in args.parts:
        kernel_part(args.workloads, args.repeats, args.duration)
    if "backend" in args.parts:
        backend_part(args.workloads, args.repeats, args.duration)
    print(f"# total {time.perf_counter() - tic:.1f} s")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What plotting a non-diagonal observable costs after a run: wall clock of ``results.expect([sum_k sigma_x^k])`` on a
fresh ``QutipEmulator(<north-star inputs>, evaluation_times="Full").run()`` (3 101 stored states), and - where the
checkout has it - the time of the ``engine.expect_sparse`` kernel alone over the same snapshots, with the bytes it
has to move (the states once, the triplets once per state tile) over that time.

    python tools/expect_bench.py [--atoms 14 12] [--repeat 3] [--kernel-reps 10] [--tree DIR]

--tree DIR: import ``pulser_amd`` from another checkout (a built tree of the parent commit) - the same script, the same
process layout, so that two commits are compared by running this file twice.  One JSON line per configuration.
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
TRIPLET_BYTES = 4 + 4 + 16  # row, column, value


def sigma_x_sum(n):
    import scipy.sparse as sp

    sx = sp.csr_matrix(np.array([[0, 1], [1, 0]], dtype=complex))
    return sum(sp.kron(sp.kron(sp.identity(2**k), sx), sp.identity(2**(n - 1 - k))) for k in range(n)).tocsr()


def fresh_results(inputs):
    from pulser_amd import QutipEmulator

    emu = QutipEmulator(inputs, evaluation_times="Full")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return emu.run()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, nargs="+", default=[14, 12])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import torch

    import pulser_amd.engine as engine
    from api_bench import north_star_inputs

    assert os.path.abspath(engine.__file__).startswith(os.path.abspath(args.tree)), engine.__file__
    for n in args.atoms:
        inputs = north_star_inputs(n)
        op = sigma_x_sum(n)
        walls, values, on_device = [], None, None
        for rep in range(args.repeat + 1):  # the first round warms up the solve, the upload paths and the kernel
            res = fresh_results(inputs)
            store = res.states[1]._store
            torch.cuda.synchronize()
            tic = time.perf_counter()
            values = res.expect([op])[0]
            torch.cuda.synchronize()
            if rep:
                walls.append(time.perf_counter() - tic)
            on_device = store.device_tensor is not None
            if rep < args.repeat:
                del res, store
        row = {"label": args.label or os.path.basename(os.path.abspath(args.tree)), "atoms": n, "n_states": len(values),
               "nnz": int(op.nnz), "expect_wall_ms": [round(w * 1e3, 3) for w in walls],
               "expect_wall_ms_median": round(float(np.median(walls)) * 1e3, 3), "snapshots_still_on_device": bool(on_device),
               "checksum": float(np.sum(values))}
        if hasattr(engine, "expect_sparse") and on_device:
            dev = store.device_tensor
            x = dev[:, 0]
            engine.expect_sparse(x, op)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.kernel_reps)]
            lib, check = engine._lib.load(), engine._lib.check
            # the launch alone (zeroing of `out` included): the triplets are uploaded once, outside the timed window
            from scipy.sparse import csr_matrix

            m = csr_matrix(op).astype(np.complex128)
            m.sum_duplicates()
            m.sort_indices()
            rows = np.repeat(np.arange(m.shape[0], dtype=np.int32), np.diff(m.indptr))
            rd, cd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (rows, m.indices))
            vd = torch.from_numpy(np.ascontiguousarray(m.data)).cuda()
            out = torch.empty(x.shape[0], dtype=torch.complex128, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            for a, b in ev:
                a.record()
                check(lib.ryd_expect_sparse(x.data_ptr(), int(x.shape[0]), int(x.stride(0)), int(x.shape[1]), 0, rd.data_ptr(),
                                            cd.data_ptr(), vd.data_ptr(), int(m.nnz), out.data_ptr(), 0, stream))
                b.record()
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in ev]
            tile = 8  # kExpectTile (pulser_amd/csrc/k_expect.hpp)
            n_tiles = -(-int(x.shape[0]) // tile)
            state_bytes = int(x.shape[0]) * int(x.shape[1]) * 16
            triplet_bytes = n_tiles * int(m.nnz) * TRIPLET_BYTES
            gathered = 2 * 16 * int(m.nnz) * int(x.shape[0])  # what the lanes ask of L2: two entries per term and state
            k_ms = float(np.median(ms))
            row.update({"kernel_ms": [round(v, 4) for v in ms], "kernel_ms_median": round(k_ms, 4),
                        "state_bytes": state_bytes, "triplet_bytes": triplet_bytes,
                        "must_move_GBps": round((state_bytes + triplet_bytes) / k_ms / 1e6, 1),
                        "gathered_bytes": gathered, "gathered_GBps": round(gathered / k_ms / 1e6, 1),
                        "kernel_matches_expect": bool(np.allclose(out.cpu().numpy()[:].real, values[1:], rtol=0, atol=1e-9))})
        print(json.dumps(row), flush=True)
        del res, store


if __name__ == "__main__":
    main()

"""Per-launch cost of k_split_reg from a rocprofv3 --kernel-trace CSV of bench.py (profiles/check_segments.md):

  python tools/check_segments_fit.py trace_kernel_trace.csv [steps]

Every k_split_reg launch follows a k_split_coefs launch whose grid has one row per stage record, so the trace itself
carries the stage count of each run.  Prints the least-squares fit duration = intercept + slope x stages (plain runs and
the launches of a step-size check separately: a check is a 1-sub-step run followed by a 2-sub-step run), the mean
k_split_coefs duration, the idle gaps between consecutive kernels of the stream and the launch counts per step."""
import csv, sys

import numpy as np


def main(path, steps=4):
    rows = [r for r in csv.DictReader(open(path)) if r["Kind"] == "KERNEL_DISPATCH"]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ker = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"])))
           for r in rows]
    first = next(i for i, k in enumerate(ker) if k[0].startswith("k_split_coefs"))
    last = max(i for i, k in enumerate(ker) if "k_split_reg" in k[0])
    ker = ker[first:last + 1]
    runs, coefs, gaps_cr, gaps_rc, others = [], [], [], [], {}
    for i, (name, t0, t1, gy) in enumerate(ker):
        if "k_split_reg" in name:
            pn, pt0, pt1, pgy = ker[i - 1]
            assert pn.startswith("k_split_coefs"), pn
            runs.append((pgy, (t1 - t0) * 1e-3, name))
            gaps_cr.append((t0 - pt1) * 1e-3)
        elif name.startswith("k_split_coefs"):
            coefs.append((gy, (t1 - t0) * 1e-3))
            if i and "k_split_reg" in ker[i - 1][0]:
                gaps_rc.append((t0 - ker[i - 1][2]) * 1e-3)
        else:
            others[name.split("(")[0]] = others.get(name.split("(")[0], 0) + 1
    n = np.array([r[0] for r in runs], float)
    d = np.array([r[1] for r in runs], float)
    # the launches of a check: k_split_reg_seg (a stretch and its check as segments), or, as launches of their own, 11 (or 7)
    # records = the wide step, then 21 (or 13) = its two halves
    seg = np.array(["k_split_reg_seg" in r[2] for r in runs])
    chk = np.zeros(len(runs), bool)
    for i in range(len(runs) - 1):
        if (n[i], n[i + 1]) in ((11, 21), (7, 13)) and not seg[i] and not seg[i + 1]:
            chk[i] = chk[i + 1] = True
    print(f"launches: {len(runs)} k_split_reg ({int(chk.sum())} of them in {int(chk.sum()) // 2} checks of two launches, {int(seg.sum())} "
          f"segment launches), {len(coefs)} k_split_coefs "
          f"over {steps} steps = {len(runs) / steps:.1f} + {len(coefs) / steps:.1f} per step; other kernels {others}")
    print(f"stage records: {int(n.sum())} over {steps} steps = {n.sum() / steps:.0f} per step")
    for label, m in (("plain runs", ~chk & ~seg), ("check launches", chk), ("segment launches", seg), ("all", np.ones(len(runs), bool))):
        if m.sum() < 2 or np.ptp(n[m]) == 0:
            continue
        A = np.stack([np.ones(m.sum()), n[m]], 1)
        (c0, c1), res, *_ = np.linalg.lstsq(A, d[m], rcond=None)
        rms = float(np.sqrt(np.mean((A @ np.array([c0, c1]) - d[m]) ** 2)))
        print(f"{label}: {int(m.sum())} launches, stages {int(n[m].min())} .. {int(n[m].max())}: duration = {c0:.1f} us + {c1:.3f} us x stages (rms {rms:.1f} us)")
    cd = np.array([c[1] for c in coefs])
    print(f"k_split_coefs: mean {cd.mean():.1f} us, median {np.median(cd):.1f}, min {cd.min():.1f}, max {cd.max():.1f}")
    for label, g in (("k_split_coefs -> k_split_reg", gaps_cr), ("k_split_reg -> next k_split_coefs", gaps_rc)):
        g = np.array(g)
        print(f"idle gap {label}: median {np.median(g):.1f} us, mean {g.mean():.1f}, 90th percentile {np.percentile(g, 90):.1f} ({len(g)} gaps)")
    print(f"sum over the trace: k_split_reg {d.sum() / steps * 1e-3:.2f} ms, k_split_coefs {cd.sum() / steps * 1e-3:.2f} ms, "
          f"gaps {(np.sum(gaps_cr) + np.sum(gaps_rc)) / steps * 1e-3:.2f} ms per step")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4)

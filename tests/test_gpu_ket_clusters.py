"""The two-level Schroedinger path from 15 to 25 atoms (and its pass kernels below) against exact cluster-product kets.

Every case of the table in tests/ket_cluster_ref.py is run on the plan it names and the WHOLE ket is compared on the
device, at every evaluation time (t = 0 included), with the cluster-product reference: registers made of strongly
interacting clusters of 1 to 6 atoms, 1000 um apart, whose ket is exactly the tensor product of tight oracle solutions on
at most 64 amplitudes (tests/ket_cluster_ref.py; tests/test_ket_cluster_ref.py pins it on the full-space oracle and
checks the table).  No two atoms of a register are alike (own position in an own cluster, own waveforms, own entangled
initial ket) and the atoms of a cluster are scattered over the atom indices so that interacting pairs straddle every pair
of bit classes of the plan (low 4 tile bits, kept tile bits, tile bits of the first tiling only, each high-bit group): a
high-bit group on the wrong bits, two atoms' coefficients exchanged, an E0 entry read at the wrong index, a gauge phase
with the wrong sign are O(0.01 - 1) errors - the older product-state tests (identical far-apart atoms, one global real
drive) are blind to every one of them.

Plans (each case asserts from ``eng.stats()`` that its plan ran):

* split-operator passes on the default path, ``k_split_s<12>`` in tan form: 15, 17, 20 atoms (3, 5, 8 high bits), complex
  and real per-atom drives, the global drive, |g...g>, the 6-um pitch, evaluation times inside one knot interval, a batch
  of two different 17-atom registers (``e0_stride`` != 0);
* 2^13 tiles (``k_split_s<13>``) at 21 and 22 atoms, the same registers on two passes of 2^12 tiles
  (``split_small_tiles``), one without the step-size controller (``split_fixed``);
* three tilings at 23 (5 + 6 high bits) and 25 atoms (6 + 7 high bits, 0.5 GiB, 64-bit offsets);
* the non-static pass kernel ``k_split_t<SPLIT_NT>`` (tiles below 2^12: the split path forced at 10 atoms);
* the pass kernels forced at 13 and 14 atoms (``split_no_loop``), where the tight fixtures also apply;
* CF4 + Taylor on the ``k_apply`` passes at 17, 21 (one launch) and 24 atoms (2^14 tiles + two passes), ``tol=1e-13``.

Which inputs reach which kernel instantiation, and the ones no case reaches: profiles/ket_clusters.md.

Bars (both from the project): max |psi - psi_ref| < 1e-7 on every amplitude and |psi - psi_ref|_2 < 1e-7 (the
controller's sequence budget of 8e-8 is a 2-norm bound; the reference floor is below 1e-11); where the controller runs,
also |psi - psi_ref|_2 <= 3 x its booked estimate + 1e-9; | |psi|_2 - 1 | < 1e-9.  Measured maxima: profiles/ket_clusters.md.

What this cannot see: couplings of more than 6 atoms (tests/ket_cluster_ref.py, module docstring).
"""
import numpy as np
import pytest

import ket_cluster_ref as R

from pulser_amd.engine import Engine
from pulser_amd.terms import lower

pytestmark = pytest.mark.gpu

NORM_DRIFT = 1e-9


def _check_plan(case, s):
    """The intended plan ran: from the solve statistics, by the means of the existing tests."""
    n, ns = case.n, case.setups[0].ns
    path = dict(case.path)
    if case.plan == "taylor":
        assert s["passes"] == R.apply_plan(n, len(case.setups))[1], s
        assert s["reserved"][0] == 0.0 and s["n_applications"] > 0, s  # nothing booked by a step-size controller
        assert 2 <= s["last_order"] <= 32 and s["n_launches"] == s["passes"] * s["n_applications"], s  # the Taylor order; tiled passes
        return
    assert s["passes"] == R.split_passes(n, path.get("split_small_tiles", False)), s
    # (`last_order` is the Taylor order the schedule builder worked out and says nothing about a split-operator run)
    if case.controlled:
        assert 0 < s["reserved"][0] <= R.SPLIT_BUDGET, s  # the controller's accumulated estimate met its target
        assert s["n_applications"] >= max(10 * ns // 8, 6 * (len(case.times) - 1)), s
    else:
        # one 6-stage sub-step per schedule step (two steps per knot interval and evaluation time), nothing booked
        assert s["reserved"][0] == 0.0 and s["n_applications"] == 6 * s["n_steps"] and s["n_steps"] >= 2 * ns, s


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.CASES])
def test_kets_match_the_cluster_product(case):
    import torch

    times = case.times
    sols = [R.cluster_solutions(s, times) for s in case.setups]

    def reference(b, i, device):
        s = case.setups[b]
        return R.product(s.layout, [c[i] for c in sols[b]], s.n, device)

    worst = {"amp": 0.0, "norm2": 0.0, "drift": 0.0}

    def book(got, b, i):
        ref = reference(b, i, got.device)
        worst["drift"] = max(worst["drift"], abs(float(torch.linalg.vector_norm(got).item()) - 1.0))
        ref.sub_(got)
        worst["norm2"] = max(worst["norm2"], float(torch.linalg.vector_norm(ref).item()))
        worst["amp"] = max(worst["amp"], float(ref.abs().max().item()))

    with Engine(lower([R.assemble(s) for s in case.setups]), mode="sesolve") as eng:
        if case.path:
            eng.set_path(False, **dict(case.path))
        state = torch.empty(eng.state_shape, dtype=torch.complex128, device=eng.device)
        for b in range(len(case.setups)):
            state[b].copy_(reference(b, 0, eng.device))
            book(state[b], b, 0)
        opts = {"tol": 1e-13} if case.method == "taylor" else {}
        snaps = eng.solve(state, np.asarray(times), method=case.method, **opts)
        stats = eng.stats()
        for i in range(1, len(times)):
            for b in range(len(case.setups)):
                book(snaps[i - 1][b], b, i)
        differ = float(torch.linalg.vector_norm(snaps[-1][0] - snaps[-1][1]).item()) if len(case.setups) > 1 else None
    print(f"ket-clusters {case.name}: max-abs {worst['amp']:.2e}, 2-norm {worst['norm2']:.2e}, norm drift {worst['drift']:.2e}; "
          f"n_steps {stats['n_steps']}, launches {stats['n_launches']}, applications {stats['n_applications']}, "
          f"passes {stats['passes']}, last_order {stats['last_order']}, reserved {stats['reserved']}")
    _check_plan(case, stats)
    assert worst["amp"] < R.AMP_TOL, worst
    assert worst["norm2"] < R.NORM_BAR, worst
    if case.controlled:
        assert worst["norm2"] <= 3 * stats["reserved"][0] + 1e-9, (worst, stats["reserved"])  # the estimate covers the error
    assert worst["drift"] < NORM_DRIFT, worst
    if differ is not None:  # the batch entries really differ
        assert differ > 1e-3 and case.setups[0].layout != case.setups[1].layout, differ

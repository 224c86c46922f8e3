"""GPU: the uniform-drive kernels of the register-resident split-operator path (k_split_reg_uni, k_split_reg_seg_uni: one
coefficient record per sequence and stage; profiles/uniform_drive.md) against the general kernels with a record per atom.

  * 12, 13 and 14 atoms, three sequences of the anneal with different amplitude and detuning scales on a Global channel, the
    120 ns behind the 0.5-us kink (one-knot steps next to the kink, multi-knot steps behind them, a step-size check), the
    check as segments of one launch and in launches of its own: the same stages and launches as with
    ``uniform_drive=False``, the uniform kernels ran, and the kets agree within 1e-12 - the bound
    tests/test_gpu_split_reg_waits.py applies to the default kernel against the pass-by-pass launches.  Measured on MI355X:
    5.0e-16 (12 atoms), 2.6e-16 (13), 4.7e-16 (14), the same with and without segments: the lane's detuning sum is a product
    instead of a chain of additions, everything else is the same arithmetic.
  * A table with one atom's ``det_scale`` off by 1e-3, and a complex (gauged) drive: no uniform launch, and the kets are bit
    for bit those of ``uniform_drive=False``.
"""
from __future__ import annotations

import numpy as np
import pytest

from helpers import blockade_radius
from pulser_amd import problem as P
from pulser_amd.engine import Engine
from pulser_amd.terms import lower

pytestmark = pytest.mark.gpu

T0, T1 = 0.5, 0.62  # us: the kink at the end of the amplitude ramp, 120 ns of the sweep
SCALES = ((1.0, 1.0), (0.8, 1.1), (1.15, 0.9))  # (amplitude, detuning) of the three sequences


def _probs(n, phase=0.0):
    coords = P.register_coords(P.triangular_rect(2, 7) if n == 14 else P.square_rect(1, n), blockade_radius())
    out = []
    for fa, fd in SCALES:
        s = P.anneal_samples()
        out.append(P.make_ising_problem(coords, {"amp": fa * s["amp"], "det": fd * s["det"], "phase": s["phase"] + phase}))
    return out


def _run(tables, **kw):
    with Engine(tables, mode="sesolve") as eng:
        eng.set_path(False, **kw)
        st = eng.new_state()
        eng.evolve(st, T0, T1, method="split")
        return st.cpu().numpy(), eng.stats(), eng.uniform_launches()


@pytest.mark.parametrize("check_segments", [True, False])
@pytest.mark.parametrize("n", [12, 13, 14])
def test_uniform_kernels_equal_the_general_ones(n, check_segments):
    tables = lower(_probs(n))
    uni, s_uni, l_uni = _run(tables, check_segments=check_segments)
    gen, s_gen, l_gen = _run(tables, check_segments=check_segments, uniform_drive=False)
    diff = float(np.max(np.abs(uni - gen)))
    print(f"n = {n}, segments {check_segments}: max |uniform - general| = {diff:.3e}; stages {s_uni['n_applications']} / "
          f"{s_gen['n_applications']}; launches {s_uni['n_launches']} / {s_gen['n_launches']}; uniform launches {l_uni} / {l_gen}")
    assert s_uni["n_applications"] == s_gen["n_applications"] and s_uni["n_launches"] == s_gen["n_launches"]
    assert s_uni["n_steps"] == s_gen["n_steps"]
    assert l_uni == s_uni["n_launches"] and l_gen == 0  # every launch of the run was a uniform one / none was
    assert s_uni["n_launches"] >= 2  # at least a stretch and a check
    assert diff < 1e-12
    assert np.allclose(np.linalg.norm(uni, axis=-1), 1.0, atol=1e-12)
    assert np.max(np.abs(uni[0] - uni[1])) > 1e-3 and np.max(np.abs(uni[0] - uni[2])) > 1e-3  # the sequences really differ


@pytest.mark.parametrize("case", ["det_scale", "gauged"])
def test_tables_that_are_not_uniform_keep_the_general_kernels(case):
    n = 12
    if case == "det_scale":
        tables = lower(_probs(n))
        tables.desc["det_scale"][1, 5] *= 1.0 + 1e-3  # one atom of one sequence
    else:
        tables = lower(_probs(n, phase=0.5))  # a complex drive: gauged away inside the real kernels, per-atom phases
    on, s_on, l_on = _run(tables)
    off, s_off, l_off = _run(tables, uniform_drive=False)
    print(f"{case}: uniform launches {l_on} / {l_off}; launches {s_on['n_launches']} / {s_off['n_launches']}; "
          f"max |on - off| = {float(np.max(np.abs(on - off))):.1e}")
    assert l_on == 0 and l_off == 0
    assert s_on["n_launches"] == s_off["n_launches"] and s_on["n_launches"] >= 2  # (the register-resident kernel ran)
    assert np.array_equal(on, off)

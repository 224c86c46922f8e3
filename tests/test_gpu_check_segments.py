"""GPU: a stretch of k_split_reg and the step-size check behind it as segments of ONE launch (k_split_reg_seg, SplitRun.nseg;
profiles/check_segments.md) give, bit for bit, the kets of the launches they replace - the switch set_path(check_segments=False)
restores those launches on the same engine:

  (a) the first 400 ns of the anneal (cold-start check periods 16 / 32 / 64 / 128 knots: at least four checks), and 560 ns of
      it (the one-knot steps on both sides of the kink at 0.5 us: mixed runs inside the segments);
  (b) stretches that are rolled back: a square pulse of 15 rad/us from t = 0 over 200 ns on registers at 5 um - the sub-step
      the check at the product state lets through is far over its allowance 16 knots later (12 checks, reserved[3] = 3
      roll-backs at 12, 13 and 14 atoms on the separate launches, measured before the segment launch existed; the same
      pulse at the blockade radius is not rolled back);
  (c) the fallbacks: a call whose stretches end on evaluation times, and one with snapshots at every 10th knot - states and
      snapshots bit-equal, never more launches;
  (d) 14 atoms against the pass-by-pass launches, which share no stage code with the register-resident kernels.

12, 13 and 14 atoms, 3 different sequences each (scale factors spread like bench.py's spread_tables)."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from helpers import blockade_radius
from pulser_amd import problem as P
from pulser_amd.engine import Engine
from pulser_amd.terms import lower

pytestmark = pytest.mark.gpu

B = 3
# checks the controller takes on the cases below (its own trace, counted on the separate launches; 12, 13 and 14 atoms alike)
CHECKS = {0.4: 7, 0.56: 11}   # the anneal from t = 0 to 0.4 / 0.56 us
SQUARE_CHECKS = 12            # the square pulse over 200 ns


def _coords(n, spacing=None):
    layout = P.triangular_rect(2, 7) if n == 14 else P.square_rect(1, n)
    return P.register_coords(layout, blockade_radius() if spacing is None else spacing)


def _spread(prob, seed=7, spread=0.01):
    """B different sequences on one register: per-sequence amplitude / detuning scale factors (bench.py: spread_tables)."""
    t = lower([prob])
    desc = np.repeat(t.desc, B, axis=0)
    rng = np.random.default_rng(seed)
    amp = 1.0 + spread * (2.0 * rng.random(B) - 1.0)
    det = 1.0 + spread * (2.0 * rng.random(B) - 1.0)
    amp[0] = det[0] = 1.0
    desc["drive_scale"] *= amp[:, None]
    desc["det_scale"] *= det[:, None]
    return dataclasses.replace(t, batch=B, desc=desc)


def anneal_tables(n):
    return _spread(P.make_ising_problem(_coords(n), P.anneal_samples()))


def square_tables(n, amp=15.0, det=0.0, duration=201, spacing=5.0):
    """A square pulse from t = 0 (docs/KERNEL_NOTES.md 5.10): the product state the first check sits on says nothing about the
    sub-steps 16 knots later."""
    z = np.zeros(duration)
    return _spread(P.make_ising_problem(_coords(n, spacing), {"amp": z + amp, "det": z + det, "phase": z}))


def _both(tables, run):
    """run(eng) -> arrays, on ONE engine: the default (segments), then set_path(check_segments=False); fresh state, cold
    controller (another state buffer, t = 0 again) and zeroed statistics each time."""
    out = {}
    with Engine(tables, mode="sesolve") as eng:
        for name, on in (("segments", True), ("launches", False)):
            eng.set_path(False, check_segments=on)
            eng.reset_stats()
            arrays = run(eng)
            out[name] = ([np.array(a) for a in arrays], eng.stats())
    return out


def _assert_same_run(out, what):
    (xs, s), (xl, l) = out["segments"], out["launches"]
    for a, c in zip(xs, xl):
        assert a.shape == c.shape and np.array_equal(a.view(np.float64), c.view(np.float64)), \
            f"{what}: max |segments - launches| = {np.max(np.abs(a - c)):.3e}"
    print(f"{what}: stages {s['n_applications']} / {l['n_applications']}, steps {s['n_steps']} / {l['n_steps']}, launches "
          f"{s['n_launches']} / {l['n_launches']}, reserved {s['reserved'][:4]} / {l['reserved'][:4]}")
    assert s["n_applications"] == l["n_applications"] and s["n_steps"] == l["n_steps"]
    assert s["reserved"][:4] == l["reserved"][:4]
    return s, l


def _evolve(t1):
    def run(eng):
        st = eng.new_state()
        eng.evolve(st, 0.0, t1, method="split")
        return [st.cpu().numpy()]
    return run


@pytest.mark.parametrize("n", [12, 13, 14])
@pytest.mark.parametrize("t1", [0.4, 0.56])
def test_several_checks(n, t1):
    """The cold-start periods 16 / 32 / 64 / 128 knots alone give a check at 0, 16, 48, 112 and 240 ns; the amplitude trigger on
    the ramp adds some.  CHECKS pins what the controller's trace (RYD_DEV=1 RYD_SPLIT_TRACE=1) counted with the launches of
    their own, before the segment launch existed, the same at 12, 13 and 14 atoms: 7 checks over 400 ns, 11 over 560 ns - and
    ONE roll-back, at the first 9-knot sub-step behind the cold start: this case is not free of them.
    Launches: a check with a run kept back before it is one launch instead of three; the first check of a call, and the first
    one behind a roll-back, have no such run and are one launch instead of two - "two fewer per check" cannot hold for those
    two, so the bound is 2 per check taken less one each for the call's first check and for every roll-back.
    Measured: 8 / 20 launches over 400 ns, 12 / 32 over 560 ns: 12 and 20 fewer, the bound exactly."""
    out = _both(anneal_tables(n), _evolve(t1))
    s, l = _assert_same_run(out, f"n = {n}, anneal 0 .. {t1} us")
    print(f"  {CHECKS[t1]} checks: {l['n_launches'] - s['n_launches']} launches fewer")
    assert l["n_launches"] - s["n_launches"] >= 2 * CHECKS[t1] - 1 - int(l["reserved"][3])


@pytest.mark.parametrize("n", [12, 13, 14])
def test_a_rolled_back_stretch(n):
    out = _both(square_tables(n), _evolve(0.2))
    s, l = _assert_same_run(out, f"n = {n}, square pulse 15 rad/us over 200 ns")
    assert l["reserved"][3] >= 1 and s["reserved"][3] == l["reserved"][3]
    # (12 checks and 3 roll-backs in the controller's trace at 12, 13 and 14 atoms; measured 13 / 34 launches)
    assert l["n_launches"] - s["n_launches"] >= 2 * SQUARE_CHECKS - 1 - int(l["reserved"][3])


@pytest.mark.parametrize("n", [12, 13, 14])
def test_fallbacks_stretches_that_end_on_evaluation_times_and_snapshots_inside_runs(n):
    tables = anneal_tables(n)

    def solve(times):
        def run(eng):
            st = eng.new_state()
            snaps = eng.solve(st, np.asarray(times), method="split")
            return [snaps.cpu().numpy(), st.cpu().numpy()]
        return run

    for what, times in (("evaluation times at 0.1, 0.25, 0.4 us", [0.0, 0.1, 0.25, 0.4]),
                        ("snapshots at every 10th knot", np.arange(0, 41) * 0.01)):
        out = _both(tables, solve(times))
        s, l = _assert_same_run(out, f"n = {n}, {what}")
        assert s["n_launches"] <= l["n_launches"]  # (a fallback still keeps the check's own two launches in one)


def _ramp_problem(n, seed, T=81):
    """tests/test_gpu_split_reg_waits.py: per-atom real drives ramping up from zero, detunings through resonance, 80 ns."""
    rng = np.random.default_rng(seed)
    s = np.arange(T) / (T - 1.0)
    z = np.zeros(T)
    prob = P.make_ising_problem(_coords(n), {"amp": z, "det": z, "phase": z})
    loc = {}
    for q in range(n):
        a, d0, d1 = rng.uniform(4, 12), rng.uniform(-14, -6), rng.uniform(2, 10)
        loc[q] = {"amp": a * s, "det": d0 + (d1 - d0) * s, "phase": z}
    prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": loc}}
    prob["collapse_ops"] = []
    prob["depolarizing_pauli_2ds"] = {}
    return prob


def test_segment_launches_meet_the_pass_by_pass_kernels_at_14_atoms():
    probs = [_ramp_problem(14, seed=100 * 14 + b) for b in range(B)]
    outs, stats = {}, {}
    for name, kw in (("segments", {}), ("launches", {"check_segments": False}), ("passes", {"split_no_loop": True})):
        with Engine.from_problems(probs, mode="sesolve") as eng:
            eng.set_path(False, **kw)
            st = eng.new_state()
            eng.evolve(st, 0.0, 0.08, method="split")
            outs[name], stats[name] = st.cpu().numpy(), eng.stats()
    diff = float(np.max(np.abs(outs["segments"] - outs["passes"])))
    print(f"max |segments - passes| = {diff:.3e}; stages {stats['segments']['n_applications']} / {stats['passes']['n_applications']}; "
          f"launches {stats['segments']['n_launches']} / {stats['passes']['n_launches']}")
    assert stats["segments"]["n_applications"] == stats["passes"]["n_applications"]
    # the default really took segment launches: fewer than with the switch off, and the same kets
    print(f"launches with the check's own launches: {stats['launches']['n_launches']}")
    assert stats["segments"]["n_launches"] < stats["launches"]["n_launches"]
    assert np.array_equal(outs["segments"].view(np.float64), outs["launches"].view(np.float64))
    assert diff < 1e-13

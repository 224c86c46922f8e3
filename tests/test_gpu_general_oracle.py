"""-m gpu: the general path (XY mode, 3- / 4-level bases, general Lindblad) against the tight oracle at its kernel edges
(tests/golden/make_general_fixtures.py: d = 3 / 4 digit decode, the 4096-entry limit of the one-launch kernels, vector in
LDS or not, column-side Liouvillian terms, SLM switching terms, ryd_general_solve_many), and the CF4 step rule of
compute_bounds_general: the joint tightening of the static norms (general.py: _tighten_static_norms) lowers the Taylor
degree only, never the number of steps."""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_general_fixtures as G  # noqa: E402

BAR = 1e-7  # max-abs from the tight oracle: the bar of the 2-level pins
SINGLE = [name for name in G.CASES if not name.endswith("_batch")]


def _case(name):
    """Problems of case `name` rebuilt from the generator, after checking that the generator has not drifted."""
    fx = np.load(os.path.join(os.path.dirname(G.__file__), f"general_oracle_{name}.npz"))
    assert str(fx["input_sha256"]) == G.digest_case(name), f"{name}: generator drifted from the committed fixture"
    probs, mesolve, psi, times = G.build(name)
    np.testing.assert_array_equal(times, fx["times"])
    return probs, mesolve, psi, times, np.asarray(fx["states"])


def _paths(name):
    probs, mesolve, *_ = G.build(name)
    d, n = len(probs[0]["eigenbasis"]), probs[0]["n_qudits"]
    dim = d ** (2 * n if mesolve else n)
    return [(name, free, multi) for free in (True, False) for multi in (False, True) if free or dim <= 4096]


@pytest.mark.parametrize("name,matrix_free,multi", [p for name in SINGLE for p in _paths(name)],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_general_path_matches_tight_oracle(name, matrix_free, multi):
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general

    probs, mesolve, psi, times, ref = _case(name)
    tables = lower_general(probs[0], mesolve=mesolve, matrix_free=matrix_free)
    assert (tables.free is not None) == matrix_free
    with GeneralEngine(tables) as eng:
        eng.set_path(multi)
        t0 = time.time()
        out = eng.solve(eng.new_state(psi), times).cpu().numpy()[:, 0]
        secs = time.time() - t0
        st = eng.stats()
    err = [float(np.max(np.abs(out[k] - ref[0][k]))) for k in range(len(ref[0]))]
    print(f"\n{name} [{'free' if matrix_free else 'csr'}, {'multi' if multi else 'default'}] dim {tables.dim}: "
          f"max |hip - oracle| per time {', '.join(f'{e:.1e}' for e in err)}; {st['n_steps']} steps, "
          f"{secs * 1e3:.0f} ms")
    start = np.outer(psi, psi.conj()).ravel() if mesolve else psi
    assert np.max(np.abs(out[-1] - start)) > 1e-3  # (something happened)
    assert max(err) < BAR, err


def test_general_solve_many_matches_tight_oracle():
    """ryd_general_solve_many (one workgroup per problem) on three different XY 6-atom master equations."""
    from pulser_amd.engine import GeneralEngine
    from pulser_amd.general import lower_general

    probs, mesolve, psi, times, ref = _case("xy6_batch")
    engines = [GeneralEngine(lower_general(p, mesolve=mesolve)) for p in probs]
    try:
        states = [e.new_state(psi) for e in engines]
        t0 = time.time()
        outs = [o.cpu().numpy()[:, 0] for o in GeneralEngine.solve_many(engines, states, times)]
        secs = time.time() - t0
    finally:
        for e in engines:
            e.close()
    err = [float(np.max(np.abs(o - r))) for o, r in zip(outs, ref)]
    print(f"\nxy6_batch [solve_many]: max |hip - oracle| per problem {', '.join(f'{e:.1e}' for e in err)}; "
          f"{secs * 1e3:.0f} ms")
    assert max(err) < BAR, err


def _tightening_problems():
    from test_gpu_general_free import _problem_and_state

    # noises_all_0 (3-level, Ising diagonal + dephasing): the diagonal and the dissipator peak on the same rows, so the
    # joint bound equals the sum and nothing is tightened.  Relaxation on a weakly interacting triangle differs: the
    # diagonal's share drops by 6 %.  A constant drive on 250-ns knot intervals leaves the step rule of the general path as
    # the only limit on the steps (no spline curvature): ~45 CF4 steps per interval.
    ising, init = _problem_and_state("noises_all_0.npz")
    relax = G.ising_problem(np.array([[0.0, 0.0], [7.0, 0.0], [3.5, 6.06]]), 1001, 33,
                            collapse=[(np.sqrt(10.0), "sigma_gr")])
    relax["samples"]["Global"]["ground-rydberg"] = {"amp": np.full(1001, 4.0), "det": np.full(1001, -3.0),
                                                    "phase": np.full(1001, 0.5)}
    relax["sampling_rate"] = 0.005
    coords3 = np.array([[0.0, 0.0], [5.5, 0.0], [2.75, 4.8]])
    lvl3 = G.multilevel_problem(coords3, 101, 31, local=(1,), collapse=[(np.sqrt(2 * 0.7), "sigma_rr")])
    xy = G.xy_problem(np.array([[0.0, 0.0], [5.0, 0.0], [10.0, 0.0], [0.0, 5.0]]), 101, 32, dephasing=0.6)
    rng = np.random.default_rng(7)
    out = []
    for name, prob in (("noises_all_0", ising), ("ising_relaxation", relax), ("three_level_dephasing", lvl3),
                       ("xy_field", xy)):
        n, d = prob["n_qudits"], len(prob["eigenbasis"])
        psi = init if name == "noises_all_0" else rng.normal(size=d**n) + 1j * rng.normal(size=d**n)
        out.append((name, prob, psi / np.linalg.norm(psi)))
    return out


def test_static_norm_tightening_leaves_cf4_steps_alone(monkeypatch):
    """_tighten_static_norms scales the row norms of the time-independent terms (Ising diagonal, exchange pairs,
    dissipator) down to their joint bound.  That may lower the Taylor degree, but the CF4 steps must follow every term's
    OWN norm (compute_bounds_general: bd_step), the rule the general path was validated with: equal step counts with
    and without the tightening."""
    import pulser_amd.general as gen
    from pulser_amd.engine import GeneralEngine

    tightened = 0
    steps = {}
    for name, prob, psi in _tightening_problems():
        runs = {}
        for tight in (True, False):
            with monkeypatch.context() as m:
                if not tight:
                    m.setattr(gen, "_tighten_static_norms", lambda terms, dim: terms)
                tables = gen.lower_general(prob, mesolve=True, matrix_free=True)
            with GeneralEngine(tables) as eng:
                t_end = (int(prob["duration"]) - 1) * 1e-3
                eng.solve(eng.new_state(psi), [0.0, t_end])
                runs[tight] = (eng.stats(), float(tables.row_norm.sum()))
        (on, sum_on), (off, sum_off) = runs[True], runs[False]
        print(f"\n{name}: n_steps {on['n_steps']} tightened vs {off['n_steps']} not; norm_bound {on['norm_bound']:.4g} vs "
              f"{off['norm_bound']:.4g}; last_order {on['last_order']} vs {off['last_order']}")
        assert sum_on <= sum_off
        if on["norm_bound"] < 0.99 * off["norm_bound"]:
            tightened += 1
        steps[name] = (on["n_steps"], off["n_steps"])
    assert tightened >= 1  # the tightening took effect somewhere: the equalities below are not vacuous
    assert all(a == b for a, b in steps.values()), steps

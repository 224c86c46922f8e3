"""-m gpu: quantum-jump trajectories on the general path (``run(..., general_jumps=True)``): 3- / 4-level bases,
XY mode with its SLM mask, collapse operators whose sum C^dag C is not diagonal (``ryd_general_set_collapse``,
``ryd_general_mc_solve(_many)``, k_mc_general.hpp).

What is pinned, as for the 2-level kernels (tests/test_gpu_mcwf.py):

* the no-jump evolution under H_eff against the tight CPU integration of ``oracle.mcwf.effective_rhs``;
* every trajectory (number of jumps, kets at every evaluation time) against ``oracle.mcwf.mcwf_trajectory`` with
  the same Philox stream, on the persistent one-launch kernel and on the multi-launch kernels;
* trajectory averages against the master equation of the same emulator, Counters of noisy runs against MESOLVER;
* an XY register beyond the 2^26-entry Liouvillian, which only kets can hold.
"""
from __future__ import annotations

import os
import sys
from collections import Counter

import numpy as np
import pytest

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd import problem as P
from pulser_amd.engine import GeneralEngine
from pulser_amd.general import lower_general

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_general_fixtures as G  # noqa: E402

T = 201                                # samples: knots every ns over 0.2 us
OPTS = {"max_step": 5e-4}              # two CF4 steps per knot interval (more than the scheduler asks for here) ...
GRID = np.arange(2 * (T - 1) + 1) / 2000.0  # ... so that the oracle's step grid is the product's
EVAL = GRID[::50]                      # every 25 ns
NONDIAG = np.array([[1.0, 1.0], [0.0, 0.0]], dtype=complex)

def _smooth(prob):
    """The builders' drives with smooth waveforms (no phase jump, no ramp kinks), so that the CF4 steps stay one per
    knot interval and the oracle's step grid is the product's."""
    t = np.arange(prob["duration"]) / prob["duration"]
    k = 0
    for addr in ("Global", "Local"):
        for basis, s in prob["samples"][addr].items():
            entries = [s] if addr == "Global" else list(s.values())
            for e in entries:
                if not e:
                    continue
                k += 1
                e["amp"] = (6.0 + 2.0 * k) * np.sin(np.pi * t) ** 2
                e["det"] = (4.0 - k) * np.cos(2.0 * t + k)
                e["phase"] = 0.4 * k + 0.5 * t
    return prob


CASES = {
    # 3-level "all" basis, 5 atoms (243): relaxation r -> g, dephasing of r and h
    "all5": lambda: _smooth(G.multilevel_problem(P.register_coords(P.square_rect(1, 5), 6.5), T, 41, local=(1, 3),
                                         collapse=[(np.sqrt(3.0), "sigma_gr"), (np.sqrt(2 * 1.5), "sigma_rr"),
                                                   (np.sqrt(2 * 1.0), "sigma_hh")])),
    # 4-level leakage, 4 atoms (256): decay into x from r and g
    "leak4": lambda: _smooth(G.multilevel_problem(P.register_coords(P.square_rect(2, 2), 6.0), T, 42, leakage=True, local=(2,),
                                          collapse=[(np.sqrt(3.0), "sigma_xr"), (np.sqrt(2.0), "sigma_xg")])),
    # XY, 6 atoms (64) at 8 um, dephasing, SLM mask on atoms 0 and 4 until 80 ns
    "xy6_slm": lambda: _smooth(G.xy_problem(P.register_coords(P.square_rect(2, 3), 8.0), T, 43, slm_end=80, slm_targets=(0, 4),
                                    dephasing=2.0)),
    # the same register without the mask: the SLM switch is a step of a spline series, the curvature estimate
    # sub-steps the CF4 steps around it, and the trajectory test needs the oracle's step grid to be the product's
    "xy6": lambda: _smooth(G.xy_problem(P.register_coords(P.square_rect(2, 3), 8.0), T, 43, dephasing=2.0)),
    # 2-level Ising, 4 atoms, C = [[1, 1], [0, 0]]: sum C^dag C is not diagonal
    "nondiag4": lambda: _smooth(G.ising_problem(P.register_coords(P.square_rect(2, 2), 7.0), T, 44,
                                        collapse=[(np.sqrt(2.5), NONDIAG)])),
}


def _psi0(prob, seed):
    d, n = len(prob["eigenbasis"]), prob["n_qudits"]
    rng = np.random.default_rng(seed)
    psi = rng.normal(size=d**n) + 1j * rng.normal(size=d**n)
    if d == 4:  # nothing starts in the leakage state
        psi[((np.arange(d**n)[:, None] // d ** np.arange(n)) % d == 3).any(axis=1)] = 0.0
    return psi / np.linalg.norm(psi)


def _engine(prob, batch=1, matrix_free=None):
    tables, cops = lower_general(prob, mesolve=False, matrix_free=matrix_free, with_collapse=True)
    eng = GeneralEngine(tables, batch=batch)
    eng.set_collapse(cops)
    return eng


@pytest.mark.parametrize("name", ["all5", "xy6_slm", "nondiag4"])
@pytest.mark.parametrize("multi", [False, True])
def test_no_jump_evolution_under_h_eff(name, multi):
    from oracle import mcwf, qutip_path as qp

    prob = CASES[name]()
    ham = qp.build_hamiltonian(prob)
    psi0 = _psi0(prob, 1)
    ref = qp._zvode(mcwf.effective_rhs(ham), psi0, EVAL, qp.TIGHT)
    for free in (False, True):
        with _engine(prob, matrix_free=free) as eng:
            eng.set_path(multi)
            got = eng.solve(eng.new_state(psi0), EVAL, **OPTS).cpu().numpy()
        err = max(float(np.max(np.abs(got[i - 1][0] - ref[i]))) for i in range(1, len(EVAL)))
        print(f"{name} multi={multi} matrix_free={free}: max |hip - oracle| = {err:.2e}")
        assert err < 1e-8, err
    assert np.vdot(ref[-1], ref[-1]).real < 0.8  # the norm visibly decays


SEEDS = np.array([1, 2**40 + 17, 123456789012345, 2**64 - 1, 99, 4242] + list(range(1000, 1010)), dtype=np.uint64)


@pytest.mark.parametrize("name", ["all5", "leak4", "xy6", "nondiag4"])
def test_trajectories_match_cpu_restatement(name):
    """16 trajectories: ryd_general_mc_solve_many (persistent kernel, one workgroup per engine), one batched engine
    on the multi-launch kernels, and the CPU restatement with the same seeds and the same step grid."""
    from oracle import mcwf, qutip_path as qp

    prob = CASES[name]()
    ham = qp.build_hamiltonian(prob)
    psi0 = _psi0(prob, 2)
    engines = [_engine(prob) for _ in SEEDS]
    try:
        states = [e.new_state(psi0) for e in engines]
        many = np.stack([s.cpu().numpy()[:, 0] for s in GeneralEngine.mc_solve_many(engines, states, EVAL, SEEDS, **OPTS)],
                        axis=1)
        many_final = np.stack([s.cpu().numpy()[0] for s in states])
        many_counts = np.concatenate([e.mc_jumps() for e in engines])
        assert engines[0].stats()["n_steps"] == len(GRID) - 1
        assert engines[0].stats()["n_launches"] == 1
    finally:
        for e in engines:
            e.close()
    with _engine(prob, batch=len(SEEDS)) as eng:
        eng.set_path(True)
        st = eng.new_state(psi0)
        multi = eng.mc_solve(st, EVAL, SEEDS, **OPTS).cpu().numpy()
        multi_final = st.cpu().numpy()
        multi_counts = eng.mc_jumps()
        assert eng.stats()["n_steps"] == len(GRID) - 1 and eng.stats()["n_launches"] > 4 * (len(GRID) - 1)
    np.testing.assert_array_equal(many_counts, multi_counts)
    assert np.max(np.abs(many - multi)) < 1e-10
    assert np.max(np.abs(many_final - multi_final)) < 1e-10
    total = 0
    for b, seed in enumerate(SEEDS):
        ref, jumps = mcwf.mcwf_trajectory(ham, psi0, GRID, EVAL, int(seed))
        assert many_counts[b] == len(jumps), (b, jumps)
        total += len(jumps)
        for i in range(1, len(EVAL)):
            assert np.max(np.abs(many[i - 1][b] - ref[i])) < 1e-7, (b, i, jumps)
        assert np.max(np.abs(many_final[b] - ref[-1])) < 1e-7
        assert abs(np.linalg.norm(many_final[b]) - 1) < 1e-12
    assert total >= len(SEEDS)  # jumps, not only decay
    print(f"{name}: {total} jumps over {len(SEEDS)} trajectories")


def test_batched_persistent_kernel_matches_multi_launch():
    """ryd_general_mc_solve on the persistent kernel with a batch (one workgroup per trajectory) and on the
    multi-launch kernels: same jumps, same kets; an evaluation time repeated and one between two knots."""
    prob = CASES["nondiag4"]()
    times = np.array([0.0, 0.05, 0.05, 0.1234, 0.2])
    seeds = np.arange(5, 5 + 40, dtype=np.uint64) * np.uint64(2654435761)
    out = []
    for multi in (False, True):
        with _engine(prob, batch=len(seeds)) as eng:
            eng.set_path(multi)
            st = eng.new_state(_psi0(prob, 3))
            snaps = eng.mc_solve(st, times, seeds).cpu().numpy()
            out.append((snaps, eng.mc_jumps(), eng.stats()["n_launches"]))
    assert out[0][2] <= 4 and out[1][2] > 100
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert out[0][1].sum() > 0
    assert np.max(np.abs(out[0][0] - out[1][0])) < 1e-10
    assert np.allclose(np.linalg.norm(out[0][0], axis=-1), 1.0, atol=1e-12)


def _xy_inputs(rows, cols, spacing, dur, amp):
    """A global microwave pulse amp sin^2(pi t / dur) on a rows x cols XY register (C3 = 3700, field along z)."""
    from pulser_amd.hamiltonian_data import ChannelInput, SequenceInputs, Slot

    n = rows * cols
    coords = P.register_coords(P.square_rect(rows, cols), spacing)
    t = np.arange(dur)
    ch = ChannelInput("mw", "Global", "XY", amp * np.sin(np.pi * t / dur) ** 2, np.full(dur, -2.0), np.zeros(dur),
                      [Slot(0, dur, tuple(range(n)))])
    return SequenceInputs(coords, tuple(f"q{i}" for i in range(n)), [ch], 5420158.53,
                          interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))


def _xy4_inputs():
    return _xy_inputs(2, 2, 8.0, 500, 8.0)


def _all3_inputs():
    from helpers import load_fixture
    from test_host_logic import _inputs_from_problem

    prob, extra = load_fixture("noises_all_0.npz")
    meas = extra["aux"]["meas_basis"]
    return _inputs_from_problem(prob, measurement=meas if meas != "digital" else None)


@pytest.mark.parametrize("which", ["xy4", "all3"])
def test_mcsolver_average_matches_the_master_equation(which):
    inputs, nm, rate = ((_xy4_inputs(), NoiseModel(dephasing_rate=3.0), 0.1) if which == "xy4" else
                        (_all3_inputs(), NoiseModel(relaxation_rate=1.0, dephasing_rate=0.5,
                                                    hyperfine_dephasing_rate=0.3), 0.01))
    ref = QutipEmulator(inputs, sampling_rate=rate, noise_model=nm, evaluation_times="Minimal")
    with pytest.warns(DeprecationWarning):
        exact = np.asarray(ref.run().states[-1])
    ntraj = 2000
    emu = QutipEmulator(inputs, sampling_rate=rate, noise_model=nm, solver=Solver.MCSOLVER, n_trajectories=ntraj,
                        evaluation_times="Minimal")
    assert not emu._mc_fast_ok(emu._current_problem)
    with pytest.warns(DeprecationWarning):
        res = emu.run(seeds=3, general_jumps=True)
    got = np.asarray(res.states[-1])
    assert got.shape == exact.shape and len(emu.last_mc_jumps) == ntraj
    assert emu.last_mc_jumps.sum() > ntraj // 20
    assert abs(np.trace(got).real - 1) < 1e-12 and np.allclose(got, got.conj().T, atol=1e-14)
    err = float(np.max(np.abs(got - exact)))
    print(f"{which}: max |<rho>_traj - rho_me| = {err:.3e} (5 sigma = {5 * 0.5 / np.sqrt(ntraj):.3e})")
    assert err < 5 * 0.5 / np.sqrt(ntraj)
    assert np.max(np.abs(got - exact)) > 0.0


def _tv(c1, c2):
    keys = set(c1) | set(c2)
    n1, n2 = sum(c1.values()), sum(c2.values())
    return 0.5 * sum(abs(c1.get(k, 0) / n1 - c2.get(k, 0) / n2) for k in keys)


def test_noisy_default_run_matches_mesolver_and_is_reproducible():
    inputs = _xy4_inputs()
    nm = NoiseModel(dephasing_rate=3.0, state_prep_error=0.1, samples_per_run=4)
    counts = {}
    for solver, kw in ((Solver.DEFAULT, {"general_jumps": True}), (Solver.MESOLVER, {})):
        np.random.seed(7)
        emu = QutipEmulator(inputs, sampling_rate=0.1, noise_model=nm, n_trajectories=600, solver=solver,
                            evaluation_times="Minimal")
        with pytest.warns(DeprecationWarning):
            res = emu.run(seeds=5, **kw)
        counts[solver] = Counter(res[-1].bitstring_counts)
        if solver == Solver.DEFAULT:
            assert emu.last_mc_jumps.sum() > 0
            np.random.seed(7)
            emu2 = QutipEmulator(inputs, sampling_rate=0.1, noise_model=nm, n_trajectories=600,
                                 evaluation_times="Minimal")
            with pytest.warns(DeprecationWarning):
                assert Counter(emu2.run(seeds=5, general_jumps=True)[-1].bitstring_counts) == counts[solver]
    tv = _tv(counts[Solver.DEFAULT], counts[Solver.MESOLVER])
    print(f"TV(general jumps, mesolve) = {tv:.3f}")
    assert tv < 0.1


def test_xy_register_beyond_the_liouvillian_cap():
    """14 XY atoms: the Liouvillian would need 4^14 = 2^28 entries (ryd_general_create refuses it); jump
    trajectories evolve kets of 2^14."""
    n = 14
    inputs = _xy_inputs(2, 7, 9.0, 120, 30.0)
    nm = NoiseModel(dephasing_rate=6.0, state_prep_error=0.05)
    emu = QutipEmulator(inputs, noise_model=nm, solver=Solver.MCSOLVER, n_trajectories=3, evaluation_times="Minimal")
    assert emu._solver_mode(emu._current_problem) == "mcsolve"
    opts = {"general_jumps": True}
    emu._validate_options(opts)
    finals, jumps, reps = [], [], 0
    for res, r in emu._noisy_runs(**opts):  # (equal noise trajectories come as one with reps > 1)
        finals.append(np.asarray(res.states[-1]).reshape(-1))
        jumps.append(emu.last_mc_jumps.copy())
        reps += r
    assert reps == 3 and all(f.shape == (2**n,) for f in finals)
    assert all(abs(np.linalg.norm(f) - 1) < 1e-12 for f in finals)
    assert np.concatenate(jumps).sum() > 0
    with pytest.warns(DeprecationWarning):
        res = emu.run(general_jumps=True)
    assert sum(res[-1].bitstring_counts.values()) == 3 * nm.samples_per_run

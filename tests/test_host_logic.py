"""CPU tests of the host-side logic (no GPU, no pulser needed).

* the oracle against the reference's golden vectors (known answers);
* the product's restated HamiltonianData / results / sampling against fixtures
  captured from the real pulser-core (tests/golden/make_fixtures.py) and
  against the reference's seeded golden Counters, with the solver call replaced
  by the fixture's stored states (the HIP solver itself is covered by -m gpu);
* the C-ABI library loads and exports every symbol include/rydemu.h declares.
"""
import os
import re
from collections import Counter

import numpy as np
import pytest

from helpers import GOLDEN, load_fixture, with_anneal_samples

import pulser_amd
from pulser_amd import problem as P
from pulser_amd.hamiltonian_data import (ChannelInput, HamiltonianData,
                                         SequenceInputs, Slot, single_global_channel)
from pulser_amd.noise_model import NoiseModel, LEGACY_DEFAULTS
from pulser_amd.results import (CoherentResults, QState, StateResult, multinomial,
                                spam_flips)
from pulser_amd.simulation import QutipEmulator, SimConfig, Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------- oracle
@pytest.mark.parametrize("k", range(7))
def test_oracle_reproduces_reference_golden_counters_rydberg(k):
    """tests/pulser_simulation/test_simulation.py:978-1040 (seed 123)."""
    from oracle import qutip_path as qp, sampling as osamp

    prob, extra = load_fixture(f"noises_rydberg_{k}.npz")
    aux = extra["aux"]
    ham = qp.build_hamiltonian(prob)
    assert len(ham.collapse) == extra["n_collapse_ops"] * prob["n_qudits"]
    psi0 = qp.all_ground_state(prob["n_qudits"], prob["eigenbasis"])
    states = qp.mesolve(ham, psi0, aux["eval_times"], **aux["options"])
    assert np.max(np.abs(states[-1] - extra["oracle_final_state_default"])) < 1e-12
    # replay the RNG: constructor draws (first + hidden noiseless HamiltonianData)
    np.random.seed(123)
    n = prob["n_qudits"]
    ntraj = LEGACY_DEFAULTS["runs"] if False else 1
    np.random.uniform(size=n * ntraj)
    np.random.uniform(size=n)
    c = osamp.sample_state(states, aux["eval_times"], aux["eval_times"][-1], 1000, n,
                           prob["eigenbasis"], aux["meas_basis"], aux["matching_meas_basis"])
    assert dict(c) == extra["reference_golden_counter"]
    rho = states[-1]
    tr2 = np.trace(rho @ rho).real
    assert tr2 < 1 and not np.isclose(tr2, 1)  # test_simulation.py:1033-1034


def test_oracle_three_atom_state_and_lookup_quirk():
    """test_simulation.py:2156-2190 + SURVEY F5 (penultimate sample lookup)."""
    prob, extra = load_fixture("three_atom_state.npz")
    idx = int(extra["oracle_lookup_index"])
    assert idx == 3999  # first index within 1e-3 of 4.0 us, not the last one
    st = np.asarray(extra["oracle_states_default"])[2]
    st = st * np.exp(-1j * np.angle(st[np.argmax(np.abs(st))]))
    assert np.all(np.isclose(st, extra["reference_golden_state"], 1e-2))


def test_oracle_liouvillian_matches_matrix_free_rhs():
    from oracle import qutip_path as qp
    from helpers import DEPOL_PAULIS, local_problem

    ops = [(np.sqrt(0.1), "sigma_rr"), (np.sqrt(0.07), "sigma_gr")] + [(np.sqrt(0.0125), p) for p in "xyz"]
    prob = local_problem(2, seed=2, collapse_ops=ops, paulis=DEPOL_PAULIS)
    ham = qp.build_hamiltonian(prob)
    rng = np.random.default_rng(0)
    rho = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    L = qp.liouvillian(ham, 0.123)
    ref = (L @ rho.ravel(order="F")).reshape(4, 4, order="F")  # column stacking
    got = qp.lindblad_rhs(ham)(0.123, rho.ravel()).reshape(4, 4)
    assert np.max(np.abs(ref - got)) < 1e-12


# ----------------------------------------------------------- synthetic inputs
def test_synthetic_generators_match_pulser_fixtures():
    prob, extra = load_fixture("cfg1_square4_pi.npz")
    coords = P.register_coords(P.square_rect(2, 2), 5.0)
    assert np.array_equal(coords, prob["coords"])
    amp = np.concatenate([P.blackman_samples(1000, np.pi), [0.0]])
    assert np.array_equal(amp, prob["samples"]["Global"]["ground-rydberg"]["amp"])
    assert np.array_equal(P.interaction_matrix(coords, P.C6_LEVEL70), prob["interaction_matrix"])
    prob, extra = load_fixture("cfg2_chain12_anneal.npz")
    rb = float(extra["blockade_radius"])
    assert abs(rb - 8.692) < 1e-3
    assert np.allclose(P.register_coords(P.square_rect(1, 12), rb), prob["coords"], atol=1e-12)
    s = P.anneal_samples()
    assert len(s["amp"]) == 3101 and s["amp"][-1] == 0.0 and s["det"][-1] == 0.0
    prob, extra = load_fixture("cfg3_tri6_dephasing.npz")
    assert np.allclose(P.register_coords(P.triangular_rect(2, 3), float(extra["blockade_radius"])),
                       prob["coords"], atol=1e-12)


def test_problem_roundtrip(tmp_path):
    from helpers import DEPOL_PAULIS, local_problem

    prob = local_problem(3, collapse_ops=[(0.1, "x"), (0.2 + 0.1j, np.eye(2))], paulis=DEPOL_PAULIS)
    path = str(tmp_path / "p.npz")
    P.save_problem(path, prob, note="x", arr=np.arange(3))
    back, extra = P.load_problem(path)
    assert back["qubit_ids"] == prob["qubit_ids"] and extra["note"] == "x"
    assert np.array_equal(back["samples"]["Local"]["ground-rydberg"][2]["amp"],
                          prob["samples"]["Local"]["ground-rydberg"][2]["amp"])
    assert back["collapse_ops"][1][0] == 0.2 + 0.1j


# ------------------------------------------------- restated HamiltonianData
def _chain12_inputs(extra):
    coords = P.register_coords(P.square_rect(1, 12), float(extra["blockade_radius"]))
    s = P.anneal_samples()
    un = {k: v[:-1] for k, v in s.items()}  # un-extended, as the sampler hands it over
    return single_global_channel(coords, un, P.C6_LEVEL70, extended=False)


def test_noise_trajectories_follow_reference_rng_order():
    """cfg4: doppler + amplitude + SPAM, seed 0, 1024 trajectories - every draw
    must equal what pulser-core's HamiltonianData drew (fixture)."""
    prob0, extra = load_fixture("cfg4_chain12_noise.npz")
    nm = NoiseModel(**extra["noise_model"])
    assert set(nm.noise_types) == {"SPAM", "amplitude", "doppler"}
    inputs = _chain12_inputs(extra).extend_duration(3101)
    np.random.seed(0)
    hd = HamiltonianData(inputs, nm, int(extra["n_trajectories"]))
    assert np.array_equal(np.random.get_state()[1][:4], extra["rng_probe_after_ctor"])
    trajs = hd.noise_trajectories
    assert len(trajs) == 1024
    assert np.array_equal(np.array([t.bad_atoms for t in trajs]), extra["traj_bad_atoms"])
    assert np.array_equal(np.array([t.doppler_detune for t in trajs]), extra["traj_doppler"])
    assert np.array_equal(np.array([t.amp_fluctuations["ising_global"] for t in trajs]),
                          extra["traj_amp_fluctuation"])
    p = hd.problem(trajs[0], 1.0)
    for q in range(12):
        for key in ("amp", "det", "phase"):
            assert np.array_equal(p["samples"]["Local"]["ground-rydberg"][q][key],
                                  prob0["samples"]["Local"]["ground-rydberg"][q][key]), (q, key)
    assert np.array_equal(p["interaction_matrix"], prob0["interaction_matrix"])
    for i in range(3):
        pi = hd.problem(trajs[i], 1.0)
        det = np.stack([pi["samples"]["Local"]["ground-rydberg"][q]["det"] for q in range(12)])
        amp = np.stack([pi["samples"]["Local"]["ground-rydberg"][q]["amp"] for q in range(12)])
        assert np.array_equal(det[:, ::100], extra["kept_det"][i])
        assert np.array_equal(amp[:, ::100], extra["kept_amp"][i])
        assert np.array_equal(pi["interaction_matrix"], extra["kept_interaction"][i])


def test_spam_only_trajectories_are_deduplicated():
    """hamiltonian_data.py:795-835: Counter(...).most_common() -> (config, reps)."""
    _, extra = load_fixture("cfg4_chain12_noise.npz")
    inputs = _chain12_inputs(extra).extend_duration(3101)
    np.random.seed(0)
    hd = HamiltonianData(inputs, NoiseModel(state_prep_error=0.005, dephasing_rate=0.05), 1024)
    reps = [t.reps for t in hd.noise_trajectories]
    assert sum(reps) == 1024 and reps == sorted(reps, reverse=True)
    assert not hd.noise_trajectories[0].bad_atoms.any()
    assert hd.local_noises and hd.collapse_ops()[0] == [(np.sqrt(0.1), "sigma_rr")]


# ---------------------------------- emulator front-end with the solver stubbed
class _FakeSolve:
    """Stands in for the HIP solver call: returns the fixture's stored state at
    every evaluation time (only the looked-up one matters for sampling)."""

    def __init__(self, emu, state):
        self.emu, self.state = emu, state

    def __call__(self, problems, progress_bar, options, tables=None, mc_ntraj=None):
        emu = self.emu
        qids = tuple(emu.samples_obj.qubit_ids)
        me = ({"epsilon": emu.noise_model.p_false_pos, "epsilon_prime": emu.noise_model.p_false_neg}
              if "SPAM" in emu.noise_model.noise_types else None)
        res = [StateResult(qids, emu._meas_basis, QState(self.state),
                           emu._meas_basis in emu.basis_name)
               for _ in emu._eval_times_array]
        return [CoherentResults(res, len(qids), emu.basis_name, emu._eval_times_array,
                                emu._meas_basis, me) for _ in problems]


def _inputs_from_problem(prob, basis=None, c6=P.C6_LEVEL70, measurement=None):
    """SequenceInputs equivalent to a captured (noiseless-sample) problem: one
    Global channel per global basis entry, one Local channel per (basis, atom)."""
    n = prob["n_qudits"]
    chans = []
    for b, s in prob["samples"]["Global"].items():
        if basis is not None and b != basis:
            continue
        T = len(s["amp"]) - 1
        chans.append(ChannelInput(f"g_{b}", "Global", b, s["amp"][:-1], s["det"][:-1],
                                  s["phase"][:-1], [Slot(0, T, tuple(range(n)))]))
    for b, per_q in prob["samples"]["Local"].items():
        if basis is not None and b != basis:
            continue
        for q, s in per_q.items():
            T = len(s["amp"]) - 1
            chans.append(ChannelInput(f"l_{b}_{q}", "Local", b, s["amp"][:-1], s["det"][:-1],
                                      s["phase"][:-1], [Slot(0, T, (int(q),))]))
    return SequenceInputs(prob["coords"], prob["qubit_ids"], chans, c6, measurement=measurement)


def _all_basis_emulator(k):
    """Emulator for case k of test_simulation.py:1179-1300 ("all" basis)."""
    prob, extra = load_fixture(f"noises_all_{k}.npz")
    noise = tuple(extra["noise"])
    leak = "leakage" in noise
    dd = 4 if leak else 3
    params = {}
    if "relaxation" in noise:
        params["relaxation_rate"] = 1.0
    if "dephasing" in noise:
        params.update(hyperfine_dephasing_rate=0.1, dephasing_rate=0.1)
    if leak or "eff_noise" in noise:
        a = np.zeros((dd, dd), dtype=complex); a[0, 0] = 1
        b = np.zeros((dd, dd), dtype=complex); b[2, 2] = 1
        params.update(eff_noise_opers=[a, b], eff_noise_rates=[0.2, 0.2])
    meas = extra["aux"]["meas_basis"]
    emu = QutipEmulator(
        _inputs_from_problem(prob, measurement=meas if meas != "digital" else None),
        sampling_rate=0.01, noise_model=NoiseModel(with_leakage=leak, **params))
    return emu, prob, extra


@pytest.mark.parametrize("k", range(6))
def test_emulator_golden_counters_all_basis(k, monkeypatch):
    """test_simulation.py:1179-1300 (3 atoms, digital + rydberg channels, d = 3/4)."""
    emu, prob, extra = _all_basis_emulator(k)
    assert set(emu.noise_model.noise_types) == set(extra["noise"])
    assert emu.basis_name == prob["basis_name"] and emu._meas_basis == extra["aux"]["meas_basis"]
    p = emu._current_problem
    assert p["eigenbasis"] == list(prob["eigenbasis"])
    assert len(p["collapse_ops"]) == extra["n_collapse_ops"]
    assert np.array_equal(emu.evaluation_times, extra["aux"]["eval_times"])
    monkeypatch.setattr(emu, "_solve_batch", _FakeSolve(emu, extra["oracle_lookup_state_default"]))
    np.random.seed(123)  # the reference seeds right before run()
    with pytest.warns(DeprecationWarning):
        res = emu.run()
    assert res.sample_final_state() == Counter(extra["reference_golden_counter"])
    with pytest.raises(NotImplementedError, match="Cannot include depolarizing noise in all-basis."):
        QutipEmulator(_inputs_from_problem(prob), noise_model=NoiseModel(depolarizing_rate=1.0))
    with pytest.raises(ValueError, match="Incompatible shape for effective noise operator n°0."):
        QutipEmulator(_inputs_from_problem(prob), noise_model=NoiseModel(
            eff_noise_opers=[np.diag([1.0, -1.0])], eff_noise_rates=[1.0]))


@pytest.mark.parametrize("k", range(7))
def test_emulator_golden_counters_rydberg(k, monkeypatch):
    """test_simulation.py:978-1040 through the product's front-end: NoiseModel
    -> collapse specs, RNG order (constructor draws), weights, multinomial."""
    prob, extra = load_fixture(f"noises_rydberg_{k}.npz")
    noise = tuple(extra["noise"])
    params = {}
    if "dephasing" in noise:
        params.update(dephasing_rate=0.05, hyperfine_dephasing_rate=1e-3)
    if "relaxation" in noise:
        params.update(relaxation_rate=0.01)
    if "depolarizing" in noise:
        params.update(depolarizing_rate=0.05)
    leak = "leakage" in noise
    if leak or "eff_noise" in noise:
        params["eff_noise_opers"] = [np.diag([1.0, 0, 0]).astype(complex) if leak
                                     else np.diag([1.0, -1.0]).astype(complex)]
        params["eff_noise_rates"] = [0.1 if leak else 0.025]
    np.random.seed(123)
    emu = QutipEmulator(_inputs_from_problem(prob, "ground-rydberg"), sampling_rate=0.01,
                        noise_model=NoiseModel(with_leakage=leak, **params))
    assert set(emu.noise_model.noise_types) == set(noise)
    p = emu._current_problem
    assert p["basis_name"] == prob["basis_name"] and p["eigenbasis"] == list(prob["eigenbasis"])
    assert len(p["collapse_ops"]) == extra["n_collapse_ops"]
    for (c1, o1), (c2, o2) in zip(p["collapse_ops"], prob["collapse_ops"]):
        assert np.isclose(c1, c2) and (o1 == o2 if isinstance(o1, str) else np.array_equal(o1, o2))
    assert np.array_equal(emu.evaluation_times, extra["aux"]["eval_times"])
    opts = {}
    emu._validate_options(opts)
    assert opts["max_step"] == extra["aux"]["options"]["max_step"]
    assert opts["nsteps"] == extra["aux"]["options"]["nsteps"]
    monkeypatch.setattr(emu, "_solve_batch", _FakeSolve(emu, extra["oracle_lookup_state_default"]))
    with pytest.warns(DeprecationWarning, match="QutipEmulator is deprecated as of pulser 1.9"):
        res = emu.run()
    assert res.sample_final_state() == Counter(extra["reference_golden_counter"])


@pytest.mark.parametrize("k", range(7))
def test_emulator_golden_counters_digital(k, monkeypatch):
    """test_simulation.py:1079-1160 (3 atoms, digital basis, d = 2 or 3)."""
    prob, extra = load_fixture(f"noises_digital_{k}.npz")
    noise = tuple(extra["noise"])
    params = {}
    if "dephasing" in noise:
        params.update(dephasing_rate=0.05, hyperfine_dephasing_rate=0.05)
    if "depolarizing" in noise:
        params.update(depolarizing_rate=0.05)
    leak = "leakage" in noise
    if leak or "eff_noise" in noise:
        params["eff_noise_opers"] = [np.diag([0, 1.0, 0]).astype(complex) if leak
                                     else np.diag([1.0, -1.0]).astype(complex)]
        params["eff_noise_rates"] = [0.1 if leak else 0.025]
    np.random.seed(123)
    emu = QutipEmulator(_inputs_from_problem(prob, "digital"), sampling_rate=0.01,
                        noise_model=NoiseModel(with_leakage=leak, **params))
    assert emu.basis_name == prob["basis_name"] and emu._meas_basis == "digital"
    assert emu._current_problem["eigenbasis"] == list(prob["eigenbasis"])
    monkeypatch.setattr(emu, "_solve_batch", _FakeSolve(emu, extra["oracle_lookup_state_default"]))
    with pytest.warns(DeprecationWarning):
        res = emu.run()
    assert res.sample_final_state() == Counter(extra["reference_golden_counter"])


def test_emulator_validation_messages_and_defaults():
    _, extra = load_fixture("cfg4_chain12_noise.npz")
    inputs = _chain12_inputs(extra)
    with pytest.raises(ValueError, match="must be greater than 0 and less than or equal to 1"):
        QutipEmulator(inputs, sampling_rate=0.0)
    with pytest.raises(ValueError, match="`sampling_rate` is too small, less than 4 data points."):
        QutipEmulator(inputs, sampling_rate=0.001)
    with pytest.raises(ValueError, match="'n_trajectories' must be defined"):
        QutipEmulator(inputs, noise_model=NoiseModel(temperature=50.0))
    with pytest.raises(TypeError, match="valid SequenceSamples instance"):
        QutipEmulator("nope")
    emu = QutipEmulator(inputs, evaluation_times="Minimal")
    assert np.array_equal(emu.evaluation_times, [0.0, 3.1])
    assert emu.total_duration_ns == 3100 and emu.dim == 2 and emu.basis_name == "ground-rydberg"
    assert len(emu.sampling_times) == 3101
    emu.set_evaluation_times(0.5)
    assert len(emu.evaluation_times) == 1550  # int(0.5 * 3101) knots, ends included
    with pytest.raises(ValueError, match="extends further than sequence duration"):
        emu.set_evaluation_times([0.0, 5.0])
    with pytest.raises(ValueError, match="Wrong evaluation time label"):
        emu.set_evaluation_times("Best")
    with pytest.raises(ValueError, match="Incompatible shape of initial state.Expected 4096, got 3"):
        emu.set_initial_state(np.ones(3))
    assert np.asarray(emu.initial_state)[-1, 0] == 1.0
    # a density matrix is no initial state: the reference wraps the input in ket dimensions (simulation.py:519-529:
    # qutip.Qobj(state, dims=[[d] * N, [1] * N])), which qutip refuses for a D x D array; a column vector is a ket
    with pytest.raises(ValueError, match="the initial state is a ket"):
        emu.set_initial_state(np.eye(4096))
    col = np.zeros((4096, 1)); col[5, 0] = 2.0
    emu.set_initial_state(col)
    assert np.asarray(emu.initial_state)[5, 0] == 1.0
    emu.set_initial_state("all-ground")
    opts = {}
    emu._validate_options(opts)
    assert opts == {"max_step": 0.001, "nsteps": 3100 // 0.001}  # = 3099999.0, as simulation.py:778-780 computes it
    # solver selection of simulation.py:705-718
    noisy = QutipEmulator(inputs, noise_model=NoiseModel(temperature=50.0, dephasing_rate=0.1),
                          n_trajectories=2)
    assert noisy._solver_mode({"collapse_ops": [1]}) == "mcsolve"
    assert noisy._solver_mode({"collapse_ops": []}) == "sesolve"
    assert noisy._mc_fast_ok(noisy._current_problem)
    deph = QutipEmulator(inputs, noise_model=NoiseModel(dephasing_rate=0.1))
    assert deph._solver_mode({"collapse_ops": [1]}) == "mesolve"
    from pulser_amd.simulation import Solver
    assert QutipEmulator(inputs, noise_model=NoiseModel(dephasing_rate=0.1), solver=Solver.MCSOLVER,
                         n_trajectories=3)._solver_mode({"collapse_ops": [1]}) == "mcsolve"
    sd = noisy._mc_seeds(4, {"seeds": 7})
    noisy._mc_rng = None
    assert sd.dtype == np.uint64 and np.array_equal(sd, noisy._mc_seeds(4, {"seeds": 7}))
    op = emu.build_operator([("sigma_rr", ["q0", "q11"])])
    assert op.shape == (4096, 4096) and op[0, 0] == 1 and op[1, 1] == 0
    with pytest.raises(ValueError, match="Duplicate atom ids"):
        emu.build_operator([("sigma_rr", ["q0", "q0"])])


def test_simconfig_noise_model_roundtrip():
    with pytest.warns(DeprecationWarning, match="'SimConfig' has been deprecated"):
        cfg = SimConfig(noise=("SPAM", "doppler", "dephasing"), eta=0.02, temperature=30.0, runs=7)
    nm = cfg.to_noise_model()
    assert set(nm.noise_types) == {"SPAM", "doppler", "dephasing"}
    assert nm.state_prep_error == 0.02 and abs(nm.temperature - 30.0) < 1e-9 and nm.runs == 7
    with pytest.warns(DeprecationWarning):
        back = SimConfig.from_noise_model(nm)
    assert set(back.noise) == set(nm.noise_types) and back.eta == 0.02


# ------------------------------------------------------------ results/sampling
def test_weights_multinomial_and_flips_match_oracle():
    from oracle import sampling as osamp

    rng = np.random.default_rng(3)
    n = 5
    psi = rng.normal(size=32) + 1j * rng.normal(size=32)
    psi /= np.linalg.norm(psi)
    res = StateResult(tuple(range(n)), "ground-rydberg", QState(psi), True)
    w = res._weights()
    assert np.array_equal(w, osamp.weights(psi, n, ["r", "g"], "ground-rydberg"))
    assert np.array_equal(w, (np.abs(psi) ** 2)[::-1] / sum((np.abs(psi) ** 2)[::-1]))
    np.random.seed(5)
    a = res.get_samples(500)
    np.random.seed(5)
    b = osamp.get_samples(w, 500, n)
    assert a == b and list(a) == list(b)  # same insertion order
    np.random.seed(9)
    fa = spam_flips(a, 0.01, 0.05)
    np.random.seed(9)
    fb = osamp.spam_flips(b, 0.01, 0.05)
    assert fa == fb
    rho = np.outer(psi, psi.conj())
    assert np.allclose(StateResult(tuple(range(n)), "ground-rydberg", QState(rho), True)._weights(), w)
    # reference's own multinomial test (tests/math/test_multinomial.py:19-37)
    np.random.seed(1337)
    probs = np.array([0.2, 0.5, 0.3])
    idx = multinomial(10000, probs)
    assert np.allclose(np.bincount(idx) / 10000, probs, atol=0.02)


def test_cfg3_counters_with_spam_flips():
    """Product sampling (weights + multinomial + flips) against the oracle's
    Counters for the cfg3 physics at N = 6 (seed 123)."""
    prob, extra = load_fixture("cfg3_tri6_dephasing.npz")
    states = np.asarray(extra["oracle_states_default"])
    times = np.asarray(extra["eval_times"])
    qids = tuple(prob["qubit_ids"])
    res = [StateResult(qids, "ground-rydberg", QState(s), True) for s in states]
    cr = CoherentResults(res, 6, "ground-rydberg", times, "ground-rydberg",
                         dict(extra["meas_errors"]))
    assert cr._get_index_from_time(3.1) == 4  # first match: the 3.099 us sample
    np.random.seed(123)
    c = cr.sample_state(3.099, 1000)
    assert c == Counter(extra["oracle_counter_t3099_spam"])
    dens = cr._calc_pseudo_density(5)
    assert abs(np.trace(np.asarray(dens)) - 1) < 1e-12
    nk = np.diag(1.0 - ((np.arange(64) >> 5) & 1)).astype(complex)
    e = cr.expect([nk])[0]
    assert e.shape == (6,) and 0 <= e[-1] <= 1


# ------------------------------------------------------------------ lowering
def test_lowering_matches_oracle_terms():
    from oracle import qutip_path as qp
    from pulser_amd.terms import lower

    prob, _ = load_fixture("cfg2_chain12_anneal.npz")
    prob = with_anneal_samples(prob)
    t = lower([prob])
    ham = qp.build_hamiltonian(prob)
    assert np.array_equal(t.tknots, ham.tlist) and t.pp.shape == (2, 3100, 4)
    labels = [x.label for x in ham.terms]
    assert labels == ["int", "G:ground-rydberg:sigma_gr", "G:ground-rydberg:sigma_rr"]
    d = t.desc[0, 0]
    for tt in (0.0, 0.4999, 0.5003, 1.7, 3.0999):
        i = min(int(np.searchsorted(t.tknots, tt, side="right")) - 1, 3099)
        u = tt - t.tknots[i]
        val = lambda s: np.polyval(t.pp[s, i], u)  # noqa: E731
        c_or = ham.splines[0](tt)
        det_or = -2 * ham.splines[1](tt).real
        assert abs(val(d["drive_series"]) - c_or) < 1e-12
        assert abs(val(d["det_series"]).real - det_or) < 1e-11
    assert np.array_equal(t.interaction[0], prob["interaction_matrix"][0])
    with pytest.raises(NotImplementedError, match="not supported by the MI355X backend"):
        lower([load_fixture("noises_digital_5.npz")[0]])


# ------------------------------------------------------------------ C ABI
def _header_prototypes():
    """Function names with a prototype in include/rydemu.h (comments stripped first,
    so a mention inside a comment cannot stand in for a declaration)."""
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    protos = re.findall(r"\b(ryd_[a-z0-9_]+)\s*\(", code)
    return header, set(protos)


def test_header_parser_ignores_comments():
    _, protos = _header_prototypes()
    assert "ryd_set_detuning_terms" in protos and "ryd_create" in protos and "ryd_last_error" in protos
    code = "/* ryd_fake (0 = none) */ int ryd_real(int a);"
    stripped = re.sub(r"/\*.*?\*/", " ", code, flags=re.S)
    assert re.findall(r"(ryd_[a-z0-9_]+)\s*\(", stripped) == ["ryd_real"]


def test_library_exports_every_declared_symbol():
    import shutil
    import subprocess

    from pulser_amd import _lib

    header, declared = _header_prototypes()
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.ryd_abi_version() == _lib.RYD_ABI_VERSION
    assert f"#define RYD_ABI_VERSION {_lib.RYD_ABI_VERSION}" in header
    # both directions: the dynamic symbol table exports exactly the declared entry points
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ryd_")}
    assert exported == declared, exported ^ declared


def test_engine_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pulser_amd.engine import Engine

    prob, _ = load_fixture("cfg1_square4_pi.npz")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine.from_problems([prob])


def test_factored_trajectory_lowering_equals_general_lowering():
    """HamiltonianData.device_tables (scales/offsets on shared series) must give
    the same time-dependent coefficients as lowering every noisy problem."""
    from pulser_amd.terms import lower

    _, extra = load_fixture("cfg4_chain12_noise.npz")
    nm = NoiseModel(temperature=50.0, amp_sigma=0.05, laser_waist=175.0, detuning_sigma=0.3,
                    state_prep_error=0.2, p_false_pos=0.01)
    inputs = _chain12_inputs(extra).extend_duration(3101)
    np.random.seed(3)
    hd = HamiltonianData(inputs, nm, 6)
    assert hd.factorable()
    trajs = hd.noise_trajectories
    assert any(t.bad_atoms.any() for t in trajs)
    fac = hd.device_tables(trajs, 1.0)
    gen = lower([hd.problem(t, 1.0) for t in trajs])
    assert fac.pp.shape[0] == 3 and gen.pp.shape[0] > 20
    assert np.array_equal(fac.interaction, gen.interaction)

    def coefs(tb, b, k, i, u):
        d = tb.desc[b, k]
        val = lambda s: np.polyval(tb.pp[s, i], u) if s >= 0 else 0.0  # noqa: E731
        c = d["drive_scale"] * val(d["drive_series"])
        dl = d["det_scale"] * np.real(val(d["det_series"])) + d["off_scale"] * np.real(val(d["off_series"]))
        return c, dl

    for b in range(len(trajs)):
        for k in range(12):
            for i, u in ((0, 0.0004), (499, 0.0009), (1700, 0.0005), (3099, 0.00099)):
                cf, df = coefs(fac, b, k, i, u)
                cg, dg = coefs(gen, b, k, i, u)
                assert abs(cf - cg) < 1e-12 * max(1.0, abs(cg)), (b, k, i)
                assert abs(df - dg) < 1e-11 * max(1.0, abs(dg)), (b, k, i)


# ------------------------------------------------------------------ XY mode
def _xy_emulator(k, solver=Solver.MESOLVER):
    """Emulator for MESOLVER case k of test_simulation.py:1536-1690 (XY mode)."""
    prob, extra = load_fixture(f"noisy_xy_{k}.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    noise = extra["noise"]
    leak = noise == "leakage"
    if leak or noise == "eff_noise":
        op = np.diag([1.0, -1.0, 0.0]).astype(complex) if leak else np.diag([1.0, -1.0]).astype(complex)
        params = dict(eff_noise_opers=[op], eff_noise_rates=[1.0])
    else:
        params = {f"{noise}_rate": LEGACY_DEFAULTS[f"{noise}_rate"]}
    nm = NoiseModel(samples_per_run=10, with_leakage=leak, state_prep_error=0.4,
                    p_false_pos=0.01, p_false_neg=0.05, **params)
    np.random.seed(int(extra["seed"]))
    emu = QutipEmulator(inputs, sampling_rate=0.1, noise_model=nm, n_trajectories=15, solver=solver)
    return emu, extra


class _FakeSolvePerTrajectory:
    def __init__(self, emu, states):
        self.emu, self.states, self.k = emu, list(states), 0

    def __call__(self, problems, progress_bar, options, tables=None, mc_ntraj=None):
        out = []
        for _ in range(len(problems) if tables is None else tables.batch):
            out += _FakeSolve(self.emu, self.states[self.k])([None], progress_bar, options)
            self.k += 1
        return out


@pytest.mark.parametrize("k", range(6))
def test_emulator_golden_counters_xy(k, monkeypatch):
    """XY mode, SLM mask, SPAM state-preparation trajectories (deduplicated),
    per-evaluation-time sampling with measurement flips, final resampling of
    the NoisyResults: the reference's golden Counters with the solver stubbed."""
    emu, extra = _xy_emulator(k)
    noise = extra["noise"]
    assert set(emu.noise_model.noise_types) == ({"SPAM", noise} if noise != "leakage"
                                                 else {"SPAM", "leakage", "eff_noise"})
    assert emu.basis_name == ("XY_with_error" if noise == "leakage" else "XY")
    trajs = emu._hamiltonian_data.noise_trajectories
    assert list(trajs[0].bad_atoms) == [True, False, True, False]  # test_simulation.py:1669-1674
    assert np.array_equal([t.reps for t in trajs], extra["traj_reps"])
    assert np.array_equal(np.array([t.bad_atoms for t in trajs]), extra["traj_bad_atoms"])
    assert len(emu._current_problem["collapse_ops"]) == extra["n_collapse_ops"]
    assert np.array_equal(emu.evaluation_times, extra["eval_times"])
    assert emu._current_problem["interaction_matrix"].shape == (2, 4, 4)
    monkeypatch.setattr(emu, "_solve_batch",
                        _FakeSolvePerTrajectory(emu, extra["oracle_traj_lookup_states"]))
    with pytest.warns(DeprecationWarning):
        r = emu.run()
    idx = r._get_index_from_time(emu._eval_times_array[-1])
    assert dict(r[idx].bitstring_counts) == extra["oracle_total_final_counter"]
    assert r.sample_final_state() == Counter(extra["reference_golden_counter"])
    with pytest.raises(NotImplementedError, match="mode 'XY' does not support simulation of"):
        QutipEmulator(SequenceInputs.from_dict(load_fixture(f"noisy_xy_{k}.npz")[0]["inputs"]),
                      noise_model=NoiseModel(temperature=50), n_trajectories=1)


# ------------------------------------------------------------------ DMM channels
def test_dmm_channel_samples_and_noise_follow_pulser_core():
    """Detuning-map-modulator channel (sampler/samples.py:448-456, 560-608) next to
    a global Rydberg channel: per-qubit weights, dmm_sigma / crosstalk / doppler
    trajectories exactly as pulser-core's HamiltonianData produced them -
    including the reference's shared ``dmm_det_fluctuation`` dict (every
    trajectory carries the factor drawn last, hamiltonian_data.py:794, 880-888)."""
    prob, extra = load_fixture("dmm_square4.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    dmm = [c for c in inputs.channels if c.is_dmm]
    assert len(dmm) == 1 and dmm[0].addressing == "Global" and not np.any(dmm[0].amp)
    assert np.allclose(dmm[0].dmm_weight_map(None), [0.1, 0.4, 0.2, 0.3])
    ext = inputs.extend_duration(inputs.max_duration + 1)
    # noiseless: global channel stays global, the DMM is distributed per qubit
    np.random.seed(77)
    hd = HamiltonianData(ext, NoiseModel(), 1)
    assert np.array_equal(np.random.get_state()[1][:4], extra["noiseless_rng_probe"])
    nested = hd.problem(hd.noise_trajectories[0], 1.0)["samples"]
    assert np.any(nested["Global"]["ground-rydberg"]["amp"])
    loc = nested["Local"]["ground-rydberg"]
    assert np.array_equal(np.stack([loc[q]["det"] for q in range(4)]), extra["noiseless_det"][0])
    assert not np.any(np.stack([loc[q]["amp"] for q in range(4)]))
    # noisy: everything local; detuning = rydberg det + doppler (twice: once per
    # channel slot, as the reference adds it) + factor * crosstalk weight * dmm det
    nm = NoiseModel(**extra["noisy_model"])
    assert {"dmm_sigma", "dmm_crosstalk", "doppler", "SPAM"} <= set(nm.noise_types)
    np.random.seed(77)
    hd = HamiltonianData(ext, nm, 5)
    assert np.array_equal(np.random.get_state()[1][:4], extra["noisy_rng_probe"])
    trajs = hd.noise_trajectories
    assert len(trajs) == 5 and not hd.factorable()
    assert np.allclose([t.dmm_det_fluctuation["dmm_0"] for t in trajs], extra["noisy_dmm_factor"])
    assert len(set(extra["noisy_dmm_factor"])) == 1  # the shared-dict quirk
    assert np.array_equal(np.array([t.bad_atoms for t in trajs]), extra["noisy_bad"])
    for i, t in enumerate(trajs):
        loc = hd.problem(t, 1.0)["samples"]["Local"]["ground-rydberg"]
        assert np.array_equal(np.stack([loc[q]["det"] for q in range(4)]), extra["noisy_det"][i]), i
        assert np.array_equal(np.stack([loc[q]["amp"] for q in range(4)]), extra["noisy_amp"][i]), i
    # round trip of the DMM fields
    back = SequenceInputs.from_dict(inputs.to_dict())
    assert np.array_equal(back.channels[0].dmm_weight_map(4.0) if back.channels[0].is_dmm
                          else back.channels[1].dmm_weight_map(4.0), dmm[0].dmm_weight_map(4.0))


# ----------------------------------------------------- Results abstract repr
def test_results_abstract_repr_and_aggregation_match_pulser_core():
    """JSON written by pulser-core's own ``Results.to_abstract_repr`` and
    ``Results.aggregate`` (pulser/backend/results.py:267-488; fixture): read it,
    write it back identically, aggregate identically."""
    import json

    from pulser_amd.backend import Results, RydState

    _, extra = load_fixture("results_abstract_repr.npz")
    mine = []
    for text in extra["json_texts"]:
        res = Results.from_abstract_repr(text)
        assert res.atom_order == ("q0", "q1", "q2") and res.total_duration == 1000
        assert res.get_result("expectation", 1.0) == complex(0.5, json.loads(text)["results"][
            str(res._tagmap["expectation"])][1]["imag"])
        assert res.get_result_times("occupation") == [0.5, 1.0]
        assert json.loads(res.to_abstract_repr()) == json.loads(text)
        mine.append(res)
    assert mine[1].bitstrings[1] == {"010": 4, "111": 11}
    import warnings as _w
    with _w.catch_warnings():  # 'custom_skipped' is SKIP: dropped silently
        _w.simplefilter("error")
        agg = Results.aggregate(mine)
    ref = json.loads(extra["aggregated_json"])
    got = json.loads(agg.to_abstract_repr())
    assert set(got["tagmap"]) == set(ref["tagmap"]) and "custom_skipped" not in got["tagmap"]
    assert got == ref
    mean, std = agg.get_result("array", 1.0)
    assert np.allclose(mean, [1.0, 3.0, 1.5]) and np.allclose(std, [0.0, 1.0, 0.0])
    # user-supplied aggregators and incompatible inputs (results.py:356-430)
    top = Results.aggregate(mine, energy=max, occupation="skip")
    assert top.get_result("energy", 0.5) == 2 - 3.25 * 0.5 and "occupation" not in top.get_result_tags()
    other = Results(("q0", "q1"), 1000)
    with pytest.raises(ValueError, match="result `bitstrings` is not present in all results"):
        Results.aggregate([mine[0], other])
    other = Results.from_abstract_repr(extra["json_texts"][0])
    other.atom_order = ("q0", "q1")
    with pytest.raises(ValueError, match="same atom order"):
        Results.aggregate([mine[0], other])
    other = Results.from_abstract_repr(extra["json_texts"][0])
    other.total_duration = 2000
    with pytest.raises(ValueError, match="same sequence duration"):
        Results.aggregate([mine[0], other])
    with pytest.raises(ValueError, match="No results to aggregate."):
        Results.aggregate([])
    assert Results.aggregate([mine[0]]) is mine[0]
    # states serialise only when built from amplitudes (backend/state.py:234-254)
    st = RydState.from_state_amplitudes(eigenstates=("r", "g"), amplitudes={"rg": 0.6, "gr": 0.8j})
    d = json.loads(json.dumps({"s": st}, cls=type(agg)._encoder()))
    assert d["s"]["eigenstates"] == ["r", "g"] and d["s"]["amplitudes"]["gr"] == {"real": 0.0, "imag": 0.8}
    with pytest.raises(ValueError, match="from_state_amplitudes"):
        RydState(np.array([1.0, 0.0]), eigenstates=("r", "g"))._to_abstract_repr()


# ------------------------------------------------------- SimConfig surface
def _two_atom_inputs():
    coords = np.array([[0.0, 0.0], [0.0, 5.0]])
    n = 2500
    return single_global_channel(coords, {"amp": np.full(n, np.pi), "det": np.zeros(n),
                                          "phase": np.zeros(n)}, P.C6_LEVEL70, extended=False)


@pytest.mark.filterwarnings("ignore::DeprecationWarning")
def test_simconfig_str_and_validation():
    """tests/pulser_simulation/test_simconfig.py:40-100."""
    config = SimConfig(noise=("SPAM", "doppler", "dephasing", "amplitude"), temperature=1000.0, runs=100)
    assert config.temperature == 1000.0 * 1e-6  # stored in K
    text = config.__str__(True)
    assert "SPAM, doppler, dephasing, amplitude" in text
    assert "1000.0µK" in text and "100" in text and "Solver Options" in text
    assert config.to_noise_model().temperature == 1000.0
    config = SimConfig(noise=("depolarizing", "relaxation", "doppler"))
    assert config.temperature == pytest.approx(50.0e-6)
    assert config.to_noise_model().temperature == 50.0
    text = config.__str__(True)
    assert f"Depolarizing rate: {config.depolarizing_rate}" in text
    assert f"Relaxation rate: {config.relaxation_rate}" in text
    assert config.spam_dict == {"eta": 0.005, "epsilon": 0.01, "epsilon_prime": 0.05}
    # KEFF * sqrt(KB * T / MASS), hamiltonian_data.py:49-54, 122-129
    assert config.doppler_sigma == pytest.approx(8.7 * np.sqrt(1.38e-23 * 50e-6 / 1.45e-25))
    assert not config.with_leakage and "dmm_sigma" in config.supported_noises["ising"]
    with pytest.raises(ValueError, match="is not a valid noise type."):
        SimConfig(noise="bad_noise")
    with pytest.raises(ValueError, match="SPAM parameter"):
        SimConfig(eta=-1.0)
    with pytest.raises(TypeError, match="'temperature' must be a float"):
        SimConfig(temperature="0.0")
    with pytest.raises(ValueError, match="must be equal"):
        SimConfig(noise="eff_noise", eff_noise_opers=[np.eye(2)], eff_noise_rates=[])


@pytest.mark.filterwarnings("ignore::DeprecationWarning")
def test_emulator_simconfig_surface(capsys):
    """tests/pulser_simulation/test_simulation.py:828-891 and :1315-1395 (the parts
    that do not need the solver): set / add / reset / show config."""
    z3 = np.diag([1.0, -1.0, 0.0]).astype(complex)
    np.random.seed(123)
    with pytest.warns(DeprecationWarning, match="Supplying a 'SimConfig' to QutipEmulator"):
        sim = QutipEmulator(_two_atom_inputs(), config=SimConfig(noise="SPAM"))
    sim.reset_config()
    assert sim.config == SimConfig()
    sim.show_config()
    assert "Number of runs:" in capsys.readouterr().out
    with pytest.raises(ValueError, match="not a valid"):
        sim.set_config("bad_config")
    new_cfg = SimConfig(noise="doppler", temperature=10000)
    with pytest.warns(DeprecationWarning, match="Supplying a 'SimConfig' to QutipEmulator"):
        sim.set_config(new_cfg)
    assert sim.config == new_cfg
    ground2 = np.zeros(4); ground2[3] = 1
    assert np.array_equal(np.asarray(sim.initial_state)[:, 0], ground2)
    # in the ground state: the initial state follows the new dimension silently
    sim.set_config(SimConfig(noise=("leakage", "eff_noise"), eff_noise_opers=[z3], eff_noise_rates=[0.1]))
    assert sim.dim == 3
    ground3 = np.zeros(9); ground3[4] = 1  # |g g> with (r, g, x) ordering
    assert np.array_equal(np.asarray(sim.initial_state)[:, 0], ground3)
    # otherwise it is reset to all-ground with a warning
    other = np.zeros(9); other[0] = 1
    sim.set_initial_state(other)
    with pytest.warns(UserWarning, match="Current initial state's dimension does not match new dim"):
        sim.set_config(SimConfig(noise="SPAM", eta=0.5))
    assert np.array_equal(np.asarray(sim.initial_state)[:, 0], ground2)
    # add_config (test_simulation.py:1315-1395)
    with pytest.raises(ValueError, match="is not a valid"):
        sim.add_config("bad_cfg")
    sim.add_config(SimConfig(noise=("SPAM", "doppler", "eff_noise"),
                             eff_noise_opers=[np.eye(2), np.array([[0, 1.0], [1.0, 0]])],
                             eff_noise_rates=[0.4, 0.6], temperature=20000))
    assert {"doppler", "SPAM", "eff_noise"} <= set(sim.config.noise)
    assert sim.config.eta == 0.5 and sim.config.temperature == 20000.0e-6
    sim.set_config(SimConfig(noise="doppler", laser_waist=175.0))
    sim.add_config(SimConfig(noise=("SPAM", "amplitude", "dephasing"), laser_waist=172.0, amp_sigma=1e-2))
    assert {"amplitude", "dephasing", "SPAM"} <= set(sim.config.noise)
    assert sim.config.laser_waist == 172.0 and sim.config.amp_sigma == 1e-2
    sim.set_config(SimConfig(noise="SPAM", eta=0.5))
    sim.add_config(SimConfig(noise="depolarizing"))
    assert "depolarizing" in sim.config.noise
    with pytest.raises(NotImplementedError, match="does not support simulation of noise types"):
        xy = SequenceInputs.from_dict(load_fixture("noisy_xy_0.npz")[0]["inputs"])
        QutipEmulator(xy).set_config(SimConfig(noise="doppler"))


def test_sampled_result_sampling_errors_and_plots(tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from pulser_amd.results import NoisyResults, SampledResult

    res = SampledResult(("q0", "q1"), "ground-rydberg", Counter({"00": 60, "11": 40}))
    assert res.sampling_errors == {"00": pytest.approx(np.sqrt(0.6 * 0.4 / 100)),
                                   "11": pytest.approx(np.sqrt(0.6 * 0.4 / 100))}
    times = np.array([0.0, 1.0])
    noisy = NoisyResults([res, res], 2, "ground-rydberg", times, 100)
    op = np.diag([1.0, 0.0, 0.0, 0.0])
    noisy.plot(op, label="x")
    noisy.plot(op, error_bars=False)
    plt.savefig(tmp_path / "p.png")
    plt.close("all")
    emu = QutipEmulator(_two_atom_inputs())
    emu.draw(fig_name=str(tmp_path / "seq.png"))
    assert (tmp_path / "seq.png").exists()


# ------------------------------------- reference goldens of the detuning noise
def _three_channel_inputs(duration=10):
    """The sequence of test_simulation.py:2269-2290: a global Rydberg channel with
    two pulses and two local Raman channels (q0, q1), all amplitudes zero."""
    z = np.zeros(2 * duration)
    coords = np.array([[0.0, 0.0], [10.0, 10.0]])
    chans = [
        ChannelInput("ch0", "Global", "ground-rydberg", z, z, z,
                     [Slot(0, duration, (0, 1)), Slot(duration, 2 * duration, (0, 1))]),
        ChannelInput("ch1", "Local", "digital", z, z, z, [Slot(0, duration, (0,))]),
        ChannelInput("ch2", "Local", "digital", z, z, z, [Slot(0, duration, (1,))]),
    ]
    return SequenceInputs(coords, ("q0", "q1"), chans, P.C6_LEVEL70)


def test_detuning_sigma_noise_reference_golden():
    """tests/pulser_simulation/test_simulation.py:2269-2310 (seed 1337)."""
    duration = 10
    np.random.seed(1337)
    sim = QutipEmulator(_three_channel_inputs(duration), noise_model=NoiseModel(detuning_sigma=0.1),
                        n_trajectories=1)
    s = sim._current_problem["samples"]
    assert s["Global"] == {}
    ryd, dig = s["Local"]["ground-rydberg"], s["Local"]["digital"]
    assert np.allclose(ryd[0]["det"], [-0.04902824] * (2 * duration) + [0.0])
    assert np.allclose(ryd[1]["det"], [-0.04902824] * (2 * duration) + [0.0])
    assert np.allclose(dig[0]["det"], [-0.17550787] * duration + [0.0] * (duration + 1))
    assert np.allclose(dig[1]["det"], [-0.20112646] * duration + [0.0] * (duration + 1))


def test_detuning_hf_noise_reference_golden():
    """tests/pulser_simulation/test_simulation.py:2313-2413 (seed 1337)."""
    np.random.seed(1337)
    nm = NoiseModel(detuning_hf_psd=2.0 * np.pi * np.array([1, 2, 3]),
                    detuning_hf_omegas=2.0 * np.pi * np.array([4, 5, 6]))
    sim = QutipEmulator(_three_channel_inputs(10), noise_model=nm, n_trajectories=1)
    s = sim._current_problem["samples"]
    ryd, dig = s["Local"]["ground-rydberg"], s["Local"]["digital"]
    rydberg_expected = [
        -17.09974803, -17.62331808, -18.12297186, -18.59816646, -19.04839245, -19.47317443,
        -19.87207157, -20.24467805, -20.59062348, -20.9095733, -21.20122904, -21.46532868,
        -21.70164676, -21.90999467, -22.09022068, -22.24221006, -22.36588509, -22.46120504,
        -22.52816608, -22.56680119, 0.0]
    assert np.allclose(ryd[0]["det"], rydberg_expected)
    assert np.allclose(ryd[1]["det"], rydberg_expected)
    assert np.allclose(dig[0]["det"], [
        -20.70981369, -20.9854774, -21.23382708, -21.4546608, -21.64781307, -21.81315499,
        -21.95059426, -22.06007519, -22.1415786, -22.19512177] + [0.0] * 11)
    assert np.allclose(dig[1]["det"], [
        -20.13322478, -19.96053451, -19.76371088, -19.54313969, -19.29923617, -19.03244438,
        -18.74323637, -18.43211151, -18.09959565, -17.74624031] + [0.0] * 11)


def _spam_all_emulator():
    """test_simulation.py:889-903 (test_noise): CCZ sequence, eta = 0.9, seed 3."""
    prob, extra = load_fixture("noise_spam_all.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    nm = NoiseModel(samples_per_run=5, p_false_pos=0.01, p_false_neg=0.05, state_prep_error=0.9)
    np.random.seed(int(extra["seed"]))
    emu = QutipEmulator(inputs, sampling_rate=0.01, noise_model=nm, n_trajectories=15)
    return emu, extra


def test_emulator_golden_counter_spam_trajectories_all_basis(monkeypatch, capsys):
    """The reference's ``test_noise`` golden (test_simulation.py:904-923): 15 SPAM
    trajectories deduplicated to reps [13, 1, 1], 3-level "all" basis measured in
    the digital basis, per-time sampling + flips, final resampling; solver stubbed."""
    emu, extra = _spam_all_emulator()
    trajs = emu._hamiltonian_data.noise_trajectories
    assert [t.reps for t in trajs] == list(extra["traj_reps"]) == [13, 1, 1]
    assert np.array_equal(np.array([t.bad_atoms for t in trajs]), extra["traj_bad_atoms"])
    assert emu.basis_name == "all" and emu._meas_basis == "digital"
    assert np.array_equal(emu.evaluation_times, extra["eval_times"])
    assert emu._current_problem["samples"]["Global"] == {}  # SPAM -> everything local
    bad = trajs[0].bad_atoms
    assert any(bad)
    for basis in ("ground-rydberg", "digital"):
        for q in np.nonzero(bad)[0]:
            for qty in ("amp", "det", "phase"):
                assert np.all(emu._current_problem["samples"]["Local"][basis][int(q)][qty] == 0.0)
    monkeypatch.setattr(emu, "_solve_batch",
                        _FakeSolvePerTrajectory(emu, extra["oracle_traj_lookup_states"]))
    with pytest.warns(DeprecationWarning):
        r = emu.run(print_progress=True)
    assert capsys.readouterr().out.rstrip("\n").split("\n") == [
        "Emulating Trajectories [1 - 13]/15", "Emulating Trajectory 14/15",
        "Emulating Trajectory 15/15"]
    idx = r._get_index_from_time(emu._eval_times_array[-1])
    assert dict(r[idx].bitstring_counts) == extra["oracle_total_final_counter"]
    assert r.sample_final_state() == Counter(extra["reference_golden_counter"])
    with pytest.raises(NotImplementedError, match="Cannot include"):
        QutipEmulator(SequenceInputs.from_dict(load_fixture("noise_spam_all.npz")[0]["inputs"]),
                      noise_model=NoiseModel(depolarizing_rate=0.05))


def _results_noisy_emulator():
    """tests/pulser_simulation/test_simresults.py:63-90 (``results_noisy``), seed 123."""
    prob, extra = load_fixture("results_noisy.npz")
    nm = NoiseModel(**{k: (int(v) if k == "samples_per_run" else float(v))
                       for k, v in extra["noise_model"].items()})
    np.random.seed(int(extra["seed"]))
    emu = QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), noise_model=nm, n_trajectories=15)
    return emu, extra


def _check_results_noisy(r, extra):
    """test_simresults.py:383-389 (expect ~ 0.68), :446-456 (seeded final Counter)."""
    op = np.kron(np.eye(2), np.diag([1.0, 0.0])).astype(complex)
    assert np.isclose(r.expect([op])[0][-1], float(extra["reference_expect_last"]))
    bad = op.copy()
    bad[0, 1] = 1.0
    with pytest.raises(ValueError, match="non-diagonal"):
        r.expect([bad])
    np.random.seed(123)
    assert r.sample_final_state(N_samples=1234) == Counter(extra["reference_golden_counter"])


def test_results_noisy_reference_goldens(monkeypatch):
    """Doppler + laser-waist amplitude + SPAM trajectories sampled at all 1001
    evaluation times: the reference's seeded ``results_noisy`` goldens with the
    solver stubbed (RNG order of 15 x 1001 sample_state calls)."""
    emu, extra = _results_noisy_emulator()
    assert set(emu.noise_model.noise_types) == {"SPAM", "doppler", "amplitude"}
    assert np.array_equal(emu.evaluation_times, extra["eval_times"]) and len(emu.evaluation_times) == 1001
    assert [t.reps for t in emu._hamiltonian_data.noise_trajectories] == [1] * 15
    monkeypatch.setattr(emu, "_solve_batch",
                        _FakeSolvePerTrajectory(emu, extra["oracle_traj_lookup_states"]))
    with pytest.warns(DeprecationWarning):
        r = emu.run()
    assert len(r) == 1001 and r._use_pseudo_dens
    assert dict(r[-1].bitstring_counts) == extra["oracle_total_final_counter"]
    _check_results_noisy(r, extra)


def _final_state_noisy_emulator():
    """tests/pulser_simulation/test_simresults.py:244-261, seed 123."""
    prob, extra = load_fixture("final_state_noisy.npz")
    nm = NoiseModel(**{k: (int(v) if k == "samples_per_run" else float(v))
                       for k, v in extra["noise_model"].items()})
    np.random.seed(int(extra["seed"]))
    emu = QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), noise_model=nm, n_trajectories=15)
    return emu, extra


def _check_final_state_noisy(r, extra):
    """test_simresults.py:267-275."""
    r._meas_basis = "digital"
    final = np.asarray(r.get_final_state())
    assert np.count_nonzero(final - np.diag(np.diagonal(final))) == 0
    r._meas_basis = "ground-rydberg"
    assert final[0, 0] == 0.04 + 0j and final[2, 2] == 0.96 + 0j
    assert np.array_equal(np.asarray(r.states[-1]), final)
    assert r.results[-1] == Counter(extra["reference_golden_results_last"])


def test_get_final_state_noisy_reference_golden(monkeypatch):
    """Digital basis, local Raman pulse, doppler + trap position fluctuations +
    SPAM: the reference's seeded pseudo-density golden with the solver stubbed."""
    emu, extra = _final_state_noisy_emulator()
    assert set(emu.noise_model.noise_types) == {"SPAM", "doppler", "register"}
    assert emu.basis_name == "digital" and emu._meas_basis == "digital"
    assert [t.reps for t in emu._hamiltonian_data.noise_trajectories] == list(extra["traj_reps"])
    monkeypatch.setattr(emu, "_solve_batch",
                        _FakeSolvePerTrajectory(emu, extra["oracle_traj_lookup_states"]))
    with pytest.warns(DeprecationWarning):
        r = emu.run()
    _check_final_state_noisy(r, extra)


def _slm_effective_size_emulator(ch):
    """test_simulation.py:1928-1988: square(2) register, 1.5 us constant pulse,
    SLM mask on atom1, state_prep_error 0.4, seed 15092021."""
    prob, extra = load_fixture(f"slm_effective_size_{ch}.npz")
    nm = NoiseModel(**{k: (int(v) if k == "samples_per_run" else float(v))
                       for k, v in extra["noise_model"].items()})
    np.random.seed(int(extra["seed"]))
    emu = QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), sampling_rate=0.01,
                        noise_model=nm, n_trajectories=15)
    return emu, extra


@pytest.mark.parametrize("ch", ["mw_global", "rydberg_global", "raman_global"])
def test_slm_mask_and_bad_atoms_effective_size(ch):
    """test_simulation.py:1960-2042 (``test_effective_size_disjoint``): the first
    trajectory's bad atoms and per-atom samples - the SLM detuning map on the
    masked atom (-10 x amp), zeroed pulses on the badly prepared atoms - equal what
    pulser-core's HamiltonianData produced."""
    emu, extra = _slm_effective_size_emulator(ch)
    assert list(emu._hamiltonian_data.noise_trajectories[0].bad_atoms) == [True, False, True, False]
    assert list(extra["traj0_bad_atoms"]) == [True, False, True, False]
    assert emu.samples_obj.slm_end == int(extra["slm_end"]) == 1500
    loc = emu._current_problem["samples"]["Local"]
    keys = [k for k in extra if k.startswith("local__")]
    assert {k.split("__")[1] for k in keys} == set(loc)
    for k in keys:
        _, basis, q, qty = k.split("__")
        assert np.array_equal(loc[basis][int(q)][qty], extra[k]), k
    if ch != "mw_global":
        basis = "ground-rydberg" if ch == "rydberg_global" else "digital"
        amp = np.concatenate((np.ones(1500), [0.0]))
        assert np.array_equal(loc[basis][1]["amp"], amp) and np.array_equal(loc[basis][3]["amp"], amp)
        assert np.all(loc["ground-rydberg"][1]["det"] == -10 * amp)
        assert not np.any(loc[basis][3]["det"]) and not np.any(loc[basis][0]["amp"])


def _slm_mask_emulators(*names):
    prob, extra = load_fixture("slm_masks.npz")
    return [QutipEmulator(SequenceInputs.from_dict(prob[n])) for n in names], extra


def test_slm_mask_next_to_a_local_channel():
    """test_simulation.py:1841-1926: the global Rydberg pulse stays global, the SLM
    mask appears as a -10 x amp detuning map on the masked atoms, the local Raman
    pulse (phase pi) stays on its target."""
    (emu,), _ = _slm_mask_emulators("local")
    assert emu.samples_obj.slm_end == 1000 and set(emu.samples_obj.slm_targets) == {0, 3}
    nested = emu._current_problem["samples"]
    g = nested["Global"]["ground-rydberg"]
    ten = np.concatenate((10.0 * np.ones(1000), [0.0]))
    assert np.array_equal(g["amp"], ten) and not np.any(g["det"]) and not np.any(g["phase"])
    loc = nested["Local"]["ground-rydberg"]
    for q in range(4):
        assert np.array_equal(loc[q]["det"], -10 * ten if q in (0, 3) else 0 * ten)
        assert not np.any(loc[q]["amp"]) and not np.any(loc[q]["phase"])
    dig = nested["Local"]["digital"]
    assert list(dig) == [0]
    assert np.array_equal(dig[0]["amp"], ten)
    assert np.array_equal(dig[0]["det"], np.concatenate((-5.0 * np.ones(1000), [0.0])))
    assert np.allclose(dig[0]["phase"], np.concatenate((np.pi * np.ones(1000), [0.0])))


def test_slm_mask_xy_equals_removing_the_qubit_host_assembly():
    """test_simulation.py:1748-1838 on the host: the problems the emulator hands to
    the solver, assembled by the oracle - masked XY Hamiltonian = two-qubit
    Hamiltonian x identity while the mask is on, = unmasked Hamiltonian afterwards."""
    from oracle import qutip_path as qp

    (masked, three, two, eq_m, eq_2), extra = _slm_mask_emulators(
        "tp_masked", "tp_three", "tp_two", "eq_masked", "eq_two")
    ti, tf = (int(x) for x in extra["tp_mask_time"])
    hm, h3, h2 = (qp.build_hamiltonian(e._current_problem) for e in (masked, three, two))
    for t in masked.sampling_times[::7]:
        m = hm.matrix(t).toarray()
        if ti <= t * 1e3 <= tf:
            assert np.allclose(m, np.kron(h2.matrix(t).toarray(), np.eye(2)), atol=1e-12), t
        else:
            assert np.allclose(m, h3.matrix(t).toarray(), atol=1e-12), t
    hm, h2 = (qp.build_hamiltonian(e._current_problem) for e in (eq_m, eq_2))
    for t in eq_2.sampling_times[::5]:
        assert np.allclose(hm.matrix(t).toarray(), np.kron(h2.matrix(t).toarray(), np.eye(2)), atol=1e-12)


@pytest.mark.parametrize("tag", ["none", "x", "y", "z"])
def test_modulated_samples_with_laser_waist_and_propagation_direction(tag):
    """test_simulation.py:2045-2153: output-modulated samples, doppler + laser-waist
    amplitude noise for the four beam propagation directions; the first trajectory's
    per-atom samples equal what pulser-core's HamiltonianData produced."""
    prob, extra = load_fixture(f"modulation_dir_{tag}.npz")
    nm = NoiseModel(**{k: (int(v) if k == "samples_per_run" else float(v))
                       for k, v in extra["noise_model"].items()})
    np.random.seed(int(extra["seed"]))
    emu = QutipEmulator(SequenceInputs.from_dict(prob["inputs"]), noise_model=nm, n_trajectories=15)
    nested = emu._current_problem["samples"]
    assert nested["Global"] == {}  # all samples stored in local (:2095-2097)
    keys = [k for k in extra if k.startswith("local__")]
    assert {k.split("__")[1] for k in keys} == set(nested["Local"])
    for k in keys:
        _, basis, q, qty = k.split("__")
        np.testing.assert_allclose(nested["Local"][basis][int(q)][qty], extra[k], rtol=1e-13, atol=1e-14,
                                   err_msg=k)
    # the reference's own checks (:2098-2150)
    mod, dt = extra["modulated_pulse"], int(extra["mod_dt"])
    dop = emu._hamiltonian_data.noise_trajectories[0].doppler_detune
    assert np.array_equal(dop, extra["doppler"])
    raman = nested["Local"]["digital"]
    for q, sl in ((1, slice(0, dt)), (0, slice(dt, 2 * dt))):  # target, control1
        np.testing.assert_allclose(raman[q]["amp"][sl], mod, atol=1e-2)
        assert np.all(raman[q]["det"][sl] == dop[q])
        np.testing.assert_allclose(raman[q]["phase"][sl], 2.0)
    coords = np.array([[-4.0, 0.0], [0.0, 4.0], [4.0, 0.0]])
    r = {"none": coords[:, 0], "y": coords[:, 0], "x": coords[:, 1],
         "z": np.linalg.norm(coords, axis=1)}[tag]
    pos = np.exp(-((r / 175.0) ** 2))
    ryd, sl = nested["Local"]["ground-rydberg"], slice(2 * dt, 3 * dt)
    base = ryd[1]["amp"][sl] / (mod * pos[1])
    for q in range(3):
        np.testing.assert_allclose(ryd[q]["amp"][sl], mod * base * pos[q])
        assert np.all(ryd[q]["det"][sl] == dop[q])


def _eom_emulator(k):
    """test_simulation.py:2593-2641: EOM mode at the detuning limits, seed 123."""
    prob, extra = load_fixture(f"eom_limit_det_{k}.npz")
    np.random.seed(int(extra["seed"]))
    return QutipEmulator(SequenceInputs.from_dict(prob["inputs"])), extra


@pytest.mark.parametrize("k", [0, 1])
def test_emulator_golden_counters_eom_detuning_limits(k, monkeypatch):
    """The reference's seeded Counters of ``test_eom_limit_det`` (detuning_on =
    +/- max_abs_detuning, phase-drift correction) with the solver stubbed."""
    emu, extra = _eom_emulator(k)
    assert emu._tot_duration == 4520 and np.array_equal(emu.evaluation_times, extra["eval_times"])
    det = emu._current_problem["samples"]["Global"]["ground-rydberg"]["det"]
    assert abs(det).max() == pytest.approx(max(abs(float(extra["detuning_on"])),
                                               abs(float(extra["detuning_off"]))))
    # the sequence ends in EOM mode: the extra trailing sample keeps the block's
    # detuning_off instead of zero (sampler/samples.py:170-180)
    assert np.array_equal(det, extra["reference_det"]) and det[-1] != 0.0
    assert emu.samples_obj.channels[0].final_detuning == det[-1]
    monkeypatch.setattr(emu, "_solve_batch", _FakeSolve(emu, extra["oracle_lookup_state"]))
    with pytest.warns(DeprecationWarning):
        res = emu.run()
    assert res.sample_final_state() == Counter(extra["reference_golden_counter"])


MULTICHANNEL_CASES = ["amp_sigma", "runs_detuning_sigma", "runs_amp_sigma", "runs_temperature",
                      "runs_trap", "runs_hf", "concurrent"]


@pytest.mark.parametrize("name", MULTICHANNEL_CASES)
def test_multichannel_noisy_samples_follow_pulser_core(name):
    """Per-trajectory samples of multi-channel sequences - one amplitude factor per
    channel with two local channels sharing a basis (test_simulation.py:2193-2266),
    the five ``test_noisy_runs`` noise models (:2422-2470) and concurrent local +
    global pulses under doppler noise (:1401-1427) - equal pulser-core's."""
    prob, extra = load_fixture("multichannel_noise.npz")
    inputs = SequenceInputs.from_dict(prob[name])
    kw = dict(extra[f"{name}__noise_model"])
    for k in ("detuning_hf_psd", "detuning_hf_omegas"):
        if k in kw:
            kw[k] = tuple(kw[k])
    if "samples_per_run" in kw:
        kw["samples_per_run"] = int(kw["samples_per_run"])
    np.random.seed(int(extra[f"{name}__seed"]))
    hd = HamiltonianData(inputs.extend_duration(inputs.max_duration + 1), NoiseModel(**kw),
                         int(extra[f"{name}__n_trajectories"]))
    assert np.array_equal(np.random.get_state()[1][:4], extra[f"{name}__rng_probe"])
    trajs = hd.noise_trajectories
    assert len(trajs) == int(extra[f"{name}__n_distinct"])
    for i, t in enumerate(trajs):
        p = hd.problem(t, 1.0)
        assert p["samples"]["Global"] == {} and t.reps == int(extra[f"{name}__traj{i}__reps"])
        keys = [k for k in extra if k.startswith(f"{name}__traj{i}__") and k.count("__") == 4]
        assert {k.split("__")[2] for k in keys} == set(p["samples"]["Local"])
        for k in keys:
            _, _, basis, q, qty = k.split("__")
            np.testing.assert_allclose(p["samples"]["Local"][basis][int(q)][qty], extra[k],
                                       rtol=1e-14, atol=1e-14, err_msg=k)
        np.testing.assert_allclose(p["interaction_matrix"], extra[f"{name}__traj{i}__interaction"],
                                   rtol=1e-13, atol=0)
    if name == "amp_sigma":  # the reference's own assertions (:2226-2266)
        loc = hd.problem(trajs[0], 1.0)["samples"]["Local"]
        f0 = loc["ground-rydberg"][0]["amp"][0]
        f1, f2 = loc["digital"][0]["amp"][0], loc["digital"][1]["amp"][0]
        assert len({f0, f1, f2}) == 3 and all(f > 0 and f != 1 for f in (f0, f1, f2))
        q1 = loc["digital"][1]["amp"]
        assert np.all(q1[:120] == f2) and np.all(q1[-121:-1] == f1)


def test_backend_v2_refuses_register_noise_with_a_dmm_without_spot_waist():
    """tests/pulser_simulation/test_qutip_backend_v2.py:583-613 (pulser/backend/abc.py:106-121)."""
    from pulser_amd.backend import QutipBackendV2, QutipConfig, StateResult

    inputs = SequenceInputs.from_dict(load_fixture("dmm_square4.npz")[0]["inputs"])
    cfg = QutipConfig(noise_model=NoiseModel(trap_waist=1.0, trap_depth=1.0, temperature=0.5),
                      observables=[StateResult(evaluation_times=[1.0])])
    with pytest.raises(ValueError, match="Combining register noise with a DMM requires"):
        QutipBackendV2(inputs, config=cfg)
    assert callable(QutipBackendV2.run_from_sequence_samples)


def test_state_result_reduce_to_basis():
    """qutip_result.py:160-242: global phase, reduction of a 3-level ket to a
    two-level basis, the population tolerance and the reference's error messages."""
    # "all" basis (r, g, h), two atoms: amplitude on |gg>, |gh>, |hg> only
    psi = np.zeros(9, dtype=complex)
    psi[4], psi[5], psi[7] = 0.6j, 0.48j, 0.64j  # gg, gh, hg
    psi[0] = 1e-5  # a little Rydberg population
    res = StateResult(("a", "b"), "digital", QState(psi), False)
    assert res._basis_name == "all" and res._eigenbasis == ["r", "g", "h"]
    red = np.asarray(res.get_state(reduce_to_basis="digital", normalize=False)).ravel()
    assert red.shape == (4,)  # gg, gh, hg, hh with the global phase of the largest term removed
    assert np.allclose(red, [0.6, 0.48, 0.64, 0.0]) and abs(red[2].imag) < 1e-15
    unit = np.asarray(res.get_state(reduce_to_basis="digital")).ravel()
    assert abs(np.linalg.norm(unit) - 1) < 1e-15
    with pytest.raises(TypeError, match="Can't reduce to chosen basis because the population"):
        res.get_state(reduce_to_basis="ground-rydberg")
    with pytest.raises(TypeError, match="Can't reduce to chosen basis because the population"):
        res.get_state(reduce_to_basis="digital", tol=1e-12)
    with pytest.raises(ValueError, match="'reduce_to_basis' must be 'ground-rydberg', 'XY', or 'digital'"):
        res.get_state(reduce_to_basis="all")
    with pytest.raises(ValueError, match="Can't reduce a state expressed in all into XY"):
        res.get_state(reduce_to_basis="XY")
    rho = QState(np.outer(psi, psi.conj()))
    with pytest.raises(NotImplementedError, match="not implemented for density matrix"):
        StateResult(("a", "b"), "digital", rho, False).get_state(reduce_to_basis="digital")
    two = StateResult(("a",), "ground-rydberg", QState(np.array([0.6, 0.8j])), True)
    with pytest.raises(TypeError, match="Can't reduce a system in ground-rydberg to the digital basis"):
        two.get_state(reduce_to_basis="digital")
    kept = np.asarray(two.get_state(ignore_global_phase=False)).ravel()
    assert np.array_equal(kept, [0.6, 0.8j])
    assert np.allclose(np.asarray(two.get_state()).ravel(), [-0.6j, 0.8])


def test_evaluation_times_instructions():
    """test_simulation.py:721-815 (``set_evaluation_times``) on the CCZ sequence."""
    inputs = SequenceInputs.from_dict(load_fixture("noise_spam_all.npz")[0]["inputs"])

    def fresh():
        return QutipEmulator(inputs, sampling_rate=1.0)

    with pytest.raises(ValueError, match="evaluation_times float must be between 0 and 1."):
        fresh().set_evaluation_times(3.0)
    for bad in (123, "Best"):
        with pytest.raises(ValueError, match="Wrong evaluation time label."):
            fresh().set_evaluation_times(bad)
    sim = fresh()
    st, end = sim.sampling_times, sim._tot_duration / 1000
    with pytest.raises(ValueError, match="Provided evaluation-time list contains negative values."):
        sim.set_evaluation_times([-1, 0, st[-2]])
    with pytest.raises(ValueError, match="Provided evaluation-time list extends further than sequence duration."):
        sim.set_evaluation_times([0, st[-1] + 10])
    sim.set_evaluation_times("Full")
    assert sim._eval_times_instruction == "Full"
    np.testing.assert_almost_equal(sim._eval_times_array, st)
    sim.set_evaluation_times("Minimal")
    np.testing.assert_almost_equal(sim._eval_times_array, [st[0], end])
    sim.set_evaluation_times([0, st[-3], end])
    np.testing.assert_almost_equal(sim._eval_times_array, [0, st[-3], end])
    for empty in ([], 0.0001):
        sim.set_evaluation_times(empty)
        np.testing.assert_almost_equal(sim._eval_times_array, [0, end])
    sim.set_evaluation_times([st[-10], st[-3]])
    np.testing.assert_almost_equal(sim._eval_times_array, [0, st[-10], st[-3], end])
    sim.set_evaluation_times(0.4)
    np.testing.assert_almost_equal(
        st[np.linspace(0, len(st) - 1, int(0.4 * len(st)), dtype=int)], sim._eval_times_array)


@pytest.mark.parametrize("dim", [2, 3])
def test_two_and_three_dimensional_registers(dim):
    """tests/pulser_simulation/test_hamiltonian.py:31-80: 2D and 3D registers with a global
    channel and two local channels build without error; U = C6 / round(r, 6)^6."""
    from oracle import qutip_path as qp

    coords = np.array([[-4.0, 0.0, 0.0], [0.0, 4.0, 3.0]])[:, :dim]
    z = np.zeros(20)
    inputs = SequenceInputs(coords, ("q0", "q1"), [
        ChannelInput("ch0", "Global", "ground-rydberg", z + 1.0, z, z, slots=[Slot(0, 20, (0, 1))]),
        ChannelInput("ch1", "Local", "digital", z, z, z, slots=[Slot(0, 10, (0,))]),
        ChannelInput("ch2", "Local", "digital", z, z, z, slots=[Slot(0, 10, (1,))])], P.C6_LEVEL70)
    emu = QutipEmulator(inputs, sampling_rate=0.5)
    prob = emu._current_problem
    r = round(float(np.linalg.norm(coords[0] - coords[1])), 6)
    assert prob["interaction_matrix"][0][0, 1] == pytest.approx(P.C6_LEVEL70 / r**6, rel=1e-14)
    assert qp.build_hamiltonian(prob).matrix(0.005).shape == (4, 4)  # the idle digital basis is unused
    np.random.seed(1)
    noisy = QutipEmulator(inputs, sampling_rate=0.5, n_trajectories=2,
                          noise_model=NoiseModel(temperature=30.0, trap_depth=150.0, trap_waist=1.0))
    assert [t.coords.shape for t in noisy._hamiltonian_data.noise_trajectories] == [(2, 3), (2, 3)]


def test_noisy_interaction_matrix_seeded_golden_and_dmm_detuning():
    """/tests/test_hamiltonian_data.py:511-560 (seed 0xDEADBEEF, state_prep_error 0.5: bad atoms
    [batman, aquaman], U(superman, ironman) = 26.4198) and :678-759 (DMM detuning with dmm_sigma:
    det_q = det + factor x weight_q x dmm_det)."""
    c6_level60 = 865723.02  # AnalogDevice (rydberg_level 60), pulser/devices/interaction_coefficients
    coords = np.array([[-4.0, 0.0], [4.0, 0.0], [0.0, 4.0], [0.0, -4.0]])
    w = np.clip(np.blackman(200), 0, np.inf)
    amp = w * (np.pi / 5) / (w.sum() * 1e-3)
    inputs = SequenceInputs(coords, ("batman", "superman", "ironman", "aquaman"),
                            [ChannelInput("ch0", "Global", "ground-rydberg", amp, 0 * amp, 0 * amp,
                                          slots=[Slot(0, 200, (0, 1, 2, 3))])], c6_level60)
    np.random.seed(0xDEADBEEF)
    hd = HamiltonianData(inputs.extend_duration(201), NoiseModel(state_prep_error=0.5), 1)
    traj = hd.noise_trajectories[0]
    assert list(traj.bad_atoms) == [True, False, False, True]
    mat = hd.problem(traj, 1.0)["interaction_matrix"]
    expected = np.zeros((1, 4, 4))
    expected[0, 1, 2] = expected[0, 2, 1] = 26.4198
    assert np.allclose(mat, expected, atol=1e-4)
    # DMM: two atoms with weights 1.0 / 0.5, constant detunings
    xy = np.array([[0.0, 0.0], [0.0, 5.0]])
    ones = np.ones(100)
    ryd = ChannelInput("ch0", "Global", "ground-rydberg", ones, -1.0 * ones, 0 * ones, slots=[Slot(0, 100, (0, 1))])
    dmm = ChannelInput("dmm_0", "Global", "ground-rydberg", 0 * ones, -10.0 * ones, 0 * ones,
                       slots=[Slot(0, 100, (0, 1))], dmm_trap_coords=xy, dmm_weights=np.array([1.0, 0.5]),
                       dmm_qubit_coords=xy)
    seq = SequenceInputs(xy, ("q0", "q1"), [ryd, dmm], c6_level60)
    np.random.seed(0xDEADBEEF)
    clean = HamiltonianData(seq.extend_duration(101), NoiseModel(), 1)
    nested = clean.problem(clean.noise_trajectories[0], 1.0)["samples"]
    loc = nested["Local"]["ground-rydberg"]  # noiseless: the Rydberg channel stays global
    assert np.allclose(nested["Global"]["ground-rydberg"]["det"][:100], -1.0)
    assert np.allclose(loc[0]["det"][:100], -10 * 1.0) and np.allclose(loc[1]["det"][:100], -10 * 0.5)
    noisy = HamiltonianData(seq.extend_duration(101), NoiseModel(dmm_sigma=0.5), 1)
    t0 = noisy.noise_trajectories[0]
    factor = t0.dmm_det_fluctuation["dmm_0"]
    assert isinstance(t0.dmm_det_fluctuation, dict) and factor >= 0 and not np.isclose(factor, 1.0)
    loc = noisy.problem(t0, 1.0)["samples"]["Local"]["ground-rydberg"]
    assert np.allclose(loc[0]["det"][:100], -1 - 10 * 1.0 * factor)
    assert np.allclose(loc[1]["det"][:100], -1 - 10 * 0.5 * factor)


def test_dmm_only_sequence_is_not_factored():
    """A DMM channel scales its detuning per qubit (weights, dmm_sigma factor, spot waist:
    hamiltonian_data.py:414-421, 880-888) - not a (series, scale) pair of the shared channel
    samples.  ``device_tables`` must therefore equal ``lower(problem(...))``: the weight-0 atom
    sees no DMM detuning and the weight-0.5 atom half of it (the factored form gave all three
    atoms the full detuning)."""
    from pulser_amd.terms import lower

    xy = np.array([[0.0, 0.0], [0.0, 6.0], [6.0, 0.0]])
    ones = np.ones(100)
    dmm = ChannelInput("dmm_0", "Global", "ground-rydberg", 0 * ones, -10.0 * ones, 0 * ones,
                       slots=[Slot(0, 100, (0, 1, 2))], dmm_trap_coords=xy,
                       dmm_weights=np.array([1.0, 0.5, 0.0]), dmm_qubit_coords=xy)
    seq = SequenceInputs(xy, ("q0", "q1", "q2"), [dmm], 865723.02)
    np.random.seed(5)
    hd = HamiltonianData(seq.extend_duration(101), NoiseModel(temperature=50.0, dmm_sigma=0.2), 3)
    assert not hd.factorable()
    trajs = hd.noise_trajectories
    fac = hd.device_tables(trajs, 1.0)
    ref = lower([hd.problem(t, 1.0) for t in trajs])
    assert np.array_equal(fac.desc, ref.desc) and np.array_equal(fac.pp, ref.pp)
    assert np.array_equal(fac.tknots, ref.tknots) and np.array_equal(fac.interaction, ref.interaction)
    # the per-atom detunings really differ by the weights
    for b, t in enumerate(trajs):
        loc = hd.problem(t, 1.0)["samples"]["Local"]["ground-rydberg"]
        f = t.dmm_det_fluctuation["dmm_0"]
        dop = [loc[q]["det"][50] + 10.0 * w * f for q, w in enumerate((1.0, 0.5, 0.0))]
        assert np.allclose(dop, np.asarray(t.doppler_detune, float), atol=1e-12), (b, dop)


@pytest.mark.parametrize("leakage", [False, True])
def test_building_basis_and_projection_operators(leakage):
    """tests/pulser_simulation/test_simulation.py:253-430: eigenbasis and dimension per
    addressed basis (with / without the leakage level), ``build_operator`` and its errors."""
    def noise(dim):
        return (NoiseModel(with_leakage=True, eff_noise_opers=[np.eye(dim)], eff_noise_rates=[0.0])
                if leakage else NoiseModel())

    def kets(dim, names):
        return {s: np.eye(dim)[:, [i]] for i, s in enumerate(names)}

    amp = np.ones(100)
    z = np.zeros(100)
    coords = np.array([[-4.0, 0.0], [0.0, 4.0], [4.0, 0.0]])
    ids = ("control1", "target", "control2")

    def emulator(channels, dim, **kw):
        return QutipEmulator(SequenceInputs(coords, ids, channels, P.C6_LEVEL70, **kw), sampling_rate=0.1,
                             noise_model=noise(dim))

    ryd = ChannelInput("ryd", "Local", "ground-rydberg", amp, z, z, slots=[Slot(0, 100, (1,))])
    ram = ChannelInput("ram", "Local", "digital", amp, z, z, slots=[Slot(0, 100, (1,))])
    glob = ChannelInput("glob", "Global", "ground-rydberg", amp, z, z, slots=[Slot(0, 100, (0, 1, 2))])
    mw = ChannelInput("mw", "Global", "XY", amp, z, z, slots=[Slot(0, 100, (0, 1, 2))])
    suffix = "_with_error" if leakage else ""
    x = ["x"] if leakage else []
    for channels, name, states, kw in (
            ([ryd, ram], "all", ["r", "g", "h"], {}),
            ([glob], "ground-rydberg", ["r", "g"], {}),
            ([ram], "digital", ["g", "h"], {}),
            ([ryd], "ground-rydberg", ["r", "g"], {}),
            ([mw], "XY", ["u", "d"], dict(interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0)))):
        dim = len(states) + leakage
        sim = emulator(channels, dim, **kw)
        assert sim.basis_name == name + suffix and sim.dim == dim
        want = kets(dim, states + x)
        assert list(sim.basis) == states + x
        for s in want:
            assert np.array_equal(np.asarray(sim.basis[s]), want[s])
        a, b = states[0], states[1]
        proj = sim.build_operator([(f"sigma_{a}{a}", ["target"])])
        assert np.array_equal(proj, np.kron(np.kron(np.eye(dim), want[a] @ want[a].T), np.eye(dim)))
        low = sim.build_operator([(f"sigma_{b}{a}", ["control2"])])
        assert np.array_equal(low, np.kron(np.eye(dim * dim), want[b] @ want[a].T))
        if leakage:
            assert np.array_equal(sim.build_operator([(f"sigma_x{a}", ["control1"])]),
                                  np.kron(want["x"] @ want[a].T, np.eye(dim * dim)))
    sim = emulator([ryd, ram], 3 + leakage)
    with pytest.raises(ValueError, match="Duplicate atom"):
        sim.build_operator([("sigma_gg", ["target", "target"])])
    with pytest.raises(ValueError, match="not a valid operator"):
        sim.build_operator([("wrong", ["target"])])
    with pytest.raises(ValueError, match="Invalid qubit names: {'wrong'}"):
        sim.build_operator([("sigma_gg", ["wrong"])])
    one = sim.build_operator(("sigma_gg", ["target"]))
    assert np.array_equal(one, sim.build_operator([("sigma_gg", ["target"])]))
    total = sim.build_operator([("sigma_rr", "global")])
    assert np.array_equal(total, sum(sim.build_operator([("sigma_rr", [q])]) for q in ids))
    zz = sim.build_operator([("sigma_gg", ["control1", "target"]), ("sigma_rr", ["control2"])])
    d = sim.dim
    g, r = np.eye(d)[:, [1]], np.eye(d)[:, [0]]
    assert np.array_equal(zz, np.kron(np.kron(g @ g.T, g @ g.T), r @ r.T))


def test_laser_waist_hf_detuning_and_register_noise_follow_pulser_core():
    """amp_sigma x finite laser waist (hamiltonian_data.py:758-780), detuning_sigma
    + high-frequency detuning PSD (:132-169), doppler and register noise (:116-130)
    in one noise model: the per-trajectory samples, noisy coordinates and
    interaction matrices equal what pulser-core produced (fixture, seed 5)."""
    prob, extra = load_fixture("waist_tri6.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    kw = dict(extra["noise_model"])
    for k in ("detuning_hf_psd", "detuning_hf_omegas"):
        kw[k] = tuple(kw[k])
    nm = NoiseModel(**kw)
    assert set(nm.noise_types) == {"amplitude", "detuning", "doppler", "register"}
    np.random.seed(int(extra["seed"]))
    hd = HamiltonianData(inputs.extend_duration(inputs.max_duration + 1), nm, 4)
    assert np.array_equal(np.random.get_state()[1][:4], extra["rng_probe"])
    assert hd.factorable()
    n = inputs.n_qudits
    for i, t in enumerate(hd.noise_trajectories):
        assert np.allclose(t.coords, extra["coords"][i], rtol=0, atol=1e-15)
        p = hd.problem(t, 1.0)
        loc = p["samples"]["Local"]["ground-rydberg"]
        assert np.allclose(np.stack([loc[q]["amp"] for q in range(n)]), extra["amp"][i], rtol=1e-15, atol=0)
        assert np.allclose(np.stack([loc[q]["det"] for q in range(n)]), extra["det"][i], rtol=1e-14, atol=1e-14)
        assert np.allclose(p["interaction_matrix"], extra["interaction"][i], rtol=1e-13, atol=0)


def _eval_tables_detuning(tables, b, k, t):
    """delta_k(t) of trajectory b from DeviceTables (host evaluation of the spline
    pieces, the arithmetic of k_eval_coefs)."""
    idx = np.clip(np.searchsorted(tables.tknots, t, side="right") - 1, 0, len(tables.tknots) - 2)
    u = t - tables.tknots[idx]

    def val(series):
        c = tables.pp[series, idx]
        return (((c[:, 0] * u + c[:, 1]) * u + c[:, 2]) * u + c[:, 3]).real

    d = tables.desc[b, k]
    out = np.zeros_like(t)
    if d["det_series"] >= 0:
        out += d["det_scale"] * val(d["det_series"])
    if d["off_series"] >= 0:
        out += d["off_scale"] * val(d["off_series"])
    e = d["extra"] - 1
    while e >= 0:
        term = tables.dterms[e]
        out += term["scale"] * val(term["series"])
        if term["remaining"] == 0:
            break
        e += 1
    return out


def test_factored_lowering_with_hf_detuning_noise_equals_per_trajectory_lowering():
    """the high-frequency detuning noise is synthesised from
    shared cos / sin series and per-trajectory amplitudes (ryd_dterm table) instead
    of one spline per (trajectory, atom): same detuning, drive and interaction as
    lowering every trajectory's noisy samples."""
    from pulser_amd.terms import lower

    prob, extra = load_fixture("waist_tri6.npz")
    inputs = SequenceInputs.from_dict(prob["inputs"])
    kw = dict(extra["noise_model"])
    for key in ("detuning_hf_psd", "detuning_hf_omegas"):
        kw[key] = tuple(kw[key])
    np.random.seed(5)
    hd = HamiltonianData(inputs.extend_duration(inputs.max_duration + 1), NoiseModel(**kw), 4)
    trajs = hd.noise_trajectories
    fact = hd.device_tables(trajs, 1.0)
    assert fact.dterms is not None and np.all(fact.desc["extra"] > 0)
    assert (fact.dterms["remaining"] == 0).sum() == 4  # one shared list per trajectory (global channel)
    full = lower([hd.problem(t, 1.0) for t in trajs])
    assert full.dterms is None and len(fact.pp) < len(full.pp)
    t = np.random.default_rng(0).uniform(0.0, inputs.max_duration * 1e-3, 400)
    for b in range(4):
        for k in range(inputs.n_qudits):
            a = _eval_tables_detuning(fact, b, k, t)
            c = _eval_tables_detuning(full, b, k, t)
            assert np.max(np.abs(a - c)) < 1e-11 * max(1.0, np.max(np.abs(c)))
    assert np.allclose(fact.interaction, full.interaction, rtol=1e-14, atol=0)


def test_config_abstract_repr_reads_and_rewrites_pulser_core_documents():
    """EmulationConfig JSON written by pulser-core (backend/config.py:438-447,
    noise_model.py:676-699, observable.py:132-139; fixture): read into a
    QutipConfig and written back - identical except for the four QuTiP-backend
    options this config adds (qutip_config.py:144-150)."""
    import json

    from pulser_amd.backend import BitStrings, Fidelity, QutipConfig, StateResult

    _, extra = load_fixture("config_abstract_repr.npz")
    for name in ("plain", "noisy", "register", "operator"):
        ref = json.loads(extra[name])
        cfg = QutipConfig.from_abstract_repr(extra[name])
        got = json.loads(cfg.to_abstract_repr())
        for key in ("sampling_rate", "solver", "print_progress", "progress_bar"):
            assert key in got
            got.pop(key)
        assert got == ref, name
    cfg = QutipConfig.from_abstract_repr(extra["noisy"])
    nm = cfg.noise_model
    assert set(nm.noise_types) == {"SPAM", "amplitude", "dephasing", "detuning", "doppler", "eff_noise"}
    assert nm.laser_waist == 150.0 and nm.detuning_hf_omegas == (3.0, 4.0) and cfg.n_trajectories == 7
    assert np.array_equal(np.asarray(nm.eff_noise_opers[1]), np.array([[1, 0], [0, -1j]]))
    reg = QutipConfig.from_abstract_repr(extra["register"]).noise_model
    assert reg.disable_doppler and "doppler" not in reg.noise_types and reg.trap_depth == 150.0
    plain = QutipConfig.from_abstract_repr(extra["plain"])
    assert [o.tag for o in plain.observables] == ["bitstrings", "occupation", "correlation_matrix",
                                                  "energy_x", "energy_variance", "energy_second_moment",
                                                  "fidelity"]
    assert isinstance(plain.observables[-1], Fidelity) and plain.observables[4].default_aggregation == "skip_warn"
    assert str(plain.observables[0]._uuid) == json.loads(extra["plain"])["observables"][0]["uuid"]
    changed = plain.with_changes(sampling_rate=0.5, n_trajectories=9)
    assert changed.sampling_rate == 0.5 and changed.n_trajectories == 9 and len(changed.observables) == 7
    # Expectation of an operator given as a sum of tensor products (operator.py:115-235)
    from pulser_amd.backend import Expectation, RydOperator, RydState
    op = QutipConfig.from_abstract_repr(extra["operator"]).observables[0].operator
    sx, sy, sz = np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.diag([1.0, -1.0])
    dense = 0.5 * np.kron(np.kron(sx, sz), sz) + (2.0 - 1.0j) * np.kron(np.kron(np.eye(2), sy), np.eye(2))
    assert np.allclose(op.to_qobj().toarray(), dense)
    psi = np.random.default_rng(3).normal(size=8) + 1j * np.random.default_rng(4).normal(size=8)
    st = RydState(psi / np.linalg.norm(psi), eigenstates=("r", "g"))
    assert np.isclose(Expectation(op).apply(state=st), np.vdot(np.asarray(st.to_qobj()), dense @ np.asarray(st.to_qobj())))
    rho = RydState(np.outer(psi, psi.conj()) / np.vdot(psi, psi), eigenstates=("r", "g"))
    assert np.isclose(op.expect(rho), op.expect(st))
    assert np.allclose(np.asarray(op.apply_to(st).to_qobj())[:, 0], dense @ np.asarray(st.to_qobj())[:, 0])
    assert (2 * op + op) == 3 * op and (op @ op).to_qobj().shape == (8, 8)
    with pytest.raises(ValueError, match="Got invalid indices"):
        RydOperator.from_operator_repr(eigenstates=("r", "g"), n_qudits=2, operations=[(1.0, [({"rr": 1}, {2})])])
    with pytest.raises(ValueError, match="Every QuditOp key must be made up"):
        RydOperator.from_operator_repr(eigenstates=("r", "g"), n_qudits=2, operations=[(1.0, [({"rx": 1}, {0})])])
    with pytest.raises(ValueError, match="Can't apply"):
        op.expect(RydState(psi, eigenstates=("g", "h")))
    with pytest.raises(ValueError, match="not supported in any remote backend"):
        QutipConfig(observables=[StateResult()]).to_abstract_repr()
    with pytest.raises(NotImplementedError, match="custom interaction matrices"):
        QutipConfig(observables=[BitStrings()], interaction_matrix=np.eye(2))


def test_default_tolerance_oracle_drift_is_a_measured_quantity():
    """SURVEY 8(d)(ii) planned to assert agreement with "QuTiP-default" output at 5e-5.  The
    restated QuTiP path at its defaults (zvode Adams, atol 1e-8, rtol 1e-6, max_step 1 ns) is
    itself ~1e-3 away from the converged solution on the 12-atom anneal (norm drift -8e-4,
    ``normalize_output=False``), so a converged solver CANNOT be within 5e-5 of it: the GPU tests
    assert <= 1e-7 against the tight oracle and <= 5e-3 against the default-tolerance one
    (tests/test_gpu_parity.py).  This pins the numbers that correction rests on."""
    _, extra = load_fixture("cfg2_chain12_anneal.npz")
    tight = np.asarray(extra["oracle_states_tight"])
    dflt = np.asarray(extra["oracle_states_default"])
    drift = np.max(np.abs(tight[-1] - dflt[-1]))
    assert 5e-5 < drift < 5e-3, drift  # measured 1.4e-3
    assert abs(np.linalg.norm(tight[-1]) - 1.0) < 1e-9
    assert 1e-4 < 1.0 - np.linalg.norm(dflt[-1]) < 2e-3  # the default run loses ~8e-4 of norm
    # and it is reproducible: re-running the oracle at its defaults gives the stored states
    from oracle import qutip_path as qp

    prob, _ = load_fixture("cfg2_chain12_anneal.npz")
    prob = with_anneal_samples(prob)
    ham = qp.build_hamiltonian(prob)
    s = prob["samples"]["Global"]["ground-rydberg"]
    opts = qp.default_options([(s["amp"], s["det"])], 3100)
    again = qp.sesolve(ham, qp.all_ground_state(12, prob["eigenbasis"]),
                       np.asarray(extra["eval_times"])[[0, 1]], **opts)[-1]
    assert np.max(np.abs(again - dflt[1])) < 1e-9


def test_engine_method_names_match_the_header():
    """ryd_opts.method codes of include/rydemu.h and the names Engine.evolve / solve accept."""
    import re

    from pulser_amd import engine

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rydemu.h")).read()
    doc = hdr[hdr.index("int32_t method;"):hdr.index("double reserved[2];")]
    assert re.search(r"0 = the library's choice", doc) and "1 = Lanczos" in doc
    assert "2 = split-operator" in doc and "3 = Taylor polynomial" in doc
    assert engine._METHODS == {"auto": 0, "krylov": 1, "split": 2, "taylor": 3}
    with pytest.raises(ValueError, match="unknown method"):
        engine._method_code("rk4")


def test_engine_set_path_bits_match_the_header():
    """Every bit Engine.set_path can set is documented in the ryd_set_path comment of include/rydemu.h and is handled
    by ryd_set_path (host_step.hpp); no two keywords share a bit."""
    import inspect
    import re

    from pulser_amd import engine

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rydemu.h")).read()
    doc = hdr[hdr.index("/* Test/bench hook (bit mask)"):hdr.index("int ryd_set_path(")]
    documented = {int(v) for v in re.findall(r"\b(\d+) =", doc)}
    src = inspect.getsource(engine.Engine.set_path)
    used = {int(v): kw for v, kw in re.findall(r"\((\d+) if (\w+) else 0\)", src)}
    used[1] = "force_generic"
    assert len(used) == len(set(used.values()))
    assert set(used) <= documented, sorted(set(used) - documented)
    host = open(os.path.join(root, "pulser_amd", "csrc", "host_step.hpp")).read()
    body = host[host.index('extern "C" int ryd_set_path('):]
    body = body[:body.index("\n}\n")]
    handled = {int(v) for v in re.findall(r"force_generic & (\d+)\)", body)}
    assert set(used) <= handled, sorted(set(used) - handled)
    assert all(b & (b - 1) == 0 for b in used)  # single bits
    params = set(inspect.signature(engine.Engine.set_path).parameters) - {"self"}
    assert params == set(used.values()), params ^ set(used.values())


def test_bench_flop_constants_match_the_compiled_kernels():
    """bench.py's roofline divides ISA-counted fp64 flops by kernel time: the constants it uses must be what
    tools/count_isa.py counts in the kernels as compiled now (hipcc cross-compiles without a GPU)."""
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    ns = {}
    for name in ("KKET_FLOPS_PER_AMP_STAGE", "KSPLIT14_FLOPS_PER_AMP_STAGE", "KSPLITREG_FLOPS_PER_AMP_STAGE"):
        exec(re.search(r"^%s = .*$" % name, src, re.M).group(0), ns)
    import tempfile

    tmp = tempfile.mkdtemp()
    asm = os.path.join(tmp, "rydemu.s")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "count_isa.py"), "split14"], check=True,
                         capture_output=True, text=True, timeout=900, env=dict(os.environ, RYD_ISA_KEEP=asm)).stdout
    row = [l for l in out.splitlines() if re.match(r"^\| \d+ \|", l)][0]
    cells = [c.strip() for c in row.strip("|").split("|")]
    assert abs(float(cells[-1]) - ns["KSPLIT14_FLOPS_PER_AMP_STAGE"]) < 0.01 * ns["KSPLIT14_FLOPS_PER_AMP_STAGE"], row
    assert int(cells[6]) <= 16, row  # scratch instructions in the stage loop: reloads of loop invariants at most
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "count_isa.py"), "splitreg"], check=True,
                         capture_output=True, text=True, timeout=900, env=dict(os.environ, RYD_ISA_TEXT=asm)).stdout
    row = [l for l in out.splitlines() if re.match(r"^\| \d+ \|", l)][0]
    cells = [c.strip() for c in row.strip("|").split("|")]
    assert abs(float(cells[-1]) - ns["KSPLITREG_FLOPS_PER_AMP_STAGE"]) < 0.01 * ns["KSPLITREG_FLOPS_PER_AMP_STAGE"], row
    assert int(cells[8]) <= 8 and int(cells[9]) == 4, row  # scratch reloads of loop invariants at most; 4 barriers per stage
    # ... and the 12-atom shape of round 5 (16 amplitudes per lane on 256 lanes)
    exec(re.search(r"^KSPLITREG_SHAPES = .*?\n\n", src, re.M | re.S).group(0), ns)
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "count_isa.py"), "splitreg", "12", "4"], check=True,
                         capture_output=True, text=True, timeout=900).stdout
    row = [l for l in out.splitlines() if re.match(r"^\| \d+ \|", l)][0]
    cells = [c.strip() for c in row.strip("|").split("|")]
    assert ns["KSPLITREG_SHAPES"][12][0] == 4 and abs(float(cells[-1]) - ns["KSPLITREG_SHAPES"][12][1]) < 0.01 * float(cells[-1]), row
    assert int(cells[8]) == 0 and int(cells[9]) == 4, row
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "count_isa.py"), "0"], check=True,
                         capture_output=True, text=True, timeout=900, env=dict(os.environ, RYD_ISA_TEXT=asm)).stdout
    per_half = [float(l.strip("|").split("|")[-1]) for l in out.splitlines() if re.match(r"^\| \d+\.\.\d+ \|", l)]
    assert per_half and abs(2 * sum(per_half) / len(per_half) - ns["KKET_FLOPS_PER_AMP_STAGE"]) < 0.02 * ns["KKET_FLOPS_PER_AMP_STAGE"]


def test_bench_driver_line_is_short_scalar_and_round_trips():
    """The driver keeps an 8-KB tail of stdout and parses its last line (round 5's 21-KB line came back `parsed: null`):
    bench.driver_line cuts the contract line from the full record - here from the committed 21-KB record of round 5 and
    from one stuffed with prose - and must stay below 6 KB, carry the contract's keys, and hold scalars only."""
    import json
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench

    full = json.load(open(os.path.join(root, "profiles", "r05_bench.json")))
    assert len(json.dumps(full)) > 20000
    stuffed = json.loads(json.dumps(full))
    stuffed["config"]["workload"] = "w" * 5000
    stuffed["roofline"]["kernel"] = "k_split_reg<14, 5> (" + "x" * 5000 + ")"
    stuffed["cpu_baseline"]["sample"] = "s" * 5000
    stuffed["collective"] = {"backend": "nccl", "world_size": 8, "distinct_devices": 8, "allreduce_of_ones": 8.0,
                             "ranks": [{"rank": r, "pci": "0000:%02x:00" % r, "name": "n" * 100} for r in range(8)]}
    for rec in (full, stuffed):
        line = bench.driver_line(rec)
        text = json.dumps(line)
        assert len(text) <= bench.MAX_LINE_BYTES < 8192, len(text)
        assert json.loads(text) == line
        assert {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"} <= set(line)
        assert line["value"] == pytest.approx(full["value"], rel=1e-5) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
        assert all(not isinstance(v, (dict, list)) for v in line["config"].values())
        assert len(line["config"]["workload"]) <= 200 and len(line["cpu_baseline"]["sample"]) <= 120
        assert {"n_atoms", "sequences_per_gpu", "stages_per_sequence", "parity_max_abs", "single_sequence_sim_us_per_s",
                "lindblad_seconds", "api_full_ms", "api_minimal_ms", "cfg2_sim_us_per_s", "cfg4_traj_per_s",
                "cfg5_sim_us_per_s"} <= set(line["config"])
        roof = line["roofline"]
        assert roof["kernel"] == "k_split_reg<14, 5>" and roof["bound"] == "valu_f64"
        assert {"achieved", "peak", "unit", "frac", "frac_algorithmic", "us_per_stage", "traffic"} <= set(roof)
        assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-4)
        assert {"value", "unit", "cores", "kind", "sample", "host_cpu_count"} <= set(line["cpu_baseline"])
    assert bench.driver_line(stuffed)["collective"] == {"backend": "nccl", "world_size": 8, "distinct_devices": 8,
                                                        "allreduce_of_ones": 8.0}
    # a line without legs / cpu leg (N > 1, --no-cpu) still carries the keys
    bare = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                 "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    bare["config"] = {"workload": "x"}
    line = bench.driver_line(bare)
    assert line["roofline"] is None and line["cpu_baseline"] is None



def test_bench_output_sample_is_seeded_bounded_and_float64(tmp_path):
    """bench.py --dump-outputs: the final state of the last timed step whole when it fits the budget, else the same
    seeded sample of 2^14-amplitude pieces every run (the 256 x 14-atom headline batch: 128 kets); float64 files only,
    together below 64 MB, and the pieces kept are the state's own rows."""
    import sys

    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench

    g = torch.Generator().manual_seed(3)
    occ = torch.rand(15, dtype=torch.float64, generator=g)
    small = torch.randn(16, 4096, dtype=torch.complex128, generator=g)
    out = bench.output_sample(torch, small, occ)
    assert np.array_equal(out["final_state"][..., 0] + 1j * out["final_state"][..., 1], small.numpy())
    assert np.array_equal(out["final_state_pieces"], np.arange(16)) and np.array_equal(out["occupations"], occ.numpy())
    big = torch.randn(256, 2**14, dtype=torch.complex128, generator=g)
    out = bench.output_sample(torch, big, occ)
    rows = out["final_state_pieces"].astype(int)
    assert out["final_state"].shape == (128, 2**14, 2) and len(np.unique(rows)) == 128
    assert np.array_equal(out["final_state"][..., 0] + 1j * out["final_state"][..., 1], big.numpy()[rows])
    assert np.array_equal(bench.output_sample(torch, big * 2, occ)["final_state_pieces"], out["final_state_pieces"])
    bench.write_outputs(str(tmp_path / "dump"), out)
    files = sorted((tmp_path / "dump").iterdir())
    assert [f.name for f in files] == ["final_state.npy", "final_state_pieces.npy", "occupations.npy"]
    assert sum(f.stat().st_size for f in files) <= 64e6
    assert all(np.load(f).dtype == np.float64 for f in files)

def test_c_replay_equals_the_numpy_replay():
    """ryd_replay_samples (host_replay.hpp; host arithmetic only, so it runs without a GPU): weights, cumulative sums,
    searchsorted and the SPAM flips of a block of states in the same IEEE operations as the NumPy replay
    (distributed.cumulative_weights + np.searchsorted + flips_with = qutip_result.py:101-158, multinomial.py:32-36,
    simresults.py:537-568) - identical histograms for kets and density-matrix diagonals, both measurement bases, a
    non-matching basis, with and without measurement errors, empty rows, one and several host threads."""
    from pulser_amd.distributed import cumulative_weights, flips_with, replay_block_native

    rng = np.random.default_rng(0)
    n, n_eval, B = 9, 3, 17
    D = 2**n
    for is_ket in (True, False):
        for basis, matching in (("ground-rydberg", True), ("digital", True), ("ground-rydberg", False)):
            for meas in (True, False):
                host = rng.normal(size=(n_eval, B, D)) + 1j * rng.normal(size=(n_eval, B, D))
                host[1, 2, 5:40] = 0.0  # runs of equal cumulative weights
                if not is_ket:
                    host = np.abs(host) ** 2 + 0j
                counts = rng.integers(0, 700, size=(n_eval, B))
                counts[0, 0] = 0
                starts = np.concatenate([[0], np.cumsum(counts.reshape(-1))[:-1]]).reshape(n_eval, B)
                total = int(counts.sum())
                rnd, mat = rng.random(total), (rng.random((total, n)) if meas else None)
                want = np.zeros((n_eval, D), dtype=np.int64)
                cum = cumulative_weights(host, is_ket, basis, matching)
                for ti in range(n_eval):
                    for j in range(B):
                        a, c = starts[ti, j], counts[ti, j]
                        ind = flips_with(np.searchsorted(cum[ti, j], rnd[a:a + c]), n, mat[a:a + c] if meas else None, 0.03, 0.08)
                        want[ti] += np.bincount(ind, minlength=D)
                for threads in (1, 4):
                    got = np.full((n_eval, D), 7, dtype=np.int64)  # (accumulates into what is there)
                    replay_block_native(host, is_ket, basis, matching, n, starts, counts, rnd, mat, 0.03, 0.08, got, n_threads=threads)
                    assert np.array_equal(got - 7, want), (is_ket, basis, matching, meas, threads)
    # a uniform beyond the last cumulative weight is refused (NumPy would index past the histogram)
    host = np.zeros((1, 1, 4), dtype=complex)
    host[0, 0, 0] = 1.0
    from pulser_amd import _lib

    with pytest.raises(_lib.RydError, match="beyond the last cumulative weight"):
        replay_block_native(host, True, "digital", True, 2, np.zeros((1, 1), dtype=np.int64), np.ones((1, 1), dtype=np.int64),
                            np.array([1.5]), None, 0.0, 0.0, np.zeros((1, 4), dtype=np.int64))


def test_phase_gauge_of_the_split_operator_stages_is_an_identity():
    """SplitRun.gauge (k_split.hpp: k_split_coefs): a rotation by a complex drive c = |c| e^{i theta} is Z R(|c|) Z^+ with
    the diagonal Z = exp(-i theta n), and Z commutes with the D factors - so the composition D R(c_S) D ... R(c_1) D equals
    the one with real rotations R(|c_j|) whose D factors carry theta_j - theta_{j-1} on top of the detuning integral
    (theta_0 = 0, the closing D returns to theta = 0).  The kernel's conventions restated in NumPy for one atom: index 0 =
    bit clear (n = 1), index 1 = bit set (n = 0); y0 = C a0 + g' a1, y1 = C a1 + g a0 with g = -i S c, g' = (-Re g, Im g);
    D = diag(exp(i Delta), 1).  A drive that vanishes at a stage (theta undefined -> 0) is included."""
    rng = np.random.default_rng(0)
    S = 10
    beta = rng.normal(size=S) * 0.3
    c = rng.normal(size=S) + 1j * rng.normal(size=S)
    c[3] = 0.0
    delta = rng.normal(size=S + 1)

    def rot(cj, b):
        m = abs(cj)
        C, Sn = np.cos(b * m), (np.sin(b * m) / m if m > 1e-300 else b)
        g = -1j * Sn * cj
        return np.array([[C, complex(-g.real, g.imag)], [g, C]])

    def diag(d):
        return np.diag([np.exp(1j * d), 1.0])

    U = np.eye(2, dtype=complex)
    for j in range(S):
        U = rot(c[j], beta[j]) @ diag(delta[j]) @ U
    U = diag(delta[S]) @ U
    theta = [np.angle(x) if abs(x) > 1e-300 else 0.0 for x in c]
    V, prev = np.eye(2, dtype=complex), 0.0
    for j in range(S):
        V = rot(abs(c[j]), beta[j]) @ diag(delta[j] + theta[j] - prev) @ V
        prev = theta[j]
    V = diag(delta[S] - prev) @ V
    assert np.max(np.abs(U - V)) < 1e-14


def test_fuzz_cases_are_seeded_and_well_formed():
    """tests/helpers.py: fuzz_case (the controller fuzz of tests/test_gpu_fuzz.py): a seed gives the same sequences every
    time (named regressions stay the cases they were), samples carry the extra trailing sample of simulation.py:173 with
    amp = det = 0, amplitudes are non-negative, all problems of a batch share register and duration."""
    from helpers import fuzz_case

    kinds = set()
    for seed in (0, 40, 263, 279, 306):
        probs, desc = fuzz_case(seed)
        again, desc2 = fuzz_case(seed)
        assert desc == desc2 and len(probs) == len(again)
        for p, q in zip(probs, again):
            a, b = p["samples"]["Global"]["ground-rydberg"], q["samples"]["Global"]["ground-rydberg"]
            for k in ("amp", "det", "phase"):
                assert np.array_equal(a[k], b[k])
            assert len(a["amp"]) == p["duration"] and a["amp"][-1] == 0.0 and a["det"][-1] == 0.0
            assert np.all(a["amp"] >= 0.0) and np.all(np.isfinite(a["det"])) and a["amp"].max() <= 30.0 + 1e-9
            assert np.array_equal(p["coords"], probs[0]["coords"]) and p["duration"] == probs[0]["duration"]
        kinds.add(desc.split("(")[1].split(",")[0])
    assert fuzz_case(40)[1].startswith("seed 40: 12 atoms (chain, 5.03 um), 3415 ns")
    assert fuzz_case(263)[1].startswith("seed 263: 16 atoms (chain, 6.51 um), 283 ns")
    assert len(kinds) >= 1


def test_every_launched_k_split_reg_instantiation_is_listed_for_the_part_units():
    """The library is four translation units (k_split_reg_inst.hpp): rydemu.hip declares the k_split_reg instantiations
    `extern template` and rydemu_splitreg.hip defines them from ONE list - an instantiation launched by host_split.hpp but
    missing from the list would only fail at link time on the build box."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inst = open(os.path.join(root, "pulser_amd", "csrc", "k_split_reg_inst.hpp")).read()
    host = open(os.path.join(root, "pulser_amd", "csrc", "host_split.hpp")).read()
    generic = {tuple(x.strip() for x in m.split(",")) for m in re.findall(r"X\(N_, ([^)]*)\)", inst)}
    extra = {(n,) + tuple(x.strip() for x in rest.split(",")) for n, rest in re.findall(r"X\((\d+), ([^)]*)\)", inst)}

    def canon(args):
        args = [a.strip() for a in args]
        return tuple(args + ["false"] * (5 - len(args)))  # NR, DECAY, ROWS, CPLX, SNAP

    launched = re.findall(r"k_split_reg<(N|\d+), ([^>]*)>", host)
    assert launched
    for n, rest in launched:
        args = canon(rest.split(","))
        if n == "N":
            assert args in generic, (n, args)
        else:
            assert args in generic or (n,) + args in extra, (n, args)


def test_window_tables_are_cuts_of_the_full_sequence_tables():
    """simulation.QutipEmulator._window_tables (round 6: evaluation_times="Full" in time-parallel windows): entry b * J + j of
    the window batch carries the spline PIECES [a_j, a_j + m) of every series sequence b uses, bit for bit, over relative
    knots; descriptors re-pointed, scales untouched."""
    from pulser_amd.simulation import QutipEmulator
    from pulser_amd.terms import DESC_DTYPE, DeviceTables

    rng = np.random.default_rng(0)
    B, n, K, m, n_ser = 2, 3, 41, 4, 5
    tk = np.arange(K + 1) * 1e-3 + 0.25
    pp = rng.normal(size=(n_ser, K, 4)) + 1j * rng.normal(size=(n_ser, K, 4))
    desc = np.zeros((B, n), dtype=DESC_DTYPE)
    desc["drive_series"] = rng.integers(-1, n_ser, size=(B, n))
    desc["det_series"] = rng.integers(-1, n_ser, size=(B, n))
    desc["off_series"] = -1
    desc["drive_scale"] = rng.normal(size=(B, n))
    tables = DeviceTables(n_qubits=n, batch=B, tknots=tk, pp=pp, desc=desc, interaction=rng.normal(size=(B, n, n)),
                          dissipator=None, series_knots=[])
    J = K // m
    anchors = np.arange(J + 1) * m
    wt = QutipEmulator._window_tables(tables, anchors, m)
    assert wt.batch == B * J and wt.pp.shape == (n_ser * J, m, 4) and wt.desc.shape == (B * J, n)
    assert np.allclose(wt.tknots, np.arange(m + 1) * 1e-3, rtol=0, atol=1e-15)
    assert wt.interaction.shape == (B * J, n, n)
    for b in range(B):
        for j in range(J):
            e = b * J + j
            assert np.array_equal(wt.interaction[e], tables.interaction[b])
            for k in range(n):
                for f in ("drive_series", "det_series", "off_series"):
                    sid, wid = int(desc[b, k][f]), int(wt.desc[e, k][f])
                    if sid < 0:
                        assert wid == -1
                    else:
                        assert np.array_equal(wt.pp[wid], pp[sid, anchors[j]: anchors[j] + m])
                assert wt.desc[e, k]["drive_scale"] == desc[b, k]["drive_scale"]
    assert tables.batch == B and tables.pp is pp  # the full tables are untouched


def test_window_knots_variable_falls_back_to_the_default_with_a_warning():
    """PULSER_AMD_WINDOW_KNOTS (read once, at import): an integer >= 2 is taken as it is; anything else gives the default
    32 and one warning naming the variable and the value (0 used to end in a ZeroDivisionError in _window_plan)."""
    import subprocess
    import sys

    code = (
        "import sys, warnings; sys.path.insert(0, sys.argv[1])\n"
        "with warnings.catch_warnings(record=True) as w:\n"
        "    warnings.simplefilter('always')\n"
        "    from pulser_amd.simulation import QutipEmulator\n"
        "msgs = [str(x.message) for x in w if 'PULSER_AMD_WINDOW_KNOTS' in str(x.message)]\n"
        "print(QutipEmulator._WINDOW_KNOTS, len(msgs), msgs[0] if msgs else '', sep='|')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = {"0": 32, "-4": 32, "abc": 32, "16": 16}
    procs = {v: subprocess.Popen([sys.executable, "-c", code, root], stdout=subprocess.PIPE, text=True,
                                 env={**os.environ, "PULSER_AMD_WINDOW_KNOTS": v}) for v in cases}
    for v, want in cases.items():
        out, _ = procs[v].communicate(timeout=300)
        assert procs[v].returncode == 0, v
        knots, n_warn, msg = out.strip().split("|", 2)
        assert int(knots) == want, (v, out)
        if want == 16:
            assert int(n_warn) == 0, (v, out)
        else:
            assert int(n_warn) == 1 and repr(v) in msg, (v, out)

"""CPU: the host side of ``Fidelity`` / ``Expectation`` over quantum-jump ensembles (``run(mc_ensemble=True,
mc_ensemble_targets=..., mc_ensemble_operators=...)``) - ``EnsembleState`` carrying the four arrays, the running sums
of ``_EnsembleSums`` against NumPy, the validation of the two options, the predicate and the option hand-over of
``QutipBackendV2.mc_ensemble``, and the operator matching of ``SimulationResults.expect``.

Bounds of the ``_EnsembleSums`` check (u = 2^-53, n trajectories, the per-trajectory numbers given exactly):
 * a mean of n float64 numbers, summed in any order and divided once: (n - 1) u + u of sum |v_b| / n; the fidelity
   terms v_b = (Re z_b)^2 + (Im z_b)^2 are formed with three roundings, 2 u v_b to first order: (n + 2) u mean |v_b|
   for both (the figure the GPU tests use after the kernel's own term).
 * a variance by the sum-of-squares formula, (sum v^2 - n mean^2) / (n - 1): the rounding of sum v^2 and of n mean^2
   at (n + 8) u sum v_b^2, plus sum 2 |v_b| dv_b with dv_b = 2 u v_b for the fidelity terms (0 for the parts of e_b,
   which are given), all over n - 1.  The code hands out the standard error sqrt(var / n): getting var back from it
   (the division, the root, the square and the product taken here, one rounding each) adds 4 u var.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import load_fixture, with_anneal_samples
from test_host_logic import _inputs_from_problem

from pulser_amd import NoiseModel, QutipEmulator, Solver
from pulser_amd.backend import (BitStrings, Expectation, Fidelity, Occupation, QutipBackendV2, QutipConfig, RydOperator,
                                RydState, _mc_ensemble_route, _overlap_form)
from pulser_amd.results import CoherentResults, EnsembleState, StateResult, operator_key
from pulser_amd.simulation import _EnsembleSums

LD = np.longdouble
U53 = 2.0 ** -53
N = 4
D = 16
QIDS = tuple(f"q{k}" for k in range(N))


def _state(ntraj=7, **kw):
    return EnsembleState(np.full(D, ntraj / D), ntraj, occupation=np.full(N, 0.5), correlation=np.full((N, N), 0.25),
                         energy=1.5, energy2=4.0, norm2=1.0, occupation_stderr=np.full(N, 0.1), **kw)


def _sigma_x_sum(n=N):
    sx = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
    out = sp.csr_matrix((2**n, 2**n))
    for q in range(n):
        out = out + sp.kron(sp.kron(sp.identity(2**q), sx), sp.identity(2**(n - q - 1)))
    return out.tocsr()


# ---------------------------------------------------------------------------------------------------------------------
# EnsembleState
# ---------------------------------------------------------------------------------------------------------------------
def test_ensemble_state_has_empty_arrays_when_nothing_was_registered():
    st = _state()
    assert st.fidelity.shape == st.fidelity_stderr.shape == st.expectation.shape == st.expectation_stderr.shape == (0,)
    assert st.fidelity.dtype == st.fidelity_stderr.dtype == st.expectation_stderr.dtype == np.float64
    assert st.expectation.dtype == np.complex128 and st.operators == ()


def test_ensemble_state_carries_the_four_arrays_in_registration_order():
    keys = [operator_key(_sigma_x_sum()), operator_key(np.diag(np.arange(D, dtype=float)))]
    st = _state(fidelity=[0.25, 1.0, 0.0], fidelity_stderr=[0.01, 0.0, 0.0], expectation=[0.5 - 0.25j, 3.0],
                expectation_stderr=[0.02, 0.03], operators=keys)
    assert st.fidelity.tolist() == [0.25, 1.0, 0.0] and st.fidelity_stderr.tolist() == [0.01, 0.0, 0.0]
    assert st.expectation.tolist() == [0.5 - 0.25j, 3.0] and st.expectation_stderr.tolist() == [0.02, 0.03]
    assert st.fidelity.dtype == np.float64 and st.expectation.dtype == np.complex128
    assert st.registered(keys[1]) == 1 and st.registered(operator_key(2 * _sigma_x_sum())) is None
    with pytest.raises(ValueError):
        _state(fidelity=[0.5], fidelity_stderr=[])
    with pytest.raises(ValueError):
        _state(expectation=[0.5], expectation_stderr=[0.1])  # no operator behind the value
    with pytest.raises(NotImplementedError, match="mc_ensemble_targets.*mc_ensemble_operators"):
        st.overlap(np.ones(D))
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        st.overlap(np.ones(D))


# ---------------------------------------------------------------------------------------------------------------------
# _EnsembleSums
# ---------------------------------------------------------------------------------------------------------------------
def _rows(n_t, n_b):
    """What ``observe_many`` returns for ``n_t`` times and ``n_b`` trajectories (the values do not matter here)."""
    return {"norm2": np.ones((n_t, n_b)), "occupation": np.full((n_t, n_b, N), 0.5),
            "correlation": np.full((n_t, n_b, N, N), 0.25), "energy": np.ones((n_t, n_b)), "energy2": np.ones((n_t, n_b))}


def _fed(z, e, z0, e0, chunks):
    """``_EnsembleSums`` fed the first time with weight n and the other times in ``chunks`` of trajectories."""
    n_t, n = z.shape[0] + 1, z.shape[1]
    keys = [operator_key(sp.csr_matrix(([float(k + 1)], ([0], [1])), shape=(D, D))) for k in range(e.shape[2])]
    sums = _EnsembleSums(n_t, N, n_targets=z.shape[2], operators=keys)
    sums.add(_rows(1, 1), slice(0, 1), n)
    sums.add_overlaps(z0[None, None], e0[None, None], slice(0, 1), n)
    lo = 0
    for b in chunks:
        sums.add(_rows(n_t - 1, b), slice(1, None))
        sums.add_overlaps(z[:, lo:lo + b], e[:, lo:lo + b], slice(1, None))
        lo += b
    assert lo == n
    return sums.states(np.full((n_t, D), n / D), n), keys


def test_sums_in_two_unequal_chunks_equal_numpy_within_the_bound():
    rng = np.random.default_rng(5)
    n, n_t, F, K = 37, 4, 3, 2
    z = (rng.normal(size=(n_t - 1, n, F)) + 1j * rng.normal(size=(n_t - 1, n, F))) / 2
    e = rng.normal(size=(n_t - 1, n, K)) * 3 + 1j * rng.normal(size=(n_t - 1, n, K))
    z0 = np.array([1.0, 0.6 - 0.3j, 0.0])
    e0 = np.array([0.5 + 0.0j, -2.0 + 1.5j])
    states, keys = _fed(z, e, z0, e0, (29, 8))
    assert len(states) == n_t and all(st.operators == tuple(keys) for st in states)
    # the first evaluation time: the initial ket with weight n, no spread
    st = states[0]
    p0 = z0.real.astype(LD) ** 2 + z0.imag.astype(LD) ** 2
    assert np.all(np.abs(st.fidelity - p0) <= (n + 2) * U53 * p0) and st.fidelity[0] == 1.0 and st.fidelity[2] == 0.0
    assert np.all(np.abs(st.expectation.real - e0.real) <= (n + 2) * U53 * np.abs(e0))
    assert np.all(np.abs(st.expectation.imag - e0.imag) <= (n + 2) * U53 * np.abs(e0))
    assert np.all(st.fidelity_stderr == 0) and np.all(st.expectation_stderr == 0)
    worst = np.zeros(4)
    for i in range(1, n_t):
        st = states[i]
        p = z[i - 1].real.astype(LD) ** 2 + z[i - 1].imag.astype(LD) ** 2  # [n, F]
        err = np.abs(st.fidelity.astype(LD) - p.mean(axis=0, dtype=LD))
        bound = (n + 2) * U53 * p.mean(axis=0, dtype=LD)
        worst[0] = max(worst[0], float(np.max(err / bound)))
        assert np.all(err <= bound)
        var = (st.fidelity_stderr.astype(LD) ** 2) * n
        b_var = ((n + 8) * U53 * (p ** 2).sum(axis=0) + (2 * p * 2 * U53 * p).sum(axis=0)) / (n - 1)
        ref = np.var(p, axis=0, ddof=1)
        err = np.abs(var - ref)
        worst[1] = max(worst[1], float(np.max(err / (b_var + 4 * U53 * ref))))
        assert np.all(ref > 1e-6) and np.all(err <= b_var + 4 * U53 * ref)  # (+ the sqrt and the square taken here)
        ex = e[i - 1]
        scale = np.abs(ex).mean(axis=0, dtype=LD)
        for part in (np.real, np.imag):
            err = np.abs(part(st.expectation).astype(LD) - part(ex).astype(LD).mean(axis=0, dtype=LD))
            worst[2] = max(worst[2], float(np.max(err / ((n + 2) * U53 * scale))))
            assert np.all(err <= (n + 2) * U53 * scale)
        re, im = ex.real.astype(LD), ex.imag.astype(LD)
        ref = np.var(re, axis=0, ddof=1) + np.var(im, axis=0, ddof=1)
        b_var = (n + 8) * U53 * ((re ** 2).sum(axis=0) + (im ** 2).sum(axis=0)) / (n - 1)
        err = np.abs((st.expectation_stderr.astype(LD) ** 2) * n - ref)
        worst[3] = max(worst[3], float(np.max(err / (b_var + 4 * U53 * ref))))
        assert np.all(ref > 1e-6) and np.all(err <= b_var + 4 * U53 * ref)
    print("RATIO _EnsembleSums (fidelity, its variance, expectation, its variance):", " ".join(f"{v:.3e}" for v in worst))


def test_one_trajectory_has_no_standard_error_and_nothing_registered_gives_empty_arrays():
    rng = np.random.default_rng(6)
    z = rng.normal(size=(2, 1, 2)) + 1j * rng.normal(size=(2, 1, 2))
    e = rng.normal(size=(2, 1, 1)) + 1j * rng.normal(size=(2, 1, 1))
    states, _ = _fed(z, e, np.array([1.0, 0.5j]), np.array([0.25 + 0j]), (1,))
    for i, st in enumerate(states):
        assert np.all(np.isnan(st.fidelity_stderr)) and np.all(np.isnan(st.expectation_stderr))
        assert st.fidelity.shape == (2,) and st.expectation.shape == (1,)
    assert np.array_equal(states[1].expectation, e[0, 0])
    assert np.array_equal(states[2].fidelity, z[1, 0].real ** 2 + z[1, 0].imag ** 2)
    sums = _EnsembleSums(2, N)
    sums.add(_rows(1, 1), slice(0, 1), 3)
    sums.add(_rows(1, 3), slice(1, None))
    for st in sums.states(np.full((2, D), 3 / D), 3):
        assert st.fidelity.shape == st.expectation.shape == st.fidelity_stderr.shape == (0,) and st.operators == ()


# ---------------------------------------------------------------------------------------------------------------------
# the options
# ---------------------------------------------------------------------------------------------------------------------
NOISE = dict(dephasing_rate=0.3, relaxation_rate=0.2)


def _tri4_inputs():
    prob, _ = load_fixture("cfg3_tri4_dephasing.npz")
    return _inputs_from_problem(with_anneal_samples(prob), "ground-rydberg")


def _emulator():
    return QutipEmulator(_tri4_inputs(), noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=12,
                         evaluation_times="Minimal")


def test_options_are_normalised_to_kets_and_csr_matrices():
    emu = _emulator()
    ket = np.arange(D) + 1j
    targets, ops = emu._ensemble_observables({"mc_ensemble_targets": [ket, ket.reshape(D, 1) * 2],
                                              "mc_ensemble_operators": [_sigma_x_sum(), np.eye(D)]})
    assert targets.shape == (2, D) and targets.dtype == np.complex128
    assert np.array_equal(targets[0], ket) and np.array_equal(targets[1], 2 * ket)
    assert [m.shape for m in ops] == [(D, D)] * 2 and all(sp.issparse(m) and m.dtype == np.complex128 for m in ops)
    assert ops[0].nnz == N * D and ops[1].nnz == D
    targets, ops = emu._ensemble_observables({"mc_ensemble_targets": np.stack([ket, ket])})  # [F, D]
    assert targets.shape == (2, D) and ops == []
    targets, ops = emu._ensemble_observables({})
    assert targets.shape == (0, D) and ops == []


@pytest.mark.parametrize("options,message", [
    ({"mc_ensemble_targets": [np.eye(D)]}, "default route"),  # a mixed state
    ({"mc_ensemble_targets": [np.ones(D), np.ones(D - 1)]}, r"mc_ensemble_targets\[1\]"),
    ({"mc_ensemble_targets": [np.ones((1, D))]}, r"mc_ensemble_targets\[0\]"),  # a bra
    ({"mc_ensemble_targets": [np.array(["a"] * D)]}, "not numeric"),
    ({"mc_ensemble_operators": [np.eye(D - 1)]}, r"mc_ensemble_operators\[0\]"),
    ({"mc_ensemble_operators": [np.eye(D), sp.identity(2 * D).tocsr()]}, r"mc_ensemble_operators\[1\]"),
    ({"mc_ensemble_operators": [np.ones((D, 2 * D))]}, r"mc_ensemble_operators\[0\]"),
    ({"mc_ensemble_operators": [np.full((D, D), "a")]}, "not numeric"),
], ids=["matrix", "length", "bra", "text", "small", "large", "rectangular", "text-operator"])
def test_invalid_options_raise_before_anything_is_solved(options, message, monkeypatch):
    emu = _emulator()
    monkeypatch.setattr(emu, "_solve_batch", lambda *a, **kw: pytest.fail("the solve was reached"))
    with pytest.raises(ValueError, match=message):
        emu._validate_options(dict(options))
    for route in ({"mc_ensemble": True}, {}):  # (raised whether or not the run would use them)
        with pytest.warns(DeprecationWarning), pytest.raises(ValueError, match=message):
            emu.run(**route, **options)


def test_run_docstring_documents_the_options():
    doc = QutipEmulator.run.__doc__
    assert "mc_ensemble_targets" in doc and "mc_ensemble_operators" in doc and "fidelity_stderr" in doc


# ---------------------------------------------------------------------------------------------------------------------
# the V2 backend
# ---------------------------------------------------------------------------------------------------------------------
DETERMINISTIC = dict(noise_model=NoiseModel(**NOISE), solver=Solver.MCSOLVER, n_trajectories=12)
EIG = ("r", "g")


def _ket_target():
    return RydState.from_state_amplitudes(eigenstates=EIG, amplitudes={"rgrg": 0.6, "gggg": 0.8j})


def _sim(cfg):
    return QutipBackendV2(_tri4_inputs(), config=cfg)._sim_obj


def _route(observables, **kw):
    cfg = QutipConfig(observables=observables, **{**DETERMINISTIC, **kw})
    return _mc_ensemble_route(_sim(cfg), cfg, ket_observables=True)


def test_predicate_admits_ket_fidelity_and_expectation_themselves():
    op = RydOperator(_sigma_x_sum(), eigenstates=EIG)
    assert _route([Fidelity(_ket_target())]) is True
    assert _route([Expectation(op)]) is True
    assert _route([Expectation(np.eye(D))]) is True
    assert _route([Fidelity(_ket_target()), Expectation(op), Expectation(np.eye(D), tag_suffix="b"), Occupation(),
                   BitStrings(num_shots=5)]) is True
    # the one classifier: what the predicate admits is what _overlap_form calls "ket" / "op" at the run's dimension
    assert _overlap_form(Fidelity(_ket_target()), EIG, D, False) == "ket"
    assert _overlap_form(Expectation(op), EIG, D, False) == "op"


def test_predicate_keeps_the_default_route_for_everything_else():
    mixed = RydState(np.eye(D) / D, eigenstates=EIG)
    assert _overlap_form(Fidelity(mixed), EIG, D, True) == "dm" and _route([Fidelity(mixed)]) is False

    class MyFidelity(Fidelity):  # a subclass may read anything of the state
        pass

    class MyExpectation(Expectation):
        pass

    assert _route([MyFidelity(_ket_target())]) is False
    assert _route([MyExpectation(np.eye(D))]) is False
    # other eigenstates (the same set in another order, another set) and another size
    swapped = RydState.from_state_amplitudes(eigenstates=("g", "r"), amplitudes={"gggg": 1.0})
    digital = RydState.from_state_amplitudes(eigenstates=("g", "h"), amplitudes={"gggg": 1.0})
    small = RydState.from_state_amplitudes(eigenstates=EIG, amplitudes={"ggg": 1.0})
    for target in (swapped, digital, small):
        assert _route([Fidelity(target)]) is False
    assert _route([Expectation(RydOperator(_sigma_x_sum(), eigenstates=("g", "r")))]) is False
    assert _route([Expectation(RydOperator(_sigma_x_sum(3), eigenstates=EIG))]) is False
    assert _route([Expectation(np.eye(D // 2))]) is False
    assert _route([Expectation(np.ones((D, D, 1)))]) is False
    # a callback reads the state
    assert _route([Fidelity(_ket_target())], callbacks=[lambda **kw: None]) is False
    # without collapse operators there are no jumps
    cfg = QutipConfig(observables=[Fidelity(_ket_target())], solver=Solver.MCSOLVER)
    assert _mc_ensemble_route(_sim(cfg), cfg, ket_observables=True) is False


class _StubEngine:
    def stats(self):
        return {}

    def close(self):
        pass


@pytest.mark.parametrize("mixed", [False, True])
def test_backend_registers_the_targets_and_operators_with_the_solve(mixed, monkeypatch):
    from pulser_amd import engine

    stub = _StubEngine()
    monkeypatch.setattr(engine.Engine, "from_problems", classmethod(lambda cls, problems, mode=None, **kw: stub))
    seen = {}

    class _Solved(Exception):
        pass

    def run(self, progress_bar=False, print_progress=False, **options):
        seen.update(options)
        raise _Solved

    monkeypatch.setattr(QutipEmulator, "run", run)
    op = RydOperator(_sigma_x_sum(), eigenstates=EIG)
    dense = np.diag(np.arange(D, dtype=float))
    dense[0, 3] = 2.0
    target = RydState(np.eye(D) / D, eigenstates=EIG) if mixed else _ket_target()
    cfg = QutipConfig(observables=[Occupation(), Expectation(op), Fidelity(target), Expectation(dense, tag_suffix="b")],
                      **DETERMINISTIC)
    backend = QutipBackendV2(_tri4_inputs(), config=cfg)
    backend.mc_ensemble = True
    with pytest.raises(_Solved):
        backend.run()
    if mixed:  # the default route, nothing handed over
        assert not any(k.startswith("mc_ensemble") for k in seen)
        return
    assert seen.get("mc_ensemble") is True and seen.get("mc_ensemble_observer") is stub
    assert len(seen["mc_ensemble_targets"]) == 1
    assert np.array_equal(seen["mc_ensemble_targets"][0], np.asarray(target.to_qobj()).reshape(-1))
    assert len(seen["mc_ensemble_operators"]) == 2 and seen["mc_ensemble_operators"][1] is dense
    assert (sp.csr_matrix(seen["mc_ensemble_operators"][0]) != _sigma_x_sum()).nnz == 0


def test_state_around_an_ensemble_returns_the_seeded_values():
    fid, exp = Fidelity(_ket_target()), Expectation(np.eye(D))
    state = RydState(_state(), eigenstates=EIG)
    with pytest.raises(NotImplementedError):  # unseeded: the matrix would be needed
        fid.apply(state=state)
    state.seed(fid, 0.75)
    state.seed(exp, 0.5 - 0.25j)
    assert fid.apply(state=state) == 0.75 and exp.apply(state=state) == 0.5 - 0.25j
    other = RydState(_state(), eigenstates=EIG)  # (seeds belong to one state)
    with pytest.raises(NotImplementedError):
        exp.apply(state=other)


# ---------------------------------------------------------------------------------------------------------------------
# SimulationResults.expect
# ---------------------------------------------------------------------------------------------------------------------
def _results(operators, values):
    keys = [operator_key(m) for m in operators]
    states = [_state(expectation=v, expectation_stderr=np.zeros(len(v)), operators=keys) for v in values]
    rs = [StateResult(QIDS, "ground-rydberg", s, True, evaluation_time=t) for s, t in zip(states, (0.0, 1.0))]
    return CoherentResults(rs, N, "ground-rydberg", np.array([0.0, 0.1]), "ground-rydberg", None)


def test_expect_serves_a_registered_operator_by_its_non_zeros():
    sx = _sigma_x_sum()
    hop = sp.csr_matrix(([1.0], ([4], [8])), shape=(D, D))  # not Hermitian
    res = _results([sx, hop], [[0.5 + 1e-3j, 0.1 - 0.2j], [-1.5 + 0j, 0.3 + 0.4j]])
    # an equal-non-zeros rebuild in every accepted form: dense, another sparse format, explicit zeros stored
    padded = sx.tolil()
    padded[0, 0] = 0.0
    with_zero = sp.csr_matrix((np.append(sx.tocoo().data, 0.0), (np.append(sx.tocoo().row, 5), np.append(sx.tocoo().col, 5))),
                              shape=(D, D))
    for rebuilt in (sx.toarray(), sx.tocoo(), _sigma_x_sum(), padded, with_zero, sx.astype(complex)):
        got = res.expect([rebuilt])[0]
        assert got.dtype == np.float64 and got.tolist() == [0.5, -1.5]  # Hermitian: the real part
    got = res.expect([hop.toarray(), sx])
    assert got[0].dtype == np.complex128 and got[0].tolist() == [0.1 - 0.2j, 0.3 + 0.4j] and got[1].tolist() == [0.5, -1.5]
    # one entry differs, one entry more, one entry fewer, another operator
    one = sx.toarray()
    one[0, 1] = 1.0 + 1e-15
    more = sx.toarray()
    more[0, 3] = more[3, 0] = 1.0
    fewer = sx.toarray()
    fewer[0, 1] = fewer[1, 0] = 0.0
    for other in (one, more, fewer, hop.T.tocsr(), 2 * sx):
        with pytest.raises(NotImplementedError, match="mc_ensemble_operators"):
            res.expect([other])
    with pytest.raises(NotImplementedError, match="mc_ensemble=False"):
        res.expect([one])
    # a diagonal operator needs no registration
    assert res.expect([np.diag(np.arange(D, dtype=float))])[0].tolist() == [7.5, 7.5]  # (1/16 per entry: exact)

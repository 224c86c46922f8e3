"""-m gpu: the Lanczos exponential (``method="krylov"``, k_krylov.hpp / host_krylov.hpp) against an exact propagator.

For a Hamiltonian that is constant in time both exponentials of every CF4 step are exp(-i h H / 2) exactly, so the whole
run is exp(-i H t): the only errors left are the truncation of the Lanczos process and rounding, and the bar is
``lanczos_ref.bar`` = |psi| n_exp (3 tol + floor) on the 2-norm of every batch entry's error (derivation there).  The
reference is a dense eigendecomposition (up to 10 atoms) or scipy's expm_multiply (13, 14 atoms) of the oracle's H
(tests/test_lanczos_ref.py checks the reference itself).

Both iterations of exp_step_krylov are run and told apart by their launch count: every exponential launches 3 kernels
before its loop and 2 after it; an iteration is the generator (one launch per pass) plus k_kry_update_fused (fused: one
k_apply pass that is not a 2^14 register tile) or plus k_kry_reset, k_kry_dot, k_kry_update and k_kry_normalize (every
other plan).  ``n_applications`` counts the iterations, so

    n_launches == 5 n_exp + n_applications (passes + 1)      fused (passes == 1)
    n_launches == 5 n_exp + n_applications (passes + 4)      five-launch

Measured figures: profiles/lanczos_edges.md."""
from __future__ import annotations

import numpy as np
import pytest

import lanczos_ref as L
from helpers import local_problem, rand_state

pytestmark = pytest.mark.gpu

TOL = 1e-12
FUSED, FIVE = "fused", "five-launch"


def _run(probs, kets, t0, t1, tol=TOL, tile_bits=0, path=None, method="krylov", times=None):
    """One engine, one evolve (or solve through ``times``): (final kets [B, D], stored kets or None, stats)."""
    from pulser_amd.engine import Engine

    with Engine.from_problems(probs, mode="sesolve", tile_bits=tile_bits) as eng:
        if path:
            eng.set_path(False, **path)
        st = eng.new_state(np.asarray(kets))
        snaps = None
        if times is None:
            eng.evolve(st, t0, t1, method=method, tol=tol)
        else:
            snaps = eng.solve(st, times, method=method, tol=tol).cpu().numpy()
        import torch

        assert bool(torch.isfinite(torch.view_as_real(st)).all())
        return st.cpu().numpy(), snaps, eng.stats()


def _assert_iteration(s, which):
    n_exp = 2 * s["n_steps"]
    per_iteration = s["passes"] + (1 if which == FUSED else 4)
    assert which == FIVE or s["passes"] == 1
    assert s["n_launches"] == 5 * n_exp + s["n_applications"] * per_iteration, (which, s)


def _reference(prob, t, psi):
    return (L.exact_propagate if int(prob["n_qudits"]) <= 10 else L.sparse_propagate)(prob, t, psi)


def _judge(label, got, ref, norm0, n_exp, tol=TOL, floor_only=False):
    """Print error / bar of one ket, then assert."""
    err = float(np.linalg.norm(got - ref))
    bound = norm0 * n_exp * L.FLOOR if floor_only else L.bar(norm0, n_exp, tol)
    print(f"{label}: error {err:.2e} / bar {bound:.2e} = {err / bound if bound > 0 else 0.0:.3f}")
    assert err <= bound, (label, err, bound)
    return err / bound if bound > 0 else 0.0


# ------------------------------------------------------------------ A. every generator plan the exponential can sit on
PLANS = [
    # n, batch, tile_bits, set_path, passes (None: at least 2), iteration
    pytest.param(3, 1, 0, None, 1, FUSED, id="3-one-tile-partly-filled-workgroup"),
    pytest.param(8, 1, 0, None, 1, FUSED, id="8-one-tile"),
    pytest.param(9, 1, 5, {"force_single_pass": True}, 1, FUSED, id="9-single-launch-partner-reads"),
    pytest.param(9, 1, 4, None, None, FIVE, id="9-multi-pass"),
    pytest.param(13, 2, 0, None, 1, FUSED, id="13x2-single-launch-auto-tile"),
    pytest.param(14, 1, 0, None, 1, FUSED, id="14-single-launch"),
    pytest.param(14, 1, 0, {"force_tile14": True}, 1, FIVE, id="14-register-tile"),
]


@pytest.mark.parametrize("n, batch, tile_bits, path, passes, which", PLANS)
def test_every_generator_plan_against_the_exact_propagator(n, batch, tile_bits, path, passes, which):
    """Interacting chain at 7 um, per-atom complex constant drives, a seeded random unnormalised ket per entry."""
    probs = [L.plan_problem(n, s) for s in range(batch)]
    kets = np.stack([(0.37 + 2.1 * s) * rand_state(2**n, 20 + s) for s in range(batch)])
    out, _, s = _run(probs, kets, 0.0, L.T1, tile_bits=tile_bits, path=path)
    assert (s["passes"] == passes) if passes else (s["passes"] >= 2), s
    _assert_iteration(s, which)
    assert s["norm_bound"] * 0.004 / 2 <= 6.0  # the premise of the bar: four-knot steps are the longest
    for b in range(batch):
        _judge(f"plan n={n} entry {b} [{which}, {s['passes']} passes, m={s['last_order']}, {s['n_launches']} launches, "
               f"{s['n_applications']} applications, {s['n_steps']} steps]",
               out[b], _reference(probs[b], L.T1, kets[b]), np.linalg.norm(kets[b]), 2 * s["n_steps"])


# ------------------------------------------------------------------------------------------------------ B. batch edges
B_BATCH = 130  # k_kry_reset runs 128-thread blocks: the second block has two live threads
B_ZERO, B_BASIS = 7, 11


@pytest.mark.parametrize("tile_bits, which", [(0, FUSED), (3, FIVE)])
def test_batch_of_130_entries_with_their_own_norms_a_zero_vector_and_a_basis_state(tile_bits, which):
    """Per-entry alpha, beta, sq, acc and coef strides: three distinct 6-atom problems cycled over 130 entries, every entry
    with its own random ket and a norm between 1e-3 and 1e3, one zero vector, one basis state; every entry is judged
    against its own norm."""
    three = L.batch_problems()
    probs = [three[b % 3] for b in range(B_BATCH)]
    norms = 10.0 ** np.linspace(-3, 3, B_BATCH)[np.random.default_rng(5).permutation(B_BATCH)]
    kets = np.stack([norms[b] * rand_state(64, 500 + b) for b in range(B_BATCH)])
    kets[B_ZERO] = 0.0
    kets[B_BASIS] = 0.0
    kets[B_BASIS, 37] = 1.0
    out, _, s = _run(probs, kets, 0.0, L.T1, tile_bits=tile_bits)
    _assert_iteration(s, which)
    assert np.all(np.isfinite(out.view(float)))
    assert np.all(out[B_ZERO] == 0.0)  # exactly
    worst, at = 0.0, -1
    for b in range(B_BATCH):
        ref = L.exact_propagate(three[b % 3], L.T1, kets[b])
        n0 = float(np.linalg.norm(kets[b]))
        ratio = float(np.linalg.norm(out[b] - ref)) / L.bar(n0, 2 * s["n_steps"], TOL) if n0 > 0 else 0.0
        if ratio > worst:
            worst, at = ratio, b
    print(f"batch of {B_BATCH} [{which}, {s['passes']} passes, m={s['last_order']}, {s['n_launches']} launches]: worst "
          f"error / bar = {worst:.3f} at entry {at} (norm {np.linalg.norm(kets[at]):.2e}); basis-state entry "
          f"{np.linalg.norm(out[B_BASIS] - L.exact_propagate(three[B_BASIS % 3], L.T1, kets[B_BASIS])) / L.bar(1.0, 2 * s['n_steps'], TOL):.3f}")
    assert worst <= 1.0, (worst, at)


# ------------------------------------------------------------------------------------ C. breakdown of the recurrence
ITERATIONS_SMALL = [pytest.param(0, FUSED, id=FUSED), pytest.param(3, FIVE, id=FIVE)]


@pytest.mark.parametrize("tile_bits, which", ITERATIONS_SMALL)
def test_exact_breakdown_at_the_first_vector_of_a_diagonal_hamiltonian(tile_bits, which):
    """Amplitude 0, non-zero detunings, interacting: every basis state is an eigenvector, u = 0 at j = 0 and nothing
    after it may produce a NaN.  From all-ground and from a (scaled) random basis state: e^{-i E t} times the start,
    within rounding (n_exp x floor)."""
    prob = L.diagonal_problem()
    D = 2 ** int(prob["n_qudits"])
    kets = np.zeros((2, D), complex)
    kets[0, D - 1] = 1.0
    k = int(np.random.default_rng(9).integers(1, D - 1))
    kets[1, k] = 2.5
    out, _, s = _run([prob, prob], kets, 0.0, L.T1, tile_bits=tile_bits)
    _assert_iteration(s, which)
    assert np.all(np.isfinite(out.view(float)))
    E = L.hamiltonian(prob).diagonal().real
    for b, idx in ((0, D - 1), (1, k)):
        ref = np.exp(-1j * E[idx] * L.T1) * kets[b]
        _judge(f"diagonal H, basis state {idx} [{which}, m={s['last_order']}]", out[b], ref, np.linalg.norm(kets[b]),
               2 * s["n_steps"], floor_only=True)


@pytest.mark.parametrize("tile_bits, which", ITERATIONS_SMALL)
def test_breakdown_inside_the_run_on_an_invariant_subspace(tile_bits, which):
    """4 atoms without interaction under one global real drive, from all-ground: the Krylov space is the 5-dimensional
    symmetric subspace, so beta_4 is rounding (3.8e-15 against beta_0..3 of 6 - 7 on the host) while the library asks
    for 7 vectors or more.  The five-launch iteration zeroes the vector below its 1e-14 threshold, the fused one carries
    on with normalised noise: both must meet the ordinary bar, against the eigendecomposition and against the product
    of exact single-atom propagators."""
    prob = L.symmetric_problem()
    t1 = 0.032  # eight four-knot steps: the last exponential has the full argument too
    ket = np.zeros((1, 16), complex)
    ket[0, 15] = 1.0
    out, _, s = _run([prob], ket, 0.0, t1, tile_bits=tile_bits)
    _assert_iteration(s, which)
    assert s["last_order"] >= 7, s
    _judge(f"invariant subspace vs eigh [{which}, m={s['last_order']}]", out[0], L.exact_propagate(prob, t1, ket[0]), 1.0,
           2 * s["n_steps"])
    _judge(f"invariant subspace vs single-atom product [{which}]", out[0], L.single_atom_product(prob, t1, 4), 1.0,
           2 * s["n_steps"])


@pytest.mark.parametrize("tile_bits, which", [pytest.param(0, FUSED, id=FUSED), pytest.param(4, FIVE, id=FIVE)])
def test_weak_drive_on_a_strong_diagonal_from_all_ground(tile_bits, which):
    """Near breakdown without reaching it: drives of 0.01 - 0.05 rad/us on a diagonal of 2 700 rad/us, from all-ground.
    |u|^2 / |w|^2 of the first iteration is 2e-10, below the 1e-8 at which k_kry_update_fused drops the cancelling
    formula |w|^2 - alpha^2 - beta^2 and scales by |w|: the next stored vector has a norm of 1e-5, and every later use of
    sq[] (the true beta, the coefficient of v_{j-1}, the tridiagonal matrix, the combination) must divide it out."""
    prob = L.weak_drive_problem()
    ket = np.zeros((1, 512), complex)
    ket[0, 511] = 1.3
    out, _, s = _run([prob], ket, 0.0, L.T1, tile_bits=tile_bits)
    _assert_iteration(s, which)
    assert s["norm_bound"] * 0.004 / 2 <= 6.0
    _judge(f"weak drive, all-ground [{which}, m={s['last_order']}]", out[0], L.exact_propagate(prob, L.T1, ket[0]), 1.3,
           2 * s["n_steps"])


# --------------------------------------------------------------------------------------- D. Krylov dimension edges
@pytest.mark.parametrize("tile_bits, which", [pytest.param(0, FUSED, id=FUSED), pytest.param(2, FIVE, id=FIVE)])
def test_tiny_argument_takes_two_basis_vectors(tile_bits, which):
    prob = L.tiny_step_problem()
    ket = 1.7 * rand_state(8, 31)[None, :]
    t0, t1 = 0.01, 0.01 + 1e-7
    out, _, s = _run([prob], ket, t0, t1, tile_bits=tile_bits)
    _assert_iteration(s, which)
    assert s["n_steps"] == 1 and s["last_order"] == 2 and s["n_applications"] == 4, s
    _judge(f"tiny argument [{which}, rho = {s['norm_bound'] * (t1 - t0) / 2:.1e}]", out[0],
           L.exact_propagate(prob, t1 - t0, ket[0]), 1.7, 2)


@pytest.mark.parametrize("tile_bits, which", [pytest.param(0, FUSED, id=FUSED), pytest.param(4, FIVE, id=FIVE)])
def test_large_argument_at_two_tolerances(tile_bits, which):
    """9 atoms at 4.5 um (about 650 rad/us between neighbours): a four-knot step has an argument of about 5, k_kry_small
    runs several sub-steps of its 30-term series.  tol = 1e-12 and 1e-8 each hold their own bar, and the looser run takes
    fewer basis vectors.  Two kets: a random one, and a superposition of the two ends of the spectrum with a global
    phase that is not real (the polynomial must hold over the whole interval; a Lanczos process with wrong diagonal
    coefficients still matches the first m - 1 moments and only shows there)."""
    prob = L.dense_chain_problem()
    kets = np.stack([0.8 * rand_state(512, 32), L.edge_superposition(9)])
    norms = np.linalg.norm(kets, axis=1)
    refs = [L.exact_propagate(prob, L.T1, k) for k in kets]
    orders = {}
    for tol in (1e-12, 1e-8):
        out, _, s = _run([prob, prob], kets, 0.0, L.T1, tol=tol, tile_bits=tile_bits)
        _assert_iteration(s, which)
        rho_mean, rho_max = s["norm_bound"] * (L.T1 / s["n_steps"]) / 2, s["norm_bound"] * 0.004 / 2
        assert rho_mean >= 3.0, s  # the longest step is at least the mean one: one exponential or more at rho >= 3
        assert rho_max <= 6.0, s   # the premise of the bar
        orders[tol] = s["last_order"]
        for b, name in enumerate(("random ket", "spectrum edges")):
            _judge(f"large argument, {name}, tol={tol:g} [{which}, rho <= {rho_max:.2f}, m={s['last_order']}, "
                   f"{s['n_steps']} steps]", out[b], refs[b], norms[b], 2 * s["n_steps"], tol=tol)
    assert orders[1e-12] >= 16 and orders[1e-8] < orders[1e-12], orders


# --------------------------------------------------------------------------------------------------- E. stored states
@pytest.mark.parametrize("tile_bits, which", [pytest.param(0, FUSED, id=FUSED), pytest.param(4, FIVE, id=FIVE)])
def test_stored_states_at_evaluation_times_that_cut_steps_short(tile_bits, which):
    """solve() with evaluation times inside knot intervals, one of them 0.5 ns after the previous: every stored state
    against the exact one at its time (the exponentials up to a stored time are at most those of the whole run)."""
    prob = L.plan_problem(9)
    ket = 1.3 * rand_state(512, 33)[None, :]
    times = [0.0, 0.011, 0.0115, 0.03]
    out, snaps, s = _run([prob], ket, None, None, tile_bits=tile_bits, times=times)
    _assert_iteration(s, which)
    assert np.array_equal(snaps[-1], out)
    for k, t in enumerate(times[1:]):
        _judge(f"stored state at {t} us [{which}, {s['n_steps']} steps]", snaps[k, 0], L.exact_propagate(prob, t, ket[0]),
               1.3, 2 * s["n_steps"])


# ----------------------------------------------------------------------------- F. time-dependent drives, same schedule
@pytest.mark.parametrize("tile_bits, which", [pytest.param(0, FUSED, id=FUSED), pytest.param(4, FIVE, id=FIVE)])
def test_time_dependent_drives_against_the_taylor_exponential_on_the_same_schedule(tile_bits, which):
    """Per-atom modulated complex drives: the schedule does not depend on the method, so the two runs compute the same
    CF4 exponentials and differ by their own truncations only."""
    prob = local_problem(9, duration=101)
    ket = 0.6 * rand_state(512, 34)[None, :]
    outs, stats = {}, {}
    for method in ("taylor", "krylov"):
        outs[method], _, stats[method] = _run([prob], ket, 0.0, L.T1, tile_bits=tile_bits, method=method)
    _assert_iteration(stats["krylov"], which)
    assert stats["taylor"]["n_steps"] == stats["krylov"]["n_steps"], stats
    n_exp = 2 * stats["krylov"]["n_steps"]
    # Lanczos: 3 tol + floor (lanczos_ref.bar).  Taylor: the remainder rho^(m+1) / (m+1)! is at most tol, times at most 2 for the
    # rest of the tail (rho <= (m + 2) / 2), and its own rounding floor
    bound = 0.6 * n_exp * (3 * TOL + 2 * TOL + 2 * L.FLOOR)
    err = float(np.linalg.norm(outs["taylor"][0] - outs["krylov"][0]))
    print(f"taylor vs krylov [{which}, {n_exp} exponentials]: difference {err:.2e} / bar {bound:.2e} = {err / bound:.3f}")
    assert err <= bound

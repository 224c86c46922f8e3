"""Two exact quantum-jump references for the two-level kernels, and the case table of the device tests
(tests/test_mcwf_ref.py, tests/test_gpu_mcwf_edges.py): NumPy / SciPy only.

Both follow the jump rule fixed in ``oracle/mcwf.py`` (Philox4x32-10 keyed by the seed, counter = jump index; the
threshold tested at the end of every step of the grid; candidates atom-major, operator-minor, the first index whose
cumulative weight exceeds ``r2 * total``; ``ref = |psi0|^2`` before the first jump) and both use a structure the kernels
know nothing about, so they stay exact and cheap where the full-space restatement (zvode on 2^N amplitudes, once per
step) takes minutes per trajectory:

A. :func:`product_trajectory` - driven, no interaction, product initial ket.  H_eff is a sum of one-atom terms and every
   collapse operator is local, so the ket stays a product of N one-atom kets for ever.  The no-jump step of atom ``a`` is
   a 2 x 2 propagator, integrated once per (atom, step) with the oracle's own one-atom H_eff (``qp.build_hamiltonian`` of
   the one-atom problem, ``mcwf.effective_rhs``, ``qp._zvode`` under ``qp.TIGHT``); norms and weights are products of
   one-atom numbers (kept in ``np.longdouble``), a jump replaces one factor: O(N) per step.  The 2^N ket is a chain of
   Kronecker products, formed at the evaluation times only.  Atom 0 is the highest bit.
B. :func:`diagonal_trajectory` - interacting, undriven, entangled.  H_eff(t) is diagonal: between jumps amplitude ``i`` is
   multiplied by ``exp(-i int E_i dt - Gamma_i h / 2)`` per step, with ``int E_i dt = sum_a n_a(i) (-int delta_a dt) +
   h U_i`` (``n_a`` = 1 where atom ``a`` is in ``r``; ``int delta_a dt`` the exact integral of the cubic spline the oracle
   builds for the samples) and ``Gamma_i`` the diagonal of ``sum C^dag C``.  A jump applies the 2 x 2 operator to one bit
   of the full vector: O(2^N) per step.

Each returns the normalised kets at the evaluation times, the jumps [(time, atom, operator)] and the two smallest
margins of the trajectory: ``min over steps |n2 - target ref| / ref`` (how close a threshold test came to going the
other way) and ``min over jumps and boundaries |cum_k - x| / total`` (how close a selection came to its neighbour).

What the references can and cannot see: A sees the drive (both drive models), the decay and the jump bookkeeping of a
product ket at any size, never an interaction or an entangled ket; B sees interaction, time-dependent detunings, decay
and jumps of an entangled, unnormalised ket, never a drive.  Driven and interacting trajectories above 3 atoms stay
with the kernel-against-kernel tests.

``python tests/mcwf_ref.py`` prints, per case of :data:`CASES`, the figures the conditions of tests/test_mcwf_ref.py are
about (jumps, margins, skipped seeds, coverage, CPU time).
"""
from __future__ import annotations

import functools
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root holds ``oracle`` and ``pulser_amd``
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulser_amd import problem as P

DURATION = 61
GRID = np.arange(DURATION) / 1000.0  # 60 one-nanosecond steps
EVAL = np.array([0.0, 0.02, 0.06])
MARGIN = 1e-6

KINDS = ("sigma_gr", "sigma_rr", "x", "y", "z")
# rates (squares of the coefficients) of test_quantum_jumps_on_the_split_operator_passes_match_the_taylor_path
STRONG_RATES = (6.0, 2 * 1.5, 2.0 / 4, 2.0 / 4, 2.0 / 4)
PAULIS = {
    "x": [(1, "sigma_gr"), (1, "sigma_rg")],
    "y": [(1j, "sigma_gr"), (-1j, "sigma_rg")],
    "z": [(1, "sigma_rr"), (-1, "sigma_gg")],
}
LD = np.longdouble
CLD = np.clongdouble


def collapse_ops(n, scale):
    """The strong rates times ``scale / n`` (a trajectory of n atoms then jumps about as often at every n)."""
    return [(float(np.sqrt(r * scale / n)), k) for r, k in zip(STRONG_RATES, KINDS)]


def blockade_spacing():
    return (P.C6_LEVEL70 / (4 * 2 * np.pi / 2)) ** (1 / 6)  # helpers.blockade_radius


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def problem_a(n, model, scale, seed):
    """Driven, no interaction.  ``model`` 0: per-atom complex drives (amplitude, detuning and phase all depend on time);
    1: one global real drive (phase 0) with a global detuning.  The waveforms are slow enough for the step-size rule of
    the library (host_sched.hpp: the curvature estimate, summed over the atoms) to take one CF4 step per sample
    interval at every size - the threshold is tested at the end of every step, so the references must walk the grid
    of the device."""
    rng = np.random.default_rng(seed)
    t = GRID
    zero = np.zeros(DURATION)
    coords = P.register_coords(P.square_rect(1, n), 7.0)
    prob = P.make_ising_problem(coords, {"amp": zero, "det": zero, "phase": zero})
    if model == 0:
        loc = {}
        for q in range(n):
            a, b, c = rng.uniform(2, 12, 3)
            loc[q] = {"amp": a * (1 + 0.3 * np.sin((2 + q % 5) * t + q)),
                      "det": b * np.cos(3 * t + q) - c,
                      "phase": 0.3 * q + 0.5 * np.sin(4 * t)}
        prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": loc}}
    else:
        a, b, c = rng.uniform(4, 12, 3)
        prob["samples"] = {"Global": {"ground-rydberg": {"amp": a * (1 + 0.3 * np.sin(5 * t)),
                                                         "det": b * np.cos(4 * t) - c, "phase": zero.copy()}},
                           "Local": {}}
    prob["interaction_matrix"] = np.zeros_like(prob["interaction_matrix"])
    prob["collapse_ops"] = collapse_ops(n, scale)
    prob["depolarizing_pauli_2ds"] = dict(PAULIS)
    return prob


def problem_b(n, scale, seed):
    """Undriven, interacting chain at the blockade spacing (12.6 rad/us between neighbours) with per-atom detunings that
    depend on time (slowly: see :func:`problem_a`)."""
    rng = np.random.default_rng(seed)
    t = GRID
    zero = np.zeros(DURATION)
    coords = P.register_coords(P.square_rect(1, n), blockade_spacing())
    prob = P.make_ising_problem(coords, {"amp": zero, "det": zero, "phase": zero})
    loc = {}
    for q in range(n):
        b, c, w = rng.uniform(2, 12, 3)
        loc[q] = {"amp": zero.copy(), "det": b * np.cos(0.5 * w * t + q) - c + 60.0 * t * (q % 3 - 1), "phase": zero.copy()}
    prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": loc}}
    prob["collapse_ops"] = collapse_ops(n, scale)
    prob["depolarizing_pauli_2ds"] = dict(PAULIS)
    return prob


def one_atom_problem(prob, a):
    """The problem of atom ``a`` alone: its own samples (and the global ones), no interaction."""
    one = dict(prob)
    one["n_qudits"] = 1
    one["qubit_ids"] = (prob["qubit_ids"][a],)
    one["coords"] = np.asarray(prob["coords"])[[a]]
    one["interaction_matrix"] = np.zeros((1, 1, 1))
    one["bad_atoms"] = np.zeros(1, dtype=bool)
    local = {}
    for basis, per in prob["samples"].get("Local", {}).items():
        if a in per:
            local[basis] = {0: per[a]}
    one["samples"] = {"Global": prob["samples"].get("Global", {}), "Local": local}
    return one


def local_collapse(prob):
    """The 2 x 2 collapse operators in the order of ``prob["collapse_ops"]`` (from the oracle's one-atom build)."""
    from oracle import qutip_path as qp

    return [np.asarray(c.toarray()) for c in qp.build_hamiltonian(one_atom_problem(prob, 0)).collapse]


# ---------------------------------------------------------------------------------------------------------------------
# A: product reference
# ---------------------------------------------------------------------------------------------------------------------
def one_atom_propagators(prob, step_times):
    """complex[n_steps, N, 2, 2]: the no-jump propagator of every atom over every step under its one-atom H_eff(t).
    Atoms whose one-atom problems are the same object-for-object (a global drive only) share one integration."""
    from oracle import mcwf, qutip_path as qp

    n = int(prob["n_qudits"])
    step_times = np.asarray(step_times, dtype=float)
    out = np.zeros((len(step_times) - 1, n, 2, 2), dtype=complex)
    shared = not any(prob["samples"].get("Local", {}).values())
    for a in range(n):
        if shared and a > 0:
            out[:, a] = out[:, 0]
            continue
        rhs1 = mcwf.effective_rhs(qp.build_hamiltonian(one_atom_problem(prob, a)))

        def rhs(t, y):
            return rhs1(t, y.reshape(2, 2)).reshape(-1)

        for i in range(len(step_times) - 1):
            y = qp._zvode(rhs, np.eye(2, dtype=complex).reshape(-1), step_times[i:i + 2], qp.TIGHT)[-1]
            out[i, a] = y.reshape(2, 2)
    return out


def kron_chain(factors):
    """The 2^N ket of N one-atom kets, atom 0 the highest bit; complex128."""
    out = np.ones(1, dtype=complex)
    for f in factors:
        out = np.kron(out, np.asarray(f, dtype=complex))
    return out


def product_trajectory(prob, factors0, step_times, eval_times, seed, props=None, form_kets=True, perturb=None):
    """One trajectory of reference A from the product ket of ``factors0`` (complex[N, 2], any norms).
    Returns (kets at eval_times - normalised, or the normalised factor lists with ``form_kets=False`` -, jumps, margins).
    ``perturb(atom, operator, weight)`` replaces a weight of the selection (the sensitivity check of
    tests/test_mcwf_ref.py: what a wrong weight on the device would do to the jump list)."""
    from oracle.mcwf import mc_uniforms

    n = int(prob["n_qudits"])
    step_times = np.asarray(step_times, dtype=float)
    eval_times = np.asarray(eval_times, dtype=float)
    if props is None:
        props = one_atom_propagators(prob, step_times)
    props = props.astype(CLD)
    cops = [c.astype(CLD) for c in local_collapse(prob)]
    phi = np.asarray(factors0).astype(CLD).reshape(n, 2).copy()

    def norms(x):
        return (x.real ** 2 + x.imag ** 2).sum(axis=-1)

    def emit():
        f = phi / np.sqrt(norms(phi))[:, None]
        return kron_chain(f) if form_kets else np.asarray(f, dtype=complex)

    ref = LD(np.prod(norms(phi)))
    count = 0
    target = LD(mc_uniforms(seed, 0)[0])
    jumps, out = [], []
    m_thr, m_sel = np.inf, np.inf
    ei = 0
    if abs(eval_times[0] - step_times[0]) < 1e-12:
        out.append(emit())
        ei = 1
    for i in range(len(step_times) - 1):
        t1 = step_times[i + 1]
        phi = np.einsum("aij,aj->ai", props[i], phi)
        na = norms(phi)
        n2 = LD(np.prod(na))
        m_thr = min(m_thr, float(abs(n2 - target * ref) / ref))
        if n2 <= target * ref:
            # weight of (atom a, operator k) = |C_k phi_a|^2 prod_{b != a} |phi_b|^2, atom-major / operator-minor
            rest = np.array([np.prod(np.delete(na, a)) for a in range(n)], dtype=LD)
            cand = []
            for a in range(n):
                for k, c in enumerate(cops):
                    v = c @ phi[a]
                    w = LD(norms(v)) * rest[a]
                    cand.append((a, k, v, w if perturb is None else LD(perturb(a, k, w))))
            total = sum(c[3] for c in cand)
            if total > 0:
                x = LD(mc_uniforms(seed, count)[1]) * total
                cum = LD(0)
                pick = None
                for c in cand:
                    cum += c[3]
                    m_sel = min(m_sel, float(abs(cum - x) / total))
                    if pick is None and c[3] > 0 and cum > x:
                        pick = c
                if pick is None:
                    pick = [c for c in cand if c[3] > 0][-1]
                phi = phi / np.sqrt(na)[:, None]
                phi[pick[0]] = pick[2] / np.sqrt(norms(pick[2]))
                jumps.append((float(t1), pick[0], pick[1]))
                count += 1
                target = LD(mc_uniforms(seed, count)[0])
                ref = LD(1)
        while ei < len(eval_times) and abs(eval_times[ei] - t1) < 1e-12:
            out.append(emit())
            ei += 1
    if ei != len(eval_times):
        raise ValueError("every evaluation time must be a point of the step grid")
    return out, jumps, (m_thr, m_sel)


# ---------------------------------------------------------------------------------------------------------------------
# B: diagonal reference
# ---------------------------------------------------------------------------------------------------------------------
def _in_r(n):
    """bool[N, 2^N]: atom a of basis state i is in local state 0 (= r); atom 0 is the highest bit."""
    idx = np.arange(1 << n)
    return np.array([((idx >> (n - 1 - a)) & 1) == 0 for a in range(n)])


def diagonal_factors(prob, step_times):
    """complex[n_steps, 2^N]: exp(-i int E_i dt - Gamma_i h / 2) of every step."""
    from scipy.interpolate import make_interp_spline

    from oracle import qutip_path as qp

    n = int(prob["n_qudits"])
    step_times = np.asarray(step_times, dtype=float)
    in_r = _in_r(n).astype(float)
    # static part: the interaction (sum_{a<b} U_ab n_a n_b) and the decay diagonal
    u = np.asarray(prob["interaction_matrix"], dtype=float)[-1]
    energy = np.zeros(1 << n)
    for a in range(n):
        for b in range(a + 1, n):
            energy += u[a, b] * in_r[a] * in_r[b]
    m = sum(c.conj().T @ c for c in local_collapse(prob))
    if abs(m[0, 1]) + abs(m[1, 0]) > 1e-14:
        raise ValueError("sum C^dag C is not diagonal")
    gamma = np.zeros(1 << n)
    for a in range(n):
        gamma += np.where(in_r[a] > 0, m[0, 0].real, m[1, 1].real)
    # detunings: the one-atom Hamiltonian's diagonal terms, c(t) op + h.c. with op = sigma_rr and real knots -delta / 2
    integ = np.zeros((len(step_times) - 1, n))
    for a in range(n):
        ham = qp.build_hamiltonian(one_atom_problem(prob, a))
        for term in ham.terms:
            if term.knots is None:
                if abs(term.op).sum() != 0:
                    raise ValueError("reference B: a static one-atom term")
                continue
            op = np.asarray(term.op.toarray())
            if abs(op[0, 1]) + abs(op[1, 0]) + abs(op[1, 1]) != 0 or np.any(np.imag(term.knots) != 0):
                raise ValueError("reference B takes no drive")
            spl = make_interp_spline(ham.tlist, np.real(term.knots) * 2.0 * op[0, 0].real, k=3)  # (coefficient_spline)
            for i in range(len(step_times) - 1):
                integ[i, a] += spl.integrate(step_times[i], step_times[i + 1])
    h = np.diff(step_times)
    phase = integ @ in_r + h[:, None] * energy[None, :]
    return np.exp(-1j * phase - 0.5 * h[:, None] * gamma[None, :])


def _apply_local(op, psi, n, a):
    v = psi.reshape(1 << a, 2, 1 << (n - 1 - a))
    return np.einsum("ij,ajb->aib", op, v).reshape(-1)


def diagonal_trajectory(prob, psi0, step_times, eval_times, seed, factors=None, perturb=None):
    """One trajectory of reference B from ``psi0`` (any norm).  Returns (normalised kets at eval_times, jumps, margins).
    ``perturb``: as in :func:`product_trajectory`."""
    from oracle.mcwf import mc_uniforms

    n = int(prob["n_qudits"])
    step_times = np.asarray(step_times, dtype=float)
    eval_times = np.asarray(eval_times, dtype=float)
    if factors is None:
        factors = diagonal_factors(prob, step_times)
    cops = local_collapse(prob)
    psi = np.asarray(psi0, dtype=complex).reshape(-1).copy()
    ref = float(np.vdot(psi, psi).real)
    count = 0
    target = mc_uniforms(seed, 0)[0]
    jumps, out = [], []
    m_thr, m_sel = np.inf, np.inf
    ei = 0
    if abs(eval_times[0] - step_times[0]) < 1e-12:
        out.append(psi / np.sqrt(ref))
        ei = 1
    for i in range(len(step_times) - 1):
        t1 = step_times[i + 1]
        psi = factors[i] * psi
        n2 = float(np.vdot(psi, psi).real)
        m_thr = min(m_thr, abs(n2 - target * ref) / ref)
        if n2 <= target * ref:
            cand = []
            for a in range(n):
                for k, c in enumerate(cops):
                    v = _apply_local(c, psi, n, a)
                    w = float(np.vdot(v, v).real)
                    cand.append((a, k, v, w if perturb is None else float(perturb(a, k, w))))
            total = sum(c[3] for c in cand)
            if total > 0.0:
                x = mc_uniforms(seed, count)[1] * total
                cum = 0.0
                pick = None
                for c in cand:
                    cum += c[3]
                    m_sel = min(m_sel, abs(cum - x) / total)
                    if pick is None and c[3] > 0.0 and cum > x:
                        pick = c
                if pick is None:
                    pick = [c for c in cand if c[3] > 0.0][-1]
                psi = pick[2] / np.sqrt(float(np.vdot(pick[2], pick[2]).real))
                jumps.append((float(t1), pick[0], pick[1]))
                count += 1
                target = mc_uniforms(seed, count)[0]
                ref = 1.0
                n2 = 1.0
        while ei < len(eval_times) and abs(eval_times[ei] - t1) < 1e-12:
            out.append(psi / np.sqrt(n2))
            ei += 1
    if ei != len(eval_times):
        raise ValueError("every evaluation time must be a point of the step grid")
    return out, jumps, (float(m_thr), float(m_sel))


# ---------------------------------------------------------------------------------------------------------------------
# The case table of the device tests
# ---------------------------------------------------------------------------------------------------------------------
# Seeds: the four that split differently into the low and high word of the Philox key first (2^32 = high word 1, low word
# 0 and 2^64 - 1 = all ones lead: the batch of two at 20 atoms has room for no more), then a fixed multiplicative
# sequence.  A case takes the first ``batch`` seeds of its list whose two margins are at least MARGIN; one seed in 12 may
# be skipped.
SPECIAL_SEEDS = (2 ** 32, 2 ** 64 - 1, 0, 2 ** 32 - 1)


def seed_list(salt, length):
    more = [((k + 1) * 0x9E3779B97F4A7C15 + salt * 0xD1B54A32D192ED03 + 12345) % 2 ** 64 for k in range(length)]
    return list(SPECIAL_SEEDS) + more


@dataclass(frozen=True)
class Case:
    kind: str          # "A" (product reference) or "B" (diagonal reference)
    n: int
    model: int         # A: 0 per-atom complex drives, 1 one global real drive; B: -1
    batch: int
    scale: float       # collapse rates = STRONG_RATES * scale / n
    salt: int = 0      # seeds the initial kets and the tail of the seed list
    norm2: float = 1.0  # squared norm of every initial ket (B: ignored when 0 - each ket keeps a norm of its own)

    @property
    def name(self):
        tag = f"{self.kind}{self.model if self.kind == 'A' else ''}-n{self.n}"
        return tag + (f"-norm{self.norm2:g}" if self.kind == "A" and self.norm2 != 1.0 else "")


SCALE = 5.0  # collapse rates = STRONG_RATES * SCALE / n: one to two jumps per trajectory at every size

# (kind, n, model[, norm2]) -> salt where salt 0 (3 for the unnormalised starts) misses a condition of
# tests/test_mcwf_ref.py (a case without a trajectory that does not jump, a seed too many below MARGIN, no jump on atom 0
# or N - 1 at that size); found with the references alone (`python tests/mcwf_ref.py` prints what the conditions are about)
_SALT = {("A", 10, 0): 1, ("B", 10, -1): 1,
         ("A", 11, 0): 3, ("A", 11, 1): 2, ("B", 11, -1): 2,
         ("A", 12, 0): 1, ("A", 12, 1): 1, ("B", 12, -1): 1,
         ("A", 14, 0): 20, ("A", 14, 1): 11, ("B", 14, -1): 20,
         ("A", 16, 0): 5, ("A", 12, 0, 0.37): 2, ("A", 12, 1, 2.5): 2}


def _table():
    def a(n, model, batch, norm2=1.0):
        key = ("A", n, model) if norm2 == 1.0 else ("A", n, model, norm2)
        return Case("A", n, model, batch, SCALE, _SALT.get(key, 0 if norm2 == 1.0 else 3), norm2)

    def b(n, batch):
        return Case("B", n, -1, batch, SCALE, _SALT.get(("B", n, -1), 0), norm2=0.0)

    cases = []
    for n in (1, 4, 5, 6, 9, 10, 11, 12, 13):
        cases += [a(n, 0, 12), a(n, 1, 12), b(n, 12)]
    cases += [a(14, 0, 8), a(14, 1, 8), b(14, 8)]
    for n, batch in ((16, 4), (20, 2)):
        cases += [a(n, 0, batch), a(n, 1, batch)]
    # unnormalised starts (reference A scales one factor; reference B's kets are unnormalised anyway)
    for n in (6, 12):
        cases += [a(n, 0, 12, 0.37), a(n, 1, 12, 2.5)]
    return cases


CASES = _table()


def initial_factors(case, b):
    """Reference A: the one-atom kets of trajectory ``b``: random directions; from 16 atoms on the inner atoms lean to g
    (their r amplitude times 0.15), so that the few jumps of a small batch still reach both ends of the register.  The
    first factor carries the squared norm of the case."""
    rng = np.random.default_rng([7, case.n, case.model + 1, case.salt, b])
    f = rng.normal(size=(case.n, 2)) + 1j * rng.normal(size=(case.n, 2))
    if case.n >= 16:
        f[1:-1, 0] *= 0.15
    f /= np.linalg.norm(f, axis=1)[:, None]
    f[0] *= np.sqrt(case.norm2)
    return f


def initial_ket(case, b):
    """Reference B: a random entangled ket; squared norm drawn between 0.3 and 3 (never 1)."""
    rng = np.random.default_rng([11, case.n, case.salt, b])
    v = rng.normal(size=1 << case.n) + 1j * rng.normal(size=1 << case.n)
    norm2 = case.norm2 if case.norm2 > 0 else float(rng.uniform(0.3, 3.0))
    return v * np.sqrt(norm2) / np.linalg.norm(v)


@dataclass
class CaseData:
    case: Case
    problem: dict
    seeds: np.ndarray       # uint64[batch]: the seeds used
    skipped: list           # seeds of the list passed over for a margin below MARGIN
    psi0: np.ndarray        # complex[batch, 2^N]
    kets: list              # per trajectory: the normalised kets at EVAL
    jumps: list             # per trajectory: [(time, atom, operator)]
    margins: list           # per trajectory: (threshold margin, selection margin)
    cpu_seconds: float


@functools.lru_cache(maxsize=None)
def _problem_and_steps(kind, n, model, scale):
    """The problem of a case and its no-jump steps (A: one-atom propagators, B: diagonal factors)."""
    if kind == "A":
        prob = problem_a(n, model, scale, 1000 + 10 * n + model)
        return prob, one_atom_propagators(prob, GRID)
    prob = problem_b(n, scale, 2000 + n)
    return prob, diagonal_factors(prob, GRID)


@functools.lru_cache(maxsize=None)
def case_data(case: Case, form_kets: bool = True) -> CaseData:
    """The reference trajectories of one case (computed once per process; nothing may change what it returns).
    ``form_kets=False`` (reference A only) leaves the 2^N kets out: jumps and margins of the big cases on the CPU."""
    t0 = time.perf_counter()
    prob, steps = _problem_and_steps(case.kind, case.n, case.model, case.scale)
    seeds, skipped, psi0, kets, jumps, margins = [], [], [], [], [], []
    for seed in seed_list(case.salt * 64 + case.n, case.batch):
        b = len(seeds)
        if b == case.batch:
            break
        if case.kind == "A":
            f0 = initial_factors(case, b)
            k, j, m = product_trajectory(prob, f0, GRID, EVAL, seed, props=steps, form_kets=form_kets)
            start = kron_chain(f0) if form_kets else f0
        else:
            start = initial_ket(case, b)
            k, j, m = diagonal_trajectory(prob, start, GRID, EVAL, seed, factors=steps)
        if min(m) < MARGIN:
            skipped.append(seed)
            continue
        seeds.append(seed)
        psi0.append(start)
        kets.append(k)
        jumps.append(j)
        margins.append(m)
    if len(seeds) != case.batch:
        raise RuntimeError(f"{case.name}: the seed list ran out")
    return CaseData(case, prob, np.array(seeds, dtype=np.uint64), skipped, np.stack(psi0), kets, jumps, margins,
                    time.perf_counter() - t0)


def table_report(form_kets=False, out=print):
    """One line per case: what tests/test_mcwf_ref.py asserts, from the references alone."""
    for case in CASES:
        d = case_data(case, form_kets if case.kind == "A" else True)
        counts = [len(j) for j in d.jumps]
        atoms = sorted({a for j in d.jumps for _, a, _ in j})
        ops = sorted({KINDS[k] for j in d.jumps for _, _, k in j})
        out(f"{case.name:14s} scale {case.scale:5.2f} salt {case.salt}  jumps {sum(counts):3d} {counts}  "
            f"margins {min(m[0] for m in d.margins):.1e} {min(m[1] for m in d.margins):.1e}  skipped {len(d.skipped)}  "
            f"atoms {atoms}  ops {ops}  cpu {d.cpu_seconds:.1f} s")


if __name__ == "__main__":
    table_report()

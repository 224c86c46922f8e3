"""An exact quantum-jump reference for the general-path kernels (multi-level and XY registers: k_mc_general.hpp, the
in-kernel copy in k_gen_traj_mc, host_mc_general.hpp), and the case table of their device tests
(tests/test_mcwf_general_ref.py, tests/test_gpu_mcwf_general_edges.py): NumPy / SciPy only.

The jump rule is that of ``oracle/mcwf.py``, unchanged (Philox4x32-10 keyed by the seed, counter = jump index; the
threshold tested at the end of every step of the grid; candidates atom-major, operator-minor, the first index whose
cumulative weight exceeds ``r2 * total``; ``ref = |psi0|^2`` before the first jump).  The full-space restatement runs
zvode on d^N amplitudes once per step: minutes per trajectory at 3^7.  This reference uses a structure the kernels know
nothing about:

* the problems are the bundles of tests/golden/make_general_fixtures.py (``xy_problem``, ``multilevel_problem`` with and
  without leakage, ``ising_problem`` with a non-diagonal operator) with slow analytic waveforms and an
  ``interaction_matrix`` that is **block-diagonal over clusters of 1 - 3 atoms**: cross-cluster entries are exactly 0.0
  (not a large distance: the XY exchange falls as 1/r^3 only).  ``lower_general`` keeps zero-weight pairs as ordinary
  groups, so nothing in the library can exploit it.  Inside a cluster the atoms are driven and interacting (XY: exchange
  and the u-u diagonal; multi-level: C6 on r-r); the members of a cluster are scattered over the atom indices by a
  seeded permutation, so strides mix inside a cluster; every atom that the term table has room for carries a local drive
  of its own on top of the global one.
* every collapse operator is local, so the ket stays a tensor product of cluster kets for ever.  The no-jump propagator
  of a cluster over a grid step is a d^k x d^k matrix (d^k <= 64), integrated once per cluster with the oracle's own
  pieces (``qp.build_hamiltonian`` of the cluster's sub-problem, ``mcwf.effective_rhs``, ``qp._zvode`` under
  ``qp.TIGHT``: one run over the grid from the identity, the step propagators are U(t_i+1) U(t_i)^-1).  A trajectory costs
  matrix-vector products only; norms and weights are products over clusters, kept in ``np.longdouble``
  (``|C_k^(a) psi|^2`` = the cluster's own value times the other clusters' norms); a jump replaces one cluster factor.
  The d^N ket is formed by index arithmetic at the evaluation times only.

:func:`cluster_trajectory` returns what ``tests/mcwf_ref.py`` returns: the normalised kets at the evaluation times, the
jumps [(time, atom, operator)] and the two smallest margins (threshold, selection).  ``MARGIN``, the seed list and the
skipped-seed rule are those of tests/mcwf_ref.py.

What the reference can and cannot see: drive, interaction, decay and jump bookkeeping of kets that are entangled inside
clusters of up to three atoms, at any size; never entanglement between clusters.  The kernels treat every atom pair
alike, so an error that depends on the strides of a pair shows inside the clusters (their members are scattered).

``python tests/mcwf_general_ref.py`` prints, per case of :data:`CASES`, the figures the conditions of
tests/test_mcwf_general_ref.py are about (jumps, margins, skipped seeds, coverage, CPU seconds).
"""
from __future__ import annotations

import functools
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # run as a script: the repository root holds ``oracle`` and ``pulser_amd``
    sys.path.insert(0, os.path.dirname(_HERE))
for _p in (_HERE, os.path.join(_HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_general_fixtures as G  # noqa: E402
from mcwf_ref import CLD, DURATION, EVAL, GRID, LD, MARGIN, seed_list  # noqa: E402,F401  (shared, not forked)

from pulser_amd import problem as P  # noqa: E402

MC_MAX_OPS = 16      # k_mc.hpp
MAX_GEN_TERMS = 96   # k_general.hpp

NONDIAG2 = np.array([[1.0, 1.0], [0.0, 0.0]], dtype=complex)          # tests/test_gpu_mcwf_general.py: NONDIAG
NONDIAG3 = np.array([[0, 0, 0], [1, 0, 1], [0, 0, 0]], dtype=complex)  # |g>(<r| + <h|) in (r, g, h)


def _ops16():
    """Exactly MC_MAX_OPS operators of d = 3: the nine |a><b| and seven combinations, rates 1.0 - 2.5."""
    mats = []
    for i in range(3):
        for j in range(3):
            m = np.zeros((3, 3), dtype=complex)
            m[i, j] = 1.0
            mats.append(m)
    rng = np.random.default_rng(1616)
    for _ in range(7):
        mats.append((rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3))) / 3.0)
    return [(float(np.sqrt(1.0 + 0.1 * k)), m) for k, m in enumerate(mats)]


# name -> (builder key, operators as (rate, kind or matrix)); the physical sets are those of CASES of
# tests/test_gpu_mcwf_general.py
OPERATORS = {
    "all": [(3.0, "sigma_gr"), (2 * 1.5, "sigma_rr"), (2 * 1.0, "sigma_hh")],
    "leak": [(3.0, "sigma_xr"), (2.0, "sigma_xg")],          # weight zero until the first leak: nothing starts in x
    # one atom cannot leak twice: its case adds the dephasing of r
    "leak+": [(3.0, "sigma_xr"), (2.0, "sigma_xg"), (2 * 1.5, "sigma_rr")],
    "xy": [(2 * 2.0, "sigma_dd")],                           # a single operator
    "nondiag2": [(2.5, NONDIAG2)],
    "nondiag3": [(2.5, NONDIAG3), (2 * 1.5, "sigma_rr"), (2 * 1.0, "sigma_hh")],
    "ops16": [(c * c, m) for c, m in _ops16()],
}
# collapse rates = rate * SCALE / n: one to two jumps per trajectory over the 60 ns at every size
SCALE = {"all": 10.0, "leak": 16.0, "leak+": 8.0, "xy": 14.0, "nondiag2": 10.0, "nondiag3": 9.0, "ops16": 1.6}
BASIS = {"all": "all", "leak": "leak", "leak+": "leak", "xy": "xy", "nondiag2": "ising", "nondiag3": "all", "ops16": "all"}
LOCAL_DIM = {"all": 3, "leak": 4, "xy": 2, "ising": 2}
QUIET = {"all": 1, "leak": 2, "xy": 0, "ising": 1}  # digit of g / h / u / g: (nearly) no collapse operator acts on it


def op_label(ops, k):
    kind = OPERATORS[ops][k][1]
    return kind if isinstance(kind, str) else f"{ops}[{k}]"


# ---------------------------------------------------------------------------------------------------------------------
# The case table
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    ops: str            # key of OPERATORS (fixes the basis and the local dimension)
    n: int              # atoms
    parts: tuple        # cluster sizes, 1 - 3 each
    batch: int
    routes: tuple       # of "many" (ryd_general_mc_solve_many, one engine per trajectory: dim <= 4096), "batched"
                        # (ryd_general_mc_solve on the persistent kernel), "chain" (the multi-launch kernels)
    norm2: float = 1.0  # squared norm of every initial ket
    lean: bool = False  # few terms (no detunings, local drives on atoms 0 and N - 1 only): what the rule of
                        # use_persistent_general_mc (groups x rows <= 13) lets onto the batched persistent kernel
    salt: int = 0       # seeds the initial kets and the tail of the seed list

    @property
    def basis(self):
        return BASIS[self.ops]

    @property
    def d(self):
        return LOCAL_DIM[self.basis]

    @property
    def dim(self):
        return self.d ** self.n

    @property
    def name(self):
        tag = f"{self.ops}-n{self.n}" + ("-lean" if self.lean else "")
        tag += f"-norm{self.norm2:g}" if self.norm2 != 1.0 else ""
        return tag + (f"-b{self.batch}" if self.batch not in (12, 8, 4, 2) else "")


def _batch_of(dim):
    """Batches shrink with size, as in the two-level table."""
    return 12 if dim <= 1024 else 8 if dim <= 4096 else 4 if dim <= 19683 else 2


# (ops, n, lean[, norm2 | batch]) -> salt where salt 0 misses a condition of tests/test_mcwf_general_ref.py; found with
# the reference alone (`python tests/mcwf_general_ref.py` prints what the conditions are about)
# leak 6: salt 0 has no jump on atom 5 at the cap; ops16 7 (no level is quiet under 16 operators): no trajectory without a jump
_SALT: dict = {("leak", 6, False): 1, ("ops16", 7, False): 2}


def _table():
    def c(ops, n, parts, routes, batch=None, norm2=1.0, lean=False):
        assert sum(parts) == n and all(1 <= p <= 3 for p in parts)
        batch = batch or _batch_of(LOCAL_DIM[BASIS[ops]] ** n)
        key = (ops, n, lean) + ((norm2,) if norm2 != 1.0 else ()) + ((batch,) if batch in (1, 130) else ())
        return Case(ops, n, tuple(parts), batch, tuple(routes), norm2, lean, _SALT.get(key, 0))

    pc = ("many", "chain")
    pbc = ("many", "batched", "chain")
    cases = [
        # fewer rows than one wave
        c("xy", 1, (1,), pbc), c("all", 1, (1,), pbc), c("leak+", 1, (1,), pbc),
        # the batched persistent kernel (lean: the sizes that pass the rule), batches of 1, 12 and 130
        c("xy", 6, (3, 2, 1), pbc, lean=True), c("xy", 6, (3, 2, 1), pbc, batch=130, lean=True),
        c("xy", 6, (3, 2, 1), pbc, batch=1, lean=True),
        c("leak", 3, (2, 1), pbc, lean=True), c("nondiag2", 6, (3, 2, 1), pbc, lean=True),
        c("all", 5, (2, 2, 1), pbc, lean=True), c("nondiag3", 4, (2, 1, 1), pbc, lean=True),
        c("all", 6, (3, 2, 1), pbc, lean=True), c("leak", 5, (2, 2, 1), pbc, lean=True),
        # the persistent kernel's register rows: j = 0 partly filled / full, two rows, j = 2 with 139 rows, the cap
        c("all", 5, (2, 2, 1), pc), c("all", 6, (3, 2, 1), pc), c("leak", 5, (2, 2, 1), pc),
        c("xy", 10, (3, 3, 2, 2), pc), c("xy", 11, (3, 3, 3, 2), pc),
        c("all", 7, (3, 2, 2), pc), c("nondiag3", 7, (3, 3, 1), pc),
        c("leak", 6, (3, 2, 1), pc), c("xy", 12, (3, 3, 3, 2, 1), pc),
        # the selection table at its limits; unnormalised starts
        # (16 complex operators: the only ones whose C^dag C has an imaginary part - at j = 0, on rows j >= 1, batched)
        c("ops16", 6, (3, 2, 1), pc), c("ops16", 7, (3, 3, 1), pc), c("ops16", 5, (2, 2, 1), pbc, lean=True),
        c("all", 6, (3, 2, 1), pc, norm2=0.37), c("xy", 10, (3, 3, 2, 2), pc, norm2=2.5),
        # the multi-launch chain at its natural sizes: 6, 19, 16, 8, 16 blocks and the cap of 128
        c("all", 8, (3, 3, 2), ("chain",)), c("all", 9, (3, 3, 2, 1), ("chain",)),
        c("leak", 7, (3, 2, 1, 1), ("chain",)), c("xy", 13, (3, 3, 3, 2, 2), ("chain",)),
        c("xy", 14, (3, 3, 3, 3, 2), ("chain",)), c("xy", 18, (3, 3, 3, 3, 3, 2, 1), ("chain",)),
    ]
    assert len({x.name for x in cases}) == len(cases)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def clusters_of(case):
    """The atoms of every cluster (each sorted): a seeded permutation cut into ``case.parts``."""
    for attempt in range(64):  # (the first permutation that leaves some cluster's members apart, from 5 atoms on)
        perm = np.random.default_rng([31, case.n, len(case.parts), LOCAL_DIM[case.basis], attempt]).permutation(case.n)
        out, at = [], 0
        for p in case.parts:
            out.append(tuple(sorted(int(a) for a in perm[at:at + p])))
            at += p
        if case.n < 5 or any(c[-1] - c[0] >= len(c) for c in out):
            return out
    raise RuntimeError("no scattered clusters")


def n_local_drives(case):
    """Atoms with a local drive: as many as MAX_GEN_TERMS allows (a drive is 4 matrix-free terms: amplitude and
    detuning, each with its adjoint), atoms 0 and N - 1 first.  Lean cases: those two only."""
    if case.lean:
        return min(case.n, 2)
    fixed = 4 + (4 if case.basis == "xy" else 1) + 1  # global drive, interaction, decay
    return min(case.n, (MAX_GEN_TERMS - fixed) // 4)


def _wave(k, lean):
    """Drive number ``k``: analytic and slow (the curvature estimate of host_sched.hpp, summed over the terms, stays
    below the bound at which the stepper sub-divides a sample interval, at every size of the table)."""
    t = GRID
    rng = np.random.default_rng([77, k])
    a, b, c = rng.uniform(4, 10), rng.uniform(2, 8), rng.uniform(-3, 3)
    return {"amp": a * (1 + 0.3 * np.sin((1 + k % 3) * t + k)),
            "det": np.zeros(DURATION) if lean else b * np.cos(2 * t + k) - c,
            "phase": 0.4 * k + 0.3 * np.sin(2 * t)}


@functools.lru_cache(maxsize=None)
def _problem(ops, n, parts, lean):
    case = Case(ops, n, parts, 1, (), lean=lean)
    basis = case.basis
    coords = P.register_coords(P.square_rect(1, n), 7.0)
    rates = [(float(np.sqrt(r * SCALE[ops] / n)), k) for r, k in OPERATORS[ops]]
    if basis == "xy":
        prob = G.xy_problem(coords, DURATION, 1)
        prob["collapse_ops"] = rates
        local_basis, global_basis = "XY", "XY"
    elif basis == "ising":
        prob = G.ising_problem(coords, DURATION, 1, collapse=rates)
        local_basis, global_basis = "ground-rydberg", "ground-rydberg"
    else:
        prob = G.multilevel_problem(coords, DURATION, 1, leakage=basis == "leak", collapse=rates)
        local_basis, global_basis = "digital", "ground-rydberg"
    # waveforms
    prob["samples"]["Global"][global_basis] = _wave(0, lean)
    order = [0, n - 1] + list(range(1, n - 1))
    prob["samples"]["Local"][local_basis] = {q: _wave(1 + q, lean) for q in sorted(set(order[:n_local_drives(case)]))}
    # interaction: block-diagonal over the clusters, couplings of their own inside each
    rng = np.random.default_rng([55, n, len(parts), case.d])
    imat = np.zeros_like(np.asarray(prob["interaction_matrix"], dtype=float))
    for cl in clusters_of(case):
        for x, i in enumerate(cl):
            for j in cl[x + 1:]:
                for layer in range(imat.shape[0]):
                    v = rng.uniform(3.0, 12.0) * (rng.choice([-1.0, 1.0]) if basis == "xy" and layer == 0 else 1.0)
                    imat[layer, i, j] = imat[layer, j, i] = v
    prob["interaction_matrix"] = imat
    return prob


def problem_of(case):
    """The problem bundle of a case (shared by the cases that differ in batch, start norm or salt only: read-only)."""
    return _problem(case.ops, case.n, case.parts, case.lean)


def cluster_problem(prob, atoms):
    """The problem of the atoms ``atoms`` alone: their samples (and the global ones), their block of the interaction."""
    atoms = list(atoms)
    sub = dict(prob)
    sub["n_qudits"] = len(atoms)
    sub["qubit_ids"] = tuple(prob["qubit_ids"][a] for a in atoms)
    sub["coords"] = np.asarray(prob["coords"])[atoms]
    sub["interaction_matrix"] = np.asarray(prob["interaction_matrix"])[:, atoms][:, :, atoms]
    sub["bad_atoms"] = np.zeros(len(atoms), dtype=bool)
    local = {}
    for basis, per in prob["samples"].get("Local", {}).items():
        local[basis] = {i: per[a] for i, a in enumerate(atoms) if a in per}
    sub["samples"] = {"Global": prob["samples"].get("Global", {}), "Local": local}
    return sub


def local_collapse(prob):
    """The d x d collapse operators in the order of ``prob["collapse_ops"]`` (from the oracle's one-atom build)."""
    from oracle import qutip_path as qp

    return [np.asarray(c.toarray()) for c in qp.build_hamiltonian(cluster_problem(prob, [0])).collapse]


def cluster_propagators(prob, atoms, step_times):
    """complex[n_steps, m, m], m = d^k: the no-jump propagators of the cluster over every step under its own H_eff(t)."""
    from oracle import mcwf, qutip_path as qp

    ham = qp.build_hamiltonian(cluster_problem(prob, atoms))
    m = ham.d ** ham.n
    rhs1 = mcwf.effective_rhs(ham)

    def rhs(t, y):
        return rhs1(t, y.reshape(m, m)).reshape(-1)

    step_times = np.asarray(step_times, dtype=float)
    us = [u.reshape(m, m) for u in qp._zvode(rhs, np.eye(m, dtype=complex).reshape(-1), step_times, qp.TIGHT)]
    # U(t_i+1, t_i) = U(t_i+1, 0) U(t_i, 0)^-1 (the decay over the run is a factor of a few: well conditioned)
    return np.stack([np.linalg.solve(us[i].T, us[i + 1].T).T for i in range(len(step_times) - 1)])


@functools.lru_cache(maxsize=None)
def _case_propagators(ops, n, parts, lean, cluster):
    case = Case(ops, n, parts, 1, (), lean=lean)
    return cluster_propagators(problem_of(case), clusters_of(case)[cluster], GRID)


@functools.lru_cache(maxsize=None)
def _gather_index(d, n, clusters):
    """int64[n_clusters, d^n]: the index into cluster c's ket of every basis state (atom 0 the highest digit)."""
    idx = np.arange(d ** n, dtype=np.int64)
    out = np.zeros((len(clusters), d ** n), dtype=np.int64)
    for c, cl in enumerate(clusters):
        for a in cl:
            out[c] = out[c] * d + (idx // d ** (n - 1 - a)) % d
    return out


def product_ket(d, n, clusters, factors):
    """The d^n ket of the cluster kets ``factors`` (complex128)."""
    gi = _gather_index(d, n, tuple(clusters))
    out = np.asarray(factors[0], dtype=complex)[gi[0]]
    for c in range(1, len(clusters)):
        out = out * np.asarray(factors[c], dtype=complex)[gi[c]]
    return out


def _norm2(x):
    return (x.real ** 2 + x.imag ** 2).sum()


def _apply_site(op, phi, d, k, p):
    """op on position p of a k-atom cluster ket."""
    v = phi.reshape(d ** p, d, d ** (k - 1 - p))
    return np.einsum("ij,ajb->aib", op, v).reshape(-1)


def cluster_trajectory(d, n, clusters, cops, props, factors0, step_times, eval_times, seed, form_kets=True,
                       perturb=None, override=None, trace=None):
    """One trajectory from the product of the cluster kets ``factors0`` (any norms).  ``props[c]``: complex[n_steps, m, m].
    Returns (kets at eval_times - normalised, or the normalised factor lists with ``form_kets=False`` -, jumps, margins).
    ``perturb(atom, operator, weight)`` replaces a weight of the selection, ``override(jump index, atom, operator)``
    returns the (atom, operator) to jump with instead (the sensitivity checks of tests/test_mcwf_general_ref.py).
    ``trace``: a list that receives (step, squared norm / ref before the test, jumps so far) per step, and
    ("select", candidates before the pick with weight zero) per jump."""
    from oracle.mcwf import mc_uniforms

    step_times = np.asarray(step_times, dtype=float)
    eval_times = np.asarray(eval_times, dtype=float)
    props = [np.asarray(p).astype(CLD) for p in props]
    cops = [np.asarray(c).astype(CLD) for c in cops]
    phi = [np.asarray(f).astype(CLD).copy() for f in factors0]
    where = {a: (c, p) for c, cl in enumerate(clusters) for p, a in enumerate(cl)}

    def emit():
        f = [x / np.sqrt(_norm2(x)) for x in phi]
        return product_ket(d, n, clusters, f) if form_kets else [np.asarray(x, dtype=complex) for x in f]

    ref = LD(np.prod(np.array([_norm2(x) for x in phi], dtype=LD)))
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
        phi = [props[c][i] @ phi[c] for c in range(len(clusters))]
        nc = np.array([_norm2(x) for x in phi], dtype=LD)
        n2 = LD(np.prod(nc))
        m_thr = min(m_thr, float(abs(n2 - target * ref) / ref))
        if trace is not None:
            trace.append((i, float(n2 / ref), count))
        if n2 <= target * ref:
            rest = [LD(np.prod(np.delete(nc, c))) for c in range(len(clusters))]
            cand = []
            for a in range(n):  # atom-major, operator-minor
                c, p = where[a]
                for k, op in enumerate(cops):
                    v = _apply_site(op, phi[c], d, len(clusters[c]), p)
                    w = LD(_norm2(v)) * rest[c]
                    cand.append((a, k, v, w if perturb is None else LD(perturb(a, k, w))))
            total = sum(x[3] for x in cand)
            if total > 0:
                x = LD(mc_uniforms(seed, count)[1]) * total
                cum = LD(0)
                pick = None
                for pos, cd in enumerate(cand):
                    cum += cd[3]
                    m_sel = min(m_sel, float(abs(cum - x) / total))
                    if pick is None and cd[3] > 0 and cum > x:
                        pick = cd
                        if trace is not None:
                            trace.append(("select", sum(1 for q in cand[:pos] if q[3] == 0)))
                if pick is None:
                    pick = [cd for cd in cand if cd[3] > 0][-1]
                if override is not None:
                    a, k = override(count, pick[0], pick[1])
                    if (a, k) != (pick[0], pick[1]):
                        pick = [cd for cd in cand if (cd[0], cd[1]) == (a, k)][0]
                phi = [x / np.sqrt(_norm2(x)) for x in phi]
                c = where[pick[0]][0]
                phi[c] = pick[2] / np.sqrt(_norm2(pick[2]))
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


def initial_factors(case, b):
    """The cluster kets of trajectory ``b``: seeded, entangled inside the cluster, nothing in the leakage state; the
    first one carries the squared norm of the case.  Trajectory 1 of every batch leans to the level that (nearly) no
    operator of its basis acts on (every other digit costs a factor 0.15), so that the small batches too hold a
    trajectory that decays too slowly to jump."""
    d = case.d
    out = []
    for c, cl in enumerate(clusters_of(case)):
        rng = np.random.default_rng([13, case.n, d, case.salt, b, c])
        m = d ** len(cl)
        v = rng.normal(size=m) + 1j * rng.normal(size=m)
        digits = (np.arange(m)[:, None] // d ** np.arange(len(cl))) % d
        if case.basis == "leak":
            v[(digits == 3).any(axis=1)] = 0.0
        if case.batch >= 2 and b == 1:
            v *= 0.15 ** (digits != QUIET[case.basis]).sum(axis=1)
        out.append(v / np.linalg.norm(v))
    out[0] = out[0] * np.sqrt(case.norm2)
    return out


CASES = _table()


@dataclass
class CaseData:
    case: Case
    problem: dict
    clusters: list
    seeds: np.ndarray       # uint64[batch]: the seeds used
    skipped: list           # seeds of the list passed over for a margin below MARGIN
    factors0: list          # per trajectory: the initial cluster kets
    kets: list              # per trajectory: the normalised kets (or factor lists) at EVAL
    jumps: list             # per trajectory: [(time, atom, operator)]
    margins: list           # per trajectory: (threshold margin, selection margin)
    traces: list            # per trajectory: the ``trace`` of cluster_trajectory
    cpu_seconds: float

    def psi0(self):
        """complex[batch, d^n]: the initial kets."""
        c = self.case
        return np.stack([product_ket(c.d, c.n, self.clusters, f) for f in self.factors0])


def case_parts(case):
    """(clusters, local collapse operators, propagators per cluster) of a case; the propagators are cached per
    (problem, cluster)."""
    clusters = clusters_of(case)
    props = [_case_propagators(case.ops, case.n, case.parts, case.lean, c) for c in range(len(clusters))]
    return clusters, local_collapse(problem_of(case)), props


@functools.lru_cache(maxsize=None)
def case_data(case: Case, form_kets: bool = True) -> CaseData:
    """The reference trajectories of one case (computed once per process; nothing may change what it returns).
    ``form_kets=False`` leaves the d^n kets out: jumps and margins on the CPU."""
    t0 = time.perf_counter()
    clusters, cops, props = case_parts(case)
    seeds, skipped, f0s, kets, jumps, margins, traces = [], [], [], [], [], [], []
    for seed in seed_list(case.salt * 64 + case.n, case.batch):
        b = len(seeds)
        if b == case.batch:
            break
        f0 = initial_factors(case, b)
        tr = []
        k, j, m = cluster_trajectory(case.d, case.n, clusters, cops, props, f0, GRID, EVAL, seed, form_kets=form_kets,
                                     trace=tr)
        if min(m) < MARGIN:
            skipped.append(seed)
            continue
        seeds.append(seed)
        f0s.append(f0)
        kets.append(k)
        jumps.append(j)
        margins.append(m)
        traces.append(tr)
    if len(seeds) != case.batch:
        raise RuntimeError(f"{case.name}: the seed list ran out")
    return CaseData(case, problem_of(case), clusters, np.array(seeds, dtype=np.uint64), skipped, f0s, kets, jumps,
                    margins, traces, time.perf_counter() - t0)


def schedule_estimates(tables, decay_norm=0.0):
    """The two per-interval figures by which build_schedule (host_sched.hpp) sub-divides a sample interval on the
    general path, restated from the lowered tables: (max curvature estimate / its bound, max step argument / its
    bound).  Both below 1: one CF4 step per sample interval.  ``decay_norm``: the norm of the static decay term that
    set_collapse adds (n times the largest row sum of sum C^dag C / 2); it counts for the second figure only."""
    pp = np.asarray(tables.pp)
    dt = np.diff(np.asarray(tables.tknots))[None, :]
    curv = np.abs(pp[:, :, 1]) * dt ** 2 + np.abs(pp[:, :, 0]) * dt ** 3
    mag = np.abs(pp[:, :, 3]) + np.abs(pp[:, :, 2]) * dt + curv
    bd_curv = np.zeros(pp.shape[1])
    bd_step = np.zeros(pp.shape[1]) + decay_norm
    for t in range(len(tables.series)):
        w = abs(tables.scale[t]) * float(tables.row_norm[t])
        s = int(tables.series[t])
        if s >= 0:
            bd_curv += w * curv[s]
            bd_step += w * mag[s]
        else:
            bd_step += w
    h = float(dt.max())
    return float((1e-5 * h * bd_curv).max() / 1e-10), float((0.5 * h * bd_step).max() / 1.5)


def table_report(out=print):
    """One line per case: what tests/test_mcwf_general_ref.py asserts, from the reference alone."""
    for case in CASES:
        d = case_data(case, False)
        counts = [len(j) for j in d.jumps]
        atoms = sorted({a for j in d.jumps for _, a, _ in j})
        ops = sorted({k for j in d.jumps for _, _, k in j})
        shown = counts if len(counts) <= 12 else f"{counts[:12]}..."
        out(f"{case.name:22s} dim {case.dim:6d} salt {case.salt}  jumps {sum(counts):3d} {shown}  "
            f"margins {min(m[0] for m in d.margins):.1e} {min(m[1] for m in d.margins):.1e}  skipped {len(d.skipped)}  "
            f"atoms {atoms}  ops {ops}  cpu {d.cpu_seconds:.1f} s")


if __name__ == "__main__":
    table_report()

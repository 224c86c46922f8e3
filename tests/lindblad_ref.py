"""Cluster-product reference for the two-level master-equation kernels, and the case table of the device tests
(tests/test_lindblad_ref.py, tests/test_gpu_lindblad_edges.py): NumPy, SciPy and the repository's ``oracle`` only.

A register is made of small clusters (1 to 4 atoms, :data:`SPECIES`).  Atoms interact strongly inside a cluster - at the
blockade radius (U = 12.6 rad/us) or at a tight 6 um (U = 116 rad/us) - and the cluster centres sit on a line
:data:`CENTRE_PITCH` = 1000 um apart, so that the summed cross-cluster interaction times the duration is below 1e-10
(:func:`separation`; one pair at 1000 um is 5.4e-12 rad/us).  Every collapse operator is local, so rho(t) is the tensor
product of the cluster density matrices, each one a Lindblad solve on at most 4^4 = 256 entries with the oracle under
``qp.TIGHT`` (:func:`cluster_solutions`, cached).  The structured evaluators (:class:`Reference`) never form the 4^N
matrix above 9 atoms.  Atom 0 is the highest bit; tests/test_lindblad_ref.py checks that, and the whole construction,
against the full-space oracle at 4 to 6 atoms.

What the reference can and cannot see.  It sees interaction (blockade included), entanglement inside a cluster, per-atom
time-dependent complex or real drives, all dissipators together, and - because the atoms of a cluster may sit on any atom
indices and no two atoms of a register are alike - a factor applied to the wrong row or column bit, a drive read from the
wrong atom, a pair pass that couples the wrong bits.  It cannot see a register in which every atom interacts with every
other: a defect that shows only when more than four atoms are coupled (an interaction diagonal wrong for five or more
excitations, a splitting error that grows with the number of coupled neighbours) stays with the dephasing fixtures
(``cfg3_tri*_dephasing.npz``) and the path-against-path tests.

Dissipator cases (:data:`DISS`): the rates of ``ME_CASES`` (tests/test_gpu_parity.py) and ``DBL_CASES``
(tests/test_gpu_ket.py).  ``ME_CASES["dephasing"]`` (sqrt(0.1) sigma_rr) IS gamma = 0.05 / us with sqrt(2 gamma), the
slow-dephasing case of the split-operator rows; so that the six cases stay distinct, "dephasing" here takes gamma = 0.2 / us
(the rate of ``test_split_operator_rows_batch_of_two_different_12_atom_registers``: above the 0.06 / us at which the row
path stops taking four-knot halves).

Reference floor (measured: ``python tests/lindblad_ref.py``, asserted by tests/test_lindblad_ref.py): the cluster product
against the full-space oracle, both under ``qp.TIGHT``, over 40 ns at 4 to 6 atoms, every dissipator case, family and
initial state: max |product - full| = :data:`FLOOR_MEASURED`; the test allows :data:`FLOOR_FACTOR` times that.

``python tests/lindblad_ref.py`` prints the figures the CPU tests assert (floor, separation sums, motion, sensitivity
ratios) and the CPU time of all references of :data:`CASES`.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root holds ``oracle`` and ``pulser_amd``
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulser_amd import problem as P

BAR = 1e-7            # the project's parity bar on every compared entry of rho (AMP_TOL)
TRACE_BAR = 2e-8      # the existing bar of the row path on the trace
DURATION = 41         # samples: 40 ns
GRID = np.arange(DURATION) / 1000.0
EVAL = (0.0, 0.013, 0.04)       # up to 12 atoms
EVAL_BIG = (0.0, 0.008, 0.02)   # 13 and 14 atoms
CENTRE_PITCH = 1000.0           # um between cluster centres
SEPARATION_BAR = 1e-10          # sum over cross-cluster pairs of U_ij x duration
TIGHT_PITCH = 6.0               # um: U = 116 rad/us between neighbours

# measured by `python tests/lindblad_ref.py`: 6.3e-12 over the comparisons of :func:`floor_setups`, 6.8e-12 with the whole
# cross of (dissipator, family, initial state) on both 6-atom layouts as well (100 comparisons); the test's bar is
# FLOOR_FACTOR x FLOOR_MEASURED
FLOOR_MEASURED = 6.8e-12
FLOOR_FACTOR = 5.0

PAULIS = {
    "x": [(1, "sigma_gr"), (1, "sigma_rg")],
    "y": [(1j, "sigma_gr"), (-1j, "sigma_rg")],
    "z": [(1, "sigma_rr"), (-1, "sigma_gg")],
}  # helpers.DEPOL_PAULIS

_DEPOL = [(float(np.sqrt(0.05 / 4)), p) for p in "xyz"]
DISS = {
    "dephasing": [(float(np.sqrt(2 * 0.2)), "sigma_rr")],
    "slow-dephasing": [(float(np.sqrt(2 * 0.05)), "sigma_rr")],
    "relaxation": [(float(np.sqrt(0.07)), "sigma_gr")],
    "relaxation+dephasing": [(float(np.sqrt(2 * 0.05)), "sigma_rr"), (float(np.sqrt(0.03)), "sigma_gr")],
    "depolarizing": list(_DEPOL),
    "all": [(float(np.sqrt(0.1)), "sigma_rr"), (float(np.sqrt(0.07)), "sigma_gr")] + list(_DEPOL),
    "none": [],  # (the motion check of tests/test_lindblad_ref.py: the same case without collapse operators)
}
DISS_CASES = ("dephasing", "slow-dephasing", "relaxation", "relaxation+dephasing", "depolarizing", "all")
DOUBLE_FLIP = ("relaxation", "relaxation+dephasing", "depolarizing", "all")
FAMILIES = ("complex", "real", "global")


def blockade_pitch():
    return (P.C6_LEVEL70 / (4 * 2 * np.pi / 2)) ** (1 / 6)  # helpers.blockade_radius


# ---------------------------------------------------------------------------------------------------------------------
# species
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Species:
    name: str
    shape: tuple   # positions in units of the pitch
    seed: int

    @property
    def size(self):
        return len(self.shape)


_H = float(np.sqrt(3) / 2)
SPECIES = {s.name: s for s in (
    Species("one", ((0.0, 0.0),), 101),
    Species("pair", ((0.0, 0.0), (1.0, 0.0)), 102),
    Species("pair'", ((0.0, 0.0), (0.9, 0.8)), 103),                      # 1.2 pitches apart
    Species("chain3", ((0.0, 0.0), (1.0, 0.0), (2.0, 0.0)), 104),
    Species("tri3", ((0.0, 0.0), (1.0, 0.0), (0.5, _H)), 105),
    Species("square4", ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)), 106),
    Species("rhomb4", ((0.0, 0.0), (1.0, 0.0), (0.5, _H), (1.5, _H)), 107),
)}


def species_waveforms(sp: Species, family: str):
    """Per-atom samples of a species: "complex" - amplitude, detuning and phase all depend on time
    (helpers.local_problem's shapes); "real" - phase 0 (test_gpu_ket.real_local_problem's)."""
    rng = np.random.default_rng([sp.seed, 1])
    t = GRID
    out = []
    for k in range(sp.size):
        a, b, c = rng.uniform(2, 12, 3)
        w = 1 + (sp.seed + 3 * k) % 4
        out.append({"amp": a * (1 + 0.5 * np.sin(2 * np.pi * w * t / (4 * t[-1]) + 0.7 * k)),
                    "det": b * np.cos(3 * t + k + 0.1 * sp.seed) - c,
                    "phase": (0.3 * k + 0.05 * sp.seed + 0.8 * np.sin(5 * t + k)) if family == "complex" else np.zeros(DURATION)})
    return out


def global_waveform():
    """The one global real drive of the ``REALU`` instantiation of ``k_traj_dm``."""
    t = GRID
    return {"amp": 9.0 * (1 + 0.3 * np.sin(5 * t)), "det": 7.0 * np.cos(4 * t) - 5.0, "phase": np.zeros(DURATION)}


def species_ket(sp: Species, init: str):
    """"ket": a seeded random normalised ket of the cluster; "ground": |g...g> (local state 1 of every atom)."""
    d = 1 << sp.size
    if init == "ground":
        v = np.zeros(d, dtype=complex)
        v[-1] = 1.0
        return v
    rng = np.random.default_rng([sp.seed, 2])
    v = rng.normal(size=d) + 1j * rng.normal(size=d)
    return v / np.linalg.norm(v)


# ---------------------------------------------------------------------------------------------------------------------
# assembly
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Setup:
    """One register and its problem: ``layout`` = ((species name, atom indices), ...); hashable."""
    n: int
    layout: tuple
    diss: str = "all"
    family: str = "complex"
    init: str = "ket"
    pitch: str = "blockade"          # or "tight"
    bad: tuple = ()                  # atom indices of badly prepared atoms (masked out of the interaction)
    centre_pitch: float = CENTRE_PITCH

    def swapped(self, **kw):
        return dataclasses.replace(self, **kw)


def layout_of(n, parts, perm=None):
    """((species, atoms), ...) with the clusters of ``parts`` placed, in order, on the atom indices ``perm``
    (default: 0 .. n - 1 in order)."""
    perm = list(range(n)) if perm is None else [int(p) for p in perm]
    assert sorted(perm) == list(range(n)) and sum(SPECIES[s].size for s in parts) == n, (n, parts, perm)
    out, pos = [], 0
    for s in parts:
        k = SPECIES[s].size
        out.append((s, tuple(perm[pos:pos + k])))
        pos += k
    return tuple(out)


def _pitch(setup):
    return blockade_pitch() if setup.pitch == "blockade" else TIGHT_PITCH


def assemble(setup: Setup):
    """The full problem (``P.make_ising_problem`` + samples, collapse operators, Pauli table, bad-atom mask)."""
    n = setup.n
    coords = np.zeros((n, 2))
    loc = {}
    for c, (name, atoms) in enumerate(setup.layout):
        sp = SPECIES[name]
        waves = species_waveforms(sp, setup.family) if setup.family != "global" else None
        for k, a in enumerate(atoms):
            coords[a] = np.asarray(sp.shape[k]) * _pitch(setup) + np.array([c * setup.centre_pitch, 0.0])
            if waves is not None:
                loc[a] = waves[k]
    zero = np.zeros(DURATION)
    glob = global_waveform() if setup.family == "global" else {"amp": zero, "det": zero, "phase": zero}
    prob = P.make_ising_problem(coords, glob, collapse_ops=DISS[setup.diss])
    if setup.family != "global":
        prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": {a: loc[a] for a in sorted(loc)}}}
    prob["depolarizing_pauli_2ds"] = dict(PAULIS)
    bad = np.zeros(n, dtype=bool)
    bad[list(setup.bad)] = True
    prob["bad_atoms"] = bad
    prob["interaction_matrix"] = P.interaction_matrix(coords, P.C6_LEVEL70, bad)
    return prob


def sub_problem(prob, atoms):
    """The problem of the atoms ``atoms`` alone: the same coordinates, samples (renumbered), collapse operators, mask."""
    atoms = list(atoms)
    sub = dict(prob)
    sub["n_qudits"] = len(atoms)
    sub["qubit_ids"] = tuple(prob["qubit_ids"][a] for a in atoms)
    sub["coords"] = np.asarray(prob["coords"])[atoms]
    sub["bad_atoms"] = np.asarray(prob["bad_atoms"])[atoms]
    sub["interaction_matrix"] = np.asarray(prob["interaction_matrix"])[:, atoms][:, :, atoms]
    local = {}
    for basis, per in prob["samples"].get("Local", {}).items():
        local[basis] = {k: per[a] for k, a in enumerate(atoms) if a in per}
    sub["samples"] = {"Global": prob["samples"].get("Global", {}), "Local": local}
    return sub


def separation(setup: Setup, duration=GRID[-1]):
    """Sum over cross-cluster pairs of U_ij x duration (a condition, not a measurement)."""
    prob = assemble(setup.swapped(bad=()))
    u = np.asarray(prob["interaction_matrix"])[-1]
    owner = np.zeros(setup.n, dtype=int)
    for c, (_, atoms) in enumerate(setup.layout):
        owner[list(atoms)] = c
    cross = owner[:, None] != owner[None, :]
    return float(np.sum(np.triu(u * cross, 1)) * duration)


def permute_axes(t, flat):
    """``t`` has one axis per entry of ``flat`` (axis i = atom flat[i]) [+ trailing axes]: axis a = atom a."""
    order = list(np.argsort(flat)) + list(range(len(flat), t.ndim))
    return np.transpose(t, order)


def product_ket(setup: Setup):
    """The register's initial ket: the product of the cluster kets, atom 0 the highest bit."""
    t = np.ones((), dtype=complex)
    flat = []
    for name, atoms in setup.layout:
        sp = SPECIES[name]
        t = np.multiply.outer(t, species_ket(sp, setup.init).reshape((2,) * sp.size))
        flat += list(atoms)
    return np.ascontiguousarray(permute_axes(t, flat)).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the reference solve
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cluster_solve(name, pitch, diss, family, init, times, bad_local):
    from oracle import qutip_path as qp

    sp = SPECIES[name]
    one = Setup(sp.size, ((name, tuple(range(sp.size))),), diss, family, init, pitch, bad_local)
    ham = qp.build_hamiltonian(assemble(one))
    out = qp.mesolve(ham, species_ket(sp, init), np.asarray(times, dtype=float), max_step=1e-3, **qp.TIGHT)
    out = np.stack(out)
    out.setflags(write=False)
    return out


def solve_problem_clusters(prob, setup: Setup, times):
    """The cluster solutions of ANY problem on the register of ``setup`` (not cached): each cluster's sub-problem
    (:func:`sub_problem`) from its species' initial ket.  With ``prob = assemble(setup)`` this is what
    :func:`cluster_solutions` returns; the sensitivity checks pass an edited problem."""
    from oracle import qutip_path as qp

    out = []
    for name, atoms in setup.layout:
        ham = qp.build_hamiltonian(sub_problem(prob, atoms))
        out.append(np.stack(qp.mesolve(ham, species_ket(SPECIES[name], setup.init), np.asarray(times, dtype=float),
                                       max_step=1e-3, **qp.TIGHT)))
    return out


def cluster_solutions(setup: Setup, times):
    """Per cluster of ``setup``: complex[len(times), 2^k, 2^k], the tight Lindblad solution of its sub-problem (solved
    once per (species, pitch, dissipator case, family, initial ket, times, mask) and shared)."""
    times = tuple(float(t) for t in times)
    out = []
    for name, atoms in setup.layout:
        bad_local = tuple(k for k, a in enumerate(atoms) if a in setup.bad)
        out.append(_cluster_solve(name, setup.pitch, setup.diss, setup.family, setup.init, times, bad_local))
    return out


class Reference:
    """rho at one time as the tensor product of cluster matrices ``mats`` placed on the atoms of ``layout``."""

    def __init__(self, n, layout, mats):
        self.n = n
        self.clusters = [tuple(atoms) for _, atoms in layout]
        self.mats = [np.asarray(m, dtype=complex) for m in mats]
        self.flat = [a for atoms in self.clusters for a in atoms]

    def _sub(self, idx, atoms):
        """Cluster-local index of the register index ``idx`` (atom 0 of the cluster its highest bit)."""
        idx = np.asarray(idx, dtype=np.int64)
        out = np.zeros_like(idx)
        for a in atoms:
            out = (out << 1) | ((idx >> (self.n - 1 - a)) & 1)
        return out

    def entries(self, rows, cols):
        rows, cols = np.broadcast_arrays(np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))
        out = np.ones(rows.shape, dtype=complex)
        for atoms, m in zip(self.clusters, self.mats):
            out = out * m[self._sub(rows, atoms), self._sub(cols, atoms)]
        return out

    def _kron(self, vecs):
        t = np.ones((), dtype=complex)
        for atoms, v in zip(self.clusters, vecs):
            t = np.multiply.outer(t, np.asarray(v).reshape((2,) * len(atoms)))
        return np.ascontiguousarray(permute_axes(t, self.flat)).reshape(-1)

    def row(self, r):
        """Row r as a Kronecker product of cluster rows, permuted to the register's bit order."""
        return self._kron([m[int(self._sub(r, atoms))] for atoms, m in zip(self.clusters, self.mats)])

    def rows(self, rs):
        return np.stack([self.row(int(r)) for r in rs])

    def diagonal(self):
        return self._kron([np.diagonal(m) for m in self.mats])

    def trace(self):
        return complex(np.prod([np.trace(m) for m in self.mats]))

    def occupations(self):
        """<n_a> of every atom (n = |r><r|, local state 0); the traces of the other clusters are kept."""
        traces = [np.trace(m) for m in self.mats]
        out = np.zeros(self.n)
        for c, (atoms, m) in enumerate(zip(self.clusters, self.mats)):
            k = len(atoms)
            d = np.diagonal(m).reshape((2,) * k)
            rest = np.prod([t for j, t in enumerate(traces) if j != c])
            for pos, a in enumerate(atoms):
                out[a] = float(np.real(np.take(d, 0, axis=pos).sum() * rest))
        return out

    def matmul(self, v):
        """rho @ V for V complex[2^N, p]: every cluster factor applied along its own axes."""
        v = np.asarray(v, dtype=complex)
        p = v.shape[1]
        t = v.reshape((2,) * self.n + (p,))
        for atoms, m in zip(self.clusters, self.mats):
            k = len(atoms)
            mt = m.reshape((2,) * (2 * k))
            t = np.tensordot(mt, t, axes=(list(range(k, 2 * k)), list(atoms)))  # new axes first, in cluster order
            t = np.moveaxis(t, list(range(k)), list(atoms))
        return t.reshape(1 << self.n, p)

    def full(self):
        if self.n > 9:
            raise ValueError("the full matrix is formed up to 9 atoms only")
        k = [len(a) for a in self.clusters]
        t = np.ones((), dtype=complex)
        for m, kk in zip(self.mats, k):
            t = np.multiply.outer(t, m.reshape((2,) * (2 * kk)))
        # axes now: per cluster (row bits, column bits); wanted: row bit of atom 0 .. n-1, then the column bits
        src_row, src_col, pos = {}, {}, 0
        for atoms in self.clusters:
            for j, a in enumerate(atoms):
                src_row[a] = pos + j
                src_col[a] = pos + len(atoms) + j
            pos += 2 * len(atoms)
        order = [src_row[a] for a in range(self.n)] + [src_col[a] for a in range(self.n)]
        return np.ascontiguousarray(np.transpose(t, order)).reshape(1 << self.n, 1 << self.n)


def references(setup: Setup, times):
    """One :class:`Reference` per time."""
    sols = cluster_solutions(setup, times)
    return [Reference(setup.n, setup.layout, [s[i] for s in sols]) for i in range(len(times))]


def full_space_solution(setup: Setup, times):
    """The same problem on the full space (the floor of tests/test_lindblad_ref.py; up to 6 atoms)."""
    from oracle import qutip_path as qp

    ham = qp.build_hamiltonian(assemble(setup))
    return np.stack(qp.mesolve(ham, product_ket(setup), np.asarray(times, dtype=float), max_step=1e-3, **qp.TIGHT))


# ---------------------------------------------------------------------------------------------------------------------
# what the device tests compare at 10 to 14 atoms
# ---------------------------------------------------------------------------------------------------------------------
def probe_vectors(n, probes=4, seed=23):
    rng = np.random.default_rng([seed, n])
    v = rng.standard_normal((1 << n, probes)) + 1j * rng.standard_normal((1 << n, probes))
    return v / np.linalg.norm(v, axis=0)


def compared_rows(n, seed=29):
    d = 1 << n
    rng = np.random.default_rng([seed, n])
    return np.concatenate([[0, d - 1], rng.choice(np.arange(1, d - 1), 6, replace=False)]).astype(np.int64)


def compared_entries(setup: Setup, seed=31):
    """(rows, cols): 4096 seeded random entries, then the structured ones - the largest entry of the initial ket with all
    its single-flip neighbours, and its 16 largest entries (rows x columns of both sets: the largest entries of rho(0),
    among them pairs that differ in many bits, where a dissipator acts most) - and, for the Hermiticity check, the
    transposed of every pair (second half of the arrays)."""
    n, d = setup.n, 1 << setup.n
    rng = np.random.default_rng([seed, n])
    r = rng.integers(0, d, 4096)
    c = rng.integers(0, d, 4096)
    psi = np.abs(product_ket(setup))
    top = int(np.argmax(psi))
    for near in (np.array([top] + [top ^ (1 << b) for b in range(n)], dtype=np.int64),
                 np.argsort(-psi, kind="stable")[:16].astype(np.int64)):
        sr, sc = np.meshgrid(near, near, indexing="ij")
        r = np.concatenate([r, sr.ravel()])
        c = np.concatenate([c, sc.ravel()])
    return np.concatenate([r, c]).astype(np.int64), np.concatenate([c, r]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# pair passes (host_handle.hpp: plan_passes, master equation with double-flip dissipators), restated
# ---------------------------------------------------------------------------------------------------------------------
def auto_tile_bits(nb, batch=1):
    """ryd_create's choice of the tile size for ``tile_bits = 0`` (master equation: no 2^13 tile)."""
    def passes(t):
        return 1 if nb <= t else 1 + (nb - t + (t - 5)) // (t - 4)

    best = 12
    for t in range(12, 7, -1):
        if passes(t) > passes(12):
            break
        best = t
        if (batch << max(nb - t, 0)) >= 256:
            break
    return best


def pair_pass_groups(n, batch=1, tile_bits=0):
    """The atoms of every pair pass: atoms are taken from the low-bit end (atom N - 1 first), ``T // 2`` in the first
    pass, ``(T - c) // 2`` in the later ones, which keep ``c = min(4, done, T - 2)`` run bits in the tile."""
    nb = 2 * n
    t = min(tile_bits or auto_tile_bits(nb, batch), nb)
    groups, done, first = [], 0, True
    while done < n:
        if first:
            g = min(n, max(1, t // 2))
        else:
            c = max(0, min(min(4, done), t - 2))
            g = min(n - done, max(1, (t - c) // 2))
        groups.append([n - 1 - (done + j) for j in range(g)])
        done += max(g, 1)
        first = False
    return groups


# ---------------------------------------------------------------------------------------------------------------------
# the case table of the device tests
# ---------------------------------------------------------------------------------------------------------------------
PARTS = {
    4: ("pair", "pair'"), 5: ("tri3", "pair"), 6: ("chain3", "tri3"), 7: ("rhomb4", "tri3"),
    8: ("square4", "chain3", "one"), 9: ("rhomb4", "tri3", "pair'"), 10: ("square4", "chain3", "pair", "one"),
    11: ("rhomb4", "square4", "tri3"), 12: ("square4", "rhomb4", "chain3", "one"),
    13: ("rhomb4", "square4", "tri3", "pair'"), 14: ("square4", "rhomb4", "chain3", "pair", "one"),
}
# a second split of the same size for the batches of different registers
PARTS_B = {4: ("chain3", "one"), 5: ("square4", "one"), 6: ("rhomb4", "pair'"), 11: ("square4", "chain3", "pair", "pair'")}
PARTS_C = {4: ("tri3", "one"), 5: ("chain3", "pair'"), 6: ("tri3", "pair'", "one")}


def scrambled(n, salt=0):
    """A fixed permutation of the atom indices that puts atom 0 and atom n - 1 into the first cluster and spreads every
    cluster of two or more atoms over both sides of every pair-pass boundary (checked by tests/test_lindblad_ref.py)."""
    rng = np.random.default_rng([41, n, salt])
    mid = [int(v) for v in rng.permutation(np.arange(1, n - 1))]
    return [0, n - 1] + mid if n > 2 else list(range(n))


def default_layout(n, parts=None, salt=0):
    parts = parts or PARTS[n]
    # the first cluster has at least two atoms wherever the register has such a cluster: it gets atoms 0 and n - 1
    parts = tuple(sorted(parts, key=lambda s: -SPECIES[s].size))
    return layout_of(n, parts, scrambled(n, salt))


@dataclass(frozen=True)
class Case:
    plan: str
    setups: tuple                   # one Setup per batch entry
    path: tuple = ()                # set_path keyword arguments, as sorted items
    tile_bits: int = 0
    tag: str = ""

    @property
    def n(self):
        return self.setups[0].n

    @property
    def times(self):
        return EVAL if self.n <= 12 else EVAL_BIG

    @property
    def name(self):
        s = self.setups[0]
        bits = [self.plan, f"n{s.n}", s.diss, s.family]
        if s.init != "ket":
            bits.append(s.init)
        if s.pitch != "blockade":
            bits.append(s.pitch)
        if len(self.setups) > 1:
            bits.append(f"batch{len(self.setups)}")
        if self.tag:
            bits.append(self.tag)
        return "-".join(bits)


def _table():
    cases = []

    def add(plan, n, diss, family, path=None, tile_bits=0, tag="", init="ket", pitch="blockade", setups=None):
        if setups is None:
            setups = (Setup(n, default_layout(n), diss, family, init, pitch),)
        cases.append(Case(plan, tuple(setups), tuple(sorted((path or {}).items())), tile_bits, tag))

    # persistent k_traj_dm (default path)
    for n in (4, 5, 6):
        for diss in DISS_CASES:
            add("persistent", n, diss, "complex")
        for diss in ("dephasing", "all"):
            add("persistent", n, diss, "global")
        add("persistent", n, "all", "complex", init="ground")
        lay = [default_layout(n), default_layout(n, PARTS_B[n], 1), default_layout(n, PARTS_C[n], 2)]
        add("persistent", n, "all", "complex", setups=[Setup(n, l, "all", "complex") for l in lay])
        # one entry with a badly prepared atom (atom 1: inside a cluster of the scrambled layouts)
        add("persistent", n, "all", "global", tag="bad-atom",
            setups=[Setup(n, lay[0], "all", "global"), Setup(n, lay[1], "all", "global", bad=(1,))])
    # tiled multi-launch kernels
    for diss in DISS_CASES:
        add("tiled", 5, diss, "complex", {"force_generic": True}, tile_bits=6, tag="t6")
        add("tiled", 7, diss, "complex", {"force_generic": True}, tile_bits=0, tag="t0")
        add("tiled", 7, diss, "complex", {"force_generic": True}, tile_bits=7, tag="t7")
    for n in (8, 9):
        for diss in DOUBLE_FLIP:
            add("tiled", n, diss, "complex", {"force_generic": True})
    add("tiled-single-launch", 7, "dephasing", "complex", {"force_generic": True, "no_tile14": True})
    # Hermitian path: k_apply14 row pass + k_symm
    for n in (7, 8, 9, 10):
        for diss in ("dephasing", "slow-dephasing"):
            path = {"force_generic": False, "force_tile14": True}
            if n == 10:
                path["no_ket"] = True
            add("hermitian", n, diss, "complex", path)
    # polynomial rows: k_ket ROWS + k_transpose_conj
    for n in (10, 11):
        for diss in ("dephasing", "slow-dephasing"):
            add("rows-ket", n, diss, "real", {"force_generic": False})
    add("rows-ket", 10, "slow-dephasing", "real", {"force_generic": False, "no_merge": True}, tag="no-merge")
    add("rows-ket", 10, "slow-dephasing", "real", {"force_generic": False}, init="ground")
    for n in (12, 13):
        for diss in ("dephasing", "slow-dephasing"):
            add("rows-ket", n, diss, "real", {"force_generic": False, "rows_ket": True})
    add("rows-ket", 14, "slow-dephasing", "real", {"force_generic": False, "rows_ket": True})
    add("rows-ket-by-estimate", 12, "slow-dephasing", "real", {"force_generic": False}, pitch="tight")
    # split-operator rows: k_split_reg<N, 5, false, ROWS>
    for n in (12, 13, 14):
        add("rows-split", n, "slow-dephasing", "real", {"force_generic": False})
    add("rows-split", 12, "slow-dephasing", "real", {"force_generic": False}, init="ground")
    # rows with k_local_exp
    for n in (10, 11, 12, 13):
        for diss in DOUBLE_FLIP:
            add("rows-local-exp", n, diss, "real", {"force_generic": False})
    add("rows-local-exp", 14, "all", "real", {"force_generic": False})
    add("rows-local-exp", 11, "all", "real", {"force_generic": False},
        setups=[Setup(11, default_layout(11), "all", "real"), Setup(11, default_layout(11, PARTS_B[11], 1), "all", "real")])
    # multi-launch Lindbladian with pair passes at row-path sizes
    for n in (10, 11):
        add("pair-passes", n, "all", "real", {"force_generic": False, "no_ket": True})
    return cases


CASES = _table()


# ---------------------------------------------------------------------------------------------------------------------
# figures (what tests/test_lindblad_ref.py asserts)
# ---------------------------------------------------------------------------------------------------------------------
FLOOR_LAYOUTS = (
    (4, ("pair", "pair'"), (0, 2, 1, 3)),
    (5, ("tri3", "pair"), (0, 2, 4, 1, 3)),
    (6, ("chain3", "tri3"), (0, 2, 4, 1, 3, 5)),
    (6, ("pair", "pair'", "pair"), (0, 3, 1, 4, 2, 5)),
)


def floor_setups():
    """What the cluster product is compared with the full-space oracle on: every dissipator case x {complex, real} x both
    initial states at the 4- and 5-atom layouts; at 6 atoms (2.5 s per full-space solve) every dissipator case twice, with
    both families and both initial states between the two runs, which alternate between the two layouts; the global drive with "dephasing" and "all" at 4 and 5 atoms."""
    out = []
    for li, (n, parts, perm) in enumerate(FLOOR_LAYOUTS):
        lay = layout_of(n, parts, perm)
        for di, diss in enumerate(DISS_CASES):
            for fi, family in enumerate(("complex", "real")):
                for ii, init in enumerate(("ket", "ground")):
                    if n < 6 or ((fi == ii) == (di % 2 == 0) and fi == li % 2):
                        out.append(Setup(n, lay, diss, family, init))
    for n, parts, perm in FLOOR_LAYOUTS[:2]:
        for diss in ("dephasing", "all"):
            out.append(Setup(n, layout_of(n, parts, perm), diss, "global", "ket"))
    return out


def floor_error(setup, times=EVAL):
    full = full_space_solution(setup, times)
    refs = references(setup, times)
    return max(float(np.max(np.abs(r.full() - f))) for r, f in zip(refs, full))


def motion(setup, times):
    """(max |rho(t_end) - rho(0)|, max |rho(t_end) - rho(t_end) without collapse operators|) over the compared entries
    (the whole matrix up to 9 atoms)."""
    refs = references(setup, times)
    free = references(setup.swapped(diss="none"), times)

    def values(ref):
        if setup.n <= 9:
            return ref.full().ravel()
        r, c = compared_entries(setup)
        return np.concatenate([ref.entries(r, c), ref.rows(compared_rows(setup.n)[:2]).ravel()])

    a, b, c = values(refs[-1]), values(refs[0]), values(free[-1])
    return float(np.max(np.abs(a - b))), float(np.max(np.abs(a - c)))


def _report(out=print):
    t0 = time.perf_counter()
    seen = {}
    for case in CASES:
        for s in case.setups:
            seen.setdefault((s, case.times), case.name)
    worst_sep = 0.0
    for (s, times), name in seen.items():
        references(s, times)
        worst_sep = max(worst_sep, separation(s))
    t_ref = time.perf_counter() - t0
    out(f"{len(CASES)} cases, {len(seen)} distinct (register, times), {_cluster_solve.cache_info().currsize} cluster solves: "
        f"{t_ref:.1f} s CPU; largest separation sum {worst_sep:.2e} (bar {SEPARATION_BAR:g})")
    mv = [(motion(s, times), name) for (s, times), name in seen.items()]
    out(f"motion: smallest |rho(T) - rho(0)| {min(m[0][0] for m in mv):.2e}, smallest effect of the dissipator "
        f"{min(m[0][1] for m in mv):.2e} ({min(mv, key=lambda m: m[0][1])[1]})")
    t0 = time.perf_counter()
    errs = [(floor_error(s), s) for s in floor_setups()]
    worst = max(errs, key=lambda e: e[0])
    out(f"floor: max |cluster product - full space| over {len(errs)} comparisons = {worst[0]:.2e} "
        f"(n = {worst[1].n}, {worst[1].diss}, {worst[1].family}, {worst[1].init}); {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    _report()

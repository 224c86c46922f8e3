"""Cluster-product reference for the two-level Schroedinger path above 14 atoms, and the case table of the device tests
(tests/test_ket_cluster_ref.py, tests/test_gpu_ket_clusters.py): NumPy, SciPy, the repository's ``oracle`` and torch (on
the CPU in the CPU tests, on the device in the GPU tests).

A register is made of small clusters (1 to 6 atoms, :data:`SHAPES`: a line, a triangle, a square, a rhombus, a 5-atom
cross, a 2 x 3 patch).  Atoms interact strongly inside a cluster - at the blockade pitch (U = 12.6 rad/us between
neighbours) or at a tight 6 um (U = 116 rad/us) - and the cluster centres sit on a line 1000 um apart, so that the summed
cross-cluster interaction times the duration is below 1e-10 (:func:`separation`).  The exact ket is then the tensor
product of the cluster kets, each one a tight oracle solve on at most 64 amplitudes (:func:`cluster_solutions`, cached).
:func:`product` forms the whole 2^N ket by index arithmetic (on the device at 15 - 25 atoms), so EVERY amplitude is
compared.  Atom 0 is the highest bit.

Unlike tests/lindblad_ref.py, whose waveforms are seeded per species, waveforms and initial kets are seeded here per
(register seed, cluster instance, atom): no two atoms of a register are alike even when a 25-atom register repeats a
cluster shape.  The atoms of the clusters are scattered over the atom indices (:func:`scatter`) so that, for every plan a
register runs on (:func:`split_plan`, :func:`apply_plan`: the host's tilings restated), every pair of bit classes is
straddled by an interacting pair and every class of two or more bits holds one: a high-bit group placed on the wrong
bits, two atoms' coefficients exchanged, an E0 entry read at the wrong index are O(0.01 - 1) errors.

What the reference cannot see: couplings of more than 6 atoms.  A defect that shows only when more than six atoms
interact (an interaction diagonal wrong for seven or more excitations, a splitting error that grows with the number of
coupled neighbours) stays with ``ns_rect16_anneal.npz`` and the path-against-path tests of tests/test_gpu_split.py.

Reference floor (measured: ``python tests/ket_cluster_ref.py``, asserted by tests/test_ket_cluster_ref.py): the cluster
product against the full-space oracle, both under ``qp.TIGHT``, 20 ns at 8 to 12 atoms: :data:`FLOOR_MEASURED`
(max-abs, 2-norm); the test allows :data:`FLOOR_FACTOR` times that.

``python tests/ket_cluster_ref.py`` prints the figures the CPU tests assert (floor, separation sums, motion, sensitivity)
and the CPU time of all references of :data:`CASES`.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root holds ``oracle`` and ``pulser_amd``
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lindblad_ref import auto_tile_bits, blockade_pitch, permute_axes, sub_problem

from pulser_amd import problem as P

AMP_TOL = 1e-7          # the project's parity bar on every amplitude
NORM_BAR = 1e-7         # ... and on the 2-norm of the error (the controller's budget SPLIT_BUDGET = 8e-8 is a 2-norm bound)
SPLIT_BUDGET = 8e-8     # helpers.SPLIT_BUDGET (host_split.hpp: kSplitTolTotal)
CENTRE_PITCH = 1000.0   # um between cluster centres
SEPARATION_BAR = 1e-10  # sum over cross-cluster pairs of U_ij x duration
TIGHT_PITCH = 6.0       # um: U = 116 rad/us between neighbours
NEIGHBOUR = 1.5         # pitches: atoms of a cluster up to this far apart count as an interacting pair (U >= 1.1 rad/us)

# measured by `python tests/ket_cluster_ref.py` over :func:`floor_setups`: (max-abs, 2-norm) of product - full space
FLOOR_MEASURED = (4.2e-12, 8.7e-12)
FLOOR_FACTOR = 5.0

FAMILIES = ("complex", "real", "global")

_H = float(np.sqrt(3) / 2)
SHAPES = {  # positions in units of the pitch
    "one": ((0.0, 0.0),),
    "line2": ((0.0, 0.0), (1.0, 0.0)),
    "line3": ((0.0, 0.0), (1.0, 0.0), (2.0, 0.0)),
    "tri3": ((0.0, 0.0), (1.0, 0.0), (0.5, _H)),
    "square4": ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)),
    "rhomb4": ((0.0, 0.0), (1.0, 0.0), (0.5, _H), (1.5, _H)),
    "cross5": ((0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)),
    "patch6": ((0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (0.0, 1.0), (1.0, 1.0), (2.0, 1.0)),
}


def shape_pairs(name):
    """The interacting pairs (local atom numbers) of a cluster shape: at most :data:`NEIGHBOUR` pitches apart."""
    pos = np.asarray(SHAPES[name])
    return [(i, j) for i, j in itertools.combinations(range(len(pos)), 2)
            if np.linalg.norm(pos[i] - pos[j]) <= NEIGHBOUR + 1e-9]


# ---------------------------------------------------------------------------------------------------------------------
# registers
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Setup:
    """One register and its problem: ``layout`` = ((shape name, atom indices), ...); hashable.  ``ns``: the duration
    in ns (``ns + 1`` samples); ``boost`` scales the drive amplitudes (the short large-ket cases)."""
    n: int
    layout: tuple
    family: str = "complex"
    init: str = "ket"               # or "ground"
    pitch: str = "blockade"         # or "tight"
    ns: int = 20
    boost: float = 1.0
    seed: int = 0
    centre_pitch: float = CENTRE_PITCH

    def swapped(self, **kw):
        return dataclasses.replace(self, **kw)

    @property
    def t_end(self):
        return self.ns * 1e-3

    @property
    def pairs(self):
        """The interacting pairs of the register, as atom indices."""
        return [(atoms[i], atoms[j]) for name, atoms in self.layout for i, j in shape_pairs(name)]


def layout_of(n, parts, perm=None):
    """((shape, atoms), ...) with the clusters of ``parts`` placed, in order, on the atom indices ``perm``."""
    perm = list(range(n)) if perm is None else [int(p) for p in perm]
    assert sorted(perm) == list(range(n)) and sum(len(SHAPES[s]) for s in parts) == n, (n, parts, perm)
    out, pos = [], 0
    for s in parts:
        k = len(SHAPES[s])
        out.append((s, tuple(perm[pos:pos + k])))
        pos += k
    return tuple(out)


def _grid(setup):
    return np.arange(setup.ns + 1) / 1000.0


def atom_waveform(setup: Setup, c: int, k: int):
    """Samples of atom ``k`` of cluster instance ``c``, seeded by (register seed, c, k).  "complex": amplitude, detuning and
    phase all depend on time (the phase-gauge path); "real": phase 0."""
    rng = np.random.default_rng([setup.seed, c, k, 1])
    t = _grid(setup)
    a, b, d = rng.uniform(2, 12, 3)
    w0, w1, w2, p0 = rng.uniform(0.0, 2 * np.pi, 4)
    phase = (p0 + 0.6 * np.sin(40.0 * t + w2)) if setup.family == "complex" else np.zeros(len(t))
    return {"amp": setup.boost * a * (1 + 0.5 * np.sin(25.0 * t + w0)), "det": b * np.cos(30.0 * t + w1) - d, "phase": phase}


def global_waveform(setup: Setup):
    """The one global real drive of the "global" family."""
    t = _grid(setup)
    return {"amp": setup.boost * 9.0 * (1 + 0.3 * np.sin(25.0 * t)), "det": 7.0 * np.cos(20.0 * t) - 5.0,
            "phase": np.zeros(len(t))}


def cluster_ket(setup: Setup, c: int):
    """"ket": a seeded random normalised (entangled) ket of cluster instance ``c``; "ground": |g...g>."""
    d = 1 << len(setup.layout[c][1])
    if setup.init == "ground":
        v = np.zeros(d, dtype=complex)
        v[-1] = 1.0
        return v
    rng = np.random.default_rng([setup.seed, c, 2])
    v = rng.normal(size=d) + 1j * rng.normal(size=d)
    return v / np.linalg.norm(v)


def assemble(setup: Setup):
    """The full problem (``P.make_ising_problem`` + per-atom samples)."""
    n = setup.n
    pitch = blockade_pitch() if setup.pitch == "blockade" else TIGHT_PITCH
    coords = np.zeros((n, 2))
    loc = {}
    for c, (name, atoms) in enumerate(setup.layout):
        for k, a in enumerate(atoms):
            coords[a] = np.asarray(SHAPES[name][k]) * pitch + np.array([c * setup.centre_pitch, 0.0])
            if setup.family != "global":
                loc[a] = atom_waveform(setup, c, k)
    zero = np.zeros(setup.ns + 1)
    glob = global_waveform(setup) if setup.family == "global" else {"amp": zero, "det": zero, "phase": zero}
    prob = P.make_ising_problem(coords, glob)
    if setup.family != "global":
        prob["samples"] = {"Global": {}, "Local": {"ground-rydberg": {a: loc[a] for a in sorted(loc)}}}
    return prob


def separation(setup: Setup):
    """Sum over cross-cluster pairs of U_ij x duration (a condition, not a measurement)."""
    u = np.asarray(assemble(setup)["interaction_matrix"])[-1]
    owner = np.zeros(setup.n, dtype=int)
    for c, (_, atoms) in enumerate(setup.layout):
        owner[list(atoms)] = c
    cross = owner[:, None] != owner[None, :]
    return float(np.sum(np.triu(u * cross, 1)) * setup.t_end)


# ---------------------------------------------------------------------------------------------------------------------
# the reference solve
# ---------------------------------------------------------------------------------------------------------------------
def solve_problem_clusters(prob, setup: Setup, times):
    """The cluster solutions of ANY problem on the register of ``setup`` (not cached): complex[len(times), 2^k] per
    cluster, its sub-problem (lindblad_ref.sub_problem) from its own initial ket under ``qp.TIGHT``."""
    from oracle import qutip_path as qp

    out = []
    for c, (_, atoms) in enumerate(setup.layout):
        ham = qp.build_hamiltonian(sub_problem(prob, atoms))
        out.append(np.stack(qp.sesolve(ham, cluster_ket(setup, c), np.asarray(times, dtype=float), max_step=1e-3, **qp.TIGHT)))
    return out


@functools.lru_cache(maxsize=None)
def cluster_solutions(setup: Setup, times):
    """Per cluster of ``setup``: complex[len(times), 2^k], read-only, solved once per (register, times)."""
    out = solve_problem_clusters(assemble(setup), setup, times)
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def product(layout, cluster_kets, n, device="cpu"):
    """The 2^N ket of the clusters' kets as a complex128 torch tensor on ``device``, atom 0 the highest bit, by index
    arithmetic: per cluster, the cluster's bits of ``arange(2^N)`` gathered into a sub-index (the cluster's atom 0 its
    highest bit), the cluster ket indexed with it, the factors multiplied in cluster order.  The same function builds
    the initial ket and every reference ket; intermediates are freed as it goes (25 atoms: about 1 GiB beside the
    result)."""
    import torch

    idx = torch.arange(1 << n, dtype=torch.int64, device=device)
    out = None
    for (_, atoms), ket in zip(layout, cluster_kets):
        sub = torch.zeros_like(idx)
        for a in atoms:
            sub.mul_(2).add_((idx >> (n - 1 - a)) & 1)
        factor = torch.from_numpy(np.array(ket, dtype=np.complex128)).to(device)[sub]
        del sub
        out = factor if out is None else out.mul_(factor)
        del factor
    return out


def product_numpy(setup: Setup, kets):
    """The same ket as an explicit outer product + axis permutation (what :func:`product` is checked against)."""
    t = np.ones((), dtype=complex)
    flat = []
    for (_, atoms), v in zip(setup.layout, kets):
        t = np.multiply.outer(t, np.asarray(v).reshape((2,) * len(atoms)))
        flat += list(atoms)
    return np.ascontiguousarray(permute_axes(t, flat)).reshape(-1)


def initial_kets(setup: Setup):
    return [cluster_ket(setup, c) for c in range(len(setup.layout))]


def product_distance(kets_a, kets_b):
    """|a - b|_2 of two product kets over the SAME clusters, from the cluster kets alone."""
    na = np.prod([np.vdot(a, a).real for a in kets_a])
    nb = np.prod([np.vdot(b, b).real for b in kets_b])
    ov = np.prod([np.vdot(a, b) for a, b in zip(kets_a, kets_b)])
    return float(np.sqrt(max(na + nb - 2.0 * ov.real, 0.0)))


def exchange_distance(setup: Setup, kets, a, b):
    """|psi - SWAP_ab psi|_2 for atoms a, b of DIFFERENT clusters of the product ket psi: 2 - 2 tr(rho_a rho_b) with the
    one-atom reduced density matrices (what placing the two atoms on each other's bits does to the ket)."""
    def reduced(atom):
        for (name, atoms), v in zip(setup.layout, kets):
            if atom in atoms:
                t = np.moveaxis(np.asarray(v).reshape((2,) * len(atoms)), atoms.index(atom), 0).reshape(2, -1)
                return t @ t.conj().T
        raise KeyError(atom)

    return float(np.sqrt(max(2.0 - 2.0 * np.trace(reduced(a) @ reduced(b)).real, 0.0)))


def full_space_solution(setup: Setup, times):
    """The same problem on the full space (the floor of tests/test_ket_cluster_ref.py; up to 12 atoms)."""
    from oracle import qutip_path as qp

    ham = qp.build_hamiltonian(assemble(setup))
    psi0 = product_numpy(setup, initial_kets(setup))
    return np.stack(qp.sesolve(ham, psi0, np.asarray(times, dtype=float), max_step=1e-3, **qp.TIGHT))


# ---------------------------------------------------------------------------------------------------------------------
# plans (host_split.hpp: split_tile_bits / split_plan; host_handle.hpp: ryd_create / plan_passes for kets), restated
# ---------------------------------------------------------------------------------------------------------------------
def split_tile_bits(n, small_tiles=False):
    return 13 if (21 <= n <= 22 and not small_tiles) else min(n, 12)


def split_plan(n, small_tiles=False):
    """The tilings of the split-operator passes as lists of bits: the low T bits, then one tiling per group of high bits
    (at most T - 4 each, spread evenly) that keeps the low T - n_high bits."""
    t = split_tile_bits(n, small_tiles)
    tilings = [list(range(t))]
    rem, at = n - t, t
    if rem > 0:
        cap = t - 4
        extra = (rem + cap - 1) // cap
        for e in range(extra):
            nh = rem // (extra - e)
            tilings.append(list(range(t - nh)) + list(range(at, at + nh)))
            at += nh
            rem -= nh
    return tilings


def split_passes(n, small_tiles=False):
    """``ryd_stats.passes`` of a split-operator run: passes over the ket per stage."""
    m = len(split_plan(n, small_tiles))
    return m - 1 if m > 1 else 1


def high_groups(n, small_tiles=False):
    """(offset, length) of every high-bit group."""
    t = split_tile_bits(n, small_tiles)
    out = []
    for til in split_plan(n, small_tiles)[1:]:
        high = [b for b in til if b >= t]
        out.append((high[0], len(high)))
    return out


def apply_plan(n, batch=1):
    """The ``k_apply`` plan of a two-level ket (``method="taylor"``, automatic tile size): (tilings, passes).  States up to
    128 MiB with at most 10 bits outside the tile run in ONE launch (the tile in LDS, the partner of every higher bit read
    from another tile: the second "tiling" lists those outer bits); beyond that a first pass on 2^14 register tiles where
    the launch has 512 of them (else 2^T), then passes of the remaining bits spread evenly, each beside the low run bits."""
    nb = n
    log_b = int(np.ceil(np.log2(batch)))
    passes = lambda t: 1 if nb <= t else 1 + (nb - t + (t - 5)) // (t - 4)  # noqa: E731
    t = auto_tile_bits(nb, batch)
    if passes(13) < passes(12) and (batch << max(nb - 13, 0)) >= 128:
        t = 13
    t = min(t, nb)
    tiles14 = batch << max(nb - 14, 0)
    p12, p14 = 1 + (max(nb - 12, 0) + 7) // 8, 1 + (nb - 14 + 7) // 8
    tile14 = nb >= 14 and (tiles14 >= 512 or (p14 < p12 and tiles14 >= 48))
    ts = max(min(12, max(9, nb + log_b - 8)), nb - 10) if nb > t else t
    if nb > t and nb > ts and nb - ts <= 10 and (batch * 16 << nb) <= (128 << 20) and not (tile14 and nb == 14):
        return [list(range(ts)), list(range(ts, nb))], 1
    tilings, done, first = [], 0, True
    while done < nb:
        if first:
            g = 14 if tile14 else t
            tilings.append(list(range(min(g, nb))))
        else:
            cmin = max(0, min(min(4, done), t - 1))
            cap = max(1, t - cmin)
            left = nb - done
            k = (left + cap - 1) // cap
            g = max(1, (left + k - 1) // k)
            c = cmin
            lb = int(np.floor(np.log2(batch)))
            while c + g < t and c < done and (nb - (c + 1 + g)) + lb >= 10:
                c += 1
            tilings.append(list(range(c)) + list(range(done, done + g)))
        done += max(g, 1)
        first = False
    return tilings, len(tilings)


def bit_classes(tilings, n):
    """The bits 0 .. n - 1 (bit = N - 1 - atom) in classes: the low 4 tile bits; the tile bits beyond them that a later
    tiling keeps; the tile bits that only the first tiling holds; each high-bit group.  (Where two high groups differ in
    length by one - 23 and 25 atoms - the tiling of the shorter group keeps one bit more than the other.  That bit is
    counted with the kept bits: as a class of its own it would need partners in five other classes, one of them the two
    kept bits, which have to share a cluster themselves - more than a cluster of six atoms can give.)"""
    first = set(tilings[0])
    sig = {}
    for b in range(n):
        if b < 4:
            key = (0, "low4")
        elif b in first:
            key = (1, "kept") if any(b in til for til in tilings[1:]) else (2, "first")
        else:
            key = (3, next(i for i, til in enumerate(tilings) if b in til))
        sig.setdefault(key, []).append(b)
    return [sig[k] for k in sorted(sig)]


def plans_of(n, plans):
    """{plan name: bit classes} of the plans a register runs on: "split", "split-small" (2^12 tiles at 21 - 22 atoms),
    "taylor"."""
    out = {}
    for p in plans:
        if p == "split":
            out[p] = bit_classes(split_plan(n), n)
        elif p == "split-small":
            out[p] = bit_classes(split_plan(n, True), n)
        elif p == "taylor":
            out[p] = bit_classes(apply_plan(n)[0], n)
        else:
            raise KeyError(p)
    return out


def coverage_gaps(n, pairs, classes):
    """The conditions a layout misses on one plan: pairs of bit classes no interacting pair straddles, and classes of two
    or more bits that hold no interacting pair."""
    cls = {}
    for i, bits in enumerate(classes):
        for b in bits:
            cls[b] = i
    seen = {tuple(sorted((cls[n - 1 - a], cls[n - 1 - b]))) for a, b in pairs}
    want = {(i, j) for i in range(len(classes)) for j in range(i + 1, len(classes))}
    want |= {(i, i) for i, bits in enumerate(classes) if len(bits) >= 2}
    return sorted(want - seen)


def scatter(n, parts, plans, seed=0):
    """A seeded permutation of the atom indices on which the clusters of ``parts`` meet every condition of
    :func:`coverage_gaps` on every plan of ``plans``: random swaps that never add a gap, from a random start."""
    rng = np.random.default_rng([53, n, seed])
    classes = list(plans_of(n, plans).values())
    local = [(pos + i, pos + j) for pos, s in zip(np.cumsum([0] + [len(SHAPES[s]) for s in parts[:-1]]), parts)
             for i, j in shape_pairs(s)]

    tables = []
    for c in classes:
        cls = np.zeros(n, dtype=int)
        for i, bits in enumerate(c):
            cls[[n - 1 - b for b in bits]] = i      # indexed by ATOM
        want = {(i, j) for i in range(len(c)) for j in range(i + 1, len(c))} | {(i, i) for i, bits in enumerate(c) if len(bits) >= 2}
        tables.append((cls, want))

    def gaps(perm):
        total = 0
        for cls, want in tables:
            seen = set()
            for i, j in local:
                x, y = cls[perm[i]], cls[perm[j]]
                seen.add((x, y) if x <= y else (y, x))
            total += len(want - seen)
        return total

    for _ in range(20):
        perm = [int(v) for v in rng.permutation(n)]
        g = gaps(perm)
        for _ in range(4000):
            if g == 0:
                return layout_of(n, parts, perm)
            i, j = (int(v) for v in rng.choice(n, 2, replace=False))
            perm[i], perm[j] = perm[j], perm[i]
            g2 = gaps(perm)
            if g2 <= g:
                g = g2
            else:
                perm[i], perm[j] = perm[j], perm[i]
    raise RuntimeError(f"no layout of {parts} on {n} atoms covers {plans}")


# ---------------------------------------------------------------------------------------------------------------------
# the case table of the device tests
# ---------------------------------------------------------------------------------------------------------------------
PARTS = {
    8: ("patch6", "line2"), 9: ("cross5", "square4"), 10: ("patch6", "rhomb4"), 11: ("patch6", "cross5"),
    12: ("patch6", "tri3", "line3"), 13: ("patch6", "cross5", "line2"), 14: ("patch6", "cross5", "tri3"),
    15: ("patch6", "cross5", "square4"), 17: ("patch6", "cross5", "rhomb4", "line2"),
    20: ("patch6", "cross5", "square4", "rhomb4", "one"), 21: ("patch6", "patch6", "cross5", "square4"),
    22: ("patch6", "patch6", "cross5", "rhomb4", "one"), 23: ("patch6", "patch6", "cross5", "square4", "line2"),
    24: ("patch6", "patch6", "cross5", "square4", "tri3"), 25: ("patch6", "patch6", "cross5", "rhomb4", "square4"),
}
PARTS_B = {17: ("patch6", "square4", "tri3", "line3", "one")}  # the second register of the batch
PLANS = {  # the plans a register of this size runs on in the table
    10: ("split",), 13: ("split",), 14: ("split",), 15: ("split",), 17: ("split", "taylor"), 20: ("split",),
    21: ("split", "split-small", "taylor"), 22: ("split", "split-small"), 23: ("split",), 24: ("taylor",), 25: ("split",),
}


@functools.lru_cache(maxsize=None)
def default_layout(n, parts=None, salt=0):
    return scatter(n, parts or PARTS[n], PLANS.get(n, ("split",)), salt)


def _ns(n):
    return 20 if n <= 20 else 8 if n <= 22 else 6


def _boost(n):
    return 1.0 if n <= 20 else 3.0


def setup_of(n, family="complex", init="ket", pitch="blockade", parts=None, salt=0):
    """The register of the table at ``n`` atoms (one layout per size and composition, shared by the families and
    plans).  Durations: 20 ns up to 20 atoms, 8 ns at 21 - 22, 6 ns from 23 atoms on, there with drives three times as
    strong (the sensitivity condition of tests/test_ket_cluster_ref.py)."""
    return Setup(n, default_layout(n, parts, salt), family, init, pitch, _ns(n), _boost(n), seed=100 * n + salt)


@dataclass(frozen=True)
class Case:
    plan: str                       # "split", "split-small", "taylor"
    setups: tuple                   # one Setup per batch entry
    path: tuple = ()                # set_path keyword arguments, as sorted items
    method: str = "auto"
    times: tuple = ()
    tag: str = ""

    @property
    def n(self):
        return self.setups[0].n

    @property
    def name(self):
        s = self.setups[0]
        bits = [self.plan, f"n{s.n}", s.family]
        if s.init != "ket":
            bits.append(s.init)
        if s.pitch != "blockade":
            bits.append(s.pitch)
        if len(self.setups) > 1:
            bits.append(f"batch{len(self.setups)}")
        if self.tag:
            bits.append(self.tag)
        return "-".join(bits)

    @property
    def controlled(self):
        """Does the step-size controller of the split-operator path run?"""
        return self.plan != "taylor" and not dict(self.path).get("split_fixed", False)


def eval_times(ns, knot_pair=False):
    """t = 0, a time between two knots, the end; ``knot_pair``: two more inside one knot interval."""
    t = [0.0, (0.35 * ns + 0.37) * 1e-3, ns * 1e-3]
    if knot_pair:
        t[2:2] = [(0.5 * ns + 0.5) * 1e-3, (0.5 * ns + 0.7) * 1e-3]
    return tuple(round(v, 9) for v in t)


def _table():
    cases = []

    def add(plan, n, family, path=None, method="auto", tag="", init="ket", pitch="blockade", setups=None, knot_pair=False):
        if setups is None:
            setups = (setup_of(n, family, init, pitch),)
        cases.append(Case(plan, tuple(setups), tuple(sorted((path or {}).items())), method,
                          eval_times(setups[0].ns, knot_pair), tag))

    # split passes on the default path: k_split_s<12> in tan form, two tilings with 3 / 5 / 8 high bits
    for n in (15, 17, 20):
        add("split", n, "complex")
        add("split", n, "real", knot_pair=(n == 17))
    add("split", 17, "global")
    add("split", 15, "complex", init="ground")
    add("split", 15, "real", pitch="tight")
    # drives ten times as strong (up to 180 rad/us): the step-size controller has to cut the sub-steps
    add("split", 15, "real", tag="strong", setups=[dataclasses.replace(setup_of(15, "real"), boost=10.0)])
    # a batch of two different 17-atom registers: e0_stride != 0
    add("split", 17, "complex", setups=[setup_of(17, "complex"), setup_of(17, "complex", parts=PARTS_B[17], salt=1)])
    # 2^13 tiles (k_split_s<13>) and the same registers on two passes of 2^12 tiles
    for n in (21, 22):
        for family in ("real", "complex"):
            add("split", n, family)
            add("split-small", n, family, {"split_small_tiles": True})
    add("split", 21, "real", init="ground", pitch="tight")
    add("split", 22, "complex", {"split_fixed": True}, tag="fixed")
    # three tilings: 5 + 6 and 6 + 7 high bits (25 atoms: 0.5 GiB, 64-bit offsets)
    add("split", 23, "complex")
    add("split", 23, "real", init="ground", pitch="tight")
    add("split", 25, "complex")
    # the non-static kernel k_split_t<SPLIT_NT>: tiles smaller than 2^12 (the split path forced below 12 atoms)
    add("split", 10, "complex", method="split", tag="forced")
    # the pass kernels at one and two tilings where the tight fixtures also apply
    for n in (13, 14):
        add("split", n, "complex", {"split_no_loop": True}, method="split", tag="no-loop")
    # CF4 + Taylor on the tiled k_apply passes: one launch at 17 and 21 atoms, 2^14 tiles + two passes at 24
    for n in (17, 21, 24):
        add("taylor", n, "complex", method="taylor")
    return cases


CASES = _table()


def all_setups():
    """{(setup, times): name of the first case that uses it}."""
    seen = {}
    for case in CASES:
        for s in case.setups:
            seen.setdefault((s, case.times), case.name)
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# figures (what tests/test_ket_cluster_ref.py asserts)
# ---------------------------------------------------------------------------------------------------------------------
FLOOR_PERMS = {8: (0, 7, 2, 5, 3, 6, 1, 4), 9: (8, 0, 4, 2, 6, 1, 5, 3, 7), 10: (9, 0, 5, 3, 7, 1, 8, 2, 6, 4),
               11: (0, 10, 4, 7, 2, 9, 5, 1, 8, 3, 6), 12: (11, 0, 6, 3, 9, 1, 7, 4, 10, 2, 8, 5)}


def floor_setups():
    """What the cluster product is compared with the full-space oracle on, 20 ns: every family and both initial states at 8
    and 9 atoms (2 x 3 patch + pair, cross + square), both pitches at 10 atoms (2 x 3 patch + rhombus), one run each at 11
    and 12 atoms."""
    out = []
    for n in (8, 9):
        lay = layout_of(n, PARTS[n], FLOOR_PERMS[n])
        for family in FAMILIES:
            for init in ("ket", "ground"):
                out.append(Setup(n, lay, family, init, seed=n))
    lay = layout_of(10, PARTS[10], FLOOR_PERMS[10])
    out += [Setup(10, lay, "complex", "ket", "blockade", seed=10), Setup(10, lay, "real", "ket", "tight", seed=10),
            Setup(10, lay, "complex", "ground", "tight", seed=10)]
    out.append(Setup(11, layout_of(11, PARTS[11], FLOOR_PERMS[11]), "real", "ket", seed=11))
    out.append(Setup(12, layout_of(12, PARTS[12], FLOOR_PERMS[12]), "complex", "ket", seed=12))
    return out


def floor_error(setup, times=None):
    """(max-abs, 2-norm) of cluster product - full space, the worst over ``times``."""
    times = eval_times(setup.ns) if times is None else times
    full = full_space_solution(setup, times)
    sols = cluster_solutions(setup, times)
    worst = (0.0, 0.0)
    for i in range(len(times)):
        d = product(setup.layout, [s[i] for s in sols], setup.n).numpy() - full[i]
        worst = (max(worst[0], float(np.max(np.abs(d)))), max(worst[1], float(np.linalg.norm(d))))
    return worst


def motion(setup, times):
    """(|psi(T) - psi(0)|_2, |psi(T) - psi(T) with the interaction matrix zeroed|_2), from cluster solves alone."""
    sols = cluster_solutions(setup, times)
    prob = assemble(setup)
    prob["interaction_matrix"] = np.zeros_like(prob["interaction_matrix"])
    free = solve_problem_clusters(prob, setup, (times[0], times[-1]))
    end = [s[-1] for s in sols]
    return product_distance(end, [s[0] for s in sols]), product_distance(end, [f[-1] for f in free])


def _class_of(classes, bit):
    return next(i for i, bits in enumerate(classes) if bit in bits)


def sensitivity(setup, times, plans):
    """(waveform exchange, atom move) in units of the 2-norm bar: |psi(T) - psi'(T)|_2 / NORM_BAR where psi' has the
    waveforms of two atoms of different clusters exchanged (per-atom families; None for the global drive), and where an
    atom of one cluster sits on the bit of an atom of another cluster in another bit class of every plan (the smallest
    over the plans)."""
    sols = cluster_solutions(setup, times)
    end = [s[-1] for s in sols]
    a, b = setup.layout[0][1][0], setup.layout[1][1][0]
    d_swap = None
    if setup.family != "global":
        prob = assemble(setup)
        loc = prob["samples"]["Local"]["ground-rydberg"]
        loc[a], loc[b] = loc[b], loc[a]
        edited = solve_problem_clusters(prob, setup, (times[0], times[-1]))
        d_swap = product_distance(end, [e[-1] for e in edited]) / NORM_BAR
    d_move = np.inf
    for classes in plans_of(setup.n, plans).values():
        n = setup.n
        pick = next((x, y) for x in setup.layout[0][1] for _, other in setup.layout[1:] for y in other
                    if _class_of(classes, n - 1 - x) != _class_of(classes, n - 1 - y))
        d_move = min(d_move, exchange_distance(setup, end, *pick) / NORM_BAR)
    return d_swap, float(d_move)


def _report(out=print):
    t0 = time.perf_counter()
    seen = all_setups()
    worst_sep = 0.0
    for (s, times), name in seen.items():
        cluster_solutions(s, times)
        worst_sep = max(worst_sep, separation(s))
    out(f"{len(CASES)} cases, {len(seen)} distinct (register, times): all references {time.perf_counter() - t0:.1f} s CPU; "
        f"largest separation sum {worst_sep:.2e} (bar {SEPARATION_BAR:g})")
    mv = {name: motion(s, times) for (s, times), name in seen.items()}
    a, b = min(mv, key=lambda k: mv[k][0]), min(mv, key=lambda k: mv[k][1])
    out(f"motion: smallest |psi(T) - psi(0)|_2 {mv[a][0]:.2e} ({a}); smallest effect of the interaction {mv[b][1]:.2e} ({b})")
    for (s, times), name in seen.items():
        d_swap, d_move = sensitivity(s, times, PLANS.get(s.n, ("split",)))
        out(f"sensitivity {name}: exchanged waveforms {'-' if d_swap is None else f'{d_swap:.3g}'} bars, moved atom {d_move:.3g} bars")
    t0 = time.perf_counter()
    errs = [(floor_error(s), s) for s in floor_setups()]
    wa, wn = max(errs, key=lambda e: e[0][0]), max(errs, key=lambda e: e[0][1])
    out(f"floor over {len(errs)} comparisons: max |product - full| = {wa[0][0]:.2e} (n = {wa[1].n}, {wa[1].family}, {wa[1].init}, "
        f"{wa[1].pitch}); 2-norm {wn[0][1]:.2e} (n = {wn[1].n}, {wn[1].family}, {wn[1].init}, {wn[1].pitch}); "
        f"{time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    _report()

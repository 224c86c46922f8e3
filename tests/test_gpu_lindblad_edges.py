"""The two-level master-equation kernels (``mode="mesolve"``) against exact Lindblad solutions on every plan.

Every case of the table in tests/lindblad_ref.py is run on the plan it names and compared, at every evaluation time
(t = 0 included: the uploaded product ket through ``ryd_ket_to_dm``), with the cluster-product reference: registers
made of strongly interacting clusters of 1 to 4 atoms, 1000 um apart, whose density matrix is exactly the tensor product
of tight Lindblad solutions on at most 256 entries (tests/lindblad_ref.py; tests/test_lindblad_ref.py pins it on the
full-space oracle and checks the table).  No two atoms of a register are alike (own position in an own cluster shape,
own waveforms, entangled own initial ket) and the atoms of a cluster are scattered over the atom indices, so the
interacting pairs straddle every tile and pair-pass boundary: a factor on the wrong row or column bit, a drive read from
the wrong atom or a pair pass that couples the wrong bits is an O(0.01 - 1) error.

Plans (each case asserts from ``eng.stats()`` that its plan ran):

* persistent ``k_traj_dm`` at 4, 5, 6 atoms: all six dissipator cases (``DBL`` on and off), the global real drive
  (``REALU``), |g...g> as a second initial state, a batch of 3 different registers, a batch entry with a bad atom;
* tiled multi-launch ``k_apply`` passes: 5 atoms with 2^6 tiles, 7 with 2^7 and automatic tiles, the pair passes at 8 and 9
  atoms (two and three passes), the single-launch plan at 7;
* Hermitian path (``k_apply14`` row pass + ``k_symm``) at 7 - 10 atoms;
* polynomial rows (``k_ket`` ROWS + ``k_transpose_conj``) at 10 - 14 atoms, with and without multi-knot steps, and the
  6-um pitch at 12 atoms, which must land there through ``rows_split_estimate``;
* split-operator rows (``k_split_reg<N, 5, false, ROWS>``) at 12, 13, 14 atoms;
* rows with ``k_local_exp`` (double-flip dissipators) at 10 - 14 atoms and a batch of 2 at 11;
* the multi-launch Lindbladian with pair passes at 10 and 11 atoms.

Compared: up to 9 atoms the whole rho on the host; from 10 atoms on entries gathered on the device (rows 0 and D - 1, six
seeded rows, 4096 seeded entries, the largest entries of rho(0) and all single-flip neighbours of the largest, each with
its transposed for the Hermiticity check) and, on the device, the diagonal, the trace, the occupations and rho @ V for four
unit-norm probes.  Bars: 1e-7 on every entry of rho and of rho @ V (a row of rho is propagated as a ket under a 2-norm
budget, so |d rho v|_inf is bounded by the largest row 2-norm error) and on the occupations, 2e-8 on the trace.
Measured maxima per plan: profiles/lindblad_edges.md.

What this cannot see: tests/lindblad_ref.py (module docstring) - a register in which every atom interacts with every other.
"""
import functools

import numpy as np
import pytest

import lindblad_ref as R

from pulser_amd.engine import Engine
from pulser_amd.terms import lower

pytestmark = pytest.mark.gpu

HERMITICITY = 5e-12  # the row path's figure in tests/test_gpu_ket.py (rounding: not enforced there)


@functools.lru_cache(maxsize=None)
def _reference(setup, times):
    """What is compared, per time; computed once per (register, times) and shared by the plans (read-only)."""
    out = []
    v = R.probe_vectors(setup.n) if setup.n > 9 else None
    for ref in R.references(setup, times):
        d = {"trace": ref.trace(), "occupations": ref.occupations()}
        if setup.n <= 9:
            d["full"] = ref.full()
        else:
            r, c = R.compared_entries(setup)
            d.update(entries=ref.entries(r, c), rows=ref.rows(R.compared_rows(setup.n)), diagonal=ref.diagonal(),
                     probes=ref.matmul(v))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def _device_indices(setup, device):
    import torch

    r, c = R.compared_entries(setup)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return to(r), to(c), to(R.compared_rows(setup.n)), to(R.probe_vectors(setup.n))


def _compare(eng, rho_b, occ, setup, want):
    """Errors of one density matrix (device tensor [D, D]) and its occupations against one reference time."""
    import torch

    err = {"trace": abs(float(occ[-1]) - want["trace"].real), "occupations": float(np.max(np.abs(occ[:-1] - want["occupations"])))}
    if setup.n <= 9:
        rho = rho_b.cpu().numpy()
        err["entries"] = float(np.max(np.abs(rho - want["full"])))
        err["hermiticity"] = float(np.max(np.abs(rho - rho.conj().T)))
        err["trace"] = max(err["trace"], abs(np.trace(rho) - want["trace"]))
        return err
    r, c, rows, v = _device_indices(setup, rho_b.device)
    got = rho_b[r, c].cpu().numpy()
    half = len(got) // 2
    err["entries"] = float(np.max(np.abs(got - want["entries"])))
    err["hermiticity"] = float(np.max(np.abs(got[:half] - got[half:].conj())))
    err["rows"] = float(np.max(np.abs(rho_b[rows].cpu().numpy() - want["rows"])))
    diag = torch.diagonal(rho_b)
    ref_diag = torch.from_numpy(np.ascontiguousarray(want["diagonal"])).to(rho_b.device)
    err["diagonal"] = float(torch.max(torch.abs(diag - ref_diag)).item())
    err["trace"] = max(err["trace"], abs(complex(diag.sum().item()) - want["trace"]))
    ref_pv = torch.from_numpy(np.ascontiguousarray(want["probes"])).to(rho_b.device)
    err["probes"] = float(torch.max(torch.abs(rho_b @ v - ref_pv)).item())
    return err


def _check_plan(case, s):
    """The intended plan ran: from the solve statistics, by the means of the existing tests."""
    plan, n, batch = case.plan, case.n, len(case.setups)
    dbl = case.setups[0].diss in R.DOUBLE_FLIP
    if plan == "persistent":
        assert s["n_launches"] == 1, s  # the whole solve is one launch of k_traj_dm
    elif plan in ("tiled", "pair-passes"):
        if dbl:
            assert s["passes"] == len(R.pair_pass_groups(n, batch, case.tile_bits)), s
        elif case.tile_bits:
            assert s["passes"] >= 2, s
        assert s["n_launches"] == s["passes"] * s["n_applications"] and s["n_launches"] > 50, s
    elif plan == "tiled-single-launch":
        assert s["passes"] == 1 and s["n_launches"] == s["n_applications"] and s["n_launches"] > 50, s
    elif plan == "hermitian":
        assert s["n_launches"] == 2 * s["n_applications"] and s["n_launches"] > 50, s  # row pass + symmetrisation
    elif plan in ("rows-ket", "rows-ket-by-estimate"):
        # a conjugation = 2 row passes + 1 transposition; nothing measured or booked by the split-operator sub-steps (which
        # book at least their a-priori rate: rows-split below)
        assert s["reserved"][0] == 0.0 and s["reserved"][1] == 0.0, s
        assert s["n_launches"] % 3 == 0 and s["n_launches"] < 12 * s["n_steps"], s
    elif plan == "rows-split":
        assert s["last_order"] in (6, 10) and s["reserved"][3] == 0 and 0 < s["reserved"][0] <= 8e-8, s
        assert s["n_launches"] % 3 == 0, s
    elif plan == "rows-local-exp":
        assert s["passes"] == len(R.pair_pass_groups(n, batch)), s
        assert s["n_launches"] < 12 * s["n_steps"], s  # not one launch set per application
    else:
        raise AssertionError(plan)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.CASES])
def test_density_matrices_match_the_cluster_product(case):
    times = case.times
    refs = [_reference(s, times) for s in case.setups]
    kets = np.stack([R.product_ket(s) for s in case.setups])
    worst = {}

    def book(err):
        for k, e in err.items():
            worst[k] = max(worst.get(k, 0.0), e)

    with Engine(lower([R.assemble(s) for s in case.setups]), mode="mesolve", tile_bits=case.tile_bits) as eng:
        path = dict(case.path)
        if path:
            eng.set_path(path.pop("force_generic"), **path)
        state = eng.new_state(kets)
        occ = eng.occupations(state).cpu().numpy()
        for b, s in enumerate(case.setups):
            book(_compare(eng, state[b], occ[b], s, refs[b][0]))
        snaps = eng.solve(state, np.asarray(times))
        stats = eng.stats()
        for i in range(1, len(times)):
            occ = eng.occupations(snaps[i - 1]).cpu().numpy()
            for b, s in enumerate(case.setups):
                book(_compare(eng, snaps[i - 1][b], occ[b], s, refs[b][i]))
    print(f"lindblad-edges {case.name}: " + ", ".join(f"{k} {e:.2e}" for k, e in sorted(worst.items()))
          + f"; n_steps {stats['n_steps']}, launches {stats['n_launches']}, applications {stats['n_applications']}, "
          f"passes {stats['passes']}, last_order {stats['last_order']}, reserved {stats['reserved']}")
    _check_plan(case, stats)
    for k in ("entries", "rows", "diagonal", "probes", "occupations"):
        assert worst.get(k, 0.0) < R.BAR, (k, worst)
    assert worst["trace"] < R.TRACE_BAR, worst
    assert worst["hermiticity"] < HERMITICITY, worst
    if len(case.setups) > 1:  # the batch entries really differ
        assert np.max(np.abs(refs[0][-1]["occupations"][:3] - refs[1][-1]["occupations"][:3])) > 1e-3

#!/usr/bin/env python
"""Tight-oracle fixtures of the general path (XY mode, 3- / 4-level bases, general Lindblad).

The general path (pulser_amd/general.py -> k_general.hpp: k_gen_traj, k_gen_apply_fused, ryd_general_solve_many) was
pinned to the oracle on 3-atom cases only; its other GPU tests compare one HIP path with another.  Every case here sits on
an edge of those kernels - digit decode for d = 3 / 4, the 4096-entry limit of the one-launch kernels, whether the vector
fits in LDS, column-side Liouvillian terms, SLM switching terms - and is integrated with the TIGHT oracle
(oracle/qutip_path.py: zvode Adams, rtol 1e-13, atol 1e-15; oracle/fast_lindblad.py for the 2-level master equation).

Problems are built here with NumPy and pulser_amd.problem only.  A fixture stores the oracle states at the evaluation
times (one of them between two knots), the number of right-hand sides, and a SHA-256 of the case's inputs, so that a
drift of this generator is caught (tests/test_gpu_general_oracle.py rebuilds every problem from `build`).

    python tests/golden/make_general_fixtures.py [case ...]      (default: every case; prints the cost of each)

Output: tests/golden/general_oracle_<case>.npz, written with fixed zip timestamps (regeneration is bit for bit)."""
from __future__ import annotations

import hashlib
import io
import os
import sys
import time
import zipfile

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pulser_amd import problem as P  # noqa: E402

C3_XY = 3700.0  # rad um^3 / us (the XY devices' interaction_coeff_xy)
MAG = np.array([0.0, 0.0, 30.0])


# ---------------------------------------------------------------------------
# Problem builders (the bundle of pulser_amd.problem: what the emulator hands to the solvers)
# ---------------------------------------------------------------------------


def _drive(T, rng, amp_max, det_span, phase0=0.0, jump=None):
    """Amplitude up-ramp / plateau / down-ramp, a detuning ramp, a phase with a jump at sample `jump`."""
    amp = amp_max * np.minimum(1.0, np.minimum(np.arange(T) / (0.3 * T), (T - 1 - np.arange(T)) / (0.2 * T)))
    amp = np.clip(amp, 0.0, None) * (1.0 + 0.15 * np.sin(np.arange(T) * 2 * np.pi / T * rng.uniform(1, 3)))
    det = np.linspace(-det_span, det_span, T) + rng.uniform(-1, 1)
    phase = np.full(T, float(phase0))
    if jump is not None:
        phase[jump:] += rng.uniform(0.5, 2.5)
    return {"amp": amp, "det": det, "phase": phase}


def _base(coords, eigenbasis, basis_name, T, interaction_type="ising"):
    n = len(coords)
    return {
        "n_qudits": n, "qubit_ids": tuple(f"q{i}" for i in range(n)), "coords": np.asarray(coords, float),
        "eigenbasis": list(eigenbasis), "basis_name": basis_name, "interaction_type": interaction_type,
        "duration": int(T), "sampling_rate": 1.0, "samples": {"Global": {}, "Local": {}},
        "bad_atoms": np.zeros(n, dtype=bool), "collapse_ops": [], "depolarizing_pauli_2ds": {},
        "slm_end": 0, "slm_targets": (), "reps": 1,
    }


def xy_problem(coords, T, seed, slm_end=0, slm_targets=(), dephasing=0.0):
    """XY mode: C3 (1 - 3 cos^2 theta) / r^3 exchange with theta to a magnetic field along z (tilted register: the
    in-plane field of hamiltonian_data.py would do as well), C6 / r^6 on the u-u diagonal, global microwave drive."""
    rng = np.random.default_rng(seed)
    coords = np.asarray(coords, float)
    n = len(coords)
    pos = np.column_stack((coords, 0.35 * coords[:, 0]))  # out of plane: the angles to the field differ per pair
    imat = np.zeros((2, n, n))
    for i in range(n):
        for j in range(i + 1, n):
            diff = pos[i] - pos[j]
            r = np.linalg.norm(diff)
            cos = diff @ MAG / (r * np.linalg.norm(MAG))
            imat[0, i, j] = imat[0, j, i] = C3_XY * (1 - 3 * cos**2) / r**3
            imat[1, i, j] = imat[1, j, i] = P.C6_LEVEL70 / np.linalg.norm(coords[i] - coords[j]) ** 6
    prob = _base(coords, ["u", "d"], "XY", T, "XY")
    prob["interaction_matrix"] = imat
    prob["samples"]["Global"]["XY"] = _drive(T, rng, 18.0, 12.0, phase0=rng.uniform(0, 1), jump=T // 2)
    prob["samples"]["Local"]["XY"] = {}
    prob["slm_end"] = int(slm_end)
    prob["slm_targets"] = tuple(slm_targets)
    if dephasing:
        prob["collapse_ops"] = [(np.sqrt(2 * dephasing), "sigma_dd")]
    return prob


def multilevel_problem(coords, T, seed, leakage=False, local=(), collapse=()):
    """3-level "all" basis (r, g, h) - or 4-level with the leakage state x - global ground-rydberg drive with a phase jump,
    local raman (digital) drives with complex phases on the atoms of `local`."""
    rng = np.random.default_rng(seed)
    eig = ["r", "g", "h", "x"] if leakage else ["r", "g", "h"]
    prob = _base(coords, eig, "all_with_error" if leakage else "all", T)
    prob["interaction_matrix"] = P.interaction_matrix(coords, P.C6_LEVEL70)
    prob["samples"]["Global"]["ground-rydberg"] = _drive(T, rng, 14.0, 10.0, phase0=0.3, jump=T // 3)
    prob["samples"]["Local"]["digital"] = {int(q): _drive(T, rng, rng.uniform(4, 9), rng.uniform(2, 5),
                                                          phase0=rng.uniform(0, 2), jump=2 * T // 3) for q in local}
    prob["collapse_ops"] = list(collapse)
    return prob


def ising_problem(coords, T, seed, collapse=()):
    rng = np.random.default_rng(seed)
    prob = _base(coords, ["r", "g"], "ground-rydberg", T)
    prob["interaction_matrix"] = P.interaction_matrix(coords, P.C6_LEVEL70)
    prob["samples"]["Global"]["ground-rydberg"] = _drive(T, rng, 16.0, 20.0, phase0=0.7, jump=T // 2)
    prob["collapse_ops"] = list(collapse)
    return prob


def _hexagon(spacing):
    ang = np.arange(6) * np.pi / 3
    return np.vstack([[0.0, 0.0], spacing * np.column_stack((np.cos(ang), np.sin(ang)))])


EFF_NOISE = np.array([[0.3, 0.5 - 0.2j], [0.1j, -0.3]])

# name -> (builder () -> [problems], mesolve, why)
CASES = {
    "xy8_slm": (lambda: [xy_problem(P.register_coords(P.square_rect(2, 4), 5.0), 241, 1, slm_end=97,
                                    slm_targets=(0, 5))], False,
                "XY ket, 8 atoms: pair-local terms, SLM mask switching off at 97 ns (k_gen_traj, k_gen_apply_fused)"),
    "xy12": (lambda: [xy_problem(P.register_coords(P.square_rect(3, 4), 5.5), 161, 2)], False,
             "XY ket, 12 atoms = 4096 amplitudes: the one-launch size limit, vector in LDS"),
    "xy13": (lambda: [xy_problem(P.register_coords(P.triangular_rect(3, 5), 6.0)[:13], 121, 3)], False,
             "XY ket, 13 atoms = 8192 amplitudes: multi-launch, vector out of LDS"),
    "all7": (lambda: [multilevel_problem(P.register_coords(P.triangular_rect(2, 4), 6.5)[:7], 161, 4,
                                         local=(0, 3, 6))], False,
             "3-level ket, 7 atoms = 2187: d = 3 digit decode, vector in LDS"),
    "all9": (lambda: [multilevel_problem(P.register_coords(P.square_rect(3, 3), 6.5), 101, 5, local=(1, 4, 8))], False,
             "3-level ket, 9 atoms = 19683: d = 3 digit decode, vector out of LDS"),
    "leak6": (lambda: [multilevel_problem(P.register_coords(P.square_rect(2, 3), 6.0), 161, 6, leakage=True,
                                          local=(2, 5))], False,
              "4-level (leakage) ket, 6 atoms = 4096: d = 4 decode at the one-launch edge"),
    "xy5_me": (lambda: [xy_problem(P.register_coords(P.square_rect(1, 5), 5.0), 201, 7, dephasing=0.8)], True,
               "XY mesolve, 5 atoms (rho 1024), dephasing: column-side Liouvillian terms"),
    "xy6_me": (lambda: [xy_problem(P.register_coords(P.square_rect(2, 3), 5.0), 161, 8, dephasing=0.8)], True,
               "XY mesolve, 6 atoms (rho 4096), dephasing: one-launch edge for rho"),
    "ising7_me": (lambda: [ising_problem(_hexagon(5.5), 1001, 9,
                                         collapse=[(np.sqrt(2 * 0.6), "sigma_rr"), (np.sqrt(0.8), EFF_NOISE)])], True,
                  "Ising mesolve, 7 atoms at 5.5 um (rho 16384), dephasing + non-diagonal eff_noise, 1 us: static "
                  "diagonal + dissipator, CF4 steps"),
    "all4_me": (lambda: [multilevel_problem(P.register_coords(P.square_rect(2, 2), 6.0), 161, 10, local=(1,),
                                            collapse=[(np.sqrt(0.5), "sigma_gr"), (np.sqrt(2 * 0.7), "sigma_rr"),
                                                      (np.sqrt(2 * 0.3), "sigma_hh")])], True,
                "3-level mesolve, 4 atoms (rho 6561), relaxation + dephasing: d = 3 superoperator on the digit pairs"),
    "xy6_batch": (lambda: [xy_problem(P.register_coords(P.square_rect(2, 3), s), 121, 20 + k, dephasing=0.5)
                           for k, s in enumerate((4.5, 5.0, 6.0))], True,
                  "three XY mesolve 6-atom registers (rho 4096) of different pitch and drive: ryd_general_solve_many"),
}


def build(name):
    """(problems, mesolve, initial ket, evaluation times in us) of case `name`."""
    make, mesolve, _ = CASES[name]
    probs = make()
    n, d = probs[0]["n_qudits"], len(probs[0]["eigenbasis"])
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    psi = rng.normal(size=d**n) + 1j * rng.normal(size=d**n)
    if d == 4:  # nothing starts in the leakage state
        psi[((np.arange(d**n)[:, None] // d ** np.arange(n)) % d == 3).any(axis=1)] = 0.0
    psi /= np.linalg.norm(psi)
    t_end = (probs[0]["duration"] - 1) * 1e-3
    times = np.array([0.0, round(0.37 * t_end, 3) + 0.0004, round(0.71 * t_end, 3), t_end])  # 2nd: between knots
    return probs, mesolve, psi, times


def digest(prob) -> str:
    m = hashlib.sha256()

    def feed(obj):
        if isinstance(obj, dict):
            for k in sorted(obj, key=str):
                m.update(repr(k).encode())
                feed(obj[k])
        elif isinstance(obj, (list, tuple)):
            m.update(b"[")
            for v in obj:
                feed(v)
            m.update(b"]")
        elif isinstance(obj, np.ndarray) or isinstance(obj, (float, complex)):
            # to 10 significant digits: np.sin & co. may differ in the last bit between CPUs (SIMD paths)
            a = np.asarray(obj)
            m.update(str(a.dtype).encode() + repr(a.shape).encode())
            parts = (a.real, a.imag) if np.iscomplexobj(a) else (a,)
            for part in parts:
                m.update(" ".join(f"{v + 0.0:.9e}" for v in np.ravel(part).astype(float)).encode())
        else:
            m.update(repr(obj).encode())

    feed(prob)
    return m.hexdigest()


def digest_case(name) -> str:
    probs, mesolve, psi, times = build(name)
    m = hashlib.sha256()
    for p in probs:
        m.update(digest(p).encode())
    m.update(" ".join(f"{v + 0.0:.9e}" for v in np.concatenate([psi.real, psi.imag, times])).encode() + bytes([mesolve]))
    return m.hexdigest()


# ---------------------------------------------------------------------------
# Oracle
# ---------------------------------------------------------------------------


def oracle_states(prob, mesolve, psi, times):
    from oracle import qutip_path as qp

    chans = [(s["amp"], s["det"]) for addr in prob["samples"] for basis, s in prob["samples"][addr].items()
             if s and addr == "Global"]
    chans += [(s["amp"], s["det"]) for basis, loc in prob["samples"]["Local"].items() for s in loc.values()]
    opts = qp.default_options(chans, prob["duration"])
    opts.update(qp.TIGHT)
    ham = qp.build_hamiltonian(prob)
    counter = [0]
    if not mesolve:
        out = qp.sesolve(ham, psi, times, counter=counter, **opts)
    elif len(prob["eigenbasis"]) == 2 and prob["interaction_type"] == "ising":
        from oracle import fast_lindblad

        fl = fast_lindblad.FastLindblad(ham)
        assert fl.check() < 1e-9, fl.check()
        out = qp._zvode(fl, np.outer(psi, psi.conj()).ravel(), times, opts, counter)
    else:
        out = [r.ravel() for r in qp.mesolve(ham, psi, times, counter=counter, **opts)]
    return np.stack([np.asarray(o).ravel() for o in out[1:]]), counter[0]


def _save(path, **arrays):
    """np.savez_compressed with fixed zip timestamps, so that a regeneration is bit for bit."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def make(name):
    probs, mesolve, psi, times = build(name)
    tic = time.time()
    states, rhs = [], []
    for p in probs:
        s, r = oracle_states(p, mesolve, psi, times)
        states.append(s)
        rhs.append(r)
    secs = time.time() - tic
    path = os.path.join(HERE, f"general_oracle_{name}.npz")
    _save(path, states=np.stack(states), times=times, mesolve=np.array(mesolve), rhs_evals=np.array(rhs),
          input_sha256=np.array(digest_case(name)), description=np.array(CASES[name][2]),
          oracle=np.array("zvode Adams rtol 1e-13 atol 1e-15 (oracle.qutip_path.TIGHT), random initial ket"))
    tr = ""
    if mesolve:
        D = int(round(np.sqrt(states[0].shape[1])))
        tr = f"; |tr rho - 1| {max(abs(np.trace(s[-1].reshape(D, D)) - 1) for s in states):.1e}"
    else:
        tr = f"; norm drift {max(abs(np.linalg.norm(s[-1]) - 1) for s in states):.1e}"
    print(f"{name}: dim {states[0].shape[1]}, {sum(rhs)} RHS in {secs:.1f} s{tr}; "
          f"{os.path.getsize(path) / 2**20:.2f} MiB", flush=True)


def main():
    names = sys.argv[1:] or list(CASES)
    for name in names:
        make(name)


if __name__ == "__main__":
    main()

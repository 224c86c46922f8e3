"""Many sequences in one solve: ``solve_many`` and the public ``run_batch``.

The library's throughput comes from batching - one workgroup per sequence, one sequence per CU - while ``run()``
solves one sequence on one CU.  ``run_batch`` takes a list of emulators (a Rabi or duration scan, a calibration grid,
the inner loop of a pulse optimisation) and solves every noiseless two-level Ising sequence among them in as few
launch sequences as possible, entries of different durations included:

* ``terms.lower_ragged`` puts entries of different durations into ONE table set (each entry keeps its own pieces);
* the evaluation times of all entries form one union grid; a snapshot map (``ryd_set_snapshot_map``) sends every
  entry's state at ITS times to its own rows of one compact output and stores nothing else;
* ``run_batch`` wraps each entry's rows as the ``CoherentResults`` its own ``run()`` returns.

DESIGN.md section 5.14.
"""

from __future__ import annotations

import time
from collections import Counter
from dataclasses import dataclass, field
from typing import Any, Mapping, Sequence

import numpy as np

from .terms import lower_ragged, sampling_times

# engine keywords solve_many passes on (Engine.solve)
_SOLVE_KEYS = ("tol", "taylor_order", "max_order", "magnus_tol", "max_step", "split_steps", "method")


def union_grid(eval_times: Sequence[Sequence[float]]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The common time grid of entries that ask for different evaluation times, and where each entry's states go.

    Every ``eval_times[b]`` is non-decreasing and starts at the same initial time.  Returns ``(grid, offsets, base)``:
    ``grid`` holds the initial time and then every later time of every entry, a time that an entry lists k times
    appearing max_b k times; ``offsets`` int64[batch, len(grid) - 1] sends the j-th occurrence of a time in entry b to
    ket ``base[b] + (its index in eval_times[b]) - 1`` and every other slot to -1; the output is entry-major and compact:
    entry b owns kets ``base[b] .. base[b] + len(eval_times[b]) - 2``."""
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in eval_times]
    if not ts:
        raise ValueError("at least one entry is required")
    t0 = ts[0][0] if len(ts[0]) else None
    for b, t in enumerate(ts):
        if len(t) < 2:
            raise ValueError(f"entry {b}: at least two evaluation times are required")
        if t[0] != t0:
            raise ValueError(f"entry {b} starts at {t[0]}, entry 0 at {t0}: every entry starts at the same time")
        if np.any(np.diff(t) < 0):
            raise ValueError(f"entry {b}: evaluation times must be non-decreasing")
    mult: Counter = Counter()
    for t in ts:
        for v, k in Counter(t[1:].tolist()).items():
            mult[v] = max(mult[v], k)
    rest = sorted(mult)
    first_slot: dict[float, int] = {}
    grid = [float(t0)]
    for v in rest:
        first_slot[v] = len(grid) - 1
        grid.extend([v] * mult[v])
    base = np.zeros(len(ts), dtype=np.int64)
    base[1:] = np.cumsum([len(t) - 1 for t in ts])[:-1]
    offsets = np.full((len(ts), len(grid) - 1), -1, dtype=np.int64)
    for b, t in enumerate(ts):
        seen: Counter = Counter()
        for i, v in enumerate(t[1:].tolist()):
            offsets[b, first_slot[v] + seen[v]] = base[b] + i
            seen[v] += 1
    return np.asarray(grid, dtype=np.float64), offsets, base


def ragged_groups(problems: Sequence[Mapping[str, Any]]) -> list[list[int]]:
    """Indices of ``problems`` that can share one table set (``lower_ragged``): the same register size, sampling rate
    and basis, and knot times that are a prefix of the group's longest entry's.  Longest first within a key; list order
    otherwise."""
    keyed: dict[tuple, list[int]] = {}
    for i, p in enumerate(problems):
        keyed.setdefault((int(p["n_qudits"]), float(p.get("sampling_rate", 1.0)), p["basis_name"]), []).append(i)
    groups: list[list[int]] = []
    for (_, rate, _), idx in keyed.items():
        mine: list[tuple[np.ndarray, list[int]]] = []
        for i in sorted(idx, key=lambda i: -int(problems[i]["duration"])):
            tk = sampling_times(int(problems[i]["duration"]), rate)
            for gk, g in mine:
                if len(tk) <= len(gk) and np.array_equal(tk, gk[: len(tk)]):
                    g.append(i)
                    break
            else:
                mine.append((tk, [i]))
        groups.extend(sorted(g) for _, g in mine)
    return groups


@dataclass
class ManySolve:
    """What :func:`solve_many` returns.  ``states[b]``: complex128[len(eval_times[b]) - 1, 2^N] on the device, the
    states at ``eval_times[b][1:]``; ``stats[b]``: the engine statistics of the solve that held entry b;
    ``chunks``: the entries of every solve; ``lower_s`` / ``solve_s``: host seconds spent lowering / solving (the
    solve waits for the device)."""

    states: list[Any]
    stats: list[dict[str, Any]]
    chunks: list[list[int]] = field(default_factory=list)
    lower_s: float = 0.0
    solve_s: float = 0.0


def _chunks(idx: list[int], n_slots: Sequence[int], dim: int) -> list[list[int]]:
    """Cut a group so that the stored states and the solver's work copies of each solve fit the device."""
    import torch

    free, _ = torch.cuda.mem_get_info()
    cap = 0.45 * free / (16.0 * dim)  # kets
    out: list[list[int]] = []
    cur: list[int] = []
    kets = 0
    for i in idx:
        need = n_slots[i] + 5
        if cur and kets + need > cap:
            out.append(cur)
            cur, kets = [], 0
        cur.append(i)
        kets += need
    if cur:
        out.append(cur)
    return out


def solve_many(problems: Sequence[Mapping[str, Any]], eval_times: Sequence[Sequence[float]],
               initial_kets: Sequence[Any] | None = None, path: Mapping[str, bool] | None = None,
               **options: Any) -> ManySolve:
    """Solve noiseless two-level Ising problems of possibly different durations and registers, each at its own
    evaluation times (us, starting at 0), in as few solves as the grouping allows (:func:`ragged_groups`; one
    ``Engine`` per group, large groups cut into chunks whose snapshots fit the device).

    ``initial_kets[b]``: entry b's initial ket (2^N amplitudes) or ``None`` for ``|g...g>`` (basis vector 2^N - 1);
    ``options``: ``Engine.solve`` keywords (``tol``, ``max_step``, ``method``, ...); ``path``: ``Engine.set_path``
    test hooks.  The step-size controller's sub-steps are shared by the entries of a solve, so a state equals that of a
    solo solve within the two error estimates, not bit for bit."""
    from .engine import Engine
    from .simulation import QutipEmulator

    if len(eval_times) != len(problems):
        raise ValueError(f"need one evaluation-time array per problem ({len(problems)}), got {len(eval_times)}")
    if initial_kets is not None and len(initial_kets) != len(problems):
        raise ValueError(f"need one initial ket (or None) per problem ({len(problems)}), got {len(initial_kets)}")
    unknown = set(options) - set(_SOLVE_KEYS)
    if unknown:
        raise TypeError(f"unknown solve options {sorted(unknown)}; one of {_SOLVE_KEYS}")
    ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in eval_times]
    for b, (p, t) in enumerate(zip(problems, ts)):
        if not QutipEmulator._fast_path_ok(p) or p.get("collapse_ops"):
            raise ValueError(f"entry {b} is not a noiseless two-level Ising problem")
        if len(t) < 2 or t[0] != 0.0:
            raise ValueError(f"entry {b}: evaluation times must start at 0 and hold at least two values")
    states: list[Any] = [None] * len(problems)
    stats: list[dict[str, Any]] = [{}] * len(problems)
    res = ManySolve(states, stats)
    for group in ragged_groups(problems):
        n = int(problems[group[0]]["n_qudits"])
        dim = 1 << n
        for chunk in _chunks(group, [len(t) - 1 for t in ts], dim):
            t_lower = time.perf_counter()
            tables = lower_ragged([problems[i] for i in chunk])
            res.lower_s += time.perf_counter() - t_lower
            grid, offsets, base = union_grid([ts[i] for i in chunk])
            total = int(sum(len(ts[i]) - 1 for i in chunk))
            QutipEmulator._check_snapshot_budget(-(-total // len(chunk)), 16 * dim * len(chunk))
            kets = np.empty((len(chunk), dim), dtype=np.complex128)
            for r, i in enumerate(chunk):
                k = None if initial_kets is None else initial_kets[i]
                if k is None:
                    kets[r] = 0.0
                    kets[r, -1] = 1.0
                else:
                    k = np.asarray(k, dtype=np.complex128).reshape(-1)
                    if k.size != dim:
                        raise ValueError(f"entry {i}: the initial ket has {k.size} amplitudes, 2^{n} expected")
                    kets[r] = k
            t_solve = time.perf_counter()
            with Engine(tables, mode="sesolve") as eng:
                if path:
                    eng.set_path(**{"force_generic": False, **path})
                eng.set_snapshot_map(offsets)
                state = eng.new_state(kets)
                out = eng.solve(state, grid, store=True, **options)
                eng.torch.cuda.current_stream(eng.device).synchronize()
                st = eng.stats()
            res.solve_s += time.perf_counter() - t_solve
            st["batch"] = len(chunk)
            for r, i in enumerate(chunk):
                states[i] = out[int(base[r]): int(base[r]) + len(ts[i]) - 1]
                stats[i] = st
            res.chunks.append(list(chunk))
    return res


def _batchable(emu: Any, options: Mapping[str, Any]) -> bool:
    """Would ``emu.run(**options)`` send its one sequence through ``_solve_batch`` on the tuned ket kernels?"""
    from .noise_model import has_stochastic_noise

    prob = emu._current_problem
    if has_stochastic_noise(emu.noise_model) or emu._solver_mode(prob) != "sesolve":
        return False
    if not emu._fast_path_ok(prob) or prob.get("collapse_ops"):
        return False
    init = np.asarray(emu._initial_state)
    return init.size == 2 ** int(emu._hamiltonian_data.n_qudits)  # a ket (a density matrix goes through run())


def run_batch(emulators: Sequence[Any], progress_bar: bool = False, **options: Any) -> list[Any]:
    """``[emu.run(**options) for emu in emulators]``, with the noiseless two-level Ising sequences among them solved
    together: grouped by register size, sampling rate and knot grid (durations may differ), one solve per group
    (a group too large for the device's memory in several), every CU busy with a sequence of its own.

    Every other emulator - noisy, XY, multi-level, master equation, the general path - runs its own ``run(**options)``,
    in list order.  Each result is what that emulator's ``run()`` returns: a ``CoherentResults`` with its own evaluation
    times and initial state, states kept on the device until read, evaluation times normalised by its own duration;
    ``last_engine_stats`` is set on every emulator (for a batched one: the statistics of the solve that held it, with
    ``batch`` = its size).  Evaluation-time windows are not used: the batch fills the CUs itself.

    Accuracy: the step-size controller's sub-steps are shared by the sequences of a solve, so a state equals its solo
    ``run()`` within the two runs' error estimates (about 1e-7), not bit for bit."""
    if progress_bar not in (True, False, None):
        raise ValueError("`progress_bar` must be a bool.")
    from .results import CoherentResults, LazyState, QState, SnapshotStore, StateResult

    emulators = list(emulators)
    out: list[Any] = [None] * len(emulators)
    groups: dict[tuple, list[int]] = {}
    for i, emu in enumerate(emulators):
        own = dict(options)  # (validation fills in each emulator's own defaults, max_step among them)
        emu._validate_options(own)
        if _batchable(emu, own):
            kw = emu._engine_kwargs(own)
            groups.setdefault(tuple(sorted(kw.items())), []).append(i)
    batched = {i for idx in groups.values() for i in idx}
    for kw_items, idx in groups.items():
        probs = [emulators[i]._current_problem for i in idx]
        times = [np.asarray(emulators[i]._eval_times_array, dtype=np.float64) for i in idx]
        kets = [np.asarray(emulators[i]._initial_state).reshape(-1) for i in idx]
        solved = solve_many(probs, times, kets, **dict(kw_items))
        for r, i in enumerate(idx):
            emu = emulators[i]
            emu.last_engine_stats = solved.stats[r]
            n = int(emu._hamiltonian_data.n_qudits)
            store = SnapshotStore(solved.states[r].reshape(len(times[r]) - 1, 1, 2**n))
            meas_errors = (
                {"epsilon": emu.noise_model.p_false_pos, "epsilon_prime": emu.noise_model.p_false_neg}
                if "SPAM" in emu.noise_model.noise_types else None
            )
            qids = tuple(emu.samples_obj.qubit_ids)
            matching = emu._meas_basis in emu.basis_name
            t_unit = emu._tot_duration * 1e-3
            results = []
            for k, t in enumerate(times[r]):
                st = QState(np.asarray(kets[r], dtype=np.complex128)) if k == 0 else LazyState(store, k - 1, 0, (2**n, 1))
                results.append(StateResult(qids, emu._meas_basis, st, matching, evaluation_time=float(t / t_unit)))
            out[i] = CoherentResults(results, n, emu.basis_name, times[r], emu._meas_basis, meas_errors)
    for i, emu in enumerate(emulators):
        if i not in batched:
            out[i] = emu.run(progress_bar=progress_bar, **options)
    return out

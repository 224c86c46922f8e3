"""CPU: the host side of many-sequence solves (pulser_amd.batch, terms.lower_ragged): ragged tables, grouping, the union
time grid and its offset table, and the new C ABI symbol."""
from __future__ import annotations

import ctypes
import dataclasses
import os

import numpy as np
import pytest

from helpers import fuzz_case

from pulser_amd import problem as P
from pulser_amd.batch import _batchable, ragged_groups, union_grid
from pulser_amd.terms import lower, lower_ragged, sampling_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuzz_entries():
    out = []
    for seed in range(12):
        probs, _ = fuzz_case(seed, n_atoms=8 + seed % 5 if seed % 5 < 4 else 10)
        out.append(probs[0])
    return out


def test_ragged_tables_keep_every_entry_and_extrapolate_its_last_cubic():
    entries = _fuzz_entries()
    for n in sorted({int(p["n_qudits"]) for p in entries}):
        probs = [p for p in entries if int(p["n_qudits"]) == n]
        T = lower_ragged(probs)
        durations = [int(p["duration"]) for p in probs]
        assert np.array_equal(T.tknots, sampling_times(max(durations), 1.0))
        assert np.array_equal(T.t_end, np.asarray(durations) / 1000.0)
        for b, p in enumerate(probs):
            solo = lower([p])
            m = solo.pp.shape[1]
            assert T.interaction[b if T.interaction.shape[0] > 1 else 0].tolist() == solo.interaction[0].tolist()
            for f in ("drive_series", "det_series"):
                for k in range(n):
                    sid, rid = int(solo.desc[0][f][k]), int(T.desc[b][f][k])
                    assert (sid < 0) == (rid < 0)
                    if sid < 0:
                        continue
                    assert T.desc[b][f.replace("series", "scale")][k] == solo.desc[0][f.replace("series", "scale")][k]
                    # the entry's own pieces, bit for bit
                    assert np.array_equal(T.pp[rid, :m], solo.pp[sid])
                    if m == T.pp.shape[1]:
                        continue
                    # [t_{d-1}, t_end]: the extrapolated last cubic, re-based to knot d - 1
                    x = np.linspace(T.tknots[m], T.t_end[b], 9)
                    want = np.polyval(solo.pp[sid, m - 1], x - T.tknots[m - 1])
                    got = np.polyval(T.pp[rid, m], x - T.tknots[m])
                    assert np.max(np.abs(got - want)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300)
                    assert not np.any(T.pp[rid, m + 1:])


def test_ragged_tables_refuse_mixed_batches_and_non_prefix_grids():
    probs, _ = fuzz_case(3, n_atoms=9)
    other, _ = fuzz_case(4, n_atoms=10)
    with pytest.raises(ValueError, match="share N"):
        lower_ragged([probs[0], other[0]])
    a = dict(probs[0], sampling_rate=0.5, duration=300)
    b = dict(probs[0], sampling_rate=0.5, duration=301)
    if not np.array_equal(sampling_times(300, 0.5), sampling_times(301, 0.5)[:150]):
        with pytest.raises(ValueError, match="prefix"):
            lower_ragged([a, b])
    # the example of the issue: at other rates adapt_to_sampling_rate breaks the prefix property
    bad = [(d1, d2) for d1 in range(200, 240) for d2 in range(d1 + 1, 260)
           if not np.array_equal(sampling_times(d1, 0.3), sampling_times(d2, 0.3)[: len(sampling_times(d1, 0.3))])]
    assert bad
    d1, d2 = bad[0]
    s = probs[0]["samples"]
    with pytest.raises(ValueError, match="prefix"):
        lower_ragged([dict(probs[0], sampling_rate=0.3, duration=d1), dict(probs[0], sampling_rate=0.3, duration=d2)])
    assert s is probs[0]["samples"]
    with pytest.raises(NotImplementedError, match="noiseless"):
        lower_ragged([dict(probs[0], collapse_ops=[(1.0, "sigma_rr")])])


def test_ragged_groups():
    a, _ = fuzz_case(1, n_atoms=9)
    b, _ = fuzz_case(2, n_atoms=9)
    c, _ = fuzz_case(5, n_atoms=10)
    d1, d2 = next((x, y) for x in range(200, 240) for y in range(x + 1, 260)
                  if not np.array_equal(sampling_times(x, 0.3), sampling_times(y, 0.3)[: len(sampling_times(x, 0.3))]))
    probs = [a[0], c[0], b[0], dict(a[0], sampling_rate=0.3, duration=d1), dict(a[0], sampling_rate=0.3, duration=d2),
             dict(b[0], duration=150), dict(b[0], sampling_rate=0.5, duration=200)]
    groups = ragged_groups(probs)
    # at sampling rate 1 every knot grid is a prefix of a longer one; other rates, registers sizes: apart
    assert sorted(map(sorted, groups)) == [[0, 2, 5], [1], [3], [4], [6]]


def test_union_grid_offsets_unmapped_slots_and_duplicate_times():
    grid, off, base = union_grid([[0.0, 0.1, 0.3], [0.0, 0.2, 0.2, 0.3, 0.5], [0.0, 0.5]])
    assert grid.tolist() == [0.0, 0.1, 0.2, 0.2, 0.3, 0.5]
    assert base.tolist() == [0, 2, 6]
    assert off.tolist() == [[0, -1, -1, 1, -1],
                            [-1, 2, 3, 4, 5],
                            [-1, -1, -1, -1, 6]]
    # compact and entry-major: every ket of the output is owned exactly once
    assert sorted(off[off >= 0].tolist()) == list(range(7))
    # an entry that repeats a time more often than any other sets its multiplicity
    grid, off, _ = union_grid([[0.0, 0.4, 0.4, 0.4], [0.0, 0.4]])
    assert grid.tolist() == [0.0, 0.4, 0.4, 0.4] and off.tolist() == [[0, 1, 2], [3, -1, -1]]
    with pytest.raises(ValueError, match="same time"):
        union_grid([[0.0, 1.0], [0.1, 1.0]])
    with pytest.raises(ValueError, match="non-decreasing"):
        union_grid([[0.0, 1.0, 0.5]])


def test_grouping_decisions_for_mixed_lists():
    """What run_batch batches and what runs on its own: noise (master equation, trajectories) and XY."""
    import warnings

    from pulser_amd import NoiseModel, QutipEmulator
    from pulser_amd.hamiltonian_data import single_global_channel

    def emu(n=4, dur=200, xy=False, **kw):
        coords = P.register_coords(P.square_rect(1, n), 7.0)
        t = np.arange(dur) / dur
        s = {"amp": 5.0 * np.sin(np.pi * t) ** 2, "det": -5.0 + 10.0 * t, "phase": np.zeros(dur)}
        inputs = single_global_channel(coords, s, 3700.0 if xy else P.C6_LEVEL70,
                                       basis="XY" if xy else "ground-rydberg", extended=False)
        if xy:  # (C3 = 3700, field along z)
            inputs = dataclasses.replace(inputs, interaction_coeff_xy=3700.0, magnetic_field=(0.0, 0.0, 30.0))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            return QutipEmulator(inputs, **kw)

    plain = emu()
    assert _batchable(plain, {})
    assert _batchable(emu(n=5, dur=333, sampling_rate=0.5), {})
    assert not _batchable(emu(xy=True), {})
    assert not _batchable(emu(noise_model=NoiseModel(dephasing_rate=0.1)), {})
    assert not _batchable(emu(noise_model=NoiseModel(samples_per_run=1, temperature=20000), n_trajectories=3), {})
    own = emu()
    own.set_initial_state(np.full(16, 0.25, dtype=complex))
    assert _batchable(own, {})


def test_the_snapshot_map_symbol_resolves():
    with open(os.path.join(ROOT, "include", "rydemu.h")) as f:
        assert "int ryd_set_snapshot_map(ryd_handle* h, int32_t n_slots, const int64_t* offsets);" in f.read()
    from pulser_amd import _lib

    assert "ryd_set_snapshot_map" in _lib.SYMBOLS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ryd_set_snapshot_map")
    fn = lib.ryd_set_snapshot_map
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert fn(None, 0, None) == -1  # RYD_ERR_INVALID: a null handle is refused without touching a device

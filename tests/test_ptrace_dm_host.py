"""CPU: the host side of the partial trace of density matrices - the ``ryd_reduced_density_dm`` declaration, binding and
export, its argument checks (decided before the device is touched), and what ``engine.reduced_density_dm`` refuses
before it needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pulser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = ["const void* states_dev", "int32_t n_times", "int32_t n_batch", "int64_t stride_t", "int64_t stride_b",
             "int64_t dim", "int32_t local_dim", "int32_t n_sites", "const int32_t* keep", "int32_t n_keep",
             "void* out_dev", "int32_t n_split", "void* scratch_dev", "int64_t scratch_bytes", "int32_t device",
             "void* stream"]


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rydemu.h")).read()
    m = re.search(r"int ryd_reduced_density_dm\(([^;]*)\);", header)
    assert m, "ryd_reduced_density_dm is not declared in include/rydemu.h"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split(",")]
    assert args == PROTOTYPE, args
    restype, argtypes = _lib.SYMBOLS["ryd_reduced_density_dm"]
    want = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    assert restype is C.c_int and list(argtypes) == want
    assert list(argtypes) == list(_lib.SYMBOLS["ryd_reduced_density"][1])  # the ket call's, argument for argument
    # (loading the library needs no device)
    assert hasattr(_lib.load(), "ryd_reduced_density_dm")
    assert _lib.RYD_ABI_VERSION == 1 and re.search(r"#define\s+RYD_ABI_VERSION\s+1\b", header)
    assert "Replaces: Qobj.ptrace" in header[:header.index("int ryd_reduced_density_dm(")].rsplit("/*", 1)[1]


def test_abi_rejects_bad_arguments_without_a_device():
    """Every RYD_ERR_INVALID case is decided before the device is touched (test_gpu_reduced_density_dm repeats them with
    live pointers).  Arguments: states, n_times, n_batch, stride_t, stride_b, dim, local_dim, n_sites, keep, n_keep, out,
    n_split, scratch, scratch_bytes.  The strides are those of matrices: dim * dim = 64 for three qubits."""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data

    def keep(*sites):
        a = np.array(sites, dtype=np.int32)
        return a, a.ctypes.data, len(sites)

    k1, pk1, _ = keep(1)
    good = (p, 1, 1, 64, 64, 8, 2, 3, pk1, 1, p, 1, None, 0)
    bad = {
        "states null": (None,) + good[1:],
        "out null": good[:10] + (None,) + good[11:],
        "keep null": good[:8] + (None,) + good[9:],
        "n_times < 0": (p, -1) + good[2:],
        "n_batch = 0": (p, 1, 0) + good[3:],
        "n_batch < 0": (p, 1, -2) + good[3:],
        "dim != d^n": good[:5] + (9,) + good[6:],
        "dim != d^n (n)": good[:7] + (4,) + good[8:],
        "local_dim 1": good[:6] + (1,) + good[7:],
        "local_dim 5": good[:6] + (5,) + good[7:],
        "stride_t < dim^2": (p, 2, 1, 63) + good[4:],
        "stride_b < dim^2": (p, 1, 2, 64, 63) + good[5:],
        "stride_t = dim": (p, 2, 1, 8) + good[4:],  # a ket's stride is no matrix's
        "stride_b = dim": (p, 1, 2, 64, 8) + good[5:],
        "n_keep = 0": good[:9] + (0,) + good[10:],
        "n_keep < 0": good[:9] + (-1,) + good[10:],
        "n_split < 0": good[:11] + (-1,) + good[12:],
        "split without scratch": good[:11] + (2, None, 0),
        "scratch too small": good[:11] + (2, p, 2 * 4 * 16 - 1),
        "null states, no times": (None, 0) + good[2:],
    }
    for sites in ((3,), (-1,), (1, 1), (2, 1), (0, 1, 2, 3)):  # out of range, repeated, descending, more than n_sites
        arr, ptr, cnt = keep(*sites)
        bad[f"keep {sites}"] = good[:8] + (ptr, cnt) + good[10:]
        bad[f"keep {sites}"] += (arr,)  # (keeps the array alive; cut off below)
    for name, args in bad.items():
        assert lib.ryd_reduced_density_dm(*args[:14], 0, None) == -1, name  # RYD_ERR_INVALID
        assert "reduced_density_dm" in lib.ryd_last_error().decode(), name
    # dA > 64: seven of eight qubits, four of five qutrits, four four-level atoms
    for d, n, cnt in ((2, 8, 7), (3, 5, 4), (4, 4, 4)):
        arr, ptr, _ = keep(*range(cnt))
        dim = d**n
        assert lib.ryd_reduced_density_dm(p, 1, 1, dim * dim, dim * dim, dim, d, n, ptr, cnt, p, 1, None, 0, 0, None) == -1
        assert "64" in lib.ryd_last_error().decode()
    # n_times = 0: nothing to do, nothing launched - with or without a split
    assert lib.ryd_reduced_density_dm(p, 0, 1, 64, 64, 8, 2, 3, pk1, 1, p, 1, None, 0, 0, None) == 0
    assert lib.ryd_reduced_density_dm(p, 0, 1, 64, 64, 8, 2, 3, pk1, 1, p, 0, None, 0, 0, None) == 0
    assert lib.ryd_reduced_density_dm(p, 0, 1, 64, 64, 8, 2, 3, pk1, 1, p, 3, p, 0, 0, None) == 0
    # keeping every site is valid
    arr, ptr, cnt = keep(0, 1, 2)
    assert lib.ryd_reduced_density_dm(p, 0, 1, 64, 64, 8, 2, 3, ptr, cnt, p, 1, None, 0, 0, None) == 0


def test_density_snapshots_on_the_host_keep_the_host_formula(monkeypatch):
    """A store over a host tensor, and a stand-in that merely says ``is_cuda``: no device call, the host formula."""
    import torch

    from pulser_amd import QState, engine
    from pulser_amd.results import CoherentResults, DeviceState, LazyState, SnapshotStore, StateResult, _ptrace_host

    def no_device(*args, **kw):
        raise AssertionError("the device route was taken")

    monkeypatch.setattr(engine, "reduced_density_dm", no_device)
    monkeypatch.setattr(engine, "reduced_density", no_device)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(3, 1, 8, 8)) + 1j * rng.normal(size=(3, 1, 8, 8))

    class StandIn:
        is_cuda = True

        def __init__(self, a):
            self.a = a

        shape = property(lambda self: self.a.shape)
        nbytes = property(lambda self: self.a.nbytes)

        def dim(self):
            return self.a.ndim

        def __getitem__(self, key):
            return StandIn(self.a[key])

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    for tensor in (torch.from_numpy(x), StandIn(x)):
        store = SnapshotStore(tensor)
        states = [QState(np.eye(8))] + [LazyState(store, i, 0, (8, 8)) for i in range(3)]
        rs = [StateResult(("a", "b", "c"), "ground-rydberg", st, True, evaluation_time=k / 3) for k, st in enumerate(states)]
        res = CoherentResults(rs, 3, "ground-rydberg", np.linspace(0.0, 0.1, 4), "ground-rydberg", None)
        one = states[2].ptrace([2, 0])  # a single state first: read, then the host formula
        assert np.array_equal(one, _ptrace_host(x[1, 0], False, [0, 2], 2))
        got = res.reduced_states([1])
        assert np.array_equal(got[0], _ptrace_host(np.eye(8), False, [1], 2))
        for i in range(3):
            assert np.array_equal(got[i + 1], _ptrace_host(x[i, 0], False, [1], 2))
    assert np.array_equal(DeviceState(tensor=torch.from_numpy(x[0, 0])).ptrace([0]), _ptrace_host(x[0, 0], False, [0], 2))


def test_split_count_restates_the_library_rule():
    """``reduced_density_dm_splits``: min(1024 // T, steps // 8), steps = R / NS (dA^2 <= 256), else R // 4; at least 1."""
    from pulser_amd.engine import reduced_density_dm_splits as splits

    assert splits(1, 2**14, 2) == 16      # R = 8192, 64 slots: 128 steps
    assert splits(1, 2**13, 4) == 16      # R = 2048, 16 slots: 128 steps
    assert splits(12, 2**6, 4) == 1       # R = 16, 16 slots: one step
    assert splits(1, 2**13, 64) == 32     # 16 entries per thread: R = 128 steps, 4 per split
    assert splits(1, 2**10, 32) == 8      # 4 entries per thread: R = 32
    assert splits(128, 2**10, 2) == 1     # R = 512, 64 slots: 8 steps
    assert splits(512, 2**14, 2) == 2     # capped by 1024 // T
    assert splits(1, 3**5, 3, 3) == 1     # R = 81, 27 slots: 3 steps
    assert splits(1, 3**8, 3, 3) == 10    # R = 2187, 27 slots: 81 steps
    assert splits(1, 2, 2) == 1 and splits(0, 4, 2) == 1


def test_engine_wrapper_refuses_before_it_needs_a_device():
    import torch

    from pulser_amd.engine import reduced_density, reduced_density_dm  # (the ket call is still there, as it was)

    assert callable(reduced_density)
    x = torch.zeros((2, 3, 8, 8), dtype=torch.complex128)
    with pytest.raises(ValueError, match="CUDA"):  # a host tensor, everything else in order
        reduced_density_dm(x, [1])
    with pytest.raises(ValueError, match="CUDA"):
        reduced_density_dm(x.numpy(), [1])
    with pytest.raises(TypeError, match="complex128"):
        reduced_density_dm(x.to(torch.complex64), [1])
    with pytest.raises(TypeError, match="complex128"):
        reduced_density_dm(x.real, [1])
    for shape in ((2, 3, 64), (2, 8, 8), (2, 3, 8, 4), (2, 0, 8, 8), (2, 1, 2, 8, 8)):
        with pytest.raises(ValueError, match="shape"):
            reduced_density_dm(torch.zeros(shape, dtype=torch.complex128), [1])
    with pytest.raises(ValueError, match="contiguous"):  # a transposed matrix axis
        reduced_density_dm(x.transpose(2, 3), [1])
    with pytest.raises(ValueError, match="contiguous"):  # a padded row
        reduced_density_dm(torch.zeros((2, 3, 8, 12), dtype=torch.complex128)[..., :8], [1])
    with pytest.raises(ValueError, match="contiguous"):  # every second column
        reduced_density_dm(torch.zeros((2, 3, 8, 16), dtype=torch.complex128)[..., ::2], [1])
    with pytest.raises(ValueError, match="64"):
        reduced_density_dm(torch.zeros((1, 1, 128, 128), dtype=torch.complex128), range(7))
    with pytest.raises(ValueError, match="64"):
        reduced_density_dm(torch.zeros((1, 1, 81, 81), dtype=torch.complex128), range(4), local_dim=3)
    for keep in ([], [1, 1], [3], [-1], [0.5]):
        with pytest.raises(ValueError):
            reduced_density_dm(x, keep)
    with pytest.raises(ValueError, match="power"):
        reduced_density_dm(x, [0], local_dim=3)  # 8 is no power of 3
    with pytest.raises(ValueError, match="local_dim"):
        reduced_density_dm(x, [0], local_dim=5)
    with pytest.raises(ValueError, match="n_split"):
        reduced_density_dm(x, [0], n_split=-1)

"""Python face of the C ABI: device tables in, torch tensors as state storage.

PyTorch is plumbing only (device memory, streams).  All arithmetic of the hot
path happens in the hand-written HIP kernels of ``csrc/rydemu.hip`` through
``librydemu.so``; this module never computes a fallback on the host.
"""

from __future__ import annotations

import ctypes as C
from typing import Any, Mapping, NamedTuple, Sequence

import numpy as np

from . import _lib
from ._lib import RYD_GENERAL_DENSITY, RYD_MESOLVE, RYD_SESOLVE, RydConfig, RydOpts, RydQDesc, RydStats
from .terms import DeviceTables, lower


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(
            "pulser_amd needs an AMD GPU visible to PyTorch-ROCm "
            "(torch.cuda.is_available() is False); there is no CPU fallback."
        )
    return torch


# ryd_opts.method: propagator of the multi-launch sesolve path ("auto": split-operator for
# two-level kets of 15+ atoms, Taylor polynomial otherwise)
_METHODS = {"auto": 0, "krylov": 1, "split": 2, "taylor": 3}


def _method_code(method: str) -> int:
    try:
        return _METHODS[method]
    except KeyError:
        raise ValueError(f"unknown method {method!r}; one of {sorted(_METHODS)}") from None


def _obs_what(occupation: bool, correlation: bool, energy: bool, density: bool = False) -> int:
    """The RYD_OBS_* bits of the ``what`` argument of the observe calls."""
    return (1 if occupation else 0) | (2 if correlation else 0) | (4 if energy else 0) | (8 if density else 0)


def _obs_unpack(out: Any, n: int) -> dict[str, np.ndarray]:
    """Host views of the observe calls' output ``[..., N*N + N + 3]`` (any leading axes), by name."""
    o = out.cpu().numpy()
    return {"occupation": o[..., :n], "norm2": o[..., n],
            "correlation": o[..., n + 1:n + 1 + n * n].reshape(*o.shape[:-1], n, n),
            "energy": o[..., n * n + n + 1], "energy2": o[..., n * n + n + 2]}


def _many_args(torch: Any, device: Any, states: Any, times: Any,
               tail: tuple[int, ...]) -> tuple[int, int, int, int, np.ndarray]:
    """The arguments the ``*_many`` observe calls share.  ``states`` is a complex128 tensor ``[T, B >= 1, *tail]`` on
    ``device`` whose trailing axes are contiguous (the first two may be strided); ``tail`` is ``(dim,)`` for kets and
    ``(d, d)`` for density matrices.  ``times`` has one entry per state of the first axis.  Returns T, B, the strides
    of the first two axes in elements and ``times`` as a contiguous float64 array."""
    if not (isinstance(states, torch.Tensor) and states.is_cuda and states.device == device):
        raise ValueError(f"states must be a torch tensor on {device}")
    if states.dtype != torch.complex128:
        raise ValueError(f"states must be complex128, got {states.dtype}")
    if states.dim() != 2 + len(tail) or tuple(states.shape[2:]) != tail or int(states.shape[1]) < 1:
        raise ValueError(f"states must have the shape [T, B >= 1, {', '.join(map(str, tail))}], got {tuple(states.shape)}")
    if states.stride(-1) != 1 or (len(tail) == 2 and states.stride(2) != tail[1]):
        raise ValueError(f"the last {'axis' if len(tail) == 1 else 'two axes'} of states must be contiguous"
                         " (the first two may be strided)")
    n_t, n_b = int(states.shape[0]), int(states.shape[1])
    tt = np.ascontiguousarray(times, dtype=np.float64)
    if tt.shape != (n_t,):
        raise ValueError(f"need one time per state of the first axis ({n_t}), got {tt.shape}")
    # (the stride of an axis of length 1 is arbitrary in torch and never used: any valid value will do)
    elems = int(np.prod(tail))
    stride_b = int(states.stride(1)) if n_b > 1 else elems
    stride_t = int(states.stride(0)) if n_t > 1 else max(n_b * stride_b, elems)
    return n_t, n_b, stride_t, stride_b, tt


def outer_accumulate(psi: Any, acc: Any, weights: Any = None) -> None:
    """``acc[D, D] += sum_b w_b |psi_b><psi_b|`` on the device, without a solver handle and for any
    state dimension (``ryd_outer_accumulate_dim``): the trajectory mean of
    pulser_simulation/aggregators.py:20-37.  ``psi`` complex128[B, D] and ``acc`` complex128[D, D]
    are contiguous CUDA tensors on the same device."""
    torch = _torch()
    if not (psi.is_cuda and acc.is_cuda and psi.device == acc.device):
        raise ValueError("psi and acc must be CUDA tensors on the same device")
    if psi.dtype != torch.complex128 or acc.dtype != torch.complex128:
        raise TypeError("complex128 tensors expected")
    if psi.dim() != 2 or tuple(acc.shape) != (psi.shape[1], psi.shape[1]):
        raise ValueError(f"shapes {tuple(psi.shape)} / {tuple(acc.shape)} do not match [B, D] / [D, D]")
    if not (psi.is_contiguous() and acc.is_contiguous()):
        raise ValueError("contiguous tensors expected")
    wptr = None
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (psi.shape[0],):
            raise ValueError(f"need one weight per state ({psi.shape[0]}), got {weights.shape}")
        wptr = weights.ctypes.data
    _lib.check(_lib.load().ryd_outer_accumulate_dim(
        psi.data_ptr(), int(psi.shape[0]), int(psi.shape[1]), wptr, acc.data_ptr(), int(psi.device.index or 0),
        torch.cuda.current_stream(psi.device).cuda_stream))


def ensemble_diag(states: Any, diag: Any) -> None:
    """``diag[i, x] += sum_b |states[i, b, x]|^2`` on the device, without a solver handle and for any state dimension
    (``ryd_ensemble_diag``): the diagonal of the trajectory sum of pulser_simulation/aggregators.py:20-37 at every
    evaluation time, all that sampling the averaged state reads - the ``[D, D]`` matrices are never formed.  ``states``
    is a complex128 CUDA tensor ``[T, B >= 1, D]`` or a view of one whose last axis is contiguous (the strides of the
    first two axes are passed on); ``diag`` is a contiguous float64 ``[T, D]`` on the same device and is accumulated
    into: zero it once, call once per chunk of trajectories.  No atomics: repeated calls give bitwise equal sums."""
    torch = _torch()
    if not (isinstance(states, torch.Tensor) and isinstance(diag, torch.Tensor)
            and states.is_cuda and diag.is_cuda and states.device == diag.device):
        raise ValueError("states and diag must be CUDA tensors on the same device")
    if states.dtype != torch.complex128 or diag.dtype != torch.float64:
        raise TypeError("a complex128 states tensor and a float64 diag tensor expected")
    if states.dim() != 3 or int(states.shape[1]) < 1 or int(states.shape[2]) < 1 \
            or tuple(diag.shape) != (states.shape[0], states.shape[2]):
        raise ValueError(f"shapes {tuple(states.shape)} / {tuple(diag.shape)} do not match [T, B >= 1, D] / [T, D]")
    if not diag.is_contiguous():
        raise ValueError("a contiguous diag tensor expected")
    n_t, n_b, dim = (int(v) for v in states.shape)
    if n_t == 0:
        return
    if states.stride(2) != 1 and dim > 1:
        raise ValueError("the last axis of states must be contiguous (the first two may be strided)")
    # (the stride of an axis of length 1 is arbitrary in torch and never used: any valid value will do)
    stride_b = int(states.stride(1)) if n_b > 1 else dim
    stride_t = int(states.stride(0)) if n_t > 1 else max(n_b * stride_b, dim)
    if stride_b < dim or stride_t < dim:
        raise ValueError(f"strides {stride_t} / {stride_b} of the first two axes are smaller than a state ({dim})")
    _lib.check(_lib.load().ryd_ensemble_diag(
        states.data_ptr(), n_t, n_b, stride_t, stride_b, dim, diag.data_ptr(), int(states.device.index or 0),
        torch.cuda.current_stream(states.device).cuda_stream))


# dA of ryd_reduced_density and ryd_reduced_density_dm at most: six qubits, three qutrits, three four-level atoms
REDUCED_DENSITY_MAX_ROWS = 64


def check_keep(keep: Any, n_sites: int) -> tuple[int, ...]:
    """``keep`` (any iterable of ints: the sites of a subsystem) sorted, as a tuple.  ``ValueError`` when it is empty,
    holds something that is no integer, a duplicate, or a site outside ``0 .. n_sites - 1``."""
    try:
        raw = list(keep)
    except TypeError:
        raise ValueError(f"keep must be an iterable of site indices, got {keep!r}") from None
    if not raw:
        raise ValueError("keep is empty: a subsystem needs at least one site")
    if not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in raw):
        raise ValueError(f"keep must hold integers, got {raw!r}")
    sites = tuple(sorted(int(k) for k in raw))
    if len(set(sites)) != len(sites):
        raise ValueError(f"keep holds a site twice: {raw!r}")
    if sites[0] < 0 or sites[-1] >= n_sites:
        raise ValueError(f"keep {raw!r} holds a site outside 0 .. {n_sites - 1}")
    return sites


def sites_of_dim(dim: int, local_dim: int) -> int:
    """n with ``local_dim**n == dim``; ``ValueError`` when there is none."""
    if local_dim < 2:
        raise ValueError(f"local_dim must be at least 2, got {local_dim}")
    n, d = 0, 1
    while d < dim:
        d *= local_dim
        n += 1
    if d != dim or n < 1:
        raise ValueError(f"the dimension {dim} is not a power (>= 1) of local_dim = {local_dim}")
    return n


def reduced_density(states: Any, keep: Any, local_dim: int = 2, out: Any = None, n_split: int = 0) -> Any:
    """``out[t, a, a'] += sum_b sum_r psi(t, b)[idx(a, r)] conj psi(t, b)[idx(a', r)]`` on the device
    (``ryd_reduced_density``): the partial trace ``Tr_rest |psi><psi|`` of every ket over the sites ``keep``, summed
    over axis 1 - what ``Qobj.ptrace(keep)`` gives for the states of a run, without a state leaving the device.

    ``states`` is a complex128 CUDA tensor ``[T, B >= 1, D]`` with ``D = local_dim**n`` (``local_dim`` 2, 3 or 4), or a
    view of one whose last axis is contiguous (the strides of the first two axes are passed on, as for
    ``ensemble_diag``); a caller who wants one matrix per ``(t, b)`` passes ``x.reshape(T * B, 1, D)``.  Site 0 is the
    most significant digit.  ``keep`` is any iterable of distinct sites; it is sorted, and row ``a`` of the result is
    the number formed by the kept digits in ascending site order.  ``dA = local_dim**len(keep)`` is at most 64.

    Returns ``out``, complex128 ``[T, dA, dA]`` contiguous on the same device: a new zero tensor when none is given,
    else the one given, which is ACCUMULATED into (call once per chunk of trajectories).  Both triangles are written,
    exactly conjugate to each other.  ``n_split`` workgroups share one time: 1 is one workgroup per time, 0 lets the
    library choose.  A scratch tensor is allocated only when a split is used: ``T * n_split * dA * dA`` complex128 for
    a given ``n_split > 1``, and for ``n_split = 0`` at most ``min(1024 // T, D // 512)`` such partials per time
    (none when that is below 2: the library then takes one workgroup per time).  No atomics: repeated calls with the
    same ``n_split`` give bitwise equal results."""
    torch = _torch()
    if not (isinstance(states, torch.Tensor) and states.is_cuda):
        raise ValueError("states must be a CUDA tensor")
    if states.dtype != torch.complex128:
        raise TypeError(f"a complex128 states tensor expected, got {states.dtype}")
    if states.dim() != 3 or int(states.shape[1]) < 1 or int(states.shape[2]) < 1:
        raise ValueError(f"shape {tuple(states.shape)} does not match [T, B >= 1, D]")
    n_t, n_b, dim = (int(v) for v in states.shape)
    if int(local_dim) not in (2, 3, 4):
        raise ValueError(f"local_dim must be 2, 3 or 4, got {local_dim}")
    local_dim = int(local_dim)
    n_sites = sites_of_dim(dim, local_dim)
    sites = check_keep(keep, n_sites)
    d_a = local_dim ** len(sites)
    if d_a > REDUCED_DENSITY_MAX_ROWS:
        raise ValueError(f"{len(sites)} sites of local dimension {local_dim} make a {d_a} x {d_a} matrix: the device "
                         f"partial trace serves at most {REDUCED_DENSITY_MAX_ROWS} rows")
    if out is None:
        out = torch.zeros((n_t, d_a, d_a), dtype=torch.complex128, device=states.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == states.device):
            raise ValueError("states and out must be CUDA tensors on the same device")
        if out.dtype != torch.complex128:
            raise TypeError(f"a complex128 out tensor expected, got {out.dtype}")
        if tuple(out.shape) != (n_t, d_a, d_a):
            raise ValueError(f"out has the shape {tuple(out.shape)}, expected {(n_t, d_a, d_a)}")
        if not out.is_contiguous():
            raise ValueError("a contiguous out tensor expected")
    n_split = int(n_split)
    if n_split < 0:
        raise ValueError(f"n_split must be 0 (the library's choice) or positive, got {n_split}")
    if n_t == 0:
        return out
    if states.stride(2) != 1 and dim > 1:
        raise ValueError("the last axis of states must be contiguous (the first two may be strided)")
    # (the stride of an axis of length 1 is arbitrary in torch and never used: any valid value will do)
    stride_b = int(states.stride(1)) if n_b > 1 else dim
    stride_t = int(states.stride(0)) if n_t > 1 else max(n_b * stride_b, dim)
    if stride_b < dim or stride_t < dim:
        raise ValueError(f"strides {stride_t} / {stride_b} of the first two axes are smaller than a state ({dim})")
    parts = n_split
    if n_split == 0:
        parts = min(1024 // n_t, dim // 512)
        if parts < 2:
            n_split, parts = 1, 1
    scratch = None
    if parts > 1:
        scratch = torch.empty((n_t, parts, d_a, d_a), dtype=torch.complex128, device=states.device)
    keep_arr = np.ascontiguousarray(sites, dtype=np.int32)
    _lib.check(_lib.load().ryd_reduced_density(
        states.data_ptr(), n_t, n_b, stride_t, stride_b, dim, local_dim, n_sites, keep_arr.ctypes.data, len(sites),
        out.data_ptr(), n_split, None if scratch is None else scratch.data_ptr(),
        0 if scratch is None else scratch.numel() * 16, int(states.device.index or 0),
        torch.cuda.current_stream(states.device).cuda_stream))
    return out


def reduced_density_dm_splits(n_times: int, dim: int, d_a: int, local_dim: int = 2) -> int:
    """The most workgroups per time ``ryd_reduced_density_dm`` takes when it chooses (``n_split = 0``), given the
    scratch for them - the library's own rule: ``min(1024 // T, steps // 8)``, at least 1, where a workgroup walks
    ``steps = R / NS`` steps per matrix, ``R = D / dA`` and ``NS`` the largest power of ``local_dim`` with
    ``NS * dA^2 <= 256`` (at most ``R``); from ``dA^2 > 256`` on ``NS = 1`` and the rule is ``steps // 4``."""
    rest = dim // d_a
    slots, per_split = 1, 4
    if d_a * d_a <= 256:
        per_split = 8
        while slots * local_dim <= rest and d_a * d_a * slots * local_dim <= 256:
            slots *= local_dim
    return max(1, min(1024 // max(n_times, 1), rest // slots // per_split))


def reduced_density_dm(states: Any, keep: Any, local_dim: int = 2, out: Any = None, n_split: int = 0) -> Any:
    """``out[t, a, a'] += sum_b sum_r rho(t, b)[idx(a, r), idx(a', r)]`` on the device (``ryd_reduced_density_dm``):
    the partial trace ``Tr_rest rho`` of every density matrix over the sites ``keep``, summed over axis 1 - what
    ``Qobj.ptrace(keep)`` gives for the matrices of a master-equation run, without a matrix leaving the device.  Only
    ``dA * D`` of the ``D * D`` elements of a matrix are read.

    ``states`` is a complex128 CUDA tensor ``[T, B >= 1, D, D]`` with ``D = local_dim**n`` (``local_dim`` 2, 3 or 4), or
    a view of one whose last two axes are contiguous (the strides of the first two axes are passed on).  Sites, ``keep``
    and the row order are those of ``reduced_density``; ``dA = local_dim**len(keep)`` is at most 64, and keeping every
    site is valid.  Nothing is assumed Hermitian: every entry is the sum of the stored elements the formula names,
    nothing is mirrored, conjugated or divided by a trace.

    Returns ``out``, complex128 ``[T, dA, dA]`` contiguous on the same device: a new zero tensor when none is given,
    else the one given, which is ACCUMULATED into.  ``n_split`` workgroups share one time: 1 is one workgroup per time,
    0 lets the library choose.  A scratch tensor is allocated only when a split is used: ``T * n_split * dA * dA``
    complex128 for a given ``n_split > 1``, and for ``n_split = 0`` the ``reduced_density_dm_splits(T, D, dA, local_dim)``
    partials per time the library can use (none when that is 1: one workgroup per time).  No atomics: repeated
    calls with the same ``n_split`` give bitwise equal results."""
    import torch

    # (what can be said of a tensor wherever it lives is said first: the checks below need no device)
    if not isinstance(states, torch.Tensor):
        raise ValueError("states must be a CUDA tensor")
    if states.dtype != torch.complex128:
        raise TypeError(f"a complex128 states tensor expected, got {states.dtype}")
    if states.dim() != 4 or int(states.shape[1]) < 1 or int(states.shape[2]) < 1 or states.shape[2] != states.shape[3]:
        raise ValueError(f"shape {tuple(states.shape)} does not match [T, B >= 1, D, D]")
    n_t, n_b, dim = (int(v) for v in states.shape[:3])
    if int(local_dim) not in (2, 3, 4):
        raise ValueError(f"local_dim must be 2, 3 or 4, got {local_dim}")
    local_dim = int(local_dim)
    n_sites = sites_of_dim(dim, local_dim)
    sites = check_keep(keep, n_sites)
    d_a = local_dim ** len(sites)
    if d_a > REDUCED_DENSITY_MAX_ROWS:
        raise ValueError(f"{len(sites)} sites of local dimension {local_dim} make a {d_a} x {d_a} matrix: the device "
                         f"partial trace serves at most {REDUCED_DENSITY_MAX_ROWS} rows")
    if n_t > 0 and ((states.stride(3) != 1 and dim > 1) or states.stride(2) != dim):
        raise ValueError("the last two axes of states must be contiguous (the first two may be strided)")
    n_split = int(n_split)
    if n_split < 0:
        raise ValueError(f"n_split must be 0 (the library's choice) or positive, got {n_split}")
    if not states.is_cuda:
        raise ValueError("states must be a CUDA tensor")
    _torch()
    if out is None:
        out = torch.zeros((n_t, d_a, d_a), dtype=torch.complex128, device=states.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == states.device):
            raise ValueError("states and out must be CUDA tensors on the same device")
        if out.dtype != torch.complex128:
            raise TypeError(f"a complex128 out tensor expected, got {out.dtype}")
        if tuple(out.shape) != (n_t, d_a, d_a):
            raise ValueError(f"out has the shape {tuple(out.shape)}, expected {(n_t, d_a, d_a)}")
        if not out.is_contiguous():
            raise ValueError("a contiguous out tensor expected")
    if n_t == 0:
        return out
    # (the stride of an axis of length 1 is arbitrary in torch and never used: any valid value will do)
    stride_b = int(states.stride(1)) if n_b > 1 else dim * dim
    stride_t = int(states.stride(0)) if n_t > 1 else max(n_b * stride_b, dim * dim)
    if stride_b < dim * dim or stride_t < dim * dim:
        raise ValueError(f"strides {stride_t} / {stride_b} of the first two axes are smaller than a matrix ({dim * dim})")
    parts = n_split
    if n_split == 0:
        parts = reduced_density_dm_splits(n_t, dim, d_a, local_dim)
        if parts < 2:
            n_split, parts = 1, 1
    scratch = None
    if parts > 1:
        scratch = torch.empty((n_t, parts, d_a, d_a), dtype=torch.complex128, device=states.device)
    keep_arr = np.ascontiguousarray(sites, dtype=np.int32)
    _lib.check(_lib.load().ryd_reduced_density_dm(
        states.data_ptr(), n_t, n_b, stride_t, stride_b, dim, local_dim, n_sites, keep_arr.ctypes.data, len(sites),
        out.data_ptr(), n_split, None if scratch is None else scratch.data_ptr(),
        0 if scratch is None else scratch.numel() * 16, int(states.device.index or 0),
        torch.cuda.current_stream(states.device).cuda_stream))
    return out


def accumulate(x: Any, acc: Any, weight: float = 1.0) -> None:
    """``acc += weight * x`` elementwise on the device (``ryd_accumulate``): the running sum of
    trajectory density matrices of aggregators.py:29-35."""
    torch = _torch()
    if not (x.is_cuda and acc.is_cuda and x.device == acc.device) or x.shape != acc.shape:
        raise ValueError("x and acc must be CUDA tensors of one shape on the same device")
    if x.dtype != torch.complex128 or acc.dtype != torch.complex128 or not (x.is_contiguous() and acc.is_contiguous()):
        raise TypeError("contiguous complex128 tensors expected")
    _lib.check(_lib.load().ryd_accumulate(
        x.data_ptr(), float(weight), int(x.numel()), acc.data_ptr(), int(x.device.index or 0),
        torch.cuda.current_stream(x.device).cuda_stream))


class SparseTriplets(NamedTuple):
    """The stored non-zeros of a ``dim`` x ``dim`` operator as ``ryd_expect_sparse`` reads them, already on a device:
    ``idx`` int32[2 nnz] (the rows, then the columns) and ``vals`` complex128[nnz], duplicates summed, sorted by
    (row, column).  ``sparse_triplets`` builds one; ``expect_sparse`` takes it in place of the operator, so that a
    caller with many stacks of states (the chunks of a trajectory ensemble) uploads the operator once."""

    dim: int
    nnz: int
    idx: Any
    vals: Any


def _host_triplets(operator: Any, dim: int) -> tuple[np.ndarray, np.ndarray]:
    """(rows then columns int32[2 nnz], values complex128[nnz]) of ``operator``'s stored non-zeros, checked against
    ``dim``."""
    import scipy.sparse as sp

    m = sp.csr_matrix(operator) if not sp.issparse(operator) else operator.tocsr()
    if m.shape[0] != m.shape[1]:
        raise ValueError(f"square operator expected, got {tuple(m.shape)}")
    if m.shape[0] != dim:
        raise ValueError(f"operator of shape {tuple(m.shape)} does not match states of dimension {dim}")
    if m.nnz >= 2**31:
        raise ValueError(f"{m.nnz} non-zeros: at most 2^31 - 1")
    m = m.astype(np.complex128)  # (a copy: the caller's matrix is not reordered)
    m.sum_duplicates()
    m.sort_indices()
    nnz = int(m.nnz)
    cols = np.ascontiguousarray(m.indices, dtype=np.int32)
    rows = np.repeat(np.arange(dim, dtype=np.int32), np.diff(m.indptr))
    if nnz and (len(rows) != nnz or cols.min() < 0 or cols.max() >= dim):
        raise ValueError("operator indices outside [0, dim)")
    return np.concatenate([rows, cols]), np.ascontiguousarray(m.data, dtype=np.complex128)


def sparse_triplets(operator: Any, dim: int, device: Any) -> SparseTriplets:
    """``operator`` (anything ``scipy.sparse`` accepts, ``dim`` x ``dim``) as :class:`SparseTriplets` on ``device``."""
    torch = _torch()
    idx, vals = _host_triplets(operator, int(dim))
    return SparseTriplets(int(dim), len(vals), torch.from_numpy(idx).to(device), torch.from_numpy(vals).to(device))


def expect_sparse(states: Any, operator: Any, *, density: bool = False) -> Any:
    """``<x_s| O |x_s>`` for kets ``states`` complex128[S, D], or ``Tr(O rho_s)`` for density matrices
    complex128[S, D, D] (``density=True``), on the device and for every state in one launch
    (``ryd_expect_sparse``): ``qutip.expect`` of simresults.py:89-132 over the states of a run.  ``states`` is a
    CUDA tensor whose inner dimensions are contiguous; dim 0 may be strided (``dev[:, b]`` of a ``[T, B, D]``
    snapshot tensor).  ``operator`` is anything ``scipy.sparse`` accepts, D x D; only its stored non-zeros are
    visited - or the :class:`SparseTriplets` of one, uploaded earlier to the device of ``states``.  Returns a CUDA
    complex128 tensor [S]."""
    torch = _torch()
    if not (hasattr(states, "is_cuda") and states.is_cuda):
        raise ValueError("states must be a CUDA tensor")
    if states.dtype != torch.complex128:
        raise TypeError("complex128 tensor expected")
    if states.dim() != (3 if density else 2) or (density and states.shape[1] != states.shape[2]):
        raise ValueError(f"shape {tuple(states.shape)} does not match {'[S, D, D]' if density else '[S, D]'}")
    n_states, dim = int(states.shape[0]), int(states.shape[-1])
    inner = (dim, 1) if density else (1,)
    if dim < 1 or (n_states > 0 and tuple(states.stride()[1:]) != inner) or (n_states > 1 and states.stride(0) < dim ** len(inner)):
        raise ValueError("the inner dimensions of states must be contiguous (dim 0 may be strided)")
    if isinstance(operator, SparseTriplets):
        if operator.dim != dim:
            raise ValueError(f"operator of shape {(operator.dim, operator.dim)} does not match states of dimension {dim}")
        if operator.idx.device != states.device or operator.vals.device != states.device:
            raise ValueError(f"operator triplets on {operator.idx.device}, states on {states.device}")
        host = None
    else:
        host = _host_triplets(operator, dim)
    out = torch.empty(n_states, dtype=torch.complex128, device=states.device)
    if n_states == 0:
        return out
    if host is None:
        nnz, idx, vals = operator.nnz, operator.idx, operator.vals
    else:
        nnz = len(host[1])
        idx = torch.from_numpy(host[0]).to(states.device)
        vals = torch.from_numpy(host[1]).to(states.device)
    stride = int(states.stride(0)) if n_states > 1 else dim ** len(inner)
    _lib.check(_lib.load().ryd_expect_sparse(
        states.data_ptr(), n_states, stride, dim, int(bool(density)), idx.data_ptr(), idx.data_ptr() + 4 * nnz,
        vals.data_ptr(), nnz, out.data_ptr(), int(states.device.index or 0),
        torch.cuda.current_stream(states.device).cuda_stream))
    return out


def overlap_many(states: Any, targets: Any, *, density: bool = False, outer: bool = False) -> tuple[Any, Any]:
    """``z[s, f] = <a_f|x_s>`` and ``norm[s] = <x_s|x_s>`` for kets ``states`` complex128[S, D]; with ``density=True``,
    ``states`` complex128[S, D, D], ``z[s, f] = Tr(A_f^dag rho_s)`` for matrix targets or, with ``outer=True``,
    ``<phi_f|rho_s|phi_f>`` for ket targets (``|phi><phi|`` is never formed), and ``norm[s] = Re Tr rho_s`` - for every
    state and target in one launch (``ryd_overlap_many``): ``QutipState.overlap`` of qutip_state.py:86-110 over the
    states of a run, with the number each state is normalised by.  ``states`` is a CUDA tensor whose inner dimensions
    are contiguous; dim 0 may be strided (``dev[:, b]`` of a ``[T, B, D]`` snapshot tensor).  ``targets`` is a CUDA
    tensor or a host array, ``[F, D]`` (kets, or ``outer``) or ``[F, D * D]`` / ``[F, D, D]`` (matrix targets); F = 0
    gives the norms alone.  Returns CUDA tensors ``z`` complex128[S, F] and ``norm`` float64[S]."""
    torch = _torch()
    if not (hasattr(states, "is_cuda") and states.is_cuda):
        raise ValueError("states must be a CUDA tensor")
    if states.dtype != torch.complex128:
        raise TypeError("complex128 tensor expected")
    if outer and not density:
        raise ValueError("outer=True (ket targets on density matrices) needs density=True")
    if states.dim() != (3 if density else 2) or (density and states.shape[1] != states.shape[2]):
        raise ValueError(f"shape {tuple(states.shape)} does not match {'[S, D, D]' if density else '[S, D]'}")
    n_states, dim = int(states.shape[0]), int(states.shape[-1])
    inner = (dim, 1) if density else (1,)
    elems = dim ** len(inner)
    if dim < 1 or (n_states > 0 and tuple(states.stride()[1:]) != inner) or (n_states > 1 and states.stride(0) < elems):
        raise ValueError("the inner dimensions of states must be contiguous (dim 0 may be strided)")
    tlen = dim if outer else elems
    if isinstance(targets, torch.Tensor):
        if targets.dtype != torch.complex128:
            raise TypeError(f"complex128 targets expected, got {targets.dtype}")
        if targets.device != states.device and targets.is_cuda:
            raise ValueError(f"targets on {targets.device}, states on {states.device}")
        tg = targets
    else:
        host = np.asarray(targets)
        if host.dtype.kind not in "biufc":
            raise TypeError(f"numeric targets expected, got {host.dtype}")
        tg = torch.from_numpy(np.ascontiguousarray(host, dtype=np.complex128))
    shapes = [(tlen,)] + ([(dim, dim)] if density and not outer else [])
    if tg.dim() < 2 or tuple(int(v) for v in tg.shape[1:]) not in shapes:
        raise ValueError(f"targets of shape {tuple(tg.shape)} do not match "
                         + " or ".join(f"[F, {', '.join(map(str, s))}]" for s in shapes))
    n_targets = int(tg.shape[0])
    if n_targets > 4 * 65535:  # (tiles of 4 targets along one grid dimension)
        raise ValueError(f"{n_targets} targets: at most {4 * 65535}")
    tg = tg.reshape(n_targets, tlen).contiguous().to(states.device)
    z = torch.empty((n_states, n_targets), dtype=torch.complex128, device=states.device)
    norm = torch.empty(n_states, dtype=torch.float64, device=states.device)
    if n_states == 0:
        return z, norm
    stride = int(states.stride(0)) if n_states > 1 else elems
    _lib.check(_lib.load().ryd_overlap_many(
        states.data_ptr(), n_states, stride, dim, int(bool(density)), tg.data_ptr() if n_targets else None, n_targets,
        int(bool(outer)), z.data_ptr() if n_targets else None, norm.data_ptr(), int(states.device.index or 0),
        torch.cuda.current_stream(states.device).cuda_stream))
    return z, norm


class Engine:
    """One ``ryd_handle``: a batch of B states of N atoms on one device.

    Mirrors the role of the ``QobjEvo`` + solver pair the reference builds at
    pulser-simulation/pulser_simulation/simulation.py:729-735.
    """

    def __init__(
        self,
        tables: DeviceTables,
        mode: str = "sesolve",
        device: int | None = None,
        tile_bits: int = 0,
    ) -> None:
        self.torch = _torch()
        self.lib = _lib.load()
        self.tables = tables
        self.n = tables.n_qubits
        self.batch = tables.batch
        if mode not in ("sesolve", "mesolve", "mcsolve"):
            raise ValueError(f"unknown mode {mode!r}")
        self.mode = RYD_MESOLVE if mode == "mesolve" else RYD_SESOLVE
        self.monte_carlo = mode == "mcsolve"
        self.device_index = (
            self.torch.cuda.current_device() if device is None else int(device)
        )
        self.device = self.torch.device("cuda", self.device_index)
        cfg = RydConfig(
            abi_version=_lib.RYD_ABI_VERSION,
            n_qubits=self.n,
            batch=self.batch,
            mode=self.mode,
            device=self.device_index,
            tile_bits=tile_bits,
        )
        self._h = C.c_void_p()
        _lib.check(self.lib.ryd_create(C.byref(cfg), C.byref(self._h)))
        self._snap_map: tuple[int, int] | None = None  # (slots, kets the map reaches) of set_snapshot_map
        self._upload()

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ryd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "Engine":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()

    # -- tables -----------------------------------------------------------
    def _upload(self) -> None:
        t = self.tables
        tk = np.ascontiguousarray(t.tknots, dtype=np.float64)
        pp = np.ascontiguousarray(t.pp, dtype=np.complex128)
        _lib.check(
            self.lib.ryd_set_series(
                self._h, pp.shape[0], len(tk), tk.ctypes.data, pp.ctypes.data
            )
        )
        desc = np.ascontiguousarray(t.desc)
        assert desc.dtype.itemsize == C.sizeof(RydQDesc)
        _lib.check(self.lib.ryd_set_qubit_desc(self._h, desc.ctypes.data))
        if t.dterms is not None and len(t.dterms):
            dt = np.ascontiguousarray(t.dterms)
            assert dt.dtype.itemsize == C.sizeof(_lib.RydDTerm)
            _lib.check(self.lib.ryd_set_detuning_terms(self._h, len(dt), dt.ctypes.data))
        u = np.ascontiguousarray(t.interaction, dtype=np.float64)
        _lib.check(self.lib.ryd_set_interaction(self._h, u.ctypes.data, u.shape[0]))
        if self.mode == RYD_MESOLVE and t.dissipator is not None:
            s = np.ascontiguousarray(t.dissipator, dtype=np.complex128)
            _lib.check(self.lib.ryd_set_dissipator(self._h, s.ctypes.data))
        if self.monte_carlo:
            if t.collapse_local is None:
                raise ValueError("mcsolve needs collapse operators (tables.collapse_local)")
            c = np.ascontiguousarray(t.collapse_local, dtype=np.complex128)
            if c.shape[1:] != (2, 2):
                raise NotImplementedError("Monte-Carlo trajectories need 2-level collapse operators")
            _lib.check(self.lib.ryd_set_collapse(self._h, c.shape[0], c.ctypes.data))

    @classmethod
    def from_problems(
        cls, problems: Sequence[Mapping[str, Any]], mode: str | None = None, **kw: Any
    ) -> "Engine":
        tables = lower(problems)
        if mode is None:
            mode = "mesolve" if tables.dissipator is not None else "sesolve"
        return cls(tables, mode=mode, **kw)

    # -- state helpers ----------------------------------------------------
    @property
    def dim(self) -> int:
        return 1 << self.n

    @property
    def state_shape(self) -> tuple[int, ...]:
        if self.mode == RYD_MESOLVE:
            return (self.batch, self.dim, self.dim)
        return (self.batch, self.dim)

    def _stream(self) -> int:
        return int(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _check_state(self, x: Any, shape: tuple[int, ...] | None = None) -> None:
        torch = self.torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous()):
            raise TypeError("state must be a contiguous CUDA/HIP torch tensor")
        if x.dtype != torch.complex128:
            raise TypeError("state must be complex128")
        if tuple(x.shape) != (shape or self.state_shape):
            raise ValueError(
                f"Incompatible shape of state. Expected {shape or self.state_shape}, "
                f"got {tuple(x.shape)}."
            )

    def new_state(self, kets: np.ndarray | None = None) -> Any:
        """Device state from host ket(s) ``complex[B?, 2^N]``.

        Default (``kets=None``): basis vector ``2^N - 1``, every atom in local state 1.
        That is ``|g...g>`` in the ground-rydberg order ``[r, g]`` (simulation.py:498-505)
        - and only there: in the digital order ``[g, h]`` it would be ``|h...h>``, so the
        front-end (``QutipEmulator``) always passes the initial ket explicitly."""
        torch = self.torch
        if kets is None:
            psi = torch.zeros((self.batch, self.dim), dtype=torch.complex128, device=self.device)
            psi[:, -1] = 1.0
        else:
            host = np.asarray(kets, dtype=np.complex128).reshape(-1, self.dim)
            if host.shape[0] == 1 and self.batch > 1:
                # one ket for the whole batch: upload it once, replicate on the device (a batch of 256
                # 12-atom kets is 16 MB of pageable host memory otherwise: 9 ms per block of trajectories)
                one = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
                psi = one.expand(self.batch, self.dim).contiguous()
            else:
                psi = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
        if self.mode != RYD_MESOLVE:
            return psi
        rho = torch.empty(self.state_shape, dtype=torch.complex128, device=self.device)
        _lib.check(
            self.lib.ryd_ket_to_dm(self._h, psi.data_ptr(), rho.data_ptr(), self._stream())
        )
        return rho

    # -- hot path ---------------------------------------------------------
    def evolve(
        self,
        state: Any,
        t0: float,
        t1: float,
        taylor_order: int = 0,
        tol: float = 0.0,
        max_step: float = 0.0,
        max_order: int = 0,
        magnus_tol: float = 0.0,
        split_steps: int = 0,
        method: str = "auto",
    ) -> None:
        """In place: ``state <- U(t1, t0) state`` (times in us)."""
        self._check_state(state)
        opts = RydOpts(
            taylor_order=int(taylor_order),
            max_order=int(max_order),
            tol=float(tol),
            max_step=float(max_step),
            magnus_tol=float(magnus_tol),
            split_steps=int(split_steps),
            method=_method_code(method),
        )
        _lib.check(
            self.lib.ryd_evolve(
                self._h, state.data_ptr(), float(t0), float(t1), C.byref(opts), self._stream()
            )
        )
        self._split_budget_check(method, float(tol))

    def _split_budget_check(self, method: str, tol: float) -> None:
        """The split-operator controller books its local-error estimates in ``ryd_stats.reserved[0]``;
        when it could not hold the sequence budget (retries used up, nothing to roll back to) say so."""
        if not (method == "split" or (method == "auto" and self.n >= 12)):
            return  # (12 - 14 atoms may, 15+ atoms do take the split-operator path by default; quantum jumps included:
            #          a jump solve cannot roll back, so an overrun is only ever booked - and must be reported; the
            #          split-operator master equation of 12 - 14 atoms books its a-priori estimate the same way)
        est = self.stats()["reserved"][0]
        budget = 500.0 * tol if tol > 0 else 8e-8  # (host_split.hpp: kSplitTolTotal, a bound on the 2-norm of the error since round 6; the bar itself is 1e-7)
        if est > (1000.0 * tol if tol > 0 else 1e-7):
            import warnings

            warnings.warn(
                f"split-operator step-size controller: accumulated local-error estimate {est:.1e} exceeds "
                f"the budget {budget:.1e} of this solve; tighten `tol` or use method='taylor'.",
                RuntimeWarning, stacklevel=3)

    def solve(
        self,
        state: Any,
        times: Sequence[float],
        store: bool = True,
        taylor_order: int = 0,
        tol: float = 0.0,
        max_step: float = 0.0,
        max_order: int = 0,
        magnus_tol: float = 0.0,
        split_steps: int = 0,
        method: str = "auto",
        out: Any = None,
    ) -> Any:
        """Advance ``state`` in place through ``times`` (us); with ``store``
        return complex128[len(times)-1, B, dim...] = the states at times[1:]
        (``result.states[1:]`` of the reference's solver call,
        simulation.py:729-748).  With a snapshot map (:meth:`set_snapshot_map`) the states go to their
        mapped kets of a complex128[rows, dim] tensor instead - ``out`` if given (at least as many rows as the map
        reaches; rows nothing maps to are left as they are), else a new one."""
        self._check_state(state)
        t = np.ascontiguousarray(times, dtype=np.float64)
        if t.ndim != 1 or len(t) < 2:
            raise ValueError("times must hold at least two values")
        if store and self._snap_map is not None:
            slots, rows = self._snap_map
            if len(t) - 1 != slots:
                raise ValueError(f"the snapshot map has {slots} slots, these times {len(t) - 1}")
            if out is None:
                out = self.torch.empty((rows, self.dim), dtype=self.torch.complex128, device=self.device)
            elif (not isinstance(out, self.torch.Tensor) or out.dtype != self.torch.complex128 or not out.is_contiguous()
                  or out.device != self.device or out.dim() != 2 or out.shape[1] != self.dim or out.shape[0] < rows):
                raise ValueError(f"out must be a contiguous complex128 tensor [>= {rows}, {self.dim}] on {self.device}")
        elif store and out is None:
            out = self.torch.empty(
                (len(t) - 1,) + self.state_shape,
                dtype=self.torch.complex128,
                device=self.device,
            )
        elif store:
            if (not isinstance(out, self.torch.Tensor) or out.dtype != self.torch.complex128 or not out.is_contiguous()
                    or out.device != self.device or tuple(out.shape) != (len(t) - 1,) + self.state_shape):
                raise ValueError(f"out must be a contiguous complex128 tensor {(len(t) - 1,) + self.state_shape} "
                                 f"on {self.device}")
        else:
            out = None
        opts = RydOpts(
            taylor_order=int(taylor_order),
            max_order=int(max_order),
            tol=float(tol),
            max_step=float(max_step),
            magnus_tol=float(magnus_tol),
            split_steps=int(split_steps),
            method=_method_code(method),
        )
        _lib.check(
            self.lib.ryd_solve(
                self._h,
                state.data_ptr(),
                len(t),
                t.ctypes.data,
                out.data_ptr() if out is not None else None,
                C.byref(opts),
                self._stream(),
            )
        )
        self._split_budget_check(method, float(tol))
        return out

    def set_snapshot_map(self, offsets: Any) -> None:
        """``ryd_set_snapshot_map``: from now on :meth:`solve` stores batch entry b's state at ``times[i]`` to ket
        ``offsets[b, i - 1]`` of its output (int64[batch, n_slots]; -1 = not stored), so that the entries of one solve
        may ask for different evaluation times (:func:`pulser_amd.batch.solve_many`).  ``None`` removes the map.  Noiseless
        two-level ket engines only."""
        if offsets is None:
            _lib.check(self.lib.ryd_set_snapshot_map(self._h, 0, None))
            self._snap_map = None
            return
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if off.ndim != 2 or off.shape[0] != self.batch or off.shape[1] < 1:
            raise ValueError(f"offsets must be int64[{self.batch}, n_slots >= 1], got shape {off.shape}")
        if off.min() < -1:
            raise ValueError("snapshot offsets are kets (>= 0) or -1")
        _lib.check(self.lib.ryd_set_snapshot_map(self._h, int(off.shape[1]), off.ctypes.data))
        self._snap_map = (int(off.shape[1]), int(off.max()) + 1)

    def mc_solve(
        self,
        state: Any,
        times: Sequence[float],
        seeds: Sequence[int],
        store: bool = True,
        taylor_order: int = 0,
        tol: float = 0.0,
        max_step: float = 0.0,
        max_order: int = 0,
        magnus_tol: float = 0.0,
        method: str = "auto",
    ) -> Any:
        """One quantum-jump trajectory per batch entry (``qutip.mcsolve`` with
        ``ntraj=1``, simulation.py:705-735): ``seeds`` holds one uint64 per batch
        entry.  Returns the normalised kets at times[1:] like :meth:`solve`."""
        if not self.monte_carlo:
            raise RuntimeError("engine was not created with mode='mcsolve'")
        self._check_state(state)
        t = np.ascontiguousarray(times, dtype=np.float64)
        if t.ndim != 1 or len(t) < 2:
            raise ValueError("times must hold at least two values")
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.shape != (self.batch,):
            raise ValueError(f"need one seed per batch entry ({self.batch}), got {sd.shape}")
        out = None
        if store:
            out = self.torch.empty((len(t) - 1,) + self.state_shape, dtype=self.torch.complex128,
                                   device=self.device)
        opts = RydOpts(taylor_order=int(taylor_order), max_order=int(max_order), tol=float(tol),
                       max_step=float(max_step), magnus_tol=float(magnus_tol), method=_method_code(method))
        _lib.check(
            self.lib.ryd_mc_solve(
                self._h, state.data_ptr(), len(t), t.ctypes.data,
                out.data_ptr() if out is not None else None, sd.ctypes.data, C.byref(opts),
                self._stream(),
            )
        )
        self._split_budget_check(method, float(tol))
        return out

    def mc_jumps(self) -> np.ndarray:
        """Number of collapses of every trajectory of the last :meth:`mc_solve`."""
        counts = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self.lib.ryd_mc_get_jumps(self._h, counts.ctypes.data, self._stream()))
        return counts

    def set_path(self, force_generic: bool, no_tile14: bool = False,
                 force_tile14: bool = False, no_single_pass: bool = False,
                 force_single_pass: bool = False, no_ket: bool = False,
                 force_ket: bool = False, no_split: bool = False,
                 split_fixed: bool = False, split_no_loop: bool = False,
                 no_merge: bool = False, split_small_tiles: bool = False, split_s6: bool = False,
                 no_split14: bool = False, split_turns: bool = False, rows_ket: bool = False,
                 snaps_outside: bool = False, check_segments: bool = True, uniform_drive: bool = True) -> None:
        """Test/bench hook: disable the persistent small-N kernel and/or the 2^14
        register-tile kernel with the Hermitian mesolve path (the tiled
        multi-pass kernels are used instead), or force the register tiles;
        ``no_single_pass`` disables the one-launch plan of states up to 128 MiB;
        ``no_ket`` disables the register-resident ket kernel and the split-operator
        master equation built on it, ``force_ket`` uses them from 10 atoms on;
        ``no_split`` keeps the Taylor polynomial for kets of 15+ atoms, ``split_fixed``
        switches the step-size control of the split-operator path off; ``no_merge`` keeps
        every CF4 step inside one knot interval (no multi-knot steps on smooth stretches);
        ``split_small_tiles`` keeps the 2^12 tiles of the split-operator passes where 2^14 tiles are the default
        (21 - 23 atoms); ``no_split14`` keeps batches of 14-atom sequences on the polynomial
        register-resident kernel (k_ket) instead of the split-operator one (k_split14_loop);
        ``rows_ket`` keeps the row passes of the split-operator master equation on k_ket (round 3) instead of k_split_reg;
        ``split_turns`` runs them on the round-3 kernel (two LDS turns per stage) instead of k_split_reg;
        ``snaps_outside``: every evaluation time closes a run of k_split_reg (round 4) instead of a snapshot stored from
        the registers inside the run;
        ``check_segments=False``: the step-size check of k_split_reg in launches of its own (the run that ends the stretch,
        the double step, the two regular sub-steps) instead of as segments of one launch - the same kets bit for bit;
        ``uniform_drive=False``: sequences whose atoms all see one drive and one detuning (a Global channel) run the general
        kernels of k_split_reg with a coefficient record per atom instead of k_split_reg_uni with one per sequence - the
        same stages and launches, kets equal up to rounding (:meth:`uniform_launches` counts the uniform launches);
        ``split_s6`` keeps the 4th-order composition with sub-steps that end at every knot
        (round 2) where the 6th-order one with multi-knot sub-steps is the default."""
        _lib.check(self.lib.ryd_set_path(
            self._h, int(bool(force_generic)) | (2 if no_single_pass else 0)
            | (4 if no_tile14 else 0) | (8 if force_tile14 else 0)
            | (16 if force_single_pass else 0) | (32 if no_ket else 0)
            | (64 if force_ket else 0) | (128 if no_split else 0)
            | (256 if split_fixed else 0) | (512 if split_no_loop else 0)
            | (1024 if no_merge else 0) | (2048 if split_small_tiles else 0) | (8192 if split_s6 else 0)
            | (16384 if no_split14 else 0) | (32768 if split_turns else 0) | (65536 if rows_ket else 0)
            | (131072 if snaps_outside else 0) | (1048576 if check_segments else 0)
            | (2097152 if uniform_drive else 0)))

    def uniform_launches(self) -> int:
        """Launches of the uniform kernels (k_split_reg_uni, k_split_reg_seg_uni) on this engine so far."""
        n = C.c_int64(0)
        _lib.check(self.lib.ryd_split_uniform_launches(self._h, C.byref(n)))
        return int(n.value)

    def apply_generator(self, x: Any, t: float) -> Any:
        """``G(t) x`` with ``G = -iH`` (sesolve) or the Lindbladian (mesolve)."""
        self._check_state(x)
        out = self.torch.empty_like(x)
        _lib.check(
            self.lib.ryd_apply_generator(
                self._h, x.data_ptr(), out.data_ptr(), float(t), self._stream()
            )
        )
        return out

    def probabilities(self, state: Any, reverse: bool = False) -> Any:
        self._check_state(state)
        w = self.torch.empty((self.batch, self.dim), dtype=self.torch.float64, device=self.device)
        _lib.check(
            self.lib.ryd_probabilities(
                self._h, state.data_ptr(), w.data_ptr(), int(bool(reverse)), self._stream()
            )
        )
        return w

    def observe(self, state: Any, t: float, occupation: bool = True, correlation: bool = True,
                energy: bool = True, density: bool = False) -> dict[str, np.ndarray]:
        """``ryd_observe``: occupations, correlation matrix and energy moments of every batch
        entry in one device call (no per-observable launches, no H(t) materialisation).
        ``density``: ``state`` is a density matrix ``[B, D, D]`` observed with this (ket) engine's
        Hamiltonian.  Returns host arrays: ``norm2`` [B] (trace for density matrices),
        ``occupation`` [B, N], ``correlation`` [B, N, N], ``energy`` [B], ``energy2`` [B] - NOT
        normalised (divide by ``norm2``)."""
        if density and self.mode != RYD_MESOLVE:
            want = (self.batch, self.dim, self.dim)
            if (tuple(state.shape) != want or state.dtype != self.torch.complex128
                    or not state.is_contiguous() or state.device != self.device):
                raise ValueError(f"density matrix must be a contiguous complex128 tensor of shape {want} on {self.device}")
        else:
            self._check_state(state)
        n = self.n
        what = _obs_what(occupation, correlation, energy, density)
        out = self.torch.empty((self.batch, n * n + n + 3), dtype=self.torch.float64, device=self.device)
        _lib.check(self.lib.ryd_observe(self._h, state.data_ptr(), float(t), what, out.data_ptr(),
                                        self._stream()))
        return _obs_unpack(out, n)

    def observe_many(self, states: Any, times: Any, occupation: bool = True, correlation: bool = True,
                     energy: bool = True) -> dict[str, np.ndarray]:
        """``ryd_observe_many``: what ``observe`` returns, for the kets of every evaluation time of a run in one device
        call (a memset and at most three launches) and one device-to-host copy.  ``states`` is a complex128 tensor
        ``[T, B, D]`` on this engine's device, or any view of one whose last axis is contiguous: the strides of the
        first two axes are passed on, so ``dev[:, b:b + 1]`` of a snapshot tensor is observed in place.  ``times``
        [T] (us) need not be sorted or distinct.  ``B`` is this engine's batch (entry b has problem b) or anything
        when the batch is 1 (the one problem serves every entry).  Two-level Ising sesolve engines only.  Returns host
        arrays ``norm2`` [T, B], ``occupation`` [T, B, N], ``correlation`` [T, B, N, N], ``energy`` [T, B],
        ``energy2`` [T, B] - NOT normalised (divide by ``norm2``); what was not asked for is 0."""
        torch = self.torch
        n_t, n_b, stride_t, stride_b, tt = _many_args(torch, self.device, states, times, (self.dim,))
        n = self.n
        what = _obs_what(occupation, correlation, energy)
        out = torch.empty((n_t, n_b, n * n + n + 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ryd_observe_many(self._h, states.data_ptr(), n_t, n_b, stride_t, stride_b, tt.ctypes.data,
                                             what, out.data_ptr(), self._stream()))
        return _obs_unpack(out, n)

    def observe_density_many(self, states: Any, times: Any, occupation: bool = True, correlation: bool = True,
                             energy: bool = True) -> dict[str, np.ndarray]:
        """``ryd_observe_density_many``: what ``observe(..., density=True)`` returns, for the density matrices of every
        evaluation time of a master-equation run in one device call (a memset and at most three launches) and one
        device-to-host copy.  ``states`` is a complex128 tensor ``[T, B, D, D]`` (``D = 2 ** n``) on this engine's
        device, or any view of one whose last two axes are contiguous: the strides of the first two axes are passed
        on, so ``dev[:, b:b + 1]`` and ``dev[i0:i1:step]`` of a snapshot tensor are observed in place.  ``times`` [T]
        (us) need not be sorted or distinct.  ``B`` is this engine's batch (entry b has problem b) or anything when the
        batch is 1.  Two-level Ising engines in sesolve mode (the Hamiltonian is this engine's, as with ``density=True``)
        or mesolve mode, without quantum jumps and extra detuning terms.  Returns host arrays ``norm2`` [T, B] (the
        trace), ``occupation`` [T, B, N], ``correlation`` [T, B, N, N], ``energy`` [T, B], ``energy2`` [T, B] - NOT
        normalised (divide by ``norm2``); what was not asked for is 0."""
        torch = self.torch
        d = 1 << self.n
        n_t, n_b, stride_t, stride_b, tt = _many_args(torch, self.device, states, times, (d, d))
        n = self.n
        what = _obs_what(occupation, correlation, energy)
        out = torch.empty((n_t, n_b, n * n + n + 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ryd_observe_density_many(self._h, states.data_ptr(), n_t, n_b, stride_t, stride_b,
                                                     tt.ctypes.data, what, out.data_ptr(), self._stream()))
        return _obs_unpack(out, n)

    def occupations(self, state: Any) -> Any:
        """float64[B, N+1]: <n_k> and, last, the squared norm / trace."""
        self._check_state(state)
        out = self.torch.empty((self.batch, self.n + 1), dtype=self.torch.float64, device=self.device)
        _lib.check(
            self.lib.ryd_occupations(self._h, state.data_ptr(), out.data_ptr(), self._stream())
        )
        return out

    def outer_accumulate(self, psi: Any, acc: Any, weights: np.ndarray | None = None) -> None:
        self._check_state(psi, (self.batch, self.dim))
        self._check_state(acc, (self.dim, self.dim))
        wptr = None
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            assert weights.shape == (self.batch,)
            wptr = weights.ctypes.data
        _lib.check(
            self.lib.ryd_outer_accumulate(
                self._h, psi.data_ptr(), wptr, acc.data_ptr(), self._stream()
            )
        )

    # -- introspection ----------------------------------------------------
    def stats(self) -> dict[str, Any]:
        s = RydStats()
        _lib.check(self.lib.ryd_get_stats(self._h, C.byref(s)))
        return {
            "n_applications": int(s.n_applications),
            "n_launches": int(s.n_launches),
            "n_steps": int(s.n_steps),
            "passes": int(s.passes),
            "last_order": int(s.last_order),
            "norm_bound": float(s.norm_bound),
            # split-operator path: accumulated local-error estimate of the last solve, last
            # measured local error, its sub-step (us), checkpoint restores
            "reserved": [float(v) for v in s.reserved],
        }

    def reset_stats(self) -> None:
        _lib.check(self.lib.ryd_reset_stats(self._h))

    def set_kernel_timing(self, enable: bool) -> None:
        _lib.check(self.lib.ryd_set_kernel_timing(self._h, int(bool(enable))))

    def kernel_timing(self) -> tuple[float, int]:
        ms = C.c_double()
        n = C.c_int64()
        _lib.check(self.lib.ryd_get_kernel_timing(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)


def _general_opts(opts: Mapping[str, Any]) -> RydOpts:
    return RydOpts(taylor_order=int(opts.get("taylor_order", 0)), max_order=int(opts.get("max_order", 0)),
                   tol=float(opts.get("tol", 0.0)), max_step=float(opts.get("max_step", 0.0)),
                   magnus_tol=float(opts.get("magnus_tol", 0.0)))


MAX_COLLAPSE_OPS = 16  # MC_MAX_OPS of the library
MAX_COLLAPSE_DIM = 4   # MCG_MAX_D: local dimensions of the general jump kernels


def check_collapse_args(local_dim: int, n_atoms: int, ops: Sequence[np.ndarray], dim: int,
                        is_density: bool) -> np.ndarray:
    """What ``ryd_general_set_collapse`` accepts, checked before the call: the operators as one
    complex128[n_ops, d, d] array."""
    if not 2 <= int(local_dim) <= MAX_COLLAPSE_DIM:
        raise ValueError(f"quantum jumps on the general path take local dimensions 2 - {MAX_COLLAPSE_DIM}, "
                         f"got {local_dim}")
    if is_density:
        raise ValueError("collapse operators need a ket engine (lower_general(..., mesolve=False))")
    if int(local_dim) ** int(n_atoms) != int(dim):
        raise ValueError(f"dim {dim} is not {local_dim}^{n_atoms}")
    m = np.ascontiguousarray(np.asarray(ops, dtype=np.complex128).reshape(-1, local_dim, local_dim)) \
        if len(ops) else np.zeros((0, local_dim, local_dim), dtype=np.complex128)
    if len(m) > MAX_COLLAPSE_OPS:
        raise ValueError(f"at most {MAX_COLLAPSE_OPS} local collapse operators, got {len(m)}")
    return m


class GeneralEngine:
    """Explicit-term engine for the systems the tuned kernels do not cover
    (multi-level bases, leakage, XY, arbitrary eff_noise); see
    ``pulser_amd.general``.  One problem per engine; ``batch`` > 1 holds several kets of it (quantum-jump
    trajectories of one Hamiltonian: :meth:`mc_solve`)."""

    def __init__(self, tables: Any, device: int | None = None, batch: int = 1) -> None:
        from ._lib import RydGeneralConfig

        self.torch = _torch()
        self.lib = _lib.load()
        self.tables = tables
        self.dim = int(tables.dim)
        self.local_dim = int(tables.local_dim)
        self.n = int(tables.n_qudits)
        self.is_density = bool(tables.is_density)
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be at least 1, got {batch}")
        self.n_collapse = 0
        self.device_index = self.torch.cuda.current_device() if device is None else int(device)
        self.device = self.torch.device("cuda", self.device_index)
        cfg = RydGeneralConfig(abi_version=_lib.RYD_ABI_VERSION, batch=self.batch, device=self.device_index,
                               reserved=RYD_GENERAL_DENSITY if self.is_density else 0, dim=self.dim)
        self._h = C.c_void_p()
        _lib.check(self.lib.ryd_general_create(C.byref(cfg), C.byref(self._h)))
        tk = np.ascontiguousarray(tables.tknots, dtype=np.float64)
        pp = np.ascontiguousarray(tables.pp, dtype=np.complex128)
        _lib.check(self.lib.ryd_set_series(self._h, pp.shape[0], len(tk), tk.ctypes.data,
                                           pp.ctypes.data))
        for i in range(len(tables.values)):
            free = tables.free[i] if getattr(tables, "free", None) is not None else None
            tail = (int(tables.series[i]), int(tables.conj[i]), float(tables.scale[i].real),
                    float(tables.scale[i].imag), float(tables.row_norm[i]))
            if free is not None and free[0] == "diag":
                v = np.ascontiguousarray(free[1], dtype=np.complex128)
                _lib.check(self.lib.ryd_general_add_diag_term(self._h, v.ctypes.data, *tail))
                continue
            if free is not None:
                _, d, p, st, w, rr, cc, vals = free
                st = np.ascontiguousarray(st, dtype=np.int64)
                w = np.ascontiguousarray(w, dtype=np.float64)
                rr = np.ascontiguousarray(rr, dtype=np.int32)
                cc = np.ascontiguousarray(cc, dtype=np.int32)
                vals = np.ascontiguousarray(vals, dtype=np.complex128)
                _lib.check(self.lib.ryd_general_add_local_term(
                    self._h, int(d), int(p), len(w), st.ctypes.data, w.ctypes.data, len(vals), rr.ctypes.data,
                    cc.ctypes.data, vals.ctypes.data, *tail))
                continue
            rp, ci, va = tables.row_ptr[i], tables.col_idx[i], tables.values[i]
            _lib.check(self.lib.ryd_general_add_term(
                self._h, len(va), rp.ctypes.data, ci.ctypes.data if len(va) else None,
                va.ctypes.data if len(va) else None, int(tables.series[i]), int(tables.conj[i]),
                float(tables.scale[i].real), float(tables.scale[i].imag), float(tables.row_norm[i])))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ryd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "GeneralEngine":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()

    def _stream(self) -> int:
        return int(self.torch.cuda.current_stream(self.device).cuda_stream)

    def new_state(self, ket: np.ndarray) -> Any:
        """Device vector from a host ket: psi, or row-major vec(|psi><psi|)."""
        v = np.asarray(ket, dtype=np.complex128).reshape(-1)
        if self.is_density:
            v = np.outer(v, v.conj()).reshape(-1)
        if v.size != self.dim:
            raise ValueError(f"Incompatible shape of state. Expected {self.dim}, got {v.size}.")
        v = np.repeat(v[None, :], self.batch, axis=0)
        return self.torch.from_numpy(v).to(self.device)

    def solve(self, state: Any, times: Sequence[float], **opts: Any) -> Any:
        t = np.ascontiguousarray(times, dtype=np.float64)
        out = self.torch.empty((len(t) - 1, self.batch, self.dim), dtype=self.torch.complex128,
                               device=self.device)
        o = RydOpts(taylor_order=int(opts.get("taylor_order", 0)), max_order=int(opts.get("max_order", 0)),
                    tol=float(opts.get("tol", 0.0)), max_step=float(opts.get("max_step", 0.0)),
                    magnus_tol=float(opts.get("magnus_tol", 0.0)))
        _lib.check(self.lib.ryd_solve(self._h, state.data_ptr(), len(t), t.ctypes.data,
                                      out.data_ptr(), C.byref(o), self._stream()))
        return out

    @staticmethod
    def solve_many(engines: Sequence["GeneralEngine"], states: Sequence[Any], times: Sequence[float],
                   **opts: Any) -> list[Any]:
        """Advance ``states[b]`` (in place) of every engine through ``times`` in ONE launch
        (``ryd_general_solve_many``: one workgroup per problem, vectors of at most 4096 entries) and return
        the snapshots complex128[len(times) - 1, 1, dim_b] per engine - the noise trajectories of a
        multi-level run (simulation.py:903-915)."""
        if not engines:
            return []
        e0 = engines[0]
        t = np.ascontiguousarray(times, dtype=np.float64)
        outs = [e.torch.empty((len(t) - 1, 1, e.dim), dtype=e.torch.complex128, device=e.device) for e in engines]
        n = len(engines)
        hs = (C.c_void_p * n)(*[e._h for e in engines])
        sp = (C.c_void_p * n)(*[s.data_ptr() for s in states])
        op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        o = RydOpts(taylor_order=int(opts.get("taylor_order", 0)), max_order=int(opts.get("max_order", 0)),
                    tol=float(opts.get("tol", 0.0)), max_step=float(opts.get("max_step", 0.0)),
                    magnus_tol=float(opts.get("magnus_tol", 0.0)))
        _lib.check(e0.lib.ryd_general_solve_many(hs, n, sp, len(t), t.ctypes.data, op, C.byref(o), e0._stream()))
        return outs

    # -- quantum-jump trajectories (ryd_general_set_collapse / ryd_general_mc_solve) --------------------------------
    def set_collapse(self, ops: Sequence[np.ndarray]) -> None:
        """Place the local d x d collapse operators ``ops`` on every atom (``lower_general(..., with_collapse=True)``
        gives them in the reference's order): from then on :meth:`solve` integrates the no-jump evolution under
        H_eff = H - (i/2) sum C^dag C and :meth:`mc_solve` runs jump trajectories; ``[]`` removes them."""
        m = check_collapse_args(self.local_dim, self.n, ops, self.dim, self.is_density)
        _lib.check(self.lib.ryd_general_set_collapse(self._h, self.local_dim, self.n, len(m),
                                                     m.ctypes.data if len(m) else None))
        self.n_collapse = len(m)

    def _check_batch_state(self, x: Any, rows: int) -> None:
        # the C side trusts the pointer: a mis-sized vector would read / write out of bounds
        if (tuple(x.shape) != (rows, self.dim) or x.dtype != self.torch.complex128
                or not x.is_contiguous() or x.device != self.device):
            raise ValueError(f"state must be a contiguous complex128 tensor of shape ({rows}, {self.dim}) "
                             f"on {self.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")

    def mc_solve(self, state: Any, times: Sequence[float], seeds: Sequence[int], **opts: Any) -> Any:
        """One quantum-jump trajectory per batch entry (``ryd_general_mc_solve``; the jump rule of
        ``Engine.mc_solve``): advances ``state`` [batch, dim] in place and returns the normalised kets
        complex128[len(times) - 1, batch, dim] at times[1:]."""
        if self.n_collapse == 0:
            raise RuntimeError("set_collapse has not been called")
        self._check_batch_state(state, self.batch)
        t = np.ascontiguousarray(times, dtype=np.float64)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.shape != (self.batch,):
            raise ValueError(f"need one seed per batch entry ({self.batch}), got {sd.shape}")
        out = self.torch.empty((len(t) - 1, self.batch, self.dim), dtype=self.torch.complex128, device=self.device)
        _lib.check(self.lib.ryd_general_mc_solve(self._h, state.data_ptr(), len(t), t.ctypes.data, out.data_ptr(),
                                                 sd.ctypes.data, C.byref(_general_opts(opts)), self._stream()))
        return out

    @staticmethod
    def mc_solve_many(engines: Sequence["GeneralEngine"], states: Sequence[Any], times: Sequence[float],
                      seeds: Sequence[int], **opts: Any) -> list[Any]:
        """One jump trajectory of every engine (batch 1, at most 4096 entries, :meth:`set_collapse` called) in ONE
        launch (``ryd_general_mc_solve_many``), seed ``seeds[b]`` for engine b: the noise trajectories of a
        multi-level / XY run under ``qutip.mcsolve``.  Returns the normalised kets per engine like :meth:`solve_many`."""
        if not engines:
            return []
        e0 = engines[0]
        for e, s in zip(engines, states):
            if e.batch != 1 or e.n_collapse == 0:
                raise ValueError("mc_solve_many takes engines of batch 1 with collapse operators")
            e._check_batch_state(s, 1)
        n = len(engines)
        if len(states) != n:
            raise ValueError(f"need one state per engine ({n}), got {len(states)}")
        t = np.ascontiguousarray(times, dtype=np.float64)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.shape != (n,):
            raise ValueError(f"need one seed per engine ({n}), got {sd.shape}")
        outs = [e.torch.empty((len(t) - 1, 1, e.dim), dtype=e.torch.complex128, device=e.device) for e in engines]
        hs = (C.c_void_p * n)(*[e._h for e in engines])
        sp = (C.c_void_p * n)(*[s.data_ptr() for s in states])
        op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        _lib.check(e0.lib.ryd_general_mc_solve_many(hs, n, sp, len(t), t.ctypes.data, op, sd.ctypes.data,
                                                    C.byref(_general_opts(opts)), e0._stream()))
        return outs

    def mc_jumps(self) -> np.ndarray:
        """Number of collapses of every trajectory of the last :meth:`mc_solve` / :meth:`mc_solve_many`."""
        counts = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self.lib.ryd_mc_get_jumps(self._h, counts.ctypes.data, self._stream()))
        return counts

    def apply_generator(self, x: Any, t: float) -> Any:
        """``G(t) x`` for one vector ``(1, dim)`` or one per batch entry ``(batch, dim)``."""
        # the C side trusts the pointer and launches the handle's batch: the output is sized for it
        if tuple(x.shape) not in ((1, self.dim), (self.batch, self.dim)):
            raise ValueError(f"state must be a contiguous complex128 tensor of shape (1, {self.dim}) or "
                             f"({self.batch}, {self.dim}) on {self.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        rows = int(x.shape[0])
        self._check_batch_state(x, rows)
        if rows == self.batch:
            out = self.torch.empty_like(x)
            _lib.check(self.lib.ryd_apply_generator(self._h, x.data_ptr(), out.data_ptr(), float(t), self._stream()))
            return out
        # one vector on a batched handle: padded to the batch, the first row is the answer
        xin = x.expand(self.batch, self.dim).contiguous()
        out = self.torch.empty_like(xin)
        _lib.check(self.lib.ryd_apply_generator(self._h, xin.data_ptr(), out.data_ptr(), float(t), self._stream()))
        return out[:1].contiguous()

    def observe(self, state: Any, t: float, one: int = 0, occupation: bool = True, correlation: bool = True,
                energy: bool = True, density: bool = False) -> dict[str, np.ndarray]:
        """``ryd_general_observe``: occupations and correlation matrix of ``n_k = |one><one|_k`` (``one``: index of the
        eigenstate, digit value) and the energy moments of every batch entry in one device call.  ``state``:
        ``[batch, dim]`` (kets, or ``vec(rho)`` on a density engine); ``density``: this ket engine observes density
        matrices ``[batch, dim, dim]`` with its Hamiltonian.  Returns the host arrays of :meth:`Engine.observe`:
        ``norm2`` [B] (trace for density states), ``occupation`` [B, N], ``correlation`` [B, N, N], ``energy`` [B],
        ``energy2`` [B] - NOT normalised (divide by ``norm2``)."""
        one = int(one)
        if not 0 <= one < self.local_dim:
            raise ValueError(f"'one' must be a digit in [0, {self.local_dim}), got {one}")
        if not 2 <= self.local_dim <= 4:
            raise ValueError(f"observe takes local dimensions 2 - 4, got {self.local_dim}")
        if density and self.is_density:
            raise ValueError("density=True is for ket engines; a density engine observes vec(rho) as it is")
        n = self.n
        side = self.local_dim ** n
        if side ** (2 if self.is_density else 1) != self.dim:
            raise ValueError(f"dim {self.dim} is not {self.local_dim}^{n}" + (" squared" if self.is_density else ""))
        if density:
            want = (self.batch, self.dim, self.dim)
            if (tuple(state.shape) != want or state.dtype != self.torch.complex128
                    or not state.is_contiguous() or state.device != self.device):
                raise ValueError(f"density matrix must be a contiguous complex128 tensor of shape {want} on "
                                 f"{self.device}, got {tuple(state.shape)} {state.dtype} on {state.device}")
        else:
            self._check_batch_state(state, self.batch)
        what = _obs_what(occupation, correlation, energy, density)
        out = self.torch.empty((self.batch, n * n + n + 3), dtype=self.torch.float64, device=self.device)
        _lib.check(self.lib.ryd_general_observe(self._h, state.data_ptr(), float(t), what, self.local_dim, n, one,
                                                out.data_ptr(), self._stream()))
        return _obs_unpack(out, n)

    def observe_many(self, states: Any, times: Any, one: int = 0, occupation: bool = True, correlation: bool = True,
                     energy: bool = True) -> dict[str, np.ndarray]:
        """``ryd_general_observe_many``: what :meth:`observe` returns, for the kets of every evaluation time of a run in
        one device call (a memset and at most three launches) and one device-to-host copy.  ``states`` is a complex128
        tensor ``[T, B, dim]`` on this engine's device, or any view of one whose last axis is contiguous: the strides of
        the first two axes are passed on, so ``dev[:, b:b + 1]`` of a snapshot tensor is observed in place.  ``times``
        [T] (us) need not be sorted or distinct.  ``B`` is anything: the engine's one problem serves every entry.  Ket
        engines only; the energy moments need the padded-table application (:meth:`apply_path` ``fused`` /
        ``fused_lds``) and an engine without collapse operators - :meth:`observe` serves the rest, one time per call.
        Returns host arrays ``norm2`` [T, B], ``occupation`` [T, B, N], ``correlation`` [T, B, N, N], ``energy``
        [T, B], ``energy2`` [T, B] - NOT normalised (divide by ``norm2``); what was not asked for is 0."""
        torch = self.torch
        one = int(one)
        if not 0 <= one < self.local_dim:
            raise ValueError(f"'one' must be a digit in [0, {self.local_dim}), got {one}")
        if not 2 <= self.local_dim <= 4:
            raise ValueError(f"observe_many takes local dimensions 2 - 4, got {self.local_dim}")
        n_t, n_b, stride_t, stride_b, tt = _many_args(torch, self.device, states, times, (self.dim,))
        n = self.n
        what = _obs_what(occupation, correlation, energy)
        out = torch.empty((n_t, n_b, n * n + n + 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ryd_general_observe_many(self._h, states.data_ptr(), n_t, n_b, stride_t, stride_b,
                                                     tt.ctypes.data, what, self.local_dim, n, one, out.data_ptr(),
                                                     self._stream()))
        return _obs_unpack(out, n)

    def observe_density_many(self, states: Any, times: Any, one: int = 0, occupation: bool = True,
                             correlation: bool = True, energy: bool = True) -> dict[str, np.ndarray]:
        """``ryd_general_observe_density_many``: what :meth:`observe` with ``density=True`` returns, for the density
        matrices of every evaluation time of a master-equation run in one device call and one device-to-host copy.
        ``states`` is a complex128 tensor ``[T, B, dim, dim]`` on this engine's device, or any view of one whose last
        two axes are contiguous: the strides of the first two axes are passed on, so ``dev[:, b:b + 1]`` of a snapshot
        tensor is observed in place.  ``times`` [T] (us) need not be sorted or distinct; ``B`` is anything.  Ket engines
        only (H(t) is this engine's); the energy moments need :meth:`apply_path` ``fused`` / ``fused_lds`` and an engine
        without collapse operators.  The matrices are read as stored (not assumed Hermitian), the real part is kept.
        Returns host arrays ``norm2`` [T, B] (the trace), ``occupation`` [T, B, N], ``correlation`` [T, B, N, N],
        ``energy`` [T, B], ``energy2`` [T, B] - NOT normalised (divide by ``norm2``); what was not asked for is 0."""
        torch = self.torch
        one = int(one)
        if not 0 <= one < self.local_dim:
            raise ValueError(f"'one' must be a digit in [0, {self.local_dim}), got {one}")
        if not 2 <= self.local_dim <= 4:
            raise ValueError(f"observe_density_many takes local dimensions 2 - 4, got {self.local_dim}")
        if self.is_density:
            raise ValueError("observe_density_many is for ket engines; a density engine observes vec(rho) with observe")
        n_t, n_b, stride_t, stride_b, tt = _many_args(torch, self.device, states, times, (self.dim, self.dim))
        n = self.n
        what = _obs_what(occupation, correlation, energy)
        out = torch.empty((n_t, n_b, n * n + n + 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ryd_general_observe_density_many(self._h, states.data_ptr(), n_t, n_b, stride_t, stride_b,
                                                             tt.ctypes.data, what, self.local_dim, n, one,
                                                             out.data_ptr(), self._stream()))
        return _obs_unpack(out, n)

    def set_path(self, force_multi_launch: bool, no_sites: bool = False, no_fused: bool = False,
                 observe_small_chunks: bool = False) -> None:
        """Test hook: one launch per Taylor stage instead of the persistent
        one-launch kernel used for vectors of at most 4096 entries; ``no_sites``: the term-by-term
        kernel instead of the site-fused application of matrix-free terms; ``no_fused``: the round-3 site kernel
        (k_gen_apply_sites) instead of the padded site tables of k_gen_apply_fused; ``observe_small_chunks``:
        :meth:`observe` of density matrices takes 5 columns per chunk (the chunked path on a small state),
        :meth:`observe_many` and :meth:`observe_density_many` 5 evaluation times per chunk of tables."""
        _lib.check(self.lib.ryd_set_path(self._h, int(bool(force_multi_launch)) | (4096 if no_sites else 0)
                                         | (262144 if no_fused else 0) | (524288 if observe_small_chunks else 0)))

    def reset_stats(self) -> None:
        _lib.check(self.lib.ryd_reset_stats(self._h))

    def apply_path(self) -> str:
        """The kernel that the next application of the generator runs with (``ryd_general_apply_path``): what
        ``stats()["apply_path"]`` says after an application, known before the first one."""
        path = C.c_int32(0)
        _lib.check(self.lib.ryd_general_apply_path(self._h, C.byref(path)))
        return ("terms", "sites", "fused", "fused_lds")[path.value]

    def stats(self) -> dict[str, Any]:
        s = RydStats()
        _lib.check(self.lib.ryd_get_stats(self._h, C.byref(s)))
        return {"n_applications": int(s.n_applications), "n_launches": int(s.n_launches),
                "n_steps": int(s.n_steps), "passes": 1, "last_order": int(s.last_order),
                "norm_bound": float(s.norm_bound),
                # kernel of the last generator application (ryd_stats.reserved[3] of a general handle)
                "apply_path": ("terms", "sites", "fused", "fused_lds")[int(s.reserved[3])]}

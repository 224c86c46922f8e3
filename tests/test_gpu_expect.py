"""GPU: ``engine.expect_sparse`` (ryd_expect_sparse, k_expect_sparse) against the longdouble host reference of
tests/expect_ref.py under its derived bound (nnz + 16) u S_abs per real and imaginary part, at the kernel's edges; then
``SimulationResults.expect`` of non-diagonal observables on a run whose snapshots stay on the device.

States come from ``helpers.rand_state`` (some scaled away from norm 1); operators are random complex and
non-Hermitian unless a case says otherwise.  Every case prints error / tolerance before it asserts."""
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from expect_ref import part_errors, ref_expect, tol_expect, triplets
from helpers import load_fixture, local_problem, rand_state

pytestmark = pytest.mark.gpu

CHUNK, TILE = 2048, 8  # kExpectChunk, kExpectTile of pulser_amd/csrc/k_expect.hpp (checked below)


def _report(what, err, tol):
    """Print error / tolerance of one output (max over its elements), then say whether it holds."""
    err, tol = np.asarray(err, dtype=float), np.asarray(tol, dtype=float)
    ok = bool(np.all(err <= tol))
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0, tol, np.finfo(float).tiny))))
    print(f"RATIO k_expect_sparse  {what:44s} err {float(np.max(err)):.3e} tol {float(np.max(tol)):.3e} ratio {ratio:.3e}")
    return ok


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _operator(D, nnz, seed, rows=None):
    """Random complex operator with exactly ``nnz`` stored non-zeros (in the rows ``rows`` only, when given)."""
    rng = np.random.default_rng(seed)
    rows = np.arange(D) if rows is None else np.asarray(rows)
    flat = rng.choice(len(rows) * D, size=nnz, replace=False)
    m = sp.csr_matrix((rng.normal(size=nnz) + 1j * rng.normal(size=nnz), (rows[flat // D], flat % D)), shape=(D, D))
    assert m.nnz == nnz
    return m


def _kets(S, D, seed):
    return np.stack([(0.3 + 0.7 * s) * rand_state(D, seed + s) for s in range(S)])  # norms 0.3, 1.0, 1.7, ...


def _sigma_x_sum(n):
    sx = sp.csr_matrix(np.array([[0, 1], [1, 0]], dtype=complex))
    return sum(sp.kron(sp.kron(sp.identity(2**k), sx), sp.identity(2**(n - 1 - k))) for k in range(n)).tocsr()


def _check(what, operator, states_host, states_dev, density=False):
    from pulser_amd.engine import expect_sparse

    got = expect_sparse(states_dev, operator, density=density).cpu().numpy()
    ref, s_abs = ref_expect(operator, states_host, density=density)
    assert got.shape == (len(states_host),) and got.dtype == np.complex128
    assert _report(what, part_errors(got, ref), tol_expect(len(triplets(operator)[2]), s_abs))
    return got


def test_the_constants_of_this_file_are_the_kernels():
    src = open(os.path.join(os.path.dirname(__file__), "..", "pulser_amd", "csrc", "k_expect.hpp")).read()
    assert int(re.search(r"kExpectChunk = (\d+)", src).group(1)) == CHUNK
    assert int(re.search(r"kExpectTile = (\d+)", src).group(1)) == TILE


@pytest.mark.parametrize("D, nnz, S, edge", [
    (8, 5, 1, "fewer non-zeros than one wave"),
    (64, CHUNK, 3, "exactly one chunk"),
    (64, CHUNK + 1, 3, "a second workgroup with one term"),
    (81, 81 * 81, 2, "3^4, dense: every row longer than a wave"),
])
def test_kets_at_the_chunk_edges(D, nnz, S, edge):
    O = _operator(D, nnz, seed=D + nnz) if nnz < D * D else np.asarray(_operator(D, nnz, seed=1).toarray())
    x = _kets(S, D, seed=300 + D)
    _check(f"D={D} nnz={nnz} S={S}: {edge}", O, x, _cuda(x))


def test_a_strided_view_of_a_snapshot_tensor_and_a_partial_state_tile():
    """``dev[:, 1]`` of a [37, 3, 1024] tensor: stride(0) = 3 D, 37 = 4 tiles of 8 + 5."""
    S, B, D = 37, 3, 1024
    data = np.stack([_kets(B, D, seed=1000 + 7 * s) for s in range(S)])
    dev = _cuda(data)
    view = dev[:, 1]
    assert view.stride(0) == B * D and not view.is_contiguous() and S % TILE
    O = _operator(D, 5000, seed=9)
    _check("D=1024 S=37 dev[:, 1] of [37, 3, 1024]", O, data[:, 1], view)
    _check("D=1024 S=37 contiguous copy", O, data[:, 1], view.contiguous())


def test_empty_rows_an_empty_leading_block_and_the_empty_operator():
    from pulser_amd.engine import expect_sparse

    D, S = 1024, 5
    x = _kets(S, D, seed=77)
    rows = np.arange(512, D, 3)  # rows 0..511 hold nothing, and two of three rows after them
    O = _operator(D, 3000, seed=4, rows=rows)
    assert O[:512].nnz == 0 and np.count_nonzero(np.diff(O.indptr)) <= len(rows)
    _check("D=1024 empty rows + empty leading block", O, x, _cuda(x))
    low = x.copy()
    low[:, 512:] = 0.0  # states that live on the empty block alone: every term has a zero factor
    assert np.all(expect_sparse(_cuda(low), O).cpu().numpy() == 0)
    assert np.all(expect_sparse(_cuda(x), sp.csr_matrix((D, D), dtype=complex)).cpu().numpy() == 0)  # nnz = 0
    rho = np.stack([rand_state(64 * 64, 5 + s).reshape(64, 64) for s in range(3)])
    assert np.all(expect_sparse(_cuda(rho), sp.csr_matrix((64, 64)), density=True).cpu().numpy() == 0)
    import torch

    assert expect_sparse(torch.empty((0, D), dtype=torch.complex128, device="cuda"), O).shape == (0,)  # no launch


def test_a_hermitian_pauli_sum_is_real_and_a_diagonal_operator_is_the_weighted_norm():
    n, S = 8, 5
    D = 2**n
    x = _kets(S, D, seed=21)
    O = _sigma_x_sum(n)
    got = _check("D=256 S=5 sum sigma_x", O, x, _cuda(x))
    _, s_abs = ref_expect(O, x)
    assert _report("D=256 S=5 sum sigma_x: imaginary part", np.abs(got.imag), tol_expect(O.nnz, s_abs))
    d = np.random.default_rng(2).normal(size=D)
    got = _check("D=256 S=5 diagonal", sp.diags(d).tocsr(), x, _cuda(x))
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    w = ((xr * xr + xi * xi) * d.astype(np.longdouble))
    assert _report("D=256 S=5 diagonal against sum |x|^2 d", np.abs(got.real - w.sum(axis=1)).astype(float),
                   tol_expect(D, np.abs(w).sum(axis=1)))


def test_the_workloads_dimension_once():
    """14 atoms, sum_k sigma_x^k: 14 * 16 384 non-zeros = 112 chunks."""
    n, S = 14, 5
    x = _kets(S, 2**n, seed=1400)
    O = _sigma_x_sum(n)
    assert O.nnz == n * 2**n
    _check("D=16384 S=5 sum sigma_x", O, x, _cuda(x))


@pytest.mark.parametrize("D, strided", [(8, False), (64, True), (81, False)])
def test_density_matrices(D, strided):
    S = 3
    rho = np.stack([(0.5 + s) * rand_state(D * D, 500 + D + s).reshape(D, D) for s in range(S)])  # not Hermitian, trace != 1
    O = _operator(D, min(D * D, 3 * D + 1), seed=D)
    if strided:
        full = np.stack([rho, rho[::-1] * 2.0], axis=1)  # [S, 2, D, D]; entry 0 of every time is the case
        dev = _cuda(full)[:, 0]
        assert dev.stride(0) == 2 * D * D
    else:
        dev = _cuda(rho)
    _check(f"density D={D} S={S}{' strided' if strided else ''}", O, rho, dev, density=True)


def test_the_call_overwrites_its_output():
    """ryd_expect_sparse itself on an ``out`` pre-filled with a sentinel (the wrapper allocates its own)."""
    import torch

    from pulser_amd import _lib

    D, S = 64, 11
    x = _kets(S, D, seed=8)
    O = _operator(D, 700, seed=8)
    r, c, v = triplets(O)
    xd, rd, cd, vd = _cuda(x), _cuda(r.astype(np.int32)), _cuda(c.astype(np.int32)), _cuda(v)
    out = torch.full((S + 2,), 1e300 + 1e300j, dtype=torch.complex128, device="cuda")
    _lib.check(_lib.load().ryd_expect_sparse(xd.data_ptr(), S, D, D, 0, rd.data_ptr(), cd.data_ptr(), vd.data_ptr(), len(v),
                                             out.data_ptr() + 16, 0, torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    assert got[0] == 1e300 + 1e300j and got[-1] == 1e300 + 1e300j  # nothing outside out[0 .. S)
    ref, s_abs = ref_expect(O, x)
    assert _report("sentinel D=64 S=11", part_errors(got[1:-1], ref), tol_expect(len(v), s_abs))
    # argument errors of the C entry point: nothing is launched
    for bad in (dict(stride=D - 1), dict(dim=0), dict(n=-1), dict(nnz=-1), dict(states=0)):
        with pytest.raises(_lib.RydError):
            _lib.check(_lib.load().ryd_expect_sparse(
                bad.get("states", xd.data_ptr()), bad.get("n", S), bad.get("stride", D), bad.get("dim", D), 0, rd.data_ptr(),
                cd.data_ptr(), vd.data_ptr(), bad.get("nnz", len(v)), out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
    with pytest.raises(_lib.RydError):  # density: the stride must hold dim x dim (8 x 8 = 64 > 63)
        _lib.check(_lib.load().ryd_expect_sparse(xd.data_ptr(), 1, D - 1, 8, 1, rd.data_ptr(), cd.data_ptr(), vd.data_ptr(), 1,
                                                 out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))


def test_wrapper_errors():
    import torch

    from pulser_amd.engine import expect_sparse

    D = 16
    x = _cuda(_kets(2, D, seed=1))
    O = _operator(D, 20, seed=1)
    with pytest.raises(TypeError, match="complex128"):
        expect_sparse(x.to(torch.complex64), O)
    with pytest.raises(ValueError, match="CUDA"):
        expect_sparse(x.cpu(), O)
    with pytest.raises(ValueError, match="does not match"):
        expect_sparse(x, _operator(8, 5, seed=1))
    with pytest.raises(ValueError, match="does not match"):
        expect_sparse(x, O, density=True)  # [S, D] is not [S, D, D]
    with pytest.raises(ValueError, match="square"):
        expect_sparse(x, sp.csr_matrix((D, D + 1)))
    with pytest.raises(ValueError, match="contiguous"):
        expect_sparse(_cuda(np.zeros((2, D, 2), dtype=complex))[:, :, 0], O)
    bad = sp.csr_matrix((D, D), dtype=complex)
    bad.data, bad.indices, bad.indptr = np.ones(1, complex), np.array([D], dtype=np.int32), np.array([0] + [1] * D, dtype=np.int32)
    with pytest.raises(ValueError, match="indices outside"):
        expect_sparse(x, bad)


# -- the public interface ---------------------------------------------------------------------------------------------
def _run_full(inputs, **kw):
    from pulser_amd import QutipEmulator

    emu = QutipEmulator(inputs, evaluation_times="Full", **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return emu.run()


def _against_reference(what, values, op, host_states):
    density = host_states[0].shape[1] > 1
    ref, s_abs = ref_expect(op, [a if density else a.reshape(-1) for a in host_states], density=density)
    got = np.asarray(values).astype(complex)
    return _report(what, part_errors(got, ref), tol_expect(len(triplets(op)[2]), s_abs))


def test_results_expect_leaves_the_snapshots_on_the_device():
    from test_host_logic import _inputs_from_problem

    n = 6
    D = 2**n
    res = _run_full(_inputs_from_problem(local_problem(n, seed=6, duration=61)))
    sx = _sigma_x_sum(n)
    sp_2 = np.kron(np.kron(np.eye(4), np.array([[0, 1], [0, 0]], dtype=complex)), np.eye(8))  # sigma_+ on atom 2: dense
    proj = np.zeros((D, D))
    proj[np.arange(D // 2), np.arange(D // 2)] = 1.0  # |r><r| on atom 0: diagonal
    obs = [sx, sp_2, proj]
    states = res.states
    store = states[1]._store
    assert len(states) > 17 and store.device_tensor is not None and store.device_tensor.is_cuda
    vals = res.expect(obs)
    assert store.device_tensor is not None and all(s._q is None and s._store is store for s in states[1:])
    assert store._reads == 0
    assert [v.dtype for v in vals] == [np.float64, np.complex128, np.float64] and all(v.shape == (len(states),) for v in vals)
    host = [np.asarray(s) for s in states]  # now read everything back (the store spills on the 17th read)
    assert store.device_tensor is None
    ok = [_against_reference(f"emulator n=6 observable {k}", v, sp.csr_matrix(o), host) for k, (v, o) in enumerate(zip(vals, obs))]
    assert all(ok)
    # a spilled store takes the host formulas: the same values within the same bound
    res2 = _run_full(_inputs_from_problem(local_problem(n, seed=6, duration=61)))
    dev_vals = res2.expect(obs)
    res2.to_host()
    assert res2.states[1]._store.device_tensor is None
    host_vals = res2.expect(obs)
    host2 = [np.asarray(s) for s in res2.states]
    for k, (a, b, o) in enumerate(zip(dev_vals, host_vals, obs)):
        assert a.dtype == b.dtype
        _, s_abs = ref_expect(sp.csr_matrix(o), [h.reshape(-1) for h in host2])
        assert _report(f"emulator n=6 observable {k}: spilled store", part_errors(a, b), tol_expect(sp.csr_matrix(o).nnz, s_abs))


def test_results_expect_over_density_matrix_snapshots():
    """A mesolve run (two atoms, dephasing): the store is [times, 1, D, D] and every observable takes the kernel."""
    from dataclasses import replace

    from pulser_amd import NoiseModel
    from pulser_amd.hamiltonian_data import SequenceInputs

    inputs = replace(SequenceInputs.from_dict(load_fixture("results_noisy.npz")[0]["inputs"]), measurement="ground-rydberg")
    res = _run_full(inputs, noise_model=NoiseModel(dephasing_rate=0.01))
    states = res.states
    store = states[1]._store
    assert states[1].isoper and store.device_tensor.dim() == 4
    rng = np.random.default_rng(3)
    A = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    obs = [_sigma_x_sum(2), A, np.diag([1.0, 0.0, 0.5, 0.0])]
    vals = res.expect(obs)
    assert store.device_tensor is not None and store._reads == 0 and all(s._q is None for s in states[1:])
    assert [v.dtype for v in vals] == [np.float64, np.complex128, np.float64]
    host = [np.asarray(s) for s in states]
    assert all([_against_reference(f"mesolve 2 atoms observable {k}", v, sp.csr_matrix(o), host)
                for k, (v, o) in enumerate(zip(vals, obs))])

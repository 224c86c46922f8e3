// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_ensemble_diag: diag[i][x] += sum_b |psi(i, b)[x]|^2 - the diagonal of the trajectory-summed density matrix
// ---------------------------------------------------------------------------
// What a quantum-jump ensemble needs of rho = mean_b |psi_b><psi_b| in order to be sampled (QutipResult._weights,
// pulser_simulation/qutip_result.py:101-118, reads diag rho and nothing else): the [dim][dim] matrix is never formed.
//
// The work is reading the kets once: 16 B per amplitude and trajectory, 8 B written per (time, amplitude).  One lane
// owns ONE amplitude x of one time i and walks the trajectory axis: a wave reads 1 KiB contiguous per trajectory
// (global_load_dwordx4 per lane), the b loop is unrolled kEnsembleUnroll times with every load of a round issued
// before the first square is added, and the sum leaves as one coalesced 8-byte store.  blockIdx.x is the chunk of
// 256 amplitudes, blockIdx.y the time (times beyond 65 535 are walked with stride gridDim.y).
//
// Summation order: a lane adds its trajectories in the order b = 0, 1, ..., n_batch - 1 onto the value it found in
// diag - no atomics, no cross-lane step, nothing that depends on the launch geometry or on the unroll factor.  Two calls
// on the same input are bitwise equal.  The trajectory axis is NOT split across workgroups: n_times * dim / 256
// workgroups is what there is (512 for 32 times of a 12-atom register), and a register small enough to leave CUs idle
// has kets small enough that the call is launch latency either way (profiles/mc_ensemble.md).
// Every offset into the states is 64-bit.
constexpr int kEnsembleUnroll = 8;

__global__ __launch_bounds__(256) void k_ensemble_diag(const cplx* __restrict__ states, int n_times, int n_batch,
                                                       long long stride_t, long long stride_b, long long dim,
                                                       double* __restrict__ diag) {
  const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
  if (x >= dim) return;
  for (long long i = blockIdx.y; i < n_times; i += gridDim.y) {
    const cplx* p = states + i * stride_t + x;
    double acc = diag[i * dim + x];
    int b = 0;
    for (; b + kEnsembleUnroll <= n_batch; b += kEnsembleUnroll) {
      cplx v[kEnsembleUnroll];
#pragma unroll
      for (int k = 0; k < kEnsembleUnroll; ++k) v[k] = p[(long long)(b + k) * stride_b];
#pragma unroll
      for (int k = 0; k < kEnsembleUnroll; ++k) acc += v[k].x * v[k].x + v[k].y * v[k].y;
    }
    for (; b < n_batch; ++b) {
      const cplx v = p[(long long)b * stride_b];
      acc += v.x * v.x + v.y * v.y;
    }
    diag[i * dim + x] = acc;
  }
}

extern "C" int ryd_ensemble_diag(const void* states_dev, int32_t n_times, int32_t n_batch, int64_t stride_t,
                                 int64_t stride_b, int64_t dim, double* diag_dev, int32_t device, void* stream) {
  if (n_times < 0) return fail(RYD_ERR_INVALID, "ensemble_diag: n_times %d is negative", (int)n_times);
  if (n_batch < 1) return fail(RYD_ERR_INVALID, "ensemble_diag: n_batch %d is smaller than 1", (int)n_batch);
  if (dim < 1) return fail(RYD_ERR_INVALID, "ensemble_diag: dim %lld is smaller than 1", (long long)dim);
  if (stride_t < dim || stride_b < dim)
    return fail(RYD_ERR_INVALID, "ensemble_diag: strides %lld / %lld are smaller than a ket of dim %lld",
                (long long)stride_t, (long long)stride_b, (long long)dim);
  if (!states_dev) return fail(RYD_ERR_INVALID, "ensemble_diag: states_dev is null");
  if (!diag_dev) return fail(RYD_ERR_INVALID, "ensemble_diag: diag_dev is null");
  if (n_times == 0) return RYD_OK;
  const int64_t n_chunks = (dim + 255) / 256;
  if (n_chunks > INT32_MAX) return fail(RYD_ERR_INVALID, "ensemble_diag: dim %lld is too large", (long long)dim);
  HIPCHK(hipSetDevice(device));
  const dim3 grid((unsigned)n_chunks, (unsigned)std::min<int32_t>(n_times, 65535));
  hipLaunchKernelGGL(k_ensemble_diag, grid, dim3(256), 0, (hipStream_t)stream, (const cplx*)states_dev, (int)n_times,
                     (int)n_batch, (long long)stride_t, (long long)stride_b, (long long)dim, diag_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_ensemble_diag: %s", hipGetErrorString(e));
  return RYD_OK;
}

// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_general_observe: the V2 observables of one state of a d-level register (3-level "all" basis, leakage, XY mode)
// in one call, on the device - the siblings of k_observe.hpp for the general path.
// ---------------------------------------------------------------------------
// Occupations <n_k>, correlations <n_k n_l> with n_k = |one><one|_k (default_observables.py:291-435) and the energy
// moments <H>, <H^2> (:437-580).  Kets: one generator application w = -i H x and the fused dot k_obs_energy.
// Density matrices on a ket handle: the COLUMNS of rho are staged as a batch of vectors X (tiled transpose: rows of rho
// are contiguous, columns are not, and sum_ab H_ab rho_ab would be Tr(H^T rho)), W = -i H X and W2 = -i H W = -H^2 X are
// one batched launch each, and
//     Tr(H rho) = -Im sum_c W[c][c],      Tr(H^2 rho) = -Re sum_c W2[c][c].
// rho is read as stored (no Hermitian symmetry is assumed) and the real part of either trace is kept, as k_obs_energy_dm
// does for two-level registers.

// Bit k of the word: digit k (atom k, stride d^(N-1-k)) of `idx` equals `one`.  d = 2 / 4: shifts; d = 3: the quotient by
// the multiply-shift (idx * 0xAAAAAAAB) >> 33, exact for every 32-bit idx.
__device__ __forceinline__ unsigned gen_obs_word(unsigned idx, int d, int N, unsigned one) {
  unsigned w = 0;
  for (int p = 0; p < N; ++p) {  // least significant digit first: atom N - 1 - p
    unsigned q, a;
    if (d == 2) { q = idx >> 1; a = idx & 1u; }
    else if (d == 4) { q = idx >> 2; a = idx & 3u; }
    else { q = __umulhi(idx, 0xAAAAAAABu) >> 1; a = idx - 3u * q; }
    w |= (unsigned)(a == one) << (N - 1 - p);
    idx = q;
  }
  return w;
}

// out[s] = the row of k_obs_pairs for state s = it * n_batch + b at states + it * stride_t + b * stride_b (64-bit
// offsets), the states taken from the second grid axis with a stride (it is capped at 65 535 workgroups), exactly as
// k_obs_pairs addresses them: ryd_general_observe passes n_states = n_batch = its batch, ryd_general_observe_many every
// evaluation time of a run.  One block stages a chunk of probabilities in LDS and, beside each, the digit word of its
// index (computed once per block: it does not depend on the state), then takes the pair sums of k_observe.hpp on the words.
// is_dm: a state is [D][D] (a density matrix, or vec(rho) of a RYD_GENERAL_DENSITY handle; stride_b = D * D) and
// p_i = Re rho_ii.  N <= 26 (d^N <= 2^26).
__global__ __launch_bounds__(256) void k_gen_obs_pairs(const cplx* __restrict__ states, long long n_states, int n_batch,
                                                       long long stride_t, long long stride_b, unsigned D, int N, int d,
                                                       int one, int is_dm, int what, double* __restrict__ out,
                                                       int out_stride) {
  __shared__ double ps[kObsCH];
  __shared__ unsigned wd[kObsCH];
  const size_t base = (size_t)blockIdx.x * kObsCH;
  for (int i = threadIdx.x; i < kObsCH; i += blockDim.x) {
    const size_t g = base + i;
    wd[i] = g < D ? gen_obs_word((unsigned)g, d, N, (unsigned)one) : 0u;
  }
  for (long long s = blockIdx.y; s < n_states; s += gridDim.y) {
    const long long it = s / n_batch, b = s - it * n_batch;
    const cplx* __restrict__ sb = states + it * stride_t + b * stride_b;
    for (int i = threadIdx.x; i < kObsCH; i += blockDim.x) {
      const size_t g = base + i;
      double p = 0.0;
      if (g < D) {
        if (is_dm) p = sb[g * D + g].x;
        else { const cplx v = sb[g]; p = v.x * v.x + v.y * v.y; }
      }
      ps[i] = p;
    }
    __syncthreads();
    obs_pair_sums<true>(ps, wd, base, N, what, out + (size_t)s * out_stride);
    __syncthreads();  // `ps` is filled again for the next state of this workgroup
  }
}

// X[b * nc + j][a] = rho[b][a][c0 + j] for j < nc: columns c0 .. c0 + nc of every D x D matrix as contiguous vectors,
// 32 x 32 tiles through LDS (k_transpose_conj without the conjugate, any D).  grid (ceil(nc / 32), ceil(D / 32), batch).
__global__ __launch_bounds__(256) void k_gen_obs_stage_cols(const cplx* __restrict__ rho, cplx* __restrict__ X, unsigned D,
                                                            unsigned c0, unsigned nc) {
  __shared__ cplx t[32][33];
  const size_t b = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const unsigned j0 = blockIdx.x * 32, a0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned a = a0 + ty + 8 * r, j = j0 + tx;
    t[ty + 8 * r][tx] = (a < D && j < nc) ? rho[(b * D + a) * D + c0 + j] : make_double2(0.0, 0.0);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned j = j0 + ty + 8 * r, a = a0 + tx;
    if (j < nc && a < D) X[(b * nc + j) * D + a] = t[tx][ty + 8 * r];
  }
}

// Entry c0 + j of vector b * nc + j, summed over j < nc: the part of a trace that the columns c0 .. c0 + nc carry.
// second = 0: o[off] += -Im (W = -i H X: Re Tr(H rho)); second = 1: o[off + 1] += -Re (W2 = -H^2 X: Re Tr(H^2 rho)).
__global__ __launch_bounds__(256) void k_gen_obs_trace(const cplx* __restrict__ W, unsigned D, unsigned c0, unsigned nc,
                                                       int second, double* __restrict__ out, int out_stride, int off) {
  const size_t b = blockIdx.y;
  double e = 0.0;
  for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < nc; j += gridDim.x * 256) {
    const cplx v = W[(b * nc + j) * D + c0 + j];
    e -= second ? v.x : v.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out + b * out_stride + off + second, e);
}

// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_general_observe: the V2 observables of one state of a d-level register (3-level "all" basis, leakage, XY mode)
// in one call, on the device - the siblings of k_observe.hpp for the general path.
// ---------------------------------------------------------------------------
// Occupations <n_k>, correlations <n_k n_l> with n_k = |one><one|_k (default_observables.py:291-435) and the energy
// moments <H>, <H^2> (:437-580).  Kets: one generator application w = -i H x and one fused dot, as k_obs_energy.
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

// out[b][0..N-1] = <n_k>, out[b][N] = sum p, out[b][N+1 + k*N + l] = <n_k n_l> (the layout of k_obs_pairs).
// One block stages a chunk of probabilities in LDS and, beside each, the digit word of its index (computed once per
// element); thread <-> (k, l) pair; wave-uniform chunk index -> LDS broadcast reads; one atomic per pair and block.
// is_dm: `st` is [batch][D][D] (a density matrix, or vec(rho) of a RYD_GENERAL_DENSITY handle) and p_i = Re rho_ii.
// `what`: RYD_OBS_OCCUPATION and / or RYD_OBS_CORRELATION - the slots of the one not asked for stay 0 (the norm is
// written with either).  N <= 26 (d^N <= 2^26).
__global__ __launch_bounds__(256) void k_gen_obs_pairs(const cplx* __restrict__ st, unsigned D, int N, int d, int one,
                                                       int is_dm, int what, double* __restrict__ out, int out_stride) {
  constexpr int CH = 2048;
  __shared__ double ps[CH];
  __shared__ unsigned wd[CH];
  const int b = blockIdx.y;
  const int npair = N * (N + 1) / 2;
  const size_t base = (size_t)blockIdx.x * CH;
  const cplx* __restrict__ sb = st + (size_t)b * D * (is_dm ? (size_t)D : 1);
  for (int i = threadIdx.x; i < CH; i += blockDim.x) {
    const size_t g = base + i;
    double p = 0.0;
    unsigned w = 0;
    if (g < D) {
      if (is_dm) p = sb[g * D + g].x;
      else { const cplx v = sb[g]; p = v.x * v.x + v.y * v.y; }
      w = gen_obs_word((unsigned)g, d, N, (unsigned)one);
    }
    ps[i] = p;
    wd[i] = w;
  }
  __syncthreads();
  double* o = out + (size_t)b * out_stride;
  for (int pr = threadIdx.x; pr <= npair; pr += blockDim.x) {
    if (pr == npair) {  // the norm
      double s = 0.0;
      for (int i = 0; i < CH; ++i) s += ps[i];
      atomicAdd(o + N, s);
      continue;
    }
    // pair index -> (k <= l)
    int k = 0, rem = pr;
    while (rem >= N - k) { rem -= N - k; ++k; }
    const int l = k + rem;
    if (k != l && !(what & RYD_OBS_CORRELATION)) continue;
    const unsigned m = (1u << k) | (1u << l);
    double s = 0.0;
    for (int i = 0; i < CH; ++i)
      if ((wd[i] & m) == m) s += ps[i];
    if (k == l && (what & RYD_OBS_OCCUPATION)) atomicAdd(o + k, s);
    if (!(what & RYD_OBS_CORRELATION)) continue;
    atomicAdd(o + N + 1 + k * N + l, s);
    if (k != l) atomicAdd(o + N + 1 + l * N + k, s);
  }
}

// o[0] += -Im <x|w>, o[1] += |w|^2 over vectors of any length D (3^N): wave64 shuffles, one atomic pair per wave.
__global__ __launch_bounds__(256) void k_gen_obs_energy(const cplx* __restrict__ x, const cplx* __restrict__ w, size_t D,
                                                        double* __restrict__ out, int out_stride, int off) {
  const size_t boff = (size_t)blockIdx.y * D;
  double e = 0.0, e2 = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < D; i += (size_t)gridDim.x * 256) {
    const cplx a = x[boff + i], c = w[boff + i];
    e -= a.x * c.y - a.y * c.x;
    e2 = fma(c.x, c.x, fma(c.y, c.y, e2));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { e += __shfl_down(e, o, 64); e2 += __shfl_down(e2, o, 64); }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out + (size_t)blockIdx.y * out_stride + off, e);
    atomicAdd(out + (size_t)blockIdx.y * out_stride + off + 1, e2);
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

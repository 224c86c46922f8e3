// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_overlap_many: <a_f|x_s>, <phi_f|rho_s|phi_f> or Tr(A_f^dag rho_s), and the norm or trace of every stored state
// ---------------------------------------------------------------------------
// Replaces the loop of Fidelity.apply over the evaluation times (QutipState.overlap, qutip_state.py:86-110) for the
// states that are still device snapshots, and brings the number Fidelity and Expectation divide by.
//
//   z[s][f] = sum_e w_f[e] x_s[e]      e over the `len` stored elements of a state (dim, or dim * dim row-major)
//     FORM 0:  w_f[e] = conj(a_f[e])                       a_f given element by element (ket on kets, matrix on matrices)
//     FORM 1:  w_f[e] = conj(phi_f[e / dim]) phi_f[e % dim]  A = |phi><phi| formed on the fly: <phi|rho|phi>
//   nrm[s]  = sum_e |x_s[e]|^2 (TRACE 0)   or   sum_i Re x_s[i (dim + 1)] (TRACE 1)
//
// The work is reading the states once; the targets are small and live in L2.  One workgroup owns kOverlapChunk
// consecutive elements (blockIdx.x), a tile of TILE targets (blockIdx.y; kOverlapTile, or 1 for a call with one target
// or none: 128 instead of 248 VGPRs, 4 instead of 2 waves per SIMD) and every gridDim.z-th state
// (blockIdx.z): a lane loads its 8 weights per target once into registers, then per state does 8 coalesced 16-byte
// loads (lane l of sweep k reads element chunk + 256 k + l; the next state's loads are issued before this state's sums
// are reduced) into TILE complex sums + 1 norm.  These are reduced over the 64 lanes with __shfl_down, over the four
// waves through LDS, and leave as one fp64 atomicAdd per value, workgroup and state (the pattern of k_expect_sparse).
// Elements past `len` and targets past `n_targets` contribute exact zeros: their loads are not issued and their
// weights are 0.  Only the first target tile adds the norms.  Every offset into the states is 64-bit.
constexpr int kOverlapChunk = 2048;  // elements per workgroup: 8 per lane
constexpr int kOverlapSweeps = kOverlapChunk / 256;
constexpr int kOverlapTile = 4;      // targets per workgroup: 64 fp64 weight registers per lane (TILE = 1: a lone target)

template <int FORM, int TRACE, int TILE>
__global__ __launch_bounds__(256) void k_overlap_many(const cplx* __restrict__ states, long long n_states, long long stride,
                                                      long long dim, long long len, const cplx* __restrict__ targets,
                                                      int n_targets, double* __restrict__ out, double* __restrict__ nrm) {
  constexpr int NV = 2 * TILE + 1;  // values a workgroup adds per state
  __shared__ double part[4][NV];
  const long long e0 = (long long)blockIdx.x * kOverlapChunk + threadIdx.x;
  const int f0 = blockIdx.y * TILE;
  const int nf = n_targets - f0 < TILE ? (n_targets - f0 > 0 ? n_targets - f0 : 0) : TILE;
  const long long tlen = FORM ? dim : len;  // elements of one target
  cplx w[TILE][kOverlapSweeps];
  bool diag[kOverlapSweeps];
#pragma unroll
  for (int k = 0; k < kOverlapSweeps; ++k) {
    const long long e = e0 + 256 * k;
    const bool in = e < len;
    diag[k] = TRACE && in && e % (dim + 1) == 0;
    const long long i = FORM && in ? e / dim : 0, j = FORM && in ? e % dim : 0;
#pragma unroll
    for (int f = 0; f < TILE; ++f) {
      w[f][k] = make_double2(0.0, 0.0);
      if (in && f < nf) {
        const cplx* a = targets + (long long)(f0 + f) * tlen;
        if (FORM) {
          const cplx p = a[i], q = a[j];  // conj(p) q
          w[f][k] = make_double2(p.x * q.x + p.y * q.y, p.x * q.y - p.y * q.x);
        } else {
          const cplx v = a[e];
          w[f][k] = make_double2(v.x, -v.y);
        }
      }
    }
  }
  auto load = [&](cplx (&x)[kOverlapSweeps], long long s) {
    const cplx* base = states + s * stride;
#pragma unroll
    for (int k = 0; k < kOverlapSweeps; ++k) {
      const long long e = e0 + 256 * k;
      x[k] = e < len ? base[e] : make_double2(0.0, 0.0);
    }
  };
  cplx x[kOverlapSweeps], nx[kOverlapSweeps];
  long long s = blockIdx.z;
  if (s < n_states) load(x, s);
  for (; s < n_states; s += gridDim.z) {
    const bool more = s + gridDim.z < n_states;
    if (more) load(nx, s + gridDim.z);
    double v[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = 0.0;
#pragma unroll
    for (int k = 0; k < kOverlapSweeps; ++k) {
#pragma unroll
      for (int f = 0; f < TILE; ++f) {
        v[2 * f] += w[f][k].x * x[k].x - w[f][k].y * x[k].y;
        v[2 * f + 1] += w[f][k].x * x[k].y + w[f][k].y * x[k].x;
      }
      if (TRACE)
        v[NV - 1] += diag[k] ? x[k].x : 0.0;
      else
        v[NV - 1] += x[k].x * x[k].x + x[k].y * x[k].y;
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int q = 0; q < NV; ++q) part[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    const int q = threadIdx.x;
    if (q < 2 * nf)  // (target of the tile, real / imaginary part) <-> out's interleaved doubles
      atomicAdd(out + 2 * (s * n_targets + f0) + q, (part[0][q] + part[1][q]) + (part[2][q] + part[3][q]));
    else if (q == NV - 1 && blockIdx.y == 0)
      atomicAdd(nrm + s, (part[0][q] + part[1][q]) + (part[2][q] + part[3][q]));
    __syncthreads();  // `part` is written again for the next state of this workgroup
    if (more) {
#pragma unroll
      for (int k = 0; k < kOverlapSweeps; ++k) x[k] = nx[k];
    }
  }
}

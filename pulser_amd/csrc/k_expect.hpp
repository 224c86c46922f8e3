// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_expect_sparse: <x_s| O |x_s> or Tr(O rho_s) of a user's operator over many stored states
// ---------------------------------------------------------------------------
// The operator comes as its non-zeros (rows[j], cols[j], vals[j]), sorted by (row, col).  Replaces the loop of
// qutip.expect over result.states (simresults.py:89-132) for the states that are still device snapshots.
//
//   kets:     out[s] += conj(x_s[rows[j]]) * vals[j] * x_s[cols[j]]
//   density:  out[s] += vals[j] * rho_s[cols[j]][rows[j]]            (rho_s row-major dim x dim)
//
// Work is split over the non-zeros, not over rows: in coordinate form a row of 1 and a row of 16 384 entries are the
// same case.  One workgroup owns kExpectChunk consecutive triplets (blockIdx.x) and a tile of kExpectTile states
// (blockIdx.y, grid-strided): a lane reads its triplet once - three coalesced loads - and gathers the two state
// entries of each state of the tile from L2 (a 14-atom ket is 256 KiB; sorted rows make x[row] the same address for
// neighbouring lanes).  kExpectTile complex sums per lane stay in registers, are reduced over the 64 lanes with
// __shfl_down, over the four waves through LDS, and leave as one fp64 atomicAdd pair per workgroup and state (the
// pattern of k_obs_energy).  States past the end of a partial tile alias the tile's first state, so that the inner
// loop has no branch; their sums are dropped.  Every offset into the states is 64-bit (stride * n_states exceeds
// 2^31 at 14 atoms with every evaluation time stored).
constexpr int kExpectChunk = 2048;  // triplets per workgroup: 8 per lane
constexpr int kExpectTile = 8;      // states per workgroup: 16 fp64 accumulators per lane

template <int DENSITY>
__global__ __launch_bounds__(256) void k_expect_sparse(const cplx* __restrict__ states, long long n_states, long long stride,
                                                       long long dim, const int* __restrict__ rows,
                                                       const int* __restrict__ cols, const cplx* __restrict__ vals,
                                                       long long nnz, double* __restrict__ out) {
  __shared__ double part[4][2 * kExpectTile];
  const long long j0 = (long long)blockIdx.x * kExpectChunk;
  const long long j1 = j0 + kExpectChunk < nnz ? j0 + kExpectChunk : nnz;
  const long long n_tiles = (n_states + kExpectTile - 1) / kExpectTile;
  for (long long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const long long s0 = tile * kExpectTile;
    const int ns = (int)(n_states - s0 < kExpectTile ? n_states - s0 : kExpectTile);
    const cplx* base[kExpectTile];
#pragma unroll
    for (int s = 0; s < kExpectTile; ++s) base[s] = states + (s0 + (s < ns ? s : 0)) * stride;
    double re[kExpectTile], im[kExpectTile];
#pragma unroll
    for (int s = 0; s < kExpectTile; ++s) re[s] = im[s] = 0.0;
    for (long long j = j0 + threadIdx.x; j < j1; j += 256) {
      const long long r = rows[j], c = cols[j];
      const cplx v = vals[j];
      if (DENSITY) {
        const long long e = c * dim + r;
#pragma unroll
        for (int s = 0; s < kExpectTile; ++s) {
          const cplx x = base[s][e];
          re[s] += v.x * x.x - v.y * x.y;
          im[s] += v.x * x.y + v.y * x.x;
        }
      } else {
#pragma unroll
        for (int s = 0; s < kExpectTile; ++s) {
          const cplx a = base[s][r], b = base[s][c];
          const double wx = v.x * b.x - v.y * b.y, wy = v.x * b.y + v.y * b.x;  // v x_c
          re[s] += a.x * wx + a.y * wy;                                          // conj(x_r) (v x_c)
          im[s] += a.x * wy - a.y * wx;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < kExpectTile; ++s) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        re[s] += __shfl_down(re[s], o, 64);
        im[s] += __shfl_down(im[s], o, 64);
      }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int s = 0; s < kExpectTile; ++s) {
        part[threadIdx.x >> 6][2 * s] = re[s];
        part[threadIdx.x >> 6][2 * s + 1] = im[s];
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * ns) {
      const int k = threadIdx.x;  // (state of the tile, real / imaginary part) <-> out's interleaved doubles
      atomicAdd(out + 2 * s0 + k, (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]));
    }
    __syncthreads();  // `part` is written again by the next tile of this workgroup
  }
}

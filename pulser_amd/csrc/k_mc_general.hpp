// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// Quantum-jump kernels of the general path (local dimension D = 2 .. 4, any D x D collapse operator, XY
// and multi-level registers): the counterpart of k_mc.hpp for vectors psi[d^N] whose atom a is the base-D
// digit of stride D^(N-1-a).  H_eff's decay -(i/2) sum_a sum_k C_k^dag C_k is an ordinary local term of the
// handle (ryd_general_set_collapse), so the stepper integrates the no-jump evolution; what is left is the
// bookkeeping after each CF4 step, with the jump rule of ryd_mc_solve unchanged:
//   norm:     ||psi||^2 per trajectory;
//   reduced:  for the trajectories whose norm fell below the threshold only, the site-reduced matrices
//             rho_a[j][k] = sum_rest psi[..j..] conj(psi[..k..]) (D^2 complex sums per atom);
//   select:   weights ||C_k psi||^2 = Re sum_jl (C_k^dag C_k)[l][j] rho_a[j][l], atom-major / operator-minor,
//             Philox4x32-10 (key = seed, counter = jump index) exactly as k_mc_select;
//   jump:     psi <- C_k^(a) psi / ||C_k psi||, in place (each thread owns the D amplitudes it gathers).
// McState is shared with k_mc.hpp; for the general path `red` is [B][N][D*D] complex (2 doubles each) and
// `ops` holds the C_k ([MC_MAX_OPS][D*D]) followed by the M_k = C_k^dag C_k (same layout).
// ---------------------------------------------------------------------------
#define MCG_MAX_D 4

__device__ __forceinline__ size_t mcg_stride(int D, int N, int a) {
  size_t s = 1;
  for (int i = 0; i < N - 1 - a; ++i) s *= (size_t)D;
  return s;
}

// first index of the D-tuple number i (digit of stride s = 0)
__device__ __forceinline__ size_t mcg_base(size_t i, size_t s, int D) { return (i / s) * s * (size_t)D + (i % s); }

// ||C psi||^2 = Re sum_{j,l} M[l][j] rho[j][l], rho interleaved (re, im) [D*D]
template <int D>
__device__ __forceinline__ double mcg_weight(const cplx* __restrict__ M, const double* rho) {
  double p = 0.0;
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int l = 0; l < D; ++l) {
      const cplx m = M[l * D + j];
      p += m.x * rho[2 * (j * D + l)] - m.y * rho[2 * (j * D + l) + 1];
    }
  return p;
}

__global__ __launch_bounds__(256) void k_mcg_norm(const cplx* __restrict__ st, long long dim,
                                                  double* __restrict__ norm2) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const cplx* __restrict__ x = st + (size_t)b * dim;
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)dim; i += (size_t)gridDim.x * 256) {
    const cplx v = x[i];
    s = fma(v.x, v.x, fma(v.y, v.y, s));
  }
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) atomicAdd(&norm2[b], s);
}

// start of a solve: thresholds of jump 0, reference norms (norm2 slot 0 holds the initial squared norms)
__global__ void k_mcg_init(McState M, int B, int red_per_b) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double ut, us;
  mc_uniforms(M.seeds[b], 0u, &ut, &us);
  M.target[b] = ut;
  M.refnorm[b] = M.norm2[b];
  M.lastnorm[b] = M.norm2[b];
  M.norm2[b] = 0.0;
  M.norm2[B + b] = 0.0;
  M.count[b] = 0;
  M.flag[b] = 0;
  for (int i = 0; i < red_per_b; ++i) M.red[(size_t)b * red_per_b + i] = 0.0;
}

// grid (blocks, B, N): the reduced matrix of atom blockIdx.z, only for the trajectories that jump this step
template <int D>
__global__ __launch_bounds__(256) void k_mcg_reduced(const cplx* __restrict__ st, long long dim, int N, McState M,
                                                     int B) {
  __shared__ double sh[4];
  const int b = blockIdx.y, a = blockIdx.z;
  if (!(M.norm2[b] <= M.target[b] * M.refnorm[b])) return;  // block-uniform
  const size_t s = mcg_stride(D, N, a), rest = (size_t)dim / D;
  const cplx* __restrict__ x = st + (size_t)b * dim;
  double acc[2 * D * D];
#pragma unroll
  for (int e = 0; e < 2 * D * D; ++e) acc[e] = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < rest; i += (size_t)gridDim.x * 256) {
    const size_t r0 = mcg_base(i, s, D);
    cplx v[D];
#pragma unroll
    for (int j = 0; j < D; ++j) v[j] = x[r0 + (size_t)j * s];
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        acc[2 * (j * D + k)] += v[j].x * v[k].x + v[j].y * v[k].y;      // psi_j conj(psi_k)
        acc[2 * (j * D + k) + 1] += v[j].y * v[k].x - v[j].x * v[k].y;
      }
  }
  double* red = M.red + ((size_t)b * N + a) * 2 * D * D;
#pragma unroll
  for (int e = 0; e < 2 * D * D; ++e) {
    const double t = block_sum256(acc[e], sh);
    if (threadIdx.x == 0) atomicAdd(red + e, t);
  }
}

template <int D>
__global__ void k_mcg_select(McState M, int B, int N) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double n2 = M.norm2[b];
  M.norm2[B + b] = 0.0;
  M.norm2[b] = 0.0;
  int flag = 0;
  double last = n2;
  if (n2 <= M.target[b] * M.refnorm[b]) {
    double* red = M.red + (size_t)b * N * 2 * D * D;
    const cplx* Ms = M.ops + MC_MAX_OPS * D * D;
    double total = 0.0;
    for (int a = 0; a < N; ++a)
      for (int k = 0; k < M.n_ops; ++k) total += fmax(mcg_weight<D>(Ms + k * D * D, red + a * 2 * D * D), 0.0);
    if (total > 0.0) {
      const unsigned j = (unsigned)M.count[b];
      double ut, us;
      mc_uniforms(M.seeds[b], j, &ut, &us);
      const double x = us * total;
      double cum = 0.0, psel = 0.0, plast = 0.0;
      int sel = -1, lastpos = -1;
      for (int a = 0; a < N; ++a)
        for (int k = 0; k < M.n_ops; ++k) {
          const double p = fmax(mcg_weight<D>(Ms + k * D * D, red + a * 2 * D * D), 0.0);
          cum += p;
          if (p > 0.0) { lastpos = a * MC_MAX_OPS + k; plast = p; }
          if (sel < 0 && p > 0.0 && cum > x) { sel = a * MC_MAX_OPS + k; psel = p; }
        }
      if (sel < 0) { sel = lastpos; psel = plast; }  // rounding left x >= cum
      M.sel[b] = sel;
      M.scale[b] = 1.0 / sqrt(psel);
      M.count[b] = (int)j + 1;
      mc_uniforms(M.seeds[b], j + 1u, &ut, &us);
      M.target[b] = ut;
      M.refnorm[b] = 1.0;
      last = 1.0;
      flag = 1;
    }
    for (int i = 0; i < N * 2 * D * D; ++i) red[i] = 0.0;
  }
  M.flag[b] = flag;
  M.lastnorm[b] = last;
}

// psi <- C^(atom) psi / ||C psi|| for the flagged trajectories: thread i owns the D-tuple i of the selected digit
template <int D>
__global__ __launch_bounds__(256) void k_mcg_jump(cplx* __restrict__ st, long long dim, int N, McState M) {
  const int b = blockIdx.y;
  if (!M.flag[b]) return;
  const int sel = M.sel[b];
  const size_t s = mcg_stride(D, N, sel / MC_MAX_OPS), rest = (size_t)dim / D;
  const cplx* __restrict__ C = M.ops + (sel % MC_MAX_OPS) * D * D;
  cplx c[D * D];
#pragma unroll
  for (int e = 0; e < D * D; ++e) c[e] = C[e];
  const double sc = M.scale[b];
  cplx* __restrict__ x = st + (size_t)b * dim;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < rest; i += (size_t)gridDim.x * 256) {
    const size_t r0 = mcg_base(i, s, D);
    cplx v[D];
#pragma unroll
    for (int j = 0; j < D; ++j) v[j] = x[r0 + (size_t)j * s];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      cplx o = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < D; ++k) o = cfma(c[j * D + k], v[k], o);
      x[r0 + (size_t)j * s] = make_double2(sc * o.x, sc * o.y);
    }
  }
}

// dst = src / ||src|| with the norm recorded after the last step (dst may be src)
__global__ __launch_bounds__(256) void k_mcg_normalize(const cplx* __restrict__ src, cplx* __restrict__ dst,
                                                       long long dim, const double* __restrict__ lastnorm) {
  const int b = blockIdx.y;
  const double s = rsqrt(lastnorm[b]);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)dim; i += (size_t)gridDim.x * 256) {
    const cplx v = src[(size_t)b * dim + i];
    dst[(size_t)b * dim + i] = make_double2(s * v.x, s * v.y);
  }
}

// ---------------------------------------------------------------------------
// The same bookkeeping inside the persistent one-workgroup kernel (k_gen_traj_mc: 1024 threads, rows
// tid + j * 1024, j < 4, dim <= 4096): the vector is in registers, `ws` is an LDS copy for the partner
// reads, `sh` [16][2 D^2] and `rho` [N][2 D^2] doubles of LDS scratch.  Block-uniform control flow; the
// caller has synchronised since its last read of `ws`.
// ---------------------------------------------------------------------------
struct McgTraj {
  double target, ref, n2;
  int count;
  unsigned long long seed;
};

#define MCG_TRAJ_SH (16 * 2 * MCG_MAX_D * MCG_MAX_D)  // doubles of `sh`
#define MCG_TRAJ_RHO 256                              // doubles of `rho`: N D^2 <= 96 complex for dim <= 4096

// squared norm of the workgroup's vector (every thread gets it)
__device__ __forceinline__ double mcg_traj_norm(const cplx psi[4], int dim, double* sh) {
  constexpr int NTT = 1024, R = 4, NW = NTT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s2 = 0.0;
#pragma unroll
  for (int j = 0; j < R; ++j)
    if (tid + j * NTT < dim) s2 = fma(psi[j].x, psi[j].x, fma(psi[j].y, psi[j].y, s2));
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_down(s2, o, 64);
  if (lane == 0) sh[wave] = s2;
  __syncthreads();
  double n2 = 0.0;
#pragma unroll
  for (int wv = 0; wv < NW; ++wv) n2 += sh[wv];
  __syncthreads();
  return n2;
}

template <int D>
__device__ __forceinline__ void mcg_traj_step(cplx psi[4], const unsigned long long digits[4], int dim, int N,
                                              const cplx* __restrict__ ops, int n_ops, cplx* ws, double* sh,
                                              double* rho, McgTraj& T) {
  constexpr int NTT = 1024, R = 4, NW = NTT / 64, E = 2 * D * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double n2 = mcg_traj_norm(psi, dim, sh);
  T.n2 = n2;
  if (!(n2 <= T.target * T.ref)) return;
#pragma unroll
  for (int j = 0; j < R; ++j)
    if (tid + j * NTT < dim) ws[tid + j * NTT] = psi[j];
  __syncthreads();
  for (int a = 0; a < N; ++a) {
    const int s = (int)mcg_stride(D, N, a), shift = 2 * (N - 1 - a);  // packed digits: 2 bits per digit (D <= 4)
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int row = tid + j * NTT;
      if (row >= dim) continue;
      const int dj = (int)((digits[j] >> shift) & 3u);
      const cplx v = psi[j];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const cplx u = ws[row + (k - dj) * s];
#pragma unroll
        for (int jj = 0; jj < D; ++jj)
          if (jj == dj) {
            acc[2 * (jj * D + k)] += v.x * u.x + v.y * u.y;
            acc[2 * (jj * D + k) + 1] += v.y * u.x - v.x * u.y;
          }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      double t = acc[e];
      for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
      if (lane == 0) sh[wave * E + e] = t;
    }
    __syncthreads();
    if (tid < E) {
      double t = 0.0;
      for (int wv = 0; wv < NW; ++wv) t += sh[wv * E + tid];
      rho[a * E + tid] = t;
    }
    __syncthreads();
  }
  // selection: every thread repeats the (uniform) arithmetic of k_mcg_select
  const cplx* Ms = ops + MC_MAX_OPS * D * D;
  double total = 0.0;
  for (int a = 0; a < N; ++a)
    for (int k = 0; k < n_ops; ++k) total += fmax(mcg_weight<D>(Ms + k * D * D, rho + a * E), 0.0);
  if (total > 0.0) {
    double ut, us;
    mc_uniforms(T.seed, (unsigned)T.count, &ut, &us);
    const double x = us * total;
    double cum = 0.0, psel = 0.0, plast = 0.0;
    int sel = -1, lastpos = -1;
    for (int a = 0; a < N; ++a)
      for (int k = 0; k < n_ops; ++k) {
        const double p = fmax(mcg_weight<D>(Ms + k * D * D, rho + a * E), 0.0);
        cum += p;
        if (p > 0.0) { lastpos = a * MC_MAX_OPS + k; plast = p; }
        if (sel < 0 && p > 0.0 && cum > x) { sel = a * MC_MAX_OPS + k; psel = p; }
      }
    if (sel < 0) { sel = lastpos; psel = plast; }
    const int a = sel / MC_MAX_OPS;
    const int s = (int)mcg_stride(D, N, a), shift = 2 * (N - 1 - a);
    const cplx* C = ops + (sel % MC_MAX_OPS) * D * D;
    const double sc = 1.0 / sqrt(psel);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int row = tid + j * NTT;
      if (row >= dim) continue;
      const int dj = (int)((digits[j] >> shift) & 3u);
      cplx o = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < D; ++k) o = cfma(C[dj * D + k], ws[row + (k - dj) * s], o);
      psi[j] = make_double2(sc * o.x, sc * o.y);
    }
    ++T.count;
    mc_uniforms(T.seed, (unsigned)T.count, &ut, &us);
    T.target = ut;
    T.ref = 1.0;
    T.n2 = 1.0;
  }
  __syncthreads();  // partner reads of ws done before the next step rewrites it
}

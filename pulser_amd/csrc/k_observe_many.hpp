// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_observe_many: the V2 observables of EVERY evaluation time of a run in one call
// ---------------------------------------------------------------------------
// ryd_observe (k_observe.hpp) serves one state per call: the backend uploaded each state, ran five launches and read
// the result back, once per evaluation time (3 101 times for a 14-atom run with evaluation_times="Full").  The
// snapshots of a solve are one device tensor already, so the same numbers for all of them are a memset and at most
// three launches.  Two-level Ising kets only.  State s = i * n_batch + b of the call lives at
// states + i * stride_t + b * stride_b (64-bit offsets: 3 101 x 2^14 amplitudes exceed 2^31 bytes), is observed with
// the coefficients of row (i, hb) of the table below, hb = b when the handle has one problem per entry and 0 when its
// one problem serves every entry, and writes row s of out ([N*N + N + 3] doubles, the layout of ryd_observe).
// The second grid axis is the state; it is capped at 65 535 workgroups, so every kernel strides over s.

// One (interval, offset into it) per evaluation time, found on the host exactly as ryd_observe finds it.
struct ObsManyTime {
  double u;
  int idx;
  int pad;
};

// coefs[i][hb][k] = (Re c, Im c, delta, 0) of atom k at time i: the arithmetic of k_eval_coefs with w1 = 1, w2 = 0,
// term for term and in the same order, one thread per (i, hb, k) (there a wave per entry shares the list of extra
// detuning terms; that list is not evaluated here: ryd_observe_many refuses handles that carry one).
__global__ __launch_bounds__(256) void k_eval_coefs_many(const cplx* __restrict__ pp, int n_int,
                                                         const ryd_qdesc* __restrict__ desc,
                                                         const ObsManyTime* __restrict__ tm, int per_time,
                                                         long long total, double* __restrict__ coefs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long it = i / per_time;
  const ryd_qdesc d = desc[i - it * per_time];
  const int idx = tm[it].idx;
  const double u = tm[it].u;
  const double w1 = 1.0, w2 = 0.0;
  auto val = [&](int s) -> cplx {
    const cplx* p = pp + ((size_t)s * n_int + idx) * 4;
    cplx r = p[0];
    r = make_double2(fma(r.x, u, p[1].x), fma(r.y, u, p[1].y));
    r = make_double2(fma(r.x, u, p[2].x), fma(r.y, u, p[2].y));
    r = make_double2(fma(r.x, u, p[3].x), fma(r.y, u, p[3].y));
    return r;
  };
  double cr = 0, ci = 0, dl = 0;
  if (d.drive_series >= 0) {
    const cplx a = val(d.drive_series), b2 = val(d.drive_series);
    cr = d.drive_scale * (w1 * a.x + w2 * b2.x);
    ci = d.drive_scale * (w1 * a.y + w2 * b2.y);
  }
  if (d.det_series >= 0) dl += d.det_scale * (w1 * val(d.det_series).x + w2 * val(d.det_series).x);
  if (d.off_series >= 0) dl += d.off_scale * (w1 * val(d.off_series).x + w2 * val(d.off_series).x);
  coefs[4 * (size_t)i + 0] = cr;
  coefs[4 * (size_t)i + 1] = ci;
  coefs[4 * (size_t)i + 2] = dl;
  coefs[4 * (size_t)i + 3] = 0.0;
}

// The pair reduction of k_obs_pairs (same chunk, same thread <-> pair map, same order of the sums) over kets taken
// from the grid: out[s][0..N-1] = <n_k>, out[s][N] = sum p, out[s][N+1 + k*N + l] = <n_k n_l>.
__global__ __launch_bounds__(256) void k_obs_pairs_many(const cplx* __restrict__ states, long long n_states,
                                                        int n_batch, long long stride_t, long long stride_b, int N,
                                                        int what, double* __restrict__ out, int out_stride) {
  constexpr int CH = 2048;
  __shared__ double ps[CH];
  const size_t D = (size_t)1 << N;
  const int npair = N * (N + 1) / 2;
  const size_t base = (size_t)blockIdx.x * CH;
  for (long long s = blockIdx.y; s < n_states; s += gridDim.y) {
    const long long it = s / n_batch, b = s - it * n_batch;
    const cplx* st = states + it * stride_t + b * stride_b;
    for (int i = threadIdx.x; i < CH; i += blockDim.x) {
      const size_t g = base + i;
      double p = 0.0;
      if (g < D) { const cplx v = st[g]; p = v.x * v.x + v.y * v.y; }
      ps[i] = p;
    }
    __syncthreads();
    double* o = out + (size_t)s * out_stride;
    for (int pr = threadIdx.x; pr <= npair; pr += blockDim.x) {
      if (pr == npair) {  // the norm
        double sum = 0.0;
        for (int i = 0; i < CH; ++i) sum += ps[i];
        atomicAdd(o + N, sum);
        continue;
      }
      int k = 0, rem = pr;
      while (rem >= N - k) { rem -= N - k; ++k; }
      const int l = k + rem;
      if (k != l && !(what & RYD_OBS_CORRELATION)) continue;
      if (k == l && !(what & (RYD_OBS_OCCUPATION | RYD_OBS_CORRELATION))) continue;
      const unsigned mk = 1u << (N - 1 - k), ml = 1u << (N - 1 - l);
      double sum = 0.0;
      for (int i = 0; i < CH; ++i) {
        const unsigned g = (unsigned)(base + i);
        if (!(g & mk) && !(g & ml)) sum += ps[i];  // n = 1 <=> bit 0 (local state 0 = r)
      }
      if (k == l && (what & RYD_OBS_OCCUPATION)) atomicAdd(o + k, sum);
      if (!(what & RYD_OBS_CORRELATION)) continue;
      atomicAdd(o + N + 1 + k * N + l, sum);
      if (k != l) atomicAdd(o + N + 1 + l * N + k, sum);
    }
    __syncthreads();  // `ps` is filled again for the next state of this workgroup
  }
}

// <H> and <H^2> of a ket without writing w = H x anywhere: one workgroup stages a tile of 2^TB consecutive amplitudes
// of one state in LDS and forms, for each of them,
//   w_a = (e0[a] - sum_{k: bit_k(a) = 0} delta_k) x_a + sum_k h_k(a) x_{a ^ k},   h_k(a) = bit_k(a) ? c_k : conj(c_k)
// (atom k on bit N-1-k: the conventions of k_obs_energy_dm and k_build_e0).  The partner of a flip of one of the low TB
// bits is in the tile (one 16-byte LDS read, consecutive lanes on consecutive slots); the partner of a higher bit is
// the same slot of another tile, a coalesced 16-byte load that L2 serves (a 14-atom ket is 256 KiB).  Re(conj(x_a) w_a)
// and |w_a|^2 stay in registers, go through __shfl_down and then LDS across the four waves, and leave as one fp64
// atomicAdd pair per workgroup (the pattern of k_obs_energy / k_expect_sparse).  TB = 11: 32 KiB of LDS, so four
// workgroups share a CU, and a 14-atom state is 8 workgroups - 3 101 states fill the 256 CUs many times over, while
// only 3 of the 14 partners of an amplitude come from outside the tile.  Registers of fewer than TB atoms fill a part
// of the tile and load no partner from global memory.  `with_norm`: also out[s][N] += sum |x_a|^2 (energy-only calls,
// where k_obs_pairs_many does not run).
constexpr int kObsManyTB = 11;

__global__ __launch_bounds__(256) void k_obs_energy_many(const cplx* __restrict__ states, long long n_states,
                                                         int n_batch, long long stride_t, long long stride_b, int N,
                                                         const double* __restrict__ coefs, int handle_batch,
                                                         const double* __restrict__ e0, long long e0_stride,
                                                         int with_norm, double* __restrict__ out, int out_stride) {
  constexpr int TILE = 1 << kObsManyTB;
  __shared__ cplx tile[TILE];
  __shared__ double cf[4 * RYD_MAX_QUBITS];
  __shared__ double part[4][3];
  const size_t D = (size_t)1 << N;
  const size_t a0 = (size_t)blockIdx.x * TILE;
  const int n_in = (int)(D - a0 < (size_t)TILE ? D - a0 : (size_t)TILE);  // amplitudes of this tile (D < TILE: all of them)
  const int off = N * N + N + 1;
  for (long long s = blockIdx.y; s < n_states; s += gridDim.y) {
    const long long it = s / n_batch, b = s - it * n_batch;
    const long long hb = handle_batch == 1 ? 0 : b;
    const cplx* st = states + it * stride_t + b * stride_b;
    const double* cfg = coefs + ((size_t)it * handle_batch + hb) * N * 4;
    const double* e0b = e0 + hb * e0_stride;
    for (int i = threadIdx.x; i < n_in; i += 256) tile[i] = st[a0 + i];
    for (int i = threadIdx.x; i < 4 * N; i += 256) cf[i] = cfg[i];
    __syncthreads();
    double e1 = 0.0, e2 = 0.0, nrm = 0.0;
    for (int i = threadIdx.x; i < n_in; i += 256) {
      const size_t a = a0 + i;
      const cplx x = tile[i];
      double diag = e0b[a];
      double wx = 0.0, wy = 0.0;
      for (int k = 0; k < N; ++k) {
        const int p = N - 1 - k;
        const bool bit = (a >> p) & 1;
        const double cr = cf[4 * k], ci = bit ? cf[4 * k + 1] : -cf[4 * k + 1];
        if (!bit) diag -= cf[4 * k + 2];
        const cplx y = p < kObsManyTB ? tile[i ^ (1 << p)] : st[a ^ ((size_t)1 << p)];
        wx += cr * y.x - ci * y.y;
        wy += cr * y.y + ci * y.x;
      }
      wx = fma(diag, x.x, wx);
      wy = fma(diag, x.y, wy);
      e1 += x.x * wx + x.y * wy;
      e2 = fma(wx, wx, fma(wy, wy, e2));
      nrm = fma(x.x, x.x, fma(x.y, x.y, nrm));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      e1 += __shfl_down(e1, o, 64);
      e2 += __shfl_down(e2, o, 64);
      nrm += __shfl_down(nrm, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      part[threadIdx.x >> 6][0] = e1;
      part[threadIdx.x >> 6][1] = e2;
      part[threadIdx.x >> 6][2] = nrm;
    }
    __syncthreads();
    if (threadIdx.x < 3 && (threadIdx.x < 2 || with_norm)) {
      const int j = threadIdx.x;
      const double v = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
      atomicAdd(out + (size_t)s * out_stride + (j < 2 ? off + j : N), v);
    }
    __syncthreads();  // `tile`, `cf` and `part` are written again for the next state of this workgroup
  }
}

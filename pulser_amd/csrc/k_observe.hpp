// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_observe: the V2 observables of one state in one call, on the device (ryd_observe_many: second half of the file)
// ---------------------------------------------------------------------------
// Occupations <n_k>, correlations <n_k n_l> (default_observables.py:291-435) and the energy
// moments <H>, <H^2> (:437-580, through one generator application w = -i H x:
// <H> = -Im <x|w>, <H^2> = |w|^2).  Replaces N(N+1)/2 + 2 qutip.expect calls and the per-time
// materialisation of H(t) (qutip_backend.py:259-264).

// The pair sums of one staged chunk, shared by every pair kernel: ps[i] is the probability of chunk element i (0 past the
// end of the state), o the output row: o[0..N-1] += <n_k>, o[N] += sum p, o[N+1 + k*N + l] += <n_k n_l>.
// thread <-> (k <= l) pair (several per thread when N(N+1)/2 >= blockDim), one more for the norm; the chunk index is
// wave-uniform -> LDS broadcast reads; one atomic per pair and block.  `what`: RYD_OBS_OCCUPATION and / or
// RYD_OBS_CORRELATION - the slots of the one not asked for stay 0, and with neither only the norm is written.
// "Atoms k and l of element i are in the one-state" - DIGITS = false: bits N-1-k and N-1-l of the index base + i are 0
// (two-level registers: n = 1 <=> bit 0, local state 0 = r); DIGITS = true: bits k and l of the staged word wd[i] are set.
constexpr int kObsCH = 2048;

template <bool DIGITS>
__device__ __forceinline__ void obs_pair_sums(const double* ps, const unsigned* wd, size_t base, int N, int what,
                                              double* __restrict__ o) {
  const int npair = N * (N + 1) / 2;
  for (int pr = threadIdx.x; pr <= npair; pr += blockDim.x) {
    if (pr == npair) {  // the norm
      double s = 0.0;
      for (int i = 0; i < kObsCH; ++i) s += ps[i];
      atomicAdd(o + N, s);
      continue;
    }
    // pair index -> (k <= l)
    int k = 0, rem = pr;
    while (rem >= N - k) { rem -= N - k; ++k; }
    const int l = k + rem;
    if (k != l && !(what & RYD_OBS_CORRELATION)) continue;
    if (k == l && !(what & (RYD_OBS_OCCUPATION | RYD_OBS_CORRELATION))) continue;
    const unsigned m = DIGITS ? (1u << k) | (1u << l) : (1u << (N - 1 - k)) | (1u << (N - 1 - l));
    double s = 0.0;
    for (int i = 0; i < kObsCH; ++i)
      if (DIGITS ? (wd[i] & m) == m : !((unsigned)(base + i) & m)) s += ps[i];
    if (k == l && (what & RYD_OBS_OCCUPATION)) atomicAdd(o + k, s);
    if (!(what & RYD_OBS_CORRELATION)) continue;
    atomicAdd(o + N + 1 + k * N + l, s);
    if (k != l) atomicAdd(o + N + 1 + l * N + k, s);
  }
}

// Row s of out ([out_stride] doubles, laid out as above) for state s = it * n_batch + b at states + it * stride_t +
// b * stride_b (64-bit offsets), the states taken from the second grid axis with a stride (it is capped at 65 535
// workgroups).  One block stages a chunk of probabilities in LDS: |x_g|^2 of a ket, Re rho_gg of a density matrix
// (is_dm: stride_b = D * D).  ryd_observe: n_states = n_batch = its batch.
__global__ __launch_bounds__(256) void k_obs_pairs(const cplx* __restrict__ states, long long n_states, int n_batch,
                                                   long long stride_t, long long stride_b, int N, int is_dm, int what,
                                                   double* __restrict__ out, int out_stride) {
  __shared__ double ps[kObsCH];
  const size_t D = (size_t)1 << N;
  const size_t base = (size_t)blockIdx.x * kObsCH;
  for (long long s = blockIdx.y; s < n_states; s += gridDim.y) {
    const long long it = s / n_batch, b = s - it * n_batch;
    const cplx* st = states + it * stride_t + b * stride_b;
    for (int i = threadIdx.x; i < kObsCH; i += blockDim.x) {
      const size_t g = base + i;
      double p = 0.0;
      if (g < D) {
        if (is_dm) p = st[g * (D + 1)].x;
        else { const cplx v = st[g]; p = v.x * v.x + v.y * v.y; }
      }
      ps[i] = p;
    }
    __syncthreads();
    obs_pair_sums<false>(ps, nullptr, base, N, what, out + (size_t)s * out_stride);
    __syncthreads();  // `ps` is filled again for the next state of this workgroup
  }
}

// o[0] += -Im <x|w>, o[1] += |w|^2 over vectors of any length D: wave64 shuffles, one atomic pair per wave.
__global__ __launch_bounds__(256) void k_obs_energy(const cplx* __restrict__ x, const cplx* __restrict__ w, size_t D,
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

// Density matrices: <H> = Tr(H rho) and <H^2> = Tr(H^2 rho) only touch the matrix elements of H
// and H^2 around the diagonal: with h_k(a) = H_{a, a^k} = (bit_k(a) ? c_k : conj c_k),
//   (H)_{aa} = E(a);            (H^2)_{aa}      = E(a)^2 + sum_k |c_k|^2
//   (H)_{a,a^k} = h_k(a);       (H^2)_{a,a^k}   = h_k(a) (E(a) + E(a^k))
//                               (H^2)_{a,a^k^l} = 2 h_k(a) h_l(a)      (k != l)
// so one thread per row index a gathers 1 + N + N(N-1)/2 elements of column a.  No H(t) is built
// (qutip_backend.py:259-264 materialises it) and rho is not multiplied by anything dense.

// E(s) = e0[s] - sum_{k: bit_k(s) = 0} delta_k (atom k on bit N-1-k; cf = the (Re c, Im c, delta, 0) rows of one time)
__device__ __forceinline__ double obs_dm_diag(const double* e0b, const double* cf, int N, size_t s) {
  double e = e0b[s];
  for (int k = 0; k < N; ++k)
    if (!((s >> (N - 1 - k)) & 1)) e -= cf[4 * k + 2];
  return e;
}

// sum_k |c_k|^2
__device__ __forceinline__ double obs_dm_c2(const double* cf, int N) {
  double c2 = 0.0;
  for (int k = 0; k < N; ++k) c2 += cf[4 * k] * cf[4 * k] + cf[4 * k + 1] * cf[4 * k + 1];
  return c2;
}

// What ONE stored element x = rho[r][c] adds to e1 = Tr(H rho) and e2 = Tr(H^2 rho) - the arithmetic of both density
// kernels, k_obs_energy_dm (a thread gathers column c) and k_obs_energy_dm_many (eight lanes read a 128-byte piece of
// row r).  `flips` = popcount(r ^ c): 0 - the diagonal; 1 - r ^ c is the bit of atom k; 2 - the bits of atoms k < l;
// anything else adds nothing.  rho is read as stored (not assumed Hermitian) and the real part is kept.
// Er = E(r), Ec = E(c), c2 = sum_k |c_k|^2; k, l are read only where `flips` says so.
__device__ __forceinline__ void obs_dm_add(const cplx x, const int flips, const int k, const int l, const size_t c,
                                           const int N, const double* cf, const double Er, const double Ec,
                                           const double c2, double& e1, double& e2) {
  if (flips == 0) {
    e1 += Ec * x.x;
    e2 += (Ec * Ec + c2) * x.x;
  } else if (flips == 1 || flips == 2) {
    const bool bk = (c >> (N - 1 - k)) & 1;
    const cplx hk = make_double2(cf[4 * k], bk ? cf[4 * k + 1] : -cf[4 * k + 1]);  // h_k(c)
    if (flips == 1) {
      const double re = hk.x * x.x - hk.y * x.y;  // Re(h_k rho_{c^k,c}); the imaginary parts cancel in the trace
      e1 += re;
      e2 += re * (Ec + Er);
    } else {
      const bool bl = (c >> (N - 1 - l)) & 1;
      const cplx hl = make_double2(cf[4 * l], bl ? cf[4 * l + 1] : -cf[4 * l + 1]);
      const cplx hh = cmul(hk, hl);
      e2 += 2.0 * (hh.x * x.x - hh.y * x.y);
    }
  }
}

__global__ __launch_bounds__(256) void k_obs_energy_dm(const cplx* __restrict__ rho, int N,
                                                       const double* __restrict__ coefs,
                                                       const double* __restrict__ e0, long long e0_stride,
                                                       double* __restrict__ out, int out_stride, int off) {
  const size_t D = (size_t)1 << N;
  const int b = blockIdx.y;
  const cplx* r = rho + ((size_t)b << (2 * N));
  const double* cf = coefs + (size_t)b * N * 4;
  const double* e0b = e0 + (size_t)b * e0_stride;
  double e1 = 0.0, e2 = 0.0;
  for (size_t a = (size_t)blockIdx.x * 256 + threadIdx.x; a < D; a += (size_t)gridDim.x * 256) {
    const double Ea = obs_dm_diag(e0b, cf, N, a);
    const double c2 = obs_dm_c2(cf, N);
    obs_dm_add(r[a * D + a], 0, 0, 0, a, N, cf, Ea, Ea, c2, e1, e2);
    for (int k = 0; k < N; ++k) {
      const size_t ak = a ^ ((size_t)1 << (N - 1 - k));
      obs_dm_add(r[ak * D + a], 1, k, 0, a, N, cf, obs_dm_diag(e0b, cf, N, ak), Ea, c2, e1, e2);  // rho_{a^k, a}
      for (int l = k + 1; l < N; ++l)
        obs_dm_add(r[(ak ^ ((size_t)1 << (N - 1 - l))) * D + a], 2, k, l, a, N, cf, 0.0, Ea, c2, e1, e2);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { e1 += __shfl_down(e1, o, 64); e2 += __shfl_down(e2, o, 64); }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out + (size_t)b * out_stride + off, e1);
    atomicAdd(out + (size_t)b * out_stride + off + 1, e2);
  }
}

// ---------------------------------------------------------------------------
// ryd_observe_many: the V2 observables of EVERY evaluation time of a run in one call
// ---------------------------------------------------------------------------
// ryd_observe serves one state per call: the backend uploaded each state, ran five launches and read
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

// coefs[i][hb][k] = (Re c, Im c, delta, 0) of atom k at time i, one thread per (i, hb, k): qdesc_coefs at one time with
// weight 1, as k_eval_coefs evaluates it (there a wave per entry shares the list of extra detuning terms; that list is
// not evaluated here: ryd_observe_many refuses handles that carry one).
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
  double cr, ci, dl;
  qdesc_coefs(pp, n_int, d, idx, u, 1.0, idx, u, 0.0, cr, ci, dl);
  coefs[4 * (size_t)i + 0] = cr;
  coefs[4 * (size_t)i + 1] = ci;
  coefs[4 * (size_t)i + 2] = dl;
  coefs[4 * (size_t)i + 3] = 0.0;
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
// where k_obs_pairs does not run).
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

// ---------------------------------------------------------------------------
// ryd_observe_density_many: Tr(H rho), Tr(H^2 rho) of EVERY density matrix of a master-equation run in one launch
// ---------------------------------------------------------------------------
// k_obs_energy_dm gives lane a the elements rho[(a ^ m) * D + a] of COLUMN a: the 64 lanes of a wave read 64 different
// rows, one 16-byte element each.  Here the work is organised by the ROW that holds the elements (rho is row-major):
// of row r the sums need the columns c = r ^ m with popcount(m) <= 2, and with m = hi | lo (lo = the low three bits)
// the eight columns (r ^ hi) ^ lo, lo = 0 .. 7, are ONE aligned 128-byte piece of the row.  Eight lanes read it with
// one 16-byte load each, so a wave instruction covers eight whole 128-byte pieces (of eight consecutive rows), and the
// pieces fetched per row are, for N >= 3,
//   hi = 0:                   1 piece,                 7 of its 8 elements add something (lo = 7 flips three atoms)
//   hi = one higher bit:      N - 3 pieces,            4 of 8 (lo = 0: that atom alone; one low bit: a pair)
//   hi = two higher bits:     (N - 3)(N - 4) / 2,      1 of 8 (lo = 0)
// = 1 + (N - 3) + (N - 3)(N - 4) / 2 pieces of 128 bytes (29 of the 128 of a 10-atom row).  An element that adds
// nothing costs its lane nothing but the load: obs_dm_add ignores more than two flips.  Registers of N < 3 atoms have
// rows of 2 or 4 elements, read by the first 2 or 4 lanes of a group.
// The piece is the same for the eight groups of a wave (and the four waves of the workgroup), so whether E(c) is needed
// (one flip: only where hi has at most one bit) is uniform: the loops over the pieces do not diverge.  E(r) is formed
// once per row and lane, E(c) by the lanes that need it (e0 is 2^N doubles per problem and stays in cache); the 4N
// coefficients of the state's time are staged in LDS once per state.  Partial sums: __shfl_down, LDS across the four
// waves, one fp64 atomicAdd pair per workgroup and state (k_obs_energy_many's pattern).  State s = it * n_batch + b
// comes from the second grid axis with a stride (capped at 65 535), its coefficients are row (it, hb) of the table of
// k_eval_coefs_many, hb = b or 0 (handle_batch = 1).  Rows: group g of workgroup x takes r = 32 x + g, + 32 gridDim.x, ...
// `with_norm`: also out[s][N] += sum_r Re rho_rr (energy-only calls, where k_obs_pairs does not run).
__global__ __launch_bounds__(256) void k_obs_energy_dm_many(const cplx* __restrict__ states, long long n_states,
                                                            int n_batch, long long stride_t, long long stride_b, int N,
                                                            const double* __restrict__ coefs, int handle_batch,
                                                            const double* __restrict__ e0, long long e0_stride,
                                                            int with_norm, double* __restrict__ out, int out_stride) {
  __shared__ double cf[4 * RYD_MAX_QUBITS];
  __shared__ double part[4][3];
  const unsigned D = 1u << N;
  const unsigned g = threadIdx.x >> 3, lo = threadIdx.x & 7;
  const int off = N * N + N + 1;
  for (long long s = blockIdx.y; s < n_states; s += gridDim.y) {
    const long long it = s / n_batch, b = s - it * n_batch;
    const long long hb = handle_batch == 1 ? 0 : b;
    const cplx* st = states + it * stride_t + b * stride_b;
    const double* cfg = coefs + ((size_t)it * handle_batch + hb) * N * 4;
    const double* e0b = e0 + hb * e0_stride;
    for (int i = threadIdx.x; i < 4 * N; i += 256) cf[i] = cfg[i];
    __syncthreads();
    const double c2 = obs_dm_c2(cf, N);
    double e1 = 0.0, e2 = 0.0, nrm = 0.0;
    for (unsigned r = blockIdx.x * 32 + g; r < D; r += gridDim.x * 32) {
      const cplx* row = st + (size_t)r * D;
      const double Er = obs_dm_diag(e0b, cf, N, r);
      // the piece of row r that holds column r ^ hi; `one`: some lane of it is one flip away from r
      auto piece = [&](const unsigned hi, const bool one) {
        const unsigned c = ((r ^ hi) & ~7u) | lo;
        if (c >= D) return;  // (N < 3: a row is shorter than a piece)
        const unsigned m = r ^ c;
        const int flips = __popc(m);
        // atoms k < l of the flipped bits (atom k on bit N-1-k): k from the highest set bit, l from the lowest
        const int k = m ? N - 1 - (31 - __clz((int)m)) : 0, l = m ? N - 1 - (__ffs((int)m) - 1) : 0;
        const double Ec = flips == 0 ? Er : (one && flips == 1) ? obs_dm_diag(e0b, cf, N, c) : 0.0;
        const cplx x = row[c];
        obs_dm_add(x, flips, k, l, c, N, cf, Er, Ec, c2, e1, e2);
        if (flips == 0) nrm += x.x;
      };
      piece(0u, true);
      for (int p = 3; p < N; ++p) piece(1u << p, true);
      for (int p = 3; p < N; ++p)
        for (int q = p + 1; q < N; ++q) piece((1u << p) | (1u << q), false);
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
    __syncthreads();  // `cf` and `part` are written again for the next state of this workgroup
  }
}

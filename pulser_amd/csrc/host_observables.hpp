// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// observables / marshalling
// ---------------------------------------------------------------------------
extern "C" int ryd_probabilities(ryd_handle* h, const void* state_dev, double* w_dev,
                                 int32_t reverse, void* stream) {
  if (!h || !state_dev || !w_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (h->general) return fail(RYD_ERR_INVALID, "not available on a general-path handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t D = (size_t)1 << h->N;
  dim3 grid((unsigned)((D + 255) / 256), h->B);
  hipLaunchKernelGGL(k_probabilities, grid, dim3(256), 0, (hipStream_t)stream,
                     (const cplx*)state_dev, h->N, h->cfg.mode == RYD_MESOLVE, reverse, w_dev);
  HIPCHK(hipGetLastError());
  return RYD_OK;
}

extern "C" int ryd_occupations(ryd_handle* h, const void* state_dev, double* out_dev,
                               void* stream) {
  if (!h || !state_dev || !out_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (h->general) return fail(RYD_ERR_INVALID, "not available on a general-path handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(out_dev, 0, (size_t)h->B * (h->N + 1) * sizeof(double), st));
  const size_t D = (size_t)1 << h->N;
  const unsigned nblk = (unsigned)std::min<size_t>((D + 255) / 256, 1024);
  hipLaunchKernelGGL(k_occupations, dim3(nblk, h->B), dim3(256), 0, st, (const cplx*)state_dev,
                     h->N, h->cfg.mode == RYD_MESOLVE, out_dev);
  HIPCHK(hipGetLastError());
  return RYD_OK;
}

extern "C" int ryd_observe(ryd_handle* h, const void* state_dev, double t, int32_t what,
                           double* out_dev, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!state_dev || !out_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (h->general) return fail(RYD_ERR_INVALID, "not available on a general-path handle");
  const bool dm = h->cfg.mode == RYD_MESOLVE || (what & RYD_OBS_DENSITY) != 0;
  if (2 * h->N > RYD_MAX_QUBITS && dm) return fail(RYD_ERR_INVALID, "2N exceeds %d", RYD_MAX_QUBITS);
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N;
  const int stride = N * N + N + 3;
  HIPCHK(hipMemsetAsync(out_dev, 0, (size_t)h->B * stride * sizeof(double), st));
  const size_t D = (size_t)1 << N;
  if (what & (RYD_OBS_OCCUPATION | RYD_OBS_CORRELATION)) {
    hipLaunchKernelGGL(k_obs_pairs, dim3((unsigned)((D + 2047) / 2048), h->B), dim3(256), 0, st, (const cplx*)state_dev,
                       (long long)h->B, h->B, 0ll, (long long)(dm ? D * D : D), N, dm ? 1 : 0, (int)what, out_dev, stride);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
  }
  if (what & RYD_OBS_ENERGY) {
    if (!h->bounds_valid) compute_bounds(h);
    if ((rc = launch_eval(h, mix_at(h, t), st))) return rc;
    if (dm) {
      // Tr(H rho), Tr(H^2 rho) from the elements of rho within two bit flips of the diagonal
      const unsigned nblk = (unsigned)std::min<size_t>(std::max<size_t>(D >> 8, 1), 1024);
      hipLaunchKernelGGL(k_obs_energy_dm, dim3(nblk, h->B), dim3(256), 0, st, (const cplx*)state_dev, N,
                         (const double*)h->coefs_dev, (const double*)h->e0_dev,
                         h->e0_mats == 1 ? 0ll : (long long)D, out_dev, stride, N * N + N + 1);
      HIPCHK(hipGetLastError());
      h->stats.n_launches++;
      return RYD_OK;
    }
    if (h->cfg.mode != RYD_SESOLVE)
      return fail(RYD_ERR_UNSUPPORTED, "ket energy moments need a sesolve handle");
    if ((rc = apply_generator(h, (const cplx*)state_dev, nullptr, h->wA, 1.0, 1.0, 0.0,
                              make_double2(1.0, 0.0), st)))
      return rc;
    const unsigned nblk = (unsigned)std::min<size_t>(std::max<size_t>(D >> 10, 1), 1024);
    hipLaunchKernelGGL(k_obs_energy, dim3(nblk, h->B), dim3(256), 0, st, (const cplx*)state_dev,
                       (const cplx*)h->wA, D, out_dev, stride, N * N + N + 1);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
  }
  return RYD_OK;
}

// ryd_observe for a general-path handle (d-level registers): k_gen_observe.hpp
static const size_t kGenObsScratchCap = (size_t)256 << 20;  // staged columns of rho + H applied to them

extern "C" int ryd_general_observe(ryd_handle* h, const void* state_dev, double t, int32_t what, int32_t local_dim,
                                   int32_t n_atoms, int32_t one_digit, double* out_dev, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!h->general) return fail(RYD_ERR_INVALID, "not a general-path handle: use ryd_observe");
  if (!state_dev || !out_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (local_dim < 2 || local_dim > 4 || n_atoms < 1 || n_atoms > 26 || one_digit < 0 || one_digit >= local_dim)
    return fail(RYD_ERR_INVALID, "observe: local_dim=%d n_atoms=%d one_digit=%d out of range", local_dim, n_atoms, one_digit);
  size_t D = 1;
  for (int i = 0; i < n_atoms; ++i) {
    D *= (size_t)local_dim;
    if (D > ((size_t)1 << 26)) return fail(RYD_ERR_INVALID, "observe: %d^%d exceeds 2^26", local_dim, n_atoms);
  }
  if (h->dim != (h->gen_density ? D * D : D))
    return fail(RYD_ERR_INVALID, "observe: dim %lld is not %d^%d%s", (long long)h->dim, local_dim, n_atoms,
                h->gen_density ? " squared" : "");
  const bool dm = h->gen_density || (what & RYD_OBS_DENSITY) != 0;
  if (dm && D > ((size_t)1 << 13)) return fail(RYD_ERR_INVALID, "observe: a %lld x %lld density matrix exceeds 2^26 entries", (long long)D, (long long)D);
  if (what & RYD_OBS_ENERGY) {
    if (h->gen_density)
      return fail(RYD_ERR_UNSUPPORTED, "energy moments need a ket handle: this handle's generator is the Liouvillian");
    if (h->gen_mc_term >= 0)
      return fail(RYD_ERR_UNSUPPORTED, "energy moments need a handle without collapse operators (its generator is H_eff)");
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  const int N = n_atoms, B = h->B;
  const int stride = N * N + N + 3, off = N * N + N + 1;
  HIPCHK(hipMemsetAsync(out_dev, 0, (size_t)B * stride * sizeof(double), st));
  if (what & (RYD_OBS_OCCUPATION | RYD_OBS_CORRELATION)) {
    hipLaunchKernelGGL(k_gen_obs_pairs, dim3((unsigned)((D + 2047) / 2048), B), dim3(256), 0, st, (const cplx*)state_dev,
                       (long long)B, B, 0ll, (long long)(dm ? D * D : D), (unsigned)D, N, (int)local_dim, (int)one_digit,
                       dm ? 1 : 0, (int)what, out_dev, stride);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
  }
  if (!(what & RYD_OBS_ENERGY)) return RYD_OK;
  const MixPoint m = mix_at(h, t);
  if ((rc = launch_eval_general(h, m, st))) return rc;
  if (!dm) {
    if ((rc = apply_general(h, m, (const cplx*)state_dev, nullptr, h->wA, 1.0, st))) return rc;
    const unsigned nblk = (unsigned)std::min<size_t>(std::max<size_t>(D >> 10, 1), 1024);
    hipLaunchKernelGGL(k_obs_energy, dim3(nblk, B), dim3(256), 0, st, (const cplx*)state_dev, (const cplx*)h->wA, D,
                       out_dev, stride, off);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
    return RYD_OK;
  }
  // density matrix on a ket handle: H on the columns of rho, nc columns of every batch entry per chunk
  size_t nc = std::min<size_t>(D, kGenObsScratchCap / (2 * sizeof(cplx) * (size_t)B * D));
  nc = std::min<size_t>(nc, 65535 / (size_t)B);  // (the batch axis of the application is blockIdx.y)
  if (h->gen_obs_small_chunks) nc = std::min<size_t>(nc, 5);
  if (nc < 1)  // (65535 / B >= 1: ryd_general_create caps the batch there)
    return fail(RYD_ERR_UNSUPPORTED, "observe: one column of every batch entry (%d x %lld) exceeds the 256-MiB scratch cap", B, (long long)D);
  const size_t half = nc * (size_t)B * D, bytes = 2 * half * sizeof(cplx);
  if (bytes > h->gen_obs_scratch_bytes) {
    if (h->gen_obs_scratch) HIPCHK(hipFree(h->gen_obs_scratch));
    h->gen_obs_scratch = nullptr;
    h->gen_obs_scratch_bytes = 0;
    HIPCHK(hipMalloc((void**)&h->gen_obs_scratch, bytes));
    h->gen_obs_scratch_bytes = bytes;
  }
  cplx* X = h->gen_obs_scratch;
  cplx* W = X + half;
  for (size_t c0 = 0; c0 < D; c0 += nc) {
    const unsigned n = (unsigned)std::min<size_t>(nc, D - c0);
    const int n_vec = (int)n * B;
    const unsigned tblk = std::min<unsigned>((n + 255) / 256, 64);
    hipLaunchKernelGGL(k_gen_obs_stage_cols, dim3((n + 31) / 32, (unsigned)((D + 31) / 32), B), dim3(256), 0, st,
                       (const cplx*)state_dev, X, (unsigned)D, (unsigned)c0, n);
    HIPCHK(hipGetLastError());
    if ((rc = apply_general(h, m, X, nullptr, W, 1.0, st, n_vec))) return rc;   // W  = -i H X
    hipLaunchKernelGGL(k_gen_obs_trace, dim3(tblk, B), dim3(256), 0, st, (const cplx*)W, (unsigned)D, (unsigned)c0, n, 0,
                       out_dev, stride, off);
    HIPCHK(hipGetLastError());
    if ((rc = apply_general(h, m, W, nullptr, X, 1.0, st, n_vec))) return rc;   // W2 = -H^2 X
    hipLaunchKernelGGL(k_gen_obs_trace, dim3(tblk, B), dim3(256), 0, st, (const cplx*)X, (unsigned)D, (unsigned)c0, n, 1,
                       out_dev, stride, off);
    HIPCHK(hipGetLastError());
    h->stats.n_launches += 3;
  }
  return RYD_OK;
}

// The scratch of the *_many calls, owned by the handle: [n_times] ObsManyTime - the (interval, offset) of every time, found
// on the host exactly as ryd_observe finds it and uploaded from a pinned copy - followed by `table_bytes` for the caller's
// coefficient table.  Grows on demand (the only host synchronisation); calls on one handle are ordered by using ONE
// stream, as with coefs_dev / wA of ryd_observe.
static int obs_many_stage_times(ryd_handle* h, int n_times, const double* times, size_t table_bytes, hipStream_t st,
                                ObsManyTime** tm_dev, void** table) {
  const size_t tm_bytes = ((size_t)n_times * sizeof(ObsManyTime) + 255) & ~(size_t)255;
  const size_t need = tm_bytes + table_bytes;
  if (need > h->obs_many_bytes) {
    HIPCHK(hipStreamSynchronize(st));  // (an earlier call on this stream may still read the old scratch)
    if (h->obs_many_dev) HIPCHK(hipFree(h->obs_many_dev));
    h->obs_many_dev = nullptr;
    h->obs_many_bytes = 0;
    HIPCHK(hipMalloc(&h->obs_many_dev, need));
    h->obs_many_bytes = need;
  }
  if (!h->obs_many_ev) HIPCHK(hipEventCreateWithFlags(&h->obs_many_ev, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(h->obs_many_ev));  // the last upload has left the pinned buffer
  if ((size_t)n_times > h->obs_many_pin_cap) {
    if (h->obs_many_pin) HIPCHK(hipHostFree(h->obs_many_pin));
    h->obs_many_pin = nullptr;
    h->obs_many_pin_cap = 0;
    HIPCHK(hipHostMalloc((void**)&h->obs_many_pin, (size_t)n_times * sizeof(ObsManyTime), hipHostMallocDefault));
    h->obs_many_pin_cap = (size_t)n_times;
  }
  for (int i = 0; i < n_times; ++i) {
    const MixPoint m = mix_at(h, times[i]);
    h->obs_many_pin[i] = {m.u1, m.idx1, 0};
  }
  *tm_dev = (ObsManyTime*)h->obs_many_dev;
  *table = (char*)h->obs_many_dev + tm_bytes;
  HIPCHK(hipMemcpyAsync(*tm_dev, h->obs_many_pin, (size_t)n_times * sizeof(ObsManyTime), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(h->obs_many_ev, st));
  return RYD_OK;
}

// the coefficient table [n_times][B][N][4] of k_eval_coefs_many in the handle's scratch: one upload, one launch
static int obs_many_coef_table(ryd_handle* h, int n_times, const double* times, hipStream_t st, double** table) {
  const int B = h->B, N = h->N;
  ObsManyTime* tm_dev = nullptr;
  int rc = obs_many_stage_times(h, n_times, times, (size_t)n_times * B * N * 4 * sizeof(double), st, &tm_dev, (void**)table);
  if (rc) return rc;
  const long long total = (long long)n_times * B * N;
  hipLaunchKernelGGL(k_eval_coefs_many, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const cplx*)h->pp_dev,
                     h->n_knots - 1, (const ryd_qdesc*)h->desc_dev, (const ObsManyTime*)tm_dev, B * N, total, *table);
  HIPCHK(hipGetLastError());
  h->stats.n_launches++;
  return RYD_OK;
}

// What the four *_many calls share once the handle is known to be theirs.  obs_many_front refuses the shapes (`who`
// opens every message; one state is a ket of D amplitudes or, with `dm`, a matrix of D * D elements; an Ising handle of
// batch B serves B states per time, or any number when B is 1), answers RYD_OK with n_states == 0 to a call without
// times, zeroes the output [n_states][N*N+N+3] on the caller's stream and settles the pair kernel's launch.  A
// general-path handle asked for the energy moments meets its two refusals here too, where they always stood: after the
// shapes when it has collapse operators, after the device is set when it lacks the padded site tables (built there).
struct ObsManyFront {
  hipStream_t st;
  int stride;          // N*N + N + 3 doubles per state
  long long n_states;  // n_times * n_batch
  unsigned gy;         // gridDim.y of every kernel: the states, grid-strided beyond 65535
  bool pairs;          // the pair kernel runs and brings the norm / trace; else the energy kernel of an energy-only call does
};

static int obs_many_front(ryd_handle* h, const char* who, bool dm, int64_t D, int N, int32_t n_times, int32_t n_batch,
                          int64_t stride_t, int64_t stride_b, const void* states_dev, const double* times, int32_t what,
                          double* out_dev, void* stream, ObsManyFront* f) {
  const bool gen_energy = h->general && (what & RYD_OBS_ENERGY);
  const int64_t elems = dm ? D * D : D;
  f->n_states = 0;
  if (n_times < 0 || n_batch < 1) return fail(RYD_ERR_INVALID, "%s: %d times, batch %d", who, n_times, n_batch);
  if (!h->general && h->B != n_batch && h->B != 1)
    return fail(RYD_ERR_INVALID, "%s: a handle of batch %d cannot observe %d states per time (its batch or 1)", who, h->B, n_batch);
  if (stride_t < elems || stride_b < elems)
    return fail(RYD_ERR_INVALID, "%s: strides %lld / %lld are smaller than a %s of %lld %s", who, (long long)stride_t,
                (long long)stride_b, dm ? "density matrix" : "ket", (long long)elems, dm ? "elements" : "amplitudes");
  if (gen_energy && h->gen_mc_term >= 0)
    return fail(RYD_ERR_UNSUPPORTED, "%s: energy moments need a handle without collapse operators (its generator is H_eff); ryd_general_observe says the same, ask for the pair sums only", who);
  if (n_times == 0) return RYD_OK;
  if (!states_dev || !times || !out_dev) return fail(RYD_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (gen_energy) {
    int rc;
    if (!h->gen_sites_valid && (rc = gen_build_sites(h))) return rc;
    if (!h->gen_fused_ok)
      return fail(RYD_ERR_UNSUPPORTED, "%s: energy moments need the padded site tables (k_gen_apply_fused); this handle applies its generator another way: use ryd_general_observe per time", who);
  }
  f->st = (hipStream_t)stream;
  f->stride = N * N + N + 3;
  f->n_states = (long long)n_times * n_batch;
  HIPCHK(hipMemsetAsync(out_dev, 0, (size_t)f->n_states * f->stride * sizeof(double), f->st));
  f->gy = (unsigned)std::min<long long>(f->n_states, 65535);
  f->pairs = (what & (RYD_OBS_OCCUPATION | RYD_OBS_CORRELATION)) || !(what & RYD_OBS_ENERGY);
  return RYD_OK;
}

// ryd_observe for every evaluation time of a run of a two-level Ising handle (the second half of k_observe.hpp): the kets
// of a sesolve run or, with `dm`, the density matrices of a master-equation run (ryd_observe + RYD_OBS_DENSITY).
// k_obs_pairs on the amplitudes / the diagonals, k_eval_coefs_many, k_obs_energy_many / k_obs_energy_dm_many.
static int ising_observe_many(ryd_handle* h, bool dm, const void* states_dev, int32_t n_times, int32_t n_batch,
                              int64_t stride_t, int64_t stride_b, const double* times, int32_t what, double* out_dev,
                              void* stream) {
  const char* who = dm ? "observe_density_many" : "observe_many";
  if (!h) return fail(RYD_ERR_INVALID, "null handle");
  if (h->general) return fail(RYD_ERR_INVALID, "%s: not available on a general-path handle", who);
  int rc = check_ready(h);
  if (rc) return rc;
  if (dm) {
    if (h->mc) return fail(RYD_ERR_UNSUPPORTED, "observe_density_many: Monte-Carlo handles are not served (use ryd_observe)");
  } else {
    if (h->cfg.mode != RYD_SESOLVE || h->mc)
      return fail(RYD_ERR_UNSUPPORTED, "observe_many: kets of a sesolve handle without collapse operators only");
    if (what & RYD_OBS_DENSITY) return fail(RYD_ERR_UNSUPPORTED, "observe_many: RYD_OBS_DENSITY is not served (use ryd_observe)");
  }
  if (!h->dterms_host.empty())
    return fail(RYD_ERR_UNSUPPORTED, "%s: handles with extra detuning terms are not served (use ryd_observe)", who);
  const int N = h->N;
  if (dm && 2 * N > RYD_MAX_QUBITS) return fail(RYD_ERR_INVALID, "2N exceeds %d", RYD_MAX_QUBITS);
  const int64_t D = (int64_t)1 << N;
  ObsManyFront f;
  rc = obs_many_front(h, who, dm, D, N, n_times, n_batch, stride_t, stride_b, states_dev, times, what, out_dev, stream, &f);
  if (rc || !f.n_states) return rc;
  if (f.pairs) {
    hipLaunchKernelGGL(k_obs_pairs, dim3((unsigned)((D + 2047) / 2048), f.gy), dim3(256), 0, f.st, (const cplx*)states_dev,
                       f.n_states, (int)n_batch, (long long)stride_t, (long long)stride_b, N, dm ? 1 : 0, (int)what, out_dev,
                       f.stride);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
  }
  if (!(what & RYD_OBS_ENERGY)) return RYD_OK;
  // the (interval, offset) of every time on the host, the table of every time in one launch
  double* table = nullptr;
  if ((rc = obs_many_coef_table(h, n_times, times, f.st, &table))) return rc;
  // kets: 2^kObsManyTB amplitudes per workgroup.  Matrices: a workgroup takes 32 rows at a time, 256 rows where there are that many
  const unsigned gx = dm ? (unsigned)std::min<int64_t>(std::max<int64_t>(D >> 8, 1), 1024)
                         : (unsigned)std::max<int64_t>(D >> kObsManyTB, 1);
  const auto energy_kernel = dm ? k_obs_energy_dm_many : k_obs_energy_many;  // (one argument list serves both)
  hipLaunchKernelGGL(energy_kernel, dim3(gx, f.gy), dim3(256), 0, f.st,
                     (const cplx*)states_dev, f.n_states, (int)n_batch, (long long)stride_t, (long long)stride_b, N,
                     (const double*)table, h->B, (const double*)h->e0_dev, h->e0_mats == 1 ? 0ll : (long long)D,
                     f.pairs ? 0 : 1, out_dev, f.stride);
  HIPCHK(hipGetLastError());
  h->stats.n_launches++;
  return RYD_OK;
}

extern "C" int ryd_observe_many(ryd_handle* h, const void* states_dev, int32_t n_times, int32_t n_batch,
                                int64_t stride_t, int64_t stride_b, const double* times, int32_t what,
                                double* out_dev, void* stream) {
  return ising_observe_many(h, false, states_dev, n_times, n_batch, stride_t, stride_b, times, what, out_dev, stream);
}

extern "C" int ryd_observe_density_many(ryd_handle* h, const void* states_dev, int32_t n_times, int32_t n_batch,
                                        int64_t stride_t, int64_t stride_b, const double* times, int32_t what,
                                        double* out_dev, void* stream) {
  return ising_observe_many(h, true, states_dev, n_times, n_batch, stride_t, stride_b, times, what, out_dev, stream);
}

// The energy moments of ryd_general_observe_many (kets, k_gen_obs_energy_many) and ryd_general_observe_density_many (`dm`:
// D x D matrices, k_gen_obs_energy_dm_many) after obs_many_front: per chunk of times one table launch and one energy launch.
static int gen_obs_many_energy(ryd_handle* h, bool dm, const ObsManyFront& f, int64_t D, int N, const void* states_dev,
                               int32_t n_times, int32_t n_batch, int64_t stride_t, int64_t stride_b, const double* times,
                               double* out_dev) {
  int rc;
  const hipStream_t st = f.st;
  const int stride = f.stride;
  // (interval, offset) of every time on the host; per time tcoef[n_terms] and mvals[E + Dg] in the handle's scratch (the
  // handle's own gen_tcoef / gen_fused.mvals / wA are not written).  Calls on one handle are ordered by using ONE stream.
  const GenFusedDev& F = h->gen_fused;
  const int n_terms = (int)h->gen_host.size();
  const size_t per_time = (size_t)(n_terms + F.E + F.Dg);
  size_t chunk = std::max<size_t>(kGenObsScratchCap / (per_time * sizeof(cplx)), 1);
  if (h->gen_obs_small_chunks) chunk = std::min<size_t>(chunk, 5);
  chunk = std::min<size_t>(chunk, (size_t)n_times);
  ObsManyTime* tm_dev = nullptr;
  cplx* table = nullptr;
  if ((rc = obs_many_stage_times(h, n_times, times, chunk * per_time * sizeof(cplx), st, &tm_dev, (void**)&table))) return rc;
  {
    static bool attr[64] = {};
    const int dev = h->cfg.device;
    if (dev < 0 || dev >= 64 || !attr[dev]) {
      HIPCHK(hipFuncSetAttribute((const void*)k_gen_obs_energy_many<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)k_gen_obs_energy_many<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)k_gen_obs_energy_dm_many, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      if (dev >= 0 && dev < 64) attr[dev] = true;
    }
  }
  GenObsManyArgs A;
  A.terms = h->gen_terms_dev;
  A.diag_terms = h->gen_diag_terms_dev;
  for (int k = 0; k < 4; ++k) {
    const bool have = k < h->gen_n_diag;
    A.diag_idx[k] = have ? h->gen_diag_host[k] : 0;
    A.diag_val[k] = have ? h->gen_host[h->gen_diag_host[k]].dev.val : nullptr;
  }
  A.F = F;
  A.stride_t = stride_t;
  A.stride_b = stride_b;
  A.dim = (long long)D;
  A.n_batch = n_batch;
  A.n_terms = n_terms;
  A.n_diag = h->gen_n_diag;
  A.d = h->gen_d;
  A.n_dig = h->gen_ndig;
  A.with_norm = f.pairs ? 0 : 1;
  A.out_stride = stride;
  A.off = N * N + N + 1;
  A.norm_off = N;
  A.table = table;
  // kets: the application's LDS image and a second buffer for the waves' partial sums (<= 150 KiB + 8 KiB of the CU's 160).
  // matrices: the tables, three partial sums of three waves, the row offsets (the application's image without the vector + 1 KiB)
  const size_t lds = dm ? (size_t)(F.E + F.Dg) * sizeof(cplx) + 3 * GEN_FUSED_ROWS * 3 * sizeof(cplx) +
                              (size_t)((F.E + 3) & ~3) * sizeof(int)
                        : h->gen_fused_lds + 4 * GEN_FUSED_ROWS * 2 * sizeof(cplx);
  const unsigned n_rb = (unsigned)((D + GEN_FUSED_ROWS - 1) / GEN_FUSED_ROWS);
  const unsigned gx = (n_rb + GEN_OBS_ROW_BLOCKS - 1) / GEN_OBS_ROW_BLOCKS;
  for (size_t t0 = 0; t0 < (size_t)n_times; t0 += chunk) {  // (one chunk unless the tables exceed kGenObsScratchCap)
    const size_t nt = std::min<size_t>(chunk, (size_t)n_times - t0);
    hipLaunchKernelGGL(k_gen_coefs_fused_many, dim3((unsigned)nt), dim3(256), 0, st, (const cplx*)h->pp_dev, h->n_knots - 1,
                       (const int*)h->gen_series_dev, (const int*)h->gen_conj_dev, (const cplx*)h->gen_scale_dev, n_terms,
                       (const ObsManyTime*)(tm_dev + t0), table, F);
    HIPCHK(hipGetLastError());
    A.states = (const cplx*)states_dev + (long long)t0 * stride_t;
    A.n_states = (long long)nt * n_batch;
    A.out = out_dev + t0 * (size_t)n_batch * stride;
    const dim3 grid(gx, (unsigned)std::min<long long>(A.n_states, 65535));
    if (dm) hipLaunchKernelGGL(k_gen_obs_energy_dm_many, grid, dim3(256), lds, st, A);
    else if (h->gen_fused_xlds) hipLaunchKernelGGL(k_gen_obs_energy_many<true>, grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL(k_gen_obs_energy_many<false>, grid, dim3(256), lds, st, A);
    HIPCHK(hipGetLastError());
    h->stats.n_launches += 2;
  }
  return RYD_OK;
}

// ryd_general_observe for every evaluation time of a run (kets of a general-path handle): k_gen_obs_pairs,
// k_gen_coefs_fused_many and k_gen_obs_energy_many (k_general.hpp)
extern "C" int ryd_general_observe_many(ryd_handle* h, const void* states_dev, int32_t n_times, int32_t n_batch,
                                        int64_t stride_t, int64_t stride_b, const double* times, int32_t what,
                                        int32_t local_dim, int32_t n_atoms, int32_t one_digit, double* out_dev,
                                        void* stream) {
  if (!h) return fail(RYD_ERR_INVALID, "null handle");
  if (!h->general) return fail(RYD_ERR_INVALID, "general observe_many: not a general-path handle: use ryd_observe_many");
  int rc = check_ready(h);
  if (rc) return rc;
  if (local_dim < 2 || local_dim > 4 || n_atoms < 1 || n_atoms > 26 || one_digit < 0 || one_digit >= local_dim)
    return fail(RYD_ERR_INVALID, "general observe_many: local_dim=%d n_atoms=%d one_digit=%d out of range", local_dim, n_atoms, one_digit);
  if (h->gen_density)
    return fail(RYD_ERR_UNSUPPORTED, "general observe_many: kets of a ket handle only; a RYD_GENERAL_DENSITY handle observes vec(rho) with ryd_general_observe");
  if (what & RYD_OBS_DENSITY)
    return fail(RYD_ERR_UNSUPPORTED, "general observe_many: RYD_OBS_DENSITY is not served (use ryd_general_observe)");
  int64_t D = 1;
  for (int i = 0; i < n_atoms; ++i) {
    D *= local_dim;
    if (D > ((int64_t)1 << 26)) return fail(RYD_ERR_INVALID, "general observe_many: %d^%d exceeds 2^26", local_dim, n_atoms);
  }
  if ((int64_t)h->dim != D)
    return fail(RYD_ERR_INVALID, "general observe_many: dim %lld is not %d^%d", (long long)h->dim, local_dim, n_atoms);
  const int N = n_atoms;
  ObsManyFront f;
  rc = obs_many_front(h, "general observe_many", false, D, N, n_times, n_batch, stride_t, stride_b, states_dev, times, what,
                      out_dev, stream, &f);
  if (rc || !f.n_states) return rc;
  if (f.pairs) {
    hipLaunchKernelGGL(k_gen_obs_pairs, dim3((unsigned)((D + 2047) / 2048), f.gy), dim3(256), 0, f.st,
                       (const cplx*)states_dev, f.n_states, (int)n_batch, (long long)stride_t, (long long)stride_b,
                       (unsigned)D, N, (int)local_dim, (int)one_digit, 0, (int)what, out_dev, f.stride);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
  }
  if (!(what & RYD_OBS_ENERGY)) return RYD_OK;
  return gen_obs_many_energy(h, false, f, D, N, states_dev, n_times, n_batch, stride_t, stride_b, times, out_dev);
}

// ryd_general_observe + RYD_OBS_DENSITY for every density matrix of a master-equation run on the general path:
// k_gen_obs_pairs on the diagonals, k_gen_coefs_fused_many and k_gen_obs_energy_dm_many (k_general.hpp)
extern "C" int ryd_general_observe_density_many(ryd_handle* h, const void* states_dev, int32_t n_times, int32_t n_batch,
                                                int64_t stride_t, int64_t stride_b, const double* times, int32_t what,
                                                int32_t local_dim, int32_t n_atoms, int32_t one_digit, double* out_dev,
                                                void* stream) {
  const char* who = "general observe_density_many";
  if (!h) return fail(RYD_ERR_INVALID, "%s: null handle", who);
  if (!h->general) return fail(RYD_ERR_INVALID, "%s: not a general-path handle: use ryd_observe_density_many", who);
  int rc = check_ready(h);
  if (rc) return rc;
  if (local_dim < 2 || local_dim > 4 || n_atoms < 1 || n_atoms > 26 || one_digit < 0 || one_digit >= local_dim)
    return fail(RYD_ERR_INVALID, "%s: local_dim=%d n_atoms=%d one_digit=%d out of range", who, local_dim, n_atoms, one_digit);
  if (h->gen_density)
    return fail(RYD_ERR_UNSUPPORTED, "%s: matrices on a ket handle only; a RYD_GENERAL_DENSITY handle observes vec(rho) with ryd_general_observe", who);
  int64_t D = 1;
  for (int i = 0; i < n_atoms; ++i) {
    D *= local_dim;
    if (D > ((int64_t)1 << 13))
      return fail(RYD_ERR_INVALID, "%s: a %d^%d x %d^%d density matrix exceeds 2^26 entries", who, local_dim, n_atoms, local_dim, n_atoms);
  }
  if ((int64_t)h->dim != D)
    return fail(RYD_ERR_INVALID, "%s: dim %lld is not %d^%d", who, (long long)h->dim, local_dim, n_atoms);
  const int N = n_atoms;
  what &= ~RYD_OBS_DENSITY;
  ObsManyFront f;
  rc = obs_many_front(h, who, true, D, N, n_times, n_batch, stride_t, stride_b, states_dev, times, what, out_dev, stream, &f);
  if (rc || !f.n_states) return rc;
  if (f.pairs) {
    hipLaunchKernelGGL(k_gen_obs_pairs, dim3((unsigned)((D + 2047) / 2048), f.gy), dim3(256), 0, f.st,
                       (const cplx*)states_dev, f.n_states, (int)n_batch, (long long)stride_t, (long long)stride_b,
                       (unsigned)D, N, (int)local_dim, (int)one_digit, 1, (int)what, out_dev, f.stride);
    HIPCHK(hipGetLastError());
    h->stats.n_launches++;
  }
  if (!(what & RYD_OBS_ENERGY)) return RYD_OK;
  return gen_obs_many_energy(h, true, f, D, N, states_dev, n_times, n_batch, stride_t, stride_b, times, out_dev);
}

extern "C" int ryd_ket_to_dm(ryd_handle* h, const void* psi_dev, void* rho_dev, void* stream) {
  if (!h || !psi_dev || !rho_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (h->general) return fail(RYD_ERR_INVALID, "not available on a general-path handle");
  if (2 * h->N > RYD_MAX_QUBITS) return fail(RYD_ERR_INVALID, "2N exceeds %d", RYD_MAX_QUBITS);
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t DD = (size_t)1 << (2 * h->N);
  dim3 grid((unsigned)((DD + 255) / 256), h->B);
  hipLaunchKernelGGL(k_ket_to_dm, grid, dim3(256), 0, (hipStream_t)stream, (const cplx*)psi_dev,
                     h->N, (cplx*)rho_dev);
  HIPCHK(hipGetLastError());
  return RYD_OK;
}

// acc[D][D] += sum_b w_b |psi_b><psi_b| for any state dimension: the fp64 matrix cores on 64 x 64
// upper-triangle tiles when D is a multiple of 64 (every two-level register of 6+ atoms, 4-level
// registers of 3+), one thread per entry otherwise.
static int outer_accumulate_impl(const void* psi_dev, int64_t B, int64_t D, const double* weights,
                                 void* acc_dev, hipStream_t st) {
  if (B <= 0 || D <= 0 || B > INT32_MAX) return fail(RYD_ERR_INVALID, "batch %lld, dim %lld", (long long)B, (long long)D);
  double* wdev = nullptr;
  if (weights) {
    HIPCHK(hipMalloc((void**)&wdev, B * sizeof(double)));
    hipError_t e = hipMemcpyAsync(wdev, weights, B * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { hipFree(wdev); return fail(RYD_ERR_HIP, "weights upload: %s", hipGetErrorString(e)); }
  }
  if (D % 64 == 0) {
    constexpr int KT = 16;
    const unsigned nt = (unsigned)(D / 64);
    hipLaunchKernelGGL(k_outer_mfma<KT>, dim3(nt, nt), dim3(256), 2 * KT * 128 * sizeof(double), st,
                       (const cplx*)psi_dev, (size_t)D, (int)B, wdev, (cplx*)acc_dev);
  } else {
    const size_t DD = (size_t)D * (size_t)D;
    hipLaunchKernelGGL(k_outer_acc, dim3((unsigned)((DD + 255) / 256)), dim3(256), 0, st,
                       (const cplx*)psi_dev, (size_t)D, (int)B, wdev, (cplx*)acc_dev);
  }
  hipError_t e = hipGetLastError();
  if (wdev) { hipStreamSynchronize(st); hipFree(wdev); }
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_outer_acc: %s", hipGetErrorString(e));
  return RYD_OK;
}

extern "C" int ryd_outer_accumulate(ryd_handle* h, const void* psi_dev, const double* weights,
                                    void* acc_dev, void* stream) {
  if (!h || !psi_dev || !acc_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (h->general) return fail(RYD_ERR_INVALID, "not available on a general-path handle");
  if (2 * h->N > RYD_MAX_QUBITS) return fail(RYD_ERR_INVALID, "2N exceeds %d", RYD_MAX_QUBITS);
  HIPCHK(hipSetDevice(h->cfg.device));
  return outer_accumulate_impl(psi_dev, h->B, (int64_t)1 << h->N, weights, acc_dev, (hipStream_t)stream);
}

extern "C" int ryd_outer_accumulate_dim(const void* psi_dev, int64_t batch, int64_t dim,
                                        const double* weights, void* acc_dev, int32_t device,
                                        void* stream) {
  if (!psi_dev || !acc_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (dim > ((int64_t)1 << (RYD_MAX_QUBITS / 2))) return fail(RYD_ERR_INVALID, "dim %lld too large", (long long)dim);
  HIPCHK(hipSetDevice(device));
  return outer_accumulate_impl(psi_dev, batch, dim, weights, acc_dev, (hipStream_t)stream);
}

// out[s] = <x_s| O |x_s> (kets) or Tr(O rho_s) for O given by its sorted non-zeros: k_expect.hpp
extern "C" int ryd_expect_sparse(const void* states_dev, int64_t n_states, int64_t stride, int64_t dim, int32_t density,
                                 const int32_t* rows_dev, const int32_t* cols_dev, const void* vals_dev, int64_t nnz,
                                 void* out_dev, int32_t device, void* stream) {
  if (n_states < 0 || nnz < 0) return fail(RYD_ERR_INVALID, "expect: %lld states, %lld non-zeros", (long long)n_states, (long long)nnz);
  if (nnz > INT32_MAX) return fail(RYD_ERR_INVALID, "expect: %lld non-zeros exceed 2^31 - 1", (long long)nnz);
  if (dim < 1 || dim > INT32_MAX) return fail(RYD_ERR_INVALID, "expect: dim %lld outside [1, 2^31 - 1]", (long long)dim);
  if (stride < (density ? dim * dim : dim))
    return fail(RYD_ERR_INVALID, "expect: stride %lld is smaller than a %s of dim %lld", (long long)stride,
                density ? "density matrix" : "ket", (long long)dim);
  if (n_states == 0) return RYD_OK;
  if (!out_dev) return fail(RYD_ERR_INVALID, "null argument");
  if (nnz > 0 && (!states_dev || !rows_dev || !cols_dev || !vals_dev)) return fail(RYD_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(out_dev, 0, (size_t)n_states * sizeof(cplx), st));
  if (nnz == 0) return RYD_OK;
  const int64_t n_tiles = (n_states + kExpectTile - 1) / kExpectTile;
  const dim3 grid((unsigned)((nnz + kExpectChunk - 1) / kExpectChunk), (unsigned)std::min<int64_t>(n_tiles, 65535));
  if (density)
    hipLaunchKernelGGL(k_expect_sparse<1>, grid, dim3(256), 0, st, (const cplx*)states_dev, (long long)n_states,
                       (long long)stride, (long long)dim, rows_dev, cols_dev, (const cplx*)vals_dev, (long long)nnz,
                       (double*)out_dev);
  else
    hipLaunchKernelGGL(k_expect_sparse<0>, grid, dim3(256), 0, st, (const cplx*)states_dev, (long long)n_states,
                       (long long)stride, (long long)dim, rows_dev, cols_dev, (const cplx*)vals_dev, (long long)nnz,
                       (double*)out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_expect_sparse: %s", hipGetErrorString(e));
  return RYD_OK;
}

// z[s][f] = <a_f|x_s>, Tr(A_f^dag rho_s) or <phi_f|rho_s|phi_f>, and the norm / trace of every state: k_overlap.hpp
extern "C" int ryd_overlap_many(const void* states_dev, int64_t n_states, int64_t stride, int64_t dim, int32_t density,
                                const void* targets_dev, int32_t n_targets, int32_t target_form, void* out_dev,
                                double* norm_dev, int32_t device, void* stream) {
  if (n_states < 0) return fail(RYD_ERR_INVALID, "overlap: n_states %lld is negative", (long long)n_states);
  if (n_targets < 0) return fail(RYD_ERR_INVALID, "overlap: n_targets %d is negative", (int)n_targets);
  // (dim * dim elements per matrix: 2^31 - 1 of them is already 32 GiB)
  if (dim < 1 || dim > (density ? 46340 : INT32_MAX))
    return fail(RYD_ERR_INVALID, "overlap: dim %lld outside [1, %d]", (long long)dim, density ? 46340 : INT32_MAX);
  if (target_form != 0 && target_form != 1) return fail(RYD_ERR_INVALID, "overlap: target_form %d is not 0 or 1", (int)target_form);
  if (target_form == 1 && !density)
    return fail(RYD_ERR_INVALID, "overlap: target_form 1 (|phi><phi| formed on the fly) needs density = 1");
  const int64_t len = density ? dim * dim : dim;
  if (stride < len)
    return fail(RYD_ERR_INVALID, "overlap: stride %lld is smaller than a %s of dim %lld", (long long)stride,
                density ? "density matrix" : "ket", (long long)dim);
  if (n_states == 0) return RYD_OK;
  if (!states_dev) return fail(RYD_ERR_INVALID, "overlap: states_dev is null");
  if (!norm_dev) return fail(RYD_ERR_INVALID, "overlap: norm_dev is null");
  if (n_targets > 0 && !targets_dev) return fail(RYD_ERR_INVALID, "overlap: targets_dev is null with %d targets", (int)n_targets);
  if (n_targets > 0 && !out_dev) return fail(RYD_ERR_INVALID, "overlap: out_dev is null with %d targets", (int)n_targets);
  const int64_t n_chunks = (len + kOverlapChunk - 1) / kOverlapChunk;
  const int tile = n_targets <= 1 ? 1 : kOverlapTile;  // a lone target (or none): a quarter of the weight registers
  const int64_t n_tiles = std::max<int64_t>(1, ((int64_t)n_targets + tile - 1) / tile);
  if (n_tiles > 65535) return fail(RYD_ERR_INVALID, "overlap: n_targets %d exceeds %d", (int)n_targets, 65535 * kOverlapTile);
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(norm_dev, 0, (size_t)n_states * sizeof(double), st));
  if (n_targets > 0) HIPCHK(hipMemsetAsync(out_dev, 0, (size_t)n_states * (size_t)n_targets * sizeof(cplx), st));
  // a workgroup keeps its weights in registers and walks every grid.z-th state: about 4 096 workgroups in all, so that
  // small states still fill the device and large ones amortise the weight loads over many states
  const int64_t per_state = n_chunks * n_tiles;
  const int64_t gz = std::min<int64_t>(std::min<int64_t>(n_states, 65535), std::max<int64_t>(1, 4096 / per_state));
  const dim3 grid((unsigned)n_chunks, (unsigned)n_tiles, (unsigned)gz);
#define RYD_OVERLAP_LAUNCH_T(FORM, TRACE, TILE)                                                                          \
  hipLaunchKernelGGL((k_overlap_many<FORM, TRACE, TILE>), grid, dim3(256), 0, st, (const cplx*)states_dev,               \
                     (long long)n_states, (long long)stride, (long long)dim, (long long)len, (const cplx*)targets_dev,   \
                     (int)n_targets, (double*)out_dev, norm_dev)
#define RYD_OVERLAP_LAUNCH(FORM, TRACE)                  \
  do {                                                   \
    if (tile == 1)                                       \
      RYD_OVERLAP_LAUNCH_T(FORM, TRACE, 1);              \
    else                                                 \
      RYD_OVERLAP_LAUNCH_T(FORM, TRACE, kOverlapTile);   \
  } while (0)
  if (!density)
    RYD_OVERLAP_LAUNCH(0, 0);
  else if (target_form)
    RYD_OVERLAP_LAUNCH(1, 1);
  else
    RYD_OVERLAP_LAUNCH(0, 1);
#undef RYD_OVERLAP_LAUNCH
#undef RYD_OVERLAP_LAUNCH_T
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_overlap_many: %s", hipGetErrorString(e));
  return RYD_OK;
}

extern "C" int ryd_accumulate(const void* x_dev, double weight, int64_t count, void* acc_dev,
                              int32_t device, void* stream) {
  if (!x_dev || !acc_dev || count <= 0) return fail(RYD_ERR_INVALID, "null argument or empty array");
  HIPCHK(hipSetDevice(device));
  const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 8192);
  hipLaunchKernelGGL(k_axpy, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const cplx*)x_dev, weight,
                     (size_t)count, (cplx*)acc_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_axpy: %s", hipGetErrorString(e));
  return RYD_OK;
}

extern "C" int ryd_get_stats(const ryd_handle* h, ryd_stats* out) {
  if (!h || !out) return fail(RYD_ERR_INVALID, "null argument");
  *out = h->stats;
  if (hermitian_path(h)) out->passes = 2;  // row pass + symmetrisation
  return RYD_OK;
}

// The kernel that the NEXT application of a general handle's generator runs with, from its site tables (a function of the
// terms and of ryd_set_path; built here if no call has needed them yet): what ryd_stats.reserved[3] reports after an
// application, asked before the first one - ryd_general_observe_many serves the energy moments of 2 and 3 only.
extern "C" int ryd_general_apply_path(ryd_handle* h, int32_t* path) {
  if (!h || !path) return fail(RYD_ERR_INVALID, "null argument");
  if (!h->general || h->gen_host.empty()) return fail(RYD_ERR_INVALID, "ryd_general_apply_path needs a general-path handle");
  if (!h->gen_sites_valid) {
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = gen_build_sites(h);
    if (rc) return rc;
  }
  *path = h->gen_fused_ok ? (h->gen_fused_xlds ? 3 : 2) : h->gen_sites_ok ? 1 : 0;
  return RYD_OK;
}

extern "C" int ryd_reset_stats(ryd_handle* h) {
  if (!h) return fail(RYD_ERR_INVALID, "null handle");
  const int passes = h->stats.passes;
  std::memset(&h->stats, 0, sizeof h->stats);
  h->stats.passes = passes;
  return RYD_OK;
}

extern "C" int ryd_set_kernel_timing(ryd_handle* h, int32_t enable) {
  if (!h) return fail(RYD_ERR_INVALID, "null handle");
  h->timing = enable != 0;
  if (enable) { h->timing_ms = 0; h->timing_launches = 0; }
  return RYD_OK;
}

extern "C" int ryd_get_kernel_timing(ryd_handle* h, double* total_ms, int64_t* launches) {
  if (!h || !total_ms || !launches) return fail(RYD_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  for (auto& ev : h->ev_used) {
    HIPCHK(hipEventSynchronize(ev.second));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
    h->timing_ms += ms;
    h->timing_launches++;
    h->ev_free.push_back(ev);
  }
  h->ev_used.clear();
  *total_ms = h->timing_ms;
  *launches = h->timing_launches;
  return RYD_OK;
}

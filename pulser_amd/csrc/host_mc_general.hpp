// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// Quantum-jump trajectories on the general path - host side (kernels: k_mc_general.hpp).  The decay of
// H_eff is a local term of the handle, so the CF4 stepper, its bounds and every apply kernel are the
// general path's own; this file adds the collapse operators, the jump state and the per-step hooks.
// ---------------------------------------------------------------------------
static void gen_free_term(GenTermHost& t) {
  hipFree((void*)t.dev.row_ptr);
  hipFree((void*)t.dev.col);
  hipFree((void*)t.dev.val);
  hipFree((void*)t.dev.strides);
  hipFree((void*)t.dev.shifts);
  hipFree((void*)t.dev.weights);
  hipFree((void*)t.dev.rstart);
  hipFree((void*)t.dev.ecol);
}

static int gen_mc_remove(ryd_handle* h) {
  if (h->gen_mc_term >= 0) {
    gen_free_term(h->gen_host[h->gen_mc_term]);
    h->gen_host.erase(h->gen_host.begin() + h->gen_mc_term);
    h->gen_mc_term = -1;
    if (!h->gen_host.empty()) {
      int rc = gen_publish_terms(h);
      if (rc) return rc;
    }
    h->bounds_valid = false;
    h->gen_sites_valid = false;
  }
  h->mc = false;
  h->mc_n_ops = 0;
  h->mcs.n_ops = 0;
  return RYD_OK;
}

extern "C" int ryd_general_set_collapse(ryd_handle* h, int32_t local_dim, int32_t n_atoms, int32_t n_ops,
                                        const double* ops) {
  if (local_dim < 2 || local_dim > MCG_MAX_D)
    return fail(RYD_ERR_INVALID, "local_dim=%d out of range [2, %d]", local_dim, MCG_MAX_D);
  if (n_ops < 0 || n_ops > MC_MAX_OPS || (n_ops > 0 && !ops))
    return fail(RYD_ERR_INVALID, "n_ops=%d out of range [0, %d]", n_ops, MC_MAX_OPS);
  if (n_atoms < 1 || n_atoms > 26) return fail(RYD_ERR_INVALID, "n_atoms=%d out of range [1, 26]", n_atoms);
  if (!h || !h->general) return fail(RYD_ERR_INVALID, "not a general-path handle");
  if (h->gen_density)
    return fail(RYD_ERR_INVALID, "collapse operators need a ket handle; this one evolves vec(rho)");
  {
    size_t v = 1;
    for (int i = 0; i < n_atoms; ++i) v *= (size_t)local_dim;
    if (v != h->dim)
      return fail(RYD_ERR_INVALID, "dim=%zu is not local_dim^n_atoms = %d^%d", h->dim, local_dim, n_atoms);
  }
  if (h->gen_d && h->gen_d != local_dim)
    return fail(RYD_ERR_INVALID, "local_dim=%d differs from the terms' %d", local_dim, h->gen_d);
  HIPCHK(hipSetDevice(h->cfg.device));
  int rc = gen_mc_remove(h);
  if (rc || n_ops == 0) return rc;
  const int D = local_dim, DD = D * D;
  // C_k, M_k = C_k^dag C_k, and their sum
  std::vector<std::complex<double>> C((size_t)n_ops * DD), Mk((size_t)n_ops * DD), S(DD);
  for (int k = 0; k < n_ops; ++k)
    for (int e = 0; e < DD; ++e) C[(size_t)k * DD + e] = {ops[2 * ((size_t)k * DD + e)], ops[2 * ((size_t)k * DD + e) + 1]};
  for (int k = 0; k < n_ops; ++k)
    for (int l = 0; l < D; ++l)
      for (int j = 0; j < D; ++j) {
        std::complex<double> m = 0.0;
        for (int i = 0; i < D; ++i) m += std::conj(C[(size_t)k * DD + i * D + l]) * C[(size_t)k * DD + i * D + j];
        Mk[(size_t)k * DD + l * D + j] = m;
        S[l * D + j] += m;
      }
  // the jump state, sized for (batch, atoms, D)
  const size_t B = (size_t)h->B, N = (size_t)n_atoms;
  if (h->mc_pool && (h->gen_mc_d != D || h->gen_mc_atoms != n_atoms)) {
    hipFree(h->mc_pool);
    h->mc_pool = nullptr;
  }
  if (!h->mc_pool) {
    const size_t n_dbl = 2 * B + 2 * (size_t)DD * N * B + 4 * B;
    const size_t bytes = 2 * MC_MAX_OPS * (size_t)DD * sizeof(cplx) + n_dbl * sizeof(double) +
                         B * sizeof(unsigned long long) + 3 * B * sizeof(int);
    HIPCHK(hipMalloc(&h->mc_pool, bytes));
    HIPCHK(hipMemset(h->mc_pool, 0, bytes));
    char* p = (char*)h->mc_pool;  // 16-byte objects first, then 8-byte, then 4-byte ones
    h->mc_ops_dev = (cplx*)p;     p += 2 * MC_MAX_OPS * (size_t)DD * sizeof(cplx);
    h->mcs.norm2 = (double*)p;    p += 2 * B * sizeof(double);
    h->mcs.red = (double*)p;      p += 2 * (size_t)DD * N * B * sizeof(double);
    h->mcs.target = (double*)p;   p += B * sizeof(double);
    h->mcs.refnorm = (double*)p;  p += B * sizeof(double);
    h->mcs.lastnorm = (double*)p; p += B * sizeof(double);
    h->mcs.scale = (double*)p;    p += B * sizeof(double);
    h->mc_seeds_dev = (unsigned long long*)p; p += B * sizeof(unsigned long long);
    h->mcs.flag = (int*)p;        p += B * sizeof(int);
    h->mcs.sel = (int*)p;         p += B * sizeof(int);
    h->mcs.count = (int*)p;
    h->mcs.seeds = h->mc_seeds_dev;
    h->mcs.ops = h->mc_ops_dev;
    h->gen_mc_d = D;
    h->gen_mc_atoms = n_atoms;
  }
  std::vector<cplx> tab(2 * MC_MAX_OPS * (size_t)DD, make_double2(0.0, 0.0));
  for (int k = 0; k < n_ops; ++k)
    for (int e = 0; e < DD; ++e) {
      const std::complex<double> c = C[(size_t)k * DD + e], m = Mk[(size_t)k * DD + e];
      tab[(size_t)k * DD + e] = make_double2(c.real(), c.imag());
      tab[(size_t)(MC_MAX_OPS + k) * DD + e] = make_double2(m.real(), m.imag());
    }
  HIPCHK(hipMemcpy(h->mc_ops_dev, tab.data(), tab.size() * sizeof(cplx), hipMemcpyHostToDevice));
  // -(1/2) sum_k C_k^dag C_k on every atom: one static local term of the generator
  std::vector<int32_t> rows, cols;
  std::vector<double> vals;
  double rmax = 0.0;
  for (int r = 0; r < D; ++r) {
    double rs = 0.0;
    for (int c = 0; c < D; ++c) {
      const std::complex<double> v = -0.5 * S[r * D + c];
      if (v == std::complex<double>(0.0)) continue;
      rows.push_back(r);
      cols.push_back(c);
      vals.push_back(v.real());
      vals.push_back(v.imag());
      rs += std::abs(v);
    }
    rmax = std::max(rmax, rs);
  }
  if (!h->gen_d) {  // digits of the vector index for the jump kernels (CSR-only handles)
    h->gen_d = D;
    h->gen_ndig = n_atoms;
  }
  if (!rows.empty()) {
    std::vector<int64_t> strides(N);
    std::vector<double> weights(N, 1.0);
    int64_t s = 1;
    for (int a = n_atoms - 1; a >= 0; --a) { strides[a] = s; s *= D; }
    rc = ryd_general_add_local_term(h, D, 1, n_atoms, strides.data(), weights.data(), (int32_t)rows.size(),
                                    rows.data(), cols.data(), vals.data(), -1, 0, 1.0, 0.0, n_atoms * rmax);
    if (rc) return rc;
    h->gen_mc_term = (int)h->gen_host.size() - 1;
  }
  h->mcs.n_ops = n_ops;
  h->mc_n_ops = n_ops;
  h->mc = true;
  return RYD_OK;
}

// the launches of one step's bookkeeping; D a template argument of the kernels
template <int D>
static void mcg_launch_step(ryd_handle* h, cplx* state, hipStream_t st) {
  const unsigned nblk = mc_blocks(h);
  const int N = h->gen_mc_atoms;
  hipLaunchKernelGGL(k_mcg_norm, dim3(nblk, h->B), dim3(256), 0, st, state, (long long)h->dim, h->mcs.norm2);
  hipLaunchKernelGGL(k_mcg_reduced<D>, dim3(nblk, h->B, N), dim3(256), 0, st, state, (long long)h->dim, N, h->mcs, h->B);
  hipLaunchKernelGGL(k_mcg_select<D>, dim3((h->B + 127) / 128), dim3(128), 0, st, h->mcs, h->B, N);
  hipLaunchKernelGGL(k_mcg_jump<D>, dim3(nblk, h->B), dim3(256), 0, st, state, (long long)h->dim, N, h->mcs);
}

static int mc_after_step_general(ryd_handle* h, cplx* state, hipStream_t st) {
  switch (h->gen_mc_d) {
    case 2: mcg_launch_step<2>(h, state, st); break;
    case 3: mcg_launch_step<3>(h, state, st); break;
    case 4: mcg_launch_step<4>(h, state, st); break;
    default: return fail(RYD_ERR_STATE, "no collapse operators on this handle");
  }
  HIPCHK(hipGetLastError());
  h->stats.n_launches += 4;
  return RYD_OK;
}

// The persistent kernel keeps systems whose application is cheaper than a launch (use_persistent_general's
// rule), now for any batch: one workgroup per trajectory.
static bool use_persistent_general_mc(const ryd_handle* h) {
  if (!(h->dim <= 4096 && !h->force_generic && !h->gen_host.empty())) return false;
  const double rows = std::max(1.0, (double)h->dim / 1024.0);
  double groups = 0.0;
  for (const GenTermHost& t : h->gen_host) groups += t.dev.kind == 1 ? (double)t.dev.n_groups : 1.0;
  return groups * rows <= 13.0;
}

static int gen_mc_launch(ryd_handle* h0, const std::vector<GenMcTrajArgs>& args, int D, hipStream_t st) {
  const size_t n = args.size();
  if (h0->gen_mc_args_cap < n) {
    if (h0->gen_mc_args_dev) hipFree(h0->gen_mc_args_dev);
    h0->gen_mc_args_dev = nullptr;
    h0->gen_mc_args_cap = 0;
    HIPCHK(hipMalloc(&h0->gen_mc_args_dev, n * sizeof(GenMcTrajArgs)));
    h0->gen_mc_args_cap = n;
  }
  HIPCHK(hipStreamSynchronize(st));  // an earlier launch may still read the argument table
  HIPCHK(hipMemcpyAsync(h0->gen_mc_args_dev, args.data(), n * sizeof(GenMcTrajArgs), hipMemcpyHostToDevice, st));
  const size_t lds = 2 * 4096 * sizeof(cplx) + 2 * MAX_GEN_TERMS * sizeof(cplx) + GEN_MC_LDS;
  static bool attr_set[64] = {};
  const int dev = h0->cfg.device;
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    HIPCHK(hipFuncSetAttribute((const void*)k_gen_traj_mc<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void*)k_gen_traj_mc<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void*)k_gen_traj_mc<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const GenMcTrajArgs* a = (const GenMcTrajArgs*)h0->gen_mc_args_dev;
  switch (D) {
    case 2: hipLaunchKernelGGL(k_gen_traj_mc<2>, dim3((unsigned)n), dim3(1024), lds, st, a); break;
    case 3: hipLaunchKernelGGL(k_gen_traj_mc<3>, dim3((unsigned)n), dim3(1024), lds, st, a); break;
    case 4: hipLaunchKernelGGL(k_gen_traj_mc<4>, dim3((unsigned)n), dim3(1024), lds, st, a); break;
    default: return fail(RYD_ERR_STATE, "no collapse operators on this handle");
  }
  HIPCHK(hipGetLastError());
  h0->stats.n_launches++;
  return RYD_OK;
}

// every trajectory of a batched handle in one launch; the jump state continues from the handle's McState
static int run_persistent_general_mc(ryd_handle* h, cplx* state, const std::vector<StepDesc>& sched, cplx* snaps,
                                     hipStream_t st) {
  if (sched.empty()) return RYD_OK;
  GenTrajArgs g;
  std::memset(&g, 0, sizeof g);
  int rc = fill_gen_traj_args(h, state, sched, snaps, st, g);
  if (rc) return rc;
  const std::vector<unsigned long long>& seeds = h->gen_mc_seeds;
  std::vector<GenMcTrajArgs> args(h->B);
  for (int b = 0; b < h->B; ++b) {
    GenMcTrajArgs& a = args[b];
    std::memset(&a, 0, sizeof a);
    a.g = g;
    a.g.state = state + (size_t)b * h->dim;
    a.g.snaps = snaps ? snaps + (size_t)b * h->dim : nullptr;
    a.mc = h->mcs;
    a.snap_stride = (long long)h->dim * h->B;
    a.seed = seeds[b];
    a.b = b;
    a.n_atoms = h->gen_mc_atoms;
    a.init = 0;
  }
  if ((rc = gen_mc_launch(h, args, h->gen_mc_d, st))) return rc;
  for (const StepDesc& d : sched) {
    h->stats.n_applications += d.order_a + d.order_b;
    h->stats.n_steps++;
  }
  return RYD_OK;
}

extern "C" int ryd_general_mc_solve(ryd_handle* h, void* state_dev, int32_t n_times, const double* times,
                                    void* out_dev, const uint64_t* seeds, const ryd_opts* opts, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!h->general) return fail(RYD_ERR_INVALID, "not a general-path handle");
  if (!h->mc) return fail(RYD_ERR_STATE, "ryd_general_set_collapse has not been called");
  if (!state_dev || !seeds) return fail(RYD_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  h->gen_mc_seeds.assign(seeds, seeds + h->B);  // (the persistent kernel takes them by argument)
  HIPCHK(hipMemcpyAsync(h->mc_seeds_dev, h->gen_mc_seeds.data(), (size_t)h->B * sizeof(unsigned long long),
                        hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(h->mcs.norm2, 0, 2 * (size_t)h->B * sizeof(double), st));
  hipLaunchKernelGGL(k_mcg_norm, dim3(mc_blocks(h), h->B), dim3(256), 0, st, (const cplx*)state_dev,
                     (long long)h->dim, h->mcs.norm2);
  hipLaunchKernelGGL(k_mcg_init, dim3((h->B + 127) / 128), dim3(128), 0, st, h->mcs, h->B,
                     2 * h->gen_mc_d * h->gen_mc_d * h->gen_mc_atoms);
  HIPCHK(hipGetLastError());
  h->mc_active = true;
  rc = ryd_solve(h, state_dev, n_times, times, out_dev, opts, stream);
  if (rc == RYD_OK) rc = snapshot_copy(h, (const cplx*)state_dev, (cplx*)state_dev, st);
  h->mc_active = false;
  return rc;
}

extern "C" int ryd_general_mc_solve_many(ryd_handle** hs, int32_t n, void* const* states_dev, int32_t n_times,
                                         const double* times, void* const* outs_dev, const uint64_t* seeds,
                                         const ryd_opts* opts, void* stream) {
  if (!hs || n < 1 || !states_dev || !times || !seeds || n_times < 2)
    return fail(RYD_ERR_INVALID, "null argument / no problems");
  for (int i = 1; i < n_times; ++i)
    if (!(times[i] > times[i - 1])) return fail(RYD_ERR_INVALID, "times must be strictly increasing");
  ryd_opts o;
  std::memset(&o, 0, sizeof o);
  if (opts) o = *opts;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  for (int b = 0; b < n; ++b) {
    ryd_handle* h = hs[b];
    if ((rc = check_ready(h))) return rc;
    if (!h->general || h->B != 1 || h->dim > 4096 || h->gen_host.empty())
      return fail(RYD_ERR_UNSUPPORTED, "problem %d: ryd_general_mc_solve_many takes general handles of one state "
                  "with at most 4096 entries", b);
    if (!h->mc) return fail(RYD_ERR_STATE, "problem %d: ryd_general_set_collapse has not been called", b);
    if (h->gen_mc_d != hs[0]->gen_mc_d)
      return fail(RYD_ERR_INVALID, "problem %d: local dimension %d differs from problem 0's %d", b, h->gen_mc_d,
                  hs[0]->gen_mc_d);
    if (h->cfg.device != hs[0]->cfg.device) return fail(RYD_ERR_INVALID, "problem %d lives on another device", b);
    if (!states_dev[b]) return fail(RYD_ERR_INVALID, "problem %d: null state", b);
  }
  HIPCHK(hipSetDevice(hs[0]->cfg.device));
  std::vector<GenMcTrajArgs> args(n);
  for (int b = 0; b < n; ++b) {
    ryd_handle* h = hs[b];
    if (!h->bounds_valid) compute_bounds_general(h);
    std::vector<StepDesc> sched;
    for (int i = 1; i < n_times; ++i) {
      build_schedule(h, times[i - 1], times[i], o, sched, false, kMergeMax);
      if (outs_dev && outs_dev[b]) sched.back().snap = i - 1;
    }
    GenMcTrajArgs& a = args[b];
    std::memset(&a, 0, sizeof a);
    if ((rc = fill_gen_traj_args(h, (cplx*)states_dev[b], sched, outs_dev ? (cplx*)outs_dev[b] : nullptr, st, a.g)))
      return rc;
    a.mc = h->mcs;
    a.snap_stride = (long long)h->dim;
    a.seed = seeds[b];
    a.b = 0;
    a.n_atoms = h->gen_mc_atoms;
    a.init = 1;
    for (const StepDesc& d : sched) {
      h->stats.n_applications += d.order_a + d.order_b;
      h->stats.n_steps++;
    }
  }
  return gen_mc_launch(hs[0], args, hs[0]->gen_mc_d, st);
}

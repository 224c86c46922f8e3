// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// Register-resident ket path (k_ket) and the split-operator master equation
// ---------------------------------------------------------------------------
// sesolve, N = 13/14, every drive coefficient real: one workgroup per sequence,
// the whole schedule in one launch (k_ket).
//
// mesolve, N = 12..14, dissipators without double flips (dephasing-type, i.e. the
// Lindbladian is  -i[H, .] + (real elementwise diagonal)  in the |a><b| basis):
//
//     rho(t + tau) = D(tau/2) . U ( D(tau/2) . rho ) U^dagger  + O(tau^3)        (Strang)
//
// with D(s)[a,b] = exp(s * d(a,b)) elementwise and U the unitary propagator of
// H(t) over tau = K CF4 steps.  U rho U^dagger is two passes of the SAME ket kernel
// over the 2^N rows (each row is a ket that is right-multiplied by U^dagger) with a
// conjugate transposition between them:  X = rho U^dagger;  Y = X^dagger = U rho;
// Y U^dagger = U rho U^dagger.  The result is Hermitian again, so there is no
// transposition back.  Per block of K steps the density matrix crosses HBM three
// times (96 B per element) instead of 72 B per element per generator application
// (22 applications per ns at 14 atoms): the path is bound by the fp64 vector pipe,
// not by HBM.  Splitting error measured against the tight oracle (6-atom
// triangular register, 3.1 us anneal, tests/probes/split_probe.py): K = 1/2/4/8 ns ->
// 6e-10 / 5e-10 / 1.2e-9 / 8.7e-9 at gamma = 0.05; it grows with gamma K^2, so K
// is chosen from the dissipator rate.

static bool ket_path(const ryd_handle* h) {
  if (h->general || h->cfg.mode != RYD_SESOLVE || h->mc || h->no_ket) return false;
  // complex drives: gauged away inside the kernel (KET_GAUGE) when no drive passes close to zero while its
  // phase turns (compute_bounds: gauge_ok)
  if (!h->drive_real && !h->gauge_ok) return false;
  if (h->force_ket) return h->N >= 10 && h->N <= 14;
  // <= 13 atoms: the LDS-resident kernel k_traj.  One workgroup evolves one sequence on ONE CU
  // (10 us per stage), so a handful of sequences is faster on the multi-launch tiled kernels that
  // spread each ket over the chip (measured, full 3.1 us anneal: 1 sequence 9.5 vs 6.9 sim-us/s;
  // 8 sequences 48 vs 55; 16 sequences 81 vs 111)
  // 13 atoms, 256 sequences: 2 950 sim-us/s here vs 1 280 on k_traj<13> (which spills); 12 atoms: equal
  return (h->N == 13 || h->N == 14) && h->B >= 8 && !h->force_generic;
}

static bool row_path(const ryd_handle* h) {
  if (h->general || h->cfg.mode != RYD_MESOLVE || h->N > 14) return false;
  // measured against the multi-launch Lindbladian (Hermitian path), ms per simulated ns, dephasing:
  // 10 atoms 0.10 vs 0.41, 11: 0.32 vs 1.08, 12: 1.40 vs 5.41, 13: 5.85 vs 20.7, 14: 23.7 vs 89
  if (h->N < 10) return false;
  if (!h->drive_real || (h->force_generic && !h->force_ket) || h->no_ket || !h->auto_tile) return false;
  if (h->has_dbl) return true;  // dissipator factor by k_local_exp (any complex 4x4 with this sparsity)
  for (int k = 0; k < 4; ++k)
    if (h->Sd[k].y != 0.0) return false;  // the elementwise factor must be real
  return true;
}

// spectral bound / shift of  w1 H(t1) + w2 H(t2)  as a KET generator (also for mesolve
// handles, whose rows are kets)
static void ket_bound(const ryd_handle* h, int idx, double w1, double w2, double* bound, double* shift,
                      int span = 1) {
  const double wmix = w1 + w2;
  const double drive = wmix * span_max(h->bd_drive, idx, span);
  const double dpos = wmix * span_max(h->bd_pos, idx, span), dneg = wmix * span_max(h->bd_neg, idx, span);
  double lo = wmix * h->e0_min - dpos, hi = wmix * h->e0_max + dneg;
  if (!h->drive_real && h->cfg.mode == RYD_SESOLVE) {
    // KET_GAUGE: the detunings carry theta' = d/dt arg c_k of the complex drives (sum over atoms of the
    // bounds of either sign, with the margin of compute_bounds)
    lo -= wmix * span_max(h->bd_gpos, idx, span);
    hi += wmix * span_max(h->bd_gneg, idx, span);
  }
  *shift = 0.5 * (lo + hi);
  *bound = 0.5 * (hi - lo) + drive;
}

// cheapest (scheme, sub-exponentials) whose fitted interval covers x = h ||H~|| / nsub
static int pick_scheme(double x, double tol, short* sch, short* nsub) {
  int best = -1, best_n = 0;
  double best_cost = 0.0;
  for (int n = 1; n <= 64; ++n) {
    for (int s = 0; s < kNumSymp; ++s) {
      if (kSymp[s].X < x / n || kSymp[s].err > tol) continue;
      const double cost = (double)n * kSymp[s].m + 0.5;  // + the closing half-stage
      if (best < 0 || cost < best_cost) { best = s; best_n = n; best_cost = cost; }
    }
    if (best >= 0 && n >= best_n + 2) break;
  }
  if (best < 0) {
    // tighter than any fitted scheme: the most accurate one that covers the argument (the table
    // bottoms out at a few 1e-13 per exponential), sub-divided until its interval fits
    for (int n = 1; n <= 4096 && best < 0; n *= 2)
      for (int s = 0; s < kNumSymp; ++s)
        if (kSymp[s].X >= x / n && (best < 0 || kSymp[s].err < kSymp[best].err)) { best = s; best_n = n; }
    if (best < 0) return fail(RYD_ERR_INVALID, "no in-place exponential scheme covers x = %g", x);
  }
  *sch = (short)best;
  *nsub = (short)best_n;
  return RYD_OK;
}

// the default per-exponential accuracy of the in-place schemes.  Their error is attained (not a
// worst-case bound like the Taylor remainder), so the default is a decade tighter than kDefaultTol.
static const double kDefaultSympTol = 2e-11;

static int to_ket_steps(ryd_handle* h, const std::vector<StepDesc>& sched, const ryd_opts& o,
                        double conj_sign, std::vector<KetStep>& out) {
  const double tol = o.tol > 0 ? o.tol : kDefaultSympTol * budget_scale(h);
  int rc;
  double phase = 0.0;  // accumulated spectral shifts: a global phase, applied at snapshots / final stores
  for (const StepDesc& d : sched) {
    KetStep k;
    std::memset(&k, 0, sizeof k);
    k.h = d.h; k.u1 = d.u1; k.u2 = d.u2; k.idx = d.idx; k.snap = d.snap;
    double ba, bb;
    ket_bound(h, d.idx, kA1, kA2, &ba, &k.shift_a, d.pad);
    ket_bound(h, d.idx, kA2, kA1, &bb, &k.shift_b, d.pad);
    if ((rc = pick_scheme(std::fabs(d.h) * ba, tol, &k.sch_a, &k.sub_a))) return rc;
    if ((rc = pick_scheme(std::fabs(d.h) * bb, tol, &k.sch_b, &k.sub_b))) return rc;
    phase += conj_sign * d.h * (k.shift_a + k.shift_b);
    k.cum_phase = phase;
    k.cum_cs = std::cos(phase);
    k.cum_sn = std::sin(phase);
    h->stats.last_order = kSymp[k.sch_a].m * k.sub_a;
    h->stats.norm_bound = ba / (kA1 + kA2);
    out.push_back(k);
  }
  return RYD_OK;
}

static int upload_ket_steps(ryd_handle* h, const std::vector<KetStep>& ks, hipStream_t st) {
  static_assert(sizeof(KetStep) <= 2 * sizeof(StepDesc), "schedule buffer sizing");
  const size_t bytes = ks.size() * sizeof(KetStep);
  if (h->ksched_cap < ks.size()) {
    if (h->ksched_dev) hipFree(h->ksched_dev);
    h->ksched_dev = nullptr;
    h->ksched_cap = 0;
    HIPCHK(hipMalloc((void**)&h->ksched_dev, bytes * 2));
    h->ksched_cap = ks.size() * 2;
  }
  HIPCHK(hipStreamSynchronize(st));  // the buffer may still be read by an earlier launch
  HIPCHK(hipMemcpyAsync(h->ksched_dev, ks.data(), bytes, hipMemcpyHostToDevice, st));
  return RYD_OK;
}

template <int MODE>
static int ket_set_lds_limit() {
  HIPCHK(hipFuncSetAttribute((const void*)k_ket<10, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)k_ket<11, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)k_ket<12, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)k_ket<13, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void*)k_ket<14, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return RYD_OK;
}

static int ket_init_device(ryd_handle* h) {
  static bool done[64] = {};
  const int dev = h->cfg.device;
  if (dev >= 0 && dev < 64 && done[dev]) return RYD_OK;
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(kSympDev), kSymp, sizeof(kSymp)));
  int rc;
  if ((rc = ket_set_lds_limit<KET_PLAIN>()) || (rc = ket_set_lds_limit<KET_ROWS>()) ||
      (rc = ket_set_lds_limit<KET_GAUGE>()))
    return rc;
  if (dev >= 0 && dev < 64) done[dev] = true;
  return RYD_OK;
}

template <int MODE>
static int launch_ket_mode(ryd_handle* h, const KetArgs& A, size_t n_rows, size_t lds, hipStream_t st) {
  switch (h->N) {
    case 10: hipLaunchKernelGGL((k_ket<10, MODE>), dim3((unsigned)n_rows), dim3(512), lds, st, A); break;
    case 11: hipLaunchKernelGGL((k_ket<11, MODE>), dim3((unsigned)n_rows), dim3(512), lds, st, A); break;
    case 12: hipLaunchKernelGGL((k_ket<12, MODE>), dim3((unsigned)n_rows), dim3(512), lds, st, A); break;
    case 13: hipLaunchKernelGGL((k_ket<13, MODE>), dim3((unsigned)n_rows), dim3(512), lds, st, A); break;
    case 14: hipLaunchKernelGGL((k_ket<14, MODE>), dim3((unsigned)n_rows), dim3(512), lds, st, A); break;
    default: return fail(RYD_ERR_INVALID, "k_ket needs 10 <= N <= 14");
  }
  return RYD_OK;
}

static int launch_ket(ryd_handle* h, const KetArgs& A, size_t n_rows, hipStream_t st, int mode = KET_PLAIN) {
  const size_t D = (size_t)1 << h->N;
  const size_t R = D / 512;
  const size_t lds = D * sizeof(double) + (64 + 64 + 2 * R + 32 + 128 + R + 64 + 32 + 2 * R) * sizeof(double);
  std::pair<hipEvent_t, hipEvent_t> ev;
  int rc;
  if (h->timing) { if ((rc = timing_begin(h, st, ev))) return rc; }
  rc = mode == KET_ROWS ? launch_ket_mode<KET_ROWS>(h, A, n_rows, lds, st)
       : mode == KET_GAUGE ? launch_ket_mode<KET_GAUGE>(h, A, n_rows, lds, st)
                           : launch_ket_mode<KET_PLAIN>(h, A, n_rows, lds, st);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  if (h->timing) { HIPCHK(hipEventRecord(ev.second, st)); h->ev_used.push_back(ev); }
  h->stats.n_launches++;
  return RYD_OK;
}

static void fill_ket_args(const ryd_handle* h, KetArgs& A) {
  std::memset(&A, 0, sizeof A);
  A.pp = h->pp_dev;
  A.desc = h->desc_dev;
  A.dterms = h->dterms_dev;
  A.e0 = h->e0_dev;
  A.e0_stride = h->e0_mats == 1 ? 0 : ((long long)1 << h->N);
  A.n_int = h->n_knots - 1;
  A.a1 = kA1;
  A.a2 = kA2;
  A.conj_sign = 1.0;
  A.fin_cs = 1.0;
}

static void count_ket_work(ryd_handle* h, const std::vector<KetStep>& ks, size_t i0, size_t i1, int passes) {
  for (size_t i = i0; i < i1; ++i) {
    // m stages = m generator applications (+ the closing half-stage)
    h->stats.n_applications += (int64_t)passes * (kSymp[ks[i].sch_a].m * ks[i].sub_a + kSymp[ks[i].sch_b].m * ks[i].sub_b + 1);
  }
}

// sesolve: one launch for the whole schedule, one workgroup per sequence
static int run_ket(ryd_handle* h, cplx* state, const std::vector<StepDesc>& sched, cplx* snaps,
                   const ryd_opts& o, hipStream_t st) {
  if (sched.empty()) return RYD_OK;
  int rc;
  if ((rc = ket_init_device(h))) return rc;
  std::vector<KetStep> ks;
  if ((rc = to_ket_steps(h, sched, o, 1.0, ks))) return rc;
  if ((rc = upload_ket_steps(h, ks, st))) return rc;
  KetArgs A;
  fill_ket_args(h, A);
  A.state = state;
  A.snaps = snaps;
  A.snap_map = h->snap_map_dev;
  A.snap_map_slots = h->snap_map_slots;
  A.steps = h->ksched_dev;
  A.n_steps = (int)ks.size();
  A.rows_log2 = 0;
  A.fin_cs = ks.back().cum_cs;
  A.fin_sn = ks.back().cum_sn;
  A.gauge_eps2 = h->gauge_eps2;
  if ((rc = launch_ket(h, A, (size_t)h->B, st, h->drive_real ? KET_PLAIN : KET_GAUGE))) return rc;
  count_ket_work(h, ks, 0, ks.size(), 1);
  h->stats.n_steps += (int64_t)ks.size();
  return RYD_OK;
}

// exp(f S) of the local 4x4 superoperator (diagonal + double-flip entries): 00 <-> 11 and 01 <-> 10
// are independent 2x2 blocks; scaling-and-squaring Taylor series on each.
static void local_super_exp(const ryd_handle* h, double f, cplx Mdiag[4], cplx Mflip[4]) {
  typedef std::complex<double> cd;
  for (int blk = 0; blk < 2; ++blk) {
    const int r0 = blk == 0 ? 0 : 1, r1 = 3 - r0;
    cd a[2][2] = {{cd(h->Sd[r0].x, h->Sd[r0].y) * f, cd(h->J[r0].x, h->J[r0].y) * f},
                  {cd(h->J[r1].x, h->J[r1].y) * f, cd(h->Sd[r1].x, h->Sd[r1].y) * f}};
    double nrm = 0.0;
    for (auto& row : a) for (auto& v : row) nrm = std::max(nrm, std::abs(v));
    int sq = 0;
    while (nrm > 0.25) { nrm *= 0.5; ++sq; }
    const double sc = std::ldexp(1.0, -sq);
    for (auto& row : a) for (auto& v : row) v *= sc;
    cd e[2][2] = {{1.0, 0.0}, {0.0, 1.0}}, term[2][2] = {{1.0, 0.0}, {0.0, 1.0}};
    for (int k = 1; k <= 18; ++k) {
      cd nt[2][2];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) nt[i][j] = (term[i][0] * a[0][j] + term[i][1] * a[1][j]) / (double)k;
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) { term[i][j] = nt[i][j]; e[i][j] += nt[i][j]; }
    }
    for (int s = 0; s < sq; ++s) {
      cd n2[2][2];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) n2[i][j] = e[i][0] * e[0][j] + e[i][1] * e[1][j];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) e[i][j] = n2[i][j];
    }
    Mdiag[r0] = make_double2(e[0][0].real(), e[0][0].imag());
    Mflip[r0] = make_double2(e[0][1].real(), e[0][1].imag());
    Mflip[r1] = make_double2(e[1][0].real(), e[1][0].imag());
    Mdiag[r1] = make_double2(e[1][1].real(), e[1][1].imag());
  }
}

// rho <- exp(f * dissipator) rho by the pair passes (k_local_exp), in place
static int launch_local_exp(ryd_handle* h, cplx* rho, double f, hipStream_t st) {
  if (!h->passes_valid) plan_passes(h);
  LocalExpArgs A;
  std::memset(&A, 0, sizeof A);
  local_super_exp(h, f, A.Mdiag, A.Mflip);
  A.rho = rho;
  A.nb = h->nb;
  static bool attr_set[64] = {};
  const int dev = h->cfg.device;
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    HIPCHK(hipFuncSetAttribute((const void*)k_local_exp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  for (const Pass& p : h->passes) {
    if (p.dbl.empty()) return fail(RYD_ERR_STATE, "pair passes expected for a double-flip dissipator");
    A.tile = p.tile;
    A.outer = p.outer;
    A.T = p.T;
    A.n_dbl = (int)p.dbl.size();
    for (int i = 0; i < A.n_dbl; ++i) {
      A.dbl_qb[i] = (signed char)p.dbl[i].first;
      A.dbl_qa[i] = (signed char)p.dbl[i].second;
    }
    std::pair<hipEvent_t, hipEvent_t> ev;
    int rc;
    if (h->timing) { if ((rc = timing_begin(h, st, ev))) return rc; }
    hipLaunchKernelGGL(k_local_exp, dim3((unsigned)(1ull << p.n_outer_bits), h->B), dim3(512),
                       ((size_t)1 << p.T) * sizeof(cplx), st, A);
    HIPCHK(hipGetLastError());
    if (h->timing) { HIPCHK(hipEventRecord(ev.second, st)); h->ev_used.push_back(ev); }
    h->stats.n_launches++;
  }
  return RYD_OK;
}

// CF4 steps per HALF block of the 4th-order splitting (below): two steps (tau = 4 ns at
// sampling rate 1) keep the splitting error at the level of the CF4 error (<= 1e-9 after 3.1 us
// for dephasing rates up to 0.5 / us and drives up to 25 rad/us, tests/probes/split_probe.py); faster
// dephasing halves the block.
static int row_block_steps(const ryd_handle* h, const ryd_opts& o) {
  if (o.split_steps > 0) return o.split_steps;
  double g = 0.0;
  for (int k = 0; k < 4; ++k) g = std::max(g, std::fabs(h->Sd[k].x));
  return g <= 0.5 ? 2 : 1;
}

// |change of the dissipator diagonal under one bit flip| is the same for every flip (pure dephasing)
static bool row_uniform_g(const ryd_handle* h) {
  const double g01 = h->Sd[1].x - h->Sd[0].x, g10 = h->Sd[2].x - h->Sd[0].x;
  const double g31 = h->Sd[1].x - h->Sd[3].x, g32 = h->Sd[2].x - h->Sd[3].x;
  return std::fabs(std::fabs(g01) - std::fabs(g10)) < 1e-14 * (1 + std::fabs(g01)) &&
         std::fabs(std::fabs(g01) - std::fabs(g31)) < 1e-14 * (1 + std::fabs(g01)) &&
         std::fabs(std::fabs(g01) - std::fabs(g32)) < 1e-14 * (1 + std::fabs(g01));
}

// Half a block of the split-operator master equation, in knot intervals (what a multi-knot CF4
// step must not exceed).
static bool rows_split_ok(const ryd_handle* h, const ryd_opts& o);
static double rows_split_estimate(const ryd_handle* h);
static int rows_split_probe(ryd_handle* h, const cplx* rho, const std::vector<StepDesc>& sb, size_t i0, size_t i1,
                            hipStream_t st, double* e_out, double* tau_out);
static int row_half_knots(const ryd_handle* h, const ryd_opts& o) {
  static const int kh_env = dev_env_int("RYD_ROWS_KH", 0, 1, 8);  // dev A/B (RYD_DEV=1)
  if (kh_env > 0 && o.split_steps <= 0) return kh_env;
  int Kh = row_block_steps(h, o);
  if ((!row_uniform_g(h) || h->has_dbl) && o.split_steps <= 0) Kh = 1;
  // Round 4, row passes on k_split_reg: the splitting error of a block grows with g tau^4 (measured over the whole
  // anneal on the interacting 12-atom register against two-knot halves, tools/rows_tune2.py: four-knot halves 5.5e-9
  // at g = 0.05, 2.2e-8 at g = 0.2), so slow dephasing (g <= 0.06 / us; the 12-atom tight fixture at 0.05: entries of rho within 5.9e-9) takes blocks of 4 + 4 knots - the
  // unitary of a half is then ONE 6th-order sub-step where the waveforms are one polynomial: 18.4 -> 13 s at 14 atoms
  if (Kh == 2 && o.split_steps <= 0 && rows_split_ok(h, o) && row_uniform_g(h) && !h->has_dbl) {
    double g = 0.0;
    for (int k = 0; k < 4; ++k) g = std::max(g, std::fabs(h->Sd[k].x));
    // (the block error comes from the commutators of the dissipator with the DRIVE - the diagonal part of H commutes with
    // dephasing - so the drive bound caps the rule too: measured at |c| = Omega / 2 = 12.6 rad / us, allowed up to 16)
    double cmax = 0.0;
    for (double v : h->bd_c1) cmax = std::max(cmax, v);
    // ... and only for drives without abrupt edges (round 5).  The rule was calibrated along the anneal, whose state follows
    // the drive adiabatically; after a QUENCH - the all-ground matrix dropped into a strong drive, which is what every
    // square / EOM pulse does - the four-knot halves left 1e-8 within 20 ns where the two-knot ones and the polynomial
    // rows agree with the tight Lindbladian to 1e-9 (tools/rows_quench_probe.py).  No edge = the drive never changes by
    // more than a tenth of its maximum within 10 ns.
    double dcmax = 0.0;
    for (double v : h->bd_dc) dcmax = std::max(dcmax, v);
    const bool smooth_drive = dcmax * 0.01 <= 0.1 * std::max(cmax, 1e-300);
    if (g <= 0.06 && cmax <= 16.0 && smooth_drive) Kh = 4;  // (0.06: entries of rho within ~7e-9 of the 12-atom tight oracle, its probe products within 8e-8)
  }
  return Kh;
}

// Row passes on the register-resident split-operator kernel (k_split_reg<N, 5, false, ROWS>, host_split.hpp; round 4):
// the unitary of a half block as 6th-order (4th-order for one-knot steps) split-operator sub-steps, one per CF4 step of
// the schedule, instead of CF4 + in-place symplectic exponentials on k_ket.  Returns 1 when the run cannot take the
// tan-form rotations (|beta c| > 1: drives of hundreds of rad/us) - the caller then uses k_ket for this conjugation.
static int rows_split_pass(ryd_handle* h, cplx* buf, const std::vector<StepDesc>& sb, size_t i0, size_t i1, bool use_pre,
                           bool use_post, const double* tdev, double kick_pre, double kick_post, int kick_idx,
                           double kick_u, size_t n_rows, bool count_stages, hipStream_t st);

// mesolve by operator splitting (header of this file).  Blocks of two halves, 4th order
// (Chin's scheme 4A: all coefficients positive, so the dissipative factor never runs backwards):
//
//   rho <- D(tau/6) . W2 ( D(2 tau/3) . W1 ( D(tau/6) . rho ) W1^+ ) W2^+
//   W1 = V U(t + tau/2, t),   W2 = U(t + tau, t + tau/2) V,   V = exp(+i (eps/2) H_drive(t + tau/2))
//
// V carries the commutator correction [B, [A, B]] of the scheme: for an elementwise diagonal
// B = d(a, b) whose value changes by +-g when one index bit flips, [B, [A, B]] = -g^2 A_drive
// exactly, so the "modified potential" is a drive-only rotation by eps = tau^3 g^2 / 72 - it is
// what makes the splitting 4th order in tau (without it the error is O(tau^2 g^2)).  It is
// only exact when every single-bit flip changes d by the same |g| (pure dephasing: Sd = (0, -g,
// -g, 0)); other diagonal dissipators fall back to the 2nd-order behaviour of the uncorrected
// scheme with half the block length.
static int run_rows(ryd_handle* h, cplx* state, const std::vector<StepDesc>& sched, cplx* snaps,
                    const ryd_opts& o, hipStream_t st) {
  if (sched.empty()) return RYD_OK;
  int rc;
  if ((rc = ket_init_device(h))) return rc;
  // ---- blocks of the 4th-order splitting: two halves of EQUAL duration, always ----
  // A block gathers up to 2 Kh knot units of the schedule (a requested evaluation time ends it early) and is
  // cut at its time midpoint; a step that straddles the midpoint is split there (a CF4 step may start and end
  // anywhere inside its spline piece).  Round 2 took the halves by step COUNT and fell back to a Strang block
  // for a lone half: next to an evaluation time or to the sub-stepped intervals around a waveform kink the
  // halves then differed (2 ns + 1 ns) and the block was only 2nd order - one such block before t = 1.3 us
  // cost 2e-7 on the interacting 10-atom register (tests/test_gpu_fullsize.py, the fixture the round-2
  // verdict asked for); with equal halves every block is Chin's scheme 4A.
  const int Kh = row_half_knots(h, o);
  std::vector<StepDesc> sb;                      // the schedule with the straddling steps split
  struct Block { size_t i0, mid, i1; double tau; };
  std::vector<Block> blocks;
  {
    auto part = [](const StepDesc& d, double off, double len) {  // the piece [off, off + len) of step d
      StepDesc e = d;
      const double us = d.u1 - kC1 * d.h + off;
      e.h = len;
      e.u1 = us + kC1 * len;
      e.u2 = us + kC2 * len;
      return e;
    };
    size_t i = 0;
    while (i < sched.size()) {
      size_t j = i;
      int u = 0;
      bool cut = false;
      double tau = 0.0;
      while (j < sched.size() && u < 2 * Kh && !cut) {
        // four-knot halves: a block does not grow past 2 Kh knot intervals (where the estimate accepts three-knot steps the
        // old rule gathered 3 + 3 + 3 knots and cut the middle step: halves of a three-knot and a 1.5-knot sub-step, 20 + 1
        // stage bodies per 4.5 knots on the last third of the anneal; now 3 + 3: 10 + 1 per 3 knots)
        if (Kh > 2 && j > i && u + std::max(sched[j].pad, 1) > 2 * Kh) break;
        tau += sched[j].h; u += std::max(sched[j].pad, 1); cut = sched[j].snap >= 0; ++j;
      }
      Block b{sb.size(), 0, 0, tau};
      const double half = 0.5 * tau, tol = 1e-12 * std::max(tau, 1e-6);
      double acc = 0.0;
      bool placed = false;
      for (size_t k = i; k < j; ++k) {
        const StepDesc& d = sched[k];
        if (!placed && acc + d.h > half + tol) {
          const double hA = half - acc;
          if (hA > tol) {
            StepDesc a = part(d, 0.0, hA);
            a.snap = -1;
            sb.push_back(a);
          }
          b.mid = sb.size();
          sb.push_back(part(d, std::max(hA, 0.0), d.h - std::max(hA, 0.0)));
          placed = true;
        } else {
          sb.push_back(d);
          if (!placed && std::fabs(acc + d.h - half) <= tol) { b.mid = sb.size(); placed = true; }
        }
        acc += d.h;
      }
      b.i1 = sb.size();
      blocks.push_back(b);
      i = j;
    }
  }
  std::vector<KetStep> ks;
  if ((rc = to_ket_steps(h, sb, o, -1.0, ks))) return rc;
  for (KetStep& k : ks) k.snap = -1;  // snapshots are whole-matrix copies between blocks
  if ((rc = upload_ket_steps(h, ks, st))) return rc;
  bool rsplit = rows_split_ok(h, o);  // (the k_ket schedule stays uploaded: a conjugation may fall back to it)
  // Error control of the split-operator rows.  rows_split_ok has filtered by the caller's options and an
  // a-priori estimate; here the local error of the unitary sub-steps is MEASURED on the heaviest row of the matrix
  // (rows_split_probe: one sub-step whole against two halves) - at the first block, then after 16, 32, ... 256 knot
  // intervals (a sequence starts from a product state, the least representative one) and whenever the drive bound has grown
  // by half - against this solve's budget (5e-8 over a sequence, or 500 tol; the two-sided product U rho U^+ carries the
  // error twice).  A probe that finds a sub-step more than 4 x over its allowance hands the REST of the call to the
  // polynomial rows (k_ket: a-priori tolerance per exponential); the measured rate is booked in ryd_stats.reserved[0].
  const double rows_budget = o.tol > 0 ? 500.0 * o.tol : 5e-8;
  const double rows_T = std::max(h->tknots.size() >= 2 ? h->tknots.back() - h->tknots.front() : 0.0, 1e-12);
  int probe_period = 16, probe_since = 0;
  double probe_time_since = 0.0;  // simulated time (us) the blocks since the last probe have covered
  bool probed = false;
  double probe_rate = 0.0, probe_amp = 0.0, amp_max_rows = 0.0;
  for (double v : h->bd_c1) amp_max_rows = std::max(amp_max_rows, v);
  // |change of d under one bit flip|: (0,0)<->(0,1)/(1,0) and (1,1)<->(0,1)/(1,0)
  const double g01 = h->Sd[1].x - h->Sd[0].x, g10 = h->Sd[2].x - h->Sd[0].x;
  const double g31 = h->Sd[1].x - h->Sd[3].x, g32 = h->Sd[2].x - h->Sd[3].x;
  const bool uniform_g = row_uniform_g(h);
  const double gflip = std::fabs(g01);
  (void)g10; (void)g31; (void)g32;
  const bool dbl = h->has_dbl;  // the dissipator factor is not elementwise: k_local_exp passes
  double pending = 0.0;         // dissipator time not applied yet (adjacent factors merge)
  const size_t D = (size_t)1 << h->N;
  const size_t n_rows = D * (size_t)h->B;
  const size_t bytes = h->dim * (size_t)h->B * sizeof(cplx);
  const unsigned nt = (unsigned)(D / 32);
  if (!h->ftab_dev) HIPCHK(hipMalloc((void**)&h->ftab_dev, 4 * 128 * sizeof(double)));
  cplx* cur = state;
  cplx* other = h->wA;
  int tab_slot = 0;

  // one conjugation  X <- W X W^+  over the steps [i0, i1): two row passes + a conjugate transposition
  auto conjugate = [&](size_t i0, size_t i1, double f_in, double f_out, double kick_pre, double kick_post,
                       int kick_idx, double kick_u) -> int {
    // elementwise factors exp(f * d(a, b)) as four 16-entry tables (counts n00, n01, n10, n11): slot
    // [0] on the load of the first pass, [1] on the store of the second.  Four rotating slots, so a
    // table is never rewritten while a queued launch may still read it (the stream serialises more
    // than four launches apart only after a synchronisation every 4th conjugation).
    double tab[128];
    for (int k = 0; k < 4; ++k)
      for (int n = 0; n < 16; ++n) {
        tab[k * 16 + n] = std::exp(f_in * h->Sd[k].x * n);
        tab[64 + k * 16 + n] = std::exp(f_out * h->Sd[k].x * n);
      }
    if (dbl) {
      pending += f_in;
      int rcl;
      if (pending != 0.0 && (rcl = launch_local_exp(h, cur, pending, st))) return rcl;
      pending = 0.0;
    }
    if (tab_slot == 0) HIPCHK(hipStreamSynchronize(st));
    double* tdev = h->ftab_dev + 128 * tab_slot;
    tab_slot = (tab_slot + 1) & 3;
    HIPCHK(hipMemcpyAsync(tdev, tab, sizeof tab, hipMemcpyHostToDevice, st));
    KetArgs A;
    fill_ket_args(h, A);
    A.steps = h->ksched_dev + i0;
    A.n_steps = (int)(i1 - i0);
    A.rows_log2 = h->N;
    A.conj_sign = -1.0;
    A.kick_pre = kick_pre;
    A.kick_post = kick_post;
    A.kick_idx = kick_idx;
    A.kick_u = kick_u;
    {
      const double ph = ks[i1 - 1].cum_phase - (i0 > 0 ? ks[i0 - 1].cum_phase : 0.0);
      A.fin_cs = std::cos(ph);
      A.fin_sn = std::sin(ph);
    }
    A.ftab = tdev;
    A.state = cur;
    A.use_pre = !dbl && f_in != 0.0;
    int rc2;
    bool this_split = rsplit;
    if (this_split) {
      rc2 = rows_split_pass(h, cur, sb, i0, i1, A.use_pre != 0, false, tdev, kick_pre, kick_post, kick_idx, kick_u, n_rows, false, st);
      if (rc2 == 1) {  // (nothing has been launched)
        this_split = false;
      }
      else if (rc2) return rc2;
    }
    if (!this_split && (rc2 = launch_ket(h, A, n_rows, st, KET_ROWS))) return rc2;
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (h->timing) { if ((rc2 = timing_begin(h, st, ev))) return rc2; }
    hipLaunchKernelGGL(k_transpose_conj, dim3(nt, nt, h->B), dim3(256), 0, st, cur, other, h->N);
    HIPCHK(hipGetLastError());
    if (h->timing) { HIPCHK(hipEventRecord(ev.second, st)); h->ev_used.push_back(ev); }
    h->stats.n_launches++;
    std::swap(cur, other);
    A.state = cur;
    A.use_pre = 0;
    A.use_post = !dbl && f_out != 0.0;
    if (this_split) {
      if ((rc2 = rows_split_pass(h, cur, sb, i0, i1, false, A.use_post != 0, tdev, kick_pre, kick_post, kick_idx, kick_u, n_rows, true, st)))
        return rc2 == 1 ? fail(RYD_ERR_STATE, "split-operator row pass refused after its first half ran") : rc2;
    } else if ((rc2 = launch_ket(h, A, n_rows, st, KET_ROWS))) return rc2;
    if (dbl) pending += f_out;
    if (!this_split) count_ket_work(h, ks, i0, i1, 1);  // one Lindbladian application ~ one two-sided ket stage
    h->stats.n_steps += (int64_t)(i1 - i0);
    return RYD_OK;
  };

  for (const Block& b : blocks) {
    // rho <- D(tau/6) W2 ( D(2 tau/3) W1 ( D(tau/6) rho ) W1^+ ) W2^+ with halves of tau / 2 each
    const double tau = b.tau;
    if (rsplit) {
      int knots_b = 0;
      double amp_b = 0.0;
      for (size_t k = b.i0; k < b.i1; ++k) {
        knots_b += std::max(1, sb[k].pad);
        amp_b = std::max(amp_b, span_max(h->bd_c1, sb[k].idx, std::max(1, sb[k].pad)));
      }
      if (!probed || probe_since >= probe_period || amp_b > std::max(1.5 * probe_amp, 0.1 * amp_max_rows)) {
        double e = 0.0, tau_s = 0.0;
        if ((rc = rows_split_probe(h, cur, sb, b.i0, b.mid, st, &e, &tau_s))) return rc;
        const double allowed = 0.5 * rows_budget * tau_s / rows_T;
        if (tau_s > 0.0 && e > 4.0 * allowed) {
          rsplit = false;                 // the polynomial rows from here on
          h->stats.reserved[3] += 1.0;
          // ... and the stretch since the last probe ran at a rate nobody had measured: booked at this probe's rate, like
          // run_split books an overrun (the estimate a caller reads must not under-report)
          h->stats.reserved[0] += 2.0 * std::max(0.0, e / tau_s - probe_rate) * probe_time_since;
        } else if (tau_s > 0.0) {
          probe_rate = std::max(0.5 * (probe_rate + e / tau_s), e / tau_s);
        }
        probed = true;
        probe_since = 0;
        probe_time_since = 0.0;
        probe_period = std::min(256, 2 * probe_period);
        probe_amp = amp_b;
      }
      probe_since += knots_b;
      probe_time_since += tau;
      if (rsplit) h->stats.reserved[0] += 2.0 * probe_rate * tau;
    }
    const double eps = (uniform_g && !dbl) ? tau * tau * tau * gflip * gflip / 72.0 : 0.0;
    const StepDesc& m0 = sb[b.mid];
    const double kick_u = m0.u1 - kC1 * m0.h;  // start of the step `mid` inside its knot interval
    if ((rc = conjugate(b.i0, b.mid, tau / 6.0, tau / 3.0, 0.0, 0.5 * eps, m0.idx, kick_u))) return rc;
    if ((rc = conjugate(b.mid, b.i1, tau / 3.0, tau / 6.0, 0.5 * eps, 0.0, m0.idx, kick_u))) return rc;
    const int snap = sb[b.i1 - 1].snap;
    if (dbl && pending != 0.0 && (snap >= 0 || &b == &blocks.back())) {
      if ((rc = launch_local_exp(h, cur, pending, st))) return rc;
      pending = 0.0;
    }
    if (snap >= 0 && snaps)
      HIPCHK(hipMemcpyAsync(snaps + (size_t)snap * h->dim * h->B, cur, bytes, hipMemcpyDeviceToDevice, st));
  }
  if (cur != state) HIPCHK(hipMemcpyAsync(state, cur, bytes, hipMemcpyDeviceToDevice, st));
  return RYD_OK;
}

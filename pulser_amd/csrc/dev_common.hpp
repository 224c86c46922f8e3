// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                        \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess)                                                   \
      return fail(RYD_ERR_HIP, "%s failed: %s (%s:%d)", #expr,              \
                  hipGetErrorString(e_), __FILE__, __LINE__);               \
  } while (0)

// ---------------------------------------------------------------------------
// development switches
// ---------------------------------------------------------------------------
// Every A/B switch of the library that changes numerics or the kernel chosen is read through dev_env: it sees the
// variable only when RYD_DEV=1 is set as well, so a stray variable in a production environment cannot change a run
// (RYD_CHECK and RYD_HOST_TIMING only observe and stay ungated).  Values are clamped where they are used.
static const char* dev_env(const char* name) {
  static const bool dev = [] {
    const char* d = std::getenv("RYD_DEV");
    return d && d[0] == '1' && d[1] == 0;
  }();
  if (!dev) {
    // a gated switch that is set without RYD_DEV=1 has no effect: say so once (a probe that labels its output with the
    // variable would otherwise report an A/B that never happened - ADVICE r05)
    const char* ignored = std::getenv(name);
    if (ignored && ignored[0]) {
      static std::atomic<bool> told{false};
      if (!told.exchange(true))
        std::fprintf(stderr, "librydemu: %s is set but ignored (development switches need RYD_DEV=1)\n", name);
    }
    return nullptr;
  }
  return std::getenv(name);
}
static void dev_env_rejected(const char* name, const char* value) {
  std::fprintf(stderr, "librydemu: %s=%s is not a valid value, the default is used\n", name, value);
}
static int dev_env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = dev_env(name);
  if (!e || !e[0]) return dflt;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  if (end == e || v < lo || v > hi) {  // garbage or out of range: the default, not a surprise - and not silently
    dev_env_rejected(name, e);
    return dflt;
  }
  return (int)v;
}
static double dev_env_double(const char* name, double dflt, double lo, double hi) {
  const char* e = dev_env(name);
  if (!e || !e[0]) return dflt;
  char* end = nullptr;
  const double v = std::strtod(e, &end);
  if (end == e || !(v >= lo && v <= hi)) {
    dev_env_rejected(name, e);
    return dflt;
  }
  return v;
}
static bool dev_env_flag(const char* name, bool dflt) {  // "0" / "1"
  const char* e = dev_env(name);
  if (!e || !e[0]) return dflt;
  return e[0] != '0';
}

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
struct Segs {
  int lo[3];
  int len[3];
};

__host__ __device__ __forceinline__ unsigned long long deposit(
    unsigned long long v, const Segs& s) {
  unsigned long long r = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r |= (v & ((1ull << s.len[i]) - 1ull)) << s.lo[i];
    v >>= s.len[i];
  }
  return r;
}

__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ cplx cfma(cplx a, cplx b, cplx c) {  // a*b + c
  return make_double2(fma(a.x, b.x, fma(-a.y, b.y, c.x)),
                      fma(a.x, b.y, fma(a.y, b.x, c.y)));
}

// The cubic of series `series` on knot interval `idx` at offset u into it; pp: [n_series][n_int][4] complex, highest
// power first (Horner: three FMAs per component).
__device__ __forceinline__ cplx pp_eval(const cplx* pp, int n_int, int series, int idx, double u) {
  const cplx* p = pp + ((size_t)series * n_int + idx) * 4;
  cplx r = p[0];
  r = make_double2(fma(r.x, u, p[1].x), fma(r.y, u, p[1].y));
  r = make_double2(fma(r.x, u, p[2].x), fma(r.y, u, p[2].y));
  r = make_double2(fma(r.x, u, p[3].x), fma(r.y, u, p[3].y));
  return r;
}

// Drive (cr + i ci) and detuning (dl) of one atom: w1 * val(idx1, u1) + w2 * val(idx2, u2) of its drive, detuning and
// offset series, each times its scale.  Extra detuning terms (ryd_qdesc.extra) are the caller's.
__device__ __forceinline__ void qdesc_coefs(const cplx* pp, int n_int, const ryd_qdesc d, int idx1, double u1, double w1,
                                            int idx2, double u2, double w2, double& cr, double& ci, double& dl) {
  cr = ci = dl = 0.0;
  if (d.drive_series >= 0) {
    const cplx a = pp_eval(pp, n_int, d.drive_series, idx1, u1), b = pp_eval(pp, n_int, d.drive_series, idx2, u2);
    cr = d.drive_scale * (w1 * a.x + w2 * b.x);
    ci = d.drive_scale * (w1 * a.y + w2 * b.y);
  }
  if (d.det_series >= 0)
    dl += d.det_scale * (w1 * pp_eval(pp, n_int, d.det_series, idx1, u1).x + w2 * pp_eval(pp, n_int, d.det_series, idx2, u2).x);
  if (d.off_series >= 0)
    dl += d.off_scale * (w1 * pp_eval(pp, n_int, d.off_series, idx1, u1).x + w2 * pp_eval(pp, n_int, d.off_series, idx2, u2).x);
}

// wave-uniform double -> scalar registers
__device__ __forceinline__ double uniform_d(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// Where batch entry b's snapshot of evaluation slot `slot` goes: the dense layout [slot][B][D] of ryd_solve, or with a
// snapshot map (ryd_set_snapshot_map) map[b][slot] kets into `snaps` - null when the map leaves that state unstored.
// The map is read with (uniform) loads only.
__device__ __forceinline__ cplx* snap_dst(cplx* snaps, const long long* __restrict__ map, int map_slots, int slot, int B,
                                          int b, size_t D) {
  if (map == nullptr) return snaps + ((size_t)slot * B + b) * D;
  const long long off = map[(size_t)b * map_slots + slot];
  return off < 0 ? nullptr : snaps + (size_t)off * D;
}

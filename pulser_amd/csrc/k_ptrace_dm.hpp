// Part of librydemu (included by rydemu.hip, one translation unit; after k_ptrace.hpp).
// ---------------------------------------------------------------------------
// ryd_reduced_density_dm: out[i][a][a'] += sum_b sum_r rho(i, b)[idx(a, r)][idx(a', r)] - the partial trace
// rho_A = Tr_rest rho of every stored density matrix over a small set A of atoms, summed over the trajectory axis
// ---------------------------------------------------------------------------
// What Qobj.ptrace(sel) computes of the matrices a master-equation run hands out, without a matrix leaving the device.
// Of the dim^2 elements of a matrix only dA dim are read: element (idx(a, r), idx(a', r)) sits at
//   A(a) dim + A(a') + F(r) (dim + 1),   A: the kept digits times their strides, F: the free digits times theirs,
// so an entry (a, a') is a fixed offset and r walks a "diagonal" of stride multiples of dim + 1.  This is a gather, not
// a stream: two r never share a cache line, and the dA columns of one row are adjacent only where the kept sites are
// the lowest ones.  The kernel is bound by the lines it touches (at most dA^2 R = dA dim per matrix) and by the loads
// in flight, not by the bytes it uses.
//
// Tiling.  A workgroup of 256 threads owns one (time i, split s) and walks the trajectories b and its share of the r
// range.  Up to 256 entries (dA <= 16, K = 1): thread tid holds ONE entry e = tid % dA^2 (a' fastest: adjacent lanes
// read adjacent columns whenever the kept sites allow it) of r slot tid / dA^2; the NS = LD^m <= 256 / dA^2 slots are
// the configurations of the m lowest free sites, so a thread's offset inside a matrix is the same for every step of
// the walk.  More entries (dA = 27, 32: K = 4; dA = 64: K = 16): one slot, thread tid holds the entries tid + 256 k in
// K complex accumulators.  The digit arithmetic of entry and slot runs once per workgroup (by the compile-time local
// dimension LD - no division in the loop); the walk over the remaining free sites ("outer" index o) is uniform: one
// scalar digit walk per step.  U steps (8, 2, 1 for K = 1, 4, 16) are fetched before the first is added: 8 - 16
// independent global_load_dwordx4 per thread in flight.  The accumulators stay in registers across steps and
// trajectories and leave once: the slots are added through LDS in the order slot 0 .. NS - 1 by the thread of slot 0,
// and the sum is added onto `out` (n_split = 1) or stored to this split's partial (n_split > 1), which
// k_ptrace_dm_sum then adds onto `out` in the order split 0 .. n_split - 1.  (k_ptrace_sum of the ket call mirrors the
// upper triangle onto the lower one; here nothing is Hermitian by assumption, so every entry has a thread of its own.)
// Lanes without an entry (256 is no multiple of dA^2 for qutrits; dA^2 = 729 of 1024) read and write nothing.
//
// Summation order: fixed by (dim, keep, n_batch, n_split) alone - per thread b ascending, inside it o ascending; then
// slots, then splits.  No atomics; two calls with the same n_split are bitwise equal.  Every one of the dA^2 entries
// is the sum of the stored elements the formula names: nothing is mirrored, conjugated or divided by a trace.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch, no spills:
//   k_ptrace_dm<2|3|4, 1, 8>:   44 VGPRs, 79-80 SGPRs, LDS 4 096 B (the slot sums): 8 waves per SIMD
//   k_ptrace_dm<2|3,   4, 2>:   64 VGPRs, 67-68 SGPRs, no LDS:                    8 waves per SIMD
//   k_ptrace_dm<2|4,  16, 1>:  196 VGPRs, 84 SGPRs,    no LDS:                    2 waves per SIMD (16 accumulators, 16
//                              values in flight and 16 64-bit offsets per thread)
//   k_ptrace_dm_sum:            18 VGPRs, 22 SGPRs,    no LDS
constexpr int kPtraceDmKeepSites = 6;    // 2^6 = 64 rows at most
constexpr int kPtraceDmSlotSites = 8;    // 2^8 = 256 slots at most
constexpr int kPtraceDmOuterSites = 40;
constexpr int kPtraceDmTargetWgs = 1024; // what n_split = 0 aims at: 4 workgroups per CU

struct PtraceDmGeom {
  long long keep_stride[kPtraceDmKeepSites];    // stride of the j-th digit of a row index a, least significant first
  long long slot_stride[kPtraceDmSlotSites];    // (dim + 1) * stride of the j-th free site inside the slots, lowest first
  long long outer_stride[kPtraceDmOuterSites];  // (dim + 1) * stride of the j-th free site outside them, lowest first
  long long dim;
  int n_keep, n_slot_sites, n_outer_sites;
  int dA, dA2, NS;                              // rows, entries, r slots of a workgroup
  unsigned n_outer;                             // steps of the walk per matrix: R / NS
};

template <int LD, int K, int U>
__global__ __launch_bounds__(256) void k_ptrace_dm(const cplx* __restrict__ states, int n_times, int n_batch,
                                                   long long stride_t, long long stride_b, const PtraceDmGeom g,
                                                   int n_split, cplx* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) cplx lds[K == 1 ? 256 : 1];
  const int tid = threadIdx.x;
  const int dA = g.dA, dA2 = g.dA2;

  // where this thread's entries sit inside a matrix: the same for every step (-1: no entry)
  long long eoff[K];
  const int slot = K == 1 ? tid / dA2 : 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = K == 1 ? tid - slot * dA2 : tid + k * 256;
    eoff[k] = -1;
    if (slot < g.NS && e < dA2) {
      unsigned a = (unsigned)(e / dA), c = (unsigned)(e - (e / dA) * dA), s = (unsigned)slot;
      long long row = 0, col = 0, off = 0;
      for (int j = 0; j < g.n_keep; ++j) {
        const unsigned qa = a / LD, qc = c / LD;
        row += (long long)(a - qa * LD) * g.keep_stride[j];
        col += (long long)(c - qc * LD) * g.keep_stride[j];
        a = qa;
        c = qc;
      }
      for (int j = 0; j < g.n_slot_sites; ++j) {
        const unsigned q = s / LD;
        off += (long long)(s - q * LD) * g.slot_stride[j];
        s = q;
      }
      eoff[k] = row * g.dim + col + off;
    }
  }
  const int split = blockIdx.x;
  const unsigned o0 = (unsigned)((unsigned long long)g.n_outer * split / n_split);
  const unsigned o1 = (unsigned)((unsigned long long)g.n_outer * (split + 1) / n_split);

  for (long long i = blockIdx.y; i < n_times; i += gridDim.y) {
    cplx acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = make_double2(0.0, 0.0);
    for (int b = 0; b < n_batch; ++b) {
      const cplx* m = states + (i * stride_t + (long long)b * stride_b);
      for (unsigned o = o0; o < o1; o += U) {
        cplx v[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int k = 0; k < K; ++k) v[u][k] = make_double2(0.0, 0.0);
          if (o + u < o1) {  // (uniform)
            unsigned w = o + u;
            long long base = 0;
            for (int j = 0; j < g.n_outer_sites; ++j) {
              const unsigned q = w / LD;
              base += (long long)(w - q * LD) * g.outer_stride[j];
              w = q;
            }
            const cplx* p = m + base;
#pragma unroll
            for (int k = 0; k < K; ++k)
              if (eoff[k] >= 0) v[u][k] = p[eoff[k]];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (o + u < o1) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
              acc[k].x += v[u][k].x;
              acc[k].y += v[u][k].y;
            }
          }
      }
    }
    cplx* tgt = dst + (n_split == 1 ? i : i * n_split + split) * (long long)dA2;
    if (K == 1) {
      // the slots of an entry, in the order 0 .. NS - 1, by the thread of slot 0
      __syncthreads();  // (the previous time's sums are read)
      lds[tid] = acc[0];
      __syncthreads();
      if (tid < dA2) {
        cplx s = lds[tid];
        for (int sl = 1; sl < g.NS; ++sl) {
          const cplx t = lds[sl * dA2 + tid];
          s.x += t.x;
          s.y += t.y;
        }
        if (n_split == 1) {
          const cplx old = tgt[tid];
          s = make_double2(old.x + s.x, old.y + s.y);
        }
        tgt[tid] = s;
      }
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (eoff[k] >= 0) {
          const int e = tid + k * 256;
          cplx s = acc[k];
          if (n_split == 1) {
            const cplx old = tgt[e];
            s = make_double2(old.x + s.x, old.y + s.y);
          }
          tgt[e] = s;
        }
    }
  }
}

// out[i] += part[i][0] + part[i][1] + ... in that order; one thread per entry.  blockIdx.y walks the times with stride
// gridDim.y.
__global__ __launch_bounds__(256) void k_ptrace_dm_sum(const cplx* __restrict__ part, int n_times, int n_split, int dA2,
                                                       cplx* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= dA2) return;
  for (long long i = blockIdx.y; i < n_times; i += gridDim.y) {
    const cplx* p = part + i * n_split * dA2 + e;
    cplx s = out[i * dA2 + e];
    for (int k = 0; k < n_split; ++k) {
      const cplx t = p[(long long)k * dA2];
      s.x += t.x;
      s.y += t.y;
    }
    out[i * dA2 + e] = s;
  }
}

template <int LD, int K, int U>
static void ptrace_dm_launch(dim3 grid, hipStream_t stream, const cplx* states, int n_times, int n_batch,
                             long long stride_t, long long stride_b, const PtraceDmGeom& g, int n_split, cplx* dst) {
  hipLaunchKernelGGL((k_ptrace_dm<LD, K, U>), grid, dim3(256), 0, stream, states, n_times, n_batch, stride_t, stride_b,
                     g, n_split, dst);
}

extern "C" int ryd_reduced_density_dm(const void* states_dev, int32_t n_times, int32_t n_batch, int64_t stride_t,
                                      int64_t stride_b, int64_t dim, int32_t local_dim, int32_t n_sites,
                                      const int32_t* keep, int32_t n_keep, void* out_dev, int32_t n_split,
                                      void* scratch_dev, int64_t scratch_bytes, int32_t device, void* stream) {
  if (n_times < 0) return fail(RYD_ERR_INVALID, "reduced_density_dm: n_times %d is negative", (int)n_times);
  if (n_batch < 1) return fail(RYD_ERR_INVALID, "reduced_density_dm: n_batch %d is smaller than 1", (int)n_batch);
  if (local_dim < 2 || local_dim > 4)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: local_dim %d is not 2, 3 or 4", (int)local_dim);
  if (n_sites < 1 || n_sites > 62)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: n_sites %d is not in 1..62", (int)n_sites);
  int64_t want = 1;
  for (int k = 0; k < n_sites; ++k) {
    if (want > INT64_MAX / local_dim) return fail(RYD_ERR_INVALID, "reduced_density_dm: local_dim^n_sites overflows");
    want *= local_dim;
  }
  if (dim != want)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: dim %lld is not local_dim^n_sites = %d^%d", (long long)dim,
                (int)local_dim, (int)n_sites);
  if (dim > INT32_MAX) return fail(RYD_ERR_INVALID, "reduced_density_dm: dim %lld is too large", (long long)dim);
  const int64_t dim2 = dim * dim;  // (below 2^62)
  if (stride_t < dim2 || stride_b < dim2)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: strides %lld / %lld are smaller than a matrix of %lld elements",
                (long long)stride_t, (long long)stride_b, (long long)dim2);
  if (!keep) return fail(RYD_ERR_INVALID, "reduced_density_dm: keep is null");
  if (n_keep < 1 || n_keep > n_sites)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: n_keep %d is not in 1..n_sites = %d", (int)n_keep, (int)n_sites);
  for (int k = 0; k < n_keep; ++k)
    if (keep[k] < 0 || keep[k] >= n_sites || (k > 0 && keep[k] <= keep[k - 1]))
      return fail(RYD_ERR_INVALID, "reduced_density_dm: keep[%d] = %d is out of range or not strictly ascending", k,
                  (int)keep[k]);
  int64_t dA64 = 1;
  for (int k = 0; k < n_keep && dA64 <= 64; ++k) dA64 *= local_dim;
  if (dA64 > 64)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: %d kept sites of local dimension %d exceed 64 rows", (int)n_keep,
                (int)local_dim);
  if (n_split < 0) return fail(RYD_ERR_INVALID, "reduced_density_dm: n_split %d is negative", (int)n_split);
  if (scratch_bytes < 0) return fail(RYD_ERR_INVALID, "reduced_density_dm: scratch_bytes is negative");
  if (!states_dev) return fail(RYD_ERR_INVALID, "reduced_density_dm: states_dev is null");
  if (!out_dev) return fail(RYD_ERR_INVALID, "reduced_density_dm: out_dev is null");
  const int dA = (int)dA64, dA2 = dA * dA;
  const int64_t part_bytes = (int64_t)dA2 * (int64_t)sizeof(cplx);  // one (time, split) partial
  const int K = dA2 <= 256 ? 1 : dA2 <= 1024 ? 4 : 16;

  // the slots: the lowest free sites, as many as 256 threads hold with one entry each
  PtraceDmGeom g{};
  g.dA = dA;
  g.dA2 = dA2;
  g.dim = dim;
  g.n_keep = n_keep;
  if (n_keep > kPtraceDmKeepSites) return fail(RYD_ERR_INVALID, "reduced_density_dm: internal geometry error");
  std::vector<int64_t> stride(n_sites);
  {
    int64_t s = 1;
    for (int k = n_sites - 1; k >= 0; --k, s *= local_dim) stride[k] = s;
  }
  std::vector<char> kept(n_sites, 0);
  for (int k = 0; k < n_keep; ++k) {
    kept[keep[k]] = 1;
    g.keep_stride[n_keep - 1 - k] = stride[keep[k]];  // the last kept site is the least significant digit of a
  }
  int NS = 1;
  int64_t n_outer = 1;
  for (int k = n_sites - 1; k >= 0; --k) {  // lowest stride first
    if (kept[k]) continue;
    if (K == 1 && g.n_outer_sites == 0 && (int64_t)dA2 * NS * local_dim <= 256) {
      g.slot_stride[g.n_slot_sites++] = stride[k] * (dim + 1);
      NS *= local_dim;
    } else {
      if (g.n_outer_sites >= kPtraceDmOuterSites)
        return fail(RYD_ERR_INVALID, "reduced_density_dm: dim %lld is too large", (long long)dim);
      g.outer_stride[g.n_outer_sites++] = stride[k] * (dim + 1);
      n_outer *= local_dim;
    }
  }
  g.NS = NS;
  g.n_outer = (unsigned)n_outer;  // (below dim <= INT32_MAX)
  if (g.n_slot_sites > kPtraceDmSlotSites || (int64_t)NS * dA2 > 256 * (int64_t)K)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: internal geometry error");

  if (n_split == 0) {
    // enough workgroups to fill the device, every split with at least as many steps as one round of loads in flight
    // covers (and at least 4); never more than the scratch given holds
    const int64_t min_steps = K == 1 ? 8 : 4;
    int64_t s = std::min<int64_t>(kPtraceDmTargetWgs / std::max<int32_t>(n_times, 1), n_outer / min_steps);
    if (n_times > 0 && scratch_dev) s = std::min<int64_t>(s, scratch_bytes / (part_bytes * n_times));
    else s = 1;
    n_split = (int32_t)std::max<int64_t>(s, 1);
  } else if (n_split > 1) {
    if (!scratch_dev) return fail(RYD_ERR_INVALID, "reduced_density_dm: n_split %d needs scratch_dev", (int)n_split);
    if (n_split > 65535) return fail(RYD_ERR_INVALID, "reduced_density_dm: n_split %d exceeds 65535", (int)n_split);
    if (scratch_bytes / part_bytes / n_split < n_times)
      return fail(RYD_ERR_INVALID,
                  "reduced_density_dm: scratch of %lld bytes is smaller than the %lld needed by n_split %d",
                  (long long)scratch_bytes, (long long)(part_bytes * n_split * n_times), (int)n_split);
  }
  if (n_times == 0) return RYD_OK;
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int n_ty = std::min<int32_t>(n_times, 65535);
  const dim3 grid((unsigned)n_split, (unsigned)n_ty);
  cplx* dst = n_split == 1 ? (cplx*)out_dev : (cplx*)scratch_dev;
  const cplx* x = (const cplx*)states_dev;
  bool launched = false;
#define PTRACE_DM_CASE(LD_, K_, U_)                                                                                  \
  if (local_dim == LD_ && K == K_) {                                                                                 \
    ptrace_dm_launch<LD_, K_, U_>(grid, st, x, (int)n_times, (int)n_batch, (long long)stride_t, (long long)stride_b, \
                                  g, (int)n_split, dst);                                                             \
    launched = true;                                                                                                 \
  }
  PTRACE_DM_CASE(2, 1, 8) PTRACE_DM_CASE(2, 4, 2) PTRACE_DM_CASE(2, 16, 1)
  PTRACE_DM_CASE(3, 1, 8) PTRACE_DM_CASE(3, 4, 2)
  PTRACE_DM_CASE(4, 1, 8) PTRACE_DM_CASE(4, 16, 1)
#undef PTRACE_DM_CASE
  if (!launched)  // (never a silent RYD_OK: every reachable (local_dim, K) has a case above)
    return fail(RYD_ERR_INVALID, "reduced_density_dm: no kernel for local_dim %d with %d rows", (int)local_dim, dA);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_ptrace_dm: %s", hipGetErrorString(e));
  if (n_split > 1) {
    hipLaunchKernelGGL(k_ptrace_dm_sum, dim3((unsigned)((dA2 + 255) / 256), (unsigned)n_ty), dim3(256), 0, st,
                       (const cplx*)scratch_dev, (int)n_times, (int)n_split, dA2, (cplx*)out_dev);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_ptrace_dm_sum: %s", hipGetErrorString(e));
  }
  return RYD_OK;
}

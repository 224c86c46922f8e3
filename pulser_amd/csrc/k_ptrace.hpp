// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// ryd_reduced_density: out[i][a][a'] += sum_b sum_r psi(i, b)[idx(a, r)] conj psi(i, b)[idx(a', r)] - the partial trace
// rho_A = Tr_rest |psi><psi| of every stored ket over a small set A of atoms, summed over the trajectory axis
// ---------------------------------------------------------------------------
// What Qobj.ptrace(sel) computes of the states the emulator hands out, without the states leaving the device.  With the
// ket viewed as a dA x R matrix M (rows: configurations of the kept atoms, columns: configurations of the rest),
// rho_A = M M^dagger: the GEMM-shaped operation of k_outer_mfma (k_small.hpp) with "trajectory" replaced by
// "configuration of the rest", on v_mfma_f64_16x16x4_f64 with the same operand trick
//   Re = X X^T + Y Y^T,  Im = Y X^T - X Y^T:  A_re = (x, y, x', y'), A_im = (y, -x, y', -x'), B = (x, y, x', y'),
// two columns r, r' per K = 4.
//
// Tiling.  A workgroup of 256 threads (4 waves) owns one (time i, split s) and walks the trajectories b and the tiles of
// its share of the r range.  A tile is the kept sites plus the lowest free sites: dA x KC amplitudes, at most 2048.  The
// threads walk a tile in MEMORY order (its digits sorted by stride, lowest fastest): site n-1 is always in the tile (kept,
// or the lowest free site), so whatever `keep` is a wave reads runs of consecutive amplitudes, one global_load_dwordx4
// per lane, up to 8 per thread in flight; the tile after it is fetched into registers while this one is multiplied.
// Where a thread's amplitudes sit inside a tile (global offset, LDS slot) is the same for every tile: the digit
// arithmetic runs once per workgroup (32-bit, by the compile-time local dimension LD - no division in the loop), and a
// tile's base offset costs one uniform digit walk of its index per tile.
// Each amplitude goes to LDS at [r_local][a], row stride RS = dA | 1 amplitudes (odd: threads that are consecutive in r
// write 16-byte slots of different banks); the transposition happens there.  Rows beyond dA of the 16 NT-row operand
// (NT = ceil(dA / 16)) and the odd column of a tile with an odd column count are ZEROS made in registers, never read:
// nothing of the padding exists in memory, so nothing of it can leak.
// Up to 8 rows (dA <= 8) leave most of a 16-row operand empty: G = 16 / dA column groups then share it (operand row
// g dA + a is row a of the columns of group g), one MFMA multiplies 2 G columns, and only the G diagonal dA x dA blocks of
// its result are read - they are added in the order g = 0 .. G - 1 when the accumulators leave.  Without this the
// one- and two-qubit calls were bound by the matrix pipe at a ninth of the HBM rate (profiles/reduced_density.md).
// Each wave multiplies every fourth column pair of the tile into ALL 16 x 16 blocks on or above the diagonal
// (NT (NT + 1) / 2 blocks, real and imaginary accumulator each); the accumulators stay in registers across tiles and
// trajectories and leave once: block by block the four waves' partial sums are added through LDS in the order wave
// 0, 1, 2, 3 (inside each column group), and the sum is added onto `out` (n_split = 1) or stored to this split's
// partial (n_split > 1), which k_ptrace_sum then adds onto `out` in the order split 0 .. n_split - 1.
//
// Summation order: fixed by (dim, keep, n_batch, n_split) alone - no atomics, nothing that depends on timing.  Two calls
// with the same n_split are bitwise equal.  Hermiticity is exact by construction: only entries with row <= col are
// taken from the accumulators; [col][row] receives (re, -im) of the SAME numbers, and a diagonal entry's imaginary part
// (which the MFMA would leave as rounding noise y x - x y) is never added.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), LDS 40 960 B per workgroup
// (2560 amplitudes: KC RS <= 2560; the cross-wave sums reuse 16 KiB of it) -> 3 workgroups per CU by LDS:
//   k_ptrace<2|3|4, 1>: 120 VGPRs +  20 AGPRs, 97-98 SGPRs,   no scratch: 3 waves per SIMD (registers and LDS alike)
//   k_ptrace<2|3,   2>: 123 VGPRs +  52 AGPRs, 105-106 SGPRs, no scratch: 2 waves per SIMD
//   k_ptrace<2|4,   4>: 124 VGPRs + 164 AGPRs, 106 SGPRs,     no scratch: 1 wave per SIMD (20 accumulators of 8 registers;
//                       held to 256 registers for two waves the compiler spills 96 bytes per lane, so it is not)
//   k_ptrace_sum:        24 VGPRs, no LDS, no scratch
// Measured on MI355X (profiles/reduced_density.md): 3 101 kets of 14 atoms are read at 3.1 - 3.9 TB/s for dA = 2 .. 16
// wherever the kept sites sit; dA = 64 is bound by the matrix pipe at one wave per SIMD (28 TFLOP/s of MFMAs issued).
constexpr int kPtraceTile = 2048;      // amplitudes of a tile at most
constexpr int kPtraceLds = 2560;       // amplitudes of the LDS image at most (KC * RS)
constexpr int kPtracePer = kPtraceTile / 256;
constexpr int kPtraceTileSites = 11;   // 2^11 = 2048
constexpr int kPtraceOuterSites = 40;
constexpr int kPtraceTargetWgs = 1024; // what n_split = 0 aims at: 4 workgroups per CU

struct PtraceGeom {
  int tile_stride[kPtraceTileSites];          // stride of the tile's j-th digit in the ket, lowest stride first
  long long outer_stride[kPtraceOuterSites];  // stride of the j-th free site outside the tile, lowest first
  int tile_lw[kPtraceTileSites];              // what a unit of the tile's j-th digit adds to the LDS slot
  int n_tile, n_outer_sites;
  int E, KC, RS, dA;                          // tile amplitudes, tile columns, LDS row stride, rows
  int G;                                      // column groups that share the 16 operand rows (16 / dA; 1 from dA = 9 on)
  unsigned n_outer;                           // tiles per ket
};

template <int LD, int NT>
__global__ __launch_bounds__(256) void k_ptrace(const cplx* __restrict__ states, int n_times, int n_batch,
                                                long long stride_t, long long stride_b, const PtraceGeom g,
                                                int n_split, cplx* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) cplx lds[kPtraceLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;  // operand row / column, k slot: column (lk >> 1) of the pair, component lk & 1

  // where this thread's amplitudes of a tile sit: the same for every tile
  int goff[kPtracePer];  // (inside one ket: below dim < 2^31)
  int slot[kPtracePer];
#pragma unroll
  for (int it = 0; it < kPtracePer; ++it) {
    unsigned e = tid + it * 256;
    goff[it] = -1;
    slot[it] = 0;
    if ((int)e < g.E) {
      int off = 0, s = 0;
      for (int j = 0; j < g.n_tile; ++j) {
        const unsigned q = e / LD, dg = e - q * LD;
        off += (int)dg * g.tile_stride[j];
        s += (int)dg * g.tile_lw[j];
        e = q;
      }
      goff[it] = off;
      slot[it] = s;
    }
  }
  const int split = blockIdx.x;
  const unsigned o0 = (unsigned)((unsigned long long)g.n_outer * split / n_split);
  const unsigned o1 = (unsigned)((unsigned long long)g.n_outer * (split + 1) / n_split);
  const int dA = g.dA, G = g.G;
  const int npairs = (g.KC + 2 * G - 1) / (2 * G);
  // operand row li of a one-block matrix (NT = 1): row ai of column group gi - G columns share one MFMA operand, the
  // products between different groups land in result entries that are never read
  const int gi = NT == 1 ? li / dA : 0, ai = NT == 1 ? li - gi * dA : li;

  for (long long i = blockIdx.y; i < n_times; i += gridDim.y) {
    mfma_d4 cre[NT][NT], cim[NT][NT];  // (only rb <= cb are used)
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        cre[r][c] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
        cim[r][c] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
      }
    cplx v[kPtracePer];
    auto fetch = [&](int b, unsigned o) {
      long long base = i * stride_t + (long long)b * stride_b;
      for (int j = 0; j < g.n_outer_sites; ++j) {
        const unsigned q = o / LD;
        base += (long long)(o - q * LD) * g.outer_stride[j];
        o = q;
      }
      const cplx* p = states + base;
#pragma unroll
      for (int it = 0; it < kPtracePer; ++it) {
        v[it] = make_double2(0.0, 0.0);
        if (goff[it] >= 0) v[it] = p[goff[it]];
      }
    };
    int b = 0;
    unsigned o = o0;
    bool have = o0 < o1;
    if (have) fetch(b, o);
    while (have) {
      __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
      for (int it = 0; it < kPtracePer; ++it)
        if (goff[it] >= 0) lds[slot[it]] = v[it];
      __syncthreads();
      if (++o == o1) {
        o = o0;
        ++b;
      }
      have = b < n_batch;
      if (have) fetch(b, o);
      for (int p = wave; p < npairs; p += 4) {
        const int col = (2 * p + (lk >> 1)) * G + gi, comp = lk & 1;
        double are[NT], aim[NT];
#pragma unroll
        for (int r = 0; r < NT; ++r) {
          const int a = 16 * r + ai;
          cplx w = make_double2(0.0, 0.0);
          if (col < g.KC && (NT == 1 ? gi < G : a < dA)) w = lds[col * g.RS + a];
          are[r] = comp ? w.y : w.x;
          aim[r] = comp ? -w.x : w.y;  // (y, -x)
        }
#pragma unroll
        for (int r = 0; r < NT; ++r)
#pragma unroll
          for (int c = r; c < NT; ++c) {
            cre[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(are[r], are[c], cre[r][c], 0, 0, 0);
            cim[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim[r], are[c], cim[r][c], 0, 0, 0);
          }
      }
    }
    // the four waves' sums, block by block, in the order wave 0, 1, 2, 3; result lane map of the f64 MFMA:
    // col = lane & 15, row = (lane >> 4) + 4 * reg.  Thread (gq = tid >> 6, lane) owns register gq of the block.
    cplx* tgt = dst + (n_split == 1 ? i : i * n_split + split) * (long long)(dA * dA);
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
      for (int c = r; c < NT; ++c) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) lds[(wave * 4 + q) * 64 + lane] = make_double2(cre[r][c][q], cim[r][c][q]);
        __syncthreads();
        // thread (r16, c16) owns one entry of the block: the sum over the column groups and, inside, over the waves;
        // entry (row, col) of wave w's block sits in register row >> 2 of lane (row & 3) * 16 + col
        const int r16 = tid >> 4, c16 = tid & 15;
        const int row = 16 * r + r16, cl = 16 * c + c16;
        cplx s = make_double2(0.0, 0.0);
        if (row < dA && cl < dA && row <= cl) {
          for (int gg = 0; gg < G; ++gg) {
            const int rl = gg * dA + r16, cc = gg * dA + c16;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const cplx t = lds[(w * 4 + (rl >> 2)) * 64 + (rl & 3) * 16 + cc];
              s.x += t.x;
              s.y += t.y;
            }
          }
        }
        if (row < dA && cl < dA && row <= cl) {
          if (n_split != 1) {
            tgt[row * dA + cl] = make_double2(s.x, row == cl ? 0.0 : s.y);
          } else if (row == cl) {
            tgt[row * dA + cl].x += s.x;
          } else {
            const cplx up = tgt[row * dA + cl], lo = tgt[cl * dA + row];
            tgt[row * dA + cl] = make_double2(up.x + s.x, up.y + s.y);
            tgt[cl * dA + row] = make_double2(lo.x + s.x, lo.y - s.y);
          }
        }
      }
    __syncthreads();  // (the next time's tiles overwrite the LDS image)
  }
}

// out[i] += part[i][0] + part[i][1] + ... in that order; one thread per entry on or above the diagonal, which also
// writes the mirror entry from the same numbers.  blockIdx.y walks the times with stride gridDim.y.
__global__ __launch_bounds__(256) void k_ptrace_sum(const cplx* __restrict__ part, int n_times, int n_split, int dA,
                                                    cplx* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x, d2 = dA * dA;
  if (e >= d2) return;
  const int row = e / dA, cl = e - row * dA;
  if (row > cl) return;
  for (long long i = blockIdx.y; i < n_times; i += gridDim.y) {
    cplx* o = out + i * d2;
    const cplx* p = part + i * n_split * d2 + e;
    cplx up = o[e], lo = o[cl * dA + row];
    for (int s = 0; s < n_split; ++s) {
      const cplx t = p[(long long)s * d2];
      up.x += t.x;
      up.y += t.y;
      lo.x += t.x;
      lo.y -= t.y;
    }
    if (row == cl) {
      o[e].x = up.x;
    } else {
      o[e] = up;
      o[cl * dA + row] = lo;
    }
  }
}

template <int LD, int NT>
static void ptrace_launch(dim3 grid, hipStream_t stream, const cplx* states, int n_times, int n_batch,
                          long long stride_t, long long stride_b, const PtraceGeom& g, int n_split, cplx* dst) {
  hipLaunchKernelGGL((k_ptrace<LD, NT>), grid, dim3(256), 0, stream, states, n_times, n_batch, stride_t, stride_b, g,
                     n_split, dst);
}

extern "C" int ryd_reduced_density(const void* states_dev, int32_t n_times, int32_t n_batch, int64_t stride_t,
                                   int64_t stride_b, int64_t dim, int32_t local_dim, int32_t n_sites,
                                   const int32_t* keep, int32_t n_keep, void* out_dev, int32_t n_split,
                                   void* scratch_dev, int64_t scratch_bytes, int32_t device, void* stream) {
  if (n_times < 0) return fail(RYD_ERR_INVALID, "reduced_density: n_times %d is negative", (int)n_times);
  if (n_batch < 1) return fail(RYD_ERR_INVALID, "reduced_density: n_batch %d is smaller than 1", (int)n_batch);
  if (local_dim < 2 || local_dim > 4)
    return fail(RYD_ERR_INVALID, "reduced_density: local_dim %d is not 2, 3 or 4", (int)local_dim);
  if (n_sites < 1 || n_sites > 62) return fail(RYD_ERR_INVALID, "reduced_density: n_sites %d is not in 1..62", (int)n_sites);
  int64_t want = 1;
  for (int k = 0; k < n_sites; ++k) {
    if (want > INT64_MAX / local_dim) return fail(RYD_ERR_INVALID, "reduced_density: local_dim^n_sites overflows");
    want *= local_dim;
  }
  if (dim != want)
    return fail(RYD_ERR_INVALID, "reduced_density: dim %lld is not local_dim^n_sites = %d^%d", (long long)dim,
                (int)local_dim, (int)n_sites);
  if (stride_t < dim || stride_b < dim)
    return fail(RYD_ERR_INVALID, "reduced_density: strides %lld / %lld are smaller than a ket of dim %lld",
                (long long)stride_t, (long long)stride_b, (long long)dim);
  if (!keep) return fail(RYD_ERR_INVALID, "reduced_density: keep is null");
  if (n_keep < 1 || n_keep > n_sites)
    return fail(RYD_ERR_INVALID, "reduced_density: n_keep %d is not in 1..n_sites = %d", (int)n_keep, (int)n_sites);
  for (int k = 0; k < n_keep; ++k)
    if (keep[k] < 0 || keep[k] >= n_sites || (k > 0 && keep[k] <= keep[k - 1]))
      return fail(RYD_ERR_INVALID, "reduced_density: keep[%d] = %d is out of range or not strictly ascending", k,
                  (int)keep[k]);
  int64_t dA64 = 1;
  for (int k = 0; k < n_keep && dA64 <= 64; ++k) dA64 *= local_dim;
  if (dA64 > 64)
    return fail(RYD_ERR_INVALID, "reduced_density: %d kept sites of local dimension %d exceed 64 rows", (int)n_keep,
                (int)local_dim);
  if (n_split < 0) return fail(RYD_ERR_INVALID, "reduced_density: n_split %d is negative", (int)n_split);
  if (scratch_bytes < 0) return fail(RYD_ERR_INVALID, "reduced_density: scratch_bytes is negative");
  if (!states_dev) return fail(RYD_ERR_INVALID, "reduced_density: states_dev is null");
  if (!out_dev) return fail(RYD_ERR_INVALID, "reduced_density: out_dev is null");
  const int dA = (int)dA64;
  const int64_t part_bytes = (int64_t)dA * dA * (int64_t)sizeof(cplx);  // one (time, split) partial

  // the tile: every kept site and the lowest free sites that fit
  PtraceGeom g{};
  g.dA = dA;
  g.RS = dA | 1;
  g.G = dA <= 8 ? 16 / dA : 1;
  if (dim > INT32_MAX) return fail(RYD_ERR_INVALID, "reduced_density: dim %lld is too large", (long long)dim);
  std::vector<char> kept(n_sites, 0);
  for (int k = 0; k < n_keep; ++k) kept[keep[k]] = 1;
  const int n_free = n_sites - n_keep;
  int nf_tile = 0, KC = 1;
  while (nf_tile < n_free && (int64_t)dA * KC * local_dim <= kPtraceTile && (int64_t)g.RS * KC * local_dim <= kPtraceLds) {
    KC *= local_dim;
    ++nf_tile;
  }
  g.KC = KC;
  g.E = dA * KC;
  int64_t a_w = 1, r_w = 1, n_outer = 1;
  int free_seen = 0;
  std::vector<int64_t> stride(n_sites);
  {
    int64_t s = 1;
    for (int k = n_sites - 1; k >= 0; --k, s *= local_dim) stride[k] = s;
  }
  for (int k = n_sites - 1; k >= 0; --k) {  // lowest stride first
    if (kept[k]) {
      g.tile_stride[g.n_tile] = (int)stride[k];
      g.tile_lw[g.n_tile++] = (int)a_w;
      a_w *= local_dim;
    } else if (free_seen < nf_tile) {
      g.tile_stride[g.n_tile] = (int)stride[k];
      g.tile_lw[g.n_tile++] = (int)(r_w * g.RS);
      r_w *= local_dim;
      ++free_seen;
    } else {
      if (g.n_outer_sites >= kPtraceOuterSites || n_outer > INT32_MAX / local_dim)
        return fail(RYD_ERR_INVALID, "reduced_density: dim %lld is too large", (long long)dim);
      g.outer_stride[g.n_outer_sites++] = stride[k];
      n_outer *= local_dim;
    }
  }
  g.n_outer = (unsigned)n_outer;
  if (g.n_tile > kPtraceTileSites || g.E > kPtraceTile || (int64_t)g.KC * g.RS > kPtraceLds)
    return fail(RYD_ERR_INVALID, "reduced_density: internal tile geometry error");

  if (n_split == 0) {
    // enough workgroups to fill the device, every split with at least four tiles and with at least as many bytes to
    // read as its partial has to write and read back; never more than the scratch given holds
    const int64_t min_tiles = std::max<int64_t>(4, ((int64_t)dA * dA * 4 + g.E - 1) / g.E);
    int64_t s = std::min<int64_t>(kPtraceTargetWgs / std::max<int32_t>(n_times, 1), n_outer / min_tiles);
    if (n_times > 0 && scratch_dev) s = std::min<int64_t>(s, scratch_bytes / (part_bytes * n_times));
    else s = 1;
    n_split = (int32_t)std::max<int64_t>(s, 1);
  } else if (n_split > 1) {
    if (!scratch_dev) return fail(RYD_ERR_INVALID, "reduced_density: n_split %d needs scratch_dev", (int)n_split);
    if (n_split > 65535) return fail(RYD_ERR_INVALID, "reduced_density: n_split %d exceeds 65535", (int)n_split);
    if (scratch_bytes / part_bytes / n_split < n_times)
      return fail(RYD_ERR_INVALID, "reduced_density: scratch of %lld bytes is smaller than the %lld needed by n_split %d",
                  (long long)scratch_bytes, (long long)(part_bytes * n_split * n_times), (int)n_split);
  }
  if (n_times == 0) return RYD_OK;
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int n_ty = std::min<int32_t>(n_times, 65535);
  const dim3 grid((unsigned)n_split, (unsigned)n_ty);
  cplx* dst = n_split == 1 ? (cplx*)out_dev : (cplx*)scratch_dev;
  const cplx* x = (const cplx*)states_dev;
  const int NT = (dA + 15) / 16;
#define PTRACE_CASE(LD_, NT_)                                                                                \
  if (local_dim == LD_ && NT == NT_)                                                                         \
    ptrace_launch<LD_, NT_>(grid, st, x, (int)n_times, (int)n_batch, (long long)stride_t, (long long)stride_b, g, \
                            (int)n_split, dst);
  PTRACE_CASE(2, 1) PTRACE_CASE(2, 2) PTRACE_CASE(2, 4)
  PTRACE_CASE(3, 1) PTRACE_CASE(3, 2)
  PTRACE_CASE(4, 1) PTRACE_CASE(4, 4)
#undef PTRACE_CASE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_ptrace: %s", hipGetErrorString(e));
  if (n_split > 1) {
    hipLaunchKernelGGL(k_ptrace_sum, dim3((unsigned)((dA * dA + 255) / 256), (unsigned)n_ty), dim3(256), 0, st,
                       (const cplx*)scratch_dev, (int)n_times, (int)n_split, dA, (cplx*)out_dev);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(RYD_ERR_HIP, "k_ptrace_sum: %s", hipGetErrorString(e));
  }
  return RYD_OK;
}

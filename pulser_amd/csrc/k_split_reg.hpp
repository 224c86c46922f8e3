// Part of librydemu (included by rydemu.hip, one translation unit).
// ---------------------------------------------------------------------------
// k_split_reg<N, NR>: register-resident split-operator kets, 2^NR amplitudes per lane (round 4)
// ---------------------------------------------------------------------------
// Same seam, composition, coefficient tables and step-size controller as k_split14_loop (k_split.hpp; the call
// replaced is qutip.sesolve behind simulation.py:729-735): one workgroup per sequence holds the whole ket in registers
// over every stage of a closed run.  Positions of the N index bits: NR register bits, 6 lane bits, NW = N - 6 - NR
// wave bits (64 << NW lanes).  A stage = D (phase) + the N single-atom rotations; every rotation is done where its bit
// is cheapest to reach:
//   * register bits: plain FMAs (tan form: x' = x - T y_p, y' = y + T x_p, the same formula on both partners);
//   * the low ND = 6 - (NR - NW) lane bits: the partner comes over the DPP crossbar (quad permutes, row rotate by 8,
//     row (half) mirror: every bit's direction is ONE pattern, SPLITR_HM) - no layout change, no LDS; for a real drive
//     only the imaginary parts travel, as a chain of hops from direction to direction (SPLITR_YCHAIN, split_ychain.hpp);
//   * the upper NTB = NR - NW lane bits: an INTRA-WAVE transposition through LDS exchanges them with the register bits
//     NW .. NR-1 ("T bits").  A wave only reads what it wrote itself: no barrier, only the LDS queue's own order, so
//     the waves of a workgroup drift apart and the transposition of one overlaps the FMAs of another (and, inside a
//     wave, the next group's phase factors);
//   * the NW wave bits: one pass through LDS per stage exchanges them with register bits 0 .. NW-1, in four chunks
//     (the top two T bits fixed) through two buffers: 4 workgroup barriers per stage, the next chunk's rotations issue
//     while the LDS absorbs the current chunk's stores.  Lane bits do not take part: every ds_write_b128 /
//     ds_read_b128 of a wave covers 1 KiB of consecutive addresses.
// After a stage the T bits and the upper lane bits have changed places, and so have the wave bits and the low register
// bits: layouts alternate with period 2.  The code of a stage only knows POSITIONS; which atom's coefficient belongs
// to a position is decided when the stage's coefficients are loaded (scalar loads, parity of the stage), and the E0
// pieces of the two layouts are selected by parity - ONE stage body in the loop (half the instruction footprint of
// even / odd copies).  The closing stage of a run (D only: its rotation angles are zero, tan = 0) runs the same body, so a
// run may end in either layout; the store addresses follow.
// Phase factors: E0 is pairwise additive, so for lane t and register r
//   exp(-i phi) = B(t) G(r) prod_{j excited in r} F_j(t),
// B = the lane's atoms alone (+ their detunings, + the cosines of the previous stage's tan-form rotations), F_j =
// register atom j against the lane's excited atoms (+ its detuning), G = the register atoms among themselves (uniform:
// lane r of every wave computes G(r) into a wave-private LDS table, read back as broadcasts): NR + 2 table-and-series
// sin / cos per lane and stage, then one complex multiplication per amplitude down a product tree, the uniform factor,
// and the amplitude itself.
// Roofline: fp64 vector pipe (the ket never leaves the CU between the first load and the last store).

#ifndef SPLITR_TRIG
#define SPLITR_TRIG 256  /* phase table entries: exp(2 pi i k / SPLITR_TRIG) */
#endif
// dev probe (tools/lane_variants.sh): knock out one component of the stage (wrong results, timing only)
//   1 the intra-wave transposition, 2 lane-bit rotations (DPP), 4 the LDS pass and its barriers, 8 phase,
//   16 register rotations
#ifndef SPLITR_KO
#define SPLITR_KO 0
#endif
// A/B switches (dev builds, profiles/r04_ksplit14_variants.md):
//   SPLITR_TMODE 1: lane bits 4, 5 by v_permlane16_swap / v_permlane32_swap instead of the LDS transposition (NTB == 2);
//                2: the LDS transposition, D first and half of the DPP rotations as its filler;
//                3: no exchange: partners of lane bits 4, 5 over the LDS crossbar (ds_swizzle / ds_bpermute; NTB == 2)
//   SPLITR_GMODE 1: the uniform factor G(r) by v_readlane from the lane that computed it instead of the LDS table
//   SPLITR_WMODE 1: the stages' E0 weights from an LDS table filled at launch (no kernel-argument loads per stage)
#ifndef SPLITR_TMODE
#define SPLITR_TMODE 1
#endif
#ifndef SPLITR_GMODE
#define SPLITR_GMODE 0
#endif
#ifndef SPLITR_WMODE
#define SPLITR_WMODE 1
#endif
//   SPLITR_EMODE 1: the per-lane E0 pieces et / eg of both layouts in LDS (read once per stage) instead of 8 registers
//   SPLITR_KWARM: the next stage's coefficient record (written by k_split_coefs, never read by this CU: a cold miss) is
//                touched half a stage ahead (profiles/stage_waits.md)
//                1: one scalar load per 64-B line right behind the first barrier of the pass, folded on the spot: every
//                   wave of the workgroup waits out the miss there, a few cycles after they all left the same barrier;
//                2 (default): the same loads behind the phase factors of the last group, folded only in front of the
//                   pass's first barrier: ~460 vector instructions without an LDS read or a scalar load lie in between
//                   (scalar loads return out of order, so ANY wait on the LDS / scalar counter while a touch is in flight
//                   is a full wait - the placement is the point; between the group loop and pre(C0), fenced on both sides,
//                   they cost more than half of the gain);
//                3: ONE vector load per wave at the same place, lane k on line k: warms the L2 only, its value is
//                   consumed a stage later (the vector counter: no wait inside the stage)
//   SPLITR_PREF  1: the detuning integrals and the E0 weight of the NEXT stage are loaded at the end of a stage
#ifndef SPLITR_EMODE
#define SPLITR_EMODE 0
#endif
#ifndef SPLITR_KWARM
#define SPLITR_KWARM 2
#endif
//   SPLITR_GAHEAD (SPLITR_TMODE 1 with two T bits, SPLITR_GMODE 0; profiles/stage_waits.md): the LDS reads of the phase
//                factors are issued long before their values are needed instead of 4 - 8 fp64 instructions ahead:
//                0: G(r) is read where phase_group uses it, the table entry of an expmi inside it;
//                1 (default): the seven table reads of the stage's expmi are issued as soon as their indices exist,
//                   in front of the series of all seven; G's own factor comes first, so that the four G values of the first
//                   group are read behind it and arrive under the six other series; the four G values of group g - 1 are
//                   read at the start of group g's work into registers of their own (16 on top of the 229);
//                2: the G values of group g - 1 are read behind group g's phase factors (no second set of G registers)
//                Complex drives and the row kernels keep the old order (256 vector registers without it).
#ifndef SPLITR_GAHEAD
#define SPLITR_GAHEAD 1
#endif
#ifndef SPLITR_PREF
#define SPLITR_PREF 0
#endif
//   SPLITR_LATE 1: complex drives: the rotation coefficients are loaded after the phase factors (scalar register pressure)
#ifndef SPLITR_LATE
#define SPLITR_LATE 1
#endif
//   SPLITR_XPASS 1 (default; the plain real-drive kernels with two T bits and wave bits, <14, 5> and <12, 4>, and the SNAP twin
//                of <12, 4> - splitr_xpass() below; profiles/xpass.md): lane bits 4, 5 change places with the two T bits INSIDE the LDS pass instead of by
//                128 v_permlane16/32_swap per stage.  Convention: the register NAMED with T bits (s0, s1) holds, on a lane with bits
//                (l4, l5), the amplitude whose T-position index bits are (s0 ^ l4, s1 ^ l5).  The exchange is then: reader lane l
//                fills its registers named (s0, s1) from the registers of the same name of lane l ^ (s0 << 4 | s1 << 5) - a constant
//                per chunk, chunk (0, 0) reads its own lane, the four chunks, the two buffers and the 4 barriers stay, and every
//                16-lane group of a ds_read_b128 still covers 256 consecutive bytes.  The convention reproduces itself: writer lane
//                bit a' = s ^ a holds (T position P = a', lane position Q = a); the reader with l5 = a gets lane-position bit Q = a
//                and T bit P = s ^ a, named s again.  What follows from it:
//                  * addresses (load, store, snapshot, check epilogue) are "lane word XOR register constant": SplitRegLayout::index_x;
//                  * tan-form rotations use one formula on both partners, so a rotation of a T bit does not care which name is which;
//                    the two atoms that arrive from lane bits 4, 5 are rotated AFTER the pass, as soon as their pairs of chunks are in;
//                  * phase factors stay decomposed in ACTUAL excitation bits: on a lane whose T bit j is flipped the product tree
//                    runs over named bits with F'_j = 1 / F_j and B' = B F_j - done on the arguments: ev'_j = -ev_j, et' = et +
//                    sum of the flipped ev_j (per-lane constants of the prologue), the sign of Dr[j] by an integer XOR, and in the
//                    lane's detuning sum the terms of lane bits 4, 5 select between two scalars (l5 ? Dr[T1] : Dl[5]: the T-position
//                    atom and its lane-position partner contribute under complementary conditions - one select, one addition);
//                  * G(r) is uniform in actual bits: a lane reads G[r ^ c], c = l4 << NW | l5 << (NW + 1); every wave writes its table
//                    four times, permuted (copy c holds G[r ^ c] at slot r, copies one slot apart in the banks: a 16-lane read group
//                    meets two copies), and the 2^NR reads stay reads at offsets 16 k on one address register.
//                0: the swaps (A/B)
#ifndef SPLITR_XPASS
#define SPLITR_XPASS 1
#endif
#ifndef SPLITR_LATE_REAL
#define SPLITR_LATE_REAL 0  /* the same for real drives (A/B) */
#endif
//   SPLITR_YCHAIN (real drives, SPLITR_TMODE 1, SPLITR_HM 1, no SPLITR_B2; profiles/ychain.md):
//                0: every DPP lane bit fetches both parts of its partner (4 moves per amplitude and bit); the stores of the
//                   pass are issued in one block;
//                1 (default): the rotation of a DPP bit is two real rotations on the pairs (x(L), y(L ^ m)) and (x(L ^ m), y(L)),
//                   so the lane keeps its x, holds the partner's y and does both FMAs itself - the same FMAs on the same
//                   operands, bit for bit the same results; only y travels, from direction to direction (hop plan:
//                   split_ychain.hpp), and comes home after the last rotation: 12 moves per amplitude instead of 16 with four
//                   DPP bits.  The chain runs hop by hop over a chunk, and the stores of the previous chunk are spread over
//                   its steps (write_pre below) - that, not the moves, is most of what was measured;
//                2: the way home rides on the LDS pass instead (NW > 0): pass_write stores x to the lane's own
//                   slot and y to the slot of the lane it belongs to (same wave, same 8-lane group, before the same barrier):
//                   10 moves per amplitude, but two 8-byte stores per amplitude, 2-way bank conflicts each (measured: not
//                   faster than 1 beyond the noise)
#ifndef SPLITR_YCHAIN
#define SPLITR_YCHAIN 1
#endif
#include "split_ychain.hpp"

template <int N, int NR>
struct SplitRegLayout {
  static constexpr int NW = N - 6 - NR;   // wave bits
  static constexpr int NTB = NR - NW;     // register bits exchanged with lane bits inside a wave
  static constexpr int ND = 6 - NTB;      // lane bits served by the DPP crossbar
  static_assert(NW >= 0 && NW <= 3 && NTB >= 2 && ND >= 1 && ND <= 4, "unsupported shape");
  // index bit held by a position at the start of an even / odd stage
  // (SPLITR_TMODE 3: the T registers and the upper lane bits never change places - those lane bits get their rotation
  // through partner fetches over the LDS crossbar)
  static constexpr bool kXchg = SPLITR_TMODE != 3;
  __host__ __device__ static constexpr int regbit(bool odd, int j) {
    if (!odd) return 6 + NW + j;
    return j < NW ? 6 + j : (kXchg ? ND + (j - NW) : 6 + NW + j);
  }
  __host__ __device__ static constexpr int lanebit(bool odd, int j) {
    if (j < ND || !odd || !kXchg) return j;
    return 6 + 2 * NW + (j - ND);
  }
  __host__ __device__ static constexpr int wavebit(bool odd, int j) { return odd ? 6 + NW + j : 6 + j; }
  __host__ __device__ static constexpr unsigned index(bool odd, unsigned t, unsigned r) {
    unsigned i = 0;
    for (int j = 0; j < 6; ++j) i |= ((t >> j) & 1u) << lanebit(odd, j);
    for (int j = 0; j < NW; ++j) i |= ((t >> (6 + j)) & 1u) << wavebit(odd, j);
    for (int j = 0; j < NR; ++j) i |= ((r >> j) & 1u) << regbit(odd, j);
    return i;
  }
  // SPLITR_XPASS: the same map where a T register bit named s holds the T-position bit s ^ (the lane's bit ND + m): the lane's
  // word carries its upper lane bits a second time, on the T positions, and the register's bits are XORed onto it
  __host__ __device__ static constexpr unsigned index_x(bool odd, unsigned t, unsigned r) {
    unsigned i = index(odd, t, r);
    for (int m = 0; m < NTB; ++m) i ^= ((t >> (ND + m)) & 1u) << regbit(odd, NW + m);
    return i;
  }
  // ... as the kernel computes it: the lane's word lw = index_x(odd, t, 0) XOR the named T bits, plus the other register bits
  // (constants per register; SplitXAddrCheck below sweeps every lane and register of both parities at compile time)
  __host__ __device__ static constexpr unsigned addr_x(bool odd, unsigned lw, unsigned r) {
    constexpr unsigned tmask = ((1u << NTB) - 1u) << NW;
    return (lw ^ index(odd, 0u, r & tmask)) + index(odd, 0u, r & ~tmask);
  }
  // swizzle of the intra-wave transposition: slot of (low lane bits a, X, run Y) = a + 2^ND (X ^ (Y & FM)); chosen so
  // that the 16-lane groups of a ds_read_b128 and the 8-lane groups of a ds_write_b128 meet 16 different bank quads
  // (tools/lane_layout_check.py replays the bank rules of the guide for every instantiated shape)
  static constexpr int FM = ND == 4 ? 0 : (ND == 3 ? 2 : 3);
  __host__ __device__ static constexpr int swz(int y) { return ND == 3 ? ((y >> 1) & 1) : (y & FM); }
};

// SPLITR_XPASS: the instantiations whose lane bits 4, 5 change places with the T bits inside the pass, and the slots of 16 bytes
// their G tables take per wave (four copies, NA + 1 slots apart) - the kernel's carve-up of the LDS and the host's request
// (host_split.hpp: launch_split_reg) both come from here
// (SNAP at 32 amplitudes per lane keeps the swaps: with the snapshot store in the loop the kernel sits at 256 vector registers
// without scratch only with them; at 16 amplitudes per lane the snapshot twin takes the exchange like the plain kernel)
template <int N, int NR>
__host__ __device__ constexpr bool splitr_xpass(bool decay, bool rows, bool cplx, bool snap) {
  return SPLITR_XPASS != 0 && SPLITR_TMODE == 1 && SplitRegLayout<N, NR>::NTB == 2 && SplitRegLayout<N, NR>::NW > 0 && !decay && !rows &&
         !cplx && !(snap && NR >= 5) && !SPLITR_GMODE && !(SPLITR_KO & 4);
}
template <int N, int NR>
__host__ __device__ constexpr int splitr_gtab_slots(bool decay, bool rows, bool cplx, bool snap) {
  return splitr_xpass<N, NR>(decay, rows, cplx, snap) ? 4 * ((1 << NR) + 1) : (1 << NR);
}

template <int N, int NR>
constexpr bool splitr_xaddr_ok(bool odd, unsigned r) {  // addr_x against index_x on every lane, register r
  typedef SplitRegLayout<N, NR> L;
  for (unsigned t = 0; t < (64u << L::NW); ++t)
    if (L::addr_x(odd, L::index_x(odd, t, 0u), r) != L::index_x(odd, t, r) || L::index_x(odd, t, r) >= (1u << N)) return false;
  return true;
}
template <int N, int NR, int R>
struct SplitXAddrCheck {  // (one assertion per register: each stays inside the compiler's budget of constant-expression steps)
  static_assert(splitr_xaddr_ok<N, NR>(false, R) && splitr_xaddr_ok<N, NR>(true, R),
                "SPLITR_XPASS: lane word XOR named T bits + the other register bits must be index_x, even and odd layout");
  static constexpr bool ok = SplitXAddrCheck<N, NR, R - 1>::ok;
};
template <int N, int NR>
struct SplitXAddrCheck<N, NR, -1> {
  static constexpr bool ok = true;
};

// compile-time loop: every register index below is a constant expression (runtime-trip loops with `continue` filters
// over 64 registers were left rolled by the unroller - 2 400 scratch instructions per stage - hence no loops at all)
template <int I, int E, class Fn>
__device__ __forceinline__ void splitr_for(Fn&& f) {
  if constexpr (I < E) {
    f(std::integral_constant<int, I>{});
    splitr_for<I + 1, E>(f);
  }
}
template <int V>
using splitr_c = std::integral_constant<int, V>;
__host__ __device__ constexpr int splitr_low_clear(int v) {
  int j = 0;
  while (v & (1 << j)) ++j;
  return j;
}

template <int CTRL>
__device__ __forceinline__ double splitr_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
//   SPLITR_B2 1: the partner of lane bit 2 (xor 4: no single DPP pattern - two dependent v_mov_dpp per dword) over the LDS
//                crossbar instead (ds_swizzle, xor mask 4: no vector-pipe cycles beyond the issue) - round-5 variant
#ifndef SPLITR_B2
#define SPLITR_B2 0
#endif
//   SPLITR_HM 1 (round 6, default): the third DPP lane bit is the DIRECTION xor 7 of the lane number instead of xor 4 - one
//                row_half_mirror move per dword where xor 4 takes two dependent ones (640 -> 512 DPP moves per stage at
//                32 amplitudes per lane).  {1, 2, 7, 8} is a basis of the 4-bit lane numbers of a row like {1, 2, 4, 8}: a lane
//                holds the index bits (b0, b1, b2) = (l0 ^ l2, l1 ^ l2, l2) on its three low positions - splitr_lane() below;
//                everything that asks "which index bits does this lane hold" goes through it, the LDS passes and the swaps
//                only ever pair a lane with itself or with lanes of the same low bits and do not care.
#ifndef SPLITR_HM
#define SPLITR_HM 1
#endif
// the lane / thread number whose BITS are the index bits a lane holds (positions as in SplitRegLayout)
// (only where lane bit 2 is a DPP bit, ND >= 3: with ND = 2 it is a T bit, the LDS transposition moves it, and the two low
// bits must not depend on it)
template <int ND>
__device__ __forceinline__ unsigned splitr_lane(unsigned t) { return (SPLITR_HM && ND >= 3) ? t ^ ((t & 4u) ? 3u : 0u) : t; }
template <int F>
__device__ __forceinline__ double splitr_partner(double v) {
  if constexpr (F == 0) return splitr_dpp<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (F == 1) return splitr_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  else if constexpr (F == 3) return splitr_dpp<0x128>(v);  // row_ror:8
  else if constexpr (SPLITR_HM == 1) return splitr_dpp<0x141>(v);  // row_half_mirror: xor 7 (F == 2 is only asked for with ND >= 3)
  else if constexpr (SPLITR_B2 == 1) {
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x101F);  // bit-mask mode: and 0x1F, or 0, xor 4
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x101F);
    return __hiloint2double(hi, lo);
  }
  else return splitr_dpp<0x1B>(splitr_dpp<0x141>(v));      // xor 4 = (xor 3) o (xor 7): row_half_mirror, quad reverse
}

// ROWS: the kets are the rows of a density matrix (the split-operator master equation of host_ket.hpp): blockIdx.z = the
// matrix, and the workgroups of a matrix are PERSISTENT - workgroup blockIdx.y takes the rows blockIdx.y, + gridDim.y, ...
// one after another (tables, E0 pieces and stage weights are set up once, and the store of a row overlaps the load of
// the next).  The coefficients and E0 of the matrix serve its 2^N rows, the propagator
// may be the complex conjugate one (SplitArgs.conj), the elementwise dissipator factors are applied at the load and /
// or the store (SplitArgs.ftab: exponentials of linear functions of the bit-pair counts, so the factor of an
// amplitude is (a factor of its lane) x (a factor of its register)), and the run may open with / close on the
// drive-only kick of the 4th-order splitting (SplitRun.kick_*).
// CPLX: complex drive coefficients (a pulse with a phase, local addressing with per-atom phases): the rotation of an atom
// is C (1 + u |1><0| - conj(u) |0><1|), u = (Re g + i Im g) / C (SplitRun.tan_form 2: both slots of the table) - 4 FMAs
// per amplitude and bit instead of 2; on the DPP bits the sign of the Re part depends on the lane's own bit.
// SNAP: evaluation-time snapshots inside the run (round 5): after the last stage of a sub-step s with R.snap[s] >= 0 the
// registers - the OPEN state, see SplitArgs.snaps - are stored to the snapshot slot; k_split_snap_close finishes them.  A
// front end that asks for the state at every knot (evaluation_times="Full", the reference's default, simulation.py:137)
// or at every 10th used to close a run - a launch, a load and a store of the ket, a closing stage - per evaluation time.
// SEG (k_split_reg_seg below; plain kets only): the run is a row of SEGMENTS (SplitRun.nseg, seg_end, seg_flags), each a
// closed run of its own - load or keep the registers, stage loop, closing stage, the sinks of the controller's check - one
// after another in ONE launch: a stretch, the double step of the step-size check behind it (out of place, from the registers
// the stretch has just stored) and the two regular sub-steps the check compares it with.  The trig table, the stage weights
// of all segments and the E0 pieces are set up once; the segment loop is the row loop of ROWS, and the stage body is the one
// of the plain kernel.  The kernel without segments is a separate instantiation of the same body and does not change.
// UNI (k_split_reg_uni, k_split_reg_seg_uni below; plain real-drive kets only): every atom of a sequence has the same drive
// and the same detuning (a Global channel: ryd_handle.desc_uniform), and the sequence's coefficients of a stage are ONE
// record of 32 bytes, [record][B][4] = (C^N, Im g / C, Im g, Delta) - k_split_coefs in its uniform mode: one scalar load per
// stage instead of 14 x (C, T, Delta), every position's T and Delta the same scalar, the cosine product of the stage read
// instead of multiplied up, and the lane's detuning sum Delta x (the number of its atoms in the excited state - a per-lane
// constant of the prologue) instead of a chain of selects and additions.  Everything else is the one stage body.
template <int N, int NR, bool DECAY, bool ROWS, bool CPLX, bool SNAP, bool SEG, bool UNI = false>
__device__ __forceinline__ void split_reg_body(const SplitArgs& A, const SplitRun& R, const long long stage_stride) {
  static_assert(!(SNAP && (ROWS || DECAY)), "snapshots inside a run: plain ket runs only");
  static_assert(!(SEG && (ROWS || DECAY || CPLX || SNAP)), "segments: plain real-drive ket runs only");
  static_assert(!(UNI && (ROWS || DECAY || CPLX || SNAP)), "one record per sequence: plain real-drive ket runs only");
  static_assert(!(UNI && (SPLITR_PREF || SPLITR_LATE_REAL)), "one record per sequence: loaded where the stage starts");
  // (the prefetch of the next stage's record starts at record 0 and flips the parity at every stage: it knows neither where a
  // segment starts nor that the closing stage keeps the layout)
  static_assert(!(SEG && SPLITR_PREF), "segments: SPLITR_PREF is not carried across segment boundaries");
  typedef SplitRegLayout<N, NR> L;
  constexpr int NW = L::NW, NTB = L::NTB, ND = L::ND;
  constexpr int NT = 64 << NW;
  constexpr int NA = 1 << NR;          // amplitudes per lane
  constexpr int PW = (1 << NW) - 1;    // register bits the pass exchanges
  constexpr int CH = NA / 4;           // registers per chunk of the pass (top two T bits fixed) = LDS runs per wave
  constexpr int NG = 1 << NW;          // groups of the transposition (pass bits fixed)
  constexpr int GR = 1 << NTB;         // registers per group
  constexpr int NBUF = CH / GR;        // groups that fit a wave's private slice of buffer 0 (1 or 2)
  // SPLITR_XPASS: the kernels whose lane bits 4, 5 change places with the T bits inside the pass (the layout is private to a launch)
  constexpr bool kX = splitr_xpass<N, NR>(DECAY, ROWS, CPLX, SNAP);
  static_assert(!kX || (CH == (1 << NW) && (NR == 4 || NR == 5)), "SPLITR_XPASS: a chunk = one named T pair, 1 or 2 lanes per G value");
  constexpr int GC = kX ? 4 : 1;       // copies of a wave's G table (copy c holds G[r ^ (c << NW)] at slot r)
  constexpr int GS = kX ? NA + 1 : NA; // slots from copy to copy: the two copies a 16-lane read group meets lie 4 banks apart
  if constexpr (kX) static_assert(SplitXAddrCheck<N, NR, NA - 1>::ok, "SPLITR_XPASS: the address form of the loads and stores");
  static_assert(GC * GS == splitr_gtab_slots<N, NR>(DECAY, ROWS, CPLX, SNAP), "the host sizes the G tables by splitr_gtab_slots");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cplx* pbuf = reinterpret_cast<cplx*>(smem);  // 2 buffers x (NT * CH) slots of 16 B
  cplx* trig = pbuf + 2 * NT * CH;             // SPLITR_TRIG
  cplx* gtab = trig + SPLITR_TRIG;             // [waves][GC][GS]: G(r) of the current stage, wave-private
  double* wtab = reinterpret_cast<double*>(gtab + (NT / 64) * GC * GS);  // [SPLIT_MAX_SUB * SPLIT_MAX_STAGES + 1] (WMODE 1)
  double* etab = wtab + (SPLIT_MAX_SUB * SPLIT_MAX_STAGES + 2);     // [4][NT]: et, eg of the even / odd layout (EMODE 1)

  const unsigned t = threadIdx.x;
  const unsigned l = t & 63u, w = t >> 6;
  const unsigned tq = splitr_lane<ND>(t);  // the thread number by the index bits it holds (SPLITR_HM)
  const int b = ROWS ? (int)blockIdx.z : (int)blockIdx.y;
  const int n_pre = R.kick_pre != 0.0 ? 1 : 0;  // the opening kick is an extra stage 0 (no D)
  // (SEG: the records of all segments, a closing one each; no kicks there)
  const int n_stages = SEG ? splitrun_records(R) : splitrun_first(R, R.nsub) + 1 + n_pre;
  // (SplitArgs.conj: conj(U) psi = conj(U conj(psi)) - the ket is conjugated at the load and at the store, the stages
  // in between are the ordinary ones: nothing in the stage loop knows about it)
  const double csgn = (ROWS && A.conj) ? -1.0 : 1.0;
  const double* __restrict__ coefs = A.ccur + (size_t)b * (UNI ? 1 : N) * 4;
  const double* __restrict__ e0 = A.e0 + (size_t)b * A.e0_stride;

  if (SPLITR_WMODE) {
    // weight of E0 in the D of stage j: a_i tau (+ the last a tau carried over from the previous sub-step)
    for (int jj = (int)t; jj < n_stages; jj += NT) {
      if constexpr (SEG) {  // record jj of the launch = stage jj - rec0 of the segment it lies in
        const SplitSegView g = splitrun_seg(R, splitrun_seg_of(R, jj));
        wtab[jj] = splitrun_weight(R, g, jj - g.rec0);
      } else {
        const int j = jj - n_pre;
        wtab[jj] = j < 0 ? 0.0 : splitrun_weight(R, j);
      }
    }
  }
  for (unsigned k = t; k < SPLITR_TRIG; k += NT) {  // (before the state is loaded: the library routine wants registers)
    double sn, cs;
    sincospi((double)k * (2.0 / SPLITR_TRIG), &sn, &cs);
    trig[k] = make_double2(cs, sn);
  }
  // E0 pieces of the two layouts (bit = 1 is the ground state: all register bits set = the lane's atoms alone, all
  // lane / wave bits set = the register atoms alone)
  double et[2], ev[2][NR], eg[2];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    et[o] = e0[L::index(o, tq, NA - 1)];
#pragma unroll
    for (int j = 0; j < NR; ++j) ev[o][j] = e0[L::index(o, tq, (NA - 1) ^ (1u << j))] - et[o];
    eg[o] = e0[L::index(o, NT - 1, l & (NA - 1))];
    if constexpr (kX) {
      // (SPLITR_XPASS) the pieces above are in ACTUAL bits; on a lane whose T bit m is flipped the tree runs over the named bit:
      // F' = 1 / F, B' = B F.  No pair term of the two T atoms here: G carries it (the lane reads G[r ^ c]).
#pragma unroll
      for (int m = 0; m < NTB; ++m) {
        if ((l >> (ND + m)) & 1u) {
          et[o] += ev[o][NW + m];
          ev[o][NW + m] = -ev[o][NW + m];
        }
      }
    }
    if (SPLITR_EMODE) {
      etab[(2 * o) * NT + t] = et[o];
      etab[(2 * o + 1) * NT + t] = eg[o];
    }
  }
  // ROWS: elementwise factor of amplitude (row a, column i) = prod_k tab_k[n_k], n = the counts of (row bit, column bit)
  // = (0,0), (0,1), (1,0), (1,1); every table is an exponential of a linear function, so the product splits into a
  // factor of the lane's column bits and one of the register's column bits (uniform: table of NA per layout use)
  double* ftl = etab + (SPLITR_EMODE ? 4 * NT : 0);  // [128] the host's tables, [NA] register factors (rewritten per use)
  unsigned a_row = 0;  // ROWS: the current row
  auto row_factor = [&](int which, unsigned col_bits, unsigned mask) -> double {
    const unsigned a = a_row;
    const int n11 = __popc(a & col_bits & mask), n10 = __popc(a & ~col_bits & mask), n01 = __popc(~a & col_bits & mask);
    const int n00 = __popc(mask) - n11 - n10 - n01;
    const double* tb = ftl + 64 * which;
    return tb[n00] * tb[16 + n01] * tb[32 + n10] * tb[48 + n11];
  };
  if (ROWS && (A.use_pre || A.use_post) && t < 128) ftl[t] = A.ftab[t];
  __syncthreads();
  typedef const __attribute__((address_space(4))) double* cptr_t;
  // exp(-i phi) = (cos, -sin): table of exp(2 pi i k / SPLITR_TRIG), series on |rr| <= pi / SPLITR_TRIG
  // (two halves, so that a stage can issue the table reads of all its phases before the first series: SPLITR_GAHEAD)
  auto expmi_arg = [&](double phi, double& rr) -> cplx {  // the table entry; rr = the reduced argument
    const double kk = rint(phi * (SPLITR_TRIG / 6.283185307179586));
    rr = fma(-kk, 6.283185307179586 / SPLITR_TRIG, phi);
    rr = fma(-kk, 2.4492935982947064e-16 / SPLITR_TRIG, rr);  // 2 pi - double(2 pi)
    return trig[((int)kk) & (SPLITR_TRIG - 1)];
  };
  auto expmi_fin = [&](double rr, cplx tb) -> cplx {
    const double r2 = rr * rr;
    double cr, sr;
    if (SPLITR_TRIG >= 512) {  // |rr| <= pi / 512: the next terms are r^6 / 720 <= 7e-17 (cosine) and r^7 / 5040 <= 6e-20 (sine)
      cr = fma(r2, fma(r2, 4.1666666666666664e-02, -0.5), 1.0);
      sr = rr * fma(r2, fma(r2, 8.333333333333333e-03, -1.6666666666666666e-01), 1.0);
    } else {
      cr = fma(r2, fma(r2, fma(r2, -1.3888888888888889e-03, 4.1666666666666664e-02), -0.5), 1.0);
      sr = rr * fma(r2, fma(r2, fma(r2, -1.984126984126984e-04, 8.333333333333333e-03), -1.6666666666666666e-01), 1.0);
    }
    return make_double2(fma(tb.x, cr, -tb.y * sr), -fma(tb.y, cr, tb.x * sr));
  };
  auto expmi = [&](double phi) -> cplx {
    double rr;
    const cplx tb = expmi_arg(phi, rr);
    return expmi_fin(rr, tb);
  };
  auto cm = [](cplx a, cplx c) -> cplx { return make_double2(fma(a.x, c.x, -a.y * c.y), fma(a.x, c.y, a.y * c.x)); };
  // private slice of buffer 0: the slots a wave's own pass stores go to (slot = l + 64 (w + NG q), q < CH)
  cplx* __restrict__ const tslice = pbuf + 64 * w;
  const unsigned la = l & ((1u << ND) - 1u), lT = l >> ND;

  // UNI: the number of the lane's own atoms whose detuning integral joins B's argument (the clear bits among its DPP lane
  // bits and wave bits; SPLITR_XPASS: lane bits 4, 5 always bring one - their own atom's or the T-position partner's)
  double n_t = 0.0;
  if constexpr (UNI) {
#pragma unroll
    for (int j = 0; j < 6; ++j) n_t += (kX && j >= ND) ? 1.0 : (((tq >> j) & 1u) ? 0.0 : 1.0);
#pragma unroll
    for (int j = 0; j < NW; ++j) n_t += ((tq >> (6 + j)) & 1u) ? 0.0 : 1.0;
  }
  double xr[NA], xi[NA];  // (outside the loop: a segment may go on from the registers of the one before it)
  // (SEG: `row` counts the segments)
  for (unsigned row = ROWS ? blockIdx.y : 0u; row < (ROWS ? (1u << N) : SEG ? (unsigned)R.nseg : 1u); row += ROWS ? gridDim.y : 1u) {
  a_row = ROWS ? row : 0u;
  cplx* __restrict__ st = A.state + ((((size_t)b << (ROWS ? N : 0)) + (ROWS ? row : 0u)) << N);
  if (ROWS) __syncthreads();  // the previous row's readers of the factor table are done
  if (ROWS && A.use_pre && t < NA) ftl[128 + t] = row_factor(0, L::index(false, 0u, t), L::index(false, 0u, NA - 1));
  if (ROWS && A.use_pre) __syncthreads();
  const SplitSegView seg = SEG ? splitrun_seg(R, (int)row) : SplitSegView{0, 0, 0};
  const int seg_flags = SEG ? R.seg_flags[row] : 0;
  // the segment before this one is done with the G tables (its compare reduces through them), and what it stored - the
  // state a later segment loads, the buffer it compares with, by the same lanes at the same addresses - is complete
  if (SEG && row > 0) __syncthreads();
  if (!SEG || !(seg_flags & SPLIT_SEG_CONT)) {
    const double fl = (ROWS && A.use_pre) ? row_factor(0, L::index(false, tq, 0u), L::index(false, NT - 1, 0u)) : 1.0;
    // (SPLITR_XPASS: address = the lane's word XOR the named T bits, plus the pass bits)
    // (SEG: the lane's word is laundered through an empty asm, as for the snapshot stores below: the addresses are invariant
    // in the segment loop, and hoisted out of it they are 64 more live registers over the stage loop - they spill, and every
    // load of a segment then waits for the one before it)
    unsigned lw0 = kX ? L::index_x(false, tq, 0u) : (SEG ? L::index(false, tq, 0u) : 0u);
    if constexpr (SEG) asm volatile("" : "+v"(lw0));
    splitr_for<0, NA>([&](auto Rc) {
      constexpr int r = decltype(Rc)::value;
      cplx v;
      if constexpr (kX) v = st[L::addr_x(false, lw0, r)];
      else if constexpr (SEG) v = st[lw0 + L::index(false, 0u, r)];
      else v = st[L::index(false, tq, r)];
      const double f = (ROWS && A.use_pre) ? fl * ftl[128 + r] : 1.0;
      xr[r] = v.x * f;
      xi[r] = v.y * (ROWS ? f * csgn : f);
    });
  }


  // rotation of register bit J (tan T) on the registers r with (r & MASK) == VAL
  auto rot_reg = [&](auto J, double T, double U, auto MASK, auto VAL) {  // T = Im g / C, U = Re g / C (CPLX only)
    if (SPLITR_KO & 16) return;
    splitr_for<0, NA>([&](auto Rc) {
      constexpr int r = decltype(Rc)::value, j = decltype(J)::value;
      if constexpr ((r & decltype(MASK)::value) == decltype(VAL)::value && !(r & (1 << j))) {
        constexpr int q = r | (1 << j);
        const double a0x = xr[r], a0y = xi[r], a1x = xr[q], a1y = xi[q];
        if constexpr (CPLX) {
          xr[r] = fma(-U, a1x, fma(-T, a1y, a0x));
          xi[r] = fma(-U, a1y, fma(T, a1x, a0y));
          xr[q] = fma(U, a0x, fma(-T, a0y, a1x));
          xi[q] = fma(U, a0y, fma(T, a0x, a1y));
        } else {
          xr[r] = fma(-T, a1y, a0x);
          xi[r] = fma(T, a1x, a0y);
          xr[q] = fma(-T, a0y, a1x);
          xi[q] = fma(T, a0x, a1y);
        }
      }
    });
  };

  double cprod = 1.0;  // product of the cosines of the previous stage's rotations (tan form): rides on B
  bool odd = false;
  // (SPLITR_PREF) the detuning integrals by position and the E0 weight of the next stage, loaded a stage ahead
  double Dn[6 + NW + NR], wEn = 0.0;
  auto load_next = [&](int sn, bool oddn) {
    cptr_t cn = (cptr_t)(unsigned long long)(coefs + (size_t)sn * stage_stride);
#pragma unroll
    for (int j = 0; j < 6; ++j) Dn[j] = cn[4 * (N - 1 - (oddn ? L::lanebit(true, j) : L::lanebit(false, j))) + 3];
#pragma unroll
    for (int j = 0; j < NW; ++j) Dn[6 + j] = cn[4 * (N - 1 - (oddn ? L::wavebit(true, j) : L::wavebit(false, j))) + 3];
#pragma unroll
    for (int j = 0; j < NR; ++j) Dn[6 + NW + j] = cn[4 * (N - 1 - (oddn ? L::regbit(true, j) : L::regbit(false, j))) + 3];
    if (SPLITR_WMODE) wEn = uniform_d(wtab[sn]);
  };
  if (SPLITR_PREF) load_next(0, false);
  unsigned warm = 0;
  unsigned warm_v = 0, warm_va = 0;  // SPLITR_KWARM 3: the value in flight and the fold of the earlier ones (per lane)
  const unsigned long long stage_bytes = (unsigned long long)stage_stride * sizeof(double);
  // One stage.  PLAIN_CLOSE: the closing stage of a run without a closing kick - D only (its rotation angles are zero):
  // the phase factors and nothing else, the layout stays (an instantiation of the same body after the loop: the loop's
  // back edge sees one register assignment)
  auto stage = [&](const int sg, auto plain_close_t) {
    constexpr bool PLAIN_CLOSE = decltype(plain_close_t)::value;
    // ---- coefficients by POSITION (uniform: scalar loads; the index bit of a position depends on the parity) ----
    cptr_t c4 = (cptr_t)(unsigned long long)(coefs + (size_t)sg * stage_stride);
    auto coef = [&](int bit_even, int bit_odd, int field) -> double {
      const int p = odd ? bit_odd : bit_even;
      return c4[4 * (N - 1 - p) + field];
    };
    double Tl[6], Dl[6], Tw[NW > 0 ? NW : 1], Dw[NW > 0 ? NW : 1], Tr[NR], Dr[NR];
    double Ul[6], Uw[NW > 0 ? NW : 1], Ur[NR];  // CPLX: Re g / C by position
    constexpr int TF = CPLX ? 2 : 1;  // the field that holds Im g / C (SplitRun.tan_form)
    double cnext = 1.0;
    // the detuning integrals first (the phase factors need them at once); the rotation coefficients follow - for
    // complex drives only AFTER the phase factors (SPLITR_LATE: the pointer is laundered through an empty asm so that
    // the loads cannot be hoisted): 14 x (C, Re g / C, Im g / C) on top of the 14 integrals do not fit the scalar
    // registers (79 spilled, and a spilled scalar load is a serialised one: +1 us per stage, round-4 variants table)
    // UNI: the sequence's record of this stage, one scalar load of 32 bytes
    typedef double splitr_rec_t __attribute__((ext_vector_type(4)));
    splitr_rec_t rec = {1.0, 0.0, 0.0, 0.0};
    double Du = 0.0;  // its Delta
    if constexpr (UNI) {
      rec = *reinterpret_cast<const __attribute__((address_space(4))) splitr_rec_t*>(c4);
      Du = rec[3];
#pragma unroll
      for (int j = 0; j < 6; ++j) Dl[j] = Du;
#pragma unroll
      for (int j = 0; j < NW; ++j) Dw[j] = Du;
#pragma unroll
      for (int j = 0; j < NR; ++j) Dr[j] = Du;
    } else {
#pragma unroll
    for (int j = 0; j < 6; ++j) Dl[j] = SPLITR_PREF ? Dn[j] : coef(L::lanebit(false, j), L::lanebit(true, j), 3);
#pragma unroll
    for (int j = 0; j < NW; ++j) Dw[j] = SPLITR_PREF ? Dn[6 + j] : coef(L::wavebit(false, j), L::wavebit(true, j), 3);
#pragma unroll
    for (int j = 0; j < NR; ++j) Dr[j] = SPLITR_PREF ? Dn[6 + NW + j] : coef(L::regbit(false, j), L::regbit(true, j), 3);
    }
    auto load_rot = [&](cptr_t cl) {
      if constexpr (UNI) {  // one T for every position; the product of the N cosines is the record's first field
        const double Tu = rec[TF];
#pragma unroll
        for (int j = 0; j < 6; ++j) { Tl[j] = Tu; Ul[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < NW; ++j) { Tw[j] = Tu; Uw[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < NR; ++j) { Tr[j] = Tu; Ur[j] = 0.0; }
        cnext = rec[0];
        return;
      }
      auto coefl = [&](int bit_even, int bit_odd, int field) -> double {
        const int p = odd ? bit_odd : bit_even;
        return cl[4 * (N - 1 - p) + field];
      };
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        Tl[j] = coefl(L::lanebit(false, j), L::lanebit(true, j), TF);
        Ul[j] = CPLX ? coefl(L::lanebit(false, j), L::lanebit(true, j), 1) : 0.0;
        cnext *= coefl(L::lanebit(false, j), L::lanebit(true, j), 0);
      }
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        Tw[j] = coefl(L::wavebit(false, j), L::wavebit(true, j), TF);
        Uw[j] = CPLX ? coefl(L::wavebit(false, j), L::wavebit(true, j), 1) : 0.0;
        cnext *= coefl(L::wavebit(false, j), L::wavebit(true, j), 0);
      }
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        Tr[j] = coefl(L::regbit(false, j), L::regbit(true, j), TF);
        Ur[j] = CPLX ? coefl(L::regbit(false, j), L::regbit(true, j), 1) : 0.0;
        cnext *= coefl(L::regbit(false, j), L::regbit(true, j), 0);
      }
    };
    constexpr bool kLate = (SPLITR_LATE && CPLX) || (SPLITR_LATE_REAL && !CPLX);
    if (!kLate && !PLAIN_CLOSE) load_rot(c4);
    // weight of E0 in this stage's D: a_i tau (+ the last a tau carried over from the previous sub-step)
    double wE;
    if (SPLITR_WMODE && SPLITR_PREF) {
      wE = wEn;
    } else if (SPLITR_WMODE) {
      wE = uniform_d(wtab[sg]);
    } else {
      const int sj = sg - n_pre;
      wE = sj < 0 ? 0.0 : splitrun_weight(R, sj);
    }
    double et_s, eg_s;
    if (SPLITR_EMODE) {
      et_s = etab[(odd ? 2 : 0) * NT + t];
      eg_s = etab[(odd ? 3 : 1) * NT + t];
    } else {
      et_s = odd ? et[1] : et[0];
      eg_s = odd ? eg[1] : eg[0];
    }

    // ---- the lane's phase factors ----
    cplx Bf, F[NR], Gl;
    // SPLITR_GAHEAD: the shapes and builds that read their phase tables ahead; Gq = the G values of the group whose
    // phase factors come next (register r = g | (rho << NW) in Gq[rho])
    // (not ROWS, not CPLX: the 16 registers do not fit there - the row kernel spills 22 vector registers instead of 12)
    constexpr bool kGAhead = SPLITR_GAHEAD != 0 && !SPLITR_GMODE && SPLITR_TMODE == 1 && NTB == 2 && !CPLX && !ROWS && !PLAIN_CLOSE && !(SPLITR_KO & 8);
    cplx Gq[GR];
    auto g_fetch = [&](auto Gc) {
      constexpr int g = decltype(Gc)::value;
      // (SPLITR_XPASS: the copy of the lane's (l4, l5) - G[r ^ c] at slot r)
      const cplx* __restrict__ gq = kX ? gtab + w * (GC * GS) + ((l >> ND) & 3u) * GS : gtab + w * NA;
      splitr_for<0, GR>([&](auto Ic) {
        constexpr int rho = GR - 1 - decltype(Ic)::value;  // (the order phase_group uses them in)
        Gq[rho] = gq[g | (rho << NW)];
      });
    };
    if (!(SPLITR_KO & 8)) {
      double dthr = UNI ? Du * n_t : 0.0;
#pragma unroll
      for (int j = 0; j < (UNI ? 0 : 6); ++j) {
        // (SPLITR_XPASS: a lane with bit ND + m set holds the atom of T bit m flipped - that atom's integral joins B's argument
        // exactly where the lane's own does not: one select, one addition)
        if (kX && j >= ND) dthr += ((tq >> j) & 1u) ? Dr[NW + (j >= ND ? j - ND : 0)] : Dl[j];
        else dthr += ((tq >> j) & 1u) ? 0.0 : Dl[j];
      }
#pragma unroll
      for (int j = 0; j < (UNI ? 0 : NW); ++j) dthr += ((tq >> (6 + j)) & 1u) ? 0.0 : Dw[j];
      double sc = cprod;
      if (DECAY)  // H_eff: the real factor exp(wE (dec_a + dec_b popc(index))): lane part here, register part in F
        sc *= exp(wE * (A.dec_a + A.dec_b * (double)(__popc(tq) + NR)));
      const double dF = DECAY ? exp(-wE * A.dec_b) : 1.0;  // an excited register atom: one set bit fewer
      // the detuning integral of register bit j in F_j's argument (SPLITR_XPASS: minus it where the lane holds T bit j flipped)
      auto drs = [&](int j) -> double {
        if (kX && j >= NW) return __hiloint2double(__double2hiint(Dr[j]) ^ (int)(((l >> (ND + (j >= NW ? j - NW : 0))) & 1u) << 31), __double2loint(Dr[j]));
        return Dr[j];
      };
      // the G table of the wave (SPLITR_XPASS: four permuted copies, lane l & (NA - 1) of each replica writes its share of them)
      auto g_store = [&]() {
        if constexpr (kX) {
          constexpr int RB = 6 - NR;  // 2^RB lanes hold the same G value
          splitr_for<0, (4 >> RB)>([&](auto Ic) {
            const unsigned cpy = RB == 2 ? (l >> 4) : ((unsigned)decltype(Ic)::value | ((l >> 5) << 1));
            gtab[w * (GC * GS) + cpy * GS + ((l & (NA - 1)) ^ (cpy << NW))] = Gl;
          });
        }
      };
      if constexpr (kGAhead) {
        // the same seven expmi on the same arguments; only the order of issue differs: table reads, G's series, the G
        // table and the first group's reads of it, then the other six series (which cover those reads)
        double rB, rF[NR], rG;
        const cplx tG = expmi_arg(wE * eg_s, rG);
        const cplx tB = expmi_arg(fma(wE, et_s, -dthr), rB);
        cplx tF[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) tF[j] = expmi_arg(fma(wE, odd ? ev[1][j] : ev[0][j], -drs(j)), rF[j]);
        __builtin_amdgcn_sched_barrier(0);
        Gl = expmi_fin(rG, tG);
        if constexpr (kX) g_store();
        else gtab[w * NA + (l & (NA - 1))] = Gl;
        __builtin_amdgcn_wave_barrier();
        g_fetch(splitr_c<NG - 1>{});
        __builtin_amdgcn_sched_barrier(0);
        Bf = expmi_fin(rB, tB);
        Bf = make_double2(Bf.x * sc, Bf.y * sc);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          F[j] = expmi_fin(rF[j], tF[j]);
          if (DECAY) F[j] = make_double2(F[j].x * dF, F[j].y * dF);
        }
      } else {
      Bf = expmi(fma(wE, et_s, -dthr));
      Bf = make_double2(Bf.x * sc, Bf.y * sc);
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        F[j] = expmi(fma(wE, odd ? ev[1][j] : ev[0][j], -drs(j)));
        if (DECAY) F[j] = make_double2(F[j].x * dF, F[j].y * dF);
      }
      Gl = expmi(wE * eg_s);
      if (!SPLITR_GMODE) {
        if constexpr (kX) g_store();
        else gtab[w * NA + (l & (NA - 1))] = Gl;
        __builtin_amdgcn_wave_barrier();
      }
      }
    }
    if (kLate && !PLAIN_CLOSE) {
      unsigned long long cl = (unsigned long long)(coefs + (size_t)sg * stage_stride);
      asm volatile("" : "+s"(cl));
      load_rot((cptr_t)cl);
    }
    cprod = cnext;
    const cplx* __restrict__ gw = kX ? gtab + w * (GC * GS) + ((l >> ND) & 3u) * GS : gtab + w * NA;
    auto gval = [&](auto Rc) -> cplx {  // G(r): uniform
      constexpr int r = decltype(Rc)::value;
      if (SPLITR_GMODE) {
        const int a = __builtin_amdgcn_readlane(__double2loint(Gl.x), r), b2 = __builtin_amdgcn_readlane(__double2hiint(Gl.x), r);
        const int c = __builtin_amdgcn_readlane(__double2loint(Gl.y), r), d = __builtin_amdgcn_readlane(__double2hiint(Gl.y), r);
        return make_double2(__hiloint2double(b2, a), __hiloint2double(d, c));
      }
      return gw[r];
    };

    // ---- per group (pass bits fixed): D, the T-bit rotations, the intra-wave transposition, the rotations of
    //      the lane bits that arrived.  Product tree: groups from NG-1 down (parent = lowest clear bit set), the T
    //      bits innermost. ----
    cplx Pg[NG];
    auto phase_group = [&](auto Gc) {
      constexpr int g = decltype(Gc)::value;
      if (SPLITR_KO & 8) return;
      cplx Gg[GR];  // (SPLITR_GAHEAD) this group's G values, read a group ago; Gq takes the next group's
      if constexpr (kGAhead) {
        splitr_for<0, GR>([&](auto Ic) { Gg[decltype(Ic)::value] = Gq[decltype(Ic)::value]; });
        if constexpr (SPLITR_GAHEAD == 1 && g > 0) {
          g_fetch(splitr_c<(g > 0 ? g - 1 : 0)>{});
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (g == NG - 1) Pg[g] = Bf;
      else Pg[g] = cm(Pg[g | (1 << splitr_low_clear(g))], F[splitr_low_clear(g)]);
      cplx Pt[GR];
      splitr_for<0, GR>([&](auto Ic) {
        constexpr int rho = GR - 1 - decltype(Ic)::value;
        if constexpr (rho == GR - 1) Pt[rho] = Pg[g];
        else Pt[rho] = cm(Pt[rho | (1 << splitr_low_clear(rho))], F[NW + splitr_low_clear(rho)]);
        constexpr int r = g | (rho << NW);
        cplx gv;
        if constexpr (kGAhead) gv = Gg[rho];
        else gv = gval(splitr_c<r>{});
        const cplx q = cm(Pt[rho], gv);
        const double ax = xr[r], ay = xi[r];
        xr[r] = fma(ax, q.x, -ay * q.y);
        xi[r] = fma(ax, q.y, ay * q.x);
      });
      if constexpr (kGAhead && SPLITR_GAHEAD == 2 && g > 0) {
        g_fetch(splitr_c<(g > 0 ? g - 1 : 0)>{});
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    auto swap_d = [](double& a, double& c, auto is32) {
      unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
      unsigned clo = (unsigned)__double2loint(c), chi = (unsigned)__double2hiint(c);
      if constexpr (decltype(is32)::value) {
        auto p = __builtin_amdgcn_permlane32_swap(alo, clo, false, false);
        auto q = __builtin_amdgcn_permlane32_swap(ahi, chi, false, false);
        alo = p[0]; clo = p[1]; ahi = q[0]; chi = q[1];
      } else {
        auto p = __builtin_amdgcn_permlane16_swap(alo, clo, false, false);
        auto q = __builtin_amdgcn_permlane16_swap(ahi, chi, false, false);
        alo = p[0]; clo = p[1]; ahi = q[0]; chi = q[1];
      }
      a = __hiloint2double((int)ahi, (int)alo);
      c = __hiloint2double((int)chi, (int)clo);
    };
    // SPLITR_YCHAIN: the shapes and builds that take the y chain, and whether its last hop rides on the pass
    constexpr bool kYChain = SPLITR_YCHAIN != 0 && !CPLX && SPLITR_HM == 1 && SPLITR_TMODE == 1 && !SPLITR_B2 && !(SPLITR_KO & 2) && ND >= 2;
    constexpr bool kYStore = kYChain && SPLITR_YCHAIN == 2 && NW > 0 && !(SPLITR_KO & 4);
    auto t_swap = [&](auto Gc) {  // SPLITR_TMODE 1 (NTB == 2): T bit 0 <-> lane bit 4, T bit 1 <-> lane bit 5
      constexpr int g = decltype(Gc)::value;
      if (SPLITR_KO & 1) return;
      constexpr int r0 = g, r1 = g | (1 << NW), r2 = g | (2 << NW), r3 = g | (3 << NW);
      swap_d(xr[r0], xr[r1], std::false_type{}); swap_d(xi[r0], xi[r1], std::false_type{});
      swap_d(xr[r2], xr[r3], std::false_type{}); swap_d(xi[r2], xi[r3], std::false_type{});
      swap_d(xr[r0], xr[r2], std::true_type{}); swap_d(xi[r0], xi[r2], std::true_type{});
      swap_d(xr[r1], xr[r3], std::true_type{}); swap_d(xi[r1], xi[r3], std::true_type{});
    };
    auto t_write = [&](auto Gc) {
      constexpr int g = decltype(Gc)::value;
      if (SPLITR_KO & 1) return;
      splitr_for<0, GR>([&](auto Ic) {
        constexpr int rho = decltype(Ic)::value;
        constexpr int run = rho + (NBUF == 2 ? (g & 1) * GR : 0);
        tslice[64 * NG * run + la + ((lT ^ (unsigned)L::swz(rho)) << ND)] = make_double2(xr[g | (rho << NW)], xi[g | (rho << NW)]);
      });
    };
    auto t_read = [&](auto Gc) {
      constexpr int g = decltype(Gc)::value;
      if (SPLITR_KO & 1) return;
      __builtin_amdgcn_wave_barrier();
      const unsigned run = lT + (NBUF == 2 ? (g & 1) * GR : 0);
      splitr_for<0, GR>([&](auto Ic) {
        constexpr int rho = decltype(Ic)::value;
        const cplx v = tslice[64 * NG * run + la + (((unsigned)rho ^ (unsigned)L::swz((int)lT)) << ND)];
        xr[g | (rho << NW)] = v.x;
        xi[g | (rho << NW)] = v.y;
      });
    };
    auto rot_t_old = [&](auto Gc) {  // the T bits this layout holds
      splitr_for<0, NTB>([&](auto Mc) {
        constexpr int m = decltype(Mc)::value;
        rot_reg(splitr_c<NW + m>{}, Tr[NW + m], Ur[NW + m], splitr_c<PW>{}, Gc);
      });
    };
    auto rot_t_new = [&](auto Gc) {  // the upper lane bits, now in the T registers
      splitr_for<0, NTB>([&](auto Mc) {
        constexpr int m = decltype(Mc)::value;
        rot_reg(splitr_c<NW + m>{}, Tl[ND + m], Ul[ND + m], splitr_c<PW>{}, Gc);
      });
    };
    // CPLX: Re g / C of the DPP bits with the sign of the lane's own bit (+ on bit 1, - on bit 0)
    double Us[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (CPLX) {
#pragma unroll
      for (int j = 0; j < 6; ++j) Us[j] = ((tq >> j) & 1u) ? Ul[j] : -Ul[j];
    }
    // SPLITR_TMODE 3: partner of lane bit 4 (ds_swizzle, xor 16 inside 32 lanes) / 5 (ds_bpermute) of a double - the LDS
    // crossbar, no LDS memory, no vector-pipe cycles beyond the issue
    auto xpartner = [&](double v, auto Jc) -> double {
      int lo = __double2loint(v), hi = __double2hiint(v);
      if constexpr (decltype(Jc)::value == 4) {
        lo = __builtin_amdgcn_ds_swizzle(lo, 0x401F);
        hi = __builtin_amdgcn_ds_swizzle(hi, 0x401F);
      } else {
        const int addr = (int)((l ^ 32u) << 2);
        lo = __builtin_amdgcn_ds_bpermute(addr, lo);
        hi = __builtin_amdgcn_ds_bpermute(addr, hi);
      }
      return __hiloint2double(hi, lo);
    };
    auto rot_lane_x = [&](auto Rc) {
      constexpr int r = decltype(Rc)::value;
      if (SPLITR_KO & 1) return;
      splitr_for<4, 6>([&](auto Jc) {
        constexpr int j = decltype(Jc)::value;
        const double T = Tl[j], px = xpartner(xr[r], Jc), py = xpartner(xi[r], Jc);
        if constexpr (CPLX) {
          xr[r] = fma(Us[j], px, fma(-T, py, xr[r]));
          xi[r] = fma(Us[j], py, fma(T, px, xi[r]));
        } else {
          xr[r] = fma(-T, py, xr[r]);
          xi[r] = fma(T, px, xi[r]);
        }
      });
    };
    // rotations of the DPP lane bits in MASK on register r (any time between this stage's D and the next one's: they
    // commute with every other rotation and exchange of the stage)
    auto rot_lane = [&](auto Rc, auto MASK) {
      constexpr int r = decltype(Rc)::value, mask = decltype(MASK)::value;
      if (SPLITR_KO & 2) return;
      if constexpr (ND > 0 && (mask & 1)) {
        const double T = Tl[0], px = splitr_partner<0>(xr[r]), py = splitr_partner<0>(xi[r]);
        if constexpr (CPLX) {
          xr[r] = fma(Us[0], px, fma(-T, py, xr[r]));
          xi[r] = fma(Us[0], py, fma(T, px, xi[r]));
        } else {
          xr[r] = fma(-T, py, xr[r]);
          xi[r] = fma(T, px, xi[r]);
        }
      }
      if constexpr (ND > 1 && (mask & 2)) {
        const double T = Tl[1], px = splitr_partner<1>(xr[r]), py = splitr_partner<1>(xi[r]);
        if constexpr (CPLX) {
          xr[r] = fma(Us[1], px, fma(-T, py, xr[r]));
          xi[r] = fma(Us[1], py, fma(T, px, xi[r]));
        } else {
          xr[r] = fma(-T, py, xr[r]);
          xi[r] = fma(T, px, xi[r]);
        }
      }
      if constexpr (ND > 3 && (mask & 8)) {
        const double T = Tl[3], px = splitr_partner<3>(xr[r]), py = splitr_partner<3>(xi[r]);
        if constexpr (CPLX) {
          xr[r] = fma(Us[3], px, fma(-T, py, xr[r]));
          xi[r] = fma(Us[3], py, fma(T, px, xi[r]));
        } else {
          xr[r] = fma(-T, py, xr[r]);
          xi[r] = fma(T, px, xi[r]);
        }
      }
      if constexpr (ND > 2 && (mask & 4)) {
        const double T = Tl[2], px = splitr_partner<2>(xr[r]), py = splitr_partner<2>(xi[r]);
        if constexpr (CPLX) {
          xr[r] = fma(Us[2], px, fma(-T, py, xr[r]));
          xi[r] = fma(Us[2], py, fma(T, px, xi[r]));
        } else {
          xr[r] = fma(-T, py, xr[r]);
          xi[r] = fma(T, px, xi[r]);
        }
      }
    };
    // SPLITR_TMODE 2: the transposition through LDS with the vector work arranged around it - D on every group first
    // (its G-table reads would otherwise sit in the LDS queue between a group's stores and loads and every wait for a
    // G value would wait for the transposition too), then per group the old T bits, the DPP bits TMASK (filler: the
    // LDS takes ~540 cycles per group for the 8 waves), the stores, the loads; the other DPP bits stay with the pass
    if constexpr (PLAIN_CLOSE) {
      splitr_for<0, NG>([&](auto Ic) { phase_group(splitr_c<(NG - 1 - decltype(Ic)::value)>{}); });
    } else {
    // SPLITR_KWARM 2 / 3: the touches of the next stage's record are issued behind the phase factors of the LAST group - the
    // last LDS read of the group loop is behind, the next wait on that counter is the one in front of the pass's first
    // barrier; that group's rotations, pre(C0) and write_pre(C0, C1) lie in between - and are folded into `warm` only there.
    // (Shapes whose groups go through the LDS transposition issue them behind the group loop.)  The address is the scalar
    // c4 plus the stride; the touched values pass through an empty asm so that their use cannot be pulled forward.
    constexpr int NWV = UNI ? 1 : 8;  // touches of the next record (UNI: its 32 bytes lie in one line)
    unsigned wv[NWV];
    constexpr bool kWarmLate = (SPLITR_KWARM == 2 || SPLITR_KWARM == 3) && NW > 0 && !(SPLITR_KO & 4);
    // (complex drives issue them behind the loop too: <14, 5, DECAY, CPLX> spills a vector register otherwise)
    constexpr bool kWarmInLoop = kWarmLate && SPLITR_TMODE == 1 && NTB == 2 && !CPLX;
    auto warm_issue = [&]() {
      const unsigned long long nv = (unsigned long long)c4 + (sg + 1 < n_stages ? stage_bytes : 0ull);
      // (uniform by construction; the first-lane reads are free where the compiler already holds it in scalar registers
      // and keep the asm's scalar constraint legal where it does not)
      unsigned long long na = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(nv >> 32)) << 32) |
                              (unsigned)__builtin_amdgcn_readfirstlane((int)nv);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+s"(na));
      if constexpr (SPLITR_KWARM == 2) {
        typedef const __attribute__((address_space(4))) unsigned* uptr_t;
        uptr_t nx = (uptr_t)na;
#pragma unroll
        // (one word per 64-byte line of the sequence's 8 N words, the last line by its last word - and never beyond it: at 12
        // atoms the record is 6 lines, line 6 is the next sequence's, and behind the last sequence of the last record the end of
        // the table - on a page boundary when the records are a multiple of 32, which a launch with segments can be)
        for (int k = 0; k < NWV; ++k) wv[k] = UNI ? nx[0] : nx[(k < 7 && 16 * k < 8 * N) ? 16 * k : 8 * N - 1];
      } else {
        // lane k on line k (the last line by its last word); the value of the PREVIOUS stage's touch is folded first
        warm_va ^= warm_v;
        const unsigned k = l & 7u;
        // (the global address space by name: a generic pointer would make it a flat load, which counts on the LDS /
        // scalar counter as well)
        typedef const __attribute__((address_space(1))) unsigned* gptr_t;
        warm_v = ((gptr_t)na)[UNI ? 0u : (k < 7u && 16u * k < 8u * N) ? 16u * k : 8u * N - 1u];
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    constexpr int TMASK = SPLITR_TMODE == 2 ? 3 : 0;           // DPP lane bits rotated inside the transposition loop
    constexpr int PMASK = ((1 << ND) - 1) & ~TMASK;            // ... and with the pass chunks
    if constexpr (SPLITR_TMODE == 2) {
      splitr_for<0, NG>([&](auto Ic) { phase_group(splitr_c<(NG - 1 - decltype(Ic)::value)>{}); });
      splitr_for<0, NG>([&](auto Ic) {
        constexpr int g = NG - 1 - decltype(Ic)::value;
        rot_t_old(splitr_c<g>{});
        splitr_for<0, GR>([&](auto Qc) { rot_lane(splitr_c<(g | (decltype(Qc)::value << NW))>{}, splitr_c<TMASK>{}); });
        t_write(splitr_c<g>{});
        t_read(splitr_c<g>{});
        if constexpr (g + 1 < NG) rot_t_new(splitr_c<g + 1>{});
      });
      rot_t_new(splitr_c<0>{});
    } else {
      splitr_for<0, NG>([&](auto Ic) {
        constexpr int g = NG - 1 - decltype(Ic)::value;
        phase_group(splitr_c<g>{});
        if constexpr (g == 0 && kWarmInLoop) warm_issue();
        rot_t_old(splitr_c<g>{});
        if constexpr (SPLITR_TMODE == 3) {
          // nothing to exchange
        } else if constexpr (kX) {
          // (SPLITR_XPASS) lane bits 4, 5 arrive with the pass; their rotations follow its reads (rot_x below)
        } else if constexpr (SPLITR_TMODE == 1 && NTB == 2) {
          t_swap(splitr_c<g>{});
          rot_t_new(splitr_c<g>{});
        } else {
          t_write(splitr_c<g>{});
          t_read(splitr_c<g>{});
          if constexpr (g + 1 < NG) rot_t_new(splitr_c<g + 1>{});
        }
      });
      if constexpr (!(SPLITR_TMODE == 1 && NTB == 2) && SPLITR_TMODE != 3) rot_t_new(splitr_c<0>{});
    }

    // ---- per chunk (top two T bits fixed): the pass bits and the DPP lane bits, then the pass ----
    constexpr int CM = 3 << (NR - 2);  // the chunk's bits of the register index
    auto pre_regs = [&](auto Cc) {  // the pass bits
      constexpr int c = decltype(Cc)::value;
      splitr_for<0, NW>([&](auto Jc) { rot_reg(Jc, Tr[decltype(Jc)::value], Ur[decltype(Jc)::value], splitr_c<CM>{}, splitr_c<(c << (NR - 2))>{}); });
    };
    // SPLITR_YCHAIN: step I of the y chain on the registers of a chunk - the hop to the direction of the plan's I-th bit (one
    // or two patterns, generated from the table and from nothing else), then that bit's rotation; step ND = the way home
    // (no pattern when the pass stores y shifted).  Lane L keeps x(L) and holds y(L ^ shift).  Hop by hop over the whole
    // chunk: CH independent registers between a move and the FMA that waits for it.
    auto chain_step = [&](auto Cc, auto Ic) {
      constexpr int c = decltype(Cc)::value, i = decltype(Ic)::value;
      typedef SplitYPlan<ND, (kYStore ? 1 : 0)> PL;
      constexpr SplitYHop h = PL::hops[i];
      if constexpr (h.n > 0) splitr_for<0, CH>([&](auto Kc) { constexpr int r = decltype(Kc)::value | (c << (NR - 2)); xi[r] = splitr_dpp<h.ctrl[0]>(xi[r]); });
      if constexpr (h.n > 1) splitr_for<0, CH>([&](auto Kc) { constexpr int r = decltype(Kc)::value | (c << (NR - 2)); xi[r] = splitr_dpp<h.ctrl[1]>(xi[r]); });
      if constexpr (i < ND) {
        const double T = Tl[PL::order[i < ND ? i : 0]];
        splitr_for<0, CH>([&](auto Kc) {
          constexpr int r = decltype(Kc)::value | (c << (NR - 2));
          const double x0 = xr[r];
          xr[r] = fma(-T, xi[r], x0);  // x'(L) = x(L) - T y(L ^ m)
          xi[r] = fma(T, x0, xi[r]);   // y'(L ^ m) = y(L ^ m) + T x(L)
        });
      }
    };
    auto pre = [&](auto Cc) {
      constexpr int c = decltype(Cc)::value;
      pre_regs(Cc);
      if constexpr (kYChain) {
        splitr_for<0, ND + 1>([&](auto Ic) { chain_step(Cc, Ic); });
      } else {
        splitr_for<0, CH>([&](auto Kc) {
          rot_lane(splitr_c<(decltype(Kc)::value | (c << (NR - 2)))>{}, splitr_c<PMASK>{});
          if constexpr (SPLITR_TMODE == 3) rot_lane_x(splitr_c<(decltype(Kc)::value | (c << (NR - 2)))>{});
        });
      }
    };
    auto post = [&](auto Cc) {  // the wave bits, now register bits 0 .. NW-1
      constexpr int c = decltype(Cc)::value;
      splitr_for<0, NW>([&](auto Jc) { rot_reg(Jc, Tw[decltype(Jc)::value], Uw[decltype(Jc)::value], splitr_c<CM>{}, splitr_c<(c << (NR - 2))>{}); });
    };
    // slot = l + 64 (A + NG (B + NG s)):  writer A = wave, B = its pass bits;  reader A = its pass bits, B = its wave;
    // s = the chunk's T bits below the top two
    auto pass_write_part = [&](auto Cc, auto K0c, auto K1c) {
      constexpr int c = decltype(Cc)::value, K0 = decltype(K0c)::value, K1 = decltype(K1c)::value;
      if constexpr (kYStore) {
        // (SPLITR_YCHAIN 2) the lane holds y of lane t ^ shift: x to its own slot, y to that lane's - the last hop of the chain
        constexpr unsigned S = SplitYPlan<ND, 1>::final_shift;
        double* __restrict__ px = reinterpret_cast<double*>(pbuf + (c & 1) * (NT * CH) + t);
        double* __restrict__ py = reinterpret_cast<double*>(pbuf + (c & 1) * (NT * CH) + (t ^ S)) + 1;
        splitr_for<K0, K1>([&](auto Kc) {
          constexpr int k = decltype(Kc)::value, kp = k & PW, ks = k >> NW;
          px[2 * 64 * NG * (kp + NG * ks)] = xr[k | (c << (NR - 2))];
          py[2 * 64 * NG * (kp + NG * ks)] = xi[k | (c << (NR - 2))];
        });
        return;
      }
      cplx* __restrict__ pb = pbuf + (c & 1) * (NT * CH) + t;
      splitr_for<K0, K1>([&](auto Kc) {
        constexpr int k = decltype(Kc)::value, kp = k & PW, ks = k >> NW;
        pb[64 * NG * (kp + NG * ks)] = make_double2(xr[k | (c << (NR - 2))], xi[k | (c << (NR - 2))]);
      });
    };
    auto pass_write = [&](auto Cc) { pass_write_part(Cc, splitr_c<0>{}, splitr_c<CH>{}); };
    // pass_write(Cw), then pre(Cp).  With the y chain the stores are SPREAD over the steps of Cp's chain (scheduling fences keep
    // them there): issued back to back behind a barrier, the stores of the 8 waves fill the LDS queue and every wave waits at
    // its last store before it can issue the rotations that would cover them (profiles/ychain.md: SQ_WAIT_INST_LDS)
    auto write_pre = [&](auto Cw, auto Cp) {
      if constexpr (kYChain) {
        pre_regs(Cp);
        splitr_for<0, ND + 1>([&](auto Ic) {
          constexpr int i = decltype(Ic)::value;
          pass_write_part(Cw, splitr_c<(i * CH / (ND + 1))>{}, splitr_c<((i + 1) * CH / (ND + 1))>{});
          __builtin_amdgcn_sched_barrier(0);
          chain_step(Cp, Ic);
          __builtin_amdgcn_sched_barrier(0);
        });
      } else {
        pass_write(Cw);
        pre(Cp);
      }
    };
    auto pass_read = [&](auto Cc) {
      constexpr int c = decltype(Cc)::value;
      // (SPLITR_XPASS: the chunk named (s0, s1) comes from the registers of the same name of lane l ^ (s0 << 4 | s1 << 5))
      const cplx* __restrict__ pb = pbuf + (c & 1) * (NT * CH) + (kX ? l ^ (unsigned)(c << ND) : l) + 64 * NG * w;
      splitr_for<0, CH>([&](auto Kc) {
        constexpr int k = decltype(Kc)::value, kp = k & PW, ks = k >> NW;
        const cplx v = pb[64 * (kp + NG * NG * ks)];
        xr[k | (c << (NR - 2))] = v.x;
        xi[k | (c << (NR - 2))] = v.y;
      });
    };
    typedef splitr_c<0> C0; typedef splitr_c<1> C1; typedef splitr_c<2> C2; typedef splitr_c<3> C3;
    // SPLITR_XPASS: the atom that arrived on T bit M from lane bit ND + M, on the pairs of chunks whose other T bit is V
    auto rot_x = [&](auto Mc, auto Vc) {
      constexpr int m = decltype(Mc)::value, v = decltype(Vc)::value;
      rot_reg(splitr_c<NW + m>{}, Tl[ND + m], Ul[ND + m], splitr_c<(1 << (NW + 1 - m))>{}, splitr_c<(v << (NW + 1 - m))>{});
    };
    if constexpr (NW == 0 || (SPLITR_KO & 4)) {
      pre(C0{}); pre(C1{}); pre(C2{}); pre(C3{});
      post(C0{}); post(C1{}); post(C2{}); post(C3{});
    } else {
      // (no barrier here: until the first one below a wave only touches its own slice of buffer 0 - the
      // transposition above and pass_write(0) - and buffer 0's last cross-wave reads, pass_read(2) of the previous
      // stage, sit before that stage's last barrier)
      if constexpr (kWarmLate && !kWarmInLoop) warm_issue();
      pre(C0{});
      write_pre(C0{}, C1{});
      if constexpr (SPLITR_KWARM == 2) {
#pragma unroll
        for (int k = 0; k < NWV; ++k) {
          asm volatile("" : "+s"(wv[k]));
          warm ^= wv[k];
        }
      }
      __syncthreads();
      pass_read(C0{});
      if (SPLITR_KWARM == 1) {
        typedef const __attribute__((address_space(4))) unsigned* uptr_t;
        uptr_t nx = (uptr_t)(unsigned long long)(coefs + (size_t)(sg + 1 < n_stages ? sg + 1 : sg) * stage_stride);
#pragma unroll
        for (int k = 0; k < NWV; ++k) warm ^= UNI ? nx[0] : nx[(k < 7 && 16 * k < 8 * N) ? 16 * k : 8 * N - 1];
      }
      write_pre(C1{}, C2{});
      __syncthreads();
      pass_read(C1{});
      write_pre(C2{}, C3{});
      __syncthreads();
      pass_read(C2{});
      pass_write(C3{});
      post(C0{});
      post(C1{});
      // (SPLITR_XPASS) the arriving atoms.  A rotation restricted to some chunks commutes with another one only if both are
      // whole on the registers they share: T bit 0 on the pair (C0, C1) once both have their wave bits; T bit 1 mixes C0 with
      // C2 and C1 with C3, so it waits until T bit 0 is done on all four - after pass_read(C3).  That tail overlaps the next
      // stage's table-and-series work, which does not depend on it.
      if constexpr (kX) {
        post(C2{});
        rot_x(C0{}, C0{});
      }
      __syncthreads();
      pass_read(C3{});
      if (SPLITR_PREF) load_next(sg + 1 < n_stages ? sg + 1 : sg, !odd);
      if constexpr (!kX) post(C2{});
      post(C3{});
      if constexpr (kX) {
        rot_x(C0{}, C1{});
        rot_x(C1{}, C0{});
        rot_x(C1{}, C1{});
      }
    }
    odd = !odd;
    }
    if (SPLITR_KWARM) asm volatile("" ::"s"(warm));
    if constexpr (SPLITR_KWARM == 3) asm volatile("" ::"v"(warm_va));
  };
  const int n_full = R.kick_post == 0.0 ? n_stages - 1 : n_stages;
  if constexpr (SEG) {
    // the records of this segment: its stages (an even number: it ends in the even layout, like every segment before
    // it), then its own closing D
    const int sg_close = seg.rec0 + splitrun_seg_stages(R, seg);
    for (int sg = seg.rec0; sg < sg_close; ++sg) stage(sg, std::false_type{});
    stage(sg_close, std::true_type{});
  } else if constexpr (SNAP) {
    int snap_at = splitrun_first(R, 1) + n_pre - 1, snap_sub = 0;  // the stage that ends sub-step snap_sub
    for (int sg = 0; sg < n_full; ++sg) {
      stage(sg, std::false_type{});
      if (sg == snap_at) {
        const int slot = R.snap[snap_sub];
        const long long moff = (slot >= 0 && A.snap_map_slots > 0) ? A.snap_map[(size_t)b * A.snap_map_slots + slot] : 0;
        if (slot >= 0 && moff >= 0) {
          // address = uniform base + the lane's word + a constant per register.  The lane's word is laundered through an
          // empty asm: loop-invariant otherwise, and the 32 hoisted 64-bit addresses cost 20 spilled vector registers
          // in every stage of the loop (measured: 10.6 instead of 9.4 us per stage)
          // (SPLITR_XPASS: the lane's word XOR the named T bits - four bases - plus the other register bits)
          unsigned lw = kX ? (odd ? L::index_x(true, tq, 0u) : L::index_x(false, tq, 0u)) : (odd ? L::index(true, tq, 0u) : L::index(false, tq, 0u));
          asm volatile("" : "+v"(lw));
          cplx* __restrict__ sd = A.snap_map_slots > 0 ? A.snaps + ((size_t)moff << N)
                                             : A.snaps + (size_t)slot * A.snap_stride + ((size_t)b << N);
          if (odd) {
            splitr_for<0, NA>([&](auto Rc) {
              constexpr int r = decltype(Rc)::value;
              const unsigned ix = kX ? L::addr_x(true, lw, r) : lw + L::index(true, 0u, r);
              __builtin_nontemporal_store(xr[r], &sd[ix].x);
              __builtin_nontemporal_store(xi[r], &sd[ix].y);
            });
          } else {
            splitr_for<0, NA>([&](auto Rc) {
              constexpr int r = decltype(Rc)::value;
              const unsigned ix = kX ? L::addr_x(false, lw, r) : lw + L::index(false, 0u, r);
              __builtin_nontemporal_store(xr[r], &sd[ix].x);
              __builtin_nontemporal_store(xi[r], &sd[ix].y);
            });
          }
        }
        ++snap_sub;
        snap_at = snap_sub < R.nsub ? splitrun_first(R, snap_sub + 1) + n_pre - 1 : (1 << 30);
      }
    }
  } else {
    for (int sg = 0; sg < n_full; ++sg) stage(sg, std::false_type{});
  }
  if (SPLITR_KWARM == 3) asm volatile("" ::"v"(warm_v));
  if (!SEG && n_full < n_stages) stage(n_stages - 1, std::true_type{});
  // the layout is the odd one when an odd number of full stages ran
  // (tan form defers the product of a stage's cosines to the next stage's D; a run that closes on the kick has no next
  // stage, so the row is finished here: prod_k cos(kick c_k) = 1 - O(1e-18) for the default kick, 1e-13 per atom for
  // long blocks set by the caller - a trace drift that accumulated over the blocks)
  double fl = (ROWS && n_full == n_stages) ? cprod : 1.0;
  if (ROWS && n_full == n_stages && !A.use_post) {
    splitr_for<0, NA>([&](auto Rc) {
      constexpr int r = decltype(Rc)::value;
      xr[r] *= fl;
      xi[r] *= fl;
    });
  }
  if (ROWS && A.use_post) {
    __syncthreads();
    if (t < NA) ftl[128 + t] = row_factor(1, odd ? L::index(true, 0u, t) : L::index(false, 0u, t), odd ? L::index(true, 0u, NA - 1) : L::index(false, 0u, NA - 1));
    __syncthreads();
    fl *= row_factor(1, odd ? L::index(true, tq, 0u) : L::index(false, tq, 0u), odd ? L::index(true, NT - 1, 0u) : L::index(false, NT - 1, 0u));
  }
  bool stored = false;
  if constexpr (!ROWS) {
    // (SEG: the sinks are chosen per segment)
    cplx* const e_dst = (!SEG || (seg_flags & SPLIT_SEG_DST)) ? A.dst : nullptr;
    cplx* const e_dst2 = (!SEG || (seg_flags & SPLIT_SEG_CMP)) ? A.dst2 : nullptr;
    const cplx* const e_cmp = (!SEG || (seg_flags & SPLIT_SEG_CMP)) ? A.cmp : nullptr;
    if (e_dst || e_dst2 || e_cmp) {
      // the controller's check (SplitArgs.dst / dst2 / cmp): out-of-place store, second store, comparison on the way out
      stored = true;
      const size_t boff = (size_t)b << N;
      cplx* __restrict__ out = e_dst ? e_dst + boff : st;
      cplx* __restrict__ out2 = e_dst2 ? e_dst2 + boff : nullptr;
      const cplx* __restrict__ ref = e_cmp ? e_cmp + boff : nullptr;
      unsigned lw = kX ? (odd ? L::index_x(true, tq, 0u) : L::index_x(false, tq, 0u)) : (odd ? L::index(true, tq, 0u) : L::index(false, tq, 0u));
      if constexpr (SEG) asm volatile("" : "+v"(lw));  // (not hoisted out of the segment loop: see the load)
      double dmax = 0.0, dsum = 0.0;
      auto put = [&](unsigned ix, double vx, double vy) {
        const cplx v = make_double2(vx, vy);
        out[ix] = v;
        if (out2) out2[ix] = v;
        if (ref) {
          const cplx c = ref[ix];
          const double dx = vx - c.x, dy = vy - c.y;
          const double d2 = fma(dx, dx, dy * dy);
          dmax = fmax(dmax, d2);
          dsum += d2;
        }
      };
      // (SPLITR_XPASS: the named T bits are XORed onto the lane's word, the other register bits added)
      if (odd) {
        splitr_for<0, NA>([&](auto Rc) { constexpr int r = decltype(Rc)::value; put(kX ? L::addr_x(true, lw, r) : lw + L::index(true, 0u, r), xr[r], xi[r]); });
      } else {
        splitr_for<0, NA>([&](auto Rc) { constexpr int r = decltype(Rc)::value; put(kX ? L::addr_x(false, lw, r) : lw + L::index(false, 0u, r), xr[r], xi[r]); });
      }
      if (ref) {
        for (int o = 32; o > 0; o >>= 1) {
          dmax = fmax(dmax, __shfl_xor(dmax, o, 64));
          dsum += __shfl_xor(dsum, o, 64);
        }
        double* red = reinterpret_cast<double*>(gtab);  // (the G tables are dead after the last stage)
        __syncthreads();
        if (l == 0) { red[2 * w] = dmax; red[2 * w + 1] = dsum; }
        __syncthreads();
        if (t == 0) {
          double m = red[0], sm = red[1];
          for (int k = 1; k < NT / 64; ++k) { m = fmax(m, red[2 * k]); sm += red[2 * k + 1]; }
          A.cmp_err[b] = m;                 // max |x - cmp|^2
          A.cmp_err[gridDim.y + b] = sm;    // sum |x - cmp|^2 (the 2-norm of the difference, squared)
        }
      }
    }
  }
  if (SEG && !stored) {
    // (the same store with the addresses formed here, from the laundered word of the lane)
    unsigned lw = kX ? (odd ? L::index_x(true, tq, 0u) : L::index_x(false, tq, 0u)) : (odd ? L::index(true, tq, 0u) : L::index(false, tq, 0u));
    asm volatile("" : "+v"(lw));
    if (odd) {
      splitr_for<0, NA>([&](auto Rc) { constexpr int r = decltype(Rc)::value; st[kX ? L::addr_x(true, lw, r) : lw + L::index(true, 0u, r)] = make_double2(xr[r], xi[r]); });
    } else {
      splitr_for<0, NA>([&](auto Rc) { constexpr int r = decltype(Rc)::value; st[kX ? L::addr_x(false, lw, r) : lw + L::index(false, 0u, r)] = make_double2(xr[r], xi[r]); });
    }
  }
  if (!SEG && !stored) {
  splitr_for<0, NA>([&](auto Rc) {
    constexpr int r = decltype(Rc)::value;
    const double f = (ROWS && A.use_post) ? fl * ftl[128 + r] : 1.0;
    const unsigned ix = kX ? (odd ? L::index_x(true, tq, r) : L::index_x(false, tq, r)) : (odd ? L::index(true, tq, r) : L::index(false, tq, r));
    st[ix] = make_double2(xr[r] * f, xi[r] * (ROWS ? f * csgn : f));
  });
  }
  }  // rows
}

template <int N, int NR, bool DECAY, bool ROWS = false, bool CPLX = false, bool SNAP = false>
__global__ __launch_bounds__(64 << (N - 6 - NR)) __attribute__((amdgpu_waves_per_eu(1, NR >= 6 ? 1 : 2))) void k_split_reg(const SplitArgs A, const SplitRun R, long long stage_stride) {
  split_reg_body<N, NR, DECAY, ROWS, CPLX, SNAP, false>(A, R, stage_stride);
}

// the plain real-drive ket kernel over the segments of R (R.nseg >= 1): same launch shape and LDS as k_split_reg<N, NR, false>
// (two waves per SIMD asked for, not merely allowed: with the load and the sinks inside the segment loop the allocator
// otherwise takes more than 256 vector registers at 12 and 13 atoms, and a CU holds one workgroup where the plain kernel has two)
template <int N, int NR>
__global__ __launch_bounds__(64 << (N - 6 - NR)) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_split_reg_seg(const SplitArgs A, const SplitRun R, long long stage_stride) {
  split_reg_body<N, NR, false, false, false, false, true>(A, R, stage_stride);
}

// the same two kernels for sequences whose atoms all see one drive and one detuning (UNI above): one coefficient record of 32
// bytes per sequence and stage (stage_stride = 4 B doubles).  Kernels of their own, not a template argument of the general
// ones: those keep their names and their code.
template <int N, int NR>
__global__ __launch_bounds__(64 << (N - 6 - NR)) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_split_reg_uni(const SplitArgs A, const SplitRun R, long long stage_stride) {
  split_reg_body<N, NR, false, false, false, false, false, true>(A, R, stage_stride);
}
template <int N, int NR>
__global__ __launch_bounds__(64 << (N - 6 - NR)) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_split_reg_seg_uni(const SplitArgs A, const SplitRun R, long long stage_stride) {
  split_reg_body<N, NR, false, false, false, false, true, true>(A, R, stage_stride);
}

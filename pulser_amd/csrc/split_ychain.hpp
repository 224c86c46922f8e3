// Part of librydemu (included by k_split_reg.hpp).  No device code: the hop plan of the y chain as data, checked at
// compile time.
// ---------------------------------------------------------------------------
// For a REAL drive the tan-form rotation of the index bit in lane direction m (partner = lane L ^ m),
//   x'(L) = x(L) - T y(L ^ m),   y'(L) = y(L) + T x(L ^ m),
// is two independent real rotations, on the pairs (x(L), y(L ^ m)) and (x(L ^ m), y(L)).  A lane that holds x(L) and
// Y = y(L ^ m) updates both locally - x' = fma(-T, Y, x), Y' = fma(T, x, Y): the same two FMAs on the same operands that
// lanes L and L ^ m execute when each fetches both parts of its partner, so the results are bit for bit the same - and
// only y has to travel.  y is kept SHIFTED: lane L holds y(L ^ s), and before the rotation of a bit the cumulative shift s
// must equal that bit's direction.  The hops between consecutive shifts are DPP patterns that are fixed-point-free
// involutions of the 16 lanes of a row, i.e. xors:
//   quad_perm [1,0,3,2] = xor 1    quad_perm [2,3,0,1] = xor 2    quad_perm [3,2,1,0] = xor 3
//   row_half_mirror     = xor 7    row_ror:8           = xor 8    row_mirror          = xor 15
// With the rotation order of k_split_reg (bit 0 = xor 1, bit 1 = xor 2, bit 3 = xor 8, bit 2 = xor 7: SPLITR_HM) the
// shifts 1, 2, 8, 7 take the hops 1, 3, (2, 8), 15 and 7 brings y home: six patterns = 12 moves per amplitude where the
// partner fetches take 16.  (A closed walk of five single hops does not exist: the cumulative shifts must be a basis of
// the 4-bit lane numbers and every step and the way home must come from the six xors above, which forces 7 twice.)
// STORE = 1: the last hop is left to the LDS pass - y stays shifted by SplitYPlan::final_shift and the lane stores it
// into the slot of lane t ^ final_shift (same wave, same 8-lane group, before the same barrier).
#pragma once

struct SplitYHop {
  int n;        // patterns of the hop (0: none, the shift stays)
  int ctrl[2];  // DPP control words, applied in this order
};

// xor mask of a DPP control word on the 16 lanes of a row, or -1 if it is none of the six involutions
constexpr int splity_xor_of(int ctrl) {
  return ctrl == 0xB1 ? 1 : ctrl == 0x4E ? 2 : ctrl == 0x1B ? 3 : ctrl == 0x141 ? 7 : ctrl == 0x128 ? 8 : ctrl == 0x140 ? 15 : -1;
}
// source lane of lane l under a DPP control word (v_mov_b32_dpp: dst[l] = src[source(l)]), from the ISA's definitions
constexpr int splity_dpp_source(int ctrl, int l) {
  if (ctrl >= 0 && ctrl <= 0xFF) return (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);  // quad_perm
  if (ctrl > 0x120 && ctrl <= 0x12F) return (l + 16 - (ctrl & 15)) & 15;            // row_ror:n
  if (ctrl == 0x140) return 15 - l;                                                 // row_mirror
  if (ctrl == 0x141) return (l & 8) | (7 - (l & 7));                                // row_half_mirror
  return -1;
}

template <int ND, int STORE>
struct SplitYPlan;

template <int STORE>
struct SplitYPlan<4, STORE> {
  static constexpr int order[4] = {0, 1, 3, 2};  // DPP bits in the order of their rotations
  static constexpr int dir[4] = {1, 2, 8, 7};    // lane direction of each (xor mask of the partner)
  static constexpr SplitYHop hops[5] = {{1, {0xB1, 0}}, {1, {0x1B, 0}}, {2, {0x4E, 0x128}}, {1, {0x140, 0}},
                                        STORE ? SplitYHop{0, {0, 0}} : SplitYHop{1, {0x141, 0}}};
  static constexpr int final_shift = STORE ? 7 : 0;
  static constexpr int fetch_moves = 16;  // dword moves per amplitude of the partner fetches this plan replaces
};
template <int STORE>
struct SplitYPlan<3, STORE> {
  static constexpr int order[3] = {0, 1, 2};
  static constexpr int dir[3] = {1, 2, 7};
  static constexpr SplitYHop hops[4] = {{1, {0xB1, 0}}, {1, {0x1B, 0}}, {2, {0x141, 0x4E}},
                                        STORE ? SplitYHop{0, {0, 0}} : SplitYHop{1, {0x141, 0}}};
  static constexpr int final_shift = STORE ? 7 : 0;
  static constexpr int fetch_moves = 12;
};
template <int STORE>
struct SplitYPlan<2, STORE> {
  static constexpr int order[2] = {0, 1};
  static constexpr int dir[2] = {1, 2};
  static constexpr SplitYHop hops[3] = {{1, {0xB1, 0}}, {1, {0x1B, 0}}, STORE ? SplitYHop{0, {0, 0}} : SplitYHop{1, {0x4E, 0}}};
  static constexpr int final_shift = STORE ? 2 : 0;
  static constexpr int fetch_moves = 8;
};

// dword moves per amplitude of a plan (two per pattern: a double is two dwords)
template <class PLAN, int ND>
constexpr int splity_moves() {
  int n = 0;
  for (int i = 0; i <= ND; ++i) n += 2 * PLAN::hops[i].n;
  return n;
}

// Replays the plan on the 16 lanes of a row as permutations: pos[l] = the lane whose y lane l holds.
//   0 = the plan is sound; otherwise the first rule it breaks:
//   1 a control word is none of the six involutions (or is not fixed-point free / not an involution when replayed)
//   2 before the rotation of a bit the cumulative shift is not that bit's direction
//   3 the final shift is not what the store expects
//   4 the order is not a permutation of the ND bits, or the directions are no basis (some lane pair is never rotated apart)
//   5 the plan does not save moves
template <class PLAN, int ND>
constexpr int splity_check() {
  int pos[16] = {};
  for (int l = 0; l < 16; ++l) pos[l] = l;
  int seen = 0, span[16] = {};
  span[0] = 1;
  for (int i = 0; i <= ND; ++i) {
    const SplitYHop h = PLAN::hops[i];
    if (h.n < 0 || h.n > 2) return 1;
    for (int k = 0; k < h.n; ++k) {
      const int x = splity_xor_of(h.ctrl[k]);
      if (x <= 0) return 1;
      int nxt[16] = {};
      for (int l = 0; l < 16; ++l) {
        const int s = splity_dpp_source(h.ctrl[k], l);
        if (s != (l ^ x) || s == l || splity_dpp_source(h.ctrl[k], s) != l) return 1;
        nxt[l] = pos[s];
      }
      for (int l = 0; l < 16; ++l) pos[l] = nxt[l];
    }
    if (i < ND) {
      if (PLAN::order[i] < 0 || PLAN::order[i] >= ND || (seen & (1 << PLAN::order[i]))) return 4;
      seen |= 1 << PLAN::order[i];
      for (int l = 0; l < 16; ++l)
        if (pos[l] != (l ^ PLAN::dir[i])) return 2;
      int grown[16] = {};
      for (int v = 0; v < 16; ++v)
        if (span[v]) grown[v] = grown[v ^ PLAN::dir[i]] = 1;
      for (int v = 0; v < 16; ++v) span[v] = grown[v];
    }
  }
  for (int l = 0; l < 16; ++l)
    if (pos[l] != (l ^ PLAN::final_shift)) return 3;
  int dim = 0;
  for (int v = 0; v < 16; ++v) dim += span[v];
  if (seen != (1 << ND) - 1 || dim != (1 << ND)) return 4;
  if (splity_moves<PLAN, ND>() >= PLAN::fetch_moves) return 5;
  return 0;
}

#define SPLITY_ASSERT_PLAN(ND_, STORE_)                                                                                                                   \
  static_assert(splity_check<SplitYPlan<ND_, STORE_>, ND_>() != 1, "y chain: a control word is not one of the six fixed-point-free involutions"); \
  static_assert(splity_check<SplitYPlan<ND_, STORE_>, ND_>() != 2, "y chain: the cumulative shift before a rotation is not that bit's direction");  \
  static_assert(splity_check<SplitYPlan<ND_, STORE_>, ND_>() != 3, "y chain: the final shift is not what the store expects");                       \
  static_assert(splity_check<SplitYPlan<ND_, STORE_>, ND_>() != 4, "y chain: the bits / directions do not cover the DPP lane bits");                \
  static_assert(splity_check<SplitYPlan<ND_, STORE_>, ND_>() == 0, "y chain: the plan takes no fewer moves than the partner fetches");
SPLITY_ASSERT_PLAN(4, 0)
SPLITY_ASSERT_PLAN(4, 1)
SPLITY_ASSERT_PLAN(3, 0)
SPLITY_ASSERT_PLAN(3, 1)
SPLITY_ASSERT_PLAN(2, 0)
SPLITY_ASSERT_PLAN(2, 1)
static_assert(splity_moves<SplitYPlan<4, 0>, 4>() == 12 && splity_moves<SplitYPlan<4, 1>, 4>() == 10, "y chain, 4 bits: 12 / 10 moves");
static_assert(splity_moves<SplitYPlan<3, 0>, 3>() == 10 && splity_moves<SplitYPlan<3, 1>, 3>() == 8, "y chain, 3 bits: 10 / 8 moves");
static_assert(splity_moves<SplitYPlan<2, 0>, 2>() == 6 && splity_moves<SplitYPlan<2, 1>, 2>() == 4, "y chain, 2 bits: 6 / 4 moves");

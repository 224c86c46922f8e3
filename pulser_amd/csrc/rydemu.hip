// rydemu.hip - MI355X (gfx950 / CDNA4) emulation core behind include/rydemu.h.
//
// What it computes (restating, from scratch, the arithmetic the reference hands
// to QuTiP at pulser-simulation/pulser_simulation/simulation.py:729-735):
//
//   sesolve:  d/dt psi = G(t) psi,   G = -i H(t)
//   mesolve:  d/dt rho = G(t) rho,   G = Lindbladian, rho as a 2N-bit vector
//
// with, in both cases, G a sum of
//   * a diagonal   g(i)           (interaction + detuning + dissipator diagonal)
//   * single-bit flips  coef_p[bit_p(i)] * x[i ^ 2^p]   (the Rabi drive)
//   * (mesolve) double flips on the digit pair (a_k, b_k)  (C rho C^+ jumps).
//
// Time stepping: commutator-free 4th-order Magnus (two exponentials per step of
// the Hamiltonian evaluated at the two Gauss points), each exponential by a
// Horner-form Taylor polynomial whose only primitive is the generator
// application  out = base + scale * (G~ x)  - the batched matrix-free
// "state-vector x Hamiltonian matvec" of the north star.
//
// Kernel design for CDNA4: one workgroup owns a tile of 2^T amplitudes
// (T = 12 -> 64 KiB of LDS, two workgroups per CU).  The tile is staged into
// LDS with coalesced 16-byte loads (each lane one complex128; the low C tile
// bits are the low address bits, so a wave reads whole 1 KiB / 256 B runs),
// every flip partner inside the tile is one ds_read_b128, and index bits that
// do not fit the tile are handled by further passes over a different tiling
// that accumulate into a partial-sum buffer.  HBM-bound by construction: the
// algorithmic traffic is 32 B per amplitude per application.
//
// No reference code is used; file:line citations name the behaviour restated.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/rydemu.h"

typedef double2 cplx;

#include "dev_common.hpp"
#include "k_apply.hpp"
#include "k_apply14.hpp"
#include "k_small.hpp"
#include "k_mc.hpp"
#include "k_mc_general.hpp"
#include "k_traj.hpp"
#include "k_traj_dm.hpp"
#include "k_ket.hpp"
#include "k_krylov.hpp"
#include "k_split.hpp"
#include "k_split_reg.hpp"
#include "k_split_reg_inst.hpp"
#ifdef RYD_SPLIT_TUS
// the register-resident split-operator kernels are compiled by rydemu_splitreg.hip (three part units, in parallel)
SPLITR_INSTANCES_12(SPLITR_EXTERN)
SPLITR_INSTANCES_13(SPLITR_EXTERN)
SPLITR_INSTANCES_14(SPLITR_EXTERN)
SPLITR_SEG_INSTANCES_12(SPLITR_SEG_EXTERN)
SPLITR_SEG_INSTANCES_12(SPLITR_UNI_EXTERN)
SPLITR_SEG_INSTANCES_13(SPLITR_SEG_EXTERN)
SPLITR_SEG_INSTANCES_13(SPLITR_UNI_EXTERN)
SPLITR_SEG_INSTANCES_14(SPLITR_SEG_EXTERN)
SPLITR_SEG_INSTANCES_14(SPLITR_UNI_EXTERN)
#endif
#include "k_observe.hpp"
#include "k_gen_observe.hpp"
#include "k_expect.hpp"
#include "k_overlap.hpp"
#include "k_general.hpp"
#include "host_handle.hpp"
#include "host_apply.hpp"
#include "host_general.hpp"
#include "host_sched.hpp"
#include "host_ket.hpp"
#include "host_krylov.hpp"
#include "host_split.hpp"
#include "host_step.hpp"
#include "host_mc_general.hpp"
#include "host_observables.hpp"
#include "k_ensemble.hpp"
#include "k_ptrace.hpp"
#include "k_ptrace_dm.hpp"
#include "host_replay.hpp"

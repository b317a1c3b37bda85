// MI355X (gfx950) kernels for the batched pick-and-place simulator.
//
// Hot path replaced (reference): PickPlaceGymEnv.step (mujoco_manip/gym_env.py:536-581)
//   = decode_action -> 16 x (IKController.compute controller.py:87-137 ; mujoco.mj_step env.py:121)
//     -> mujoco.mj_forward (gym_env.py:560) -> reward (gym_env.py:352-470) -> obs (gym_env.py:283-339)
// plus reset/randomization (gym_env.py:477-534, randomization.py:11-98) and the FSM expert
// (pick_and_place.py:167-291).
//
// Execution model: ONE ENVIRONMENT PER 64-LANE WORKGROUP (one wavefront).  The env record is
// read from HBM once per env step (coalesced, env-major), the 16 substeps run entirely out of
// the workgroup's LDS (state, body poses, mass matrix, contacts, constraint rows, Newton
// Hessian), and the record + observation are written back once.  Inside a substep the wave
// splits the work by phase:
//   serial tree recursions (kinematics, RNE, composite inertia, IK, integration): lane 0;
//   CRBA entries, body-pair/geom-pair broadphase + narrowphase, constraint-row assembly,
//   Newton gradient / Hessian / Cholesky / line search: all 64 lanes, joined by wave shuffles.
// Physics follows MuJoCo's documented pipeline (the fp64 oracle in oracle/ is the checker).
//
// This file is everything that is compiled once per LDS-row layout: the LDS record (EnvSh), the phases,
// substep / step_begin / step_finish, the six step kernels (mmx_env_step_kernel, its budgeted form on the
// one-wave layout, mmx_env_traj_kernel, mmx_env_policy_kernel, mmx_env_dagger_kernel, and the one-substep kernel
// of the physics harness) and their launchers.  It is included, never compiled on its own: by mmx_kernels.hip at the default
// MMX_LDSEFC = 128, which adds the kernels that exist once (forward, reset, expert, reward, queue, order), and
// by mmx_step_l192.hip at 192 rows with MMX_STEP_SUFFIX _l192 on the kernels' and launchers' names
// (MMX_STEP_SYM).
//
// The file itself holds the includes and the macros and constants every part shares; the text is in eight
// parts, included below in this order.  They are ordered fragments of one translation unit, not headers: each
// uses what the parts before it define (its opening comment says what), none includes anything, and none is
// included anywhere else.
//   mmx_step_lds.inc          the env's LDS: contact records, EnvSh, the scratch overlays, accessors, wave primitives
//   mmx_step_dynamics.inc     kinematics and dynamics
//   mmx_step_collision.inc    broadphase list, narrowphase passes, contact sort
//   mmx_step_constraints.inc  the constraint rows
//   mmx_step_solver.inc       the Newton solver (LANE is the opaque lane id inside it)
//   mmx_step_integrate.inc    implicitfast + advance, the IK, mj_step_wave and its barrier table
//   mmx_step_task.inc         numpy's PCG64, the task layer, record I/O
//   mmx_step_kernels.inc      step_end, substep / step_begin / step_finish, the fused step loop -- stated there once
//                             per wave (MMX_ENV_WAVE_STEPS, MMX_HELPER_WAVE_STEPS) with the kernel entry
//                             (MMX_STEP_KERNEL_ENTRY); the five fused kernels only add to it -- the kernels, the launchers
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include <type_traits>

#define MMX_MODEL_QUAL static __constant__
#include "mmx_model_gen.h"
#include "mmx_device.h"
#include "mmx_clock.h"
#include "mmx_geom.h"
#include "mmx_state.h"
#include "mmx_launch.h"
#include "mmx_policy.h"
#include "mmx_dagger.h"

#define WG 64  // lanes of the wave that runs a phase
// lane within the wave (a workgroup is one wave: one env)
// Lane id re-materialised per use (an opaque copy of threadIdx.x): nothing lane-derived (lane masks,
// per-lane dof / row indices) is hoisted to a function's entry and kept live across it.  In the
// Newton solver, where the substep's register peak sits, that frees registers.  When adopted (C3
// +2.4 %) it counted for the callee-saved save area the substep then had (592 -> 436 B per lane); the
// substep saves nothing for its caller now (MMX_NO_TAIL_MARK) and the copy still pays, through the
// substep's own spills: with the plain lane id 35 scratch stores / 48 loads and 315 SGPR-spill
// writelanes against 6 / 9 and 101 (128-row build), C3 -10.4 % (profiles/r07_ab_nocsr.json).  Applied
// everywhere it costs more re-materialisation than it saves (-0.6 %), and in the constraint /
// collision / integrate + IK sections as well -0.8 to -1.7 %.  So its scope is one file: mmx_step_solver.inc
// redefines LANE to it in its first lines and restores the plain lane id in its last.
DEV int lane_opaque() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t & 63;
}
#define LANE ((int)(threadIdx.x & 63))
// SYNC: wave-local LDS ordering (a phase runs on ONE wave: its lanes exchange data through LDS,
// whose operations a wave issues and completes in order, so no s_barrier / waitcnt is needed,
// only a compiler fence).  XSYNC: the workgroup barrier (s_barrier + memory fence) between env steps.
DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#define SYNC() wave_sync()
#define XSYNC() __syncthreads()

static constexpr float kDt = 0.002f;
static constexpr float kHome[7] = {1.5708f, -0.2f, 0.0f, -2.1f, 0.0f, 1.8f, 0.785f};  // controller.py:8
static constexpr int kBinBody[3] = {MMX_BODY_BIN_RED, MMX_BODY_BIN_GREEN, MMX_BODY_BIN_BLUE};

#define NSLOT 14  // arm bodies 1..11 -> slots 0..10, cubes 16..18 -> slots 11..13
#define MMX_CAND_MARGIN 0.08f  // m: the list's inflation of the sphere / plane test (A/B: 0.04 +0.2 %, 0.08 +0.8 %, 0.15 -0.6 %)
#define LD 28     // padded row stride for 27-wide rows

#include "mmx_step_lds.inc"
#include "mmx_step_dynamics.inc"
#include "mmx_step_collision.inc"
#include "mmx_step_constraints.inc"
#include "mmx_step_solver.inc"
#include "mmx_step_integrate.inc"
#include "mmx_step_task.inc"
#include "mmx_step_kernels.inc"

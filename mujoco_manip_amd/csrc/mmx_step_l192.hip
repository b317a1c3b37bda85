// The step kernels and their launchers a second time, with 192 constraint rows in LDS and two waves per
// env (the helper wave: MMX_STEP_HELPER in mmx_step_lds.inc; four envs per CU, 248 VGPRs).  What this object
// holds, every name with MMX_STEP_SUFFIX _l192 (mmx_step_kernels.inc):
//   mmx_env_step_kernel_l192    / mmx_launch_step_l192      env steps, host actions or the FSM expert
//   mmx_env_traj_kernel_l192    / mmx_launch_traj_l192      env steps with an action row and a record per step
//   mmx_env_policy_kernel_l192  / mmx_launch_policy_l192    env steps with an MLP policy's actions
//   mmx_env_dagger_kernel_l192  / mmx_launch_dagger_l192    env steps with the policy or the FSM expert, by a gate
//   mmx_substep_kernel_l192     / mmx_launch_physics_l192   the physics harness's one substep per launch
// (the budgeted step kernel exists on the one-wave layout only).  The 128-row build (twelve per CU) wins once the
// batch fills the workgroup slots; with four or fewer envs per CU each env's own speed is what counts
// and this one is faster (C2's 1024 envs: 1.52 M vs 1.29 M env steps/s).  mmx_api.cpp picks
// per sim from the batch size (mmx_set_step_rows, include/mmx_tuning.h).  Same sources, same arithmetic, bit-identical results: only where the rows past
// the LDS ones live and the register budget differ, and the two waves are ordered by workgroup barriers
// wherever one writes what the other reads (mj_step_wave in mmx_step_integrate.inc, MMX_HELPER_WAVE_STEPS in
// mmx_step_kernels.inc; tests/test_helper_layout.py delays either).
#define MMX_LDSEFC 192
#define MMX_STEP_SUFFIX _l192
#include "mmx_step.inc"
// mmx_api.cpp allocates S.efc_ovf with the 128-row build's per-env stride, which must cover this one's
static_assert(MMX_OVF_F <= MMX_OVF_F_AT(128), "overflow block stride exceeds the allocation");

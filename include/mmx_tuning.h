/* mmx_tuning.h — measurement and tuning entry points of libmmx.so (no reference counterpart).
 *
 * The reference boundary is include/mmx_api.h; a host binding of PickPlaceGymEnv needs nothing from
 * this header.  These calls report or choose how the batch is launched (rollout lanes and launch
 * lengths, the env-step kernel's LDS layout, the dispatch order of env steps) and time the launches
 * for bench.py.  None of them changes a result: every choice here is bit-identical to the default
 * (tests/test_gpu.py: test_step_layouts_agree, test_step_order_bit_identical,
 * test_rollout_lanes_bit_identical, test_fused_rollout_bit_identical; tests/test_step_budget.py).  Same
 * conventions as mmx_api.h (0 or a negative MMX_E* code, never an abort). */
#ifndef MMX_TUNING_H
#define MMX_TUNING_H
#include "mmx_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Constraint rows the env-step kernel (mmx_step, mmx_rollout_expert) keeps in LDS: 128 (twelve envs
 * per CU: the fastest layout once the batch fills the GPU's workgroup slots, C3 / C5 / dataset
 * generation) or 192 (four envs per CU, each with a second "helper" wave that runs its IK, dynamics and
 * GJK / EPA pairs beside the env wave's kinematics, broadphase and box pairs: faster per env, for
 * batches of at most four envs per CU, e.g. C2's 1024).  mmx_create picks by the batch size (192 up to
 * four envs per CU); env MMX_STEP_ROWS overrides at create.  The rows past the LDS ones live in the env's HBM overflow block; the two layouts are
 * bit-identical (a performance choice only).  MMX_EINVAL for any other value. */
int mmx_set_step_rows(mmx_sim* sim, int32_t rows);
int mmx_step_rows(const mmx_sim* sim);

/* Dispatch order of env-step launches (mmx_step, mmx_rollout_expert): 1 (default) = each launch's
 * envs longest first by FSM phase (a one-workgroup counting sort before the launch: the envs holding
 * an object, then closing / settling, then releasing, then the rest; within a phase class more
 * constraint rows in the last substep first), 0 = env index order.  Env
 * MMX_STEP_ORDER=0 sets 0 at create.  Only the hardware's workgroup schedule changes: results are
 * bit-identical either way.  MMX_EINVAL for other values; mmx_step_order returns -1 for NULL. */
int mmx_set_step_order(mmx_sim* sim, int32_t on);
int mmx_step_order(const mmx_sim* sim);

/* The most launches any rollout lane makes in mmx_rollout_expert(sim, n_env_steps): a launch runs
 * len = min(steps_per_launch, ceil(n / 4)) consecutive steps (1 with cameras); lane l of L starts with
 * a launch of l * len / L steps, then launches of len, then the remainder, so the lanes' launch
 * boundaries (each launch ends with a drain) do not fall together.  0 for a null sim or n <= 0. */
int mmx_rollout_launches(const mmx_sim* sim, int32_t n_env_steps);

/* Number of independent env ranges a multi-step rollout runs concurrently (one internal stream
 * each, forked from and joined back to cfg.stream; env MMX_STREAMS overrides the default of one
 * range per 1024 envs, at most 4).  Single-step calls always run as one launch on cfg.stream. */
int mmx_rollout_lanes(const mmx_sim* sim);

/* Render launches per rollout step: 1 with cameras (the env-step launch of all envs, then one render
 * launch over all envs), 0 without. */
int mmx_rollout_render_launches(const mmx_sim* sim);

/* 1 when camera rollouts (mmx_rollout_expert, more than one env step) render step k on a stream of
 * their own beside the env-step launch of step k + 1, the body poses double-buffered (the default
 * with cameras; env MMX_RENDER_OVERLAP=0 at create: render, then the next step); 0 otherwise.
 * Timing only: images and states are bit-identical either way. */
int mmx_rollout_render_overlap(const mmx_sim* sim);

/* Upper bound of the env steps one mmx_env_step_kernel launch runs per env in mmx_rollout_expert: 1
 * with cameras (every step is rendered), else 32 (env MMX_FUSE overrides).  A fused launch runs its
 * envs' steps back to back inside each workgroup; the trajectories are bit-identical to one
 * launch per step.  0 for a null sim. */
int mmx_rollout_steps_per_launch(const mmx_sim* sim);

/* Time-budgeted launches of mmx_rollout_expert (1, the default; env MMX_ROLLOUT_BUDGET=0 sets 0 at create):
 * on the 128-row layout without cameras, in calls whose lanes make at least 6 launches, a launch's
 * workgroups stop at about the same time instead of after the same number of env steps, so the slots a
 * launch frees are freed together and refilled by the lane's next launch.  The budget is the launch's
 * length times the lane's measured time per env step (summed on the device by the lane's earlier launches:
 * no host synchronisation); an env's step count stays within half a launch length of the fixed plan, the
 * lane's first launch and the last launches of a call taper to fixed counts, and the call leaves every env
 * at exactly n_env_steps.  So between the launches of one call envs may be at different step counts;
 * nothing a caller can observe changes, and the results are bit-identical either way (envs are independent
 * and plan, reset and step on the device).  mmx_step, the rollouts with per-step actions or a per-step
 * record, camera rollouts and the 192-row layout always run fixed counts.
 * MMX_EINVAL for other values; mmx_rollout_budget returns -1 for NULL.
 * mmx_rollout_step_counts waits for the sim's stream and copies out (host int32 [num_envs]) the env steps
 * each env made in the last budgeted call (zeros before one), and, when log is given, the counts after each
 * launch of the env's lane (host int32 [log_launches][num_envs], zero rows past the lane's launches;
 * log_launches must equal env MMX_ROLLOUT_LOG at create, which allocates the log: tests, diagnostics). */
int mmx_set_rollout_budget(mmx_sim* sim, int32_t on);
int mmx_rollout_budget(const mmx_sim* sim);
int mmx_rollout_step_counts(mmx_sim* sim, int32_t* out, int32_t* log, int32_t log_launches);

/* Per-launch kernel timing of mmx_rollout_expert (measurement): with enable = 1 every step-kernel
 * and render-kernel launch is bracketed by a HIP event pair on the stream it runs on (a new
 * collection starts); enable = 0 stops collecting.  mmx_kernel_times waits for the recorded events
 * and returns the summed launch durations (ms) and launch counts of each kernel; NULL skips a
 * field. */
int mmx_kernel_timing(mmx_sim* sim, int32_t enable);
int mmx_kernel_times(mmx_sim* sim, float* step_ms, int32_t* step_launches, float* render_ms,
                     int32_t* render_launches);

/* The render kernels' raster layout, read only (no sim needed): an image of side image_size is rendered
 * on a grid of side Sg = image_size rounded up to 16, in horizontal bands of mmx_render_band_rows rows (the
 * fewest bands whose rows fit the kernel's LDS z-buffer, balanced; 0 for a size outside 1 .. 1024), and one
 * workgroup takes mmx_render_bands_per_workgroup consecutive bands through that one z-buffer.
 * tests/test_render_flat_pixels.py pins the image per pixel at the sizes where this layout changes shape
 * and asserts the layout of those sizes through these calls. */
int mmx_render_band_rows(int image_size);
int mmx_render_bands_per_workgroup(void);

#ifdef __cplusplus
}
#endif
#endif

/* mmx_api.h — C-ABI of the MI355X batched pick-and-place simulator (libmmx.so).
 *
 * The reference path sits behind the Gymnasium Env API of PickPlaceGymEnv
 * (mujoco_manip/gym_env.py:39-602) and, below it, the MuJoCo C API reached through
 * pybind11 (mujoco.mj_step env.py:121, mj_forward gym_env.py:560, mj_jac controller.py:101).
 * This header is the boundary a host binding (ctypes here; cgo/JNI/N-API elsewhere) binds
 * to.  Plain C: no C++ or torch types, plain pointers and sizes.
 *
 * Conventions
 *  - every function returns 0 on success or a negative MMX_E* code and never aborts;
 *    mmx_last_error() gives a message;
 *  - device buffers are fp32/int32, env-major (one contiguous record per env, matching a
 *    torch [N, F] tensor): element (env i, field f) is at ptr[i * F + f];
 *  - sim-owned buffers returned by mmx_get_buffers stay valid until mmx_destroy;
 *  - all launches are asynchronous on the sim's stream (cfg.stream, or the null stream);
 *  - one sim per host thread at a time (not re-entrant); per-env faults go to the
 *    env_error buffer, never to return codes, except the reference's one raising case, spawn
 *    sampling exhaustion (MMX_ESAMPLING);
 *  - every entry point makes the sim's device (cfg.device) current for its HIP calls and
 *    restores the caller's current device before returning.
 */
#ifndef MMX_API_H
#define MMX_API_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMX_OK 0
#define MMX_EINVAL (-1)   /* bad argument (ValueError in the reference) */
#define MMX_EDEVICE (-2)  /* HIP runtime error */
#define MMX_ENOMEM (-3)   /* device allocation failed */
#define MMX_ESAMPLING (-4) /* object spawn sampling exhausted its 1000 attempts (RuntimeError in the
                              reference, randomization.py:84-87); reported by the synchronous
                              mmx_reset, and for autoresets inside steps / rollouts / the episode queue
                              by the next mmx_synchronize; the env's env_error carries bit 8 */

/* action modes, gym_env.py:30-36 */
enum { MMX_ACTION_ABS_POS = 0, MMX_ACTION_EE_POS_QUAT_G = 1, MMX_ACTION_EE_POS_ROT6D_G = 2,
       MMX_ACTION_EE_POS_QUAT_G_REL = 3, MMX_ACTION_EE_POS_ROT6D_G_REL = 4 };
/* reward types, gym_env.py:86 */
enum { MMX_REWARD_DENSE = 0, MMX_REWARD_SPARSE = 1, MMX_REWARD_STAGED = 2 };

typedef struct mmx_sim mmx_sim;

/* Constructor arguments of PickPlaceGymEnv (gym_env.py:62-75) plus batching knobs. */
typedef struct {
  int32_t num_envs;
  int32_t device;               /* HIP device ordinal */
  int32_t action_mode;          /* MMX_ACTION_* */
  int32_t reward_type;          /* MMX_REWARD_* */
  int32_t max_episode_steps;    /* truncation limit (constants.py:27) */
  int32_t randomize_objects;    /* randomization.py on reset */
  double spawn_x_range[2];      /* fp64: the spawn draws are numpy-identical fp64 */
  double spawn_y_range[2];
  int32_t n_tasks;              /* task pool (constants.py:11-25), objects/bins 0=red 1=green 2=blue */
  int8_t task_obj[9];
  int8_t task_bin[9];
  int32_t fixed_task_obj;       /* -1: sample from the pool (gym_env.py:511-517) */
  int32_t fixed_task_bin;
  int32_t image_size;           /* camera image side (any, <= 1024; sides that are multiples of 16 write
                                   whole dwords); 0 = no rendering */
  int32_t autoreset;            /* same-step autoreset on terminated/truncated/FSM done */
  int32_t solver_iterations;    /* Newton iteration cap (default 30) */
  float solver_tolerance;       /* relative gradient-norm tolerance (default 1e-6) */
  void* stream;                 /* hipStream_t, NULL = default stream */
} mmx_config;

/* Env-major device buffers (sim-owned): [N][F]. */
typedef struct {
  int32_t num_envs;
  float* qpos;               /* [N][30] */
  float* qvel;               /* [N][27] */
  float* ctrl;               /* [N][8]  */
  float* qacc_warmstart;     /* [N][27] */
  float* obs;                /* [N][85] numeric observation, gym_env.py:295-339 order */
  float* reward;             /* [N] */
  int32_t* done;             /* [N][3] terminated, truncated, success */
  float* reward_components;  /* [N][6] staged breakdown (gym_env.py:568-573) */
  int32_t* episode_i;        /* [N][18] obj, bin, step_count, flags, fsm_state, fsm_task_index,
                                fsm_settle, fsm_gripper_open, fsm_has_target, env_error, ncon, nefc,
                                episodes (resets so far), rng_has32, then sticky counters never
                                cleared by a reset: successes (episodes that ended with
                                info["success"] under autoreset), placed (episodes that ended with
                                the target cube in the target bin), error_resets (autoresets forced by
                                a diverged state: NaN / Inf / |qvel| or |qacc| >= 1e10, reported
                                as truncated), and fsm_phases (bitmask of the FSM states visited
                                since the last reset) */
  float* episode_f;          /* [N][28] T_init(12), hwm(5), target_kp(4), fsm_target(3), transit(3), return */
  float* kin;                /* [N][63] hand pos/mat, arm joint axes/anchors and cube positions of the
                                last position stage (what data.xpos holds after mj_step) */
  float* stats;              /* [N][19] sum nefc, sum ncon, sum solver iterations, substeps, max residual,
                                then shader-clock cycles spent per phase: ik, kinematics, dynamics,
                                collision, constraints, solver, integrate, step end (reward/obs/reset),
                                4 sub-phase probes (cycle fields: diagnostic build only, else 0), then
                                the substeps whose solve ended above the tolerance: by no progress
                                (step < 1e-9, an fp32 stall), by the iteration cap */
  float* contacts;           /* [N][64][13] dist, pos3, normal3, mu3 (slide, spin, roll), dim, geom1, geom2
                                (last substep) */
  uint8_t* images;           /* [N][2][S][S][3] RGB of the overhead and wrist cameras (S = image_size),
                                rendered after every reset / step / forward; NULL when image_size = 0 */
  uint8_t* seg;              /* [N][2][S][S] segment ids: 0 sky, 1 floor, 2 table, 3-5 bins (red, green,
                                blue), 6-8 cubes (red, green, blue), 9 robot; NULL when image_size = 0 */
  float* target;             /* [N][4] decoded EE target (IKController.compute's target_pos) + gripper
                                value of the current step; writable for physics-level harnesses */
} mmx_buffers;

void mmx_config_default(mmx_config* cfg);

/* PickPlaceGymEnv.__init__ (gym_env.py:62-208) for num_envs environments. */
int mmx_create(const mmx_config* cfg, mmx_sim** out);
void mmx_destroy(mmx_sim* sim);
const char* mmx_last_error(const mmx_sim* sim);

/* PickPlaceGymEnv.reset (gym_env.py:477-534) for the envs selected by env_mask (host,
 * N bytes, NULL = all).  seeds: host, N entries, or NULL to continue each env's stream
 * (gym semantics: reset(seed=None)).  seed_given: host, N bytes, NULL = all seeds valid.
 * task_override: host, N entries of (obj << 4 | bin), -1 = none (options["task"]).
 * Synchronous.  Returns MMX_ESAMPLING when an env's spawn sampling (randomize_objects) found no
 * separated placement in 1000 attempts: as where the reference raises, that env's cubes stay at the
 * keyframe and its task is not redrawn (its random stream stays the reference's); the others reset. */
int mmx_reset(mmx_sim* sim, const uint64_t* seeds, const uint8_t* seed_given, const int32_t* task_override,
              const uint8_t* env_mask);

/* PickPlaceGymEnv.step (gym_env.py:536-581): action_dev is a device pointer to [N][action_dim]
 * fp32 (row-major, env-major).  Runs decode -> 16 x (IK + mj_step) -> mj_forward -> reward -> obs. */
int mmx_step(mmx_sim* sim, const float* action_dev, int32_t action_dim);

/* Host helper of the dataset path (dataset.py collect_episodes, generate_dataset.py:250-260's
 * per-frame PNG files): copies n byte ranges, len[k] bytes from host address src[k] to dst[k]
 * (ranges must not overlap); returns the bytes copied, -1 on bad arguments (nothing copied).  One
 * call per camera and step appends every slot's new PNG file to its episode's buffer straight out of
 * the pinned copy of the step, with no Python object per frame (ctypes releases the GIL for the call). */
int64_t mmx_copy_ranges(int64_t n, const uint64_t* src, const uint64_t* dst, const int64_t* len);

/* PickAndPlaceTask.plan(n_steps) (pick_and_place.py:167-277) for every env; writes the
 * abs_pos action [N][4] = (target_xyz, gripper_val) to action_dev_out (may be NULL). */
int mmx_expert_plan(mmx_sim* sim, int32_t n_steps, float* action_dev_out);

/* Expert rollout driver (scripts/generate_dataset.py:140-196): n_env_steps x (plan(16) ->
 * step(abs_pos)); envs whose FSM is done auto-reset when cfg.autoreset is set.
 * Requires action_mode == MMX_ACTION_ABS_POS. */
int mmx_rollout_expert(mmx_sim* sim, int32_t n_env_steps);

/* Per-step record of a rollout: caller-owned device arrays [T][N][F] (T = n_env_steps), NULL = not
 * recorded.  Slice k holds what the sim-owned buffer of the same name (mmx_buffers) holds after env
 * step k of the rollout. */
typedef struct {
  float* obs;                /* [T][N][85] */
  float* reward;             /* [T][N] */
  int32_t* done;             /* [T][N][3] terminated, truncated, success */
  float* reward_components;  /* [T][N][6] */
  float* target;             /* [T][N][4] decoded EE target + gripper value (the expert's abs_pos action) */
  int32_t* episode_i;        /* [T][N][18] */
  float* qpos;               /* [T][N][30] */
  float* qvel;               /* [T][N][27] */
} mmx_trajectory;

/* Action-sequence rollouts (the driver loops of scripts/replay_actions.py:128-148 and
 * scripts/generate_dataset.py:140-196) in fused launches, with an optional per-step record.
 * mmx_rollout_actions steps every env through actions_dev, a device array [T][N][action_dim] fp32:
 * afterwards every sim-owned buffer is bit for bit what T calls mmx_step(actions_dev + k * N *
 * action_dim, action_dim), k = 0 .. T - 1, leave, and slice k of every array of rec is bit for bit what
 * the matching sim-owned buffer holds after the k-th of those calls.  mmx_rollout_expert_record is the
 * same against T x (mmx_expert_plan(16) -> mmx_step): mmx_rollout_expert with a record; rec->target is
 * then the expert's action.  Autoreset, truncation, divergence resets and MMX_ESAMPLING (reported by the
 * next mmx_synchronize) behave as in those loops; on the step an env autoresets the record holds, like
 * the buffers, the first observation of the new episode (the ended episode's final observation is not
 * kept).  With cameras the images / seg buffers hold the last step's frame; images are not recorded.
 * rec may be NULL (nothing recorded); the arrays must stay valid until the sim's stream has run the
 * rollout.  n_env_steps == 0 does nothing and returns MMX_OK.  MMX_EINVAL, with nothing launched, for a
 * NULL sim, NULL actions_dev, n_env_steps < 0, action_dim below the action mode's dimension, and for
 * mmx_rollout_expert_record on a sim whose action_mode is not MMX_ACTION_ABS_POS. */
int mmx_rollout_actions(mmx_sim* sim, const float* actions_dev, int32_t action_dim, int32_t n_env_steps,
                        const mmx_trajectory* rec);
int mmx_rollout_expert_record(mmx_sim* sim, int32_t n_env_steps, const mmx_trajectory* rec);

/* Snapshot and restore of whole environments on the device, one to many (no reference counterpart: the
 * reference has one env per process and no state setter; sampling planners, branching data collection,
 * curriculum restarts and failure debugging start many envs from one state).  A restored env continues
 * bit for bit as the env the record was taken from would have: a record holds every per-env array a
 * launch reads or a facade returns, in this fixed order (_lib.SNAPSHOT_FIELDS mirrors it):
 *     rng                [4] uint64   PCG64 state hi, lo, increment hi, lo
 *     rng32              [1] uint32   buffered upper half of the last 64-bit draw
 *     qpos               [30] fp32
 *     qvel               [27] fp32
 *     ctrl               [8] fp32
 *     qacc_warmstart     [27] fp32
 *     kin                [63] fp32    the stale kinematics cache the IK and the FSM read
 *     target             [4] fp32
 *     episode_i          [18] int32   whole, the sticky counters included: a branch is a copy
 *     episode_f          [28] fp32
 *     obs                [85] fp32
 *     reward             [1] fp32
 *     reward_components  [6] fp32
 *     done               [3] int32
 *     rpose              [168] fp32   body poses the cameras draw from; only when image_size > 0
 * The fields are packed (1236 bytes) and padded to MMX_SNAPSHOT_BYTES = 1248; a sim with cameras appends
 * rpose there: MMX_SNAPSHOT_BYTES_CAMERAS = 1920.  mmx_snapshot_bytes returns the sim's record size (-1 for
 * a NULL sim); it depends on nothing else in the configuration.
 * Not in a record: contacts and stats (diagnostics of the last launch; the next step overwrites them), the
 * images and segment ids (redrawn on restore), the episode queue's slot table, the sim-level
 * sampling-fault flag (MMX_ESAMPLING) and the configuration.
 * mmx_snapshot writes N records into caller-owned device memory, 16-byte aligned: record i is env i, at
 * snap_dev + i * rec_bytes.  mmx_restore: env i takes record src_dev[i] (device int32 [N]) of the n_records
 * records at snap_dev; -1, or any value outside [0, n_records), leaves env i exactly as it is and nothing
 * outside the blob is ever read; src_dev == NULL: env i takes record i where i < n_records and is kept
 * otherwise.  One record may go to any number of envs (the branch).  With cameras the restored envs, and
 * only those, are re-rendered from the restored poses with the sim's current render effects: their images
 * and seg are then what they were at snapshot time (under the same effects).
 * Both are asynchronous on the sim's stream, ordered with steps and rollouts like any other launch.
 * MMX_EINVAL, with nothing launched, for a NULL sim, a NULL (or not 16-byte aligned) blob, rec_bytes !=
 * mmx_snapshot_bytes(sim), or n_records < 0; n_records == 0 does nothing and returns MMX_OK.
 * A blob may be restored into another sim of the same process and device, with another num_envs and
 * another step layout; the record size rejects a camera / no-camera mismatch.  A different action mode,
 * reward type, episode limit or solver setting between the two sims is the caller's responsibility: the
 * record carries state, not configuration. */
#define MMX_SNAPSHOT_BYTES 1248
#define MMX_SNAPSHOT_BYTES_CAMERAS 1920
int64_t mmx_snapshot_bytes(const mmx_sim* sim);
int mmx_snapshot(mmx_sim* sim, void* snap_dev, int64_t rec_bytes);
int mmx_restore(mmx_sim* sim, const void* snap_dev, int64_t rec_bytes, int32_t n_records,
                const int32_t* src_dev);

/* MPPI planning on the device: sample, branch, roll out, reweight (no reference counterpart: the sampling
 * planner that mmx_snapshot / mmx_restore were added for, as one library call with no host round trip).
 * Information-theoretic model-predictive path integral control; random shooting is its temperature-0 limit.
 * One camera-less planner sim of N = M * K envs serves M controlled envs with K candidates each: planner
 * env i = m * K + k rolls out candidate k of controlled env m.  A is the planner sim's action dimension
 * (4, 8 or 10).
 * mmx_mppi_plan, asynchronous on the planner sim's stream, with no host synchronisation and no device
 * allocation after mmx_mppi_create:
 *  1. sample: xi is the caller's xi_dev or the library's draw, Philox4x32-10 with key = seed and counter =
 *     (call low, call high, i, 4 t + a / 4), whose four outputs give two Box-Muller pairs: component a takes
 *     normal a % 4 of its block, so element (t, i, a) depends on seed, call, t, i and a only, never on K, M or
 *     the launch shape.  eps_0 = xi_0, eps_t = beta eps_{t-1} + sqrt(1 - beta^2) xi_t; candidate k = 0 of
 *     every group gets eps = 0 (the nominal plan is always a candidate, whatever xi_dev holds); then
 *     actions[t][i][a] = clamp(nominal[t][m][a] + sigma[a] eps[t][i][a], low[a], high[a]);
 *  2. branch: planner env i takes record i / K of the n_records = M records at snap_dev (the restore kernel
 *     of mmx_restore with a src array built at create).  rec_bytes may be MMX_SNAPSHOT_BYTES or
 *     MMX_SNAPSHOT_BYTES_CAMERAS: the planner reads the fixed MMX_SNAPSHOT_BYTES prefix of each record at
 *     stride rec_bytes, so a controlled sim with cameras can be planned for (mmx_restore itself keeps
 *     rejecting a size mismatch);
 *  3. roll out: actions through the machinery of mmx_rollout_actions, reward and done recorded;
 *  4. reweight: R_i = sum_t gamma^t reward[t][i] alive_t with alive_0 = 1, alive_{t+1} = alive_t and not
 *     (terminated_t or truncated_t): the ending step's reward counts, nothing after it.  A candidate whose
 *     return is not finite (a test of the bits) is excluded: weight 0.  Per group: best = the argmax of R
 *     (lowest k on ties), w_k = exp((R_k - max R) / lambda) normalised to sum 1, or one-hot on best when
 *     temperature == 0; nominal'[t][m] = sum_k w_k actions[t][i] (kept within [low, high]);
 *     action_out[m] = nominal'[0][m]; then the shift nominal[t] = nominal'[t + 1] for t < H - 1, the last
 *     step repeated.  A group whose candidates are all excluded keeps its nominal as it was (no shift), gets
 *     weights 0 and best -1, and action_out[m] = nominal[0][m].  Every sum has a fixed order and no
 *     floating-point atomics: the same inputs give the same bits on every run.
 * MMX_EINVAL, with nothing launched, for a NULL planner, blob or output, a blob that is not 16-byte aligned,
 * rec_bytes other than the two record sizes, and n_records != M.  mmx_mppi_create returns MMX_EINVAL for a
 * config field outside its stated range, low[a] > high[a], sigma[a] < 0 or a value of these that is not
 * finite (a < A; an unbounded component takes +-FLT_MAX), a planner sim with cameras (rendering candidates
 * is waste) and num_envs % samples != 0.  mmx_mppi_reset sets every step of
 * every nominal plan to action_dev [M][A] (kept within [low, high]) and the call counter to 0; the counter
 * increments by one per successful mmx_mppi_plan call, with caller-supplied xi_dev too.  The planner never
 * touches the controlled sim: the caller snapshots it, and orders that snapshot before the plan call when
 * the two sims use different streams; snap_dev, xi_dev and action_out_dev must stay valid until the planner
 * sim's stream has run the call.  Equal configuration of the two sims is the caller's responsibility,
 * as for mmx_restore.  mmx_mppi_destroy before mmx_destroy of the planner sim; the buffers of
 * mmx_mppi_get_buffers are valid until then. */
#define MMX_MPPI_MAX_HORIZON 64
#define MMX_MPPI_MAX_ADIM 10
typedef struct mmx_mppi mmx_mppi;
typedef struct {
  int32_t horizon;      /* H env steps per candidate, 1 .. MMX_MPPI_MAX_HORIZON */
  int32_t samples;      /* K >= 2 candidates per controlled env; planner num_envs % K == 0, M = num_envs / K */
  float temperature;    /* lambda > 0 (with a finite 1 / lambda): w_k ~ exp((R_k - max R) / lambda); 0: all
                           weight on the best candidate, lowest k on ties */
  float discount;       /* gamma in (0, 1] */
  float noise_beta;     /* in [0, 1): eps_0 = xi_0, eps_t = beta eps_{t-1} + sqrt(1 - beta^2) xi_t */
  float sigma[MMX_MPPI_MAX_ADIM], low[MMX_MPPI_MAX_ADIM], high[MMX_MPPI_MAX_ADIM];  /* per action component;
                           the first A are read */
  uint64_t seed;
} mmx_mppi_config;
typedef struct {        /* planner-owned device arrays, valid until mmx_mppi_destroy; i = m * K + k */
  float* nominal;       /* [H][M][A] */
  float* noise;         /* [H][M*K][A] eps of the last call (0 for k == 0) */
  float* actions;       /* [H][M*K][A] the candidates the last call rolled out */
  float* reward;        /* [H][M*K] */
  int32_t* done;        /* [H][M*K][3] */
  float* returns;       /* [M*K] */
  float* weights;       /* [M*K], each group of K sums to 1 */
  int32_t* best;        /* [M] argmax_k R within the group */
} mmx_mppi_buffers;
int  mmx_mppi_create(mmx_sim* planner, const mmx_mppi_config* cfg, mmx_mppi** out);
void mmx_mppi_destroy(mmx_mppi* p);
int  mmx_mppi_reset(mmx_mppi* p, const float* action_dev /* [M][A]: every step of every nominal plan */);
int  mmx_mppi_plan(mmx_mppi* p, const void* snap_dev, int64_t rec_bytes, int32_t n_records,
                   const float* xi_dev /* NULL, or [H][M*K][A] standard-normal draws */,
                   float* action_out_dev /* [M][A] */);
int  mmx_mppi_get_buffers(mmx_mppi* p, mmx_mppi_buffers* out);
/* Reweight-layer harness: step 4 of mmx_mppi_plan alone, on the planner's reward, done, actions and nominal
 * arrays as they stand (a test writes its own rewards and done flags there): returns, weights, best, the
 * shifted nominal and action_out as after a plan call.  No sampling, branch or rollout, and the call counter
 * stays.  Asynchronous on the planner sim's stream; MMX_EINVAL for a NULL planner or output. */
int  mmx_mppi_reweight(mmx_mppi* p, float* action_out_dev);

/* Closed-loop MLP policies inside the fused step launches (no reference counterpart: the reference steps one env
 * per process from Python, so a learned policy there is a torch call between two env.step() calls; here the env's
 * own wave evaluates a_t = pi(obs_t) between two env steps of one launch and the observation never leaves the
 * device).  The network is a multi-layer perceptron on the numeric observation [85]:
 *     x = (obs - obs_shift) * obs_scale            (a scale of 0 drops an entry)
 *     h_l = act(W_l h_{l-1} + b_l), l < n_layers - 1;   mean = W_last h + b_last        (fp32; one accumulator per
 *     neuron that starts at the bias and adds the inputs in ascending order with fused multiply-adds; tanh as
 *     1 - 2 / (1 + exp2(2 x log2 e)) with the hardware's exp2 and reciprocal, within 8 * 2^-24 of tanh, exactly +-1
 *     for |x| >= 23 and 0 at 0)
 *     action[a] = clamp(mean[a] + exp(log_std[a]) z[a], low[a], high[a])
 * z is the draw of mmx_mppi_plan's step 1: element (rollout step t, env i, component a) of call `call` under the
 * policy's seed is Philox4x32-10 with key = seed and counter = (call low, call high, i, 4 t + a / 4), Box-Muller on
 * its outputs; it depends on (seed, call, t, i, a) alone, never on lanes or the launch plan.
 * mmx_policy_config: every pointer is a HOST pointer, read during mmx_policy_create only.  n_layers in 1 ..
 * MMX_POLICY_MAX_LAYERS linear layers (1: a linear policy); width[l] in 1 .. MMX_POLICY_MAX_WIDTH = the outputs of
 * layer l, the last one the action dimension (<= MMX_MPPI_MAX_ADIM) of the sims the policy will drive; activation
 * after every layer but the last; weight[l] row-major [width[l]][inputs] (torch.nn.Linear.weight), inputs = 85 for
 * l = 0 and width[l - 1] after; bias[l] [width[l]] or NULL (0); obs_shift, obs_scale [85] or NULL (0, 1); log_std
 * [A] or NULL (deterministic: action = clamp(mean)); low, high [A] or NULL (no clamp).
 * mmx_policy_create copies everything to the sim's device once (weights transposed and padded for the kernel's
 * coalesced reads, exp(log_std) evaluated on the host) and allocates nothing afterwards; MMX_EINVAL, with nothing
 * allocated, for a NULL argument, n_layers outside 1 .. 4, a width outside 1 .. 256, a last width above
 * MMX_MPPI_MAX_ADIM, a NULL weight[l] or an unknown activation.  mmx_policy_destroy frees it (before mmx_destroy
 * of the creating sim, after the last launch that uses it has run).
 * mmx_policy_eval: the network alone, mean_out_dev [n][A] from obs_dev [n][85] (device pointers; one wave per
 * row), asynchronous on the creating sim's stream: behaviour-cloning validation on dataset observations.
 * MMX_EINVAL for a NULL argument or n < 0; n == 0 does nothing.
 * mmx_rollout_policy: n_env_steps env steps of every env of `sim` in the fused launches of mmx_rollout_actions
 * (lanes, launch plan, dispatch order, both camera paths), the action of rollout step t and env i computed from
 * the observation that env holds before the step (the sim's obs buffer: after an autoreset the new episode's first
 * observation) and written to prec->actions[t][i][0 .. A) (device, [T][N][A], required); prec->mean (the network's
 * output) and prec->noise (z; 0 for a deterministic policy) are optional, same shape.  rec: the per-step record of
 * mmx_rollout_actions, may be NULL.  call: the caller increments it per call for fresh noise.  With cameras the
 * policy still reads the numeric observation only.
 * Contract: afterwards every sim-owned buffer and every slice of rec is bit for bit what mmx_rollout_actions(sim,
 * prec->actions, A, n_env_steps, rec) gives from the same starting state.
 * n_env_steps == 0 returns MMX_OK; MMX_EINVAL, with nothing launched, for a NULL sim, policy, prec or
 * prec->actions, n_env_steps < 0, a policy whose action width is not the sim's action dimension, and a policy
 * created on another device. */
#define MMX_POLICY_MAX_LAYERS 4
#define MMX_POLICY_MAX_WIDTH 256
#define MMX_POLICY_TANH 0
#define MMX_POLICY_RELU 1
typedef struct mmx_policy mmx_policy;
typedef struct {
  int32_t n_layers;
  int32_t width[MMX_POLICY_MAX_LAYERS];
  int32_t activation;   /* MMX_POLICY_TANH, MMX_POLICY_RELU */
  const float* weight[MMX_POLICY_MAX_LAYERS];
  const float* bias[MMX_POLICY_MAX_LAYERS];
  const float* obs_shift;
  const float* obs_scale;
  const float* log_std;
  const float* low;
  const float* high;
  uint64_t seed;
} mmx_policy_config;
typedef struct {        /* caller-owned device arrays [T][N][A] */
  float* actions;       /* required: the actions the envs were stepped with */
  float* mean;          /* NULL, or the network's output before noise and clamp */
  float* noise;         /* NULL, or z */
} mmx_policy_record;
int  mmx_policy_create(mmx_sim* sim, const mmx_policy_config* cfg, mmx_policy** out);
void mmx_policy_destroy(mmx_policy* p);
int  mmx_policy_eval(mmx_policy* p, const float* obs_dev, int32_t n, float* mean_out_dev);
int  mmx_rollout_policy(mmx_sim* sim, mmx_policy* policy, int32_t n_env_steps, uint64_t call,
                        const mmx_policy_record* prec, const mmx_trajectory* rec);

/* Fitting a policy on the device (no reference counterpart): minibatch gradient steps of the mean-squared error
 * between the network's output (mean: before noise and clamp) and given targets, which update the policy's packed
 * weights in place on the creating sim's stream; the next mmx_rollout_policy, mmx_rollout_dagger or mmx_policy_eval
 * on that stream runs the new weights with nothing in between.  Every layer's weights and biases are trained (a
 * bias that was NULL at create starts from 0); obs_shift, obs_scale, log_std, low and high are not.
 *     L = 1 / (B A) sum_{s < B, a < A} (mean(obs[p_s])[a] - target[p_s][a])^2,   B = cfg->batch
 * Optimisation step k (k = t - 1; t counts the policy's steps from 1 across calls) draws pair p_s of sample s as
 *     shuffle 0: (k B + s) mod n_pairs (sequential sweeps);
 *     shuffle 1: (uint64(x) n_pairs) >> 32, x = word s % 4 of Philox4x32-10 with key = cfg->seed and counter =
 *                (k low, k high, s / 4, 0xF17BA7C4): with replacement, a function of (seed, k, s) alone.
 * MMX_FIT_SGD: w = fma(-lr, g, w).  MMX_FIT_ADAM (torch.optim.Adam's defaults: no weight decay, no amsgrad), one
 * rounding per operation: m = fma(beta1, m, (1 - beta1) g); v = fma(beta2, v, ((1 - beta2) g) g); w = w - (lr (m c1))
 * / (sqrt(v c2) + eps), c1 = 1 / (1 - beta1^t) and c2 = 1 / (1 - beta2^t) evaluated per step on the host in fp64 and
 * rounded to fp32; IEEE square root and division.  m, v and t belong to the policy and persist across calls;
 * cfg->reset_optimizer = 1 zeroes them before the call's first step.  SGD advances t too (it numbers the batches).
 * Everything is fp32; the gradient sums run over the samples in a fixed order (tiles of 16 samples, chunks of 512,
 * then chunk by chunk): there are no atomics, and the same call on the same state gives the same bits every time.
 * mmx_policy_fit: obs_dev [n_pairs][85], target_dev [n_pairs][A] (device pointers, read by every step's launches:
 * keep them unchanged until the stream has run them); n_steps optimisation steps are queued without a host
 * synchronisation; loss_out_dev [n_steps] (device) or NULL: loss_out[i] = the batch loss before update i of this
 * call.  The first call allocates the workspace (activations, deltas, partial sums, m, v) and a later call with a
 * larger batch synchronises the stream and grows it; mmx_policy_create allocates none of it, mmx_policy_destroy
 * frees it.  A policy shared by several sims is fitted on its creator's stream only: ordering against rollouts of
 * the other sims (other streams) is the caller's responsibility.
 * MMX_EINVAL, with nothing touched, for a NULL p, obs_dev, target_dev or cfg, n_pairs < 1 or > 2^31 - 1, n_steps < 0
 * (0 does nothing), batch outside 1 .. MMX_FIT_MAX_BATCH, an unknown optimizer, lr or eps not finite or <= 0,
 * beta1 or beta2 outside [0, 1).
 * mmx_policy_get_weights: synchronises the stream and copies the layers out in mmx_policy_config's layout
 * (weight_host[l] [width[l]][inputs], bias_host[l] [width[l]]; host pointers; bias_host or an entry of either NULL:
 * skipped).  mmx_policy_set_weights: the reverse, in place on the stream (returns when the copy is done; a NULL
 * bias_host or bias_host[l]: zeros; every weight_host[l] required); m, v and t stay as they are. */
#define MMX_FIT_SGD 0
#define MMX_FIT_ADAM 1
#define MMX_FIT_MAX_BATCH 65536
typedef struct {
  int32_t optimizer;       /* MMX_FIT_SGD | MMX_FIT_ADAM */
  int32_t batch;           /* 1 .. MMX_FIT_MAX_BATCH */
  int32_t shuffle;         /* 0: sequential sweeps, 1: Philox draws with replacement */
  int32_t reset_optimizer; /* 1: zero m, v and t before the first step of this call */
  float lr, beta1, beta2, eps;
  uint64_t seed;
} mmx_fit_config;
int  mmx_policy_fit(mmx_policy* p, const float* obs_dev, const float* target_dev, int64_t n_pairs, int32_t n_steps,
                    const mmx_fit_config* cfg, float* loss_out_dev);
int  mmx_policy_get_weights(mmx_policy* p, float* const* weight_host, float* const* bias_host);
int  mmx_policy_set_weights(mmx_policy* p, const float* const* weight_host, const float* const* bias_host);

/* Policy-gradient fits on the device (no reference counterpart): generalised advantage estimation (Schulman et al.
 * 2016) over a rollout record, and PPO's clipped surrogate (Schulman et al. 2017) as a second objective of the fit
 * above.  A critic is an mmx_policy of width 1 (log_std, low, high NULL) fitted with mmx_policy_fit on the returns;
 * roll out -> mmx_policy_eval of the critic -> mmx_gae -> mmx_policy_fit_pg and mmx_policy_fit -> roll out runs
 * with the observations, actions and weights never leaving the device.  Everything is fp32 in a stated operation
 * order (csrc/mmx_pg.h), without atomics: the same call on the same state gives the same bits every time.
 * mmx_gae: per env column i, t from T - 1 down to 0,
 *     end   = done[t][i][0] != 0 (terminated) || done[t][i][1] != 0 (truncated)
 *     nv    = end ? 0 : (t == T - 1 ? value_last[i] : value[t + 1][i])
 *     delta = fma(gamma, nv, reward[t][i]) - value[t][i]
 *     adv[t][i] = end ? delta : fma(gamma lambda, adv[t + 1][i], delta);      ret[t][i] = adv[t][i] + value[t][i]
 * value[t][i] = V of the observation env i held before step t, value_last[i] = V of the observation after the last
 * step.  A truncated step takes next value 0 like a terminated one: the record keeps the new episode's first
 * observation, not the ended one's last, so the cut-off state's value cannot be evaluated from it.  normalize != 0
 * rescales adv_out (not ret_out) afterwards over all n = T N entries: mean = sum / n, var = sum (x - mean)^2 / n,
 * adv = (adv - mean) / (sqrt(var) + 1e-8), both sums in an order fixed by n alone.  Device pointers; asynchronous on
 * the sim's stream; N need not be the sim's num_envs; ret_out_dev may be NULL.  T == 0 returns MMX_OK; MMX_EINVAL,
 * with nothing launched, for a NULL sim, cfg or required pointer, T < 0, N < 1, T N > 2^31 - 1, gamma or lambda
 * outside [0, 1] or not finite.
 * mmx_policy_fit_pg: mmx_policy_fit with the objective (B = cfg->fit.batch, pairs p_s drawn as there)
 *     L = -1 / B sum_{s < B} min(r_s Adv[p_s], clamp(r_s, 1 - clip, 1 + clip) Adv[p_s]),
 *     r_s = exp(sum_a 0.5 (z_a^2 - z'_a^2)),  z = noise[p_s],  z'_a = (fma(std_a, z_a, mean_old[p_s][a]) - mean_a) / std_a
 * the ratio of the Gaussian densities, now and at the rollout, of the sample BEFORE the clamp (the clamp is part of
 * the environment); mean = the network's output now; mean_old_dev and noise_dev [n_pairs][A] are a rollout's
 * mmx_policy_record, adv_dev [n_pairs] mmx_gae's output.  std = exp(log_std) is not trained: with it fixed the ratio
 * needs nothing else.  stats_out_dev [n_steps][3] (device) or NULL: per step, before its update, the surrogate loss
 * L, the approximate KL 1 / B sum ((r_s - 1) - log r_s), and the fraction of samples whose gradient the clip removed.
 * m, v, t, the batch draw, the workspace, stream ordering and the in-place update are mmx_policy_fit's, shared with
 * it: a step of either objective advances the same t.
 * MMX_EINVAL, with nothing touched, for everything mmx_policy_fit refuses (mean_old_dev, noise_dev and adv_dev are
 * required), a deterministic policy (created without log_std, or any std[a] == 0 for a < A), clip not finite or
 * outside (0, 1).
 * mmx_policy_set_log_std: std[a] = exp(log_std_host[a]) evaluated on the host in fp64 as mmx_policy_create does, written
 * into the policy in place on the stream (returns when the copy is done); nothing else of the policy changes, and a
 * policy created without log_std draws noise from then on.  MMX_EINVAL for a NULL argument or an entry not finite. */
typedef struct { float gamma, lambda; int32_t normalize; } mmx_gae_config;
int  mmx_gae(mmx_sim* sim, const mmx_gae_config* cfg, int32_t T, int32_t N, const float* reward_dev,
             const int32_t* done_dev, const float* value_dev, const float* value_last_dev, float* adv_out_dev,
             float* ret_out_dev);
typedef struct { mmx_fit_config fit; float clip; } mmx_pg_config;
int  mmx_policy_fit_pg(mmx_policy* p, const float* obs_dev, const float* mean_old_dev, const float* noise_dev,
                       const float* adv_dev, int64_t n_pairs, int32_t n_steps, const mmx_pg_config* cfg,
                       float* stats_out_dev);
int  mmx_policy_set_log_std(mmx_policy* p, const float* log_std_host);

/* DAgger rollouts (Ross et al. 2011; no reference counterpart): mmx_rollout_policy with the FSM expert beside the
 * learner, in the same fused launches (lanes, launch plan, dispatch order, both camera paths; with cameras the
 * numeric observation is read and the images hold the last frame).  Per rollout step t and env i, inside the launch:
 *   1. the learner's action a_policy = the policy's action of the observation the env holds (mean, noise, clamp: as
 *      mmx_rollout_policy, the same draws);
 *   2. the expert's label a_expert = what mmx_expert_plan(sim, 16, .) returns at that state.  The expert plans at
 *      EVERY step, whoever acts: its FSM only moves when it plans, so it shadows the learner as it does in a loop
 *      that calls mmx_expert_plan ahead of every mmx_step;
 *   3. the gate.  bit 0 (Bernoulli): u < cfg->beta, u in [0, 1) the second uniform of the policy's draw at component
 *      12 = Philox4x32-10 with key = the policy's seed, counter = (call low, call high, i, 4 t + 3), u = (x1 >> 8)
 *      2^-24: the counter word no noise component uses, a function of (seed, call, t, i) alone, never of lanes or
 *      the launch plan; beta = 0 never fires, beta = 1 always.  bit 1 (takeover; off when cfg->takeover_dist == 0):
 *      d = a_policy - a_expert over xyz, d2 = fma(dz, dz, fma(dy, dy, dx dx)) in fp32, d2 > takeover_dist^2: the
 *      expert intervenes when the learner strays;
 *   4. the env is stepped with a_expert (all four components) when the gate is not 0, else with a_policy.
 * mmx_dagger_record: caller-owned device arrays; actions is required, every other may be NULL.  obs_in[t][i] is the
 * observation the learner was given at step t (after an autoreset: the new episode's first), which pairs with
 * expert_action[t][i] as a training example.  rec: the per-step record of mmx_rollout_actions, may be NULL.
 * Contract: afterwards every sim-owned buffer and every slice of rec is bit for bit what the loop
 * mmx_expert_plan(sim, 16, lab) -> mmx_step(sim, drec->actions[t], 4) over t = 0 .. n_env_steps - 1 gives from the
 * same starting state, and expert_action[t] is that loop's lab; autoreset on the FSM's DONE, truncation and
 * divergence behave as in that loop.
 * n_env_steps == 0 returns MMX_OK; MMX_EINVAL, with nothing launched, for a NULL sim, policy, cfg, drec or
 * drec->actions, n_env_steps < 0, a sim whose action_mode is not MMX_ACTION_ABS_POS, a policy whose action width is
 * not 4, a policy created on another device, beta outside [0, 1] or not finite, takeover_dist < 0 or not finite. */
typedef struct { float beta; float takeover_dist; } mmx_dagger_config;
typedef struct {            /* caller-owned device arrays: float [T][N][4], but gate int32 [T][N], obs_in [T][N][85] */
  float* actions;           /* required: the executed actions */
  float* expert_action;     /* the label: what mmx_expert_plan(16) returns at that state */
  float* policy_action;     /* the learner's action (after noise and clamp) */
  float* mean;              /* as mmx_policy_record */
  float* noise;             /* as mmx_policy_record */
  int32_t* gate;            /* bit 0 Bernoulli, bit 1 takeover; 0: the learner acted */
  float* obs_in;            /* the observation the learner was given at step t (pairs with the label) */
} mmx_dagger_record;
int  mmx_rollout_dagger(mmx_sim* sim, mmx_policy* policy, int32_t n_env_steps, uint64_t call,
                        const mmx_dagger_config* cfg, const mmx_dagger_record* drec, const mmx_trajectory* rec);

/* Batched PNG encoder (dataset emission, generate_dataset.py:250-260: LeRobot embeds image
 * features as PNG files).  Encodes n RGB8 images (device, image i at rgb_dev + i * img_stride,
 * rows of 3 * width bytes, height <= 1024, width <= MMX_PNG_MAX_WIDTH: the encoder's row-above match
 * uses deflate distance 3 * width + 1, capped at 32768) into complete PNG files: image i's file is written at
 * out_dev + i * out_stride (out_stride >= mmx_png_bound(width, height)) and its byte size to
 * sizes_dev[i] (int32).  scratch_dev: n * mmx_png_scratch(width, height) bytes of device memory.
 * mmx_png_pack copies the n files back to back into packed_dev at offsets_dev[i] (int64, device).
 * Asynchronous on the sim's stream; bounds return -1 for unsupported sizes. */
#define MMX_PNG_MAX_WIDTH 10922
int64_t mmx_png_bound(int32_t width, int32_t height);
int64_t mmx_png_scratch(int32_t width, int32_t height);
int mmx_png_encode(mmx_sim* sim, const uint8_t* rgb_dev, int64_t img_stride, int32_t n, int32_t width,
                   int32_t height, uint8_t* out_dev, int64_t out_stride, int32_t* sizes_dev, void* scratch_dev);
int mmx_png_pack(mmx_sim* sim, const uint8_t* out_dev, int64_t out_stride, const int32_t* sizes_dev,
                 const int64_t* offsets_dev, int32_t n, uint8_t* packed_dev);

/* Per-image channel statistics of n RGB8 images (device, image i at rgb_dev + i * img_stride, rows
 * of 3 * width bytes, width and height <= 4096): out_dev[i] = int64 [min R G B, max R G B, sum R G B,
 * sum of squares R G B] over every pixel (LeRobot's image feature statistics, which the dataset
 * writer scales to [0, 1]; generate_dataset.py:250-260).  Asynchronous on the sim's stream. */
int mmx_image_stats(mmx_sim* sim, const uint8_t* rgb_dev, int64_t img_stride, int32_t n, int32_t width,
                    int32_t height, int64_t* out_dev);

/* Physics-level entry points (parity harnesses): n x mujoco.mj_step with the current ctrl
 * (env.py:119-121), optionally preceded by IKController.compute toward the decoded target
 * each substep; and the mj_forward position stage (kinematics + IK cache).  mmx_physics_step
 * runs one launch per substep of the one-substep kernel of the sim's step layout (mmx_step_rows,
 * mmx_tuning.h): the 128-row single-wave kernel, or the 192-row kernel with its helper wave, so a
 * harness checks the very code (row build, solver, overflow rows) that mmx_step runs at that layout. */
int mmx_physics_step(mmx_sim* sim, int32_t n, int32_t with_ik);
int mmx_forward(mmx_sim* sim);

/* Per-physics-step expert loop (main.py:65-91; tests/test_pick_and_place.py:147-166):
 * n x (PickAndPlaceTask.update() = plan(1) + _actuate() (pick_and_place.py:279-304) ;
 * mujoco.mj_step), the FSM reading data.xpos as the previous mj_step left it.  No gym
 * bookkeeping (no reward, observation or autoreset); the FSM state is in episode_i.  This loop
 * exists in the 128-row layout only, whatever mmx_step_rows says. */
int mmx_expert_physics(mmx_sim* sim, int32_t n_physics_steps);

/* Contact forces of every env's current state (the reference: data.contact[i], mujoco.mj_contactForce(model,
 * data, i, out), data.efc_force and data.qacc after env.step(), valid there because step() ends with mj_forward,
 * gym_env.py:560).  mmx_contact_forces runs that forward solve as a pass of its own: kinematics, dynamics,
 * collision, the constraint rows and the Newton solve (cfg.solver_iterations / solver_tolerance, started from
 * qacc_warmstart as a substep's is) on the state in the sim's buffers, without integrating, then MuJoCo's
 * mj_contactForce / mju_decodePyramid: pyramid edge force f_e = -D e on the active edges, fn = the sum of a
 * contact's edge forces, tangent / torsion component k = mu_k (f_k+ - f_k-).  Valid after mmx_reset, mmx_step,
 * any rollout (the final state, the rule for images), mmx_restore and mmx_set_state.  Asynchronous on the sim's
 * stream, ordered with steps and rollouts like any other launch.
 * The outputs are sim-owned device arrays, allocated at the first call (MMX_ENOMEM when that fails) and valid
 * until mmx_destroy:
 *     contact      [N][64][13] fp32   the contacts of the current state in the record of mmx_buffers.contacts
 *                                     (dist, pos3, normal3, mu3, dim, geom1, geom2); zero past ncon
 *     force        [N][64][5] fp32    per contact, same index: fn; the force vector in the world frame ACTING ON
 *                                     GEOM2'S BODY (geom1's body takes the opposite), the normal pointing from
 *                                     geom1 to geom2; the torsional torque about the normal (0 for condim 3);
 *                                     zero past ncon
 *     body_wrench  [N][13][6] fp32    net contact force (3) and torque about the body frame's origin (3), world
 *                                     frame, of the 13 moving bodies in model order: links 2..8, hand 9, fingers
 *                                     10, 11, cubes 16, 17, 18; a body's contacts are added in index order
 *     touch        [N][2] fp32        per finger (body 10, 11): the sum of fn over the contacts between that
 *                                     finger's geoms and any cube (the grip force)
 *     qacc         [N][27] fp32       the solve's acceleration (data.qacc after mj_forward)
 *     solve        [N][6] fp32        ncon; nefc (MuJoCo's count); Newton iterations; relative residual; exit
 *                                     (0 converged, 1 fp32 stall, 2 iteration cap); overflow flags (2: contacts
 *                                     dropped, 4: rows dropped)
 * No floating-point atomics and a fixed order of every sum: the same state gives the same bits on every call.
 * Not touched: every array of mmx_buffers (qacc_warmstart included: mj_forward does not advance it; contacts,
 * stats and episode_i stay those of the last step), the images, and the step kernels' broadphase list and axis
 * cache (the pass works in an overflow block of its own), so a sim continues bit for bit the same whether the
 * pass runs between its steps or not.  Forces are not in a snapshot record: they are derived, and recomputed on
 * demand after mmx_restore.
 * MMX_EINVAL for a NULL argument, and for mmx_get_force_buffers before the first successful
 * mmx_contact_forces (nothing is allocated yet). */
typedef struct {
  int32_t num_envs;
  float* contact;      /* [N][64][13] */
  float* force;        /* [N][64][5] */
  float* body_wrench;  /* [N][13][6] */
  float* touch;        /* [N][2] */
  float* qacc;         /* [N][27] */
  float* solve;        /* [N][6] */
} mmx_force_buffers;
int mmx_contact_forces(mmx_sim* sim);
int mmx_get_force_buffers(mmx_sim* sim, mmx_force_buffers* out);

/* Reward-layer parity harness (gym_env.py:341-470, 562-573).  For every env: the object at
 * obj_dev[N][3], the EE at ee_dev[N][3], gripper ctrl ctrl7_dev[N] and this step's contacts as
 * geom-id pairs pairs_dev[N][max_pairs][2] (int32, a negative id ends the list; geom ids as in the
 * compiled model = MuJoCo's).  Evaluates _compute_reward, updating the sticky flags and
 * high-water marks like a step, and writes reward, reward_components, done[0] (terminated) and
 * done[2] (success).  All pointers are device pointers. */
int mmx_eval_reward(mmx_sim* sim, const float* obj_dev, const float* ee_dev, const float* ctrl7_dev,
                    const int32_t* pairs_dev, int32_t max_pairs);

/* Opt-in camera effects (off by default: the images are then exactly what they were without this
 * call).  MMX_RENDER_SHADOWS: the scene's directional light (dir 0 0 -1, castshadow) casts shadows: a
 * surface point loses the light's term where an opaque, non-floor surface lies above it (a per-env
 * height map, 130 KB per env, allocated at the first call that asks for it).  MMX_RENDER_TRANSLUCENT:
 * the three bins are blended at their material alpha 0.4 over what lies behind them, every layer.
 * Segment ids do not change.  mmx_set_render_effects takes a mask of the flags and takes effect from
 * the next render (reset / step / forward / rollout); it does not render by itself.  MMX_EINVAL for
 * unknown bits or a sim without cameras (image_size == 0); MMX_ENOMEM when the map cannot be
 * allocated (the previous flags stay).  mmx_get_render_effects returns the mask (0 for a NULL sim). */
enum { MMX_RENDER_SHADOWS = 1, MMX_RENDER_TRANSLUCENT = 2 };
int mmx_set_render_effects(mmx_sim* sim, int32_t flags);
int mmx_get_render_effects(const mmx_sim* sim);

int mmx_get_buffers(mmx_sim* sim, mmx_buffers* out);
/* Waits for the sim's stream; MMX_ESAMPLING when an autoreset since the last check (mmx_reset or
 * mmx_synchronize) exhausted its spawn sampling (that env's env_error has bit 8). */
int mmx_synchronize(mmx_sim* sim);

/* Host copies of the core state (host arrays of [N][field] fp32). NULL skips a field. */
int mmx_get_state(mmx_sim* sim, float* qpos, float* qvel, float* ctrl, float* qacc_warmstart);
int mmx_set_state(mmx_sim* sim, const float* qpos, const float* qvel, const float* ctrl, const float* qacc_warmstart);

/* Device-side episode queue of dataset generation (scripts/generate_dataset.py:140-198 runs
 * run_episode per episode with seeds / tasks from :263-277): n_episodes episodes stream through the
 * N env slots with no host synchronisation per step.  mmx_queue_init uploads every episode's task
 * (host, n_episodes entries of obj << 4 | bin, -1 = the env's own draw) and, when seeds (host,
 * n_episodes entries) is non-NULL, its PCG64(SeedSequence(seed)) state; no slot holds an episode
 * yet (synchronous; replaces a previous queue).  mmx_queue_advance, asynchronous on the sim's
 * stream: every slot that holds no episode or whose episode's FSM reached DONE takes the next
 * episode, in ascending slot order, and is reset (PickPlaceGymEnv.reset with the episode's seed
 * and task, gym_env.py:477-534) and re-rendered; slot_ep_dev (device int32 [N], may be NULL)
 * receives each slot's episode afterwards (-1: none left) and fin_ep_dev (device int32 [N], may be
 * NULL) the episode that ended in the slot at this call (-1: none).  MMX_EINVAL without a queue. */
int mmx_queue_init(mmx_sim* sim, int32_t n_episodes, const uint64_t* seeds, const int32_t* tasks);
int mmx_queue_advance(mmx_sim* sim, int32_t* slot_ep_dev, int32_t* fin_ep_dev);

/* Host helper: SeedSequence(root).spawn(n)[index].generate_state(1)[0]
 * (scripts/generate_dataset.py:263-268). */
uint32_t mmx_episode_seed(uint64_t root_seed, int32_t index);

/* Measurement and tuning entry points (launch shape, layout, dispatch order, per-launch timing) have
 * no reference counterpart and are declared in mmx_tuning.h; a reference-side binding needs none. */

#ifdef __cplusplus
}
#endif
#endif

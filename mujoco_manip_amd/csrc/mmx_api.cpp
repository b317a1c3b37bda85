// C-ABI implementation (include/mmx_api.h, include/mmx_tuning.h): device allocation, launches.  The kernel
// sources' launchers come from mmx_launch.h; the host-only parts are headers of their own: the seeding
// (mmx_seed.h) and the rollout's launch plan (mmx_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "../../include/mmx_api.h"
#include "../../include/mmx_tuning.h"
#include "mmx_dagger.h"
#include "mmx_launch.h"
#include "mmx_mppi.h"
#include "mmx_pg.h"
#include "mmx_plan.h"
#include "mmx_policy.h"
#include "mmx_policy_fit.h"
#include "mmx_seed.h"
#include "mmx_state.h"

using namespace mmx_host;

struct mmx_sim {
  MMXState S;
  mmx_config cfg;
  hipStream_t stream;
  std::string err;
  std::vector<void*> allocs;
  // a dalloc of this sim has failed: read by mmx_create alone, once, after its allocations (later callers of
  // dalloc, mmx_queue_init and mmx_set_render_effects, test the pointer they get; the flag then only stays set)
  bool alloc_failed = false;
  float* expert_action;  // [N][4]
  unsigned char* d_mask;
  int* d_task;
  int* d_order;  // [N] dispatch order of the rollout's step launches (MMX_STEP_ORDER)
  // Multi-step rollouts split the envs into `nlanes` independent ranges, each stepped on its own
  // stream (lane 0 = the caller's stream): the ranges never wait for each other between steps,
  // so one range's last-wave tail overlaps the next step of the others (at most kMaxLanes, mmx_plan.h).
  int nlanes = 1;
  // cap on the env steps per mmx_env_step_kernel launch in expert rollouts without cameras (MMX_FUSE
  // overrides): with the staggered lanes 32 beat 16 by 0.5 % and 8 lost 2.7 % on 512-step C3 windows
  // (profiles/r06_sweep_launch_shape.json)
  int fuse = 32;
  // constraint rows the env-step kernel keeps in LDS: 128 (twelve envs per CU) or 192 (four per CU, each
  // with a helper wave, mmx_step_l192.hip: faster when the batch leaves CU slots empty); chosen at create
  // from the batch size, mmx_set_step_rows / MMX_STEP_ROWS override
  int step_rows = 128;
  // env steps launched longest first (mmx_order_kernel; mmx_set_step_order, MMX_STEP_ORDER=0 at
  // create turns it off): the launch's order only, never its results
  int step_order = 1;
  // time-budgeted launches of mmx_rollout_expert (128 rows, no cameras, lanes of at least 6 launches:
  // rollout_bounds, mmx_plan.h; mmx_set_rollout_budget, MMX_ROLLOUT_BUDGET=0 at create turns it off): how an
  // env's steps fall into launches only, never its results.  d_done [N] = the envs' step counts of the
  // current call, d_acc [kMaxLanes][3][2] = each lane's steps and clock ticks per launch (MMXBudget),
  // d_log [log_launches][N] = the counts after each launch of a lane (MMX_ROLLOUT_LOG=launches at create:
  // tests, diagnostics)
  int budget = 1;
  int* d_done = nullptr;
  unsigned long long* d_acc = nullptr;
  int* d_log = nullptr;
  int log_launches = 0;
  hipStream_t lane[kMaxLanes] = {};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxLanes] = {};
  // camera rollouts render step k on their own stream beside step k + 1 (MMX_RENDER_OVERLAP=0 at
  // create: serial): the body poses alternate between S.rpose and rpose_alt; ev_step = the step
  // launch done, ev_rend[k & 1] = render k done
  int render_overlap = 0;
  float* rpose_alt = nullptr;
  hipStream_t rstream = nullptr;
  hipEvent_t ev_step = nullptr, ev_rend[2] = {};
  // opt-in render effects (mmx_set_render_effects): the flags and the per-env shadow height maps
  // (allocated when shadows are first asked for), passed to every render launch (render() below)
  int render_effects = 0;
  unsigned short* shmap = nullptr;
  // the contact-force pass's outputs and its own overflow block (mmx_contact_forces allocates them at its first
  // call, one block; force.contact == nullptr: not yet)
  MMXForce force = {};
  // per-launch kernel timing (mmx_kernel_timing): an event pair around every step / render launch
  // on the stream it runs on; pairs come from a pool reused after each read-out
  bool timing = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<std::pair<size_t, size_t>> t_step, t_render;
  // device-side episode queue (mmx_queue_init / mmx_queue_advance): per-slot episode, next episode,
  // and the episodes' tasks / PCG64 states; q_n < 0: no queue
  int* q_slot = nullptr;
  int* q_next = nullptr;
  int* q_task = nullptr;
  unsigned long long* q_rng = nullptr;
  int q_n = -1;
  // mmx_gae's normalisation: the mean and the denominator (two floats, allocated at the first normalised call)
  float* pg_moments = nullptr;
};

// A planner bound to its (camera-less) planner sim: the launch parameters, its device arrays (its own
// allocations, freed by mmx_mppi_destroy), the branch's src array (i -> i / K) and the call counter
struct mmx_mppi {
  mmx_sim* sim = nullptr;
  int device = 0;  // the sim's (kept for mmx_mppi_destroy)
  MppiParams P{};
  MppiBufs B{};
  float* box = nullptr;  // [3][MMX_MPPI_MAX_ADIM] sigma, low, high
  int* src = nullptr;    // [N]
  uint64_t call = 0;
  std::vector<void*> allocs;
};

// An MLP policy on the device of the sim it was created with: the launch parameters and its one device
// allocation (the packed weights and vectors, mmx_policy.h), freed by mmx_policy_destroy
struct mmx_policy {
  mmx_sim* sim = nullptr;
  int device = 0;  // the sim's (kept for mmx_policy_destroy and mmx_rollout_policy's check)
  MmxPolicy P{};
  float* data = nullptr;
  // mmx_policy_fit's state, allocated at the first fit: the optimiser's m and v (indexed like the blob's layers),
  // its step counter t (0: no step yet), and the workspace of a batch of up to fit_batch samples
  float* fit_m = nullptr;
  float* fit_v = nullptr;
  float* fit_ws = nullptr;
  int fit_batch = 0;
  uint64_t fit_t = 0;
  // the blob's std entries as the host last wrote them (mmx_policy_create, mmx_policy_set_log_std): what
  // mmx_policy_fit_pg asks for a stochastic policy without reading the device
  float std_host[MMX_MPPI_MAX_ADIM] = {};
};

namespace {

// Makes the sim's device current for the duration of an entry point (NULL-stream launches and
// hipMemcpy go to the current device) and restores the caller's device afterwards.  From the device number
// alone for the planner's and the policy's destroy, which may outlive their sim (a device < 0, as for no sim: no switch).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) {
      if (hipSetDevice(device) != hipSuccess) prev = -1;
    } else {
      prev = -1;
    }
  }
  explicit DeviceGuard(const mmx_sim* sim) : DeviceGuard(sim ? sim->cfg.device : -1) {}
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int fail(mmx_sim* sim, int code, const std::string& msg) {
  if (sim) sim->err = msg;
  return code;
}
int hip_check(mmx_sim* sim, hipError_t e, const char* what) {
  if (e == hipSuccess) return MMX_OK;
  return fail(sim, MMX_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
// After a stream synchronisation: the sim's fault word (ERR_SAMPLING of a reset since the last check,
// set by the reset kernel or a step's autoreset) is read, cleared and returned as MMX_ESAMPLING with
// the message randomization.py:84-87 raises.
int check_fault(mmx_sim* sim, const char* what) {
  int f = 0;
  if (hipMemcpy(&f, sim->S.fault, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(sim, MMX_EDEVICE, std::string(what) + ": fault readback");
  if (!(f & ERR_SAMPLING)) return MMX_OK;
  if (hipMemset(sim->S.fault, 0, sizeof(int)) != hipSuccess) return fail(sim, MMX_EDEVICE, std::string(what) + ": fault clear");
  return fail(sim, MMX_ESAMPLING, "Failed to sample 3 positions with min_separation=0.08 in 1000 attempts");
}

template <typename T>
T* dalloc(mmx_sim* sim, size_t count) {
  void* p = nullptr;
  if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) p = nullptr;
  if (p && hipMemset(p, 0, count * sizeof(T)) != hipSuccess) {
    (void)hipFree(p);
    p = nullptr;
  }
  if (p)
    sim->allocs.push_back(p);
  else
    sim->alloc_failed = true;
  return static_cast<T*>(p);
}
// the render of envs [base, base + count) of `S` (the sim's state, or the overlap branch's copy of it with
// the other pose buffer) with the sim's effects; mask: device bytes, null = every env
hipError_t render(const mmx_sim* sim, const MMXState& S, int base, int count, const unsigned char* mask, hipStream_t st) {
  return mmx_launch_render(&S, base, count, mask, sim->render_effects, sim->shmap, st);
}
// a task code of mmx_reset's task_override / mmx_queue_init's tasks: negative (none) or obj << 4 | bin
bool task_code_ok(int t) { return t < 0 || ((t >> 4) <= 2 && (t & 15) <= 2); }

}  // namespace

namespace {
static constexpr size_t kTimingPoolPresize = 2048;
// an event of the timing pool recorded on `st` (its index), or SIZE_MAX when the pool cannot grow
size_t timing_mark(mmx_sim* sim, hipStream_t st) {
  if (sim->ev_used == sim->ev_pool.size()) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return SIZE_MAX;
    sim->ev_pool.push_back(ev);
  }
  const size_t k = sim->ev_used;
  if (hipEventRecord(sim->ev_pool[k], st) != hipSuccess) return SIZE_MAX;
  sim->ev_used++;
  return k;
}
// launch `f` on `st`, bracketed by a timing event pair when timing is on
template <class F>
hipError_t timed(mmx_sim* sim, hipStream_t st, std::vector<std::pair<size_t, size_t>>& pairs, F f) {
  const size_t a = sim->timing ? timing_mark(sim, st) : SIZE_MAX;
  const hipError_t e = f();
  if (a != SIZE_MAX && e == hipSuccess) {
    const size_t b = timing_mark(sim, st);
    if (b != SIZE_MAX) pairs.emplace_back(a, b);
  }
  return e;
}
}  // namespace

extern "C" {

void mmx_config_default(mmx_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->num_envs = 1;
  c->action_mode = MMX_ACTION_EE_POS_QUAT_G_REL;  // gym_env.py:67
  c->reward_type = MMX_REWARD_DENSE;              // gym_env.py:68
  c->max_episode_steps = 500;                     // constants.py:27
  c->spawn_x_range[0] = -0.20;
  c->spawn_x_range[1] = 0.20;
  c->spawn_y_range[0] = 0.30;
  c->spawn_y_range[1] = 0.45;
  c->n_tasks = 9;  // "all" (constants.py:19)
  for (int k = 0; k < 9; k++) {
    c->task_obj[k] = static_cast<int8_t>(k / 3);
    c->task_bin[k] = static_cast<int8_t>(k % 3);
  }
  c->fixed_task_obj = -1;
  c->fixed_task_bin = -1;
  c->image_size = 224;  // constants.py:23
  c->solver_iterations = 30;
  c->solver_tolerance = 1e-6f;
}

int mmx_create(const mmx_config* cfg, mmx_sim** out) {
  if (!cfg || !out) return MMX_EINVAL;
  *out = nullptr;
  if (cfg->image_size < 0 || cfg->image_size > 1024) return MMX_EINVAL;
  if (cfg->num_envs <= 0 || cfg->action_mode < 0 || cfg->action_mode > 4 || cfg->reward_type < 0 ||
      cfg->reward_type > 2 || cfg->n_tasks < 1 || cfg->n_tasks > 9)
    return MMX_EINVAL;
  for (int k = 0; k < cfg->n_tasks; k++)
    if (cfg->task_obj[k] < 0 || cfg->task_obj[k] > 2 || cfg->task_bin[k] < 0 || cfg->task_bin[k] > 2) return MMX_EINVAL;
  mmx_sim* sim = new mmx_sim();
  sim->cfg = *cfg;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
    delete sim;
    return MMX_EDEVICE;
  }
  DeviceGuard guard(sim);  // allocations and streams on cfg->device; the caller's device restored
  sim->stream = static_cast<hipStream_t>(cfg->stream);
  const int N = cfg->num_envs;
  MMXState& S = sim->S;
  std::memset(&S, 0, sizeof(S));
  S.N = N;
  S.action_mode = cfg->action_mode;
  S.reward_type = cfg->reward_type;
  S.max_episode_steps = cfg->max_episode_steps;
  S.randomize = cfg->randomize_objects;
  S.image_size = cfg->image_size;
  S.autoreset = cfg->autoreset;
  S.spawn_x0 = cfg->spawn_x_range[0];
  S.spawn_x1 = cfg->spawn_x_range[1];
  S.spawn_y0 = cfg->spawn_y_range[0];
  S.spawn_y1 = cfg->spawn_y_range[1];
  S.ntask = cfg->n_tasks;
  for (int k = 0; k < 9; k++) {
    S.task_obj[k] = k < cfg->n_tasks ? cfg->task_obj[k] : 0;
    S.task_bin[k] = k < cfg->n_tasks ? cfg->task_bin[k] : 0;
  }
  S.fixed_obj = cfg->fixed_task_obj;
  S.fixed_bin = cfg->fixed_task_bin;
  S.solver = MMX_SOLVER_NEWTON;
  S.solver_max_iter = cfg->solver_iterations > 0 ? cfg->solver_iterations : 30;
  S.solver_tol = cfg->solver_tolerance > 0 ? cfg->solver_tolerance : 1e-6f;
  const size_t n = static_cast<size_t>(N);
  S.qpos = dalloc<float>(sim, MMX_NQ_ * n);
  S.qvel = dalloc<float>(sim, MMX_NV_ * n);
  S.ctrl = dalloc<float>(sim, MMX_NU_ * n);
  S.qacc_ws = dalloc<float>(sim, MMX_NV_ * n);
  S.kin = dalloc<float>(sim, KIN_N * n);
  S.target = dalloc<float>(sim, 4 * n);
  S.epi = dalloc<int>(sim, EPI_N * n);
  S.epf = dalloc<float>(sim, EPF_N * n);
  S.rng = dalloc<unsigned long long>(sim, 4 * n);
  S.rng32 = dalloc<unsigned int>(sim, n);
  S.obs = dalloc<float>(sim, MMX_NOBS * n);
  S.reward = dalloc<float>(sim, n);
  S.reward_components = dalloc<float>(sim, 6 * n);
  S.done = dalloc<int>(sim, 3 * n);
  S.con = dalloc<float>(sim, static_cast<size_t>(MMX_MAXCON) * CON_F * n);
  S.stats = dalloc<float>(sim, STAT_N * n);
  // (zeroed, as every dalloc: the axis cache's entries in it start empty, mmx_gjk_cache.h)
  S.efc_ovf = dalloc<float>(sim, static_cast<size_t>(MMX_OVF_F) * n);
  S.fault = dalloc<int>(sim, 1);
  sim->expert_action = dalloc<float>(sim, 4 * n);
  sim->d_mask = dalloc<unsigned char>(sim, n);
  sim->d_task = dalloc<int>(sim, n);
  sim->d_order = dalloc<int>(sim, n);
  sim->d_done = dalloc<int>(sim, n);
  sim->d_acc = dalloc<unsigned long long>(sim, 6 * kMaxLanes);
  if (const char* v = std::getenv("MMX_ROLLOUT_LOG")) sim->log_launches = std::max(0, std::min(std::atoi(v), 1024));
  if (sim->log_launches) sim->d_log = dalloc<int>(sim, n * sim->log_launches);
  if (cfg->image_size > 0) {  // camera renderer (mmx_render.hip): poses + RGB + segment ids
    const size_t px = static_cast<size_t>(cfg->image_size) * cfg->image_size;
    S.rpose = dalloc<float>(sim, 14 * 12 * n);
    sim->rpose_alt = dalloc<float>(sim, 14 * 12 * n);
    S.images = dalloc<unsigned char>(sim, 2 * px * 3 * n);
    S.seg = dalloc<unsigned char>(sim, 2 * px * n);
    const size_t sg = static_cast<size_t>((cfg->image_size + 15) & ~15);
    S.bg_overhead = dalloc<unsigned int>(sim, sg * sg);
  }
  if (sim->alloc_failed) {  // any of the buffers above
    mmx_destroy(sim);
    return MMX_ENOMEM;
  }
  // gymnasium's lazily created np_random uses OS entropy when never seeded
  std::random_device rd;
  std::vector<unsigned long long> rng(4 * n);
  for (size_t i = 0; i < n; i++) pcg64_seed_row(&rng[4 * i], (static_cast<uint64_t>(rd()) << 32) ^ rd());
  if (hipMemcpy(S.rng, rng.data(), rng.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(sim->d_done, 0, n * sizeof(int)) != hipSuccess ||
      (sim->d_log && hipMemset(sim->d_log, 0, n * sim->log_launches * sizeof(int)) != hipSuccess)) {  // (no budgeted call yet: mmx_rollout_step_counts)
    mmx_destroy(sim);
    return MMX_EDEVICE;
  }
  // rollout lanes: MMX_STREAMS overrides; by default one lane per 1024 envs, at most 4 (the
  // process's hardware queues: more lanes multiplex onto them and gain nothing, C5 8 vs 4 lanes
  // -0.8 %), at most kMaxLanes
  int lanes = std::min(N / 1024, 4);
  if (const char* v = std::getenv("MMX_STREAMS")) lanes = std::atoi(v);
  if (const char* v = std::getenv("MMX_FUSE")) sim->fuse = std::max(1, std::atoi(v));
  // the layout: 192 rows (one env wave + its helper wave, four envs per CU) while the batch fits the
  // chip at four per CU, where each env's own speed counts (C2's 1024 envs: 1.52 M vs 1.29 M env
  // steps/s); 128 rows (twelve per CU) for larger batches, where slots count
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess) cus = 0;
  sim->step_rows = cus > 0 && N <= 4 * cus ? 192 : 128;
  if (const char* v = std::getenv("MMX_STEP_ROWS")) {
    const int r = std::atoi(v);
    if (r == 128 || r == 192) sim->step_rows = r;
  }
  sim->step_order = 1;
  if (const char* v = std::getenv("MMX_STEP_ORDER")) sim->step_order = std::atoi(v) != 0;
  if (const char* v = std::getenv("MMX_ROLLOUT_BUDGET")) sim->budget = std::atoi(v) != 0;
  lanes = std::max(1, std::min(lanes, std::min(N, int(kMaxLanes))));
  if (hipEventCreateWithFlags(&sim->ev_fork, hipEventDisableTiming) != hipSuccess) lanes = 1;
  for (int l = 1; l < lanes; l++)
    if (hipStreamCreateWithFlags(&sim->lane[l], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&sim->ev_join[l], hipEventDisableTiming) != hipSuccess) {
      if (sim->lane[l]) (void)hipStreamDestroy(sim->lane[l]);
      lanes = l;
      break;
    }
  sim->nlanes = lanes;
  sim->render_overlap = sim->rpose_alt != nullptr;
  if (const char* v = std::getenv("MMX_RENDER_OVERLAP")) sim->render_overlap = sim->render_overlap && std::atoi(v) != 0;
  if (sim->render_overlap && (hipStreamCreateWithFlags(&sim->rstream, hipStreamNonBlocking) != hipSuccess ||
                              hipEventCreateWithFlags(&sim->ev_step, hipEventDisableTiming) != hipSuccess ||
                              hipEventCreateWithFlags(&sim->ev_rend[0], hipEventDisableTiming) != hipSuccess ||
                              hipEventCreateWithFlags(&sim->ev_rend[1], hipEventDisableTiming) != hipSuccess))
    sim->render_overlap = 0;
  // the fixed overhead camera's background, once; the handle is published only when the sim is
  // complete (on a failure every allocation is released and *out stays null)
  int rc = S.bg_overhead ? hip_check(sim, mmx_launch_render_bg(&S, sim->stream), "mmx_create background") : 0;
  if (!rc) rc = hip_check(sim, hipDeviceSynchronize(), "mmx_create");
  if (rc) {
    mmx_destroy(sim);
    return rc;
  }
  *out = sim;
  return 0;
}

void mmx_destroy(mmx_sim* sim) {
  if (!sim) return;
  DeviceGuard guard(sim);
  (void)hipDeviceSynchronize();
  for (void* p : sim->allocs)
    if (p) (void)hipFree(p);
  for (int l = 1; l < sim->nlanes; l++) {
    (void)hipEventDestroy(sim->ev_join[l]);
    (void)hipStreamDestroy(sim->lane[l]);
  }
  if (sim->ev_fork) (void)hipEventDestroy(sim->ev_fork);
  for (hipEvent_t ev : {sim->ev_step, sim->ev_rend[0], sim->ev_rend[1]})
    if (ev) (void)hipEventDestroy(ev);
  if (sim->rstream) (void)hipStreamDestroy(sim->rstream);
  for (hipEvent_t ev : sim->ev_pool) (void)hipEventDestroy(ev);
  delete sim;
}

const char* mmx_last_error(const mmx_sim* sim) { return sim ? sim->err.c_str() : "null sim"; }

int mmx_reset(mmx_sim* sim, const uint64_t* seeds, const uint8_t* seed_given, const int32_t* task_override,
              const uint8_t* env_mask) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  MMXState& S = sim->S;
  const size_t n = static_cast<size_t>(S.N);
  if (seeds) {
    // re-seed selected envs: PCG64(SeedSequence(seed)); the 32-bit buffer is cleared
    std::vector<unsigned long long> rng(4 * n);
    if (hipStreamSynchronize(sim->stream) != hipSuccess) return fail(sim, MMX_EDEVICE, "mmx_reset sync");
    if (hipMemcpy(rng.data(), S.rng, rng.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
      return fail(sim, MMX_EDEVICE, "rng readback");
    std::vector<int> epi(EPI_N * n);
    if (hipMemcpy(epi.data(), S.epi, epi.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      return fail(sim, MMX_EDEVICE, "epi readback");
    for (size_t i = 0; i < n; i++) {
      if (env_mask && !env_mask[i]) continue;
      if (seed_given && !seed_given[i]) continue;
      pcg64_seed_row(&rng[4 * i], seeds[i]);
      epi[EPI_N * i + EPI_RNG_HAS32] = 0;
    }
    if (hipMemcpy(S.rng, rng.data(), rng.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(S.epi, epi.data(), epi.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      return fail(sim, MMX_EDEVICE, "rng upload");
  }
  const unsigned char* dmask = nullptr;
  const int* dtask = nullptr;
  if (env_mask) {
    if (hipMemcpyAsync(sim->d_mask, env_mask, n, hipMemcpyHostToDevice, sim->stream) != hipSuccess)
      return fail(sim, MMX_EDEVICE, "mask upload");
    dmask = sim->d_mask;
  }
  if (task_override) {
    for (size_t i = 0; i < n; i++)
      if (!task_code_ok(task_override[i])) return fail(sim, MMX_EINVAL, "task_override out of range");
    if (hipMemcpyAsync(sim->d_task, task_override, n * sizeof(int), hipMemcpyHostToDevice, sim->stream) != hipSuccess)
      return fail(sim, MMX_EDEVICE, "task upload");
    dtask = sim->d_task;
  }
  int rc = hip_check(sim, mmx_launch_reset(&S, dmask, dtask, sim->stream), "mmx_reset");
  if (rc) return rc;
  rc = hip_check(sim, render(sim, S, 0, S.N, nullptr, sim->stream), "mmx_reset render");
  if (rc) return rc;
  rc = hip_check(sim, hipStreamSynchronize(sim->stream), "mmx_reset sync");
  return rc ? rc : check_fault(sim, "mmx_reset");
}

namespace {
// the step kernels' launchers of the sim's LDS-row layout (mmx_step.inc is built at 128 and at 192 rows):
// the one place the layout is chosen, for mmx_step, the rollouts and mmx_physics_step
struct StepLaunchers {
  decltype(&mmx_launch_step) step;
  decltype(&mmx_launch_traj) traj;
  decltype(&mmx_launch_physics) physics;
  decltype(&mmx_launch_policy) policy;
  decltype(&mmx_launch_dagger) dagger;
};
StepLaunchers step_launchers(const mmx_sim* sim) {
  return sim->step_rows == 192 ? StepLaunchers{mmx_launch_step_l192, mmx_launch_traj_l192, mmx_launch_physics_l192, mmx_launch_policy_l192,
                                               mmx_launch_dagger_l192}
                               : StepLaunchers{mmx_launch_step, mmx_launch_traj, mmx_launch_physics, mmx_launch_policy,
                                               mmx_launch_dagger};
}
// floats per env that each action mode's action needs
constexpr int kDim[5] = {4, 8, 10, 8, 10};
}  // namespace

int mmx_set_step_rows(mmx_sim* sim, int32_t rows) {
  if (!sim || (rows != 128 && rows != 192)) return MMX_EINVAL;
  sim->step_rows = rows;
  return MMX_OK;
}
int mmx_step_rows(const mmx_sim* sim) { return sim ? sim->step_rows : 0; }
int mmx_set_step_order(mmx_sim* sim, int32_t on) {
  if (!sim || (on != 0 && on != 1)) return MMX_EINVAL;
  sim->step_order = on;
  return MMX_OK;
}
int mmx_step_order(const mmx_sim* sim) { return sim ? sim->step_order : -1; }
int mmx_set_rollout_budget(mmx_sim* sim, int32_t on) {
  if (!sim || (on != 0 && on != 1)) return MMX_EINVAL;
  sim->budget = on;
  return MMX_OK;
}
int mmx_rollout_budget(const mmx_sim* sim) { return sim ? sim->budget : -1; }
int mmx_rollout_step_counts(mmx_sim* sim, int32_t* out, int32_t* log, int32_t log_launches) {
  if (!sim || (!out && !log) || (log && log_launches != sim->log_launches))
    return sim ? fail(sim, MMX_EINVAL, "mmx_rollout_step_counts: bad arguments") : MMX_EINVAL;
  DeviceGuard guard(sim);
  const size_t n = static_cast<size_t>(sim->S.N);
  hipError_t e = hipStreamSynchronize(sim->stream);
  if (e == hipSuccess && out) e = hipMemcpy(out, sim->d_done, n * sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess && log && log_launches) e = hipMemcpy(log, sim->d_log, n * log_launches * sizeof(int), hipMemcpyDeviceToHost);
  return hip_check(sim, e, "mmx_rollout_step_counts");
}

int mmx_step(mmx_sim* sim, const float* action_dev, int32_t action_dim) {
  if (!sim || !action_dev) return MMX_EINVAL;
  DeviceGuard guard(sim);
  if (action_dim < kDim[sim->S.action_mode]) return fail(sim, MMX_EINVAL, "action_dim too small for action_mode");
  // longest first by FSM phase (the expert's plan keeps it current; with policy actions it stays idle
  // and the order is index order up to ties)
  int* ord = sim->step_order ? sim->d_order : nullptr;
  hipError_t e = ord ? mmx_launch_order(&sim->S, 0, sim->S.N, ord, 1024, sim->stream) : hipSuccess;
  if (e == hipSuccess) e = step_launchers(sim).step(&sim->S, action_dev, action_dim, 0, 0, sim->S.N, 1, sim->stream, ord);
  if (e == hipSuccess) e = render(sim, sim->S, 0, sim->S.N, nullptr, sim->stream);
  return hip_check(sim, e, "mmx_step");
}

int mmx_expert_plan(mmx_sim* sim, int32_t n_steps, float* action_dev_out) {
  if (!sim || n_steps < 0) return MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, mmx_launch_expert(&sim->S, n_steps, action_dev_out, sim->stream), "mmx_expert_plan");
}


int mmx_kernel_timing(mmx_sim* sim, int32_t enable) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  if (enable) {  // start a new collection (the pool's events are reused)
    sim->ev_used = 0;
    sim->t_step.clear();
    sim->t_render.clear();
    // pre-size the pool, so no hipEventCreate runs between the launches of a timed window (2 events
    // per launch: a C5 window of 128 env steps on 4 lanes records 2048)
    while (sim->ev_pool.size() < kTimingPoolPresize) {
      hipEvent_t ev;
      if (hipEventCreate(&ev) != hipSuccess) break;
      sim->ev_pool.push_back(ev);
    }
  }
  sim->timing = enable != 0;
  return MMX_OK;
}

int mmx_kernel_times(mmx_sim* sim, float* step_ms, int32_t* step_launches, float* render_ms, int32_t* render_launches) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  auto sum = [&](const std::vector<std::pair<size_t, size_t>>& v, float* ms, int32_t* n) -> hipError_t {
    double tot = 0.0;
    for (const auto& pr : v) {
      hipError_t e = hipEventSynchronize(sim->ev_pool[pr.second]);
      float t = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&t, sim->ev_pool[pr.first], sim->ev_pool[pr.second]);
      if (e != hipSuccess) return e;
      tot += t;
    }
    if (ms) *ms = (float)tot;
    if (n) *n = (int32_t)v.size();
    return hipSuccess;
  };
  hipError_t e = sum(sim->t_step, step_ms, step_launches);
  if (e == hipSuccess) e = sum(sim->t_render, render_ms, render_launches);
  return hip_check(sim, e, "mmx_kernel_times");
}

// The rollout's launch plan (mmx_plan.h) with the sim's lanes, fuse cap and cameras; MMX_PLAN overrides it
static int rollout_lanes(const mmx_sim* sim) { return rollout_lanes(sim->nlanes, sim->S.image_size > 0); }
static RolloutPlan rollout_plan(const mmx_sim* sim, int n) {
  return rollout_plan(n, sim->nlanes, sim->fuse, sim->S.image_size > 0, std::getenv("MMX_PLAN"));
}
int mmx_rollout_launches(const mmx_sim* sim, int32_t n_env_steps) {
  return sim ? (int)rollout_plan(sim, n_env_steps).rounds : 0;
}
// The rollout's choreography, once, for both step kernels: `launch(S, base, count, nsteps, k0, st, order, B)`
// launches `nsteps` env steps of envs [base, base + count) on `st`, k0 = the rollout step that lane has
// reached (the trajectory kernel's action rows and record slices; the step kernel ignores it).  `what`
// names the entry point in the error text.  (A template, not std::function: the launch is inlined.)
// `budgeted` (mmx_rollout_expert on the 128-row kernel alone): when a lane makes enough launches
// (rollout_bounds), every launch of the call gets B, its bounds on the envs' step counts and the lane's
// step-time sums, in place of nsteps (null otherwise: the fixed count).
extern "C++" {
template <class Launch>
static int rollout(mmx_sim* sim, int n, const char* what, bool budgeted, Launch launch) {
  if (n <= 0) return MMX_OK;
  DeviceGuard guard(sim);
  const int N = sim->S.N;
  hipError_t e = hipSuccess;
  if (sim->render_overlap && sim->S.image_size > 0 && n > 1) {
    // the render of step k on its own stream beside the step k + 1 on the caller's stream (a render
    // workgroup's 80 KB of LDS fits a CU the step launch's tail has half emptied: C5 +6.6 %, DESIGN
    // §8 f1); step k writes the pose buffer render k - 2 read, so it waits for that render only
    hipStream_t rs = sim->rstream;
    float* rp[2] = {sim->S.rpose, sim->rpose_alt};
    for (int k = 0; k < n && e == hipSuccess; k++) {
      MMXState Sk = sim->S;
      Sk.rpose = rp[k & 1];
      if (k >= 2) e = hipStreamWaitEvent(sim->stream, sim->ev_rend[k & 1], 0);
      int* ord = sim->step_order ? sim->d_order : nullptr;
      if (e == hipSuccess && ord) e = mmx_launch_order(&Sk, 0, N, ord, 1024, sim->stream);
      if (e == hipSuccess)
        e = timed(sim, sim->stream, sim->t_step, [&] { return launch(&Sk, 0, N, 1, k, sim->stream, ord, nullptr); });
      if (e == hipSuccess) e = hipEventRecord(sim->ev_step, sim->stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(rs, sim->ev_step, 0);
      if (e == hipSuccess) e = timed(sim, rs, sim->t_render, [&] { return render(sim, Sk, 0, N, nullptr, rs); });
      if (e == hipSuccess) e = hipEventRecord(sim->ev_rend[k & 1], rs);
    }
    // the caller's stream sees the last render; S.rpose names the newest poses
    if (e == hipSuccess) e = hipStreamWaitEvent(sim->stream, sim->ev_rend[(n - 1) & 1], 0);
    if (e == hipSuccess && ((n - 1) & 1)) std::swap(sim->S.rpose, sim->rpose_alt);
    return hip_check(sim, e, what);
  }
  // step k of range l only depends on step k-1 of range l.  Without cameras a launch runs up to `fuse`
  // consecutive steps of its envs (mmx_rollout_steps_per_launch); with cameras every step is rendered,
  // one step per launch.
  const RolloutPlan P = rollout_plan(sim, n);
  const int L = P.lanes;
  // the launches' bounds; the counts and the lanes' sums start at zero before the fork (no host wait anywhere:
  // a lane's launch reads the sums its earlier launches added, ordered by the lane's stream)
  LaunchBounds bounds[kMaxLanes];
  budgeted = budgeted && sim->budget && sim->S.image_size == 0;
  bool use_budget = false;
  for (int l = 0; l < L && budgeted; l++) {
    bounds[l] = rollout_bounds(P.len[l], rollout_len(n, sim->fuse, false), true);
    for (size_t r = 0; r < P.len[l].size(); r++) use_budget = use_budget || bounds[l].lo[r] < bounds[l].hi[r];
  }
  if (use_budget) {
    e = hipMemsetAsync(sim->d_done, 0, sizeof(int) * N, sim->stream);
    if (e == hipSuccess) e = hipMemsetAsync(sim->d_acc, 0, sizeof(unsigned long long) * 6 * kMaxLanes, sim->stream);
    if (e == hipSuccess && sim->d_log) e = hipMemsetAsync(sim->d_log, 0, sizeof(int) * N * sim->log_launches, sim->stream);
    if (e != hipSuccess) return hip_check(sim, e, what);
  }
  if (L > 1) {  // fork: every lane starts after the work already queued on the caller's stream
    e = hipEventRecord(sim->ev_fork, sim->stream);
    for (int l = 1; l < L && e == hipSuccess; l++) e = hipStreamWaitEvent(sim->lane[l], sim->ev_fork, 0);
  }
  int k0[kMaxLanes] = {};  // the rollout step each lane's next launch starts at
  // with cameras (L = 1): the step of all envs, then ONE render launch over all envs (the render's
  // 80 KB workgroups cannot share a CU with the step kernel's: a render per lane beside the other
  // lanes' steps ran as a trickle, C5 -2.8 %)
  for (size_t r = 0; r < P.rounds && e == hipSuccess; r++) {
    for (int l = 0; l < L && e == hipSuccess; l++) {
      if (r >= P.len[l].size()) continue;
      const int ns = P.len[l][r];
      const int b0 = (int)((long)N * l / L), b1 = (int)((long)N * (l + 1) / L);
      hipStream_t st = l ? sim->lane[l] : sim->stream;
      int* ord = sim->step_order ? sim->d_order + b0 : nullptr;  // the lane's slice of the order buffer
      if (ord) e = mmx_launch_order(&sim->S, b0, b1 - b0, ord, L > 1 ? 64 : 1024, st);
      MMXBudget B{sim->d_done, sim->d_acc + 6 * l, (int)r, nullptr, 0, 0, ns};
      if (use_budget) {
        B.lo = bounds[l].lo[r];
        B.hi = bounds[l].hi[r];
        if (sim->d_log && r < (size_t)sim->log_launches) B.log = sim->d_log + r * (size_t)N;
      }
      if (e == hipSuccess)
        e = timed(sim, st, sim->t_step, [&] { return launch(&sim->S, b0, b1 - b0, ns, k0[l], st, ord, use_budget ? &B : nullptr); });
      k0[l] += ns;
    }
    if (e == hipSuccess && sim->S.image_size > 0)
      e = timed(sim, sim->stream, sim->t_render, [&] { return render(sim, sim->S, 0, N, nullptr, sim->stream); });
  }
  if (L > 1)  // join: the caller's stream sees the whole rollout, as with a single launch chain
    for (int l = 1; l < L; l++) {
      hipError_t j = hipEventRecord(sim->ev_join[l], sim->lane[l]);
      if (j == hipSuccess) j = hipStreamWaitEvent(sim->stream, sim->ev_join[l], 0);
      if (e == hipSuccess) e = j;
    }
  return hip_check(sim, e, what);
}
}  // extern "C++"

// The step kernel plans with the FSM itself (expert = 1) and writes no record.
int mmx_rollout_expert(mmx_sim* sim, int32_t n_env_steps) {
  if (!sim || sim->S.action_mode != MMX_ACTION_ABS_POS) return MMX_EINVAL;
  const auto step = step_launchers(sim).step;
  return rollout(sim, n_env_steps, "mmx_rollout_expert", sim->step_rows == 128,
                 [&](const MMXState* S, int base, int count, int ns, int, hipStream_t st, const int* ord, const MMXBudget* B) {
                   return B ? mmx_launch_step_budget(S, B, sim->expert_action, 4, base, count, st, ord)
                            : step(S, sim->expert_action, 4, 1, base, count, ns, st, ord);
                 });
}

// the caller's record as the kernels take it (no record: every array null, nothing is written)
static MMXTraj traj_arg(const mmx_trajectory* rec) {
  if (!rec) return MMXTraj{};
  return MMXTraj{rec->obs, rec->reward, rec->done, rec->reward_components, rec->target, rec->episode_i, rec->qpos, rec->qvel};
}

// The same rollout on the trajectory kernel: every launch also gets the rollout step k0 its lane has
// reached, which selects its action rows (expert = 0) and its slices of the record `rec`.
static int rollout_traj(mmx_sim* sim, const float* actions, int adim, int expert, int n, const mmx_trajectory* rec,
                        const char* what) {
  const MMXTraj R = traj_arg(rec);
  const auto traj = step_launchers(sim).traj;
  return rollout(sim, n, what, false,
                 [&](const MMXState* S, int base, int count, int ns, int k0, hipStream_t st, const int* ord, const MMXBudget*) {
                   return traj(S, &R, actions, adim, expert, base, count, ns, k0, st, ord);
                 });
}

int mmx_rollout_actions(mmx_sim* sim, const float* actions_dev, int32_t action_dim, int32_t n_env_steps,
                        const mmx_trajectory* rec) {
  if (!sim || !actions_dev || n_env_steps < 0) return sim ? fail(sim, MMX_EINVAL, "mmx_rollout_actions: bad arguments") : MMX_EINVAL;
  if (action_dim < kDim[sim->S.action_mode]) return fail(sim, MMX_EINVAL, "action_dim too small for action_mode");
  return rollout_traj(sim, actions_dev, action_dim, 0, n_env_steps, rec, "mmx_rollout_actions");
}

int mmx_rollout_expert_record(mmx_sim* sim, int32_t n_env_steps, const mmx_trajectory* rec) {
  if (!sim || n_env_steps < 0) return sim ? fail(sim, MMX_EINVAL, "mmx_rollout_expert_record: bad arguments") : MMX_EINVAL;
  if (sim->S.action_mode != MMX_ACTION_ABS_POS) return fail(sim, MMX_EINVAL, "mmx_rollout_expert_record needs action_mode abs_pos");
  return rollout_traj(sim, sim->expert_action, 4, 1, n_env_steps, rec, "mmx_rollout_expert_record");
}

int mmx_rollout_lanes(const mmx_sim* sim) { return sim ? rollout_lanes(sim) : 0; }
int mmx_rollout_render_overlap(const mmx_sim* sim) { return sim ? sim->render_overlap : 0; }
int mmx_rollout_render_launches(const mmx_sim* sim) {
  return sim && sim->S.image_size > 0 ? 1 : 0;
}

// the row-above match uses deflate distance 3 W + 1, which deflate caps at 32768: W <= 10922
static bool png_size_ok(int32_t width, int32_t height) {
  return width > 0 && height > 0 && height <= 1024 && width <= MMX_PNG_MAX_WIDTH;
}
int64_t mmx_png_bound(int32_t width, int32_t height) {
  return png_size_ok(width, height) ? mmx_png_bound_bytes(width, height) : -1;
}
int64_t mmx_png_scratch(int32_t width, int32_t height) {
  return png_size_ok(width, height) ? mmx_png_scratch_bytes(width, height) : -1;
}

int mmx_png_encode(mmx_sim* sim, const uint8_t* rgb_dev, int64_t img_stride, int32_t n, int32_t width, int32_t height,
                   uint8_t* out_dev, int64_t out_stride, int32_t* sizes_dev, void* scratch_dev) {
  if (!sim || n < 0 || (n > 0 && (!rgb_dev || !out_dev || !sizes_dev || !scratch_dev)) || !png_size_ok(width, height) ||
      img_stride < 3LL * width * height || out_stride < mmx_png_bound_bytes(width, height))
    return sim ? fail(sim, MMX_EINVAL, "mmx_png_encode: bad arguments") : MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, mmx_launch_png(rgb_dev, img_stride, n, width, height, out_dev, out_stride, sizes_dev,
                                       static_cast<uint32_t*>(scratch_dev), sim->stream), "mmx_png_encode");
}

int mmx_png_pack(mmx_sim* sim, const uint8_t* out_dev, int64_t out_stride, const int32_t* sizes_dev,
                 const int64_t* offsets_dev, int32_t n, uint8_t* packed_dev) {
  if (!sim || n < 0 || (n > 0 && (!out_dev || !sizes_dev || !offsets_dev || !packed_dev)))
    return sim ? fail(sim, MMX_EINVAL, "mmx_png_pack: bad arguments") : MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, mmx_launch_png_pack(out_dev, out_stride, sizes_dev, offsets_dev, n, packed_dev, sim->stream),
                   "mmx_png_pack");
}

int mmx_image_stats(mmx_sim* sim, const uint8_t* rgb_dev, int64_t img_stride, int32_t n, int32_t width, int32_t height,
                    int64_t* out_dev) {
  if (!sim || n < 0 || (n > 0 && (!rgb_dev || !out_dev)) || width <= 0 || height <= 0 || width > 4096 ||
      height > 4096 || img_stride < 3LL * width * height)
    return sim ? fail(sim, MMX_EINVAL, "mmx_image_stats: bad arguments") : MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, mmx_launch_image_stats(rgb_dev, img_stride, n, (int64_t)width * height, out_dev, sim->stream),
                   "mmx_image_stats");
}

int64_t mmx_copy_ranges(int64_t n, const uint64_t* src, const uint64_t* dst, const int64_t* len) {
  if (n < 0 || (n > 0 && (!src || !dst || !len))) return -1;
  int64_t total = 0;
  for (int64_t k = 0; k < n; k++) {
    if (len[k] < 0) return -1;
    total += len[k];
  }
  for (int64_t k = 0; k < n; k++)
    if (len[k])
      std::memcpy(reinterpret_cast<void*>(static_cast<uintptr_t>(dst[k])),
                  reinterpret_cast<const void*>(static_cast<uintptr_t>(src[k])), (size_t)len[k]);
  return total;
}

int mmx_rollout_steps_per_launch(const mmx_sim* sim) {
  return sim ? (sim->S.image_size > 0 ? 1 : sim->fuse) : 0;
}

int mmx_physics_step(mmx_sim* sim, int32_t n, int32_t with_ik) {
  if (!sim || n < 0) return MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, step_launchers(sim).physics(&sim->S, n, with_ik, sim->stream), "mmx_physics_step");
}

int mmx_expert_physics(mmx_sim* sim, int32_t n) {
  if (!sim || n < 0) return MMX_EINVAL;
  DeviceGuard guard(sim);
  hipError_t e = hipSuccess;
  for (int k = 0; k < n && e == hipSuccess; k += 256)  // bounded launches (a few ms each)
    e = mmx_launch_expert_physics(&sim->S, std::min(256, n - k), sim->stream);
  return hip_check(sim, e, "mmx_expert_physics");
}

int mmx_contact_forces(mmx_sim* sim) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  MMXForce& F = sim->force;
  if (!F.contact) {  // one allocation, zeroed (the pass's axis cache starts empty), carved in 16-byte steps
    const size_t n = static_cast<size_t>(sim->S.N);
    const size_t widths[7] = {size_t(MMX_MAXCON) * CON_F, size_t(MMX_MAXCON) * FRC_F, size_t(FRC_NBODY) * 6, 2, MMX_NV_,
                              FRC_SOLVE_F, MMX_OVF_F};
    size_t at[8] = {0};
    for (int k = 0; k < 7; k++) at[k + 1] = at[k] + (widths[k] * n + 3) / 4 * 4;
    float* base = dalloc<float>(sim, at[7]);
    if (!base) return fail(sim, MMX_ENOMEM, "mmx_contact_forces: output arrays");
    F.force = base + at[1];
    F.wrench = base + at[2];
    F.touch = base + at[3];
    F.qacc = base + at[4];
    F.solve = base + at[5];
    F.ovf = base + at[6];
    F.contact = base;
  }
  return hip_check(sim, mmx_launch_contact_force(&sim->S, &F, sim->stream), "mmx_contact_forces");
}

int mmx_get_force_buffers(mmx_sim* sim, mmx_force_buffers* out) {
  if (!sim || !out) return MMX_EINVAL;
  const MMXForce& F = sim->force;
  if (!F.contact) return fail(sim, MMX_EINVAL, "mmx_get_force_buffers: no mmx_contact_forces call yet (nothing allocated)");
  out->num_envs = sim->S.N;
  out->contact = F.contact;
  out->force = F.force;
  out->body_wrench = F.wrench;
  out->touch = F.touch;
  out->qacc = F.qacc;
  out->solve = F.solve;
  return MMX_OK;
}

int mmx_eval_reward(mmx_sim* sim, const float* obj, const float* ee, const float* ctrl7, const int32_t* pairs,
                    int32_t max_pairs) {
  if (!sim || !obj || !ee || !ctrl7 || max_pairs < 0 || (max_pairs > 0 && !pairs)) return MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, mmx_launch_reward(&sim->S, obj, ee, ctrl7, pairs, max_pairs, sim->stream), "mmx_eval_reward");
}

int mmx_forward(mmx_sim* sim) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  hipError_t e = mmx_launch_forward(&sim->S, sim->stream);
  if (e == hipSuccess) e = render(sim, sim->S, 0, sim->S.N, nullptr, sim->stream);
  return hip_check(sim, e, "mmx_forward");
}

int mmx_set_render_effects(mmx_sim* sim, int32_t flags) {
  if (!sim) return MMX_EINVAL;
  if (flags & ~(MMX_RENDER_SHADOWS | MMX_RENDER_TRANSLUCENT)) return fail(sim, MMX_EINVAL, "mmx_set_render_effects: unknown flag bits");
  if (sim->S.image_size <= 0) return fail(sim, MMX_EINVAL, "mmx_set_render_effects: the sim has no cameras (image_size = 0)");
  DeviceGuard guard(sim);
  if ((flags & MMX_RENDER_SHADOWS) && !sim->shmap) {
    const size_t per_env = mmx_render_shadow_map_bytes() / sizeof(unsigned short);
    sim->shmap = dalloc<unsigned short>(sim, per_env * static_cast<size_t>(sim->S.N));
    if (!sim->shmap) return fail(sim, MMX_ENOMEM, "mmx_set_render_effects: shadow maps");
  }
  sim->render_effects = flags;
  return MMX_OK;
}
int mmx_get_render_effects(const mmx_sim* sim) { return sim ? sim->render_effects : 0; }

int mmx_get_buffers(mmx_sim* sim, mmx_buffers* b) {
  if (!sim || !b) return MMX_EINVAL;
  const MMXState& S = sim->S;
  b->num_envs = S.N;
  b->qpos = S.qpos;
  b->qvel = S.qvel;
  b->ctrl = S.ctrl;
  b->qacc_warmstart = S.qacc_ws;
  b->obs = S.obs;
  b->reward = S.reward;
  b->done = S.done;
  b->reward_components = S.reward_components;
  b->episode_i = S.epi;
  b->episode_f = S.epf;
  b->kin = S.kin;
  b->stats = S.stats;
  b->contacts = S.con;
  b->images = S.images;
  b->seg = S.seg;
  b->target = S.target;
  return MMX_OK;
}

int mmx_synchronize(mmx_sim* sim) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  const int rc = hip_check(sim, hipStreamSynchronize(sim->stream), "mmx_synchronize");
  return rc ? rc : check_fault(sim, "mmx_synchronize");
}

int mmx_get_state(mmx_sim* sim, float* qpos, float* qvel, float* ctrl, float* ws) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  const size_t n = static_cast<size_t>(sim->S.N);
  hipError_t e = hipStreamSynchronize(sim->stream);
  if (e == hipSuccess && qpos) e = hipMemcpy(qpos, sim->S.qpos, MMX_NQ_ * n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && qvel) e = hipMemcpy(qvel, sim->S.qvel, MMX_NV_ * n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && ctrl) e = hipMemcpy(ctrl, sim->S.ctrl, MMX_NU_ * n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && ws) e = hipMemcpy(ws, sim->S.qacc_ws, MMX_NV_ * n * 4, hipMemcpyDeviceToHost);
  return hip_check(sim, e, "mmx_get_state");
}

int mmx_set_state(mmx_sim* sim, const float* qpos, const float* qvel, const float* ctrl, const float* ws) {
  if (!sim) return MMX_EINVAL;
  DeviceGuard guard(sim);
  const size_t n = static_cast<size_t>(sim->S.N);
  hipError_t e = hipStreamSynchronize(sim->stream);
  if (e == hipSuccess && qpos) e = hipMemcpy(sim->S.qpos, qpos, MMX_NQ_ * n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && qvel) e = hipMemcpy(sim->S.qvel, qvel, MMX_NV_ * n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && ctrl) e = hipMemcpy(sim->S.ctrl, ctrl, MMX_NU_ * n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && ws) e = hipMemcpy(sim->S.qacc_ws, ws, MMX_NV_ * n * 4, hipMemcpyHostToDevice);
  return hip_check(sim, e, "mmx_set_state");
}

// Snapshot / restore (mmx_snapshot.hip).  A record's size depends on the cameras only (the body poses).
int64_t mmx_snapshot_bytes(const mmx_sim* sim) { return sim ? mmx_snapshot_record_bytes(sim->S.image_size > 0) : -1; }

static bool snapshot_args_ok(const mmx_sim* sim, const void* blob, int64_t rec_bytes) {
  return sim && blob && reinterpret_cast<uintptr_t>(blob) % 16 == 0 && rec_bytes == mmx_snapshot_bytes(sim);
}

int mmx_snapshot(mmx_sim* sim, void* snap_dev, int64_t rec_bytes) {
  if (!snapshot_args_ok(sim, snap_dev, rec_bytes))
    return sim ? fail(sim, MMX_EINVAL, "mmx_snapshot: bad arguments (NULL or unaligned blob, or not this sim's record size)") : MMX_EINVAL;
  DeviceGuard guard(sim);
  return hip_check(sim, mmx_launch_snapshot(&sim->S, snap_dev, sim->stream), "mmx_snapshot");
}

int mmx_restore(mmx_sim* sim, const void* snap_dev, int64_t rec_bytes, int32_t n_records, const int32_t* src_dev) {
  if (!snapshot_args_ok(sim, snap_dev, rec_bytes) || n_records < 0)
    return sim ? fail(sim, MMX_EINVAL, "mmx_restore: bad arguments (NULL or unaligned blob, not this sim's record size, or n_records < 0)")
               : MMX_EINVAL;
  if (n_records == 0) return MMX_OK;
  DeviceGuard guard(sim);
  const MMXState& S = sim->S;  // S.rpose: the pose buffer that is current now (camera rollouts swap it)
  unsigned char* mask = S.image_size > 0 ? sim->d_mask : nullptr;
  hipError_t e = mmx_launch_restore(&S, snap_dev, n_records, src_dev, mask, sim->stream);
  // the restored envs' images and segment ids, redrawn from the restored poses with the sim's current effects
  if (e == hipSuccess && mask) e = render(sim, S, 0, S.N, mask, sim->stream);
  return hip_check(sim, e, "mmx_restore");
}

// MPPI planner (mmx_mppi.hip, mmx_mppi.h): sample -> branch (the restore kernel at the blob's stride) -> the
// trajectory rollout with reward and done recorded -> reweight, all queued on the planner sim's stream.
int mmx_mppi_create(mmx_sim* sim, const mmx_mppi_config* c, mmx_mppi** out) {
  if (out) *out = nullptr;
  if (!sim || !c || !out) return sim ? fail(sim, MMX_EINVAL, "mmx_mppi_create: NULL argument") : MMX_EINVAL;
  if (sim->S.image_size > 0) return fail(sim, MMX_EINVAL, "mmx_mppi_create: the planner sim must have no cameras");
  const int A = kDim[sim->S.action_mode], N = sim->S.N;
  // (written so that a NaN fails every range test)
  bool ok = c->horizon >= 1 && c->horizon <= MMX_MPPI_MAX_HORIZON && c->samples >= 2 && N % c->samples == 0;
  // (a temperature whose reciprocal overflows would turn the best candidate's exponent 0 * Inf into NaN)
  ok = ok && c->temperature >= 0.f && c->temperature <= FLT_MAX && (c->temperature == 0.f || 1.f / c->temperature <= FLT_MAX);
  ok = ok && c->discount > 0.f && c->discount <= 1.f;
  ok = ok && c->noise_beta >= 0.f && c->noise_beta < 1.f && A <= MMX_MPPI_MAX_ADIM;
  for (int a = 0; a < A && ok; a++)
    ok = c->sigma[a] >= 0.f && c->sigma[a] <= FLT_MAX && c->low[a] <= c->high[a] && c->low[a] >= -FLT_MAX && c->high[a] <= FLT_MAX;
  if (!ok) return fail(sim, MMX_EINVAL, "mmx_mppi_create: a config field is outside its range, or num_envs % samples != 0");
  DeviceGuard guard(sim);
  mmx_mppi* p = new (std::nothrow) mmx_mppi();
  if (!p) return fail(sim, MMX_ENOMEM, "mmx_mppi_create: host allocation");
  p->sim = sim;
  p->device = sim->cfg.device;
  MppiParams& P = p->P;
  P.H = c->horizon, P.K = c->samples, P.M = N / c->samples, P.A = A;
  P.inv_lambda = c->temperature > 0.f ? 1.f / c->temperature : 0.f;
  P.gamma = c->discount;
  P.beta = c->noise_beta;
  P.beta_c = std::sqrt(1.f - c->noise_beta * c->noise_beta);
  P.seed_lo = (uint32_t)c->seed, P.seed_hi = (uint32_t)(c->seed >> 32);
  const size_t H = (size_t)P.H, M = (size_t)P.M, n = (size_t)N, a = (size_t)A;
  auto alloc = [&](size_t bytes) -> void* {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
    if (hipMemset(d, 0, bytes) != hipSuccess) {
      (void)hipFree(d);
      return nullptr;
    }
    p->allocs.push_back(d);
    return d;
  };
  MppiBufs& B = p->B;
  B.nominal = static_cast<float*>(alloc(H * M * a * 4));
  B.noise = static_cast<float*>(alloc(H * n * a * 4));
  B.actions = static_cast<float*>(alloc(H * n * a * 4));
  B.reward = static_cast<float*>(alloc(H * n * 4));
  B.done = static_cast<int*>(alloc(H * n * 3 * 4));
  B.returns = static_cast<float*>(alloc(n * 4));
  B.weights = static_cast<float*>(alloc(n * 4));
  B.best = static_cast<int*>(alloc(M * 4));
  p->box = static_cast<float*>(alloc(3 * MMX_MPPI_MAX_ADIM * 4));
  p->src = static_cast<int*>(alloc(n * 4));
  if (p->allocs.size() != 10) {
    mmx_mppi_destroy(p);
    return fail(sim, MMX_ENOMEM, "mmx_mppi_create: device allocation");
  }
  float box[3 * MMX_MPPI_MAX_ADIM] = {};
  for (int k = 0; k < A; k++) box[k] = c->sigma[k], box[MMX_MPPI_MAX_ADIM + k] = c->low[k], box[2 * MMX_MPPI_MAX_ADIM + k] = c->high[k];
  std::vector<int> src(n);
  for (size_t i = 0; i < n; i++) src[i] = (int)(i / (size_t)P.K);
  hipError_t e = hipMemcpy(p->box, box, sizeof(box), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->src, src.data(), n * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    mmx_mppi_destroy(p);
    return hip_check(sim, e, "mmx_mppi_create upload");
  }
  *out = p;
  return MMX_OK;
}

void mmx_mppi_destroy(mmx_mppi* p) {
  if (!p) return;
  DeviceGuard guard(p->device);
  for (void* d : p->allocs) (void)hipFree(d);
  delete p;
}

int mmx_mppi_reset(mmx_mppi* p, const float* action_dev) {
  if (!p || !action_dev) return p ? fail(p->sim, MMX_EINVAL, "mmx_mppi_reset: NULL action") : MMX_EINVAL;
  DeviceGuard guard(p->sim);
  p->call = 0;
  return hip_check(p->sim, mmx_launch_mppi_fill(&p->P, p->B.nominal, p->box, action_dev, p->sim->stream), "mmx_mppi_reset");
}

int mmx_mppi_plan(mmx_mppi* p, const void* snap_dev, int64_t rec_bytes, int32_t n_records, const float* xi_dev,
                  float* action_out_dev) {
  if (!p) return MMX_EINVAL;
  mmx_sim* sim = p->sim;
  if (!snap_dev || !action_out_dev || reinterpret_cast<uintptr_t>(snap_dev) % 16 != 0 ||
      (rec_bytes != MMX_SNAPSHOT_BYTES && rec_bytes != MMX_SNAPSHOT_BYTES_CAMERAS) || n_records != p->P.M)
    return fail(sim, MMX_EINVAL, "mmx_mppi_plan: bad arguments (NULL or unaligned blob, NULL output, not a record size, or "
                                 "n_records != num_envs / samples)");
  DeviceGuard guard(sim);
  MppiParams P = p->P;
  P.call_lo = (uint32_t)p->call, P.call_hi = (uint32_t)(p->call >> 32);
  hipError_t e = mmx_launch_mppi_sample(&P, &p->B, p->box, xi_dev, sim->stream);
  if (e == hipSuccess) e = mmx_launch_restore_strided(&sim->S, snap_dev, rec_bytes, n_records, p->src, nullptr, sim->stream);
  if (e != hipSuccess) return hip_check(sim, e, "mmx_mppi_plan");
  mmx_trajectory rec{};
  rec.reward = p->B.reward;
  rec.done = p->B.done;
  const int rc = rollout_traj(sim, p->B.actions, P.A, 0, P.H, &rec, "mmx_mppi_plan");
  if (rc != MMX_OK) return rc;
  e = mmx_launch_mppi_update(&P, &p->B, p->box, action_out_dev, sim->stream);
  if (e == hipSuccess) p->call++;
  return hip_check(sim, e, "mmx_mppi_plan");
}

int mmx_mppi_reweight(mmx_mppi* p, float* action_out_dev) {
  if (!p || !action_out_dev) return p ? fail(p->sim, MMX_EINVAL, "mmx_mppi_reweight: NULL output") : MMX_EINVAL;
  DeviceGuard guard(p->sim);
  return hip_check(p->sim, mmx_launch_mppi_update(&p->P, &p->B, p->box, action_out_dev, p->sim->stream), "mmx_mppi_reweight");
}

int mmx_mppi_get_buffers(mmx_mppi* p, mmx_mppi_buffers* out) {
  if (!p || !out) return MMX_EINVAL;
  const MppiBufs& B = p->B;
  *out = mmx_mppi_buffers{B.nominal, B.noise, B.actions, B.reward, B.done, B.returns, B.weights, B.best};
  return MMX_OK;
}

// MLP policies (mmx_policy.h; mmx_policy.hip, mmx_env_policy_kernel of mmx_step_kernels.inc)
int mmx_policy_create(mmx_sim* sim, const mmx_policy_config* c, mmx_policy** out) {
  if (out) *out = nullptr;
  if (!sim || !c || !out) return sim ? fail(sim, MMX_EINVAL, "mmx_policy_create: NULL argument") : MMX_EINVAL;
  bool ok = c->n_layers >= 1 && c->n_layers <= MMX_POLICY_MAX_LAYERS &&
            (c->activation == MMX_POLICY_TANH || c->activation == MMX_POLICY_RELU);
  for (int l = 0; l < c->n_layers && ok; l++) ok = c->width[l] >= 1 && c->width[l] <= MMX_POLICY_MAX_WIDTH && c->weight[l];
  ok = ok && c->width[c->n_layers - 1] <= MMX_MPPI_MAX_ADIM;
  if (!ok)
    return fail(sim, MMX_EINVAL, "mmx_policy_create: n_layers outside 1..4, a width outside 1..256, a last width above 10, a NULL "
                                 "weight or an unknown activation");
  mmx_policy* p = new (std::nothrow) mmx_policy();
  if (!p) return fail(sim, MMX_ENOMEM, "mmx_policy_create: host allocation");
  p->sim = sim;
  p->device = sim->cfg.device;
  MmxPolicy& P = p->P;
  P.n_layers = c->n_layers;
  P.activation = c->activation;
  for (int l = 0; l < c->n_layers; l++) P.in[l] = l ? c->width[l - 1] : MMX_NOBS, P.out[l] = c->width[l];
  P.A = c->width[c->n_layers - 1];
  P.stochastic = c->log_std != nullptr;
  P.seed_lo = (uint32_t)c->seed, P.seed_hi = (uint32_t)(c->seed >> 32);
  std::vector<float> blob(policy_layout(P));
  policy_pack(P, c->weight, c->bias, c->obs_shift, c->obs_scale, c->log_std, c->low, c->high, blob.data());
  std::copy(blob.begin() + P.std_off, blob.begin() + P.std_off + MMX_MPPI_MAX_ADIM, p->std_host);
  DeviceGuard guard(sim);
  void* d = nullptr;
  if (hipMalloc(&d, blob.size() * sizeof(float)) != hipSuccess) {
    delete p;
    return fail(sim, MMX_ENOMEM, "mmx_policy_create: device allocation");
  }
  p->data = static_cast<float*>(d);
  P.data = p->data;
  const hipError_t e = hipMemcpy(d, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    mmx_policy_destroy(p);
    return hip_check(sim, e, "mmx_policy_create upload");
  }
  *out = p;
  return MMX_OK;
}

void mmx_policy_destroy(mmx_policy* p) {
  if (!p) return;
  DeviceGuard guard(p->device);
  if (p->data) (void)hipFree(p->data);
  for (float* a : {p->fit_m, p->fit_v, p->fit_ws})
    if (a) (void)hipFree(a);
  delete p;
}

int mmx_policy_eval(mmx_policy* p, const float* obs_dev, int32_t n, float* mean_out_dev) {
  if (!p) return MMX_EINVAL;
  if (!obs_dev || !mean_out_dev || n < 0) return fail(p->sim, MMX_EINVAL, "mmx_policy_eval: NULL argument or n < 0");
  DeviceGuard guard(p->sim);
  return hip_check(p->sim, mmx_launch_policy_eval(&p->P, obs_dev, n, mean_out_dev, p->sim->stream), "mmx_policy_eval");
}

// What mmx_policy_fit and mmx_policy_fit_pg ask of their common arguments (`data_ok`: the caller's own pointers),
// each refusal under the caller's name
static int policy_fit_args(mmx_sim* sim, const char* who, bool data_ok, int64_t n_pairs, int32_t n_steps, const mmx_fit_config* c) {
  const std::string w(who);
  if (!data_ok || !c) return fail(sim, MMX_EINVAL, w + ": NULL argument");
  if (n_pairs < 1 || n_pairs > INT32_MAX || n_steps < 0) return fail(sim, MMX_EINVAL, w + ": n_pairs outside 1 .. 2^31 - 1 or n_steps < 0");
  if (c->batch < 1 || c->batch > MMX_FIT_MAX_BATCH) return fail(sim, MMX_EINVAL, w + ": batch outside 1 .. 65536");
  if (c->optimizer != MMX_FIT_SGD && c->optimizer != MMX_FIT_ADAM) return fail(sim, MMX_EINVAL, w + ": unknown optimizer");
  // (written so that a NaN fails every test)
  if (!(c->lr > 0.f && c->lr <= FLT_MAX) || !(c->eps > 0.f && c->eps <= FLT_MAX))
    return fail(sim, MMX_EINVAL, w + ": lr or eps not finite or <= 0");
  if (!(c->beta1 >= 0.f && c->beta1 < 1.f) || !(c->beta2 >= 0.f && c->beta2 < 1.f))
    return fail(sim, MMX_EINVAL, w + ": a beta outside [0, 1)");
  return MMX_OK;
}
// The state both fits share, made ready for a call of n_steps > 0: m and v (allocated and cleared at the first fit),
// the workspace of a batch of c->batch (grown behind a stream synchronisation; it always holds the PG statistics'
// partials too), the optimiser's reset; then F's and G's fields that do not depend on the objective
static int policy_fit_prepare(mmx_policy* p, const char* who, const mmx_fit_config* c, const float* obs_dev, int64_t n_pairs, MmxFit* F,
                              MmxPg* G) {
  mmx_sim* sim = p->sim;
  const std::string w(who);
  const MmxPolicy& P = p->P;
  const size_t params = policy_fit_param_floats(P);
  if (!p->fit_m) {
    void *m = nullptr, *v = nullptr;
    if (hipMalloc(&m, params * sizeof(float)) != hipSuccess || hipMalloc(&v, params * sizeof(float)) != hipSuccess) {
      if (m) (void)hipFree(m);
      return fail(sim, MMX_ENOMEM, w + ": device allocation");
    }
    p->fit_m = static_cast<float*>(m), p->fit_v = static_cast<float*>(v);
    if (hipMemsetAsync(m, 0, params * sizeof(float), sim->stream) != hipSuccess ||
        hipMemsetAsync(v, 0, params * sizeof(float), sim->stream) != hipSuccess)
      return fail(sim, MMX_EDEVICE, w + ": clearing the optimiser state");
  }
  if (c->batch > p->fit_batch) {
    if (p->fit_ws) {  // launches queued by an earlier call may still use it
      if (hipStreamSynchronize(sim->stream) != hipSuccess) return fail(sim, MMX_EDEVICE, w + " sync");
      (void)hipFree(p->fit_ws);
      p->fit_ws = nullptr, p->fit_batch = 0;
    }
    void* ws = nullptr;
    if (hipMalloc(&ws, mmx_policy_fit_pg_workspace_floats(&P, c->batch, nullptr, nullptr) * sizeof(float)) != hipSuccess)
      return fail(sim, MMX_ENOMEM, w + ": device allocation (workspace)");
    p->fit_ws = static_cast<float*>(ws), p->fit_batch = c->batch;
  }
  if (c->reset_optimizer) {
    if (hipMemsetAsync(p->fit_m, 0, params * sizeof(float), sim->stream) != hipSuccess ||
        hipMemsetAsync(p->fit_v, 0, params * sizeof(float), sim->stream) != hipSuccess)
      return fail(sim, MMX_EDEVICE, w + ": clearing the optimiser state");
    p->fit_t = 0;
  }
  F->obs = obs_dev, F->n = n_pairs, F->ws = p->fit_ws;
  (void)mmx_policy_fit_pg_workspace_floats(&P, c->batch, F, G);
  F->seed_lo = (uint32_t)c->seed, F->seed_hi = (uint32_t)(c->seed >> 32);
  F->B = c->batch, F->shuffle = c->shuffle != 0;
  F->inv_count = policy_fit_inv_count(c->batch, P.A), F->dscale = 2.f * F->inv_count;
  return MMX_OK;
}

// The policy's training step (mmx_policy_fit.h; mmx_policy_fit.hip): n_steps times three launches on the stream
int mmx_policy_fit(mmx_policy* p, const float* obs_dev, const float* target_dev, int64_t n_pairs, int32_t n_steps,
                   const mmx_fit_config* c, float* loss_out_dev) {
  if (!p) return MMX_EINVAL;
  mmx_sim* sim = p->sim;
  if (const int rc = policy_fit_args(sim, "mmx_policy_fit", obs_dev && target_dev, n_pairs, n_steps, c)) return rc;
  if (n_steps == 0) return MMX_OK;
  DeviceGuard guard(sim);
  MmxFit F{};
  MmxPg G{};
  if (const int rc = policy_fit_prepare(p, "mmx_policy_fit", c, obs_dev, n_pairs, &F, &G)) return rc;
  F.target = target_dev;
  for (int32_t i = 0; i < n_steps; i++) {
    F.k = p->fit_t++;
    const MmxFitOpt O = policy_fit_opt(c->optimizer, c->lr, c->beta1, c->beta2, c->eps, p->fit_t);
    const hipError_t e = mmx_launch_policy_fit_step(&p->P, &F, &O, p->data, p->fit_m, p->fit_v,
                                                    loss_out_dev ? loss_out_dev + i : nullptr, sim->stream);
    if (e != hipSuccess) return hip_check(sim, e, "mmx_policy_fit");
  }
  return MMX_OK;
}

// The policy-gradient step (mmx_pg.h; mmx_policy_fit.hip): the same state and workspace, PPO's clipped surrogate as
// the output delta, n_steps times four launches on the stream.  std_host: the policy's std as the blob holds it
int mmx_policy_fit_pg(mmx_policy* p, const float* obs_dev, const float* mean_old_dev, const float* noise_dev, const float* adv_dev,
                      int64_t n_pairs, int32_t n_steps, const mmx_pg_config* c, float* stats_out_dev) {
  if (!p) return MMX_EINVAL;
  mmx_sim* sim = p->sim;
  if (const int rc = policy_fit_args(sim, "mmx_policy_fit_pg", obs_dev && mean_old_dev && noise_dev && adv_dev, n_pairs, n_steps,
                                     c ? &c->fit : nullptr))
    return rc;
  if (!(c->clip > 0.f && c->clip < 1.f)) return fail(sim, MMX_EINVAL, "mmx_policy_fit_pg: clip not finite or outside (0, 1)");
  for (int a = 0; a < p->P.A; a++)
    if (!(p->std_host[a] > 0.f))
      return fail(sim, MMX_EINVAL, "mmx_policy_fit_pg: a deterministic policy (no log_std, or a std of 0) has no likelihood ratio");
  if (n_steps == 0) return MMX_OK;
  DeviceGuard guard(sim);
  MmxFit F{};
  MmxPg G{};
  if (const int rc = policy_fit_prepare(p, "mmx_policy_fit_pg", &c->fit, obs_dev, n_pairs, &F, &G)) return rc;
  G.mean_old = mean_old_dev, G.noise = noise_dev, G.adv = adv_dev;
  G.invB = pg_inv_batch(c->fit.batch), G.lo = 1.f - c->clip, G.hi = 1.f + c->clip;
  for (int32_t i = 0; i < n_steps; i++) {
    F.k = p->fit_t++;
    const MmxFitOpt O = policy_fit_opt(c->fit.optimizer, c->fit.lr, c->fit.beta1, c->fit.beta2, c->fit.eps, p->fit_t);
    const hipError_t e = mmx_launch_policy_fit_pg_step(&p->P, &F, &G, &O, p->data, p->fit_m, p->fit_v,
                                                       stats_out_dev ? stats_out_dev + 3 * (size_t)i : nullptr, sim->stream);
    if (e != hipSuccess) return hip_check(sim, e, "mmx_policy_fit_pg");
  }
  return MMX_OK;
}

// exp(log_std) as mmx_policy_create evaluates it, into the blob's std entries in place on the stream
int mmx_policy_set_log_std(mmx_policy* p, const float* log_std_host) {
  if (!p) return MMX_EINVAL;
  if (!log_std_host) return fail(p->sim, MMX_EINVAL, "mmx_policy_set_log_std: NULL argument");
  float sd[MMX_MPPI_MAX_ADIM] = {};
  for (int a = 0; a < p->P.A; a++) {
    if (!(log_std_host[a] >= -FLT_MAX && log_std_host[a] <= FLT_MAX)) return fail(p->sim, MMX_EINVAL, "mmx_policy_set_log_std: an entry that is not finite");
    sd[a] = (float)exp((double)log_std_host[a]);
  }
  DeviceGuard guard(p->sim);
  // (synchronised: the host array is this frame's)
  if (hipMemcpyAsync(p->data + p->P.std_off, sd, sizeof(sd), hipMemcpyHostToDevice, p->sim->stream) != hipSuccess ||
      hipStreamSynchronize(p->sim->stream) != hipSuccess)
    return fail(p->sim, MMX_EDEVICE, "mmx_policy_set_log_std: upload");
  std::copy(sd, sd + MMX_MPPI_MAX_ADIM, p->std_host);
  p->P.stochastic = 1;
  return MMX_OK;
}

// Generalised advantage estimation over a rollout record (mmx_pg.h), and the advantages' normalisation
int mmx_gae(mmx_sim* sim, const mmx_gae_config* c, int32_t T, int32_t N, const float* reward_dev, const int32_t* done_dev,
            const float* value_dev, const float* value_last_dev, float* adv_out_dev, float* ret_out_dev) {
  if (!sim) return MMX_EINVAL;
  if (!c || !reward_dev || !done_dev || !value_dev || !value_last_dev || !adv_out_dev) return fail(sim, MMX_EINVAL, "mmx_gae: NULL argument");
  if (T < 0 || N < 1 || (int64_t)T * (int64_t)N > INT32_MAX) return fail(sim, MMX_EINVAL, "mmx_gae: T < 0, N < 1 or T N > 2^31 - 1");
  if (!(c->gamma >= 0.f && c->gamma <= 1.f) || !(c->lambda >= 0.f && c->lambda <= 1.f))
    return fail(sim, MMX_EINVAL, "mmx_gae: gamma or lambda outside [0, 1] or not finite");
  if (T == 0) return MMX_OK;
  DeviceGuard guard(sim);
  if (c->normalize && !sim->pg_moments) {
    sim->pg_moments = dalloc<float>(sim, 2);
    if (!sim->pg_moments) return fail(sim, MMX_ENOMEM, "mmx_gae: device allocation");
  }
  return hip_check(sim, mmx_launch_gae(c->gamma, c->gamma * c->lambda, T, N, reward_dev, done_dev, value_dev, value_last_dev, adv_out_dev,
                                       ret_out_dev, c->normalize ? sim->pg_moments : nullptr, sim->stream), "mmx_gae");
}

int mmx_policy_get_weights(mmx_policy* p, float* const* weight_host, float* const* bias_host) {
  if (!p) return MMX_EINVAL;
  if (!weight_host && !bias_host) return fail(p->sim, MMX_EINVAL, "mmx_policy_get_weights: NULL arguments");
  DeviceGuard guard(p->sim);
  const MmxPolicy& P = p->P;
  std::vector<float> blob(policy_fit_param_floats(P));
  if (hipStreamSynchronize(p->sim->stream) != hipSuccess ||
      hipMemcpy(blob.data(), p->data, blob.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(p->sim, MMX_EDEVICE, "mmx_policy_get_weights: readback");
  for (int l = 0; l < P.n_layers; l++) {
    const int in = P.in[l], out = P.out[l];
    for (int j = 0; j < out; j++) {
      if (weight_host && weight_host[l])
        for (int k = 0; k < in; k++) weight_host[l][(size_t)j * (size_t)in + (size_t)k] = blob[(size_t)P.woff[l] + policy_windex(out, k, j)];
      if (bias_host && bias_host[l]) bias_host[l][j] = blob[(size_t)P.boff[l] + (size_t)j];
    }
  }
  return MMX_OK;
}

int mmx_policy_set_weights(mmx_policy* p, const float* const* weight_host, const float* const* bias_host) {
  if (!p) return MMX_EINVAL;
  const MmxPolicy& P = p->P;
  bool ok = weight_host != nullptr;
  for (int l = 0; l < P.n_layers && ok; l++) ok = weight_host[l] != nullptr;
  if (!ok) return fail(p->sim, MMX_EINVAL, "mmx_policy_set_weights: a NULL weight");
  DeviceGuard guard(p->sim);
  // the layers' part of the blob, packed as at create: the vectors behind it (shift .. high) are not touched
  std::vector<float> blob(policy_fit_param_floats(P));
  for (int l = 0; l < P.n_layers; l++) {
    const int in = P.in[l], out = P.out[l], outp = policy_padded(out);
    const float* b = bias_host ? bias_host[l] : nullptr;
    for (int j = 0; j < outp; j++) {
      for (int k = 0; k < in; k++)
        blob[(size_t)P.woff[l] + policy_windex(out, k, j)] = j < out ? weight_host[l][(size_t)j * (size_t)in + (size_t)k] : 0.f;
      blob[(size_t)P.boff[l] + (size_t)j] = j < out && b ? b[j] : 0.f;
    }
  }
  if (hipMemcpyAsync(p->data, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, p->sim->stream) != hipSuccess ||
      hipStreamSynchronize(p->sim->stream) != hipSuccess)
    return fail(p->sim, MMX_EDEVICE, "mmx_policy_set_weights: upload");
  return MMX_OK;
}

// What mmx_rollout_policy and mmx_rollout_dagger ask of their arguments, in this order, each refusal with the
// caller's own text: `args_ok` (the caller's NULL and count test, which may not touch sim or policy unless both are
// given), the sim's action mode where the rollout needs one (`mode` >= 0), the policy's action width, the policy's
// device.  On MMX_OK *P holds the policy's parameters with the call counter of this rollout filled in.
struct PolicyRolloutTexts { const char *args, *mode, *width, *device; };
static int policy_rollout_args(mmx_sim* sim, const mmx_policy* policy, bool args_ok, int mode, int width, uint64_t call,
                               const PolicyRolloutTexts& text, MmxPolicy* P) {
  if (!sim || !policy || !args_ok) return sim ? fail(sim, MMX_EINVAL, text.args) : MMX_EINVAL;
  if (mode >= 0 && sim->S.action_mode != mode) return fail(sim, MMX_EINVAL, text.mode);
  if (policy->P.A != (width ? width : kDim[sim->S.action_mode])) return fail(sim, MMX_EINVAL, text.width);
  if (policy->device != sim->cfg.device) return fail(sim, MMX_EINVAL, text.device);
  *P = policy->P;
  P->call_lo = (uint32_t)call, P->call_hi = (uint32_t)(call >> 32);
  return MMX_OK;
}

int mmx_rollout_policy(mmx_sim* sim, mmx_policy* policy, int32_t n_env_steps, uint64_t call, const mmx_policy_record* prec,
                       const mmx_trajectory* rec) {
  MmxPolicy P;
  const int rc = policy_rollout_args(  // (width 0: the sim's action dimension)
      sim, policy, prec && prec->actions && n_env_steps >= 0, -1, 0, call,
      {"mmx_rollout_policy: bad arguments (NULL policy or actions, or n_env_steps < 0)", nullptr,
       "mmx_rollout_policy: the policy's action width is not the sim's action dimension",
       "mmx_rollout_policy: the policy was created on another device"},
      &P);
  if (rc != MMX_OK) return rc;
  const MMXTraj R = traj_arg(rec);
  const MMXPolicyRec PR{prec->actions, prec->mean, prec->noise};
  const auto launch = step_launchers(sim).policy;
  return rollout(sim, n_env_steps, "mmx_rollout_policy", false,
                 [&](const MMXState* S, int base, int count, int ns, int k0, hipStream_t st, const int* ord, const MMXBudget*) {
                   return launch(S, &R, &P, &PR, base, count, ns, k0, st, ord);
                 });
}

// DAgger rollouts (mmx_dagger.h; mmx_env_dagger_kernel of mmx_step_kernels.inc): mmx_rollout_policy's launches
// with the FSM expert planning beside the learner and a gate choosing who acts
int mmx_rollout_dagger(mmx_sim* sim, mmx_policy* policy, int32_t n_env_steps, uint64_t call, const mmx_dagger_config* cfg,
                       const mmx_dagger_record* drec, const mmx_trajectory* rec) {
  MmxPolicy P;
  const int rc = policy_rollout_args(
      sim, policy, cfg && drec && drec->actions && n_env_steps >= 0, MMX_ACTION_ABS_POS, 4, call,
      {"mmx_rollout_dagger: bad arguments (NULL policy, cfg, drec or actions, or n_env_steps < 0)",
       "mmx_rollout_dagger needs action_mode abs_pos", "mmx_rollout_dagger: the policy's action width is not 4",
       "mmx_rollout_dagger: the policy was created on another device"},
      &P);
  if (rc != MMX_OK) return rc;
  // (written so that a NaN fails every test)
  if (!(cfg->beta >= 0.f && cfg->beta <= 1.f)) return fail(sim, MMX_EINVAL, "mmx_rollout_dagger: beta outside [0, 1]");
  if (!(cfg->takeover_dist >= 0.f && cfg->takeover_dist <= FLT_MAX))
    return fail(sim, MMX_EINVAL, "mmx_rollout_dagger: takeover_dist negative or not finite");
  const MMXTraj R = traj_arg(rec);
  // the learner's row: the caller's policy_action, or the actions array itself (read back before it is overwritten)
  float* const learner = drec->policy_action ? drec->policy_action : drec->actions;
  const MMXPolicyRec PR{learner, drec->mean, drec->noise};
  const MMXDagger D{drec->actions, drec->expert_action, learner, drec->gate, drec->obs_in, cfg->beta, cfg->takeover_dist};
  const auto launch = step_launchers(sim).dagger;
  return rollout(sim, n_env_steps, "mmx_rollout_dagger", false,
                 [&](const MMXState* S, int base, int count, int ns, int k0, hipStream_t st, const int* ord, const MMXBudget*) {
                   return launch(S, &R, &P, &PR, &D, base, count, ns, k0, st, ord);
                 });
}

int mmx_queue_init(mmx_sim* sim, int32_t n_episodes, const uint64_t* seeds, const int32_t* tasks) {
  if (!sim || n_episodes < 0 || (n_episodes > 0 && !tasks)) return MMX_EINVAL;
  DeviceGuard guard(sim);
  const size_t E = static_cast<size_t>(n_episodes), n = static_cast<size_t>(sim->S.N);
  for (size_t e = 0; e < E; e++)
    if (!task_code_ok(tasks[e])) return fail(sim, MMX_EINVAL, "queue task out of range");
  if (hipStreamSynchronize(sim->stream) != hipSuccess) return fail(sim, MMX_EDEVICE, "mmx_queue_init sync");
  for (void* p : {static_cast<void*>(sim->q_slot), static_cast<void*>(sim->q_next), static_cast<void*>(sim->q_task),
                  static_cast<void*>(sim->q_rng)}) {
    if (!p) continue;
    sim->allocs.erase(std::remove(sim->allocs.begin(), sim->allocs.end(), p), sim->allocs.end());
    (void)hipFree(p);
  }
  sim->q_rng = nullptr;
  sim->q_n = -1;
  sim->q_slot = dalloc<int>(sim, n);
  sim->q_next = dalloc<int>(sim, 1);
  sim->q_task = dalloc<int>(sim, std::max<size_t>(E, 1));
  if (!sim->q_slot || !sim->q_next || !sim->q_task) return fail(sim, MMX_EDEVICE, "queue allocation");
  std::vector<int> slot(n, -1);
  hipError_t e = hipMemcpy(sim->q_slot, slot.data(), n * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess && E) e = hipMemcpy(sim->q_task, tasks, E * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess && seeds && E) {  // PCG64(SeedSequence(seed_e)) of every episode, once
    std::vector<unsigned long long> rng(4 * E);
    for (size_t k = 0; k < E; k++) pcg64_seed_row(&rng[4 * k], seeds[k]);
    sim->q_rng = dalloc<unsigned long long>(sim, 4 * E);
    if (!sim->q_rng) return fail(sim, MMX_EDEVICE, "queue allocation");
    e = hipMemcpy(sim->q_rng, rng.data(), rng.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) return hip_check(sim, e, "mmx_queue_init upload");
  sim->q_n = n_episodes;
  return MMX_OK;
}

int mmx_queue_advance(mmx_sim* sim, int32_t* slot_ep_dev, int32_t* fin_ep_dev) {
  if (!sim) return MMX_EINVAL;
  if (sim->q_n < 0) return fail(sim, MMX_EINVAL, "mmx_queue_advance without mmx_queue_init");
  DeviceGuard guard(sim);
  MMXState& S = sim->S;
  hipError_t e = mmx_launch_queue(&S, sim->q_slot, sim->q_next, sim->q_n, sim->q_rng, sim->q_task, sim->d_mask,
                                  sim->d_task, slot_ep_dev, fin_ep_dev, sim->stream);
  if (e == hipSuccess) e = mmx_launch_reset(&S, sim->d_mask, sim->d_task, sim->stream);
  if (e == hipSuccess) e = render(sim, S, 0, S.N, sim->d_mask, sim->stream);
  return hip_check(sim, e, "mmx_queue_advance");
}

uint32_t mmx_episode_seed(uint64_t root, int32_t index) {
  return episode_seed(root, index);
}

}  // extern "C"

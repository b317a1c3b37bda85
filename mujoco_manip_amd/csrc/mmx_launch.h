// The host seam between mmx_api.cpp and the kernel sources: every non-kernel extern "C" function that one
// source defines and another calls, declared once.  mmx_api.cpp includes it and so does every source that
// defines one of them (mmx_step.inc, whose launchers are in mmx_step_kernels.inc, mmx_render.hip, mmx_png.hip, mmx_snapshot.hip, mmx_mppi.hip, mmx_policy.hip, mmx_policy_fit.hip), so a parameter list
// changed on one side only is a compile error.  (The diagnostic exports that tools load through ctypes,
// mmx_fsm_profile and mmx_render_clock among them, are not called across sources and are not listed.)
#ifndef MMX_LAUNCH_H
#define MMX_LAUNCH_H
#include <hip/hip_runtime.h>

#include "mmx_state.h"

struct MppiParams;
struct MppiBufs;
struct MmxPolicy;
struct MMXPolicyRec;
struct MMXDagger;
struct MmxFit;
struct MmxFitOpt;
struct MmxPg;

extern "C" {

// mmx_step_kernels.inc (the last part of mmx_step.inc), built once per LDS-row layout: the launchers' names
// carry the layout's suffix
#define MMX_DECLARE_STEP_LAUNCHERS(sfx)                                                                                \
  hipError_t mmx_launch_step##sfx(const MMXState* S, const float* action, int adim, int expert, int base, int count,   \
                                  int nsteps, hipStream_t st, const int* order);                                       \
  hipError_t mmx_launch_traj##sfx(const MMXState* S, const MMXTraj* R, const float* actions, int adim, int expert,     \
                                  int base, int count, int nsteps, int k0, hipStream_t st, const int* order);          \
  hipError_t mmx_launch_physics##sfx(const MMXState* S, int n, int with_ik, hipStream_t st);                           \
  hipError_t mmx_launch_policy##sfx(const MMXState* S, const MMXTraj* R, const MmxPolicy* P, const MMXPolicyRec* PR,   \
                                    int base, int count, int nsteps, int k0, hipStream_t st, const int* order);  \
  hipError_t mmx_launch_dagger##sfx(const MMXState* S, const MMXTraj* R, const MmxPolicy* P, const MMXPolicyRec* PR,   \
                                    const MMXDagger* D, int base, int count, int nsteps, int k0, hipStream_t st,       \
                                    const int* order);
MMX_DECLARE_STEP_LAUNCHERS()
MMX_DECLARE_STEP_LAUNCHERS(_l192)
#undef MMX_DECLARE_STEP_LAUNCHERS
// the 128-row build alone: expert steps up to cumulative bounds and a time budget (MMXBudget, mmx_state.h)
hipError_t mmx_launch_step_budget(const MMXState* S, const MMXBudget* B, const float* action, int adim, int base, int count,
                                  hipStream_t st, const int* order);

// mmx_kernels.hip
hipError_t mmx_launch_order(const MMXState* S, int base, int count, int* order, int threads, hipStream_t st);
hipError_t mmx_launch_queue(const MMXState* S, int* slot, int* next, int n_ep, const unsigned long long* rng,
                            const int* qtask, unsigned char* mask, int* task, int* slot_out, int* fin_out, hipStream_t st);
hipError_t mmx_launch_reset(const MMXState* S, const unsigned char* mask, const int* task, hipStream_t st);
hipError_t mmx_launch_expert(const MMXState* S, int n, float* action, hipStream_t st);
hipError_t mmx_launch_expert_physics(const MMXState* S, int n, hipStream_t st);
// the contact-force pass on the current state of every env, into the arrays of F (MMXForce, mmx_state.h)
hipError_t mmx_launch_contact_force(const MMXState* S, const MMXForce* F, hipStream_t st);
hipError_t mmx_launch_reward(const MMXState* S, const float* obj, const float* ee, const float* ctrl7, const int* pairs,
                             int max_pairs, hipStream_t st);
hipError_t mmx_launch_forward(const MMXState* S, hipStream_t st);

// mmx_render.hip; mmx_launch_render_lit, mmx_render_shadow_map_bytes: its second build, mmx_render_lit.hip.
// The render of envs [base, base + count), with a device mask (N bytes; may be null) only of the envs whose
// byte is set; flags = the sim's MMX_RENDER_* effects (0: the flat kernel, else mmx_launch_render_lit),
// shmap = its shadow maps (null without MMX_RENDER_SHADOWS)
hipError_t mmx_launch_render(const MMXState* S, int base, int count, const unsigned char* mask, int flags,
                             unsigned short* shmap, hipStream_t st);
hipError_t mmx_launch_render_lit(const MMXState* S, int base, int count, const unsigned char* mask, int flags,
                                 unsigned short* shmap, hipStream_t st);
hipError_t mmx_launch_render_bg(const MMXState* S, hipStream_t st);
size_t mmx_render_lds_bytes();
size_t mmx_render_shadow_map_bytes();

// mmx_png.hip
hipError_t mmx_launch_png(const uint8_t* rgb, int64_t img_stride, int n, int W, int H, uint8_t* out, int64_t out_stride,
                          int32_t* sizes, uint32_t* scratch, hipStream_t st);
hipError_t mmx_launch_png_pack(const uint8_t* out, int64_t out_stride, const int32_t* sizes, const int64_t* offsets, int n,
                               uint8_t* packed, hipStream_t st);
hipError_t mmx_launch_image_stats(const uint8_t* rgb, int64_t img_stride, int n, int64_t npx, int64_t* out, hipStream_t st);
int64_t mmx_png_bound_bytes(int width, int height);
int64_t mmx_png_scratch_bytes(int width, int height);

// mmx_snapshot.hip
hipError_t mmx_launch_snapshot(const MMXState* S, void* blob, hipStream_t st);
hipError_t mmx_launch_restore(const MMXState* S, const void* blob, int n_records, const int* src, unsigned char* mask,
                              hipStream_t st);
// the same restore of records that lie rec_bytes apart (>= the sim's own record size: a camera-less sim reads
// the fixed prefix of records taken with cameras); mmx_launch_restore is this at the sim's own record size
hipError_t mmx_launch_restore_strided(const MMXState* S, const void* blob, int64_t rec_bytes, int n_records, const int* src,
                                      unsigned char* mask, hipStream_t st);
int64_t mmx_snapshot_record_bytes(int cameras);

// mmx_mppi.hip (MppiParams, MppiBufs: mmx_mppi.h); box = device [3][MPPI_MAX_ADIM] sigma, low, high
hipError_t mmx_launch_mppi_sample(const MppiParams* P, const MppiBufs* B, const float* box, const float* xi, hipStream_t st);
hipError_t mmx_launch_mppi_update(const MppiParams* P, const MppiBufs* B, const float* box, float* action_out,
                                  hipStream_t st);
hipError_t mmx_launch_mppi_fill(const MppiParams* P, float* nominal, const float* box, const float* action, hipStream_t st);

// mmx_policy.hip (MmxPolicy, MMXPolicyRec: mmx_policy.h): the network alone on n observation rows, one wave each
hipError_t mmx_launch_policy_eval(const MmxPolicy* P, const float* obs, int n, float* mean_out, hipStream_t st);

// mmx_policy_fit.hip (MmxFit, MmxFitOpt: mmx_policy_fit.h): the floats of the workspace of a batch of B (F, when not
// null, gets its three bases), and the three launches of one optimisation step; m, v: the optimiser's arrays,
// loss_out: one float or null
size_t mmx_policy_fit_workspace_floats(const MmxPolicy* P, int B, MmxFit* F);
hipError_t mmx_launch_policy_fit_step(const MmxPolicy* P, const MmxFit* F, const MmxFitOpt* O, float* blob, float* m, float* v,
                                      float* loss_out, hipStream_t st);
// the policy-gradient step (MmxPg: mmx_pg.h): the workspace with the statistics' partials behind it (G, when not
// null, gets stat_base), and one step's launches; stats_out: three floats or null.  mmx_launch_gae: the advantages
// of a [T][N] record, normalised in place when `moments` (two device floats of scratch) is not null
size_t mmx_policy_fit_pg_workspace_floats(const MmxPolicy* P, int B, MmxFit* F, MmxPg* G);
hipError_t mmx_launch_policy_fit_pg_step(const MmxPolicy* P, const MmxFit* F, const MmxPg* G, const MmxFitOpt* O, float* blob, float* m,
                                         float* v, float* stats_out, hipStream_t st);
hipError_t mmx_launch_gae(float gamma, float gl, int T, int N, const float* reward, const int32_t* done, const float* value,
                          const float* value_last, float* adv_out, float* ret_out, float* moments, hipStream_t st);

}  // extern "C"

#endif

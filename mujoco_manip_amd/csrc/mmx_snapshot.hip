// Snapshot and restore of whole environments on the device (mmx_snapshot / mmx_restore, include/mmx_api.h).
//
// What crosses a launch for one env is a dozen env-major arrays of MMXState (load_env / store_env and the
// EPI / EPF accesses of mmx_step_task.inc, the random stream, the facade's outputs and, with cameras, the body
// poses the renderer draws from).  A record is those rows of one env back to back, in the order of
// kFields below (the order documented in mmx_api.h and mirrored by _lib.SNAPSHOT_FIELDS):
//
//   bytes 0 .. 31        rng       4 x uint64  (32-byte aligned: copied as 64-bit words)
//   then packed dwords   rng32, qpos, qvel, ctrl, qacc_warmstart, kin, target, episode_i, episode_f, obs,
//                        reward, reward_components, done
//   padded to 16 bytes   = kFixedBytes (the record of a sim without cameras)
//   then                 rpose     [14][12] fp32, cameras only (16-byte aligned: copied as 16-byte words)
//
// One wave per env record, kWaves records per workgroup.  The rows of the env-major arrays are 4, 12, 16,
// 32, 72, 108 ... bytes long, so an env's row is only dword aligned in general: lane l moves dwords l,
// l + 64, ... of a field, coalesced on both sides; rng and rpose rows are 32 and 672 bytes, aligned, and
// move in 8- and 16-byte words.  No LDS, no atomics; the only data-dependent value is the restore's
// record index, read once per env and made wave-uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmx_state.h"
#include "mmx_launch.h"

namespace {

constexpr int kWaves = 4;           // env records per workgroup
constexpr int kRposeN = 14 * 12;    // MMXState::rpose: [14 slots][R row-major 9, p 3]
// dwords of the fields that follow rng, in record order
constexpr int kDwords[] = {1, MMX_NQ_, MMX_NV_, MMX_NU_, MMX_NV_, KIN_N, 4, EPI_N, EPF_N, MMX_NOBS, 1, 6, 3};
constexpr int kNFields = sizeof(kDwords) / sizeof(kDwords[0]);
constexpr int kMaxIter = 2;  // dwords per lane of the widest field (obs: 85)
constexpr int kRngBytes = 4 * 8;
constexpr int sum_dwords(int n) { return n == 0 ? 0 : kDwords[n - 1] + sum_dwords(n - 1); }
constexpr int max_dwords(int n) { return n == 0 ? 0 : (kDwords[n - 1] > max_dwords(n - 1) ? kDwords[n - 1] : max_dwords(n - 1)); }
static_assert(max_dwords(kNFields) <= 64 * kMaxIter, "a field's dwords: at most kMaxIter per lane");
constexpr int kFixedBytes = (kRngBytes + 4 * sum_dwords(kNFields) + 15) / 16 * 16;
constexpr int kCameraBytes = kFixedBytes + 4 * kRposeN;
static_assert(kFixedBytes == 1248 && kCameraBytes == 1920, "the record sizes include/mmx_api.h documents");
static_assert(kRngBytes % 8 == 0 && kFixedBytes % 16 == 0 && (4 * kRposeN) % 16 == 0, "alignment of the wide words");

// the env's rows of the dword fields, in record order
struct Rows {
  uint32_t* p[kNFields];
};
__device__ __forceinline__ Rows rows_of(const MMXState& S, size_t i) {
  Rows r;
  int f = 0;
  r.p[f++] = S.rng32 + i;
  r.p[f++] = reinterpret_cast<uint32_t*>(S.qpos + i * MMX_NQ_);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.qvel + i * MMX_NV_);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.ctrl + i * MMX_NU_);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.qacc_ws + i * MMX_NV_);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.kin + i * KIN_N);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.target + i * 4);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.epi + i * EPI_N);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.epf + i * EPF_N);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.obs + i * MMX_NOBS);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.reward + i);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.reward_components + i * 6);
  r.p[f++] = reinterpret_cast<uint32_t*>(S.done + i * 3);
  return r;
}

// Env i's rows <-> the record at `rec` (kRestore: record -> env).  Every lane of the wave calls it.
template <bool kRestore>
__device__ __forceinline__ void copy_record(const MMXState& S, size_t i, unsigned char* rec, int lane) {
  unsigned long long* rng_env = S.rng + 4 * i;
  unsigned long long* rng_rec = reinterpret_cast<unsigned long long*>(rec);
  float4* pose_env = S.rpose ? reinterpret_cast<float4*>(S.rpose + i * kRposeN) : nullptr;
  float4* pose_rec = reinterpret_cast<float4*>(rec + kFixedBytes);
  const Rows env = rows_of(S, i);
  uint32_t* const w0 = reinterpret_cast<uint32_t*>(rec + kRngBytes);
  // every load first, then every store: the loads are in flight together (one memory latency per record,
  // not one per field; the compiler cannot tell that the two sides never overlap)
  unsigned long long rng = 0ull;
  uint32_t v[kNFields][kMaxIter];
  float4 pose = float4{0.f, 0.f, 0.f, 0.f};
  if (lane < 4) rng = kRestore ? rng_rec[lane] : rng_env[lane];
  const uint32_t* w = w0;
#pragma unroll
  for (int f = 0; f < kNFields; f++) {
#pragma unroll
    for (int it = 0; it < kMaxIter; it++) {
      const int k = lane + 64 * it;
      if (64 * it < kDwords[f] && k < kDwords[f]) v[f][it] = kRestore ? w[k] : env.p[f][k];
    }
    w += kDwords[f];
  }
  if (pose_env && lane < kRposeN / 4) pose = kRestore ? pose_rec[lane] : pose_env[lane];
  if (lane < 4) (kRestore ? rng_env : rng_rec)[lane] = rng;
  uint32_t* o = w0;
#pragma unroll
  for (int f = 0; f < kNFields; f++) {
#pragma unroll
    for (int it = 0; it < kMaxIter; it++) {
      const int k = lane + 64 * it;
      if (64 * it < kDwords[f] && k < kDwords[f]) (kRestore ? env.p[f] : o)[k] = v[f][it];
    }
    o += kDwords[f];
  }
  if (pose_env && lane < kRposeN / 4) (kRestore ? pose_env : pose_rec)[lane] = pose;
}

}  // namespace

// record i = env i
extern "C" __global__ void __launch_bounds__(64 * kWaves) mmx_snapshot_kernel(MMXState S, unsigned char* blob, size_t rec_bytes) {
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
  if (i >= S.N) return;
  copy_record<false>(S, (size_t)i, blob + (size_t)i * rec_bytes, threadIdx.x & 63);
}

// env i takes record src[i] (src null: record i); an index outside [0, n_records) keeps the env and reads
// nothing of the blob.  mask (may be null): byte i = 1 when env i was restored, else 0, for the masked render.
extern "C" __global__ void __launch_bounds__(64 * kWaves)
mmx_restore_kernel(MMXState S, const unsigned char* blob, size_t rec_bytes, int n_records, const int* src, unsigned char* mask) {
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
  if (i >= S.N) return;
  const int r = __builtin_amdgcn_readfirstlane(src ? src[i] : i);
  const bool take = r >= 0 && r < n_records;
  if (mask && lane == 0) mask[i] = take ? 1 : 0;
  if (!take) return;
  copy_record<true>(S, (size_t)i, const_cast<unsigned char*>(blob) + (size_t)r * rec_bytes, lane);
}

// bytes of one env's record: with cameras the body poses are part of it
extern "C" int64_t mmx_snapshot_record_bytes(int cameras) { return cameras ? kCameraBytes : kFixedBytes; }

extern "C" hipError_t mmx_launch_snapshot(const MMXState* S, void* blob, hipStream_t st) {
  const size_t rec_bytes = (size_t)mmx_snapshot_record_bytes(S->rpose != nullptr);
  hipLaunchKernelGGL(mmx_snapshot_kernel, dim3((S->N + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, st, *S,
                     static_cast<unsigned char*>(blob), rec_bytes);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_restore_strided(const MMXState* S, const void* blob, int64_t rec_bytes, int n_records,
                                                 const int* src, unsigned char* mask, hipStream_t st) {
  if (rec_bytes < mmx_snapshot_record_bytes(S->rpose != nullptr) || rec_bytes % 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mmx_restore_kernel, dim3((S->N + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, st, *S,
                     static_cast<const unsigned char*>(blob), (size_t)rec_bytes, n_records, src, mask);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_restore(const MMXState* S, const void* blob, int n_records, const int* src,
                                         unsigned char* mask, hipStream_t st) {
  return mmx_launch_restore_strided(S, blob, mmx_snapshot_record_bytes(S->rpose != nullptr), n_records, src, mask, st);
}

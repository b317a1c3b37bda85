// The per-env cache of separating axes of the GJK pair class (convex_convex in mmx_geom.h; the table in the
// env's overflow block, MMX_OVF_AXIS_AT in mmx_state.h), as host + device inline functions: the step kernels
// call them, and a stand-alone host program (tests/host/mmx_gjk_cache_selftest.cpp, plain g++) runs the very
// same code.
//
// A GJK call that ends "separated" leaves the direction it ended on, normalised, in the pair's entry.  The
// next substep tests that direction first: one support query on the CURRENT poses, w = s_A(d) - s_B(-d), and
// w . d < -m proves that the origin lies outside A - B, whatever the entry holds: stale, of another episode,
// of a snapshot restored into the sim, or garbage.  A pair proven separated emits no contact and sets no flag
// on either path, and nothing else reads the cache, so no result depends on it.
#ifndef MMX_GJK_CACHE_H
#define MMX_GJK_CACHE_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GJKC_HD __host__ __device__ inline
#else
#define GJKC_HD inline
#endif
// device code: the value behind an opaque register copy, so that a test of its bits reads what the ALU
// produced (the compiler saw the value computed, and under -ffinite-math-only may fold a test it can see through)
#if defined(__HIP_DEVICE_COMPILE__)
#define GJKC_OPAQUE(v) asm volatile("" : "+v"(v))
#else
#define GJKC_OPAQUE(v) (void)0
#endif

// 0: compiled out (the test build libmmx_nocache.so): every call takes the uncached path
#ifndef MMX_GJK_CACHE
#define MMX_GJK_CACHE 1
#endif
// Entries per env, one per lane of the wave that runs the pair class (lane s owns entry s on the load and on
// the store).  Sized from the measured maximum of GJK candidates of one collision pass over a C3 rollout
// (profiles/r18_gjk_candidates.json: 4, and more than 2 in 0.9 % of the passes); a pair that finds no entry and
// no free slot takes the uncached path.
#define MMX_AXIS_SLOTS 8
#define MMX_AXIS_WORDS 4  // tag (pair index + 1; 0: empty), direction x, y, z
static_assert(MMX_AXIS_SLOTS <= 32, "the slot masks are 32-bit");

// The margin m of the cached verdict.  The test's value w . d is computed in fp32 from support points of
// the current poses: coordinates stay under 2 m (ulp 2.4e-7), a support point is a few fused multiply-adds
// of such values (G.x + R p: three products and adds, each rounding at most half an ulp of a value under
// 2 m: ~4e-7 per coordinate of a and of b), and the dot with the unit direction sums three products of
// |w_k| <= 4 m more (3 x 2^-24 x 4 m ~ 7e-7, less the direction's components being under 1): about 1e-6 m
// in all.  m is at least 8 x that bound, so a cached "separated" is a true gap of 9e-6 m or more, well
// outside the band in which gjk() may end on a degenerate-simplex exit and hand a near-zero depth to EPA;
// and under 4e-5 m, the smallest gap of the narrowphase sweep's near misses, so that those scenes are
// decided by the cached path when an entry exists.
#define MMX_AXIS_MARGIN 1e-5f

GJKC_HD uint32_t gjkc_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}
// A direction component the cache may hold: finite and of magnitude at most 1 + 2^-7, as a test of the bits
// (the device code is built -ffinite-math-only: a floating-point comparison on a NaN may be folded either
// way, an integer comparison may not).  Zero passes here and fails the verdict: 0 < -m is false.
GJKC_HD bool gjkc_component_ok(float v) { return (gjkc_bits(v) & 0x7fffffffu) <= 0x3f810000u; }
GJKC_HD bool gjkc_dir_ok(float x, float y, float z) {
  return gjkc_component_ok(x) && gjkc_component_ok(y) && gjkc_component_ok(z);
}
// The verdict: entry (tag, d) proves pair `pair` separated given the support difference w along d.  The
// tag is matched as an integer; the direction's bits are tested before any arithmetic on them, and its
// length may not exceed 1 (+ rounding), so that m is a metric margin; the value's own bits are tested
// finite before its comparison counts (w comes from the env's state, which a diverged env may have left
// non-finite).
GJKC_HD bool gjkc_separated(int tag, int pair, float dx, float dy, float dz, float wx, float wy, float wz) {
  if (tag != pair + 1 || !gjkc_dir_ok(dx, dy, dz)) return false;
  const float n2 = dx * dx + dy * dy + dz * dz;
  float s = wx * dx + wy * dy + wz * dz;
  GJKC_OPAQUE(s);
  const bool finite = (gjkc_bits(s) & 0x7f800000u) != 0x7f800000u;
  return finite && n2 <= 1.001f && s < -MMX_AXIS_MARGIN;
}
// The slot a pair's new entry goes to.  hit: the slots whose tag is the pair's (the lowest wins); busy: the
// slots this collision pass has already read a verdict from or written.  No hit: the first slot from
// pair % MMX_AXIS_SLOTS on, cyclically, that is not busy, so two pairs of one pass never evict each other;
// -1 when every slot is busy (the pair then stays uncached).  Always in [-1, MMX_AXIS_SLOTS).
GJKC_HD int gjkc_slot(unsigned hit, unsigned busy, int pair) {
  const unsigned all = (1u << MMX_AXIS_SLOTS) - 1u;
  hit &= all;
  if (hit) {
    int s = 0;
    while (!((hit >> s) & 1u)) s++;
    return s;
  }
  const int s0 = (int)((unsigned)pair % MMX_AXIS_SLOTS);
  for (int k = 0; k < MMX_AXIS_SLOTS; k++) {
    const int s = (s0 + k) % MMX_AXIS_SLOTS;
    if (!((busy >> s) & 1u)) return s;
  }
  return -1;
}

#endif

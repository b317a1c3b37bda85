// Stand-alone host program for tests/test_gjk_axis_cache_host.py: the axis cache's verdict and slot policy
// (csrc/mmx_gjk_cache.h, the code the step kernels run) built with plain g++ and the sanitizers.
//   verdict        reads lines "tag pair dxbits dybits dzbits wxbits wybits wzbits" (bits: hex words) from stdin,
//                  prints one 0 / 1 per line
//   slots SEED N   N random (hit, busy, pair) triples through gjkc_slot, each written into a table of exactly
//                  MMX_AXIS_SLOTS entries on the heap (AddressSanitizer sees a slot outside it); prints the
//                  triples and their slots as JSON lines
//   constants      MMX_AXIS_SLOTS, MMX_AXIS_WORDS and the margin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mujoco_manip_amd/csrc/mmx_gjk_cache.h"

static float from_bits(uint32_t b) {
  float v;
  memcpy(&v, &b, 4);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "constants")) {
    printf("{\"slots\": %d, \"words\": %d, \"margin\": %.9g}\n", MMX_AXIS_SLOTS, MMX_AXIS_WORDS, (double)MMX_AXIS_MARGIN);
    return 0;
  }
  if (!strcmp(argv[1], "verdict")) {
    int tag, pair;
    unsigned b[6];
    while (scanf("%d %d %x %x %x %x %x %x", &tag, &pair, &b[0], &b[1], &b[2], &b[3], &b[4], &b[5]) == 8)
      printf("%d\n", gjkc_separated(tag, pair, from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), from_bits(b[3]),
                                    from_bits(b[4]), from_bits(b[5])) ? 1 : 0);
    return 0;
  }
  if (!strcmp(argv[1], "slots") && argc == 4) {
    uint64_t s = strtoull(argv[2], nullptr, 10) * 2 + 1;
    const int n = atoi(argv[3]);
    std::vector<float> table(MMX_AXIS_SLOTS * MMX_AXIS_WORDS, 0.f);  // exactly the env's table
    for (int k = 0; k < n; k++) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      // every bit pattern of the masks' 32 bits (bits above the table included: the policy must ignore them),
      // and pair indices over the whole int range
      const unsigned hit = (k % 3 == 0) ? 0u : (unsigned)(s >> 32) & (unsigned)(s >> 7);
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const unsigned busy = (k % 5 == 0) ? 0xffffffffu : (unsigned)(s >> 32);
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const int pair = (k % 7 == 0) ? (int)(s >> 33) : (int)((s >> 40) % 780);
      const int slot = gjkc_slot(hit, busy, pair);
      if (slot >= 0) table.data()[MMX_AXIS_WORDS * slot + 3] = 1.f;  // the last word of the entry
      printf("{\"hit\": %u, \"busy\": %u, \"pair\": %d, \"slot\": %d}\n", hit, busy, pair, slot);
    }
    return 0;
  }
  return 2;
}

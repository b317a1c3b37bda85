// Host-side seeding: numpy's SeedSequence / PCG64 initialisation restated (the reference seeds every
// episode through gymnasium: Generator(PCG64(SeedSequence(seed))), gym_env.py:491), so the device PCG64
// streams are bit-identical to the reference's np_random streams.  Host code only, no HIP:
// tests/host/mmx_host_selftest.cpp runs it under the sanitizers against numpy.
#ifndef MMX_SEED_H
#define MMX_SEED_H
#include <stdint.h>

#include <vector>

namespace mmx_host {

constexpr uint32_t kInitA = 0x43b0d7e5u, kMultA = 0x931e8875u, kInitB = 0x8b51f9ddu, kMultB = 0x58f38dedu;
constexpr uint32_t kMixL = 0xca01f9ddu, kMixR = 0x4973f715u;

inline uint32_t hashmix(uint32_t v, uint32_t& hc) {
  v ^= hc;
  hc *= kMultA;
  v *= hc;
  v ^= v >> 16;
  return v;
}
inline uint32_t mix(uint32_t x, uint32_t y) {
  uint32_t r = kMixL * x - kMixR * y;
  return r ^ (r >> 16);
}
inline std::vector<uint32_t> seed_words(uint64_t s) {
  std::vector<uint32_t> w{static_cast<uint32_t>(s)};
  if (s >> 32) w.push_back(static_cast<uint32_t>(s >> 32));
  return w;
}
// SeedSequence(entropy, spawn_key).generate_state(n_out, uint32)
inline std::vector<uint32_t> seedseq(std::vector<uint32_t> ent, const std::vector<uint32_t>& spawn, int n_out) {
  if (!spawn.empty() && ent.size() < 4) ent.resize(4, 0u);
  ent.insert(ent.end(), spawn.begin(), spawn.end());
  uint32_t pool[4];
  uint32_t hc = kInitA;
  for (int i = 0; i < 4; i++) pool[i] = hashmix(i < static_cast<int>(ent.size()) ? ent[i] : 0u, hc);
  for (int s = 0; s < 4; s++)
    for (int d = 0; d < 4; d++)
      if (s != d) pool[d] = mix(pool[d], hashmix(pool[s], hc));
  for (size_t s = 4; s < ent.size(); s++)
    for (int d = 0; d < 4; d++) pool[d] = mix(pool[d], hashmix(ent[s], hc));
  std::vector<uint32_t> out(n_out);
  uint32_t hb = kInitB;
  for (int i = 0; i < n_out; i++) {
    uint32_t v = pool[i % 4];
    v ^= hb;
    hb *= kMultB;
    v *= hb;
    v ^= v >> 16;
    out[i] = v;
  }
  return out;
}
// SeedSequence(root).spawn(n)[index].generate_state(1)[0] (mmx_episode_seed)
inline uint32_t episode_seed(uint64_t root, int32_t index) {
  return seedseq(seed_words(root), {static_cast<uint32_t>(index)}, 1)[0];
}

using u128 = unsigned __int128;

// PCG64(SeedSequence(seed)) initial (state hi, state lo, inc hi, inc lo)
inline void pcg64_seed(uint64_t seed, uint64_t out[4]) {
  const u128 mult = (static_cast<u128>(0x2360ED051FC65DA4ull) << 64) | 0x4385DF649FCCF645ull;
  std::vector<uint32_t> st = seedseq(seed_words(seed), {}, 8);
  uint64_t v[4];
  for (int i = 0; i < 4; i++) v[i] = static_cast<uint64_t>(st[2 * i]) | (static_cast<uint64_t>(st[2 * i + 1]) << 32);
  u128 initstate = (static_cast<u128>(v[0]) << 64) | v[1];
  u128 initseq = (static_cast<u128>(v[2]) << 64) | v[3];
  u128 inc = (initseq << 1) | 1;
  u128 s = 0;
  s = s * mult + inc;
  s += initstate;
  s = s * mult + inc;
  out[0] = static_cast<uint64_t>(s >> 64);
  out[1] = static_cast<uint64_t>(s);
  out[2] = static_cast<uint64_t>(inc >> 64);
  out[3] = static_cast<uint64_t>(inc);
}
// the same into one row of a device-layout rng array (MMXState::rng: [n][4])
inline void pcg64_seed_row(unsigned long long* dst, uint64_t seed) {
  uint64_t st[4];
  pcg64_seed(seed, st);
  for (int k = 0; k < 4; k++) dst[k] = st[k];
}

}  // namespace mmx_host

#endif

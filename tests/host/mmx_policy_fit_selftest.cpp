// The closed forms of the policy's training step (csrc/mmx_policy_fit.h: the code the kernels run) on the host: a
// stand-alone program for tests/test_policy_fit_host.py, built with g++ and the sanitizers.  One JSON line per
// result; floats travel as their bit patterns.
//   step <case file>   one policy_fit_step_ref on a blob of exactly the computed size: the loss, every layer's
//                      weights and biases afterwards (torch layout), the count of padding entries that are not 0
//                      and of entries outside the layers that changed
//   adam w g m v t lr beta1 beta2 eps ...   (bit patterns, t an integer) -> w, m, v after one Adam update
//   index shuffle seed k B n                 -> the batch's pair indices
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../mujoco_manip_amd/csrc/mmx_policy_fit.h"

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static std::vector<float> read_floats(std::ifstream& in, size_t n) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; i++) {
    uint32_t u;
    in >> u;
    v[i] = from_bits(u);
  }
  return v;
}
static void print_words(const char* name, const std::vector<float>& v) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) printf("%s%" PRIu32, i ? "," : "", bits(v[i]));
  printf("]");
}

static int run_step(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  MmxPolicy P{};
  int B, shuffle, optimizer;
  int64_t n;
  uint64_t seed, k, t;
  uint32_t lr, b1, b2, eps;
  in >> P.n_layers >> P.activation >> B >> n >> shuffle >> seed >> k >> optimizer >> lr >> b1 >> b2 >> eps >> t;
  for (int l = 0; l < P.n_layers; l++) in >> P.out[l], P.in[l] = l ? P.out[l - 1] : POLICY_NOBS;
  P.A = P.out[P.n_layers - 1];
  std::vector<std::vector<float>> W((size_t)P.n_layers), Bv((size_t)P.n_layers);
  const float* wp[POLICY_MAX_LAYERS] = {};
  const float* bp[POLICY_MAX_LAYERS] = {};
  for (int l = 0; l < P.n_layers; l++) {
    int has_bias;
    in >> has_bias;
    W[(size_t)l] = read_floats(in, (size_t)P.out[l] * (size_t)P.in[l]);
    if (has_bias) Bv[(size_t)l] = read_floats(in, (size_t)P.out[l]);
    wp[l] = W[(size_t)l].data();
    bp[l] = has_bias ? Bv[(size_t)l].data() : nullptr;
  }
  const std::vector<float> shift = read_floats(in, POLICY_NOBS), scale = read_floats(in, POLICY_NOBS);
  const std::vector<float> obs = read_floats(in, (size_t)n * POLICY_NOBS), target = read_floats(in, (size_t)n * (size_t)P.A);
  if (!in) return 3;
  std::vector<float> blob(policy_layout(P));
  policy_pack(P, wp, bp, shift.data(), scale.data(), nullptr, nullptr, nullptr, blob.data());
  const std::vector<float> before = blob;
  std::vector<float> m(policy_fit_param_floats(P), 0.f), v(policy_fit_param_floats(P), 0.f);
  const MmxFitOpt opt = policy_fit_opt(optimizer, from_bits(lr), from_bits(b1), from_bits(b2), from_bits(eps), t);
  const float loss = policy_fit_step_ref(P, blob.data(), obs.data(), target.data(), n, B, shuffle, seed, k, opt, m.data(), v.data());
  long pad_nonzero = 0, outside_changed = 0;
  for (int l = 0; l < P.n_layers; l++)
    for (int c = 0; c <= P.in[l]; c++)
      for (int j = P.out[l]; j < policy_padded(P.out[l]); j++) pad_nonzero += bits(blob[(size_t)P.woff[l] + policy_windex(P.out[l], c, j)]) != 0u;
  for (size_t i = policy_fit_param_floats(P); i < blob.size(); i++) outside_changed += bits(blob[i]) != bits(before[i]);
  printf("{\"loss\": %" PRIu32 ", \"pad_nonzero\": %ld, \"outside_changed\": %ld, \"floats\": %zu, \"layers\": [", bits(loss), pad_nonzero,
         outside_changed, blob.size());
  for (int l = 0; l < P.n_layers; l++) {
    std::vector<float> w((size_t)P.out[l] * (size_t)P.in[l]), b((size_t)P.out[l]);
    for (int j = 0; j < P.out[l]; j++) {
      for (int c = 0; c < P.in[l]; c++) w[(size_t)j * (size_t)P.in[l] + (size_t)c] = blob[(size_t)P.woff[l] + policy_windex(P.out[l], c, j)];
      b[(size_t)j] = blob[(size_t)P.boff[l] + (size_t)j];
    }
    printf("%s{", l ? ", " : "");
    print_words("W", w);
    printf(", ");
    print_words("b", b);
    printf("}");
  }
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "step" && argc == 3) return run_step(argv[2]);
  if (mode == "adam" && (argc - 2) % 9 == 0) {
    for (int i = 2; i < argc; i += 9) {
      auto word = [&](int q) { return from_bits((uint32_t)strtoul(argv[i + q], nullptr, 10)); };
      float m = word(2), v = word(3);
      const MmxFitOpt o = policy_fit_opt(FIT_ADAM, word(5), word(6), word(7), word(8), strtoull(argv[i + 4], nullptr, 10));
      const float w = policy_fit_update(word(0), word(1), &m, &v, o);
      printf("{\"w\": %" PRIu32 ", \"m\": %" PRIu32 ", \"v\": %" PRIu32 "}\n", bits(w), bits(m), bits(v));
    }
    return 0;
  }
  if (mode == "index" && argc == 7) {
    const int shuffle = atoi(argv[2]);
    const uint64_t seed = strtoull(argv[3], nullptr, 10), k = strtoull(argv[4], nullptr, 10);
    const uint32_t B = (uint32_t)strtoul(argv[5], nullptr, 10);
    const int64_t n = strtoll(argv[6], nullptr, 10);
    printf("{\"index\": [");
    for (uint32_t s = 0; s < B; s++)
      printf("%s%" PRId64, s ? "," : "", policy_fit_index(shuffle, (uint32_t)seed, (uint32_t)(seed >> 32), k, s, B, n));
    printf("]}\n");
    return 0;
  }
  return 2;
}

// The closed forms of the policy-gradient fit (csrc/mmx_pg.h: the code the kernels run) on the host: a stand-alone
// program for tests/test_pg_host.py, built with g++ and the sanitizers.  One JSON line per result; floats travel as
// their bit patterns.
//   step <case file>   one policy_pg_step_ref on a blob of exactly the computed size: the three statistics, every
//                      layer's weights and biases afterwards (torch layout), the count of padding entries that are
//                      not 0 and of entries outside the layers that changed.  The file is mmx_policy_fit_selftest's
//                      (mean_old where it has the targets) with log_std [A], noise [n][A], adv [n] and clip behind it
//   gae <case file>    T N normalize gamma lambda, then reward [T][N], done [T][N][3] (integers), value [T][N],
//                      value_last [N] -> adv, ret of pg_gae_ref (and pg_normalise_ref)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../mujoco_manip_amd/csrc/mmx_pg.h"

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
  const std::vector<float> obs = read_floats(in, (size_t)n * POLICY_NOBS), mean_old = read_floats(in, (size_t)n * (size_t)P.A);
  const std::vector<float> log_std = read_floats(in, (size_t)P.A), noise = read_floats(in, (size_t)n * (size_t)P.A);
  const std::vector<float> adv = read_floats(in, (size_t)n), clip = read_floats(in, 1);
  if (!in) return 3;
  std::vector<float> blob(policy_layout(P));
  policy_pack(P, wp, bp, shift.data(), scale.data(), log_std.data(), nullptr, nullptr, blob.data());
  const std::vector<float> before = blob;
  std::vector<float> m(policy_fit_param_floats(P), 0.f), v(policy_fit_param_floats(P), 0.f), stats(3);
  const MmxFitOpt opt = policy_fit_opt(optimizer, from_bits(lr), from_bits(b1), from_bits(b2), from_bits(eps), t);
  policy_pg_step_ref(P, blob.data(), obs.data(), mean_old.data(), noise.data(), adv.data(), n, B, shuffle, seed, k, clip[0], opt,
                     m.data(), v.data(), stats.data());
  long pad_nonzero = 0, outside_changed = 0;
  for (int l = 0; l < P.n_layers; l++)
    for (int c = 0; c <= P.in[l]; c++)
      for (int j = P.out[l]; j < policy_padded(P.out[l]); j++) pad_nonzero += bits(blob[(size_t)P.woff[l] + policy_windex(P.out[l], c, j)]) != 0u;
  for (size_t i = policy_fit_param_floats(P); i < blob.size(); i++) outside_changed += bits(blob[i]) != bits(before[i]);
  printf("{");
  print_words("stats", stats);
  printf(", \"pad_nonzero\": %ld, \"outside_changed\": %ld, \"layers\": [", pad_nonzero, outside_changed);
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

static int run_gae(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  int T, N, normalize;
  uint32_t gamma, lambda;
  in >> T >> N >> normalize >> gamma >> lambda;
  const size_t n = (size_t)T * (size_t)N;
  const std::vector<float> reward = read_floats(in, n);
  std::vector<int32_t> done(3 * n);
  for (int32_t& d : done) in >> d;
  const std::vector<float> value = read_floats(in, n), value_last = read_floats(in, (size_t)N);
  if (!in) return 3;
  std::vector<float> adv(n), ret(n);
  pg_gae_ref(from_bits(gamma), from_bits(lambda), T, N, reward.data(), done.data(), value.data(), value_last.data(), adv.data(), ret.data());
  if (normalize) pg_normalise_ref(adv.data(), (int64_t)n);
  printf("{");
  print_words("adv", adv);
  printf(", ");
  print_words("ret", ret);
  printf("}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string mode = argv[1];
  if (mode == "step") return run_step(argv[2]);
  if (mode == "gae") return run_gae(argv[2]);
  return 2;
}

// Stand-alone host program over csrc/mmx_policy.h, the closed forms the MLP policy's kernels run (built by
// tests/test_policy_host.py with g++ and AddressSanitizer + UndefinedBehaviorSanitizer, run as a child process).
// It prints JSON lines that the test compares with its own fp64 restatements:
//   mmx_policy_selftest pack                     the packed layout of one layer per (inputs, width) pair: every weight
//                                                found at policy_windex, the padding zero, in a blob of exactly
//                                                policy_layout floats (a read or write past it is the sanitizer's)
//   mmx_policy_selftest forward FILE             policy_forward_ref of the case in FILE (text: n_layers activation
//                                                rows, the widths, per layer has_bias + weights [out][in] (+ bias),
//                                                shift [85], scale [85], obs [rows][85]); the means as bit patterns
//   mmx_policy_selftest tanh x...                policy_tanh of each argument, as bit patterns
//   mmx_policy_selftest action (mean std z lo hi)...   policy_action of each group of five, as bit patterns
// Exit status 1: a layout check fails, or a file cannot be read.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mujoco_manip_amd/csrc/mmx_policy.h"

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

static int pack() {
  const int widths[] = {1, 63, 64, 65, 256}, inputs[] = {1, POLICY_NOBS, 256};
  int bad = 0;
  for (int in : inputs)
    for (int out : widths) {
      MmxPolicy P{};
      P.n_layers = 1, P.in[0] = in, P.out[0] = out, P.A = out < POLICY_MAX_ADIM ? out : POLICY_MAX_ADIM;
      const size_t n = policy_layout(P);
      std::vector<float> W((size_t)in * out), b(out), blob(n, -1.f);
      for (int j = 0; j < out; j++) {
        b[j] = -(float)(j + 2);  // (never the blob's fill value -1)
        for (int k = 0; k < in; k++) W[(size_t)j * in + k] = (float)(j * 1000 + k + 1);
      }
      const float* wp[POLICY_MAX_LAYERS] = {W.data()};
      const float* bp[POLICY_MAX_LAYERS] = {b.data()};
      policy_pack(P, wp, bp, nullptr, nullptr, nullptr, nullptr, nullptr, blob.data());
      const int outp = policy_padded(out);
      int wrong = 0;
      for (int k = 0; k < in; k++)
        for (int j = 0; j < outp; j++) {
          const size_t at = (size_t)P.woff[0] + policy_windex(out, k, j);
          wrong += at >= (size_t)P.boff[0] || blob[at] != (j < out ? W[(size_t)j * in + k] : 0.f);
        }
      for (int j = 0; j < outp; j++) wrong += blob[(size_t)P.boff[0] + j] != (j < out ? b[j] : 0.f);
      for (int k = 0; k < POLICY_NOBS; k++) wrong += blob[P.shift_off + k] != 0.f || blob[P.scale_off + k] != 1.f;
      for (int a = 0; a < POLICY_MAX_ADIM; a++)
        wrong += blob[P.std_off + a] != 0.f || blob[P.low_off + a] != -FLT_MAX || blob[P.high_off + a] != FLT_MAX;
      for (float v : blob) wrong += v == -1.f;  // every float of the blob was written
      // the last row a lane reads: neuron outp - 1 of input in - 1 lies inside the layer's weights
      wrong += policy_windex(out, in - 1, outp - 1) + 1 != (size_t)in * outp;
      // a neuron through the packed layout
      std::vector<float> x(in);
      for (int k = 0; k < in; k++) x[k] = k % 2 ? 0.5f : -0.25f;
      const int j = out - 1;
      float acc = b[j];
      for (int k = 0; k < in; k++) acc = fmaf(W[(size_t)j * in + k], x[k], acc);
      wrong += policy_neuron(blob.data() + P.woff[0], out, in, j, blob[P.boff[0] + j], x.data()) != acc;
      printf("{\"kind\": \"pack\", \"in\": %d, \"out\": %d, \"padded\": %d, \"floats\": %zu, \"layer_floats\": %zu, \"wrong\": %d}\n", in,
             out, outp, n, policy_layer_floats(in, out), wrong);
      bad |= wrong != 0;
    }
  return bad;
}

static bool read_n(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  for (size_t k = 0; k < n; k++)
    if (fscanf(f, "%f", &v[k]) != 1) return false;
  return true;
}

static int forward(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 1;
  MmxPolicy P{};
  int rows = 0;
  bool ok = fscanf(f, "%d %d %d", &P.n_layers, &P.activation, &rows) == 3 && P.n_layers >= 1 && P.n_layers <= POLICY_MAX_LAYERS &&
            rows >= 1;
  std::vector<float> W[POLICY_MAX_LAYERS], b[POLICY_MAX_LAYERS], shift, scale, obs;
  const float* wp[POLICY_MAX_LAYERS] = {};
  const float* bp[POLICY_MAX_LAYERS] = {};
  for (int l = 0; ok && l < P.n_layers; l++) {
    ok = fscanf(f, "%d", &P.out[l]) == 1 && P.out[l] >= 1 && P.out[l] <= POLICY_MAX_WIDTH;
    P.in[l] = l ? P.out[l - 1] : POLICY_NOBS;
  }
  for (int l = 0; ok && l < P.n_layers; l++) {
    int has_bias = 0;
    ok = fscanf(f, "%d", &has_bias) == 1 && read_n(f, W[l], (size_t)P.out[l] * P.in[l]) && (!has_bias || read_n(f, b[l], P.out[l]));
    wp[l] = W[l].data();
    bp[l] = has_bias ? b[l].data() : nullptr;
  }
  ok = ok && read_n(f, shift, POLICY_NOBS) && read_n(f, scale, POLICY_NOBS) && read_n(f, obs, (size_t)rows * POLICY_NOBS);
  fclose(f);
  if (!ok || P.out[P.n_layers - 1] > POLICY_MAX_ADIM) return 1;
  P.A = P.out[P.n_layers - 1];
  std::vector<float> blob(policy_layout(P)), buf(2 * POLICY_MAX_WIDTH + POLICY_NOBS), mean((size_t)rows * P.A);
  policy_pack(P, wp, bp, shift.data(), scale.data(), nullptr, nullptr, nullptr, blob.data());
  for (int r = 0; r < rows; r++)
    policy_forward_ref(P, blob.data(), obs.data() + (size_t)r * POLICY_NOBS, mean.data() + (size_t)r * P.A, buf.data());
  printf("{\"kind\": \"forward\", \"rows\": %d, \"A\": %d, \"mean\": [", rows, P.A);
  for (size_t k = 0; k < mean.size(); k++) printf("%s%" PRIu32, k ? ", " : "", bits(mean[k]));
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "pack")) return pack();
  if (argc == 3 && !strcmp(argv[1], "forward")) return forward(argv[2]);
  if (argc >= 2 && !strcmp(argv[1], "tanh")) {
    for (int k = 2; k < argc; k++) {
      const float x = strtof(argv[k], nullptr);
      printf("{\"kind\": \"tanh\", \"x\": %.9g, \"y\": %" PRIu32 "}\n", (double)x, bits(policy_tanh(x)));
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "action")) {
    for (int k = 2; k + 4 < argc; k += 5) {
      float v[5];
      for (int j = 0; j < 5; j++) v[j] = strtof(argv[k + j], nullptr);
      printf("{\"kind\": \"action\", \"y\": %" PRIu32 "}\n", bits(policy_action(v[0], v[1], v[2], v[3], v[4])));
    }
    return 0;
  }
  fprintf(stderr, "usage: mmx_policy_selftest pack | forward FILE | tanh x... | action (mean std z lo hi)...\n");
  return 2;
}

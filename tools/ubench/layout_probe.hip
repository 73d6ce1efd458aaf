// Developer probe (tools/features_bench.py builds and runs it): FeatureLayoutKernel's one launch for a batch, with
// hipEvents around the launch alone.  (The kernel it replaced, one launch per utterance, is gone from the library; the
// comparison with it is recorded in profiles/features_layout.json.)  Linked against the library's own kernel unit:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I pocketkaldi_amd/csrc -I include tools/ubench/layout_probe.hip \
//         pocketkaldi_amd/csrc/features.hip -o tools/ubench/layout_probe
//   tools/ubench/layout_probe [utts 256] [frames 998] [dim 40] [left 5] [right 5] [reps 20]
// Prints one JSON object: the median in microseconds, the traffic floor, and whether Yt is the padded transpose.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "pk_score.h"

#define CHECK(e)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (e);                                                               \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); return 1; } \
  } while (0)

static float Median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  const int U = argc > 1 ? atoi(argv[1]) : 256, T = argc > 2 ? atoi(argv[2]) : 998, D = argc > 3 ? atoi(argv[3]) : 40;
  const int L = argc > 4 ? atoi(argv[4]) : 5, R = argc > 5 ? atoi(argv[5]) : 5, reps = argc > 6 ? atoi(argv[6]) : 20;
  if (U <= 0 || T <= 0 || D <= 0 || L < 0 || R < 0 || reps <= 0) { fprintf(stderr, "bad arguments\n"); return 2; }
  const int64_t cols = (int64_t)U * (T + L + R), ldy = (cols + 255) / 256 * 256;
  std::vector<float> feats((size_t)U * T * D);
  for (size_t i = 0; i < feats.size(); ++i) feats[i] = (float)(int)(i % 8191) - 4095.0f;
  std::vector<int64_t> raw_base(U), pad_base(U), wave_off(U, 0);
  std::vector<int32_t> frames(U, T);
  for (int u = 0; u < U; ++u) { raw_base[u] = (int64_t)u * T; pad_base[u] = (int64_t)u * (T + L + R); }
  float *d_feats, *d_a;
  int64_t *d_raw, *d_pad, *d_woff;
  int32_t *d_T;
  CHECK(hipMalloc(&d_feats, sizeof(float) * feats.size()));
  CHECK(hipMalloc(&d_a, sizeof(float) * ldy * D));
  CHECK(hipMalloc(&d_raw, sizeof(int64_t) * U));
  CHECK(hipMalloc(&d_pad, sizeof(int64_t) * U));
  CHECK(hipMalloc(&d_woff, sizeof(int64_t) * U));
  CHECK(hipMalloc(&d_T, sizeof(int32_t) * U));
  CHECK(hipMemcpy(d_feats, feats.data(), sizeof(float) * feats.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_raw, raw_base.data(), sizeof(int64_t) * U, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_pad, pad_base.data(), sizeof(int64_t) * U, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_woff, wave_off.data(), sizeof(int64_t) * U, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_T, frames.data(), sizeof(int32_t) * U, hipMemcpyHostToDevice));
  CHECK(hipMemset(d_a, 0, sizeof(float) * ldy * D));
  hipStream_t s;
  hipEvent_t e0, e1;
  CHECK(hipStreamCreate(&s));
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const pkmi::UttLayout lay{d_woff, d_T, d_raw, d_pad};
  auto one = [&] { pkmi::LaunchFeatureLayout(d_feats, lay, U, T, D, L, R, d_a, ldy, s); };
  std::vector<float> t_one;
  for (int i = 0; i < 3 + reps; ++i) {                      // three warm-up rounds
    float ms = 0;
    CHECK(hipEventRecord(e0, s));
    one();
    CHECK(hipEventRecord(e1, s));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (i >= 3) t_one.push_back(ms * 1000.0f);
  }
  CHECK(hipGetLastError());
  std::vector<float> a((size_t)ldy * D), b((size_t)ldy * D, 0.0f);
  CHECK(hipMemcpy(a.data(), d_a, sizeof(float) * a.size(), hipMemcpyDeviceToHost));
  for (int u = 0; u < U; ++u)                               // the padded transpose on the host (am.cc:73-75)
    for (int d = 0; d < D; ++d)
      for (int c = 0; c < T + L + R; ++c)
        b[(size_t)d * ldy + pad_base[u] + c] = feats[(size_t)(raw_base[u] + std::min(std::max(c - L, 0), T - 1)) * D + d];
  const bool same = memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0;
  const double bytes = 2.0 * 4.0 * D * (double)U * T, floor_us = bytes / 8e12 * 1e6;
  printf("{\"utts\": %d, \"frames\": %d, \"dim\": %d, \"left\": %d, \"right\": %d, \"reps\": %d, "
         "\"feature_layout_us\": %.3f, \"feature_layout_min_us\": %.3f, \"traffic_bytes\": %.0f, \"floor_us_at_8TBps\": %.3f, "
         "\"achieved_GBps\": %.1f, \"same_yt\": %s}\n",
         U, T, D, L, R, reps, Median(t_one), *std::min_element(t_one.begin(), t_one.end()), bytes, floor_us,
         bytes / (Median(t_one) * 1e-6) / 1e9, same ? "true" : "false");
  return same ? 0 : 3;
}

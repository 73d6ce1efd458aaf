// capi_resample.hip -- the host side of the resampler (pk_resample.h): a rate's table on the device, the checked plan
// upload and launch every converting object goes through, and the single-wave entry pk_mi355_resample.
#include <hip/hip_runtime.h>

#include <vector>

#include "pk_host.h"
#include "pk_resample.h"

using namespace pkmi;
using namespace pkhost;

namespace pkhost {

int Resampler::Table(int rate, const DeviceResampleTable **out) {
  for (const DeviceResampleTable *t : tables)
    if (t->host.rate == rate) { *out = t; return 0; }
  DeviceResampleTable *t = new DeviceResampleTable();
  auto failed = [&](int rc) {
    hipFree(t->d_first); hipFree(t->d_count); hipFree(t->d_weights);
    delete t;
    return rc;
  };
  if (BuildResampleTable(rate, &t->host))
    return failed(Fail(PK_MI355_E_INVALID, "sample rate %d is not supported: 8000 .. 96000 Hz with a polyphase table of at most %d entries",
                       rate, kResampleMaxEntries));
  const ResampleTable &h = t->host;
  // what the kernel indexes with: every window inside [min_first, max_end), every count within a weight row
  for (int p = 0; p < h.P; ++p)
    if (h.count[p] < 0 || h.count[p] > h.max_taps || h.first[p] < h.min_first || h.first[p] + h.count[p] > h.max_end)
      return failed(Fail(PK_MI355_E_INVALID, "internal: resample table of rate %d: phase %d out of range", rate, p));
  hipError_t e = hipMalloc(&t->d_first, sizeof(int32_t) * h.P);
  if (e == hipSuccess) e = hipMalloc(&t->d_count, sizeof(int32_t) * h.P);
  if (e == hipSuccess) e = hipMalloc(&t->d_weights, sizeof(float) * h.weights.size());
  if (e == hipSuccess) e = hipMemcpy(t->d_first, h.first.data(), sizeof(int32_t) * h.P, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(t->d_count, h.count.data(), sizeof(int32_t) * h.P, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(t->d_weights, h.weights.data(), sizeof(float) * h.weights.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return failed(Fail(PK_MI355_E_DEVICE, "resample table: %s", hipGetErrorString(e)));
  tables.push_back(t);
  *out = t;
  return 0;
}

ResampleItem Resampler::Item(const DeviceResampleTable &t, const float *x, int64_t x0, int64_t n_valid, int64_t j0, int64_t j1, float *y) {
  const ResampleTable &h = t.host;
  return ResampleItem{x, x0, n_valid, j0, j1, y, t.d_first, t.d_count, t.d_weights, h.Q, h.P, h.max_taps, h.min_first, h.max_end, h.Span()};
}

int Resampler::Run(const std::vector<ResampleItem> &items, hipStream_t stream) {
  const int n = (int)items.size();
  if (n == 0) return 0;
  size_t lds = 0;
  int64_t max_tiles = 0;
  for (const ResampleItem &it : items) {
    const DeviceResampleTable *t = nullptr;
    for (const DeviceResampleTable *c : tables)
      if (c->d_weights == it.weights) t = c;
    if (!t || it.first != t->d_first || it.count != t->d_count || it.Q != t->host.Q || it.P != t->host.P ||
        it.max_taps != t->host.max_taps || it.min_first != t->host.min_first || it.max_end != t->host.max_end || it.span != t->host.Span())
      return Fail(PK_MI355_E_INVALID, "internal: resample plan without a table of this object");
    if (it.j0 < 0 || it.j1 < it.j0 || it.n_valid < 0 || (it.n_valid > 0 && !it.x) || (it.j1 > it.j0 && !it.y))
      return Fail(PK_MI355_E_INVALID, "internal: resample plan out of range");
    lds = std::max(lds, ResampleLdsBytes(it.P, it.max_taps, it.span));
    max_tiles = std::max<int64_t>(max_tiles, (it.j1 - it.j0 + kResampleTile - 1) / kResampleTile);
  }
  if (max_tiles == 0) return 0;
  if (lds > lds_allowed) {
    if (lds > 160 * 1024 || ResampleAllowLds(lds) != 0) return Fail(PK_MI355_E_DEVICE, "resample: %zu bytes of LDS are not available", lds);
    lds_allowed = lds;
  }
  if (!uploaded) HIP_TRY(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
  else HIP_TRY(hipEventSynchronize(uploaded));       // the previous launch's plan has left h_items
  if (n > items_cap) {
    if (h_items) hipHostFree(h_items);
    hipFree(d_items);
    h_items = nullptr; d_items = nullptr; items_cap = 0;
    const int cap = std::max(n, 64);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_items), sizeof(ResampleItem) * cap, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&d_items, sizeof(ResampleItem) * cap));
    items_cap = cap;
  }
  memcpy(h_items, items.data(), sizeof(ResampleItem) * n);
  HIP_TRY(hipMemcpyAsync(d_items, h_items, sizeof(ResampleItem) * n, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(uploaded, stream));
  constexpr int kMaxGridY = 32768;
  for (int at = 0; at < n; at += kMaxGridY) {
    LaunchResample(d_items + at, std::min(kMaxGridY, n - at), max_tiles, lds, stream);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

void Resampler::Free() {
  for (DeviceResampleTable *t : tables) {
    hipFree(t->d_first); hipFree(t->d_count); hipFree(t->d_weights);
    delete t;
  }
  tables.clear();
  if (h_items) hipHostFree(h_items);
  hipFree(d_items);
  if (uploaded) hipEventDestroy(uploaded);
  h_items = nullptr; d_items = nullptr; uploaded = nullptr; items_cap = 0;
}

}  // namespace pkhost

extern "C" {

int pk_mi355_resample(const pk_vector_t *wave, int rate, pk_vector_t *out) {
  if (!wave || !out || wave->dim < 0 || (wave->dim > 0 && !wave->data)) return Fail(PK_MI355_E_INVALID, "null argument");
  ResampleTable plan;
  if (BuildResampleTable(rate, &plan))
    return Fail(PK_MI355_E_INVALID, "sample rate %d is not supported: 8000 .. 96000 Hz with a polyphase table of at most %d entries", rate,
                kResampleMaxEntries);
  const int64_t n_out = ResampleNumOutput(plan, wave->dim);
  if (n_out > INT32_MAX) return Fail(PK_MI355_E_INVALID, "resample: %lld output samples do not fit a pk_vector_t", (long long)n_out);
  float *host = static_cast<float *>(realloc(out->data, sizeof(float) * (n_out > 0 ? n_out : 1)));
  if (!host) return Fail(PK_MI355_E_INVALID, "out of host memory");
  out->data = host;
  out->dim = (int)n_out;
  if (n_out == 0) return 0;
  if (rate == kResampleOutRate) {                      // the identity: nothing is launched
    memcpy(host, wave->data, sizeof(float) * n_out);
    return 0;
  }
  int rc = UseDevice(CurrentDevice());
  if (rc) return rc;
  Resampler rs;
  float *d_x = nullptr, *d_y = nullptr;
  auto run = [&]() -> int {
    const DeviceResampleTable *t = nullptr;
    if (int r = rs.Table(rate, &t)) return r;
    HIP_TRY(hipMalloc(&d_x, sizeof(float) * wave->dim));
    HIP_TRY(hipMalloc(&d_y, sizeof(float) * n_out));
    HIP_TRY(hipMemcpy(d_x, wave->data, sizeof(float) * wave->dim, hipMemcpyHostToDevice));
    if (int r = rs.Run({Resampler::Item(*t, d_x, 0, wave->dim, 0, n_out, d_y)}, nullptr)) return r;
    HIP_TRY(hipMemcpy(host, d_y, sizeof(float) * n_out, hipMemcpyDeviceToHost));
    return 0;
  };
  rc = run();
  hipFree(d_x); hipFree(d_y);
  rs.Free();
  return rc;
}

}  // extern "C"

// capi_io.hip -- model files to a device model (the readers are pk_files.cc), Fbank::Compute / CMVN for one
// utterance, and the parity-test hooks.
#include <hip/hip_runtime.h>

#include <vector>

#include "pk_frontend.h"
#include "pk_host.h"

using namespace pkmi;
using namespace pkhost;

namespace {
// pk_mi355_am_read.  files_fit: called with the first linear layer's input width once every file is read
// and before the model -- and with it the device -- is touched; its code, if not 0, is the entry's.
template <class FilesFit>
int AmRead(pk_mi355_am_t *am, const char *nnet_path, const char *prior_path, const char *tid2pdf_path, int left_context, int right_context,
           int num_pdfs, FilesFit files_fit) {
  if (!am || am->finalized) return Fail(PK_MI355_E_STATE, "model already finalized");
  std::vector<HostLayer> layers;
  std::vector<float> prior;
  std::vector<int32_t> tid;
  int rc;
  if ((rc = ReadNnet(nnet_path, &layers)) || (rc = ReadVec(prior_path, &prior)) ||
      (tid2pdf_path && (rc = ReadVec(tid2pdf_path, &tid))))
    return rc;
  if ((int)prior.size() != num_pdfs)
    return Fail(PK_MI355_E_INVALID, "prior has %d entries, num_pdfs = %d", (int)prior.size(), num_pdfs);
  for (const HostLayer &L : layers)
    if (L.type == PK_NNET_LINEAR_LAYER) {
      if ((rc = files_fit(L.in_dim))) return rc;
      break;
    }
  for (const HostLayer &L : layers) {
    if (L.type == PK_NNET_LINEAR_LAYER) rc = pk_mi355_am_add_linear(am, L.in_dim, L.out_dim, L.W.data(), L.b.data());
    else if (L.type == PK_NNET_ADD_LAYER || L.type == PK_NNET_MUL_LAYER) rc = pk_mi355_am_add_vector_layer(am, L.type, L.in_dim, L.b.data());
    else if (L.type == PK_MI355_NNET_PNORM_LAYER) rc = pk_mi355_am_add_pnorm(am, L.in_dim, L.out_dim);
    else if (L.type == PK_MI355_NNET_TIME_SPLICE_LAYER) rc = pk_mi355_am_add_time_splice(am, L.in_dim, L.offsets.data(), (int)L.offsets.size());
    else rc = pk_mi355_am_add_layer(am, L.type);
    if (rc) return rc;
  }
  return pk_mi355_am_finalize(am, prior.data(), num_pdfs, left_context, right_context,
                              tid.empty() ? nullptr : tid.data(), (int)tid.size());
}
}  // namespace

extern "C" {

int pk_mi355_am_read(pk_mi355_am_t *am, const char *nnet_path, const char *prior_path,
                     const char *tid2pdf_path, int left_context, int right_context,
                     int num_pdfs) {
  return AmRead(am, nnet_path, prior_path, tid2pdf_path, left_context, right_context, num_pdfs, [](int) { return 0; });
}

// pk_load's share of this path (pocketkaldi.cc:72-144)
int pk_mi355_load(const char *config_path, int precision, pk_mi355_am_t **am_out, float *cmvn_stats41) {
  if (!config_path || !am_out || !cmvn_stats41) return Fail(PK_MI355_E_INVALID, "null argument");
  *am_out = nullptr;
  static_assert(kCmvnStats == kNumBins + 1, "one sum per mel bin and the frame count");
  ModelConfig conf;
  int rc = ReadModelConfig(config_path, &conf);
  if (rc) return rc;
  pk_mi355_am_t *am = pk_mi355_am_create();
  if (!am) return PK_MI355_E_DEVICE;
  if ((rc = pk_mi355_am_set_precision(am, precision)) ||
      (rc = pk_mi355_am_read(am, conf.nnet.c_str(), conf.prior.c_str(), conf.tid2pdf.c_str(), conf.left, conf.right,
                             conf.num_pdfs))) {
    pk_mi355_am_destroy(am);
    return rc;
  }
  memcpy(cmvn_stats41, conf.cmvn_stats, sizeof(conf.cmvn_stats));
  *am_out = am;
  return 0;
}

// pk_mi355_load for a model of any feature dimension: the statistics vector at the model's length
int pk_mi355_load_stats(const char *config_path, int precision, pk_mi355_am_t **am_out, float *stats, int stats_cap, int *stats_len) {
  return LoadStatsBlocks(config_path, precision, 1, am_out, stats, stats_cap, stats_len);
}

}  // extern "C"

// blocks: 1, or the order + 1 blocks of a deltas spec -- the statistics are then at feat_dim / blocks; 0: a transform
// stands in front of the model, the statistics are at the transform's base dimension and
// pk_mi355_transform_batch_create holds them to it
int pkhost::LoadStatsBlocks(const char *config_path, int precision, int blocks, pk_mi355_am_t **am_out, float *stats, int stats_cap,
                            int *stats_len) {
  if (!config_path || !am_out || !stats || !stats_len) return Fail(PK_MI355_E_INVALID, "null argument");
  *am_out = nullptr; *stats_len = 0;
  if (stats_cap <= 0) return Fail(PK_MI355_E_INVALID, "bad statistics capacity %d", stats_cap);
  ModelConfig conf;
  int rc = ReadModelConfigStats(config_path, stats_cap, &conf);
  if (rc) return rc;
  pk_mi355_am_t *am = pk_mi355_am_create();
  if (!am) return PK_MI355_E_DEVICE;
  // the statistics against the model's feature dimension -- the first layer's width over the spliced frames -- as soon as
  // the files are read (a width that is no multiple of the frames is the model's own refusal, at finalize)
  auto stats_fit = [&](int in_dim) {
    if (blocks == 0) return 0;
    const int frames = conf.left + conf.right + 1, feat_dim = in_dim / frames, dim = feat_dim / blocks;
    if (in_dim % frames != 0 || (int)conf.stats.size() == dim + 1) return 0;
    if (blocks > 1 && feat_dim % blocks != 0) return 0;      // (pk_mi355_deltas_batch_create's refusal, which names both numbers)
    if (blocks > 1)
      return Fail(PK_MI355_E_IO, "cmvn_stats in %s has %d entries, the %d-dim model of %s with %d delta blocks needs %d (the sums, then the count)",
                  conf.cmvn_path.c_str(), (int)conf.stats.size(), feat_dim, config_path, blocks, dim + 1);
    return Fail(PK_MI355_E_IO, "cmvn_stats in %s has %d entries, the %d-dim model of %s needs %d (the sums, then the count)", conf.cmvn_path.c_str(),
                (int)conf.stats.size(), dim, config_path, dim + 1);
  };
  if ((rc = pk_mi355_am_set_precision(am, precision)) ||
      (rc = AmRead(am, conf.nnet.c_str(), conf.prior.c_str(), conf.tid2pdf.c_str(), conf.left, conf.right, conf.num_pdfs, stats_fit))) {
    pk_mi355_am_destroy(am);
    return rc;
  }
  memcpy(stats, conf.stats.data(), sizeof(float) * conf.stats.size());
  *stats_len = (int)conf.stats.size();
  *am_out = am;
  return 0;
}

extern "C" {

int pk_mi355_test_logf(const float *x, int n, float *out) {
  if (!x || !out || n < 0) return Fail(PK_MI355_E_INVALID, "bad argument");
  int rc = UseDevice(CurrentDevice());
  if (rc || n == 0) return rc;
  FrontendTables host;
  if (BuildFrontendTables(&host)) return Fail(PK_MI355_E_INVALID, "front-end table construction failed");
  FrontendTables *d_tab = nullptr;
  float *d_x = nullptr, *d_y = nullptr;
  hipError_t e = hipMalloc(&d_tab, sizeof(host));
  if (e == hipSuccess) e = hipMalloc(&d_x, sizeof(float) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_y, sizeof(float) * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(d_tab, &host, sizeof(host), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_x, x, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    LaunchLogfTest(d_x, n, d_tab, d_y, nullptr);
    e = hipMemcpy(out, d_y, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
  }
  hipFree(d_tab); hipFree(d_x); hipFree(d_y);
  if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "test_logf: %s", hipGetErrorString(e));
  return 0;
}

int pk_mi355_test_srfft512(const float *frames, int num_frames, float *spectra) {
  if (!frames || !spectra || num_frames < 0) return Fail(PK_MI355_E_INVALID, "bad argument");
  int rc = UseDevice(CurrentDevice());
  if (rc || num_frames == 0) return rc;
  FrontendTables host;
  if (BuildFrontendTables(&host)) return Fail(PK_MI355_E_INVALID, "front-end table construction failed");
  const size_t bytes = sizeof(float) * (size_t)num_frames * kFftSize;
  FrontendTables *d_tab = nullptr;
  float *d_x = nullptr, *d_y = nullptr;
  hipError_t e = hipMalloc(&d_tab, sizeof(host));
  if (e == hipSuccess) e = hipMalloc(&d_x, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_y, bytes);
  if (e == hipSuccess) e = hipMemcpy(d_tab, &host, sizeof(host), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_x, frames, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    LaunchSrfft512Test(d_x, num_frames, d_tab, d_y, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(spectra, d_y, bytes, hipMemcpyDeviceToHost);
  hipFree(d_tab); hipFree(d_x); hipFree(d_y);
  if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "test_srfft512: %s", hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------ single-utterance front-end

int pk_mi355_fbank_compute(const pk_vector_t *wave, pk_matrix_t *out) {
  if (!wave || !out) return Fail(PK_MI355_E_INVALID, "null argument");
  int rc = UseDevice(CurrentDevice());
  if (rc) return rc;
  const int T = pk_mi355_num_frames(wave->dim);
  if (T == 0) return ResizeHostMatrix(out, 0, 0);          // fbank.cc:272-273
  if ((rc = ResizeHostMatrix(out, kNumBins, T))) return rc;
  FrontendTables host;
  if (BuildFrontendTables(&host)) return Fail(PK_MI355_E_INVALID, "front-end table construction failed");
  FrontendTables *d_tab = nullptr;
  float *d_wave = nullptr, *d_raw = nullptr;
  int64_t *d_i64 = nullptr;
  int32_t *d_T = nullptr;
  int64_t zeros[2] = {0, 0};
  int32_t hT = T;
  int ret = 0;
  hipError_t e = hipSuccess;
  auto step = [&](hipError_t x) { if (e == hipSuccess) e = x; };
  step(hipMalloc(&d_tab, sizeof(FrontendTables)));
  step(hipMalloc(&d_wave, sizeof(float) * wave->dim));
  step(hipMalloc(&d_raw, sizeof(float) * (size_t)T * kNumBins));
  step(hipMalloc(&d_i64, sizeof(int64_t) * 2));
  step(hipMalloc(&d_T, sizeof(int32_t)));
  if (e == hipSuccess) {
    step(hipMemcpy(d_tab, &host, sizeof(FrontendTables), hipMemcpyHostToDevice));
    step(hipMemcpy(d_wave, wave->data, sizeof(float) * wave->dim, hipMemcpyHostToDevice));
    step(hipMemcpy(d_i64, zeros, sizeof(zeros), hipMemcpyHostToDevice));
    step(hipMemcpy(d_T, &hT, sizeof(hT), hipMemcpyHostToDevice));
  }
  if (e == hipSuccess) {
    UttLayout lay{d_i64, d_T, d_i64 + 1, d_i64 + 1};
    LaunchFbank(d_wave, nullptr, lay, 1, T, d_tab, d_raw, nullptr);
    step(hipGetLastError());
    step(hipMemcpy(out->data, d_raw, sizeof(float) * (size_t)T * kNumBins, hipMemcpyDeviceToHost));
  }
  if (e != hipSuccess) ret = Fail(PK_MI355_E_DEVICE, "fbank_compute: %s", hipGetErrorString(e));
  hipFree(d_tab); hipFree(d_wave); hipFree(d_raw); hipFree(d_i64); hipFree(d_T);
  return ret;
}

int pk_mi355_frontend_compute(const pk_mi355_frontend_spec_t *spec, const pk_vector_t *wave, pk_matrix_t *out) {
  if (!spec || !wave || !out) return Fail(PK_MI355_E_INVALID, "null argument");
  std::vector<FrontendAnyTables> any(1);
  if (int rc = BuildFrontendAnyTables(spec, any.data())) return rc;      // before any device call
  int rc = UseDevice(CurrentDevice());
  if (rc) return rc;
  const int T = pk_mi355_num_frames(wave->dim), D = any[0].dim;
  if (T == 0) return ResizeHostMatrix(out, 0, 0);
  if ((rc = ResizeHostMatrix(out, D, T))) return rc;
  FrontendTables host;
  if (BuildFrontendTables(&host)) return Fail(PK_MI355_E_INVALID, "front-end table construction failed");
  FrontendTables *d_tab = nullptr;
  FrontendAnyTables *d_any = nullptr;
  float *d_wave = nullptr, *d_raw = nullptr;
  int64_t *d_i64 = nullptr;
  int32_t *d_T = nullptr;
  int64_t zeros[2] = {0, 0};
  int32_t hT = T;
  int ret = 0;
  hipError_t e = hipSuccess;
  auto step = [&](hipError_t x) { if (e == hipSuccess) e = x; };
  step(hipMalloc(&d_tab, sizeof(FrontendTables)));
  step(hipMalloc(&d_any, sizeof(FrontendAnyTables)));
  step(hipMalloc(&d_wave, sizeof(float) * wave->dim));
  step(hipMalloc(&d_raw, sizeof(float) * (size_t)T * D));
  step(hipMalloc(&d_i64, sizeof(int64_t) * 2));
  step(hipMalloc(&d_T, sizeof(int32_t)));
  if (e == hipSuccess) {
    step(hipMemcpy(d_tab, &host, sizeof(FrontendTables), hipMemcpyHostToDevice));
    step(hipMemcpy(d_any, any.data(), sizeof(FrontendAnyTables), hipMemcpyHostToDevice));
    step(hipMemcpy(d_wave, wave->data, sizeof(float) * wave->dim, hipMemcpyHostToDevice));
    step(hipMemcpy(d_i64, zeros, sizeof(zeros), hipMemcpyHostToDevice));
    step(hipMemcpy(d_T, &hT, sizeof(hT), hipMemcpyHostToDevice));
  }
  if (e == hipSuccess) {
    UttLayout lay{d_i64, d_T, d_i64 + 1, d_i64 + 1};
    LaunchFbankAny(d_wave, nullptr, lay, 1, T, d_tab, d_any, D, d_raw, nullptr);
    step(hipGetLastError());
    step(hipMemcpy(out->data, d_raw, sizeof(float) * (size_t)T * D, hipMemcpyDeviceToHost));
  }
  if (e != hipSuccess) ret = Fail(PK_MI355_E_DEVICE, "frontend_compute: %s", hipGetErrorString(e));
  hipFree(d_tab); hipFree(d_any); hipFree(d_wave); hipFree(d_raw); hipFree(d_i64); hipFree(d_T);
  return ret;
}

int pk_mi355_cmvn_apply(const pk_vector_t *global_stats, const pk_matrix_t *raw, pk_matrix_t *out) {
  if (!global_stats || !raw || !out) return Fail(PK_MI355_E_INVALID, "null argument");
  if (global_stats->dim != kNumBins + 1 || (raw->ncol > 0 && raw->nrow != kNumBins))
    return Fail(PK_MI355_E_INVALID, "cmvn expects 41 global stats and 40-dim features");
  int rc = UseDevice(CurrentDevice());
  if (rc) return rc;
  const int T = raw->ncol;
  if ((rc = ResizeHostMatrix(out, T > 0 ? kNumBins : 0, T))) return rc;
  if (T == 0) return 0;
  float *d_raw = nullptr, *d_g = nullptr, *d_yt = nullptr;
  CmvnTables *d_ctab = nullptr;
  CmvnTables ctab;
  BuildCmvnTables(global_stats->data[kNumBins], &ctab);
  int64_t *d_i64 = nullptr;
  int32_t *d_T = nullptr;
  int64_t zeros[2] = {0, 0};
  int32_t hT = T;
  const int64_t ld = RoundUp(T, 64);
  std::vector<float> tmp((size_t)kNumBins * T);
  hipError_t e = hipSuccess;
  auto step = [&](hipError_t x) { if (e == hipSuccess) e = x; };
  float *d_raw_alloc = nullptr;
  const size_t raw_floats = (size_t)T * kNumBins + kCmvnRawLead + kCmvnRawSlack;
  step(hipMalloc(&d_raw_alloc, sizeof(float) * raw_floats));
  if (e == hipSuccess) step(hipMemset(d_raw_alloc, 0, sizeof(float) * raw_floats));
  d_raw = d_raw_alloc ? d_raw_alloc + kCmvnRawLead : nullptr;
  step(hipMalloc(&d_g, sizeof(float) * (kNumBins + 1)));
  step(hipMalloc(&d_ctab, sizeof(CmvnTables)));
  step(hipMalloc(&d_yt, sizeof(float) * ld * kNumBins));
  step(hipMalloc(&d_i64, sizeof(int64_t) * 2));
  step(hipMalloc(&d_T, sizeof(int32_t)));
  if (e == hipSuccess) {
    step(hipMemcpy(d_raw, raw->data, sizeof(float) * (size_t)T * kNumBins, hipMemcpyHostToDevice));
    step(hipMemcpy(d_g, global_stats->data, sizeof(float) * (kNumBins + 1), hipMemcpyHostToDevice));
    step(hipMemcpy(d_ctab, &ctab, sizeof(CmvnTables), hipMemcpyHostToDevice));
    step(hipMemcpy(d_i64, zeros, sizeof(zeros), hipMemcpyHostToDevice));
    step(hipMemcpy(d_T, &hT, sizeof(hT), hipMemcpyHostToDevice));
  }
  if (e == hipSuccess) {
    UttLayout lay{d_i64, d_T, d_i64, d_i64 + 1};
    LaunchCmvn(d_raw, lay, 1, d_g, d_ctab, 0, 0, d_yt, ld, nullptr);
    step(hipGetLastError());
    step(hipMemcpy2D(tmp.data(), sizeof(float) * T, d_yt, sizeof(float) * ld, sizeof(float) * T, kNumBins,
                     hipMemcpyDeviceToHost));
  }
  int ret = 0;
  if (e != hipSuccess) ret = Fail(PK_MI355_E_DEVICE, "cmvn_apply: %s", hipGetErrorString(e));
  else
    for (int t = 0; t < T; ++t)
      for (int d = 0; d < kNumBins; ++d) out->data[(size_t)t * kNumBins + d] = tmp[(size_t)d * T + t];
  hipFree(d_raw_alloc); hipFree(d_g); hipFree(d_ctab); hipFree(d_yt); hipFree(d_i64); hipFree(d_T);
  return ret;
}

}  // extern "C"

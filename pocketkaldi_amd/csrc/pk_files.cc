// pk_files.cc -- the host-only file readers and the error state (pk_files.h): the NNT0 / LAY0 / MAT0 / VEC0 model
// files (nnet.cc:80-147), pk_load's key = value file (pocketkaldi.cc:72-144), strict 16 kHz WAV ingestion
// (pcm_reader.cc:45-220), the pk::fst_0 graph (fst.cc:29-110) and its split into the decoder's arc lists.
// Every size a file states is checked against the bytes the file holds before anything is allocated from it.
#include "pk_files.h"

#include <ctype.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <utility>

namespace {
thread_local char g_err[512] = "";
thread_local int g_err_code = 0;
}  // namespace

namespace pkhost {

int Fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  g_err_code = code;
  return code;
}
const char *LastError() { return g_err; }

// ------------------------------------------------------------------ section files

int ReadNnet(const char *path, std::vector<HostLayer> *layers) {
  FileBuf f;
  int rc = f.Open(path);
  if (rc) return rc;
  int32_t sec, num_layers;
  if (!f.Tag("NNT0") || !f.I32(&sec) || !f.I32(&num_layers) || sec != 4)
    return Fail(PK_MI355_E_IO, "NNT0 section expected in %s", path);
  for (int l = 0; l < num_layers; ++l) {
    HostLayer L;
    if (!f.Tag("LAY0") || !f.I32(&sec) || !f.I32(&L.type))
      return Fail(PK_MI355_E_IO, "LAY0 section expected in %s", path);
    if (sec != 4)    // nnet.cc:94-101
      return Fail(PK_MI355_E_IO, "read_layer: section_size == 4 expected, but %d found (%s)", sec, path);
    if (L.type == PK_NNET_LINEAR_LAYER) {
      int32_t rows, cols;
      if (!f.Tag("MAT0") || !f.I32(&sec) || !f.I32(&rows) || !f.I32(&cols) || rows <= 0 || cols <= 0)
        return Fail(PK_MI355_E_IO, "MAT0 section expected in %s", path);
      // rows x VEC0 of cols entries take rows * (12 + 4 cols) bytes (asked as a quotient: the product leaves 64 bits).
      // A file that holds fewer is rejected by the row that falls short, below, with nothing allocated for the rows it
      // does not have.
      if ((uint64_t)rows <= (uint64_t)(f.d.size() - f.pos) / (12 + 4 * (uint64_t)cols)) L.W.reserve((size_t)rows * cols);
      std::vector<float> row;
      for (int r = 0; r < rows; ++r) {
        if ((rc = f.Vec(&row))) return rc;
        if ((int)row.size() != cols)
          return Fail(PK_MI355_E_IO, "Matrix::Read: row dim %d expected, but %d found: %s", cols, (int)row.size(), path);
        L.W.insert(L.W.end(), row.begin(), row.end());
      }
      if ((rc = f.Vec(&L.b))) return rc;
      if ((int)L.b.size() != rows) return Fail(PK_MI355_E_IO, "bias dimension mismatch in %s", path);
      L.in_dim = cols;
      L.out_dim = rows;
    } else if (L.type == PK_NNET_ADD_LAYER || L.type == PK_NNET_MUL_LAYER) {
      // one VEC0, what convert_am.py's write_layer emits for kind 5 (a FixedScaleComponent).  Its kind-4 branch
      // contradicts itself and its parser never produces that kind: 4 is defined here like 5.
      if ((rc = f.Vec(&L.b))) return rc;
      if (L.b.empty()) return Fail(PK_MI355_E_IO, "read_layer: empty vector in a layer of type %d (%s)", L.type, path);
      L.in_dim = L.out_dim = (int)L.b.size();
    } else if (L.type == PK_MI355_NNET_PNORM_LAYER) {
      if (!f.I32(&L.in_dim) || !f.I32(&L.out_dim))
        return Fail(PK_MI355_E_IO, "read_layer: p-norm dimensions expected in %s", path);
      if (L.in_dim <= 0 || L.out_dim <= 0 || L.in_dim % L.out_dim != 0)
        return Fail(PK_MI355_E_IO, "read_layer: p-norm input width %d is not a multiple of the output width %d (%s)", L.in_dim, L.out_dim, path);
    } else if (L.type == PK_MI355_NNET_TIME_SPLICE_LAYER) {
      int32_t n;
      // (a kind 9 with nothing behind it keeps the words a file of an unknown kind is refused with)
      if (!f.I32(&L.in_dim) || !f.I32(&n))
        return Fail(PK_MI355_E_IO, "read_layer: unexpected layer type: %d without a time-splice layer's in_dim and offset count (%s)", L.type, path);
      if (L.in_dim <= 0 || n < 1 || n > 16)
        return Fail(PK_MI355_E_IO, "read_layer: time-splice layer of width %d with %d offsets (%s)", L.in_dim, n, path);
      L.offsets.resize(n);
      for (int c = 0; c < n; ++c) {
        if (!f.I32(&L.offsets[c])) return Fail(PK_MI355_E_IO, "read_layer: %d time-splice offsets expected in %s", n, path);
        if (L.offsets[c] < -32 || L.offsets[c] > 32 || (c > 0 && L.offsets[c] <= L.offsets[c - 1]))
          return Fail(PK_MI355_E_IO, "read_layer: time-splice offset %d (index %d) is out of range or out of order (%s)", L.offsets[c], c, path);
      }
      L.out_dim = n * L.in_dim;
    } else if (L.type != PK_NNET_RELU_LAYER && L.type != PK_NNET_NORMALIZE_LAYER && L.type != PK_NNET_SOFTMAX_LAYER &&
               L.type != PK_MI355_NNET_SIGMOID_LAYER && L.type != PK_MI355_NNET_TANH_LAYER) {
      return Fail(PK_MI355_E_IO, "read_layer: unexpected layer type: %d (%s)", L.type, path);   // nnet.cc:106-127 knows 0..3
    }
    layers->push_back(std::move(L));
  }
  return 0;
}

// ------------------------------------------------------------------ the key = value model file

namespace {

std::string TrimWs(const std::string &s) {
  size_t a = 0, b = s.size();
  while (a < b && isspace((unsigned char)s[a])) ++a;
  while (b > a && isspace((unsigned char)s[b - 1])) --b;
  return s.substr(a, b - a);
}

// configuration.cc:16-55: '#' comments and blank lines skipped, exactly one '=' per line,
// keys lower-cased, empty values rejected.
struct ConfigFile {
  std::string filename;
  std::vector<std::pair<std::string, std::string>> table;

  int Read(const char *path) {
    filename = path;
    FILE *f = fopen(path, "r");
    if (!f) return Fail(PK_MI355_E_IO, "cannot open %s", path);
    std::string text;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
    fclose(f);
    size_t pos = 0;
    while (pos < text.size()) {
      size_t e = text.find('\n', pos);
      if (e == std::string::npos) e = text.size();
      const std::string line = TrimWs(text.substr(pos, e - pos));
      pos = e + 1;
      if (line.empty() || line[0] == '#') continue;
      const size_t eq = line.find('=');
      if (eq == std::string::npos || line.find('=', eq + 1) != std::string::npos)
        return Fail(PK_MI355_E_IO, "Unexpected line in %s: %s", path, line.c_str());
      std::string key = TrimWs(line.substr(0, eq));
      const std::string value = TrimWs(line.substr(eq + 1));
      for (auto &c : key) c = (char)tolower((unsigned char)c);
      if (value.empty()) return Fail(PK_MI355_E_IO, "Value cound not be empty: %s: %s", path, line.c_str());
      bool found = false;
      for (auto &kv : table)
        if (kv.first == key) { kv.second = value; found = true; }
      if (!found) table.emplace_back(key, value);
    }
    return 0;
  }
  const std::string *Find(const char *key) const {
    for (const auto &kv : table)
      if (kv.first == key) return &kv.second;
    return nullptr;
  }
  // configuration.cc:57-72: relative paths are relative to the directory of the file
  int Path(const char *key, std::string *out) const {
    const std::string *v = Find(key);
    if (!v) return Fail(PK_MI355_E_IO, "Unable to find key '%s' in %s", key, filename.c_str());
    const size_t slash = filename.rfind('/');
    *out = ((*v)[0] == '/' || slash == std::string::npos) ? *v : filename.substr(0, slash + 1) + *v;
    return 0;
  }
  int Integer(const char *key, int *out) const {
    const std::string *v = Find(key);
    if (!v) return Fail(PK_MI355_E_IO, "Unable to find key '%s' in %s", key, filename.c_str());
    char *end = nullptr;
    const long x = strtol(v->c_str(), &end, 10);
    if (end == v->c_str()) return Fail(PK_MI355_E_IO, "key '%s' in %s is not an integer: %s", key, filename.c_str(), v->c_str());
    *out = (int)x;
    return 0;
  }
};

}  // namespace

namespace {
int ReadModelConfigAt(const char *config_path, int stats_cap, ModelConfig *out);   // stats_cap 0: the reference's 41
}

int ReadModelConfig(const char *config_path, ModelConfig *out) { return ReadModelConfigAt(config_path, 0, out); }

int ReadModelConfigStats(const char *config_path, int stats_cap, ModelConfig *out) {
  if (stats_cap <= 0) return Fail(PK_MI355_E_INVALID, "bad statistics capacity %d", stats_cap);
  return ReadModelConfigAt(config_path, stats_cap, out);
}

namespace {
int ReadModelConfigAt(const char *config_path, int stats_cap, ModelConfig *out) {
  ConfigFile conf;
  int rc = conf.Read(config_path);
  if (rc) return rc;
  // CMVN global statistics, pocketkaldi.cc:101-116: VEC0 of 40 sums + the frame count
  std::string cmvn_path;
  std::vector<float> stats;
  if ((rc = conf.Path("cmvn_stats", &cmvn_path)) || (rc = ReadVec(cmvn_path.c_str(), &stats))) return rc;
  if (stats_cap == 0) {
    if ((int)stats.size() != kCmvnStats)
      return Fail(PK_MI355_E_IO, "cmvn_stats in %s has %d entries, %d expected", cmvn_path.c_str(), (int)stats.size(), kCmvnStats);
    memcpy(out->cmvn_stats, stats.data(), sizeof(out->cmvn_stats));
  } else {
    if (stats.empty() || (int)stats.size() > stats_cap)
      return Fail(PK_MI355_E_IO, "cmvn_stats in %s has %d entries, 1 to %d expected", cmvn_path.c_str(), (int)stats.size(), stats_cap);
    out->stats = stats;
    out->cmvn_path = cmvn_path;
  }
  // AcousticModel::Read, am.cc:22-62 (a missing left_context is not an error there either)
  if ((rc = conf.Path("nnet", &out->nnet)) || (rc = conf.Path("prior", &out->prior))) return rc;
  if (conf.Find("left_context") && (rc = conf.Integer("left_context", &out->left))) return rc;
  if ((rc = conf.Integer("right_context", &out->right)) || (rc = conf.Integer("num_pdfs", &out->num_pdfs)) ||
      (rc = conf.Path("tid2pdf", &out->tid2pdf)))
    return rc;
  if (out->left < 0 || out->right < 0) return Fail(PK_MI355_E_INVALID, "negative context in %s", config_path);
  return 0;
}
}  // namespace

// ------------------------------------------------------------------ WAV

namespace {

// One reader for both entries.  strict: pk_16kpcm_read's refusals (mono, 16 kHz) in its words; otherwise any positive
// rate and 1 .. 8 channels, of which `channel` is returned.  Every other check is the same, in the same order.
int ReadWaveFile(const char *filename, bool strict, int channel, std::vector<float> *samples, int *rate_out, int *channels_out) {
  FileBuf f;
  int rc = f.Open(filename);
  if (rc) return rc;
  const unsigned char *b = f.d.data();
  const long size = (long)f.d.size();
  auto i32 = [&](long off) { int32_t v; memcpy(&v, b + off, 4); return v; };
  auto i16 = [&](long off) { int16_t v; memcpy(&v, b + off, 2); return (int)v; };
  if (size < 44) return Fail(PK_MI355_E_IO, "file too short for a WAVE header: %s", filename);
  if (memcmp(b, "RIFF", 4)) return Fail(PK_MI355_E_IO, "chunk_name == 'RIFF' expected: %s", filename);
  if (i32(4) != size - 8) return Fail(PK_MI355_E_IO, "chunk_size == %ld expected, but %d found: %s", size - 8, i32(4), filename);
  if (memcmp(b + 8, "WAVE", 4)) return Fail(PK_MI355_E_IO, "Format == 'WAVE' expected: %s", filename);
  if (memcmp(b + 12, "fmt ", 4)) return Fail(PK_MI355_E_IO, "subchunk1 == 'fmt ' expected: %s", filename);
  if (i32(16) != 16) return Fail(PK_MI355_E_IO, "subchunk1_size == 16 expected, but %d found: %s", i32(16), filename);
  if (i16(20) != 1) return Fail(PK_MI355_E_IO, "audio_format == 1 (PCM) expected, but %d found: %s", i16(20), filename);
  const int channels = i16(22);
  if (strict && channels != 1) return Fail(PK_MI355_E_IO, "num_channels == 1 (mono) expected, but %d found: %s", channels, filename);
  if (channels < 1 || channels > 8) return Fail(PK_MI355_E_IO, "num_channels == 1 .. 8 expected, but %d found: %s", channels, filename);
  const int rate = i32(24);
  if (strict && rate != 16000) return Fail(PK_MI355_E_IO, "sample_rate == 16000 expected, but %d found: %s", rate, filename);
  if (rate <= 0) return Fail(PK_MI355_E_IO, "sample_rate > 0 expected, but %d found: %s", rate, filename);
  const int byte_rate = i32(28), align = i16(32), bits = i16(34);
  if (bits != 8 && bits != 16 && bits != 32)
    return Fail(PK_MI355_E_IO, "bits_per_sample == 8, 16 or 32 expected, but %d found: %s", bits, filename);
  const int64_t want_rate = (int64_t)rate * channels * bits / 8;
  if (byte_rate != want_rate) return Fail(PK_MI355_E_IO, "bytes_rate == %lld expected, but %d found: %s", (long long)want_rate, byte_rate, filename);
  if (align != channels * bits / 8) return Fail(PK_MI355_E_IO, "block_align == %d expected, but %d found: %s", channels * bits / 8, align, filename);
  if (memcmp(b + 36, "data", 4)) return Fail(PK_MI355_E_IO, "subchunk2 == 'data' expected: %s", filename);
  if (i32(40) != size - 44) return Fail(PK_MI355_E_IO, "subchunk2_size == %ld expected, but %d found: %s", size - 44, i32(40), filename);
  if (channel < 0 || channel >= channels)
    return Fail(PK_MI355_E_INVALID, "channel %d asked of a file with %d: %s", channel, channels, filename);
  const int width = bits / 8;
  const int n = (int)((size - 44) / align);              // whole sample blocks (a trailing partial block is dropped)
  samples->resize(n);
  const unsigned char *p = b + 44 + channel * width;     // de-interleave: one block of `align` bytes per sample time
  for (int i = 0; i < n; ++i, p += align) {
    float &s = (*samples)[i];
    if (bits == 8) { s = (float)(int8_t)p[0]; }
    else if (bits == 16) { int16_t v; memcpy(&v, p, 2); s = (float)v; }
    else { int32_t v; memcpy(&v, p, 4); s = (float)v; }
  }
  if (rate_out) *rate_out = rate;
  if (channels_out) *channels_out = channels;
  return 0;
}

}  // namespace

int ReadWav16k(const char *filename, std::vector<float> *samples) {
  return ReadWaveFile(filename, true, 0, samples, nullptr, nullptr);
}

int ReadWave(const char *filename, int channel, std::vector<float> *samples, int *rate, int *channels) {
  return ReadWaveFile(filename, false, channel, samples, rate, channels);
}

// ------------------------------------------------------------------ graph

int ReadFst(const char *path, pk_mi355_fst *f) {
  FileBuf fb;
  int rc = fb.Open(path);
  if (rc) return rc;
  const std::vector<unsigned char> &d = fb.d;
  if (d.size() < 48) return Fail(PK_MI355_E_IO, "%s: malformed graph: truncated header", path);
  char name[32];
  memcpy(name, d.data(), 32);
  name[31] = '\0';
  if (strcmp(name, "pk::fst_0") != 0) return Fail(PK_MI355_E_IO, "%s: malformed graph: section name 'pk::fst_0' expected", path);
  int32_t size, ns, na, start;
  memcpy(&size, &d[32], 4); memcpy(&ns, &d[36], 4); memcpy(&na, &d[40], 4); memcpy(&start, &d[44], 4);
  if (ns < 0 || na < 0) return Fail(PK_MI355_E_IO, "%s: malformed graph: negative state or arc count", path);
  const int64_t expect = 12 + (int64_t)ns * 8 + (int64_t)na * 16;
  if (expect != size) return Fail(PK_MI355_E_IO, "%s: malformed graph: section size %d, %lld expected", path, size, (long long)expect);
  if ((int64_t)d.size() < 36 + expect) return Fail(PK_MI355_E_IO, "%s: malformed graph: truncated (%zu bytes, %lld expected)", path,
                                                   d.size(), (long long)(36 + expect));
  if (start < 0 || start >= ns) return Fail(PK_MI355_E_INVALID, "%s: invalid graph: start state %d out of range", path, start);
  f->num_states = ns; f->num_arcs = na; f->start = start;
  f->final_w.resize(ns); f->first.resize(ns); f->arcs.resize(na);
  if (ns) {
    memcpy(f->final_w.data(), &d[48], (size_t)ns * 4);
    memcpy(f->first.data(), &d[48 + (size_t)ns * 4], (size_t)ns * 4);
  }
  if (na) memcpy(f->arcs.data(), &d[48 + (size_t)ns * 8], (size_t)na * 16);
  // Fst::CountArcs (fst.cc:94-110): a state's arcs end at the `first` of the next state whose first is > 0
  f->arc_first.assign(ns, 0); f->arc_count.assign(ns, 0);
  int32_t next_idx = na;
  for (int s = ns - 1; s >= 0; --s) {
    const int32_t fs = f->first[s];
    if (fs >= 0) {
      if (fs > na || next_idx < fs)
        return Fail(PK_MI355_E_INVALID, "%s: invalid graph: arc range [%d, %d) of state %d outside the arc array", path, fs, next_idx, s);
      f->arc_first[s] = fs;
      f->arc_count[s] = next_idx - fs;
    }
    if (fs > 0) next_idx = fs;
  }
  for (int s = 0; s < ns; ++s)
    if (std::isnan(f->final_w[s]))
      return Fail(PK_MI355_E_INVALID, "%s: invalid graph: final weight of state %d is NaN", path, s);
  for (int a = 0; a < na; ++a) {
    const auto &arc = f->arcs[a];
    if (!std::isfinite(arc.weight)) return Fail(PK_MI355_E_INVALID, "%s: invalid graph: arc %d: weight is not finite", path, a);
    if (arc.next < 0 || arc.next >= ns) return Fail(PK_MI355_E_INVALID, "%s: invalid graph: arc %d: next state %d out of range", path, a, arc.next);
    if (arc.ilabel < 0 || arc.olabel < 0) return Fail(PK_MI355_E_INVALID, "%s: invalid graph: arc %d: negative label", path, a);
  }
  return 0;
}

int SplitGraph(const pk_mi355_fst &f, const std::vector<int32_t> &tid2pdf, int num_pdfs, GraphSplit *out) {
  const int S = f.num_states;
  out->e_off.assign(S + 1, 0);
  out->n_off.assign(S + 1, 0);
  for (int s = 0; s < S; ++s) {
    for (int i = 0; i < f.arc_count[s]; ++i) {
      const int a = f.arc_first[s] + i;
      const auto &arc = f.arcs[a];
      SplitArc v = {arc.next, 0, 0, a};
      memcpy(&v.weight_bits, &arc.weight, 4);
      if (arc.ilabel == 0) {
        out->n_arc.push_back(v); out->n_src.push_back(s);
      } else {
        if (!tid2pdf.empty() && arc.ilabel >= (int)tid2pdf.size())
          return Fail(PK_MI355_E_INVALID, "decoder: arc %d: transition id %d outside the model's tid2pdf (%zu entries)",
                      a, arc.ilabel, tid2pdf.size());
        v.pdf = tid2pdf.empty() ? arc.ilabel : tid2pdf[arc.ilabel];
        if (v.pdf < 0 || v.pdf >= num_pdfs)
          return Fail(PK_MI355_E_INVALID, "decoder: arc %d: transition id %d maps to pdf %d, the model has %d", a, arc.ilabel,
                      v.pdf, num_pdfs);
        out->e_arc.push_back(v); out->e_src.push_back(s);
      }
      if (out->e_arc.size() >= kMaxSplitArcs || out->n_arc.size() >= kMaxSplitArcs)
        return Fail(PK_MI355_E_INVALID, "decoder: too many arcs");
    }
    out->e_off[s + 1] = (int)out->e_arc.size();
    out->n_off[s + 1] = (int)out->n_arc.size();
  }
  out->olabel.resize(f.num_arcs);
  for (int a = 0; a < f.num_arcs; ++a) out->olabel[a] = f.arcs[a].olabel;
  return 0;
}

int PathWords(const std::vector<int32_t> &olabel, const int32_t *arcs, int num_arcs, int *words, int max_words) {
  int n = 0;
  for (int i = 0; i < num_arcs; ++i) {
    const int arc = arcs[i];
    const int w = (arc >= 0 && arc < (int)olabel.size()) ? olabel[arc] : 0;
    if (w != 0) {
      if (words && n < max_words) words[n] = w;
      ++n;
    }
  }
  return n;
}

void LabelsOf(const pk_mi355_fst &f, ArcLabels *out) {
  out->ilabel.resize(f.num_arcs); out->olabel.resize(f.num_arcs); out->weight.resize(f.num_arcs);
  for (int a = 0; a < f.num_arcs; ++a) {
    out->ilabel[a] = f.arcs[a].ilabel; out->olabel[a] = f.arcs[a].olabel; out->weight[a] = f.arcs[a].weight;
  }
}

int WordSegments(const ArcLabels &g, const int32_t *arcs, int num_arcs, const float *ac, int num_ac, pk_mi355_word_t *out,
                 int max) {
  int n = 0, frame = 0;
  bool open = false;
  pk_mi355_word_t cur = {0, 0, 0, 0.0f, 0.0f};
  double graph = 0.0, acoustic = 0.0;
  auto close = [&]() {
    cur.graph_cost = (float)graph;
    cur.acoustic_cost = ac ? (float)acoustic : NAN;
    if (out && n < max) out[n] = cur;
    ++n;
  };
  for (int i = 0; i < num_arcs; ++i) {
    const int arc = arcs[i];
    const bool known = arc >= 0 && arc < (int)g.olabel.size();      // (an id outside the graph: an epsilon arc of weight 0)
    const int word = known ? g.olabel[arc] : 0;
    if (word != 0 || !open) {
      if (open) close();
      open = true;
      cur.word = word; cur.start_frame = frame; cur.num_frames = 0;
      graph = 0.0; acoustic = 0.0;
    }
    if (known) graph += (double)g.weight[arc];
    if (known && g.ilabel[arc] != 0) {
      acoustic += (ac && frame < num_ac) ? (double)ac[frame] : (double)NAN;
      ++cur.num_frames;
      ++frame;
    }
  }
  if (open) close();
  return n;
}

int PathFrames(const ArcLabels &g, const int32_t *arcs, const float *arc_ac, int num_arcs, int expect_frames,
               int32_t *arc_ids, int32_t *trans_ids, float *ac, int max_frames) {
  int frames = 0;
  for (int i = 0; i < num_arcs; ++i) {
    const int arc = arcs[i];
    const int tid = (arc >= 0 && arc < (int)g.ilabel.size()) ? g.ilabel[arc] : 0;
    if (tid == 0) continue;
    if (frames < max_frames) {
      if (arc_ids) arc_ids[frames] = arc;
      if (trans_ids) trans_ids[frames] = tid;
      if (ac) ac[frames] = arc_ac ? arc_ac[i] : NAN;
    }
    ++frames;
  }
  if (frames != expect_frames)
    return Fail(PK_MI355_E_DEVICE, "alignment: the path has %d emitting arcs, %d frames were decoded", frames, expect_frames);
  return frames;
}

int ConfigPath(const char *config_path, const char *key, std::string *out) {
  ConfigFile conf;
  int rc = conf.Read(config_path);
  return rc ? rc : conf.Path(key, out);
}

// ------------------------------------------------------------------ symbol table

int ReadSymtab(const char *path, pk_mi355_symtab *st) {
  FileBuf f;
  int rc = f.Open(path);
  if (rc) return rc;
  int32_t section, size, buffer_size;
  if (!f.Tag("SYM0") || !f.I32(&section)) return Fail(PK_MI355_E_IO, "SYM0 section expected in %s", path);
  if (!f.I32(&size) || !f.I32(&buffer_size)) return Fail(PK_MI355_E_IO, "%s: malformed symbol table: truncated header", path);
  if (size < 0 || buffer_size < 0)
    return Fail(PK_MI355_E_IO, "%s: malformed symbol table: negative size %d or buffer size %d", path, size, buffer_size);
  const int64_t expect = 8 + 4 * (int64_t)size + (int64_t)buffer_size;      // symbol_table.cc:45-54
  if (expect != section)
    return Fail(PK_MI355_E_IO, "pk_symboltable_read: section_size = %lld expected, but %d found (%s)", (long long)expect, section,
                path);
  if ((uint64_t)(expect - 8) > (uint64_t)(f.d.size() - f.pos))
    return Fail(PK_MI355_E_IO, "%s: malformed symbol table: truncated (%zu bytes, %lld expected)", path, f.d.size(),
                (long long)(8 + expect));
  st->index.resize(size);
  if (size) memcpy(st->index.data(), &f.d[f.pos], (size_t)size * 4);
  f.pos += (size_t)size * 4;
  st->buffer.assign(f.d.begin() + f.pos, f.d.begin() + f.pos + buffer_size);
  if (buffer_size > 0 && st->buffer.back() != '\0')
    return Fail(PK_MI355_E_IO, "%s: malformed symbol table: the string buffer does not end in NUL", path);
  for (int i = 0; i < size; ++i)
    if (st->index[i] < 0 || st->index[i] >= buffer_size)
      return Fail(PK_MI355_E_INVALID, "%s: invalid symbol table: offset %d of symbol %d outside [0, %d)", path, st->index[i], i,
                  buffer_size);
  return 0;
}

}  // namespace pkhost

using namespace pkhost;

extern "C" {

const char *pk_mi355_last_error(void) { return g_err; }
int pk_mi355_last_error_code(void) { return g_err_code; }

int pk_mi355_16kpcm_read(const char *filename, pk_vector_t *pcm_data) {
  if (!filename || !pcm_data) return Fail(PK_MI355_E_INVALID, "null argument");
  std::vector<float> samples;
  int rc = ReadWav16k(filename, &samples);
  if (rc) return rc;
  const size_t n = samples.size();
  float *s = static_cast<float *>(realloc(pcm_data->data, sizeof(float) * (n > 0 ? n : 1)));
  if (!s) return Fail(PK_MI355_E_INVALID, "out of host memory");
  if (n) memcpy(s, samples.data(), sizeof(float) * n);
  pcm_data->data = s;
  pcm_data->dim = (int)n;
  return 0;
}

int pk_mi355_wave_read(const char *filename, int channel, pk_vector_t *pcm_data, int *rate, int *channels) {
  if (!filename || !pcm_data) return Fail(PK_MI355_E_INVALID, "null argument");
  std::vector<float> samples;
  int rc = ReadWave(filename, channel, &samples, rate, channels);
  if (rc) return rc;
  const size_t n = samples.size();
  float *s = static_cast<float *>(realloc(pcm_data->data, sizeof(float) * (n > 0 ? n : 1)));
  if (!s) return Fail(PK_MI355_E_INVALID, "out of host memory");
  if (n) memcpy(s, samples.data(), sizeof(float) * n);
  pcm_data->data = s;
  pcm_data->dim = (int)n;
  return 0;
}

pk_mi355_fst_t *pk_mi355_fst_read(const char *path) {
  if (!path) { Fail(PK_MI355_E_INVALID, "null path"); return nullptr; }
  pk_mi355_fst *f = new pk_mi355_fst();
  if (ReadFst(path, f)) { delete f; return nullptr; }
  return f;
}

void pk_mi355_fst_destroy(pk_mi355_fst_t *fst) { delete fst; }
int pk_mi355_fst_num_states(const pk_mi355_fst_t *fst) { return fst ? fst->num_states : Fail(PK_MI355_E_INVALID, "null graph"); }
int pk_mi355_fst_num_arcs(const pk_mi355_fst_t *fst) { return fst ? fst->num_arcs : Fail(PK_MI355_E_INVALID, "null graph"); }
int pk_mi355_fst_start(const pk_mi355_fst_t *fst) { return fst ? fst->start : Fail(PK_MI355_E_INVALID, "null graph"); }

int pk_mi355_fst_arc_range(const pk_mi355_fst_t *fst, int state, int *first, int *count) {
  if (!fst || state < 0 || state >= fst->num_states) return Fail(PK_MI355_E_INVALID, "bad graph state");
  if (first) *first = fst->arc_first[state];
  if (count) *count = fst->arc_count[state];
  return 0;
}

pk_mi355_symtab_t *pk_mi355_symtab_read(const char *path) {
  if (!path) { Fail(PK_MI355_E_INVALID, "null path"); return nullptr; }
  pk_mi355_symtab *st = new pk_mi355_symtab();
  if (ReadSymtab(path, st)) { delete st; return nullptr; }
  return st;
}

void pk_mi355_symtab_destroy(pk_mi355_symtab_t *st) { delete st; }
int pk_mi355_symtab_size(const pk_mi355_symtab_t *st) { return st ? (int)st->index.size() : Fail(PK_MI355_E_INVALID, "null symbol table"); }

const char *pk_mi355_symtab_get(const pk_mi355_symtab_t *st, int id) {
  if (!st) { Fail(PK_MI355_E_INVALID, "null symbol table"); return nullptr; }
  if (id < 0 || id >= (int)st->index.size()) {
    Fail(PK_MI355_E_INVALID, "symbol id %d outside [0, %d)", id, (int)st->index.size());
    return nullptr;
  }
  return st->buffer.data() + st->index[id];
}

// ---- endpoint rules (pk_mi355_online_decoder_set_endpointing): the usual five at a 10 ms frame shift, and their test

int pk_mi355_endpoint_default_rules(pk_mi355_endpoint_rule_t *rules, int max) {
  const pk_mi355_endpoint_rule_t usual[5] = {
      {0, 500, INFINITY, 0}, {1, 50, 2.0f, 0}, {1, 100, 8.0f, 0}, {1, 200, INFINITY, 0}, {0, 0, INFINITY, 2000}};
  for (int i = 0; rules && i < 5 && i < max; ++i) rules[i] = usual[i];
  return 5;
}

int pk_mi355_endpoint_eval(const pk_mi355_endpoint_rule_t *rules, int num_rules, int frames, int trailing_silence_frames,
                           float relative_cost) {
  if (!rules || frames <= 0) return 0;
  const bool contains_nonsilence = frames > trailing_silence_frames;
  for (int i = 0; i < num_rules; ++i) {
    const pk_mi355_endpoint_rule_t &r = rules[i];
    if ((contains_nonsilence || !r.must_contain_nonsilence) && trailing_silence_frames >= r.min_trailing_silence_frames &&
        relative_cost <= r.max_relative_cost && frames >= r.min_utterance_frames)
      return i + 1;
  }
  return 0;
}

}  // extern "C"

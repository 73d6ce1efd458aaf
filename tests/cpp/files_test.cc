// files_test.cc -- the host-only file readers (csrc/pk_files.cc) in a process of their own: no HIP, no library, no
// Python.  Built plain and with -fsanitize=address,undefined by tests/test_files_host.py.
//
//   files_test <golden dir> <scratch dir>
//
// 1. positive: the reference-written fixtures, read and printed as dims + 64-bit FNV-1a of every array's bytes (the
//    test compares them with hashes from independent Python parsers);
// 2. sweep: every 4-byte header field of every fixture overwritten with each of eight hostile values, the rows and cols
//    of every MAT0 with each pair of them (a size computed from both can overflow only when both are large), and the
//    file truncated at every section boundary and one byte either side; each variant must end in 0, E_INVALID or E_IO;
// 3. the named regressions: MAT0 / VEC0 headers whose sizes no file could hold.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"

using namespace pkhost;
typedef std::vector<unsigned char> Bytes;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static unsigned long long Fnv(const void *p, size_t n) {
  unsigned long long h = 14695981039346656037ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 1099511628211ull;
  return h;
}
template <typename T>
static unsigned long long Fnv(const std::vector<T> &v) { return Fnv(v.data(), v.size() * sizeof(T)); }

static Bytes Slurp(const std::string &path) {
  Bytes b;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { printf("cannot open %s\n", path.c_str()); exit(2); }
  unsigned char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}
static void Spit(const std::string &path, const Bytes &b) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(b.data(), 1, b.size(), f) != b.size()) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}
static int32_t I32At(const Bytes &b, size_t off) { int32_t v; memcpy(&v, &b[off], 4); return v; }
static void PutI32(Bytes *b, size_t off, int32_t v) { memcpy(&(*b)[off], &v, 4); }

// ------------------------------------------------------------------ the layout of each kind of file
struct Layout {
  std::vector<size_t> fields;       // offsets of the 4-byte header fields
  std::vector<size_t> boundaries;   // offsets where a section starts or ends
  std::vector<size_t> mats;         // offsets of the rows field of every MAT0 (cols follows it)
};

static void WalkVec(const Bytes &b, size_t *pos, Layout *l) {
  l->boundaries.push_back(*pos);
  l->fields.push_back(*pos + 4);
  l->fields.push_back(*pos + 8);
  *pos += 12 + 4 * (size_t)I32At(b, *pos + 8);
}
static Layout VecLayout(const Bytes &b) {
  Layout l;
  size_t pos = 0;
  WalkVec(b, &pos, &l);
  l.boundaries.push_back(12);
  l.boundaries.push_back(pos);
  return l;
}
static Layout NnetLayout(const Bytes &b) {
  Layout l;
  l.boundaries.push_back(0);
  l.fields.push_back(4);
  l.fields.push_back(8);
  size_t pos = 12;
  for (int i = 0, n = I32At(b, 8); i < n; ++i) {
    l.boundaries.push_back(pos);
    l.fields.push_back(pos + 4);
    l.fields.push_back(pos + 8);
    const int type = I32At(b, pos + 8);
    pos += 12;
    if (type != PK_NNET_LINEAR_LAYER) continue;
    l.boundaries.push_back(pos);
    for (int k = 1; k <= 3; ++k) l.fields.push_back(pos + 4 * k);
    l.mats.push_back(pos + 8);
    const int rows = I32At(b, pos + 8);
    pos += 16;
    for (int r = 0; r <= rows && pos + 12 <= b.size(); ++r) WalkVec(b, &pos, &l);   // the rows and the bias, as far as the file has them
  }
  l.boundaries.push_back(pos);
  return l;
}
static Layout FstLayout(const Bytes &b) {
  Layout l;
  const size_t ns = I32At(b, 36), na = I32At(b, 40);
  for (size_t off : {32, 36, 40, 44}) l.fields.push_back(off);
  for (size_t s = 0; s < ns; ++s) l.fields.push_back(48 + 4 * ns + 4 * s);
  for (size_t a = 0; a < na; ++a)
    for (size_t k = 0; k < 3; ++k) l.fields.push_back(48 + 8 * ns + 16 * a + 4 * k);
  l.boundaries = {0, 32, 36, 48, 48 + 4 * ns, 48 + 8 * ns, 48 + 8 * ns + 16 * na};
  return l;
}
static Layout WavLayout(const Bytes &b) {
  Layout l;
  l.fields = {4, 16, 20, 24, 28, 32, 40};   // chunk size, fmt size, format | channels, rate, byte rate, align | bits, data size
  l.boundaries = {0, 12, 36, 44, b.size()};
  return l;
}
static Layout ConfLayout(const Bytes &b) {   // text: no binary fields; the lines are its sections
  Layout l;
  l.boundaries.push_back(0);
  for (size_t i = 0; i < b.size(); ++i)
    if (b[i] == '\n') l.boundaries.push_back(i + 1);
  l.boundaries.push_back(b.size());
  return l;
}

// ------------------------------------------------------------------ the sweep
static const int32_t kValues[8] = {0, 1, -1, 1 << 20, 1 << 29, 1 << 30, INT32_MAX, INT32_MIN};

template <typename Run>
static void Sweep(const char *name, const Bytes &good, const Layout &l, const std::string &variant, Run run) {
  std::set<int> codes;
  int cases = 0;
  auto one = [&](const Bytes &b, const char *what, size_t at, long long v) {
    Spit(variant, b);
    Fail(0, "%s", "");     // the error text is the thread's last: empty it, so that a failure has to set its own
    const int rc = run(variant.c_str());
    ++cases;
    codes.insert(rc);
    CHECK(rc == 0 || rc == PK_MI355_E_INVALID || rc == PK_MI355_E_IO, "%s: %s at %zu (%lld): code %d", name, what, at, v, rc);
    CHECK(rc == 0 || LastError()[0] != '\0', "%s: %s at %zu (%lld): no error text", name, what, at, v);
  };
  for (size_t off : l.fields)
    for (int32_t v : kValues) {
      Bytes b = good;
      PutI32(&b, off, v);
      one(b, "field", off, v);
    }
  for (size_t off : l.mats)
    for (int32_t rows : kValues)
      for (int32_t cols : kValues) {
        Bytes b = good;
        PutI32(&b, off, rows);
        PutI32(&b, off + 4, cols);
        one(b, "rows x cols", off, (long long)rows * cols);
      }
  std::set<size_t> cuts;
  for (size_t at : l.boundaries)
    for (size_t len : {at ? at - 1 : 0, at, at + 1}) cuts.insert(len);
  for (size_t len : cuts) {
    Bytes b = good;
    b.resize(len, 0);      // (one byte past the end of the file: a zero byte more)
    one(b, "cut", len, 0);
  }
  printf("sweep %s fields %zu mats %zu cases %d codes", name, l.fields.size(), l.mats.size(), cases);
  for (int c : codes) printf(" %d", c);
  printf("\n");
}

// ------------------------------------------------------------------ positive
static void PrintFst(const char *name, const std::string &path, const std::vector<int32_t> &tid2pdf, int num_pdfs) {
  pk_mi355_fst_t *f = pk_mi355_fst_read(path.c_str());
  CHECK(f, "%s: %s", name, LastError());
  if (!f) return;
  printf("fst %s states %d arcs %d start %d final %016llx first %016llx arc_first %016llx arc_count %016llx arcs %016llx\n", name,
         pk_mi355_fst_num_states(f), pk_mi355_fst_num_arcs(f), pk_mi355_fst_start(f), Fnv(f->final_w), Fnv(f->first),
         Fnv(f->arc_first), Fnv(f->arc_count), Fnv(f->arcs));
  GraphSplit g;
  const int rc = SplitGraph(*f, tid2pdf, num_pdfs, &g);
  CHECK(rc == 0, "%s: split: %s", name, LastError());
  printf("split %s e %zu n %zu e_off %016llx n_off %016llx e_src %016llx n_src %016llx e_arc %016llx n_arc %016llx olabel %016llx\n",
         name, g.e_arc.size(), g.n_arc.size(), Fnv(g.e_off), Fnv(g.n_off), Fnv(g.e_src), Fnv(g.n_src), Fnv(g.e_arc), Fnv(g.n_arc),
         Fnv(g.olabel));
  pk_mi355_fst_destroy(f);
}

// a graph that reads is also split and walked
static int RunFst(const char *path, const std::vector<int32_t> &tid2pdf, int num_pdfs) {
  pk_mi355_fst_t *f = pk_mi355_fst_read(path);
  if (!f) return pk_mi355_last_error_code();
  GraphSplit g;
  int rc = SplitGraph(*f, tid2pdf, num_pdfs, &g);
  if (rc == 0) {
    std::vector<int32_t> path_arcs, words(f->num_arcs + 1);
    for (int a = -1; a <= f->num_arcs; ++a) path_arcs.push_back(a);
    const int n = PathWords(g.olabel, path_arcs.data(), (int)path_arcs.size(), words.data(), f->num_arcs);
    CHECK(n >= 0 && n <= f->num_arcs, "PathWords: %d words of %d arcs", n, f->num_arcs);
    int first, count;
    for (int s = 0; s < f->num_states; ++s)
      CHECK(pk_mi355_fst_arc_range(f, s, &first, &count) == 0 && first >= 0 && count >= 0 && first + count <= f->num_arcs,
            "arc range of state %d", s);
  }
  pk_mi355_fst_destroy(f);
  return rc;
}

static Bytes NnetWithMat0(int32_t rows, int32_t cols) {   // NNT0 4 1, LAY0 4 0, MAT0 8 rows cols: 40 bytes
  Bytes b(40);
  memcpy(&b[0], "NNT0", 4); PutI32(&b, 4, 4); PutI32(&b, 8, 1);
  memcpy(&b[12], "LAY0", 4); PutI32(&b, 16, 4); PutI32(&b, 20, 0);
  memcpy(&b[24], "MAT0", 4); PutI32(&b, 28, 8); PutI32(&b, 32, rows); PutI32(&b, 36, cols);
  return b;
}

int main(int argc, char **argv) {
  if (argc != 3) { printf("usage: files_test <golden dir> <scratch dir>\n"); return 2; }
  const std::string G = argv[1], S = argv[2], M = G + "/refmodel/";

  // ---- positive
  std::vector<HostLayer> layers;
  CHECK(ReadNnet((M + "refmodel.nnet").c_str(), &layers) == 0, "%s", LastError());
  printf("nnet layers %zu\n", layers.size());
  for (size_t i = 0; i < layers.size(); ++i)
    printf("layer %zu type %d in %d out %d W %016llx b %016llx\n", i, layers[i].type, layers[i].in_dim, layers[i].out_dim,
           Fnv(layers[i].W), Fnv(layers[i].b));
  std::vector<float> prior, cmvn;
  std::vector<int32_t> tid2pdf;
  CHECK(ReadVec((M + "refmodel.prior").c_str(), &prior) == 0, "%s", LastError());
  CHECK(ReadVec((M + "refmodel_tid2pdf.bin").c_str(), &tid2pdf) == 0, "%s", LastError());
  CHECK(ReadVec((M + "refmodel_cmvn.bin").c_str(), &cmvn) == 0, "%s", LastError());
  printf("prior n %zu %016llx\n", prior.size(), Fnv(prior));
  printf("tid2pdf n %zu %016llx\n", tid2pdf.size(), Fnv(tid2pdf));
  printf("cmvn n %zu %016llx\n", cmvn.size(), Fnv(cmvn));
  ModelConfig conf;
  CHECK(ReadModelConfig((M + "refmodel.conf").c_str(), &conf) == 0, "%s", LastError());
  printf("conf left %d right %d num_pdfs %d stats %016llx nnet %s prior %s tid2pdf %s\n", conf.left, conf.right, conf.num_pdfs,
         Fnv(conf.cmvn_stats, sizeof(conf.cmvn_stats)), conf.nnet.c_str(), conf.prior.c_str(), conf.tid2pdf.c_str());
  pk_vector_t wav = {0, nullptr};
  CHECK(pk_mi355_16kpcm_read((G + "/en-us-hello.wav").c_str(), &wav) == 0, "%s", LastError());
  printf("wav n %d %016llx\n", wav.dim, Fnv(wav.data, sizeof(float) * wav.dim));
  free(wav.data);
  const int num_pdfs = conf.num_pdfs;
  PrintFst("testinput.fst", G + "/testinput.fst", tid2pdf, num_pdfs);
  PrintFst("wordloop.fst", M + "wordloop.fst", tid2pdf, num_pdfs);

  // ---- sweep
  const std::string V = S + "/variant.bin";
  Bytes b = Slurp(M + "refmodel.nnet");
  Sweep("refmodel.nnet", b, NnetLayout(b), V, [](const char *p) { std::vector<HostLayer> l; return ReadNnet(p, &l); });
  b = NnetWithMat0(24, 160);            // the 40-byte file: a MAT0 header and nothing behind it
  Sweep("mat0_40_bytes", b, NnetLayout(b), V, [](const char *p) { std::vector<HostLayer> l; return ReadNnet(p, &l); });
  b = Slurp(M + "refmodel.prior");
  Sweep("refmodel.prior", b, VecLayout(b), V, [](const char *p) { std::vector<float> v; return ReadVec(p, &v); });
  b = Slurp(M + "refmodel_tid2pdf.bin");
  Sweep("refmodel_tid2pdf.bin", b, VecLayout(b), V, [](const char *p) { std::vector<int32_t> v; return ReadVec(p, &v); });
  // the CMVN statistics are read through the model config: a config in the scratch directory names the variant
  const std::string text = "cmvn_stats = variant.bin\nnnet = a\nprior = b\nright_context = 1\nnum_pdfs = 18\ntid2pdf = c\n";
  Spit(S + "/cmvn.conf", Bytes(text.begin(), text.end()));
  const std::string cmvn_conf = S + "/cmvn.conf";
  b = Slurp(M + "refmodel_cmvn.bin");
  Sweep("refmodel_cmvn.bin", b, VecLayout(b), V, [&](const char *) { ModelConfig c; return ReadModelConfig(cmvn_conf.c_str(), &c); });
  Spit(S + "/refmodel_cmvn.bin", b);    // what the variants of refmodel.conf name, next to them
  b = Slurp(M + "refmodel.conf");
  Sweep("refmodel.conf", b, ConfLayout(b), V, [](const char *p) { ModelConfig c; return ReadModelConfig(p, &c); });
  b = Slurp(G + "/en-us-hello.wav");
  Sweep("en-us-hello.wav", b, WavLayout(b), V, [](const char *p) { std::vector<float> s; return ReadWav16k(p, &s); });
  for (const std::string &path : {G + "/testinput.fst", M + "wordloop.fst"}) {
    b = Slurp(path);
    Sweep(path.substr(path.rfind('/') + 1).c_str(), b, FstLayout(b), V,
          [&](const char *p) { return RunFst(p, tid2pdf, num_pdfs); });
  }

  // ---- named regressions
  std::vector<HostLayer> none;
  const int32_t mat0[4][2] = {{1 << 30, 1 << 30}, {1 << 20, 1 << 20},
                              {1 << 30, INT32_MAX}, {INT32_MAX, 1 << 30}};   // rows * (12 + 4 cols) leaves 63 bits
  for (const auto &dim : mat0) {
    Spit(V, NnetWithMat0(dim[0], dim[1]));
    const int rc = ReadNnet(V.c_str(), &none);
    printf("regression mat0 %d x %d: %d\n", dim[0], dim[1], rc);
    CHECK(rc == PK_MI355_E_IO && strstr(LastError(), V.c_str()), "MAT0 %d x %d: %d %s", dim[0], dim[1], rc, LastError());
  }
  {
    Bytes v(12 + 64);     // bytes = 4: what 4 n + 4 comes to in 32 bits
    memcpy(&v[0], "VEC0", 4); PutI32(&v, 4, 4); PutI32(&v, 8, 1 << 30);
    Spit(V, v);
    const int rc = ReadVec(V.c_str(), &prior);
    printf("regression vec0 n %d: %d\n", 1 << 30, rc);
    CHECK(rc == PK_MI355_E_IO && strstr(LastError(), V.c_str()), "VEC0: %d %s", rc, LastError());
  }
  {
    pk_mi355_fst f;       // a directory opens, and has no bytes
    int rc = ReadNnet(S.c_str(), &none);
    if (rc == PK_MI355_E_IO) rc = ReadVec(S.c_str(), &prior);
    if (rc == PK_MI355_E_IO) rc = ReadWav16k(S.c_str(), &cmvn);
    if (rc == PK_MI355_E_IO) rc = ReadFst(S.c_str(), &f);
    if (rc == PK_MI355_E_IO) rc = ReadModelConfig(S.c_str(), &conf);
    printf("regression directory: %d\n", rc);
    CHECK(rc == PK_MI355_E_IO, "directory: %d %s", rc, LastError());
  }
  if (g_failures) printf("files_test FAILED (%d)\n", g_failures);
  else printf("files_test ok\n");
  return g_failures ? 1 : 0;
}

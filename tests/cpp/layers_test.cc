// layers_test.cc -- the host side of the layer kinds 4 to 8 (csrc/pk_layers.cc) and the model-file
// reader's share of them (csrc/pk_files.cc) in a process of its own: no HIP, no library, no Python.  Built plain and with
// -fsanitize=address,undefined by tests/test_cpp_layers.py, which restates the inputs below in numpy and compares the
// hashes this program prints with those of the rules of tests/layer_cases.py.
//
//   layers_test [model.nnet]
//
// Cases: the rules at the edge widths {1, 7, 16, 17, 129} and rows {1, 67} in exactly sized buffers (p-norm: groups of
// 1, 2, 5 and 10), hashed with every NaN made the canonical one; the refusals of the entries; the reader on a
// well-formed file of every new kind, on every proper prefix of it (cuts inside the vector and inside the two ints
// among them), on an empty vector, on a p-norm whose in_dim is no multiple of its out_dim and on kinds outside 0..8.
// With a path: the layers of that file, one line each (what pocketkaldi_amd.write_nnet wrote).
// Input entry i: kSpecial[(i / 13) % 25] where i % 13 == 5, else ((h(i + 99) >> 12) / 16384 - 32) as float, with
// h(k) = k * 2654435761 mod 2^32; vector entry i: ((h(i + 7) >> 12) / 262144 - 2) as float.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"
#include "../../pocketkaldi_amd/csrc/pk_layers.h"

using pkhost::HostLayer;
using pkhost::LastError;
using pkhost::ReadNnet;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool Has(const char *text, const std::string &what) { return std::string(text).find(what) != std::string::npos; }
static uint32_t H(uint32_t k) { return k * 2654435761u; }

static unsigned long long Fnv(const void *data, size_t bytes) {
  unsigned long long h = 14695981039346656037ull;
  const unsigned char *p = static_cast<const unsigned char *>(data);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

static unsigned long long HashRows(std::vector<float> y) {
  for (float &v : y)
    if (v != v) { const uint32_t q = 0x7fc00000u; memcpy(&v, &q, 4); }
  return Fnv(y.data(), y.size() * sizeof(float));
}

// +-0, +-1e-8, subnormals, +-1, +-17, +-88, +-104, +-2e19, +-inf, NaN
static const uint32_t kSpecial[25] = {0x00000000u, 0x80000000u, 0x322bcc77u, 0xb22bcc77u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu,
                                      0x00400000u, 0x80400000u, 0x3f800000u, 0xbf800000u, 0x41880000u, 0xc1880000u, 0x42b00000u, 0xc2b00000u,
                                      0x42d00000u, 0xc2d00000u, 0x5f8ac723u, 0xdf8ac723u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x7f800000u,
                                      0xff800000u};

static std::vector<float> Input(size_t n) {
  std::vector<float> x(n);
  for (size_t i = 0; i < n; ++i) {
    if (i % 13 == 5) memcpy(&x[i], &kSpecial[(i / 13) % 25], 4);
    else x[i] = (float)((double)(H((uint32_t)i + 99u) >> 12) / 16384.0 - 32.0);
  }
  return x;
}

static std::vector<float> Vector(size_t n) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (float)((double)(H((uint32_t)i + 7u) >> 12) / 262144.0 - 2.0);
  return v;
}

static void Put32(std::string *s, int32_t v) { s->append(reinterpret_cast<const char *>(&v), 4); }
static std::string Vec0(const std::vector<float> &v) {
  std::string s = "VEC0";
  Put32(&s, (int32_t)(4 * v.size() + 4));
  Put32(&s, (int32_t)v.size());
  s.append(reinterpret_cast<const char *>(v.data()), 4 * v.size());
  return s;
}
static std::string Nnt0(int layers) {
  std::string s = "NNT0";
  Put32(&s, 4);
  Put32(&s, layers);
  return s;
}
static std::string Lay0(int kind, const std::string &payload) {
  std::string s = "LAY0";
  Put32(&s, 4);
  Put32(&s, kind);
  return s + payload;
}
static std::string Ints(int32_t a, int32_t b) {
  std::string s;
  Put32(&s, a);
  Put32(&s, b);
  return s;
}

static std::string g_dir;
static int ReadBytes(const std::string &bytes, std::vector<HostLayer> *layers) {
  const std::string path = g_dir + "/m.nnet";
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) { printf("FAILED cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
  layers->clear();
  return ReadNnet(path.c_str(), layers);
}

int main(int argc, char **argv) {
  if (argc > 1) {                       // the layers of a file
    std::vector<HostLayer> layers;
    const int rc = ReadNnet(argv[1], &layers);
    if (rc) { printf("FAILED ReadNnet: %d (%s)\n", rc, LastError()); return 1; }
    for (const HostLayer &L : layers)
      printf("layer %d %d %d %016llx %016llx\n", L.type, L.in_dim, L.out_dim, Fnv(L.W.data(), L.W.size() * 4), Fnv(L.b.data(), L.b.size() * 4));
    printf("layers_test ok\n");
    return 0;
  }

  // ---- the rules, in exactly sized buffers
  const int widths[] = {1, 7, 16, 17, 129}, row_counts[] = {1, 67}, groups[] = {1, 2, 5, 10};
  const int kinds[] = {PK_NNET_ADD_LAYER, PK_NNET_MUL_LAYER, PK_MI355_NNET_SIGMOID_LAYER, PK_MI355_NNET_TANH_LAYER};
  for (int kind : kinds)
    for (int D : widths)
      for (int T : row_counts) {
        const std::vector<float> x = Input((size_t)T * D), v = Vector(D);
        std::vector<float> y((size_t)T * D);
        const int rc = pk_mi355_layer_apply_host(kind, x.data(), T, D, pklayers::IsVectorKind(kind) ? v.data() : nullptr, D, y.data());
        CHECK(rc == 0, "kind %d D %d T %d: %d (%s)", kind, D, T, rc, LastError());
        printf("rule %d %d %d %016llx\n", kind, D, T, HashRows(y));
      }
  for (int O : widths)
    for (int G : groups)
      for (int T : row_counts) {
        const std::vector<float> x = Input((size_t)T * O * G);
        std::vector<float> y((size_t)T * O);
        const int rc = pk_mi355_layer_apply_host(PK_MI355_NNET_PNORM_LAYER, x.data(), T, O * G, nullptr, O, y.data());
        CHECK(rc == 0, "p-norm O %d G %d T %d: %d (%s)", O, G, T, rc, LastError());
        printf("pnorm %d %d %d %016llx\n", O, G, T, HashRows(y));
      }
  {   // zero rows touch nothing; known values
    CHECK(pk_mi355_layer_apply_host(PK_MI355_NNET_TANH_LAYER, nullptr, 0, 4, nullptr, 4, nullptr) == 0, "T = 0: %s", LastError());
    const float x[4] = {3.0f, 4.0f, 0.0f, -0.0f};
    float y[2] = {-1.0f, -1.0f};
    CHECK(pk_mi355_layer_apply_host(PK_MI355_NNET_PNORM_LAYER, x, 1, 4, nullptr, 2, y) == 0 && y[0] == 5.0f && y[1] == 0.0f, "3-4-5");
    float s[2] = {0.0f, INFINITY}, out[2];
    CHECK(pk_mi355_layer_apply_host(PK_MI355_NNET_SIGMOID_LAYER, s, 1, 2, nullptr, 2, out) == 0 && out[0] == 0.5f && out[1] == 1.0f, "sigmoid");
  }

  // ---- the refusals
  {
    float x[6] = {0}, y[6];
    const float bad[3] = {1.0f, NAN, 2.0f};
    for (int kind : {0, 1, 2, 3, 9, -1})
      CHECK(pk_mi355_layer_apply_host(kind, x, 1, 6, nullptr, 6, y) == PK_MI355_E_INVALID && Has(LastError(), "unexpected layer type"), "kind %d", kind);
    CHECK(pk_mi355_layer_apply_host(PK_MI355_NNET_PNORM_LAYER, x, 1, 6, nullptr, 4, y) == PK_MI355_E_INVALID &&
              Has(LastError(), "input width 6 is not a multiple of the output width 4"), "p-norm 6 -> 4: %s", LastError());
    CHECK(pk_mi355_layer_apply_host(PK_MI355_NNET_PNORM_LAYER, x, 1, 6, nullptr, 0, y) == PK_MI355_E_INVALID, "p-norm 6 -> 0");
    CHECK(pk_mi355_layer_apply_host(PK_MI355_NNET_TANH_LAYER, x, 1, 6, nullptr, 3, y) == PK_MI355_E_INVALID, "tanh 6 -> 3");
    CHECK(pk_mi355_layer_apply_host(PK_NNET_ADD_LAYER, x, 1, 3, nullptr, 3, y) == PK_MI355_E_INVALID, "add without a vector");
    CHECK(pk_mi355_layer_apply_host(PK_NNET_MUL_LAYER, x, 1, 3, bad, 3, y) == PK_MI355_E_INVALID && Has(LastError(), "entry 1 is not finite"),
          "mul with a NaN entry: %s", LastError());
    CHECK(pk_mi355_layer_apply_host(PK_NNET_MUL_LAYER, x, -1, 3, bad, 3, y) == PK_MI355_E_INVALID, "negative rows");
    CHECK(pk_mi355_layer_apply_host(PK_NNET_MUL_LAYER, nullptr, 1, 3, x, 3, y) == PK_MI355_E_INVALID && Has(LastError(), "null argument"), "null rows");
    CHECK(pklayers::CheckPnorm(12, 4) == 0 && pklayers::CheckVectorLayer(PK_NNET_ADD_LAYER, 6, x) == 0, "well-formed parameters");
    CHECK(pklayers::CheckVectorLayer(PK_MI355_NNET_TANH_LAYER, 6, x) == PK_MI355_E_INVALID, "tanh is no vector layer");
  }

  // ---- the reader
  char tmpl[] = "/tmp/pk_layers_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("FAILED mkdtemp\n"); return 2; }
  g_dir = tmpl;
  std::vector<HostLayer> layers;
  const std::vector<float> v5 = Vector(5);
  const std::string whole = Nnt0(5) + Lay0(PK_NNET_ADD_LAYER, Vec0(v5)) + Lay0(PK_MI355_NNET_SIGMOID_LAYER, "") +
                            Lay0(PK_MI355_NNET_PNORM_LAYER, Ints(10, 5)) + Lay0(PK_MI355_NNET_TANH_LAYER, "") + Lay0(PK_NNET_MUL_LAYER, Vec0(v5));
  int rc = ReadBytes(whole, &layers);
  CHECK(rc == 0 && layers.size() == 5, "the well-formed file: %d (%s)", rc, LastError());
  if (layers.size() == 5) {
    CHECK(layers[0].type == PK_NNET_ADD_LAYER && layers[0].b == v5 && layers[0].in_dim == 5 && layers[0].out_dim == 5, "add");
    CHECK(layers[1].type == PK_MI355_NNET_SIGMOID_LAYER && layers[1].b.empty(), "sigmoid");
    CHECK(layers[2].type == PK_MI355_NNET_PNORM_LAYER && layers[2].in_dim == 10 && layers[2].out_dim == 5, "p-norm");
    CHECK(layers[3].type == PK_MI355_NNET_TANH_LAYER, "tanh");
    CHECK(layers[4].type == PK_NNET_MUL_LAYER && layers[4].b == v5, "mul");
  }
  for (size_t cut = 0; cut < whole.size(); ++cut) {        // every proper prefix: inside the vectors, inside the two ints
    rc = ReadBytes(whole.substr(0, cut), &layers);
    CHECK(rc == PK_MI355_E_IO, "cut at %zu of %zu: %d", cut, whole.size(), rc);
  }
  rc = ReadBytes(Nnt0(1) + Lay0(PK_MI355_NNET_PNORM_LAYER, Ints(10, 4)), &layers);
  CHECK(rc == PK_MI355_E_IO && Has(LastError(), "input width 10 is not a multiple of the output width 4"), "p-norm 10 -> 4: %d (%s)", rc, LastError());
  for (int o : {0, -5})
    CHECK(ReadBytes(Nnt0(1) + Lay0(PK_MI355_NNET_PNORM_LAYER, Ints(10, o)), &layers) == PK_MI355_E_IO, "p-norm 10 -> %d", o);
  CHECK(ReadBytes(Nnt0(1) + Lay0(PK_MI355_NNET_PNORM_LAYER, Ints(0, 5)), &layers) == PK_MI355_E_IO, "p-norm 0 -> 5");
  CHECK(ReadBytes(Nnt0(1) + Lay0(PK_NNET_MUL_LAYER, Vec0({})), &layers) == PK_MI355_E_IO && Has(LastError(), "empty vector"), "empty vector");
  {   // a vector whose header states more entries than the file holds
    std::string s = Nnt0(1) + Lay0(PK_NNET_ADD_LAYER, "VEC0");
    Put32(&s, 4 * 1000 + 4);
    Put32(&s, 1000);
    s.append(16, '\0');
    CHECK(ReadBytes(s, &layers) == PK_MI355_E_IO && Has(LastError(), "corrupted VEC0"), "over-long vector: %s", LastError());
  }
  for (int kind : {9, 10, -1, 1 << 30}) {
    rc = ReadBytes(Nnt0(1) + Lay0(kind, ""), &layers);
    CHECK(rc == PK_MI355_E_IO && Has(LastError(), "read_layer: unexpected layer type: " + std::to_string(kind)), "kind %d: %d (%s)", kind, rc, LastError());
  }
  unlink((g_dir + "/m.nnet").c_str());
  rmdir(g_dir.c_str());

  if (g_failures) { printf("%d failures\n", g_failures); return 1; }
  printf("layers_test ok\n");
  return 0;
}

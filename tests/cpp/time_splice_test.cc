// time_splice_test.cc -- the host side of the time-splice layer, kind 9 (csrc/pk_layers.cc) and the
// model-file reader's share of it (csrc/pk_files.cc) in a process of its own: no HIP, no library, no Python.  Built plain
// and with -fsanitize=address,undefined by tests/test_cpp_time_splice.py, which restates the inputs below in numpy and
// compares the hashes this program prints with those of the rule of tests/time_splice_cases.py.
//
//   time_splice_test
//
// Cases: the rule at the widths {1, 7, 16, 17, 129}, the offset lists below and lo + hi + {1, 67} rows in exactly sized
// buffers (a read one row outside is a sanitizer report), hashed byte for byte; the refusals of the entry; the reader on a
// well-formed file of two such layers, on every proper prefix of it and on malformed ones.
// Input word i (bits, so that NaN payloads travel): h(i + 99) where i % 13 != 5, else kSpecial[(i / 13) % 8], with
// h(k) = k * 2654435761 mod 2^32.
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

// NaNs with payloads, a signalling one, +-0, the smallest subnormal, +-inf
static const uint32_t kSpecial[8] = {0x7fc00001u, 0xffc12345u, 0x7f800001u, 0x80000000u, 0x00000000u, 0x00000001u, 0x7f800000u, 0xff800000u};

static std::vector<float> Input(size_t n) {
  std::vector<float> x(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t w = i % 13 == 5 ? kSpecial[(i / 13) % 8] : H((uint32_t)i + 99u);
    memcpy(&x[i], &w, 4);
  }
  return x;
}

static void Put32(std::string *s, int32_t v) { s->append(reinterpret_cast<const char *>(&v), 4); }
static std::string Nnt0(int layers) {
  std::string s = "NNT0";
  Put32(&s, 4);
  Put32(&s, layers);
  return s;
}
static std::string Splice(int in_dim, const std::vector<int32_t> &offsets, long stated = 1L << 40) {      // stated: the count the file states, if not the list's
  std::string s = "LAY0";
  Put32(&s, 4);
  Put32(&s, PK_MI355_NNET_TIME_SPLICE_LAYER);
  Put32(&s, in_dim);
  Put32(&s, stated != 1L << 40 ? (int32_t)stated : (int32_t)offsets.size());
  for (int32_t o : offsets) Put32(&s, o);
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

int main() {
  // ---- the rule, in exactly sized buffers
  const int widths[] = {1, 7, 16, 17, 129};
  const std::vector<std::vector<int32_t>> lists = {{0}, {-1, 0, 1}, {-3, 3}, {0, 2}, {-2, 1}, {-7, 2}, {-32, 32}};
  for (size_t li = 0; li < lists.size(); ++li)
    for (int D : widths)
      for (int more : {1, 67}) {
        const std::vector<int32_t> &o = lists[li];
        const int n = (int)o.size(), lo = pklayers::TimeLo(o.data(), n), hi = pklayers::TimeHi(o.data(), n), T = lo + hi + more;
        const std::vector<float> x = Input((size_t)T * D);
        std::vector<float> y((size_t)more * n * D);
        const int rc = pk_mi355_time_splice_host(x.data(), T, D, o.data(), n, y.data());
        CHECK(rc == 0, "list %zu D %d T %d: %d (%s)", li, D, T, rc, LastError());
        printf("splice %zu %d %d %016llx\n", li, D, T, Fnv(y.data(), y.size() * sizeof(float)));
        // one row too few: refused, nothing written
        std::vector<float> none(1, 7.0f);
        CHECK(pk_mi355_time_splice_host(x.data(), lo + hi, D, o.data(), n, none.data()) == PK_MI355_E_INVALID && none[0] == 7.0f &&
                  Has(LastError(), std::to_string(lo + hi) + " rows, the offsets consume " + std::to_string(lo) + " on the left and " + std::to_string(hi)),
              "list %zu D %d rows %d: %s", li, D, lo + hi, LastError());
      }

  // ---- the refusals
  {
    float x[8] = {0}, y[16];
    const int32_t asc[3] = {-1, 0, 1}, eq[3] = {-1, -1, 1}, desc[3] = {-1, 2, 1}, far[2] = {0, 33}, near[2] = {-33, 0};
    int32_t many[17];
    for (int i = 0; i < 17; ++i) many[i] = i - 8;
    CHECK(pklayers::CheckTimeSplice(4, asc, 3) == 0 && pklayers::CheckTimeSplice(4, many, 16) == 0, "well-formed: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(0, asc, 3) == PK_MI355_E_INVALID && Has(LastError(), "in_dim 0"), "in_dim 0: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(4, asc, 0) == PK_MI355_E_INVALID && Has(LastError(), "0 offsets, between 1 and 16"), "n 0: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(4, many, 17) == PK_MI355_E_INVALID && Has(LastError(), "17 offsets, between 1 and 16"), "n 17: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(4, nullptr, 2) == PK_MI355_E_INVALID, "null offsets");
    CHECK(pklayers::CheckTimeSplice(4, eq, 3) == PK_MI355_E_INVALID && Has(LastError(), "offset -1 (index 1) follows -1"), "equal: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(4, desc, 3) == PK_MI355_E_INVALID && Has(LastError(), "offset 1 (index 2) follows 2"), "descending: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(4, far, 2) == PK_MI355_E_INVALID && Has(LastError(), "offset 33 (index 1) is outside [-32, 32]"), "33: %s", LastError());
    CHECK(pklayers::CheckTimeSplice(4, near, 2) == PK_MI355_E_INVALID && Has(LastError(), "offset -33 (index 0) is outside [-32, 32]"), "-33: %s", LastError());
    CHECK(pk_mi355_time_splice_host(nullptr, 4, 2, asc, 3, y) == PK_MI355_E_INVALID && Has(LastError(), "null argument"), "null rows");
    CHECK(pk_mi355_time_splice_host(x, 4, 2, eq, 3, y) == PK_MI355_E_INVALID, "equal offsets through the entry");
    CHECK(pk_mi355_time_splice_host(x, -1, 2, asc, 3, y) == PK_MI355_E_INVALID, "negative rows");
  }

  // ---- the reader
  char tmpl[] = "/tmp/pk_time_splice_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("FAILED mkdtemp\n"); return 2; }
  g_dir = tmpl;
  std::vector<HostLayer> layers;
  const std::string whole = Nnt0(2) + Splice(10, {-1, 2}) + Splice(34, {-7, -3, 0, 3, 32});
  int rc = ReadBytes(whole, &layers);
  CHECK(rc == 0 && layers.size() == 2, "the well-formed file: %d (%s)", rc, LastError());
  if (layers.size() == 2) {
    CHECK(layers[0].type == PK_MI355_NNET_TIME_SPLICE_LAYER && layers[0].in_dim == 10 && layers[0].out_dim == 20 &&
              layers[0].offsets == std::vector<int32_t>({-1, 2}), "first layer");
    CHECK(layers[1].in_dim == 34 && layers[1].out_dim == 170 && layers[1].offsets == std::vector<int32_t>({-7, -3, 0, 3, 32}) && layers[1].W.empty() &&
              layers[1].b.empty(), "second layer");
  }
  for (size_t cut = 0; cut < whole.size(); ++cut) {        // every proper prefix
    rc = ReadBytes(whole.substr(0, cut), &layers);
    CHECK(rc == PK_MI355_E_IO, "cut at %zu of %zu: %d", cut, whole.size(), rc);
  }
  CHECK(ReadBytes(Nnt0(1) + Splice(0, {0}), &layers) == PK_MI355_E_IO && Has(LastError(), "width 0"), "in_dim 0: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(-4, {0}), &layers) == PK_MI355_E_IO, "in_dim -4");
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {}), &layers) == PK_MI355_E_IO && Has(LastError(), "0 offsets"), "n 0: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(4, std::vector<int32_t>(17, 0)), &layers) == PK_MI355_E_IO && Has(LastError(), "17 offsets"), "n 17: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {}, -2), &layers) == PK_MI355_E_IO, "n negative");
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {0, 1}, 16), &layers) == PK_MI355_E_IO && Has(LastError(), "16 time-splice offsets expected"),
        "more offsets stated than the file holds: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {1, 1}), &layers) == PK_MI355_E_IO && Has(LastError(), "out of order"), "equal: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {2, 1}), &layers) == PK_MI355_E_IO && Has(LastError(), "out of order"), "descending: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {33}), &layers) == PK_MI355_E_IO && Has(LastError(), "out of range"), "33: %s", LastError());
  CHECK(ReadBytes(Nnt0(1) + Splice(4, {-33}), &layers) == PK_MI355_E_IO && Has(LastError(), "out of range"), "-33: %s", LastError());
  unlink((g_dir + "/m.nnet").c_str());
  rmdir(g_dir.c_str());

  if (g_failures) { printf("%d failures\n", g_failures); return 1; }
  printf("time_splice_test ok\n");
  return 0;
}

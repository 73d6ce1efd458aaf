// files_stats_test.cc -- the model file of a model of any feature dimension (ReadModelConfigStats, csrc/pk_files.cc,
// DESIGN.md section 18) in a process of its own: no HIP, no library, no Python.  Built plain and with
// -fsanitize=address,undefined by tests/test_frontend_stream_host.py.
//
//   files_stats_test <scratch dir>
//
// It writes its own model files: the keys that are paths are never opened by this reader.  Cases: good cmvn_stats vectors
// of 14 and 81 floats; a vector longer than the capacity; a truncated vector; vectors whose length fields lie; and
// ReadModelConfig on the same files, which keeps its "41 expected".
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"

using namespace pkhost;
typedef std::vector<unsigned char> Bytes;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void Spit(const std::string &path, const Bytes &b) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || (!b.empty() && fwrite(b.data(), 1, b.size(), f) != b.size())) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}
static void PutI32(Bytes *b, int32_t v) { b->insert(b->end(), reinterpret_cast<unsigned char *>(&v), reinterpret_cast<unsigned char *>(&v) + 4); }

// a VEC0 whose fields say `bytes` and `n` and which holds `have` floats, entry i = i + 0.5
static Bytes Vec0(int32_t bytes, int32_t n, int have) {
  Bytes b = {'V', 'E', 'C', '0'};
  PutI32(&b, bytes);
  PutI32(&b, n);
  for (int i = 0; i < have; ++i) {
    const float v = i + 0.5f;
    b.insert(b.end(), reinterpret_cast<const unsigned char *>(&v), reinterpret_cast<const unsigned char *>(&v) + 4);
  }
  return b;
}
static Bytes Good(int n) { return Vec0(4 * n + 4, n, n); }

static bool Has(const char *text, const std::string &what) { return std::string(text).find(what) != std::string::npos; }

int main(int argc, char **argv) {
  if (argc != 2) { printf("usage: files_stats_test <scratch dir>\n"); return 2; }
  const std::string dir = argv[1], conf = dir + "/model.conf", stats = dir + "/stats.bin";
  const std::string text = "cmvn_stats = stats.bin\nnnet = am.nnet\nprior = am.prior\ntid2pdf = tid2pdf.bin\nleft_context = 2\n"
                           "right_context = 1\nnum_pdfs = 18\n";
  Spit(conf, Bytes(text.begin(), text.end()));

  // ---- good vectors of 14 and 81 floats
  for (int n : {14, 81, 129, 1}) {
    Spit(stats, Good(n));
    ModelConfig c;
    const int rc = ReadModelConfigStats(conf.c_str(), 129, &c);
    CHECK(rc == 0, "%d floats: code %d (%s)", n, rc, LastError());
    CHECK((int)c.stats.size() == n && c.cmvn_path == stats, "%d floats: %d read from %s", n, (int)c.stats.size(), c.cmvn_path.c_str());
    for (int i = 0; i < (int)c.stats.size(); ++i) CHECK(c.stats[i] == i + 0.5f, "%d floats: entry %d", n, i);
    CHECK(c.left == 2 && c.right == 1 && c.num_pdfs == 18 && c.nnet == dir + "/am.nnet", "%d floats: the other keys", n);
    printf("good %d ok\n", n);
    // the reference's reader keeps its refusal, word for word
    ModelConfig c41;
    const int rc41 = ReadModelConfig(conf.c_str(), &c41);
    char want[512];
    snprintf(want, sizeof(want), "cmvn_stats in %s has %d entries, 41 expected", stats.c_str(), n);
    CHECK(rc41 == PK_MI355_E_IO && std::string(LastError()) == want, "ReadModelConfig on %d floats: %d '%s'", n, rc41, LastError());
  }
  {
    Spit(stats, Good(41));
    ModelConfig c, c41;
    CHECK(ReadModelConfig(conf.c_str(), &c41) == 0 && c41.cmvn_stats[40] == 40.5f, "ReadModelConfig on 41 floats");
    CHECK(ReadModelConfigStats(conf.c_str(), 41, &c) == 0 && c.stats.size() == 41 && c.stats[40] == 40.5f, "41 floats at capacity 41");
  }

  // ---- longer than the capacity: E_IO, both numbers and the file named
  for (int cap : {13, 80, 129}) {
    const int n = cap + 1;
    Spit(stats, Good(n));
    ModelConfig c;
    const int rc = ReadModelConfigStats(conf.c_str(), cap, &c);
    CHECK(rc == PK_MI355_E_IO, "%d floats at capacity %d: code %d", n, cap, rc);
    CHECK(Has(LastError(), std::to_string(n)) && Has(LastError(), std::to_string(cap)) && Has(LastError(), stats), "%d over %d: '%s'", n, cap,
          LastError());
    CHECK(c.stats.empty(), "a refused vector is not handed out");
  }
  {
    Spit(stats, Good(0));
    ModelConfig c;
    CHECK(ReadModelConfigStats(conf.c_str(), 129, &c) == PK_MI355_E_IO && Has(LastError(), "0 entries"), "an empty vector: '%s'", LastError());
    CHECK(ReadModelConfigStats(conf.c_str(), 0, &c) == PK_MI355_E_INVALID, "capacity 0");
    CHECK(ReadModelConfigStats(conf.c_str(), -5, &c) == PK_MI355_E_INVALID, "capacity -5");
  }
  printf("capacity ok\n");

  // ---- truncated: the fields say 81 floats, the file holds fewer (every count from none to 80, and a cut inside a float)
  for (int have = 0; have <= 80; ++have) {
    Spit(stats, Vec0(4 * 81 + 4, 81, have));
    ModelConfig c;
    const int rc = ReadModelConfigStats(conf.c_str(), 129, &c);
    CHECK(rc == PK_MI355_E_IO && Has(LastError(), "corrupted VEC0"), "81 stated, %d held: %d '%s'", have, rc, LastError());
  }
  {
    Bytes b = Good(81);
    for (int cut : {1, 2, 3, 5, 320}) {
      Spit(stats, Bytes(b.begin(), b.end() - cut));
      ModelConfig c;
      CHECK(ReadModelConfigStats(conf.c_str(), 129, &c) == PK_MI355_E_IO, "81 floats less %d bytes", cut);
    }
    for (int keep : {0, 3, 4, 7, 8, 11}) {                 // inside the header
      Spit(stats, Bytes(b.begin(), b.begin() + keep));
      ModelConfig c;
      CHECK(ReadModelConfigStats(conf.c_str(), 129, &c) == PK_MI355_E_IO, "the first %d bytes", keep);
    }
  }
  printf("truncated ok\n");

  // ---- length-poisoned: fields no file could back, and fields that disagree, around 14 real floats
  const int32_t hostile[] = {-1, -2147483647 - 1, 2147483647, 0x40000000, 0x3FFFFFFF, 0x20000000, 1073741825, 536870913, 82, 15, 13, 0};
  int cases = 0;
  for (int32_t n : hostile)
    for (int32_t bytes : {4 * 14 + 4, (int32_t)(4u * (uint32_t)n + 4u), n, 0, -1, 2147483647}) {       // (4 n + 4 as the format's 32 bits wrap it)
      if (n == 13 && bytes == 4 * 13 + 4) continue;        // (a well-formed 13-float vector with one float behind it)
      Spit(stats, Vec0(bytes, n, 14));
      ModelConfig c;
      const int rc = ReadModelConfigStats(conf.c_str(), 129, &c);
      const bool fine = n == 0 && bytes == 4;              // an empty vector, well-formed: refused for its length
      CHECK(rc == PK_MI355_E_IO && (fine || Has(LastError(), "corrupted VEC0")), "n %d bytes %d: %d '%s'", n, bytes, rc, LastError());
      CHECK(c.stats.empty(), "n %d bytes %d: a refused vector is not handed out", n, bytes);
      ++cases;
    }
  printf("poisoned %d ok\n", cases);

  // ---- a missing key, a missing file
  {
    Spit(conf, Bytes(text.begin() + text.find('\n') + 1, text.end()));
    ModelConfig c;
    CHECK(ReadModelConfigStats(conf.c_str(), 129, &c) == PK_MI355_E_IO && Has(LastError(), "Unable to find key 'cmvn_stats'"), "'%s'", LastError());
    const std::string other = "cmvn_stats = nowhere.bin\n" + text.substr(text.find('\n') + 1);
    Spit(conf, Bytes(other.begin(), other.end()));
    CHECK(ReadModelConfigStats(conf.c_str(), 129, &c) == PK_MI355_E_IO && Has(LastError(), "cannot open"), "'%s'", LastError());
  }
  if (g_failures) { printf("files_stats_test: %d FAILED\n", g_failures); return 1; }
  printf("files_stats_test ok\n");
  return 0;
}

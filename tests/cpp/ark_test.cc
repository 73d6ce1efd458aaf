// ark_test.cc -- the Kaldi archive reader (csrc/pk_ark.cc) in a process of its own: no HIP, no library, no Python.
// Built plain and with -fsanitize=address,undefined by tests/test_ark_host.py.
//
//   ark_test <scratch dir> <three-entry archive> <spec> [<spec> ...]
//
// 1. positive: every spec read entry by entry and printed as key, dims and the 64-bit FNV-1a of the float bytes (the
//    test compares them with what its own writer put in);
// 2. truncation sweep: every prefix of the three-entry archive must yield whole entries -- the archive's own, bit for
//    bit -- and then 0 or PK_MI355_E_IO;
// 3. header-field sweep: rows or cols of -1, 2^31 - 1 and 2^30 x 2^30, size bytes 0 and 8, an scp offset past the end;
//    double matrices too: 2^31 - 1 squared, and dimensions whose count x 8 wraps in 64 bits to fewer bytes than the file holds.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"

typedef std::vector<unsigned char> Bytes;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static unsigned long long Fnv(const void *p, size_t n) {
  unsigned long long h = 14695981039346656037ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 1099511628211ull;
  return h;
}

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
  if (!f || (!b.empty() && fwrite(b.data(), 1, b.size(), f) != b.size())) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

struct Entry { std::string key; int rows, cols; unsigned long long hash; };

// Reads `spec` to its end: the entries, and the code that ended the reading (0 or negative; -100: it could not be opened).
static int ReadAll(const std::string &spec, std::vector<Entry> *out) {
  out->clear();
  pk_mi355_ark_t *h = pk_mi355_ark_open(spec.c_str());
  if (!h) return -100 + pk_mi355_last_error_code();
  int rc;
  while ((rc = pk_mi355_ark_next(h)) == 1) {
    pk_matrix_t m;
    CHECK(pk_mi355_ark_matrix(h, &m) == 0, "matrix of a current entry");
    out->push_back({pk_mi355_ark_key(h), m.ncol, m.nrow, Fnv(m.data, sizeof(float) * (size_t)m.ncol * (size_t)m.nrow)});
  }
  if (rc < 0) CHECK(pk_mi355_ark_next(h) == rc, "the code is repeated");
  pk_mi355_ark_close(h);
  return rc;
}

static Bytes BinaryEntry(const std::string &key, unsigned char size_rows, int32_t rows, unsigned char size_cols, int32_t cols, size_t payload,
                         char type = 'F') {
  Bytes b(key.begin(), key.end());
  b.push_back(' '); b.push_back(0); b.push_back('B'); b.push_back((unsigned char)type); b.push_back('M'); b.push_back(' ');
  for (int i = 0; i < 2; ++i) {
    b.push_back(i ? size_cols : size_rows);
    const uint32_t v = (uint32_t)(i ? cols : rows);
    for (int k = 0; k < 4; ++k) b.push_back((unsigned char)(v >> (8 * k)));
  }
  b.resize(b.size() + payload, 0x3f);
  return b;
}

int main(int argc, char **argv) {
  if (argc < 4) { printf("usage: ark_test <scratch dir> <three-entry archive> <spec> ...\n"); return 2; }
  const std::string scratch = argv[1], three = argv[2];
  std::vector<Entry> got;

  // 1. positive
  for (int i = 3; i < argc; ++i) {
    const int rc = ReadAll(argv[i], &got);
    for (const Entry &e : got) printf("entry %s %d %d %016llx\n", e.key.c_str(), e.rows, e.cols, e.hash);
    printf("end %s %d\n", argv[i], rc);
  }

  // 2. truncation sweep
  std::vector<Entry> whole;
  CHECK(ReadAll(three, &whole) == 0 && whole.size() == 3, "the three-entry archive reads to its end");
  const Bytes all = Slurp(three);
  int ended_clean = 0, ended_io = 0;
  const std::string cut = scratch + "/prefix.ark";
  for (size_t n = 0; n <= all.size(); ++n) {
    Spit(cut, Bytes(all.begin(), all.begin() + n));
    const int rc = ReadAll(cut, &got);
    CHECK(rc == 0 || rc == PK_MI355_E_IO, "prefix %zu ends in %d", n, rc);
    CHECK(got.size() <= whole.size(), "prefix %zu yields %zu entries", n, got.size());
    for (size_t k = 0; k < got.size() && k < whole.size(); ++k)
      CHECK(got[k].key == whole[k].key && got[k].rows == whole[k].rows && got[k].cols == whole[k].cols && got[k].hash == whole[k].hash,
            "prefix %zu entry %zu is not the archive's", n, k);
    (rc == 0 ? ended_clean : ended_io) += 1;
  }
  printf("sweep prefixes %zu clean %d io %d\n", all.size() + 1, ended_clean, ended_io);

  // 3. header fields
  const int32_t big = 0x7fffffff, gib = 1 << 30;
  // (2^30 + 23170) x (2^31 - 46339) = 2^61 + 67194 values: times 8 that is 537552 modulo 2^64, less than the payload
  const int32_t wrap_rows = gib + 23170, wrap_cols = big - 46338;
  struct Case { const char *name; unsigned char sr; int32_t rows; unsigned char sc; int32_t cols; size_t payload; int want; char type; };
  const Case cases[] = {
      {"DM 2^31-1 x 2^31-1", 4, big, 4, big, 64, PK_MI355_E_IO, 'D'},
      {"DM count x 8 wraps", 4, wrap_rows, 4, wrap_cols, 600000, PK_MI355_E_IO, 'D'},
      {"DM 2^30 x 2^30", 4, gib, 4, gib, 64, PK_MI355_E_IO, 'D'},
      {"DM healthy 2 x 3", 4, 2, 4, 3, 48, 0, 'D'},
      {"rows -1", 4, -1, 4, 3, 64, PK_MI355_E_IO, 'F'},         {"cols -1", 4, 3, 4, -1, 64, PK_MI355_E_IO, 'F'},
      {"rows 2^31-1", 4, big, 4, 3, 64, PK_MI355_E_IO, 'F'},    {"cols 2^31-1", 4, 3, 4, big, 64, PK_MI355_E_IO, 'F'},
      {"2^30 x 2^30", 4, gib, 4, gib, 64, PK_MI355_E_IO, 'F'},  {"2^31-1 x 2^31-1", 4, big, 4, big, 64, PK_MI355_E_IO, 'F'},
      {"size byte 0 (rows)", 0, 2, 4, 3, 24, PK_MI355_E_IO, 'F'}, {"size byte 8 (rows)", 8, 2, 4, 3, 24, PK_MI355_E_IO, 'F'},
      {"size byte 0 (cols)", 4, 2, 0, 3, 24, PK_MI355_E_IO, 'F'}, {"size byte 8 (cols)", 4, 2, 8, 3, 24, PK_MI355_E_IO, 'F'},
      {"healthy 2 x 3", 4, 2, 4, 3, 24, 0, 'F'},                {"0 x 2^31-1", 4, 0, 4, big, 0, 0, 'F'},
  };
  const std::string field = scratch + "/field.ark";
  for (const Case &c : cases) {
    Spit(field, BinaryEntry("k", c.sr, c.rows, c.sc, c.cols, c.payload, c.type));
    const int rc = ReadAll(field, &got);
    CHECK(rc == c.want, "%s: %d", c.name, rc);
    printf("field %s: %d\n", c.name, rc);
  }
  {
    Spit(field, BinaryEntry("k", 4, 2, 4, 3, 24));
    const std::string scp = scratch + "/offset.scp";
    const std::string good = "a " + field + ":2\n", past = "a " + field + ":2\nb " + field + ":100000\n";
    Spit(scp, Bytes(good.begin(), good.end()));
    CHECK(ReadAll(scp, &got) == 0 && got.size() == 1 && got[0].rows == 2 && got[0].cols == 3, "scp with an offset");
    Spit(scp, Bytes(past.begin(), past.end()));
    const int rc = ReadAll(scp, &got);
    CHECK(rc == PK_MI355_E_IO && got.size() == 1, "scp offset past the end: %d after %zu entries", rc, got.size());
    printf("field scp offset past the end: %d\n", rc);
    pk_mi355_ark_t *one = pk_mi355_ark_read_object((field + ":2").c_str());
    pk_matrix_t m;
    CHECK(one && pk_mi355_ark_matrix(one, &m) == 0 && m.ncol == 2 && m.nrow == 3 && pk_mi355_ark_next(one) == 0, "one keyless object");
    pk_mi355_ark_close(one);
    CHECK(pk_mi355_ark_read_object((field + ":100000").c_str()) == nullptr && pk_mi355_last_error_code() == PK_MI355_E_IO, "object offset past the end");
  }
  // null arguments
  {
    pk_matrix_t m;
    CHECK(pk_mi355_ark_open(nullptr) == nullptr && pk_mi355_ark_read_object(nullptr) == nullptr, "null spec");
    CHECK(pk_mi355_ark_next(nullptr) == PK_MI355_E_INVALID && pk_mi355_ark_matrix(nullptr, &m) == PK_MI355_E_INVALID, "null handle");
    CHECK(std::string(pk_mi355_ark_key(nullptr)).empty(), "null handle's key");
    pk_mi355_ark_close(nullptr);
  }
  if (g_failures) { printf("ark_test FAILED (%d)\n", g_failures); return 1; }
  printf("ark_test ok\n");
  return 0;
}

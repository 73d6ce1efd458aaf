// symtab_test.cc -- the symbol-table reader and the word-segment function (csrc/pk_files.cc) in a process of their
// own: no HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by tests/test_symtab_host.py.
//
//   symtab_test <golden dir> <scratch dir>
//
// 1. positive: both symbol-table fixtures, every string printed (the test compares them with an independent parse);
// 2. sweep: every 4-byte header field (section size, size, buffer_size, every offset) overwritten with each of the eight
//    hostile values of files_test.cc, the file cut at every length, an offset == buffer_size and a buffer without its
//    final NUL; each variant must end in 0, E_INVALID or E_IO;
// 3. segments: WordSegments on hand-written paths over a hand-written graph, printed with the costs' bit patterns.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"

using namespace pkhost;
typedef std::vector<unsigned char> Bytes;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

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

static const int32_t kValues[8] = {0, 1, -1, 1 << 20, 1 << 29, 1 << 30, INT32_MAX, INT32_MIN};

// a table that reads is also walked: every string through the public getter, and the ids either side of the range
static int RunSymtab(const char *path) {
  pk_mi355_symtab_t *st = pk_mi355_symtab_read(path);
  if (!st) return pk_mi355_last_error_code();
  const int n = pk_mi355_symtab_size(st);
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const char *s = pk_mi355_symtab_get(st, i);
    CHECK(s, "symbol %d of %d: %s", i, n, LastError());
    if (s) total += strlen(s);
  }
  CHECK(total <= st->buffer.size(), "strings longer than the buffer");
  CHECK(!pk_mi355_symtab_get(st, -1) && pk_mi355_last_error_code() == PK_MI355_E_INVALID, "id -1");
  CHECK(!pk_mi355_symtab_get(st, n) && pk_mi355_last_error_code() == PK_MI355_E_INVALID, "id size");
  pk_mi355_symtab_destroy(st);
  return 0;
}

static int One(const std::string &variant, const Bytes &b, const char *name, const char *what, size_t at, long long v) {
  Spit(variant, b);
  Fail(0, "%s", "");       // the error text is the thread's last: empty it, so that a failure has to set its own
  const int rc = RunSymtab(variant.c_str());
  CHECK(rc == 0 || rc == PK_MI355_E_INVALID || rc == PK_MI355_E_IO, "%s: %s at %zu (%lld): code %d", name, what, at, v, rc);
  CHECK(rc == 0 || LastError()[0] != '\0', "%s: %s at %zu (%lld): no error text", name, what, at, v);
  return rc;
}

static void Sweep(const char *name, const Bytes &good, const std::string &variant) {
  std::set<int> codes;
  int cases = 0;
  const size_t size = (size_t)I32At(good, 8), buffer_size = (size_t)I32At(good, 12);
  std::vector<size_t> fields = {4, 8, 12};
  for (size_t i = 0; i < size; ++i) fields.push_back(16 + 4 * i);
  for (size_t off : fields)
    for (int32_t v : kValues) {
      Bytes b = good;
      PutI32(&b, off, v);
      codes.insert(One(variant, b, name, "field", off, v));
      ++cases;
    }
  for (size_t len = 0; len <= good.size() + 1; ++len) {
    Bytes b = good;
    b.resize(len, 0);       // (one byte past the end of the file: a zero byte more)
    const int rc = One(variant, b, name, "cut", len, 0);
    CHECK(len >= good.size() || rc == PK_MI355_E_IO, "%s: cut at %zu: code %d", name, len, rc);
    codes.insert(rc);
    ++cases;
  }
  printf("sweep %s fields %zu cases %d codes", name, fields.size(), cases);
  for (int c : codes) printf(" %d", c);
  printf("\n");
  if (size > 0) {
    Bytes b = good;
    PutI32(&b, 16 + 4 * (size - 1), (int32_t)buffer_size);
    printf("case %s offset_eq_buffer_size: %d\n", name, One(variant, b, name, "offset", 16 + 4 * (size - 1), (long long)buffer_size));
  }
  if (buffer_size > 0) {
    Bytes b = good;
    b.back() = 'x';
    printf("case %s no_final_nul: %d\n", name, One(variant, b, name, "nul", b.size() - 1, 'x'));
  }
}

static void PrintTable(const char *name, const std::string &path) {
  pk_mi355_symtab_t *st = pk_mi355_symtab_read(path.c_str());
  CHECK(st, "%s: %s", name, LastError());
  if (!st) return;
  printf("symtab %s size %d\n", name, pk_mi355_symtab_size(st));
  for (int i = 0; i < pk_mi355_symtab_size(st); ++i) printf("sym %s %d %s\n", name, i, pk_mi355_symtab_get(st, i));
  pk_mi355_symtab_destroy(st);
}

static unsigned Bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

static void Segments(const char *name, const ArcLabels &g, const std::vector<int32_t> &path, const std::vector<float> *ac) {
  const int n = WordSegments(g, path.data(), (int)path.size(), ac ? ac->data() : nullptr, ac ? (int)ac->size() : 0, nullptr, 0);
  std::vector<pk_mi355_word_t> seg(n + 1);
  const int again = WordSegments(g, path.data(), (int)path.size(), ac ? ac->data() : nullptr, ac ? (int)ac->size() : 0, seg.data(), n);
  CHECK(again == n, "%s: %d segments, then %d", name, n, again);
  printf("segments %s %d", name, n);
  for (int i = 0; i < n; ++i)
    printf(" | %d %d %d %08x %08x", seg[i].word, seg[i].start_frame, seg[i].num_frames, Bits(seg[i].graph_cost), Bits(seg[i].acoustic_cost));
  printf("\n");
  if (n > 1) {               // a short output buffer: the count is still returned, nothing behind max is written
    std::vector<pk_mi355_word_t> few(2, pk_mi355_word_t{-7, -7, -7, 0.0f, 0.0f});
    CHECK(WordSegments(g, path.data(), (int)path.size(), nullptr, 0, few.data(), 1) == n && few[1].word == -7, "%s: max 1", name);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) { printf("usage: symtab_test <golden dir> <scratch dir>\n"); return 2; }
  const std::string G = argv[1], S = argv[2], V = S + "/variant.bin";
  const std::string files[2][2] = {{"symboltable_test.bin", G + "/symboltable_test.bin"},
                                   {"wordloop_words.bin", G + "/refmodel/wordloop_words.bin"}};
  for (const auto &f : files) PrintTable(f[0].c_str(), f[1]);
  for (const auto &f : files) Sweep(f[0].c_str(), Slurp(f[1]), V);
  {
    pk_mi355_symtab st;      // a directory opens, and has no bytes; a missing file does not open
    int rc = ReadSymtab(S.c_str(), &st);
    if (rc == PK_MI355_E_IO) rc = ReadSymtab((S + "/absent.bin").c_str(), &st);
    printf("case directory_and_missing: %d\n", rc);
    Bytes empty_table(16, 0);                           // size 0, buffer_size 0: a table without symbols reads
    memcpy(&empty_table[0], "SYM0", 4);
    PutI32(&empty_table, 4, 8);
    printf("case empty_table: %d\n", One(V, empty_table, "empty", "table", 0, 0));
  }

  // ---- segments: arcs 0..6 as (ilabel, olabel, weight)
  ArcLabels g;
  g.ilabel = {0, 3, 0, 4, 2, 1, 0};
  g.olabel = {0, 0, 5, 6, 7, 0, 8};
  g.weight = {0.25f, 0.5f, 0.125f, 1.5f, 0.1f, 0.2f, 0.3f};
  const std::vector<float> ac = {1.0f, 2.5f, 0.3f, 0.7f};
  Segments("eps_olabel", g, {1, 2, 3, 5}, &ac);
  Segments("two_olabels_no_frame", g, {3, 2, 6, 5, 4}, &ac);
  Segments("leading_eps", g, {0, 0, 1, 3, 4}, &ac);
  Segments("no_olabel", g, {0, 1, 5, 1, 0}, &ac);
  Segments("empty", g, {}, &ac);
  Segments("no_ac", g, {1, 2, 3, 5}, nullptr);
  if (g_failures) printf("symtab_test FAILED (%d)\n", g_failures);
  else printf("symtab_test ok\n");
  return g_failures ? 1 : 0;
}

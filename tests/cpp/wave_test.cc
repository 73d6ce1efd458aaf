// wave_test.cc -- the any-rate WAV reader (csrc/pk_files.cc: ReadWave, pk_mi355_wave_read) and the resampler's table
// builder (csrc/pk_tables.cc) in a process of their own: no HIP, no library, no Python.  Built plain and with
// -fsanitize=address,undefined by tests/test_wave_host.py.
//
//   wave_test <scratch dir> <wave file> ...
//
// 1. every wave file named (the test wrote them: 1 / 2 / 8 channels, 8 / 16 / 32 bits), every channel: rate, channel
//    count, sample count and the FNV-1a of the float samples' bytes (the test compares with its own de-interleaving);
// 2. sweep over the first file named: every header field overwritten with each of eight hostile values, and the file cut
//    at every length 0 .. len + 1; each variant must end in 0, E_INVALID or E_IO;
// 3. the named cases: a payload that is not a multiple of block_align, a channel outside the file, a 16 kHz mono file
//    through both readers;
// 4. the table builder for every rate 7990 .. 96010: every supported rate's table inside its own bounds.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"
#include "../../pocketkaldi_amd/csrc/pk_resample.h"

using namespace pkhost;
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
  if (!f || fwrite(b.data(), 1, b.size(), f) != b.size()) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}
static void Put(Bytes *b, size_t off, int64_t v, int width) { memcpy(&(*b)[off], &v, width); }   // little-endian host

// a well-formed file: header + interleaved payload of `frames` blocks (+ `extra` stray bytes), sample = 3 i + 7 c - 50
static Bytes MakeWave(int channels, int bits, int rate, int frames, int extra) {
  const int width = bits / 8, align = channels * width;
  const int payload = frames * align + extra;
  Bytes b(44 + payload, 0);
  memcpy(&b[0], "RIFF", 4); Put(&b, 4, 36 + payload, 4); memcpy(&b[8], "WAVEfmt ", 8);
  Put(&b, 16, 16, 4); Put(&b, 20, 1, 2); Put(&b, 22, channels, 2); Put(&b, 24, rate, 4);
  Put(&b, 28, (int64_t)rate * align, 4); Put(&b, 32, align, 2); Put(&b, 34, bits, 2);
  memcpy(&b[36], "data", 4); Put(&b, 40, payload, 4);
  for (int i = 0; i < frames; ++i)
    for (int c = 0; c < channels; ++c) Put(&b, 44 + (size_t)i * align + c * width, 3 * i + 7 * c - 50, width);
  return b;
}

int main(int argc, char **argv) {
  if (argc < 3) { printf("usage: wave_test <scratch dir> <wave file> ...\n"); return 2; }
  const std::string S = argv[1];

  // ---- 1. the files of the test, every channel
  for (int a = 2; a < argc; ++a) {
    int rate = 0, channels = 0;
    std::vector<float> s;
    CHECK(ReadWave(argv[a], 0, &s, &rate, &channels) == 0, "%s: %s", argv[a], LastError());
    for (int c = 0; c < channels; ++c) {
      pk_vector_t v = {0, nullptr};
      int r2 = 0, c2 = 0;
      CHECK(pk_mi355_wave_read(argv[a], c, &v, &r2, &c2) == 0, "%s", LastError());
      CHECK(r2 == rate && c2 == channels, "header fields differ between channels");
      printf("wave %s ch %d rate %d channels %d n %d fnv %016llx\n", argv[a], c, r2, c2, v.dim, Fnv(v.data, sizeof(float) * v.dim));
      free(v.data);
    }
    CHECK(ReadWave(argv[a], channels, &s, nullptr, nullptr) == PK_MI355_E_INVALID, "channel == channels accepted");
    CHECK(ReadWave(argv[a], -1, &s, nullptr, nullptr) == PK_MI355_E_INVALID, "channel -1 accepted");
  }

  // ---- 2. sweep over the first file
  {
    const Bytes good = Slurp(argv[2]);
    const std::string path = S + "/sweep.wav";
    struct Field { size_t off; int width; };
    const Field fields[] = {{4, 4}, {16, 4}, {20, 2}, {22, 2}, {24, 4}, {28, 4}, {32, 2}, {34, 2}, {40, 4}};
    const int64_t hostile[] = {0, 1, -1, 2, 9, 0x7FFFFFFF, (int64_t)0x80000000u, 0x7FFF};
    std::set<int> codes;
    int cases = 0;
    std::vector<float> s;
    for (const Field &f : fields)
      for (int64_t v : hostile) {
        Bytes b = good;
        Put(&b, f.off, v, f.width);
        Spit(path, b);
        for (int ch : {0, 1}) { codes.insert(ReadWave(path.c_str(), ch, &s, nullptr, nullptr)); ++cases; }
      }
    for (size_t len = 0; len <= good.size() + 1; ++len) {
      Bytes b = good;
      b.resize(len, 0);
      Spit(path, b);
      codes.insert(ReadWave(path.c_str(), 0, &s, nullptr, nullptr));
      ++cases;
    }
    printf("sweep fields %zu cases %d codes", sizeof(fields) / sizeof(fields[0]), cases);
    for (int c : codes) printf(" %d", c);
    printf("\n");
    for (int c : codes) CHECK(c == 0 || c == PK_MI355_E_INVALID || c == PK_MI355_E_IO, "code %d", c);
  }

  // ---- 3. named cases
  {
    const std::string path = S + "/case.wav";
    std::vector<float> s, s16;
    int rate = 0, channels = 0;
    // a payload of 10 stereo 16-bit blocks and 3 stray bytes: the whole blocks are read, nothing behind them
    Spit(path, MakeWave(2, 16, 44100, 10, 3));
    int rc = ReadWave(path.c_str(), 1, &s, &rate, &channels);
    printf("case ragged_payload: %d n %zu\n", rc, s.size());
    CHECK(rc == 0 && s.size() == 10 && rate == 44100 && channels == 2, "ragged payload");
    for (size_t i = 0; i < s.size(); ++i) CHECK(s[i] == (float)(3 * (int)i + 7 - 50), "sample %zu", i);
    // a truncated payload whose sizes were NOT fixed up is refused by the size checks
    Bytes cut = MakeWave(2, 16, 44100, 10, 0);
    cut.resize(cut.size() - 5);
    Spit(path, cut);
    printf("case truncated_payload: %d\n", ReadWave(path.c_str(), 0, &s, nullptr, nullptr));
    // nine channels, zero channels
    for (int ch : {0, 9}) {
      Bytes b = MakeWave(2, 16, 8000, 4, 0);
      Put(&b, 22, ch, 2);
      Spit(path, b);
      printf("case channels_%d: %d\n", ch, ReadWave(path.c_str(), 0, &s, nullptr, nullptr));
    }
    // byte_rate and block_align of a mono file in a stereo header
    Bytes b = MakeWave(2, 16, 48000, 4, 0);
    Put(&b, 28, 48000 * 2, 4);
    Spit(path, b);
    printf("case mono_byte_rate: %d\n", ReadWave(path.c_str(), 0, &s, nullptr, nullptr));
    b = MakeWave(2, 16, 48000, 4, 0);
    Put(&b, 32, 2, 2);
    Spit(path, b);
    printf("case mono_block_align: %d\n", ReadWave(path.c_str(), 0, &s, nullptr, nullptr));
    // 16 kHz mono, every width: both readers give the same samples
    for (int bits : {8, 16, 32}) {
      Spit(path, MakeWave(1, bits, 16000, 33, 0));
      CHECK(ReadWave(path.c_str(), 0, &s, &rate, &channels) == 0 && ReadWav16k(path.c_str(), &s16) == 0, "%s", LastError());
      CHECK(rate == 16000 && channels == 1 && s.size() == 33 && s == s16, "16 kHz mono, %d bits", bits);
      printf("case mono16k_%d: same %d\n", bits, (int)(s == s16));
    }
    // what the strict reader refuses, the other one reads
    Spit(path, MakeWave(2, 16, 16000, 5, 0));
    printf("case strict_stereo: %d %d\n", ReadWav16k(path.c_str(), &s16), ReadWave(path.c_str(), 1, &s, nullptr, nullptr));
    Spit(path, MakeWave(1, 16, 8000, 5, 0));
    printf("case strict_rate: %d %d\n", ReadWav16k(path.c_str(), &s16), ReadWave(path.c_str(), 0, &s, nullptr, nullptr));
    pk_vector_t v = {0, nullptr};
    printf("case null_arguments: %d %d\n", pk_mi355_wave_read(nullptr, 0, &v, nullptr, nullptr), pk_mi355_wave_read(path.c_str(), 0, nullptr, nullptr, nullptr));
  }

  // ---- 4. the table builder, every rate
  {
    int supported = 0, largest = 0, largest_rate = 0;
    for (int rate = 7990; rate <= 96010; ++rate) {
      pkmi::ResampleTable t;
      int q = 0, p = 0, taps = 0;
      const int rc = pkmi::BuildResampleTable(rate, &t);
      CHECK((rc == 0) == (pk_mi355_resample_plan(rate, &q, &p, &taps) == 0), "rate %d: plan and builder disagree", rate);
      if (rc) { CHECK(pk_mi355_resample_num_output(rate, 5) == PK_MI355_E_INVALID, "rate %d", rate); continue; }
      ++supported;
      CHECK(rate >= 8000 && rate <= 96000 && q == t.Q && p == t.P && taps == t.max_taps, "rate %d", rate);
      CHECK((int64_t)t.Q * 16000 == (int64_t)t.P * rate && t.P * t.max_taps <= pkmi::kResampleMaxEntries, "rate %d", rate);
      CHECK((int)t.first.size() == t.P && (int)t.count.size() == t.P && (int)t.weights.size() == t.P * t.max_taps, "rate %d", rate);
      double worst = 0;
      for (int ph = 0; ph < t.P; ++ph) {
        CHECK(t.count[ph] >= 1 && t.count[ph] <= t.max_taps && t.first[ph] >= t.min_first && t.first[ph] + t.count[ph] <= t.max_end, "rate %d phase %d", rate, ph);
        double sum = 0;
        for (int k = 0; k < t.max_taps; ++k) {
          const float w = t.weights[(size_t)ph * t.max_taps + k];
          CHECK(k < t.count[ph] || w == 0.0f, "rate %d phase %d: padding is not zero", rate, ph);
          sum += w;
        }
        worst = std::max(worst, sum > 1 ? sum - 1 : 1 - sum);
      }
      CHECK(rate == 16000 || (worst > 0 && worst < 2e-3), "rate %d: phase sums off by %g", rate, worst);
      CHECK(t.Span() >= t.max_end - t.min_first && t.Span() <= 9000, "rate %d: span %d", rate, t.Span());
      CHECK(pk_mi355_resample_num_output(rate, t.Q) == t.P, "rate %d", rate);
      if (t.P * t.max_taps > largest) { largest = t.P * t.max_taps; largest_rate = rate; }
    }
    printf("tables supported %d largest %d at %d\n", supported, largest, largest_rate);
  }

  if (g_failures) { printf("wave_test: %d failure(s)\n", g_failures); return 1; }
  printf("wave_test ok\n");
  return 0;
}

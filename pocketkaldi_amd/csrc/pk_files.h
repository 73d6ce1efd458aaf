// pk_files.h -- everything of libpk_mi355.so that reads a caller's file, and the error state those readers report
// through (pk_files.cc).  Plain C++: no HIP header, compiled by g++ like pk_tables.cc, so the readers also build into
// a stand-alone program that runs under the host sanitizers (tests/cpp/files_test.cc).  Internal, like pk_host.h.
#ifndef PK_FILES_H_
#define PK_FILES_H_

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/pk_mi355.h"

namespace pkhost {

// ------------------------------------------------------------------ errors

// formats the thread's error text (pk_mi355_last_error) and returns `code`
int Fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const char *LastError();

// ------------------------------------------------------------------ section files
// "VEC0" i32 bytes(=4n+4) i32 n, n x 4 bytes (vector.cc:393-425);
// "MAT0" i32 8, i32 rows, i32 cols, rows x VEC0 (matrix.cc:288-319);
// "NNT0" i32 4, i32 layers; "LAY0" i32 4, i32 type [+ MAT0 W, VEC0 b] (nnet.cc:80-147);
// beyond the reference's reader: type 4 / 5 + VEC0 v, type 8 + i32 in_dim, i32 out_dim, types 6 / 7 bare;
// (section 29) type 9 + i32 in_dim, i32 n, n x i32 offset

struct FileBuf {
  std::vector<unsigned char> d;
  size_t pos = 0;
  std::string path;
  int Open(const char *p) {
    path = p;
    FILE *f = fopen(p, "rb");
    if (!f) return Fail(PK_MI355_E_IO, "cannot open %s", p);
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    // n is what the file system says (2^63 - 1 for a directory, -1 for a pipe): the buffer grows with the bytes read
    unsigned char buf[65536];
    size_t got = 1;
    while (got > 0 && (long)d.size() < n) {
      got = fread(buf, 1, (size_t)std::min<long>(sizeof(buf), n - (long)d.size()), f);
      d.insert(d.end(), buf, buf + got);
    }
    fclose(f);
    if ((long)d.size() != n) return Fail(PK_MI355_E_IO, "short read on %s", p);
    return 0;
  }
  bool Tag(const char *t) {
    if (pos + 4 > d.size() || memcmp(&d[pos], t, 4) != 0) return false;
    pos += 4;
    return true;
  }
  bool I32(int32_t *v) {
    if (pos + 4 > d.size()) return false;
    memcpy(v, &d[pos], 4);
    pos += 4;
    return true;
  }
  template <typename T>
  int Vec(std::vector<T> *out) {
    int32_t bytes, n;
    if (!Tag("VEC0") || !I32(&bytes) || !I32(&n))
      return Fail(PK_MI355_E_IO, "VEC0 section expected in %s", path.c_str());
    if (n < 0 || bytes != (int64_t)n * 4 + 4 || (uint64_t)n * 4 > d.size() - pos)   // (4 n + 4 leaves 32 bits from n = 2^29)
      return Fail(PK_MI355_E_IO, "corrupted VEC0 section in %s", path.c_str());
    out->resize(n);
    if (n) memcpy(out->data(), &d[pos], (size_t)n * 4);
    pos += (size_t)n * 4;
    return 0;
  }
};

// a file that is one VEC0
template <typename T>
int ReadVec(const char *path, std::vector<T> *out) {
  FileBuf f;
  int rc = f.Open(path);
  return rc ? rc : f.Vec(out);
}

struct HostLayer {
  int type = 0;
  int in_dim = 0, out_dim = 0;
  std::vector<float> W;   // [out][in]
  std::vector<float> b;   // the bias; kinds 4 and 5: the vector (in_dim = out_dim = its length).  Kind 8: the two dims only
  std::vector<int32_t> offsets;   // kind 9: the frame offsets (out_dim = their count times in_dim)
};

int ReadNnet(const char *path, std::vector<HostLayer> *layers);

// ------------------------------------------------------------------ pk_load's key = value model file

constexpr int kCmvnStats = 41;   // 40 sums + the frame count

// what pk_load takes from the model file (pocketkaldi.cc:72-144, am.cc:22-62)
struct ModelConfig {
  float cmvn_stats[kCmvnStats];
  std::vector<float> stats;        // ReadModelConfigStats: the cmvn_stats vector at its own length (cmvn_stats is then not set)
  std::string cmvn_path;           // the file it came from
  std::string nnet, prior, tid2pdf;
  int left = 0, right = 0, num_pdfs = 0;
};
int ReadModelConfig(const char *config_path, ModelConfig *out);
// The same file for a model of any feature dimension: a cmvn_stats vector of 1 .. stats_cap floats (PK_MI355_E_IO
// otherwise, both numbers and the file named).  Whether it fits the model is the caller's check.
int ReadModelConfigStats(const char *config_path, int stats_cap, ModelConfig *out);

// ------------------------------------------------------------------ WAV
// pcm_reader.cc:45-220: strict 44-byte-header RIFF/WAVE PCM, mono, 16 kHz, 8/16/32-bit,
// sample values kept unscaled as float.
int ReadWav16k(const char *filename, std::vector<float> *samples);
// The same header checks for any positive rate and 1 .. 8 interleaved channels (byte_rate and block_align against the
// channel count): channel `channel` of the file, de-interleaved, sample values as ReadWav16k gives them.  A channel
// outside the file is PK_MI355_E_INVALID; rate / channels (may be null) receive the header's.
int ReadWave(const char *filename, int channel, std::vector<float> *samples, int *rate, int *channels);

}  // namespace pkhost

// ------------------------------------------------------------------ graph (Fst::Read / CountArcs, fst.cc:29-110)

struct pk_mi355_fst {
  int num_states = 0, num_arcs = 0, start = 0;
  std::vector<float> final_w;
  std::vector<int32_t> first;
  std::vector<int32_t> arc_first, arc_count;    // Fst::CountArcs per state
  struct Arc { int32_t next, ilabel, olabel; float weight; };
  std::vector<Arc> arcs;
};

namespace pkhost {

int ReadFst(const char *path, pk_mi355_fst *f);

// The graph as the decoder walks it: emitting and epsilon CSR lists (arc order kept), ilabels mapped to pdfs through
// tid2pdf (identity when it is empty) and checked against num_pdfs.
struct SplitArc { int32_t next, pdf, weight_bits, arc; };   // arc: the original arc id
constexpr size_t kMaxSplitArcs = 0x7FFFFFFFu;               // the decoder's candidate ids keep the top bit for epsilon arcs
struct GraphSplit {
  std::vector<int32_t> e_off, n_off, e_src, n_src;
  std::vector<SplitArc> e_arc, n_arc;
  std::vector<int32_t> olabel;                              // by original arc id
};
int SplitGraph(const pk_mi355_fst &f, const std::vector<int32_t> &tid2pdf, int num_pdfs, GraphSplit *out);

// The words of a path: its arcs' non-zero olabels, in path order.  Returns their number; writes at most max_words.
int PathWords(const std::vector<int32_t> &olabel, const int32_t *arcs, int num_arcs, int *words, int max_words);

// The graph's labels and weights by original arc id, as the segment function reads them.
struct ArcLabels {
  std::vector<int32_t> ilabel, olabel;
  std::vector<float> weight;
};
void LabelsOf(const pk_mi355_fst &f, ArcLabels *out);

// The word segments of a path (pk_mi355_word_t, include/pk_mi355.h): a segment begins at every arc whose olabel is
// not 0 and runs up to the next such arc; the arcs before the first one form a leading segment with word 0.  ac: the
// acoustic cost of each of the path's num_ac frames, or null (acoustic_cost is then NaN).  Sums are taken in double
// in path order and rounded to float once.  Returns the number of segments; writes at most max.
int WordSegments(const ArcLabels &g, const int32_t *arcs, int num_arcs, const float *ac, int num_ac, pk_mi355_word_t *out,
                 int max);

// The frames of a path: its arcs whose ilabel is not 0, in path order.  arc_ac: one cost per arc of the path (an
// epsilon arc's is ignored).  Per frame the arc id, its ilabel and its cost (any pointer may be null; at most
// max_frames entries written).  Returns the frames, or PK_MI355_E_DEVICE when the path's emitting arcs are not
// expect_frames -- the verdict AlignKernel gives for a path whose emitting arcs are not the utterance's frames.
int PathFrames(const ArcLabels &g, const int32_t *arcs, const float *arc_ac, int num_arcs, int expect_frames,
               int32_t *arc_ids, int32_t *trans_ids, float *ac, int max_frames);

// pk_load's own keys (pocketkaldi.cc:81-88, 117-124): the path a key of the model file names, resolved against the
// file's directory; a missing key is "Unable to find key '<key>' in <file>".
int ConfigPath(const char *config_path, const char *key, std::string *out);

}  // namespace pkhost

// ------------------------------------------------------------------ symbol table (pk_symboltable_read, symbol_table.cc:23-73)

struct pk_mi355_symtab {
  std::vector<int32_t> index;      // offset of symbol i's string in buffer
  std::vector<char> buffer;        // NUL-terminated strings; ends in NUL when not empty
};

namespace pkhost {
int ReadSymtab(const char *path, pk_mi355_symtab *st);
}  // namespace pkhost

#endif  // PK_FILES_H_

// pk_ark.cc -- the reader for Kaldi archives and script files of float matrices (pk_mi355_ark_*).
// Plain C++ like pk_files.cc (whose error state it reports through): no HIP header, so it also builds into a
// stand-alone program that runs under the host sanitizers (tests/cpp/ark_test.cc).
//
// The format, from its public definition:
//   binary matrix   "\0B", the token "FM " (float) or "DM " (double), the byte 4 and a little-endian int32 rows, the byte 4
//                   and a little-endian int32 cols, then rows x cols little-endian values, row-major;
//   text matrix     " [", rows of whitespace-separated numbers (as strtod reads them: nan, inf, -inf too), one row per
//                   line, " ]" behind the last row; " [ ]" is the empty matrix;
//   archive         objects one after the other, each preceded by its key (non-space bytes) and one space;
//   scp             lines "<key> <path>" or "<key> <path>:<offset>", the offset being the byte position of the object
//                   (just past the key's space); paths are opened as given.
// A matrix is rows = frames: its bytes are a pk_matrix_t with nrow = cols and ncol = rows as they lie; doubles are
// narrowed with one (float) cast; a matrix of at most kWideRows rows -- a CMVN statistics record, whose sums need their
// doubles -- is kept as doubles too (pk_mi355_ark_matrix_f64).  An archive is read entry by entry; every size a file states is checked in 64 bits
// against the bytes that remain in the file before anything is allocated from it.
// PK_MI355_E_IO: what cannot be opened, is truncated or is malformed.  PK_MI355_E_INVALID: well-formed input this reader
// does not take -- compressed matrices, vectors, scp ranges, pipes -- named in the text (an scp line by its number).
#include <errno.h>
#include <stdlib.h>

#include <exception>
#include <new>

#include "pk_files.h"

using pkhost::Fail;

struct pk_mi355_ark {
  FILE *f = nullptr;            // the archive, or the scp list
  bool scp = false, single = false;
  std::string path;             // of f
  int line = 0;                 // scp: lines read
  int failed = 0;               // the code of the failure that ended the reading
  std::string key;
  std::vector<float> data;      // the current entry, [rows][cols]
  std::vector<double> wide;     // the same values before the narrowing, when rows <= kWideRows (otherwise empty)
  int rows = 0, cols = 0;
  bool have = false;
};

namespace {

constexpr size_t kMaxKey = 4096;        // a "key" longer than this is garbage, not a key
constexpr int kWideRows = 2;            // matrices of at most this many rows are also kept as doubles

int64_t Remaining(FILE *f) {            // bytes from the position to the end of the file; -1: not a seekable file
  const off_t at = ftello(f);
  if (at < 0 || fseeko(f, 0, SEEK_END) != 0) return -1;
  const off_t end = ftello(f);
  if (end < 0 || fseeko(f, at, SEEK_SET) != 0) return -1;
  return end >= at ? (int64_t)(end - at) : 0;
}

// The binary object behind "\0B" at the position of f.  `where` names the object in the error text.
int ReadBinaryMatrix(FILE *f, const char *where, std::vector<float> *data, std::vector<double> *wide, int *rows, int *cols) {
  char tok[8];
  size_t n = 0;
  for (;;) {                                            // the token, up to and with its space
    const int c = fgetc(f);
    if (c == EOF) return Fail(PK_MI355_E_IO, "%s: truncated in the type token", where);
    if (c == ' ') break;
    if (n >= 4 || !((c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9')))                // (digits: CM2, CM3)
      return Fail(PK_MI355_E_IO, "%s: garbage where a type token belongs", where);
    tok[n++] = (char)c;
  }
  tok[n] = 0;
  const std::string t(tok);
  if (t == "CM" || t == "CM2" || t == "CM3")
    return Fail(PK_MI355_E_INVALID, "%s: a compressed matrix (%s); this reader takes float and double matrices: write it uncompressed "
                "(copy-feats --compress=false)", where, tok);
  if (t == "FV" || t == "DV") return Fail(PK_MI355_E_INVALID, "%s: a vector (%s) where a matrix is expected", where, tok);
  if (t != "FM" && t != "DM") return Fail(PK_MI355_E_IO, "%s: unknown type token '%s'", where, tok);
  const int width = t == "FM" ? 4 : 8;
  int32_t dim[2];
  for (int i = 0; i < 2; ++i) {
    unsigned char head[5];
    if (fread(head, 1, 5, f) != 5) return Fail(PK_MI355_E_IO, "%s: truncated in the header", where);
    if (head[0] != 4) return Fail(PK_MI355_E_IO, "%s: size byte %d where 4 is expected", where, head[0]);
    dim[i] = (int32_t)((uint32_t)head[1] | (uint32_t)head[2] << 8 | (uint32_t)head[3] << 16 | (uint32_t)head[4] << 24);
  }
  if (dim[0] < 0 || dim[1] < 0) return Fail(PK_MI355_E_IO, "%s: negative dimensions %d x %d", where, dim[0], dim[1]);
  const uint64_t count = (uint64_t)dim[0] * (uint64_t)dim[1];          // (< 2^62; count x width could wrap: divide instead)
  const int64_t remain = Remaining(f);
  if (remain < 0) return Fail(PK_MI355_E_IO, "%s: the file cannot be measured", where);
  if (count > (uint64_t)remain / (uint64_t)width)
    return Fail(PK_MI355_E_IO, "%s: truncated: %d x %d values of %d bytes, %lld bytes remain", where, dim[0], dim[1], width, (long long)remain);
  data->resize((size_t)count);
  const bool keep = dim[0] <= kWideRows;
  wide->clear();
  if (keep) wide->reserve((size_t)count);
  if (width == 4) {
    if (count && fread(data->data(), 4, (size_t)count, f) != count) return Fail(PK_MI355_E_IO, "%s: short read", where);
    if (keep) wide->assign(data->begin(), data->end());
  } else {
    double buf[1024];
    for (uint64_t done = 0; done < count;) {
      const size_t take = (size_t)std::min<uint64_t>(1024, count - done);
      if (fread(buf, 8, take, f) != take) return Fail(PK_MI355_E_IO, "%s: short read", where);
      for (size_t i = 0; i < take; ++i) (*data)[(size_t)done + i] = (float)buf[i];
      if (keep) wide->insert(wide->end(), buf, buf + take);
      done += take;
    }
  }
  *rows = dim[0];
  *cols = dim[1];
  return 0;
}

// The text object at the position of f (which is past any "\0B" test): " [", rows, "]".
int ReadTextMatrix(FILE *f, const char *where, std::vector<float> *data, std::vector<double> *wide, int *rows, int *cols) {
  int c;
  do c = fgetc(f); while (c == ' ' || c == '\t' || c == '\n' || c == '\r');
  if (c == EOF) return Fail(PK_MI355_E_IO, "%s: truncated where an object begins", where);
  if (c != '[') return Fail(PK_MI355_E_IO, "%s: garbage where '\\0B' or '[' belongs", where);
  data->clear();
  wide->clear();
  int nrows = 0, ncols = -1, in_row = 0;
  auto end_row = [&]() -> int {
    if (in_row == 0) return 0;
    if (ncols >= 0 && in_row != ncols) return Fail(PK_MI355_E_IO, "%s: ragged text matrix (row %d has %d values, the rows before it %d)", where, nrows, in_row, ncols);
    ncols = in_row;
    in_row = 0;
    ++nrows;
    return 0;
  };
  std::string word;
  for (;;) {
    c = fgetc(f);
    if (c == EOF) return Fail(PK_MI355_E_IO, "%s: truncated text matrix (no ']')", where);
    if (c == ' ' || c == '\t' || c == '\r') continue;
    if (c == '\n') { if (int rc = end_row()) return rc; continue; }
    if (c == ']') {
      if (int rc = end_row()) return rc;
      c = fgetc(f);                                     // the line's end behind it, when there is one
      while (c == ' ' || c == '\r') c = fgetc(f);
      if (c != '\n' && c != EOF) ungetc(c, f);
      break;
    }
    word.assign(1, (char)c);
    for (;;) {
      c = fgetc(f);
      if (c == EOF || c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == ']') break;
      if (word.size() >= 64) return Fail(PK_MI355_E_IO, "%s: garbage where a number belongs", where);
      word.push_back((char)c);
    }
    if (c != EOF) ungetc(c, f);
    if (memchr(word.data(), 0, word.size())) return Fail(PK_MI355_E_IO, "%s: garbage where a number belongs", where);
    char *end = nullptr;
    const double v = strtod(word.c_str(), &end);
    if (end == word.c_str() || *end != 0) return Fail(PK_MI355_E_IO, "%s: '%s' where a number belongs", where, word.c_str());
    data->push_back((float)v);
    if (nrows < kWideRows) wide->push_back(v);
    else if (!wide->empty()) std::vector<double>().swap(*wide);      // a third row: not a statistics record
    ++in_row;
  }
  *rows = nrows;
  *cols = ncols < 0 ? 0 : ncols;
  return 0;
}

// One object at the position of f: binary when it begins with "\0B", text otherwise.
int ReadObject(FILE *f, const char *where, std::vector<float> *data, std::vector<double> *wide, int *rows, int *cols) {
  const int c = fgetc(f);
  if (c == EOF) return Fail(PK_MI355_E_IO, "%s: truncated where an object begins", where);
  if (c != 0) {
    ungetc(c, f);
    return ReadTextMatrix(f, where, data, wide, rows, cols);
  }
  if (fgetc(f) != 'B') return Fail(PK_MI355_E_IO, "%s: garbage where '\\0B' belongs", where);
  return ReadBinaryMatrix(f, where, data, wide, rows, cols);
}

// "path" or "path:offset" -> the object there.  Ranges, pipes and "-" are named and refused.
int ReadRx(const std::string &rx, const char *where, std::vector<float> *data, std::vector<double> *wide, int *rows, int *cols) {
  if (rx.empty()) return Fail(PK_MI355_E_IO, "%s: no file name", where);
  if (rx == "-" || rx.back() == '|' || rx.front() == '|')
    return Fail(PK_MI355_E_INVALID, "%s: '%s' is a pipe or the standard input; this reader opens files", where, rx.c_str());
  if (rx.back() == ']') return Fail(PK_MI355_E_INVALID, "%s: '%s' has a row or column range; this reader takes whole matrices", where, rx.c_str());
  std::string path = rx;
  int64_t offset = 0;
  const size_t colon = rx.rfind(':');
  if (colon != std::string::npos && colon + 1 < rx.size() && rx.find_first_not_of("0123456789", colon + 1) == std::string::npos) {
    if (rx.size() - colon - 1 > 18) return Fail(PK_MI355_E_IO, "%s: offset out of range in '%s'", where, rx.c_str());
    offset = strtoll(rx.c_str() + colon + 1, nullptr, 10);
    path = rx.substr(0, colon);
  }
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return Fail(PK_MI355_E_IO, "%s: cannot open %s", where, path.c_str());
  int rc = 0;
  const int64_t size = Remaining(f);
  if (size < 0) rc = Fail(PK_MI355_E_IO, "%s: %s cannot be measured", where, path.c_str());
  else if (offset > size) rc = Fail(PK_MI355_E_IO, "%s: offset %lld is past the end of %s (%lld bytes)", where, (long long)offset, path.c_str(), (long long)size);
  else if (fseeko(f, (off_t)offset, SEEK_SET) != 0) rc = Fail(PK_MI355_E_IO, "%s: cannot seek in %s", where, path.c_str());
  else rc = ReadObject(f, where, data, wide, rows, cols);
  fclose(f);
  return rc;
}

// The next key of an archive: 1, 0 at the end of the file, negative for an error.
int ReadKey(FILE *f, const char *path, std::string *key) {
  int c;
  do c = fgetc(f); while (c == '\n' || c == '\r' || c == ' ' || c == '\t');
  if (c == EOF) return 0;
  key->clear();
  for (;;) {
    if (c == 0 || key->size() >= kMaxKey) return Fail(PK_MI355_E_IO, "%s: garbage where a key belongs", path);
    key->push_back((char)c);
    c = fgetc(f);
    if (c == ' ') return 1;
    if (c == EOF || c == '\n' || c == '\t' || c == '\r') return Fail(PK_MI355_E_IO, "%s: key '%s' without an object", path, key->c_str());
  }
}

int NextScp(pk_mi355_ark *h) {
  std::string text;
  for (;;) {
    text.clear();
    int c;
    while ((c = fgetc(h->f)) != EOF && c != '\n') {
      if (text.size() >= 65536) return Fail(PK_MI355_E_IO, "%s line %d: line too long", h->path.c_str(), h->line + 1);
      text.push_back((char)c);
    }
    if (c == EOF && text.empty()) return 0;
    ++h->line;
    while (!text.empty() && (text.back() == '\r' || text.back() == ' ' || text.back() == '\t')) text.pop_back();
    if (!text.empty()) break;                            // (an empty line is skipped)
  }
  const size_t sp = text.find_first_of(" \t");
  if (sp == std::string::npos || sp == 0 || memchr(text.data(), 0, text.size()))
    return Fail(PK_MI355_E_IO, "%s line %d: '<key> <file>' expected", h->path.c_str(), h->line);
  const size_t at = text.find_first_not_of(" \t", sp);
  h->key = text.substr(0, sp);
  char where[256];
  snprintf(where, sizeof(where), "%.150s line %d", h->path.c_str(), h->line);
  return ReadRx(text.substr(at), where, &h->data, &h->wide, &h->rows, &h->cols) ? pk_mi355_last_error_code() : 1;
}

}  // namespace

extern "C" {

pk_mi355_ark_t *pk_mi355_ark_open(const char *spec) {
  if (!spec) { Fail(PK_MI355_E_INVALID, "null argument"); return nullptr; }
  std::string s(spec);
  bool scp = s.size() > 4 && s.compare(s.size() - 4, 4, ".scp") == 0;
  if (s.compare(0, 3, "ark") == 0 || s.compare(0, 3, "scp") == 0) {            // "ark:", "scp:", with options ("ark,t:")
    const size_t colon = s.find(':');
    if (colon != std::string::npos && (colon == 3 || s[3] == ',')) {
      scp = s[0] == 's';
      s = s.substr(colon + 1);
    }
  }
  if (s.empty()) { Fail(PK_MI355_E_IO, "no file name in '%s'", spec); return nullptr; }
  if (s == "-" || s.back() == '|' || s.front() == '|') {
    Fail(PK_MI355_E_INVALID, "'%s' is a pipe or the standard input; this reader opens files", spec);
    return nullptr;
  }
  FILE *f = fopen(s.c_str(), "rb");
  if (!f) { Fail(PK_MI355_E_IO, "cannot open %s", s.c_str()); return nullptr; }
  pk_mi355_ark *h = new pk_mi355_ark();
  h->f = f; h->scp = scp; h->path = s;
  return h;
}

pk_mi355_ark_t *pk_mi355_ark_read_object(const char *rxfilename) {
  if (!rxfilename) { Fail(PK_MI355_E_INVALID, "null argument"); return nullptr; }
  pk_mi355_ark *h = new pk_mi355_ark();
  h->single = true; h->path = rxfilename;
  int rc;
  try {
    rc = ReadRx(h->path, rxfilename, &h->data, &h->wide, &h->rows, &h->cols);
  } catch (const std::exception &) {                     // (no exception crosses the C boundary)
    rc = Fail(PK_MI355_E_IO, "%s: out of host memory", rxfilename);
  }
  if (rc) { delete h; return nullptr; }
  h->have = true;
  return h;
}

int pk_mi355_ark_next(pk_mi355_ark_t *h) {
  if (!h) return Fail(PK_MI355_E_INVALID, "null argument");
  h->have = false;
  if (h->single) return 0;                               // the one object was read by pk_mi355_ark_read_object
  if (h->failed) return Fail(h->failed, "%s: the reader stopped at an earlier error", h->path.c_str());
  int rc;
  try {
    if (h->scp) {
      rc = NextScp(h);
    } else {
      rc = ReadKey(h->f, h->path.c_str(), &h->key);
      if (rc == 1) {
        char where[256];
        snprintf(where, sizeof(where), "%.120s key '%.100s'", h->path.c_str(), h->key.c_str());
        if (ReadObject(h->f, where, &h->data, &h->wide, &h->rows, &h->cols)) rc = pk_mi355_last_error_code();
      }
    }
  } catch (const std::exception &) {                     // an entry the host cannot hold; no exception crosses the C boundary
    rc = Fail(PK_MI355_E_IO, "%s: out of host memory", h->path.c_str());
  }
  if (rc < 0) h->failed = rc;
  h->have = rc == 1;
  return rc;
}

const char *pk_mi355_ark_key(const pk_mi355_ark_t *h) { return h && h->have ? h->key.c_str() : ""; }

int pk_mi355_ark_matrix(const pk_mi355_ark_t *h, pk_matrix_t *view) {
  if (!h || !view) return Fail(PK_MI355_E_INVALID, "null argument");
  if (!h->have) return Fail(PK_MI355_E_STATE, "no current entry");
  view->ncol = h->rows;                                  // frames
  view->nrow = h->cols;                                  // the feature dimension
  view->data = h->data.empty() ? nullptr : const_cast<float *>(h->data.data());
  return 0;
}

int pk_mi355_ark_matrix_f64(const pk_mi355_ark_t *h, double *out, int capacity) {
  if (!h || !out) return Fail(PK_MI355_E_INVALID, "null argument");
  if (!h->have) return Fail(PK_MI355_E_STATE, "no current entry");
  if (h->rows > kWideRows) return Fail(PK_MI355_E_INVALID, "the entry has %d rows: doubles are kept for matrices of at most %d rows", h->rows, kWideRows);
  const size_t count = (size_t)h->rows * (size_t)h->cols;
  if (h->wide.size() != count) return Fail(PK_MI355_E_STATE, "internal: the entry's doubles were not kept");
  if (capacity < 0 || (size_t)capacity < count) return Fail(PK_MI355_E_INVALID, "the entry has %d x %d values, the buffer holds %d", h->rows, h->cols, capacity);
  for (size_t i = 0; i < count; ++i) out[i] = h->wide[i];
  return (int)count;
}

void pk_mi355_ark_close(pk_mi355_ark_t *h) {
  if (!h) return;
  if (h->f) fclose(h->f);
  delete h;
}

}  // extern "C"

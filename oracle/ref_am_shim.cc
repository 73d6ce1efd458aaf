// ref_am_shim.cc -- extern "C" entry points over the reference's whole acoustic path, compiled
// from its own sources where they lie (oracle/Makefile: ref_am):
//   pcm_reader.cc  fbank.cc  cmvn.cc  nnet.cc  am.cc  decodable.cc  configuration.cc
//   vector.cc  matrix.cc  util.cc  srfft.cc  gemm.cc  gemm_haswell.cc  pool.cc  strlcpy.cc  hashtable.cc
// TEST INFRASTRUCTURE ONLY.  Nothing of the reference is copied into this repository; its headers
// are included by path.  Outputs: oracle/_ref/libpkref_am.so (assertions on, as the reference's
// Makefile.am builds) and oracle/_ref/libpkref_am_ndebug.so (-DNDEBUG, for the one non-finite case:
// with assertions on, a NaN reaching ApplyLog aborts at vector.cc:336).
//
// vector.cc:5 and matrix.cc:10 include <cblas.h> but the reference uses no cblas_ symbol anywhere;
// the recipe puts an EMPTY file of that name on the include path (a scratch directory, removed
// again) and links no BLAS.  The empty header declares nothing and nothing is called through it.
//
// Only pkref_* is exported (oracle/ref_am.map, -Bsymbolic): the reference's pk_decodable_*,
// pk_matrix_*, pk_vector_* are names the product library exports too and must never bind across.
//
// pk_matrix_t is column-major with one frame per column: the same bytes as a row-major [T][D].
#include "am.h"
#include "cmvn.h"
#include "configuration.h"
#include "decodable.h"
#include "fbank.h"
#include "nnet.h"
#include "pcm_reader.h"

#include <stdlib.h>
#include <string.h>

namespace {

// A borrowed [T][D] buffer seen as the reference's D x T column-major matrix.
pk_matrix_t Borrow(const float *data, int T, int D) {
  pk_matrix_t m;
  m.nrow = D;
  m.ncol = T;
  m.data = const_cast<float *>(data);
  return m;
}

struct RefAm {
  pocketkaldi::Configuration conf;
  pocketkaldi::AcousticModel am;
};

void CopyMessage(char *msg, const char *text) {
  if (!msg) return;
  strncpy(msg, text, 255);
  msg[255] = 0;
}

}  // namespace

extern "C" {

// pk_16kpcm_read (pk_read_audio, pocketkaldi.cc:167-174).  *out is malloc'ed (pkref_free); returns
// the number of samples, or -1 with the reference's message in msg[256].
int pkref_wav_read(const char *path, float **out, char *msg) {
  pk_status_t status;
  pk_status_init(&status);
  pk_vector_t wave;
  pk_vector_init(&wave, 0, NAN);
  pk_16kpcm_read(path, &wave, &status);
  if (!status.ok) {
    CopyMessage(msg, status.message);
    pk_vector_destroy(&wave);
    return -1;
  }
  int n = wave.dim;
  *out = static_cast<float *>(malloc(sizeof(float) * (n > 0 ? n : 1)));
  if (n > 0) memcpy(*out, wave.data, sizeof(float) * n);
  pk_vector_destroy(&wave);
  return n;
}

void pkref_free(void *p) { free(p); }

// Fbank::Compute (pocketkaldi.cc:190-192).  n >= 1 (pk_process returns before it for an empty
// wave).  Returns the reference's frame count T and writes T x 40 floats if T <= max_frames -- NOTHING otherwise: the
// caller compares T with its bound (oracle.py: ref_fbank does).
int pkref_fbank(const float *wave, int n, float *out, int max_frames) {
  pocketkaldi::Fbank fbank;
  pk_vector_t w;
  w.dim = n;
  w.data = const_cast<float *>(wave);
  pk_matrix_t feats;
  pk_matrix_init(&feats, 0, 0);
  fbank.Compute(&w, &feats);
  int T = feats.ncol;
  if (T > 0 && feats.nrow == PK_FBANK_DIM && T <= max_frames)
    memcpy(out, feats.data, sizeof(float) * T * PK_FBANK_DIM);
  pk_matrix_destroy(&feats);
  return T;
}

// CMVN + GetFrame per frame, as pk_process does (pocketkaldi.cc:196-204).  stats41 with a positive
// count; T >= 1.
void pkref_cmvn(const float *stats41, const float *raw, int T, float *out) {
  pk_vector_t g;
  g.dim = PK_FBANK_DIM + 1;
  g.data = const_cast<float *>(stats41);
  pk_matrix_t raw_feats = Borrow(raw, T, PK_FBANK_DIM);
  pk_matrix_t feats = Borrow(out, T, PK_FBANK_DIM);
  pocketkaldi::CMVN cmvn(&g, &raw_feats);
  for (int frame = 0; frame < raw_feats.ncol; ++frame) {
    pk_vector_t frame_col = pk_matrix_getcol(&feats, frame);
    cmvn.GetFrame(frame, &frame_col);
  }
}

// Nnet::Read on an NNT0 file.  NULL on failure (message in msg[256]).
void *pkref_nnet_load(const char *path, char *msg) {
  pocketkaldi::util::ReadableFile fd;
  pocketkaldi::Status st = fd.Open(path);
  pocketkaldi::Nnet *nn = new pocketkaldi::Nnet();
  if (st.ok()) st = nn->Read(&fd);
  if (!st.ok()) {
    CopyMessage(msg, st.what().c_str());
    delete nn;
    return NULL;
  }
  return nn;
}

// Nnet::Propagate on x[T][D], T >= 1.  *out is malloc'ed [T][dim] (pkref_free); returns dim.
int pkref_nnet_propagate(void *nnet, const float *x, int T, int D, float **out) {
  pk_matrix_t in = Borrow(x, T, D);
  pk_matrix_t res;
  pk_matrix_init(&res, 0, 0);
  static_cast<pocketkaldi::Nnet *>(nnet)->Propagate(&in, &res);
  int dim = res.nrow;
  *out = res.data;            // handed over, not destroyed: pk_matrix_resize gets it from pk_realloc, which is realloc
                              // (util.cc:62-64), so pkref_free's free() is its match
  return res.ncol == T ? dim : -1;
}

void pkref_nnet_free(void *nnet) { delete static_cast<pocketkaldi::Nnet *>(nnet); }

// Configuration::Read + AcousticModel::Read (pk_load's share, pocketkaldi.cc:76-79, 111-114).
void *pkref_am_load(const char *conf_path, char *msg) {
  RefAm *r = new RefAm();
  pocketkaldi::Status st = r->conf.Read(conf_path);
  if (st.ok()) st = r->am.Read(r->conf);
  if (!st.ok()) {
    CopyMessage(msg, st.what().c_str());
    delete r;
    return NULL;
  }
  return r;
}

void pkref_am_free(void *am) { delete static_cast<RefAm *>(am); }

int pkref_am_num_pdfs(void *am) { return static_cast<RefAm *>(am)->am.num_pdfs(); }

// AcousticModel::TransitionIdToPdfId; tid within the table (the reference asserts it).
int pkref_am_tid2pdf(void *am, int tid) { return static_cast<RefAm *>(am)->am.TransitionIdToPdfId(tid); }

// pk_decodable_init -> copy log_prob out -> pk_decodable_destroy (pocketkaldi.cc:210-216, 247).
// feats[T][D], T >= 1; out[T][max_dim].  Returns the reference's log_prob row length and writes the matrix only if that
// is <= max_dim (and the frame count is T): the caller compares it with num_pdfs (oracle.py: RefAm.decodable does).
int pkref_decodable(void *am, float prob_scale, const float *feats, int T, int D, float *out, int max_dim) {
  pk_matrix_t f = Borrow(feats, T, D);
  pk_decodable_t dec;
  pk_decodable_init(&dec, &static_cast<RefAm *>(am)->am, prob_scale, &f);
  int dim = dec.log_prob.nrow;
  if (dim <= max_dim && dec.log_prob.ncol == T) memcpy(out, dec.log_prob.data, sizeof(float) * T * dim);
  pk_decodable_destroy(&dec);
  return dim;
}

}  // extern "C"

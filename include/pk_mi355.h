/*
 * pk_mi355.h -- C ABI of libpk_mi355.so: pocketkaldi's acoustic-scoring hot path
 * (fbank -> CMVN -> splice -> nnet -> log-likelihoods) on AMD MI355X (gfx950).
 *
 * This is the drop-in boundary.  Plain C types only; every entry point cites the
 * reference interface (path:line under the pocketkaldi tree) it replaces.
 * INTEGRATION.md shows the reference-side change that binds to it.
 *
 * Error model: the reference's boundary has no status channel (decodable.h:20-41
 * are void/float/bool; misuse is assert()).  Here every pk_mi355_* function that
 * can fail returns 0 on success and a negative code on failure, and
 * pk_mi355_last_error() returns a thread-local message.  The four pk_decodable_*
 * functions keep the reference signatures; a device failure inside
 * pk_decodable_init() leaves log_prob empty (ncol = 0) and sets the error string.
 * No C++ exception crosses this ABI.  There is no CPU fallback: without a
 * usable gfx950 device every compute entry point fails.
 */
#ifndef PK_MI355_H_
#define PK_MI355_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- data-layout contract (field order and meaning as in the reference) ----
 * Inside the reference tree (include/reference_binding/decodable.h is the file that takes the
 * place of src/decodable.h there) the reference's own matrix.h / vector.h / nnet.h come first
 * and their declarations are the ones used: the guards below are the reference's include guards
 * (matrix.h:5, vector.h:26) and layer-kind macros (nnet.h:14-17).                              */

/* matrix.h:20-24 -- column-major; memory is [ncol][nrow], i.e. for features and
 * log-likelihoods one frame (column) is contiguous.                              */
#ifndef POCKETKALDI_MATRIX_H_   /* inside the reference tree matrix.h has already declared it */
typedef struct pk_matrix_t {
  int ncol;
  int nrow;
  float *data;
} pk_matrix_t;
#endif

/* vector.h:39-42 */
#ifndef POCKETKALDI_VECTOR_H_   /* likewise vector.h */
typedef struct pk_vector_t {
  int dim;
  float *data;
} pk_vector_t;
#endif

/* Stands where `AcousticModel *` stands in the reference (am.h:23-52): holds the
 * nnet weights (in HBM), log-priors, context and the tid->pdf map (host).        */
#ifdef PK_MI355_AM_T            /* reference_binding/decodable.h: the handle keeps the NAME the
                                   reference's translation units use for this pointer
                                   (pocketkaldi::AcousticModel, decodable.h:17, pocketkaldi.h:38);
                                   across the C ABI it is the same opaque pointer                 */
typedef PK_MI355_AM_T pk_mi355_am_t;
#else
typedef struct pk_mi355_am pk_mi355_am_t;
#endif

/* decodable.h:15-18 -- same size and field offsets on LP64 (16 + 8 bytes).       */
typedef struct pk_decodable_t {
  pk_matrix_t log_prob;
  pk_mi355_am_t *am;
} pk_decodable_t;

/* Layer kinds, nnet.h:13-16 / nnet.h:28-33 */
#ifndef PK_NNET_LINEAR_LAYER    /* nnet.h #defines the same names to the same values */
enum {
  PK_NNET_LINEAR_LAYER = 0,
  PK_NNET_RELU_LAYER = 1,
  PK_NNET_NORMALIZE_LAYER = 2,
  PK_NNET_SOFTMAX_LAYER = 3
};
#endif
/* Kinds 4 and 5 carry the reference's numbers (nnet.h:18-19; its reader loads neither); 6 to 8 are this library's.
 * The rules: pk_mi355_layer_apply_host below.                                     */
#ifndef PK_NNET_ADD_LAYER
enum {
  PK_NNET_ADD_LAYER = 4,              /* y[d] = x[d] + v[d]                          */
  PK_NNET_MUL_LAYER = 5               /* y[d] = x[d] * v[d]                          */
};
#endif
enum {
  PK_MI355_NNET_SIGMOID_LAYER = 6,
  PK_MI355_NNET_TANH_LAYER = 7,
  PK_MI355_NNET_PNORM_LAYER = 8,      /* the 2-norm of groups of in_dim / out_dim consecutive features */
  PK_MI355_NNET_TIME_SPLICE_LAYER = 9 /* y[t][c in_dim + d] = x[t + o_c][d]: a splice between hidden layers (TDNN) */
};

/* Error codes */
enum {
  PK_MI355_OK = 0,
  PK_MI355_E_INVALID = -1,   /* bad argument / shape mismatch            */
  PK_MI355_E_DEVICE = -2,    /* HIP runtime failure or no gfx950 device  */
  PK_MI355_E_IO = -3,        /* file missing or corrupted                */
  PK_MI355_E_STATE = -4,     /* call order (e.g. model not finalized)    */
  PK_MI355_E_RANGE = -5,     /* f16x3 / f16: an operand left the fp16 split's range (results withheld) */
  PK_MI355_E_CAPACITY = -6   /* decoder: backtrace storage exhausted     */
};

const char *pk_mi355_last_error(void);
/* The code of the failure pk_mi355_last_error() describes (for entries that return a pointer, NULL on failure). */
int pk_mi355_last_error_code(void);

/* Select the HIP device used by objects this THREAD creates afterwards (default 0; like
 * hipSetDevice the setting is per host thread).  One process drives one GPU (one rank per GPU
 * in multi-GPU runs).
 *
 * Threads: a model may be shared by host threads.  pk_decodable_init, pk_mi355_nnet_propagate and
 * pk_mi355_process_acoustic use one device workspace per model and serialise on a per-model lock
 * (the reference's versions allocate per call, nnet.cc:149-163); the four pk_decodable_* readers
 * are lock-free.  A pk_mi355_batch_t belongs to one thread at a time; different batches of one
 * model may be driven from different threads.                                                 */
int pk_mi355_set_device(int device);

/* ------------------------------------------------------------------------- */
/* The four functions decoder.cc consumes -- decodable.h:20-41, decodable.cc:8-36 */
/* ------------------------------------------------------------------------- */

/* decodable.cc:8-17.  feats: CMVN'd features, {ncol = T, nrow = feat_dim}, host,
 * borrowed.  Allocates self->log_prob {ncol = T, nrow = num_pdfs} on the host with
 * malloc(), fills it with (log softmax - log prior) * prob_scale.
 *
 * Isolation and reuse: every call (this one and pk_mi355_nnet_propagate) is a function of its own inputs,
 * whatever the model's workspace held from earlier calls -- longer, NaN or out-of-range ones included; in F32
 * a row is a function of the frames it splices (a NaN frame makes the rows within its context NaN and no
 * others).  F16X3 / F16 exception: the range verdict covers the whole call (tests/test_gpu_isolation.py).   */
void pk_decodable_init(pk_decodable_t *self, pk_mi355_am_t *am, float prob_scale,
                       const pk_matrix_t *feats);
/* decodable.cc:19-22 */
void pk_decodable_destroy(pk_decodable_t *self);
/* decodable.cc:24-31: log_prob[frame][tid2pdf[trans_id]] -- host lookup          */
float pk_decodable_loglikelihood(pk_decodable_t *self, int frame, int trans_id);
/* decodable.cc:33-36 (frame = -1 on the decoder's first poll -> false)           */
bool pk_decodable_islastframe(pk_decodable_t *self, int frame);

/* ------------------------------------------------------------------------- */
/* Acoustic model -- replaces AcousticModel (am.h:23-52) + Nnet (nnet.h:88-104)   */
/* ------------------------------------------------------------------------- */

pk_mi355_am_t *pk_mi355_am_create(void);
void pk_mi355_am_destroy(pk_mi355_am_t *am);

/* LinearLayer(W, b), nnet.cc:11-20.  W is [out_dim][in_dim] row-major, the order
 * of the model file (convert_am.py:77-83); b is [out_dim].                        */
int pk_mi355_am_add_linear(pk_mi355_am_t *am, int in_dim, int out_dim, const float *W,
                           const float *b);
/* ReLULayer / NormalizeLayer / SoftmaxLayer, nnet.cc:38-75                       */
int pk_mi355_am_add_layer(pk_mi355_am_t *am, int layer_type);
/* The kinds without a parameter also include PK_MI355_NNET_SIGMOID_LAYER and PK_MI355_NNET_TANH_LAYER.  A bare kind
 * 4, 5 or 8 is refused there ("unexpected layer type"): those take their parameter through the two entries below.
 * The kinds 4 to 8 exist in F32 precision only (F16X3 / F16 refuse the network at finalize).
 *
 * PK_NNET_ADD_LAYER / PK_NNET_MUL_LAYER: v[dim] is copied; dim > 0 and every entry finite (PK_MI355_E_INVALID names
 * the first index that is not).  finalize holds dim to the width the layers in front leave.                        */
int pk_mi355_am_add_vector_layer(pk_mi355_am_t *am, int kind, int dim, const float *v);
/* PK_MI355_NNET_PNORM_LAYER, in_dim -> out_dim: out_dim > 0 and in_dim a multiple of it (PK_MI355_E_INVALID names
 * both numbers); the group size is in_dim / out_dim, p is 2.                                                       */
int pk_mi355_am_add_pnorm(pk_mi355_am_t *am, int in_dim, int out_dim);
/* The rule of one layer of kind 4 to 8 on the host, for rows x[rows][in_dim] -> out[rows][out_dim] (never in place
 * for kind 8); needs no GPU.  The GPU layers are held to it bit for bit.  With E = float expf, every operation IEEE,
 * none fused:
 *   add, mul : param = v[in_dim]; out_dim = in_dim; in float
 *   sigmoid  : x > 0: 1.0 / (1.0 + (double)E(-x)); otherwise e = (double)E(x), e / (e + 1.0); rounded to float once
 *   tanh     : x > 0: t = E(-x), q = t * t (float), -1.0 + 2.0 / (1.0 + (double)q); otherwise t = E(x), q = t * t,
 *              1.0 - 2.0 / (1.0 + (double)q); rounded to float once (a NaN takes the second branch and stays NaN)
 *   p-norm   : param = NULL; s = 0.0f, s = s + x[o G + g] * x[o G + g] for g = 0 .. G - 1 (float), out[o] = sqrtf(s)
 *              correctly rounded; an overflowed sum gives inf (Kaldi's rescaling fallback is not restated)
 * param = NULL and out_dim = in_dim for sigmoid and tanh.                                                          */
int pk_mi355_layer_apply_host(int kind, const float *x, int rows, int in_dim, const float *param, int out_dim, float *out);
/* PK_MI355_NNET_TIME_SPLICE_LAYER (F32 precision only): n strictly ascending frame offsets o_0 < ... < o_{n-1},
 * 1 <= n <= 16, |o_c| <= 32, in_dim > 0 (PK_MI355_E_INVALID names the offending numbers).  in_dim -> n in_dim:
 *   y[t][c in_dim + d] = x[t + o_c][d]      (a copy: every bit is kept)
 * With lo = max(0, -o_0) and hi = max(0, o_{n-1}) per layer and Lh, Rh their sums over the network (Lh + Rh <= 128 at
 * finalize), an utterance of T frames is scored as if its normalised features were extended by left_context + Lh copies
 * of the first frame in front and right_context + Rh copies of the last behind; the hidden activations at the virtual
 * frames outside [0, T) are computed from that extended input, every time-splice consumes lo frames on the left and hi
 * on the right, and exactly the frames [0, T) reach the output.  The layer needs a Linear in front of it and one
 * somewhere behind it.  Models with such layers run on the whole-utterance scorers (pk_decodable_init, the batch
 * scorers, the recognizer); pk_mi355_nnet_propagate and the online scorers refuse them.                              */
int pk_mi355_am_add_time_splice(pk_mi355_am_t *am, int in_dim, const int32_t *offsets, int n);
/* Lh and Rh as finalize's walk of the network recorded them ((0, 0) before it, and for a model without time-splice layers). */
int pk_mi355_am_time_context(const pk_mi355_am_t *am, int *left, int *right);
/* The layer's rule on the host in its shrinking form, x[rows][in_dim] -> out[rows - lo - hi][n in_dim]: output row r is
 * input frame r + lo.  PK_MI355_E_INVALID when rows <= lo + hi or the offsets break the limits above.  Needs no GPU. */
int pk_mi355_time_splice_host(const float *x, int rows, int in_dim, const int32_t *offsets, int n, float *out);

/* Arithmetic of the affine layers (set before finalize / read; default F32).
 *   F32   : fp32 MFMA, accumulation order of the reference's SGEMM -- bit-identical layers.
 *   F16X3 : every fp32 operand carried as an fp16 (hi, lo) pair, three fp16 MFMAs per
 *           product, fp32 accumulation: ~1e-6 relative on log-likelihoods (inside the
 *           1e-4 contract, not bit-exact), several times faster.  Supports
 *           (Linear [ReLU] [Normalize])+ [Softmax] networks.
 *           RANGE (round 4).  fp16 holds 2^-24 .. 65504 and the lo half sits 2^-12 below its value, so the
 *           accuracy above holds only while operands sit well inside that window.  Weights: every affine
 *           layer's W is multiplied by an exact power of two at finalize (max |W| -> [2^13, 2^14)) and the
 *           GEMM's epilogue divides it out again -- automatic, any training scale.  Activations: the operand
 *           of every affine layer carries an exponent too (x * 2^e is what is split; default 0, set by
 *           pk_mi355_am_calibrate / pk_mi355_am_set_input_exponents), and every call CHECKS what it wrote:
 *           an operand that reached the clamp at 65504, or whose largest magnitude stayed below 2^-5
 *           (every lo half subnormal), fails the call with PK_MI355_E_RANGE -- pk_decodable_init leaves
 *           log_prob empty, the batch calls return the code (score with sync, synchronize, fetch, fetch_all)
 *           -- and pk_mi355_last_error() names the layer.  Nothing out of range is returned quietly.
 *           NaN is not carried: where the reference's NormalizeLayer turns an all-zero row into NaN (0 * inf,
 *           nnet.cc:62-75) this mode keeps the row zero.  F32 reproduces the NaN.
 *   F16   : plain fp16 operands (the hi halves only), ONE fp16 MFMA per product, fp32 accumulation --
 *           the throughput ceiling of the fp16 matrix cores at a STATED, looser tolerance: ~1e-3
 *           relative on log-likelihoods, OUTSIDE the 1e-4 contract of the path (SURVEY section 7,
 *           step 8: "its own, separately reported, tolerance").  Same network restrictions as F16X3. */
enum { PK_MI355_PRECISION_F32 = 0, PK_MI355_PRECISION_F16X3 = 1, PK_MI355_PRECISION_F16 = 2 };
int pk_mi355_am_set_precision(pk_mi355_am_t *am, int precision);
int pk_mi355_am_precision(const pk_mi355_am_t *am);

/* F16X3 / F16: the operand exponents (no-ops returning 0 exponents / success in F32).
 * get: w_exp[l] = the power of two the weights of affine layer l were multiplied by at finalize, x_exp[l] = the
 *      exponent of that layer's input operand; returns the number of affine layers (<= capacity) or a negative code.
 * set_input_exponents: count == number of affine layers, each in [-30, 30].
 * calibrate: feats as for pk_decodable_init (CMVN'd features, {ncol = T, nrow = feat_dim}).  Runs the network on
 *      them, reads every operand's largest magnitude back from the device and sets its exponent so that it lands in
 *      [2^3, 2^4) (4 096 x headroom to the clamp; higher placements buy no accuracy), layer by layer, front to back.  The exponents live in the
 *      weight blob: pk_mi355_am_broadcast carries the root's calibration to every rank.  Calibrate while nothing
 *      is being scored with the model.  pk_mi355_batch_calibrate (below) does the same from the batch's waves. */
int pk_mi355_am_get_exponents(pk_mi355_am_t *am, int32_t *w_exp, int32_t *x_exp, int capacity);
int pk_mi355_am_set_input_exponents(pk_mi355_am_t *am, const int32_t *x_exp, int count);
int pk_mi355_am_calibrate(pk_mi355_am_t *am, const pk_matrix_t *feats);

/* Arithmetic of the softmax / log-likelihood tail (any time; default STABLE).
 *   STABLE    : log-softmax with the row maximum subtracted -- finite for finite logits of magnitude
 *               below FLT_MAX / log2(e) = 2.36e38 (DESIGN 3.5 says what lies past it), ~1e-6
 *               (measured 1.2e-6) from the reference wherever the reference does not overflow.
 *               A row with a NaN or +inf logit, or of nothing but -inf, is NaN throughout.
 *   REFERENCE : the reference's operations one by one (nnet.cc:38-47 -> vector.cc:265-277,
 *               am.cc:106-112): libm expf, float sum in column order, division, floor,
 *               libm logf, prior, scale.  With F32 precision the log-likelihoods are then the
 *               reference's bit patterns, its overflow for logits above 88.7 included.       */
enum { PK_MI355_SOFTMAX_STABLE = 0, PK_MI355_SOFTMAX_REFERENCE = 1 };
int pk_mi355_am_set_softmax(pk_mi355_am_t *am, int mode);
int pk_mi355_am_softmax(const pk_mi355_am_t *am);

/* AcousticModel::Read tail, am.cc:41-60: prior holds probabilities (the log is
 * taken here); tid2pdf is indexed by transition-id.  tid2pdf may be NULL (then
 * pk_decodable_loglikelihood treats trans_id as the pdf index).  Uploads the
 * packed weight blob to HBM.                                                     */
int pk_mi355_am_finalize(pk_mi355_am_t *am, const float *prior, int num_pdfs,
                         int left_context, int right_context, const int32_t *tid2pdf,
                         int num_tids);

/* Nnet::Read (nnet.cc:132-147) + prior / tid2pdf files (am.cc:28-60): the
 * NNT0/LAY0/MAT0/VEC0 little-endian section files.  tid2pdf_path may be NULL.    */
int pk_mi355_am_read(pk_mi355_am_t *am, const char *nnet_path, const char *prior_path,
                     const char *tid2pdf_path, int left_context, int right_context,
                     int num_pdfs);

/* pk_load's share of this path (pocketkaldi.cc:72-144): read the reference's "key = value" model
 * file (configuration.cc:16-72: '#' comments, keys case-insensitive, relative paths resolved
 * against the file's directory) and load what acoustic scoring needs -- cmvn_stats (VEC0 of 40
 * sums + count, into cmvn_stats41) and the AcousticModel keys nnet, prior, left_context,
 * right_context, num_pdfs, tid2pdf (am.cc:22-62).  The decoder's keys (fst, symbol_table) are
 * not touched.  precision: PK_MI355_PRECISION_*.  On success *am_out is a finalized model.     */
int pk_mi355_load(const char *config_path, int precision, pk_mi355_am_t **am_out, float *cmvn_stats41);
/* The same for a model of any feature dimension: the cmvn_stats vector may have any length up
 * to stats_cap and is copied to stats, its length to *stats_len.  PK_MI355_E_IO, both numbers and the file named, when
 * it is longer than stats_cap or not pk_mi355_am_feat_dim + 1 long (the sums, then the count).  Every other check
 * and message is pk_mi355_load's, which keeps its own "41 expected".                                             */
int pk_mi355_load_stats(const char *config_path, int precision, pk_mi355_am_t **am_out, float *stats, int stats_cap,
                        int *stats_len);

int pk_mi355_am_num_pdfs(const pk_mi355_am_t *am);      /* am.h:38 */
int pk_mi355_am_input_dim(const pk_mi355_am_t *am);     /* spliced width */
int pk_mi355_am_feat_dim(const pk_mi355_am_t *am);      /* per-frame feature dimension: input_dim / (left + 1 + right); 0: null or not finalized */
int pk_mi355_am_transition_to_pdf(const pk_mi355_am_t *am, int trans_id); /* am.h:30-32 */

/* The packed device weight blob (weights, biases, log-priors), for the one RCCL
 * broadcast of multi-GPU runs: every rank builds the same model structure, rank 0
 * holds the real values, all ranks broadcast [ptr, ptr+bytes) from rank 0.       */
void *pk_mi355_am_blob_device_ptr(pk_mi355_am_t *am);
size_t pk_mi355_am_blob_bytes(const pk_mi355_am_t *am);
/* That broadcast, for a C/C++ host (the multi-GPU form of pk_load, pocketkaldi.cc:72-144): ONE
 * ncclBroadcast of the blob from rank `root` into every rank's blob, in place, over the caller's
 * RCCL communicator.  rccl_comm: the caller's ncclComm_t (one process per GPU, the communicator's
 * device is the model's device).  stream: a hipStream_t to enqueue on (the caller synchronises it
 * before scoring), or NULL: the call then uses a stream of its own and returns when the
 * broadcast has completed.  tid2pdf and the layer structure are host-side and are NOT sent: every
 * rank reads the (small) tid2pdf file itself or builds the same structure, as bench.py does.
 * RCCL is bound at run time to the copy ALREADY LOADED in the process -- the one the communicator
 * was created with (global scope, or RTLD_LOCAL as under Python: found by soname) -- or to
 * $PK_MI355_RCCL_LIB when set; a second copy is never loaded implicitly.  libpk_mi355.so has no
 * link-time dependency on RCCL.  Behaviour at more than one rank has been exercised only through
 * the Python path's gloo rehearsal so far.                                 */
int pk_mi355_am_broadcast(pk_mi355_am_t *am, void *rccl_comm, int root, void *stream);
/* Out-of-place form: every rank still RECEIVES into `am`'s blob; on the root the bytes sent are
 * `src`'s blob (a second model with the same layer structure on the same device, e.g. one just
 * read from new files while `am` keeps serving).  src == NULL is pk_mi355_am_broadcast.  At one
 * rank this is RCCL copying src's blob into am's -- the form the one-GPU tests use to show that the
 * collective really writes the destination model's weights.                                     */
int pk_mi355_am_broadcast_from(pk_mi355_am_t *am, pk_mi355_am_t *src, void *rccl_comm, int root,
                               void *stream);

/* Nnet::Propagate, nnet.cc:149-163: in {ncol = T, nrow = in_dim} host ->
 * out {ncol = T, nrow = out_dim} host (out->data is (re)allocated with malloc). */
int pk_mi355_nnet_propagate(pk_mi355_am_t *am, const pk_matrix_t *in, pk_matrix_t *out);

/* ------------------------------------------------------------------------- */
/* Front-end -- replaces Fbank (fbank.h:47-110) and CMVN (cmvn.h:17-45)           */
/* ------------------------------------------------------------------------- */

/* Fbank::CalcNumFrames, fbank.cc:35-42 */
int pk_mi355_num_frames(int num_samples);

/* Fbank::Compute, fbank.cc:267-292: wave (host, 16 kHz, unscaled sample values)
 * -> out {ncol = T, nrow = 40} host (resized with malloc/realloc).               */
int pk_mi355_fbank_compute(const pk_vector_t *wave, pk_matrix_t *out);

/* CMVN(global_stats, raw).GetFrame(t) for t = 0..T-1, cmvn.cc:103-125:
 * global_stats dim 41 (40 sums + count); raw {ncol = T, nrow = 40} host ->
 * out {ncol = T, nrow = 40} host.                                                */
int pk_mi355_cmvn_apply(const pk_vector_t *global_stats, const pk_matrix_t *raw,
                        pk_matrix_t *out);

/* ------------------------------------------------------------------------- */
/* Sample-rate conversion to 16 kHz: 8 .. 96 kHz in, on the GPU */
/* ------------------------------------------------------------------------- */

/* The windowed-sinc rule of Kaldi's LinearResample.  Input rate fi, output rate fo = 16000, g = gcd(fi, fo),
 * Q = fi / g input samples per unit, P = fo / g phases; cutoff fc = 0.99 * 0.5 * min(fi, fo), Z = 6 zero crossings,
 * half-width w = Z / (2 fc) seconds.  Phase p (time offset p / fo) has the taps i with |i / fi - p / fo| < w: first[p]
 * is the smallest, count[p] their number, weight[p][k] = 2 fc sinc(2 fc d) 0.5 (1 + cos(2 pi fc d / Z)) / fi with
 * d = (first[p] + k) / fi - p / fo, formed in double and rounded to float once.  Output j = u P + p is
 *     y[j] = sum over k = 0 .. count[p] - 1, ascending, of weight[p][k] * x[first[p] + u Q + k]
 * in fp32 from +0.0f, each term a rounded product then a rounded add, x outside [0, n) read as +0.0f (its term is
 * still evaluated).  n inputs give floor(n P / Q) outputs.  One arithmetic order per output sample: the result does not
 * depend on batching, tiling or chunking.  Supported: 8000 <= fi <= 96000 with P * max count <= 16384; any other rate
 * fails with PK_MI355_E_INVALID and is named in pk_mi355_last_error().  fi = 16000 is the identity and launches nothing.
 *
 * Host only, no device: the plan of a rate, its table (first[P], count[P], weights[P][max_taps] with every row
 * zero-padded behind count[p]; any pointer may be NULL) and the output count (negative code on failure).            */
int pk_mi355_resample_plan(int rate, int *Q, int *P, int *max_taps);
int pk_mi355_resample_table(int rate, int32_t *first, int32_t *count, float *weights);
int64_t pk_mi355_resample_num_output(int rate, int64_t num_samples);
/* One wave (host, sample values at `rate`) -> out (host, 16 kHz; out->data is (re)allocated with realloc()), converted
 * on the device as pk_mi355_fbank_compute computes features.                                                         */
int pk_mi355_resample(const pk_vector_t *wave, int rate, pk_vector_t *out);

/* ------------------------------------------------------------------------- */
/* Batched scorer: many utterances in flight, PCM in -> log-likelihoods out,     */
/* everything device-resident (the stages of pk_process, pocketkaldi.cc:176-218). */
/* ------------------------------------------------------------------------- */

typedef struct pk_mi355_batch pk_mi355_batch_t;

/* global_stats41: the cmvn_stats vector pk_load reads (pocketkaldi.cc:96-112).
 * Capacity: at most max_utts utterances and max_total_samples PCM samples.
 *
 * Isolation and reuse: in an F32 call an utterance's results (fbank, CMVN, log-likelihoods) are a function of
 * that utterance's samples alone -- a neighbour full of NaN, Inf or loud samples changes no bit of them, and a
 * NaN or Inf sample makes NaN exactly the rows the reference makes NaN.  Every call is a function of its own
 * inputs, whatever the object scored before (other layouts, failed calls, either ingestion path).  F16X3 / F16
 * exception: the range verdict (PK_MI355_E_RANGE) covers the whole call -- one utterance out of range withholds
 * every utterance's results -- but never a later call (tests/test_gpu_isolation.py).                        */
pk_mi355_batch_t *pk_mi355_batch_create(pk_mi355_am_t *am, const float *global_stats41,
                                        int max_utts, int64_t max_total_samples);
void pk_mi355_batch_destroy(pk_mi355_batch_t *b);

/* Hand over B utterances as host PCM (float sample values as pk_16kpcm_read
 * produces them, pcm_reader.cc:189-211); copied to HBM.                          */
int pk_mi355_batch_set_waves(pk_mi355_batch_t *b, const pk_vector_t *waves, int num_utts);
/* Same, utterance u sampled at rates[u] Hz (rates == NULL: 16000 throughout).  With 16000 everywhere this IS
 * pk_mi355_batch_set_waves.  Otherwise the utterances at 16000 are copied as set_waves copies them and the others are
 * staged at their own rate (a page-locked and a device buffer the batch makes and grows on demand) and converted on the
 * batch's stream straight to where set_waves would have put them: scoring reads the same layout.  Capacity
 * (max_total_samples) counts 16 kHz samples, the sum of pk_mi355_resample_num_output over the utterances.
 * (Named with the resampler's entries: it is pk_mi355_batch_set_waves with a conversion in front.)                  */
int pk_mi355_resample_set_waves(pk_mi355_batch_t *b, const pk_vector_t *waves, const int *rates, int num_utts);
/* Same, from one concatenated host int16 buffer (the WAV payload itself).        */
int pk_mi355_batch_set_waves_i16(pk_mi355_batch_t *b, const int16_t *samples,
                                 const int *num_samples, int num_utts);
/* Same, PCM already resident in HBM: d_samples is a device pointer to the
 * concatenated float samples of all utterances.                                  */
int pk_mi355_batch_set_waves_device(pk_mi355_batch_t *b, const float *d_samples,
                                    const int *num_samples, int num_utts);

/* ---- Features instead of audio.  Everything behind the set_* call -- score, synchronize,
 * calibrate, fetch, fetch_all, gather_loglik, loglik_device, timing, pk_mi355_decoder_decode_batch -- sees a batch
 * of num_utts utterances of T_u frames, whatever it was fed.  (Named with a prefix of their own, as
 * pk_mi355_resample_set_waves is: they are batch entries with another source in front.)                          */
#define PK_MI355_FEATS_NORMALIZED 0   /* ready for the splice, as pk_decodable_init takes them */
#define PK_MI355_FEATS_RAW        1   /* raw features (40-dim log-mel fbank, or any dimension on an object made by a
                                         _create_stats entry): the sliding-window CMVN is applied first */

/* A batch scorer without a front-end.  Any model (any feat_dim; F16X3 / F16: a multiple of 8, as pk_decodable_init).
 * global_stats41 may be NULL; given (41 floats, feat_dim must be 40) it enables PK_MI355_FEATS_RAW.  Capacity in
 * frames, not samples.  The wave entries fail with PK_MI355_E_STATE on such a batch.                             */
pk_mi355_batch_t *pk_mi355_features_batch_create(pk_mi355_am_t *am, const float *global_stats41,
                                                 int max_utts, int64_t max_total_frames);
/* The same with statistics at the model's own dimension: global_stats holds feat_dim sums, then
 * the frame count, and stats_len must be pk_mi355_am_feat_dim(am) + 1 -- otherwise PK_MI355_E_INVALID, whose text names
 * both numbers; a null model or null statistics are refused too.  At feat_dim == 40 it is the entry above.  At any other
 * dimension PK_MI355_FEATS_RAW runs cmvn.cc's rule (mean normalisation, elementwise in the feature index) column by
 * column: column d of the result is, bit for bit, what the 40-dim path gives for a matrix that holds that column, with
 * the same sum and count.                                                                                          */
pk_mi355_batch_t *pk_mi355_features_batch_create_stats(pk_mi355_am_t *am, const float *global_stats, int stats_len,
                                                       int max_utts, int64_t max_total_frames);
/* feats[u]: nrow = feat_dim, ncol = T_u, memory [T_u][feat_dim] (the pk_matrix_t image pk_decodable_init takes);
 * copied to HBM.  T_u = 0 is an utterance without rows.  Also on a batch made by pk_mi355_batch_create (feat_dim 40,
 * both kinds, capacity: the frames its sample capacity can produce, max_total_samples / 160 + max_utts); a later
 * set_waves* switches such a batch back to audio.  PK_MI355_E_INVALID, before anything is copied or launched: a null
 * argument, nrow != feat_dim, a negative ncol, an unknown kind, RAW on a batch without statistics (with feat_dim != 40
 * only pk_mi355_features_batch_create_stats gives it some) whose normalisation spec is the sliding rule
 * (pk_mi355_norm_set), more utterances, frames or columns than the capacity; the batch keeps what it held.           */
int pk_mi355_features_set(pk_mi355_batch_t *b, const pk_matrix_t *feats, int num_utts, int kind);
/* Same, features already in HBM, utterance after utterance, [sum T][feat_dim] (4-byte aligned).  NORMALIZED: not
 * copied, must stay valid until scored.  RAW: one device-to-device copy on the batch's stream.                   */
int pk_mi355_features_set_device(pk_mi355_batch_t *b, const float *d_feats, const int *num_frames,
                                       int num_utts, int kind);
int pk_mi355_features_dim(const pk_mi355_batch_t *b);

/* ---- The front-end at a specification: log-mel fbank with any number of bins over any band,
 * and MFCC on top of it, on the GPU, for models whose features are not the reference's 40-bin fbank.              */
#define PK_MI355_FRONTEND_FBANK 0
#define PK_MI355_FRONTEND_MFCC  1
#define PK_MI355_WINDOW_HAMMING 0   /* the reference's (fbank.cc:249-256) */
#define PK_MI355_WINDOW_POVEY   1   /* Kaldi's default: pow(0.5 - 0.5 cos(a i), 0.85) */
typedef struct pk_mi355_frontend_spec {
  int32_t kind;            /* PK_MI355_FRONTEND_FBANK 0, PK_MI355_FRONTEND_MFCC 1 */
  int32_t num_mel_bins;    /* 3 .. 128 */
  int32_t num_ceps;        /* MFCC: 1 .. num_mel_bins;  FBANK: must be 0 */
  int32_t window;          /* PK_MI355_WINDOW_HAMMING 0 (the reference's), PK_MI355_WINDOW_POVEY 1 (Kaldi's default) */
  float   low_freq;        /* Hz, >= 0 */
  float   high_freq;       /* Hz; <= 0: that much below 8000 (Kaldi's convention) */
  float   cepstral_lifter; /* MFCC: >= 0, 0 = none (Kaldi: 22);  FBANK: ignored */
} pk_mi355_frontend_spec_t;
/* The output dimension is num_mel_bins (fbank) or num_ceps (MFCC).  Everything else is the reference's and fixed:
 * 16 kHz, 400-sample frames every 160 samples (pk_mi355_num_frames), DC removal, pre-emphasis 0.97 in double, the
 * 512-point split-radix FFT, power spectrum, floor FLT_EPSILON, logf; no dither, energy, deltas or VTLN.
 *
 * The rule.  Up to the power spectrum P[0..256]: the arithmetic of pk_mi355_fbank_compute bit for bit, with the spec's
 * window (both formed in double and rounded to float once; Povey's cosine is the double cosine of the reference's
 * float angle step times i).  Mel triangles: fbank.cc:103-163 in the reference's float expressions with num_mel_bins
 * bins between low_freq and the resolved high_freq; a bin needs at least one tap (Kaldi's condition).  Mel energy of
 * bin b: e = +0.0f; for j ascending: e += w[j] * P[off + j] -- a rounded product, a rounded add, no fma -- then
 * max(e, FLT_EPSILON) and logf.  No spectrum value outside a bin's own taps influences it.  MFCC: c[k] = +0.0f; for b
 * ascending: c[k] += dct[k][b] * logmel[b], the same roundings; then c[k] *= lifter[k].  dct[0][b] = sqrt(1 / B),
 * dct[k][b] = sqrt(2 / B) cos(pi / B (b + 0.5) k), lifter[k] = 1 + 0.5 Q sin(pi k / Q) (Q = 0: 1), formed in double
 * and rounded to float once: Kaldi's definitions.  Kaldi leaves the order of the dot to BLAS, so agreement with Kaldi
 * is within rounding, not bitwise.
 *
 * Refused with PK_MI355_E_INVALID and a text that names the field, before any device call: an unknown kind or window;
 * num_mel_bins outside 3 .. 128; num_ceps outside 1 .. num_mel_bins (MFCC) or nonzero (fbank); a negative or
 * non-finite low_freq, a non-finite high_freq, a negative or non-finite cepstral_lifter; a resolved high_freq above
 * 8000 or not above low_freq; a triangle without a tap (the text names the bin).
 *
 * Host only, no device: the check, the dimension (negative code on failure), the reference's configuration, and the
 * tables -- window[400], mel_off[B] (first FFT bin), mel_len[B], mel_weights (the bins' taps back to back, sum of
 * mel_len <= 512 floats), dct[num_ceps][B] and lifter[num_ceps] (MFCC only; untouched for fbank); any pointer may be
 * NULL.                                                                                                             */
int pk_mi355_frontend_check(const pk_mi355_frontend_spec_t *spec);
int pk_mi355_frontend_dim(const pk_mi355_frontend_spec_t *spec);
int pk_mi355_frontend_default(pk_mi355_frontend_spec_t *spec);
int pk_mi355_frontend_tables(const pk_mi355_frontend_spec_t *spec, float *window, int32_t *mel_off, int32_t *mel_len,
                             float *mel_weights, float *dct, float *lifter);
/* One wave (host, 16 kHz, unscaled sample values) -> out {ncol = T, nrow = dim} host, as pk_mi355_fbank_compute.   */
int pk_mi355_frontend_compute(const pk_mi355_frontend_spec_t *spec, const pk_vector_t *wave, pk_matrix_t *out);
/* A batch scorer with this front-end: pk_mi355_batch_create for a model of pk_mi355_frontend_dim(spec) features.
 * global_stats: dim sums, then the frame count.  PK_MI355_E_INVALID, naming both numbers: a spec dimension that is not
 * pk_mi355_am_feat_dim(am), a stats_len that is not that + 1; F16X3 / F16 need a dimension that is a multiple of 8.
 * Every set_waves* entry (pk_mi355_resample_set_waves too; capacity counts 16 kHz samples) and everything behind
 * them works as on pk_mi355_batch_create's object, with the isolation contract above: score runs FbankAnyKernel in the
 * PK_MI355_K_FBANK slot -- always, at the default spec too -- and then the CMVN of the dimension; fetch_fbank returns
 * the front-end's rows [T][dim].  pk_mi355_features_set* work on it, and a later set_waves* switches back.  (Named
 * with the front-end's entries, as the feature entries are: pk_mi355_batch_create with another front-end.)         */
pk_mi355_batch_t *pk_mi355_frontend_batch_create(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t *spec,
                                                 const float *global_stats, int stats_len, int max_utts,
                                                 int64_t max_total_samples);

/* ---- Normalisation at a specification: what Kaldi's apply-cmvn does per utterance or per
 * speaker, with or without variance, or nothing -- instead of cmvn.cc's sliding rule -- between the front-end (or the
 * caller's raw features) and the first layer of a batch scorer.                                                    */
#define PK_MI355_NORM_SLIDING   0   /* cmvn.cc's rule (the default; what every scorer did before): means only */
#define PK_MI355_NORM_NONE      1   /* the raw rows go to the first layer as they are; both switches are ignored */
#define PK_MI355_NORM_UTTERANCE 2   /* statistics of the utterance's own frames */
#define PK_MI355_NORM_SPEAKER   3   /* statistics the caller hands over (pk_mi355_norm_set_speaker_stats) */
typedef struct pk_mi355_norm_spec {
  int32_t mode;         /* PK_MI355_NORM_* */
  int32_t norm_means;   /* 0 or 1 (SLIDING: must be 1) */
  int32_t norm_vars;    /* 0 or 1 (SLIDING: must be 0) */
} pk_mi355_norm_spec_t;
/* Statistics of one utterance or speaker at dimension D are 2 x (D + 1) doubles, the matrix compute-cmvn-stats writes:
 * row 0 the D sums and then the frame count, row 1 the D sums of squares and then 0.
 *
 * The rule, every column d on its own.  UTTERANCE, T frames: S0 = S1 = 0.0; for t ascending: S0 += (double)x[t][d],
 * S1 += (double)x[t][d] * (double)x[t][d]; N = T.  SPEAKER: S0, S1, N are the caller's.  Then, in double:
 * mean = norm_means ? S0 / N : 0; without norm_vars scale = 1, offset = -mean; with it var = S1 / N - mean * mean,
 * raised to 1e-20 where it is below (a NaN stays), scale = 1 / sqrt(var), offset = -(mean * scale).  Both are rounded
 * to float once, and y = norm_vars ? (x * scale) + offset : x + offset in float, a rounded product and a rounded add
 * (Kaldi's AccCmvnStats and ApplyCmvn).  An utterance without frames does nothing; one frame with norm_vars meets the
 * floor; a NaN makes its own column of its own utterance NaN and touches nothing else.  The statistics an UTTERANCE
 * call computes are compute-cmvn-stats' bits, and the sum of several utterances' records is a valid speaker record.
 *
 * pk_mi355_norm_check: PK_MI355_E_INVALID with a text that names the field -- a null spec, an unknown mode, a switch
 * that is neither 0 nor 1 (any mode but NONE), SLIDING with norm_means = 0 or norm_vars = 1, UTTERANCE or SPEAKER with
 * both switches 0 ("use mode none").  Host only.                                                                  */
int pk_mi355_norm_check(const pk_mi355_norm_spec_t *spec);
/* The rule on the host, for one matrix x [T][D] -> y [T][D] (not in place): the restatement the GPU path is held to.
 * stats: the 2 x (D + 1) record of SPEAKER mode (required there, ignored otherwise).  stats_out (may be NULL): the
 * record an UTTERANCE call accumulated.  SLIDING is refused: pk_mi355_cmvn_apply is that rule.  A count that is not
 * positive and finite: PK_MI355_E_INVALID.                                                                        */
int pk_mi355_norm_apply(const pk_mi355_norm_spec_t *spec, const float *x, int num_frames, int dim, const double *stats,
                        float *y, double *stats_out);
/* The spec of a batch scorer of any kind (pk_mi355_batch_create, pk_mi355_features_batch_create*,
 * pk_mi355_frontend_batch_create); it holds until it is set again and takes effect at the next score call.  With a
 * mode other than SLIDING a features-only batch made without statistics takes PK_MI355_FEATS_RAW.  With SLIDING the
 * batch launches what it always launched.  NormKernel and FeatureLayoutKernel share the PK_MI355_K_CMVN timing slot.
 * (Named with a prefix of their own, as the feature entries are: batch entries with another normalisation.)        */
int pk_mi355_norm_set(pk_mi355_batch_t *b, const pk_mi355_norm_spec_t *spec);
/* SPEAKER mode: [num_utts][2][feat_dim + 1] doubles, utterance u's speaker record at stats + u * 2 * (feat_dim + 1).
 * They belong to the NEXT score call and are consumed by it.  PK_MI355_E_INVALID, naming the utterance, for a count
 * that is not positive and finite -- here, before any launch.  pk_mi355_batch_score in SPEAKER mode without records,
 * or with records for another number of utterances than the call's: PK_MI355_E_STATE.                            */
int pk_mi355_norm_set_speaker_stats(pk_mi355_batch_t *b, const double *stats, int num_utts);
/* The 2 x (feat_dim + 1) record the last score call computed for utterance utt in UTTERANCE mode;
 * PK_MI355_E_STATE when the last score was not one in that mode.                                                   */
int pk_mi355_norm_fetch_stats(pk_mi355_batch_t *b, int utt, double *out);

/* ---- Online CMVN: Kaldi's OnlineCmvn -- the rule of apply-cmvn-online and of a live recogniser
 * -- restated: a sliding window of cmn_window frames carried in double, with or without variance, smoothed first by the
 * speaker's statistics and then by global ones while the window is not yet full.  Means are always normalised.  (Not
 * compared with a Kaldi binary; no Freeze, no skip_dims.)                                                          */
typedef struct pk_mi355_online_cmvn_spec {
  int32_t cmn_window;       /* W, in [1, 6000]; Kaldi's default 600 */
  int32_t speaker_frames;   /* >= 0; at most this many frames of the speaker's statistics smooth a window (600) */
  int32_t global_frames;    /* >= 0; at most this many frames of the global statistics (200); > 0 needs them */
  int32_t norm_vars;        /* 0 or 1 */
} pk_mi355_online_cmvn_spec_t;
/* Global and speaker statistics are 2 x (D + 1) doubles, as above.  The rule, every column d on its own, the state in
 * double: S0 = S1 = 0.0; for t ascending:
 *   1. S0 += (double)x[t], then S1 += (double)x[t] * (double)x[t];
 *   2. if t >= W: S0 -= (double)x[t - W], then S1 -= (double)x[t - W] * (double)x[t - W] (after the additions);
 *   3. N = min(t + 1, W);
 *   4. on copies s0, s1, N, every a + f * b a rounded product and a rounded add: nothing if N >= W; with a speaker
 *      record of count C > 0: c = min(W - N, speaker_frames, C), and if c > 0: f = c / C, s0 += f * spk[0][d],
 *      s1 += f * spk[1][d], N += f * C; if still N < W and global_frames > 0: c = min(W - N, global_frames), f = c / G
 *      (G the global count), s0 += f * glob[0][d], s1 += f * glob[1][d], N += f * G;
 *   5. mean, scale, offset and y[t] from s0, s1, N as above (norm_means = 1; the floor 1e-20; one rounding to float each).
 * The smoothed copies never feed back into S0, S1.  No frames: nothing happens.  A NaN makes its own column of its own
 * utterance NaN from its frame on (x - x of a NaN or an inf is NaN: it does not leave with the window).
 *
 * pk_mi355_online_cmvn_check: PK_MI355_E_INVALID with a text that names the field -- a null spec, cmn_window outside
 * [1, 6000], a negative speaker_frames or global_frames, a norm_vars that is neither 0 nor 1, global_frames > 0 with
 * global_stats NULL or with a global count (global_stats[dim]) that is not positive and finite.  global_stats may be
 * NULL when global_frames is 0.  Host only.                                                                        */
int pk_mi355_online_cmvn_check(const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats, int dim);
/* The rule on the host, for one matrix x [T][D] -> y [T][D] (not in place): the restatement the GPU path is held to.
 * speaker_stats (may be NULL: no speaker prior; a count of 0 means the same): PK_MI355_E_INVALID for a count that is
 * negative or not finite.  state_out (may be NULL): 2 x (D + 1) doubles, the window state behind the last frame -- row
 * 0 the D sums S0 and then the frames seen, row 1 the D sums S1 and then 0.                                        */
int pk_mi355_online_cmvn_apply(const pk_mi355_online_cmvn_spec_t *spec, const float *x, int num_frames, int dim,
                               const double *global_stats, const double *speaker_stats, float *y, double *state_out);
/* Online CMVN as the normalisation of a batch scorer of any kind, in NormKernel's place: OnlineCmvnKernel, then
 * FeatureLayoutKernel, in the PK_MI355_K_CMVN timing slot.  global_stats: 2 x (feat_dim + 1) doubles, copied (NULL
 * with global_frames = 0).  The refusals are pk_mi355_online_cmvn_check's, before any launch; the batch then keeps the
 * norm it had.  It holds until a pk_mi355_norm_set leaves it.  As with every spec but SLIDING, a features-only batch
 * made without statistics then takes PK_MI355_FEATS_RAW.  pk_mi355_norm_set_speaker_stats is legal in this mode: the
 * records are optional, belong to the next score call and are consumed by it; a count that is negative or not finite
 * is PK_MI355_E_INVALID (the utterance named), records for another number of utterances than the call's make
 * pk_mi355_batch_score fail with PK_MI355_E_STATE.  pk_mi355_norm_fetch_stats has nothing to return in this mode
 * (PK_MI355_E_STATE).  Device memory, made at the first call: the [max_frames][feat_dim] float staging (shared with
 * the other modes) and 16 * (feat_dim + 1) * (max_utts + 1) bytes of statistics.                                    */
int pk_mi355_norm_set_online_cmvn(pk_mi355_batch_t *b, const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats);

/* ---- Delta features: Kaldi's add-deltas between the normalisation and the splice of a batch
 * scorer, for models whose first layer expects (order + 1) x the dimension the front-end, the statistics and the
 * normalisation work at (13 MFCC -> 39, 40 fbank -> 120).  Restated from Kaldi's DeltaFeatures; not compared with a
 * Kaldi binary (Kaldi leaves the axpy to BLAS, so agreement with it is within rounding).  No energy.  The online
 * objects: pk_mi355_deltas_stream_create below.                                                                    */
typedef struct pk_mi355_deltas_spec {
  int32_t order;    /* 1 .. 3 (Kaldi's default 2) */
  int32_t window;   /* 1 .. 8 (Kaldi's default 2) */
} pk_mi355_deltas_spec_t;
/* Base dimension Db -> output dimension (order + 1) * Db: block 0 the features, block i their i-th differences.
 *
 * Scales, in float: s[0] = [1.0f].  For i = 1 .. order: s[i] has len(s[i-1]) + 2 * window entries, all +0.0f at first;
 * with po = (len(s[i-1]) - 1) / 2, for j = -window .. window ascending and inside that for k = -po .. po ascending:
 * s[i][j + k + po + window] += (float)j * s[i-1][k + po], a rounded product and a rounded add; then every entry is
 * multiplied by (float)(1.0 / (double)normalizer), normalizer the sum of j * j accumulated in float.
 *
 * Apply, every column on its own, T frames: block i of output frame t is acc = +0.0f; for j = -M_i .. M_i ascending
 * (M_i = i * window): if s[i][j + M_i] != 0.0f then acc = acc + (s[i][j + M_i] * x[clamp(t + j, 0, T - 1)]), a rounded
 * product and a rounded add, no fma.  Taps whose scale is zero are skipped, as Kaldi skips them (an inf at the centre
 * of a first-order delta does not become NaN).  Block 0 is therefore +0.0f + 1.0f * x: -0.0 comes out as +0.0, NaN and
 * inf pass through.  No frames: nothing happens.  A NaN spoils its own column only, within M_i frames of it, in its own
 * utterance.
 *
 * pk_mi355_deltas_check: PK_MI355_E_INVALID with a text that names the field -- a null spec, order outside [1, 3],
 * window outside [1, 8].  pk_mi355_deltas_dim: (order + 1) * base_dim, or the negative code.  pk_mi355_deltas_scales:
 * the table, [order + 1][2 * order * window + 1] floats, row i centred (entry j of s[i] at column order * window + j)
 * and zero around it.  pk_mi355_deltas_apply: the rule on the host for one matrix x [T][base_dim] ->
 * y [T][(order + 1) * base_dim] (not in place): the restatement the GPU path is held to.  Host only, all four.      */
int pk_mi355_deltas_check(const pk_mi355_deltas_spec_t *spec);
int pk_mi355_deltas_dim(const pk_mi355_deltas_spec_t *spec, int base_dim);
int pk_mi355_deltas_scales(const pk_mi355_deltas_spec_t *spec, float *table);
int pk_mi355_deltas_apply(const pk_mi355_deltas_spec_t *spec, const float *x, int num_frames, int base_dim, float *y);
/* A batch scorer with deltas in front of the splice.  Db = pk_mi355_am_feat_dim(am) / (order + 1), which must divide
 * exactly.  frontend: a spec of Db features (then capacity counts 16 kHz samples, and global_stats is required), or
 * NULL: features only (capacity counts frames; global_stats may be NULL, as on pk_mi355_features_batch_create).
 * global_stats: Db sums and the count; stats_len must be Db + 1.  PK_MI355_E_INVALID, naming both numbers, for a
 * feat_dim that (order + 1) does not divide, a front-end of another dimension than Db, another stats_len; the deltas
 * and front-end specs are refused in their checks' words; F16X3 / F16 need feat_dim to be a multiple of 8.
 * Stage order: front-end or the caller's PK_MI355_FEATS_RAW rows [T][Db] -> the normalisation at Db (any spec of
 * pk_mi355_norm_set or pk_mi355_norm_set_online_cmvn; SLIDING at any Db, 40 too, runs the chain kernel, whose columns
 * are the 40-dim path's bit for bit) -> DeltaKernel into a [max_frames][feat_dim] staging of its own, inside the
 * PK_MI355_K_CMVN timing slot -> the layout at feat_dim -> the layers.  On such a batch everything in front of the
 * deltas is at Db: the RAW rows of pk_mi355_features_set*, fetch_fbank, speaker and global records, fetch_stats.
 * PK_MI355_FEATS_NORMALIZED features stay "ready for the splice": [T][feat_dim], past the norm and the deltas.
 * pk_mi355_batch_fetch_cmvn returns what the first layer reads, [T][feat_dim].                                      */
pk_mi355_batch_t *pk_mi355_deltas_batch_create(pk_mi355_am_t *am, const pk_mi355_deltas_spec_t *deltas,
                                               const pk_mi355_frontend_spec_t *frontend, const float *global_stats,
                                               int stats_len, int max_utts, int64_t capacity);
/* Db of a batch made by the entry above; feat_dim on every other batch; 0 for NULL.                                 */
int pk_mi355_deltas_base_dim(const pk_mi355_batch_t *b);

/* ---- Feature transforms: Kaldi's splice-feats | transform-feats (LDA+MLLT: 13 x 7 = 91 -> 40)
 * and per-utterance transform-feats (fMLLR: 40 -> 40, a matrix per speaker) as the last stage in front of the first
 * layer of a batch scorer, behind the normalisation and the deltas.  Restated from the tools' description (splice-feats
 * repeats the first and last frame; transform-feats does AddMatMat, then adds the offset column with AddVecToRows --
 * hence "offset last"); it has not been compared with a Kaldi binary, and Kaldi leaves the product's order to BLAS, so
 * agreement with Kaldi is within rounding.  The online objects: pk_mi355_transform_stream_create below.              */
typedef struct pk_mi355_transform_spec {
  int32_t left_context, right_context;   /* frames spliced to the left and right: each 0 .. 16, together at most 16 */
  int32_t in_dim;                        /* Dp, the width of the rows the stage reads: 1 .. 512 */
  int32_t rows, cols;                    /* the matrix: rows 1 .. 2048 outputs; cols K = (left + right + 1) * Dp (linear)
                                            or K + 1 (affine: the last column is the offset) */
  const float *matrix;                   /* row-major [rows][cols], Kaldi's layout; every entry finite */
} pk_mi355_transform_spec_t;
/* in_dim is explicit because at left = right = 0 a 41-column matrix may be 41 -> linear or 40 -> affine.
 * matrix == NULL with rows == cols == 0 and left == right == 0: no global stage -- the object then exists for
 * per-utterance matrices only, and its output dimension is in_dim.
 *
 * One output o of frame t of an utterance of T frames, in float, with L = left_context, R = right_context:
 *   acc = +0.0f
 *   for j = -L .. R ascending, for d = 0 .. Dp - 1 ascending:
 *     acc = acc + (m[o][(j + L) * Dp + d] * x[clamp(t + j, 0, T - 1)][d])      a rounded product, a rounded add, no fma
 *   if affine: acc = acc + m[o][K]
 * No tap is skipped: a zero matrix entry times an inf is NaN, as BLAS would give.  T == 0: nothing happens.  A NaN at
 * x[t][d] makes every output of frames [t - R, t + L] of its own utterance NaN and touches nothing else.  -0.0 cannot
 * survive the +0.0f start.  The per-utterance stage is the same rule with L = R = 0, in_dim = the global stage's output
 * dimension (the model's feat_dim) and utterance u's own [feat_dim][feat_dim] or [feat_dim][feat_dim + 1] matrix; it
 * runs after the global stage, in the call for which matrices were handed over.
 *
 * pk_mi355_transform_check: PK_MI355_E_INVALID with a text that names the field -- a null spec, a context outside
 * [0, 16] or a sum above 16, in_dim outside [1, 512], rows outside [1, 2048], cols that is neither K nor K + 1 (both
 * numbers named), a null matrix in any but the all-zero form, an entry that is not finite (the first such row and
 * column named).  pk_mi355_transform_out_dim: rows (in_dim without a matrix), or the negative code.
 * pk_mi355_transform_apply: the rule on the host for one matrix x [T][in_dim] -> y [T][out_dim] (not in place; without
 * a matrix a copy): the restatement the GPU path is held to.  Host only, all three.                                  */
int pk_mi355_transform_check(const pk_mi355_transform_spec_t *spec);
int pk_mi355_transform_out_dim(const pk_mi355_transform_spec_t *spec);
int pk_mi355_transform_apply(const pk_mi355_transform_spec_t *spec, const float *x, int num_frames, float *y);
/* A batch scorer with the transform in front of the splice.  deltas may be NULL; frontend NULL: features only (capacity
 * counts frames; global_stats may be NULL), else capacity counts 16 kHz samples and global_stats is required.
 * Db = in_dim / (order + 1) with deltas (must divide), in_dim without; a front-end must produce Db; stats_len must be
 * Db + 1; pk_mi355_transform_out_dim must be pk_mi355_am_feat_dim(am).  PK_MI355_E_INVALID naming both numbers
 * otherwise.  Checked in this order: model state, null arguments, deltas spec, transform spec, divisibility, front-end
 * spec, front-end dimension, stats_len, output dimension, capacity, the f16 multiple-of-8 rule on feat_dim.
 * Stage order: front-end or the caller's PK_MI355_FEATS_RAW rows [T][Db] -> the normalisation at Db (any spec; SLIDING
 * runs the chain kernel at every Db) -> DeltaKernel (with deltas) -> TransformKernel with the global matrix (if there is
 * one) -> TransformKernel with the matrices of pk_mi355_transform_set_utt (if any were handed over for the call) -> the
 * layout at feat_dim -> the layers; the transform launches lie inside the PK_MI355_K_CMVN timing slot.  Everything in
 * front of the transform is at Db, as on a deltas batch: the RAW rows of pk_mi355_features_set*, fetch_fbank, speaker
 * and global records, fetch_stats.  PK_MI355_FEATS_NORMALIZED features stay [T][feat_dim], past every stage.
 * pk_mi355_batch_fetch_cmvn returns what the first layer reads.  The matrix is copied: it need not outlive the call.  */
pk_mi355_batch_t *pk_mi355_transform_batch_create(pk_mi355_am_t *am, const pk_mi355_transform_spec_t *transform,
                                                  const pk_mi355_deltas_spec_t *deltas, const pk_mi355_frontend_spec_t *frontend,
                                                  const float *global_stats, int stats_len, int max_utts, int64_t capacity);
/* in_dim of a batch made by the entry above; feat_dim on every other batch; 0 for NULL.                             */
int pk_mi355_transform_in_dim(const pk_mi355_batch_t *b);
/* Per-utterance matrices for the NEXT score call, which consumes them (as speaker records): mats [num_utts][rows][cols],
 * rows = feat_dim, cols = feat_dim (linear) or feat_dim + 1 (affine), else PK_MI355_E_INVALID; an entry that is not
 * finite is PK_MI355_E_INVALID and names the utterance.  Matrices for another number of utterances than the call's make
 * pk_mi355_batch_score fail with PK_MI355_E_STATE; so does this call on a batch not made by
 * pk_mi355_transform_batch_create.  No matrices handed over: the stage does not run.                                */
int pk_mi355_transform_set_utt(pk_mi355_batch_t *b, const float *mats, int rows, int cols, int num_utts);

/* ---- Kaldi archives and script files of float matrices: where features usually are on disk.
 * Read on the host, HIP-free.  Binary ("\0B", "FM " / "DM ", 4 + int32 rows, 4 + int32 cols, values) and text (" [", one
 * row per line, " ]") matrices, any mixture in one archive; doubles are narrowed with one (float) cast.  An archive is
 * read entry by entry, and every size a file states is checked against the bytes that remain before anything is
 * allocated.  PK_MI355_E_IO: a file that cannot be opened, a truncated object, a size byte other than 4, negative
 * dimensions, a ragged text matrix, garbage where a key or token belongs.  PK_MI355_E_INVALID: well-formed input this
 * reader does not take, named in pk_mi355_last_error (an scp line by its number): compressed matrices ("CM ", "CM2 ",
 * "CM3 ": write them uncompressed), vectors ("FV ", "DV "), scp row or column ranges ("path[a:b]"), pipes and "-".  */
typedef struct pk_mi355_ark pk_mi355_ark_t;
/* spec: "ark:<path>", "scp:<path>" (options as in "ark,t:" are skipped), or a bare path: a ".scp" suffix means a script
 * file ("<key> <path>" or "<key> <path>:<offset>" per line, paths opened as given), anything else an archive.  NULL on
 * failure.                                                                                                          */
pk_mi355_ark_t *pk_mi355_ark_open(const char *spec);
/* Advance: 1 for an entry, 0 at the end, a negative code for an error (every later call repeats the code).         */
int pk_mi355_ark_next(pk_mi355_ark_t *h);
/* The current entry's key ("" when there is none) and matrix: view->nrow = the feature dimension, view->ncol = the
 * frames, memory [frames][dim] -- the image pk_mi355_features_set takes.  Both are valid until the next call on h.  */
const char *pk_mi355_ark_key(const pk_mi355_ark_t *h);
int pk_mi355_ark_matrix(const pk_mi355_ark_t *h, pk_matrix_t *view);
/* The current entry's values as doubles, before the narrowing, [rows][cols] into out (capacity: doubles it holds) -> the
 * number written.  Kept for matrices of at most two rows: CMVN statistics records (compute-cmvn-stats writes doubles,
 * and a variance is the difference of two of its quotients).  PK_MI355_E_INVALID: more rows, or a buffer too small.  */
int pk_mi355_ark_matrix_f64(const pk_mi355_ark_t *h, double *out, int capacity);
void pk_mi355_ark_close(pk_mi355_ark_t *h);
/* One keyless object from "path" or "path:offset" (a global CMVN statistics file, say): a handle whose current entry
 * is that object (pk_mi355_ark_matrix; pk_mi355_ark_next gives 0), to be closed as any other.  NULL on failure.     */
pk_mi355_ark_t *pk_mi355_ark_read_object(const char *rxfilename);

/* Run fbank -> CMVN -> nnet -> log-likelihood tail for the current utterances.
 * Asynchronous on the batch's stream unless sync != 0.  Results stay in HBM.     */
int pk_mi355_batch_score(pk_mi355_batch_t *b, float prob_scale, int sync);
int pk_mi355_batch_synchronize(pk_mi355_batch_t *b);
/* F16X3 / F16: pk_mi355_am_calibrate on the utterances currently set (front-end included).  Overwrites the
 * batch's results; score again afterwards.                                                               */
int pk_mi355_batch_calibrate(pk_mi355_batch_t *b);

int pk_mi355_batch_num_utts(const pk_mi355_batch_t *b);
int pk_mi355_batch_num_frames(const pk_mi355_batch_t *b, int utt);
int64_t pk_mi355_batch_total_frames(const pk_mi355_batch_t *b);

/* Device pointer to utterance utt's [T][num_pdfs] log-likelihoods.               */
const float *pk_mi355_batch_loglik_device(const pk_mi355_batch_t *b, int utt);
/* Copy utterance utt's results into a host decodable (malloc'd log_prob), ready
 * for Decoder::Decode (decoder.cc:39).                                           */
int pk_mi355_batch_fetch(pk_mi355_batch_t *b, int utt, pk_decodable_t *out);
/* All utterances at once: ONE device-to-host transfer into a page-locked arena the batch owns
 * (made on first use), and out[0..num_out) (num_out == pk_mi355_batch_num_utts) filled as
 * decodables whose log_prob VIEWS that arena -- same fields, same [T][num_pdfs] layout, usable
 * by Decoder::Decode like any other (decoder.cc:39); their `am` field is an opaque tagged handle
 * (that is how pk_decodable_destroy tells a view from a malloc'd matrix): copy such a struct whole
 * and hand it to the pk_decodable_* functions only.  pk_decodable_destroy on such a view
 * frees nothing of the caller's and may happen at any time, also after pk_mi355_batch_destroy
 * (pocketkaldi.cc:247 destroys its decodable unconditionally): the arena is released when the
 * batch is gone AND the views of its last fetch_all have been destroyed (each fetch_all is a
 * generation of its own: destroying views of an earlier one never releases memory under the
 * current ones).  Rely on the CONTENTS of the views only until the batch is scored again or
 * destroyed; the views of the LAST fetch_all in fact stay readable until the last of them goes.  With sync == 0 the copy is queued on
 * the device's result stream, ordered after this batch's scoring and before anything queued
 * later on the batch's stream; pk_mi355_batch_synchronize completes it, so it overlaps another
 * batch's scoring.  F16X3 / F16 with sync == 0: the views exist before the score call's range verdict does; if
 * pk_mi355_batch_synchronize then returns PK_MI355_E_RANGE the results are withheld -- pk_decodable_loglikelihood
 * on those views returns NaN from then on (do not read log_prob.data of views whose synchronize failed).      */
int pk_mi355_batch_fetch_all(pk_mi355_batch_t *b, pk_decodable_t *out, int num_out, int sync);
/* Intermediate stages, for parity tests: raw fbank / CMVN'd features of utt, copied to host as [T][40] /
 * [T][feat_dim].  fetch_cmvn returns what the first layer reads: after pk_mi355_features_set(NORMALIZED) the input itself,
 * bit for bit.  fetch_fbank after pk_mi355_features_set(RAW) returns the input; after NORMALIZED there is no fbank:
 * PK_MI355_E_STATE.                                                                                           */
int pk_mi355_batch_fetch_fbank(pk_mi355_batch_t *b, int utt, float *out);
int pk_mi355_batch_fetch_cmvn(pk_mi355_batch_t *b, int utt, float *out);
/* Parity-test hook: the front-end's logf (fbank.cc:244-245 -> vector.cc:334-339 -> libm logf,
 * restated for the device in csrc/pk_logf.h) on n host floats (positive normal, +inf or NaN).  */
int pk_mi355_test_logf(const float *x, int n, float *out);
/* Parity-test hook: the front-end's 512-point real FFT alone -- pk_srfft_compute (srfft.cc:371-461,
 * forward) as FbankKernel runs it, on num_frames host frames of 512 floats; spectra receives the
 * reference's packed layout [Re0+Im0, Re0-Im0, Re1, Im1, ..., Re255, Im255] per frame.            */
int pk_mi355_test_srfft512(const float *frames, int num_frames, float *spectra);

/* Device-side pk_decodable_loglikelihood (decodable.cc:24-31) for a GPU-resident consumer
 * (decoder.cc:252-279 evaluates one (frame, transition-id) pair per arc): n pairs in
 * device memory -> out[i] = log_prob[frame[i]][tid2pdf[trans_id[i]]] of utterance utt,
 * on the batch's stream, nothing leaves HBM.                                       */
int pk_mi355_batch_gather_loglik(pk_mi355_batch_t *b, int utt, const int32_t *d_frames,
                                 const int32_t *d_trans_ids, int n, float *d_out);

/* Device buffers for callers without a HIP toolchain of their own (the inputs of
 * pk_mi355_batch_set_waves_device / pk_mi355_batch_gather_loglik).  A process must use ONE
 * HIP runtime: allocate through these (or through the runtime this library is bound to).
 * kind: 1 host->device, 2 device->host, 3 device->device; synchronous.              */
void *pk_mi355_device_malloc(size_t bytes);
void pk_mi355_device_free(void *ptr);
int pk_mi355_memcpy(void *dst, const void *src, size_t bytes, int kind);
/* Page-locked host memory for PCM handed to pk_mi355_batch_set_waves_i16 / _set_waves: from
 * such a buffer the upload is a true asynchronous DMA that overlaps another batch's scoring
 * and result transfer (from pageable memory the runtime stages it and the call blocks).     */
void *pk_mi355_host_malloc(size_t bytes);
void pk_mi355_host_free(void *ptr);

/* The HIP stream the batch launches on (hipStream_t as void*), so callers can
 * bracket it with their own events.                                              */
void *pk_mi355_batch_stream(pk_mi355_batch_t *b);

/* Per-kernel timing of the LAST score call measured with hipEvents on the batch's
 * stream (enable before scoring).  Kinds index the arrays below.                 */
enum {
  PK_MI355_K_FBANK = 0,
  PK_MI355_K_CMVN = 1,       /* features: FeatureLayoutKernel after NORMALIZED (and no fbank launch) */
  PK_MI355_K_GEMM = 2,       /* all affine-layer launches */
  PK_MI355_K_TAIL = 3,       /* log-softmax / prior / scale */
  PK_MI355_K_OTHER = 4,
  PK_MI355_K_COUNT = 5
};
int pk_mi355_batch_enable_timing(pk_mi355_batch_t *b, int enable);
/* total milliseconds and launch count per kind for the last score call           */
int pk_mi355_batch_get_timing(pk_mi355_batch_t *b, float ms[PK_MI355_K_COUNT],
                              int launches[PK_MI355_K_COUNT]);
/* algorithmic FLOPs of the affine layers per frame (2 * sum K*N)                 */
double pk_mi355_am_flops_per_frame(const pk_mi355_am_t *am);

/* ------------------------------------------------------------------------- */
/* The acoustic half of pk_process (pocketkaldi.cc:176-218) and its input reader   */
/* ------------------------------------------------------------------------- */

/* pk_16kpcm_read, pcm_reader.cc:45-220: strict 44-byte-header RIFF/WAVE PCM, mono,
 * 16 kHz, 8/16/32-bit; samples are stored unscaled as float.  pcm_data->data is
 * (re)allocated with realloc().  Host only, needs no GPU.                          */
int pk_mi355_16kpcm_read(const char *filename, pk_vector_t *pcm_data);
/* The same reader for the files people have: the same header checks in the same order, but any positive sample rate
 * and 1 .. 8 interleaved channels (byte_rate and block_align are checked against the channel count).  pcm_data
 * receives channel `channel` (0-based), de-interleaved on the host, sample values as pk_mi355_16kpcm_read gives them;
 * *rate and *channels (may be NULL) the header's.  A channel outside the file is PK_MI355_E_INVALID; a trailing
 * partial sample block is dropped, as pk_16kpcm_read drops a partial sample.  Host only, needs no GPU.             */
int pk_mi355_wave_read(const char *filename, int channel, pk_vector_t *pcm_data, int *rate, int *channels);

/* Stages 1-3 of pk_process fused on the device: raw_wave -> fbank -> CMVN -> nnet ->
 * decodable (host log_prob, ready for Decoder::Decode).  An empty wave gives an empty
 * decodable (pocketkaldi.cc:180-184).  verbose != 0 prints the reference's per-stage
 * lines ("Fbank: ..ms", "CMVN: ..ms", "NNET: ..ms", pocketkaldi.cc:194,206,218) to stderr. */
int pk_mi355_process_acoustic(pk_mi355_am_t *am, const pk_vector_t *cmvn_global_stats,
                              const pk_vector_t *raw_wave, float prob_scale, pk_decodable_t *out,
                              int verbose);

/* ------------------------------------------------------------------------- */
/* Graph and decoder -- Fst (fst.h) + Decoder::Decode / BestPath (decoder.cc:39-339) */
/* on the GPU, batched: one workgroup per utterance, log-likelihoods read in HBM.     */
/* Semantics and the three deliberate differences from the reference: DESIGN.md.     */
/* ------------------------------------------------------------------------- */

/* Fst::Read (fst.cc:29-92): section name "pk::fst_0", i32 size, i32 states, arcs, start,
 * float final[states], i32 first[states], arcs {i32 next, ilabel, olabel; float weight}.
 * Host only, needs no GPU.  NULL on failure: PK_MI355_E_IO for a malformed file (name, size,
 * truncation), PK_MI355_E_INVALID for a graph that does not make sense (next state, start state
 * or arc range out of range, negative label); pk_mi355_last_error() says which.            */
typedef struct pk_mi355_fst pk_mi355_fst_t;
pk_mi355_fst_t *pk_mi355_fst_read(const char *path);
void pk_mi355_fst_destroy(pk_mi355_fst_t *fst);
int pk_mi355_fst_num_states(const pk_mi355_fst_t *fst);
int pk_mi355_fst_num_arcs(const pk_mi355_fst_t *fst);
int pk_mi355_fst_start(const pk_mi355_fst_t *fst);
/* Fst::CountArcs (fst.cc:94-110), its quirk included: a state's arcs end at the `first` of the
 * next state whose first is > 0 (not >= 0).  *count = 0 for a state with first < 0.           */
int pk_mi355_fst_arc_range(const pk_mi355_fst_t *fst, int state, int *first, int *count);

/* A device copy of the graph, checked against am: every non-zero ilabel must map through the
 * model's tid2pdf (identity without one) to a pdf < num_pdfs, otherwise PK_MI355_E_INVALID.
 * max_utts: utterances per call.  trace_capacity: tokens of backtrace storage (8 bytes each)
 * shared by the utterances of one call; 0 = 2^27.  Device memory: 68 bytes x states x max_utts
 * + 12 x trace_capacity + the graph (DESIGN.md "Decoder"; pk_mi355_decoder_set_alignment adds 4 bytes x arcs
 * + 8 bytes x frames of a call from its first enable on).  The decoder is bound to am: it
 * decodes batches scored with that model only.  A decoder belongs to one host thread at a
 * time, like a batch.  Arc weights must be finite and final weights not NaN (the reader
 * rejects others with PK_MI355_E_INVALID).                                                    */
typedef struct pk_mi355_decoder pk_mi355_decoder_t;
pk_mi355_decoder_t *pk_mi355_decoder_create(const pk_mi355_fst_t *fst, const pk_mi355_am_t *am,
                                            int max_utts, int64_t trace_capacity);
void pk_mi355_decoder_destroy(pk_mi355_decoder_t *d);
/* Decoder::beam_ (default 16.0) and kBeamSize (max-active, default 30000).                    */
int pk_mi355_decoder_set_beam(pk_mi355_decoder_t *d, float beam, int max_active);
/* Backtrace garbage collection, off (0) by default; takes effect at the next decode /
 * decode_batch (a call already queued keeps the mode it was queued with, as with set_beam).
 * On: each of the n utterances of a call owns floor(trace_capacity / n) records of the arena
 * (n is that call's count, not max_utts) and compacts them -- keeps the records its live tokens
 * can still reach -- whenever more than half are in use before a frame.  Results are the same,
 * bit for bit; what is bounded is no longer the records a call writes but those one utterance
 * keeps alive: a slice needs about twice its live records plus one frame's records
 * (pk_mi355_decoder_trace_stats measures it).  A slice still full after compaction, or a frame
 * that writes more than the free part, ends the call with PK_MI355_E_CAPACITY as below.  No
 * additional device memory.                                                                    */
int pk_mi355_decoder_set_trace_gc(pk_mi355_decoder_t *d, int enable);
/* All utterances of a scored batch, on the batch's stream, ordered after its scoring; nothing
 * leaves HBM.  If the score call ended in PK_MI355_E_RANGE the results are withheld (with
 * sync == 0 pk_mi355_decoder_synchronize returns the code).  The batch must be neither scored
 * again nor destroyed before the decoder has been synchronised.                               */
int pk_mi355_decoder_decode_batch(pk_mi355_decoder_t *d, pk_mi355_batch_t *b, int sync);
/* Host decodables ({ncol = T, nrow = num_pdfs}; fetch_all views accepted): uploaded, then
 * decoded.  With sync == 0 the decodables' memory must stay valid until synchronize.          */
int pk_mi355_decoder_decode(pk_mi355_decoder_t *d, const pk_decodable_t *utts, int num_utts, int sync);
/* Waits for the last call.  PK_MI355_E_CAPACITY (trace storage exhausted) and
 * PK_MI355_E_INVALID (a negative epsilon cycle kept the closure from settling) name the first
 * utterance concerned in pk_mi355_last_error(); no result of that call is readable then.        */
int pk_mi355_decoder_synchronize(pk_mi355_decoder_t *d);
/* Results of the last call, readable after synchronize (or sync != 0).  Words in spoken order
 * (as pk_process prints them after its std::reverse, pocketkaldi.cc:226-227; at most max_words
 * written), weight = Hypothesis::weight() (the final weight counted twice, as the reference
 * does), ok = Decode()'s return (0 also where the beam emptied mid-utterance: no words, weight
 * 0).  Returns the word count.                                                                 */
int pk_mi355_decoder_result(const pk_mi355_decoder_t *d, int utt, int *words, int max_words,
                            float *weight, int *ok);
/* Test hooks: the original arc ids of the best path (epsilon arcs included, start to end; at
 * most max_arcs written, the length returned), and the largest per-frame count of states the
 * decoder touched in utt (states <= R0 after the emitting step plus those the closure added):
 * an upper bound on the reference's token count, so <= max-active shows it did not bind.      */
int pk_mi355_decoder_best_path_arcs(const pk_mi355_decoder_t *d, int utt, int32_t *arcs, int max_arcs);
int pk_mi355_decoder_active_bound(const pk_mi355_decoder_t *d, int utt);
/* Backtrace use of the last call, for sizing trace_capacity (any pointer may be NULL).  With
 * trace gc on: the most records utt's slice held at once (sampled before every compaction and
 * at the end), the slice's size, and how often it was compacted.  With it off: the records the
 * whole call wrote (the same for every utt), trace_capacity, and 0.  PK_MI355_E_STATE before
 * any result is readable.                                                                      */
int pk_mi355_decoder_trace_stats(const pk_mi355_decoder_t *d, int utt, int64_t *peak_records,
                                 int64_t *slice_records, int *compactions);

/* ------------------------------------------------------------------------- */
/* Online scorer -- live PCM in chunks, pk_process's acoustic stages (pocketkaldi.cc: */
/* 176-218) frame by frame as frames become final; DESIGN.md section 10.             */
/* ------------------------------------------------------------------------- */

/* The reference pipeline is causal: fbank frame t reads samples [160 t, 160 t + 400) (fbank.cc:35-42),
 * CMVN is online (cmvn.cc:35-71: a running window sum rounded to float every frame), and the splice needs R
 * frames of look-ahead and clamps only at the first and last frame (am.cc:65-88).  So every frame's
 * log-likelihoods equal those of pk_mi355_batch_score on the whole wave bit for bit, whatever the chunk sizes.
 *
 * A stream object has max_streams slots.  A slot is opened, fed PCM any number of times, and closed; each
 * pk_mi355_stream_step scores, for every slot, the frames that became final since the last step: frames
 * [a, n - R) while the slot is open (n: frames whose 400 samples have arrived, R: the model's right context),
 * frames [a, n) in the step after pk_mi355_stream_close (the right edge replicated, am.cc:73-75).  That step
 * frees the slot; it may then be opened again.  A slot closed with fewer than 400 samples yields no frames.
 *
 * Isolation and reuse: a slot's rows are a function of the samples pushed to that slot since it was opened --
 * what the other slots stream (NaN, Inf, loud samples) changes no bit of them.  Every opening of a slot is a
 * function of its own pushes, whatever the slot or the object carried before (tests/test_gpu_isolation.py).
 *
 * F32 models only (PK_MI355_PRECISION_F32, both softmax modes); an F16X3 or F16 model is refused with
 * PK_MI355_E_INVALID (their calibration and range verdict are per batch).  Capacity: max_step_samples PCM
 * samples pushed, over all slots, between two steps.  global_stats41: as pk_mi355_batch_create.  Like a
 * batch, a stream object belongs to one host thread at a time.  Device memory per slot: 96 000 bytes of
 * CMVN window + 3 360 bytes + 160 x (L + R) bytes; per object: step buffers sized by max_step_samples
 * (DESIGN.md section 10).                                                                              */
typedef struct pk_mi355_stream pk_mi355_stream_t;
pk_mi355_stream_t *pk_mi355_stream_create(pk_mi355_am_t *am, const float *global_stats41, int max_streams,
                                          int64_t max_step_samples);
void pk_mi355_stream_destroy(pk_mi355_stream_t *s);
/* PK_MI355_E_STATE if the slot is open, or closed and not yet flushed by a step.                   */
int pk_mi355_stream_open(pk_mi355_stream_t *s, int slot);
/* The same for audio sampled at `rate` Hz (pk_mi355_stream_open is open_rate(16000)): pk_mi355_stream_push / _push_i16 then
 * take samples at that rate, and every step first converts, on the device, the 16 kHz samples that became final -- output
 * j is final once the last input its window reads has arrived; after pk_mi355_stream_close every j < floor(n P / Q) is
 *  -- into the place pushed 16 kHz samples lie, then runs the same sequence.  Every frame's
 * log-likelihoods equal those of the batch scorer on the whole converted wave bit for bit, whatever the chunk sizes.
 * The rate is fixed until the slot is flushed; an unsupported rate fails with PK_MI355_E_INVALID and opens nothing.
 * Capacity: max_step_samples keeps its meaning, 16 kHz samples between two steps; such a slot counts floor(n P / Q) minus
 * the outputs already converted -- what a close would make final: the filter's half-width, 6 to 12 samples, more than
 * what is final now -- so that a close never exceeds the capacity; a push that would is refused with PK_MI355_E_INVALID and consumes nothing.
 * Memory: at the first such open the object makes a page-locked and a device buffer of 4 B x (6 max_step_samples +
 * 8448 max_streams) for samples at their own rate; a slot keeps the at most Q + max_taps input samples the next output
 * still reads on the host with its pushes and sends them with the next step's.                                      */
int pk_mi355_stream_open_rate(pk_mi355_stream_t *s, int slot, int rate);
/* The rate the slot was last opened at (16000 before its first opening); negative on misuse.                        */
int pk_mi355_stream_rate(const pk_mi355_stream_t *s, int slot);
/* Append host PCM (float sample values as pk_16kpcm_read produces them, pcm_reader.cc:189-211) to an
 * open slot; copied, the caller's buffer is free on return.  num_samples may be 0.  A push that would take
 * the samples pending for the next step beyond max_step_samples fails with PK_MI355_E_INVALID and
 * consumes nothing; a push to a slot that is not open fails with PK_MI355_E_STATE.                    */
int pk_mi355_stream_push(pk_mi355_stream_t *s, int slot, const float *samples, int num_samples);
/* Same, int16 samples (the WAV payload itself; exact in float).                                      */
int pk_mi355_stream_push_i16(pk_mi355_stream_t *s, int slot, const int16_t *samples, int num_samples);
/* No more samples: the next step flushes the frames held back for look-ahead.                        */
int pk_mi355_stream_close(pk_mi355_stream_t *s, int slot);
/* One step for every open or closed-but-unflushed slot (PK_MI355_E_STATE if there is none): fbank, CMVN
 * carried over from the slot's last step, layer stack and log-likelihood tail, all on the stream object's
 * HIP stream.  Asynchronous unless sync != 0.  The results of the previous step are void from here on.  */
int pk_mi355_stream_step(pk_mi355_stream_t *s, float prob_scale, int sync);
int pk_mi355_stream_synchronize(pk_mi355_stream_t *s);
/* The rows the last step scored for slot: device pointer to [count][num_pdfs] log-likelihoods of frames
 * first_frame .. first_frame + count - 1 (NULL and count 0 if it scored none).  Valid until the next step;
 * read on the stream object's stream or after pk_mi355_stream_synchronize.                            */
const float *pk_mi355_stream_loglik_device(const pk_mi355_stream_t *s, int slot, int *first_frame, int *count);
/* The same rows copied into a host decodable ({ncol = count, nrow = num_pdfs}, malloc'd like
 * pk_mi355_batch_fetch; release with pk_decodable_destroy); *first_frame (may be NULL) receives the
 * global index of its frame 0.  Synchronous.                                                          */
int pk_mi355_stream_fetch(pk_mi355_stream_t *s, int slot, pk_decodable_t *out, int *first_frame);

/* Live features.  A feature slot is opened with a kind (PK_MI355_FEATS_NORMALIZED: ready for the
 * splice; PK_MI355_FEATS_RAW: 40-dim log-mel fbank, the sliding-window CMVN is applied first, carried from step to step
 * as for audio) and fed frames, frame-major [num_frames][feat_dim], any number per push, 0 included.  With n the frames
 * received and a the frames scored: a step scores frames [a, max(a, n - R)) while the slot is open and [a, n) after its
 * close (frame 0 replicated to the left, the last frame to the right, am.cc:73-75) -- the audio slot's rule with "frames
 * computed" replaced by "frames pushed".  Over a slot's life the rows equal, bit for bit and at every chunking, those of
 * pk_mi355_features_set + pk_mi355_batch_score on the whole matrix (RAW on a wave's fbank: those of the audio slot on
 * the wave).  NORMALIZED frames are copied: every bit pattern reaches the first layer as pushed.  Isolation and reuse
 * hold as for audio; feature slots and audio slots may share a step.  close, step, synchronize, loglik_device and fetch
 * serve both slot types.
 *
 * pk_mi355_features_stream_create: an online scorer without a front-end, for a model of any feat_dim (F32 only).
 * Capacity: max_step_frames frames pushed, over all slots, between two steps.  global_stats41 may be NULL; given (41
 * floats, feat_dim must be 40) it enables PK_MI355_FEATS_RAW.  It owns no PCM buffers: pk_mi355_stream_open, _open_rate,
 * _push and _push_i16 fail on it with PK_MI355_E_STATE.  Device memory per slot: 8 x max(L + R, 1) x feat_dim bytes,
 * and with statistics the audio object's 96 000 + 160 x (1 + max(L + R, 1)) bytes of CMVN state.                      */
pk_mi355_stream_t *pk_mi355_features_stream_create(pk_mi355_am_t *am, const float *global_stats41, int max_streams,
                                                   int64_t max_step_frames);
/* The same with statistics at the model's own dimension (feat_dim sums, then the count; stats_len must be
 * pk_mi355_am_feat_dim(am) + 1, else PK_MI355_E_INVALID naming both numbers; null statistics are refused).  At
 * feat_dim == 40 the object is the one the entry above makes.  At any other dimension a RAW slot carries feat_dim
 * running sums and a ring of the last 600 raw frames: 4 x feat_dim + 2400 x feat_dim bytes per slot, beside the
 * 8 x max(L + R, 1) x feat_dim bytes of every feature slot.                                                        */
pk_mi355_stream_t *pk_mi355_features_stream_create_stats(pk_mi355_am_t *am, const float *global_stats, int stats_len,
                                                         int max_streams, int64_t max_step_frames);
/* An online scorer with this front-end: pk_mi355_stream_create for a model of
 * pk_mi355_frontend_dim(spec) features, F32 only.  Every frame's row is, bit for bit, the row of
 * pk_mi355_frontend_batch_create's object on the whole wave, at every chunking and in both softmax modes; at the
 * default spec also pk_mi355_stream_create's.  What is final is unchanged: an open slot scores [a, n - R), the step
 * after close the rest.  open, open_rate (8 - 96 kHz), push, push_i16 and open_features / push_features (RAW and
 * NORMALIZED, [n][dim]; a frame counts 160 samples) work in the same step.  Device memory per slot at dim != 40:
 * 4 x dim + 2400 x dim + 8 x max(L + R, 1) x dim bytes of CMVN state and history beside the 3 192 bytes of tails.
 * Before any device call: PK_MI355_E_INVALID for a bad spec (in pk_mi355_frontend_check's words), a spec whose
 * dimension is not the model's (both numbers named), stats_len != feat_dim + 1 (both named), an f16 model, a
 * capacity <= 0; PK_MI355_E_STATE for a model that is not finalized.  NULL on failure.                            */
pk_mi355_stream_t *pk_mi355_frontend_stream_create(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t *spec,
                                                   const float *global_stats, int stats_len, int max_streams,
                                                   int64_t max_step_samples);
/* Open slot for features of `kind`.  Also valid on an object made by pk_mi355_stream_create (40-dim, both kinds): there
 * a pushed frame counts as 160 samples against max_step_samples.  The NORMALIZED slots' device state is made at the
 * first such open.  PK_MI355_E_INVALID: an unknown kind, RAW on an object without statistics; PK_MI355_E_STATE: the
 * slot is open, or closed and not yet flushed.                                                                       */
int pk_mi355_stream_open_features(pk_mi355_stream_t *s, int slot, int kind);
/* Append num_frames x feat_dim floats to an open feature slot; copied, the caller's buffer is free on return.  A push
 * beyond the step capacity fails with PK_MI355_E_INVALID and consumes nothing; a slot that is not open, or is open for
 * audio, fails with PK_MI355_E_STATE (as pk_mi355_stream_push does on a feature slot).                               */
int pk_mi355_stream_push_features(pk_mi355_stream_t *s, int slot, const float *frames, int num_frames);
/* The model's feature dimension: the length of a pushed frame.  Negative on a null object.                          */
int pk_mi355_stream_feat_dim(const pk_mi355_stream_t *s);
/* An online scorer with deltas in front of the splice: pk_mi355_deltas_batch_create's arguments,
 * checks (in its order, with its texts) and meaning of Db, frontend (NULL: features only, capacity in frames pushed
 * between two steps; else capacity in 16 kHz samples and global_stats required), global_stats and stats_len; an f16
 * model is refused as on every stream entry.  Everything in front of the deltas works at Db, as on a deltas batch: the
 * front-end, the statistics, every normalisation the online scorer accepts (pk_mi355_stream_norm_set*: sliding -- the
 * chain kernel at every Db, 40 too --, none, speaker, online CMVN), their speaker and global records,
 * pk_mi355_stream_norm_fetch_stats, and PK_MI355_FEATS_RAW slots, whose pushes are [n][Db].  PK_MI355_FEATS_NORMALIZED
 * slots stay [n][feat_dim] and take no deltas.
 *
 * The rule for a live slot.  M = order * window, R the model's right context; per slot n normalised base frames so far,
 * nd delta frames final so far, a rows scored so far.  One step: delta frames [nd, nd') become final, nd' = closed ? n :
 * max(nd, n - M); delta frame t, block i, is the apply rule above over the normalised base frames clamp(t + j, 0, n - 1)
 * (while the slot is open t + M <= n - 1, so the upper clamp binds only after close; the lower clamp is frame 0 of this
 * opening); rows [a, b) are scored, b = closed ? nd' : max(a, nd' - R), spliced over delta frames as on every stream.
 * The look-ahead of a live slot is therefore M + R frames; a slot closed with n = 0 gives nothing, one closed with
 * n <= M + R gives all its rows at the flush, one closed a step after its last push flushes M + R frames from its
 * history.  Over a slot's life the rows are those of a batch made by pk_mi355_deltas_batch_create on the whole input
 * under the same normalisation, bit for bit, at every chunking and in both softmax modes.
 * Memory beyond a stream without deltas: 16 * M * Db bytes of ring per slot, a staging of
 * (max_frames + max_streams * M) * feat_dim floats, and M more rows per slot in the layer buffers.  A step that cannot
 * fit fails with PK_MI355_E_INVALID and consumes nothing.                                                            */
pk_mi355_stream_t *pk_mi355_deltas_stream_create(pk_mi355_am_t *am, const pk_mi355_deltas_spec_t *deltas,
                                                 const pk_mi355_frontend_spec_t *frontend, const float *global_stats,
                                                 int stats_len, int max_streams, int64_t capacity);
/* Db of a stream made by the entry above; feat_dim on every other stream; PK_MI355_E_INVALID for NULL.              */
int pk_mi355_stream_base_dim(const pk_mi355_stream_t *s);
/* An online scorer with the transform in front of the splice: pk_mi355_transform_batch_create's
 * arguments, checks (in its order, with its texts, through the same code) and meaning of Db, deltas (may be NULL),
 * frontend (NULL: features only, capacity in frames pushed between two steps; else capacity in 16 kHz samples and
 * global_stats required), global_stats and stats_len.  An f16 model is refused besides, as on every stream entry; the
 * null arguments and the two specs are checked before the model is looked at.  Everything in front of the transform
 * works at Db, as on a transform batch: the front-end, the statistics, every normalisation the online scorer accepts,
 * their records, pk_mi355_stream_norm_fetch_stats and PK_MI355_FEATS_RAW slots, whose pushes are [n][Db].
 * PK_MI355_FEATS_NORMALIZED slots stay [n][feat_dim] and pass no stage.  The matrix is copied.
 *
 * The rule for a live slot.  Lt, Rt the spec's contexts, C = Lt + Rt; R the model's right context; M = order * window
 * with deltas, 0 without.  Per slot: nin, the transform's input frames final so far (the normalised base frames n
 * without deltas, the nd' of the deltas rule above with them); nx, transform frames final so far; a, rows scored so far.
 * One step:
 *   - transform frames [nx, nx') become final, nx' = closed ? nin : max(nx, nin - Rt);
 *   - transform frame t is the apply rule of pk_mi355_transform_spec_t over the input frames clamp(t + j, 0, nin - 1),
 *     j = -Lt .. Rt (while the slot is open t + Rt <= nin - 1, so the upper clamp binds only after close; the lower
 *     clamp is frame 0 of this opening);
 *   - the slot's own matrix (pk_mi355_stream_transform_set_slot), if it has one, is applied to the newly final frames
 *     [nx, nx') with L = R = 0; a slot without one passes its rows on as bits (a copy, not an identity product: -0.0,
 *     NaN payloads and inf survive, as on a batch call without matrices);
 *   - rows [a, b) are scored, b = closed ? nx' : max(a, nx' - R), spliced over transform frames as on every stream.
 * The look-ahead of a live slot is therefore M + Rt + R frames; a slot closed with n = 0 gives nothing, one closed with
 * n <= M + Rt + R gives all its rows at the flush, one closed a step after its last push flushes from its history alone.
 * Over a slot's life the rows are those of a batch made by pk_mi355_transform_batch_create on the whole input under the
 * same normalisation, deltas and matrices, bit for bit, at every chunking and in both softmax modes.
 * Memory beyond a stream without a transform: 8 * max(C, 1) * in_dim bytes of ring per slot, a staging of
 * (max_frames + max_streams * (M + Rt)) * feat_dim floats (a second one, as large, from the first
 * pk_mi355_stream_transform_set_slot on, with (feat_dim + 1) * RoundUp(feat_dim, 64) floats of matrix per slot), the
 * matrix, Rt more rows per slot in the layer buffers, and two more record arrays of 96 * max_streams bytes.  A step that
 * cannot fit fails with PK_MI355_E_INVALID and consumes nothing.                                                     */
pk_mi355_stream_t *pk_mi355_transform_stream_create(pk_mi355_am_t *am, const pk_mi355_transform_spec_t *transform,
                                                    const pk_mi355_deltas_spec_t *deltas, const pk_mi355_frontend_spec_t *frontend,
                                                    const float *global_stats, int stats_len, int max_streams, int64_t capacity);
/* in_dim of a stream made by the entry above; feat_dim on every other stream; PK_MI355_E_INVALID for NULL.          */
int pk_mi355_stream_in_dim(const pk_mi355_stream_t *s);
/* The slot's own matrix (fMLLR for the speaker on that slot): row-major [rows][cols], rows = feat_dim, cols = feat_dim
 * (linear) or feat_dim + 1 (affine), every entry finite, else PK_MI355_E_INVALID (naming row and column); feat_dim
 * above 1024 is PK_MI355_E_INVALID too.  For an open audio or RAW slot before its first transform frame is computed;
 * otherwise, on a NORMALIZED slot, or on a stream of another entry: PK_MI355_E_STATE.  The matrix is copied and lasts
 * until the slot is opened again.  Optional: a slot without one skips the stage.                                     */
int pk_mi355_stream_transform_set_slot(pk_mi355_stream_t *s, int slot, const float *matrix, int rows, int cols);

/* ---- The normalisation of an online scorer of any kind (pk_mi355_stream_create, pk_mi355_features_stream_create*,
 * pk_mi355_frontend_stream_create): every row a slot's life produces is the row the batch scorer produces under the
 * same spec on the whole input, bit for bit, whatever the chunks.  Both set entries: only while no slot is in use (open,
 * or closed and not yet flushed), else PK_MI355_E_STATE, and the object keeps the norm it had.  With anything but
 * SLIDING the audio and RAW slots' fresh rows go through StreamNormKernel (NONE: nothing) and
 * StreamFeatureLayoutKernel at every dimension, 40 included, and an object made without statistics takes
 * PK_MI355_FEATS_RAW slots; with SLIDING (never set, or set again) it launches what it always launched.
 * pk_mi355_stream_norm_set: SLIDING, NONE or SPEAKER; UTTERANCE is PK_MI355_E_INVALID (an utterance's statistics do
 * not exist while it is live); the other refusals are pk_mi355_norm_check's.
 * pk_mi355_stream_norm_set_online_cmvn: as pk_mi355_norm_set_online_cmvn.
 * Device memory, made by the first call that needs it, S slots at dimension D: 16 D S bytes of whole-slot sums;
 * SPEAKER 8 D S bytes of tables; online CMVN 16 D S bytes of window sums, 16 (D + 1) (S + 1) bytes of records and
 * 4 cmn_window D S bytes of raw rows; and the layout history 8 max(L + R, 1) D S bytes where it does not exist yet. */
int pk_mi355_stream_norm_set(pk_mi355_stream_t *s, const pk_mi355_norm_spec_t *spec);
int pk_mi355_stream_norm_set_online_cmvn(pk_mi355_stream_t *s, const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats);
/* The speaker's 2 x (feat_dim + 1) record of an open slot, handed over before the slot's first frame is computed (else,
 * or for a slot of NORMALIZED features, or under SLIDING or NONE: PK_MI355_E_STATE); it lasts until the slot is opened
 * again.  SPEAKER: required -- pk_mi355_stream_step with an audio or RAW slot in use that has none fails with
 * PK_MI355_E_STATE, names the slot and consumes nothing; a count that is not positive and finite is PK_MI355_E_INVALID.
 * Online CMVN: optional; a count of 0 is no prior, one that is negative or not finite PK_MI355_E_INVALID.           */
int pk_mi355_stream_norm_set_speaker_stats(pk_mi355_stream_t *s, int slot, const double *stats);
/* SPEAKER and online CMVN: the 2 x (feat_dim + 1) record of all frames of the slot computed since it was opened (it
 * stays readable after the slot's flush, until the slot is opened again), accumulated in the UTTERANCE rule's order:
 * the bits pk_mi355_norm_fetch_stats gives for the whole input, so a caller can add it to the speaker's record for the
 * next utterance.  PK_MI355_E_STATE under SLIDING or NONE and for a slot of NORMALIZED features.  Synchronises.      */
int pk_mi355_stream_norm_fetch_stats(pk_mi355_stream_t *s, int slot, double *out);
/* What the slot was last opened as: -1 for audio (also before its first opening), else its PK_MI355_FEATS_* kind.  A
 * null object or a slot out of range gives PK_MI355_E_INVALID, which is -1 as well, and sets pk_mi355_last_error.     */
int pk_mi355_stream_slot_kind(const pk_mi355_stream_t *s, int slot);

/* ------------------------------------------------------------------------- */
/* Online decoder -- Decoder::Decode (decoder.cc:49-70) frame-synchronous across calls: */
/* partial hypotheses while a stream is live, BestPath (decoder.cc:304-339) at its end. */
/* ------------------------------------------------------------------------- */

/* Semantics are the batch decoder's (N1, N2, exact max-active, the three documented
 * differences): a slot fed its frames in chunks of any size ends with the words, weight bits, ok, best-path arcs
 * and active_bound of pk_mi355_decoder_decode on the whole utterance.  Each slot has a backtrace arena of
 * trace_capacity records (8 bytes each; 0 = 2^20); when one is more than half full between two frames its
 * reachable records are compacted, and a slot still full ends with PK_MI355_E_CAPACITY
 * while the other slots go on.  Device memory: the batch decoder's with max_utts = max_streams and
 * max_streams x trace_capacity records, plus 4 bytes per record.  One host thread at a time.             */
typedef struct pk_mi355_online_decoder pk_mi355_online_decoder_t;
pk_mi355_online_decoder_t *pk_mi355_online_decoder_create(const pk_mi355_fst_t *fst, const pk_mi355_am_t *am, int max_streams,
                                                          int64_t trace_capacity);
void pk_mi355_online_decoder_destroy(pk_mi355_online_decoder_t *d);
/* Decoder::beam_ and kBeamSize, as pk_mi355_decoder_set_beam (takes effect at the next advance).             */
int pk_mi355_online_decoder_set_beam(pk_mi355_online_decoder_t *d, float beam, int max_active);
/* Start an utterance in slot (InitDecoding runs with its first frames).  PK_MI355_E_STATE if it is open.    */
int pk_mi355_online_decoder_open(pk_mi355_online_decoder_t *d, int slot);
/* The rows the online scorer's last pk_mi355_stream_step scored, slot for slot (decoder slot i takes scorer slot
 * i; the scorer needs no more slots than the decoder), read in HBM and queued on the scorer's stream after its
 * step.  A slot the step flushed (it was closed) is finished: BestPath runs.  Only open decoder slots take part.
 * Call it after every step and before the next one.                                                         */
int pk_mi355_online_decoder_advance(pk_mi355_online_decoder_t *d, pk_mi355_stream_t *s, int sync);
/* Host chunks: chunks[i] ({ncol = frames, nrow = num_pdfs}, ncol may be 0) continues open slot slots[i];
 * final_[i] != 0 (final_ may be NULL) finishes the slot after them.  Copied before the call returns.         */
int pk_mi355_online_decoder_advance_host(pk_mi355_online_decoder_t *d, const int *slots, const pk_decodable_t *chunks,
                                         const int *final_, int n, int sync);
/* Waits for the last advance.  PK_MI355_E_CAPACITY / PK_MI355_E_INVALID name the first slot of that call that
 * ended so (the others' results stay readable).                                                              */
int pk_mi355_online_decoder_synchronize(pk_mi355_online_decoder_t *d);
/* The partial hypothesis after the slot's last advance: the path of the best token (lowest cost, lowest state on
 * a tie, no final weight), its words in spoken order (at most max_words written) and its cost; the word count is
 * returned.  After the slot's final advance this is the final result.                                        */
int pk_mi355_online_decoder_partial(const pk_mi355_online_decoder_t *d, int slot, int *words, int max_words, float *cost);
/* A finished slot: as pk_mi355_decoder_result.  PK_MI355_E_STATE before the slot's final advance.             */
int pk_mi355_online_decoder_result(const pk_mi355_online_decoder_t *d, int slot, int *words, int max_words, float *weight,
                                   int *ok);
/* Test hooks, as pk_mi355_decoder_best_path_arcs / _active_bound (the arcs of the partial path while live).  */
int pk_mi355_online_decoder_best_path_arcs(const pk_mi355_online_decoder_t *d, int slot, int32_t *arcs, int max_arcs);
int pk_mi355_online_decoder_active_bound(const pk_mi355_online_decoder_t *d, int slot);
/* The frames the slot has decoded so far (0 after open; what a slot that ended early had decoded).            */
int pk_mi355_online_decoder_num_frames(const pk_mi355_online_decoder_t *d, int slot);

/* ------------------------------------------------------------------------- */
/* Best-path alignment and word segments ("Alignment")       */
/* ------------------------------------------------------------------------- */

/* Off (0) by default; like set_trace_gc it takes effect at the next decode / decode_batch.  On: one more launch
 * follows the decode on the same stream and, for every utterance with ok = 1 and a best path, writes per FRAME t
 * the original arc id of the t-th emitting arc of the path (ilabel != 0) and its acoustic cost
 * -N1(log_prob[t][pdf of that arc]) (N1: a NaN log-likelihood counts as -inf, so the cost is +inf), reading the
 * log-likelihoods where they lie in HBM.  Words, weight, ok and best-path arcs are those of the mode off, bit for
 * bit.  Device memory the mode adds: 4 bytes x arcs of the graph (allocated and uploaded at the first enable, not
 * at create) + 8 bytes x frames of the largest call + 16 bytes x max_utts.                                        */
int pk_mi355_decoder_set_alignment(pk_mi355_decoder_t *d, int enable);
/* The alignment of utt in the last call: per frame the arc id, its transition-id (the arc's ilabel) and its
 * acoustic cost (any pointer may be NULL; at most max_frames entries written).  Returns the frames aligned: the
 * utterance's frame count, or 0 for an utterance that ended with ok = 0 or has no best path.  PK_MI355_E_STATE
 * when the call ran with alignment off.                                                                          */
int pk_mi355_decoder_alignment(const pk_mi355_decoder_t *d, int utt, int32_t *arc_ids, int32_t *trans_ids,
                               float *acoustic_cost, int max_frames);
/* One segment of the best path per word.  A segment begins at every arc whose olabel is not 0 (epsilon arcs
 * included) and runs up to the next such arc, exclusive; the arcs before the first one form a leading segment with
 * word = 0 (a path without any olabel is one such segment, an empty path gives none).  start_frame: emitting arcs
 * of the path before the segment's first arc; num_frames: emitting arcs inside it (may be 0); graph_cost: (float)
 * of the sum in double, in path order, of the segment's arc weights; acoustic_cost: the same over its frames'
 * acoustic costs.  The final weight belongs to no segment.                                                       */
typedef struct pk_mi355_word_t {
  int32_t word;
  int32_t start_frame;
  int32_t num_frames;
  float graph_cost;
  float acoustic_cost;
} pk_mi355_word_t;
/* Segments of utt in the last call (at most max written, the count returned).  PK_MI355_E_STATE when the call ran
 * with alignment off.                                                                                            */
int pk_mi355_decoder_word_segments(const pk_mi355_decoder_t *d, int utt, pk_mi355_word_t *out, int max);
/* Online alignment.  Off (0) by default; the mode is the object's (one launch serves every slot), so it can be
 * changed only while no slot is open: PK_MI355_E_STATE otherwise.  On: every backtrace record also keeps the
 * acoustic cost of its arc -- -N1(log_prob[t][pdf]) for an emitting arc, the bits the batch decoder's alignment
 * gives, 0 for an epsilon arc -- written when the frame is decoded (the only moment its row exists), moved by the
 * trace compaction and read out with the path.  Words, weight, ok, best-path arcs and active_bound are those of the
 * mode off, bit for bit.  Device memory the mode adds: 8 bytes x max_streams x trace_capacity, allocated at the
 * first enable, not at create.  A finished slot keeps the mode it was opened with.  A call still in flight is waited
 * for first; what it says of a slot (PK_MI355_E_CAPACITY, ...) is not this entry's failure and stays readable in the
 * slot's result.                                                                                                   */
int pk_mi355_online_decoder_set_alignment(pk_mi355_online_decoder_t *d, int enable);
/* The alignment of the slot's current path -- partial while the slot is live, final after its last advance -- as
 * pk_mi355_decoder_alignment: per frame the arc id, its transition-id and its acoustic cost (any pointer may be
 * NULL; at most max_frames entries written).  Returns the frames aligned: pk_mi355_online_decoder_num_frames, or 0
 * for a slot without a path or one that ended with ok = 0.  PK_MI355_E_STATE with the mode off (or for a slot opened
 * with it off); PK_MI355_E_DEVICE if the path's emitting arcs are not the slot's decoded frames.                  */
int pk_mi355_online_decoder_alignment(const pk_mi355_online_decoder_t *d, int slot, int32_t *arc_ids, int32_t *trans_ids,
                                      float *acoustic_cost, int max_frames);
/* Segments of the slot's current path: the partial hypothesis while the slot is live, the final one after its
 * last advance.  With alignment off acoustic_cost is NaN in every segment: the online scorer's rows are void after
 * each step, so no log-likelihood of the path's frames is left to read.  With alignment on it is the sum over the
 * costs kept with the trace, as pk_mi355_decoder_word_segments gives it.                                         */
int pk_mi355_online_decoder_word_segments(const pk_mi355_online_decoder_t *d, int slot, pk_mi355_word_t *out, int max);

/* ------------------------------------------------------------------------- */
/* Online commit mode ("Commit"): streams of any length     */
/* ------------------------------------------------------------------------- */

/* Off (0) by default; like online alignment the mode is the object's and can be changed only while no slot is open
 * (PK_MI355_E_STATE otherwise); a finished slot keeps the mode it was opened with.  On: at the end of every launch
 * that does not finish the slot, the arcs that the backtraces of ALL the slot's tokens share -- which no later audio
 * can change -- are handed to the host, but for the last of them, and leave the slot's arena; that last shared record
 * stays as the arena's root.  The arena, the end-of-launch path walk and the copy to the host are then bounded by the
 * undecided tail, not by the time since open: a stream may be longer than trace_capacity, while a single launch must
 * still fit it.  Nothing is committed while a token still sits at the start or two first arcs are alive, and nothing
 * for a slot that ended (status, ok = 0): such a slot reports no path, whatever it committed earlier, as does a slot
 * that finishes without a token in a final state (BestPath's empty hypothesis).  Every getter
 * sees committed ++ tail: words, costs, weight bits, arcs, alignment, segments and active_bound are those of the mode
 * off, bit for bit.  No device memory is added; host memory grows by 4 bytes per committed arc, 8 with alignment,
 * until the slot is opened again.                                                                                    */
int pk_mi355_online_decoder_set_commit(pk_mi355_online_decoder_t *d, int enable);
/* The committed prefix of the slot's path after its last advance: its words in spoken order (olabel != 0; at most
 * max_words written, the count returned), the number of committed arcs and of emitting arcs among them (either
 * pointer may be NULL).  It only ever grows while the slot is live, and every later path of the slot starts with it.
 * 0 / 0 / 0 with the mode off, and for a slot that ended.                                                            */
int pk_mi355_online_decoder_committed(const pk_mi355_online_decoder_t *d, int slot, int *words, int max_words, int *num_arcs,
                                      int *num_frames);
/* The slot's backtrace arena (any pointer may be NULL): records in it after the slot's last launch; the most it
 * held since open; its capacity in records (trace_capacity).  With the commit mode on the peak is sampled before
 * every compaction and commit and at the end of each launch, as pk_mi355_decoder_trace_stats does; with the mode off
 * the kernel is the one that knows no such mode and keeps no maximum, so the peak is sampled at the end of each
 * launch only.  PK_MI355_E_STATE before the slot's first launch.                                                     */
int pk_mi355_online_decoder_trace_stats(const pk_mi355_online_decoder_t *d, int slot, int64_t *in_use, int64_t *peak,
                                        int64_t *capacity);

/* ------------------------------------------------------------------------- */
/* Online endpointing ("Endpointing"): when has the speaker stopped */
/* ------------------------------------------------------------------------- */

/* One rule, in frames (10 ms each).  With contains_nonsilence = frames > trailing_silence_frames it fires when
 *   (contains_nonsilence || !must_contain_nonsilence) && trailing_silence_frames >= min_trailing_silence_frames &&
 *   relative_cost <= max_relative_cost && frames >= min_utterance_frames,
 * and never at frames == 0.  Every test is on integers but the one float comparison.                               */
typedef struct pk_mi355_endpoint_rule_t {
  int must_contain_nonsilence;
  int min_trailing_silence_frames;
  float max_relative_cost;           /* +inf: the final-state cost is not asked                                     */
  int min_utterance_frames;
} pk_mi355_endpoint_rule_t;
/* What the rules are tried on, for one slot after its last advance.  frames: decoded since open.
 * trailing_silence_frames: the emitting arcs of the best partial path (lowest cost, lowest state on a tie) after its
 * last arc that emits a pdf outside the silence set -- all of them if it has none.  best_cost: the lowest token cost
 * (the partial's cost).  final_cost: the lowest (double)cost + (double)final weight over the num_final tokens for
 * which that is not INFINITY, as float; relative_cost: the difference of the two, taken in double, as float.  Both
 * +inf with num_final == 0.  rule: 1 + the first rule that fires, 0 for none.  valid == 0 (and all else 0): the slot
 * has not advanced, finished, ended (status, ok = 0) or holds no token.                                             */
typedef struct pk_mi355_endpoint_t {
  int valid, frames, trailing_silence_frames, num_final, rule;
  float best_cost, final_cost, relative_cost;
} pk_mi355_endpoint_t;
/* The five usual rules at a 10 ms frame shift, (must_contain_nonsilence, min_trailing_silence_frames,
 * max_relative_cost, min_utterance_frames): (0, 500, inf, 0), (1, 50, 2.0, 0), (1, 100, 8.0, 0), (1, 200, inf, 0),
 * (0, 0, inf, 2000).  Writes at most max of them (rules may be NULL); returns 5.  Host only, needs no GPU.           */
int pk_mi355_endpoint_default_rules(pk_mi355_endpoint_rule_t *rules, int max);
/* 1 + the index of the first rule that fires, 0 if none does (also for num_rules <= 0).  Host only, needs no GPU.    */
int pk_mi355_endpoint_eval(const pk_mi355_endpoint_rule_t *rules, int num_rules, int frames, int trailing_silence_frames,
                           float relative_cost);
/* Off by default; num_rules == 0 turns it off.  Like alignment and commit the mode is the object's: set while no
 * slot is open (PK_MI355_E_STATE otherwise), a call in flight is waited for first.  silence_pdfs: the pdfs (after the
 * model's transition-id map) that count as silence; may be empty.  PK_MI355_E_INVALID for a pdf outside
 * [0, num_pdfs), a negative frame count or a NaN max_relative_cost -- checked before anything else.  On: after every
 * launch a second kernel leaves one record per slot of the call, fetched with the results; the decode kernels and
 * every result are those of the mode off.  Device memory: 4 bytes per arc, num_pdfs / 8 bytes and 40 bytes per slot,
 * from the first enable.                                                                                            */
int pk_mi355_online_decoder_set_endpointing(pk_mi355_online_decoder_t *d, const int32_t *silence_pdfs, int num_silence,
                                            const pk_mi355_endpoint_rule_t *rules, int num_rules);
/* The slot's record after its last advance (out may be NULL); returns its rule.  PK_MI355_E_STATE with the mode off. */
int pk_mi355_online_decoder_endpoint(const pk_mi355_online_decoder_t *d, int slot, pk_mi355_endpoint_t *out);
/* Ends each listed open slot now, with no new frame: the slot's closing launch (BestPath with final weights over the
 * frames decoded so far) on the decoder's own stream, after a pending advance.  result, word_segments and alignment
 * are then those of pk_mi355_decoder_decode on the rows the slot has seen, bit for bit, and the slot can be opened
 * again at once.  A slot that was never advanced gives the empty utterance's result.  An utterance ended while no
 * token is final has no words (BestPath's empty hypothesis), as in the reference.  PK_MI355_E_STATE for a slot that
 * is not open.  Needs no endpointing mode.                                                                          */
int pk_mi355_online_decoder_finish(pk_mi355_online_decoder_t *d, const int *slots, int n, int sync);

/* ------------------------------------------------------------------------- */
/* Symbol table -- pk_symboltable_read / _get (symbol_table.cc:23-79)              */
/* ------------------------------------------------------------------------- */

/* "SYM0", i32 section size, i32 size, i32 buffer_size, size x i32 offsets, buffer_size bytes of NUL-terminated
 * strings.  Host only, needs no GPU.  NULL on failure: PK_MI355_E_IO for a malformed or truncated file (tag,
 * section size != 8 + 4 size + buffer_size, negative counts, fewer bytes than stated, a non-empty buffer that does
 * not end in NUL), PK_MI355_E_INVALID for an offset outside [0, buffer_size).                                     */
typedef struct pk_mi355_symtab pk_mi355_symtab_t;
pk_mi355_symtab_t *pk_mi355_symtab_read(const char *path);
void pk_mi355_symtab_destroy(pk_mi355_symtab_t *st);
int pk_mi355_symtab_size(const pk_mi355_symtab_t *st);
/* The string of symbol id; NULL (PK_MI355_E_INVALID) outside [0, size) -- the reference asserts there.  The pointer
 * is valid until the table is destroyed.                                                                         */
const char *pk_mi355_symtab_get(const pk_mi355_symtab_t *st, int id);

/* ------------------------------------------------------------------------- */
/* Recognizer -- pk_load + pk_process (pocketkaldi.cc:72-248): model file and waves to text */
/* ------------------------------------------------------------------------- */

/* pk_load: reads the model file's fst, cmvn_stats, AcousticModel keys (through pk_mi355_load) and symbol_table,
 * and owns a batch scorer (max_utts, max_total_samples: as pk_mi355_batch_create) and a decoder with alignment on
 * (trace_capacity: as pk_mi355_decoder_create).  A missing key is reported in the reference's words ("Unable to
 * find key 'fst' in ..."); every olabel of the graph must be < the symbol table's size, else PK_MI355_E_INVALID
 * (the reference asserts this at lookup).  The keys and the host-side files are checked before the device is
 * touched.  NULL on failure.                                                                                     */
typedef struct pk_mi355_recognizer pk_mi355_recognizer_t;
pk_mi355_recognizer_t *pk_mi355_recognizer_load(const char *config_path, int precision, int max_utts,
                                                int64_t max_total_samples, int64_t trace_capacity);
/* The same for a model of pk_mi355_frontend_dim(spec) features: pk_mi355_load_stats and
 * pk_mi355_frontend_batch_create in place of pk_mi355_load and pk_mi355_batch_create, whose refusals are this
 * entry's; a bad spec is refused first.  Every other entry works unchanged; process_features takes [T][dim].    */
pk_mi355_recognizer_t *pk_mi355_frontend_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *spec,
                                                         int precision, int max_utts, int64_t max_total_samples,
                                                         int64_t trace_capacity);
/* The same with deltas for a model of (order + 1) * pk_mi355_frontend_dim(frontend_spec)
 * features: the model file's cmvn_stats holds pk_mi355_frontend_dim + 1 entries, and the batch is
 * pk_mi355_deltas_batch_create's, whose refusals are this entry's; bad specs are refused first.  process_features with
 * PK_MI355_FEATS_RAW takes [T][pk_mi355_frontend_dim], with PK_MI355_FEATS_NORMALIZED [T][feat_dim].               */
pk_mi355_recognizer_t *pk_mi355_deltas_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *frontend_spec,
                                                       const pk_mi355_deltas_spec_t *deltas_spec, int precision, int max_utts,
                                                       int64_t max_total_samples, int64_t trace_capacity);
/* The same with a transform, behind deltas when deltas_spec is not NULL, for a model whose
 * features are the transform's output: the model file's cmvn_stats holds pk_mi355_frontend_dim + 1 entries, and the
 * batch is pk_mi355_transform_batch_create's, whose refusals are this entry's; bad specs are refused first.
 * Per-utterance matrices for a process call: pk_mi355_transform_set_utt on pk_mi355_recognizer_batch before it, as
 * speaker records are handed over.  process_features with PK_MI355_FEATS_RAW takes [T][pk_mi355_frontend_dim].      */
pk_mi355_recognizer_t *pk_mi355_transform_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *frontend_spec,
                                                          const pk_mi355_deltas_spec_t *deltas_spec,
                                                          const pk_mi355_transform_spec_t *transform_spec, int precision, int max_utts,
                                                          int64_t max_total_samples, int64_t trace_capacity);
void pk_mi355_recognizer_destroy(pk_mi355_recognizer_t *r);
/* The owned objects: beam, trace gc, softmax mode, f16 calibration and every result getter (words, weight, ok,
 * alignment, word segments) are their existing entries.                                                          */
pk_mi355_am_t *pk_mi355_recognizer_am(pk_mi355_recognizer_t *r);
pk_mi355_batch_t *pk_mi355_recognizer_batch(pk_mi355_recognizer_t *r);
pk_mi355_decoder_t *pk_mi355_recognizer_decoder(pk_mi355_recognizer_t *r);
const pk_mi355_symtab_t *pk_mi355_recognizer_symtab(const pk_mi355_recognizer_t *r);
/* pk_process for n waves at once: set_waves, score (prob_scale 0.1), decode_batch, synchronize.                   */
int pk_mi355_recognizer_process(pk_mi355_recognizer_t *r, const pk_vector_t *waves, int n);
/* Same, wave u sampled at rates[u] Hz (pk_mi355_resample_set_waves; rates == NULL: 16000 throughout).  Capacity and
 * every result -- frames, word times -- are those of the converted 16 kHz audio.                                  */
int pk_mi355_recognizer_process_rates(pk_mi355_recognizer_t *r, const pk_vector_t *waves, const int *rates, int n);
/* Same from features (pk_mi355_features_set on the recognizer's batch: its failures are this entry's); the
 * results are read as after pk_mi355_recognizer_process.                                                        */
int pk_mi355_recognizer_process_features(pk_mi355_recognizer_t *r, const pk_matrix_t *feats, int n, int kind);
/* utt->hyp of the last process: the words' strings in spoken order joined by one space, no trailing space; "" for
 * an utterance without words (also one the decoder ended with ok = 0).  Valid until the next process.  NULL on
 * misuse.                                                                                                        */
const char *pk_mi355_recognizer_hyp(const pk_mi355_recognizer_t *r, int utt);
/* utt->loglikelihood_per_frame: weight / num_frames in float; 0.0f for an utterance without words (NaN on misuse). */
float pk_mi355_recognizer_loglikelihood_per_frame(const pk_mi355_recognizer_t *r, int utt);

/* ------------------------------------------------------------------------- */
/* Online recognizer -- pk_load + a live pk_process: PCM chunks to text             */
/* ------------------------------------------------------------------------- */

/* pk_load as pk_mi355_recognizer_load does it (same keys, order, messages and olabel check; host-side files before
 * the device is touched), F32 only (the online scorer refuses f16 models).  Owns graph, symbol table, model, an
 * online scorer (max_streams, max_step_samples: as pk_mi355_stream_create) and an online decoder with alignment on
 * (trace_capacity: as pk_mi355_online_decoder_create).  It computes nothing itself: beam, softmax mode and every
 * result getter (words, weight, ok, alignment, word segments) are the owned objects' entries.  NULL on failure.   */
typedef struct pk_mi355_online_recognizer pk_mi355_online_recognizer_t;
pk_mi355_online_recognizer_t *pk_mi355_online_recognizer_load(const char *config_path, int max_streams,
                                                              int64_t max_step_samples, int64_t trace_capacity);
/* The same for a model of pk_mi355_frontend_dim(spec) features: pk_mi355_load_stats and
 * pk_mi355_frontend_stream_create in place of pk_mi355_load and pk_mi355_stream_create, whose refusals are this
 * entry's; a bad spec is refused first.  Every other entry works unchanged; push_features takes [n][dim].       */
pk_mi355_online_recognizer_t *pk_mi355_frontend_online_recognizer_load(const char *config_path,
                                                                       const pk_mi355_frontend_spec_t *spec, int max_streams,
                                                                       int64_t max_step_samples, int64_t trace_capacity);
/* The same with deltas for a model of (order + 1) * pk_mi355_frontend_dim(frontend_spec)
 * features whose cmvn_stats hold the front-end's dimension + 1 entries: pk_mi355_deltas_stream_create in place of
 * pk_mi355_frontend_stream_create, whose refusals are this entry's; bad specs are refused first.  push_features of a
 * RAW slot takes [n][Db].                                                                                           */
pk_mi355_online_recognizer_t *pk_mi355_deltas_online_recognizer_load(const char *config_path,
                                                                     const pk_mi355_frontend_spec_t *frontend_spec,
                                                                     const pk_mi355_deltas_spec_t *deltas_spec, int max_streams,
                                                                     int64_t max_step_samples, int64_t trace_capacity);
/* The same with a transform, behind deltas when deltas_spec is not NULL, for a model whose
 * features are the transform's output and whose cmvn_stats hold the front-end's dimension + 1 entries:
 * pk_mi355_transform_stream_create in place of pk_mi355_frontend_stream_create, whose refusals are this entry's; bad
 * specs are refused first.  A slot's own matrix: pk_mi355_stream_transform_set_slot on
 * pk_mi355_online_recognizer_stream once the slot is open.  With endpointing a matrix belongs to the opening: every
 * utterance cut from that opening uses it.  push_features of a RAW slot takes [n][Db].                             */
pk_mi355_online_recognizer_t *pk_mi355_transform_online_recognizer_load(const char *config_path,
                                                                        const pk_mi355_frontend_spec_t *frontend_spec,
                                                                        const pk_mi355_deltas_spec_t *deltas_spec,
                                                                        const pk_mi355_transform_spec_t *transform_spec,
                                                                        int max_streams, int64_t max_step_samples,
                                                                        int64_t trace_capacity);
void pk_mi355_online_recognizer_destroy(pk_mi355_online_recognizer_t *r);
pk_mi355_am_t *pk_mi355_online_recognizer_am(pk_mi355_online_recognizer_t *r);
pk_mi355_stream_t *pk_mi355_online_recognizer_stream(pk_mi355_online_recognizer_t *r);
pk_mi355_online_decoder_t *pk_mi355_online_recognizer_decoder(pk_mi355_online_recognizer_t *r);
const pk_mi355_symtab_t *pk_mi355_online_recognizer_symtab(const pk_mi355_online_recognizer_t *r);
/* Start an utterance in slot: opens the scorer's slot and the decoder's (neither, if either refuses).  Open, push,
 * close and step through these entries, not through the owned objects: a slot closed behind the recognizer's back
 * is never reported finished.                                                                                      */
int pk_mi355_online_recognizer_open(pk_mi355_online_recognizer_t *r, int slot);
/* The same for audio sampled at `rate` Hz: pk_mi355_stream_open_rate for the scorer's slot.                         */
int pk_mi355_online_recognizer_open_rate(pk_mi355_online_recognizer_t *r, int slot, int rate);
/* As pk_mi355_stream_push / _push_i16 / _close.                                                                    */
int pk_mi355_online_recognizer_push(pk_mi355_online_recognizer_t *r, int slot, const float *samples, int num_samples);
int pk_mi355_online_recognizer_push_i16(pk_mi355_online_recognizer_t *r, int slot, const int16_t *samples, int num_samples);
int pk_mi355_online_recognizer_close(pk_mi355_online_recognizer_t *r, int slot);
/* The slot fed with features instead of audio: pk_mi355_stream_open_features / _push_features for the scorer's slot (the
 * recognizer's model is 40-dim; RAW is what a front-end of the caller's would produce).  Everything after the scorer --
 * step, partial, stable, result, utterances, endpointing, commit -- is the same.                                     */
int pk_mi355_online_recognizer_open_features(pk_mi355_online_recognizer_t *r, int slot, int kind);
int pk_mi355_online_recognizer_push_features(pk_mi355_online_recognizer_t *r, int slot, const float *frames, int num_frames);
/* pk_mi355_stream_step (prob_scale 0.1), pk_mi355_online_decoder_advance (synchronous), then the text of every slot
 * is refreshed.  Returns what those return: a slot the decoder ended (PK_MI355_E_CAPACITY, ...) stays ended until
 * it is closed, flushed by a step and opened again, while the other slots go on.                                  */
int pk_mi355_online_recognizer_step(pk_mi355_online_recognizer_t *r);
/* The slot's current hypothesis: the words' strings in spoken order joined by one space ("" without words).  Valid
 * until the next step.  NULL on misuse.                                                                            */
const char *pk_mi355_online_recognizer_partial(const pk_mi355_online_recognizer_t *r, int slot);
/* The words of the hypothesis that are final now: the decoder's committed prefix (pk_mi355_online_decoder_committed)
 * joined as the partial is; the partial always starts with it.  "" while the owned decoder's commit mode is off
 * (pk_mi355_online_decoder_set_commit on pk_mi355_online_recognizer_decoder).  Valid until the next step.           */
const char *pk_mi355_online_recognizer_stable(const pk_mi355_online_recognizer_t *r, int slot);
/* 1 once the step after the slot's close has run (its result is final), 0 before; negative on misuse.             */
int pk_mi355_online_recognizer_finished(const pk_mi355_online_recognizer_t *r, int slot);
/* A finished slot's utt->hyp and utt->loglikelihood_per_frame, by pk_mi355_recognizer_hyp's rules: "" and 0.0f for a
 * slot without words (also one the decoder ended with ok = 0), else weight / frames in float.  Before the slot is
 * finished: NULL / NaN with PK_MI355_E_STATE.  Valid until the slot is opened again.                               */
const char *pk_mi355_online_recognizer_hyp(const pk_mi355_online_recognizer_t *r, int slot);
float pk_mi355_online_recognizer_loglikelihood_per_frame(const pk_mi355_online_recognizer_t *r, int slot);

/* Endpointing: pk_mi355_online_decoder_set_endpointing on the owned decoder, and the stream of every slot is cut into
 * utterances.  While no slot is open (PK_MI355_E_STATE otherwise); num_rules == 0 turns it off.  On: after a step's
 * advance every live slot that is not closing and whose endpoint rule fired is finished with the frames decoded so far
 * (pk_mi355_online_decoder_finish, one call for all of them), kept as an utterance, and its decoder slot is opened
 * again.  The scorer's slot stays open -- CMVN, context and resampler state run on -- so every later row is still the
 * batch scorer's row on the whole wave, and an utterance is pk_mi355_decoder_decode on the rows
 * [first_frame, first_frame + num_frames).  After close and the flushing step the rest is appended as the last
 * utterance, with rule 0; _hyp and _loglikelihood_per_frame are that last one's, _partial and _stable the current
 * one's.  The utterances are kept until the slot is opened again.  Off: no utterance is kept, and no entry changes.   */
int pk_mi355_online_recognizer_set_endpointing(pk_mi355_online_recognizer_t *r, const int32_t *silence_pdfs, int num_silence,
                                               const pk_mi355_endpoint_rule_t *rules, int num_rules);
typedef struct pk_mi355_utterance_t {
  int first_frame, num_frames;       /* of the slot's stream: first_frame is the sum of the earlier num_frames       */
  int rule;                          /* 1 + the rule that ended it; 0: the stream's end                               */
  int ok, num_words, num_word_segments;
  float weight;
  float loglikelihood_per_frame;     /* weight / num_frames; 0.0f without words, as is the text ""                    */
} pk_mi355_utterance_t;
int pk_mi355_online_recognizer_num_utterances(const pk_mi355_online_recognizer_t *r, int slot);
int pk_mi355_online_recognizer_utterance(const pk_mi355_online_recognizer_t *r, int slot, int i, pk_mi355_utterance_t *out);
/* Valid until the slot is opened again.  NULL on misuse.                                                            */
const char *pk_mi355_online_recognizer_utterance_hyp(const pk_mi355_online_recognizer_t *r, int slot, int i);
/* At most max written, the count returned.  Segment frames are relative to the utterance's first_frame.            */
int pk_mi355_online_recognizer_utterance_words(const pk_mi355_online_recognizer_t *r, int slot, int i, int *words, int max);
int pk_mi355_online_recognizer_utterance_word_segments(const pk_mi355_online_recognizer_t *r, int slot, int i,
                                                       pk_mi355_word_t *out, int max);

/* Library / device facts */
int pk_mi355_device_count(void);
const char *pk_mi355_version(void);

#ifdef __cplusplus
}
#endif
#endif  /* PK_MI355_H_ */

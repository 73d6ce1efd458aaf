// pk_create.h -- a scorer as it was asked for: the one request every public create entry of the
// batch and the online scorer fills, the part of its checks that needs no model, and the argument checks of the
// recognizers' load entries.  Plain C++: no HIP header, so it also builds into a stand-alone program that runs under
// the host sanitizers (tests/cpp/create_request_test.cc).  pkhost::CheckCreate (capi_batch.hip) goes on from here with
// the model.  Internal.
#ifndef PK_CREATE_H_
#define PK_CREATE_H_

#include <vector>

#include "pk_delta.h"
#include "pk_files.h"
#include "pk_frontend.h"
#include "pk_transform.h"

namespace pkhost {

// What a public create entry was handed.  units: utterances or slots.  stats41: 41 statistics by the entry's contract (a
// 40-dim model's; no stats_len).  audio: the capacity is in samples and there is a front-end -- the spec's, or without one
// the reference's 40 bins; else it is in frames.  null_arg: the entry found one of the pointers it needs null.  live: an
// online scorer's entry: an f16 model is refused besides, the model is looked at only behind the null arguments and the
// specs, and a null model is named "null model" (null_model_invalid; the four entries older than the deltas) or, as
// every batch entry names it, "model not finalized".  chunk_cap: rows per pass of a batch (0: the public entries').
struct CreateRequest {
  const float *stats; int stats_len; bool stats41; int units; int64_t capacity; bool audio, null_arg;
  const pk_mi355_frontend_spec_t *frontend; const pk_mi355_deltas_spec_t *deltas;
  const pk_mi355_transform_spec_t *xform = nullptr;
  bool live = false, null_model_invalid = false;
  int64_t chunk_cap = 0;
};
// What the checks worked out: the front-end spec's tables (null without one), the width of the rows a transform reads
// (the model's features without one) and the dimension in front of deltas and transform.
struct CreateDims {
  std::vector<pkmi::FrontendAnyTables> tables; int in_dim = 0, base_dim = 0;
  const pkmi::FrontendAnyTables *any() const { return tables.empty() ? nullptr : tables.data(); }
};

inline bool BuildRequestTables(const CreateRequest &r, CreateDims *dims) {       // (names the field)
  dims->tables.assign(r.frontend ? 1 : 0, pkmi::FrontendAnyTables());
  return !(r.frontend && pkmi::BuildFrontendAnyTables(r.frontend, dims->tables.data()));
}

// The checks in front of the model's, in the one order of DESIGN.md section 28.  model_usable: there is a model, and for
// a batch entry it is finalized (a live entry looks at its model behind these).  False: refused, the text is
// pk_mi355_last_error's.  A live entry's front-end tables are in *dims afterwards; a batch entry builds its own behind
// the dimension checks, where it has always named a bad front-end spec.
inline bool CheckRequestArgs(bool model_usable, const CreateRequest &r, CreateDims *dims) {
  if (!model_usable) {
    if (r.null_model_invalid) Fail(PK_MI355_E_INVALID, "null model"); else Fail(PK_MI355_E_STATE, "model not finalized");
    return false;
  }
  if (r.null_arg) { Fail(PK_MI355_E_INVALID, "null argument"); return false; }
  if (r.deltas && pkdelta::CheckSpec(r.deltas)) return false;         // (names the field)
  if (r.xform && pkxf::CheckSpec(r.xform)) return false;              // (names the field)
  return !r.live || BuildRequestTables(r, dims);
}

// The argument checks of the recognizers' eight load entries.  required: the specs the entry cannot do without (the path
// always is; an entry that takes no spec at all names it "null path").  Then the specs given, each in its own words, then
// the capacities, in capacity_text's.
enum { kNeedFrontend = 1, kNeedDeltas = 2, kNeedTransform = 4 };
inline bool CheckLoadArgs(const char *config_path, int required, const pk_mi355_frontend_spec_t *frontend, const pk_mi355_deltas_spec_t *deltas,
                          const pk_mi355_transform_spec_t *xform, int units, int64_t capacity, int64_t trace_capacity, const char *capacity_text) {
  if (!config_path || ((required & kNeedFrontend) && !frontend) || ((required & kNeedDeltas) && !deltas) || ((required & kNeedTransform) && !xform)) {
    Fail(PK_MI355_E_INVALID, required ? "null argument" : "null path");
    return false;
  }
  if ((frontend && pkmi::BuildFrontendAnyTables(frontend, nullptr)) || (deltas && pkdelta::CheckSpec(deltas)) || (xform && pkxf::CheckSpec(xform)))
    return false;                                         // (name the field)
  if (units <= 0 || capacity <= 0 || trace_capacity < 0) { Fail(PK_MI355_E_INVALID, "%s", capacity_text); return false; }
  return true;
}

}  // namespace pkhost

#endif  // PK_CREATE_H_

// create_request_test.cc -- the part of a scorer's creation that needs no device (csrc/pk_create.h; DESIGN.md section
// 28) in a process of its own: no HIP, no library, no Python.  The request, its checks in front of the model's
// (CheckRequestArgs: the model's presence, null arguments, the three specs) for a batch and a live entry, and the
// argument checks of the recognizers' load entries (CheckLoadArgs).  Built plain and with -fsanitize=address,undefined
// by tests/test_cpp_create_request.py, which holds the expected lines, written out there and not by calling this code.
//
//   create_request_test
//
// Prints one line per call: what was asked, then "ok" or the code and the text of the refusal.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_create.h"

using namespace pkhost;

static void Verdict(const char *what, bool ok) {
  if (ok) printf("%s: ok\n", what);
  else printf("%s: %d %s\n", what, pk_mi355_last_error_code(), pk_mi355_last_error());
}

int main() {
  const pk_mi355_frontend_spec_t fe{PK_MI355_FRONTEND_MFCC, 23, 13, PK_MI355_WINDOW_POVEY, 20.0f, 0.0f, 22.0f};
  pk_mi355_frontend_spec_t fe_bad = fe;
  fe_bad.num_mel_bins = 129;
  const pk_mi355_deltas_spec_t dl{2, 2}, dl_bad{4, 2};
  std::vector<float> m(40 * (7 * 13 + 1));
  for (size_t i = 0; i < m.size(); ++i) m[i] = 0.001f * (float)(i % 97) - 0.04f;
  const pk_mi355_transform_spec_t xf{3, 3, 13, 40, 7 * 13 + 1, m.data()};
  pk_mi355_transform_spec_t xf_bad = xf;
  xf_bad.left_context = 17;
  std::vector<float> holed = m;
  holed[2 * (7 * 13 + 1) + 5] = INFINITY;
  pk_mi355_transform_spec_t xf_holed = xf;
  xf_holed.matrix = holed.data();
  const float stats[14] = {0};

  // ---- CheckRequestArgs: a batch entry, then a live entry with each of the two texts for a missing model
  for (int live = 0; live < 2; ++live)
    for (int invalid = 0; invalid <= live; ++invalid) {
      char what[96];
      auto ask = [&](const char *name, bool model_usable, bool null_arg, const pk_mi355_frontend_spec_t *f, const pk_mi355_deltas_spec_t *d,
                     const pk_mi355_transform_spec_t *x) {
        CreateRequest r{stats, 14, false, 2, 1600, f != nullptr, null_arg, f, d, x, live != 0, invalid != 0};
        CreateDims dims;
        const bool ok = CheckRequestArgs(model_usable, r, &dims);
        snprintf(what, sizeof(what), "%s%s %s", live ? "live" : "batch", invalid ? " (null model)" : "", name);
        Verdict(what, ok);
        // a live entry that passed holds its front-end's tables; a batch entry builds its own later, with the model
        const bool want_tables = live && f;
        if (ok && ((dims.any() != nullptr) != want_tables || (want_tables && dims.any()->dim != 13) || dims.in_dim != 0 || dims.base_dim != 0)) {
          printf("create_request_test FAILED: %s: tables\n", what);
          return false;
        }
        return true;
      };
      if (!ask("no model", false, false, &fe, &dl, &xf) || !ask("no model, everything else bad too", false, true, &fe_bad, &dl_bad, &xf_bad) ||
          !ask("null argument", true, true, &fe, &dl, &xf) || !ask("null argument, bad specs", true, true, &fe_bad, &dl_bad, &xf_bad) ||
          !ask("bad deltas", true, false, &fe, &dl_bad, &xf) || !ask("bad deltas, transform, front-end", true, false, &fe_bad, &dl_bad, &xf_bad) ||
          !ask("bad transform", true, false, &fe, &dl, &xf_bad) || !ask("bad transform, front-end", true, false, &fe_bad, &dl, &xf_bad) ||
          !ask("transform not finite", true, false, &fe, nullptr, &xf_holed) || !ask("bad front-end", true, false, &fe_bad, &dl, &xf) ||
          !ask("bad front-end alone", true, false, &fe_bad, nullptr, nullptr) || !ask("all three", true, false, &fe, &dl, &xf) ||
          !ask("front-end alone", true, false, &fe, nullptr, nullptr) || !ask("no spec", true, false, nullptr, nullptr, nullptr))
        return 1;
    }

  // ---- CheckLoadArgs: the four kinds of load entry
  struct Kind { const char *name; int required; const char *text; };
  const Kind kinds[] = {{"plain", 0, "bad recognizer capacity"},
                        {"frontend", kNeedFrontend, "bad online recognizer capacity"},
                        {"deltas", kNeedFrontend | kNeedDeltas, "bad recognizer capacity"},
                        {"transform", kNeedFrontend | kNeedTransform, "bad online recognizer capacity"}};
  for (const Kind &k : kinds) {
    char what[96];
    auto ask = [&](const char *name, const char *path, const pk_mi355_frontend_spec_t *f, const pk_mi355_deltas_spec_t *d,
                   const pk_mi355_transform_spec_t *x, int units, int64_t cap, int64_t trace) {
      snprintf(what, sizeof(what), "load %s %s", k.name, name);
      Verdict(what, CheckLoadArgs(path, k.required, f, d, x, units, cap, trace, k.text));
    };
    const pk_mi355_frontend_spec_t *f = k.required & kNeedFrontend ? &fe : nullptr, *fb = f ? &fe_bad : nullptr;
    const pk_mi355_deltas_spec_t *d = k.required & (kNeedDeltas | kNeedTransform) ? &dl : nullptr, *db = d ? &dl_bad : nullptr;
    const pk_mi355_transform_spec_t *x = k.required & kNeedTransform ? &xf : nullptr, *xb = x ? &xf_bad : nullptr;
    ask("good", "m.conf", f, d, x, 2, 1600, 0);
    ask("null path", nullptr, f, d, x, 2, 1600, 0);
    ask("null path, all else bad", nullptr, fb, db, xb, 0, 0, -1);
    ask("no front-end", "m.conf", nullptr, d, x, 2, 1600, 0);
    ask("no deltas", "m.conf", f, nullptr, x, 2, 1600, 0);
    ask("no transform", "m.conf", f, d, nullptr, 2, 1600, 0);
    ask("bad specs, bad capacity", "m.conf", fb, db, xb, 0, 1600, 0);
    ask("bad deltas, transform", "m.conf", f, db, xb, 2, 1600, 0);
    ask("bad transform", "m.conf", f, d, xb, 2, 1600, 0);
    ask("no utterances", "m.conf", f, d, x, 0, 1600, 0);
    ask("no samples", "m.conf", f, d, x, 2, 0, 0);
    ask("negative trace", "m.conf", f, d, x, 2, 1600, -1);
  }
  printf("create_request_test ok\n");
  return 0;
}

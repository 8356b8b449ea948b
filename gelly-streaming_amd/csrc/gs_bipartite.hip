// gs_bipartite.hip — BipartitenessCheck over a window stream:
//   library/BipartitenessCheck.java:40-136 on WindowGraphAggregation.java:47-65 (GraphAggregation's Merger,
//   transientState = false): every window's edges are folded into a Candidates (updateFunction ->
//   edgeToCandidate :57-64 -> Candidates.merge, example/util/Candidates.java:76-138) and merged into the
//   running state (combineFunction -> Candidates.merge).  The state after a window says whether the graph
//   of all the edges seen so far has an odd cycle and, if it has none, holds its components with every
//   vertex's side.
//
// gs_window_bipartite computes the canonical form of that state (DESIGN.md "BipartitenessCheck") on the
// GPU from the window's edges and the previous state's (vertex, label, sign) rows.  Both are constraints
// (x, y, d): x and y lie on different sides (d = 1: a window edge, a state row with sign false) or on the
// same side (d = 0: a state row with sign true); x == y only makes x present.  It is the union-find window
// driver of gs_cc_common.hpp over the signed forest (word = parent << 1 | parity; the argument why its
// concurrent unions decide every constraint correctly stands with that policy).  Every vertex ends as its
// component's smallest vertex and its side relative to that vertex, the canonical (label, sign = parity == 0);
// a constraint that closes an odd cycle sets the fail word, and the window's state is (false,{}).
#include "gs_cc_common.hpp"

using namespace gs;

extern "C" {

gs_status gs_window_bipartite(gs_ctx* c, const gs_edge_batch* b, const gs_signed_batch* prev, gs_signed_out* out) {
  if (!c) return GS_EINVAL;
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (prev && prev->n && (!prev->keys || !prev->labels || !prev->signs)) return set_error(c, GS_EINVAL, "bad previous state");
  if (!out || !out->n_out || !out->success || (out->capacity && (!out->keys || !out->labels || !out->signs)))
    return set_error(c, GS_EINVAL, "bad gs_signed_out");
  GS_TRY(begin_call(c));
  hipEventRecord(c->ev[0], c->stream);
  *out->n_out = 0;
  *out->success = 0;
  if (prev && prev->failed) return GS_OK;   // Candidates.java:78-80: a failed state stays failed
  *out->success = 1;
  static const UfOp op{5, false, "bipartiteness state needs %llu vertices",
                       "bipartiteness: %llu vertices, the packed parent word holds 2^31 - 1"};
  return uf_window<SignedForest>(c, op, b, prev ? *prev : gs_signed_batch{}, *out);
}

}  // extern "C"

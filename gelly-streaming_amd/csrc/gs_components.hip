// gs_components.hip — ConnectedComponents over a window stream:
//   library/ConnectedComponents.java:56-131 on WindowGraphAggregation.java:47-65 (GraphAggregation's
//   Merger, transientState = false): every window's edges are folded into a DisjointSet (UpdateCC ->
//   DisjointSet.union, example/util/DisjointSet.java:97-123) and merged into the running state
//   (CombineCC -> DisjointSet.merge :132-136).  The state after a window is the partition of every
//   vertex seen so far into weakly connected components.
//
// gs_window_components computes that state on the GPU from the window's edges and the previous state
// (vertex, label) rows, which join the window as edges vertex -- label: the union-find window driver of
// gs_cc_common.hpp over the plain forest (word = parent).  Every vertex's root is the smallest vertex of
// its component (the compact ids are order-preserving), the canonical label of the partition.
// Which vertex the reference's DisjointSet keeps as a root depends on HashMap iteration order; the
// partition (what ConnectedComponentsTest and DisjointSet.toString observe) does not.
#include "gs_cc_common.hpp"

using namespace gs;

extern "C" {

gs_status gs_window_components(gs_ctx* c, const gs_edge_batch* b, const gs_partial_batch* prev, gs_vertex_out* out) {
  if (!c) return GS_EINVAL;
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (prev && prev->n && (!prev->keys || !prev->vals)) return set_error(c, GS_EINVAL, "bad previous state");
  if (prev && prev->n && prev->val_dtype != GS_I64) return set_error(c, GS_EINVAL, "state labels must be I64");
  if (!out || !out->n_out || (out->capacity && (!out->keys || !out->vals))) return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  GS_TRY(begin_call(c));
  hipEventRecord(c->ev[0], c->stream);
  *out->n_out = 0;
  gs_signed_batch state{};
  if (prev && prev->n) state = {prev->keys, (const int64_t*)prev->vals, nullptr, prev->n, prev->mem, 0};
  const gs_signed_out rows{out->keys, (int64_t*)out->vals, nullptr, out->capacity, out->n_out, nullptr, out->mem, 0};
  static const UfOp op{4, true, "components need %llu vertices", nullptr};   // (no limit below the 2^32 - 1 of the word)
  return uf_window<PlainForest>(c, op, b, state, rows);
}

}  // extern "C"

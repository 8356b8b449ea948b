// gs_aggregate.hip — SimpleEdgeStream.aggregate / globalAggregate with the built-in mappers: running per-vertex
// (or stream-wide) SUM / MIN / MAX / COUNT of the edge values, one output record per input record.
//
//   gs_agg_edges   <- aggregate(edgeMapper, vertexMapper) (SimpleEdgeStream.java:493-498: flatMap -> keyBy(0) -> map)
//                     with edgeMapper = DegreeTypeSeparator's order (:444-463) carrying the edge's value, and
//                     vertexMapper = a HashMap<K, VV> combined with the op
//   gs_agg_global  <- globalAggregate(edgeMapper, vertexMapper, collectUpdates) (:509-539; GlobalAggregateMapper
//                     :525-539 keeps a record only when the value differs from the previous one)
//
// A keyed gs_agg owns gs_ctable.hpp's table, vertex -> the 64 bits of its accumulator (a 4-byte accumulator in the
// low half).  An accumulator may hold any bit pattern, so "present" is the key being in the table; vertex -1 has
// the side word meta[CT_SIDE] and its presence flag meta[AG_HAS].  A global gs_agg is those two words alone.
// One keyed batch:
//
//   ct_sorted_runs      the stable sort with the arrival index as payload, run keys[U], offsets[U + 1]
//                       (shared with gs_cont_degrees)
//   k_ag_gather         vs[p] = val[rec[p]] (val[rec[p] >> 1] under ALL): the values in sorted order
//   k_ag_upsert         one lane per run: claim the slot, base[u] = the accumulator before the batch,
//                       where[u] = the slot and the fresh flag (the slot's new value falls out of the scan)
//   k_ag_scan<.., 0>    per tile of AG_TILE sorted positions: the segmented aggregate (heads, trailing partial);
//                       a run's head element is base[u] (+) value, or the value itself for a fresh vertex
//   k_ag_carry          one block: the exclusive segmented scan of the tile aggregates, in place
//   k_ag_scan<.., 1>    the same tile again with its carry: the inclusive segmented scan, out[rec[p]], and at a
//                       run's last position the accumulator into its slot
//   k_ct_expand_all     the vertex column (a copy under IN / OUT)
//
// Three launches, no waiting between workgroups: a hub's run spans many tiles and its carry comes from
// k_ag_carry.  Global mode is the same scan over one run (offs = {0, R}, base = the stream's accumulator) with
// rec = identity; with collect_updates: flags where the value's bits (NaN canonical) differ from the previous
// record's, xscan, k_ag_compact.
// Combine rules are gs_rbk.hpp's ValueOp (gs_window_reduce's): integer sums wrap at their width, MIN / MAX as
// Math.min / Math.max.  A float SUM is a scan, so it is associated differently from the arrival-order fold (and
// differently for different batch cuts): equal where every partial sum is exact, within rounding otherwise.
#include "gs_ctable.hpp"

namespace gs {

enum { AG_HAS = 4, AG_META = 5 };   // meta[AG_HAS]: vertex -1 (keyed) / the stream (global) has an accumulator
constexpr int AG_BLOCK = 256, AG_ITEMS = 8, AG_TILE = AG_BLOCK * AG_ITEMS;
// where[u]: the slot of run u's vertex, and
constexpr unsigned long long AG_FRESH = 1ull << 63;   // no accumulator before this batch
constexpr unsigned long long AG_SIDE = 1ull << 62;    // the accumulator is meta[CT_SIDE]
constexpr unsigned long long AG_NONE = 1ull << 61;    // the table was full (the call fails): nothing to write

template <typename T>
__device__ __forceinline__ unsigned long long ag_bits(T v) {
  if constexpr (sizeof(T) == 8) {
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
    return b;
  } else {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
  }
}
template <typename T>
__device__ __forceinline__ T ag_value(unsigned long long b) {
  T v;
  if constexpr (sizeof(T) == 8) {
    __builtin_memcpy(&v, &b, 8);
  } else {
    const uint32_t w = (uint32_t)b;
    __builtin_memcpy(&v, &w, 4);
  }
  return v;
}

// the exclusive segmented scan of one Seg per thread over the block (gs_rbk.hpp's seg_combine, as
// k_reduce_by_key scans its thread aggregates); total: the block's aggregate, in every thread.
// s_wagg: BLOCK / WAVE entries, written once per call.
template <class Op, int BLOCK>
__device__ __forceinline__ Seg<typename Op::Acc> block_seg_exclusive(Seg<typename Op::Acc> agg, Seg<typename Op::Acc>* s_wagg,
                                                                     Seg<typename Op::Acc>& total) {
  using S = Seg<typename Op::Acc>;
  constexpr int NW = BLOCK / WAVE;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  S inc = agg;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    S y;
    y.cnt = __shfl_up(inc.cnt, o, WAVE);
    y.valid = __shfl_up(inc.valid, o, WAVE);
    y.v = shfl_up_acc(inc.v, o);
    if (lane >= o) inc = seg_combine<Op>(y, inc);
  }
  S excl;
  excl.cnt = __shfl_up(inc.cnt, 1, WAVE);
  excl.valid = __shfl_up(inc.valid, 1, WAVE);
  excl.v = shfl_up_acc(inc.v, 1);
  if (lane == 0) {
    excl.valid = 0;
    excl.cnt = 0;
  }
  if (lane == 63) s_wagg[wid] = inc;
  __syncthreads();
  S pre{0u, 0u, typename Op::Acc()}, tot{0u, 0u, typename Op::Acc()};
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const S x = s_wagg[w];
    if (w < wid) pre = seg_combine<Op>(pre, x);
    tot = seg_combine<Op>(tot, x);
  }
  total = tot;
  return seg_combine<Op>(pre, excl);
}

// the values in sorted order (W: the value's bits, 4 or 8 bytes); rec == nullptr: arrival order itself
template <typename W>
__global__ __launch_bounds__(256) void k_ag_gather(const W* __restrict__ val, const uint32_t* __restrict__ rec, int all,
                                                   uint64_t R, W* __restrict__ vs) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < R; p += (uint64_t)gridDim.x * 256) {
    const uint64_t r = rec ? rec[p] : p;
    vs[p] = val[all ? r >> 1 : r];
  }
}

// lane per run u of the batch: claim the vertex's slot; base[u] = its accumulator before the batch
__global__ __launch_bounds__(256) void k_ag_upsert(CtTable t, const int64_t* __restrict__ run_keys, uint32_t U,
                                                   uint64_t* __restrict__ base, unsigned long long* __restrict__ where) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long n_fresh = 0;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u < U; u += (uint64_t)gridDim.x * 256) {
    bool fresh = false;
    const unsigned long long id = (unsigned long long)run_keys[u];
    unsigned long long w;
    uint64_t b = 0;
    if (id == TAB_EMPTY) {
      fresh = t.meta[AG_HAS] == 0;
      b = t.meta[CT_SIDE];
      t.meta[AG_HAS] = 1;
      w = AG_SIDE;
    } else {
      const unsigned long long s = ct_slot(t, id, &fresh);
      if (s == ~0ull) {
        fresh = false;
        atomicOr(&t.meta[CT_ERR], 1ull);
        w = AG_NONE;
      } else {
        b = fresh ? 0 : t.slots[2 * s + 1];
        w = s;
      }
    }
    base[u] = b;
    where[u] = w | (fresh ? AG_FRESH : 0ull);
    n_fresh += fresh;
  }
  block_add(&t.meta[CT_DISTINCT], n_fresh, s_part);
}

// global mode: the stream is one run over the side word.  run[0..1] = offsets {0, R}, run[2] = base, run[3] = where
__global__ void k_ag_global_seed(unsigned long long* __restrict__ meta, uint64_t R, uint64_t* __restrict__ run) {
  run[0] = 0;
  run[1] = R;
  run[2] = meta[CT_SIDE];
  run[3] = AG_SIDE | (meta[AG_HAS] ? 0ull : AG_FRESH);
  meta[AG_HAS] = 1;
}

// PHASE 0: tile_cnt[tile] / tile_v[tile] = the tile's heads and trailing partial.
// PHASE 1: with tile_cnt[tile] (carry valid) / tile_v[tile] (carry) from k_ag_carry: out[rec[p]] = the running
// accumulator at sorted position p, and each run's last value into its slot.
// vs: 16-byte aligned (a ctx buffer); HAS_V false: every value is 1 (COUNT).
template <typename T, int OP, bool HAS_V, int PHASE>
__global__ __launch_bounds__(AG_BLOCK) void k_ag_scan(const T* __restrict__ vs, const uint64_t* __restrict__ offs,
                                                      const uint64_t* __restrict__ base,
                                                      const unsigned long long* __restrict__ where, uint32_t U, uint32_t R,
                                                      uint64_t* __restrict__ tile_cnt, uint64_t* __restrict__ tile_v,
                                                      const uint32_t* __restrict__ rec, T* __restrict__ out,
                                                      unsigned long long* __restrict__ slots,
                                                      unsigned long long* __restrict__ meta) {
  using Op = ValueOp<T, OP>;
  using S = Seg<T>;
  constexpr int PER = 16 / sizeof(T);
  __shared__ __attribute__((aligned(16))) T s_v[AG_TILE + AG_TILE / 32 + 2];
  __shared__ S s_wagg[AG_BLOCK / WAVE];
  __shared__ uint32_t s_lo, s_hi;
  const int tid = threadIdx.x;
  const uint32_t tile = blockIdx.x;
  const uint64_t t0 = (uint64_t)tile * AG_TILE;
  if (t0 >= R) return;
  const uint32_t tile_n = (uint32_t)min((uint64_t)AG_TILE, (uint64_t)R - t0);
  if (tid == 0) s_lo = ct_run_of(offs, 0, U - 1, t0);
  if (tid == 64) s_hi = ct_run_of(offs, 0, U - 1, t0 + tile_n - 1);
  if constexpr (HAS_V) {
    if (tile_n == AG_TILE) {   // striped 16-byte loads
      const T* tv = vs + t0;
      T lv[AG_ITEMS];
#pragma unroll
      for (int j = 0; j < AG_ITEMS / PER; ++j) {
        const u32x4 q = ld16w<false>(tv + (size_t)(j * AG_BLOCK + tid) * PER);
        __builtin_memcpy(&lv[j * PER], &q, 16);
      }
#pragma unroll
      for (int j = 0; j < AG_ITEMS / PER; ++j)
#pragma unroll
        for (int e = 0; e < PER; ++e) s_v[pad32((uint32_t)(j * AG_BLOCK + tid) * PER + e)] = lv[j * PER + e];
    } else {
      for (uint32_t i = tid; i < tile_n; i += AG_BLOCK) s_v[pad32(i)] = vs[t0 + i];
    }
  }
  __syncthreads();

  // thread-local: AG_ITEMS consecutive sorted positions; a run's head element carries the run's seed
  const uint32_t first = (uint32_t)tid * AG_ITEMS;
  const uint32_t mine = first < tile_n ? min((uint32_t)AG_ITEMS, tile_n - first) : 0u;
  const uint64_t p0 = t0 + first;
  uint32_t u0 = 0;
  uint64_t next0 = 0;
  bool head0 = false;
  if (mine) {
    u0 = ct_run_of(offs, s_lo, s_hi, p0);
    head0 = offs[u0] == p0;
    next0 = offs[u0 + 1];
  }
  T e[AG_ITEMS];
  uint32_t headmask = 0;
  S agg{0u, mine > 0 ? 1u : 0u, T()};
  {
    uint32_t u = u0;
    uint64_t next = next0;
#pragma unroll
    for (int j = 0; j < AG_ITEMS; ++j) {
      e[j] = T();
      if ((uint32_t)j < mine) {
        const uint64_t p = p0 + j;
        bool head = head0;
        if (j > 0) {
          head = p == next;
          if (head) {
            ++u;
            next = offs[u + 1];
          }
        }
        T x = T(1);
        if constexpr (HAS_V) x = s_v[pad32(first + j)];
        if (head) {
          if (!(where[u] & AG_FRESH)) x = Op::combine(ag_value<T>(base[u]), x);
          headmask |= 1u << j;
          agg.cnt++;
          agg.v = x;
        } else {
          agg.v = (j == 0) ? x : Op::combine(agg.v, x);
        }
        e[j] = x;
      }
    }
  }
  S total;
  const S excl = block_seg_exclusive<Op, AG_BLOCK>(agg, s_wagg, total);
  if constexpr (PHASE == 0) {
    if (tid == 0) {
      tile_cnt[tile] = total.cnt;
      tile_v[tile] = ag_bits(total.v);
    }
  } else {
    S pre{0u, 0u, T()};
    if (tile > 0 && tile_cnt[tile]) {
      pre.valid = 1;
      pre.v = ag_value<T>(tile_v[tile]);
    }
    const S start = seg_combine<Op>(pre, excl);
    T run = start.v;
    uint32_t u = u0;
    uint64_t next = next0;
    // every thread has passed block_seg_exclusive's barrier, after its last read of s_v: the slots are free
#pragma unroll
    for (int j = 0; j < AG_ITEMS; ++j) {
      if ((uint32_t)j < mine) {
        const uint64_t p = p0 + j;
        if (j > 0 && p == next) {
          ++u;
          next = offs[u + 1];
        }
        run = (headmask & (1u << j)) ? e[j] : Op::combine(run, e[j]);
        s_v[pad32(first + j)] = run;
        if (p + 1 == next) {   // the run ends here: its vertex's accumulator after the batch
          const unsigned long long w = where[u];
          if (w & AG_SIDE) meta[CT_SIDE] = ag_bits(run);
          else if (!(w & AG_NONE)) slots[2 * (w & ~AG_FRESH) + 1] = ag_bits(run);
        }
      }
    }
    __syncthreads();
    for (uint32_t i = tid; i < tile_n; i += AG_BLOCK) {
      const uint64_t p = t0 + i;
      out[rec ? rec[p] : p] = s_v[pad32(i)];
    }
  }
}

// one block: (tile_cnt, tile_v)[0 .. nt) -> each tile's carry in: tile_cnt = the carry is valid, tile_v = its value.
// Thread t owns ceil(nt / SCAN_BLOCK) consecutive tiles (block_scan_array_chunked's traversal).
template <typename T, int OP>
__global__ __launch_bounds__(SCAN_BLOCK) void k_ag_carry(uint64_t* __restrict__ tile_cnt, uint64_t* __restrict__ tile_v,
                                                         uint32_t nt) {
  using Op = ValueOp<T, OP>;
  using S = Seg<T>;
  __shared__ S s_wagg[SCAN_BLOCK / WAVE];
  const uint32_t per = (nt + SCAN_BLOCK - 1) / SCAN_BLOCK, lo = min(nt, threadIdx.x * per), hi = min(nt, lo + per);
  S agg{0u, 0u, T()};
  for (uint32_t i = lo; i < hi; ++i) agg = seg_combine<Op>(agg, S{(uint32_t)tile_cnt[i], 1u, ag_value<T>(tile_v[i])});
  S total;
  S run = block_seg_exclusive<Op, SCAN_BLOCK>(agg, s_wagg, total);
  for (uint32_t i = lo; i < hi; ++i) {
    const S x{(uint32_t)tile_cnt[i], 1u, ag_value<T>(tile_v[i])};
    tile_cnt[i] = run.valid;
    tile_v[i] = ag_bits(run.v);
    run = seg_combine<Op>(run, x);
  }
}

// Java equals on the boxed value: the bits, every NaN as one (kind 1: float, 2: double)
__device__ __forceinline__ unsigned long long ag_canon(unsigned long long b, int kind) {
  if (kind == 1 && (b & 0x7fffffffull) > 0x7f800000ull) return 0x7fc00000ull;
  if (kind == 2 && (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return 0x7ff8000000000000ull;
  return b;
}

// global mode, collect_updates: flags[r] = record r's value differs from the record before it (run[2] / run[3]:
// the accumulator before the batch and whether there was one)
template <typename W>
__global__ __launch_bounds__(256) void k_ag_changed(const W* __restrict__ full, uint64_t R, const uint64_t* __restrict__ run,
                                                    int kind, uint64_t* __restrict__ flags) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
    const unsigned long long x = ag_canon(full[r], kind);
    bool keep;
    if (r == 0) keep = (run[3] & AG_FRESH) || x != ag_canon((W)run[2], kind);
    else keep = x != ag_canon(full[r - 1], kind);
    flags[r] = keep;
  }
}

// kept record r -> output row pos[r]; dir picks the record's vertex (out_k may be null)
template <typename W>
__global__ __launch_bounds__(256) void k_ag_compact(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ pos,
                                                    uint64_t R, const W* __restrict__ full, const int64_t* __restrict__ src,
                                                    const int64_t* __restrict__ dst, int dir, int64_t* __restrict__ out_k,
                                                    W* __restrict__ out_v) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
    if (!flags[r]) continue;
    const uint64_t k = pos[r];
    out_v[k] = full[r];
    if (out_k) out_k[k] = dir == GS_DIR_ALL ? ((r & 1) ? dst[r >> 1] : src[r >> 1]) : dir == GS_DIR_OUT ? src[r] : dst[r];
  }
}

// checkpoint: the occupied slots as (id with the sign bit flipped, accumulator bits) rows in any order; n rows expected
__global__ __launch_bounds__(256) void k_ag_dump(CtTable t, unsigned long long* __restrict__ ok,
                                                 unsigned long long* __restrict__ oa, uint64_t n) {
  const uint64_t cap = t.mask + 1, stride = (uint64_t)gridDim.x * 256;
  if (blockIdx.x == 0 && threadIdx.x == 0 && t.meta[AG_HAS]) {
    const unsigned long long i = atomicAdd(&t.meta[CT_SUM], 1ull);
    if (i < n) {
      ok[i] = TAB_EMPTY ^ TAB_SIGN;
      oa[i] = t.meta[CT_SIDE];
    }
  }
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 < cap; s0 += stride) {
    const uint64_t s = s0 + threadIdx.x;
    const unsigned long long id = s < cap ? t.slots[2 * s] : TAB_EMPTY;
    const bool occ = id != TAB_EMPTY;
    const unsigned long long i = wave_compact_base(occ, &t.meta[CT_SUM]);
    if (occ && i < n) {
      ok[i] = id ^ TAB_SIGN;
      oa[i] = t.slots[2 * s + 1];
    }
  }
}

// a checkpoint's 64-bit accumulator words -> 4-byte values
__global__ __launch_bounds__(256) void k_ag_narrow(const uint64_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) out[i] = (uint32_t)in[i];
}

// restore: lane per row (W: the accumulator's bits); a vertex that comes twice sets error bit 2
template <typename W>
__global__ __launch_bounds__(256) void k_ag_import(CtTable t, const int64_t* __restrict__ keys, const W* __restrict__ vals,
                                                   uint64_t n) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long n_fresh = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    bool fresh = false;
    const unsigned long long id = (unsigned long long)keys[i];
    if (id == TAB_EMPTY) {
      fresh = atomicExch(&t.meta[AG_HAS], 1ull) == 0;
      if (fresh) t.meta[CT_SIDE] = vals[i];
    } else {
      const unsigned long long s = ct_slot(t, id, &fresh);
      if (s == ~0ull) atomicOr(&t.meta[CT_ERR], 1ull);
      else if (fresh) t.slots[2 * s + 1] = vals[i];
    }
    if (!fresh) atomicOr(&t.meta[CT_ERR], 2ull);
    n_fresh += fresh;
  }
  block_add(&t.meta[CT_DISTINCT], n_fresh, s_part);
}

}  // namespace gs

using namespace gs;

struct gs_agg {
  int device = 0;
  int32_t mode = GS_AGG_KEYED, op = GS_OP_SUM, dtype = GS_I64;
  unsigned long long* slots = nullptr;  // device [cap][2] (keyed)
  unsigned long long* meta = nullptr;   // device u64[AG_META]
  uint64_t cap = 0;                     // slots (power of two; 0: global)
  uint64_t distinct = 0, records = 0, growths = 0;
};

namespace {

CtTable table_of(const gs_agg* t) { return CtTable{t->slots, t->cap - 1, t->meta}; }

// accumulator dtype: the value dtype, I64 for COUNT
int acc_dtype(const gs_agg* t) { return t->op == GS_OP_COUNT ? GS_I64 : t->dtype; }

gs_status check_state(gs_ctx* c, const gs_agg* t) {
  if (!c) return GS_EINVAL;
  if (!t) return set_error(c, GS_EINVAL, "null aggregate state");
  if (t->device != c->device)
    return set_error(c, GS_EINVAL, "aggregate state lives on device %d, the ctx on device %d", t->device, c->device);
  return GS_OK;
}

struct ScanArgs {
  const void* vs;
  const uint64_t *offs, *base;
  const unsigned long long* where;
  uint32_t U, R;
  uint64_t *tile_cnt, *tile_v;
  const uint32_t* rec;
  void* out;
  unsigned long long *slots, *meta;
};

template <typename T, int OP, bool HAS_V>
gs_status run_scan(gs_ctx* c, const ScanArgs& a) {
  const uint32_t nt = (a.R + AG_TILE - 1) / AG_TILE;
  if (nt > 1) {
    hipLaunchKernelGGL((k_ag_scan<T, OP, HAS_V, 0>), dim3(nt), dim3(AG_BLOCK), 0, c->stream, (const T*)a.vs, a.offs, a.base,
                       a.where, a.U, a.R, a.tile_cnt, a.tile_v, a.rec, (T*)a.out, a.slots, a.meta);
    GS_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ag_carry<T, OP>), dim3(1), dim3(SCAN_BLOCK), 0, c->stream, a.tile_cnt, a.tile_v, nt);
    GS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((k_ag_scan<T, OP, HAS_V, 1>), dim3(nt), dim3(AG_BLOCK), 0, c->stream, (const T*)a.vs, a.offs, a.base,
                     a.where, a.U, a.R, a.tile_cnt, a.tile_v, a.rec, (T*)a.out, a.slots, a.meta);
  GS_HIP(hipGetLastError());
  return GS_OK;
}

template <typename T>
gs_status scan_ops(gs_ctx* c, int op, const ScanArgs& a) {
  switch (op) {
    case GS_OP_SUM: return run_scan<T, OP_SUM, true>(c, a);
    case GS_OP_MIN: return run_scan<T, OP_MIN, true>(c, a);
    case GS_OP_MAX: return run_scan<T, OP_MAX, true>(c, a);
  }
  return set_error(c, GS_EINVAL, "bad op %d", op);
}

gs_status scan_dispatch(gs_ctx* c, const gs_agg* t, const ScanArgs& a) {
  if (t->op == GS_OP_COUNT) return run_scan<int64_t, OP_SUM, false>(c, a);
  switch (t->dtype) {
    case GS_I32: return scan_ops<int32_t>(c, t->op, a);
    case GS_I64: return scan_ops<int64_t>(c, t->op, a);
    case GS_F32: return scan_ops<float>(c, t->op, a);
    case GS_F64: return scan_ops<double>(c, t->op, a);
  }
  return set_error(c, GS_EINVAL, "bad dtype %d", t->dtype);
}

// one micro-batch through the state (global: collect >= 0)
gs_status agg_batch(gs_ctx* c, gs_agg* t, const gs_edge_batch* b, int32_t dir, gs_vertex_out* out, int mode, int collect) {
  GS_TRY(check_state(c, t));
  GS_TRY(check_batch(c, b, dir));
  if (t->mode != mode)
    return set_error(c, GS_EINVAL, "a %s aggregate state: use %s", t->mode == GS_AGG_KEYED ? "keyed" : "global",
                     t->mode == GS_AGG_KEYED ? "gs_agg_edges" : "gs_agg_global");
  if (b->val_dtype != t->dtype)
    return set_error(c, GS_EINVAL, "batch dtype %d, the aggregate state's is %d", b->val_dtype, t->dtype);
  const bool has_v = t->op != GS_OP_COUNT;
  if (has_v && b->n && !b->val) return set_error(c, GS_EINVAL, "null val");
  if (!out || !out->n_out || (out->capacity && (!out->vals || (mode == GS_AGG_KEYED && !out->keys))))
    return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  const uint64_t R = dir == GS_DIR_ALL ? 2 * b->n : b->n;
  *out->n_out = R;
  if (out->capacity < R) return set_error(c, GS_ECAPACITY, "output needs room for %llu records", (unsigned long long)R);
  GS_TRY(begin_call(c));
  *out->n_out = 0;
  if (R == 0) return GS_OK;
  const size_t ab = dtype_bytes(acc_dtype(t));   // accumulator = value width (COUNT: no value column is read)
  const uint64_t nt = (R + AG_TILE - 1) / AG_TILE;
  const bool keyed = mode == GS_AGG_KEYED;
  // everything that can fail for want of memory comes before the state changes
  GS_TRY(ensure(c, c->ct[0], R * 8));
  GS_TRY(ensure(c, c->ct[1], (R + 3) * 8));   // run offsets; global: the one run's four words
  GS_TRY(ensure(c, c->ct[2], R * 8));
  GS_TRY(ensure(c, c->ct[3], (R + 1) * 8));
  GS_TRY(ensure(c, c->ct[4], R * 8 + nt * 16));
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t* ov = out->keys;
  void* ox = out->vals;
  if (!direct) {
    if (ov) {
      GS_TRY(ensure(c, c->out_keys, R * 8));
      ov = c->out_keys.as<int64_t>();
    }
    GS_TRY(ensure(c, c->out_a, R * 8));
    ox = c->out_a.p;
  }
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, has_v));
  void* vs = c->ct[4].p;
  uint64_t* tile_v = (uint64_t*)((char*)vs + R * 8);
  uint64_t* tile_cnt = tile_v + nt;
  const int all = dir == GS_DIR_ALL;
  ScanArgs a{vs, nullptr, nullptr, nullptr, 1u, (uint32_t)R, tile_cnt, tile_v, nullptr, ox, t->slots, t->meta};
  uint64_t rows = R;
  if (keyed) {
    Sorted s;
    int64_t* rk = c->ct[0].as<int64_t>();
    uint64_t* offs = c->ct[1].as<uint64_t>();
    uint64_t* base = c->ct[2].as<uint64_t>();
    unsigned long long* where = c->ct[3].as<unsigned long long>();
    uint64_t U = 0;
    GS_TRY(ct_sorted_runs(c, src, dst, b->n, dir, R, &s, rk, offs, &U));
    // the batch brings at most U new vertices: room for them at load <= 1/2, or the call ends here
    GS_TRY(ct_reserve(c, t, t->distinct + U, AG_META));
    const uint32_t* rec = (const uint32_t*)s.vals;
    if (has_v) {
      if (ab == 4) hipLaunchKernelGGL(k_ag_gather<uint32_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint32_t*)val, rec, all, R, (uint32_t*)vs);
      else hipLaunchKernelGGL(k_ag_gather<uint64_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint64_t*)val, rec, all, R, (uint64_t*)vs);
      GS_HIP(hipGetLastError());
    }
    // ---- the table changes from here on ----
    a.slots = t->slots;   // ct_reserve may have replaced the table
    hipLaunchKernelGGL(k_ag_upsert, dim3(tab_grid_tab(U)), dim3(256), 0, c->stream, table_of(t), rk, (uint32_t)U, base, where);
    GS_HIP(hipGetLastError());
    a.offs = offs;
    a.base = base;
    a.where = where;
    a.U = (uint32_t)U;
    a.rec = rec;
    GS_TRY(scan_dispatch(c, t, a));
    if (all) {
      hipLaunchKernelGGL(k_ct_expand_all, dim3(tab_grid(R)), dim3(256), 0, c->stream, src, dst, b->n, ov);
      GS_HIP(hipGetLastError());
    } else {
      GS_HIP(hipMemcpyAsync(ov, dir == GS_DIR_OUT ? src : dst, R * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    GS_TRY(tab_read_meta(c, t->meta, AG_META));
    if (c->host_small[8 + CT_ERR]) return set_error(c, GS_EDEVICE, "aggregate state: the vertex table filled up");
    t->distinct = c->host_small[8 + CT_DISTINCT];
  } else {
    uint64_t* flags = c->ct[0].as<uint64_t>();
    uint64_t* run = c->ct[1].as<uint64_t>();
    void* full = c->ct[2].p;
    uint64_t* pos = c->ct[3].as<uint64_t>();
    if (has_v) {
      if (ab == 4) hipLaunchKernelGGL(k_ag_gather<uint32_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint32_t*)val, (const uint32_t*)nullptr, all, R, (uint32_t*)vs);
      else hipLaunchKernelGGL(k_ag_gather<uint64_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint64_t*)val, (const uint32_t*)nullptr, all, R, (uint64_t*)vs);
      GS_HIP(hipGetLastError());
    }
    // ---- the state changes from here on ----
    hipLaunchKernelGGL(k_ag_global_seed, dim3(1), dim3(1), 0, c->stream, t->meta, R, run);
    GS_HIP(hipGetLastError());
    a.offs = run;
    a.base = run + 2;
    a.where = (const unsigned long long*)(run + 3);
    a.slots = nullptr;
    if (collect) a.out = full;
    GS_TRY(scan_dispatch(c, t, a));
    if (collect) {
      const int kind = t->op == GS_OP_COUNT ? 0 : t->dtype == GS_F32 ? 1 : t->dtype == GS_F64 ? 2 : 0;
      if (ab == 4) hipLaunchKernelGGL(k_ag_changed<uint32_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint32_t*)full, R, (const uint64_t*)run, kind, flags);
      else hipLaunchKernelGGL(k_ag_changed<uint64_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint64_t*)full, R, (const uint64_t*)run, kind, flags);
      GS_HIP(hipGetLastError());
      GS_TRY(xscan(c, flags, R, pos));
      if (ab == 4) hipLaunchKernelGGL(k_ag_compact<uint32_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint64_t*)flags, (const uint64_t*)pos, R, (const uint32_t*)full, src, dst, (int)dir, ov, (uint32_t*)ox);
      else hipLaunchKernelGGL(k_ag_compact<uint64_t>, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint64_t*)flags, (const uint64_t*)pos, R, (const uint64_t*)full, src, dst, (int)dir, ov, (uint64_t*)ox);
      GS_HIP(hipGetLastError());
      GS_HIP(hipMemcpyAsync(c->host_small + 6, pos + R, 8, hipMemcpyDeviceToHost, c->stream));
      GS_TRY(host_wait(c));
      rows = c->host_small[6];
      if (rows > R) return set_error(c, GS_EDEVICE, "aggregate state: %llu updates in %llu records",
                                     (unsigned long long)rows, (unsigned long long)R);
    } else if (ov) {
      if (all) {
        hipLaunchKernelGGL(k_ct_expand_all, dim3(tab_grid(R)), dim3(256), 0, c->stream, src, dst, b->n, ov);
        GS_HIP(hipGetLastError());
      } else {
        GS_HIP(hipMemcpyAsync(ov, dir == GS_DIR_OUT ? src : dst, R * 8, hipMemcpyDeviceToDevice, c->stream));
      }
    }
    t->distinct = 1;
  }
  t->records += R;
  *out->n_out = rows;
  if (!direct && rows) {
    if (out->keys) GS_TRY(deliver(c, out->keys, ov, rows * 8, out->mem));
    GS_TRY(deliver(c, out->vals, ox, rows * ab, out->mem));
    GS_TRY(host_wait(c));
  }
  return GS_OK;
}

// an empty state again (after a refused import)
gs_status clear_state(gs_ctx* c, gs_agg* t) {
  if (t->slots) {
    hipLaunchKernelGGL(k_ct_clear, dim3(tab_grid(t->cap)), dim3(256), 0, c->stream, (ulonglong2*)t->slots, t->cap);
    GS_HIP(hipGetLastError());
  }
  GS_HIP(hipMemsetAsync(t->meta, 0, AG_META * 8, c->stream));
  t->distinct = t->records = 0;
  return host_wait(c);
}

}  // namespace

extern "C" {

gs_status gs_agg_create(gs_ctx* c, int32_t mode, int32_t op, int32_t val_dtype, uint64_t reserve_vertices, gs_agg** out) {
  if (!c) return GS_EINVAL;
  if (!out) return set_error(c, GS_EINVAL, "gs_agg_create: null argument");
  *out = nullptr;
  if (mode != GS_AGG_KEYED && mode != GS_AGG_GLOBAL) return set_error(c, GS_EINVAL, "gs_agg_create: bad mode %d", mode);
  if (op < GS_OP_SUM || op > GS_OP_COUNT) return set_error(c, GS_EINVAL, "gs_agg_create: bad op %d", op);
  if (val_dtype < GS_I32 || val_dtype > GS_NONE || (val_dtype == GS_NONE && op != GS_OP_COUNT))
    return set_error(c, GS_EINVAL, "gs_agg_create: bad dtype %d for op %d", val_dtype, op);
  if (reserve_vertices > (1ull << 38)) return set_error(c, GS_ENOMEM, "gs_agg_create: %llu vertices",
                                                       (unsigned long long)reserve_vertices);
  (void)hipGetLastError();
  GS_HIP(hipSetDevice(c->device));
  gs_agg* t = new (std::nothrow) gs_agg();
  if (!t) return set_error(c, GS_ENOMEM, "gs_agg_create");
  t->device = c->device;
  t->mode = mode;
  t->op = op;
  t->dtype = val_dtype;
  gs_status st = GS_OK;
  if (mode == GS_AGG_KEYED) {
    t->cap = 64;
    while (t->cap / 2 < reserve_vertices) t->cap *= 2;
    st = ct_alloc_table(c, t->cap, &t->slots);
  }
  if (st == GS_OK && hipMalloc((void**)&t->meta, AG_META * 8) != hipSuccess) {
    (void)hipGetLastError();
    st = set_error(c, GS_ENOMEM, "gs_agg_create: state words");
  }
  if (st == GS_OK) st = hip_check(c, hipMemsetAsync(t->meta, 0, AG_META * 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) st = host_wait(c);
  if (st != GS_OK) {
    gs_agg_destroy(t);
    return st;
  }
  *out = t;
  return GS_OK;
}

void gs_agg_destroy(gs_agg* t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->slots) hipFree(t->slots);
  if (t->meta) hipFree(t->meta);
  delete t;
}

gs_status gs_agg_size(const gs_agg* t, uint64_t* distinct_vertices, uint64_t* records) {
  if (!t) return GS_EINVAL;
  if (distinct_vertices) *distinct_vertices = t->distinct;
  if (records) *records = t->records;
  return GS_OK;
}

gs_status gs_agg_capacity(const gs_agg* t, uint64_t* slots, uint64_t* growths) {
  if (!t) return GS_EINVAL;
  if (slots) *slots = t->cap;
  if (growths) *growths = t->growths;
  return GS_OK;
}

gs_status gs_agg_edges(gs_ctx* c, gs_agg* t, const gs_edge_batch* b, int32_t dir, gs_vertex_out* out) {
  return agg_batch(c, t, b, dir, out, GS_AGG_KEYED, 0);
}

gs_status gs_agg_global(gs_ctx* c, gs_agg* t, const gs_edge_batch* b, int32_t dir, int32_t collect_updates,
                        gs_vertex_out* out) {
  return agg_batch(c, t, b, dir, out, GS_AGG_GLOBAL, collect_updates != 0);
}

gs_status gs_agg_export(gs_ctx* c, const gs_agg* t, gs_vertex_out* out) {
  GS_TRY(check_state(c, t));
  if (!out || !out->n_out || (out->capacity && (!out->keys || !out->vals)))
    return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  const uint64_t D = t->distinct;
  *out->n_out = D;
  if (out->capacity < D) return set_error(c, GS_ECAPACITY, "output needs %llu vertices", (unsigned long long)D);
  if (D >= (1ull << 32)) return set_error(c, GS_EUNSUPPORTED, "export of %llu vertices (limit 2^32 - 1)", (unsigned long long)D);
  GS_TRY(begin_call(c));
  if (D == 0) return GS_OK;
  const size_t ab = dtype_bytes(acc_dtype(t));
  if (t->mode == GS_AGG_GLOBAL) {   // one row: (0, the accumulator)
    GS_TRY(ensure(c, c->ct[0], 16));
    GS_HIP(hipMemsetAsync(c->ct[0].p, 0, 8, c->stream));
    GS_TRY(deliver(c, out->keys, c->ct[0].p, 8, out->mem));
    GS_TRY(deliver(c, out->vals, t->meta + CT_SIDE, ab, out->mem));   // little-endian: a 4-byte value is the low half
    return host_wait(c);
  }
  GS_TRY(ensure(c, c->ct[0], D * 8));
  GS_TRY(ensure(c, c->ct[1], D * 8));
  GS_TRY(ensure(c, c->out_keys, D * 8));
  GS_TRY(ensure(c, c->out_a, D * 4));
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t* ok = direct ? out->keys : c->out_keys.as<int64_t>();
  unsigned long long* dk = c->ct[0].as<unsigned long long>();
  unsigned long long* da = c->ct[1].as<unsigned long long>();
  GS_HIP(hipMemsetAsync(t->meta + CT_SUM, 0, 8, c->stream));
  hipLaunchKernelGGL(k_ag_dump, dim3(tab_grid(t->cap)), dim3(256), 0, c->stream, table_of(t), dk, da, D);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, AG_META));
  if (c->host_small[8 + CT_SUM] != D)
    return set_error(c, GS_EDEVICE, "aggregate state: %llu entries in the table, %llu expected",
                     (unsigned long long)c->host_small[8 + CT_SUM], (unsigned long long)D);
  // ascending signed ids = ascending (id ^ sign bit) as unsigned
  Sorted s;
  GS_TRY(sort_buffer(c, (const uint64_t*)dk, da, D, &s, 64, 8));
  if (s.wide)
    hipLaunchKernelGGL(k_tab_unkey<uint64_t>, dim3(tab_grid(D)), dim3(256), 0, c->stream, (const uint64_t*)s.keys,
                       s.key_xor, D, ok);
  else
    hipLaunchKernelGGL(k_tab_unkey<uint32_t>, dim3(tab_grid(D)), dim3(256), 0, c->stream, (const uint32_t*)s.keys,
                       s.key_xor, D, ok);
  GS_HIP(hipGetLastError());
  const void* vals = s.vals;
  if (ab == 4) {
    hipLaunchKernelGGL(k_ag_narrow, dim3(tab_grid(D)), dim3(256), 0, c->stream, (const uint64_t*)s.vals, D,
                       c->out_a.as<uint32_t>());
    GS_HIP(hipGetLastError());
    vals = c->out_a.p;
  }
  GS_TRY(deliver(c, out->keys, ok, D * 8, out->mem));
  GS_TRY(deliver(c, out->vals, vals, D * ab, out->mem));
  return host_wait(c);
}

gs_status gs_agg_import(gs_ctx* c, gs_agg* t, const gs_partial_batch* rows, uint64_t records) {
  GS_TRY(check_state(c, t));
  if (!rows || (rows->n && (!rows->keys || !rows->vals))) return set_error(c, GS_EINVAL, "gs_agg_import: null rows");
  if (rows->val_dtype != acc_dtype(t))
    return set_error(c, GS_EINVAL, "gs_agg_import: accumulators of dtype %d expected", acc_dtype(t));
  if (t->distinct || t->records) return set_error(c, GS_EINVAL, "gs_agg_import: the state is not empty");
  if (rows->n > (1ull << 38)) return set_error(c, GS_EINVAL, "gs_agg_import: %llu rows", (unsigned long long)rows->n);
  if (records < rows->n || (rows->n == 0 && records) || (t->mode == GS_AGG_GLOBAL && rows->n > 1))
    return set_error(c, GS_EINVAL, "gs_agg_import: %llu rows with %llu records", (unsigned long long)rows->n,
                     (unsigned long long)records);
  GS_TRY(begin_call(c));
  const uint64_t n = rows->n;
  if (n == 0) return GS_OK;
  const size_t ab = dtype_bytes(acc_dtype(t));
  if (t->mode == GS_AGG_GLOBAL) {
    GS_TRY(ensure(c, c->ct[0], 16));
    unsigned long long* w = c->ct[0].as<unsigned long long>();
    GS_HIP(hipMemsetAsync(w, 0, 16, c->stream));
    GS_HIP(hipMemcpyAsync(w, rows->vals, ab, rows->mem == GS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          c->stream));
    GS_HIP(hipMemsetAsync(w + 1, 1, 1, c->stream));   // the presence flag: 1
    GS_HIP(hipMemcpyAsync(t->meta + CT_SIDE, w, 8, hipMemcpyDeviceToDevice, c->stream));
    GS_HIP(hipMemcpyAsync(t->meta + AG_HAS, w + 1, 8, hipMemcpyDeviceToDevice, c->stream));
    GS_TRY(host_wait(c));
    t->distinct = 1;
    t->records = records;
    return GS_OK;
  }
  const int64_t* dk = rows->keys;
  const void* da = rows->vals;
  if (rows->mem != GS_MEM_DEVICE) {
    GS_TRY(ensure(c, c->ct[0], n * 8));
    GS_TRY(ensure(c, c->ct[1], n * 8));
    GS_HIP(hipMemcpyAsync(c->ct[0].p, rows->keys, n * 8, hipMemcpyHostToDevice, c->stream));
    GS_HIP(hipMemcpyAsync(c->ct[1].p, rows->vals, n * ab, hipMemcpyHostToDevice, c->stream));
    dk = c->ct[0].as<int64_t>();
    da = c->ct[1].p;
  }
  GS_TRY(ct_reserve(c, t, n, AG_META));
  // ---- the table changes from here on (a refused import clears it again: it was empty) ----
  GS_HIP(hipMemsetAsync(t->meta + CT_ERR, 0, 8, c->stream));
  if (ab == 4) hipLaunchKernelGGL(k_ag_import<uint32_t>, dim3(tab_grid_tab(n)), dim3(256), 0, c->stream, table_of(t), dk, (const uint32_t*)da, n);
  else hipLaunchKernelGGL(k_ag_import<uint64_t>, dim3(tab_grid_tab(n)), dim3(256), 0, c->stream, table_of(t), dk, (const uint64_t*)da, n);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, AG_META));
  const uint64_t err = c->host_small[8 + CT_ERR];
  if (err) {
    GS_TRY(clear_state(c, t));
    if (err & 1) return set_error(c, GS_EDEVICE, "aggregate state: the vertex table filled up");
    return set_error(c, GS_EINVAL, "gs_agg_import: a vertex comes twice");
  }
  t->distinct = c->host_small[8 + CT_DISTINCT];
  t->records = records;
  return GS_OK;
}

}  // extern "C"

// gs_distinct.hip — SimpleEdgeStream.distinct() (SimpleEdgeStream.java:305-327: keyBy(0) -> DistinctEdgeMapper
// :313-327): a device-resident edge set that outlives a batch.
//
// The key is a pair of arbitrary int64 ids (KEYED) or the target alone (INSTANCE).  128 bits fit neither the
// window sort's compact keys nor a compare-and-swap, so this operator does not go through sort -> run heads:
// it is a lock-free "first arrival wins" hash set.
//
//   log_src[] / log_dst[]  one entry per distinct edge in first-arrival order, append-only: the operator's
//                          output stream so far, and the export
//   slots[cap]             one 64-bit word each, cap a power of two, linear probing, load <= 1/2 before a
//                          batch.  EMPTY (all ones) or [tag:23 | batch:1 | index:40]: batch = 0 -> index is a
//                          log entry, batch = 1 -> index is an arrival position of the batch now running,
//                          whose key is read from the batch's own columns (device memory, unchanged during
//                          the call).  tag = other bits of the slot hash: it spares most key fetches, and is
//                          never taken as proof -- equality is decided on the full ids.
//
// One batch of n edges (all launches in the ctx stream's order, one kernel after the other):
//   reserve        room for distinct + n keys (n bounds the new ones), table and log, before any write; growth
//                  rebuilds the slot table from the log (k_ds_rebuild), the old table is not consulted
//   k_ds_claim     lane per edge i: probe to EMPTY or to an equal key.  EMPTY: CAS EMPTY -> (tag,1,i), on
//                  failure examine the word that won.  Equal log key, or equal batch key j < i: i is dropped.
//                  Equal batch key j > i: CAS (tag,1,j) -> (tag,1,i), on failure examine the word that won.
//                  A slot's key never changes once set and every retry sees a strictly smaller index, so the
//                  loop is bounded without waiting for any other lane.  held[i] = the slot, or NONE.
//   k_ds_keep      keep[i] = (slots[held[i]] == (tag,1,i)): the smallest arrival index of every new key
//   xscan          rank of every kept edge among the batch's kept edges
//   k_ds_compact   kept edge i of rank k: log[before + k] = its key, the asked-for output columns at row k,
//                  its slot -> (tag,0,before + k).  Only the winner writes its slot.
// The slot words are read and written with agent-scope atomics inside k_ds_claim (lanes of other CUs change
// them meanwhile); everything else a kernel reads was written by an earlier kernel or copy of the stream.
#include "gs_table.hpp"

namespace gs {

constexpr unsigned long long DS_NONE = ~0ull;            // held[i]: edge i holds no slot
constexpr unsigned long long DS_BATCH = 1ull << 40;
constexpr unsigned long long DS_INDEX = DS_BATCH - 1;
constexpr int DS_TAG_SHIFT = 41;
enum { DS_ERR = 0, DS_META = 2 };   // u64 words of gs_distinct::meta ([1]: padding)

struct DsTable {
  unsigned long long* slots;
  unsigned long long mask;   // cap - 1
  const int64_t* log_src;
  const int64_t* log_dst;
  unsigned long long* meta;
};

template <bool KEYED>
__device__ __forceinline__ unsigned long long ds_hash(int64_t s, int64_t d) {
  return KEYED ? ct_hash(ct_hash((unsigned long long)s) ^ ((unsigned long long)d * 0x9e3779b97f4a7c15ull))
               : ct_hash((unsigned long long)d);
}
__device__ __forceinline__ unsigned long long ds_tag(unsigned long long h) { return (h >> DS_TAG_SHIFT) << DS_TAG_SHIFT; }

// lane per edge of the batch: the slot it holds for its key (the smallest arrival index seen so far), or NONE
template <bool KEYED>
__global__ __launch_bounds__(256) void k_ds_claim(DsTable t, const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                  uint64_t n, unsigned long long* __restrict__ held) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const int64_t s = bs[i], d = bd[i];
    const unsigned long long h = ds_hash<KEYED>(s, d), tag = ds_tag(h), mine = tag | DS_BATCH | i;
    unsigned long long slot = h & t.mask, got = DS_NONE;
    bool done = false;
    for (unsigned long long probes = 0; probes <= t.mask && !done; ++probes, slot = (slot + 1) & t.mask) {
      unsigned long long w = __hip_atomic_load(&t.slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w == TAB_EMPTY) {
        w = atomicCAS(&t.slots[slot], TAB_EMPTY, mine);
        if (w == TAB_EMPTY) {
          got = slot;
          done = true;
          break;
        }
      }
      if (ds_tag(w) != tag) continue;   // another key for good
      const unsigned long long j = w & DS_INDEX;
      const bool in_batch = (w & DS_BATCH) != 0;
      const int64_t ks = KEYED ? (in_batch ? bs[j] : t.log_src[j]) : 0;
      const int64_t kd = in_batch ? bd[j] : t.log_dst[j];
      if (kd != d || (KEYED && ks != s)) continue;
      // the slot holds this lane's key, and will for the rest of the call: only its index can still fall
      done = true;
      while ((w & DS_BATCH) && (w & DS_INDEX) > i) {
        const unsigned long long prev = atomicCAS(&t.slots[slot], w, mine);
        if (prev == w) {
          got = slot;
          break;
        }
        w = prev;   // a smaller index of the same key took the slot meanwhile
      }
    }
    if (!done) atomicOr(&t.meta[DS_ERR], 1ull);
    held[i] = got;
  }
}

// after the claims have settled: edge i is kept iff its slot still names it
__global__ __launch_bounds__(256) void k_ds_keep(const unsigned long long* __restrict__ slots,
                                                 const unsigned long long* __restrict__ held, uint64_t n,
                                                 uint64_t* __restrict__ keep) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const unsigned long long sl = held[i];
    keep[i] = sl != DS_NONE && (slots[sl] & (DS_BATCH | DS_INDEX)) == (DS_BATCH | i);
  }
}

struct DsOut {
  int64_t* src;
  int64_t* dst;
  void* val;
  uint64_t* index;
};

// kept edge i of rank k = pos[i]: the log's entry before + k, output row k, and its slot now names the log entry.
// VB: bytes of a value (0: no value column asked for)
template <bool KEYED, int VB>
__global__ __launch_bounds__(256) void k_ds_compact(unsigned long long* __restrict__ slots, int64_t* __restrict__ log_src,
                                                    int64_t* __restrict__ log_dst, const int64_t* __restrict__ bs,
                                                    const int64_t* __restrict__ bd, const void* __restrict__ bv,
                                                    uint64_t n, const unsigned long long* __restrict__ held,
                                                    const uint64_t* __restrict__ keep, const uint64_t* __restrict__ pos,
                                                    uint64_t before, DsOut o) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (!keep[i]) continue;
    const uint64_t k = pos[i], e = before + k;
    const int64_t s = bs[i], d = bd[i];
    log_src[e] = s;
    log_dst[e] = d;
    if (o.src) o.src[k] = s;
    if (o.dst) o.dst[k] = d;
    if (VB == 4) ((uint32_t*)o.val)[k] = ((const uint32_t*)bv)[i];
    if (VB == 8) ((uint64_t*)o.val)[k] = ((const uint64_t*)bv)[i];
    if (o.index) o.index[k] = i;
    slots[held[i]] = ds_tag(ds_hash<KEYED>(s, d)) | e;
  }
}

__global__ __launch_bounds__(256) void k_ds_clear(unsigned long long* __restrict__ slots, uint64_t cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * 256) slots[s] = TAB_EMPTY;
}

// growth: a streaming read of the log into a cleared table (the log's keys are distinct: claims only)
template <bool KEYED>
__global__ __launch_bounds__(256) void k_ds_rebuild(DsTable t, uint64_t D) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < D; e += (uint64_t)gridDim.x * 256) {
    const unsigned long long h = ds_hash<KEYED>(t.log_src[e], t.log_dst[e]), mine = ds_tag(h) | e;
    unsigned long long slot = h & t.mask;
    bool done = false;
    for (unsigned long long probes = 0; probes <= t.mask; ++probes, slot = (slot + 1) & t.mask) {
      unsigned long long w = __hip_atomic_load(&t.slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w == TAB_EMPTY) w = atomicCAS(&t.slots[slot], TAB_EMPTY, mine);
      if (w == TAB_EMPTY) {
        done = true;
        break;
      }
    }
    if (!done) atomicOr(&t.meta[DS_ERR], 1ull);
  }
}

}  // namespace gs

using namespace gs;

struct gs_distinct {
  int device = 0;
  int mode = GS_DISTINCT_KEYED;
  unsigned long long* slots = nullptr;   // device [cap]
  int64_t* log_src = nullptr;            // device [cap / 2]
  int64_t* log_dst = nullptr;            // device [cap / 2]
  unsigned long long* meta = nullptr;    // device u64[DS_META]
  uint64_t cap = 0;                      // slots (power of two); the log holds cap / 2 entries
  uint64_t distinct = 0, records = 0, growths = 0;
  bool broken = false;                   // a batch failed on the device midway: the slots may name that batch
};

namespace {

constexpr uint64_t DS_MAX_CAP = 1ull << 40;   // 2^39 log entries: below the 40 index bits of a slot word
constexpr uint64_t DS_CHUNK = 1ull << 31;     // gs_distinct_import: rows per pass

DsTable table_of(const gs_distinct* t) { return DsTable{t->slots, t->cap - 1, t->log_src, t->log_dst, t->meta}; }

void free_tables(unsigned long long* slots, int64_t* ls, int64_t* ld) {
  if (slots) hipFree(slots);
  if (ls) hipFree(ls);
  if (ld) hipFree(ld);
}

// a cleared table of cap slots and an (unwritten) log of cap / 2 entries
gs_status alloc_tables(gs_ctx* c, uint64_t cap, unsigned long long** slots, int64_t** ls, int64_t** ld) {
  *slots = nullptr;
  *ls = *ld = nullptr;
  if (cap > DS_MAX_CAP || hipMalloc((void**)slots, cap * 8) != hipSuccess ||
      hipMalloc((void**)ls, cap / 2 * 8) != hipSuccess || hipMalloc((void**)ld, cap / 2 * 8) != hipSuccess) {
    (void)hipGetLastError();
    free_tables(*slots, *ls, *ld);
    *slots = nullptr;
    *ls = *ld = nullptr;
    return set_error(c, GS_ENOMEM, "distinct state: an edge table of %llu slots does not fit", (unsigned long long)cap);
  }
  hipLaunchKernelGGL(k_ds_clear, dim3(tab_grid(cap)), dim3(256), 0, c->stream, *slots, cap);
  const gs_status st = hip_check(c, hipGetLastError(), "k_ds_clear");
  if (st != GS_OK) {
    free_tables(*slots, *ls, *ld);
    *slots = nullptr;
    *ls = *ld = nullptr;
  }
  return st;
}

// room for `need` distinct edges at load <= 1/2, table and log: grow by doubling (allocate, copy the log,
// rebuild the slots from it, swap).  On any failure the old state stays as it was.
gs_status reserve(gs_ctx* c, gs_distinct* t, uint64_t need) {
  if (need <= t->cap / 2) return GS_OK;
  uint64_t cap, doublings;
  if (!tab_plan_growth(t->cap, need, DS_MAX_CAP, &cap, &doublings))
    return set_error(c, GS_ENOMEM, "distinct state: %llu edges", (unsigned long long)need);
  unsigned long long* ns;
  int64_t *nls, *nld;
  GS_TRY(alloc_tables(c, cap, &ns, &nls, &nld));
  gs_status st = GS_OK;
  const uint64_t D = t->distinct;
  if (D) {
    st = hip_check(c, hipMemcpyAsync(nls, t->log_src, D * 8, hipMemcpyDeviceToDevice, c->stream), "log copy");
    if (st == GS_OK) st = hip_check(c, hipMemcpyAsync(nld, t->log_dst, D * 8, hipMemcpyDeviceToDevice, c->stream), "log copy");
    if (st == GS_OK) {
      const DsTable nt{ns, cap - 1, nls, nld, t->meta};
      if (t->mode == GS_DISTINCT_KEYED)
        hipLaunchKernelGGL(k_ds_rebuild<true>, dim3(tab_grid(D)), dim3(256), 0, c->stream, nt, D);
      else
        hipLaunchKernelGGL(k_ds_rebuild<false>, dim3(tab_grid(D)), dim3(256), 0, c->stream, nt, D);
      st = hip_check(c, hipGetLastError(), "k_ds_rebuild");
    }
  }
  if (st == GS_OK) st = tab_read_meta(c, t->meta, DS_META);
  if (st == GS_OK && c->host_small[8 + DS_ERR]) st = set_error(c, GS_EDEVICE, "distinct state: rebuild failed");
  if (st != GS_OK) {
    free_tables(ns, nls, nld);
    return st;
  }
  free_tables(t->slots, t->log_src, t->log_dst);
  t->slots = ns;
  t->log_src = nls;
  t->log_dst = nld;
  t->cap = cap;
  t->growths += doublings;
  return GS_OK;
}

gs_status check_state(gs_ctx* c, const gs_distinct* t) {
  if (!c) return GS_EINVAL;
  if (!t) return set_error(c, GS_EINVAL, "null distinct state");
  if (t->device != c->device)
    return set_error(c, GS_EINVAL, "distinct state lives on device %d, the ctx on device %d", t->device, c->device);
  if (t->broken) return set_error(c, GS_EDEVICE, "distinct state: an earlier batch failed on the device");
  return GS_OK;
}

template <bool KEYED>
void launch_compact(gs_ctx* c, gs_distinct* t, const int64_t* src, const int64_t* dst, const void* val, int vb, uint64_t n,
                    const unsigned long long* held, const uint64_t* keep, const uint64_t* pos, DsOut o) {
  const dim3 g(tab_grid(n)), b(256);
  if (vb == 4)
    hipLaunchKernelGGL((k_ds_compact<KEYED, 4>), g, b, 0, c->stream, t->slots, t->log_src, t->log_dst, src, dst, val, n, held,
                       keep, pos, t->distinct, o);
  else if (vb == 8)
    hipLaunchKernelGGL((k_ds_compact<KEYED, 8>), g, b, 0, c->stream, t->slots, t->log_src, t->log_dst, src, dst, val, n, held,
                       keep, pos, t->distinct, o);
  else
    hipLaunchKernelGGL((k_ds_compact<KEYED, 0>), g, b, 0, c->stream, t->slots, t->log_src, t->log_dst, src, dst, val, n, held,
                       keep, pos, t->distinct, o);
}

// the scratch columns of a pass of n edges
gs_status ensure_scratch(gs_ctx* c, uint64_t n) {
  GS_TRY(ensure(c, c->ct[0], n * 8));
  GS_TRY(ensure(c, c->ct[3], n * 8));
  return ensure(c, c->ct[4], (n + 1) * 8);
}

// n staged edges (device columns) through the state, room reserved by the caller: the kept edges' columns
// into o (device pointers or NULL), their number into *kept.  vb: bytes of a value when o.val is set.
gs_status run_batch(gs_ctx* c, gs_distinct* t, const int64_t* src, const int64_t* dst, const void* val, int vb, uint64_t n,
                    DsOut o, uint64_t* kept) {
  unsigned long long* held = c->ct[0].as<unsigned long long>();
  uint64_t* keep = c->ct[3].as<uint64_t>();
  uint64_t* pos = c->ct[4].as<uint64_t>();
  const bool keyed = t->mode == GS_DISTINCT_KEYED;
  const dim3 g(tab_grid(n)), b(256);
  // ---- the table changes from here on ----
  t->broken = true;
  if (keyed) hipLaunchKernelGGL(k_ds_claim<true>, g, b, 0, c->stream, table_of(t), src, dst, n, held);
  else hipLaunchKernelGGL(k_ds_claim<false>, g, b, 0, c->stream, table_of(t), src, dst, n, held);
  GS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_ds_keep, g, b, 0, c->stream, t->slots, held, n, keep);
  GS_HIP(hipGetLastError());
  GS_TRY(xscan(c, keep, n, pos));
  if (keyed) launch_compact<true>(c, t, src, dst, val, o.val ? vb : 0, n, held, keep, pos, o);
  else launch_compact<false>(c, t, src, dst, val, o.val ? vb : 0, n, held, keep, pos, o);
  GS_HIP(hipGetLastError());
  GS_HIP(hipMemcpyAsync(c->host_small + 8 + DS_META, pos + n, 8, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(tab_read_meta(c, t->meta, DS_META));
  if (c->host_small[8 + DS_ERR]) return set_error(c, GS_EDEVICE, "distinct state: the edge table filled up");
  *kept = c->host_small[8 + DS_META];
  if (*kept > n) return set_error(c, GS_EDEVICE, "distinct state: %llu kept of %llu edges", (unsigned long long)*kept,
                                  (unsigned long long)n);
  t->distinct += *kept;
  t->records += n;
  t->broken = false;
  return GS_OK;
}

}  // namespace

extern "C" {

gs_status gs_distinct_create(gs_ctx* c, int32_t mode, uint64_t reserve_edges, gs_distinct** out) {
  if (!c) return GS_EINVAL;
  if (!out) return set_error(c, GS_EINVAL, "gs_distinct_create: null argument");
  *out = nullptr;
  if (mode != GS_DISTINCT_KEYED && mode != GS_DISTINCT_INSTANCE)
    return set_error(c, GS_EINVAL, "gs_distinct_create: bad mode %d", mode);
  if (reserve_edges > DS_MAX_CAP / 2)
    return set_error(c, GS_ENOMEM, "gs_distinct_create: %llu edges", (unsigned long long)reserve_edges);
  (void)hipGetLastError();
  GS_HIP(hipSetDevice(c->device));
  gs_distinct* t = new (std::nothrow) gs_distinct();
  if (!t) return set_error(c, GS_ENOMEM, "gs_distinct_create");
  t->device = c->device;
  t->mode = mode;
  t->cap = 64;
  while (t->cap / 2 < reserve_edges) t->cap *= 2;
  gs_status st = alloc_tables(c, t->cap, &t->slots, &t->log_src, &t->log_dst);
  if (st == GS_OK && hipMalloc((void**)&t->meta, DS_META * 8) != hipSuccess) {
    (void)hipGetLastError();
    st = set_error(c, GS_ENOMEM, "gs_distinct_create: state words");
  }
  if (st == GS_OK) st = hip_check(c, hipMemsetAsync(t->meta, 0, DS_META * 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) st = host_wait(c);
  if (st != GS_OK) {
    gs_distinct_destroy(t);
    return st;
  }
  *out = t;
  return GS_OK;
}

void gs_distinct_destroy(gs_distinct* t) {
  if (!t) return;
  hipSetDevice(t->device);
  free_tables(t->slots, t->log_src, t->log_dst);
  if (t->meta) hipFree(t->meta);
  delete t;
}

gs_status gs_distinct_size(const gs_distinct* t, uint64_t* distinct_edges, uint64_t* records) {
  if (!t) return GS_EINVAL;
  if (distinct_edges) *distinct_edges = t->distinct;
  if (records) *records = t->records;
  return GS_OK;
}

gs_status gs_distinct_capacity(const gs_distinct* t, uint64_t* slots, uint64_t* growths) {
  if (!t) return GS_EINVAL;
  if (slots) *slots = t->cap;
  if (growths) *growths = t->growths;
  return GS_OK;
}

gs_status gs_distinct_edges(gs_ctx* c, gs_distinct* t, const gs_edge_batch* b, gs_edge_out* out) {
  GS_TRY(check_state(c, t));
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (!out || !out->n_out) return set_error(c, GS_EINVAL, "bad gs_edge_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_edge_out.mem %d", out->mem);
  const size_t vb = dtype_bytes(b->val_dtype);
  if (out->val && (vb == 0 || (b->n && !b->val)))
    return set_error(c, GS_EINVAL, "gs_distinct_edges: a value column asked of a batch without values");
  const uint64_t n = b->n;
  const bool any = out->src || out->dst || out->val || out->index;
  *out->n_out = n;
  if (any && out->capacity < n) return set_error(c, GS_ECAPACITY, "output needs room for %llu edges", (unsigned long long)n);
  GS_TRY(begin_call(c));
  *out->n_out = 0;
  if (n == 0) return GS_OK;
  // everything that can fail for want of memory comes before the table changes
  GS_TRY(ensure_scratch(c, n));
  const bool direct = out->mem == GS_MEM_DEVICE;
  DsOut o{out->src, out->dst, out->val, out->index};
  if (!direct) {
    if (out->src) {
      GS_TRY(ensure(c, c->out_keys, n * 8));
      o.src = c->out_keys.as<int64_t>();
    }
    if (out->dst) {
      GS_TRY(ensure(c, c->out_a, n * 8));
      o.dst = c->out_a.as<int64_t>();
    }
    if (out->val) {
      GS_TRY(ensure(c, c->out_b, n * vb));
      o.val = c->out_b.p;
    }
    if (out->index) {
      GS_TRY(ensure(c, c->aux, n * 8));
      o.index = c->aux.as<uint64_t>();
    }
  }
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, out->val != nullptr));
  GS_TRY(reserve(c, t, t->distinct + n));
  uint64_t kept = 0;
  GS_TRY(run_batch(c, t, src, dst, val, (int)vb, n, o, &kept));
  *out->n_out = kept;
  if (!direct && kept && any) {
    if (out->src) GS_TRY(deliver(c, out->src, o.src, kept * 8, out->mem));
    if (out->dst) GS_TRY(deliver(c, out->dst, o.dst, kept * 8, out->mem));
    if (out->val) GS_TRY(deliver(c, out->val, o.val, kept * vb, out->mem));
    if (out->index) GS_TRY(deliver(c, out->index, o.index, kept * 8, out->mem));
    GS_TRY(host_wait(c));
  }
  return GS_OK;
}

gs_status gs_distinct_export(gs_ctx* c, const gs_distinct* t, gs_edge_out* out) {
  GS_TRY(check_state(c, t));
  if (!out || !out->n_out) return set_error(c, GS_EINVAL, "bad gs_edge_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_edge_out.mem %d", out->mem);
  if (out->val || out->index) return set_error(c, GS_EINVAL, "gs_distinct_export writes src and dst only");
  const uint64_t D = t->distinct;
  *out->n_out = D;
  if (out->capacity < D) return set_error(c, GS_ECAPACITY, "output needs %llu edges", (unsigned long long)D);
  GS_TRY(begin_call(c));
  if (D == 0) return GS_OK;
  if (out->src) GS_TRY(deliver(c, out->src, t->log_src, D * 8, out->mem));
  if (out->dst) GS_TRY(deliver(c, out->dst, t->log_dst, D * 8, out->mem));
  return out->mem == GS_MEM_DEVICE ? GS_OK : host_wait(c);
}

gs_status gs_distinct_import(gs_ctx* c, gs_distinct* t, const gs_edge_batch* rows) {
  GS_TRY(check_state(c, t));
  if (!rows || (rows->n && (!rows->src || !rows->dst))) return set_error(c, GS_EINVAL, "gs_distinct_import: null rows");
  if (rows->mem != GS_MEM_HOST && rows->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "gs_distinct_import: bad mem");
  if (t->distinct || t->records) return set_error(c, GS_EINVAL, "gs_distinct_import: the state is not empty");
  if (rows->n > DS_MAX_CAP / 2) return set_error(c, GS_EINVAL, "gs_distinct_import: %llu rows", (unsigned long long)rows->n);
  GS_TRY(begin_call(c));
  const uint64_t n = rows->n;
  if (n == 0) return GS_OK;
  GS_TRY(ensure_scratch(c, std::min(n, DS_CHUNK)));
  if (rows->mem != GS_MEM_DEVICE) {
    GS_TRY(ensure(c, c->in_src, std::min(n, DS_CHUNK) * 8));
    GS_TRY(ensure(c, c->in_dst, std::min(n, DS_CHUNK) * 8));
  }
  GS_TRY(reserve(c, t, n));
  for (uint64_t a = 0; a < n; a += DS_CHUNK) {
    gs_edge_batch part = *rows;
    part.src += a;
    part.dst += a;
    part.val = nullptr;
    part.val_dtype = GS_NONE;
    part.n = std::min(DS_CHUNK, n - a);
    const int64_t *src, *dst;
    const void* val;
    GS_TRY(stage_batch(c, &part, &src, &dst, &val, false));
    uint64_t kept = 0;
    GS_TRY(run_batch(c, t, src, dst, nullptr, 0, part.n, DsOut{nullptr, nullptr, nullptr, nullptr}, &kept));
  }
  t->records = t->distinct;
  return GS_OK;
}

}  // extern "C"

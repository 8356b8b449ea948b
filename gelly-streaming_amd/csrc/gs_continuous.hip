// gs_continuous.hip — the continuous (non-windowed) operators of SimpleEdgeStream: state that outlives a batch.
//
//   gs_cont_degrees   <- getDegrees / getInDegrees / getOutDegrees (SimpleEdgeStream.java:416-442:
//                        DegreeTypeSeparator :444-463 -> keyBy(0) -> DegreeMapFunction :465-482)
//   gs_cont_vertices  <- getVertices (:119-125: EmitSrcAndTarget :185-192 -> keyBy(0) -> FilterDistinctVertices
//                        :194-209) and numberOfVertices (:370-387 through globalAggregate :509-539)
//
// The reference keeps a HashMap<K, Long> (a HashSet<K>) per operator and emits one record per input record
// forever.  Here a gs_cont owns an open-addressing table in HBM -- full int64 vertex id -> 64-bit record
// count -- that persists across calls; one call takes a micro-batch of the stream:
//
//   sort_window(PAY_IDX)   stable sort of the direction-expanded records, payload = arrival index r
//   launch_rbk<CountOp>    run heads of the sorted keys: full ids keys[U], offsets[U + 1]
//   k_ct_upsert            one lane per run (the batch's keys are distinct here, so lanes contend for slots,
//                          never for a key's count): probe, claim an empty slot with a 64-bit CAS,
//                          base[u] = count before the batch, count += run length
//   k_ct_emit              per sorted position p of run u with r = rec[p]:
//                          out_degree[r] = base[u] + (p - offsets[u]) + 1
//   k_ct_expand_all        out_vertex[r] = the record's own key, straight from the columns (a copy for IN / OUT)
//   (vertices)             k_ct_upsert flags rec[offsets[u]] of every run with base 0 (stability: the run's
//                          earliest arrival), xscan over arrival positions, k_ct_compact
//
// The output of one state depends only on the stream, not on how it is cut into batches.
// Table: slots[cap] of 16 bytes (id, count), so a hit touches one line; cap a power of two, linear probing
// from a murmur3 finaliser, load <= 1/2 (grown by doubling + re-insert before a batch whose U distinct keys
// could exceed it).  An empty slot holds TAB_EMPTY (the bits of vertex -1); vertex -1 itself lives in a side
// slot (meta[CT_SIDE], present iff its count != 0).
// Keys are claimed through gs_table.hpp's tab_claim; counts are touched by their key's one lane.
// The table, its growth and the batch's runs are gs_ctable.hpp's, shared with gs_aggregate.hip.
#include "gs_ctable.hpp"

namespace gs {

constexpr int CT_META = 4;   // u64 words of gs_cont::meta (gs_ctable.hpp names them)
constexpr int CT_EMIT_TILE = 2048;

// lane per run u of the batch: base[u] = the vertex's count before the batch, count += the run's length.
// FLAG_NEW: flags[rec[head]] = 1 for a vertex never seen before (its earliest arrival in the batch).
template <bool FLAG_NEW>
__global__ __launch_bounds__(256) void k_ct_upsert(CtTable t, const int64_t* __restrict__ run_keys,
                                                   const uint64_t* __restrict__ offs, uint32_t U,
                                                   uint64_t* __restrict__ base, const uint32_t* __restrict__ rec,
                                                   uint64_t* __restrict__ flags) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long n_fresh = 0;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u < U; u += (uint64_t)gridDim.x * 256) {
    bool fresh = false;
    const unsigned long long id = (unsigned long long)run_keys[u];
    const uint64_t h = offs[u], len = offs[u + 1] - h;
    uint64_t b = 0;
    if (id == TAB_EMPTY) {
      b = t.meta[CT_SIDE];
      t.meta[CT_SIDE] = b + len;
      fresh = b == 0;
    } else {
      const unsigned long long s = ct_slot(t, id, &fresh);
      if (s == ~0ull) {
        fresh = false;
        atomicOr(&t.meta[CT_ERR], 1ull);
      } else {
        b = fresh ? 0 : t.slots[2 * s + 1];
        t.slots[2 * s + 1] = b + len;
      }
    }
    base[u] = b;
    if (FLAG_NEW && fresh) flags[rec[h]] = 1;
    n_fresh += fresh;
  }
  block_add(&t.meta[CT_DISTINCT], n_fresh, s_part);
}

// block per tile of sorted positions: the tile's first and last run by a search over all offsets, then each
// position's run by a search between the two (a hub's run spans many tiles: the search is then empty)
__global__ __launch_bounds__(256) void k_ct_emit(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ base,
                                                 uint32_t U, const uint32_t* __restrict__ rec, uint32_t R,
                                                 int64_t* __restrict__ out_d) {
  __shared__ uint32_t s_lo, s_hi;
  const uint64_t t0 = (uint64_t)blockIdx.x * CT_EMIT_TILE, t1 = min((uint64_t)R, t0 + CT_EMIT_TILE);
  if (t0 >= t1) return;
  if (threadIdx.x == 0) s_lo = ct_run_of(offs, 0, U - 1, t0);
  if (threadIdx.x == 64) s_hi = ct_run_of(offs, 0, U - 1, t1 - 1);
  __syncthreads();
  const uint32_t lo = s_lo, hi = s_hi;
  for (uint64_t p = t0 + threadIdx.x; p < t1; p += 256) {
    const uint32_t u = ct_run_of(offs, lo, hi, p);
    out_d[rec[p]] = (int64_t)(base[u] + (p - offs[u]) + 1);
  }
}

// arrival position r flagged as a first occurrence -> output row pos[r]: (vertex, running numberOfVertices)
__global__ __launch_bounds__(256) void k_ct_compact(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ pos,
                                                    uint32_t R, const int64_t* __restrict__ src,
                                                    const int64_t* __restrict__ dst, uint64_t distinct_before,
                                                    int64_t* __restrict__ out_v, int64_t* __restrict__ out_c) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
    if (!flags[r]) continue;
    const uint64_t k = pos[r];
    out_v[k] = (r & 1) ? dst[r >> 1] : src[r >> 1];   // ALL: record 2i = src[i], 2i + 1 = dst[i]
    out_c[k] = (int64_t)(distinct_before + k + 1);
  }
}

// checkpoint: the occupied slots as (id with the sign bit flipped, count) rows in any order; n rows expected
__global__ __launch_bounds__(256) void k_ct_dump(CtTable t, unsigned long long* __restrict__ ok,
                                                 unsigned long long* __restrict__ oc, uint64_t n) {
  const uint64_t cap = t.mask + 1, stride = (uint64_t)gridDim.x * 256;
  if (blockIdx.x == 0 && threadIdx.x == 0 && t.meta[CT_SIDE]) {
    const unsigned long long i = atomicAdd(&t.meta[CT_SUM], 1ull);
    if (i < n) {
      ok[i] = TAB_EMPTY ^ TAB_SIGN;
      oc[i] = t.meta[CT_SIDE];
    }
  }
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 < cap; s0 += stride) {
    const uint64_t s = s0 + threadIdx.x;
    const unsigned long long id = s < cap ? t.slots[2 * s] : TAB_EMPTY;
    const bool occ = id != TAB_EMPTY;
    const unsigned long long i = wave_compact_base(occ, &t.meta[CT_SUM]);
    if (occ && i < n) {
      ok[i] = id ^ TAB_SIGN;
      oc[i] = t.slots[2 * s + 1];
    }
  }
}

// restore: any count < 1 sets the error word (checked before the table is touched)
__global__ __launch_bounds__(256) void k_ct_check_counts(const int64_t* __restrict__ counts, uint64_t n,
                                                         unsigned long long* __restrict__ err) {
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) bad |= counts[i] < 1;
  if (bad) atomicOr(err, 2ull);
}

// restore: lane per row (rows of one vertex add up); meta[CT_SUM] += the counts
__global__ __launch_bounds__(256) void k_ct_import(CtTable t, const int64_t* __restrict__ keys,
                                                   const int64_t* __restrict__ counts, uint64_t n) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long n_fresh = 0, sum = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    bool fresh = false;
    const unsigned long long id = (unsigned long long)keys[i];
    const unsigned long long cnt = (unsigned long long)counts[i];
    sum += cnt;
    if (id == TAB_EMPTY) {
      fresh = atomicAdd(&t.meta[CT_SIDE], cnt) == 0;
    } else {
      const unsigned long long s = ct_slot(t, id, &fresh);
      if (s == ~0ull) {
        fresh = false;
        atomicOr(&t.meta[CT_ERR], 1ull);
      } else {
        atomicAdd(&t.slots[2 * s + 1], cnt);
      }
    }
    n_fresh += fresh;
  }
  block_add(&t.meta[CT_DISTINCT], n_fresh, s_part);
  block_add(&t.meta[CT_SUM], sum, s_part);
}

}  // namespace gs

using namespace gs;

struct gs_cont {
  int device = 0;
  unsigned long long* slots = nullptr;  // device [cap][2]
  unsigned long long* meta = nullptr;   // device u64[CT_META]
  uint64_t cap = 0;                     // slots (power of two)
  uint64_t distinct = 0, records = 0, growths = 0;
};

namespace {

CtTable table_of(const gs_cont* t) { return CtTable{t->slots, t->cap - 1, t->meta}; }

gs_status check_state(gs_ctx* c, const gs_cont* t) {
  if (!c) return GS_EINVAL;
  if (!t) return set_error(c, GS_EINVAL, "null continuous state");
  if (t->device != c->device)
    return set_error(c, GS_EINVAL, "continuous state lives on device %d, the ctx on device %d", t->device, c->device);
  return GS_OK;
}

// one micro-batch through the state: per-record degrees, or the newly seen vertices
gs_status cont_batch(gs_ctx* c, gs_cont* t, const gs_edge_batch* b, int32_t dir, gs_vertex_out* out, bool vertices) {
  GS_TRY(check_state(c, t));
  GS_TRY(check_batch(c, b, dir));
  if (!out || !out->n_out || (out->capacity && (!out->keys || !out->vals)))
    return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  const uint64_t R = dir == GS_DIR_ALL ? 2 * b->n : b->n;
  *out->n_out = R;
  if (out->capacity < R) return set_error(c, GS_ECAPACITY, "output needs room for %llu records", (unsigned long long)R);
  GS_TRY(begin_call(c));
  *out->n_out = 0;
  if (R == 0) return GS_OK;
  // everything that can fail for want of memory comes before the table changes
  GS_TRY(ensure(c, c->ct[0], R * 8));
  GS_TRY(ensure(c, c->ct[1], (R + 1) * 8));
  GS_TRY(ensure(c, c->ct[2], R * 8));
  if (vertices) {
    GS_TRY(ensure(c, c->ct[3], R * 8));
    GS_TRY(ensure(c, c->ct[4], (R + 1) * 8));
  }
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t *ov = out->keys, *ox = (int64_t*)out->vals;
  if (!direct) {
    GS_TRY(ensure(c, c->out_keys, R * 8));
    GS_TRY(ensure(c, c->out_a, R * 8));
    ov = c->out_keys.as<int64_t>();
    ox = c->out_a.as<int64_t>();
  }
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, false));
  Sorted s;
  int64_t* rk = c->ct[0].as<int64_t>();
  uint64_t* offs = c->ct[1].as<uint64_t>();
  uint64_t* base = c->ct[2].as<uint64_t>();
  uint64_t U = 0;
  GS_TRY(ct_sorted_runs(c, src, dst, b->n, dir, R, &s, rk, offs, &U));
  // the batch brings at most U new vertices: room for them at load <= 1/2, or the call ends here
  GS_TRY(ct_reserve(c, t, t->distinct + U, CT_META));
  const uint32_t* rec = (const uint32_t*)s.vals;
  const uint64_t before = t->distinct;
  // ---- the table changes from here on ----
  if (vertices) {
    uint64_t* flags = c->ct[3].as<uint64_t>();
    uint64_t* pos = c->ct[4].as<uint64_t>();
    GS_HIP(hipMemsetAsync(flags, 0, R * 8, c->stream));
    hipLaunchKernelGGL(k_ct_upsert<true>, dim3(tab_grid_tab(U)), dim3(256), 0, c->stream, table_of(t), rk, offs, (uint32_t)U,
                       base, rec, flags);
    GS_HIP(hipGetLastError());
    GS_TRY(xscan(c, flags, R, pos));
    hipLaunchKernelGGL(k_ct_compact, dim3(tab_grid(R)), dim3(256), 0, c->stream, flags, pos, (uint32_t)R, src, dst, before,
                       ov, ox);
    GS_HIP(hipGetLastError());
  } else {
    hipLaunchKernelGGL(k_ct_upsert<false>, dim3(tab_grid_tab(U)), dim3(256), 0, c->stream, table_of(t), rk, offs, (uint32_t)U,
                       base, rec, (uint64_t*)nullptr);
    GS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ct_emit, dim3((unsigned)((R + CT_EMIT_TILE - 1) / CT_EMIT_TILE)), dim3(256), 0, c->stream, offs,
                       base, (uint32_t)U, rec, (uint32_t)R, ox);
    GS_HIP(hipGetLastError());
    if (dir == GS_DIR_ALL) {
      hipLaunchKernelGGL(k_ct_expand_all, dim3(tab_grid(R)), dim3(256), 0, c->stream, src, dst, b->n, ov);
      GS_HIP(hipGetLastError());
    } else {
      GS_HIP(hipMemcpyAsync(ov, dir == GS_DIR_OUT ? src : dst, R * 8, hipMemcpyDeviceToDevice, c->stream));
    }
  }
  GS_TRY(tab_read_meta(c, t->meta, CT_META));
  if (c->host_small[8 + CT_ERR]) return set_error(c, GS_EDEVICE, "continuous state: the vertex table filled up");
  t->distinct = c->host_small[8 + CT_DISTINCT];
  t->records += R;
  const uint64_t rows = vertices ? t->distinct - before : R;
  *out->n_out = rows;
  if (!direct && rows) {
    GS_TRY(deliver(c, out->keys, ov, rows * 8, out->mem));
    GS_TRY(deliver(c, out->vals, ox, rows * 8, out->mem));
    GS_TRY(host_wait(c));
  }
  return GS_OK;
}

}  // namespace

extern "C" {

gs_status gs_cont_create(gs_ctx* c, uint64_t reserve_vertices, gs_cont** out) {
  if (!c) return GS_EINVAL;
  if (!out) return set_error(c, GS_EINVAL, "gs_cont_create: null argument");
  *out = nullptr;
  if (reserve_vertices > (1ull << 38)) return set_error(c, GS_ENOMEM, "gs_cont_create: %llu vertices",
                                                       (unsigned long long)reserve_vertices);
  (void)hipGetLastError();
  GS_HIP(hipSetDevice(c->device));
  gs_cont* t = new (std::nothrow) gs_cont();
  if (!t) return set_error(c, GS_ENOMEM, "gs_cont_create");
  t->device = c->device;
  t->cap = 64;
  while (t->cap / 2 < reserve_vertices) t->cap *= 2;
  gs_status st = ct_alloc_table(c, t->cap, &t->slots);
  if (st == GS_OK && hipMalloc((void**)&t->meta, CT_META * 8) != hipSuccess) {
    (void)hipGetLastError();
    st = set_error(c, GS_ENOMEM, "gs_cont_create: state words");
  }
  if (st == GS_OK) st = hip_check(c, hipMemsetAsync(t->meta, 0, CT_META * 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) st = host_wait(c);
  if (st != GS_OK) {
    gs_cont_destroy(t);
    return st;
  }
  *out = t;
  return GS_OK;
}

void gs_cont_destroy(gs_cont* t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->slots) hipFree(t->slots);
  if (t->meta) hipFree(t->meta);
  delete t;
}

gs_status gs_cont_size(const gs_cont* t, uint64_t* distinct_vertices, uint64_t* records) {
  if (!t) return GS_EINVAL;
  if (distinct_vertices) *distinct_vertices = t->distinct;
  if (records) *records = t->records;
  return GS_OK;
}

gs_status gs_cont_capacity(const gs_cont* t, uint64_t* slots, uint64_t* growths) {
  if (!t) return GS_EINVAL;
  if (slots) *slots = t->cap;
  if (growths) *growths = t->growths;
  return GS_OK;
}

gs_status gs_cont_degrees(gs_ctx* c, gs_cont* t, const gs_edge_batch* b, int32_t dir, gs_vertex_out* out) {
  return cont_batch(c, t, b, dir, out, false);
}

gs_status gs_cont_vertices(gs_ctx* c, gs_cont* t, const gs_edge_batch* b, gs_vertex_out* out) {
  return cont_batch(c, t, b, GS_DIR_ALL, out, true);
}

gs_status gs_cont_export(gs_ctx* c, const gs_cont* t, gs_vertex_out* out) {
  GS_TRY(check_state(c, t));
  if (!out || !out->n_out || (out->capacity && (!out->keys || !out->vals)))
    return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  const uint64_t D = t->distinct;
  *out->n_out = D;
  if (out->capacity < D) return set_error(c, GS_ECAPACITY, "output needs %llu vertices", (unsigned long long)D);
  if (D >= (1ull << 32)) return set_error(c, GS_EUNSUPPORTED, "export of %llu vertices (limit 2^32 - 1)", (unsigned long long)D);
  GS_TRY(begin_call(c));
  if (D == 0) return GS_OK;
  GS_TRY(ensure(c, c->ct[0], D * 8));
  GS_TRY(ensure(c, c->ct[1], D * 8));
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t* ok = out->keys;
  if (!direct) {
    GS_TRY(ensure(c, c->out_keys, D * 8));
    ok = c->out_keys.as<int64_t>();
  }
  unsigned long long* dk = c->ct[0].as<unsigned long long>();
  unsigned long long* dc = c->ct[1].as<unsigned long long>();
  GS_HIP(hipMemsetAsync(t->meta + CT_SUM, 0, 8, c->stream));
  hipLaunchKernelGGL(k_ct_dump, dim3(tab_grid(t->cap)), dim3(256), 0, c->stream, table_of(t), dk, dc, D);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, CT_META));
  if (c->host_small[8 + CT_SUM] != D)
    return set_error(c, GS_EDEVICE, "continuous state: %llu entries in the table, %llu expected",
                     (unsigned long long)c->host_small[8 + CT_SUM], (unsigned long long)D);
  // ascending signed ids = ascending (id ^ sign bit) as unsigned
  Sorted s;
  GS_TRY(sort_buffer(c, (const uint64_t*)dk, dc, D, &s, 64, 8));
  if (s.wide)
    hipLaunchKernelGGL(k_tab_unkey<uint64_t>, dim3(tab_grid(D)), dim3(256), 0, c->stream, (const uint64_t*)s.keys,
                       s.key_xor, D, ok);
  else
    hipLaunchKernelGGL(k_tab_unkey<uint32_t>, dim3(tab_grid(D)), dim3(256), 0, c->stream, (const uint32_t*)s.keys,
                       s.key_xor, D, ok);
  GS_HIP(hipGetLastError());
  GS_TRY(deliver(c, out->keys, ok, D * 8, out->mem));
  GS_TRY(deliver(c, out->vals, s.vals, D * 8, out->mem));
  return host_wait(c);
}

gs_status gs_cont_import(gs_ctx* c, gs_cont* t, const gs_partial_batch* rows) {
  GS_TRY(check_state(c, t));
  if (!rows || (rows->n && (!rows->keys || !rows->vals))) return set_error(c, GS_EINVAL, "gs_cont_import: null rows");
  if (rows->val_dtype != GS_I64) return set_error(c, GS_EINVAL, "gs_cont_import: counts are I64");
  if (t->distinct || t->records) return set_error(c, GS_EINVAL, "gs_cont_import: the state is not empty");
  if (rows->n > (1ull << 38)) return set_error(c, GS_EINVAL, "gs_cont_import: %llu rows", (unsigned long long)rows->n);
  GS_TRY(begin_call(c));
  const uint64_t n = rows->n;
  if (n == 0) return GS_OK;
  const int64_t* dk = rows->keys;
  const int64_t* dc = (const int64_t*)rows->vals;
  if (rows->mem != GS_MEM_DEVICE) {
    GS_TRY(ensure(c, c->ct[0], n * 8));
    GS_TRY(ensure(c, c->ct[1], n * 8));
    GS_HIP(hipMemcpyAsync(c->ct[0].p, rows->keys, n * 8, hipMemcpyHostToDevice, c->stream));
    GS_HIP(hipMemcpyAsync(c->ct[1].p, rows->vals, n * 8, hipMemcpyHostToDevice, c->stream));
    dk = c->ct[0].as<int64_t>();
    dc = c->ct[1].as<int64_t>();
  }
  GS_HIP(hipMemsetAsync(t->meta + CT_ERR, 0, 16, c->stream));   // error word, count sum
  hipLaunchKernelGGL(k_ct_check_counts, dim3(tab_grid(n)), dim3(256), 0, c->stream, dc, n, t->meta + CT_ERR);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, CT_META));
  if (c->host_small[8 + CT_ERR]) {
    GS_HIP(hipMemsetAsync(t->meta + CT_ERR, 0, 8, c->stream));
    return set_error(c, GS_EINVAL, "gs_cont_import: every count must be at least 1");
  }
  GS_TRY(ct_reserve(c, t, n, CT_META));
  // ---- the table changes from here on ----
  hipLaunchKernelGGL(k_ct_import, dim3(tab_grid_tab(n)), dim3(256), 0, c->stream, table_of(t), dk, dc, n);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, CT_META));
  if (c->host_small[8 + CT_ERR]) return set_error(c, GS_EDEVICE, "continuous state: the vertex table filled up");
  t->distinct = c->host_small[8 + CT_DISTINCT];
  t->records = c->host_small[8 + CT_SUM];
  return GS_OK;
}

}  // extern "C"

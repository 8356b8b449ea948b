// gs_ctable.hpp — the vertex table of the continuous operators: what gs_continuous.hip (vertex -> record count)
// and gs_aggregate.hip (vertex -> running accumulator) share on top of gs_table.hpp.
//
// Table: slots[cap] of 16 bytes (id, one 64-bit word), so a hit touches one line; cap a power of two, linear
// probing from a murmur3 finaliser, load <= 1/2 (grown by doubling + re-insert before a batch whose U distinct keys
// could exceed it).  An empty slot holds TAB_EMPTY (the bits of vertex -1); vertex -1 itself lives in a side
// slot (meta[CT_SIDE]).
// A batch reaches the table as runs: sort_window(PAY_IDX) of the direction-expanded records (stable, payload =
// arrival index), then the run heads -- full ids keys[U], offsets[U + 1] (ct_sorted_runs).
#pragma once
#include "gs_table.hpp"

namespace gs {

// u64 words of a state's meta block that both operators use the same way
enum { CT_DISTINCT = 0, CT_SIDE = 1, CT_ERR = 2, CT_SUM = 3 };

struct CtTable {
  unsigned long long* slots;   // [cap][2]: id (or TAB_EMPTY), word -- one 16-byte slot, one line per hit
  unsigned long long mask;     // cap - 1
  unsigned long long* meta;
};

// the slot of `id` (!= TAB_EMPTY: vertex -1 has the side slot), claimed if absent (*fresh); ~0: the table is full
__device__ __forceinline__ unsigned long long ct_slot(const CtTable& t, unsigned long long id, bool* fresh) {
  return tab_claim<2>(t.slots, t.mask, id, fresh);
}

// largest u in [lo, hi] with offs[u] <= p (offs[lo] <= p given)
__device__ __forceinline__ uint32_t ct_run_of(const uint64_t* __restrict__ offs, uint32_t lo, uint32_t hi, uint64_t p) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (offs[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the vertex column of the per-record outputs needs no sort: record 2i is src[i], 2i + 1 is dst[i] (ALL)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_ct_expand_all(const int64_t* __restrict__ src,
                                                                               const int64_t* __restrict__ dst, uint64_t n,
                                                                               int64_t* __restrict__ out_v) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < 2 * n; r += (uint64_t)gridDim.x * 256)
    out_v[r] = (r & 1) ? dst[r >> 1] : src[r >> 1];
}

// every slot free: (TAB_EMPTY, 0)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_ct_clear(ulonglong2* __restrict__ slots, uint64_t cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * 256)
    slots[s] = make_ulonglong2(TAB_EMPTY, 0ull);
}

// growth: every entry of the old table into the new one (keys distinct: claims only)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_ct_rehash(const ulonglong2* __restrict__ oslots, uint64_t ocap,
                                                                           CtTable t) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < ocap; s += (uint64_t)gridDim.x * 256) {
    const ulonglong2 o = oslots[s];
    const unsigned long long id = o.x;
    if (id == TAB_EMPTY) continue;
    bool fresh;
    const unsigned long long d = ct_slot(t, id, &fresh);
    if (d == ~0ull) atomicOr(&t.meta[CT_ERR], 1ull);
    else t.slots[2 * d + 1] = o.y;
  }
}

namespace {

// a table of cap free slots (cleared in the ctx stream's order)
[[maybe_unused]] gs_status ct_alloc_table(gs_ctx* c, uint64_t cap, unsigned long long** slots) {
  *slots = nullptr;
  if (cap > (1ull << 40) || hipMalloc((void**)slots, cap * 16) != hipSuccess) {
    (void)hipGetLastError();
    *slots = nullptr;
    return set_error(c, GS_ENOMEM, "continuous state: a vertex table of %llu slots does not fit",
                     (unsigned long long)cap);
  }
  hipLaunchKernelGGL(k_ct_clear, dim3(tab_grid(cap)), dim3(256), 0, c->stream, (ulonglong2*)*slots, cap);
  const gs_status st = hip_check(c, hipGetLastError(), "k_ct_clear");
  if (st != GS_OK) {
    hipFree(*slots);
    *slots = nullptr;
  }
  return st;
}

// room for `need` distinct vertices at load <= 1/2: grow by doubling (allocate, re-insert, swap).  On any
// failure the old table stays as it was.  State: slots, meta (meta_words u64), cap, distinct, growths.
template <class State>
gs_status ct_reserve(gs_ctx* c, State* t, uint64_t need, int meta_words) {
  if (need <= t->cap / 2) return GS_OK;
  uint64_t cap, doublings;
  // a table of 2^40 slots may still double: ct_alloc_table refuses the 2^41 it plans
  if (!tab_plan_growth(t->cap, need, 1ull << 41, &cap, &doublings))
    return set_error(c, GS_ENOMEM, "continuous state: %llu vertices", (unsigned long long)need);
  unsigned long long* ns;
  GS_TRY(ct_alloc_table(c, cap, &ns));
  gs_status st = GS_OK;
  if (t->distinct) {
    hipLaunchKernelGGL(k_ct_rehash, dim3(tab_grid(t->cap)), dim3(256), 0, c->stream, (const ulonglong2*)t->slots, t->cap,
                       CtTable{ns, cap - 1, t->meta});
    st = hip_check(c, hipGetLastError(), "k_ct_rehash");
  }
  if (st == GS_OK) st = tab_read_meta(c, t->meta, meta_words);
  if (st == GS_OK && c->host_small[8 + CT_ERR]) st = set_error(c, GS_EDEVICE, "continuous state: re-insert failed");
  if (st != GS_OK) {
    hipFree(ns);
    return st;
  }
  hipFree(t->slots);
  t->slots = ns;
  t->cap = cap;
  t->growths += doublings;
  return GS_OK;
}

// the batch as runs: the stable sort of its direction-expanded records with the arrival index as payload
// (s->vals: uint32_t rec[R]), the run keys rk[U] and the run offsets offs[U + 1]
[[maybe_unused]] gs_status ct_sorted_runs(gs_ctx* c, const int64_t* src, const int64_t* dst, uint64_t n, int32_t dir, uint64_t R,
                                          Sorted* s, int64_t* rk, uint64_t* offs, uint64_t* U) {
  GS_TRY(sort_window(c, src, dst, nullptr, 0, n, dir, PAY_IDX, s));
  GS_HIP(hipMemsetAsync(offs, 0, 8, c->stream));
  *U = 0;
  GS_TRY((s->wide ? launch_rbk<uint64_t, CountOp>(c, *s, CsrOut{rk, offs}, U)
                  : launch_rbk<uint32_t, CountOp>(c, *s, CsrOut{rk, offs}, U)));
  if (*U == 0 || *U > R) return set_error(c, GS_EDEVICE, "continuous state: %llu runs in %llu records",
                                          (unsigned long long)*U, (unsigned long long)R);
  return GS_OK;
}

}  // namespace

}  // namespace gs

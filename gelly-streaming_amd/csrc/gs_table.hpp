// gs_table.hpp — what the device-resident tables share: probing, block-wide counters, compaction, growth planning.
//
// gs_continuous.hip (vertex -> count), gs_matching.hip (vertex -> weight and link) and gs_assign.hip (vertex ->
// label) keep an open-addressing table in HBM across calls whose slot key is a whole 64-bit vertex id: cap slots,
// cap a power of two, linear probing from the low bits of ct_hash(id), load <= 1/2, grown by doubling and re-insert.  They
// take everything here.  gs_distinct.hip takes the host helpers and TAB_EMPTY only: its slot words are an index
// into a log, not the key, and its probe loops (like those of gs_trisample.hip's per-batch table) compare keys
// through that index, so they stay where they are.
//
// The find-or-claim protocol (tab_claim).  A key word only ever changes TAB_EMPTY -> id, through an agent-scope
// compare-and-swap, and never changes again while the table lives (growth builds a new table).  So:
//   - a word read as another id is that id for good: the probe moves on and never reads it again;
//   - a word read as `id` is the slot: some lane claimed it, in this kernel or an earlier one;
//   - only a word read as TAB_EMPTY can still change, and the CAS decides who claims it.  The loser gets the
//     winner's id back and treats it like a read: equal -> the slot, else -> the next one.
// The reads are relaxed agent-scope atomic loads: every probe reads the word anew, past the CU's own cache, and
// orders nothing.  Nothing but the key is published by the claim: a slot's other words are written by the lane
// that owns the key in the running kernel, or read by a later kernel of the same stream.  Two lanes with the
// same id inside one kernel therefore get the same slot, and exactly one of them sees *fresh.
// At load <= 1/2 the probe always ends; the "table full" return is there so a broken invariant sets the state's
// error word instead of looping.
//
// The error word.  A failed claim ORs 1 into the state's error word, which the host reads back after the kernel.
// gs_matching.hip and gs_assign.hip clear that word before a growth's re-insert ("the error word is this
// re-insert's alone"); gs_continuous.hip and gs_distinct.hip do not, so there a bit left by an earlier failed
// call also fails the next growth.  The difference is known and is behaviour: it is not this layer's to change.
#pragma once
#include "gs_ops.hpp"

namespace gs {

constexpr unsigned long long TAB_EMPTY = ~0ull;        // a free slot's key: the bits of vertex -1, which lives in a side slot
constexpr unsigned long long TAB_SIGN = 1ull << 63;    // id ^ TAB_SIGN: ascending unsigned = ascending signed id
constexpr int TAB_PART = 16;                           // block_add's LDS words: the waves of a 1024-thread block

// the slot of `id` (!= TAB_EMPTY) in the key column key0[WORDS * slot], claimed if absent (*fresh); ~0 when the
// table is full.  WORDS: 64-bit words per slot.
template <unsigned WORDS>
__device__ __forceinline__ unsigned long long tab_claim(unsigned long long* key0, unsigned long long mask,
                                                        unsigned long long id, bool* fresh) {
  *fresh = false;
  unsigned long long s = ct_hash(id) & mask;
  for (unsigned long long i = 0; i <= mask; ++i, s = (s + 1) & mask) {
    unsigned long long* key = key0 + WORDS * s;
    unsigned long long k = __hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == TAB_EMPTY) {
      k = atomicCAS(key, TAB_EMPTY, id);
      if (k == TAB_EMPTY) {
        *fresh = true;
        return s;
      }
    }
    if (k == id) return s;
  }
  return ~0ull;
}

// the slot of `id` (!= TAB_EMPTY) if the table holds it, else ~0: claims nothing, for kernels that run after the
// claims of an earlier kernel
template <unsigned WORDS>
__device__ __forceinline__ unsigned long long tab_lookup(const unsigned long long* key0, unsigned long long mask,
                                                         unsigned long long id) {
  unsigned long long s = ct_hash(id) & mask;
  for (unsigned long long i = 0; i <= mask; ++i, s = (s + 1) & mask) {
    const unsigned long long k = key0[WORDS * s];
    if (k == id) return s;
    if (k == TAB_EMPTY) return ~0ull;
  }
  return ~0ull;
}

// *word += the block's sum of v with one atomic per block: every thread of the block (up to 1024) calls it, once
// per word and kernel.  s_part: TAB_PART words of LDS, reusable from one call to the next.
// One atomic per wave is too many here: nearly every wave of a batch holds some new vertex, and a single word
// takes ~90 atomics per microsecond (963 000 runs, 15 000 waves: 202 us per call, 72 us this way).
__device__ __forceinline__ void block_add(unsigned long long* word, unsigned long long v, unsigned long long* s_part) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  const int waves = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int i = 0; i < waves; ++i) tot += s_part[i];
    if (tot) atomicAdd(word, tot);
  }
  __syncthreads();
}

// the wave's lanes with `occ` take consecutive rows from *counter, one atomic per wave (by its first such lane):
// this lane's row, meaningful where occ.  Whole waves call it.
__device__ __forceinline__ unsigned long long wave_compact_base(bool occ, unsigned long long* counter) {
  const unsigned long long m = __ballot(occ);
  if (!m) return 0;
  const int lane = threadIdx.x & 63, leader = __ffsll(m) - 1;
  unsigned long long first = 0;
  if (lane == leader) first = atomicAdd(counter, (unsigned long long)__popcll(m));
  first = __shfl(first, leader);
  return first + __popcll(m & ((1ull << lane) - 1));
}

// a checkpoint's sorted keys (id ^ TAB_SIGN, in the sort's compact form) back to int64 ids
template <typename K>
__global__ __launch_bounds__(256) void k_tab_unkey(const K* __restrict__ sk, uint64_t key_xor, uint64_t n,
                                                   int64_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    out[i] = (int64_t)(((uint64_t)sk[i] ^ key_xor) ^ TAB_SIGN);
}

namespace {

// blocks of 256 lanes over n items, each looping.  tab_grid_tab: for the kernels that end in one atomic per block
// on a shared word -- a few blocks per CU
unsigned tab_grid(uint64_t n) { return grid_for(n, 256, 16384); }
[[maybe_unused]] unsigned tab_grid_tab(uint64_t n) { return grid_for(n, 256, 2048); }

// a state's device words meta[0 .. words) -> host_small[8 .. 8 + words), and a wait for the stream
gs_status tab_read_meta(gs_ctx* c, const unsigned long long* meta, int words) {
  GS_HIP(hipMemcpyAsync(c->host_small + 8, meta, (size_t)words * 8, hipMemcpyDeviceToHost, c->stream));
  return host_wait(c);
}

// the doubling plan of a reserve(): the smallest cap * 2^doublings with need <= half of it.  false when a table
// of max_cap slots would have to double (the caller's GS_ENOMEM).
bool tab_plan_growth(uint64_t cap, uint64_t need, uint64_t max_cap, uint64_t* new_cap, uint64_t* doublings) {
  *doublings = 0;
  while (need > cap / 2) {
    if (cap >= max_cap) return false;
    cap *= 2;
    ++*doublings;
  }
  *new_cap = cap;
  return true;
}

}  // namespace

}  // namespace gs

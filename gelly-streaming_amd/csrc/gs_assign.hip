// gs_assign.hip — example/IterativeConnectedComponents (IterativeConnectedComponents.java:67-168: the
// AssignComponents mapper at parallelism 1): a device-resident partition of the vertices seen so far that emits
// one (vertex, label) record per vertex whose label changes, label = the smallest vertex of the component.
//
// Reading (include/gelly_hip.h, "AssignComponents"): the mapper as its comments describe it -- a
// vertex that joins a component with a smaller id is added to it, where addToExistingComponent :136-139 emits it
// and forgets it.  Under that reading a record that returns over the feedback edge is a no-op, so the output is a
// function of the edge stream.  Inside one edge's emission the records come ascending by vertex (the reference:
// HashSet iteration order), the two of a new component as (src, dst).  Vertex -1 is an ordinary vertex.
//
// Vertex table (HBM), as gs_continuous.hip's: slots[cap + 1] of 16 bytes (id, label), cap a power of two, linear
// probing from a murmur3 finaliser of the full int64 id, load <= 1/2, grown by doubling before a batch whose 2n
// endpoints could overflow it.  An empty slot's id is ~0 (the bits of vertex -1); vertex -1 lives in the side slot
// slots[cap].  lslot[s] = the slot of s's label vertex, AS_NONE while s is not part of the state: a slot a batch
// claimed and then could not deliver (GS_ECAPACITY) stays claimed and absent, and the next growth drops it.
//
// One batch of n edges, edge = its index i.  Nodes = slots: the old labels the endpoints map to, and the batch's
// new vertices as singletons labelled with themselves; first[v] = the smallest edge that touches a new v.
//   k_as_insert   claims the endpoints' slots
//   k_as_nodes    the node of every endpoint, first[]
//   rounds, driven from the host with one read-back each (minedge words carry the round in their upper half, so
//   they are never reset):
//     k_as_find     live edge i: roots a, b of its ends (pointer halving); a == b: the edge is gone for good;
//                   else atomicMin(minedge[a], i), atomicMin(minedge[b], i), and i stays on the live list
//     k_as_decide   from the roots and minedge of k_as_find alone: mutual minimum -> the larger label loses; the
//                   minimum edge of the larger label only -> that one loses (its composition at time i is exact,
//                   the other side's label can only fall); else the edge waits.  The loser lo of edge i:
//                   retire[lo] = i, hook[lo] = winner root, parent[lo] = winner root (a root loses at its one
//                   minimum edge: plain stores, read by no decision of the round)
//   the smallest live edge is a mutual minimum, so every round finalises one: a round that does not ends the call
//   with GS_EDEVICE.  Finalised edges are minimum outgoing edges of their components, i.e. the minimum spanning
//   forest under arrival index (cut property); a dropped edge closes a cycle of earlier forest edges.
//   k_as_plabel   retired label mu, i = retire[mu]: along hook[] past every label retired before i: the label the
//                 winner side held at time i
//   k_as_records  one pass over the table, old and new vertices: from the vertex's label before the batch along
//                 plabel[] while the label is retired, a record (retire[mu], vertex, plabel[mu]) per step; plus the
//                 winner's own record of a new component and the two of a self-loop on a new vertex.  COUNT: the
//                 records per slot; after the scan the same walk writes them, and the new labels -- the only
//                 kernel of a batch that changes the state, and it runs after every check that can refuse the call
//   sort          by the order key inside an edge (skipped when every edge emitted one record), then stably by edge
#include "gs_table.hpp"

namespace gs {

constexpr uint32_t AS_NONE = 0xFFFFFFFFu;
// u64 words of gs_assign::meta
enum { AS_ERR = 0, AS_CLAIM = 1, AS_PEND = 2, AS_FIN = 3, AS_NEW = 4, AS_RETIRED = 5, AS_LOOPS = 6, AS_DUMP = 7, AS_ROOTS = 8,
       AS_META = 16 };

struct AsSlot {
  unsigned long long id;
  long long label;
};

struct AsTable {
  AsSlot* slots;                 // [cap + 1]; [cap]: vertex -1
  uint32_t* lslot;               // [cap + 1] slot of the label vertex, AS_NONE: not in the state
  // per batch, indexed by node = slot
  uint32_t* parent;              // AS_NONE: a root
  unsigned long long* minedge;   // (~round) << 32 | smallest live edge at this root
  uint32_t* retire;              // the edge at which this label lost, AS_NONE: alive
  uint32_t* hook;                // the winner side's root then
  uint32_t* plabel;              // the winner side's label then
  uint32_t* first;               // new vertices: the smallest edge of the batch that touches it
  unsigned long long* counts;    // records per slot, [cap + 2]
  unsigned long long* pos;       // their exclusive scan, [cap + 2]
  unsigned long long mask;       // cap - 1
  unsigned long long* meta;
};

// the slot of `id`, claimed if absent (*fresh); vertex -1: the side slot, never fresh; AS_NONE (what tab_claim's
// ~0 narrows to: slots stay below 2^31) when the table is full
__device__ __forceinline__ uint32_t as_slot(const AsTable& t, unsigned long long id, bool* fresh) {
  *fresh = false;
  if (id == TAB_EMPTY) return (uint32_t)(t.mask + 1);
  return (uint32_t)tab_claim<sizeof(AsSlot) / 8>(&t.slots->id, t.mask, id, fresh);
}

// the slot of `id` if the table holds it, else AS_NONE (claims nothing)
__device__ __forceinline__ uint32_t as_lookup(const AsTable& t, unsigned long long id) {
  if (id == TAB_EMPTY) return (uint32_t)(t.mask + 1);
  return (uint32_t)tab_lookup<sizeof(AsSlot) / 8>(&t.slots->id, t.mask, id);
}

__device__ __forceinline__ unsigned long long as_word(uint32_t round, uint32_t i) {
  return ((unsigned long long)(~round) << 32) | i;
}

// root of x; every vertex on the way skips to its grandparent (parents only ever move to an ancestor)
__device__ __forceinline__ uint32_t as_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == AS_NONE) return x;
    const uint32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g != AS_NONE) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
  }
}

// every slot free and outside the state; the side slot's id is vertex -1 from the start
__global__ __launch_bounds__(256) void k_as_clear(AsSlot* __restrict__ slots, uint32_t* __restrict__ lslot, uint64_t cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= cap; s += (uint64_t)gridDim.x * 256) {
    slots[s] = AsSlot{TAB_EMPTY, 0ll};
    lslot[s] = AS_NONE;
  }
}

// lane per edge: the slots of its endpoints (claimed if absent), live[i] = i, no loser yet
__global__ __launch_bounds__(256) void k_as_insert(AsTable t, const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                   uint64_t n, uint32_t* __restrict__ va, uint32_t* __restrict__ vb,
                                                   uint32_t* __restrict__ live, uint32_t* __restrict__ loser) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long claims = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    bool fa, fb;
    uint32_t a = as_slot(t, (unsigned long long)bs[i], &fa);
    uint32_t b = as_slot(t, (unsigned long long)bd[i], &fb);
    claims += (fa ? 1 : 0) + (fb ? 1 : 0);
    if (a == AS_NONE || b == AS_NONE) {
      atomicOr(&t.meta[AS_ERR], 1ull);
      a = b = (uint32_t)(t.mask + 1);   // a valid slot: nothing later leaves the arrays
    }
    va[i] = a;
    vb[i] = b;
    if (live) live[i] = (uint32_t)i;
    if (loser) loser[i] = AS_NONE;
  }
  block_add(&t.meta[AS_CLAIM], claims, s_part);
}

// lane per edge: the nodes of its endpoints -- a vertex outside the state is a new singleton (its own slot) and
// takes part in first[]; a known vertex stands for its label's slot
__global__ __launch_bounds__(256) void k_as_nodes(AsTable t, uint64_t n, const uint32_t* __restrict__ va,
                                                  const uint32_t* __restrict__ vb, uint32_t* __restrict__ ra,
                                                  uint32_t* __restrict__ rb) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t s = e ? vb[i] : va[i];
      uint32_t node = t.lslot[s];
      if (node == AS_NONE) {
        node = s;
        atomicMin(&t.first[s], (uint32_t)i);
      }
      (e ? rb : ra)[i] = node;
    }
  }
}

// round step 1, lane per live edge
__global__ __launch_bounds__(256) void k_as_find(AsTable t, const uint32_t* __restrict__ live, uint32_t cnt, uint32_t round,
                                                 uint32_t* __restrict__ ra, uint32_t* __restrict__ rb,
                                                 uint32_t* __restrict__ next) {
  const uint64_t rounded = ((uint64_t)cnt + 255) & ~255ull;   // whole waves reach the ballot
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < rounded; p += (uint64_t)gridDim.x * 256) {
    bool stay = false;
    uint32_t i = 0;
    if (p < cnt) {
      i = live[p];
      const uint32_t a = as_find(t.parent, ra[i]), b = as_find(t.parent, rb[i]);
      ra[i] = a;
      rb[i] = b;
      if (a != b) {
        // a word that is below w already stays below it: most edges at a hub's root skip the atomic (one word
        // takes ~90 atomics per microsecond, and the giant component's root is an end of most live edges)
        const unsigned long long w = as_word(round, i);
        if (__hip_atomic_load(&t.minedge[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > w) atomicMin(&t.minedge[a], w);
        if (__hip_atomic_load(&t.minedge[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > w) atomicMin(&t.minedge[b], w);
        stay = true;
      }
    }
    const unsigned long long k = wave_compact_base(stay, &t.meta[AS_PEND]);
    if (stay) next[k] = i;
  }
}

// round steps 2 and 3, lane per edge that k_as_find kept (meta[AS_PEND] of them, at most cnt)
__global__ __launch_bounds__(256) void k_as_decide(AsTable t, const uint32_t* __restrict__ live, uint32_t cnt, uint32_t round,
                                                   const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb,
                                                   uint32_t* __restrict__ loser) {
  __shared__ unsigned long long s_part[TAB_PART];
  const uint64_t have = min((unsigned long long)cnt, t.meta[AS_PEND]);
  unsigned long long fin = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < have; p += (uint64_t)gridDim.x * 256) {
    const uint32_t i = live[p];
    const uint32_t a = ra[i], b = rb[i];
    const unsigned long long w = as_word(round, i);
    const bool ma = t.minedge[a] == w, mb = t.minedge[b] == w;
    const long long la = (long long)t.slots[a].id, lb = (long long)t.slots[b].id;   // a root's id is its label
    uint32_t lo = AS_NONE, wi = AS_NONE;
    if (ma && mb) {
      lo = la > lb ? a : b;
      wi = la > lb ? b : a;
    } else if (mb && lb > la) {
      lo = b;
      wi = a;
    } else if (ma && la > lb) {
      lo = a;
      wi = b;
    }
    if (lo == AS_NONE) continue;
    t.retire[lo] = i;
    t.hook[lo] = wi;
    __hip_atomic_store(&t.parent[lo], wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    loser[i] = lo;
    ++fin;
  }
  block_add(&t.meta[AS_FIN], fin, s_part);
}

// lane per edge that retired a label: the label its winner side held at that time
__global__ __launch_bounds__(256) void k_as_plabel(AsTable t, uint64_t n, const uint32_t* __restrict__ loser) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t lo = loser[i];
    if (lo == AS_NONE) continue;
    uint32_t l = t.hook[lo];
    for (;;) {
      const uint32_t r = t.retire[l];
      if (r == AS_NONE || r >= (uint32_t)i) break;
      l = t.hook[l];
    }
    t.plabel[lo] = l;
  }
}

struct AsRec {
  unsigned long long* edge;   // sort key 2: the batch index of the record's edge
  unsigned long long* key;    // sort key 1: the order inside one edge
  int64_t* vertex;
  int64_t* label;
  uint32_t* iota;
};

// lane per slot.  COUNT: counts[s] = the records of the slot's vertex, and the batch's new vertices, retired
// labels and self-loops on new vertices.  Otherwise: the records at pos[s] .. (rec.edge == nullptr: none are
// written) and the vertex's new label -- a lane writes its own slot's (label, lslot) only and reads no other
// slot's, so "new" is read off first[], which this kernel leaves alone.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_as_records(AsTable t, const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                    const uint32_t* __restrict__ va, const uint32_t* __restrict__ vb, AsRec rec) {
  __shared__ unsigned long long s_part[TAB_PART];
  const uint64_t cap = t.mask + 1;
  unsigned long long n_new = 0, n_retired = 0, n_loops = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= cap; s += (uint64_t)gridDim.x * 256) {
    const uint32_t own = t.lslot[s];
    const uint32_t f = t.first[s];
    const bool is_new = own == AS_NONE && f != AS_NONE;
    if (COUNT) t.counts[s] = 0;
    if (own == AS_NONE && !is_new) continue;
    const long long id = (long long)t.slots[s].id;
    // what the vertex's first edge adds to the ordinary records
    int extra = 0;
    bool pair = false, pair_second = false;   // a new component's pair: order key 0 (src) / 1 (dst)
    if (is_new) {
      const uint32_t a = va[f], b = vb[f];
      if (a == b) {
        extra = 2;
      } else if (t.first[a] == f && t.first[b] == f) {
        pair = true;
        pair_second = (uint32_t)s == b;
        extra = id == min((long long)bs[f], (long long)bd[f]) ? 1 : 0;
      }
    }
    uint32_t mu = is_new ? (uint32_t)s : own;
    if (COUNT) {
      unsigned long long c = extra;
      n_new += is_new;
      n_loops += extra == 2;
      n_retired += mu == (uint32_t)s && t.retire[mu] != AS_NONE;
      while (t.retire[mu] != AS_NONE) {
        ++c;
        mu = t.plabel[mu];
      }
      t.counts[s] = c;
    } else {
      unsigned long long k = t.pos[s];
      const bool write = rec.edge != nullptr;
      if (write)
        for (int x = 0; x < extra; ++x, ++k) {
          rec.edge[k] = f;
          rec.key[k] = extra == 2 ? (unsigned long long)x : (pair_second ? 1ull : 0ull);
          rec.vertex[k] = id;
          rec.label[k] = id;
          rec.iota[k] = (uint32_t)k;
        }
      bool moved = false;
      for (uint32_t r; (r = t.retire[mu]) != AS_NONE; ++k) {
        const uint32_t l = t.plabel[mu];
        if (write) {
          rec.edge[k] = r;
          rec.key[k] = (pair && r == f) ? (pair_second ? 1ull : 0ull) : ((unsigned long long)id ^ TAB_SIGN);
          rec.vertex[k] = id;
          rec.label[k] = (long long)t.slots[l].id;
          rec.iota[k] = (uint32_t)k;
        }
        mu = l;
        moved = true;
      }
      if (moved || is_new) {
        t.slots[s].label = (long long)t.slots[mu].id;
        t.lslot[s] = mu;
      }
    }
  }
  if (COUNT) {
    block_add(&t.meta[AS_NEW], n_new, s_part);
    block_add(&t.meta[AS_RETIRED], n_retired, s_part);
    block_add(&t.meta[AS_LOOPS], n_loops, s_part);
  }
}

// between the two sorts: the edge keys and the record numbers in the first sort's order
__global__ __launch_bounds__(256) void k_as_regroup(const uint32_t* __restrict__ perm, uint64_t R,
                                                    const unsigned long long* __restrict__ edge,
                                                    unsigned long long* __restrict__ ek, uint32_t* __restrict__ ev) {
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < R; k += (uint64_t)gridDim.x * 256) {
    const uint32_t r = perm[k];
    ek[k] = edge[r];
    ev[k] = r;
  }
}

__global__ __launch_bounds__(256) void k_as_gather(const uint32_t* __restrict__ perm, uint64_t R, AsRec rec,
                                                   int64_t* __restrict__ ov, int64_t* __restrict__ ol, uint32_t* __restrict__ oe) {
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < R; k += (uint64_t)gridDim.x * 256) {
    const uint32_t r = perm[k];
    if (ov) ov[k] = rec.vertex[r];
    if (ol) ol[k] = rec.label[r];
    if (oe) oe[k] = (uint32_t)rec.edge[r];
  }
}

// growth, step 1: every vertex of the state into the new table with its label; map[old slot] = new slot
__global__ __launch_bounds__(256) void k_as_rehash(const AsSlot* __restrict__ os, const uint32_t* __restrict__ ol, uint64_t ocap,
                                                   AsTable t, uint32_t* __restrict__ map) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= ocap; s += (uint64_t)gridDim.x * 256) {
    uint32_t d = AS_NONE;
    if (ol[s] != AS_NONE) {
      bool fresh;
      d = as_slot(t, os[s].id, &fresh);
      if (d == AS_NONE) atomicOr(&t.meta[AS_ERR], 1ull);
      else t.slots[d].label = os[s].label;
    }
    map[s] = d;
  }
}
// step 2: the label slots, translated
__global__ __launch_bounds__(256) void k_as_relink(const uint32_t* __restrict__ ol, uint64_t ocap, uint32_t* __restrict__ nl,
                                                   const uint32_t* __restrict__ map) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= ocap; s += (uint64_t)gridDim.x * 256) {
    const uint32_t l = ol[s];
    if (l == AS_NONE) continue;
    const uint32_t d = map[s], p = map[l];
    if (d != AS_NONE && p != AS_NONE) nl[d] = p;
  }
}

// checkpoint: the state's vertices as (id ^ sign bit, label) rows in any order; V rows expected
__global__ __launch_bounds__(256) void k_as_dump(AsTable t, unsigned long long* __restrict__ keys, long long* __restrict__ labels,
                                                 uint64_t V) {
  const uint64_t cap = t.mask + 1;
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 <= cap; s0 += (uint64_t)gridDim.x * 256) {
    const uint64_t s = s0 + threadIdx.x;
    const bool occ = s <= cap && t.lslot[s] != AS_NONE;
    const unsigned long long k = wave_compact_base(occ, &t.meta[AS_DUMP]);
    if (occ && k < V) {
      keys[k] = t.slots[s].id ^ TAB_SIGN;
      labels[k] = t.slots[s].label;
    }
  }
}

// restore, step 1: row i marks its vertex's slot (first[] = the smallest row of the vertex)
__global__ __launch_bounds__(256) void k_as_import_mark(AsTable t, uint64_t n, const uint32_t* __restrict__ va) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    atomicMin(&t.first[va[i]], (uint32_t)i);
}
// step 2: one row per vertex, label <= vertex, and the label's own row carries label == vertex; ls[i] = its slot
__global__ __launch_bounds__(256) void k_as_import_check(AsTable t, uint64_t n, const int64_t* __restrict__ keys,
                                                         const int64_t* __restrict__ labels, const uint32_t* __restrict__ va,
                                                         uint32_t* __restrict__ ls) {
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const int64_t l = labels[i];
    uint32_t s = AS_NONE;
    if (t.first[va[i]] != (uint32_t)i || l > keys[i]) {
      bad = true;
    } else {
      s = as_lookup(t, (unsigned long long)l);
      const uint32_t j = s == AS_NONE ? AS_NONE : t.first[s];
      if (j == AS_NONE || labels[j] != l) bad = true;   // (first[s] = j: keys[j] == l)
    }
    ls[i] = s;
  }
  if (bad) atomicOr(&t.meta[AS_ERR], 2ull);
}
__global__ __launch_bounds__(256) void k_as_import_write(AsTable t, uint64_t n, const int64_t* __restrict__ labels,
                                                         const uint32_t* __restrict__ va, const uint32_t* __restrict__ ls) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long roots = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t s = va[i];
    t.slots[s].label = labels[i];
    t.lslot[s] = ls[i];
    roots += ls[i] == s;
  }
  block_add(&t.meta[AS_ROOTS], roots, s_part);
}

}  // namespace gs

using namespace gs;

struct gs_assign {
  int device = 0;
  char* block = nullptr;         // one allocation: the table and the per-batch node arrays
  AsTable tab{};                 // pointers into it
  unsigned long long* meta = nullptr;   // device u64[AS_META]
  uint64_t cap = 0;              // slots (power of two)
  uint64_t occupied = 0;         // claimed slots, vertices outside the state included (an upper bound after a growth)
  uint64_t vertices = 0, components = 0, records = 0, growths = 0;
  uint64_t rounds = 0, merging = 0, last_records = 0, live_after[4] = {0, 0, 0, 0};   // the last batch
  bool broken = false;           // the record pass failed on the device midway
};

namespace {

constexpr uint64_t AS_MAX_CAP = 1ull << 31;   // slot numbers are 32-bit, AS_NONE is none of them

size_t as_round(size_t b) { return (b + 255) & ~(size_t)255; }

// one block of HBM for a table of cap slots; every array holds cap + 2 entries
gs_status alloc_table(gs_ctx* c, uint64_t cap, unsigned long long* meta, char** block, AsTable* t) {
  *block = nullptr;
  const uint64_t m = cap + 2;
  const size_t total = as_round(m * sizeof(AsSlot)) + 6 * as_round(m * 4) + 3 * as_round(m * 8);
  if (cap > AS_MAX_CAP || hipMalloc((void**)block, total) != hipSuccess) {
    (void)hipGetLastError();
    *block = nullptr;
    return set_error(c, GS_ENOMEM, "assign state: a vertex table of %llu slots does not fit", (unsigned long long)cap);
  }
  char* p = *block;
  auto take = [&p](size_t bytes) {
    char* q = p;
    p += as_round(bytes);
    return q;
  };
  t->slots = (AsSlot*)take(m * sizeof(AsSlot));
  t->minedge = (unsigned long long*)take(m * 8);
  t->counts = (unsigned long long*)take(m * 8);
  t->pos = (unsigned long long*)take(m * 8);
  t->lslot = (uint32_t*)take(m * 4);
  t->parent = (uint32_t*)take(m * 4);
  t->retire = (uint32_t*)take(m * 4);
  t->hook = (uint32_t*)take(m * 4);
  t->plabel = (uint32_t*)take(m * 4);
  t->first = (uint32_t*)take(m * 4);
  t->mask = cap - 1;
  t->meta = meta;
  hipLaunchKernelGGL(k_as_clear, dim3(tab_grid(cap + 1)), dim3(256), 0, c->stream, t->slots, t->lslot, cap);
  const gs_status st = hip_check(c, hipGetLastError(), "k_as_clear");
  if (st != GS_OK) {
    hipFree(*block);
    *block = nullptr;
  }
  return st;
}

// room for `need` claimed slots at load <= 1/2: grow by doubling (allocate, re-insert the state's vertices,
// swap).  On any failure the old table stays as it was.
gs_status reserve(gs_ctx* c, gs_assign* t, uint64_t need) {
  if (need <= t->cap / 2) return GS_OK;
  need = need - t->occupied + t->vertices;   // the re-insert leaves the vertices outside the state behind
  uint64_t cap, doublings;
  if (!tab_plan_growth(t->cap, need, AS_MAX_CAP, &cap, &doublings))
    return set_error(c, GS_ENOMEM, "assign state: %llu vertices", (unsigned long long)need);
  GS_TRY(ensure(c, c->ts[11], (t->cap + 2) * 4));
  char* nb;
  AsTable nt;
  GS_TRY(alloc_table(c, cap, t->meta, &nb, &nt));
  uint32_t* map = c->ts[11].as<uint32_t>();
  gs_status st = hip_check(c, hipMemsetAsync(t->meta + AS_ERR, 0, 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) {
    hipLaunchKernelGGL(k_as_rehash, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, (const AsSlot*)t->tab.slots,
                       (const uint32_t*)t->tab.lslot, t->cap, nt, map);
    st = hip_check(c, hipGetLastError(), "k_as_rehash");
  }
  if (st == GS_OK) {
    hipLaunchKernelGGL(k_as_relink, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, (const uint32_t*)t->tab.lslot, t->cap,
                       nt.lslot, (const uint32_t*)map);
    st = hip_check(c, hipGetLastError(), "k_as_relink");
  }
  if (st == GS_OK) st = tab_read_meta(c, t->meta, AS_META);
  if (st == GS_OK && c->host_small[8 + AS_ERR]) {
    hipMemsetAsync(t->meta + AS_ERR, 0, 8, c->stream);
    st = set_error(c, GS_EDEVICE, "assign state: re-insert failed");
  }
  if (st != GS_OK) {
    hipFree(nb);
    return st;
  }
  hipFree(t->block);
  t->block = nb;
  t->tab = nt;
  t->cap = cap;
  t->occupied = t->vertices;
  t->growths += doublings;
  return GS_OK;
}

gs_status check_state(gs_ctx* c, const gs_assign* t) {
  if (!c) return GS_EINVAL;
  if (!t) return set_error(c, GS_EINVAL, "null assign state");
  if (t->device != c->device)
    return set_error(c, GS_EINVAL, "assign state lives on device %d, the ctx on device %d", t->device, c->device);
  if (t->broken) return set_error(c, GS_EDEVICE, "assign state: an earlier batch failed on the device");
  return GS_OK;
}

// the per-batch node arrays back to "no parent, no minimum edge, alive, not new"
gs_status reset_nodes(gs_ctx* c, const gs_assign* t, bool rounds) {
  const uint64_t m = t->cap + 2;
  GS_HIP(hipMemsetAsync(t->tab.first, 0xFF, m * 4, c->stream));
  if (!rounds) return GS_OK;
  GS_HIP(hipMemsetAsync(t->tab.parent, 0xFF, m * 4, c->stream));
  GS_HIP(hipMemsetAsync(t->tab.retire, 0xFF, m * 4, c->stream));
  GS_HIP(hipMemsetAsync(t->tab.minedge, 0xFF, m * 8, c->stream));
  return GS_OK;
}

// the rounds of one batch (see the head of this file); they write the per-batch arrays only
gs_status run_rounds(gs_ctx* c, gs_assign* t, uint64_t n) {
  uint32_t *ra = c->ts[2].as<uint32_t>(), *rb = c->ts[3].as<uint32_t>();
  uint32_t *cur = c->ts[4].as<uint32_t>(), *nxt = c->ts[5].as<uint32_t>();
  uint32_t* loser = c->ts[6].as<uint32_t>();
  uint64_t cnt = n;
  t->rounds = t->merging = 0;
  for (int k = 0; k < 4; ++k) t->live_after[k] = 0;
  for (uint32_t round = 0; cnt; ++round) {
    const dim3 g(tab_grid(cnt)), b(256);
    GS_HIP(hipMemsetAsync(t->meta + AS_PEND, 0, 16, c->stream));   // live edges, finalised edges
    hipLaunchKernelGGL(k_as_find, g, b, 0, c->stream, t->tab, (const uint32_t*)cur, (uint32_t)cnt, round, ra, rb, nxt);
    GS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_as_decide, g, b, 0, c->stream, t->tab, (const uint32_t*)nxt, (uint32_t)cnt, round,
                       (const uint32_t*)ra, (const uint32_t*)rb, loser);
    GS_HIP(hipGetLastError());
    GS_TRY(tab_read_meta(c, t->meta, AS_META));
    const uint64_t live = c->host_small[8 + AS_PEND], fin = c->host_small[8 + AS_FIN];
    if (live == 0) break;
    if (live > cnt || fin > live || fin == 0)
      return set_error(c, GS_EDEVICE, "assign state: a round finalised %llu of %llu live edges", (unsigned long long)fin,
                       (unsigned long long)live);
    ++t->rounds;
    t->merging += fin;
    for (int k = 0; k < 4; ++k)
      if (t->rounds == (1ull << k)) t->live_after[k] = live - fin;
    if (live == fin) break;
    cnt = live;
    std::swap(cur, nxt);
  }
  return GS_OK;
}

}  // namespace

extern "C" {

gs_status gs_assign_create(gs_ctx* c, uint64_t reserve_vertices, gs_assign** out) {
  if (!c) return GS_EINVAL;
  if (!out) return set_error(c, GS_EINVAL, "gs_assign_create: null argument");
  *out = nullptr;
  if (reserve_vertices > AS_MAX_CAP / 2)
    return set_error(c, GS_ENOMEM, "gs_assign_create: %llu vertices", (unsigned long long)reserve_vertices);
  (void)hipGetLastError();
  GS_HIP(hipSetDevice(c->device));
  gs_assign* t = new (std::nothrow) gs_assign();
  if (!t) return set_error(c, GS_ENOMEM, "gs_assign_create");
  t->device = c->device;
  t->cap = 64;
  while (t->cap / 2 < reserve_vertices) t->cap *= 2;
  gs_status st = GS_OK;
  if (hipMalloc((void**)&t->meta, AS_META * 8) != hipSuccess) {
    (void)hipGetLastError();
    t->meta = nullptr;
    st = set_error(c, GS_ENOMEM, "gs_assign_create: state words");
  }
  if (st == GS_OK) st = alloc_table(c, t->cap, t->meta, &t->block, &t->tab);
  if (st == GS_OK) st = hip_check(c, hipMemsetAsync(t->meta, 0, AS_META * 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) st = host_wait(c);
  if (st != GS_OK) {
    gs_assign_destroy(t);
    return st;
  }
  *out = t;
  return GS_OK;
}

void gs_assign_destroy(gs_assign* t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->block) hipFree(t->block);
  if (t->meta) hipFree(t->meta);
  delete t;
}

gs_status gs_assign_size(const gs_assign* t, uint64_t* vertices, uint64_t* components, uint64_t* records) {
  if (!t) return GS_EINVAL;
  if (vertices) *vertices = t->vertices;
  if (components) *components = t->components;
  if (records) *records = t->records;
  return GS_OK;
}

gs_status gs_assign_capacity(const gs_assign* t, uint64_t* slots, uint64_t* growths) {
  if (!t) return GS_EINVAL;
  if (slots) *slots = t->cap;
  if (growths) *growths = t->growths;
  return GS_OK;
}

gs_status gs_assign_last_batch(const gs_assign* t, uint64_t* rounds, uint64_t* merging_edges, uint64_t* records,
                               uint64_t* live_after) {
  if (!t) return GS_EINVAL;
  if (rounds) *rounds = t->rounds;
  if (merging_edges) *merging_edges = t->merging;
  if (records) *records = t->last_records;
  if (live_after)
    for (int k = 0; k < 4; ++k) live_after[k] = t->live_after[k];
  return GS_OK;
}

gs_status gs_assign_edges(gs_ctx* c, gs_assign* t, const gs_edge_batch* b, gs_assign_out* out) {
  GS_TRY(check_state(c, t));
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (!out || !out->n_out) return set_error(c, GS_EINVAL, "bad gs_assign_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_assign_out.mem %d", out->mem);
  const uint64_t n = b->n;
  const bool any = out->vertex || out->label || out->edge;
  GS_TRY(begin_call(c));
  *out->n_out = 0;
  if (n == 0) {
    t->rounds = t->merging = t->last_records = 0;
    for (int k = 0; k < 4; ++k) t->live_after[k] = 0;
    return GS_OK;
  }
  for (int k = 0; k <= 6; ++k) GS_TRY(ensure(c, c->ts[k], n * 4));
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, false));
  GS_TRY(reserve(c, t, t->occupied + 2 * n));
  uint32_t *va = c->ts[0].as<uint32_t>(), *vb = c->ts[1].as<uint32_t>();
  uint32_t* loser = c->ts[6].as<uint32_t>();
  const AsTable tab = t->tab;
  GS_HIP(hipMemsetAsync(t->meta, 0, AS_META * 8, c->stream));
  GS_TRY(reset_nodes(c, t, true));
  hipLaunchKernelGGL(k_as_insert, dim3(tab_grid_tab(n)), dim3(256), 0, c->stream, tab, src, dst, n, va, vb,
                     c->ts[4].as<uint32_t>(), loser);
  GS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_as_nodes, dim3(tab_grid(n)), dim3(256), 0, c->stream, tab, n, (const uint32_t*)va, (const uint32_t*)vb,
                     c->ts[2].as<uint32_t>(), c->ts[3].as<uint32_t>());
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, AS_META));
  t->occupied += c->host_small[8 + AS_CLAIM];   // the claims stay whatever happens next: outside the state until a batch delivers
  if (c->host_small[8 + AS_ERR]) return set_error(c, GS_EDEVICE, "assign state: the vertex table filled up");
  GS_TRY(run_rounds(c, t, n));
  hipLaunchKernelGGL(k_as_plabel, dim3(tab_grid(n)), dim3(256), 0, c->stream, tab, n, (const uint32_t*)loser);
  GS_HIP(hipGetLastError());
  const dim3 gt(tab_grid_tab(t->cap + 1)), bl(256);
  hipLaunchKernelGGL(k_as_records<true>, gt, bl, 0, c->stream, tab, src, dst, (const uint32_t*)va, (const uint32_t*)vb, AsRec{});
  GS_HIP(hipGetLastError());
  GS_TRY(xscan(c, (const uint64_t*)tab.counts, t->cap + 1, (uint64_t*)tab.pos));
  GS_HIP(hipMemcpyAsync(c->host_small + 8 + AS_META, tab.pos + t->cap + 1, 8, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(tab_read_meta(c, t->meta, AS_META));
  const uint64_t R = c->host_small[8 + AS_META];
  const uint64_t n_new = c->host_small[8 + AS_NEW], n_retired = c->host_small[8 + AS_RETIRED];
  const uint64_t n_loops = c->host_small[8 + AS_LOOPS];
  if (n_retired != t->merging || n_new > 2 * n)
    return set_error(c, GS_EDEVICE, "assign state: %llu labels retired by %llu merging edges", (unsigned long long)n_retired,
                     (unsigned long long)t->merging);
  *out->n_out = R;
  if (any && out->capacity < R) return set_error(c, GS_ECAPACITY, "output needs room for %llu records", (unsigned long long)R);
  if (any && R >= (1ull << 32))
    return set_error(c, GS_EUNSUPPORTED, "the batch emits %llu records (limit 2^32 - 1): split it", (unsigned long long)R);
  const bool direct = out->mem == GS_MEM_DEVICE;
  AsRec rec{};
  int64_t *ov = out->vertex, *ol = out->label;
  uint32_t* oe = out->edge;
  // every edge with records emitted exactly one, or a self-loop's identical two: no order inside an edge to settle
  const bool flat = R == n_retired + 2 * n_loops;
  if (any && R) {
    for (int k = 7; k <= 10; ++k) GS_TRY(ensure(c, c->ts[k], R * 8));
    GS_TRY(ensure(c, c->ct[0], R * 8));
    GS_TRY(ensure(c, c->ct[1], R * 4));
    GS_TRY(ensure(c, c->ct[2], R * 4));
    GS_TRY(ensure(c, c->keysA, R * 8));   // the sorts' own buffers: theirs to size, but no allocation may fail later
    GS_TRY(ensure(c, c->keysB, R * 8));
    GS_TRY(ensure(c, c->valsA, R * 4));
    GS_TRY(ensure(c, c->valsB, R * 4));
    GS_TRY(ensure(c, c->sort_status, ((R + SORT_TILE - 1) / SORT_TILE) * RADIX * 8, true));
    if (!direct) {
      if (ov) {
        GS_TRY(ensure(c, c->out_keys, R * 8));
        ov = c->out_keys.as<int64_t>();
      }
      if (ol) {
        GS_TRY(ensure(c, c->out_a, R * 8));
        ol = c->out_a.as<int64_t>();
      }
      if (oe) {
        GS_TRY(ensure(c, c->out_b, R * 4));
        oe = c->out_b.as<uint32_t>();
      }
    }
    rec = AsRec{c->ts[7].as<unsigned long long>(), c->ts[8].as<unsigned long long>(), c->ts[9].as<int64_t>(),
                c->ts[10].as<int64_t>(), c->ct[1].as<uint32_t>()};
  }
  // ---- the state changes from here on ----
  t->broken = true;
  hipLaunchKernelGGL(k_as_records<false>, gt, bl, 0, c->stream, tab, src, dst, (const uint32_t*)va, (const uint32_t*)vb, rec);
  GS_HIP(hipGetLastError());
  GS_TRY(host_wait(c));
  t->broken = false;
  t->vertices += n_new;
  t->components += n_new - n_retired;
  t->records += R;
  t->last_records = R;
  if (!(any && R)) return GS_OK;
  const uint32_t* perm = rec.iota;
  Sorted s1, s2;
  if (!flat) {
    GS_TRY(sort_buffer(c, (const uint64_t*)rec.key, rec.iota, R, &s1, 64, 4));
    perm = (const uint32_t*)s1.vals;
  }
  unsigned long long* ek = c->ct[0].as<unsigned long long>();
  uint32_t* ev = c->ct[2].as<uint32_t>();
  hipLaunchKernelGGL(k_as_regroup, dim3(tab_grid(R)), dim3(256), 0, c->stream, perm, R, (const unsigned long long*)rec.edge, ek, ev);
  GS_HIP(hipGetLastError());
  GS_TRY(sort_buffer(c, (const uint64_t*)ek, ev, R, &s2, 32, 4));
  hipLaunchKernelGGL(k_as_gather, dim3(tab_grid(R)), dim3(256), 0, c->stream, (const uint32_t*)s2.vals, R, rec, ov, ol, oe);
  GS_HIP(hipGetLastError());
  if (direct) return GS_OK;
  if (out->vertex) GS_TRY(deliver(c, out->vertex, ov, R * 8, out->mem));
  if (out->label) GS_TRY(deliver(c, out->label, ol, R * 8, out->mem));
  if (out->edge) GS_TRY(deliver(c, out->edge, oe, R * 4, out->mem));
  return host_wait(c);
}

gs_status gs_assign_export(gs_ctx* c, const gs_assign* t, gs_vertex_out* out) {
  GS_TRY(check_state(c, t));
  if (!out || !out->n_out || (out->capacity && (!out->keys || !out->vals))) return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_vertex_out.mem %d", out->mem);
  const uint64_t V = t->vertices;
  *out->n_out = V;
  if (out->capacity < V) return set_error(c, GS_ECAPACITY, "output needs %llu vertices", (unsigned long long)V);
  if (V >= (1ull << 32)) return set_error(c, GS_EUNSUPPORTED, "export of %llu vertices (limit 2^32 - 1)", (unsigned long long)V);
  GS_TRY(begin_call(c));
  if (V == 0) return GS_OK;
  GS_TRY(ensure(c, c->ts[7], V * 8));
  GS_TRY(ensure(c, c->ts[8], V * 8));
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t* ok = out->keys;
  if (!direct) {
    GS_TRY(ensure(c, c->out_keys, V * 8));
    ok = c->out_keys.as<int64_t>();
  }
  unsigned long long* dk = c->ts[7].as<unsigned long long>();
  long long* dl = c->ts[8].as<long long>();
  GS_HIP(hipMemsetAsync(t->meta + AS_DUMP, 0, 8, c->stream));
  hipLaunchKernelGGL(k_as_dump, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, t->tab, dk, dl, V);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, AS_META));
  if (c->host_small[8 + AS_DUMP] != V)
    return set_error(c, GS_EDEVICE, "assign state: %llu vertices in the table, %llu expected",
                     (unsigned long long)c->host_small[8 + AS_DUMP], (unsigned long long)V);
  // ascending signed ids = ascending (id ^ sign bit) as unsigned
  Sorted s;
  GS_TRY(sort_buffer(c, (const uint64_t*)dk, dl, V, &s, 64, 8));
  if (s.wide)
    hipLaunchKernelGGL(k_tab_unkey<uint64_t>, dim3(tab_grid(V)), dim3(256), 0, c->stream, (const uint64_t*)s.keys, s.key_xor, V, ok);
  else
    hipLaunchKernelGGL(k_tab_unkey<uint32_t>, dim3(tab_grid(V)), dim3(256), 0, c->stream, (const uint32_t*)s.keys, s.key_xor, V, ok);
  GS_HIP(hipGetLastError());
  GS_TRY(deliver(c, out->keys, ok, V * 8, out->mem));
  GS_TRY(deliver(c, out->vals, s.vals, V * 8, out->mem));
  return host_wait(c);
}

gs_status gs_assign_import(gs_ctx* c, gs_assign* t, const gs_partial_batch* rows) {
  GS_TRY(check_state(c, t));
  if (!rows || (rows->n && (!rows->keys || !rows->vals))) return set_error(c, GS_EINVAL, "gs_assign_import: null rows");
  if (rows->val_dtype != GS_I64) return set_error(c, GS_EINVAL, "gs_assign_import: labels are I64");
  if (rows->mem != GS_MEM_HOST && rows->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "gs_assign_import: bad mem");
  if (t->vertices || t->records) return set_error(c, GS_EINVAL, "gs_assign_import: the state is not empty");
  if (rows->n > AS_MAX_CAP / 2) return set_error(c, GS_EINVAL, "gs_assign_import: %llu rows", (unsigned long long)rows->n);
  GS_TRY(begin_call(c));
  const uint64_t n = rows->n;
  if (n == 0) return GS_OK;
  GS_TRY(ensure(c, c->ts[0], n * 4));
  GS_TRY(ensure(c, c->ts[1], n * 4));
  const int64_t* dk = rows->keys;
  const int64_t* dl = (const int64_t*)rows->vals;
  if (rows->mem != GS_MEM_DEVICE) {
    GS_TRY(ensure(c, c->in_src, n * 8));
    GS_TRY(ensure(c, c->in_dst, n * 8));
    GS_HIP(hipMemcpyAsync(c->in_src.p, rows->keys, n * 8, hipMemcpyHostToDevice, c->stream));
    GS_HIP(hipMemcpyAsync(c->in_dst.p, rows->vals, n * 8, hipMemcpyHostToDevice, c->stream));
    dk = c->in_src.as<int64_t>();
    dl = c->in_dst.as<int64_t>();
  }
  GS_TRY(reserve(c, t, t->occupied + n));
  uint32_t *va = c->ts[0].as<uint32_t>(), *ls = c->ts[1].as<uint32_t>();
  const AsTable tab = t->tab;
  const dim3 g(tab_grid_tab(n)), bl(256);
  GS_HIP(hipMemsetAsync(t->meta, 0, AS_META * 8, c->stream));
  GS_TRY(reset_nodes(c, t, false));
  // the vertices' slots: k_as_insert over (vertex, vertex) rows
  hipLaunchKernelGGL(k_as_insert, g, bl, 0, c->stream, tab, dk, dk, n, va, ls, (uint32_t*)nullptr, (uint32_t*)nullptr);
  GS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_as_import_mark, g, bl, 0, c->stream, tab, n, (const uint32_t*)va);
  GS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_as_import_check, g, bl, 0, c->stream, tab, n, dk, dl, (const uint32_t*)va, ls);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, AS_META));
  t->occupied += c->host_small[8 + AS_CLAIM];
  if (c->host_small[8 + AS_ERR] & 1) return set_error(c, GS_EDEVICE, "assign state: the vertex table filled up");
  if (c->host_small[8 + AS_ERR])
    return set_error(c, GS_EINVAL, "gs_assign_import: a vertex twice, a label above its vertex, or a label whose own row "
                                   "does not carry it");
  // ---- the state changes from here on ----
  t->broken = true;
  hipLaunchKernelGGL(k_as_import_write, g, bl, 0, c->stream, tab, n, dl, (const uint32_t*)va, (const uint32_t*)ls);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, AS_META));
  t->vertices = n;
  t->components = c->host_small[8 + AS_ROOTS];
  t->broken = false;
  return GS_OK;
}

}  // extern "C"

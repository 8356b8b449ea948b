// gs_matching.hip — example/CentralizedWeightedMatching (CentralizedWeightedMatching.java:67-108: one
// WeightedMatchingFlatMapper at parallelism 1 emitting MatchingEvent, MatchingEvent.java:24-42): a
// device-resident matching that outlives a batch.
//
// The reference keeps a HashSet M of edges and, per arriving edge e = (u, v, w): C = the edges of M sharing an
// endpoint with e, sum = their values, and if w > 2 * sum (Java long: wrapping adds, signed compare) it emits
// REMOVE c for every c in C, drops them, adds e and emits ADD e.  M is always a matching, so |C| <= 2 and the
// state is per vertex.
//
// Event order.  Per arriving edge the events are the reference's as a set, every REMOVE before the ADD, as in
// the reference.  Between two REMOVEs the reference follows HashSet<Edge> iteration order (Tuple3.hashCode and
// the set's insertion history), which nothing here pins; this library emits the edge matched at the arriving
// edge's src first, then the one at its dst.
//
// Vertex table (HBM): slots[cap + 1] of 32 bytes {id, weight, link, reservation}, cap a power of two, linear
// probing from a murmur3 finaliser of the full int64 id, load <= 1/2, grown by doubling (re-insert) before a
// batch whose 2n endpoints could overflow it.  An empty slot's id is ~0 (the bits of vertex -1); vertex -1
// itself lives in the side slot slots[cap].  link = [flags | partner slot:32]: MT_MATCHED, and MT_SRC when the
// vertex is the src end of its stored edge (a REMOVE reproduces the stored (src, dst, val), not the arriving
// edge's orientation).  A stored self-loop (x, x) is x matched to itself.
//
// One batch of n edges, edge = its index i.  Rounds over the still-pending edges, driven from the host; a
// round's reservation words are tagged with the round's epoch, so no word is ever reset:
//   word(i) = epoch << 32 | (2^32 - 1 - i); atomicMax keeps the newest round's smallest index, and a word of an
//   earlier round is smaller than every word of this one (= unreserved).
//   k_mt_eval    pending edge i reads match[u], match[v]: footprint S_i = {u, v, partner(u), partner(v)} and
//                its tentative decision under the current state; an accepting edge reserves all of S_i
//   k_mt_block   to a fixed point: a rejecting, not yet blocked edge with an earlier reservation somewhere on
//                S_i becomes blocked and reserves S_i (it may flip to accept once an earlier edge commits, so
//                everything later on its footprint waits for it too).  The blocked set only grows.
//   k_mt_final   rejecting and not blocked: final, no events.  Accepting and holding all of S_i: commits --
//                the (at most 2) removed edges into per-edge scratch, freed partners cleared, itself written at
//                u and v.  Committing edges of a round hold disjoint footprints: their writes never collide.
//                Everything else goes to the next round's (compacted) pending list.
//   k_mt_tail    once the pending edges fit one workgroup it runs the remaining rounds in one launch, a thread
//                per edge, with __syncthreads() between the steps and nothing else
//   xscan + k_mt_emit   after the last round: events in index order
// The smallest pending index is final in every round, so pending strictly decreases: a round that finalises
// nothing ends the call with GS_EDEVICE.  No device-side waits, no grid-wide barriers.
// Every touched vertex is a batch endpoint or the batch-start partner of one; k_mt_insert saves those slots'
// (weight, link), and a call that cannot deliver (GS_ECAPACITY, an allocation) puts them back (k_mt_restore).
#include "gs_table.hpp"

namespace gs {

constexpr unsigned long long MT_MATCHED = 1ull << 32, MT_SRC = 1ull << 33;
constexpr uint32_t MT_NONE = 0xFFFFFFFFu;   // footprint entry: no vertex
constexpr int MT_TAIL = 1024;               // pending edges one workgroup finishes by itself
constexpr int MT_BLOCK_GROUP = 4;           // blocking iterations per read-back
// u64 words of gs_match::meta
enum { MT_ERR = 0, MT_FRESH = 1, MT_PEND = 2, MT_CHG = 3, MT_DCNT = 7, MT_DW = 8, MT_TROUNDS = 9, MT_TBLK = 10, MT_PA = 11,
       MT_META = 16 };

struct MtSlot {
  unsigned long long id, wgt, link, resv;
};

struct MtTable {
  MtSlot* slots;       // [cap + 1]; [cap]: vertex -1
  ulonglong2* saved;   // [cap + 1] (weight, link) at the start of the running batch
  unsigned long long mask;   // cap - 1
  unsigned long long* meta;
};

// the slot of `id`, claimed if absent (*fresh); vertex -1: the side slot, never fresh; MT_NONE (what tab_claim's
// ~0 narrows to: slots stay below 2^31) when the table is full
__device__ __forceinline__ uint32_t mt_slot(const MtTable& t, unsigned long long id, bool* fresh) {
  *fresh = false;
  if (id == TAB_EMPTY) return (uint32_t)(t.mask + 1);
  return (uint32_t)tab_claim<sizeof(MtSlot) / 8>(&t.slots->id, t.mask, id, fresh);
}

__device__ __forceinline__ unsigned long long mt_word(uint32_t epoch, uint32_t i) {
  return ((unsigned long long)epoch << 32) | (0xFFFFFFFFu - i);
}
__device__ __forceinline__ unsigned long long mt_resv(const MtSlot* sl, uint32_t x) {
  return __hip_atomic_load(&sl[x].resv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void mt_reserve(MtSlot* sl, const uint32_t fp[4], unsigned long long mine) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (fp[k] != MT_NONE) atomicMax(&sl[fp[k]].resv, mine);
}
// some vertex of the footprint carries an earlier edge's reservation of this round
__device__ __forceinline__ bool mt_behind(const MtSlot* sl, const uint32_t fp[4], unsigned long long mine) {
  bool b = false;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (fp[k] != MT_NONE) b |= mt_resv(sl, fp[k]) > mine;
  return b;
}
__device__ __forceinline__ bool mt_holds(const MtSlot* sl, const uint32_t fp[4], unsigned long long mine) {
  bool h = true;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (fp[k] != MT_NONE) h &= mt_resv(sl, fp[k]) == mine;
  return h;
}

// the matched edges at slots a (the arriving edge's src) and b (its dst): is there one at a, and another one
// at b (u matched to v, or a self-loop, is one edge: the HashSet counts it once)
__device__ __forceinline__ void mt_collisions(unsigned long long la, unsigned long long lb, uint32_t a, uint32_t b, bool* ma,
                                              bool* mb) {
  *ma = (la & MT_MATCHED) != 0;
  *mb = (lb & MT_MATCHED) != 0 && b != a && !(*ma && (uint32_t)la == b);
}

// footprint and tentative decision of edge (a, b, w) under the current state
__device__ __forceinline__ bool mt_evaluate(const MtSlot* sl, uint32_t a, uint32_t b, long long w, uint32_t fp[4]) {
  const unsigned long long la = sl[a].link, lb = sl[b].link;
  bool ma, mb;
  mt_collisions(la, lb, a, b, &ma, &mb);
  const uint32_t pa = ma ? (uint32_t)la : MT_NONE, pb = mb ? (uint32_t)lb : MT_NONE;
  fp[0] = a;
  fp[1] = b != a ? b : MT_NONE;
  fp[2] = (pa != a && pa != b) ? pa : MT_NONE;
  fp[3] = (pb != a && pb != b) ? pb : MT_NONE;
  const unsigned long long sum = (ma ? sl[a].wgt : 0ull) + (mb ? sl[b].wgt : 0ull);   // Java long: wraps
  return w > (long long)(2ull * sum);
}

// edge i = (u, v, w) at slots (a, b) enters the matching: removed edges -> rem[6i ..], nev[i] = events
__device__ __forceinline__ void mt_commit(MtSlot* sl, uint32_t a, uint32_t b, uint64_t i, long long u, long long v, long long w,
                                          uint64_t* __restrict__ nev, long long* __restrict__ rem) {
  const unsigned long long la = sl[a].link, lb = sl[b].link;
  bool ma, mb;
  mt_collisions(la, lb, a, b, &ma, &mb);
  const uint32_t pa = (uint32_t)la, pb = (uint32_t)lb;
  long long* r = rem + 6 * i;
  if (ma) {
    const long long p = (long long)sl[pa].id;
    const bool src_end = (la & MT_SRC) != 0;
    r[0] = src_end ? u : p;
    r[1] = src_end ? p : u;
    r[2] = (long long)sl[a].wgt;
    r += 3;
  }
  if (mb) {
    const long long p = (long long)sl[pb].id;
    const bool src_end = (lb & MT_SRC) != 0;
    r[0] = src_end ? v : p;
    r[1] = src_end ? p : v;
    r[2] = (long long)sl[b].wgt;
  }
  if (ma) sl[pa].link = 0;
  if (mb) sl[pb].link = 0;
  sl[a].wgt = (unsigned long long)w;
  sl[a].link = MT_MATCHED | MT_SRC | b;
  if (b != a) {
    sl[b].wgt = (unsigned long long)w;
    sl[b].link = MT_MATCHED | a;
  }
  nev[i] = 1 + (ma ? 1 : 0) + (mb ? 1 : 0);
}

__device__ __forceinline__ void mt_save(const MtTable& t, uint32_t s) {
  const unsigned long long l = t.slots[s].link;
  t.saved[s] = make_ulonglong2(t.slots[s].wgt, l);
  if (l & MT_MATCHED) {
    const uint32_t p = (uint32_t)l;
    t.saved[p] = make_ulonglong2(t.slots[p].wgt, t.slots[p].link);
  }
}

// lane per edge: the slots of its endpoints (claimed if new), their state and their partners' saved, pend[i] = i.
// Lanes that save one slot write the same words (the matching does not change in this kernel).
__global__ __launch_bounds__(256) void k_mt_insert(MtTable t, const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                   uint64_t n, uint32_t* __restrict__ su, uint32_t* __restrict__ sv,
                                                   uint32_t* __restrict__ pend) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long n_fresh = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    bool fa, fb;
    const uint32_t a = mt_slot(t, (unsigned long long)bs[i], &fa);
    const uint32_t b = mt_slot(t, (unsigned long long)bd[i], &fb);
    n_fresh += (fa ? 1 : 0) + (fb ? 1 : 0);
    if (a == MT_NONE || b == MT_NONE) {
      atomicOr(&t.meta[MT_ERR], 1ull);
      su[i] = sv[i] = (uint32_t)(t.mask + 1);   // a valid slot: later kernels stay in bounds
    } else {
      su[i] = a;
      sv[i] = b;
      mt_save(t, a);
      mt_save(t, b);
    }
    if (pend) pend[i] = (uint32_t)i;
  }
  block_add(&t.meta[MT_FRESH], n_fresh, s_part);
}

// a batch that cannot deliver: every slot it may have touched back to its saved (weight, link)
__global__ __launch_bounds__(256) void k_mt_restore(MtTable t, uint64_t n, const uint32_t* __restrict__ su,
                                                    const uint32_t* __restrict__ sv) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t s = e ? sv[i] : su[i];
      const ulonglong2 o = t.saved[s];
      t.slots[s].wgt = o.x;
      t.slots[s].link = o.y;
      if (o.y & MT_MATCHED) {
        const uint32_t p = (uint32_t)o.y;
        const ulonglong2 q = t.saved[p];
        t.slots[p].wgt = q.x;
        t.slots[p].link = q.y;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_mt_eval(MtTable t, const uint32_t* __restrict__ pend, uint32_t cnt,
                                                 const uint32_t* __restrict__ su, const uint32_t* __restrict__ sv,
                                                 const int64_t* __restrict__ bw, uint32_t epoch, uint4* __restrict__ fps,
                                                 uint8_t* __restrict__ st) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < cnt; p += (uint64_t)gridDim.x * 256) {
    const uint32_t i = pend[p];
    uint32_t fp[4];
    const bool acc = mt_evaluate(t.slots, su[i], sv[i], bw[i], fp);
    fps[p] = make_uint4(fp[0], fp[1], fp[2], fp[3]);
    st[p] = acc ? 1 : 0;
    if (acc) mt_reserve(t.slots, fp, mt_word(epoch, i));
  }
}

// one blocking iteration; *chg = 1 when some edge became blocked
__global__ __launch_bounds__(256) void k_mt_block(MtTable t, const uint32_t* __restrict__ pend, uint32_t cnt, uint32_t epoch,
                                                  const uint4* __restrict__ fps, uint8_t* __restrict__ st,
                                                  unsigned long long* __restrict__ chg) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < cnt; p += (uint64_t)gridDim.x * 256) {
    if (st[p] != 0) continue;
    const uint4 f = fps[p];
    const uint32_t fp[4] = {f.x, f.y, f.z, f.w};
    const unsigned long long mine = mt_word(epoch, pend[p]);
    if (mt_behind(t.slots, fp, mine)) {
      st[p] = 2;
      mt_reserve(t.slots, fp, mine);
      *chg = 1ull;
    }
  }
}

__global__ __launch_bounds__(256) void k_mt_final(MtTable t, const uint32_t* __restrict__ pend, uint32_t cnt,
                                                  const uint32_t* __restrict__ su, const uint32_t* __restrict__ sv,
                                                  const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                  const int64_t* __restrict__ bw, uint32_t epoch, const uint4* __restrict__ fps,
                                                  const uint8_t* __restrict__ st, uint64_t* __restrict__ nev,
                                                  long long* __restrict__ rem, uint32_t* __restrict__ next) {
  const uint64_t rounded = ((uint64_t)cnt + 255) & ~255ull;   // whole waves reach the ballot
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < rounded; p += (uint64_t)gridDim.x * 256) {
    bool stay = false;
    uint32_t i = 0;
    if (p < cnt) {
      i = pend[p];
      const uint8_t s = st[p];
      if (s == 0) {
        nev[i] = 0;
      } else {
        const uint4 f = fps[p];
        const uint32_t fp[4] = {f.x, f.y, f.z, f.w};
        if (s == 1 && mt_holds(t.slots, fp, mt_word(epoch, i))) mt_commit(t.slots, su[i], sv[i], i, bs[i], bd[i], bw[i], nev, rem);
        else stay = true;
      }
    }
    const unsigned long long k = wave_compact_base(stay, &t.meta[MT_PEND]);
    if (stay) next[k] = i;
  }
}

// the remaining rounds of cnt <= MT_TAIL pending edges in one workgroup, a thread per edge.  round0: rounds
// done before (the pending counts after rounds 1, 2, 4 and 8 go to meta[MT_PA ..])
__global__ __launch_bounds__(MT_TAIL) void k_mt_tail(MtTable t, const uint32_t* __restrict__ pend, uint32_t cnt,
                                                     const uint32_t* __restrict__ su, const uint32_t* __restrict__ sv,
                                                     const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                     const int64_t* __restrict__ bw, uint32_t epoch0,
                                                     uint64_t* __restrict__ nev, long long* __restrict__ rem, uint32_t round0) {
  bool active = threadIdx.x < cnt;
  const uint32_t i = active ? pend[threadIdx.x] : 0;
  const uint32_t a = active ? su[i] : 0, b = active ? sv[i] : 0;
  const long long w = active ? bw[i] : 0;
  uint32_t rounds = 0, left = cnt;
  unsigned long long blk = 0;
  while (left && rounds <= cnt) {   // every round finalises its smallest pending index: at most cnt rounds
    const unsigned long long mine = mt_word(epoch0 + rounds, i);
    uint32_t fp[4] = {MT_NONE, MT_NONE, MT_NONE, MT_NONE};
    int s = 0;
    if (active) {
      s = mt_evaluate(t.slots, a, b, w, fp) ? 1 : 0;
      if (s) mt_reserve(t.slots, fp, mine);
    }
    __syncthreads();
    for (;;) {
      bool changed = false;
      if (active && s == 0 && mt_behind(t.slots, fp, mine)) {
        s = 2;
        mt_reserve(t.slots, fp, mine);
        changed = true;
      }
      ++blk;
      if (!__syncthreads_or(changed)) break;
    }
    bool fin = false;
    if (active) {
      if (s == 0) {
        nev[i] = 0;
        fin = true;
      } else if (s == 1 && mt_holds(t.slots, fp, mine)) {
        mt_commit(t.slots, a, b, i, bs[i], bd[i], w, nev, rem);
        fin = true;
      }
    }
    if (fin) active = false;
    const uint32_t now = (uint32_t)__syncthreads_count(active);
    ++rounds;
    if (threadIdx.x == 0) {
      const uint32_t r = round0 + rounds;
      if (r == 1 || r == 2 || r == 4 || r == 8) t.meta[MT_PA + (r == 1 ? 0 : r == 2 ? 1 : r == 4 ? 2 : 3)] = now;
    }
    if (now == left) break;   // nothing finalised: reported through meta[MT_PEND]
    left = now;
  }
  if (threadIdx.x == 0) {
    t.meta[MT_PEND] = left;
    t.meta[MT_TROUNDS] = rounds;
    t.meta[MT_TBLK] = blk;
  }
}

struct MtOut {
  uint8_t* type;
  int64_t* src;
  int64_t* dst;
  int64_t* val;
  uint64_t* index;
};

// lane per edge: its events at rows pos[i] .. (REMOVE of the edge matched at its src, then at its dst, then
// its ADD); meta[MT_DCNT] / [MT_DW] += the change of |M| and of M's summed values (wrapping)
__global__ __launch_bounds__(256) void k_mt_emit(const int64_t* __restrict__ bs, const int64_t* __restrict__ bd,
                                                 const int64_t* __restrict__ bw, uint64_t n, const uint64_t* __restrict__ nev,
                                                 const uint64_t* __restrict__ pos, const long long* __restrict__ rem, MtOut o,
                                                 unsigned long long* __restrict__ meta) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long dcnt = 0, dw = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t e = nev[i];
    if (!e) continue;
    uint64_t k = pos[i];
    const long long* r = rem + 6 * i;
    for (uint64_t j = 0; j + 1 < e; ++j, ++k, r += 3) {
      if (o.type) o.type[k] = 1;
      if (o.src) o.src[k] = r[0];
      if (o.dst) o.dst[k] = r[1];
      if (o.val) o.val[k] = r[2];
      if (o.index) o.index[k] = i;
      dw -= (unsigned long long)r[2];
    }
    if (o.type) o.type[k] = 0;
    if (o.src) o.src[k] = bs[i];
    if (o.dst) o.dst[k] = bd[i];
    if (o.val) o.val[k] = bw[i];
    if (o.index) o.index[k] = i;
    dw += (unsigned long long)bw[i];
    dcnt += 2ull - e;
  }
  block_add(&meta[MT_DCNT], dcnt, s_part);
  block_add(&meta[MT_DW], dw, s_part);
}

// every slot free and unmatched; the side slot's id is vertex -1 from the start
__global__ __launch_bounds__(256) void k_mt_clear(MtSlot* __restrict__ slots, uint64_t cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= cap; s += (uint64_t)gridDim.x * 256)
    slots[s] = MtSlot{TAB_EMPTY, 0ull, 0ull, 0ull};
}

// the epoch counter is about to wrap: every reservation word back to "no round"
__global__ __launch_bounds__(256) void k_mt_clear_resv(MtSlot* __restrict__ slots, uint64_t cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= cap; s += (uint64_t)gridDim.x * 256) slots[s].resv = 0;
}

// growth, step 1: every vertex of the old table into the new one with its weight; map[old slot] = new slot
__global__ __launch_bounds__(256) void k_mt_rehash(const MtSlot* __restrict__ os, uint64_t ocap, MtTable t,
                                                   uint32_t* __restrict__ map) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= ocap; s += (uint64_t)gridDim.x * 256) {
    const unsigned long long id = os[s].id;
    if (s < ocap && id == TAB_EMPTY) continue;
    bool fresh;
    const uint32_t d = mt_slot(t, id, &fresh);
    map[s] = d;
    if (d == MT_NONE) atomicOr(&t.meta[MT_ERR], 1ull);
    else t.slots[d].wgt = os[s].wgt;
  }
}
// step 2: the links, partner slots translated
__global__ __launch_bounds__(256) void k_mt_relink(const MtSlot* __restrict__ os, uint64_t ocap, MtSlot* __restrict__ ns,
                                                   const uint32_t* __restrict__ map) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= ocap; s += (uint64_t)gridDim.x * 256) {
    const unsigned long long l = os[s].link;
    if (!(l & MT_MATCHED) || (s < ocap && os[s].id == TAB_EMPTY)) continue;
    const uint32_t d = map[s], p = map[(uint32_t)l];
    if (d != MT_NONE && p != MT_NONE) ns[d].link = (l & ~0xFFFFFFFFull) | p;
  }
}

// checkpoint: the matched edges (at their src ends) as (src ^ sign bit, row) sort keys and (src, dst, val)
// rows, in any order; M rows expected
__global__ __launch_bounds__(256) void k_mt_dump(MtTable t, unsigned long long* __restrict__ keys, uint32_t* __restrict__ rows,
                                                 int64_t* __restrict__ es, int64_t* __restrict__ ed, int64_t* __restrict__ ew,
                                                 uint64_t M) {
  const uint64_t cap = t.mask + 1;
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= cap; s += (uint64_t)gridDim.x * 256) {
    const unsigned long long l = t.slots[s].link;
    if ((l & (MT_MATCHED | MT_SRC)) != (MT_MATCHED | MT_SRC)) continue;
    const unsigned long long k = atomicAdd(&t.meta[MT_PEND], 1ull);
    if (k >= M) continue;
    const unsigned long long id = t.slots[s].id;
    keys[k] = id ^ TAB_SIGN;
    rows[k] = (uint32_t)k;
    es[k] = (int64_t)id;
    ed[k] = (int64_t)t.slots[(uint32_t)l].id;
    ew[k] = (int64_t)t.slots[s].wgt;
  }
}
__global__ __launch_bounds__(256) void k_mt_gather(const uint32_t* __restrict__ rows, uint64_t M, const int64_t* __restrict__ es,
                                                   const int64_t* __restrict__ ed, const int64_t* __restrict__ ew,
                                                   int64_t* __restrict__ os, int64_t* __restrict__ od, int64_t* __restrict__ ow) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < M; r += (uint64_t)gridDim.x * 256) {
    const uint32_t k = rows[r];
    if (os) os[r] = es[k];
    if (od) od[r] = ed[k];
    if (ow) ow[r] = ew[k];
  }
}

// restore: every row reserves its two endpoints; a row that does not hold both shares one with another row
__global__ __launch_bounds__(256) void k_mt_import_claim(MtTable t, uint64_t n, const uint32_t* __restrict__ su,
                                                         const uint32_t* __restrict__ sv, uint32_t epoch) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const unsigned long long mine = mt_word(epoch, (uint32_t)i);
    atomicMax(&t.slots[su[i]].resv, mine);
    atomicMax(&t.slots[sv[i]].resv, mine);
  }
}
__global__ __launch_bounds__(256) void k_mt_import_check(MtTable t, uint64_t n, const uint32_t* __restrict__ su,
                                                         const uint32_t* __restrict__ sv, uint32_t epoch) {
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const unsigned long long mine = mt_word(epoch, (uint32_t)i);
    bad |= mt_resv(t.slots, su[i]) != mine || mt_resv(t.slots, sv[i]) != mine;
  }
  if (bad) atomicOr(&t.meta[MT_ERR], 2ull);
}
__global__ __launch_bounds__(256) void k_mt_import_write(MtTable t, uint64_t n, const uint32_t* __restrict__ su,
                                                         const uint32_t* __restrict__ sv, const int64_t* __restrict__ bw) {
  __shared__ unsigned long long s_part[TAB_PART];
  unsigned long long dw = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t a = su[i], b = sv[i];
    const unsigned long long w = (unsigned long long)bw[i];
    t.slots[a].wgt = w;
    t.slots[a].link = MT_MATCHED | MT_SRC | b;
    if (b != a) {
      t.slots[b].wgt = w;
      t.slots[b].link = MT_MATCHED | a;
    }
    dw += w;
  }
  block_add(&t.meta[MT_DW], dw, s_part);
}

}  // namespace gs

using namespace gs;

struct gs_match {
  int device = 0;
  MtSlot* slots = nullptr;        // device [cap + 1]
  ulonglong2* saved = nullptr;    // device [cap + 1]
  unsigned long long* meta = nullptr;   // device u64[MT_META]
  uint64_t cap = 0;               // slots (power of two)
  uint64_t vertices = 0;          // occupied slots of the table (vertex -1 not counted: it has its own)
  uint64_t matched = 0, records = 0, growths = 0;
  uint64_t total_weight = 0;      // wrapped sum of M's values
  uint32_t epoch = 0;             // the last round's tag of the reservation words
  uint64_t rounds = 0, block_iters = 0, pending_after[4] = {0, 0, 0, 0};   // the last batch
  bool broken = false;            // a batch failed on the device midway
};

namespace {

constexpr uint64_t MT_MAX_CAP = 1ull << 31;   // slot numbers are 32-bit, cap itself is vertex -1's

MtTable table_of(const gs_match* t) { return MtTable{t->slots, t->saved, t->cap - 1, t->meta}; }

gs_status alloc_table(gs_ctx* c, uint64_t cap, MtSlot** slots, ulonglong2** saved) {
  *slots = nullptr;
  *saved = nullptr;
  if (cap > MT_MAX_CAP || hipMalloc((void**)slots, (cap + 1) * sizeof(MtSlot)) != hipSuccess ||
      hipMalloc((void**)saved, (cap + 1) * sizeof(ulonglong2)) != hipSuccess) {
    (void)hipGetLastError();
    if (*slots) hipFree(*slots);
    *slots = nullptr;
    *saved = nullptr;
    return set_error(c, GS_ENOMEM, "matching state: a vertex table of %llu slots does not fit", (unsigned long long)cap);
  }
  hipLaunchKernelGGL(k_mt_clear, dim3(tab_grid(cap + 1)), dim3(256), 0, c->stream, *slots, cap);
  const gs_status st = hip_check(c, hipGetLastError(), "k_mt_clear");
  if (st != GS_OK) {
    hipFree(*slots);
    hipFree(*saved);
    *slots = nullptr;
    *saved = nullptr;
  }
  return st;
}

// room for `need` vertices at load <= 1/2: grow by doubling (allocate, re-insert, swap).  On any failure the
// old table stays as it was.
gs_status reserve(gs_ctx* c, gs_match* t, uint64_t need) {
  if (need <= t->cap / 2) return GS_OK;
  uint64_t cap, doublings;
  if (!tab_plan_growth(t->cap, need, MT_MAX_CAP, &cap, &doublings))
    return set_error(c, GS_ENOMEM, "matching state: %llu vertices", (unsigned long long)need);
  GS_TRY(ensure(c, c->ts[9], (t->cap + 1) * 4));
  MtSlot* ns;
  ulonglong2* nsv;
  GS_TRY(alloc_table(c, cap, &ns, &nsv));
  uint32_t* map = c->ts[9].as<uint32_t>();
  // the error word is this re-insert's alone: whatever an earlier call left in it is not a failed re-insert
  gs_status pre = hip_check(c, hipMemsetAsync(t->meta + MT_ERR, 0, 8, c->stream), "hipMemsetAsync");
  if (pre != GS_OK) {
    hipFree(ns);
    hipFree(nsv);
    return pre;
  }
  hipLaunchKernelGGL(k_mt_rehash, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, (const MtSlot*)t->slots, t->cap,
                     MtTable{ns, nsv, cap - 1, t->meta}, map);
  gs_status st = hip_check(c, hipGetLastError(), "k_mt_rehash");
  if (st == GS_OK) {
    hipLaunchKernelGGL(k_mt_relink, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, (const MtSlot*)t->slots, t->cap, ns,
                       (const uint32_t*)map);
    st = hip_check(c, hipGetLastError(), "k_mt_relink");
  }
  if (st == GS_OK) st = tab_read_meta(c, t->meta, MT_META);
  if (st == GS_OK && c->host_small[8 + MT_ERR]) {
    hipMemsetAsync(t->meta + MT_ERR, 0, 8, c->stream);
    st = set_error(c, GS_EDEVICE, "matching state: re-insert failed");
  }
  if (st != GS_OK) {
    hipFree(ns);
    hipFree(nsv);
    return st;
  }
  hipFree(t->slots);
  hipFree(t->saved);
  t->slots = ns;
  t->saved = nsv;
  t->cap = cap;
  t->growths += doublings;
  return GS_OK;
}

gs_status check_state(gs_ctx* c, const gs_match* t) {
  if (!c) return GS_EINVAL;
  if (!t) return set_error(c, GS_EINVAL, "null matching state");
  if (t->device != c->device)
    return set_error(c, GS_EINVAL, "matching state lives on device %d, the ctx on device %d", t->device, c->device);
  if (t->broken) return set_error(c, GS_EDEVICE, "matching state: an earlier batch failed on the device");
  return GS_OK;
}

// room for the round tags of a batch of n edges; the words start over before the 32-bit tag would wrap
gs_status reserve_epochs(gs_ctx* c, gs_match* t, uint64_t n) {
  if ((uint64_t)t->epoch + n + 2 < (1ull << 32)) return GS_OK;
  hipLaunchKernelGGL(k_mt_clear_resv, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, t->slots, t->cap);
  GS_HIP(hipGetLastError());
  t->epoch = 0;
  return GS_OK;
}

// the scratch columns of a batch of n edges: slots of the endpoints
gs_status ensure_slots(gs_ctx* c, uint64_t n) {
  GS_TRY(ensure(c, c->ts[0], n * 4));
  return ensure(c, c->ts[1], n * 4);
}

// k_mt_insert over the batch (its table claims are kept whatever happens next: an unmatched vertex changes
// nothing the state shows)
gs_status insert_batch(gs_ctx* c, gs_match* t, const int64_t* src, const int64_t* dst, uint64_t n, uint32_t* pend) {
  GS_HIP(hipMemsetAsync(t->meta, 0, MT_META * 8, c->stream));
  t->broken = true;
  hipLaunchKernelGGL(k_mt_insert, dim3(tab_grid_tab(n)), dim3(256), 0, c->stream, table_of(t), src, dst, n,
                     c->ts[0].as<uint32_t>(), c->ts[1].as<uint32_t>(), pend);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, MT_META));
  if (c->host_small[8 + MT_ERR]) return set_error(c, GS_EDEVICE, "matching state: the vertex table filled up");
  t->vertices += c->host_small[8 + MT_FRESH];
  t->broken = false;
  return GS_OK;
}

// the rounds of one batch (see the head of this file); the matching changes from the first k_mt_final on
gs_status run_rounds(gs_ctx* c, gs_match* t, const int64_t* src, const int64_t* dst, const int64_t* val, uint64_t n) {
  const uint32_t *su = c->ts[0].as<uint32_t>(), *sv = c->ts[1].as<uint32_t>();
  uint32_t *cur = c->ts[2].as<uint32_t>(), *nxt = c->ts[3].as<uint32_t>();
  uint4* fps = c->ts[4].as<uint4>();
  uint8_t* st = c->ts[5].as<uint8_t>();
  uint64_t* nev = c->ts[6].as<uint64_t>();
  long long* rem = c->ts[8].as<long long>();
  const MtTable tab = table_of(t);
  uint64_t cnt = n;
  t->rounds = t->block_iters = 0;
  for (int k = 0; k < 4; ++k) t->pending_after[k] = 0;
  while (cnt) {
    if (cnt <= (uint64_t)MT_TAIL) {
      hipLaunchKernelGGL(k_mt_tail, dim3(1), dim3(MT_TAIL), 0, c->stream, tab, (const uint32_t*)cur, (uint32_t)cnt, su, sv, src,
                         dst, val, t->epoch + 1, nev, rem, (uint32_t)std::min<uint64_t>(t->rounds, 1u << 30));
      GS_HIP(hipGetLastError());
      GS_TRY(tab_read_meta(c, t->meta, MT_META));
      const uint64_t* m = c->host_small + 8;
      t->epoch += (uint32_t)m[MT_TROUNDS];
      for (int k = 0; k < 4; ++k)
        if (t->rounds < (1ull << k) && t->rounds + m[MT_TROUNDS] >= (1ull << k)) t->pending_after[k] = m[MT_PA + k];
      t->rounds += m[MT_TROUNDS];
      t->block_iters += m[MT_TBLK];
      if (m[MT_PEND]) return set_error(c, GS_EDEVICE, "matching state: a round finalised no edge (%llu pending)",
                                       (unsigned long long)m[MT_PEND]);
      break;
    }
    const uint32_t epoch = ++t->epoch;
    const dim3 g(tab_grid(cnt)), b(256);
    GS_HIP(hipMemsetAsync(t->meta + MT_PEND, 0, (1 + MT_BLOCK_GROUP) * 8, c->stream));
    hipLaunchKernelGGL(k_mt_eval, g, b, 0, c->stream, tab, (const uint32_t*)cur, (uint32_t)cnt, su, sv, val, epoch, fps, st);
    GS_HIP(hipGetLastError());
    for (uint64_t groups = 0;; ++groups) {
      // every changing iteration blocks at least one edge: cnt of them at the most
      if (groups * MT_BLOCK_GROUP > cnt + MT_BLOCK_GROUP) return set_error(c, GS_EDEVICE, "matching state: blocking did not settle");
      for (int k = 0; k < MT_BLOCK_GROUP; ++k)
        hipLaunchKernelGGL(k_mt_block, g, b, 0, c->stream, tab, (const uint32_t*)cur, (uint32_t)cnt, epoch, (const uint4*)fps, st,
                           t->meta + MT_CHG + k);
      GS_HIP(hipGetLastError());
      GS_TRY(tab_read_meta(c, t->meta, MT_META));
      int done = 0;
      while (done < MT_BLOCK_GROUP && c->host_small[8 + MT_CHG + done]) ++done;
      t->block_iters += std::min(done + 1, MT_BLOCK_GROUP);
      if (done < MT_BLOCK_GROUP) break;
      GS_HIP(hipMemsetAsync(t->meta + MT_CHG, 0, MT_BLOCK_GROUP * 8, c->stream));
    }
    hipLaunchKernelGGL(k_mt_final, g, b, 0, c->stream, tab, (const uint32_t*)cur, (uint32_t)cnt, su, sv, src, dst, val, epoch,
                       (const uint4*)fps, (const uint8_t*)st, nev, rem, nxt);
    GS_HIP(hipGetLastError());
    GS_TRY(tab_read_meta(c, t->meta, MT_META));
    const uint64_t left = c->host_small[8 + MT_PEND];
    ++t->rounds;
    for (int k = 0; k < 4; ++k)
      if (t->rounds == (1ull << k)) t->pending_after[k] = left;
    if (left >= cnt) return set_error(c, GS_EDEVICE, "matching state: a round finalised no edge (%llu pending)",
                                      (unsigned long long)left);
    cnt = left;
    std::swap(cur, nxt);
  }
  return GS_OK;
}

gs_status restore_batch(gs_ctx* c, gs_match* t, uint64_t n) {
  hipLaunchKernelGGL(k_mt_restore, dim3(tab_grid(n)), dim3(256), 0, c->stream, table_of(t), n, (const uint32_t*)c->ts[0].p,
                     (const uint32_t*)c->ts[1].p);
  GS_HIP(hipGetLastError());
  GS_TRY(host_wait(c));
  t->broken = false;
  return GS_OK;
}

}  // namespace

extern "C" {

gs_status gs_match_create(gs_ctx* c, uint64_t reserve_vertices, gs_match** out) {
  if (!c) return GS_EINVAL;
  if (!out) return set_error(c, GS_EINVAL, "gs_match_create: null argument");
  *out = nullptr;
  if (reserve_vertices > MT_MAX_CAP / 2)
    return set_error(c, GS_ENOMEM, "gs_match_create: %llu vertices", (unsigned long long)reserve_vertices);
  (void)hipGetLastError();
  GS_HIP(hipSetDevice(c->device));
  gs_match* t = new (std::nothrow) gs_match();
  if (!t) return set_error(c, GS_ENOMEM, "gs_match_create");
  t->device = c->device;
  t->cap = 64;
  while (t->cap / 2 < reserve_vertices) t->cap *= 2;
  gs_status st = alloc_table(c, t->cap, &t->slots, &t->saved);
  if (st == GS_OK && hipMalloc((void**)&t->meta, MT_META * 8) != hipSuccess) {
    (void)hipGetLastError();
    st = set_error(c, GS_ENOMEM, "gs_match_create: state words");
  }
  if (st == GS_OK) st = hip_check(c, hipMemsetAsync(t->meta, 0, MT_META * 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) st = host_wait(c);
  if (st != GS_OK) {
    gs_match_destroy(t);
    return st;
  }
  *out = t;
  return GS_OK;
}

void gs_match_destroy(gs_match* t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->slots) hipFree(t->slots);
  if (t->saved) hipFree(t->saved);
  if (t->meta) hipFree(t->meta);
  delete t;
}

gs_status gs_match_size(const gs_match* t, uint64_t* matched_edges, uint64_t* records, int64_t* total_weight) {
  if (!t) return GS_EINVAL;
  if (matched_edges) *matched_edges = t->matched;
  if (records) *records = t->records;
  if (total_weight) *total_weight = (int64_t)t->total_weight;
  return GS_OK;
}

gs_status gs_match_capacity(const gs_match* t, uint64_t* slots, uint64_t* growths) {
  if (!t) return GS_EINVAL;
  if (slots) *slots = t->cap;
  if (growths) *growths = t->growths;
  return GS_OK;
}

gs_status gs_match_last_batch(const gs_match* t, uint64_t* rounds, uint64_t* block_iterations, uint64_t* pending_after) {
  if (!t) return GS_EINVAL;
  if (rounds) *rounds = t->rounds;
  if (block_iterations) *block_iterations = t->block_iters;
  if (pending_after)
    for (int k = 0; k < 4; ++k) pending_after[k] = t->pending_after[k];
  return GS_OK;
}

gs_status gs_match_edges(gs_ctx* c, gs_match* t, const gs_edge_batch* b, gs_match_out* out) {
  GS_TRY(check_state(c, t));
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (!out || !out->n_out) return set_error(c, GS_EINVAL, "bad gs_match_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_match_out.mem %d", out->mem);
  if (b->val_dtype != GS_I64 || (b->n && !b->val))
    return set_error(c, GS_EUNSUPPORTED, "gs_match_edges: the edge values are I64 (Edge<Long, Long>)");
  const uint64_t n = b->n;
  const bool any = out->type || out->src || out->dst || out->val || out->index;
  GS_TRY(begin_call(c));
  *out->n_out = 0;
  if (n == 0) return GS_OK;
  // everything a batch of n edges needs, before the first write to the table
  GS_TRY(ensure_slots(c, n));
  GS_TRY(ensure(c, c->ts[2], n * 4));
  GS_TRY(ensure(c, c->ts[3], n * 4));
  GS_TRY(ensure(c, c->ts[4], n * 16));
  GS_TRY(ensure(c, c->ts[5], n));
  GS_TRY(ensure(c, c->ts[6], n * 8));
  GS_TRY(ensure(c, c->ts[7], (n + 1) * 8));
  GS_TRY(ensure(c, c->ts[8], n * 48));
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, true));
  GS_TRY(reserve(c, t, t->vertices + 2 * n));
  GS_TRY(reserve_epochs(c, t, n));
  GS_TRY(insert_batch(c, t, src, dst, n, c->ts[2].as<uint32_t>()));
  // ---- the matching changes from here on ----
  t->broken = true;
  GS_TRY(run_rounds(c, t, src, dst, (const int64_t*)val, n));
  uint64_t* nev = c->ts[6].as<uint64_t>();
  uint64_t* pos = c->ts[7].as<uint64_t>();
  {
    const gs_status sc = xscan(c, nev, n, pos);   // allocates its tile sums: the one allocation after the rounds
    if (sc == GS_ENOMEM) {
      const std::string why = c->err;
      GS_TRY(restore_batch(c, t, n));
      return set_error(c, sc, "%s", why.c_str());
    }
    GS_TRY(sc);
  }
  GS_HIP(hipMemcpyAsync(c->host_small + 8 + MT_META, pos + n, 8, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(host_wait(c));
  const uint64_t E = c->host_small[8 + MT_META];
  if (E > 3 * n) return set_error(c, GS_EDEVICE, "matching state: %llu events of %llu edges", (unsigned long long)E,
                                  (unsigned long long)n);
  *out->n_out = E;
  if (any && out->capacity < E) {
    GS_TRY(restore_batch(c, t, n));
    return set_error(c, GS_ECAPACITY, "output needs room for %llu events", (unsigned long long)E);
  }
  const bool direct = out->mem == GS_MEM_DEVICE;
  MtOut o{out->type, out->src, out->dst, out->val, out->index};
  if (!direct && any && E) {
    gs_status st = GS_OK;
    if (out->type && (st = ensure(c, c->ts[10], E)) == GS_OK) o.type = c->ts[10].as<uint8_t>();
    if (st == GS_OK && out->src && (st = ensure(c, c->out_keys, E * 8)) == GS_OK) o.src = c->out_keys.as<int64_t>();
    if (st == GS_OK && out->dst && (st = ensure(c, c->out_a, E * 8)) == GS_OK) o.dst = c->out_a.as<int64_t>();
    if (st == GS_OK && out->val && (st = ensure(c, c->out_b, E * 8)) == GS_OK) o.val = c->out_b.as<int64_t>();
    if (st == GS_OK && out->index && (st = ensure(c, c->aux, E * 8)) == GS_OK) o.index = c->aux.as<uint64_t>();
    if (st != GS_OK) {
      *out->n_out = 0;
      const std::string why = c->err;
      GS_TRY(restore_batch(c, t, n));
      return set_error(c, st, "%s", why.c_str());
    }
  }
  hipLaunchKernelGGL(k_mt_emit, dim3(tab_grid_tab(n)), dim3(256), 0, c->stream, src, dst, (const int64_t*)val, n,
                     (const uint64_t*)nev, (const uint64_t*)pos, (const long long*)c->ts[8].p, o, t->meta);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, MT_META));
  t->matched += c->host_small[8 + MT_DCNT];
  t->total_weight += c->host_small[8 + MT_DW];
  t->records += n;
  t->broken = false;
  if (!direct && any && E) {
    if (out->type) GS_TRY(deliver(c, out->type, o.type, E, out->mem));
    if (out->src) GS_TRY(deliver(c, out->src, o.src, E * 8, out->mem));
    if (out->dst) GS_TRY(deliver(c, out->dst, o.dst, E * 8, out->mem));
    if (out->val) GS_TRY(deliver(c, out->val, o.val, E * 8, out->mem));
    if (out->index) GS_TRY(deliver(c, out->index, o.index, E * 8, out->mem));
    GS_TRY(host_wait(c));
  }
  return GS_OK;
}

gs_status gs_match_export(gs_ctx* c, const gs_match* t, gs_edge_out* out) {
  GS_TRY(check_state(c, t));
  if (!out || !out->n_out) return set_error(c, GS_EINVAL, "bad gs_edge_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_edge_out.mem %d", out->mem);
  if (out->index) return set_error(c, GS_EINVAL, "gs_match_export writes src, dst and val only");
  const uint64_t M = t->matched;
  *out->n_out = M;
  if (out->capacity < M) return set_error(c, GS_ECAPACITY, "output needs %llu edges", (unsigned long long)M);
  GS_TRY(begin_call(c));
  if (M == 0) return GS_OK;
  GS_TRY(ensure(c, c->ts[0], M * 8));
  GS_TRY(ensure(c, c->ts[1], M * 4));
  GS_TRY(ensure(c, c->ts[2], M * 8));
  GS_TRY(ensure(c, c->ts[3], M * 8));
  GS_TRY(ensure(c, c->ts[4], M * 8));
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t *os = out->src, *od = out->dst, *ow = (int64_t*)out->val;
  if (!direct) {
    if (os) {
      GS_TRY(ensure(c, c->out_keys, M * 8));
      os = c->out_keys.as<int64_t>();
    }
    if (od) {
      GS_TRY(ensure(c, c->out_a, M * 8));
      od = c->out_a.as<int64_t>();
    }
    if (ow) {
      GS_TRY(ensure(c, c->out_b, M * 8));
      ow = c->out_b.as<int64_t>();
    }
  }
  unsigned long long* keys = c->ts[0].as<unsigned long long>();
  int64_t *es = c->ts[2].as<int64_t>(), *ed = c->ts[3].as<int64_t>(), *ew = c->ts[4].as<int64_t>();
  GS_HIP(hipMemsetAsync(t->meta + MT_PEND, 0, 8, c->stream));
  hipLaunchKernelGGL(k_mt_dump, dim3(tab_grid(t->cap + 1)), dim3(256), 0, c->stream, table_of(t), keys, c->ts[1].as<uint32_t>(),
                     es, ed, ew, M);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, MT_META));
  if (c->host_small[8 + MT_PEND] != M)
    return set_error(c, GS_EDEVICE, "matching state: %llu edges in the table, %llu expected",
                     (unsigned long long)c->host_small[8 + MT_PEND], (unsigned long long)M);
  // a vertex is in one matched edge at the most: the src ids are distinct, and ascending (src, dst) is
  // ascending src = ascending (src ^ sign bit) as unsigned
  Sorted s;
  GS_TRY(sort_buffer(c, (const uint64_t*)keys, c->ts[1].p, M, &s, 64, 4));
  hipLaunchKernelGGL(k_mt_gather, dim3(tab_grid(M)), dim3(256), 0, c->stream, (const uint32_t*)s.vals, M, (const int64_t*)es,
                     (const int64_t*)ed, (const int64_t*)ew, os, od, ow);
  GS_HIP(hipGetLastError());
  if (direct) return GS_OK;
  if (out->src) GS_TRY(deliver(c, out->src, os, M * 8, out->mem));
  if (out->dst) GS_TRY(deliver(c, out->dst, od, M * 8, out->mem));
  if (out->val) GS_TRY(deliver(c, out->val, ow, M * 8, out->mem));
  return host_wait(c);
}

gs_status gs_match_import(gs_ctx* c, gs_match* t, const gs_edge_batch* rows) {
  GS_TRY(check_state(c, t));
  if (!rows || (rows->n && (!rows->src || !rows->dst || !rows->val)))
    return set_error(c, GS_EINVAL, "gs_match_import: null rows");
  if (rows->val_dtype != GS_I64) return set_error(c, GS_EINVAL, "gs_match_import: the values are I64");
  if (rows->mem != GS_MEM_HOST && rows->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "gs_match_import: bad mem");
  if (t->matched || t->records) return set_error(c, GS_EINVAL, "gs_match_import: the state is not empty");
  if (rows->n >= (1ull << 32)) return set_error(c, GS_EINVAL, "gs_match_import: %llu rows", (unsigned long long)rows->n);
  GS_TRY(begin_call(c));
  const uint64_t n = rows->n;
  if (n == 0) return GS_OK;
  GS_TRY(ensure_slots(c, n));
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, rows, &src, &dst, &val, true));
  GS_TRY(reserve(c, t, t->vertices + 2 * n));
  GS_TRY(reserve_epochs(c, t, 1));
  GS_TRY(insert_batch(c, t, src, dst, n, nullptr));
  const uint32_t *su = c->ts[0].as<uint32_t>(), *sv = c->ts[1].as<uint32_t>();
  const uint32_t epoch = ++t->epoch;
  const dim3 g(tab_grid_tab(n)), bl(256);
  hipLaunchKernelGGL(k_mt_import_claim, g, bl, 0, c->stream, table_of(t), n, su, sv, epoch);
  GS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mt_import_check, g, bl, 0, c->stream, table_of(t), n, su, sv, epoch);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, MT_META));
  if (c->host_small[8 + MT_ERR]) {
    GS_HIP(hipMemsetAsync(t->meta + MT_ERR, 0, 8, c->stream));   // no word of the refused rows stays behind
    return set_error(c, GS_EINVAL, "gs_match_import: two rows share an endpoint");
  }
  // ---- the matching changes from here on ----
  t->broken = true;
  hipLaunchKernelGGL(k_mt_import_write, g, bl, 0, c->stream, table_of(t), n, su, sv, (const int64_t*)val);
  GS_HIP(hipGetLastError());
  GS_TRY(tab_read_meta(c, t->meta, MT_META));
  t->matched = n;
  t->records = n;
  t->total_weight = c->host_small[8 + MT_DW];
  t->broken = false;
  return GS_OK;
}

}  // extern "C"

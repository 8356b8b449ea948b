// gs_trisample.hip — the sampling triangle estimators (example/BroadcastTriangleCount.java:62-135,
// example/IncidenceSamplingTriangleCount.java:125-203): S independent samplers of the Buriol et al. estimator
// whose state stays in HBM across batches.
//
// The reference tests every edge against every sampler, O(S * E).  Here a sampler's life inside a batch is cut
// into EPOCHS, the stretches between two of its replacements; an epoch wants two vertex pairs, {src, third}
// and {trg, third}, and all a batch has to tell it is the first position at which each pair arrives.  So one
// pass over the batch probes a table of the wanted pairs, and everything else is work on epochs and events.
//
//   rows[S][8]     the state: one row per sampler (gelly_hip.h, GS_TRISAMPLE_ROW_WORDS); nothing else is
//                  resident.  Counters (edges seen, beta sum, last emitted sum) live on the host side.
//
// One batch of n edges at the stream positions seen + 1 .. seen + n (all launches in the ctx stream's order).
// Everything up to the commit writes scratch of the ctx only, so any failure before it leaves the state as it was:
//   k_ts_count     lane per sampler: walk the replacement chain through (seen, seen + n], 1 + replacements epochs
//   xscan          epoch offsets per sampler
//   k_ts_fill      lane per sampler: the same walk, now writing each epoch's (sampler, open interval, end),
//                  (src, trg, third) -- endpoints read from the batch at the replacement position -- and its two
//                  first-match words (the carried epoch's found flags count as position 0); the sampler's new row
//   k_ts_insert    lane per wanted pair (epoch, which) of an open epoch: into a linear-probing table of 32-bit
//                  slots keyed by the normalised pair (min, max).  A slot holds the head of a chain of all wants
//                  of one pair (push-front by compare-and-swap); the pair itself is read from the epoch arrays,
//                  so equality is decided on the full ids.  Also sets the pair's bit in a 2^19-bit filter.
//   k_ts_stream    THE HOT KERNEL: one pass over src / dst, 16 B per edge.  A block first copies the filter
//                  into 64 KiB of LDS (two blocks per CU), then reads tiles of GS_TRISAMPLE_TILE edges with
//                  16-byte loads; an edge whose bit is clear is done after one LDS read.  The others probe the
//                  table and, on an equal pair, walk the chain: atomicMin of the edge's position into the
//                  first-match word of every want whose epoch is open at that position.  No lane waits on another.
//   k_ts_events    lane per epoch: find = max of the two first matches; a find is a +1 event at its position, the
//                  end of an epoch that had beta = 1 a -1 event at the replacement position; a sampler's last
//                  epoch writes the flags of its new row
//   sort           events by (position, sampler) -- one 63-bit key [position:31 | sampler:31 | is_plus:1]
//   k_ts_decode, xscan, k_ts_cand, xscan, k_ts_cfill, k_ts_eflag, xscan, k_ts_out
//                  running beta sum after every event; the candidates (BROADCAST: the last event of every
//                  position, INCIDENCE: every +1 event) with their sums; a candidate is a record iff its sum
//                  differs from the previous candidate's (the carried last emitted sum for the first)
//   commit         the new rows over the state's (one device copy), the host counters
#include <vector>

#include "gs_ops.hpp"

namespace gs {

constexpr int TS_ROW = GS_TRISAMPLE_ROW_WORDS;
enum { TSR_SRC, TSR_TRG, TSR_THIRD, TSR_FLAGS, TSR_J, TSR_LAST, TSR_NEXT, TSR_RSV };
constexpr uint64_t TS_NEVER = 1ull << 31;      // a replacement position no stream reaches
constexpr uint64_t TS_MAX_EDGES = TS_NEVER - 1;
constexpr uint32_t TS_INF = 0xffffffffu;       // first-match word: not seen
constexpr uint32_t TS_EMPTY = 0xffffffffu;     // table slot / end of a chain
constexpr int TS_FILTER_BITS = 19;             // 2^19 bits = 64 KiB of LDS per block, two blocks per CU
constexpr uint32_t TS_FILTER_WORDS = 1u << (TS_FILTER_BITS - 5);
constexpr int TS_TILE = GS_TRISAMPLE_TILE;     // 256 lanes x 4 loads x 2 edges
enum { TSM_ERR = 0, TSM_NEV, TSM_NOUT, TSM_NCAND, TSM_LAST, TSM_TOTAL, TSM_WORDS = 8 };   // u64 words of meta

// splitmix64(seed, i) of gs_gen.hip:11
__host__ __device__ __forceinline__ uint64_t ts_mix(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// r(seed, sampler, j, a): draw a of the sampler's replacement j
__host__ __device__ __forceinline__ uint64_t ts_draw(uint64_t seed, uint64_t sampler, uint64_t j, uint64_t a) {
  return ts_mix(ts_mix(ts_mix(seed, sampler), j), a);
}
// the position of the replacement after the one at K (1 <= K < 2^31), from draw 0 of that one
__host__ __device__ __forceinline__ uint64_t ts_next(uint64_t K, uint64_t r) {
  const uint64_t k = (K << 32) / ((r >> 32) + 1) + 1;
  return k > TS_MAX_EDGES ? TS_NEVER : k;
}

struct TsBatch {
  const int64_t* src;
  const int64_t* dst;
  uint64_t seen, end;   // positions (seen, end] = the batch
};

// the epochs of a batch (SoA over E epochs; a want w = 2 * epoch + which)
struct TsEpochs {
  uint4* info;      // x sampler, y / z open interval [lo, hi) of match positions, w = end position (0: still
                    // running at the batch's end) | beta carried in << 31
  int64_t* ids;     // [3E] src, trg, third
  uint32_t* fm;     // [2E] first match per want
  uint32_t* next;   // [2E] chain of the wants of one pair
};

struct TsTable {
  uint32_t* slots;
  uint32_t mask;
  uint32_t* filter;   // [TS_FILTER_WORDS] global copy of the presence filter
};

__device__ __forceinline__ unsigned long long ts_pair_hash(int64_t a, int64_t b) {
  return ct_hash(ct_hash((unsigned long long)a) ^ ((unsigned long long)b * 0x9e3779b97f4a7c15ull));
}
__device__ __forceinline__ void ts_want_pair(const int64_t* __restrict__ ids, uint32_t w, int64_t* a, int64_t* b) {
  const int64_t x = ids[3ull * (w >> 1) + (w & 1)], t = ids[3ull * (w >> 1) + 2];
  *a = x < t ? x : t;
  *b = x < t ? t : x;
}

__global__ __launch_bounds__(256) void k_ts_count(const int64_t* __restrict__ rows, uint64_t S, uint64_t first,
                                                  uint64_t seed, uint64_t end, uint64_t* __restrict__ cnt) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= S; s += (uint64_t)gridDim.x * 256) {
    if (s == S) {
      cnt[s] = 0;
      continue;
    }
    uint64_t next = (uint64_t)rows[s * TS_ROW + TSR_NEXT], j = (uint64_t)rows[s * TS_ROW + TSR_J], e = 1;
    while (next <= end) {
      next = ts_next(next, ts_draw(seed, first + s, j, 0));
      ++j;
      ++e;
    }
    cnt[s] = e;
  }
}

__global__ __launch_bounds__(256) void k_ts_fill(const int64_t* __restrict__ rows, uint64_t S, uint64_t first,
                                                 uint64_t seed, uint64_t V, TsBatch b,
                                                 const uint64_t* __restrict__ off, TsEpochs ep,
                                                 int64_t* __restrict__ newrows) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < S; s += (uint64_t)gridDim.x * 256) {
    const int64_t* row = rows + s * TS_ROW;
    uint64_t e = off[s];
    int64_t src = row[TSR_SRC], trg = row[TSR_TRG], third = row[TSR_THIRD];
    const uint64_t flags = (uint64_t)row[TSR_FLAGS];
    uint64_t j = (uint64_t)row[TSR_J], last = (uint64_t)row[TSR_LAST], next = (uint64_t)row[TSR_NEXT];
    // the epoch carried in (empty before the first edge: next = seen + 1 there)
    uint32_t fm0 = (flags & 1) ? 0u : TS_INF, fm1 = (flags & 2) ? 0u : TS_INF, beta = (uint32_t)(flags >> 2) & 1u;
    uint64_t lo = b.seen + 1;
    for (;;) {
      const uint64_t hi = next <= b.end ? next : b.end + 1;
      ep.info[e] = make_uint4((uint32_t)s, (uint32_t)lo, (uint32_t)hi, (next <= b.end ? (uint32_t)next : 0u) | (beta << 31));
      ep.ids[3 * e] = src;
      ep.ids[3 * e + 1] = trg;
      ep.ids[3 * e + 2] = third;
      ep.fm[2 * e] = fm0;
      ep.fm[2 * e + 1] = fm1;
      if (next > b.end) break;
      // replacement j at position K = next
      const uint64_t K = next;
      next = ts_next(K, ts_draw(seed, first + s, j, 0));
      src = b.src[K - b.seen - 1];
      trg = b.dst[K - b.seen - 1];
      for (uint64_t a = 1;; ++a) {
        third = (int64_t)__umul64hi(ts_draw(seed, first + s, j, a), V);
        if (third != src && third != trg) break;
      }
      ++j;
      last = K;
      lo = K + 1;
      fm0 = fm1 = TS_INF;
      beta = 0;
      ++e;
    }
    int64_t* nr = newrows + s * TS_ROW;
    nr[TSR_SRC] = src;
    nr[TSR_TRG] = trg;
    nr[TSR_THIRD] = third;
    nr[TSR_FLAGS] = 0;   // k_ts_events
    nr[TSR_J] = (int64_t)j;
    nr[TSR_LAST] = (int64_t)last;
    nr[TSR_NEXT] = (int64_t)next;
    nr[TSR_RSV] = 0;
  }
}

__global__ __launch_bounds__(256) void k_ts_clear(uint32_t* __restrict__ p, uint64_t n, uint32_t v) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) p[i] = v;
}

// lane per want: open epochs' still-missing pairs into the table.  The pairs were written by k_ts_fill, so a
// slot's want index is all another lane needs to compare keys; next[] is read by k_ts_stream only.
__global__ __launch_bounds__(256) void k_ts_insert(TsEpochs ep, uint64_t W, TsTable t, unsigned long long* __restrict__ meta) {
  for (uint64_t w64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; w64 < W; w64 += (uint64_t)gridDim.x * 256) {
    const uint32_t w = (uint32_t)w64;
    const uint4 in = ep.info[w >> 1];
    if ((in.w >> 31) || in.y >= in.z || ep.fm[w] != TS_INF) continue;
    int64_t a, b;
    ts_want_pair(ep.ids, w, &a, &b);
    const unsigned long long h = ts_pair_hash(a, b);
    const uint32_t bit = (uint32_t)(h >> (64 - TS_FILTER_BITS));
    atomicOr(&t.filter[bit >> 5], 1u << (bit & 31));
    uint32_t slot = (uint32_t)h & t.mask;
    bool done = false;
    for (uint32_t probes = 0; probes <= t.mask && !done; ++probes, slot = (slot + 1) & t.mask) {
      uint32_t cur = __hip_atomic_load(&t.slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == TS_EMPTY) {
        ep.next[w] = TS_EMPTY;
        cur = atomicCAS(&t.slots[slot], TS_EMPTY, w);
        if (cur == TS_EMPTY) {
          done = true;
          break;
        }
      }
      int64_t ca, cb;
      ts_want_pair(ep.ids, cur, &ca, &cb);
      if (ca != a || cb != b) continue;
      // the slot is this pair's for the rest of the batch: push in front of whichever want heads it now
      for (;;) {
        ep.next[w] = cur;
        const uint32_t prev = atomicCAS(&t.slots[slot], cur, w);
        if (prev == cur) break;
        cur = prev;
      }
      done = true;
    }
    if (!done) atomicOr(&meta[TSM_ERR], 1ull);
  }
}

__device__ __forceinline__ void ts_edge(int64_t s, int64_t d, uint32_t pos, const uint32_t* __restrict__ s_filter,
                                        bool use_filter, const TsEpochs& ep, const TsTable& t) {
  const int64_t a = s < d ? s : d, b = s < d ? d : s;
  const unsigned long long h = ts_pair_hash(a, b);
  if (use_filter) {
    const uint32_t bit = (uint32_t)(h >> (64 - TS_FILTER_BITS));
    if (!((s_filter[bit >> 5] >> (bit & 31)) & 1u)) return;
  }
  uint32_t slot = (uint32_t)h & t.mask;
  for (uint32_t probes = 0; probes <= t.mask; ++probes, slot = (slot + 1) & t.mask) {
    const uint32_t head = t.slots[slot];
    if (head == TS_EMPTY) return;
    int64_t ca, cb;
    ts_want_pair(ep.ids, head, &ca, &cb);
    if (ca != a || cb != b) continue;
    for (uint32_t w = head; w != TS_EMPTY; w = ep.next[w]) {
      const uint4 in = ep.info[w >> 1];
      if (pos >= in.y && pos < in.z) atomicMin(&ep.fm[w], pos);
    }
    return;
  }
}

// the streaming pass.  VEC: both columns are 16-byte aligned, a lane reads two edges per load
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_ts_stream(TsBatch b, uint64_t n, TsEpochs ep, TsTable t, int use_filter) {
  __shared__ uint32_t s_filter[TS_FILTER_WORDS];
  if (use_filter) {
    const uint4* g = (const uint4*)t.filter;
    for (uint32_t i = threadIdx.x; i < TS_FILTER_WORDS / 4; i += 256) ((uint4*)s_filter)[i] = g[i];
    __syncthreads();
  }
  const uint64_t tiles = (n + TS_TILE - 1) / TS_TILE;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t base = tile * TS_TILE + 2ull * threadIdx.x;
    int64_t s[4][2], d[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t i = base + (uint64_t)k * 512;
      if (VEC && i + 1 < n) {
        const longlong2 vs = *(const longlong2*)(b.src + i), vd = *(const longlong2*)(b.dst + i);
        s[k][0] = vs.x;
        s[k][1] = vs.y;
        d[k][0] = vd.x;
        d[k][1] = vd.y;
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          s[k][q] = i + q < n ? b.src[i + q] : 0;
          d[k][q] = i + q < n ? b.dst[i + q] : 0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint64_t i = base + (uint64_t)k * 512 + q;
        if (i < n) ts_edge(s[k][q], d[k][q], (uint32_t)(b.seen + 1 + i), s_filter, use_filter != 0, ep, t);
      }
    }
  }
}

// lane per epoch: its events, and the flags of the sampler's new row from its last epoch
__global__ __launch_bounds__(256) void k_ts_events(TsEpochs ep, uint64_t E, unsigned long long* __restrict__ evk,
                                                   unsigned long long* __restrict__ meta, int64_t* __restrict__ newrows) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (uint64_t)gridDim.x * 256) {
    const uint4 in = ep.info[e];
    const uint32_t f0 = ep.fm[2 * e], f1 = ep.fm[2 * e + 1];
    const bool beta_in = (in.w >> 31) != 0;
    const unsigned long long end = in.w & 0x7fffffffu, samp = in.x;
    const uint32_t find = f0 > f1 ? f0 : f1;
    const bool found = !beta_in && find != TS_INF;
    if (found) evk[atomicAdd(&meta[TSM_NEV], 1ull)] = ((unsigned long long)find << 33) | (samp << 1) | 1ull;
    if (end && (beta_in || found)) evk[atomicAdd(&meta[TSM_NEV], 1ull)] = (end << 33) | (samp << 1);
    if (!end)
      newrows[samp * TS_ROW + TSR_FLAGS] = (f0 != TS_INF ? 1 : 0) | (f1 != TS_INF ? 2 : 0) | ((beta_in || found) ? 4 : 0);
  }
}

// sorted keys -> full event words and their deltas (+1 / -1 as wrapping u64)
template <typename K>
__global__ __launch_bounds__(256) void k_ts_decode(const K* __restrict__ keys, uint64_t key_xor, uint64_t n,
                                                   uint64_t* __restrict__ ev, uint64_t* __restrict__ delta) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t k = key_xor ^ (uint64_t)keys[i];
    ev[i] = k;
    delta[i] = (k & 1) ? 1ull : ~0ull;
  }
}

__global__ __launch_bounds__(256) void k_ts_cand(const uint64_t* __restrict__ ev, uint64_t n, int incidence,
                                                 uint64_t* __restrict__ cand) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    cand[i] = incidence ? (ev[i] & 1) : (uint64_t)(i + 1 == n || (ev[i + 1] >> 33) != (ev[i] >> 33));
}

__global__ __launch_bounds__(256) void k_ts_cfill(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ delta,
                                                  const uint64_t* __restrict__ excl, const uint64_t* __restrict__ cand,
                                                  const uint64_t* __restrict__ crank, uint64_t n, uint64_t beta0,
                                                  uint64_t* __restrict__ cval, uint64_t* __restrict__ cpos) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (!cand[i]) continue;
    const uint64_t k = crank[i];
    cval[k] = beta0 + excl[i] + delta[i];
    cpos[k] = ev[i] >> 33;
  }
}

// candidate k is a record iff its sum differs from the one before it (entries past the candidates: 0)
__global__ __launch_bounds__(256) void k_ts_eflag(const uint64_t* __restrict__ cval, const uint64_t* __restrict__ crank,
                                                  uint64_t n, uint64_t last_emitted, uint64_t* __restrict__ eflag) {
  const uint64_t nc = crank[n];
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256)
    eflag[k] = k < nc && cval[k] != (k ? cval[k - 1] : last_emitted);
}

__global__ void k_ts_totals(const uint64_t* __restrict__ excl, const uint64_t* __restrict__ crank,
                            const uint64_t* __restrict__ erank, const uint64_t* __restrict__ cval, uint64_t n,
                            unsigned long long* __restrict__ meta) {
  const uint64_t nc = crank[n];
  meta[TSM_NOUT] = erank[n];
  meta[TSM_NCAND] = nc;
  meta[TSM_LAST] = nc ? cval[nc - 1] : 0;
  meta[TSM_TOTAL] = excl[n];
}

__global__ __launch_bounds__(256) void k_ts_out(const uint64_t* __restrict__ cval, const uint64_t* __restrict__ cpos,
                                                const uint64_t* __restrict__ eflag, const uint64_t* __restrict__ erank,
                                                uint64_t n, int64_t* __restrict__ keys, int64_t* __restrict__ vals) {
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (uint64_t)gridDim.x * 256) {
    if (!eflag[k]) continue;
    const uint64_t o = erank[k];
    if (keys) keys[o] = (int64_t)cpos[k];
    if (vals) vals[o] = (int64_t)cval[k];
  }
}

}  // namespace gs

using namespace gs;

struct gs_trisample {
  int device = 0;
  int mode = GS_TRISAMPLE_BROADCAST;
  uint64_t samples = 0, first = 0, vertices = 0, seed = 0;
  int64_t* rows = nullptr;               // device [samples][TS_ROW]
  unsigned long long* meta = nullptr;    // device u64[TSM_WORDS]
  uint64_t seen = 0;
  int64_t beta_sum = 0, last_emitted = 0;
  bool broken = false;                   // a commit failed midway
};

namespace {

enum { TSB_CNT, TSB_OFF, TSB_ROWS, TSB_INFO, TSB_IDS, TSB_FM, TSB_NEXT, TSB_SLOTS, TSB_FILTER, TSB_EVK, TSB_WORK };
static_assert(TSB_WORK < 12, "gs_ctx::ts");

unsigned ts_grid(uint64_t n) { return grid_for(n, 256, 16384); }

gs_status check_state(gs_ctx* c, const gs_trisample* t) {
  if (!c) return GS_EINVAL;
  if (!t) return set_error(c, GS_EINVAL, "null triangle sampler state");
  if (t->device != c->device)
    return set_error(c, GS_EINVAL, "triangle sampler state lives on device %d, the ctx on device %d", t->device, c->device);
  if (t->broken) return set_error(c, GS_EDEVICE, "triangle sampler state: an earlier batch failed during its commit");
  return GS_OK;
}

gs_status read_meta(gs_ctx* c, const gs_trisample* t) {
  GS_HIP(hipMemcpyAsync(c->host_small + 8, t->meta, TSM_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
  return host_wait(c);
}

void fresh_rows(std::vector<int64_t>& rows, uint64_t S) {
  rows.assign(S * TS_ROW, 0);
  for (uint64_t s = 0; s < S; ++s) {
    rows[s * TS_ROW + TSR_THIRD] = -1;
    rows[s * TS_ROW + TSR_NEXT] = 1;
  }
}

// a row some run of `seen` edges can have left (the header's counters are checked against the rows' betas)
bool row_ok(const int64_t* r, uint64_t seen) {
  const uint64_t fl = (uint64_t)r[TSR_FLAGS], j = (uint64_t)r[TSR_J], last = (uint64_t)r[TSR_LAST], next = (uint64_t)r[TSR_NEXT];
  if (fl > 7 || ((fl & 3) == 3) != ((fl & 4) != 0) || r[TSR_RSV] != 0) return false;
  if (seen == 0) return fl == 0 && j == 0 && last == 0 && next == 1;
  return j >= 1 && last >= 1 && last <= seen && next > seen && next <= TS_NEVER;
}

}  // namespace

extern "C" {

gs_status gs_trisample_create(gs_ctx* c, int32_t mode, uint64_t samples, uint64_t first_sampler, uint64_t vertex_count,
                              uint64_t seed, gs_trisample** out) {
  if (!c) return GS_EINVAL;
  if (!out) return set_error(c, GS_EINVAL, "gs_trisample_create: null argument");
  *out = nullptr;
  if (mode != GS_TRISAMPLE_BROADCAST && mode != GS_TRISAMPLE_INCIDENCE)
    return set_error(c, GS_EINVAL, "gs_trisample_create: bad mode %d", mode);
  if (samples == 0 || samples > TS_MAX_EDGES)
    return set_error(c, GS_EINVAL, "gs_trisample_create: %llu samples (1 .. 2^31 - 1)", (unsigned long long)samples);
  if (vertex_count < 3 || vertex_count > (1ull << 63) - 1)
    return set_error(c, GS_EINVAL, "gs_trisample_create: vertex count %llu (a third vertex needs 3)", (unsigned long long)vertex_count);
  if (first_sampler + samples < first_sampler) return set_error(c, GS_EINVAL, "gs_trisample_create: sampler ids overflow");
  GS_TRY(begin_call(c));
  gs_trisample* t = new (std::nothrow) gs_trisample();
  if (!t) return set_error(c, GS_ENOMEM, "gs_trisample_create");
  t->device = c->device;
  t->mode = mode;
  t->samples = samples;
  t->first = first_sampler;
  t->vertices = vertex_count;
  t->seed = seed;
  gs_status st = GS_OK;
  if (hipMalloc((void**)&t->rows, samples * TS_ROW * 8) != hipSuccess || hipMalloc((void**)&t->meta, TSM_WORDS * 8) != hipSuccess) {
    (void)hipGetLastError();
    st = set_error(c, GS_ENOMEM, "gs_trisample_create: %llu sampler rows do not fit", (unsigned long long)samples);
  }
  std::vector<int64_t> rows;
  if (st == GS_OK) {
    fresh_rows(rows, samples);
    st = hip_check(c, hipMemcpyAsync(t->rows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, c->stream), "sampler rows");
  }
  if (st == GS_OK) st = hip_check(c, hipMemsetAsync(t->meta, 0, TSM_WORDS * 8, c->stream), "hipMemsetAsync");
  if (st == GS_OK) st = host_wait(c);
  if (st != GS_OK) {
    gs_trisample_destroy(t);
    return st;
  }
  *out = t;
  return GS_OK;
}

void gs_trisample_destroy(gs_trisample* t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->rows) hipFree(t->rows);
  if (t->meta) hipFree(t->meta);
  delete t;
}

gs_status gs_trisample_size(const gs_trisample* t, uint64_t* edges_seen, int64_t* beta_sum) {
  if (!t) return GS_EINVAL;
  if (edges_seen) *edges_seen = t->seen;
  if (beta_sum) *beta_sum = t->beta_sum;
  return GS_OK;
}

gs_status gs_trisample_edges(gs_ctx* c, gs_trisample* t, const gs_edge_batch* b, gs_vertex_out* out) {
  GS_TRY(check_state(c, t));
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (!out || !out->n_out) return set_error(c, GS_EINVAL, "bad gs_vertex_out");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_vertex_out.mem %d", out->mem);
  if (b->mem != GS_MEM_HOST && b->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_edge_batch.mem %d", b->mem);
  const uint64_t n = b->n, S = t->samples;
  *out->n_out = 0;
  if (n > TS_MAX_EDGES - t->seen)
    return set_error(c, GS_EINVAL, "gs_trisample_edges: %llu + %llu edges, the stream's edge count is an int",
                     (unsigned long long)t->seen, (unsigned long long)n);
  GS_TRY(begin_call(c));
  if (n == 0) return GS_OK;
  const bool any = out->keys || out->vals;
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, false));
  const TsBatch tb{src, dst, t->seen, t->seen + n};

  // ---- epochs ----
  GS_TRY(ensure(c, c->ts[TSB_CNT], (S + 1) * 8));
  GS_TRY(ensure(c, c->ts[TSB_OFF], (S + 2) * 8));
  GS_TRY(ensure(c, c->ts[TSB_ROWS], S * TS_ROW * 8));
  uint64_t* cnt = c->ts[TSB_CNT].as<uint64_t>();
  uint64_t* off = c->ts[TSB_OFF].as<uint64_t>();
  int64_t* newrows = c->ts[TSB_ROWS].as<int64_t>();
  hipLaunchKernelGGL(k_ts_count, dim3(ts_grid(S + 1)), dim3(256), 0, c->stream, t->rows, S, t->first, t->seed, tb.end, cnt);
  GS_HIP(hipGetLastError());
  GS_TRY(xscan(c, cnt, S + 1, off));
  GS_HIP(hipMemcpyAsync(c->host_small + 8, off + S, 8, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(host_wait(c));
  const uint64_t E = c->host_small[8], W = 2 * E;
  if (E < S || W >= TS_EMPTY)
    return set_error(c, E < S ? GS_EDEVICE : GS_ENOMEM, "gs_trisample_edges: %llu epochs in one batch", (unsigned long long)E);
  uint64_t cap = 64;
  while (cap < 2 * W) cap *= 2;
  GS_TRY(ensure(c, c->ts[TSB_INFO], E * 16));
  GS_TRY(ensure(c, c->ts[TSB_IDS], 3 * E * 8));
  GS_TRY(ensure(c, c->ts[TSB_FM], W * 4));
  GS_TRY(ensure(c, c->ts[TSB_NEXT], W * 4));
  GS_TRY(ensure(c, c->ts[TSB_SLOTS], cap * 4));
  GS_TRY(ensure(c, c->ts[TSB_FILTER], TS_FILTER_WORDS * 4));
  GS_TRY(ensure(c, c->ts[TSB_EVK], W * 8));
  const TsEpochs ep{c->ts[TSB_INFO].as<uint4>(), c->ts[TSB_IDS].as<int64_t>(), c->ts[TSB_FM].as<uint32_t>(),
                    c->ts[TSB_NEXT].as<uint32_t>()};
  const TsTable tab{c->ts[TSB_SLOTS].as<uint32_t>(), (uint32_t)(cap - 1), c->ts[TSB_FILTER].as<uint32_t>()};
  unsigned long long* evk = c->ts[TSB_EVK].as<unsigned long long>();
  hipLaunchKernelGGL(k_ts_fill, dim3(ts_grid(S)), dim3(256), 0, c->stream, t->rows, S, t->first, t->seed, t->vertices, tb,
                     (const uint64_t*)off, ep, newrows);
  GS_HIP(hipGetLastError());

  // ---- wanted table ----
  GS_HIP(hipMemsetAsync(tab.slots, 0xff, cap * 4, c->stream));
  GS_HIP(hipMemsetAsync(tab.filter, 0, TS_FILTER_WORDS * 4, c->stream));
  GS_HIP(hipMemsetAsync(t->meta, 0, TSM_WORDS * 8, c->stream));
  hipLaunchKernelGGL(k_ts_insert, dim3(ts_grid(W)), dim3(256), 0, c->stream, ep, W, tab, t->meta);
  GS_HIP(hipGetLastError());

  // ---- the streaming pass ----
  // past one want per four filter bits the filter passes most edges anyway: skip its copy and its read
  const int use_filter = W <= (1ull << (TS_FILTER_BITS - 2));
  const uint64_t tiles = (n + TS_TILE - 1) / TS_TILE;
  if (!c->n_cu) {
    int cu = 0;
    GS_HIP(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device));
    c->n_cu = std::max(1, cu);
  }
  const unsigned sgrid = grid_for(tiles, 1, 2 * c->n_cu);
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0)
    hipLaunchKernelGGL(k_ts_stream<true>, dim3(sgrid), dim3(256), 0, c->stream, tb, n, ep, tab, use_filter);
  else
    hipLaunchKernelGGL(k_ts_stream<false>, dim3(sgrid), dim3(256), 0, c->stream, tb, n, ep, tab, use_filter);
  GS_HIP(hipGetLastError());

  // ---- events ----
  hipLaunchKernelGGL(k_ts_events, dim3(ts_grid(E)), dim3(256), 0, c->stream, ep, E, evk, t->meta, newrows);
  GS_HIP(hipGetLastError());
  GS_TRY(read_meta(c, t));
  if (c->host_small[8 + TSM_ERR]) return set_error(c, GS_EDEVICE, "triangle sampler: the wanted table filled up");
  const uint64_t nev = c->host_small[8 + TSM_NEV];
  if (nev > W) return set_error(c, GS_EDEVICE, "triangle sampler: %llu events of %llu epochs", (unsigned long long)nev, (unsigned long long)E);

  // ---- emit ----
  uint64_t nout = 0, ncand = 0;
  int64_t total = 0, last_val = 0;
  uint64_t *cval = nullptr, *cpos = nullptr, *eflag = nullptr, *erank = nullptr;
  if (nev) {
    Sorted s;
    GS_TRY(sort_buffer(c, (const uint64_t*)evk, nullptr, nev, &s, 64, 4));
    const uint64_t L = nev + 2;   // words per work column
    GS_TRY(ensure(c, c->ts[TSB_WORK], 9 * L * 8));
    uint64_t* w0 = c->ts[TSB_WORK].as<uint64_t>();
    uint64_t *ev = w0, *delta = w0 + L, *excl = w0 + 2 * L, *cand = w0 + 3 * L, *crank = w0 + 4 * L;
    cval = w0 + 5 * L;
    cpos = w0 + 6 * L;
    eflag = w0 + 7 * L;
    erank = w0 + 8 * L;
    const dim3 g(ts_grid(nev)), blk(256);
    if (s.wide)
      hipLaunchKernelGGL(k_ts_decode<uint64_t>, g, blk, 0, c->stream, (const uint64_t*)s.keys, s.key_xor, nev, ev, delta);
    else
      hipLaunchKernelGGL(k_ts_decode<uint32_t>, g, blk, 0, c->stream, (const uint32_t*)s.keys, s.key_xor, nev, ev, delta);
    GS_HIP(hipGetLastError());
    GS_TRY(xscan(c, delta, nev, excl));
    hipLaunchKernelGGL(k_ts_cand, g, blk, 0, c->stream, (const uint64_t*)ev, nev, t->mode == GS_TRISAMPLE_INCIDENCE ? 1 : 0, cand);
    GS_HIP(hipGetLastError());
    GS_TRY(xscan(c, cand, nev, crank));
    hipLaunchKernelGGL(k_ts_cfill, g, blk, 0, c->stream, (const uint64_t*)ev, (const uint64_t*)delta, (const uint64_t*)excl,
                       (const uint64_t*)cand, (const uint64_t*)crank, nev, (uint64_t)t->beta_sum, cval, cpos);
    hipLaunchKernelGGL(k_ts_eflag, g, blk, 0, c->stream, (const uint64_t*)cval, (const uint64_t*)crank, nev,
                       (uint64_t)t->last_emitted, eflag);
    GS_HIP(hipGetLastError());
    GS_TRY(xscan(c, eflag, nev, erank));
    hipLaunchKernelGGL(k_ts_totals, dim3(1), dim3(1), 0, c->stream, (const uint64_t*)excl, (const uint64_t*)crank,
                       (const uint64_t*)erank, (const uint64_t*)cval, nev, t->meta);
    GS_HIP(hipGetLastError());
    GS_TRY(read_meta(c, t));
    nout = c->host_small[8 + TSM_NOUT];
    ncand = c->host_small[8 + TSM_NCAND];
    last_val = (int64_t)c->host_small[8 + TSM_LAST];
    total = (int64_t)c->host_small[8 + TSM_TOTAL];
    if (nout > nev || ncand > nev) return set_error(c, GS_EDEVICE, "triangle sampler: %llu records of %llu events",
                                                    (unsigned long long)nout, (unsigned long long)nev);
  }
  *out->n_out = nout;
  if (any && out->capacity < nout) return set_error(c, GS_ECAPACITY, "output needs room for %llu records", (unsigned long long)nout);
  const bool direct = out->mem == GS_MEM_DEVICE;
  int64_t *ok = out->keys, *ov = (int64_t*)out->vals;
  if (any && nout) {
    if (!direct) {
      if (out->keys) {
        GS_TRY(ensure(c, c->out_keys, nout * 8));
        ok = c->out_keys.as<int64_t>();
      }
      if (out->vals) {
        GS_TRY(ensure(c, c->out_a, nout * 8));
        ov = c->out_a.as<int64_t>();
      }
    }
    hipLaunchKernelGGL(k_ts_out, dim3(ts_grid(nev)), dim3(256), 0, c->stream, (const uint64_t*)cval, (const uint64_t*)cpos,
                       (const uint64_t*)eflag, (const uint64_t*)erank, nev, ok, ov);
    GS_HIP(hipGetLastError());
  }
  // ---- commit: the state changes from here on ----
  t->broken = true;
  GS_HIP(hipMemcpyAsync(t->rows, newrows, S * TS_ROW * 8, hipMemcpyDeviceToDevice, c->stream));
  t->seen += n;
  t->beta_sum += total;
  if (ncand) t->last_emitted = last_val;
  t->broken = false;
  if (any && nout && !direct) {
    if (out->keys) GS_TRY(deliver(c, out->keys, ok, nout * 8, out->mem));
    if (out->vals) GS_TRY(deliver(c, out->vals, ov, nout * 8, out->mem));
    GS_TRY(host_wait(c));
  }
  return GS_OK;
}

gs_status gs_trisample_export(gs_ctx* c, const gs_trisample* t, gs_trisample_header* header, int64_t* rows,
                              uint64_t capacity_rows, int32_t mem, uint64_t* n_out) {
  GS_TRY(check_state(c, t));
  if (!header || !n_out) return set_error(c, GS_EINVAL, "gs_trisample_export: null argument");
  if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "gs_trisample_export: bad mem %d", mem);
  *n_out = t->samples;
  if (!rows || capacity_rows < t->samples)
    return set_error(c, GS_ECAPACITY, "output needs %llu rows", (unsigned long long)t->samples);
  GS_TRY(begin_call(c));
  *header = gs_trisample_header{t->seen, t->beta_sum, t->last_emitted, t->samples, t->first, t->vertices, t->seed, t->mode, 0};
  GS_TRY(deliver(c, rows, t->rows, t->samples * TS_ROW * 8, mem));
  return mem == GS_MEM_DEVICE ? GS_OK : host_wait(c);
}

gs_status gs_trisample_import(gs_ctx* c, gs_trisample* t, const gs_trisample_header* h, const int64_t* rows, uint64_t n_rows,
                              int32_t mem) {
  GS_TRY(check_state(c, t));
  if (!h || !rows) return set_error(c, GS_EINVAL, "gs_trisample_import: null argument");
  if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "gs_trisample_import: bad mem %d", mem);
  if (t->seen) return set_error(c, GS_EINVAL, "gs_trisample_import: the state is not fresh");
  if (h->mode != t->mode || h->samples != t->samples || h->first_sampler != t->first || h->vertex_count != t->vertices ||
      h->seed != t->seed || n_rows != t->samples)
    return set_error(c, GS_EINVAL, "gs_trisample_import: the checkpoint is of a state with other parameters");
  if (h->edges_seen > TS_MAX_EDGES) return set_error(c, GS_EINVAL, "gs_trisample_import: %llu edges", (unsigned long long)h->edges_seen);
  GS_TRY(begin_call(c));
  // S rows of 64 bytes: checked on the host, whichever memory they come from
  std::vector<int64_t> host(n_rows * TS_ROW);
  if (mem == GS_MEM_DEVICE) {
    GS_HIP(hipMemcpyAsync(host.data(), rows, host.size() * 8, hipMemcpyDeviceToHost, c->stream));
    GS_TRY(host_wait(c));
  } else {
    std::copy(rows, rows + host.size(), host.begin());
  }
  int64_t betas = 0;
  for (uint64_t s = 0; s < n_rows; ++s) {
    if (!row_ok(&host[s * TS_ROW], h->edges_seen))
      return set_error(c, GS_EINVAL, "gs_trisample_import: row %llu is not a sampler's row after %llu edges",
                       (unsigned long long)s, (unsigned long long)h->edges_seen);
    betas += (host[s * TS_ROW + TSR_FLAGS] >> 2) & 1;
  }
  if (betas != h->beta_sum || h->last_emitted < 0 || (uint64_t)h->last_emitted > n_rows ||
      (t->mode == GS_TRISAMPLE_BROADCAST && h->last_emitted != h->beta_sum))
    return set_error(c, GS_EINVAL, "gs_trisample_import: the header's sums do not fit the rows");
  // ---- the state changes from here on ----
  t->broken = true;
  GS_HIP(hipMemcpyAsync(t->rows, host.data(), host.size() * 8, hipMemcpyHostToDevice, c->stream));
  GS_TRY(host_wait(c));
  t->seen = h->edges_seen;
  t->beta_sum = h->beta_sum;
  t->last_emitted = h->last_emitted;
  t->broken = false;
  return GS_OK;
}

}  // extern "C"

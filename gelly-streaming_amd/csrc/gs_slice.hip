// gs_slice.hip — all tumbling windows of a batch in one call.
//
//   gs_slice_reduce          <- SimpleEdgeStream.slice(size).reduceOnEdges / foldNeighbors over many windows
//   gs_slice_fold_degree_max <- the same with the degree / max-neighbour fold
// Flink keys (vertex, window) state for all open windows at once (SimpleEdgeStream.java:159-167); here the window
// becomes the high part of the sort key:
//   k_sl_range    one read of the timestamp and key column(s): min / max timestamp and vertex (one read-back);
//   k_sl_keys     composite key ((ts / size - first window) << vbits | (vertex - min vertex)) and payload per
//                 record, direction-expanded;
//   sort_buffer   stable LSD sort of the composite keys (it histograms them itself: its one read-back);
//   launch_rbk    the reduce-by-key of every operator; the Out functors here unpack the key into the vertex and
//                 leave the row's window index in a scratch column;
//   k_sl_wcount / k_scan_chunks / k_sl_wemit   rows whose window index differs from the previous row's start a
//                 window: counted per tile, scanned, then written as window_start[] and row_begin[].
// Nothing of a call outlives it: the ctx keeps the buffers (sl[]) and no state.
#include "gs_ops.hpp"

using namespace gs;

namespace gs {
namespace {

constexpr uint64_t SIGN = 1ull << 63;   // int64 -> the unsigned word of the same order

// the geometry of one call's composite keys (by value to every kernel)
struct SlGeom {
  int64_t size;     // window length
  uint64_t q0;      // first window's number: min(ts) / size (truncated), as an unsigned word
  uint64_t v0;      // min vertex, as an unsigned word
  uint64_t vmask;   // low vbits
  uint32_t vbits;   // width of the vertex span (64: the window part is empty)
  __device__ __forceinline__ uint64_t key(int64_t vertex, int64_t t) const {
    const uint64_t w = (uint64_t)(t / size) - q0;
    return (vbits >= 64 ? 0ull : w << vbits) | ((uint64_t)vertex - v0);
  }
  __device__ __forceinline__ int64_t vertex(uint64_t k) const { return (int64_t)(v0 + (k & vmask)); }
  __device__ __forceinline__ uint64_t window(uint64_t k) const { return vbits >= 64 ? 0ull : k >> vbits; }
  __device__ __forceinline__ int64_t start(uint64_t w) const { return (int64_t)(q0 + w) * size; }
};

// ---- k_sl_range -----------------------------------------------------------------------------------------------
// out[0] = min ts, out[1] = min vertex (atomicMin), out[2] = max ts, out[3] = max vertex (atomicMax), all as
// sign-flipped words; the window start is monotone in ts, so the extreme windows are those of the extreme ts
template <int DIR, bool VEC>
__global__ __launch_bounds__(256) void k_sl_range(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                  const int64_t* __restrict__ ts, uint64_t n,
                                                  unsigned long long* __restrict__ out) {
  __shared__ int64_t s_r[4][256 / WAVE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t tmin = INT64_MAX, tmax = INT64_MIN, vmin = INT64_MAX, vmax = INT64_MIN;
  auto add = [&](int64_t s, int64_t d, int64_t t) {
    tmin = t < tmin ? t : tmin;
    tmax = t > tmax ? t : tmax;
    if (DIR != DIR_IN) {
      vmin = s < vmin ? s : vmin;
      vmax = s > vmax ? s : vmax;
    }
    if (DIR != DIR_OUT) {
      vmin = d < vmin ? d : vmin;
      vmax = d > vmax ? d : vmax;
    }
  };
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  if constexpr (VEC) {
    const uint64_t npair = n >> 1;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + tid; q < npair; q += stride) {
      u64x2 s{0, 0}, d{0, 0};
      if (DIR != DIR_IN) s = ld16<false>(src + 2 * q);
      if (DIR != DIR_OUT) d = ld16<false>(dst + 2 * q);
      const u64x2 t = ld16<false>(ts + 2 * q);
      add((int64_t)s.x, (int64_t)d.x, (int64_t)t.x);
      add((int64_t)s.y, (int64_t)d.y, (int64_t)t.y);
    }
    if ((n & 1) && blockIdx.x == 0 && tid == 0) add(src[n - 1], dst[n - 1], ts[n - 1]);
  } else {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + tid; i < n; i += stride) add(src[i], dst[i], ts[i]);
  }
  tmin = wave_min(tmin);
  vmin = wave_min(vmin);
  tmax = wave_max(tmax);
  vmax = wave_max(vmax);
  if (lane == 0) {
    s_r[0][w] = tmin;
    s_r[1][w] = vmin;
    s_r[2][w] = tmax;
    s_r[3][w] = vmax;
  }
  __syncthreads();
  if (tid < 4) {
    int64_t x = s_r[tid][0];
    for (int i = 1; i < 256 / WAVE; ++i) {
      const int64_t y = s_r[tid][i];
      x = tid < 2 ? (y < x ? y : x) : (y > x ? y : x);
    }
    // (a block that saw no record holds the identities: they change nothing)
    const unsigned long long u = (unsigned long long)x ^ SIGN;
    if (tid < 2) atomicMin(out + tid, u);
    else atomicMax(out + tid, u);
  }
}

// ---- k_sl_keys ------------------------------------------------------------------------------------------------
// record r of the batch: OUT (src[r], dst[r]); IN (dst[r], src[r]); ALL r = 2i -> (src[i], dst[i]), 2i + 1 ->
// (dst[i], src[i]), both with edge i's timestamp.  keys[r] = composite key; pay[r] = the value (PAY_VAL), the
// neighbour (PAY_NBR) or nothing.  VEC: two edges per thread through 16-byte column loads (every column 16-byte
// aligned), the keys and payloads of both stored as vectors
template <int DIR, int PAY, typename V, bool VEC>
__global__ __launch_bounds__(256) void k_sl_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                 const V* __restrict__ val, const int64_t* __restrict__ ts, uint64_t n,
                                                 const SlGeom g, uint64_t* __restrict__ keys, V* __restrict__ pay) {
  const int tid = threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  // one edge, scalar stores (the unaligned path and the odd last edge)
  auto one = [&](uint64_t i) {
    const int64_t s = src[i], d = dst[i], t = ts[i];
    V v{};
    if constexpr (PAY == PAY_VAL) v = val[i];
    if constexpr (DIR == DIR_ALL) {
      keys[2 * i] = g.key(s, t);
      keys[2 * i + 1] = g.key(d, t);
      if constexpr (PAY == PAY_NBR) {
        pay[2 * i] = (V)d;
        pay[2 * i + 1] = (V)s;
      } else if constexpr (PAY == PAY_VAL) {
        pay[2 * i] = v;
        pay[2 * i + 1] = v;
      }
    } else {
      keys[i] = g.key(DIR == DIR_IN ? d : s, t);
      if constexpr (PAY == PAY_NBR) pay[i] = (V)(DIR == DIR_IN ? s : d);
      else if constexpr (PAY == PAY_VAL) pay[i] = v;
    }
  };
  if constexpr (!VEC) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + tid; i < n; i += stride) one(i);
  } else {
    const uint64_t npair = n >> 1;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + tid; q < npair; q += stride) {
      const u64x2 s = ld16<true>(src + 2 * q), d = ld16<true>(dst + 2 * q), t = ld16<true>(ts + 2 * q);
      V v0{}, v1{};
      if constexpr (PAY == PAY_VAL) {
        if constexpr (sizeof(V) == 8) {
          const u64x2 x = ld16<true>(val + 2 * q);
          v0 = (V)x.x;
          v1 = (V)x.y;
        } else {
          const u32x2 x = ld8w<true>(val + 2 * q);
          v0 = (V)x.x;
          v1 = (V)x.y;
        }
      }
      if constexpr (DIR == DIR_ALL) {
        u64x2* ko = reinterpret_cast<u64x2*>(keys + 4 * q);
        ko[0] = u64x2{g.key((int64_t)s.x, (int64_t)t.x), g.key((int64_t)d.x, (int64_t)t.x)};
        ko[1] = u64x2{g.key((int64_t)s.y, (int64_t)t.y), g.key((int64_t)d.y, (int64_t)t.y)};
        if constexpr (PAY == PAY_NBR) {
          u64x2* po = reinterpret_cast<u64x2*>(pay + 4 * q);
          po[0] = u64x2{d.x, s.x};
          po[1] = u64x2{d.y, s.y};
        } else if constexpr (PAY == PAY_VAL && sizeof(V) == 8) {
          u64x2* po = reinterpret_cast<u64x2*>(pay + 4 * q);
          po[0] = u64x2{(unsigned long long)v0, (unsigned long long)v0};
          po[1] = u64x2{(unsigned long long)v1, (unsigned long long)v1};
        } else if constexpr (PAY == PAY_VAL) {
          *reinterpret_cast<u32x4*>(pay + 4 * q) = u32x4{(uint32_t)v0, (uint32_t)v0, (uint32_t)v1, (uint32_t)v1};
        }
      } else {
        const u64x2 kv = DIR == DIR_IN ? d : s, nb = DIR == DIR_IN ? s : d;
        *reinterpret_cast<u64x2*>(keys + 2 * q) = u64x2{g.key((int64_t)kv.x, (int64_t)t.x), g.key((int64_t)kv.y, (int64_t)t.y)};
        if constexpr (PAY == PAY_NBR) *reinterpret_cast<u64x2*>(pay + 2 * q) = nb;
        else if constexpr (PAY == PAY_VAL && sizeof(V) == 8)
          *reinterpret_cast<u64x2*>(pay + 2 * q) = u64x2{(unsigned long long)v0, (unsigned long long)v1};
        else if constexpr (PAY == PAY_VAL) *reinterpret_cast<u32x2*>(pay + 2 * q) = u32x2{(uint32_t)v0, (uint32_t)v1};
      }
    }
    if ((n & 1) && blockIdx.x == 0 && tid == 0) one(n - 1);
  }
}

// ---- outputs of the reduce-by-key: the row's vertex, its value(s), and its window index --------------------
template <class Op, bool HAS_INIT>
struct SlicedValueOut {
  int64_t* keys;
  typename Op::Acc* vals;
  uint64_t* win;
  typename Op::Acc init;
  SlGeom g;
  __device__ void store(uint32_t u, int64_t k, typename Op::Acc a, uint32_t) const {
    keys[u] = g.vertex((uint64_t)k);
    win[u] = g.window((uint64_t)k);
    vals[u] = HAS_INIT ? Op::combine(init, a) : a;
  }
};
struct SlicedCountOut {
  int64_t* keys;
  int64_t* vals;
  uint64_t* win;
  int64_t init;
  SlGeom g;
  __device__ void store(uint32_t u, int64_t k, uint64_t a, uint32_t) const {
    keys[u] = g.vertex((uint64_t)k);
    win[u] = g.window((uint64_t)k);
    vals[u] = (int64_t)((uint64_t)init + a);
  }
};
struct SlicedDegMaxOut {
  int64_t* keys;
  int64_t* deg;
  int64_t* mx;
  uint64_t* win;
  int64_t init_max;
  SlGeom g;
  __device__ void store(uint32_t u, int64_t k, DegMax a, uint32_t) const {
    keys[u] = g.vertex((uint64_t)k);
    win[u] = g.window((uint64_t)k);
    deg[u] = (int64_t)a.cnt;
    mx[u] = a.mx > init_max ? a.mx : init_max;
  }
};

// ---- the windows of the rows ----------------------------------------------------------------------------------
// Row r starts a window when r == 0 or win[r] != win[r - 1].  One tile of SLW_TILE rows per block, SLW_ITEMS
// consecutive rows per thread: k_sl_wcount leaves the tile's number of starts in cnt[tile], k_scan_chunks turns
// cnt into the starts before each tile (and the total at cnt[tiles]), k_sl_wemit repeats the flags and writes.
constexpr int SLW_BLOCK = 256, SLW_ITEMS = 8, SLW_TILE = SLW_BLOCK * SLW_ITEMS;

__device__ __forceinline__ uint32_t sl_heads(const uint64_t* __restrict__ win, uint32_t U, uint64_t first, uint32_t& mask) {
  uint32_t c = 0;
  mask = 0;
  if (first < U) {
    uint64_t prev = first ? win[first - 1] : 0;
#pragma unroll
    for (int j = 0; j < SLW_ITEMS; ++j) {
      const uint64_t r = first + j;
      if (r < U) {
        const uint64_t w = win[r];
        if (r == 0 || w != prev) {
          mask |= 1u << j;
          ++c;
        }
        prev = w;
      }
    }
  }
  return c;
}

__global__ __launch_bounds__(SLW_BLOCK) void k_sl_wcount(const uint64_t* __restrict__ win, uint32_t U,
                                                         uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_w[SLW_BLOCK / WAVE];
  uint32_t mask, total;
  const uint32_t c = sl_heads(win, U, (uint64_t)blockIdx.x * SLW_TILE + (uint64_t)threadIdx.x * SLW_ITEMS, mask);
  block_exclusive_sum<SLW_BLOCK>(c, s_w, total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// cnt: the scanned tile counts, cnt[tiles] the number of windows (<= the capacity of both output columns)
__global__ __launch_bounds__(SLW_BLOCK) void k_sl_wemit(const uint64_t* __restrict__ win, uint32_t U,
                                                        const uint32_t* __restrict__ cnt, uint32_t tiles, const SlGeom g,
                                                        int64_t* __restrict__ window_start,
                                                        unsigned long long* __restrict__ row_begin) {
  __shared__ uint32_t s_w[SLW_BLOCK / WAVE];
  const uint64_t first = (uint64_t)blockIdx.x * SLW_TILE + (uint64_t)threadIdx.x * SLW_ITEMS;
  uint32_t mask, total;
  const uint32_t c = sl_heads(win, U, first, mask);
  uint32_t o = cnt[blockIdx.x] + block_exclusive_sum<SLW_BLOCK>(c, s_w, total);
#pragma unroll
  for (int j = 0; j < SLW_ITEMS; ++j) {
    if (mask & (1u << j)) {   // (set only for rows below U)
      window_start[o] = g.start(win[first + j]);
      row_begin[o] = first + j;
      ++o;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) row_begin[cnt[tiles]] = U;
}

// ---- host side ------------------------------------------------------------------------------------------------
int width_of(uint64_t span) { return span ? 64 - __builtin_clzll(span) : 0; }

template <int DIR>
gs_status launch_range(gs_ctx* c, const int64_t* src, const int64_t* dst, const int64_t* ts, uint64_t n,
                       unsigned long long* words) {
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(ts)) & 15) == 0;
  const unsigned g = grid_for(n, 2048, 2048);
  if (vec) hipLaunchKernelGGL((k_sl_range<DIR, true>), dim3(g), dim3(256), 0, c->stream, src, dst, ts, n, words);
  else hipLaunchKernelGGL((k_sl_range<DIR, false>), dim3(g), dim3(256), 0, c->stream, src, dst, ts, n, words);
  return hip_check(c, hipGetLastError(), "k_sl_range");
}

template <int DIR, int PAY, typename V>
gs_status launch_keys(gs_ctx* c, const int64_t* src, const int64_t* dst, const void* val, const int64_t* ts, uint64_t n,
                      const SlGeom& g, uint64_t* keys, void* pay) {
  const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) |
                       reinterpret_cast<uintptr_t>(ts) | (PAY == PAY_VAL ? reinterpret_cast<uintptr_t>(val) : 0);
  const unsigned grid = grid_for(n, 2048, 4096);
  if ((al & 15) == 0)
    hipLaunchKernelGGL((k_sl_keys<DIR, PAY, V, true>), dim3(grid), dim3(256), 0, c->stream, src, dst, (const V*)val, ts, n,
                       g, keys, (V*)pay);
  else
    hipLaunchKernelGGL((k_sl_keys<DIR, PAY, V, false>), dim3(grid), dim3(256), 0, c->stream, src, dst, (const V*)val, ts,
                       n, g, keys, (V*)pay);
  return hip_check(c, hipGetLastError(), "k_sl_keys");
}

template <int DIR>
gs_status launch_keys_pay(gs_ctx* c, int pay_kind, int vbytes, const int64_t* src, const int64_t* dst, const void* val,
                          const int64_t* ts, uint64_t n, const SlGeom& g, uint64_t* keys, void* pay) {
  if (pay_kind == PAY_NONE) return launch_keys<DIR, PAY_NONE, uint8_t>(c, src, dst, val, ts, n, g, keys, pay);
  if (pay_kind == PAY_NBR) return launch_keys<DIR, PAY_NBR, uint64_t>(c, src, dst, val, ts, n, g, keys, pay);
  if (vbytes == 4) return launch_keys<DIR, PAY_VAL, uint32_t>(c, src, dst, val, ts, n, g, keys, pay);
  return launch_keys<DIR, PAY_VAL, uint64_t>(c, src, dst, val, ts, n, g, keys, pay);
}

template <typename T, int OP>
gs_status sliced_value_rbk(gs_ctx* c, const Sorted& s, int64_t* keys, void* vals, uint64_t* win, const void* init,
                           const SlGeom& g, uint64_t* U) {
  using Op = ValueOp<T, OP>;
  const SlicedValueOut<Op, true> oi{keys, (T*)vals, win, init ? *(const T*)init : T{}, g};
  const SlicedValueOut<Op, false> on{keys, (T*)vals, win, T{}, g};
  if (s.wide) return init ? launch_rbk<uint64_t, Op>(c, s, oi, U) : launch_rbk<uint64_t, Op>(c, s, on, U);
  return init ? launch_rbk<uint32_t, Op>(c, s, oi, U) : launch_rbk<uint32_t, Op>(c, s, on, U);
}

template <typename T>
gs_status sliced_value_op(gs_ctx* c, int op, const Sorted& s, int64_t* keys, void* vals, uint64_t* win,
                          const void* init, const SlGeom& g, uint64_t* U) {
  switch (op) {
    case OP_SUM: return sliced_value_rbk<T, OP_SUM>(c, s, keys, vals, win, init, g, U);
    case OP_MIN: return sliced_value_rbk<T, OP_MIN>(c, s, keys, vals, win, init, g, U);
    case OP_MAX: return sliced_value_rbk<T, OP_MAX>(c, s, keys, vals, win, init, g, U);
  }
  return set_error(c, GS_EINVAL, "bad op %d", op);
}

// deg: the degree fold (op and init unused); else reduce (init NULL) or fold
gs_status slice_impl(gs_ctx* c, const gs_edge_batch* b, const int64_t* ts, int32_t ts_mem, int64_t window_ms,
                     int32_t dir, int32_t op, const void* init, bool deg, int64_t init_max, gs_sliced_out* out) {
  GS_TRY(check_batch(c, b, dir));
  if (!out || !out->n_windows || !out->n_rows) return set_error(c, GS_EINVAL, "bad gs_sliced_out");
  if (out->capacity_rows && (!out->keys || !out->vals || (deg && !out->vals2)))
    return set_error(c, GS_EINVAL, "bad gs_sliced_out: null row columns");
  if (out->capacity_windows && (!out->window_start || !out->row_begin))
    return set_error(c, GS_EINVAL, "bad gs_sliced_out: null window columns");
  if (out->mem != GS_MEM_HOST && out->mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_mem %d", out->mem);
  if (ts_mem != GS_MEM_HOST && ts_mem != GS_MEM_DEVICE) return set_error(c, GS_EINVAL, "bad gs_mem %d of ts", ts_mem);
  if (window_ms <= 0) return set_error(c, GS_EINVAL, "window of %lld ms", (long long)window_ms);
  if (b->n && !ts) return set_error(c, GS_EINVAL, "null ts");
  if (!deg) {
    if (op < GS_OP_SUM || op > GS_OP_COUNT) return set_error(c, GS_EINVAL, "bad op %d", op);
    if (op != GS_OP_COUNT && (b->val_dtype == GS_NONE || (b->n && !b->val)))
      return set_error(c, GS_EINVAL, "op %d needs edge values", op);
  }
  GS_TRY(begin_call(c));
  const uint64_t n = b->n, R = dir == GS_DIR_ALL ? 2 * n : n;
  const bool out_dev = out->mem == GS_MEM_DEVICE;
  if (R == 0) {
    *out->n_windows = 0;
    *out->n_rows = 0;
    if (out->row_begin) {
      if (out_dev) GS_HIP(hipMemsetAsync(out->row_begin, 0, 8, c->stream));
      else out->row_begin[0] = 0;
    }
    return GS_OK;
  }
  const bool count = !deg && op == GS_OP_COUNT;
  const int64_t *src, *dst;
  const void* val;
  GS_TRY(stage_batch(c, b, &src, &dst, &val, !deg && !count));
  if (ts_mem == GS_MEM_HOST) {
    GS_TRY(ensure(c, c->sl[0], n * 8));
    GS_HIP(hipMemcpyAsync(c->sl[0].p, ts, n * 8, hipMemcpyHostToDevice, c->stream));
    ts = c->sl[0].as<int64_t>();
  }

  // the ranges: [tiles + 1] tile counts of the rows' windows, then the four range words
  const uint64_t max_tiles = (R + SLW_TILE - 1) / SLW_TILE;
  const size_t words_at = ((max_tiles + 1) * 4 + 15) / 16 * 16;
  GS_TRY(ensure(c, c->sl[4], words_at + 32));
  auto* words = reinterpret_cast<unsigned long long*>(c->sl[4].as<char>() + words_at);
  GS_HIP(hipMemsetAsync(words, 0xFF, 16, c->stream));
  GS_HIP(hipMemsetAsync(words + 2, 0, 16, c->stream));
  switch (dir) {
    case DIR_IN: GS_TRY(launch_range<DIR_IN>(c, src, dst, ts, n, words)); break;
    case DIR_OUT: GS_TRY(launch_range<DIR_OUT>(c, src, dst, ts, n, words)); break;
    default: GS_TRY(launch_range<DIR_ALL>(c, src, dst, ts, n, words)); break;
  }
  GS_HIP(hipMemcpyAsync(c->host_small + 8, words, 32, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(host_wait(c));
  const int64_t tmin = (int64_t)(c->host_small[8] ^ SIGN), vmin = (int64_t)(c->host_small[9] ^ SIGN);
  const int64_t tmax = (int64_t)(c->host_small[10] ^ SIGN), vmax = (int64_t)(c->host_small[11] ^ SIGN);
  // window numbers ts / size (truncated, as ts - ts % size is): their span and the vertices' in unsigned words
  const uint64_t wspan = (uint64_t)(tmax / window_ms) - (uint64_t)(tmin / window_ms);
  const uint64_t vspan = (uint64_t)vmax - (uint64_t)vmin;
  const int wbits = width_of(wspan), vbits = width_of(vspan);
  if (wbits + vbits > 64)
    return set_error(c, GS_EUNSUPPORTED, "sliced key needs %d window bits + %d vertex bits; 64 fit", wbits, vbits);
  SlGeom g;
  g.size = window_ms;
  g.q0 = (uint64_t)(tmin / window_ms);
  g.v0 = (uint64_t)vmin;
  g.vbits = (uint32_t)vbits;
  g.vmask = vbits >= 64 ? ~0ull : (1ull << vbits) - 1;

  // composite keys and payloads
  const int vbytes = (int)dtype_bytes(b->val_dtype);
  const int pay_kind = deg ? PAY_NBR : count ? PAY_NONE : PAY_VAL;
  const int pb = deg ? 8 : count ? 0 : vbytes;
  GS_TRY(ensure(c, c->sl[1], R * 8));
  if (pb) GS_TRY(ensure(c, c->sl[2], R * (size_t)pb));
  uint64_t* keys = c->sl[1].as<uint64_t>();
  void* pay = pb ? c->sl[2].p : nullptr;
  switch (dir) {
    case DIR_IN: GS_TRY(launch_keys_pay<DIR_IN>(c, pay_kind, vbytes, src, dst, val, ts, n, g, keys, pay)); break;
    case DIR_OUT: GS_TRY(launch_keys_pay<DIR_OUT>(c, pay_kind, vbytes, src, dst, val, ts, n, g, keys, pay)); break;
    default: GS_TRY(launch_keys_pay<DIR_ALL>(c, pay_kind, vbytes, src, dst, val, ts, n, g, keys, pay)); break;
  }
  Sorted s;
  GS_TRY(sort_buffer(c, keys, pay, R, &s, std::max(1, wbits + vbits), pb ? pb : 4));

  // rows: straight into the caller's device columns when they hold every record, else staged
  const size_t ob = (deg || count) ? 8 : (size_t)vbytes;
  const bool direct = out_dev && out->capacity_rows >= R;
  int64_t* kd = out->keys;
  void* vd = out->vals;
  int64_t* md = out->vals2;
  if (!direct) {
    GS_TRY(ensure(c, c->out_keys, R * 8));
    GS_TRY(ensure(c, c->out_a, R * ob));
    if (deg) GS_TRY(ensure(c, c->out_b, R * 8));
    kd = c->out_keys.as<int64_t>();
    vd = c->out_a.p;
    md = c->out_b.as<int64_t>();
  }
  GS_TRY(ensure(c, c->sl[3], R * 8));
  uint64_t* win = c->sl[3].as<uint64_t>();
  uint64_t U = 0;
  if (deg) {
    const SlicedDegMaxOut o{kd, (int64_t*)vd, md, win, init_max, g};
    GS_TRY((s.wide ? launch_rbk<uint64_t, DegMaxOp>(c, s, o, &U) : launch_rbk<uint32_t, DegMaxOp>(c, s, o, &U)));
  } else if (count) {
    const SlicedCountOut o{kd, (int64_t*)vd, win, init ? *(const int64_t*)init : 0, g};
    GS_TRY((s.wide ? launch_rbk<uint64_t, CountOp>(c, s, o, &U) : launch_rbk<uint32_t, CountOp>(c, s, o, &U)));
  } else {
    switch (b->val_dtype) {
      case GS_I32: GS_TRY(sliced_value_op<int32_t>(c, op, s, kd, vd, win, init, g, &U)); break;
      case GS_I64: GS_TRY(sliced_value_op<int64_t>(c, op, s, kd, vd, win, init, g, &U)); break;
      case GS_F32: GS_TRY(sliced_value_op<float>(c, op, s, kd, vd, win, init, g, &U)); break;
      default: GS_TRY(sliced_value_op<double>(c, op, s, kd, vd, win, init, g, &U)); break;
    }
  }
  if (U == 0 || U > R) return set_error(c, GS_EDEVICE, "sliced reduce: %llu rows of %llu records", (unsigned long long)U,
                                        (unsigned long long)R);

  // the rows' windows
  const uint32_t tiles = (uint32_t)((U + SLW_TILE - 1) / SLW_TILE);   // <= max_tiles
  uint32_t* cnt = c->sl[4].as<uint32_t>();
  hipLaunchKernelGGL(k_sl_wcount, dim3(tiles), dim3(SLW_BLOCK), 0, c->stream, win, (uint32_t)U, cnt);
  GS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_scan_chunks<uint32_t>, dim3(1), dim3(SCAN_BLOCK), 0, c->stream, cnt, tiles);
  GS_HIP(hipGetLastError());
  GS_HIP(hipMemcpyAsync(c->host_small + 12, cnt + tiles, 4, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(host_wait(c));
  const uint64_t NW = (uint32_t)c->host_small[12];
  *out->n_windows = NW;
  *out->n_rows = U;
  if (NW > out->capacity_windows || U > out->capacity_rows)
    return set_error(c, GS_ECAPACITY, "output needs %llu windows and %llu rows", (unsigned long long)NW,
                     (unsigned long long)U);
  int64_t* wsd = out->window_start;
  auto* rbd = reinterpret_cast<unsigned long long*>(out->row_begin);
  if (!out_dev) {
    GS_TRY(ensure(c, c->sl[5], (2 * NW + 1) * 8));
    wsd = c->sl[5].as<int64_t>();
    rbd = c->sl[5].as<unsigned long long>() + NW;
  }
  hipLaunchKernelGGL(k_sl_wemit, dim3(tiles), dim3(SLW_BLOCK), 0, c->stream, win, (uint32_t)U, cnt, tiles, g, wsd, rbd);
  GS_HIP(hipGetLastError());
  if (!out_dev) {
    GS_TRY(deliver(c, out->window_start, wsd, NW * 8, out->mem));
    GS_TRY(deliver(c, out->row_begin, rbd, (NW + 1) * 8, out->mem));
  }
  if (!direct) {
    GS_TRY(deliver(c, out->keys, kd, U * 8, out->mem));
    GS_TRY(deliver(c, out->vals, vd, U * ob, out->mem));
    if (deg) GS_TRY(deliver(c, out->vals2, md, U * 8, out->mem));
  }
  if (!out_dev) GS_TRY(host_wait(c));
  return GS_OK;
}

}  // namespace
}  // namespace gs

extern "C" {

gs_status gs_slice_reduce(gs_ctx* c, const gs_edge_batch* b, const int64_t* ts, int32_t ts_mem, int64_t window_ms,
                          int32_t dir, int32_t op, const void* init, gs_sliced_out* out) {
  return slice_impl(c, b, ts, ts_mem, window_ms, dir, op, init, false, 0, out);
}

gs_status gs_slice_fold_degree_max(gs_ctx* c, const gs_edge_batch* b, const int64_t* ts, int32_t ts_mem,
                                   int64_t window_ms, int32_t dir, int64_t init_max, gs_sliced_out* out) {
  return slice_impl(c, b, ts, ts_mem, window_ms, dir, 0, nullptr, true, init_max, out);
}

}  // extern "C"

// gs_cc_common.hpp — the window aggregations over a union-find (gs_components.hip, gs_bipartite.hip): two
// forest policies, the kernels templated on them and the one host driver, uf_window.
//
// uf_window computes the state after a window from the window's edges and the previous state's rows, which
// join the window as constraints vertex -- label:
//   1. ids: when they span <= 2^28 values, the ids minus a common base index the word array directly (present
//      vertices found after the union-find and compacted by a scan); else compact ids from relabel_endpoints
//      (sort of the 2(n + m) endpoints, order-preserving)
//   2. union-find, one 32-bit word per vertex (the policy says what it holds), the larger root always linked
//      under the smaller one (atomicCAS on the root's word), find with pointer halving; parents only ever
//      decrease, so stale reads only cost retries.  From 65536 records on, in two phases (GS_CC_SAMPLE = k, a
//      power of two; 0 or 1: one pass): every k-th constraint first, a full compression, then the rest, which
//      skips a constraint that is decided already -- both endpoints in the giant tree (GS_CC_GIANT: a table of
//      1 or 2 bits per vertex, L2-resident) or under one parent.  On a skewed graph the sampled constraints
//      leave one giant tree, so most of the rest end after two reads: no find chains, no CAS, no halving writes
//   3. every vertex's root = the smallest id of its component, the canonical label of the partition
// The kernels have internal linkage: each translation unit launches its own instantiations (no relocatable
// device code).
#pragma once
#include <cstdlib>

#include "gs_ops.hpp"

namespace gs {

// ---- direct ids (the window's ids span <= CC_DIRECT_BITS bits: no relabel) ---------------------------
constexpr uint32_t CC_DIRECT_BITS = 28;

// OR of (id ^ k0) over both columns, k0 = *k0p (the first id of the call)
static __global__ __launch_bounds__(256) void k_cc_mask(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                        uint64_t n, const int64_t* __restrict__ k0p,
                                                        unsigned long long* __restrict__ mask) {
  const uint64_t k0 = (uint64_t)*k0p;
  uint64_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    m |= ((uint64_t)a[i] ^ k0) | ((uint64_t)b[i] ^ k0);
  m = wave_or(m);
  if ((threadIdx.x & 63) == 0 && m) atomicOr(mask, (unsigned long long)m);
}

static __global__ __launch_bounds__(256) void k_cc_flags(const uint8_t* __restrict__ mark, uint32_t V,
                                                         uint64_t* __restrict__ f) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V; i += gridDim.x * 256u) f[i] = mark[i];
}

static __global__ __launch_bounds__(256) void k_cc_concat(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                          uint64_t n, int64_t* __restrict__ oa, int64_t* __restrict__ ob) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    oa[i] = a[i];
    ob[i] = b[i];
  }
}

// the giant tree after phase 0 of the two-phase unions: the most frequent root among the parents of 1024 sampled
// edges' sources (one block; any root would be correct -- the table built from it only lets edges skip that are
// joined already)
// (compact ids: at != nullptr, the sources at[2e] instead of a[e] ^ key_xor; SHIFT: the root is parent[v] >> SHIFT,
// 1 for the signed words of gs_bipartite.hip)
template <int SHIFT>
static __global__ __launch_bounds__(1024) void k_cc_giant(const int64_t* __restrict__ a, const uint32_t* __restrict__ at,
                                                          uint64_t n, uint64_t key_xor, const uint32_t* __restrict__ parent,
                                                          uint32_t* __restrict__ giant) {
  __shared__ uint32_t s_r[1024];
  __shared__ unsigned long long s_best;
  const uint32_t t = threadIdx.x;
  const uint64_t e = (uint64_t)t * (n / 1024);
  s_r[t] = parent[at ? at[2 * e] : (uint32_t)((uint64_t)a[e] ^ key_xor)] >> SHIFT;
  if (t == 0) s_best = 0;
  __syncthreads();
  const uint32_t mine = s_r[t];
  uint32_t c = 0;
  for (int i = 0; i < 1024; ++i) c += s_r[i] == mine ? 1u : 0u;
  atomicMax(&s_best, ((unsigned long long)c << 32) | mine);
  __syncthreads();
  if (t == 0) *giant = (uint32_t)s_best;
}

// ---- the forest policies -----------------------------------------------------------------------------
// Forest<false>, the plain forest: word = parent.  A constraint (x, y) says "one component"; nothing can fail.
// Forest<true>, the signed forest: word = parent << 1 | parity, the vertex's side relative to its parent, read
// and written whole.  A constraint (x, y, d) says x and y lie on different sides (d = 1) or on the same side
// (d = 0); find halves paths by storing grandparent << 1 | (p_x ^ p_y), and a constraint whose endpoints already
// share a root is checked against their parities: a mismatch is an odd cycle.
//   Why stale reads and lost races are harmless there: the constraints whose CAS succeeded form a forest S
//   (each joins two trees: every vertex below a root has a larger id than the root), so S alone has a
//   2-colouring, unique per component up to a flip.  Every word ever stored -- a CAS or a halving -- is a
//   relation "x is on side p of a smaller vertex" that follows from S, hence true in that colouring; a stale
//   word only names an older, longer path.  Every other constraint was checked, at the moment its endpoints
//   shared a root, against parities that are true in S's colouring: no fail word means every constraint holds
//   in it (the graph is bipartite), a fail word means one does not (an odd cycle).  The walks terminate because
//   parents only decrease.
// Everything parity is behind `if constexpr (SIGNED)`: the plain instantiations read no sign column, keep no
// parity and touch no fail word.
template <bool SIGNED_>
struct Forest {
  static constexpr bool SIGNED = SIGNED_;
  static constexpr int SHIFT = SIGNED ? 1 : 0;                           // a word's parent: w >> SHIFT (k_cc_giant)
  static constexpr uint32_t TABLE_BITS = SIGNED ? 2 : 1;                 // the giant tree's table, bits per vertex
  static constexpr uint64_t MAX_VERTICES = (1ull << (32 - SHIFT)) - 1;   // what the parent field holds

  static __device__ __forceinline__ uint32_t word(uint32_t parent, uint32_t side) {
    if constexpr (SIGNED) return (parent << 1) | side;
    else return parent;
  }
  static __device__ __forceinline__ uint32_t root_word(uint32_t v) { return word(v, 0); }
  static __device__ __forceinline__ uint32_t side(uint32_t w) {
    if constexpr (SIGNED) return w & 1u;
    else return 0;
  }

  // root of x, *par ^= x's side relative to it (pointer halving on the way: x skips to its grandparent).  Two
  // spellings of one loop.  A single one in the plain loop's shape leaves the plain kernels' code as it is but
  // takes the signed hook kernels from 23 to 27 VGPRs and from 380 to 388 instructions; the signed spelling is the
  // one the bipartite measurements of DESIGN.md were taken with
  static __device__ __forceinline__ uint32_t find(uint32_t* w, uint32_t x, uint32_t* par) {
    if constexpr (SIGNED) {
      uint32_t wx = w[x], y = wx >> 1;
      if (y != x) {
        for (;;) {
          const uint32_t wy = w[y], z = wy >> 1;
          *par ^= wx & 1u;   // the start vertex relative to y
          if (z == y) break;
          w[x] = (z << 1) | ((wx ^ wy) & 1u);
          x = y;
          wx = wy;
          y = z;
        }
      }
      return y;
    } else {
      uint32_t y = w[x];
      if (y != x) {
        uint32_t z;
        while (y > (z = w[y])) {
          w[x] = z;
          x = y;
          y = z;
        }
      }
      return y;
    }
  }

  // phase 1 of the sampled unions, after phase 0's full compression.  Returns 0: not decided, 1: the constraint
  // holds already, 2: it closes an odd cycle (signed only).  Both endpoints in the giant tree (gtab, k_uf_table)
  // are decided before any word is read -- signed: by their sides relative to its root, which is why that table
  // holds two bits, one cannot tell the side; else two endpoints whose words name the same parent are decided
  // (parents only move to smaller ids) -- signed: by the two parity bits.  A shortcut never skips a constraint
  // undecided
  static __device__ __forceinline__ uint32_t decided(const uint32_t* w, const uint32_t* __restrict__ gtab, uint32_t x,
                                                     uint32_t y, uint32_t d) {
    constexpr uint32_t PER = 32 / TABLE_BITS;
    if (gtab) {
      const uint32_t tx = gtab[x / PER] >> ((x % PER) * TABLE_BITS), ty = gtab[y / PER] >> ((y % PER) * TABLE_BITS);
      if (tx & ty & 1u) return verdict((tx ^ ty) >> 1, d);
    }
    const uint32_t wx = w[x], wy = w[y];
    if ((wx >> SHIFT) != (wy >> SHIFT)) return 0;
    return verdict(wx ^ wy, d);
  }
  // two vertices of one tree whose sides relative to a common ancestor differ by bit 0 of `parity`, against d
  static __device__ __forceinline__ uint32_t verdict(uint32_t parity, uint32_t d) {
    if constexpr (SIGNED) return (parity & 1u) == d ? 1u : 2u;
    else return 1u;
  }

  // from vertex r up to its root; *par ^= the sides on the way (compress, emit)
  static __device__ __forceinline__ uint32_t walk(const uint32_t* w, uint32_t r, uint32_t* par) {
    for (;;) {
      const uint32_t wr = w[r];
      if ((wr >> SHIFT) == r) return r;
      if constexpr (SIGNED) *par ^= wr & 1u;
      r = wr >> SHIFT;
    }
  }
};
using PlainForest = Forest<false>;
using SignedForest = Forest<true>;

// ---- the kernels, templated on the policy ------------------------------------------------------------
template <class F>
static __global__ __launch_bounds__(256) void k_uf_init(uint32_t* __restrict__ w, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) w[i] = F::root_word(i);
}

template <class F>
static __device__ __forceinline__ void uf_report(uint32_t bad, uint32_t* fail) {
  if constexpr (F::SIGNED)
    if (wave_or(bad) && (threadIdx.x & 63) == 0) atomicOr(fail, 1u);
}

// The hook kernel: one constraint (x, y, d) per iteration.
//   DIRECT: x, y = a[e] ^ key_xor, b[e] ^ key_xor; a self-loop, a state row of a root, marks its vertex present (it
//     has no link).  signs == nullptr: window edges (d = 1), else state rows (d = !signs[e]).
//   else (compact ids): x, y = at[2e], at[2e + 1]; rows [0, m) are the state's (d = !signs[e]), the rest edges.
// phase 0: every (sample_mask + 1)-th constraint (sample_mask 0: every constraint, the one-pass unions); 1: the
// rest, shortcuts first.
// The union loop stands here, in the kernel's own loop body, and nowhere else: moved into a function of its own
// (a policy's unite(), inlined or not) the compiler lays the plain kernel out differently -- 227 instructions
// instead of 232 -- and that kernel is 1.8 % slower on an R-MAT s24 window (profiles/unionfind_refactor/).  As it
// stands the plain direct-id instantiation is instruction for instruction the kernel components ran before the two
// operators shared this file; the arguments it never reads come last for the same reason.
template <class F, bool DIRECT>
static __global__ __launch_bounds__(256) void k_uf_hook(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                        uint64_t n, uint64_t key_xor, uint32_t* w,
                                                        uint8_t* __restrict__ mark, uint32_t sample_mask, int phase,
                                                        const uint32_t* __restrict__ gtab, const uint32_t* __restrict__ at,
                                                        const uint8_t* __restrict__ signs, uint64_t m, uint32_t* fail) {
  uint32_t bad = 0;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
    if (((e & sample_mask) == 0) != (phase == 0)) continue;
    uint32_t x, y, d = 1;
    if constexpr (DIRECT) {
      x = (uint32_t)((uint64_t)a[e] ^ key_xor), y = (uint32_t)((uint64_t)b[e] ^ key_xor);
      if (x == y) {
        mark[x] = 1;
        continue;
      }
      if constexpr (F::SIGNED) d = signs ? (signs[e] ? 0u : 1u) : 1u;
    } else {
      x = at[2 * e], y = at[2 * e + 1];
      if (x == y) continue;
      if constexpr (F::SIGNED) d = e < m ? (signs[e] ? 0u : 1u) : 1u;
    }
    if (phase == 1) {
      const uint32_t k = F::decided(w, gtab, x, y, d);
      bad |= k >> 1;
      if (k) continue;
    }
    // the union loop: find both roots, CAS the larger root under the smaller, continue from the loser's root
    uint32_t pa = 0, pb = 0;
    uint32_t ra = F::find(w, x, &pa), rb = F::find(w, y, &pb);
    bool linked = false;
    while (ra != rb) {
      const bool s = ra > rb;
      const uint32_t hi = s ? ra : rb, lo = s ? rb : ra;
      const uint32_t old = atomicCAS(&w[hi], F::root_word(hi), F::word(lo, pa ^ pb ^ d));
      if (old == F::root_word(hi)) {   // hi was a root: linked under lo (on the side the constraint asks for)
        linked = true;
        break;
      }
      // hi got a parent meanwhile (always smaller): continue from its current root, parities accumulated
      uint32_t ph = 0;
      ra = F::find(w, old >> F::SHIFT, &ph);
      if constexpr (F::SIGNED) {
        ph ^= (s ? pa : pb) ^ (old & 1u);
        pb = s ? pb : pa;
        pa = ph;
      }
      rb = lo;
    }
    // one tree already: the constraint is checked against the two parities; a mismatch closes an odd cycle
    if constexpr (F::SIGNED) bad |= (!linked && (pa ^ pb) != d) ? 1u : 0u;
  }
  uf_report<F>(bad, fail);
}

// the giant tree's table after phase 0's compression (w[v] names v's root): per vertex, bit 0 = that root is
// the giant root and, signed, bit 1 = v's side relative to it
template <class F>
static __global__ __launch_bounds__(256) void k_uf_table(const uint32_t* __restrict__ w, uint32_t V,
                                                         const uint32_t* __restrict__ giant, uint32_t* __restrict__ gtab) {
  constexpr uint32_t PER = 32 / F::TABLE_BITS;
  const uint32_t g = *giant;
  for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < (V + PER - 1) / PER; t += gridDim.x * 256u) {
    uint32_t bits = 0;
    for (uint32_t k = 0; k < PER && t * PER + k < V; ++k) {
      const uint32_t wv = w[t * PER + k];
      bits |= (((wv >> F::SHIFT) == g ? 1u : 0u) | (F::side(wv) << 1)) << (F::TABLE_BITS * k);
    }
    gtab[t] = bits;
  }
}

// full compression: w[i] = (root, side relative to the root).  mark != nullptr (direct ids): a linked vertex is
// present and so is its root (every root of a linked tree is an endpoint: links only ever join the roots of
// trees that hold endpoints)
template <class F>
static __global__ __launch_bounds__(256) void k_uf_compress(uint32_t* w, uint32_t V, uint8_t* __restrict__ mark) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V; i += gridDim.x * 256u) {
    const uint32_t wi = w[i];
    uint32_t r = wi >> F::SHIFT, p = F::side(wi);
    if (r == i) continue;
    r = F::walk(w, r, &p);
    w[i] = F::word(r, p);
    if (mark) {
      mark[i] = 1;
      mark[r] = 1;
    }
  }
}

// direct ids, after k_uf_compress: present vertices -> (vertex, label[, sign]) at their scan positions
template <class F>
static __global__ __launch_bounds__(256) void k_uf_emit_ids(const uint32_t* __restrict__ w, const uint8_t* __restrict__ mark,
                                                            const uint64_t* __restrict__ pos, uint32_t V, uint64_t key_xor,
                                                            int64_t* __restrict__ keys, int64_t* __restrict__ labels,
                                                            uint8_t* __restrict__ signs) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V; i += gridDim.x * 256u) {
    if (!mark[i]) continue;
    const uint64_t at = pos[i];
    const uint32_t wi = w[i];
    keys[at] = (int64_t)(key_xor ^ i);
    labels[at] = (int64_t)(key_xor ^ (wi >> F::SHIFT));
    if constexpr (F::SIGNED) signs[at] = (uint8_t)((wi & 1u) ^ 1u);
  }
}

// compact ids: roots (= smallest compact id of the component) -> labels in original ids[, with the side]
template <class F>
static __global__ __launch_bounds__(256) void k_uf_emit(const uint32_t* __restrict__ w, const int64_t* __restrict__ uniq,
                                                        uint32_t n, int64_t* __restrict__ keys, int64_t* __restrict__ labels,
                                                        uint8_t* __restrict__ signs) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    uint32_t p = 0;
    const uint32_t r = F::walk(w, i, &p);
    keys[i] = uniq[i];
    labels[i] = uniq[r];
    if constexpr (F::SIGNED) signs[i] = (uint8_t)(p ^ 1u);
  }
}

// ---- the host driver ----------------------------------------------------------------------------------
// what an operator adds to its forest policy
struct UfOp {
  int path;               // gs_stage_times.path
  bool set_last_U;        // c->last_U = the vertex count
  const char* need;       // GS_ECAPACITY: the output's capacity, one %llu
  const char* word_full;  // GS_ECAPACITY: more compact ids than the word's parent field holds, one %llu; nullptr: no check
};

// The window's edges b and the previous state's rows prev (signs: signed forests only) -> the state after the
// window in out (signs / success: signed forests only; a window that closes an odd cycle sets *success = 0 and
// delivers no rows).  The caller has validated both, begun the call, recorded ev[0] and set *n_out = 0 (and
// *success = 1); everything from the state rows' copy to the stage times happens here.
template <class F>
static gs_status uf_window(gs_ctx* c, const UfOp& op, const gs_edge_batch* b, const gs_signed_batch& prev,
                           const gs_signed_out& out) {
  const uint64_t n = b->n, m = prev.n, N = n + m;
  if (N == 0) return GS_OK;
  // 1. the state's rows on the device (cc[0] / cc[1] rows [0, m), their signs in cc[3]); the window's columns are
  //    read where they are (no copy of them into one edge list -- 16 B read + 16 B written per edge -- unless the
  //    ids take the relabel path, which appends them at rows [m, N))
  GS_TRY(ensure(c, c->cc[0], N * 8));
  GS_TRY(ensure(c, c->cc[1], N * 8));
  if (F::SIGNED) GS_TRY(ensure(c, c->cc[3], m + 8));
  int64_t* A = c->cc[0].as<int64_t>();
  int64_t* Bc = c->cc[1].as<int64_t>();
  const uint8_t* S = F::SIGNED ? c->cc[3].as<uint8_t>() : nullptr;
  const int64_t *src = nullptr, *dst = nullptr;
  if (n) {
    const void* val;
    GS_TRY(stage_batch(c, b, &src, &dst, &val, false));
  }
  if (m) {
    const hipMemcpyKind k = prev.mem == GS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    GS_HIP(hipMemcpyAsync(A, prev.keys, m * 8, k, c->stream));
    GS_HIP(hipMemcpyAsync(Bc, prev.labels, m * 8, k, c->stream));
    if (F::SIGNED) GS_HIP(hipMemcpyAsync(c->cc[3].p, prev.signs, m, k, c->stream));
  }
  GS_HIP(hipGetLastError());
  // the two segments of constraints: the window's edges, the state's rows
  struct Seg {
    const int64_t *a, *b;
    const uint8_t* signs;
    uint64_t n;
  };
  const Seg seg[2] = {{src, dst, nullptr, n}, {A, Bc, S, m}};
  const Seg& big = n >= m ? seg[0] : seg[1];   // the larger segment's sources are sampled for the giant tree
  const int64_t* k0p = n ? src : A;
  char* sm = c->small.as<char>();
  unsigned long long* dmask = (unsigned long long*)(sm + SM_TABLE);
  uint32_t* fail = (uint32_t*)(sm + SM_TABLE + 8);   // (signed forests only)
  GS_HIP(hipMemsetAsync(dmask, 0, F::SIGNED ? 16 : 8, c->stream));
  // GS_CC_SAMPLE = k (a power of two): the two-phase unions over every k-th constraint first (0 or 1: one pass
  // over every constraint); GS_CC_GIANT=0: no giant-tree table (A/B)
  static const int sample_env = getenv("GS_CC_SAMPLE") ? atoi(getenv("GS_CC_SAMPLE")) : 16;   // (8: +0.2-0.4 ms, 32: +0.2, 64: +0.6)
  static const int giant_env = getenv("GS_CC_GIANT") ? atoi(getenv("GS_CC_GIANT")) : 1;
  const bool two_phase = sample_env > 1 && (sample_env & (sample_env - 1)) == 0 && N >= 65536;
  const uint32_t smask = two_phase ? (uint32_t)sample_env - 1 : 0;

  // the union-find over V words: the hooks of one phase are launched by hook(phase, table).  One pass: phase 0 with
  // sample mask 0, which is every constraint.  Two-phase: the sampled constraints, a full compression (every vertex
  // they linked then names its tree's root), the giant tree's table from ne >= 1024 sampled sources (a[] ^ key_xor,
  // or the compact pairs at[]), the rest.
  // The table lives in aux: cc[3] holds the signed state's signs, which phase 1 still reads.  aux is dead here
  // on both paths of both operators -- no step of this driver before the output staging touches it (stage_batch
  // fills in_src / in_dst, relabel_endpoints rl[], xscan its own buffers), and what an earlier call left in it
  // ended with that call -- and the table is dead after hook(1), before stage_out takes aux for the signs
  auto unions = [&](uint32_t* w, uint32_t V, uint8_t* mark, const int64_t* ga, const uint32_t* gat, uint64_t ne,
                    uint64_t key_xor, auto&& hook) -> gs_status {
    const uint32_t* gtab = nullptr;
    hook(0, gtab);
    if (!two_phase) return GS_OK;
    hipLaunchKernelGGL(k_uf_compress<F>, dim3(grid_for(V, 256, 16384)), dim3(256), 0, c->stream, w, V, mark);
    if (giant_env && ne >= 1024) {
      const size_t words = ((size_t)V * F::TABLE_BITS + 31) / 32;
      GS_TRY(ensure(c, c->aux, words * 4 + 64));
      uint32_t* t = c->aux.as<uint32_t>();
      uint32_t* giant = t + words;
      hipLaunchKernelGGL(k_cc_giant<F::SHIFT>, dim3(1), dim3(1024), 0, c->stream, ga, gat, ne, key_xor, (const uint32_t*)w,
                         giant);
      hipLaunchKernelGGL(k_uf_table<F>, dim3(grid_for(words, 256, 16384)), dim3(256), 0, c->stream, (const uint32_t*)w, V,
                         (const uint32_t*)giant, t);
      gtab = t;
    }
    hook(1, gtab);
    return GS_OK;
  };
  // the outputs: the caller's device columns, or staging for deliver
  const bool direct_out = out.mem == GS_MEM_DEVICE;
  int64_t* kd = out.keys;
  int64_t* ld = out.labels;
  uint8_t* sd = out.signs;
  auto stage_out = [&](uint64_t U) -> gs_status {
    *out.n_out = U;
    if (op.set_last_U) c->last_U = U;
    if (U > out.capacity) return set_error(c, GS_ECAPACITY, op.need, (unsigned long long)U);
    if (direct_out) return GS_OK;
    GS_TRY(ensure(c, c->out_keys, U * 8 + 8));
    GS_TRY(ensure(c, c->out_a, U * 8 + 8));
    kd = c->out_keys.as<int64_t>();
    ld = c->out_a.as<int64_t>();
    if (F::SIGNED) {
      GS_TRY(ensure(c, c->aux, U + 8));
      sd = c->aux.as<uint8_t>();
    }
    return GS_OK;
  };
  // after the emit (failed: instead of it): ev[3], the rows to the caller, the stage times
  auto finish = [&](bool failed, uint64_t U, uint32_t B) -> gs_status {
    GS_HIP(hipGetLastError());
    hipEventRecord(c->ev[3], c->stream);
    if (failed) {
      *out.success = 0;
      U = 0;
    }
    if (!direct_out) {
      GS_TRY(deliver(c, out.keys, kd, U * 8, out.mem));
      GS_TRY(deliver(c, out.labels, ld, U * 8, out.mem));
      if (F::SIGNED) GS_TRY(deliver(c, out.signs, sd, U, out.mem));
    }
    GS_TRY(host_wait(c));
    gs_stage_times& t = c->times;
    t = gs_stage_times{};
    t.pass_ms[0] = event_ms(c->ev[0], c->ev[1]);   // staging + id range + init / compact ids
    t.pass_ms[1] = event_ms(c->ev[1], c->ev[2]);   // union-find (+ compression)
    t.pass_ms[2] = event_ms(c->ev[2], c->ev[3]);   // present vertices -> labels
    t.total_ms = event_ms(c->ev[0], c->ev[3]);
    t.records = N;
    t.vertices = U;
    t.key_bits = B;
    t.path = op.path;
    return GS_OK;
  };

  // 2a. ids spanning <= CC_DIRECT_BITS bits: the union-find over the ids themselves (no relabel sort)
  for (const Seg& g : seg)
    if (g.n) hipLaunchKernelGGL(k_cc_mask, dim3(grid_for(g.n, 256, 8192)), dim3(256), 0, c->stream, g.a, g.b, g.n, k0p, dmask);
  GS_HIP(hipGetLastError());
  GS_HIP(hipMemcpyAsync(c->host_small + 12, dmask, 8, hipMemcpyDeviceToHost, c->stream));
  GS_HIP(hipMemcpyAsync(c->host_small + 13, k0p, 8, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(host_wait(c));
  const uint64_t mask = c->host_small[12], k0 = c->host_small[13];
  const uint32_t B = mask ? 64 - __builtin_clzll(mask) : 1;
  if (B <= CC_DIRECT_BITS) {
    const uint64_t key_xor = k0 & ~((1ull << B) - 1);
    const uint32_t V = 1u << B;
    GS_TRY(ensure(c, c->cc[2], (size_t)V * 4));
    GS_TRY(ensure(c, c->out_b, (size_t)V));
    GS_TRY(ensure(c, c->rl[2], (size_t)V * 8 + 8));
    GS_TRY(ensure(c, c->rl[3], (size_t)V * 8 + 8));
    uint32_t* w = c->cc[2].as<uint32_t>();
    uint8_t* mark = c->out_b.as<uint8_t>();
    const unsigned gv = grid_for(V, 256, 16384);
    hipLaunchKernelGGL(k_uf_init<F>, dim3(gv), dim3(256), 0, c->stream, w, V);
    GS_HIP(hipMemsetAsync(mark, 0, V, c->stream));
    hipEventRecord(c->ev[1], c->stream);
    GS_TRY(unions(w, V, mark, big.a, nullptr, big.n, key_xor, [&](int phase, const uint32_t* gtab) {
      for (const Seg& g : seg)
        if (g.n)
          hipLaunchKernelGGL((k_uf_hook<F, true>), dim3(grid_for(g.n, 256, 8192)), dim3(256), 0, c->stream, g.a, g.b, g.n, key_xor, w, mark,
                             smask, phase, gtab, (const uint32_t*)nullptr, g.signs, g.n, fail);
    }));
    hipLaunchKernelGGL(k_uf_compress<F>, dim3(gv), dim3(256), 0, c->stream, w, V, mark);
    GS_HIP(hipGetLastError());
    hipEventRecord(c->ev[2], c->stream);
    uint64_t* flags = c->rl[2].as<uint64_t>();
    uint64_t* pos = c->rl[3].as<uint64_t>();
    hipLaunchKernelGGL(k_cc_flags, dim3(gv), dim3(256), 0, c->stream, (const uint8_t*)mark, V, flags);
    GS_TRY(xscan(c, flags, V, pos));
    // the vertex count and, signed, the fail word in one read-back
    GS_HIP(hipMemcpyAsync(c->host_small + 12, pos + V, 8, hipMemcpyDeviceToHost, c->stream));
    if (F::SIGNED) GS_HIP(hipMemcpyAsync(c->host_small + 13, fail, 4, hipMemcpyDeviceToHost, c->stream));
    GS_TRY(host_wait(c));
    const uint64_t U = c->host_small[12];
    if (F::SIGNED && (uint32_t)c->host_small[13] != 0) return finish(true, 0, B);
    GS_TRY(stage_out(U));
    hipLaunchKernelGGL(k_uf_emit_ids<F>, dim3(gv), dim3(256), 0, c->stream, (const uint32_t*)w, (const uint8_t*)mark,
                       (const uint64_t*)pos, V, key_xor, kd, ld, sd);
    return finish(false, U, B);
  }
  // 2b. compact ids: the window's edges appended to the state's rows (one edge list for the relabel sort; row e
  //     keeps its position, so rows [0, m) take their d from the state's signs)
  if (n) hipLaunchKernelGGL(k_cc_concat, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, src, dst, n, A + m, Bc + m);
  const int64_t *ca, *cb, *uniq;
  uint64_t U = 0;
  GS_TRY(relabel_endpoints(c, A, Bc, N, &ca, &cb, &uniq, &U));
  if (op.word_full && U > F::MAX_VERTICES) return set_error(c, GS_ECAPACITY, op.word_full, (unsigned long long)U);
  hipEventRecord(c->ev[1], c->stream);
  // 3. union-find over the compact endpoint pairs (rl[4]: at[2e], at[2e + 1]); every compact id is present (no
  //    marks), and there is no final compression: the emit walks to the root
  GS_TRY(ensure(c, c->cc[2], U * 4 + 4));
  uint32_t* w = c->cc[2].as<uint32_t>();
  const uint32_t* at = c->rl[4].as<uint32_t>();
  const unsigned gu = grid_for(U, 256, 16384);
  hipLaunchKernelGGL(k_uf_init<F>, dim3(gu), dim3(256), 0, c->stream, w, (uint32_t)U);
  if (F::SIGNED) GS_HIP(hipMemsetAsync(fail, 0, 4, c->stream));   // (the relabel sort shares the small buffer)
  GS_TRY(unions(w, (uint32_t)U, nullptr, nullptr, at, N, 0, [&](int phase, const uint32_t* gtab) {
    hipLaunchKernelGGL((k_uf_hook<F, false>), dim3(grid_for(N, 256, 16384)), dim3(256), 0, c->stream, (const int64_t*)nullptr,
                       (const int64_t*)nullptr, N, 0ull, w, (uint8_t*)nullptr, smask, phase, gtab, at, S, m, fail);
  }));
  GS_HIP(hipGetLastError());
  hipEventRecord(c->ev[2], c->stream);
  if (F::SIGNED) {
    // the fail word decides whether anything is emitted (the relabel sort has waited on the host several times;
    // this is one more wait, on this path only)
    GS_HIP(hipMemcpyAsync(c->host_small + 13, fail, 4, hipMemcpyDeviceToHost, c->stream));
    GS_TRY(host_wait(c));
    if ((uint32_t)c->host_small[13] != 0) return finish(true, 0, 0);
  }
  // 4. labels
  GS_TRY(stage_out(U));
  hipLaunchKernelGGL(k_uf_emit<F>, dim3(gu), dim3(256), 0, c->stream, (const uint32_t*)w, uniq, (uint32_t)U, kd, ld, sd);
  return finish(false, U, 0);
}

}  // namespace gs

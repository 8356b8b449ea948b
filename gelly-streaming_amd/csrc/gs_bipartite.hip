// gs_bipartite.hip — BipartitenessCheck over a window stream:
//   library/BipartitenessCheck.java:40-136 on WindowGraphAggregation.java:47-65 (GraphAggregation's Merger,
//   transientState = false): every window's edges are folded into a Candidates (updateFunction ->
//   edgeToCandidate :57-64 -> Candidates.merge, example/util/Candidates.java:76-138) and merged into the
//   running state (combineFunction -> Candidates.merge).  The state after a window says whether the graph
//   of all the edges seen so far has an odd cycle and, if it has none, holds its components with every
//   vertex's side.
//
// gs_window_bipartite computes the canonical form of that state (DESIGN.md "BipartitenessCheck") on the
// GPU from the window's edges and the previous state's (vertex, label, sign) rows.  Both are constraints
// (x, y, d): x and y lie on different sides (d = 1: a window edge, a state row with sign false) or on the
// same side (d = 0: a state row with sign true); x == y only makes x present.
//   1. ids as gs_components.hip: the ids minus a common base when they span <= 2^28 values, else compact
//      ids from relabel_endpoints
//   2. signed union-find: one word per vertex, parent << 1 | parity (the vertex's side relative to its
//      parent), read and written whole.  The larger root is always linked under the smaller one
//      (atomicCAS on the root's word); find halves paths by storing grandparent << 1 | (p_x ^ p_y).
//      A constraint whose endpoints already share a root is checked against their parities: a mismatch is
//      an odd cycle and sets the fail word.
//      Why stale reads and lost races are harmless: the constraints whose CAS succeeded form a forest S
//      (each joins two trees: every vertex below a root has a larger id than the root), so S alone has a
//      2-colouring, unique per component up to a flip.  Every word ever stored -- a CAS or a halving --
//      is a relation "x is on side p of a smaller vertex" that follows from S, hence true in that
//      colouring; a stale word only names an older, longer path.  Every other constraint was checked, at
//      the moment its endpoints shared a root, against parities that are true in S's colouring: no fail
//      word means every constraint holds in it (the graph is bipartite), a fail word means one does not
//      (an odd cycle).  The walks terminate because parents only decrease.
//   3. full compression: every vertex's word = its component's smallest vertex << 1 | its side relative
//      to that vertex, the canonical (label, sign = parity == 0).
// The two-phase sampled unions of gs_components.hip are kept (GS_CC_SAMPLE), and every phase-1 shortcut
// tests parity: two endpoints whose words name the same parent are decided by their two parity bits, and
// the giant tree's table (GS_CC_GIANT) holds two bits per vertex -- in the tree, and on which side of its
// root -- because one bit cannot tell the side.  A shortcut either finds the constraint satisfied or sets
// the fail word; it never skips a constraint undecided.
#include "gs_cc_common.hpp"

namespace gs {

// root of x and *par = x's side relative to it (pointer halving on the way)
__device__ __forceinline__ uint32_t bp_find(uint32_t* w, uint32_t x, uint32_t* par) {
  uint32_t wx = w[x], y = wx >> 1, p = 0;
  if (y != x) {
    for (;;) {
      const uint32_t wy = w[y], z = wy >> 1;
      p ^= wx & 1u;   // the start vertex relative to y
      if (z == y) break;
      w[x] = (z << 1) | ((wx ^ wy) & 1u);   // x skips to its grandparent
      x = y;
      wx = wy;
      y = z;
    }
  }
  *par = p;
  return y;
}

// the constraint (x, y, d), x != y; returns 1 when it closes an odd cycle
__device__ __forceinline__ uint32_t bp_unite(uint32_t* w, uint32_t x, uint32_t y, uint32_t d) {
  uint32_t pa, pb;
  uint32_t a = bp_find(w, x, &pa), b = bp_find(w, y, &pb);
  while (a != b) {
    const bool s = a > b;
    const uint32_t hi = s ? a : b, lo = s ? b : a;
    const uint32_t old = atomicCAS(&w[hi], hi << 1, (lo << 1) | (pa ^ pb ^ d));
    if (old == hi << 1) return 0;   // hi was a root: linked under lo on the side the constraint asks for
    // hi got a parent meanwhile (always smaller): continue from its current root, parities accumulated
    uint32_t q;
    const uint32_t r = bp_find(w, old >> 1, &q);
    const uint32_t ph = (s ? pa : pb) ^ (old & 1u) ^ q, pl = s ? pb : pa;
    a = r;
    pa = ph;
    b = lo;
    pb = pl;
  }
  return (pa ^ pb) != d ? 1u : 0u;
}

// phase 1 of the sampled unions, after phase 0's full compression.  Returns 0: not decided, 1: the constraint
// holds already, 2: it closes an odd cycle.  Both endpoints in the giant tree (gtab: two L2-resident bits per
// vertex, k_bp_gtab) are decided by their sides relative to its root before any word is read; else two
// endpoints whose words name the same parent are decided by the two parity bits
__device__ __forceinline__ uint32_t bp_decided(const uint32_t* w, const uint32_t* __restrict__ gtab, uint32_t x, uint32_t y,
                                               uint32_t d) {
  if (gtab) {
    const uint32_t tx = gtab[x >> 4] >> ((x & 15u) * 2), ty = gtab[y >> 4] >> ((y & 15u) * 2);
    if (tx & ty & 1u) return (((tx ^ ty) >> 1) & 1u) == d ? 1u : 2u;
  }
  const uint32_t wx = w[x], wy = w[y];
  if ((wx >> 1) != (wy >> 1)) return 0;
  return ((wx ^ wy) & 1u) == d ? 1u : 2u;
}

__device__ __forceinline__ void bp_report(uint32_t bad, uint32_t* fail) {
  if (wave_or(bad) && (threadIdx.x & 63) == 0) atomicOr(fail, 1u);
}

__global__ __launch_bounds__(256) void k_bp_init(uint32_t* __restrict__ w, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) w[i] = i << 1;
}

// direct ids: constraints over (a[e] ^ key_xor, b[e] ^ key_xor); signs == nullptr: window edges (d = 1), else
// state rows (d = !signs[e]).  sample_mask / phase as k_cc_hook_ids_phase (phase < 0: every constraint)
__global__ __launch_bounds__(256) void k_bp_hook_ids(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                     const uint8_t* __restrict__ signs, uint64_t n, uint64_t key_xor,
                                                     uint32_t* w, uint8_t* __restrict__ mark, uint32_t sample_mask,
                                                     int phase, const uint32_t* __restrict__ gtab, uint32_t* fail) {
  uint32_t bad = 0;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
    if (phase >= 0 && ((e & sample_mask) == 0) != (phase == 0)) continue;
    const uint32_t x = (uint32_t)((uint64_t)a[e] ^ key_xor), y = (uint32_t)((uint64_t)b[e] ^ key_xor);
    if (x == y) {   // a self-loop, a state row of a root: the vertex is present, nothing to link
      mark[x] = 1;
      continue;
    }
    const uint32_t d = signs ? (signs[e] ? 0u : 1u) : 1u;
    if (phase == 1) {
      const uint32_t k = bp_decided(w, gtab, x, y, d);
      bad |= k >> 1;
      if (k) continue;
    }
    bad |= bp_unite(w, x, y, d);
  }
  bp_report(bad, fail);
}

// compact ids: constraints over the endpoint pairs at[2e], at[2e + 1]; rows [0, m) are the state's
__global__ __launch_bounds__(256) void k_bp_hook(const uint32_t* __restrict__ at, const uint8_t* __restrict__ signs,
                                                 uint64_t m, uint64_t ne, uint32_t* w, uint32_t sample_mask, int phase,
                                                 const uint32_t* __restrict__ gtab, uint32_t* fail) {
  uint32_t bad = 0;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (uint64_t)gridDim.x * 256) {
    if (phase >= 0 && ((e & sample_mask) == 0) != (phase == 0)) continue;
    const uint32_t x = at[2 * e], y = at[2 * e + 1];
    if (x == y) continue;
    const uint32_t d = e < m ? (signs[e] ? 0u : 1u) : 1u;
    if (phase == 1) {
      const uint32_t k = bp_decided(w, gtab, x, y, d);
      bad |= k >> 1;
      if (k) continue;
    }
    bad |= bp_unite(w, x, y, d);
  }
  bp_report(bad, fail);
}

// two bits per vertex after phase 0's compression (w[v] = root << 1 | side): bit 0 = v's root is the giant
// root, bit 1 = v's side relative to it.  One bit (k_cc_gbits) cannot decide a constraint; with the side it can
__global__ __launch_bounds__(256) void k_bp_gtab(const uint32_t* __restrict__ w, uint32_t V, const uint32_t* __restrict__ giant,
                                                 uint32_t* __restrict__ gtab) {
  const uint32_t g = *giant;
  for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < (V + 15) / 16; t += gridDim.x * 256u) {
    uint32_t bits = 0;
    for (uint32_t k = 0; k < 16 && t * 16 + k < V; ++k) {
      const uint32_t wv = w[t * 16 + k];
      bits |= (((wv >> 1) == g ? 1u : 0u) | ((wv & 1u) << 1)) << (2 * k);
    }
    gtab[t] = bits;
  }
}

// full compression: w[i] = root << 1 | side relative to the root.  mark != nullptr (direct ids): a linked
// vertex is present and so is its root (k_cc_compress)
__global__ __launch_bounds__(256) void k_bp_compress(uint32_t* w, uint32_t V, uint8_t* __restrict__ mark) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V; i += gridDim.x * 256u) {
    const uint32_t wi = w[i];
    uint32_t r = wi >> 1, p = wi & 1u;
    if (r == i) continue;
    for (;;) {
      const uint32_t wr = w[r];
      if ((wr >> 1) == r) break;
      p ^= wr & 1u;
      r = wr >> 1;
    }
    w[i] = (r << 1) | p;
    if (mark) {
      mark[i] = 1;
      mark[r] = 1;
    }
  }
}

// direct ids, after k_bp_compress: present vertices -> (vertex, label, sign) at their scan positions
__global__ __launch_bounds__(256) void k_bp_emit_ids(const uint32_t* __restrict__ w, const uint8_t* __restrict__ mark,
                                                     const uint64_t* __restrict__ pos, uint32_t V, uint64_t key_xor,
                                                     int64_t* __restrict__ keys, int64_t* __restrict__ labels,
                                                     uint8_t* __restrict__ signs) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V; i += gridDim.x * 256u) {
    if (!mark[i]) continue;
    const uint64_t at = pos[i];
    const uint32_t wi = w[i];
    keys[at] = (int64_t)(key_xor ^ i);
    labels[at] = (int64_t)(key_xor ^ (wi >> 1));
    signs[at] = (uint8_t)((wi & 1u) ^ 1u);
  }
}

// compact ids: roots (= smallest compact id of the component) -> labels in original ids, with the side
__global__ __launch_bounds__(256) void k_bp_emit(const uint32_t* __restrict__ w, const int64_t* __restrict__ uniq, uint32_t n,
                                                 int64_t* __restrict__ keys, int64_t* __restrict__ labels,
                                                 uint8_t* __restrict__ signs) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    uint32_t r = i, p = 0;
    for (;;) {
      const uint32_t wr = w[r];
      if ((wr >> 1) == r) break;
      p ^= wr & 1u;
      r = wr >> 1;
    }
    keys[i] = uniq[i];
    labels[i] = uniq[r];
    signs[i] = (uint8_t)(p ^ 1u);
  }
}

}  // namespace gs

using namespace gs;

extern "C" {

gs_status gs_window_bipartite(gs_ctx* c, const gs_edge_batch* b, const gs_signed_batch* prev, gs_signed_out* out) {
  if (!c) return GS_EINVAL;
  GS_TRY(check_batch(c, b, GS_DIR_OUT));
  if (prev && prev->n && (!prev->keys || !prev->labels || !prev->signs)) return set_error(c, GS_EINVAL, "bad previous state");
  if (!out || !out->n_out || !out->success || (out->capacity && (!out->keys || !out->labels || !out->signs)))
    return set_error(c, GS_EINVAL, "bad gs_signed_out");
  GS_TRY(begin_call(c));
  hipEventRecord(c->ev[0], c->stream);
  *out->n_out = 0;
  *out->success = 0;
  if (prev && prev->failed) return GS_OK;   // Candidates.java:78-80: a failed state stays failed
  const uint64_t n = b->n, m = prev ? prev->n : 0, N = n + m;
  *out->success = 1;
  if (N == 0) return GS_OK;
  // 1. the state's rows on the device (cc[0] / cc[1] rows [0, m), their signs in cc[3]); the window's columns are
  //    read where they are unless the ids take the relabel path, which appends them at rows [m, N)
  GS_TRY(ensure(c, c->cc[0], N * 8));
  GS_TRY(ensure(c, c->cc[1], N * 8));
  GS_TRY(ensure(c, c->cc[3], m + 8));
  int64_t* A = c->cc[0].as<int64_t>();
  int64_t* Bc = c->cc[1].as<int64_t>();
  uint8_t* S = c->cc[3].as<uint8_t>();
  const int64_t *src = nullptr, *dst = nullptr;
  if (n) {
    const void* val;
    GS_TRY(stage_batch(c, b, &src, &dst, &val, false));
  }
  if (m) {
    const hipMemcpyKind k = prev->mem == GS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    GS_HIP(hipMemcpyAsync(A, prev->keys, m * 8, k, c->stream));
    GS_HIP(hipMemcpyAsync(Bc, prev->labels, m * 8, k, c->stream));
    GS_HIP(hipMemcpyAsync(S, prev->signs, m, k, c->stream));
  }
  GS_HIP(hipGetLastError());
  // the two segments of constraints: the window's edges, the state's rows
  struct Seg {
    const int64_t *a, *b;
    const uint8_t* signs;
    uint64_t n;
  };
  const Seg seg[2] = {{src, dst, nullptr, n}, {A, Bc, S, m}};
  const int64_t* k0p = n ? src : A;
  char* sm = c->small.as<char>();
  unsigned long long* dmask = (unsigned long long*)(sm + SM_TABLE);
  uint32_t* fail = (uint32_t*)(sm + SM_TABLE + 8);
  GS_HIP(hipMemsetAsync(dmask, 0, 16, c->stream));
  // GS_CC_SAMPLE = k (a power of two): the two-phase unions over every k-th constraint first, as gs_components.hip
  static const int sample_env = getenv("GS_CC_SAMPLE") ? atoi(getenv("GS_CC_SAMPLE")) : 16;
  const bool two_phase = sample_env > 1 && (sample_env & (sample_env - 1)) == 0 && N >= 65536;
  const uint32_t smask = two_phase ? (uint32_t)sample_env - 1 : 0;
  // the giant tree's two-bit table for phase 1 (GS_CC_GIANT=0: none; A/B), from the sources of a[] ^ key_xor or of
  // the compact pairs at[]; it lives in aux, which is free until the outputs are staged
  static const int giant_env = getenv("GS_CC_GIANT") ? atoi(getenv("GS_CC_GIANT")) : 1;
  auto giant_table = [&](const int64_t* a, const uint32_t* at, uint64_t ne, uint64_t key_xor, const uint32_t* w, uint32_t V,
                         const uint32_t** tab) -> gs_status {
    *tab = nullptr;
    if (!giant_env || ne < 1024) return GS_OK;
    const size_t words = ((size_t)V + 15) / 16;
    GS_TRY(ensure(c, c->aux, words * 4 + 64));
    uint32_t* t = c->aux.as<uint32_t>();
    uint32_t* giant = t + words;
    hipLaunchKernelGGL(k_cc_giant<1>, dim3(1), dim3(1024), 0, c->stream, a, at, ne, key_xor, w, giant);
    hipLaunchKernelGGL(k_bp_gtab, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, 16384)), dim3(256), 0, c->stream, w,
                       V, (const uint32_t*)giant, t);
    *tab = t;
    return GS_OK;
  };
  const bool direct_out = out->mem == GS_MEM_DEVICE;
  int64_t* kd = out->keys;
  int64_t* ld = out->labels;
  uint8_t* sd = out->signs;
  auto stage_out = [&](uint64_t U) -> gs_status {
    if (direct_out) return GS_OK;
    GS_TRY(ensure(c, c->out_keys, U * 8 + 8));
    GS_TRY(ensure(c, c->out_a, U * 8 + 8));
    GS_TRY(ensure(c, c->aux, U + 8));
    kd = c->out_keys.as<int64_t>();
    ld = c->out_a.as<int64_t>();
    sd = c->aux.as<uint8_t>();
    return GS_OK;
  };
  auto finish = [&](uint64_t U, uint32_t B) -> gs_status {
    if (!direct_out) {
      GS_TRY(deliver(c, out->keys, kd, U * 8, out->mem));
      GS_TRY(deliver(c, out->labels, ld, U * 8, out->mem));
      GS_TRY(deliver(c, out->signs, sd, U, out->mem));
    }
    GS_TRY(host_wait(c));
    gs_stage_times& t = c->times;
    t = gs_stage_times{};
    t.pass_ms[0] = event_ms(c->ev[0], c->ev[1]);   // staging + id range + init / compact ids
    t.pass_ms[1] = event_ms(c->ev[1], c->ev[2]);   // signed union-find + compression
    t.pass_ms[2] = event_ms(c->ev[2], c->ev[3]);   // present vertices -> (label, sign)
    t.total_ms = event_ms(c->ev[0], c->ev[3]);
    t.records = N;
    t.vertices = U;
    t.key_bits = B;
    t.path = 5;
    return GS_OK;
  };
  // 2a. ids spanning <= CC_DIRECT_BITS bits: the union-find over the ids themselves (no relabel sort)
  {
    auto grid = [](uint64_t x) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((x + 255) / 256, 8192)); };
    for (const Seg& g : seg)
      if (g.n) hipLaunchKernelGGL(k_cc_mask, dim3(grid(g.n)), dim3(256), 0, c->stream, g.a, g.b, g.n, k0p, dmask);
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
      const unsigned gv = (unsigned)std::min<uint64_t>((V + 255) / 256, 16384);
      hipLaunchKernelGGL(k_bp_init, dim3(gv), dim3(256), 0, c->stream, w, V);
      GS_HIP(hipMemsetAsync(mark, 0, V, c->stream));
      hipEventRecord(c->ev[1], c->stream);
      const uint32_t* gtab = nullptr;
      if (two_phase) {
        for (const Seg& g : seg)
          if (g.n)
            hipLaunchKernelGGL(k_bp_hook_ids, dim3(grid(g.n)), dim3(256), 0, c->stream, g.a, g.b, g.signs, g.n, key_xor, w,
                               mark, smask, 0, gtab, fail);
        hipLaunchKernelGGL(k_bp_compress, dim3(gv), dim3(256), 0, c->stream, w, V, mark);
        const Seg& big = n >= m ? seg[0] : seg[1];   // the larger segment's sources are sampled
        GS_TRY(giant_table(big.a, nullptr, big.n, key_xor, w, V, &gtab));
      }
      for (const Seg& g : seg)
        if (g.n)
          hipLaunchKernelGGL(k_bp_hook_ids, dim3(grid(g.n)), dim3(256), 0, c->stream, g.a, g.b, g.signs, g.n, key_xor, w, mark,
                             smask, two_phase ? 1 : -1, gtab, fail);
      hipLaunchKernelGGL(k_bp_compress, dim3(gv), dim3(256), 0, c->stream, w, V, mark);
      GS_HIP(hipGetLastError());
      hipEventRecord(c->ev[2], c->stream);
      uint64_t* flags = c->rl[2].as<uint64_t>();
      uint64_t* pos = c->rl[3].as<uint64_t>();
      hipLaunchKernelGGL(k_cc_flags, dim3(gv), dim3(256), 0, c->stream, mark, V, flags);
      GS_TRY(xscan(c, flags, V, pos));
      // the vertex count and the fail word in one read-back
      GS_HIP(hipMemcpyAsync(c->host_small + 12, pos + V, 8, hipMemcpyDeviceToHost, c->stream));
      GS_HIP(hipMemcpyAsync(c->host_small + 13, fail, 4, hipMemcpyDeviceToHost, c->stream));
      GS_TRY(host_wait(c));
      const uint64_t U = c->host_small[12];
      const bool failed = (uint32_t)c->host_small[13] != 0;
      if (failed) {
        *out->success = 0;
        hipEventRecord(c->ev[3], c->stream);
        return finish(0, B);
      }
      *out->n_out = U;
      if (U > out->capacity) return set_error(c, GS_ECAPACITY, "bipartiteness state needs %llu vertices", (unsigned long long)U);
      GS_TRY(stage_out(U));
      hipLaunchKernelGGL(k_bp_emit_ids, dim3(gv), dim3(256), 0, c->stream, w, mark, pos, V, key_xor, kd, ld, sd);
      GS_HIP(hipGetLastError());
      hipEventRecord(c->ev[3], c->stream);
      return finish(U, B);
    }
  }
  // 2b. compact ids: the window's edges appended to the state's rows (one edge list for the relabel sort; row e
  //     keeps its position, so rows [0, m) take their d from the state's signs)
  if (n)
    hipLaunchKernelGGL(k_cc_concat, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 8192)), dim3(256), 0, c->stream, src,
                       dst, n, A + m, Bc + m);
  const int64_t *ca, *cb, *uniq;
  uint64_t U = 0;
  GS_TRY(relabel_endpoints(c, A, Bc, N, &ca, &cb, &uniq, &U));
  if (U >= (1ull << 31))
    return set_error(c, GS_ECAPACITY, "bipartiteness: %llu vertices, the packed parent word holds 2^31 - 1",
                     (unsigned long long)U);
  hipEventRecord(c->ev[1], c->stream);
  // 3. signed union-find over the compact endpoint pairs (rl[4]: at[2e], at[2e + 1])
  GS_TRY(ensure(c, c->cc[2], U * 4 + 4));
  uint32_t* w = c->cc[2].as<uint32_t>();
  const uint32_t* at = c->rl[4].as<uint32_t>();
  const unsigned gu = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((U + 255) / 256, 16384));
  const unsigned ge = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((N + 255) / 256, 16384));
  hipLaunchKernelGGL(k_bp_init, dim3(gu), dim3(256), 0, c->stream, w, (uint32_t)U);
  GS_HIP(hipMemsetAsync(fail, 0, 4, c->stream));   // (the relabel sort shares the small buffer)
  const uint32_t* gtab = nullptr;
  if (two_phase) {
    hipLaunchKernelGGL(k_bp_hook, dim3(ge), dim3(256), 0, c->stream, at, (const uint8_t*)S, m, N, w, smask, 0, gtab, fail);
    hipLaunchKernelGGL(k_bp_compress, dim3(gu), dim3(256), 0, c->stream, w, (uint32_t)U, (uint8_t*)nullptr);
    GS_TRY(giant_table(nullptr, at, N, 0, w, (uint32_t)U, &gtab));
  }
  hipLaunchKernelGGL(k_bp_hook, dim3(ge), dim3(256), 0, c->stream, at, (const uint8_t*)S, m, N, w, smask, two_phase ? 1 : -1,
                     gtab, fail);
  GS_HIP(hipGetLastError());
  hipEventRecord(c->ev[2], c->stream);
  // the fail word decides whether anything is emitted (the relabel sort has waited on the host several times; this
  // is one more wait, on this path only)
  GS_HIP(hipMemcpyAsync(c->host_small + 13, fail, 4, hipMemcpyDeviceToHost, c->stream));
  GS_TRY(host_wait(c));
  const bool failed = (uint32_t)c->host_small[13] != 0;
  if (failed) {
    *out->success = 0;
    hipEventRecord(c->ev[3], c->stream);
    return finish(0, 0);
  }
  // 4. labels and signs
  *out->n_out = U;
  if (U > out->capacity) return set_error(c, GS_ECAPACITY, "bipartiteness state needs %llu vertices", (unsigned long long)U);
  GS_TRY(stage_out(U));
  hipLaunchKernelGGL(k_bp_emit, dim3(gu), dim3(256), 0, c->stream, (const uint32_t*)w, uniq, (uint32_t)U, kd, ld, sd);
  GS_HIP(hipGetLastError());
  hipEventRecord(c->ev[3], c->stream);
  return finish(U, 0);
}

}  // extern "C"

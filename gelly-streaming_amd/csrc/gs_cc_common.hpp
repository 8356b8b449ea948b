// gs_cc_common.hpp — the id front end shared by the window aggregations over a union-find
// (gs_components.hip, gs_bipartite.hip): the id range of the window plus the state, the present-vertex
// flags of the direct path and the (state rows, window rows) edge list of the relabel path.  The kernels
// have internal linkage: each translation unit launches its own copy (no relocatable device code).
#pragma once
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

}  // namespace gs

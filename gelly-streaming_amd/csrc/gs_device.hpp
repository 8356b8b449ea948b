// gs_device.hpp — wave64 / inter-workgroup primitives shared by the gfx950 kernels.
//
// Conventions (cdna_hip_programming.md §1, §6 G16; MI355X_MICROARCH.md "Workgroup dispatch"):
//  - a wave is 64 lanes; ballots are 64-bit;
//  - look-back status words are single 8-byte granules written and read with agent-scope
//    relaxed atomics (global_store/load ... sc1), tagged with a per-call epoch so nothing has
//    to be zeroed between calls; multi-word payloads are stored sc1, drained with
//    `s_waitcnt vmcnt(0)`, then the flag granule is stored (the "sc1 payload -> vmcnt(0) ->
//    sc1 flag" hand-off);
//  - tiles are claimed in order from an atomic counter, so every tile a look-back waits on is
//    already running: the spin always terminates; it is still bounded and reports a timeout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {

constexpr int WAVE = 64;

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }

// number of set bits of `mask` in lanes below this one
__device__ __forceinline__ uint32_t mbcnt(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }

// lanes of the wave holding the same RADIX_BITS-bit digit as this lane (wave-level match_any)
template <int BITS>
__device__ __forceinline__ uint64_t match_digit(uint32_t d, uint64_t active) {
  uint64_t peers = active;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const uint64_t m = ballot((d >> b) & 1u);
    peers &= ((d >> b) & 1u) ? m : ~m;
  }
  return peers;
}

template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T x) {
  const int l = lane_id();
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    T y = __shfl_up(x, o, WAVE);
    if (l >= o) x += y;
  }
  return x;
}

__device__ __forceinline__ uint64_t wave_or(uint64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o, WAVE);
  return x;
}

// the wave's total, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
  return x;
}

// the wave's minimum / maximum, in every lane (T of 4 or 8 bytes)
template <typename T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T y = __shfl_xor(x, o, WAVE);
    x = y < x ? y : x;
  }
  return x;
}
template <typename T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T y = __shfl_xor(x, o, WAVE);
    x = y > x ? y : x;
  }
  return x;
}

// ---- streaming global loads ----------------------------------------------------------------------------------
// One load instruction per call, NT chosen at compile time: plain (the default cache policy) or non-temporal (`nt`:
// a stream that is read once).  The 16- and 8-byte forms are clang ext-vector types: a load through one stays one
// global_load_dwordx4 / dwordx2, where HIP's ulonglong2 / uint2 (structs of scalars) are split into their members
// and may be merged again differently -- a branch of 16-byte loads next to a branch of 8-byte loads compiled to one
// shared tail of 8-byte loads that way.  The address is aligned to the size of T.
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ u64x2 ld16(const void* p) { return ld_stream<NT>(static_cast<const u64x2*>(p)); }
template <bool NT>
__device__ __forceinline__ u32x4 ld16w(const void* p) { return ld_stream<NT>(static_cast<const u32x4*>(p)); }
template <bool NT>
__device__ __forceinline__ u32x2 ld8w(const void* p) { return ld_stream<NT>(static_cast<const u32x2*>(p)); }
template <bool NT>
__device__ __forceinline__ uint64_t ld8(const void* p) { return ld_stream<NT>(static_cast<const uint64_t*>(p)); }

// The block-wide exclusive scan of one value per thread: returns the sum of x over the threads below this one
// and sets `total` to the sum over the whole block, in every thread (an inclusive result is the return value + x).
//  - BLOCK is the launch's thread count (one-dimensional): exactly BLOCK / WAVE wave totals are written and read,
//    so a BLOCK that is not the launch's reads words nobody wrote, or misses waves;
//  - every thread of the block calls it, from uniform control flow: there is one barrier between the wave totals'
//    stores and their loads, and with RESYNC one more after the loads, so that s_w (BLOCK / WAVE words of LDS)
//    may be written again at once, by the next call for instance;
//  - with RESYNC = false the caller names the later barrier that every thread passes before s_w is written again.
template <int BLOCK, typename T, bool RESYNC = true>
__device__ __forceinline__ T block_exclusive_sum(T x, T* s_w, T& total) {
  static_assert(BLOCK % WAVE == 0 && BLOCK <= 1024, "whole waves, one workgroup");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  constexpr int NW = BLOCK / WAVE;
  const T inc = wave_inclusive_sum(x);
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  T off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const T v = s_w[i];
    off += i < w ? v : T(0);
    tot += v;
  }
  if constexpr (RESYNC) __syncthreads();
  total = tot;
  return off + inc - x;
}

// ---- one block scans an array in place (exclusive), SCAN_BLOCK threads ------------------------------------
// Two traversals, both kept: a contiguous chunk per thread (the class-major and owner-major count tables, a few
// thousand words read twice by the same thread), and coalesced SCAN_BLOCK-wide chunks with a carry (the tile
// counts of the text parser and of the u64 scan).  Neither has been measured on the other's inputs.
constexpr int SCAN_BLOCK = 1024;

// a[0 .. n) in place, thread t owning the ceil(n / SCAN_BLOCK) elements from t * ceil(n / SCAN_BLOCK); returns the
// total.  A thread's stores are ordered against the other threads' loads only by the caller's next barrier.
__device__ __forceinline__ uint32_t block_scan_array_chunked(uint32_t* a, uint32_t n, uint32_t* s_w) {
  const uint32_t per = (n + SCAN_BLOCK - 1) / SCAN_BLOCK, lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
  uint32_t sum = 0, total;
  for (uint32_t i = lo; i < hi; ++i) sum += a[i];
  uint32_t run = block_exclusive_sum<SCAN_BLOCK>(sum, s_w, total);
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t x = a[i];
    a[i] = run;
    run += x;
  }
  return total;
}

// a[0 .. n) in place and the total at a[n]: chunk after chunk of SCAN_BLOCK elements, the carry in a register
template <typename T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_chunks(T* __restrict__ a, uint32_t n) {
  __shared__ T s_w[SCAN_BLOCK / WAVE];
  T carry = 0;
  for (uint32_t base = 0; base < n; base += SCAN_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const T x = i < n ? a[i] : T(0);
    T total;
    const T below = block_exclusive_sum<SCAN_BLOCK>(x, s_w, total);
    if (i < n) a[i] = carry + below;
    carry += total;
  }
  if (threadIdx.x == 0) a[n] = carry;
}

// ---- look-back granules: [63:62] flag, [61:40] epoch, [39:0] value -------------------------
constexpr uint64_t FLAG_AGG = 1ull, FLAG_INC = 2ull;
constexpr uint32_t EPOCH_BITS = 22;
constexpr uint64_t VALUE_MASK = (1ull << 40) - 1;

__device__ __forceinline__ uint64_t granule(uint64_t flag, uint32_t epoch, uint64_t v) {
  return (flag << 62) | ((uint64_t)(epoch & ((1u << EPOCH_BITS) - 1)) << 40) | (v & VALUE_MASK);
}
__device__ __forceinline__ uint64_t g_flag(uint64_t g) { return g >> 62; }
__device__ __forceinline__ uint32_t g_epoch(uint64_t g) { return (uint32_t)(g >> 40) & ((1u << EPOCH_BITS) - 1); }
__device__ __forceinline__ uint64_t g_value(uint64_t g) { return g & VALUE_MASK; }

__device__ __forceinline__ void st_agent(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_agent(uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

constexpr uint32_t SPIN_LIMIT = 1u << 26;

// poll a granule until it carries `epoch` and a flag; bounded: sets *timeout and returns 0 on give-up
__device__ __forceinline__ uint64_t poll_granule(uint64_t* p, uint32_t epoch, uint32_t* timeout) {
  for (uint32_t spins = 0;; ++spins) {
    const uint64_t g = ld_agent(p);
    if (g_flag(g) != 0 && g_epoch(g) == (epoch & ((1u << EPOCH_BITS) - 1))) return g;
    if (spins >= SPIN_LIMIT) {
      atomicOr(timeout, 1u);
      return granule(FLAG_INC, epoch, 0);
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

}  // namespace gs

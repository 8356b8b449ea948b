// Achievable HBM rate for the C2 scatter's byte mix (read 16 B, write 4 B per record), perfectly
// coalesced: the floor the speculative scatter is compared with.
//   hipcc -O3 --offload-arch=gfx950 stream_mix.hip -o stream_mix && ./stream_mix
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

// The two kernels of round 3, as recorded.  They use some of each uint4's words only, so the compiler narrows
// their loads to four global_load_dword per iteration each: the figures DESIGN.md quotes from
// them were not taken with 16-byte loads.
__global__ __launch_bounds__(256) void k_mix(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                             uint2* __restrict__ out, uint64_t n2) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * 256) {
    const uint4 x = a[i], y = b[i];   // two records' keys, two records' values
    out[i] = make_uint2(x.x ^ y.x, x.z ^ y.z);
  }
}
// The same byte mix with every loaded word used: one global_load_dwordx4 per column (an ext-vector load), plain
// or non-temporal
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ __launch_bounds__(256) void k_mix16(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                               uint2* __restrict__ out, uint64_t n2) {
  const u32x4 *a4 = reinterpret_cast<const u32x4*>(a), *b4 = reinterpret_cast<const u32x4*>(b);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * 256) {
    const u32x4 x = NT ? __builtin_nontemporal_load(a4 + i) : a4[i], y = NT ? __builtin_nontemporal_load(b4 + i) : b4[i];
    out[i] = make_uint2(x.x ^ y.x ^ x.y ^ y.y, x.z ^ y.z ^ x.w ^ y.w);
  }
}
__global__ __launch_bounds__(256) void k_read(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                              uint32_t* __restrict__ sink, uint64_t n2) {
  uint32_t acc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * 256) {
    const uint4 x = a[i], y = b[i];
    acc ^= x.x ^ y.y ^ x.z ^ y.w;
  }
  if (acc == 0x12345678u) sink[0] = acc;
}

int main() {
  const uint64_t n = 1ull << 28;   // records
  uint4 *a, *b;
  uint2* o;
  uint32_t* sink;
  hipMalloc(&a, n * 8);
  hipMalloc(&b, n * 8);
  hipMalloc(&o, n * 4);
  hipMalloc(&sink, 64);
  hipMemset(a, 1, n * 8);
  hipMemset(b, 2, n * 8);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int grid : {1024, 2048, 4096, 8192}) {
    for (int which = 0; which < 4; ++which) {
      float best = 1e9f;
      for (int rep = 0; rep < 10; ++rep) {
        hipEventRecord(e0);
        if (which == 0) hipLaunchKernelGGL(k_mix, dim3(grid), dim3(256), 0, 0, a, b, o, n / 2);
        else if (which == 2) hipLaunchKernelGGL(k_mix16<false>, dim3(grid), dim3(256), 0, 0, a, b, o, n / 2);
        else if (which == 3) hipLaunchKernelGGL(k_mix16<true>, dim3(grid), dim3(256), 0, 0, a, b, o, n / 2);
        else hipLaunchKernelGGL(k_read, dim3(grid), dim3(256), 0, 0, a, b, sink, n / 2);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (rep > 1 && ms < best) best = ms;
      }
      const double bytes = which != 1 ? 20.0 * n : 16.0 * n;
      printf("%s grid %5d: %.4f ms  %.2f TB/s\n",
             which == 0   ? "read16+write4 (4 x dword) "
             : which == 1 ? "read16 (4 x dword)       "
             : which == 2 ? "read16+write4 (dwordx4)  "
                          : "read16+write4 (dwordx4 nt)",
             grid, best,
             bytes / (best * 1e-3) / 1e12);
    }
  }
  return 0;
}

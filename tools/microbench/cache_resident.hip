// Does a freshly written partition survive a read-once stream in the 256 MiB last-level cache, and does the
// load's cache hint decide it?  ("Stream loads".)  Per case: write P MB with plain stores, stream
// 4 GB of other memory with plain or non-temporal 16-byte loads (or nothing: the resident baseline), then time
// one re-read of P with plain or non-temporal 16-byte loads.  The median of 5 rounds, as GB/s of the re-read.
//   hipcc -O3 --offload-arch=gfx950 cache_resident.hip -o cache_resident && ./cache_resident
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdint>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);     \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)

__global__ __launch_bounds__(256) void k_fill(u32x4* __restrict__ p, uint64_t n16) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256) {
    const uint32_t x = (uint32_t)i;
    p[i] = u32x4{x, x + 1, x + 2, x + 3};
  }
}
template <bool NT>
__global__ __launch_bounds__(256) void k_read(const u32x4* __restrict__ p, uint32_t* __restrict__ sink, uint64_t n16) {
  uint32_t acc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256) {
    const u32x4 x = NT ? __builtin_nontemporal_load(p + i) : p[i];
    acc ^= x.x ^ x.y ^ x.z ^ x.w;
  }
  if (acc == 0x12345678u) sink[0] = acc;
}

int main() {
  const uint64_t stream_bytes = 4ull << 30, pmax = 256ull << 20;
  const int grid = 4096, rounds = 5;
  u32x4 *s, *p;
  uint32_t* sink;
  CHECK(hipMalloc(&s, stream_bytes));
  CHECK(hipMalloc(&p, pmax));
  CHECK(hipMalloc(&sink, 64));
  CHECK(hipMemset(s, 1, stream_bytes));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const char* stream_name[3] = {"none", "plain", "nt"};
  printf("P_MB stream reread  us      GB/s\n");
  for (uint64_t pmb : {64, 128, 192, 256}) {
    const uint64_t n16 = (pmb << 20) / 16;
    for (int stream = 0; stream < 3; ++stream) {
      for (int reread = 0; reread < 2; ++reread) {
        float t[rounds];
        for (int r = 0; r < rounds; ++r) {
          hipLaunchKernelGGL(k_fill, dim3(grid), dim3(256), 0, 0, p, n16);
          if (stream == 1) hipLaunchKernelGGL(k_read<false>, dim3(grid), dim3(256), 0, 0, s, sink, stream_bytes / 16);
          if (stream == 2) hipLaunchKernelGGL(k_read<true>, dim3(grid), dim3(256), 0, 0, s, sink, stream_bytes / 16);
          CHECK(hipEventRecord(e0));
          if (reread == 0) hipLaunchKernelGGL(k_read<false>, dim3(grid), dim3(256), 0, 0, p, sink, n16);
          else hipLaunchKernelGGL(k_read<true>, dim3(grid), dim3(256), 0, 0, p, sink, n16);
          CHECK(hipEventRecord(e1));
          CHECK(hipEventSynchronize(e1));
          CHECK(hipEventElapsedTime(&t[r], e0, e1));
        }
        std::sort(t, t + rounds);
        const float ms = t[rounds / 2];
        printf("%4llu %-6s %-6s %7.1f %8.1f\n", (unsigned long long)pmb, stream_name[stream], reread ? "nt" : "plain",
               ms * 1e3, (double)(pmb << 20) / (ms * 1e-3) / 1e9);
      }
    }
  }
  CHECK(hipDeviceSynchronize());
  return 0;
}

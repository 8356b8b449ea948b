// matching_cpu.cpp — one-thread host restatement of CentralizedWeightedMatching's mapper for
// tools/time_continuous.py's `matching` leg: the per-vertex form of CentralizedWeightedMatching.java:77-107
// (M is a matching, so the collision scan finds at most the edge at src and the edge at dst) over a
// std::unordered_map, events written to preallocated columns.  One thread is the reference's parallelism.
//
//   matching_cpu FILE N BATCHES PASSES
// FILE: int64 src[N * BATCHES], dst[...], val[...] (raw); "-" reads them from standard input.  Prints one
// JSON line: per pass and batch the milliseconds and the events; pass 0 starts from an empty matching, every
// later pass continues on the state.
//
// Build: g++ -O2 -std=c++17 -o tools/matching_cpu tools/matching_cpu.cpp
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

struct Entry {
  int64_t partner, val;
  bool matched, src_end;
};

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const uint64_t n = strtoull(argv[2], nullptr, 10), batches = strtoull(argv[3], nullptr, 10);
  const int passes = atoi(argv[4]);
  const uint64_t total = n * batches;
  std::vector<int64_t> col(3 * total);
  FILE* f = strcmp(argv[1], "-") ? fopen(argv[1], "rb") : stdin;
  if (!f || fread(col.data(), 8, 3 * total, f) != 3 * total) return 3;
  if (f != stdin) fclose(f);
  const int64_t *src = col.data(), *dst = src + total, *val = dst + total;
  std::vector<uint8_t> ot(3 * n);
  std::vector<int64_t> os(3 * n), od(3 * n), ov(3 * n);
  std::vector<uint64_t> oi(3 * n);
  std::unordered_map<int64_t, Entry> at;
  printf("{\"passes\": [");
  for (int p = 0; p < passes; ++p) {
    printf("%s{\"ms_per_batch\": [", p ? ", " : "");
    std::vector<uint64_t> events;
    for (uint64_t b = 0; b < batches; ++b) {
      const auto t0 = std::chrono::steady_clock::now();
      uint64_t k = 0;
      for (uint64_t i = b * n; i < (b + 1) * n; ++i) {
        const int64_t u = src[i], v = dst[i], w = val[i];
        Entry& eu = at[u];
        Entry& ev = at[v];   // references into an unordered_map stay valid across insertions
        const bool mu = eu.matched, mv = ev.matched && u != v && !(mu && eu.partner == v);
        const uint64_t sum = (mu ? (uint64_t)eu.val : 0) + (mv ? (uint64_t)ev.val : 0);
        if (!(w > (int64_t)(2 * sum))) continue;
        auto emit = [&](uint8_t t, int64_t a, int64_t c, int64_t x) {
          ot[k] = t; os[k] = a; od[k] = c; ov[k] = x; oi[k] = i - b * n; ++k;
        };
        if (mu) {
          emit(1, eu.src_end ? u : eu.partner, eu.src_end ? eu.partner : u, eu.val);
          at[eu.partner].matched = false;
        }
        if (mv) {
          emit(1, ev.src_end ? v : ev.partner, ev.src_end ? ev.partner : v, ev.val);
          at[ev.partner].matched = false;
        }
        eu = Entry{v, w, true, true};
        if (u != v) ev = Entry{u, w, true, false};
        emit(0, u, v, w);
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      printf("%s%.3f", b ? ", " : "", ms);
      events.push_back(k);
    }
    printf("], \"events_per_batch\": [");
    for (uint64_t b = 0; b < batches; ++b) printf("%s%llu", b ? ", " : "", (unsigned long long)events[b]);
    printf("]}");
  }
  printf("], \"vertices\": %llu, \"checksum\": %llu}\n", (unsigned long long)at.size(),
         (unsigned long long)(ot[0] + os[0] + od[0] + ov[0] + oi[0]));
  return 0;
}

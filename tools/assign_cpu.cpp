// assign_cpu.cpp — one-thread host restatement of AssignComponents (the reading include/gelly_hip.h builds) for
// tools/time_continuous.py's `assign` leg: vertex -> label in a std::unordered_map, label -> member vector, the
// records of a relabelled component ascending by vertex, written to growing columns.  One thread is the
// reference's parallelism for this operator.
//
//   assign_cpu FILE N BATCHES PASSES
// FILE: int64 src[N * BATCHES], dst[...] (raw); "-" reads them from standard input.  Prints one JSON line: per
// pass and batch the milliseconds and the records; pass 0 starts from an empty state, every later pass continues
// on it.
//
// Build: g++ -O2 -std=c++17 -o tools/assign_cpu tools/assign_cpu.cpp
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const uint64_t n = strtoull(argv[2], nullptr, 10), batches = strtoull(argv[3], nullptr, 10);
  const int passes = atoi(argv[4]);
  const uint64_t total = n * batches;
  std::vector<int64_t> col(2 * total);
  FILE* f = strcmp(argv[1], "-") ? fopen(argv[1], "rb") : stdin;
  if (!f || fread(col.data(), 8, 2 * total, f) != 2 * total) return 3;
  if (f != stdin) fclose(f);
  const int64_t *src = col.data(), *dst = src + total;
  std::vector<int64_t> ov, ol;
  std::vector<uint32_t> oe;
  std::unordered_map<int64_t, int64_t> label;
  std::unordered_map<int64_t, std::vector<int64_t>> members;
  uint64_t checksum = 0;
  printf("{\"passes\": [");
  for (int p = 0; p < passes; ++p) {
    printf("%s{\"ms_per_batch\": [", p ? ", " : "");
    std::vector<uint64_t> records;
    for (uint64_t b = 0; b < batches; ++b) {
      const auto t0 = std::chrono::steady_clock::now();
      ov.clear();
      ol.clear();
      oe.clear();
      for (uint64_t i = b * n; i < (b + 1) * n; ++i) {
        const int64_t s = src[i], t = dst[i];
        const uint32_t e = (uint32_t)(i - b * n);
        auto emit = [&](int64_t v, int64_t c) {
          ov.push_back(v);
          ol.push_back(c);
          oe.push_back(e);
        };
        // the component `from` takes the label `to`: its vertices ascending, then into to's member list
        auto relabel = [&](int64_t from, int64_t to) {
          std::vector<int64_t> moved = std::move(members[from]);
          members.erase(from);
          std::sort(moved.begin(), moved.end());
          for (int64_t v : moved) {
            emit(v, to);
            label[v] = to;
          }
          std::vector<int64_t>& into = members[to];
          if (into.empty()) into = std::move(moved);
          else into.insert(into.end(), moved.begin(), moved.end());
        };
        const auto is = label.find(s), it = label.find(t);
        const bool ks = is != label.end(), kt = it != label.end();
        if (!ks && !kt) {
          const int64_t m = std::min(s, t);
          label[s] = m;
          label[t] = m;
          std::vector<int64_t>& mem = members[m];
          mem.push_back(s);
          if (t != s) mem.push_back(t);
          emit(s, m);
          emit(t, m);
        } else if (ks != kt) {
          const int64_t c = ks ? is->second : it->second, x = ks ? t : s;
          if (x < c) {
            relabel(c, x);
            label[x] = x;
            members[x].push_back(x);
          } else {
            label[x] = c;
            members[c].push_back(x);
            emit(x, c);
          }
        } else if (is->second != it->second) {
          const int64_t a = is->second, c = it->second;
          relabel(std::max(a, c), std::min(a, c));
        }
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      printf("%s%.3f", b ? ", " : "", ms);
      records.push_back(ov.size());
      if (!ov.empty()) checksum += (uint64_t)ov.back() + (uint64_t)ol.back() + oe.back();
    }
    printf("], \"records_per_batch\": [");
    for (uint64_t b = 0; b < batches; ++b) printf("%s%llu", b ? ", " : "", (unsigned long long)records[b]);
    printf("]}");
  }
  printf("], \"vertices\": %llu, \"components\": %llu, \"checksum\": %llu}\n", (unsigned long long)label.size(),
         (unsigned long long)members.size(), (unsigned long long)checksum);
  return 0;
}

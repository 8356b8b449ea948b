/*
 * gs_oracle.c — CPU restatement of gelly-streaming's per-window neighbourhood path.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load this library, and only as the checker / the timed CPU
 * baseline.  The product path (gelly-streaming_amd + libgellyhip.so) never calls it.
 *
 * Parity pinning: the reference is Java on Flink 1.0.3 and cannot be compiled or run in
 * this container (no JDK, no Flink jars, no network).  This restatement is
 * pinned by the reference's own fixtures, extracted into tests/golden/ by
 * tests/golden/extract_reference_fixtures.py:
 *   - TestSlice.java:70-229 (9 goldens: fold/reduce/apply x OUT/IN/ALL on the 7-edge graph
 *     of GraphStreamTestUtils.java:56-67),
 *   - TestReverse / TestUndirected (direction expansion),
 *   - WindowTrianglesITCase + ExamplesTestData.java:21-34 (3 windows of 400 ms).
 * Large-scale behaviour is cross-checked between two independent triangle algorithms
 * (the reference's candidate rule vs. the forward algorithm) in tests/.
 *
 * Semantics restated (file:line in /root/reference/src/main/java/org/apache/flink/graph/streaming):
 *   direction expansion   SimpleEdgeStream.java:153-171 (OUT key=src; IN reverse() :332-341;
 *                         ALL undirected() :354-365 emits e then e.reverse())
 *   key selection         SimpleEdgeStream.java:173-183 (f0 of the expanded edge)
 *   reduceOnEdges         GraphWindowStream.java:101-121: left fold of values in arrival order,
 *                         output (vertex, value) after project(0, 2)
 *   foldNeighbors         GraphWindowStream.java:62-87: acc = f(acc, vertex, neighbour, value)
 *   applyOnNeighbors      GraphWindowStream.java:130-175: neighbours (f1, f2) in arrival order
 *   GenerateCandidateEdges example/WindowTriangles.java:83-116 (HashSet order, j >= i, i < len-1)
 *   CountTriangles        example/WindowTriangles.java:119-140 (int counters, emit iff edges > 0)
 *   timeWindowAll.sum(0)  example/WindowTriangles.java:66 (Integer sum, wraps mod 2^32)
 *   edge text input       example/WindowTriangles.java:175-185 (readTextFile, split("\\s"),
 *                         Long.parseLong; gso_parse_edges_text at the end of this file)
 *
 * Arithmetic follows Java: Integer/Long sums wrap (done in unsigned arithmetic),
 * Float/Double sums are IEEE adds in arrival order, min/max follow Math.min/Math.max.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GSO_API __attribute__((visibility("default")))

enum { DIR_IN = 0, DIR_OUT = 1, DIR_ALL = 2 };            /* EdgeDirection ordinals */
enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2, OP_COUNT = 3 };
enum { DT_I32 = 0, DT_I64 = 1, DT_F32 = 2, DT_F64 = 3, DT_NONE = 4 };

/* ------------------------------------------------------------------------------------ */
/* counter-based RNG + synthetic streams (bit-identical to gelly-streaming_amd/csrc/gen) */
/* ------------------------------------------------------------------------------------ */
GSO_API uint64_t gso_splitmix64(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static uint64_t perm_vertex(uint64_t x, int scale, uint64_t seed) {
  /* bijection on [0, 2^scale): 3 rounds of odd-multiply + xorshift, all mod 2^scale */
  const uint64_t mask = (scale >= 64) ? ~0ull : ((1ull << scale) - 1);
  const uint64_t k0 = gso_splitmix64(seed, 0x51) | 1ull, k1 = gso_splitmix64(seed, 0x52) | 1ull;
  const uint64_t a0 = gso_splitmix64(seed, 0x53), a1 = gso_splitmix64(seed, 0x54);
  const int sh = scale > 1 ? (scale + 1) / 2 : 1;
  x = (x * k0 + a0) & mask;
  x ^= x >> sh;
  x = (x * k1 + a1) & mask;
  x ^= x >> sh;
  x = (x * k0 + a1) & mask;
  return x;
}

/* R-MAT edge i: one 32-bit uniform per level (2 levels per splitmix64 call). */
static void rmat_edge(int scale, uint64_t seed, uint32_t a, uint32_t ab, uint32_t abc, uint64_t i,
                      uint64_t* s, uint64_t* d) {
  uint64_t u = 0, v = 0, r = 0;
  for (int l = 0; l < scale; ++l) {
    if ((l & 1) == 0) r = gso_splitmix64(seed, i * (uint64_t)((scale + 1) / 2) + (uint64_t)(l >> 1));
    const uint32_t x = (l & 1) ? (uint32_t)(r >> 32) : (uint32_t)r;
    const uint64_t sb = (x >= ab), db = (x >= a && x < ab) || (x >= abc);
    u = (u << 1) | sb;
    v = (v << 1) | db;
  }
  *s = u;
  *d = v;
}

GSO_API void gso_gen_rmat(int scale, uint64_t n, uint64_t seed, uint32_t a_fx, uint32_t b_fx,
                          uint32_t c_fx, int permute, int no_self_loops, uint64_t first_edge,
                          int64_t* src, int64_t* dst) {
  const uint32_t a = a_fx, ab = a_fx + b_fx, abc = a_fx + b_fx + c_fx;
  const uint64_t V = 1ull << scale;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = first_edge + k;
    uint64_t s, d;
    rmat_edge(scale, seed, a, ab, abc, i, &s, &d);
    if (no_self_loops && s == d) d = (s + 1 + gso_splitmix64(seed ^ 0x5E1F100Bull, i) % (V - 1)) & (V - 1);
    if (permute) { s = perm_vertex(s, scale, seed); d = perm_vertex(d, scale, seed); }
    src[k] = (int64_t)s;
    dst[k] = (int64_t)d;
  }
}

GSO_API void gso_gen_uniform(uint64_t V, uint64_t n, uint64_t seed, uint64_t first_edge, int64_t* src,
                             int64_t* dst) {
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = first_edge + k;
    const uint64_t s = gso_splitmix64(seed, 2 * i) % V;
    const uint64_t d = (s + 1 + gso_splitmix64(seed, 2 * i + 1) % (V - 1)) % V;
    src[k] = (int64_t)s;
    dst[k] = (int64_t)d;
  }
}

GSO_API void gso_gen_values(uint64_t n, uint64_t seed, uint64_t first_edge, int dtype, void* val) {
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t r = gso_splitmix64(seed ^ 0xA5A5A5A5F00DF00Dull, first_edge + k);
    switch (dtype) {
      case DT_I32: ((int32_t*)val)[k] = (int32_t)(r & 0xFFFF); break;
      case DT_I64: ((int64_t*)val)[k] = (int64_t)(r & 0xFFFF); break;
      case DT_F32: ((float*)val)[k] = (float)(r >> 40) * (1.0f / 16777216.0f); break;
      case DT_F64: ((double*)val)[k] = (double)(r >> 11) * (1.0 / 9007199254740992.0); break;
      default: break;
    }
  }
}

/* ------------------------------------------------------------------------------------ */
/* direction expansion: record r of the keyed stream                                    */
/* ------------------------------------------------------------------------------------ */
static inline uint64_t n_records(uint64_t n, int dir) { return dir == DIR_ALL ? 2 * n : n; }
/* returns edge index; sets key / neighbour of record r (ALL: r = 2i is e, r = 2i+1 is e.reverse()) */
static inline uint64_t record(const int64_t* src, const int64_t* dst, int dir, uint64_t r, int64_t* key,
                              int64_t* nbr) {
  uint64_t i = r;
  int rev = (dir == DIR_IN);
  if (dir == DIR_ALL) { i = r >> 1; rev = (int)(r & 1); }
  *key = rev ? dst[i] : src[i];
  *nbr = rev ? src[i] : dst[i];
  return i;
}

/* ------------------------------------------------------------------------------------ */
/* open-addressing map vertex -> slot (slots in first-arrival order)                    */
/* ------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t cap;   /* power of two */
  int64_t* keys;
  int64_t* slot;  /* -1 empty */
  uint64_t size;
} vmap;

static uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
static int vmap_init(vmap* m, uint64_t expect) {
  uint64_t c = 16;
  while (c < 2 * expect + 2) c <<= 1;
  m->cap = c;
  m->size = 0;
  m->keys = (int64_t*)malloc(c * sizeof(int64_t));
  m->slot = (int64_t*)malloc(c * sizeof(int64_t));
  if (!m->keys || !m->slot) return -1;
  memset(m->slot, 0xff, c * sizeof(int64_t));
  return 0;
}
static void vmap_free(vmap* m) { free(m->keys); free(m->slot); }
/* returns slot; *is_new set when inserted */
static inline int64_t vmap_get(vmap* m, int64_t k, int* is_new) {
  uint64_t h = mix64((uint64_t)k) & (m->cap - 1);
  for (;;) {
    if (m->slot[h] < 0) {
      m->keys[h] = k;
      m->slot[h] = (int64_t)m->size++;
      *is_new = 1;
      return m->slot[h];
    }
    if (m->keys[h] == k) { *is_new = 0; return m->slot[h]; }
    h = (h + 1) & (m->cap - 1);
  }
}

/* ------------------------------------------------------------------------------------ */
/* Java arithmetic                                                                        */
/* ------------------------------------------------------------------------------------ */
static inline double java_min_d(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && signbit(b)) return b;
  return (a <= b) ? a : b;
}
static inline double java_max_d(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && signbit(a)) return b;
  return (a >= b) ? a : b;
}
static inline float java_min_f(float a, float b) {
  if (a != a) return a;
  if (a == 0.0f && b == 0.0f && signbit(b)) return b;
  return (a <= b) ? a : b;
}
static inline float java_max_f(float a, float b) {
  if (a != a) return a;
  if (a == 0.0f && b == 0.0f && signbit(a)) return b;
  return (a >= b) ? a : b;
}

/* acc (8 bytes, typed by dtype) = op(acc, value of edge i) */
static inline void apply_op(int op, int dtype, uint64_t* acc, const void* val, uint64_t i) {
  switch (dtype) {
    case DT_I32: {
      int32_t a = (int32_t)(uint32_t)*acc, v = ((const int32_t*)val)[i];
      if (op == OP_SUM) a = (int32_t)((uint32_t)a + (uint32_t)v);
      else if (op == OP_MIN) a = v < a ? v : a;
      else if (op == OP_MAX) a = v > a ? v : a;
      *acc = (uint32_t)a;
      break;
    }
    case DT_I64: {
      int64_t a = (int64_t)*acc, v = ((const int64_t*)val)[i];
      if (op == OP_SUM) a = (int64_t)((uint64_t)a + (uint64_t)v);
      else if (op == OP_MIN) a = v < a ? v : a;
      else if (op == OP_MAX) a = v > a ? v : a;
      *acc = (uint64_t)a;
      break;
    }
    case DT_F32: {
      float a, v = ((const float*)val)[i];
      uint32_t bits = (uint32_t)*acc;
      memcpy(&a, &bits, 4);
      if (op == OP_SUM) a = a + v;
      else if (op == OP_MIN) a = java_min_f(a, v);
      else if (op == OP_MAX) a = java_max_f(a, v);
      memcpy(&bits, &a, 4);
      *acc = bits;
      break;
    }
    case DT_F64: {
      double a, v = ((const double*)val)[i];
      memcpy(&a, acc, 8);
      if (op == OP_SUM) a = a + v;
      else if (op == OP_MIN) a = java_min_d(a, v);
      else if (op == OP_MAX) a = java_max_d(a, v);
      memcpy(acc, &a, 8);
      break;
    }
  }
}
static inline uint64_t load_val(int dtype, const void* val, uint64_t i) {
  uint64_t r = 0;
  switch (dtype) {
    case DT_I32: r = (uint32_t)((const int32_t*)val)[i]; break;
    case DT_I64: r = (uint64_t)((const int64_t*)val)[i]; break;
    case DT_F32: memcpy(&r, (const float*)val + i, 4); break;
    case DT_F64: memcpy(&r, (const double*)val + i, 8); break;
  }
  return r;
}
static inline size_t dt_size(int dtype) { return (dtype == DT_I32 || dtype == DT_F32) ? 4 : 8; }
static inline void store_val(int dtype, void* out, uint64_t j, uint64_t bits) {
  if (dt_size(dtype) == 4) ((uint32_t*)out)[j] = (uint32_t)bits;
  else ((uint64_t*)out)[j] = bits;
}

/* sort (key, slot) pairs by key so outputs ascend like the engine's */
typedef struct { int64_t k; int64_t s; } kv;
static int cmp_kv(const void* a, const void* b) {
  const int64_t x = ((const kv*)a)->k, y = ((const kv*)b)->k;
  return (x > y) - (x < y);
}
static kv* sorted_slots(vmap* m) {
  kv* p = (kv*)malloc((m->size ? m->size : 1) * sizeof(kv));
  uint64_t j = 0;
  for (uint64_t h = 0; h < m->cap; ++h)
    if (m->slot[h] >= 0) { p[j].k = m->keys[h]; p[j].s = m->slot[h]; ++j; }
  qsort(p, m->size, sizeof(kv), cmp_kv);
  return p;
}

/* ------------------------------------------------------------------------------------ */
/* reduceOnEdges / foldNeighbors with a built-in associative op                          */
/* ------------------------------------------------------------------------------------ */
/* has_init = 0: reduceOnEdges (acc starts at the first value, GraphWindowStream.java:116-120)
 * has_init = 1: foldNeighbors (acc starts at a copy of init, GraphWindowStream.java:62-80)
 * COUNT: acc is an Int64 count (init + number of records).  Returns U, or -1 when cap < U. */
static int64_t window_fold(const int64_t* src, const int64_t* dst, const void* val, uint64_t n,
                           int dtype, int dir, int op, int has_init, uint64_t init_bits,
                           int64_t* out_keys, void* out_vals, uint64_t cap) {
  const uint64_t R = n_records(n, dir);
  vmap m;
  if (vmap_init(&m, R < 1024 ? R : R / 2) != 0) return -2;
  uint64_t* acc = (uint64_t*)malloc((R ? R : 1) * sizeof(uint64_t));
  for (uint64_t r = 0; r < R; ++r) {
    int64_t key, nbr;
    const uint64_t i = record(src, dst, dir, r, &key, &nbr);
    int is_new;
    const int64_t s = vmap_get(&m, key, &is_new);
    if (op == OP_COUNT) {
      if (is_new) acc[s] = has_init ? init_bits : 0;
      acc[s] += 1;
    } else if (is_new && !has_init) {
      acc[s] = load_val(dtype, val, i);
    } else {
      if (is_new) acc[s] = init_bits;
      apply_op(op, dtype, &acc[s], val, i);
    }
  }
  const uint64_t U = m.size;
  if (U <= cap) {
    kv* p = sorted_slots(&m);
    const int odt = (op == OP_COUNT) ? DT_I64 : dtype;
    for (uint64_t j = 0; j < U; ++j) {
      out_keys[j] = p[j].k;
      store_val(odt, out_vals, j, acc[p[j].s]);
    }
    free(p);
  }
  free(acc);
  vmap_free(&m);
  return U <= cap ? (int64_t)U : -1 - (int64_t)U;
}

GSO_API int64_t gso_window_reduce(const int64_t* src, const int64_t* dst, const void* val, uint64_t n,
                                  int dtype, int dir, int op, int64_t* out_keys, void* out_vals,
                                  uint64_t cap) {
  return window_fold(src, dst, val, n, dtype, dir, op, 0, 0, out_keys, out_vals, cap);
}

GSO_API int64_t gso_window_fold(const int64_t* src, const int64_t* dst, const void* val, uint64_t n,
                                int dtype, int dir, int op, const void* init, int64_t* out_keys,
                                void* out_vals, uint64_t cap) {
  const uint64_t ib = (op == OP_COUNT) ? (uint64_t)*(const int64_t*)init : load_val(dtype, init, 0);
  return window_fold(src, dst, val, n, dtype, dir, op, 1, ib, out_keys, out_vals, cap);
}

/* foldNeighbors(new Tuple3(0, 0, init_max), degree/max-neighbour fold) — TestSlice.java:233-239 shape */
GSO_API int64_t gso_window_fold_degree_max(const int64_t* src, const int64_t* dst, uint64_t n, int dir,
                                           int64_t init_max, int64_t* out_keys, int64_t* out_deg,
                                           int64_t* out_max, uint64_t cap) {
  const uint64_t R = n_records(n, dir);
  vmap m;
  if (vmap_init(&m, R < 1024 ? R : R / 2) != 0) return -2;
  int64_t* deg = (int64_t*)malloc((R ? R : 1) * sizeof(int64_t));
  int64_t* mx = (int64_t*)malloc((R ? R : 1) * sizeof(int64_t));
  for (uint64_t r = 0; r < R; ++r) {
    int64_t key, nbr;
    record(src, dst, dir, r, &key, &nbr);
    int is_new;
    const int64_t s = vmap_get(&m, key, &is_new);
    if (is_new) { deg[s] = 0; mx[s] = init_max; }
    deg[s] += 1;
    if (nbr > mx[s]) mx[s] = nbr;
  }
  const uint64_t U = m.size;
  if (U <= cap) {
    kv* p = sorted_slots(&m);
    for (uint64_t j = 0; j < U; ++j) {
      out_keys[j] = p[j].k;
      out_deg[j] = deg[p[j].s];
      out_max[j] = mx[p[j].s];
    }
    free(p);
  }
  free(deg); free(mx); vmap_free(&m);
  return U <= cap ? (int64_t)U : -1 - (int64_t)U;
}

/* ------------------------------------------------------------------------------------ */
/* applyOnNeighbors grouping: CSR in arrival order (GraphWindowStream.java:144-175)      */
/* ------------------------------------------------------------------------------------ */
GSO_API int64_t gso_window_csr(const int64_t* src, const int64_t* dst, const void* val, uint64_t n,
                               int dtype, int dir, int64_t* keys, uint64_t* offsets, int64_t* nbrs,
                               void* vals, uint64_t cap_v) {
  const uint64_t R = n_records(n, dir);
  vmap m;
  if (vmap_init(&m, R < 1024 ? R : R / 2) != 0) return -2;
  int64_t* slot_of = (int64_t*)malloc((R ? R : 1) * sizeof(int64_t));
  uint64_t* cnt = (uint64_t*)calloc(R ? R : 1, sizeof(uint64_t));
  for (uint64_t r = 0; r < R; ++r) {
    int64_t key, nbr;
    record(src, dst, dir, r, &key, &nbr);
    int is_new;
    slot_of[r] = vmap_get(&m, key, &is_new);
    cnt[slot_of[r]]++;
  }
  const uint64_t U = m.size;
  if (U <= cap_v) {
    kv* p = sorted_slots(&m);
    uint64_t* start = (uint64_t*)malloc((U ? U : 1) * sizeof(uint64_t));
    uint64_t off = 0;
    for (uint64_t j = 0; j < U; ++j) {
      keys[j] = p[j].k;
      offsets[j] = off;
      start[p[j].s] = off;
      off += cnt[p[j].s];
    }
    offsets[U] = off;
    for (uint64_t r = 0; r < R; ++r) {
      int64_t key, nbr;
      const uint64_t i = record(src, dst, dir, r, &key, &nbr);
      const uint64_t o = start[slot_of[r]]++;
      nbrs[o] = nbr;
      if (vals && dtype != DT_NONE) store_val(dtype, vals, o, load_val(dtype, val, i));
    }
    free(start);
    free(p);
  }
  free(slot_of); free(cnt); vmap_free(&m);
  return U <= cap_v ? (int64_t)U : -1 - (int64_t)U;
}

/* ------------------------------------------------------------------------------------ */
/* java.util.HashSet<Long> iteration order (JDK 8+ HashMap)                              */
/* ------------------------------------------------------------------------------------ */
/* HashSet() -> HashMap(16, 0.75): table doubles when ++size > 0.75*cap.  Long.hashCode =
 * (int)(x ^ (x >>> 32)); HashMap.hash spreads h ^ (h >>> 16); bucket = hash & (cap-1).
 * Iteration walks buckets 0..cap-1, each bin in insertion order (resize splits preserve
 * order) -- as long as no bin ever reaches 9 nodes; hashset_order below simulates the whole map. */
GSO_API uint64_t gso_java_hashset_cap(uint64_t k) {
  uint64_t cap = 16;
  while ((double)k > 0.75 * (double)cap) cap <<= 1;
  return cap;
}
GSO_API uint32_t gso_java_long_bucket(int64_t x, uint64_t cap) {
  const uint32_t h = (uint32_t)((uint64_t)x ^ ((uint64_t)x >> 32));
  return (h ^ (h >> 16)) & (uint32_t)(cap - 1);
}
typedef struct { uint32_t b; uint32_t ord; int64_t x; } hsent;
static int cmp_hs(const void* a, const void* b) {
  const hsent* p = (const hsent*)a; const hsent* q = (const hsent*)b;
  if (p->b != q->b) return p->b < q->b ? -1 : 1;
  return (p->ord > q->ord) - (p->ord < q->ord);
}

/* The exact java.util.HashMap<Long, Object> of a HashSet<Long> built by add() in arrival order (JDK 8+
 * HashMap.putVal / resize / treeifyBin / TreeNode.treeify / putTreeVal / balanceInsertion / rotateLeft /
 * rotateRight / moveRootToFront / split / untreeify, restated over index-linked nodes; pinned by the
 * independent object model tests/jdk_hashmap_ref.py and its paper answers):
 *  - a list bin that reaches 9 nodes calls treeifyBin: below capacity 64 that resizes the table instead
 *    (so the final capacity is not a function of the size alone);
 *  - a tree bin keeps its nodes in a red-black tree ordered by (hash as a SIGNED int, Long value) AND in
 *    its `next` list, which iteration follows: treeify keeps the list order but moves the root to the
 *    front; a later insert goes right after its tree parent, then the (new) root moves to the front;
 *  - resize splits every bin into lo / hi lists in list order; a tree half of <= 6 nodes becomes a list
 *    again, a larger one is re-treeified (unless the other half is empty).
 * Iteration walks bins 0..cap-1 and follows `next`. */
typedef struct {
  int64_t key;
  uint32_t hash;
  int32_t next, prev, parent, left, right;
  uint8_t red, tree;
} jnode;
typedef struct {
  jnode* nd;
  int32_t* tab;
  uint32_t cap, thr, size;
  int flags;   /* bit 0: a bin treeified; bit 1: a collision resize (treeifyBin below capacity 64) */
} jmap;

static uint32_t j_hash(int64_t x) {
  const uint32_t h = (uint32_t)((uint64_t)x ^ ((uint64_t)x >> 32));
  return h ^ (h >> 16);
}
/* putTreeVal / treeify comparison: Node.hash is a Java int, so `(ph = p.hash) > h` is a SIGNED compare (the
 * stored hash stays uint32_t for the bin masks; bit 31 of it is bit 31 xor bit 63 of the id) */
static int j_dir(const jnode* p, uint32_t h, int64_t k) {
  if ((int32_t)p->hash > (int32_t)h) return -1;
  if ((int32_t)p->hash < (int32_t)h) return 1;
  return k < p->key ? -1 : 1;   /* Long.compareTo; keys are distinct */
}
static int32_t j_rotl(jnode* n, int32_t root, int32_t p) {
  int32_t r, pp, rl;
  if (p >= 0 && (r = n[p].right) >= 0) {
    if ((rl = n[p].right = n[r].left) >= 0) n[rl].parent = p;
    if ((pp = n[r].parent = n[p].parent) < 0) { root = r; n[r].red = 0; }
    else if (n[pp].left == p) n[pp].left = r;
    else n[pp].right = r;
    n[r].left = p;
    n[p].parent = r;
  }
  return root;
}
static int32_t j_rotr(jnode* n, int32_t root, int32_t p) {
  int32_t l, pp, lr;
  if (p >= 0 && (l = n[p].left) >= 0) {
    if ((lr = n[p].left = n[l].right) >= 0) n[lr].parent = p;
    if ((pp = n[l].parent = n[p].parent) < 0) { root = l; n[l].red = 0; }
    else if (n[pp].right == p) n[pp].right = l;
    else n[pp].left = l;
    n[l].right = p;
    n[p].parent = l;
  }
  return root;
}
static int32_t j_balance(jnode* n, int32_t root, int32_t x) {
  n[x].red = 1;
  for (;;) {
    int32_t xp = n[x].parent, xpp, xppl, xppr;
    if (xp < 0) { n[x].red = 0; return x; }
    if (!n[xp].red || (xpp = n[xp].parent) < 0) return root;
    if (xp == (xppl = n[xpp].left)) {
      if ((xppr = n[xpp].right) >= 0 && n[xppr].red) {
        n[xppr].red = 0; n[xp].red = 0; n[xpp].red = 1; x = xpp;
      } else {
        if (x == n[xp].right) {
          root = j_rotl(n, root, x = xp);
          xpp = (xp = n[x].parent) < 0 ? -1 : n[xp].parent;
        }
        if (xp >= 0) {
          n[xp].red = 0;
          if (xpp >= 0) { n[xpp].red = 1; root = j_rotr(n, root, xpp); }
        }
      }
    } else {
      if (xppl >= 0 && n[xppl].red) {
        n[xppl].red = 0; n[xp].red = 0; n[xpp].red = 1; x = xpp;
      } else {
        if (x == n[xp].left) {
          root = j_rotr(n, root, x = xp);
          xpp = (xp = n[x].parent) < 0 ? -1 : n[xp].parent;
        }
        if (xp >= 0) {
          n[xp].red = 0;
          if (xpp >= 0) { n[xpp].red = 1; root = j_rotl(n, root, xpp); }
        }
      }
    }
  }
}
static void j_root_front(jmap* m, int32_t root) {
  jnode* n = m->nd;
  const uint32_t idx = n[root].hash & (m->cap - 1);
  const int32_t first = m->tab[idx];
  if (root != first) {
    m->tab[idx] = root;
    const int32_t rp = n[root].prev, rn = n[root].next;
    if (rn >= 0) n[rn].prev = rp;
    if (rp >= 0) n[rp].next = rn;
    if (first >= 0) n[first].prev = root;
    n[root].next = first;
    n[root].prev = -1;
  }
}
/* TreeNode.treeify from list head hd (nodes already tree-marked, prev/next linked) */
static void j_treeify(jmap* m, int32_t hd) {
  jnode* n = m->nd;
  int32_t root = -1;
  for (int32_t x = hd, nx; x >= 0; x = nx) {
    nx = n[x].next;
    n[x].left = n[x].right = -1;
    if (root < 0) { n[x].parent = -1; n[x].red = 0; root = x; continue; }
    for (int32_t p = root;;) {
      const int dir = j_dir(&n[p], n[x].hash, n[x].key);
      const int32_t xp = p;
      if ((p = dir <= 0 ? n[p].left : n[p].right) < 0) {
        n[x].parent = xp;
        if (dir <= 0) n[xp].left = x; else n[xp].right = x;
        root = j_balance(n, root, x);
        break;
      }
    }
  }
  j_root_front(m, root);
}
static void j_untreeify(jnode* n, int32_t hd) {
  for (int32_t x = hd; x >= 0; x = n[x].next) { n[x].tree = 0; n[x].left = n[x].right = n[x].parent = -1; }
}
static void j_resize(jmap* m);
static void j_split(jmap* m, int32_t* ntab, int32_t b, uint32_t index, uint32_t bit) {
  jnode* n = m->nd;
  int32_t loH = -1, loT = -1, hiH = -1, hiT = -1;
  uint32_t lc = 0, hc = 0;
  for (int32_t e = b, nx; e >= 0; e = nx) {
    nx = n[e].next;
    n[e].next = -1;
    if ((n[e].hash & bit) == 0) {
      if ((n[e].prev = loT) < 0) loH = e; else n[loT].next = e;
      loT = e; ++lc;
    } else {
      if ((n[e].prev = hiT) < 0) hiH = e; else n[hiT].next = e;
      hiT = e; ++hc;
    }
  }
  /* treeify / root_front index through the new table */
  int32_t* otab = m->tab; const uint32_t ocap = m->cap;
  m->tab = ntab; m->cap = ocap * 2;
  if (loH >= 0) {
    if (lc <= 6) { j_untreeify(n, loH); ntab[index] = loH; }
    else { ntab[index] = loH; if (hiH >= 0) j_treeify(m, loH); }
  }
  if (hiH >= 0) {
    if (hc <= 6) { j_untreeify(n, hiH); ntab[index + bit] = hiH; }
    else { ntab[index + bit] = hiH; if (loH >= 0) j_treeify(m, hiH); }
  }
  m->tab = otab; m->cap = ocap;
}
static void j_resize(jmap* m) {
  const uint32_t ocap = m->cap, ncap = ocap ? ocap * 2 : 16;
  int32_t* ntab = (int32_t*)malloc(ncap * sizeof(int32_t));
  for (uint32_t i = 0; i < ncap; ++i) ntab[i] = -1;
  jnode* n = m->nd;
  for (uint32_t j = 0; j < ocap; ++j) {
    const int32_t e = m->tab[j];
    if (e < 0) continue;
    if (n[e].next < 0) { ntab[n[e].hash & (ncap - 1)] = e; }
    else if (n[e].tree) { j_split(m, ntab, e, j, ocap); }
    else {
      int32_t loH = -1, loT = -1, hiH = -1, hiT = -1;
      for (int32_t x = e, nx; x >= 0; x = nx) {
        nx = n[x].next;
        if ((n[x].hash & ocap) == 0) { if (loT < 0) loH = x; else n[loT].next = x; loT = x; }
        else { if (hiT < 0) hiH = x; else n[hiT].next = x; hiT = x; }
      }
      if (loT >= 0) { n[loT].next = -1; ntab[j] = loH; }
      if (hiT >= 0) { n[hiT].next = -1; ntab[j + ocap] = hiH; }
    }
  }
  free(m->tab);
  m->tab = ntab;
  m->cap = ncap;
  m->thr = ncap / 4 * 3;
}
static void j_treeify_bin(jmap* m, uint32_t hash) {
  if (m->cap < 64) { m->flags |= 2; j_resize(m); return; }
  jnode* n = m->nd;
  const int32_t hd = m->tab[hash & (m->cap - 1)];
  int32_t tl = -1;
  for (int32_t e = hd; e >= 0; e = n[e].next) { n[e].tree = 1; n[e].prev = tl; tl = e; }
  m->flags |= 1;
  j_treeify(m, hd);
}
/* HashMap.putVal for a key not yet present (the caller feeds distinct keys in arrival order) */
static void j_put(jmap* m, int32_t x) {
  jnode* n = m->nd;
  if (!m->tab) j_resize(m);
  const uint32_t h = n[x].hash, i = h & (m->cap - 1);
  n[x].next = n[x].prev = n[x].parent = n[x].left = n[x].right = -1;
  n[x].red = 0; n[x].tree = 0;
  int32_t p = m->tab[i];
  if (p < 0) {
    m->tab[i] = x;
  } else if (n[p].tree) {   /* putTreeVal: p is the bin's root (moveRootToFront) */
    int32_t root = p;
    while (n[root].parent >= 0) root = n[root].parent;
    n[x].tree = 1;
    for (int32_t q = root;;) {
      const int dir = j_dir(&n[q], h, n[x].key);
      const int32_t xp = q;
      if ((q = dir <= 0 ? n[q].left : n[q].right) < 0) {
        const int32_t xpn = n[xp].next;
        n[x].next = xpn;
        if (dir <= 0) n[xp].left = x; else n[xp].right = x;
        n[xp].next = x;
        n[x].parent = n[x].prev = xp;
        if (xpn >= 0) n[xpn].prev = x;
        j_root_front(m, j_balance(n, root, x));
        break;
      }
    }
  } else {
    for (int bin = 0;; ++bin) {
      const int32_t e = n[p].next;
      if (e < 0) {
        n[p].next = x;
        if (bin >= 7) j_treeify_bin(m, h);
        break;
      }
      p = e;
    }
  }
  if (++m->size > m->thr) j_resize(m);
}

/* distinct[] in first-arrival order -> ids[] in HashSet iteration order; returns the flags above */
static int hashset_order(const int64_t* distinct, uint64_t k, int64_t* ids, hsent* tmp) {
  (void)tmp;
  jmap m = {0};
  m.nd = (jnode*)malloc((k + 1) * sizeof(jnode));
  for (uint64_t j = 0; j < k; ++j) {
    m.nd[j].key = distinct[j];
    m.nd[j].hash = j_hash(distinct[j]);
    j_put(&m, (int32_t)j);
  }
  uint64_t o = 0;
  for (uint32_t b = 0; b < m.cap; ++b)
    for (int32_t e = m.tab[b]; e >= 0; e = m.nd[e].next) ids[o++] = m.nd[e].key;
  free(m.tab);
  free(m.nd);
  return m.flags;
}

/* the plain-bin model (final capacity from the size alone, insertion order inside a bin) -- what the
 * GPU's sort-based order computes; tests compare it with the exact model */
GSO_API int gso_hashset_order(const int64_t* distinct, uint64_t k, int64_t* ids_exact, int64_t* ids_plain) {
  hsent* tmp = (hsent*)malloc((k + 1) * sizeof(hsent));
  const int flags = hashset_order(distinct, k, ids_exact, tmp);
  const uint64_t cap = gso_java_hashset_cap(k);
  for (uint64_t j = 0; j < k; ++j) {
    tmp[j].b = gso_java_long_bucket(distinct[j], cap);
    tmp[j].ord = (uint32_t)j;
    tmp[j].x = distinct[j];
  }
  qsort(tmp, k, sizeof(hsent), cmp_hs);
  for (uint64_t j = 0; j < k; ++j) ids_plain[j] = tmp[j].x;
  free(tmp);
  return flags;
}

/* per-vertex distinct neighbours (first arrival order) from the CSR */
typedef struct {
  uint64_t U, R;
  int64_t* keys; uint64_t* off; int64_t* nbr;
} csr_t;
static int build_csr_all(const int64_t* src, const int64_t* dst, uint64_t n, csr_t* c) {
  c->R = 2 * n;
  c->keys = (int64_t*)malloc((c->R + 1) * sizeof(int64_t));
  c->off = (uint64_t*)malloc((c->R + 2) * sizeof(uint64_t));
  c->nbr = (int64_t*)malloc((c->R + 1) * sizeof(int64_t));
  const int64_t u = gso_window_csr(src, dst, NULL, n, DT_NONE, DIR_ALL, c->keys, c->off, c->nbr, NULL,
                                   c->R + 1);
  c->U = (uint64_t)u;
  return u < 0 ? -1 : 0;
}
static void free_csr(csr_t* c) { free(c->keys); free(c->off); free(c->nbr); }

static uint64_t distinct_of(const int64_t* nb, uint64_t d, int64_t* out) {
  /* first-arrival distinct; d is small in the oracle's test sizes -> local map */
  vmap m;
  vmap_init(&m, d);
  uint64_t k = 0;
  for (uint64_t j = 0; j < d; ++j) {
    int is_new;
    vmap_get(&m, nb[j], &is_new);
    if (is_new) out[k++] = nb[j];
  }
  vmap_free(&m);
  return k;
}

/* applyOnNeighbors(GenerateCandidateEdges) over slice(ALL) — WindowTriangles.java:83-116.
 * Writes records in vertex-ascending order; returns the record count (or -1-needed when cap short).
 * *treeified = 1 if some neighbour set would use a tree bin (iteration order then unpinned). */
GSO_API int64_t gso_window_candidates(const int64_t* src, const int64_t* dst, uint64_t n, int64_t* a,
                                      int64_t* b, uint8_t* flag, uint64_t cap, int* treeified) {
  csr_t c;
  if (build_csr_all(src, dst, n, &c) != 0) return -2;
  int64_t* dist = (int64_t*)malloc((c.R + 1) * sizeof(int64_t));
  int64_t* ids = (int64_t*)malloc((c.R + 1) * sizeof(int64_t));
  hsent* tmp = (hsent*)malloc((c.R + 1) * sizeof(hsent));
  uint64_t o = 0;
  *treeified = 0;
  for (uint64_t u = 0; u < c.U; ++u) {
    const int64_t v = c.keys[u];
    const uint64_t lo = c.off[u], hi = c.off[u + 1];
    for (uint64_t j = lo; j < hi; ++j) {  /* (v, t, false) per neighbour record :96-100 */
      if (o < cap) { a[o] = v; b[o] = c.nbr[j]; flag[o] = 0; }
      ++o;
    }
    const uint64_t k = distinct_of(c.nbr + lo, hi - lo, dist);
    *treeified |= hashset_order(dist, k, ids, tmp);
    /* the ids above v, in HashSet order (kept in place in `ids`); the loops below emit the pairs
     * (i, j), i < len-1, j >= i, of those: C(m, 2) + m records, less the self pair of the last element
     * when it is above v */
    const int last_above = k > 0 && ids[k - 1] > v;   /* then it is also the last id above v */
    uint64_t m = 0;
    for (uint64_t i = 0; i < k; ++i)
      if (ids[i] > v) ids[m++] = ids[i];
    const uint64_t cnt = m * (m - 1) / 2 + m - (uint64_t)last_above;
    if (o + cnt > cap) {   /* a size query (or past capacity): the count only */
      o += cnt;
      continue;
    }
    for (uint64_t i = 0; i < m; ++i) {             /* i < len-1 :104 (the last element only as j) */
      if (last_above && i + 1 == m) break;
      for (uint64_t j = i; j < m; ++j) {          /* j = i (self pair) :105; both above v :108 */
        a[o] = ids[i]; b[o] = ids[j]; flag[o] = 1;
        ++o;
      }
    }
  }
  free(dist); free(ids); free(tmp); free_csr(&c);
  return o <= cap ? (int64_t)o : -1 - (int64_t)o;
}

/* GenerateCandidateEdges over `threads` threads with a consumer (bench.py's C5 cpu_baseline): the same
 * records as gso_window_candidates (WindowTriangles.java:91-114: the edge records, then the HashSet-ordered
 * pairs), each thread taking blocks of 64 vertices from a shared counter and writing its records into its
 * own chunk of `chunk` records (a, b, flag columns), which a consumer then reads back whole (column sums,
 * as the GPU line's device consumer does) before the chunk is reused.  The CSR is built first, on one
 * thread.  Returns the record count; sums[0..2] = the a, b and flag column sums (order-free, so they equal
 * the sums over gso_window_candidates' output). */
typedef struct {
  const csr_t* c;
  uint64_t chunk, maxd;
  volatile uint64_t* next;
  uint64_t recs, s[3];
} cand_mt_arg;
static void cand_consume(const int64_t* a, const int64_t* b, const uint8_t* f, uint64_t n, uint64_t* s) {
  uint64_t sa = 0, sb = 0, sf = 0;
  for (uint64_t i = 0; i < n; ++i) {
    sa += (uint64_t)a[i];
    sb += (uint64_t)b[i];
    sf += f[i];
  }
  s[0] += sa; s[1] += sb; s[2] += sf;
}
static void* cand_mt_worker(void* p) {
  cand_mt_arg* g = (cand_mt_arg*)p;
  const csr_t* c = g->c;
  const uint64_t C = g->chunk;
  int64_t* a = (int64_t*)malloc(C * sizeof(int64_t));
  int64_t* b = (int64_t*)malloc(C * sizeof(int64_t));
  uint8_t* f = (uint8_t*)malloc(C);
  int64_t* dist = (int64_t*)malloc((g->maxd + 1) * sizeof(int64_t));
  int64_t* ids = (int64_t*)malloc((g->maxd + 1) * sizeof(int64_t));
  hsent* tmp = (hsent*)malloc((g->maxd + 1) * sizeof(hsent));
  uint64_t o = 0;
#define CAND_PUT(x, y, fl) do { a[o] = (x); b[o] = (y); f[o] = (fl); if (++o == C) { cand_consume(a, b, f, o, g->s); g->recs += o; o = 0; } } while (0)
  for (;;) {
    const uint64_t u0 = __sync_fetch_and_add(g->next, 64);
    if (u0 >= c->U) break;
    const uint64_t u1 = u0 + 64 < c->U ? u0 + 64 : c->U;
    for (uint64_t u = u0; u < u1; ++u) {
      const int64_t v = c->keys[u];
      const uint64_t lo = c->off[u], hi = c->off[u + 1];
      for (uint64_t j = lo; j < hi; ++j) CAND_PUT(v, c->nbr[j], 0);
      const uint64_t k = distinct_of(c->nbr + lo, hi - lo, dist);
      hashset_order(dist, k, ids, tmp);
      const int last_above = k > 0 && ids[k - 1] > v;
      uint64_t m = 0;
      for (uint64_t i = 0; i < k; ++i)
        if (ids[i] > v) ids[m++] = ids[i];
      for (uint64_t i = 0; i < m; ++i) {
        if (last_above && i + 1 == m) break;
        for (uint64_t j = i; j < m; ++j) CAND_PUT(ids[i], ids[j], 1);
      }
    }
  }
#undef CAND_PUT
  cand_consume(a, b, f, o, g->s);
  g->recs += o;
  free(a); free(b); free(f); free(dist); free(ids); free(tmp);
  return NULL;
}
GSO_API int64_t gso_candidates_mt(const int64_t* src, const int64_t* dst, uint64_t n, int threads, uint64_t chunk,
                                  uint64_t* sums) {
  csr_t c;
  if (build_csr_all(src, dst, n, &c) != 0) return -2;
  uint64_t maxd = 1;
  for (uint64_t u = 0; u < c.U; ++u)
    if (c.off[u + 1] - c.off[u] > maxd) maxd = c.off[u + 1] - c.off[u];
  if (threads < 1) threads = 1;
  if (chunk < 1) chunk = 1;
  volatile uint64_t next = 0;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)threads);
  cand_mt_arg* args = (cand_mt_arg*)calloc((size_t)threads, sizeof(cand_mt_arg));
  for (int t = 0; t < threads; ++t) {
    args[t].c = &c;
    args[t].chunk = chunk;
    args[t].maxd = maxd;
    args[t].next = &next;
    pthread_create(&th[t], NULL, cand_mt_worker, &args[t]);
  }
  uint64_t recs = 0;
  sums[0] = sums[1] = sums[2] = 0;
  for (int t = 0; t < threads; ++t) {
    pthread_join(th[t], NULL);
    recs += args[t].recs;
    for (int q = 0; q < 3; ++q) sums[q] += args[t].s[q];
  }
  free(th); free(args); free_csr(&c);
  return (int64_t)recs;
}

/* ------------------------------------------------------------------------------------ */
/* WindowTriangles, reference rule: candidates -> keyBy(0,1) CountTriangles -> sum(0)    */
/* ------------------------------------------------------------------------------------ */
typedef struct { int64_t a, b; uint8_t f; } rec3;
static int cmp_rec(const void* x, const void* y) {
  const rec3* p = (const rec3*)x; const rec3* q = (const rec3*)y;
  if (p->a != q->a) return p->a < q->a ? -1 : 1;
  if (p->b != q->b) return p->b < q->b ? -1 : 1;
  return 0;
}
/* Returns the Integer the reference emits (WindowTriangles.java:126-137, :66) and *exact. */
GSO_API int32_t gso_window_triangles_ref(const int64_t* src, const int64_t* dst, uint64_t n,
                                         uint64_t* exact, int* has_output, int* treeified) {
  *exact = 0; *has_output = 0;
  if (n == 0) return 0;
  int64_t need = gso_window_candidates(src, dst, n, NULL, NULL, NULL, 0, treeified);
  const uint64_t P = (uint64_t)(-1 - need);
  int64_t* a = (int64_t*)malloc(P * sizeof(int64_t));
  int64_t* b = (int64_t*)malloc(P * sizeof(int64_t));
  uint8_t* f = (uint8_t*)malloc(P);
  gso_window_candidates(src, dst, n, a, b, f, P, treeified);
  rec3* r = (rec3*)malloc(P * sizeof(rec3));
  for (uint64_t i = 0; i < P; ++i) { r[i].a = a[i]; r[i].b = b[i]; r[i].f = f[i]; }
  qsort(r, P, sizeof(rec3), cmp_rec);
  uint32_t sum = 0;   /* Integer sum, wraps */
  uint64_t ex = 0;
  for (uint64_t i = 0; i < P;) {
    uint64_t j = i;
    uint32_t cand = 0, edges = 0;
    uint64_t cand64 = 0;
    while (j < P && r[j].a == r[i].a && r[j].b == r[i].b) {
      if (r[j].f) { cand++; cand64++; } else edges++;
      ++j;
    }
    if (edges > 0) { sum += cand; ex += cand64; *has_output = 1; }
    i = j;
  }
  free(a); free(b); free(f); free(r);
  *exact = ex;
  return (int32_t)sum;
}

/* ------------------------------------------------------------------------------------ */
/* WindowTriangles, forward algorithm (independent check; scales to millions of edges)   */
/* ------------------------------------------------------------------------------------ */
static int cmp_i64(const void* x, const void* y) {
  const int64_t p = *(const int64_t*)x, q = *(const int64_t*)y;
  return (p > q) - (p < q);
}
/* count = T (triangles of the simple undirected graph, each once) + S (self-pair quirk:
 * for each v, each distinct neighbour x > v that has a self-loop, except the last element
 * of v's HashSet order).  Same value as gso_window_triangles_ref. */
GSO_API int32_t gso_window_triangles_fwd(const int64_t* src, const int64_t* dst, uint64_t n,
                                         uint64_t* exact, int* has_output) {
  *exact = 0; *has_output = (n > 0);
  if (n == 0) return 0;
  csr_t c;
  if (build_csr_all(src, dst, n, &c) != 0) return 0;
  /* distinct neighbour lists (sorted), self-loop flags */
  uint64_t* doff = (uint64_t*)malloc((c.U + 1) * sizeof(uint64_t));
  int64_t* dn = (int64_t*)malloc((c.R + 1) * sizeof(int64_t));
  uint8_t* loop = (uint8_t*)calloc(c.U + 1, 1);
  int64_t* dist = (int64_t*)malloc((c.R + 1) * sizeof(int64_t));
  int64_t* ids = (int64_t*)malloc((c.R + 1) * sizeof(int64_t));
  hsent* tmp = (hsent*)malloc((c.R + 1) * sizeof(hsent));
  uint64_t S = 0, o = 0;
  for (uint64_t u = 0; u < c.U; ++u) {
    const int64_t v = c.keys[u];
    const uint64_t lo = c.off[u], hi = c.off[u + 1];
    const uint64_t k = distinct_of(c.nbr + lo, hi - lo, dist);
    doff[u] = o;
    for (uint64_t j = 0; j < k; ++j) {
      if (dist[j] == v) loop[u] = 1;
      else dn[o++] = dist[j];
    }
    qsort(dn + doff[u], o - doff[u], sizeof(int64_t), cmp_i64);
  }
  doff[c.U] = o;
  /* self-loop lookup by binary search over keys */
  for (uint64_t u = 0; u < c.U; ++u) {
    const int64_t v = c.keys[u];
    const uint64_t lo = c.off[u], hi = c.off[u + 1];
    const uint64_t k = distinct_of(c.nbr + lo, hi - lo, dist);
    if (k < 2) continue;
    hashset_order(dist, k, ids, tmp);
    for (uint64_t i = 0; i + 1 < k; ++i) {
      if (ids[i] <= v) continue;
      int64_t* pos = (int64_t*)bsearch(&ids[i], c.keys, c.U, sizeof(int64_t), cmp_i64);
      if (pos && loop[pos - c.keys]) S++;
    }
  }
  /* T: for each u, for neighbours v > u, count w > v in N(u) ∩ N(v) */
  uint64_t T = 0;
  for (uint64_t u = 0; u < c.U; ++u) {
    const int64_t uk = c.keys[u];
    for (uint64_t p = doff[u]; p < doff[u + 1]; ++p) {
      const int64_t vk = dn[p];
      if (vk <= uk) continue;
      int64_t* pos = (int64_t*)bsearch(&vk, c.keys, c.U, sizeof(int64_t), cmp_i64);
      const uint64_t v = (uint64_t)(pos - c.keys);
      uint64_t x = p + 1, y = doff[v];
      while (x < doff[u + 1] && y < doff[v + 1]) {
        if (dn[x] < dn[y]) ++x;
        else if (dn[x] > dn[y]) ++y;
        else { if (dn[x] > vk) T++; ++x; ++y; }
      }
    }
  }
  free(doff); free(dn); free(loop); free(dist); free(ids); free(tmp); free_csr(&c);
  *exact = T + S;
  return (int32_t)(uint32_t)(T + S);
}

/* ------------------------------------------------------------------------------------ */
/* CPU baseline: keyBy(vertex) over P threads + per-subtask hash-map fold (bench only)  */
/* ------------------------------------------------------------------------------------ */
typedef struct { int64_t key; uint64_t val; } shuffled;  /* a record on the wire after keyBy */
enum { BL_DEGMAX = 4 };   /* gso_baseline_reduce op: the degree / max-neighbour fold (val = neighbour) */
typedef struct {
  const int64_t* src; const int64_t* dst; const void* val;
  uint64_t n; int dtype, dir, op, P, tid;
  /* phase 1 output: per (producer, consumer) record buffers — the keyBy network channels */
  shuffled** part; uint64_t* part_n;   /* [P*P] */
  uint64_t vertices;
  pthread_barrier_t* bar;
} bl_arg;

static void* bl_worker(void* p) {
  bl_arg* A = (bl_arg*)p;
  const int P = A->P, t = A->tid;
  const uint64_t R = n_records(A->n, A->dir);
  const uint64_t lo = R * (uint64_t)t / (uint64_t)P, hi = R * (uint64_t)(t + 1) / (uint64_t)P;
  /* phase 1: this source subtask routes its records by hash(key) % P (the keyBy shuffle) */
  uint64_t* cnt = (uint64_t*)calloc((size_t)P, sizeof(uint64_t));
  for (uint64_t r = lo; r < hi; ++r) {
    int64_t key, nbr;
    record(A->src, A->dst, A->dir, r, &key, &nbr);
    cnt[mix64((uint64_t)key) % (uint64_t)P]++;
  }
  for (int q = 0; q < P; ++q) {
    A->part[t * P + q] = (shuffled*)malloc((cnt[q] ? cnt[q] : 1) * sizeof(shuffled));
    A->part_n[t * P + q] = 0;
  }
  for (uint64_t r = lo; r < hi; ++r) {
    int64_t key, nbr;
    const uint64_t i = record(A->src, A->dst, A->dir, r, &key, &nbr);
    const int q = (int)(mix64((uint64_t)key) % (uint64_t)P);
    shuffled* o = &A->part[t * P + q][A->part_n[t * P + q]++];
    o->key = key;
    o->val = A->op == OP_COUNT ? 0 : A->op == BL_DEGMAX ? (uint64_t)nbr : load_val(A->dtype, A->val, i);
  }
  free(cnt);
  pthread_barrier_wait(A->bar);
  /* phase 2: window operator subtask t folds its keys in arrival order into one open-addressing
   * table of {key, acc} slots (one cache line touch per record) */
  uint64_t mine = 0;
  for (int q = 0; q < P; ++q) mine += A->part_n[q * P + t];
  uint64_t cap = 16;
  while (cap < 2 * (mine / 2 + 16)) cap <<= 1;
  typedef struct { int64_t key; uint64_t acc; int64_t acc2; } slot_t;
  slot_t* tab = (slot_t*)malloc(cap * sizeof(slot_t));
  uint8_t* used = (uint8_t*)calloc(cap, 1);
  uint64_t size = 0;
  for (int q = 0; q < P; ++q) {
    const shuffled* lst = A->part[q * P + t];
    for (uint64_t j = 0; j < A->part_n[q * P + t]; ++j) {
      uint64_t h = mix64((uint64_t)lst[j].key) & (cap - 1);
      while (used[h] && tab[h].key != lst[j].key) h = (h + 1) & (cap - 1);
      if (!used[h]) {
        used[h] = 1;
        tab[h].key = lst[j].key;
        tab[h].acc = (A->op == OP_COUNT || A->op == BL_DEGMAX) ? 1 : lst[j].val;
        tab[h].acc2 = (int64_t)lst[j].val;
        ++size;
      } else if (A->op == OP_COUNT) {
        tab[h].acc++;
      } else if (A->op == BL_DEGMAX) {   /* foldNeighbors(degree, max neighbour) */
        tab[h].acc++;
        if ((int64_t)lst[j].val > tab[h].acc2) tab[h].acc2 = (int64_t)lst[j].val;
      } else {
        apply_op(A->op, A->dtype, &tab[h].acc, &lst[j].val, 0);
      }
    }
  }
  A->vertices = size;
  free(tab);
  free(used);
  return NULL;
}

/* Returns the number of output vertices (sum over subtasks). */
GSO_API uint64_t gso_baseline_reduce(const int64_t* src, const int64_t* dst, const void* val, uint64_t n,
                                     int dtype, int dir, int op, int threads) {
  const int P = threads < 1 ? 1 : threads;
  pthread_t* th = (pthread_t*)malloc((size_t)P * sizeof(pthread_t));
  bl_arg* args = (bl_arg*)malloc((size_t)P * sizeof(bl_arg));
  shuffled** part = (shuffled**)malloc((size_t)P * P * sizeof(shuffled*));
  uint64_t* part_n = (uint64_t*)calloc((size_t)P * P, sizeof(uint64_t));
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, NULL, (unsigned)P);
  for (int t = 0; t < P; ++t) {
    args[t] = (bl_arg){src, dst, val, n, dtype, dir, op, P, t, part, part_n, 0, &bar};
    pthread_create(&th[t], NULL, bl_worker, &args[t]);
  }
  uint64_t U = 0;
  for (int t = 0; t < P; ++t) { pthread_join(th[t], NULL); U += args[t].vertices; }
  pthread_barrier_destroy(&bar);
  for (int i = 0; i < P * P; ++i) free(part[i]);
  free(part); free(part_n); free(args); free(th);
  return U;
}

/* ------------------------------------------------------------------------------------ */
/* edge text input: example/WindowTriangles.java:175-185 (also ConnectedComponentsExample */
/* .java:113-115): env.readTextFile(path) -> s.split("\\s") -> Long.parseLong(fields[0..2]) */
/* ------------------------------------------------------------------------------------ */
/* Flink 1.0.3 TextInputFormat: records are split at '\n'; a trailing '\r' is dropped from a
 * record; the text after the last '\n' is a record only if it is non-empty.
 * String.split("\\s") splits at every single whitespace char [ \t\n\x0B\f\r] and drops trailing
 * empty strings, so field k (k < 3) is the run of non-whitespace chars that starts one separator
 * after field k-1; an empty field (two separators in a row, leading whitespace, fewer than three
 * fields) makes Long.parseLong throw, as does a sign without digits, any other char, or a value
 * outside [-2^63, 2^63).  Fields after the third are ignored. */
static int gso_is_ws(unsigned char ch) {
  return ch == ' ' || ch == '\t' || ch == '\n' || ch == 0x0B || ch == '\f' || ch == '\r';
}

/* Long.parseLong(s[p..q)) -> 0 ok */
static int gso_parse_long(const unsigned char* s, uint64_t p, uint64_t q, int64_t* out) {
  if (p >= q) return -1;
  int neg = 0;
  if (s[p] == '-' || s[p] == '+') {
    neg = s[p] == '-';
    ++p;
    if (p >= q) return -1;
  }
  const uint64_t lim = neg ? (1ull << 63) : (1ull << 63) - 1;
  uint64_t v = 0;
  for (; p < q; ++p) {
    const unsigned d = (unsigned)s[p] - '0';
    if (d > 9) return -1;
    if (v > (lim - d) / 10) return -1;
    v = v * 10 + d;
  }
  *out = neg ? (int64_t)(0 - v) : (int64_t)v;
  return 0;
}

/* Parse one record s[p..q) (no '\n'); returns 0 ok. */
static int gso_parse_record(const unsigned char* s, uint64_t p, uint64_t q, int64_t f[3]) {
  if (q > p && s[q - 1] == '\r') --q;
  uint64_t at = p;
  for (int k = 0; k < 3; ++k) {
    uint64_t e = at;
    while (e < q && !gso_is_ws(s[e])) ++e;
    if (gso_parse_long(s, at, e, &f[k])) return -1;
    at = e + 1;
  }
  return 0;
}

/* returns the record count (>= 0), or -(1 + index of the first malformed record); outputs are
 * written while the count fits cap */
GSO_API int64_t gso_parse_edges_text(const char* text, uint64_t bytes, int64_t* src, int64_t* dst, int64_t* ts,
                                     uint64_t cap) {
  const unsigned char* s = (const unsigned char*)text;
  uint64_t p = 0, n = 0;
  while (p < bytes) {
    const unsigned char* nl = memchr(s + p, '\n', bytes - p);
    const uint64_t q = nl ? (uint64_t)(nl - s) : bytes;
    int64_t f[3];
    if (gso_parse_record(s, p, q, f)) return -1 - (int64_t)n;
    if (n < cap) {
      src[n] = f[0];
      dst[n] = f[1];
      ts[n] = f[2];
    }
    ++n;
    p = q + 1;
  }
  return (int64_t)n;
}

/* ------------------------------------------------------------------------------------ */
/* Zipf(s) source stream ("a Zipf(s=1.1) source stream over 2^24 IDs"): */
/* src = k with probability (k+1)^-s / H(V, s), hubs at the lowest IDs; dst uniform.      */
/* Inverse CDF over a 53-bit fixed-point table; the table is a sequential double sum of   */
/* pow() terms, so gs_generate_zipf (library host code, same arithmetic) is bit-identical. */
/* ------------------------------------------------------------------------------------ */
GSO_API void gso_zipf_cdf(uint64_t V, double s, uint64_t* cdf) {
  double cum = 0.0;
  for (uint64_t k = 0; k < V; ++k) cum += pow((double)(k + 1), -s);
  const double total = cum;
  cum = 0.0;
  for (uint64_t k = 0; k < V; ++k) {
    cum += pow((double)(k + 1), -s);
    cdf[k] = (uint64_t)((cum / total) * 9007199254740992.0);
  }
  cdf[V - 1] = 1ull << 53;
}

GSO_API int gso_gen_zipf(uint64_t V, double s, uint64_t n, uint64_t seed, uint64_t first_edge, int64_t* src,
                         int64_t* dst) {
  uint64_t* cdf = (uint64_t*)malloc(V * sizeof(uint64_t));
  if (!cdf) return -1;
  gso_zipf_cdf(V, s, cdf);
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = first_edge + k;
    const uint64_t u = gso_splitmix64(seed ^ 0x21F0A5EDull, i) >> 11;
    uint64_t lo = 0, hi = V - 1;   /* smallest j with cdf[j] > u */
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (cdf[mid] > u) hi = mid;
      else lo = mid + 1;
    }
    src[k] = (int64_t)lo;
    dst[k] = (int64_t)(gso_splitmix64(seed ^ 0xD5D5D5D5ull, i) % V);
  }
  free(cdf);
  return 0;
}

/* ------------------------------------------------------------------------------------ */
/* Large-window restatement of the folds (config-size parity).    */
/* The same left fold as window_fold / gso_window_fold_degree_max, spread over P threads  */
/* the way keyBy spreads a window over Flink subtasks (SimpleEdgeStream.java:159-167):    */
/* producer p routes its contiguous record range by hash(key) % P; consumer q folds the   */
/* records of producers 0..P-1 in that order, so every key still sees its records in      */
/* arrival order (float sums identical to the sequential fold).  Outputs ascend by key.   */
/* ------------------------------------------------------------------------------------ */
enum { MT_REDUCE = 0, MT_FOLD = 1, MT_DEGMAX = 2 };
typedef struct {
  const int64_t* src; const int64_t* dst; const void* val;
  uint64_t n; int dtype, dir, op, mode, P, tid;
  uint64_t init_bits; int64_t init_max;
  uint32_t** part; uint64_t* part_n;   /* [P*P] record indices routed producer -> consumer */
  int64_t* keys; uint64_t* a; int64_t* b; uint64_t U;   /* consumer output, ascending keys */
  int err;
  pthread_barrier_t* bar;
} mt_arg;

static void* mt_worker(void* p) {
  mt_arg* A = (mt_arg*)p;
  const int P = A->P, t = A->tid;
  const uint64_t R = n_records(A->n, A->dir);
  const uint64_t lo = R * (uint64_t)t / (uint64_t)P, hi = R * (uint64_t)(t + 1) / (uint64_t)P;
  uint64_t* cnt = (uint64_t*)calloc((size_t)P, sizeof(uint64_t));
  for (uint64_t r = lo; r < hi; ++r) {
    int64_t key, nbr;
    record(A->src, A->dst, A->dir, r, &key, &nbr);
    cnt[mix64((uint64_t)key) % (uint64_t)P]++;
  }
  for (int q = 0; q < P; ++q) {
    A->part[t * P + q] = (uint32_t*)malloc((cnt[q] ? cnt[q] : 1) * sizeof(uint32_t));
    A->part_n[t * P + q] = 0;
  }
  for (uint64_t r = lo; r < hi; ++r) {
    int64_t key, nbr;
    record(A->src, A->dst, A->dir, r, &key, &nbr);
    const int q = (int)(mix64((uint64_t)key) % (uint64_t)P);
    A->part[t * P + q][A->part_n[t * P + q]++] = (uint32_t)r;
  }
  free(cnt);
  pthread_barrier_wait(A->bar);
  uint64_t mine = 0;
  for (int q = 0; q < P; ++q) mine += A->part_n[q * P + t];
  vmap m;
  if (vmap_init(&m, mine + 1) != 0) { A->err = 1; return NULL; }
  uint64_t* acc = (uint64_t*)malloc((mine + 1) * sizeof(uint64_t));
  int64_t* acc2 = A->mode == MT_DEGMAX ? (int64_t*)malloc((mine + 1) * sizeof(int64_t)) : NULL;
  for (int q = 0; q < P; ++q) {          /* producers in order: arrival order per key */
    const uint32_t* lst = A->part[q * P + t];
    for (uint64_t j = 0; j < A->part_n[q * P + t]; ++j) {
      int64_t key, nbr;
      const uint64_t i = record(A->src, A->dst, A->dir, lst[j], &key, &nbr);
      int is_new;
      const int64_t s = vmap_get(&m, key, &is_new);
      if (A->mode == MT_DEGMAX) {
        if (is_new) { acc[s] = 0; acc2[s] = A->init_max; }
        acc[s] += 1;
        if (nbr > acc2[s]) acc2[s] = nbr;
      } else if (A->op == OP_COUNT) {
        if (is_new) acc[s] = A->mode == MT_FOLD ? A->init_bits : 0;
        acc[s] += 1;
      } else if (is_new && A->mode == MT_REDUCE) {
        acc[s] = load_val(A->dtype, A->val, i);
      } else {
        if (is_new) acc[s] = A->init_bits;
        apply_op(A->op, A->dtype, &acc[s], A->val, i);
      }
    }
  }
  kv* srt = sorted_slots(&m);
  A->U = m.size;
  A->keys = (int64_t*)malloc((m.size + 1) * sizeof(int64_t));
  A->a = (uint64_t*)malloc((m.size + 1) * sizeof(uint64_t));
  A->b = acc2 ? (int64_t*)malloc((m.size + 1) * sizeof(int64_t)) : NULL;
  for (uint64_t j = 0; j < m.size; ++j) {
    A->keys[j] = srt[j].k;
    A->a[j] = acc[srt[j].s];
    if (acc2) A->b[j] = acc2[srt[j].s];
  }
  free(srt); free(acc); free(acc2); vmap_free(&m);
  return NULL;
}

/* mode MT_REDUCE (reduceOnEdges), MT_FOLD (foldNeighbors from *init), MT_DEGMAX (degree / max
 * neighbour from init_max; out_b = maxima).  Returns U, -1 - U when cap is short, -2 on failure. */
GSO_API int64_t gso_window_fold_mt(const int64_t* src, const int64_t* dst, const void* val, uint64_t n, int dtype,
                                   int dir, int op, int mode, const void* init, int64_t init_max, int threads,
                                   int64_t* out_keys, void* out_a, int64_t* out_b, uint64_t cap) {
  const int P = threads < 1 ? 1 : threads;
  uint64_t init_bits = 0;
  if (mode == MT_FOLD) init_bits = (op == OP_COUNT) ? (uint64_t)*(const int64_t*)init : load_val(dtype, init, 0);
  pthread_t* th = (pthread_t*)malloc((size_t)P * sizeof(pthread_t));
  mt_arg* args = (mt_arg*)calloc((size_t)P, sizeof(mt_arg));
  uint32_t** part = (uint32_t**)calloc((size_t)P * P, sizeof(uint32_t*));
  uint64_t* part_n = (uint64_t*)calloc((size_t)P * P, sizeof(uint64_t));
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, NULL, (unsigned)P);
  for (int t = 0; t < P; ++t) {
    args[t] = (mt_arg){src, dst, val, n, dtype, dir, op, mode, P, t, init_bits, init_max, part, part_n,
                       NULL, NULL, NULL, 0, 0, &bar};
    pthread_create(&th[t], NULL, mt_worker, &args[t]);
  }
  uint64_t U = 0;
  int err = 0;
  for (int t = 0; t < P; ++t) { pthread_join(th[t], NULL); U += args[t].U; err |= args[t].err; }
  pthread_barrier_destroy(&bar);
  for (int i = 0; i < P * P; ++i) free(part[i]);
  int64_t ret = err ? -2 : (U <= cap ? (int64_t)U : -1 - (int64_t)U);
  if (!err && U <= cap) {   /* P-way merge of the consumers' ascending outputs */
    uint64_t* at = (uint64_t*)calloc((size_t)P, sizeof(uint64_t));
    const int odt = (mode == MT_DEGMAX || op == OP_COUNT) ? DT_I64 : dtype;
    for (uint64_t o = 0; o < U; ++o) {
      int best = -1;
      for (int t = 0; t < P; ++t)
        if (at[t] < args[t].U && (best < 0 || args[t].keys[at[t]] < args[best].keys[at[best]])) best = t;
      const uint64_t j = at[best]++;
      out_keys[o] = args[best].keys[j];
      store_val(odt, out_a, o, args[best].a[j]);
      if (mode == MT_DEGMAX) out_b[o] = args[best].b[j];
    }
    free(at);
  }
  for (int t = 0; t < P; ++t) { free(args[t].keys); free(args[t].a); free(args[t].b); }
  free(part); free(part_n); free(args); free(th);
  return ret;
}

/* ------------------------------------------------------------------------------------ */
/* Forward-algorithm triangle count, multi-threaded: an independent check of the engine's  */
/* count at R-MAT scale 20-22 (the reference's candidate rule cannot run there).  Counts  */
/* T, the triangles of the window's simple undirected graph (multi-edges deduplicated as  */
/* the HashSet of WindowTriangles.java:101 does).  Self-loop-free windows only: returns -1 */
/* when the window has a self-loop (its self-pair term: gso_window_triangles_fwd).         */
/* IDs are arbitrary Longs (compacted by sort + unique).                                  */
/* ------------------------------------------------------------------------------------ */
static void radix_u64(uint64_t* a, uint64_t* tmp, uint64_t n, int bits) {
  /* LSD radix sort of the low `bits` bits, 16-bit digits */
  uint64_t* cnt = (uint64_t*)malloc(65536 * sizeof(uint64_t));
  for (int sh = 0; sh < bits; sh += 16) {
    memset(cnt, 0, 65536 * sizeof(uint64_t));
    for (uint64_t i = 0; i < n; ++i) cnt[(a[i] >> sh) & 0xFFFF]++;
    uint64_t run = 0;
    for (int d = 0; d < 65536; ++d) { const uint64_t c = cnt[d]; cnt[d] = run; run += c; }
    for (uint64_t i = 0; i < n; ++i) tmp[cnt[(a[i] >> sh) & 0xFFFF]++] = a[i];
    uint64_t* x = a; a = tmp; tmp = x;
    if (((bits + 15) / 16) % 2 == 1 && sh + 16 >= bits) memcpy(tmp, a, n * sizeof(uint64_t));
  }
  free(cnt);
}

typedef struct {
  const int64_t* ids; uint64_t V;        /* sorted distinct IDs (compaction) */
  const int64_t* in; uint32_t* out; uint64_t lo, hi;
  const uint64_t* off; const uint32_t* nbr; /* oriented out-lists */
  volatile uint64_t* next; uint64_t T;
} tri_arg;

static void* tri_map_worker(void* p) {   /* endpoint -> compact ID by binary search */
  tri_arg* A = (tri_arg*)p;
  for (uint64_t i = A->lo; i < A->hi; ++i) {
    uint64_t lo = 0, hi = A->V - 1;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A->ids[mid] < A->in[i]) lo = mid + 1;
      else hi = mid;
    }
    A->out[i] = (uint32_t)lo;
  }
  return NULL;
}

/* Parallel phases of the forward count (test infrastructure: makes the config-size triangle parity
 * tests (R-MAT s24 / s26, 2^28 / 2^30 edges) run in a minute or so).  Every phase is a plain loop
 * split over threads; shared counters use relaxed atomics. */
typedef struct tf_ctx {
  const int64_t *src, *dst; uint64_t n;
  int64_t kmin; uint64_t range;            /* direct compaction: ids in [kmin, kmin + range) */
  uint32_t* map;                           /* id - kmin -> compact id + 1 (0: absent) */
  uint32_t *cs, *cd; uint64_t V;
  uint64_t *off, *cur;                     /* CSR by the smaller endpoint, then by orientation */
  uint32_t *lst, *ucnt, *deg, *rank, *nbr;
  uint64_t* uoff; uint32_t* ulst;          /* distinct undirected edges (a < b), by a */
  uint64_t *ioff, *ipos; uint32_t* iown;   /* in-lists: for y, the out-list positions p of x -> y, and x */
  volatile uint64_t next; int P; int bad;
  uint64_t split[65];
  int64_t mn[64], mx[64]; uint64_t T[64];
} tf_ctx;
typedef struct { tf_ctx* c; int t; void (*fn)(tf_ctx*, int); } tf_job;
static void* tf_tramp(void* p) { tf_job* j = (tf_job*)p; j->fn(j->c, j->t); return NULL; }
static void tf_par(tf_ctx* c, void (*fn)(tf_ctx*, int)) {
  pthread_t th[64]; tf_job jb[64];
  for (int t = 0; t < c->P; ++t) { jb[t] = (tf_job){c, t, fn}; pthread_create(&th[t], NULL, tf_tramp, &jb[t]); }
  for (int t = 0; t < c->P; ++t) pthread_join(th[t], NULL);
}
#define TF_LO(c, t, N) ((N) * (uint64_t)(t) / (uint64_t)(c)->P)
#define TF_HI(c, t, N) ((N) * (uint64_t)((t) + 1) / (uint64_t)(c)->P)
static void tf_minmax(tf_ctx* c, int t) {
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (uint64_t i = TF_LO(c, t, c->n); i < TF_HI(c, t, c->n); ++i) {
    const int64_t a = c->src[i], b = c->dst[i];
    if (a == b) c->bad = 1;
    lo = a < lo ? a : lo; lo = b < lo ? b : lo;
    hi = a > hi ? a : hi; hi = b > hi ? b : hi;
  }
  c->mn[t] = lo; c->mx[t] = hi;
}
static void tf_mark(tf_ctx* c, int t) {
  for (uint64_t i = TF_LO(c, t, c->n); i < TF_HI(c, t, c->n); ++i) {
    c->map[(uint64_t)c->src[i] - (uint64_t)c->kmin] = 1;
    c->map[(uint64_t)c->dst[i] - (uint64_t)c->kmin] = 1;
  }
}
static void tf_remap(tf_ctx* c, int t) {
  for (uint64_t i = TF_LO(c, t, c->n); i < TF_HI(c, t, c->n); ++i) {
    c->cs[i] = c->map[(uint64_t)c->src[i] - (uint64_t)c->kmin] - 1;
    c->cd[i] = c->map[(uint64_t)c->dst[i] - (uint64_t)c->kmin] - 1;
  }
}
static void tf_count_lo(tf_ctx* c, int t) {   /* records per smaller endpoint */
  for (uint64_t i = TF_LO(c, t, c->n); i < TF_HI(c, t, c->n); ++i) {
    const uint32_t a = c->cs[i] < c->cd[i] ? c->cs[i] : c->cd[i];
    __atomic_fetch_add(&c->off[a + 1], 1, __ATOMIC_RELAXED);
  }
}
/* fills without atomics: thread t owns the keys [split[t], split[t+1]) (equal shares of the entries, by
 * the offsets) and scans every record for its own -- an atomic cursor per key serialised the threads on
 * the R-MAT hubs */
static void tf_split(tf_ctx* c, const uint64_t* off, uint64_t V) {
  uint64_t k = 0;
  for (int t = 0; t <= c->P; ++t) {
    const uint64_t want = off[V] * (uint64_t)t / (uint64_t)c->P;
    while (k < V && off[k] < want) ++k;
    c->split[t] = t == c->P ? V : k;
  }
}
static void tf_fill_lo(tf_ctx* c, int t) {
  const uint32_t k0 = (uint32_t)c->split[t], k1 = (uint32_t)c->split[t + 1];
  for (uint64_t i = 0; i < c->n; ++i) {
    const uint32_t a = c->cs[i] < c->cd[i] ? c->cs[i] : c->cd[i];
    if (a - k0 < k1 - k0) c->lst[c->cur[a]++] = c->cs[i] ^ c->cd[i] ^ a;
  }
}
static int tf_cmp_u32(const void* x, const void* y) {
  const uint32_t a = *(const uint32_t*)x, b = *(const uint32_t*)y;
  return a < b ? -1 : a > b;
}
static void tf_sort_unique(tf_ctx* c, int t) {   /* each vertex's partners above it: sorted, distinct */
  for (;;) {
    const uint64_t x0 = __sync_fetch_and_add(&c->next, 1024);
    if (x0 >= c->V) break;
    const uint64_t x1 = x0 + 1024 < c->V ? x0 + 1024 : c->V;
    for (uint64_t a = x0; a < x1; ++a) {
      uint32_t* L = c->lst + c->off[a];
      const uint64_t k = c->off[a + 1] - c->off[a];
      if (k > 1) qsort(L, k, 4, tf_cmp_u32);
      uint64_t u = 0;
      for (uint64_t i = 0; i < k; ++i)
        if (i == 0 || L[i] != L[i - 1]) L[u++] = L[i];
      c->ucnt[a] = (uint32_t)u;
    }
  }
}
static void tf_degrees(tf_ctx* c, int t) {
  for (uint64_t a = TF_LO(c, t, c->V); a < TF_HI(c, t, c->V); ++a) {
    const uint32_t* L = c->lst + c->off[a];
    __atomic_fetch_add(&c->deg[a], c->ucnt[a], __ATOMIC_RELAXED);
    for (uint32_t i = 0; i < c->ucnt[a]; ++i) __atomic_fetch_add(&c->deg[L[i]], 1, __ATOMIC_RELAXED);
  }
}
/* orientation x -> y iff (deg x, x) < (deg y, y), i.e. rank x < rank y; out-lists are stored over the
 * ranks, so hot (high-degree) vertices share the top of the id space and stay in cache.  The partner
 * lists are rewritten to ranks in place first (one random read each), then counted and filled */
static void tf_rank_lists(tf_ctx* c, int t) {
  for (uint64_t a = TF_LO(c, t, c->V); a < TF_HI(c, t, c->V); ++a) {
    uint32_t* L = c->lst + c->off[a];
    for (uint32_t i = 0; i < c->ucnt[a]; ++i) L[i] = c->rank[L[i]];
  }
}
static void tf_count_out(tf_ctx* c, int t) {
  for (uint64_t a = TF_LO(c, t, c->V); a < TF_HI(c, t, c->V); ++a) {
    const uint32_t* L = c->lst + c->off[a];
    const uint32_t ra = c->rank[a];
    for (uint32_t i = 0; i < c->ucnt[a]; ++i) {
      const uint32_t x = ra < L[i] ? ra : L[i];
      __atomic_fetch_add(&c->uoff[x + 1], 1, __ATOMIC_RELAXED);
    }
  }
}
static void tf_fill_out(tf_ctx* c, int t) {
  const uint32_t k0 = (uint32_t)c->split[t], k1 = (uint32_t)c->split[t + 1];
  for (uint64_t a = 0; a < c->V; ++a) {
    const uint32_t* L = c->lst + c->off[a];
    const uint32_t ra = c->rank[a];
    for (uint32_t i = 0; i < c->ucnt[a]; ++i) {
      const uint32_t rb = L[i], x = ra < rb ? ra : rb;
      if (x - k0 < k1 - k0) c->nbr[c->cur[x]++] = ra ^ rb ^ x;
    }
  }
}
static void tf_sort_out(tf_ctx* c, int t) {
  for (;;) {
    const uint64_t x0 = __sync_fetch_and_add(&c->next, 1024);
    if (x0 >= c->V) break;
    const uint64_t x1 = x0 + 1024 < c->V ? x0 + 1024 : c->V;
    for (uint64_t x = x0; x < x1; ++x) {
      const uint64_t k = c->uoff[x + 1] - c->uoff[x];
      if (k > 1) qsort(c->nbr + c->uoff[x], k, 4, tf_cmp_u32);
    }
  }
}
/* in-lists: every out-list entry p of x (x -> y) is listed under y with its owner x */
static void tf_count_in(tf_ctx* c, int t) {
  for (uint64_t p = TF_LO(c, t, c->uoff[c->V]); p < TF_HI(c, t, c->uoff[c->V]); ++p)
    __atomic_fetch_add(&c->ioff[c->nbr[p] + 1], 1, __ATOMIC_RELAXED);
}
static void tf_fill_in(tf_ctx* c, int t) {
  const uint32_t k0 = (uint32_t)c->split[t], k1 = (uint32_t)c->split[t + 1];
  for (uint64_t x = 0; x < c->V; ++x)
    for (uint64_t p = c->uoff[x]; p < c->uoff[x + 1]; ++p) {
      const uint32_t y = c->nbr[p];
      if (y - k0 >= k1 - k0) continue;
      const uint64_t q = c->cur[y]++;
      c->ipos[q] = p;
      c->iown[q] = (uint32_t)x;
    }
}
/* T = sum over y, over in-neighbours x of y (x -> y), of |{w in N+(x) after y} ∩ N+(y)|: a triangle
 * x -> y -> w (ranks x < y < w) is counted once, at its middle vertex y.  N+(y) is marked in a per-thread
 * bitmap over the ranks (V bits: 8 MB at scale 26), each w of N+(x) past y (the out-list is sorted, so
 * that is the suffix after position p) tested against it, the marks cleared again.  The suffix makes
 * this ~4x fewer probes than testing all of N+(y) for every x -> y (R-MAT s22: 7.2 G vs 28.7 G). */
static void tf_intersect(tf_ctx* c, int t) {
  uint64_t* bits = (uint64_t*)calloc((c->V >> 6) + 1, sizeof(uint64_t));
  uint64_t T = 0;
  for (;;) {
    const uint64_t y0 = __sync_fetch_and_add(&c->next, 256);
    if (y0 >= c->V) break;
    const uint64_t y1 = y0 + 256 < c->V ? y0 + 256 : c->V;
    for (uint64_t y = y0; y < y1; ++y) {
      const uint64_t b = c->uoff[y], e = c->uoff[y + 1];
      if (e == b || c->ioff[y + 1] == c->ioff[y]) continue;
      for (uint64_t p = b; p < e; ++p) bits[c->nbr[p] >> 6] |= 1ull << (c->nbr[p] & 63);
      for (uint64_t i = c->ioff[y]; i < c->ioff[y + 1]; ++i) {
        const uint32_t x = c->iown[i];
        const uint32_t* L = c->nbr;
        for (uint64_t q = c->ipos[i] + 1; q < c->uoff[x + 1]; ++q) T += (bits[L[q] >> 6] >> (L[q] & 63)) & 1;
      }
      for (uint64_t p = b; p < e; ++p) bits[c->nbr[p] >> 6] = 0;
    }
  }
  c->T[t] = T;
  free(bits);
}

GSO_API int gso_triangles_fwd_mt(const int64_t* src, const int64_t* dst, uint64_t n, int threads, uint64_t* T_out) {
  *T_out = 0;
  if (n == 0) return 0;
  tf_ctx* c = (tf_ctx*)calloc(1, sizeof(tf_ctx));
  c->src = src; c->dst = dst; c->n = n;
  c->P = threads < 1 ? 1 : threads > 64 ? 64 : threads;
  tf_par(c, tf_minmax);
  if (c->bad) { free(c); return -1; }
  int64_t kmin = INT64_MAX, kmax = INT64_MIN;
  for (int t = 0; t < c->P; ++t) { kmin = c->mn[t] < kmin ? c->mn[t] : kmin; kmax = c->mx[t] > kmax ? c->mx[t] : kmax; }
  c->cs = (uint32_t*)malloc(n * sizeof(uint32_t));
  c->cd = (uint32_t*)malloc(n * sizeof(uint32_t));
  /* 1. compact IDs, ascending in id order: a direct map when the id span is small, else sort + unique */
  const uint64_t span = (uint64_t)kmax - (uint64_t)kmin + 1;
  if (span != 0 && span < (1ull << 32) && span <= 8 * n + (1u << 20)) {
    c->kmin = kmin; c->range = span;
    c->map = (uint32_t*)calloc(span, sizeof(uint32_t));
    tf_par(c, tf_mark);
    uint32_t V = 0;
    for (uint64_t i = 0; i < span; ++i) if (c->map[i]) c->map[i] = ++V;
    c->V = V;
    tf_par(c, tf_remap);
    free(c->map);
  } else {
    uint64_t* e = (uint64_t*)malloc(2 * n * sizeof(uint64_t));
    uint64_t* tmp = (uint64_t*)malloc(2 * n * sizeof(uint64_t));
    for (uint64_t i = 0; i < n; ++i) {
      e[2 * i] = (uint64_t)src[i] ^ (1ull << 63);
      e[2 * i + 1] = (uint64_t)dst[i] ^ (1ull << 63);
    }
    radix_u64(e, tmp, 2 * n, 64);
    uint64_t V = 0;
    for (uint64_t i = 0; i < 2 * n; ++i)
      if (i == 0 || e[i] != e[i - 1]) e[V++] = e[i];
    int64_t* ids = (int64_t*)malloc(V * sizeof(int64_t));
    for (uint64_t i = 0; i < V; ++i) ids[i] = (int64_t)(e[i] ^ (1ull << 63));
    free(e); free(tmp);
    pthread_t* th = (pthread_t*)malloc((size_t)c->P * sizeof(pthread_t));
    tri_arg* args = (tri_arg*)calloc((size_t)c->P, sizeof(tri_arg));
    for (int side = 0; side < 2; ++side) {
      for (int t = 0; t < c->P; ++t) {
        args[t] = (tri_arg){ids, V, side ? dst : src, side ? c->cd : c->cs, n * (uint64_t)t / c->P,
                            n * (uint64_t)(t + 1) / c->P, NULL, NULL, NULL, 0};
        pthread_create(&th[t], NULL, tri_map_worker, &args[t]);
      }
      for (int t = 0; t < c->P; ++t) pthread_join(th[t], NULL);
    }
    free(th); free(args); free(ids);
    c->V = V;
  }
  const uint64_t V = c->V;
  /* 2. distinct undirected edges: records grouped by the smaller endpoint, each group sorted + unique */
  c->off = (uint64_t*)calloc(V + 1, sizeof(uint64_t));
  c->cur = (uint64_t*)malloc((V + 1) * sizeof(uint64_t));
  c->lst = (uint32_t*)malloc((n + 1) * sizeof(uint32_t));
  c->ucnt = (uint32_t*)malloc((V + 1) * sizeof(uint32_t));
  tf_par(c, tf_count_lo);
  for (uint64_t x = 0; x < V; ++x) c->off[x + 1] += c->off[x];
  memcpy(c->cur, c->off, (V + 1) * sizeof(uint64_t));
  tf_split(c, c->off, V);
  tf_par(c, tf_fill_lo);
  free(c->cs); free(c->cd);
  c->next = 0;
  tf_par(c, tf_sort_unique);
  /* 3. degrees over distinct edges; orientation x -> y iff (deg x, x) < (deg y, y); sorted out-lists */
  c->deg = (uint32_t*)calloc(V + 1, sizeof(uint32_t));
  tf_par(c, tf_degrees);
  /* ranks: a counting sort by degree, ties by id */
  uint32_t dmax = 0;
  for (uint64_t x = 0; x < V; ++x) dmax = c->deg[x] > dmax ? c->deg[x] : dmax;
  uint64_t* dcnt = (uint64_t*)calloc((uint64_t)dmax + 2, sizeof(uint64_t));
  for (uint64_t x = 0; x < V; ++x) ++dcnt[c->deg[x] + 1];
  for (uint64_t d = 0; d <= dmax; ++d) dcnt[d + 1] += dcnt[d];
  c->rank = (uint32_t*)malloc((V + 1) * sizeof(uint32_t));
  for (uint64_t x = 0; x < V; ++x) c->rank[x] = (uint32_t)dcnt[c->deg[x]]++;
  free(dcnt);
  tf_par(c, tf_rank_lists);
  c->uoff = (uint64_t*)calloc(V + 1, sizeof(uint64_t));
  tf_par(c, tf_count_out);
  for (uint64_t x = 0; x < V; ++x) c->uoff[x + 1] += c->uoff[x];
  memcpy(c->cur, c->uoff, (V + 1) * sizeof(uint64_t));
  tf_split(c, c->uoff, V);
  c->nbr = (uint32_t*)malloc((c->uoff[V] + 1) * sizeof(uint32_t));
  tf_par(c, tf_fill_out);
  c->next = 0;
  tf_par(c, tf_sort_out);
  /* 4. in-lists, then the count */
  const uint64_t Ep = c->uoff[V];
  c->ioff = (uint64_t*)calloc(V + 1, sizeof(uint64_t));
  tf_par(c, tf_count_in);
  for (uint64_t x = 0; x < V; ++x) c->ioff[x + 1] += c->ioff[x];
  memcpy(c->cur, c->ioff, (V + 1) * sizeof(uint64_t));
  tf_split(c, c->ioff, V);
  c->ipos = (uint64_t*)malloc((Ep + 1) * sizeof(uint64_t));
  c->iown = (uint32_t*)malloc((Ep + 1) * sizeof(uint32_t));
  tf_par(c, tf_fill_in);
  c->next = 0;
  tf_par(c, tf_intersect);
  uint64_t T = 0;
  for (int t = 0; t < c->P; ++t) T += c->T[t];
  *T_out = T;
  free(c->off); free(c->cur); free(c->lst); free(c->ucnt); free(c->deg); free(c->rank); free(c->uoff); free(c->ioff); free(c->ipos); free(c->iown); free(c->nbr); free(c);
  return 0;
}

/* ---- ConnectedComponents (library/ConnectedComponents.java:56-131, example/util/DisjointSet.java) ----
 * DisjointSet restated over the window's ids (sorted distinct ids -> index): union(e1, e2) makes absent
 * elements their own set, finds both roots with path compression (find :71-85) and links by rank,
 * ties under root1 (:113-122).  merge(other) = union(key, value) over other's entries (:132-136).
 * ConnectedComponents folds a window's edges into a DisjointSet (UpdateCC :86-90) and the Merger combines
 * it into the running state (CombineCC :120-130; GraphAggregation Merger, transientState = false):
 * the state after a window = union of the previous state's (vertex, parent) entries and the window's
 * edges.  Output: every vertex of the state, ascending, with the smallest vertex of its component
 * (the partition is what the reference's toString / ConnectedComponentsTest observe; which vertex is
 * a root depends on HashMap iteration order and is not part of it).  Returns the vertex count. */
static int64_t ds_find(int64_t* parent, int64_t e) {
  int64_t p = parent[e];
  if (p != e) {
    const int64_t t = ds_find(parent, p);
    if (t != p) {
      p = t;
      parent[e] = p;
    }
  }
  return p;
}

static void ds_union(int64_t* parent, int32_t* rank, int64_t e1, int64_t e2) {
  const int64_t r1 = ds_find(parent, e1), r2 = ds_find(parent, e2);
  if (r1 == r2) return;
  if (rank[r1] > rank[r2]) parent[r2] = r1;
  else if (rank[r1] < rank[r2]) parent[r1] = r2;
  else {
    parent[r2] = r1;
    rank[r1] += 1;
  }
}

static int64_t idx_of(const int64_t* ids, int64_t n, int64_t x) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t m = (a + b) / 2;
    if (ids[m] < x) a = m + 1;
    else b = m;
  }
  return a;
}

GSO_API int64_t gso_components(const int64_t* src, const int64_t* dst, uint64_t n, const int64_t* prev_v,
                               const int64_t* prev_l, uint64_t m, int64_t* out_v, int64_t* out_l) {
  const uint64_t tot = 2 * n + 2 * m;
  int64_t* ids = (int64_t*)malloc((tot + 1) * sizeof(int64_t));
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i) { ids[k++] = src[i]; ids[k++] = dst[i]; }
  for (uint64_t i = 0; i < m; ++i) { ids[k++] = prev_v[i]; ids[k++] = prev_l[i]; }
  qsort(ids, k, sizeof(int64_t), cmp_i64);
  int64_t u = 0;
  for (uint64_t i = 0; i < k; ++i)
    if (i == 0 || ids[i] != ids[i - 1]) ids[u++] = ids[i];
  int64_t* parent = (int64_t*)malloc((u + 1) * sizeof(int64_t));
  int32_t* rank = (int32_t*)calloc(u + 1, sizeof(int32_t));
  for (int64_t i = 0; i < u; ++i) parent[i] = i;
  /* the running state first (its entries merged edge by edge), then the window's edges: the partition
   * is the same in any order */
  for (uint64_t i = 0; i < m; ++i) ds_union(parent, rank, idx_of(ids, u, prev_v[i]), idx_of(ids, u, prev_l[i]));
  for (uint64_t i = 0; i < n; ++i) ds_union(parent, rank, idx_of(ids, u, src[i]), idx_of(ids, u, dst[i]));
  /* canonical label: the smallest vertex of the component */
  int64_t* minv = (int64_t*)malloc((u + 1) * sizeof(int64_t));
  for (int64_t i = 0; i < u; ++i) minv[i] = INT64_MAX;
  for (int64_t i = 0; i < u; ++i) {
    const int64_t r = ds_find(parent, i);
    if (ids[i] < minv[r]) minv[r] = ids[i];
  }
  for (int64_t i = 0; i < u; ++i) {
    out_v[i] = ids[i];
    out_l[i] = minv[ds_find(parent, i)];
  }
  free(minv);
  free(rank);
  free(parent);
  free(ids);
  return u;
}

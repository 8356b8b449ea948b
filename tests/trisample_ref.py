"""A plain restatement of the reference's sampling triangle estimators, the yardstick of the GPU path.

TriangleSamplerRef is BroadcastTriangleCount.java:62-135 (mode "broadcast") and
IncidenceSamplingTriangleCount.java:125-203 (mode "incidence") edge by edge and sampler by sampler, with the
reference's Math.random() replaced by the counter-based draws include/gelly_hip.h documents (the reference's own
random stream is not reproducible).  TriangleSummerRef is :138-174.  Nothing here is shared with the engine:
the loop runs over the edges one at a time, numpy only spreads one edge over the samplers.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
NEVER = 1 << 31
INT_MAX = (1 << 31) - 1
INT_MIN = -(1 << 31)


def mix(seed: int, i: int) -> int:
    """splitmix64 of seed + (i + 1) * golden"""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, sampler: int, j: int, a: int) -> int:
    """r(seed, sampler, j, a): draw a of replacement j of the (global) sampler"""
    return mix(mix(mix(seed & M64, sampler), j), a)


def next_position(K: int, r: int) -> int:
    """the replacement after the one at K: P(> m) = K / m, the product of the coins 1 - 1/k, K < k <= m"""
    k = (K << 32) // ((r >> 32) + 1) + 1
    return NEVER if k > INT_MAX else k


class TriangleSamplerRef:
    def __init__(self, mode: str, samples: int, vertex_count: int, seed: int = 0, first_sampler: int = 0, trace: bool = False):
        assert mode in ("broadcast", "incidence") and samples >= 1 and vertex_count >= 3
        S = samples
        self.mode, self.S, self.V, self.seed, self.first = mode, S, vertex_count, seed, first_sampler
        self.src = np.zeros(S, np.int64)
        self.trg = np.zeros(S, np.int64)
        self.third = np.full(S, -1, np.int64)
        self.src_found = np.zeros(S, bool)
        self.trg_found = np.zeros(S, bool)
        self.beta = np.zeros(S, bool)
        self.held = np.zeros(S, bool)            # a sampler holds an edge after its first replacement
        self.j = np.zeros(S, np.int64)           # replacements done
        self.last = np.zeros(S, np.int64)        # position of the held edge
        self.next = np.ones(S, np.int64)         # position of the next replacement (K_0 = 1)
        self.edge_count = 0
        self.previous = 0
        self.trace = [] if trace else None       # (what, position, sampler): replace / reset / flag / find

    def _note(self, what, i):
        if self.trace is not None:
            self.trace.append((what, self.edge_count, int(i)))

    def edge(self, s: int, d: int) -> list:
        """one edge through all samplers; the TriangleEstimate records (edgeCount, localBetaSum) it emits"""
        self.edge_count += 1
        k = self.edge_count
        before = self.beta.copy()
        # the coin: replaced at the positions of the chain
        for i in np.nonzero(self.next == k)[0]:
            g, j = self.first + int(i), int(self.j[i])
            self.next[i] = next_position(k, draw(self.seed, g, j, 0))
            a = 1
            while True:
                t = (draw(self.seed, g, j, a) * self.V) >> 64
                if t != s and t != d:
                    break
                a += 1
            self._note("reset" if self.beta[i] else "replace", i)
            self.src[i], self.trg[i], self.third[i] = s, d, t
            self.src_found[i] = self.trg_found[i] = self.beta[i] = False
            self.held[i] = True
            self.j[i] = j + 1
            self.last[i] = k
        # the closing edges, while beta == 0
        open_ = self.held & ~self.beta
        hit_s = open_ & (((self.src == s) & (self.third == d)) | ((self.third == s) & (self.src == d)))
        hit_t = open_ & (((self.trg == s) & (self.third == d)) | ((self.third == s) & (self.trg == d)))
        finds = ()
        if hit_s.any() or hit_t.any():
            if self.trace is not None:
                for i in np.nonzero((hit_s & ~self.src_found) | (hit_t & ~self.trg_found))[0]:
                    self._note("flag", i)
            self.src_found |= hit_s
            self.trg_found |= hit_t
            found = open_ & self.src_found & self.trg_found
            self.beta |= found
            finds = np.nonzero(found)[0]
            for i in finds:
                self._note("find", i)
        out = []
        if self.mode == "broadcast":
            total = int(self.beta.sum())
            if total != self.previous:
                self.previous = total
                out.append((k, total))
        else:
            # a record per sampler that just found its triangle, in sampler order: the samplers before it
            # have been through this edge, those after it have not
            for i in finds:
                total = int(self.beta[:i + 1].sum()) + int(before[i + 1:].sum())
                if total != self.previous:
                    self.previous = total
                    out.append((k, total))
        return out

    def edges(self, src, dst) -> list:
        out = []
        for s, d in zip(np.asarray(src, np.int64).tolist(), np.asarray(dst, np.int64).tolist()):
            out.extend(self.edge(s, d))
        return out

    def beta_sum(self) -> int:
        return int(self.beta.sum())

    def rows(self) -> np.ndarray:
        """the checkpoint rows include/gelly_hip.h documents (GS_TRISAMPLE_ROW_WORDS)"""
        r = np.zeros((self.S, 8), np.int64)
        r[:, 0], r[:, 1], r[:, 2] = self.src, self.trg, self.third
        r[:, 3] = self.src_found * 1 + self.trg_found * 2 + self.beta * 4
        r[:, 4], r[:, 5], r[:, 6] = self.j, self.last, self.next
        return r


def java_int_cast(x: float) -> int:
    if x != x:
        return 0
    if x >= INT_MAX:
        return INT_MAX
    if x <= INT_MIN:
        return INT_MIN
    return int(x)


class TriangleSummerRef:
    """BroadcastTriangleCount.java:138-174"""

    def __init__(self, sample_size: int, vertices: int):
        self.results = {}
        self.max_edges = 0
        self.sample_size = sample_size
        self.previous = 0
        self.vertices = vertices

    def estimate(self, source: int, edge_count: int, beta: int) -> list:
        self.results[source] = beta
        self.max_edges = max(self.max_edges, edge_count)
        global_beta = sum(self.results.values())
        result = java_int_cast((1.0 / float(self.sample_size)) * global_beta * self.max_edges * (self.vertices - 2))
        if result != self.previous:
            self.previous = result
            return [(self.max_edges, result)]
        return []

    def feed(self, source: int, records) -> list:
        out = []
        for k, b in records:
            out.extend(self.estimate(source, int(k), int(b)))
        return out

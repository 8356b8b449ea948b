"""CPU helpers of the BipartitenessCheck tests (not a test module).

canonical(): the canonical bipartiteness state DESIGN.md defines ("BipartitenessCheck"), by a sequential
parity union-find -- what gs_window_bipartite must return, bit for bit.

reference_candidates(): a restatement of the reference's own state machine, written from
example/util/Candidates.java and library/BipartitenessCheck.java (cited per line), order dependence and all.
It returns the text line the reference's DataStream<Candidates>.writeAsText would hold after one window at
parallelism 1."""
from __future__ import annotations

import numpy as np


def canonical(src, dst, prev=None):
    """(success, vertices ascending, label = smallest vertex of the component, sign = 1 iff on the label's
    side) over the constraints of `prev` (a previous return value) and the edges; a failed state has no rows
    and stays failed."""
    empty = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.uint8))
    if prev is not None and not prev[0]:
        return (False,) + empty
    x, y = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    d = np.ones(len(x), np.int64)
    if prev is not None and len(prev[1]):
        x = np.concatenate([np.asarray(prev[1], np.int64), x])
        y = np.concatenate([np.asarray(prev[2], np.int64), y])
        d = np.concatenate([1 - np.asarray(prev[3]).astype(np.int64), d])
    ids = np.unique(np.concatenate([x, y]))
    U = len(ids)
    parent, par = list(range(U)), [0] * U

    def find(v):
        path = []
        while parent[v] != v:
            path.append(v)
            v = parent[v]
        p = 0
        for u in reversed(path):   # from the root's child down: side relative to the root
            p ^= par[u]
            parent[u], par[u] = v, p
        return v, (par[path[0]] if path else 0)

    for a, b, dd in zip(np.searchsorted(ids, x).tolist(), np.searchsorted(ids, y).tolist(), d.tolist()):
        if a == b:
            continue   # a self-loop only makes its vertex present
        (ra, pa), (rb, pb) = find(a), find(b)
        if ra == rb:
            if pa ^ pb != dd:
                return (False,) + empty
            continue
        hi, lo = max(ra, rb), min(ra, rb)   # the smaller root stays: the root is its component's smallest vertex
        parent[hi], par[hi] = lo, pa ^ pb ^ dd
    labels, signs = np.empty(U, np.int64), np.empty(U, np.uint8)
    for v in range(U):
        r, p = find(v)
        labels[v], signs[v] = ids[r], 1 - p
    return True, ids, labels, signs


# ---- the reference's Candidates, restated -------------------------------------------------------------
class _Candidates:
    """Candidates.java:26-196: (success, TreeMap<component, TreeMap<vertex, sign>>); the TreeMaps are dicts
    read in ascending key order."""

    def __init__(self, success):   # :30-33
        self.success = success
        self.map = {}

    def add(self, component, vertex, sign):   # :60-73
        comp = self.map.setdefault(component, {})   # :61-63
        if vertex in comp and comp[vertex] != sign:   # :64-68 (returns before the put)
            return False
        comp[vertex] = sign   # :70
        return True

    def add_all(self, component, vertices):   # :51-58
        for v in sorted(vertices):
            if not self.add(component, v, vertices[v]):
                return False
        return True

    def merge(self, inp):   # :76-138
        if not inp.success or not self.success:   # :78-80
            return _Candidates(False)
        for in_key in sorted(inp.map):   # :83
            in_comp = inp.map[in_key]
            merge_with = []   # :85
            for self_key in sorted(self.map):   # :87
                self_comp = self.map[self_key]
                if set(in_comp) == set(self_comp):   # :91-94 equal vertex sets: skipped, whatever the signs
                    continue
                if any(v in self_comp for v in in_comp):   # :97-104
                    merge_with.append(self_key)
            if not merge_with:
                self.add_all(in_key, in_comp)   # :107-110
            else:
                merge_with.sort()   # :113
                first = merge_with[0]
                if not _merge_into(inp, self, in_key, first):   # :117-120
                    return _Candidates(False)
                first = min(in_key, first)   # :122 (the component `merge_with[0]` is not retired)
                for other in merge_with[1:]:   # :125-133
                    _merge_into(self, self, other, first)   # :127-130: the result of fail() is dropped
                    del self.map[other]   # :132
        return self   # :137

    def __str__(self):   # Tuple2.toString over AbstractMap.toString over SignedVertex (a Tuple2)
        comps = ", ".join(
            f"{k}={{{', '.join(f'{v}=({v},{str(s).lower()})' for v, s in sorted(self.map[k].items()))}}}"
            for k in sorted(self.map))
        return f"({str(self.success).lower()},{{{comps}}})"


def _merge_into(inp, cand, in_key, self_key):   # Candidates.java:141-191 (the private merge)
    in_comp, self_comp = inp.map[in_key], cand.map[self_key]
    merge_by = [v for v in sorted(in_comp) if v in self_comp]   # :146-152
    reverse = in_comp[merge_by[0]] != self_comp[merge_by[0]]   # :155-157
    for v in merge_by:   # :160-172
        if (in_comp[v] != self_comp[v]) != reverse:
            return False
    common = min(in_key, self_key)   # :175
    for v, s in sorted(in_comp.items()):   # :178-188
        if not cand.add(common, v, (not s) if reverse else s):
            return False
    return True


def edge_to_candidate(v1, v2):   # BipartitenessCheck.java:57-64
    s, t = min(v1, v2), max(v1, v2)
    c = _Candidates(True)
    c.add(s, s, True)
    c.add(s, t, False)
    return c


def reference_candidates(edges):
    """The line after one window: updateFunction folds the edges into Candidates(true)
    (BipartitenessCheck.java:54, :96-98), the Merger combines the partial with its empty running state
    (GraphAggregation.java:107, combineFunction :131-133)."""
    state = _Candidates(True)
    for a, b in edges:
        state = state.merge(edge_to_candidate(int(a), int(b)))
    return str(state.merge(_Candidates(True)))

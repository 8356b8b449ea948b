"""AssignComponents (example/IterativeConnectedComponents.java:67-168), restated edge by edge from the
semantics table of include/gelly_hip.h ("AssignComponents"): the partition of the vertices seen so far, every
component labelled with its smallest vertex, and one (vertex, label) record per vertex whose label changes.

`AssignLiteral` keeps the mapper's own shape: a dictionary label -> set of vertices and, per edge, a scan over
its entries for the two endpoints.  `AssignFast` keeps vertex -> label and label -> members and is pinned to the
literal one by tests/test_assign_ref.py; the large streams use it.

Reading.  The mapper's comments say "add the target to the source's component"; its addToExistingComponent
(:136-139) emits a vertex that joins a component with a smaller id but never adds it to the set.  `literal=True`
reproduces that; the default is the comments' reading, the one the library builds.  Inside one edge's emission
the mapper follows HashSet iteration order; here the order is canonical: ascending by vertex, and (src, dst)
for the two records of a new component.  Vertex -1 is an ordinary vertex (the mapper uses -1 as "no
component")."""
import random


class AssignLiteral:
    def __init__(self, literal=False):
        self.components = {}   # label -> set of vertices
        self.literal = literal

    def edge(self, s, t):
        """the (vertex, label) records of one arriving edge"""
        sc = tc = None
        for label, members in self.components.items():
            if s in members:
                sc = label
            if t in members:
                tc = label
        if sc is not None and tc is not None:
            return self._merge(sc, tc)
        if sc is not None:
            return self._add(sc, t)
        if tc is not None:
            return self._add(tc, s)
        m = min(s, t)
        self.components[m] = {s, t}
        return [(s, m), (t, m)]

    def _add(self, c, x):
        members = self.components.pop(c)
        if x < c:
            out = [(v, x) for v in sorted(members)]
            members.add(x)
            self.components[x] = members
            return out
        if not self.literal:
            members.add(x)
        self.components[c] = members
        return [(x, c)]

    def _merge(self, a, b):
        if a == b:
            return []
        lo, hi = min(a, b), max(a, b)
        moved = self.components.pop(hi)
        out = [(v, lo) for v in sorted(moved)]
        self.components[lo] |= moved
        return out

    def state(self):
        return {v: label for label, members in self.components.items() for v in members}


class AssignFast:
    """the intended reading with vertex -> label and label -> members: O(records) per edge"""

    def __init__(self):
        self.label = {}
        self.members = {}

    def edge(self, s, t):
        L, M = self.label, self.members
        a, b = L.get(s), L.get(t)
        if a is None and b is None:
            m = min(s, t)
            M[m] = [s] if s == t else [s, t]
            L[s] = L[t] = m
            return [(s, m), (t, m)]
        if a is None or b is None:
            c, x = (b, s) if a is None else (a, t)
            if x < c:
                moved = M.pop(c)
                out = [(v, x) for v in sorted(moved)]
                for v in moved:
                    L[v] = x
                moved.append(x)
                M[x] = moved
                L[x] = x
                return out
            M[c].append(x)
            L[x] = c
            return [(x, c)]
        if a == b:
            return []
        lo, hi = min(a, b), max(a, b)
        moved = M.pop(hi)
        out = [(v, lo) for v in sorted(moved)]
        for v in moved:
            L[v] = lo
        M[lo].extend(moved)
        return out

    def state(self):
        return dict(self.label)


def run(edges, ref=None, base=0):
    """records (vertex, label, position of the edge in the stream) of a stream, and the reference object"""
    ref = ref if ref is not None else AssignFast()
    out = []
    for i, (s, t) in enumerate(edges):
        out.extend((v, c, base + i) for v, c in ref.edge(int(s), int(t)))
    return out, ref


def components_of(edges):
    """vertex -> smallest vertex of its component over the whole stream (a plain union-find)"""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for s, t in edges:
        s, t = int(s), int(t)
        parent.setdefault(s, s)
        parent.setdefault(t, t)
        a, b = find(s), find(t)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return {v: find(v) for v in parent}


# ---- the streams of the tests (CPU model and GPU alike) ------------------------------------------------
BUILTIN = [(k, k + i) for k in range(1, 11) for i in (1, 2)]   # getEdgesDataSet: generateSequence(1, 10) x {+1, +2}
# derived by hand: (1, 2) opens component 1 with (1, 1), (2, 1); edge (k, k + 2), at position 2k - 1, brings the
# unknown k + 2 > 1 into it; every edge (k, k + 1) after the first has both ends in component 1
BUILTIN_RECORDS = [(1, 1, 0), (2, 1, 0)] + [(k + 2, 1, 2 * k - 1) for k in range(1, 11)]

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SPECIAL_IDS = [-1, I64_MIN, I64_MAX, (1 << 32) + 1, (1 << 40) + 5, -(1 << 33), 0, 1]


def rmat_edges(scale, n, seed, a=0.57, b=0.19, c=0.19):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = t = 0
        for _ in range(scale):
            r = rng.random()
            s = 2 * s + (r >= a + b)
            t = 2 * t + (a <= r < a + b or r >= a + b + c)
        out.append((s, t))
    return out


def random_edges(V, n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(V), rng.randrange(V)) for _ in range(n)]


def streams():
    """name -> edge list; `short` ones also run one edge per batch"""
    rng = random.Random(11)
    pairs = [(2 * k, 2 * k + 1) for k in range(150)]
    zipf = [(2 * k + 1, 2 * k + 2) for k in range(149)]
    special = [(rng.choice(SPECIAL_IDS), rng.choice(SPECIAL_IDS)) for _ in range(60)]
    wide = [(2 * k, 2 * k + 1) for k in range(15000)]
    rng.shuffle(wide)
    loops = [(5, 5), (5, 5), (3, 5), (3, 3), (9, 8), (8, 8), (9, 9), (-1, -1), (-1, 3), (7, 7), (2, 7), (2, 2), (2, 9)]
    return {
        "builtin": BUILTIN,
        "random_v8": random_edges(8, 400, 1),
        "random_v200": random_edges(200, 2000, 2),
        "random_v2000": random_edges(2000, 5000, 3),
        "chain_up": [(k, k + 1) for k in range(300)],
        "chain_down": [(k + 1, k) for k in range(299, -1, -1)],
        "star": [(0, k) if k % 2 else (k, 0) for k in range(1, 301)],
        "hub_relabelled": [(300, k) for k in range(299, -1, -1)],
        "pairs_zip_forward": pairs + zipf,
        "pairs_zip_backward": pairs + zipf[::-1],
        "rmat12": rmat_edges(12, 20000, 5),
        "self_loops": loops,
        "special_ids": special,
        "wide_30000": wide,
    }


SHORT = ("builtin", "random_v8", "chain_up", "chain_down", "star", "hub_relabelled", "pairs_zip_forward",
         "pairs_zip_backward", "self_loops", "special_ids")

"""Record-by-record restatement of example/CentralizedWeightedMatching.java's WeightedMatchingFlatMapper
(:67-108) in plain Python: a set of edge tuples, scanned for collisions literally as the Java does, with Java
long arithmetic.  The one thing the Java leaves to HashSet iteration order -- which of two colliding edges is
removed first -- follows the library's canonical order: the edge matched at the arriving edge's src, then the
one at its dst (include/gelly_hip.h, "CentralizedWeightedMatching")."""

ADD, REMOVE = 0, 1          # MatchingEvent.Type ordinals (MatchingEvent.java:26)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def java_long(x: int) -> int:
    """two's-complement wrap to 64 bits"""
    return ((int(x) - I64_MIN) & 0xFFFFFFFFFFFFFFFF) + I64_MIN


class Matching:
    """localMatching (:70) and flatMap (:77-107)"""

    def __init__(self):
        self.M = set()      # (src, dst, val)
        self.records = 0

    def flat_map(self, src: int, dst: int, val: int) -> list:
        """the MatchingEvents of one arriving edge as (type, src, dst, val)"""
        self.records += 1
        collisions = set()                                          # :80-88
        for (s, d, v) in self.M:
            if s == src or s == dst or d == src or d == dst:
                collisions.add((s, d, v))
        total = 0                                                   # :91-94
        for (_, _, v) in collisions:
            total = java_long(total + v)
        if not val > java_long(2 * total):                          # :96
            return []
        # canonical REMOVE order: the collision touching the arriving src first, then the one touching its dst
        ordered = sorted(collisions, key=lambda c: 0 if src in (c[0], c[1]) else 1)
        out = []
        for c in ordered:                                           # :99-102
            self.M.remove(c)
            out.append((REMOVE,) + c)
        self.M.add((src, dst, val))                                 # :104-105
        out.append((ADD, src, dst, val))
        return out

    def edges(self, src, dst, val) -> list:
        """a stream through the mapper: (type, src, dst, val, position in the stream) per event"""
        out = []
        for i, (s, d, v) in enumerate(zip(src, dst, val)):
            out.extend(e + (i,) for e in self.flat_map(int(s), int(d), int(v)))
        return out

    def is_matching(self) -> bool:
        """no vertex in two edges of M"""
        seen = set()
        for (s, d, _) in self.M:
            ends = {s, d}
            if seen & ends:
                return False
            seen |= ends
        return True

    def export(self) -> list:
        return sorted(self.M)

    def total_weight(self) -> int:
        return java_long(sum(v for _, _, v in self.M))


class FastMatching(Matching):
    """The same mapper with the collision scan replaced by a vertex -> edge dictionary (M is a matching, so the
    scan finds at most the edge at src and the edge at dst).  test_matching_ref.py pins it to Matching; the GPU
    tests use it for streams where the literal scan would take minutes."""

    def __init__(self):
        super().__init__()
        self.at = {}

    def flat_map(self, src, dst, val):
        self.records += 1
        ordered = []
        for x in (src, dst):
            c = self.at.get(x)
            if c is not None and c not in ordered:
                ordered.append(c)
        total = 0
        for (_, _, v) in ordered:
            total = java_long(total + v)
        if not val > java_long(2 * total):
            return []
        out = []
        for c in ordered:
            self.M.remove(c)
            self.at.pop(c[0], None)
            self.at.pop(c[1], None)
            out.append((REMOVE,) + c)
        e = (src, dst, val)
        self.M.add(e)
        self.at[src] = self.at[dst] = e
        out.append((ADD,) + e)
        return out

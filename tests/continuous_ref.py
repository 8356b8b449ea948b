"""Plain-Python restatement of SimpleEdgeStream's continuous operators at parallelism 1: a dict (a set)
updated record by record, as DegreeMapFunction (SimpleEdgeStream.java:465-482), FilterDistinctVertices
(:194-209), VertexCountMapper + GlobalAggregateMapper (:375-387, :525-539) and TotalEdgeCountMapper
(:396-408) are written.  Nothing here sorts or groups: it shares no method with the engine."""
IN, OUT, ALL = 0, 1, 2


def expand(src, dst, direction):
    """DegreeTypeSeparator (:444-463) / EmitSrcAndTarget (:185-192): the source's record first, then the
    target's, as the direction collects them."""
    for s, d in zip(src, dst):
        if direction in (OUT, ALL):
            yield int(s)
        if direction in (IN, ALL):
            yield int(d)


class DegreeState:
    """One DegreeMapFunction: vertex -> records seen so far, over any number of batches."""

    def __init__(self, counts=None):
        self.counts = dict(counts or {})
        self.records = 0

    def degrees(self, src, dst, direction):
        out = []
        for v in expand(src, dst, direction):
            self.counts[v] = self.counts.get(v, 0) + 1
            out.append((v, self.counts[v]))
        self.records += len(out)
        return out

    def vertices(self, src, dst):
        """(vertex, number of distinct vertices so far) for every vertex at its first appearance."""
        out = []
        for v in expand(src, dst, ALL):
            if v not in self.counts:
                out.append((v, len(self.counts) + 1))
            self.counts[v] = self.counts.get(v, 0) + 1
        self.records += 2 * len(src)
        return out

    def export(self):
        return sorted(self.counts.items())


def get_degrees(edges, direction):
    return DegreeState().degrees([e[0] for e in edges], [e[1] for e in edges], direction)


def get_vertices(edges):
    return [(v,) for v, _ in DegreeState().vertices([e[0] for e in edges], [e[1] for e in edges])]


def number_of_vertices(edges):
    seen, out, prev = set(), [], None
    for v in expand([e[0] for e in edges], [e[1] for e in edges], ALL):
        seen.add(v)
        if len(seen) != prev:   # GlobalAggregateMapper: only when the value changes
            prev = len(seen)
            out.append(prev)
    return out


def number_of_edges(edges):
    out, count = [], 0
    for _ in edges:
        count += 1
        out.append(count)
    return out


def lines(records):
    """Flink's writeAsCsv of the records, as compareResultsByLinesInMemory reads them: sorted lines."""
    def line(r):
        if not isinstance(r, tuple):
            return str(r)
        return ",".join(str(x) for x in r) + (",(null)" if len(r) == 1 else "")
    return sorted(line(r) for r in records)

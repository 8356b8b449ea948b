"""Plain-Python restatement of SimpleEdgeStream.distinct() (SimpleEdgeStream.java:305-327), record by record.

KEYED is the Javadoc's reading (:300-303, the one TestDistinct pins): a set of targets per source.  INSTANCE is
DistinctEdgeMapper as written (:313-327) at parallelism 1: one set of targets for the whole operator.  Nothing
here sorts or groups: it shares no method with the engine."""
KEYED, INSTANCE = "keyed", "instance"


class DistinctState:
    """One distinct() operator over any number of batches."""

    def __init__(self, mode=KEYED):
        self.mode = mode
        self.neighbors = {} if mode == KEYED else set()
        self.log = []       # the (src, dst) emitted so far, in order
        self.records = 0

    def _new(self, s, d):
        seen = self.neighbors.setdefault(s, set()) if self.mode == KEYED else self.neighbors
        if d in seen:
            return False
        seen.add(d)
        return True

    def edges(self, src, dst, val=None):
        """the batch's emitted edges as (src, dst, val, index inside the batch) rows, in arrival order"""
        out = []
        for i, (s, d) in enumerate(zip(src, dst)):
            s, d = int(s), int(d)
            if self._new(s, d):
                out.append((s, d, None if val is None else val[i], i))
                self.log.append((s, d))
        self.records += len(src)
        return out


def distinct(edges, mode=KEYED):
    """edges: tuples (src, dst, ...) -> the tuples distinct() lets through, whole and in order"""
    st = DistinctState(mode)
    return [tuple(edges[r[3]]) for r in st.edges([e[0] for e in edges], [e[1] for e in edges])]


def lines(records):
    """Flink's writeAsCsv of the records, as compareResultsByLinesInMemory reads them: sorted lines."""
    return sorted(",".join(str(x) for x in r) for r in records)

"""example/CentralizedWeightedMatching.java on the engine.

The reference pipeline is
    graph.getEdges().flatMap(new WeightedMatchingFlatMapper()).setParallelism(1)          (:58-60)
one mapper holding a HashSet of matched edges (:67-108) and emitting MatchingEvents (example/util/
MatchingEvent.java).  Here the matching is a device-resident state (Engine.weighted_matching,
gs_matching.hip) fed in micro-batches; the events are the reference's, with the order of two REMOVEs of one
arriving edge fixed as "the edge at its src, then the edge at its dst" (include/gelly_hip.h) where the
reference follows HashSet iteration order.  The operator is parallelism 1, as in the reference:
env.getParallelism() does not change it.
"""
from __future__ import annotations

import enum

import numpy as np

from .stream import DataStream, SimpleEdgeStream, WindowOutput


class MatchingEvent(tuple):
    """MatchingEvent extends Tuple2<Type, Edge<Long, Long>> (MatchingEvent.java:24-42): (type, (src, dst, val))."""

    class Type(enum.IntEnum):
        ADD = 0
        REMOVE = 1

    ADD, REMOVE = Type.ADD, Type.REMOVE

    def __new__(cls, type_, edge):
        return super().__new__(cls, (cls.Type(int(type_)), tuple(int(x) for x in edge)))

    def geType(self):      # the reference's spelling (:35)
        return self[0]

    getType = geType

    def getEdge(self):
        return self[1]


def _host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def centralized_weighted_matching(edges: SimpleEdgeStream) -> DataStream:
    """CentralizedWeightedMatching (:56-60): the MatchingEvents of the edge stream, in stream order.  The
    stream goes through one fresh device state in env.getMicroBatch()-sized batches; the result does not depend
    on that size.  Edge values are int64 (Edge<Long, Long>)."""
    e = edges.getEdges()
    if e.val is None:
        raise ValueError("CentralizedWeightedMatching needs edge values (Edge<Long, Long>)")
    n = len(e)
    mb = edges.getContext().getMicroBatch() or max(n, 1)
    out = DataStream()
    with edges.getContext().engine.weighted_matching() as state:
        for a in range(0, n, mb):
            t, s, d, v, _ = state.edges(e.src[a:a + mb], e.dst[a:a + mb], e.val[a:a + mb])
            records = [MatchingEvent(ty, (ss, dd, vv))
                       for ty, ss, dd, vv in zip(_host(t).tolist(), _host(s).tolist(), _host(d).tolist(), _host(v).tolist())]
            out.windows.append(WindowOutput(0, 0, ("records", records)))
    return out

"""GraphStream.aggregate(...) for the two aggregations the reference's library ships: ConnectedComponents
(library/ConnectedComponents.java:43-131) and BipartitenessCheck (library/BipartitenessCheck.java:40-136),
both on WindowGraphAggregation.java:30-65 and GraphAggregation.java's Merger.

Per tumbling window of `mergeWindowTime` ms the reference folds the window's edges into a DisjointSet
(UpdateCC -> union) and the parallelism-1 Merger combines it into its running state (CombineCC ->
DisjointSet.merge; transientState = false, so the state accumulates over windows) and emits the state.
Here each window is one gs_window_components call on the GPU with the previous state as input: the
emitted record per vertex is (vertex, smallest vertex of its component) -- the partition DisjointSet
holds (its toString groups by root; which vertex is the root depends on HashMap order).

Parallelism (GraphAggregation.java:103-116, WindowGraphAggregation.java:54-58): the reference keys the
edges by the partition index of the map subtask that saw them (InitialMapper), folds each partition's
window separately, and its parallelism-1 Merger emits the running state after EVERY partial it receives.
At environment parallelism P a window therefore emits one state per non-empty partition, the last of
them the state after the whole window (the only one ConnectedComponentsTest reads: its parser takes the
last line).  The mirror deals the edges to the P partitions as Flink's rebalance from a parallelism-1
source does (round robin over the stream's arrival order) and emits the states after partials 0, 1, ...
in partition order -- one of the orders the reference's merger can see (the partials race to it).

BipartitenessCheck runs the same way on gs_window_bipartite: its state is a Candidates -- (success, the
components with every vertex's side) -- in the canonical form DESIGN.md defines ("BipartitenessCheck"), which
is the reference's Candidates.merge output when the edges arrive in ascending order of min(src, dst).  Each
emission is one Candidates record, as the reference's DataStream<Candidates>."""
from __future__ import annotations

import numpy as np

from .stream import DataStream, WindowOutput, _take


class WindowGraphAggregation:
    """WindowGraphAggregation.java:30-65: windowed fold + merge of a graph property."""

    def __init__(self, mergeWindowTime: int):
        self.mergeWindowTime = int(mergeWindowTime)

    def run(self, stream) -> DataStream:
        raise NotImplementedError

    def _run(self, stream, step, columns) -> DataStream:
        """The windowed fold + merge: state = step(src, dst, state) per partial (one per window at parallelism
        1, one per non-empty round-robin partition at parallelism P), each emitted as columns(state)."""
        env = stream.getContext()
        P = env.getParallelism()
        out = DataStream()
        state = None
        for start, end, w, idx in stream._windows(self.mergeWindowTime, with_index=True):
            if P == 1:
                state = step(w.src, w.dst, state)
                out.windows.append(WindowOutput(start, end, columns(state)))
                continue
            part = np.asarray(idx) % P   # rebalance: record i of the stream to map subtask i mod P
            for k in range(P):
                sel = np.flatnonzero(part == k)
                if len(sel) == 0:   # no fold window for a partition without records: no partial, no emission
                    continue
                state = step(_take(w.src, sel), _take(w.dst, sel), state)
                out.windows.append(WindowOutput(start, end, columns(state)))
        return out


class ConnectedComponents(WindowGraphAggregation):
    """library/ConnectedComponents.java: weakly connected components, merged across windows."""

    def run(self, stream) -> DataStream:
        return self._run(stream, stream.getContext().engine.components, lambda state: state)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


class Candidates:
    """example/util/Candidates.java:26-196, a Tuple2<Boolean, TreeMap<Long, Map<Long, SignedVertex>>>, as
    columns: success and, per vertex (ascending), its component's label and its sign (True = on the label's
    side).  A failed state holds no rows (Candidates.fail() :193-195).  The columns stay where the engine left
    them (device tensors / numpy); str() and == read them on the host."""

    def __init__(self, success, vertices=(), labels=(), signs=()):
        self.success = bool(success)
        self.vertices, self.labels, self.signs = vertices, labels, signs

    def _rows(self):
        v, lab, s = _host(self.vertices).astype(np.int64), _host(self.labels).astype(np.int64), _host(self.signs)
        return v, lab, s.astype(bool)

    def __eq__(self, other):
        if not isinstance(other, Candidates):
            return NotImplemented
        return self.success == other.success and all(np.array_equal(a, b) for a, b in zip(self._rows(), other._rows()))

    __hash__ = None

    def __str__(self):
        """Tuple2.toString of (Boolean, TreeMap): (true,{1={1=(1,true), 2=(2,false)}, 7={...}}) / (false,{})."""
        v, lab, s = self._rows()
        order = np.lexsort((v, lab))   # TreeMap of components by label, each a TreeMap by vertex
        comps, cur = [], None
        for i in order:
            if cur is None or lab[i] != cur:
                cur = lab[i]
                comps.append((cur, []))
            comps[-1][1].append(f"{v[i]}=({v[i]},{'true' if s[i] else 'false'})")
        body = ", ".join(f"{k}={{{', '.join(rows)}}}" for k, rows in comps)
        return f"({'true' if self.success else 'false'},{{{body}}})"

    def __repr__(self):
        return f"Candidates{self}" if len(self.vertices) <= 16 else f"Candidates(success={self.success}, {len(self.vertices)} vertices)"


class BipartitenessCheck(WindowGraphAggregation):
    """library/BipartitenessCheck.java: whether the edges seen so far have an odd cycle, and the two sides of
    every component while they have none; merged across windows."""

    def run(self, stream) -> DataStream:
        return self._run(stream, stream.getContext().engine.bipartite, lambda state: ("records", [Candidates(*state)]))

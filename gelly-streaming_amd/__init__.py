"""gelly-streaming_amd — MI355X-native engine for gelly-streaming's per-window neighbourhood path.

The drop-in boundary is the C ABI of libgellyhip.so (include/gelly_hip.h).  This package is the
host-side mirror of the reference's Java API for that path (SimpleEdgeStream.slice ->
GraphWindowStream.reduceOnEdges / foldNeighbors / applyOnNeighbors, WindowTriangles), the engine
binding, and the multi-GPU window shuffle.

The directory name contains a hyphen, so it is loaded by path:
    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("gelly_streaming_amd", ".../gelly-streaming_amd/__init__.py")
or with ``load_package()`` from __graft_entry__.py.
"""
from ._lib import GsError, load as load_library  # noqa: F401
from .engine import (AggregateState, AssignComponentsState, CommGroup, ContinuousState, DistinctState, Engine, StageTimes,  # noqa: F401
                     TriangleSamplerState, WeightedMatchingState)
from .functions import (Collector, CountFold, CountReduce, DegreeMaxNeighborFold, EdgesApply, EdgesFold,  # noqa: F401
                        EdgesReduce, MaxReduce, MaxValuesFold, MinReduce, MinValuesFold, SumReduce, SumValuesFold,
                        EdgeValueSeparator, GlobalRunningCount, GlobalRunningMax, GlobalRunningMin, GlobalRunningSum,
                        RunningCount, RunningMax, RunningMin, RunningSum)
from .stream import (AscendingTimestampExtractor, DataStream, EdgeColumns, EdgeDirection,  # noqa: F401
                     EdgeValueTimestampExtractor, GraphWindowStream, SimpleEdgeStream, SlicePlan,
                     StreamExecutionEnvironment, Time, TimeUnit, plan_slice, window_span)
from .triangles import CountTriangles, GenerateCandidateEdges, window_triangles  # noqa: F401
from .triangle_estimate import (TriangleSummer, broadcast_triangle_count,  # noqa: F401
                                incidence_sampling_triangle_count)
from .matching import MatchingEvent, centralized_weighted_matching  # noqa: F401
from .iterative_cc import AssignComponents, IterativeConnectedComponents  # noqa: F401
from .aggregation import BipartitenessCheck, Candidates, ConnectedComponents, WindowGraphAggregation  # noqa: F401

__all__ = [n for n in dir() if not n.startswith("_")]

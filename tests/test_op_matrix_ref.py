"""CPU: the cross-operator matrix's catalogue (tests/op_matrix.py) is what it says it is, and the matrix can fail.

* every variant's precondition holds against the thresholds read from the code, and its expected is non-trivial;
* the pair sequences over the whole catalogue visit every ordered pair of variants, self-pairs included;
* a ModelEngine that answers every call from the references passes the whole matrix, and two deliberately leaky
  models -- one that answers a reduce with the previous reduce's key range (a leaked prediction), one whose
  gs_fetch_last_output returns the previous call's staged rows (stale scratch) -- are each caught by a named pair.
  No library code is mutated: the models stand in for the engine."""
import numpy as np
import pytest

import assign_ref
import continuous_ref
import distinct_ref
import matching_ref
import op_matrix as M
import trisample_ref
from bipartite_cpu import canonical
from idmaps import id_span, mask_bits


def _oracle():
    import __graft_entry__ as ge
    return ge.load_oracle()


# ---- the catalogue ----------------------------------------------------------------------------------------------
ISSUE_NAMES = """reduce_i64_a reduce_i64_crowded reduce_i64_escapes reduce_f64_all reduce_i32_min_in reduce_count_out
fold_i64_in_init degmax_all degmax_far reduce_i64_wide reduce_f32_narrow4 csr_out_i32 csr_all_f64 csr_in_wide
tri_b14_loops tri_b18 tri_b24 tri_relabel candidates_sparse count_candidates candidate_count cc_small cc_two_phase
cc_relabel_state bip_two_phase bip_relabel bip_odd_cycle parse_text partials_merge reduce_chunked cont_degrees_all
distinct_keyed matching assign trisample_broadcast err_capacity_reduce err_capacity_cc err_bad_direction err_text
err_cand_session""".split()


def test_catalogue_is_the_issues():
    assert list(M.NAMES) == ISSUE_NAMES
    assert len(M.PLAIN) == 35 and len(M.ERRORS) == 5
    assert [n for n in M.NAMES if M.VARIANTS[n].stateful] == ["cont_degrees_all", "distinct_keyed", "matching", "assign",
                                                             "trisample_broadcast", "err_cand_session"]


@pytest.mark.parametrize("name", M.NAMES)
def test_precondition_and_expected(name):
    v = M.VARIANTS[name]
    v.precondition()
    e = v.expected()
    assert e is v.expected()   # computed once
    v.nontrivial(e)
    for col in v.inputs():
        if isinstance(col, np.ndarray):
            assert len(col) <= 70_000 and not col.flags.writeable


def test_thresholds_the_issue_names():
    V = M.VARIANTS
    assert len(V["cc_two_phase"].inputs()[0]) >= 65_536 and len(V["bip_two_phase"].inputs()[0]) >= 65_536
    assert V["bip_odd_cycle"].expected()[0] is False and canonical(*V["bip_odd_cycle"].inputs()[:2])[0] is False
    for name in ("tri_b14_loops", "tri_b18", "tri_b24", "tri_relabel"):
        assert V[name].expected()[0] > 0
    for name in M.BUCKET:   # (span >> S) + 1 in (1, 2048), S by accumulator width
        v = V[name]
        s, d = v.inputs()[:2]
        direction = {"reduce_f64_all": M.ALL, "degmax_all": M.ALL, "reduce_i32_min_in": M.IN, "fold_i64_in_init": M.IN}.get(name, M.OUT)
        S = {"reduce_i32_min_in": 15, "reduce_count_out": 15, "degmax_all": 13, "degmax_far": 13}.get(name, 14)
        assert 1 < (id_span(*M._key_columns(s, d, direction)) >> S) + 1 < 2048, name
    s, d, _ = V["reduce_i64_wide"].inputs()
    assert mask_bits(s, s) > 32
    s, d = V["csr_in_wide"].inputs()[:2]
    assert mask_bits(d, d) > 32
    for name, col in (("csr_out_i32", 0), ("csr_all_f64", 0), ("csr_in_wide", 1)):
        inp = V[name].inputs()
        assert int(np.sum(inp[col] == inp[3])) > 8192, name   # the hub's run crosses a SORT_TILE
    # the three same-geometry variants share (base, S, direction) and the bucket count
    spans = {id_span(*M._key_columns(*V[n].inputs()[:2], M.OUT)) for n in ("reduce_i64_a", "reduce_i64_crowded", "reduce_i64_escapes")}
    assert spans == {(1 << 18) - 1}
    assert (1 << 24) > M.TRI_PARTITIONED_V and mask_bits(*V["tri_b24"].inputs()) == 24


def test_pair_sequences_visit_every_ordered_pair():
    N = len(M.NAMES)
    seen = set()
    for a in M.NAMES:
        for b in M.NAMES:
            seq = M.pair_sequence(a, b)
            assert len(seq) == 6
            assert M.ordered_pairs(seq) >= {(a, b), (b, b), (b, a), (a, a)}
            seen |= M.ordered_pairs(seq)
    assert len(seen) == N * N == 1600
    assert seen == {(a, b) for a in M.NAMES for b in M.NAMES}


def test_expand_gives_state_variants_their_two_halves():
    calls = M.expand(M.pair_sequence("matching", "reduce_i64_a"))
    assert calls == [("matching", "first"), ("reduce_i64_a", "first"), ("reduce_i64_a", "first"), ("matching", "second"),
                     ("matching", "first"), ("reduce_i64_a", "first"), ("matching", "second")]
    calls = M.expand(M.pair_sequence("assign", "matching"))   # the other operator runs inside the stream, both ways
    assert calls[:4] == [("assign", "first"), ("matching", "first"), ("matching", "second"), ("assign", "second")]
    assert calls[4:] == [("assign", "first"), ("matching", "first"), ("assign", "second"), ("matching", "second")]
    for seed in range(4):
        w = M.walk(seed, 200)
        assert len(w) == 200 and set(w) <= set(M.PLAIN) and w == M.walk(seed, 200)
        ex = M.expand(w)
        for n in M.NAMES:   # every first half has its second
            halves = [h for name, h in ex if name == n]
            if M.VARIANTS[n].stateful:
                assert halves[0::2] == ["first"] * (len(halves) // 2) and halves[1::2] == ["second"] * (len(halves) // 2)
    assert set().union(*(set(M.walk(seed, 200)) for seed in range(4))) == set(M.PLAIN)


# ---- the models -------------------------------------------------------------------------------------------------
class ModelError(Exception):
    def __init__(self, status):
        super().__init__(f"status {status}")
        self.status = status


_MEMO = {}


def _key(x):
    """a column by the memory it views (the catalogue's inputs are built once and frozen; a batch is a slice of one)"""
    if isinstance(x, np.ndarray):
        return (x.ctypes.data, x.shape, x.dtype.str)
    if isinstance(x, (tuple, list)):
        return tuple(_key(y) for y in x)
    return x


def _memo(what, args, fn):
    """the reference's answer for these arguments, computed once per process: the matrix asks ten thousand times"""
    k = (what, _key(args))
    if k not in _MEMO:
        _MEMO[k] = (fn(), args)   # (the arguments are kept: their memory stays theirs while the entry lives)
    return _MEMO[k][0]


class _ModelState:
    """A device-resident state: the reference object of its kind, fed batch by batch.  The answers are memoized by
    the batches fed so far, and the reference itself is only run (over all of them) when an answer is missing."""

    def __init__(self, engine, kind, make, feed, export):
        self.engine, self.closed = engine, False
        self.kind, self.make, self.feed_ref, self.export_ref = kind, make, feed, export
        self.fed = []
        engine.open_states += 1

    def close(self):
        if not self.closed:
            self.closed = True
            self.engine.open_states -= 1

    def _replay(self):
        ref, outs = self.make(), []
        for batch in self.fed:
            outs.append(self.feed_ref(ref, *batch))
        return outs[-1], self.export_ref(ref)

    def _answer(self):
        return _memo(self.kind, tuple(self.fed), self._replay)

    def edges(self, *batch):
        assert not self.closed
        self.engine._begin()
        self.fed.append(batch)
        return self._answer()[0]

    def degrees(self, s, d, direction):
        return self.edges(s, d, direction)

    def export(self):
        assert not self.closed
        return self._answer()[1]


def _assign_feed(ref, s, d):
    rec, _ = assign_ref.run(list(zip(s.tolist(), d.tolist())), ref)
    return M._columns(rec, (np.int64, np.int64, np.uint32))


_STATES = {
    "continuous": (continuous_ref.DegreeState,
                   lambda r, s, d, direction: M._columns(r.degrees(s, d, direction), (np.int64, np.int64)),
                   lambda r: M._columns(r.export(), (np.int64, np.int64))),
    "distinct": (lambda: distinct_ref.DistinctState(distinct_ref.KEYED),
                 lambda r, s, d, v: M._columns(r.edges(s, d, v), (np.int64,) * 4),
                 lambda r: M._columns(r.log, (np.int64, np.int64))),
    "matching": (matching_ref.FastMatching,
                 lambda r, s, d, v: M._columns(r.edges(s, d, v), (np.uint8, np.int64, np.int64, np.int64, np.int64)),
                 lambda r: M._columns(r.export(), (np.int64,) * 3)),
    "assign": (assign_ref.AssignFast, _assign_feed,
               lambda r: M._columns(sorted(r.state().items()), (np.int64, np.int64))),
}


class ModelEngine:
    """Every entry point the catalogue calls, answered from the references.  What a real ctx shares between calls is
    modelled as far as the leaky subclasses need: the key range the last reduce measured, the rows it staged, and
    the call sequence number that ends a candidates session."""

    def __init__(self):
        self.o = _oracle()
        self.call_seq, self.cand = 0, None
        self.range, self.staged = None, None
        self.max_records = 0
        self.open_states = 0
        self.last_candidates_jdk_flags = 0

    def _begin(self):
        self.call_seq += 1

    # the reduce family: one place where a result is delivered, so a leak has one place to enter
    def _deliver(self, rows):
        self.range = (int(rows[0].min()), int(rows[0].max())) if len(rows[0]) else None
        self.staged = rows
        return rows

    def _window(self, direction, what, args, fn):
        self._begin()
        if direction not in (M.IN, M.OUT, M.ALL):
            raise ModelError(M.GS_EINVAL)
        return self._deliver(_memo(what, args + (direction,), fn))

    def reduce(self, s, d, v, direction, op):
        return self._window(direction, "reduce", (s, d, v, op), lambda: self.o.window_reduce(s, d, v, direction, op))

    def fold(self, s, d, v, direction, op, init):
        return self._window(direction, "fold", (s, d, v, op, init), lambda: self.o.window_fold(s, d, v, direction, op, init))

    def fold_degree_max(self, s, d, direction):
        return self._window(direction, "degmax", (s, d), lambda: self.o.window_fold_degree_max(s, d, direction))

    def set_max_window_records(self, n):
        self.max_records = n

    def reduce_partials(self, s, d, v, direction, op, nparts):
        k, p = self.reduce(s, d, v, direction, op)
        owner = (k.view(np.uint64) % np.uint64(nparts)).astype(np.int64)   # any fixed owner function will do
        order = np.argsort(owner, kind="stable")
        return k[order], p[order], np.bincount(owner, minlength=nparts).tolist()

    def merge_partials(self, k, p, op):
        assert op == M.SUM
        self._begin()
        return self._deliver(self.o.window_reduce(k, k, p, M.OUT, M.SUM))

    def reduce_short_then_fetch(self, s, d, v, direction, op):
        self._begin()
        rows = _memo("reduce", (s, d, v, op, direction), lambda: self.o.window_reduce(s, d, v, direction, op))
        self._stage_failed(rows)
        return (M.GS_ECAPACITY, len(rows[0])) + tuple(self.staged)

    def _stage_failed(self, rows):
        self.staged = rows

    def csr(self, s, d, v, direction):
        self._begin()
        return _memo("csr", (s, d, v, direction), lambda: self.o.window_csr(s, d, v, direction))

    def triangles(self, s, d):
        self._begin()

        def count():
            if np.any(s == d):
                w, ex, has, _ = self.o.window_triangles_ref(s, d)
            else:
                w, ex, has = self.o.window_triangles_fwd(s, d)
            return ex, w, has
        return _memo("triangles", (s, d), count)

    def _candidates(self, s, d):
        return _memo("candidates", (s, d), lambda: self.o.window_candidates(s, d))

    def candidates(self, s, d):
        self._begin()
        a, b, f, flags = self._candidates(s, d)
        self.last_candidates_jdk_flags = flags
        return a, b, f

    def candidate_count(self, s, d):
        self._begin()
        return _memo("candidate_count", (s, d), lambda: self.o.candidate_count(s, d))

    def count_candidates(self, a, b, f):
        self._begin()
        w, ex, has, groups = _memo("count_candidates", (a, b, f), lambda: self.o.count_candidates(a, b, f))
        return ex, w, has, groups

    def candidates_begin(self, s, d):
        self._begin()
        a, b, f, _ = self._candidates(s, d)
        self.cand = {"seq": self.call_seq, "rows": (a, b, f), "at": 0}
        return len(a)

    def candidates_next(self, capacity):
        if self.cand is None or self.cand["seq"] != self.call_seq:
            raise ModelError(M.GS_EINVAL)
        at, rows = self.cand["at"], self.cand["rows"]
        self.cand["at"] = end = min(at + capacity, len(rows[0]))
        return tuple(r[at:end] for r in rows) + (at, end == len(rows[0]))

    def components(self, s, d, prev=None):
        self._begin()
        return _memo("components", (s, d, prev), lambda: self.o.components(s, d, prev))

    def components_short(self, s, d, U):
        return M.GS_ECAPACITY, len(self.components(s, d)[0])

    def bipartite(self, s, d):
        self._begin()
        return _memo("bipartite", (s, d), lambda: canonical(s, d))

    def parse_edges_text(self, text, out_device=False):
        self._begin()

        def parse():
            try:
                return self.o.parse_edges_text(text)
            except ValueError:
                return ModelError(M.GS_EINVAL)
        got = _memo("text", (text,), parse)
        if isinstance(got, ModelError):
            raise got
        return got

    def _state(self, kind):
        return _ModelState(self, kind, *_STATES[kind])

    def continuous(self):
        return self._state("continuous")

    def distinct(self, mode):
        assert mode == "keyed"
        return self._state("distinct")

    def weighted_matching(self):
        return self._state("matching")

    def assign_components(self):
        return self._state("assign")

    def triangle_sampler(self, mode, samples, vertex_count, seed):
        def export(r):
            return {"edges_seen": r.edge_count, "beta_sum": r.beta_sum(), "last_emitted": r.previous}, r.rows()
        return _ModelState(self, ("trisample", mode, samples, vertex_count, seed),
                           lambda: trisample_ref.TriangleSamplerRef(mode, samples, vertex_count, seed=seed),
                           lambda r, s, d: M._columns(r.edges(s, d), (np.int64, np.int64)), export)


class LeakyPrediction(ModelEngine):
    """a reduce answered with the previous reduce's key range: rows outside it are lost"""

    def _deliver(self, rows):
        prev = self.range
        super()._deliver(rows)
        if prev is None:
            return rows
        keep = (rows[0] >= prev[0]) & (rows[0] <= prev[1])
        return tuple(r[keep] for r in rows)


class StaleScratch(ModelEngine):
    """gs_fetch_last_output after a short output delivers what the call before staged"""

    def _stage_failed(self, rows):
        if self.staged is None:   # (nothing staged before: nothing stale to hand out)
            self.staged = rows


# ---- the harness has teeth ---------------------------------------------------------------------------------------
def _failing_pairs(model_class, pairs):
    failed = []
    for a, b in pairs:
        eng = model_class()
        try:
            M.run_sequence(eng, M.pair_sequence(a, b))
        except AssertionError as e:
            failed.append((a, b, str(e)))
        assert eng.open_states == 0, (a, b)   # a failing sequence closes what it opened
    return failed


def test_honest_model_passes_the_whole_matrix():
    eng = ModelEngine()   # one engine, as the GPU module shares one
    for a in M.NAMES:
        for b in M.NAMES:
            M.run_sequence(eng, M.pair_sequence(a, b))
    assert eng.open_states == 0
    for e in M.ERRORS:
        for b in M.PLAIN:
            M.run_sequence(eng, [b, e, b])
    M.run_sequence(eng, M.walk(0, 200))
    assert eng.open_states == 0 and eng.max_records == 0


REDUCES = [n for n in M.NAMES if M.VARIANTS[n].group in ("bucket", "sort")]


def test_leaked_prediction_is_caught():
    pairs = [(a, b) for a in REDUCES for b in REDUCES]
    failed = _failing_pairs(LeakyPrediction, pairs)
    caught = {(a, b) for a, b, _ in failed}
    assert ("reduce_i64_a", "reduce_i32_min_in") in caught and ("reduce_i64_a", "reduce_i64_wide") in caught
    assert not any(a == b for a, b in caught)   # a window after itself has its own range: no false alarm
    msg = next(m for a, b, m in failed if (a, b) == ("reduce_i64_a", "reduce_i32_min_in"))
    # the message names the sequence, the position and the previous call
    assert "call 1 = reduce_i32_min_in.first after reduce_i64_a.first" in msg and "reduce_i64_a" in msg.split(":")[0]


def test_stale_scratch_is_caught():
    failed = _failing_pairs(StaleScratch, [(a, "err_capacity_reduce") for a in M.NAMES])
    caught = {a for a, _, _ in failed}
    assert set(REDUCES) <= caught and "err_capacity_reduce" not in caught
    assert _failing_pairs(StaleScratch, [("reduce_i64_a", "tri_b18"), ("cc_small", "csr_out_i32")]) == []


def test_an_open_state_variant_is_closed_when_its_partner_fails():
    eng = LeakyPrediction()
    with pytest.raises(AssertionError, match="reduce_i32_min_in.first after matching.first"):
        M.run_sequence(eng, ["reduce_i64_a", "matching", "reduce_i32_min_in"])
    assert eng.open_states == 0


def test_cand_session_ends_with_the_next_entry_point():
    eng = ModelEngine()
    M.run_sequence(eng, ["err_cand_session", "err_cand_session"])            # back to back: chunk 2 follows chunk 1
    M.run_sequence(eng, ["err_cand_session", "cc_small", "err_cand_session"])   # a call in between: EINVAL

    class Stale(ModelEngine):   # a session that survives other calls hands out stale records: caught
        def candidates_next(self, capacity):
            self.cand["seq"] = self.call_seq
            return super().candidates_next(capacity)

    with pytest.raises(AssertionError, match="err_cand_session.second"):
        M.run_sequence(Stale(), ["err_cand_session", "cc_small"])

"""GPU: the device-resident hash tables (gs_continuous / gs_distinct / gs_matching / gs_assign / gs_trisample)
under hash collisions built with tests/hash_adversary.py.  Random ids give probe chains of one to three slots;
these streams put K keys into one probe chain, so probes wrap past the last slot, hundreds of lanes of several
workgroups claim slots of one cluster in one kernel, tags and whole 64-bit hashes match between different keys,
and clusters survive or split at a doubling.  Every state starts with reserve 0 (64 slots) and grows under the
cluster.  Every case first asserts its evidence -- with the helper, at the slot count the state reports, the keys
do share a home slot; the table doubled -- and then compares with the reference model of the same stream, exactly."""
import copy
import functools

import numpy as np
import pytest
import torch

import assign_ref
import continuous_ref as cref
import distinct_ref
import hash_adversary as ha
import matching_ref
import trisample_ref

pytestmark = pytest.mark.gpu
K = ha.K
OUT, ALL = 1, 2
GS_ECAPACITY = -2


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def _rows(cols):
    return list(zip(*(_np(c).tolist() for c in cols)))


def _cuts(n, sizes, base=0):
    """[(a, b)] covering [base, base + n): batches of the given sizes, the last size repeating"""
    out, a, i = [], 0, 0
    while a < n:
        b = min(n, a + sizes[min(i, len(sizes) - 1)])
        out.append((base + a, base + b))
        a, i = b, i + 1
    return out


def _cut_list(n, cut):
    if cut == "whole":
        return [(0, n)]
    if cut == "random":      # the first batches are small: the first table (64 slots) holds a cluster before it doubles
        return _cuts(n, [16, 16, 32, 64, 128] + np.random.default_rng(0xC07).integers(1, 900, 64).tolist())
    return _cuts(n, [int(cut)])


def _need(name, n, slots):
    """the keys that must share the fullest home slot when n keys of the id set are in a table of `slots`"""
    if name == "adjacent":
        return (n + 1) // 2
    if name == "splits":
        return -(-n * ha.INITIAL_SLOTS // slots)
    return n


class Evidence:
    """per state: after every batch, the cluster ids seen so far collide at the slot count the state reports"""

    def __init__(self, clusters):
        self.sets = {name: set(ids.tolist()) for name, ids in clusters.items()}
        self.inside = {name: [] for name in clusters}
        self.slots = None
        self.grown_with = 0      # the most cluster ids a table held when it was doubled

    def see(self, ids):
        for name, s in self.sets.items():
            have = set(self.inside[name])
            self.inside[name] += [v for v in dict.fromkeys(ids) if v in s and v not in have]

    def check(self, slots, before=None):
        if self.slots is not None and slots != self.slots:
            self.grown_with = max(self.grown_with, sum(before) if before is not None else 0)
        self.slots = slots
        for name, ids in self.inside.items():
            top = ha.check_cluster(name, ids, slots)
            assert top >= _need(name, len(ids), slots), (name, top, len(ids), slots)

    def counts(self):
        return [len(v) for v in self.inside.values()]


# ---- ContinuousState -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cont(name):
    return ha.continuous_stream(name)


def _cont_batch(st, model, S, D, src, dst, a, b, op):
    """one batch through the state and through the model: (got rows, wanted rows)"""
    s, d = src[a:b].tolist(), dst[a:b].tolist()
    if op == "vertices":
        return _rows(st.vertices(S[a:b], D[a:b])), model.vertices(s, d)
    direction = ALL if op == "all" else OUT
    return _rows(st.degrees(S[a:b], D[a:b], direction)), model.degrees(s, d, direction)


@pytest.mark.parametrize("cut", ["whole", "257", "random"])
@pytest.mark.parametrize("op", ["all", "out", "vertices"])
@pytest.mark.parametrize("name", ha.ID_SETS)
def test_continuous_state_with_one_cluster(engine, name, op, cut):
    src, dst, cluster = _cont(name)
    S, D = _dev(src), _dev(dst)
    model, ev = cref.DegreeState(), Evidence({name: cluster})
    with engine.continuous() as st:
        assert st.capacity() == (ha.INITIAL_SLOTS, 0)
        for i, (a, b) in enumerate(_cut_list(len(src), cut)):
            before = ev.counts()
            got, want = _cont_batch(st, model, S, D, src, dst, a, b, op)
            ev.see(src[a:b].tolist() + ([] if op == "out" else dst[a:b].tolist()))
            slots, growths = st.capacity()
            ev.check(slots, before)
            if name == "splits" and cut == "random" and i == 0:     # one cluster in the first table
                assert slots == ha.INITIAL_SLOTS and growths == 0
                assert ha.check_cluster(name, ev.inside[name], slots) == ev.counts()[0] >= (8 if op == "out" else 20)
            assert 2 * len(model.counts) <= slots
            assert got == want, (a, b)
            assert st.size() == (len(model.counts), model.records)
        assert ev.counts() == [K] and growths >= 3
        if cut != "whole":
            assert ev.grown_with >= 20           # a rehash moved keys of the cluster
        ex = _rows(st.export())
        assert ex == model.export() and [k for k, _ in ex] == sorted(k for k, _ in ex)


@pytest.mark.parametrize("name", ha.ID_SETS)
def test_continuous_export_load_in_mid_stream(engine, name):
    src, dst, cluster = _cont(name)
    S, D = _dev(src), _dev(dst)
    n, h = len(src), len(src) // 2
    model, ev = cref.DegreeState(), Evidence({name: cluster})
    with engine.continuous() as a, engine.continuous() as b:
        for lo, hi in _cuts(h, [257]):
            got, want = _cont_batch(a, model, S, D, src, dst, lo, hi, "all")
            assert got == want
        ev.see(src[:h].tolist() + dst[:h].tolist())
        ev.check(a.capacity()[0])
        assert ev.counts()[0] > K // 2
        keys, counts = a.export()
        assert _rows((keys, counts)) == model.export()
        b.load(keys, counts)                       # every key of the cluster claims its slot in one kernel
        ev.check(b.capacity()[0])
        assert b.capacity()[1] >= 3 and b.size() == a.size() and _rows(b.export()) == model.export()
        for lo, hi in _cuts(n - h, [257], h):
            ga, want = _cont_batch(a, model, S, D, src, dst, lo, hi, "all")
            gb = _rows(b.degrees(S[lo:hi], D[lo:hi], ALL))
            assert ga == want and gb == want
        ev.see(src.tolist() + dst.tolist())
        ev.check(a.capacity()[0])
        ev.check(b.capacity()[0])
        assert ev.counts() == [K]
        assert _rows(a.export()) == model.export() and _rows(b.export()) == model.export() and a.size() == b.size()


# ---- DistinctState ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dist(mode):
    src, dst, val, groups = ha.distinct_stream(mode)
    h = {g: ha.distinct_key_hash(mode, *groups[g]) for g in groups}
    keyed = mode == "keyed"
    planted = {(s, d) if keyed else d for g in ("a", "b") for s, d in zip(groups[g][0].tolist(), groups[g][1].tolist())}
    return src, dst, val, h, planted


def _dist_evidence(mode, h, slots):
    """at this slot count: a's K keys and b's 301 share the last slot as their home (b shares one tag, which is a
    tag of a too); keyed: c's 65 keys share the whole 64-bit hash"""
    tail = np.concatenate([h["a"], h["b"]])
    assert len(tail) == K + 301 and np.all(ha.home(tail, slots) == slots - 1)
    assert len(np.unique(ha.tag(h["a"]))) == K and set(ha.tag(h["b"]).tolist()) < set(ha.tag(h["a"]).tolist())
    if mode == "keyed":
        assert len(h["c"]) == 65 and len(np.unique(h["c"])) == 1


def _dist_feed(st, model, mode, cols, cuts, h, planted, dev):
    """the batches through the state and the model, compared column by column; the most planted keys the log
    held at a doubling"""
    src, dst, val = cols
    S, D, V = (_dev(src), _dev(dst), _dev(val)) if dev else cols
    keyed = mode == "keyed"
    slots, in_log, grown_with = st.capacity()[0], sum(((s, d) if keyed else d) in planted for s, d in model.log), 0
    for a, b in cuts:
        want = model.edges(src[a:b].tolist(), dst[a:b].tolist(), val[a:b].tolist())
        os_, od, ov, oi = st.edges(S[a:b], D[a:b], V[a:b])
        now = st.capacity()[0]
        if now != slots:                 # the planted keys' hashes are fixed: the evidence depends on the slot count alone
            _dist_evidence(mode, h, now)
            grown_with, slots = max(grown_with, in_log), now
        assert _np(os_).tolist() == [r[0] for r in want], (a, b)
        assert _np(od).tolist() == [r[1] for r in want], (a, b)
        assert _np(ov).tolist() == [r[2] for r in want], (a, b)
        assert _np(oi).tolist() == [r[3] for r in want], (a, b)        # the smallest arrival won its slot
        in_log += sum(((r[0], r[1]) if keyed else r[1]) in planted for r in want)
    _dist_evidence(mode, h, slots)
    return grown_with


@pytest.mark.parametrize("cut", ["whole", "257", "1"])
@pytest.mark.parametrize("mode", ["keyed", "instance"])
def test_distinct_state_with_one_cluster(engine, mode, cut):
    src, dst, val, h, planted = _dist(mode)
    model = distinct_ref.DistinctState(mode)
    with engine.distinct(mode) as st:
        assert st.capacity() == (ha.INITIAL_SLOTS, 0)
        grown_with = _dist_feed(st, model, mode, (src, dst, val), _cut_list(len(src), cut), h, planted, dev=cut != "1")
        slots, growths = st.capacity()
        assert growths >= 3 and 2 * len(model.log) <= slots
        if cut != "whole":
            assert grown_with >= K // 2          # k_ds_rebuild re-inserted a log that held the cluster
        assert len(planted & {(s, d) if mode == "keyed" else d for s, d in model.log}) == K + 301
        assert st.size() == (len(model.log), len(src))
        assert _rows(st.export()) == model.log


@pytest.mark.parametrize("mode", ["keyed", "instance"])
def test_distinct_checkpoint_and_restore_in_mid_stream(engine, mode):
    src, dst, val, h, planted = _dist(mode)
    n, half = len(src), len(src) // 2
    model, model_b = distinct_ref.DistinctState(mode), None
    with engine.distinct(mode) as a, engine.distinct(mode) as b:
        _dist_feed(a, model, mode, (src, dst, val), _cuts(half, [257]), h, planted, dev=True)
        es, ed = a.export()
        assert _rows((es, ed)) == model.log and len(model.log) > K
        b.load(es, ed)                             # the whole cluster claims its slots in one kernel
        _dist_evidence(mode, h, b.capacity()[0])
        assert b.capacity()[1] >= 3 and b.size() == (len(model.log), len(model.log)) and _rows(b.export()) == model.log
        model_b = copy.deepcopy(model)
        rest = _cuts(n - half, [257], half)
        _dist_feed(a, model, mode, (src, dst, val), rest, h, planted, dev=True)
        _dist_feed(b, model_b, mode, (src, dst, val), rest, h, planted, dev=True)
        assert model.log == model_b.log and _rows(a.export()) == model.log and _rows(b.export()) == model.log


# ---- WeightedMatchingState -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _match(upto=None):
    """(src, dst, val, clusters, events, M sorted, total weight) of the stream's first `upto` edges"""
    src, dst, val, clusters = ha.edge_stream(["tail"], 3000, repeats=300, weights=True)
    m = matching_ref.FastMatching()
    ev = m.edges(src[:upto].tolist(), dst[:upto].tolist(), val[:upto].tolist())
    return src, dst, val, clusters, ev, m.export(), m.total_weight()


def _events(cols, base):
    t, s, d, v, i = (_np(c).tolist() for c in cols)
    return [(a, b, c, e, f + base) for a, b, c, e, f in zip(t, s, d, v, i)]


def _edge_feed(call, ev, src, dst, cuts):
    """the batches through `call` (-> rows, the state's slot count), the evidence checked after every batch"""
    got = []
    for a, b in cuts:
        before = ev.counts()
        rows, slots = call(a, b)
        got += rows
        ev.see(src[a:b].tolist() + dst[a:b].tolist())
        ev.check(slots, before)
    return got


@pytest.mark.parametrize("cut", [None, 7])
def test_matching_with_partners_in_one_cluster(engine, cut):
    src, dst, val, clusters, want, M, w = _match()
    n = len(src)
    ev = Evidence(clusters)
    with engine.weighted_matching() as st:
        assert st.capacity() == (ha.INITIAL_SLOTS, 0)

        def call(a, b):
            return _events(st.edges(src[a:b], dst[a:b], val[a:b]), a), st.capacity()[0]
        got = _edge_feed(call, ev, src, dst, _cuts(n, [cut or n]))
        assert ev.counts() == [K] and st.capacity()[1] >= 3
        if cut:
            assert ev.grown_with >= K // 4        # growth in mid-stream: the rehash moved a cluster
        assert got == want
        assert st.size() == (len(M), n, w) and _rows(st.export()) == M


def test_matching_export_import_then_continue(engine):
    src, dst, val, clusters, want, M, w = _match()
    n, half = len(src), len(src) // 2
    head, M_half = _match(half)[4:6]
    with engine.weighted_matching() as a, engine.weighted_matching() as b:
        ev = Evidence(clusters)
        got = _edge_feed(lambda lo, hi: (_events(a.edges(src[lo:hi], dst[lo:hi], val[lo:hi]), lo), a.capacity()[0]),
                         ev, src, dst, _cuts(half, [64]))
        assert got == head
        cols = a.export()
        assert _rows(cols) == M_half
        b.import_(*cols)
        in_m = Evidence(clusters)
        in_m.see(_np(cols[0]).tolist() + _np(cols[1]).tolist())
        in_m.check(b.capacity()[0])
        assert in_m.counts()[0] > 200 and b.size() == (len(M_half), len(M_half), a.size()[2]) and _rows(b.export()) == M_half
        tail = [e for e in want if e[4] >= half]
        for st, e in ((a, ev), (b, in_m)):
            got = _edge_feed(lambda lo, hi: (_events(st.edges(src[lo:hi], dst[lo:hi], val[lo:hi]), lo), st.capacity()[0]),
                             e, src, dst, _cuts(n - half, [64], half))
            assert got == tail and _rows(st.export()) == M
        assert a.size() == (len(M), n, w) and b.size()[0::2] == (len(M), w)


# ---- AssignComponentsState -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _assign():
    src, dst, clusters = ha.edge_stream(["tail", "adjacent"], 3000)
    recs, ref = assign_ref.run(list(zip(src.tolist(), dst.tolist())))
    return src, dst, clusters, recs, sorted(ref.state().items())


def _records(cols, base=0):
    v, c, e = (_np(x).tolist() for x in cols)
    return [(a, b, i + base) for a, b, i in zip(v, c, e)]


@pytest.mark.parametrize("cut", [None, 7])
def test_assign_components_with_two_clusters(engine, cut):
    src, dst, clusters, want, rows = _assign()
    n = len(src)
    ev = Evidence(clusters)
    with engine.assign_components() as st:
        assert st.capacity() == (ha.INITIAL_SLOTS, 0)
        got = _edge_feed(lambda a, b: (_records(st.edges(src[a:b], dst[a:b]), a), st.capacity()[0]), ev, src, dst,
                         _cuts(n, [cut or n]))
        assert ev.counts() == [K, K] and st.capacity()[1] >= 3
        if cut:
            assert ev.grown_with >= K // 4
        assert got == want
        assert _rows(st.export()) == rows and st.size() == (len(rows), len({c for _, c in rows}), len(want))
        k, v = engine.components(src, dst)            # the window operator over the whole stream
        ek, evv = st.export()
        assert np.array_equal(ek, k) and np.array_equal(evv, v)


def _group_edges(rng, new, known, n):
    """n edges: a source among `new` (every new id at least once), a target among new and known ids"""
    s = np.concatenate([new, rng.choice(new, n - len(new))])
    d = rng.choice(np.concatenate([new, known]), n)
    return s.astype(np.int64), d.astype(np.int64)


def test_assign_refused_batches_leave_absent_slots_inside_the_cluster(engine, pkg):
    """A batch that does not fit its output is refused after its endpoints have claimed their slots: the slots
    stay claimed and outside the state, in the middle of the cluster, until the next doubling drops them.  Later
    batches probe past them, claim behind them, and the refused batch itself finds its own slots again."""
    tail = ha.cluster_ids("tail")
    rng = np.random.default_rng(0xA551)
    g = {"A": tail[:300], "B": tail[300:330], "C": tail[330:360], "D": tail[360:900], "E": tail[900:930],
         "F": tail[930:960], "G": tail[960:990]}
    batch = {}
    model = assign_ref.AssignFast()
    delivered = []

    def deliver(st, name):
        s, d = batch[name]
        want, _ = assign_ref.run(list(zip(s.tolist(), d.tolist())), model)
        assert _records(st.edges(s, d)) == want, name
        delivered.append((s, d))
        assert _rows(st.export()) == sorted(model.state().items()), name

    def refuse(st, name):
        s, d = batch[name]
        want, _ = assign_ref.run(list(zip(s.tolist(), d.tolist())), copy.deepcopy(model))
        assert len(want) > 1
        size = st.size()
        with pytest.raises(pkg.GsError) as err:
            st.edges(s, d, capacity=1)
        assert err.value.status == GS_ECAPACITY and st.last_records == len(want)
        assert st.size() == size and _rows(st.export()) == sorted(model.state().items()), name

    # targets reach back only to groups delivered (or, for G, at least claimed) before
    batch["A"] = _group_edges(rng, g["A"], np.empty(0, dtype=np.int64), 300)
    batch["B"] = _group_edges(rng, g["B"], g["A"], 30)
    batch["C"] = _group_edges(rng, g["C"], g["A"], 30)
    batch["D"] = _group_edges(rng, g["D"], np.concatenate([g["A"], g["B"], g["C"]]), 540)
    seen = np.concatenate([g[x] for x in "ABCD"])
    batch["E"] = _group_edges(rng, g["E"], seen, 30)
    batch["F"] = _group_edges(rng, g["F"], seen, 30)
    batch["G"] = _group_edges(rng, g["G"], np.concatenate([seen, g["E"], g["F"]]), 30)
    with engine.assign_components() as st:
        deliver(st, "A")
        slots = st.capacity()[0]
        assert ha.check_cluster("tail", g["A"], slots) == 300
        # before the next doubling: B's slots are claimed and absent, C probes past them, B comes back
        refuse(st, "B")
        deliver(st, "C")
        deliver(st, "B")
        refuse(st, "E")                             # E's slots stay behind, absent, when D doubles the table
        assert st.capacity()[0] == slots and ha.check_cluster("tail", tail[:390], slots) == 390
        deliver(st, "D")
        slots2, growths = st.capacity()
        assert slots2 > slots and ha.check_cluster("tail", tail[:930], slots2) == 930
        # after it: E again (its claims were dropped), and the same three steps in the larger table
        deliver(st, "E")
        refuse(st, "F")
        deliver(st, "G")
        deliver(st, "F")
        assert st.capacity()[0] == slots2
        rows = sorted(model.state().items())
        assert st.size()[:2] == (len(rows), len({c for _, c in rows}))
        s, d = np.concatenate([x for x, _ in delivered]), np.concatenate([y for _, y in delivered])
        k, v = engine.components(s, d)
        ek, evv = st.export()
        assert np.array_equal(ek, k) and np.array_equal(evv, v)


def test_assign_load_walks_past_absent_slots(engine, pkg):
    """a state whose first batch was refused is still empty, so it takes a checkpoint: the restore looks every
    label up (as_lookup) along a probe chain that starts with the refused batch's claimed, absent slots"""
    tail = ha.cluster_ids("tail")
    rng = np.random.default_rng(0xA552)
    refused, kept, later = tail[:600], tail[600:700], tail[700:760]
    rs, rd = _group_edges(rng, refused, np.empty(0, dtype=np.int64), 600)
    ks, kd = kept, np.repeat(kept[::4], 4)          # the checkpoint: 25 components of four vertices
    model = assign_ref.AssignFast()
    assign_ref.run(list(zip(ks.tolist(), kd.tolist())), model)
    rows = sorted(model.state().items())
    assert len(rows) == 100 and len({c for _, c in rows}) == 25
    with engine.assign_components() as st:
        with pytest.raises(pkg.GsError) as err:
            st.edges(rs, rd, capacity=1)
        assert err.value.status == GS_ECAPACITY and st.size() == (0, 0, 0) and _rows(st.export()) == []
        slots = st.capacity()[0]
        assert ha.check_cluster("tail", tail[:700], slots) == 700 and 2 * 700 <= slots
        st.load(np.array([v for v, _ in rows], dtype=np.int64), np.array([c for _, c in rows], dtype=np.int64))
        assert st.capacity()[0] == slots            # no doubling in between: the absent slots are still there
        assert _rows(st.export()) == rows and st.size() == (100, len({c for _, c in rows}), 0)
        ls, ld = _group_edges(rng, later, np.concatenate([kept, refused[:50]]), 120)
        want, _ = assign_ref.run(list(zip(ls.tolist(), ld.tolist())), model)
        assert _records(st.edges(ls, ld)) == want
        assert _rows(st.export()) == sorted(model.state().items())


# ---- TriangleSamplerState --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _warm(mode):
    """(the reference sampler after the warm-up, the records of the warm-up)"""
    st = trisample_ref.TriangleSamplerRef(mode, ha.TS_S, ha.TS_V, seed=ha.TS_SEED)
    rec = st.edges(*ha.trisample_warmup())
    return st, rec


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("mode", ["broadcast", "incidence"])
def test_triangle_sampler_with_decoys_of_its_wanted_pairs(engine, mode, aligned):
    warm, warm_rec = _warm(mode)
    ws, wd = ha.trisample_warmup()
    n = ha.TS_BATCH
    with engine.triangle_sampler(mode, ha.TS_S, ha.TS_V, ha.TS_SEED) as st:
        assert _rows(st.edges(_dev(ws), _dev(wd))) == warm_rec
        rows = st.export()[1]
        assert np.array_equal(rows, warm.rows())
        src, dst = ha.trisample_batch(rows, ha.TS_WARM, n, ha.TS_V)
        # the evidence, from the exported rows: decoys with the 64-bit hash of a pair wanted at batch start, and
        # decoys that pass the filter and land on a wanted pair's home slot with another key
        full, near = ha.count_decoys(rows, ha.TS_WARM, src, dst)
        assert full >= 32 and near >= 32, (full, near)
        off = 0 if aligned else 1                   # 16-byte aligned columns, or offset by one element
        S, D = torch.empty(n + 2, dtype=torch.int64, device="cuda"), torch.empty(n + 2, dtype=torch.int64, device="cuda")
        S, D = S[off:off + n], D[off:off + n]
        S.copy_(torch.from_numpy(np.array(src)))
        D.copy_(torch.from_numpy(np.array(dst)))
        assert (S.data_ptr() % 16 == 0) == aligned and (D.data_ptr() % 16 == 0) == aligned
        ref = copy.deepcopy(warm)
        want = ref.edges(src, dst)
        assert len(want) > 20
        assert _rows(st.edges(S, D)) == want
        hdr, after = st.export()
        assert np.array_equal(after, ref.rows())
        assert st.size() == (ha.TS_WARM + n, ref.beta_sum())
        assert (hdr["edges_seen"], hdr["beta_sum"], hdr["last_emitted"]) == (ha.TS_WARM + n, ref.beta_sum(), ref.previous)

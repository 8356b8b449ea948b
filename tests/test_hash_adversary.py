"""CPU: tests/hash_adversary.py -- the restated hashes invert, every constructor delivers the collision it names,
the restatement is pinned to the sources it restates, and every adversarial stream meets its preconditions when
run through its reference model alone (so test_gpu_hash_collisions.py compares against something non-trivial)."""
import copy
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import assign_ref
import continuous_ref
import distinct_ref
import hash_adversary as ha
import matching_ref
import trisample_ref

CSRC = Path(__file__).resolve().parent.parent / "gelly-streaming_amd" / "csrc"
I64_MIN, I64_MAX = ha.I64_MIN, ha.I64_MAX
EXTREME = [0, 1, -1, 2, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 1 << 32, (1 << 33) - 1, -(1 << 33)]


# ---- helper properties ---------------------------------------------------------------------------------------
def _fmix_plain(x):
    """the finaliser once more, on Python ints alone"""
    x &= ha.M64
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & ha.M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & ha.M64
    return x ^ (x >> 33)


def test_inverse_round_trip_on_random_and_extreme_values():
    rng = np.random.default_rng(0xADE5)
    x = np.concatenate([rng.integers(I64_MIN, I64_MAX, 20_000), np.array(EXTREME, dtype=np.int64)])
    h = ha.fmix64(x)
    assert h.dtype == np.uint64 and np.array_equal(ha.fmix64_inv(h), x)
    assert np.array_equal(ha.fmix64(ha.fmix64_inv(h)), h)
    assert len(np.unique(h)) == len(np.unique(x))
    for v in EXTREME + x[:200].tolist():
        assert ha.fmix64(v) == _fmix_plain(v) == int(ha.fmix64(np.array([v], dtype=np.int64))[0])
        assert ha.fmix64_inv(ha.fmix64(v)) == v and ha.fmix64(ha.fmix64_inv(v)) == v & ha.M64
    assert ha.fmix64(0) == 0 and ha.fmix64_inv(0) == 0          # the finaliser's fixed point


def test_pair_hash_and_its_inverse_in_b():
    rng = np.random.default_rng(0xADE6)
    a, b = rng.integers(I64_MIN, I64_MAX, 5000), rng.integers(I64_MIN, I64_MAX, 5000)
    h = ha.pair_hash(a, b)
    assert np.array_equal(ha.pair_with_hash(h, a), b)
    for x, y in zip(EXTREME, reversed(EXTREME)):
        want = _fmix_plain(_fmix_plain(x) ^ (y * 0x9E3779B97F4A7C15 & ha.M64))
        assert ha.pair_hash(x, y) == want and ha.pair_with_hash(want, x) == y
    target = rng.integers(0, 1 << 63, 5000).astype(np.uint64)
    assert np.array_equal(ha.pair_hash(a, ha.pair_with_hash(target, a)), target)


@pytest.mark.parametrize("value,bits", [(ha.TAIL, 24), (ha.MID, 24), (0, 24), (ha.SPLIT_VALUE, 6), (1, 1)])
def test_ids_with_low_bits(value, bits):
    ids = ha.ids_with_low_bits(value, bits, 5000)
    assert ids.dtype == np.int64 and len(set(ids.tolist())) == 5000 and -1 not in ids
    h = ha.fmix64(ids)
    slots = 1
    while slots <= 1 << bits:                       # one home for every power-of-two slot count up to 2^bits
        assert np.all(ha.home(h, slots) == value & (slots - 1))
        slots *= 2
    skipped = ha.ids_with_low_bits(value, bits, 100, skip=ids[:50])
    assert not set(skipped.tolist()) & set(ids[:50].tolist()) and len(set(skipped.tolist())) == 100


def test_ids_with_low_bits_never_returns_the_empty_word():
    """with 63 bits given there are two candidates, j = 0 and 1; for the low bits of ct_hash(-1) one of them is -1"""
    value = ha.fmix64(-1) & ((1 << 63) - 1)
    both = ha.ids_with_hash(np.array([value, (1 << 63) | value], dtype=np.uint64)).tolist()
    assert -1 in both
    ids = ha.ids_with_low_bits(value, 63, 1)
    assert ids.tolist() == [v for v in both if v != -1]
    assert ha.ids_with_low_bits(ha.fmix64(-1) & 0xFFF, 12, 100).tolist().count(-1) == 0


@pytest.mark.parametrize("ordered", [False, True])
def test_pairs_with_hash_of(ordered):
    for a0, b0 in [(3, 7), (-5, 1 << 40), (I64_MIN, I64_MAX), (0, 0)]:
        a, b = ha.pairs_with_hash_of(a0, b0, 200, ordered)
        pairs = set(zip(a.tolist(), b.tolist()))
        assert len(pairs) == 200 and (a0, b0) not in pairs
        assert np.all(ha.pair_hash(a, b) == ha.pair_hash(a0, b0))
        assert not ordered or np.all(a < b)


@pytest.mark.parametrize("home_bits", [24, 20, 6])
@pytest.mark.parametrize("ordered", [False, True])
def test_pairs_same_home_and_tag(home_bits, ordered):
    for a0, b0 in [(3, 7), (-5, 1 << 40), (I64_MIN, I64_MAX)]:
        a, b = ha.pairs_same_home_and_tag(a0, b0, 300, home_bits, ordered)
        h, h0 = ha.pair_hash(a, b), ha.pair_hash(a0, b0)
        assert len(set(zip(a.tolist(), b.tolist()))) == 300 and len(np.unique(h)) == 300
        assert np.all(h != h0) and np.all(ha.tag(h) == ha.tag(h0)) and np.all(ha.filter_bit(h) == ha.filter_bit(h0))
        slots = 1
        while slots <= 1 << home_bits:
            assert np.all(ha.home(h, slots) == ha.home(h0, slots))
            slots *= 2
        assert np.all((h ^ np.uint64(h0)) >> np.uint64(home_bits) << np.uint64(64 - ha.TAG_SHIFT + home_bits) != 0)
        assert not ordered or np.all(a < b)


def test_home_tag_and_filter_bit_are_the_bits_they_name():
    h = 0xFEDCBA9876543210
    assert ha.home(h, 64) == 0x10 and ha.home(h, 1 << 24) == 0x543210 and ha.home(h, 1) == 0
    assert ha.tag(h) == h >> 41 and ha.tag(h) < 1 << 23
    assert ha.filter_bit(h) == h >> 45 and ha.filter_bit(ha.M64) == (1 << 19) - 1
    arr = np.array([h, 1, ha.M64], dtype=np.uint64)
    assert ha.home(arr, 256).tolist() == [0x10, 1, 0xFF] and ha.tag(arr).tolist() == [h >> 41, 0, (1 << 23) - 1]


# ---- the restatement is pinned to the sources ------------------------------------------------------------------
CT_HASH_BODY = "x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x;"
PAIR_EXPR = "ct_hash(ct_hash((unsigned long long)A) ^ ((unsigned long long)B * 0x9e3779b97f4a7c15ull))"
SLOT_FROM_LOW_BITS = {                       # file -> (the mask's name, every way it takes a home slot from a hash)
    "gs_table.hpp": (r"mask", [r"ct_hash\(id\) & mask"]),
    "gs_distinct.hip": (r"t\.mask", [r"slot = h & t\.mask"]),
    "gs_trisample.hip": (r"t\.mask", [r"slot = \(uint32_t\)h & t\.mask"]),
}
ID_KEYED = ["gs_continuous.hip", "gs_matching.hip", "gs_assign.hip"]   # they probe through gs_table.hpp alone
WHO = "tests/hash_adversary.py restates this hash: change both, or its collision streams stop colliding"


def _norm(text):
    return re.sub(r"\s+", " ", text).strip()


def _function_body(text, head):
    """the whitespace-normalised body of the function whose signature matches `head`"""
    m = re.search(head + r"\s*\{", text)
    assert m, f"{head!r} not found -- {WHO}"
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return _norm(text[m.end():i - 1])


def source_pins(csrc):
    """[(what, found, expected)] for the sources under `csrc`: every line must have found == expected"""
    ops = (csrc / "gs_ops.hpp").read_text()
    ds = (csrc / "gs_distinct.hip").read_text()
    ts = (csrc / "gs_trisample.hip").read_text()
    pins = [("ct_hash body (gs_ops.hpp)", _function_body(ops, r"unsigned long long ct_hash\(unsigned long long x\)"), CT_HASH_BODY)]
    body = _function_body(ds, r"unsigned long long ds_hash\(int64_t s, int64_t d\)")
    pins.append(("ds_hash (gs_distinct.hip)", body,
                 "return KEYED ? " + PAIR_EXPR.replace("A", "s").replace("B", "d") + " : ct_hash((unsigned long long)d);"))
    body = _function_body(ts, r"unsigned long long ts_pair_hash\(int64_t a, int64_t b\)")
    pins.append(("ts_pair_hash (gs_trisample.hip)", body, "return " + PAIR_EXPR.replace("A", "a").replace("B", "b") + ";"))
    for name, text, want in (("DS_TAG_SHIFT", ds, ha.TAG_SHIFT), ("TS_FILTER_BITS", ts, ha.FILTER_BITS)):
        m = re.search(r"constexpr int " + name + r" = (\d+);", text)
        pins.append((name, int(m.group(1)) if m else None, want))
    pins.append(("ds_tag", _function_body(ds, r"unsigned long long ds_tag\(unsigned long long h\)"),
                 "return (h >> DS_TAG_SHIFT) << DS_TAG_SHIFT;"))
    pins.append(("the filter bit", len(re.findall(r"bit = \(uint32_t\)\(h >> \(64 - TS_FILTER_BITS\)\);", ts)), 2))
    for fname, (mask, patterns) in SLOT_FROM_LOW_BITS.items():
        text = (csrc / fname).read_text()
        masked = len(re.findall(r"(?<!\+ 1\) )& " + mask, text))      # every `& mask` that is not a probe's step
        found = sum(len(re.findall(p, text)) for p in patterns)
        pins.append((f"home slots from the low hash bits ({fname})", (found > 0, found), (True, masked)))
    for fname in ID_KEYED:
        masked = len(re.findall(r"(?<!\+ 1\) )& t\.mask", (csrc / fname).read_text()))
        pins.append((f"no home slot of its own: the probes are gs_table.hpp's ({fname})", masked, 0))
    return pins


def check_source_pins(csrc):
    for what, found, want in source_pins(csrc):
        assert found == want, f"{what}: found {found!r}, expected {want!r} -- {WHO}"


def test_restatement_is_pinned_to_the_sources():
    check_source_pins(CSRC)
    assert ha.C1 == 0xff51afd7ed558ccd and ha.C2 == 0xc4ceb9fe1a85ec53 and ha.GOLDEN == 0x9e3779b97f4a7c15
    assert ha.C1 * ha.C1_INV & ha.M64 == 1 and ha.C2 * ha.C2_INV & ha.M64 == 1 and ha.GOLDEN * ha.GOLDEN_INV & ha.M64 == 1


@pytest.mark.parametrize("fname,old,new", [
    ("gs_ops.hpp", "x *= 0xc4ceb9fe1a85ec53ull;", "x *= 0xc4ceb9fe1a85ec55ull;"),
    ("gs_ops.hpp", "  x ^= x >> 33;\n  return x;", "  x ^= x >> 32;\n  return x;"),
    ("gs_distinct.hip", "(unsigned long long)d * 0x9e3779b97f4a7c15ull", "(unsigned long long)d * 0x9e3779b97f4a7c17ull"),
    ("gs_trisample.hip", "(unsigned long long)b * 0x9e3779b97f4a7c15ull", "(unsigned long long)b * 0x9e3779b97f4a7c13ull"),
    ("gs_distinct.hip", "DS_TAG_SHIFT = 41;", "DS_TAG_SHIFT = 40;"),
    ("gs_trisample.hip", "TS_FILTER_BITS = 19;", "TS_FILTER_BITS = 18;"),
    ("gs_table.hpp", "unsigned long long s = ct_hash(id) & mask;", "unsigned long long s = (ct_hash(id) >> 7) & mask;"),
    ("gs_matching.hip", "  return (uint32_t)tab_claim<sizeof(MtSlot) / 8>(&t.slots->id, t.mask, id, fresh);",
     "  unsigned long long s = ct_hash(id) & t.mask;\n  return (uint32_t)s;"),
    ("gs_distinct.hip", "slot = h & t.mask", "slot = (h >> 20) & t.mask"),
])
def test_an_edited_copy_of_the_sources_fails_the_pin(tmp_path, fname, old, new):
    for f in ["gs_ops.hpp"] + list(SLOT_FROM_LOW_BITS) + ID_KEYED:
        text = (CSRC / f).read_text()
        if f == fname:
            assert old in text
            text = text.replace(old, new)
        (tmp_path / f).write_text(text)
    with pytest.raises(AssertionError, match="hash_adversary.py"):
        check_source_pins(tmp_path)


# ---- the streams, through their reference models alone -----------------------------------------------------------
K = ha.K


def test_cluster_size_spans_several_workgroups():
    assert K >= 512          # two 256-lane workgroups at the least


@pytest.mark.parametrize("name", ha.ID_SETS)
def test_id_sets_collide_as_named(name):
    ids = ha.cluster_ids(name)
    assert len(ids) == K and len(set(ids.tolist())) == K and -1 not in ids
    slots = ha.INITIAL_SLOTS
    while slots <= 1 << 16:
        top = ha.check_cluster(name, ids, slots)
        if name in ("tail", "one_home"):
            assert top == K
        elif name == "adjacent":
            assert top == K - K // 2
        else:
            assert (top == K) == (slots == ha.INITIAL_SLOTS) and top * slots >= K * ha.INITIAL_SLOTS
        slots *= 2
    if name == "splits":         # one cluster in the first table, two halves after the first doubling, and so on
        homes = [len(np.unique(ha.home(ha.fmix64(ids), s))) for s in (64, 128, 256, 4096)]
        assert homes == [1, 2, 4, 64]
    pool, clusters = ha.single_id_pool([name])
    assert {-1, I64_MIN, I64_MAX} <= set(pool.tolist()) and len(pool) >= K + 300 and np.array_equal(clusters[name], ids)


@pytest.mark.parametrize("name", ha.ID_SETS)
def test_continuous_stream_preconditions(name):
    src, dst, cluster = ha.continuous_stream(name)
    for direction in (continuous_ref.ALL, continuous_ref.OUT):
        m = continuous_ref.DegreeState()
        rows = m.degrees(src.tolist(), dst.tolist(), direction)
        per = 6 if direction == continuous_ref.ALL else 3
        assert all(m.counts[v] == per for v in cluster.tolist())        # every cluster id recurs
        assert len(m.counts) >= K + 303 and max(c for _, c in rows) == per
    v = continuous_ref.DegreeState().vertices(src.tolist(), dst.tolist())
    assert set(cluster.tolist()) <= {x for x, _ in v} and [c for _, c in v] == list(range(1, len(v) + 1))
    if name == "splits":        # the first 16 edges fit the first table and put one cluster into it
        first = set(src[:16].tolist()) | set(dst[:16].tolist())
        inside = [x for x in first if x in set(cluster.tolist())]
        assert len(first) <= ha.INITIAL_SLOTS // 2 and ha.check_cluster(name, inside, ha.INITIAL_SLOTS) == len(inside) >= 20
        assert len(set(src[:16].tolist()) & set(cluster.tolist())) >= 8          # and under OUT, the sources alone


@pytest.mark.parametrize("mode", ["keyed", "instance"])
def test_distinct_stream_preconditions(mode):
    src, dst, val, groups = ha.distinct_stream(mode)
    assert sorted(groups) == (["a", "b", "c", "fill"] if mode == "keyed" else ["a", "b", "fill"])
    h = {g: ha.distinct_key_hash(mode, *groups[g]) for g in groups}
    key = (lambda s, d: (s, d)) if mode == "keyed" else (lambda s, d: d)
    keys = {g: [key(s, d) for s, d in zip(groups[g][0].tolist(), groups[g][1].tolist())] for g in groups}
    planted = [k for g in sorted(groups) if g != "fill" for k in keys[g]]
    assert len(set(planted)) == len(planted) == K + 301 + (65 if mode == "keyed" else 0)
    # a: one home (the last slot of every table), every tag different
    assert len(h["a"]) == K and np.all(ha.home(h["a"], 1 << 24) == ha.TAIL) and len(np.unique(ha.tag(h["a"]))) == K
    # b: the same home, one tag -- that of a's key 4 -- and different hashes
    assert len(h["b"]) == 301 and np.all(ha.home(h["b"], 1 << 24) == ha.TAIL) and len(np.unique(h["b"])) == 301
    assert set(ha.tag(h["b"]).tolist()) == {5} and int(ha.tag(h["a"])[4]) == 5
    if mode == "keyed":         # c: one 64-bit hash for 65 different pairs
        assert len(h["c"]) == 65 and len(np.unique(h["c"])) == 1 and ha.home(int(h["c"][0]), 1 << 24) == ha.MID
    # every planted key stands four times; the model lets the first through and drops the other three
    st = distinct_ref.DistinctState(mode)
    out = st.edges(src.tolist(), dst.tolist(), val.tolist())
    stream_keys = [key(s, d) for s, d in zip(src.tolist(), dst.tolist())]
    count = {}
    for k in stream_keys:
        count[k] = count.get(k, 0) + 1
    assert all(count[k] == 4 for k in planted)
    assert len(out) == len(count) and len(src) - len(out) >= 3 * len(planted)
    first = {}
    for i, k in enumerate(stream_keys):
        first.setdefault(k, i)
    assert [r[3] for r in out] == sorted(first.values()) and [r[2] for r in out] == [r[3] for r in out]
    # duplicates inside one batch of 257 and across batches, both
    pos = {}
    for i, k in enumerate(stream_keys):
        pos.setdefault(k, []).append(i // 257)
    same = sum(len(set(pos[k])) < 4 for k in planted)
    assert same > 100 and sum(len(set(pos[k])) > 1 for k in planted) > len(planted) - 10
    if mode == "instance":      # the copies of a target carry different sources: only the target is the key
        by_dst = {}
        for s, d in zip(src.tolist(), dst.tolist()):
            by_dst.setdefault(d, set()).add(s)
        assert sum(len(by_dst[d]) > 1 for d in keys["a"]) > K - 20


def test_matching_stream_preconditions():
    src, dst, val, clusters = ha.edge_stream(["tail"], 3000, repeats=300, weights=True)
    ends = set(src.tolist()) | set(dst.tolist())
    assert set(clusters["tail"].tolist()) <= ends and {-1, I64_MIN, I64_MAX} <= ends
    assert 0 <= int(val.min()) and int(val.max()) < 1 << 16
    edges = list(zip(src.tolist(), dst.tolist()))
    assert len(edges) - len(set(edges)) >= 300
    m = matching_ref.FastMatching()
    ev = m.edges(src.tolist(), dst.tolist(), val.tolist())
    adds, removes = sum(e[0] == matching_ref.ADD for e in ev), sum(e[0] == matching_ref.REMOVE for e in ev)
    assert adds > 500 and removes > 100 and m.is_matching()
    cluster = set(clusters["tail"].tolist())
    assert sum(s in cluster and d in cluster for s, d, _ in m.M) > 200      # partners inside one cluster


def test_assign_stream_preconditions():
    src, dst, clusters = ha.edge_stream(["tail", "adjacent"], 3000)
    ends = set(src.tolist()) | set(dst.tolist())
    for name in ("tail", "adjacent"):
        assert set(clusters[name].tolist()) <= ends
    recs, ref = assign_ref.run(list(zip(src.tolist(), dst.tolist())))
    labels = set(ref.state().values())
    assert len(ref.state()) == len(ends) == 2 * K + 303 and 1 < len(labels) < 400
    assert len(recs) > 3 * len(ends)                 # components merge and are relabelled again and again


TS_S, TS_V, TS_WARM, TS_BATCH = ha.TS_S, ha.TS_V, ha.TS_WARM, ha.TS_BATCH


@functools.lru_cache(maxsize=None)
def warm_sampler(mode):
    """the reference sampler after the warm-up (copy it before feeding it more)"""
    st = trisample_ref.TriangleSamplerRef(mode, TS_S, TS_V, seed=ha.TS_SEED)
    st.edges(*ha.trisample_warmup())
    return st


@pytest.mark.parametrize("mode", ["broadcast", "incidence"])
def test_trisample_batch_preconditions(mode):
    warm = warm_sampler(mode)
    rows = warm.rows()
    want = ha.wanted_pairs(rows, TS_WARM, TS_BATCH)
    assert len({i for i, _, _ in want}) > 100
    src, dst = ha.trisample_batch(rows, TS_WARM, TS_BATCH, TS_V)
    full, near = ha.count_decoys(rows, TS_WARM, src, dst)
    assert full >= 32 and near >= 32
    st = copy.deepcopy(warm)
    rec = st.edges(src, dst)
    assert len(rec) > 20 and st.beta_sum() > warm.beta_sum() + 20            # the planted wanted edges close triangles
    assert 0 < np.sum(st.rows()[:, ha.TSR_J] != rows[:, ha.TSR_J]) < TS_S // 2   # a few replacements inside the batch

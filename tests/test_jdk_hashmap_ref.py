"""CPU: the independent java.util.HashMap<Long> model (tests/jdk_hashmap_ref.py), the paper answers that hold it,
and the oracle's hashset_order held to the model.

WindowTriangles reads HashSet<Long>.toArray(), so the oracle (oracle/gs_oracle.c) and the kernels (gs_hashset.hip)
both restate HashMap; every GPU test compares the two, and both came from one reading.  Here a second restatement
over linked objects is pinned by answers derived on paper and by the red-black and list invariants after every
put, and then the oracle must equal it, order and flags, over families of id sets built to leave the plain-bin
model -- most of them with tree bins whose hashes have both signs, where `(ph = p.hash) > h` being a signed
compare decides the tree, and through putTreeVal's link position and moveRootToFront the iteration order.
(Before j_dir compared signed, the oracle differed from the model on exactly the families marked `mixed`
below and equalled it on the rest.)  tests/test_gpu_jdk_order.py then holds the kernels to the same model."""
import numpy as np
import pytest
from jdk_hashmap_ref import (FLAG_COLLISION_RESIZE, FLAG_TREEIFIED, build, candidate_records, check_invariants,
                             hashset_order, java_hash)

B31, B63 = 1 << 31, 1 << 63
CHECK_EVERY_PUT_UP_TO = 400   # check_invariants walks the whole map: after every put on the smaller sets only


def _signed_family_11():
    return [(j << 6) | ((j & 1) << 31) for j in range(1, 12)]


def _bit63_family(n):
    return [(j << 6) - ((j & 1) << 63) for j in range(1, n + 1)]


def test_java_hash_is_a_signed_int():
    """Long.hashCode folds the high word in, HashMap.hash folds the high half in, both ints: bit 31 of the hash
    is bit 31 xor bit 63 of the id."""
    assert java_hash(0) == 0 and java_hash(64) == 64 and java_hash(1 << 16) == (1 << 16) | 1
    assert java_hash(B31 | 64) == -B31 + 0x8000 + 64          # bit 31: negative
    assert java_hash(64 - B63) == -B31 + 0x8000 + 64          # bit 63 folds onto bit 31
    assert java_hash((B31 | 64) - B63) == 64                  # both: positive again
    assert java_hash(-1) == 0                                 # 0xFFFFFFFF ^ 0xFFFFFFFF
    assert java_hash(1 << 32) == 1


def test_model_known_answers_plain_and_unsigned_free():
    """The three answers of test_oracle_golden.test_hashset_exact_known_answers, derived there from the JDK's
    method bodies; all hashes are non-negative, so they do not see the sign:
     - 16, 32, .., 144 sit in bucket 0 of 16; the 9th add walks 8 nodes (binCount 7) and calls treeifyBin, which
       below capacity 64 resizes to 32: evens (hash & 16 == 0) stay in bin 0, odds go to bin 16, in order;
     - eight of them stay one list bin;
     - 64, .., 704 sit in bucket 0 at 16, 32 and 64: the 9th and 10th adds resize, the 11th treeifies.  Ascending
       red-black inserts of 1..11, each new key the right child of the last (R red, B black):
         3   parent 2 red, uncle null: 2B 1R rotateLeft(1)                 -> 2B(1R,3R)
         4   uncle 1 red: recolour, root black again                       -> 2B(1B,3B(-,4R))
         5   uncle null: 4B 3R rotateLeft(3)                               -> 2B(1B,4B(3R,5R))
         6   uncle 3 red: 3B 5B 4R, and 4's parent is black                -> 2B(1B,4R(3B,5B(-,6R)))
         7   uncle null: 6B 5R rotateLeft(5)                               -> 2B(1B,4R(3B,6B(5R,7R)))
         8   uncle 5 red: 5B 7B 6R, x = 6; parent 4 red, uncle 1 black: 4B 2R rotateLeft(2)
                                                                           -> 4B(2R(1B,3B),6R(5B,7B(-,8R)))
         9   uncle null: 8B 7R rotateLeft(7);  10  uncle 7 red, then uncle 2 red: recolour up to the root;
         11  uncle null: rotateLeft(9).  The root stays 4
       = key 256, which moveRootToFront unlinks and puts first; the rest keep the list order."""
    assert hashset_order([16 * j for j in range(1, 10)]) == ([32, 64, 96, 128, 16, 48, 80, 112, 144], 2)
    assert hashset_order([16 * j for j in range(1, 9)]) == ([16 * j for j in range(1, 9)], 0)
    assert hashset_order([64 * j for j in range(1, 12)]) == ([256, 64, 128, 192] + [64 * j for j in range(5, 12)], 3)
    assert hashset_order([5, 5, 3, 5, 3]) == ([3, 5], 0)      # HashSet.add of a present key changes nothing


def test_model_known_answer_bit31_signed():
    """ids (j << 6) | ((j & 1) << 31), j = 1..11.  Even j: hash 64 j.  Odd j: x = 2^31 + 64 j, x >>> 16 =
    0x8000 + (j >> 10), so hash = 2^31 + 0x8000 + 64 j as bits = -2^31 + 32768 + 64 j as an int.  All are
    multiples of 64: bucket 0 at capacities 16, 32 and 64.  The 9th add (binCount 7) and the 10th (binCount 8)
    call treeifyBin below 64: resize to 32, then 64 (flag 2), the bin whole and in order; the 11th treeifies it
    (flag 1) in list order j = 1..11.

    Signed, the odd j sort first: o1 < o3 < o5 < o7 < o9 < o11 < e2 < e4 < e6 < e8 < e10, ranks 1..11, and the
    list order inserts ranks 1 7 2 8 3 9 4 10 5 11 6 (R red, B black):
      1        1B
      7        1B(-,7R)
      2        left of 7; parent red, uncle (1.left) null, x a left child of a right child: rotateRight(7),
               rotateLeft(1)                                        -> 2B(1R,7R)
      8        right of 7; uncle 1 red: recolour, root black again     -> 2B(1B,7B(-,8R))
      3        left of 7, parent black                                 -> 2B(1B,7B(3R,8R))
      9        right of 8; uncle 3 red: 3B 8B 7R, then 7's parent is black -> 2B(1B,7R(3B,8B(-,9R)))
      4        right of 3, parent black                                -> .. 3B(-,4R)
      10       right of 9; uncle null, outer child: 9B 8R rotateLeft(8)  -> .. 7R(3B(-,4R),9B(8R,10R))
      5        right of 4; uncle null, outer child: 4B 3R rotateLeft(3)  -> .. 7R(4B(3R,5R),9B(8R,10R))
      11       right of 10; uncle 8 red: 8B 10B 9R, x = 9; parent 7 red, uncle 1 black, outer child: 7B 2R
               rotateLeft(2)                       -> 7B(2R(1B,4B(3R,5R)),9R(8B,10B(-,11R)))
      6        right of 5; uncle 3 red: 3B 5B 4R, x = 4; parent 2 red, uncle 9 red: 9B 2B 7R, x = 7 = root: black
    Root: rank 7 = e2 = 128.  moveRootToFront takes it from second place to the front; the list is otherwise the
    insertion order: 128, o1, o3, e4, o5, ...

    Unsigned, the evens sort first and the same inserts are ranks 6 1 7 2 8 3 9 4 10 5 11, whose root is rank 6
    = o1, already first: insertion order unchanged.  The model's unsigned switch shows that reading."""
    ids = _signed_family_11()
    want = [128, 2147483712, 2147483840, 256, 2147483968, 384, 2147484096, 512, 2147484224, 640, 2147484352]
    assert hashset_order(ids) == (want, 3)
    assert hashset_order(ids, signed=False) == (ids, 3)


# the second paper answer: eleven keys as above with the sign from bit 63, then two putTreeVal inserts
BIT63_ANSWER_IDS = _bit63_family(11) + [128 - B63, 576]
BIT63_ANSWER = [128, 64 - B63, 128 - B63, 192 - B63, 256, 320 - B63, 384, 448 - B63, 512, 576 - B63, 640, 576,
                704 - B63]


def test_model_known_answer_bit63_signed():
    """ids 64 j - ((j & 1) << 63), j = 1..11, then 128 - 2^63, then 576.  For odd j, x >>> 32 = 0x80000000, so
    Long.hashCode = 2^31 + 64 j and the hash is the one of the bit-31 answer: -2^31 + 32768 + 64 j.  The first
    eleven adds therefore repeat that derivation: two collision resizes, treeify at 64, root e2.  Its last tree
    7B(2B(1B,4R(3B,5B(-,6R))),9B(8B,10B(-,11R))), written by key (ranks 1..6 are o1 o3 o5 o7 o9 o11, ranks 7..11
    are e2 e4 e6 e8 e10), is
        e2B( o3B(o1B, o7R(o5B, o9B(-,o11R))), e6B(e4B, e8B(-,e10R)) )
    and the list is e2 o1 o3 e4 o5 e6 o7 e8 o9 e10 o11.
      12th  n = 128 - 2^63: hash -2^31 + 32768 + 128, between o1 and o3.  putTreeVal from the root: < e2, < o3,
            > o1: right child of o1, linked right after o1 in the list (mid-list); o1 is black: no rebalancing,
            the root stays.
      13th  p = 576: hash 576, between e8 (512) and e10 (640): > e2, > e6, > e8, < e10: left child of e10, linked
            right after e10, before o11.  Parent e10 red, uncle (e8.left) null, inner child: rotateRight(e10),
            then p black, e8 red, rotateLeft(e8): e6.right = pB(e8R,e10R).  The root stays.
    Order: e2 o1 n o3 e4 o5 e6 o7 e8 o9 e10 p o11.  Unsigned, n and every o sort above the evens, so n hangs
    elsewhere and the order differs."""
    assert hashset_order(BIT63_ANSWER_IDS) == (BIT63_ANSWER, 3)
    assert hashset_order(BIT63_ANSWER_IDS, signed=False)[0] != BIT63_ANSWER


# ---- families ---------------------------------------------------------------------------------------------
SIZES = (9, 40, 200, 1500, 6000)


def _orders(ids, rng):
    ids = np.asarray(ids, dtype=np.int64)
    return [("asc", ids), ("desc", ids[::-1]), ("shuffled", rng.permutation(ids))]


def _shift_family(s, variant):
    def gen():
        rng = np.random.default_rng(1000 * s + len(variant))
        for k in SIZES:
            ids = np.arange(1, k + 1, dtype=np.int64) << s
            half = rng.random(k) < 0.5
            if variant == "bit63":
                ids = np.where(half, ids ^ np.int64(-B63), ids)
            elif variant == "bit31":
                # set on a random half; j << s may hold bit 31 itself, so two j can meet: keep the first
                ids = np.where(half, ids | np.int64(B31), ids)
                ids = ids[np.sort(np.unique(ids, return_index=True)[1])]
            assert len(np.unique(ids)) == len(ids) and len(ids) >= k // 2   # at most one of each pair is lost
            # all three orders up to 1500 keys; the 6000-key sets shuffled (the others add run time, no path)
            for name, o in _orders(ids, rng):
                if k <= 1500 or name == "shuffled":
                    yield f"{k}-{name}", o
    return gen


def _one(ids):
    return lambda: iter([("set", np.asarray(ids, dtype=np.int64))])


def _hub_groups():
    rng = np.random.default_rng(41)
    for crowd, spread in ((4000, 6000), (300, 60), (2500, 100)):
        ids = np.concatenate([np.arange(1, crowd + 1, dtype=np.int64) << 24,
                              rng.integers(1, 1 << 40, spread).astype(np.int64),
                              -rng.integers(1, 1 << 62, spread).astype(np.int64)])
        yield f"{crowd}+{spread}", rng.permutation(np.unique(ids))


def _thresholds():
    # the size thresholds 12, 48, 192, 384 (3C/4 of 16, 64, 256, 512): one key below, at, and two above; the ids
    # crowd bucket 0 with both hash signs, so trees exist from the 11th key on
    for k in (11, 12, 13, 14, 47, 48, 49, 50, 191, 192, 193, 194, 383, 384, 385, 386):
        j = np.arange(1, k + 1, dtype=np.int64)
        yield f"{k}", np.where(j & 1, (j << 24) | np.int64(-B63), j << 24)


def _flag2_only():
    # nine keys in one bin at capacity 16 (ids 16 j) or at 32 (thirteen spread keys first, then ids 32 j), spread
    # before the bin can reach nine again: a collision resize and no tree
    yield "cap16", np.array([16 * j for j in range(1, 10)] + [3, 5, 7], dtype=np.int64)
    yield "cap32", np.array(list(range(1, 14)) + [32 * j for j in range(1, 10)], dtype=np.int64)
    yield "cap16-then-32", np.array([16 * j for j in range(1, 10)] + [32 * j + 1 for j in range(9)], dtype=np.int64)


_rng20 = np.random.default_rng(20)
FAMILIES = {   # name -> (generator of (label, ids), some tree bin holds both hash signs)
    "table-64j": (_one([64 * j for j in range(1, 12)]), False),
    "table-j20-2047": (_one([j << 20 for j in range(1, 2048)]), False),
    "table-j24-200": (_one([j << 24 for j in range(1, 201)]), True),
    "table-j20-3000": (_one([j << 20 for j in range(1, 3001)]), True),
    "table-j20-3000-permuted": (_one(_rng20.permutation([j << 20 for j in range(1, 3001)])), True),
    "table-bit31-11": (_one(_signed_family_11()), True),
    "table-bit63-39": (_one(_bit63_family(39)), True),
    "hub-groups": (_hub_groups, True),
    "thresholds": (_thresholds, True),
    "flag2-only": (_flag2_only, False),
}
for _s in (16, 20, 24, 28):
    for _v in ("plain", "bit63", "bit31"):
        # j << 16 hashes to (j << 16) ^ j: spread over the buckets, never a tree
        FAMILIES[f"shift{_s}-{_v}"] = (_shift_family(_s, _v), _s != 16)


@pytest.fixture(scope="module")
def family_sets():
    """Every family's sets and their models, built once for the tests below (the models are not modified)."""
    out = {}
    for name, (gen, _) in FAMILIES.items():
        sets = []
        for label, ids in gen():
            m = build(ids.tolist(), check_every_put=len(ids) <= CHECK_EVERY_PUT_UP_TO)
            check_invariants(m)
            sets.append((label, ids, m))
        out[name] = sets
    return out


def test_at_least_half_of_the_families_have_mixed_sign_tree_bins():
    mixed = [name for name, (_, mx) in FAMILIES.items() if mx]
    assert 2 * len(mixed) >= len(FAMILIES), (len(mixed), len(FAMILIES))


@pytest.mark.parametrize("name", list(FAMILIES))
def test_oracle_equals_model(oracle, family_sets, name):
    """oracle.hashset_order == the model, order and flags, on every set of the family; and the family has (or has
    not) a tree bin that compared hashes of different sign, as the table above says -- from the model, so the
    families cannot quietly lose their point."""
    saw_mixed = False
    for label, ids, m in family_sets[name]:
        ex, _, flags = oracle.hashset_order(ids)
        assert flags == m.flags, (name, label)
        assert ex.tolist() == m.keys(), (name, label)
        saw_mixed |= m.mixed_sign_compares > 0
        assert (m.mixed_sign_tree_bins() > 0) <= (m.mixed_sign_compares > 0)
    assert saw_mixed == FAMILIES[name][1], name


def test_flag2_family_has_no_tree(family_sets):
    for label, ids, m in family_sets["flag2-only"]:
        assert m.flags == FLAG_COLLISION_RESIZE, label
    assert [m.capacity() for _, _, m in family_sets["flag2-only"]] == [32, 64, 64]


def test_table_sets_separate_the_readings(family_sets):
    """The issue's table: the unsigned reading gives another order on exactly the five mixed-sign sets, and
    another LAST element (which the self-pair term skips) on two of them."""
    last_differs = []
    for name in [n for n in FAMILIES if n.startswith("table-")]:
        (_, ids, m), = family_sets[name]
        unsigned = build(ids.tolist(), signed=False)
        check_invariants(unsigned)
        assert (unsigned.keys() != m.keys()) == FAMILIES[name][1], name
        if unsigned.keys()[-1] != m.keys()[-1]:
            last_differs.append((name, unsigned.keys()[-1], m.keys()[-1]))
    assert last_differs == [("table-j24-200", 3338665984, 2130706432), ("table-j20-3000", 2951741440, 2683305984)]


# ---- the plain-bin claim of k_hs_detect ----------------------------------------------------------------------
def _plain_capacity(k):
    cap = 16
    while k > cap // 4 * 3:
        cap <<= 1
    return cap


def stage_rule_fires(ids):
    """The rule in gs_hashset.hip above k_hs_first: stage capacity C = 16, 32, .., final holds the first
    min(k, 3C/4 + 1) distinct arrivals (all k at the final stage); the set is complex iff some bucket
    hash & (C - 1) of some stage reaches 9."""
    k = len(ids)
    if k < 9:
        return False
    h = np.array([java_hash(int(x)) for x in ids], dtype=np.int64) & 0xFFFFFFFF
    capf = _plain_capacity(k)
    C = 16
    while C <= capf:
        n_c = k if C == capf else 3 * C // 4 + 1
        if np.bincount(h[:n_c] & (C - 1), minlength=C).max() >= 9:
            return True
        C <<= 1
    return False


def ids_plain(ids):
    """Final capacity from the size alone, buckets ascending, arrival order inside a bucket."""
    cap = _plain_capacity(len(ids))
    b = np.array([java_hash(int(x)) & (cap - 1) for x in ids], dtype=np.int64)
    return [int(ids[i]) for i in np.argsort(b, kind="stable")]


def test_plain_bin_claim_of_the_detector(family_sets):
    """flags == 0 <=> the stage-counter rule stays silent, and then the model's order is the plain one; over every
    family set, over every prefix of the small ones (so the sizes just below the first bin of 9 are there), and
    over random spread sets."""
    cases = [(f"{name}/{label}", ids) for name, sets in family_sets.items() for label, ids, _ in sets]
    cases += [(f"{c}[:{n}]", ids[:n]) for c, ids in list(cases) if len(ids) <= 50 for n in range(1, len(ids))]
    rng = np.random.default_rng(23)
    for k in (1, 8, 9, 12, 13, 100, 1000, 5000):
        cases.append((f"random-{k}", rng.permutation(np.unique(rng.integers(-(1 << 62), 1 << 62, k)))))
    for k in (30, 100, 400):   # crowded enough that some fire and some do not
        for t in range(8):
            cases.append((f"crowded-{k}-{t}", rng.permutation(np.unique(rng.integers(0, 5 * k, k))) * 4))
    plain = fired = 0
    for label, ids in cases:
        order, flags = hashset_order(ids.tolist())
        assert stage_rule_fires(ids) == (flags != 0), label
        if flags == 0:
            assert order == ids_plain(ids), label
            plain += 1
        else:
            assert flags & (FLAG_TREEIFIED | FLAG_COLLISION_RESIZE) == flags
            fired += 1
    assert plain >= 20 and fired >= 20, (plain, fired)


def test_candidate_records_equal_the_oracle(oracle):
    """The model's restatement of GenerateCandidateEdges (jdk_hashmap_ref.candidate_records, the expectation of
    tests/test_gpu_jdk_order.py) and the oracle's agree record for record: vertex order, arrival order with
    multi-edges and self-loops, the filter, the missing last self pair; plain windows and crowded ones."""
    rng = np.random.default_rng(91)
    for trial in range(24):
        V, n = int(rng.integers(3, 60)), int(rng.integers(1, 500))
        s, d = rng.integers(-V, V, n).astype(np.int64), rng.integers(-V, V, n).astype(np.int64)
        if trial % 3 == 1:
            s, d = s * 65537, d * 65537
        elif trial % 3 == 2:   # crowded buckets with both hash signs: trees
            s, d = np.where(s & 1, (s << 24) ^ np.int64(-B63), s << 24), np.where(d & 1, (d << 24) ^ np.int64(-B63), d << 24)
        ra, rb, rf, flags = oracle.window_candidates(s, d)
        wa, wb, wf, wflags = candidate_records(s, d)
        assert flags == wflags, trial
        assert np.array_equal(ra, wa) and np.array_equal(rb, wb) and np.array_equal(rf, wf), trial

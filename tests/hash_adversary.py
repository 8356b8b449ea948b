"""Constructed hash collisions for the device-resident tables (a plain module, like valcheck.py).

Five operators keep a linear-probing table in HBM and take the home slot from the low bits of one function:
ct_hash (gs_ops.hpp), the murmur3 64-bit finaliser.  The pair tables (gs_distinct.hip KEYED, gs_trisample.hip)
hash ct_hash(ct_hash(a) ^ b * GOLDEN).  The finaliser is a bijection -- x ^= x >> 33 undoes itself and the two
odd multipliers have inverses mod 2^64 -- and the pair mix is linear in b, so ids and pairs with any wanted hash
are computed, not searched for.  This module restates the hashes and their inverses; test_hash_adversary.py
pins the restatement to the sources.

Every function takes Python ints or NumPy integer arrays (any mix of signed ids and unsigned hashes, taken
mod 2^64).  Hashes come back unsigned (int or uint64 array), ids signed (int or int64 array).
"""
import numpy as np

M64 = (1 << 64) - 1
C1 = 0xFF51AFD7ED558CCD
C2 = 0xC4CEB9FE1A85EC53
GOLDEN = 0x9E3779B97F4A7C15
C1_INV = pow(C1, -1, 1 << 64)
C2_INV = pow(C2, -1, 1 << 64)
GOLDEN_INV = pow(GOLDEN, -1, 1 << 64)
TAG_SHIFT = 41       # gs_distinct.hip DS_TAG_SHIFT: a slot word's tag is hash bits 41..63
FILTER_BITS = 19     # gs_trisample.hip TS_FILTER_BITS: the filter bit is the hash's top 19 bits
HOME_BITS = 24       # the constructors' default: equal homes for every table of up to 2^24 slots


def _u64(x):
    """x mod 2^64 as a uint64 array (0-d for a scalar)"""
    if isinstance(x, (int, np.integer)):
        return np.array(int(x) & M64, dtype=np.uint64)
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return a
    if a.dtype == np.int64:
        return a.view(np.uint64)
    return np.array([int(v) & M64 for v in a.ravel().tolist()], dtype=np.uint64).reshape(a.shape)


def _unsigned(a, like):
    return int(a) if np.ndim(like) == 0 and np.ndim(a) == 0 else a


def _signed(a):
    a = np.asarray(a, dtype=np.uint64)
    return int(a.astype(np.int64)) if a.ndim == 0 else a.view(np.int64)


def _mul(x, c):
    with np.errstate(over="ignore"):
        return x * np.uint64(c)


def _fmix(x):
    x = x ^ (x >> np.uint64(33))
    x = _mul(x, C1)
    x = x ^ (x >> np.uint64(33))
    x = _mul(x, C2)
    return x ^ (x >> np.uint64(33))


def _fmix_inv(y):
    y = y ^ (y >> np.uint64(33))
    y = _mul(y, C2_INV)
    y = y ^ (y >> np.uint64(33))
    y = _mul(y, C1_INV)
    return y ^ (y >> np.uint64(33))


def fmix64(x):
    """ct_hash: the hash (unsigned) of an id"""
    return _unsigned(_fmix(_u64(x)), x)


def fmix64_inv(y):
    """the id (signed) whose ct_hash is y"""
    return _signed(_fmix_inv(_u64(y)))


def pair_hash(a, b):
    """ds_hash<KEYED> / ts_pair_hash of the pair (a, b)"""
    h = _fmix(_fmix(_u64(a)) ^ _mul(_u64(b), GOLDEN))
    return int(h) if h.ndim == 0 else h


def pair_with_hash(target, a):
    """the b (signed) with pair_hash(a, b) == target"""
    return _signed(_mul(_fmix_inv(_u64(target)) ^ _fmix(_u64(a)), GOLDEN_INV))


def home(h, slots):
    """the home slot of hash h in a table of `slots` (a power of two) slots"""
    assert slots > 0 and slots & (slots - 1) == 0
    return _unsigned(_u64(h) & np.uint64(slots - 1), h)


def tag(h):
    """the 23 tag bits gs_distinct.hip keeps beside a slot's index"""
    return _unsigned(_u64(h) >> np.uint64(TAG_SHIFT), h)


def filter_bit(h):
    """the bit of gs_trisample.hip's 2^19-bit filter"""
    return _unsigned(_u64(h) >> np.uint64(64 - FILTER_BITS), h)


def ids_with_hash(hashes):
    """the ids (int64 array) whose ct_hash is the given one, element by element"""
    return fmix64_inv(np.asarray(hashes, dtype=np.uint64))


def ids_with_low_bits(value, bits, count, skip=()):
    """`count` distinct ids whose hash has the given low `bits`: fmix64_inv((j << bits) | value), j = 0, 1, ...
    Ids in `skip` and -1 (the empty-slot word: the tables keep it in a side slot) are passed over."""
    assert 0 < bits < 64 and 0 <= value < 1 << bits and count <= 1 << (64 - bits)
    banned = {int(v) for v in skip} | {-1}
    out, j = [], 0
    while len(out) < count:
        m = count - len(out)
        h = (np.arange(j, j + m, dtype=np.uint64) << np.uint64(bits)) | np.uint64(value)
        out.extend(v for v in ids_with_hash(h).tolist() if v not in banned)
        j += m
    return np.array(out, dtype=np.int64)


def _spread(a0, b0, j):
    """a deterministic, well spread first id for the j-th constructed pair"""
    return fmix64((int(a0) ^ (int(b0) * 3) ^ 0xADE5) + j + 1)


def pairs_with_hash_of(a0, b0, count, ordered=False):
    """(a, b) int64 columns of `count` distinct pairs that differ from (a0, b0) and have its 64-bit pair hash.
    ordered=True keeps only pairs with a < b (signed), the triangle sampler's normalised (min, max) pairs."""
    a0, b0 = int(a0), int(b0)
    target = pair_hash(a0, b0)
    A, B, seen, j = [], [], {_signed(_u64(a0))}, 0
    while len(A) < count:
        a = _signed(_u64(_spread(a0, b0, j)))
        j += 1
        if a in seen:
            continue
        seen.add(a)
        b = pair_with_hash(target, a)
        if ordered and not a < b:
            continue
        A.append(a)
        B.append(b)
    return np.array(A, dtype=np.int64), np.array(B, dtype=np.int64)


def pairs_same_home_and_tag(a0, b0, count, home_bits=HOME_BITS, ordered=False):
    """(a, b) int64 columns of `count` distinct pairs that differ from (a0, b0), whose pair hash shares bits
    0 .. home_bits - 1 (the home in every table of up to 2^home_bits slots) and bits 41 .. 63 (the tag, and
    with it the filter bit) with its hash, and differs from it somewhere in between.  ordered=True keeps only
    pairs with a < b (signed)."""
    assert 0 < home_bits < TAG_SHIFT and count < 1 << (TAG_SHIFT - home_bits)
    h0 = pair_hash(a0, b0)
    width = TAG_SHIFT - home_bits
    keep = h0 & ~(((1 << width) - 1) << home_bits) & M64
    mid0 = (h0 >> home_bits) & ((1 << width) - 1)
    A, B, j = [], [], 0
    while len(A) < count:
        assert j < (1 << width) - 1
        mid = (mid0 + 1 + j) & ((1 << width) - 1)
        a = _signed(_u64(_spread(a0, b0, j)))
        b = pair_with_hash(keep | (mid << home_bits), a)
        j += 1
        if ordered and not a < b:
            continue
        A.append(a)
        B.append(b)
    return np.array(A, dtype=np.int64), np.array(B, dtype=np.int64)


# ---- the adversarial streams: test_hash_adversary.py checks them against the reference models alone (CPU),
# ---- test_gpu_hash_collisions.py feeds them to the device tables ------------------------------------------
K = 1500                       # keys of one cluster: several 256-lane workgroups claim slots of one probe chain
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TAIL = (1 << HOME_BITS) - 1    # low hash bits all ones: the home is the last slot of every table
MID = 0x5A5A5A                 # a mid-table home
ADJ = 0x2B3C4C                 # even, so ADJ and ADJ + 1 are neighbouring homes in every table
INITIAL_SLOTS = 64             # a state created with reserve 0
SPLIT_VALUE = 0x2A             # `splits`: only the low log2(INITIAL_SLOTS) hash bits agree
ID_SETS = ("tail", "one_home", "adjacent", "splits")


def _rng(*words):
    return np.random.default_rng([0xC0111DE] + [int.from_bytes(str(w).encode(), "little") % (1 << 63) for w in words])


def _ro(*cols):
    out = []
    for c in cols:
        c = np.ascontiguousarray(c, dtype=np.int64)
        c.setflags(write=False)
        out.append(c)
    return tuple(out)


def cluster_ids(name, k=K):
    """the k ids of one id set of the single-id tables (ContinuousState, WeightedMatchingState, AssignComponentsState)"""
    if name == "tail":
        return ids_with_low_bits(TAIL, HOME_BITS, k)
    if name == "one_home":
        return ids_with_low_bits(MID, HOME_BITS, k)
    if name == "adjacent":
        return np.concatenate([ids_with_low_bits(ADJ, HOME_BITS, k // 2), ids_with_low_bits(ADJ + 1, HOME_BITS, k - k // 2)])
    assert name == "splits"
    bits = INITIAL_SLOTS.bit_length() - 1
    high = np.unique(_rng("splits").integers(0, 1 << (63 - bits), 2 * k, dtype=np.uint64))
    ids = ids_with_hash((_rng("order").permutation(high) << np.uint64(bits)) | np.uint64(SPLIT_VALUE))
    return ids[ids != -1][:k]


def fillers(rng, n=300):
    """a few hundred ordinary ids, and the three ids at the edges of int64 (-1 is the empty-slot word)"""
    return np.concatenate([rng.choice(1_000_000, n, replace=False), [-1, I64_MIN, I64_MAX]]).astype(np.int64)


def check_cluster(name, ids, slots):
    """asserts that `ids`, all of the id set `name`, collide as the set promises in a table of `slots` slots;
    returns the number of them in the fullest home slot"""
    if len(ids) == 0:
        return 0
    homes, counts = np.unique(home(fmix64(np.asarray(ids, dtype=np.int64)), slots), return_counts=True)
    if name == "tail":
        assert homes.tolist() == [slots - 1], homes
    elif name == "one_home":
        assert homes.tolist() == [MID & (slots - 1)], homes
    elif name == "adjacent":
        h = ADJ & (slots - 1)
        assert set(homes.tolist()) <= {h, h + 1} and h + 1 < slots, homes
    else:
        assert np.all(homes % INITIAL_SLOTS == SPLIT_VALUE), homes
        assert int(counts.max()) * slots >= len(ids) * INITIAL_SLOTS
    return int(counts.max())


def single_id_pool(names, k=K):
    """(ids, {name: cluster ids}) -- the clusters of the named id sets, mixed with the fillers"""
    clusters = {name: cluster_ids(name, k) for name in names}
    ids = np.concatenate(list(clusters.values()) + [fillers(_rng("fill", *names))])
    assert len(set(ids.tolist())) == len(ids)
    return ids, clusters


def continuous_stream(name, k=K):
    """(src, dst, cluster): every id of the set and of the fillers three times as a source and three times as a
    target, in six independent orders"""
    ids, clusters = single_id_pool([name], k)
    rng = _rng("continuous", name)
    src = np.concatenate([rng.permutation(ids) for _ in range(3)])
    dst = np.concatenate([rng.permutation(ids) for _ in range(3)])
    return _ro(src, dst) + (clusters[name],)


def distinct_stream(mode, k=K):
    """(src, dst, val, groups) for DistinctState.  groups: name -> (src, dst) of the distinct keys planted:
      a  k keys whose home is the last slot, every tag different;
      b  301 keys whose home is the last slot too, all with one tag -- the tag of a's key 4;
      c  (keyed only) 65 keys with one 64-bit hash, at a mid-table home;
      fill  200 ordinary keys.
    Every key of a, b and c stands four times in the stream, the stream is in random order: the first arrival
    wins, the other three are duplicates, inside its batch or batches later.  In instance mode the key is dst
    alone and the four copies carry four different sources.  val = the position in the stream."""
    keyed = mode == "keyed"
    rng = _rng("distinct", mode)
    one = np.uint64(1)
    mids = rng.permutation(1 << (TAG_SHIFT - HOME_BITS)).astype(np.uint64)
    ha = ((np.arange(k, dtype=np.uint64) + one) << np.uint64(TAG_SHIFT)) | (mids[:k] << np.uint64(HOME_BITS)) | np.uint64(TAIL)
    hb = (np.uint64(5) << np.uint64(TAG_SHIFT)) | (mids[k:k + 301] << np.uint64(HOME_BITS)) | np.uint64(TAIL)
    groups = {}
    if keyed:
        sa = rng.integers(I64_MIN, I64_MAX, k)
        groups["a"] = (sa, pair_with_hash(ha, sa))
        b0 = (77, pair_with_hash(int(hb[0]), 77))
        sb, db = pairs_same_home_and_tag(*b0, 300)
        groups["b"] = (np.concatenate([[b0[0]], sb]), np.concatenate([[b0[1]], db]))
        c0 = (11, pair_with_hash((9 << TAG_SHIFT) | MID, 11))
        sc, dc = pairs_with_hash_of(*c0, 64)
        groups["c"] = (np.concatenate([[c0[0]], sc]), np.concatenate([[c0[1]], dc]))
    else:
        groups["a"] = (rng.integers(0, 1000, k), ids_with_hash(ha))
        groups["b"] = (rng.integers(0, 1000, 301), ids_with_hash(hb))
    planted = [np.concatenate([groups[g][i] for g in sorted(groups)]).astype(np.int64) for i in (0, 1)]
    fill = (rng.integers(0, 50, 200), rng.integers(2000, 2050, 200))
    groups["fill"] = fill
    src = [planted[0]] + [planted[0] if keyed else rng.integers(1000, 2000, len(planted[0])) for _ in range(3)] + [fill[0]]
    dst = [planted[1]] * 4 + [fill[1]]
    order = rng.permutation(sum(len(x) for x in src))
    src, dst = np.concatenate(src)[order], np.concatenate(dst)[order]
    return _ro(src, dst, np.arange(len(src))) + (groups,)


def distinct_key_hash(mode, src, dst):
    return pair_hash(src, dst) if mode == "keyed" else fmix64(dst)


def edge_stream(names, n_random, k=K, repeats=0, weights=False):
    """(src, dst[, val], clusters): random edges among the ids of the named id sets and the fillers -- every id is
    an endpoint at least once; `repeats` of the edges stand twice; val: 16-bit weights"""
    ids, clusters = single_id_pool(names, k)
    rng = _rng("edges", *names)
    p = rng.permutation(ids)
    if len(p) % 2:
        p = np.concatenate([p, p[:1]])
    src = np.concatenate([p[0::2], rng.choice(ids, n_random)])
    dst = np.concatenate([p[1::2], rng.choice(ids, n_random)])
    again = rng.choice(len(src), repeats, replace=False)
    src, dst = np.concatenate([src, src[again]]), np.concatenate([dst, dst[again]])
    order = rng.permutation(len(src))
    cols = (src[order], dst[order]) + ((rng.integers(0, 1 << 16, len(src)),) if weights else ())
    return _ro(*cols) + (clusters,)


# ---- the triangle sampler: decoys for the pairs its samplers want ------------------------------------------
TS_HOME_BITS = 20    # the sampler's table size is not exposed: homes are compared on the low 20 hash bits
TSR_SRC, TSR_TRG, TSR_THIRD, TSR_FLAGS, TSR_J, TSR_LAST, TSR_NEXT = range(7)   # GS_TRISAMPLE_ROW_WORDS layout
# the sampler of the tests: 256 samplers over 1000 vertices, warmed up so that replacements are rare; the batch
# is more than one tile of the streaming pass and of odd length
TS_S, TS_V, TS_SEED, TS_WARM, TS_BATCH = 256, 1000, 0x7A5, 20_000, 3001


def trisample_warmup():
    """(src, dst): TS_WARM ordinary edges over [0, TS_V)"""
    rng = _rng("warmup")
    return _ro(rng.integers(0, TS_V, TS_WARM), rng.integers(0, TS_V, TS_WARM))


def wanted_pairs(rows, seen, n):
    """[(sampler, a, b)]: the normalised (min, max) pairs wanted through the whole coming batch of n edges -- the
    two of every sampler that holds an edge, has neither found flag set and is not replaced before seen + n"""
    out = []
    for i, r in enumerate(np.asarray(rows).tolist()):
        if r[TSR_J] >= 1 and r[TSR_FLAGS] == 0 and r[TSR_NEXT] > seen + n:
            for x in (r[TSR_SRC], r[TSR_TRG]):
                out.append((i, min(x, r[TSR_THIRD]), max(x, r[TSR_THIRD])))
    return out


def trisample_batch(rows, seen, n, vertex_count, seed=0):
    """(src, dst): n edges for a sampler state whose exported rows are `rows` after `seen` edges.  Ordinary
    edges over [0, vertex_count), and planted into them, for every wanted pair: one decoy pair with its 64-bit
    pair hash, one decoy that shares its filter bit and its home slot but not its hash -- both in the first
    half of the batch -- and, for the samplers with an even number, the wanted edge itself in the second half
    (so those samplers find their triangle).  Planted edges come in either orientation."""
    rng = _rng("trisample", seed)
    src, dst = rng.integers(0, vertex_count, n), rng.integers(0, vertex_count, n)
    want = wanted_pairs(rows, seen, n)
    assert 3 * len(want) <= n // 2
    early = iter(rng.choice(n // 2, 2 * len(want), replace=False).tolist())
    late = iter((n // 2 + rng.choice(n - n // 2, len(want), replace=False)).tolist())
    for i, a, b in want:
        da, db = pairs_with_hash_of(a, b, 1, ordered=True)
        ha_, hb_ = pairs_same_home_and_tag(a, b, 1, home_bits=TS_HOME_BITS, ordered=True)
        plant = [(next(early), int(da[0]), int(db[0])), (next(early), int(ha_[0]), int(hb_[0]))]
        if i % 2 == 0:
            plant.append((next(late), a, b))
        for pos, x, y in plant:
            src[pos], dst[pos] = (x, y) if rng.random() < 0.5 else (y, x)
    return _ro(src, dst)


def count_decoys(rows, seen, src, dst):
    """(full, near): the edges of the batch that are no wanted pair but share the 64-bit hash of one (full), or
    share filter bit and home slot -- on the low TS_HOME_BITS bits -- with one and not its hash (near)"""
    want = wanted_pairs(rows, seen, len(src))
    pairs = {(a, b) for _, a, b in want}
    wh = pair_hash(np.array([a for _, a, _ in want], dtype=np.int64), np.array([b for _, _, b in want], dtype=np.int64))
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    h = pair_hash(lo, hi)
    other = np.array([(a, b) not in pairs for a, b in zip(lo.tolist(), hi.tolist())])
    same_hash = np.isin(h, wh)

    def near_key(x):
        return (filter_bit(x) << np.uint64(TS_HOME_BITS)) | home(x, 1 << TS_HOME_BITS)
    near = np.isin(near_key(h), near_key(wh)) & ~same_hash
    return int(np.sum(other & same_hash)), int(np.sum(other & near))

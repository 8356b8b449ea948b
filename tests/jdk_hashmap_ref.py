"""An independent model of java.util.HashMap<Long, Object> as HashSet<Long>.add uses it (JDK 8 and later).

WindowTriangles reads HashSet<Long>.toArray(), so its candidate records and its self-pair term depend on the
exact JDK iteration order.  The project restates HashMap twice over index-linked arrays (the oracle's
hashset_order and the kernels of gs_hashset.hip), and both came from one reading.  This file is a second, literal
restatement over node objects with references, written from the JDK's method bodies (putVal, resize, treeifyBin,
TreeNode.treeify / putTreeVal / split / untreeify / balanceInsertion / rotateLeft / rotateRight /
moveRootToFront), method for method and branch for branch.  It imports neither the oracle nor the package, and it
is held to answers derived on paper (tests/test_jdk_hashmap_ref.py) and to the invariants that the JDK's own
TreeNode.checkInvariants implies (check_invariants below).

Hashes are Java ints: kept as SIGNED 32-bit values.  `hash & mask` on a negative Python int acts on its two's
complement, as in Java, so the bin index and the split bit need no conversion; the tree order compares the signed
value, as `(ph = p.hash) > h` does.  `HashMap(signed=False)` compares the hashes as unsigned instead: that is not
the JDK, it is the reading the project had, kept so that a test can show from the model that a case separates
the two."""

TREEIFY_THRESHOLD = 8
UNTREEIFY_THRESHOLD = 6
MIN_TREEIFY_CAPACITY = 64
DEFAULT_INITIAL_CAPACITY = 16

FLAG_TREEIFIED = 1         # some bin became a red-black tree
FLAG_COLLISION_RESIZE = 2  # treeifyBin below MIN_TREEIFY_CAPACITY resized the table instead


def _int32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def long_hash_code(x):
    """Long.hashCode: (int)(value ^ (value >>> 32))."""
    u = x & 0xFFFFFFFFFFFFFFFF
    return _int32(u ^ (u >> 32))


def spread(h):
    """HashMap.hash: h ^ (h >>> 16), an int."""
    u = h & 0xFFFFFFFF
    return _int32(u ^ (u >> 16))


def java_hash(x):
    return spread(long_hash_code(x))


class Node:
    __slots__ = ("hash", "key", "next")

    def __init__(self, hash_, key, next_):
        self.hash, self.key, self.next = hash_, key, next_


class TreeNode(Node):
    __slots__ = ("parent", "left", "right", "prev", "red")

    def __init__(self, hash_, key, next_):
        super().__init__(hash_, key, next_)
        self.parent = self.left = self.right = self.prev = None
        self.red = False

    def root(self):
        r = self
        while True:
            p = r.parent
            if p is None:
                return r
            r = p


class HashMap:
    def __init__(self, signed=True):
        self.table = None
        self.threshold = 0
        self.size = 0
        self.flags = 0
        self.signed = signed
        self.mixed_sign_compares = 0   # tree comparisons between hashes of different sign
        self.root_moves_at = []        # the map's size before each put whose putTreeVal moved a new root to the front

    # ---- the tree order: (ph = p.hash) > h ? -1 : ph < h ? 1 : k.compareTo(pk) ----------------------------
    def _dir(self, ph, pk, h, k):
        if (ph < 0) != (h < 0):
            self.mixed_sign_compares += 1
        if not self.signed:
            ph, h = ph & 0xFFFFFFFF, h & 0xFFFFFFFF
        if ph > h:
            return -1
        if ph < h:
            return 1
        return -1 if k < pk else 1   # Long.compareTo; equal keys never get here (see put_tree_val)

    # ---- HashSet.add -> HashMap.put -> putVal --------------------------------------------------------------
    def put(self, key):
        """True if the key was added (HashSet.add's result)."""
        hash_ = java_hash(key)
        tab = self.table
        if tab is None or len(tab) == 0:
            tab = self.resize()
        n = len(tab)
        i = (n - 1) & hash_
        p = tab[i]
        if p is None:
            tab[i] = Node(hash_, key, None)
        else:
            e = None
            if p.hash == hash_ and p.key == key:
                e = p
            elif isinstance(p, TreeNode):
                e = self.put_tree_val(p, tab, hash_, key)
            else:
                bin_count = 0
                while True:
                    e = p.next
                    if e is None:
                        p.next = Node(hash_, key, None)
                        if bin_count >= TREEIFY_THRESHOLD - 1:   # -1 for 1st
                            self.treeify_bin(tab, hash_)
                        break
                    if e.hash == hash_ and e.key == key:
                        break
                    p = e
                    bin_count += 1
            if e is not None:   # existing mapping for key
                return False
        self.size += 1
        if self.size > self.threshold:
            self.resize()
        return True

    def resize(self):
        old_tab = self.table
        old_cap = 0 if old_tab is None else len(old_tab)
        old_thr = self.threshold
        new_thr = 0
        if old_cap > 0:
            new_cap = old_cap << 1
            if old_cap >= DEFAULT_INITIAL_CAPACITY:
                new_thr = old_thr << 1   # double threshold
        elif old_thr > 0:
            new_cap = old_thr
        else:                            # zero initial threshold signifies using defaults
            new_cap = DEFAULT_INITIAL_CAPACITY
            new_thr = int(0.75 * DEFAULT_INITIAL_CAPACITY)
        if new_thr == 0:
            new_thr = int(new_cap * 0.75)
        self.threshold = new_thr
        new_tab = [None] * new_cap
        self.table = new_tab
        if old_tab is not None:
            for j in range(old_cap):
                e = old_tab[j]
                if e is None:
                    continue
                old_tab[j] = None
                if e.next is None:
                    new_tab[e.hash & (new_cap - 1)] = e
                elif isinstance(e, TreeNode):
                    self.split(e, new_tab, j, old_cap)
                else:   # preserve order
                    lo_head = lo_tail = hi_head = hi_tail = None
                    while True:
                        next_ = e.next
                        if (e.hash & old_cap) == 0:
                            if lo_tail is None:
                                lo_head = e
                            else:
                                lo_tail.next = e
                            lo_tail = e
                        else:
                            if hi_tail is None:
                                hi_head = e
                            else:
                                hi_tail.next = e
                            hi_tail = e
                        e = next_
                        if e is None:
                            break
                    if lo_tail is not None:
                        lo_tail.next = None
                        new_tab[j] = lo_head
                    if hi_tail is not None:
                        hi_tail.next = None
                        new_tab[j + old_cap] = hi_head
        return new_tab

    def treeify_bin(self, tab, hash_):
        n = 0 if tab is None else len(tab)
        if tab is None or n < MIN_TREEIFY_CAPACITY:
            self.flags |= FLAG_COLLISION_RESIZE
            self.resize()
            return
        index = (n - 1) & hash_
        e = tab[index]
        if e is not None:
            hd = tl = None
            while True:
                p = TreeNode(e.hash, e.key, None)   # replacementTreeNode
                if tl is None:
                    hd = p
                else:
                    p.prev = tl
                    tl.next = p
                tl = p
                e = e.next
                if e is None:
                    break
            tab[index] = hd
            if hd is not None:
                self.flags |= FLAG_TREEIFIED
                self.treeify(hd, tab)

    # ---- TreeNode methods (`this` is the first argument) ------------------------------------------------------
    def treeify(self, this, tab):
        root = None
        x = this
        while x is not None:
            next_ = x.next
            x.left = x.right = None
            if root is None:
                x.parent = None
                x.red = False
                root = x
            else:
                k, h = x.key, x.hash
                p = root
                while True:
                    dir_ = self._dir(p.hash, p.key, h, k)
                    xp = p
                    p = p.left if dir_ <= 0 else p.right
                    if p is None:
                        x.parent = xp
                        if dir_ <= 0:
                            xp.left = x
                        else:
                            xp.right = x
                        root = balance_insertion(root, x)
                        break
            x = next_
        move_root_to_front(tab, root)

    def put_tree_val(self, this, tab, h, k):
        root = this.root() if this.parent is not None else this
        p = root
        while True:
            if p.hash == h and p.key == k:
                return p
            dir_ = self._dir(p.hash, p.key, h, k)
            xp = p
            p = p.left if dir_ <= 0 else p.right
            if p is None:
                xpn = xp.next
                x = TreeNode(h, k, xpn)   # newTreeNode
                if dir_ <= 0:
                    xp.left = x
                else:
                    xp.right = x
                xp.next = x
                x.parent = x.prev = xp
                if xpn is not None:
                    xpn.prev = x
                if move_root_to_front(tab, balance_insertion(root, x)):
                    self.root_moves_at.append(self.size)
                return None

    def untreeify(self, this):
        hd = tl = None
        q = this
        while q is not None:
            p = Node(q.hash, q.key, None)   # replacementNode
            if tl is None:
                hd = p
            else:
                tl.next = p
            tl = p
            q = q.next
        return hd

    def split(self, this, tab, index, bit):
        b = this
        # relink into lo and hi lists, preserving order
        lo_head = lo_tail = hi_head = hi_tail = None
        lc = hc = 0
        e = b
        while e is not None:
            next_ = e.next
            e.next = None
            if (e.hash & bit) == 0:
                e.prev = lo_tail
                if lo_tail is None:
                    lo_head = e
                else:
                    lo_tail.next = e
                lo_tail = e
                lc += 1
            else:
                e.prev = hi_tail
                if hi_tail is None:
                    hi_head = e
                else:
                    hi_tail.next = e
                hi_tail = e
                hc += 1
            e = next_
        if lo_head is not None:
            if lc <= UNTREEIFY_THRESHOLD:
                tab[index] = self.untreeify(lo_head)
            else:
                tab[index] = lo_head
                if hi_head is not None:   # (else is already treeified)
                    self.treeify(lo_head, tab)
        if hi_head is not None:
            if hc <= UNTREEIFY_THRESHOLD:
                tab[index + bit] = self.untreeify(hi_head)
            else:
                tab[index + bit] = hi_head
                if lo_head is not None:
                    self.treeify(hi_head, tab)

    # ---- iteration: bins 0 .. cap-1, each along `next` --------------------------------------------------------
    def keys(self):
        out = []
        for e in self.table or ():
            while e is not None:
                out.append(e.key)
                e = e.next
        return out

    def capacity(self):
        return 0 if self.table is None else len(self.table)

    def mixed_sign_tree_bins(self):
        """How many bins are trees right now whose hashes have both signs."""
        c = 0
        for e in self.table or ():
            if isinstance(e, TreeNode):
                neg = pos = False
                while e is not None:
                    neg, pos = neg or e.hash < 0, pos or e.hash >= 0
                    e = e.next
                c += neg and pos
        return c


def move_root_to_front(tab, root):
    """Returns whether the root was moved (the JDK's is void; the model's callers count the moves)."""
    moved = False
    n = 0 if tab is None else len(tab)
    if root is not None and tab is not None and n > 0:
        index = (n - 1) & root.hash
        first = tab[index]
        if root is not first:
            tab[index] = root
            rp = root.prev
            rn = root.next
            if rn is not None:
                rn.prev = rp
            if rp is not None:
                rp.next = rn
            if first is not None:
                first.prev = root
            root.next = first
            root.prev = None
            moved = True
    return moved


def rotate_left(root, p):
    if p is not None:
        r = p.right
        if r is not None:
            rl = p.right = r.left
            if rl is not None:
                rl.parent = p
            pp = r.parent = p.parent
            if pp is None:
                root = r
                root.red = False
            elif pp.left is p:
                pp.left = r
            else:
                pp.right = r
            r.left = p
            p.parent = r
    return root


def rotate_right(root, p):
    if p is not None:
        l = p.left
        if l is not None:
            lr = p.left = l.right
            if lr is not None:
                lr.parent = p
            pp = l.parent = p.parent
            if pp is None:
                root = l
                root.red = False
            elif pp.right is p:
                pp.right = l
            else:
                pp.left = l
            l.right = p
            p.parent = l
    return root


def balance_insertion(root, x):
    x.red = True
    while True:
        xp = x.parent
        if xp is None:
            x.red = False
            return x
        if not xp.red:
            return root
        xpp = xp.parent
        if xpp is None:
            return root
        xppl = xpp.left
        if xp is xppl:
            xppr = xpp.right
            if xppr is not None and xppr.red:
                xppr.red = False
                xp.red = False
                xpp.red = True
                x = xpp
            else:
                if x is xp.right:
                    x = xp
                    root = rotate_left(root, x)
                    xp = x.parent
                    xpp = None if xp is None else xp.parent
                if xp is not None:
                    xp.red = False
                    if xpp is not None:
                        xpp.red = True
                        root = rotate_right(root, xpp)
        else:
            if xppl is not None and xppl.red:
                xppl.red = False
                xp.red = False
                xpp.red = True
                x = xpp
            else:
                if x is xp.left:
                    x = xp
                    root = rotate_right(root, x)
                    xp = x.parent
                    xpp = None if xp is None else xp.parent
                if xp is not None:
                    xp.red = False
                    if xpp is not None:
                        xpp.red = True
                        root = rotate_left(root, xpp)


# ---- what the JDK's TreeNode.checkInvariants implies, and what a table implies -------------------------------
def check_invariants(m):
    """Asserts: every node sits in the bin of its hash; a list bin holds plain nodes; in a tree bin next/prev are
    consistent, the first node is the (black) root, parent/child links are consistent, the tree holds exactly
    the bin's nodes in BST order under (hash, key) -- signed hash for a JDK map --, no red node has a red child,
    and every root-to-leaf path has the same number of black nodes; the sizes add up."""
    tab = m.table
    if tab is None:
        assert m.size == 0
        return
    cap = len(tab)
    assert cap >= 16 and cap & (cap - 1) == 0 and m.threshold == cap // 4 * 3
    assert m.size <= m.threshold, "a put returned above the threshold"
    total = 0
    for index, first in enumerate(tab):
        if first is None:
            continue
        chain = []
        e = first
        while e is not None:
            assert (cap - 1) & e.hash == index and e.hash == java_hash(e.key), (index, e.key)
            assert -(1 << 31) <= e.hash < (1 << 31)
            chain.append(e)
            e = e.next
            assert len(chain) <= m.size, "cycle in next"
        total += len(chain)
        assert len({id(e) for e in chain}) == len(chain)
        if not isinstance(first, TreeNode):
            assert all(type(e) is Node for e in chain), index
            continue
        assert all(type(e) is TreeNode for e in chain), index
        assert len(chain) > UNTREEIFY_THRESHOLD, "a tree bin this small is untreeified by split, never made"
        prev = None
        for e in chain:   # next / prev
            assert e.prev is prev, (index, e.key)
            prev = e
        assert first.parent is None and not first.red, "the bin's first node is its root"
        key_of = (lambda e: (e.hash, e.key)) if m.signed else (lambda e: (e.hash & 0xFFFFFFFF, e.key))
        seen = []

        def walk(t, lo, hi):   # -> black height
            if t is None:
                return 1
            seen.append(id(t))
            kk = key_of(t)
            assert (lo is None or lo < kk) and (hi is None or kk < hi), ("BST order", index, t.key)
            for c in (t.left, t.right):
                if c is not None:
                    assert c.parent is t, ("parent/child", index, t.key)
                    assert not (t.red and c.red), ("red-red", index, t.key)
            hl, hr = walk(t.left, lo, kk), walk(t.right, kk, hi)
            assert hl == hr, ("black height", index, t.key)
            return hl + (0 if t.red else 1)

        walk(first, None, None)
        assert sorted(seen) == sorted(id(e) for e in chain), ("tree and list hold the same nodes", index)
    assert total == m.size


def build(ids, signed=True, check_every_put=False):
    m = HashMap(signed=signed)
    for x in ids:
        m.put(int(x))
        if check_every_put:
            check_invariants(m)
    return m


def hashset_order(ids, signed=True):
    """ids in arrival order (duplicates allowed) -> (HashSet iteration order, flags)."""
    m = build(ids, signed=signed)
    return m.keys(), m.flags


# ---- GenerateCandidateEdges over slice(ALL), WindowTriangles.java:91-114, on top of the model -----------------
def candidate_records(src, dst):
    """(a, b, is_candidate, flags): per vertex in ascending id order, its edge records (v, t, false) in arrival
    order (edge i is a record of src[i], then one of dst[i]), then for i < n-1, j >= i over the HashSet's array the
    pair (ids[i], ids[j], true) when both are above v.  flags: the model's, or-ed over the vertices."""
    import numpy as np

    nbrs = {}
    for s, d in zip((int(x) for x in src), (int(x) for x in dst)):
        nbrs.setdefault(s, []).append(d)
        nbrs.setdefault(d, []).append(s)
    a, b, f, flags = [], [], [], 0
    for v in sorted(nbrs):
        a.append(np.full(len(nbrs[v]), v, dtype=np.int64))
        b.append(np.array(nbrs[v], dtype=np.int64))
        f.append(np.zeros(len(nbrs[v]), dtype=np.uint8))
        order, fl = hashset_order(nbrs[v])
        flags |= fl
        ids = np.array(order, dtype=np.int64)
        for i in range(len(ids) - 1):
            if ids[i] > v:
                js = ids[i:][ids[i:] > v]
                a.append(np.full(len(js), ids[i], dtype=np.int64))
                b.append(js)
                f.append(np.ones(len(js), dtype=np.uint8))
    return np.concatenate(a), np.concatenate(b), np.concatenate(f), flags

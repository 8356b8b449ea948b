"""A sequential Python model of gs_matching.hip's batch scheme, step for step: epoch-tagged reservation words
(word(i) = epoch << 32 | (2^32 - 1 - i), kept by max), de-duplicated footprints of slot numbers, the evaluate /
block-to-a-fixed-point / finalise rounds and the commit's writes.  Where the kernels run lanes in parallel the
model visits edges in a shuffled order (blocking passes, commits of one round), so a result that depended on
that order would show.  test_matching_rounds_model.py holds it against matching_ref: the exactness argument of
DESIGN ("CentralizedWeightedMatching"), checkable without a GPU."""
import random

import matching_ref as ref

MASK = (1 << 64) - 1
MATCHED, SRC = 1 << 32, 1 << 33
NONE = 0xFFFFFFFF


class RoundsModel:
    def __init__(self, seed=0):
        self.slot = {}
        self.id, self.wgt, self.link, self.resv = [], [], [], []
        self.epoch = self.rounds = self.block_iterations = 0
        self.rng = random.Random(seed)

    def _slot(self, v):                                  # mt_slot
        if v not in self.slot:
            self.slot[v] = len(self.id)
            self.id.append(v); self.wgt.append(0); self.link.append(0); self.resv.append(0)
        return self.slot[v]

    @staticmethod
    def _collisions(la, lb, a, b):                       # mt_collisions
        ma = bool(la & MATCHED)
        mb = bool(lb & MATCHED) and b != a and not (ma and (la & 0xFFFFFFFF) == b)
        return ma, mb

    def _evaluate(self, a, b, w):                        # mt_evaluate
        la, lb = self.link[a], self.link[b]
        ma, mb = self._collisions(la, lb, a, b)
        pa = (la & 0xFFFFFFFF) if ma else NONE
        pb = (lb & 0xFFFFFFFF) if mb else NONE
        fp = [a, b if b != a else NONE, pa if pa not in (a, b) else NONE, pb if pb not in (a, b) else NONE]
        total = ((self.wgt[a] if ma else 0) + (self.wgt[b] if mb else 0)) & MASK
        return w > ref.java_long((2 * total) & MASK), [x for x in fp if x != NONE]

    def _commit(self, a, b, u, v, w):                    # mt_commit
        la, lb = self.link[a], self.link[b]
        ma, mb = self._collisions(la, lb, a, b)
        pa, pb = la & 0xFFFFFFFF, lb & 0xFFFFFFFF
        ev = []
        if ma:
            p = self.id[pa]
            ev.append((ref.REMOVE,) + ((u, p) if la & SRC else (p, u)) + (ref.java_long(self.wgt[a]),))
        if mb:
            p = self.id[pb]
            ev.append((ref.REMOVE,) + ((v, p) if lb & SRC else (p, v)) + (ref.java_long(self.wgt[b]),))
        if ma:
            self.link[pa] = 0
        if mb:
            self.link[pb] = 0
        self.wgt[a], self.link[a] = w & MASK, MATCHED | SRC | b
        if b != a:
            self.wgt[b], self.link[b] = w & MASK, MATCHED | a
        return ev + [(ref.ADD, u, v, w)]

    def _reserve(self, fp, word):
        for x in fp:
            self.resv[x] = max(self.resv[x], word)

    def batch(self, src, dst, val, base=0):
        """one gs_match_edges call: (type, src, dst, val, base + index) per event"""
        n = len(src)
        su, sv = [self._slot(x) for x in src], [self._slot(x) for x in dst]
        pend, events = list(range(n)), [None] * n
        while pend:
            self.epoch += 1
            self.rounds += 1
            word = {i: (self.epoch << 32) | (0xFFFFFFFF - i) for i in pend}
            fps, st = {}, {}
            for i in pend:                               # k_mt_eval: decisions under the round's starting state
                acc, fps[i] = self._evaluate(su[i], sv[i], val[i])
                st[i] = 1 if acc else 0
            for i in pend:
                if st[i]:
                    self._reserve(fps[i], word[i])
            while True:                                  # k_mt_block to its fixed point
                self.block_iterations += 1
                changed = False
                for i in self.rng.sample(pend, len(pend)):
                    if st[i] == 0 and any(self.resv[x] > word[i] for x in fps[i]):
                        st[i], changed = 2, True
                        self._reserve(fps[i], word[i])
                if not changed:
                    break
            commits, nxt = [], []
            for i in pend:                               # k_mt_final
                if st[i] == 0:
                    events[i] = []
                elif st[i] == 1 and all(self.resv[x] == word[i] for x in fps[i]):
                    commits.append(i)
                else:
                    nxt.append(i)
            held = [x for i in commits for x in fps[i]]
            assert len(held) == len(set(held)), "committing edges of one round share a vertex"
            self.rng.shuffle(commits)
            for i in commits:
                events[i] = self._commit(su[i], sv[i], src[i], dst[i], val[i])
            assert len(nxt) < len(pend) and min(pend) not in nxt, "the smallest pending index is final in every round"
            pend = nxt
        return [e + (base + i,) for i in range(n) for e in events[i]]

"""A sequential model of gs_assign.hip's batch algorithm (DESIGN.md §4 "AssignComponents"): the nodes, the
rounds with their snapshot rule, retire / hook, the winner-label walk, the `first` rule and the record order.
Where the kernels run one lane per edge or per vertex, the model visits them in shuffled order, so nothing it
computes may depend on the order of the lanes.  tests/test_assign_rounds_model.py holds it against
tests/assign_ref.py record for record.

The one liberty: the kernels' record pass streams over the whole vertex table; the model keeps label -> members
beside the state and visits only the vertices whose label retired -- the others emit nothing in that pass."""
import random


class RoundsModel:
    def __init__(self, seed=0):
        self.label = {}     # the state: vertex -> label
        self.members = {}   # label -> vertices (model only, see above)
        self.rng = random.Random(seed)
        self.rounds = 0
        self.live_after = {}

    def _shuffled(self, xs):
        xs = list(xs)
        self.rng.shuffle(xs)
        return xs

    def batch(self, edges, base=0):
        """the records (vertex, label, base + index of the edge) of one batch, in output order"""
        edges = [(int(s), int(t)) for s, t in edges]
        n = len(edges)
        label = self.label
        # nodes: the old labels the endpoints map to, and the new vertices as singletons labelled with themselves
        new, first = set(), {}
        for i in self._shuffled(range(n)):
            for v in edges[i]:
                if v not in label:
                    new.add(v)
                    first[v] = min(first.get(v, n), i)   # atomicMin
        node = lambda v: v if v in new else label[v]
        ra = [node(s) for s, _ in edges]
        rb = [node(t) for _, t in edges]
        parent, retire, hook = {}, {}, {}

        def find(x):
            while x in parent:
                p = parent[x]
                if p in parent:
                    parent[x] = parent[p]   # pointer halving: only ever to an ancestor
                x = p
            return x

        live, rounds = list(range(n)), 0
        self.live_after = {}
        while live:
            # step 1: roots of the live edges; joined edges drop out for good; minimum edge per root
            minedge, nxt = {}, []
            for i in self._shuffled(live):
                a, b = find(ra[i]), find(rb[i])
                ra[i], rb[i] = a, b
                if a == b:
                    continue
                minedge[a] = min(minedge.get(a, n), i)
                minedge[b] = min(minedge.get(b, n), i)
                nxt.append(i)
            if not nxt:
                break
            # steps 2 and 3: decided from ra / rb / minedge (the round-start snapshot) alone; a root loses at its
            # one minimum edge, so the link is a plain store and no decision reads it
            finalised = 0
            for i in self._shuffled(nxt):
                a, b = ra[i], rb[i]
                ma, mb = minedge[a] == i, minedge[b] == i
                if ma and mb:
                    lo, wi = (a, b) if a > b else (b, a)
                elif mb and b > a:
                    lo, wi = b, a
                elif ma and a > b:
                    lo, wi = a, b
                else:
                    continue
                assert lo not in retire
                retire[lo], hook[lo], parent[lo] = i, wi, wi
                finalised += 1
            assert finalised, "a round with live edges finalised nothing"
            rounds += 1
            if rounds in (1, 2, 4, 8):
                self.live_after[rounds] = len(nxt) - finalised
            live = nxt
        self.rounds = rounds
        # winner labels: the label the winner side held when the loser retired
        plabel = {}
        for mu in self._shuffled(retire):
            i, l = retire[mu], hook[mu]
            while l in retire and retire[l] < i:
                l = hook[l]
            plabel[mu] = l
        # records: (edge, order key inside the edge, vertex, label)
        rec = []
        for v in new:
            self.members[v] = [v]
        touched = self._shuffled(v for mu in retire for v in self.members[mu])
        moves = {}
        for v in touched:
            mu = node(v)
            while mu in retire:
                rec.append((retire[mu], v, v, plabel[mu]))
                mu = plabel[mu]
            moves[v] = mu
        for v in self._shuffled(new):
            f = first[v]
            s, t = edges[f]
            if s == t:
                rec += [(f, 0, v, v), (f, 1, v, v)]
            elif s in new and t in new and first[s] == f and first[t] == f and v == min(s, t):
                rec.append((f, None, v, v))
        # the new component's pair goes out as (src, dst); every other edge ascending by vertex
        out = []
        for e, key, v, c in rec:
            s, t = edges[e]
            if s != t and s in new and t in new and first[s] == e and first[t] == e:
                key = 0 if v == s else 1
            out.append((e, key, v, c))
        out.sort(key=lambda r: (r[0], r[1]))
        # commit
        for v in new:
            label[v] = v
        for mu in retire:
            del self.members[mu]
        for v, mu in moves.items():
            label[v] = mu
            self.members[mu].append(v)
        return [(v, c, base + e) for e, _, v, c in out]

    def state(self):
        return dict(self.label)


def run(edges, cut=None, seed=0):
    m = RoundsModel(seed)
    cut = cut or max(1, len(edges))
    out = []
    for at in range(0, len(edges), cut):
        out += m.batch(edges[at:at + cut], at)
    return out, m

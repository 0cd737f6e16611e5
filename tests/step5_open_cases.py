"""Hand-made inputs of the tests of Step 5's opening (step5.opening: the paths index, Unsat's links, LayoutReads): small graphs built with
the Builder of step4_cases WITH mirror images, so that inv[e] = e ^ 1 until a palindromic edge (its own mirror) is added; K = 20, no real
sequence overlap (nothing here reads a base), a handful of reads.  Every case writes down what must come out:

    cases() -> {name: Case}; Case.inputs() -> (hbv, inv, paths, read_len)
    Case.index    {edge: [read ids]}                 edges not named hold nothing, here and below
    Case.links    {edge: [(link_to, pid)]}
    Case.mult     {(edge, link_to): multiplicity}
    Case.layout   {edge: [(pos, read id, forward)]}
    Case.counters every one of step5.OPEN_COUNTERS

    recorded() -> the names of the cases (hand-made, and random_<seed> for SEEDS) whose run of the reference's own invert and LayoutReads
                  lies under tests/golden/refruns/step5_open_<name>/
    reference_run(name, workdir) -> (index, layout) of that run, as per_edge gives them

Unless a case says otherwise an edge has 30 bases (11 K-mers) and a read has 10 bases at offset 0 of a one-edge path [e]: its layout
entries are (e, 0, forward) and (inv e, 30 - 10 = 20, reverse).  In the search cases the pair is (a read on `a`, a read on inv t) for a
forward edge t = W -> X: x1 = [a], x2 = [t], the search runs from v = to_right[a] for w = W, and an unsatisfied pair links a -> t and
inv t -> inv a."""
import os

import numpy as np

from conftest import reference_outputs
from step4_cases import Builder
from w2rap_contigger_amd import formats as F

K = 20
COUNTERS = ("n_pairs_placed", "n_meet", "n_same_vertex", "n_reached", "n_unsat_depth", "n_unsat_overflow", "n_unsat_same_end",
            "n_links", "n_kinds", "n_index", "n_layout")


def counters(**kw):
    """the counters named, the others 0"""
    assert set(kw) <= set(COUNTERS)
    return {k: kw.get(k, 0) for k in COUNTERS}


class Case:
    def __init__(self):
        self.b = Builder(K)
        self.inv, self.paths, self.offs, self.rlen = [], [], [], []
        self.index, self.links, self.mult, self.layout, self.counters = {}, {}, {}, {}, {}

    def vertex(self):
        return self.b.vertex()

    def edge(self, u, v, n=30):
        """u -> v and its mirror image; -> the id of u -> v"""
        e = self.b.edge(u, v, np.zeros(n, np.uint8))
        self.inv += [e + 1, e]
        return e

    def palindrome(self, u, n=30):
        """u -> mirror of u, an edge that is its own mirror image: inv[e] == e"""
        e = self.b.edge(u, u ^ 1, np.zeros(n, np.uint8), mirror=False)
        self.inv.append(e)
        return e

    def m(self, e):
        return self.inv[e]

    def chain(self, n):
        """n edges v0 -> v1 -> ... -> vn; -> the vertices"""
        vs = [self.vertex() for _ in range(n + 1)]
        for i in range(n):
            self.edge(vs[i], vs[i + 1])
        return vs

    def read(self, path=(), offset=0, length=10):
        self.paths.append(list(path)); self.offs.append(offset); self.rlen.append(length)
        return len(self.paths) - 1

    def pair(self, a, t):
        """a read on a and its mate on inv t; -> the pid"""
        r = self.read([a]); self.read([self.m(t)])
        return r // 2

    def inputs(self):
        h = self.b.hbv()
        po = np.zeros(len(self.paths) + 1, np.uint64)
        np.cumsum([len(p) for p in self.paths], out=po[1:])
        paths = (np.array(self.offs, np.int32), po, np.array([e for p in self.paths for e in p], np.int32))
        return h, np.array(self.inv, np.int32), paths, np.array(self.rlen, np.uint32)


def per_edge(off, *arrays):
    """a CSR over the edges as {edge: [tuple of the arrays' values]} (a bare value with one array), empty edges left out"""
    off = [int(x) for x in off]
    out = {}
    for e in range(len(off) - 1):
        if off[e + 1] > off[e]:
            rows = [tuple(int(a[j]) for a in arrays) for j in range(off[e], off[e + 1])]
            out[e] = [r[0] for r in rows] if len(arrays) == 1 else rows
    return out


def kinds(r):
    return {(int(e), int(t)): int(m) for e, t, m in zip(r.kind_from, r.kind_to, r.kind_mult)}


def _search_scene(c):
    """a = s -> v, the edge the first read lies on, and t = W -> X, the edge whose mirror image the mate lies on; -> (a, t, v, W)"""
    s, v, W, X = c.vertex(), c.vertex(), c.vertex(), c.vertex()
    return c.edge(s, v), c.edge(W, X), v, W


def cases():
    out = {}

    # ---- the search: one boundary each
    for n, name in ((15, "w_at_depth_15_is_reached"), (16, "w_at_depth_16_is_not")):
        c = Case(); a, t, v, W = _search_scene(c)
        vs = [v] + [c.vertex() for _ in range(n - 1)] + [W]                  # v -> ... -> W over n edges
        for i in range(n):
            c.edge(vs[i], vs[i + 1])
        c.pair(a, t)
        c.index = {a: [0], c.m(t): [1]}
        c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
        if n == 15:
            c.counters = counters(n_pairs_placed=1, n_reached=1, n_index=2, n_layout=4)
        else:
            c.links = {a: [(t, 0)], c.m(t): [(c.m(a), 0)]}
            c.mult = {(a, t): 1, (c.m(t), c.m(a)): 1}
            c.counters = counters(n_pairs_placed=1, n_unsat_depth=1, n_links=2, n_kinds=2, n_index=2, n_layout=4)
        out[name] = c

    # v =(n parallel edges)=> m -> W: a level of 50 goes on, a level of 51 ends the search
    for n, name in ((50, "level_of_50_goes_on"), (51, "level_of_51_overflows")):
        c = Case(); a, t, v, W = _search_scene(c)
        m = c.vertex()
        for _ in range(n):
            c.edge(v, m)
        c.edge(m, W)
        c.pair(a, t)
        c.index = {a: [0], c.m(t): [1]}
        c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
        if n == 50:
            c.counters = counters(n_pairs_placed=1, n_reached=1, n_index=2, n_layout=4)
        else:
            c.links = {a: [(t, 0)], c.m(t): [(c.m(a), 0)]}
            c.mult = {(a, t): 1, (c.m(t), c.m(a)): 1}
            c.counters = counters(n_pairs_placed=1, n_unsat_overflow=1, n_links=2, n_kinds=2, n_index=2, n_layout=4)
        out[name] = c

    # 51 successors of v, one of them W (neither the first nor the last out-edge of v): a hit in the level that overflows wins
    c = Case(); a, t, v, W = _search_scene(c)
    m = c.vertex()
    for i in range(51):
        c.edge(v, W if i == 20 else m)
    c.pair(a, t)
    c.index = {a: [0], c.m(t): [1]}
    c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
    c.counters = counters(n_pairs_placed=1, n_reached=1, n_index=2, n_layout=4)
    out["w_among_51_successors_is_reached"] = c

    # a diamond v -> {x, y} -> z: z stands in level 2 TWICE, so its 26 out-edges to q make a level of 52 and the search ends; a search
    # that kept a visited set would see 26, go on and reach W behind q
    c = Case(); a, t, v, W = _search_scene(c)
    x, y, z, q = c.vertex(), c.vertex(), c.vertex(), c.vertex()
    c.edge(v, x); c.edge(v, y); c.edge(x, z); c.edge(y, z)
    for _ in range(26):
        c.edge(z, q)
    c.edge(q, W)
    c.pair(a, t)
    c.index = {a: [0], c.m(t): [1]}
    c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
    c.links = {a: [(t, 0)], c.m(t): [(c.m(a), 0)]}
    c.mult = {(a, t): 1, (c.m(t), c.m(a)): 1}
    c.counters = counters(n_pairs_placed=1, n_unsat_overflow=1, n_links=2, n_kinds=2, n_index=2, n_layout=4)
    out["diamond_counts_a_vertex_twice"] = c

    # the same diamond with 25 out-edges: 2 x 25 = 50 goes on, W is found in level 4
    c = Case(); a, t, v, W = _search_scene(c)
    x, y, z, q = c.vertex(), c.vertex(), c.vertex(), c.vertex()
    c.edge(v, x); c.edge(v, y); c.edge(x, z); c.edge(y, z)
    for _ in range(25):
        c.edge(z, q)
    c.edge(q, W)
    c.pair(a, t)
    c.index = {a: [0], c.m(t): [1]}
    c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
    c.counters = counters(n_pairs_placed=1, n_reached=1, n_index=2, n_layout=4)
    out["diamond_twice_25_goes_on"] = c

    # a self-loop at v, W in another component: fifteen levels of one vertex, no overflow
    c = Case(); a, t, v, W = _search_scene(c)
    c.edge(v, v)
    c.pair(a, t)
    c.index = {a: [0], c.m(t): [1]}
    c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
    c.links = {a: [(t, 0)], c.m(t): [(c.m(a), 0)]}
    c.mult = {(a, t): 1, (c.m(t), c.m(a)): 1}
    c.counters = counters(n_pairs_placed=1, n_unsat_depth=1, n_links=2, n_kinds=2, n_index=2, n_layout=4)
    out["self_loop_runs_15_levels"] = c

    # ---- the rules before the search
    # p1 = [a, b], p2 = [inv b]: x2 = [b] shares b with x1.  The two-edge read: forward (a, 0), (b, 0 - 11); reverse y = [inv b, inv a],
    # len = 30 + 11, pos = 41 - 10 = 31: (inv b, 31), (inv a, 31 - 11)
    c = Case(); vs = c.chain(2); a, b = 0, 2
    c.read([a, b]); c.read([c.m(b)])
    c.index = {a: [0], b: [0], c.m(b): [1]}
    c.layout = {a: [(0, 0, True)], b: [(-11, 0, True), (20, 1, False)], c.m(b): [(0, 1, True), (31, 0, False)], c.m(a): [(20, 0, False)]}
    c.counters = counters(n_pairs_placed=1, n_meet=1, n_index=3, n_layout=6)
    out["mates_share_an_edge"] = c

    # a = s -> v, t = v -> X: v == w
    c = Case(); vs = c.chain(2); a, t = 0, 2
    c.pair(a, t)
    c.index = {a: [0], c.m(t): [1]}
    c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
    c.counters = counters(n_pairs_placed=1, n_same_vertex=1, n_index=2, n_layout=4)
    out["v_equals_w"] = c

    # pair 0: the second read has no path; pair 1: the first has none
    c = Case(); a, t, v, W = _search_scene(c)
    c.read([a]); c.read(); c.read(); c.read([c.m(t)])
    c.index = {a: [0], c.m(t): [3]}
    c.layout = {a: [(0, 0, True)], c.m(a): [(20, 0, False)], c.m(t): [(0, 3, True)], t: [(20, 3, False)]}
    c.counters = counters(n_index=2, n_layout=4)
    out["one_read_without_a_path"] = c

    # both mates end on a: x2 = [inv a], w = the mirror of v, out of reach; unsatisfied, but p1.back == p2.back gives no link
    c = Case(); a, t, v, W = _search_scene(c)
    c.read([a]); c.read([a])
    c.index = {a: [0, 1]}
    c.layout = {a: [(0, 0, True), (0, 1, True)], c.m(a): [(20, 0, False), (20, 1, False)]}
    c.counters = counters(n_pairs_placed=1, n_unsat_depth=1, n_unsat_same_end=1, n_index=2, n_layout=4)
    out["unsatisfied_with_the_same_last_edge"] = c

    # pairs 0, 1, 3 link a -> t, pair 2 links a -> s (t < s as edge ids: pid 2 sorts behind pids 0, 1, 3)
    c = Case(); a, t, v, W = _search_scene(c)
    s = c.edge(c.vertex(), c.vertex())
    c.pair(a, t); c.pair(a, t); c.pair(a, s); c.pair(a, t)
    c.index = {a: [0, 2, 4, 6], c.m(t): [1, 3, 7], c.m(s): [5]}
    c.layout = {a: [(0, 0, True), (0, 2, True), (0, 4, True), (0, 6, True)], c.m(a): [(20, 0, False), (20, 2, False), (20, 4, False), (20, 6, False)],
                c.m(t): [(0, 1, True), (0, 3, True), (0, 7, True)], t: [(20, 1, False), (20, 3, False), (20, 7, False)],
                c.m(s): [(0, 5, True)], s: [(20, 5, False)]}
    c.links = {a: [(t, 0), (t, 1), (t, 3), (s, 2)], c.m(t): [(c.m(a), 0), (c.m(a), 1), (c.m(a), 3)], c.m(s): [(c.m(a), 2)]}
    c.mult = {(a, t): 3, (a, s): 1, (c.m(t), c.m(a)): 3, (c.m(s), c.m(a)): 1}
    c.counters = counters(n_pairs_placed=4, n_unsat_depth=4, n_links=8, n_kinds=4, n_index=8, n_layout=16)
    out["multiplicities_3_and_1"] = c

    # a palindromic edge P = u -> mirror of u behind g = x -> u: inv[P] == P.  The first read lies on P: v = the mirror of u, from where
    # only inv g leads on; links P -> t and inv t -> inv P = P.  P's own read: forward (P, 0), reverse (P, 20)
    c = Case(); W, X, x, u = c.vertex(), c.vertex(), c.vertex(), c.vertex()
    t = c.edge(W, X); g = c.edge(x, u); P = c.palindrome(u)
    assert c.m(P) == P
    c.pair(P, t)
    c.index = {P: [0], c.m(t): [1]}
    c.layout = {P: [(0, 0, True), (20, 0, False)], c.m(t): [(0, 1, True)], t: [(20, 1, False)]}
    c.links = {P: [(t, 0)], c.m(t): [(P, 0)]}
    c.mult = {(P, t): 1, (c.m(t), P): 1}
    c.counters = counters(n_pairs_placed=1, n_unsat_depth=1, n_links=2, n_kinds=2, n_index=2, n_layout=4)
    out["palindromic_edge"] = c

    # ---- the layout
    # e0 .. e3 of 30, 40, 50, 60 bases = 11, 21, 31, 41 K-mers.  Mates have no paths.
    #   read 0 [e0] offset 5, 10 bases:    forward (e0, 5); reverse len 30, pos 30 - 15 = 15: (e0', 15)
    #   read 2 [e0, e1] offset 3, 30:      forward (e0, 3), (e1, 3 - 11 = -8); reverse y = [e1', e0'], len 40 + 11 = 51, pos 51 - 33 = 18:
    #                                      (e1', 18), (e0', 18 - 21 = -3)
    #   read 4 [e0 .. e3] offset 7, 100:   forward (e0, 7), (e3, 7 - 11 = -4) -- only e0's K-mers come off; walking the path would give
    #                                      7 - 11 - 21 - 31 = -56; reverse y = [e3', e2', e1', e0'], len 60 + 31 + 21 + 11 = 123,
    #                                      pos 123 - 107 = 16: (e3', 16), (e0', 16 - 41 = -25) -- walking would give -77
    c = Case(); vs = [c.vertex() for _ in range(5)]
    e0, e1, e2, e3 = (c.edge(vs[i], vs[i + 1], 30 + 10 * i) for i in range(4))
    c.read([e0], 5, 10); c.read(); c.read([e0, e1], 3, 30); c.read(); c.read([e0, e1, e2, e3], 7, 100); c.read()
    c.index = {e0: [0, 2, 4], e1: [2, 4], e2: [4], e3: [4]}
    c.layout = {e0: [(3, 2, True), (5, 0, True), (7, 4, True)], c.m(e0): [(-25, 4, False), (-3, 2, False), (15, 0, False)],
                e1: [(-8, 2, True)], c.m(e1): [(18, 2, False)], e3: [(-4, 4, True)], c.m(e3): [(16, 4, False)]}
    c.counters = counters(n_index=7, n_layout=10)
    out["paths_of_1_2_and_4_edges"] = c

    # one edge e of 30 bases: read 0 [e] at offset -4, read 2 [e] at offset 6, read 4 [e'] at offset 25, 10 bases: its reverse entry
    # lies on e at 30 - 35 = -5.  Negative positions sort in front as signed values
    c = Case(); e = c.edge(c.vertex(), c.vertex())
    c.read([e], -4); c.read(); c.read([e], 6); c.read(); c.read([c.m(e)], 25); c.read()
    c.index = {e: [0, 2], c.m(e): [4]}
    c.layout = {e: [(-5, 4, False), (-4, 0, True), (6, 2, True)], c.m(e): [(14, 2, False), (24, 0, False), (25, 4, True)]}
    c.counters = counters(n_index=3, n_layout=6)
    out["negative_positions_sort_as_signed"] = c

    # ties.  Reads 0, 2, 6 at offset 5 of e (10, 12 and 10 bases): three forward entries at 5, in read order; reverse 15, 13, 15.
    # Read 4 on the palindromic edge P at offset 10: forward (P, 10) and reverse (P, 30 - 20 = 10): forward first
    c = Case(); x, u = c.vertex(), c.vertex()
    e = c.edge(x, u); P = c.palindrome(u)
    c.read([e], 5, 10); c.read(); c.read([e], 5, 12); c.read(); c.read([P], 10, 10); c.read(); c.read([e], 5, 10); c.read()
    c.index = {e: [0, 2, 6], P: [4]}
    c.layout = {e: [(5, 0, True), (5, 2, True), (5, 6, True)], c.m(e): [(13, 2, False), (15, 0, False), (15, 6, False)],
                P: [(10, 4, True), (10, 4, False)]}
    c.counters = counters(n_index=4, n_layout=8)
    out["ties_by_read_then_forward_first"] = c

    # ---- the index: read 0 crosses a twice ([a, lp, a] round the circle u -> v -> u, offset 2, 60 bases), its mate lies on a
    #   read 0: forward (a, 2), (a, 2 - 11 = -9); reverse y = [a', lp', a'], len 30 + 11 + 11 = 52, pos 52 - 62 = -10: (a', -10), (a', -21)
    #   the pair: x2 = [a'], no shared edge, w = the mirror of v; fifteen levels round the circle; p1.back == p2.back == a
    c = Case(); u, v = c.vertex(), c.vertex()
    a = c.edge(u, v); lp = c.edge(v, u)
    c.read([a, lp, a], 2, 60); c.read([a])
    c.index = {a: [0, 0, 1], lp: [0]}
    c.layout = {a: [(-9, 0, True), (0, 1, True), (2, 0, True)], c.m(a): [(-21, 0, False), (-10, 0, False), (20, 1, False)]}
    c.counters = counters(n_pairs_placed=1, n_unsat_depth=1, n_unsat_same_end=1, n_index=4, n_layout=6)
    out["read_crosses_an_edge_twice"] = c
    return out


# ---- generated cases ---------------------------------------------------------------------------------------------------------------
SEEDS = (2, 3, 4)              # chosen on the CPU: at each the model alone meets every condition of seed_conditions


def random_case(seed, n_reads=2000):
    """-> (hbv, inv, paths, read_len): a mirrored random graph of a few hundred edges (K = 20, edges of 20 .. 120 bases) with two hubs of
    55 out-edges, cycles and three palindromic edges; reads are random walks of 1 .. 5 edges at offsets in [-50, first edge's length),
    one in ten without a path; a mate is the mirror image of a walk that starts near the read's end (satisfied, same vertex, shared
    edge), of the read's own path turned round, or of a walk anywhere in the graph; pure Python, the same on every machine"""
    import random
    rng = random.Random(seed)
    c = Case()
    vs = [c.vertex() for _ in range(90)]
    anyv = lambda: rng.choice(vs) ^ (rng.random() < 0.15)                     # mostly the forward half, so that the halves are joined thinly
    for _ in range(130):
        c.edge(anyv(), anyv(), rng.randint(20, 120))
    for hub in rng.sample(vs, 2):
        c.edge(anyv(), hub, rng.randint(20, 120))
        for _ in range(55):
            c.edge(hub, anyv(), rng.randint(20, 120))
    for u in rng.sample(vs, 3):
        c.palindrome(u, rng.randint(20, 120))
    out_edges = {}
    for e, (u, v, _) in enumerate(c.b.edges):
        out_edges.setdefault(u, []).append(e)
    right = [v for _, v, _ in c.b.edges]
    n_edges = len(c.b.edges)

    def walk(first, n):
        p = [first]
        while len(p) < n and out_edges.get(right[p[-1]]):
            p.append(rng.choice(out_edges[right[p[-1]]]))
        return p

    def mirrored(p):
        return [c.m(e) for e in reversed(p)]

    for _ in range(n_reads // 2):
        p1 = walk(rng.randrange(n_edges), rng.randint(1, 5))
        how = rng.random()
        nxt = out_edges.get(right[p1[-1]])
        if how < 0.35 and nxt:                                               # nearby: up to three edges on, then the mate's walk
            gap = walk(rng.choice(nxt), rng.randint(1, 4))
            x2 = walk(gap[-1], rng.randint(1, 5))
        elif how < 0.42 and nxt:                                             # the mate's walk starts at the read's last vertex
            x2 = walk(rng.choice(nxt), rng.randint(1, 5))
        elif how < 0.48:                                                     # the mate's walk starts inside the read's
            x2 = walk(rng.choice(p1), rng.randint(1, 5))
        elif how < 0.51:                                                     # both mates end on the same edge
            x2 = mirrored(walk(p1[-1], 1) if rng.random() < 0.5 else p1)
        else:                                                                # far away
            x2 = walk(rng.randrange(n_edges), rng.randint(1, 5))
        for p in (p1, mirrored(x2)):
            if rng.random() < 0.1:
                c.read()
            else:
                c.read(p, rng.randrange(-50, len(c.b.edges[p[0]][2])), rng.randint(50, 150))
    return c.inputs()


def seed_conditions(m):
    """what a generated case must exercise, judged on the model's result alone -> the list of what is missing"""
    missing = [k for k in COUNTERS if m.counters[k] < 1]
    if not (len(m.kind_mult) and int(max(m.kind_mult)) > 1):
        missing.append("a kind with multiplicity above 1")
    if not (len(m.layout_pos) and int(min(m.layout_pos)) < 0):
        missing.append("a negative layout position")
    return missing


# ---- recorded runs of the reference's invert and LayoutReads ------------------------------------------------------------------------
INPUTS = ["t.hbv", "t.paths", "frag_reads_orig.fastb", "t.inv"]
OUTPUTS = ["t.index.txt", "t.layout.txt"]
# cases the reference could not be run on -> its message; they stay on literals and model
NOT_RECORDED = {}
_INPUTS = {}


def inputs_of(name):
    """the inputs of a hand-made case, or of the generated case random_<seed>, made once"""
    if name not in _INPUTS:
        _INPUTS[name] = random_case(int(name[len("random_"):])) if name.startswith("random_") else cases()[name].inputs()
    return _INPUTS[name]


def recorded():
    return [n for n in sorted(cases()) + [f"random_{s}" for s in SEEDS] if n not in NOT_RECORDED]


def reference_run(name, workdir):
    """stages the case's inputs in workdir (reads of the case's lengths, every base A: LayoutReads asks for the sizes only; t.inv, the
    case's own involution, one integer per line), puts the recorded t.index.txt and t.layout.txt beside them (recording: runs
    oracle/_ref/ref_step5 at 1 thread and at 4, which must agree) -> ({edge: [read ids]}, {edge: [(pos, id, forward)]}), in the
    reference's order"""
    h, inv, paths, read_len = inputs_of(name)
    F.write_hbv(os.path.join(workdir, "t.hbv"), h)
    F.write_paths(os.path.join(workdir, "t.paths"), *paths)
    off = np.zeros(len(read_len) + 1, np.uint64); np.cumsum(read_len, out=off[1:])
    F.write_fastb(os.path.join(workdir, "frag_reads_orig.fastb"), *F.pack_bases(np.zeros(int(off[-1]), np.uint8), off))
    with open(os.path.join(workdir, "t.inv"), "w") as f:
        f.write("".join(f"{int(x)}\n" for x in inv))

    def run():
        from oracle import oracle5
        got = []
        for threads in (1, 4):
            oracle5.run_reference5(workdir, "open", threads)
            got.append([open(os.path.join(workdir, o), "rb").read() for o in OUTPUTS])
        assert got[0] == got[1], f"{name}: the reference's result at 4 threads is not its result at 1"
    reference_outputs(f"step5_open_{name}", workdir, INPUTS, OUTPUTS, run)
    rows = [[[int(x) for x in line.split()] for line in open(os.path.join(workdir, o)).read().split("\n")[:-1]] for o in OUTPUTS]
    assert len(rows[0]) == len(rows[1]) == h.n_edges
    index = {e: l for e, l in enumerate(rows[0]) if l}
    layout = {e: [(l[j], l[j + 1], bool(l[j + 2])) for j in range(0, len(l), 3)] for e, l in enumerate(rows[1]) if l}
    return index, layout

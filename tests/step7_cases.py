"""Inputs of the Step-7 tests: hand-made contig graphs with hand-written lines and their LITERAL outcomes (derived by hand from the
reference text, src/paths/long/large/MakeGaps.cc and Lines.cc), generated graphs for the shapes at which a kernel can go wrong, and the
recorded runs of the reference's own main (tests/golden/refruns/step7_*).

A case is a dict: hbv, inv, paths, lines (formats.Lines), nested (the same as lists), npairs (None: LINKS reads what LINES counts),
min_line, min_link_count, and for a hand-made case `expect`, a dict of literal outcomes (see check_expect).

Recorded runs.
  step7_s6_<fixture>   the reference's main with ``--from_step 6 --to_step 6`` on the recorded clean graph and paths of a Step-4 fixture
                       (refruns/step4_<fixture>_s<min_size>/) staged as t.large_K.final.hbv/.paths beside its reads: t.contig.hbv/.paths,
                       t.fin.lines and t.fin.lines.npairs.  LINES must give the recorded npairs byte for byte.
  step7_s7_<case>      the reference's main with ``--from_step 7`` on t.contig.hbv/.paths, t.fin.lines and t.fin.lines.npairs of a case:
                       t_assembly_raw.gfa, t_assembly.lines, t_assembly.lines.npairs and stdout.  `planted` is two blocks of 7 kb around
                       150 bases no read covers, 2,482 pairs of error-free 150-base reads from 700-base fragments, taken through the
                       reference's own Steps 2-6 (its contig files are tests/golden/step7_planted.*); the others are hand-made cases
                       of this file, built with real sequences.
  step7_fn_<case>      the reference's own GetTol, GetLineLengths, GetLineNpairs and MakeGaps (without its cleanup, verbose) called on
                       EVERY hand-made and generated case as it stands (oracle/ref_step7_driver.cc): t.lines.txt, t.gaps.txt and
                       t.verbose.txt -- see lines_run, gaps_run, check_lines_record and check_gaps_record.
Every run is recorded at 1 thread and at 4; the two had to agree, the 1-thread files are kept."""
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT, reference_outputs
from w2rap_contigger_amd import formats as F

K = 20
LONG = 6000               # K-mers of a contig that passes min_line 5000


# ---------------------------------------------------------------------------------------------------------------- the builder
_REAL = False             # what Contigs(real=None) builds: hand_cases(real=True) sets it while it builds its graphs


class Contigs:
    """A contig graph from vertices and edges given in K-mers, the mirror image of everything added: vertex v has the mirror v ^ 1, the
    edge e (u -> v) the mirror e ^ 1 (v ^ 1 -> u ^ 1), so inv[e] = e ^ 1.  Adjacency lists sorted by vertex, ties in insertion order, as a
    HyperBasevector built by AddEdge holds them.  real: the edges get sequences that overlap by K - 1 (every vertex a random (K-1)-mer),
    for the cases the reference's main reads; otherwise the bases are zeros -- Step 7 reads lengths only."""

    def __init__(self, seed=1, real=None, K=K):
        self.K, self.real, self.rng = K, _REAL if real is None else real, np.random.default_rng(seed)
        self.edges, self.nv, self.J, self.pairs = [], 0, {}, []

    def v(self):
        self.nv += 2
        if self.real:
            j = self.rng.integers(0, 4, self.K - 1).astype(np.uint8)
            self.J[self.nv - 2] = j; self.J[self.nv - 1] = (3 - j[::-1]).astype(np.uint8)
        return self.nv - 2

    def e(self, u, v, kmers):
        """-> the edge's id; its mirror is id + 1"""
        n = kmers + self.K - 1
        if self.real:
            assert n >= 2 * (self.K - 1), "a real edge holds both vertices' (K-1)-mers"
            s = np.concatenate([self.J[u], self.rng.integers(0, 4, n - 2 * (self.K - 1)).astype(np.uint8), self.J[v]])
        else:
            s = np.zeros(n, np.uint8)
        self.edges.append((u, v, s)); self.edges.append((v ^ 1, u ^ 1, (3 - s[::-1]).astype(np.uint8)))
        return len(self.edges) - 2

    def contig(self, kmers=LONG):
        return self.e(self.v(), self.v(), kmers)

    def chain(self, kmers):
        """edges in a row -> their ids"""
        vs = [self.v() for _ in range(len(kmers) + 1)]
        return [self.e(vs[i], vs[i + 1], k) for i, k in enumerate(kmers)]

    def pair(self, p1, p2, n=1):
        """n pairs whose reads have the paths p1 and p2 (p2 as the second read itself lies: on the other strand)"""
        self.pairs += [(list(p1), list(p2))] * n

    def link(self, a, b, n):
        """n pairs with read 1 on a and read 2 on the mirror of b: the nears (a, b) and (b ^ 1, a ^ 1), n times each"""
        self.pair([a], [b ^ 1], n)

    def hbv(self):
        frm = [[] for _ in range(self.nv)]; to = [[] for _ in range(self.nv)]
        for e, (u, v, _) in enumerate(self.edges):
            frm[u].append((v, e)); to[v].append((u, e))
        for l in frm + to:
            l.sort(key=lambda x: x[0])
        fo = np.zeros(self.nv + 1, np.uint64); t_o = np.zeros(self.nv + 1, np.uint64)
        np.cumsum([len(x) for x in frm], out=fo[1:]); np.cumsum([len(x) for x in to], out=t_o[1:])
        ln = np.array([len(s) for _, _, s in self.edges], np.uint32)
        if self.real:
            off = np.zeros(len(self.edges) + 1, np.uint64)
            np.cumsum(ln, out=off[1:])
            pk, bo, ln = F.pack_bases(np.concatenate([s for _, _, s in self.edges]), off)
        else:
            bo = np.zeros(len(ln) + 1, np.uint64)
            np.cumsum((ln.astype(np.uint64) + 3) // 4, out=bo[1:])
            pk = np.zeros(int(bo[-1]), np.uint8)
        return F.HBV(self.K, fo, np.array([v for l in frm for v, _ in l], np.int32), np.array([e for l in frm for _, e in l], np.int32),
                     t_o, np.array([e for l in to for _, e in l], np.int32), pk, bo, ln)

    def case(self, lines=(), npairs=None, min_line=5000, min_link_count=3, expect=None):
        """lines: hand-written lines (nested lists); every edge that none of them names gets a line of its own IN FRONT of them (GetTol:
        the last line that names an edge wins).  npairs: None, one value for every line, or the list"""
        E = len(self.edges)
        named = {e for line in lines for cell in line for path in cell for e in path}
        nested = [[[[e]]] for e in range(E) if e not in named] + [[[list(p) for p in cell] for cell in line] for line in lines]
        po = np.zeros(2 * len(self.pairs) + 1, np.uint64)
        flat = [p for pr in self.pairs for p in pr]
        if flat:
            np.cumsum([len(p) for p in flat], out=po[1:])
        paths = (np.zeros(len(flat), np.int32), po, np.array([e for p in flat for e in p], np.int32))
        if npairs is not None and np.ndim(npairs) == 0:
            npairs = [int(npairs)] * len(nested)
        return dict(hbv=self.hbv(), inv=np.arange(E, dtype=np.int32) ^ 1, paths=paths, lines=F.Lines.from_nested(nested), nested=nested,
                    npairs=None if npairs is None else np.array(npairs, np.int32), min_line=min_line, min_link_count=min_link_count, expect=expect or {})


def mirror_line(line):
    """the line of the mirror edges: cells and paths reversed, every edge e ^ 1 (the paths of a cell keep their order)"""
    return [[[e ^ 1 for e in reversed(p)] for p in cell] for cell in reversed(line)]


# ---------------------------------------------------------------------------------------------------------------- literal cases
# Edge ids: the builder numbers edges in creation order, 2 per call (forward, mirror).  R: link -> reason name (formats of step7.REASONS).
def _two(n, a_kmers=LONG, seed=1):
    g = Contigs(seed)
    a, b = g.contig(a_kmers), g.contig()
    g.link(a, b, n)
    return g, a, b


def hand_cases(real=False):
    """name -> case.  real: the same graphs, lines, pairs and literal outcomes with real sequences (what the reference's main reads)"""
    global _REAL
    _REAL = real
    try:
        return _hand_cases()
    finally:
        _REAL = False


def _hand_cases():
    out = {}
    # ---- count 2 and 3 at min_link_count 3.  A = 0, B = 2; the pair names the lines of A, A', B', B: npairs n each (part LINES feeds LINKS)
    g, a, b = _two(2)
    out["count_2"] = g.case(expect=dict(npairs=[2, 2, 2, 2], llens=[LONG] * 4, reasons={(0, 2): "count", (3, 1): "count"}, gaps=[], n_nears=4, n_near_kinds=2, n_links=2))
    g, a, b = _two(3)
    out["count_3"] = g.case(expect=dict(npairs=[3, 3, 3, 3], reasons={(0, 2): "accepted", (3, 1): "accepted"}, gaps=[(0, 2), (3, 1)], gap_inv=[1, 0], n_sym_deleted=0, n_sym_added=0,
                                        near_max1=[3, 0, 0, 3], near_max2=[0, 3, 3, 0], n_pass_placed=6, n_pass_none=0))
    # ---- llens at min_line - 1 and at min_line
    g, a, b = _two(3, 4999)
    out["line_4999"] = g.case(expect=dict(llens=[4999, 4999, LONG, LONG], reasons={(0, 2): "line", (3, 1): "line"}, gaps=[]))
    g, a, b = _two(3, 5000)
    out["line_5000"] = g.case(expect=dict(reasons={(0, 2): "accepted", (3, 1): "accepted"}, gaps=[(0, 2), (3, 1)]))
    # ---- the coverage ratio in double.  Equal lengths 6000: cov = 100.0 * n / 6000.0.  n = 6 and 5: 0.1 / 0.08333333333333333 is
    # 1.2000000000000002 in double, minus 1.0 = 0.20000000000000018 > 0.2: REJECTED at this length; at equal lengths 5000 (cov 0.12 and
    # 0.1) the quotient is 1.2 and 1.2 - 1.0 = 0.19999999999999996: passes.  (Python's float is the same IEEE double.)
    g, a, b = _two(3)
    assert (100.0 * 6 / 6000.0) / (100.0 * 5 / 6000.0) - 1.0 > 20.0 / 100.0
    out["cov_6_5_len_6000"] = g.case(npairs=[6, 6, 5, 5], expect=dict(reasons={(0, 2): "coverage", (3, 1): "coverage"}, gaps=[]))
    g = Contigs(1); a, b = g.contig(5000), g.contig(5000); g.link(a, b, 3)
    assert not (100.0 * 6 / 5000.0) / (100.0 * 5 / 5000.0) - 1.0 > 20.0 / 100.0 and (100.0 * 6 / 5000.0) / (100.0 * 5 / 5000.0) - 1.0 == 0.19999999999999996
    out["cov_6_5_len_5000"] = g.case(npairs=[6, 6, 5, 5], expect=dict(reasons={(0, 2): "accepted", (3, 1): "accepted"}, gaps=[(0, 2), (3, 1)]))
    g = Contigs(1); a, b = g.contig(5000), g.contig(5000); g.link(a, b, 3)
    assert (100.0 * 601 / 5000.0) / (100.0 * 500 / 5000.0) - 1.0 > 20.0 / 100.0
    out["cov_601_500"] = g.case(npairs=[601, 601, 500, 500], expect=dict(reasons={(0, 2): "coverage", (3, 1): "coverage"}, gaps=[]))
    # no pairs on one side: inf rejects; none on both: NaN passes
    g, a, b = _two(3)
    out["cov_zero_one_side"] = g.case(npairs=[0, 0, 5, 5], expect=dict(reasons={(0, 2): "coverage", (3, 1): "coverage"}, gaps=[]))
    g, a, b = _two(3)
    out["cov_zero_both"] = g.case(npairs=0, expect=dict(reasons={(0, 2): "accepted", (3, 1): "accepted"}, gaps=[(0, 2), (3, 1)]))
    # ---- max_alt equal to count, and count + 1.  A = 0, B = 2, C = 4
    g = Contigs(2); a, b, c = g.contig(), g.contig(), g.contig(); g.link(a, b, 3); g.link(a, c, 3)
    out["alt_equal"] = g.case(npairs=10, expect=dict(reasons={(0, 2): "accepted", (0, 4): "accepted", (3, 1): "accepted", (5, 1): "accepted"}, n_not_one_to_one=4, gaps=[],
                                                    near_max1=[3, 0, 0, 3, 0, 3], near_max2=[0, 3, 3, 0, 3, 0]))
    g = Contigs(2); a, b, c = g.contig(), g.contig(), g.contig(); g.link(a, b, 3); g.link(a, c, 4)
    out["alt_count_plus_1"] = g.case(npairs=10, expect=dict(reasons={(0, 2): "alt", (0, 4): "accepted", (3, 1): "alt", (5, 1): "accepted"}, gaps=[(0, 4), (5, 1)], gap_inv=[1, 0],
                                                           near_max1=[4, 0, 0, 3, 0, 4], near_max2=[0, 4, 3, 0, 4, 0]))
    # ---- a hang of 800 K-mers and of 801: e (0) -> v -> {e1 (2, the hang), e2 (4, 30 K-mers)}, dead ends; B = 6; 3 pairs from e1 to B
    for hang in (800, 801):
        g = Contigs(3); u, v, w1, w2 = g.v(), g.v(), g.v(), g.v()
        e = g.e(u, v, LONG); e1 = g.e(v, w1, hang); e2 = g.e(v, w2, 30); b = g.contig(); g.link(e1, b, 3)
        if hang == 800:       # e turns sink-like (its mirror source-like on the reversed graph): the reads on e1 count for e
            exp = dict(tom=[0, 1, 0, 1, 0, 1, 6, 7], dist_to_end=[800, 800, 0, 0, 0, 0, 0, 0], sink_like=[1, 1, 1, 0, 1, 0, 1, 1], source_like=[1, 1, 0, 1, 0, 1, 1, 1],
                       n_group_loop1=6, n_group_loop2=0, reasons={(0, 6): "accepted", (7, 1): "accepted"}, gaps=[(0, 6), (7, 1)])
        else:
            exp = dict(tom=list(range(8)), dist_to_end=[0] * 8, sink_like=[0, 1, 1, 0, 1, 0, 1, 1], source_like=[1, 0, 0, 1, 0, 1, 1, 1], n_group_loop1=0,
                       reasons={(2, 6): "line", (7, 3): "line"}, gaps=[])
        out[f"hang_{hang}"] = g.case(npairs=10, expect=exp)
    # ---- e2 at 3 steps and at 4: e1 -> a -> b -> c (-> d)
    g = Contigs(4); e1, a, b, c = g.chain([LONG, 100, 100, LONG]); g.link(e1, c, 3)
    out["steps_3"] = g.case(npairs=10, expect=dict(n_close=[0, 0, 0, 2], n_links=0, n_pred_start=0, gaps=[]))
    g = Contigs(4); e1, a, b, c, d = g.chain([LONG, 100, 100, 100, LONG]); g.link(e1, d, 3)
    out["steps_4"] = g.case(npairs=10, expect=dict(n_close=[0, 0, 0, 0], n_links=2, reasons={(0, 8): "accepted", (9, 1): "accepted"}, gaps=[(0, 8), (9, 1)]))
    # ---- an intermediate at 1500 K-mers and at 1501, at the first level (e1 -> a -> c) and at the second (e1 -> a -> b -> c, a + b)
    for ka in (1500, 1501):
        g = Contigs(5); e1, a, c = g.chain([LONG, ka, LONG]); g.link(e1, c, 3)
        out[f"inter_{ka}"] = g.case(npairs=10, expect=dict(n_close=[0, 0, 2, 0], n_links=0) if ka == 1500 else dict(n_close=[0, 0, 0, 0], n_links=2, gaps=[(0, 4), (5, 1)]))
        g = Contigs(5); e1, a, b, c = g.chain([LONG, 700, ka - 700, LONG]); g.link(e1, c, 3)
        out[f"inter2_{ka}"] = g.case(npairs=10, expect=dict(n_close=[0, 0, 0, 2], n_links=0) if ka == 1500 else dict(n_close=[0, 0, 0, 0], n_links=2, gaps=[(0, 6), (7, 1)]))
    # ---- the predecessor start.  p (0): s -> t; e1 (2): t -> u; a (4): t -> x; b (6): x -> y; c (8): y -> z.  From e1 the only way on is p,
    # 6000 K-mers, never stepped from; from the root p: a, b, then c by the last step.  The mirror near (c', e1') has no such root and is 4
    # steps away: it becomes the link, and the forced symmetry adds (e1, c).  One pair from e1 to p: e2 IS the predecessor; its mirror near
    # (p', e1') is one step (e1' enters the left vertex of p')
    for extra in (False, True):
        g = Contigs(6); s, t, u, x, y, z = (g.v() for _ in range(6))
        p = g.e(s, t, LONG); e1 = g.e(t, u, LONG); a = g.e(t, x, 100); b = g.e(x, y, 100); c = g.e(y, z, LONG)
        g.link(e1, c, 3)
        if not extra:
            g.link(e1, p, 1)
            exp = dict(n_near_kinds=4, n_pred_start=2, n_close=[1, 1, 0, 1], n_links=1, reasons={(9, 3): "accepted"}, n_sym_added=1, n_sym_deleted=0, gaps=[(2, 8), (9, 3)], gap_inv=[1, 0])
        else:                 # a second edge into t: no predecessor root, nothing close
            g.e(g.v(), t, LONG)
            exp = dict(n_near_kinds=2, n_pred_start=0, n_close=[0, 0, 0, 0], n_links=2, reasons={(2, 8): "accepted", (9, 3): "accepted"}, n_sym_added=0, gaps=[(2, 8), (9, 3)])
        out["pred_start" if not extra else "pred_start_two_in"] = g.case(npairs=10, expect=exp)
    # ---- a line of 500 K-mers and of 501
    g, a, b = _two(3, 500)
    out["ignore_500"] = g.case(npairs=10, expect=dict(n_pass_placed=6, n_pass_none=6, n_nears=0, n_links=0, gaps=[]))
    g, a, b = _two(3, 501)
    out["ignore_501"] = g.case(npairs=10, expect=dict(n_pass_none=0, n_nears=6, reasons={(0, 2): "line", (3, 1): "line"}, gaps=[]))
    # ---- tom of tom, two nears that become one link under tom, and the numbering that decides the pass in which an edge turns sink-like.
    # A tree of short hangs (30 K-mers each) below e0 (6000): e0 -> {e, x}; e -> {e1, e2}; x -> {x1, xa}; x1 -> {x2, xb}; x2 -> {l1, l2}.
    # An edge fires once both its children are sink-like, in the same sweep when they are numbered below it, in the next otherwise.
    # first numbering (x 0, e 2, e0 4, x1 6, x2 8, e1 10, e2 12, xa 14, xb 16, l1 18, l2 20): x2 and e fire in pass 1, x1 in pass 2, x in
    # pass 3 -- and only then e0, BEHIND e's turn of pass 3: tom[e] = e0 comes after tom[e1] = tom[e] = e.  tom[tom[e1]] != tom[e1].
    # second numbering (e0 0, x 2, e 4, ...): in pass 3 e0's turn comes BEFORE x fires: e0 never turns sink-like.
    def tree(order):
        g = Contigs(7); vs = {n: g.v() for n in ("u0", "v0", "v1", "vx", "vx1", "vx2", "d1", "d2", "da", "db", "dl1", "dl2")}
        ends = dict(e0=("u0", "v0", LONG), e=("v0", "v1", 30), x=("v0", "vx", 30), e1=("v1", "d1", 30), e2=("v1", "d2", 30), x1=("vx", "vx1", 30), xa=("vx", "da", 30),
                    x2=("vx1", "vx2", 30), xb=("vx1", "db", 30), l1=("vx2", "dl1", 30), l2=("vx2", "dl2", 30))
        ids = {n: g.e(vs[ends[n][0]], vs[ends[n][1]], ends[n][2]) for n in order}
        return g, ids
    names = ("x", "e", "e0", "x1", "x2", "e1", "e2", "xa", "xb", "l1", "l2")
    g, t = tree(names)
    b = g.contig()            # 22
    g.link(t["e1"], b, 3); g.link(t["e"], b, 3)
    fwd = [[[t["e0"]] + [t[n] for n in names if n != "e0"]]]
    tom_f = dict(x=4, e=4, e0=4, x1=0, x2=0, e1=2, e2=2, xa=0, xb=0, l1=0, l2=0)
    tom = list(range(24))
    for n, v in tom_f.items():
        tom[t[n]] = v; tom[t[n] + 1] = v + 1
    dist = [0] * 24
    for n, v in dict(x=90, e=30, e0=120, x1=60, x2=30).items():
        dist[t[n]] = dist[t[n] + 1] = v
    # the nears (e, B) and (e0, B) -- e1's reads under tom, e's reads under tom -- are two links (e0, B) after the second tom: both pass
    # the filters, and the one-to-one rule deletes them and their mirrors
    # (the mirror line written out: it must START with e0', the edge MakeGaps looks for at lines[l].front()[0][0])
    out["tom_of_tom"] = g.case(lines=[fwd, [[[e ^ 1 for e in fwd[0][0]]]]], npairs=10,
                               expect=dict(tom=tom, dist_to_end=dist, n_near_kinds=4, n_pred_start=1, links=[(4, 22, 3), (4, 22, 3), (23, 5, 3), (23, 5, 3)],
                                           n_reason=[4, 0, 0, 0, 0, 0, 0], n_not_one_to_one=4, gaps=[], near_max1_at={4: 3, 2: 3, 23: 3}, near_max2_at={22: 3, 3: 3, 5: 3}))
    names2 = ("e0", "x", "e", "x1", "x2", "e1", "e2", "xa", "xb", "l1", "l2")
    g, t = tree(names2)
    tom_f = dict(e0=0, x=2, e=4, x1=2, x2=2, e1=4, e2=4, xa=2, xb=2, l1=2, l2=2)
    tom = list(range(22))
    for n, v in tom_f.items():
        tom[t[n]] = v; tom[t[n] + 1] = v + 1
    sink = [0] * 22
    for n in names2:
        sink[t[n]] = int(n != "e0")          # forward: everything but e0 (leaves are dead ends, the others fired)
        sink[t[n] + 1] = int(n == "e0")      # mirrors: only e0' ends in a dead end (the mirror of e0's source vertex)
    out["numbering_keeps_e0_out"] = g.case(npairs=10, expect=dict(tom=tom, sink_like=sink))
    # ---- 0 to 4 simple bubbles between A0 and the end of its line; the A behind a bubble are 900 K-mers (no hang fires: 50 + 900 > 800)
    for nb in range(5):
        g = Contigs(8 + nb); vs = [g.v() for _ in range(2 * nb + 2)]
        line = [[[g.e(vs[0], vs[1], LONG)]]]
        for i in range(nb):
            b1 = g.e(vs[2 * i + 1], vs[2 * i + 2], 50); b2 = g.e(vs[2 * i + 1], vs[2 * i + 2], 60); an = g.e(vs[2 * i + 2], vs[2 * i + 3], 900)
            line += [[[b1], [b2]], [[an]]]
        b = g.contig()
        a0, last = line[0][0][0], line[-1][0][0]
        g.link(a0, b, 3)
        if nb <= 3:
            exp = dict(reasons={(a0, b): "accepted", (b + 1, a0 + 1): "accepted"}, n_advanced=2 if nb else 0, gaps=sorted([(last, b), (b + 1, last + 1)]), tom=list(range(len(g.edges))))
        else:
            exp = dict(reasons={(a0, b): "left_end", (b + 1, a0 + 1): "right_end"}, gaps=[])
        # npairs in proportion to the lengths (B, B', the line, its mirror): the coverage test passes
        out[f"bubbles_{nb}"] = g.case(lines=[line, mirror_line(line)], npairs=[600, 600] + [(LONG + 955 * nb) // 10] * 2, expect=exp)
    # ---- a gap added for symmetry: B' (3) sits in a hand-written line that ends in Z (4), so (B', A') fails the line-end test
    g = Contigs(20); a, b, z = g.contig(), g.contig(), g.contig(); g.link(a, b, 3)
    out["symmetry_adds"] = g.case(lines=[[[[b + 1]], [[z]], [[z]]]], npairs=[10, 10, 10, 10, 30],        # (the line of 18000 K-mers has three times the pairs)
                                  expect=dict(reasons={(0, 2): "accepted", (3, 1): "left_end"}, n_unique=1, n_sym_added=1, n_sym_deleted=0, gaps=[(0, 2), (3, 1)], gap_inv=[1, 0]))
    # ---- gaps deleted for symmetry: A 0, B 2, C 4, Z 6.  (C, B) fails at the left end (C's line ends in Z), (B', A') at the right end
    # (A''s line starts with Z'); (A, B) and (B', C') are accepted, neither has its mirror, and B' on the left of one / B on the right of
    # the other forbids adding it: both are deleted, and the reference prints "adding -2 gaps"
    g = Contigs(21); a, b, c, z = g.contig(), g.contig(), g.contig(), g.contig(); g.link(a, b, 3); g.link(c, b, 3)
    out["symmetry_deletes"] = g.case(lines=[[[[c]], [[z]], [[z]]], [[[z + 1]], [[z + 1]], [[a + 1]]]], npairs=[10, 10, 10, 10, 30, 30],
                                     expect=dict(reasons={(0, 2): "accepted", (3, 1): "right_end", (3, 5): "accepted", (4, 2): "left_end"}, n_not_one_to_one=0, n_unique=2,
                                                 n_sym_deleted=2, n_sym_added=-2, gaps=[]))
    # ---- an overlinked edge: A1 (0) -> bubble (2, 4) -> M (6); (A1, B) advances to (M, B) and meets (M, C)
    g = Contigs(22); vs = [g.v() for _ in range(4)]
    a1 = g.e(vs[0], vs[1], LONG); b1 = g.e(vs[1], vs[2], 50); b2 = g.e(vs[1], vs[2], 60); m = g.e(vs[2], vs[3], LONG); b, c = g.contig(), g.contig()
    g.link(a1, b, 3); g.link(m, c, 3)
    line = [[[a1]], [[b1], [b2]], [[m]]]
    out["overlinked"] = g.case(lines=[line, mirror_line(line)], npairs=[10, 10, 10, 10, 20, 20], expect=dict(n_reason=[4, 0, 0, 0, 0, 0, 0], n_not_one_to_one=0, n_advanced=2, n_unique=4, n_sym_added=0,
                                                                                       n_sym_deleted=0, n_overlinked=4, gaps=[]))
    _median_cases(out)
    _in_edge_cases(out)
    _list_cases(out)
    return out


MEDIANS = {3: ((50, 50, 70), 50), 4: ((40, 60, 60, 81), 60), 5: ((90, 30, 30, 75, 30), 30), 6: ((10, 20, 30, 41, 50, 60), 35), 7: ((5, 5, 5, 5, 9, 9, 9), 5)}


def _median_cases(out):
    """A line a (0) -> a cell of n parallel paths -> c, n = 3 .. 7 with ties among the lengths (Lines.h:84-96: one path its length, two
    their mean, more the median of the sorted lengths, for an even n the mean of the two middle ones, in int), and a cell of one path of
    two edges beside two of one.  B is as long as the line: 3 pairs from c to B and 2 whose first read walks a, the first path and c: every
    pair names all four lines (npairs 5 each, equal coverage), (c, B) has 5 nears and is accepted, (a, B) and (p, B) have 2.
    (Edges of 5 K-mers hold no two (K-1)-mers: these graphs are built without sequences in either mode.)"""
    def finish(name, g, a, first, c, line, med):
        b = g.contig(2 * LONG + med)
        g.link(c, b, 3); g.pair([a] + first + [c], [b ^ 1], 2)
        R = {(c, b): "accepted", (b + 1, c + 1): "accepted"}
        for e in [a] + first:
            R[(e, b)] = "count"; R[(b + 1, e + 1)] = "count"
        out[name] = g.case(lines=[line, mirror_line(line)], expect=dict(llens=[2 * LONG + med] * 4, npairs=[5] * 4, tol=[2, 3] * (b // 2) + [0, 1], reasons=R, gaps=[(c, b), (b + 1, c + 1)],
                                                                        gap_inv=[1, 0], near_max1_at={c: 5, a: 2, b + 1: 5}, near_max2_at={b: 5, c + 1: 5, a + 1: 2}))
    for n, (lens, med) in MEDIANS.items():
        g = Contigs(40 + n, real=False); v = [g.v() for _ in range(4)]
        a = g.e(v[0], v[1], LONG); ps = [g.e(v[1], v[2], k) for k in lens]; c = g.e(v[2], v[3], LONG)
        finish(f"median_{n}", g, a, [ps[0]], c, [[[a]], [[p] for p in ps], [[c]]], med)
    # x (100) and y (110) in a row beside z (200) and z2 (300): 210 is the median
    g = Contigs(50, real=False); v = [g.v() for _ in range(5)]
    a = g.e(v[0], v[1], LONG); x = g.e(v[1], v[2], 100); y = g.e(v[2], v[3], 110); z = g.e(v[1], v[3], 200); z2 = g.e(v[1], v[3], 300); c = g.e(v[3], v[4], LONG)
    finish("median_two_edge_path", g, a, [x, y], c, [[[a]], [[z2], [x, y], [z]], [[c]]], 210)


def _in_edge_cases(out):
    """The search through in-edges (MakeGaps.cc:244-252: a node's children are the out-edges of its right vertex AND the in-edges of its
    left vertex).  e1 (0): s -> t, 6000 K-mers; 3 pairs from e1 to e2, every edge a line of its own, npairs 10 everywhere.  A vertex whose
    single in-edge would become a predecessor root (0 K-mers, which would take the limit away) has a second one, `o`."""
    def scene(seed):
        g = Contigs(seed); s, t = g.v(), g.v()
        return g, s, t, g.e(s, t, LONG)
    two = lambda e1, e2: dict(n_near_kinds=2, n_pred_start=0, n_close=[0, 0, 0, 0], n_links=2, reasons={(e1, e2): "accepted", (e2 + 1, e1 + 1): "accepted"}, n_sym_added=0,
                              gaps=[(e1, e2), (e2 + 1, e1 + 1)], gap_inv=[1, 0])
    # e2 and o enter s: e2 is met at step 1 as an in-edge of e1's left vertex, which has no predecessor root.  The mirror near (e2', e1'):
    # e1' is the one edge into the left vertex of e2', the predecessor root itself (step 0)
    g, s, t, e1 = scene(60); e2 = g.e(g.v(), s, LONG); g.e(g.v(), s, LONG); g.link(e1, e2, 3)
    out["in_step_1"] = g.case(npairs=10, expect=dict(n_near_kinds=2, n_pred_start=1, n_close=[1, 1, 0, 0], n_links=0, gaps=[]))
    # n (100): t -> x, e2: y -> t.  From e1 out to n, then in: the in-edges of n's left vertex t are e1 and e2 (step 2).  The mirror near:
    # the left vertex t' of e2' has the one in-edge n', the predecessor root, whose out-edges are e2' and e1' (step 1)
    g, s, t, e1 = scene(61); n = g.e(t, g.v(), 100); e2 = g.e(g.v(), t, LONG); g.link(e1, e2, 3)
    out["out_in_step_2"] = g.case(npairs=10, expect=dict(n_near_kinds=2, n_pred_start=1, n_close=[0, 1, 1, 0], n_links=0, gaps=[]))
    for kn in (1500, 1501):
        # in, in: n (kn): x -> s, o -> s, e2: y -> x, z: x -> w.  n is expanded at 1500 K-mers (e2 at step 2) and not at 1501.  The mirror
        # near walks the same edges: n' is one of the two in-edges of the left vertex x' of e2', e1' the in-edge of the left vertex of n'
        g, s, t, e1 = scene(62); x = g.v(); n = g.e(x, s, kn); g.e(g.v(), s, LONG); e2 = g.e(g.v(), x, LONG); g.e(x, g.v(), LONG); g.link(e1, e2, 3)
        out[f"in_in_{kn}"] = g.case(npairs=10, expect=dict(n_near_kinds=2, n_pred_start=0, n_close=[0, 0, 2, 0], n_links=0, gaps=[]) if kn == 1500 else two(e1, e2))
        # in, in, in: a (700): x -> s, o -> s, b (kn - 700): y -> x, e2: q -> y, z: y -> w.  b, at depth 1, is expanded with 1500 K-mers
        # behind it and not with 1501; e2 enters the LEFT vertex of b
        g, s, t, e1 = scene(63); x, y = g.v(), g.v(); a = g.e(x, s, 700); g.e(g.v(), s, LONG); b = g.e(y, x, kn - 700); e2 = g.e(g.v(), y, LONG); g.e(y, g.v(), LONG); g.link(e1, e2, 3)
        out[f"in_in_in_{kn}"] = g.case(npairs=10, expect=dict(n_near_kinds=2, n_pred_start=0, n_close=[0, 0, 0, 2], n_links=0, gaps=[]) if kn == 1500 else two(e1, e2))
    # out, out, in: a (100): t -> u, c and c2 (100) out of u, e2: q -> u.  e2 is no child of a (it ENTERS a's right vertex); it enters the
    # left vertex of c (step 3).  The mirror near: in (c'), out (a'), out (e1'): step 3 by the other clause
    g, s, t, e1 = scene(64); u = g.v(); a = g.e(t, u, 100); c = g.e(u, g.v(), 100); c2 = g.e(u, g.v(), 100); e2 = g.e(g.v(), u, LONG); g.link(e1, e2, 3)
    out["out_out_in_step_3"] = g.case(npairs=10, expect=dict(n_near_kinds=2, n_pred_start=0, n_close=[0, 0, 0, 2], n_links=0, gaps=[]))
    # a first level of 140: 70 out-edges of t and 70 in-edges of s (x_i -> s), 100 K-mers each, all in one line (over the 500 K-mers
    # below which reads are ignored).  Behind the in-edges (children 70 .. 139 of the root): e2 -> x_64 and e3 -> x_1 (step 2), e4 -> m
    # (100) -> x_69 (step 3); behind the out-edge 66: e5 (step 2); the in-edge 67 itself (step 1).  The mirror nears: the left vertex of
    # e2', e3' and of the mirror of the in-edge 67 has one in-edge, the predecessor root -- for the last it IS e1' (step 0), for e2' and
    # e3' e1' is a child of it (step 1) --; m' is the predecessor root of e4' (step 2); e5' has none (out, out: step 2)
    g, s, t, e1 = scene(65)
    zs = [g.v() for _ in range(70)]; outs = [g.e(t, z, 100) for z in zs]
    xs = [g.v() for _ in range(70)]; ins = [g.e(x, s, 100) for x in xs]
    e2 = g.e(g.v(), xs[64], LONG); e3 = g.e(g.v(), xs[1], LONG); y = g.v(); m = g.e(y, xs[69], 100); e4 = g.e(g.v(), y, LONG); e5 = g.e(zs[66], g.v(), LONG)
    for e in (e2, e3, e4, e5, ins[67]):
        g.link(e1, e, 3)
    short = outs + ins + [m]
    out["hub_in_70"] = g.case(lines=[[[short]], [[[e + 1 for e in short]]]], npairs=10, min_line=50,
                              expect=dict(n_near_kinds=10, n_pred_start=4, n_close=[1, 3, 5, 1], n_links=0, gaps=[], n_nears=30))


def _list_cases(out):
    """y of exactly NEAR_LIST = 16 kept edges and of 17 (the list of k7_nears, and the walk beyond it), each near 3 times; 1, 3, 4 and 5
    distinct nears (a block of k7_close takes 4)."""
    for n in (16, 17):
        # A (0, 600 K-mers, as long as the others: equal coverage) and a chain of n edges of 600: 3 pairs from A whose second read walks
        # the whole chain.  Pass 1: x = [A], y = the chain; pass 2: x = the mirror chain, y = [A'].  2 n links of count 3, all accepted --
        # A on the left of n of them, A' on the right of the others: none is one-to-one
        g = Contigs(66 + n); a = g.contig(600); ch = g.chain([600] * n)
        g.pair([a], [e ^ 1 for e in reversed(ch)], 3)
        out[f"y_{n}"] = g.case(npairs=10, min_line=500, expect=dict(n_pass_placed=6, n_pass_y_long=3 * (n > 16), n_pass_none=0, n_nears=6 * n, n_near_kinds=2 * n, n_close=[0, 0, 0, 0], n_links=2 * n,
                                                                     n_reason=[2 * n, 0, 0, 0, 0, 0, 0], n_not_one_to_one=2 * n, gaps=[], near_max1_at={a: 3, ch[0] + 1: 3}, near_max2_at={a + 1: 3, ch[n - 1]: 3}))
    # two-sided: 3 pairs from a contig to another, the near and its mirror image.  one-sided: A -> three edges of 100 K-mers -> B, 3 pairs
    # whose first read walks all five and whose second lies on B'.  Pass 1: the short lines are ignored, x = [A, B], y = [B]: (A, B), and B
    # is in y; pass 2: x = [B'] is in y = [B', A']: no mirror near.  B is 4 steps from A: a link, accepted, its mirror added for symmetry
    for kinds, (double, single) in {1: (0, 1), 3: (1, 1), 4: (2, 0), 5: (2, 1)}.items():
        g = Contigs(80 + kinds); gaps = []
        for _ in range(double):
            a, b = g.contig(), g.contig(); g.link(a, b, 3); gaps += [(a, b), (b + 1, a + 1)]
        for _ in range(single):
            ch = g.chain([LONG, 100, 100, 100, LONG]); g.pair(ch, [ch[4] ^ 1], 3); gaps += [(ch[0], ch[4]), (ch[4] + 1, ch[0] + 1)]
        out[f"kinds_{kinds}"] = g.case(npairs=10, expect=dict(n_near_kinds=kinds, n_pred_start=0, n_close=[0, 0, 0, 0], n_links=kinds, n_reason=[kinds, 0, 0, 0, 0, 0, 0], n_not_one_to_one=0,
                                                              n_pass_none=3 * single, n_sym_added=single, n_sym_deleted=0, gaps=sorted(gaps)))


def check_expect(case, got):
    """holds a result -- anything with the arrays and counters of include/w2rap_step7.h by name: the model's dict or the library's
    Step7Result turned into one by as_dict -- to the literal outcomes of a hand-made case"""
    from w2rap_contigger_amd.step7 import REASONS
    for k, v in case["expect"].items():
        if k == "reasons":
            links = {}
            for f, t, r in zip(got["link_from"], got["link_to"], got["link_reason"]):
                links.setdefault((int(f), int(t)), set()).add(REASONS[int(r)])
            assert links == {ft: {r} for ft, r in v.items()}, (k, links)
        elif k == "links":
            assert [(int(f), int(t), int(n)) for f, t, n in zip(got["link_from"], got["link_to"], got["link_count"])] == v, k
        elif k == "gaps":
            assert [(int(f), int(t)) for f, t in zip(got["gap_from"], got["gap_to"])] == v, (k, list(got["gap_from"]), list(got["gap_to"]))
        elif k.endswith("_at"):
            assert {i: int(got[k[:-3]][i]) for i in v} == v, k
        elif k in got:
            assert [int(x) for x in got[k]] == [int(x) for x in v], (k, list(got[k]))
        else:
            c = got["counters"][k]
            assert (list(c) if isinstance(c, list) else c) == v, (k, c)


def as_dict(res):
    """a step7.Step7Result as the model's dict"""
    d = {k: v for k, v in res.arrays.items() if v is not None}
    d["counters"] = res.counters
    return d


# ---------------------------------------------------------------------------------------------------------------- generated cases
def random_case(n_contigs, n_pairs, seed, max_path=3, count_spread=4):
    """isolated contigs of mixed lengths (some under the 500 and the 5000 K-mer limits), a few bubbles and hangs; pairs between random
    places, in runs of random length, mates with no path among them"""
    rng = np.random.default_rng(seed)
    g = Contigs(seed)
    walks = []
    for i in range(n_contigs):
        kind = rng.integers(0, 6)
        if kind == 0:       # a line with a bubble
            vs = [g.v() for _ in range(4)]
            a = g.e(vs[0], vs[1], int(rng.integers(400, 7000))); b1 = g.e(vs[1], vs[2], 40); b2 = g.e(vs[1], vs[2], 45); c = g.e(vs[2], vs[3], int(rng.integers(30, 7000)))
            walks += [[a], [a, b1, c], [a, b2, c], [c]]
        elif kind == 1:     # a hang
            vs = [g.v() for _ in range(4)]
            a = g.e(vs[0], vs[1], int(rng.integers(400, 7000))); h1 = g.e(vs[1], vs[2], int(rng.integers(20, 900))); h2 = g.e(vs[1], vs[3], int(rng.integers(20, 900)))
            walks += [[a], [a, h1], [a, h2], [h1]]
        elif kind == 2:     # a chain of short edges between two long ones: the search
            ids = g.chain([LONG] + [int(rng.integers(100, 900)) for _ in range(int(rng.integers(1, 5)))] + [LONG])
            walks += [[ids[0]], [ids[-1]], ids[:2], ids[-2:]]
        else:
            walks.append([g.contig(int(rng.choice([300, 501, 4000, 5000, 6000, 7000])))])
    done = 0
    while done < n_pairs:
        n = min(int(rng.integers(1, count_spread + 1)), n_pairs - done)
        w1, w2 = walks[rng.integers(len(walks))], walks[rng.integers(len(walks))]
        p1 = w1[:max_path]; p2 = [e ^ 1 for e in reversed(w2[:max_path])]
        r = rng.integers(0, 10)
        g.pair([] if r == 0 else p1, [] if r == 1 else p2, n)
        done += n
    return g.case(min_line=int(rng.choice([400, 5000])))


def runs_case(counts=(1, 63, 64, 65, 256, 257, 1025)):
    """one pair of contigs per count: runs of that many equal nears"""
    g = Contigs(31)
    for n in counts:
        g.link(g.contig(), g.contig(), n)
    return g.case()


def long_paths_case():
    """paths of 0, 1, 9, 17 and 40 edges over chains whose edges have lines of their own: a pair that names more than PAIR_LINES lines (the
    spill path of LINES) and a y longer than NEAR_LIST (the rescan of the nears), beside ones that stay within both"""
    g = Contigs(32)
    c9, c17, c40 = g.chain([600] * 9), g.chain([600] * 17), g.chain([600] * 40)
    a = g.contig()
    rev = lambda p: [e ^ 1 for e in reversed(p)]
    for p1, p2 in (([], []), ([a], []), ([], [a]), (c9, rev(c9)), (c9, [a ^ 1]), ([a], rev(c9)), (c17, [a ^ 1]), ([a], rev(c17)), (c40, rev(c9)), (c9, rev(c40)), (c40, rev(c17)),
                   (c9[:8], rev(c9[:8])), (c9[:4], rev(c9[:4])), (c9 + c9, [a ^ 1])):
        g.pair(p1, p2, 2)
    return g.case(min_line=500)


def inverse_in_line_case():
    """an edge and its inverse in ONE line (a pair on it counts that line once), beside the same in two lines"""
    g = Contigs(33); a, b, c = g.contig(), g.contig(), g.contig()
    g.link(a, b, 3); g.link(b, c, 2); g.pair([a], [], 4)
    return g.case(lines=[[[[a, a + 1]]]])


def hub_case(deg=300):
    """the search through a hub: e1 -> h, `deg` parallel edges h -> h2, `deg` edges out of h2 and d, a long one (2 steps from e1); the
    last of the `deg` is continued by c (3 steps from e1: by the last step, which is asked, not enumerated) and c by c2 (4 steps from e1:
    a link; 3 from a parallel edge)"""
    g = Contigs(34); s, h, h2 = g.v(), g.v(), g.v()
    e1 = g.e(s, h, LONG)
    par = [g.e(h, h2, 100) for _ in range(deg)]
    for _ in range(deg - 1):
        g.e(h2, g.v(), 100)
    w, w2 = g.v(), g.v()
    last = g.e(h2, w, 100); c = g.e(w, w2, 100); c2 = g.e(w2, g.v(), LONG)
    d = g.e(h2, g.v(), LONG)
    g.link(e1, c, 3); g.link(e1, c2, 3); g.link(e1, d, 3); g.link(par[7], c2, 3); g.link(e1, last, 3)
    short = [e for e in range(0, len(g.edges), 2) if e not in (e1, c2, d)]       # one line for the 100-K-mer edges: over the 500 K-mers below which reads are ignored
    return g.case(lines=[[[short]], [[[e + 1 for e in short]]]], npairs=10, min_line=50)


def many_links_case(n=3000):
    """n contigs, one pair from each to the next: more distinct links than a scan tile holds"""
    g = Contigs(35)
    cs = [g.contig() for _ in range(n)]
    for i in range(n - 1):
        g.link(cs[i], cs[i + 1], 1)
    return g.case(min_link_count=1)


def generated_cases():
    out = {f"pairs_{n}": random_case(12, n, 100 + n) for n in (1, 63, 64, 65, 257)}
    out.update(random_2000=random_case(60, 2000, 7, count_spread=6), runs=runs_case(), long_paths=long_paths_case(), inverse_in_line=inverse_in_line_case(), hub_300=hub_case(),
               many_links=many_links_case())
    return out


# ---------------------------------------------------------------------------------------------------------------- recorded runs
REF_MAIN = os.path.join(ROOT, "oracle", "_ref", "w2rap-contigger-gpu")
S6_FIXTURES = ("errs2", "repeats_snps", "palindrome_circle")         # Step-4 fixtures (tests/step4_cases.py), at the min_size that deletes something
S6_OUTPUTS = ["t.contig.hbv", "t.contig.paths", "t.fin.lines", "t.fin.lines.npairs"]
S7_INPUTS = ["t.contig.hbv", "t.contig.paths", "t.fin.lines", "t.fin.lines.npairs"]
S7_OUTPUTS = ["t_assembly_raw.gfa", "t_assembly.lines", "t_assembly.lines.npairs"]
S7_HAND = ("count_2", "count_3", "alt_count_plus_1", "bubbles_2", "symmetry_adds", "symmetry_deletes")      # hand-made cases the reference's main has run


def _main_twice(workdir, args, outputs):
    """the reference's main at 1 thread and at 4 on copies of workdir; the outputs must agree; the 1-thread files are put into workdir"""
    res = []
    for t in (1, 4):
        d = os.path.join(workdir, f"threads{t}")
        shutil.copytree(workdir, d, ignore=shutil.ignore_patterns("threads*"))
        out = subprocess.run([REF_MAIN, "-r", "x", "-o", d, "-p", "t", "-t", str(t), "-m", "16"] + args, check=True, capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(t))).stdout
        res.append((d, [open(os.path.join(d, f), "rb").read() for f in outputs], re.findall(r"deleting (-?\d+) gaps and adding (-?\d+) gaps", out), out))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2], "the reference's outputs differ between 1 thread and 4"
    for f in outputs:
        shutil.copy(os.path.join(res[0][0], f), os.path.join(workdir, f))
    for d, *_ in res:
        shutil.rmtree(d)
    return "".join(f"deleting {d} gaps and adding {a} gaps to force symmetry\n" for d, a in res[0][2])      # (of stdout, the one line the tests read)


def step6_run(name, workdir):
    """stages a Step-4 fixture's recorded clean graph and paths as t.large_K.final.* beside its reads in workdir and puts the recorded
    outputs of the reference's Step 6 beside them -> (hbv, paths, Lines, npairs)"""
    import step4_cases as S4
    g, r, ms = S4.FIXTURES[name]
    src = os.path.join(GOLDEN, "refruns", f"step4_{name}_s{ms}")
    for s, d in ((os.path.join(src, "t.large_K.clean.hbv"), "t.large_K.final.hbv"), (os.path.join(src, "t.large_K.clean.paths"), "t.large_K.final.paths"),
                 (os.path.join(GOLDEN, f"{r}.fastb"), "frag_reads_orig.fastb"), (os.path.join(GOLDEN, f"{r}.qualp"), "frag_reads_orig.qualp")):
        shutil.copy(s, os.path.join(workdir, d))
    reference_outputs(f"step7_s6_{name}", workdir, ["t.large_K.final.hbv", "t.large_K.final.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp"], S6_OUTPUTS,
                      lambda: _main_twice(workdir, ["--from_step", "6", "--to_step", "6"], S6_OUTPUTS) and None)
    w = lambda f: os.path.join(workdir, f)
    return F.read_hbv(w("t.contig.hbv")), F.read_paths(w("t.contig.paths")), F.read_lines(w("t.fin.lines")), F.read_int_vec(w("t.fin.lines.npairs"))


def planted_case():
    g = lambda ext: os.path.join(GOLDEN, "step7_planted." + ext)
    h = F.read_hbv(g("contig.hbv"))
    lines = F.read_lines(g("fin.lines"))
    from w2rap_contigger_amd.step7 import involution
    return dict(hbv=h, inv=involution(h), paths=F.read_paths(g("contig.paths")), lines=lines, nested=lines.nested(), npairs=F.read_int_vec(g("fin.lines.npairs")),
                min_line=5000, min_link_count=3, expect={})


def step7_run(name, case, workdir):
    """writes the case as the four files the reference's Step 7 reads and puts its recorded outputs beside them
    -> (the text of t_assembly_raw.gfa, (deleted, added) as stdout has them)"""
    w = lambda f: os.path.join(workdir, f)
    F.write_hbv(w("t.contig.hbv"), case["hbv"]); F.write_paths(w("t.contig.paths"), *case["paths"]); F.write_lines(w("t.fin.lines"), case["lines"])
    F.write_int_vec(w("t.fin.lines.npairs"), case["npairs"] if case["npairs"] is not None else case["expect"]["npairs"])      # (what part LINES counts, as Step 6 would have written it)
    out = reference_outputs(f"step7_s7_{name}", workdir, S7_INPUTS, S7_OUTPUTS, lambda: _main_twice(workdir, ["--from_step", "7"], S7_OUTPUTS))
    m = re.findall(r"deleting (-?\d+) gaps and adding (-?\d+) gaps", out)
    assert len(m) == 1
    return open(w("t_assembly_raw.gfa")).read(), (int(m[0][0]), int(m[0][1]))


# ---------------------------------------------------------------------------------------------------------------- recorded calls
# step7_fn_<case>: the reference's public functions called on a case as it stands (oracle/ref_step7_driver.cc -> oracle/_ref/ref_step7):
# no sequences, the case's own involution as text.  `lines`: GetTol, GetLineLengths, GetLineNpairs -> t.lines.txt.  `gaps`: MakeGaps
# without its cleanup -> t.gaps.txt (every gap edge it appended, `e1 e2 mirror_index`, read from the edited graph) and its stdout,
# t.verbose.txt.  Of stdout the dated prefix of a line and the time after `done making gaps` are dropped: no clock enters a fixture.
REF_STEP7 = os.path.join(ROOT, "oracle", "_ref", "ref_step7")
FN_INPUTS = ["t.contig.hbv", "t.contig.paths", "t.fin.lines", "t.inv"]
FN_OUTPUTS = ["t.lines.txt", "t.gaps.txt", "t.verbose.txt"]
FN_QUIET = ("many_links",)                    # recorded with verbose = 0: 5,998 accepted links are 790 KB of text
BOUNDARY_PAIRS = (("count_2", "count_3"), ("line_4999", "line_5000"), ("alt_equal", "alt_count_plus_1"), ("hang_800", "hang_801"), ("steps_3", "steps_4"), ("inter_1500", "inter_1501"),
                  ("inter2_1500", "inter2_1501"), ("bubbles_3", "bubbles_4"), ("in_in_1500", "in_in_1501"), ("in_in_in_1500", "in_in_in_1501"))
_DATED = re.compile(r"^\S+ \S+ +\d+ \d\d:\d\d:\d\d \d{4}: ")


def _undated(text):
    return "".join(re.sub(r"(done making gaps), time used = .*", r"\1", _DATED.sub("", line)) + "\n" for line in text.splitlines())


def _ints(line):
    return [int(x) for x in line.split()]


def _fn_twice(workdir, case, verbose):
    """ref_step7 lines and ref_step7 gaps at 1 thread and at 4 on copies of workdir; the outputs must agree; the 1-thread files are put
    into workdir.  Where the case gives no npairs, MakeGaps reads what GetLineNpairs of the same run counted"""
    res = []
    for t in (1, 4):
        d = os.path.join(workdir, f"threads{t}")
        shutil.copytree(workdir, d, ignore=shutil.ignore_patterns("threads*"))
        env = dict(os.environ, OMP_NUM_THREADS=str(t))
        subprocess.run([REF_STEP7, "lines", d, str(t)], check=True, capture_output=True, env=env)
        if case["npairs"] is None:
            F.write_int_vec(os.path.join(d, "t.fin.lines.npairs"), _ints(open(os.path.join(d, "t.lines.txt")).read().split("\n")[2]))
        out = subprocess.run([REF_STEP7, "gaps", d, str(t), str(case["min_line"]), str(case["min_link_count"]), str(int(verbose))], check=True, capture_output=True, text=True, env=env).stdout
        with open(os.path.join(d, "t.verbose.txt"), "w") as fh:
            fh.write(_undated(out))
        res.append((d, [open(os.path.join(d, f), "rb").read() for f in FN_OUTPUTS]))
    assert res[0][1] == res[1][1], "the reference's outputs differ between 1 thread and 4"
    for f in FN_OUTPUTS:
        shutil.copy(os.path.join(res[0][0], f), os.path.join(workdir, f))
    for d, _ in res:
        shutil.rmtree(d)


def _fn_run(name, case, workdir):
    """stages the case in workdir (regenerated here; held to the record by SHA-256) and puts the recorded outputs beside it"""
    w = lambda f: os.path.join(workdir, f)
    F.write_hbv(w("t.contig.hbv"), case["hbv"]); F.write_paths(w("t.contig.paths"), *case["paths"]); F.write_lines(w("t.fin.lines"), case["lines"])
    with open(w("t.inv"), "w") as fh:
        fh.write("".join(f"{int(x)}\n" for x in case["inv"]))
    inputs = list(FN_INPUTS)
    if case["npairs"] is not None:
        F.write_int_vec(w("t.fin.lines.npairs"), case["npairs"])
        inputs.append("t.fin.lines.npairs")
    reference_outputs(f"step7_fn_{name}", workdir, inputs, FN_OUTPUTS, lambda: _fn_twice(workdir, case, name not in FN_QUIET))
    if case["npairs"] is None:                # as Step 6 would have written it: the recorded GetLineNpairs of this case
        F.write_int_vec(w("t.fin.lines.npairs"), _ints(open(w("t.lines.txt")).read().split("\n")[2]))


def lines_run(name, case, workdir):
    """-> dict(tol, llens, npairs) of the recorded GetTol, GetLineLengths and GetLineNpairs on the case"""
    _fn_run(name, case, workdir)
    rows = open(os.path.join(workdir, "t.lines.txt")).read().split("\n")
    assert len(rows) == 4 and rows[3] == ""
    return dict(tol=_ints(rows[0]), llens=_ints(rows[1]), npairs=_ints(rows[2]))


def _run_list(text):
    """`22^3,4,7^2` -> [(22, 3), (4, 1), (7, 2)]"""
    return [(int(x.split("^")[0]), int(x.split("^")[1]) if "^" in x else 1) for x in text.split(",") if x]


def parse_verbose(text):
    """MakeGaps' stdout -> dict(accepted: one dict per numbered entry -- e1, e2, count, lines ((tol, len) of either end), lefts and rights
    (the runs of nears1[e1] and nears2[e2]), left_group, right_group --, deleting: the links the one-to-one rule removed, symmetry:
    (deleted, added)).  Every line must be one the reference's text can have written."""
    acc, deleting, sym = [], [], []
    for line in text.splitlines():
        m = re.fullmatch(r"(\d+)\. \[(\d+)\] (\d+) --> (\d+)", line)
        if m:
            assert int(m[1]) == len(acc) + 1
            acc.append(dict(count=int(m[2]), e1=int(m[3]), e2=int(m[4])))
            continue
        m = re.fullmatch(r"lines: (\d+)\[len=(\d+)\], (\d+)\[len=(\d+)\]", line)
        if m:
            acc[-1]["lines"] = ((int(m[1]), int(m[2])), (int(m[3]), int(m[4])))
            continue
        m = re.fullmatch(r"(lefts|rights): ([\d^,]*)", line)
        if m:
            acc[-1][m[1]] = _run_list(m[2])
            continue
        m = re.fullmatch(r"(left|right) edge group: ([\d,]*)", line)
        if m:
            acc[-1][m[1] + "_group"] = [int(x) for x in m[2].split(",") if x]
            continue
        m = re.fullmatch(r"deleting (\d+) --> (\d+)", line)
        if m:
            deleting.append((int(m[1]), int(m[2])))
            continue
        m = re.fullmatch(r"deleting (-?\d+) gaps and adding (-?\d+) gaps to force symmetry", line)
        if m:
            sym.append((int(m[1]), int(m[2])))
            continue
        assert line in ("", "done making gaps"), line
    assert len(sym) == 1 and all(len(a) == 8 for a in acc)
    return dict(accepted=acc, deleting=deleting, symmetry=sym[0])


def gaps_run(name, case, workdir):
    """-> dict(gap_from, gap_to, gap_inv: the gap edges MakeGaps appended, in its order; symmetry; accepted and deleting, None for a case
    recorded without verbose) of the recorded MakeGaps on the case"""
    _fn_run(name, case, workdir)
    rows = [_ints(r) for r in open(os.path.join(workdir, "t.gaps.txt")).read().splitlines()]
    assert all(len(r) == 3 for r in rows)
    v = parse_verbose(open(os.path.join(workdir, "t.verbose.txt")).read())
    quiet = name in FN_QUIET
    assert not (quiet and (v["accepted"] or v["deleting"]))
    return dict(gap_from=[r[0] for r in rows], gap_to=[r[1] for r in rows], gap_inv=[r[2] for r in rows], symmetry=v["symmetry"], accepted=None if quiet else v["accepted"],
                deleting=None if quiet else v["deleting"])


def check_lines_record(rec, got):
    """tol, llens and -- where part LINES ran -- npairs of a result (see check_expect) are the recorded ones"""
    for k in ("tol", "llens") + (("npairs",) if got.get("npairs") is not None else ()):
        assert [int(x) for x in got[k]] == rec[k], k


def check_gaps_record(rec, got):
    """a result of part LINKS held to the recorded MakeGaps: the gaps with their own ids, in order; the accepted links as a multiset
    (ParallelSortSync leaves equal links in no stated order); per accepted link the longest runs of its nears, its edge groups and its
    lines; the count of the one-to-one rule; the symmetry counts"""
    from collections import Counter
    from w2rap_contigger_amd.step7 import REASONS
    for k in ("gap_from", "gap_to", "gap_inv"):
        assert [int(x) for x in got[k]] == rec[k], (k, list(got[k]), rec[k])
    assert (got["counters"]["n_sym_deleted"], got["counters"]["n_sym_added"]) == rec["symmetry"]
    if rec["accepted"] is None:
        return
    mine = Counter((int(f), int(t), int(n)) for f, t, n, r in zip(got["link_from"], got["link_to"], got["link_count"], got["link_reason"]) if REASONS[int(r)] == "accepted")
    assert mine == Counter((a["e1"], a["e2"], a["count"]) for a in rec["accepted"])
    tom, tol, llens = [int(x) for x in got["tom"]], [int(x) for x in got["tol"]], [int(x) for x in got["llens"]]
    groups = {}
    for e, t in enumerate(tom):
        groups.setdefault(t, []).append(e)
    for a in rec["accepted"]:
        e1, e2 = a["e1"], a["e2"]
        assert max(n for _, n in a["lefts"]) == int(got["near_max1"][e1]) and max(n for _, n in a["rights"]) == int(got["near_max2"][e2]), (e1, e2)
        assert a["left_group"] == groups.get(e1, []) and a["right_group"] == groups.get(e2, []), (e1, e2)
        assert a["lines"] == ((tol[e1], llens[tol[e1]]), (tol[e2], llens[tol[e2]])), (e1, e2)
    assert got["counters"]["n_not_one_to_one"] == len(rec["deleting"])


_COMP = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s.translate(_COMP)[::-1]


def gfa_half_gaps(text):
    """Gap edges have no bases and RemoveUnneededVertices2 keeps their ends: an S line without sequence.  A gap and its mirror image are two
    such segments, and GFADump writes a connection once, from its smaller canonical edge: of the two flanks of a gap, each is stated once,
    on the gap or -- mirrored -- on its mirror.  `L a sa b sb` says that a (reverse-complemented when sa is '-') is followed by b
    (likewise).  -> {empty segment: {"left": the sequence in front of it, "right": the sequence behind it}}, sides nobody states missing"""
    seq, links = {}, []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] == "S":
            seq[f[1]] = f[2]
        elif f[0] == "L":
            links.append((f[1], f[2], f[3], f[4]))
    empty = {s: {} for s, q in seq.items() if q == ""}
    orient = lambda s, sign: seq[s] if sign == "+" else _rc(seq[s])
    flip = {"+": "-", "-": "+"}
    for a, sa, b, sb in links:
        assert not (a in empty and b in empty)
        if b in empty:                             # a(sa) -> gap(sb); with sb '-' that is gap+ -> a(flipped)
            side, s = ("left", orient(a, sa)) if sb == "+" else ("right", orient(a, flip[sa]))
            assert side not in empty[b]
            empty[b][side] = s
        elif a in empty:                           # gap(sa) -> b(sb)
            side, s = ("right", orient(b, sb)) if sa == "+" else ("left", orient(b, flip[sb]))
            assert side not in empty[a]
            empty[a][side] = s
    return empty


def check_gaps_against_gfa(text, case, gap_from, gap_to, gap_inv):
    """The gaps of a result ARE the gaps of the reference's t_assembly_raw.gfa, by flank sequence (the cleanup renumbers): as many empty
    segments as gaps; every stated flank is the left flank of exactly one gap of the result, or the right flank of one (the overlinked rule
    leaves an edge on either side of one gap at most); a segment's two statements name the same gap; no gap is named by two segments; the
    statements are one per segment in all, two per gap and its mirror image, and each such couple is named"""
    codes, off = case["hbv"].edge_codes()
    s = lambda e: "".join("ACGT"[c] for c in codes[int(off[e]):int(off[e + 1])])
    n = len(gap_from)
    by = {"left": {s(int(e)): k for k, e in enumerate(gap_from)}, "right": {s(int(e)): k for k, e in enumerate(gap_to)}}
    assert len(by["left"]) == n and len(by["right"]) == n
    segs = gfa_half_gaps(text)
    assert len(segs) == n, (len(segs), n)
    used, stated = set(), 0
    for g, sides in segs.items():
        ks = {by[side].get(q, -1) for side, q in sides.items()}
        stated += len(sides)
        if ks:
            assert len(ks) == 1 and -1 not in ks, (g, ks)
            assert not (ks & used)
            used |= ks
    assert stated == n
    assert all(k in used or int(gap_inv[k]) in used for k in range(n)) and all(int(i) >= 0 for i in gap_inv)
    return n

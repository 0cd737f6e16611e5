"""Inputs for AddNewStuff (w2rap_step5_add_new_stuff): hand-made cases with literal expected paths, three seeded random cases, the
recorded runs of the reference's own AddNewStuff on them (tests/golden/refruns/step5_addref_<case>/) and the recorded runs of the
reference's builder on an encoding of `allx` (step5_add_<case>/).  Shared by test_step5_add_model.py (CPU: the model against the records
and the literals) and test_gpu_step5_add.py (the library against records, literals and model).

A literal is written in SEQUENCES, not ids: the expected path of a read is a list of edge sequences of the new graph (slices of the
case's genome) and an offset; the numbering of the new graph (lexicographic by default) never enters."""
import os
from dataclasses import dataclass

import numpy as np

import step5_add_model as M
from w2rap_contigger_amd import formats as F

rc = M.rc


def R(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint8)


def alt(b):
    return np.uint8((int(b) + 1) & 3)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
class Gb:
    """a graph given edge by edge, (sequence, left vertex, right vertex); the reverse complement of every edge is added between the mirror
    vertices.  Forward edge i gets id 2i, its reverse complement 2i + 1; vertex v mirrors to v + nv"""

    def __init__(self, K, nv):
        self.K, self.nv, self.e = K, nv, []

    def add(self, seq, a, b):
        self.e.append((np.asarray(seq, np.uint8), a, b))
        return 2 * (len(self.e) - 1)

    def hbv(self):
        seqs, left, right = [], [], []
        for s, a, b in self.e:
            seqs += [s, rc(s)]; left += [a, b + self.nv]; right += [b, a + self.nv]
        return hbv_of(self.K, seqs, np.array(left, np.int64), np.array(right, np.int64), 2 * self.nv)


def hbv_of(K, seqs, left, right, nv):
    n = len(seqs)
    ids = np.arange(n, dtype=np.int64)
    kf = np.lexsort((ids, right, left)); kt = np.lexsort((ids, left, right))      # AddEdge: by target, ties in id order
    from_off = np.zeros(nv + 1, np.uint64); np.cumsum(np.bincount(left, minlength=nv), out=from_off[1:])
    to_off = np.zeros(nv + 1, np.uint64); np.cumsum(np.bincount(right, minlength=nv), out=to_off[1:])
    codes = np.concatenate(seqs) if n else np.zeros(0, np.uint8)
    off = np.zeros(n + 1, np.uint64); np.cumsum([len(s) for s in seqs], out=off[1:])
    pk, bo, ln = F.pack_bases(codes, off)
    return F.HBV(K, from_off, right[kf].astype(np.int32), kf.astype(np.int32), to_off, kt.astype(np.int32), pk, bo, ln)


def empty_hbv(K):
    z = np.zeros(1, np.uint64)
    return F.HBV(K, z, np.zeros(0, np.int32), np.zeros(0, np.int32), z.copy(), np.zeros(0, np.int32), np.zeros(0, np.uint8), z.copy(), np.zeros(0, np.uint32))


def built(K, seqs):
    """the unipath graph of the sequences, by the builder itself"""
    return M.rebuild(empty_hbv(K), list(seqs)).hbv


def edge_id(h, seq):
    key = np.asarray(seq, np.uint8).tobytes()
    for e, s in enumerate(M.edge_seqs(h)):
        if s.tobytes() == key:
            return e
    raise KeyError("no such edge")


def pack_seqs(seqs):
    n = len(seqs)
    codes = np.concatenate(seqs).astype(np.uint8) if n else np.zeros(0, np.uint8)
    off = np.zeros(n + 1, np.uint64); np.cumsum([len(s) for s in seqs], out=off[1:])
    return F.pack_bases(codes, off)


def make_paths(plist, offsets):
    n = len(plist)
    off = np.zeros(n + 1, np.uint64); np.cumsum([len(p) for p in plist], out=off[1:])
    return np.asarray(offsets, np.int32), off, np.array([e for p in plist for e in p], np.int32)


class Case:
    """reads: list of (bases, quals or a constant, path in old ids, offset, expected (offset, [edge sequences]) or None)"""

    def __init__(self, h, new=(), min_gain=5):
        self.h, self.new, self.min_gain, self.reads, self.counters, self.edges = h, [np.asarray(s, np.uint8) for s in new], min_gain, [], {}, None

    def read(self, bases, quals, path, offset, expect=None):
        q = np.full(len(bases), quals, np.uint8) if np.isscalar(quals) else np.asarray(quals, np.uint8)
        self.reads.append((np.asarray(bases, np.uint8), q, list(path), offset, expect))

    def inputs(self):
        """-> (hbv, paths, reads, quals, new_seqs)"""
        reads = pack_seqs([r[0] for r in self.reads])
        quals = np.concatenate([r[1] for r in self.reads]) if self.reads else np.zeros(0, np.uint8)
        return self.h, make_paths([r[2] for r in self.reads], [r[3] for r in self.reads]), reads, quals, self.new

    def check(self, res):
        """res: anything with hbv, path_offset, path_off, path_edges, counters: the literals"""
        if self.edges is not None:
            assert sorted(s.tobytes() for s in M.edge_seqs(res.hbv)) == sorted(np.asarray(s, np.uint8).tobytes() for s in self.edges), "the new graph's edges"
        pf = res.path_off.astype(np.int64)
        for i, r in enumerate(self.reads):
            if r[4] is None:
                continue
            off, seqs = r[4]
            assert [int(e) for e in res.path_edges[pf[i]:pf[i + 1]]] == [edge_id(res.hbv, s) for s in seqs], f"read {i}: path"
            assert int(res.path_offset[i]) == off, f"read {i}: offset"
        for k, v in self.counters.items():
            assert res.counters[k] == v, f"{k}: {res.counters[k]}, expected {v}"


def both(seqs):
    return [x for s in seqs for x in (np.asarray(s, np.uint8), rc(s))]


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------
def chain3(K=80, seed=1):
    """three edges in a row, no new_stuff: they merge into one, the offsets gain left3; nothing to extend into (a sink)"""
    g = R(np.random.default_rng(seed), 5 * K)
    a, b = 2 * K, 3 * K                                   # e0 = g[0:a], e1 = g[a-K+1:b], e2 = g[b-K+1:]
    G = Gb(K, 4)
    e0 = G.add(g[:a], 0, 1); e1 = G.add(g[a - K + 1:b], 1, 2); e2 = G.add(g[b - K + 1:], 2, 3)
    c = Case(G.hbv())
    c.edges = both([g])
    rd = lambda s, n=150: g[s:s + n]
    c.read(rd(a - K + 1 + 5), 30, [e1], 5, (a - K + 1 + 5, [g]))
    c.read(rd(100), 30, [e0, e1, e2], 100, (100, [g]))
    c.read(rd(0), 30, [e0], -10, (-10, [g]))                          # negative offset: translated, never extended
    c.read(rd(0), 30, [], 7, (7, []))                                 # empty path: kept, offset and all
    c.read(rc(g)[20:170], 30, [e2 + 1], 20, (20, [rc(g)]))
    c.read(np.concatenate([g[5 * K - 100:], np.zeros(50, np.uint8)]), 30, [e2], 5 * K - 100 - (b - K + 1), (5 * K - 100, [g]))     # hangs over the end of a sink by 50: not tried
    c.counters = dict(n_all=6 + 4, n_junctions=4, n_all_bases=2 * (a + (b - a + K - 1) + (5 * K - b + K - 1)) + 4 * (K + 1), n_unipaths=1,
                      n_tr_empty=1, n_tr_first=5, n_tr_walked=0, n_tr_cleared=0, n_ext_tried=0)
    return c


def gap_bridge(K=80, seed=2):
    """two edges with a gap between them, a patch that overlaps K bases on each side: one edge"""
    g = R(np.random.default_rng(seed), 600 + 2 * K)
    x, y = 250, 350 + K
    G = Gb(K, 4)
    e0 = G.add(g[:x], 0, 1); e1 = G.add(g[y:], 2, 3)
    c = Case(G.hbv(), [g[x - K:y + K]])
    c.edges = both([g])
    c.read(g[200:350], 30, [e0], 200, (200, [g]))
    c.read(g[y + 40:y + 190], 30, [e1], 40, (y + 40, [g]))
    c.read(rc(g)[10:160], 30, [e1 + 1], 10, (10, [rc(g)]))
    c.counters = dict(n_all=5, n_junctions=0, n_unipaths=1, n_tr_first=3, n_ext_tried=0)
    return c


def branch_patch(K=80, seed=3):
    """a patch with a SNP opens a bubble inside edges: to3 has several entries.  e0 = g[0:450] and e1 = g[300:700] overlap (the old graph
    is no unipath graph: TranslatePaths does not ask), so to3[e0] = [L, A] and to3[e1] = [L, A, R] overlap by TWO; the chain c0, c1 merges
    into H, so to3[c0] = to3[c1] = [H] overlap by ONE"""
    rng = np.random.default_rng(seed)
    g = R(rng, 700); h = R(rng, 300)
    p = 400
    g2 = g.copy(); g2[p] = alt(g[p])
    G = Gb(K, 7)
    e0 = G.add(g[:450], 0, 1); e1 = G.add(g[300:], 2, 3)
    c0 = G.add(h[:160], 4, 5); c1 = G.add(h[160 - K + 1:], 5, 6)
    c = Case(G.hbv(), [g2[p - 100:p + 100]])
    L, A, A2, Rr = g[:p], g[p - K + 1:p + K], g2[p - K + 1:p + K], g[p + 1:]
    c.edges = both([L, A, A2, Rr, h])
    qs = np.full(150, 30, np.uint8)
    # starts in the first piece's last K-1 bases: stays on the first piece; then ext = 100 over A (K K-mers) and R, against A2: gain 30
    c.read(g[350:500], qs, [e0], 350, (350, [L, A, Rr]))
    # starts past the first piece: walks
    c.read(g[450:600], qs, [e1], 150, (450 - (p - K + 1), [A, Rr]))          # [A] at 129, ext 120: R alone covers behind A
    c.read(g[500:650], qs, [e1], 200, (500 - (p + 1), [Rr]))
    # two maps overlapping by two entries: [L, A] + [L, A, R] -> [L, A, R]; start 420 walks onto A at 99
    c.read(g[420:570], qs, [e0, e1], 420, (420 - (p - K + 1), [A, Rr]))
    # overlapping by one entry: [H] + [H] -> [H]; start 310 >= 300 runs off the end: cleared, the offset stays
    c.read(h[:150], qs, [c0, c1], 310, (310, []))
    c.read(h[100:250], qs, [c0, c1], 100, (100, [h]))
    # the read carries the patch's allele: extends onto A2
    c.read(g2[350:500], qs, [e0], 350, (350, [L, A2, Rr]))
    c.counters = dict(n_junctions=2, n_tr_first=3, n_tr_walked=3, n_tr_cleared=1, n_tr_empty=0, n_ext_tried=4, n_ext_extended=4)
    return c


def extensions(K=80, seed=4):
    """ExtendPath on a SNP bubble L -> a0 | a1 -> R (the read ends on the SNP or behind it), and on a branch T -> x0 | x1 whose arms end at
    once.  No new_stuff: the graph comes back as it went in"""
    rng = np.random.default_rng(seed)
    g = R(rng, 600); t = R(rng, 230)
    p = 300
    g2 = g.copy(); g2[p] = alt(g[p])
    t2 = t.copy(); t2[200] = alt(t[200])
    G = Gb(K, 9)
    L = G.add(g[:p], 0, 1); a0 = G.add(g[p - K + 1:p + K], 1, 2); a1 = G.add(g2[p - K + 1:p + K], 1, 2); Rr = G.add(g[p + 1:], 2, 3)
    T = G.add(t[:200], 4, 5); x0 = G.add(t[200 - K + 1:], 5, 6); x1 = G.add(t2[200 - K + 1:], 5, 7)
    c = Case(G.hbv())
    sL, sa0, sa1, sR, sT = g[:p], g[p - K + 1:p + K], g2[p - K + 1:p + K], g[p + 1:], t[:200]
    c.edges = both([sL, sa0, sa1, sR, sT, t[200 - K + 1:], t2[200 - K + 1:]])

    def rd(s, q_snp, n=150, src=g):
        q = np.full(n, 30, np.uint8)
        if s <= p < s + n:
            q[p - s] = q_snp
        return src[s:s + n], q
    c.read(*rd(150, 30), [L], 150, (150, [sL]))                       # ext = 0: the read ends with the edge
    c.read(*rd(151, 5), [L], 151, (151, [sL, sa0]))                   # ext = 1: the SNP itself, gain = min_gain
    c.read(*rd(151, 4), [L], 151, (151, [sL]))                        # gain = min_gain - 1
    c.read(*rd(151, 0), [L], 151, (151, [sL]))                        # a mismatch at quality 0: gain 0
    c.read(*rd(215, 30), [L], 215, (215, [sL, sa0]))                  # ext = 65
    c.read(*rd(215, 30, src=g2), [L], 215, (215, [sL, sa1]))
    c.read(*rd(100, 30), [L], -5, (-5, [sL]))                         # negative offset
    c.read(*rd(0, 30), [], 0, (0, []))                                # empty path
    c.read(np.concatenate([g[p + 1 + 200:], np.zeros(51, np.uint8)]), 30, [Rr], 200, (200, [sR]))          # the last edge ends in a sink (the read hangs over by 51)
    c.read(t[100:230].tolist() + [0] * 20, 30, [T], 100, (100, [sT]))                 # ext = 50, the arms have 30 K-mers and end: nothing covers
    c.counters = dict(n_unipaths=7, n_junctions=2 * (2 + 2 + 2), n_tr_empty=1, n_tr_first=9, n_ext_tried=6, n_ext_extended=3, n_ext_ambiguous=2, n_ext_no_cover=1,
                      n_ext_too_many=0)
    return c


def k_edges(K=80, seed=5):
    """three SNPs K + 1 apart: the edges between the bubbles have exactly K bases.  A 250-base read extends over two of them"""
    g = R(np.random.default_rng(seed), 800)
    ps = [300, 300 + K + 1, 300 + 2 * (K + 1)]
    seqs = [g]
    for p in ps:
        v = g[p - K:p + K + 1].copy(); v[K] = alt(g[p]); seqs.append(v)
    h = built(K, both(seqs))
    c = Case(h)
    L = g[:ps[0]]; arm = lambda p: g[p - K + 1:p + K]; mid = lambda p: g[p + 1:p + 1 + K]
    assert len(mid(ps[0])) == K
    c.read(g[220:470], 30, [edge_id(h, L)], 220, (220, [L, arm(ps[0]), mid(ps[0]), arm(ps[1]), mid(ps[1]), arm(ps[2])]))      # ext = 170 = K + 1 + K + 1 + 8
    c.counters = dict(n_unipaths=10, n_ext_tried=1, n_ext_extended=1)
    return c


def ladder(extra_tip, K=20, seed=6):
    """bubbles of 2, 4, 2 and 3 arms, 24 apart: a read that runs 90 bases past its edge lists 1 + 2 (2 + 8 + 16) + 48 = 101 extensions and is
    extended; with one more arm at the first vertex -- a tip that ends at once -- the list has 102 entries and the read is left alone"""
    rng = np.random.default_rng(seed)
    g = R(rng, 400)
    ps, arms = [200, 224, 248, 272], [2, 4, 2, 3]
    seqs = [g]
    for p, n in zip(ps, arms):
        for k in range(1, n):
            v = g[p - K:p + K + 1].copy(); v[K] = np.uint8((int(g[p]) + k) & 3); seqs.append(v)
    if extra_tip:
        tip = np.concatenate([g[ps[0] - K:ps[0]], [(int(g[ps[0]]) + 2) & 3], [(int(g[ps[0] + 1]) + 1) & 3, (int(g[ps[0] + 2]) + 1) & 3]]).astype(np.uint8)
        seqs.append(tip)
    h = built(K, both(seqs))
    c = Case(h)
    L = g[:ps[0]]
    arm = lambda p: g[p - K + 1:p + K]; mid = lambda a, b: g[a + 1:b]
    want = [L, arm(ps[0]), mid(ps[0], ps[1]), arm(ps[1]), mid(ps[1], ps[2]), arm(ps[2]), mid(ps[2], ps[3]), arm(ps[3])]
    # the read: 200 bases from 90, so ext = 200 - (200 - 90) = 90 > 3 * 24 + ... the arms of the last bubble cover it: 20 + 4 + 20 + 4 + 20 + 4 + 20 = 92 K-mers
    c.read(g[90:290], 30, [edge_id(h, L)], 90, (90, [L] if extra_tip else want))
    c.counters = dict(n_ext_tried=1, n_ext_too_many=1 if extra_tip else 0, n_ext_extended=0 if extra_tip else 1)
    return c


def six_junctions(K=80, seed=7):
    """a vertex with 2 in-edges and 3 out-edges: six crossings (twelve with the other strand); edges of K, K + 1, K + 15, K + 32 and K + 70 bases"""
    rng = np.random.default_rng(seed)
    cc = R(rng, K - 1)
    i0 = np.concatenate([[0], cc]).astype(np.uint8); i1 = np.concatenate([[2, 1], cc]).astype(np.uint8)
    o0 = np.concatenate([cc, [0]]).astype(np.uint8); o1 = np.concatenate([cc, [1], R(rng, 15)]).astype(np.uint8); o2 = np.concatenate([cc, [2], R(rng, 70)]).astype(np.uint8)
    o3 = np.concatenate([o1[-(K - 1):], R(rng, 33)]).astype(np.uint8)         # behind o1, K + 32 bases ... which the builder merges with o1
    G = Gb(K, 7)
    a = G.add(i0, 0, 2); b = G.add(i1, 1, 2); G.add(o0, 2, 3); G.add(o1, 2, 4); G.add(o2, 2, 5); G.add(o3, 4, 6)
    c = Case(G.hbv())
    o13 = np.concatenate([o1, o3[K - 1:]])
    c.edges = both([i0, i1, o0, o13, o2])
    rd = np.concatenate([i1, o2[K - 1:K - 1 + 19]])                            # 100 bases: ext = 19; o0 has one K-mer and ends, o1+o3 and o2 cover
    c.read(rd, 30, [b], 0, (0, [i1, o2]))
    rd0 = np.concatenate([i0, o13[K - 1:K - 1 + 40]])
    c.read(rd0, 30, [a], 0, (0, [i0, o13]))
    c.counters = dict(n_junctions=2 * 6 + 2, n_ext_tried=2, n_ext_extended=2)
    return c


def short_patches(K=80, seed=8):
    """new_stuff entries of length 0, K - 1 and K beside a real one: the first two hold no K-mer, the third becomes an edge of its own"""
    rng = np.random.default_rng(seed + 100)
    c = gap_bridge(K, seed)
    lone = R(rng, K)
    c.new = [np.zeros(0, np.uint8), R(rng, K - 1)] + c.new + [lone]
    c.edges = c.edges + both([lone])
    c.counters = dict(n_all=8, n_junctions=0, n_unipaths=2, n_tr_first=3)
    return c


def palindrome(K=80, seed=9):
    """a palindromic K-mer P = x rc(x) in the genome.  P is its own reverse complement, so in the unipath graph it is an edge of one K-mer
    that is its own inverse: E1 and rc(E2) enter the vertex in front of it, E2 and rc(E1) leave the one behind it, and the four crossings
    (a P, rc(b) P, P b, P rc(a)) enter allx.  The old graph is the builder's own on the genome; a patch with a SNP behind P splits E2"""
    rng = np.random.default_rng(seed)
    x = R(rng, K // 2)
    g = np.concatenate([R(rng, 300), x, rc(x), R(rng, 300)]).astype(np.uint8)
    a, b = 300, 300 + K                                                # P = g[a:b]
    assert g[a - 1] != 3 - g[b]                                        # (else P would not branch)
    h = built(K, both([g]))
    E1, P, E2 = g[:b - 1], g[a:b], g[a + 1:]
    assert sorted(s.tobytes() for s in M.edge_seqs(h)) == sorted(s.tobytes() for s in both([E1, E2]) + [P])
    p = 450
    g2 = g.copy(); g2[p] = alt(g[p])
    c = Case(h, [g2[p - 100:p + 100]])
    E2a, A, A2, Rr = g[a + 1:p], g[p - K + 1:p + K], g2[p - K + 1:p + K], g[p + 1:]
    c.edges = both([E1, E2a, A, A2, Rr]) + [P]
    # over the palindrome: ext = 150 - (379 - 250) = 21; behind E1 comes P alone, behind P come E2a and rc(E1)
    c.read(g[250:400], 30, [edge_id(h, E1)], 250, (250, [E1, P, E2a]))
    # on the palindrome itself: ext = 70, exactly the K-mers of E2a
    c.read(g[a:a + 150], 30, [edge_id(h, P)], 0, (0, [P, E2a]))
    # the other strand: rc(E2) maps to [rc(R), rc(A), rc(E2a)]; start 250 walks onto rc(A) at 100; ext = 91 runs over rc(E2a) and P into rc(E1)
    c.read(rc(g)[250:400], 30, [edge_id(h, rc(E2))], 250, (250 - (len(Rr) - K + 1), [rc(A), rc(E2a), P, rc(E1)]))
    c.counters = dict(n_all=5 + 4 + 1, n_junctions=4, n_unipaths=6, n_tr_first=2, n_tr_walked=1, n_tr_cleared=0, n_tr_empty=0, n_ext_tried=3, n_ext_extended=3)
    return c


def empty_graph(K=80, patch=False, seed=10):
    """no edge object at all (allx is empty, or holds one patch alone); the reads have no path and keep none"""
    g = R(np.random.default_rng(seed), 300)
    c = Case(empty_hbv(K), [g] if patch else [])
    c.edges = both([g]) if patch else []
    c.read(g[:150], 30, [], 0, (0, []))
    c.read(g[100:250], 30, [], 3, (3, []))
    c.counters = dict(n_all=int(patch), n_junctions=0, n_all_bases=300 * int(patch), n_kmer_instances=(300 - K + 1) * int(patch), n_unipaths=int(patch),
                      n_tr_empty=2, n_tr_first=0, n_ext_tried=0)
    return c


def tandem(K=20, u=24, seed=13):
    """X U U U Y with a unit U of u >= K bases: the cycle of U's K-mers is entered from X and left to Y, so it is two edges, D (U itself,
    u - K + 1 K-mers) and C (the K - 1 K-mers that wrap), and the genome reads In D C D C D Out.  The old graph is two edges that meet
    inside the second D, so their maps hold the loop's edges more than once: [In D C D] and [D C D Out], which overlap by one entry and
    by three.  OverlapAppend takes the three (Vec.h:612, longest first) -- and so drops a turn of the loop; the reference does."""
    rng = np.random.default_rng(seed)
    X, U, Y = R(rng, 120), R(rng, u), R(rng, 150)
    g = np.concatenate([X, U, U, U, Y]).astype(np.uint8)
    p0 = len(X); a = u - K + 1
    assert X[-1] != U[-1] and Y[0] != U[0] and u >= K
    In, D, C, Out = g[:p0 + K - 1], g[p0:p0 + u], g[p0 + u - K + 1:p0 + u + K - 1], g[p0 + 3 * u - K + 1:]
    s = p0 + u + 2 + K                                                 # e0's last K-mer is D's third, e1's first D's fourth
    G = Gb(K, 3)
    e0 = G.add(g[:s], 0, 1); e1 = G.add(g[s - K + 1:], 1, 2)
    c = Case(G.hbv(), [g[p0 - 30:p0 + 3 * u + 30]])                    # the patch spans the array
    c.edges = both([In, D, C, Out])
    # walks, in the first map alone: 150 - 120 = 30 >= 24 -> 25 on C; then ext = 60 - 13 = 47 = 5 + 19 + 5 + 18 over D C D into Out
    c.read(g[150:210], 30, [e0, e1], 150, (25, [C, D, C, D, Out]))
    # an offset past the first edge's end walks through the appended list [In D C D Out]: 65 -> 60 -> 41 -> 36 on Out (a sink: not tried);
    # [In D C D C D Out], the shortest overlap, would stop on the second C
    c.read(g[185:245], 30, [e0, e1], 185, (36, [Out]))
    tile = lambda n: np.concatenate([g[100:p0 + u]] + [U] * (n // u + 1)).astype(np.uint8)[:n]
    # the list goes round the cycle: entry 0; turn t adds D (a + t u K-mers), C ((t + 1) u) and Out.  ext = 20: D is expanded, C and Out cover
    c.read(tile(39 + 20), 30, [e0], 100, (100, [In, D, C]))
    c.read(tile(39 + 20), [30] * 39 + [0] * 20, [e0], 100, (100, [In]))                 # the same at quality 0: a tie
    # 33 u < ext <= a + 33 u: the D of turn 33 is entry 100 and is not expanded: 101 entries, and only that D matches a read that goes on turning
    c.read(tile(39 + a + 33 * u), 30, [e0], 100, (100, [In] + [D, C] * 33 + [D]))
    # one base more: that D is expanded too, entries 101 and 102 exist, the reference gives up
    c.read(tile(39 + a + 33 * u + 1), 30, [e0], 100, (100, [In]))
    c.counters = dict(n_junctions=2, n_unipaths=4, n_tr_first=4, n_tr_walked=2, n_tr_cleared=0, n_ext_tried=5, n_ext_extended=3, n_ext_ambiguous=1, n_ext_too_many=1,
                      n_ext_no_cover=0)
    return c


def hairpin(K=20, seed=15):
    """inverted repeats.  A S rc(S) B: the middle is its own reverse complement and both strands run through it; the builder cuts it at
    the palindromic K-mer P, so the edge E = S + 9 bases is followed by P and P by rc(E).  And A S l rc(S) B with a loop l of 5 bases:
    the edge of S, a bubble of the loop and its reverse complement, the reverse complement of the edge of S.  One read through each"""
    rng = np.random.default_rng(seed)
    A, S, B = R(rng, 100), R(rng, 40), R(rng, 100)
    B[0] = 3 - alt(A[-1])                                              # (the two strands part where the repeat ends, not a base later)
    g = np.concatenate([A, S, rc(S), B]).astype(np.uint8)
    A2, S2, l2, B2 = R(rng, 100), R(rng, 40), R(rng, 5), R(rng, 100)
    B2[0] = 3 - alt(A2[-1])
    g2 = np.concatenate([A2, S2, l2, rc(S2), B2]).astype(np.uint8)
    assert l2.tobytes() != rc(l2).tobytes()
    h = built(K, both([g, g2]))
    c = Case(h)
    Ea, E, P, Eb = g[:100 + K - 1], g[100:140 + K // 2 - 1], g[140 - K // 2:140 + K // 2], g[180 - K + 1:]
    assert P.tobytes() == rc(P).tobytes()
    Ea2, Es, El, Eb2 = g2[:100 + K - 1], g2[100:140], g2[140 - K + 1:145 + K - 1], g2[185 - K + 1:]
    c.edges = both([Ea, E, Eb, Ea2, Es, El, Eb2]) + [P]
    # ext = 150 - 59 = 91: E (30 K-mers), P (1), rc(E) (30), then Eb against rc(Ea)
    c.read(g[60:210], 30, [edge_id(h, Ea)], 60, (60, [Ea, E, P, rc(E), Eb]))
    # ext = 155 - 59 = 96: Es (21), the loop against its reverse complement (24), rc(Es) (21), then Eb2 against rc(Ea2)
    c.read(g2[60:215], 30, [edge_id(h, Ea2)], 60, (60, [Ea2, Es, El, rc(Es), Eb2]))
    c.counters = dict(n_unipaths=8, n_tr_first=2, n_ext_tried=2, n_ext_extended=2)
    return c


STRIDE_M = (62, 63, 64, 65, 127, 128)


def stride(K=20, seed=14, min_gain=5):
    """One base decides, at extension base m = 62 ... 128, once as the read's last base (ext = m + 1) and once just past it (ext = m),
    at quality min_gain (extended) and min_gain - 1 (not), the extension starting at read base 0, 1, 2, 3 mod 4.
    Per m a contig with two SNP bubbles, the second SNP at base m: L -> a0 | a1 -> Mid -> b0 | b1 -> R; all four combinations cover,
    the first SNP costs 30, the second the deciding quality.  There the deciding base is always the first of its piece (the arm b);
    so per m also a fork W -> x0 | x1 of two unrelated arms of 140 bases, read at quality 0 but for base m, where the arms differ:
    the deciding base lies m bases inside one piece."""
    rng = np.random.default_rng(seed)
    seqs, bub, fork = [], [], []
    for m in STRIDE_M:
        g = R(rng, 100 + m + 60); p1, p2 = 100, 100 + m
        v1 = g[p1 - K:p1 + K + 1].copy(); v1[K] = alt(g[p1])
        v2 = g[p2 - K:p2 + K + 1].copy(); v2[K] = alt(g[p2])
        seqs += [g, v1, v2]; bub.append((m, g, p1, p2))
        W, x0, x1 = R(rng, 60), R(rng, 140), R(rng, 140)
        if x1[0] == x0[0]:
            x1[0] = alt(x0[0])
        if x1[m] == x0[m]:
            x1[m] = alt(x0[m])
        seqs += [np.concatenate([W, x0]), np.concatenate([W[-K:], x1])]; fork.append((m, W, x0, x1))
    h = built(K, both(seqs))
    c = Case(h, min_gain=min_gain)
    c.edges = []
    i = 0
    for m, g, p1, p2 in bub:
        L, a0, Mid, b0, Rr = g[:p1], g[p1 - K + 1:p1 + K], g[p1 + 1:p2], g[p2 - K + 1:p2 + K], g[p2 + 1:]
        a1 = a0.copy(); a1[K - 1] = alt(g[p1]); b1 = b0.copy(); b1[K - 1] = alt(g[p2])
        c.edges += both([L, a0, a1, Mid, b0, b1, Rr])
        for ext, q in ((m + 1, min_gain), (m + 1, min_gain - 1), (m, min_gain), (m, min_gain - 1)):
            rstop = 40 + i % 4; i += 1
            n = rstop + ext
            ql = np.full(n, 30, np.uint8)
            if ext > m:
                ql[rstop + m] = q
            want = [L, a0, Mid] if ext == m else [L, a0, Mid, b0] if q >= min_gain else [L]
            c.read(g[p1 - rstop:p1 - rstop + n], ql, [edge_id(h, L)], p1 - rstop, (p1 - rstop, want))
        if m == 64:                                                    # the read's base at the second SNP at quality 0: b1 costs nothing
            ql = np.full(40 + m + 1, 30, np.uint8); ql[40 + m] = 0
            c.read(g[p1 - 40:p1 + m + 1], ql, [edge_id(h, L)], p1 - 40, (p1 - 40, [L]))
    for m, W, x0, x1 in fork:
        e0, e1 = np.concatenate([W[-(K - 1):], x0]), np.concatenate([W[-(K - 1):], x1])
        c.edges += both([W, e0, e1])
        wx = np.concatenate([W, x0])
        for ext, q in ((m + 1, min_gain), (m + 1, min_gain - 1), (m, min_gain), (m, min_gain - 1)):
            rstop = 30 + i % 4; i += 1
            n = rstop + ext
            ql = np.concatenate([np.full(rstop, 30), np.zeros(ext)]).astype(np.uint8)
            if ext > m:
                ql[rstop + m] = q
            want = [W, e0] if ext > m and q >= min_gain else [W]       # ext = m: base m is not the read's, both arms cost 0
            c.read(wx[60 - rstop:60 - rstop + n], ql, [edge_id(h, W)], 60 - rstop, (60 - rstop, want))
    nm = len(STRIDE_M)
    c.counters = dict(n_tr_first=8 * nm + 1, n_ext_tried=8 * nm + 1, n_ext_extended=3 * nm + nm, n_ext_ambiguous=nm + 1 + 3 * nm, n_ext_too_many=0, n_ext_no_cover=0)
    return c


MIXED_LENS = (100, 149, 150, 151, 250, 251)
MIXED_COUNTS = (1, 63, 64, 65, 256, 257)


def mixed_lengths(n_reads, K=80, seed=4):
    """`extensions`' graph, n_reads reads of 100, 149, 150, 151, 250 and 251 bases in turn: every read's byte and quality offset depends on
    the lengths before it.  A read ends 1 ... 79 bases behind the SNP, carries either allele, the SNP at quality 30, min_gain,
    min_gain - 1 or 0; every seventh has no path, every eleventh a negative offset"""
    e = extensions(K, seed)
    hs = M.edge_seqs(e.h)
    p = 300
    sL, sa0, sa1, sR = hs[0], hs[2], hs[4], hs[6]                      # (Gb numbers the forward edges 0, 2, 4, ...)
    g = np.concatenate([sL, sa0[K - 1:K], sR]).astype(np.uint8)       # the genome: L, the SNP, R
    assert len(sL) == p and len(g) == 600
    g2 = g.copy(); g2[p] = sa1[K - 1]
    c = Case(e.h)
    c.edges = e.edges
    exts = (1, 2, 3, 4, 5, 63, 64, 65, 79)
    cnt = dict(n_tr_empty=0, n_tr_first=0, n_tr_walked=0, n_tr_cleared=0, n_ext_tried=0, n_ext_extended=0, n_ext_ambiguous=0, n_ext_no_cover=0, n_ext_too_many=0)
    for i in range(n_reads):
        n = MIXED_LENS[i % 6]; ext = exts[(i // 2) % len(exts)]; q = (30, 5, 4, 0)[(i // 3) % 4]; other = i % 2
        s = p + ext - n
        ql = np.full(n, 30, np.uint8); ql[p - s] = q
        b = (g2 if other else g)[s:s + n]
        if i % 7 == 3:
            c.read(b, ql, [], i, (i, [])); cnt["n_tr_empty"] += 1
        elif i % 11 == 5:
            c.read(b, ql, [0], -5, (-5, [sL])); cnt["n_tr_first"] += 1
        else:
            c.read(b, ql, [0], s, (s, [sL, sa1 if other else sa0] if q >= 5 else [sL]))
            cnt["n_tr_first"] += 1; cnt["n_ext_tried"] += 1; cnt["n_ext_extended" if q >= 5 else "n_ext_ambiguous"] += 1
    c.counters = cnt
    return c


def cases():
    d = {"chain3": chain3, "gap_bridge": gap_bridge, "branch_patch": branch_patch, "extensions": extensions, "k_edges": k_edges,
         "ladder_101": lambda: ladder(False), "ladder_102": lambda: ladder(True), "six_junctions": six_junctions, "short_patches": short_patches,
         "palindrome": palindrome, "chain3_K96": lambda: chain3(96, 11), "gap_bridge_K200": lambda: gap_bridge(200, 12),
         "empty_graph": empty_graph, "empty_graph_one_patch": lambda: empty_graph(patch=True),
         "tandem": tandem, "hairpin": hairpin, "stride": stride}
    for n in MIXED_COUNTS:
        d[f"mixed_lengths_{n}"] = lambda n=n: mixed_lengths(n)
    return d


# ---- seeded random cases ------------------------------------------------------------------------------------------------------------
SEEDS = (1, 2, 3)
RANDOM_K = 20       # with 150-base reads only a small K lets a list reach 102 entries (a SNP bubble's arm has K K-mers)


def random_case(seed):
    """a genome of about 3 kb: SNP bubbles, a dense ladder of them, contigs with gaps between them, patches cut from the genome across the
    gaps (some with a SNP of their own, one that joins nothing), 400 reads of 150 bases with errors and qualities, placed on the old graph"""
    K = RANDOM_K
    rng = np.random.default_rng(1000 + seed)
    g = R(rng, 3000)
    gaps = [(400, 470), (1000, 1040), (1600, 1700), (2100, 2150), (2700, 2760)]
    snps = sorted(int(x) for x in rng.choice(np.arange(100, 2000, 50), 12, replace=False) + rng.integers(0, 20, 12))
    snps = [p for p in snps if not any(a - 2 * K <= p <= b + 2 * K for a, b in gaps)] + [2650]       # (2650: a bubble whose arms end at the last gap)
    dense = [2300 + 23 * i for i in range(8)]
    variants = []
    for p in snps + dense:
        for k in range(1, 2 + (p in dense) * int(rng.integers(0, 3))):
            v = g[p - K:p + K + 1].copy(); v[K] = np.uint8((int(g[p]) + k) & 3); variants.append(v)
    pieces, at = [], 0
    for a, b in gaps:
        pieces.append(g[at:a]); at = b
    pieces.append(g[at:])
    h = built(K, both(pieces + variants))
    new = []
    for i, (a, b) in enumerate(gaps[:4]):
        s = g[a - K - 20:b + K + 20].copy()
        if i == 1:
            s[len(s) // 2] = alt(s[len(s) // 2])
        new.append(s if i != 2 else rc(s))
    new += [g[2500:2500 + 90].copy(), R(rng, 70), R(rng, K - 1), np.zeros(0, np.uint8)]
    new[4][45] = alt(new[4][45])                                       # a patch that opens a bubble inside an edge
    # the old graph's K-mers -> (edge, offset)
    where = {}
    for e, s in enumerate(M.edge_seqs(h)):
        for i in range(len(s) - K + 1):
            where[s[i:i + K].tobytes()] = (e, i)
    c = Case(h, new)
    for r in range(400):
        s = int(rng.integers(0, 3000 - 150))
        b = g[s:s + 150].copy()
        q = rng.integers(2, 41, 150).astype(np.uint8)
        for p in snps + dense:                                         # the read's own alleles
            if s <= p < s + 150 and rng.random() < 0.5:
                b[p - s] = np.uint8((int(g[p]) + 1) & 3)
        err = rng.random(150) < 0.01
        b[err] = (b[err] + 1) & 3; q[err] = rng.integers(0, 12, int(err.sum()))
        if rng.random() < 0.5:
            b = rc(b); q = q[::-1].copy()
        shift = int(rng.integers(0, 30)) if rng.random() < 0.3 else 0
        path, off = [], 0
        hit = where.get(b[shift:shift + K].tobytes())
        if hit is not None and rng.random() < 0.9:
            path, off = [hit[0]], hit[1] - shift
            if rng.random() < 0.4:                                     # follow the read over the next edges
                for i in range(shift + 1, 150 - K + 1):
                    nx = where.get(b[i:i + K].tobytes())
                    if nx is None:
                        break
                    if nx[1] == 0 and nx[0] != path[-1]:
                        path.append(nx[0])
            if rng.random() < 0.03:
                off += 400                                             # a wrong offset: past the end
        c.read(b, q, path, off)
    return c


def seed_conditions(m):
    """what a generated case must exercise, by the model's own count -> the list of what is missing"""
    return [k for k in M.COUNTERS if m.counters[k] < 1]


_CASES = {}


def get(name):
    """a hand-made case or random_<seed>, made once"""
    if name not in _CASES:
        _CASES[name] = random_case(int(name[len("random_"):])) if name.startswith("random_") else cases()[name]()
    return _CASES[name]


# ---- recorded runs of the reference's builder on allx ----------------------------------------------------------------------------------
# Recorded with `python tests/golden/make_golden.py refruns` (every record of the repository) or, these runs only,
# `... refruns tests/test_step5_add_model.py`.  Twelve hand-made cases are recorded this way; every case has a record of the
# whole call (reference_add below).
RECORDED = ("chain3", "gap_bridge", "branch_patch", "extensions", "k_edges", "six_junctions", "short_patches", "palindrome", "chain3_K96", "gap_bridge_K200",
            "ladder_101", "ladder_102")
# not recorded here: empty_graph* (the reference's Step 3 is not run on a graph without an edge object), random_* (hundreds of sequences each)
INPUTS = ["t.small_K.hbv", "t.small_K.paths"]
OUTPUTS = ["t.large_K.hbv", "t.large_K.paths"]


def reference_run(name, workdir):
    """stages the encoding of the case's allx in workdir as the reference's Step 3 reads it and puts the recorded t.large_K.hbv / .paths
    beside it (recording: oracle/_ref/ref_step3 at 1 thread and at 4, which must agree after hbvtool's canonicalisation; the 1-thread files
    are kept) -> (the new graph, the paths of the encoding's reads on it)"""
    from conftest import reference_outputs
    from w2rap_contigger_amd import hbvtool
    c = get(name)
    eh, ep, _ = M.encode(c.h, c.new)
    F.write_hbv(os.path.join(workdir, INPUTS[0]), eh)
    F.write_paths(os.path.join(workdir, INPUTS[1]), *ep)

    def run():
        from oracle import oracle3
        got = []
        for threads in (4, 1):
            oracle3.run_reference3(workdir, "t", c.h.K, threads)
            ch, cp, _ = hbvtool.canonicalise(F.read_hbv(os.path.join(workdir, OUTPUTS[0])), F.read_paths(os.path.join(workdir, OUTPUTS[1])))
            got.append(F.hbv_to_bytes(ch, zero_padding=True) + F.paths_to_bytes(*cp))
        assert got[0] == got[1], f"{name}: the reference's result at 4 threads is not its result at 1"
    reference_outputs(f"step5_add_{name}", workdir, INPUTS, OUTPUTS, run)
    return F.read_hbv(os.path.join(workdir, OUTPUTS[0])), F.read_paths(os.path.join(workdir, OUTPUTS[1]))


def involution(h):
    """the involution of a graph's edge objects, by content"""
    seqs = M.edge_seqs(h)
    by = {s.tobytes(): i for i, s in enumerate(seqs)}
    assert len(by) == len(seqs), "two edge objects of the graph have the same sequence"
    return np.array([by[rc(s).tobytes()] for s in seqs], np.int32)


# ---- recorded runs of the reference's AddNewStuff itself ------------------------------------------------------------------------------
# tests/golden/refruns/step5_addref_<case>/: oracle/_ref/ref_step5 in mode `add` (the whole call: BuildAll, the builder, TranslatePaths,
# Involution, ExtendPath) on the case as it stands -- new_stuff unencoded, repeats and entries below K kept, no reverse complements added.
ADD_INPUTS = ["t.hbv", "t.inv", "t.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp", "new_stuff.fastb"]
ADD_OUTPUTS = ["t.out.hbv", "t.out.paths", "t.out.inv"]
# AddNewStuff's own Validate aborts when two consecutive path edges share no vertex; branch_patch's read [e0, e1] is such a path.  Its
# second half alone (mode `tail`: TranslatePaths, resize(1), ExtendPath) runs on the recorded builder's graph and map of that case
TAIL_INPUTS = ["t.hbv", "t.map.txt", "t.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp"]
TAIL_OUTPUTS = ["t.out.paths"]
TAIL_ONLY = ("branch_patch",)
# the only cases without a record, and why: (name, reason)
NOT_ADD_RECORDED = ()


def add_recorded():
    """every case that has a step5_addref_ record (mode `add`, or `tail` for TAIL_ONLY)"""
    left_out = [n for n, _ in NOT_ADD_RECORDED]
    return [n for n in list(cases()) + [f"random_{s}" for s in SEEDS] if n not in left_out]


@dataclass
class AddRecord:
    hbv: F.HBV                    # the new graph as the reference numbered it (TAIL_ONLY: the step5_add_ record's)
    inv: np.ndarray
    path_offset: np.ndarray
    path_off: np.ndarray
    path_edges: np.ndarray
    rebuilt: object = None        # TAIL_ONLY: the Rebuilt the tail ran on (graph, to3, left3)


def _stage_reads(c, workdir):
    h, paths, reads, quals, new = c.inputs()
    F.write_paths(os.path.join(workdir, "t.paths"), *paths)
    F.write_fastb(os.path.join(workdir, "frag_reads_orig.fastb"), *reads)
    off = np.zeros(len(reads[2]) + 1, np.uint64); np.cumsum(reads[2], out=off[1:])
    F.write_qualp(os.path.join(workdir, "frag_reads_orig.qualp"), quals, off)


def reference_add(name, workdir):
    """stages the case's files in workdir as ref_step5 reads them and puts the recorded outputs beside them (recording: the binary at 4
    threads and at 1, which must agree on graph and paths after hbvtool's canonicalisation; the 1-thread files are kept) -> AddRecord"""
    from conftest import reference_outputs
    from w2rap_contigger_amd import hbvtool
    c = get(name)
    os.makedirs(workdir, exist_ok=True)
    _stage_reads(c, workdir)
    P = lambda f: os.path.join(workdir, f)
    if name in TAIL_ONLY:
        sub = os.path.join(workdir, "builder"); os.makedirs(sub, exist_ok=True)
        rec_env = os.environ.pop("W2RAP_RECORD_REFERENCE", None)       # the builder's record is replayed even while this one is made:
        try:                                                           # the tail's inputs are that record's numbering
            B, _ = recorded_rebuilt(name, sub)
        finally:
            if rec_env is not None:
                os.environ["W2RAP_RECORD_REFERENCE"] = rec_env
        F.write_hbv(P("t.hbv"), B.hbv)
        with open(P("t.map.txt"), "w") as fh:
            for l3, t3 in zip(B.left3, B.to3):
                fh.write(" ".join(str(x) for x in [l3] + t3) + "\n")
        mode, ins, outs = "tail", TAIL_INPUTS, TAIL_OUTPUTS
    else:
        F.write_hbv(P("t.hbv"), c.h)
        with open(P("t.inv"), "w") as fh:
            fh.write("".join(f"{int(x)}\n" for x in involution(c.h)))
        F.write_fastb(P("new_stuff.fastb"), *pack_seqs(c.new))
        mode, ins, outs = "add", ADD_INPUTS, ADD_OUTPUTS

    def run():
        from oracle import oracle5
        got = []
        for threads in (4, 1):
            out = oracle5.run_reference5(workdir, mode, threads, min_gain=c.min_gain)      # (raises when the binary exits non-zero)
            g = F.read_hbv(P("t.out.hbv")) if mode == "add" else B.hbv
            ch, cp, _ = hbvtool.canonicalise(g, F.read_paths(P("t.out.paths")))
            got.append(F.hbv_to_bytes(ch, zero_padding=True) + F.paths_to_bytes(*cp))
        assert got[0] == got[1], f"{name}: the reference's result at 4 threads is not its result at 1"
        return out.split("REF_STEP5")[-1].strip()
    reference_outputs(f"step5_addref_{name}", workdir, ins, outs, run)
    po, pf, pe = F.read_paths(P("t.out.paths"))
    if mode == "tail":
        return AddRecord(B.hbv, B.inv, po, pf, pe, B)
    inv = np.array(open(P("t.out.inv")).read().split(), np.int32)
    g = F.read_hbv(P("t.out.hbv"))
    if g.K != c.h.K:
        # When allx holds no K-mer at all the reference's builder only Clear()s hb3 (BigKPather.cc:475-478) and AddNewStuff assigns it: the
        # graph it writes has the K of a default HyperBasevector, 0.  The library keeps the call's K (its result stays a legal input of
        # PartnersToEnds); such a record is read with the case's K.  Nothing else may differ in K
        import dataclasses
        assert g.K == 0 and g.n_edges == 0 and g.n_vertices == 0 and not any(len(s) >= c.h.K for s in list(M.edge_seqs(c.h)) + c.new)
        g = dataclasses.replace(g, K=c.h.K)
    return AddRecord(g, inv, po, pf, pe)


def recorded_rebuilt(name, workdir):
    """-> (step5_add_model.Rebuilt from the record, the hint (codes, off) that replays its edge order)"""
    from oracle import oracle as O
    c = get(name)
    g, (po, pf, pe) = reference_run(name, workdir)
    # the involution of the recorded graph, by content
    seqs = M.edge_seqs(g)
    by = {s.tobytes(): i for i, s in enumerate(seqs)}
    inv = np.array([by[rc(s).tobytes()] for s in seqs], np.int32)
    n_uni = sum(1 for i in range(len(seqs)) if inv[i] >= i)
    return M.rebuilt_from(c.h, g, po, pf, pe, inv, n_uni), O.edge_hint_from_hbv(g)

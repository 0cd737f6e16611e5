"""Hand-made Step-3 inputs (small-K edge objects + read paths) for the corners the Step-2 fixtures do not reach:
a smooth circle in the large-K graph, a palindromic K2-mer, places that wrap a circular edge several times, long multi-edge
paths, a place of exactly K2 bases.  Shared by the CPU test (oracle against the reference binary) and the GPU test
(library against the oracle)."""
import numpy as np

from w2rap_contigger_amd import formats as F

K = 60


def rc(a):
    return (3 - np.asarray(a, np.uint8)[::-1]).astype(np.uint8)


def make_hbv(seqs):
    """an HBV holding the given edge objects, every object between two vertices of its own (Step 3 without extend_paths
    reads only the edge objects of the graph; the adjacency just has to load)"""
    n = len(seqs)
    codes = np.concatenate(seqs).astype(np.uint8)
    off = np.zeros(n + 1, np.uint64); np.cumsum([len(s) for s in seqs], out=off[1:])
    packed, boff, lens = F.pack_bases(codes, off)
    nv = 2 * n
    from_off = np.zeros(nv + 1, np.uint64); to_off = np.zeros(nv + 1, np.uint64)
    from_off[1:] = np.repeat(np.arange(1, n + 1), 2)[:nv] if n else 0          # vertex 2o has one out-edge, 2o+1 none
    for o in range(n):
        from_off[2 * o + 1] = o + 1; from_off[2 * o + 2] = o + 1
        to_off[2 * o + 1] = o; to_off[2 * o + 2] = o + 1
    from_v = np.array([2 * o + 1 for o in range(n)], np.int32)
    from_e = np.arange(n, dtype=np.int32); to_e = np.arange(n, dtype=np.int32)
    return F.HBV(K, from_off, from_v, from_e, to_off, to_e, packed, boff, lens)


def make_paths(plist, offsets=None):
    n = len(plist)
    off = np.zeros(n + 1, np.uint64); np.cumsum([len(p) for p in plist], out=off[1:])
    edges = np.array([e for p in plist for e in p], np.int32)
    po = np.zeros(n, np.int32) if offsets is None else np.asarray(offsets, np.int32)
    return po, off, edges


def case(name, seed=5):
    rng = np.random.default_rng(seed)
    R = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    if name == "circle":
        # a circular small-K edge (its first K-1 bases repeat at the end) read around the junction: the K2-mers close a smooth circle
        circ = R(1000)
        e = np.concatenate([circ, circ[:K - 1]])
        seqs = [e, rc(e)]
        paths = [[0], [0, 0], [1, 1], [0, 0, 0], [1], [], [0, 0], [1]]          # (reads come in pairs: FragDist takes 2i with 2i+1)
        return make_hbv(seqs), make_paths(paths, [3, 900, 950, 990, 7, 0, -20, 40])
    if name == "palindrome":
        x = R(100)
        pal = np.concatenate([x, rc(x)])                       # a 200-base palindrome: one palindromic K2-mer at K2 = 200
        e = np.concatenate([R(300), pal, R(300)])
        short = np.concatenate([R(100), pal[:150]])            # a second edge sharing 150 bases of it (K2-mers differ)
        seqs = [e, rc(e), short, rc(short), pal.copy()]        # the palindrome itself as an edge object: its own reverse complement
        paths = [[0], [1], [2], [3], [4], [4], [0], []]
        return make_hbv(seqs), make_paths(paths, [0, 5, 1, 2, 0, 3, 700, 0])
    if name == "chains":
        # a chain of short edges overlapping by K-1: long multi-edge paths, truncation at both ends, a place of exactly K2 bases
        g = R(4000)
        cuts = [0, 700, 761, 830, 1500, 1561, 1640, 2400, 2470, 3300, 4000 - (K - 1)]
        fw = [g[cuts[i]:cuts[i + 1] + K - 1] for i in range(len(cuts) - 1)]
        seqs = []
        for s in fw:
            seqs += [s, rc(s)]
        nE = len(fw)
        P = lambda *ix: [2 * i for i in ix]
        Pr = lambda *ix: [2 * i + 1 for i in reversed(ix)]
        exact = g[100:100 + 200]                                # an edge of exactly 200 bases
        seqs += [exact, rc(exact)]
        paths = [P(0, 1, 2, 3), Pr(0, 1, 2, 3), P(1, 2), P(2), P(3, 4, 5, 6, 7, 8, 9), Pr(5, 6, 7), P(4, 5), [2 * nE], [2 * nE + 1], P(1), P(0), Pr(9),
                 P(2, 3), [], P(6, 7, 8), Pr(0)]
        return make_hbv(seqs), make_paths(paths, list(range(-7, -7 + len(paths))))
    raise ValueError(name)


CASES = ["circle", "palindrome", "chains"]


# ---------------------------------------------------------------------------------------------------------------------------------
# Cases for Step 3's own edges (tests/test_step3_oracle.py pins the oracle on them to recorded reference runs, tests/test_gpu_step3_edges.py
# holds the library to the oracle).  Inputs only: nothing below is computed by the library or the oracle.

# the reference's -K list (w2rap-contigger.cc:60-62) within BigK's (LargeKDispatcher.h:22-27), above the small K of 60
REFERENCE_K2 = [72, 80, 84, 88, 96, 100, 108, 116, 128, 136, 144, 152, 160, 168, 172, 180, 188, 196, 200, 208, 216, 224, 232, 240, 260, 280, 300,
                320, 368, 400, 500, 544, 640]
# K2 = 2 mod 4: the library takes every even K2 in 62..640, BigK has multiples of 4 only.  (K2-1) mod 8 is 1 or 5 only here
ORACLE_ONLY_K2 = [62, 66, 94, 126, 130, 190, 254, 258, 638]
# and the word counts no K2 of the reference's list has (11, 14, 15, 18, 19 words of 32 bases), also 2 mod 4
ORACLE_ONLY_K2 += [350, 446, 478, 574, 606]


class _Graph:
    """edge objects with their inverses, and read paths over them"""
    def __init__(self):
        self.seqs, self.inv, self.paths = [], [], []

    def add(self, s):
        """-> the id of edge object s; its reverse complement becomes the next object unless s is its own"""
        s = np.asarray(s, np.uint8)
        e = len(self.seqs)
        self.seqs.append(s)
        if np.array_equal(s, rc(s)):
            self.inv.append(e)
        else:
            self.seqs.append(rc(s)); self.inv += [e + 1, e]
        return e

    def fw(self, *edges):
        self.paths.append(list(edges))

    def rv(self, *edges):
        self.paths.append([self.inv[e] for e in reversed(edges)])

    def done(self, rng, shuffle=True):
        paths = [self.paths[i] for i in rng.permutation(len(self.paths))] if shuffle else list(self.paths)
        if len(paths) % 2:
            paths.append([])                                    # (FragDist reads paths[id1 + 1] unchecked: an even number of reads)
        return make_hbv(self.seqs), make_paths(paths, rng.integers(-9, 51, len(paths)))


def chain_edges(g, lens):
    """g cut into edges of the given lengths, neighbours overlapping by K-1 bases"""
    out, a = [], 0
    for n in lens:
        out.append(g[a:a + n]); a += n - (K - 1)
    assert a + K - 1 == len(g)
    return out


def mix(K2):
    """one small-K graph per K2 with every shape that matters at large K, each between vertices of its own: a palindromic K2-mer inside an
    edge and as an edge that is its own inverse; a circle of 97 bases wrapped until the place reaches K2 bases; the homopolymer circle (a
    cycle of ONE K2-mer, paths of hundreds of edges); a chain whose end edges have K2-1, K2 and K2+1 bases (Repath.cc:113-122); a fork with
    four in- and four out-edges around one middle edge"""
    rng = np.random.default_rng(7000 + K2)
    R = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    G = _Graph()
    # palindrome of exactly K2 bases
    x = R(K2 // 2)
    pal = np.concatenate([x, rc(x)])
    a = G.add(np.concatenate([R(K2 + 37), pal, R(K2 + 5)]))
    p = G.add(pal)
    assert G.inv[p] == p
    G.fw(a); G.rv(a); G.fw(p); G.fw(p)
    # circle of circumference 97: n copies imply 97 n + 59 bases
    circ = R(97)
    c = G.add(np.concatenate([circ, circ[:K - 1]]))
    n = max(1, -(-(K2 - (K - 1)) // 97))
    assert 97 * n + K - 1 >= K2 and (n == 1 or 97 * (n - 1) + K - 1 < K2)
    G.fw(*[c] * n); G.rv(*[c] * (n + 1)); G.fw(*[c] * (n + 2)); G.fw(c); G.rv(c); G.rv(*[c] * n)
    # homopolymer circle: m copies imply m + 59 bases
    hp = G.add(np.zeros(K, np.uint8))
    G.fw(*[hp] * (K2 - 60)); G.fw(*[hp] * (K2 - 59)); G.rv(*[hp] * (K2 - 58)); G.fw(*[hp] * (K2 - 56)); G.rv(*[hp] * (K2 - 59))
    # chain of eight
    lens = [K2 - 1, K2, K2 + 1, 61, 75, K2 + 1, K2, K2 - 1]
    ch = [G.add(s) for s in chain_edges(R(sum(lens) - 7 * (K - 1)), lens)]
    G.fw(ch[0], ch[1]); G.fw(ch[1], ch[2]); G.fw(ch[2], ch[3]); G.fw(*ch); G.rv(*ch[5:]); G.rv(*ch[3:6])
    G.fw(ch[0]); G.fw(ch[1]); G.fw(ch[2]); G.rv(ch[2]); G.rv(ch[0], ch[1])
    # fork: the in-edges differ in the base before the shared (K-1)-mer, the out-edges in the base behind it
    mid = R(K2 + 20)
    m = G.add(mid)
    ins = [G.add(np.concatenate([R(K2 - 57 + b if b < 2 else 25 + b), [b], mid[:K - 1]])) for b in range(4)]       # two longer than K2, two shorter
    outs = [G.add(np.concatenate([mid[-(K - 1):], [b], R(K2 - 58 + b if b >= 2 else 30 + b)])) for b in range(4)]
    for b in range(4):
        G.fw(ins[b], m, outs[(b + 1) % 4]); G.rv(ins[b], m, outs[(b + 1) % 4])
    return G.done(rng)


# FragDist (GapToyTools3.cc:616-635): what the pairs of fragdist() must give, bin -> count; every other bin is 0
FRAGDIST_BINS = {0: 6, 1: 6, 30: 1, 50: 9, 98: 3, 99: 6}
FRAGDIST_D = [-1, 0, 9, 10, 11, 989, 990, 999, 1000, 500, 500, 500]


def fragdist(n_filler_pairs=0):
    """pairs ([e] at o1, [inv e] at len - d - o1) imply a fragment of d bases: on an edge of exactly 10000 bases and on its inverse object, on one
    of 10001 bases with a negative offset, and on one of 9999 bases, which is too short to count; then a mate on another edge's inverse, an
    empty first mate, an empty second mate, and a second mate of two edges that starts on the right edge.  n_filler_pairs pairs of reads
    without a path come first."""
    rng = np.random.default_rng(616)
    R = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    G = _Graph()
    e0, e1, e2 = G.add(R(10000)), G.add(R(9999)), G.add(R(10001))
    f = G.add(np.concatenate([G.seqs[G.inv[e0]][-(K - 1):], R(300)]))        # follows the inverse of e0
    paths, offs = [[]] * (2 * n_filler_pairs), [0] * (2 * n_filler_pairs)

    def pair(first, o1, d, second=None):
        L = len(G.seqs[first])
        paths.extend([[first], second or [G.inv[first]]]); offs.extend([o1, L - d - o1])
    for first, o1s in ((e0, rng.integers(0, 8000, 12)), (G.inv[e0], rng.integers(0, 8000, 12)), (e2, [-7] * 12), (e1, rng.integers(0, 8000, 12))):
        for d, o1 in zip(FRAGDIST_D, o1s):
            pair(first, int(o1), d)
    pair(e0, 100, 400, [G.inv[e2]])                                          # e1 != inv[e2]
    paths.extend([[], [G.inv[e0]]]); offs.extend([0, 9000])
    paths.extend([[e0], []]); offs.extend([20, 0])
    pair(e0, 50, 300, [G.inv[e0], f])                                        # only the first edge of the mate counts: bin 30
    assert len(paths) % 2 == 0
    return make_hbv(G.seqs), make_paths(paths, offs)


COUNTS = [(255, 1023, 100), (256, 1024, 100), (257, 1025, 100),          # k3_kmer_keys: 1024 occurrences a block; 256 places a block
          (1, 1025, 100), (3, 2048, 100), (5, 2049, 100),                # N = 2 D nodes: k3_head_cands' 4096-node block at 4096 and 4098 nodes
          (1024, 4096, 100), (1000, 4097, 100),                          # k3_dict_part: 4096 pairs a block
          (1, 1, 100), (1, 2, 100),
          (3, 2048, 640), (257, 1025, 640)]                              # 20-word places: a block's window passes KW_WORDS (StreamWin::at's global fallback)
COUNTS_RECORDED = [(1, 1025, 100), (3, 2048, 100), (5, 2049, 100)]


def counts(U, N2, K2):
    """U unrelated random edges with their inverses, each its own one-edge place; together N2 K2-mer occurrences, all distinct, in U unipaths;
    every second place is read through its reverse object"""
    rng = np.random.default_rng([U, N2, K2])
    G = _Graph()
    for i in range(U):
        e = G.add(rng.integers(0, 4, K2 + N2 // U + (i < N2 % U) - 1, dtype=np.uint8))
        G.fw(e) if i % 2 == 0 else G.rv(e)
    return G.done(rng, shuffle=False)


def make_hbv_joined(seqs):
    """an HBV with the adjacency the sequences imply: a vertex is a distinct (K-1)-mer at an edge's start or end; a vertex's out-edges ascend
    by target and its in-edges by source (--extend_paths walks the graph, Repath.cc:76-90)"""
    n = len(seqs)
    ids = {}
    vid = lambda s: ids.setdefault(np.asarray(s, np.uint8).tobytes(), len(ids))
    left, right = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for e, s in enumerate(seqs):
        left[e] = vid(s[:K - 1]); right[e] = vid(s[-(K - 1):])
    nv = len(ids)
    fr = sorted(range(n), key=lambda e: (left[e], right[e], e))
    to = sorted(range(n), key=lambda e: (right[e], left[e], e))
    from_off = np.zeros(nv + 1, np.uint64); np.cumsum(np.bincount(left, minlength=nv), out=from_off[1:])
    to_off = np.zeros(nv + 1, np.uint64); np.cumsum(np.bincount(right, minlength=nv), out=to_off[1:])
    off = np.zeros(n + 1, np.uint64); np.cumsum([len(s) for s in seqs], out=off[1:])
    packed, boff, lens = F.pack_bases(np.concatenate(seqs).astype(np.uint8), off)
    return F.HBV(K, from_off, right[fr].astype(np.int32), np.array(fr, np.int32), to_off, np.array(to, np.int32), packed, boff, lens)


JOINED_K2 = [100, 200, 260]


def joined(K2):
    """for --extend_paths: a chain of five unbranched edges, a fork of two out-edges behind it (which stops the extension), a one-edge circle
    (the Member(p, e) break, Repath.cc:84,88); places on inner chain edges, across the fork, on the circle once and twice, on both strands"""
    rng = np.random.default_rng(8000 + K2)
    R = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    G = _Graph()
    lens = [300, 280, 310, 270, 290]
    ch = [G.add(s) for s in chain_edges(R(sum(lens) - 4 * (K - 1)), lens)]
    tail = G.seqs[ch[4]][-(K - 1):]
    fk = [G.add(np.concatenate([tail, [b], R(250 + b)])) for b in (1, 2)]
    o = R(400)
    cir = G.add(np.concatenate([o, o[:K - 1]]))
    G.fw(ch[1]); G.fw(ch[2], ch[3]); G.rv(ch[2]); G.fw(ch[4], fk[0]); G.rv(ch[3], ch[4], fk[1]); G.fw(cir); G.fw(cir, cir); G.rv(cir); G.fw(fk[1])
    G.fw(); G.fw(ch[0]); G.rv(ch[0], ch[1]); G.rv(cir, cir, cir)
    paths = G.paths + ([[]] if len(G.paths) % 2 else [])
    return make_hbv_joined(G.seqs), make_paths(paths, rng.integers(-9, 51, len(paths)))


# ---- a plain-numpy statement of what Step 3 must give, for the K2 the reference cannot run (and on the library's own output)
def _place_seq(seqs, x, K2):
    """the bases a place implies (Repath.cc:109-122): the edges joined with K-1 overlaps; with several edges, the first and the last give at
    most K2 bases.  -> (bases, bases cut off on the left)"""
    b = seqs[x[0]]
    for e in x[1:]:
        b = np.concatenate([b[:len(b) - (K - 1)], seqs[e]])
    lt = 0
    if len(x) > 1:
        if len(seqs[x[-1]]) > K2:
            b = b[:len(b) - (len(seqs[x[-1]]) - K2)]
        if len(seqs[x[0]]) > K2:
            lt = len(seqs[x[0]]) - K2
            b = b[lt:]
    return b, lt


def _canon(k):
    a, b = k.tobytes(), rc(k).tobytes()
    return min(a, b)


def check_invariants(h, p, K2, obj_seqs, inv2, left, right, out_paths, n_distinct):
    """h, p: the input; obj_seqs / inv2 / left / right: the large-K edge objects, their inverses and vertices; out_paths = (offset, off, edges)
    of the translated reads.  Asserts what any correct Step 3 gives (the order of the edge objects is left open)."""
    codes, off = h.edge_codes(); off = off.astype(np.int64)
    seqs = [codes[off[e]:off[e + 1]] for e in range(h.n_edges)]
    po, pf, pe = p[0], p[1].astype(np.int64), p[2]
    reads = []                                                   # per read: (its place's bases as the read runs, bases cut on the left) or None
    place_kmers = set()
    for i in range(len(po)):
        x = list(pe[pf[i]:pf[i + 1]])
        if not x or sum(len(seqs[e]) - (K - 1) for e in x) + (K - 1) < K2:       # Repath.cc:56-59
            reads.append(None); continue
        b, lt = _place_seq(seqs, x, K2)
        reads.append((b, lt))
        place_kmers.update(_canon(b[t:t + K2]) for t in range(len(b) - K2 + 1))
    # the K2-mers of the edge objects are those of the places; each lies once on one object and once on that object's inverse
    where = {}
    for o, s in enumerate(obj_seqs):
        assert len(s) >= K2 and np.array_equal(obj_seqs[inv2[o]], rc(s)) and inv2[inv2[o]] == o
        for t in range(len(s) - K2 + 1):
            where.setdefault(_canon(s[t:t + K2]), []).append(o)
    assert set(where) == place_kmers and len(where) == n_distinct
    n_self = 0
    for c, objs in where.items():
        if c == rc(np.frombuffer(c, np.uint8)).tobytes():       # a palindromic K2-mer: an object of its own, which is its own inverse
            assert len(objs) == 1 and len(obj_seqs[objs[0]]) == K2 and inv2[objs[0]] == objs[0]
            n_self += 1
        else:
            assert len(objs) == 2 and inv2[objs[0]] == objs[1] and objs[0] != objs[1]
    assert n_self == sum(1 for o in range(len(obj_seqs)) if inv2[o] == o)
    # no edge can be extended
    nv = int(max(max(left, default=-1), max(right, default=-1))) + 1
    ins, outs = [[] for _ in range(nv)], [[] for _ in range(nv)]
    for o in range(len(obj_seqs)):
        outs[left[o]].append(o); ins[right[o]].append(o)
        assert np.array_equal(obj_seqs[o][:K2 - 1], obj_seqs[outs[left[o]][0]][:K2 - 1]) and np.array_equal(obj_seqs[o][-(K2 - 1):], obj_seqs[ins[right[o]][0]][-(K2 - 1):])
    for v in range(nv):
        if len(ins[v]) == 1 and len(outs[v]) == 1:
            a, b = ins[v][0], outs[v][0]
            assert a == b or inv2[a] == a or inv2[b] == b, (v, a, b)
    # every read path spells its place
    qo, qf, qe = out_paths[0], out_paths[1].astype(np.int64), out_paths[2]
    assert len(qo) == len(po)
    for i, rd in enumerate(reads):
        y = list(qe[qf[i]:qf[i + 1]])
        if rd is None:
            assert not y
            continue
        b, lt = rd
        assert y, i
        sp = obj_seqs[y[0]]
        for u, w in zip(y, y[1:]):
            assert right[u] == left[w] and np.array_equal(obj_seqs[u][-(K2 - 1):], obj_seqs[w][:K2 - 1])
            sp = np.concatenate([sp, obj_seqs[w][K2 - 1:]])
        start = int(qo[i]) - int(po[i]) + lt
        assert 0 <= start <= len(obj_seqs[y[0]]) - K2, i                                    # the first K2-mer lies on the first object
        assert np.array_equal(sp[start:start + len(b)], b), i
        assert len(sp) - len(obj_seqs[y[-1]]) <= start + len(b) - K2 <= len(sp) - K2, i      # and the last one on the last


def recorded_step3(case, h, p, d, K2, extend_paths=False):
    """the reference's Step 3 (1 thread) on (h, p), replayed from tests/golden/refruns/<case>/ (conftest.reference_outputs; recorded by
    `make_golden.py refruns tests/test_step3_oracle.py`) -> (its large-K graph, the bytes of its .large_K.paths, the text of its .first.frags.dist)"""
    import os
    from conftest import reference_outputs
    from oracle import oracle3 as O3
    d = str(d)
    F.write_hbv(os.path.join(d, "t.small_K.hbv"), h)
    F.write_paths(os.path.join(d, "t.small_K.paths"), *p)
    reference_outputs(case, d, ["t.small_K.hbv", "t.small_K.paths"], ["t.large_K.hbv", "t.large_K.paths", "t.first.frags.dist"],
                      lambda: O3.run_reference3(d, "t", K2, 1, extend_paths=extend_paths))
    return F.read_hbv(os.path.join(d, "t.large_K.hbv")), open(os.path.join(d, "t.large_K.paths"), "rb").read(), open(os.path.join(d, "t.first.frags.dist")).read()


def objects_of(obj_codes, obj_off):
    off = np.asarray(obj_off, np.int64)
    return [obj_codes[off[i]:off[i + 1]] for i in range(len(off) - 1)]

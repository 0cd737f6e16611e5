"""Hand-made inputs of the Step-5 tests (PartnersToEnds): a few edges, two to a few hundred reads cut from the edge sequences with
planted substitutions and chosen qualities.  Every case names the reads it is about and what must become of them, as literals.

    cases() -> {name: Case}; Case.inputs() -> (hbv, paths, (packed, byte_off, read_len), quals)
    Case.expect   {read id: ([edge ids], offset)}   the path and offset the read must have afterwards
    Case.counters {counter name: value}             counters worth pinning (any of step5.COUNTERS)

The usual scene: an edge M (300 bases, 101 K-mers) a -> b that the placed mates lie on, and a target edge T b -> c with c a sink, so
that D(b) = the K-mers of T.  An unplaced read is cut from T; its mate lies on M with path [M].  Graphs are built with the Builder of
step4_cases without mirror images (PartnersToEnds asks for no involution), random sequences, K = 200."""
import numpy as np

from step4_cases import Builder
from w2rap_contigger_amd import formats as F

K = 200


class Case:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b = Builder(K)
        self.codes, self.quals, self.paths, self.offs = [], [], [], []
        self.expect, self.counters = {}, {}

    def seq(self, n):
        return self.rng.integers(0, 4, n).astype(np.uint8)

    def vertex(self):
        return self.b.vertex()

    def edge(self, u, v, seq):
        """an edge u -> v, n random bases or the given sequence; -> its id"""
        s = self.seq(seq) if np.ndim(seq) == 0 else np.asarray(seq, np.uint8)
        return self.b.edge(u, v, s, mirror=False)

    def eseq(self, e):
        return self.b.edges[e][2]

    def scene(self, t_len=400, m_len=300):
        """a -> b (M) -> c (T); -> (M, T, b)"""
        a, b_, c = self.vertex(), self.vertex(), self.vertex()
        return self.edge(a, b_, m_len), self.edge(b_, c, t_len), b_

    def read(self, codes, qual=35, path=(), offset=0):
        codes = np.asarray(codes, np.uint8)
        q = np.full(len(codes), qual, np.uint8) if np.ndim(qual) == 0 else np.asarray(qual, np.uint8)
        assert len(q) == len(codes)
        self.codes.append(codes); self.quals.append(q); self.paths.append(list(path)); self.offs.append(offset)
        return len(self.codes) - 1

    def mate(self, M, start=10, length=100):
        """a placed read on M"""
        return self.read(self.eseq(M)[start:start + length], 35, [M], start)

    def pair(self, M, codes, qual=35, offset=0, first=False):
        """an unplaced read and its placed mate on M; first: the unplaced one gets the even id; -> the unplaced read's id"""
        if first:
            r = self.read(codes, qual, (), offset); self.mate(M)
        else:
            self.mate(M); r = self.read(codes, qual, (), offset)
        return r

    def mutated(self, codes, at, qual=35, low=10):
        """codes with substitutions at the positions `at`, and qualities `qual` but `low` at those positions"""
        c = np.array(codes, np.uint8); q = np.full(len(c), qual, np.uint8)
        for p in at:
            c[p] = (c[p] + 1) & 3; q[p] = low
        return c, q

    def inputs(self):
        h = self.b.hbv()
        n = len(self.codes)
        po = np.zeros(n + 1, np.uint64); ro = np.zeros(n + 1, np.uint64)
        np.cumsum([len(p) for p in self.paths], out=po[1:]); np.cumsum([len(c) for c in self.codes], out=ro[1:])
        paths = (np.array(self.offs, np.int32), po, np.array([e for p in self.paths for e in p], np.int32))
        return h, paths, F.pack_bases(np.concatenate(self.codes), ro), np.concatenate(self.quals)


def _control(c, seed_len=400):
    """a second scene with one read that is placed, so that a case about reads that are NOT selected still runs every phase;
    -> (read id, edge, offset)"""
    M, T, _ = c.scene(seed_len)
    r = c.pair(M, c.eseq(T)[50:200])
    c.expect[r] = ([T], 50)
    return r


def _embed(c, s, n=100, at=10):
    """n random bases holding the sequence s from position `at`"""
    x = c.seq(n); x[at:at + len(s)] = s
    return x


def cases():
    out = {}

    # ---- read selection and the near-an-end rule
    c = Case(1); M, T, _ = c.scene()
    r27 = c.pair(M, c.eseq(T)[100:127]); r28 = c.pair(M, c.eseq(T)[100:128])
    c.expect = {r27: ([], 0), r28: ([], 0)}                    # 28 bases are looked up (one 28-mer, one candidate) but never overlap by 60
    c.counters = dict(n_interesting=1, n_read_kmers=1, n_candidates=1, n_good=0, n_placed=0)
    out["length_27_is_not_interesting_28_is"] = c

    c = Case(2); M, T, _ = c.scene()
    r0 = c.read(c.eseq(T)[100:250]); r1 = c.read(c.eseq(T)[150:300])        # both of the pair unplaced
    c.expect = {r0: ([], 0), r1: ([], 0)}; _control(c)
    c.counters = dict(n_interesting=1, n_placed=1)
    out["mate_without_a_path"] = c

    c = Case(3); M, T, _ = c.scene()
    c.mate(M); r = c.read(c.eseq(T)[100:250], 35, [T], 5)                    # has a path already (a wrong offset stays wrong)
    c.expect = {r: ([T], 5)}; _control(c)
    c.counters = dict(n_interesting=1, n_placed=1)
    out["read_with_a_path_is_left_alone"] = c

    c = Case(4); M, T, _ = c.scene()
    ro = c.pair(M, c.eseq(T)[100:250]); re = c.pair(M, c.eseq(T)[30:180], first=True)
    assert ro % 2 == 1 and re % 2 == 0
    c.expect = {ro: ([T], 100), re: ([T], 30)}
    c.counters = dict(n_interesting=2, n_read_kmers=246, n_candidates=2, n_good=2, n_placed=2, n_ambiguous=0)
    out["odd_and_even_ids"] = c

    c = Case(5); M, T, _ = c.scene(t_len=699)                                # T has 500 K-mers: D(b) == 500
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([T], 100)}
    c.counters = dict(n_interesting=1, n_placed=1)
    out["distance_500_is_near"] = c

    c = Case(6); M, T, _ = c.scene(t_len=700)                                # 501 K-mers
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([], 0)}; _control(c)
    c.counters = dict(n_interesting=1, n_placed=1)
    out["distance_501_is_not"] = c

    c = Case(7); M, T, b = c.scene(t_len=499)                                # walks of 300 and 600 K-mers from b: the maximum counts
    T2 = c.edge(b, c.vertex(), 799)
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([], 0)}; _control(c)
    c.counters = dict(n_interesting=1, n_placed=1)
    out["two_walks_the_longer_counts"] = c

    c = Case(8); M, T, b = c.scene()                                         # a cycle b -> d -> b beside the exit T to a sink
    d = c.vertex(); c.edge(b, d, 210); c.edge(d, b, 220)
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([], 0)}; _control(c)
    c.counters = dict(n_interesting=1, n_placed=1)
    out["cycle_with_an_exit"] = c

    c = Case(9); a, b, d = c.vertex(), c.vertex(), c.vertex()                # a -> b, then only the circle b -> d -> b: no sink
    M = c.edge(a, b, 300); T = c.edge(b, d, 400); c.edge(d, b, 220)
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([], 0)}; _control(c)
    c.counters = dict(n_interesting=1, n_placed=1)
    out["pure_cycle"] = c

    # a chain of 620 edges of one K-mer each, v0 -> v1 -> ... -> v620 (the sink), edge ids ascending towards the sink: a relaxation that
    # walks the edges in id order moves a distance one edge per sweep, so v5 hears of the sink only after 615 sweeps.  v5 also has a
    # one-K-mer exit to a sink of its own: its first answer is 1, the right one (the maximum) is 615.  The mate on chain edge 4 ends at
    # v5: not near.  The mate on chain edge 219 ends at v220, 400 K-mers from the sink: near
    c = Case(22); vs = [c.vertex() for _ in range(621)]
    ch = [c.edge(vs[i], vs[i + 1], K) for i in range(620)]
    c.edge(vs[5], c.vertex(), K)
    rf = c.pair(ch[4], c.eseq(ch[300])[20:170])
    c.mate(ch[219], 10, 100); rn = c.read(c.eseq(ch[400])[30:180])
    c.expect = {rf: ([], 0), rn: ([ch[400]], 30)}
    c.counters = dict(n_interesting=1, n_read_kmers=123, n_candidates=1, n_good=1, n_placed=1, n_ambiguous=0)
    out["chain_of_620_edges_far_and_near"] = c

    # ---- dictionary multiplicity.  S is a 28-mer; a "filler" is a read of 28 bases, S itself: one 28-mer, never placed (under 60 bases)
    for n_fill, name in ((80, "kmer_in_80_reads_is_kept"), (81, "kmer_in_81_reads_is_dropped")):
        c = Case(10); M, T, _ = c.scene()
        S = c.seq(28)                                                        # in no edge
        for _ in range(n_fill):
            r = c.pair(M, S); c.expect[r] = ([], 0)
        c.counters = dict(n_interesting=n_fill, n_read_kmers=n_fill, n_dict_kmers=1 if n_fill <= 80 else 0, n_candidates=0)
        out[name] = c

    # X is T[64:164] with low-quality substitutions at 20, 35, 64, 80: every 28-mer of X but the one at 36 (S = T[100:128]) holds one,
    # so S is X's only link to T; four mismatches in any window pass.  S lies in 40 interesting reads (X and 39 fillers) and in n_e edges
    # (T and n_e - 1 random edges that hold a copy): 40 + 40 = 80 is kept and X is placed, 40 + 41 is dropped and X stays unplaced
    for n_e, name in ((40, "40_reads_plus_40_edges_is_kept"), (41, "40_reads_plus_41_edges_is_dropped")):
        c = Case(11); M, T, _ = c.scene()
        S = c.eseq(T)[100:128]
        for _ in range(n_e - 1):
            c.edge(c.vertex(), c.vertex(), _embed(c, c.eseq(T)[99:129], 230, 89))     # (with T's base on either side: X's substitutions there match no copy)
        x, q = c.mutated(c.eseq(T)[64:164], (20, 35, 64, 80))
        rx = c.pair(M, x, q)
        for _ in range(39):
            r = c.pair(M, S); c.expect[r] = ([], 0)
        c.expect[rx] = ([T], 64) if n_e == 40 else ([], 0)
        # distinct 28-mers of the reads: S and 72 more in X.  Kept: 40 reads x 40 edges candidates, one good
        c.counters = dict(n_interesting=40, n_read_kmers=73 + 39, n_dict_kmers=73 if n_e == 40 else 72,
                          n_candidates=1600 if n_e == 40 else 0, n_good=1 if n_e == 40 else 0, n_placed=1 if n_e == 40 else 0, n_ambiguous=0)
        out[name] = c

    # ---- candidate deduplication
    c = Case(12); M, T, _ = c.scene()
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([T], 100)}            # 123 shared 28-mers, one placement
    c.counters = dict(n_interesting=1, n_read_kmers=123, n_dict_kmers=123, n_candidates=1, n_good=1, n_placed=1, n_ambiguous=0)
    out["123_shared_kmers_are_one_candidate"] = c

    # a substitution in the middle splits the shared 28-mers into two runs on one diagonal: still one candidate
    c = Case(13); M, T, _ = c.scene()
    x, q = c.mutated(c.eseq(T)[100:250], (75,))
    r = c.pair(M, x, q); c.expect = {r: ([T], 100)}
    c.counters = dict(n_candidates=1, n_good=1, n_placed=1, n_ambiguous=0)
    out["two_runs_on_one_diagonal_are_one_candidate"] = c

    # ---- the window check
    for ov, name in ((59, "overhang_at_edge_start_59_rejected"), (60, "overhang_at_edge_start_60_accepted")):
        c = Case(14); M, T, _ = c.scene()
        r = c.pair(M, np.concatenate([c.seq(100 - ov), c.eseq(T)[:ov]]))     # the read hangs off the front: a negative start
        c.expect = {r: ([T], -(100 - ov)) if ov == 60 else ([], 0)}
        c.counters = dict(n_candidates=1, n_good=int(ov == 60))
        out[name] = c
    for ov, name in ((59, "overhang_at_edge_end_59_rejected"), (60, "overhang_at_edge_end_60_accepted")):
        c = Case(15); M, T, _ = c.scene()
        r = c.pair(M, np.concatenate([c.eseq(T)[400 - ov:], c.seq(100 - ov)]))
        c.expect = {r: ([T], 400 - ov) if ov == 60 else ([], 0)}
        c.counters = dict(n_candidates=1, n_good=int(ov == 60))
        out[name] = c
    for ql, name in ((30, "one_mismatch_at_quality_30_rejected"), (29, "one_mismatch_at_quality_29_accepted")):
        c = Case(16); M, T, _ = c.scene()
        x, q = c.mutated(c.eseq(T)[100:250], (75,), low=ql)
        r = c.pair(M, x, q, offset=7)                                        # (a rejected read keeps even an odd offset: nothing touches it)
        c.expect = {r: ([T], 100) if ql == 29 else ([], 7)}
        c.counters = dict(n_candidates=1, n_good=int(ql == 29))
        out[name] = c
    # reads of 60 bases have one window; of 61, two
    for ln, at, good, name in ((60, (0, 1, 2, 3), True, "4_mismatches_in_the_only_window_good"), (60, (0, 1, 2, 3, 4), False, "5_mismatches_in_the_only_window_rejected"),
                               (61, (0, 1, 2, 3, 4), True, "5_in_the_first_window_4_in_the_next_good")):
        c = Case(17); M, T, _ = c.scene()
        x, q = c.mutated(c.eseq(T)[100:100 + ln], at)
        r = c.pair(M, x, q); c.expect = {r: ([T], 100) if good else ([], 0)}
        c.counters = dict(n_candidates=1, n_good=int(good))
        out[name] = c

    # ---- the decision
    c = Case(18); M, T, _ = c.scene()
    T2 = c.edge(c.vertex(), c.vertex(), _embed(c, c.eseq(T)[100:250], 380, 33))   # a second edge holds the same 150 bases
    r = c.pair(M, c.eseq(T)[100:250], offset=7); c.expect = {r: ([], 0)}           # ambiguous: emptied, offset reset to 0
    c.counters = dict(n_candidates=2, n_good=2, n_placed=0, n_ambiguous=1)
    out["two_edges_ambiguous"] = c

    c = Case(19); a, b, d = c.vertex(), c.vertex(), c.vertex()
    X = c.seq(100)
    M = c.edge(a, b, 300); T = c.edge(b, d, np.concatenate([c.seq(120), X, X, c.seq(130)]))     # a tandem repeat inside one edge
    r = c.pair(M, X); c.expect = {r: ([], 0)}
    c.counters = dict(n_candidates=2, n_good=2, n_placed=0, n_ambiguous=1)
    out["one_edge_two_offsets_ambiguous"] = c

    c = Case(20); M, T, _ = c.scene()
    other = np.array(c.eseq(T)[100:250]); other[75] = (other[75] + 1) & 3          # the copy differs where the read is sure of itself
    c.edge(c.vertex(), c.vertex(), _embed(c, other, 380, 33))
    r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([T], 100)}
    c.counters = dict(n_candidates=2, n_good=1, n_placed=1, n_ambiguous=0)
    out["one_good_one_bad_is_placed"] = c

    # ---- boundaries: a wavefront of interesting reads, and (four candidates to a block of the verify kernel) 63, 64 and 65 candidates
    for n_r in (63, 64, 65):
        c = Case(21); M, T, _ = c.scene()
        for i in range(n_r):
            r = c.pair(M, c.eseq(T)[3 * i:3 * i + 100], first=bool(i & 1)); c.expect[r] = ([T], 3 * i)
        c.counters = dict(n_interesting=n_r, n_read_kmers=73 * n_r, n_candidates=n_r, n_good=n_r, n_placed=n_r, n_ambiguous=0)
        out[f"{n_r}_interesting_reads"] = c
    return out

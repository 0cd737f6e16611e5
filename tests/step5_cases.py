"""Hand-made inputs of the Step-5 tests (PartnersToEnds): a few edges, two to a few hundred reads cut from the edge sequences with
planted substitutions and chosen qualities.  Every case names the reads it is about and what must become of them, as literals.

    cases() -> {name: Case}; Case.inputs() -> (hbv, paths, (packed, byte_off, read_len), quals)
    Case.expect   {read id: ([edge ids], offset)}   the path and offset the read must have afterwards
    Case.counters {counter name: value}             counters worth pinning (any of step5.COUNTERS)

The usual scene: an edge M (300 bases, 101 K-mers) a -> b that the placed mates lie on, and a target edge T b -> c with c a sink, so
that D(b) = the K-mers of T.  An unplaced read is cut from T; its mate lies on M with path [M].  Graphs are built with the Builder of
step4_cases without mirror images (PartnersToEnds asks for no involution), random sequences, K = 200 unless a case says otherwise.

    random_case(seed) -> the same inputs, generated: a graph of 40-100 edges at K = 60 and 400-1000 reads (SEEDS, seed_conditions)
    recorded() -> the names of the cases whose run of the reference's own PartnersToEnds lies under tests/golden/refruns/step5_tail_<name>/
    reference_run(name, workdir) -> the reference's paths for that case, (offset, path_off, edges)"""
import os

import numpy as np

from conftest import reference_outputs
from step4_cases import Builder
from w2rap_contigger_amd import formats as F

K = 200


class Case:
    def __init__(self, seed, K=K):
        self.rng = np.random.default_rng(seed)
        self.K = K
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


def one_window_mismatches(L, w):
    """positions of substitutions in a read of L bases that leave exactly one window of 60 with at most 4 of them, the one that starts at
    w: four inside it (at w + 1, w + 2, w + 57, w + 58: 54 clean bases between them, so the read shares 28-mers with its edge), the three
    positions on either side of it, and every 12th position further out (5 to a window); w + 3 is free for the twin's fifth"""
    inside = [w + 1, w + 2, w + 57, w + 58]
    beside = [p for p in (w - 3, w - 2, w - 1, w + 60, w + 61, w + 62) if 0 <= p < L]
    further = [p for p in range(0, L, 12) if not w - 3 <= p < w + 63]
    return sorted(inside + beside + further)


def good_window_starts(L, at):
    """the window starts s (s + 60 <= L) with at most 4 of the positions `at` inside [s, s + 60), by counting"""
    return [s for s in range(L - 59) if sum(1 for p in at if s <= p < s + 60) <= 4]


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

    # ---- the verify kernel's 64-position chunks.  Reads that lie inside T overlap it by their own length L; one low-quality substitution
    # at the last position of each (of the 250-base read: at 192, lane 0 of its fourth chunk)
    c = Case(23); M, T, _ = c.scene()
    for i, L in enumerate((64, 65, 127, 128, 129, 250)):
        x, q = c.mutated(c.eseq(T)[7 * i + 5:7 * i + 5 + L], (192 if L == 250 else L - 1,))
        r = c.pair(M, x, q, first=bool(i & 1)); c.expect[r] = ([T], 7 * i + 5)
    c.counters = dict(n_interesting=6, n_candidates=6, n_good=6, n_placed=6, n_ambiguous=0)
    out["overlap_lengths_on_the_chunk_edges"] = c

    # exactly one window start w has at most 4 mismatches (one_window_mismatches; asserted here by counting, not by model or kernel);
    # the twin holds one more inside that window and has none
    for L in (150, 250):
        c = Case(24); M, T, _ = c.scene()
        for i, w in enumerate((0, 4, 5, 63, 64, 65, L - 60)):
            at = one_window_mismatches(L, w)
            assert good_window_starts(L, at) == [w] and good_window_starts(L, at + [w + 3]) == []
            s = 20 + 3 * i
            x, q = c.mutated(c.eseq(T)[s:s + L], at)
            r = c.pair(M, x, q, first=bool(i & 1)); c.expect[r] = ([T], s)
            x, q = c.mutated(c.eseq(T)[s:s + L], at + [w + 3])
            r = c.pair(M, x, q, first=bool(i & 1)); c.expect[r] = ([], 0)
        c.counters = dict(n_interesting=14, n_candidates=14, n_good=7, n_placed=7, n_ambiguous=0)
        out[f"one_good_window_in_{L}_bases"] = c

    # a trusted mismatch at the last position of an overlap of 129 (chunk 2, lane 0) is fatal; one position behind the overlap (the read
    # hangs off the edge end, every base of the overhang at quality 35) or in the overhang off the edge start it is not looked at
    c = Case(25); M, T, _ = c.scene(); t = c.eseq(T)
    x, q = c.mutated(t[100:229], (128,), low=30)
    ra = c.pair(M, x, q)
    rb = c.pair(M, np.concatenate([t[271:400], (t[:10] + 1) & 3]))
    rc = c.pair(M, np.concatenate([(t[390:400] + 2) & 3, t[:140]]))
    c.expect = {ra: ([], 0), rb: ([T], 271), rc: ([T], -10)}
    c.counters = dict(n_interesting=3, n_candidates=3, n_good=2, n_placed=2, n_ambiguous=0)
    out["trusted_mismatch_at_and_behind_the_overlap_end"] = c

    # the first compared base at 1, 2, 3 bases into the read's packed bytes (the read hangs off the edge start) and into the edge's
    c = Case(26); M, T, _ = c.scene(); t = c.eseq(T)
    for h in (1, 2, 3):
        x, q = c.mutated(np.concatenate([c.seq(h), t[:100 - h]]), (50,))
        r = c.pair(M, x, q); c.expect[r] = ([T], -h)
    for o in (1, 2, 3):
        x, q = c.mutated(t[o:o + 100], (50,))
        r = c.pair(M, x, q, first=True); c.expect[r] = ([T], o)
    c.counters = dict(n_interesting=6, n_candidates=6, n_good=6, n_placed=6, n_ambiguous=0)
    out["read_and_edge_starts_inside_a_byte"] = c

    # multiplicity counts locations, not reads: T[100:200] and then a run of one base (not T[199]) at quality 10.  A run of 107 holds its
    # 28-mer at 80 locations of this one read: kept; of 108, at 81: dropped.  Distinct 28-mers: 73 inside T[100:200], 27 across the joint,
    # the run's one.  The read is placed through the first 73 either way (its first window is clean)
    for run, name in ((107, "one_read_holds_a_kmer_80_times_kept"), (108, "one_read_holds_a_kmer_81_times_dropped")):
        c = Case(27); M, T, _ = c.scene(); t = c.eseq(T)
        x = np.concatenate([t[100:200], np.full(run, (int(t[199]) + 1) & 3, np.uint8)])
        r = c.pair(M, x, np.concatenate([np.full(100, 35, np.uint8), np.full(run, 10, np.uint8)])); c.expect[r] = ([T], 100)
        c.counters = dict(n_interesting=1, n_read_kmers=73 + run, n_dict_kmers=101 if run == 107 else 100, n_candidates=1, n_good=1, n_placed=1, n_ambiguous=0)
        out[name] = c

    # S at 10 and 60 of a read and at 50 and 120 of an edge: four diagonals (-40, -110, 10, -60), four candidates, none good; and the control's
    c = Case(28); M, T, _ = c.scene()
    S = c.seq(28)
    x = c.seq(300); x[50:78] = S; x[120:148] = S
    c.edge(c.vertex(), c.vertex(), x)
    x = c.seq(100); x[10:38] = S; x[60:88] = S
    r = c.pair(M, x); c.expect = {r: ([], 0)}; _control(c)
    c.counters = dict(n_interesting=2, n_read_kmers=73 + 123, n_candidates=5, n_good=1, n_placed=1, n_ambiguous=0)
    out["kmer_twice_in_a_read_and_twice_in_an_edge"] = c

    # ---- the mate's LAST edge decides.  x -P-> a -M-> b -T-> s (a sink), b -Q-> d, d -> d (no sink behind d): D(b) = 201, D(a) = 400 + 201,
    # D(d) = none.  M and T are near an end, P and Q are not
    c = Case(29); vx, va, vb, vs, vd = (c.vertex() for _ in range(5))
    P = c.edge(vx, va, 300); M = c.edge(va, vb, 599); T = c.edge(vb, vs, 400); Q = c.edge(vb, vd, 300); c.edge(vd, vd, 250)
    t = c.eseq(T)
    c.read(np.concatenate([c.eseq(P)[250:], c.eseq(M)[199:249]]), 35, [P, M], 250); r1 = c.read(t[100:250])
    r2 = c.read(t[120:270]); c.read(np.concatenate([c.eseq(M)[520:], c.eseq(Q)[199:220]]), 35, [M, Q], 520)
    c.read(t[10:110], 35, [T], 10); r3 = c.read(t[150:300])                  # the placed mate lies on T itself
    c.expect = {r1: ([T], 100), r2: ([], 0), r3: ([T], 150)}
    c.counters = dict(n_interesting=2, n_read_kmers=246, n_candidates=2, n_good=2, n_placed=2, n_ambiguous=0)
    out["the_mates_last_edge_decides"] = c

    # ---- reads of 28, 60, 150, 251 and 600 bases in one call, and a read of 650 that has a path: the diagonals are numbered by the longest
    # read of the call, looked up or not.  T has 451 K-mers
    c = Case(30); M, T, _ = c.scene(t_len=650); t = c.eseq(T)
    r28 = c.pair(M, t[100:128]); r60 = c.pair(M, t[200:260], first=True); r150 = c.pair(M, t[300:450])
    r251 = c.pair(M, t[330:581], first=True); r600 = c.pair(M, t[20:620])
    c.read(t, 35, [T], 0); c.mate(M)
    c.expect = {r28: ([], 0), r60: ([T], 200), r150: ([T], 300), r251: ([T], 330), r600: ([T], 20)}
    c.counters = dict(n_interesting=5, n_read_kmers=1 + 33 + 123 + 224 + 573, n_candidates=5, n_good=4, n_placed=4, n_ambiguous=0)
    out["read_lengths_28_to_600_in_one_call"] = c

    # ---- other K: the distance pair and the two id parities at K = 60 and K = 260 (an edge of n K-mers has n + K - 1 bases)
    for k in (60, 260):
        c = Case(4, k); M, T, _ = c.scene()
        ro = c.pair(M, c.eseq(T)[100:250]); re = c.pair(M, c.eseq(T)[30:180], first=True)
        c.expect = {ro: ([T], 100), re: ([T], 30)}
        c.counters = dict(n_interesting=2, n_read_kmers=246, n_candidates=2, n_good=2, n_placed=2, n_ambiguous=0)
        out[f"odd_and_even_ids_K{k}"] = c

        c = Case(5, k); M, T, _ = c.scene(t_len=499 + k)
        r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([T], 100)}
        c.counters = dict(n_interesting=1, n_placed=1)
        out[f"distance_500_is_near_K{k}"] = c

        c = Case(6, k); M, T, _ = c.scene(t_len=500 + k)
        r = c.pair(M, c.eseq(T)[100:250]); c.expect = {r: ([], 0)}; _control(c)
        c.counters = dict(n_interesting=1, n_placed=1)
        out[f"distance_501_is_not_K{k}"] = c
    return out


# ---- generated cases ---------------------------------------------------------------------------------------------------------------
SEEDS = (1, 2, 3)              # chosen on the CPU: at each the model alone meets every condition of seed_conditions
KR = 60                        # the K of the generated graphs


def random_case(seed):
    """-> (hbv, paths, (packed, byte_off, read_len), quals): a graph at K = 60 of 40-100 edges of 60-700 bases without mirror images
    (chains that end in sinks, branches to sinks of their own -- two of them exactly 500 and 501 K-mers long, others within 5 of 500 --,
    edges from one chain over to a later one, a cycle beside a way on to a sink, a cycle behind which there is no sink, three stretches
    of 100-200 bases copied from one edge into another and a tandem repeat of 2 x 120) and 400-1000 reads of 28-300 bases cut from the
    edges, one in four hanging off an edge end, with substitutions at qualities 2 .. 40.  About a third of the reads have no path; a
    placed read lies on a walk of one to three edges at an offset >= 0.  85 unplaced reads whose mates end on an edge into a sink hold a
    28-mer that is in no edge, 80 others hold one that is in one edge and in no other read; six are cut from inside the repeats, four hang
    off an edge start with 60 bases or more on the edge, and one pair has no path at all.  Pure Python, the same on every machine"""
    import random
    rng = random.Random(seed)
    c = Case(0, KR)
    out_edges, in_edges = {}, {}

    def rseq(n):
        return np.array([rng.randrange(4) for _ in range(n)], np.uint8)

    def edge(u, v, n):
        e = c.edge(u, v, rseq(n))
        out_edges.setdefault(u, []).append(e); in_edges.setdefault(v, []).append(e)
        return e

    chains, sink_edges = [], []
    for _ in range(rng.randint(6, 8)):
        n = rng.randint(4, 7)
        vs = [c.vertex() for _ in range(n + 1)]
        chains.append((vs, [edge(vs[i], vs[i + 1], rng.randint(60, 700)) for i in range(n)]))
        sink_edges.append(chains[-1][1][-1])
    for kmers in [500, 501] + [rng.choice((rng.randint(495, 505), rng.randint(1, 300))) for _ in range(rng.randint(3, 6))]:
        sink_edges.append(edge(rng.choice(rng.choice(chains)[0][:-1]), c.vertex(), kmers + KR - 1))
    for _ in range(rng.randint(3, 6)):                                       # from a chain over to a later one: no cycle comes of these
        i, j = sorted(rng.sample(range(len(chains)), 2))
        edge(rng.choice(chains[i][0][:-1]), rng.choice(chains[j][0][1:]), rng.randint(60, 400))
    u, w = chains[0][0][1], c.vertex()                                       # u -> w -> u beside u's way on along its chain
    edge(u, w, rng.randint(150, 300)); edge(w, u, rng.randint(150, 300))
    p, q = c.vertex(), c.vertex()                                            # into p -> q -> p, from where nothing leads out
    edge(chains[1][0][1], p, rng.randint(60, 300)); edge(p, q, rng.randint(60, 300)); edge(q, p, rng.randint(60, 300))
    read_edges = list(range(len(c.b.edges)))
    repeats = []
    for _ in range(3):
        n = rng.randint(100, 200)
        src, dst = rng.sample([e for e in read_edges if len(c.eseq(e)) >= n + 20], 2)
        a, b = rng.randrange(len(c.eseq(src)) - n + 1), rng.randrange(len(c.eseq(dst)) - n + 1)
        c.eseq(dst)[b:b + n] = c.eseq(src)[a:a + n]; repeats.append((src, a, n))
    e = rng.choice([e for e in read_edges if len(c.eseq(e)) >= 320])
    a = rng.randrange(len(c.eseq(e)) - 240 + 1)
    c.eseq(e)[a:a + 120] = rseq(120); c.eseq(e)[a + 120:a + 240] = c.eseq(e)[a:a + 120]; repeats.append((e, a, 120))
    Z = edge(c.vertex(), c.vertex(), 200)                                    # no read is cut from Z
    S1, S2 = rseq(28), c.eseq(Z)[50:78].copy()

    def cut(e, length, start):
        """`length` bases from `start` of edge e; random where that is off the edge"""
        s = c.eseq(e); x = rseq(length)
        lo, hi = max(0, start), min(len(s), start + length)
        x[lo - start:hi - start] = s[lo:hi]
        return x

    def walk(first, n):
        path = [first]
        while len(path) < n and out_edges.get(c.b.edges[path[-1]][1]):
            path.append(rng.choice(out_edges[c.b.edges[path[-1]][1]]))
        return path

    def placed(path):
        e = path[0]
        start = rng.randrange(len(c.eseq(e)))
        return (cut(e, rng.randint(28, 300), start), 35, path, start)

    def placed_anywhere():
        return placed(walk(rng.choice(read_edges), rng.randint(1, 3)))

    def placed_near_an_end():
        path = [rng.choice(sink_edges)]
        while len(path) < rng.randint(1, 3) and in_edges.get(c.b.edges[path[0]][0]):
            path.insert(0, rng.choice(in_edges[c.b.edges[path[0]][0]]))
        return placed(path)

    def unplaced(min_len=28):
        e = rng.choice(read_edges)
        n = min(rng.randint(min_len, 300), len(c.eseq(e)))
        start = rng.randrange(len(c.eseq(e)) - n + 1)
        if rng.random() < 0.25:
            start = rng.choice((-rng.randint(1, 40), len(c.eseq(e)) - n + rng.randint(1, 40)))
        x = cut(e, n, start); ql = np.full(n, 35, np.uint8)
        for _ in range(rng.choice((0, 0, 0, 1, 1, 2, 3, 6))):
            at = rng.randrange(n)
            x[at] = (x[at] + rng.randint(1, 3)) & 3; ql[at] = rng.randint(2, 40)
        return (x, ql, (), 0)

    def planted(S):
        x, ql, _, _ = unplaced(60)
        at = rng.randrange(len(x) - 27)
        x[at:at + 28] = S; ql[at:at + 28] = rng.randint(2, 10)
        return (x, ql, (), 0)

    def pair(a, b):
        for r in ((a, b) if rng.random() < 0.5 else (b, a)):
            c.read(*r)

    for _ in range(85):
        pair(planted(S1), placed_near_an_end())
    for _ in range(80):
        pair(planted(S2), placed_near_an_end())
    for _ in range(6):
        e, a, n = rng.choice(repeats)
        ln = rng.randint(60, min(n, 150))
        pair((cut(e, ln, a + rng.randrange(n - ln + 1)), 35, (), 0), placed_near_an_end())
    for _ in range(4):
        e = rng.choice([e for e in read_edges if len(c.eseq(e)) >= 150])
        pair((cut(e, rng.randint(90, 150), -rng.randint(1, 30)), 35, (), 0), placed_near_an_end())
    pair(unplaced(), unplaced())
    for _ in range(rng.randint(90, 300)):
        how = rng.random()
        if how < 0.35:
            pair(unplaced(), placed_anywhere())
        elif how < 0.38:
            pair(unplaced(), unplaced())
        else:
            pair(placed_anywhere(), placed_anywhere())
    assert 40 <= len(c.b.edges) <= 100 and 400 <= len(c.codes) <= 1000
    return c.inputs()


def seed_conditions(m):
    """what a generated case must exercise, judged on the model's result alone -> the list of what is missing.  (The generator places
    no read at a negative offset, so a path at one is a read this call placed.)"""
    missing = [k for k, v in m.counters.items() if v < 1]
    missing += [k for k in ("n_rejected", "n_dropped_by_reads", "n_dropped_by_total") if m.extra[k] < 1]
    plen = np.diff(m.path_off.astype(np.int64))
    if not np.any((m.path_offset < 0) & (plen > 0)):
        missing.append("a read placed at a negative offset")
    return missing


# ---- recorded runs of the reference's PartnersToEnds --------------------------------------------------------------------------------
INPUTS = ["t.hbv", "t.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp"]
OUTPUTS = ["t.out.paths"]
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
    """stages the case's inputs in workdir as the reference's main reads them, puts the recorded t.out.paths beside them (recording:
    runs oracle/_ref/ref_step5 at 1 thread and at 4, which must agree) -> (offset, path_off, edges)"""
    h, paths, reads, quals = inputs_of(name)
    F.write_hbv(os.path.join(workdir, "t.hbv"), h)
    F.write_paths(os.path.join(workdir, "t.paths"), *paths)
    F.write_fastb(os.path.join(workdir, "frag_reads_orig.fastb"), *reads)
    off = np.zeros(len(reads[2]) + 1, np.uint64); np.cumsum(reads[2], out=off[1:])
    F.write_qualp(os.path.join(workdir, "frag_reads_orig.qualp"), quals, off)

    def run():
        from oracle import oracle5
        got = []
        for threads in (1, 4):
            oracle5.run_reference5(workdir, "partners", threads)
            got.append(open(os.path.join(workdir, OUTPUTS[0]), "rb").read())
        assert got[0] == got[1], f"{name}: the reference's result at 4 threads is not its result at 1"
    reference_outputs(f"step5_tail_{name}", workdir, INPUTS, OUTPUTS, run)
    return F.read_paths(os.path.join(workdir, OUTPUTS[0]))

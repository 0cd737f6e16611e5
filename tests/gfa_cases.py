"""Hand-made inputs of the tests of the GFA dump (gfa.gfa_dump, csrc/gfa_dump.hip; the reference's hbv2gfa without line finding):
graphs built with the Builder of step4_cases WITH mirror images, K = 12, real sequences.  The reference pairs the objects by sorting
their sequences (HyperBasevector::Involution), so no two objects of a case share a sequence and no edge is palindromic unless the case
says so: a sequence is A + random bases + A (T .. T for an edge whose mirror image is the canonical one), which never equals a reverse
complement of its kind, and every sequence a case hands out is checked against the ones it handed out before.

    cases() -> {name: Case}; Case.hbv(); Case.inv (the case's own involution); Case.genome_kb (the reference's -g)
    Case.s_ids  the ids of the S lines that must come out, from how the case was built (never from the oracle)
    Case.lines  for the small cases: the L lines that must come out, in order, written by hand from GFADump.cc:228-286
    random_case(seed), SEEDS, seed_conditions(...)   three generated graphs
    ORACLE_ONLY  the cases that are not run against the reference (the oracle's text is the expectation)
    recorded() -> the names whose run of the reference tool lies under tests/golden/refruns/gfa_case_<name>/
    reference_run(name, workdir) -> (bytes of o_raw.gfa or None, its SHA-256, the statistics text)

GFADump.cc:258-285, per object e that is not REV, in ascending e: the followers all_next = the objects leaving to_right[e] and the
inverses of the objects entering to_left[inv e], as a set in ascending id; each n is named by cn = n when n is not REV, else inv[n];
dropped when cn < e; else `L edge<e> + edge<cn> (+ when cn == n, else -) 0M`.  Then the predecessors all_prev = the objects entering
to_left[e] and the inverses of those leaving to_right[inv e] likewise: `L edge<e> - edge<cp> (- when cp == p, else +) 0M`.

An S line is `S\\tedge<id>\\t<bases>\\tCL:z:black\\n`: 19 + digits(id) + length bytes."""
import hashlib
import os
import random

import numpy as np

from conftest import reference_outputs
from step4_cases import Builder, _rc
from w2rap_contigger_amd import formats as F

K = 12
A, C, G, T = 0, 1, 2, 3


def L(e, s1, c, s2):
    return b"L\tedge%d\t%s\tedge%d\t%s\t0M" % (e, s1.encode(), c, s2.encode())


class Case:
    def __init__(self, seed=0, genome_kb=1):
        self.b, self.inv, self.rng, self.used, self.self_mirror = Builder(K), [], random.Random(seed), set(), set()
        self.s_ids, self.lines, self.genome_kb = [], None, genome_kb

    def vertex(self, self_mirror=False):
        """a vertex and its mirror image v ^ 1; self_mirror: a vertex that is its own mirror image (its partner keeps no edges)"""
        v = self.b.vertex()
        if self_mirror:
            self.self_mirror.add(v)
        return v

    def mv(self, v):
        return v if v in self.self_mirror else v ^ 1

    def claim(self, s):
        """s is new to the case, and so is its reverse complement"""
        s = np.asarray(s, np.uint8)
        a, r = s.tobytes(), _rc(s).tobytes()
        assert a not in self.used and r not in self.used, "two objects of a case share a sequence"
        self.used |= {a, r}
        return s

    def seq(self, n, rev=False, middle=None):
        """n bases, A + random + A (rev: T + random + T), new to the case.  Its canonical form is FWD (rev: REV): at an even length base 0
        is A against the T of the reverse complement, at an odd length the middle base is one of A, C (rev: G, T) or `middle`"""
        end = T if rev else A
        for _ in range(400):
            s = [end] + [self.rng.randrange(4) for _ in range(n - 2)] + [end] if n > 1 else [end]
            if n & 1 and n > 1:
                s[n // 2] = self.rng.choice((G, T) if rev else (A, C)) if middle is None else middle
            s = np.array(s, np.uint8)
            if s.tobytes() not in self.used and _rc(s).tobytes() not in self.used:
                return s
        raise ValueError(f"no sequence of {n} bases is left")

    def edge(self, u, v, n=20, rev=False, seq=None):
        """u -> v and its mirror image; rev: the mirror image is the canonical one of the two (seq: `rev` must say what its form is);
        -> the id of u -> v"""
        s = self.claim(self.seq(n, rev) if seq is None else seq)
        e = self.b.edge(u, v, s, mirror=False)
        self.b.edge(self.mv(v), self.mv(u), _rc(s), mirror=False)
        self.inv += [e + 1, e]
        self.s_ids.append(e + 1 if rev else e)
        return e

    def palindrome(self, u, n=20, seq=None):
        """u -> mirror of u with a sequence that is its own reverse complement (n even): inv[e] == e, form PALINDROME, an S line"""
        if seq is None:
            assert n % 2 == 0
            while True:
                x = np.array([self.rng.randrange(4) for _ in range(n // 2)], np.uint8)
                seq = np.concatenate([x, _rc(x)])
                if seq.tobytes() not in self.used:
                    break
        assert np.array_equal(seq, _rc(seq)) and seq.tobytes() not in self.used
        self.used.add(seq.tobytes())
        e = self.b.edge(u, self.mv(u), seq, mirror=False)
        self.inv.append(e)
        self.s_ids.append(e)
        return e

    def hbv(self):
        return self.b.hbv()

    def s_line_lengths(self):
        """the byte count of every S line, in order"""
        return [19 + len(str(e)) + len(self.b.edges[e][2]) for e in sorted(self.s_ids)]


# ---- the link rules, one case each ---------------------------------------------------------------------------------------------------
def _link_cases(out):
    # 0 = a -> v, 2 = v -> v, 4 = v -> b.  e = 0: followers {2, 4}.  e = 2: followers {2, 4}; predecessors {0, 2}: 0 < 2 goes, 2 stays.
    # e = 4: no followers, predecessors {0, 2} both smaller
    c = Case(1); a, v, b = c.vertex(), c.vertex(), c.vertex()
    c.edge(a, v, 14); c.edge(v, v, 15); c.edge(v, b, 16)
    c.lines = [L(0, "+", 2, "+"), L(0, "+", 4, "+"), L(2, "+", 2, "+"), L(2, "+", 4, "+"), L(2, "-", 2, "-")]
    assert c.s_ids == [0, 2, 4]
    out["self_loop"] = c

    # p is its own mirror image: 0 = x -> a, 2 = a -> p, 3 = its inverse p -> mirror of a.  e = 0: follower 2.  e = 2: the follower is 3,
    # REV, named through inv: cn = 2 == e stays, with a minus; predecessor 0 < 2 goes
    c = Case(2); x, a, p = c.vertex(), c.vertex(), c.vertex(self_mirror=True)
    c.edge(x, a, 13); c.edge(a, p, 17)
    c.lines = [L(0, "+", 2, "+"), L(2, "+", 2, "-")]
    assert c.s_ids == [0, 2]
    out["hairpin"] = c

    # 0, 2 = a -> b twice, 4 = b -> d
    c = Case(3); a, b, d = c.vertex(), c.vertex(), c.vertex()
    c.edge(a, b, 18); c.edge(a, b, 18); c.edge(b, d, 12)
    c.lines = [L(0, "+", 4, "+"), L(2, "+", 4, "+")]
    assert c.s_ids == [0, 2, 4]
    out["parallel_edges"] = c

    # 0 = x -> u, 1 = its mirror u' -> x', 2 = P: u -> u' (inv[2] == 2, 14 bases), 3 = u' -> y, 4 = its mirror y' -> u.
    # e = 0: follower 2.  e = 2: followers leaving u' = {1, 3}: 1 is REV, cn = 0 < 2 goes; 3 stays.  predecessors entering u = {0, 4}:
    # 0 goes; 4 is REV, cp = 3, named through inv: plus.  e = 3: predecessor 2 < 3 goes
    c = Case(4); x, u, y = c.vertex(), c.vertex(), c.vertex()
    c.edge(x, u, 15); P = c.palindrome(u, 14); c.edge(u ^ 1, y, 19)
    assert P == 2 and c.inv[P] == P and len(c.b.edges[P][2]) % 2 == 0
    c.lines = [L(0, "+", 2, "+"), L(2, "+", 3, "+"), L(2, "-", 3, "+")]
    assert c.s_ids == [0, 2, 3]
    out["palindromic_edge"] = c

    # 0 = a -> v, 2 = v -> b.  The followers of 0: its own list names 2; the mirrored list (the objects entering the left end of
    # inv 0 = 1, which is the mirror of v: {3}, through inv) names 2 again: one line.  Three-way the same for 4, 6, 8 behind it
    c = Case(5); a, v, b, d = c.vertex(), c.vertex(), c.vertex(), c.vertex()
    c.edge(a, v, 21); c.edge(v, b, 22); c.edge(b, d, 23); c.edge(b, d, 24); c.edge(b, d, 25)
    c.lines = [L(0, "+", 2, "+"), L(2, "+", 4, "+"), L(2, "+", 6, "+"), L(2, "+", 8, "+")]
    assert c.s_ids == [0, 2, 4, 6, 8]
    out["both_lists_name_one_follower"] = c

    # v -> v' carries 2 and its own inverse 3 side by side: both follow 0 = a -> v, two lines for the one segment, + first (raw id 2 in
    # front of raw id 3).  In the second component 6 is REV and 7 the segment: raw id 6 comes first, named through inv: minus first
    c = Case(6); a, v, a2, v2 = c.vertex(), c.vertex(), c.vertex(), c.vertex()
    c.edge(a, v, 13); c.edge(v, v ^ 1, 15); c.edge(a2, v2, 17); c.edge(v2, v2 ^ 1, 19, rev=True)
    c.lines = [L(0, "+", 2, "+"), L(0, "+", 2, "-"), L(4, "+", 7, "-"), L(4, "+", 7, "+")]
    assert c.s_ids == [0, 2, 4, 7]
    out["follower_and_its_inverse"] = c

    # 0 = a -> v is REV, its mirror 1 = v' -> a' is the segment; 2 = v -> b.  e = 1: the predecessors entering v' = {3}, REV, cp = 2:
    # kept from this end, named through inv: plus.  e = 2: predecessor 0 is REV, cp = 1 < 2: dropped
    c = Case(7); a, v, b = c.vertex(), c.vertex(), c.vertex()
    c.edge(a, v, 16, rev=True); c.edge(v, b, 18)
    c.lines = [L(1, "-", 2, "+")]
    assert c.s_ids == [1, 2]
    out["link_dropped_at_one_end_kept_at_the_other"] = c

    c = Case(8); c.edge(c.vertex(), c.vertex(), 27)
    c.lines = []
    assert c.s_ids == [0]
    out["isolated_edge"] = c

    # vertices without edges in front, in the middle and four at the end: both offset arrays hold repeats, the last ones equal to the
    # number of objects
    c = Case(9); c.vertex(); a = c.vertex(); c.vertex(); b = c.vertex(); d = c.vertex(); c.vertex(); c.vertex()
    c.edge(a, b, 14); c.edge(b, d, 15)
    c.lines = [L(0, "+", 2, "+")]
    assert c.s_ids == [0, 2]
    h = c.hbv()
    assert h.n_vertices == 14 and int(h.from_off[-5]) == int(h.from_off[-1]) == 4 and int(h.from_off[2]) == 0
    out["vertices_without_edges"] = c


# ---- the canonical form --------------------------------------------------------------------------------------------------------------
FORM_ODD = (3, 5, 7, 63, 65)                    # the middle base is base 31 of word 0 at 63, base 0 of word 1 at 65
# (length, d): the object and its reverse complement agree on bases [0, d) and differ at base d.  What differs at d differs at
# length - 1 - d as well, so d < length / 2: the first difference lies in word 0 up to length 64, and at 66 it can be base 31 (the last
# of word 0) or base 32 (the first of word 1); it never lies in the last, partial word.  That word decides only for a palindrome, which
# is compared to its end
FORM_EVEN = ((2, 0), (32, 0), (32, 15), (34, 0), (34, 16), (64, 0), (64, 31), (66, 0), (66, 31), (66, 32))
FORM_PALINDROMES = (2, 32, 34, 64, 66)


def _even_seq(rng, n, d, rev):
    """n bases (n even) that equal their reverse complement on [0, d) and differ from it at d, smaller there (rev: larger)"""
    while True:
        s = [rng.randrange(4) for _ in range(n)]
        for i in range(d):
            s[n - 1 - i] = 3 - s[i]
        a, b = s[d], 3 - s[n - 1 - d]
        if (a > b) if rev else (a < b):
            return np.array(s, np.uint8)


def _form_case():
    c = Case(10)
    c.edge(c.vertex(), c.vertex(), seq=[A]); c.edge(c.vertex(), c.vertex(), seq=[G], rev=True)     # one base: it is the middle
    for n in FORM_ODD:
        for mid in (A, C, G, T):
            c.edge(c.vertex(), c.vertex(), seq=c.seq(n, middle=mid), rev=mid in (G, T))
    for n, d in FORM_EVEN:
        for rev in (False, True):
            while True:
                s = _even_seq(c.rng, n, d, rev)
                if s.tobytes() not in c.used and _rc(s).tobytes() not in c.used:
                    break
            c.edge(c.vertex(), c.vertex(), seq=s, rev=rev)
    for n in FORM_PALINDROMES:
        c.palindrome(c.vertex(), n)
    c.lines = []
    return c


# ---- the chunk writer ----------------------------------------------------------------------------------------------------------------
CHUNK_SEED = 0     # set below: chosen on the CPU, the case asserts what it was chosen for


def _chunk_case(seed):
    """edges of every length 1 .. 48 and nine more of 16 bases in a seeded order over 9 vertices, some REV first; ids of
    one, two and three digits.  -> (case, what it lacks)"""
    c = Case(seed)
    rest = list(range(5, 49)) + [16] * 3
    c.rng.shuffle(rest)
    rest = [1, 2, 3, 4] + rest                      # the shortest lines need ids of one digit
    vs = [c.vertex() for _ in range(9)]
    pos, want, sixteens, i = 0, [0, 1], 4, 0        # four more edges of 16 bases are placed where their bases start at 0 and at 1 mod 16
    while rest or sixteens:
        rev = c.rng.random() < 0.3
        e = len(c.b.edges) + rev
        start = (pos + 7 + len(str(e))) % 16
        if sixteens and (start in want or not rest):
            n = 16; sixteens -= 1
            if start in want:
                want.remove(start)
        else:
            n = rest.pop(0)
        c.edge(vs[i % 9], vs[(4 * i + 1) % 9], n, rev=rev)
        pos += 19 + len(str(e)) + n; i += 1
    lens = c.s_line_lengths()
    for m in sorted(set(range(21, max(lens) + 1)) - set(lens)):        # line lengths still missing: an id of three digits and m - 22 bases
        assert len(c.b.edges) >= 100
        c.edge(vs[i % 9], vs[(4 * i + 1) % 9], m - 22); i += 1
    lens = c.s_line_lengths()
    starts = [sum(lens[:i]) for i in range(len(lens))]
    ids = sorted(c.s_ids)
    seq_start_16 = {(st + 7 + len(str(e))) % 16 for st, e in zip(starts, ids) if len(c.b.edges[e][2]) == 16}
    lacks = []
    if {s % 16 for s in starts} != set(range(16)):
        lacks.append("a line start on every residue mod 16")
    if set(lens) != set(range(21, max(lens) + 1)):
        lacks.append("every S line length from 21 bytes up")
    if not {0, 1} <= seq_start_16:
        lacks.append("16 bases that start on a 16-byte boundary, and one byte off")
    if {len(str(e)) for e in ids} != {1, 2, 3}:
        lacks.append("ids of one, two and three digits")
    return c, lacks


# ---- digit counts --------------------------------------------------------------------------------------------------------------------
DIGIT_IDS = [10 ** k - 1 for k in range(1, 6)] + [10 ** k for k in range(1, 6)]


def chain_case(n_pairs):
    """a chain v0 -> v1 -> .. of n_pairs edges of 13 bases (A + 5 + middle + 5 + A, the ten free bases spell the pair's number) and
    their mirror images, closed by a vertex that is its own mirror image: pair i is the objects 2 i and 2 i + 1, and the last edge is
    followed by its own inverse.  The middle base is A, so the even id is the segment -- except in the pairs 4, 49, 499, 4999, 49999,
    whose middle base is G: there the odd id 9, 99, .. is the segment.  Every segment but the first is the second id of an L line of
    the one before it, every segment but the last the first id of its line to the next; the last, 2 n_pairs - 2, has its hairpin
    line.  With 50,001 pairs: 100,002 objects, and 10^k - 1 and 10^k for k = 1 .. 5 each stand as an S id, a first id and a second
    id.  Ids of seven or more digits stay unexercised: ndigits and put_uint loop, nothing in them changes past six digits, and a graph
    of a million objects is too slow for the Python oracle."""
    c = Case()
    flipped = {(10 ** k - 2) // 2 for k in range(1, 6)}
    vs = [c.vertex() for _ in range(n_pairs)] + [c.vertex(self_mirror=True)]
    for i in range(n_pairs):
        free = [(i >> (2 * j)) & 3 for j in range(10)]
        mid = G if i in flipped else A
        c.edge(vs[i], vs[i + 1], seq=[A] + free[:5] + [mid] + free[5:] + [A], rev=mid == G)
    return c


def digit_conditions(text, n_objects):
    """-> which of DIGIT_IDS below n_objects is missing as an S id, as the first or as the second id of an L line of `text`"""
    s, first, second = set(), set(), set()
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        if f[0] == b"S":
            s.add(int(f[1][4:]))
        elif f[0] == b"L":
            first.add(int(f[1][4:])); second.add(int(f[3][4:]))
    return [(i, what) for i in DIGIT_IDS if i < n_objects for what, have in (("S", s), ("first", first), ("second", second)) if i not in have]


# ---- the hub -------------------------------------------------------------------------------------------------------------------------
def hub_case(n):
    """n edges into one vertex and n out of it: n * n L lines, up to 25 bytes each, n of them per object"""
    c = Case(11)
    hub = c.vertex()
    for i in range(n):
        c.edge(c.vertex(), hub, 12 + i % 40, rev=i % 3 == 0)
    for i in range(n):
        c.edge(hub, c.vertex(), 12 + i % 37, rev=i % 5 == 0)
    return c


# ---- the statistics ------------------------------------------------------------------------------------------------------------------
def walk(sizes, denom, stop_at_end, rule):
    """hbv2gfa.cc:70-90 on the canonical sizes under a rule for "the percentage reached" -> the nine values printed"""
    sizes = sorted(sizes, reverse=True)
    k, cs, out = 0, 0, []
    for i in range(10, 100, 10):
        while rule(cs, denom) < i and (not stop_at_end or k < len(sizes)):
            cs += sizes[k]; k += 1
        out.append("n/a" if stop_at_end and k == len(sizes) else str(sizes[k - 1]))
    return out


def ieee(cs, denom):
    """as the source reads"""
    return cs * 100.0 / denom


def reassociated(cs, denom):
    """as the reference tool built with its own flags behaves: one ulp low where the sum lands on a decile"""
    return cs * (100.0 / denom)


def find_stats_lists(seed=5, n_differ=20, n_plain=4):
    """the search that found STATS_LISTS: seeded lists of 3 .. 25 sizes, the first n_differ on which the two rules differ on an N line
    and the first n_plain on which they differ nowhere.  On an NG line at the reference's -g 1 they cannot differ: a sum is a whole
    number, so it reaches a decile of 1000 exactly only at 100, 200 .. 900, and d * 100 * (100.0 / 1000) is not below 10 d for any of
    the nine (nor at -g 2 .. 13); stats_rules_differ counts that too.  The NG walk is held to the rule at genome sizes that are no
    multiple of 1000, the sum of a list among them, against the oracle"""
    R = random.Random(seed)
    differ, plain = [], []
    while len(differ) < n_differ or len(plain) < n_plain:
        sizes = [R.randint(1, 60) * R.choice([1, 5, 10]) + 12 for _ in range(R.randint(3, 25))]
        dn = walk(sizes, sum(sizes), False, ieee) != walk(sizes, sum(sizes), False, reassociated)
        dg = walk(sizes, 1000, True, ieee) != walk(sizes, 1000, True, reassociated)
        if dn and len(differ) < n_differ:
            differ.append(sizes)
        elif not dn and not dg and len(plain) < n_plain:
            plain.append(sizes)
    return differ + plain


STATS_LISTS = [
    [41, 502, 31, 61, 62, 51, 92, 172, 107, 47, 412, 402, 22, 107, 18, 207, 182, 572, 492],
    [237, 212, 27, 482, 292, 16, 282],
    [66, 45, 462, 197],
    [522, 552, 29, 69, 432, 292, 307, 107, 30, 292, 53, 14, 312, 242, 15, 312],
    [232, 16, 247, 187, 152, 232, 412, 232, 16, 51, 237, 312, 552, 17, 41, 57, 55, 142],
    [482, 332, 392, 27, 132, 127, 82, 522, 142, 202, 36, 40, 252, 352],
    [402, 53, 257, 122, 57, 262, 187],
    [33, 18, 482, 31, 71, 162, 65, 77, 59, 59, 32, 82, 63, 54],
    [242, 272, 65, 61, 36, 42, 152, 57, 27, 66, 77, 52, 362, 522, 23, 50, 22, 152, 32],
    [37, 272, 157, 372, 72, 69, 452, 482, 60, 16, 167, 67, 432, 552, 35, 262, 55, 82, 462, 137, 42, 502, 56, 60],
    [127, 402, 257, 582, 71, 52, 31, 82, 272, 58, 67, 167, 312, 252, 242, 77, 29],
    [29, 312, 342, 20, 58, 92, 54, 492, 22, 292, 61, 267, 69, 52, 552, 20, 38],
    [53, 20, 97, 232, 282, 57, 38, 117, 59, 47, 492, 54],
    [50, 92, 67, 222, 452, 45, 46, 212, 142, 20],
    [232, 42, 172, 132, 352, 53, 53, 212, 45, 602, 372, 362, 43],
    [197, 142, 61, 302, 30, 46, 532, 92, 52, 182, 62, 71, 222, 212, 37, 97, 177, 38, 242, 102, 87, 207],
    [237, 302, 39, 117, 207, 32, 22, 122],
    [272, 97, 382, 422, 62, 42, 192, 282, 302, 34, 72, 157, 342, 22],
    [252, 442, 287, 532, 51, 207, 262, 362, 277],
    [39, 45, 22, 222, 61, 292, 292, 42, 49, 14, 462],
    [182, 242, 552, 432, 22, 62, 54, 70, 52, 43, 262, 82, 28, 59, 147, 72, 23, 102, 212, 21, 13, 26],
    [68, 107, 142, 582, 53, 132, 77, 32],
    [39, 72, 29, 122, 542, 50, 402, 242, 37, 127, 322, 33, 167, 58],
    [29, 252, 287, 32],
]


def stats_rules_differ():
    """-> (on how many of STATS_LISTS the two rules differ on an N line, on how many on an NG line at 1000), from the formulas alone"""
    dn = sum(walk(s, sum(s), False, ieee) != walk(s, sum(s), False, reassociated) for s in STATS_LISTS)
    dg = sum(walk(s, 1000, True, ieee) != walk(s, 1000, True, reassociated) for s in STATS_LISTS)
    return dn, dg


def sizes_case(sizes, seed):
    """disjoint edges of these lengths, one in three REV first"""
    c = Case(seed)
    for i, n in enumerate(sizes):
        c.edge(c.vertex(), c.vertex(), n, rev=i % 3 == 1)
    c.lines = []
    return c


def _stats_cases(out):
    for i, sizes in enumerate(STATS_LISTS):
        out[f"stats_{i:02d}"] = sizes_case(sizes, 100 + i)
    out["stats_sizes_1_to_39"] = sizes_case(list(range(1, 40)), 130)          # sum 780: 702 is 90 % exactly, N90 is 12 and not 13
    out["stats_one_contig"] = sizes_case([57], 131)
    out["stats_equal_lengths"] = sizes_case([40] * 25, 132)                   # sum 1000 = the genome size: every decile is hit exactly
    out["stats_genome_larger_than_everything"] = sizes_case([40, 30, 20], 133)   # 90 bases never reach 10 % of 1000: every NG line n/a
    # 300 reaches 30 %; the 200 behind it brings the sum to 50 %, but it is the last contig: NG40 and NG50 are n/a, not 200
    out["stats_decile_reached_on_the_last_contig"] = sizes_case([300, 200], 134)


# ---- generated graphs ----------------------------------------------------------------------------------------------------------------
SEEDS = (1, 2, 3)      # chosen on the CPU: at each the oracle's output alone meets every condition of seed_conditions


def random_case(seed):
    """a mirrored random graph of a few hundred objects, lengths 1 .. 120: 60 vertices, 90 random edges (one in seven across to the
    mirror half), a hub of 55 out-edges and one of 55 in-edges, three cycles, three palindromic edges, three hairpin ends, three
    self-loops and three edges that lie beside their own inverse; pure Python, the same on every machine"""
    c = Case(seed)
    rng = c.rng
    vs = [c.vertex() for _ in range(60)]
    anyv = lambda: rng.choice(vs) ^ (rng.random() < 0.15)
    short = [1, 2, 3]

    def length():
        return short.pop() if short and rng.random() < 0.2 else rng.randint(4, 120)

    def edge(u, v):
        for _ in range(20):
            try:
                return c.edge(u, v, length(), rev=rng.random() < 0.4)
            except ValueError:
                pass
        raise AssertionError("no sequence left")

    for _ in range(90):
        edge(anyv(), anyv())
    out_hub, in_hub = rng.sample(vs, 2)
    for _ in range(55):
        edge(out_hub, anyv()); edge(anyv(), in_hub)
    for _ in range(3):
        cyc = rng.sample(vs, rng.randint(2, 5))
        for i in range(len(cyc)):
            edge(cyc[i], cyc[(i + 1) % len(cyc)])
        c.palindrome(rng.choice(vs), 2 * rng.randint(3, 60))
        edge(rng.choice(vs), c.vertex(self_mirror=True))
        v = rng.choice(vs); edge(v, v)
        v = rng.choice(vs); edge(v, v ^ 1)
    return c


def seed_conditions(c, text, inv):
    """what a generated case must contain, judged from the oracle's text and involution alone -> the list of what is missing"""
    missing = []
    links, per_obj = set(), {}
    s_len = set()
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        if f[0] == b"S":
            s_len.add(len(f[2]))
        elif f[0] == b"L":
            e, n = int(f[1][4:]), int(f[3][4:])
            links.add((e, f[2], n, f[4])); per_obj[e] = per_obj.get(e, 0) + 1
    for s1 in (b"+", b"-"):
        for s2 in (b"+", b"-"):
            if not any(l[1] == s1 and l[3] == s2 and l[0] != l[2] for l in links):
                missing.append(f"an L line {s1.decode()} {s2.decode()} between two segments")
    if not any(l[0] == l[2] and l[1] == l[3] for l in links):
        missing.append("a self-loop's line")
    if not any(l[0] == l[2] and l[1] == b"+" and l[3] == b"-" for l in links):
        missing.append("a hairpin's line")
    if not any((e, s1, n, b"-" if s2 == b"+" else b"+") in links for e, s1, n, s2 in links if e != n):
        missing.append("a segment linked with both signs from one end of another")
    if int(np.sum(np.asarray(inv) == np.arange(len(inv)))) < 3:
        missing.append("three palindromic edges")
    if max(per_obj.values(), default=0) < 55:
        missing.append("an object with 55 L lines")
    if not (min(s_len, default=99) <= 3 and max(s_len, default=0) >= 100):
        missing.append("segments of at most 3 and of at least 100 bases")
    if not 300 <= len(inv) <= 900:
        missing.append("a few hundred objects")
    return missing


# ---- all of them ---------------------------------------------------------------------------------------------------------------------
_CASES = None


def cases():
    """every hand-made case, built once; do not change what it returns"""
    global _CASES
    if _CASES is None:
        out = {}
        _link_cases(out)
        out["canonical_forms"] = _form_case()
        out["chunk_writer"], lacks = _chunk_case(CHUNK_SEED)
        assert not lacks, lacks
        out["digits_1000"] = chain_case(500)
        out["hub_300"] = hub_case(300)
        out["hub_40"] = hub_case(40)
        _stats_cases(out)
        _CASES = out
    return _CASES


# not run against the reference: the oracle's text is the expectation
ORACLE_ONLY = ("digits_100002",)
# the reference's _raw.gfa of these is larger than a committed file may be (hub_300: 90,000 L lines, 2.2 MB): its SHA-256 is recorded in
# o_raw.gfa.sha256 instead of the file, the stdout as everywhere; hub_40 is the same construction with the file itself recorded
DIGEST_ONLY = ("hub_300",)
# cases the reference could not be run on -> its message; they stay on literals and oracle
NOT_RECORDED = {}
_MADE = {}


def case_of(name):
    """the case of any name: hand-made, random_<seed>, or digits_100002; made once"""
    if name not in _MADE:
        if name.startswith("random_"):
            _MADE[name] = random_case(int(name[len("random_"):]))
        elif name == "digits_100002":
            _MADE[name] = chain_case(50001)
        else:
            _MADE[name] = cases()[name]
    return _MADE[name]


def all_names():
    return sorted(cases()) + [f"random_{s}" for s in SEEDS] + list(ORACLE_ONLY)


def recorded():
    return [n for n in all_names() if n not in NOT_RECORDED and n not in ORACLE_ONLY]


_ORACLE = {}


def oracle_of(name):
    """-> (raw_gfa, involution) of the oracle on the case, computed once per session"""
    from oracle import oracle_gfa as OG
    if name not in _ORACLE:
        h = case_of(name).hbv()
        _ORACLE[name] = (OG.raw_gfa(h), OG.involution(h))
    return _ORACLE[name]


def reference_run(name, workdir):
    """stages the case's graph as g.hbv with an empty g.paths in workdir and replays the recorded run of the reference tool
    (recording: oracle/_ref/ref_hbv2gfa -i g -o o -g <genome_kb> at 1 thread and at 4, which must agree)
    -> (the bytes of o_raw.gfa, or None for a case of DIGEST_ONLY; their SHA-256; the statistics text of the stdout)"""
    c = case_of(name)
    F.write_hbv(os.path.join(workdir, "g.hbv"), c.hbv())
    F.write_paths(os.path.join(workdir, "g.paths"), np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, np.int32))
    digest_only = name in DIGEST_ONLY

    def run():
        from oracle import oracle_gfa as OG
        got = [OG.run_reference_gfa(workdir, "g", "o", c.genome_kb, threads=t) for t in (1, 4)]
        assert got[0] == got[1], f"{name}: the reference's result at 4 threads is not its result at 1"
        if digest_only:
            with open(os.path.join(workdir, "o_raw.gfa.sha256"), "w") as f:
                f.write(hashlib.sha256(got[0][1]).hexdigest() + "\n")
        return got[0][0]
    txt = reference_outputs(f"gfa_case_{name}", workdir, ["g.hbv", "g.paths"], ["o_raw.gfa.sha256" if digest_only else "o_raw.gfa"], run)
    stats = txt.split("=== Graph stats === \n")[1].split("Dumping gfa")[0]
    if digest_only:
        return None, open(os.path.join(workdir, "o_raw.gfa.sha256")).read().strip(), stats
    raw = open(os.path.join(workdir, "o_raw.gfa"), "rb").read()
    return raw, hashlib.sha256(raw).hexdigest(), stats

"""Hand-made inputs for the vote of Step 4 (k4_walks .. k4_verdict) at K = 20, built with step4_cases.Hand: every case sits on a boundary
of the reference's rule (Clean200.cc:267-443), so that one wrong comparison, index or partial sum flips what is deleted.
test_step4_vote_model.py proves on the CPU model that each case sits where its name says; test_gpu_step4_vote.py compares the library.

    vote_cases() -> name -> Case(inputs = (hbv, paths, (packed, byte_off, read_len), quals, min_size), expect = {...}, hand = the Hand)
    random_case(seed) -> Hand          SEEDS: the 24 seeds the tests run

The building block is the SNP bubble a -> v -> {b, c, ..}: the out-edges are J[v] + 300 shared inner bases + J[w] and differ in one base,
so a read cut from [a, b] scores for b exactly the quality it has at that base (its margin), and a read that does not cover the base is a
placement that scores nothing.  The order of the placements within one (vertex, task) is arbitrary on the device: no case depends on it.

expect: deleted = what pass 1's vote (and min_size) deletes; vertex / offset = the tested branch vertex and the placement of the pass at
which it starts; drop_keeps / dup_keeps = read ids of which ANY one removed / duplicated must leave nothing deleted; walks = {vertex: walks};
depth = {vertex: depth}; skipped = n_skipped_too_many_exts of pass 1; placements = n_placements of pass 1; fewer_than_listed = the skip
rule of roles 1 and 3 dropped some listing."""
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from step4_cases import Hand, _rc, _seq

K = 20


@dataclass
class Case:
    inputs: tuple
    expect: dict = field(default_factory=dict)
    hand: object = None


def bubble(h, n_out=2, snp=30, own=False, inner=300, n_in=1, in_len=200):
    """n_in in-edges -> v -> n_out out-edges that share their inner bases.  own: out-edge j has its own substitution at edge position
    snp + j; else out-edge 0 is the shared sequence and out-edge j > 0 has base + j at edge position snp"""
    us = [h.vertex() for _ in range(n_in)]
    v = h.vertex()
    ins = [h.edge(u, v, in_len) for u in us]
    shared = _seq(h.rng, inner)
    outs = []
    for j in range(n_out):
        w = h.vertex()
        s = shared.copy()
        if own:
            s[snp + j - (K - 1)] = (s[snp + j - (K - 1)] + 1) & 3
        elif j:
            s[snp - (K - 1)] = (s[snp - (K - 1)] + j) & 3
        outs.append(h.edge(v, w, 0, seq=np.concatenate([h.J[v], s, h.J[w]])))
    return SimpleNamespace(v=v, ins=ins, outs=outs, snp=snp, own=own)


def vread(h, B, j, q, i_in=0, offset=None, length=150, rc=False, other=30):
    """a read from [in-edge i_in, out-edge j] with quality q at out-edge j's SNP, 0 at the other out-edges' own SNPs, `other` elsewhere"""
    a = B.ins[i_in]
    A = len(h.b.edges[a][2]) - (K - 1)                       # the walk position of the out-edge's base 0
    mine = B.snp + (j if B.own else 0)
    if offset is None:
        offset = A + mine - 99
    qual = np.full(length, other, np.uint8)
    if B.own:
        for k in range(len(B.outs)):
            if 0 <= A + B.snp + k - offset < length:
                qual[A + B.snp + k - offset] = 0
    if 0 <= A + mine - offset < length:
        qual[A + mine - offset] = q
    h.read([a, B.outs[j]], offset, length, qual=qual, rc=rc)
    return len(h.paths) - 1


def votes(h, B, j, margins, i_in=None, first_rc=0):
    """one read per margin for out-edge j, every second one from the other strand, at varying offsets; -> their read ids"""
    out = []
    for i, q in enumerate(margins):
        A = len(h.b.edges[B.ins[0]][2]) - (K - 1)
        mine = B.snp + (j if B.own else 0)
        out.append(vread(h, B, j, q, i_in=(i % len(B.ins)) if i_in is None else i_in, offset=A + mine - 140 + (i * 7) % 90, rc=bool((i + first_rc) & 1)))
    return out


def fillers(h, B, n):
    """n reads on the in-edge alone: placements of v that lie before the window and score nothing"""
    out = []
    for i in range(n):
        h.read([B.ins[0]], 5 + (i * 3) % 100, 60, qual=np.full(60, (i * 5) % 64, np.uint8), rc=bool(i & 1))
        out.append(len(h.paths) - 1)
    return out


def empty_read(h, length):
    """a read that has no path"""
    h.paths.append([]); h.offs.append(0); h.codes.append(_seq(h.rng, length)); h.quals.append(np.full(length, 41, np.uint8))


def _both(e):
    return sorted([e, e + 1])                                # an edge and its mirror (Hand adds the mirror right behind it)


def _case(h, expect, min_size=0):
    return Case(h.case() + (min_size,), expect, h)


# ------------------------------------------------------------------------------------------------------------------ A: the verdict
def _two_sided(seed, win, lose):
    h = Hand(seed=seed); B = bubble(h)
    votes(h, B, 0, win); votes(h, B, 1, lose, first_rc=1)
    return h, B


def group_a():
    out = {}
    def pair(name, seed, del_case, keep_case):
        for tag, (win, lose), dele in (("deletes", del_case, True), ("keeps", keep_case, False)):
            h, B = _two_sided(seed, win, lose)
            out[f"a_{name}_{tag}"] = _case(h, {"deleted": _both(B.outs[1]) if dele else [], "vertex": B.v})
    pair("min_win_100_99", 101, ([40, 40, 20], []), ([40, 40, 19], []))
    pair("max_lose_50_51", 102, ([63, 63, 63, 63, 8], [50]), ([63, 63, 63, 63, 63], [51]))
    pair("max_lose_50_51_two_reads", 103, ([63] * 5, [20, 30]), ([63] * 5, [21, 30]))
    pair("min_ratio_150_149", 104, ([63, 63, 24], [30]), ([63, 63, 23], [30]))
    pair("min_ratio_two_losers", 105, ([63, 63, 34], [16, 16]), ([63, 63, 33], [16, 16]))
    # the loser's margins are all d: it is dropped at threshold d exactly; the winner reaches min_win at d (63 + n * (d + 1)) and falls to 63
    # at d + 1, so margins d + 1 on the loser's side keep it at every threshold
    for d in (0, 1, 7, 14):
        n_win = -(-37 // (d + 1))
        n_lose = {0: 2, 1: 51, 7: 8, 14: 4}[d]
        keep_lose = -(-51 // (d + 1))
        pair(f"threshold_d{d}", 110 + d, ([63] + [d + 1] * n_win, [d] * n_lose), ([63] + [d + 1] * n_win, [d + 1] * keep_lose))
    pair("threshold_d15", 125, ([63, 63], [15] * 4), ([63, 63], [16] * 4))
    # three out-edges
    def three(name, seed, sums, dead):
        h = Hand(seed=seed); B = bubble(h, n_out=3)
        for j, ms in enumerate(sums):
            votes(h, B, j, ms, first_rc=j)
        out[f"a_three_way_{name}"] = _case(h, {"deleted": sorted(x for j in dead for x in _both(B.outs[j])), "vertex": B.v})
    three("ranks_1_and_2_deleted", 130, ([63, 63], [10, 10], [5, 5]), (1, 2))
    three("middle_ties_with_loser_both_deleted", 131, ([63, 63], [12, 13], [13, 12]), (1, 2))
    three("middle_ties_with_loser_ratio_keeps_both", 132, ([63, 62], [26], [26]), ())
    three("only_the_last_rank", 133, ([63, 63], [26, 26], [5, 5]), (2,))
    three("two_tie_at_the_top", 134, ([10, 10], [63, 63], [63, 63]), (0,))
    return out


# ------------------------------------------------------------------------------------------------------------------ B: k4_reduce tiles
def group_b():
    out = {}
    def padded(seed, pads):
        h = Hand(seed=seed)
        for n in pads:
            fillers(h, bubble(h), n)
        return h, bubble(h)
    # four placements of margin 25 at placements 254 .. 257: two in each tile, top = 100 needs every one
    h, B = padded(201, (200, 54))
    r = votes(h, B, 0, [25] * 4)
    out["b_straddle_winner"] = _case(h, {"deleted": _both(B.outs[1]), "vertex": B.v, "offset": 254, "drop_keeps": r})
    # the loser holds 25 + 25 = 50 against 4 x 63: its forward read is placement 254 or 255, its reverse read lies in the next tile, so
    # its sum is made of two partial sums whatever the order within a task; one of them added twice (75) keeps c.  (Margins of 10 would
    # not do: a sum of them counted twice is still dropped as a whole at threshold 10, where c is then deleted after all)
    h, B = padded(202, (101, 153))
    l = [vread(h, B, 1, 25, offset=140), vread(h, B, 1, 25, offset=163, rc=True)]
    vread(h, B, 0, 63, offset=151)
    for i in range(3):
        vread(h, B, 0, 63, offset=120 + 13 * i, rc=True)
    out["b_straddle_loser"] = _case(h, {"deleted": _both(B.outs[1]), "vertex": B.v, "offset": 254, "n": 6, "dup_keeps": l})
    # placements 250 .. 769: 250 + 50 scoring reads of margin 1 and 220 that do not cover the SNP; 250 >= 5 * 50 exactly
    h, B = padded(203, (250,))
    w = votes(h, B, 0, [1] * 250); f = fillers(h, B, 220); l = votes(h, B, 1, [1] * 50, first_rc=1)
    out["b_three_tiles"] = _case(h, {"deleted": _both(B.outs[1]), "vertex": B.v, "offset": 250, "n": 520, "drop_keeps": w[::31] + w[-1:], "dup_keeps": l[::9] + l[-1:]})
    # 40 vertices of 5 or 6 placements in one tile, top = 100 and top = 99 in turn
    h = Hand(seed=204); dead = []; tops = {}
    for i in range(40):
        B = bubble(h)
        votes(h, B, 0, [25, 25, 25, 25 - (i & 1)], first_rc=i)
        fillers(h, B, 1 + (i % 3 == 0))
        tops[B.v] = 100 - (i & 1)
        if not i & 1:
            dead += _both(B.outs[1])
    out["b_many_vertices_in_a_tile"] = _case(h, {"deleted": sorted(dead), "max_placements": 256, "n_vertices": 40})
    return out


# ------------------------------------------------------------------------------------------------------------------ C: shapes of the vertex
def group_c():
    out = {}
    # in-degree 3: reads through every in-edge (listed under the out-edge as well: skipped there), reads that start on an out-edge (placed
    # there), both strands.  The loser holds 50: a read placed under both roles would count twice
    h = Hand(seed=301); B = bubble(h, n_in=3)
    votes(h, B, 0, [63] * 6); votes(h, B, 1, [17, 17, 16], first_rc=1)
    for i in range(4):                                       # start on the out-edge, SNP covered: margin 1 each for b
        q = np.full(150, 30, np.uint8); q[B.snp - 3 * i] = 1
        h.read([B.outs[0]], 3 * i, 150, qual=q, rc=bool(i & 1))
    out["c_in_degree_3"] = _case(h, {"deleted": _both(B.outs[1]), "vertex": B.v, "fewer_than_listed": True, "walks": {B.v: 2}})
    # out-degree 10, the last out-edge wins / is the only loser
    h = Hand(seed=302); B = bubble(h, n_out=10, own=True)
    votes(h, B, 9, [63, 63]); votes(h, B, 0, [30, 30], first_rc=1)
    out["c_out_degree_10_last_wins"] = _case(h, {"deleted": sorted(x for j in range(1, 9) for x in _both(B.outs[j])), "vertex": B.v, "walks": {B.v: 10}})
    h = Hand(seed=303); B = bubble(h, n_out=10, own=True)
    for j in range(9):
        votes(h, B, j, [63, 63], first_rc=j)
    votes(h, B, 9, [10, 10])
    out["c_out_degree_10_last_loses"] = _case(h, {"deleted": _both(B.outs[9]), "vertex": B.v, "walks": {B.v: 10}})
    h = Hand(seed=304); B = bubble(h, n_out=11, own=True)
    votes(h, B, 10, [63, 63]); votes(h, B, 0, [30, 30], first_rc=1)
    out["c_out_degree_11_skipped"] = _case(h, {"deleted": [], "skipped": 1, "placements": 0})
    # a self-loop beside an in-edge and an out-edge: the loop is in To(v) and in From(v); walks [l, l, l], [b], [l, b], [l, l, b]
    h = Hand(seed=305); u, v, w = h.vertex(), h.vertex(), h.vertex()
    a = h.edge(u, v, 200); l = h.edge(v, v, 100); b = h.edge(v, w, 300)
    for i in range(4):
        h.read([a, b], 150 + 4 * i, 150, rc=bool(i & 1))
        h.read([a, l, b], 160 + 5 * i, 250, qual=np.arange(250) % 64, rc=bool(i & 1))
        h.read([a, l, l, b], 170 + 6 * i, 380, qual=(np.arange(380) * 7) % 64, rc=not i & 1)
    h.read([l, l], 7, 200); h.read([l], 3, 90, rc=True)
    out["c_self_loop"] = _case(h, {"deleted": [], "vertex": v, "walks": {v: 4}})
    # an out-edge v -> v' that is its own mirror image, beside b which shares its first half but for the SNP.  inv[pal] == pal: a read of
    # [a, pal] is placed forward through a and once more as a reverse placement through pal.  The palindrome is the last edge made, so
    # that every other edge has its mirror at id ^ 1
    h = Hand(seed=306); u, v, w = h.vertex(), h.vertex(), h.vertex()
    a = h.edge(u, v, 200)
    half = _seq(h.rng, 150)
    s = np.concatenate([half, _rc(half)]); s[30 - (K - 1)] = (s[30 - (K - 1)] + 1) & 3
    b = h.edge(v, w, 0, seq=np.concatenate([h.J[v], s, h.J[w]]))
    pal = h.edge(v, v ^ 1, 0, seq=np.concatenate([h.J[v], half, _rc(half), h.J[v ^ 1]]))
    assert pal == len(h.b.edges) - 1
    for i in range(4):
        q = np.full(150, 30, np.uint8); q[219 + 30 - (150 + 5 * i)] = 25
        h.read([a, b], 150 + 5 * i, 150, qual=q, rc=bool(i & 1))
    for i in range(2):
        q = np.full(150, 30, np.uint8); q[219 + 30 - (140 + 9 * i)] = 10
        h.read([a, pal], 140 + 9 * i, 150, qual=q)
        c = h.cat([a, pal])[131 + 9 * i:281 + 9 * i]        # the same walk read from the other strand: [pal, a']
        h.paths.append([pal, a + 1]); h.offs.append(len(h.cat([a, pal])) - 281 - 9 * i); h.codes.append(_rc(c)); h.quals.append(np.full(150, 7 + i, np.uint8))
    out["c_palindromic_out_edge"] = _case(h, {"deleted": [pal], "vertex": v, "walks": {v: 2}, "more_placements_than_reads": True})
    # out-edge b of exactly 249 / 250 / 251 k-mers with two edges behind it; c differs from every walk through b in the SNP and from
    # position 19 + m on.  Qualities are 0 but at the SNP and at window positions 268 (the last one: counts) and 269 (the first outside)
    def walk_len(kmers, fan, seed):
        h = Hand(seed=seed); u, v, w, x = h.vertex(), h.vertex(), h.vertex(), h.vertex()
        m = kmers - (K - 1)
        a = h.edge(u, v, 200)
        shared = _seq(h.rng, 300)
        b = h.edge(v, w, 0, seq=np.concatenate([h.J[v], shared[:m], h.J[w]]))
        fs = [h.edge(w, h.vertex(), 300) for _ in range(fan)]
        walks = [h.cat([b, f]) for f in fs]
        s = shared.copy(); s[30 - (K - 1)] = (s[30 - (K - 1)] + 1) & 3
        for p in range(K - 1 + m, K - 1 + 300):
            s[p - (K - 1)] = next(t for t in range(4) if all(wk[p] != t for wk in walks[:2]))
        c = h.edge(v, x, 0, seq=np.concatenate([h.J[v], s, h.J[x]]))
        def rd(path, q_snp, q268, q269, rc):
            q = np.zeros(300, np.uint8); q[219 + 30 - 200] = q_snp; q[219 + 268 - 200] = q268; q[219 + 269 - 200] = q269
            h.read(path, 200, 300, qual=q, rc=rc)
        for i in range(4):
            rd([a, b, fs[i % 2]], 20, 5, 40, bool(i & 1))     # 4 x 25 = 100 if position 268 counts and 269 does not
        for i in range(5):
            rd([a, c], 5, 5, 40, not i & 1)                  # 5 x 10 = 50 likewise
        return h, v, b, c
    for kmers, n_walks in ((249, 3), (250, 2), (251, 2)):
        h, v, b, c = walk_len(kmers, 2, 310 + kmers)
        out[f"c_walk_{kmers}_kmers"] = _case(h, {"deleted": _both(c), "vertex": v, "walks": {v: n_walks}, "depth": {v: 250}})
    # ten edges behind b: at 250 k-mers b is not extended (2 walks, voted), at 249 it is (11 walks, skipped)
    h, v, b, c = walk_len(250, 10, 320)
    out["c_walk_250_kmers_fan_10"] = _case(h, {"deleted": _both(c), "vertex": v, "walks": {v: 2}, "skipped": 0})
    h, v, b, c = walk_len(249, 10, 321)
    out["c_walk_249_kmers_fan_10"] = _case(h, {"deleted": [], "vertex": v, "skipped": 1})
    # a dead end of K - 1 k-mers behind c (119 k-mers): depth 138 after pass 1 of GetExtensions, window 157
    h = Hand(seed=322); u, v, w, x, y = (h.vertex() for _ in range(5))
    a = h.edge(u, v, 200)
    shared = _seq(h.rng, 300)
    b = h.edge(v, w, 0, seq=np.concatenate([h.J[v], shared, h.J[w]]))
    s = shared[:100].copy(); s[30 - (K - 1)] = (s[30 - (K - 1)] + 1) & 3
    c = h.edge(v, x, 0, seq=np.concatenate([h.J[v], s, h.J[x]]))
    t = h.edge(x, y, 0)
    bw, cw = h.cat([b]), h.cat([c, t])
    differ = [p for p in range(119, 157) if bw[p] != cw[p]]
    last = max(differ)                                       # the last window position at which the walks differ ...
    after = next(p for p in range(157, 200) if bw[p] != (cw[p] if p < len(cw) else 9))      # ... and a base of the read behind the window
    for i in range(4):
        q = np.zeros(300, np.uint8); q[219 + 30 - 100] = 20; q[219 + last - 100] = 5; q[219 + after - 100] = 40
        h.read([a, b], 100, 300, qual=q, rc=bool(i & 1))
    for i in range(5):
        n = 219 + len(cw) - 100
        q = np.zeros(n, np.uint8); q[219 + 30 - 100] = 5; q[219 + last - 100] = 5
        h.read([a, c, t], 100, n, qual=q, rc=not i & 1)
    out["c_dead_end_lowers_depth"] = _case(h, {"deleted": _both(c), "vertex": v, "walks": {v: 2}, "depth": {v: 138}})
    return out


# ------------------------------------------------------------------------------------------------------------------ D: read windows
def group_d():
    out = {}
    def base(seed, snp=30, win=(25, 25, 25)):
        h = Hand(seed=seed); B = bubble(h, snp=snp)
        votes(h, B, 0, list(win))
        return h, B
    def pair(name, seed, make, snp=30):
        """three reads of margin 25 and the read under test: 100 if it scores exactly 25, else 75 or another sum"""
        for tag, q in (("deletes", 25), ("keeps", 24)):
            h, B = base(seed, snp)
            make(h, B, q)
            out[f"d_{name}_{tag}"] = _case(h, {"deleted": _both(B.outs[1]) if q == 25 else [], "vertex": B.v})
    A = 219
    # the read starts 100 bases before the window (start = -100) / 218 before it
    pair("starts_100_before", 401, lambda h, B, q: vread(h, B, 0, q, offset=A - 100))
    pair("starts_100_before_rc", 402, lambda h, B, q: vread(h, B, 0, q, offset=A - 100, rc=True))
    # 400 bases over a window of 269: the read overhangs both ends
    pair("longer_than_the_window", 403, lambda h, B, q: vread(h, B, 0, q, offset=A - 100, length=400, other=63))
    pair("longer_than_the_window_rc", 404, lambda h, B, q: vread(h, B, 0, q, offset=A - 100, length=400, other=63, rc=True))
    # quality 63 at the SNP: 63 + 37 = 100, 63 + 36 = 99
    for tag, q in (("deletes", 37), ("keeps", 36)):
        h = Hand(seed=405); B = bubble(h)
        votes(h, B, 0, [63, q])
        out[f"d_quality_63_{tag}"] = _case(h, {"deleted": _both(B.outs[1]) if q == 37 else [], "vertex": B.v})
    # the only base of the read inside the window is the window's last one (position 268): the first base of a forward read, the last base
    # of a read of the other strand.  The SNP at 268 scores, the SNP at 269 does not
    for rc in (False, True):
        for snp, dele in ((268, True), (269, False)):
            h = Hand(seed=406); B = bubble(h, snp=snp)
            for i in range(3):                                # these start on b: 25 at the SNP each
                q = np.full(150, 30, np.uint8); q[snp - (128 + 7 * i)] = 25
                h.read([B.outs[0]], 128 + 7 * i, 150, qual=q, rc=bool(i & 1))
            q = np.full(60, 30, np.uint8); q[snp - 268] = 25
            h.read([B.outs[0]], 268, 60, qual=q, rc=rc)
            out[f"d_one_base_inside_{'rc' if rc else 'fw'}_snp_{snp}"] = _case(h, {"deleted": _both(B.outs[1]) if dele else [], "vertex": B.v})
    # reads placed wholly outside the window (before it on a, behind it on b), one with quality 0 under the mismatch; the loser holds 50
    for tag, q0 in (("deletes", 0), ("keeps", 16)):
        h = Hand(seed=407); B = bubble(h)
        votes(h, B, 0, [63] * 4); votes(h, B, 1, [25, 25], first_rc=1)
        vread(h, B, 1, q0, rc=True); vread(h, B, 1, q0, offset=120)
        h.read([B.ins[0]], 0, 100, qual=63); h.read([B.ins[0]], 19, 100, qual=63, rc=True)            # ends 100 bases before the window
        h.read([B.outs[0]], 269, 60, qual=63); h.read([B.outs[1]], 275, 60, qual=63, rc=True)           # starts at the window's end / behind it
        out[f"d_quality_0_and_outside_{tag}"] = _case(h, {"deleted": _both(B.outs[1]) if q0 == 0 else [], "vertex": B.v})
    # read lengths 149, 150, 151, 153: four reads of the other strand whose SNP falls on each of the four bases of a packed byte, and empty
    # paths between them
    for length in (149, 150, 151, 153):
        for tag, last in (("deletes", 25), ("keeps", 24)):
            h = Hand(seed=410 + length); B = bubble(h)
            phases = []
            for i in range(4):
                empty_read(h, 61 + i)
                off = A + 30 - 60 - i                         # the SNP at base 60 + i of the cut, base length - 61 - i of the read
                vread(h, B, 0, last if i == 3 else 25, offset=off, length=length, rc=True)
                phases.append((length - 61 - i) % 4)
            assert sorted(phases) == [0, 1, 2, 3]
            empty_read(h, 20)
            out[f"d_length_{length}_{tag}"] = _case(h, {"deleted": _both(B.outs[1]) if last == 25 else [], "vertex": B.v})
    return out


# ------------------------------------------------------------------------------------------------------------------ E: min_size
def group_e():
    h = Hand(seed=501)
    def lone(kmers):
        u, v = h.vertex(), h.vertex()
        if kmers >= K - 1:
            return h.edge(u, v, kmers - (K - 1))
        s = _seq(h.rng, kmers + K - 1)                        # shorter than two junctions: they overlap
        h.J[u] = s[:K - 1]; h.J[u ^ 1] = _rc(h.J[u]); h.J[v] = s[-(K - 1):]; h.J[v ^ 1] = _rc(h.J[v])
        return h.edge(u, v, 0, seq=s)
    e40, e41, e1, e2 = lone(40), lone(41), lone(1), lone(2)
    v = h.vertex(); loop = h.edge(v, v, 2)                    # a self-loop component: v == w
    s0, s1, t = h.vertex(), h.vertex(), h.vertex()
    two_in = [h.edge(s0, t, 3), h.edge(s1, t, 4)]             # the end vertex has a second in-edge
    x, y, z = h.vertex(), h.vertex(), h.vertex()
    chain = [h.edge(x, y, 1), h.edge(y, z, 2)]                # the start vertex of y -> z has an in-edge
    B = bubble(h)                                            # a branch, so that the vote runs as well
    votes(h, B, 0, [40, 40, 20])
    h.read([e41], 5, 50); h.read([e40], 2, 45, rc=True); h.read(chain, 3, 40)
    dead = sorted(x for e in (e40, e1, e2, B.outs[1]) for x in _both(e))
    return {"e_min_size_40": _case(h, {"deleted": dead, "stay": [e41, loop] + two_in + chain}, min_size=40)}


def vote_cases():
    out = {}
    for g in (group_a, group_b, group_c, group_d, group_e):
        out.update(g())
    return out


# ------------------------------------------------------------------------------------------------------------------ F: random graphs
SEEDS = list(range(24))


def mirror_ids(h):
    """edge id -> the id of its mirror image (itself for a palindromic edge)"""
    m, i, E = {}, 0, h.b.edges
    while i < len(E):
        if i + 1 < len(E) and E[i + 1][0] == E[i][1] ^ 1 and E[i + 1][1] == E[i][0] ^ 1 and np.array_equal(E[i + 1][2], _rc(E[i][2])) \
                and not (E[i][1] == E[i][0] ^ 1 and np.array_equal(E[i][2], _rc(E[i][2]))):
            m[i] = i + 1; m[i + 1] = i; i += 2
        else:
            m[i] = i; i += 1
    return m


def random_case(seed):
    """a graph of runs, bubbles, branches, tips, at most one vertex of out-degree 10 .. 12, one self-loop, one palindromic edge and one
    circle of one-in one-out vertices, with reads along weighted random walks: an edge of weight 0 has no read and loses the vote"""
    rng = np.random.default_rng(7000 + seed)
    h = Hand(K=K, seed=9000 + seed)
    W = {}

    def edge(u, v, m, w=1.0, seq=None):
        e = h.edge(u, v, m, seq=seq); W[e] = w
        return e

    target = int(rng.integers(30, 121))
    left = lambda: target - h.b.nv // 2
    once = {"big": seed % 3 != 2, "loop": seed % 2 == 0, "deep": seed % 4 < 2, "circle": seed % 5 < 3}
    pal_at = None
    cur = h.vertex()

    def run(n):
        nonlocal cur
        for _ in range(n):
            nxt = h.vertex(); edge(cur, nxt, int(rng.integers(1, 70))); cur = nxt

    def side(frm, w, m=None):
        """a side branch off `frm`: one edge, sometimes a second behind it"""
        x = h.vertex(); edge(frm, x, int(rng.integers(80, 330)) if m is None else m, w)
        if rng.random() < 0.3:
            edge(x, h.vertex(), int(rng.integers(20, 200)), w)

    run(int(rng.integers(1, 6)))
    while left() > 14:
        kind = rng.choice(["run", "bubble", "branch", "tip", "deep", "big", "loop", "circle"], p=[0.22, 0.22, 0.2, 0.12, 0.08, 0.06, 0.05, 0.05])
        if kind == "run":
            run(int(min(rng.integers(1, 41), left() - 14)))
        elif kind == "bubble":
            nxt = h.vertex(); m = int(rng.integers(60, 330))
            s = _seq(rng, m); s2 = s.copy()
            for p in rng.choice(m, int(rng.integers(1, 4)), replace=False):
                s2[p] = (s2[p] + int(rng.integers(1, 4))) & 3
            edge(cur, nxt, 0, 1.0, np.concatenate([h.J[cur], s, h.J[nxt]]))
            edge(cur, nxt, 0, float(rng.choice([1.0, 0.05, 0.0, 0.0])), np.concatenate([h.J[cur], s2, h.J[nxt]]))
            cur = nxt
        elif kind == "branch":
            for _ in range(int(rng.integers(0, 3))):
                edge(h.vertex(), cur, int(rng.integers(50, 250)))
            for _ in range(int(rng.integers(1, 4))):
                side(cur, float(rng.choice([1.0, 0.3, 0.0, 0.0])))
            nxt = h.vertex(); edge(cur, nxt, int(rng.integers(80, 330))); cur = nxt
        elif kind == "tip":
            edge(cur, h.vertex(), int(rng.integers(0, 42)), float(rng.choice([1.0, 0.1, 0.0])))          # 19 .. 60 k-mers
            nxt = h.vertex(); edge(cur, nxt, int(rng.integers(100, 300))); cur = nxt
        elif kind == "deep" and once["deep"]:
            # 12 walks at cur in pass 1 (skipped); pass 1 cuts the fan behind b down to one edge, pass 2 votes at cur and deletes c
            once["deep"] = False
            w, x = h.vertex(), h.vertex()
            edge(cur, w, 100); edge(cur, x, 100, 0.0)
            nxt = h.vertex(); edge(w, nxt, 300)
            for _ in range(5):
                edge(w, h.vertex(), 300, 0.0)
            for _ in range(6):
                edge(x, h.vertex(), 300, 0.0)
            cur = nxt
        elif kind == "big" and once["big"]:
            once["big"] = False
            deg = int(rng.integers(10, 13))
            nxt = h.vertex(); edge(cur, nxt, int(rng.integers(240, 330)))
            for _ in range(deg - 1):
                edge(cur, h.vertex(), int(rng.integers(240, 330)), float(rng.choice([1.0, 0.0])))
            cur = nxt
        elif kind == "loop" and once["loop"]:
            once["loop"] = False
            edge(cur, cur, int(rng.integers(30, 120)), 0.4)
            nxt = h.vertex(); edge(cur, nxt, int(rng.integers(100, 300))); cur = nxt
            if pal_at is None:
                pal_at = cur
        elif kind == "circle" and once["circle"]:
            once["circle"] = False
            c = [h.vertex() for _ in range(3)]
            for i in range(3):
                edge(c[i], c[(i + 1) % 3], int(rng.integers(30, 90)))
    run(max(1, left()))
    if pal_at is not None and seed % 4 == 0:                  # the palindromic edge is made last: every other mirror sits at id ^ 1
        half = _seq(rng, int(rng.integers(20, 160)))
        edge(pal_at, pal_at ^ 1, 0, 0.5, np.concatenate([h.J[pal_at], half, _rc(half), h.J[pal_at ^ 1]]))
    # ---- reads
    mir = mirror_ids(h)
    E = h.b.edges
    wt = np.array([W.get(e, W.get(mir[e], 0.0)) for e in range(len(E))])
    outs = {}
    for e, (u, v, _) in enumerate(E):
        outs.setdefault(u, []).append(e)
    p_start = wt * np.array([len(s) for _, _, s in E], float)
    p_start /= p_start.sum()
    for _ in range(int(rng.integers(200, 1501))):
        length = int(rng.integers(60, 301))
        if rng.random() < 0.1:
            h.paths.append([]); h.offs.append(0); h.codes.append(_seq(rng, length)); h.quals.append(rng.integers(0, 64, length).astype(np.uint8))
            continue
        e = int(rng.choice(len(E), p=p_start))
        path = [e]
        offset = int(rng.integers(0, len(E[e][2]) - K + 1))
        have = len(E[e][2]) - offset
        while have < length:
            nx = outs.get(E[path[-1]][1], [])
            pw = np.array([wt[x] for x in nx])
            if not len(nx) or pw.sum() == 0:
                break
            path.append(int(rng.choice(nx, p=pw / pw.sum())))
            have += len(E[path[-1]][2]) - (K - 1)
        if have < length:                                     # the walk ended: the read ends with it, and starts earlier if that makes it too short
            offset = max(0, offset - max(0, 60 - have))
            length = len(h.cat(path)) - offset
        if length < 60:
            path, offset, length = [], 0, 60
            h.paths.append([]); h.offs.append(0); h.codes.append(_seq(rng, length)); h.quals.append(rng.integers(0, 64, length).astype(np.uint8))
            continue
        c = h.cat(path)[offset:offset + length].copy()
        for p in rng.choice(length, int(rng.integers(0, 3)), replace=False):
            c[p] = (c[p] + int(rng.integers(1, 4))) & 3
        h.paths.append(path); h.offs.append(offset); h.codes.append(c); h.quals.append(rng.integers(0, 64, length).astype(np.uint8))
    return h

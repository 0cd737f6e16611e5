"""Hand-made graphs for the graph edit of Step 4 (delete, merge runs, renumber), at K = 20, built with step4_cases.Hand / Builder.
Each is the smallest graph that exercises one rule of RemoveUnneededVertices2 / CleanupCore as the two stacks of the reference define
it; `edit_cases()` also returns, per case, what test_step4_edit_model.py asserts about the model's output so that a green test means
the rule was really exercised.

    edit_cases() -> name -> Case(inputs = (hbv, paths, (packed, byte_off, read_len), quals, min_size), expect = {...})

`empty_cases()` and `no_reads_case()` are the shapes at which the driver around the edit, not the edit, can go wrong: a graph without an
edge (nothing to run a kernel on: the device edit declines) and a graph that changes while there is no read path to rewrite.

Everything Hand / Builder makes is numbered alike: a vertex and its mirror are v and v ^ 1, an edge and its mirror e and e + 1, lists tie in
ascending id.  `renumbered()` gives any of these inputs the numbering of a real graph (random vertex and edge ids, so inv[e] != e ^ 1);
`size_case(name)` puts the counts of the edit (kill vertices NK, new edges M, E + M) on block and sort-tile edges and has the edges of one
k-mer that real large-K graphs are full of; `all_deleted_case()` and `bad_inv_cases()` reach the driver's remaining paths."""
from dataclasses import dataclass, field

import numpy as np

import step4_cases as S
from w2rap_contigger_amd import formats as F
from step4_cases import Hand, _rc, _seq


@dataclass
class Case:
    inputs: tuple
    expect: dict = field(default_factory=dict)


def _chain(h, vs, ms):
    return [h.edge(vs[i], vs[i + 1], ms[i]) for i in range(len(vs) - 1)]


def _both(h, path):
    """a merged run's new edges in creation order: the mirror's first (popped first), then the run's own"""
    c = h.cat(path)
    return [_rc(c), c]


def edit_cases():
    out = {}

    # (a) four runs s -> k1 -> k2 -> t.  Smallest kill vertex: A < B < C < D; largest kill vertex: D < C < B < A; eleft: B < D < A < C.
    # The new ids follow the LARGEST kill vertex, ascending: D', D, C', C, B', B, A', A
    h = Hand(seed=31)
    first = {r: h.vertex() for r in "ABCD"}
    second = {r: h.vertex() for r in "DCBA"}
    ends = {r: (h.vertex(), h.vertex()) for r in "ABCD"}
    runs = {}
    for k, r in enumerate("BDAC"):
        runs[r] = _chain(h, [ends[r][0], first[r], second[r], ends[r][1]], [21 + 4 * k, 30 + k, 41 + 2 * k])
    h.read(runs["A"][1:], 5, 60); h.read(runs["C"], 9, 120, rc=True)
    out["a_interleaved_runs"] = Case(h.case() + (0,), {"merged": [8, 0], "edges": [s for r in "DCBA" for s in _both(h, runs[r])],
                                                        "by_smallest": [s for r in "ABCD" for s in _both(h, runs[r])],
                                                        "by_eleft": [s for r in "BDAC" for s in _both(h, runs[r])]})

    # (b) one run of 300 kill vertices (301 edges), lengths 39 .. 45 bases: no multiple of 4 in a row, packed bytes straddle
    h = Hand(seed=32)
    vs = [h.vertex() for _ in range(302)]
    es = _chain(h, vs, [1 + (i * 3) % 7 for i in range(301)])
    h.read(es[150:154], 4, 70); h.read(es[299:], 2, 40, rc=True); h.read(es[:3], 0, 50); h.read(es[64:67], 11, 50, rc=True)
    out["b_long_run"] = Case(h.case() + (0,), {"merged": [2, 0], "edges": _both(h, es), "run_size": 301})

    # (c) two runs between the same end vertices: both new edges are s -> t, creation order decides their place in From(s) and To(t).
    # The run through the smaller kill vertex is made from the edges created LAST
    h = Hand(seed=33)
    k_lo, k_hi, s, t = h.vertex(), h.vertex(), h.vertex(), h.vertex()
    hi = _chain(h, [s, k_hi, t], [25, 33]); lo = _chain(h, [s, k_lo, t], [37, 22])
    h.read(lo, 3, 60); h.read(hi[1:], 2, 40, rc=True)
    # k_lo < k_hi (and their mirrors likewise): lo', lo, hi', hi -> final ids 0..3; From(s) = [lo, hi], From(t') = [lo', hi']
    out["c_parallel_runs"] = Case(h.case() + (0,), {"merged": [4, 0], "edges": _both(h, lo) + _both(h, hi), "from_lists": [[0, 2], [1, 3]]})

    # (d) a new edge s -> t beside an old surviving edge s -> t: the old entry comes first
    h = Hand(seed=34)
    s, k, t = h.vertex(), h.vertex(), h.vertex()
    run = _chain(h, [s, k, t], [26, 31]); old = h.edge(s, t, 45)
    h.read(run, 6, 70)
    out["d_new_beside_old"] = Case(h.case() + (0,), {"merged": [2, 0], "edges": [h.b.edges[old][2], h.b.edges[old + 1][2]] + _both(h, run),
                                                      "from_lists": [[0, 3], [1, 2]]})

    # (e) circles made of kill vertices only; the mirror image of each is a different circle.  Circle 1: only the circle itself is pushed
    # (e = out-edge of its largest vertex < inv[e]; the mirror circle's e' > inv[e']).  Circle 2: the edge into its largest vertex was
    # created mirror first, so both the circle and its mirror circle are pushed: four copies
    h = Hand(seed=35)
    c = [h.vertex() for _ in range(3)]
    c1 = [h.edge(c[0], c[1], 50), h.edge(c[1], c[2], 61), h.edge(c[2], c[0], 43)]
    d = [h.vertex() for _ in range(3)]
    sq = np.concatenate([h.J[d[1]], _seq(h.rng, 35), h.J[d[2]]])
    h.b.edge(d[2] ^ 1, d[1] ^ 1, _rc(sq), mirror=False); h.b.edge(d[1], d[2], sq, mirror=False)
    d_in = len(h.b.edges) - 1
    c2 = [h.edge(d[2], d[0], 47), h.edge(d[0], d[1], 52)]
    h.read([c1[1], c1[2], c1[0]], 10, 150); h.read([c2[0], c2[1], d_in], 5, 130)
    out["e_circles"] = Case(h.case() + (0,), {"merged": [6, 0], "n_edges": 12})

    # (f) a run that is its own mirror image (u -> k -> k' -> u', the middle edge a palindrome): eleft == inv[eright], not merged
    h = Hand(seed=36)
    u, k = h.vertex(), h.vertex()
    e0 = h.edge(u, k, 33)
    half = _seq(h.rng, 17)
    pal = h.edge(k, k ^ 1, 0, seq=np.concatenate([h.J[k], half, _rc(half), h.J[k ^ 1]]))
    h.read([e0, pal, e0 ^ 1], 8, 100)
    out["f_self_mirror_run"] = Case(h.case() + (0,), {"merged": [0, 0], "n_edges": 3})

    # (g) min_size deletes the one-edge component on the FIRST vertices: every later vertex is renumbered, beside a run that merges
    h = Hand(seed=37)
    t0, t1 = h.vertex(), h.vertex()
    h.edge(t0, t1, 5)
    vs = [h.vertex() for _ in range(3)]
    run = _chain(h, vs, [100, 90])
    h.read(run, 10, 150)
    out["g_vertex_loses_all_edges"] = Case(h.case() + (40,), {"merged": [2, 0], "deleted0": 2, "edges": _both(h, run), "n_vertices": 4})

    # (h) pass 1 cannot vote at v (12 walks) but cuts the fan behind b down to one edge and merges it with b; pass 2 votes at v, deletes c
    # and merges a with the edge pass 1 made: ids and offsets of two passes compose (reads start on b and on the fan edge)
    h = Hand(seed=13); a, b, cc = S._branch(h, 8, 0, long_b=100, fan=6)
    w = h.b.edges[b][1]
    f0 = next(e for e, (x, _, _) in enumerate(h.b.edges) if x == w)
    for i in range(6):
        h.read([b, f0], 50 + 3 * i, 150, rc=bool(i & 1))
    h.read([f0], 20, 100); h.read([b, f0], 100, 90, rc=True)
    out["h_two_passes_compose"] = Case(h.case() + (0,), {"merged_each": True, "contains": h.cat([a, b, f0])})

    # (i) the lists of one vertex given out of order (a graph AddEdge did not build): the device edit declines, the host edit runs
    h = Hand(seed=38)
    x, y1, y2 = h.vertex(), h.vertex(), h.vertex()
    h.edge(x, y1, 30); h.edge(x, y2, 44)
    vs = [h.vertex() for _ in range(4)]
    run = _chain(h, vs, [27, 35, 29])
    h.read(run[1:], 4, 60)
    hb, paths, reads, quals = h.case()
    fo = int(hb.from_off[x])
    assert int(hb.from_off[x + 1]) - fo == 2 and hb.from_v[fo] < hb.from_v[fo + 1]
    hb.from_v[[fo, fo + 1]] = hb.from_v[[fo + 1, fo]]; hb.from_e[[fo, fo + 1]] = hb.from_e[[fo + 1, fo]]
    out["i_unsorted_lists"] = Case((hb, paths, reads, quals, 0), {"merged": [2, 0], "unsorted": True})
    return out


def empty_cases():
    """name -> (hbv, paths, (packed, byte_off, read_len), quals): a graph without an edge, with no vertex and with three isolated
    vertices, and two reads (30 and 45 bases) whose paths are empty"""
    rng = np.random.default_rng(39)
    ro = np.array([0, 30, 75], np.uint64)
    reads = F.pack_bases(_seq(rng, 75), ro)
    paths = (np.zeros(2, np.int32), np.zeros(3, np.uint64), np.zeros(0, np.int32))
    i32, u8 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    return {f"nv{nv}": (F.HBV(20, np.zeros(nv + 1, np.uint64), i32, i32, np.zeros(nv + 1, np.uint64), i32, u8, np.zeros(1, np.uint64), np.zeros(0, np.uint32)),
                        paths, reads, np.full(75, 30, np.uint8)) for nv in (0, 3)}


def no_reads_case():
    """-> (hbv, paths, (packed, byte_off, read_len), quals, min_size): the graph of b_long_run without a read"""
    h = edit_cases()["b_long_run"].inputs[0]
    return (h, (np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, np.int32)), F.pack_bases(np.zeros(0, np.uint8), np.zeros(1, np.uint64)), np.zeros(0, np.uint8), 0)


# ------------------------------------------------------------------------------------------------------------------- real numbering
def renumbered(inputs, seed, ties="asc"):
    """the same graph, reads and paths under a seeded random permutation of the vertex ids and of the edge ids: adjacency lists sorted
    by neighbour, equal neighbours in ascending (ties="asc") or descending ("desc") new edge id -- both are lists AddEdge can have built,
    and both meet the device edit's precondition.  Reads and qualities are untouched; inv is for the callee to derive (pass None)"""
    assert ties in ("asc", "desc")
    h, paths, reads, quals = inputs[:4]
    rng = np.random.default_rng(seed)
    nv, ne = h.n_vertices, h.n_edges
    pv, pe = rng.permutation(nv), rng.permutation(ne)          # old id -> new id
    tl, tr = h.to_left_right()
    assert ne == 0 or (tl.min() >= 0 and tr.min() >= 0)
    codes, off = h.edge_codes()
    off = off.astype(np.int64)
    old_of = np.argsort(pe)
    frm = [[] for _ in range(nv)]; to = [[] for _ in range(nv)]
    for e in range(ne):
        u, v, n = int(pv[tl[e]]), int(pv[tr[e]]), int(pe[e])
        frm[u].append((v, n)); to[v].append((u, n))
    sign = 1 if ties == "asc" else -1
    for l in frm + to:
        l.sort(key=lambda x: (x[0], sign * x[1]))
    fo = np.zeros(nv + 1, np.uint64); t_o = np.zeros(nv + 1, np.uint64)
    if nv:
        np.cumsum([len(x) for x in frm], out=fo[1:]); np.cumsum([len(x) for x in to], out=t_o[1:])
    noff = np.zeros(ne + 1, np.uint64)
    if ne:
        np.cumsum([off[e + 1] - off[e] for e in old_of], out=noff[1:])
    pk, bo, ln = F.pack_bases(np.concatenate([codes[off[e]:off[e + 1]] for e in old_of]) if ne else np.zeros(0, np.uint8), noff)
    hb = F.HBV(h.K, fo, np.array([v for l in frm for v, _ in l], np.int32), np.array([e for l in frm for _, e in l], np.int32),
               t_o, np.array([e for l in to for _, e in l], np.int32), pk, bo, ln)
    pth = (np.array(paths[0], np.int32), np.array(paths[1], np.uint64), pe[np.asarray(paths[2], np.int64)].astype(np.int32))
    return (hb, pth, reads, quals) + tuple(inputs[4:])


RENUMBER = [(101, "asc"), (101, "desc"), (202, "asc"), (202, "desc")]          # two seeds x both tie orders
RANDOM_SEEDS = list(range(0, 24, 2))                                            # of step4_vote_cases.random_case
_VARIANTS, _SOURCES = {}, {}
_HAND = sorted(["circle", "contested_branch_kept", "dead_end_lowers_depth", "edge_twice", "eleven_walks_skipped", "no_branches_min_size", "no_reads",
                "offset_moves_in_run", "palindrome_next_to_run", "pass2_exposes", "reverse_strand_only", "ten_walks_voted", "weak_branch"])
_EDIT = ["a_interleaved_runs", "b_long_run", "c_parallel_runs", "d_new_beside_old", "e_circles", "f_self_mirror_run", "g_vertex_loses_all_edges", "h_two_passes_compose"]


def variant_names():
    """the renumbered inputs the GPU tests run, as names only (nothing is built): every edit_cases() entry but i_unsorted_lists (renumbering
    sorts its lists), every step4_cases.hand_cases() entry and the hub of the size cases, each under RENUMBER; random_case(seed) for
    RANDOM_SEEDS, each under one numbering"""
    out = [f"{k}-{seed}-{ties}" for k in _EDIT + [f"hand_{k}" for k in _HAND] + ["hub"] for seed, ties in RENUMBER]
    return out + [f"random_{seed}-{300 + seed}-{'desc' if seed & 2 else 'asc'}" for seed in RANDOM_SEEDS]


def _source(k):
    if not _SOURCES:
        _SOURCES["edit"] = edit_cases(); _SOURCES["hand"] = S.hand_cases()
        assert sorted(_SOURCES["hand"]) == _HAND and sorted(set(_SOURCES["edit"]) - {"i_unsorted_lists"}) == _EDIT
    if k not in _SOURCES:
        if k.startswith("random_"):
            import step4_vote_cases as V
            _SOURCES[k] = V.random_case(int(k[7:])).case() + (0,)
        elif k.startswith("hand_"):
            _SOURCES[k] = _SOURCES["hand"][k[5:]]
        else:
            _SOURCES[k] = size_case("hub").inputs if k == "hub" else _SOURCES["edit"][k].inputs
    return _SOURCES[k]


def renumbered_variant(name):
    """-> (hbv, paths, reads, quals, min_size) of one of variant_names(), built on first use"""
    if name not in _VARIANTS:
        k, seed, ties = name.rsplit("-", 2)
        _VARIANTS[name] = renumbered(_source(k), int(seed), ties)
    return _VARIANTS[name]


# ---------------------------------------------------------------------------------------------------------------- sizes and short edges
def _cut(h, kmers):
    """one random sequence cut into consecutive edges of kmers[i] k-mers each (K - 1 + kmers[i] bases, real overlaps) over new vertices
    -> (vertices, edge ids)"""
    K = h.K
    s = _seq(h.rng, sum(kmers) + K - 1)
    at = np.concatenate([[0], np.cumsum(kmers)])
    vs = []
    for p in at:
        v = h.b.vertex(); h.J[v] = s[p:p + K - 1]; h.J[v ^ 1] = _rc(h.J[v]); vs.append(v)
    return vs, [h.b.edge(vs[i], vs[i + 1], s[at[i]:at[i + 1] + K - 1]) for i in range(len(kmers))]


MIXED = [1, 1, 2, 1, 3, 4, 1, 5]


def one_kmer_members(K=20, n=70, members=(1, 2, 37, 70)):
    """a run of n edges of ONE k-mer each (K bases: in k4e_gather the four bases of an output byte come from four members, offsets[e]
    advances by one a member) and a run of MIXED k-mers; reads that start on the given members of the first run (1-based) on both
    strands, each covering the run to its end so that it starts at offset 0 of its first edge on either strand"""
    h = Hand(K=K, seed=40 + K)
    _, es = _cut(h, [1] * n)
    _, mx = _cut(h, MIXED)
    whole = lambda path: len(h.cat(path))
    for m in members:
        h.read(es[m - 1:], 0, whole(es[m - 1:]))                          # starts on member m
        h.read(es[:n - m + 1], 0, whole(es[:n - m + 1]), rc=True)         # starts on member m of the mirror run
    h.read(mx[1:], 0, whole(mx[1:])); h.read(mx[3:6], 1, K + 4); h.read(mx[:5], 0, whole(mx[:5]), rc=True)
    return Case(h.case() + (0,), {"merged": [4, 0], "run_size": n, "min_kmers": 1, "edges": _both(h, es) + _both(h, mx)})


def runs_p(P):
    """P separate runs s -> k -> t, inner lengths 1 .. 7 cycling: M = 2 P new edges"""
    h = Hand(seed=50)
    runs = []
    for i in range(P):
        s, k, t = h.vertex(), h.vertex(), h.vertex()
        runs.append(_chain(h, [s, k, t], [1 + i % 7, 1 + (i + 3) % 7]))
    for i in (0, P // 2, P - 1):
        h.read(runs[i][1:], 2, 30, rc=bool(i & 1)); h.read(runs[i], 1, 45)
    return Case(h.case() + (0,), {"merged": [2 * P, 0], "n_edges": 2 * P})


def parallel_runs(P=1025):
    """P runs between the same s and t: every new edge of From(s) ties on the neighbour, over more than one sort tile of 2048 pairs"""
    h = Hand(seed=51)
    s, t = h.vertex(), h.vertex()
    runs = []
    for i in range(P):
        runs.append(_chain(h, [s, h.vertex(), t], [1 + i % 5, 2 + i % 3]))
    for i in (0, 1, P - 1):
        h.read(runs[i], 3, 40, rc=bool(i & 1))
    # run i is the i-th by kill vertex: its mirror becomes edge 2 i, the run itself 2 i + 1
    return Case(h.case() + (0,), {"merged": [2 * P, 0], "n_edges": 2 * P, "from_s": [2 * i + 1 for i in range(P)], "to_s_mirror": [2 * i for i in range(P)]})


def run_len(L):
    """one run of L kill vertices alone in the graph (NK = 2 L); a read starts on its last member"""
    h = Hand(seed=52)
    vs = [h.vertex() for _ in range(L + 2)]
    es = _chain(h, vs, [1 + (5 * i) % 7 for i in range(L + 1)])
    h.read(es[-1:], 1, 25); h.read(es[-1:], 0, 30, rc=True); h.read(es[:2], 4, 40)
    return Case(h.case() + (0,), {"merged": [2, 0], "n_edges": 2, "run_size": L + 1, "edges": _both(h, es)})


def circle_len(L):
    """a circle of L one-in one-out vertices (L = 2: neither is a kill vertex, from(v) == to(v)) beside one run that merges"""
    h = Hand(seed=53)
    c = [h.vertex() for _ in range(L)]
    ce = [h.edge(c[i], c[(i + 1) % L], 20 + 3 * i) for i in range(L)]
    vs = [h.vertex() for _ in range(3)]
    run = _chain(h, vs, [30, 41])
    h.read(ce + ce[:1], 5, 60); h.read(ce[1:] + ce[:1], 2, 50, rc=True); h.read(run, 7, 60)
    return Case(h.case() + (0,), {"n_edges": 2 * L + 2})


HUB_N = 40


def hub():
    """x has HUB_N out-neighbours in ascending id; neighbour i has, by i % 4: an old edge that survives / a run / an old edge and two runs /
    three old parallel edges and a run.  From(x) of the result interleaves old and new entries all along; To(x') likewise.
    The survivors keep their order (final ids 0 .. n_old - 1, an edge and then its mirror); run j by kill vertex becomes n_old + 2 j + 1, its
    mirror n_old + 2 j"""
    h = Hand(seed=54)
    x = h.vertex()
    ws = [h.vertex() for _ in range(HUB_N)]
    plan = [(1, 0), (0, 1), (1, 2), (3, 1)]                     # (old edges, runs) by i % 4
    n_old = 2 * sum(plan[i % 4][0] for i in range(HUB_N))
    frm, to, old_at, runs = [], [], 0, 0
    for i, w in enumerate(ws):                                  # the old edges first: ids 0 .. n_old - 1, all of which survive
        for j in range(plan[i % 4][0]):
            h.edge(x, w, 10 + (i + j) % 9)
    for i, w in enumerate(ws):
        n_o, n_r = plan[i % 4]
        frm += [old_at + 2 * j for j in range(n_o)]; to += [old_at + 2 * j + 1 for j in range(n_o)]
        old_at += 2 * n_o
        for _ in range(n_r):
            r = _chain(h, [x, h.vertex(), w], [3 + runs % 6, 8 + runs % 5])
            if runs % 7 == 0:
                h.read(r, 2, 40, rc=bool(runs & 1))
            frm.append(n_old + 2 * runs + 1); to.append(n_old + 2 * runs)
            runs += 1
    return Case(h.case() + (0,), {"merged": [2 * runs, 0], "n_edges": n_old + 2 * runs, "hub_from": frm, "hub_to": to})


RUNS_P = (127, 128, 129, 1023, 1024, 1025)
RUN_LEN = (1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257)
CIRCLE_LEN = (2, 3, 4, 5, 8, 9)
_SIZE = {}
_SIZE_MAKERS = {"one_kmer_members": one_kmer_members, "one_kmer_members_K200": lambda: one_kmer_members(K=200, n=12, members=(1, 2, 7, 12)),
                "parallel_1025": parallel_runs, "hub": hub}
_SIZE_MAKERS.update({f"runs_{P}": (lambda P=P: runs_p(P)) for P in RUNS_P})
_SIZE_MAKERS.update({f"run_len_{L}": (lambda L=L: run_len(L)) for L in RUN_LEN})
_SIZE_MAKERS.update({f"circle_{L}": (lambda L=L: circle_len(L)) for L in CIRCLE_LEN})


def size_names():
    return sorted(_SIZE_MAKERS)


def size_case(name):
    """-> Case, built on first use"""
    if name not in _SIZE:
        _SIZE[name] = _SIZE_MAKERS[name]()
    return _SIZE[name]


# ---------------------------------------------------------------------------------------------------------------- the driver's other paths
def all_deleted_case():
    """-> (hbv, paths, reads, quals, min_size): three isolated edges of 24 .. 26 k-mers and min_size 40: pass 1 deletes every edge, pass 2
    starts on a graph without one"""
    h = Hand(seed=55)
    es = [h.edge(h.vertex(), h.vertex(), 5 + i) for i in range(3)]
    h.read(es[:1], 3, 30); h.read(es[2:], 0, 35, rc=True)
    return h.case() + (40,)


def bad_inv_cases():
    """name -> (hbv, paths, reads, quals, inv): an inv that w2rap_step4_run accepts (an involution of edges of equal length) but that
    does not mirror runs onto runs.  No vertex branches, so nothing but the edit reads inv.
    self: a run's right edge and that edge's mirror are each their own partner.  swap: two runs of equal edge lengths with the mirror
    partners of their right edges swapped.  circle: a run's right edge is paired with an edge of a circle of kill vertices, so the walk
    along the 'mirror run' goes round the circle and never meets its end"""
    out = {}
    h = Hand(seed=56)
    r = _chain(h, [h.vertex() for _ in range(4)], [30, 31, 32])
    h.read(r, 3, 60)
    inv = np.arange(len(h.b.edges), dtype=np.int32) ^ 1
    inv[r[2]] = r[2]; inv[r[2] + 1] = r[2] + 1
    out["self"] = h.case() + (inv,)
    h = Hand(seed=57)
    a = _chain(h, [h.vertex() for _ in range(3)], [30, 33]); b = _chain(h, [h.vertex() for _ in range(3)], [30, 33])
    h.read(a, 3, 60); h.read(b, 5, 50, rc=True)
    inv = np.arange(len(h.b.edges), dtype=np.int32) ^ 1
    inv[[a[1], b[1] + 1]] = [b[1] + 1, a[1]]; inv[[b[1], a[1] + 1]] = [a[1] + 1, b[1]]
    out["swap"] = h.case() + (inv,)
    h = Hand(seed=58)
    a = _chain(h, [h.vertex() for _ in range(3)], [30, 33])
    c = [h.vertex() for _ in range(3)]
    ce = [h.edge(c[i], c[(i + 1) % 3], 33) for i in range(3)]
    h.read(a, 3, 60); h.read(ce, 5, 70)
    inv = np.arange(len(h.b.edges), dtype=np.int32) ^ 1
    inv[[a[1], ce[0]]] = [ce[0], a[1]]; inv[[a[1] + 1, ce[0] + 1]] = [ce[0] + 1, a[1] + 1]
    out["circle"] = h.case() + (inv,)
    return out

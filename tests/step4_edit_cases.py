"""Hand-made graphs for the graph edit of Step 4 (delete, merge runs, renumber), at K = 20, built with step4_cases.Hand / Builder.
Each is the smallest graph that exercises one rule of RemoveUnneededVertices2 / CleanupCore as the two stacks of the reference define
it; `edit_cases()` also returns, per case, what test_step4_edit_model.py asserts about the model's output so that a green test means
the rule was really exercised.

    edit_cases() -> name -> Case(inputs = (hbv, paths, (packed, byte_off, read_len), quals, min_size), expect = {...})

`empty_cases()` and `no_reads_case()` are the shapes at which the driver around the edit, not the edit, can go wrong: a graph without an
edge (nothing to run a kernel on: the device edit declines) and a graph that changes while there is no read path to rewrite."""
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

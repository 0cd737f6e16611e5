"""A small CPU restatement of the reference's Step 4, Clean200x (src/paths/long/large/Clean200.cc:202-389 with Cleanup,
GapToyTools.cc:417-472, and RemoveUnneededVertices2, GapToyTools3.cc:87-294): plain Python lists and numpy, written to be read next
to the reference, one statement for one statement where the order of things decides a number.  test_step4_model.py pins it to
recorded runs of the reference byte for byte; test_gpu_step4.py then uses it to judge the HIP library on inputs the reference was
never run on.

    clean200x(hbv, inv, paths, reads, min_size=0, vote=True) -> Model4Result
    one_pass(g, inv, offs, paths, reads, min_size, vote, counters) -> sorted unique deleted edge ids (graph, inv, paths edited in place)

`vote=False` disables the weak-branch vote: what is left is min_size, Cleanup and the renumbering."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

from w2rap_contigger_amd import formats as F

MAX_EXTS = 10
MAX_RL = 250
MAX_DEL, MIN_WIN, MAX_LOSE, MIN_RATIO = 15, 100, 50, 5
RUN_SIZES = []          # edges per merged run of the runs made so far (read by the tests that assert what the fixtures exercise)
RUNS = []               # per call of remove_unneeded_vertices2 (one a pass) the list of its pushed runs, in the order they were found
# a pushed run: its ends, its kill vertices from eleft to eright, and those of its mirror image (inv[eright], inv[eleft]) where the same
# pass found that as a run of its own (None: a circle whose mirror edge lies on the same circle, or an inv that mirrors no run onto it)
Run = namedtuple("Run", "eleft eright kill mirror_kill")
PLACEMENTS = None       # a list: vote() appends (vertex, walks, depth, placements) per voted branch vertex, in the order of the flat placement list


class Graph:
    """digraphE<basevector>: per vertex the ordered lists from_, from_edge_obj_, to_, to_edge_obj_; edge objects as base-code arrays"""

    def __init__(self, K, frm, frm_e, to, to_e, edges):
        self.K, self.frm, self.frm_e, self.to, self.to_e, self.edges = K, frm, frm_e, to, to_e, edges

    @staticmethod
    def from_hbv(h: F.HBV) -> "Graph":
        codes, off = h.edge_codes()
        off = off.astype(np.int64)
        edges = [codes[off[e]:off[e + 1]].copy() for e in range(h.n_edges)]
        fo = np.asarray(h.from_off, np.int64); to = np.asarray(h.to_off, np.int64)
        nv = h.n_vertices
        frm = [[int(x) for x in h.from_v[fo[v]:fo[v + 1]]] for v in range(nv)]
        frm_e = [[int(x) for x in h.from_e[fo[v]:fo[v + 1]]] for v in range(nv)]
        to_e = [[int(x) for x in h.to_e[to[v]:to[v + 1]]] for v in range(nv)]
        left = {}
        for v in range(nv):
            for e in frm_e[v]:
                left[e] = v
        tov = [[left[e] for e in to_e[v]] for v in range(nv)]
        return Graph(int(h.K), frm, frm_e, tov, to_e, edges)

    def to_hbv(self) -> F.HBV:
        nv = len(self.frm)
        fo = np.zeros(nv + 1, np.uint64); to = np.zeros(nv + 1, np.uint64)
        np.cumsum([len(x) for x in self.frm], out=fo[1:]) if nv else None
        np.cumsum([len(x) for x in self.to_e], out=to[1:]) if nv else None
        flat = lambda ll: np.array([x for l in ll for x in l], dtype=np.int32)
        off = np.zeros(len(self.edges) + 1, np.uint64)
        if self.edges:
            np.cumsum([len(x) for x in self.edges], out=off[1:])
        codes = np.concatenate(self.edges).astype(np.uint8) if self.edges else np.zeros(0, np.uint8)
        pk, bo, ln = F.pack_bases(codes, off)
        return F.HBV(self.K, fo, flat(self.frm), flat(self.frm_e), to, flat(self.to_e), pk, bo, ln)

    def n_edge_objs(self):
        return len(self.edges)

    def kmers(self, e):
        return len(self.edges[e]) - self.K + 1

    def to_left_right(self):
        tl = [-1] * len(self.edges); tr = [-1] * len(self.edges)
        for v in range(len(self.frm)):
            for e in self.frm_e[v]:
                tl[e] = v
            for e in self.to_e[v]:
                tr[e] = v
        return tl, tr

    def used(self):
        u = [False] * len(self.edges)
        for l in self.to_e:
            for e in l:
                u[e] = True
        return u

    def add_edge(self, v, w, seq):                     # DigraphTemplate.h:1829-1839
        import bisect
        n = len(self.edges)
        self.edges.append(seq)
        i = bisect.bisect_right(self.frm[v], w)
        self.frm[v].insert(i, w); self.frm_e[v].insert(i, n)
        j = bisect.bisect_right(self.to[w], v)
        self.to[w].insert(j, v); self.to_e[w].insert(j, n)
        return n

    def delete_edges(self, dead):                      # DigraphTemplate.h:2017-2027: the lists keep their order
        dead = set(dead)
        for v in range(len(self.frm)):
            if any(e in dead for e in self.frm_e[v]):
                keep = [k for k, e in enumerate(self.frm_e[v]) if e not in dead]
                self.frm[v] = [self.frm[v][k] for k in keep]; self.frm_e[v] = [self.frm_e[v][k] for k in keep]
            if any(e in dead for e in self.to_e[v]):
                keep = [k for k, e in enumerate(self.to_e[v]) if e not in dead]
                self.to[v] = [self.to[v][k] for k in keep]; self.to_e[v] = [self.to_e[v][k] for k in keep]


def involution(g: Graph):
    """HyperBasevector::Involution (HyperBasevector.cc:648-660): rank in sequence order matched with rank in reverse-complement order"""
    seqs = [bytes(x) for x in g.edges]
    rcs = [bytes((3 - x[::-1]).astype(np.uint8)) for x in g.edges]
    x1 = sorted(range(len(seqs)), key=lambda i: seqs[i])
    x2 = sorted(range(len(seqs)), key=lambda i: rcs[i])
    inv = [0] * len(seqs)
    for a, b in zip(x1, x2):
        inv[a] = b
    return inv


@dataclass
class Reads:
    codes: np.ndarray      # u8 base codes, concatenated
    quals: np.ndarray      # u8 raw qualities, same offsets
    off: np.ndarray        # i64[n+1]


@dataclass
class Counters:
    n_branch_vertices: int = 0
    n_skipped_too_many_exts: int = 0
    n_placements: int = 0
    n_deleted: list = field(default_factory=list)
    n_runs_merged: list = field(default_factory=list)


def get_extensions(g: Graph, to_right, v, depth):       # Clean200.cc:445-470
    exts = []
    for _ in range(2):
        exts = [[e] for e in g.frm_e[v]]
        i = 0
        while i < len(exts):
            if i >= MAX_EXTS:
                break
            ln = sum(g.kmers(e) for e in exts[i])
            if ln >= depth:
                i += 1
                continue
            w = to_right[exts[i][-1]]
            if not g.frm[w]:
                depth = min(depth, ln)
                i += 1
                continue
            p = exts[i]
            for m, e in enumerate(g.frm_e[w]):
                if m == 0:
                    exts[i] = p + [e]
                else:
                    exts.append(p + [e])
    return exts, depth


def cat(g: Graph, x):
    out = [g.edges[x[0]]]
    for e in x[1:]:
        out.append(g.edges[e][g.K - 1:])
    return np.concatenate(out)


def analyze_scores(g, inv, v, scores, to_delete):       # Clean200.cc:391-443, version 3
    n = len(g.frm[v])
    for d in range(MAX_DEL + 1):
        qsum = [sum(s for s in scores[j] if s > d) for j in range(n)]
        ids = sorted(range(n), key=lambda j: -qsum[j])
        qs = [qsum[j] for j in ids]
        for r in range(1, n):
            if qs[0] >= MIN_WIN and qs[r] <= MAX_LOSE and qs[0] >= MIN_RATIO * qs[r]:
                for j in range(r, n):
                    e2 = g.frm_e[v][ids[j]]
                    to_delete += [e2, inv[e2]]
                return


def vote(g: Graph, inv, offs, paths, reads: Reads, cnt: Counters):
    K = g.K
    tl, to_right = g.to_left_right()
    paths_index = {}
    for rid, p in enumerate(paths):                     # invert(): one listing per occurrence
        for e in p:
            paths_index.setdefault(e, []).append(rid)
    to_delete = []
    roff = reads.off
    for v in range(len(g.frm)):
        if not g.to[v] or len(g.frm[v]) <= 1:
            continue
        cnt.n_branch_vertices += 1
        n = len(g.frm[v])
        exts, depth = get_extensions(g, to_right, v, MAX_RL)
        if len(exts) > MAX_EXTS:
            cnt.n_skipped_too_many_exts += 1
            continue
        N = len(exts)
        ei = [g.frm_e[v].index(x[0]) for x in exts]
        L = depth + K - 1
        bexts = np.stack([cat(g, x)[:L] for x in exts])             # [N, L]
        scores = [[] for _ in range(n)]
        ins = g.to_e[v]
        pi = []
        for e in ins:
            for rid in paths_index.get(e, ()):
                p = paths[rid]
                for j in range(len(p)):
                    if p[j] == e:
                        pi.append((rid, offs[rid] - sum(g.kmers(x) for x in p[:j + 1])))
        for ep in g.frm_e[v]:
            for rid in paths_index.get(ep, ()):
                p = paths[rid]
                for j in range(len(p)):
                    if p[j] == ep:
                        if j > 0 and p[j - 1] in ins:
                            continue
                        pi.append((rid, offs[rid] - sum(g.kmers(x) for x in p[:j])))
        rpi = []
        res = [inv[e] for e in ins]
        for re in res:
            for rid in paths_index.get(re, ()):
                p = paths[rid]
                for j in range(len(p)):
                    if p[j] == re:
                        rpi.append((rid, offs[rid] - sum(g.kmers(x) for x in p[:j])))
        for ep in g.frm_e[v]:
            rep = inv[ep]
            for rid in paths_index.get(rep, ()):
                p = paths[rid]
                for j in range(len(p)):
                    if p[j] == rep:
                        if j < len(p) - 1 and p[j + 1] in res:
                            continue
                        rpi.append((rid, offs[rid] - sum(g.kmers(x) for x in p[:j + 1])))
        cnt.n_placements += len(pi) + len(rpi)
        if PLACEMENTS is not None:
            PLACEMENTS.append((v, N, depth, len(pi) + len(rpi)))
        for fw, lst in ((True, pi), (False, rpi)):
            for rid, start in lst:
                b = reads.codes[roff[rid]:roff[rid + 1]]
                qv = reads.quals[roff[rid]:roff[rid + 1]].astype(np.int64)
                pos = np.arange(L)
                rpos = pos - start if fw else K - 2 - pos - start
                ok = (rpos >= 0) & (rpos < len(b))
                pos, rpos = pos[ok], rpos[ok]
                if fw:
                    mism = bexts[:, pos] != b[rpos][None, :]
                else:
                    mism = (3 - bexts[:, pos]) != b[rpos][None, :]
                q = (mism * qv[rpos][None, :]).sum(axis=1)
                qq = [1000000000] * n
                for l in range(N):
                    qq[ei[l]] = min(qq[ei[l]], int(q[l]))
                idx = sorted(range(n), key=lambda j: qq[j])
                if qq[idx[0]] < qq[idx[1]]:
                    scores[idx[0]].append(qq[idx[1]] - qq[idx[0]])
        analyze_scores(g, inv, v, scores, to_delete)
    return to_delete


def tiny_components(g: Graph, min_size):                # Clean200.cc:370-380
    out = []
    for v in range(len(g.frm)):
        if g.to[v] or len(g.frm[v]) != 1:
            continue
        w = g.frm[v][0]
        if v == w or len(g.to[w]) != 1 or g.frm[w]:
            continue
        e = g.frm_e[v][0]
        if g.kmers(e) > min_size:
            continue
        out.append(e)
    return out


def remove_unneeded_vertices2(g: Graph, inv, offs, paths):          # GapToyTools3.cc:87-294; -> number of new edges
    nv = len(g.frm)
    to_left, to_right = g.to_left_right()
    kill = [False] * nv
    queue = []
    for v in range(nv):
        if len(g.frm[v]) == 1 and len(g.to[v]) == 1 and g.frm[v][0] != g.to[v][0] \
                and len(g.edges[g.frm_e[v][0]]) > 0 and len(g.edges[g.to_e[v][0]]) > 0:
            kill[v] = True
            queue.append(v)
    bound = []
    found, pushed = {}, []                             # (recording only: RUNS)
    while queue:
        v = queue.pop()
        if not kill[v]:
            continue
        vleft = v
        seen_left, seen_right = [], []
        while True:
            kill[vleft] = False
            seen_left.append(vleft)
            eleft = g.to_e[vleft][0]
            vleft = g.to[vleft][0]
            if not kill[vleft]:
                break
        vright = v
        while True:
            kill[vright] = False
            seen_right.append(vright)
            eright = g.frm_e[vright][0]
            vright = g.frm[vright][0]
            if not kill[vright]:
                break
        found[(eleft, eright)] = tuple(seen_left[::-1] + seen_right[1:])
        if eleft < inv[eright]:
            bound.append((eleft, eright))
            bound.append((inv[eright], inv[eleft]))
            pushed.append((eleft, eright))
    RUNS.append([Run(a, b, found[(a, b)], found.get((inv[b], inv[a]))) for a, b in pushed])
    E0 = len(g.edges)
    renum = list(range(E0))
    offsets = [0] * E0
    new_nos = []
    dead = []
    while bound:
        first, second = bound.pop()
        new_no = len(g.edges)
        off = g.kmers(first)
        renum[first] = new_no
        dead.append(first)
        seq = [g.edges[first]]
        v = to_right[first]
        while v != to_right[second]:
            e = g.frm_e[v][0]
            dead.append(e)
            offsets[e] = off
            renum[e] = new_no
            off += g.kmers(e)
            v = g.frm[v][0]
        new_edge = g.edges[first]
        v = to_right[first]
        while v != to_right[second]:
            e = g.frm_e[v][0]
            new_edge = np.concatenate([new_edge[:offsets[e]], g.edges[e]])
            v = g.frm[v][0]
        g.add_edge(to_left[first], to_right[second], new_edge)
        RUN_SIZES.append(sum(1 for x in renum if x == new_no))
        new_nos.append(new_no)
    g.delete_edges(dead)
    inv += [-1] * (len(g.edges) - len(inv))
    for k in range(0, len(new_nos), 2):
        inv[new_nos[k]] = new_nos[k + 1]
        inv[new_nos[k + 1]] = new_nos[k]
    for i, old in enumerate(paths):
        if old:
            offs[i] += offsets[old[0]]
            p = [renum[old[0]]]
            for e in old[1:]:
                if renum[e] != p[-1]:
                    p.append(renum[e])
            paths[i] = p
    return len(new_nos)


def cleanup_core(g: Graph, inv, paths):                 # GapToyTools.cc:417-453
    used = g.used()
    to_new, c = [-1] * len(used), 0
    for i, u in enumerate(used):
        if u:
            to_new[i] = c
            c += 1
    inv[:] = [(-1 if inv[i] < 0 else to_new[inv[i]]) for i in range(len(used)) if used[i]]
    for p in paths:
        for j in range(len(p)):
            if to_new[p[j]] >= 0:
                p[j] = to_new[p[j]]
    g.edges = [g.edges[i] for i in range(len(used)) if used[i]]                 # RemoveDeadEdgeObjects
    g.frm_e = [[to_new[e] for e in l] for l in g.frm_e]
    g.to_e = [[to_new[e] for e in l] for l in g.to_e]
    keep = [v for v in range(len(g.frm)) if g.frm[v] or g.to[v]]               # RemoveEdgelessVertices
    newv = {v: k for k, v in enumerate(keep)}
    g.frm = [[newv[w] for w in g.frm[v]] for v in keep]; g.to = [[newv[w] for w in g.to[v]] for v in keep]
    g.frm_e = [g.frm_e[v] for v in keep]; g.to_e = [g.to_e[v] for v in keep]


def cleanup(g: Graph, inv, offs, paths):                # GapToyTools.cc:455-472; -> runs merged
    used = g.used()
    for i, p in enumerate(paths):
        for j, e in enumerate(p):
            if e < 0 or e >= len(used) or not used[e]:
                paths[i] = p[:j]
                break
    merged = remove_unneeded_vertices2(g, inv, offs, paths)
    cleanup_core(g, inv, paths)
    return merged


def one_pass(g: Graph, inv, offs, paths, reads: Reads, min_size, do_vote, cnt: Counters, edit=True):
    to_delete = vote(g, inv, offs, paths, reads, cnt) if do_vote else []
    if min_size > 0:
        to_delete += tiny_components(g, min_size)
    dead = sorted(set(to_delete))
    cnt.n_deleted.append(len(dead))
    if edit:
        g.delete_edges(dead)
        cnt.n_runs_merged.append(cleanup(g, inv, offs, paths))
    return dead


@dataclass
class Model4Result:
    hbv: F.HBV
    inv: np.ndarray
    path_offset: np.ndarray
    path_off: np.ndarray
    path_edges: np.ndarray
    deleted: list            # per pass: sorted unique edge ids of that pass's input graph
    counters: Counters


def reads_of(packed, byte_off, read_len, quals):
    codes, off = F.unpack_bases(packed, byte_off, read_len)
    return Reads(codes, np.asarray(quals, np.uint8), off.astype(np.int64))


def clean200x(hbv: F.HBV, inv, paths, reads: Reads, min_size=0, vote=True, vote_only=False) -> Model4Result:
    """paths = (offset i32[n], path_off u64[n+1], edges i32[]); inv None = the graph's involution"""
    g = Graph.from_hbv(hbv)
    inv = involution(g) if inv is None else [int(x) for x in inv]
    po = np.asarray(paths[1], np.int64)
    offs = [int(x) for x in paths[0]]
    pl = [[int(e) for e in paths[2][po[i]:po[i + 1]]] for i in range(len(offs))]
    cnt = Counters()
    deleted = []
    for _ in range(1 if vote_only else 2):
        deleted.append(one_pass(g, inv, offs, pl, reads, min_size, vote, cnt, edit=not vote_only))
    npo = np.zeros(len(pl) + 1, np.uint64)
    if pl:
        np.cumsum([len(p) for p in pl], out=npo[1:])
    return Model4Result(g.to_hbv(), np.array(inv, np.int32), np.array(offs, np.int32), npo,
                        np.array([e for p in pl for e in p], np.int32), deleted, cnt)

"""Inputs of the Step-4 tests: the recorded runs of the reference's Step 4 (tests/golden/refruns/step4_<case>/) and hand-made graphs.

A recorded case is the reference's own main run with ``--from_step 4 --to_step 4 -s <min_size>`` on a directory holding
frag_reads_orig.fastb/.qualp and t.large_K.hbv/.paths; its t.large_K.clean.hbv/.paths are the expected output.
`step4_errs2` is the fixture made for the vote: 2,400 read pairs (1 % errors) of a 12 kb two-haplotype genome with repeats
(synth.diploid_genome(12000, 31, snp_every=400), synth.sample_reads(.., 2400, 32, err_rate=0.01)), the reference's Steps 2 and 3 run
with min_freq 2 so that error branches reach the large-K graph."""
import os
import shutil
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT, reference_outputs
from w2rap_contigger_amd import formats as F

# fixture -> (graph files' stem, reads files' stem, a min_size that deletes something)
FIXTURES = {
    "random20k": ("random20k.ref", "random20k", 300),
    "repeats_snps": ("repeats_snps.ref", "repeats_snps", 300),
    "palindrome_circle": ("palindrome_circle.ref", "palindrome_circle", 1000),
    "long_mixed": ("long_mixed.ref", "long_mixed", 300),
    "errs2": ("step4_errs2", "step4_errs2", 300),
}
CASES = [(name, ms) for name, v in FIXTURES.items() for ms in (0, v[2])]
INPUTS = ["frag_reads_orig.fastb", "frag_reads_orig.qualp", "t.large_K.hbv", "t.large_K.paths"]
OUTPUTS = ["t.large_K.clean.hbv", "t.large_K.clean.paths"]


def stage(name, workdir):
    g, r, _ = FIXTURES[name]
    for src, dst in ((f"{g}.large_K.hbv", "t.large_K.hbv"), (f"{g}.large_K.paths", "t.large_K.paths"), (f"{r}.fastb", "frag_reads_orig.fastb"), (f"{r}.qualp", "frag_reads_orig.qualp")):
        shutil.copy(os.path.join(GOLDEN, src), os.path.join(workdir, dst))


def reference_run(name, min_size, workdir):
    """stages the inputs in workdir and puts the reference's recorded outputs beside them"""
    stage(name, workdir)

    def run():
        exe = os.path.join(ROOT, "oracle", "_ref", "w2rap-contigger-gpu")
        return subprocess.run([exe, "-r", "x", "-o", workdir, "-p", "t", "-t", "8", "-m", "16", "--from_step", "4", "--to_step", "4", "-s", str(min_size)],
                              check=True, capture_output=True, text=True).stdout and None
    reference_outputs(f"step4_{name}_s{min_size}", workdir, INPUTS, OUTPUTS, run)


_LOADED = {}


def load(name):
    """-> (hbv, paths, (packed, byte_off, read_len), quals) of a fixture"""
    if name not in _LOADED:
        g, r, _ = FIXTURES[name]
        pq, po = F.read_qualp(os.path.join(GOLDEN, f"{r}.qualp"))
        _LOADED[name] = (F.read_hbv(os.path.join(GOLDEN, f"{g}.large_K.hbv")), F.read_paths(os.path.join(GOLDEN, f"{g}.large_K.paths")),
                         F.read_fastb(os.path.join(GOLDEN, f"{r}.fastb")), F.qualp_to_raw(pq, po)[0])
    return _LOADED[name]


# ---------------------------------------------------------------------------------------------------------------- hand-made graphs
def _seq(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _rc(s):
    return (3 - s[::-1]).astype(np.uint8)


class Builder:
    """a graph from named vertices and edge sequences, with the mirror image (reverse complement) of everything added, as a
    HyperBasevector built by AddEdge would hold it: adjacency lists sorted by vertex, ties in insertion order"""

    def __init__(self, K):
        self.K, self.edges, self.nv = K, [], 0

    def vertex(self):
        self.nv += 2
        return self.nv - 2                 # v and its mirror v + 1 (an edge u -> v has the mirror v + 1 -> u + 1)

    def edge(self, u, v, seq, mirror=True):
        self.edges.append((u, v, np.asarray(seq, np.uint8)))
        if mirror:
            self.edges.append((v ^ 1, u ^ 1, _rc(np.asarray(seq, np.uint8))))
        return len(self.edges) - (2 if mirror else 1)

    def hbv(self):
        frm = [[] for _ in range(self.nv)]; to = [[] for _ in range(self.nv)]
        for e, (u, v, _) in enumerate(self.edges):
            frm[u].append((v, e)); to[v].append((u, e))
        for l in frm + to:
            l.sort(key=lambda x: x[0])
        fo = np.zeros(self.nv + 1, np.uint64); t_o = np.zeros(self.nv + 1, np.uint64)
        np.cumsum([len(x) for x in frm], out=fo[1:]); np.cumsum([len(x) for x in to], out=t_o[1:])
        off = np.zeros(len(self.edges) + 1, np.uint64)
        np.cumsum([len(s) for _, _, s in self.edges], out=off[1:])
        pk, bo, ln = F.pack_bases(np.concatenate([s for _, _, s in self.edges]), off)
        return F.HBV(self.K, fo, np.array([v for l in frm for v, _ in l], np.int32), np.array([e for l in frm for _, e in l], np.int32),
                     t_o, np.array([e for l in to for _, e in l], np.int32), pk, bo, ln)


class Hand:
    """a hand-made graph whose edges really overlap by K - 1: every vertex has a (K-1)-mer, an edge u -> v with m inner bases is
    J[u] + m random bases + J[v]; reads are cut from the concatenation of an edge path"""

    def __init__(self, K=20, seed=1):
        self.K, self.rng, self.b, self.J = K, np.random.default_rng(seed), Builder(K), {}
        self.paths, self.offs, self.codes, self.quals = [], [], [], []

    def vertex(self):
        v = self.b.vertex()
        self.J[v] = _seq(self.rng, self.K - 1); self.J[v ^ 1] = _rc(self.J[v])
        return v

    def edge(self, u, v, m, seq=None):
        s = np.concatenate([self.J[u], _seq(self.rng, m), self.J[v]]) if seq is None else seq
        return self.b.edge(u, v, s, mirror=not np.array_equal(s, _rc(s)) or (v != (u ^ 1)))

    def cat(self, path):
        out = [self.b.edges[path[0]][2]]
        for e in path[1:]:
            out.append(self.b.edges[e][2][self.K - 1:])
        return np.concatenate(out)

    def read(self, path, offset, length, qual=30, errors=(), rc=False):
        """a read of `length` bases from offset `offset` of the walk `path`; rc: the read of the other strand, pathed on the mirror edges;
        qual: one value for every base, or one value per base in the walk's direction (reversed with the bases when rc)"""
        c = self.cat(path)[offset:offset + length].copy()
        q = np.full(len(c), qual, np.uint8) if np.ndim(qual) == 0 else np.array(qual, np.uint8)
        assert len(q) == len(c)
        for p in errors:
            c[p] = (c[p] + 1) & 3
        if rc:
            total = len(self.cat(path))
            path = [e ^ 1 for e in reversed(path)]
            offset = total - offset - length
            c = _rc(c); q = q[::-1].copy()
        self.paths.append(list(path)); self.offs.append(offset); self.codes.append(c); self.quals.append(q)

    def case(self):
        h = self.b.hbv()
        po = np.zeros(len(self.paths) + 1, np.uint64); ro = np.zeros(len(self.paths) + 1, np.uint64)
        if self.paths:
            np.cumsum([len(p) for p in self.paths], out=po[1:]); np.cumsum([len(c) for c in self.codes], out=ro[1:])
        paths = (np.array(self.offs, np.int32), po, np.array([e for p in self.paths for e in p], np.int32))
        codes = np.concatenate(self.codes) if self.codes else np.zeros(0, np.uint8)
        quals = np.concatenate(self.quals) if self.quals else np.zeros(0, np.uint8)
        return h, paths, F.pack_bases(codes, ro), quals


def _branch(h, n_good=8, n_bad=0, long_b=300, short=None, fan=0):
    """in-edge a -> v -> {b (supported by n_good reads), c (n_bad reads)}; `short`: c is a dead end of that many inner bases;
    fan: both branches end in a vertex with `fan` out-edges; -> the edge ids (a, b, c)"""
    u, v, w, x = h.vertex(), h.vertex(), h.vertex(), h.vertex()
    a = h.edge(u, v, 200); b = h.edge(v, w, long_b); c = h.edge(v, x, long_b if short is None else short)
    for t in (w, x):
        for _ in range(fan):
            h.edge(t, h.vertex(), 300)
    for i in range(n_good):
        h.read([a, b], 120 + 5 * i, 150, rc=bool(i & 1))
    for i in range(n_bad):
        h.read([a, c], 130 + 5 * i, 150 if short is None else min(150, 2 * (h.K - 1) + 200 + short - 140 - 5 * i), rc=bool(i & 1))
    return a, b, c


def hand_cases():
    """name -> (hbv, paths, (packed, byte_off, read_len), quals, min_size): one quirk of Clean200x / Cleanup each"""
    out = {}
    h = Hand(seed=1); _branch(h, 8, 0); out["weak_branch"] = h.case() + (0,)
    h = Hand(seed=12); _branch(h, 8, 1); out["contested_branch_kept"] = h.case() + (0,)
    h = Hand(seed=2); _branch(h, 8, 0, short=30); out["dead_end_lowers_depth"] = h.case() + (0,)
    h = Hand(seed=3); _branch(h, 8, 0, long_b=100, fan=6); out["eleven_walks_skipped"] = h.case() + (0,)
    h = Hand(seed=4); _branch(h, 8, 0, long_b=100, fan=5); out["ten_walks_voted"] = h.case() + (0,)
    # a read holding the in-edge twice (a, loop, a, b): listed twice, placed four times
    h = Hand(seed=5); a, b, c = _branch(h, 6, 0)
    v0, v1 = h.b.edges[a][0], h.b.edges[a][1]
    lp = h.edge(v1, v0, 10)
    for i in range(3):
        h.read([a, lp, a, b], 150 + i, 400, rc=bool(i & 1))
    out["edge_twice"] = h.case() + (0,)
    # a branch seen only from the reverse strand
    h = Hand(seed=6); u, v, w, x = h.vertex(), h.vertex(), h.vertex(), h.vertex()
    a = h.edge(u, v, 200); b = h.edge(v, w, 300); c = h.edge(v, x, 300)
    for i in range(8):
        h.read([a, b], 120 + 5 * i, 150, rc=True)
    out["reverse_strand_only"] = h.case() + (0,)
    # a circle made entirely of 1-in/1-out vertices, beside a branch
    h = Hand(seed=7); _branch(h, 8, 0)
    c0, c1, c2 = h.vertex(), h.vertex(), h.vertex()
    e0 = h.edge(c0, c1, 50); e1 = h.edge(c1, c2, 60); e2 = h.edge(c2, c0, 70)
    h.read([e1, e2, e0, e1], 10, 200); h.read([e2, e0], 30, 100, rc=True)
    out["circle"] = h.case() + (0,)
    # a palindromic edge (its own mirror) between a run that merges and its mirror image; a read that starts inside the run
    h = Hand(seed=8); p0, p1, p2 = h.vertex(), h.vertex(), h.vertex()
    r0 = h.edge(p0, p1, 40); r1 = h.edge(p1, p2, 50)
    half = _seq(h.rng, 30)
    pal = np.concatenate([h.J[p2], half, _rc(half), h.J[p2 ^ 1]])
    pe = h.edge(p2, p2 ^ 1, 0, seq=pal)
    h.read([r1, pe, r1 ^ 1], 20, 200); h.read([r0, r1], 5, 120); h.read([r1], 3, 60, rc=True)
    out["palindrome_next_to_run"] = h.case() + (0,)
    # a run of four edges: the reads that start on its 2nd, 3rd and 4th edge have their offsets moved
    h = Hand(seed=9); vs = [h.vertex() for _ in range(5)]
    es = [h.edge(vs[i], vs[i + 1], 30 + 10 * i) for i in range(4)]
    for k in range(4):
        h.read(es[k:], 7 + k, 100, rc=bool(k & 1))
    out["offset_moves_in_run"] = h.case() + (0,)
    # pass 2 votes where pass 1 could not: v has 12 walks (skipped) until pass 1 has cut the fan behind b down to one edge and merged it
    h = Hand(seed=13); a, b, c = _branch(h, 8, 0, long_b=100, fan=6)
    w = h.b.edges[b][1]
    f0 = next(e for e, (u, _, _) in enumerate(h.b.edges) if u == w)
    for i in range(6):
        h.read([b, f0], 50 + 3 * i, 150, rc=bool(i & 1))
    out["pass2_exposes"] = h.case() + (0,)
    h = Hand(seed=10); _branch(h, 0, 0); out["no_reads"] = h.case() + (0,)
    h = Hand(seed=11); vs = [h.vertex() for _ in range(3)]
    es = [h.edge(vs[0], vs[1], 100), h.edge(vs[1], vs[2], 100)]
    h.read(es, 10, 150); t0, t1 = h.vertex(), h.vertex(); h.edge(t0, t1, 5)
    out["no_branches_min_size"] = h.case() + (40,)
    return out

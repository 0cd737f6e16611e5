"""Inputs of the tests of w2rap_step7_line_files (DumpLineFiles): cases the reference's own main has run, and cases only the model
(tests/step7_fasta_model.py) and literal outcomes derived by hand can hold.

RECORDED (tests/golden/refruns/step7_ff_<case>/): the reference's main with ``--from_step 7`` on the case written as t.contig.hbv/.paths,
t.fin.lines and t.fin.lines.npairs, at 1 thread and at 4, which had to agree: a.lines.fasta, a.lines.efasta, a.lines.src, stats and
t_assembly.lines.  A record pins the function only if Step 7 left its inputs alone, so the recording fails otherwise:
  no-gap cases   the recorded t_assembly_raw.gfa IS the dump of the case's own graph (oracle/oracle_gfa.py; but for the colour tags): the inputs of the function
                 are the case's graph, paths and involution, and the recorded t_assembly.lines as the lines;
  gap cases      every old edge's S line is unchanged.  Step 7 truncates the paths behind its gaps and does not write them out, so
                 these cases pin the texts only where no cell has two or more paths (no vote depends on the paths) -- both of them
                 are such; a gap case with bubbles would pin efasta and src only.
Contigs are 600 K-mers: lines of less than 1000 K-mers are taken out by Step 7's cleanup (a bubble between two contigs of 500 stays,
of 450 goes; looked for when the cases were recorded), gap cases 6000 (main's MIN_LINE is 5000).

MODEL ONLY: what no run of main can show -- lines shorter than the cleanup leaves, more than 50 paths in a cell (FindLines gives up
there), a line that is its own mirror, shares of 0 (in a real graph the paths of a cell share the K-1 bases of their vertex), paths of
edges of exactly K bases, branches of several edges (the cleanup joins a chain into one edge), hand-written unsorted line orders."""
import os
import re
import shutil

import numpy as np

import step7_cases as S
import step7_fasta_model as M
import step7_model as M7
from conftest import reference_outputs
from w2rap_contigger_amd import formats as F

K = S.K
BODY = 600
FF_OUTPUTS = ["a.lines.fasta", "a.lines.efasta", "a.lines.src", "stats", "t_assembly.lines"]


# ---------------------------------------------------------------------------------------------------------------- builders
def seq_edge(g, u, v, middle):
    """a real edge u -> v whose bases between the two vertices' (K-1)-mers are `middle` (codes 0..3) -> its id"""
    s = np.concatenate([g.J[u], np.asarray(middle, np.uint8), g.J[v]])
    g.edges.append((u, v, s)); g.edges.append((v ^ 1, u ^ 1, (3 - s[::-1]).astype(np.uint8)))
    return len(g.edges) - 2


def raw_edge(g, codes):
    """an edge between two vertices of its own with exactly these bases (no overlap with anything) -> its id"""
    u, v = g.v(), g.v()
    s = np.asarray(codes, np.uint8)
    g.edges.append((u, v, s)); g.edges.append((v ^ 1, u ^ 1, (3 - s[::-1]).astype(np.uint8)))
    return len(g.edges) - 2


def bubble(g, branches, body=BODY):
    """a -> {branches} -> c; a branch is a K-mer count (one edge), a list of them (a chain) or an array of middle codes
    -> (a, [the edges of every branch], c)"""
    v = [g.v() for _ in range(4)]
    a = g.e(v[0], v[1], body)
    out = []
    for b in branches:
        if isinstance(b, np.ndarray):
            out.append([seq_edge(g, v[1], v[2], b)])
        elif isinstance(b, int):
            out.append([g.e(v[1], v[2], b)])
        else:
            vs = [v[1]] + [g.v() for _ in b[1:]] + [v[2]]
            out.append([g.e(vs[i], vs[i + 1], k) for i, k in enumerate(b)])
    return a, out, g.e(v[2], v[3], body)


def through(g, a, branch, c, n=1, mirrored=False):
    """n pairs whose first read walks a, the branch and c (mirrored: the same walk on the other strand)"""
    p = [a] + list(branch) + [c]
    if mirrored:
        g.pair([e ^ 1 for e in reversed(p)], [a], n)
    else:
        g.pair(p, [c ^ 1], n)


def finish(g, lines=None, **kw):
    """the case with npairs as Step 6 would have written them (the model of part LINES); lines None: one line per edge"""
    lines = [] if lines is None else [l for line in lines for l in (line, S.mirror_line(line))]
    case = g.case(lines=lines, **kw)
    case["npairs"] = np.array(M7.run(case["hbv"], case["inv"], case["paths"], case["nested"], parts=("lines",))["npairs"], np.int32)
    return case


def both(lines):
    """every line followed by its mirror image"""
    return [l for line in lines for l in (line, S.mirror_line(line))]


def line_of(a, branches, c):
    return [[[a]], [list(b) for b in branches], [[c]]]


# ---------------------------------------------------------------------------------------------------------------- recorded cases
def _tie(n, tied, seed):
    g = S.Contigs(seed, real=True)
    a, br, c = bubble(g, [40 + i for i in range(n)])
    for t in tied:
        through(g, a, br[t], c, 2)
    return finish(g, [line_of(a, br, c)])


def recorded_cases():
    """name -> (case, kind); the lines given to main are hand-written (what Step 6 would have found), the lines of the function are
    the recorded t_assembly.lines"""
    out = {}
    # the issue's bubble: three crossing reads on the 45-K-mer branch, one of them on the other strand, against one
    g = S.Contigs(1, real=True); a, br, c = bubble(g, [40, 45])
    through(g, a, br[1], c, 2); through(g, a, br[1], c, 1, mirrored=True); through(g, a, br[0], c, 1)
    out["bubble"] = finish(g, [line_of(a, br, c)])
    # reads that end at e, that end inside a branch two paths share, on the other strand only, and one through e twice
    g = S.Contigs(2, real=True); v = [g.v() for _ in range(5)]
    a = g.e(v[0], v[1], BODY); p = g.e(v[1], v[4], 30); q1 = g.e(v[4], v[2], 31); q2 = g.e(v[4], v[2], 33); r = g.e(v[1], v[2], 50); c = g.e(v[2], v[3], BODY)
    g.pair([a], [c ^ 1], 3)                                       # ends at e: matches every path by truncation
    g.pair([a, p], [c ^ 1], 2)                                    # ends inside the shared branch: two paths match
    g.pair([c ^ 1, q2 ^ 1, p ^ 1, a ^ 1], [a], 2)                 # the other strand only
    g.pair([a, r, c], [c ^ 1], 1)
    out["read_ends"] = finish(g, [[[[a]], [[p, q1], [p, q2], [r]], [[c]]]])
    g = S.Contigs(3, real=True); a, br, c = bubble(g, [40, 45])
    g.pair([a, br[0][0], a, br[1][0]], [c ^ 1], 1)                # through e twice: counted four times (path 0 twice, path 1 twice)
    through(g, a, br[1], c, 1)
    out["twice"] = finish(g, [line_of(a, br, c)])
    # ties: std::sort decides
    out["tie_3"] = _tie(3, (1, 2), 4)
    out["tie_16"] = _tie(16, (3, 7, 15), 5)
    out["tie_17"] = _tie(17, (3, 7, 16), 6)
    out["tie_17_ends"] = _tie(17, (0, 16), 7)
    out["tie_20"] = _tie(20, (3, 7, 18), 8)
    # a cell of 50 paths
    g = S.Contigs(9, real=True); a, br, c = bubble(g, [40 + i for i in range(50)])
    for t, n in ((49, 3), (17, 2), (0, 1)):
        through(g, a, br[t], c, n)
    out["cell_50"] = finish(g, [line_of(a, br, c)])
    # 0, 1, 63, 64, 65 and 257 index entries of e: one bubble per count
    g = S.Contigs(11, real=True); lines = []
    for i, n in enumerate((0, 1, 63, 64, 65, 257)):
        a, br, c = bubble(g, [40, 45], BODY + 10 * i)
        if n:
            g.pair([a, br[i & 1][0]], [], n)                       # (the mate has no path: inv[e] stays without entries)
        lines.append(line_of(a, br, c))
    out["entries"] = finish(g, lines)
    # efasta: path 0 a prefix of path 1; shares that meet in the middle (x0 = ..ACAC, x1 = ..ACTAC: left 2, right 2 of the middles)
    rng = np.random.default_rng(12)
    g = S.Contigs(12, real=True); m0 = rng.integers(0, 4, 30).astype(np.uint8)
    a, br, c = bubble(g, [m0, np.concatenate([m0, rng.integers(0, 4, 7).astype(np.uint8)])])
    a2, br2, c2 = bubble(g, [np.array([0, 1, 0, 1], np.uint8), np.array([0, 1, 3, 0, 1], np.uint8)], BODY + 7)
    through(g, a, br[1], c, 1); through(g, a2, br2[0], c2, 1)
    out["efasta_shares"] = finish(g, [line_of(a, br, c), line_of(a2, br2, c2)])
    # circular lines: kind 2 a loop of one edge, kind 1 a -> {b1, b2} -> back to a
    g = S.Contigs(13, real=True); u = g.v(); loop = g.e(u, u, 2 * BODY)
    v1, v2 = g.v(), g.v(); a = g.e(v1, v2, 2 * BODY); b1 = g.e(v2, v1, 40); b2 = g.e(v2, v1, 45)
    g.pair([a, b2, a], [a ^ 1], 2); g.pair([a, b1], [a ^ 1], 1)
    out["circular"] = dict(finish(g, [[[[loop]]], [[[a]], [[b1], [b2]], [[a]]]]))
    # generated: bubbles of 2 to 4 branches between contigs of mixed lengths, reads along random walks (branches of one edge: the
    # cleanup joins a chain of edges into one)
    for seed in (21, 22):
        rng = np.random.default_rng(seed); g = S.Contigs(seed, real=True); lines = []
        for i in range(6):
            nb = int(rng.integers(2, 5))
            a, br, c = bubble(g, [int(rng.integers(25, 70)) for _ in range(nb)], int(rng.integers(BODY, 2 * BODY)))
            for _ in range(int(rng.integers(0, 7))):
                b = br[int(rng.integers(nb))]; kind = int(rng.integers(4))
                if kind < 2:
                    through(g, a, b, c, int(rng.integers(1, 4)), mirrored=kind == 1)
                else:
                    g.pair([a] + b[:int(rng.integers(1, len(b) + 1))], [] if kind == 3 else [a ^ 1], 1)
            lines.append(line_of(a, br, c))
        lone = g.contig(2 * BODY)
        lines.append([[[lone]]])
        out[f"generated_{seed}"] = finish(g, lines)
    cases = {k: (v, "nogap") for k, v in out.items()}
    # gaps: count_3 of the Step-7 cases (two contigs, three pairs across), and three contigs in a row
    cases["gap_1"] = (S.hand_cases(real=True)["count_3"], "gap")
    g = S.Contigs(30, real=True); a, b, c = g.contig(), g.contig(), g.contig(); g.link(a, b, 3); g.link(b, c, 3)
    g.pair([a], [a ^ 1], 3); g.pair([c], [c ^ 1], 3)            # (as many pairs on the outer contigs as on the middle one: the coverage test passes)
    cases["gap_2"] = (finish(g), "gap")
    return cases


def _s_lines(text):
    return {f[1]: f[2] for f in (row.split("\t") for row in text.splitlines()) if f[0] == "S"}


def _record(name, case, kind, workdir):
    from oracle import oracle_gfa
    S._main_twice(workdir, ["--from_step", "7"], FF_OUTPUTS + ["t_assembly_raw.gfa"])
    gfa = open(os.path.join(workdir, "t_assembly_raw.gfa"), "rb").read()
    own = oracle_gfa.raw_gfa(case["hbv"])
    if kind == "nogap":                                          # (main colours the segments by line, the plain dump writes "black")
        plain = lambda t: re.sub(rb"\tCL:z:[a-z0-9]+\n", b"\n", t)
        assert plain(gfa) == plain(own), f"{name}: Step 7 did not leave the graph alone; the record would not pin the function"
    else:
        new, old = _s_lines(gfa.decode()), _s_lines(own.decode())
        assert all(new.get(k) == v for k, v in old.items()), f"{name}: Step 7 changed an old edge"
        lines = F.read_lines(os.path.join(workdir, "t_assembly.lines")).nested()
        assert all(len(cell) == 1 for line in lines for cell in line), f"{name}: a gap case with a cell of several paths pins efasta and src only"
    return None


def fasta_run(name, case, kind, workdir):
    """stages the case as the files main reads (held to the record by SHA-256) and -> dict(fasta, efasta, src, stats: the recorded
    bytes; lines: the recorded t_assembly.lines as formats.Lines)"""
    w = lambda f: os.path.join(workdir, f)
    F.write_hbv(w("t.contig.hbv"), case["hbv"]); F.write_paths(w("t.contig.paths"), *case["paths"]); F.write_lines(w("t.fin.lines"), case["lines"])
    F.write_int_vec(w("t.fin.lines.npairs"), case["npairs"] if case["npairs"] is not None else case["expect"]["npairs"])
    reference_outputs(f"step7_ff_{name}", workdir, S.S7_INPUTS, FF_OUTPUTS, lambda: _record(name, case, kind, workdir))
    rd = lambda f: open(w(f), "rb").read()
    return dict(fasta=rd("a.lines.fasta"), efasta=rd("a.lines.efasta"), src=rd("a.lines.src"), stats=rd("stats"), lines=F.read_lines(w("t_assembly.lines")))


_RECORDS = {}


def recorded(tmp_root):
    """every recorded case once per session: name -> (case, kind, record)"""
    if not _RECORDS:
        for name, (case, kind) in recorded_cases().items():
            d = os.path.join(str(tmp_root), name)
            os.makedirs(d, exist_ok=True)
            _RECORDS[name] = (case, kind, fasta_run(name, case, kind, d))
            shutil.rmtree(d)
    return _RECORDS


# ---------------------------------------------------------------------------------------------------------------- model-only cases
def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def model_cases():
    """name -> case with hand-written lines (`nested`); `expect` holds literal outcomes derived by hand"""
    out = {}
    rng = np.random.default_rng(40)
    # text layout: bodies of 79, 80, 81 and 160 characters (one edge, the line's last cell: no cut), forward lines first so that all
    # are printed; rows: 1 short, 1 full and no empty row, 2, 2 full
    g = S.Contigs(40, real=True); es = [raw_edge(g, _rand(rng, n)) for n in (79, 80, 81, 160)]
    c = g.case(lines=[[[[e]]] for e in es] + [[[[e ^ 1]]] for e in es])
    c["expect"] = dict(printed=[1] * 8, fasta_sizes=[(18 + 79 + 1), (18 + 80 + 1), (18 + 81 + 2), (18 + 160 + 2)])
    out["layout_rows"] = c
    # headers: 101 forward lines, then their mirrors: line_9 / line_10 and line_99 / line_100 are printed (an unsorted order prints both strands)
    g = S.Contigs(41, real=True); es = [raw_edge(g, _rand(rng, 20 + i % 7)) for i in range(101)]
    c = g.case(lines=[[[[e]]] for e in es] + [[[[e ^ 1]]] for e in es])
    c["expect"] = dict(printed=[1] * 202)
    out["layout_headers"] = c
    # pieces at every output offset modulo 16 and base offset modulo 4: one cell of one path of 70 edges of K .. K + 40 bases (an edge
    # behind the first starts at base K - 1), and bubbles whose branches share 0 .. 7 bases more than the vertex: the clipped pieces of
    # efasta start at every base offset
    g = S.Contigs(42, real=True); chain = [raw_edge(g, _rand(rng, K + int(rng.integers(0, 41)))) for _ in range(70)]
    lines = [[[chain]], [[[e ^ 1 for e in reversed(chain)]]]]
    for i in range(8):
        shared = _rand(rng, i)
        a, br, cc = bubble(g, [np.concatenate([shared, [0], _rand(rng, 9 + i)]), np.concatenate([shared, [1], _rand(rng, 5)])], 37 + i)
        through(g, a, br[i & 1], cc, 1)
        lines += [line_of(a, br, cc), S.mirror_line(line_of(a, br, cc))]
    out["layout_offsets"] = g.case(lines=lines)
    assert len(out["layout_offsets"]["nested"]) == len(lines)
    # the back-cut across K - 1 and more edges of exactly K bases: a (50 bases) then 19, 20 and 25 edges of K bases, each adding one base;
    # K - 1 = 19 bases are cut: the pieces of the last 19 edges are empty, with 19 edges only a's own are left.  A gap and c follow
    g = S.Contigs(43, real=True); lines = []; sizes = []
    for n in (19, 20, 25):
        a = raw_edge(g, _rand(rng, 50)); tail = [raw_edge(g, _rand(rng, K)) for _ in range(n)]; c2 = raw_edge(g, _rand(rng, 30))
        lines.append([[[a] + tail], [[]], [[c2]]])
        sizes += [50 + n - (K - 1) + 100 + 30, 30 - (K - 1) + 100 + 50 + n]
    c = g.case(lines=both(lines))
    # the mirror image of such a line is PRINTED too: the rule compares front()[0][0] with inv of back()[0][0], and the last cell of the
    # mirror starts with the mirror of the tail's last edge, not of a.  There the path is the line's last cell: nothing is cut
    c["expect"] = dict(printed=[1] * 6, body_sizes=sizes, n_gap_cells=6)
    out["back_cut"] = c
    # the skip rule: a line next to its mirror image (the second is skipped), the same two the other way round with a line between
    # them (both printed), and a line that is its own mirror: an edge with inv[e] == e (printed when it is first; skipped behind itself)
    g = S.Contigs(44, real=True); x, y, z = (raw_edge(g, _rand(rng, 45)) for _ in range(3))
    c = g.case(lines=[[[[x]]], [[[x ^ 1]]], [[[y ^ 1]]], [[[z]]], [[[y]]], [[[z ^ 1]]]])
    c["expect"] = dict(printed=[1, 0, 1, 1, 1, 1])
    out["skip_mirror"] = c
    g = S.Contigs(45, real=True); half = _rand(rng, 30); pal = raw_edge(g, np.concatenate([half, (3 - half[::-1])]))
    c = g.case(lines=[[[[pal]]], [[[pal]]], [[[pal ^ 1]]]])
    c["inv"] = c["inv"].copy(); c["inv"][pal] = pal; c["inv"][pal ^ 1] = pal ^ 1       # (the edge and the builder's copy of it are each their own mirror)
    c["expect"] = dict(printed=[1, 0, 1])
    out["skip_own_mirror"] = c
    # circular lines of each kind, hand-written: a loop u -> u; a -> {b1, b2} -> a with the last cell not written
    g = S.Contigs(46, real=True); u = g.v(); loop = g.e(u, u, 90)
    v1, v2 = g.v(), g.v(); a = g.e(v1, v2, 70); b1 = g.e(v2, v1, 40); b2 = g.e(v2, v1, 45)
    g.pair([a, b2, a], [a ^ 1], 2)
    c = g.case(lines=both([[[[loop]]], [[[a]], [[b1], [b2]], [[a]]]]))
    c["expect"] = dict(printed=[1, 0, 1, 0], n_circular1=1, n_circular2=1, body_sizes=[109, None, 70 + 45, None])
    out["circular_hand"] = c
    # shares of 0: two raw paths that differ in their first and in their last base; and path 0 a prefix of path 1
    g = S.Contigs(47, real=True); a = raw_edge(g, _rand(rng, 40)); m = _rand(rng, 30)
    p0 = raw_edge(g, np.concatenate([[0], m, [0], _rand(rng, K - 1)])); p1 = raw_edge(g, np.concatenate([[1], m, [1], _rand(rng, K - 1)])); cc = raw_edge(g, _rand(rng, 40))
    q0 = raw_edge(g, np.concatenate([m, _rand(rng, K - 1)])); q1 = raw_edge(g, np.concatenate([m, [2, 3], _rand(rng, K - 1)]))
    d = raw_edge(g, _rand(rng, 40))
    c = g.case(lines=both([[[[a]], [[p0], [p1]], [[cc]], [[q0], [q1]], [[d]]]]))
    c["expect"] = dict(shares=[(0, 0), (0, 0), (0, 0), (30, 0), (0, 0)] + [(0, 0)] * 5)
    out["shares_zero"] = c
    # a cell of 70 paths (no LDS row) with one winner, and its votes spread over 64 lanes and more: 130 reads
    g = S.Contigs(48, real=True); a, br, cc = bubble(g, [40 + i % 9 for i in range(70)], 60)
    for t, n in ((69, 70), (64, 40), (3, 20)):
        through(g, a, br[t], cc, n)
    c = g.case(lines=[line_of(a, br, cc), S.mirror_line(line_of(a, br, cc))])
    c["expect"] = dict(n_cells_wide=1, best_of_cell_1=69)
    out["cell_70"] = c
    # branches of 10 edges (main joins such a chain into one edge: no record), reads on either strand and one that stops inside
    g = S.Contigs(50, real=True); a, br, cc = bubble(g, [[30 + i for i in range(10)], [41 + i for i in range(10)]], 60)
    through(g, a, br[1], cc, 2); through(g, a, br[0], cc, 1, mirrored=True); g.pair([a] + br[0][:4], [a ^ 1], 2)
    c = g.case(lines=both([line_of(a, br, cc)]))
    c["expect"] = dict(cov_of_cell_1=[3, 2])
    out["branch_10"] = c
    # generated with branches of 1 to 3 edges
    rg = np.random.default_rng(51); g = S.Contigs(51, real=True); lines = []
    for i in range(5):
        nb = int(rg.integers(2, 5))
        a, br, cc = bubble(g, [[int(rg.integers(25, 70)) for _ in range(int(rg.integers(1, 4)))] for _ in range(nb)], int(rg.integers(60, 200)))
        for _ in range(int(rg.integers(0, 7))):
            b = br[int(rg.integers(nb))]; kind = int(rg.integers(4))
            if kind < 2:
                through(g, a, b, cc, int(rg.integers(1, 4)), mirrored=kind == 1)
            else:
                g.pair([a] + b[:int(rg.integers(1, len(b) + 1))], [] if kind == 3 else [a ^ 1], 1)
        lines.append(line_of(a, br, cc))
    out["generated_chains"] = g.case(lines=both(lines))
    # no read at all
    g = S.Contigs(49, real=True); a, br, cc = bubble(g, [40, 45], 60)
    out["no_reads"] = g.case(lines=[line_of(a, br, cc), S.mirror_line(line_of(a, br, cc))])
    return out


# ---------------------------------------------------------------------------------------------------------------- checks
TIE_BEST = {"tie_3": 1, "tie_16": 3, "tie_17": 16, "tie_17_ends": 16, "tie_20": 18}      # the path main flattened (std::sort: the lowest tied index up to 16 paths only)


def as_dict(res):
    """a step7.LineFiles as the model's dict"""
    d = dict(fasta=res.fasta, efasta=res.efasta, src=res.src, counters=res.counters)
    d.update({k: (None if v is None else [int(x) for x in v]) for k, v in res.arrays.items()})
    return d


def inputs_of(name, case, kind, rec):
    """what the function is given for a recorded case: the case's graph, involution and paths, the RECORDED lines"""
    return case["hbv"], case["inv"], case["paths"], rec["lines"]


def check_expect(case, got):
    """holds a result (the model's dict, or as_dict of the library's) to the literal outcomes of a model-only case"""
    nested = case["nested"]
    bodies = [b"".join(rec.split(b"\n")[1:]) for rec in got["fasta"].split(b">")[1:]]
    shown = iter(bodies)
    per_line = [next(shown) if p else None for p in got["printed"]]
    first_cell = np.cumsum([0] + [len(line) for line in nested])
    for k, v in case["expect"].items():
        if k == "printed":
            assert list(got["printed"]) == v, (k, got["printed"])
        elif k == "body_sizes":
            assert [None if b is None else len(b) for b in per_line] == v, (k, [None if b is None else len(b) for b in per_line])
        elif k == "fasta_sizes":
            assert [len(r) + 1 for r in got["fasta"].split(b">")[1:]][:len(v)] == v, k
        elif k == "shares":
            assert list(zip(got["left_share"], got["right_share"])) == v, (k, got["left_share"], got["right_share"])
        elif k == "best_of_cell_1":
            assert got["best"][1] == v, (k, got["best"][1])
        elif k == "cov_of_cell_1":
            assert got["cov"][1:1 + len(v)] == v, (k, got["cov"][:8])
        else:
            assert got["counters"][k] == v, (k, got["counters"][k])
    assert len(first_cell) == len(nested) + 1


def compare(got, want, what=("fasta", "efasta", "src", "printed", "best", "cov", "left_share", "right_share")):
    """a result of the library against the model's, array for array and counter for counter"""
    for k in what:
        a, b = got[k], want[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert (a == b if isinstance(a, bytes) else [int(x) for x in a] == [int(x) for x in b]), k
    assert got["counters"] == want["counters"], {k: (got["counters"][k], want["counters"][k]) for k in want["counters"] if got["counters"][k] != want["counters"][k]}

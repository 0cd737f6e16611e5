"""Inputs of the tests of w2rap_step7_coverage (ComputeCoverage, CNIntegerFraction, .covs, .lines.stats): cases the reference's own
main has run, and cases only the model (tests/step7_cov_model.py) and literal outcomes derived by hand can hold.  K = 20.

RECORDED (tests/golden/refruns/step7_cov_<case>/): the reference's main with ``--from_step 7`` on the case written as t.contig.hbv/.paths,
t.fin.lines and t.fin.lines.npairs, at 1 thread and at 4, which had to agree: t_assembly.covs, t_assembly.lines.stats,
t_assembly.lines.npairs and t_assembly.lines.  A record pins the function only if Step 7 left graph and paths alone, so the recording
asserts that t_assembly_raw.gfa IS the dump of the case's own graph (no case has a gap) and that the recorded npairs are what the model
of part LINES counts on the case's paths and the recorded lines.  Every line is 1,100 K-mers or more: the cleanup takes out a lone contig of 1,000 K-mers (seen when the cases were recorded).
The lines the function is given are the RECORDED t_assembly.lines (FindLines and SortLines of the run).

STEP-6 RECORDS (step7_cn_<name>/): ``--from_step 6 --to_step 6``; t.contig.hbv, t.contig.paths and t.fin.lines are the inputs
ComputeCoverage had there, the `CN fraction good = ...` line of stdout is what CNIntegerFraction made of it.  One per Step-4 fixture and
`hand`, a hand-staged input (stage_cn_hand) with copy numbers of 1.3, 2.3 and 0.7 among eight contigs: the reference takes it as it is and
prints 0.625, 10 of 16 -- the integer reading of abs would print 1.

Recording (with the reference built under oracle/_ref): ``python tests/golden/make_golden.py refruns tests/test_step7_cov_model.py`` -- the
file is named on the command line; make_golden.py's own list of test files is left as it is.

MODEL ONLY: hand-written lines no FindLines would give, own-inverse edges, the sizes at which a kernel takes another way."""
import os
import re
import shutil

import numpy as np

import step7_cases as S
import step7_cov_model as M
import step7_fasta_cases as SF
from conftest import GOLDEN, reference_outputs
from w2rap_contigger_amd import formats as F

K = S.K
COV_OUTPUTS = ["t_assembly.covs", "t_assembly.lines.stats", "t_assembly.lines.npairs", "t_assembly.lines"]


# ---------------------------------------------------------------------------------------------------------------- the reciprocal search
def reciprocal_search(max_pairs=4000, lens=(1024, 1536, 1280, 1792, 1152, 1408, 1664, 1920), base_lens=range(9001, 9999, 2), base_pairs=(1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64, 128, 256, 512)):
    """Brute force over (npairs m, llens L, base_cov = nb / LB): the triples where float((m / L) / b) and float((m / L) * (1.0 / b))
    differ.  The two doubles differ by an ulp at most, so the floats differ only where a float rounding boundary lies between them, and a
    quotient of such small integers comes that close to a boundary only when m * LB / (L * nb) IS one: L * nb a power of two (times what
    divides m * LB) and m * LB an odd number of 25 bits.  A blind search over m <= 2000, L in [1000, 2000), nb <= 600 and LB in
    [9000, 9080) -- 10^11 triples -- found none; this one looks where they can be.  -> [(m, L, nb, LB, as written, by the reciprocal)],
    sorted.  Seconds of numpy; its first result with nb = 512 is RECIPROCAL_HIT below"""
    m = np.arange(1, max_pairs + 1, dtype=np.float64)[:, None]
    LBs = np.array(list(base_lens), np.float64)[None, :]
    hits = []
    for L in lens:
        x = m / np.float64(L)
        for nb in base_pairs:
            b = np.float64(nb) / LBs
            q1, q2 = (x / b).astype(np.float32), (x * (np.float64(1.0) / b)).astype(np.float32)
            hits += [(int(m[i, 0]), L, nb, int(LBs[0, j]), float(q1[i, j]), float(q2[i, j])) for i, j in np.argwhere(q1 != q2)]
    return sorted(hits)


# the search's result: m pairs on L K-mers over base_cov = nb / LB; the float as written, the float by the reciprocal
RECIPROCAL_HIT = (2839, 1024, 512, 9907, 53.64603805541992, 53.646034240722656)


def check_reciprocal_hit():
    m, L, nb, LB, q1, q2 = RECIPROCAL_HIT
    x, b = m / L, nb / LB
    assert float(np.float32(x / b)) == q1 and float(np.float32(x * (1.0 / b))) == q2 and q1 != q2


# ---------------------------------------------------------------------------------------------------------------- builders
def lone(g, kmers, n, kind=0):
    """a contig of its own with n pairs on it: kind 0 one mate on e and one on inv[e], 1 both mates on e, 2 the second mate unplaced"""
    a = g.contig(kmers)
    if n:
        g.pair([a], [[a ^ 1], [a], []][kind], n)
    return a


def contigs_case(seed, specs):
    """specs: (kmers, pairs) per contig, the kinds of reads in turn"""
    g = S.Contigs(seed, real=True)
    for i, (kmers, n) in enumerate(specs):
        lone(g, kmers, n, i % 3)
    return SF.finish(g)


def _peak_specs(rng, n, centre, spread, length=(1100, 1500)):
    """n contigs whose coverages scatter around `centre` (pairs per K-mer), densest in the middle"""
    out = []
    for i in range(n):
        L = int(rng.integers(*length))
        d = float(rng.normal(0.0, spread))
        out.append((L, max(1, int(round(centre * (1.0 + d) * L)))))
    return out


def bubble_line(g, branches, body=1000):
    a, br, c = SF.bubble(g, branches, body)
    return a, br, c, SF.line_of(a, br, c)


def recorded_cases():
    """name -> case; the lines given to main are hand-written (what Step 6 would have found)"""
    out = {}
    # a handful of lone contigs, fewer than 21 candidates: the candidate of the largest mass.  The contig of 1,100 lies below min_len
    # (3000 / 2) and has the highest coverage of all: it must not become a candidate
    out["lone_few"] = contigs_case(1, [(3000, 9), (2000, 7), (1500, 4), (2500, 8), (1100, 30)])
    # 10 and 11 contigs with pairs: 20 and 22 candidates (every line comes with its mirror at the same coverage), on either side of
    # size > 2 * min_shoulder
    # size > 2 * min_shoulder: coverages 5% apart (a candidate's mass is itself and its two neighbours), the longest contig in the middle, so that with 22 the middle is a peak of the shoulder of 10
    # (its window of +-5% is too thin: still the largest mass in the end)
    spec = [(1500 - 40 * abs(i - 5), int(round(0.1 * (1 + 0.05 * (i - 5)) * (1500 - 40 * abs(i - 5))))) for i in range(11)]
    out["cand_20"] = contigs_case(2, spec[:10])
    out["cand_22"] = contigs_case(2, spec)
    # about 80 lines, one peak
    rng = np.random.default_rng(3)
    out["one_peak"] = contigs_case(3, _peak_specs(rng, 40, 0.03, 0.07))
    # about 120 lines, peaks at c and 2c, the larger mass on the second: halved at the end of FindPeak
    rng = np.random.default_rng(4)
    out["two_peaks"] = contigs_case(4, _peak_specs(rng, 24, 0.02, 0.04) + _peak_specs(rng, 36, 0.04, 0.04))
    # the same with a far outlier above 5x the main peak
    rng = np.random.default_rng(4)
    out["two_peaks_outlier"] = contigs_case(5, _peak_specs(rng, 24, 0.02, 0.04) + _peak_specs(rng, 36, 0.04, 0.04) + [(1100, 280)])
    # no pairs at all: base_cov 0, every quotient NaN
    out["no_pairs"] = contigs_case(6, [(1500, 0), (1100, 0), (2100, 0)])
    # pairs only on a line below min_len: no candidate, base_cov 0, that line's coverage inf
    out["pairs_on_short_only"] = contigs_case(7, [(3000, 0), (1200, 5), (2000, 0)])
    # bubbles: branches of 1,000 and 1,001 K-mers (both classes pass), of 999 and 1,000 (one passes, one is skipped), pairs through the branches
    g = S.Contigs(8, real=True); lines = []
    for i, (br, through) in enumerate((((1000, 1001), (3, 5)), ((999, 1000), (4, 2)))):
        a, b, c, line = bubble_line(g, list(br), 1000 + 10 * i)
        for k, n in enumerate(through):
            SF.through(g, a, b[k], c, n)
        SF.through(g, a, b[0], c, 1, mirrored=True)
        g.pair([b[1][0]], [b[1][0] ^ 1], 2)                      # both mates inside a branch
        lines.append(line)
    big = lone(g, 9000, 40)
    out["bubbles_1000"] = SF.finish(g, lines + [[[[big]]]])
    # classes of two and of four parallel paths: a -> {p -> {m1 .. mn} -> q, r} -> c; the class (p, q) has n paths, its length the UPPER median
    for n, mids in ((2, (300, 350)), (4, (300, 350, 310, 340))):
        g = S.Contigs(10 + n, real=True); lines = []
        v = [g.v() for _ in range(6)]
        a = g.e(v[0], v[1], 1100); pp = g.e(v[1], v[2], 400); ms = [g.e(v[2], v[3], k) for k in mids]; q = g.e(v[3], v[4], 400); r = g.e(v[1], v[4], 1200); c = g.e(v[4], v[5], 1100)
        for i, e in enumerate(ms):
            g.pair([a, pp, e, q, c], [c ^ 1], 1 + i)
        g.pair([r], [r ^ 1], 3); g.pair([c ^ 1, q ^ 1], [a], 2)
        big = lone(g, 9000, 45)
        out[f"parallel_{n}"] = SF.finish(g, [[[[a]], [[pp, e, q] for e in ms] + [[r]], [[c]]], [[[big]]]])
    # the long-edge rule: a -> {p -> {q1, q2}, r} -> c.  The firsts are {p, r}, the lasts {q1, q2, r}: the sizes differ, no class is formed, and
    # p is left to the long-edge rule at 1,000 K-mers and undefined at 999 (a cell of [p, q1], [p, q2] alone cannot be recorded: main joins
    # a and p into one edge).  One read goes through p twice
    g = S.Contigs(20, real=True); lines = []
    for i, k in enumerate((1000, 999)):
        v = [g.v() for _ in range(5)]
        a = g.e(v[0], v[1], 1100 + i); pp = g.e(v[1], v[2], k); q1 = g.e(v[2], v[3], 31); q2 = g.e(v[2], v[3], 33); r = g.e(v[1], v[3], 50); c = g.e(v[3], v[4], 1100)
        g.pair([pp], [pp ^ 1], 4); g.pair([a, pp, q1, c], [c ^ 1], 2); g.pair([pp, q2, pp], [], 1); g.pair([c ^ 1, q2 ^ 1, pp ^ 1], [a], 3)
        lines.append([[[a]], [[pp, q1], [pp, q2], [r]], [[c]]])
    big = lone(g, 9000, 45)
    out["long_edges"] = SF.finish(g, lines + [[[[big]]]])
    # the reciprocal search's line under each of the three rules: base_cov = 512 / 9907 from the one candidate (min_len is 4,953); a lone
    # contig of 1,024 K-mers with 2,839 pairs (line rule), a branch of 1,024 with 2,839 pairs (cell rule), a shared first edge of 1,024
    # with 2,839 pairs (long-edge rule)
    m, L, nb, LB, _, _ = RECIPROCAL_HIT
    g = S.Contigs(30, real=True)
    big = lone(g, LB, nb); t = lone(g, L, m)
    a, b, c, bl = bubble_line(g, [L, 1500], 1100); g.pair([b[0][0]], [], m)
    v = [g.v() for _ in range(5)]
    a2 = g.e(v[0], v[1], 1101); pp = g.e(v[1], v[2], L); q1 = g.e(v[2], v[3], 31); q2 = g.e(v[2], v[3], 33); r = g.e(v[1], v[3], 50); c2 = g.e(v[3], v[4], 1101)
    g.pair([pp], [], m)
    out["reciprocal"] = SF.finish(g, [[[[big]]], [[[t]]], bl, [[[a2]], [[pp, q1], [pp, q2], [r]], [[c2]]]])
    return out


def _record(name, case, workdir):
    from oracle import oracle_gfa
    S._main_twice(workdir, ["--from_step", "7"], COV_OUTPUTS + ["t_assembly_raw.gfa"])
    gfa = open(os.path.join(workdir, "t_assembly_raw.gfa"), "rb").read()
    plain = lambda t: re.sub(rb"\tCL:z:[a-z0-9]+\n", b"\n", t)
    assert plain(gfa) == plain(oracle_gfa.raw_gfa(case["hbv"])), f"{name}: Step 7 did not leave the graph alone; the record would not pin the function"
    lines = F.read_lines(os.path.join(workdir, "t_assembly.lines")).nested()
    assert all(len(line[0][0]) + 0 and M.line_lengths(case["hbv"], [line])[0] >= 1000 for line in lines), f"{name}: a line below 1,000 K-mers"
    want = M.line_npairs(case["inv"], case["paths"], lines, len(case["hbv"].edge_len))
    assert F.read_int_vec(os.path.join(workdir, "t_assembly.lines.npairs")).tolist() == want, f"{name}: Step 7 did not leave the paths alone"
    return None


def cov_run(name, case, workdir):
    """stages the case as the files main reads (held to the record by SHA-256) -> dict(covs, stats, npairs: the recorded bytes; lines: the
    recorded t_assembly.lines as formats.Lines)"""
    w = lambda f: os.path.join(workdir, f)
    F.write_hbv(w("t.contig.hbv"), case["hbv"]); F.write_paths(w("t.contig.paths"), *case["paths"]); F.write_lines(w("t.fin.lines"), case["lines"])
    F.write_int_vec(w("t.fin.lines.npairs"), case["npairs"])
    reference_outputs(f"step7_cov_{name}", workdir, S.S7_INPUTS, COV_OUTPUTS, lambda: _record(name, case, workdir))
    rd = lambda f: open(w(f), "rb").read()
    return dict(covs=rd("t_assembly.covs"), stats=rd("t_assembly.lines.stats"), npairs=rd("t_assembly.lines.npairs"), lines=F.read_lines(w("t_assembly.lines")))


_RECORDS = {}


def recorded(tmp_root):
    """every recorded case once per session: name -> (case, record)"""
    if not _RECORDS:
        for name, case in recorded_cases().items():
            d = os.path.join(str(tmp_root), name)
            os.makedirs(d, exist_ok=True)
            _RECORDS[name] = (case, cov_run(name, case, d))
            shutil.rmtree(d)
    return _RECORDS


# ---------------------------------------------------------------------------------------------------------------- Step-6 records
CN_OUTPUTS = ["t.contig.hbv", "t.contig.paths", "t.fin.lines"]
_CN_LINE = re.compile(r"^CN fraction good = .*$", re.M)


def _cn_main_twice(workdir):
    """as step7_cases._main_twice for ``--from_step 6 --to_step 6``, keeping the CN line of stdout (equal at 1 thread and at 4)"""
    import subprocess
    res = []
    for t in (1, 4):
        d = os.path.join(workdir, f"threads{t}")
        shutil.copytree(workdir, d, ignore=shutil.ignore_patterns("threads*"))
        out = subprocess.run([S.REF_MAIN, "-r", "x", "-o", d, "-p", "t", "-t", str(t), "-m", "16", "--from_step", "6", "--to_step", "6"], check=True, capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(t))).stdout
        res.append((d, [open(os.path.join(d, f), "rb").read() for f in CN_OUTPUTS], _CN_LINE.findall(out)))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2] and len(res[0][2]) == 1, "the reference's outputs differ between 1 thread and 4"
    for f in CN_OUTPUTS:
        shutil.copy(os.path.join(res[0][0], f), os.path.join(workdir, f))
    for d, *_ in res:
        shutil.rmtree(d)
    return res[0][2][0] + "\n"


def cn_run(name, workdir):
    """a Step-4 fixture's recorded clean graph and paths staged as t.large_K.final.* beside its reads (as step7_cases.step6_run)
    -> (hbv, paths, Lines, the CN line)"""
    import step4_cases as S4
    g, r, ms = S4.FIXTURES[name]
    src = os.path.join(GOLDEN, "refruns", f"step4_{name}_s{ms}")
    for s, d in ((os.path.join(src, "t.large_K.clean.hbv"), "t.large_K.final.hbv"), (os.path.join(src, "t.large_K.clean.paths"), "t.large_K.final.paths"),
                 (os.path.join(GOLDEN, f"{r}.fastb"), "frag_reads_orig.fastb"), (os.path.join(GOLDEN, f"{r}.qualp"), "frag_reads_orig.qualp")):
        shutil.copy(s, os.path.join(workdir, d))
    out = reference_outputs(f"step7_cn_{name}", workdir, ["t.large_K.final.hbv", "t.large_K.final.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp"], CN_OUTPUTS,
                            lambda: _cn_main_twice(workdir))
    w = lambda f: os.path.join(workdir, f)
    return F.read_hbv(w("t.contig.hbv")), F.read_paths(w("t.contig.paths")), F.read_lines(w("t.fin.lines")), out.strip()


# The hand-staged input: eight isolated contigs of 2,400 to 3,800 bases at K = 200 with random bases, each with its reverse complement, staged
# as t.large_K.final.hbv/.paths; error-free pairs of 150-base reads (quality 40) cut from fragments of 400 bases at seeded places, read 1 on
# the contig and read 2 on its reverse complement, as frag_reads_orig.fastb/.qualp with the paths they have.  The pair counts are 0.05 per
# K-mer times HAND_CN: five contigs at copy number 1 and one each near 1.3, 2.3 and 0.7 -- where |int(cov + 0.5) - cov| is about 0.3 as a
# double and 0 as an int.  The copy numbers that come out are what the recorded t.contig.* give; the model is held to the printed fraction.
HAND_K = 200
HAND_BASES = (3800, 2400, 2600, 2800, 3000, 3200, 3400, 3600)
HAND_CN = (1.0, 1.0, 1.0, 1.0, 1.0, 1.3, 2.3, 0.7)
HAND_INPUTS = ["t.large_K.final.hbv", "t.large_K.final.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp"]


def stage_cn_hand(workdir, seed=77):
    rng = np.random.default_rng(seed)
    seqs = []
    for n in HAND_BASES:
        s = rng.integers(0, 4, n).astype(np.uint8)
        seqs += [s, (3 - s[::-1]).astype(np.uint8)]
    E, NV = len(seqs), 2 * len(seqs)                             # edge e from vertex 2e to 2e + 1
    v = np.arange(NV)
    from_off = np.zeros(NV + 1, np.uint64); np.cumsum(v % 2 == 0, out=from_off[1:])
    to_off = np.zeros(NV + 1, np.uint64); np.cumsum(v % 2 == 1, out=to_off[1:])
    e = np.arange(E, dtype=np.int32)
    off = np.zeros(E + 1, np.uint64); np.cumsum([len(s) for s in seqs], out=off[1:])
    pk, bo, ln = F.pack_bases(np.concatenate(seqs), off)
    hbv = F.HBV(HAND_K, from_off, (2 * e + 1).astype(np.int32), e, to_off, e.copy(), pk, bo, ln)
    reads, offsets, edges = [], [], []
    for i, (n, cn) in enumerate(zip(HAND_BASES, HAND_CN)):
        for s in rng.integers(0, n - 400 + 1, int(round(0.05 * cn * (n - HAND_K + 1)))).tolist():
            reads += [seqs[2 * i][s:s + 150], seqs[2 * i + 1][n - (s + 400):n - (s + 400) + 150]]
            offsets += [s, n - (s + 400)]; edges += [2 * i, 2 * i + 1]
    roff = np.arange(len(reads) + 1, dtype=np.uint64) * 150
    w = lambda f: os.path.join(workdir, f)
    F.write_hbv(w("t.large_K.final.hbv"), hbv)
    F.write_paths(w("t.large_K.final.paths"), np.array(offsets, np.int32), np.arange(len(reads) + 1, dtype=np.uint64), np.array(edges, np.int32))
    F.write_fastb(w("frag_reads_orig.fastb"), *F.pack_bases(np.concatenate(reads), roff))
    F.write_qualp(w("frag_reads_orig.qualp"), np.full(150 * len(reads), 40, np.uint8), roff)


def cn_hand_run(workdir):
    """-> (hbv, paths, Lines, the CN line) of the recorded Step 6 on the hand-staged input"""
    stage_cn_hand(workdir)
    out = reference_outputs("step7_cn_hand", workdir, HAND_INPUTS, CN_OUTPUTS, lambda: _cn_main_twice(workdir))
    w = lambda f: os.path.join(workdir, f)
    return F.read_hbv(w("t.contig.hbv")), F.read_paths(w("t.contig.paths")), F.read_lines(w("t.fin.lines")), out.strip()


_CN_RECORDS = {}


CN_NAMES = tuple(S.S6_FIXTURES) + ("hand",)


def cn_recorded(tmp_root):
    if not _CN_RECORDS:
        for name in CN_NAMES:
            d = os.path.join(str(tmp_root), "cn_" + name)
            os.makedirs(d, exist_ok=True)
            _CN_RECORDS[name] = cn_hand_run(d) if name == "hand" else cn_run(name, d)
            shutil.rmtree(d)
    return _CN_RECORDS


# ---------------------------------------------------------------------------------------------------------------- model-only cases
def _entries_case(counts, seed):
    """one long edge (1,000 K-mers, inside a cell whose two paths share it: no line rule, no cell rule) per count, with that many index
    entries: pairs whose first read lies on it, the mate unplaced"""
    g = S.Contigs(seed); lines = []; want = {}
    for i, n in enumerate(counts):
        v = [g.v() for _ in range(5)]
        a = g.e(v[0], v[1], 1200 + i); p = g.e(v[1], v[2], 1000); q1 = g.e(v[2], v[3], 30); q2 = g.e(v[2], v[3], 35); c = g.e(v[3], v[4], 1200)
        if n:
            g.pair([p], [], n)
        line = [[[a]], [[p, q1], [p, q2]], [[c]]]
        lines += [line, S.mirror_line(line)]
        want[p] = n; want[p ^ 1] = n
    case = g.case(lines=lines)
    case["expect"] = dict(long_pairs=want)
    return case


def model_cases():
    """name -> case with hand-written lines (`nested`); `expect` holds literal outcomes derived by hand (see check_expect)"""
    out = {}
    # ---- the overwrite order.  A (0, 3000, 30 pairs), B (2, 1000, 20 pairs).  Line X = [A] [[b1],[b2]] [B] ... ; line Y names b1 as its
    # even cell.  b1 = 4 (1000), b2 = 6 (1001).  Lines: ..., X, X', Y = [[b1]], Y' -- Y comes later: tol[b1] = Y.
    # base_cov: candidates are the lines of llens >= min(10000, max_len / 2).  All pairs lie on A: npairs(X) = 30, llens(X) = 3000 + 1000 + 1000
    # = 5000 (mean of 1000 and 1001 in int); Y: no pair names b1: npairs 0.  Candidates: X and X' only (covl 0.006): base_cov = 0.006.
    # line rule: cov[A] = cov[B] = 1 from X; cov[b1] = 0 / 1000 / 0.006 = 0 from Y (Y >= 1000).  cell rule (X's cell, classes (b1,b1) len
    # 1000 and (b2,b2) len 1001, no pairs on either): cov[b1] = 0 again but by the CELL rule, which runs after every line rule: rule 2
    g = S.Contigs(60); v = [g.v() for _ in range(4)]
    A = g.e(v[0], v[1], 3000); b1 = g.e(v[1], v[2], 1000); b2 = g.e(v[1], v[2], 1001); B = g.e(v[2], v[3], 1000)
    g.pair([A], [A ^ 1], 30)
    X = [[[A]], [[b1], [b2]], [[B]]]
    c = g.case(lines=[X, S.mirror_line(X), [[[b1]]], [[[b1 ^ 1]]]])
    c["expect"] = dict(base_cov=30 / 5000, rule={A: "line", B: "line", b1: "cell", b2: "cell"}, cov={A: 1.0, B: 1.0, b1: 0.0, b2: 0.0}, n_groups=4)
    out["overwrite_cell_over_line"] = c
    # ---- a cell named twice, in two lines with different pair counts: the later line's write stays.  Lines P = [A][cell][B] and
    # Q = [C][cell][D] share the cell {b1, b2}; 2 pairs through b1
    g = S.Contigs(61); v = [g.v() for _ in range(4)]
    A = g.e(v[0], v[1], 2000); b1 = g.e(v[1], v[2], 1000); b2 = g.e(v[1], v[2], 1200); B = g.e(v[2], v[3], 2000); C2 = g.contig(2000); D = g.contig(2000)
    g.pair([A, b1, B], [B ^ 1], 2); g.pair([C2], [C2 ^ 1], 8)
    P = [[[A]], [[b1], [b2]], [[B]]]; Q = [[[C2]], [[b1], [b2]], [[D]]]
    c = g.case(lines=[P, S.mirror_line(P), Q, S.mirror_line(Q)])
    # llens 5100 each; tol[b1], tol[b2] = Q' (the last line that names them): the 2 pairs name P (A, B), P' and, through b1, Q and Q'.
    # npairs: P 2, P' 2, Q 10, Q' 10.  covl 2/5100 and 10/5100; four candidates; radius 8%: masses 10200 each: the FIRST largest: covx[0]:
    # base_cov = 2/5100.  Groups in loop order: P.b1, P.b2, P'.b1', P'.b2', Q.b1, Q.b2, Q'.b1', Q'.b2'; pairs of b1: 2, of b2: 0
    c["expect"] = dict(base_cov=2 / 5100, n_groups=8, group_pairs=[2, 0, 2, 0, 2, 0, 2, 0], cov={b1: np.float32((2 / 1000) / (2 / 5100)), b2: 0.0, A: 1.0, C2: 5.0},
                       rule={b1: "cell", A: "line"})
    out["cell_named_twice"] = c
    # ---- a group holding e and inv[e], and an edge that is its own inverse (Pids reads its row twice: the pairs count once)
    g = S.Contigs(62); v = [g.v() for _ in range(4)]
    A = g.e(v[0], v[1], 2000); p = g.e(v[1], v[2], 1000); r = g.e(v[1], v[2], 1500); B = g.e(v[2], v[3], 2000)
    g.pair([p], [p ^ 1], 3); g.pair([p ^ 1], [], 2); g.pair([r], [], 4)
    X = [[[A]], [[p, p ^ 1, p], [r]], [[B]]]                      # a hand-written path through p, its inverse and p again
    c = g.case(lines=[X, S.mirror_line(X)])
    c["inv"] = c["inv"].copy(); c["inv"][r] = r; c["inv"][r ^ 1] = r ^ 1          # r is its own inverse (and so is the builder's copy)
    # class (p, p): len 3000, e = {p, p'}, pairs 3 + 2 = 5; class (r, r): len 1500, pairs 4
    c["expect"] = dict(group_pairs_head=[5, 4])
    out["inverse_in_group"] = c
    # ---- index rows of 0, 1, 63, 64, 65 and 257 entries
    out["entries"] = _entries_case((0, 1, 63, 64, 65, 257), 63)
    # ---- a pair whose two entries fall on either side of position 64 of a row: 63 pairs with one read on p, then a pair with both
    g = S.Contigs(64); v = [g.v() for _ in range(5)]
    a = g.e(v[0], v[1], 1200); p = g.e(v[1], v[2], 1000); q1 = g.e(v[2], v[3], 30); q2 = g.e(v[2], v[3], 35); cc = g.e(v[3], v[4], 1200)
    g.pair([p], [], 63); g.pair([p], [p], 1); g.pair([p, q1, p], [], 1)
    line = [[[a]], [[p, q1], [p, q2]], [[cc]]]
    c = g.case(lines=[line, S.mirror_line(line)])
    c["expect"] = dict(long_pairs={p: 65})
    out["pair_across_64"] = c
    # ---- a group of 20 edges: a class whose one path is a chain of 20 edges of 60 K-mers (1200), beside a branch of 1100
    g = S.Contigs(65); v = [g.v() for _ in range(4)]
    A = g.e(v[0], v[1], 2000); vs = [v[1]] + [g.v() for _ in range(19)] + [v[2]]
    chain = [g.e(vs[i], vs[i + 1], 60) for i in range(20)]; r = g.e(v[1], v[2], 1100); B = g.e(v[2], v[3], 2000)
    for i, e in enumerate(chain):
        g.pair([e], [e ^ 1], 1 + i % 3)
    g.pair(chain[:5], [chain[7] ^ 1], 2)
    X = [[[A]], [chain, [r]], [[B]]]
    c = g.case(lines=[X, S.mirror_line(X)])
    c["expect"] = dict(group_pairs_head=[sum(1 + i % 3 for i in range(20)) + 2, 0])
    out["group_of_20"] = c
    # ---- 1, 255, 256 and 257 groups: that many bubbles of two long branches
    # (the mirror edges get lines of one edge each from the builder: no cell, no group)
    for n in (1, 255, 256, 257):
        g = S.Contigs(70 + n % 7); lines = []; pairs = []
        for i in range((n + 1) // 2):
            two = 2 * i + 1 < n                                   # the last bubble of an odd n has one branch of 999: one group
            a, b, cc, line = bubble_line(g, [1000 + i % 5, 1100 if two else 999], 1000)
            SF.through(g, a, b[0], cc, 1 + i % 3)
            if two:
                g.pair([b[1][0]], [], i % 2)
            pairs += [1 + i % 3] + ([i % 2] if two else [])
            lines.append(line)
        c = g.case(lines=lines)
        c["expect"] = dict(n_groups=n, group_pairs=pairs)
        out[f"groups_{n}"] = c
    # ---- empty paths and empty cells: x[0].empty() (a gap cell) skips the cell
    g = S.Contigs(66); a, b = g.contig(1500), g.contig(1500)
    g.pair([a], [a ^ 1], 4)
    X = [[[a]], [[]], [[b]]]
    c = g.case(lines=[X, S.mirror_line(X)])
    c["expect"] = dict(n_cells=2, n_cells_empty=2, n_groups=0)
    out["gap_cell"] = c
    # ---- the inf and NaN texts of .lines.stats: pairs only on a line below min_len (a NaN prints as ` cov=?x`: the record step7_cov_no_pairs)
    g = S.Contigs(67); a = lone(g, 3000, 0); b = lone(g, 1200, 5); cc = lone(g, 2000, 0)
    c = g.case()
    c["expect"] = dict(base_cov=0.0, stats="line[0] 0..0 len=3000 npairs=0 cov=?x\nline[1] 1..1 len=3000 npairs=0 cov=?x\nline[2] 2..2 len=1200 npairs=5 cov=infx\nline[3] 3..3 len=1200 npairs=5 cov=infx\n"
                       "line[4] 4..4 len=2000 npairs=0 cov=?x\nline[5] 5..5 len=2000 npairs=0 cov=?x\n", n_undefined=4)
    out["inf_and_nan"] = c
    # ---- 21 candidates: ten contigs and one line that is its own mirror image (an edge with inv[e] == e): on the other side of size > 20
    for n in (20, 21):
        g = S.Contigs(68)
        for i in range(10):
            lone(g, 1200 + 50 * i, 10 + i)
        if n == 21:
            e = g.contig(1300); g.pair([e], [e], 12)
        c = g.case()
        if n == 21:                                               # (the builder's copy of e is its own mirror too; no pair names it: no candidate)
            c["inv"] = c["inv"].copy(); c["inv"][e] = e; c["inv"][e ^ 1] = e ^ 1
        c["expect"] = dict(n_candidates=n, **({"n_simple": 0} if n == 20 else {}))
        out[f"candidates_{n}"] = c
    # ---- the prefilter at 5x: 60 contigs around c and 60 around 6.5c, each cluster dense enough for a peak of its own; the far one is
    # above 5x the largest-mass peak and goes, the one that is left is a single peak
    rng = np.random.default_rng(69); g = S.Contigs(69)
    for kmers, n in _peak_specs(rng, 60, 0.03, 0.05) + _peak_specs(rng, 60, 0.195, 0.05):
        lone(g, kmers, n)
    c = g.case()
    c["expect"] = dict(n_prefiltered=1, n_peaks=1, peak_way=1)
    out["prefilter_5x"] = c
    return out


# ---------------------------------------------------------------------------------------------------------------- checks
def as_dict(res):
    """a step7.Coverage as the model's dict"""
    a = res.arrays
    groups = [dict(line=int(a["group_line"][g]), cell=int(a["group_cell"][g]), len=int(a["group_len"][g]), pairs=int(a["group_pairs"][g]), z=a["group_z"][g]) for g in range(len(a["group_line"]))]
    counters = {k: v for k, v in res.counters.items() if k not in ("n_candidates", "n_groups", "n_cn_edges", "n_cn_good", "n_group_entries", "index_built")}
    return dict(npairs=a["npairs"].tolist(), llens=a["llens"].tolist(), covl=a["covl"].tolist(), covx=a["covx"].tolist(), mass=a["mass"].tolist(), ids=a["ids"].tolist(),
                base_cov=res.base_cov, max_len=res.max_len, min_len=res.min_len, cov=a["cov"], rule=a["rule"].tolist(), groups=groups, n_cn_edges=res.counters["n_cn_edges"],
                n_cn_good=res.counters["n_cn_good"], cn_fraction=res.cn_fraction, counters=counters)


def bits32(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def bits64(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def compare(got, want):
    """a result of the library against the model's: array for array, bit for bit, counter for counter"""
    for k in ("npairs", "llens", "mass", "ids", "rule", "groups", "max_len", "min_len", "n_cn_edges", "n_cn_good"):
        assert got[k] == want[k], k
    for k in ("covl", "covx"):
        assert bits64(got[k]) == bits64(want[k]), k
    assert bits64([got["base_cov"]]) == bits64([want["base_cov"]]), "base_cov"
    assert bits64([got["cn_fraction"]]) == bits64([want["cn_fraction"]]), "cn_fraction"
    assert bits32(got["cov"]) == bits32(want["cov"]), "cov"
    assert got["counters"] == want["counters"], {k: (got["counters"].get(k), want["counters"].get(k)) for k in want["counters"] if got["counters"].get(k) != want["counters"].get(k)}


def check_expect(case, got):
    """holds a result (the model's dict, or as_dict of the library's) to the literal outcomes of a model-only case"""
    for k, v in case["expect"].items():
        if k == "base_cov":
            assert got["base_cov"] == v, (k, got["base_cov"])
        elif k == "rule":
            assert {e: M.RULES[got["rule"][e]] for e in v} == v, (k, {e: M.RULES[got["rule"][e]] for e in v})
        elif k == "cov":
            assert {e: float(got["cov"][e]) for e in v} == {e: float(np.float32(x)) for e, x in v.items()}, (k, {e: float(got["cov"][e]) for e in v})
        elif k == "n_groups":
            assert v is None or len(got["groups"]) == v, (k, len(got["groups"]))
        elif k == "group_pairs":
            assert [g["pairs"] for g in got["groups"]] == v, (k, [g["pairs"] for g in got["groups"]])
        elif k == "group_pairs_head":
            assert [g["pairs"] for g in got["groups"]][:len(v)] == v, (k, [g["pairs"] for g in got["groups"]])
        elif k == "long_pairs":                                   # the long-edge rule: cov = float(pairs / Kmers / base_cov)
            for e, n in v.items():
                assert got["rule"][e] == 3, (k, e, got["rule"][e])
                assert bits32([got["cov"][e]]) == bits32([M._over_base(M._div(float(n), float(M.kmers(case["hbv"], e))), got["base_cov"], M.RECIP["long"])]), (k, e)
        elif k == "stats":
            assert M.line_stats_text(got, case["nested"]) == v, k
        elif k == "n_candidates":
            assert len(got["covx"]) == v, (k, len(got["covx"]))
        else:
            assert got["counters"][k] == v, (k, got["counters"][k])

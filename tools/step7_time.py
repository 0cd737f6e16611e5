"""Times Step 7's read-sized passes (w2rap_step7_links: the pairs of every line, MakeGaps up to its accepted gaps) on a GENERATED workload
and prints one JSON line.

    python tools/step7_time.py [--contigs 20000] [--reads 4000000] [--seed 7] [--span 0.1] [--unplaced 0.02] [--calls 7]

The workload, stated here because nothing else defines it: --contigs isolated contigs of 3,000 to 12,000 K-mers (K = 200, seeded), each
with its mirror image, every edge a line of its own -- a graph as Step 6 leaves a genome that assembled into contigs without branches;
--reads / 2 read pairs, each on a seeded contig i: --span of them with read 1 on contig i and read 2 on the mirror of contig i + 1 (a pair
that spans to the neighbour: the near (i, i + 1)), --unplaced of them with a mate that has no path, the others with both mates on contig i
(no near).  One edge per path.  npairs is counted in the same call (part LINES) and read by LINKS.  The call runs --calls times in this
process; per call the wall time, the per-part device milliseconds and the per-kernel lines of w2rap_step7_profile.  Nothing is compared:
the reference cannot time these passages alone, and no speed is claimed against it.

    python tools/step7_time.py --line_files [--contigs 20000] [--reads 4000000] [--seed 7] [--calls 7]

times w2rap_step7_line_files (DumpLineFiles: a.lines.fasta, .efasta, .src) instead, on the same contigs with RANDOM BASES: every tenth
contig is a -> {b1, b2} -> c, a bubble of 250 and 260 K-mers in its middle whose branches share the (K-1)-mers of their vertices, one line
of three cells; the others stay one-edge lines; every line is followed by its mirror image (which is not printed).  The read pairs lie
on a seeded contig: on a bubble contig read 1 walks a, one of the branches (seeded, 3 in 4 the second) and c, read 2 lies on the mirror
of c; elsewhere one edge each.  Per call the wall time, the per-part device milliseconds, the per-kernel lines of
w2rap_step7_line_files_profile and the writer's rate: (text written + a quarter of it read as packed bases) / the time of the two
k7f_write kernels -- counted as NOTES counts kg_seg_write's 1.08 TB/s, the only comparison there is: one kernel of ours beside another
of ours, not against the reference, which cannot time this passage alone.

    python tools/step7_time.py --coverage [--contigs 20000] [--reads 4000000] [--seed 7] [--span 0.1] [--unplaced 0.02] [--calls 7]

times w2rap_step7_coverage (ComputeCoverage and CNIntegerFraction) on the contigs of the first workload with their pairs (lengths only,
as there), and: every tenth contig a is followed by a bubble whose two branches are 1,200 K-mers and a closing edge c of 1,000 -- one
line a -> {b1, b2} -> c, so the cell rule runs: two classes per line --; every twentieth instead by a cell whose two paths share a first
edge of 1,200 K-mers, a -> {[p, q1], [p, q2]} -> c with q1 and q2 of 40 and 45 -- no class is formed and p is left to the long-edge rule.
Every line is followed by its mirror image.  Read 1 of a pair on such a contig walks a, one of the two paths (seeded) and c, read 2 lies
on the mirror of c (or, for --span of the pairs, of the next contig's first edge); --unplaced as above.  Per call the wall time, the
per-part device milliseconds and the per-kernel lines of w2rap_step7_profile.  The calls take the two forms of the long edges' count in
turn (sorted, sort-free, sorted, ...): ms_long is the device time of that round alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from w2rap_contigger_amd import formats as F, step7  # noqa: E402

K = 200


def workload(n_contigs, n_reads, seed, span, unplaced):
    rng = np.random.default_rng(seed)
    E, NV = 2 * n_contigs, 4 * n_contigs
    kmers = rng.integers(3000, 12001, n_contigs)
    edge_len = np.repeat(kmers + K - 1, 2).astype(np.uint32)
    # contig i: edge 2i from vertex 4i to 4i + 2, its mirror 2i + 1 from 4i + 3 to 4i + 1
    v = np.arange(NV)
    from_off = np.zeros(NV + 1, np.uint64); np.cumsum(np.isin(v % 4, (0, 3)), out=from_off[1:])
    to_off = np.zeros(NV + 1, np.uint64); np.cumsum(np.isin(v % 4, (2, 1)), out=to_off[1:])
    i = np.arange(n_contigs)
    from_v = np.stack([4 * i + 2, 4 * i + 1], 1).reshape(-1).astype(np.int32)      # vertices 4i, 4i + 3 in order
    from_e = np.stack([2 * i, 2 * i + 1], 1).reshape(-1).astype(np.int32)
    to_e = np.stack([2 * i + 1, 2 * i], 1).reshape(-1).astype(np.int32)            # vertices 4i + 1, 4i + 2 in order
    bo = np.zeros(E + 1, np.uint64); np.cumsum((edge_len.astype(np.uint64) + 3) // 4, out=bo[1:])
    hbv = F.HBV(K, from_off, from_v, from_e, to_off, to_e, np.zeros(int(bo[-1]), np.uint8), bo, edge_len)
    inv = (np.arange(E) ^ 1).astype(np.int32)
    e = np.arange(E + 1, dtype=np.uint64)
    lines = F.Lines(e, e.copy(), e.copy(), np.arange(E, dtype=np.int32))
    NP = n_reads // 2
    c = rng.integers(0, n_contigs - 1, NP)
    kind = rng.random(NP)
    r1 = 2 * c
    r2 = np.where(kind < span, 2 * (c + 1) + 1, 2 * c + 1)
    has1 = ~((kind >= span) & (kind < span + unplaced / 2)); has2 = ~((kind >= span + unplaced / 2) & (kind < span + unplaced))
    plen = np.stack([has1, has2], 1).reshape(-1)
    path_off = np.zeros(2 * NP + 1, np.uint64); np.cumsum(plen, out=path_off[1:])
    edges = np.stack([r1, r2], 1).reshape(-1)[plen].astype(np.int32)
    return hbv, inv, (np.zeros(2 * NP, np.int32), path_off, edges), lines


def workload_line_files(n_contigs, n_reads, seed):
    rng = np.random.default_rng(seed)
    kmers = rng.integers(3000, 12001, n_contigs)
    ends, seqs, nested, walks = [], [], [], []             # (u, v) of every edge, its bases; vertex v has the mirror v ^ 1, edge e the mirror e ^ 1
    nv = 0

    def edge(u, v, s):
        ends.append((u, v)); ends.append((v ^ 1, u ^ 1)); seqs.append(s); seqs.append((3 - s[::-1]).astype(np.uint8))
        return len(ends) - 2
    for i in range(n_contigs):
        k = int(kmers[i])
        if i % 10:
            e = edge(nv, nv + 2, rng.integers(0, 4, k + K - 1).astype(np.uint8)); nv += 4
            nested += [[[[e]]], [[[e ^ 1]]]]; walks.append(([e], [e ^ 1]))
            continue
        ka = k // 2
        sa, sc = rng.integers(0, 4, ka + K - 1).astype(np.uint8), rng.integers(0, 4, k - ka + K - 1).astype(np.uint8)
        j1, j2 = sa[-(K - 1):], sc[:K - 1]
        a = edge(nv, nv + 2, sa); b1 = edge(nv + 2, nv + 4, np.concatenate([j1, rng.integers(0, 4, 250 - K + 1).astype(np.uint8), j2]))
        b2 = edge(nv + 2, nv + 4, np.concatenate([j1, rng.integers(0, 4, 260 - K + 1).astype(np.uint8), j2])); c = edge(nv + 4, nv + 6, sc); nv += 8
        line = [[[a]], [[b1], [b2]], [[c]]]
        nested += [line, [[[c ^ 1]], [[b1 ^ 1], [b2 ^ 1]], [[a ^ 1]]]]
        walks.append(([a, b1, c], [a, b2, c], [c ^ 1]))
    E = len(ends)
    u, v = np.array(ends).T
    fo = np.argsort(u, kind="stable"); fo = fo[np.argsort(v[fo], kind="stable")]; fo = fo[np.argsort(u[fo], kind="stable")]      # by (vertex, target), ties in edge order
    to = np.argsort(v, kind="stable")
    from_off = np.zeros(nv + 1, np.uint64); np.cumsum(np.bincount(u, minlength=nv), out=from_off[1:])
    to_off = np.zeros(nv + 1, np.uint64); np.cumsum(np.bincount(v, minlength=nv), out=to_off[1:])
    off = np.zeros(E + 1, np.uint64); np.cumsum([len(s) for s in seqs], out=off[1:])
    pk, bo, ln = F.pack_bases(np.concatenate(seqs), off)
    hbv = F.HBV(K, from_off, v[fo].astype(np.int32), fo.astype(np.int32), to_off, to.astype(np.int32), pk, bo, ln)
    NP = n_reads // 2
    where, second = rng.integers(0, n_contigs, NP), rng.random(NP) < 0.75
    flat = []
    for w, s2 in zip(where.tolist(), second.tolist()):
        t = walks[w]
        flat += [t[0], t[1]] if len(t) == 2 else [t[1] if s2 else t[0], t[2]]
    path_off = np.zeros(2 * NP + 1, np.uint64); np.cumsum([len(p) for p in flat], out=path_off[1:])
    edges = np.fromiter((e for p in flat for e in p), np.int32, int(path_off[-1]))
    return hbv, (np.arange(E) ^ 1).astype(np.int32), (np.zeros(2 * NP, np.int32), path_off, edges), F.Lines.from_nested(nested)


def workload_coverage(n_contigs, n_reads, seed, span, unplaced):
    rng = np.random.default_rng(seed)
    kmers = rng.integers(3000, 12001, n_contigs)
    lens, nested = [], []                                   # K-mers of every edge (e and its mirror e ^ 1); the lines
    W = np.full((n_contigs, 2, 4), -1, np.int64)            # read 1's walk on contig i, either variant
    first, last = np.zeros(n_contigs, np.int64), np.zeros(n_contigs, np.int64)

    def edge(k):
        lens.extend((k, k))
        return len(lens) - 2
    for i in range(n_contigs):
        a = edge(int(kmers[i]))
        first[i] = a
        if i % 10:
            nested += [[[[a]]], [[[a ^ 1]]]]; W[i, :, 0] = a; last[i] = a
            continue
        if i % 20:
            b1, b2, c = edge(1200), edge(1200), edge(1000)
            line = [[[a]], [[b1], [b2]], [[c]]]
            W[i, 0, :3] = (a, b1, c); W[i, 1, :3] = (a, b2, c)
        else:
            p, q1, q2, c = edge(1200), edge(40), edge(45), edge(1000)
            line = [[[a]], [[p, q1], [p, q2]], [[c]]]
            W[i, 0] = (a, p, q1, c); W[i, 1] = (a, p, q2, c)
        nested += [line, [[[e ^ 1 for e in reversed(path)] for path in cell] for cell in reversed(line)]]
        last[i] = c
    E = len(lens)
    edge_len = (np.array(lens) + K - 1).astype(np.uint32)
    bo = np.zeros(E + 1, np.uint64); np.cumsum((edge_len.astype(np.uint64) + 3) // 4, out=bo[1:])
    z = np.zeros(1, np.uint64)
    hbv = F.HBV(K, z, np.zeros(0, np.int32), np.zeros(0, np.int32), z.copy(), np.zeros(0, np.int32), np.zeros(0, np.uint8), bo, edge_len)      # (the call reads K and the lengths only)
    NP = n_reads // 2
    c = rng.integers(0, n_contigs - 1, NP)
    kind, variant = rng.random(NP), rng.integers(0, 2, NP)
    r1 = W[c, variant]                                       # [NP, 4]
    r2 = np.where(kind < span, first[c + 1] ^ 1, last[c] ^ 1)
    has1 = ~((kind >= span) & (kind < span + unplaced / 2)); has2 = ~((kind >= span + unplaced / 2) & (kind < span + unplaced))
    both = np.concatenate([r1, r2[:, None], np.full((NP, 3), -1, np.int64)], 1).reshape(2 * NP, 4)       # row 2p: read 1, row 2p + 1: read 2
    both[0::2][~has1] = -1; both[1::2][~has2] = -1
    keep = both >= 0
    path_off = np.zeros(2 * NP + 1, np.uint64); np.cumsum(keep.sum(1), out=path_off[1:])
    return hbv, (np.arange(E) ^ 1).astype(np.int32), (np.zeros(2 * NP, np.int32), path_off, both[keep].astype(np.int32)), F.Lines.from_nested(nested)


def main_coverage(a):
    hbv, inv, paths, lines = workload_coverage(a.contigs, a.reads, a.seed, a.span, a.unplaced)
    walls, parts, kernels, forms = [], [], [], []
    for i in range(max(1, a.calls)):                        # the two forms of the long edges' count in turn (ms_long is their round, inside ms_groups)
        forms.append(("sorted", "sort_free")[i % 2])
        t0 = time.perf_counter()
        res = step7.coverage(hbv, inv, paths, lines, long_form=forms[-1])
        walls.append(round(time.perf_counter() - t0, 4))
        parts.append({k: round(v, 4) for k, v in res.ms.items()})
        kernels.append({k: [round(v[0], 4), v[1]] for k, v in step7.profile().items()})
        print(f"call {len(walls)} ({forms[-1]}): wall {walls[-1]:.4f} s, device {sum(v for k, v in res.ms.items() if k != 'ms_long'):.3f} ms, long edges {res.ms['ms_long']:.4f} ms", file=sys.stderr)
    out = {"workload": f"generated (tools/step7_time.py --coverage): {a.contigs} contigs of 3,000-12,000 K-mers, every tenth followed by a bubble of two 1,200-K-mer branches, every "
                       f"twentieth by a cell whose two paths share a first edge of 1,200 K-mers, every line followed by its mirror image, {a.reads} reads, {a.span:g} of the pairs span "
                       f"to the neighbour contig, {a.unplaced:g} have a mate without a path (seed {a.seed})",
           "entry": "w2rap_step7_coverage", "parts": "npairs+peak+edges", "edge_objects": int(len(hbv.edge_len)), "lines": int(lines.n_lines), "reads": int(len(paths[0])),
           "path_entries": int(paths[1][-1]), "base_cov": res.base_cov, "cn_fraction": res.cn_fraction, "counters": res.counters, "wall_s_calls": walls, "ms_parts_calls": parts,
           "ms_device_sum_calls": [round(sum(v for k, v in p.items() if k != "ms_long"), 3) for p in parts], "kernels_calls": kernels,
           "long_form_calls": forms, "ms_long_calls": [p["ms_long"] for p in parts]}
    print(json.dumps(out))


def main_line_files(a):
    hbv, inv, paths, lines = workload_line_files(a.contigs, a.reads, a.seed)
    walls, parts, kernels, rates = [], [], [], []
    for _ in range(max(1, a.calls)):
        t0 = time.perf_counter()
        res = step7.line_files(hbv, inv, paths, lines)
        walls.append(round(time.perf_counter() - t0, 4))
        parts.append({k: round(v, 3) for k, v in res.ms.items()})
        prof = step7.profile(line_files=True)
        kernels.append({k: [round(v[0], 4), v[1]] for k, v in prof.items()})
        text = len(res.fasta) + len(res.efasta)
        ms = prof["k7f_write_fasta"][0] + prof["k7f_write_efasta"][0]
        rates.append(round((text + text / 4) / (ms * 1e-3) / 1e12, 4))
        print(f"call {len(walls)}: wall {walls[-1]:.4f} s, device {sum(res.ms.values()):.3f} ms, writer {rates[-1]:.3f} TB/s", file=sys.stderr)
    out = {"workload": f"generated (tools/step7_time.py --line_files): {a.contigs} contigs of 3,000-12,000 K-mers with random bases, every tenth with a two-branch bubble (250 and 260 "
                       f"K-mers) in its middle, every line followed by its mirror image, {a.reads} reads, on a bubble contig read 1 through a branch (seed {a.seed})",
           "entry": "w2rap_step7_line_files", "parts": "fasta+efasta+src", "edge_objects": int(hbv.n_edges), "lines": int(lines.n_lines), "reads": int(len(paths[0])),
           "path_entries": int(paths[1][-1]), "fasta_bytes": len(res.fasta), "efasta_bytes": len(res.efasta), "src_bytes": len(res.src), "counters": res.counters,
           "wall_s_calls": walls, "ms_parts_calls": parts, "ms_device_sum_calls": [round(sum(p.values()), 3) for p in parts], "kernels_calls": kernels,
           "writer_TB_per_s_calls": rates, "writer_rate_is": "(text bytes written + text bytes / 4 read as packed bases) / (k7f_write_fasta + k7f_write_efasta time)",
           "kg_seg_write_TB_per_s_NOTES": 1.08}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--line_files", action="store_true", help="time w2rap_step7_line_files instead")
    ap.add_argument("--coverage", action="store_true", help="time w2rap_step7_coverage instead")
    ap.add_argument("--contigs", type=int, default=20_000)
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--span", type=float, default=0.1)
    ap.add_argument("--unplaced", type=float, default=0.02)
    ap.add_argument("--calls", type=int, default=7)
    a = ap.parse_args()
    if a.line_files:
        return main_line_files(a)
    if a.coverage:
        return main_coverage(a)
    hbv, inv, paths, lines = workload(a.contigs, a.reads, a.seed, a.span, a.unplaced)
    walls, parts, kernels = [], [], []
    for _ in range(max(1, a.calls)):
        t0 = time.perf_counter()
        res = step7.find_gaps(hbv, inv, paths, lines)
        walls.append(round(time.perf_counter() - t0, 4))
        parts.append({k: round(v, 3) for k, v in res.ms.items()})
        kernels.append({k: [round(v[0], 4), v[1]] for k, v in step7.profile().items()})
        print(f"call {len(walls)}: wall {walls[-1]:.4f} s, device {sum(res.ms.values()):.3f} ms", file=sys.stderr)
    out = {"workload": f"generated (tools/step7_time.py): {a.contigs} isolated contigs of 3,000-12,000 K-mers as one-edge lines, {a.reads} reads, {a.span:g} of the pairs span to the "
                       f"neighbour contig, {a.unplaced:g} have a mate without a path (seed {a.seed})",
           "entry": "w2rap_step7_links", "parts": "lines+links", "edge_objects": int(hbv.n_edges), "lines": int(lines.n_lines), "reads": int(len(paths[0])),
           "path_entries": int(paths[1][-1]), "counters": res.counters, "wall_s_calls": walls, "ms_parts_calls": parts,
           "ms_device_sum_calls": [round(sum(p.values()), 3) for p in parts], "kernels_calls": kernels}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

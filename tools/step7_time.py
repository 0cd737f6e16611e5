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
of ours, not against the reference, which cannot time this passage alone."""
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
    ap.add_argument("--contigs", type=int, default=20_000)
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--span", type=float, default=0.1)
    ap.add_argument("--unplaced", type=float, default=0.02)
    ap.add_argument("--calls", type=int, default=7)
    a = ap.parse_args()
    if a.line_files:
        return main_line_files(a)
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

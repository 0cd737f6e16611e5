"""Times Step 7's read-sized passes (w2rap_step7_links: the pairs of every line, MakeGaps up to its accepted gaps) on a GENERATED workload
and prints one JSON line.

    python tools/step7_time.py [--contigs 20000] [--reads 4000000] [--seed 7] [--span 0.1] [--unplaced 0.02] [--calls 7]

The workload, stated here because nothing else defines it: --contigs isolated contigs of 3,000 to 12,000 K-mers (K = 200, seeded), each
with its mirror image, every edge a line of its own -- a graph as Step 6 leaves a genome that assembled into contigs without branches;
--reads / 2 read pairs, each on a seeded contig i: --span of them with read 1 on contig i and read 2 on the mirror of contig i + 1 (a pair
that spans to the neighbour: the near (i, i + 1)), --unplaced of them with a mate that has no path, the others with both mates on contig i
(no near).  One edge per path.  npairs is counted in the same call (part LINES) and read by LINKS.  The call runs --calls times in this
process; per call the wall time, the per-part device milliseconds and the per-kernel lines of w2rap_step7_profile.  Nothing is compared:
the reference cannot time these passages alone, and no speed is claimed against it."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=20_000)
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--span", type=float, default=0.1)
    ap.add_argument("--unplaced", type=float, default=0.02)
    ap.add_argument("--calls", type=int, default=7)
    a = ap.parse_args()
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

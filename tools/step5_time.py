"""Times the tail of Step 5 (PartnersToEnds, w2rap_step5_partners_to_ends) or, with --opening, its opening (w2rap_step5_open: the paths
index, Unsat's links, LayoutReads) or, with --add, AddNewStuff (w2rap_step5_add_new_stuff) on the planted workload and prints one JSON line.

    python tools/step5_time.py [--reads 4000000] [--seed 77] [--min_freq 4] [--blank 0.02] [--blank_seed 1] [--calls 7] [--opening | --add]

The reads go through Steps 2, 3 and 4 of this library (the workload of tools/step4_time.py); then a seeded fraction of the reads have
their paths set to zero length, no edges, offset 0, and the call runs --calls times in this process.  Per call: the wall time and the
per-phase device milliseconds; of the last call: the per-kernel lines of w2rap_step5_profile and the counters.  Nothing is compared:
the reference cannot run this function alone.  --opening: the call takes the graph, its involution and ALL paths as Step 4 leaves them
(nothing is blanked); per call the wall time, the per-part device milliseconds and the per-kernel lines.  Nothing in the reference
isolates those passages for a timed comparison either.  --add: the graph, ALL paths, the reads and their qualities as Step 4 leaves them;
new_stuff = a seeded --patches (1000) pieces of 400 bases cut from the genome across dead ends of the graph (200 bases of an edge that
ends in a sink and the 200 bases the genome goes on with); per call the wall time, the per-phase device milliseconds and the per-kernel
lines.  The reference cannot run AddNewStuff alone either: nothing is compared."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from w2rap_contigger_amd import formats as F, step2, step3, step4, step5, synth  # noqa: E402


def time_opening(a, r4, ln):
    paths = (r4.path_offset, r4.path_off, r4.path_edges)
    walls, parts, kernels = [], [], []
    for _ in range(max(1, a.calls)):
        t0 = time.perf_counter()
        res = step5.opening(r4.hbv, r4.inv, paths, ln)
        walls.append(round(time.perf_counter() - t0, 4))
        parts.append({k: round(v, 3) for k, v in res.ms.items()})
        kernels.append({k: [round(v[0], 4), v[1]] for k, v in step5.profile().items()})
        print(f"call {len(walls)}: wall {walls[-1]:.4f} s, device {sum(res.ms.values()):.3f} ms", file=sys.stderr)
    out = {"workload": f"bench.planted_reads({a.reads}, {a.seed}) through Steps 2-4, graph, involution and all paths as Step 4 leaves them",
           "entry": "w2rap_step5_open", "min_freq": a.min_freq, "edge_objects": int(r4.hbv.n_edges), "reads": int(len(ln)), "path_entries": int(r4.path_off[-1]),
           "counters": res.counters, "wall_s_calls": walls, "ms_parts_calls": parts, "ms_device_sum_calls": [round(sum(p.values()), 3) for p in parts],
           "kernels_calls": kernels}
    print(json.dumps(out))


def planted_genome(n_reads, seed):
    """the first haplotype of bench.planted_reads(n_reads, seed): the same draws in the same order"""
    rng = np.random.default_rng(seed)
    G = n_reads * 5 // 2
    g = rng.integers(0, 4, G, dtype=np.uint8)
    fams = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(500, 5001, 40)]
    for k in range(2000):
        f = fams[k % len(fams)]
        at = int(rng.integers(1000, G - 6000))
        g[at:at + len(f)] = (3 - f[::-1]) if k % 3 == 0 else f
    return g


def dead_end_patches(hbv, g, n_patches, seed, W=32, half=200):
    """pieces of 2 * half bases of the genome g centred where an edge that ends in a sink ends, found by the edge's last W bases"""
    codes, off = hbv.edge_codes()
    off = off.astype(np.int64)
    tl, tr = hbv.to_left_right()
    outdeg = np.diff(hbv.from_off.astype(np.int64))
    sinks = np.nonzero(outdeg[tr] == 0)[0]
    key = np.zeros(len(g) - W + 1, np.uint64)
    for i in range(W):
        key = (key << np.uint64(2)) | g[i:len(g) - W + 1 + i].astype(np.uint64)
    order = np.argsort(key, kind="stable"); skey = key[order]
    rng = np.random.default_rng(seed)
    pieces = []
    for e in rng.permutation(sinks):
        last = codes[off[e + 1] - W:off[e + 1]]
        for w, fwd in ((last, True), ((3 - last[::-1]).astype(np.uint8), False)):
            k = np.uint64(0)
            for b in w:
                k = (k << np.uint64(2)) | np.uint64(b)
            j = int(np.searchsorted(skey, k))
            if j < len(skey) and skey[j] == k:
                c = int(order[j]) + (W if fwd else 0)              # where the edge ends in the genome
                if half <= c <= len(g) - half:
                    pieces.append(g[c - half:c + half].copy())
                break
        if len(pieces) == n_patches:
            break
    return pieces, int(len(sinks))


def time_add(a, r4, reads, quals, off):
    g = planted_genome(a.reads, a.seed)
    pieces, n_sinks = dead_end_patches(r4.hbv, g, a.patches, a.patch_seed)
    poff = np.zeros(len(pieces) + 1, np.uint64); np.cumsum([len(p) for p in pieces], out=poff[1:])
    new = F.pack_bases(np.concatenate(pieces) if pieces else np.zeros(0, np.uint8), poff)
    paths = (r4.path_offset, r4.path_off, r4.path_edges)
    walls, phases, kernels = [], [], []
    for _ in range(max(1, a.calls)):
        t0 = time.perf_counter()
        res = step5.add_new_stuff(r4.hbv, paths, reads, quals, new, qual_off=off)
        walls.append(round(time.perf_counter() - t0, 4))
        phases.append({k: round(v, 3) for k, v in res.ms.items()})
        kernels.append({k: [round(v[0], 4), v[1]] for k, v in step5.profile().items()})
        print(f"call {len(walls)}: wall {walls[-1]:.4f} s, device {sum(res.ms.values()):.3f} ms", file=sys.stderr)
    out = {"workload": f"bench.planted_reads({a.reads}, {a.seed}) through Steps 2-4, graph, all paths, reads and qualities as Step 4 leaves them; new_stuff = "
                       f"{len(pieces)} pieces of 400 bases of the genome across dead ends (seed {a.patch_seed}; the graph has {n_sinks} edges that end in a sink)",
           "entry": "w2rap_step5_add_new_stuff", "min_freq": a.min_freq, "edge_objects": int(r4.hbv.n_edges), "reads": int(len(reads[2])), "patches": len(pieces),
           "new_edge_objects": int(res.hbv.n_edges), "counters": res.counters, "wall_s_calls": walls, "ms_phases_calls": phases,
           "ms_device_sum_calls": [round(sum(p.values()), 3) for p in phases], "kernels_calls": kernels}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--min_freq", type=int, default=4)
    ap.add_argument("--blank", type=float, default=0.02)
    ap.add_argument("--blank_seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--opening", action="store_true", help="time w2rap_step5_open instead of PartnersToEnds")
    ap.add_argument("--add", action="store_true", help="time w2rap_step5_add_new_stuff instead of PartnersToEnds")
    ap.add_argument("--patches", type=int, default=1000, help="--add: pieces of new_stuff")
    ap.add_argument("--patch_seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    d = bench.planted_reads(a.reads, a.seed, torch.device("cuda", 0))
    torch.cuda.synchronize()
    codes = synth.unpack_fixed(d["packed"], synth.READ_LEN).cpu().numpy().reshape(-1)
    quals = d["quals"].cpu().numpy().reshape(-1)
    off = np.arange(d["n"] + 1, dtype=np.uint64) * synth.READ_LEN
    del d
    torch.cuda.empty_cache()
    pk, bo, ln = F.pack_bases(codes, off)
    r2 = step2.build_read_qgraph(pk, bo, ln, quals=quals, qual_off=off, min_freq=a.min_freq)
    r3 = step3.repath_in_memory(r2.hbv, (r2.path_offset, r2.path_off, r2.path_edges), 200)
    r4 = step4.clean200x(r3.hbv, (r3.path_offset, r3.path_off, r3.path_edges), pk, bo, ln, quals, off, inv=r3.inv2)
    n = len(ln)
    if a.opening:
        return time_opening(a, r4, ln)
    if a.add:
        return time_add(a, r4, (pk, bo, ln), quals, off)
    blank = np.random.default_rng(a.blank_seed).random(n) < a.blank
    po = r4.path_off.astype(np.int64)
    plen = np.diff(po); plen[blank] = 0
    npo = np.zeros(n + 1, np.uint64); np.cumsum(plen, out=npo[1:])
    offset = r4.path_offset.copy(); offset[blank] = 0
    paths = (offset, npo, r4.path_edges[np.repeat(~blank, np.diff(po))])
    walls, phases = [], []
    for _ in range(max(1, a.calls)):
        t0 = time.perf_counter()
        res = step5.partners_to_ends(r4.hbv, paths, (pk, bo, ln), quals, qual_off=off)
        walls.append(round(time.perf_counter() - t0, 4))
        phases.append({k: round(v, 3) for k, v in res.ms.items()})
        print(f"call {len(walls)}: wall {walls[-1]:.4f} s, device {sum(res.ms.values()):.3f} ms", file=sys.stderr)
    out = {"workload": f"bench.planted_reads({a.reads}, {a.seed}) through Steps 2-4, paths of {a.blank:g} of the reads (seed {a.blank_seed}) blanked",
           "entry": "w2rap_step5_partners_to_ends", "min_freq": a.min_freq, "edge_objects": int(r4.hbv.n_edges), "reads": int(n), "reads_blanked": int(blank.sum()),
           "counters": res.counters, "wall_s_calls": walls, "ms_phases_calls": phases, "ms_device_sum_calls": [round(sum(p.values()), 3) for p in phases],
           "kernels_last_call": {k: [round(v[0], 4), v[1]] for k, v in step5.profile().items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Times the tail of Step 5 (PartnersToEnds, w2rap_step5_partners_to_ends) or, with --opening, its opening (w2rap_step5_open: the paths
index, Unsat's links, LayoutReads) on the planted workload and prints one JSON line.

    python tools/step5_time.py [--reads 4000000] [--seed 77] [--min_freq 4] [--blank 0.02] [--blank_seed 1] [--calls 7] [--opening]

The reads go through Steps 2, 3 and 4 of this library (the workload of tools/step4_time.py); then a seeded fraction of the reads have
their paths set to zero length, no edges, offset 0, and the call runs --calls times in this process.  Per call: the wall time and the
per-phase device milliseconds; of the last call: the per-kernel lines of w2rap_step5_profile and the counters.  Nothing is compared:
the reference cannot run this function alone.  --opening: the call takes the graph, its involution and ALL paths as Step 4 leaves them
(nothing is blanked); per call the wall time, the per-part device milliseconds and the per-kernel lines.  Nothing in the reference
isolates those passages for a timed comparison either."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--min_freq", type=int, default=4)
    ap.add_argument("--blank", type=float, default=0.02)
    ap.add_argument("--blank_seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--opening", action="store_true", help="time w2rap_step5_open instead of PartnersToEnds")
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

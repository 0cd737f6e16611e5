"""Times Step 4 (Clean200x) behind Steps 2 and 3 on the planted workload and prints one JSON line.

    python tools/step4_time.py [--reads 4000000] [--seed 77] [--min_freq 4] [--min_size 0] [--repeats 3] [--reference] [--host_edit] [--chained]

Per pass: ms_index, ms_vote, ms_paths (device events) and ms_graph_edit_host (host clock, NOT device time); ms_k4e_sum, the device
time of the graph edit's kernels (the k4e_* lines of the profile, both passes; 0 with --host_edit); placements per second of the
scoring kernel; the per-kernel table of w2rap_step4_profile; the scoring kernel's bytes per second, loaded (mostly from L2) and compulsory
(against the 8 TB/s HBM roof).  The figures are
those of the LAST of --repeats runs (the first ones warm the context's memory pool).  --reference: the wall time of the reference's
own Step 4 (oracle/_ref/w2rap-contigger-gpu --from_step 4 --to_step 4) on the same files, with a same-output verdict.
--chained: the same workload through the device-resident hand-over.  The reads go once into a Step2Context; every repeat runs count,
graph, paths, Step 3 with keep_on_device and no fetch, then step4.clean200x_after_step3; wall_s_call is that last call alone."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from w2rap_contigger_amd import formats as F, step2, step3, step4, synth  # noqa: E402

HBM_ROOF = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--min_freq", type=int, default=4)
    ap.add_argument("--min_size", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--host_edit", action="store_true", help="edit the graph on the host (W2RAP_STEP4_EDIT_ON_HOST)")
    ap.add_argument("--chained", action="store_true", help="Step 4 behind Step 3 in HBM (w2rap_step2_run_step4_after_step3), not on host arrays")
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
    edit = "host" if a.host_edit else "device"
    ctx = None
    if a.chained:
        if a.reference:
            ap.error("--reference needs the large-K files, which --chained never brings down")
        ctx = step2.Step2Context(0)
        ctx.set_reads_host(pk, bo, ln, quals=quals, qual_off=off)
    else:
        r2 = step2.build_read_qgraph(pk, bo, ln, quals=quals, qual_off=off, min_freq=a.min_freq)
        r3 = step3.repath_in_memory(r2.hbv, (r2.path_offset, r2.path_off, r2.path_edges), 200)
        paths = (r3.path_offset, r3.path_off, r3.path_edges)
    walls, k4e = [], []
    for _ in range(max(1, a.repeats)):
        if a.chained:
            ctx.count_kmers(7, a.min_freq); ctx.build_graph(None); ctx.path_reads()
            r3 = step3.repath_after_step2(ctx, 200, fetch=False, keep_on_device=True)
        t0 = time.perf_counter()
        if a.chained:
            r4 = step4.clean200x_after_step3(ctx, min_size=a.min_size, edit=edit)
        else:
            r4 = step4.clean200x(r3.hbv, paths, pk, bo, ln, quals, off, min_size=a.min_size, inv=r3.inv2, edit=edit)
        wall = time.perf_counter() - t0
        walls.append(round(wall, 4))
        k4e.append(round(sum(v[0] for k, v in step4.profile().items() if k.startswith("k4e_")), 4))
        print(f"call {len(walls)}: wall {wall:.4f} s, k4e_* {k4e[-1]:.4f} ms", file=sys.stderr)
    if ctx is not None:
        ctx.close()
    prof = step4.profile()
    edit_path = prof.pop("edit_path_device", (0.0, 0))
    score_ms = prof.get("k4_score", (0.0, 0))[0]
    L = 250 + 200 - 1
    # Two byte counts for k4_score over both passes.  LOADED: what its threads ask for -- per scored position 16 B of walk table, 1 B of quality,
    # 1/4 B of bases, + the 16-B placement and the 8-B result; the table rows are shared by a vertex's placements and are served by L2, so
    # this figure is NOT HBM traffic.  COMPULSORY: what must come from HBM at least once per pass -- placements and results, every read's
    # bases and qualities once, every vertex's table once; this is the figure to hold against the HBM roof.
    n_reads = len(ln)
    bytes_loaded = r4.n_placements * (synth.READ_LEN * (16 + 1 + 0.25) + 24)
    bytes_compulsory = r4.n_placements * 24 + 2 * n_reads * synth.READ_LEN * 1.25 + r4.n_branch_vertices * ((L + 3) // 4 * 4) * 16
    out = {"workload": f"bench.planted_reads({a.reads}, {a.seed})", "entry": "w2rap_step2_run_step4_after_step3" if a.chained else "w2rap_step4_run", "min_freq": a.min_freq, "min_size": a.min_size, "walk_positions": L,
           "large_K_edge_objects_in": int(r3.n_edge_objs), "edge_objects_out": int(r4.hbv.n_edges),
           "n_branch_vertices": r4.n_branch_vertices, "n_skipped_too_many_exts": r4.n_skipped_too_many_exts, "n_placements": r4.n_placements,
           "n_deleted": list(r4.n_deleted), "n_runs_merged": list(r4.n_runs_merged),
           "ms_index": [round(x, 3) for x in r4.ms_index], "ms_vote": [round(x, 3) for x in r4.ms_vote], "ms_paths": [round(x, 3) for x in r4.ms_paths],
           "ms_graph_edit_host": [round(x, 3) for x in r4.ms_graph_edit_host], "wall_s_call": round(wall, 4),
           "wall_s_calls": walls, "ms_k4e_sum": k4e[-1], "ms_k4e_sum_calls": k4e, "edit_on_device": bool(r4.edit_on_device),
           "edit_passes_on_device": int(edit_path[1]),
           "placements_per_s_k4_score": round(r4.n_placements / (score_ms * 1e-3), 1) if score_ms else None,
           "k4_score_loaded_bytes_per_s_mostly_L2": round(bytes_loaded / (score_ms * 1e-3), 1) if score_ms else None,
           "k4_score_compulsory_hbm_bytes_per_s": round(bytes_compulsory / (score_ms * 1e-3), 1) if score_ms else None,
           "k4_score_compulsory_fraction_of_8TBps": round(bytes_compulsory / (score_ms * 1e-3) / HBM_ROOF, 5) if score_ms else None,
           "kernels": {k: [round(v[0], 4), v[1]] for k, v in prof.items()}}
    if a.reference:
        exe = os.path.join(ROOT, "oracle", "_ref", "w2rap-contigger-gpu")
        with tempfile.TemporaryDirectory() as t:
            F.write_hbv(os.path.join(t, "t.large_K.hbv"), r3.hbv); F.write_paths(os.path.join(t, "t.large_K.paths"), *paths)
            F.write_fastb(os.path.join(t, "frag_reads_orig.fastb"), pk, bo, ln); F.write_qualp(os.path.join(t, "frag_reads_orig.qualp"), quals, off)
            t0 = time.perf_counter()
            subprocess.run([exe, "-r", "x", "-o", t, "-p", "t", "-t", "16", "-m", "64", "--from_step", "4", "--to_step", "4", "-s", str(a.min_size)], check=True, stdout=subprocess.DEVNULL)
            out["reference_wall_s_with_file_io"] = round(time.perf_counter() - t0, 3)
            ref = F.read_hbv(os.path.join(t, "t.large_K.clean.hbv"))
            out["same_output_as_reference"] = bool(F.hbv_to_bytes(ref, zero_padding=True) == F.hbv_to_bytes(r4.hbv, zero_padding=True) and
                                                   open(os.path.join(t, "t.large_K.clean.paths"), "rb").read() == F.paths_to_bytes(r4.path_offset, r4.path_off, r4.path_edges))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

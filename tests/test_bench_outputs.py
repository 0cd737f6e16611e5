"""bench.py --dump-outputs: the files it writes for a Step-2 result (host logic, no GPU) and, on the GPU, a plain run's line and outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from w2rap_contigger_amd import formats as F, step2


def golden_result(name):
    """a Step2Result made of the reference's own files of a golden fixture (the arrays the library does not write get stand-ins)"""
    h = F.read_hbv(os.path.join(GOLDEN, f"{name}.ref.hbv"))
    offset, po, edges = F.read_paths(os.path.join(GOLDEN, f"{name}.ref.paths"))
    ne = h.n_edges
    left, right = h.to_left_right()
    return step2.Step2Result(h, left, right, right.copy(), np.arange(ne, dtype=np.int32), np.arange(ne, dtype=np.int32)[::-1].copy(),
                             offset, po, edges, np.arange(101, dtype=np.uint64), 123, 45, 6, len(offset), 0, 1.0, 2.0, 3.0)


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    res = golden_result("random20k")
    bench.dump_outputs(str(tmp_path), res)
    got = load_dir(tmp_path)
    assert len(got) == 18 and all(x.dtype == np.float64 for x in got.values())
    assert np.array_equal(got["path_edges"], res.path_edges) and np.array_equal(got["path_off"], res.path_off)
    assert np.array_equal(got["hbv_edge_packed"], res.hbv.edge_packed) and np.array_equal(got["hbv_from_e"], res.hbv.from_e)
    assert np.array_equal(got["hist"], res.hist) and list(got["counts"]) == [123, 45, 6, len(res.path_offset), 0]


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    res = golden_result("repeats_snps")
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    a, b = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    pe = a["path_edges"]
    assert len(res.path_edges) > 1000 and len(pe) == 1000
    # the sample keeps the order of the array: a subsequence of it
    it = iter(res.path_edges.astype(np.float64))
    assert all(any(v == w for w in it) for v in pe)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20


@pytest.mark.gpu
def test_plain_bench_line_and_outputs(tmp_path):
    """a plain run: the line's keys, --steps obeyed, nothing from --full; two runs with the same arguments write the same outputs,
    and the outputs' statistics are the line's"""
    def run(d):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--reads", "2e6",
               "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        return json.loads(lines[0])
    r1 = run(tmp_path / "a")
    r2 = run(tmp_path / "b")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r1, k
    assert r1["metric"] == "step2_k60_canonical_kmers_per_s" and r1["steps"] == 2 and r1["ms_per_step"] > 0
    assert not {"cpu_baseline", "extras", "planted_workload", "host_resident"} & r1.keys()
    assert "measured_copy_GBs" not in r1["roofline"] and r1["roofline"].get("not_overlapped") is None
    a, b = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert len(a) == 18 and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    c = r1["config"]
    assert list(a["counts"][:4]) == [c["kmer_instances"], c["kmers_distinct"], c["kmers_solid"], c["reads_pathed"]]
    assert r2["config"] == c

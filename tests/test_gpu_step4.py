"""Step 4 (Clean200x) on the GPU: byte equality with recorded runs of the unmodified reference, per-pass deleted lists and counters
against the CPU model (tests/step4_model.py, itself pinned to the reference by test_step4_model.py), hand-made graphs for the quirks,
and the pipeline / tool round trips.  No comparison has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import step4_cases as S
import step4_model as M
from conftest import ROOT, planted_reads
from w2rap_contigger_amd import formats as F, pipeline, step2, step3, step4

pytestmark = pytest.mark.gpu


def _same(res, m, vote_only=False):
    assert F.hbv_to_bytes(res.hbv, zero_padding=True) == F.hbv_to_bytes(m.hbv, zero_padding=True), "graph differs from the model"
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(m.path_offset, m.path_off, m.path_edges), "paths differ"
    assert np.array_equal(res.inv, m.inv)
    assert [list(x) for x in res.deleted] == m.deleted
    c = m.counters
    assert (res.n_branch_vertices, res.n_skipped_too_many_exts, res.n_placements) == (c.n_branch_vertices, c.n_skipped_too_many_exts, c.n_placements)
    k = 1 if vote_only else 2
    assert list(res.n_deleted[:k]) == c.n_deleted
    if not vote_only:
        assert list(res.n_runs_merged) == c.n_runs_merged


@pytest.mark.parametrize("name,min_size", S.CASES)
def test_equals_the_recorded_reference(name, min_size, tmp_path):
    d = str(tmp_path)
    S.reference_run(name, min_size, d)
    h, paths, (pk, bo, ln), quals = S.load(name)
    res = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=min_size)
    assert F.hbv_to_bytes(res.hbv, zero_padding=True) == F.hbv_to_bytes(F.read_hbv(os.path.join(d, "t.large_K.clean.hbv")), zero_padding=True)
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == open(os.path.join(d, "t.large_K.clean.paths"), "rb").read()
    _same(res, M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), min_size))


@pytest.mark.parametrize("name", ["long_mixed", "errs2"])
def test_vote_only(name):
    h, paths, (pk, bo, ln), quals = S.load(name)
    res = step4.clean200x(h, paths, pk, bo, ln, quals, vote_only=True)
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), 0, vote_only=True)
    assert len(m.deleted) == 1 and len(m.deleted[0]) > 0
    _same(res, m, vote_only=True)
    assert F.hbv_to_bytes(res.hbv, zero_padding=True) == F.hbv_to_bytes(h, zero_padding=True)
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(*paths)


@pytest.mark.parametrize("name", sorted(S.hand_cases()))
def test_hand_made_quirks(name):
    h, paths, (pk, bo, ln), quals, ms = S.hand_cases()[name]
    res = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms)
    _same(res, M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms))


def test_given_involution_equals_computed():
    h, paths, (pk, bo, ln), quals = S.load("errs2")
    inv = M.involution(M.Graph.from_hbv(h))
    a = step4.clean200x(h, paths, pk, bo, ln, quals, inv=np.array(inv, np.int32))
    b = step4.clean200x(h, paths, pk, bo, ln, quals)
    assert F.hbv_to_bytes(a.hbv) == F.hbv_to_bytes(b.hbv) and np.array_equal(a.path_edges, b.path_edges)


@pytest.mark.parametrize("n_reads,seed,min_freq,min_size", [(40_000, 5, 2, 0), (60_000, 6, 1, 500)])
def test_against_the_model_on_generated_reads(n_reads, seed, min_freq, min_size):
    """Steps 2 and 3 of this library on the planted workload with sequencing errors (canonical Step-3 edge order), then Step 4 against the model"""
    r = planted_reads(n_reads, seed)
    r2 = step2.build_read_qgraph(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"], min_freq=min_freq)
    r3 = step3.repath_in_memory(r2.hbv, (r2.path_offset, r2.path_off, r2.path_edges), 200)
    paths = (r3.path_offset, r3.path_off, r3.path_edges)
    res = step4.clean200x(r3.hbv, paths, r["pk"], r["bo"], r["ln"], r["quals"], min_size=min_size, inv=r3.inv2)
    m = M.clean200x(r3.hbv, r3.inv2, paths, M.Reads(r["codes"], r["quals"], r["off"].astype(np.int64)), min_size)
    print(f"generated {n_reads}: {r3.hbv.n_edges} edges, deleted {m.counters.n_deleted}, merged {m.counters.n_runs_merged}, placements {m.counters.n_placements}")
    _same(res, m)
    assert step4.profile().get("k4_score", (0, 0))[1] >= 1


def test_pipeline_and_tool(tmp_path):
    G = os.path.join(ROOT, "tests", "golden")
    reads = f"{G}/step1_r1.fastq,{G}/step1_r2.fastq"
    a, b, c = (str(tmp_path / x) for x in "abc")
    assert pipeline.main(["-r", reads, "-o", a, "-p", "t", "--min_freq", "2", "--from_step", "1", "--to_step", "4", "-s", "300", "--dump_all", "1"]) == 0
    assert pipeline.main(["-r", reads, "-o", b, "-p", "t", "--min_freq", "2", "--from_step", "1", "--to_step", "3"]) == 0
    assert pipeline.main(["-o", b, "-p", "t", "--from_step", "4", "--to_step", "4", "-s", "300"]) == 0
    rd = lambda d, f: open(os.path.join(d, f), "rb").read()
    for f in ("t.large_K.hbv", "t.large_K.paths", "t.large_K.clean.hbv", "t.large_K.clean.paths"):
        assert rd(a, f) == rd(b, f), f
    os.makedirs(c)
    for f in ("t.large_K.hbv", "t.large_K.paths", "frag_reads_orig.fastb", "frag_reads_orig.qualp"):
        open(os.path.join(c, f), "wb").write(rd(b, f))
    r = subprocess.run([os.path.join(ROOT, "w2rap_contigger_amd", "w2rap-step4"), "-o", c, "-p", "t", "-s", "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for f in ("t.large_K.clean.hbv", "t.large_K.clean.paths"):
        assert rd(c, f) == rd(b, f), f
    # without --dump_all a run that ends at step 4 does not write the large-K files (w2rap-contigger.cc:373: dump_all || to_step == 3)
    e = str(tmp_path / "e")
    assert pipeline.main(["-r", reads, "-o", e, "-p", "t", "--min_freq", "2", "--to_step", "4", "-s", "300"]) == 0
    assert not os.path.exists(os.path.join(e, "t.large_K.hbv")) and rd(e, "t.large_K.clean.hbv") == rd(b, "t.large_K.clean.hbv")
    assert pipeline.main(["-r", reads, "-o", e, "-p", "t", "--to_step", "5"]) == 1

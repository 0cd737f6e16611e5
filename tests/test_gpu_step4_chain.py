"""Step 4 behind Step 3 in HBM (w2rap_step2_run_step4_after_step3 on the large-K result that W2RAP_STEP3_KEEP_DEVICE leaves in a Step-2
context): the chained call against the host-array call on the fetched Step-3 result and against the CPU model (tests/step4_model.py),
the lifetime of the kept result, the context's device bytes from round to round, and the pipeline.  Every comparison is exact.

The issue's second check -- the chained result against the recorded reference runs refruns/step4_errs2_s0 / _s300 -- is left out: it
presupposes that Steps 2 and 3 reproduce the golden step4_errs2.large_K.* from these reads, and on the CPU the oracles (oracle.run at
min_freq 2, oracle3 with the edge order of step4_errs2.large_K.hbv) reproduce the graph but not the paths (same offsets, same number
of entries, some entries on another edge: the reference's small-K pathing breaks ties by ITS arbitrary small-K edge numbering, which
the fixture does not record).  The recorded runs stay covered by test_gpu_step4.py on the golden large-K files themselves."""
import os

import numpy as np
import pytest

import step4_model as M
from conftest import GOLDEN, planted_reads
from w2rap_contigger_amd import formats as F, pipeline, step2, step3, step4

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = 1, 4
_MEMO = {}


def _errs2():
    """step4_errs2: 4,800 reads, the smallest input of the repository on which the vote deletes edges and runs merge"""
    if "errs2" not in _MEMO:
        pk, bo, ln = F.read_fastb(os.path.join(GOLDEN, "step4_errs2.fastb"))
        pq, po = F.read_qualp(os.path.join(GOLDEN, "step4_errs2.qualp"))
        _MEMO["errs2"] = dict(pk=pk, bo=bo, ln=ln, pq=pq, po=po, quals=F.qualp_to_raw(pq, po)[0])
    return _MEMO["errs2"]


def _errs2_ctx(ctx):
    r = _errs2()
    ctx.set_reads_host(r["pk"], r["bo"], r["ln"], pq=r["pq"], pq_off=r["po"])
    ctx.count_kmers(7, 2); ctx.build_graph(None); ctx.path_reads()
    return r


def _paths(x):
    return (x.path_offset, x.path_off, x.path_edges)


def _same(a, b, what, vote_only=False):
    """a Step4Result against another one"""
    assert F.hbv_to_bytes(a.hbv, zero_padding=True) == F.hbv_to_bytes(b.hbv, zero_padding=True), f"graph differs from {what}"
    assert F.paths_to_bytes(*_paths(a)) == F.paths_to_bytes(*_paths(b)), f"paths differ from {what}"
    assert np.array_equal(a.inv, b.inv), what
    assert [list(x) for x in a.deleted] == [list(x) for x in b.deleted], what
    assert tuple(a.n_deleted) == tuple(b.n_deleted), what
    if not vote_only:
        assert tuple(a.n_runs_merged) == tuple(b.n_runs_merged), what
    assert (a.n_branch_vertices, a.n_skipped_too_many_exts, a.n_placements) == (b.n_branch_vertices, b.n_skipped_too_many_exts, b.n_placements), what


def _same_model(a, m):
    assert F.hbv_to_bytes(a.hbv, zero_padding=True) == F.hbv_to_bytes(m.hbv, zero_padding=True), "graph differs from the model"
    assert F.paths_to_bytes(*_paths(a)) == F.paths_to_bytes(*_paths(m)), "paths differ from the model"
    assert np.array_equal(a.inv, m.inv)
    assert [list(x) for x in a.deleted] == m.deleted
    c = m.counters
    assert list(a.n_deleted) == c.n_deleted and list(a.n_runs_merged) == c.n_runs_merged
    assert (a.n_branch_vertices, a.n_skipped_too_many_exts, a.n_placements) == (c.n_branch_vertices, c.n_skipped_too_many_exts, c.n_placements)


@pytest.mark.parametrize("min_size", [0, 300])
def test_chained_equals_unchained_and_model_on_the_vote_fixture(min_size):
    with step2.Step2Context(0) as ctx:
        r = _errs2_ctx(ctx)
        r3 = step3.repath_after_step2(ctx, 200, keep_on_device=True)
        res = step4.clean200x_after_step3(ctx, min_size=min_size)
    assert r3.n_edge_objs == r3.hbv.n_edges and r3.n_vertices == r3.hbv.n_vertices
    assert res.edit_on_device and sum(res.n_deleted) > 0 and sum(res.n_runs_merged) > 0
    un = step4.clean200x(r3.hbv, _paths(r3), r["pk"], r["bo"], r["ln"], r["quals"], min_size=min_size, inv=r3.inv2)
    _same(res, un, "the host-array call")
    _same_model(res, M.clean200x(r3.hbv, r3.inv2, _paths(r3), M.reads_of(r["pk"], r["bo"], r["ln"], r["quals"]), min_size))


def test_planted_reads_with_errors_device_and_host_edit():
    """the parameters of test_gpu_step4.test_against_the_model_on_generated_reads; raw qualities, not PQVec blobs"""
    r = planted_reads(40_000, 5)
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"])
        ctx.count_kmers(7, 2); ctx.build_graph(None); ctx.path_reads()
        r3 = step3.repath_after_step2(ctx, 200, keep_on_device=True)
        dev = step4.clean200x_after_step3(ctx)
        assert step4.profile().get("k4_score", (0, 0))[1] >= 1
        step3.repath_after_step2(ctx, 200, keep_on_device=True, fetch=False)
        hst = step4.clean200x_after_step3(ctx, edit="host")
    assert dev.edit_on_device and not hst.edit_on_device
    un = step4.clean200x(r3.hbv, _paths(r3), r["pk"], r["bo"], r["ln"], r["quals"], inv=r3.inv2)
    _same(dev, un, "the host-array call")
    _same(hst, dev, "the chained call with the device edit")
    _same_model(dev, M.clean200x(r3.hbv, r3.inv2, _paths(r3), M.Reads(r["codes"], r["quals"], r["off"].astype(np.int64)), 0))


def test_lifetime_of_the_kept_result():
    def state_error(ctx):
        with pytest.raises(step2.Step2Error) as e:
            step4.clean200x_after_step3(ctx)
        assert e.value.code == E_STATE and "Step 3" in str(e.value), str(e.value)

    with step2.Step2Context(0) as ctx:
        r = _errs2_ctx(ctx)
        state_error(ctx)                                           # nothing kept yet
        plain = step3.repath_after_step2(ctx, 200)
        state_error(ctx)                                           # a Step 3 without the flag keeps nothing
        f0 = ctx.fetch()
        with pytest.raises(step2.Step2Error) as e:
            step3.repath_after_step2(ctx, 200, keep_on_device=True, places_only=True)
        assert e.value.code == E_ARG
        with pytest.raises(step2.Step2Error) as e:
            step3.repath_in_memory(f0.hbv, _paths(f0), 200, keep_on_device=True)
        assert e.value.code == E_ARG
        r3 = step3.repath_after_step2(ctx, 200, keep_on_device=True)
        vote = step4.clean200x_after_step3(ctx, vote_only=True)   # edits nothing, consumes nothing
        assert not vote.edit_on_device and len(vote.deleted) == 1 and len(vote.deleted[0]) > 0
        assert F.hbv_to_bytes(vote.hbv, zero_padding=True) == F.hbv_to_bytes(r3.hbv, zero_padding=True)
        assert F.paths_to_bytes(*_paths(vote)) == F.paths_to_bytes(*_paths(r3)) and np.array_equal(vote.inv, r3.inv2)
        full = step4.clean200x_after_step3(ctx)
        assert list(full.deleted[0]) == list(vote.deleted[0]) and full.edit_on_device
        state_error(ctx)                                           # the full run has consumed it
        # the Step-2 state is intact: fetch and a plain Step 3 give what they gave before
        f1 = ctx.fetch()
        assert F.hbv_to_bytes(f1.hbv) == F.hbv_to_bytes(f0.hbv) and F.paths_to_bytes(*_paths(f1)) == F.paths_to_bytes(*_paths(f0))
        again = step3.repath_after_step2(ctx, 200)
        assert F.hbv_to_bytes(again.hbv) == F.hbv_to_bytes(plain.hbv) and F.paths_to_bytes(*_paths(again)) == F.paths_to_bytes(*_paths(plain))
        assert np.array_equal(again.inv2, plain.inv2) and np.array_equal(again.frag_count, plain.frag_count)
        # keep, then a new count: what the result was derived from is gone, and so is the result
        step3.repath_after_step2(ctx, 200, keep_on_device=True, fetch=False)
        ctx.count_kmers(7, 2)
        state_error(ctx)
        ctx.build_graph(None); ctx.path_reads()
        # keep, then a Step 3 without the flag
        step3.repath_after_step2(ctx, 200, keep_on_device=True, fetch=False)
        step3.repath_after_step2(ctx, 200)
        state_error(ctx)
        # and the full result once more on the rebuilt state, against the host-array call
        r3b = step3.repath_after_step2(ctx, 200, keep_on_device=True)
        last = step4.clean200x_after_step3(ctx, min_size=300)
    assert F.hbv_to_bytes(r3b.hbv) == F.hbv_to_bytes(r3.hbv)
    _same(last, step4.clean200x(r3.hbv, _paths(r3), r["pk"], r["bo"], r["ln"], r["quals"], min_size=300, inv=r3.inv2), "the host-array call")


@pytest.mark.parametrize("consume", [True, False])
def test_no_device_bytes_leak_from_round_to_round(consume):
    """count, graph, paths, Step 3 with keep, then the chained Step 4 (or nothing: a kept result nobody consumes): the peak of the context's
    live device bytes is the same in round 3 as in round 2, and what is live at the end of a round is what the reads and Step 2 hold"""
    with step2.Step2Context(0) as ctx:
        r = _errs2()
        ctx.set_reads_host(r["pk"], r["bo"], r["ln"], pq=r["pq"], pq_off=r["po"])
        peaks, live = [], []
        for _ in range(3):
            ctx.count_kmers(7, 2); ctx.build_graph(None); ctx.path_reads()
            before = ctx.device_bytes()
            step3.repath_after_step2(ctx, 200, keep_on_device=True, fetch=False)
            assert ctx.device_bytes() > before                     # the kept result is live ...
            if consume:
                step4.clean200x_after_step3(ctx, min_size=300)
                assert ctx.device_bytes() == before                # ... and gone, with everything the call allocated
            peaks.append(ctx.device_peak_bytes(reset=True))
            live.append(ctx.device_bytes())
        assert peaks[1] == peaks[2] and live[1] == live[2], (peaks, live)


def test_pipeline_hands_over_in_hbm(tmp_path, monkeypatch):
    reads = f"{GOLDEN}/step1_r1.fastq,{GOLDEN}/step1_r2.fastq"
    a, b, c = (str(tmp_path / x) for x in "abc")
    rd = lambda d, f: open(os.path.join(d, f), "rb").read()
    assert pipeline.main(["-r", reads, "-o", b, "-p", "t", "--min_freq", "2", "--from_step", "1", "--to_step", "3"]) == 0
    assert pipeline.main(["-o", b, "-p", "t", "--from_step", "4", "--to_step", "4", "-s", "300"]) == 0

    def forbidden(*args, **kw):
        raise AssertionError("a run from step 1 to step 4 read the reads back from disk or unpacked their qualities on the host")
    with monkeypatch.context() as mp:
        mp.setattr(F, "qualp_to_raw", forbidden)
        mp.setattr(F, "read_fastb", forbidden)
        lines = []
        out = pipeline.run(reads, a, "t", min_freq=2, to_step=4, min_size=300, log=lines.append)
        assert pipeline.main(["-r", reads, "-o", c, "-p", "t", "--min_freq", "2", "--to_step", "4", "-s", "300", "--dump_all", "1"]) == 0
    assert out["step4"].edit_on_device
    n_large = F.read_hbv(os.path.join(b, "t.large_K.hbv")).n_edges
    assert any(l.startswith("Repathing to second graph DONE:") and l.endswith(f" {n_large} large-K edge objects") for l in lines), lines
    for f in ("t.large_K.clean.hbv", "t.large_K.clean.paths", "t.first.frags.dist", "small_K.freqs", "frag_reads_orig.fastb", "frag_reads_orig.qualp"):
        assert rd(a, f) == rd(b, f) == rd(c, f), f
    assert not os.path.exists(os.path.join(a, "t.large_K.hbv"))    # w2rap-contigger.cc:373: dump_all || to_step == 3
    for f in ("t.large_K.hbv", "t.large_K.paths"):
        assert rd(c, f) == rd(b, f), f

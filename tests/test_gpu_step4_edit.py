"""Step 4's graph edit on the GPU (the k4e_* kernels): byte equality with the recorded runs of the unmodified reference, equality with the
library's host edit in everything it returns, and the CPU model (tests/step4_model.py) as the judge on hand-made graphs, one rule of the
reference's numbering each (tests/step4_edit_cases.py); the same graphs under the numbering of a real graph (random vertex and edge ids,
both tie orders), counts on the edges of a block and of a sort tile, members of one k-mer, a pass that deletes every edge, and an inv
that mirrors no run onto a run.  test_step4_edit_model.py proves on the CPU what each of those inputs exercises.  No comparison has a
tolerance."""
import os

import numpy as np
import pytest

import step4_cases as S
import step4_edit_cases as EC
import step4_model as M
from conftest import planted_reads
from w2rap_contigger_amd import formats as F, step2, step3, step4

pytestmark = pytest.mark.gpu


def _k4e():
    return {k: v for k, v in step4.profile().items() if k.startswith("k4e_")}


def _same(res, m, vote_only=False):
    assert F.hbv_to_bytes(res.hbv, zero_padding=True) == F.hbv_to_bytes(m.hbv, zero_padding=True), "graph differs from the model"
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(m.path_offset, m.path_off, m.path_edges), "paths differ"
    assert np.array_equal(res.inv, m.inv)
    assert [list(x) for x in res.deleted] == m.deleted
    c = m.counters
    assert (res.n_branch_vertices, res.n_skipped_too_many_exts, res.n_placements) == (c.n_branch_vertices, c.n_skipped_too_many_exts, c.n_placements)
    assert list(res.n_deleted[:1 if vote_only else 2]) == c.n_deleted
    if not vote_only:
        assert list(res.n_runs_merged) == c.n_runs_merged


def _same_results(a, b):
    """everything two runs of the library return, but the timings"""
    assert F.hbv_to_bytes(a.hbv) == F.hbv_to_bytes(b.hbv), "graph bytes differ"
    assert F.paths_to_bytes(a.path_offset, a.path_off, a.path_edges) == F.paths_to_bytes(b.path_offset, b.path_off, b.path_edges), "paths differ"
    for f in ("vleft", "vright", "to_v", "inv"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert [list(x) for x in a.deleted] == [list(x) for x in b.deleted]
    for f in ("n_deleted", "n_runs_merged", "n_branch_vertices", "n_skipped_too_many_exts", "n_placements"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("name,min_size", S.CASES)
def test_device_edit_equals_the_recorded_reference_and_the_host_edit(name, min_size, tmp_path):
    d = str(tmp_path)
    S.reference_run(name, min_size, d)
    h, paths, (pk, bo, ln), quals = S.load(name)
    dev = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=min_size, edit="device")
    k4e = _k4e()
    assert dev.edit_on_device is True and k4e and all(v[1] >= 1 for v in k4e.values()), k4e
    assert F.hbv_to_bytes(dev.hbv, zero_padding=True) == F.hbv_to_bytes(F.read_hbv(os.path.join(d, "t.large_K.clean.hbv")), zero_padding=True)
    assert F.paths_to_bytes(dev.path_offset, dev.path_off, dev.path_edges) == open(os.path.join(d, "t.large_K.clean.paths"), "rb").read()
    host = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=min_size, edit="host")
    assert host.edit_on_device is False and not _k4e()
    _same_results(dev, host)


@pytest.mark.parametrize("name", sorted(S.hand_cases()))
def test_existing_hand_made_graphs_on_the_device(name):
    h, paths, (pk, bo, ln), quals, ms = S.hand_cases()[name]
    res = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert res.edit_on_device is True
    _same(res, M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms))


_EDIT_CASES = EC.edit_cases()


@pytest.mark.parametrize("name", sorted(_EDIT_CASES))
def test_edit_rules_on_both_paths(name):
    h, paths, (pk, bo, ln), quals, ms = _EDIT_CASES[name].inputs
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)
    dev = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert dev.edit_on_device is (not _EDIT_CASES[name].expect.get("unsorted", False))
    _same(dev, m)
    host = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="host")
    assert host.edit_on_device is False
    _same(host, m)
    _same_results(dev, host)


def test_generated_reads_device_host_model():
    """Steps 2 and 3 of this library on the planted workload with sequencing errors, then Step 4: device edit == host edit == model"""
    r = planted_reads(40_000, 5)
    r2 = step2.build_read_qgraph(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"], min_freq=2)
    r3 = step3.repath_in_memory(r2.hbv, (r2.path_offset, r2.path_off, r2.path_edges), 200)
    paths = (r3.path_offset, r3.path_off, r3.path_edges)
    dev = step4.clean200x(r3.hbv, paths, r["pk"], r["bo"], r["ln"], r["quals"], inv=r3.inv2, edit="device")
    assert dev.edit_on_device is True and _k4e()
    host = step4.clean200x(r3.hbv, paths, r["pk"], r["bo"], r["ln"], r["quals"], inv=r3.inv2, edit="host")
    m = M.clean200x(r3.hbv, r3.inv2, paths, M.Reads(r["codes"], r["quals"], r["off"].astype(np.int64)), 0)
    print(f"generated: {r3.hbv.n_edges} edges, deleted {m.counters.n_deleted}, merged {m.counters.n_runs_merged}; k4e_* {sum(v[0] for v in _k4e().values()):.3f} ms")
    assert sum(m.counters.n_runs_merged) > 0
    _same(dev, m)
    _same_results(dev, host)


def _vote_only_edits_nothing(edit):
    h, paths, (pk, bo, ln), quals = S.load("errs2")
    res = step4.clean200x(h, paths, pk, bo, ln, quals, vote_only=True, edit=edit)
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), 0, vote_only=True)
    assert len(m.deleted[0]) > 0
    _same(res, m, vote_only=True)
    assert F.hbv_to_bytes(res.hbv, zero_padding=True) == F.hbv_to_bytes(h, zero_padding=True)
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(*paths)


def test_vote_only_edits_nothing_on_the_device_path():
    _vote_only_edits_nothing("device")


def test_vote_only_hands_the_input_graph_on_with_the_host_edit():
    """the editor that edits nothing returns the pass's input graph as the next one: its blocks must outlive the pass"""
    _vote_only_edits_nothing("host")


@pytest.mark.parametrize("edit", ["device", "host"])
@pytest.mark.parametrize("min_size", [0, 40])
@pytest.mark.parametrize("name", sorted(EC.empty_cases()))
def test_a_graph_without_edges_takes_the_host_edit(name, min_size, edit):
    """nothing to run a kernel on: the device edit declines, the call starts over on the host and returns the empty graph"""
    h, paths, (pk, bo, ln), quals = EC.empty_cases()[name]
    res = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=min_size, edit=edit)
    assert res.edit_on_device is False and not _k4e()
    assert (res.hbv.n_vertices, res.hbv.n_edges) == (0, 0)
    assert [list(x) for x in res.deleted] == [[], []] and res.n_deleted == (0, 0) and res.n_runs_merged == (0, 0)
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(*paths)
    _same(res, M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), min_size))


def test_the_graph_changes_without_a_read_path_to_rewrite():
    h, paths, (pk, bo, ln), quals, ms = EC.no_reads_case()
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)
    dev = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert dev.edit_on_device is True and _k4e()
    host = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="host")
    assert host.edit_on_device is False and not _k4e()
    assert list(dev.n_runs_merged) == list(host.n_runs_merged) == _EDIT_CASES["b_long_run"].expect["merged"]
    _same(dev, m)
    _same(host, m)
    _same_results(dev, host)


def test_a_call_after_a_fallback_finds_a_clean_context():
    """the restart on the host drops everything of the abandoned attempt: the next call in the process edits on the device again"""
    h, paths, (pk, bo, ln), quals, ms = _EDIT_CASES["i_unsorted_lists"].inputs
    first = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert first.edit_on_device is False and not _k4e()
    h, paths, (pk, bo, ln), quals, ms = _EDIT_CASES["a_interleaved_runs"].inputs
    second = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert second.edit_on_device is True and _k4e()
    _same(second, M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms))


# ---- real numbering, sizes, the driver's other paths (step4_edit_cases.py; each is proven on the model in test_step4_edit_model.py)
_MODELS = {}


def _model(key, inputs):
    if key not in _MODELS:
        h, paths, (pk, bo, ln), quals, ms = inputs
        _MODELS[key] = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)
        M.RUNS.clear(); M.RUN_SIZES.clear()                   # (the model's records for the CPU proofs: not read here)
    return _MODELS[key]


def _device_host_model(key, inputs):
    h, paths, (pk, bo, ln), quals, ms = inputs
    m = _model(key, inputs)
    dev = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert dev.edit_on_device is True and _k4e()
    _same(dev, m)
    host = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="host")
    assert host.edit_on_device is False
    _same(host, m)
    _same_results(dev, host)


@pytest.mark.parametrize("name", EC.size_names())
def test_counts_on_block_and_tile_edges_and_members_of_one_kmer(name):
    _device_host_model(("size", name), EC.size_case(name).inputs)


@pytest.mark.parametrize("name", sorted(EC.variant_names()))
def test_renumbered_graphs_on_both_paths(name):
    _device_host_model(("variant", name), EC.renumbered_variant(name))


def test_pass_one_deletes_every_edge():
    """pass 2 has no edge to run a kernel on: the device edit declines there, the one-shot call starts over on the host"""
    inputs = EC.all_deleted_case()
    h, paths, (pk, bo, ln), quals, ms = inputs
    m = _model("all_deleted", inputs)
    assert m.deleted == [[0, 1, 2, 3, 4, 5], []] and m.hbv.n_edges == 0
    dev = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert dev.edit_on_device is False and not _k4e()
    _same(dev, m)
    host = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="host")
    _same(host, m)
    _same_results(dev, host)


def test_pass_one_deletes_every_edge_behind_step3():
    """the chained call cannot start over (pass 1 has consumed Step 3's result): the host editor goes on at pass 2 from the empty graph on
    the device.  300 error-free reads of one random 1 kb genome: the large-K graph is isolated edges, all within min_size"""
    rng = np.random.default_rng(61)
    genome = rng.integers(0, 4, 1000).astype(np.uint8)
    codes = []
    for _ in range(300):
        at = int(rng.integers(0, 1000 - 150 + 1))
        r = genome[at:at + 150]
        codes.append((3 - r[::-1]).astype(np.uint8) if rng.random() < 0.5 else r)
    off = np.arange(301, dtype=np.uint64) * 150
    pk, bo, ln = F.pack_bases(np.concatenate(codes), off)
    quals = np.full(300 * 150, 30, np.uint8)
    paths_of = lambda x: (x.path_offset, x.path_off, x.path_edges)
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=quals, qual_off=off)
        ctx.count_kmers(7, 2); ctx.build_graph(None); ctx.path_reads()
        idle = ctx.device_bytes()
        r3 = step3.repath_after_step2(ctx, 200, keep_on_device=True)
        assert r3.hbv.n_edges > 0 and ctx.device_bytes() > idle
        ms = int(r3.hbv.edge_len.max())                              # above every edge's k-mers
        res = step4.clean200x_after_step3(ctx, min_size=ms)
        assert res.edit_on_device is False
        assert ctx.device_bytes() == idle
        # the context is as good as before: the next round edits on the device and leaves as little behind
        ctx.count_kmers(7, 2); ctx.build_graph(None); ctx.path_reads()
        assert ctx.device_bytes() == idle
        step3.repath_after_step2(ctx, 200, keep_on_device=True, fetch=False)
        nxt = step4.clean200x_after_step3(ctx)
        assert nxt.edit_on_device is True and ctx.device_bytes() == idle
    m = M.clean200x(r3.hbv, r3.inv2, paths_of(r3), M.reads_of(pk, bo, ln, quals), ms)
    assert m.deleted == [list(range(r3.hbv.n_edges)), []] and m.hbv.n_edges == 0
    _same(res, m)
    one_shot = step4.clean200x(r3.hbv, paths_of(r3), pk, bo, ln, quals, min_size=ms, inv=r3.inv2)
    assert one_shot.edit_on_device is False
    _same_results(res, one_shot)
    m0 = M.clean200x(r3.hbv, r3.inv2, paths_of(r3), M.reads_of(pk, bo, ln, quals), 0)
    _same(nxt, m0)


@pytest.mark.parametrize("edit", ["host", "device"])
@pytest.mark.parametrize("name", ["circle", "self", "swap"])
def test_an_inv_that_mirrors_no_run_onto_a_run_is_an_error(name, edit):
    """the argument check accepts it; on the device k4e_records declines, and the host edit, which walks the 'mirror run' as the reference
    does, stops at the first vertex that is not on a run (tools/step4_bad_inv.cpp is the same under the host sanitizers)"""
    h, paths, (pk, bo, ln), quals, inv = EC.bad_inv_cases()[name]
    with pytest.raises(step2.Step2Error) as e:
        step4.clean200x(h, paths, pk, bo, ln, quals, inv=inv, edit=edit)
    assert e.value.code == 6 and "inv" in str(e.value), str(e.value)
    h, paths, (pk, bo, ln), quals, ms = _EDIT_CASES["a_interleaved_runs"].inputs
    after = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert after.edit_on_device is True and _k4e()
    _same(after, _model("a_interleaved_runs", _EDIT_CASES["a_interleaved_runs"].inputs))

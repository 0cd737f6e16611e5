"""AddNewStuff on the GPU (w2rap_step5_add_new_stuff, step5.add_new_stuff / finish) against the recorded runs of the reference's own
AddNewStuff (graph, involution and paths, id for id), the recorded runs of the reference's builder, the literal outcomes of the hand-made
cases and the model (step5_add_model), array for array and counter for counter.  Records are replayed: no reference binary runs here."""
import numpy as np
import pytest

import step5_add_cases as T
import step5_add_model as M
from w2rap_contigger_amd import formats as F, step5
from w2rap_contigger_amd.step2 import Step2Error

pytestmark = pytest.mark.gpu

ALL = sorted(T.cases()) + [f"random_{s}" for s in T.SEEDS]
_MODEL = {}


def model_of(name):
    if name not in _MODEL:
        c = T.get(name)
        _MODEL[name] = M.add_new_stuff(*c.inputs(), min_gain=c.min_gain)
    return _MODEL[name]


def library(name, **kw):
    c = T.get(name)
    h, paths, reads, quals, new = c.inputs()
    return step5.add_new_stuff(h, paths, reads, quals, T.pack_seqs(new), min_gain=c.min_gain, **kw)


def same_graph(a, b):
    assert F.hbv_to_bytes(a, zero_padding=True) == F.hbv_to_bytes(b, zero_padding=True)


def same_map(res, to3, left3):
    off = res.to3[0].astype(np.int64)
    assert [[int(e) for e in res.to3[1][off[e]:off[e + 1]]] for e in range(len(off) - 1)] == to3
    assert [int(x) for x in res.left3] == left3


@pytest.mark.parametrize("name", ALL)
def test_library_equals_model_and_literals(name):
    res = library(name, keep_map=True)
    m = model_of(name)
    print(name, res.counters)
    T.get(name).check(res)
    same_graph(res.hbv, m.hbv)
    assert np.array_equal(res.inv, m.inv)
    tl, tr = m.hbv.to_left_right()
    assert np.array_equal(res.vleft, tl) and np.array_equal(res.vright, tr)
    same_map(res, m.to3, m.left3)
    assert np.array_equal(res.path_off, m.path_off)
    assert np.array_equal(res.path_edges, m.path_edges)
    assert np.array_equal(res.path_offset, m.path_offset)
    assert res.counters == m.counters
    c = res.counters
    assert c["n_tr_empty"] + c["n_tr_first"] + c["n_tr_walked"] + c["n_tr_cleared"] == len(res.path_offset)
    assert c["n_ext_tried"] == c["n_ext_too_many"] + c["n_ext_no_cover"] + c["n_ext_ambiguous"] + c["n_ext_extended"]


@pytest.mark.parametrize("name", T.RECORDED)
def test_library_equals_the_recorded_reference(name, tmp_path):
    """the recorded edge order replayed: objects, adjacency and involution are the record's, and so are to3 and left3"""
    B, (hc, ho) = T.recorded_rebuilt(name, str(tmp_path))
    res = library(name, keep_map=True, hint=F.pack_bases(hc, ho))
    same_graph(res.hbv, B.hbv)
    assert np.array_equal(res.inv, B.inv)
    same_map(res, B.to3, B.left3)
    T.get(name).check(res)


@pytest.mark.parametrize("name", T.add_recorded())
def test_library_equals_the_recorded_add_new_stuff(name, tmp_path):
    """the record's edge order replayed: the graph, the involution and every path are the reference's, id for id; without the hint they
    are the same up to the numbering; the counters are the model's"""
    from oracle import oracle as O
    from w2rap_contigger_amd import hbvtool
    rec = T.reference_add(name, str(tmp_path))
    hc, ho = O.edge_hint_from_hbv(rec.hbv)
    res = library(name, hint=F.pack_bases(hc, ho))
    same_graph(res.hbv, rec.hbv)
    assert np.array_equal(res.inv, rec.inv)
    assert np.array_equal(res.path_offset, rec.path_offset)
    assert np.array_equal(res.path_off, rec.path_off)
    assert np.array_equal(res.path_edges, rec.path_edges)
    assert res.counters == model_of(name).counters
    plain = library(name)
    ca, pa, _ = hbvtool.canonicalise(plain.hbv, (plain.path_offset, plain.path_off, plain.path_edges))
    cb, pb, _ = hbvtool.canonicalise(rec.hbv, (rec.path_offset, rec.path_off, rec.path_edges))
    same_graph(ca, cb)
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert plain.counters == res.counters


@pytest.mark.parametrize("seed", T.SEEDS)
def test_generated_cases_reach_every_counter_in_the_library(seed):
    """every branch the counters stand for is taken by the kernels themselves: judged on the library's own counters"""
    assert T.seed_conditions(library(f"random_{seed}")) == []


def test_argument_errors():
    c = T.get("gap_bridge")
    h, paths, reads, quals, new = c.inputs()
    new = T.pack_seqs(new)

    def refused(hh=h, pp=paths, **kw):
        with pytest.raises(Step2Error) as e:
            step5.add_new_stuff(hh, pp, reads, quals, new, **kw)
        assert e.value.code == 1                              # W2RAP_E_ARG
        return str(e.value)
    assert "ext_mode" in refused(ext_mode=2)
    assert "ext_mode" in refused(ext_mode=0)
    assert "min_gain" in refused(min_gain=0)
    assert "min_gain" in refused(min_gain=-3)
    import dataclasses
    assert "K must be even" in refused(hh=dataclasses.replace(h, K=79))
    assert "K must be even" in refused(hh=dataclasses.replace(h, K=14))
    assert "K must be even" in refused(hh=dataclasses.replace(h, K=642))
    assert "shorter than K" in refused(hh=dataclasses.replace(h, K=400))
    bad = (paths[0], paths[1], np.full_like(paths[2], h.n_edges))
    assert "does not exist" in refused(pp=bad)
    # an unknown flag, through the C entry itself
    import ctypes as C
    L = step5.lib()
    i, keep = step5._step5_in(h, paths, reads, quals, None)
    prm = step5.Step5AddParams(0, 5, 1, None, 2)
    o = step5.Step5AddOut(); err = C.create_string_buffer(256)
    nln = np.ascontiguousarray(new[2], np.uint32); nbo = np.ascontiguousarray(new[1], np.uint64); npk = np.ascontiguousarray(new[0], np.uint8)
    assert L.w2rap_step5_add_new_stuff(C.byref(i), len(nln), npk.ctypes.data, nbo.ctypes.data, nln.ctypes.data, C.byref(prm), C.byref(o), err, 256) == 1
    assert b"flag" in err.value


def test_second_call_in_the_same_process_and_profile():
    a = library("branch_patch")
    b = library("branch_patch")
    assert np.array_equal(a.path_edges, b.path_edges) and np.array_equal(a.path_offset, b.path_offset) and a.counters == b.counters
    same_graph(a.hbv, b.hbv)
    assert a.to3 is None and a.left3 is None
    prof = step5.profile()
    for k in ("k5a_fill", "k5a_translate", "k5a_extend", "k3_kmer_keys"):
        assert k in prof and prof[k][1] >= 1, k
    assert all(v >= 0 for v in a.ms.values()) and set(a.ms) == set(step5.ADD_PHASES)


def test_finish_is_the_two_calls():
    c = T.get("random_1")
    h, paths, reads, quals, new = c.inputs()
    new = T.pack_seqs(new)
    n = len(reads[2]) & ~1                                  # PartnersToEnds pairs read r with r ^ 1
    assert n == len(reads[2])
    f = step5.finish(h, paths, reads, quals, new)
    a = step5.add_new_stuff(h, paths, reads, quals, new)
    p = step5.partners_to_ends(a.hbv, (a.path_offset, a.path_off, a.path_edges), reads, quals)
    same_graph(f.added.hbv, a.hbv)
    assert np.array_equal(f.placed.path_off, p.path_off) and np.array_equal(f.placed.path_edges, p.path_edges) and np.array_equal(f.placed.path_offset, p.path_offset)
    assert f.placed.counters == p.counters and f.added.counters == a.counters

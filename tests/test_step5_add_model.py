"""The yardstick of AddNewStuff on the CPU: step5_add_model (a restatement of BuildAll, TranslatePaths and ExtendPath, its graph from
oracle3.run) against recorded runs of the reference's own AddNewStuff (tests/golden/refruns/step5_addref_<case>/: the whole call, or
for a case its Validate refuses TranslatePaths and ExtendPath behind the recorded builder), against recorded runs of the reference's
builder on an encoding of `allx` (step5_add_<case>/) and against the literal outcomes of the hand-made cases."""
import numpy as np
import pytest

import step5_add_cases as T
import step5_add_model as M
from w2rap_contigger_amd import formats as F, hbvtool


def run_model(name, **kw):
    c = T.get(name)
    return M.add_new_stuff(*c.inputs(), min_gain=c.min_gain, **kw)


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_model_gives_the_literal_outcomes(name):
    m = run_model(name)
    T.get(name).check(m)
    assert sum(m.counters[k] for k in ("n_tr_empty", "n_tr_first", "n_tr_walked", "n_tr_cleared")) == len(m.path_offset)


@pytest.mark.parametrize("name", T.RECORDED)
def test_builder_model_equals_the_recorded_reference(name, tmp_path):
    """oracle3.run on the encoding, the recorded edge order replayed: the graph and every old edge's path and first skip are the record's"""
    B, hint = T.recorded_rebuilt(name, str(tmp_path))
    c = T.get(name)
    mine = M.rebuild(c.h, c.new, hint)
    assert F.hbv_to_bytes(mine.hbv, zero_padding=True) == F.hbv_to_bytes(B.hbv, zero_padding=True)
    assert np.array_equal(mine.inv, B.inv)
    assert mine.to3 == B.to3 and mine.left3 == B.left3 and mine.n_unipaths == B.n_unipaths
    # and the whole call on the recorded graph gives what it gives on the model's own, up to the numbering
    a = M.add_new_stuff(*c.inputs(), min_gain=c.min_gain, rebuilt=B)
    b = run_model(name)
    c.check(a)
    _, pa, _ = hbvtool.canonicalise(a.hbv, (a.path_offset, a.path_off, a.path_edges))
    _, pb, _ = hbvtool.canonicalise(b.hbv, (b.path_offset, b.path_off, b.path_edges))
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert a.counters == b.counters


def seq_paths(h, path_off, path_edges):
    seqs = [x.tobytes() for x in M.edge_seqs(h)]
    pf = np.asarray(path_off, np.int64)
    return [[seqs[int(e)] for e in path_edges[pf[i]:pf[i + 1]]] for i in range(len(pf) - 1)]


@pytest.mark.parametrize("name", T.add_recorded())
def test_model_equals_the_recorded_add_new_stuff(name, tmp_path):
    """the model against the reference's own call, numbering aside: graph, involution, every read's offset and its path in sequences;
    and the record itself gives the case's literals"""
    rec = T.reference_add(name, str(tmp_path))
    c = T.get(name)
    m = M.add_new_stuff(*c.inputs(), min_gain=c.min_gain, rebuilt=rec.rebuilt) if name in T.TAIL_ONLY else run_model(name)
    ca, _, _ = hbvtool.canonicalise(rec.hbv)
    cb, _, _ = hbvtool.canonicalise(m.hbv)
    assert F.hbv_to_bytes(ca, zero_padding=True) == F.hbv_to_bytes(cb, zero_padding=True)
    assert np.array_equal(rec.inv, T.involution(rec.hbv)) and np.array_equal(m.inv, T.involution(m.hbv))
    assert len(rec.path_offset) == len(c.reads)
    assert np.array_equal(rec.path_offset, m.path_offset)
    assert seq_paths(rec.hbv, rec.path_off, rec.path_edges) == seq_paths(m.hbv, m.path_off, m.path_edges)
    rec.counters = m.counters
    c.check(rec)


def test_every_case_has_a_recorded_add_new_stuff():
    """nothing but what NOT_ADD_RECORDED names, with its reason, is left out"""
    import os
    from conftest import REFRUNS
    assert all(n.startswith("empty_graph") and why for n, why in T.NOT_ADD_RECORDED)
    for name in T.add_recorded():
        assert os.path.exists(os.path.join(REFRUNS, f"step5_addref_{name}", "run.json")), name
    assert set(T.add_recorded()) | {n for n, _ in T.NOT_ADD_RECORDED} == set(T.cases()) | {f"random_{s}" for s in T.SEEDS}


@pytest.mark.parametrize("seed", T.SEEDS)
def test_generated_cases_reach_every_counter(seed):
    c = T.get(f"random_{seed}")
    h, paths, reads, quals, new = c.inputs()
    assert 2800 <= sum(int(x) for x in h.edge_len) // 2 and len(reads[2]) == 400 and set(int(x) for x in reads[2]) == {150}
    m = run_model(f"random_{seed}")
    print(seed, h.n_edges, m.counters)
    assert T.seed_conditions(m) == []


def test_overlap_append_takes_the_longest_overlap():
    v = [1, 2, 3, 2, 3]
    assert M.overlap_append(v, [2, 3, 2, 3, 9]) == 4 and v == [1, 2, 3, 2, 3, 9]
    v = [1, 2]
    assert M.overlap_append(v, [3]) == 0 and v == [1, 2, 3]
    v = []
    assert M.overlap_append(v, [5, 6]) == 0 and v == [5, 6]

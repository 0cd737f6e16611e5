"""The graph edit of Step 4 without a GPU: the interface of the device / host switch, and the proof that the hand-made graphs of
step4_edit_cases.py exercise, in the CPU model (tests/step4_model.py, pinned to the reference by test_step4_model.py), the rule each one
exists for.  A fixture that does not exercise its rule fails here."""
import os
import re

import numpy as np
import pytest

import step4_cases as S
import step4_edit_cases as EC
import step4_model as M
from conftest import ROOT
from w2rap_contigger_amd import step2, step4

CASES = EC.edit_cases()


def _model(name):
    h, paths, (pk, bo, ln), quals, ms = CASES[name].inputs
    M.RUN_SIZES.clear()
    return M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)


def _edges(hbv):
    codes, off = hbv.edge_codes()
    off = off.astype(np.int64)
    return [codes[off[e]:off[e + 1]] for e in range(hbv.n_edges)]


def _same_edges(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_edit_argument_is_checked():
    h, paths, (pk, bo, ln), quals = S.load("random20k")
    with pytest.raises(ValueError):
        step4.clean200x(h, paths, pk, bo, ln, quals, edit="sideways")
    with pytest.raises(ValueError):
        step4.run_step4_files("/nonexistent", "t", edit="sideways")


def test_unknown_flag_is_refused_before_the_device():
    import ctypes as C
    i, o = step4.Step4In(), step4.Step4Out()
    i.K = 200
    err = C.create_string_buffer(256)
    for flags, ok in ((4, False), (2 | 4, False), (8, False)):
        rc = step4.lib().w2rap_step4_run(C.byref(i), C.byref(step4.Step4Params(0, 0, flags)), C.byref(o), err, 256)
        assert rc == 1 and b"unknown flag" in err.value, (flags, rc, err.value)


def test_header_defines_the_flag():
    text = open(os.path.join(ROOT, "include", "w2rap_step4.h")).read()
    m = re.search(r"#define\s+W2RAP_STEP4_EDIT_ON_HOST\s+(\d+)u\b", text)
    assert m and int(m.group(1)) == 2 == step4.EDIT_ON_HOST
    assert step4.EDIT_ON_HOST & step4.VOTE_ONLY == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_exercises_the_rule(name):
    x = CASES[name].expect
    m = _model(name)
    got = _edges(m.hbv)
    if "merged" in x:
        assert m.counters.n_runs_merged == x["merged"], m.counters
    if "edges" in x:
        assert _same_edges(got, x["edges"]), "the new edges are not numbered by ascending largest kill vertex, mirror first"
    for wrong in ("by_smallest", "by_eleft"):
        if wrong in x:
            assert not _same_edges(got, x[wrong]), f"the fixture cannot tell the rule from ranking {wrong}"
    if "run_size" in x:
        assert max(M.RUN_SIZES) == x["run_size"], M.RUN_SIZES
    if "from_lists" in x:
        fo = m.hbv.from_off.astype(np.int64)
        lists = sorted([int(e) for e in m.hbv.from_e[fo[v]:fo[v + 1]]] for v in range(m.hbv.n_vertices) if fo[v + 1] - fo[v] > 1)
        assert lists == x["from_lists"], lists
        to = m.hbv.to_off.astype(np.int64)
        assert sorted([int(e) for e in m.hbv.to_e[to[v]:to[v + 1]]] for v in range(m.hbv.n_vertices) if to[v + 1] - to[v] > 1) == x["from_lists"]
    if "n_edges" in x:
        assert m.hbv.n_edges == x["n_edges"]
    if "n_vertices" in x:
        assert m.hbv.n_vertices == x["n_vertices"]
    if "deleted0" in x:
        assert len(m.deleted[0]) == x["deleted0"]
    if "merged_each" in x:
        assert all(k > 0 for k in m.counters.n_runs_merged) and len(m.deleted[0]) > 0 and len(m.deleted[1]) > 0, (m.counters, m.deleted)
        assert any(np.array_equal(e, x["contains"]) for e in got), "pass 2 did not merge the edge pass 1 made"
    if "unsorted" in x:
        h = CASES[name].inputs[0]
        fo = h.from_off.astype(np.int64)
        assert any(np.any(np.diff(h.from_v[fo[v]:fo[v + 1]]) < 0) for v in range(h.n_vertices))


def test_circles_are_handled_as_the_model_says():
    """(e): circle 1 pushes itself only, circle 2 and its mirror circle both push: six copies in pass 1, each the edge it copies; the copied
    edges are the out-edges of the circles' largest vertices and their inv, and pass 2 finds no e < inv[e] any more"""
    h, paths, (pk, bo, ln), quals, ms = CASES["e_circles"].inputs
    before = _edges(h)
    m = _model("e_circles")
    after = _edges(m.hbv)
    assert M.RUN_SIZES == [1] * 6
    # pass 1 keeps the six untouched edges in order and appends copies of 5, 4 (circle 1), 9, 8 (circle 2), 7, 6 (its mirror circle)
    assert _same_edges(after, [before[e] for e in (0, 1, 2, 3, 10, 11, 5, 4, 9, 8, 7, 6)])
    assert list(m.inv) == [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10]


@pytest.mark.parametrize("name", sorted(EC.empty_cases()))
@pytest.mark.parametrize("min_size", [0, 40])
def test_the_model_returns_an_empty_graph_for_a_graph_without_edges(name, min_size):
    h, paths, (pk, bo, ln), quals = EC.empty_cases()[name]
    assert h.n_edges == 0 and len(paths[0]) == 2 and len(paths[2]) == 0
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), min_size)
    assert (m.hbv.n_vertices, m.hbv.n_edges, m.deleted, m.counters.n_runs_merged) == (0, 0, [[], []], [0, 0])
    assert (list(m.path_offset), list(m.path_off), list(m.path_edges)) == ([0, 0], [0, 0, 0], [])


def test_the_model_merges_the_long_run_without_reads():
    h, paths, (pk, bo, ln), quals, ms = EC.no_reads_case()
    M.RUN_SIZES.clear()
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)
    x = CASES["b_long_run"].expect
    assert m.counters.n_runs_merged == x["merged"] and max(M.RUN_SIZES) == x["run_size"] and _same_edges(_edges(m.hbv), x["edges"])
    assert len(m.path_offset) == 0 and list(m.path_off) == [0]

"""The graph edit of Step 4 without a GPU: the interface of the device / host switch, and the proof that the hand-made graphs of
step4_edit_cases.py exercise, in the CPU model (tests/step4_model.py, pinned to the reference by test_step4_model.py), the rule each one
exists for.  A fixture that does not exercise its rule fails here."""
import os
import re
import subprocess

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


# ---- real numbering, sizes on block and tile edges, one-k-mer members: what the fixtures of those must exercise in the model
_MODELS = {}


def _run_model(key, inputs):
    """-> (Model4Result, RUNS per pass, RUN_SIZES) of one input, computed once"""
    if key not in _MODELS:
        h, paths, (pk, bo, ln), quals, ms = inputs
        M.RUN_SIZES.clear(); M.RUNS.clear()
        m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)
        _MODELS[key] = (m, [list(x) for x in M.RUNS], list(M.RUN_SIZES))
    return _MODELS[key]


def _lists(hbv, side):
    off, le = (hbv.from_off, hbv.from_e) if side == "from" else (hbv.to_off, hbv.to_e)
    off = off.astype(np.int64)
    tl, tr = hbv.to_left_right()
    nb = tr if side == "from" else tl
    return [[(int(nb[e]), int(e)) for e in le[off[v]:off[v + 1]]] for v in range(hbv.n_vertices)]


def _ties(hbv):
    """-> (ascending, descending): the number of neighbouring list entries on the same vertex whose edge ids ascend / descend"""
    up = down = 0
    for side in ("from", "to"):
        for l in _lists(hbv, side):
            assert [w for w, _ in l] == sorted(w for w, _ in l), "a renumbered list is not sorted by neighbour"
            for (w0, e0), (w1, e1) in zip(l, l[1:]):
                up += w0 == w1 and e0 < e1; down += w0 == w1 and e0 > e1
    return up, down


def test_renumbering_keeps_the_graph_and_the_result():
    """the renumbered input is the same graph: the model's clean graph has the same multiset of edge sequences, and the read paths spell
    the same bases"""
    for name in ("a_interleaved_runs", "h_two_passes_compose", "b_long_run"):
        base = CASES[name].inputs
        m0, _, _ = _run_model(("base", name), base)
        for seed, ties in EC.RENUMBER:
            m1, _, _ = _run_model(("var", name, seed, ties), EC.renumbered(base, seed, ties))
            assert sorted(bytes(x) for x in _edges(m1.hbv)) == sorted(bytes(x) for x in _edges(m0.hbv))
            assert list(m1.path_offset) == list(m0.path_offset) and list(m1.path_off) == list(m0.path_off)
            e0, e1 = _edges(m0.hbv), _edges(m1.hbv)
            assert all(np.array_equal(e0[a], e1[b]) for a, b in zip(m0.path_edges, m1.path_edges))
            assert m1.counters.n_runs_merged == m0.counters.n_runs_merged and m1.counters.n_deleted == m0.counters.n_deleted


def test_the_renumbered_variants_have_the_numbering_of_a_real_graph():
    V = {name: EC.renumbered_variant(name) for name in EC.variant_names()}
    assert len(V) == 4 * (len(CASES) - 1 + len(S.hand_cases()) + 1) + 12
    not_xor = above = below = interior = reordered = asc_down = desc_down = 0
    for name, inputs in V.items():
        h = inputs[0]
        inv = M.involution(M.Graph.from_hbv(h))
        not_xor += any(x != (e ^ 1) for e, x in enumerate(inv))
        up, down = _ties(h)
        if name.endswith("-asc"):
            asc_down += down
        else:
            desc_down += down
        _, runs, _ = _run_model(("variant", name), inputs)
        for per_pass in runs:
            chains = [r for r in per_pass if r.eleft != r.eright]
            for r in chains:
                if r.mirror_kill is not None:
                    above += max(r.kill) > max(r.mirror_kill); below += max(r.kill) < max(r.mirror_kill)
                interior += len(r.kill) >= 3 and max(r.kill) not in (r.kill[0], r.kill[-1])
            by = lambda key: [(r.eleft, r.eright) for r in sorted(chains, key=key)]
            largest = by(lambda r: max(r.kill))
            reordered += largest != by(lambda r: min(r.kill)) and largest != by(lambda r: r.eleft)
    assert not_xor == len(V), "a variant is numbered as the builder numbers"
    assert above >= 20 and below >= 20, (above, below)
    assert interior >= 20 and reordered >= 10, (interior, reordered)
    assert asc_down == 0 and desc_down >= 20, (asc_down, desc_down)


@pytest.mark.parametrize("name", EC.size_names())
def test_the_size_cases_exercise_their_point(name):
    c = EC.size_case(name)
    x = c.expect
    h = c.inputs[0]
    m, runs, sizes = _run_model(("size", name), c.inputs)
    got = _edges(m.hbv)
    fam, _, num = name.rpartition("_")
    if fam == "runs":
        P = int(num)
        assert m.counters.n_runs_merged == [2 * P, 0] and P in EC.RUNS_P and len(runs[0]) == P
        if P % 128 == 0:
            assert (2 * P) % 256 == 0 and (h.n_edges + 2 * P) % 256 == 0, "M and E + M are to end on a block of 256 threads"
    if fam == "run_len":
        L = int(num)
        assert len(runs[0]) == 1 and len(runs[0][0].kill) == L == len(runs[0][0].mirror_kill) and sizes == [L + 1, L + 1] and m.counters.n_runs_merged == [2, 0]
        assert int(m.path_offset[0]) > int(c.inputs[1][0][0]), "the read on the last member did not move"
    if fam == "circle":
        L = int(num)
        circles = [r for r in runs[0] if r.eleft == r.eright]
        assert [len(r.kill) for r in circles] == ([] if L == 2 else [L]) and len(runs[0]) - len(circles) == 1
    if "merged" in x:
        assert m.counters.n_runs_merged == x["merged"]
    if "n_edges" in x:
        assert m.hbv.n_edges == x["n_edges"]
    if "edges" in x:
        assert _same_edges(got, x["edges"])
    if "run_size" in x:
        assert x["run_size"] in sizes, sizes
    if "min_kmers" in x:
        g = M.Graph.from_hbv(h)
        members = [sorted({g.to_e[v][0] for v in r.kill} | {g.frm_e[v][0] for v in r.kill}) for r in runs[0]]
        assert min(g.kmers(e) for mem in members for e in mem) == x["min_kmers"] == 1
        assert any(len(mem) == x["run_size"] and all(g.kmers(e) == 1 for e in mem) for mem in members)
        assert sorted(int(o) for o in m.path_offset)[-1] == x["run_size"] - 1, "no read starts on the last member"
    if "from_s" in x:
        fr, to = _lists(m.hbv, "from"), _lists(m.hbv, "to")
        assert m.hbv.n_vertices == 4 and len(x["from_s"]) == 1025
        assert [e for _, e in fr[0]] == x["from_s"] == [e for _, e in to[2]]
        assert [e for _, e in to[1]] == x["to_s_mirror"] == [e for _, e in fr[3]]
    if "hub_from" in x:
        fr, to = _lists(m.hbv, "from"), _lists(m.hbv, "to")
        assert x["hub_from"][:9] == [0, 101, 2, 103, 105, 4, 6, 8, 107] and len(x["hub_from"]) == 90
        assert [e for _, e in fr[0]] == x["hub_from"], "From(x): old before new on an equal neighbour, new in creation order"
        assert [e for _, e in to[1]] == x["hub_to"] == [e - 1 if e >= 100 else e + 1 for e in x["hub_from"]]
        kinds = "".join("n" if e >= 100 else "o" for _, e in fr[0])
        assert kinds == "ononnooon" * 10


def test_pass_one_can_delete_every_edge():
    h, paths, (pk, bo, ln), quals, ms = EC.all_deleted_case()
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms)
    assert m.deleted == [[0, 1, 2, 3, 4, 5], []] and (m.hbv.n_vertices, m.hbv.n_edges) == (0, 0)
    assert list(m.path_off) == [0, 0, 0] and len(m.path_edges) == 0


def test_the_bad_inv_inputs_pass_the_argument_check_and_break_the_model():
    """each inv is an involution of edges of equal length (what w2rap_step4_run checks) and no vertex branches (nothing but the edit reads
    inv); the model, which restates the reference's unguarded walk, runs off the graph on the two inputs whose walk ends"""
    B = EC.bad_inv_cases()
    assert sorted(B) == ["circle", "self", "swap"]
    for name, (h, paths, (pk, bo, ln), quals, inv) in B.items():
        assert all(inv[inv[e]] == e and h.edge_len[inv[e]] == h.edge_len[e] for e in range(h.n_edges))
        assert list(inv) != M.involution(M.Graph.from_hbv(h))
        fo, to = np.diff(h.from_off.astype(np.int64)), np.diff(h.to_off.astype(np.int64))
        assert not np.any((fo > 1) & (to > 0))
        if name != "circle":
            with pytest.raises(IndexError):
                M.clean200x(h, inv, paths, M.reads_of(pk, bo, ln, quals), 0)


def test_the_host_edit_answers_a_bad_inv_with_an_error_under_the_host_sanitizers(tmp_path):
    """tools/step4_bad_inv.cpp: edit_graph itself, host code only, with AddressSanitizer and UndefinedBehaviorSanitizer, on the three
    inputs of bad_inv_cases() and on the good inv: W2RAP_E_GRAPH with a message that names inv, no report, no endless walk"""
    exe = str(tmp_path / "step4_bad_inv")
    csrc = os.path.join(ROOT, "w2rap_contigger_amd", "csrc")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", csrc,
                    os.path.join(ROOT, "tools", "step4_bad_inv.cpp"), os.path.join(csrc, "step4_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    for which in ("good", "self", "swap", "circle"):
        r = subprocess.run([exe, which], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (which, r.stdout, r.stderr)
        assert (" rc 6," in r.stdout and "inv" in r.stdout) if which != "good" else " rc 0, merged 2," in r.stdout, r.stdout

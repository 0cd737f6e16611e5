"""The vote of Step 4 without a GPU: the proof that every input of step4_vote_cases.py sits, in the CPU model (tests/step4_model.py, pinned
to the reference by test_step4_model.py), on the boundary its name says -- what is deleted, both sides of each pair, that one read fewer
or more flips the verdict, where the tested vertex starts in the flat placement list, how many walks a vertex has -- and that the 24
random graphs exercise what they are there for.  A fixture that does not exercise its boundary fails here, before any GPU run."""
import functools

import numpy as np
import pytest

import step4_model as M
import step4_vote_cases as V
from step4_cases import Hand
from w2rap_contigger_amd import formats as F

CASES = V.vote_cases()
# pairs whose two sides differ in ONE quality value and in nothing else
ONE_VALUE = ["a_min_win_100_99", "a_max_lose_50_51_two_reads", "a_min_ratio_150_149", "a_min_ratio_two_losers", "d_starts_100_before", "d_starts_100_before_rc",
             "d_longer_than_the_window", "d_longer_than_the_window_rc", "d_quality_63", "d_length_149", "d_length_150", "d_length_151", "d_length_153"]


def _run(inputs, **kw):
    h, paths, (pk, bo, ln), quals, ms = inputs
    M.PLACEMENTS = rec = []
    try:
        return M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms, **kw), rec
    finally:
        M.PLACEMENTS = None


def _variant(case, drop=None, dup=None):
    """the case's inputs with one read removed or one read given twice"""
    h = case.hand
    keep = (h.paths, h.offs, h.codes, h.quals)
    idx = [i for i in range(len(h.paths)) if i != drop] + ([dup] if dup is not None else [])
    h.paths, h.offs, h.codes, h.quals = ([x[i] for i in idx] for x in keep)
    try:
        return h.case() + (case.inputs[4],)
    finally:
        h.paths, h.offs, h.codes, h.quals = keep


def test_hand_read_takes_a_quality_per_base():
    h = Hand(seed=1); u, v = h.vertex(), h.vertex(); e = h.edge(u, v, 60)
    q = np.arange(40, dtype=np.uint8)
    h.read([e], 5, 40, qual=q); h.read([e], 5, 40, qual=q, rc=True); h.read([e], 5, 40, qual=17)
    assert np.array_equal(h.quals[0], q) and np.array_equal(h.quals[1], q[::-1]) and np.array_equal(h.quals[2], np.full(40, 17))
    assert np.array_equal(h.codes[1], (3 - h.codes[0][::-1]))
    with pytest.raises(AssertionError):
        h.read([e], 5, 40, qual=q[:39])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_case_sits_where_it_claims(name):
    case = CASES[name]; x = case.expect
    hb, paths, (pk, bo, ln), quals, ms = case.inputs
    m, rec = _run(case.inputs, vote_only=True)
    assert m.deleted[0] == x["deleted"], (m.deleted, rec)
    at = {v: k for k, (v, _, _, _) in enumerate(rec)}
    for v, n in x.get("walks", {}).items():
        assert rec[at[v]][1] == n, rec
    for v, d in x.get("depth", {}).items():
        assert rec[at[v]][2] == d, rec
    if "skipped" in x:
        assert m.counters.n_skipped_too_many_exts == x["skipped"]
    if "placements" in x:
        assert m.counters.n_placements == x["placements"]
    if "offset" in x:
        assert sum(n for _, _, _, n in rec[:at[x["vertex"]]]) == x["offset"], rec
        assert x["offset"] < 256 < x["offset"] + rec[at[x["vertex"]]][3]
    if "n" in x:
        assert rec[at[x["vertex"]]][3] == x["n"] and (x["n"] < 256 or x["offset"] + x["n"] > 512)
    if "max_placements" in x:
        assert len(rec) == x["n_vertices"] and m.counters.n_placements <= x["max_placements"] and all(5 <= n <= 6 for _, _, _, n in rec)
    for e in x.get("stay", ()):
        assert e not in m.deleted[0] and e + 1 not in m.deleted[0]
    if x.get("more_placements_than_reads"):
        assert m.counters.n_placements > len(ln)
    if x.get("fewer_than_listed"):
        # without the skip of roles 1 and 3 every listing of an in-edge, an out-edge or one of their mirrors would be a placement
        g = M.Graph.from_hbv(hb); inv = M.involution(g); v = x["vertex"]
        tasks = g.to_e[v] + g.frm_e[v] + [inv[e] for e in g.to_e[v]] + [inv[e] for e in g.frm_e[v]]
        po = paths[1].astype(np.int64)
        listed = sum(int(np.sum(paths[2] == e)) for e in tasks)
        assert rec[at[v]][3] < listed, (rec, listed)
        fw = sum(1 for i in range(len(ln)) if po[i + 1] - po[i] == 2 and paths[2][po[i]] in g.to_e[v])
        rv = sum(1 for i in range(len(ln)) if po[i + 1] - po[i] == 2 and paths[2][po[i] + 1] in [inv[e] for e in g.to_e[v]])
        assert fw > 0 and rv > 0 and listed - rec[at[v]][3] == fw + rv
        assert {int(paths[2][po[i]]) for i in range(len(ln)) if po[i + 1] - po[i] == 2} >= set(g.to_e[v]), "a read enters through every in-edge"
    for rid in x.get("drop_keeps", ()):
        assert _run(_variant(case, drop=rid), vote_only=True)[0].deleted[0] == [], f"without read {rid} the verdict must flip"
    for rid in x.get("dup_keeps", ()):
        assert _run(_variant(case, dup=rid), vote_only=True)[0].deleted[0] == [], f"with read {rid} counted twice the verdict must flip"


def test_the_cases_cover_the_issue():
    names = set(CASES)
    for stem in [n[:-8] for n in names if n.endswith("_deletes")]:
        a, b = CASES[stem + "_deletes"], CASES[stem + "_keeps"]
        assert a.expect["deleted"] and b.expect["deleted"] == []
        assert F.hbv_to_bytes(a.inputs[0]) == F.hbv_to_bytes(b.inputs[0]), stem
    for stem in ONE_VALUE:
        a, b = CASES[stem + "_deletes"].inputs, CASES[stem + "_keeps"].inputs
        assert F.paths_to_bytes(*a[1]) == F.paths_to_bytes(*b[1]) and all(np.array_equal(p, q) for p, q in zip(a[2], b[2])), stem
        assert int(np.sum(a[3] != b[3])) == 1, stem
    for d in (0, 1, 7, 14, 15):
        assert f"a_threshold_d{d}_deletes" in names
    for g in "abcde":
        assert any(n.startswith(g + "_") for n in names)
    # half of the reads of every case of group A are of the other strand (their paths run on the mirror edges, the odd ids)
    for n in names:
        if n.startswith("a_"):
            po = CASES[n].inputs[1][1].astype(np.int64); pe = CASES[n].inputs[1][2]
            odd = sum(int(pe[po[i]] & 1) for i in range(len(po) - 1))
            assert abs(2 * odd - (len(po) - 1)) <= 2, n


# ---------------------------------------------------------------------------------------------------------------- the random graphs
@functools.lru_cache(maxsize=None)
def _random(seed):
    h = V.random_case(seed)
    inputs = h.case() + (0,)
    first, _ = _run(inputs, vote_only=True)
    full, _ = _run(inputs)
    return h, inputs, first, full


def test_random_case_is_a_function_of_its_seed():
    a, b = V.random_case(3).case(), V.random_case(3).case()
    assert F.hbv_to_bytes(a[0]) == F.hbv_to_bytes(b[0]) and F.paths_to_bytes(*a[1]) == F.paths_to_bytes(*b[1]) and np.array_equal(a[3], b[3])
    assert F.hbv_to_bytes(a[0]) != F.hbv_to_bytes(V.random_case(4).case()[0])


def test_random_graphs_have_the_parts_and_exercise_the_step():
    assert len(V.SEEDS) == 24 == len(set(V.SEEDS))
    n = dict(vote=0, pass2=0, merged=0, skipped=0, large=0, big=0, loop=0, pal=0)
    for seed in V.SEEDS:
        h, (hb, paths, (pk, bo, ln), quals, _), first, full = _random(seed)
        assert hb.K == 20 and 30 <= hb.n_vertices // 2 <= 120, seed
        assert 200 <= len(ln) <= 1500 and ln.min() >= 60 and ln.max() <= 300 and quals.max() <= 63
        po = paths[1].astype(np.int64)
        empty = int(np.sum(np.diff(po) == 0)); odd = sum(int(paths[2][po[i]] & 1) for i in range(len(ln)) if po[i + 1] > po[i])
        assert 0.05 * len(ln) <= empty <= 0.2 * len(ln) and 0.25 * len(ln) <= odd <= 0.65 * len(ln), (seed, empty, odd)
        # the preconditions of the device edit: adjacency lists sorted by neighbour, every edge paired with its mirror image
        fo = hb.from_off.astype(np.int64)
        assert all(np.all(np.diff(hb.from_v[fo[v]:fo[v + 1]]) >= 0) for v in range(hb.n_vertices))
        mir = V.mirror_ids(h)
        assert list(first.inv) == [mir[e] for e in range(hb.n_edges)] or sorted(first.inv) == list(range(hb.n_edges))
        deg = np.diff(fo)
        assert int(np.sum(deg >= 10)) <= 1 and deg.max() <= 12
        E = h.b.edges
        loops = sum(1 for u, v, _ in E if u == v); pals = sum(1 for e in range(len(E)) if mir[e] == e)
        assert loops <= 2 and pals <= 1                      # (a self-loop and its mirror image)
        c = full.counters
        n["vote"] += len(first.deleted[0]) > 0; n["pass2"] += c.n_deleted[1] > 0; n["merged"] += sum(c.n_runs_merged) > 0
        n["skipped"] += first.counters.n_skipped_too_many_exts > 0; n["large"] += first.counters.n_placements > 512
        n["big"] += deg.max() >= 10; n["loop"] += loops > 0; n["pal"] += pals > 0
    assert n["vote"] >= 12 and n["pass2"] >= 3 and n["merged"] == 24 and n["skipped"] >= 2 and n["large"] >= 6, n
    assert n["big"] >= 3 and n["loop"] >= 3 and n["pal"] >= 1, n

"""The yardstick of Step 5's tail is right: step5_model.partners_to_ends gives the outcomes the hand-made cases write down as literals,
and its distances with the cap at 501 give the verdict D <= 500 of the reference's worklist with a cap far above any distance at hand."""
import numpy as np
import pytest

import step5_cases as S
import step5_model as M
from step4_cases import Builder

CASES = S.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_gives_the_literal_outcomes(name):
    c = CASES[name]
    h, paths, reads, quals = c.inputs()
    m = M.partners_to_ends(h, paths, reads, quals)
    po = m.path_off.astype(np.int64)
    assert c.expect, "a case names the reads it is about"
    for r, (path, offset) in c.expect.items():
        assert (list(m.path_edges[po[r]:po[r + 1]]), int(m.path_offset[r])) == (path, offset), f"read {r}"
    for k, v in c.counters.items():
        assert m.counters[k] == v, k
    # every read the case does not name had a path and keeps it
    opo = paths[1].astype(np.int64)
    for r in range(len(opo) - 1):
        if r not in c.expect:
            assert list(m.path_edges[po[r]:po[r + 1]]) == list(paths[2][opo[r]:opo[r + 1]]) and m.path_offset[r] == paths[0][r]


def test_cases_cover_both_outcomes_of_each_rule():
    placed = sum(1 for c in CASES.values() for p, _ in c.expect.values() if p)
    empty = sum(1 for c in CASES.values() for p, _ in c.expect.values() if not p)
    assert placed > 20 and empty > 20


@pytest.mark.parametrize("seed", range(12))
def test_saturated_distance_gives_the_worklists_verdict(seed):
    """random graphs of 20 to 60 vertices, edges of 1 .. 250 K-mers, two in three seeds with back edges (cycles)"""
    rng = np.random.default_rng(1000 + seed)
    nv = int(rng.integers(20, 61))
    b = Builder(20)
    b.nv = nv
    for _ in range(int(rng.integers(nv, 2 * nv))):
        u, v = (int(x) for x in rng.integers(0, nv, 2))
        if seed % 3 == 0 and u >= v:                         # acyclic: edges go up only
            u, v = min(u, v), max(u, v) + 1
            if v >= nv:
                continue
        b.edge(u, v, np.zeros(int(rng.integers(1, 251)) + 19, np.uint8), mirror=False)
    h = b.hbv()
    low = M.distances_to_end(h, 501)
    high = M.distances_to_end(h, 2000)
    assert [d <= 500 for d in low] == [d <= 500 for d in high]
    assert any(d <= 500 for d in high)
    assert M.near_end_edges(h) == M.near_end_edges(h, 2000)

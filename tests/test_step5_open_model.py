"""The yardstick of Step 5's opening is right: step5_open_model.opening gives, for every hand-made case, the index, links, multiplicities,
layout entries and counters the case writes down as literals."""
import numpy as np
import pytest

import step5_open_cases as S
import step5_open_model as M

CASES = S.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_gives_the_literal_outcomes(name):
    c = CASES[name]
    m = M.opening(*c.inputs())
    assert c.counters and c.layout and c.index, "a case writes down what it expects"
    assert m.counters == c.counters
    assert S.per_edge(m.index_off, m.index_read) == c.index
    assert S.per_edge(m.link_off, m.link_to, m.link_pid) == c.links
    assert S.kinds(m) == c.mult
    assert S.per_edge(m.layout_off, m.layout_pos, m.layout_id, m.layout_fw) == c.layout


def test_cases_reach_every_counter():
    total = {k: sum(c.counters[k] for c in CASES.values()) for k in S.COUNTERS}
    assert all(v > 0 for v in total.values()), total
    assert any(m > 1 for c in CASES.values() for m in c.mult.values())
    assert any(p < 0 for c in CASES.values() for l in c.layout.values() for p, _, _ in l)


def test_kinds_are_the_runs_of_the_links():
    """kind_mult is the run length of (edge, link_to) in the link lists, in the lists' order"""
    m = M.opening(*CASES["multiplicities_3_and_1"].inputs())
    off = m.link_off.astype(np.int64)
    runs = []
    for e in range(len(off) - 1):
        for j in range(off[e], off[e + 1]):
            if runs and runs[-1][:2] == [e, int(m.link_to[j])]:
                runs[-1][2] += 1
            else:
                runs.append([e, int(m.link_to[j]), 1])
    assert runs == [[int(a), int(b), int(k)] for a, b, k in zip(m.kind_from, m.kind_to, m.kind_mult)]


@pytest.mark.parametrize("seed", S.SEEDS)
def test_generated_cases_reach_every_branch(seed):
    """the seeds test_gpu_step5_open.py uses: by the model's own count every counter is at least 1, a link kind has multiplicity above 1
    and a layout position is negative"""
    h, inv, paths, read_len = S.random_case(seed)
    assert 200 <= h.n_edges <= 900 and len(read_len) == 2000
    m = M.opening(h, inv, paths, read_len)
    print(seed, h.n_edges, m.counters, int(max(m.kind_mult)))
    assert S.seed_conditions(m) == []

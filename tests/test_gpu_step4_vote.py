"""The vote of Step 4 on the GPU (k4_walks, k4_item_count, k4_place_count, k4_place_fill, k4_score, k4_reduce, k4_verdict, and k4e_min_size)
against the CPU model (tests/step4_model.py) on the boundary cases of step4_vote_cases.py -- each proven on the CPU to sit on its boundary
by test_step4_vote_model.py -- and on 24 seeded random graphs, device edit and host edit.  All arithmetic is integer: no comparison has
a tolerance."""
import functools

import pytest

import step4_model as M
import step4_vote_cases as V
from test_gpu_step4_edit import _same, _same_results
from w2rap_contigger_amd import formats as F, step4

pytestmark = pytest.mark.gpu

CASES = V.vote_cases()
VOTE_KERNELS = ("k4_walks", "k4_item_count", "k4_place_count", "k4_place_fill", "k4_score", "k4_reduce", "k4_verdict")


def _voted():
    prof = step4.profile()
    return all(prof.get(k, (0.0, 0))[1] >= 1 for k in VOTE_KERNELS), prof


@pytest.mark.parametrize("name", sorted(CASES))
def test_boundary_case_on_the_device(name):
    h, paths, (pk, bo, ln), quals, ms = CASES[name].inputs
    reads = M.reads_of(pk, bo, ln, quals)
    m = M.clean200x(h, None, paths, reads, ms)
    res = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
    assert res.edit_on_device is True
    if m.counters.n_placements:
        ok, prof = _voted()
        assert ok, prof
    assert [list(x) for x in res.deleted][0] == CASES[name].expect["deleted"] == m.deleted[0], "pass 1 deletes something else"
    _same(res, m)
    m1 = M.clean200x(h, None, paths, reads, ms, vote_only=True)
    only = step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, vote_only=True, edit="device")
    assert list(only.deleted[0]) == m1.deleted[0]
    _same(only, m1, vote_only=True)
    assert F.hbv_to_bytes(only.hbv, zero_padding=True) == F.hbv_to_bytes(h, zero_padding=True)
    assert F.paths_to_bytes(only.path_offset, only.path_off, only.path_edges) == F.paths_to_bytes(*paths)


def test_every_group_runs_the_vote_kernels():
    for g in "abcde":
        name = sorted(n for n in CASES if n.startswith(g + "_"))[0]
        h, paths, (pk, bo, ln), quals, ms = CASES[name].inputs
        step4.clean200x(h, paths, pk, bo, ln, quals, min_size=ms, edit="device")
        ok, prof = _voted()
        assert ok, (name, prof)
        if g == "e":
            assert prof.get("k4e_min_size", (0.0, 0))[1] >= 1, prof


@pytest.mark.parametrize("seed", V.SEEDS)
def test_random_graph_device_host_model(seed):
    h, paths, (pk, bo, ln), quals = V.random_case(seed).case()
    m = M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), 0)
    dev = step4.clean200x(h, paths, pk, bo, ln, quals, edit="device")
    assert dev.edit_on_device is True
    _same(dev, m)
    host = step4.clean200x(h, paths, pk, bo, ln, quals, edit="host")
    assert host.edit_on_device is False
    _same(host, m)
    _same_results(dev, host)

"""The yardsticks of Step 5 against the reference itself: step5_model.partners_to_ends equals recorded runs of the reference's own
PartnersToEnds, and step5_open_model's paths index and read layout equal recorded runs of its invert and LayoutReads
(oracle/ref_step5_driver.cc; tests/golden/refruns/step5_tail_<case>/ and step5_open_<case>/, recorded by `make_golden.py refruns` at
1 thread and at 4, which had to agree).  Every hand-made case and every generated one.  Unsat's Phase 1 has no output of its own in the
reference, so the links stay on the literals of step5_open_cases and on the model."""
import numpy as np
import pytest

import step5_cases as T
import step5_model as TM
import step5_open_cases as S
import step5_open_model as SM


def same_paths(got, ref):
    """got: anything with path_offset / path_off / path_edges; ref: (offset, path_off, edges) as formats.read_paths gives them"""
    assert np.array_equal(got.path_off, ref[1])
    assert np.array_equal(got.path_edges, ref[2])
    assert np.array_equal(got.path_offset, ref[0])


def same_index_and_layout(got, ref_index, ref_layout):
    """got: anything with the index_* and layout_* arrays.  The index list for list.  The layout per edge: the positions in order, and
    the (pos, id, forward) entries as a multiset -- SortSync leaves the order of entries that tie on pos open, the library's is its own"""
    assert S.per_edge(got.index_off, got.index_read) == ref_index
    lay = S.per_edge(got.layout_off, got.layout_pos, got.layout_id, got.layout_fw)
    lay = {e: [(p, i, bool(f)) for p, i, f in l] for e, l in lay.items()}
    assert sorted(lay) == sorted(ref_layout)
    for e, l in lay.items():
        assert [p for p, _, _ in l] == [p for p, _, _ in ref_layout[e]], f"edge {e}"
        assert sorted(l) == sorted(ref_layout[e]), f"edge {e}"


def test_every_case_is_recorded_or_accounted_for():
    assert set(T.NOT_RECORDED) <= set(T.cases()) and set(S.NOT_RECORDED) <= set(S.cases())
    assert len(T.recorded()) + len(T.NOT_RECORDED) == len(T.cases()) + len(T.SEEDS)
    assert len(S.recorded()) + len(S.NOT_RECORDED) == len(S.cases()) + len(S.SEEDS)


@pytest.mark.parametrize("name", T.recorded())
def test_tail_model_equals_the_recorded_reference(name, tmp_path):
    ref = T.reference_run(name, str(tmp_path))
    same_paths(TM.partners_to_ends(*T.inputs_of(name)), ref)


@pytest.mark.parametrize("seed", T.SEEDS)
def test_generated_tail_cases_reach_every_branch(seed):
    """the seeds test_gpu_step5.py uses: by the model's own count every counter is at least 1, 28-mers are dropped by either filter,
    candidates are rejected and a read is placed at a negative offset"""
    h, paths, reads, quals = T.inputs_of(f"random_{seed}")
    assert h.K == 60 and 40 <= h.n_edges <= 100 and 400 <= len(reads[2]) <= 1000
    assert 28 <= int(min(reads[2])) and int(max(reads[2])) <= 300
    n_unplaced = int(np.sum(np.diff(paths[1].astype(np.int64)) == 0))
    assert 0.25 <= n_unplaced / len(reads[2]) <= 0.42
    m = TM.partners_to_ends(h, paths, reads, quals)
    print(seed, h.n_edges, len(reads[2]), m.counters, m.extra)
    assert T.seed_conditions(m) == []


@pytest.mark.parametrize("name", S.recorded())
def test_opening_model_equals_the_recorded_reference(name, tmp_path):
    index, layout = S.reference_run(name, str(tmp_path))
    same_index_and_layout(SM.opening(*S.inputs_of(name)), index, layout)

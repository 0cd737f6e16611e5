"""The model of DumpLineFiles, SortLines and the stats file (tests/step7_fasta_model.py) held to the recorded runs of the reference's
main (tests/golden/refruns/step7_ff_*) byte for byte, and to literal outcomes derived by hand.  No GPU."""
import numpy as np
import pytest

import step7_fasta_cases as C
import step7_fasta_model as M

RECORDED = sorted(C.recorded_cases())
MODEL_ONLY = sorted(C.model_cases())


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return C.recorded(tmp_path_factory.mktemp("ff"))


@pytest.fixture(scope="module")
def model_cases():
    return C.model_cases()


def _model(case, kind, rec):
    hbv, inv, paths, lines = C.inputs_of(None, case, kind, rec)
    return M.run(hbv, inv, paths, lines.nested(), recorded_fasta=rec["fasta"])


@pytest.mark.parametrize("name", RECORDED)
def test_model_writes_the_recorded_files(records, name):
    case, kind, rec = records[name]
    got = _model(case, kind, rec)
    for k in ("fasta", "efasta", "src"):
        assert got[k] == rec[k], k
    assert M.stats_text(M.line_lengths(case["hbv"], rec["lines"].nested()), case["hbv"].K, "t_assembly").encode() == rec["stats"]


@pytest.mark.parametrize("name", [n for n in RECORDED if not n.startswith("gap_")])
def test_sort_lines_gives_the_recorded_order(records, name):
    case, kind, rec = records[name]
    nested = rec["lines"].nested()
    order = np.random.default_rng(len(name)).permutation(len(nested))
    assert M.sort_lines(case["hbv"], case["inv"], [nested[i] for i in order]) == nested


@pytest.mark.parametrize("name", sorted(C.TIE_BEST))
def test_ties_follow_std_sort(records, name):
    """the table of the ties: the lowest tied index up to 16 paths, not from 17 -- where the model reads the record"""
    case, kind, rec = records[name]
    got = _model(case, kind, rec)
    assert got["best"][1] == C.TIE_BEST[name] and got["counters"]["n_cells_tied"] == 1
    n = len(rec["lines"].nested()[0][1])
    cov = got["cov"][1:1 + n]
    assert max(cov) == 2 and cov[C.TIE_BEST[name]] == 2 and cov.count(2) in (2, 3)


def test_literal_votes(records):
    """derived by hand from Lines.cc:713-766"""
    got = _model(*records["bubble"])          # three reads on the 45-K-mer branch, one on the other strand, against one; a mirrored read's mate ends at e
    assert got["cov"][1:3] == [1, 3] and got["best"][1] == 1 and got["counters"]["n_match_several"] == 1
    got = _model(*records["read_ends"])       # 3 reads end at e (every path matches), 2 inside the shared branch (two match), 2 mirrored through {p, q2}, 1 through r
    assert got["cov"][1:4] == [0, 2, 1] and got["counters"]["n_match_several"] == 3 + 2 + 2 and got["counters"]["n_match_none"] == 0
    got = _model(*records["twice"])           # [a, b1, a, b2]: two entries x two occurrences, each path twice; one read through b2
    assert got["cov"][1:3] == [2, 3] and got["counters"]["n_occurrences"] == 5 and got["counters"]["n_entries"] == 3
    got = _model(*records["entries"])
    assert got["counters"]["n_entries"] == 0 + 1 + 63 + 64 + 65 + 257 and got["counters"]["n_cells_voted"] == 6
    got = _model(*records["circular"])
    assert got["counters"]["n_circular1"] == 1 and got["counters"]["n_circular2"] == 1 and got["printed"] == [1, 0, 1, 0]
    got = _model(*records["gap_2"])
    assert got["counters"]["n_gap_cells"] == 2 and got["counters"]["n_printed"] == 1 and got["fasta"].count(b"N") == 200


def test_literal_efasta(records):
    case, kind, rec = records["efasta_shares"]
    got = _model(case, kind, rec)
    K = case["hbv"].K
    # path 0 a prefix of path 1: the left share is all of path 0 (K-1 vertex bases + 30), nothing is left for the right one; the
    # shares that meet: K-1 + 2 from the left, 2 from the right, path 0's middle is empty
    assert sorted(zip(got["left_share"], got["right_share"]))[-2:] == [(K - 1 + 2, 2), (K - 1 + 30, 0)]
    assert b"{,T}" in rec["efasta"].replace(b"\n", b"") and got["efasta"] == rec["efasta"]


@pytest.mark.parametrize("name", MODEL_ONLY)
def test_model_only_cases_have_their_literal_outcomes(model_cases, name):
    case = model_cases[name]
    C.check_expect(case, M.run(case["hbv"], case["inv"], case["paths"], case["nested"]))


def test_layout_rows_text(model_cases):
    case = model_cases["layout_rows"]
    got = M.run(case["hbv"], case["inv"], case["paths"], case["nested"])
    rows = got["fasta"].split(b"\n")
    assert rows[0] == b">flattened_line_0" and len(rows[1]) == 79 and rows[2] == b">flattened_line_1" and len(rows[3]) == 80 and rows[4] == b">flattened_line_2"
    assert [len(r) for r in rows[5:7]] == [80, 1] and [len(r) for r in rows[8:10]] == [80, 80] and rows[10] == b">flattened_line_4"
    assert got["efasta"] == got["fasta"].replace(b">flattened_", b">")
    heads = [r for r in M.run(*(model_cases["layout_headers"][k] for k in ("hbv", "inv", "paths", "nested")))["efasta"].split(b"\n") if r.startswith(b">")]
    assert heads[9:11] == [b">line_9", b">line_10"] and heads[99:101] == [b">line_99", b">line_100"]

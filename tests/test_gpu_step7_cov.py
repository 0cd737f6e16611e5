"""w2rap_step7_coverage on the GPU held to the recorded runs of the reference (covs bit for bit, .lines.stats byte for byte, npairs, the
CN line), to the literal outcomes of the model-only cases, and to the model array for array: rule, the group records and every counter;
and the two forms of the long edges' count held to each other."""
import os

import numpy as np
import pytest

import step7_cov_cases as C
import step7_cov_model as M
from w2rap_contigger_amd import formats as F, step7

pytestmark = pytest.mark.gpu

RECORDED = sorted(C.recorded_cases())
MODEL_ONLY = sorted(C.model_cases())


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return C.recorded(tmp_path_factory.mktemp("cov"))


@pytest.fixture(scope="module")
def cn_records(tmp_path_factory):
    return C.cn_recorded(tmp_path_factory.mktemp("cn"))


@pytest.fixture(scope="module")
def model_cases():
    return C.model_cases()


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_files_and_model(records, name):
    case, rec = records[name]
    res = step7.coverage(case["hbv"], case["inv"], case["paths"], rec["lines"])
    assert F.int_vec_to_bytes(res.npairs) == rec["npairs"]
    assert F.covs_to_bytes([res.cov]) == rec["covs"]
    assert step7.line_stats_text(res, rec["lines"]).encode() == rec["stats"]
    C.compare(C.as_dict(res), M.run(case["hbv"], case["inv"], case["paths"], rec["lines"].nested()))


@pytest.mark.parametrize("name", C.CN_NAMES)
def test_recorded_cn_line(cn_records, name):
    hbv, paths, lines, text = cn_records[name]
    inv = step7.involution(hbv)
    res = step7.coverage(hbv, inv, paths, lines)
    assert res.cn_line() == text
    C.compare(C.as_dict(res), M.run(hbv, inv, paths, lines.nested()))


@pytest.mark.parametrize("name", MODEL_ONLY)
def test_model_only_cases(model_cases, name):
    case = model_cases[name]
    res = step7.coverage(case["hbv"], case["inv"], case["paths"], case["lines"])
    got = C.as_dict(res)
    C.check_expect(case, got)
    C.compare(got, M.run(case["hbv"], case["inv"], case["paths"], case["nested"]))
    assert step7.line_stats_text(res, case["lines"]) == M.line_stats_text(got, case["nested"])


LONG_CASES = ("entries", "pair_across_64", "inverse_in_group", "cell_named_twice", "inf_and_nan")


@pytest.mark.parametrize("name", LONG_CASES + ("rec_long_edges", "rec_reciprocal", "rec_no_pairs", "cn_repeats_snps"))
def test_sorted_and_sort_free_counts_agree(model_cases, records, cn_records, name):
    """the long edges' pairs by keys and one sort, and by flags and binary search: the same edges, the same counts (those of Pids), the
    same result"""
    if name.startswith("rec_"):
        case, rec = records[name[4:]]
        args = (case["hbv"], case["inv"], case["paths"], rec["lines"])
    elif name.startswith("cn_"):
        hbv, paths, lines, _ = cn_records[name[3:]]
        args = (hbv, step7.involution(hbv), paths, lines)
    else:
        case = model_cases[name]
        args = (case["hbv"], case["inv"], case["paths"], case["lines"])
    a, b = step7.coverage(*args, long_form="sorted"), step7.coverage(*args, long_form="sort_free")
    assert "k7c_single_flag" in step7.profile() or b.counters["n_group_entries"][1] == 0
    lst = lambda x: [] if x is None else x.tolist()              # (no long edge: null arrays)
    assert lst(a.long_edge) == lst(b.long_edge) and lst(a.long_pairs) == lst(b.long_pairs)
    po, pe = [int(x) for x in args[2][1]], [int(x) for x in args[2][2]]
    index = [[] for _ in range(len(args[0].edge_len))]
    for r in range(len(po) - 1):
        for e in pe[po[r]:po[r + 1]]:
            index[e].append(r)
    assert lst(a.long_pairs) == [len(M.pids(int(e), args[1], index)) for e in lst(a.long_edge)]
    assert a.counters["n_long_asked"] == len(lst(a.long_edge)) and (name not in ("entries", "rec_long_edges", "rec_no_pairs") or len(lst(a.long_edge)) > 0)
    C.compare(C.as_dict(b), C.as_dict(a))


def test_parts_and_parameters(model_cases):
    """npairs alone launches no kernel of the other parts; frac and min_edge_size reach CNIntegerFraction"""
    case = model_cases["cell_named_twice"]
    args = (case["hbv"], case["inv"], case["paths"], case["lines"])
    want = M.run(case["hbv"], case["inv"], case["paths"], case["nested"])
    res = step7.coverage(*args, parts=("npairs",))
    assert res.npairs.tolist() == want["npairs"] and res.llens.tolist() == want["llens"] and res.cov is None and res.covl is None and res.group_z is None
    assert not any(k.startswith("k7c_") or k.startswith("k5o_") for k in step7.profile())
    res = step7.coverage(*args, parts=("peak",))
    assert res.base_cov == want["base_cov"] and res.covx.tolist() == want["covx"] and res.cov is None and res.counters["index_built"] == 0
    res = step7.coverage(*args)
    prof = step7.profile()
    assert {"k7_pair_lines", "k7_line_stats", "k5o_index_emit", "k7c_row_len", "k7c_emit", "k7c_group_count", "k7c_line_pos", "k7c_cell_pos", "k7c_edge_cov", "k7c_edge_long"} <= set(prof)
    for frac, size in ((0.0, 2000), (0.5, 1020), (0.1, 1 << 30)):
        w = M.run(case["hbv"], case["inv"], case["paths"], case["nested"], frac=frac, min_edge_size=size)
        res = step7.coverage(*args, frac=frac, min_edge_size=size)
        assert (res.counters["n_cn_edges"], res.counters["n_cn_good"]) == (w["n_cn_edges"], w["n_cn_good"]) and C.bits64([res.cn_fraction]) == C.bits64([w["cn_fraction"]])


def test_no_index_without_groups_or_long_edges(records):
    """lone contigs: every edge has the line rule's value, nothing asks for the paths index"""
    case, rec = records["lone_few"]
    res = step7.coverage(case["hbv"], case["inv"], case["paths"], rec["lines"])
    assert res.counters["index_built"] == 0 and res.counters["n_long_asked"] == 0 and "k5o_index_emit" not in step7.profile()


def test_cli_writes_the_recorded_files(records, tmp_path, capsys):
    case, rec = records["bubbles_1000"]
    d = str(tmp_path)
    F.write_hbv(os.path.join(d, "t.contig.hbv"), case["hbv"]); F.write_paths(os.path.join(d, "t.contig.paths"), *case["paths"])
    F.write_lines(os.path.join(d, "the.lines"), rec["lines"])
    assert step7.main([d, "t", "--coverage", os.path.join(d, "the.lines")]) == 0
    for f, k in (("t_assembly.covs", "covs"), ("t_assembly.lines.npairs", "npairs"), ("t_assembly.lines.stats", "stats")):
        assert open(os.path.join(d, f), "rb").read() == rec[k], f
    want = M.run(case["hbv"], case["inv"], case["paths"], rec["lines"].nested())
    assert capsys.readouterr().out.strip().splitlines()[-1] == M.cn_line(want["cn_fraction"])
    assert [c.tobytes() for c in F.read_covs(os.path.join(d, "t_assembly.covs"))] == [want["cov"].tobytes()]

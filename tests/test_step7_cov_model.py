"""The model of ComputeCoverage, CNIntegerFraction and WriteLineStats (tests/step7_cov_model.py) held to the recorded runs of the
reference's main (tests/golden/refruns/step7_cov_* and step7_cn_*): covs bit for bit, .lines.stats byte for byte, npairs, the CN line as
text -- and to literal outcomes derived by hand.  No GPU."""
import numpy as np
import pytest

import step7_cov_cases as C
import step7_cov_model as M
from w2rap_contigger_amd import formats as F
from w2rap_contigger_amd.step7 import involution

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


_MODEL = {}


def model_of(records, name):
    if name not in _MODEL:
        case, rec = records[name]
        _MODEL[name] = M.run(case["hbv"], case["inv"], case["paths"], rec["lines"].nested())
    return _MODEL[name]


@pytest.mark.parametrize("name", RECORDED)
def test_model_gives_the_recorded_files(records, name):
    case, rec = records[name]
    got = model_of(records, name)
    print(name, "base_cov", got["base_cov"], "candidates", len(got["covx"]), "way", M.WAYS[got["counters"]["peak_way"]], "groups", len(got["groups"]), "rules", got["counters"]["n_rule"])
    assert F.int_vec_to_bytes(got["npairs"]) == rec["npairs"]
    assert F.covs_to_bytes([got["cov"]]) == rec["covs"]
    assert M.line_stats_text(got, rec["lines"].nested()).encode() == rec["stats"]


@pytest.mark.parametrize("name", C.CN_NAMES)
def test_model_prints_the_recorded_cn_line(cn_records, name):
    hbv, paths, lines, text = cn_records[name]
    got = M.run(hbv, involution(hbv), paths, lines.nested())
    print(name, text, "|", got["n_cn_good"], "/", got["n_cn_edges"])
    assert M.cn_line(got["cn_fraction"]) == text


def test_the_record_says_abs_is_the_floating_function(cn_records):
    """abs(int_cov - frac_cov) without std:: -- the integer function would truncate every difference to 0 and count every edge as good:
    the record of repeats_snps prints 0.8, 16 of 20"""
    hbv, paths, lines, text = cn_records["repeats_snps"]
    as_int = M.run(hbv, involution(hbv), paths, lines.nested(), abs_floating=False)
    assert text == "CN fraction good = 0.8" and M.cn_line(as_int["cn_fraction"]) == "CN fraction good = 1" and M.ABS_FLOATING
    hbv, paths, lines, text = cn_records["hand"]                  # the hand-staged contigs: copy numbers 1 (five), 1.3, 2.3 and 0.7, each with its mirror
    got = M.run(hbv, involution(hbv), paths, lines.nested())
    as_int = M.run(hbv, involution(hbv), paths, lines.nested(), abs_floating=False)
    assert text == "CN fraction good = 0.625" and (got["n_cn_good"], got["n_cn_edges"]) == (10, 16) and (as_int["n_cn_good"], as_int["n_cn_edges"]) == (16, 16)
    assert sorted(round(float(x), 1) for x in got["cov"]) == [0.7, 0.7] + [1.0] * 10 + [1.3, 1.3, 2.3, 2.3]
    assert cn_records["errs2"][3] == "CN fraction good = -nan"      # no edge of 2,000 bases has a defined coverage there: 0 / 0, printed as the C library prints it


def test_the_ways_of_the_peak_finder(records):
    """which branch each record takes: below 21 candidates the largest mass; a single peak; two peaks scored and the second halved"""
    way = lambda name: M.WAYS[model_of(records, name)["counters"]["peak_way"]]
    assert way("lone_few") == "largest_mass" and way("cand_20") == "largest_mass" and way("no_pairs") == "no_data" and way("pairs_on_short_only") == "no_data"
    assert len(model_of(records, "cand_20")["covx"]) == 20 and len(model_of(records, "cand_22")["covx"]) == 22
    assert model_of(records, "cand_20")["counters"]["n_simple"] == 0 and model_of(records, "cand_22")["counters"]["n_simple"] > 0      # the two sides of size > 2 * min_shoulder
    assert way("one_peak") == "single"
    two = model_of(records, "two_peaks")
    assert M.WAYS[two["counters"]["peak_way"]] == "scored" and two["counters"]["halved"] == 1
    assert model_of(records, "two_peaks_outlier")["counters"]["halved"] == 1
    few = model_of(records, "lone_few")
    assert few["min_len"] == 1500 and len(few["covx"]) == 8      # the contig of 1,100 K-mers, the best covered of all, is no candidate


def test_the_two_sides_of_1000(records):
    """branches of 999, 1,000 and 1,001 K-mers: the class of 999 is skipped, on the records alone"""
    case, rec = records["bubbles_1000"]
    got = model_of(records, "bubbles_1000")
    assert sorted(g["len"] for g in got["groups"]) == [1000, 1000, 1000, 1000, 1001, 1001] and got["counters"]["n_classes_short"] == 2
    covs = F.covs_from_bytes(rec["covs"])[0]
    lens = {int(case["hbv"].edge_len[e]) - C.K + 1: e for e in range(len(covs))}
    assert covs[lens[999]] == -1 and covs[lens[1001]] >= 0


def _recorded_cov(case, rec):
    covs = F.covs_from_bytes(rec["covs"])
    assert len(covs) == 1 and len(covs[0]) == len(case["hbv"].edge_len)
    return covs[0]


def test_the_long_edge_rule_at_999_and_1000(records):
    case, rec = records["long_edges"]
    covs = _recorded_cov(case, rec)
    kmers = [int(x) - C.K + 1 for x in case["hbv"].edge_len]
    assert [float(covs[e]) for e in range(len(kmers)) if kmers[e] == 999] == [-1.0, -1.0]
    # 4 + 2 + 1 + 3 = 10 distinct pairs on p or its inverse (the read through p twice counts once): 10 / 1000 / 0.005 = 2
    assert [float(covs[e]) for e in range(len(kmers)) if kmers[e] == 1000] == [2.0, 2.0]
    got = model_of(records, "long_edges")
    assert got["counters"]["n_cells_sizes"] == 4 and got["counters"]["n_rule"][3] == 2 and got["base_cov"] == 45 / 9000


def test_the_upper_median(records):
    """two parallel paths of 1,100 and 1,150 K-mers: 1,150; four of 1,100, 1,110, 1,140 and 1,150: v[2] = 1,140, not the mean of the middle two"""
    for name, want in (("parallel_2", 1150), ("parallel_4", 1140)):
        got = model_of(records, name)
        assert sorted(g["len"] for g in got["groups"]) == [want, want, 1200, 1200], name
        case, rec = records[name]
        covs = _recorded_cov(case, rec)
        g = next(g for g in got["groups"] if g["len"] == want)
        assert len(g["z"]) == 2 and all(C.bits32([covs[e]]) == C.bits32([np.float32(g["pairs"] / want / got["base_cov"])]) for e in g["z"]), name


def test_the_record_says_division_as_written(records):
    """the reciprocal search's line stands under each of the three rules in the record `reciprocal`: with x * (1.0 / base_cov) in any one
    of them the model leaves the recorded covs"""
    case, rec = records["reciprocal"]
    nested = rec["lines"].nested()
    m, L, nb, LB, q1, q2 = C.RECIPROCAL_HIT
    covs = _recorded_cov(case, rec)
    assert model_of(records, "reciprocal")["base_cov"] == nb / LB
    hit = [e for e in range(len(covs)) if int(case["hbv"].edge_len[e]) - C.K + 1 == L]
    assert len(hit) == 6 and all(float(covs[e]) == q1 for e in hit)
    for rule in ("line", "cell", "long"):
        other = M.run(case["hbv"], case["inv"], case["paths"], nested, recip={**M.RECIP, rule: True})
        assert sorted(float(other["cov"][e]) for e in hit) == [q2, q2, q1, q1, q1, q1], rule
        assert F.covs_to_bytes([other["cov"]]) != rec["covs"], rule
    assert M.RECIP == dict(line=False, cell=False, long=False)


def test_no_pairs_is_all_nan(records):
    case, rec = records["no_pairs"]
    covs = F.covs_from_bytes(rec["covs"])[0]
    assert np.isnan(covs).all() and rec["stats"].count(b" cov=?x\n") == len(covs)      # `defined` is true of a NaN, Def() inside is not: the -Ofast build
    case, rec = records["pairs_on_short_only"]
    assert b"cov=infx" in rec["stats"]


@pytest.mark.parametrize("name", MODEL_ONLY)
def test_model_only_cases_have_their_literal_outcomes(model_cases, name):
    case = model_cases[name]
    C.check_expect(case, M.run(case["hbv"], case["inv"], case["paths"], case["nested"]))


def test_reciprocal_hit_is_what_the_file_says():
    C.check_reciprocal_hit()


def test_covs_bytes_round_trip(tmp_path):
    a = np.array([1.5, -1.0, np.inf, 0.0], np.float32)
    F.write_covs(tmp_path / "x.covs", [a])
    back = F.read_covs(tmp_path / "x.covs")
    assert len(back) == 1 and back[0].tobytes() == a.tobytes()
    assert (tmp_path / "x.covs").read_bytes() == b"BINWRITE" + (1).to_bytes(8, "little") + (4).to_bytes(8, "little") + a.tobytes()

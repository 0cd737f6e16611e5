"""w2rap_step7_links on the GPU held to the recorded runs of the reference's main, to the recorded calls of the reference's own GetTol,
GetLineLengths, GetLineNpairs and MakeGaps on every case (replayed from tests/golden/refruns/step7_fn_*), to the literal outcomes of the
hand-made cases and to the CPU model (tests/step7_model.py), array for array, counters included -- at the shapes where a kernel can go wrong: 1, 63, 64, 65 and
257 pairs; runs of 1, 63, 64, 65, 256, 257 and 1025 equal nears; paths of 0, 1, 9, 17 and 40 edges (both sides of the per-thread lists);
an edge and its inverse in one line and in two; a hub of 300 edges in the search; more distinct links than a scan tile holds; medians of
3 to 7 parallel paths; the search through in-edges (steps 1 to 3, the 1500 K-mer limit, a first level of 140 with the out/in boundary
behind lane 63); y of 16 and 17 kept edges; 1, 3, 4 and 5 candidates of the search."""
import numpy as np
import pytest

import step7_cases as C
import step7_model as M
from w2rap_contigger_amd import formats as F, step7

pytestmark = pytest.mark.gpu

HAND = C.hand_cases()
GENERATED = C.generated_cases()
_MODEL = {}


def model(name, case, parts):
    key = (name, parts)
    if key not in _MODEL:
        _MODEL[key] = M.run(case["hbv"], case["inv"], case["paths"], case["nested"], npairs=case["npairs"], min_line=case["min_line"], min_link_count=case["min_link_count"],
                            parts=parts, shortcut_last=name == "hub_300")
    return _MODEL[key]


def library(case, parts):
    return step7.run(case["hbv"], case["inv"], case["paths"], case["lines"], parts=parts, npairs=case["npairs"], min_line=case["min_line"], min_link_count=case["min_link_count"])


def same(res, want):
    """every array and every counter the model has, and nothing of a part that was not asked for"""
    for k in step7.ARRAYS:
        if k in want:
            assert res.arrays[k] is not None and np.array_equal(res.arrays[k].astype(np.int64), np.array(want[k], np.int64)), k
        else:
            assert res.arrays[k] is None, k
    for k in step7.LINES_COUNTERS + step7.LINKS_COUNTERS:
        assert res.counters[k] == want["counters"].get(k, [0] * len(res.counters[k]) if isinstance(res.counters[k], list) else 0), (k, res.counters[k])


def parts_of(case):
    return ("lines", "links") if case["npairs"] is None else ("links",)


def held_to_the_records(name, case, res, tmp_path):
    """the recorded calls of the reference's own GetTol, GetLineLengths, GetLineNpairs and MakeGaps on this case (refruns/step7_fn_<name>/,
    replayed): tol, llens, npairs where part LINES ran; the gaps with their ids and mirror indices, in order; the accepted links, their
    nears' longest runs, edge groups and lines; the one-to-one and the symmetry counts"""
    got = C.as_dict(res)
    C.check_lines_record(C.lines_run(name, case, str(tmp_path)), got)
    C.check_gaps_record(C.gaps_run(name, case, str(tmp_path)), got)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases(name, tmp_path):
    case = HAND[name]
    res = library(case, parts_of(case))
    C.check_expect(case, C.as_dict(res))
    held_to_the_records(name, case, res, tmp_path)
    same(res, model(name, case, parts_of(case)))


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_cases(name, tmp_path):
    case = GENERATED[name]
    res = library(case, parts_of(case))
    held_to_the_records(name, case, res, tmp_path)
    same(res, model(name, case, parts_of(case)))
    assert all(v >= 0 for v in res.ms.values())


@pytest.mark.parametrize("name", ("long_paths", "inverse_in_line", "random_2000"))
def test_lines_alone(name):
    case = GENERATED[name]
    res = step7.line_stats(case["hbv"], case["inv"], case["paths"], case["lines"])
    same(res, model(name, case, ("lines",)))
    assert res.ms["ms_nears"] == 0 and res.ms["ms_search"] == 0 and res.ms["ms_filter"] == 0


@pytest.mark.parametrize("name", sorted({**HAND, **GENERATED}))
def test_lines_are_the_recorded_ones(name, tmp_path):
    """part LINES alone on every case, whether it gives npairs or not: the recorded tol, llens and npairs, value for value"""
    case = {**HAND, **GENERATED}[name]
    res = step7.line_stats(case["hbv"], case["inv"], case["paths"], case["lines"])
    assert res.npairs is not None
    C.check_lines_record(C.lines_run(name, case, str(tmp_path)), C.as_dict(res))


def test_links_read_the_given_npairs_not_their_own():
    """LINES and LINKS in one call with npairs given: LINES returns what it counts, LINKS filters by the GIVEN values (one side without
    pairs: the coverage test rejects what the counted values accept)"""
    case = HAND["count_3"]
    res = step7.run(case["hbv"], case["inv"], case["paths"], case["lines"], parts=("lines", "links"), npairs=[0, 0, 5, 5])
    assert res.npairs.tolist() == [3, 3, 3, 3] and [step7.REASONS[r] for r in res.link_reason] == ["coverage", "coverage"] and res.counters["n_gaps"] == 0
    assert step7.find_gaps(case["hbv"], case["inv"], case["paths"], case["lines"]).gaps() == [(0, 2), (3, 1)]


@pytest.mark.parametrize("name", C.S6_FIXTURES)
def test_lines_give_the_reference_npairs(name, tmp_path):
    """(a): what the reference's Step 6 wrote as .fin.lines.npairs, byte for byte"""
    hbv, paths, lines, npairs = C.step6_run(name, str(tmp_path))
    res = step7.line_stats(hbv, step7.involution(hbv), paths, lines)
    assert F.int_vec_to_bytes(res.npairs) == open(tmp_path / "t.fin.lines.npairs", "rb").read()
    want = M.run(hbv, step7.involution(hbv), paths, lines.nested(), parts=("lines",))
    same(res, want)


@pytest.mark.parametrize("name", ("planted",) + C.S7_HAND)
def test_gaps_are_the_reference_gaps(name, tmp_path):
    """(b): the gaps of the reference's t_assembly_raw.gfa by flank sequence, and the symmetry counts of its stdout"""
    case = (C.planted_case() if name == "planted" else C.hand_cases(real=True)[name])
    gfa, (deleted, added) = C.step7_run(name, case, str(tmp_path))
    res = step7.find_gaps(case["hbv"], case["inv"], case["paths"], case["lines"], npairs=F.read_int_vec(tmp_path / "t.fin.lines.npairs"))
    C.check_gaps_against_gfa(gfa, case, res.gap_from, res.gap_to, res.gap_inv)
    assert (res.counters["n_sym_deleted"], res.counters["n_sym_added"]) == (deleted, added)


def test_command_line(tmp_path):
    """python -m w2rap_contigger_amd.step7 DIR PREFIX on the four files of the planted case"""
    case = C.planted_case()
    C.step7_run("planted", case, str(tmp_path))
    assert step7.main([str(tmp_path), "t"]) == 0
    text = open(tmp_path / "t.gaps.txt").read().splitlines()
    res = step7.find_gaps(case["hbv"], case["inv"], case["paths"], case["lines"], npairs=case["npairs"])
    assert text[:-1] == [f"{f} {t} {i}" for (f, t), i in zip(res.gaps(), res.gap_inv.tolist())] and len(text) == 3
    assert text[-1] == "# deleting 0 gaps and adding 0 gaps to force symmetry"


def test_profile_names_the_kernels():
    library(GENERATED["runs"], ("lines", "links"))
    p = step7.profile()
    for k in ("k7_path_len", "k7_line_stats", "k7_pair_lines", "k7_nears_count", "k7_nears_fill", "k7_heads", "k7_kinds", "k7_kind_max", "k7_close", "k7_link_flag", "k7_link_fill",
              "k7_filter"):
        assert k in p and p[k][1] >= 1, k


def test_empty_inputs():
    """no pairs; no graph at all"""
    g = C.Contigs(1); g.contig(); g.contig()
    case = g.case()
    res = library(case, ("lines", "links"))
    same(res, model("no_pairs", case, ("lines", "links")))
    empty = F.HBV(20, np.zeros(1, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                  np.zeros(0, np.uint32))
    res = step7.run(empty, np.zeros(0, np.int32), (np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, np.int32)), F.Lines.from_nested([]))
    assert res.counters["n_gaps"] == 0 and res.counters["n_pairs"] == 0 and len(res.tol) == 0

"""The CPU model of Step 7's read-sized passes (tests/step7_model.py) held to the recorded runs of the reference's own main
(tests/golden/refruns/step7_s6_*, step7_s7_*), to the recorded calls of its own GetTol, GetLineLengths, GetLineNpairs and MakeGaps on every
hand-made and generated case (refruns/step7_fn_*) and to the literal outcomes of the hand-made cases (tests/step7_cases.py); the file formats of the
lines and of npairs held to the reference's files; and the things that do not exist without the feature."""
import ctypes

import pytest

import step7_cases as C
import step7_model as M
from w2rap_contigger_amd import formats as F, step7

HAND = C.hand_cases()


def model(case, **kw):
    parts = ("lines", "links") if case["npairs"] is None else ("links",)
    return M.run(case["hbv"], case["inv"], case["paths"], case["nested"], npairs=case["npairs"], min_line=case["min_line"], min_link_count=case["min_link_count"],
                 parts=kw.pop("parts", parts), **kw)


# ---- what fails without the feature
def test_the_module_the_entry_and_the_readers_exist():
    from w2rap_contigger_amd.step2 import lib
    L = lib()
    for sym in ("w2rap_step7_links", "w2rap_step7_free", "w2rap_step7_profile"):
        assert isinstance(getattr(L, sym), ctypes._CFuncPtr), sym
    assert callable(F.read_lines) and callable(F.write_lines) and callable(F.read_int_vec) and callable(F.write_int_vec)
    assert callable(step7.line_stats) and callable(step7.find_gaps)


# ---- formats
@pytest.mark.parametrize("name", C.S6_FIXTURES)
def test_lines_and_npairs_files_round_trip(name, tmp_path):
    C.step6_run(name, str(tmp_path))
    raw = open(tmp_path / "t.fin.lines", "rb").read()
    lines = F.read_lines(tmp_path / "t.fin.lines")
    assert F.lines_to_bytes(lines) == raw
    F.write_lines(tmp_path / "again.lines", F.Lines.from_nested(lines.nested()))
    assert open(tmp_path / "again.lines", "rb").read() == raw
    F.write_int_vec(tmp_path / "again.npairs", F.read_int_vec(tmp_path / "t.fin.lines.npairs"))
    assert open(tmp_path / "again.npairs", "rb").read() == open(tmp_path / "t.fin.lines.npairs", "rb").read()


def test_readers_refuse_broken_files(tmp_path):
    good = F.lines_to_bytes(F.Lines.from_nested([[[[1, 2]], [[3], []], [[4]]]]))
    for name, raw in (("magic", b"BINWRITX" + good[8:]), ("truncated", good[:-3]), ("trailing", good + b"\0"), ("huge", good[:8] + (2 ** 40).to_bytes(8, "little") + good[16:])):
        (tmp_path / name).write_bytes(raw)
        with pytest.raises(ValueError):
            F.read_lines(tmp_path / name)
    v = F.int_vec_to_bytes([1, -2, 3])
    for name, raw in (("vmagic", b"X" + v[1:]), ("vshort", v[:-1]), ("vlong", v + b"\0\0\0\0")):
        (tmp_path / name).write_bytes(raw)
        with pytest.raises(ValueError):
            F.read_int_vec(tmp_path / name)
    (tmp_path / "ok").write_bytes(v)
    assert F.read_int_vec(tmp_path / "ok").tolist() == [1, -2, 3]
    (tmp_path / "none").write_bytes(F.lines_to_bytes(F.Lines.from_nested([])))
    assert F.read_lines(tmp_path / "none").n_lines == 0


# ---- the model against the recorded runs
@pytest.mark.parametrize("name", C.S6_FIXTURES)
def test_model_counts_the_reference_npairs(name, tmp_path):
    """(a): GetLineNpairs as the reference's Step 6 wrote it"""
    hbv, paths, lines, npairs = C.step6_run(name, str(tmp_path))
    got = M.run(hbv, step7.involution(hbv), paths, lines.nested(), parts=("lines",))
    assert F.int_vec_to_bytes(got["npairs"]) == open(tmp_path / "t.fin.lines.npairs", "rb").read()
    assert got["counters"]["n_line_hits"] == int(npairs.sum())


def s7_cases():
    real = C.hand_cases(real=True)
    return {"planted": C.planted_case(), **{n: real[n] for n in C.S7_HAND}}


@pytest.mark.parametrize("name", ("planted",) + C.S7_HAND)
def test_model_finds_the_reference_gaps(name, tmp_path):
    """(b): the gaps of the reference's t_assembly_raw.gfa by flank sequence, and the symmetry counts of its stdout"""
    case = s7_cases()[name]
    gfa, (deleted, added) = C.step7_run(name, case, str(tmp_path))
    got = M.run(case["hbv"], case["inv"], case["paths"], case["nested"], npairs=F.read_int_vec(tmp_path / "t.fin.lines.npairs"), parts=("links",))
    C.check_gaps_against_gfa(gfa, case, got["gap_from"], got["gap_to"], got["gap_inv"])
    assert (got["counters"]["n_sym_deleted"], got["counters"]["n_sym_added"]) == (deleted, added)
    final = F.read_lines(tmp_path / "t_assembly.lines")              # the lines FinalFiles found behind the gaps: the readers take them too
    assert F.lines_to_bytes(final) == open(tmp_path / "t_assembly.lines", "rb").read()
    assert len(F.read_int_vec(tmp_path / "t_assembly.lines.npairs")) == final.n_lines
    if case["npairs"] is not None:            # (the literal outcomes hold for the real sequences too; count_2 / count_3 state theirs with part LINES)
        C.check_expect(case, got)


def test_the_records_hold_an_accepted_gap_and_a_filtered_link(tmp_path):
    seen = set()
    for name, case in s7_cases().items():
        d = tmp_path / name
        d.mkdir()
        ref_gaps = C.gfa_half_gaps(C.step7_run(name, case, str(d))[0])
        got = M.run(case["hbv"], case["inv"], case["paths"], case["nested"], npairs=F.read_int_vec(d / "t.fin.lines.npairs"), parts=("links",))
        seen |= {"gap"} if ref_gaps else set()
        seen |= {"filtered"} if any(r != M.R_ACCEPTED for r in got["link_reason"]) else set()
    assert seen == {"gap", "filtered"}


# ---- the model against the recorded calls of the reference's own functions (refruns/step7_fn_<case>/): every case of step7_cases.py
GENERATED = C.generated_cases()
ALL = {**HAND, **GENERATED}


@pytest.mark.parametrize("name", sorted(ALL))
def test_model_gives_the_reference_tol_llens_npairs(name, tmp_path):
    """GetTol, GetLineLengths and GetLineNpairs, value for value (part LINES for every case, whether it gives npairs or not)"""
    case = ALL[name]
    rec = C.lines_run(name, case, str(tmp_path))
    got = model(case, parts=("lines",))
    assert got["npairs"] is not None
    C.check_lines_record(rec, got)
    if "npairs" in case["expect"]:            # (the literal is the recorded value too)
        assert case["expect"]["npairs"] == rec["npairs"]


@pytest.mark.parametrize("name", sorted(ALL))
def test_model_makes_the_reference_gaps(name, tmp_path):
    """MakeGaps: its gap edges with their own ids, in its order, and what its verbose text states about every accepted link"""
    case = ALL[name]
    rec = C.gaps_run(name, case, str(tmp_path))
    got = model(case, shortcut_last=name == "hub_300")
    C.check_lines_record(C.lines_run(name, case, str(tmp_path)), got)
    C.check_gaps_record(rec, got)
    assert F.read_int_vec(tmp_path / "t.fin.lines.npairs").tolist() == (case["npairs"].tolist() if case["npairs"] is not None else got["npairs"])


@pytest.mark.parametrize("a,b", C.BOUNDARY_PAIRS)
def test_the_records_show_the_verdict_of_a_boundary_pair(a, b, tmp_path):
    """on the records alone: the two sides of a limit differ in the gaps the reference made -- one side has none, the other two.  (A case
    that drifted into `rejected for another reason` on both sides fails here)"""
    gaps = []
    for name in (a, b):
        d = tmp_path / name
        d.mkdir()
        C.gaps_run(name, HAND[name], str(d))
        gaps.append(open(d / "t.gaps.txt").read())
    assert gaps[0] != gaps[1] and sorted(len(g.splitlines()) for g in gaps) == [0, 2], gaps


def test_the_records_reach_what_the_new_cases_are_for():
    """the medians are the literal ones; the in-edge searches are close or not as derived; y of 16 and 17; 1, 3, 4 and 5 candidates"""
    for n, (lens, med) in C.MEDIANS.items():
        assert M.line_lengths(M.Graph(HAND[f"median_{n}"]["hbv"]), HAND[f"median_{n}"]["nested"])[-1] == 2 * C.LONG + med and len(lens) == n
    assert [model(HAND[f"kinds_{k}"])["counters"]["n_near_kinds"] for k in (1, 3, 4, 5)] == [1, 3, 4, 5]
    assert [model(HAND[f"y_{n}"])["counters"]["n_pass_y_long"] for n in (16, 17)] == [0, 3]


# ---- the model against the literal outcomes
@pytest.mark.parametrize("name", sorted(HAND))
def test_model_literal_outcomes(name):
    C.check_expect(HAND[name], model(HAND[name]))


def test_real_sequences_change_nothing():
    real = C.hand_cases(real=True)
    for name in C.S7_HAND:
        a, b = model(HAND[name]), model(real[name])
        assert a == b, name
        assert real[name]["inv"].tolist() == step7.involution(real[name]["hbv"]).tolist()


# ---- the model against itself: the queue with its third level enumerated, and with the last step asked instead
@pytest.mark.parametrize("name", ("pairs_65", "pairs_257", "long_paths"))
def test_last_step_shortcut_changes_nothing(name):
    case = C.generated_cases()[name]
    assert model(case) == model(case, shortcut_last=True)


def test_generated_cases_reach_the_branches():
    """the generated cases are there for the kernels' shapes: they must reach what they are meant to reach"""
    g = C.generated_cases()
    c = model(g["long_paths"])["counters"]
    assert c["n_pairs_spilled"] > 0 and c["n_pairs_listed"] > 0 and c["n_pairs_no_path"] > 0 and c["n_pass_y_long"] > 0
    assert sorted(set(model(g["runs"])["link_count"])) == [1, 63, 64, 65, 256, 257, 1025]
    r = model(g["inverse_in_line"], parts=("lines",))
    assert r["tol"][0] == r["tol"][1] and r["npairs"][r["tol"][0]] == 7 and r["tol"][2] != r["tol"][3]
    h = model(g["hub_300"], shortcut_last=True)["counters"]
    assert h["n_close"][2] >= 1 and h["n_close"][3] >= 1 and h["n_links"] >= 1
    assert model(g["many_links"])["counters"]["n_links"] > 4096
    big = model(g["random_2000"])["counters"]
    assert big["n_gaps"] > 0 and big["n_group_loop1"] > 0 and sum(big["n_close"]) > 0 and min(big["n_reason"][:3]) > 0

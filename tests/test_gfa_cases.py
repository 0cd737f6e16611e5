"""The GFA-dump oracle (oracle/oracle_gfa.py) on the hand-made and generated graphs of gfa_cases.py: against the recorded runs of the
reference tool (tests/golden/refruns/gfa_case_<name>/, recorded by `make_golden.py refruns tests/test_gfa_cases.py` at 1 thread and at
4, which had to agree), against the cases' literal L lines and S ids, and against the cases' own involution.  No GPU."""
import hashlib

import numpy as np
import pytest

import gfa_cases as G
from oracle import oracle_gfa as OG


def split(text):
    """-> (the ids of the S lines, the L lines) of a _raw.gfa"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    return [int(l.split(b"\t")[1][4:]) for l in lines if l[:1] == b"S"], [l for l in lines if l[:1] == b"L"]


def test_every_case_is_recorded_or_accounted_for():
    assert set(G.NOT_RECORDED) <= set(G.all_names()) and not set(G.NOT_RECORDED) & set(G.ORACLE_ONLY)
    assert len(G.recorded()) + len(G.NOT_RECORDED) + len(G.ORACLE_ONLY) == len(G.all_names())


@pytest.mark.parametrize("name", G.recorded())
def test_gfa_oracle_equals_the_recorded_reference(name, tmp_path):
    raw, digest, stats = G.reference_run(name, str(tmp_path))
    c = G.case_of(name)
    got = G.oracle_of(name)[0]
    assert raw is None or got == raw
    assert hashlib.sha256(got).hexdigest() == digest
    assert OG.stats_text(c.hbv(), 1000 * c.genome_kb) == stats


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_gfa_oracle_gives_the_literals(name):
    c = G.case_of(name)
    text, inv = G.oracle_of(name)
    s_ids, l_lines = split(text)
    assert s_ids == sorted(c.s_ids)
    if c.lines is not None:
        assert set(c.lines) <= set(l_lines)
        assert l_lines == c.lines                     # and nothing else, in this order
    assert np.array_equal(inv, c.inv)


def test_chunk_writer_case_meets_what_it_was_built_for():
    c, lacks = G._chunk_case(G.CHUNK_SEED)
    assert lacks == []
    lens = c.s_line_lengths()
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert set(int(s) % 16 for s in starts) == set(range(16)) and min(lens) == 21 and c.hbv().n_edges >= 100
    assert sorted(set(int(x) for x in c.hbv().edge_len)) == list(range(1, 49))


def test_canonical_form_case_holds_every_path():
    from oracle import oracle as O
    c = G.case_of("canonical_forms")
    forms = {}
    for e, (_, _, s) in enumerate(c.b.edges):
        forms.setdefault((len(s), O.eform(s)), []).append(e)
    for n in (1,) + G.FORM_ODD:
        assert (n, 0) in forms and (n, 1) in forms
    for n in (3, 5, 7, 63, 65):
        assert {int(c.b.edges[e][2][n // 2]) for e in forms[(n, 0)] + forms[(n, 1)]} == {0, 1, 2, 3}
    for n in G.FORM_PALINDROMES:
        assert (n, 0) in forms and (n, 1) in forms and (n, 2) in forms
    for e in sorted(c.s_ids):
        assert O.eform(c.b.edges[e][2]) != 1


def test_digit_chain_reaches_every_digit_count():
    """the 1,000-object prefix (recorded) covers ids of up to three digits, the 100,002-object chain (oracle only) up to six"""
    assert G.digit_conditions(G.oracle_of("digits_1000")[0], 1000) == []
    c = G.case_of("digits_100002")
    assert c.hbv().n_edges == 100002
    text, inv = G.oracle_of("digits_100002")
    assert G.digit_conditions(text, 100002) == []
    assert np.array_equal(inv, c.inv) and split(text)[0] == sorted(c.s_ids)


def test_hub_has_300_edges_on_either_side():
    h = G.case_of("hub_300").hbv()
    assert int(np.max(np.diff(h.from_off.astype(np.int64)))) == 300 and int(np.max(np.diff(h.to_off.astype(np.int64)))) == 300
    text = G.oracle_of("hub_300")[0]
    assert text.count(b"\nL\t") == 300 * 300 and len(text) > (1 << 20)     # why its file is recorded by digest


def test_statistics_lists_tell_the_two_rules_apart():
    """from the two formulas alone: 20 of the 24 lists differ on an N line.  None can differ on an NG line at a genome size of 1000
    (see find_stats_lists); the lists are the ones the seeded search finds"""
    assert len(G.STATS_LISTS) == 24 and G.STATS_LISTS == G.find_stats_lists()
    dn, dg = G.stats_rules_differ()
    assert dn >= 20 and dg == 0
    for d in range(1, 10):
        assert G.reassociated(100 * d, 1000) >= 10 * d
    assert G.walk(range(1, 40), 780, False, G.reassociated)[8] == "12" and G.walk(range(1, 40), 780, False, G.ieee)[8] == "13"
    assert G.walk([300, 200], 1000, True, G.reassociated) == ["300"] * 3 + ["n/a"] * 6
    # with the sum of a list as the genome size the NG walk meets the same exact deciles
    assert sum(G.walk(s, sum(s), True, G.ieee) != G.walk(s, sum(s), True, G.reassociated) for s in G.STATS_LISTS) >= 10


@pytest.mark.parametrize("seed", G.SEEDS)
def test_generated_cases_hold_what_they_must(seed):
    name = f"random_{seed}"
    c = G.case_of(name)
    text, inv = G.oracle_of(name)
    assert G.seed_conditions(c, text, inv) == []
    assert np.array_equal(inv, c.inv) and split(text)[0] == sorted(c.s_ids)
    assert 1 <= int(min(c.hbv().edge_len)) and int(max(c.hbv().edge_len)) <= 120

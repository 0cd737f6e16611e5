"""The GFA dump on the GPU (gfa.gfa_dump) on the hand-made and generated graphs of gfa_cases.py: the recorded output of the reference
tool byte for byte and its statistics text (tests/golden/refruns/gfa_case_<name>/), the oracle's text where no run is recorded, the
cases' literal lines, the oracle's involution.  Reads recorded files only."""
import hashlib

import numpy as np
import pytest

import gfa_cases as G
from test_gfa_cases import split
from w2rap_contigger_amd import formats as F, gfa
from oracle import oracle_gfa as OG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"


@pytest.mark.parametrize("name", G.all_names())
def test_gpu_gfa_case(name, tmp_path):
    c = G.case_of(name)
    h = c.hbv()
    gs = 1000 * c.genome_kb
    r = gfa.gfa_dump(h, gs)
    want, inv = G.oracle_of(name)
    if name in G.recorded():
        raw, digest, stats = G.reference_run(name, str(tmp_path))
        assert raw is None or r.gfa == raw
        assert hashlib.sha256(r.gfa).hexdigest() == digest
        assert r.stats_text() == stats
    assert r.gfa == want and r.stats_text() == OG.stats_text(h, gs)
    s_ids, l_lines = split(r.gfa)
    assert s_ids == sorted(c.s_ids)
    if c.lines is not None:
        assert set(c.lines) <= set(l_lines) and l_lines == c.lines
    assert np.array_equal(r.inv, inv) and np.array_equal(r.inv, c.inv)
    assert r.n_segments == len(s_ids) and r.n_links == len(l_lines) and r.gfa_len == len(r.gfa)
    assert r.segment_bytes == sum(c.s_line_lengths())
    q = gfa.gfa_dump(h, gs, flags=gfa.NO_FETCH)
    assert q.gfa == b"" and q.gfa_len == len(r.gfa) and q.n_links == r.n_links and q.stats_text() == r.stats_text()
    if name == "digits_100002":
        assert G.digit_conditions(r.gfa, 100002) == []


@pytest.mark.parametrize("i", range(len(G.STATS_LISTS)))
def test_gpu_gfa_statistics_at_other_genome_sizes(i):
    """the lists again at genome sizes that are no multiple of 1000 (the reference takes whole kb only): the oracle is the expectation.
    At the sum of the list the NG walk lands on the same exact deciles as the N walk"""
    sizes = G.STATS_LISTS[i]
    h = G.case_of(f"stats_{i:02d}").hbv()
    for gs in (1234, sum(sizes), sum(sizes) + 1):
        r = gfa.gfa_dump(h, gs, flags=gfa.STATS_ONLY)
        assert r.stats_text() == OG.stats_text(h, gs)
        n = [str(v) for v in r.nxx]
        assert n == G.walk(sizes, sum(sizes), False, G.reassociated)
        assert ["n/a" if v < 0 else str(v) for v in r.ngxx] == G.walk(sizes, gs, True, G.reassociated)


def test_gpu_gfa_of_the_empty_graph():
    """literals only: the reference divides by zero here"""
    z64, z32 = np.zeros(1, np.uint64), np.zeros(0, np.int32)
    h = F.HBV(G.K, z64, z32, z32, z64.copy(), z32, np.zeros(0, np.uint8), z64.copy(), np.zeros(0, np.uint32))
    for gs in (0, 1000):
        r = gfa.gfa_dump(h, gs)
        assert r.gfa == b"" and r.gfa_len == 0 and r.n_segments == 0 and r.n_links == 0 and list(r.nxx) == [0] * 9 and len(r.inv) == 0
        assert r.canonical_size == 0 and r.n_canonical == 0

"""The absence filter whose word comes from the minimizer windows at every FMER_STRIDE-th offset (csrc/common.h fmer_key, k_filter32 of
csrc/step2_graph.hip) and the adjacency sort over the bits a vertex pair can hold (graph_finish): runs of equal words on every wavefront
and block edge, streams that are one run or end a run at every position class, read pathing on reads with one substitution where probe3,
the diagonal check and the ladder decide -- through the dictionary, the index and without the filter -- and graphs whose vertex count sits
on the digit edges of the narrowed sort."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    from w2rap_contigger_amd import formats as F, step2
    from oracle import oracle as O
    return F, step2, O


# ---------------------------------------------------------------------------------------------- the builder against the host loop
SLICES = [(0, 16), (5, 11)]                                          # the whole filter; a slice of its words, as filter32_slice builds it


@pytest.mark.parametrize("lo,hi", SLICES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025])
def test_random_stream_runs_on_every_wavefront_and_block_edge(mods, n, lo, hi):
    """n 31-mer positions of a random stream: runs of equal words (about five positions long on two interleaved chains at stride 2) begin and end on both sides
    of every wavefront (64) and block (256) edge, and one position past them"""
    F, step2, O = mods
    L = step2.lib()
    L.w2rap_step2_selftest_filter32.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.w2rap_step2_selftest_filter32.restype = C.c_int
    with step2.Step2Context(0) as ctx:
        assert L.w2rap_step2_selftest_filter32(ctx.h, 30 + n, 7000 + n, lo, hi) == 0


@pytest.mark.parametrize("lo,hi", SLICES)
@pytest.mark.parametrize("n", [64, 257, 1025])
@pytest.mark.parametrize("period", [1, 2, 3, 4, 17])
def test_periodic_stream_equals_the_host_loop(mods, period, n, lo, hi):
    """a stream that repeats its first `period` bases: with period 1 the whole stream is ONE run in one word (every wavefront's first lane
    is a head, and nothing else); period p has p words that come round every p positions -- with 17 a run ends at every position class"""
    F, step2, O = mods
    L = step2.lib()
    L.w2rap_step2_selftest_filter32_periodic.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    L.w2rap_step2_selftest_filter32_periodic.restype = C.c_int
    with step2.Step2Context(0) as ctx:
        for seed in (1, 2, 3):
            assert L.w2rap_step2_selftest_filter32_periodic(ctx.h, 30 + n, period, 100 * period + seed, lo, hi) == 0


# ---------------------------------------------------------------------------------------------- Step 2 behind it
def _run_step2(mods, codes, quals, off):
    F, step2, O = mods
    pk, bo, ln = F.pack_bases(codes, off)
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=quals, qual_off=off)
        ctx.count_kmers(7, 4)
        ctx.build_graph(None)
        ctx.path_reads()
        return ctx.fetch()


def _equals_oracle(mods, res, orc):
    F, step2, O = mods
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)


_SUBST = {}


def _substituted_reads(O):
    """a 20 kb genome; 150-base reads every 10 bases without errors (what makes its 60-mers solid) and reads of 60, 61, 90, 91 and 150 bases
    with ONE substituted base at 0, 29, 30, 59, 60, 89, 90 or the last base: the spoilt k-mers reach the read's start, its end or neither,
    and the 31-mers asked for sit on the `tmax` / `last` clamps of the short reads.  The oracle's Step 2, computed once."""
    if not _SUBST:
        rng = np.random.default_rng(2231)
        G = 20000
        g = rng.integers(0, 4, G, dtype=np.uint8)
        reads = [g[s:s + 150] for s in range(0, G - 150 + 1, 10)]
        for L in (60, 61, 90, 91, 150):
            for e in sorted({0, 29, 30, 59, 60, 89, 90, L - 1}):
                if e >= L:
                    continue
                for s in rng.integers(0, G - L + 1, 48):
                    r = g[s:s + L].copy()
                    r[e] = (r[e] + rng.integers(1, 4)) & 3
                    reads.append(r if rng.integers(0, 2) else (3 - r[::-1]).astype(np.uint8))
        codes = np.concatenate(reads)
        off = np.zeros(len(reads) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in reads])
        quals = np.full(len(codes), 40, np.uint8)
        _SUBST["case"] = (codes, quals, off, O.run(codes, quals, off))
    return _SUBST["case"]


@pytest.mark.parametrize("route", ["dictionary", "index", "no_filter"])
def test_paths_of_reads_with_one_substitution(mods, monkeypatch, route):
    """the same paths and graph bytes as the oracle whether read pathing asks the dictionary, the index (W2RAP_PATH_INDEX=1) or has no
    filter at all (W2RAP_NO_FILTER32=1: every absent k-mer is found absent one by one)"""
    F, step2, O = mods
    if route == "index":
        monkeypatch.setenv("W2RAP_PATH_INDEX", "1")
    if route == "no_filter":
        monkeypatch.setenv("W2RAP_NO_FILTER32", "1")
    codes, quals, off, orc = _substituted_reads(O)
    assert len(off) - 1 > 3000 and orc.n_vertices > 0
    _equals_oracle(mods, _run_step2(mods, codes, quals, off), orc)


# ---------------------------------------------------------------------------------------------- the adjacency sort
@pytest.mark.parametrize("NV", [254, 256, 258, 65534, 65536, 65538])
def test_adjacency_order_at_the_digit_edges_of_the_vertex_bits(mods, NV):
    """graph_finish sorts the keys (this vertex << w | other vertex) over 2 w bits, w = the bits of NV - 1: 2^8 and 2^16 vertices are the
    last counts with w = 8 and 16 (two and four whole digits), two vertices more take a ninth and a seventeenth bit (a last digit of two
    bits).  A vertex is a 59-mer and never its own reverse complement (odd length), so vertices come in pairs and NV is even: 255, 257,
    65 535 and 65 537 do not exist, their even neighbours stand in.  Disjoint contigs of 61 bases (four vertices each: two ends, two
    strands) and one circle of 70 (two vertices), every read four times; the .hbv bytes hold the adjacency in the sorted order."""
    F, step2, O = mods
    rng = np.random.default_rng(NV)
    n_lin, n_circ = NV // 4, (NV % 4) // 2
    reads = []
    for _ in range(n_lin):
        c = rng.integers(0, 4, 61, dtype=np.uint8)
        reads += [c] * 4
    for _ in range(n_circ):
        c = rng.integers(0, 4, 70, dtype=np.uint8)
        reads += [np.concatenate([c, c])[:130]] * 4
    codes = np.concatenate(reads)
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    quals = np.full(len(codes), 40, np.uint8)
    orc = O.run(codes, quals, off)
    assert orc.n_vertices == NV
    res = _run_step2(mods, codes, quals, off)
    assert res.hbv.n_vertices == NV
    _equals_oracle(mods, res, orc)

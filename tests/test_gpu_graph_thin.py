"""The thin kernels of the graph phase at their block and thread edges: the 31-mer absence filter (one position per thread), the
per-k-mer kernels k_rank_finish and k_assign (RANK_U k-mers per thread, loads staged by hop) and the look-back of the one-sweep radix
sort and of the scans across 64 and more tiles, csrc/step2_graph.hip and csrc/step2_prims.hip."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILTER_P = 1          # csrc/step2_graph.hip: positions per thread of k_filter32 (a block takes 256 FILTER_P)
RANK_U = 4            # csrc/step2_graph.hip: k-mers per thread of k_rank_finish and k_assign (a block takes 256 RANK_U)
BP, BU = 256 * FILTER_P, 256 * RANK_U


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    from w2rap_contigger_amd import formats as F, step2
    from oracle import oracle as O
    return F, step2, O


# ---------------------------------------------------------------------------------------------- the absence filter
@pytest.mark.parametrize("lo,hi", [(0, 16), (5, 11)])              # the whole filter; a slice of its words, as filter32_slice builds it
@pytest.mark.parametrize("npos", sorted({1, 63, 64, 65, 255, 256, 257, BP - 1, BP, BP + 1, 3 * BP + 17}))
def test_filter_words_equal_the_host_loop(mods, npos, lo, hi):
    """npos 31-mer positions of a random stream (nbases = npos + 30): one wavefront round, one block round, one block, several blocks --
    each a position short, exact and one over -- built by the graph phase's launch code and compared word by word with fmer_key on the host"""
    F, step2, O = mods
    L = step2.lib()
    L.w2rap_step2_selftest_filter32.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.w2rap_step2_selftest_filter32.restype = C.c_int
    with step2.Step2Context(0) as ctx:
        assert L.w2rap_step2_selftest_filter32(ctx.h, npos + 30, 1000 + npos, lo, hi) == 0


# ---------------------------------------------------------------------------------------------- look-back of the sort (and the scans)
@pytest.mark.parametrize("key_bits", [8, 60, -13])
@pytest.mark.parametrize("n", [64 * 2048 - 1, 64 * 2048, 64 * 2048 + 1, 65 * 2048 + 1, 129 * 2048 + 1,      # sort tiles: 64 | 64 | 65 | 66 | 130
                               64 * 4096 - 1, 64 * 4096 + 1, 65 * 4096 + 1])                                # scan tiles: 64 | 65 | 66
def test_look_back_across_many_tiles(mods, n, key_bits):
    """sorts of 64 - 130 tiles (a block's look-back walks that many predecessors) and scans across the 64-tile window of theirs, against
    the host (tests/test_gpu_prims.py has the sizes around one tile and the large ones)"""
    F, step2, O = mods
    L = step2.lib()
    L.w2rap_step2_selftest_prims.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
    L.w2rap_step2_selftest_prims.restype = C.c_int
    with step2.Step2Context(0) as ctx:
        assert L.w2rap_step2_selftest_prims(ctx.h, n, 17 + n, key_bits) == 0


# ---------------------------------------------------------------------------------------------- k_rank_finish, k_assign
def _canonical_kmers(g):
    rc = (3 - g[::-1]).astype(np.uint8)
    return {min(g[i:i + 60].tobytes(), rc[len(g) - 60 - i:len(g) - i].tobytes()) for i in range(len(g) - 59)}


def _exact_case(S):
    """reads whose solid 60-mers are exactly S: a random genome of S + 59 bases without a repeated 60-mer (either strand), every 100-base
    window of it (the whole genome where it is shorter) four times, all qualities 40 -- every 60-mer is counted at least four times = min_freq.
    S = 1: a read yields k-mers only if it is longer than 60 bases, and 61 bases hold ONE 60-mer only if they are a homopolymer: A^61."""
    rng = np.random.default_rng(9000 + S)
    if S == 1:
        g = np.zeros(61, np.uint8)
    else:
        while True:
            g = rng.integers(0, 4, S + 59, dtype=np.uint8)
            if len(_canonical_kmers(g)) == S:
                break
    L = min(100, len(g))
    reads = [g[s:s + L] for s in range(len(g) - L + 1) for _ in range(4)]
    codes = np.concatenate(reads)
    off = np.arange(len(reads) + 1, dtype=np.uint64) * L
    return codes, np.full(len(codes), 40, np.uint8), off


_CASES = {}


def _case(O, S):
    """the reads of _exact_case(S) with the oracle's Step 2 on them, computed once"""
    if S not in _CASES:
        codes, quals, off = _exact_case(S)
        _CASES[S] = (codes, quals, off, O.run(codes, quals, off))
    return _CASES[S]


def _step2_equals_oracle(mods, S, step3=False):
    F, step2, O = mods
    codes, quals, off, orc = _case(O, S)
    assert len(orc.k_hi) == S
    pk, bo, ln = F.pack_bases(codes, off)
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=quals, qual_off=off)
        st = ctx.count_kmers(7, 4)
        assert st["S"] == S
        ctx.build_graph(None)
        hi, lo, cnt, c, e, o = ctx.table(S)
        order = np.lexsort((lo, hi))
        assert np.array_equal(e[order], orc.k_edge) and np.array_equal(o[order], orc.k_off)          # k_assign's records, k-mer by k-mer
        ctx.path_reads()
        r3 = None
        if step3:
            from w2rap_contigger_amd import step3 as S3
            r3 = S3.repath_after_step2(ctx, 200)
        res = ctx.fetch()
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)
    return orc, r3


@pytest.mark.parametrize("S", [1, 3, 255, BU - 1, BU, BU + 1, 2 * BU + 5])
def test_per_kmer_kernels_at_block_and_thread_edges(mods, S):
    """S solid k-mers exactly: one thread, one round short of a wavefront's, a block short by one, exact, one over (a second block with one
    live thread), two blocks and five -- graph bytes, (edge, offset) of every k-mer and every path equal the oracle's"""
    _step2_equals_oracle(mods, S)


def test_per_kmer_kernels_with_wide_node_ids(mods, monkeypatch):
    monkeypatch.setenv("W2RAP_WIDE_IDS", "1")
    _step2_equals_oracle(mods, 2 * BU + 5)


def test_step3_ranks_as_arrays_behind_it(mods):
    """Step 3 behind that Step 2: its list ranking asks k_rank_finish for the ranks as arrays (nxt, rnk non-null) and skips the middle bases"""
    F, step2, O = mods
    from oracle import oracle3 as O3
    orc, r3 = _step2_equals_oracle(mods, 2 * BU + 5, step3=True)
    o3 = O3.run(O.to_hbv(orc), (orc.path_offset, orc.path_off, orc.path_edges), 200)
    assert F.hbv_to_bytes(r3.hbv) == F.hbv_to_bytes(O3.to_hbv(o3))
    assert np.array_equal(r3.path_offset, o3.path_offset) and np.array_equal(r3.path_off, o3.path_off) and np.array_equal(r3.path_edges, o3.path_edges)

"""Step 3 on the GPU at its own edges (csrc/step3_repath.hip, csrc/step3_back.h): every large K the reference runs, the K2 = 2 mod 4 it cannot
run, the graph shapes that matter at large K, FragDist's bounds, the exact launch sizes, --extend_paths on a graph with its true adjacency.
The inputs are tests/step3_cases.py; the oracle is pinned on them to recorded reference runs by tests/test_step3_oracle.py, so a difference
between the library and the oracle here is a library bug.  Everything is exact equality; the only normalisation is zero_padding=True against
the reference's files."""
import functools
import os

import numpy as np
import pytest

import step3_cases as SC
from test_gpu_step3 import _check_against_oracle, _check_extended, _dictionary_kernels
from w2rap_contigger_amd import formats as F
from oracle import oracle as O, oracle3 as O3

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(kind, *args):
    return getattr(SC, kind)(*args)


@functools.lru_cache(maxsize=None)
def _oracle(kind, args, K2, extend_paths=False):
    """the oracle's result in canonical order: computed once, shared and never changed"""
    h, p = _case(kind, *args)
    return O3.run(h, p, K2, extend_paths=extend_paths)


@functools.lru_cache(maxsize=None)
def _places_before(kind, args, K2):
    h, p = _case(kind, *args)
    return len(O3.run(h, p, K2, stop_after=1).place_off) - 1


def _hint(rh):
    hc, ho = O.edge_hint_from_hbv(rh)
    return hc, ho, F.pack_bases(hc, ho)


def _reversed_order(r):
    """an arbitrary edge order to replay: the oracle's canonical unipaths, reversed"""
    canon = [s for s in SC.objects_of(r.obj_codes, r.obj_off) if O.eform(s) != 1][::-1]
    hoff = np.zeros(len(canon) + 1, np.uint64); np.cumsum([len(s) for s in canon], out=hoff[1:])
    return (np.concatenate(canon) if canon else np.zeros(0, np.uint8)), hoff


def _equals_record(step3, res, rh, paths_bytes, frags):
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == paths_bytes
    assert F.hbv_to_bytes(res.hbv, zero_padding=True) == F.hbv_to_bytes(rh, zero_padding=True)
    assert step3.frags_text(res.frag_count) == frags


@pytest.mark.parametrize("K2", SC.REFERENCE_K2)
def test_gpu_step3_mix_at_every_large_k_the_reference_runs(K2, tmp_path):
    """mix(K2) at the 33 values of the reference's -K list: K2 mod 32 = 0 .. 28 (the `j == NW-1 && tail < 32` branches of kword_f / kword_r,
    step3_repath.hip:64-72, and of k3_kmer_keys, :561-564) and NW = 3 .. 20 (kequal's batches of four words with j clamped to NW-1, :84-95).
    The graph holds a palindromic K2-mer inside an edge and as an edge of its own (k3_kmer_keys' pal bit, :569), circles of 97 K2-mers and of
    ONE K2-mer (k3_minjump / k3_cycle_cut, :949-975: pointer doubling over a 1-cycle), a place of exactly K2 bases without a context (:571),
    end edges of K2-1 / K2 / K2+1 bases (k3_place_layout, :396: Repath.cc:113-122) and a K2-mer with four predecessors next to one with four
    successors (the context byte, :572-573).  With the recorded edge order: the reference's bytes and the oracle; in canonical order: the oracle."""
    from w2rap_contigger_amd import step3
    h, p = _case("mix", K2)
    rh, pb, fd = SC.recorded_step3(f"step3_mix_K{K2}", h, p, tmp_path, K2)
    hc, ho, packed = _hint(rh)
    res = step3.repath_in_memory(h, p, K2, edge_order_hint=packed)
    pr = step3.profile()
    assert "k3_cycle_cut" in pr and "k3_minjump" in pr and "k3_edge_from_hint" in pr
    _equals_record(step3, res, rh, pb, fd)
    _check_against_oracle(res, O3.run(h, p, K2, hc, ho))
    res = step3.repath_in_memory(h, p, K2)
    pr = step3.profile()
    assert all(k in pr for k in ("k3_cycle_cut", "k3_minjump", "k3_edge_tie_sort", "k3_dict_group"))
    _check_against_oracle(res, _oracle("mix", (K2,), K2))


@pytest.mark.parametrize("K2", SC.ORACLE_ONLY_K2)
def test_gpu_step3_mix_at_k2_of_2_mod_4(K2):
    """the library takes every even K2 in 62 .. 640 (step3_repath.hip:2131,2171); BigK has multiples of 4 only, so these rest on the oracle
    and on the plain-numpy invariants.  Only here (K2-1) mod 8 is 1 or 5: the scalar tail of k3_end_hash (:1161) and the `p + 8 <= K2 - 1`
    split of k3_end_words (:1178,1190); K2 = 62 has two words and a tail of 30, K2 = 638 twenty and 30."""
    from w2rap_contigger_amd import step3
    h, p = _case("mix", K2)
    res = step3.repath_in_memory(h, p, K2)
    _check_against_oracle(res, _oracle("mix", (K2,), K2))
    codes, off = res.hbv.edge_codes()
    SC.check_invariants(h, p, K2, SC.objects_of(codes, off), res.inv2, res.vleft, res.vright, (res.path_offset, res.path_off, res.path_edges), res.n_kmers_distinct)
    assert int(np.sum(res.inv2 == np.arange(len(res.inv2)))) == 1


@pytest.mark.parametrize("env,kernels", [({"W2RAP_TEST_SORT_BITS": "4", "W2RAP_TEST_DICT_AVG": "8"}, (True, False)),     # 16 tags, small partitions: every probe compares contents
                                         ({"W2RAP_TEST_DICT_CAP": "2"}, (True, True)),                                # a partition overflows: the sorted form takes over
                                         ({"W2RAP_STEP3_SORT_DICT": "1"}, (False, True)),
                                         ({"W2RAP_TEST_STEP3_FULL_SORTS": "1"}, (True, False)),
                                         ({"W2RAP_TEST_TIE_RUN": "1"}, (True, False)),
                                         ({"W2RAP_TEST_ENDS_COLLISION": "1"}, (True, False))])
@pytest.mark.parametrize("K2", [84, 188, 300])
def test_gpu_step3_dictionary_and_sort_corners_at_other_tails(K2, env, kernels, monkeypatch, tmp_path):
    """the corners the test hooks reach, so far run at K2 = 200 and 72 only (tails of 8): kequal (step3_repath.hip:84-95) behind k3_dict_group's
    tag matches (:713) and k3_group / k3_group_fix's runs (:595,614), the word-by-word sorts of places, unipaths (k3_head_word :1026,
    k3_edge_tie_sort :1034) and ends (k3_end_words :1165) -- at tails of 20, 28 and 12 bases and 3, 6 and 10 words, on mix(K2)"""
    from w2rap_contigger_amd import step3
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, p = _case("mix", K2)
    res = step3.repath_in_memory(h, p, K2)
    assert _dictionary_kernels(step3) == kernels
    _check_against_oracle(res, _oracle("mix", (K2,), K2))
    rh, pb, fd = SC.recorded_step3(f"step3_mix_K{K2}", h, p, tmp_path, K2)
    hc, ho, packed = _hint(rh)
    res = step3.repath_in_memory(h, p, K2, edge_order_hint=packed)
    _equals_record(step3, res, rh, pb, fd)
    _check_against_oracle(res, O3.run(h, p, K2, hc, ho))


def _bins(count):
    return {j: int(c) for j, c in enumerate(count) if c}


def test_gpu_step3_fragdist_bounds(tmp_path):
    """FragDist on the GPU rides in k3_place_keys (step3_repath.hip:218-231, summed by k3_frag_sum :285): len >= 10000 (:227), 0 <= d < 1000
    and d / 10 (:229), e1 == inv[e2], an empty mate (:225), a negative offset, a second mate of two edges; GapToyTools3.cc:625-635.  The
    literal bins are what the reference gave on these pairs."""
    from w2rap_contigger_amd import step3
    h, p = _case("fragdist")
    rh, pb, fd = SC.recorded_step3("step3_fragdist_K200", h, p, tmp_path, 200)
    hc, ho, packed = _hint(rh)
    res = step3.repath_in_memory(h, p, 200, edge_order_hint=packed)
    assert _bins(res.frag_count) == SC.FRAGDIST_BINS
    _equals_record(step3, res, rh, pb, fd)
    _check_against_oracle(res, O3.run(h, p, 200, hc, ho))
    _check_against_oracle(step3.repath_in_memory(h, p, 200), _oracle("fragdist", (), 200))


@pytest.mark.parametrize("n_filler_pairs", [62, 63, 254, 255])
def test_gpu_step3_fragdist_across_wavefronts_and_blocks(n_filler_pairs):
    """the same pairs behind 62, 63, 254 and 255 pairs of reads without a path: they straddle the ends of the wavefronts (the __shfl_down that
    hands the odd mate's edge down, step3_repath.hip:224) and of the 256-thread blocks of k3_place_keys, so LDS bins of two blocks (:219)
    and several of the 32 stripes (:283) must add up in k3_frag_sum (:285)"""
    from w2rap_contigger_amd import step3
    h, p = _case("fragdist", n_filler_pairs)
    res = step3.repath_in_memory(h, p, 200)
    assert _bins(res.frag_count) == SC.FRAGDIST_BINS
    _check_against_oracle(res, _oracle("fragdist", (n_filler_pairs,), 200))


@pytest.mark.parametrize("U,N2,K2", SC.COUNTS)
def test_gpu_step3_exact_launch_sizes(U, N2, K2, tmp_path):
    """U places, N2 K2-mer occurrences, D = N2 distinct K2-mers, E = U unipaths, one below / at / one above what a block takes: 1024
    occurrences for k3_kmer_keys with the block's last place looked up through blk[] (step3_repath.hip:526-531), 4096 nodes of N = 2 D for
    k3_head_cands (:976), 4096 pairs for k3_dict_part (:657), 256 for everything else (grid_for, :110).  At K2 = 640 a block's places do not
    fit KW_WORDS and StreamWin::at reads from global memory (:502).  Canonical order, an arbitrary order replayed, and the same with
    W2RAP_STEP3_UNIQUE_KMERS (k3_lone_places, :481: the K2-mers strictly inside skip the hashing)."""
    from w2rap_contigger_amd import step3
    h, p = _case("counts", U, N2, K2)
    r = _oracle("counts", (U, N2, K2), K2)
    res = step3.repath_in_memory(h, p, K2)
    assert (res.n_unique_places, res.n_kmer_instances, res.n_kmers_distinct, res.n_unipaths) == (U, N2, N2, U)
    _check_against_oracle(res, r)
    _check_against_oracle(step3.repath_in_memory(h, p, K2, unique_kmers=True), r)
    assert "k3_lone_places" in step3.profile()
    hc, hoff = _reversed_order(r)
    _check_against_oracle(step3.repath_in_memory(h, p, K2, edge_order_hint=F.pack_bases(hc, hoff)), O3.run(h, p, K2, hc, hoff))
    if (U, N2, K2) in SC.COUNTS_RECORDED:
        rh, pb, fd = SC.recorded_step3(f"step3_counts_{U}_{N2}_K{K2}", h, p, tmp_path, K2)
        _equals_record(step3, step3.repath_in_memory(h, p, K2, edge_order_hint=_hint(rh)[2]), rh, pb, fd)


@pytest.mark.parametrize("K2", SC.JOINED_K2)
def test_gpu_step3_extend_paths_on_a_joined_graph(K2, tmp_path):
    """--extend_paths where places really are extended (k3_vertex_deg, k3_extend_len, k3_extend_fill, step3_repath.hip:354-395; Repath.cc:72-96):
    along a chain, stopped by a fork, and the Member(p, e) break on a one-edge circle (Repath.cc:84,88).  The recorded reference run
    replayed; n_unique_places stays the number before the extension (Repath.cc:71); without the flag the plain result."""
    from w2rap_contigger_amd import step3
    h, p = _case("joined", K2)
    before = _places_before("joined", (K2,), K2)
    rh, pb, fd = SC.recorded_step3(f"step3_joined_K{K2}_extend", h, p, tmp_path, K2, extend_paths=True)
    hc, ho, packed = _hint(rh)
    res = step3.repath_in_memory(h, p, K2, edge_order_hint=packed, extend_paths=True)
    _equals_record(step3, res, rh, pb, fd)
    assert res.n_unique_places == before == 11
    _check_extended(res, O3.run(h, p, K2, hc, ho, extend_paths=True), before)
    r = _oracle("joined", (K2,), K2, True)
    assert len(r.place_off) - 1 == 17
    _check_extended(step3.repath_in_memory(h, p, K2, extend_paths=True), r, before)
    _check_extended(step3.repath_in_memory(h, p, K2, extend_paths=True, unique_kmers=True), r, before)
    assert "k3_lone_places" in step3.profile()
    plain = _oracle("joined", (K2,), K2)
    _check_against_oracle(step3.repath_in_memory(h, p, K2), plain)
    _check_against_oracle(step3.repath_in_memory(h, p, K2, unique_kmers=True), plain)
    assert "k3_lone_places" in step3.profile()


def test_standalone_step3_tool_on_a_hand_made_graph(tmp_path):
    """w2rap-step3 (csrc/w2rap_step3_main.cpp) through files on mix(200) -- so far it ran on the fixtures only: the recorded reference run's
    files with its edge order replayed, and the in-memory call's bytes in canonical order"""
    import subprocess
    from conftest import ROOT
    from w2rap_contigger_amd import step3
    tool = os.path.join(ROOT, "w2rap_contigger_amd", "w2rap-step3")
    h, p = _case("mix", 200)
    ref = tmp_path / "ref"; ref.mkdir()
    rh, pb, fd = SC.recorded_step3("step3_mix_K200", h, p, ref, 200)
    d = tmp_path / "out"; d.mkdir()
    F.write_hbv(d / "x.small_K.hbv", h); F.write_paths(d / "x.small_K.paths", *p)
    out = subprocess.run([tool, "-o", str(d), "-p", "x", "-K", "200", "--edge_order_from", str(ref / "t.large_K.hbv")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert f"{_places_before('mix', (200,), 200)} unique places" in out.stdout
    assert open(d / "x.large_K.paths", "rb").read() == pb and open(d / "x.first.frags.dist").read() == fd
    assert F.hbv_to_bytes(F.read_hbv(d / "x.large_K.hbv"), zero_padding=True) == F.hbv_to_bytes(rh, zero_padding=True)
    out = subprocess.run([tool, "-o", str(d), "-p", "x", "-K", "200"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    res = step3.repath_in_memory(h, p, 200)
    assert open(d / "x.large_K.hbv", "rb").read() == F.hbv_to_bytes(res.hbv)
    assert open(d / "x.large_K.paths", "rb").read() == F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges)

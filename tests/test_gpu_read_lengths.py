"""Steps 2 and 3 at every read-length route, against the oracle.

Step 2 picks its kernels and sizes its scratch from the LONGEST read of the set: K1 cuts reads in passes of 128 k-mer positions
(npass >= 2 above 187 bases) and leaves the lane-per-read kernel for the wavefront one when its slots outgrow the lane's staging
(from 316 bases); pathing sends many-part reads to the listed kernel instead of the wavefront one (from 250), leaves k_path_dyn
for k_path when a lane's LDS slot passes 64 KB (from 737) and stops staging reads in LDS (from 1,533).  Each case here sits on one
side of such a threshold (or, with reads of up to 65,535 bases among short ones, takes the long-read pathing pass whose lanes are
bounded by the long reads), reads its route from the W2RAP_TRACE lines and is checked against the oracle in full: histogram, graph
bytes, paths and the pathed / multipathed counts.  The reads come from a two-haplotype genome with repeats, a SNP every ~300
bases and a stretch of one every ~70, and tandem arrays of short periods, so that many reads cross more unipaths than the first
pathing pass keeps."""
import re

import numpy as np
import pytest

from w2rap_contigger_amd import formats as F, synth
from oracle import oracle as O, oracle3 as O3

pytestmark = pytest.mark.gpu

GENOME = synth.diploid_genome(70_000, 2024, snp_every=300, dense=(8_000, 24_000, 70),
                              tandem=((28_000, 6, 1_200), (38_000, 9, 1_200), (55_000, 13, 1_500), (60_000, 21, 1_500)))

# case -> (read_len of the pairs, pairs, extra single-read lengths), expected (K1 kernel, npass, main pathing pass, many-part pass)
_RAGGED = [L for L in range(401) for _ in range(11)]
CASES = {
    "u188": ((188, 4000, []), ("lane", 2, "dyn", "wave")),
    "u249": ((249, 4000, []), ("lane", 2, "dyn", "wave")),
    "u250": ((250, 4000, []), ("lane", 2, "dyn", "listed")),
    "u251": ((251, 4000, []), ("lane", 2, "dyn", "listed")),
    "u300": ((300, 4000, []), ("lane", 2, "dyn", "listed")),
    "u315": ((315, 4000, []), ("lane", 2, "dyn", "listed")),
    "u316": ((316, 4000, []), ("wave", 3, "dyn", "listed")),
    "mix736": ((150, 8000, [736] * 6 + [500, 600]), ("wave", 6, "dyn", "listed")),
    "mix737": ((150, 8000, [737] * 6 + [736, 600]), ("wave", 6, "staged", "listed")),
    "mix1532": ((150, 8000, [1532] * 6 + [900, 1200]), ("wave", 12, "staged", "listed")),
    "mix1533": ((150, 8000, [1533] * 6 + [1532, 1000]), ("wave", 12, "global", "listed")),
    "mix65535": ((150, 12000, list(np.random.default_rng(3).integers(2_000, 20_001, 24)) + [65_535, 65_535]), ("wave", 512, "split", "listed")),
    "ragged400": ((150, 0, _RAGGED), ("wave", 3, "dyn", "listed")),
}
MIXED = ["mix736", "mix737", "mix1532", "mix1533", "mix65535"]

_READS = {}
_STEP2 = {}


def case_reads(name):
    if name not in _READS:
        (L, n_pairs, extra), _ = CASES[name]
        codes, quals, off = synth.read_length_workload(GENOME, n_pairs, 1000 + L + len(extra), read_len=L, insert=max(400, L + 100),
                                                       extra_lengths=extra)
        pk, bo, ln = F.pack_bases(codes, off)
        _READS[name] = dict(codes=codes, quals=quals, off=off, pk=pk, bo=bo, ln=ln)
    return _READS[name]


@pytest.fixture(scope="module")
def oracle_started():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    from conftest import oracle_prefetch
    for name in CASES:                               # the oracle runs start at once on host threads; a test waits for its own
        r = case_reads(name)
        oracle_prefetch(r["codes"], r["quals"], r["off"])
    return True


def routes(text):
    """-> (K1 kernels, K1 npass values, main pathing passes, many-part passes, reads of the many-part passes) named in W2RAP_TRACE output"""
    k1 = re.findall(r"K1 route: (\w+), npass (\d+)", text)
    pth = re.findall(r"pathing route: longest \d+, main (\w+), many-part (\w+)", text)
    many = re.findall(r"pathing many-part pass: (\d+) reads, (\w+)", text)
    long = re.findall(r"pathing long-read pass: (\d+) reads of more than (\d+) bases", text)
    return ({k for k, _ in k1}, {int(p) for _, p in k1}, {m for m, _ in pth}, {w for _, w in pth}, sum(int(n) for n, _ in many),
            [(int(n), int(L)) for n, L in long])


def assert_equals_oracle(res, orc):
    assert orc.n_instances > 0 and np.array_equal(res.hist, orc.hist)
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)
    assert (res.n_reads_pathed, res.n_reads_multipathed) == (orc.pathed, orc.multipathed)


def step2_result(name, monkeypatch=None, capfd=None):
    """the one-GPU dictionary result of a case (once per session); with capfd: its trace as well"""
    from w2rap_contigger_amd import step2
    if name not in _STEP2:
        r = case_reads(name)
        if monkeypatch is not None:
            monkeypatch.setenv("W2RAP_TRACE", "1")
        if capfd is not None:
            capfd.readouterr()
        res = step2.build_read_qgraph(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"])
        trace = capfd.readouterr().err if capfd is not None else None
        if monkeypatch is not None:
            monkeypatch.delenv("W2RAP_TRACE")
        _STEP2[name] = (res, trace)
    return _STEP2[name]


@pytest.mark.parametrize("name", list(CASES))
def test_step2_route_equals_the_oracle(oracle_started, name, monkeypatch, capfd):
    _STEP2.pop(name, None)
    res, trace = step2_result(name, monkeypatch, capfd)
    r = case_reads(name)
    n = len(r["ln"])
    assert n >= 4096, "fewer reads than k_path_dyn needs"
    assert int(r["ln"].max()) == max([CASES[name][0][0] if CASES[name][0][1] else 0] + list(CASES[name][0][2]))
    k1, npass, main, many, n_many, long = routes(trace)
    want_k1, want_npass, want_main, want_many = CASES[name][1]
    assert k1 == {want_k1} and npass == {want_npass}, trace
    assert main == {want_main} and many == {want_many}, trace
    if want_main == "split":                      # the long reads in a pass of their own, every other read in the listed one
        assert len(long) == 1 and long[0][0] == int((r["ln"] > long[0][1]).sum()) > 0, trace
    else:
        assert not long and n_many >= 20, f"only {n_many} reads with more parts than the first pathing pass keeps\n{trace}"
    assert_equals_oracle(res, O.run(r["codes"], r["quals"], r["off"]))


@pytest.mark.parametrize("variant", ["index", "two_ranks", "three_passes"])
@pytest.mark.parametrize("name", MIXED)
def test_mixed_lengths_other_routes_equal_the_dictionary(oracle_started, name, variant, monkeypatch):
    """the pathing index (W2RAP_PATH_INDEX), two ranks on one GPU and three hash-range counting passes: byte-equal to the one-GPU result"""
    from w2rap_contigger_amd import step2
    base, _ = step2_result(name)
    r = case_reads(name)
    kw = {}
    if variant == "index":
        monkeypatch.setenv("W2RAP_PATH_INDEX", "1")
    elif variant == "two_ranks":
        kw["devices"] = [0, 0]
    else:
        kw["n_passes"] = 3
    res = step2.build_read_qgraph(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"], **kw)
    assert np.array_equal(res.hist, base.hist)
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(base.hbv)
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(base.path_offset, base.path_off, base.path_edges)
    assert (res.n_reads_pathed, res.n_reads_multipathed) == (base.n_reads_pathed, base.n_reads_multipathed)


def _check_against_oracle3(res, r):
    assert np.array_equal(res.inv, r.inv) and np.array_equal(res.inv2, r.inv2)
    assert np.array_equal(res.frag_count.astype(np.float64), r.frag)
    assert (res.n_unique_places, res.n_kmer_instances, res.n_kmers_distinct, res.n_unipaths) == (len(r.place_off) - 1, r.n_instances, r.n_distinct, r.n_edges)
    assert res.n_place_bases == len(r.all_codes)
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O3.to_hbv(r))
    assert np.array_equal(res.vleft, r.left) and np.array_equal(res.vright, r.right) and np.array_equal(res.to_v, r.to_v)
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(r.path_offset, r.path_off, r.path_edges)


@pytest.mark.parametrize("K2", [100, 200, 260])
@pytest.mark.parametrize("name", ["u251", "u316"] + MIXED)
def test_step3_behind_long_reads_equals_the_oracle(oracle_started, name, K2):
    """Step 3 on the paths the long reads made: plain, with the unique-K-mer shortcut, and (K2 = 200) with --extend_paths"""
    from w2rap_contigger_amd import step3
    s2, _ = step2_result(name)
    paths = (s2.path_offset, s2.path_off, s2.path_edges)
    r = O3.run(s2.hbv, paths, K2)
    assert r.n_edges > 0
    _check_against_oracle3(step3.repath_in_memory(s2.hbv, paths, K2), r)
    _check_against_oracle3(step3.repath_in_memory(s2.hbv, paths, K2, unique_kmers=True), r)
    if K2 == 200:
        res = step3.repath_in_memory(s2.hbv, paths, K2, extend_paths=True)
        e = O3.run(s2.hbv, paths, K2, extend_paths=True)
        assert np.array_equal(res.inv, e.inv) and np.array_equal(res.inv2, e.inv2)
        assert (res.n_unique_places, res.n_kmers_distinct, res.n_unipaths) == (len(r.place_off) - 1, e.n_distinct, e.n_edges)
        assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O3.to_hbv(e))
        assert np.array_equal(res.vleft, e.left) and np.array_equal(res.vright, e.right) and np.array_equal(res.to_v, e.to_v)
        assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == F.paths_to_bytes(e.path_offset, e.path_off, e.path_edges)


def _with_long_reads(base, seed=11, genome_len=3_000_000):
    """the 600 k PE150 reads of conftest.PREFETCH_SYNTH plus 16 reads of 65,535 bases and 64 of 2 k to 20 k bases from the same genome"""
    import torch
    g = torch.randint(0, 4, (genome_len,), dtype=torch.uint8, device="cuda",
                      generator=torch.Generator(device="cuda").manual_seed(seed)).cpu().numpy()      # (synth.generate_reads_device's genome)
    lengths = [65_535] * 16 + list(np.random.default_rng(seed).integers(2_000, 20_001, 64))
    extra = synth.sample_reads_of_lengths([g], lengths, seed + 5)
    codes = np.concatenate([base["codes"]] + [c for c, _ in extra])
    quals = np.concatenate([base["quals"]] + [q for _, q in extra])
    off = np.concatenate([base["off"], base["off"][-1] + np.cumsum([len(c) for c, _ in extra]).astype(np.uint64)])
    return codes, quals, off


def test_few_long_reads_among_600k_short_ones_stay_within_memory(oracle_started):
    """One long read among many short ones must not size every read's (or every pathing lane's) scratch by the longest read:
    16 reads of 65,535 bases and 64 of 2 k to 20 k among 600 k PE150 reads raise the device peak by at most 2 GB, oracle parity"""
    from conftest import PREFETCH_SYNTH, synth_reads, oracle_prefetch
    from w2rap_contigger_amd import step2
    spec = [s for s in PREFETCH_SYNTH if s[0] == 600_000][0]
    base = synth_reads(*spec)
    codes, quals, off = _with_long_reads(base, spec[2], spec[1])
    oracle_prefetch(codes, quals, off)
    peaks = []
    for c, q, o in ((base["codes"], base["quals"], base["off"]), (codes, quals, off)):
        pk, bo, ln = F.pack_bases(c, o)
        with step2.Step2Context(0) as ctx:
            ctx.set_reads_host(pk, bo, ln, quals=q, qual_off=o)
            ctx.device_peak_bytes(reset=True)
            ctx.count_kmers(7, 4)
            ctx.build_graph(None)
            ctx.path_reads()
            peaks.append(ctx.device_peak_bytes() - int(bo[-1]) - len(q))         # (less the reads' own bases and qualities)
            res = ctx.fetch()
        assert_equals_oracle(res, O.run(c, q, o))
    assert peaks[1] - peaks[0] <= 2 << 30, f"device peak {peaks[0] / 2**30:.2f} GB -> {peaks[1] / 2**30:.2f} GB"


@pytest.mark.parametrize("tag", ["ref", "ref8"])
def test_long_mixed_replays_the_reference(oracle_started, tag):
    """tests/golden/long_mixed (PE250 with reads of 300 to 20,000 bases), the reference's edge order replayed: its own .hbv / .paths /
    small_K.freqs, and behind them Step 3 at K2 = 200 with its large-K edge order: its large-K paths and graph (and frags.dist)"""
    import os
    from conftest import GOLDEN, golden_bytes, load_fixture
    from w2rap_contigger_amd import step2, step3
    name = "long_mixed"
    fx = load_fixture(name)
    hc, ho = O.edge_hint_from_hbv(F.read_hbv(os.path.join(GOLDEN, f"{name}.{tag}.hbv")))
    res = step2.build_read_qgraph(fx["packed"], fx["byte_off"], fx["read_len"], pq=fx["pq"], pq_off=fx["pq_off"], edge_order_hint=F.pack_bases(hc, ho))
    assert F.hbv_to_bytes(res.hbv) == golden_bytes(name, tag, "hbv")
    assert F.paths_to_bytes(res.path_offset, res.path_off, res.path_edges) == golden_bytes(name, tag, "paths")
    assert F.freqs_text(res.hist).encode() == golden_bytes(name, "ref", "freqs")
    rh = F.read_hbv(os.path.join(GOLDEN, f"{name}.{tag}.large_K.hbv"))
    h3c, h3o = O.edge_hint_from_hbv(rh)
    r3 = step3.repath_in_memory(res.hbv, (res.path_offset, res.path_off, res.path_edges), 200, edge_order_hint=F.pack_bases(h3c, h3o))
    assert F.paths_to_bytes(r3.path_offset, r3.path_off, r3.path_edges) == golden_bytes(name, tag, "large_K.paths")
    assert F.hbv_to_bytes(r3.hbv, zero_padding=True) == F.hbv_to_bytes(rh, zero_padding=True)
    if tag == "ref":
        assert step3.frags_text(r3.frag_count) == open(os.path.join(GOLDEN, f"{name}.ref.frags.dist")).read()


def test_wavefront_k1_in_batches_equals_the_oracle(oracle_started, monkeypatch, capfd):
    """K1's wavefront kernel with its per-read descriptor slots in the batched partition (>= 2^20 reads: several batches, each with its
    own pass offsets from its first read on, double-buffered while the previous batch is scattered): the bench-like 1.1 M reads"""
    from conftest import synth_reads
    from w2rap_contigger_amd import step2
    r = synth_reads(1_100_000, 5_500_000, 78)
    monkeypatch.setenv("W2RAP_K1", "wave")
    monkeypatch.setenv("W2RAP_TRACE", "1")
    capfd.readouterr()
    res = step2.build_read_qgraph(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"])
    trace = capfd.readouterr().err
    k1 = re.findall(r"K1 route: (\w+), npass \d+, spp \d+, (\d+) reads", trace)
    assert len(k1) >= 3 and {k for k, _ in k1} == {"wave"} and max(int(n) for _, n in k1) < r["n"], trace     # (one line per batch)
    assert_equals_oracle(res, O.run(r["codes"], r["quals"], r["off"]))

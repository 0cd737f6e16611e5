"""The partition's slab route: the lane cutter stores every super-k-mer record at (bucket * C + rank) itself, ranks >= C and a read's records
beyond its staged slots go through the overflow list, and the counting kernels read a bucket as two (start, count) segments.  Every case runs
Step 2 against the CPU oracle -- histogram, solid k-mers with counts and pruned contexts, (edge, offset) per k-mer, graph bytes, every path --
with W2RAP_K1_SLABS unset and =0 (the scatter pass).  All integer work: equality, no tolerance.  The route each run took is read from the
W2RAP_TRACE line of the cutter's launch."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KPB = 4500                                             # k-mers per bucket (the library's default; W2RAP_KPB is not set here)
SLOTS = 8                                              # descriptor slots the cutter stages per PE150 read


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    from w2rap_contigger_amd import formats as F, step2
    from oracle import oracle as O
    assert step2.lib().w2rap_step2_device_count() >= 1
    return F, step2, O


def _rc(r):
    return (3 - r[::-1]).astype(np.uint8)


def _background(rng, glen=6000, n=2400, rlen=150):
    """reads of both strands over a random genome (~60x)"""
    g = rng.integers(0, 4, glen, dtype=np.uint8)
    out = []
    for s in rng.integers(0, glen - rlen, n):
        r = g[s:s + rlen]
        out.append(_rc(r) if rng.integers(0, 2) else r.copy())
    return g, out


def _pack(reads, quals=None, rng=None):
    reads = list(reads)
    quals = [np.full(len(r), 35, np.uint8) for r in reads] if quals is None else list(quals)
    if len(reads) % 2:
        reads.append(reads[0]); quals.append(quals[0])
    if rng is not None:                                  # shuffled in pairs
        order = rng.permutation(len(reads) // 2)
        reads = [reads[2 * i + j] for i in order for j in (0, 1)]; quals = [quals[2 * i + j] for i in order for j in (0, 1)]
    lens = np.array([len(r) for r in reads], np.uint64)
    off = np.zeros(len(reads) + 1, np.uint64); np.cumsum(lens, out=off[1:])
    return np.concatenate(reads).astype(np.uint8), np.concatenate(quals).astype(np.uint8), off


def bucket_runs(R, nb):
    """CPU model of the cut: for reads R[n, L] (all bases good) the number of runs of equal minimizer bucket among each read's k-mers --
    a lower bound of its records (a run longer than 63 k-mers is cut again).  15-mers LSB first, key = canonical * 0x9E3779B1, the window
    of a 60-mer is 46 keys, bucket = high word of (mix(min key) * nb)."""
    n, L = R.shape
    f = np.zeros(n, np.uint64); rc = np.zeros(n, np.uint64)
    keys = np.empty((n, L - 14), np.uint64)
    for s in range(L):
        b = R[:, s].astype(np.uint64)
        f = (f >> np.uint64(2)) | (b << np.uint64(28))
        rc = ((rc << np.uint64(2)) & np.uint64(0x3FFFFFFF)) | (b ^ np.uint64(3))
        if s >= 14:
            keys[:, s - 14] = (np.minimum(f, rc) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    mk = np.lib.stride_tricks.sliding_window_view(keys, 46, axis=1).min(axis=2)
    h = ((mk ^ (mk >> np.uint64(15))) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    bk = (h * np.uint64(nb)) >> np.uint64(32)
    return 1 + (bk[:, 1:] != bk[:, :-1]).sum(axis=1)


def _case_uniform():
    rng = np.random.default_rng(501)
    return _pack(_background(rng)[1])


def _case_heavy():
    """five reads given 511, 512, 513, 700 and 20 000 times: ranks around C = 512, deferred buckets read from slab plus overflow segment
    (a bucket holds one record of the read per copy, so its ranks stay below 65 536: _case_rank16 goes beyond)"""
    rng = np.random.default_rng(502)
    _, reads = _background(rng)
    for m in (511, 512, 513, 700, 20000):
        r = rng.integers(0, 4, 150, dtype=np.uint8)
        reads += [r] * m
    return _pack(reads, rng=rng)


def _case_rank16():
    """70 000 copies of a 122-base tandem repeat of period 30 (one minimizer: one 63-k-mer record per read): ranks beyond 65 535 in one
    bucket, which the scatter pass's 16-bit descriptors send through the list"""
    rng = np.random.default_rng(503)
    _, reads = _background(rng, n=600)
    t = np.tile(rng.integers(0, 4, 30, dtype=np.uint8), 5)[:122]
    reads += [t] * 70000
    return _pack(reads, rng=rng)


HEAVY_COPIES = 20000


def _case_heavy_behind_the_sample():
    """9600 reads over a genome of 192 000 bases (7.5x: the first 1/32 of the reads puts ~7 records into a bucket, few beyond C / 32 = 16),
    and behind them one read 20 000 times.  Not shuffled: the guard's sample sees the background only."""
    rng = np.random.default_rng(507)
    _, reads = _background(rng, glen=192000, n=9600)
    reads += [rng.integers(0, 4, 150, dtype=np.uint8)] * HEAVY_COPIES
    return _pack(reads)


def _case_slots():
    """reads that cut into more than eight records: of 6000 random reads those with the most minimizer runs, six times each"""
    rng = np.random.default_rng(504)
    _, reads = _background(rng)
    cand = rng.integers(0, 4, (6000, 150), dtype=np.uint8)
    runs = bucket_runs(cand, 1 << 24)
    pick = np.argsort(runs)[-60:]
    for i in pick:
        reads += [cand[i].copy()] * 6
    return _pack(reads, rng=rng)


def _case_read_edges():
    """reads of 61 and 62 good bases; reads with no k-mer (50 bases, 60 bases, 150 bases of which 60 are good) alone among full reads of a
    wavefront; wavefronts 10 and 11 (reads 640 .. 767) hold no k-mer at all.  Not shuffled: the places matter."""
    rng = np.random.default_rng(505)
    _, reads = _background(rng)
    quals = [np.full(150, 35, np.uint8) for _ in reads]

    def put(i, r, q=None):
        reads[i] = r; quals[i] = np.full(len(r), 35, np.uint8) if q is None else q

    for i in range(640, 768):
        put(i, rng.integers(0, 4, 50 if i % 3 else 60, dtype=np.uint8))
    for i in (3, 100, 101, 131, 190, 255, 256, 1000, 2399):
        put(i, rng.integers(0, 4, 50, dtype=np.uint8))
    for i in (5, 300, 1023):
        put(i, rng.integers(0, 4, 60, dtype=np.uint8))
    for i in (7, 320, 1024):
        put(i, rng.integers(0, 4, 150, dtype=np.uint8), np.concatenate([np.full(60, 35, np.uint8), np.full(90, 2, np.uint8)]))
    for n in (61, 62):
        r = rng.integers(0, 4, n, dtype=np.uint8)
        for j in range(40):
            put(int(rng.integers(800, 2300)), r)
        r = rng.integers(0, 4, 150, dtype=np.uint8)
        q = np.concatenate([np.full(n, 35, np.uint8), np.full(150 - n, 2, np.uint8)])
        for j in range(40):
            put(int(rng.integers(800, 2300)), r, q)
    return _pack(reads, quals)


def _case_n(n):
    """the first n reads of a 40x sample of a 300-base genome: one lane, wave edges, block edges"""
    rng = np.random.default_rng(600 + n)
    g = rng.integers(0, 4, 300, dtype=np.uint8)
    reads = []
    for s in rng.integers(0, 150, n):
        r = g[s:s + 150]
        reads.append(_rc(r) if rng.integers(0, 2) else r.copy())
    if n == 2:
        reads = [np.tile(g[:30], 5), np.tile(g[:30], 5)]   # (two reads reach min_freq only by a repeat: period 30, every k-mer six times)
    return _pack(reads)


def _case_long():
    rng = np.random.default_rng(506)
    g, reads = _background(rng)
    reads += [g[1000:1400].copy()] * 2                     # 400 good bases: beyond the lane kernel's 315
    return _pack(reads)


LAUNCH_N = (2, 62, 64, 66, 254, 256, 258)
_CASES = {"uniform": _case_uniform, "heavy": _case_heavy, "rank16": _case_rank16, "slots": _case_slots, "read_edges": _case_read_edges,
          "long": _case_long, "heavy_behind_the_sample": _case_heavy_behind_the_sample, **{f"n{n}": (lambda n=n: _case_n(n)) for n in LAUNCH_N}}
_cache = {}


def _case(mods, name):
    """reads, packed reads and the oracle's result: computed once per module, never changed"""
    if name not in _cache:
        F, step2, O = mods
        codes, quals, off = _CASES[name]()
        _cache[name] = dict(codes=codes, quals=quals, off=off, packed=F.pack_bases(codes, off), orc=O.run(codes, quals, off))
    return _cache[name]


def _routes(trace):
    """-> [(kernel, 'slabs' | 'scatter', C)] of the cutter's launches named in a W2RAP_TRACE text"""
    m = re.findall(r"K1 route: (\w+), npass \d+, spp \d+, \d+ reads, longest \d+, records (to slabs of|by scatter pass) (\d+)", trace)
    return [(k, "slabs" if how.startswith("to") else "scatter", int(c)) for k, how, c in m]


def _check_stages(mods, c, capfd, n_passes=None):
    """Step 2 stage by stage against the oracle; -> the cutter's routes"""
    F, step2, O = mods
    orc = c["orc"]
    pk, bo, ln = c["packed"]
    capfd.readouterr()
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=c["quals"], qual_off=c["off"])
        st = ctx.count_kmers(7, 4, n_passes=n_passes)
        assert (st["M"], st["D"], st["S"]) == (orc.n_instances, orc.n_distinct, len(orc.k_hi))
        assert np.array_equal(st["hist"], orc.hist)
        hi, lo, cnt, cx, e, o = ctx.table(st["S"])
        order = np.lexsort((lo, hi))
        assert np.array_equal(hi[order], orc.k_hi) and np.array_equal(lo[order], orc.k_lo)
        assert np.array_equal(cnt[order], orc.k_count) and np.array_equal(cx[order], orc.k_ctx)
        ctx.build_graph(None)
        hi, lo, cnt, cx, e, o = ctx.table(st["S"])
        assert np.array_equal(e[order], orc.k_edge) and np.array_equal(o[order], orc.k_off)
        ctx.path_reads()
        res = ctx.fetch()
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)
    assert (res.n_reads_pathed, res.n_reads_multipathed) == (orc.pathed, orc.multipathed)
    return _routes(capfd.readouterr().err)


def _run(mods, monkeypatch, capfd, name, slabs, env=None, cap=512):
    """one case on the slab route (slabs is None) or with W2RAP_K1_SLABS=0; asserts the route it took"""
    monkeypatch.setenv("W2RAP_TRACE", "1")
    if slabs is not None:
        monkeypatch.setenv("W2RAP_K1_SLABS", slabs)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    routes = _check_stages(mods, _case(mods, name), capfd)
    # (one line per launch: a second one where the first overflow list was too small and the reads were cut again)
    assert 1 <= len(routes) <= 2 and set(routes) == {("lane", "slabs", cap) if slabs is None else ("lane", "scatter", 0)}, routes
    return routes


SWITCH = pytest.mark.parametrize("slabs", [None, "0"])


@SWITCH
@pytest.mark.parametrize("cap", [None, "1", "2", "3", "64"])
def test_uniform_reads(mods, monkeypatch, capfd, slabs, cap):
    """default C, and C = 1, 2, 3 (nearly every bucket overflows; the first list is too small and the cut is repeated) and 64 (some do)"""
    env = {"W2RAP_TEST_SLAB_CAP": cap} if cap else {}
    routes = _run(mods, monkeypatch, capfd, "uniform", slabs, env, int(cap) if cap else 512)
    if slabs is None and cap != "64":                  # (~130 records a bucket: the list of C = 1 .. 3 must have been too small, the default's not)
        assert len(routes) == (1 if cap is None else 2), routes


@SWITCH
@pytest.mark.parametrize("env", [{"W2RAP_FP_DEDUP": "0"}, {"W2RAP_K3": "0"}, {"W2RAP_FUSED_PRUNE": "1"}])
def test_cap_one_with_the_other_counting_forms(mods, monkeypatch, capfd, slabs, env):
    """C = 1 with k_count_fp without record dedup, with the list kernel on slab input (W2RAP_K3=0), with the fused prune"""
    _run(mods, monkeypatch, capfd, "uniform", slabs, {"W2RAP_TEST_SLAB_CAP": "1", **env}, 1)


@SWITCH
def test_heavy_buckets(mods, monkeypatch, capfd, slabs):
    _run(mods, monkeypatch, capfd, "heavy", slabs)


@SWITCH
def test_ranks_beyond_16_bits(mods, monkeypatch, capfd, slabs):
    _run(mods, monkeypatch, capfd, "rank16", slabs)


@SWITCH
def test_more_records_than_slots(mods, monkeypatch, capfd, slabs):
    c = _case(mods, "slots")
    n = len(c["off"]) - 1
    R = c["codes"].reshape(n, 150)
    nb = c["orc"].n_instances // KPB + 1
    runs = bucket_runs(R, nb)
    assert (runs > SLOTS).sum() >= 100, (runs > SLOTS).sum()       # (the input does hold reads whose records pass their slots)
    _run(mods, monkeypatch, capfd, "slots", slabs)
    _run(mods, monkeypatch, capfd, "slots", slabs, {"W2RAP_TEST_SLAB_CAP": "3"}, 3)


@SWITCH
@pytest.mark.parametrize("n", LAUNCH_N)
def test_edges_of_the_launch(mods, monkeypatch, capfd, slabs, n):
    _run(mods, monkeypatch, capfd, f"n{n}", slabs)


@SWITCH
def test_edges_of_a_read(mods, monkeypatch, capfd, slabs):
    _run(mods, monkeypatch, capfd, "read_edges", slabs)
    _run(mods, monkeypatch, capfd, "read_edges", slabs, {"W2RAP_TEST_SLAB_CAP": "2"}, 2)


@pytest.mark.parametrize("name", ["heavy", "rank16"])
def test_guard_sends_heavy_buckets_to_the_scatter_pass(mods, monkeypatch, capfd, name):
    """inputs of 2^20 reads and more are asked first (the first 1/32 of the reads is cut, the records beyond C / 32 per bucket times 32
    estimate those beyond the slabs; more than reads / 10: the scatter pass).  The test hook asks these small inputs too: the 20 000 and the
    70 000 copies pass the limit many times over.  Two K1 lines: the sample's and the scatter pass's, none to slabs."""
    monkeypatch.setenv("W2RAP_TRACE", "1")
    monkeypatch.setenv("W2RAP_TEST_SLAB_SAMPLE_MIN", "64")
    c = _case(mods, name)
    n = len(c["off"]) - 1
    F, step2, O = mods
    pk, bo, ln = c["packed"]
    capfd.readouterr()
    routes = _check_stages(mods, c, capfd)
    assert routes == [("lane", "scatter", 0)] * 2, routes
    capfd.readouterr()
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=c["quals"], qual_off=c["off"])
        ctx.count_kmers(7, 4)
    err = capfd.readouterr().err
    m = re.search(r"partition: ~(\d+) records beyond slabs of 512 \(limit (\d+)\)", err)
    assert m and int(m.group(2)) == n // 10 and int(m.group(1)) > 3 * int(m.group(2)), err
    sample = re.findall(r"K1 route: lane, npass \d+, spp \d+, (\d+) reads", err)
    assert [int(x) for x in sample] == [n // 32, n], err


def test_sample_says_yes_but_the_list_overflows(mods, monkeypatch, capfd):
    """an asked input (the hook: from 64 reads on) whose sample holds none of the heavy buckets: the estimate stays under the limit, the
    cut to slabs needs a list of more than reads / 8 + 1024 entries, and such an input is not cut into slabs a second time -- nothing is
    kept, the scatter pass takes all reads.  Three K1 lines: the sample's, the refused cut's, the scatter pass's."""
    monkeypatch.setenv("W2RAP_TRACE", "1")
    monkeypatch.setenv("W2RAP_TEST_SLAB_SAMPLE_MIN", "64")
    c = _case(mods, "heavy_behind_the_sample")
    n = len(c["off"]) - 1
    assert HEAVY_COPIES - 512 > n // 8 + 1024                       # (a bucket holds a record of every copy: those beyond its slab alone pass the list)
    F, step2, O = mods
    pk, bo, ln = c["packed"]
    routes = _check_stages(mods, c, capfd)
    assert routes == [("lane", "scatter", 0), ("lane", "slabs", 512), ("lane", "scatter", 0)], routes
    capfd.readouterr()
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=c["quals"], qual_off=c["off"])
        ctx.count_kmers(7, 4)
    err = capfd.readouterr().err
    m = re.search(r"partition: ~(\d+) records beyond slabs of 512 \(limit (\d+)\)", err)
    assert m and int(m.group(2)) == n // 10 and int(m.group(1)) <= int(m.group(2)), err
    cut = re.findall(r"K1 route: lane, npass \d+, spp \d+, (\d+) reads", err)
    assert [int(x) for x in cut] == [n // 32, n, n], err
    assert "partition slabs:" not in err, err                       # (the line of a slab layout that was kept)


def test_fallback_two_passes(mods, monkeypatch, capfd):
    monkeypatch.setenv("W2RAP_TRACE", "1")
    routes = _check_stages(mods, _case(mods, "uniform"), capfd, n_passes=2)
    assert routes == [("lane", "scatter", 0)] * 2, routes
    monkeypatch.setenv("W2RAP_PASSES", "2")
    routes = _check_stages(mods, _case(mods, "uniform"), capfd)
    assert routes == [("lane", "scatter", 0)] * 2, routes


def test_fallback_long_read(mods, monkeypatch, capfd):
    monkeypatch.setenv("W2RAP_TRACE", "1")
    routes = _check_stages(mods, _case(mods, "long"), capfd)
    assert routes == [("wave", "scatter", 0)], routes


def test_fallback_two_ranks_on_one_device(mods, monkeypatch, capfd):
    F, step2, O = mods
    monkeypatch.setenv("W2RAP_TRACE", "1")
    c = _case(mods, "uniform"); orc = c["orc"]
    pk, bo, ln = c["packed"]
    capfd.readouterr()
    res = step2.build_read_qgraph(pk, bo, ln, quals=c["quals"], qual_off=c["off"], devices=[0, 0])
    routes = _routes(capfd.readouterr().err)
    assert routes and {r[1:] for r in routes} == {("scatter", 0)}, routes
    assert np.array_equal(res.hist, orc.hist)
    assert (res.n_kmer_instances, res.n_kmers_distinct, res.n_kmers_solid) == (orc.n_instances, orc.n_distinct, len(orc.k_hi))
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)
    assert (res.n_reads_pathed, res.n_reads_multipathed) == (orc.pathed, orc.multipathed)


def test_one_shot_call_takes_the_slabs(mods, monkeypatch, capfd):
    """the in-process call every caller uses (w2rap_step2_run), one GPU: the slab route, and the oracle's result"""
    F, step2, O = mods
    monkeypatch.setenv("W2RAP_TRACE", "1")
    c = _case(mods, "heavy"); orc = c["orc"]
    pk, bo, ln = c["packed"]
    capfd.readouterr()
    res = step2.build_read_qgraph(pk, bo, ln, quals=c["quals"], qual_off=c["off"])
    assert set(_routes(capfd.readouterr().err)) == {("lane", "slabs", 512)}
    assert np.array_equal(res.hist, orc.hist)
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_edges, orc.path_edges) and np.array_equal(res.path_off, orc.path_off)

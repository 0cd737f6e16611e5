"""k_count_fp_dedup after its instruction trims (NOTES.md section 20): the tag in the record table's words with 16-byte record reads in the
dedup stage, the hash-class test behind a uniform branch, the shorter canonical form and context bits in the window loop.  Every case is
Step 2 through the library against the CPU oracle -- histogram, solid k-mers with counts and pruned context bits, (edge, offset) per k-mer,
graph bytes and every path.  All integer work: equality, no tolerance.

W2RAP_TEST_DEDUP_TAG_MASK is ANDed to both tags before they are compared: 0 makes every held slot of a probe sequence a tag match (the
form before the tag: the content compare decides everywhere), 1 leaves one tag bit (half of all unequal records are false tag matches that
only the content compare rejects), unset is production.

The kernel's count of hash-class refinements (counters[2]) is not reachable from Python, so the hash-class cases prove the path from the
input instead: see test_hash_classes."""
import re

import numpy as np
import pytest

from test_gpu_record_dedup import _background, _case_short, _case_twins, _pack, _rc
from test_gpu_partition_slabs import _case_read_edges, _case_uniform, bucket_runs

pytestmark = pytest.mark.gpu

MASKS = pytest.mark.parametrize("mask", [None, "0", "1"])
TILES = {"22": 512, "24": 576}                   # W2RAP_K3 shape -> records of the resident tile (its record table: 1024 / 2048 entries)
RK = 4                                           # k-mers per record of the one-bucket cases: TILE x RK distinct k-mers stay below the table's fill limit


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    from w2rap_contigger_amd import formats as F, step2
    from oracle import oracle as O
    assert step2.lib().w2rap_step2_device_count() >= 1
    return F, step2, O


def _low_minimizer():
    """a 15-mer whose minimizer key (canonical value, bases LSB first, x 0x9E3779B1 mod 2^32: see bucket_runs) is smaller than any key a
    random 15-mer is likely to have: every k-mer that holds it goes to one bucket, in one record"""
    inv = pow(0x9E3779B1, -1, 1 << 32)
    for key in range(1, 1 << 16):
        c = (key * inv) & 0xFFFFFFFF
        if c >> 30:
            continue
        b = np.array([(c >> (2 * j)) & 3 for j in range(15)], np.uint8)
        r = _rc(b)
        if c <= sum(int(x) << (2 * j) for j, x in enumerate(r)):
            return b
    raise AssertionError("no 15-mer found")


def _one_bucket_records(rng, n):
    """n distinct reads of 60 + RK - 1 bases around the low minimizer: one record of RK k-mers each, all of one bucket.  The last four are
    windows of one sequence, one base apart: four different records that share a k-mer, so that the input has a solid k-mer (min_freq 4)"""
    mz = _low_minimizer()
    L = 60 + RK - 1
    R = rng.integers(0, 4, (n, L), dtype=np.uint8)
    R[:, 24:39] = mz                             # inside every k-mer of the read (k-mer i covers bases i .. i + 59, i < RK)
    y = rng.integers(0, 4, L + 3, dtype=np.uint8)
    y[24:39] = mz
    for j in range(4):
        R[n - 4 + j] = y[j:j + L]                # (the minimizer at 24 - j .. 38 - j: still inside every k-mer)
    assert len(np.unique(R, axis=0)) == n and (bucket_runs(R, 1 << 24) == 1).all()
    return [R[i].copy() for i in range(n)]


def _case_one_bucket(kind, tile):
    """the reads are the bucket: nothing else is in the input.
    distinct: TILE distinct records -- the record table half full, its design limit, probe sequences as long as they get.
    third:    3/4 TILE distinct records and a second copy of a third of them: TILE records all told (a tile holds no more), so the copies
              look for their holders in a table that is 3/8 full.
    pairs:    TILE / 2 distinct records twice: exactly TILE records, and records 0 and TILE - 1 of the tile, whichever they are, are each
              one of a pair -- the first and the last 16-byte reads of the tile.
    plus1:    pairs and one record more: TILE + 1 records, which the kernel defers to the list kernel."""
    rng = np.random.default_rng({"distinct": 71, "third": 72, "pairs": 73, "plus1": 74}[kind] * 1000 + tile)
    if kind == "distinct":
        reads = _one_bucket_records(rng, tile)
    elif kind == "third":
        reads = _one_bucket_records(rng, 3 * tile // 4)
        reads = reads + reads[:tile // 4]
    else:
        reads = _one_bucket_records(rng, tile // 2 + (kind == "plus1"))
        reads = reads + reads[:tile // 2]
    assert len(reads) == tile + (kind == "plus1")
    if kind == "plus1":
        reads.append(rng.integers(0, 4, 50, dtype=np.uint8))      # (reads come in pairs: the mate has no k-mer and adds no record)
    return _pack(reads, rng=rng)


def _case_copies():
    """seven random reads given 3, 63, 64, 65, 255, 256 and 511 times on one strand among the reads of a random genome, shuffled: with
    600 k-mers per bucket the copies of a read fill most of a tile, so that duplicates meet their holders across wave edges"""
    rng = np.random.default_rng(21)
    _, reads = _background(rng)
    for m in (3, 63, 64, 65, 255, 256, 511):
        reads += [rng.integers(0, 4, 150, dtype=np.uint8)] * m
    return _pack(reads, rng=rng)


def _case_canon():
    """k-mers at the edges of the canonical form: palindromes (a 30-mer and its reverse complement: neither strand is smaller); palindromes
    with one base changed at position 0, 15, 16 or 29, where the strands are told apart in the first word, at the last base of the first
    word, in the second word, or at the last base of the upper half (equal upper halves are a palindrome: the lower half never decides
    alone); A^61 and T^61; reads with their reverse complements; reads of 61 and 62 bases"""
    rng = np.random.default_rng(31)
    g, reads = _background(rng)

    def embed(kmer):
        return np.concatenate([rng.integers(0, 4, 45, dtype=np.uint8), kmer, rng.integers(0, 4, 45, dtype=np.uint8)]).astype(np.uint8)

    for _ in range(4):
        w = rng.integers(0, 4, 30, dtype=np.uint8)
        pal = np.concatenate([w, _rc(w)])
        assert np.array_equal(pal, _rc(pal))
        reads += [embed(pal)] * 5
        for p in (0, 15, 16, 29):
            for d in (1, 2, 3):
                q = pal.copy(); q[p] = (q[p] + d) % 4
                r = embed(q)
                reads += [r] * 3 + [_rc(r)] * 3
    reads += [np.zeros(61, np.uint8)] * 5 + [np.full(61, 3, np.uint8)] * 5
    for s in rng.integers(0, len(g) - 150, 6):
        r = g[s:s + 150].copy()
        reads += [r] * 3 + [_rc(r)] * 3
    for n in (61, 62):
        r = rng.integers(0, 4, n, dtype=np.uint8)
        reads += [r] * 5 + [_rc(r)] * 5
    return _pack(reads, rng=rng)


_CASES = {"copies": _case_copies, "twins": _case_twins, "short": _case_short, "uniform": _case_uniform, "read_edges": _case_read_edges,
          "canon": _case_canon,
          **{f"{kind}{t}": (lambda kind=kind, t=t: _case_one_bucket(kind, t)) for kind in ("distinct", "third", "pairs", "plus1") for t in TILES.values()}}
_cache = {}


def _case(mods, name):
    """reads, packed reads and the oracle's result: computed once per module, never changed"""
    if name not in _cache:
        F, step2, O = mods
        codes, quals, off = _CASES[name]()
        _cache[name] = dict(codes=codes, quals=quals, off=off, packed=F.pack_bases(codes, off), orc=O.run(codes, quals, off))
    return _cache[name]


def _check_stages(mods, c, capfd):
    """Step 2 stage by stage against the oracle; -> the buckets k_count_fp deferred to the list kernel"""
    F, step2, O = mods
    orc = c["orc"]
    pk, bo, ln = c["packed"]
    capfd.readouterr()
    with step2.Step2Context(0) as ctx:
        ctx.set_reads_host(pk, bo, ln, quals=c["quals"], qual_off=c["off"])
        st = ctx.count_kmers(7, 4)
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
    err = capfd.readouterr().err
    m = re.findall(r"k_count_fp deferred (\d+) buckets", err)
    assert len(m) == 1, err
    return int(m[0]), err


def _run(mods, monkeypatch, capfd, name, env):
    monkeypatch.setenv("W2RAP_TRACE", "1")
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, v)
    deferred, err = _check_stages(mods, _case(mods, name), capfd)
    for k, v in env.items():                      # a test hook that is honoured says so
        if k.startswith("W2RAP_TEST_") and v is not None:
            assert f"test hook {k} is set" in err
    return deferred


# ---- the tag path

@MASKS
def test_copies_across_wave_edges(mods, monkeypatch, capfd, mask):
    _run(mods, monkeypatch, capfd, "copies", {"W2RAP_KPB": "600", "W2RAP_TEST_DEDUP_TAG_MASK": mask})


@MASKS
def test_twins_stay_apart(mods, monkeypatch, capfd, mask):
    """both strands, a read ending inside the other's super-k-mer, one flank or the last base changed, 63-k-mer records differing in the
    last base: equal or not is decided by the eight dwords whatever the tags say"""
    _run(mods, monkeypatch, capfd, "twins", {"W2RAP_TEST_DEDUP_TAG_MASK": mask})


@MASKS
@pytest.mark.parametrize("kind", ["distinct", "third"])
@pytest.mark.parametrize("shape", sorted(TILES))
def test_record_table_at_its_limit(mods, monkeypatch, capfd, shape, kind, mask):
    """one bucket of exactly TILE records, counted in the tile (nothing deferred): see _case_one_bucket"""
    d = _run(mods, monkeypatch, capfd, f"{kind}{TILES[shape]}", {"W2RAP_K3": shape, "W2RAP_KPB": "600", "W2RAP_TEST_DEDUP_TAG_MASK": mask})
    assert d == 0


# ---- 16-byte record reads

@pytest.mark.parametrize("shape", sorted(TILES))
def test_first_and_last_record_of_a_full_tile(mods, monkeypatch, capfd, shape):
    assert _run(mods, monkeypatch, capfd, f"pairs{TILES[shape]}", {"W2RAP_K3": shape, "W2RAP_KPB": "600"}) == 0


@pytest.mark.parametrize("shape", sorted(TILES))
def test_one_record_more_than_the_tile(mods, monkeypatch, capfd, shape):
    """TILE + 1 records: the bucket goes to the list kernel and stays exact"""
    assert _run(mods, monkeypatch, capfd, f"plus1{TILES[shape]}", {"W2RAP_K3": shape, "W2RAP_KPB": "600"}) == 1


@pytest.mark.parametrize("name", ["copies", "third512"])
def test_two_segments(mods, monkeypatch, name):
    """two ranks on one device: every bucket's records come as two segments of the tile"""
    F, step2, O = mods
    monkeypatch.setenv("W2RAP_KPB", "600")
    c = _case(mods, name); orc = c["orc"]
    pk, bo, ln = c["packed"]
    res = step2.build_read_qgraph(pk, bo, ln, quals=c["quals"], qual_off=c["off"], devices=[0, 0])
    assert np.array_equal(res.hist, orc.hist)
    assert (res.n_kmer_instances, res.n_kmers_distinct, res.n_kmers_solid) == (orc.n_instances, orc.n_distinct, len(orc.k_hi))
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)
    assert (res.n_reads_pathed, res.n_reads_multipathed) == (orc.pathed, orc.multipathed)


# ---- the window loop: hash classes

@pytest.mark.parametrize("dedup", [None, "0"])
@pytest.mark.parametrize("hook,limit,least_p", [(None, None, 1), ("W2RAP_TEST_FP_SC", 64, 2), ("W2RAP_TEST_FP_SC", 32, 4), ("W2RAP_TEST_FP_SC", 6, 16),
                                                ("W2RAP_TEST_FP_LIMIT", 64, 2), ("W2RAP_TEST_FP_LIMIT", 32, 4), ("W2RAP_TEST_FP_LIMIT", 8, 16)])
def test_hash_classes(mods, monkeypatch, capfd, dedup, hook, limit, least_p):
    """One input counted with P == 1 and with buckets refined to P = 2, 4 and 16 or more classes.  That the refinement happens follows from
    the input: the solid k-mers fall into NB = instances / 4500 + 1 buckets, so one bucket holds at least S / NB of them; a class is emitted
    only if its solid k-mers number at most W2RAP_TEST_FP_SC (an exact test in the kernel), so that bucket -- it is counted in the tile:
    nothing is deferred -- ends at P >= S / NB / limit classes, P a power of two.  W2RAP_TEST_FP_LIMIT bounds the DISTINCT k-mers a class may
    put into the table (there are more of them than solid ones), tested between windows, so the same limits refine at least as far."""
    orc = _case(mods, "uniform")["orc"]
    if hook:
        per_bucket = -(-len(orc.k_hi) // (orc.n_instances // 4500 + 1))
        assert -(-per_bucket // limit) > least_p // 2, (per_bucket, limit)
    d = _run(mods, monkeypatch, capfd, "uniform", {"W2RAP_FP_DEDUP": dedup, **({hook: str(limit)} if hook else {})})
    assert d == 0


# ---- the window loop: canonical form and context bits

@pytest.mark.parametrize("fused", [None, "1"])
@pytest.mark.parametrize("name", ["canon", "short", "read_edges"])
def test_canonical_form_and_context(mods, monkeypatch, capfd, name, fused):
    """palindromes and near-palindromes, homopolymers, both strands, records of one to three k-mers (canon, short); context bits at both ends of
    a record with header flags 64 and 128 set and unset (read_edges) -- with the fused prune, which builds its neighbours' keys through
    fp_key too, and without"""
    _run(mods, monkeypatch, capfd, name, {"W2RAP_FUSED_PRUNE": fused})

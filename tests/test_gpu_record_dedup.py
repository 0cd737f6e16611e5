"""k_count_fp counts byte-identical super-k-mer records of a bucket once, with their multiplicity as the weight (W2RAP_FP_DEDUP=0: every record
on its own).  Hand-made reads whose records repeat -- or nearly repeat -- against the CPU oracle: histogram, solid k-mers with counts and pruned
context bits, (edge, offset) per k-mer, graph bytes and every path, with the switch on and off.  All integer work: equality, no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MULTS = (3, 64, 65, 255, 256, 300, 511)        # around the wavefront width, around 255/256 (the width of a weight), near the 512-record tile


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


def _background(rng, glen=6000, n=2400):
    """reads of both strands over a random genome (~60x): the buckets the special reads fall into are real ones"""
    g = rng.integers(0, 4, glen, dtype=np.uint8)
    out = []
    for s in rng.integers(0, glen - 150, n):
        r = g[s:s + 150]
        out.append(_rc(r) if rng.integers(0, 2) else r.copy())
    return g, out


def _pack(reads, quals=None, rng=None):
    reads = list(reads)
    quals = [np.full(len(r), 35, np.uint8) for r in reads] if quals is None else list(quals)
    if len(reads) % 2:
        reads.append(reads[0]); quals.append(quals[0])
    if rng is not None:                                  # shuffled in pairs: the copies of a read arrive from all over the input
        order = rng.permutation(len(reads) // 2)
        reads = [reads[2 * i + j] for i in order for j in (0, 1)]; quals = [quals[2 * i + j] for i in order for j in (0, 1)]
    lens = np.array([len(r) for r in reads], np.uint64)
    off = np.zeros(len(reads) + 1, np.uint64); np.cumsum(lens, out=off[1:])
    return np.concatenate(reads).astype(np.uint8), np.concatenate(quals).astype(np.uint8), off


def _case_copies(mults, seed):
    rng = np.random.default_rng(seed)
    _, reads = _background(rng)
    for m in mults:
        r = rng.integers(0, 4, 150, dtype=np.uint8)
        reads += [r] * m
    return _pack(reads, rng=rng)


def _case_twins():
    """records that are ALMOST equal and must stay apart: a locus read on both strands; a read and its prefix that ends inside the longer one's
    super-k-mers (the has-successor flag of the header differs); reads that differ in their first or their last base only (40 loci each: where the
    changed base is the flank of the neighbouring record, the records differ in nothing else; where it is inside, in one base of the record);
    and 63-k-mer records (122 bases of a tandem repeat of period 30: one minimizer, one record) that differ in their last base only"""
    rng = np.random.default_rng(4242)
    g, reads = _background(rng)
    for s in rng.integers(0, len(g) - 150, 12):
        r = g[s:s + 150].copy()
        reads += [r] * 5 + [_rc(r)] * 5                                   # both strands
        reads += [r[:int(rng.integers(70, 140))].copy()] * 5              # ends inside
    for s in rng.integers(0, len(g) - 150, 40):
        r = g[s:s + 150].copy()
        a = r.copy(); a[-1] = (a[-1] + 1 + rng.integers(0, 3)) % 4
        b = r.copy(); b[0] = (b[0] + 1 + rng.integers(0, 3)) % 4
        reads += [r] * 4 + [a] * 4 + [b] * 4
    for _ in range(3):
        t = np.tile(rng.integers(0, 4, 30, dtype=np.uint8), 5)[:122]
        u = t.copy(); u[-1] = (u[-1] + 1) % 4
        reads += [t] * 6 + [u] * 6
    return _pack(reads, rng=rng)


def _case_short():
    """61 and 62 good bases, 100 times each: records of one, two and three k-mers -- as short reads, and as 150-base reads whose tail is of quality 2"""
    rng = np.random.default_rng(99)
    _, reads = _background(rng)
    quals = [np.full(150, 35, np.uint8) for _ in reads]
    for n in (61, 62):
        r = rng.integers(0, 4, n, dtype=np.uint8)
        reads += [r] * 100; quals += [np.full(n, 35, np.uint8)] * 100
        r = rng.integers(0, 4, 150, dtype=np.uint8)
        reads += [r] * 100; quals += [np.concatenate([np.full(n, 35, np.uint8), np.full(150 - n, 2, np.uint8)])] * 100
    return _pack(reads, quals, rng=rng)


_CASES = {"copies": lambda: _case_copies(MULTS, 11), "c513": lambda: _case_copies((513,), 12), "c700": lambda: _case_copies((700,), 13),
          "c20000": lambda: _case_copies((20000,), 14), "twins": _case_twins, "short": _case_short}
_cache = {}


def _case(mods, name):
    """reads, packed reads and the oracle's result: computed once per module, never changed"""
    if name not in _cache:
        F, step2, O = mods
        codes, quals, off = _CASES[name]()
        _cache[name] = dict(codes=codes, quals=quals, off=off, packed=F.pack_bases(codes, off), orc=O.run(codes, quals, off))
    return _cache[name]


def _check_stages(mods, c):
    F, step2, O = mods
    orc = c["orc"]
    pk, bo, ln = c["packed"]
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


SWITCH = pytest.mark.parametrize("dedup", ["1", "0"])


@SWITCH
@pytest.mark.parametrize("kpb", [None, "600"])
def test_one_read_many_times(mods, monkeypatch, dedup, kpb):
    """seven random reads, given 3 .. 511 times each on one strand, among the reads of a random genome; with 600 k-mers per bucket a bucket holds
    few other records beside the copies, so that the larger multiplicities can fit the resident tile"""
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    if kpb:
        monkeypatch.setenv("W2RAP_KPB", kpb)
    _check_stages(mods, _case(mods, "copies"))


@SWITCH
@pytest.mark.parametrize("name", ["c513", "c700", "c20000"])
def test_more_copies_than_the_tile_holds(mods, monkeypatch, dedup, name):
    """513 and 700 copies: the bucket goes to the list kernel; 20 000: far beyond the tile and, flattened, beyond MAXK"""
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    monkeypatch.setenv("W2RAP_KPB", "600")
    _check_stages(mods, _case(mods, name))


@SWITCH
def test_twins_that_must_not_merge(mods, monkeypatch, dedup):
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    _check_stages(mods, _case(mods, "twins"))


@SWITCH
@pytest.mark.parametrize("env", [{"W2RAP_TEST_FP_LIMIT": "16"}, {"W2RAP_TEST_FP_SC": "6"}])
def test_hash_classes_apply_the_weight_in_every_pass(mods, monkeypatch, dedup, env):
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_stages(mods, _case(mods, "copies"))


@SWITCH
def test_duplicates_arrive_in_two_segments(mods, monkeypatch, dedup):
    """two ranks on one device: every bucket's records come as two segments of the tile"""
    F, step2, O = mods
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    c = _case(mods, "copies"); orc = c["orc"]
    pk, bo, ln = c["packed"]
    res = step2.build_read_qgraph(pk, bo, ln, quals=c["quals"], qual_off=c["off"], devices=[0, 0])
    assert np.array_equal(res.hist, orc.hist)
    assert (res.n_kmer_instances, res.n_kmers_distinct, res.n_kmers_solid) == (orc.n_instances, orc.n_distinct, len(orc.k_hi))
    assert F.hbv_to_bytes(res.hbv) == F.hbv_to_bytes(O.to_hbv(orc))
    assert np.array_equal(res.path_offset, orc.path_offset) and np.array_equal(res.path_off, orc.path_off)
    assert np.array_equal(res.path_edges, orc.path_edges)
    assert (res.n_reads_pathed, res.n_reads_multipathed) == (orc.pathed, orc.multipathed)


@SWITCH
@pytest.mark.parametrize("env", [{"W2RAP_FUSED_PRUNE": "1"}, {"W2RAP_K3": "20"}, {"W2RAP_K3": "24"}])
def test_fused_prune_and_other_shapes(mods, monkeypatch, dedup, env):
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_stages(mods, _case(mods, "copies"))


@SWITCH
def test_records_of_one_and_two_kmers(mods, monkeypatch, dedup):
    monkeypatch.setenv("W2RAP_FP_DEDUP", dedup)
    _check_stages(mods, _case(mods, "short"))

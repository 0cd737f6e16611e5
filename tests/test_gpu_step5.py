"""Step 5's tail on the GPU (w2rap_step5_partners_to_ends) against recorded runs of the reference's own PartnersToEnds (replayed from
tests/golden/refruns/step5_tail_<case>/) and against its CPU model (step5_model.py): the hand-made cases, seeded small random cases, two
generated cases behind the library's own Steps 2-4, the early return, argument errors, and a second call in the same process."""
import ctypes as C

import numpy as np
import pytest

import step5_cases as S
import step5_model as M
from conftest import _host_reads
from w2rap_contigger_amd import formats as F, step2, step3, step4, step5

pytestmark = pytest.mark.gpu

CASES = S.cases()
E_ARG = 1          # W2RAP_E_ARG (w2rap_step2.h)


def _same(res, m):
    assert res.counters == m.counters
    assert np.array_equal(res.path_off, m.path_off)
    assert np.array_equal(res.path_edges, m.path_edges)
    assert np.array_equal(res.path_offset, m.path_offset)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_cases(name):
    c = CASES[name]
    h, paths, reads, quals = c.inputs()
    res = step5.partners_to_ends(h, paths, reads, quals)
    po = res.path_off.astype(np.int64)
    for r, (path, offset) in c.expect.items():
        assert (list(res.path_edges[po[r]:po[r + 1]]), int(res.path_offset[r])) == (path, offset), f"read {r}"
    for k, v in c.counters.items():
        assert res.counters[k] == v, k
    _same(res, M.partners_to_ends(h, paths, reads, quals))


@pytest.mark.parametrize("name", S.recorded())
def test_equals_the_recorded_reference(name, tmp_path):
    """replay only: the reference's t.out.paths for the case's inputs, recorded where the reference was at hand"""
    offset, path_off, edges = S.reference_run(name, str(tmp_path))
    res = step5.partners_to_ends(*S.inputs_of(name))
    assert np.array_equal(res.path_off, path_off)
    assert np.array_equal(res.path_edges, edges)
    assert np.array_equal(res.path_offset, offset)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_against_the_model_on_random_cases(seed):
    h, paths, reads, quals = S.inputs_of(f"random_{seed}")
    m = M.partners_to_ends(h, paths, reads, quals)
    print(f"seed {seed}: {h.n_edges} edges, {len(reads[2])} reads; model {m.counters} {m.extra}")
    assert S.seed_conditions(m) == []          # every branch occurs, by the model's own count
    res = step5.partners_to_ends(h, paths, reads, quals)
    _same(res, m)
    assert step5.profile().get("k5_verify", (0, 0))[1] == 1


# ---- generated: the planted workload through Steps 2, 3 and 4 of this library, then a seeded 5 % of the reads lose their paths
_GENERATED = {}


def blank_and_plant(h, clean_paths, r, blank_seed):
    """the CPU half of the recipe: a seeded 5 % of the reads lose their paths, two 28-mers are planted -> (paths, reads, quals, note).
    20,000 reads at 30x do not reach a multiplicity of 80 by themselves, so two 28-mers go into unplaced reads whose mate ends near an end,
    at quality 2: A, random, into 81 such reads (the first filter drops it); B, the first 28 bases of the longest edge, into as many as
    bring its count in those reads to exactly 80 (kept by the first filter, dropped by the second: 80 + its occurrences in the edges)."""
    n = len(r["ln"])
    rng = np.random.default_rng(blank_seed)
    blank = rng.random(n) < 0.05
    po = np.asarray(clean_paths[1]).astype(np.int64)
    plen = np.diff(po); plen[blank] = 0
    keep = np.repeat(~blank, np.diff(po))
    npo = np.zeros(n + 1, np.uint64); np.cumsum(plen, out=npo[1:])
    offset = np.array(clean_paths[0], np.int32); offset[blank] = 0
    paths = (offset, npo, np.asarray(clean_paths[2])[keep])
    # the reads the call will look up, as the model's own rule names them
    near = M.near_end_edges(h)
    np_ = npo.astype(np.int64)
    ids = [x for x in range(n) if np_[x + 1] == np_[x] and np_[(x ^ 1) + 1] > np_[x ^ 1] and near[int(paths[2][np_[(x ^ 1) + 1] - 1])]]
    codes = r["codes"].copy(); quals = r["quals"].copy()
    off = r["off"].astype(np.int64)
    A = rng.integers(0, 4, 28).astype(np.uint8)
    ecodes, eoff = h.edge_codes()
    e_long = int(np.argmax(h.edge_len)); B = ecodes[int(eoff[e_long]):int(eoff[e_long]) + 28].copy()
    has_b = [x for x in ids if bytes(B) in bytes(codes[off[x]:off[x + 1]])]
    for x in ids[:81]:
        codes[off[x]:off[x] + 28] = A; quals[off[x]:off[x] + 28] = 2
    for x in [x for x in ids if x not in has_b][:max(0, 80 - len(has_b))]:
        codes[off[x] + 40:off[x] + 68] = B; quals[off[x] + 40:off[x] + 68] = 2
    return paths, F.pack_bases(codes, r["off"]), quals, f"{h.n_edges} edges, {int(blank.sum())} blanked, {len(ids)} to look up"


def host_planted_reads(n_reads, seed):
    """bench.planted_reads made on the CPU, so that the reads -- and with them what the seeds below were chosen for -- are the same
    on every machine"""
    import torch
    import bench
    return _host_reads(bench.planted_reads(n_reads, seed, torch.device("cpu")))


def generated(n_reads, seed, blank_seed, min_freq):
    """-> (hbv, paths, reads, quals, note): the planted workload through Steps 2, 3 and 4 of this library, then blank_and_plant"""
    key = (n_reads, seed, blank_seed, min_freq)
    if key not in _GENERATED:
        r = host_planted_reads(n_reads, seed)
        r2 = step2.build_read_qgraph(r["pk"], r["bo"], r["ln"], quals=r["quals"], qual_off=r["off"], min_freq=min_freq)
        r3 = step3.repath_in_memory(r2.hbv, (r2.path_offset, r2.path_off, r2.path_edges), 200)
        r4 = step4.clean200x(r3.hbv, (r3.path_offset, r3.path_off, r3.path_edges), r["pk"], r["bo"], r["ln"], r["quals"], inv=r3.inv2)
        _GENERATED[key] = (r4.hbv,) + blank_and_plant(r4.hbv, (r4.path_offset, r4.path_off, r4.path_edges), r, blank_seed)
    return _GENERATED[key]


# (n_reads, seed of the reads, seed of the blanking, min_freq of Step 2): seeds at which the model meets every condition asserted below
GENERATED = [(20_000, 5, 1, 2), (12_000, 8, 4, 2)]


@pytest.mark.parametrize("n_reads,seed,blank_seed,min_freq", GENERATED)
def test_against_the_model_on_generated_reads(n_reads, seed, blank_seed, min_freq):
    h, paths, reads, quals, note = generated(n_reads, seed, blank_seed, min_freq)
    m = M.partners_to_ends(h, paths, reads, quals)
    print(f"generated {n_reads}/{seed}/{blank_seed}: {note}; model {m.counters} {m.extra}")
    # every outcome occurs, by the model's own count
    assert m.counters["n_placed"] > 0 and m.counters["n_ambiguous"] > 0
    assert m.extra["n_rejected"] > 0
    assert m.extra["n_dropped_by_reads"] > 0 and m.extra["n_dropped_by_total"] > 0
    res = step5.partners_to_ends(h, paths, reads, quals)
    _same(res, m)
    assert step5.profile().get("k5_verify", (0, 0))[1] == 1


def test_nothing_to_look_up_returns_the_paths():
    """every read placed: n_interesting == 0, the reference returns at once"""
    c = S.Case(40); Mm, T, _ = c.scene()
    for i in range(6):
        c.read(c.eseq(T)[10 * i:10 * i + 100], 35, [T], 10 * i)
    h, paths, reads, quals = c.inputs()
    res = step5.partners_to_ends(h, paths, reads, quals)
    assert res.counters == dict.fromkeys(step5.COUNTERS, 0)
    assert np.array_equal(res.path_off, paths[1]) and np.array_equal(res.path_edges, paths[2]) and np.array_equal(res.path_offset, paths[0])
    assert "k5_emit" not in step5.profile() and "k5_flag" in step5.profile()


def test_argument_errors():
    c = CASES["odd_and_even_ids"]
    h, paths, reads, quals = c.inputs()
    # an odd number of paths (and of reads, so that it is the oddness that is refused)
    odd_paths = (paths[0][:-1], paths[1][:-1], paths[2][:int(paths[1][-2])])
    odd_reads = (reads[0][:int(reads[1][-2])], reads[1][:-1], reads[2][:-1])
    with pytest.raises(step2.Step2Error) as e:
        step5.partners_to_ends(h, odd_paths, odd_reads, quals[:int(np.sum(odd_reads[2]))])
    assert e.value.code == E_ARG and "odd" in str(e.value)
    bad = paths[2].copy(); bad[0] = h.n_edges
    with pytest.raises(step2.Step2Error) as e:
        step5.partners_to_ends(h, (paths[0], paths[1], bad), reads, quals)
    assert e.value.code == E_ARG and "edge object that does not exist" in str(e.value)
    qo = np.zeros(len(reads[2]) + 1, np.uint64); np.cumsum(reads[2], out=qo[1:]); qo[1] -= 1      # the first read one quality short
    with pytest.raises(step2.Step2Error) as e:
        step5.partners_to_ends(h, paths, reads, quals, qual_off=qo)
    assert e.value.code == E_ARG and "qual_off does not match read_len" in str(e.value)


def _idle_context_bytes():
    """live device bytes of the cached context the one-shot entry points use (taken from the cache and handed back)"""
    L = step5.lib()
    L.w2rap_step2_acquire.restype = C.c_void_p
    L.w2rap_step2_acquire.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.w2rap_step2_release.restype = None
    L.w2rap_step2_release.argtypes = [C.c_void_p]
    L.w2rap_step2_device_bytes.restype = C.c_uint64
    L.w2rap_step2_device_bytes.argtypes = [C.c_void_p]
    err = C.create_string_buffer(256)
    ctx = L.w2rap_step2_acquire(0, err, 256)
    assert ctx, err.value
    try:
        return int(L.w2rap_step2_device_bytes(ctx))
    finally:
        L.w2rap_step2_release(ctx)


def test_second_call_in_one_process():
    c = CASES["65_interesting_reads"]
    h, paths, reads, quals = c.inputs()
    before = _idle_context_bytes()
    a = step5.partners_to_ends(h, paths, reads, quals)
    b = step5.partners_to_ends(h, paths, reads, quals)
    assert a.counters == b.counters and a.counters["n_placed"] == 65
    assert np.array_equal(a.path_off, b.path_off) and np.array_equal(a.path_edges, b.path_edges) and np.array_equal(a.path_offset, b.path_offset)
    assert _idle_context_bytes() == before

"""A small CPU restatement of the last line of the reference's Step 5, PartnersToEnds (src/paths/long/large/GapToyTools5.cc:1150-1517,
with DistancesToEndArr, src/graph/DigraphTemplate.h:1581-1619): dictionaries of Python ints and one loop per candidate, written to be
read next to the reference.  It is deliberately naive and shares no code with the binding (w2rap_contigger_amd/step5.py) or the
kernels.  test_step5_model.py pins it to hand-made cases whose outcomes are written down as literals; test_gpu_step5.py then uses it
to judge the HIP library.

    partners_to_ends(hbv, paths, reads, quals) -> Model5Result

Two things differ from a literal transcription, neither of which changes a result:
  * the distance cap.  findInterestingReadIds calls DistancesToEndArr with max_dist = 10,000,000 and asks only D <= 500.  Here the cap
    is 501 (`distances_to_end(..., max_dist=501)`).  Equivalent: the worklist only ever raises D, and it refuses to raise a vertex only
    once that vertex is >= max_dist.  A vertex all of whose walks to a sink are <= 500 K-mers has only such vertices downstream, none of
    them is ever refused, and its D is the exact longest walk, whatever the cap (> 500).  A vertex with a walk of more than 500 K-mers to a
    sink, v0 -> v1 -> ... -> sink: whenever D[v_(i+1)] reaches its final value that vertex is processed afterwards and lifts D[v_i] to
    at least min(max_dist, that walk's remaining length), so D[v0] >= 501 with either cap.  A vertex that reaches no sink keeps -1 and
    is set to max_dist: > 500 with either cap.
  * isGood is evaluated for EVERY distinct candidate.  The reference skips it for a read already marked NOT_AN_EDGE (:1395), which
    saves time and, thread order deciding who is first, changes nothing that is kept: a read is placed if and only if exactly one of its
    candidates is good.  n_good counts all good candidates."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from w2rap_contigger_amd import formats as F

KLEN = 28                    # :1152
MAX_MULTIPLICITY = 80        # :1481
WINDOW, MAX_MISMATCHES, TRUSTED_QUAL = 60, 4, 30      # :1367-1369
GOOD_DIST = 500              # :1163
NOT_AN_EDGE = -1             # :1371


def distances_to_end(hbv: F.HBV, max_dist: int):
    """DistancesToEndArr with fw = True (DigraphTemplate.h:1581-1619) on edge lengths in K-mers (GapToyTools5.cc:1166): D[v] = the
    longest walk from v to a sink, the worklist itself, statement for statement"""
    nv = hbv.n_vertices
    fo = [int(x) for x in hbv.from_off]; to = [int(x) for x in hbv.to_off]
    to_e = [int(x) for x in hbv.to_e]
    to_left, _ = hbv.to_left_right()
    edge_lens = [int(l) - hbv.K + 1 for l in hbv.edge_len]
    D = [-1] * nv                                                     # :1588
    to_process = [False] * nv; to_processx = []
    for v in range(nv):                                               # :1589-1599
        if fo[v + 1] == fo[v]:                                        # G.Sink(v)
            D[v] = 0
            to_process[v] = True; to_processx.append(v)
    while to_processx:                                                # :1603-1617
        v = to_processx.pop()
        to_process[v] = False
        for j in range(to[v], to[v + 1]):
            e = to_e[j]
            w = int(to_left[e])                                       # G.To(v)[j]
            if D[w] >= max_dist:
                continue
            dw_new = edge_lens[e] + D[v]
            if dw_new > D[w]:
                D[w] = dw_new
                if not to_process[w]:
                    to_process[w] = True; to_processx.append(w)
    return [max_dist if d < 0 else d for d in D]                      # :1618-1619


def near_end_edges(hbv: F.HBV, max_dist=GOOD_DIST + 1):
    """endEdges of findInterestingReadIds (:1159-1171): per edge object, D[to_right[e]] <= 500"""
    D = distances_to_end(hbv, max_dist)
    _, to_right = hbv.to_left_right()
    return [D[int(v)] <= GOOD_DIST for v in to_right]


def _kmers(seq):
    """the 28-mers of a base-code sequence as Python ints, position by position (KMer<28>(itr) then toSuccessor, :1292-1295)"""
    if len(seq) < KLEN:
        return []
    out = []
    x = 0
    for i, b in enumerate(seq):
        x = ((x << 2) | int(b)) & ((1 << (2 * KLEN)) - 1)
        if i >= KLEN - 1:
            out.append(x)
    return out


def is_good(read, qual, edge, loc_offset):
    """EdgeProc::isGood (:1424-1449) with iterators written as indices"""
    offset = -loc_offset
    r_beg, r_end = 0, len(read)
    e_beg, e_end = 0, len(edge)
    q = 0
    if offset >= 0:
        e_beg += offset
    else:
        r_beg -= offset; q -= offset
    if e_end - e_beg < WINDOW or r_end - r_beg < WINDOW:
        return False
    r, e = r_beg, e_beg
    mismatches = 0
    while r != r_beg + WINDOW:
        if read[r] != edge[e]:
            if qual[q] >= TRUSTED_QUAL:
                return False
            mismatches += 1
        r += 1; e += 1; q += 1
    good = mismatches <= MAX_MISMATCHES
    while r != r_end and e != e_end:
        if read[r] != edge[e]:
            if qual[q] >= TRUSTED_QUAL:
                return False
            mismatches += 1
        if read[r_beg] != edge[e_beg]:
            mismatches -= 1
        if mismatches <= MAX_MISMATCHES:
            good = True
        r += 1; e += 1; q += 1; r_beg += 1; e_beg += 1
    return good


@dataclass
class Model5Result:
    path_offset: np.ndarray
    path_off: np.ndarray
    path_edges: np.ndarray
    counters: dict                       # the library's counters (step5.COUNTERS) ...
    extra: dict = field(default_factory=dict)   # ... and what only the model counts: n_dropped_by_reads, n_dropped_by_total, n_rejected


def partners_to_ends(hbv: F.HBV, paths, reads, quals) -> Model5Result:
    """PartnersToEnds (:1462-1517).  paths = (offset, path_off, edges); reads = (packed, byte_off, read_len); quals one byte per base"""
    codes, off = F.unpack_bases(*reads)
    off = [int(x) for x in off]
    n = len(off) - 1
    po = [int(x) for x in paths[1]]
    path = [[int(e) for e in paths[2][po[r]:po[r + 1]]] for r in range(n)]
    offs = [int(x) for x in paths[0]]
    ecodes, eoff = hbv.edge_codes()
    eoff = [int(x) for x in eoff]
    edges = [ecodes[eoff[e]:eoff[e + 1]] for e in range(hbv.n_edges)]
    read = lambda r: codes[off[r]:off[r + 1]]
    qual = lambda r: quals[off[r]:off[r + 1]]

    # findInterestingReadIds (:1154-1194)
    end_edges = near_end_edges(hbv)
    ids = []; n_kmers = 0
    for r in range(n):
        if not path[r]:
            mate = path[r ^ 1]
            if mate and end_edges[mate[-1]]:
                if off[r + 1] - off[r] >= KLEN:
                    ids.append(r); n_kmers += off[r + 1] - off[r] - KLEN + 1
    counters = dict(n_interesting=len(ids), n_read_kmers=n_kmers, n_dict_kmers=0, n_candidates=0, n_good=0, n_placed=0, n_ambiguous=0)
    extra = dict(n_dropped_by_reads=0, n_dropped_by_total=0, n_rejected=0)

    def result():
        npo = np.zeros(n + 1, np.uint64)
        if n:
            np.cumsum([len(p) for p in path], out=npo[1:])
        return Model5Result(np.array(offs, np.int32), npo, np.array([e for p in path for e in p], np.int32), counters, extra)
    if not ids:                                                       # :1473
        return result()

    # MREReadProc (:1277-1327): kmer -> [(read, offset)]; more than 80 locations: the k-mer never enters the dictionary
    locs = {}
    for r in ids:
        for o, km in enumerate(_kmers(read(r))):
            locs.setdefault(km, []).append((r, o))
    for km in [k for k, v in locs.items() if len(v) > MAX_MULTIPLICITY]:
        del locs[km]; extra["n_dropped_by_reads"] += 1
    # MREEdgeProc (:1331-1361): occurrences of the dictionary's k-mers over all edge objects
    elocs = dict.fromkeys(locs, 0)
    ekm = [_kmers(s) for s in edges]
    for kms in ekm:
        for km in kms:
            if km in elocs:
                elocs[km] += 1
    # the remove_if (:1501)
    for km in [k for k in locs if len(locs[k]) + elocs[k] > MAX_MULTIPLICITY]:
        del locs[km]; extra["n_dropped_by_total"] += 1
    counters["n_dict_kmers"] = len(locs)

    # EdgeProc::operator() (:1378-1404), edge by edge; addLocs' look at the tail of mLocs (:1413-1420) only thins what sort + unique removes
    for e, kms in enumerate(ekm):
        m_locs = []
        for e_offset, km in enumerate(kms):
            for (r, o) in locs.get(km, ()):
                m_locs.append((r, o - e_offset))
        m_locs = sorted(set(m_locs))
        counters["n_candidates"] += len(m_locs)
        for (r, lo) in m_locs:
            if is_good(read(r), qual(r), edges[e], lo):
                counters["n_good"] += 1
                if path[r]:
                    path[r][0] = NOT_AN_EDGE                          # :1400
                else:
                    path[r].append(e); offs[r] = -lo                  # :1402-1403
    extra["n_rejected"] = counters["n_candidates"] - counters["n_good"]
    # cleanAmbiguousPlacements (:1406-1410)
    for r in ids:
        if path[r] and path[r][0] == NOT_AN_EDGE:
            path[r] = []; offs[r] = 0
            counters["n_ambiguous"] += 1
        elif path[r]:
            counters["n_placed"] += 1
    return result()

"""A small CPU restatement of the three read-sized passes at the front of the reference's Step 5, written to be read next to it:

    invert(pathsr, paths_inv, E)      src/modules/w2rap-contigger.cc:427, src/VecUtilities.h:693
    Phase 1 of Unsat                  src/paths/long/large/Unsat.cc:142-207
    LayoutReads                       src/paths/long/large/GapToyTools2.cc:550-588

Plain lists and dicts, one loop per read or pair.  It is deliberately naive and shares no code with the binding
(w2rap_contigger_amd/step5.py) or the kernels.  The reference writes none of these structures to a file, so test_step5_open_model.py
pins this model to hand-made cases whose outcomes are written down as literals; test_gpu_step5_open.py then uses it to judge the HIP
library.

    opening(hbv, inv, paths, read_len) -> ModelOpening       (the fields of step5.Step5Opening, without `ms`)

One thing is the library's and not the reference's: the order of layout entries that tie on pos.  SortSync (GapToyTools2.cc:587) leaves
it unspecified and FindPidsST reads the lists as sets; the library, and this model, order ties by read id, then forward before reverse."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from w2rap_contigger_amd import formats as F

MAX_DEPTH = 15               # Unsat.cc:131
MAX_VERTS = 50               # Unsat.cc:132


@dataclass
class ModelOpening:
    index_off: np.ndarray
    index_read: np.ndarray
    link_off: np.ndarray
    link_to: np.ndarray
    link_pid: np.ndarray
    kind_from: np.ndarray
    kind_to: np.ndarray
    kind_mult: np.ndarray
    layout_off: np.ndarray
    layout_pos: np.ndarray
    layout_id: np.ndarray
    layout_fw: np.ndarray
    counters: dict


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    if lists:
        np.cumsum([len(x) for x in lists], out=off[1:])
    return off


def paths_index(n_edges, path):
    """invert (VecUtilities.h:693): per edge, the sorted ids of the reads whose path holds it, once per occurrence"""
    inv_lists = [[] for _ in range(n_edges)]
    for r, p in enumerate(path):
        for e in p:
            inv_lists[e].append(r)
    for l in inv_lists:
        l.sort()
    return inv_lists


def satisfied(From, v, w):
    """Unsat.cc:161-176 -> "reached", "depth" or "overflow" """
    s = [v]                                                            # :162
    for _d in range(1, MAX_DEPTH + 1):                                 # :163
        s2 = []; sat = False
        for x in s:                                                    # :165
            for y in From[x]:                                          # :167
                if y == w:                                             # :169
                    sat = True
                    break
                s2.append(y)                                           # :172
            if sat:
                break
        if sat:                                                        # :174
            return "reached"
        if len(s2) > MAX_VERTS:                                        # :175
            return "overflow"
        s = s2                                                         # :176
    return "depth"


def unsat_links(hbv: F.HBV, inv, path):
    """Phase 1 of Unsat (:145-207) -> (unsats, mult, counters): unsats[e] = sorted unique [(to, pid)], mult = {(e, to): count}"""
    nv = hbv.n_vertices
    fo = [int(x) for x in hbv.from_off]
    From = [[int(y) for y in hbv.from_v[fo[v]:fo[v + 1]]] for v in range(nv)]
    to_left, to_right = ([int(x) for x in a] for a in hbv.to_left_right())       # :142-143
    c = dict(n_pairs_placed=0, n_meet=0, n_same_vertex=0, n_reached=0, n_unsat_depth=0, n_unsat_overflow=0, n_unsat_same_end=0)
    unsats = [[] for _ in range(hbv.n_edges)]                          # :147
    u = [False] * (len(path) // 2)                                     # :148
    for i in range(0, len(path), 2):                                   # :150
        p1, p2 = path[i], path[i + 1]
        if len(p1) == 0 or len(p2) == 0:                               # :152
            continue
        c["n_pairs_placed"] += 1
        x1 = list(p1)                                                  # :154-155
        x2 = [inv[e] for e in reversed(p2)]                            # :156-157
        if set(x1) & set(x2):                                          # :158 Meet2
            c["n_meet"] += 1
            continue
        v, w = to_right[x1[-1]], to_left[x2[0]]                        # :159
        if v == w:                                                     # :160
            c["n_same_vertex"] += 1
            continue
        how = satisfied(From, v, w)
        if how == "reached":                                           # :177
            c["n_reached"] += 1
            continue
        c["n_unsat_depth" if how == "depth" else "n_unsat_overflow"] += 1
        u[i // 2] = True                                               # :178
    for i in range(0, len(path), 2):                                   # :179
        if not u[i // 2]:
            continue
        p1, p2 = path[i], path[i + 1]
        if p1[-1] == p2[-1]:                                           # :182
            c["n_unsat_same_end"] += 1
            continue
        unsats[p1[-1]].append((inv[p2[-1]], i // 2))                   # :183
        unsats[p2[-1]].append((inv[p1[-1]], i // 2))                   # :184
    mult = {}
    for e in range(len(unsats)):                                       # :191
        unsats[e] = sorted(set(unsats[e]))                             # :187, :192 UniqueSort; :201-207 finds nothing more to delete
        for (to, _pid) in unsats[e]:                                   # :193-198
            mult[(e, to)] = mult.get((e, to), 0) + 1
    return unsats, mult, c


def layout_reads(hbv: F.HBV, inv, path, offset, read_len):
    """LayoutReads (:550-588) -> per edge [(pos, id, fw)], sorted by (pos, id, forward first)"""
    K = hbv.K
    edge_length = [int(x) for x in hbv.edge_len]
    kmers = lambda e: edge_length[e] - K + 1                           # EdgeLengthKmers
    lay = [[] for _ in range(hbv.n_edges)]
    for i, p in enumerate(path):                                       # :556
        x = list(p)
        if not x:                                                      # :560
            continue
        pos = offset[i]                                                # :561
        for j in range(len(x)):                                        # :562
            if 0 < j < len(x) - 1:                                     # :563 -- skipped BEFORE the length comes off
                continue
            lay[x[j]].append((pos, i, True))                           # :564-566
            pos -= kmers(x[j])                                         # :567
        x = [inv[e] for e in reversed(x)]                              # :569-571
        pos = offset[i] + read_len[i]                                  # :572
        ln = edge_length[x[0]]                                         # :573
        for j in range(1, len(x)):                                     # :574-575
            ln += kmers(x[j])
        pos = ln - pos                                                 # :576
        for j in range(len(x)):                                        # :577
            if 0 < j < len(x) - 1:                                     # :578
                continue
            lay[x[j]].append((pos, i, False))                          # :579-581
            pos -= kmers(x[j])                                         # :582
    for l in lay:                                                      # :587 SortSync on pos; ties: the library's rule
        l.sort(key=lambda t: (t[0], t[1], not t[2]))
    return lay


def opening(hbv: F.HBV, inv, paths, read_len) -> ModelOpening:
    inv = [int(x) for x in inv]
    po = [int(x) for x in paths[1]]
    n = len(po) - 1
    path = [[int(e) for e in paths[2][po[r]:po[r + 1]]] for r in range(n)]
    offset = [int(x) for x in paths[0]]
    rl = [int(x) for x in read_len]
    idx = paths_index(hbv.n_edges, path)
    unsats, mult, counters = unsat_links(hbv, inv, path)
    lay = layout_reads(hbv, inv, path, offset, rl)
    kinds = sorted(mult)
    counters.update(n_links=sum(len(x) for x in unsats), n_kinds=len(kinds), n_index=sum(len(x) for x in idx), n_layout=sum(len(x) for x in lay))
    return ModelOpening(
        _csr(idx), np.array([r for l in idx for r in l], np.uint32),
        _csr(unsats), np.array([t for l in unsats for t, _ in l], np.int32), np.array([p for l in unsats for _, p in l], np.uint32),
        np.array([e for e, _ in kinds], np.int32), np.array([t for _, t in kinds], np.int32), np.array([mult[k] for k in kinds], np.uint32),
        _csr(lay), np.array([p for l in lay for p, _, _ in l], np.int32), np.array([i for l in lay for _, i, _ in l], np.uint32),
        np.array([f for l in lay for _, _, f in l], np.uint8), counters)

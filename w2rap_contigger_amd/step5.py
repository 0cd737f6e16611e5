"""ctypes binding of the Step-5 entry points of libw2rap_step2.so (include/w2rap_step5.h).

`partners_to_ends` mirrors ``PartnersToEnds(hbvr, pathsr, bases, quals)``, the last line of the reference's Step 5
(src/modules/w2rap-contigger.cc:448, src/paths/long/large/GapToyTools5.cc:1150-1517): reads without a path whose mate ends near a dead
end of the graph are looked up by their 28-mers against every edge, each hit is checked with a quality-aware window, and a read with
exactly one good (edge, offset) is placed there.  The graph is not edited.

`add_new_stuff` mirrors ``AddNewStuff(new_stuff, hbr, inv2, pathsr, bases, quals, 5, ..., 1)``, the call in front of it
(w2rap-contigger.cc:447, GapToyTools4.cc:133-368): the graph is rebuilt from its edges, its vertex crossings and the patch sequences,
every read path is moved onto the new graph and re-extended over the branches with its bases and qualities.  `finish` is the two calls
one after the other: given new_stuff, what the reference writes as .large_K.final.hbv/.paths.

The rest of Step 5 (the local assemblies, the clustering half of Unsat) and Step 6 stay the reference's (Step 7: step7.py).  The HIP library is the only
implementation (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import formats as F
from .step2 import EdgeHint, Step2Error, _np_from, _ptr, lib as _lib2, make_hint


class Step5In(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_packed", C.c_void_p), ("edge_byte_off", C.c_void_p), ("edge_len", C.c_void_p),
                ("n_vertices", C.c_uint64), ("from_off", C.c_void_p), ("from_v", C.c_void_p), ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_e", C.c_void_p),
                ("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                ("n_reads", C.c_uint64), ("read_packed", C.c_void_p), ("read_byte_off", C.c_void_p), ("read_len", C.c_void_p), ("quals", C.c_void_p), ("qual_off", C.c_void_p)]


class Step5Params(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32)]


OPEN_COUNTERS = ("n_pairs_placed", "n_meet", "n_same_vertex", "n_reached", "n_unsat_depth", "n_unsat_overflow", "n_unsat_same_end",
                 "n_links", "n_kinds", "n_index", "n_layout")
OPEN_PARTS = {"index": 1, "links": 2, "layout": 4}       # W2RAP_STEP5_OPEN_*
OPEN_PHASES = ("ms_index", "ms_links", "ms_layout")
COUNTERS = ("n_interesting", "n_read_kmers", "n_dict_kmers", "n_candidates", "n_good", "n_placed", "n_ambiguous")
PHASES = ("ms_ends", "ms_select", "ms_dict", "ms_edges", "ms_candidates", "ms_verify", "ms_paths")


class Step5Out(C.Structure):
    _fields_ = ([("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p)] +
                [(k, C.c_uint64) for k in COUNTERS] + [(k, C.c_float) for k in PHASES])


class Step5OpenIn(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_len", C.c_void_p), ("n_vertices", C.c_uint64), ("from_off", C.c_void_p), ("from_v", C.c_void_p),
                ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_e", C.c_void_p), ("inv", C.c_void_p),
                ("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p), ("read_len", C.c_void_p)]


_OPEN_ARRAYS = ("index_off", "index_read", "link_off", "link_to", "link_pid", "kind_from", "kind_to", "kind_mult", "layout_off", "layout_pos", "layout_id", "layout_fw")


class Step5OpenOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in _OPEN_ARRAYS] + [(k, C.c_uint64) for k in OPEN_COUNTERS] + [(k, C.c_float) for k in OPEN_PHASES]


ADD_KEEP_MAP = 1                  # W2RAP_STEP5_ADD_KEEP_MAP
ADD_COUNTERS = ("n_all", "n_junctions", "n_all_bases", "n_kmer_instances", "n_kmers_distinct", "n_unipaths", "n_tr_empty", "n_tr_first", "n_tr_walked",
                "n_tr_cleared", "n_ext_tried", "n_ext_too_many", "n_ext_no_cover", "n_ext_ambiguous", "n_ext_extended")
ADD_PHASES = ("ms_all", "ms_dict", "ms_graph", "ms_translate", "ms_extend")


class Step5AddParams(C.Structure):
    _fields_ = [("device", C.c_int32), ("min_gain", C.c_int32), ("ext_mode", C.c_int32), ("edge_order_hint", C.POINTER(EdgeHint)), ("flags", C.c_uint32)]


class Step5AddOut(C.Structure):
    _fields_ = ([("K", C.c_int32), ("n_vertices", C.c_uint64), ("n_edge_objs", C.c_uint64)] +
                [(k, C.c_void_p) for k in ("edge_packed", "edge_byte_off", "edge_len", "vleft", "vright", "from_off", "from_v", "from_e", "to_off", "to_v", "to_e", "inv2")] +
                [("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                 ("n_old_edge_objs", C.c_uint64), ("to3_off", C.c_void_p), ("to3", C.c_void_p), ("left3", C.c_void_p)] +
                [(k, C.c_uint64) for k in ADD_COUNTERS] + [(k, C.c_float) for k in ADD_PHASES])


_ready = False


def lib():
    global _ready
    L = _lib2()
    if not _ready:
        L.w2rap_step5_partners_to_ends.argtypes = [C.POINTER(Step5In), C.POINTER(Step5Params), C.POINTER(Step5Out), C.c_char_p, C.c_size_t]
        L.w2rap_step5_free.argtypes = [C.POINTER(Step5Out)]
        L.w2rap_step5_free.restype = None
        L.w2rap_step5_open.argtypes = [C.POINTER(Step5OpenIn), C.POINTER(Step5Params), C.POINTER(Step5OpenOut), C.c_char_p, C.c_size_t]
        L.w2rap_step5_open_free.argtypes = [C.POINTER(Step5OpenOut)]
        L.w2rap_step5_open_free.restype = None
        L.w2rap_step5_add_new_stuff.argtypes = [C.POINTER(Step5In), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Step5AddParams), C.POINTER(Step5AddOut),
                                                C.c_char_p, C.c_size_t]
        L.w2rap_step5_add_free.argtypes = [C.POINTER(Step5AddOut)]
        L.w2rap_step5_add_free.restype = None
        L.w2rap_step5_profile.argtypes = [C.c_char_p, C.c_size_t]
        L.w2rap_step5_profile.restype = C.c_size_t
        _ready = True
    return L


@dataclass
class Step5Result:
    path_offset: np.ndarray       # ALL read paths; untouched reads keep theirs
    path_off: np.ndarray
    path_edges: np.ndarray
    counters: dict                # COUNTERS -> int
    ms: dict                      # PHASES -> device milliseconds


def _step5_in(hbv, paths, reads, quals, qual_off):
    """-> (Step5In, the arrays it points into)"""
    ln = np.ascontiguousarray(reads[2], np.uint32)
    if qual_off is None:
        qual_off = np.zeros(len(ln) + 1, np.uint64)
        np.cumsum(ln, out=qual_off[1:])
    keep = [np.ascontiguousarray(hbv.edge_packed, np.uint8), np.ascontiguousarray(hbv.edge_byte_off, np.uint64), np.ascontiguousarray(hbv.edge_len, np.uint32),
            np.ascontiguousarray(hbv.from_off, np.uint64), np.ascontiguousarray(hbv.from_v, np.int32), np.ascontiguousarray(hbv.from_e, np.int32),
            np.ascontiguousarray(hbv.to_off, np.uint64), np.ascontiguousarray(hbv.to_e, np.int32),
            np.ascontiguousarray(paths[0], np.int32), np.ascontiguousarray(paths[1], np.uint64), np.ascontiguousarray(paths[2], np.int32),
            np.ascontiguousarray(reads[0], np.uint8), np.ascontiguousarray(reads[1], np.uint64), ln,
            np.ascontiguousarray(quals, np.uint8), np.ascontiguousarray(qual_off, np.uint64)]
    p = lambda a: _ptr(a) if len(a) else None
    i = Step5In(hbv.K, len(keep[2]), p(keep[0]), p(keep[1]), p(keep[2]), hbv.n_vertices, p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]),
                len(keep[8]), p(keep[8]), p(keep[9]), p(keep[10]), len(ln), p(keep[11]), p(keep[12]), p(keep[13]), p(keep[14]), p(keep[15]))
    return i, keep


def partners_to_ends(hbv: F.HBV, paths, reads, quals, device=0, qual_off=None) -> Step5Result:
    """PartnersToEnds through the C entry point (w2rap_step5_partners_to_ends).
    paths = (offset i32[n], path_off u64[n+1], edges i32[]); reads = (packed, byte_off, read_len) as formats.read_fastb gives them;
    quals = the unpacked .qualp values, one byte per base (formats.qualp_to_raw); qual_off None = the running sum of read_len."""
    L = lib()
    i, keep = _step5_in(hbv, paths, reads, quals, qual_off)
    prm = Step5Params(device, 0)
    o = Step5Out()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step5_partners_to_ends(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    try:
        po = _np_from(o.path_off, np.uint64, o.n_paths + 1)
        return Step5Result(_np_from(o.path_offset, np.int32, o.n_paths), po, _np_from(o.path_edges, np.int32, int(po[-1])),
                           {k: int(getattr(o, k)) for k in COUNTERS}, {k: float(getattr(o, k)) for k in PHASES})
    finally:
        L.w2rap_step5_free(C.byref(o))


@dataclass
class Step5Added:
    hbv: F.HBV                    # the new graph
    vleft: np.ndarray
    vright: np.ndarray
    to_v: np.ndarray
    inv: np.ndarray               # its involution
    path_offset: np.ndarray       # ALL read paths on the new graph
    path_off: np.ndarray
    path_edges: np.ndarray
    counters: dict                # ADD_COUNTERS -> int
    ms: dict                      # ADD_PHASES -> device milliseconds
    to3: tuple = None             # keep_map: (off u64[E_old+1], edges i32[]) -- the path of every old edge object through the new graph
    left3: np.ndarray = None      # keep_map: i32[E_old] its first skip


def add_new_stuff(hbv: F.HBV, paths, reads, quals, new_stuff, min_gain=5, ext_mode=1, hint=None, keep_map=False, device=0, qual_off=None) -> Step5Added:
    """AddNewStuff through the C entry point (w2rap_step5_add_new_stuff).  hbv, paths, reads, quals as for partners_to_ends;
    new_stuff = (packed, byte_off, len) in the packing of the edges (formats.pack_bases), any lengths, possibly none;
    hint = (packed, byte_off, len) of the new graph's canonical edges in the order to replay, or None for the lexicographic order."""
    L = lib()
    i, keep = _step5_in(hbv, paths, reads, quals, qual_off)
    npk = np.ascontiguousarray(new_stuff[0], np.uint8); nbo = np.ascontiguousarray(new_stuff[1], np.uint64); nln = np.ascontiguousarray(new_stuff[2], np.uint32)
    if len(nbo) != len(nln) + 1:
        raise ValueError("new_stuff: byte_off must have one entry more than len")
    hint_p = None
    if hint is not None:
        eh, k2 = make_hint(*hint)
        keep.append(k2)
        hint_p = C.pointer(eh)
    prm = Step5AddParams(device, min_gain, ext_mode, hint_p, ADD_KEEP_MAP if keep_map else 0)
    o = Step5AddOut()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step5_add_new_stuff(C.byref(i), len(nln), _ptr(npk) if len(npk) else None, _ptr(nbo), _ptr(nln) if len(nln) else None, C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    try:
        NO, NV, NP = o.n_edge_objs, o.n_vertices, o.n_paths
        boff = _np_from(o.edge_byte_off, np.uint64, NO + 1)
        h2 = F.HBV(o.K, _np_from(o.from_off, np.uint64, NV + 1), _np_from(o.from_v, np.int32, NO), _np_from(o.from_e, np.int32, NO),
                   _np_from(o.to_off, np.uint64, NV + 1), _np_from(o.to_e, np.int32, NO), _np_from(o.edge_packed, np.uint8, int(boff[-1])), boff,
                   _np_from(o.edge_len, np.uint32, NO))
        po = _np_from(o.path_off, np.uint64, NP + 1)
        res = Step5Added(h2, _np_from(o.vleft, np.int32, NO), _np_from(o.vright, np.int32, NO), _np_from(o.to_v, np.int32, NO), _np_from(o.inv2, np.int32, NO),
                         _np_from(o.path_offset, np.int32, NP), po, _np_from(o.path_edges, np.int32, int(po[-1])),
                         {k: int(getattr(o, k)) for k in ADD_COUNTERS}, {k: float(getattr(o, k)) for k in ADD_PHASES})
        if keep_map:
            t3o = _np_from(o.to3_off, np.uint64, o.n_old_edge_objs + 1)
            res.to3 = (t3o, _np_from(o.to3, np.int32, int(t3o[-1])))
            res.left3 = _np_from(o.left3, np.int32, o.n_old_edge_objs)
        return res
    finally:
        L.w2rap_step5_add_free(C.byref(o))


@dataclass
class Step5Finished:
    added: Step5Added             # the graph (added.hbv, added.inv) and everything AddNewStuff reports
    placed: Step5Result           # PartnersToEnds on it: the final read paths and its counters


def finish(hbv: F.HBV, paths, reads, quals, new_stuff, min_gain=5, ext_mode=1, hint=None, keep_map=False, device=0, qual_off=None) -> Step5Finished:
    """add_new_stuff, then partners_to_ends on its result: given new_stuff, the graph and the paths the reference writes as
    .large_K.final.hbv/.paths (w2rap-contigger.cc:447-452)."""
    a = add_new_stuff(hbv, paths, reads, quals, new_stuff, min_gain, ext_mode, hint, keep_map, device, qual_off)
    p = partners_to_ends(a.hbv, (a.path_offset, a.path_off, a.path_edges), reads, quals, device, qual_off)
    return Step5Finished(a, p)


@dataclass
class Step5Opening:
    """the three CSRs over the edge objects (include/w2rap_step5.h); the arrays of a part that was not asked for are None"""
    index_off: np.ndarray         # u64[E+1]
    index_read: np.ndarray        # u32: read ids, ascending per edge
    link_off: np.ndarray          # u64[E+1]
    link_to: np.ndarray           # i32, ordered by (link_to, pid) per edge
    link_pid: np.ndarray          # u32
    kind_from: np.ndarray         # i32[n_kinds]: the distinct (edge, link_to), in order ...
    kind_to: np.ndarray
    kind_mult: np.ndarray         # u32: ... and how many links each has
    layout_off: np.ndarray        # u64[E+1]
    layout_pos: np.ndarray        # i32, ascending (signed) per edge; ties by read id, then forward first
    layout_id: np.ndarray         # u32
    layout_fw: np.ndarray         # u8, 1 = forward
    counters: dict                # OPEN_COUNTERS -> int
    ms: dict                      # OPEN_PHASES -> device milliseconds


def opening(hbv: F.HBV, inv, paths, read_len, parts=("index", "links", "layout"), device=0) -> Step5Opening:
    """The read-sized passes at the front of Step 5 through the C entry point (w2rap_step5_open): the paths index (invert), the links
    and multiplicities of Unsat's phase 1, and LayoutReads.  paths = (offset i32[n], path_off u64[n+1], edges i32[]); inv = the graph's
    involution; read_len u32[n].  parts: any of "index", "links", "layout"."""
    L = lib()
    flags = 0
    for p in parts:
        if p not in OPEN_PARTS:
            raise ValueError(f"unknown part {p!r}: one of {sorted(OPEN_PARTS)}")
        flags |= OPEN_PARTS[p]
    if not flags:
        raise ValueError("no part asked for")
    keep = [np.ascontiguousarray(hbv.edge_len, np.uint32), np.ascontiguousarray(hbv.from_off, np.uint64), np.ascontiguousarray(hbv.from_v, np.int32),
            np.ascontiguousarray(hbv.from_e, np.int32), np.ascontiguousarray(hbv.to_off, np.uint64), np.ascontiguousarray(hbv.to_e, np.int32),
            np.ascontiguousarray(inv, np.int32), np.ascontiguousarray(paths[0], np.int32), np.ascontiguousarray(paths[1], np.uint64),
            np.ascontiguousarray(paths[2], np.int32), np.ascontiguousarray(read_len, np.uint32)]
    if len(keep[6]) != len(keep[0]):
        raise ValueError("inv must have one entry per edge object")
    if len(keep[8]) != len(keep[7]) + 1 or len(keep[10]) != len(keep[7]):
        raise ValueError("path_off must have n + 1 entries and read_len n, n = len(path_offset)")
    p = lambda a: _ptr(a) if len(a) else None
    i = Step5OpenIn(hbv.K, len(keep[0]), p(keep[0]), hbv.n_vertices, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]),
                    len(keep[7]), p(keep[7]), p(keep[8]), p(keep[9]), p(keep[10]))
    prm = Step5Params(device, flags)
    o = Step5OpenOut()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step5_open(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    try:
        E = len(keep[0])
        size = {"index_off": E + 1, "index_read": o.n_index, "link_off": E + 1, "link_to": o.n_links, "link_pid": o.n_links, "kind_from": o.n_kinds,
                "kind_to": o.n_kinds, "kind_mult": o.n_kinds, "layout_off": E + 1, "layout_pos": o.n_layout, "layout_id": o.n_layout, "layout_fw": o.n_layout}
        dtype = {"index_off": np.uint64, "index_read": np.uint32, "link_off": np.uint64, "link_to": np.int32, "link_pid": np.uint32, "kind_from": np.int32,
                 "kind_to": np.int32, "kind_mult": np.uint32, "layout_off": np.uint64, "layout_pos": np.int32, "layout_id": np.uint32, "layout_fw": np.uint8}
        arrays = {k: (_np_from(getattr(o, k), dtype[k], int(size[k])) if getattr(o, k) else None) for k in _OPEN_ARRAYS}
        return Step5Opening(**arrays, counters={k: int(getattr(o, k)) for k in OPEN_COUNTERS}, ms={k: float(getattr(o, k)) for k in OPEN_PHASES})
    finally:
        L.w2rap_step5_open_free(C.byref(o))


def profile():
    """-> {kernel name: (total ms, launches)} of the last partners_to_ends, opening or add_new_stuff in this process"""
    L = lib()
    n = L.w2rap_step5_profile(None, 0)
    buf = C.create_string_buffer(int(n) + 16)
    L.w2rap_step5_profile(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, k = line.rsplit(" ", 2)
        out[name] = (float(ms), int(k))
    return out

"""ctypes binding of the Step-5 entry points of libw2rap_step2.so (include/w2rap_step5.h).

`partners_to_ends` mirrors ``PartnersToEnds(hbvr, pathsr, bases, quals)``, the last line of the reference's Step 5
(src/modules/w2rap-contigger.cc:448, src/paths/long/large/GapToyTools5.cc:1150-1517): reads without a path whose mate ends near a dead
end of the graph are looked up by their 28-mers against every edge, each hit is checked with a quality-aware window, and a read with
exactly one good (edge, offset) is placed there.  The graph is not edited.  The rest of Step 5 (local assemblies, AddNewStuff, Unsat)
and Steps 6-7 stay the reference's.  The HIP library is the only implementation (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import formats as F
from .step2 import Step2Error, _np_from, _ptr, lib as _lib2


class Step5In(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_packed", C.c_void_p), ("edge_byte_off", C.c_void_p), ("edge_len", C.c_void_p),
                ("n_vertices", C.c_uint64), ("from_off", C.c_void_p), ("from_v", C.c_void_p), ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_e", C.c_void_p),
                ("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                ("n_reads", C.c_uint64), ("read_packed", C.c_void_p), ("read_byte_off", C.c_void_p), ("read_len", C.c_void_p), ("quals", C.c_void_p), ("qual_off", C.c_void_p)]


class Step5Params(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32)]


COUNTERS = ("n_interesting", "n_read_kmers", "n_dict_kmers", "n_candidates", "n_good", "n_placed", "n_ambiguous")
PHASES = ("ms_ends", "ms_select", "ms_dict", "ms_edges", "ms_candidates", "ms_verify", "ms_paths")


class Step5Out(C.Structure):
    _fields_ = ([("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p)] +
                [(k, C.c_uint64) for k in COUNTERS] + [(k, C.c_float) for k in PHASES])


_ready = False


def lib():
    global _ready
    L = _lib2()
    if not _ready:
        L.w2rap_step5_partners_to_ends.argtypes = [C.POINTER(Step5In), C.POINTER(Step5Params), C.POINTER(Step5Out), C.c_char_p, C.c_size_t]
        L.w2rap_step5_free.argtypes = [C.POINTER(Step5Out)]
        L.w2rap_step5_free.restype = None
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


def partners_to_ends(hbv: F.HBV, paths, reads, quals, device=0, qual_off=None) -> Step5Result:
    """PartnersToEnds through the C entry point (w2rap_step5_partners_to_ends).
    paths = (offset i32[n], path_off u64[n+1], edges i32[]); reads = (packed, byte_off, read_len) as formats.read_fastb gives them;
    quals = the unpacked .qualp values, one byte per base (formats.qualp_to_raw); qual_off None = the running sum of read_len."""
    L = lib()
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


def profile():
    """-> {kernel name: (total ms, launches)} of the last partners_to_ends in this process"""
    L = lib()
    n = L.w2rap_step5_profile(None, 0)
    buf = C.create_string_buffer(int(n) + 16)
    L.w2rap_step5_profile(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, k = line.rsplit(" ", 2)
        out[name] = (float(ms), int(k))
    return out

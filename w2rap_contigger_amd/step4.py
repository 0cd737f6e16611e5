"""ctypes binding of the Step-4 entry points of libw2rap_step2.so (include/w2rap_step4.h) + the host-side mirror of the
reference's Step-4 interface.

`clean200x` mirrors ``hbvr.Involution(inv); Clean200x(hbvr, inv, pathsr, bases, quals, 0, 3, min_size)``
(src/modules/w2rap-contigger.cc:395-399, src/paths/long/large/Clean200.cc:202-389); `run_step4_files` mirrors the reference's
``--from_step 4 --to_step 4`` run on an output directory (w2rap-contigger.cc:386-409): reads <prefix>.large_K.{hbv,paths} and
frag_reads_orig.{fastb,qualp}, writes <prefix>.large_K.clean.{hbv,paths}.

The vote over the reads, the rewrite of the read paths and the edit of the graph itself (delete, merge runs, renumber: the k4e_*
kernels) run in HIP kernels: the graph goes up once and comes down once.  ``edit="host"`` (EDIT_ON_HOST) runs the library's host edit
instead, the cross-check; a graph that misses a precondition of the device edit (adjacency lists not sorted by neighbour, a run whose
mirror image is not a run) takes it silently, with the same result.  `Step4Result.edit_on_device` tells which one ran.  An `inv` that
pairs a merged run's ends with edges no run joins (the reference would walk off the graph) raises Step2Error, W2RAP_E_GRAPH.

`clean200x_after_step3` is the same step straight behind Step 3 on one `step2.Step2Context` (w2rap_step2_run_step4_after_step3): the reads and
their qualities are the context's, the large-K graph and paths are what `step3.repath_after_step2(ctx, keep_on_device=True)` left in
HBM.  Nothing is uploaded.  The HIP library is the only implementation (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import formats as F
from .step2 import Step2Error, _np_from, _ptr, lib as _lib2


class Step4In(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_packed", C.c_void_p), ("edge_byte_off", C.c_void_p), ("edge_len", C.c_void_p),
                ("n_vertices", C.c_uint64), ("from_off", C.c_void_p), ("from_v", C.c_void_p), ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_e", C.c_void_p),
                ("inv", C.c_void_p),
                ("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                ("n_reads", C.c_uint64), ("read_packed", C.c_void_p), ("read_byte_off", C.c_void_p), ("read_len", C.c_void_p), ("quals", C.c_void_p), ("qual_off", C.c_void_p)]


class Step4Params(C.Structure):
    _fields_ = [("device", C.c_int32), ("min_size", C.c_uint32), ("flags", C.c_uint32)]


VOTE_ONLY = 1
EDIT_ON_HOST = 2


class Step4Out(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_vertices", C.c_uint64), ("n_edge_objs", C.c_uint64),
                ("edge_packed", C.c_void_p), ("edge_byte_off", C.c_void_p), ("edge_len", C.c_void_p), ("vleft", C.c_void_p), ("vright", C.c_void_p),
                ("from_off", C.c_void_p), ("from_v", C.c_void_p), ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_v", C.c_void_p), ("to_e", C.c_void_p),
                ("inv", C.c_void_p),
                ("n_paths", C.c_uint64), ("path_offset", C.c_void_p), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                ("n_deleted", C.c_uint64 * 2), ("deleted", C.c_void_p * 2), ("n_runs_merged", C.c_uint64 * 2),
                ("n_branch_vertices", C.c_uint64), ("n_skipped_too_many_exts", C.c_uint64), ("n_placements", C.c_uint64),
                ("ms_index", C.c_float * 2), ("ms_vote", C.c_float * 2), ("ms_paths", C.c_float * 2), ("ms_graph_edit_host", C.c_float * 2),
                ("_owner", C.c_void_p)]


_ready = False


def lib():
    global _ready
    L = _lib2()
    if not _ready:
        L.w2rap_step4_run.argtypes = [C.POINTER(Step4In), C.POINTER(Step4Params), C.POINTER(Step4Out), C.c_char_p, C.c_size_t]
        L.w2rap_step2_run_step4_after_step3.argtypes = [C.c_void_p, C.POINTER(Step4Params), C.POINTER(Step4Out), C.c_char_p, C.c_size_t]
        L.w2rap_step4_free.argtypes = [C.POINTER(Step4Out)]
        L.w2rap_step4_free.restype = None
        L.w2rap_step4_profile.argtypes = [C.c_char_p, C.c_size_t]
        L.w2rap_step4_profile.restype = C.c_size_t
        _ready = True
    return L


@dataclass
class Step4Result:
    hbv: F.HBV                    # the clean graph
    vleft: np.ndarray
    vright: np.ndarray
    to_v: np.ndarray
    inv: np.ndarray               # its involution
    path_offset: np.ndarray
    path_off: np.ndarray
    path_edges: np.ndarray
    deleted: list                 # per pass: sorted unique edge ids of that pass's input graph (vote_only: pass 1 only)
    n_deleted: tuple
    n_runs_merged: tuple
    n_branch_vertices: int
    n_skipped_too_many_exts: int
    n_placements: int
    ms_index: tuple               # device milliseconds per pass
    ms_vote: tuple
    ms_paths: tuple
    ms_graph_edit_host: tuple     # HOST milliseconds per pass
    edit_on_device: bool = False  # the graph edit ran in the k4e_* kernels (False: the host edit ran, or vote_only edited nothing)


def clean200x(hbv: F.HBV, paths, read_packed, read_byte_off, read_len, quals, qual_off=None, min_size=0, device=0, vote_only=False, inv=None,
              edit="device") -> Step4Result:
    """Involution + Clean200x through the one-shot C entry point (w2rap_step4_run).
    paths = (offset i32[n], path_off u64[n+1], edges i32[]); quals = the unpacked .qualp values, one byte per base (formats.qualp_to_raw);
    qual_off None = the running sum of read_len; inv = the graph's involution if the caller has it (Step 3's inv2), else computed;
    edit = "device" (the default) or "host": where the graph edit runs."""
    if edit not in ("device", "host"):
        raise ValueError(f"edit must be 'device' or 'host', not {edit!r}")
    L = lib()
    ln = np.ascontiguousarray(read_len, np.uint32)
    if qual_off is None:
        qual_off = np.zeros(len(ln) + 1, np.uint64)
        np.cumsum(ln, out=qual_off[1:])
    keep = [np.ascontiguousarray(hbv.edge_packed, np.uint8), np.ascontiguousarray(hbv.edge_byte_off, np.uint64), np.ascontiguousarray(hbv.edge_len, np.uint32),
            np.ascontiguousarray(hbv.from_off, np.uint64), np.ascontiguousarray(hbv.from_v, np.int32), np.ascontiguousarray(hbv.from_e, np.int32),
            np.ascontiguousarray(hbv.to_off, np.uint64), np.ascontiguousarray(hbv.to_e, np.int32),
            np.ascontiguousarray(paths[0], np.int32), np.ascontiguousarray(paths[1], np.uint64), np.ascontiguousarray(paths[2], np.int32),
            np.ascontiguousarray(read_packed, np.uint8), np.ascontiguousarray(read_byte_off, np.uint64), ln,
            np.ascontiguousarray(quals, np.uint8), np.ascontiguousarray(qual_off, np.uint64)]
    p = lambda a: _ptr(a) if len(a) else None
    inv_a = None if inv is None else np.ascontiguousarray(inv, np.int32)
    i = Step4In(hbv.K, len(keep[2]), p(keep[0]), p(keep[1]), p(keep[2]), hbv.n_vertices, p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]),
                None if inv_a is None or not len(inv_a) else _ptr(inv_a),
                len(keep[8]), p(keep[8]), p(keep[9]), p(keep[10]), len(ln), p(keep[11]), p(keep[12]), p(keep[13]), p(keep[14]), p(keep[15]))
    prm = Step4Params(device, int(min_size), (VOTE_ONLY if vote_only else 0) | (EDIT_ON_HOST if edit == "host" else 0))
    o = Step4Out()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step4_run(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    return _result4(L, o, vote_only)


def clean200x_after_step3(ctx, min_size=0, vote_only=False, edit="device") -> Step4Result:
    """Involution + Clean200x straight behind Step 3 on the same GPU context (w2rap_step2_run_step4_after_step3): `ctx` is a step2.Step2Context
    whose last Step 3 was step3.repath_after_step2(ctx, ..., keep_on_device=True).  A full run consumes the kept large-K result (a second
    call raises Step2Error, W2RAP_E_STATE); vote_only leaves it in place.  The context's Step-2 state is untouched."""
    if edit not in ("device", "host"):
        raise ValueError(f"edit must be 'device' or 'host', not {edit!r}")
    L = lib()
    prm = Step4Params(ctx.device, int(min_size), (VOTE_ONLY if vote_only else 0) | (EDIT_ON_HOST if edit == "host" else 0))
    o = Step4Out()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step2_run_step4_after_step3(ctx.h, C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    return _result4(L, o, vote_only)


def _result4(L, o, vote_only) -> Step4Result:
    try:
        NO, NV, NP = o.n_edge_objs, o.n_vertices, o.n_paths
        boff = _np_from(o.edge_byte_off, np.uint64, NO + 1)
        h2 = F.HBV(o.K, _np_from(o.from_off, np.uint64, NV + 1), _np_from(o.from_v, np.int32, NO), _np_from(o.from_e, np.int32, NO),
                   _np_from(o.to_off, np.uint64, NV + 1), _np_from(o.to_e, np.int32, NO),
                   _np_from(o.edge_packed, np.uint8, int(boff[-1])), boff, _np_from(o.edge_len, np.uint32, NO))
        po = _np_from(o.path_off, np.uint64, NP + 1)
        return Step4Result(h2, _np_from(o.vleft, np.int32, NO), _np_from(o.vright, np.int32, NO), _np_from(o.to_v, np.int32, NO), _np_from(o.inv, np.int32, NO),
                           _np_from(o.path_offset, np.int32, NP), po, _np_from(o.path_edges, np.int32, int(po[-1])),
                           [_np_from(o.deleted[k], np.int32, o.n_deleted[k]) for k in range(1 if vote_only else 2)],
                           tuple(o.n_deleted), tuple(o.n_runs_merged), o.n_branch_vertices, o.n_skipped_too_many_exts, o.n_placements,
                           tuple(o.ms_index), tuple(o.ms_vote), tuple(o.ms_paths), tuple(o.ms_graph_edit_host),
                           edit_on_device=profile().get("edit_path_device", (0.0, 0))[0] == 1.0)
    finally:
        L.w2rap_step4_free(C.byref(o))


def profile():
    """-> {kernel name: (total ms, launches)} of the last clean200x in this process; the entry "edit_path_device" is not a kernel:
    (1.0, passes edited on the device) or (0.0, 0)"""
    L = lib()
    n = L.w2rap_step4_profile(None, 0)
    buf = C.create_string_buffer(int(n) + 16)
    L.w2rap_step4_profile(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, k = line.rsplit(" ", 2)
        out[name] = (float(ms), int(k))
    return out


def run_step4_files(out_dir, prefix, min_size=0, device=0, edit="device") -> Step4Result:
    """The reference's Step 4 on an output directory (w2rap-contigger.cc:386-409)."""
    if edit not in ("device", "host"):
        raise ValueError(f"edit must be 'device' or 'host', not {edit!r}")
    hbv = F.read_hbv(os.path.join(out_dir, f"{prefix}.large_K.hbv"))
    paths = F.read_paths(os.path.join(out_dir, f"{prefix}.large_K.paths"))
    pk, bo, ln = F.read_fastb(os.path.join(out_dir, "frag_reads_orig.fastb"))
    pq, po = F.read_qualp(os.path.join(out_dir, "frag_reads_orig.qualp"))
    quals, qoff = F.qualp_to_raw(pq, po)
    res = clean200x(hbv, paths, pk, bo, ln, quals, qoff, min_size=min_size, device=device, edit=edit)
    F.write_hbv(os.path.join(out_dir, f"{prefix}.large_K.clean.hbv"), res.hbv)
    F.write_paths(os.path.join(out_dir, f"{prefix}.large_K.clean.paths"), res.path_offset, res.path_off, res.path_edges)
    return res

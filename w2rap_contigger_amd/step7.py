"""ctypes binding of the Step-7 entry point of libw2rap_step2.so (include/w2rap_step7.h), and a small command line.

`line_stats` is GetTol, GetLineLengths and GetLineNpairs (src/paths/long/large/Lines.cc:329-355, Lines.h:74-117): the line of every
edge, the length of every line in K-mers and the number of read pairs that touch it -- what the reference writes as .fin.lines.npairs.

`find_gaps` is MakeGaps (src/paths/long/large/MakeGaps.cc:25-427) up to its list of accepted gaps: the edge groups, the nears of every
read pair, the links that the bounded search does not find close, the per-link filters and the set rules.  The graph edit behind that
list, GAP_CLEANUP, FinalFiles and FindLines stay the reference's; the lines come in as data (formats.read_lines).

`line_files` is DumpLineFiles (Lines.cc:680-798): the texts of a.lines.fasta, a.lines.efasta and a.lines.src; `sort_lines` is SortLines
(Lines.cc:664-678) and `stats_text` the `stats` file of FinalFiles (FinalFiles.cc:73-104), both from the llens of `line_stats`.

``python -m w2rap_contigger_amd.step7 DIR PREFIX`` reads DIR/PREFIX.contig.hbv, .contig.paths, .fin.lines and .fin.lines.npairs and
writes the accepted gaps as text; with ``--line_files LINES_FILE`` it reads DIR/PREFIX.contig.hbv/.paths and that lines file and writes
a.lines.fasta, a.lines.efasta, a.lines.src and stats into DIR; with ``--coverage LINES_FILE`` it writes DIR/PREFIX_assembly.covs,
.lines.npairs and .lines.stats and prints the `CN fraction good` line of Step 6.  The HIP library is the only implementation (no CPU
fallback).

`coverage` is ComputeCoverage (Lines.cc:442-624) with CNIntegerFraction (GapToyTools5.cc:1520-1538): the copy number of every edge;
`line_stats_text` is WriteLineStats (Lines.cc:357-379)."""
from __future__ import annotations

import ctypes as C
import sys
from dataclasses import dataclass

import numpy as np

from . import formats as F
from .step2 import Step2Error, _np_from, _ptr, lib as _lib2

PARTS = {"lines": 1, "links": 2}            # W2RAP_STEP7_*
PAIR_LINES = 16                             # W2RAP_STEP7_PAIR_LINES
NEAR_LIST = 16                              # W2RAP_STEP7_NEAR_LIST
REASONS = ("accepted", "count", "line", "coverage", "alt", "left_end", "right_end")      # W2RAP_STEP7_R_*


class Step7In(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_len", C.c_void_p), ("n_vertices", C.c_uint64), ("from_off", C.c_void_p), ("from_v", C.c_void_p),
                ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_e", C.c_void_p), ("inv", C.c_void_p),
                ("n_paths", C.c_uint64), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                ("n_lines", C.c_uint64), ("line_off", C.c_void_p), ("cell_off", C.c_void_p), ("lpath_off", C.c_void_p), ("line_edges", C.c_void_p),
                ("n_npairs", C.c_uint64), ("npairs", C.c_void_p)]


class Step7Params(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("min_line", C.c_int32), ("min_link_count", C.c_int32)]


# name -> (dtype, the counter or size that gives its length)
ARRAYS = {"tol": (np.int32, "E"), "llens": (np.int32, "NL"), "npairs": (np.int32, "NL"),
          "tom": (np.int32, "E"), "sink_like": (np.uint8, "E"), "source_like": (np.uint8, "E"), "dist_to_end": (np.int32, "E"),
          "near_max1": (np.int32, "E"), "near_max2": (np.int32, "E"),
          "link_from": (np.int32, "n_links"), "link_to": (np.int32, "n_links"), "link_count": (np.int32, "n_links"), "link_reason": (np.uint8, "n_links"),
          "gap_from": (np.int32, "n_gaps"), "gap_to": (np.int32, "n_gaps"), "gap_inv": (np.int32, "n_gaps")}
LINES_COUNTERS = ("n_pairs", "n_pairs_listed", "n_pairs_spilled", "n_pairs_no_path", "n_line_hits")
LINKS_COUNTERS = ("n_group_sink", "n_group_source", "n_group_loop1", "n_group_loop2", "n_pass_placed", "n_pass_y_long", "n_pass_none", "n_nears", "n_near_kinds",
                  "n_pred_start", "n_close", "n_links", "n_reason", "n_not_one_to_one", "n_advanced", "n_unique", "n_sym_deleted", "n_sym_added", "n_overlinked", "n_gaps")
PHASES = ("ms_lines", "ms_nears", "ms_search", "ms_filter")
_CTYPE = {"n_close": C.c_uint64 * 4, "n_reason": C.c_uint64 * 7, "n_sym_added": C.c_int64}


class Step7Out(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ARRAYS] + [(k, _CTYPE.get(k, C.c_uint64)) for k in LINES_COUNTERS + LINKS_COUNTERS] + [(k, C.c_float) for k in PHASES])


_ready = False


def lib():
    global _ready
    L = _lib2()
    if not _ready:
        L.w2rap_step7_links.argtypes = [C.POINTER(Step7In), C.POINTER(Step7Params), C.POINTER(Step7Out), C.c_char_p, C.c_size_t]
        L.w2rap_step7_free.argtypes = [C.POINTER(Step7Out)]
        L.w2rap_step7_free.restype = None
        L.w2rap_step7_profile.argtypes = [C.c_char_p, C.c_size_t]
        L.w2rap_step7_profile.restype = C.c_size_t
        L.w2rap_step7_line_files.argtypes = [C.POINTER(FastaIn), C.POINTER(FastaParams), C.POINTER(FastaOut), C.c_char_p, C.c_size_t]
        L.w2rap_step7_line_files_free.argtypes = [C.POINTER(FastaOut)]
        L.w2rap_step7_line_files_free.restype = None
        L.w2rap_step7_line_files_profile.argtypes = [C.c_char_p, C.c_size_t]
        L.w2rap_step7_line_files_profile.restype = C.c_size_t
        L.w2rap_step7_coverage.argtypes = [C.POINTER(CovIn), C.POINTER(CovParams), C.POINTER(CovOut), C.c_char_p, C.c_size_t]
        L.w2rap_step7_coverage_free.argtypes = [C.POINTER(CovOut)]
        L.w2rap_step7_coverage_free.restype = None
        _ready = True
    return L


@dataclass
class Step7Result:
    """the arrays of include/w2rap_step7.h by name (None: the part was not asked for), the counters and the device times"""
    arrays: dict
    counters: dict
    ms: dict

    def __getattr__(self, k):
        try:
            return self.__dict__["arrays"][k]
        except KeyError:
            raise AttributeError(k)

    def gaps(self):
        return list(zip(self.arrays["gap_from"].tolist(), self.arrays["gap_to"].tolist()))


def run(hbv: F.HBV, inv, paths, lines: F.Lines, parts=("lines", "links"), npairs=None, min_line=5000, min_link_count=3, device=0, flags=None) -> Step7Result:
    """w2rap_step7_links.  paths = (offset, path_off u64[n+1], edges i32[]) as formats.read_paths gives them (the offsets are not read);
    inv = the graph's involution; lines = formats.Lines; npairs = the .fin.lines.npairs values for LINKS without LINES (None: LINKS reads
    what LINES of the same call counts).  flags overrides parts (the tests of the argument checks)."""
    L = lib()
    if flags is None:
        flags = 0
        for p in parts:
            if p not in PARTS:
                raise ValueError(f"unknown part {p!r}: one of {sorted(PARTS)}")
            flags |= PARTS[p]
        if not flags:
            raise ValueError("no part asked for")
    keep = [np.ascontiguousarray(hbv.edge_len, np.uint32), np.ascontiguousarray(hbv.from_off, np.uint64), np.ascontiguousarray(hbv.from_v, np.int32),
            np.ascontiguousarray(hbv.from_e, np.int32), np.ascontiguousarray(hbv.to_off, np.uint64), np.ascontiguousarray(hbv.to_e, np.int32),
            np.ascontiguousarray(inv, np.int32), np.ascontiguousarray(paths[1], np.uint64), np.ascontiguousarray(paths[2], np.int32),
            np.ascontiguousarray(lines.line_off, np.uint64), np.ascontiguousarray(lines.cell_off, np.uint64), np.ascontiguousarray(lines.lpath_off, np.uint64),
            np.ascontiguousarray(lines.edges, np.int32), None if npairs is None else np.ascontiguousarray(npairs, np.int32)]
    if len(keep[6]) != len(keep[0]):
        raise ValueError("inv must have one entry per edge object")
    if len(keep[7]) < 1 or len(keep[9]) < 1 or len(keep[10]) != int(keep[9][-1]) + 1 or len(keep[11]) != int(keep[10][-1]) + 1:
        raise ValueError("path_off, line_off, cell_off and lpath_off must each have one entry more than what they divide")
    E, NL = len(keep[0]), len(keep[9]) - 1
    p = lambda a: _ptr(a) if a is not None and len(a) else None
    i = Step7In(hbv.K, E, p(keep[0]), hbv.n_vertices, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]), len(keep[7]) - 1, p(keep[7]), p(keep[8]),
                NL, p(keep[9]), p(keep[10]), p(keep[11]), p(keep[12]), 0 if npairs is None else len(keep[13]), p(keep[13]))
    prm = Step7Params(device, flags, min_line, min_link_count)
    o = Step7Out()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step7_links(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    try:
        size = {"E": E, "NL": NL, "n_links": int(o.n_links), "n_gaps": int(o.n_gaps)}
        arrays = {k: (_np_from(getattr(o, k), dt, size[n]) if getattr(o, k) else None) for k, (dt, n) in ARRAYS.items()}
        counters = {}
        for k in LINES_COUNTERS + LINKS_COUNTERS:
            v = getattr(o, k)
            counters[k] = [int(x) for x in v] if k in ("n_close", "n_reason") else int(v)
        return Step7Result(arrays, counters, {k: float(getattr(o, k)) for k in PHASES})
    finally:
        L.w2rap_step7_free(C.byref(o))


def line_stats(hbv: F.HBV, inv, paths, lines: F.Lines, device=0) -> Step7Result:
    """Part LINES: tol, llens and npairs (GetTol, GetLineLengths, GetLineNpairs)"""
    return run(hbv, inv, paths, lines, parts=("lines",), device=device)


def find_gaps(hbv: F.HBV, inv, paths, lines: F.Lines, npairs=None, min_line=5000, min_link_count=3, device=0) -> Step7Result:
    """MakeGaps up to the accepted gaps.  npairs None: counted in the same call (part LINES); given: read as the reference's MakeGaps
    reads .fin.lines.npairs, and part LINES does not run"""
    return run(hbv, inv, paths, lines, parts=("lines", "links") if npairs is None else ("links",), npairs=npairs, min_line=min_line, min_link_count=min_link_count, device=device)


def profile(line_files=False):
    """-> {kernel name: (total ms, launches)} of the last find_gaps / line_stats (line_files: of the last line_files) in this process"""
    L = lib()
    f = L.w2rap_step7_line_files_profile if line_files else L.w2rap_step7_profile
    n = f(None, 0)
    buf = C.create_string_buffer(int(n) + 16)
    f(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, k = line.rsplit(" ", 2)
        out[name] = (float(ms), int(k))
    return out


# ---------------------------------------------------------------------------------------------------------------- the line files
FILE_PARTS = {"fasta": 1, "efasta": 2, "src": 4}            # W2RAP_STEP7_FASTA / EFASTA / SRC
VOTE_ROW = 64                                               # W2RAP_STEP7_VOTE_ROW
GAP_N = 100                                                 # W2RAP_STEP7_GAP_N


class FastaIn(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_packed", C.c_void_p), ("edge_byte_off", C.c_void_p), ("edge_len", C.c_void_p),
                ("n_vertices", C.c_uint64), ("from_off", C.c_void_p), ("from_v", C.c_void_p), ("from_e", C.c_void_p), ("to_off", C.c_void_p), ("to_e", C.c_void_p),
                ("inv", C.c_void_p), ("n_paths", C.c_uint64), ("path_off", C.c_void_p), ("path_edges", C.c_void_p),
                ("n_lines", C.c_uint64), ("line_off", C.c_void_p), ("cell_off", C.c_void_p), ("lpath_off", C.c_void_p), ("line_edges", C.c_void_p)]


class FastaParams(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32)]


FASTA_TEXTS = ("fasta", "efasta", "src")
FASTA_ARRAYS = {"printed": (np.uint8, "NL"), "best": (np.int32, "NC"), "cov": (np.uint32, "NLP"), "left_share": (np.uint32, "NC"), "right_share": (np.uint32, "NC")}
FASTA_COUNTERS = ("n_printed", "n_skipped", "n_circular1", "n_circular2", "n_gap_cells", "n_cells_voted", "n_entries", "n_occurrences", "n_match_one", "n_match_none",
                  "n_match_several", "n_cells_tied", "n_cells_wide", "n_pieces_fasta", "n_pieces_efasta")
FASTA_PHASES = ("ms_vote", "ms_share", "ms_layout", "ms_write")


class FastaOut(C.Structure):
    _fields_ = ([x for k in FASTA_TEXTS for x in ((k, C.c_void_p), (k + "_len", C.c_uint64))] + [(k, C.c_void_p) for k in FASTA_ARRAYS] +
                [(k, C.c_uint64) for k in FASTA_COUNTERS] + [(k, C.c_float) for k in FASTA_PHASES])


@dataclass
class LineFiles:
    """the texts of include/w2rap_step7.h's w2rap_step7_fasta_out as bytes (None: the part was not asked for), its arrays by name, the
    counters and the device times"""
    fasta: bytes
    efasta: bytes
    src: bytes
    arrays: dict
    counters: dict
    ms: dict

    def __getattr__(self, k):
        try:
            return self.__dict__["arrays"][k]
        except KeyError:
            raise AttributeError(k)

    def write(self, dir):
        """a.lines.fasta, a.lines.efasta and a.lines.src into dir, those that were asked for"""
        import os
        for k in FASTA_TEXTS:
            if getattr(self, k) is not None:
                with open(os.path.join(dir, f"a.lines.{k}"), "wb") as f:
                    f.write(getattr(self, k))


def line_files(hbv: F.HBV, inv, paths, lines: F.Lines, parts=FASTA_TEXTS, device=0, flags=None) -> LineFiles:
    """w2rap_step7_line_files: DumpLineFiles on the graph with its bases, its involution, the read paths (as for `run`) and the lines.
    flags overrides parts (the tests of the argument checks)"""
    L = lib()
    if flags is None:
        flags = 0
        for p in parts:
            if p not in FILE_PARTS:
                raise ValueError(f"unknown part {p!r}: one of {sorted(FILE_PARTS)}")
            flags |= FILE_PARTS[p]
        if not flags:
            raise ValueError("no part asked for")
    keep = [np.ascontiguousarray(hbv.edge_packed, np.uint8), np.ascontiguousarray(hbv.edge_byte_off, np.uint64), np.ascontiguousarray(hbv.edge_len, np.uint32),
            np.ascontiguousarray(hbv.from_off, np.uint64), np.ascontiguousarray(hbv.from_v, np.int32), np.ascontiguousarray(hbv.from_e, np.int32),
            np.ascontiguousarray(hbv.to_off, np.uint64), np.ascontiguousarray(hbv.to_e, np.int32), np.ascontiguousarray(inv, np.int32),
            np.ascontiguousarray(paths[1], np.uint64), np.ascontiguousarray(paths[2], np.int32),
            np.ascontiguousarray(lines.line_off, np.uint64), np.ascontiguousarray(lines.cell_off, np.uint64), np.ascontiguousarray(lines.lpath_off, np.uint64),
            np.ascontiguousarray(lines.edges, np.int32)]
    E = len(keep[2])
    if len(keep[8]) != E or len(keep[1]) != E + 1:
        raise ValueError("inv must have one entry per edge object, edge_byte_off one more")
    if len(keep[9]) < 1 or len(keep[11]) < 1 or len(keep[12]) != int(keep[11][-1]) + 1 or len(keep[13]) != int(keep[12][-1]) + 1:
        raise ValueError("path_off, line_off, cell_off and lpath_off must each have one entry more than what they divide")
    NL, NC, NLP = len(keep[11]) - 1, len(keep[12]) - 1, len(keep[13]) - 1
    p = lambda a: _ptr(a) if len(a) else None
    i = FastaIn(hbv.K, E, p(keep[0]), p(keep[1]), p(keep[2]), hbv.n_vertices, p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]), p(keep[8]),
                len(keep[9]) - 1, p(keep[9]), p(keep[10]), NL, p(keep[11]), p(keep[12]), p(keep[13]), p(keep[14]))
    prm = FastaParams(device, flags)
    o = FastaOut()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step7_line_files(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    try:
        size = {"NL": NL, "NC": NC, "NLP": NLP}
        texts = {k: (C.string_at(getattr(o, k), int(getattr(o, k + "_len"))) if getattr(o, k) else None) for k in FASTA_TEXTS}
        arrays = {k: (_np_from(getattr(o, k), dt, size[n]) if getattr(o, k) else None) for k, (dt, n) in FASTA_ARRAYS.items()}
        return LineFiles(texts["fasta"], texts["efasta"], texts["src"], arrays, {k: int(getattr(o, k)) for k in FASTA_COUNTERS}, {k: float(getattr(o, k)) for k in FASTA_PHASES})
    finally:
        L.w2rap_step7_line_files_free(C.byref(o))


# ---------------------------------------------------------------------------------------------------------------- the coverage
COV_PARTS = {"npairs": 1, "peak": 2, "edges": 4}           # W2RAP_STEP7_COV_*: a part brings those before it
RULES = ("none", "line", "cell", "long")                    # W2RAP_STEP7_RULE_*
PEAK_WAYS = ("no_data", "single", "largest_mass", "scored") # W2RAP_STEP7_PEAK_*


class CovIn(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_edge_objs", C.c_uint64), ("edge_len", C.c_void_p), ("inv", C.c_void_p), ("n_paths", C.c_uint64), ("path_off", C.c_void_p),
                ("path_edges", C.c_void_p), ("n_lines", C.c_uint64), ("line_off", C.c_void_p), ("cell_off", C.c_void_p), ("lpath_off", C.c_void_p), ("line_edges", C.c_void_p)]


class CovParams(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("frac", C.c_double), ("min_edge_size", C.c_int32), ("long_form", C.c_uint32)]


LONG_FORMS = {"default": 0, "sorted": 1, "sort_free": 2}    # W2RAP_STEP7_LONG_*
COV_ARRAYS = {"npairs": (np.int32, "NL"), "llens": (np.int32, "NL"), "covl": (np.float64, "NL"), "covx": (np.float64, "n_candidates"), "mass": (np.int64, "n_candidates"),
              "ids": (np.int32, "n_candidates"), "cov": (np.float32, "E"), "rule": (np.uint8, "E"), "group_line": (np.int32, "n_groups"), "group_cell": (np.int32, "n_groups"),
              "group_len": (np.int32, "n_groups"), "group_pairs": (np.int64, "n_groups"), "group_z_off": (np.uint64, "n_groups+1"), "group_z": (np.int32, "NZ"),
              "long_edge": (np.int32, "n_long_asked"), "long_pairs": (np.int64, "n_long_asked")}
COV_SCALARS = (("base_cov", C.c_double), ("cn_fraction", C.c_double), ("max_len", C.c_int32), ("min_len", C.c_int32))
COV_COUNTERS = ("n_candidates", "n_groups", "n_cn_edges", "n_cn_good", "n_simple", "n_noise", "n_edge", "n_sparse", "n_not_window_max", "n_shallow", "n_centred", "n_prefiltered",
                "n_peaks", "peak_way", "n_score_ties_taken", "halved", "n_cells", "n_cells_empty", "n_cells_sizes", "n_cells_one_in", "n_classes", "n_classes_short",
                "n_line_lines", "n_rule", "n_long_asked", "n_undefined", "n_group_entries", "index_built")
COV_PHASES = ("ms_lines", "ms_index", "ms_groups", "ms_rules", "ms_long")
_COV_CTYPE = {"n_rule": C.c_uint64 * 4, "n_group_entries": C.c_uint64 * 2}


class CovOut(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in COV_ARRAYS] + list(COV_SCALARS) + [(k, _COV_CTYPE.get(k, C.c_uint64)) for k in COV_COUNTERS] + [(k, C.c_float) for k in COV_PHASES])


@dataclass
class Coverage:
    """w2rap_step7_cov_out: the arrays by name (None: the part was not asked for; group_z as one list per group), base_cov, cn_fraction,
    max_len and min_len, the counters and the device times"""
    arrays: dict
    base_cov: float
    cn_fraction: float
    max_len: int
    min_len: int
    counters: dict
    ms: dict

    def __getattr__(self, k):
        try:
            return self.__dict__["arrays"][k]
        except KeyError:
            raise AttributeError(k)

    def cn_line(self) -> str:
        """`CN fraction good = ...` as the reference's stream prints the double (operator<< at the default precision of 6: %g)"""
        return "CN fraction good = " + _stream_double(self.cn_fraction)


def _stream_double(x: float) -> str:
    """a double through std::ostream at its defaults: %g; inf and nan as the C library prints them (a NaN of 0 / 0 carries the sign bit on
    x86-64: "-nan")"""
    import math
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%g" % x


def coverage(hbv: F.HBV, inv, paths, lines: F.Lines, parts=("edges",), frac=0.1, min_edge_size=2000, device=0, flags=None, long_form="default") -> Coverage:
    """w2rap_step7_coverage: ComputeCoverage and CNIntegerFraction for one sample.  parts: "npairs" (npairs and llens only), "peak" (and
    covl, the candidates, base_cov), "edges" (everything).  flags overrides parts (the tests of the argument checks); long_form: how the
    long edges' pairs are counted, "sorted" or "sort_free" (the same counts either way)"""
    L = lib()
    if flags is None:
        flags = 0
        for p in parts:
            if p not in COV_PARTS:
                raise ValueError(f"unknown part {p!r}: one of {sorted(COV_PARTS)}")
            flags |= COV_PARTS[p]
        if not flags:
            raise ValueError("no part asked for")
    keep = [np.ascontiguousarray(hbv.edge_len, np.uint32), np.ascontiguousarray(inv, np.int32), np.ascontiguousarray(paths[1], np.uint64), np.ascontiguousarray(paths[2], np.int32),
            np.ascontiguousarray(lines.line_off, np.uint64), np.ascontiguousarray(lines.cell_off, np.uint64), np.ascontiguousarray(lines.lpath_off, np.uint64),
            np.ascontiguousarray(lines.edges, np.int32)]
    if len(keep[1]) != len(keep[0]):
        raise ValueError("inv must have one entry per edge object")
    if len(keep[2]) < 1 or len(keep[4]) < 1 or len(keep[5]) != int(keep[4][-1]) + 1 or len(keep[6]) != int(keep[5][-1]) + 1:
        raise ValueError("path_off, line_off, cell_off and lpath_off must each have one entry more than what they divide")
    E, NL = len(keep[0]), len(keep[4]) - 1
    p = lambda a: _ptr(a) if len(a) else None
    i = CovIn(hbv.K, E, p(keep[0]), p(keep[1]), len(keep[2]) - 1, p(keep[2]), p(keep[3]), NL, p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]))
    prm = CovParams(device, flags, frac, min_edge_size, LONG_FORMS[long_form])
    o = CovOut()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step7_coverage(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc:
        raise Step2Error(rc, err.value.decode(errors="replace"))
    try:
        size = {"E": E, "NL": NL, "n_candidates": int(o.n_candidates), "n_groups": int(o.n_groups), "n_groups+1": int(o.n_groups) + 1, "n_long_asked": int(o.n_long_asked)}
        arrays = {}
        for k, (dt, n) in COV_ARRAYS.items():
            if k == "group_z":
                continue
            arrays[k] = _np_from(getattr(o, k), dt, size[n]) if getattr(o, k) else None
        if arrays["group_z_off"] is not None:
            zo = arrays.pop("group_z_off").astype(np.int64)
            z = _np_from(o.group_z, np.int32, int(zo[-1])) if o.group_z else np.zeros(0, np.int32)
            arrays["group_z"] = [z[zo[g]:zo[g + 1]].tolist() for g in range(len(zo) - 1)]
        else:
            arrays.pop("group_z_off")
            arrays["group_z"] = None
        counters = {k: ([int(x) for x in getattr(o, k)] if k in _COV_CTYPE else int(getattr(o, k))) for k in COV_COUNTERS}
        return Coverage(arrays, float(o.base_cov), float(o.cn_fraction), int(o.max_len), int(o.min_len), counters, {k: float(getattr(o, k)) for k in COV_PHASES})
    finally:
        L.w2rap_step7_coverage_free(C.byref(o))


def _fixed2(x) -> str:
    """ToString(float, 2) (feudal/CharString.h:35-37): the float through a fixed stream of precision 2 -- printf's %.2f of the float's
    value; inf and nan as the C library prints them"""
    import math
    x = float(np.float32(x))
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return "%.2f" % x


def line_stats_text(result, lines: F.Lines) -> str:
    """WriteLineStats (Lines.cc:357-379), the text of .lines.stats, for one sample: per line `line[i] e1..e2 len= npairs=` and, where the
    first edge of the line has a defined coverage (cov >= 0), ` cov=<two decimals>x`; ` cov=?x` for a NaN.  result: a Coverage (or anything with llens, npairs, cov)"""
    nested = lines.nested()
    out = []
    for i, line in enumerate(nested):
        e1, e2 = line[0][0][0], line[-1][0][0]
        row = f"line[{i}] {e1}..{e2} len={int(result.llens[i])} npairs={int(result.npairs[i])}"
        c = result.cov[e1]
        if c >= 0:
            row += f" cov={_fixed2(c)}x"
        elif c != c:                                            # a NaN (base_cov 0 and no pairs): what the reference's -Ofast build prints, see w2rap_step7.h
            row += " cov=?x"
        out.append(row + "\n")
    return "".join(out)


def sort_lines(hbv: F.HBV, inv, lines: F.Lines, paths=None, device=0) -> F.Lines:
    """SortLines (Lines.cc:664-678): the lines ordered by (-llens, min(F, inv[B]), F), F and B the first and the last edge of a line --
    the key of two different lines differs (F is the first edge of one line only), so the order does not depend on the sort.  llens comes
    from the LINES kernels (line_stats); the sort and the permutation of the nested offsets are line-sized and run here"""
    if paths is None:
        paths = (np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, np.int32))
    llens = line_stats(hbv, inv, paths, lines, device=device).llens
    nested, inv = lines.nested(), np.asarray(inv)
    key = lambda i: (-int(llens[i]), min(nested[i][0][0][0], int(inv[nested[i][-1][0][0]])), nested[i][0][0][0])
    return F.Lines.from_nested([nested[i] for i in sorted(range(len(nested)), key=key)])


def _commas(x: int) -> str:
    return f"{x:,}"


def stats_text(llens, K, prefix) -> str:
    """the `stats` file of FinalFiles (FinalFiles.cc:73-104): LineN50 over the lines of 1000 K-mers or more with K-1 added (N50 of
    math/Functions.cc:300-342 on the ascending lengths: the first length at which the running sum reaches half, the mean with the next
    one where it lands on half exactly), and the totals of the lines of 1, 10 and 100 thousand K-mers or more, each halved"""
    llens = [int(x) for x in llens]
    lens = sorted(x + K - 1 for x in llens if x >= 1000)
    n50, total, half = 0, sum(lens), 0
    for i, x in enumerate(lens):
        half += x
        if 2 * half == total and i < len(lens) - 1:
            n50 = (x + lens[i + 1]) // 2
            break
        if 2 * half >= total:
            n50 = x
            break
    tot = [sum(x for x in llens if x >= m) // 2 for m in (1000, 10000, 100000)]
    return (f"# {prefix} assembly statistics\n\nN50: {_commas(n50)}\ntotal bases in 1 kb+ sequences: {_commas(tot[0])}\n"
            f"total bases in 10 kb+ sequences: {_commas(tot[1])}\ntotal bases in 100 kb+ sequences: {_commas(tot[2])}\n")


def involution(hbv: F.HBV) -> np.ndarray:
    """HyperBasevector::Involution (src/paths/HyperBasevector.cc:648-660): the i-th edge object in sequence order pairs with the i-th in
    the order of the reverse complements.  In a graph that holds the reverse complement of every edge object once, any total order
    gives the same pairing: inv[e] is the object whose sequence is e's reverse complement"""
    codes, off = hbv.edge_codes()
    seq = [codes[int(off[e]):int(off[e + 1])] for e in range(hbv.n_edges)]
    x1 = sorted(range(len(seq)), key=lambda e: seq[e].tobytes())
    x2 = sorted(range(len(seq)), key=lambda e: (3 - seq[e][::-1]).astype(np.uint8).tobytes())
    inv = np.zeros(len(seq), np.int32)
    inv[x1] = x2
    return inv


def gaps_text(res: Step7Result) -> str:
    """one line per accepted gap: "from to inverse", then the line the reference prints about the forced symmetry"""
    a = res.arrays
    body = "".join(f"{f} {t} {i}\n" for f, t, i in zip(a["gap_from"].tolist(), a["gap_to"].tolist(), a["gap_inv"].tolist()))
    return body + f"# deleting {res.counters['n_sym_deleted']} gaps and adding {res.counters['n_sym_added']} gaps to force symmetry\n"


def main(argv=None):
    import argparse
    import os
    ap = argparse.ArgumentParser(prog="python -m w2rap_contigger_amd.step7", description="MakeGaps' accepted gaps from PREFIX.contig.hbv/.paths and PREFIX.fin.lines/.npairs")
    ap.add_argument("dir"); ap.add_argument("prefix")
    ap.add_argument("--min_line", type=int, default=5000); ap.add_argument("--min_link_count", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--out", default=None, help="the text file to write (default DIR/PREFIX.gaps.txt)")
    ap.add_argument("--line_files", metavar="LINES_FILE", default=None, help="write a.lines.fasta, a.lines.efasta, a.lines.src and stats into DIR from this lines file instead")
    ap.add_argument("--coverage", metavar="LINES_FILE", default=None, help="write PREFIX_assembly.covs, .lines.npairs and .lines.stats into DIR from this lines file and print the CN fraction")
    a = ap.parse_args(argv)
    stem = os.path.join(a.dir, a.prefix)
    hbv = F.read_hbv(stem + ".contig.hbv")
    paths = F.read_paths(stem + ".contig.paths")
    if a.coverage:
        lines = F.read_lines(a.coverage)
        res = coverage(hbv, involution(hbv), paths, lines, device=a.device)
        F.write_covs(stem + "_assembly.covs", [res.cov])
        F.write_int_vec(stem + "_assembly.lines.npairs", res.npairs)
        with open(stem + "_assembly.lines.stats", "w") as f:
            f.write(line_stats_text(res, lines))
        print(res.cn_line())
        if not a.line_files:
            return 0
    if a.line_files:
        lines, inv = F.read_lines(a.line_files), involution(hbv)
        res = line_files(hbv, inv, paths, lines, device=a.device)
        res.write(a.dir)
        with open(os.path.join(a.dir, "stats"), "w") as f:
            f.write(stats_text(line_stats(hbv, inv, paths, lines, device=a.device).llens, hbv.K, a.prefix))
        print(f"{res.counters['n_printed']} lines printed, {res.counters['n_skipped']} skipped, {res.counters['n_cells_voted']} cells voted -> {a.dir}/a.lines.fasta, .efasta, .src, stats")
        return 0
    lines = F.read_lines(stem + ".fin.lines")
    npairs = F.read_int_vec(stem + ".fin.lines.npairs")
    res = find_gaps(hbv, involution(hbv), paths, lines, npairs=npairs, min_line=a.min_line, min_link_count=a.min_link_count, device=a.device)
    out = a.out or stem + ".gaps.txt"
    with open(out, "w") as f:
        f.write(gaps_text(res))
    print(f"{res.counters['n_gaps']} gaps of {res.counters['n_links']} links ({res.counters['n_nears']} nears) -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

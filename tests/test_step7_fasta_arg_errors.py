"""What w2rap_step7_line_files refuses, each refusal once: one mutation of a small valid input, the code and the message it is answered
with.  Every one is refused on the host before the device is touched, so this runs without a GPU.

"A path shorter than the K-1 bases cut from it" cannot be reached from outside: the Cat of a path that has an edge is at least K bases
once every edge has K, and an edge shorter than K is refused first -- that refusal stands for it here."""
import ctypes as C

import numpy as np
import pytest

import step7_cases as S
import step7_fasta_cases as FC
from w2rap_contigger_amd import formats as F, step7

E_ARG, E_LIMIT = 1, 5
ARRAYS = {"edge_packed": np.uint8, "edge_byte_off": np.uint64, "edge_len": np.uint32, "from_off": np.uint64, "from_v": np.int32, "from_e": np.int32, "to_off": np.uint64,
          "to_e": np.int32, "inv": np.int32, "path_off": np.uint64, "path_edges": np.int32, "line_off": np.uint64, "cell_off": np.uint64, "lpath_off": np.uint64, "line_edges": np.int32}


def base():
    """a (0) -> {b1 (2), b2 (4)} -> c (6) -> {d1 (8), d2 (10)} -> f (12): 14 edge objects, the line of five cells and its mirror, 4 read paths"""
    g = S.Contigs(60, real=True); v = [g.v() for _ in range(6)]
    a = g.e(v[0], v[1], 60); b1 = g.e(v[1], v[2], 40); b2 = g.e(v[1], v[2], 45); c = g.e(v[2], v[3], 60); d1 = g.e(v[3], v[4], 40); d2 = g.e(v[3], v[4], 45); f = g.e(v[4], v[5], 60)
    g.pair([a, b2, c], [c ^ 1], 2)
    case = g.case(lines=FC.both([[[[a]], [[b1], [b2]], [[c]], [[d1], [d2]], [[f]]]]))
    h = case["hbv"]
    d = dict(K=h.K, n_vertices=h.n_vertices, edge_packed=h.edge_packed, edge_byte_off=h.edge_byte_off, edge_len=h.edge_len, from_off=h.from_off, from_v=h.from_v, from_e=h.from_e,
             to_off=h.to_off, to_e=h.to_e, inv=case["inv"], path_off=case["paths"][1], path_edges=case["paths"][2], flags=0, nested=case["nested"])
    d = {k: (np.array(v, ARRAYS[k]) if k in ARRAYS else v) for k, v in d.items()}
    set_lines(d, d["nested"])
    return d


def set_lines(d, nested):
    l = F.Lines.from_nested(nested)
    d.update(line_off=l.line_off, cell_off=l.cell_off, lpath_off=l.lpath_off, line_edges=l.edges)


def call(d):
    """-> (code, message) of w2rap_step7_line_files on the dict's fields; None is a null pointer"""
    L = step7.lib()
    keep = {k: (None if d[k] is None else np.ascontiguousarray(d[k], t)) for k, t in ARRAYS.items()}
    p = lambda k: None if keep[k] is None else keep[k].ctypes.data_as(C.c_void_p)
    n_lines = d.get("n_lines", 0 if d["line_off"] is None else len(d["line_off"]) - 1)
    i = step7.FastaIn(d["K"], len(d["edge_len"]), p("edge_packed"), p("edge_byte_off"), p("edge_len"), d["n_vertices"], p("from_off"), p("from_v"), p("from_e"), p("to_off"), p("to_e"),
                      p("inv"), len(d["path_off"]) - 1, p("path_off"), p("path_edges"), n_lines, p("line_off"), p("cell_off"), p("lpath_off"), p("line_edges"))
    prm = step7.FastaParams(0, d["flags"])
    o = step7.FastaOut()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step7_line_files(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc == 0:
        L.w2rap_step7_line_files_free(C.byref(o))
    return rc, err.value.decode()


def lines_of(f):
    def m(d):
        n = [[[list(p) for p in cell] for cell in line] for line in d["nested"]]
        f(n)
        set_lines(d, n)
    return m


def put(k, i, v):
    def m(d):
        d[k] = d[k].copy(); d[k][i] = v
    return m


def field(k, v):
    def m(d):
        d[k] = v
    return m


def long_line(d):
    d["edge_len"] = d["edge_len"].copy(); d["edge_len"][0] = 2 ** 30
    d["edge_byte_off"] = np.concatenate([[0], np.cumsum((d["edge_len"].astype(np.uint64) + 3) // 4)]).astype(np.uint64)      # (the packed bases are never read: refused before)
    lines_of(lambda n: n.append([[[0, 0, 0]]]))(d)


def null_line_off(d):
    d["n_lines"] = len(d["line_off"]) - 1; d["line_off"] = None


CASES = [
    # its own
    ("empty_path_in_a_cell_of_two", lines_of(lambda n: n[0][1][0].clear()), E_ARG, "an empty path in a cell of two or more paths"),
    ("gap_in_an_even_cell", lines_of(lambda n: n[0][2][0].clear()), E_ARG, "an even cell whose first path is empty"),
    ("path_shorter_than_the_cut", put("edge_len", 2, 18), E_ARG, "an edge object shorter than K bases"),
    ("packed_edges_shorter_than_edge_len", put("edge_len", 3, 99), E_ARG, "edge_byte_off does not match edge_len"),
    ("edge_byte_off_not_from_0", put("edge_byte_off", 0, 1), E_ARG, "edge_byte_off must start at 0"),
    ("null_edge_packed", field("edge_packed", None), E_ARG, "null graph array"),
    ("unknown_flag", field("flags", 8), E_ARG, "unknown flag"),
    ("K_15", field("K", 15), E_ARG, "K must be in [16, 640]"),
    # the line checks of w2rap_step7_links
    ("even_number_of_cells", lines_of(lambda n: n[-1].pop()), E_ARG, "a line with an even number of cells"),
    ("line_without_cells", lines_of(lambda n: n.append([])), E_ARG, "a line with an even number of cells"),
    ("empty_first_cell", lines_of(lambda n: n[-1][0].clear()), E_ARG, "the first or last cell of a line is empty"),
    ("empty_middle_cell", lines_of(lambda n: n[-1][1].clear()), E_ARG, "a cell without a path"),
    ("first_path_of_first_cell_empty", lines_of(lambda n: n.append([[[], [3]]])), E_ARG, "the first path of a line's first or last cell is empty"),
    ("line_edge_negative", put("line_edges", 2, -1), E_ARG, "a line names an edge object that does not exist"),
    ("line_edge_E", put("line_edges", 2, 14), E_ARG, "a line names an edge object that does not exist"),
    ("line_off_not_from_0", put("line_off", 0, 1), E_ARG, "line_off must start at 0"),
    ("cell_off_descends", put("cell_off", 1, 99), E_ARG, "cell_off is not ascending"),
    ("lpath_off_descends", put("lpath_off", 1, 99), E_ARG, "lpath_off is not ascending"),
    ("null_line_off", null_line_off, E_ARG, "null line_off"),
    ("null_line_edges", field("line_edges", None), E_ARG, "null line_edges"),
    ("line_of_2_31_kmers", long_line, E_LIMIT, "a line of 2^31 K-mers or more"),
    # the graph and the paths
    ("path_edge_E", put("path_edges", 0, 14), E_ARG, "a path names an edge object that does not exist"),
    ("path_off_descends", put("path_off", 1, 99), E_ARG, "path_off is not ascending"),
    ("inv_out_of_range", put("inv", 3, 14), E_ARG, "inv names an edge object that does not exist"),
    ("null_inv", field("inv", None), E_ARG, "null graph array"),
    ("from_v_disagrees", put("from_v", 0, 5), E_ARG, "from_v and to_e disagree about the vertex an edge enters"),
]


@pytest.mark.parametrize("name,mutation,code,msg", CASES, ids=[c[0] for c in CASES])
def test_refused_before_the_device_is_touched(name, mutation, code, msg):
    d = base()
    mutation(d)
    assert call(d) == (code, msg)


def test_null_arguments():
    L = step7.lib()
    err = C.create_string_buffer(64)
    assert L.w2rap_step7_line_files(None, None, C.byref(step7.FastaOut()), err, 64) == E_ARG and err.value == b"null argument"
    assert L.w2rap_step7_line_files(None, None, None, err, 64) == E_ARG

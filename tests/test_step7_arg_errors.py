"""What w2rap_step7_links refuses, each refusal once: one mutation of a small valid input, the code and the message it is answered with.
Every one is refused on the host before the device is touched, so this runs without a GPU.  The pieces of csrc/args.h that do the
refusing also run stand-alone under the address and undefined-behaviour sanitizers (tests/step7_args_main.cc), every array in a heap
block of exactly its size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import step7_cases as S
from conftest import ROOT
from w2rap_contigger_amd import formats as F, step7

E_ARG, E_LIMIT = 1, 5
ARRAYS = {"edge_len": np.uint32, "from_off": np.uint64, "from_v": np.int32, "from_e": np.int32, "to_off": np.uint64, "to_e": np.int32, "inv": np.int32,
          "path_off": np.uint64, "path_edges": np.int32, "line_off": np.uint64, "cell_off": np.uint64, "lpath_off": np.uint64, "line_edges": np.int32, "npairs": np.int32}


def base():
    """bubbles_1 of the hand-made cases: 10 edge objects, 6 read paths, a line with a two-path cell and its mirror, npairs given"""
    c = S.hand_cases()["bubbles_1"]
    h = c["hbv"]
    d = dict(K=h.K, n_vertices=h.n_vertices, edge_len=h.edge_len, from_off=h.from_off, from_v=h.from_v, from_e=h.from_e, to_off=h.to_off, to_e=h.to_e, inv=c["inv"],
             path_off=c["paths"][1], path_edges=c["paths"][2], npairs=c["npairs"], flags=0, min_line=5000, min_link_count=3, nested=c["nested"])
    d = {k: (np.array(v, ARRAYS[k]) if k in ARRAYS else v) for k, v in d.items()}
    set_lines(d, d["nested"])
    return d


def set_lines(d, nested):
    l = F.Lines.from_nested(nested)
    d.update(line_off=l.line_off, cell_off=l.cell_off, lpath_off=l.lpath_off, line_edges=l.edges)


def sizes(d):
    """the counts the struct carries, from the arrays unless a mutation has set them"""
    return dict(n_edge_objs=d.get("n_edge_objs", len(d["edge_len"])), n_paths=d.get("n_paths", len(d["path_off"]) - 1),
                n_lines=d.get("n_lines", 0 if d["line_off"] is None else len(d["line_off"]) - 1), n_npairs=d.get("n_npairs", 0 if d["npairs"] is None else len(d["npairs"])))


def call(d):
    """-> (code, message) of w2rap_step7_links on the dict's fields; None is a null pointer"""
    L = step7.lib()
    keep = {k: (None if d[k] is None else np.ascontiguousarray(d[k], t)) for k, t in ARRAYS.items()}
    p = lambda k: None if keep[k] is None else keep[k].ctypes.data_as(C.c_void_p)
    n = sizes(d)
    i = step7.Step7In(d["K"], n["n_edge_objs"], p("edge_len"), d["n_vertices"], p("from_off"), p("from_v"), p("from_e"), p("to_off"), p("to_e"), p("inv"),
                      n["n_paths"], p("path_off"), p("path_edges"), n["n_lines"], p("line_off"), p("cell_off"), p("lpath_off"), p("line_edges"), n["n_npairs"], p("npairs"))
    prm = step7.Step7Params(0, d["flags"], d["min_line"], d["min_link_count"])
    o = step7.Step7Out()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step7_links(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc == 0:
        L.w2rap_step7_free(C.byref(o))
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
    lines_of(lambda n: n.append([[[0, 0, 0]]]))(d)


def swap_inv(d):
    d["inv"] = d["inv"].copy(); d["inv"][0] = 0


def npairs_of(n):
    def m(d):
        d["npairs"] = np.zeros(len(d["npairs"]) + n, np.int32)
    return m


def links_only_without_npairs(d):
    d["flags"] = 2; d["npairs"] = None


# (name, mutation, code, message, answered by a piece of args.h)
CASES = [
    ("edge_in_no_line", lines_of(lambda n: n.pop(0)), E_ARG, "an edge object that belongs to no line", True),
    ("even_number_of_cells", lines_of(lambda n: n[-1].pop()), E_ARG, "a line with an even number of cells", True),
    ("line_without_cells", lines_of(lambda n: n.append([])), E_ARG, "a line with an even number of cells", True),
    ("empty_first_cell", lines_of(lambda n: n[-1][0].clear()), E_ARG, "the first or last cell of a line is empty", True),
    ("empty_last_cell", lines_of(lambda n: n[-1][-1].clear()), E_ARG, "the first or last cell of a line is empty", True),
    ("empty_middle_cell", lines_of(lambda n: n[-1][1].clear()), E_ARG, "a cell without a path", True),
    ("first_path_of_first_cell_empty", lines_of(lambda n: n.append([[[], [3]]])), E_ARG, "the first path of a line's first or last cell is empty", True),
    ("line_edge_negative", put("line_edges", 2, -1), E_ARG, "a line names an edge object that does not exist", True),
    ("line_edge_E", put("line_edges", 2, 10), E_ARG, "a line names an edge object that does not exist", True),
    ("line_off_not_from_0", put("line_off", 0, 1), E_ARG, "line_off must start at 0", True),
    ("cell_off_descends", put("cell_off", 1, 9), E_ARG, "cell_off is not ascending", True),
    ("lpath_off_descends", put("lpath_off", 1, 9), E_ARG, "lpath_off is not ascending", True),
    ("null_line_off", field("line_off", None), E_ARG, "null line_off", True),        # (n_lines stays what it was: mutated())
    ("null_cell_off", field("cell_off", None), E_ARG, "null cell_off", True),
    ("null_lpath_off", field("lpath_off", None), E_ARG, "null lpath_off", True),
    ("null_line_edges", field("line_edges", None), E_ARG, "null line_edges", True),
    ("line_of_2_31_kmers", long_line, E_LIMIT, "a line of 2^31 K-mers or more", True),
    ("odd_n_paths", field("n_paths", 5), E_ARG, "n_paths is odd: reads r and r ^ 1 are mates", True),
    ("npairs_short", npairs_of(-1), E_ARG, "npairs must have one entry per line", True),
    ("npairs_long", npairs_of(1), E_ARG, "npairs must have one entry per line", True),
    ("links_only_without_npairs", links_only_without_npairs, E_ARG, "LINKS without LINES needs npairs", True),
    ("path_edge_E", put("path_edges", 0, 10), E_ARG, "a path names an edge object that does not exist", True),
    ("path_off_descends", put("path_off", 1, 99), E_ARG, "path_off is not ascending", True),
    ("inv_out_of_range", put("inv", 3, 10), E_ARG, "inv names an edge object that does not exist", True),
    ("inv_not_an_involution", swap_inv, E_ARG, "inv is not an involution: inv[inv[e]] != e", True),
    ("null_inv", field("inv", None), E_ARG, "null graph array", True),
    ("from_v_disagrees", put("from_v", 0, 5), E_ARG, "from_v and to_e disagree about the vertex an edge enters", True),
    ("edge_shorter_than_K", put("edge_len", 4, 19), E_ARG, "an edge object shorter than K bases", True),
    ("unknown_flag", field("flags", 4), E_ARG, "unknown flag", False),
    ("K_15", field("K", 15), E_ARG, "K must be in [16, 640]", False),
    ("negative_min_line", field("min_line", -1), E_ARG, "min_line and min_link_count must not be negative", False),
    ("negative_min_link_count", field("min_link_count", -1), E_ARG, "min_line and min_link_count must not be negative", False),
]


def mutated(name):
    d = base()
    mutation = next(m for n, m, *_ in CASES if n == name)
    if name == "null_line_off":
        d["n_lines"] = len(d["line_off"]) - 1
    mutation(d)
    return d


@pytest.mark.parametrize("name,code,msg", [(n, c, m) for n, _, c, m, _ in CASES])
def test_refused_before_the_device_is_touched(name, code, msg):
    assert call(mutated(name)) == (code, msg)


def _block(name, d):
    out = [f"case {name}"]
    for k, v in {**sizes(d), "K": d["K"], "n_vertices": d["n_vertices"], "links_only": int(d["flags"] == 2)}.items():
        out.append(f"s {k} {int(v)}")
    for k in ARRAYS:
        out.append(f"a {k} null" if d[k] is None else f"a {k} {len(d[k])} " + " ".join(str(int(x)) for x in d[k]))
    return "\n".join(out + ["end"])


def test_the_new_pieces_under_a_host_sanitizer(tmp_path):
    exe = str(tmp_path / "step7_args")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "step7_args_main.cc")],
                   check=True, capture_output=True, text=True)
    shared = [n for n, _, _, _, sh in CASES if sh]
    text = "\n".join(_block(n, mutated(n)) for n in shared) + "\n" + _block("valid", base()) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    want = {n: (c, m) for n, _, c, m, _ in CASES}
    got = {}
    for line in r.stdout.splitlines():
        name, code, *msg = line.split(" ", 2)
        got[name] = (int(code), msg[0] if msg else "")
    assert got == {**{n: want[n] for n in shared}, "valid": (0, "")}

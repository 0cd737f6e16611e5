"""What w2rap_step7_coverage refuses, each refusal once: one mutation of a small valid input, the code and the message it is answered
with.  Every one is refused on the host before the device is touched, so this runs without a GPU.  The host half of the call
(csrc/step7_peak.h: the checks, the candidates, the peak finder, the grouping of the cells) also runs stand-alone under the address and
undefined-behaviour sanitizers (tests/step7_cov_main.cc) on the refusals and on every peak-finder case, each array in a heap block of
exactly its size; its base_cov must be the model's, bit for bit."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import step7_cov_cases as CC
import step7_cov_model as M
from conftest import ROOT
from w2rap_contigger_amd import formats as F, step7

E_ARG, E_LIMIT = 1, 5
ARRAYS = {"edge_len": np.uint32, "inv": np.int32, "path_off": np.uint64, "path_edges": np.int32, "line_off": np.uint64, "cell_off": np.uint64, "lpath_off": np.uint64,
          "line_edges": np.int32}


def as_input(case, nested=None):
    h = case["hbv"]
    d = dict(K=h.K, edge_len=h.edge_len, inv=case["inv"], path_off=case["paths"][1], path_edges=case["paths"][2], flags=0, frac=0.1, min_edge_size=2000,
             nested=case["nested"] if nested is None else nested)
    d = {k: (np.array(v, ARRAYS[k]) if k in ARRAYS else v) for k, v in d.items()}
    set_lines(d, d["nested"])
    return d


def base():
    """a bubble between two contigs with its mirror, and a lone contig: 10 edge objects, 5 lines"""
    return as_input(CC.model_cases()["cell_named_twice"])


def set_lines(d, nested):
    l = F.Lines.from_nested(nested)
    d.update(line_off=l.line_off, cell_off=l.cell_off, lpath_off=l.lpath_off, line_edges=l.edges)


def sizes(d):
    return dict(n_edge_objs=d.get("n_edge_objs", len(d["edge_len"])), n_paths=d.get("n_paths", len(d["path_off"]) - 1),
                n_lines=d.get("n_lines", 0 if d["line_off"] is None else len(d["line_off"]) - 1))


def call(d):
    """-> (code, message) of w2rap_step7_coverage on the dict's fields; None is a null pointer"""
    L = step7.lib()
    keep = {k: (None if d[k] is None else np.ascontiguousarray(d[k], t)) for k, t in ARRAYS.items()}
    p = lambda k: None if keep[k] is None else keep[k].ctypes.data_as(C.c_void_p)
    n = sizes(d)
    i = step7.CovIn(d["K"], n["n_edge_objs"], p("edge_len"), p("inv"), n["n_paths"], p("path_off"), p("path_edges"), n["n_lines"], p("line_off"), p("cell_off"), p("lpath_off"),
                    p("line_edges"))
    prm = step7.CovParams(0, d["flags"], d["frac"], d["min_edge_size"], d.get("long_form", 0))
    o = step7.CovOut()
    err = C.create_string_buffer(1024)
    rc = L.w2rap_step7_coverage(C.byref(i), C.byref(prm), C.byref(o), err, 1024)
    if rc == 0:
        L.w2rap_step7_coverage_free(C.byref(o))
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


def no_lines(d):
    set_lines(d, [])


def long_line(d):
    d["edge_len"] = d["edge_len"].copy(); d["edge_len"][0] = 2 ** 30
    lines_of(lambda n: n.append([[[0, 0, 0]]]))(d)


# (name, mutation, code, message)
CASES = [
    ("no_lines", no_lines, E_ARG, "no lines: the reference takes the largest of no lengths"),
    ("line_edge_E", put("line_edges", 2, 12), E_ARG, "a line names an edge object that does not exist"),
    ("line_edge_negative", put("line_edges", 2, -1), E_ARG, "a line names an edge object that does not exist"),
    ("path_edge_E", put("path_edges", 0, 12), E_ARG, "a path names an edge object that does not exist"),
    ("even_number_of_cells", lines_of(lambda n: n[-1].pop()), E_ARG, "a line with an even number of cells"),
    ("odd_n_paths", field("n_paths", 19), E_ARG, "n_paths is odd: reads r and r ^ 1 are mates"),
    ("inv_not_an_involution", put("inv", 0, 0), E_ARG, "inv is not an involution: inv[inv[e]] != e"),
    ("inv_out_of_range", put("inv", 3, 12), E_ARG, "inv names an edge object that does not exist"),
    ("edge_in_no_line", lines_of(lambda n: n.pop(0)), E_ARG, "an edge object that belongs to no line"),
    ("even_cell_first_path_empty", lines_of(lambda n: n.append([[[5]], [[4]], [[], [5]], [[4]], [[5]]])), E_ARG, "an even cell whose first path is empty"),
    ("edge_shorter_than_K", put("edge_len", 4, 19), E_ARG, "an edge object shorter than K bases"),
    ("line_of_2_31_kmers", long_line, E_LIMIT, "a line of 2^31 K-mers or more"),
    ("null_inv", field("inv", None), E_ARG, "null graph array"),
    ("unknown_flag", field("flags", 8), E_ARG, "unknown flag"),
    ("K_15", field("K", 15), E_ARG, "K must be in [16, 640]"),
    ("unknown_long_form", field("long_form", 3), E_ARG, "unknown long_form"),
    ("negative_frac", field("frac", -0.5), E_ARG, "frac and min_edge_size must not be negative"),
    ("nan_frac", field("frac", float("nan")), E_ARG, "frac and min_edge_size must not be negative"),
    ("negative_min_edge_size", field("min_edge_size", -1), E_ARG, "frac and min_edge_size must not be negative"),
]
NOT_IN_PROGRAM = ("negative_frac", "nan_frac", "unknown_long_form")         # (the stand-alone program passes frac 0.1 and long_form 0)


def mutated(name):
    d = base()
    next(m for n, m, *_ in CASES if n == name)(d)
    return d


@pytest.mark.parametrize("name,code,msg", [(n, c, m) for n, _, c, m in CASES])
def test_refused_before_the_device_is_touched(name, code, msg):
    assert call(mutated(name)) == (code, msg)


def _block(name, d, llens=(), npairs=()):
    out = [f"case {name}"]
    for k, v in {**sizes(d), "K": d["K"], "flags": d["flags"], "min_edge_size": d["min_edge_size"]}.items():
        out.append(f"s {k} {int(v)}")
    for k in ARRAYS:
        out.append(f"a {k} null" if d[k] is None else f"a {k} {len(d[k])} " + " ".join(str(int(x)) for x in d[k]))
    for k, v in (("llens", llens), ("npairs", npairs)):
        out.append(f"a {k} {len(v)} " + " ".join(str(int(x)) for x in v))
    return "\n".join(out + ["end"])


def test_the_host_half_under_a_host_sanitizer(tmp_path):
    exe = str(tmp_path / "step7_cov")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "step7_cov_main.cc")],
                   check=True, capture_output=True, text=True)
    refused = [n for n, *_ in CASES if n not in NOT_IN_PROGRAM]
    blocks = [_block(n, mutated(n)) for n in refused]
    want = {n: (c, m) for n, _, c, m in CASES if n in refused}
    # the peak-finder cases: every recorded case on its recorded lines, every model-only case
    runs = {}
    rec = CC.recorded(tmp_path)
    for name, (case, r) in rec.items():
        runs["rec_" + name] = (case, r["lines"].nested())
    for name, case in CC.model_cases().items():
        runs["mod_" + name] = (case, case["nested"])
    for name, (case, nested) in runs.items():
        m = M.run(case["hbv"], case["inv"], case["paths"], nested)
        blocks.append(_block(name, as_input(case, nested), m["llens"], m["npairs"]))
        bits = struct.unpack("<Q", struct.pack("<d", m["base_cov"]))[0]
        want[name] = (0, f"{bits:016x} {m['counters']['peak_way']} {len(m['covx'])} {len(m['groups'])} {sum(len(g['z']) for g in m['groups'])}")
    r = subprocess.run([exe], input="\n".join(blocks) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        name, code, *msg = line.split(" ", 2)
        got[name] = (int(code), msg[0] if msg else "")
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}

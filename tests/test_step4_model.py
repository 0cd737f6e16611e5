"""The CPU restatement of Step 4 (tests/step4_model.py) against recorded runs of the unmodified reference, byte for byte; and the parts
of the Step-4 interface that need no GPU (errors, exported names, struct sizes, the tool's input checks)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import step4_cases as S
import step4_model as M
from conftest import GOLDEN, ROOT
from w2rap_contigger_amd import formats as F, step2, step4


def _model(name, min_size, **kw):
    h, paths, (pk, bo, ln), quals = S.load(name)
    return M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), min_size, **kw)


@pytest.mark.parametrize("name,min_size", S.CASES)
def test_model_reproduces_the_reference(name, min_size, tmp_path):
    d = str(tmp_path)
    S.reference_run(name, min_size, d)
    m = _model(name, min_size)
    assert F.hbv_to_bytes(m.hbv, zero_padding=True) == F.hbv_to_bytes(F.read_hbv(os.path.join(d, "t.large_K.clean.hbv")), zero_padding=True)
    assert F.paths_to_bytes(m.path_offset, m.path_off, m.path_edges) == open(os.path.join(d, "t.large_K.clean.paths"), "rb").read()


def test_fixtures_exercise_the_step(tmp_path):
    """green must mean something: the vote deletes edges in two fixtures, pass 2 deletes what pass 1 did not expose, a run of three or
    more edges is merged, min_size removes a component -- all read off the recorded reference outputs and the model pinned to them"""
    voted = 0
    for name in ("long_mixed", "errs2"):
        d = str(tmp_path / name); os.makedirs(d)
        S.reference_run(name, 0, d)
        ref = open(os.path.join(d, "t.large_K.clean.hbv"), "rb").read()
        no_vote = _model(name, 0, vote=False)
        assert F.hbv_to_bytes(_model(name, 0).hbv, zero_padding=True) == F.hbv_to_bytes(F.read_hbv(os.path.join(d, "t.large_K.clean.hbv")), zero_padding=True)
        voted += F.hbv_to_bytes(no_vote.hbv, zero_padding=True) != F.hbv_to_bytes(F.read_hbv(os.path.join(d, "t.large_K.clean.hbv")), zero_padding=True)
        assert len(ref) > 0
    assert voted == 2
    m = _model("errs2", 300)
    assert len(m.deleted[1]) > 0, "pass 2 deletes nothing"
    assert len(_model("errs2", 300, vote=False).deleted[0]) < len(m.deleted[0])
    M.RUN_SIZES.clear()
    m0 = _model("errs2", 0)
    assert m0.counters.n_runs_merged[0] > 0 and max(M.RUN_SIZES) >= 3, M.RUN_SIZES
    r = _model("random20k", 300)
    assert len(r.deleted[0]) > 0 and r.hbv.n_edges < S.load("random20k")[0].n_edges


def test_hand_cases_are_what_they_claim():
    hc = S.hand_cases()
    def run(name, **kw):
        h, paths, (pk, bo, ln), quals, ms = hc[name]
        return M.clean200x(h, None, paths, M.reads_of(pk, bo, ln, quals), ms, **kw)
    assert len(run("weak_branch").deleted[0]) == 2
    assert run("contested_branch_kept").deleted[0] == [] and run("contested_branch_kept").counters.n_placements > 0
    assert len(run("dead_end_lowers_depth").deleted[0]) == 2
    s = run("eleven_walks_skipped")
    assert s.counters.n_skipped_too_many_exts >= 1 and s.deleted[0] == []
    assert run("ten_walks_voted").counters.n_skipped_too_many_exts == 0 and len(run("ten_walks_voted").deleted[0]) == 2
    assert len(run("reverse_strand_only").deleted[0]) == 2
    assert len(run("edge_twice").deleted[0]) == 2
    assert run("circle").counters.n_runs_merged[0] >= 2
    assert run("offset_moves_in_run").counters.n_runs_merged[0] == 2
    p2 = run("pass2_exposes")
    assert len(p2.deleted[0]) == 10 and len(p2.deleted[1]) == 2 and p2.counters.n_skipped_too_many_exts == 1, (p2.deleted, p2.counters)
    assert run("no_reads").deleted == [[], []]
    assert len(run("no_branches_min_size").deleted[0]) == 2


# ------------------------------------------------------------------------------------------------------------- interface, no GPU
def _declared():
    text = open(os.path.join(ROOT, "include", "w2rap_step4.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(w2rap_step4_[a-z0-9_]+)\s*\(", text))


def test_header_names_are_the_exported_ones():
    assert _declared() == {"w2rap_step4_run", "w2rap_step4_free", "w2rap_step4_profile"}
    lib = step2.lib()
    for n in _declared():
        assert hasattr(lib, n), f"libw2rap_step2.so does not export {n}"
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "w2rap_contigger_amd", "libw2rap_step2.so")], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(w2rap_step4_\w+)", out)) == _declared()


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "w2rap_step4.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(w2rap_step4_in), sizeof(w2rap_step4_params), sizeof(w2rap_step4_out));return 0;}\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(step4.Step4In), C.sizeof(step4.Step4Params), C.sizeof(step4.Step4Out)] == [176, 12, 264]


def test_errors_without_a_gpu():
    h, paths, (pk, bo, ln), quals = S.load("random20k")
    with pytest.raises(step2.Step2Error) as e:                 # argument errors come before the device is touched
        step4.clean200x(h, paths, pk, bo, ln[:-1], quals)
    assert e.value.code == 1
    bad = (paths[0], paths[1], np.where(paths[2] == 0, h.n_edges, paths[2]).astype(np.int32))
    with pytest.raises(step2.Step2Error) as e:
        step4.clean200x(h, bad, pk, bo, ln, quals)
    assert e.value.code == 1 and "edge object" in str(e.value)
    with pytest.raises(step2.Step2Error) as e:
        step4.clean200x(h, paths, pk, bo, ln, quals, inv=np.zeros(h.n_edges, np.int32))
    assert e.value.code == 1
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(step2.Step2Error) as e:
        step4.clean200x(h, paths, pk, bo, ln, quals)
    assert e.value.code == 2 and "no CPU fallback" in str(e.value)


def test_step4_tool_rejects_truncated_inputs(tmp_path):
    exe = os.path.join(ROOT, "w2rap_contigger_amd", "w2rap-step4")
    d = str(tmp_path)
    files = {f: open(os.path.join(d, f), "rb").read() for f in (S.stage("palindrome_circle", d) or S.INPUTS)}
    hb = files["t.large_K.hbv"]
    for f, blob, what in (("t.large_K.hbv", hb[: len(hb) // 2], "truncated"), ("t.large_K.hbv", b"NOTANHBV" + hb[8:], "BINWRITE"),
                          ("t.large_K.paths", files["t.large_K.paths"][:-3], "truncated"),
                          ("frag_reads_orig.fastb", files["frag_reads_orig.fastb"][: len(files["frag_reads_orig.fastb"]) // 2], "feudal"),
                          ("frag_reads_orig.qualp", files["frag_reads_orig.qualp"][: len(files["frag_reads_orig.qualp"]) // 2], "feudal")):
        for g, b in files.items():
            open(os.path.join(d, g), "wb").write(blob if g == f else b)
        r = subprocess.run([exe, "-o", d, "-p", "t"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and what in r.stderr, (f, r.stderr)

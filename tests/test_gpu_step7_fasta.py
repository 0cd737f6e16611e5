"""w2rap_step7_line_files on the GPU: the recorded runs of the reference's main (tests/golden/refruns/step7_ff_*) byte for byte, and the
model (tests/step7_fasta_model.py) array for array -- cov, best, both shares, printed and every counter -- on the recorded and the
model-only cases, all parts in one call and each part on its own.  Also step7.sort_lines, the stats file and the command line."""
import os

import numpy as np
import pytest

import step7_fasta_cases as C
import step7_fasta_model as M
from w2rap_contigger_amd import formats as F, step7

pytestmark = pytest.mark.gpu

RECORDED = sorted(C.recorded_cases())
MODEL_ONLY = sorted(C.model_cases())
ALONE = ("bubble", "tie_20", "efasta_shares", "circular", "gap_2", "generated_21")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return C.recorded(tmp_path_factory.mktemp("ff"))


@pytest.fixture(scope="module")
def model_cases():
    return C.model_cases()


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_files_byte_for_byte(records, name):
    case, kind, rec = records[name]
    hbv, inv, paths, lines = C.inputs_of(name, case, kind, rec)
    got = C.as_dict(step7.line_files(hbv, inv, paths, lines))
    for k in ("fasta", "efasta", "src"):
        assert got[k] == rec[k], k
    C.compare(got, M.run(hbv, inv, paths, lines.nested(), recorded_fasta=rec["fasta"]))
    llens = step7.line_stats(hbv, inv, paths, lines).llens
    assert step7.stats_text(llens, hbv.K, "t_assembly").encode() == rec["stats"]


@pytest.mark.parametrize("name", ALONE)
@pytest.mark.parametrize("part", ("fasta", "efasta", "src"))
def test_each_part_on_its_own(records, name, part):
    case, kind, rec = records[name]
    hbv, inv, paths, lines = C.inputs_of(name, case, kind, rec)
    res = step7.line_files(hbv, inv, paths, lines, parts=(part,))
    got = C.as_dict(res)
    assert got[part] == rec[part] and all(got[k] is None for k in ("fasta", "efasta", "src") if k != part)
    C.compare(got, M.run(hbv, inv, paths, lines.nested(), parts=(part,), recorded_fasta=rec["fasta"]))
    names = set(step7.profile(line_files=True))
    if part != "fasta":
        assert res.ms["ms_vote"] == 0 and "k7f_vote" not in names and "k5o_index_emit" not in names
    if part != "efasta":
        assert res.ms["ms_share"] == 0 and "k7f_share" not in names
    if part == "src":
        assert not names


@pytest.mark.parametrize("name", MODEL_ONLY)
def test_model_only_cases(model_cases, name):
    case = model_cases[name]
    got = C.as_dict(step7.line_files(case["hbv"], case["inv"], case["paths"], case["lines"]))
    C.compare(got, M.run(case["hbv"], case["inv"], case["paths"], case["nested"]))
    C.check_expect(case, got)


@pytest.mark.parametrize("name", ("bubble", "entries", "generated_22"))
def test_sort_lines(records, name):
    case, kind, rec = records[name]
    nested = rec["lines"].nested()
    order = np.random.default_rng(len(name)).permutation(len(nested))
    got = step7.sort_lines(case["hbv"], case["inv"], F.Lines.from_nested([nested[i] for i in order]))
    assert got.nested() == nested


def test_command_line(records, tmp_path):
    case, kind, rec = records["generated_21"]
    d = str(tmp_path)
    F.write_hbv(os.path.join(d, "t.contig.hbv"), case["hbv"]); F.write_paths(os.path.join(d, "t.contig.paths"), *case["paths"])
    F.write_lines(os.path.join(d, "t_assembly.lines"), rec["lines"])
    assert step7.main([d, "t", "--line_files", os.path.join(d, "t_assembly.lines")]) == 0
    for f, k in (("a.lines.fasta", "fasta"), ("a.lines.efasta", "efasta"), ("a.lines.src", "src")):
        assert open(os.path.join(d, f), "rb").read() == rec[k], f
    assert open(os.path.join(d, "stats"), "rb").read() == rec["stats"].replace(b"# t_assembly ", b"# t ")

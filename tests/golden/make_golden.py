#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running the REAL reference
Step 2 (oracle/_ref/ref_step2, built from /root/reference by oracle/Makefile).

Run in the build container only (the reference does not travel):
    python tests/golden/make_golden.py

For every fixture <name> this writes
    <name>.fastb / <name>.qualp      inputs in the reference's own Step-1 output format
    <name>.ref.hbv / <name>.ref.paths / <name>.ref.freqs
                                      the reference's Step-2 outputs (-t 1, deterministic)
    <name>.ref8.hbv / <name>.ref8.paths   the same with 8 threads (different edge order)
and, from the REAL reference Step 3 (oracle/_ref/ref_step3, K2 = 200) run on those Step-2 outputs,
    <name>.ref.large_K.hbv / .paths / <name>.ref.frags.dist      (1 thread, from <name>.ref.*)
    <name>.ref8.large_K.hbv / .paths                              (8 threads, from <name>.ref8.*)
and, for Step 1 (fastq ingest), step1_r1.fastq / step1_r2.fastq with the REAL reference's frag_reads_orig.fastb/.qualp for them
(step1.ref.fastb / step1.ref.qualp, from oracle/_ref/ref_step1; `make_golden.py step1`).
and, from the REAL reference hbv2gfa tool (oracle/_ref/ref_hbv2gfa -g 20; `make_golden.py gfa`), for the graphs named in GFA_GOLDENS
    <graph>.ref_raw.gfa and <graph>.ref_gfa_stats.txt (its stdout between "=== Graph stats === " and "Dumping gfa"),
and (`make_golden.py refruns`) refruns/<case>/: the files and stdout of every reference run the tests make, with the SHA-256 of its inputs.
For Step 3 (`make_golden.py refruns tests/test_step3_oracle.py`, oracle/_ref/ref_step3 at 1 thread: t.large_K.hbv, t.large_K.paths and, for the
cases of tests/step3_cases.py, t.first.frags.dist) these are: step3_<fixture>_K<K2>[_extend] (Step-2 fixtures at other K2 and with
--extend_paths), step3_case_<name>_K<K2> (circle, palindrome, chains), step3_mix_K<K2> (one graph at each of the 33 large K the reference
runs), step3_fragdist_K200 (FragDist's bounds), step3_joined_K<K2>_extend (--extend_paths on a graph with its true adjacency) and
step3_counts_<U>_<N2>_K100 (launch sizes).  ref_step3 runs every loop of the reference on one thread, so the cases of tests/step3_cases.py
are reproduced byte for byte; the step3_<fixture>_* records were made when the reference's own worklists still took every processor, which
numbers the large-K edges differently from run to run: they stay as recorded (the tests replay whatever order a record has).
For Step 7 (`make_golden.py refruns tests/test_step7_model.py`): step7_s6_<fixture> and step7_s7_<case> (the reference's main) and
step7_fn_<case> (oracle/_ref/ref_step7 lines and gaps on every case of tests/step7_cases.py, at 1 thread and at 4: t.lines.txt, t.gaps.txt,
t.verbose.txt).
All of these are data (inputs and expected outputs); no reference source is stored.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from w2rap_contigger_amd import formats as F, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

FIXTURES = {
    # name: (genome kind, genome seed, read pairs, read seed, with hand-made edge-case reads)
    "random20k": ("random", 11, 2000, 101, True),
    "repeats_snps": ("repeats_snps", 12, 6000, 102, False),
    "palindrome_circle": ("palindrome_circle", 13, 2300, 103, False),
    "long_mixed": ("long_mixed", 0, 0, 0, False),               # (long_mixed_inputs; not in conftest.FIXTURES: its tests name it)
}


def long_mixed_inputs():
    """PE250 on a small diploid genome (repeats, SNPs, a stretch of dense SNPs, short-period tandem arrays) plus 40 reads of 300 to
    3,000 bases and two of ~20 k from the same genome: the oracle pinned on reads far longer than PE150 / 251 (`make_golden.py long_mixed`)"""
    contigs = synth.diploid_genome(24_000, 21, snp_every=300, dense=(3_000, 6_000, 70), tandem=((9_000, 6, 600), (15_000, 13, 800)))
    extra = list(np.random.default_rng(22).integers(300, 3_001, 40)) + [20_000, 19_500]
    return synth.read_length_workload(contigs, 1_500, 23, read_len=250, insert=500, extra_lengths=extra)


def make_inputs(kind, gseed, n_pairs, rseed, edge_cases):
    if kind == "long_mixed":
        return long_mixed_inputs()
    contigs = synth.fixture_genome(kind, gseed)
    codes, quals = synth.sample_reads(contigs, n_pairs, rseed)
    codes, quals = codes.numpy(), quals.numpy()
    reads = [(codes[i], quals[i]) for i in range(len(codes))]
    if edge_cases:
        reads += synth.edge_case_reads(np.random.default_rng(rseed + 1), contigs[0])
    lens = np.array([len(r[0]) for r in reads], dtype=np.uint64)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return np.concatenate([r[0] for r in reads]), np.concatenate([r[1] for r in reads]), off


def step3_goldens(name):
    from oracle import oracle3 as O3
    for threads, tag in ((1, "ref"), (8, "ref8")):
        with tempfile.TemporaryDirectory() as d:
            shutil.copy(os.path.join(HERE, f"{name}.{tag}.hbv"), os.path.join(d, "t.small_K.hbv"))
            shutil.copy(os.path.join(HERE, f"{name}.{tag}.paths"), os.path.join(d, "t.small_K.paths"))
            O3.run_reference3(d, "t", 200, threads)
            shutil.copy(os.path.join(d, "t.large_K.hbv"), os.path.join(HERE, f"{name}.{tag}.large_K.hbv"))
            shutil.copy(os.path.join(d, "t.large_K.paths"), os.path.join(HERE, f"{name}.{tag}.large_K.paths"))
            if threads == 1:
                shutil.copy(os.path.join(d, "t.first.frags.dist"), os.path.join(HERE, f"{name}.ref.frags.dist"))
    if name == "repeats_snps":                 # the reference's --extend_paths (Repath.cc:72-96) on the fixture with junctions
        with tempfile.TemporaryDirectory() as d:
            shutil.copy(os.path.join(HERE, f"{name}.ref.hbv"), os.path.join(d, "t.small_K.hbv"))
            shutil.copy(os.path.join(HERE, f"{name}.ref.paths"), os.path.join(d, "t.small_K.paths"))
            O3.run_reference3(d, "t", 200, 1, extend_paths=True)
            shutil.copy(os.path.join(d, "t.large_K.hbv"), os.path.join(HERE, f"{name}.ext.large_K.hbv"))
            shutil.copy(os.path.join(d, "t.large_K.paths"), os.path.join(HERE, f"{name}.ext.large_K.paths"))


def step1_goldens():
    """step1_r1.fastq / step1_r2.fastq (1000 reads of random20k, its ragged edge-case reads included, half of the Q2 bases written as N)
    and the reference's own Step-1 output for them: step1.ref.fastb / step1.ref.qualp (oracle/_ref/ref_step1)"""
    from oracle import oracle1 as O1
    pk, bo, ln = F.read_fastb(os.path.join(HERE, "random20k.fastb"))
    codes, off = F.unpack_bases(pk, bo, ln)
    quals, _ = F.qualp_to_raw(*F.read_qualp(os.path.join(HERE, "random20k.qualp")))
    off = off.astype(np.int64)
    n = len(ln)
    pick = list(range(0, 598)) + list(range(n - 402, n))
    rng = np.random.default_rng(3)
    L = "ACGT"
    f1, f2 = open(os.path.join(HERE, "step1_r1.fastq"), "w"), open(os.path.join(HERE, "step1_r2.fastq"), "w")
    for j, r in enumerate(pick):
        q = quals[off[r]:off[r + 1]]
        s = "".join(("N" if (qq == 2 and rng.random() < 0.5) else L[c]) for c, qq in zip(codes[off[r]:off[r + 1]], q))
        if j % 7 == 3:
            s = s.lower().replace("n", "N")                      # lower-case bases are legal (Base::char2Val), a lower-case n is not
        (f1 if j % 2 == 0 else f2).write(f"@read{j // 2}/{1 + j % 2} some comment\n{s}\n+\n{''.join(chr(33 + int(x)) for x in q)}\n")
    f1.close(); f2.close()
    with tempfile.TemporaryDirectory() as d:
        for f in ("step1_r1.fastq", "step1_r2.fastq"):
            shutil.copy(os.path.join(HERE, f), os.path.join(d, f))
        O1.run_reference1(d, "step1_r1.fastq,step1_r2.fastq", 1)
        shutil.copy(os.path.join(d, "frag_reads_orig.fastb"), os.path.join(HERE, "step1.ref.fastb"))
        shutil.copy(os.path.join(d, "frag_reads_orig.qualp"), os.path.join(HERE, "step1.ref.qualp"))


GFA_GOLDENS = ("palindrome_circle.ref", "repeats_snps.ref", "repeats_snps.ref.large_K")


def gfa_goldens():
    from oracle import oracle_gfa as OG
    for g in GFA_GOLDENS:
        with tempfile.TemporaryDirectory() as d:
            shutil.copy(os.path.join(HERE, g + ".hbv"), os.path.join(d, "g.hbv"))
            shutil.copy(os.path.join(HERE, g + ".paths"), os.path.join(d, "g.paths"))
            txt, gfa = OG.run_reference_gfa(d, "g", "o", 20)
        open(os.path.join(HERE, g + ".ref_raw.gfa"), "wb").write(gfa)
        open(os.path.join(HERE, g + ".ref_gfa_stats.txt"), "w").write(txt.split("=== Graph stats === \n")[1].split("Dumping gfa")[0])


# the tests whose reference runs are replayed from refruns/<case>/ (conftest.reference_outputs)
REFRUN_TESTS = ("tests/test_step3_consumer.py", "tests/test_step3_oracle.py", "tests/test_gfa_oracle.py", "tests/test_step1_oracle.py",
                "tests/test_step5_reference.py", "tests/test_step4_model.py", "tests/test_gfa_cases.py", "tests/test_step5_add_model.py", "tests/test_step7_model.py")


def refruns(tests=()):
    """runs those tests with W2RAP_RECORD_REFERENCE=1: every reference run they make is done live and recorded.  `make_golden.py refruns
    <test file> ...` records the runs of the files named only and leaves every other case as it is"""
    import subprocess
    if not tests:
        shutil.rmtree(os.path.join(HERE, "refruns"), ignore_errors=True)
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", *(tests or REFRUN_TESTS)], cwd=ROOT,
                          env=dict(os.environ, W2RAP_RECORD_REFERENCE="1"))


def main():
    O.build(ref=True)
    if len(sys.argv) > 1 and sys.argv[1] == "refruns":
        return refruns(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "gfa":
        return gfa_goldens()
    if len(sys.argv) > 1 and sys.argv[1] == "step1":
        return step1_goldens()
    if len(sys.argv) > 1 and sys.argv[1] == "step3":          # only the Step-3 goldens, from the committed Step-2 ones
        for name in FIXTURES:
            step3_goldens(name)
        return
    names = list(FIXTURES)
    if len(sys.argv) > 1 and sys.argv[1] in FIXTURES:           # one fixture only
        names = [sys.argv[1]]
    for name in names:
        codes, quals, off = make_inputs(*FIXTURES[name])
        fastb, qualp = os.path.join(HERE, name + ".fastb"), os.path.join(HERE, name + ".qualp")
        F.write_fastb(fastb, *F.pack_bases(codes, off))
        F.write_qualp(qualp, quals, off)
        for threads, tag in ((1, "ref"), (8, "ref8")):
            with tempfile.TemporaryDirectory() as d:
                shutil.copy(fastb, os.path.join(d, "frag_reads_orig.fastb"))
                shutil.copy(qualp, os.path.join(d, "frag_reads_orig.qualp"))
                secs = O.run_reference(d, "t", threads=threads)
                shutil.copy(os.path.join(d, "t.small_K.hbv"), os.path.join(HERE, f"{name}.{tag}.hbv"))
                shutil.copy(os.path.join(d, "t.small_K.paths"), os.path.join(HERE, f"{name}.{tag}.paths"))
                if threads == 1:
                    shutil.copy(os.path.join(d, "small_K.freqs"), os.path.join(HERE, f"{name}.ref.freqs"))
        print(f"{name}: {len(off) - 1} reads, reference Step 2 took {secs:.2f}s")
        step3_goldens(name)


if __name__ == "__main__":
    main()

"""Runs oracle/_ref/ref_step5 (ref_step5_driver.cc: the reference's own PartnersToEnds, invert, LayoutReads, AddNewStuff, TranslatePaths
and ExtendPath) -- TEST INFRASTRUCTURE
ONLY.  Imported by the case modules of tests/ when a reference run is recorded; the product package never imports it."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REF5_BIN = os.path.join(HERE, "_ref", "ref_step5")


def run_reference5(workdir: str, mode: str, threads: int = 1, timeout: float = 300.0, min_gain: int = 5) -> str:
    """mode "partners": workdir/t.hbv, t.paths, frag_reads_orig.fastb/.qualp -> writes t.out.paths;
    mode "open": workdir/t.hbv, t.paths, frag_reads_orig.fastb, t.inv -> writes t.index.txt and t.layout.txt;
    mode "add": workdir/t.hbv, t.inv, t.paths, frag_reads_orig.fastb/.qualp, new_stuff.fastb -> AddNewStuff(..., min_gain, {}, workdir, 1),
    writes t.out.hbv, t.out.paths and t.out.inv;
    mode "tail": workdir/t.hbv (the new graph), t.map.txt (per old edge: left3, then to3), t.paths, frag_reads_orig.fastb/.qualp ->
    TranslatePaths, then resize(1) and ExtendPath(..., min_gain, False, 1) per read, writes t.out.paths; -> the binary's stdout"""
    assert mode in ("partners", "open", "add", "tail")
    if not os.path.exists(REF5_BIN):
        raise FileNotFoundError(REF5_BIN)
    env = dict(os.environ, OMP_NUM_THREADS=str(threads))
    p = subprocess.run([REF5_BIN, mode, workdir, str(threads)] + ([str(min_gain)] if mode in ("add", "tail") else []), capture_output=True, text=True, env=env, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"ref_step5 {mode} exited with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout

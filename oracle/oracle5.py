"""Runs oracle/_ref/ref_step5 (ref_step5_driver.cc: the reference's own PartnersToEnds, invert and LayoutReads) -- TEST INFRASTRUCTURE
ONLY.  Imported by the case modules of tests/ when a reference run is recorded; the product package never imports it."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REF5_BIN = os.path.join(HERE, "_ref", "ref_step5")


def run_reference5(workdir: str, mode: str, threads: int = 1, timeout: float = 300.0) -> str:
    """mode "partners": workdir/t.hbv, t.paths, frag_reads_orig.fastb/.qualp -> writes t.out.paths;
    mode "open": workdir/t.hbv, t.paths, frag_reads_orig.fastb, t.inv -> writes t.index.txt and t.layout.txt; -> the binary's stdout"""
    assert mode in ("partners", "open")
    if not os.path.exists(REF5_BIN):
        raise FileNotFoundError(REF5_BIN)
    env = dict(os.environ, OMP_NUM_THREADS=str(threads))
    p = subprocess.run([REF5_BIN, mode, workdir, str(threads)], capture_output=True, text=True, env=env, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"ref_step5 {mode} exited with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout

"""What the one-shot entries of Steps 3-5 answer to malformed inputs (tests/arg_error_cases.py): code and message, case by case, equal to
what the library answered before the checks moved into csrc/args.h (tests/golden/arg_errors.json names that commit).  Argument errors
come before the device is touched, so nothing here needs a GPU."""
import json
import os
import subprocess

import pytest

import arg_error_cases as A

RECORDED = json.load(open(A.RECORD))
PAIRS = [(name, e) for name, entries, _, _ in A.CASES for e in entries]
OPAQUE = ("edge_packed", "read_packed", "quals", "path_offset")        # arrays the checks only compare with null


def test_the_record_covers_the_table():
    assert len(RECORDED["recorded_from_commit"]) == 40
    assert {(n, e) for n, per in RECORDED["answers"].items() for e in per} == set(PAIRS)
    assert sum(name.startswith("both_") for name, _, _, _ in A.CASES) >= 8


@pytest.mark.parametrize("name,entry", PAIRS, ids=[f"{n}-{e}" for n, e in PAIRS])
def test_answer_is_the_recorded_one(name, entry):
    code, msg = A.call(entry, A.mutated(name, entry))
    print(name, entry, code, msg)
    assert [code, msg] == RECORDED["answers"][name][entry]
    assert code in (A.E_ARG, A.E_LIMIT)


def _block(name, entry, d):
    out = [f"case {name} {entry}"]
    for k, _ in A._STRUCT[entry]._fields_:                       # the input struct, field by field
        v = d[k]
        if k not in A._DTYPE:
            out.append(f"s {k} {int(v)}")
        elif v is None or k in OPAQUE:
            out.append(f"a {k} {'null' if v is None else 'set'}")
        else:
            out.append(f"a {k} {len(v)} " + " ".join(str(int(x)) for x in v))
    return "\n".join(out + ["end"])


def test_shared_checks_under_a_host_sanitizer(tmp_path):
    """args.h alone, in a stand-alone program built with the address and undefined-behaviour sanitizers: every case of the table whose
    answer comes from a shared piece is refused with the recorded answer, and no check reads past an array on the way."""
    exe = str(tmp_path / "arg_checks")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(A.ROOT, "tests", "arg_checks_main.cc")], check=True, capture_output=True, text=True)
    shared = [(name, e) for name, entries, _, sh in A.CASES if sh for e in entries]
    assert len(shared) > 150
    text = "\n".join(_block(n, e, A.mutated(n, e)) for n, e in shared) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        n, e, code, *msg = line.split(" ")
        got[n, e] = [int(code), " ".join(msg)]
    assert got == {(n, e): RECORDED["answers"][n][e] for n, e in shared}

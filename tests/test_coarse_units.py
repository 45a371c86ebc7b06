"""The work units of the coarse route without a GPU.

One call streams every coarse genome past the candidate list in one launch; its units are numbered top byte -> round ->
genome -> chunk (krisp_amd/csrc/co_units.inc: plain C++ for host and device, called by k_coarse_tables, by k_coarse_probe
and here).  tests/coarse_units_check.cpp is built into a stand-alone program with -fsanitize=address,undefined and run over
seeded tables of 1-5 genomes: every unit number is decoded and held to a brute-force enumeration -- every (byte, round,
genome, key) with candidates exactly once, no unit in a byte without candidates, every key range inside its bucket, and
(top byte, round) monotone over any contiguous split into 1, 3 and 7 workgroups.  The program is never loaded into Python.

Also: the constants the device tests restate are the kernel's."""
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import coarse_stream_cases as SC                                            # noqa: E402

CSRC = os.path.join(ROOT, "krisp_amd", "csrc")


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/coarse_units_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("coarse_units") / "coarse_units_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "coarse_units_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def test_units_against_brute_force(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok 20"                 # 5 genome counts x tcap 1 and 50 x 2 seeds
    seen = {tuple(int(x) for x in re.match(r"G (\d+) tcap (\d+) seed (\d+)", ln).groups()) for ln in lines[:-1]}
    assert seen == {(g, tc, s) for g in range(1, 6) for tc in (1, 50) for s in (0, 1)}
    assert all(int(ln.rsplit(":", 1)[1].split()[0]) > 0 for ln in lines[:-1])


def _define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+(.+?)\s*(//.*)?$", text, re.M)
    assert m, name
    return m.group(1)


def test_constants_restated():
    """what tests/coarse_stream_cases.py restates of the kernel, and what the issue leaves alone"""
    k = open(os.path.join(CSRC, "k_coarse.inc")).read()
    u = open(os.path.join(CSRC, "co_units.inc")).read()
    assert _define(u, "CO_CHUNK") == f"{SC.CC.CO_CHUNK}u"
    assert int(_define(k, "CO_QCAP")) == SC.QCAP
    assert int(_define(k, "CO_T")) * int(_define(k, "CO_UNROLL")) * 2 == SC.ITER
    assert int(_define(k, "CO_HB")) == SC.CC.CO_HB
    assert int(_define(k, "CO_TCAP")) == SC.CC.CO_TCAP
    assert int(_define(k, "CO_MAXG")) == SC.CC.CO_MAXG
    assert '#include "co_units.inc"' in k

"""The index arithmetic of k_gather_items without a GPU.

A workgroup of the kernel gathers the survivors of 64 items; its threads walk the workgroup's OUTPUTS and find each one's
item in the prefix sums of the counts (krisp_amd/csrc/gi_index.inc: plain C++ for host and device, called by the kernel and
here).  tests/gather_index_check.cpp is built into a stand-alone program with -fsanitize=address,undefined and run over
seeded count vectors -- all-zero vectors, one full item (the first, the last, one in between), sparse and dense vectors,
the counts 0, 1, 63, 64, 65 and several hundred, totals above 2^16: every output is held to the enumeration item by item,
entry by entry -- each entry exactly once and in order.  The program is never loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "krisp_amd", "csrc")
KINDS = ("zero", "one", "sparse", "dense", "ones", "edge", "large")


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/gather_index_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("gather_index") / "gather_index_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "gather_index_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def test_every_output_once_and_in_order(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {len(KINDS) * 4}"
    got = {}
    for ln in lines[:-1]:
        m = re.match(r"(\w+) seed (\d+): (\d+) outputs in (\d+) items", ln)
        got[(m.group(1), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)))
    assert set(got) == {(k, s) for k in KINDS for s in range(4)}
    for s in range(4):
        assert got[("zero", s)] == (0, 0)
        assert got[("one", s)][1] == 1 and got[("one", s)][0] >= 1
        assert got[("ones", s)] == (64, 64)
        assert got[("large", s)][0] > 1 << 16


def test_the_kernel_uses_the_include():
    k = open(os.path.join(CSRC, "k_intersect3.inc")).read()
    u = open(os.path.join(CSRC, "gi_index.inc")).read()
    assert '#include "gi_index.inc"' in k and "gi_slot(pre, o)" in k
    assert re.search(r"^#define\s+GI_ITEMS_LOG\s+6\s*$", u, re.M)         # (the 64 items the vectors above have)

"""The per-wave queue of live keys of the two-genome join (krisp_amd/csrc/j2_queue.inc: plain C++ for host and device, called
by k_join2<true> and here) without a GPU.

tests/join2_queue_check.cpp is built into a stand-alone program with -fsanitize=address,undefined and run directly: the places
of a ballot's live lanes against a plain loop (ballots of 0, 1, 63 and 64 lanes, every single lane, seeded random ones; starting
fills 0, 1, 63, 64 and 127), the fill never above the queue, a drain leaving fill - 64, every entry taken exactly once, the
entry's key and base for item keys of 1 to 44 bits and all four bases, and the live rule as one comparison for all bytes.
The program is never loaded into Python.

Also: the kernel includes the file and lays the queues where the include's sizes say."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "krisp_amd", "csrc")


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("join2_queue") / "join2_queue_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "join2_queue_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def test_queue_rules(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(r"ok (\d+)", r.stdout.strip())
    # 5 fills x (7 + 64 + 400) ballots, 200 runs, the entries (five p0, those that leave room for the item key), 256 bytes
    entries = sum(4 * 6 for bits in range(1, 45) for p0 in (2, 10, 12, 20, 31) if p0 + bits <= 64)
    assert m and int(m.group(1)) == 5 * 471 + 200 + entries + 256


def _define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+(.+?)\s*(//.*)?$", text, re.M)
    assert m, name
    return m.group(1)


def test_the_kernel_uses_the_include():
    q = open(os.path.join(CSRC, "j2_queue.inc")).read()
    k = open(os.path.join(CSRC, "k_join2.inc")).read()
    s = open(os.path.join(CSRC, "j2_screen.inc")).read()
    assert '#include "j2_queue.inc"' in k
    drain, cap, bits = (int(_define(q, n).rstrip("u")) for n in ("J2Q_DRAIN", "J2Q_CAP", "J2Q_KEY_BITS"))
    assert (drain, cap, bits) == (64, 128, 44)
    # eight waves' queues are exactly the survivor list lkey[J2_TAB]
    assert cap * 8 == 1 << int(_define(s, "J2_TAB_LOG"))
    for f in ("j2q_place", "j2q_fill_after", "j2q_drains", "j2q_first", "j2q_entry", "j2q_key", "j2q_base"):
        assert f + "(" in k, f
    # no HIP call, no thread index
    for word in ("threadIdx", "blockIdx", "__shared__", "atomic", "hipLaunch", "__builtin_amdgcn_mbcnt", "__builtin_amdgcn_ballot"):
        assert word not in q, word

"""The screen of the two-genome join (krisp_amd/csrc/j2_screen.inc: plain C++ for host and device, called by k_join2 and
here) without a GPU.

tests/join2_screen_check.cpp is built into a stand-alone program with -fsanitize=address,undefined and run directly: the live
rule holds for all 65 536 combinations of a candidate's bases and what other prefixes of its slot add; slot and table hash
stay inside for random and extreme keys at every (p0, sh, mlog) the item plan can produce; they depend on the prefix's bits
inside the item alone.  The program is never loaded into Python.

Also: the constants and the functions tests/join2_cases.py restates are the include's."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import join2_cases as J                                                     # noqa: E402

CSRC = os.path.join(ROOT, "krisp_amd", "csrc")


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("join2_screen") / "join2_screen_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "join2_screen_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def test_screen_rules(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(r"ok (\d+)", r.stdout.strip())
    assert m and int(m.group(1)) > 65536


def _define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+(.+?)\s*(//.*)?$", text, re.M)
    assert m, name
    return m.group(1)


def test_constants_restated():
    s = open(os.path.join(CSRC, "j2_screen.inc")).read()
    k = open(os.path.join(CSRC, "k_join2.inc")).read()
    assert int(_define(s, "J2_SCREEN_LOG")) == J.J2_SCREEN_LOG
    assert int(_define(s, "J2_TAB_LOG")) == J.J2_TAB_LOG
    assert _define(s, "J2_PROBES") == f"{J.J2_PROBES}u"
    for name, ks in (("j2_slot", J.SLOT_K), ("j2_tab_hash", J.TAB_K)):
        m = re.search(name + r"\(uint64_t ik\) \{ return j2_mix\(ik, (0x[0-9A-F]+)u, (0x[0-9A-F]+)u\)", s)
        assert m and (int(m.group(1), 16), int(m.group(2), 16)) == ks, name
    assert '#include "j2_screen.inc"' in k
    h = open(os.path.join(CSRC, "k_intersect3t.inc")).read() + open(os.path.join(CSRC, "k_intersect3.inc")).read()
    assert int(_define(h, "I3T_NB_LOG")) == J.I3T_NB_LOG and _define(h, "I3_SLOTS") == "(4 * I3_MAXT)" and int(_define(h, "I3_MAXT")) * 4 == J.I3_SLOTS


def test_numpy_restatement_of_the_live_rule():
    a, b = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    lv = J.live(a, b)
    for sa in range(16):
        for sb in range(16):
            want = sa != 0 and sb != 0 and bin(sa | sb).count("1") >= 2
            assert bool(lv[sa, sb]) == want


def test_numpy_restatement_of_slot_and_hash(program):
    rng = np.random.default_rng(15)
    iks = [0, 1, (1 << 44) - 1, 1 << 32, (1 << 32) - 1] + [int(x) for x in rng.integers(0, 1 << 44, size=200, dtype=np.uint64)]
    r = subprocess.run([program] + [f"{ik:x}" for ik in iks], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == ""
    got = np.array([[int(x) for x in ln.split()] for ln in r.stdout.strip().split("\n")])
    assert np.array_equal(got[:, 0], J.slot_of(np.array(iks, dtype=np.uint64)))
    assert np.array_equal(got[:, 1], J.tab_hash(np.array(iks, dtype=np.uint64)))

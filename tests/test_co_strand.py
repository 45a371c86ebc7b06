"""One strand of a coarse genome answering for both without a GPU.

krisp_amd/csrc/co_strand.inc is plain C++ for host and device: the digit of a forward key, the forward and the reverse class of a
candidate prefix, the pattern Q(P) and mask_rc of the reverse reading, and the reverse record's key from a forward key -- called by
k_hist8<3>, k_scatter1p<., ., ., 1>, the k_strand_* kernels, k_coarse_probe<1> and here.  tests/co_strand_check.cpp is built into a
stand-alone program with -fsanitize=address,undefined and holds all of them to a base-by-base reverse complement: every (L, 1, R)
the form takes with k <= 9 (R = 0 .. 3) over all 4^k windows; R = 4 and R = 6, which need L > R, at their smallest k -- 10 in
full, 14 on 2^20 seeded windows --; and (25, 1, 2) and (20, 1, 6) on seeded random windows.  The program is never loaded into Python."""
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
    """tests/co_strand_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("co_strand") / "co_strand_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "co_strand_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def test_both_readings_against_a_base_by_base_reverse_complement(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok 14"
    seen = {}
    for ln in lines[:-1]:
        L, R, k, how, n = re.match(r"L (\d+) R (\d+) k (\d+) (all|sampled): (\d+) windows", ln).groups()
        seen[(int(L), int(R))] = (how, int(n), int(k))
    full = {(L, R) for R in range(4) for L in range(5, 9 - R)} | {(5, 4)}
    assert set(seen) == full | {(7, 6), (25, 2), (20, 6)}
    for LR in full:
        how, n, k = seen[LR]
        assert how == "all" and n == 4 ** k and k == LR[0] + 1 + LR[1]
    assert {R for _, R in seen} == {0, 1, 2, 3, 4, 6}
    assert all(seen[LR][0] == "sampled" and seen[LR][1] >= 1 << 18 for LR in ((7, 6), (25, 2), (20, 6)))


def test_one_definition_for_every_caller():
    """the kernels and the host take the digit, the classes and the patterns from co_strand.inc, which has no HIP in it"""
    s = open(os.path.join(CSRC, "co_strand.inc")).read()
    assert not re.search(r"\bhip[A-Z_]\w*|hip_runtime|threadIdx|blockIdx|__shared__|__global__", s)
    assert '#include "co_strand.inc"' in open(os.path.join(CSRC, "krisp_hip.hip")).read()
    for f, names in (("k_sort.inc", ["cs_digit"]), ("k_sort2.inc", ["cs_digit"]),
                     ("k_coarse.inc", ["cs_class_fwd", "cs_class_rev", "cs_pattern_rev", "cs_rev_key", "mask_rc"]),
                     ("h_intersect.inc", ["cs_make"])):
        text = open(os.path.join(CSRC, f)).read()
        for n in names:
            assert n in text, (f, n)

"""One prefilter test per key, one pass per pair of rounds (DESIGN §10b "One test, one pass") without a GPU.

krisp_amd/csrc/co_pass.inc is plain C++ for host and device: M, the bits both readings of a key share; the prefilter word and
bit pair of a hash; the 16-bit slots of a pass's table; which entries make pass p of a digit, and the pass count -- called by
k_strand_tables, k_coarse_probe and here.  tests/co_pass_check.cpp is built into a stand-alone program with
-fsanitize=address,undefined: every (L, 1, R) the one-strand form takes with k <= 9 over all 4^k windows, (25, 1, 2) and (20, 1, 6)
on seeded windows; every slot a pass can hold; the passes of seeded class sizes at KR_COARSE_TCAP 1 / 10 / 50 / 6144 with the switch
on and off.  The program is never loaded into Python."""
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
    """tests/co_pass_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("co_pass") / "co_pass_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "co_pass_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def test_one_hash_serves_both_readings_slots_and_passes(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {len(lines) - 1}"
    seen, passes, slots = {}, {}, None
    for ln in lines[:-1]:
        m = re.match(r"L (\d+) R (\d+) k (\d+) (all|sampled): (\d+) windows", ln)
        if m:
            L, R, k, how, n = m.groups()
            seen[(int(L), int(R))] = (how, int(n), int(k))
            continue
        m = re.match(r"passes tcap (\d+) switch (\d): (\d+) digits, (\d+) passes", ln)
        if m:
            passes[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)))
            continue
        slots = int(re.match(r"slots: (\d+) round trips", ln).group(1))
    full = {(L, R) for R in range(4) for L in range(5, 9 - R)}
    assert set(seen) == full | {(25, 2), (20, 6)}
    for LR in full:
        how, n, k = seen[LR]
        assert how == "all" and n == 4 ** k and k == LR[0] + 1 + LR[1]
    assert all(seen[LR][0] == "sampled" and seen[LR][1] >= 1 << 18 for LR in ((25, 2), (20, 6)))
    assert slots == 4 * 12288
    assert set(passes) == {(t, s) for t in (1, 10, 50, 6144) for s in (0, 1)}
    for t in (1, 10, 50, 6144):
        # the same seeded digits under both settings: sharing a pass takes fewer of them
        assert passes[(t, 0)][0] == passes[(t, 1)][0] >= 100
        assert passes[(t, 1)][1] < passes[(t, 0)][1]


def test_one_definition_for_every_caller():
    """the kernels and the host take the mask, the prefilter bits, the slots and the passes from co_pass.inc, which has no HIP in it"""
    s = open(os.path.join(CSRC, "co_pass.inc")).read()
    assert not re.search(r"\bhip[A-Z_]\w*|hip_runtime|threadIdx|blockIdx|__shared__|__global__", s)
    k = open(os.path.join(CSRC, "k_coarse.inc")).read()
    assert '#include "co_pass.inc"' in k
    for n in ("co_pass_mask", "co_bloom_word", "co_bloom_bits", "co_slot16_home", "co_slot16_tag", "co_slot16_idx", "co_pass_count",
              "co_pass_decode"):
        assert n in k, n
    assert "coarse_pass" in open(os.path.join(CSRC, "h_intersect.inc")).read()

"""The panel pass's step file (krisp_amd/csrc/panel_step.inc: a window's key from bytes, the table's insert and probe, a
primer's codes from its template) without a GPU.  It is plain C++ for host and device; here it is built into a stand-alone
program (tests/panel_step_check.cpp) with -fsanitize=address,undefined, run over exact-size heap buffers on the planted sets
of panel_cases.py and compared with the reference's same-locus verdicts and primer texts.  The program is never loaded into
Python."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import panel_cases as PC                                                    # noqa: E402
import panel_reference as ref                                               # noqa: E402

PLANTED = ["w16", "w15", "w2047", "locus_first_window", "locus_last_window", "locus_reverse_only", "locus_fifteen", "locus_broken_n",
           "locus_poly", "clash_end3", "clash_by2", "clash_and_locus", "one_locus", "primers_10_and_60"]


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/panel_step_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("panel_step") / "panel_step_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "panel_step_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def _run(program, tmp_path, lines):
    path = str(tmp_path / "lines.txt")
    with open(path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    r = subprocess.run([program, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(lines) + 1, (len(out), len(lines))
    return [ln.split(" ") for ln in out[:-1]]


@pytest.mark.parametrize("name", PLANTED)
def test_same_locus_as_the_reference_says(name, program, tmp_path):
    """every ordered pair of a set's templates: the table of the first, the forward windows of the second"""
    t = PC.case(name)["templates"]
    pairs = [(i, j) for i in range(len(t)) for j in range(len(t)) if i != j]
    got = _run(program, tmp_path, [f"locus {t[i]} {t[j]}" for i, j in pairs])
    same = 0
    for (i, j), g in zip(pairs, got):
        want = ref.same_locus(t[i], t[j])
        assert g[0] == "locus" and int(g[1]) == int(want), (name, i, j)
        wi = ref.windows(t[i])
        assert int(g[2]) == len(wi | {ref.rc(w) for w in wi}), (name, i)       # (equal keys share a slot)
        same += want
    print(name, "pairs", len(pairs), "same", same)
    if name == "locus_poly":
        assert [int(g[2]) for g in got[:2]] == [2, 2]                          # (poly-A and poly-T: the key 0 and the flag)


def _key(w):
    k = 0
    for ch in w:
        k = (k << 2) | "ACGT".index(ch)
    return k


def test_keys_and_primer_codes(program, tmp_path):
    lines, want = [], []
    for name in ("locus_broken_n", "w16", "w15", "clash_end3"):
        c = PC.case(name)
        for t, (ls, ln, rs, rn) in zip(c["templates"], c["pairs"]):
            W = len(t)
            for i in list(range(max(W - 15, 0) + 3)) + [W, W + 100, 2147483647]:
                w = t[i:i + 16]
                ok = i + 16 <= W and not set(w) - set("ACGT")
                lines.append(f"keys {t} {i}")
                want.append(["keys", "1", str(_key(w)), str(_key(ref.rc(w)))] if ok else ["keys", "0", "0", "0"])
            if "N" in t:
                continue
            left, right = ref.primers(t, (ls, ln, rs, rn))
            for start, n, rcf, text in ((ls, ln, 0, left), (rs, rn, 1, right)):
                lines.append(f"primer {t} {start} {n} {rcf}")
                want.append(["primer", "".join(str("ACGT".index(ch)) for ch in text), "4", "4"])
            # a primer that does not lie inside the template is all 4, never a read
            lines.append(f"primer {t} {W - 3} 10 0")
            want.append(["primer", "4" * 10, "4", "4"])
            lines.append(f"primer {t} {W + 7} 10 1")
            want.append(["primer", "4" * 10, "4", "4"])
    got = _run(program, tmp_path, lines)
    assert got == want, next((g, w, ln[:60]) for g, w, ln in zip(got, want, lines) if g != w)


def test_the_step_file_is_plain():
    step = open(os.path.join(os.path.dirname(HERE), "krisp_amd", "csrc", "panel_step.inc")).read()
    for word in ("threadIdx", "__shared__", "__global__", "hipLaunch"):
        assert word not in step, word

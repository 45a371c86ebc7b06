"""The per-pair step of the bulged guide-hit pass (--guide-hit-bulges) without a GPU.

krisp_amd/csrc/gbulge_step.inc (the window a seed half fixes, the least distance over the cuts, the canonical cut, the
column mask, the motifs beside the window's real ends, the rule by which one of a row's seed pairs owns it; every index
tested against the text's ends) is plain C++ for host and device.  Here it is built into a stand-alone program
(tests/gbulge_step_check.cpp) with -fsanitize=address,undefined, every report fatal, and run as a child process over
exact-size heap buffers; the program is never loaded into Python.  It plays the scan too: every position, entry and half
is a seed pair exactly when the half lies there within M, so the lists it prints are complete only if the halves are
short enough and every row has exactly one owner.  They are compared with the definition
(guide_bulges_reference.ref_bulge_hits) row for row and field for field: complete lists, nothing skipped."""
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
import guide_bulge_cases as BC                                              # noqa: E402
import guide_bulges_reference as ref                                        # noqa: E402

CSRC = os.path.join(ROOT, "krisp_amd", "csrc")
AROUND = 60                         # bytes kept on either side of a plant's window


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/gbulge_step_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("gbulge_step") / "gbulge_step_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "gbulge_step_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def _run(program, tmp_path, cases):
    """cases: [(text, omit, guides, G, M, B, need, pam5, pam3)] -> per case the program's rows as a HIT array, ordered as
    ref_bulge_hits; a row printed twice (two owners) stays twice"""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for text, omit, guides, G, M, B, need, pam5, pam3 in cases:
            f.write(f"{G} {int(omit)} {len(guides)} {len(text)} {M} {B} {int(need)} {pam5 or '-'} {pam3 or '-'}\n".encode("ascii"))
            f.write("".join(guides).encode("ascii"))
            f.write(bytes(text))
            f.write(b"\n")
    r = subprocess.run([program, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    out, cur = [], []
    for ln in r.stdout.split("\n"):
        if ln.startswith("end "):
            assert int(ln[4:]) == len(out)
            cur.sort()
            out.append(np.array(cur, dtype=ref.HIT) if cur else np.empty(0, dtype=ref.HIT))
            cur = []
        elif ln:
            cur.append(tuple(int(x) for x in ln.split()))
    assert not cur and len(out) == len(cases), (len(out), len(cases))
    return out


def _same(mine, want, what):
    assert len(mine) == len(want), (len(mine), len(want), what)
    for f in ref.FIELDS:
        assert np.array_equal(mine[f], want[f]), (f, what, mine[f][:5].tolist(), want[f][:5].tolist())


@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_step_on_every_short_text(name, program, tmp_path):
    """the empty text, one byte, a text shorter than G - B, a guide's last G - 1 letters at the text's start (the right
    half's window would begin before the text), every bulged window alone (exactly G + b and G - b bytes), one byte short at
    either end, and inside 40 more bytes with M substitutions: every position and entry, omit-soft off and on, need_pam
    off and on -- the definition itself is asked for need_pam here"""
    c = BC.case(name)
    G, M, B, guides, pam5, pam3 = c["G"], c["M"], c["B"], c["guides"], c["pam5"], c["pam3"]
    cases, meta = [], []
    for text, plants in BC.short_texts(name):
        assert ref.comparisons(len(text), guides, B) < BC.MAX_COMPARISONS // 100
        for omit in (0, 1):
            for need in (0, 1):
                cases.append((text, omit, guides, G, M, B, need, pam5, pam3))
                meta.append((text, plants, omit, need))
    got = _run(program, tmp_path, cases)
    rows = 0
    for g, (text, plants, omit, need) in zip(got, meta):
        _same(g, ref.ref_bulge_hits(text, omit, guides, M, B, pam5, pam3, bool(need)), (name, omit, need, bytes(text)[:60]))
        if not need:
            BC.check_plants(plants, g, omit, pam=False)
        if len(text) < G - B:
            assert len(g) == 0
        rows += len(g)
    print(name, "cases", len(cases), "rows", rows)
    assert rows > 0


@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_step_around_every_plant(name, program, tmp_path):
    """[pos - 60, pos + Lw + 60) around every plant: every cut of every bulge on both strands, the straddling cut, seams
    (the slice ends where the text ends), separators, N and lower case in aligned and unpartnered bases, ties of the
    homopolymer and the repeat, the palindrome, equal texts.  need_pam's list is the other's rows with pam = 3"""
    c = BC.case(name)
    G, M, B, guides, pam5, pam3, text = c["G"], c["M"], c["B"], c["guides"], c["pam5"], c["pam3"], c["text"]
    cases, meta = [], []
    for p in c["plants"]:
        pos, _, _, bulge = p["keys"][0]
        lo, hi = max(pos - AROUND, 0), min(pos + G + bulge + AROUND, len(text))
        piece = text[lo:hi]
        for omit in (0, 1):
            for need in (0, 1):
                cases.append((piece, omit, guides, G, M, B, need, pam5, pam3))
            meta.append((piece, p, lo, omit))
    got = _run(program, tmp_path, cases)
    rows = 0
    for i, (piece, p, lo, omit) in enumerate(meta):
        g, kept = got[2 * i], got[2 * i + 1]
        want = ref.ref_bulge_hits(piece, omit, guides, M, B, pam5, pam3)
        _same(g, want, (name, p["kind"], p["keys"][0], omit))
        _same(kept, want[want["pam"] == 3], (name, p["kind"], p["keys"][0], omit, "need_pam"))
        BC.check_plants([p], g, omit, shift=lo)
        rows += len(g)
    print(name, "cases", len(cases), "rows", rows)
    assert rows >= len(meta) // 4


def test_the_step_is_plain_cpp():
    """gbulge_step.inc holds no HIP word: it compiles for the host alone, and nothing in it can stage a tile"""
    step = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "gbulge_step.inc")).read())
    for word in ("hip", "threadIdx", "blockIdx", "__shared__", "__global__", "__syncthreads"):
        assert word not in step, word
    assert "ghit_byte(" in step and "ghit_pam(" in step


@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_cases_plant_what_they_claim(name):
    """a census of a case's plants: every cut of every bulge on both strands, with 0 and with M substitutions; the straddling
    cut; seams whose seed is the first (right half) or last (left half) window of a tile and of a thread, owned by that
    half by the canonical cut the plant's row carries; position 0 and the text's end; the absent kinds"""
    c = BC.case(name)
    G, M, B, plants = c["G"], c["M"], c["B"], c["plants"]
    h = BC.half(G, B)
    assert 2 * h <= G - B + 1 and ref.comparisons(len(c["text"]), c["guides"], B) < BC.MAX_COMPARISONS
    cut = {(p["keys"][0][1], p["keys"][0][3], p["q"]): p for p in plants if p["kind"] == "cut"}
    for strand in (0, 1):
        for b in range(1, B + 1):
            assert all((strand, b, q) in cut for q in range(1, G)) and all((strand, -b, q) in cut for q in range(1, G - b))
    assert {p["subs"] for p in cut.values()} == {0, M}
    if B == 2:
        assert sorted((p["keys"][0][1], p["keys"][0][3], p["q"]) for p in plants if p["kind"] == "straddle") == \
            [(0, -2, G // 2 - 1), (1, -2, G // 2 - 1)]
        assert G // 2 - 1 < G // 2 < G // 2 - 1 + 2                      # the bulge lies in both halves of G / 2 letters
    sides = set()
    for p in plants:
        if not p["kind"].startswith("seam"):
            continue
        (pos, strand, gi, bulge), = p["keys"]
        mm, _, column = p["rows"][0][p["keys"][0]]
        skip = -bulge if bulge < 0 else 0
        q = column if strand == 0 else G - column - skip                     # the canonical cut in the entry's orientation
        if "right" in p["kind"]:
            seed = pos + G + bulge - h
            assert q < h and seed % BC.THREAD == 0 and pos < seed, (p["kind"], q, seed)
        else:
            seed = pos
            assert q >= h and (seed + 1) % BC.THREAD == 0, (p["kind"], q, seed)
        sides.add((p["kind"].split("_")[1], seed % BC.TILE in (0, BC.TILE - 1)))
    assert sides == {("right", True), ("right", False), ("left", True), ("left", False)}
    starts = {p["keys"][0][0] for p in plants}
    assert 0 in starts and any(p["keys"][0][0] + G + p["keys"][0][3] == len(c["text"]) for p in plants)
    kinds = {p["kind"] for p in plants}
    assert {"absent_record_end", "absent_record_start", "absent_N_aligned", "lower_aligned", "absent_N_unpartnered",
            "absent_separator_unpartnered", "lower_unpartnered", "homopolymer"} <= kinds
    assert ("palindrome" in kinds) == (G % 2 == 0) and ("equal_texts" in kinds) == (G in (20, 21))

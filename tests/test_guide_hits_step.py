"""The guide-hit pass (--out_guide_hits) without a GPU.

The per-hit step of the scan (krisp_amd/csrc/ghit_step.inc: the window, the column mask in the guide's orientation, both
motifs on both strands, every index tested against the text's ends) is plain C++ for host and device.  Here it is built into
a stand-alone program (tests/ghit_step_check.cpp) with -fsanitize=address,undefined, run over exact-size heap buffers on
every position and entry of short texts and of the surroundings of every plant, and compared field for field with the
definition (guide_hits_reference.ref_hits).  The program is never loaded into Python.

Also: loc_stage_byte and its restatement hold the same lines, the command line's refusals, guide_hits_refusal, the record's
layout and the header's entry points."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from krisp_amd import _native, reports
from krisp_amd import krisp_fasta as KF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import guide_hit_cases as GC                                                # noqa: E402
import guide_hits_reference as ref                                          # noqa: E402

CSRC = os.path.join(ROOT, "krisp_amd", "csrc")
AROUND = 60                         # bytes kept on either side of a plant's window


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/ghit_step_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("ghit_step") / "ghit_step_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "ghit_step_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def _run(program, tmp_path, cases):
    """cases: [(text, omit, guides, G, pam5, pam3)] -> per case the program's tuples as a HIT array, ordered as ref_hits"""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for text, omit, guides, G, pam5, pam3 in cases:
            f.write(f"{G} {int(omit)} {len(guides)} {len(text)} {pam5 or '-'} {pam3 or '-'}\n".encode("ascii"))
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


def _compare(got, text, omit, guides, M, pam5, pam3):
    """the program's tuples (everything within 3), cut to <= M, against the definition without and with need_pam"""
    got = got[got["mismatches"] <= M]
    for need in (False, True):
        want = ref.ref_hits(text, omit, guides, M, pam5, pam3, need)
        mine = got[got["pam"] == 3] if need else got
        assert len(mine) == len(want), (len(mine), len(want), need, omit, M, bytes(text)[:80])
        for f in ref.FIELDS:
            assert np.array_equal(mine[f], want[f]), (f, need, omit, M, mine[f][:5].tolist(), want[f][:5].tolist())
    return got


@pytest.mark.parametrize("name", list(GC.SETS))
def test_the_step_on_every_short_text(name, program, tmp_path):
    """the empty text, one byte, G - 1 bytes (n < G: no window), the guide alone, a window below the motif's length, M
    substitutions: every position, every entry, omit-soft off and on"""
    c0 = GC.case(name, 0)
    G, guides, pam5, pam3 = c0["G"], c0["guides"], c0["pam5"], c0["pam3"]
    cases, meta = [], []
    for M in GC.MS:
        for text, plants in GC.short_texts(name, M):
            assert ref.comparisons(len(text), guides) < GC.MAX_COMPARISONS // 100
            for omit in (0, 1):
                cases.append((text, omit, guides, G, pam5, pam3))
                meta.append((M, text, plants, omit))
    got = _run(program, tmp_path, cases)
    rows = 0
    for g, (M, text, plants, omit) in zip(got, meta):
        mine = _compare(g, text, omit, guides, M, pam5, pam3)
        GC.check_plants(plants, mine, omit)
        if len(text) < G:
            assert len(g) == 0
        rows += len(mine)
    print(name, "cases", len(cases), "rows", rows)
    assert rows > 0


@pytest.mark.parametrize("name", ["g12_long", "g28_tttv", "g40_long"])
def test_the_step_around_every_plant(name, program, tmp_path):
    """[pos - 60, pos + G + 60) around every plant of every distance: tile and thread edges, position 0 and the last window
    (the slice ends where the text ends), separators, N, lower case and IUPAC letters in windows and neighbours, '-'
    neighbours that match only after complementing, the column mask at both ends"""
    cases, meta = [], []
    for M in GC.MS:
        c = GC.case(name, M)
        G, guides, pam5, pam3, text = c["G"], c["guides"], c["pam5"], c["pam3"], c["text"]
        for p in c["plants"]:
            pos = p["rows"][0][0]
            lo, hi = max(pos - AROUND, 0), min(pos + G + AROUND, len(text))
            piece = text[lo:hi]
            assert ref.comparisons(len(piece), guides) < GC.MAX_COMPARISONS // 100
            for omit in (0, 1):
                cases.append((piece, omit, guides, G, pam5, pam3))
                meta.append((M, piece, p, lo, omit))
    got = _run(program, tmp_path, cases)
    rows = 0
    for g, (M, piece, p, lo, omit) in zip(got, meta):
        mine = _compare(g, piece, omit, guides, M, pam5, pam3)       # (a set's guides and motifs are those of every M)
        # the plant's own rows, moved into the slice.  A motif cut by the slice's start instead of the text's reads the same
        # way (outside is bad), so the pinned bits hold wherever the slice keeps every neighbour: AROUND > 8
        moved = dict(p, rows=[(pos - lo, s, gi, mm, mask) for pos, s, gi, mm, mask in p["rows"]])
        GC.check_plants([moved], mine, omit)
        rows += len(mine)
    print(name, "cases", len(cases), "rows", rows)
    assert rows >= len(cases) // 4


def _body(path, name):
    text = open(path).read()
    m = re.search(r"inline (?:u32|uint32_t) " + name + r"\((?:u32|uint32_t) b, (?:u32|uint32_t) omit\) \{\n(.*?)\n\}", text, re.S)
    assert m, name
    return m.group(1)


def test_the_step_stages_bytes_as_the_scans_do():
    """ghit_stage_byte restates loc_stage_byte: the same lines"""
    a = _body(os.path.join(CSRC, "k_scan.inc"), "loc_stage_byte")
    b = _body(os.path.join(CSRC, "ghit_step.inc"), "ghit_stage_byte")
    assert a == b and "'\\n'" in a and a.count("\n") == 2
    step = open(os.path.join(CSRC, "ghit_step.inc")).read()
    for word in ("hip", "threadIdx", "__shared__", "__global__"):
        assert word not in re.sub(r"//[^\n]*", "", step), word


# ----------------------------------------------------------------------------
# the command line, the driver's refusal, the record
# ----------------------------------------------------------------------------
NOWHERE = ["/nonexistent/in0.fa", "/nonexistent/in1.fa", "--outgroup", "/nonexistent/out0.fa", "-c", "30", "-d", "40"]


@pytest.mark.parametrize("flags, word", [
    (["--out_guide_hits", "h.tsv"], "--out_guide_hits needs --out_guides"),
    (["--guide-hit-mismatches", "1"], "--guide-hit-mismatches needs --out_guide_hits"),
    (["--out_guides", "g.tsv", "--guide-hit-mismatches", "1"], "--guide-hit-mismatches needs --out_guide_hits"),
    (["--guide-hits-need-pam"], "--guide-hits-need-pam needs --out_guide_hits"),
    (["--out_guides", "g.tsv", "--pam5", "TTTV", "--guide-hits-need-pam"], "--guide-hits-need-pam needs --out_guide_hits"),
    (["--out_guides", "g.tsv", "--out_guide_hits", "h.tsv", "--guide-hits-need-pam"], "needs a motif"),
    (["--out_guides", "g.tsv", "--out_guide_hits", "h.tsv", "--guide-hit-mismatches", "4"], "between 0 and 3"),
    (["--out_guides", "g.tsv", "--out_guide_hits", "h.tsv", "--guide-hit-mismatches", "-1"], "between 0 and 3"),
])
def test_the_command_line_refuses_before_it_reads(flags, word, tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        KF.main(NOWHERE + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert word in err and "ERROR" in err
    assert os.listdir(tmp_path) == []


def test_the_options_parse_and_need_pam_takes_either_motif():
    p = KF.build_parser()
    a = p.parse_args(NOWHERE + ["--out_guides", "g", "--out_guide_hits", "h"])
    assert a.out_guide_hits == "h" and a.guide_hit_mismatches is None and a.guide_hits_need_pam is False
    assert KF.guide_hits_refusal(28, 2, "TTTV", "", True) is None and KF.guide_hits_refusal(28, 2, "", "H", True) is None


def test_guide_hits_refusal_on_its_bounds():
    ok = KF.guide_hits_refusal
    assert ok(12, 0, "", "", False) is None and ok(40, 3, "NNNNTTTV", "HNNNNNNN", True) is None
    assert "--guide-size" in ok(11, 2, "", "", False) and "--guide-size" in ok(41, 2, "", "", False)
    assert "--guide-hit-mismatches" in ok(28, -1, "", "", False) and "--guide-hit-mismatches" in ok(28, 4, "", "", False)
    assert "--pam5" in ok(28, 2, "NNNNNTTTV", "", False) and "--pam3" in ok(28, 2, "", "HNNNNNNNN", False)
    assert "--pam5" in ok(28, 2, "TTJ", "", False) and "--pam3" in ok(28, 2, "", "X", False)
    assert "needs a motif" in ok(28, 2, "", "", True)
    for bad in ((11, 2, "", "", False), (28, 4, "", "", False), (28, 2, "TTJ", "", False), (28, 2, "", "", True)):
        with pytest.raises(ValueError):
            KF.guide_hits([b"A" * bad[0]], [[0]], ["/nonexistent/in0.fa"], [], *bad)
    # no text: no row, no file opened
    assert len(KF.guide_hits([], [], ["/nonexistent/in0.fa"], [], 28)) == 0
    with pytest.raises(ValueError):
        KF.guide_hits([b"ACGT" * 7], [[0], [1]], ["/nonexistent/in0.fa"], [], 28)


def test_the_record_and_the_header():
    d = _native.GUIDE_HIT_RAW
    assert d.itemsize == 24
    assert [(n, d.fields[n][1]) for n in d.names] == [("guide", 0), ("strand", 4), ("mismatches", 5), ("pam", 6), ("pad", 7),
                                                      ("pos", 8), ("columns", 16)]
    header = open(os.path.join(ROOT, "include", "krisp_hip.h")).read()
    bound = {n for n, _, _ in _native.SYMBOLS}
    for name in ("kr_guide_hits_table", "kr_guide_hits_scan", "kr_guide_hits_fetch", "kr_guide_hits_windows"):
        assert re.search(r"\bint64_t " + name + r"\(kr_ctx\*", header), name
        assert name in bound
    assert re.search(r"typedef struct \{ uint32_t guide; uint8_t strand, mismatches, pam, pad; uint64_t pos; uint64_t columns; \} "
                     r"kr_guide_hit;", header)
    for m in ("guide_hits_table", "guide_hits", "guide_hit_windows"):
        assert callable(getattr(_native.Engine, m))


def test_a_hit_of_a_shared_text_is_a_row_for_each_region_in_the_file_order(monkeypatch):
    """guide_hits over a stand-in for the scan: two files, text 0 shared by regions 4 and 1, text 1 of region 2; the rows
    come by (region, file, record_index, start, '+' before '-') and carry the mask's columns, the motif bits, U for T"""
    G = 12
    texts, text_regions = [b"ACGTACGTACGT", b"TTTTCCCCGGGG"], [[1, 4], [2]]
    raw = {"a.fa": [(0, 1, 0, 0, 1, 30), (1, 0, 2, (1 << 0) | (1 << 11), 3, 5)], "b.fa": [(0, 0, 1, 1 << 3, 2, 2), (0, 1, 1, 1 << 3, 3, 2)]}
    seen = {}

    class Eng:
        def __init__(self, path):
            self.path = path

        def guide_hits_table(self, t, M, pam5, pam3, need):
            seen["table"] = (bytes(t.tobytes()), M, pam5, pam3, need)

        def guide_hits(self, gid):
            hits = np.zeros(len(raw[self.path]), dtype=_native.GUIDE_HIT_RAW)
            for i, (g, s, mm, cols, pam, pos) in enumerate(raw[self.path]):
                hits[i] = (g, s, mm, pam, 0, pos, cols)
            return hits

        def guide_hit_windows(self, k):
            return np.full((len(raw[self.path]), k), ord("T"), dtype=np.uint8)

    def scan(files, Le, De, Re, k, omit_soft, device, table):
        assert (Le, De, Re, k) == (0, G, 0, G)
        for fi, path in enumerate(files):
            eng = Eng(path)
            if fi == 0:
                table(eng)
            yield eng, fi, path, path == "b.fa", lambda: (np.array([20], dtype=np.int64), ["r0", "r1"])

    monkeypatch.setattr(reports, "_scan_genomes", scan)
    rows = KF.guide_hits(texts, text_regions, ["a.fa"], ["b.fa"], G, mismatches=2, pam5="TTTV", need_pam=True)
    assert seen["table"] == (b"".join(texts), 2, "TTTV", "", True)
    got = [(int(r["region"]), r["file"], r["record"], int(r["record_index"]), int(r["start"]), int(r["end"]), r["strand"],
            int(r["mismatches"]), r["mismatch_columns"], int(r["pam5_match"]), int(r["pam3_match"]), r["sequence"]) for r in rows]
    t, u = "T" * G, "U" * G
    assert got == [(1, "a.fa", "r1", 1, 9, 21, "-", 0, "-", 1, 0, t), (1, "b.fa", "r0", 0, 2, 14, "+", 1, "4", 0, 1, u),
                   (1, "b.fa", "r0", 0, 2, 14, "-", 1, "4", 1, 1, u), (2, "a.fa", "r0", 0, 5, 17, "+", 2, "1,12", 1, 1, t),
                   (4, "a.fa", "r1", 1, 9, 21, "-", 0, "-", 1, 0, t), (4, "b.fa", "r0", 0, 2, 14, "+", 1, "4", 0, 1, u),
                   (4, "b.fa", "r0", 0, 2, 14, "-", 1, "4", 1, 1, u)]

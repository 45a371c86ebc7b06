"""--guide-hit-bulges without a GPU: the command line's refusals, guide_hits_refusal's new keyword, the record's
layout and the header's entry points, guide_bulge_hits over a stand-in for the scan, the merged file."""
import os
import re

import numpy as np
import pytest

from krisp_amd import _native, reports
from krisp_amd import krisp_fasta as KF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOWHERE = ["/nonexistent/in0.fa", "/nonexistent/in1.fa", "--outgroup", "/nonexistent/out0.fa", "-c", "30", "-d", "40"]
HITS = ["--out_guides", "g.tsv", "--out_guide_hits", "h.tsv"]


@pytest.mark.parametrize("flags, word", [
    (["--guide-hit-bulges", "1"], "--guide-hit-bulges needs --out_guide_hits"),
    (["--out_guides", "g.tsv", "--guide-hit-bulges", "1"], "--guide-hit-bulges needs --out_guide_hits"),
    (["--guide-hit-bulges", "0"], "--guide-hit-bulges needs --out_guide_hits"),
    (HITS + ["--guide-hit-bulges", "-1"], "between 0 and 2"),
    (HITS + ["--guide-hit-bulges", "3"], "between 0 and 2"),
    (HITS + ["--guide-size", "19", "--guide-hit-bulges", "1"], "--guide-size >= 20"),
    (HITS + ["--guide-hit-mismatches", "3", "--guide-hit-bulges", "1"], "--guide-hit-mismatches <= 2"),
    (HITS + ["--guide-hit-mismatches", "3", "--guide-hit-bulges", "2"], "half-guide"),
])
def test_the_command_line_refuses_before_it_reads(flags, word, tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        KF.main(NOWHERE + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert word in err and "ERROR" in err
    assert os.listdir(tmp_path) == []


def test_the_option_parses_and_zero_changes_nothing():
    p = KF.build_parser()
    assert p.parse_args(NOWHERE + HITS).guide_hit_bulges is None
    assert p.parse_args(NOWHERE + HITS + ["--guide-hit-bulges", "0"]).guide_hit_bulges == 0
    assert p.parse_args(NOWHERE + HITS + ["--guide-hit-bulges", "2"]).guide_hit_bulges == 2
    ok = KF.guide_hits_refusal
    # today's calls, and the same with bulges = 0: figures the bulged search would refuse pass
    for figures in ((12, 0, "", "", False), (19, 3, "TTTV", "", True), (40, 3, "NNNNTTTV", "HNNNNNNN", True)):
        assert ok(*figures) is None and ok(*figures, bulges=0) is None
    for figures in ((11, 2, "", "", False), (28, 4, "", "", False), (28, 2, "TTJ", "", False), (28, 2, "", "", True)):
        assert ok(*figures) == ok(*figures, bulges=0) and ok(*figures) is not None
    assert ok(20, 2, "", "", False, bulges=1) is None and ok(40, 0, "TTTV", "", True, bulges=2) is None
    assert "--guide-size" in ok(19, 2, "", "", False, bulges=1) and "DESIGN" in ok(19, 2, "", "", False, bulges=2)
    assert "--guide-hit-mismatches" in ok(28, 3, "", "", False, bulges=1)
    assert "--guide-hit-bulges" in ok(28, 2, "", "", False, bulges=3) and "--guide-hit-bulges" in ok(28, 2, "", "", False, bulges=-1)
    assert "--pam5" in ok(28, 2, "TTJ", "", False, bulges=1) and "needs a motif" in ok(28, 2, "", "", True, bulges=1)
    # the file without bulges keeps its header
    assert KF.GUIDE_HIT_HEADER.endswith("\tsequence") and "bulge" not in KF.GUIDE_HIT_HEADER
    assert KF.GUIDE_BULGE_HIT_HEADER == KF.GUIDE_HIT_HEADER + "\tbulge\tbulge_size\tbulge_column"


def test_guide_bulge_hits_refuses_what_the_command_line_does():
    for bad in (dict(guide_size=19), dict(guide_size=28, mismatches=3), dict(guide_size=28, bulges=0), dict(guide_size=28, bulges=3),
                dict(guide_size=28, need_pam=True)):
        G = bad["guide_size"]
        with pytest.raises(ValueError):
            KF.guide_bulge_hits([b"A" * G], [[0]], ["/nonexistent/in0.fa"], [], **bad)
    # no text: no row, no file opened
    assert len(KF.guide_bulge_hits([], [], ["/nonexistent/in0.fa"], [], 28)) == 0
    with pytest.raises(ValueError):
        KF.guide_bulge_hits([b"ACGT" * 7], [[0], [1]], ["/nonexistent/in0.fa"], [], 28)


def test_the_record_and_the_header():
    d = _native.GUIDE_BULGE_HIT_RAW
    assert d.itemsize == 32
    assert [(n, d.fields[n][1], d.fields[n][0].str) for n in d.names] == [
        ("guide", 0, "<u4"), ("strand", 4, "|u1"), ("mismatches", 5, "|u1"), ("pam", 6, "|u1"), ("bulge", 7, "|i1"), ("pos", 8, "<u8"),
        ("columns", 16, "<u8"), ("bulge_column", 24, "<u4"), ("length", 28, "<u4")]
    header = open(os.path.join(ROOT, "include", "krisp_hip.h")).read()
    bound = {n for n, _, _ in _native.SYMBOLS}
    for name in ("kr_guide_bulges_table", "kr_guide_bulges_scan", "kr_guide_bulges_fetch", "kr_guide_bulges_windows"):
        assert re.search(r"\bint64_t " + name + r"\(kr_ctx\*", header), name
        assert name in bound
    assert re.search(r"int64_t kr_guide_bulges_table\(kr_ctx\*, const uint8_t\* texts, uint64_t nguides, int mismatches, int bulges, "
                     r"const char\* pam5,\s+const char\* pam3, int need_pam\);", header)
    assert re.search(r"typedef struct \{ uint32_t guide; uint8_t strand, mismatches, pam; int8_t bulge; uint64_t pos; uint64_t columns;\s+"
                     r"uint32_t bulge_column, length; \} kr_guide_bulge_hit;", header)
    for m in ("guide_bulges_table", "guide_bulges", "guide_bulge_windows"):
        assert callable(getattr(_native.Engine, m))
    # the new sources are part of the one translation unit
    unit = open(os.path.join(ROOT, "krisp_amd", "csrc", "krisp_hip.hip")).read()
    assert '#include "k_guide_bulges.inc"' in unit and '#include "h_guide_bulges.inc"' in unit
    assert '#include "gbulge_step.inc"' in open(os.path.join(ROOT, "krisp_amd", "csrc", "k_guide_bulges.inc")).read()


def _stand_in(monkeypatch, G, B, raw, seen):
    """guide_bulge_hits over a stand-in for the scan: raw[path] = [(guide, strand, mismatches, columns, pam, pos, bulge,
    bulge_column)]"""
    class Eng:
        def __init__(self, path):
            self.path = path

        def guide_bulges_table(self, t, M, bulges, pam5, pam3, need):
            seen["table"] = (bytes(t.tobytes()), M, bulges, pam5, pam3, need)

        def guide_bulges(self, gid):
            hits = np.zeros(len(raw[self.path]), dtype=_native.GUIDE_BULGE_HIT_RAW)
            for i, (g, s, mm, cols, pam, pos, bulge, column) in enumerate(raw[self.path]):
                hits[i] = (g, s, mm, pam, bulge, pos, cols, column, G + bulge)
            return hits

        def guide_bulge_windows(self, width):
            assert width == G + B
            rows = np.zeros((len(raw[self.path]), width), dtype=np.uint8)
            for i, r in enumerate(raw[self.path]):
                rows[i, :G + r[6]] = ord("T")
            return rows

    def scan(files, Le, De, Re, k, omit_soft, device, table):
        assert (Le, De, Re, k) == (0, G, 0, G)
        for fi, path in enumerate(files):
            eng = Eng(path)
            if fi == 0:
                table(eng)
            yield eng, fi, path, path == "b.fa", lambda: (np.array([20], dtype=np.int64), ["r0", "r1"])

    monkeypatch.setattr(reports, "_scan_genomes", scan)


def test_a_bulged_hit_of_a_shared_text_is_a_row_for_each_region_in_the_file_order(monkeypatch):
    """two files, text 0 shared by regions 4 and 1, text 1 of region 2; the rows come by (region, file, record_index, start,
    '+' before '-', end) whatever order the scan lists them in, and carry the aligned columns, the motif bits, the kind, the
    size and the column of the bulge, end = start + G +- b, a sequence of that length, U for T"""
    G, B = 20, 2
    texts, text_regions = [b"ACGTACGTACGTACGTACGT", b"TTTTCCCCGGGGAAAATTTT"], [[1, 4], [2]]
    raw = {"a.fa": [(0, 1, 0, 0, 1, 30, 2, 7), (1, 0, 2, (1 << 0) | (1 << 19), 3, 5, -1, 3), (1, 0, 1, 1 << 4, 3, 5, 1, 18)],
           "b.fa": [(0, 0, 1, 1 << 3, 2, 2, -2, 9), (0, 1, 1, 1 << 3, 3, 2, -2, 9), (0, 0, 0, 0, 3, 2, -1, 1)]}
    seen = {}
    _stand_in(monkeypatch, G, B, raw, seen)
    rows = KF.guide_bulge_hits(texts, text_regions, ["a.fa"], ["b.fa"], G, mismatches=2, bulges=B, pam5="TTTV", need_pam=True)
    assert seen["table"] == (b"".join(texts), 2, B, "TTTV", "", True)
    assert rows.dtype == KF.GUIDE_BULGE_HIT
    got = [(int(r["region"]), r["file"], r["record"], int(r["record_index"]), int(r["start"]), int(r["end"]), r["strand"],
            int(r["mismatches"]), r["mismatch_columns"], int(r["pam5_match"]), int(r["pam3_match"]), r["sequence"], r["bulge"],
            int(r["bulge_size"]), r["bulge_column"]) for r in rows]
    t, u = lambda n: "T" * n, lambda n: "U" * n                             # noqa: E731
    a1 = ("a.fa", "r1", 1, 9, 31, "-", 0, "-", 1, 0, t(22), "DNA", 2, "7")
    b_ = [("b.fa", "r0", 0, 2, 20, "+", 1, "4", 0, 1, u(18), "RNA", 2, "9"), ("b.fa", "r0", 0, 2, 21, "+", 0, "-", 1, 1, u(19), "RNA", 1, "1"),
          ("b.fa", "r0", 0, 2, 20, "-", 1, "4", 1, 1, u(18), "RNA", 2, "9")]
    assert got == [(1,) + a1] + [(1,) + x for x in b_] + [
        (2, "a.fa", "r0", 0, 5, 24, "+", 2, "1,20", 1, 1, t(19), "RNA", 1, "3"),
        (2, "a.fa", "r0", 0, 5, 26, "+", 1, "5", 1, 1, t(21), "DNA", 1, "18")] + [(4,) + a1] + [(4,) + x for x in b_]


def test_the_merged_file_orders_both_row_sets_and_fills_the_three_columns(monkeypatch, tmp_path):
    G, B = 20, 1
    texts, text_regions = [b"ACGTACGTACGTACGTACGT"], [[0, 3]]
    raw = {"a.fa": [(0, 0, 1, 1 << 2, 3, 4, -1, 5), (0, 1, 0, 0, 3, 4, 1, 6), (0, 0, 0, 0, 3, 25, 1, 2)], "b.fa": [(0, 0, 0, 0, 3, 1, 1, 4)]}
    _stand_in(monkeypatch, G, B, raw, {})
    bulged = KF.guide_bulge_hits(texts, text_regions, ["b.fa"], ["a.fa"], G, mismatches=1, bulges=B)
    # the unbulged rows as guide_hits gives them: (region, file in command-line order -- b.fa first --, record_index, start, strand)
    plain = np.empty(6, dtype=KF.GUIDE_HIT)
    some = [("b.fa", "r0", 0, 1, 21, "-", 0, "-", 1, 1, "U" * G), ("a.fa", "r0", 0, 4, 24, "+", 0, "-", 1, 1, "T" * G),
            ("a.fa", "r1", 1, 9, 29, "+", 1, "7", 1, 0, "T" * G)]
    for i, region in enumerate((0, 3)):
        for j, r in enumerate(some):
            plain[3 * i + j] = (region,) + r
    path = str(tmp_path / "hits.tsv")
    KF.write_guide_bulge_hits(path, plain, bulged, ["b.fa", "a.fa"])
    lines = open(path).read().split("\n")
    assert lines[0] == KF.GUIDE_BULGE_HIT_HEADER and lines[-1] == "" and len(lines) == 2 + 6 + 8
    body = [ln.split("\t") for ln in lines[1:-1]]
    per_region = [
        ["b.fa", "r0", "0", "1", "22", "+", "0", "-", "1", "1", "U" * 21, "DNA", "1", "4"],
        ["b.fa", "r0", "0", "1", "21", "-", "0", "-", "1", "1", "U" * 20, "-", "0", "-"],
        ["a.fa", "r0", "0", "4", "23", "+", "1", "3", "1", "1", "T" * 19, "RNA", "1", "5"],
        ["a.fa", "r0", "0", "4", "24", "+", "0", "-", "1", "1", "T" * 20, "-", "0", "-"],
        ["a.fa", "r0", "0", "4", "25", "-", "0", "-", "1", "1", "T" * 21, "DNA", "1", "6"],
        ["a.fa", "r1", "1", "4", "25", "+", "0", "-", "1", "1", "T" * 21, "DNA", "1", "2"],
        ["a.fa", "r1", "1", "9", "29", "+", "1", "7", "1", "0", "T" * 20, "-", "0", "-"]]
    assert body == [[str(region)] + r for region in (0, 3) for r in per_region]
    # the unbulged rows of the merged file are write_guide_hits' lines
    old = str(tmp_path / "old.tsv")
    KF.write_guide_hits(old, plain)
    assert ["\t".join(r[:12]) for r in body if r[12] == "-"] == open(old).read().split("\n")[1:-1]
    assert open(old).read().startswith(KF.GUIDE_HIT_HEADER + "\n")

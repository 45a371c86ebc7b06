"""The host side of the multiplex pass (--out_panel_products, --out_panel_summary) without a GPU: the oligos
against write_panel's sequences, the kinds and the fan-out of a text several oligos share, both files' bytes on hand-made
rows, panel_products_refusal, and the record layout of MULTIPLEX_HIT beside the header."""
import os
import re

import numpy as np
import pytest

from krisp_amd import _native, reports
from krisp_amd import krisp_fasta as KF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _selection():
    """test_panel_host's hand-made selection: three regions, two with a pair, both members"""
    t = np.frombuffer(b"ACGTACGTACGGTTTTCCCCAAAAGGGG" + b"TTGACCATGCAAGGCTTAACCGGTTAAC" + b"GGGGCCCCAAAATTTTACGTACGTACGT",
                      dtype=np.uint8).reshape(3, 28)
    rec = np.zeros(3, dtype=_native.DESIGN_RECORD)
    rec["found"] = [1, 0, 1]
    rec["pair_penalty"] = [2500, 0, 1234]
    rec["product_size"] = [28, 0, 27]
    rec["left_start"], rec["left_len"], rec["right_start"], rec["right_len"] = [0, 0, 1], [10, 0, 11], [18, 0, 17], [10, 0, 11]
    order = KF.panel_candidates(rec)
    members = np.zeros(2, dtype=_native.PANEL_MEMBER)
    members["position"] = [0, 1]
    return t, rec, order, members


def test_the_oligos_are_the_sequences_write_panel_prints(tmp_path):
    t, rec, order, members = _selection()
    path = str(tmp_path / "panel.tsv")
    KF.write_panel(path, t, rec, order, members)
    lines = [ln.split("\t") for ln in open(path).read().split("\n")[1:-1]]
    head = KF.PANEL_HEADER.split("\t")
    want = []
    for ln in lines:
        want += [(ln[0] + "L", ln[head.index("left_sequence")]), (ln[0] + "R", ln[head.index("right_sequence")])]
    got = KF.panel_oligos(t, rec, order, members)
    assert got == want == [("1L", "GGGCCCCAAAA"), ("1R", "ACGTACGTACG"), ("2L", "ACGTACGTAC"), ("2R", "CCCCTTTTGG")]
    assert KF.panel_oligos(t, rec, order, members[:0]) == []
    assert KF.panel_oligos(t, rec, order, members[1:]) == [("1L", "ACGTACGTAC"), ("1R", "CCCCTTTTGG")]      # (named by acceptance)


def test_the_kinds_and_the_fan_out_of_a_shared_text():
    assert [[KF.panel_kind(i, j) for j in range(4)] for i in range(4)] == [
        ["single", "pair", "cross", "cross"], ["pair", "single", "cross", "cross"],
        ["cross", "cross", "single", "pair"], ["cross", "cross", "pair", "single"]]
    # 1L and 3L share a text, 2R has the text of 1R: equal texts once, ordered by their bytes, the owners ascending
    oligos = [("1L", "GGGGGGGGGGAA"), ("1R", "ACACACACACAC"), ("2L", "TTTTTTTTTTTT"), ("2R", "ACACACACACAC"),
              ("3L", "GGGGGGGGGGAA"), ("3R", "CCCCCCCCCCCCCC")]
    texts, owners = KF.panel_texts(oligos)
    assert texts == [b"ACACACACACAC", b"CCCCCCCCCCCCCC", b"GGGGGGGGGGAA", b"TTTTTTTTTTTT"]
    assert owners == [[1, 3], [5], [0, 4], [2]]
    # products (text 2, text 0), (text 3, text 1), (text 2, text 2): rows for every owner of either side, a product's together
    rep, fo, ro = reports._panel_fan_out(np.array([2, 3, 2]), np.array([0, 1, 2]), owners)
    assert list(zip(rep.tolist(), fo.tolist(), ro.tolist())) == [
        (0, 0, 1), (0, 0, 3), (0, 4, 1), (0, 4, 3), (1, 2, 5), (2, 0, 0), (2, 0, 4), (2, 4, 0), (2, 4, 4)]
    # 1L with 1R: pair; 1L with 2R, 1R's twin: cross; 1L with 3L, its own twin: cross; 1L with 1L: single
    assert [KF.panel_kind(0, j) for j in (1, 3, 4, 0)] == ["pair", "cross", "cross", "single"]
    assert KF.panel_texts([]) == ([], [])


def test_both_files_on_rows_made_by_hand(tmp_path):
    rows = np.zeros(3, dtype=KF.PANEL_PRODUCT)
    rows["file"] = ["a.fa", "a.fa", "b.fa.gz"]
    rows["record"] = ["chr1", "chr1", "contig 7"]
    rows["record_index"], rows["start"], rows["length"] = [0, 0, 3], [12, 12, 0], [88, 120, 45]
    rows["end"] = rows["start"] + rows["length"]
    rows["forward"], rows["reverse"], rows["kind"] = ["1L", "1L", "2R"], ["1R", "2R", "2R"], ["pair", "cross", "single"]
    rows["forward_mismatches"], rows["reverse_mismatches"] = [0, 1, 3], [0, 2, 3]
    rows["forward_end_mismatches"], rows["reverse_end_mismatches"] = [0, 0, 1], [0, 2, 0]
    rows["forward_index"], rows["reverse_index"] = [0, 0, 3], [1, 3, 3]
    path = str(tmp_path / "p.tsv")
    KF.write_panel_products(path, rows)
    assert open(path, "rb").read() == (
        b"file\trecord\trecord_index\tstart\tend\tlength\tforward\treverse\tkind\tforward_mismatches\treverse_mismatches\t"
        b"forward_end_mismatches\treverse_end_mismatches\n"
        b"a.fa\tchr1\t0\t12\t100\t88\t1L\t1R\tpair\t0\t0\t0\t0\n"
        b"a.fa\tchr1\t0\t12\t132\t120\t1L\t2R\tcross\t1\t2\t0\t2\n"
        b"b.fa.gz\tcontig 7\t3\t0\t45\t45\t2R\t2R\tsingle\t3\t3\t1\t0\n")
    KF.write_panel_products(path, rows[:0])
    assert open(path).read() == KF.PANEL_PRODUCT_HEADER + "\n"
    summary = np.zeros(2, dtype=KF.PANEL_SUMMARY)
    summary["file"], summary["forward"], summary["reverse"], summary["kind"] = ["a.fa", "b.fa.gz"], ["1L", "2R"], ["1R", "2R"], ["pair", "single"]
    summary["products"], summary["clean_end_products"] = [7, 1], [5, 0]
    KF.write_panel_summary(path, summary)
    assert open(path, "rb").read() == (b"file\tforward\treverse\tkind\tproducts\tclean_end_products\n"
                                       b"a.fa\t1L\t1R\tpair\t7\t5\nb.fa.gz\t2R\t2R\tsingle\t1\t0\n")
    KF.write_panel_summary(path, summary[:0])
    assert open(path).read() == KF.PANEL_SUMMARY_HEADER + "\n"


def test_panel_products_refusal():
    ok = KF.panel_products_refusal
    amp, size = (70, 150), (25, 35)
    assert ok(None, False, False, amp, size, 9, 1) is None                  # neither option: nothing is looked at
    assert ok(8, True, False, amp, size, 1, 1000) is None and ok(8, False, True, amp, size, 0, 150) is None
    assert ok(8, True, True, amp, size, 3, (1 << 31) - 1) is None
    assert "--out_panel_products needs --panel" in ok(None, True, True, amp, size, 1, 1000)
    assert "--out_panel_summary needs --panel" in ok(None, False, True, amp, size, 1, 1000)
    assert "between 0 and 3" in ok(8, True, False, amp, size, 4, 1000) and "between 0 and 3" in ok(8, True, False, amp, size, -1, 1000)
    assert "--amp_size, 150 bases (got 149)" in ok(8, True, False, amp, size, 1, 149)
    assert "--primer_size, 120 bases (got 119)" in ok(8, True, False, (70, 100), (25, 60), 1, 119)
    assert ok(8, True, False, (70, 100), (25, 60), 1, 120) is None
    assert "2^31" in ok(8, False, True, amp, size, 1, 1 << 31)
    # the order: the panel, the distance, the designed product, two oligos, 2^31
    assert "needs --panel" in ok(None, True, False, amp, size, 9, 1)
    assert "between" in ok(8, True, False, amp, size, 9, 1)
    assert "--amp_size" in ok(8, True, False, (70, 100), (25, 60), 1, 99)
    for line in (ok(None, True, False, amp, size, 1, 1000), ok(8, True, False, amp, size, 1, 149), ok(8, True, False, amp, size, 1, 1 << 31)):
        assert "\n" not in line
    # the pass itself refuses what the command line would: no device is touched
    oligos = [("1L", "ACGTACGTACGT"), ("1R", "GGATCCATTGCAAT")]
    for bad in (dict(mismatches=4), dict(max_product=27), dict(max_product=1 << 31)):
        with pytest.raises(ValueError):
            KF.panel_products(oligos, ["x.fa"], [], 12, 12, 28, **bad)
    for bad in ([("1L", "ACGTACGTA")], [("1L", "ACGTACGTNN")], [("1L", "A" * 61)]):
        with pytest.raises(ValueError):
            KF.panel_products(bad, ["x.fa"], [], 12, 12, 28)
    # no oligo: no row, no device, no file read
    rows, summary = KF.panel_products([], ["no_such_file.fa"], [], 12, 12, 28)
    assert len(rows) == 0 and len(summary) == 0 and rows.dtype == KF.PANEL_PRODUCT and summary.dtype == KF.PANEL_SUMMARY


def test_the_record_and_the_header():
    d = _native.MULTIPLEX_HIT
    assert d.itemsize == 24
    assert [(n, d.fields[n][1]) for n in d.names] == [("pos", 0), ("length", 8), ("fwd", 12), ("rev", 14), ("fwd_mm", 16),
                                                       ("rev_mm", 17), ("fwd_end_mm", 18), ("rev_end_mm", 19), ("pad", 20)]
    header = open(os.path.join(ROOT, "include", "krisp_hip.h")).read()
    assert re.search(r"typedef struct \{ uint64_t pos; uint32_t length; uint16_t fwd, rev; uint8_t fwd_mm, rev_mm, fwd_end_mm, "
                     r"rev_end_mm, pad\[4\]; \} kr_multiplex_hit;", header)
    bound = {n: (res, args) for n, res, args in _native.SYMBOLS}
    for name in ("kr_multiplex_table", "kr_multiplex_scan", "kr_multiplex_fetch", "kr_multiplex_sites", "kr_multiplex_tally"):
        assert re.search(r"\bint64_t " + name + r"\(kr_ctx\*", header), name
        assert name in bound
    assert len(bound["kr_multiplex_table"][1]) == 6
    for name in ("multiplex_table", "multiplex_scan", "multiplex_products", "multiplex_sites", "multiplex_tally"):
        assert callable(getattr(_native.Engine, name))
    for name in ("panel_oligos", "panel_products", "panel_products_refusal", "panel_kind", "panel_texts", "write_panel_products",
                 "write_panel_summary"):
        assert getattr(KF, name) is getattr(reports, name)
    unit = open(os.path.join(ROOT, "krisp_amd", "csrc", "krisp_hip.hip")).read()
    assert 0 < unit.index('"k_primers.inc"') < unit.index('"k_multiplex.inc"') < unit.index('"h_primers.inc"') < unit.index('"h_multiplex.inc"')
    kernel = open(os.path.join(ROOT, "krisp_amd", "csrc", "k_multiplex.inc")).read()
    assert "k_mux_join" in kernel and "k_mux_tally" in kernel and "float" not in kernel and "double" not in kernel
    # the join itself holds no atomic: the list's bytes are the same on every run (the tally adds integers)
    assert "atomic" not in kernel[kernel.index("void k_mux_join"):kernel.index("// tally[")]

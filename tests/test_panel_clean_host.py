"""The host side of the clean panel selection (--panel-clean) without a GPU: the candidates' texts and rows
against the reference's table, the file's bytes with and without `drops`, panel_clean_refusal, select_panel_clean's own
refusals, the header's entry points and the translation unit's parts, and a hand-worked example of four candidates."""
import os
import re
import sys

import numpy as np
import pytest

from krisp_amd import _native, reports
from krisp_amd import krisp_fasta as KF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import panel_clean_cases as CC                                             # noqa: E402
import panel_clean_reference as ref                                        # noqa: E402


def _as_records(c, order):
    """a set's candidates as design records behind a shuffled `order`: region order[i] is candidate i"""
    n = len(c["templates"])
    rec = np.zeros(n, dtype=_native.DESIGN_RECORD)
    t = np.zeros((n, len(c["templates"][0])), dtype=np.uint8)
    for i, region in enumerate(order):
        ls, ln, rs, rn = c["pairs"][i]
        rec[region]["found"] = 1
        rec[region]["left_start"], rec[region]["left_len"], rec[region]["right_start"], rec[region]["right_len"] = ls, ln, rs, rn
        t[region] = np.frombuffer(c["templates"][i].encode(), dtype=np.uint8)
    return t, rec


@pytest.mark.parametrize("name", ["three_owners", "palindrome", "random_65", "shared_300", "random_1"])
def test_texts_and_rows_are_the_reference_table(name):
    c = CC.case(name)
    n = len(c["templates"])
    order = np.random.default_rng(5).permutation(n)
    t, rec = _as_records(c, order)
    texts, rows = KF.panel_candidate_texts(t, rec, order)
    want_texts, want_rows = ref.table(c["templates"], c["pairs"])
    assert texts == want_texts and rows.dtype == np.uint32 and rows.shape == (n, 2) and rows.tolist() == [list(r) for r in want_rows]
    assert texts == sorted(set(texts))
    # the texts are what write_panel prints: panel_oligos over every candidate as a member
    members = np.zeros(n, dtype=_native.PANEL_MEMBER)
    members["position"] = np.arange(n)
    oligos = KF.panel_oligos(t, rec, order, members)
    assert [texts[r].decode() for row in rows.tolist() for r in row] == [x for _, x in oligos]
    if name == "shared_300":
        assert len(texts) <= 28 < n
    if name == "three_owners":
        assert rows[1, 0] == rows[2, 0] == rows[3, 0] and len(texts) == 2 * n - 2


def test_no_candidate_is_an_empty_table():
    texts, rows = KF.panel_candidate_texts(np.zeros((1, 40), dtype=np.uint8), np.zeros(1, dtype=_native.DESIGN_RECORD), [])
    assert texts == [] and rows.shape == (0, 2)
    members, fates, drops = KF.select_panel_clean(np.zeros((1, 40), dtype=np.uint8), np.zeros(1, dtype=_native.DESIGN_RECORD), [], 8,
                                                  ["none.fa"], [], 12, 12, 40)
    assert len(members) == 0 and len(fates) == 0 and drops.tolist() == [0]       # no device, no file read


def test_write_panel_with_and_without_drops(tmp_path):
    t = np.frombuffer(b"ACGTACGTACGGTTTTCCCCAAAAGGGG" + b"TTGACCATGCAAGGCTTAACCGGTTAAC" + b"GGGGCCCCAAAATTTTACGTACGTACGT", dtype=np.uint8).reshape(3, 28)
    rec = np.zeros(3, dtype=_native.DESIGN_RECORD)
    rec["found"] = [1, 0, 1]
    rec["pair_penalty"] = [2500, 0, 1234]
    rec["product_size"] = [28, 0, 27]
    rec["left_start"], rec["left_len"], rec["right_start"], rec["right_len"] = [0, 0, 1], [10, 0, 11], [18, 0, 17], [10, 0, 11]
    order = KF.panel_candidates(rec)
    members = np.zeros(2, dtype=_native.PANEL_MEMBER)
    members["position"] = [0, 1]
    members["cross_any"], members["cross_end"] = [0, 301234], [0, 273150]
    members["dropped"] = [[3, 1], [0, 2]]
    plain, clean = str(tmp_path / "plain.tsv"), str(tmp_path / "clean.tsv")
    KF.write_panel(plain, t, rec, order, members)
    KF.write_panel(clean, t, rec, order, members, np.array([9, 4, 0], dtype=np.uint32))
    head = b"member\tregion\tpair_penalty\tproduct_size\tleft_sequence\tright_sequence\tcross_any\tcross_end\tdropped_same_locus\tdropped_clash"
    rows = [b"1\t1\t1.234\t27\tGGGCCCCAAAA\tACGTACGTACG\t-273.150\t-273.150\t3\t1", b"2\t0\t2.500\t28\tACGTACGTAC\tCCCCTTTTGG\t28.084\t0.000\t0\t2"]
    assert open(plain, "rb").read() == head + b"\n" + rows[0] + b"\n" + rows[1] + b"\n"
    assert open(clean, "rb").read() == head + b"\tdropped_cross\n" + rows[0] + b"\t4\n" + rows[1] + b"\t0\n"
    KF.write_panel(clean, t, rec, order, members[:0], np.array([2], dtype=np.uint32))
    assert open(clean).read() == KF.PANEL_HEADER + "\tdropped_cross\n"


def test_panel_clean_refusal():
    ok = KF.panel_clean_refusal
    assert ok(None, False, (70, 150), (25, 35), 9, 0) is None                      # not given: nothing is looked at
    assert ok(8, True, (70, 150), (25, 35), 1, 1000) is None and ok(8, True, (70, 150), (25, 35), 0, 150) is None
    assert ok(8, True, (70, 100), (25, 60), 3, 120) is None
    assert ok(None, True, (70, 150), (25, 35), 1, 1000) == "--panel-clean needs --panel (the selection it keeps clean)"
    assert "between 0 and 3 (got 4)" in ok(8, True, (70, 150), (25, 35), 4, 1000) and "(got -1)" in ok(8, True, (70, 150), (25, 35), -1, 1000)
    assert "upper bound of --amp_size, 150 bases (got 149)" in ok(8, True, (70, 150), (25, 35), 1, 149)
    assert "twice the upper bound of --primer_size, 120 bases (got 119)" in ok(8, True, (70, 100), (25, 60), 1, 119)
    assert "smaller than 2^31" in ok(8, True, (70, 150), (25, 35), 1, 1 << 31)
    # the order: the panel, the distance, the designed product, two primers
    assert "needs --panel" in ok(None, True, (70, 150), (25, 35), 4, 10) and "--primer-mismatches" in ok(8, True, (70, 150), (25, 35), 4, 10)
    assert "--amp_size" in ok(8, True, (70, 150), (25, 35), 1, 10)
    for why in (ok(None, True, (70, 150), (25, 35), 1, 1000), ok(8, True, (70, 150), (25, 35), 4, 1000), ok(8, True, (70, 150), (25, 35), 1, 149)):
        assert "\n" not in why


def test_select_panel_clean_refuses_before_a_device_or_a_file():
    c = CC.case("cross_forward")
    t, rec = _as_records(c, [0, 1, 2])
    go = lambda **kw: KF.select_panel_clean(t, rec, [0, 1, 2], kw.pop("size", 3), ["none.fa"], [], 12, 12, 40, **kw)   # noqa: E731
    for kw, piece in ((dict(size=0), "between 1 and 64"), (dict(size=65), "between 1 and 64"), (dict(primer_size=(5, 9)), "primer_size"),
                      (dict(mismatches=4), "--primer-mismatches"), (dict(mismatches=-1), "--primer-mismatches"),
                      (dict(max_product=1 << 31), "2^31"), (dict(max_product=23), "twice the longest primer, 24 bases (got 23)")):
        with pytest.raises(ValueError, match=re.escape(piece)):
            go(**kw)


def test_the_entry_points_and_the_parts():
    header = open(os.path.join(ROOT, "include", "krisp_hip.h")).read()
    bound = {n: (res, args) for n, res, args in _native.SYMBOLS}
    nargs = {"kr_panel_sites_table": 6, "kr_panel_sites_scan": 2, "kr_panel_sites_fetch": 4, "kr_panel_run_clean": 7, "kr_panel_clean_drops": 3}
    for name, n in nargs.items():
        assert re.search(r"\bint64_t " + name + r"\(kr_ctx\*", header), name
        assert len(bound[name][1]) == n, name
    assert "const uint8_t* templates, const uint16_t* pairs, const uint32_t* texts, uint64_t ncand" in header
    assert len(bound["kr_panel_run"][1]) == 6                                      # kr_panel_run keeps its arguments
    for name in ("panel_sites_table", "panel_sites_scan", "panel_sites", "panel_clean", "panel"):
        assert callable(getattr(_native.Engine, name))
    for name in ("panel_clean_refusal", "panel_candidate_texts", "select_panel_clean", "write_panel"):
        assert getattr(KF, name) is getattr(reports, name)
    unit = open(os.path.join(ROOT, "krisp_amd", "csrc", "krisp_hip.hip")).read()
    assert (0 < unit.index('"k_panel.inc"') < unit.index('"pclean_step.inc"') < unit.index('"k_panel_clean.inc"') < unit.index('"h_panel.inc"')
            < unit.index('"h_panel_clean.inc"'))
    kernels = open(os.path.join(ROOT, "krisp_amd", "csrc", "k_panel_clean.inc")).read()
    assert "float" not in kernels and "double" not in kernels
    assert set(re.findall(r"\batomic[A-Z]\w*", kernels)) == {"atomicMin"}
    # k_panel_round is the parent's: the clean run launches it as it is
    round_kernel = open(os.path.join(ROOT, "krisp_amd", "csrc", "k_panel.inc")).read()
    assert "pclean" not in round_kernel and "template <" not in round_kernel


def test_four_candidates_worked_by_hand():
    """Primers of 10 bases at both ends of templates of 30; one file "x" of one record, max_product 60, M = 0.
    Candidate 0's left primer AACCGGTTAC and candidate 2's right primer GATTACAGAT: the file holds AACCGGTTAC, five N and the
    reverse complement ATCTGTAATC, a product of 25 bases, so candidate 2 crosses candidate 0.
    Candidate 1's right primer CCATGGATGC with itself: CCATGGATGC, three N, GCATCCATGG, a product of 23 bases: self-priming,
    fate (5, 0) before any round -- it would have been member 2.
    Candidate 0 is member 1; 1 is never alive; 2 is dropped by member 1 (4, 1); 3 is member 2."""
    t = ["AACCGGTTAC" + "ACTGACTGAC" + "TTGCAGCATA",
         "TGTGTGCACA" + "CAGTCAGTCA" + "GCATCCATGG",
         "CTCTAGAGGA" + "GTCAGTCAGT" + "ATCTGTAATC",
         "GGAATTCGCA" + "TGACTGACTG" + "CGTTAGCCAT"]
    pairs = [(0, 10, 20, 10)] * 4
    from panel_reference import primers
    assert primers(t[2], pairs[2])[1] == "GATTACAGAT" and primers(t[1], pairs[1])[1] == "CCATGGATGC"
    files = [b"NN" + b"AACCGGTTAC" + b"NNNNN" + b"ATCTGTAATC" + b"NNNN" + b"CCATGGATGC" + b"NNN" + b"GCATCCATGG" + b"NN"]
    members, fates, drops = ref.select(t, pairs, 4, 10 ** 9, files, False, 0, 60)
    assert fates == [(1, 1), (5, 0), (4, 1), (1, 2)] and drops == [1, 1, 0]
    assert [m["position"] for m in members] == [0, 3]
    # a max_product of 24 keeps the self product (23 bases) and loses the cross (25)
    _, fates, drops = ref.select(t, pairs, 4, 10 ** 9, files, False, 0, 24)
    assert fates == [(1, 1), (5, 0), (1, 2), (1, 3)] and drops == [1, 0, 0, 0]

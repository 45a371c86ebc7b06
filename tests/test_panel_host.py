"""The host side of the panel pass (--panel) without a GPU: the candidates' order against a plain sort, the
file's bytes on a hand-made selection, panel_refusal, the header's entry points and the record layouts, and a hand-worked
example of three candidates whose fates are written out here."""
import os
import re
import sys

import numpy as np
import pytest

from krisp_amd import _native, reports, thermo
from krisp_amd import krisp_fasta as KF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import panel_reference as ref                                               # noqa: E402


def _records(rows):
    """rows: (found, pair_penalty) -> DESIGN_RECORD array"""
    r = np.zeros(len(rows), dtype=_native.DESIGN_RECORD)
    r["found"] = [a for a, _ in rows]
    r["pair_penalty"] = [b for _, b in rows]
    return r


def test_the_order_without_guides_is_penalty_then_region():
    rng = np.random.default_rng(3)
    rows = [(int(rng.integers(0, 4) > 0), int(rng.integers(0, 5)) * 250) for _ in range(200)]      # (few penalties: many ties)
    rec = _records(rows)
    want = sorted((i for i, (f, _) in enumerate(rows) if f), key=lambda i: (rows[i][1], i))
    got = KF.panel_candidates(rec)
    assert got.dtype == np.int64 and got.tolist() == want and 0 < len(want) < 200
    assert KF.panel_candidates(_records([])).tolist() == [] and KF.panel_candidates(_records([(0, 5)])).tolist() == []


def test_the_order_with_guides_is_min_mismatches_first():
    rng = np.random.default_rng(4)
    n = 300
    rows = [(int(rng.integers(0, 5) > 0), int(rng.integers(0, 4)) * 500) for _ in range(n)]
    rec = _records(rows)
    guides = np.zeros(n, dtype=_native.GUIDE_RECORD)
    guides["found"] = rng.integers(0, 3, n) > 0
    guides["min_mismatches"] = rng.integers(0, 4, n)
    want = sorted((i for i in range(n) if rows[i][0] and guides["found"][i]),
                  key=lambda i: (-int(guides["min_mismatches"][i]), rows[i][1], i))
    got = KF.panel_candidates(rec, guides)
    assert got.tolist() == want and 0 < len(want) < len(KF.panel_candidates(rec))
    mm = guides["min_mismatches"][got]
    assert np.all(mm[:-1] >= mm[1:])
    with pytest.raises(ValueError):
        KF.panel_candidates(rec, guides[:-1])


def test_write_panel_on_a_hand_made_selection(tmp_path):
    t = np.frombuffer(b"ACGTACGTACGGTTTTCCCCAAAAGGGG" + b"TTGACCATGCAAGGCTTAACCGGTTAAC" + b"GGGGCCCCAAAATTTTACGTACGTACGT", dtype=np.uint8).reshape(3, 28)
    rec = np.zeros(3, dtype=_native.DESIGN_RECORD)
    rec["found"] = [1, 0, 1]
    rec["pair_penalty"] = [2500, 0, 1234]
    rec["product_size"] = [28, 0, 27]
    rec["left_start"], rec["left_len"], rec["right_start"], rec["right_len"] = [0, 0, 1], [10, 0, 11], [18, 0, 17], [10, 0, 11]
    order = KF.panel_candidates(rec)
    assert order.tolist() == [2, 0]
    members = np.zeros(2, dtype=_native.PANEL_MEMBER)
    members["position"] = [0, 1]
    members["cross_any"], members["cross_end"] = [0, 301234], [0, 273150]
    members["dropped"] = [[3, 1], [0, 2]]
    path = str(tmp_path / "panel.tsv")
    KF.write_panel(path, t, rec, order, members)
    assert open(path, "rb").read() == (
        b"member\tregion\tpair_penalty\tproduct_size\tleft_sequence\tright_sequence\tcross_any\tcross_end\tdropped_same_locus\tdropped_clash\n"
        b"1\t1\t1.234\t27\tGGGCCCCAAAA\tACGTACGTACG\t-273.150\t-273.150\t3\t1\n"
        b"2\t0\t2.500\t28\tACGTACGTAC\tCCCCTTTTGG\t28.084\t0.000\t0\t2\n")
    assert KF.PANEL_HEADER.encode() + b"\n" == open(path, "rb").read().split(b"\n")[0] + b"\n"
    KF.write_panel(path, t, rec, order, members[:0])
    assert open(path).read() == KF.PANEL_HEADER + "\n"


def test_panel_refusal():
    ok = KF.panel_refusal
    assert ok(True, 8, True, False) is None and ok(True, 1, True, False) is None and ok(True, 64, True, False) is None
    assert ok(False, None, False, False) is None and ok(True, None, False, True) is None
    assert "--panel needs --design-primers" in ok(False, 8, True, False)
    assert "between 1 and 64" in ok(True, 0, True, False) and "between 1 and 64" in ok(True, 65, True, False)
    assert "--out_panel needs --panel" in ok(True, None, True, False)
    assert "--panel needs --out_panel" in ok(True, 8, False, False)
    assert "--primer3" in ok(True, 8, True, True)
    # the order: the designer, the size, the file, Primer3
    assert "--design-primers" in ok(False, 0, False, True) and "between" in ok(True, 0, False, True) and "--out_panel" in ok(True, 8, False, True)
    with pytest.raises(ValueError):
        KF.select_panel(np.zeros((1, 40), dtype=np.uint8), _records([(1, 0)]), [0], 0)
    with pytest.raises(ValueError):
        KF.select_panel(np.zeros((1, 40), dtype=np.uint8), _records([(1, 0)]), [0], 65)
    with pytest.raises(ValueError):
        KF.select_panel(np.zeros((1, 40), dtype=np.uint8), _records([(1, 0)]), [0], 8, primer_size=(5, 9))
    # no candidate: no member, no device
    members, fates = KF.select_panel(np.zeros((1, 40), dtype=np.uint8), _records([(0, 0)]), [], 8)
    assert len(members) == 0 and len(fates) == 0 and members.dtype == _native.PANEL_MEMBER and fates.dtype == _native.PANEL_FATE


def test_the_records_and_the_header():
    d = _native.PANEL_MEMBER
    assert d.itemsize == 20
    assert [(n, d.fields[n][1]) for n in d.names] == [("position", 0), ("cross_any", 4), ("cross_end", 8), ("dropped", 12)]
    assert _native.PANEL_FATE.itemsize == 2 and _native.PANEL_FATE.names == ("fate", "by")
    header = open(os.path.join(ROOT, "include", "krisp_hip.h")).read()
    bound = {n: (res, args) for n, res, args in _native.SYMBOLS}
    for name in ("kr_panel_run", "kr_panel_fetch", "kr_panel_fates"):
        assert re.search(r"\bint64_t " + name + r"\(kr_ctx\*", header), name
        assert name in bound
    assert len(bound["kr_panel_run"][1]) == 6
    assert re.search(r"typedef struct \{ uint32_t position; int32_t cross_any, cross_end; uint32_t dropped\[2\]; \} kr_panel_member;", header)
    assert "const uint8_t* templates, const uint16_t* pairs, uint64_t ncand, int W, int size" in header
    assert callable(_native.Engine.panel)
    for name in ("panel_refusal", "panel_candidates", "select_panel", "write_panel"):
        assert getattr(KF, name) is getattr(reports, name)
    # the kernel and the step file are parts of the one translation unit, the step file in front of the kernel
    unit = open(os.path.join(ROOT, "krisp_amd", "csrc", "krisp_hip.hip")).read()
    assert 0 < unit.index('"panel_step.inc"') < unit.index('"k_panel.inc"') < unit.index('"h_panel.inc"')
    kernel = open(os.path.join(ROOT, "krisp_amd", "csrc", "k_panel.inc")).read()
    assert "des_duplex(" in kernel and "float" not in kernel and "double" not in kernel


def test_three_candidates_worked_by_hand():
    """W = 26, primers of 10 at both ends, max_sec = -100 degrees C = 173150 mK.
    Candidate 0 is member 1.
    Candidate 1 carries candidate 0's bases [5, 21) reverse-complemented at its own [4, 20): the same locus, dropped by
    member 1 without a look at its primers (fate 2, by 1).
    Candidate 2 shares no 16 bases with candidate 0.  Its left primer AAAAAAAAGC and member 1's left primer TTTTTTTTGC: the
    alignment that pairs the eight A with the eight T is a run of eight A.T pairs, read on the candidate's primer the oligo
    AAAAAAAA, whose Tm in the model is far above 173150 mK: a clash (fate 3, by 1).  Nothing is left alive: one member of
    the three asked for."""
    max_sec = thermo.options(max_sec_tm=-100)["max_sec"]
    assert max_sec == 173150
    t0 = "TTTTTTTTGC" + "ACGGTC" + "CAGTGACCTA"
    t1 = "CGTA" + ref.rc(t0[5:21]) + "GCATGC"
    t2 = "AAAAAAAAGC" + "GTCTGA" + "TCAGGTCATG"
    templates, pairs = [t0, t1, t2], [(0, 10, 16, 10)] * 3
    assert all(len(t) == 26 for t in templates)
    assert ref.same_locus(t0, t1) and not ref.same_locus(t0, t2) and not ref.windows(t0) & ref.windows(t1)
    run = ref.duplex_figure("AAAAAAAAGC", "TTTTTTTTGC")
    assert run[0] >= ref.duplex_figure("AAAAAAAA", "TTTTTTTT")[0] > max_sec
    members, fates = ref.select(templates, pairs, 3, max_sec)
    assert fates == [(1, 1), (2, 1), (3, 1)]
    assert members == [{"position": 0, "cross_any": 0, "cross_end": 0, "dropped": [1, 1]}]
    # with a max_sec nothing reaches, candidate 2 is member 2 and carries its figures against member 1
    members, fates = ref.select(templates, pairs, 3, 10 ** 9)
    assert fates == [(1, 1), (2, 1), (1, 2)]
    assert (members[1]["cross_any"], members[1]["cross_end"]) == ref.cross_figure(ref.primers(t2, pairs[2]), ref.primers(t0, pairs[0]))
    assert members[1]["cross_any"] >= run[0] and members[1]["cross_end"] <= members[1]["cross_any"]

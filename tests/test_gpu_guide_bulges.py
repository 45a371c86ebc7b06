"""--guide-hit-bulges on the GPU (kr_guide_bulges_*, csrc/k_guide_bulges.inc, csrc/gbulge_step.inc): the device's complete
list equals the definition (guide_bulges_reference.py) in every field over the seeded cases of guide_bulge_cases.py --
every case and soft-mask mode, with and without need_pam --, every plant's row is the one it pins, the windows' text;
short texts; a dense text whose seed pairs own more rows than there are pairs; the same bytes on every run and a state
that the unbulged pass does not share; the library's refusals; the command line on a golden case."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import fasta
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_bulge_cases as BC                                             # noqa: E402
import guide_bulges_reference as ref                                       # noqa: E402
from test_locate_host import FC, py_record_ids                             # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402

pytestmark = pytest.mark.gpu


def _texts(guides):
    G = len(guides[0]) if len(guides) else 1
    return np.frombuffer("".join(guides).encode("ascii"), dtype=np.uint8).reshape(-1, G)


def _locate(eng, G, omit, max_bases, uploaded):
    """the engine as a locate context for protospacers of G letters (again: the genome goes first)"""
    if uploaded:
        eng.free(0)
    eng.set_params_locate(0, G, 0, omit, max_bases=max(int(max_bases), 1))


def _as_hits(got):
    """the device's list, ordered as the reference orders its own, in the reference's dtype"""
    order = np.lexsort((got["bulge"], got["guide"], got["strand"], got["pos"]))
    out = np.zeros(len(got), dtype=ref.HIT)
    for f in ref.FIELDS:
        out[f] = got[f][order]
    return out, order


def _check(eng, text, G, B, want):
    """the scan of the genome under id 0 against the reference's hits: all nine fields, the windows' text and padding"""
    got = eng.guide_bulges(0)
    rows = eng.guide_bulge_windows(G + B)
    assert got.dtype.itemsize == 32 and len(got) == len(want), (len(got), len(want))
    mine, order = _as_hits(got)
    for f in ref.FIELDS:
        bad = np.flatnonzero(mine[f] != want[f])
        assert len(bad) == 0, (f, bad[:5].tolist(), mine[f][bad[:5]].tolist(), want[f][bad[:5]].tolist())
    assert rows.shape == (len(want), G + B)
    assert [bytes(r).decode("ascii") for r in rows[order]] == [w + "\0" * (G + B - len(w)) for w in ref.ref_windows(text, want)]
    return got, mine


# ----------------------------------------------------------------------------
# 1. the seeded cases
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
def test_every_seeded_case_equals_the_reference(name):
    from krisp_amd import _native
    c = BC.case(name)
    G, M, B, pam5, pam3 = c["G"], c["M"], c["B"], c["pam5"], c["pam3"]
    t_bytes = _texts(c["guides"])
    figures = []
    with _native.Engine() as eng:
        uploaded = False
        for omit in (False, True):
            _locate(eng, G, omit, BC.N_TEXT, uploaded)
            eng.upload(0, c["text"])
            uploaded = True
            for need in ((False, True) if (pam5 or pam3) else (False,)):
                eng.guide_bulges_table(t_bytes, M, B, pam5, pam3, need)
                want = BC.reference(name, int(omit), need)
                _, mine = _check(eng, c["text"], G, B, want)
                if not need:
                    BC.check_plants(c["plants"], mine, int(omit))
                figures.append((int(omit), int(need), len(want)))
    print(name, "(omit, need_pam, hits)", figures)
    assert all(n for _, need, n in figures if not need)


# ----------------------------------------------------------------------------
# 2. short texts
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
def test_short_texts(name):
    """0 and 1 bytes, a text shorter than G - B, a right half whose window would begin before the text, every bulged window
    alone (exactly G + b and G - b bytes), one byte short at either end, inside 40 more bytes: the reference's rows"""
    from krisp_amd import _native
    c = BC.case(name)
    G, M, B, guides, pam5, pam3 = c["G"], c["M"], c["B"], c["guides"], c["pam5"], c["pam3"]
    t_bytes = _texts(guides)
    rows = 0
    with _native.Engine() as eng:
        uploaded = False
        for omit in (False, True):
            _locate(eng, G, omit, G + 64, uploaded)
            eng.guide_bulges_table(t_bytes, M, B, pam5, pam3, False)
            for text, plants in BC.short_texts(name):
                eng.upload(0, text)
                uploaded = True
                want = ref.ref_bulge_hits(text, omit, guides, M, B, pam5, pam3)
                _, mine = _check(eng, text, G, B, want)
                BC.check_plants(plants, mine, int(omit), pam=False)
                if len(text) < G - B:
                    assert len(mine) == 0
                rows += len(mine)
    print(name, "rows", rows)
    assert rows > 0


# ----------------------------------------------------------------------------
# 3. a dense text
# ----------------------------------------------------------------------------
def test_a_dense_text_where_pairs_own_more_rows_than_there_are_pairs():
    """a period-G repeat of a guide: every exact site is shadowed by bulged rows beside its ends, a seed pair owns up to 2 B
    of them, and a block of 256 pairs writes more than 256 rows"""
    from krisp_amd import _native
    text, guides, M, B = BC.dense()
    G = len(guides[0])
    want = ref.ref_bulge_hits(text, False, guides, M, B)
    pairs = BC.seed_pairs(text, False, guides, M, B)
    print("pairs", pairs, "rows", len(want))
    assert pairs > 256 and len(want) > pairs
    with _native.Engine() as eng:
        _locate(eng, G, False, len(text), False)
        eng.upload(0, text)
        eng.guide_bulges_table(_texts(guides), M, B)
        _check(eng, text, G, B, want)


# ----------------------------------------------------------------------------
# 4. the same bytes on every run; a state of its own
# ----------------------------------------------------------------------------
def test_two_scans_and_the_unbulged_pass_beside_them():
    from krisp_amd import _native
    import guide_hits_reference as plain
    name = "g20_m2_b2_tttv"
    c = BC.case(name)
    G, M, B = c["G"], c["M"], c["B"]
    t = _texts(c["guides"])
    with _native.Engine() as eng:
        _locate(eng, G, False, BC.N_TEXT, False)
        eng.upload(0, c["text"])
        eng.guide_hits_table(t, 1, c["pam5"], c["pam3"])
        before = eng.guide_hits(0)
        before_rows = eng.guide_hit_windows(G)
        eng.guide_bulges_table(t, M, B, c["pam5"], c["pam3"])
        first = eng.guide_bulges(0)
        again = eng.guide_bulges(0)
        assert len(first) > 0 and first.tobytes() == again.tobytes()
        # the unbulged pass after a bulged table and scan: its own table (another distance), its own list
        after = eng.guide_hits(0)
        assert len(before) > 0 and after.tobytes() == before.tobytes()
        assert eng.guide_hit_windows(G).tobytes() == before_rows.tobytes()
        want_plain = plain.ref_hits(c["text"], False, c["guides"], 1, c["pam5"], c["pam3"])
        assert len(after) == len(want_plain)
        # ... and the bulged pass after that
        _check(eng, c["text"], G, B, BC.reference(name, 0))
        assert eng.guide_bulges(0).tobytes() == first.tobytes()
    print("bulged", len(first), "unbulged", len(before))


# ----------------------------------------------------------------------------
# 5. the library's refusals
# ----------------------------------------------------------------------------
def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    P, CAP, STATE = -2, -3, -4
    guide = "ACGTTGCAAGCTTGACCTGA"
    text = (b"TTTC" + guide[:9].encode() + b"G" + guide[9:].encode() + b"CAGT") * 3
    t = _texts([guide])

    def code(f):
        with pytest.raises(_native.KrispHipError) as e:
            f()
        assert "kr_guide_bulges" in str(e.value) or "kr_set_params_locate" in str(e.value)
        return e.value.code

    with _native.Engine() as eng:
        assert code(lambda: eng.guide_bulges_table(t, 1, 1)) == STATE          # no locate context
        _locate(eng, 20, False, 1000, False)
        assert code(lambda: eng.guide_bulges(0)) == P                          # a scan before a table
        eng.upload(0, text)
        for B in (-1, 0, 3):
            assert code(lambda: eng.guide_bulges_table(t, 1, B)) == P
        for M in (-1, 3):                                                      # (3 is the unbulged pass's most; not this one's)
            assert code(lambda: eng.guide_bulges_table(t, M, 1)) == P
        assert code(lambda: eng.guide_bulges_table(_texts([guide[:-1] + "N"]), 1, 1)) == P
        assert code(lambda: eng.guide_bulges_table(t, 1, 1, pam5="TTJ")) == P
        assert eng.lib.kr_guide_bulges_table(eng.ctx, None, 1, 1, 1, None, None, 0) == P
        assert eng.lib.kr_guide_bulges_table(eng.ctx, t.ctypes.data, 1 << 23, 1, 1, None, None, 0) == CAP
        assert code(lambda: eng.guide_bulges(0)) == P                          # none of them left a table behind
        eng.guide_bulges_table(t, 0, 1, pam5="tttv")
        got = eng.guide_bulges(0)
        want = ref.ref_bulge_hits(text, False, [guide], 0, 1, "TTTV", "")
        assert len(got) == len(want) == 3 and (got["bulge"] == 1).all() and (got["bulge_column"] == 9).all() and (got["pam"] == 3).all()
        out = np.zeros(4, dtype=_native.GUIDE_BULGE_HIT_RAW)
        assert eng.lib.kr_guide_bulges_fetch(eng.ctx, out.ctypes.data, 2) == CAP and eng.lib.kr_guide_bulges_fetch(eng.ctx, out.ctypes.data, 4) == 3
        assert out[:3].tobytes() == got.tobytes()
        # no guides, a genome shorter than the halves: no hits
        eng.guide_bulges_table(np.empty((0, 20), dtype=np.uint8), 1, 2)
        assert len(eng.guide_bulges(0)) == 0 and eng.guide_bulge_windows(22).shape == (0, 22)
        eng.guide_bulges_table(t, 0, 2)
        eng.upload(0, text[:8])
        assert len(eng.guide_bulges(0)) == 0
        eng.free(0)
        assert code(lambda: eng.guide_bulges(0)) == STATE                      # no genome
        # a protospacer below 20 letters: the unbulged pass takes it, this one does not (halves of fewer than 9 letters)
        _locate(eng, 19, False, 1000, False)
        eng.guide_hits_table(_texts([guide[:19]]), 1)
        assert code(lambda: eng.guide_bulges_table(_texts([guide[:19]]), 1, 1)) == P


def test_another_geometry_drops_the_table():
    """kr_set_params_locate resets the pass as it resets its siblings: the table's texts are rows of G letters and its halves
    of (G - B) / 2, so after a context of another G -- or of the same -- a scan before a new table is refused and launches
    nothing; neither do a fetch and the windows of the earlier scan survive.  With a new table the rows are the reference's"""
    from krisp_amd import _native
    P, STATE = -2, -4
    g20 = "ACGTTGCAAGCTTGACCTGA"
    g40 = "GATTACAGGCTTAACCGTAGCTAGGATCCATGCAAGTCTG"
    text20 = (b"TTTC" + g20[:9].encode() + b"G" + g20[9:].encode() + b"CAGT") * 3
    text40 = (b"CC" + g40[:17].encode() + g40[18:].encode() + b"AT") * 3 + text20
    with _native.Engine() as eng:
        _locate(eng, 20, False, 1000, False)
        eng.upload(0, text20)
        eng.guide_bulges_table(_texts([g20] * 3), 0, 1)
        assert len(eng.guide_bulges(0)) == 9
        for G in (40, 20):
            _locate(eng, G, False, 1000, True)
            eng.upload(0, text40)
            with pytest.raises(_native.KrispHipError) as e:
                eng.guide_bulges(0)
            assert e.value.code == P and "kr_guide_bulges_table first" in str(e.value)
            with pytest.raises(_native.KrispHipError) as e:
                eng.guide_bulge_windows(G + 1)
            assert e.value.code == STATE
            out = np.zeros(16, dtype=_native.GUIDE_BULGE_HIT_RAW)
            assert eng.lib.kr_guide_bulges_fetch(eng.ctx, out.ctypes.data, 16) == STATE
        _locate(eng, 40, False, 1000, True)
        eng.upload(0, text40)
        eng.guide_bulges_table(_texts([g40]), 0, 1)
        want = ref.ref_bulge_hits(text40, False, [g40], 0, 1)
        assert len(want) == 3 and (want["bulge"] == -1).all()
        _check(eng, text40, 40, 1, want)


# ----------------------------------------------------------------------------
# 6. the command line
# ----------------------------------------------------------------------------
def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def test_the_command_line_on_c1_30_40_30(tmp_path):
    """--out_guides --out_guide_hits --guide-hit-bulges 1: every other output keeps its bytes, the unbulged rows are the run's
    without the option, and every bulged row is the definition's -- re-derived from the genome text window by window
    (window_row, the motifs) and as a complete list per file (ref_bulge_hits)"""
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    omit = case["omit_soft"]
    g, pam5, pam3, gc, min_mm, M, B = 20, "TV", "", (20, 80), 0, 1, 1
    flags = ["--guide-size", str(g), "--guide-gc", str(gc[0]), str(gc[1]), "--guide-min-mismatches", str(min_mm), "--pam5", pam5,
             "--guide-hit-mismatches", str(M)]
    f = {n: str(tmp_path / n) for n in ("a.align", "b.align", "a.guides", "b.guides", "a.tsv", "b.tsv", "zero.tsv")}
    csv_a = _main(argv + flags + ["-o", f["a.align"], "--out_guides", f["a.guides"], "--out_guide_hits", f["a.tsv"]])
    csv_b = _main(argv + flags + ["-o", f["b.align"], "--out_guides", f["b.guides"], "--out_guide_hits", f["b.tsv"], "--guide-hit-bulges", str(B)])
    _main(argv + flags + ["--out_guides", f["b.guides"], "--out_guide_hits", f["zero.tsv"], "--guide-hit-bulges", "0"])
    assert csv_a == csv_b and csv_a.count("\n") > 1
    assert open(f["a.align"], "rb").read() == open(f["b.align"], "rb").read() and os.path.getsize(f["a.align"]) > 0
    assert open(f["a.guides"], "rb").read() == open(f["b.guides"], "rb").read()
    plain = open(f["a.tsv"]).read()
    assert open(f["zero.tsv"]).read() == plain and plain.startswith(KF.GUIDE_HIT_HEADER + "\n")
    got = open(f["b.tsv"]).read()
    assert got.startswith(KF.GUIDE_BULGE_HIT_HEADER + "\n")
    lines = [ln.split("\t") for ln in got.split("\n")[1:-1]]
    assert all(len(ln) == 15 for ln in lines)
    # the unbulged rows, in their order, are the other run's
    unbulged = ["\t".join(ln[:12]) for ln in lines if ln[12] == "-"]
    assert all(ln[13] == "0" and ln[14] == "-" for ln in lines if ln[12] == "-")
    assert unbulged == plain.split("\n")[1:-1] and len(unbulged) > 0
    # the order of the merged file
    files = ing + out
    keys = [(int(ln[0]), files.index(ln[1]), int(ln[3]), int(ln[4]), ln[6] == "-", int(ln[5])) for ln in lines]
    assert keys == sorted(keys)

    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], _amplicon(case), omit_soft=omit)
    ingroup = [KF.simplename(p) for p in ing] if out else None
    templates = KF.design_templates(groups, ingroup)
    guides = KF.design_guides(groups, ingroup, g, pam5, pam3, gc, min_mm, templates=templates)
    texts, text_regions = KF.guide_texts(templates[0], guides, g)
    texts = [t.decode("ascii") for t in texts]
    region_text = {r: ti for ti, rs in enumerate(text_regions) for r in rs}
    bulged = [ln for ln in lines if ln[12] != "-"]
    assert len(bulged) > 0
    want_rows = []
    for fi, path in enumerate(files):
        recs = fasta.read_records(path)
        assert not fasta.detect_rna(recs)
        ids = py_record_ids(fasta._read_raw_lines(path))
        joined = b"\n".join(recs)
        starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])])
        S, bad = ref.plain.stage(joined, omit)
        Sl, badl = S.tolist(), bad.tolist()
        # every bulged row of this file, from the text
        for ln in (x for x in bulged if x[1] == path):
            ti = region_text[int(ln[0])]
            strand = ln[6] == "-"
            bulge = int(ln[13]) * (1 if ln[12] == "DNA" else -1)
            pos = int(starts[int(ln[3])]) + int(ln[4])
            assert ids[int(ln[3])] == ln[2] and int(ln[5]) - int(ln[4]) == g + bulge
            E = ref.rc(texts[ti]) if strand else texts[ti]
            r = ref.window_row(Sl, badl, pos, E, strand, bulge, M)
            assert r is not None, ln
            cols = ",".join(str(c + 1) for c in range(64) if (r[1] >> c) & 1) or "-"
            pam = ref.plain.pam_bits(S, bad, pos, int(strand), g + bulge, pam5, pam3)
            assert (ln[7], ln[8], ln[14], ln[9], ln[10]) == (str(r[0]), cols, str(r[2]), str(pam & 1), str(pam >> 1)), (ln, r, pam)
            w = joined[pos:pos + g + bulge].upper().decode("ascii")
            assert ln[11] == (ref.rc(w) if strand else w)
        # ... and no row is missing: the complete list
        hits = ref.ref_bulge_hits(joined, omit, texts, M, B, pam5, pam3)
        for h in hits:
            pos = int(h["pos"])
            ri = int(np.searchsorted(starts, pos, side="right")) - 1
            for region in text_regions[int(h["guide"])]:
                want_rows.append((region, path, ri, pos - int(starts[ri]), "+-"[int(h["strand"])], pos - int(starts[ri]) + int(h["length"]),
                                  "DNA" if h["bulge"] > 0 else "RNA"))
    got_rows = [(int(ln[0]), ln[1], int(ln[3]), int(ln[4]), ln[6], int(ln[5]), ln[12]) for ln in bulged]
    print("texts", len(texts), "unbulged", len(unbulged), "bulged", len(bulged))
    assert sorted(got_rows) == sorted(want_rows)

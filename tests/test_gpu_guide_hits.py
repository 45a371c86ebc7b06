"""--out_guide_hits on the GPU (kr_guide_hits_*, csrc/k_guide_hits.inc, csrc/ghit_step.inc): the device's list equals the
definition (guide_hits_reference.py) in every field over the seeded cases of guide_hit_cases.py -- every set, distance and
soft-mask mode, with and without need_pam --, every plant is where it must be, the windows' text; short texts; dense texts
whose counts are known in closed form; the same bytes on every run and a state that the near pass does not disturb; the
library's refusals; the command line on a golden case, alone and with --design-primers."""
import ctypes
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import fasta
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_hit_cases as GC                                               # noqa: E402
import guide_hits_reference as ref                                         # noqa: E402
from test_locate_host import FC, py_record_ids                             # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402
from test_gpu_primers import _design_options                               # noqa: E402

pytestmark = pytest.mark.gpu

RAW = {"pos": "pos", "strand": "strand", "guide": "guide", "mismatches": "mismatches", "columns": "columns", "pam": "pam"}


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
    assert not got["pad"].any()
    assert (np.diff(got["pos"].astype(np.int64)) >= 0).all()
    order = np.lexsort((got["guide"], got["strand"], got["pos"]))
    out = np.zeros(len(got), dtype=ref.HIT)
    for f, g in RAW.items():
        out[f] = got[g][order]
    return out, order


def _check(eng, text, G, want):
    """the scan of the genome under id 0 against the reference's hits: all six fields, the windows' text"""
    got = eng.guide_hits(0)
    rows = eng.guide_hit_windows(G)
    assert got.dtype.itemsize == 24 and len(got) == len(want), (len(got), len(want))
    mine, order = _as_hits(got)
    for f in ref.FIELDS:
        bad = np.flatnonzero(mine[f] != want[f])
        assert len(bad) == 0, (f, bad[:5].tolist(), mine[f][bad[:5]].tolist(), want[f][bad[:5]].tolist())
    assert rows.shape == (len(want), G)
    assert [bytes(r).decode("ascii") for r in rows[order]] == ref.ref_windows(text, want, G)
    return got, mine


# ----------------------------------------------------------------------------
# 1. the seeded cases
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.SETS))
def test_every_seeded_case_equals_the_reference(name):
    from krisp_amd import _native
    s = GC.SETS[name]
    G = s["G"]
    pam5, pam3 = GC.MOTIFS[s["motifs"]]
    t_bytes = _texts(GC.guides(name))
    figures = []
    with _native.Engine() as eng:
        uploaded = False
        for omit in (False, True):
            _locate(eng, G, omit, GC.N_TEXT, uploaded)
            for M in GC.MS:
                c = GC.case(name, M)
                eng.upload(0, c["text"])
                uploaded = True
                for need in ((False, True) if (pam5 or pam3) else (False,)):
                    eng.guide_hits_table(t_bytes, M, pam5, pam3, need)
                    want = GC.reference(name, M, omit, need)
                    _, mine = _check(eng, c["text"], G, want)
                    if not need:
                        GC.check_plants(c["plants"], mine, int(omit))
                    figures.append((int(omit), M, int(need), len(want)))
    print(name, "(omit, M, need_pam, hits)", figures)
    assert any(n for _, _, _, n in figures)


# ----------------------------------------------------------------------------
# 2. short texts
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.SETS))
def test_short_texts(name):
    """0, 1 and G - 1 bytes: no hit (and no window to launch for); the guide alone, a window below the motif's length, M
    substitutions in G + 20 bytes: the reference's rows"""
    from krisp_amd import _native
    s = GC.SETS[name]
    G, guides = s["G"], GC.guides(name)
    pam5, pam3 = GC.MOTIFS[s["motifs"]]
    t_bytes = _texts(guides)
    rows = 0
    with _native.Engine() as eng:
        uploaded = False
        for omit in (False, True):
            _locate(eng, G, omit, G + 64, uploaded)
            for M in GC.MS:
                eng.guide_hits_table(t_bytes, M, pam5, pam3, False)
                for text, plants in GC.short_texts(name, M):
                    eng.upload(0, text)
                    uploaded = True
                    want = ref.ref_hits(text, omit, guides, M, pam5, pam3)
                    _, mine = _check(eng, text, G, want)
                    GC.check_plants(plants, mine, int(omit))
                    if len(text) < G:
                        assert len(mine) == 0
                    rows += len(mine)
    print(name, "rows", rows)
    assert rows > 0


# ----------------------------------------------------------------------------
# 3. dense texts
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("G", GC.GS)
@pytest.mark.parametrize("period", [1, 2])
def test_dense_texts_count_in_closed_form(G, period):
    """every valid window of a run is a hit: a thread emits 64 hits, a tile thousands"""
    from krisp_amd import _native
    text, guide, plus, minus = GC.dense(G, period)
    with _native.Engine() as eng:
        _locate(eng, G, False, len(text), False)
        eng.upload(0, text)
        for M in (0, 3):
            eng.guide_hits_table(_texts([guide]), M)
            got = eng.guide_hits(0)
            print("G", G, "period", period, "M", M, "hits", len(got), "want", plus, minus)
            assert int((got["strand"] == 0).sum()) == plus and int((got["strand"] == 1).sum()) == minus
            assert not got["mismatches"].any() and not got["columns"].any() and (got["pam"] == 3).all() and not got["guide"].any()
            assert (np.diff(got["pos"].astype(np.int64)) > 0).all()
            assert len(eng.guide_hit_windows(G)) == plus + minus


# ----------------------------------------------------------------------------
# 4. the same bytes on every run; a state of its own
# ----------------------------------------------------------------------------
def test_two_scans_two_tables_and_the_near_pass_beside_them():
    from krisp_amd import _native
    name, M = "g20_tttv", 2
    c = GC.case(name, M)
    want = GC.reference(name, M, False)
    with _native.Engine() as eng:
        _locate(eng, c["G"], False, GC.N_TEXT, False)
        eng.upload(0, c["text"])
        eng.guide_hits_table(_texts(c["guides"]), M, c["pam5"], c["pam3"])
        first = eng.guide_hits(0)
        again = eng.guide_hits(0)
        assert len(first) == len(want) > 0 and first.tobytes() == again.tobytes()
        # a near table and a near scan in between, of other texts and another distance: each pass keeps its own
        targets = _texts(GC.guides("g20_none")[:3])
        eng.near_table(targets, 1)
        near = eng.near(0)
        assert eng.guide_hits(0).tobytes() == first.tobytes()
        _check(eng, c["text"], c["G"], want)
        # another G, another M on the same engine
        other, M2 = "g12_h", 1
        c2 = GC.case(other, M2)
        _locate(eng, c2["G"], False, GC.N_TEXT, True)
        eng.upload(0, c2["text"])
        eng.guide_hits_table(_texts(c2["guides"]), M2, c2["pam5"], c2["pam3"])
        _check(eng, c2["text"], c2["G"], GC.reference(other, M2, False))
        # ... and the near pass afterwards on a small text: its own result (the definition without motifs names the same
        # windows: target = guide, no flank)
        g12 = GC.guides("g12_none")[:5]
        small = ("TG".join(g12) + "\n" + "N".join(ref.rc(g)[:7] + "A" + ref.rc(g)[8:] for g in g12)).encode("ascii")
        eng.upload(0, small)
        eng.near_table(_texts(g12), 1)
        near2 = eng.near(0)
        want_near = ref.ref_hits(small, False, g12, 1)
        order = np.lexsort((near2["target"], near2["strand"], near2["pos"]))
        assert len(near2) == len(want_near) > 0
        for f, g in (("pos", "pos"), ("strand", "strand"), ("target", "guide"), ("mismatches", "mismatches")):
            assert np.array_equal(near2[f][order].astype(np.int64), want_near[g]), f
        assert not near2["flank_mismatches"].any()
        _check(eng, small, c2["G"], ref.ref_hits(small, False, c2["guides"], M2, c2["pam5"], c2["pam3"]))
    print("hits", len(first), "near between", len(near), "near after", len(near2))


# ----------------------------------------------------------------------------
# 5. the library's refusals
# ----------------------------------------------------------------------------
def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    P, CAP, STATE = -2, -3, -4
    guide = "ACGTTGCAAGCTTGACCTGA"
    text = (b"TTTC" + guide.encode() + b"CAGT") * 3
    t = _texts([guide])
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731

    def code(f):
        with pytest.raises(_native.KrispHipError) as e:
            f()
        assert "kr_guide_hits" in str(e.value) or "kr_set_params_locate" in str(e.value)
        return e.value.code

    with _native.Engine() as eng:
        assert code(lambda: eng.guide_hits_table(t, 1)) == STATE               # no locate context
        # G outside 12 .. 40
        uploaded = False
        for G in (11, 41):
            _locate(eng, G, False, 1000, uploaded)
            assert code(lambda: eng.guide_hits_table(_texts(["A" * G]), 1)) == P
        _locate(eng, 20, False, 1000, False)
        out = np.zeros(4, dtype=_native.GUIDE_HIT_RAW)
        assert code(lambda: eng.guide_hits(0)) == P                            # a scan before a table
        for wrong in (_texts(["A" * 19]), _texts(["A" * 21]), np.frombuffer(guide.encode("ascii"), dtype=np.uint8)):
            with pytest.raises(ValueError):                                    # (the binding: rows of another width)
                eng.guide_hits_table(wrong, 1)
        assert eng.lib.kr_guide_hits_fetch(eng.ctx, ptr(out), 4) == STATE
        eng.upload(0, text)
        assert code(lambda: eng.guide_hits(0)) == P                            # ... also with a genome
        for M in (-1, 4):
            assert code(lambda: eng.guide_hits_table(t, M)) == P
        for bad in ("ACGTTGCAAGCTTGACCTGN", "ACGTTGCAAGCTTGACCTGa", "ACGTTGCAAGCTTGACCTG\n", "RCGTTGCAAGCTTGACCTGA"):
            assert code(lambda: eng.guide_hits_table(_texts([guide, bad]), 1)) == P
        assert code(lambda: eng.guide_hits_table(t, 1, pam5="NNNNNTTTV")) == P
        assert code(lambda: eng.guide_hits_table(t, 1, pam3="HNNNNNNNN")) == P
        assert code(lambda: eng.guide_hits_table(t, 1, pam5="TTJ")) == P
        assert code(lambda: eng.guide_hits_table(t, 1, pam3="T-")) == P
        assert eng.lib.kr_guide_hits_table(eng.ctx, None, 1, 1, None, None, 0) == P          # a null pointer with a count
        assert b"null" in eng.lib.kr_last_error(eng.ctx)
        assert eng.lib.kr_guide_hits_table(eng.ctx, ptr(t), 1 << 24, 1, None, None, 0) == CAP  # (refused before a byte is read)
        assert b"guides" in eng.lib.kr_last_error(eng.ctx)
        assert code(lambda: eng.guide_hits(0)) == P                            # none of them left a table behind
        # a valid scan on the same engine
        eng.guide_hits_table(t, 1, pam5="tttv", pam3="")
        got = eng.guide_hits(0)
        want = ref.ref_hits(text, False, [guide], 1, "TTTV", "")
        assert len(got) == len(want) == 3 and (got["pam"] == 3).all()
        # a refused table leaves the table that was there
        assert code(lambda: eng.guide_hits_table(t, 4)) == P
        assert eng.guide_hits(0).tobytes() == got.tobytes()
        assert eng.lib.kr_guide_hits_fetch(eng.ctx, ptr(out), 2) == CAP and eng.lib.kr_guide_hits_fetch(eng.ctx, ptr(out), 4) == 3
        assert out[:3].tobytes() == got.tobytes()
        # no guides, a genome shorter than G: no hits
        eng.guide_hits_table(np.empty((0, 20), dtype=np.uint8), 1)
        assert len(eng.guide_hits(0)) == 0 and eng.guide_hit_windows(20).shape == (0, 20)
        eng.guide_hits_table(t, 0)
        eng.upload(0, text[:19])
        assert len(eng.guide_hits(0)) == 0
        eng.free(0)
        assert code(lambda: eng.guide_hits(0)) == STATE                        # no genome


# ----------------------------------------------------------------------------
# 6. the command line
# ----------------------------------------------------------------------------
def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _columns(mask):
    return ",".join(str(c + 1) for c in range(64) if (mask >> c) & 1) or "-"


def _host_rows(files, texts, text_regions, G, M, pam5, pam3, need, omit):
    """the file's rows from the definition: every input file's records as the host reader yields them, joined as they are
    uploaded"""
    rows = []
    for fi, path in enumerate(files):
        recs = fasta.read_records(path)
        rna = bool(fasta.detect_rna(recs))
        assert not rna                                  # (the case is DNA: no U to write back)
        ids = py_record_ids(fasta._read_raw_lines(path))
        assert len(ids) == len(recs)
        joined = b"\n".join(recs)
        starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])])
        hits = ref.ref_hits(joined, omit, texts, M, pam5, pam3, need)
        seqs = ref.ref_windows(joined, hits, G)
        for h, seq in zip(hits, seqs):
            pos = int(h["pos"])
            ri = int(np.searchsorted(starts, pos, side="right")) - 1
            start = pos - int(starts[ri])
            for region in text_regions[int(h["guide"])]:
                rows.append((region, fi, path, ids[ri], ri, start, start + G, "+-"[int(h["strand"])], int(h["mismatches"]),
                             _columns(int(h["columns"])), int(h["pam"]) & 1, int(h["pam"]) >> 1, seq))
    rows.sort(key=lambda r: (r[0], r[1], r[4], r[5], r[7] == "-"))
    return rows


@pytest.mark.parametrize("design", [False, True], ids=["plain", "design_primers"])
def test_the_command_line_on_c1_30_40_30(design, tmp_path):
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    omit = case["omit_soft"]
    if design:
        g, pam5, pam3, gc, min_mm, M = 20, "TV", "", (20, 80), 0, 1
        opts = _design_options(case)
        for name, v in opts.items():
            argv += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
        argv += ["--design-primers"]
    else:
        g, pam5, pam3, gc, min_mm, M = 28, "", "H", (30, 70), 0, None        # (None: the default of 2)
    flags = ["--guide-size", str(g), "--guide-gc", str(gc[0]), str(gc[1]), "--guide-min-mismatches", str(min_mm)]
    flags += (["--pam5", pam5] if pam5 else []) + (["--pam3", pam3] if pam3 else [])
    f = {n: str(tmp_path / n) for n in ("a.align", "b.align", "a.guides", "b.guides", "hits.tsv", "need.tsv", "want.tsv", "want_need.tsv")}
    csv_a = _main(argv + flags + ["-o", f["a.align"], "--out_guides", f["a.guides"]])
    hit_flags = ["--out_guide_hits", f["hits.tsv"]] + (["--guide-hit-mismatches", str(M)] if M is not None else [])
    csv_b = _main(argv + flags + ["-o", f["b.align"], "--out_guides", f["b.guides"]] + hit_flags)
    _main(argv + flags + ["--out_guides", f["b.guides"], "--out_guide_hits", f["need.tsv"], "--guide-hits-need-pam"] +
          (["--guide-hit-mismatches", str(M)] if M is not None else []))
    M = 2 if M is None else M
    # every other output keeps its bytes
    assert csv_a == csv_b and csv_a.count("\n") > 1
    assert open(f["a.align"], "rb").read() == open(f["b.align"], "rb").read() and os.path.getsize(f["a.align"]) > 0
    assert open(f["a.guides"], "rb").read() == open(f["b.guides"], "rb").read()

    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], _amplicon(case), omit_soft=omit)
    ingroup = [KF.simplename(p) for p in ing] if out else None
    templates = KF.design_templates(groups, ingroup)
    bounds = regions = None
    if design:
        records = KF.design_primers(groups, ingroup, templates=templates, **opts)
        found = records["found"] != 0
        lo = records["left_start"].astype(np.int64) + records["left_len"]
        bounds = np.where(found[:, None], np.stack([lo, records["right_start"].astype(np.int64)], axis=1), 0).astype(np.uint32)
        regions = np.cumsum(found) - 1
    guides = KF.design_guides(groups, ingroup, g, pam5, pam3, gc, min_mm, bounds=bounds, templates=templates)
    texts, text_regions = KF.guide_texts(templates[0], guides, g, regions=regions)
    glines = open(f["a.guides"]).read().split("\n")[1:-1]
    assert len(texts) > 0 and len(glines) == int((guides["found"] != 0).sum())
    for need, got_path, want_path in ((False, f["hits.tsv"], f["want.tsv"]), (True, f["need.tsv"], f["want_need.tsv"])):
        rows = _host_rows(ing + out, texts, text_regions, g, M, pam5, pam3, need, omit)
        want = np.empty(len(rows), dtype=KF.GUIDE_HIT)
        for i, r in enumerate(rows):
            want[i] = (r[0],) + r[2:]
        KF.write_guide_hits(want_path, want)
        got = open(got_path).read()
        print("design", design, "need_pam", need, "texts", len(texts), "rows", len(rows))
        assert got == open(want_path).read()
        assert got.startswith(KF.GUIDE_HIT_HEADER + "\n") and got.count("\n") == len(rows) + 1
        # a picked guide's own locus: in every ingroup file a row of its region with 0 mismatches and both motifs beside it
        lines = [ln.split("\t") for ln in got.split("\n")[1:-1]]
        for gl in glines:
            region = gl.split("\t")[0]
            for path in ing:
                assert any(ln[0] == region and ln[1] == path and ln[7] == "0" and ln[8] == "-" and ln[9] == "1" and ln[10] == "1"
                           for ln in lines), (region, path)

"""--out_guides on the GPU (kr_guides_*, csrc/k_guides.inc): the device's record of every region equals the reference's
(guides_reference.py) field for field over the option sets, plants and random regions of guide_cases.py; two runs give the
same bytes; a run cut into batches equals the single run; the library's refusals and state errors; the command line end to
end on a golden case, alone and with --design-primers."""
import ctypes
import functools
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_cases                                                         # noqa: E402
import guides_reference as ref                                             # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402
from test_gpu_primers import _design_options                               # noqa: E402

pytestmark = pytest.mark.gpu


def _pack(regs):
    rows, off, bounds = guide_cases.pack(regs)
    k = len(rows[0])
    return (np.frombuffer("".join(rows).encode("ascii"), dtype=np.uint8).reshape(len(rows), k), np.array(off, dtype=np.uint64),
            np.array(bounds, dtype=np.uint32).reshape(-1, 2))


def _records(recs):
    from krisp_amd import _native
    out = np.zeros(len(recs), dtype=_native.GUIDE_RECORD)
    for i, r in enumerate(recs):
        for f in ref.FIELDS:
            out[f][i] = r[f]
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """the set's regions, packed, and the reference's records: computed once, shared, never written to"""
    s = guide_cases.SETS[name]
    regs = guide_cases.regions(name)
    want = _records(ref.guides(regs, s["geo"][0], s["geo"][1], **guide_cases.options(name)))
    return _pack(regs) + (want,)


def _table(eng, name):
    o = guide_cases.options(name)
    eng.guides_table(o["g"], KF.motif_masks(o["pam5"]), KF.motif_masks(o["pam3"]), o["gc"], o["min_mismatches"])


@pytest.mark.parametrize("name", list(guide_cases.SETS))
def test_every_record_equals_the_reference_record(name):
    """all fields of all regions, the padding zero; a second run gives the same bytes"""
    from krisp_amd import _native
    L, D, _ = guide_cases.SETS[name]["geo"]
    rows, off, bounds, want = _case(name)
    with _native.Engine() as eng:
        _table(eng, name)
        got = eng.guides(rows, off, bounds, L, D)
        again = eng.guides(rows, off, bounds, L, D)
    print(name, "regions", len(want), "rows", len(rows), "with a guide", int(want["found"].sum()), "device", int(got["found"].sum()))
    assert got.dtype.itemsize == 32 and len(got) == len(want)
    assert got.tobytes() == again.tobytes()
    for f in ref.FIELDS + ("pad",):
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (f, bad[:5].tolist(), got[f][bad[:5]].tolist(), want[f][bad[:5]].tolist())
    assert got.tobytes() == want.tobytes()


def test_the_batches_of_a_long_list_join_up():
    """more regions than one batch takes (2^18): the records are those of the same regions alone, over and over"""
    from krisp_amd import _native
    name = "12_4_12_g12"
    L, D, _ = guide_cases.SETS[name]["geo"]
    rows, off, bounds, want = _case(name)
    n, nrows = len(want), int(off[-1])
    reps = (1 << 18) // n + 2
    many_off = np.concatenate([(off[:-1][None, :] + (np.arange(reps, dtype=np.uint64) * np.uint64(nrows))[:, None]).ravel(),
                               np.array([reps * nrows], dtype=np.uint64)])
    with _native.Engine() as eng:
        _table(eng, name)
        one = eng.guides(rows, off, bounds, L, D)
        got = eng.guides(np.tile(rows, (reps, 1)), many_off, np.tile(bounds, (reps, 1)), L, D)
    assert reps * n > 1 << 18 and len(got) == reps * n
    assert one.tobytes() == want.tobytes()
    assert got.tobytes() == np.tile(one, reps).tobytes()


def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    P, CAP, STATE = -2, -3, -4
    # (with the motif T the one guide is the window [0, 12) on '-': column 12 holds A; the outgroup row differs at column 8)
    rows = np.frombuffer(b"ACGTACGTACGTAC" + b"ACGTACGTCCGTAC", dtype=np.uint8).reshape(2, 14)

    def code(f):
        with pytest.raises(_native.KrispHipError) as e:
            f()
        return e.value.code, str(e.value)

    with _native.Engine() as eng:
        out = np.zeros(4, dtype=_native.GUIDE_RECORD)
        c, msg = code(lambda: eng.guides(rows, [0, 2], [[0, 14]], 5, 4))
        assert c == STATE and "kr_guides_table first" in msg
        assert eng.lib.kr_guides_fetch(eng.ctx, out.ctypes.data_as(ctypes.c_void_p), 4) == STATE
        for size in (11, 41, 0, -5):
            c, msg = code(lambda: eng.guides_table(size))
            assert c == P and "guide_size" in msg
        assert code(lambda: eng.guides_table(20, pam5=[15] * 9))[0] == P and code(lambda: eng.guides_table(20, pam3=[8] * 9))[0] == P
        assert eng.lib.kr_guides_table(eng.ctx, None) == P
        for bad in (0, 16, 255):
            c, msg = code(lambda: eng.guides_table(20, pam5=[8, bad]))
            assert c == P and "IUPAC mask" in msg
            assert code(lambda: eng.guides_table(20, pam3=[bad]))[0] == P
        # a table that was refused leaves no table behind
        eng.guides_table(12)
        assert len(eng.guides(rows, [0, 2], [[0, 14]], 5, 4)) == 1
        assert code(lambda: eng.guides_table(11))[0] == P
        assert code(lambda: eng.guides(rows, [0, 2], [[0, 14]], 5, 4))[0] == STATE
        assert eng.lib.kr_guides_fetch(eng.ctx, out.ctypes.data_as(ctypes.c_void_p), 4) == STATE
        # the run's own refusals; none of them leaves records behind
        eng.guides_table(12, pam5=[8])
        ok = eng.guides(rows, [0, 2], [[0, 14]], 5, 4)
        assert len(ok) == 1 and [int(ok[f][0]) for f in ref.FIELDS] == [1, 1, 0, 1, 1, 6, 1]
        assert code(lambda: eng.guides(rows[:, :11], [0, 2], [[0, 11]], 5, 4))[0] == P                        # K < guide_size
        assert eng.lib.kr_guides_fetch(eng.ctx, out.ctypes.data_as(ctypes.c_void_p), 4) == STATE
        assert code(lambda: eng.guides(np.zeros((1, 2048), dtype=np.uint8), [0, 1], [[0, 2048]], 5, 4))[0] == P   # K > 2047
        assert code(lambda: eng.guides(rows, [0, 2], [[0, 14]], 12, 4))[0] == P                               # L + D > K
        assert code(lambda: eng.guides(rows, [0, 2], [[9, 8]], 5, 4))[0] == P                                 # lo > hi
        assert code(lambda: eng.guides(rows, [0, 2], [[0, 15]], 5, 4))[0] == P                                # hi > K
        assert code(lambda: eng.guides(rows, [0, 1, 1], [[0, 14], [0, 14]], 5, 4))[0] == P                    # no template
        assert code(lambda: eng.guides(rows, [0, 2, 1], [[0, 14], [0, 14]], 5, 4))[0] == P                    # descending
        assert code(lambda: eng.guides(rows, [1, 2], [[0, 14]], 5, 4))[0] == P                                # row_off[0] != 0
        off = np.array([0, 2], dtype=np.uint64)
        bnd = np.array([0, 14], dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                                     # noqa: E731
        assert eng.lib.kr_guides_run(eng.ctx, None, ptr(off), ptr(bnd), 1, 14, 5, 4) == P                     # null pointers
        assert eng.lib.kr_guides_run(eng.ctx, ptr(rows), None, ptr(bnd), 1, 14, 5, 4) == P
        assert eng.lib.kr_guides_run(eng.ctx, ptr(rows), ptr(off), None, 1, 14, 5, 4) == P
        assert eng.lib.kr_guides_run(eng.ctx, ptr(rows), ptr(off), ptr(bnd), 1, 14, 5, 4) == 1
        assert eng.lib.kr_guides_fetch(eng.ctx, ptr(out), 0) == CAP and eng.lib.kr_guides_fetch(eng.ctx, ptr(out), 4) == 1
        assert out[:1].tobytes() == ok.tobytes()
        # no region: no record
        assert len(eng.guides(np.empty((0, 14), dtype=np.uint8), [0], np.empty((0, 2), dtype=np.uint32), 5, 4)) == 0
        # K = 2047 fits the LDS of a workgroup
        assert len(eng.guides(np.full((1, 2047), ord("A"), dtype=np.uint8), [0, 1], [[0, 2047]], 1000, 47)) == 1


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _recount(lines, templates, rows, off, bounds, g, pam5, pam3, min_mm, region_of):
    """every written guide, placed back on its template: the window, the motifs, the bounds and the mismatches counted here"""
    for ln in lines:
        region, strand, start, end, m5, m3, proto, gc, dmin, ssum, cands = ln.split("\t")
        gi = region_of[int(region)]
        T = templates[gi]
        p, e = int(start), int(end)
        lo, hi = bounds[gi]
        assert e - p == g == len(proto) and len(m5) == len(pam5) and len(m3) == len(pam3) and int(cands) >= 1
        if strand == "+":
            assert T[p:e] == proto and T[p - len(m5):p] == m5 and T[e:e + len(m3)] == m3
            assert lo <= p - len(m5) and e + len(m3) <= hi
        else:
            assert strand == "-" and ref.rc(T[p:e]) == proto and ref.rc(T[e:e + len(m5)]) == m5 and ref.rc(T[p - len(m3):p]) == m3
            assert lo <= p - len(m3) and e + len(m5) <= hi
        assert all(x in ref.IUPAC[m] for x, m in zip(m5, pam5)) and all(x in ref.IUPAC[m] for x, m in zip(m3, pam3))
        assert set(proto) <= set("ACGT")
        outs = rows[int(off[gi]) + 1:int(off[gi + 1])]
        mm = [sum(1 for c in range(p, e) if o[c] in "ACGT" and o[c] != T[c]) for o in outs]
        assert int(dmin) == (min(mm) if mm else g) >= min_mm and int(ssum) == sum(mm)
        assert float(gc) == pytest.approx(100 * sum(proto.count(x) for x in "GC") / g, abs=1e-3)


@pytest.mark.parametrize("design", [False, True], ids=["plain", "design_primers"])
def test_the_command_line_on_c1_30_40_30(design, tmp_path):
    """the file is write_guides over the reference's records on the same groups; every guide recounted; the CSV and the
    alignments are those of the same command without the option"""
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    if design:
        g, pam5, pam3, gc, min_mm = 20, "TV", "", (20, 80), 0
        opts = _design_options(case)
        for name, v in opts.items():
            argv += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
        argv += ["--design-primers"]
    else:
        # (the case's two regions hold the ingroup's own difference in their diagnostic column: the template has an IUPAC
        # letter there, and the windows beside it do not differ from the outgroup -- guides only with 0 mismatches asked for)
        g, pam5, pam3, gc, min_mm = 28, "", "H", (30, 70), 0
    flags = ["--guide-size", str(g), "--guide-gc", str(gc[0]), str(gc[1]), "--guide-min-mismatches", str(min_mm)]
    flags += (["--pam5", pam5] if pam5 else []) + (["--pam3", pam3] if pam3 else [])
    f = {n: str(tmp_path / n) for n in ("plain.align", "guides.align", "g.tsv", "g_again.tsv", "want.tsv")}
    csv_plain = _main(argv + ["-o", f["plain.align"]])
    csv_guides = _main(argv + flags + ["-o", f["guides.align"], "--out_guides", f["g.tsv"]])
    _main(argv + flags + ["--out_guides", f["g_again.tsv"]])
    assert csv_plain == csv_guides and csv_plain.count("\n") > 1
    if not design:
        assert csv_plain == case["csv"]
    assert open(f["plain.align"], "rb").read() == open(f["guides.align"], "rb").read() and os.path.getsize(f["plain.align"]) > 0
    assert open(f["g.tsv"], "rb").read() == open(f["g_again.tsv"], "rb").read()

    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], _amplicon(case), omit_soft=case["omit_soft"])
    ingroup = [KF.simplename(p) for p in ing] if out else None
    trows, L, D, R = KF.design_templates(groups, ingroup)
    rows, off, _, _, _ = KF.guide_rows(groups, ingroup)
    text = [bytes(r).decode("ascii") for r in rows]
    templates = [text[int(o)] for o in off[:-1]]
    assert templates == [bytes(r).decode("ascii") for r in trows] and int(off[-1]) > len(groups)      # (outgroup rows exist)
    if design:
        records = KF.design_primers(groups, ingroup, **opts)
        found = records["found"] != 0
        bounds = [(int(r["left_start"]) + int(r["left_len"]), int(r["right_start"])) if int(r["found"]) else (0, 0) for r in records]
        regions = np.cumsum(found) - 1
        region_of = np.flatnonzero(found)
        assert 0 < found.sum()
    else:
        bounds, regions, region_of = [(0, L + D + R)] * len(groups), None, np.arange(len(groups))
    regs = [(text[int(off[i]):int(off[i + 1])], bounds[i][0], bounds[i][1]) for i in range(len(groups))]
    want = _records(ref.guides(regs, L, D, g, pam5, pam3, gc, min_mm))
    KF.write_guides(f["want.tsv"], trows, want, g, len(pam5), len(pam3), regions=regions)
    got = open(f["g.tsv"]).read()
    print("regions", len(groups), "rows", len(rows), "with a guide", int(want["found"].sum()), "lines", got.count("\n") - 1)
    assert got == open(f["want.tsv"]).read()
    lines = got.split("\n")
    assert lines[0] == KF.GUIDE_HEADER and lines[-1] == "" and len(lines) - 2 == int(want["found"].sum())
    _recount(lines[1:-1], templates, text, off, bounds, g, pam5, pam3, min_mm, region_of)
    if not design:
        # (H leaves three letters in four, and some 70 windows of a region lie beside its diagnostic column)
        assert len(lines) > 2
        # ... and with the default of 1 mismatch the file is its header
        _main(argv + ["--pam3", "H", "--out_guides", f["g_again.tsv"]])
        assert open(f["g_again.tsv"]).read() == KF.GUIDE_HEADER + "\n"

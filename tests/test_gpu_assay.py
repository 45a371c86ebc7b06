"""--out_assay_hits on the GPU (kr_assay_*, csrc/k_assay.inc): the device's assay hits against the brute-force
definition (assay_reference.py) list for list on the texts of assay_cases.py; the join leaves the two passes' lists as they
were; what the library refuses; the command line on the golden c1 files, whose file equals the join of the two files the
project wrote before, computed here in Python."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assay_cases as AC                                                    # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _argv, _files                                  # noqa: E402
from test_gpu_primers import _design_options                               # noqa: E402

pytestmark = pytest.mark.gpu

KR_ERR_PARAM, KR_ERR_STATE = -2, -4         # include/krisp_hip.h


def _engine(c, native):
    eng = native.Engine()
    eng.set_params_locate(0, c["G"], 0, c["omit"], max_bases=len(c["text"]))
    eng.upload(0, np.frombuffer(c["text"], dtype=np.uint8))
    return eng


def _tables(eng, c, links=True):
    eng.primers_table(c["left"] + c["right"], len(c["left"]), c["pairs"], c["Mp"], c["max_product"])
    eng.guide_hits_table(np.frombuffer(b"".join(c["guides"]), dtype=np.uint8).reshape(-1, c["G"]), c["Mg"], c["pam5"], c["pam3"],
                         c["need"])
    if links:
        eng.assay_table(c["links"])


def _fetch_lists(eng, native, G, n_products, n_hits):
    """the four fetches of the two passes, without a scan -> their bytes"""
    sites = eng.primer_sites()
    windows = eng.guide_hit_windows(G)
    prods = np.empty(max(n_products, 1), dtype=native.PRODUCT_HIT)
    assert eng.lib.kr_primers_fetch(eng.ctx, native._ptr(prods), n_products) == n_products
    hits = np.empty(max(n_hits, 1), dtype=native.GUIDE_HIT_RAW)
    assert eng.lib.kr_guide_hits_fetch(eng.ctx, native._ptr(hits), n_hits) == n_hits
    assert len(windows) == n_hits
    return prods[:n_products].tobytes(), sites.tobytes(), hits[:n_hits].tobytes(), windows.tobytes()


@pytest.mark.parametrize("name", AC.NAMES)
def test_every_case_equals_the_reference_list_for_list(name):
    """the products and the hits equal their references, the assay hits equal ref_assay_hits element for element, `hit` names
    the hit in the pass's list; a second join gives the same bytes; the two passes' lists have the same bytes after the join
    as before it"""
    from krisp_amd import _native
    c = AC.case(name)
    want_p, want_h, want = AC.reference(name)
    with _engine(c, _native) as eng:
        _tables(eng, c)
        counts = eng.primers_scan(0), eng.guide_hits_scan(0)
        before = _fetch_lists(eng, _native, c["G"], *counts)
        n = eng.assay_join(0)
        rows = eng.assay_hits()
        after = _fetch_lists(eng, _native, c["G"], *counts)
        assert eng.assay_join(0) == n
        again = eng.assay_hits()
        after_again = _fetch_lists(eng, _native, c["G"], *counts)
    prods = np.frombuffer(before[0], dtype=_native.PRODUCT_HIT)
    hits = np.frombuffer(before[2], dtype=_native.GUIDE_HIT_RAW)
    print(name, "products", len(prods), "hits", len(hits), "assay hits", n, "want", len(want))
    assert len(prods) == len(want_p) and len(hits) == len(want_h)
    assert list(zip(prods["pos"].tolist(), prods["length"].tolist(), prods["strand"].tolist(), prods["pair"].tolist())) == \
        list(zip(want_p["pos"].tolist(), want_p["length"].tolist(), want_p["strand"].tolist(), want_p["pair"].tolist()))
    assert sorted(zip(hits["pos"].tolist(), hits["strand"].tolist(), hits["guide"].tolist())) == \
        list(zip(want_h["pos"].tolist(), want_h["strand"].tolist(), want_h["guide"].tolist()))
    got = list(zip(*(rows[f].tolist() for f in ("pos", "length", "strand", "pair", "hit_pos", "hit_strand", "guide", "left_mm", "right_mm",
                                                "left_end_mm", "right_end_mm", "hit_mismatches", "columns", "hit_pam"))))
    assert n == len(rows) == len(want)
    assert got == [tuple(r) for r in want.tolist()]
    assert rows.tobytes() == again.tobytes()
    assert before == after == after_again
    if n:
        h = hits[rows["hit"]]
        assert (h["pos"] == rows["hit_pos"]).all() and (h["guide"] == rows["guide"]).all() and (h["strand"] == rows["hit_strand"]).all()


def test_the_join_is_of_one_genome_and_of_the_standing_tables():
    from krisp_amd import _native
    c = AC.case("spread_m1_m2")

    def state(eng, word):
        with pytest.raises(Exception, match=word) as e:
            eng.assay_join(0)
        assert e.value.code == KR_ERR_STATE

    with _engine(c, _native) as eng:
        eng.upload(1, np.frombuffer(c["text"][:5000], dtype=np.uint8))
        with pytest.raises(Exception, match="kr_primers_table first") as e:
            eng.assay_table(c["links"])
        assert e.value.code == KR_ERR_STATE
        eng.primers_table(c["left"] + c["right"], len(c["left"]), c["pairs"], c["Mp"], c["max_product"])
        with pytest.raises(Exception, match="kr_guide_hits_table first") as e:
            eng.assay_table(c["links"])
        assert e.value.code == KR_ERR_STATE
        _tables(eng, c, links=False)
        state(eng, "kr_assay_table first")
        for bad, word in (([(0, 0), (0, 0)], "ascending"), ([(1, 1), (0, 0)], "ascending"), ([(5, 0)], "names"), ([(0, 3)], "names")):
            with pytest.raises(Exception, match=word) as e:
                eng.assay_table(bad)
            assert e.value.code == KR_ERR_PARAM
        state(eng, "kr_assay_table first")          # (a refused table makes none)
        eng.assay_table(c["links"])
        state(eng, "kr_primers_scan first")
        eng.primers_scan(0)
        state(eng, "kr_guide_hits_scan first")
        eng.guide_hits_scan(0)
        n = eng.assay_join(0)
        assert n == len(AC.reference("spread_m1_m2")[2]) > 0
        # a scan of another genome, by either pass
        eng.primers_scan(1)
        state(eng, "genome 0, but the products are of genome 1")
        with pytest.raises(Exception, match="kr_assay_join first"):
            eng.assay_hits()
        eng.primers_scan(0)
        eng.guide_hits_scan(1)
        state(eng, "the hits of genome 1")
        eng.guide_hits_scan(0)
        assert eng.assay_join(0) == n
        # a new table for either pass drops the links and its list
        eng.primers_table(c["left"] + c["right"], len(c["left"]), c["pairs"], c["Mp"], c["max_product"])
        state(eng, "kr_assay_table first")
        eng.assay_table(c["links"])
        state(eng, "kr_primers_scan first")
        eng.primers_scan(0)
        assert eng.assay_join(0) == n
        eng.guide_hits_table(np.frombuffer(b"".join(c["guides"]), dtype=np.uint8).reshape(-1, c["G"]), c["Mg"], "", "", False)
        state(eng, "kr_assay_table first")
        eng.assay_table(c["links"])
        state(eng, "kr_guide_hits_scan first")
        eng.guide_hits_scan(0)
        assert eng.assay_join(0) == n
        # no links: 0
        eng.assay_table([])
        assert eng.assay_join(0) == 0 and len(eng.assay_hits()) == 0


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0], [ln.split("\t") for ln in lines[1:-1]]


def test_the_command_line_on_c1_30_40_30(tmp_path):
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    for name, v in _design_options(case).items():
        argv += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
    G = 20
    argv += ["--design-primers", "--guide-size", str(G), "--guide-gc", "20", "80", "--guide-min-mismatches", "0", "--pam5", "TV",
             "--guide-hit-mismatches", "1", "--primer-mismatches", "1"]
    f = {n: str(tmp_path / n) for n in ("a.align", "a.guides", "a.pp", "a.gh", "b.align", "b.guides", "b.pp", "b.gh", "b.assay", "c.guides",
                                        "c.assay")}
    csv_a = _main(argv + ["-o", f["a.align"], "--out_guides", f["a.guides"], "--out_primer_products", f["a.pp"], "--out_guide_hits", f["a.gh"]])
    csv_b = _main(argv + ["-o", f["b.align"], "--out_guides", f["b.guides"], "--out_primer_products", f["b.pp"], "--out_guide_hits", f["b.gh"],
                          "--out_assay_hits", f["b.assay"]])
    _main(argv + ["--out_guides", f["c.guides"], "--out_assay_hits", f["c.assay"]])
    # every other output keeps its bytes; the option alone writes the same file
    assert csv_a == csv_b and csv_a.count("\n") > 1
    for n in ("align", "guides", "pp", "gh"):
        assert open(f["a." + n], "rb").read() == open(f["b." + n], "rb").read() and os.path.getsize(f["a." + n]) > 0, n
    assert open(f["b.assay"], "rb").read() == open(f["c.assay"], "rb").read()

    # the join of the two files in Python: by region, file, record_index and containment
    header = csv_a.split("\n")[0].split(",")
    data = [ln.split(",") for ln in csv_a.split("\n")[1:-1]]
    llen = [int(r[header.index("left_length")]) for r in data]
    rlen = [int(r[header.index("right_length")]) for r in data]
    _, guides = _table(f["b.guides"])
    s_d = {int(g[0]): "+-".index(g[1]) for g in guides}
    ph, prods = _table(f["b.pp"])
    gh, hits = _table(f["b.gh"])
    assert ph == KF.PRODUCT_HEADER and gh == KF.GUIDE_HIT_HEADER and len(prods) > 0 and len(hits) > 0 and len(s_d) > 0
    files = ing + out
    want = []
    for P in prods:
        region, s_p = int(P[0]), "+-".index(P[6])
        first, second = (llen[region], rlen[region]) if s_p == 0 else (rlen[region], llen[region])
        lo, hi = int(P[4]) + first, int(P[5]) - second
        for H in hits:
            if H[0] != P[0] or H[1] != P[1] or H[3] != P[3] or not (lo <= int(H[4]) and int(H[5]) <= hi):
                continue
            s_h = "+-".index(H[6])
            want.append((region, files.index(P[1]), int(P[3]), int(P[4]), int(P[5]), s_p, int(H[4]), s_h,
                         P[:12] + [H[4], H[5], H[6], H[7], H[8], H[9], H[10],
                                            "design" if (s_h ^ s_p) == s_d[region] else "reverse", H[11]]))
    want.sort(key=lambda r: r[:8])
    ah, rows = _table(f["b.assay"])
    print("products", len(prods), "hits", len(hits), "assay rows", len(rows), "want", len(want))
    assert ah == KF.ASSAY_HIT_HEADER
    assert rows == [r[8] for r in want] and len(rows) > 0
    # the designed locus: in every ingroup genome, for every region with a pair and a guide, a row without a mismatch,
    # both motifs beside it, on the strand the design put it on
    for region in s_d:
        for path in ing:
            assert any(r[0] == str(region) and r[1] == path and r[8:12] == ["0"] * 4 and r[15] == "0" and r[16] == "-" and
                       r[17:20] == ["1", "1", "design"] for r in rows), (region, path)

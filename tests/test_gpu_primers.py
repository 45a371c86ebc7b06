"""--out_primer_products on the GPU (kr_primers_*, csrc/k_primers.inc): the device's complete site and product lists against
the brute-force definition (primers_reference.py) on the texts of primer_cases.py, for every length set, distance and
soft-mask mode; byte equality with the flank pass (kr_products_*) where the lengths are uniform; the library's refusals;
the relation to the locate pass through the designed pairs on the golden cases; the command line end to end."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import codec
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primer_cases as PC                                                  # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402
from test_gpu_products import _case as flank_case, _u8                     # noqa: E402
from test_gpu_design import E2E_CASES                                      # noqa: E402

pytestmark = pytest.mark.gpu

KR_ERR_PARAM = -2                   # include/krisp_hip.h


# ----------------------------------------------------------------------------
# the lists
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.LENGTH_SETS))
def test_sites_and_products_equal_the_brute_force_lists(name):
    """M = 0 .. 3, omit off and on: the device's sites (sorted by (pos, entry)) and products equal ref_sites / ref_products
    element for element; a second scan gives the same bytes; the pad fields are zero; positions ascend as the device
    lists the sites.  (test_primers_host.py holds the reference's lists to what the generator plants.)"""
    from krisp_amd import _native
    for M in range(4):
        text, left, right, pairs, _ = PC.case(name, M)
        for omit in (False, True):
            with _native.Engine() as eng:
                eng.set_params_locate(30, 40, 30, omit, max_bases=len(text))
                eng.upload(0, np.frombuffer(text, dtype=np.uint8))
                eng.primers_table(left + right, len(left), pairs, M, PC.MAX_PRODUCT)
                hits = eng.primer_products(0)
                sites = eng.primer_sites()
                again = eng.primer_products(0)
                sites_again = eng.primer_sites()
            assert hits.tobytes() == again.tobytes() and sites.tobytes() == sites_again.tobytes()
            assert not sites["pad"].any() and not hits["pad"].any()
            assert sites["pos"].tolist() == sorted(sites["pos"].tolist())
            want_s, want_p = PC.reference(name, M, omit)
            got_s = sorted(zip(sites["pos"].tolist(), sites["entry"].tolist(), sites["mismatches"].tolist(),
                               sites["end_mismatches"].tolist()))
            got_p = list(zip(hits["pos"].tolist(), hits["length"].tolist(), hits["strand"].tolist(), hits["pair"].tolist(),
                             hits["left_mm"].tolist(), hits["right_mm"].tolist(), hits["left_end_mm"].tolist(),
                             hits["right_end_mm"].tolist()))
            print(name, "M", M, "omit", omit, "sites", len(got_s), "want", len(want_s), "products", len(got_p), "want", len(want_p))
            assert len(want_s) > 0 and len(want_p) >= 16
            assert got_s == list(want_s)
            assert got_p == list(want_p)


@pytest.mark.parametrize("Le,Re", [(16, 16), (12, 30)])
def test_with_uniform_lengths_the_bytes_are_the_flank_passes(Le, Re):
    """all left texts of Le letters and all right texts of Re: kr_primers_fetch gives kr_products_fetch's bytes, the sorted
    sites are equal"""
    from krisp_amd import _native
    for M in range(4):
        text, left, right, pairs = flank_case(100 * Le + 10 * Re + M, Le, Re, M)
        with _native.Engine() as eng:
            eng.set_params_locate(Le, 4, Re, False, max_bases=len(text))
            eng.upload(0, np.frombuffer(text, dtype=np.uint8))
            eng.products_table(_u8(left), _u8(right), pairs, M, 520)
            want = eng.products(0)
            want_sites = eng.product_sites()
            eng.primers_table(left + right, len(left), pairs, M, 520)
            got = eng.primer_products(0)
            got_sites = eng.primer_sites()
            assert eng.products(0).tobytes() == want.tobytes()     # (the two passes keep their own state)
        print("Le", Le, "Re", Re, "M", M, "sites", len(got_sites), "products", len(got))
        assert len(want) >= 16 and got.tobytes() == want.tobytes()
        assert np.sort(got_sites, order=["pos", "entry"]).tobytes() == np.sort(want_sites, order=["pos", "entry"]).tobytes()
        assert got_sites["pos"].tolist() == sorted(got_sites["pos"].tolist())


def test_the_library_refuses_what_it_does_not_take():
    from krisp_amd import _native
    a, b = b"ACGTACGTAC", b"GGATCCATTGCA"
    with _native.Engine() as eng:
        eng.set_params_locate(10, 4, 10, False, max_bases=1000)
        eng.upload(0, np.frombuffer(b"ACGT" * 100, dtype=np.uint8))
        with pytest.raises(Exception, match="kr_primers_table first"):
            eng.primer_products(0)
        for bad in (a[:9], a * 6 + b"A"):
            with pytest.raises(Exception, match="10 .. 60 are taken") as e:
                eng.primers_table([a, bad], 1, [(0, 0)], 1, 100)
            assert e.value.code == KR_ERR_PARAM
        with pytest.raises(Exception, match="repeats"):
            eng.primers_table([a, b], 1, [(0, 0), (0, 0)], 1, 100)
        with pytest.raises(Exception, match="names text"):
            eng.primers_table([a, b], 1, [(0, 1)], 1, 100)
        with pytest.raises(Exception, match="names text"):
            eng.primers_table([a, b], 1, [(1, 0)], 1, 100)
        with pytest.raises(Exception, match="shorter than the two texts of pair 1"):
            eng.primers_table([a, b, a], 1, [(0, 1), (0, 0)], 1, 21)
        for M in (-1, 4):
            with pytest.raises(Exception, match="mismatches <= 3"):
                eng.primers_table([a, b], 1, [(0, 0)], M, 100)
        with pytest.raises(Exception, match="kr_primers_table first"):    # (a refused table is no table)
            eng.primer_products(0)
        eng.primers_table([a, a], 1, [(0, 0)], 0, 100)
        with pytest.raises(Exception, match="kr_products_table first"):
            eng.products(0)
        hits = eng.primer_products(0)
        # ACGTACGTAC at 0, 4, 8, ...; its reverse complement GTACGTACGT at 2, 6, ...
        from primers_reference import ref_products
        want = ref_products(b"ACGT" * 100, False, [a, a], 1, [(0, 0)], 0, 100)
        assert len(hits) == len(want) > 0 and hits["pos"].tolist() == want["pos"].tolist()
        assert set(hits["strand"].tolist()) == {0, 1}


# ----------------------------------------------------------------------------
# the relation that makes the feature believable: the designed product lies where the region lies
# ----------------------------------------------------------------------------
def _design_options(case):
    """test_gpu_design's recipe: primers of the last sizes that fit the flanks, loose filters"""
    k = _amplicon(case)
    Le, De, Re = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
    h = min(Le, Re, 20)
    return dict(tm=(30, 75), gc=(20, 80), amp_size=(Le + De + Re - 4, Le + De + Re), primer_size=(h - 1, h), max_sec_tm=35,
                gc_clamp=0, max_end_gc=5)


def test_every_location_of_a_region_with_a_pair_is_an_exact_product_of_the_design_size(tmp_path):
    names = [c["name"] for c in E2E_CASES]
    assert "c1_30_40_30" in names and len(names) >= 12
    with_rows, expected = [], []
    for n, case in enumerate(E2E_CASES):
        d = tmp_path / str(n)
        d.mkdir()
        ing, out = _files(case, d)
        k, L, R, omit = _amplicon(case), case["L"], case["R"], case["omit_soft"]
        groups, _ = KF.find_regions(ing, out, L, R, k, omit_soft=omit)
        ingroup = [KF.simplename(f) for f in ing] if out else None
        records = KF.design_primers(groups, ingroup, **_design_options(case))
        locs = KF.locate_regions(groups, ing, out, L, R, k, omit_soft=omit)
        prods = KF.primer_products(groups, records, ingroup, ing, out, L, R, k, mismatches=1, max_product=max(1000, k),
                                   omit_soft=omit)
        rank = np.cumsum(records["found"] != 0) - 1 if len(records) else np.empty(0, dtype=np.int64)
        want = []
        for r in locs:
            rec = records[int(r["region"])]
            if not int(rec["found"]):
                continue
            lo, hi = int(rec["left_start"]), int(rec["right_start"]) + int(rec["right_len"])
            assert hi - lo == int(rec["product_size"])
            if r["strand"] == "-":
                lo, hi = k - hi, k - lo             # mirrored through the window
            want.append((int(rank[int(r["region"])]), r["file"], int(r["record_index"]), int(r["start"]) + lo, int(r["start"]) + hi,
                         r["strand"], hi - lo))
        exact = prods[(prods["left_mismatches"] == 0) & (prods["right_mismatches"] == 0)]
        rows = set(zip(exact["region"].tolist(), exact["file"], exact["record_index"].tolist(), exact["start"].tolist(),
                       exact["end"].tolist(), exact["strand"], exact["length"].tolist()))
        assert len(rows) == len(exact)
        print(case["name"], "regions", len(groups), "with a pair", int((records["found"] != 0).sum()) if len(records) else 0,
              "locations of those", len(want), "products", len(prods), "exact", len(exact))
        assert set(want) <= rows, case["name"]
        assert (prods["end"] - prods["start"] == prods["length"]).all()
        assert not (exact["left_end_mismatches"].any() or exact["right_end_mismatches"].any())
        assert len(prods) == 0 or int(prods["region"].max()) <= int(rank[-1])
        order = list(zip(prods["region"].tolist(), [(ing + out).index(f) for f in prods["file"]], prods["record_index"].tolist(),
                         prods["start"].tolist(), prods["end"].tolist(), (prods["strand"] == "-").tolist()))
        assert order == sorted(order)
        if len(want):
            expected.append(case["name"])
        if len(prods):
            with_rows.append(case["name"])
    print("cases with rows:", with_rows)
    # a case yields rows exactly when a region with a pair has a location: every region lies in its ingroup genomes
    assert with_rows == expected
    # (the other golden cases find no region, or -- long_130_60_129 -- no pair)
    assert with_rows == ['c1_30_40_30', 'c1_30_40_30_dot', 'c1_30_0_30_all_ingroup', 'rand6_12_4_12',
                         'rand7_16_1_15', 'rand9_20_10_20', 'rand13_14_2_14', 'rand14_15_2_15',
                         'mixed_wide_20_10_20', 'mixed_wide_in_dna_out_rna_18_6_18', 'long_70_10_70', 'long_100_5_90',
                         'long_40_220_40']


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def test_the_command_line_writes_the_same_files_with_and_without_the_option(tmp_path):
    case = [c for c in FC if c["name"] == "c1_30_40_30"][0]
    flags = []
    for name, v in _design_options(case).items():
        flags += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
    argv = _argv(case, tmp_path) + flags + ["--design-primers"]
    f = {n: str(tmp_path / n) for n in ("plain.align", "prod.align", "p.tsv", "p_again.tsv", "p_m3.tsv")}
    csv_plain = _main(argv + ["-o", f["plain.align"]])
    csv_prod = _main(argv + ["-o", f["prod.align"], "--out_primer_products", f["p.tsv"]])
    _main(argv + ["--out_primer_products", f["p_again.tsv"]])
    _main(argv + ["--out_primer_products", f["p_m3.tsv"], "--primer-mismatches", "3", "--max-product", "400"])
    rd = {n: open(p, "rb").read() for n, p in f.items()}
    assert csv_plain == csv_prod and csv_plain.count("\n") > 1
    assert rd["plain.align"] == rd["prod.align"] and len(rd["plain.align"]) > 0
    assert rd["p.tsv"] == rd["p_again.tsv"]
    lines = rd["p.tsv"].decode().split("\n")
    assert lines[0] == KF.PRODUCT_HEADER and lines[-1] == "" and len(lines) > 2
    # every data row of the CSV has its designed product in every ingroup genome: its product_size, no mismatches
    header = csv_plain.split("\n")[0].split(",")
    sizes = [ln.split(",")[header.index("product_size")] for ln in csv_plain.split("\n")[1:-1]]
    exact = [ln.split("\t") for ln in lines[1:-1] if ln.split("\t")[8:] == ["0", "0", "0", "0"]]
    for region, size in enumerate(sizes):
        assert any(r[0] == str(region) and r[7] == size for r in exact), region
    # more mismatches, shorter products: the exact rows stay
    m3 = set(rd["p_m3.tsv"].decode().split("\n")[1:-1])
    assert {"\t".join(r) for r in exact if int(r[7]) <= 400} <= m3 and len(exact) > 0

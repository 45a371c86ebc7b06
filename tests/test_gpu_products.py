"""--out_products on the GPU (kr_products_*, csrc/k_products.inc): the device's complete site and product lists against the
brute-force definition (products_reference.py) on random texts over three tiles with planted regions and near-copies, for
every distance and for equal and unequal flank lengths; the relation to the locate pass on the golden cases whose flanks
are primers; the command line end to end; two runs, the same bytes."""
import io
import os
import random
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import codec, fasta
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from products_reference import ref_products, ref_sites                    # noqa: E402
from test_locate_host import FC, GOLDEN                                    # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 256 * 64                     # window starts of a tile of the scan (LOC_T * LOC_S)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(b):
    return b[::-1].translate(_COMP)


def _mutate(rng, text, nsub, cols=None):
    t = bytearray(text)
    for c in rng.sample(range(len(t)) if cols is None else cols, nsub):
        t[c] = rng.choice([b for b in b"ACGT" if b != t[c]])
    return bytes(t)


def _case(seed, Le, Re, M):
    """a text over three tiles (a fourth begun), 8 left and 8 right texts, 12 regions that share them, copies planted with
    0 .. M + 1 substitutions per flank on both strands: across every tile edge, next to and across separators, holding N,
    in lower case -> (text, left, right, pairs)"""
    rng = random.Random(seed)
    n = 3 * TILE + 900
    text = bytearray(rng.choice(b"ACGT") for _ in range(n))
    left = [bytes(rng.choice(b"ACGT") for _ in range(Le)) for _ in range(8)]
    right = [bytes(rng.choice(b"ACGT") for _ in range(Re)) for _ in range(8)]
    pairs = [(i, i) for i in range(8)] + [(0, 1), (0, 2), (3, 2), (7, 0)]

    def plant(p, pair, strand, gap, ml, mr, end_l=False, end_r=False):
        a, b = left[pairs[pair][0]], right[pairs[pair][1]]
        a = _mutate(rng, a, ml, range(Le - 5, Le) if end_l else None)
        b = _mutate(rng, b, mr, range(5) if end_r else None)
        amp = a + bytes(rng.choice(b"ACGT") for _ in range(gap)) + b
        if strand:
            amp = _rc(amp)
        text[p:p + len(amp)] = amp
        return len(amp)

    # spread over the text, 5 rounds of the 12 regions: the first round exact, then every number of substitutions on either
    # flank up to one more than allowed; regions 0-2 and 6-8 on '+', the others on '-'
    for i in range(60):
        r = i // 12
        ml, mr = (0, 0) if r == 0 else ((r + i) % (M + 2), (r + i // 3) % (M + 2))
        plant(200 + i * 780, i % 12, (i // 3) & 1, rng.choice([0, 1, 7, 40, 150, 250] if r == 0 else [0, 1, 7, 40, 250, 400]), ml, mr, end_l=i % 5 == 0, end_r=i % 7 == 0)
    # across the tile edges (the offsets differ from case to case): the first site of a product, the second, and a site
    # that ends or begins exactly there
    amp = Le + 3 + Re
    d = 1 + seed % (min(Le, Re) - 1)
    plant(TILE - d, 1, M & 1, 3, 0, 0)
    plant(2 * TILE + d - amp, 2, (M >> 1) & 1, 3, 0, 0)
    plant(3 * TILE - (Le if seed & 1 else 0), 0, 0, 0, 0, 0)             # (and its sites abut)
    # (the free stretches between the spread copies: 700 + 780 j)
    # separators: between the sites of a pair, inside a site, right before and after a product
    p = 4600
    plant(p, 0, 0, 30, 0, 0)
    text[p + Le + 10] = ord("\n")
    p = 8500
    plant(p, 1, 1, 30, 0, 0)
    text[p + 3] = ord("\n")
    p = 12400
    w = plant(p, 2, 0, 12, 0, 0)
    text[p + w] = ord("\n")
    text[p - 1] = ord("\n")
    # N between the sites and inside one
    p = 20200
    plant(p, 3, 0, 20, 0, 0)
    text[p + Le + 5] = ord("N")
    p = 24100
    plant(p, 4, 1, 20, 0, 0)
    text[p + 2] = ord("n")
    # lower case: a whole product, and only what lies between the sites
    p = 28000
    w = plant(p, 5, 0, 25, 0, 0)
    text[p:p + w] = bytes(text[p:p + w]).lower()
    p = 31900
    w = plant(p, 6, 1, 25, 0, 0)
    text[p + Re:p + Re + 25] = bytes(text[p + Re:p + Re + 25]).lower()
    # the last window of the text is a site
    tail = right[7]
    text[n - Re:] = tail
    text[n - Re - 40 - Le:n - Re - 40] = left[7]
    return bytes(text), left, right, pairs


def _u8(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)


GEOMETRIES = [(10, 10), (16, 16), (30, 30), (12, 30), (30, 10)]


@pytest.mark.parametrize("Le,Re", GEOMETRIES)
def test_sites_and_products_equal_the_brute_force_lists(Le, Re):
    """M = 0 .. 3: the device's sites and products equal ref_sites / ref_products list for list; every M and strand has a
    product without a mismatch and (M > 0) one with, every planted kind of mismatch occurs"""
    from krisp_amd import _native
    for M in range(4):
        for omit in (False, True):
            max_product = 300 if omit else 520
            text, left, right, pairs = _case(100 * Le + 10 * Re + M, Le, Re, M)
            lf, rt = _u8(left), _u8(right)
            with _native.Engine() as eng:
                eng.set_params_locate(Le, 4, Re, omit, max_bases=len(text))
                eng.upload(0, np.frombuffer(text, dtype=np.uint8))
                eng.products_table(lf, rt, pairs, M, max_product)
                hits = eng.products(0)
                sites = eng.product_sites()
                again = eng.products(0)
                sites_again = eng.product_sites()
            assert hits.tobytes() == again.tobytes() and sites.tobytes() == sites_again.tobytes()
            assert not sites["pad"].any() and not hits["pad"].any()
            assert sites["pos"].tolist() == sorted(sites["pos"].tolist())
            want_s = ref_sites(text, omit, lf, rt, Le, Re, M)
            got_s = sorted(zip(sites["pos"].tolist(), sites["entry"].tolist(), sites["mismatches"].tolist(),
                               sites["end_mismatches"].tolist()))
            print("Le", Le, "Re", Re, "M", M, "omit", omit, "sites", len(got_s), "want", len(want_s), "products", len(hits))
            assert got_s == [tuple(r) for r in want_s.tolist()]
            want_p = ref_products(text, omit, lf, rt, Le, Re, pairs, M, max_product)
            got_p = list(zip(hits["pos"].tolist(), hits["length"].tolist(), hits["strand"].tolist(), hits["pair"].tolist(),
                             hits["left_mm"].tolist(), hits["right_mm"].tolist(), hits["left_end_mm"].tolist(),
                             hits["right_end_mm"].tolist()))
            assert got_p == [tuple(r) for r in want_p.tolist()]
            _generator_did_its_work(got_s, got_p, Le, Re, M, 100 * Le + 10 * Re + M)


def _generator_did_its_work(sites, prods, Le, Re, M, seed):
    """nothing is compared against an empty list: every strand has a product without a mismatch and (M > 0) with one in
    either flank and at a 3' end, nearly every region has products, sites lie across the tile edges"""
    for strand in (0, 1):
        rows = [r for r in prods if r[2] == strand]
        assert any(r[4] == 0 and r[5] == 0 for r in rows), (M, strand)
        if M:
            assert any(r[4] > 0 for r in rows) and any(r[5] > 0 for r in rows), (M, strand)
            assert any(r[6] > 0 or r[7] > 0 for r in rows), (M, strand)
    assert len({r[3] for r in prods}) >= 10 and len(prods) >= 16
    for edge in (TILE, 2 * TILE):
        assert any(s[0] < edge < s[0] + (Le if s[1] < 16 else Re) for s in sites), edge
    edge = 3 * TILE - (Le if seed & 1 else 0)
    assert any(s[0] == edge and s[1] == 0 for s in sites) and any(r[0] == edge and r[1] == Le + Re for r in prods)


def test_an_engine_without_a_table_or_a_scan_says_so():
    from krisp_amd import _native
    with _native.Engine() as eng:
        eng.set_params_locate(10, 4, 10, False, max_bases=1000)
        eng.upload(0, np.frombuffer(b"ACGT" * 100, dtype=np.uint8))
        with pytest.raises(Exception, match="kr_products_table first"):
            eng.products(0)
        a = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8).reshape(1, 10)
        with pytest.raises(Exception, match="repeats"):
            eng.products_table(a, a, [(0, 0), (0, 0)], 1, 100)
        with pytest.raises(Exception, match="shorter than the two flanks"):
            eng.products_table(a, a, [(0, 0)], 1, 19)
        with pytest.raises(Exception, match="names text"):
            eng.products_table(a, a, [(0, 1)], 1, 100)
        eng.products_table(a, a, [(0, 0)], 0, 100)
        hits = eng.products(0)
        # ACGTACGTAC at 0, 4, 8, ...; its reverse complement GTACGTACGT at 2, 6, ...: s2 - s1 in 10 .. 90
        assert len(hits) > 0 and set(hits["strand"].tolist()) == {0, 1}
        want = ref_products(b"ACGT" * 100, False, a, a, 10, 10, [(0, 0)], 0, 100)
        assert len(hits) == len(want) and hits["pos"].tolist() == want["pos"].tolist()


# ----------------------------------------------------------------------------
# the relation to the locate pass
# ----------------------------------------------------------------------------
def _primer_case(case):
    k = _amplicon(case)
    Le, De, Re = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
    return min(Le, Re) >= KF.PRODUCT_MIN_PRIMER


PRIMER_CASES = [c for c in FC if ("csv" in c or "filtered_canon" in c) and _primer_case(c)]


def _relation(ing, out, L, R, k, omit):
    """-> (regions, exact product rows, product rows): the product rows of length k without a mismatch are a superset of
    the locations, and equal them once the rows whose window the window rules exclude are dropped"""
    groups, _ = KF.find_regions(ing, out, L, R, k, omit_soft=omit)
    locs = KF.locate_regions(groups, ing, out, L, R, k, omit_soft=omit)
    prods = KF.predict_products(groups, ing, out, L, R, k, mismatches=1, max_product=max(1000, k), omit_soft=omit)
    key = ("region", "file", "record_index", "start", "end", "strand")
    want = list(zip(*(locs[f].tolist() for f in key)))
    exact = prods[(prods["length"] == k) & (prods["left_mismatches"] == 0) & (prods["right_mismatches"] == 0)]
    rows = list(zip(*(exact[f].tolist() for f in key)))
    assert set(want) <= set(rows) and len(set(rows)) == len(rows)
    recs = {}
    kept = []
    for r in rows:
        if r[1] not in recs:
            recs[r[1]] = fasta.read_records(r[1])
        w = recs[r[1]][r[2]][r[3]:r[4]]
        assert len(w) == k
        if b"N" in w.upper() or (omit and not w.isupper()):
            continue
        kept.append(r)
    assert kept == want
    assert (prods["end"] - prods["start"] == prods["length"]).all()
    order = list(zip(prods["region"].tolist(), [(ing + out).index(f) for f in prods["file"]], prods["record_index"].tolist(),
                     prods["start"].tolist(), prods["end"].tolist(), (prods["strand"] == "-").tolist()))
    assert order == sorted(order)
    return len(groups), len(rows), len(prods)


def test_exact_products_of_the_design_length_are_the_locations(tmp_path):
    """c1_30_40_30 and every other golden case whose effective flanks are both >= 10 bases"""
    names = [c["name"] for c in PRIMER_CASES]
    assert "c1_30_40_30" in names and "rand6_12_4_12" in names and "long_130_60_129" in names and len(names) >= 15
    with_rows = 0
    for n, case in enumerate(PRIMER_CASES):
        d = tmp_path / str(n)
        d.mkdir()
        ing, out = _files(case, d)
        ngroups, nexact, nprods = _relation(ing, out, case["L"], case["R"], _amplicon(case), case["omit_soft"])
        print(case["name"], "regions", ngroups, "exact rows", nexact, "products", nprods)
        assert nexact > 0 or ngroups == 0, case["name"]
        with_rows += nexact > 0
    assert with_rows >= 12


def test_a_packed_geometry_over_the_c1_files():
    d = os.path.join(GOLDEN, "c1")
    ing = [f"{d}/ingroup{i}.fasta.gz" for i in (0, 1)]
    out = [f"{d}/outgroup{i}.fasta.gz" for i in (0, 1, 2)]
    assert not KF._is_wide(*codec.effective_geometry(12, 4, 12))
    ngroups, nexact, nprods = _relation(ing, out, 12, 12, 28, False)
    print("12/4/12 over c1: regions", ngroups, "exact rows", nexact, "products", nprods)
    assert ngroups > 0 and nexact >= 2 * ngroups and nprods >= nexact


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
    argv = _argv(case, tmp_path)
    f = {n: str(tmp_path / n) for n in ("plain.align", "prod.align", "both.align", "p_alone.tsv", "p_again.tsv", "p_both.tsv",
                                        "l_alone.tsv", "l_both.tsv", "p_m3.tsv")}
    csv_plain = _main(argv + ["-o", f["plain.align"]])
    csv_prod = _main(argv + ["-o", f["prod.align"], "--out_products", f["p_alone.tsv"]])
    csv_both = _main(argv + ["-o", f["both.align"], "--out_products", f["p_both.tsv"], "--out_locations", f["l_both.tsv"]])
    _main(argv + ["--out_locations", f["l_alone.tsv"]])
    _main(argv + ["--out_products", f["p_again.tsv"]])
    _main(argv + ["--out_products", f["p_m3.tsv"], "--primer-mismatches", "3", "--max-product", "400"])
    rd = {n: open(p, "rb").read() for n, p in f.items()}
    assert csv_plain == csv_prod == csv_both == case["csv"]
    assert rd["plain.align"] == rd["prod.align"] == rd["both.align"] and len(rd["plain.align"]) > 0
    assert rd["p_alone.tsv"] == rd["p_both.tsv"] == rd["p_again.tsv"]
    assert rd["l_alone.tsv"] == rd["l_both.tsv"]
    lines = rd["p_alone.tsv"].decode().split("\n")
    assert lines[0] == KF.PRODUCT_HEADER and lines[-1] == "" and len(lines) > 2
    # every location is a row of the products file: length 100, no mismatches
    rows = {tuple(ln.split("\t")[:7]) for ln in lines[1:-1] if ln.split("\t")[7:] == ["100", "0", "0", "0", "0"]}
    locs = {tuple(ln.split("\t")[:7]) for ln in rd["l_alone.tsv"].decode().split("\n")[1:-1]}
    assert locs and locs <= rows
    # more mismatches, shorter products: the exact rows stay
    m3 = set(rd["p_m3.tsv"].decode().split("\n")[1:-1])
    assert {ln for ln in lines[1:-1] if ln.split("\t")[7:] == ["100", "0", "0", "0", "0"]} <= m3

"""--out_panel_products on the GPU (kr_multiplex_*, csrc/k_multiplex.inc): the device's complete site and product
lists against the brute-force definition (multiplex_reference.py) on the texts of multiplex_cases.py, for every case and
soft-mask mode; the tally against the fetched rows; dense output in closed form; the library's refusals and states; the
primer pass, the guide hits and the assay join beside it in one engine; KF.panel_products over FASTA files."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiplex_cases as MC                                               # noqa: E402
from multiplex_reference import rc, ref_products, ref_sites, ref_tally    # noqa: E402

pytestmark = pytest.mark.gpu

KR_ERR_PARAM, KR_ERR_CAPACITY, KR_ERR_STATE = -2, -3, -4                   # include/krisp_hip.h
TILE = MC.TILE
SITE_FIELDS = ("pos", "entry", "mismatches", "end_mismatches")
HIT_FIELDS = ("pos", "length", "fwd", "rev", "fwd_mm", "rev_mm", "fwd_end_mm", "rev_end_mm")


def engine(omit, max_bases):
    from krisp_amd import _native
    eng = _native.Engine()
    eng.set_params_locate(7, 6, 7, omit, max_bases=max(int(max_bases), 1))
    return eng


def tuples(a, fields):
    return list(zip(*(a[f].tolist() for f in fields)))


def check(eng, T, want_s, want_p):
    """the multiplex scan of the genome under id 0 against the definition's lists: the sites sorted by (pos, entry) and the
    products equal them element for element, positions do not descend as the device lists the sites, the pads are zero, a
    second run gives the same bytes; the tally equals the fetched rows counted cell for cell, and the fetch after it the
    fetch before it"""
    from krisp_amd._native import _ptr
    hits, sites = eng.multiplex_products(0), eng.multiplex_sites()
    again, sites_again = eng.multiplex_products(0), eng.multiplex_sites()
    assert hits.tobytes() == again.tobytes() and sites.tobytes() == sites_again.tobytes()
    assert not sites["pad"].any() and not hits["pad"].any()
    assert (np.diff(sites["pos"].astype(np.int64)) >= 0).all()
    got_s, got_p = sorted(tuples(sites, SITE_FIELDS)), tuples(hits, HIT_FIELDS)
    assert len(got_s) == len(want_s) and len(got_p) == len(want_p), (len(got_s), len(want_s), len(got_p), len(want_p))
    assert got_s == list(want_s)
    assert got_p == list(want_p)
    tally = eng.multiplex_tally()
    assert tally.shape == (T, T, 2) and tally.tolist() == ref_tally(got_p, T)
    after = np.empty(max(len(hits), 1), dtype=hits.dtype)
    assert eng.lib.kr_multiplex_fetch(eng.ctx, _ptr(after), len(hits)) == len(hits)
    assert after[:len(hits)].tobytes() == hits.tobytes()
    assert eng.multiplex_tally().tobytes() == tally.tobytes()
    return hits, sites


# ----------------------------------------------------------------------------
# the lists
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,M", MC.CASES)
def test_sites_products_and_tally_equal_the_brute_force_lists(name, T, M):
    text, texts, _ = MC.case(name, T, M)
    for omit in (False, True):
        want_s, want_p = MC.reference(name, T, M, omit)
        with engine(omit, len(text)) as eng:
            eng.upload(0, np.frombuffer(text, dtype=np.uint8))
            eng.multiplex_table(texts, M, MC.MAX_PRODUCT)
            check(eng, T, want_s, want_p)
        print(name, "T", T, "M", M, "omit", omit, "sites", len(want_s), "products", len(want_p))
        assert len(want_s) > 0 and len(want_p) > 0


# ----------------------------------------------------------------------------
# dense output
# ----------------------------------------------------------------------------
DENSE_LENGTHS = (12, 15)            # no window of 12 bytes or more fits between the separators of dense_text's second tile


@pytest.mark.parametrize("name,M", [("A", 0), ("AT", 1), ("ACC", 3)])
def test_dense_output(name, M):
    """test_gpu_scan_properties.dense_text over a periodic unit; the texts are the unit's window of 12 and of 15 letters at
    every phase and their reverse complements, so the table is closed under the reverse complement: every valid window of
    either length is an opening site of one text and a closing site of one text.  max_product = 12 + 15 + 3: every opening
    site closes with every closing site for which the record has room, which counts the products in closed form"""
    from test_gpu_scan_properties import DENSE_UNITS, dense_text
    unit = DENSE_UNITS[name]
    text, _ = dense_text(unit)
    mp = sum(DENSE_LENGTHS) + 3
    texts = []
    for m in DENSE_LENGTHS:
        for ph in range(len(unit)):
            w = (unit * (m + 3))[ph:ph + m]
            for x in (w, rc(w)):
                if x not in texts:
                    texts.append(x)
    T = len(texts)
    want_s = ref_sites(text.tobytes(), False, texts, M)
    want_p = ref_products(text.tobytes(), False, texts, M, mp, sites=want_s)
    gaps = np.diff(np.concatenate([[-1], np.flatnonzero(text == 10), [len(text)]])) - 1        # the records' lengths
    room = lambda n: int(np.maximum(gaps - n + 1, 0).sum())                                    # noqa: E731
    assert len(want_s) == 2 * sum(room(m) for m in DENSE_LENGTHS) and all(s[2] == 0 for s in want_s)
    assert len(want_p) == sum(room(n) for n1 in DENSE_LENGTHS for n2 in DENSE_LENGTHS for n in range(n1 + n2, mp + 1))
    tiles = np.bincount(np.array([s[0] for s in want_s]) // TILE, minlength=4)
    assert tiles[1] == 0 and len(set(tiles.tolist())) == 4     # unequal counts, one tile without a site
    blocks = np.bincount(np.searchsorted([s[0] for s in want_s], [r[0] for r in want_p], side="left") // 256)
    assert len(blocks) > 100 and len(set(blocks.tolist())) > 3  # (the join's blocks of 256 sites: unequal counts as well)
    with engine(False, len(text)) as eng:
        eng.upload(0, text)
        eng.multiplex_table(texts, M, mp)
        check(eng, T, want_s, want_p)
    print(name, "M", M, "T", T, "sites", len(want_s), "products", len(want_p), "sites per tile", tiles.tolist())


# ----------------------------------------------------------------------------
# refusals and states
# ----------------------------------------------------------------------------
def test_the_library_refuses_what_it_does_not_take():
    from krisp_amd._native import _ptr
    a, b = b"ACGTACGTAC", b"GGATCCATTGCA"
    text = b"ACGT" * 100
    many = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(i).integers(0, 4, size=12)]) for i in range(129)]
    with engine(False, 1000) as eng:
        eng.upload(0, np.frombuffer(text, dtype=np.uint8))
        for call in (eng.multiplex_products, eng.multiplex_scan):
            with pytest.raises(Exception, match="kr_multiplex_table first") as e:
                call(0)
            assert e.value.code == KR_ERR_STATE
        for bad in (a[:9], a * 6 + b"A"):
            with pytest.raises(Exception, match="10 .. 60 are taken") as e:
                eng.multiplex_table([a, bad], 1, 200)
            assert e.value.code == KR_ERR_PARAM
        for M in (-1, 4):
            with pytest.raises(Exception, match="mismatches <= 3") as e:
                eng.multiplex_table([a, b], M, 200)
            assert e.value.code == KR_ERR_PARAM
        for texts in ([], many):
            with pytest.raises(Exception, match="1 .. 128 texts") as e:
                eng.multiplex_table(texts, 1, 200)
            assert e.value.code == KR_ERR_PARAM
        with pytest.raises(Exception, match="twice the longest text") as e:
            eng.multiplex_table([a, b], 1, 23)
        assert e.value.code == KR_ERR_PARAM
        with pytest.raises(Exception, match="kr_multiplex_table first"):     # (a refused table is no table)
            eng.multiplex_scan(0)
        assert eng.multiplex_table(many[:128], 1, 200) > 0                    # 128 texts are taken
        assert eng.multiplex_table([a, b], 0, 24) > 0                         # ... and max_product = twice the longest
        for call in (eng.multiplex_tally, eng.multiplex_sites):
            with pytest.raises(Exception, match="kr_multiplex_scan first") as e:
                call()
            assert e.value.code == KR_ERR_STATE
        out = np.empty(4, dtype=np.uint8)
        assert eng.lib.kr_multiplex_fetch(eng.ctx, _ptr(out), 0) == KR_ERR_STATE
        # T = 1: ACGTACGTAC at 0, 4, 8, ...; its reverse complement GTACGTACGT at 2, 6, ...
        eng.multiplex_table([a], 0, 100)
        hits = eng.multiplex_products(0)
        want = ref_products(text, False, [a], 0, 100)
        assert len(want) > 0 and tuples(hits, HIT_FIELDS) == want and set(hits["fwd"].tolist()) == set(hits["rev"].tolist()) == {0}
        assert eng.multiplex_tally().tolist() == [[[0, len(want)]]]
        small = np.zeros(1, dtype=np.uint32)
        assert eng.lib.kr_multiplex_tally(eng.ctx, _ptr(small), 1) == KR_ERR_CAPACITY and small[0] == 0
        # a new table: the list of the earlier one is gone
        eng.multiplex_table([a, b], 0, 100)
        with pytest.raises(Exception, match="kr_multiplex_scan first"):
            eng.multiplex_tally()
        # no products: zeros
        eng.multiplex_table([b"GGGGGGGGGGGG"], 0, 100)
        assert eng.multiplex_scan(0) == 0 and eng.multiplex_tally().tolist() == [[[0, 0]]]
        # another soft-mask mode is another context: the table is dropped
    with engine(False, 1000) as eng:
        eng.multiplex_table([a], 0, 100)
        eng.set_params_locate(7, 6, 7, True, max_bases=1000)
        eng.upload(0, np.frombuffer(text, dtype=np.uint8))
        with pytest.raises(Exception, match="kr_multiplex_table first"):
            eng.multiplex_scan(0)


# ----------------------------------------------------------------------------
# beside the primer pass, the guide hits and the assay join
# ----------------------------------------------------------------------------
def test_the_primer_pass_and_the_assay_join_keep_their_bytes_beside_a_multiplex_scan():
    """test_gpu_scan_coexist's check for this pass: a primer table, a guide table, their scans and the assay join in one
    engine; then a multiplex table and scan; the primer pass's products and sites and the assay hits, fetched WITHOUT a new
    scan or join, are the bytes they were -- and so after new scans.  The multiplex lists equal an engine's that holds
    that table alone"""
    from krisp_amd._native import PRODUCT_HIT, PRODUCT_SITE, _ptr
    rng = np.random.default_rng(24)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=TILE + 3000)].copy()
    text[[4000, 9000]] = 10
    left, right, guides = [], [], []
    for i in range(6):
        p = 500 + 2500 * i
        left.append(text[p:p + 12 + i].tobytes())
        right.append(text[p + 80:p + 94].tobytes())                         # (the template's text under the right primer)
        guides.append(text[p + 30:p + 50])
    pairs = [(i, i) for i in range(6)]
    oligos = left + [rc(t) for t in right]

    def fetch_all(eng, n_products, n_sites):
        prods = np.empty(max(n_products, 1), dtype=PRODUCT_HIT)
        sites = np.empty(max(n_sites, 1), dtype=PRODUCT_SITE)
        assert eng.lib.kr_primers_fetch(eng.ctx, _ptr(prods), n_products) == n_products
        assert eng.lib.kr_primers_sites(eng.ctx, _ptr(sites), n_sites) == n_sites
        return prods[:n_products].tobytes(), sites[:n_sites].tobytes(), eng.assay_hits().tobytes(), eng.guide_hit_windows(20).tobytes()

    with engine(False, len(text)) as alone:
        alone.upload(0, text)
        alone.multiplex_table(oligos, 1, 150)
        want = (alone.multiplex_products(0).tobytes(), alone.multiplex_sites().tobytes(), alone.multiplex_tally().tobytes())
    with engine(False, len(text)) as eng:
        eng.upload(0, text)
        eng.primers_table(left + right, 6, pairs, 1, 150)
        eng.guide_hits_table(np.array(guides, dtype=np.uint8), 1)
        eng.assay_table(pairs)
        prods, sites = eng.primer_products(0), eng.primer_sites()
        assert len(eng.guide_hits(0)) >= 6 and len(prods) >= 6
        assert eng.assay_join(0) >= 6
        before = fetch_all(eng, len(prods), len(sites))
        assert before[0] == prods.tobytes()
        eng.multiplex_table(oligos, 1, 150)
        got = (eng.multiplex_products(0).tobytes(), eng.multiplex_sites().tobytes(), eng.multiplex_tally().tobytes())
        assert got == want and len(got[0]) >= 6 * 24
        assert fetch_all(eng, len(prods), len(sites)) == before             # nothing of theirs was written
        assert eng.primer_products(0).tobytes() == prods.tobytes() and eng.assay_join(0) >= 6
        assert fetch_all(eng, len(prods), len(sites)) == before
        assert (eng.multiplex_products(0).tobytes(), eng.multiplex_sites().tobytes(), eng.multiplex_tally().tobytes()) == want
        # (the pair rows of the multiplex list are the primer pass's products: '+' as (iL, iR), '-' as (iR, iL))
        mux = np.frombuffer(want[0], dtype=eng.multiplex_products(0).dtype)
        plus = {(int(h["pos"]), int(h["length"]), int(h["fwd"])) for h in mux if h["rev"] == h["fwd"] + 6}
        minus = {(int(h["pos"]), int(h["length"]), int(h["rev"])) for h in mux if h["fwd"] == h["rev"] + 6}
        assert plus == {(int(h["pos"]), int(h["length"]), int(h["pair"])) for h in prods if h["strand"] == 0}
        assert minus == {(int(h["pos"]), int(h["length"]), int(h["pair"])) for h in prods if h["strand"] == 1}


# ----------------------------------------------------------------------------
# file level: KF.panel_products
# ----------------------------------------------------------------------------
def py_panel_rows(files, oligos, M, mp, omit=False):
    """the rows of --out_panel_products by an in-test join: every file's records (fasta.read_records) joined by '\\n', the
    definition's products of the distinct texts, every product a row for every oligo of its forward text with every oligo
    of its reverse text, each position mapped to its record; in the file's order"""
    from krisp_amd import fasta
    from test_locate_host import py_record_ids
    texts = sorted({t.encode() for _, t in oligos})
    owners = [[i for i, (_, t) in enumerate(oligos) if t.encode() == x] for x in texts]
    rows = []
    for fi, path in enumerate(files):
        recs = fasta.read_records(path)
        ids = py_record_ids(fasta._read_raw_lines(path))
        assert len(ids) == len(recs)
        first = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])])
        for pos, length, a, b, ma, mb, ea, eb in ref_products(b"\n".join(recs), omit, texts, M, mp):
            ri = int(np.searchsorted(first, pos, side="right")) - 1
            start = pos - int(first[ri])
            for i in owners[a]:
                for j in owners[b]:
                    kind = "single" if i == j else "pair" if i // 2 == j // 2 else "cross"
                    rows.append(((fi, ri, start, start + length, i, j),
                                 (path, ids[ri], ri, start, start + length, length, oligos[i][0], oligos[j][0], kind, ma, mb, ea, eb)))
    rows.sort(key=lambda r: r[0])
    return [r[1] for r in rows]


def test_panel_products_over_files_whose_record_boundaries_lie_in_the_second_and_third_tile(tmp_path):
    from krisp_amd import krisp_fasta as KF
    from krisp_amd import synth
    from test_gpu_scan_properties import write_fasta_that_moves_record_indices
    L, R, k, M, mp = 12, 12, 28, 1, 400
    rng = np.random.default_rng(77)
    paths, seqs = [], []
    for i, (name, _ing, text) in enumerate(synth.family(31, 2, 1, 45_000, records=1, mu=0.01, snp_every=300)):
        seq = text[text != 10].tobytes()
        p = str(tmp_path / f"{name}.fa")
        write_fasta_that_moves_record_indices(p, seq, k, rng, crlf=i % 2 == 1, last=("no_newline", "header", None)[i % 3])
        paths.append(p)
        seqs.append(seq)
    # three members by hand, from the first genome: member 2 lies inside member 1's reach, so 1L .. 2R and 2L .. 1R are
    # cross products; member 3's left oligo has member 1's text (a row for each of them); member 3 lies past the first tile
    s = seqs[0].upper()
    cut = lambda p, n: s[p:p + n].decode()                                                    # noqa: E731
    rcs = lambda t: rc(t.encode()).decode()                                                   # noqa: E731
    p1, p3 = 3000, TILE + 5000
    oligos = [("1L", cut(p1, 20)), ("1R", rcs(cut(p1 + 150, 22))), ("2L", cut(p1 + 60, 18)), ("2R", rcs(cut(p1 + 230, 24))),
              ("3L", cut(p1, 20)), ("3R", rcs(cut(p3, 21)))]
    assert all(set(t) <= set("ACGT") for _, t in oligos)
    want = py_panel_rows(paths, oligos, M, mp)
    rows, summary = KF.panel_products(oligos, paths[:2], paths[2:], L, R, k, mismatches=M, max_product=mp)
    got = list(zip(*(rows[f].tolist() for f in KF.PANEL_PRODUCT_HEADER.split("\t"))))
    print("rows", len(got), "kinds", sorted({r[8] for r in got}), "files", len({r[0] for r in got}))
    assert got == want
    assert {r[8] for r in got} == {"pair", "cross"} and len({r[0] for r in got}) >= 2
    assert any(r[6] == "1L" and r[7] == "2R" for r in got) and any(r[6] == "3L" and r[7] == "1R" for r in got)
    # the summary: the rows counted
    counted = {}
    for r in got:
        c = counted.setdefault((paths.index(r[0]), [n for n, _ in oligos].index(r[6]), [n for n, _ in oligos].index(r[7])), [r, 0, 0])
        c[1] += 1
        c[2] += r[11] == 0 and r[12] == 0
    want_sum = [(c[0][0], c[0][6], c[0][7], c[0][8], c[1], c[2]) for _, c in sorted(counted.items())]
    got_sum = list(zip(*(summary[f].tolist() for f in KF.PANEL_SUMMARY_HEADER.split("\t"))))
    assert got_sum == want_sum and len(got_sum) >= 6
    # rows=False: nothing but the tally comes to the host, the summary is the same
    none, summary2 = KF.panel_products(oligos, paths[:2], paths[2:], L, R, k, mismatches=M, max_product=mp, rows=False)
    assert len(none) == 0 and summary2.tolist() == summary.tolist()

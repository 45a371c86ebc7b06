"""The flank product pass (csrc/k_products.inc) and the primer product pass (csrc/k_primers.inc) against their definitions
(products_reference.py, primers_reference.py), through _native.Engine, the complete site and product lists of every text:
  * random cases from one seeded generator, product_scan_cases.cases(seed): length set x M x alphabet x separator layout x
    table size, texts of up to a little over three tiles (test_product_scan_cases.py's census asserts, on the CPU, what the
    default seeds cover); both tables live in one engine, the passes take turns over three uploads, then a second table;
  * a text planted at every start across a tile edge and at the text's end, as each of A, rc(A), B, rc(B), with exactly M
    substitutions in each column mode, and with a bad byte before / at the start / at the end / after it; a complete
    product whose opening site ends at TILE - 1, TILE, TILE + 1;
  * dense output: periodic texts over A, AT, ACC with test_gpu_scan_properties.dense_text's separators, every valid window
    a site on both strands, four closing sites in reach of every opening site, closed-form counts, tiles and join blocks
    with unequal counts and a tile with none; the primer pass also with 40 texts under one seed;
  * text lengths around the texts' lengths, 16, 64 and the tile, every window a site, every row in closed form;
  * empty and absent tables, no pairs, a text no pair names, a left text that is a right text, a palindrome;
  * multi-record FASTA files whose record boundaries lie in the second and third tile, with empty records, through
    KF.predict_products and KF.primer_products, against py_products.
KR_PRODSCAN_SEEDS sets the number of random cases (default: every length set with every M once)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import product_scan_cases as PS                                            # noqa: E402
import primers_reference as PR                                             # noqa: E402
import products_reference as FR                                            # noqa: E402

pytestmark = pytest.mark.gpu

TILE = PS.TILE
PLAIN = PS.PLAIN
N_SEEDS = int(os.environ.get("KR_PRODSCAN_SEEDS", str(PS.SEEDS)))


def engine(Le, Re, omit, max_bases):
    from krisp_amd import _native
    eng = _native.Engine()
    eng.set_params_locate(Le, 4, Re, omit, max_bases=max(int(max_bases), 1))
    return eng


def _equal(kind, fetch, fetch_sites, want_s, want_p):
    """the lists of the resident genome against the definition's: the sites sorted by (pos, entry) and the products equal
    them element for element, pos does not descend as the device lists the sites, the pad fields are zero, a second
    scan and a second fetch give the same bytes"""
    hits, sites = fetch(), fetch_sites()
    again_sites = fetch_sites()
    again = fetch()
    assert hits.tobytes() == again.tobytes() and sites.tobytes() == again_sites.tobytes() == fetch_sites().tobytes(), kind
    assert not sites["pad"].any() and not hits["pad"].any(), kind
    assert (np.diff(sites["pos"].astype(np.int64)) >= 0).all(), kind
    got_s = sorted(zip(sites["pos"].tolist(), sites["entry"].tolist(), sites["mismatches"].tolist(),
                       sites["end_mismatches"].tolist()))
    got_p = list(zip(*(hits[f].tolist() for f in ("pos", "length", "strand", "pair", "left_mm", "right_mm", "left_end_mm",
                                                   "right_end_mm"))))
    assert len(got_s) == len(want_s), (kind, "sites", len(got_s), len(want_s))
    for i, (g, w) in enumerate(zip(got_s, want_s)):
        assert g == w, (kind, "site", i, g, w)
    assert len(got_p) == len(want_p), (kind, "products", len(got_p), len(want_p))
    for i, (g, w) in enumerate(zip(got_p, want_p)):
        assert g == w, (kind, "product", i, g, w)
    return want_s, want_p


def check_products(eng, text, omit, left, right, Le, Re, pairs, M, max_product, want=None):
    """the flank pass over the genome under id 0 against ref_sites / ref_products -> (sites, products) of the definition"""
    if want is None:
        lf, rt = PS.u8(left, Le), PS.u8(right, Re)
        want = ([tuple(r) for r in FR.ref_sites(text, omit, lf, rt, Le, Re, M).tolist()],
                [tuple(r) for r in FR.ref_products(text, omit, lf, rt, Le, Re, pairs, M, max_product).tolist()])
    return _equal("flank", lambda: eng.products(0), eng.product_sites, *want)


def check_primers(eng, text, omit, left, right, pairs, M, max_product, want=None):
    """the primer pass over the genome under id 0 against ref_sites / ref_products -> (sites, products) of the definition"""
    if want is None:
        sites = PR.ref_sites(text, omit, left + right, len(left), M)
        want = ([tuple(r) for r in sites.tolist()],
                [tuple(r) for r in PR.ref_products(text, omit, left + right, len(left), pairs, M, max_product, sites=sites).tolist()])
    return _equal("primer", lambda: eng.primer_products(0), eng.primer_sites, *want)


def set_tables(eng, f, p, Mf, Mp):
    eng.products_table(PS.u8(f["left"], f["Le"]), PS.u8(f["right"], f["Re"]), f["pairs"], Mf, f["max_product"])
    eng.primers_table(p["left"] + p["right"], len(p["left"]), p["pairs"], Mp, p["max_product"])


def check_case(eng, c, text, M, want=None):
    if c["kind"] == "flank":
        return check_products(eng, text, c["omit"], c["left"], c["right"], c["Le"], c["Re"], c["pairs"], M, c["max_product"], want)
    return check_primers(eng, text, c["omit"], c["left"], c["right"], c["pairs"], M, c["max_product"], want)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_cases_equal_the_definition(seed):
    cs = PS.cases(seed)
    f, p = cs["flank"], cs["primer"]
    assert f["omit"] == p["omit"] and f["M"] == p["M"]
    M = f["M"]
    want = {}
    with engine(f["Le"], f["Re"], f["omit"], max(len(f["text"]), len(p["text"]))) as eng:
        set_tables(eng, f, p, M, M)
        # one genome resident at a time, under one id: the first, another, the first again -- of either pass in turn, so
        # that every scan follows one of the other pass (the per-tile counts and offsets are one set of scratch)
        for name in ("text", "text2", "text"):
            for c in (f, p):
                eng.upload(0, c[name])
                want[c["kind"], name] = check_case(eng, c, c[name], M, want.get((c["kind"], name)))
        # a second table with another M in the same engine
        M2 = (M + 1) % 4
        set_tables(eng, f, p, M2, M2)
        for c in (p, f):
            if c is f:
                eng.upload(0, f["text"])
            want[c["kind"], "M2"] = check_case(eng, c, c["text"], M2)
    print("seed", seed, "M", M, "omit", f["omit"], "flank", (f["Le"], f["Re"]), "n", len(f["text"]), "texts", len(f["right"]),
          "primer set", p["set"], "n", len(p["text"]), "texts", len(p["right"]),
          "(sites, products)", {k: (len(s), len(q)) for k, (s, q) in want.items()})


# ----------------------------------------------------------------------------
# every offset across a tile edge and at the text's end
# ----------------------------------------------------------------------------
EDGE_FLANK = (12, 17)               # L != R, both small; the longer window reaches into the overhang
EDGE_PRIMER = (10, 23)              # the left text has the shortest length, the right text a tail of 13
EDGE_A = b"GATTCCAGCATGTCAACGTTGCA"
EDGE_B = b"CTGAGTACCGGATATCTTGACGG"
BAD_WHERE = ("before", "first", "last", "after")
BAD_BYTE = (("\n", False), ("N", False), ("lower", False), ("lower", True))


def edge_texts(kind, M):
    """(text, pos, entry, omit, reported, where, mode, byte): the text A, rc(A), B or rc(B) written with exactly M
    substitutions at every start from TILE - maxlen - 1 to TILE + 1 and at the last three starts of its length, in a text
    of a tile and a tail; alone, and with a bad byte before it, on its first byte, on its last, after it.  The column
    mode cycles per `where` and the kind of byte ('\\n', N, lower case without and with omit-soft) per (where, entry),
    each with a counter of its own: the test asserts the combinations that come of it"""
    n1, n2 = EDGE_FLANK if kind == "flank" else EDGE_PRIMER
    A, B = EDGE_A[:n1], EDGE_B[:n2]
    head = None if kind == "flank" else min(n1, n2)
    modes = 3 if kind == "flank" else 5
    rng = np.random.default_rng(91 + M + (10 if kind == "flank" else 0))
    n = TILE + 300 + M
    base = PLAIN[rng.integers(0, 4, size=n)]
    out = []
    mode_of, byte_of = {}, {}
    for ei, x in enumerate((A, PS.rc(A), B, PS.rc(B))):
        starts = list(range(TILE - max(n1, n2) - 1, TILE + 2)) + [n - len(x) - 2, n - len(x) - 1, n - len(x)]
        for p in starts:
            for where in (None,) + BAD_WHERE:
                mode = mode_of[where] = (mode_of.get(where, ei) + 1) % modes
                cols = PS.sub_columns(len(x), head or len(x), M, M, mode, rng)
                y = bytearray(x)
                for col in cols:
                    y[col] = rng.choice([b for b in b"ACGT" if b != x[col]])
                text = base.copy()
                text[p:p + len(x)] = np.frombuffer(bytes(y), dtype=np.uint8)
                omit, reported, bi = False, True, None
                if where is not None:
                    bi = byte_of[where, ei] = (byte_of.get((where, ei), ei) + 1) % 4
                    byte, omit = BAD_BYTE[bi]
                    q = p + {"before": -1, "first": 0, "last": len(x) - 1, "after": len(x)}[where]
                    if q >= n:
                        continue
                    text[q] = text[q] | 0x20 if byte == "lower" else ord(byte)
                    reported = where in ("before", "after") or (byte == "lower" and not omit)
                out.append((text, p, ei, omit, reported, where, mode, bi))
    return out


@pytest.mark.parametrize("kind,M", [(k, M) for k in ("flank", "primer") for M in range(4)])
def test_a_site_at_every_start_across_a_tile_edge_and_at_the_end(kind, M):
    n1, n2 = EDGE_FLANK if kind == "flank" else EDGE_PRIMER
    left, right, pairs, mp = [EDGE_A[:n1]], [EDGE_B[:n2]], [(0, 0)], n1 + n2 + 40
    texts = edge_texts(kind, M)
    assert len(texts) >= (max(n1, n2) + 6) * 4 * 5 - 8
    # what the cycling gives: every column mode with every `where` among the plants the definition must report, and every
    # kind of bad byte in every place around every entry at a start whose window lies across the tile edge
    lens = (n1, n1, n2, n2)
    modes = 3 if kind == "flank" else 5
    assert {(w, m) for _, _, _, _, rep, w, m, _ in texts if rep} == {(w, m) for w in (None,) + BAD_WHERE for m in range(modes)}
    assert ({(w, b, e) for _, p, e, _, _, w, _, b in texts if w is not None and p < TILE < p + lens[e]}
            == {(w, b, e) for w in BAD_WHERE for b in range(4) for e in range(4)})
    engines = {omit: engine(n1, n2, omit, TILE + 400) for omit in (False, True)}

    def check(eng, text, omit):
        if kind == "flank":
            return check_products(eng, text, omit, left, right, n1, n2, pairs, M, mp)
        return check_primers(eng, text, omit, left, right, pairs, M, mp)

    seen = 0
    try:
        for eng in engines.values():
            if kind == "flank":
                eng.products_table(PS.u8(left, n1), PS.u8(right, n2), pairs, M, mp)
            else:
                eng.primers_table(left + right, 1, pairs, M, mp)
        for text, p, entry, omit, reported, _where, _mode, _byte in texts:
            eng = engines[omit]
            eng.upload(0, text)
            sites, _ = check(eng, text, omit)
            there = any(s[0] == p and s[1] == entry and s[2] == M for s in sites)
            assert there == reported, (p, entry, omit)          # (the definition agrees with how the text was made)
            seen += reported
        # a complete product whose opening site ends at TILE - 1, TILE, TILE + 1, on either strand
        rng = np.random.default_rng(5)
        for end in (TILE - 1, TILE, TILE + 1):
            for strand, amp in enumerate((left[0] + b"ACG" + right[0], PS.rc(left[0] + b"ACG" + right[0]))):
                text = PLAIN[rng.integers(0, 4, size=TILE + 300)]
                p = end - (n2 if strand else n1)
                text[p:p + len(amp)] = np.frombuffer(amp, dtype=np.uint8)
                engines[False].upload(0, text)
                _, prods = check(engines[False], text, False)
                assert (p, n1 + 3 + n2, strand, 0, 0, 0, 0, 0) in prods
    finally:
        for eng in engines.values():
            eng.close()
    assert seen >= (max(n1, n2) + 6) * 4 * 3


# ----------------------------------------------------------------------------
# lengths
# ----------------------------------------------------------------------------
LEN_SMIN, LEN_MAX = 10, 13
LENGTHS = [0, 1, LEN_SMIN - 1, LEN_SMIN, LEN_SMIN + 1, LEN_MAX - 1, LEN_MAX, 15, 16, 17, 63, 64, 65, TILE + LEN_SMIN - 2,
           TILE + LEN_SMIN - 1, TILE + LEN_SMIN, TILE + LEN_MAX - 1, 2 * TILE + LEN_SMIN - 1]


@pytest.mark.parametrize("trailing", [False, True], ids=["plain", "trailing_separator"])
@pytest.mark.parametrize("n", LENGTHS)
def test_text_lengths(n, trailing):
    """an all-A text and all-A texts of 10 (left) and 13 (right) letters: every window of either length is a site of the
    text as written (the reverse complements, all T, do not occur); max_product = 10 + 13 + 1: an opening site has a
    closing site right after it and one a byte on"""
    text = np.full(n, ord("A"), dtype=np.uint8)
    nsep = 1 if trailing and n else 0
    if nsep:
        text[n - 1] = 10
    m = n - nsep
    left, right, pairs = [b"A" * LEN_SMIN], [b"A" * LEN_MAX], [(0, 0)]
    mp = LEN_SMIN + LEN_MAX + 1
    sites = max(0, m - LEN_SMIN + 1) + max(0, m - LEN_MAX + 1)
    prods = max(0, m - mp + 2) + max(0, m - mp + 1)             # (of length mp - 1 and mp, on '+')
    lf, rt = PS.u8(left, LEN_SMIN), PS.u8(right, LEN_MAX)
    small = n < 1000
    with engine(LEN_SMIN, LEN_MAX, False, n) as eng:
        eng.upload(0, text)
        want_p = None
        for M in range(4):
            eng.products_table(lf, rt, pairs, M, mp)
            eng.primers_table(left + right, 1, pairs, M, mp)
            ps = PR.ref_sites(text, False, left + right, 1, M)
            want_s = [tuple(r) for r in ps.tolist()]
            assert want_s == [tuple(r) for r in FR.ref_sites(text, False, lf, rt, LEN_SMIN, LEN_MAX, M).tolist()]
            # the definition's products are a function of its sites, the separators, the pairs and max_product: over the long
            # texts they are computed once (M = 0) and stand for every M whose sites are the same list, and -- the flank
            # reference visits every two sites of a pair -- the flank pass is held to the rows in closed form there
            if small or want_p is None:
                want_p = [tuple(r) for r in PR.ref_products(text, False, left + right, 1, pairs, M, mp, sites=ps).tolist()]
                sites0 = want_s
            assert want_s == sites0
            # (every row in closed form: an opening site at p with the closing site right after it, and a byte on)
            rows = sorted([(p, mp - 1, 0, 0, 0, 0, 0, 0) for p in range(max(0, m - mp + 2))] +
                          [(p, mp, 0, 0, 0, 0, 0, 0) for p in range(max(0, m - mp + 1))])
            assert want_p == rows
            flank_p = [tuple(r) for r in FR.ref_products(text, False, lf, rt, LEN_SMIN, LEN_MAX, pairs, M, mp).tolist()] if small else rows
            assert (len(want_s), len(want_p), len(flank_p)) == (sites, prods, prods), (M, len(want_s), len(want_p), sites, prods)
            check_products(eng, text, False, left, right, LEN_SMIN, LEN_MAX, pairs, M, mp, want=(want_s, flank_p))
            check_primers(eng, text, False, left, right, pairs, M, mp, want=(want_s, want_p))


# ----------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------
def plain_text(n, seed):
    return PLAIN[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def test_empty_and_absent_tables_give_no_sites_and_no_products():
    n1, n2 = 12, 15
    text = plain_text(2 * TILE + 100, 3)
    with engine(n1, n2, False, len(text)) as eng:
        eng.upload(0, text)
        for left, right, pairs in (([], [], []), ([b"R" * n1], [b"S" * n2], [(0, 0)])):
            for M in range(4):
                eng.products_table(np.frombuffer(b"".join(left), dtype=np.uint8).reshape(len(left), n1),
                                   np.frombuffer(b"".join(right), dtype=np.uint8).reshape(len(right), n2), pairs, M, 100)
                eng.primers_table(left + right, len(left), pairs, M, 100)
                for s, p in (check_products(eng, text, False, left, right, n1, n2, pairs, M, 100),
                             check_primers(eng, text, False, left, right, pairs, M, 100)):
                    assert s == [] and p == []
                assert eng.products(0).shape == eng.primer_products(0).shape == (0,)
                assert eng.product_sites().shape == eng.primer_sites().shape == (0,)


@pytest.mark.parametrize("M", range(4))
def test_pairs_that_are_absent_unnamed_texts_equal_texts_and_a_palindrome(M):
    n1 = n2 = 12
    text = plain_text(TILE + 2000, 4 + M)
    half = b"GATTCC"
    pal = half + PS.rc(half)
    a, b, c = text[300:312].tobytes(), text[TILE - 5:TILE + 7].tobytes(), text[900:912].tobytes()
    # a ... b, a ... a, pal ... pal, rc(b) ... rc(a) and c alone
    for at, x in ((330, b), (500, a), (520, a), (700, pal), (730, pal), (1200, PS.rc(b)), (1230, PS.rc(a))):
        text[at:at + 12] = np.frombuffer(x, dtype=np.uint8)
    left, right = [a, pal, c], [b, a, pal]
    with engine(n1, n2, False, len(text)) as eng:
        eng.upload(0, text)
        for pairs in ([], [(0, 0), (0, 1), (1, 2)]):
            eng.products_table(PS.u8(left, n1), PS.u8(right, n2), pairs, M, 80)
            eng.primers_table(left + right, 3, pairs, M, 80)
            fs, fp = check_products(eng, text, False, left, right, n1, n2, pairs, M, 80)
            ps, pp = check_primers(eng, text, False, left, right, pairs, M, 80)
            assert (fs, fp) == (ps, pp)
            assert any(s[:2] == (900, 4) for s in fs)           # the text no pair names is a site all the same
            assert {(300, 0), (300, 8), (700, 2), (700, 3), (700, 10), (700, 11)} <= {s[:2] for s in fs}
            if not pairs:
                assert fp == [] and len(fs) >= 12
            else:
                rows = {r[:4] for r in fp}
                assert {(300, 42, 0, 0), (500, 32, 0, 1), (700, 42, 0, 2), (700, 42, 1, 2), (1200, 42, 1, 0)} <= rows


# ----------------------------------------------------------------------------
# dense output
# ----------------------------------------------------------------------------
DENSE_LENGTHS = (12, 15)            # no window of 12 bytes or more fits between the separators of dense_text's second tile
DENSE_CASES = [("A", 0, 0), ("AT", 1, 0), ("ACC", 3, 0), ("AT", 2, 40)]       # (unit, M, texts more under one seed)
_DENSE = {}


def dense_case(name, M, more):
    """test_gpu_scan_properties.dense_text over the unit, and tables made from the unit so that every valid window of
    either length is a site on both strands: the window at each phase and its reverse complement, as left texts (12
    letters) and as right texts (15); max_product = 12 + 15 + 3: an opening site has four places for a closing site.
    A and AT: every (left, right) is a pair, and every opening site with room for one has a product on either strand
    at each of the four places; ACC: a third of the 36 pairs (the reference visits every closing site in reach of
    every opening site of every pair: two thirds fewer visits).  more: as many left texts of 18 letters that no pair
    names, each the unit's window of 12 and a tail of its own -- the primer pass lists them all under one seed.
    -> (text, left, right, pairs, the definition's sites and products through primers_reference, computed once)"""
    if (name, M, more) in _DENSE:
        return _DENSE[name, M, more]
    from test_gpu_scan_properties import DENSE_UNITS, dense_text
    unit = DENSE_UNITS[name]
    n1, n2 = DENSE_LENGTHS
    text, _ = dense_text(unit)
    left, right = [], []
    for rows, m in ((left, n1), (right, n2)):
        for ph in range(len(unit)):
            w = (unit * (m + 3))[ph:ph + m]
            for x in (w, PS.rc(w)):
                if x not in rows:
                    rows.append(x)
    pairs = [(i, j) for i in range(len(left)) for j in range(len(right)) if name != "ACC" or (i + j) % 3 == 0]
    rng = np.random.default_rng(more)
    texts = left + [left[0] + PLAIN[rng.integers(0, 4, size=6)].tobytes() for _ in range(more)]
    sites = PR.ref_sites(text, False, texts + right, len(texts), M)
    prods = PR.ref_products(text, False, texts + right, len(texts), pairs, M, n1 + n2 + 3, sites=sites)
    _DENSE[name, M, more] = (text, texts, right, pairs, [tuple(r) for r in sites.tolist()], [tuple(r) for r in prods.tolist()])
    return _DENSE[name, M, more]


@pytest.mark.parametrize("name,M,more", DENSE_CASES)
def test_dense_output(name, M, more):
    n1, n2 = DENSE_LENGTHS
    mp = n1 + n2 + 3
    text, left, right, pairs, want_s, want_p = dense_case(name, M, more)
    gaps = np.diff(np.concatenate([[-1], np.flatnonzero(text == 10), [len(text)]])) - 1        # the records' lengths
    valid = {m: int(np.maximum(gaps - m + 1, 0).sum()) for m in (n1, n2)}
    # a valid window is the unit at one phase: the site of that text as written and of the reverse complement of another
    # (AT, 12 letters: of the same text, which is its own reverse complement)
    nl2 = 2 * len(left)
    named = [s for s in want_s if s[1] < 2 * (len(left) - more) or s[1] >= nl2]
    assert len(named) == 2 * (valid[n1] + valid[n2]) and valid[n1] > 2 * TILE - 3000
    assert all(s[2] == 0 for s in named)
    if name != "ACC":
        # either strand: a product wherever the record has room for the two sites and 0 .. 3 bytes between them
        assert len(want_p) == 2 * sum(int(np.maximum(gaps - (n1 + n2 + d) + 1, 0).sum()) for d in range(4))
    assert len(want_p) > 4 * TILE and {r[2] for r in want_p} == {0, 1} and max(r[1] for r in want_p) == mp
    tiles = np.bincount(np.array([s[0] for s in want_s]) // TILE, minlength=4)
    assert tiles[1] == 0 and len(set(tiles.tolist())) == 4     # unequal counts, one tile without a site
    blocks = np.bincount(np.searchsorted([s[0] for s in want_s], [r[0] for r in want_p], side="left") // 256)
    assert len(blocks) > 100 and len(set(blocks.tolist())) > 3  # (the join's blocks of 256 sites: unequal counts as well)
    with engine(n1, n2, False, len(text)) as eng:
        eng.upload(0, text)
        eng.primers_table(left + right, len(left), pairs, M, mp)
        check_primers(eng, text, False, left, right, pairs, M, mp, want=(want_s, want_p))
        if not more:
            # the flank pass: its own reference's sites; its products are the primer reference's, which the sites'
            # equality makes the definition's (products_reference.ref_products visits every two sites of a pair: 10^9)
            lf, rt = PS.u8(left, n1), PS.u8(right, n2)
            assert want_s == [tuple(r) for r in FR.ref_sites(text, False, lf, rt, n1, n2, M).tolist()]
            eng.products_table(lf, rt, pairs, M, mp)
            check_products(eng, text, False, left, right, n1, n2, pairs, M, mp, want=(want_s, want_p))
    print(name, "M", M, "sites", len(want_s), "products", len(want_p), "sites per tile", tiles.tolist())


# ----------------------------------------------------------------------------
# file level: positions to (record, record_index, start, end)
# ----------------------------------------------------------------------------
def py_products(files, ref, omit):
    """rows (region, file, record, record_index, start, end, strand, length, left / right mismatches, left / right end
    mismatches) in the TSV's order: every file's records (fasta.read_records) joined by '\\n', ref(text) = the
    definition's products with `pair` = the region, each position mapped to its record"""
    from krisp_amd import fasta
    from test_locate_host import py_record_ids
    rows = []
    for fi, path in enumerate(files):
        recs = fasta.read_records(path)
        assert not fasta.detect_rna(recs)
        ids = py_record_ids(fasta._read_raw_lines(path))
        assert len(ids) == len(recs)
        first = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])])       # where a record starts in the text
        for pos, length, strand, region, lm, rm, le, re_ in ref(np.frombuffer(b"\n".join(recs), dtype=np.uint8)):
            ri = int(np.searchsorted(first, pos, side="right")) - 1
            start = pos - int(first[ri])
            assert start + length <= len(recs[ri])
            rows.append((region, fi, ri, start, start + length, strand,
                         (region, path, ids[ri], ri, start, start + length, "+-"[strand], length, lm, rm, le, re_), pos))
    rows.sort(key=lambda r: r[:6])
    return [r[6] for r in rows], [r[7] for r in rows]


def product_rows(p):
    return list(zip(*(p[f].tolist() for f in ("region", "file", "record", "record_index", "start", "end", "strand", "length",
                                              "left_mismatches", "right_mismatches", "left_end_mismatches",
                                              "right_end_mismatches"))))


@pytest.mark.parametrize("seed", range(2))
def test_files_whose_record_boundaries_lie_in_the_second_and_third_tile(seed, tmp_path):
    from krisp_amd import codec, synth
    from krisp_amd import krisp_fasta as KF
    from test_gpu_scan_properties import write_fasta_that_moves_record_indices
    L, R, k, M, mp = 12, 12, 28, 1, 400
    rng = np.random.default_rng(50 + seed)
    paths = []
    for i, (name, _ing, text) in enumerate(synth.family(20 + seed, 2, 2, 45_000, records=1, mu=0.01, snp_every=300)):
        seq = text[text != 10].tobytes()
        assert len(seq) > 40_000
        p = str(tmp_path / f"{name}.fa")
        write_fasta_that_moves_record_indices(p, seq, k, rng, crlf=(i + seed) % 2 == 1, last=("no_newline", "header", None)[i % 3])
        paths.append(p)
    ing, out = paths[:2], paths[2:]
    groups, _ = KF.find_regions(ing, out, L, R, k)
    assert len(groups) >= 24
    groups = list(groups)[::8]                                  # (a smaller table: the reference compares every text everywhere)
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    left = [g[0].left.replace("U", "T").encode() for g in groups]
    right = [g[0].right.replace("U", "T").encode() for g in groups]
    assert {len(t) for t in left} == {Le} and {len(t) for t in right} == {Re}
    pairs = [(i, i) for i in range(len(groups))]                # region i is pair i: equal flanks stay texts of their own
    want, where = py_products(paths, lambda t: [tuple(r) for r in FR.ref_products(
        t, False, PS.u8(left, Le), PS.u8(right, Re), Le, Re, pairs, M, mp).tolist()], False)
    got = product_rows(KF.predict_products(groups, ing, out, L, R, k, mismatches=M, max_product=mp))
    print("seed", seed, "regions", len(groups), "flank rows", len(got), "records", sorted({r[3] for r in got}))
    assert got == want
    assert len({r[3] for r in got}) >= 6 and max(where) > TILE  # (rows in many records: those past the first tile too)
    # the designed primers: test_gpu_primers' recipe (primers of the last sizes that fit the flanks, loose filters)
    ingroup = [KF.simplename(f) for f in ing]
    h = min(Le, Re, 20)
    records = KF.design_primers(groups, ingroup, tm=(30, 75), gc=(20, 80), amp_size=(Le + De + Re - 4, Le + De + Re),
                                primer_size=(h - 1, h), max_sec_tm=35, gc_clamp=0, max_end_gc=5)
    rows, _, _, _ = KF.design_templates(groups, ingroup)
    found = [(bytes(row[int(r["left_start"]):int(r["left_start"]) + int(r["left_len"])]),
              bytes(row[int(r["right_start"]):int(r["right_start"]) + int(r["right_len"])]))
             for row, r in zip(rows, records) if int(r["found"])]
    assert len(found) >= 3
    texts = [a for a, _ in found] + [b for _, b in found]       # a region with a pair is pair `rank` of texts of its own
    ppairs = [(i, i) for i in range(len(found))]
    want, where = py_products(paths, lambda t: [tuple(r) for r in PR.ref_products(t, False, texts, len(found), ppairs, M, mp).tolist()],
                              False)
    got = product_rows(KF.primer_products(groups, records, ingroup, ing, out, L, R, k, mismatches=M, max_product=mp))
    print("seed", seed, "pairs", len(found), "primer rows", len(got), "records", sorted({r[3] for r in got}))
    assert got == want
    assert len({r[3] for r in got}) >= 6 and max(where) > TILE

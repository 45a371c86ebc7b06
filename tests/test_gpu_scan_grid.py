"""The six passes of the scan scaffold (csrc/k_scan.inc, csrc/h_scan.inc) with several tiles per workgroup.  A text of three
tiles and a begun fourth is launched with as many workgroups as it has tiles, so no workgroup of the other modules' runs
takes a second trip through its tile loop.  KR_SCAN_GRID (read when the context is made) caps the scans' grids: with 1 one
workgroup walks every tile in order, with 2 a workgroup takes tiles two apart, with 3 the workgroups of a four-tile text make
unequal numbers of trips; the element-stride launches (the windows' text, the sites' records) take the same cap and stride.

For every pass -- locate, near match, products, primer products, guide hits, bulged guide hits -- and every cap, over the
cases the pass's own module holds it to (their generators, references and check helpers, imported: nothing is defined a
second time here): the complete lists equal the brute-force definition's field by field, as that module asserts it; their
bytes, the windows' and kr_locate_seps' equal the bytes of the same run without the variable; and debug_scan() shows the cap
in force, grid == min(cap, tiles) and -- on every text of more tiles than the cap -- tiles > grid: a run whose workgroups
never looped fails."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_bulge_cases as BC                                             # noqa: E402
import guide_hit_cases as GC                                               # noqa: E402
import primer_cases as PC                                                  # noqa: E402
import product_scan_cases as PS                                            # noqa: E402
import test_gpu_guide_bulges as GB                                         # noqa: E402
import test_gpu_guide_hits as GH                                           # noqa: E402
import test_gpu_product_scan_properties as PP                              # noqa: E402
import test_gpu_scan_properties as SP                                      # noqa: E402

pytestmark = pytest.mark.gpu

ENV = "KR_SCAN_GRID"
TILE = SP.TILE
CAPS = (1, 2, 3)
RUNS = (None,) + CAPS               # the run without the variable goes first: the others' bytes are held to its


def set_cap(monkeypatch, cap):
    """the variable for the engines made from here on (None: unset)"""
    if cap is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(cap))


def digest(*arrays):
    """the bytes of the arrays, and their lengths"""
    h = hashlib.blake2b()
    for a in arrays:
        b = np.ascontiguousarray(a).tobytes()
        h.update(len(b).to_bytes(8, "little"))
        h.update(b)
    return h.digest()


def geometry(eng, cap, n, width):
    """debug_scan() right after a scan of a text of n bytes whose windows have `width` bytes, against a table that is not
    empty: the cap in force, the text's tiles, grid == min(cap, tiles) -> 1 where a workgroup took more than one tile"""
    d = eng.debug_scan()
    tiles = (max(0, n - width + 1) + TILE - 1) // TILE
    assert d["cap"] == (cap or 0), (d, cap)
    if not tiles:
        return 0
    assert d["tiles"] == tiles and d["blocks"] >= 1, (d, tiles)
    if cap:
        assert d["grid"] == min(cap, tiles), (d, cap)
    else:
        assert 1 <= d["grid"] <= tiles, d
    return int(d["tiles"] > d["grid"])


def hold_to_the_first_run(runs, looped, tiles_at_least):
    """runs: cap -> the run's digests, in RUNS' order; looped: cap -> scans whose workgroups took several tiles.  The bytes
    of every capped run are the uncapped run's; a case with a text of `tiles_at_least` tiles looped under every cap below"""
    for cap in CAPS:
        assert runs[cap] == runs[None], cap
        if tiles_at_least > cap:
            assert looped[cap] > 0, (cap, looped)


# ----------------------------------------------------------------------------
# locate and near match
# ----------------------------------------------------------------------------
def locate_and_near(eng, cap, text, L, D, R, omit, flanks, targets, M, want, out):
    """both passes and the separators over the genome under id 0, as test_gpu_scan_properties checks them; want: the
    definition's (locate, near) hits or (None, None); out: the run's digests -> (want, scans that looped)"""
    k = L + D + R
    wl, wn = want
    looped = 0
    if flanks is not None:
        wl = SP.check_locate(eng, text, L, D, R, omit, flanks, wl)
        looped += geometry(eng, cap, len(text), k)
        out.append(digest(eng.locate(0), eng.locate_windows(k)))
    if targets is not None:
        wn = SP.check_near(eng, text, L, D, R, omit, targets, M, wn)
        looped += geometry(eng, cap, len(text), k)
        out.append(digest(eng.near(0), eng.near_windows(k)))
    SP.check_seps(eng, text)
    out.append(digest(eng.locate_seps(0)))
    return (wl, wn), looped


@pytest.mark.parametrize("seed", range(SP.SEEDS))
def test_locate_and_near_random_cases(seed, monkeypatch):
    c = SP.cases(seed)
    L, D, R, omit, M = c["L"], c["D"], c["R"], c["omit"], c["M"]
    want, runs, looped = {}, {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        with SP.engine(L, D, R, omit, max(len(c["text"]), len(c["text2"]))) as eng:
            eng.locate_table(c["flanks"])
            eng.near_table(c["targets"], M)
            for name in ("text", "text2"):
                eng.upload(0, c[name])
                want[name], n = locate_and_near(eng, cap, c[name], L, D, R, omit, c["flanks"], c["targets"], M,
                                                want.get(name, (None, None)), runs[cap])
                looped[cap] += n
    hold_to_the_first_run(runs, looped, (max(0, len(c["text"]) - c["k"] + 1) + TILE - 1) // TILE)
    print("seed", seed, "n", len(c["text"]), "looped", looped, "hits", [(len(a), len(b)) for a, b in want.values()])


_EDGE_TEXTS = {}                    # (kind, M) -> (the texts, the definition's lists of each: filled by the first run)
_EDGE_BASE = {}                     # (kind, M) -> the run without the variable: (digests, scans that looped)


def edge_run(monkeypatch, kind, M, cap):
    """test_a_window_at_every_start_across_a_tile_edge_and_at_the_end's texts under one cap -> (digests, scans that looped);
    the definition's hits are computed in the first run and shared"""
    L, D, R = SP.EDGE_GEOMETRY
    k = L + D + R
    if (kind, M) not in _EDGE_TEXTS:
        _EDGE_TEXTS[kind, M] = (SP.edge_texts(kind, M), {})
    texts, wants = _EDGE_TEXTS[kind, M]
    flanks = np.concatenate([SP.EDGE_TARGET[:L], SP.EDGE_TARGET[L + D:]]).reshape(1, L + R)
    target = SP.EDGE_TARGET.reshape(1, k)
    set_cap(monkeypatch, cap)
    engines = {omit: SP.engine(L, D, R, omit, len(texts[0][0])) for omit in (False, True)}
    out, looped = [], 0
    try:
        for eng in engines.values():
            eng.locate_table(flanks)
            eng.near_table(target, M)
        for i, (text, p, strand, omit, reported) in enumerate(texts):
            eng = engines[omit]
            eng.upload(0, text)
            wants[i], n = locate_and_near(eng, cap, text, L, D, R, omit, flanks if kind == "locate" else None,
                                          target if kind == "near" else None, M, wants.get(i, (None, None)), out)
            looped += n
            w = wants[i][0] if kind == "locate" else wants[i][1]
            there = (w["pos"] == p) & (w["strand"] == strand)
            if kind == "near":
                there &= w["mismatches"] == M
            assert bool(there.any()) == reported, (p, strand, omit)
    finally:
        for eng in engines.values():
            eng.close()
    return out, looped


@pytest.mark.parametrize("cap", RUNS)
@pytest.mark.parametrize("kind,M", [("locate", 0), ("near", 0), ("near", 1), ("near", 2), ("near", 3)])
def test_locate_and_near_windows_at_every_start_across_a_tile_edge(kind, M, cap, monkeypatch):
    """(the run without the variable is a case of its own, first in order, kept for the others; a capped run alone makes it)"""
    if (kind, M) not in _EDGE_BASE:
        _EDGE_BASE[kind, M] = edge_run(monkeypatch, kind, M, None)
    base, never = _EDGE_BASE[kind, M]
    assert never == 0
    if cap is None:
        return
    out, looped = edge_run(monkeypatch, kind, M, cap)
    assert out == base
    # (two tiles and a tail are three tiles; a text leaves two digests: its list with the windows, its separators)
    assert len(base) >= (sum(SP.EDGE_GEOMETRY) + 6) * 2 * 18 * 2
    assert looped == (len(base) // 2 if cap < 3 else 0), (looped, len(base))


@pytest.mark.parametrize("F,M", [(1, 0), (1, 2), (2, 1), (2, 3), (40, 1)])
@pytest.mark.parametrize("name", list(SP.DENSE_UNITS))
def test_locate_and_near_dense_output(name, F, M, monkeypatch):
    """every window a hit on both strands, the second tile without one: a workgroup meets an empty tile, then a full one"""
    L, D, R = SP.DENSE_GEOMETRY
    unit = SP.DENSE_UNITS[name]
    text, nvalid = SP.dense_text(unit)
    flanks, targets, dist = SP.dense_tables(unit, F)
    within = sum(d <= M for d in dist)
    want, runs, looped = (None, None), {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap] = []
        with SP.engine(L, D, R, False, len(text)) as eng:
            eng.upload(0, text)
            eng.locate_table(flanks)
            eng.near_table(targets, M)
            want, looped[cap] = locate_and_near(eng, cap, text, L, D, R, False, flanks, targets, M, want, runs[cap])
    assert len(want[0]) == 2 * nvalid and len(want[1]) == 2 * nvalid * within
    tiles = np.bincount(want[1]["pos"] // TILE, minlength=4)
    assert tiles[1] == 0 and tiles[0] and tiles[2] and tiles[3]
    hold_to_the_first_run(runs, looped, 4)


# ----------------------------------------------------------------------------
# products and primer products
# ----------------------------------------------------------------------------
def products_of(eng, cap, c, text, M, want, out):
    """a case's pass (product_scan_cases: kind "flank" or "primer") and the separators over the genome under id 0
    -> (the definition's lists, scans that looped)"""
    want = PP.check_case(eng, c, text, M, want)
    width = min(c["Le"], c["Re"]) if c["kind"] == "flank" else min(len(t) for t in c["left"] + c["right"])
    looped = geometry(eng, cap, len(text), width) if c["left"] or c["right"] else 0
    if c["kind"] == "flank":
        out.append(digest(eng.products(0), eng.product_sites()))
    else:
        out.append(digest(eng.primer_products(0), eng.primer_sites()))
    seps = eng.locate_seps(0)
    assert np.array_equal(seps, np.flatnonzero(np.frombuffer(bytes(text), dtype=np.uint8) == 10))
    out.append(digest(seps))
    return want, looped


@pytest.mark.parametrize("seed", range(PS.SEEDS))
def test_products_random_cases(seed, monkeypatch):
    cs = PS.cases(seed)
    f, p = cs["flank"], cs["primer"]
    M = f["M"]
    want, runs, looped = {}, {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        with PP.engine(f["Le"], f["Re"], f["omit"], max(len(f["text"]), len(p["text"]))) as eng:
            PP.set_tables(eng, f, p, M, M)
            for name in ("text", "text2"):
                for c in (f, p):
                    eng.upload(0, c[name])
                    want[c["kind"], name], n = products_of(eng, cap, c, c[name], M, want.get((c["kind"], name)), runs[cap])
                    looped[cap] += n
    hold_to_the_first_run(runs, looped, (max(0, min(len(f["text"]), len(p["text"])) - 60 + 1) + TILE - 1) // TILE)
    print("seed", seed, "n", len(f["text"]), len(p["text"]), "looped", looped,
          "(sites, products)", {k: (len(s), len(q)) for k, (s, q) in want.items()})


def product_edge_run(monkeypatch, kind, M, cap):
    """test_a_site_at_every_start_across_a_tile_edge_and_at_the_end's texts, and its complete products whose opening site
    ends at the tile edge, under one cap -> (digests, scans that looped)"""
    n1, n2 = PP.EDGE_FLANK if kind == "flank" else PP.EDGE_PRIMER
    left, right, pairs, mp = [PP.EDGE_A[:n1]], [PP.EDGE_B[:n2]], [(0, 0)], n1 + n2 + 40
    c = dict(kind=kind, left=left, right=right, Le=n1, Re=n2, pairs=pairs, max_product=mp)
    if (kind, M) not in _EDGE_TEXTS:
        texts = [(t, p, e, omit, rep) for t, p, e, omit, rep, _w, _m, _b in PP.edge_texts(kind, M)]
        rng = np.random.default_rng(5)
        for end in (TILE - 1, TILE, TILE + 1):
            for strand, amp in enumerate((left[0] + b"ACG" + right[0], PS.rc(left[0] + b"ACG" + right[0]))):
                text = PP.PLAIN[rng.integers(0, 4, size=TILE + 300)]
                p = end - (n2 if strand else n1)
                text[p:p + len(amp)] = np.frombuffer(amp, dtype=np.uint8)
                texts.append((text, (p, n1 + 3 + n2, strand, 0, 0, 0, 0, 0), None, False, None))
        _EDGE_TEXTS[kind, M] = (texts, {})
    texts, wants = _EDGE_TEXTS[kind, M]
    set_cap(monkeypatch, cap)
    engines = {omit: PP.engine(n1, n2, omit, TILE + 400) for omit in (False, True)}
    out, looped = [], 0
    try:
        for eng in engines.values():
            if kind == "flank":
                eng.products_table(PS.u8(left, n1), PS.u8(right, n2), pairs, M, mp)
            else:
                eng.primers_table(left + right, 1, pairs, M, mp)
        for i, (text, p, entry, omit, reported) in enumerate(texts):
            eng = engines[omit]
            eng.upload(0, text)
            wants[i], n = products_of(eng, cap, dict(c, omit=omit), text, M, wants.get(i), out)
            looped += n
            sites, prods = wants[i]
            if entry is None:
                assert p in prods
            else:
                assert any(s[0] == p and s[1] == entry and s[2] == M for s in sites) == reported, (p, entry, omit)
    finally:
        for eng in engines.values():
            eng.close()
    return out, looped


@pytest.mark.parametrize("cap", RUNS)
@pytest.mark.parametrize("kind,M", [(k, M) for k in ("flank", "primer") for M in range(4)])
def test_products_sites_at_every_start_across_a_tile_edge(kind, M, cap, monkeypatch):
    if (kind, M) not in _EDGE_BASE:
        _EDGE_BASE[kind, M] = product_edge_run(monkeypatch, kind, M, None)
    base, never = _EDGE_BASE[kind, M]
    assert never == 0
    if cap is None:
        return
    out, looped = product_edge_run(monkeypatch, kind, M, cap)
    assert out == base
    # (a tile and a tail are two tiles: the workgroup of cap 1 takes both; a text leaves two digests)
    n1, n2 = PP.EDGE_FLANK if kind == "flank" else PP.EDGE_PRIMER
    assert len(base) >= ((max(n1, n2) + 6) * 4 * 5 - 8 + 6) * 2
    assert looped == (len(base) // 2 if cap < 2 else 0), (looped, len(base))


@pytest.mark.parametrize("name,M,more", PP.DENSE_CASES)
def test_products_dense_output(name, M, more, monkeypatch):
    """every valid window a site on both strands, four closing sites in reach of every opening site, the second tile
    without a site"""
    n1, n2 = PP.DENSE_LENGTHS
    mp = n1 + n2 + 3
    text, left, right, pairs, want_s, want_p = PP.dense_case(name, M, more)
    tiles = np.bincount(np.array([s[0] for s in want_s]) // TILE, minlength=4)
    assert tiles[1] == 0 and tiles[0] and tiles[2] and tiles[3] and len(want_p) > 4 * TILE
    c = dict(left=left, right=right, Le=n1, Re=n2, pairs=pairs, max_product=mp, omit=False)
    runs, looped = {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        with PP.engine(n1, n2, False, len(text)) as eng:
            eng.upload(0, text)
            eng.primers_table(left + right, len(left), pairs, M, mp)
            _, looped[cap] = products_of(eng, cap, dict(c, kind="primer"), text, M, (want_s, want_p), runs[cap])
            if not more:
                eng.products_table(PS.u8(left, n1), PS.u8(right, n2), pairs, M, mp)
                _, n = products_of(eng, cap, dict(c, kind="flank"), text, M, (want_s, want_p), runs[cap])
                looped[cap] += n
    hold_to_the_first_run(runs, looped, 4)


@pytest.mark.parametrize("name", list(PC.LENGTH_SETS))
def test_primer_products_of_every_length_set(name, monkeypatch):
    runs, looped = {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        for omit in (False, True):
            with PP.engine(30, 30, omit, PC.N_TEXT) as eng:
                for M in range(4):
                    text, left, right, pairs, _ = PC.case(name, M)
                    want_s, want_p = PC.reference(name, M, omit)
                    assert len(want_s) > 0 and len(want_p) >= 16
                    c = dict(kind="primer", left=left, right=right, pairs=pairs, max_product=PC.MAX_PRODUCT, omit=omit)
                    eng.upload(0, np.frombuffer(text, dtype=np.uint8))
                    eng.primers_table(left + right, len(left), pairs, M, PC.MAX_PRODUCT)
                    _, n = products_of(eng, cap, c, text, M, (list(want_s), list(want_p)), runs[cap])
                    looped[cap] += n
    hold_to_the_first_run(runs, looped, 4)


# ----------------------------------------------------------------------------
# guide hits
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.SETS))
def test_guide_hits_of_every_seeded_case(name, monkeypatch):
    from krisp_amd import _native
    s = GC.SETS[name]
    G = s["G"]
    pam5, pam3 = GC.MOTIFS[s["motifs"]]
    t_bytes = GH._texts(GC.guides(name))
    runs, looped = {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        with _native.Engine() as eng:
            uploaded = False
            for omit in (False, True):
                GH._locate(eng, G, omit, GC.N_TEXT, uploaded)
                for M in GC.MS:
                    c = GC.case(name, M)
                    eng.upload(0, c["text"])
                    uploaded = True
                    for need in ((False, True) if (pam5 or pam3) else (False,)):
                        eng.guide_hits_table(t_bytes, M, pam5, pam3, need)
                        got, mine = GH._check(eng, c["text"], G, GC.reference(name, M, omit, need))
                        looped[cap] += geometry(eng, cap, len(c["text"]), G)
                        if not need:
                            GC.check_plants(c["plants"], mine, int(omit))
                        runs[cap].append(digest(got, eng.guide_hit_windows(G)))
    hold_to_the_first_run(runs, looped, 4)


@pytest.mark.parametrize("G", GC.GS)
@pytest.mark.parametrize("period", [1, 2])
def test_guide_hits_dense_texts(G, period, monkeypatch):
    """every valid window of a run a hit, N over the whole second tile"""
    from krisp_amd import _native
    import guide_hits_reference as ref
    text, guide, plus, minus = GC.dense(G, period)
    want = {}
    runs, looped = {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        with _native.Engine() as eng:
            GH._locate(eng, G, False, len(text), False)
            eng.upload(0, text)
            for M in (0, 3):
                eng.guide_hits_table(GH._texts([guide]), M)
                if M not in want:
                    want[M] = ref.ref_hits(text, False, [guide], M)
                got, mine = GH._check(eng, text, G, want[M])
                looped[cap] += geometry(eng, cap, len(text), G)
                assert int((mine["strand"] == 0).sum()) == plus and int((mine["strand"] == 1).sum()) == minus
                assert not ((mine["pos"] >= TILE) & (mine["pos"] < 2 * TILE)).any()
                runs[cap].append(digest(got, eng.guide_hit_windows(G)))
    hold_to_the_first_run(runs, looped, 4)


# ----------------------------------------------------------------------------
# bulged guide hits
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
def test_guide_bulges_of_every_seeded_case(name, monkeypatch):
    from krisp_amd import _native
    c = BC.case(name)
    G, M, B, pam5, pam3 = c["G"], c["M"], c["B"], c["pam5"], c["pam3"]
    t_bytes = GB._texts(c["guides"])
    runs, looped = {}, {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        runs[cap], looped[cap] = [], 0
        with _native.Engine() as eng:
            uploaded = False
            for omit in (False, True):
                GB._locate(eng, G, omit, BC.N_TEXT, uploaded)
                eng.upload(0, c["text"])
                uploaded = True
                for need in ((False, True) if (pam5 or pam3) else (False,)):
                    eng.guide_bulges_table(t_bytes, M, B, pam5, pam3, need)
                    got, mine = GB._check(eng, c["text"], G, B, BC.reference(name, int(omit), need))
                    looped[cap] += geometry(eng, cap, len(c["text"]), BC.half(G, B))
                    if not need:
                        BC.check_plants(c["plants"], mine, int(omit))
                    runs[cap].append(digest(got, eng.guide_bulge_windows(G + B)))
    hold_to_the_first_run(runs, looped, 4)


def test_guide_bulges_dense_text(monkeypatch):
    """a period-G repeat of a guide (one tile): a block of 256 seed pairs writes more than 256 rows; with the cap the rows'
    windows are cut by one, two and three striding workgroups"""
    from krisp_amd import _native
    import guide_bulges_reference as ref
    text, guides, M, B = BC.dense()
    G = len(guides[0])
    want = ref.ref_bulge_hits(text, False, guides, M, B)
    pairs = BC.seed_pairs(text, False, guides, M, B)
    assert pairs > 256 and len(want) > pairs
    runs = {}
    for cap in RUNS:
        set_cap(monkeypatch, cap)
        with _native.Engine() as eng:
            GB._locate(eng, G, False, len(text), False)
            eng.upload(0, text)
            eng.guide_bulges_table(GB._texts(guides), M, B)
            got, _ = GB._check(eng, text, G, B, want)
            assert geometry(eng, cap, len(text), BC.half(G, B)) == 0
            assert eng.debug_scan()["blocks"] > 1                         # (the extend step's blocks of 256 pairs)
            runs[cap] = digest(got, eng.guide_bulge_windows(G + B))
    assert runs[1] == runs[2] == runs[3] == runs[None]

"""All six one-genome scans in ONE engine (csrc/h_scan.inc and the passes' host files): the locate pass and the five seed
passes -- near matches, guide hits, bulged guide hits, flank products, primer products -- each keep a table, lists and
counts of their own in the context, and share only the two-pass scratch.  The other modules put two passes side by side;
here every table is resident at once, so two passes that ended up on one buffer would write over each other.

One text of a tile and a tail (scan_table_cases' shape and geometry: (7, 6, 7), K = 20, which every pass takes), a few
dozen rows a table, M = 1.  What each pass must give comes from an engine that holds that pass's table alone, checked
against the definitions by the pass's own module's helper (SP.check_locate, SP.check_near, GH._check, GB._check,
PP.check_products, PP.check_primers).  In the one engine the six scans run in one order, then in the reverse order, then
-- after another table for the near pass and the primer pass -- the other four again: the lists', windows' and sites'
bytes and the tables' sizes equal the single engines', every list is non-empty and holds both strands.  Once without
KR_SCAN_GRID and once with KR_SCAN_GRID = 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import product_scan_cases as PS                                            # noqa: E402
import scan_table_cases as TC                                              # noqa: E402
import test_gpu_guide_bulges as GB                                         # noqa: E402
import test_gpu_guide_hits as GH                                           # noqa: E402
import test_gpu_product_scan_properties as PP                              # noqa: E402
import test_gpu_scan_grid as SG                                            # noqa: E402
import test_gpu_scan_properties as SP                                      # noqa: E402
import guide_bulges_reference as bulged                                    # noqa: E402
import guide_hits_reference as plain                                       # noqa: E402

pytestmark = pytest.mark.gpu

L, D, R = TC.GEOMETRY
K = TC.K                            # the protospacer's length too: the bulged pass's least
M = 1
BULGES = 1
PAM3 = "NGG"
FLANK_MAX = 90                      # max_product of the flank pass, of the primer pass
PRIMER_MAX = 120
ROWS = 30
PASSES = ("locate", "near", "ghit", "gbulge", "prod", "prim")
SECOND = {"near": "near2", "prim": "prim2"}             # the passes that get another table in between, and its name
_CASE = {}
_WANT = {}


def _rows(text, starts, rng, n, most):
    """n windows of the text, of either strand, with 0 .. most substitutions in turn"""
    return [TC._substitute(TC._window(text, starts, rng), rng.choice(K, size=i % (most + 1), replace=False).tolist(), rng)
            for i in range(n)]


def _pairs_of(text, starts, rng, n, lengths, reach):
    """n (left, right) texts whose product lies in the text, on the forward strand and the other in turn; lengths: what a
    text may have; reach: the most letters from the left text's first to the right text's last"""
    bad = np.concatenate([[0], np.cumsum(text == 10)])
    clear = [int(p) for p in starts if p + reach <= len(text) and bad[p + reach] == bad[p]]
    left, right = [], []
    for i in range(n):
        p = clear[int(rng.integers(0, len(clear)))]
        n1, n2 = (int(lengths[int(rng.integers(0, len(lengths)))]) for _ in (0, 1))
        q = p + n1 + int(rng.integers(0, reach - n1 - n2 + 1))
        a, b = text[p:p + n1], text[q:q + n2]
        if i % 3 == 2:                                          # a substitution in one of the two
            a = TC._substitute(a, [int(rng.integers(0, n1))], rng)
        a, b = (a, b) if i % 2 == 0 else (TC.rc(b), TC.rc(a))
        left.append(bytes(a))
        right.append(bytes(b))
    pairs = [(i, i) for i in range(n)] + [(i, (i + 1) % n) for i in range(0, n, 5)]
    return left, right, pairs


def case():
    if _CASE:
        return _CASE
    rng = np.random.default_rng(50)
    text = TC._text(rng)
    starts = TC._starts(text)
    seen, flanks = set(), []
    while len(flanks) < ROWS:
        w = TC._window(text, starts, rng)
        f = np.concatenate([w[:L], w[L + D:]])
        if f.tobytes() not in seen:
            seen.add(f.tobytes())
            flanks.append(f)
    guides = lambda rows: [bytes(r).decode("ascii") for r in rows]          # noqa: E731
    _CASE.update(
        text=text, flanks=np.array(flanks, dtype=np.uint8),
        near=(np.array(_rows(text, starts, rng, ROWS, M + 1), dtype=np.uint8), M),
        near2=(np.array(_rows(text, starts, rng, ROWS + 7, 3), dtype=np.uint8), 2),
        ghit=guides(_rows(text, starts, rng, ROWS, M + 1)),
        gbulge=guides(_rows(text, starts, rng, ROWS - 6, M)),
        prod=_pairs_of(text, starts, rng, ROWS, [L], FLANK_MAX),
        prim=_pairs_of(text, starts, rng, ROWS, [10, 11, 12, 13, 14], PRIMER_MAX) + (M,),
        prim2=_pairs_of(text, starts, rng, ROWS - 9, [10, 12, 14], PRIMER_MAX) + (0,))
    return _CASE


def table(eng, c, name):
    """the pass's table (name: a pass, or the second table of one) -> its slots"""
    if name == "locate":
        return eng.locate_table(c["flanks"])
    if name in ("near", "near2"):
        return eng.near_table(*c[name])
    if name == "ghit":
        return eng.guide_hits_table(GH._texts(c["ghit"]), M, "", PAM3)
    if name == "gbulge":
        return eng.guide_bulges_table(GB._texts(c["gbulge"]), M, BULGES, "", PAM3)
    if name == "prod":
        left, right, pairs = c["prod"]
        return eng.products_table(PS.u8(left, L), PS.u8(right, R), pairs, M, FLANK_MAX)
    left, right, pairs, m = c[name]
    return eng.primers_table(left + right, len(left), pairs, m, PRIMER_MAX)


def scan(eng, name):
    """the pass's scan of the genome under id 0 -> (its list, its windows or sites); name as table()'s"""
    if name == "locate":
        return eng.locate(0), eng.locate_windows(K)
    if name in ("near", "near2"):
        return eng.near(0), eng.near_windows(K)
    if name == "ghit":
        return eng.guide_hits(0), eng.guide_hit_windows(K)
    if name == "gbulge":
        return eng.guide_bulges(0), eng.guide_bulge_windows(K + BULGES)
    if name == "prod":
        return eng.products(0), eng.product_sites()
    return eng.primer_products(0), eng.primer_sites()


def check(eng, c, name):
    """the engine's scan against the definition, by the helper of the pass's own module"""
    text = c["text"]
    if name == "locate":
        SP.check_locate(eng, text, L, D, R, False, c["flanks"])
    elif name in ("near", "near2"):
        SP.check_near(eng, text, L, D, R, False, *c[name])
    elif name == "ghit":
        GH._check(eng, text, K, plain.ref_hits(text, False, c["ghit"], M, "", PAM3))
    elif name == "gbulge":
        GB._check(eng, text, K, BULGES, bulged.ref_bulge_hits(text, False, c["gbulge"], M, BULGES, "", PAM3))
    elif name == "prod":
        left, right, pairs = c["prod"]
        PP.check_products(eng, text, False, left, right, L, R, pairs, M, FLANK_MAX)
    else:
        left, right, pairs, m = c[name]
        PP.check_primers(eng, text, False, left, right, pairs, m, PRIMER_MAX)


def both_strands(name, hits, more):
    if name in ("prod", "prim", "prim2"):
        return set(hits["strand"].tolist()) == {0, 1} and set((more["entry"] & 1).tolist()) == {0, 1}
    return set(hits["strand"].tolist()) == {0, 1}


def result(eng, name, slots):
    hits, more = scan(eng, name)
    assert len(hits) > 0 and len(more) > 0 and both_strands(name, hits, more), (name, len(hits), len(more))
    return SG.digest(hits, more), len(hits), len(more), int(slots)


def wanted(monkeypatch):
    """name -> what an engine that holds this table alone gives (without KR_SCAN_GRID): computed once, shared"""
    if _WANT:
        return _WANT
    c = case()
    SG.set_cap(monkeypatch, None)
    for name in PASSES:
        with SP.engine(L, D, R, False, TC.N_TEXT) as eng:
            eng.upload(0, c["text"])
            for t in (name, SECOND.get(name)):
                if t:
                    slots = table(eng, c, t)
                    check(eng, c, t)
                    _WANT[t] = result(eng, t, slots)
    assert _WANT["near2"][:3] != _WANT["near"][:3] and _WANT["prim2"][:3] != _WANT["prim"][:3]
    return _WANT


@pytest.mark.parametrize("cap", [None, 1])
def test_six_tables_in_one_engine(cap, monkeypatch):
    c = case()
    want = wanted(monkeypatch)
    SG.set_cap(monkeypatch, cap)
    with SP.engine(L, D, R, False, TC.N_TEXT) as eng:
        slots = {name: table(eng, c, name) for name in PASSES}
        eng.upload(0, c["text"])
        for order in (PASSES, PASSES[::-1]):
            for name in order:
                assert result(eng, name, slots[name]) == want[name], (name, order[0])
        assert eng.debug_scan()["cap"] == (cap or 0)
        for name, second in SECOND.items():
            slots[second] = table(eng, c, second)
        for name in PASSES:
            name = SECOND.get(name, name)
            assert result(eng, name, slots[name]) == want[name], (name, "after the second tables")
    print("cap", cap, "(list, windows or sites, slots)", {name: w[1:] for name, w in want.items()})

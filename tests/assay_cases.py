"""The texts test_assay_cases.py and test_gpu_assay.py hold the assay join to: a random text of one tile of the
scans and a tail, with planted LOCI of the form primer site, interior with a guide site, primer site -- on both strands,
with the guide in both orientations, 0 .. M + 1 substitutions in each part, around separators, N and lower case, across
the tile edge --, and the shapes only the join has: 1, 257 and more than 512 products (the 256-product blocks of its
count, scan and emit: a short repeated unit), products without a hit, hits without a product, the last hit inside the last
product, a product behind every hit.  case(name) returns the tables and the text; reference(name) the brute-force lists
(primers_reference, guide_hits_reference, assay_reference), computed once per process; test_assay_cases.py holds the
REFERENCE's lists to the conditions the case set is built for, so the GPU test compares nothing against an empty list."""
import functools
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from assay_reference import ref_assay_hits                                  # noqa: E402
from guide_hits_reference import ref_hits                                   # noqa: E402
from primers_reference import ref_products, ref_sites                      # noqa: E402

TILE = 256 * 64                     # window starts of a tile of the scans (LOC_T * LOC_S)
N_TEXT = TILE + 900                 # a tile and a tail
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

# the regions of the spread cases: (primer pair, guide text or None).  Regions 0 and 1 share pair 0 AND guide 0 (one link,
# two regions), regions 2 and 3 share guide 1 under pairs of their own, region 4 has a pair and no guide
REGIONS = [(0, 0), (0, 0), (1, 1), (2, 1), (3, None), (4, 2)]
NAMES = ["spread_m1_m2", "spread_m0_m0_omit", "spread_m2_m3_pam", "one_product", "blocks_257", "blocks_520", "products_no_hit",
         "hits_no_product", "last_hit_in_last_product", "product_behind_every_hit"]


def rc(b):
    return b[::-1].translate(_COMP)


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _mutate(rng, text, nsub):
    t = bytearray(text)
    for c in rng.sample(range(len(t)), nsub):
        t[c] = rng.choice([b for b in b"ACGT" if b != t[c]])
    return bytes(t)


def links_of(regions):
    """-> (links, ascending and unique; the regions of each) from (pair, guide or None) per region: the definition of a link"""
    by = {}
    for r, (p, g) in enumerate(regions):
        if g is not None:
            by.setdefault((p, g), []).append(r)
    keys = sorted(by)
    return keys, [by[k] for k in keys]


def _tables(rng, G, lens):
    """5 left and 5 right texts of the lengths `lens`, pairs (i, i), 3 guide texts of G letters"""
    left = [_rand(rng, lens[i % len(lens)]) for i in range(5)]
    right = [_rand(rng, lens[(i + 2) % len(lens)]) for i in range(5)]
    guides = [_rand(rng, G) for _ in range(3)]
    return left, right, [(i, i) for i in range(5)], guides


class _Text:
    def __init__(self, rng, n=N_TEXT):
        self.rng, self.t = rng, bytearray(_rand(rng, n))

    def put(self, p, b):
        assert 0 <= p and p + len(b) <= len(self.t), (p, len(b))
        self.t[p:p + len(b)] = b
        return len(b)


def _locus(rng, left, right, guides, pair, guide, gs, gl, gr, ml=0, mg=0, mr=0, strand=0):
    """left text, gl random bases, the guide (its reverse complement for gs = 1), gr random bases, right text -- as a '+'
    product reads; the reverse complement of it all for strand 1.  guide None: 20 random bases in its place"""
    a, b = _mutate(rng, left[pair], ml), _mutate(rng, right[pair], mr)
    g = _rand(rng, 20) if guide is None else _mutate(rng, guides[guide], mg)
    amp = a + _rand(rng, gl) + (rc(g) if gs else g) + _rand(rng, gr) + b
    return rc(amp) if strand else amp


def _spread(name, Mp, Mg, omit, pam5="", pam3="", need=False):
    rng = random.Random(name)
    G = 20
    left, right, pairs, guides = _tables(rng, G, [18, 24, 21, 19, 22])
    tx = _Text(rng)
    at = [200]

    def put(b, step=None):
        p = at[0]
        tx.put(p, b)
        at[0] += (len(b) + 60) if step is None else step
        return p

    # every region's locus, exact, both product strands x both guide orientations
    for r, (p, g) in enumerate(REGIONS):
        for strand in (0, 1):
            for gs in (0, 1):
                put(_locus(rng, left, right, guides, p, g, gs, rng.choice([0, 3, 17]), rng.choice([0, 5, 30]), strand=strand))
    # 0 .. M + 1 substitutions in each part
    for i in range(24):
        p, g = REGIONS[(0, 2, 3, 5)[i % 4]]
        put(_locus(rng, left, right, guides, p, g, i & 1, 4, 9, ml=i % (Mp + 2), mg=(i // 2) % (Mg + 2), mr=(i // 3) % (Mp + 2),
                   strand=(i >> 1) & 1))
    # flush with either end of the interior, and with both
    put(_locus(rng, left, right, guides, 0, 0, 0, 0, 12))
    put(_locus(rng, left, right, guides, 1, 1, 1, 12, 0, strand=1))
    put(_locus(rng, left, right, guides, 2, 1, 0, 0, 0))                   # an interior of exactly G bases
    # the guide reaches two bases into the first site (its first letters become the primer's: <= 2 mismatches), and into the second
    put(left[0] + guides[0][2:] + _rand(rng, 6) + right[0])
    put(left[0] + _rand(rng, 6) + guides[0][:-2] + right[0])
    # the guide before the product, behind it, and beyond a separator that ends the record before the product
    put(guides[0] + _rand(rng, 5) + _locus(rng, left, right, guides, 0, None, 0, 3, 3))
    put(_locus(rng, left, right, guides, 0, None, 0, 3, 3) + _rand(rng, 5) + guides[0])
    p = put(guides[0] + b"\n" + _locus(rng, left, right, guides, 0, None, 0, 3, 3))
    # another region's guide inside the product: no link (pair 3 has no guide at all, pair 1 has guide 1)
    put(_locus(rng, left, right, guides, 3, 0, 0, 4, 4))
    put(_locus(rng, left, right, guides, 1, 0, 1, 4, 4, strand=1))
    # two hits in one interior; one hit in two products (the left text twice before it)
    put(left[0] + _rand(rng, 2) + guides[0] + _rand(rng, 7) + rc(guides[0]) + _rand(rng, 2) + right[0])
    put(left[2] + _rand(rng, 3) + left[2] + _rand(rng, 1) + guides[1] + _rand(rng, 4) + right[2])
    # separators, N and lower case: around the locus, inside the interior beside the guide, inside the guide
    p = put(_locus(rng, left, right, guides, 0, 0, 0, 6, 6))
    tx.t[p - 1] = tx.t[p + len(left[0]) + 6 + G + 6 + len(right[0])] = ord("\n")
    p = put(_locus(rng, left, right, guides, 0, 0, 0, 6, 6))
    tx.t[p + len(left[0]) + 2] = ord("\n")                                  # a separator in the interior: no product
    p = put(_locus(rng, left, right, guides, 0, 0, 0, 6, 6))
    tx.t[p + len(left[0]) + 2] = ord("N")                                   # an N in the interior: the product stands, the hit too
    p = put(_locus(rng, left, right, guides, 0, 0, 0, 6, 6))
    tx.t[p + len(left[0]) + 6 + 4] = ord("n")                               # an n in the guide: no hit
    w = _locus(rng, left, right, guides, 4, 2, 1, 6, 6)
    p = put(w.lower())                                                    # all lower case: a row unless omit
    w = _locus(rng, left, right, guides, 2, 1, 0, 6, 6)
    p = put(w[:len(left[2]) + 6] + w[len(left[2]) + 6:len(left[2]) + 6 + G].lower() + w[len(left[2]) + 6 + G:])
    assert at[0] < TILE - 400, at[0]
    # across the tile edge: the first site before it, the guide on it, the second site behind it; then the tail's own loci,
    # the last one a long product
    tx.put(TILE - len(left[0]) - 8, _locus(rng, left, right, guides, 0, 0, 1, 2, 9))
    tx.put(TILE + 200, _locus(rng, left, right, guides, 1, 1, 0, 2, 9, strand=1))
    tx.put(N_TEXT - 320, _locus(rng, left, right, guides, 4, 2, 0, 200, 5, strand=1))
    links, link_regions = links_of(REGIONS)
    return dict(text=bytes(tx.t), left=left, right=right, pairs=pairs, guides=guides, G=G, Mp=Mp, Mg=Mg, omit=omit, pam5=pam5, pam3=pam3,
                need=need, max_product=300, links=links, link_regions=link_regions, regions=REGIONS)


def _units(name, units, loci=(), G=12, stray_guides=(), tail_product=False):
    """Mp = Mg = 0.  `units` copies of a unit of 32 bases -- a left text of 10, the guide of 12, a right text of 10 -- with
    max_product = 32: a product per unit, a hit in each.  loci: (position, pair, guide or None) single loci beside them"""
    rng = random.Random(name)
    left, right, pairs, guides = _tables(rng, G, [10])
    tx = _Text(rng)
    unit = left[0] + guides[0] + right[0]
    assert len(unit) == 32
    tx.put(100, unit * units)
    for p, pair, g in loci:
        w = left[pair] + (guides[g] if g is not None else _rand(rng, G)) + right[pair]
        tx.put(p, w)
    for p, g in stray_guides:
        tx.put(p, guides[g])
    regions = [(0, 0), (1, 1), (2, None)]
    links, link_regions = links_of(regions)
    return dict(text=bytes(tx.t), left=left, right=right, pairs=pairs, guides=guides, G=G, Mp=0, Mg=0, omit=False, pam5="", pam3="",
                need=False, max_product=32, links=links, link_regions=link_regions, regions=regions)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: text, left, right, pairs, guides (the tables), G, Mp, Mg, omit, pam5, pam3, need, max_product, links,
    link_regions, regions"""
    if name == "spread_m1_m2":
        return _spread(name, 1, 2, False)
    if name == "spread_m0_m0_omit":
        return _spread(name, 0, 0, True)
    if name == "spread_m2_m3_pam":
        return _spread(name, 2, 3, False, pam5="N", pam3="H", need=True)
    if name == "one_product":
        return _units(name, 1)
    if name == "blocks_257":
        return _units(name, 257)
    if name == "blocks_520":
        return _units(name, 520)                    # (over the tile edge: 100 + 520 * 32 = 16740)
    if name == "products_no_hit":
        return _units(name, 0, loci=[(300 + 80 * i, i % 3, None) for i in range(40)])
    if name == "hits_no_product":
        return _units(name, 0, stray_guides=[(300 + 50 * i, i % 3) for i in range(40)])
    if name == "last_hit_in_last_product":
        return _units(name, 3, loci=[(5000, 1, 1), (N_TEXT - 40, 0, 0)], stray_guides=[(2000, 0), (3000, 1)])
    if name == "product_behind_every_hit":
        return _units(name, 2, loci=[(9000, 1, None)], stray_guides=[(4000, 1)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (products, hits, assay hits) of case(name): numpy arrays of the references' dtypes, computed once, shared by the
    tests, not changed"""
    c = case(name)
    texts = c["left"] + c["right"]
    sites = ref_sites(c["text"], c["omit"], texts, len(c["left"]), c["Mp"])
    prods = ref_products(c["text"], c["omit"], texts, len(c["left"]), c["pairs"], c["Mp"], c["max_product"], sites=sites)
    hits = ref_hits(c["text"], c["omit"], c["guides"], c["Mg"], c["pam5"], c["pam3"], c["need"])
    seps = np.flatnonzero(np.frombuffer(c["text"], dtype=np.uint8) == ord("\n")).tolist()
    rows = ref_assay_hits(prods, hits, lengths(c), c["links"], c["G"], seps)
    for a in (prods, hits, rows):
        a.setflags(write=False)
    return prods, hits, rows


def lengths(c):
    return [(len(c["left"][i]), len(c["right"][j])) for i, j in c["pairs"]]


def separators(c):
    return np.flatnonzero(np.frombuffer(c["text"], dtype=np.uint8) == ord("\n")).tolist()

"""The texts test_primers_host.py and test_gpu_primers.py hold the primer-product pass to: a random text over three tiles of
the scan (a fourth begun), 8 left and 8 right primer texts of mixed lengths, 12 pairs that share them, copies planted with
0 .. M + 1 substitutions per text on both strands, across separators, with N and lower case between and inside sites -- as
test_gpu_products._case plants them -- and the cases only mixed lengths have (SPECIALS below).  case() returns the marks
of what it planted; test_primers_host.generator_did_its_work holds the REFERENCE's lists to them, so nothing is compared
against an empty list.  reference() computes the brute-force lists once per process."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from primers_reference import ref_products, ref_sites                      # noqa: E402

TILE = 256 * 64                     # window starts of a tile of the scan (LOC_T * LOC_S)
N_TEXT = 3 * TILE + 900             # the smallest shape with two interior tile edges
SLOT = 1024                         # the text is laid out in slots: a spread copy, a special, and near a tile edge its plants
SPREAD_AT, SPECIAL_AT = 140, 540
MAX_PRODUCT = 300
PAIRS = [(i, i) for i in range(8)] + [(0, 1), (0, 2), (3, 2), (7, 0)]

# name -> (lengths of the 8 left texts, of the 8 right texts).  In every set text 0 of either side is of the longest length
# and text 1 a shorter prefix of it (not in "16": one length); left text 0 is paired with right texts 0 and 1
LENGTH_SETS = {
    "10-14": ([14, 10, 11, 12, 13, 14, 10, 12], [14, 10, 13, 12, 11, 10, 14, 13]),
    "18-24": ([24, 18, 19, 20, 21, 22, 18, 23], [24, 18, 23, 22, 21, 20, 19, 24]),
    "10,60": ([60, 10, 10, 60, 10, 60, 10, 60], [60, 10, 60, 10, 10, 60, 60, 10]),
    "10,11,37,60": ([60, 10, 37, 10, 11, 37, 10, 60], [60, 11, 37, 11, 10, 60, 37, 11]),
    "16": ([16] * 8, [16] * 8),
}
SHORTEST_LEFT = 6                   # a left text of the shortest length that is no prefix (the text's last window)

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(b):
    return b[::-1].translate(_COMP)


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _mutate(rng, text, nsub, cols=None):
    t = bytearray(text)
    for c in rng.sample(list(range(len(t)) if cols is None else cols), nsub):
        t[c] = rng.choice([b for b in b"ACGT" if b != t[c]])
    return bytes(t)


def entry_lengths(left, right):
    return [len(t) for t in left for _ in (0, 1)] + [len(t) for t in right for _ in (0, 1)]


def case(name, M):
    """-> (text, left texts, right texts, PAIRS, marks).  marks: name -> what test_primers_host checks in the reference's
    lists (positions and entries of the planted special cases; a key is absent where the set cannot have the case)"""
    llen, rlen = LENGTH_SETS[name]
    rng = random.Random(f"{name}/{M}")
    smin, lmax = min(llen + rlen), max(llen + rlen)
    mixed = lmax > smin
    assert llen[SHORTEST_LEFT] == smin and llen[0] == rlen[0] == lmax
    left = [_rand(rng, n) for n in llen]
    right = [_rand(rng, n) for n in rlen]
    if mixed:
        # left 0 holds the shortest text one byte before its end (the end of the text below), text 1 is a prefix of text 0
        left[0] = _rand(rng, lmax - 1 - smin) + left[SHORTEST_LEFT] + _rand(rng, 1)
        left[1] = left[0][:llen[1]]
        right[1] = right[0][:rlen[1]]
    right[2] = left[2][-1:] + right[2][1:]          # (left 2 and right 2 can overlap by one)
    texts = left + right
    assert len(set(texts)) == 16
    text = bytearray(_rand(rng, N_TEXT))
    marks = {}

    def put(p, b):
        assert 0 <= p and p + len(b) <= N_TEXT
        text[p:p + len(b)] = b
        return len(b)

    def plant(p, pair, strand, gap, ml=0, mr=0, end_l=False, end_r=False):
        a, b = left[PAIRS[pair][0]], right[PAIRS[pair][1]]
        a = _mutate(rng, a, ml, range(len(a) - 5, len(a)) if end_l else None)
        b = _mutate(rng, b, mr, range(5) if end_r else None)
        amp = a + _rand(rng, gap) + b
        return put(p, rc(amp) if strand else amp)

    # spread over the slots, 4 rounds of the 12 pairs: the first round exact, then every number of substitutions on either
    # text up to one more than allowed; pairs 0-2 and 6-8 on '+', the others on '-'
    for i in range(48):
        r = i // 12
        ml, mr = (0, 0) if r == 0 else ((r + i) % (M + 2), (r + i // 3) % (M + 2))
        gap = rng.choice([0, 1, 7, 40, 150] if r == 0 else [0, 1, 7, 40, 150, 250])
        plant(i * SLOT + SPREAD_AT, i % 12, (i // 3) & 1, gap, ml, mr, end_l=i % 5 == 0, end_r=i % 7 == 0)

    specials = []

    def special(fn):
        specials.append(fn)
        return fn

    # ---- what test_gpu_products._case plants: separators, N, lower case
    @special
    def sep_between(p):
        plant(p, 0, 0, 30)
        text[p + len(left[0]) + 10] = ord("\n")

    @special
    def sep_inside(p):
        plant(p, 1, 1, 30)
        text[p + 3] = ord("\n")

    @special
    def sep_around(p):
        w = plant(p, 2, 0, 12)
        text[p + w] = ord("\n")
        text[p - 1] = ord("\n")
        marks["sep_around"] = (p, w, 0, 2)

    @special
    def n_between(p):
        w = plant(p, 3, 0, 20)
        text[p + len(left[3]) + 5] = ord("N")
        marks["n_between"] = (p, w, 0, 3)

    @special
    def n_inside(p):
        plant(p, 4, 1, 20)
        text[p + 2] = ord("n")
        marks["n_inside"] = (p, 16 + 2 * 4 + 1)           # rc(right 4) opens there: no site

    @special
    def lower_whole(p):
        w = plant(p, 5, 0, 25)
        text[p:p + w] = bytes(text[p:p + w]).lower()
        marks["lower_whole"] = (p, w, 0, 5)                 # a product unless omit

    @special
    def lower_between(p):
        w = plant(p, 6, 1, 25)
        n1 = len(right[6])
        text[p + n1:p + n1 + 25] = bytes(text[p + n1:p + n1 + 25]).lower()
        marks["lower_between"] = (p, w, 1, 6)

    # ---- what only mixed lengths have
    if mixed:
        @special
        def tail_sep(p):
            put(p, left[0])
            text[p + smin] = ord("\n")                       # the first byte past the seeded columns
            marks["tail_sep"] = (p, 0, 2)                    # no site of left 0, a site of its prefix left 1

        @special
        def tail_n(p):
            put(p, left[0])
            text[p + lmax - 1] = ord("N")                    # the tail's last byte
            marks["tail_n"] = (p, 0, 2)

        @special
        def tail_mismatches(p):
            put(p, _mutate(rng, left[0], M, range(smin, lmax)))
            marks["tail_mismatches"] = (p, 0, M)             # a site of left 0 with M mismatches

        @special
        def head_and_tail(p):
            put(p, _mutate(rng, _mutate(rng, left[0], M, range(smin)), 1, range(smin, lmax)))
            marks["head_and_tail"] = (p, 0)                  # M + 1 mismatches: no site

        @special
        def prefix(p):
            put(p, right[0])
            marks["prefix"] = (p, 16, 18)                    # right 0 and right 1 are sites at one position

        @special
        def max_product_pair(p):
            # left 0 ... right 0, one byte too long; right 1, its prefix, closes a product that fits
            a, b = left[0], right[0]
            put(p, a + _rand(rng, MAX_PRODUCT + 1 - len(a) - len(b)) + b)
            marks["max_product_pair"] = (p, MAX_PRODUCT + 1 - (len(b) - len(right[1])), 8, MAX_PRODUCT + 1, 0)

    @special
    def end_opening(p):
        # a mismatch among the last five columns of the longest opening text (left 0 on '+')
        a = _mutate(rng, left[0], min(M, 1), range(lmax - 5, lmax))
        w = put(p, a + _rand(rng, 20) + right[0])
        marks["end_opening"] = (p, w, 0, 0)

    @special
    def end_closing(p):
        # a mismatch among the first five columns of a closing text (right 0 on '+')
        b = _mutate(rng, right[0], min(M, 1), range(5))
        w = put(p, left[0] + _rand(rng, 20) + b)
        marks["end_closing"] = (p, w, 0, 0)

    @special
    def abut(p):
        w = put(p, left[2] + right[2])
        marks["abut"] = (p, w, 0, 2)

    @special
    def overlap(p):
        w = put(p, left[2] + right[2][1:])
        marks["overlap"] = (p, w, 4, p + len(left[2]) - 1, 16 + 4)   # both sites, no product of pair 2 there

    for s, fn in enumerate(specials):
        fn((2 * s + 1) * SLOT + SPECIAL_AT)

    # ---- the tile edges: a site of the longest text that starts one byte before the edge, inside a product that
    # straddles it ('+' at the first and third edge, '-' at the second)
    marks["edges"] = []
    for q, edge in enumerate((TILE, 2 * TILE, 3 * TILE)):
        a, b = left[4], right[4]
        if q == 1:
            a, b = rc(b), rc(a)
        put(edge - 140, a)
        put(edge - 1, left[0])
        put(edge + 65, b)
        marks["edges"].append((edge, edge - 140, 205 + len(b), q & 1, 4))

    # ---- the end of the text: the last window is a site of the shortest text; the longest text's seeded columns fit
    # before the end, its last byte does not
    if mixed:
        put(N_TEXT - (lmax - 1), left[0][:lmax - 1])
        marks["tail_end"] = (N_TEXT - (lmax - 1), 0)
    else:
        put(N_TEXT - smin, left[SHORTEST_LEFT])
    marks["last_window"] = (N_TEXT - smin, 2 * SHORTEST_LEFT)
    return bytes(text), left, right, PAIRS, marks


@functools.lru_cache(maxsize=None)
def reference(name, M, omit):
    """-> (ref_sites, ref_products) of case(name, M) as lists of tuples: computed once, shared by the tests, not changed"""
    text, left, right, pairs, _ = case(name, M)
    sites = ref_sites(text, omit, left + right, len(left), M)
    prods = ref_products(text, omit, left + right, len(left), pairs, M, MAX_PRODUCT, sites=sites)
    return tuple(tuple(r) for r in sites.tolist()), tuple(tuple(r) for r in prods.tolist())

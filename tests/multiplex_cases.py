"""The texts test_multiplex_cases.py and test_gpu_multiplex.py hold the multiplex pass (kr_multiplex_*) to: a
random text over three tiles of the scan (a fourth begun), T oligo texts of mixed lengths, products planted with 0 .. M + 1
substitutions per site -- of every kind on both readings, across separators, with N and lower case between and inside
sites -- and the plants only this pass has (below).  No code of krisp_amd/.  Texts 2 m and 2 m + 1 are read as member m's
left and right oligo: (2 m, 2 m + 1) and (2 m + 1, 2 m) are `pair` products, (a, a) `single`, everything else `cross`.
case() returns the marks of what it planted; test_multiplex_cases.py holds the REFERENCE's lists to them, so nothing is
compared against an empty list.  reference() computes the brute-force lists once per process.

The join's blocks of 256 sites: a stretch of the text holds nothing but N and what is planted there, so the number of
sites before a plant is known from the reference -- single sites fill up to site number 255 of a block, whose partners
then lie in the next one, and 216 single sites more precede a row of 40 abutting products (DESIGN §16.1's block-edge
plant)."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multiplex_reference import rc, ref_products, ref_sites                # noqa: E402

TILE = 256 * 64                     # window starts of a tile of the scan (LOC_T * LOC_S)
BLOCK = 256                         # sites of a block of the join (LOC_T)
N_TEXT = 3 * TILE + 900             # the smallest shape with two interior tile edges
N_SHORT = 6000                      # T = 128: the reference compares every entry at every position (about 10^8 bytes a call)
SLOT = 1024                         # the text is laid out in slots: a spread product, a special
SPREAD_AT, SPECIAL_AT = 140, 540
MAX_PRODUCT = 300
QUIET = (18 * SLOT, 30 * SLOT)      # the stretch of N: the block plants
LOWER_FROM = 30                     # the first slot a plant with lower case may take (the sites before QUIET do not depend on omit)

LENGTH_SETS = {"10-14": [14, 10, 11, 12, 13], "18-24": [24, 18, 19, 20, 21, 22, 23], "10,60": [60, 10], "16": [16]}
# (length set, T, M): every set with 16 texts at every M; one text, two, and 128 on the short text
CASES = ([(name, 16, M) for name in LENGTH_SETS for M in range(4)] + [("16", 1, M) for M in range(4)]
         + [("10,60", 1, 1), ("10,60", 2, 1), ("10-14", 2, 3), ("18-24", 128, 1), ("10-14", 128, 2), ("10,60", 128, 0)])


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _mutate(rng, text, nsub, cols=None):
    t = bytearray(text)
    for c in rng.sample(list(range(len(t)) if cols is None else cols), nsub):
        t[c] = rng.choice([b for b in b"ACGT" if b != t[c]])
    return bytes(t)


def kind(a, b):
    return "single" if a == b else "pair" if a // 2 == b // 2 else "cross"


def case(name, T, M):
    """-> (text, texts, marks).  marks: name -> what test_multiplex_cases checks in the reference's lists; ("row", pos,
    length, a, b) must be a product, ("no row", pos, length, a, b) must not; other marks are described where they are made.
    A key is absent where the case cannot have the plant."""
    cyc = LENGTH_SETS[name]
    rng = random.Random(f"{name}/{T}/{M}")
    lens = [cyc[i % len(cyc)] for i in range(T)]
    smin, lmax = min(lens), max(lens)
    mixed = lmax > smin
    short = T > 16
    n_text = N_SHORT if short else N_TEXT
    texts = [_rand(rng, n) for n in lens]
    marks = {}
    PAL = RC = LONG = SHORT = None
    if T >= 2:
        texts[1] = texts[1][:-1] + rc(texts[0][-1:])    # (text 0 and rc(text 1) can overlap by one)
    if T >= 8:                                           # (the texts 0 .. 3 stay as they are: the spread's and the specials')
        if 10 in lens:
            PAL = max(i for i in range(T) if lens[i] == 10)
            half = _rand(rng, 5)
            texts[PAL] = half + rc(half)                # its own reverse complement
        same = [i for i in range(4, T) if lens[i] == lens[4] and i != PAL]
        if len(same) >= 2:
            RC = (same[0], same[1])
            texts[RC[1]] = rc(texts[RC[0]])             # a text that is another text's reverse complement
        if mixed:
            taken = (PAL,) + (RC or ())
            LONG = max(i for i in range(4, T) if lens[i] == lmax and i not in taken)
            SHORT = min(i for i in range(4, T) if lens[i] == smin and i not in taken)
            texts[LONG] = _rand(rng, lmax - smin) + texts[SHORT]    # rc(SHORT) is a prefix of rc(LONG): both close at one s2
    assert len(set(texts)) == T
    text = bytearray(_rand(rng, n_text))

    def put(p, b):
        assert 0 <= p and p + len(b) <= n_text
        text[p:p + len(b)] = b
        return len(b)

    def amp(a, b, gap, ma=0, mb=0, end_a=False, end_b=False):
        """the product (a, b): text a, gap letters, rc(text b); the 3' end of either oligo is its last columns as written"""
        x, y = texts[a], texts[b]
        x = _mutate(rng, x, ma, range(len(x) - 5, len(x)) if end_a else range(len(x) - 5))
        y = _mutate(rng, y, mb, range(len(y) - 5, len(y)) if end_b else range(len(y) - 5))
        return x + _rand(rng, gap) + rc(y)

    # ---- the ordered pairs the spread cycles through: every kind on both readings
    combos = [(0, 0)]
    if T >= 2:
        combos += [(0, 1), (1, 0), (1, 1)]
    if T >= 4:
        combos += [(0, 2), (2, 0), (1, 3), (3, 1), (2, 3), (3, 2), (T - 1, 0), (0, T - 1)]
    marks["combos"] = combos
    slots = [s for s in range(n_text // SLOT) if not (QUIET[0] <= s * SLOT < QUIET[1]) or short]
    marks["spread"] = []
    for i, s in enumerate(slots):
        r = i // len(combos)
        a, b = combos[i % len(combos)]
        ma, mb = (0, 0) if r == 0 else ((r + i) % (M + 2), (r + i // 3) % (M + 2))
        gap = rng.choice([0, 1, 7, 40, 150])
        end_a, end_b = i % 2 == 1, i % 3 == 1
        w = put(s * SLOT + SPREAD_AT, amp(a, b, gap, ma, mb, end_a, end_b))
        # (pos, length, a, b, the substitutions of either site and whether they lie in its 3' end)
        marks["spread"].append((s * SLOT + SPREAD_AT, w, a, b, ma, mb, end_a, end_b))

    specials, lowered = [], []

    def special(fn):
        specials.append(fn)
        return fn

    def lower_special(fn):
        lowered.append(fn)
        return fn

    A, B = 0, min(1, T - 1)                              # the pair most specials use (T = 1: one text with itself)
    nA, nB = len(texts[A]), len(texts[B])

    @special
    def single(p):
        w = put(p, amp(A, A, 33))
        marks["single"] = ("row", p, w, A, A)

    @special
    def diverging(p):
        # the closing entry first, the opening entry after it: primers that point away from each other
        w = put(p, rc(texts[B]) + _rand(rng, 30) + texts[A])
        marks["diverging"] = ("no row", p, w, B, A) if T >= 2 else ("no row", p, w, A, A)
        marks["diverging_sites"] = ((p, 2 * B + 1), (p + nB + 30, 2 * A))

    @special
    def abut(p):
        w = put(p, amp(A, B, 0))
        marks["abut"] = ("row", p, w, A, B)

    if T >= 2:
        @special
        def overlap(p):
            w = put(p, texts[A] + rc(texts[B])[1:])
            marks["overlap"] = ("no row", p, w, A, B)
            marks["overlap_sites"] = ((p, 2 * A), (p + nA - 1, 2 * B + 1))

    @special
    def exact_max(p):
        w = put(p, amp(A, B, MAX_PRODUCT - nA - nB))
        marks["exact_max"] = ("row", p, w, A, B)

    @special
    def one_more(p):
        w = put(p, amp(A, B, MAX_PRODUCT + 1 - nA - nB))
        marks["one_more"] = ("no row", p, w, A, B)

    @special
    def sep_between(p):
        w = put(p, amp(A, B, 30))
        text[p + nA + 10] = ord("\n")
        marks["sep_between"] = ("no row", p, w, A, B)

    @special
    def n_between(p):
        w = put(p, amp(A, B, 20))
        text[p + nA + 5] = ord("N")
        marks["n_between"] = ("row", p, w, A, B)

    @special
    def n_inside(p):
        w = put(p, amp(A, B, 20))
        text[p + 2] = ord("n")
        marks["n_inside"] = ("no row", p, w, A, B)

    @lower_special
    def lower_between(p):
        w = put(p, amp(A, B, 25))
        text[p + nA:p + nA + 25] = bytes(text[p + nA:p + nA + 25]).lower()
        marks["lower_between"] = ("row", p, w, A, B)

    @lower_special
    def lower_whole(p):
        w = put(p, amp(A, B, 25))
        text[p:p + w] = bytes(text[p:p + w]).lower()
        marks["lower_whole"] = ("row unless omit", p, w, A, B)

    if PAL is not None:
        @special
        def palindrome(p):
            # every site of a palindrome is an opening and a closing site: it closes itself downstream, never at its own position
            w = put(p, texts[PAL] + _rand(rng, 21) + texts[PAL])
            marks["palindrome"] = ("row", p, w, PAL, PAL)
            marks["palindrome_self"] = ("no row", p, 10, PAL, PAL)
            marks["palindrome_sites"] = ((p, 2 * PAL), (p, 2 * PAL + 1))

    if RC is not None:
        @special
        def rc_text(p):
            # X ... X with text r0 = X and text r1 = rc(X): entry 2 r0 opens, entry 2 r1 + 1 = X closes
            x = texts[RC[0]]
            w = put(p, x + _rand(rng, 17) + x)
            marks["rc_text"] = ("row", p, w, RC[0], RC[1])
            marks["rc_text_not"] = ("no row", p, w, RC[0], RC[0])

    if LONG is not None:
        @special
        def short_long(p):
            # at one s2 the long closing text exceeds max_product by one, its short suffix fits
            w = put(p, amp(A, LONG, MAX_PRODUCT + 1 - nA - lmax))
            marks["short_long"] = ("no row", p, w, A, LONG)
            marks["short_long_fits"] = ("row", p, w - (lmax - smin), A, SHORT)

        @special
        def tail_sep(p):
            put(p, rc(texts[LONG]))
            text[p + smin] = ord("\n")                   # the first byte past the seeded columns
            marks["tail_sep"] = (p, 2 * LONG + 1, 2 * SHORT + 1)     # no site of rc(LONG), a site of its prefix rc(SHORT)

        @special
        def tail_n(p):
            put(p, rc(texts[LONG]))
            text[p + lmax - 1] = ord("N")                # the tail's last byte
            marks["tail_n"] = (p, 2 * LONG + 1, 2 * SHORT + 1)

        @lower_special
        def tail_lower(p):
            put(p, rc(texts[LONG]))
            text[p + lmax - 2] |= 0x20
            marks["tail_lower"] = (p, 2 * LONG + 1)      # a site unless omit

    # the end mismatches of either side, alone and together: the tally's `clean` needs both values
    if M >= 1:
        for ea, eb in ((1, 0), (0, 1), (1, 1)):
            def ends(p, ea=ea, eb=eb):
                w = put(p, amp(A, B, 20, ea, eb, True, True))
                marks[f"ends_{ea}{eb}"] = ("row", p, w, A, B, ea, eb)
            specials.append(ends)

    before = [s for s in slots if s < LOWER_FROM or short]
    after = [s for s in slots if s >= LOWER_FROM and not short]
    todo = specials + (lowered if short else [])
    if short:
        todo = todo[:len(before)]                        # (the short text holds the first few: its case is about the table)
    assert len(todo) <= len(before) and (short or len(lowered) <= len(after))
    for s, fn in zip(before, todo):
        fn(s * SLOT + SPECIAL_AT)
    if not short:
        for s, fn in zip(after, lowered):
            fn(s * SLOT + SPECIAL_AT)

    # ---- the tile edges: a site of the longest text that starts one byte before the edge, inside a product whose opening
    # site lies in the tile before the edge and whose closing site lies behind it
    marks["edges"] = []
    if not short:
        E = lens.index(lmax)
        for q, edge in enumerate((TILE, 2 * TILE, 3 * TILE)):
            a, b = (A, B) if q != 1 else (B, A)
            put(edge - 140, texts[a])
            put(edge - 1, texts[E])
            put(edge + 65, rc(texts[b]))
            marks["edges"].append((edge, ("row", edge - 140, 205 + len(texts[b]), a, b), (edge - 1, 2 * E)))

    # ---- the join's blocks, in the stretch of N (where the single sites are short enough for the stretch to hold them)
    if not short and smin <= 24:
        lo, hi = QUIET
        text[lo:hi] = b"N" * (hi - lo)
        unit = next(texts[i] for i in range(T) if lens[i] == smin and len(ref_sites(b"N" + texts[i] + b"N", False, texts, M)) == 1)
        probe = amp(A, B, 40)
        # (the probe's opening site stands alone at its position: the order of a position's sites is the device's own)
        assert [s[0] for s in ref_sites(b"N" + probe + b"N", False, texts, M)].count(1) == 1
        c0 = sum(1 for s in ref_sites(bytes(text[:lo]), False, texts, M))
        at = lo + 1
        for _ in range((BLOCK - 1 - c0) % BLOCK):
            at += put(at, unit) + 1
        marks["block_255"] = ("row", at, len(probe), A, B)
        at += put(at, probe) + 1
        for _ in range(216):
            at += put(at, unit) + 1
        marks["crowd"] = (at, 40)
        at += put(at, (texts[A] + b"A" + rc(texts[B]) + b"C") * 40) + 1
        assert at < hi

    # ---- the end of the text: the last window is a site of the shortest text
    last = lens.index(smin)
    put(n_text - smin, texts[last])
    marks["last_window"] = (n_text - smin, 2 * last)
    return bytes(text), texts, marks


@functools.lru_cache(maxsize=None)
def reference(name, T, M, omit):
    """-> (ref_sites, ref_products) of case(name, T, M) as tuples of tuples: computed once, shared by the tests, not changed"""
    text, texts, _ = case(name, T, M)
    sites = ref_sites(text, omit, texts, M)
    prods = ref_products(text, omit, texts, M, MAX_PRODUCT, sites=sites)
    return tuple(sites), tuple(prods)

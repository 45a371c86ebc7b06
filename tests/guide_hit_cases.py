"""Seeded texts for the guide-hit search with what each of them must produce: no code of krisp_amd/.

A set is a protospacer length G, a motif pair and a number of guides; case(set, M) is its text for the distance M -- three
tiles of 16 384 window starts and a begun fourth -- its guides and its PLANTS, each a window written into the random text
together with the rows it must (or must not) produce under omit-soft off and on; short_texts(set, M) are texts of 0 .. G + 20
bytes with theirs; dense(G, period) is a text of period 1 or 2 in which every valid window is a hit and whose counts are
known in closed form.  reference() is guide_hits_reference.ref_hits on a case, computed once and shared.

The guides are random and written into the text, so a one-letter alphabet cannot make every window a hit."""
import functools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_hits_reference as ref                                          # noqa: E402

TILE = 16384                        # window starts of a workgroup's tile
THREAD = 64                         # ... of a thread
N_TEXT = 3 * TILE + 1100
GS = (12, 20, 28, 40)
MS = (0, 1, 2, 3)
MOTIFS = {"none": ("", ""), "tttv": ("TTTV", ""), "h": ("", "H"), "long": ("NNNNTTTV", "HNNNNNNN")}
# a text that matches the motif and whose reverse complement does not (a '-' neighbour matches only after complementing),
# and one that misses it in one letter
INSTANCE = {"": "", "TTTV": "TTTC", "H": "C", "NNNNTTTV": "CAGGTTTC", "HNNNNNNN": "CAGTCAGT"}
NON_INSTANCE = {"": "", "TTTV": "TTTT", "H": "G", "NNNNTTTV": "CAGGTTTT", "HNNNNNNN": "GAGTCAGT"}
NGUIDES = {12: 40, 20: 8, 28: 1, 40: 8}
SETS = {f"g{G}_{m}": dict(G=G, motifs=m, nguides=NGUIDES[G]) for G in GS for m in MOTIFS}
MAX_COMPARISONS = 10 ** 8           # of one reference call
PAD = 9                             # bytes beside a planted window that belong to the plant (a motif has 8 at most)


def pieces(G, M):
    """the seed pieces of the table: piece j = columns [off[j], off[j + 1])"""
    return [j * G // (M + 1) for j in range(M + 2)]


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


def guides(name):
    """the set's protospacers.  1: one random text.  8 and 40: random texts -- of the 40, 36 share their first G / 2 columns,
    a whole seed piece for M >= 1 --, one palindrome, and a last text that repeats the one before it"""
    s = SETS[name]
    G, n = s["G"], s["nguides"]
    rng = np.random.default_rng(zlib.crc32(("guides " + name).encode()))
    if n == 1:
        return [_rand(rng, G)]
    shared = n - 4 if n >= 40 else 0
    head = _rand(rng, G // 2)
    out = []
    while len(out) < n - 3:
        t = head + _rand(rng, G - G // 2) if len(out) < shared else _rand(rng, G)
        if t not in out and t != ref.rc(t):
            out.append(t)
    half = _rand(rng, G // 2)
    out.append(half + ref.rc(half))                  # n - 3: a palindrome
    out.append(_rand(rng, G))                        # n - 2 and n - 1: equal texts
    out.append(out[-1])
    return out


def palindrome_index(name):
    n = SETS[name]["nguides"]
    return n - 3 if n > 1 else None


def equal_index(name):
    n = SETS[name]["nguides"]
    return n - 2 if n > 1 else None


class _Text:
    """a text under construction: random letters, and the intervals the plants own"""

    def __init__(self, rng, n, background=None):
        self.t = bytearray((_rand(rng, n) if background is None else background).encode("ascii"))
        self.owned = []

    def free(self, lo, hi):
        return all(hi <= a or b <= lo for a, b in self.owned)

    def own(self, lo, hi):
        lo, hi = max(lo, 0), min(hi, len(self.t))
        assert self.free(lo, hi), (lo, hi)
        self.owned.append((lo, hi))

    def put(self, at, s):
        """the part of s that lies inside the text"""
        for i, ch in enumerate(s):
            if 0 <= at + i < len(self.t):
                self.t[at + i] = ord(ch)


def _motif_index(pos, strand, G, a, b, side, j):
    """the text index of letter j of the 5' (side 0) or 3' (side 1) motif of the window at pos"""
    if side == 0:
        return pos + G + a - 1 - j if strand else pos - a + j
    return pos - 1 - j if strand else pos + G + j


def plant(T, kind, guides_, pos, strand, gi, pam5, pam3, cols=(), letter=None, motifs=("hit", "hit"), damage=None, lower=False,
          also=()):
    """writes guide gi with substitutions at the guide columns `cols` as a window at pos on `strand`, and the motifs'
    neighbours beside it.  letter: the substituted letter (default: another base).  motifs: per side "hit" (an instance),
    "miss" (a text that misses the motif) or None (the random text stays: the bit is not pinned).  damage: (side, j, byte)
    overwrites motif letter j; the byte "lower" writes the instance's own letter in lower case.  lower: the window in lower
    case.  also: further guides with the same text.  -> the plant: kind, rows [(pos, strand, guide, mismatches, columns)],
    pam = (without omit, under omit) or None, present = (without omit, under omit)"""
    g = guides_[gi]
    G, a, b = len(g), len(pam5), len(pam3)
    n = len(T.t)
    T.own(pos - PAD, pos + G + PAD)
    window = list(g if strand == 0 else ref.rc(g))
    for c in cols:
        w = c if strand == 0 else G - 1 - c
        window[w] = _other(window[w]) if letter is None else letter
    text = "".join(window)
    T.put(pos, text.lower() if lower else text)
    bits = [[1, 1], [1, 1]]                         # [side][omit]
    pinned = True
    for side, (motif, how) in enumerate(zip((pam5, pam3), motifs)):
        if not motif:
            continue
        if how is None:
            pinned = False
            continue
        m = INSTANCE[motif] if how == "hit" else NON_INSTANCE[motif]
        inside = True
        for j, ch in enumerate(m):
            i = _motif_index(pos, strand, G, a, b, side, j)
            inside = inside and 0 <= i < n
            T.put(i, ref.rc(ch) if strand else ch)
        if how != "hit" or not inside:
            bits[side] = [0, 0]
    if damage is not None:
        side, j, byte = damage
        motif = (pam5, pam3)[side]
        i = _motif_index(pos, strand, G, a, b, side, j)
        if byte == "lower":
            T.put(i, chr(T.t[i]).lower())
            bits[side][1] = 0                       # bad under omit, the same letter without
        else:
            T.put(i, byte)
            bits[side] = [0, 0]
        assert motif and 0 <= i < n
    pam = tuple(bits[0][o] | (bits[1][o] << 1) for o in (0, 1)) if pinned else None
    mask = sum(1 << c for c in cols)
    rows = [(pos, strand, x, len(cols), mask) for x in (gi,) + tuple(also)]
    return dict(kind=kind, rows=rows, pam=pam, present=(True, not lower))


def _absent(p):
    p["present"] = (False, False)
    return p


@functools.lru_cache(maxsize=None)
def case(name, M):
    """-> dict(text, guides, G, M, pam5, pam3, plants)"""
    s = SETS[name]
    G, gs = s["G"], guides(name)
    pam5, pam3 = MOTIFS[s["motifs"]]
    a, b = len(pam5), len(pam3)
    rot = list(SETS).index(name) * len(MS) + M
    rng = np.random.default_rng(zlib.crc32(f"case {name} {M}".encode()))
    T = _Text(rng, N_TEXT)
    off = pieces(G, M)
    plain = [i for i in range(len(gs)) if i not in (palindrome_index(name), equal_index(name), len(gs) - 1 if len(gs) > 1 else -1)]
    turn = [rot]

    def gi():
        turn[0] += 1
        return plain[turn[0] % len(plain)]

    def P(kind, pos, strand, **kw):
        plants.append(plant(T, kind, gs, pos, strand, kw.pop("guide", None) if "guide" in kw else gi(), pam5, pam3, **kw))
        return plants[-1]

    plants = []
    # ---- positions: the tile edges (each of -1, 0, +1 and both strands over the cases), a thread edge, 0, the last window
    for e in (1, 2, 3):
        d = (e + rot) % 3 - 1
        P(f"edge{e}{d:+d}", e * TILE + d, (rot // 3 + e) % 2)
    P("thread+", THREAD * 37, 0)
    P("thread-", THREAD * 101, 1)
    P("first", 0, rot % 2)
    P("last", N_TEXT - G, 1 - rot % 2)
    # ---- the background: two separators, a run of N, a stretch of lower case
    for at, s_ in ((9001, "\n"), (33333, "\n"), (21000, "N" * 11)):
        T.own(at, at + len(s_))
        T.put(at, s_)
    T.own(40000, 40400)
    T.put(40000, bytes(T.t[40000:40400]).decode("ascii").lower())
    slots = iter(range(300, N_TEXT - 200, 1152))

    def slot():
        while True:
            p = next(slots)
            if T.free(p - PAD, p + G + PAD):
                return p

    st = [rot]

    def strand():
        st[0] += 1
        return st[0] % 2

    # ---- mismatches and the column mask
    spread = [off[j] + (off[j + 1] - off[j]) // 2 for j in range(M + 1)]
    P("subs_first_piece", slot(), strand(), cols=tuple(range(M)))
    P("subs_last_piece", slot(), strand(), cols=tuple(range(G - M, G)))
    P("subs_one_a_piece", slot(), strand(), cols=tuple(c for j, c in enumerate(spread) if j != rot % (M + 1)))
    _absent(P("over_one_a_piece", slot(), strand(), cols=tuple(spread)))
    _absent(P("over_first_columns", slot(), strand(), cols=tuple(range(M + 1))))
    if M >= 1:
        for sd in (0, 1):
            P(f"column_0_{'+-'[sd]}", slot(), sd, cols=(0,))
            P(f"column_last_{'+-'[sd]}", slot(), sd, cols=(G - 1,))
    if M >= 2:
        P("both_ends", slot(), strand(), cols=(0, G - 1))
    # ---- letters
    p = P("iupac_in_window", slot(), strand(), cols=(G // 2,), letter="R")
    if M == 0:
        _absent(p)
    P("lower_case_window", slot(), strand(), lower=True)
    # ---- motifs
    for side, motif in enumerate((pam5, pam3)):
        if not motif:
            continue
        j = len(motif) - 1
        for sd in (0, 1):
            P(f"motif{side}_miss_{'+-'[sd]}", slot(), sd, motifs=("miss", "hit") if side == 0 else ("hit", "miss"))
            P(f"motif{side}_hit_{'+-'[sd]}", slot(), sd)
        P(f"motif{side}_separator", slot(), strand(), damage=(side, j, "\n"))
        P(f"motif{side}_N", slot(), strand(), damage=(side, j, "N"))
        P(f"motif{side}_lower", slot(), strand(), damage=(side, j, "lower"))
        P(f"motif{side}_iupac", slot(), strand(), damage=(side, j, "R"))
    # ---- the table
    if len(gs) > 1:
        pi, ei = palindrome_index(name), equal_index(name)
        p = P("palindrome", slot(), 0, guide=pi)
        # the same window is the '-' hit: its motifs are the reverse complement's, which the plant did not write
        plants.append(dict(kind="palindrome-", rows=[(p["rows"][0][0], 1, pi, 0, 0)], pam=None if (a or b) else (3, 3), present=(True, True)))
        P("equal_texts", slot(), strand(), guide=ei, also=(ei + 1,))
    return dict(text=bytes(T.t), guides=gs, G=G, M=M, pam5=pam5, pam3=pam3, plants=plants)


@functools.lru_cache(maxsize=None)
def short_texts(name, M):
    """texts of 0 .. G + 20 bytes -> list of (text, plants): the empty text, one byte, G - 1 bytes, the guide alone on either
    strand (position 0 is the last window), a window at a position below a (below b on '-': the motif is cut by the text's
    start), and M substitutions inside G + 20 bytes"""
    s = SETS[name]
    G, gs = s["G"], guides(name)
    pam5, pam3 = MOTIFS[s["motifs"]]
    a, b = len(pam5), len(pam3)
    rng = np.random.default_rng(zlib.crc32(f"short {name} {M}".encode()))
    out = [(b"", []), (b"A", []), (gs[0][:G - 1].encode("ascii"), [])]
    for sd in (0, 1):
        T = _Text(rng, G)
        out.append((T, [plant(T, f"alone{'+-'[sd]}", gs, 0, sd, 0, pam5, pam3)]))
        # one byte short of the motif before the window
        before = (b if sd else a)
        pos = max(before - 1, 0)
        T = _Text(rng, pos + G + (a if sd else b))
        out.append((T, [plant(T, f"below{'+-'[sd]}", gs, pos, sd, 0, pam5, pam3)]))
        T = _Text(rng, G + 20)
        out.append((T, [plant(T, f"subs{'+-'[sd]}", gs, 10, sd, 0, pam5, pam3, cols=tuple(range(0, 2 * M, 2)))]))
    return [(bytes(t.t) if isinstance(t, _Text) else t, pl) for t, pl in out]


def dense(G, period):
    """a text of period 1 (A...) or 2 (ACAC...) and its one guide: a run on '+' that ends 50 bytes before the first tile
    edge, N over the whole second tile, the run's reverse complement from 64 bytes into the third tile to 200 bytes into the
    fourth.  Every valid window of a run is a hit at the run's phase; no other window is within 3 of the guide.
    -> (text, guide, hits on '+', hits on '-')"""
    unit = "A" if period == 1 else "AC"
    guide = (unit * G)[:G]
    r1, r2 = TILE - 50, TILE + 200 - 64
    text = (unit * r1)[:r1] + "N" * (TILE + 50 + 64) + (ref.rc(unit) * r2)[:r2]
    assert len(text) == 3 * TILE + 200 and G % 2 == 0 and r1 % 2 == 0
    count = (lambda r: r - G + 1) if period == 1 else (lambda r: (r - G) // 2 + 1)
    return text.encode("ascii"), guide, count(r1), count(r2)


@functools.lru_cache(maxsize=None)
def reference(name, M, omit, need_pam=False):
    """the reference's hits of case(name, M): computed once, shared, never written to"""
    c = case(name, M)
    hits = ref.ref_hits(c["text"], omit, c["guides"], M, c["pam5"], c["pam3"], need_pam)
    hits.setflags(write=False)
    return hits


def rows_of(hits):
    """(pos, strand, guide) -> (mismatches, columns, pam)"""
    return {(int(h["pos"]), int(h["strand"]), int(h["guide"])): (int(h["mismatches"]), int(h["columns"]), int(h["pam"])) for h in hits}


def check_plants(plants, hits, omit):
    """every plant's rows are in the list (or are not), with the mismatches, the mask and -- where pinned -- the motif bits"""
    got = rows_of(hits)
    for p in plants:
        for pos, strand, guide, mm, mask in p["rows"]:
            row = got.get((pos, strand, guide))
            if not p["present"][omit]:
                assert row is None, (p["kind"], pos, strand, guide, row)
                continue
            assert row is not None, (p["kind"], pos, strand, guide)
            assert row[:2] == (mm, mask), (p["kind"], pos, strand, guide, row, mm, mask)
            if p["pam"] is not None:
                assert row[2] == p["pam"][omit], (p["kind"], pos, strand, guide, row, p["pam"])

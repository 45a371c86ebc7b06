"""Random cases for the two product passes (kr_products_*: the flank pass; kr_primers_*: the primer pass), from one seeded
generator in the style of test_gpu_scan_properties.cases: length set x M x alphabet x separator layout x table size, texts
of up to a little over three tiles of TILE window starts.  Nothing of krisp_amd/ is imported: the texts, tables and plants
are made with numpy alone.  test_product_scan_cases.py asserts, with the brute-force references alone, what the default
seeds cover; test_gpu_product_scan_properties.py holds the kernels to the references on the same cases.

cases(seed) -> {"flank": case, "primer": case}; a case is a dict:
  text, text2     uint8 arrays: the genome as uploaded (records joined by '\\n'), and a stretch of it that starts off the tile
                  grid with three more separators (a second genome for the same tables)
  left, right     lists of bytes: the table's texts (flank pass: all left texts of Le letters, all right texts of Re)
  Le, Re          the flank pass's lengths (None in a primer case)
  pairs           [(left, right)]
  M, omit, max_product
  plants          [dict(pos, length, strand, pair, ml, mr, expect)]: a product written into the text -- the left text's site
                  with ml substitutions, the right text's with mr; expect: the definition must list it (both within M, no
                  separator inside, not longer than max_product, the sites not overlapping, not lower case under omit)
  tails           (primer) [dict(pos, entry, kind, col)]: a text longer than the shortest written at pos with a bad byte of
                  `kind` ('\\n', 'N', 'lower', 'end') in column col of its tail: no site of that entry there
M = seed % 4, the length set = seed // 4 (cycling); SEEDS covers every length set with every M once."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_scan_properties import ALPHABETS, THREAD, TILE              # noqa: E402

_COMP = bytes.maketrans(b"ACGTRYKMBVDH", b"TGCAYRMKVBHD")
PLAIN = np.frombuffer(b"ACGT", dtype=np.uint8)
IUPAC = b"RYKMSWBDHV"
PRIM_MIN, PRIM_MAX = 10, 60         # kr_primers_table's lengths


def max_flank():
    """the longest flank text kr_products_table takes: its texts have the locate context's L and R letters, and
    kr_set_params_locate takes up to KR_WIDE_MAX_FLANK of either (include/krisp_hip.h)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"#define\s+KR_WIDE_MAX_FLANK\s+(\d+)", open(os.path.join(root, "include", "krisp_hip.h")).read()).group(1))


FLANK_SETS = [(10, 10), (10, 30), (30, 10), (16, 17), (max_flank(), max_flank())]
# the lengths the texts of a side cycle through; the last set gets two left texts more that no pair names: one of 10
# letters (the shortest of the table) and one of 60
PRIMER_SETS = [[10], [60], [10, 60], [10, 11, 37, 60], [10, 11, 12, 13, 14], [20, 25, 22]]
UNPAIRED = len(PRIMER_SETS) - 1
SEEDS = 4 * len(PRIMER_SETS)
BIG_TABLE_SEED = 7                  # 3000 texts a side (a tiny text: the reference compares every text at every position)
REF_BYTES = 1.0e8                   # text bytes x entries x letters a reference call may compare (about 0.3 s)


def rc(b):
    return bytes(b)[::-1].translate(_COMP)


def pieces(n, M):
    return [j * n // (M + 1) for j in range(M + 2)]


def sub_columns(n, head, M, c, mode, rng):
    """c distinct columns of a text of n letters whose seeded columns are the first `head` (flank pass: head = n), cut
    into M + 1 pieces: mode 0 all in the first piece, 1 all in the last, 2 one per piece from the first on (c = M: every
    piece but one), 3 all in the tail, 4 all but one in the head and one in the tail; what does not fit: anywhere"""
    off = pieces(head, M)
    if mode == 0 and off[1] >= c:
        return rng.choice(off[1], size=c, replace=False).tolist()
    if mode == 1 and head - off[M] >= c:
        return (off[M] + rng.choice(head - off[M], size=c, replace=False)).tolist()
    if mode == 2 and c <= M + 1:
        return [int(rng.integers(off[p], off[p + 1])) for p in range(c)]
    if mode == 3 and n - head >= c:
        return (head + rng.choice(n - head, size=c, replace=False)).tolist()
    if mode == 4 and n > head and 1 <= c <= head + 1:
        return rng.choice(head, size=c - 1, replace=False).tolist() + [int(rng.integers(head, n))]
    return rng.choice(n, size=c, replace=False).tolist()


def _random_text(rng, n):
    return PLAIN[rng.integers(0, 4, size=n)].tobytes()


def _case(seed, kind):
    primer = kind == "primer"
    rng = np.random.default_rng(7000 + 2 * seed + primer)
    M = seed % 4
    gi = seed // 4
    omit = bool((seed // 2 + gi) % 2)
    alphabet = np.frombuffer(ALPHABETS[(seed + gi) % len(ALPHABETS)], dtype=np.uint8)
    subs = b"ACGT" + (IUPAC if b"R" in alphabet.tobytes() else b"")
    si = gi % (len(PRIMER_SETS) if primer else len(FLANK_SETS))
    cyc = PRIMER_SETS[si] if primer else None
    Le, Re = (None, None) if primer else FLANK_SETS[si]
    maxlen = max(cyc + ([PRIM_MAX] if si == UNPAIRED else [])) if primer else max(Le, Re)
    meanlen = sum(cyc) / len(cyc) if primer else (Le + Re) / 2
    tiny = seed % 16 == 7
    if tiny:
        n = int(rng.integers(0, 2 * maxlen + 40))
    elif seed % 8 == 3:
        n = int(rng.integers(TILE - 40, 2 * TILE))
    else:
        n = int(rng.integers(2 * TILE + maxlen, 3 * TILE + 3000))
    text = alphabet[rng.integers(0, len(alphabet), size=n)].copy()
    # ---- separators: at random places, in runs, on thread edges, on the first and the last byte, on tile edges; one seed
    # in eight: a record every 16 bytes or so
    if n:
        text[rng.integers(0, n, size=n // 5000 + int(rng.integers(0, 3)))] = 10
        if seed % 8 == 5:
            text[rng.integers(0, n, size=n // 12)] = 10
        if n > 1000:
            for p in rng.integers(0, n, size=2):
                text[p:p + int(rng.integers(2, 6))] = 10
            for e in rng.integers(1, n // THREAD, size=4):
                text[int(e) * THREAD - int(rng.integers(0, 2))] = 10
        if rng.random() < 0.3:
            text[0] = 10
        if rng.random() < 0.3:
            text[n - 1] = 10
    clean = []
    for e in range(TILE, n, TILE):
        if rng.random() < 0.6:
            text[e - int(rng.integers(0, 2))] = 10
            if rng.random() < 0.5:
                text[e - 1:e + 1] = 10
        else:
            clean.append(e)

    # ---- the table
    size = (3000 if seed == BIG_TABLE_SEED else 300) if tiny else [1, 4, 30][(seed + gi) % 3]
    if not tiny:
        size = max(1, min(size, int(REF_BYTES / (4 * max(n, 1) * meanlen))))
    if primer:
        llen = [cyc[i % len(cyc)] for i in range(size)]
        rlen = [cyc[(j + 1) % len(cyc)] for j in range(size)]
    else:
        llen, rlen = [Le] * size, [Re] * size
    left = [_random_text(rng, m) for m in llen]
    right = [_random_text(rng, m) for m in rlen]
    if size >= 4:
        if primer or Le == Re:
            right[1] = left[1]                                  # a left text that is a right text too
        if len(left[2]) % 2 == 0:
            half = left[2][:len(left[2]) // 2]
            left[2] = half + rc(half)                           # its own reverse complement
        right[3] = left[3][-1:] + right[3][1:]                  # (left 3 and right 3 can overlap by one)
    npaired = size
    if primer and si == UNPAIRED:
        left += [_random_text(rng, PRIM_MIN), _random_text(rng, PRIM_MAX)]
    smin = min(len(t) for t in left + right) if primer else None
    shared = []
    if primer and size > 4:
        # 1 to 40 texts that share their seeded columns and differ in the tail only
        longer = [i for i in range(4, size) if len(left[i]) > smin][:(1, 3, 40)[seed % 3]]
        for i in longer:
            left[i] = left[longer[0]][:smin] + left[i][smin:]
        shared = longer
    pairs = [(i, i) for i in range(npaired)]
    if size >= 4:
        pairs += [(0, 1), (0, 2), (1, 0), (2, 0)]
    maxpair = max(len(left[i]) + len(right[j]) for i, j in pairs)
    max_product = maxpair + ([3, 8, 15] if primer and si == UNPAIRED else [3, 40, 250])[(seed + gi) % 3]
    crowded = seed % 4 in (1, 2) and not tiny and maxlen <= PRIM_MAX and not (primer and si == UNPAIRED)
    if crowded:
        max_product = maxpair + 250                             # (a site of the row of copies has several partners)
    nl = len(left)

    # ---- the plants
    taken = []                                                  # (lo, hi) the text is spoken for

    def free(lo, hi):
        return -1 <= lo and hi <= n + 1 and all(hi <= a or lo >= b for a, b in taken)

    def mutate(x, c, mode):
        head = smin if primer else len(x)
        t = bytearray(x)
        for col in sub_columns(len(x), head, M, min(c, len(x)), mode, rng):
            t[col] = rng.choice([b for b in subs if b != x[col]])
        return bytes(t)

    plants, tails = [], []
    count = [0]

    def product(p_of, pair=None, strand=None, gap_kind=None):
        """a product of `pair` written at p_of(n1, gap, n2) (None: nowhere)"""
        i = count[0]
        count[0] += 1
        pi = i % min(len(pairs), 12) if pair is None else pair
        strand = (i // 3) & 1 if strand is None else strand
        a, b = left[pairs[pi][0]], right[pairs[pi][1]]
        room = max_product - len(a) - len(b)
        gap_kind = i % 7 if gap_kind is None else gap_kind
        if gap_kind >= 5 and size >= 4:                         # pair 3: overlapping by one, abutting
            pi = 3
            a, b = left[3], right[3]
            room = max_product - len(a) - len(b)
        gap = [0, 1, room // 2, room, room + 1, -1 if size >= 4 else 0, 0][gap_kind]
        ml, mr = (0, 0) if i < 6 else (i % (M + 2), (i // 2) % (M + 2))
        mode_l, mode_r = int(rng.integers(0, 5 if primer else 3)), int(rng.integers(0, 5 if primer else 3))
        x1, x2, c1, c2 = (a, b, ml, mr) if strand == 0 else (rc(b), rc(a), mr, ml)
        length = len(x1) + gap + len(x2)
        p = p_of(len(x1), gap, len(x2))
        if p is None or not free(p - 1, p + length + 1):
            return
        taken.append((p - 1, p + length + 1))
        if rng.random() < 0.75:
            g = text[p:p + length]
            bad = g == 10
            g[bad] = PLAIN[rng.integers(0, 4, size=int(bad.sum()))]
        y1, y2 = mutate(x1, c1, mode_l), mutate(x2, c2, mode_r)
        text[p:p + len(y1)] = np.frombuffer(y1, dtype=np.uint8)
        q = p + len(x1) + gap
        if gap < 0 and y2[0] != y1[-1]:                         # (the shared byte is the first site's: one more mismatch)
            mr, ml = (mr + 1, ml) if strand == 0 else (mr, ml + 1)
            text[q + 1:q + len(y2)] = np.frombuffer(y2[1:], dtype=np.uint8)
        else:
            text[q:q + len(y2)] = np.frombuffer(y2, dtype=np.uint8)
        lowered = False
        if (alphabet >= 97).any() and rng.random() < 0.2:
            text[p:p + length] |= 0x20
            text[p:p + length][text[p:p + length] == 42] = 10   # ('\n' | 0x20)
            lowered = True
        span = text[p:p + length]
        expect = (ml <= M and mr <= M and gap >= 0 and length <= max_product and not (span == 10).any()
                  and not (lowered and omit) and not (span == ord("n")).any() and not (span == ord("N")).any())
        plants.append(dict(pos=p, length=length, strand=strand, pair=pi, ml=ml, mr=mr, expect=bool(expect)))

    def crowd():
        """more than a join block of sites: 40 copies of pair 0's product in a row, one byte apart (every opening site
        has several closing sites in reach), after 216 single sites and before 100 more"""
        unit = np.frombuffer((left[0] + b"A" + right[0] + b"C") * 40, dtype=np.uint8)
        at = n // 2
        while not free(at - 1, at + len(unit) + 1):
            at += THREAD
            if at + len(unit) > n:
                return
        taken.append((at - 1, at + len(unit) + 1))
        text[at:at + len(unit)] = unit
        every = left + right
        for lo, hi, k in ((0, at, 216), (at + len(unit), n, 100)):
            for p in rng.integers(lo, max(lo + 1, hi - maxlen), size=3 * k).tolist():
                x = every[int(rng.integers(0, len(every)))]
                x = np.frombuffer(rc(x) if rng.random() < 0.5 else x, dtype=np.uint8)
                if k and free(p - 1, p + len(x) + 1):
                    taken.append((p - 1, p + len(x) + 1))
                    text[p:p + len(x)] = x
                    k -= 1

    if n >= maxpair:
        for q, e in enumerate(clean):
            # the opening site across the edge / the closing site across it / the sites in different tiles
            how = (seed + gi + 2 * (e // TILE)) % 5
            r = int(rng.integers(1, 10))
            product([lambda n1, g, n2: e - min(r, n1 - 1), lambda n1, g, n2: e - n1 - g - min(r, n2 - 1),
                     lambda n1, g, n2: e - n1][min(how >> 1, 2)], strand=how & 1, gap_kind=int(rng.integers(0, 4)),
                    pair=int(rng.integers(0, min(len(pairs), 12))))
        if text[0] != 10:
            product(lambda n1, g, n2: 0, gap_kind=seed % 3)
        if text[n - 1] != 10 and not (primer and seed % 2 == 0):
            product(lambda n1, g, n2: n - n1 - g - n2, gap_kind=seed % 3)
        for t in rng.integers(0, max(1, n // THREAD), size=4 if n > 1000 else 0).tolist():
            product(lambda n1, g, n2: t * THREAD + (THREAD - 1) * (t & 1))
        if crowded:
            crowd()
        for _ in range(0 if tiny else 28):
            p = int(rng.integers(0, max(1, n - maxpair)))
            product(lambda n1, g, n2: p)
    if primer and si == UNPAIRED and n > 200:
        # ---- the texts no pair names, each before a closing site: sites, no products; the walk from the site of the
        # long one ends at its first step (60 + smin > max_product)
        for i in (nl - 2, nl - 1):
            x = np.frombuffer(left[i] + right[0], dtype=np.uint8)
            p = int(rng.integers(0, n - len(x)))
            if free(p - 1, p + len(x) + 1):
                taken.append((p - 1, p + len(x) + 1))
                text[p:p + len(x)] = x
    texts = left + right
    if primer and max(len(t) for t in texts) > smin:
        # ---- a long text whose tail holds a bad byte
        long_left = [i for i in range(len(texts)) if len(texts[i]) > smin]
        kinds = ["\n", "N", "lower", "end"] if seed % 2 == 0 else ["\n", "N", "lower"]
        for t, what in enumerate(kinds * (1 if tiny else 3)):
            i = long_left[t % len(long_left)]
            e = 2 * i + int(rng.integers(0, 2))
            x = texts[i] if e % 2 == 0 else rc(texts[i])
            col = int(rng.integers(smin, len(x)))
            p = n - col if what == "end" else int(rng.integers(0, max(1, n - len(x))))
            if p < 0 or not free(p - 1, min(p + len(x), n) + 1) or (what == "end" and text[n - 1] == 10):
                continue
            taken.append((p - 1, min(p + len(x), n) + 1))
            y = np.frombuffer(x, dtype=np.uint8)[:n - p]
            text[p:p + len(y)] = y
            if what == "lower":
                text[p + col] |= 0x20
            elif what != "end":
                text[p + col] = ord(what)
            tails.append(dict(pos=p, entry=e, kind=what, col=col))
    # a second genome for the same tables: a stretch of the first that starts off the tile grid, three separators more
    a = int(rng.integers(1, 200)) if n > 400 else 0
    text2 = text[a:a + min(n - a, TILE + 5000)].copy()
    if len(text2):
        text2[rng.integers(0, len(text2), size=3)] = 10
    return dict(kind=kind, seed=seed, set=si, alphabet=(seed + gi) % len(ALPHABETS), text=text, text2=text2, left=left, right=right, Le=Le, Re=Re, pairs=pairs, M=M, omit=omit,
                max_product=max_product, plants=plants, tails=tails, shared=shared, smin=smin, maxlen=maxlen, clean=clean)


def cases(seed):
    return {"flank": _case(seed, "flank"), "primer": _case(seed, "primer")}


# ----------------------------------------------------------------------------
# the definition of a case (the references take the two passes' tables in their own forms)
# ----------------------------------------------------------------------------
def u8(rows, width):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width)


def entry_lengths(c):
    return [len(t) for t in c["left"] for _ in (0, 1)] + [len(t) for t in c["right"] for _ in (0, 1)]


def reference(c, text, M=None, max_product=None):
    """-> (ref_sites, ref_products) of a case's tables over `text`, as lists of tuples"""
    M = c["M"] if M is None else M
    max_product = c["max_product"] if max_product is None else max_product
    if c["kind"] == "flank":
        from products_reference import ref_products, ref_sites
        lf, rt = u8(c["left"], c["Le"]), u8(c["right"], c["Re"])
        sites = ref_sites(text, c["omit"], lf, rt, c["Le"], c["Re"], M)
        prods = ref_products(text, c["omit"], lf, rt, c["Le"], c["Re"], c["pairs"], M, max_product)
    else:
        from primers_reference import ref_products, ref_sites
        texts = c["left"] + c["right"]
        sites = ref_sites(text, c["omit"], texts, len(c["left"]), M)
        prods = ref_products(text, c["omit"], texts, len(c["left"]), c["pairs"], M, max_product, sites=sites)
    return [tuple(r) for r in sites.tolist()], [tuple(r) for r in prods.tolist()]

"""The locate scan (csrc/k_locate.inc) and the near-match scan (csrc/k_near.inc) against their definitions
(scan_reference.py), through _native.Engine, the complete hit list of every text:
  * random cases from one seeded generator, cases(seed): geometry x alphabet x separator layout x table, texts of up to a
    little over three tiles of LOC_T * LOC_S = 16384 window starts (test_scan_reference.py's census asserts, on the CPU, what
    the generator's default seeds cover: tile edges, thread edges, the last window, both strands, every M, ...);
  * a window planted at every start across a tile edge and at the text's end, with the substitutions in the first piece, the
    last, or one in every piece but one, and a bad byte before / at the start / at the end / after it;
  * dense output: every window a hit on both strands, 1 to 40 entries under a seed, tiles with unequal counts and one without;
  * text lengths around k, 16, 64 and the tile; empty and absent tables; equal target rows;
  * multi-record FASTA files whose record boundaries lie in the second and third tile, through KF.locate_regions and
    KF.near_matches, against py_locate / py_near.
KR_SCAN_SEEDS sets the number of random cases (default: SEEDS, every geometry of GEOMETRIES with every M once)."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scan_reference import COMP, ref_locate, ref_near, ref_seps, ref_windows       # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 16384            # LOC_T * LOC_S window starts
THREAD = 64             # LOC_S

ALPHABETS = [b"ACGT", b"ACGTACGTACGTN", b"ACGTACGTacgt", b"ACGTACGTACGTacgtNn", b"ACGTACGTACGTRYKMSWBDHVrykmswbdhv", b"AC", b"A"]
# (L, D, R) by seed // 4 (None: k = M + 1, pieces of one byte); M = seed % 4.  Three wide ones (a flank > 64, k > 256)
GEOMETRIES = [(10, 4, 10), (25, 1, 2), (0, 3, 9), (9, 3, 0), (6, 0, 5), None, (15, 2, 15), (70, 120, 70), (3, 1, 12),
              (100, 60, 130), (2, 28, 2), (80, 101, 80)]
ONE_BYTE_PIECES = [(1, 0, 0), (1, 0, 1), (1, 1, 1), (2, 1, 1)]
SEEDS = 4 * len(GEOMETRIES)
PLAIN = np.frombuffer(b"ACGT", dtype=np.uint8)


def rc(w):
    return COMP[np.asarray(w, dtype=np.uint8)[::-1]]


def pieces(k, M):
    """the columns [off[j], off[j + 1]) of the M + 1 pieces (kr_near_table)"""
    return [j * k // (M + 1) for j in range(M + 2)]


def substitute(w, cols, rng):
    t = w.copy()
    for c in cols:
        t[c] = rng.choice([b for b in b"ACGT" if b != w[c]])
    return t


def columns(k, L, D, j, M, mode, rng):
    """j distinct columns of a k-mer: mode 0 all in the first piece, 1 all in the last, 2 one per piece from the first on
    (j = M: every piece but the last -- the pigeonhole's tight case), 3 the diagnostic columns first, 4 anywhere"""
    off = pieces(k, M)
    if mode == 0 and off[1] >= j:
        return rng.choice(off[1], size=j, replace=False).tolist()
    if mode == 1 and k - off[M] >= j:
        return (off[M] + rng.choice(k - off[M], size=j, replace=False)).tolist()
    if mode == 2 and j <= M + 1:
        return [int(rng.integers(off[p], off[p + 1])) for p in range(j)]
    if mode == 3 and D:
        diag = rng.permutation(np.arange(L, L + D)).tolist()
        rest = rng.permutation([c for c in range(k) if not L <= c < L + D]).tolist()
        return (diag + rest)[:j]
    return rng.choice(k, size=j, replace=False).tolist()


def cases(seed):
    """one random case -> dict(L, D, R, k, omit, M, text, text2, flanks, targets, plants, palindrome); plants = the target
    rows made from a window of the text: (pos, strand, target, distance), distance <= M + 1; palindrome = where a window
    equal to its reverse complement was written, or None"""
    rng = np.random.default_rng(1000 + seed)
    M = seed % 4
    gi = seed // 4
    if gi < len(GEOMETRIES):
        geo = GEOMETRIES[gi] or ONE_BYTE_PIECES[M]
    else:
        geo = (int(rng.integers(0, 17)), int(rng.integers(0, 9)), int(rng.integers(0, 17)))
        if geo[0] + geo[2] == 0:
            geo = (1, geo[1], 0)
        if sum(geo) <= M:
            geo = ONE_BYTE_PIECES[M]
    L, D, R = geo
    k = L + D + R
    omit = bool(rng.integers(0, 2))
    alphabet = np.frombuffer(ALPHABETS[(seed + gi) % len(ALPHABETS)], dtype=np.uint8)
    if seed % 16 == 7:
        n = int(rng.integers(0, 2 * k + 40))                    # (0, < k, around k)
    elif seed % 8 == 3:
        n = int(rng.integers(TILE - 40, 2 * TILE))
    else:
        n = int(rng.integers(2 * TILE + k, 3 * TILE + 3000))
    text = alphabet[rng.integers(0, len(alphabet), size=n)].copy()
    nw = max(0, n - k + 1)
    # separators: at random places, in runs, on thread edges, on the first and the last byte, on tile edges
    if n:
        text[rng.integers(0, n, size=n // 5000 + int(rng.integers(0, 3)))] = 10
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
        if rng.random() < 0.4:
            text[e - int(rng.integers(0, 2))] = 10
            if rng.random() < 0.5:
                text[e - 1:e + 1] = 10
        else:
            clean.append(e)
    # the places table rows are cut from: across the tile edges left clean, a thread's last and first start, the text's
    # last and first window, anywhere; three in four of them are cleared of bad bytes
    sources = []
    if nw:
        for e in clean:
            sources += [int(e - r) for r in rng.integers(1, max(k, 2), size=3) if k > 1]
        sources += [int(t) * THREAD + 63 for t in rng.integers(0, max(1, nw // THREAD), size=3)]
        sources += [int(t) * THREAD for t in rng.integers(0, max(1, nw // THREAD), size=3)]
        sources += [nw - 1, 0] + rng.integers(0, nw, size=6).tolist()
        sources = [p for p in sources if 0 <= p < nw]
    for p in sources:
        if rng.random() < 0.75 and not (p == nw - 1 and text[n - 1] == 10) and not (p == 0 and text[0] == 10):
            w = text[p:p + k]
            bad = (w == 10) | (w == ord("N")) | (w == ord("n"))
            if omit:
                bad |= w >= 97
            w[bad] = PLAIN[rng.integers(0, 4, size=int(bad.sum()))]
    # a palindrome, a run of one base and a run of its complement
    palindrome = None
    if nw > 8 * k + 64:
        half = PLAIN[rng.integers(0, 4, size=k // 2)]
        pal = np.concatenate([half, np.frombuffer(b"W", dtype=np.uint8)[:k % 2], rc(half)])
        palindrome = int(rng.integers(0, nw))
        text[palindrome:palindrome + k] = pal
        sources.append(palindrome)
        for b in b"AT":
            p = int(rng.integers(0, nw - 8))
            text[p:p + k + 7] = b
            sources.append(p + int(rng.integers(0, 8)))
    up = np.where((text >= 97) & (text <= 122), text - 32, text).astype(np.uint8)

    def window(p):
        """the window at p as a table row: itself, or its reverse complement (strand 1 finds that)"""
        strand = int(rng.integers(0, 2))
        w = up[p:p + k].copy()
        return (rc(w) if strand else w), strand

    # ---- the flank table: the sources' flanks, rows that share their left flank, unrelated rows; 1 to a few hundred
    cols = [c for c in range(k) if c < L or c >= L + D]
    frows = []
    for p in sources:
        w, _ = window(p)
        frows.append(w[cols])
        if L and R and rng.random() < 0.5:
            other = w[cols].copy()
            other[L:] = PLAIN[rng.integers(0, 4, size=R)]
            frows.append(other)
    want_rows = int(rng.choice([1, 4, 30, 300]))
    while len(frows) < want_rows:
        frows.append(PLAIN[rng.integers(0, 4, size=L + R)])
    if want_rows == 1:
        frows = frows[:1]
    farr = np.array(frows, dtype=np.uint8).reshape(len(frows), L + R)
    _, first = np.unique(farr, axis=0, return_index=True)
    flanks = farr[np.sort(first)]

    # ---- the targets: the sources with 0 .. M + 1 substitutions, unrelated rows; few where the amplicon is wide (the
    # reference's time) or so short that every window is near every target (the number of rows)
    short = k <= 2 * M + 2
    budget = 4 if short else (8 if k > 64 else int(rng.choice([1, 5, 40, 120])))
    most = 4 if short else (8 if k > 64 else max(budget, len(sources)))
    trows, plants = [], []
    for i, p in enumerate(sources[::-1] if k > 64 and seed % 2 else sources):
        if len(trows) >= (1 if budget == 1 else most):
            break
        w, strand = window(p)
        j = min(i % (M + 2), k)                                 # 0 .. M + 1 substitutions
        t = substitute(w, columns(k, L, D, j, M, int(rng.integers(0, 5)), rng), rng) if j else w
        trows.append(t)
        plants.append((p, strand, t.tobytes(), j))
    while len(trows) < budget:
        trows.append(PLAIN[rng.integers(0, 4, size=k)])
    tarr = np.array(trows, dtype=np.uint8).reshape(len(trows), k)
    _, first = np.unique(tarr, axis=0, return_index=True)
    targets = tarr[np.sort(first)]
    index = {t.tobytes(): i for i, t in enumerate(targets)}
    plants = [(p, s, index[t], j) for p, s, t, j in plants]
    # a second genome for the same tables: a stretch of the first that starts off the tile grid, three separators more
    a = int(rng.integers(1, 200)) if n > 400 else 0
    text2 = text[a:a + min(n - a, TILE + 5000)].copy()
    if len(text2):
        text2[rng.integers(0, len(text2), size=3)] = 10
    return dict(L=L, D=D, R=R, k=k, omit=omit, M=M, text=text, text2=text2, flanks=flanks, targets=targets, plants=plants,
                palindrome=palindrome)


# ----------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------
def engine(L, D, R, omit, max_bases):
    from krisp_amd import _native
    eng = _native.Engine()
    eng.set_params_locate(L, D, R, omit, max_bases=max(int(max_bases), 1))
    return eng


def check_locate(eng, text, L, D, R, omit, flanks, want=None):
    """the scan of the genome under id 0 against ref_locate: the hits in order, their windows, a second scan the same bytes
    -> the expected hits"""
    k = L + D + R
    want = ref_locate(text, L, D, R, omit, flanks) if want is None else want
    got = eng.locate(0)
    assert len(got) == len(want), (len(got), len(want))
    for f in ("pos", "strand", "group"):
        assert np.array_equal(got[f].astype(np.int64), want[f]), f
    assert np.array_equal(eng.locate_windows(k), ref_windows(text, want, k))
    assert eng.locate(0).tobytes() == got.tobytes()
    return want


def check_near(eng, text, L, D, R, omit, targets, M, want=None):
    """the scan of the genome under id 0 against ref_near: the hits sorted by (pos, strand, target), pos non-decreasing as
    returned, their windows, a second scan the same bytes -> the expected hits"""
    k = L + D + R
    want = ref_near(text, L, D, R, omit, targets, M) if want is None else want
    got = eng.near(0)
    rows = eng.near_windows(k)
    assert len(got) == len(want), (len(got), len(want))
    assert not got["pad"].any()
    assert (np.diff(got["pos"].astype(np.int64)) >= 0).all()
    order = np.lexsort((got["target"], got["strand"], got["pos"]))
    for f in ("pos", "strand", "target", "mismatches", "flank_mismatches"):
        assert np.array_equal(got[f][order].astype(np.int64), want[f]), f
    assert np.array_equal(rows[order], ref_windows(text, want, k))
    assert eng.near(0).tobytes() == got.tobytes()
    return want


def check_seps(eng, text):
    assert np.array_equal(eng.locate_seps(0), ref_seps(text))


N_SEEDS = int(os.environ.get("KR_SCAN_SEEDS", str(SEEDS)))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_cases_equal_the_definition(seed):
    c = cases(seed)
    L, D, R, omit, M = c["L"], c["D"], c["R"], c["omit"], c["M"]
    want = {}
    with engine(L, D, R, omit, max(len(c["text"]), len(c["text2"]))) as eng:
        eng.locate_table(c["flanks"])
        eng.near_table(c["targets"], M)
        # (one genome resident at a time, under one id: the first, another, the first again)
        for name in ("text", "text2", "text"):
            text = c[name]
            eng.upload(0, text)
            wl, wn = want.get(name, (None, None))
            wl = check_locate(eng, text, L, D, R, omit, c["flanks"], wl)
            wn = check_near(eng, text, L, D, R, omit, c["targets"], M, wn)
            want[name] = (wl, wn)
            check_seps(eng, text)
    print("seed", seed, (L, D, R), "M", M, "n", len(c["text"]), "rows", len(c["flanks"]), len(c["targets"]), "hits",
          [(len(a), len(b)) for a, b in want.values()])


# ----------------------------------------------------------------------------
# every offset across a tile edge and at the text's end
# ----------------------------------------------------------------------------
EDGE_GEOMETRY = (7, 3, 5)          # L != R, k = 15
EDGE_TARGET = np.frombuffer(b"GATTCCAGCATGTCA", dtype=np.uint8)
BAD_AT = {"before": -1, "first": 0, "last": sum(EDGE_GEOMETRY) - 1, "after": sum(EDGE_GEOMETRY)}


def edge_texts(kind, M):
    """(text, pos, strand, omit, reported): a window planted at every start from TILE - k - 1 to TILE + 1 and from nw - 3
    to nw - 1 of a text of two tiles and a tail, on each strand; kind "locate": the window has the table's flanks; "near": it
    lies M columns from the target, all in the first piece / all in the last / one in every piece but the last.  Each of
    those alone, then with a bad byte ('\\n', N, lower case with and without omit-soft) before the window, on its first
    byte, on its last, after it"""
    L, D, R = EDGE_GEOMETRY
    k = L + D + R
    rng = np.random.default_rng(77 + M + (10 if kind == "locate" else 0))
    n = 2 * TILE + 300 + M
    nw = n - k + 1
    base = PLAIN[rng.integers(0, 4, size=n)]
    out = []
    for si, p in enumerate(list(range(TILE - k - 1, TILE + 2)) + [nw - 3, nw - 2, nw - 1]):
        for strand in (0, 1):
            variants = [(mode, None, None, False) for mode in (0, 1, 2)]
            for vi, (where, byte) in enumerate(itertools.product(BAD_AT, ("\n", "N", "lower"))):
                for omit in ((False, True) if byte == "lower" else (False,)):
                    variants.append(((si + vi) % 3, where, byte, omit))
            for mode, where, byte, omit in variants:
                w = EDGE_TARGET if kind == "locate" else substitute(EDGE_TARGET, columns(k, L, D, M, M, mode, rng), rng)
                text = base.copy()
                text[p:p + k] = rc(w) if strand else w
                reported = True
                if where is not None:
                    q = p + BAD_AT[where]
                    if q >= n:
                        continue
                    text[q] = text[q] | 0x20 if byte == "lower" else ord(byte)
                    reported = where in ("before", "after") or (byte == "lower" and not omit)
                out.append((text, p, strand, omit, reported))
    return out


@pytest.mark.parametrize("kind,M", [("locate", 0), ("near", 0), ("near", 1), ("near", 2), ("near", 3)])
def test_a_window_at_every_start_across_a_tile_edge_and_at_the_end(kind, M):
    L, D, R = EDGE_GEOMETRY
    k = L + D + R
    texts = edge_texts(kind, M)
    flanks = np.concatenate([EDGE_TARGET[:L], EDGE_TARGET[L + D:]]).reshape(1, L + R)
    target = EDGE_TARGET.reshape(1, k)
    assert len(texts) >= (k + 6) * 2 * 18
    seen = 0
    engines = {omit: engine(L, D, R, omit, len(texts[0][0])) for omit in (False, True)}
    try:
        for eng in engines.values():
            eng.locate_table(flanks)
            eng.near_table(target, M)
        for text, p, strand, omit, reported in texts:
            eng = engines[omit]
            eng.upload(0, text)
            if kind == "locate":
                want = check_locate(eng, text, L, D, R, omit, flanks)
                there = ((want["pos"] == p) & (want["strand"] == strand)).any()
            else:
                want = check_near(eng, text, L, D, R, omit, target, M)
                there = ((want["pos"] == p) & (want["strand"] == strand) & (want["mismatches"] == M)).any()
            assert bool(there) == reported, (p, strand, omit)       # (the definition agrees with how the text was made)
            seen += reported
    finally:
        for eng in engines.values():
            eng.close()
    assert seen >= (k + 6) * 2 * 12


# ----------------------------------------------------------------------------
# dense output
# ----------------------------------------------------------------------------
DENSE_GEOMETRY = (5, 4, 3)         # L != R; k = 12: a window of ATAT... is its own reverse complement, 3 divides k
# (ACC, not ACG: the windows of one phase lie 8 columns or more from every target made of another phase or strand, whatever
# fills the 4 diagnostic columns -- ACGACG... is 4 columns from the reverse complement of CGACGA...)
DENSE_UNITS = {"A": b"A", "AT": b"AT", "ACC": b"ACC"}


def dense_text(unit):
    """three tiles and a tail of the unit repeated, with separators that give the tiles different numbers of valid windows
    and the second tile none -> (text, the number of valid windows by the lengths between separators)"""
    k = sum(DENSE_GEOMETRY)
    n = 3 * TILE + 777
    text = np.frombuffer((unit * (n // len(unit) + 1))[:n], dtype=np.uint8).copy()
    rng = np.random.default_rng(len(unit))
    text[np.arange(TILE, 2 * TILE + k, k)] = 10              # every window that starts in the second tile holds one
    text[rng.integers(0, TILE - k, size=5)] = 10
    text[rng.integers(2 * TILE + k, 3 * TILE, size=40)] = 10
    text[[3 * TILE - 1, 3 * TILE, n - 1]] = 10
    bounds = np.concatenate([[-1], np.flatnonzero(text == 10), [n]])
    return text, int(np.maximum(np.diff(bounds) - 1 - k + 1, 0).sum())


def dense_tables(unit, F):
    """-> (flank pairs, targets, the fillings' distances): the text's window at each phase and its reverse complement; as
    targets, each with the F fillings of its diagnostic columns that lie nearest to its own (F targets that differ only
    there: with M > 0 they stand under one seed)"""
    L, D, R = DENSE_GEOMETRY
    k = L + D + R
    rows, targets, dist = [], [], None
    for ph in range(len(unit)):
        w = np.frombuffer((unit * (k + 3))[ph:ph + k], dtype=np.uint8)
        for x in (w, rc(w)):
            rows.append(x)
            own = x[L:L + D].tolist()
            fills = sorted(itertools.product(b"ACGT", repeat=D), key=lambda f: (sum(a != b for a, b in zip(f, own)), f))[:F]
            dist = [sum(a != b for a, b in zip(f, own)) for f in fills]
            for f in fills:
                t = x.copy()
                t[L:L + D] = f
                targets.append(t)
    rows = np.unique(np.array(rows, dtype=np.uint8), axis=0)
    targets = np.unique(np.array(targets, dtype=np.uint8), axis=0)
    return np.delete(rows, np.s_[L:L + D], axis=1), targets, dist


@pytest.mark.parametrize("F,M", [(1, 0), (1, 2), (2, 1), (2, 3), (40, 1)])
@pytest.mark.parametrize("name", list(DENSE_UNITS))
def test_dense_output_every_window_hits_on_both_strands(name, F, M):
    L, D, R = DENSE_GEOMETRY
    k = L + D + R
    unit = DENSE_UNITS[name]
    text, nvalid = dense_text(unit)
    flanks, targets, dist = dense_tables(unit, F)
    within = sum(d <= M for d in dist)
    # a window of phase p is one of the rows on '+' and one on '-' (AT: the same row, its own reverse complement), and lies
    # within M of `within` of the F targets made from each: 2 x within rows per valid window
    assert len(flanks) == (2, 2, 6)[len(unit) - 1] and len(targets) == F * len(flanks)
    assert nvalid > 2 * TILE - 3000 and within >= 1 and dist[0] == 0
    with engine(L, D, R, False, len(text)) as eng:
        eng.upload(0, text)
        eng.locate_table(flanks)
        loc = check_locate(eng, text, L, D, R, False, flanks)
        assert len(loc) == 2 * nvalid
        eng.near_table(targets, M)
        near = check_near(eng, text, L, D, R, False, targets, M)
        assert len(near) == 2 * nvalid * within
        check_seps(eng, text)
    tiles = np.bincount(near["pos"] // TILE, minlength=4)
    assert tiles[1] == 0 and len(set(tiles.tolist())) == 4
    print(name, "F", F, "M", M, "valid", nvalid, "locate", len(loc), "near", len(near), "per tile", tiles.tolist())


# ----------------------------------------------------------------------------
# lengths
# ----------------------------------------------------------------------------
LEN_GEOMETRY = (5, 2, 4)           # k = 11
LENGTHS = [0, 1, 11 - 1, 11, 11 + 1, 15, 16, 17, 63, 64, 65, TILE + 11 - 2, TILE + 11 - 1, TILE + 11, 2 * TILE + 11 - 1]


@pytest.mark.parametrize("trailing", [False, True], ids=["plain", "trailing_separator"])
@pytest.mark.parametrize("n", LENGTHS)
def test_text_lengths_around_k_the_load_widths_and_the_tile(n, trailing):
    """a text of n bytes in which every window is a hit of the one row"""
    L, D, R = LEN_GEOMETRY
    k = L + D + R
    text = np.full(n, ord("A"), dtype=np.uint8)
    nsep = 1 if trailing and n else 0
    if nsep:
        text[n - 1] = 10
    row = np.full((1, k), ord("A"), dtype=np.uint8)
    windows = max(0, n - nsep - k + 1)
    with engine(L, D, R, False, n) as eng:
        eng.upload(0, text)
        eng.locate_table(row[:, :L + R])
        assert len(check_locate(eng, text, L, D, R, False, row[:, :L + R])) == windows
        for M in range(4):
            eng.near_table(row, M)
            assert len(check_near(eng, text, L, D, R, False, row, M)) == windows
        check_seps(eng, text)
        assert len(eng.locate_seps(0)) == nsep


# ----------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------
def plain_text(n, seed):
    return PLAIN[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def test_an_empty_table_and_a_table_that_does_not_occur_give_no_hits():
    L, D, R = 6, 2, 6
    k = L + D + R
    text = plain_text(2 * TILE + 100, 3)
    absent = np.frombuffer(b"R" * k + b"S" * k, dtype=np.uint8).reshape(2, k)
    with engine(L, D, R, False, len(text)) as eng:
        eng.upload(0, text)
        for flanks, targets in ((np.empty((0, L + R), dtype=np.uint8), np.empty((0, k), dtype=np.uint8)),
                                (np.delete(absent, np.s_[L:L + D], axis=1), absent)):
            eng.locate_table(flanks)
            assert len(check_locate(eng, text, L, D, R, False, flanks)) == 0
            assert eng.locate_windows(k).shape == (0, k)
            for M in range(4):
                eng.near_table(targets, M)
                assert len(check_near(eng, text, L, D, R, False, targets, M)) == 0
                assert eng.near_windows(k).shape == (0, k)


@pytest.mark.parametrize("M", range(4))
def test_equal_target_rows_are_two_targets(M):
    """kr_near_table keeps equal rows as separate targets (include/krisp_hip.h): a window near one is a row of each"""
    L, D, R = 6, 2, 6
    k = L + D + R
    text = plain_text(TILE + 500, 4)
    w = text[TILE - 5:TILE - 5 + k].copy()
    targets = np.array([w, rc(text[40:40 + k]), w, substitute(w, [L], np.random.default_rng(0))], dtype=np.uint8)
    with engine(L, D, R, False, len(text)) as eng:
        eng.upload(0, text)
        eng.near_table(targets, M)
        want = check_near(eng, text, L, D, R, False, targets, M)
    at = want[(want["pos"] == TILE - 5) & (want["strand"] == 0)]
    assert at["target"].tolist() == ([0, 2] if M == 0 else [0, 2, 3])
    assert at["mismatches"].tolist() == ([0, 0] if M == 0 else [0, 0, 1])


def test_a_repeated_flank_pair_is_refused():
    from krisp_amd import _native
    flanks = np.frombuffer(b"ACGTAC" b"GGGTTT" b"ACGTAC", dtype=np.uint8).reshape(3, 6)
    with engine(3, 1, 3, False, 100) as eng:
        with pytest.raises(_native.KrispHipError, match="group 2 repeats the flanks of group 0") as e:
            eng.locate_table(flanks)
        assert e.value.code == -2      # KR_ERR_PARAM


# ----------------------------------------------------------------------------
# file level: positions to (record, record_index, start)
# ----------------------------------------------------------------------------
def write_fasta_that_moves_record_indices(path, seq, k, rng, crlf, last):
    """seq cut into records of unequal lengths (one shorter than k; boundaries in the second and third tile), with headers
    without sequence and sequence lines of white space only between and inside them; last: the file ends without a
    newline ("no_newline"), with a header ("header"), or plainly (None)"""
    nl = b"\r\n" if crlf else b"\n"
    cuts = sorted(set(rng.integers(1, len(seq), size=9).tolist() + [TILE + 700, TILE + 700 + k - 2, 2 * TILE - 3, 2 * TILE + 900]))
    out = []
    for i, (a, b) in enumerate(zip([0] + cuts, cuts + [len(seq)])):
        out.append(b">rec%d some words" % i + nl)
        rec = seq[a:b]
        for j in range(0, len(rec), 70):
            out.append(rec[j:j + 70] + nl)
            if rng.random() < 0.02:
                out.append(b" \t " + nl)
        if i % 3 == 1:
            out.append(b">empty%d" % i + nl)
            if i % 2:
                out.append(b"   " + nl)
    if last == "header":
        out.append(b">trailing" + nl)
    data = b"".join(out)
    if last == "no_newline":
        data = data[:-len(nl)]
    with open(path, "wb") as f:
        f.write(data)


@pytest.mark.parametrize("seed", range(2))
def test_files_whose_record_boundaries_lie_in_the_second_and_third_tile(seed, tmp_path):
    from krisp_amd import codec, synth
    from krisp_amd import krisp_fasta as KF
    from test_locate_host import py_locate
    from test_near_host import near_rows, py_near
    L, R, k = 10, 5, 17
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
    assert len(groups) >= 3
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    locs = KF.locate_regions(groups, ing, out, L, R, k)
    pairs = [(g[0].left.replace("U", "T"), g[0].right.replace("U", "T")) for g in groups]
    got = list(zip(locs["region"].tolist(), locs["file"], locs["record"], locs["record_index"].tolist(),
                   locs["start"].tolist(), locs["end"].tolist(), locs["strand"], locs["sequence"]))
    assert got == py_locate(paths, pairs, Le, De, Re, False)
    assert len({r[3] for r in got}) >= 6                        # (rows in many records: those past the first tile too)
    targets = KF.near_targets(groups, [KF.simplename(f) for f in ing])
    near = near_rows(KF.near_matches(groups, ing, out, L, R, k, mismatches=1))
    assert near == py_near(paths, targets, Le, De, Re, 1, False)
    assert len(near) >= 10

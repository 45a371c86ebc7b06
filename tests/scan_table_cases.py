"""Tables of thousands of rows for the seed passes and the locate pass, over a short text: no code of krisp_amd/.

Every other case of the suite has a few dozen targets, guides or groups, so its table has the least size, 1024 slots, and is
nearly empty: no probe chain of any length, none that wraps from the last slot to slot 0, no slot with entries of many
targets, no list index beyond a few hundred, a membership bitmap with a bit here and there.  The regime here is the
table's; the text is a tile and a tail.

near_case(name): thousands of targets of K = 20 letters for a distance M (NEAR_CASES) -- windows of the text on either
strand with 0 .. M + 1 substitutions, groups of rows that share their first half (a whole seed piece for M >= 1, and their
reverse complements' last), runs of equal rows (M = 0: the rows under one key), unrelated rows.  locate_case(): N_GROUPS
distinct flank pairs, most of them cut from the text.  The generators' seeds were searched, on the CPU, until the tables have what
test_scan_table_cases.py's census asserts: a long probe chain, a chain that wraps, a crowded slot, a shared bitmap bit.

The references: locate_by_dictionary (a plain dictionary of the text's windows) and near_by_packed_words (every position
with every target on both strands, the windows packed two bits a letter into 64-bit words and the differing columns
counted: no seeds, hashes or tables), over a text of A, C, G, T and separators.  near_by_packed_words holds itself to
guide_hit_cases.MAX_COMPARISONS; test_scan_table_cases.py ties both to scan_reference on a sub-sample."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guide_hit_cases import MAX_COMPARISONS                                # noqa: E402
from scan_reference import LOC_HIT, NEAR_HIT                               # noqa: E402

TILE = 16384
GEOMETRY = (7, 6, 7)                # L, D, R: K = 20, the flanks have 14 letters
K = sum(GEOMETRY)
N_TEXT = TILE + 300                 # two tiles: a window across the edge, and KR_SCAN_GRID = 1 makes a workgroup take both
N_TARGETS = 2800                    # (N_TEXT - K + 1) * N_TARGETS * 2 < MAX_COMPARISONS
N_GROUPS = 3000
# name -> (M, targets, the generator's seed: searched, see above).  With M = 3 a seed piece has five letters: a table of
# thousands of targets holds nearly every one of the 4 x 1024 keys there are -- every window of the text probes it --, and
# the set of them all has no chain that wraps in its 8192 slots, nor have its parts in 8192 or 4096 slots (too few keys
# whose place is among the last slots).  "m3_few" is a table of 2048 slots, a sixth of the keys, that has one
NEAR_CASES = {"m0": (0, N_TARGETS, 19), "m1": (1, N_TARGETS, 26), "m2": (2, N_TARGETS, 1694), "m3": (3, N_TARGETS, 1),
              "m3_few": (3, 130, 25)}
LOCATE_SEED = 13
# a key whose probe chain passes the last slot (the census says which keys do): name -> (entry, piece), and the group.  The
# entry's text stands at PLANT_POS with a substitution in every other piece, the group's flanks around six other letters
# at PLANT_POS: hits that are found through the wrapping chain or not at all
NEAR_WRAPS = {"m0": (860, 0), "m1": (1862, 1), "m2": (2870, 2), "m3_few": (114, 3)}
LOCATE_WRAPS = 1006
PLANT_POS = 500
PLAIN = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.full(256, 255, dtype=np.uint8)
_CODE[PLAIN] = np.arange(4, dtype=np.uint8)


def rc(w):
    """the reverse complement of a row of A, C, G, T"""
    return PLAIN[3 - _CODE[np.asarray(w, dtype=np.uint8)[::-1]]]


def _text(rng):
    text = PLAIN[rng.integers(0, 4, size=N_TEXT)].copy()
    text[rng.integers(0, N_TEXT, size=3)] = 10
    text[TILE + 100] = 10
    return text


def _starts(text):
    """the starts of the windows of K letters without a separator"""
    bad = np.concatenate([[0], np.cumsum(text == 10)])
    return np.flatnonzero(bad[K:] == bad[:-K])


def _window(text, starts, rng):
    p = int(starts[rng.integers(0, len(starts))])
    w = text[p:p + K].copy()
    return rc(w) if rng.integers(0, 2) else w


def _substitute(w, cols, rng):
    t = w.copy()
    for c in cols:
        t[c] = PLAIN[(int(_CODE[w[c]]) + int(rng.integers(1, 4))) % 4]
    return t


def near_case(name, seed=None):
    """-> dict(text, targets [n, K], M)"""
    M, n, own = NEAR_CASES[name]
    rng = np.random.default_rng(own if seed is None else seed)
    text = _text(rng)
    starts = _starts(text)
    many = n >= 2000
    cut = 1800 if many else 60
    rows = []
    for i in range(cut):                                        # windows with 0 .. M + 1 substitutions
        j = i % (M + 2)
        rows.append(_substitute(_window(text, starts, rng), rng.choice(K, size=j, replace=False).tolist(), rng))
    for _ in range(12 if many else 4):                          # twelve rows that share their first half: the window itself,
        base = _window(text, starts, rng)                       # one a substitution away in the other half, ten with another
        rows.append(base)
        rows.append(_substitute(base, [K // 2 + int(rng.integers(0, K - K // 2))], rng))
        for _ in range(10):
            other = base.copy()
            other[K // 2:] = PLAIN[rng.integers(0, 4, size=K - K // 2)]
            rows.append(other)
    for _ in range(3 if many else 1):                           # runs of ten equal rows
        rows += [_window(text, starts, rng)] * 10
    rows += [rows[int(i)] for i in rng.integers(0, cut, size=30 if many else 10)]      # rows equal to an earlier one
    while len(rows) < n:
        rows.append(PLAIN[rng.integers(0, 4, size=K)])
    targets = np.array(rows, dtype=np.uint8)[rng.permutation(n)]
    if name in NEAR_WRAPS:
        e, piece = NEAR_WRAPS[name]
        w = rc(targets[e // 2]) if e & 1 else targets[e // 2].copy()
        off = [j * K // (M + 1) for j in range(M + 2)]
        w = _substitute(w, [(off[j] + off[j + 1]) // 2 for j in range(M + 1) if j != piece], rng)
        text[PLANT_POS:PLANT_POS + K] = w
    return dict(text=text, targets=targets, M=M)


def locate_case(seed=None):
    """-> dict(text, flanks [N_GROUPS, L + R], distinct)"""
    L, D, R = GEOMETRY
    rng = np.random.default_rng(LOCATE_SEED if seed is None else seed)
    text = _text(rng)
    starts = _starts(text)
    seen, rows = set(), []
    while len(rows) < N_GROUPS:
        w = _window(text, starts, rng) if len(rows) < 2500 else PLAIN[rng.integers(0, 4, size=K)]
        f = np.concatenate([w[:L], w[L + D:]])
        if f.tobytes() not in seen:
            seen.add(f.tobytes())
            rows.append(f)
    flanks = np.array(rows, dtype=np.uint8)[rng.permutation(N_GROUPS)]
    text[PLANT_POS:PLANT_POS + K] = np.concatenate([flanks[LOCATE_WRAPS][:L], PLAIN[rng.integers(0, 4, size=D)], flanks[LOCATE_WRAPS][L:]])
    return dict(text=text, flanks=flanks)


# ----------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------
def locate_by_dictionary(text, L, D, R, flanks):
    """scan_reference.ref_locate's list for a text of A, C, G, T and separators: the flanks of every window, as written and
    as the other strand reads it, looked up in a dictionary of the groups"""
    k = L + D + R
    text = np.asarray(text, dtype=np.uint8)
    group = {bytes(f): g for g, f in enumerate(np.asarray(flanks, dtype=np.uint8).reshape(-1, L + R))}
    assert set(np.unique(text).tolist()) <= set(b"ACGT\n")
    out = []
    for p in range(len(text) - k + 1):
        w = text[p:p + k]
        if (w == 10).any():
            continue
        for strand, x in ((0, w), (1, rc(w))):
            g = group.get(x[:L].tobytes() + x[L + D:].tobytes())
            if g is not None:
                out.append((p, strand, g))
    return np.array(out, dtype=LOC_HIT) if out else np.empty(0, dtype=LOC_HIT)


_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.uint8)


def _popcount(x):
    return (_POP16[x & np.uint64(0xFFFF)].astype(np.int64) + _POP16[(x >> np.uint64(16)) & np.uint64(0xFFFF)]
            + _POP16[(x >> np.uint64(32)) & np.uint64(0xFFFF)] + _POP16[x >> np.uint64(48)])


def _pack(codes):
    """rows of 2-bit codes [n, k] -> uint64 [n]: column c in bits 2 c, 2 c + 1"""
    out = np.zeros(codes.shape[0], dtype=np.uint64)
    for c in range(codes.shape[1]):
        out |= codes[:, c].astype(np.uint64) << np.uint64(2 * c)
    return out


def near_by_packed_words(text, L, D, R, targets, M, chunk=64):
    """-> (scan_reference.ref_near's list, the hits' differing columns as a mask in the target's orientation: bit c = target
    column c) for a text of A, C, G, T and separators and targets of A, C, G, T, k <= 32"""
    k = L + D + R
    text = np.asarray(text, dtype=np.uint8)
    targets = np.asarray(targets, dtype=np.uint8).reshape(-1, k)
    assert k <= 32 and set(np.unique(text).tolist()) <= set(b"ACGT\n") and set(np.unique(targets).tolist()) <= set(b"ACGT")
    nw = len(text) - k + 1
    if nw <= 0 or not len(targets):
        return np.empty(0, dtype=NEAR_HIT), np.empty(0, dtype=np.uint64)
    assert nw * len(targets) * 2 <= MAX_COMPARISONS
    from numpy.lib.stride_tricks import sliding_window_view
    codes = sliding_window_view(_CODE[text], k)
    valid = ~(codes == 255).any(axis=1)
    safe = np.where(codes == 255, 0, codes)
    # the window as written, and as the other strand reads it: column c = the complement of column k - 1 - c
    words = (_pack(safe), _pack(3 - safe[:, ::-1]))
    tw = _pack(_CODE[targets])
    low = np.uint64(int("01" * k, 2))
    flank = np.uint64(sum(1 << (2 * c) for c in range(k) if c < L or c >= L + D))
    # every window with every target: first the 16 columns of the words' lower halves (their count bounds the distance from
    # below), then all columns of the pairs that are within M there
    half = min(k, 16)
    low32 = np.uint32(int("01" * half, 2))
    wlo = tuple((w & np.uint64(0xFFFFFFFF)).astype(np.uint32) for w in words)
    tlo = (tw & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    parts, masks = [], []
    for lo in range(0, len(targets), chunk):
        for strand in (0, 1):
            x = wlo[strand][None, :] ^ tlo[lo:lo + chunk, None]
            x |= x >> np.uint32(1)
            x &= low32                                          # bit 2 c: column c differs
            ti, pos = np.nonzero(_POP16[x & np.uint32(0xFFFF)] + _POP16[x >> np.uint32(16)] <= M)
            ok = valid[pos]
            ti, pos = ti[ok], pos[ok]
            xx = words[strand][pos] ^ tw[lo + ti]
            m = (xx | (xx >> np.uint64(1))) & low
            d = _popcount(m)
            ok = d <= M
            ti, pos, m, d = ti[ok], pos[ok], m[ok], d[ok]
            part = np.empty(len(pos), dtype=NEAR_HIT)
            part["pos"], part["strand"], part["target"], part["mismatches"] = pos, strand, ti + lo, d
            part["flank_mismatches"] = _popcount(m & flank)
            parts.append(part)
            masks.append(m)
    out, m = np.concatenate(parts), np.concatenate(masks)
    order = np.lexsort((out["target"], out["strand"], out["pos"]))
    columns = np.zeros(len(m), dtype=np.uint64)
    for c in range(k):
        columns |= ((m >> np.uint64(2 * c)) & np.uint64(1)) << np.uint64(c)
    return out[order], columns[order]

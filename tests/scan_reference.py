"""The locate scan and the near-match scan as definitions, in numpy, over every position of a text: what kr_locate_scan /
kr_near_scan / kr_locate_seps / kr_*_windows (include/krisp_hip.h) must return for the bytes kr_genome_upload was given.
Brute force: no hashes, seeds, tiles or tables, and no code of krisp_amd/.  test_scan_reference.py ties these functions to
the slow file-level definitions (py_locate, py_near); test_gpu_scan_properties.py holds the kernels to them."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

LOC_HIT = np.dtype([("pos", "<i8"), ("strand", "<i8"), ("group", "<i8")])
NEAR_HIT = np.dtype([("pos", "<i8"), ("strand", "<i8"), ("target", "<i8"), ("mismatches", "<i8"), ("flank_mismatches", "<i8")])

# the complement of an upper-case letter: ACGT, R/Y, M/K, B/V, D/H; every other byte is its own
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "CG", "RY", "MK", "BV", "DH"):
    COMP[ord(_a)], COMP[ord(_b)] = ord(_b), ord(_a)


def _text(text):
    return np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)


def _upper(t):
    lower = (t >= ord("a")) & (t <= ord("z"))
    return np.where(lower, t - np.uint8(32), t).astype(np.uint8)


def _strands(text, k, omit):
    """-> (the windows as written [nw, k], their reverse complements [nw, k], which of them are valid [nw]); upper case"""
    t = _text(text)
    lower = (t >= ord("a")) & (t <= ord("z"))
    bad = (t == ord("\n")) | (t == ord("N")) | (t == ord("n"))
    if omit:
        bad |= lower
    up = _upper(t)
    fwd = sliding_window_view(up, k)
    # window p read on the other strand = k bytes of the reversed, complemented text that end where p starts
    rev = sliding_window_view(COMP[up][::-1], k)[::-1]
    valid = ~sliding_window_view(bad, k).any(axis=1)
    return fwd, rev, valid


def ref_seps(text):
    """the positions of '\\n', ascending"""
    return np.flatnonzero(_text(text) == ord("\n")).astype(np.uint64)


def ref_locate(text, L, D, R, omit, flanks):
    """every (pos, strand, group): the valid window at pos, read on the strand, starts with the group's left flank and ends
    with its right one.  Ordered by position, '+' (0) before '-' (1)."""
    k = L + D + R
    flanks = np.asarray(flanks, dtype=np.uint8).reshape(-1, L + R)
    if len(_text(text)) < k or len(flanks) == 0:
        return np.empty(0, dtype=LOC_HIT)
    fwd, rev, valid = _strands(text, k, omit)
    cols = np.concatenate([np.arange(L), np.arange(L + D, k)]).astype(np.int64)
    parts = []
    for g, fl in enumerate(flanks):
        for strand, win in ((0, fwd), (1, rev)):
            # (one column first: the full comparison runs on the windows that pass it)
            cand = np.flatnonzero(valid & (win[:, cols[0]] == fl[0])) if len(cols) else np.flatnonzero(valid)
            pos = cand[(win[cand][:, cols] == fl).all(axis=1)]
            part = np.empty(len(pos), dtype=LOC_HIT)
            part["pos"], part["strand"], part["group"] = pos, strand, g
            parts.append(part)
    out = np.concatenate(parts)
    return out[np.lexsort((out["group"], out["strand"], out["pos"]))]


def ref_near(text, L, D, R, omit, targets, M):
    """every (pos, strand, target, mismatches, flank_mismatches): the valid window at pos, read on the strand, differs from
    the target in mismatches <= M columns (the same number as the window as written from the target's reverse complement),
    flank_mismatches of them in the target's columns c < L or c >= L + D.  Ordered by (pos, strand, target)."""
    k = L + D + R
    targets = np.asarray(targets, dtype=np.uint8).reshape(-1, k)
    if len(_text(text)) < k or len(targets) == 0:
        return np.empty(0, dtype=NEAR_HIT)
    fwd, rev, valid = _strands(text, k, omit)
    flank = np.ones(k, dtype=bool)
    flank[L:L + D] = False
    parts = []
    for ti, t in enumerate(targets):
        for strand, win in ((0, fwd), (1, rev)):
            d = np.count_nonzero(win != t, axis=1)
            pos = np.flatnonzero(valid & (d <= M))
            part = np.empty(len(pos), dtype=NEAR_HIT)
            part["pos"], part["strand"], part["target"], part["mismatches"] = pos, strand, ti, d[pos]
            part["flank_mismatches"] = np.count_nonzero(win[pos][:, flank] != t[flank], axis=1)
            parts.append(part)
    out = np.concatenate(parts)
    return out[np.lexsort((out["target"], out["strand"], out["pos"]))]


def ref_windows(text, hits, k):
    """the rows kr_locate_windows / kr_near_windows return for `hits` (anything with pos and strand fields): the k letters at
    pos in upper case, reverse complemented for strand 1 -> uint8 [len(hits), k]"""
    up = _upper(_text(text))
    pos = np.asarray(hits["pos"]).astype(np.int64)
    rows = up[pos[:, None] + np.arange(k, dtype=np.int64)] if len(pos) else np.empty((0, k), dtype=np.uint8)
    minus = np.asarray(hits["strand"]) == 1
    rows[minus] = COMP[rows[minus][:, ::-1]]
    return rows

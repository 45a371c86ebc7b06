"""The product pass as a definition, in numpy, over every position of a text: what kr_products_scan / kr_products_sites /
kr_products_fetch (include/krisp_hip.h) must return for the bytes kr_genome_upload was given (records joined by '\\n').
Brute force: every position, every flank text, both orientations, Hamming distance by comparison; no seeds, hashes, tiles
or tables, and no code of krisp_amd/.  test_products_host.py pins these functions to hand-made texts, test_gpu_products.py
holds the kernels to them."""
import os
import sys

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scan_reference import COMP, _text, _upper                 # noqa: E402

PRODUCT_END = 5
SITE = np.dtype([("pos", "<i8"), ("entry", "<i8"), ("mismatches", "<i8"), ("end_mismatches", "<i8")])
PRODUCT = np.dtype([("pos", "<i8"), ("length", "<i8"), ("strand", "<i8"), ("pair", "<i8"), ("left_mm", "<i8"),
                    ("right_mm", "<i8"), ("left_end_mm", "<i8"), ("right_end_mm", "<i8")])


def _rows(texts, n):
    return np.asarray(texts, dtype=np.uint8).reshape(-1, n)


def entries(left, right, Le, Re):
    """the entries in the table's numbering: 2 i = left text i, 2 i + 1 = its reverse complement, 2 nl + 2 j = right text
    j, 2 nl + 2 j + 1 = its reverse complement -> list of (text, is_left, reversed)"""
    out = []
    for rows, is_left in ((_rows(left, Le), True), (_rows(right, Re), False)):
        for t in rows:
            out.append((t, is_left, False))
            out.append((COMP[t[::-1]], is_left, True))
    return out


def ref_sites(text, omit, left, right, Le, Re, M):
    """every (pos, entry, mismatches, end_mismatches): the window of the entry's length at pos holds no '\\n', N or n (no
    lower case under omit), and its upper-case letters differ from the entry's text in mismatches <= M columns,
    end_mismatches of them in the min(5, length) columns at the primer's 3' end: the last columns of A and of rc(B) as
    written, the first of B and of rc(A).  Ordered by (pos, entry)."""
    t = _text(text)
    lower = (t >= ord("a")) & (t <= ord("z"))
    bad = (t == ord("\n")) | (t == ord("N")) | (t == ord("n"))
    if omit:
        bad |= lower
    up = _upper(t)
    parts = [np.empty(0, dtype=SITE)]
    for e, (x, is_left, rev) in enumerate(entries(left, right, Le, Re)):
        n = len(x)
        if len(t) < n:
            continue
        win = sliding_window_view(up, n)
        valid = ~sliding_window_view(bad, n).any(axis=1)
        ne = win != x
        d = np.count_nonzero(ne, axis=1)
        pos = np.flatnonzero(valid & (d <= M))
        end = min(PRODUCT_END, n)
        cols = np.arange(n - end, n) if is_left != rev else np.arange(end)
        part = np.empty(len(pos), dtype=SITE)
        part["pos"], part["entry"], part["mismatches"] = pos, e, d[pos]
        part["end_mismatches"] = np.count_nonzero(ne[pos][:, cols], axis=1)
        parts.append(part)
    out = np.concatenate(parts)
    return out[np.lexsort((out["entry"], out["pos"]))]


def ref_products(text, omit, left, right, Le, Re, pairs, M, max_product):
    """every product of every pair (row p of pairs = (left text, right text)): '+' (0) a site of A at s1 and of B at s2,
    '-' (1) a site of rc(B) at s1 and of rc(A) at s2; no '\\n' in [s1, s2 + len); s2 >= s1 + len(first);
    length = s2 + len(second) - s1 <= max_product.  Ordered by (pos, length, strand, pair)."""
    t = _text(text)
    sites = ref_sites(text, omit, left, right, Le, Re, M)
    nl = len(_rows(left, Le))
    nsep = np.concatenate([[0], np.cumsum(t == ord("\n"))])        # separators before position i
    by_entry = {}
    for s in sites:
        by_entry.setdefault(int(s["entry"]), []).append(s)
    out = []
    for p, (i, j) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)):
        A, rcA, B, rcB = 2 * i, 2 * i + 1, 2 * nl + 2 * j, 2 * nl + 2 * j + 1
        for strand, first, second, n1, n2 in ((0, A, B, Le, Re), (1, rcB, rcA, Re, Le)):
            for a in by_entry.get(int(first), []):
                for b in by_entry.get(int(second), []):
                    s1, s2 = int(a["pos"]), int(b["pos"])
                    if s2 < s1 + n1 or s2 + n2 - s1 > max_product:
                        continue
                    if nsep[s2 + n2] != nsep[s1]:
                        continue
                    lf, rt = (a, b) if strand == 0 else (b, a)
                    out.append((s1, s2 + n2 - s1, strand, p, int(lf["mismatches"]), int(rt["mismatches"]),
                                int(lf["end_mismatches"]), int(rt["end_mismatches"])))
    out.sort()
    return np.array(out, dtype=PRODUCT) if out else np.empty(0, dtype=PRODUCT)

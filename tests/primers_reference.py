"""The primer-product pass as a definition, in numpy, over every position of a text: what kr_primers_scan / kr_primers_sites
/ kr_primers_fetch (include/krisp_hip.h) must return for the bytes kr_genome_upload was given (records joined by '\\n').
It is products_reference.py with a length per text in the place of Le and Re.  Brute force: every position, every text,
both orientations, Hamming distance by comparison; no seeds, hashes, tiles or tables, and no code of krisp_amd/.
test_primers_host.py pins these functions to hand-made texts, test_gpu_primers.py holds the kernels to them."""
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


def entries(texts, nleft):
    """the entries in the table's numbering: 2 i = left text i, 2 i + 1 = its reverse complement, 2 nleft + 2 j = right
    text j, 2 nleft + 2 j + 1 = its reverse complement -> list of (text, is_left, reversed)"""
    out = []
    for i, t in enumerate(texts):
        t = np.frombuffer(bytes(t), dtype=np.uint8)
        out.append((t, i < nleft, False))
        out.append((COMP[t[::-1]], i < nleft, True))
    return out


def ref_sites(text, omit, texts, nleft, M):
    """every (pos, entry, mismatches, end_mismatches): the window of the ENTRY'S OWN length at pos holds no '\\n', N or n
    (no lower case under omit), and its upper-case letters differ from the entry's text in mismatches <= M columns,
    end_mismatches of them in the min(5, length) columns at the primer's 3' end: the last columns of A and of rc(B) as
    written, the first of B and of rc(A).  Ordered by (pos, entry)."""
    t = _text(text)
    lower = (t >= ord("a")) & (t <= ord("z"))
    bad = (t == ord("\n")) | (t == ord("N")) | (t == ord("n"))
    if omit:
        bad |= lower
    up = _upper(t)
    parts = [np.empty(0, dtype=SITE)]
    for e, (x, is_left, rev) in enumerate(entries(texts, nleft)):
        n = len(x)
        if len(t) < n:
            continue
        ne = sliding_window_view(up, n) != x
        valid = ~sliding_window_view(bad, n).any(axis=1)
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


def ref_products(text, omit, texts, nleft, pairs, M, max_product, sites=None):
    """every product of every pair (row p of pairs = (left text, right text)): '+' (0) a site of A at s1 and of B at s2,
    '-' (1) a site of rc(B) at s1 and of rc(A) at s2; no '\\n' in [s1, s2 + n2); s2 >= s1 + n1; length = s2 + n2 - s1 <=
    max_product, n1 and n2 the lengths of those two entries.  Ordered by (pos, length, strand, pair).  (sites: ref_sites of
    the same arguments, when the caller has them already.)"""
    t = _text(text)
    if sites is None:
        sites = ref_sites(text, omit, texts, nleft, M)
    lens = [len(bytes(x)) for x in texts]
    nsep = np.concatenate([[0], np.cumsum(t == ord("\n"))])        # separators before position i
    by_entry = {}
    for s in sites:
        by_entry.setdefault(int(s["entry"]), []).append(s)
    out = []
    for p, (i, j) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()):
        A, rcA, B, rcB = 2 * i, 2 * i + 1, 2 * nleft + 2 * j, 2 * nleft + 2 * j + 1
        nA, nB = lens[i], lens[nleft + j]
        for strand, first, second, n1, n2 in ((0, A, B, nA, nB), (1, rcB, rcA, nB, nA)):
            closing = by_entry.get(second, [])
            cpos = np.array([int(b["pos"]) for b in closing], dtype=np.int64)          # (ascending)
            for a in by_entry.get(first, []):
                # (only the closing sites in reach are visited; the conditions below are the definition)
                lo, hi = np.searchsorted(cpos, [int(a["pos"]), int(a["pos"]) + max_product])
                for b in closing[lo:hi]:
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

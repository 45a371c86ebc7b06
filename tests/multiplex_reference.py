"""The multiplex pass as a definition, in plain loops: what kr_multiplex_scan / kr_multiplex_sites / kr_multiplex_fetch /
kr_multiplex_tally (include/krisp_hip.h) must return for the bytes kr_genome_upload was given (records joined
by '\\n').  All the oligos of a panel share a tube: any text may open a product and any text may close one.

There are T texts of 10 .. 60 letters A, C, G, T, written 5'->3'.  Entry 2 t is text t as written: it OPENS a product and
its 3' end lies in its last columns.  Entry 2 t + 1 is its reverse complement: it CLOSES a product and its 3' end lies in
its first columns.  Brute force: every entry against every position, a loop over the entry's columns (numpy only adds up
one column over all positions at a time); the join is two nested loops.  No seeds, hashes, tiles or tables, no code of
krisp_amd/ and none of the other references: test_multiplex_cases.py pins this file to primers_reference.py."""
import numpy as np

PRODUCT_END = 5
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(b):
    return bytes(b)[::-1].translate(_COMP)


def entries(texts):
    """-> [(text of the entry as it reads on the forward strand, the columns of its 3' end)]"""
    out = []
    for t in texts:
        t = bytes(t)
        n = len(t)
        out.append((t, range(n - PRODUCT_END, n)))
        out.append((rc(t), range(PRODUCT_END)))
    return out


def ref_sites(text, omit, texts, M):
    """every (pos, entry, mismatches, end_mismatches): the window of the ENTRY'S OWN length at pos holds no '\\n', N or n
    (no lower case under omit), and its upper-case letters differ from the entry's text in mismatches <= M columns,
    end_mismatches of them in the 5 columns at the 3' end.  Ordered by (pos, entry)."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    lower = (t >= ord("a")) & (t <= ord("z"))
    bad = (t == ord("\n")) | (t == ord("N")) | (t == ord("n"))
    if omit:
        bad = bad | lower
    up = np.where(lower, t - 32, t).astype(np.uint8)
    out = []
    for e, (x, end) in enumerate(entries(texts)):
        n = len(x)
        nw = len(t) - n + 1
        if nw <= 0:
            continue
        mm = np.zeros(nw, dtype=np.int64)
        em = np.zeros(nw, dtype=np.int64)
        nbad = np.zeros(nw, dtype=np.int64)
        for q in range(n):                              # one column of the entry over every window
            differs = up[q:q + nw] != x[q]
            mm += differs
            if q in end:
                em += differs
            nbad += bad[q:q + nw]
        for pos in np.flatnonzero((nbad == 0) & (mm <= M)).tolist():
            out.append((pos, e, int(mm[pos]), int(em[pos])))
    out.sort()
    return out


def ref_products(text, omit, texts, M, max_product, sites=None):
    """every product (forward a, reverse b): an opening site of entry 2 a at s1, a closing site of entry 2 b + 1 at s2, no
    '\\n' in [s1, s2 + n_b), s2 >= s1 + n_a, s2 + n_b - s1 <= max_product; a == b is allowed -> (pos = s1, length = s2 + n_b
    - s1, fwd = a, rev = b, fwd_mm, rev_mm, fwd_end_mm, rev_end_mm), ordered by (pos, length, fwd, rev).  (sites: ref_sites
    of the same arguments, when the caller has them already.)"""
    text = bytes(text)
    if sites is None:
        sites = ref_sites(text, omit, texts, M)
    lens = [len(bytes(x)) for x in texts]
    nsep = [0]
    for c in text:                                      # separators before position i
        nsep.append(nsep[-1] + (c == 10))
    opening = [s for s in sites if s[1] % 2 == 0]
    closing = [s for s in sites if s[1] % 2 == 1]
    out = []
    lo = 0
    for s1, e1, mm1, em1 in opening:
        a = e1 // 2
        while lo < len(closing) and closing[lo][0] < s1:
            lo += 1
        for j in range(lo, len(closing)):
            s2, e2, mm2, em2 = closing[j]
            if s2 > s1 + max_product:                   # (only the closing sites in reach; the conditions below are the definition)
                break
            b = e2 // 2
            if s2 < s1 + lens[a] or s2 + lens[b] - s1 > max_product:
                continue
            if nsep[s2 + lens[b]] != nsep[s1]:
                continue
            out.append((s1, s2 + lens[b] - s1, a, b, mm1, mm2, em1, em2))
    out.sort()
    return out


def ref_tally(products, T):
    """[a][b][clean] = the products (a, b), clean = 1 where both end-mismatch figures are 0"""
    tally = [[[0, 0] for _ in range(T)] for _ in range(T)]
    for _, _, a, b, _, _, em1, em2 in products:
        tally[a][b][1 if em1 == 0 and em2 == 0 else 0] += 1
    return tally

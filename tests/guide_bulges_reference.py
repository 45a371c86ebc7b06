"""The bulged guide-hit search as a definition, in numpy and plain Python, over every position of a text: what
kr_guide_bulges_scan must return for the bytes kr_genome_upload was given.  Brute force: every position, every
protospacer, both orientations, both kinds of bulge, every size and every cut, by comparison; no seeds, halves, hashes,
tiles or tables, and no code of krisp_amd/.

Texts, entries, staging, letters, motifs and need_pam are the unbulged search's (guide_hits_reference has them in words):
entry 2 i is text i, entry 2 i + 1 its reverse complement, both compared with the forward text; a separator, N / n and --
under omit-soft -- lower case are bad bytes; letters are letters.

For an entry's text T of G letters, the staged text S and a bulge size b in 1 .. B:

  DNA bulge (the genome holds b bases the guide has no partner for): the window is [pos, pos + G + b), the cut q runs over
  1 .. G - 1, mm(q) = #{c < q: S[pos + c] != T[c]} + #{c >= q: S[pos + c + b] != T[c]}.

  RNA bulge (b guide letters have no partner in the genome): the window is [pos, pos + G - b), the cut q runs over
  1 .. G - b - 1, text columns [q, q + b) are skipped,
  mm(q) = #{c < q: S[pos + c] != T[c]} + #{c >= q + b: S[pos + c - b] != T[c]}.

A window that holds a bad byte anywhere -- the unpartnered bases of a DNA bulge included -- is no window.  bulge_column is
the number of guide columns 5' of the bulge on the guide's strand: q for an even entry; G - q (DNA) or G - q - b (RNA) for
an odd one.  (entry, kind, b, pos) is a hit when the least mm(q) is <= M: ONE row, with that mm and, of the cuts that reach
it, the one with the smallest bulge_column (the largest q of an odd entry).  `columns` is the mask of the ALIGNED guide
columns that differ at that cut, in the guide's orientation (entry column c is guide column G - 1 - c of an odd entry);
skipped columns are never set.  The motifs read beside the window's real ends, Lw = G + b or G - b.  bulge = +b for DNA,
-b for RNA."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import guide_hits_reference as plain

HIT = np.dtype([("pos", "<i8"), ("strand", "<i8"), ("guide", "<i8"), ("bulge", "<i8"), ("mismatches", "<i8"), ("columns", "<u8"),
                ("pam", "<i8"), ("bulge_column", "<i8"), ("length", "<i8")])
FIELDS = HIT.names
rc = plain.rc


def comparisons(n, texts, B):
    """the byte comparisons of a ref_bulge_hits call on n bytes: every position, two alignments of G columns, both
    orientations, 2 B bulges"""
    G = len(texts[0]) if len(texts) else 0
    return max(n - (G - B) + 1, 0) * 2 * G * 2 * len(texts) * 2 * B


def window_row(S, bad, pos, T, odd, bulge, M):
    """one window by the definition's words, in plain Python: (mismatches, columns, bulge_column) or None.  S: the staged
    letters, bad: the bad bytes, T: the entry's text"""
    G = len(T)
    b = abs(bulge)
    Lw = G + bulge
    if pos < 0 or pos + Lw > len(S) or any(bad[pos:pos + Lw]):
        return None
    best = None
    for q in range(1, (G if bulge > 0 else G - b)):
        if bulge > 0:
            cols = [c for c in range(G) if (S[pos + c] if c < q else S[pos + c + b]) != ord(T[c])]
            column = G - q if odd else q
        else:
            cols = [c for c in range(G) if (c < q and S[pos + c] != ord(T[c])) or (c >= q + b and S[pos + c - b] != ord(T[c]))]
            column = G - q - b if odd else q
        key = (len(cols), column)
        if best is None or key < best[0]:
            best = (key, cols)
    (mm, column), cols = best
    if mm > M:
        return None
    return mm, sum(1 << (G - 1 - c if odd else c) for c in cols), column


def ref_bulge_hits(text, omit, texts, M, B, pam5="", pam3="", need_pam=False):
    """every bulged hit of the definition, ordered by (pos, strand, guide, bulge).  texts: the protospacers as str or bytes"""
    texts = [t if isinstance(t, str) else bytes(t).decode("ascii") for t in texts]
    up, bad = plain.stage(text, omit)
    n = len(up)
    if not texts:
        return np.empty(0, dtype=HIT)
    G = len(texts[0])
    assert all(len(t) == G and set(t) <= set("ACGT") for t in texts) and 12 <= G <= 40 and 0 <= M <= 3 and B in (1, 2)
    out = []
    for bulge in [s * b for b in range(1, B + 1) for s in (1, -1)]:
        b, Lw = abs(bulge), G + bulge
        if n < Lw:
            continue
        skip = b if bulge < 0 else 0
        qs = np.arange(1, G - skip)                                         # the cuts
        valid = ~sliding_window_view(bad, Lw).any(axis=1)
        windows = sliding_window_view(up, Lw)
        npos = len(windows)
        for gi, t in enumerate(texts):
            for strand, x in ((0, t), (1, rc(t))):
                xa = np.frombuffer(x.encode("ascii"), dtype=np.uint8)
                # head[:, c]: S[pos + c] != T[c] (the window aligned at its start); tail[:, c]: S[pos + c + bulge] != T[c]
                # (aligned at its end); columns that fall outside the window count nothing and are never asked for
                head = np.zeros((npos, G + 1), dtype=np.int32)
                tail = np.zeros((npos, G + 1), dtype=np.int32)
                w = min(G, Lw)
                head[:, :w] = windows[:, :w] != xa[:w]
                lo = max(0, -bulge)
                tail[:, lo:G] = windows[:, lo + bulge:G + bulge] != xa[lo:G]
                below = np.concatenate([np.zeros((npos, 1), dtype=np.int32), np.cumsum(head[:, :G], axis=1)], axis=1)   # below[:, q] = # head below q
                above = np.cumsum(tail[:, ::-1], axis=1)[:, ::-1]                                                      # above[:, c] = # tail from c on
                mm = below[:, qs] + above[:, qs + skip]
                least = mm.min(axis=1)
                for pos in np.flatnonzero(valid & (least <= M)).tolist():
                    at = np.flatnonzero(mm[pos] == least[pos])
                    q = int(qs[at[-1] if strand else at[0]])
                    cols = np.concatenate([head[pos, :q], np.zeros(skip, dtype=np.int32), tail[pos, q + skip:G]]).astype(bool)
                    if strand:
                        cols = cols[::-1]
                    mask = sum(1 << int(c) for c in np.flatnonzero(cols))
                    column = q if strand == 0 else G - q - skip
                    pam = plain.pam_bits(up, bad, pos, strand, Lw, pam5, pam3)
                    if need_pam and pam != 3:
                        continue
                    out.append((pos, strand, gi, bulge, int(least[pos]), mask, pam, column, Lw))
    out.sort()
    return np.array(out, dtype=HIT) if out else np.empty(0, dtype=HIT)


def ref_windows(text, hits):
    """the hits' windows as the guide's strand reads them: upper case, the reverse complement for strand 1 -> list of str"""
    comp = bytes.maketrans(b"ATGCRYMKSWBVDHN", b"TACGYRKMSWVBHDN")
    t = bytes(text)
    out = []
    for h in hits:
        w = t[int(h["pos"]):int(h["pos"]) + int(h["length"])].upper()
        out.append((w.translate(comp)[::-1] if int(h["strand"]) else w).decode("ascii"))
    return out

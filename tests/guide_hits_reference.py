"""The guide-hit search as a definition, in numpy and plain Python, over every position of a text: what a
scan of the library must return for the bytes kr_genome_upload was given (records joined by '\\n').  Brute force: every position, every protospacer, both orientations,
Hamming distance by comparison; no seeds, hashes, tiles or tables, and no code of krisp_amd/.

Texts and entries.  Every text is one of `nguides` protospacers of one length G (12 .. 40) in the letters A, C, G, T.  Entry
2 i is text i, entry 2 i + 1 its reverse complement.

Window.  The window at pos is the G staged bytes [pos, pos + G).  Staging: a separator ('\\n'), N / n and -- under omit-soft --
every lower-case letter are bad; other lower case becomes upper case.  (The reader writes U as T before a genome reaches
the device, as for every other scan: in a file U reads as T.  In bytes uploaded as they are, a U is a letter like R.)  A
window that holds a bad byte is no window.

Hit.  (pos, entry) is a hit when the window differs from the entry's text in at most M columns; letters are letters (R
differs from A).  `columns` is a 64-bit mask in the GUIDE'S orientation: bit c is set when guide column c differs, counted
5'->3' on the protospacer -- window column c for an even entry, window column G - 1 - c for an odd one.

Motifs, with a = len(pam5), b = len(pam3), read 5'->3' on the guide's strand.  Even entry: the 5' motif reads the bytes
[pos - a, pos), the 3' motif [pos + G, pos + G + b).  Odd entry: the 5' motif reads the reverse complement of
[pos + G, pos + G + a), the 3' motif that of [pos - b, pos).  A motif matches when every staged neighbour, complemented on
'-', is one of A, C, G, T and lies in the IUPAC set of the motif's letter at that place; a neighbour that is bad, lies
outside the text or is another letter matches nothing; an empty motif matches.  pam bit 0 = the 5' motif, bit 1 = the 3'
motif.  With need_pam a hit whose pam != 3 is no hit.

A palindromic protospacer is a hit on both strands at one position: both stay.  Equal texts stay separate guides."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

HIT = np.dtype([("pos", "<i8"), ("strand", "<i8"), ("guide", "<i8"), ("mismatches", "<i8"), ("columns", "<u8"), ("pam", "<i8")])
FIELDS = ("pos", "strand", "guide", "mismatches", "columns", "pam")
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(text):
    """the reverse complement of a text of A, C, G, T"""
    return "".join(_COMPLEMENT[ch] for ch in reversed(text))


def stage(text, omit):
    """the bytes as the scan sees them -> (uint8 letters, upper case; bool: the byte is bad)"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    lower = (t >= ord("a")) & (t <= ord("z"))
    bad = (t == ord("\n")) | (t == ord("N")) | (t == ord("n"))
    if omit:
        bad = bad | lower
    return np.where(lower, t - 32, t).astype(np.uint8), bad


def motif_matches(up, bad, motif, index, minus):
    """does `motif` (IUPAC letters, 5'->3' on the guide's strand) match the neighbours at the text indices `index`, listed in
    the order the guide's strand reads them?"""
    for ch, i in zip(motif.upper(), index):
        if i < 0 or i >= len(up) or bad[i]:
            return False
        x = chr(up[i])
        if x not in _COMPLEMENT:
            return False
        if minus:
            x = _COMPLEMENT[x]
        if x not in IUPAC[ch]:
            return False
    return True


def pam_bits(up, bad, pos, strand, G, pam5, pam3):
    a, b = len(pam5), len(pam3)
    if strand == 0:
        i5 = [pos - a + j for j in range(a)]
        i3 = [pos + G + j for j in range(b)]
    else:
        i5 = [pos + G + a - 1 - j for j in range(a)]
        i3 = [pos - 1 - j for j in range(b)]
    return (1 if motif_matches(up, bad, pam5, i5, strand == 1) else 0) | (2 if motif_matches(up, bad, pam3, i3, strand == 1) else 0)


def comparisons(n, texts):
    """the byte comparisons of a ref_hits call on n bytes: what a caller holds to about 10^8"""
    G = len(texts[0]) if len(texts) else 0
    return max(n - G + 1, 0) * G * 2 * len(texts)


def ref_hits(text, omit, texts, M, pam5="", pam3="", need_pam=False):
    """every hit of the definition above, ordered by (pos, strand, guide).  texts: the protospacers as str or bytes"""
    texts = [t if isinstance(t, str) else bytes(t).decode("ascii") for t in texts]
    up, bad = stage(text, omit)
    if not texts or len(up) < len(texts[0]):
        return np.empty(0, dtype=HIT)
    G = len(texts[0])
    assert all(len(t) == G and set(t) <= set("ACGT") for t in texts) and 12 <= G <= 40 and 0 <= M <= 3
    valid = ~sliding_window_view(bad, G).any(axis=1)
    windows = sliding_window_view(up, G)
    weights = np.uint64(1) << np.arange(G, dtype=np.uint64)
    out = []
    for gi, t in enumerate(texts):
        for strand, x in ((0, t), (1, rc(t))):
            ne = windows != np.frombuffer(x.encode("ascii"), dtype=np.uint8)
            d = np.count_nonzero(ne, axis=1)
            for pos in np.flatnonzero(valid & (d <= M)).tolist():
                cols = ne[pos] if strand == 0 else ne[pos][::-1]        # guide column c = window column G - 1 - c on '-'
                pam = pam_bits(up, bad, pos, strand, G, pam5, pam3)
                if need_pam and pam != 3:
                    continue
                out.append((pos, strand, gi, int(d[pos]), int(weights[cols].sum()), pam))
    out.sort()
    return np.array(out, dtype=HIT) if out else np.empty(0, dtype=HIT)


def ref_windows(text, hits, G):
    """the hits' windows as the guide's strand reads them: upper case, the reverse complement for strand 1 (through the
    whole IUPAC code, as the other passes' windows) -> list of str"""
    comp = bytes.maketrans(b"ATGCRYMKSWBVDHN", b"TACGYRKMSWVBHDN")
    t = bytes(text)
    out = []
    for h in hits:
        w = t[int(h["pos"]):int(h["pos"]) + G].upper()
        out.append((w.translate(comp)[::-1] if int(h["strand"]) else w).decode("ascii"))
    return out

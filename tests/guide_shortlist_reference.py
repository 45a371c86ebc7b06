"""The shortlist of --guide-candidates restated over guides_reference.candidates: every candidate of a region,
sorted as the definition orders them, the first N as records; and the pick among them as plain loops over Python ints.  It
shares no code with krisp_amd/."""
from guides_reference import FIELDS, candidates


def order(cands):
    """candidates (d, s, off-centre, strand, p, gc) best first: greatest d, greatest s, best centred, '+' before '-', leftmost"""
    return sorted(cands, key=lambda c: (-c[0], -c[1], c[2], c[3], c[4]))


def shortlist(rows, lo, hi, L, D, g, top, pam5="", pam3="", gc_lo=30, gc_hi=70, min_mismatches=1):
    """one region's `top` records as dicts of FIELDS, rank 1 first; a slot beyond the candidates is zero but `candidates`"""
    cands = order(candidates(rows, lo, hi, L, D, g, pam5, pam3, gc_lo, gc_hi, min_mismatches))
    out = []
    for j in range(top):
        rec = dict.fromkeys(FIELDS, 0)
        rec["candidates"] = len(cands)
        if j < len(cands):
            d, s, _, strand, p, gc = cands[j]
            rec.update(found=1, strand=strand, start=p, min_mismatches=d, sum_mismatches=s, gc=gc)
        out.append(rec)
    return out


def shortlists(regions, L, D, g, top, pam5="", pam3="", gc=(30, 70), min_mismatches=1):
    """regions: (rows, lo, hi) each -> a list of lists of records"""
    return [shortlist(rows, lo, hi, L, D, g, top, pam5, pam3, gc[0], gc[1], min_mismatches) for rows, lo, hi in regions]


def lanes(rows, lo, hi, L, D, g, top, pam5="", pam3="", gc_lo=30, gc_hi=70, min_mismatches=1):
    """(the region's number of candidates, the kernel lanes (2 (p - lo) + strand) mod 64 of its first `top`)"""
    cands = order(candidates(rows, lo, hi, L, D, g, pam5, pam3, gc_lo, gc_hi, min_mismatches))
    return len(cands), [(2 * (c[4] - min(lo, hi)) + c[3]) % 64 for c in cands[:top]]


def pick(tallies, mismatches):
    """tallies: per slot a sequence of counts, or None for an empty slot -> (the 0-based rank of the slot with the
    lexicographically smallest (t0, ..., tM), the lower rank on a tie; the tally), (0, zeros) for no filled slot"""
    best = None
    for j, t in enumerate(tallies):
        if t is None:
            continue
        key = tuple(int(x) for x in t[:mismatches + 1])
        if best is None or key < best[1]:
            best = (j, key)
    return best if best is not None else (0, (0,) * (mismatches + 1))

"""The assay join as a definition, in plain Python: which (product, hit) pairs of one genome are assay hits.
The products are primers_reference.ref_products' list, the hits guide_hits_reference.ref_hits' list (need_pam's selection
made), both of the same bytes.  Brute force: two nested loops over the lists and the record check; no search structure, no
order that is made use of, and no code of krisp_amd/.

Product P of pair p on strand s: its FIRST site has the left text's length on strand 0 and the right text's on strand 1,
its SECOND site the other one; its interior is [P.pos + len(first), P.pos + P.length - len(second)): the bases between the
two primer sites.  The amplicon carries the primers' letters at the sites, not the genome's, so a window that reaches into
a site does not count.

Assay hit: a (P, H) with interior.lo <= H.pos, H.pos + G <= interior.hi, (P.pair, H.guide) a link, and P and H on one
record (containment implies it -- a product lies on one record --; it is checked anyway)."""
import bisect

import numpy as np

ASSAY = np.dtype([("pos", "<i8"), ("length", "<i8"), ("strand", "<i8"), ("pair", "<i8"), ("hit_pos", "<i8"), ("hit_strand", "<i8"),
                  ("guide", "<i8"), ("left_mm", "<i8"), ("right_mm", "<i8"), ("left_end_mm", "<i8"), ("right_end_mm", "<i8"),
                  ("mismatches", "<i8"), ("columns", "<u8"), ("pam", "<i8")])


def interior(P, lengths):
    """[lo, hi) of product P; lengths[p] = (the left text's length, the right text's) of pair p"""
    nl, nr = lengths[int(P["pair"])]
    first, second = (nl, nr) if int(P["strand"]) == 0 else (nr, nl)
    return int(P["pos"]) + first, int(P["pos"]) + int(P["length"]) - second


def record_of(seps, pos):
    """the record that holds position pos: the separators before it (seps: their positions, ascending)"""
    return bisect.bisect_left(list(seps), pos)


def ref_assay_hits(products, hits, lengths, links, G, seps=()):
    """every assay hit, ordered by (pos, length, strand, pair, hit_pos, hit_strand, guide).  products, hits: arrays with the
    fields of primers_reference.PRODUCT and guide_hits_reference.HIT; links: (pair, guide) rows; seps: the positions of the
    record separators (none: one record)"""
    linked = {(int(p), int(g)) for p, g in np.asarray(links, dtype=np.int64).reshape(-1, 2).tolist()}
    out = []
    for P in products:
        lo, hi = interior(P, lengths)
        for H in hits:
            hp = int(H["pos"])
            if not (lo <= hp and hp + G <= hi):
                continue
            if (int(P["pair"]), int(H["guide"])) not in linked:
                continue
            if not (record_of(seps, int(P["pos"])) == record_of(seps, hp) == record_of(seps, hp + G - 1)):
                continue
            out.append((int(P["pos"]), int(P["length"]), int(P["strand"]), int(P["pair"]), hp, int(H["strand"]), int(H["guide"]),
                        int(P["left_mm"]), int(P["right_mm"]), int(P["left_end_mm"]), int(P["right_end_mm"]), int(H["mismatches"]),
                        int(H["columns"]), int(H["pam"])))
    out.sort()
    return np.array(out, dtype=ASSAY) if out else np.empty(0, dtype=ASSAY)

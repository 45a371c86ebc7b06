"""Brute-force restatement of --primer-candidates, the yardstick of test_design_shortlist_host.py,
test_gpu_design_shortlist.py and test_gpu_primer_candidates_cli.py.  The shortlist is
sorted(design_reference.passing_pairs(...))[:N] turned into records, with the hairpin filter of hairpin_reference.py on the
candidates where the check is on; the pick is plain loops over a region's tallies.  Python ints and numpy only.
"""
import numpy as np

import design_reference as DR
import hairpin_reference as HR
from krisp_amd import thermo as T
from krisp_amd._native import DESIGN_RECORD, DESIGN_RECORD_HP


def passing(template, L, D, R, o, hairpins=False):
    """-> (left, right, rows): the candidates (with their hairpin figure where the check is on) and every passing pair as
    design_reference.passing_pairs lists it, sorted: ascending (pair_penalty, left_start, left_len, right_start, right_len)
    -- the tuple's first five entries, which no two pairs share"""
    if not hairpins:
        left, right, rows = DR.passing_pairs(template, L, D, R, o)
        return left, right, sorted(rows)
    assert len(template) == L + D + R
    left, right = DR.candidates(template, L, D, R, o)
    for side in (left, right):
        for key in list(side):
            side[key]["hairpin"] = HR.hairpin_figure(side[key]["seq"])
            if side[key]["hairpin"] > o["max_sec"]:
                del side[key]
    rows = []
    for (ls, ln), a in left.items():
        for (rs, rn), b in right.items():
            size = rs + rn - ls
            if not o["amp_lo"] <= size <= o["amp_hi"]:
                continue
            pa, pe = DR.duplex_figure(a["seq"], b["seq"])
            if pa > o["max_sec"] or pe > o["max_sec"]:
                continue
            rows.append((a["pen"] + b["pen"], ls, ln, rs, rn, size, pa, pe))
    return left, right, sorted(rows)


def record(left, right, row):
    """a passing pair's row -> the record's fields"""
    pen, ls, ln, rs, rn, size, pa, pe = row
    a, b = left[(ls, ln)], right[(rs, rn)]
    r = {"found": 1, "product_size": size, "pair_penalty": pen, "left_start": ls, "left_len": ln, "right_start": rs,
         "right_len": rn, "left_tm": a["tm"], "right_tm": b["tm"], "left_gc": a["gc"], "right_gc": b["gc"],
         "left_penalty": a["pen"], "right_penalty": b["pen"], "left_self_any": a["self_any"], "left_self_end": a["self_end"],
         "right_self_any": b["self_any"], "right_self_end": b["self_end"], "pair_any": pa, "pair_end": pe}
    if "hairpin" in a:
        r["left_hairpin"], r["right_hairpin"] = a["hairpin"], b["hairpin"]
    return r


def passing_all(templates, L, D, R, hairpins=False, **opts):
    """per template: passing(...), computed once and sliced by shortlist() for every N"""
    o = T.options(**opts)
    return [passing(t if isinstance(t, str) else bytes(t).decode("ascii"), L, D, R, o, hairpins) for t in templates]


def shortlist(passed, top, hairpins=False):
    """passing_all's list -> DESIGN_RECORD (DESIGN_RECORD_HP) [templates, top]: slot j = the pair of rank j + 1, all zero
    behind a region's last pair"""
    out = np.zeros((len(passed), top), dtype=DESIGN_RECORD_HP if hairpins else DESIGN_RECORD)
    for i, (left, right, rows) in enumerate(passed):
        for j, row in enumerate(rows[:top]):
            for k, v in record(left, right, row).items():
                out[i, j][k] = v
    return out


def tally_key(tally8, M):
    """kr_primers_tally's eight columns (t0 .. t6, clean) -> what the pick compares: (clean, t0, ..., t2M)"""
    t = [int(x) for x in tally8]
    return tuple([t[7]] + t[:2 * M + 1])


def pick(keys):
    """a region's tallies in rank order (tuples of equal length) -> the 0-based rank of the pick: the lexicographically
    smallest tally, the lower rank where tallies tie"""
    best = None
    for j, k in enumerate(keys):
        if best is None or tuple(k) < tuple(keys[best]):
            best = j
    return best


def pick_all(found, index, tallies, M):
    """found, index: [regions, top] (index -1: an empty slot), tallies: [pairs, 8] -> the rank of every region's pick, 0
    where it has no pair"""
    ranks = []
    for i in range(len(index)):
        keys = [tally_key(tallies[int(index[i][j])], M) for j in range(len(index[i])) if int(index[i][j]) >= 0]
        assert len(keys) == int(sum(int(f) != 0 for f in found[i]))
        ranks.append(pick(keys) if keys else 0)
    return ranks

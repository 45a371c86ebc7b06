"""Brute-force restatement of the primer design pass's definition, the yardstick of test_design_host.py and
test_gpu_design.py.  Python ints and numpy only; it walks every candidate, every pair within the product range, every
alignment and every run, and takes the minimum at the end: no ordering, no bound, no prefix sum.  It shares with the
package the integer tables of krisp_amd/thermo.py and nothing else.
"""
import numpy as np

from krisp_amd import thermo as T
from krisp_amd._native import DESIGN_RECORD

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(_COMP)


def duplex_tm(x, self_complementary=False, symmetry=False):
    """Tm in mK of the oligo x with its complement: nearest-neighbour sums, both terminals, salt per step, concentration"""
    dh = sum(T.NN_DH[4 * T.BASES.index(a) + T.BASES.index(b)] for a, b in zip(x, x[1:]))
    ds = sum(T.NN_DS[4 * T.BASES.index(a) + T.BASES.index(b)] for a, b in zip(x, x[1:]))
    for b in (x[0], x[-1]):
        dh += T.TERM_DH[T.BASES.index(b)]
        ds += T.TERM_DS[T.BASES.index(b)]
    ds += T.SALT_DS * (len(x) - 1)
    ds += T.CONC_SELF_DS if self_complementary else T.CONC_DS
    if symmetry:
        ds += T.SYM_DS
    assert dh < 0 and ds < 0
    return (dh * 10 ** 6) // ds


def primer_tm(x):
    pal = x == rc(x)
    return duplex_tm(x, self_complementary=pal, symmetry=pal)


def duplex_figure(x, y):
    """(any, end) of the oligos x and y, both written 5'->3': every ungapped antiparallel alignment c = i + j, every maximal
    run of at least two Watson-Crick pairs, the Tm of the run's bases on x; end: the runs that hold x[-1] or y[-1]"""
    any_, end = 0, 0
    for c in range(len(x) + len(y) - 1):
        cells = [(i, c - i) for i in range(len(x)) if 0 <= c - i < len(y)]
        paired = [x[i] == y[j].translate(_COMP) for i, j in cells]
        k = 0
        while k < len(cells):
            if not paired[k]:
                k += 1
                continue
            k1 = k
            while k1 + 1 < len(cells) and paired[k1 + 1]:
                k1 += 1
            if k1 > k:
                tm = duplex_tm(x[cells[k][0]:cells[k1][0] + 1])
                any_ = max(any_, tm)
                if any(i == len(x) - 1 or j == len(y) - 1 for i, j in cells[k:k1 + 1]):
                    end = max(end, tm)
            k = k1 + 1
    return any_, end


def single_ok(x, o):
    """the single-primer filters; -> (Tm, GC count) or None"""
    if set(x) - set("ACGT"):
        return None
    n = len(x)
    gc = x.count("G") + x.count("C")
    if not (100 * gc >= o["gc_lo"] * n and 100 * gc <= o["gc_hi"] * n):
        return None
    if any(len(set(x[i:i + T.MAX_POLY_X + 1])) == 1 for i in range(n - T.MAX_POLY_X)):
        return None
    if any(b not in "GC" for b in x[n - o["gc_clamp"]:]):
        return None
    if sum(b in "GC" for b in x[-T.END_BASES:]) > o["max_end_gc"]:
        return None
    tm = primer_tm(x)
    if not o["tm_lo"] <= tm <= o["tm_hi"]:
        return None
    return tm, gc


def penalty(tm, n, o):
    return abs(tm - o["tm_opt"]) + T.SIZE_WEIGHT * abs(2 * n - (o["size_lo"] + o["size_hi"]))


def candidates(template, L, D, R, o, self_check=True):
    """-> (left, right): dicts (start, length) -> {seq, tm, gc, pen, self_any, self_end} of the candidates that pass the
    single filters and the self figures"""
    sides = ([], [])
    for n in range(o["size_lo"], o["size_hi"] + 1):
        sides[0].extend((s, n, template[s:s + n]) for s in range(0, L - n + 1))
        sides[1].extend((s, n, rc(template[s:s + n])) for s in range(L + D, L + D + R - n + 1))
    out = ({}, {})
    for q in (0, 1):
        for s, n, x in sides[q]:
            ok = single_ok(x, o)
            if ok is None:
                continue
            sa, se = duplex_figure(x, x)
            if self_check and (sa > o["max_sec"] or se > o["max_sec"]):
                continue
            out[q][(s, n)] = {"seq": x, "tm": ok[0], "gc": ok[1], "pen": penalty(ok[0], n, o), "self_any": sa, "self_end": se}
    return out


def passing_pairs(template, L, D, R, o):
    """-> (left, right, rows): every pair that passes everything, as (pair penalty, left_start, left_len, right_start,
    right_len, product size, pair_any, pair_end)"""
    assert len(template) == L + D + R
    left, right = candidates(template, L, D, R, o)
    rows = []
    for (ls, ln), a in left.items():
        for (rs, rn), b in right.items():
            size = rs + rn - ls
            if not o["amp_lo"] <= size <= o["amp_hi"]:
                continue
            pa, pe = duplex_figure(a["seq"], b["seq"])
            if pa > o["max_sec"] or pe > o["max_sec"]:
                continue
            rows.append((a["pen"] + b["pen"], ls, ln, rs, rn, size, pa, pe))
    return left, right, rows


def design_one(template, L, D, R, o):
    """the region's answer as a dict of the record's fields, or None"""
    left, right, rows = passing_pairs(template, L, D, R, o)
    if not rows:
        return None
    pen, ls, ln, rs, rn, size, pa, pe = min(rows)
    a, b = left[(ls, ln)], right[(rs, rn)]
    return {"found": 1, "product_size": size, "pair_penalty": pen, "left_start": ls, "left_len": ln, "right_start": rs,
            "right_len": rn, "left_tm": a["tm"], "right_tm": b["tm"], "left_gc": a["gc"], "right_gc": b["gc"],
            "left_penalty": a["pen"], "right_penalty": b["pen"], "left_self_any": a["self_any"], "left_self_end": a["self_end"],
            "right_self_any": b["self_any"], "right_self_end": b["self_end"], "pair_any": pa, "pair_end": pe}


def design(templates, L, D, R, **opts):
    """templates: str or bytes rows -> DESIGN_RECORD array, one row per template (all zero: no pair)"""
    o = T.options(**opts)
    out = np.zeros(len(templates), dtype=DESIGN_RECORD)
    for i, t in enumerate(templates):
        r = design_one(t if isinstance(t, str) else bytes(t).decode("ascii"), L, D, R, o)
        if r is not None:
            for k, v in r.items():
                out[i][k] = v
    return out

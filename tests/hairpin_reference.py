"""Brute-force restatement of the hairpin figure of --design-primers --hairpins, the yardstick of
test_hairpin_host.py and test_gpu_hairpins.py.  Python ints only: every fold, every pair, every run, the maximum at the end.
The rest of the designer is design_reference.py's; the tables are krisp_amd/thermo.py's.
"""
import numpy as np

import design_reference as DR
from krisp_amd import thermo as T
from krisp_amd._native import DESIGN_RECORD, DESIGN_RECORD_HP

_PAIRS = {("A", "T"), ("T", "A"), ("C", "G"), ("G", "C")}


def admissible(x, i, j):
    """three bases at least between the two, and the two Watson-Crick"""
    return 0 <= i and j < len(x) and j - i >= T.HAIRPIN_MIN_LOOP + 1 and (x[i], x[j]) in _PAIRS


def stem_tm(x, i0, i1, loop):
    """Tm in mK of the stem whose 5' arm is x[i0 .. i1] around a loop of `loop` bases: the duplex's steps, both terminals and
    salt; the loop's dS in the place of the concentration; no symmetry term"""
    s = x[i0:i1 + 1]
    dh = sum(T.NN_DH[4 * T.BASES.index(a) + T.BASES.index(b)] for a, b in zip(s, s[1:]))
    ds = sum(T.NN_DS[4 * T.BASES.index(a) + T.BASES.index(b)] for a, b in zip(s, s[1:]))
    for b in (s[0], s[-1]):
        dh += T.TERM_DH[T.BASES.index(b)]
        ds += T.TERM_DS[T.BASES.index(b)]
    ds += T.SALT_DS * (len(s) - 1) + T.LOOP_DS[loop]
    assert dh < 0 and ds < 0 and T.HAIRPIN_MIN_LOOP <= loop <= T.HAIRPIN_MAX_LOOP
    return (dh * 10 ** 6) // ds


def stems(x):
    """every stem of the oligo x as (fold, i0, i1, loop length, Tm)"""
    out = []
    for c in range(2 * len(x) - 1):
        for i0 in range(len(x)):
            if not admissible(x, i0, c - i0) or admissible(x, i0 - 1, c - i0 + 1):
                continue                        # (a run starts where the pair before it is outside the oligo or no pair)
            i1 = i0
            while admissible(x, i1 + 1, c - i1 - 1):
                i1 += 1
            if i1 > i0:
                loop = c - 2 * i1 - 1
                out.append((c, i0, i1, loop, stem_tm(x, i0, i1, loop)))
    return out


def hairpin_figure(x):
    return max((s[4] for s in stems(x)), default=0)


def deciding_folds(x):
    """the folds on which the figure is reached (empty without a stem)"""
    st = stems(x)
    top = max((s[4] for s in st), default=0)
    return sorted({s[0] for s in st if s[4] == top})


def design_one(template, L, D, R, o):
    """design_reference.design_one with the hairpin filter on the candidates; the record's fields and the two figures"""
    assert len(template) == L + D + R
    left, right = DR.candidates(template, L, D, R, o)
    for side in (left, right):
        for key in list(side):
            side[key]["hairpin"] = hairpin_figure(side[key]["seq"])
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
    if not rows:
        return None
    pen, ls, ln, rs, rn, size, pa, pe = min(rows)
    a, b = left[(ls, ln)], right[(rs, rn)]
    return {"found": 1, "product_size": size, "pair_penalty": pen, "left_start": ls, "left_len": ln, "right_start": rs,
            "right_len": rn, "left_tm": a["tm"], "right_tm": b["tm"], "left_gc": a["gc"], "right_gc": b["gc"],
            "left_penalty": a["pen"], "right_penalty": b["pen"], "left_self_any": a["self_any"], "left_self_end": a["self_end"],
            "right_self_any": b["self_any"], "right_self_end": b["self_end"], "pair_any": pa, "pair_end": pe,
            "left_hairpin": a["hairpin"], "right_hairpin": b["hairpin"]}


def design(templates, L, D, R, hairpins=True, **opts):
    """templates: str or bytes rows -> DESIGN_RECORD_HP array, one row per template (all zero: no pair); hairpins=False:
    design_reference.design's DESIGN_RECORD array"""
    if not hairpins:
        return DR.design(templates, L, D, R, **opts)
    o = T.options(**opts)
    out = np.zeros(len(templates), dtype=DESIGN_RECORD_HP)
    for i, t in enumerate(templates):
        r = design_one(t if isinstance(t, str) else bytes(t).decode("ascii"), L, D, R, o)
        if r is not None:
            for k, v in r.items():
                out[i][k] = v
    return out


def plain(records):
    """the DESIGN_RECORD part of a DESIGN_RECORD_HP array (64 bytes a row)"""
    out = np.zeros(len(records), dtype=DESIGN_RECORD)
    for name in DESIGN_RECORD.names:
        out[name] = records[name]
    return out


def winner_sequences(template, rec):
    """the two primers of a found record, 5'->3'"""
    ls, ln, rs, rn = (int(rec[k]) for k in ("left_start", "left_len", "right_start", "right_len"))
    return template[ls:ls + ln], DR.rc(template[rs:rs + rn])

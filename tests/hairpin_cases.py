"""The templates and option sets of test_gpu_hairpins.py and the census of test_hairpin_host.py, in a module of their own so
that the brute-force reference can be run and timed over exactly them without a GPU (PYTHONPATH=. python
tests/hairpin_cases.py prints the census and the seconds).  Every case: random templates, then templates with a structure
planted inside the span the plain designer's winner covers (where it fits, else anywhere in the flank), on either flank."""
import functools
import random

import design_reference as DR
import hairpin_reference as HR
from krisp_amd import thermo as T

# name -> geometry, random templates, the plants' seeds, the options; `sets`: the --max_sec_tm values, each with the kinds of
# region the census must find under it (test_hairpin_host.py): "differs" the winner is not the plain run's, "lost" the plain
# run has a pair and the hairpin run none, "kept" a winner with a hairpin figure above 0, "round2" a winner's figure decided
# on folds of 68 or more alone (the second round of lanes: fold 4 + lane + 64), or a primer of the plain run's winner whose
# figure is above the limit and decided there alone (missing the round would leave the plain record standing)
CASES = {
    "30_40_30_short": dict(geo=(30, 40, 30), n_random=14, plants=1,
                           base=dict(primer_size=(10, 14), tm=(20, 60), gc=(20, 80), amp_size=(98, 100), gc_clamp=0, max_end_gc=5),
                           sets={-5: ("differs", "kept"), 40: ("kept",)}),
    "30_40_30": dict(geo=(30, 40, 30), n_random=6, plants=1,
                     base=dict(primer_size=(18, 24), tm=(48, 66), gc=(30, 70), amp_size=(97, 100), gc_clamp=0, max_end_gc=5),
                     sets={20: ("differs", "lost", "kept"), 40: ("differs", "lost", "kept")}),
    "12_4_12": dict(geo=(12, 4, 12), n_random=30, plants=1,
                    base=dict(primer_size=(10, 12), tm=(15, 50), gc=(20, 80), amp_size=(27, 28), gc_clamp=0, max_end_gc=5),
                    sets={-5: ("differs", "lost", "kept"), 40: ("kept",)}),
    "64_20_64": dict(geo=(64, 20, 64), n_random=2, plants=1,
                     base=dict(primer_size=(36, 38), tm=(60, 90), gc=(30, 70), amp_size=(146, 148), gc_clamp=0, max_end_gc=5),
                     sets={25: ("differs", "lost", "kept"), 40: ("lost", "kept")}),
    "60_10_60": dict(geo=(60, 10, 60), n_random=10, plants=1,
                     base=dict(primer_size=(58, 60), tm=(60, 95), gc=(30, 70), amp_size=(126, 130), gc_clamp=0, max_end_gc=5),
                     sets={30: ("lost", "kept", "round2"), 40: ("lost", "kept", "round2")}),
    "256_60_256": dict(geo=(256, 60, 256), n_random=2, plants=0,
                       base=dict(primer_size=(10, 60), tm=(58, 62), gc=(35, 65), amp_size=(564, 572), gc_clamp=1, max_end_gc=3),
                       sets={25: ("kept",)}),
}
ROUND2_FOLD = 68


def _rand(rng, n, weights=(1, 1, 1, 1)):
    return "".join(rng.choices("ACGT", weights=weights, k=n))


def stem(rng, pairs, loop, letter=None):
    """an arm of `pairs` bases (G and C twice as likely), `loop` bases that do not carry the stem on, the arm's reverse
    complement; `letter`: an IUPAC letter in the middle of the loop"""
    arm = _rand(rng, pairs, (1, 2, 2, 1))
    while True:
        lp = _rand(rng, loop)
        if loop < 5 or (lp[0], lp[-1]) not in HR._PAIRS:
            break
    if letter:
        lp = lp[:loop // 2] + letter + lp[loop // 2 + 1:]
    return arm + lp + DR.rc(arm)


def palindrome(rng, half):
    """its own reverse complement: the pairs run inwards until three bases are left between them"""
    s = _rand(rng, half, (1, 2, 2, 1))
    return s + DR.rc(s)


def split_fold(rng):
    """two stems on one fold: 3 pairs, a mismatch, 3 pairs, a loop of 4"""
    a, b = _rand(rng, 3, (1, 2, 2, 1)), _rand(rng, 3, (1, 2, 2, 1))
    return a + "A" + b + _rand(rng, 4) + DR.rc(b) + "A" + DR.rc(a)


def structures(rng):
    out = [stem(rng, p, l) for p in (2, 3, 6) for l in (3, 4, 5, 30)]
    return out + [palindrome(rng, 6), palindrome(rng, 8), split_fold(rng), stem(rng, 4, 5, letter="N"), stem(rng, 3, 7, letter="R")]


def _plant(rng, t, s, span, flank, reverse):
    """s into the template t: inside `span` = (start, length) if it fits there, else inside `flank`; None if in neither.
    reverse: the structure is written on the other strand (a right primer reads it)"""
    if reverse:
        s = DR.rc(s)
    for lo, n in (span, flank):
        if lo is not None and len(s) <= n:
            p = lo + rng.randrange(0, n - len(s) + 1)
            return t[:p] + s + t[p + len(s):]
    return None


@functools.lru_cache(maxsize=None)
def templates(name):
    case = CASES[name]
    L, D, R = case["geo"]
    W = L + D + R
    rng = random.Random(7000 * L + 10 * R + case["base"]["primer_size"][0])
    out = [_rand(rng, W) for _ in range(case["n_random"])]
    o = T.options(max_sec_tm=1000, **case["base"])
    for _ in range(case["plants"]):
        for k, s in enumerate(structures(rng)):
            t = _rand(rng, W)
            r = DR.design_one(t, L, D, R, o)
            right = k % 2 == 1
            if r is None:
                span = (None, 0)
            elif right:
                span = (r["right_start"], r["right_len"])
            else:
                span = (r["left_start"], r["left_len"])
            t2 = _plant(rng, t, s, span, (L + D, R) if right else (0, L), right)
            if t2 is not None:
                out.append(t2)
        # a short stem flush with the 3' end of the plain winner's primer: its folds are the primer's last ones
        for k in range(6):
            t = _rand(rng, W)
            r = DR.design_one(t, L, D, R, o)
            if r is None:
                continue
            s = stem(rng, 3 + k // 2 % 2, 3)
            if k % 2:
                p, s = r["right_start"], DR.rc(s)
            else:
                p = r["left_start"] + r["left_len"] - len(s)
            out.append(t[:p] + s + t[p + len(s):])
    return tuple(out)


def options(name, max_sec_tm):
    return dict(CASES[name]["base"], max_sec_tm=max_sec_tm)


@functools.lru_cache(maxsize=None)
def reference(name, max_sec_tm, hairpins=True):
    """the reference's records of the case under one option set, computed once and shared (read only)"""
    L, D, R = CASES[name]["geo"]
    recs = HR.design(templates(name), L, D, R, hairpins=hairpins, **options(name, max_sec_tm))
    recs.setflags(write=False)
    return recs


def census(name, max_sec_tm):
    """-> the number of regions of each kind, from the reference alone"""
    ts = templates(name)
    hp, pl = reference(name, max_sec_tm), reference(name, max_sec_tm, hairpins=False)
    n = dict(regions=len(ts), plain=int(pl["found"].sum()), found=int(hp["found"].sum()), differs=0, lost=0, kept=0, round2=0)
    sec = T.mk(max_sec_tm)
    for t, a, b in zip(ts, hp, pl):
        if int(b["found"]) and not int(a["found"]):
            n["lost"] += 1
        if int(b["found"]):
            n["round2"] += any(HR.hairpin_figure(x) > sec and HR.deciding_folds(x)[0] >= ROUND2_FOLD for x in HR.winner_sequences(t, b))
        if not int(a["found"]):
            continue
        if any(int(a[k]) != int(b[k]) for k in pl.dtype.names):
            n["differs"] += 1
        seqs = HR.winner_sequences(t, a)
        n["kept"] += int(a["left_hairpin"]) > 0 or int(a["right_hairpin"]) > 0
        n["round2"] += any(f and f[0] >= ROUND2_FOLD for f in map(HR.deciding_folds, seqs))
    return n


if __name__ == "__main__":
    import sys
    import time
    t00 = time.time()
    for name in (sys.argv[1:] or CASES):
        t0 = time.time()
        ts = templates(name)
        print(name, "templates", len(ts), f"{time.time() - t0:.1f} s", flush=True)
        for sec, kinds in CASES[name]["sets"].items():
            t0 = time.time()
            c = census(name, sec)
            print("  max_sec_tm", sec, c, "missing", [k for k in kinds if not c[k]], f"{time.time() - t0:.1f} s", flush=True)
    print(f"total {time.time() - t00:.1f} s")

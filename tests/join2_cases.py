"""Seeded pairs of genomes for the two-genome join (k_join2.inc, DESIGN §3 "k_join2"): one ingroup and one outgroup genome, one
diagnostic column, filter on -- at the shapes where its screen, its exact table and its range edges can go wrong.  No code of
krisp_amd/ but synth; the planting helpers are tests/coarse_cases.py's.  Every case returns (texts, flags, plants).

The host's geometry (plan_sort, item_plan) and the screen (csrc/j2_screen.inc) are restated here in numpy:
tests/test_join2_cases.py holds each case to the branch it is named for with the oracle alone, tests/test_join2_screen.py
holds the restated constants to the include, tests/test_gpu_join2.py runs the cases on the device.

The route needs the kernels with 32-bit heads: the sub-bin field of an item at most 32 bits above the prefix's lowest bit,
that is at least 2^(22 - p0) items of about 1 500 anchor keys.  With (25, 1, 2) -- p0 = 10, what the planting helpers write --
that takes genomes of 0.7 Mbp or more (PLANT_LEN); the uniform families are (20, 1, 6) at 300 kbp."""
import functools
import math
import zlib

import numpy as np

import coarse_cases as cc
from krisp_amd import synth

LDR = cc.LDR                        # (25, 1, 2): the planted cases
L, D, R = LDR
UNIFORM_LDR = (20, 1, 6)
UNIFORM_LEN = 300_000
PLANT_LEN = 800_000
RECORDS = cc.RECORDS

# h_core.inc / h_intersect.inc / k_intersect3.inc
BUCKET_AVG = 1600
I3_SLOTS = 2048
I3T_NB_LOG = 12
# j2_screen.inc
J2_SCREEN_LOG = 14
J2_TAB_LOG = 10
J2_PROBES = 64
SLOT_K = (0x9E3779B1, 0x85EBCA77)
TAB_K = (0xC2B2AE3D, 0x27D4EB2F)


def geometry(max_bases, anchor_keys, ldr):
    """what kr_set_params and item_plan make of it -> dict(b, rb, mlog, T, p0, sh, w, tagk)"""
    b = 8
    while b < 18 and ((2 * max_bases) >> b) > BUCKET_AVG:
        b += 1
    avg = max(anchor_keys, 1) / (1 << b)
    need = lambda m: m + 6.0 * math.sqrt(m) + 8.0                           # noqa: E731
    mlog = 0
    while (2 << mlog) <= (1 << b) and need(avg * (2 << mlog)) <= I3_SLOTS:
        mlog += 1
    T = int(min(512.0, max(256.0, 64.0 * math.ceil(need(avg * (1 << mlog)) / 256.0))))
    p0 = 64 - 2 * (ldr[0] + ldr[2])
    sh = 64 - b + mlog - I3T_NB_LOG
    return dict(b=b, rb=64 - b, mlog=mlog, T=T, p0=p0, sh=sh, w=sh + I3T_NB_LOG - p0,
                tagk=0 <= p0 < 32 and 32 <= sh <= p0 + 32)


def item_of(keys, geo):
    return np.asarray(keys, dtype=np.uint64) >> np.uint64(geo["rb"] + geo["mlog"])


def item_key(keys, geo):
    return (np.asarray(keys, dtype=np.uint64) >> np.uint64(geo["p0"])) & np.uint64((1 << geo["w"]) - 1)


def _mix(ik, k):
    ik = np.asarray(ik, dtype=np.uint64)
    lo, hi = ik & np.uint64(0xFFFFFFFF), ik >> np.uint64(32)
    with np.errstate(over="ignore"):
        return (lo * np.uint64(k[0]) + hi * np.uint64(k[1])) & np.uint64(0xFFFFFFFF)


def slot_of(ik):
    return (_mix(ik, SLOT_K) >> np.uint64(32 - J2_SCREEN_LOG)).astype(np.int64)


def tab_hash(ik):
    return (_mix(ik, TAB_K) >> np.uint64(32 - J2_TAB_LOG)).astype(np.int64)


def live(a, b):
    """the rule of j2_live: a, b = the four-bit base sets of the anchor and of the other genome in one slot"""
    a, b = np.asarray(a) & 15, np.asarray(b) & 15
    u = a | b
    return (a != 0) & (b != 0) & ((u & (u - 1)) != 0)


def screen(keys_a, keys_b, geo):
    """-> per item: dict slot -> (a, b) as the kernel's screen would hold them (host model, for the twin's counts)"""
    out = {}
    for side, keys in enumerate((keys_a, keys_b)):
        it = item_of(keys, geo).astype(np.int64)
        sl = slot_of(item_key(keys, geo))
        base = ((keys >> np.uint64(geo["p0"] - 2)) & np.uint64(3)).astype(np.int64)
        word = it * (1 << J2_SCREEN_LOG) + sl
        for bb in range(4):
            for wv in np.unique(word[base == bb]):
                e = out.setdefault(int(wv), [0, 0])
                e[side] |= 1 << bb
    return out


def live_share(keys_a, keys_b, geo):
    """the share of all keys whose slot is live"""
    scr = screen(keys_a, keys_b, geo)
    words = np.array(sorted(scr), dtype=np.int64)
    ab = np.array([scr[int(w)] for w in words], dtype=np.int64).reshape(-1, 2)
    lv = words[live(ab[:, 0], ab[:, 1])]
    n = tot = 0
    for keys in (keys_a, keys_b):
        word = item_of(keys, geo).astype(np.int64) * (1 << J2_SCREEN_LOG) + slot_of(item_key(keys, geo))
        n += int(np.isin(word, lv).sum())
        tot += len(keys)
    return n / max(tot, 1)


# ----------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(("join2 " + name).encode()))


def _texts(codes):
    return [synth.codes_to_text(c, RECORDS) for c in codes]


def _pair(config, anchor=0, mu=0.01):
    """codes of an ingroup and an outgroup genome of PLANT_LEN; the genome `anchor` is made the shorter one later"""
    codes, flags = cc._family_codes(config, 1, 1, PLANT_LEN, mu)
    return codes, flags


def _finish(codes, anchor):
    codes = list(codes)
    codes[anchor] = codes[anchor][:len(codes[anchor]) - 64]
    return _texts(codes)


def _plant(codes, at, prefix, base):
    cc._put(codes, at, cc.window(int(prefix) | int(base) << cc.DIAG_SHIFT))


def _prefix(rng, head=None):
    """a random 54-bit prefix (MSB-aligned), its first five bases `head` (0 .. 1023) where given"""
    p = int(rng.integers(0, 1 << 54, dtype=np.uint64))
    if head is not None:
        p = (p & ((1 << 44) - 1)) | head << 44
    return p << 10


PLANT_GEO = geometry(PLANT_LEN + RECORDS - 1, 2 * PLANT_LEN, LDR)


def uniform(config, masked, anchor):
    fam = synth.family(config, 1, 1, UNIFORM_LEN, records=RECORDS, mu=0.01, snp_every=2000,
                       n_frac=0.02 if masked else 0.0, lower_frac=0.1 if masked else 0.0)
    texts = [t for _, _, t in fam]
    texts[anchor] = texts[anchor][:len(texts[anchor]) - 64]
    return texts, [f for _, f, _ in fam], {}


TRAP_KINDS = ("overlap", "two_out", "dup", "shared")
TRAP_EACH = 6
A_, C_, G_, T_ = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def trap(anchor=0):
    """plants[kind] = prefixes.  Genome 0 (ingroup) / genome 1 (outgroup) show under them:
    "overlap" {a, c} / {c}: no candidate;  "two_out" {a} / {c, g}: a candidate with two out bits;
    "dup" {a, a} / {c}: a candidate whose ingroup key is there twice;  "shared" {a} / {a}: none"""
    rng = _rng("trap")
    codes, flags = _pair(61)
    slot = cc._slots()
    plants = {k: [] for k in TRAP_KINDS}
    show = {"overlap": ((A_, C_), (C_,)), "two_out": ((A_,), (C_, G_)), "dup": ((A_, A_), (C_,)), "shared": ((A_,), (A_,))}
    for kind in TRAP_KINDS:
        for _ in range(TRAP_EACH):
            p = _prefix(rng)
            plants[kind].append(p)
            ats = [next(slot), next(slot)]
            for g in (0, 1):
                for at, b in zip(ats, show[kind][g]):
                    _plant(codes[g], at, p, b)
    return _finish(codes, anchor), flags, plants


def _same_slot(rng, p, geo):
    """another prefix of p's item in p's screen slot"""
    ik = int(item_key(p, geo))
    top = (p >> (geo["p0"] + geo["w"])) << (geo["p0"] + geo["w"])
    while True:
        c = rng.integers(0, 1 << geo["w"], size=1 << 16, dtype=np.uint64)
        hit = c[(slot_of(c) == int(slot_of(ik))) & (c != np.uint64(ik))]
        if len(hit):
            return top | int(hit[0]) << geo["p0"]


SCREEN_KINDS = ("cand_and_shared", "only_a", "only_b")
SCREEN_EACH = 4


@functools.lru_cache(maxsize=None)
def screen_collide():
    """plants[kind] = (P, Q): two prefixes of one item in one screen slot.  P is shared with base a by both genomes.
    "cand_and_shared": Q is a candidate (c / g);  "only_a": Q with c in genome 0 only;  "only_b": Q with c in genome 1 only.
    The slot is live every time; the exact join keeps Q in the first kind and nothing in the others"""
    rng = _rng("screen collide")
    codes, flags = _pair(62)
    slot = cc._slots()
    plants = {k: [] for k in SCREEN_KINDS}
    for kind in SCREEN_KINDS:
        for _ in range(SCREEN_EACH):
            p = _prefix(rng)
            q = _same_slot(rng, p, PLANT_GEO)
            plants[kind].append((p, q))
            at_p, at_q = next(slot), next(slot)
            for g in (0, 1):
                _plant(codes[g], at_p, p, A_)
            if kind == "cand_and_shared":
                _plant(codes[0], at_q, q, C_)
                _plant(codes[1], at_q, q, G_)
            else:
                _plant(codes[0 if kind == "only_a" else 1], at_q, q, C_)
    return _finish(codes, 0), flags, plants


TABLE_KINDS = ("low_equal", "high_equal")
TABLE_EACH = 4


def _same_hash(rng, p, geo, kind):
    ik = int(item_key(p, geo))
    top = (p >> (geo["p0"] + geo["w"])) << (geo["p0"] + geo["w"])
    while True:
        if kind == "low_equal":         # the low 32 bits (what k_intersect3t calls the tag) equal, the bits above differ
            c = (rng.integers(0, 1 << (geo["w"] - 32), size=1 << 14, dtype=np.uint64) << np.uint64(32)) | np.uint64(ik & 0xFFFFFFFF)
        else:
            c = np.uint64(ik >> 32 << 32) | rng.integers(0, 1 << 32, size=1 << 14, dtype=np.uint64)
        hit = c[(tab_hash(c) == int(tab_hash(ik))) & (c != np.uint64(ik))]
        if len(hit):
            return top | int(hit[0]) << geo["p0"]
        if kind == "low_equal":
            return None


@functools.lru_cache(maxsize=None)
def table_collide():
    """plants[kind] = (P, Q): two candidates (a / c and g / t) of one item with equal table hash, whose item keys agree in
    their low 32 bits and differ above ("low_equal"), or agree above and differ in the low 32 bits ("high_equal")"""
    rng = _rng("table collide")
    codes, flags = _pair(63)
    slot = cc._slots()
    plants = {k: [] for k in TABLE_KINDS}
    for kind in TABLE_KINDS:
        while len(plants[kind]) < TABLE_EACH:
            p = _prefix(rng)
            q = _same_hash(rng, p, PLANT_GEO, kind)
            if q is None:
                continue
            plants[kind].append((p, q))
            at_p, at_q = next(slot), next(slot)
            _plant(codes[0], at_p, p, A_)
            _plant(codes[1], at_p, p, C_)
            _plant(codes[0], at_q, q, G_)
            _plant(codes[1], at_q, q, T_)
    return _finish(codes, 0), flags, plants


def _scrub(codes, *heads):
    """no window of either strand starts with the five bases of one of `heads` (0 .. 1023) any more"""
    pats = []
    for head in heads:
        pat = np.array([(head >> (8 - 2 * j)) & 3 for j in range(5)], dtype=np.uint8)
        pats += [pat, (3 - pat)[::-1]]
    n = len(codes) - 4
    rng = _rng("scrub")
    while True:
        hit = False
        for p in pats:
            m = np.ones(n, dtype=bool)
            for j in range(5):
                m &= codes[j:n + j] == p[j]
            idx = np.flatnonzero(m)
            if len(idx):
                hit = True
                at = idx + rng.integers(0, 5, size=len(idx))        # (spread over 15 other heads: none of them overflows)
                codes[at] = (codes[at] + rng.integers(1, 4, size=len(idx), dtype=np.uint8)) & 3
        if not hit:
            return


def _bulk(rng, codes, start, stride, count, head, bases, mutate_b=None):
    """`count` windows with random prefixes under `head`, `stride` bases apart from `start` on: genome g shows bases[g]"""
    ps = []
    for i in range(count):
        p = _prefix(rng, head)
        ps.append(p)
        for g, b in enumerate(bases):
            if b is not None:
                _plant(codes[g], start + i * stride, p, b)
    return ps


HEADS = dict(a_empty=0b0001101100, b_empty=0b0110001101, multi=0b1100100111, single=0b1011010001, all_cand=0b0011100101,
             full=0b0111010010, dense=0)
MULTI_B, MULTI_A = 2300, 3
ALL_CAND = 400
FULL = 1300
DENSE_BLOCKS = 1500


@functools.lru_cache(maxsize=None)
def edges():
    """genome 0 is the anchor.  Item HEADS["a_empty"]: the anchor has no key, genome 1 its usual run.  "b_empty": the other way
    round.  "multi": the anchor MULTI_A planted keys, genome 1 more than one batch (MULTI_B planted, MULTI_A of them the
    anchor's with another base: candidates).  "single": one anchor key, a candidate.  The last bucket of the key arrays: windows of
    T that differ in the diagnostic base"""
    rng = _rng("edges")
    codes, flags = _pair(64)
    _scrub(codes[0], HEADS["multi"])
    plants = {}
    plants["multi"] = _bulk(rng, codes, 210_000, 32, MULTI_B, HEADS["multi"], (None, C_))
    for i, p in enumerate(plants["multi"][:MULTI_A]):
        _plant(codes[0], 210_000 + i * 32, p, A_)
    _scrub(codes[0], HEADS["a_empty"], HEADS["single"])          # (behind the bulk: its random windows hold every five bases somewhere)
    _scrub(codes[1], HEADS["b_empty"], HEADS["single"])
    for i, p in enumerate(plants["multi"][:MULTI_A]):       # (once more: a scrub may have touched them)
        _plant(codes[0], 210_000 + i * 32, p, A_)
        _plant(codes[1], 210_000 + i * 32, p, C_)
    p = _prefix(rng, HEADS["single"])
    _plant(codes[0], 10_300, p, G_)
    _plant(codes[1], 10_300, p, T_)
    plants["single"] = [p]
    last = ((1 << 54) - 1) << 10
    _plant(codes[0], 12_300, last, A_)
    _plant(codes[1], 12_300, last, C_)
    plants["last"] = [last]
    return _finish(codes, 0), flags, plants


@functools.lru_cache(maxsize=None)
def many_survivors(count):
    """both genomes lack the item HEADS[...] but for `count` planted windows, genome 1's with the diagnostic base changed: every
    prefix of the item is a candidate.  ALL_CAND fits the exact table, FULL does not: the item is handed on"""
    head = HEADS["all_cand" if count == ALL_CAND else "full"]
    rng = _rng(f"survivors {count}")
    codes, flags = _pair(65)
    for c in codes:
        _scrub(c, head)
    plants = {"all": _bulk(rng, codes, 410_000, 32, count, head, (A_, G_))}
    return _finish(codes, 0), flags, plants


@functools.lru_cache(maxsize=None)
def dense():
    """DENSE_BLOCKS windows under AAAAA on top of the item's usual run, in both genomes, the diagnostic base an ingroup /
    outgroup site: the anchor's run exceeds the slots, the item goes through the host's redo"""
    rng = _rng("dense")
    codes, flags = _pair(66)
    plants = {"dense": _bulk(rng, codes, 610_000, 28, DENSE_BLOCKS, HEADS["dense"], (C_, T_))}
    return _finish(codes, 0), flags, plants


_CENSUS = {}


def census(K, name, texts, flags, ldr=LDR):
    """the oracle's view, once per case: keys per genome, the filtered list, its records"""
    if name not in _CENSUS:
        keys = [K.sorted_keys(t.tobytes(), *ldr) for t in texts]
        cands = K.intersect(keys, flags, *ldr, apply_filter=True)
        recs = np.sort(K.collect(keys, cands, *ldr), order=["key", "genome"])
        for a in keys + [cands, recs]:
            a.setflags(write=False)
        _CENSUS[name] = dict(keys=keys, cands=cands, recs=recs)
    return _CENSUS[name]

"""Seeded genomes for the coarse route (kr_genome_partition + k_coarse_probe) at the shapes where the probe's
loops and seams run: no code of krisp_amd/ but synth.  Every case returns (texts, flags) -- uint8 ASCII texts of four records,
ingroup genomes first -- or (texts, flags, plants) where it writes windows by hand.  The pillars are the first ingroup and
the first outgroup genome (what distributed.sharded_step sorts); the others are the coarse genomes.

tests/test_coarse_cases.py counts, with oracle/kmer_oracle alone, that each case has the shape it is meant to have;
tests/test_gpu_coarse_shapes.py runs them on the device.  The probe's constants are restated here for those counts."""
import functools
import zlib

import numpy as np

from krisp_amd import synth

LDR = (25, 1, 2)
L, D, R = LDR
PMASK = np.uint64(0xFFFFFFFFFFFFFC00)       # key & PMASK = the 54-bit prefix (left | right), MSB-aligned
DIAG_SHIFT = 8                              # the diagnostic base of a key: bits 8..9
RECORDS = 4

# k_coarse.inc
CO_CHUNK = 32768            # keys of one work unit
CO_ITER = 8192              # keys of one iteration of a unit's key loop (2 CO_T CO_UNROLL)
CO_QCAP = 1024              # queued keys of one iteration; more are looked up in place
CO_HB = 1024                # hits a unit gathers in LDS; more go straight to the list
CO_TCAP = 6144              # candidates of one table
CO_MAXG = 24                # genomes of a call on the route
COL_CAPM = 8                # keys of an arena row (kr_collect)

_BASES = "ACGT"


def _rng(name):
    return np.random.default_rng(zlib.crc32(("coarse " + name).encode()))


def _codes(s):
    return np.array([_BASES.index(c) for c in s], dtype=np.uint8)


def _texts(codes):
    return [synth.codes_to_text(c, RECORDS) for c in codes]


def _put(codes, at, window):
    """a window into one genome's codes, inside one record"""
    rl = (len(codes) + RECORDS - 1) // RECORDS
    assert at // rl == (at + len(window) - 1) // rl, "a plant across a record separator"
    codes[at:at + len(window)] = window


def _mutate(rng, codes, mu):
    n = rng.binomial(len(codes), mu)
    pos = rng.integers(0, len(codes), size=n)
    codes[pos] = (codes[pos] + rng.integers(1, 4, size=n, dtype=np.uint8)) & 3


def _family_codes(config, n_in, n_out, length, mu, snp_every=2000):
    anc = synth.ancestor(config, length)
    return ([synth.genome_codes(config, g, length, g < n_in, mu, snp_every, False, anc) for g in range(n_in + n_out)],
            [g < n_in for g in range(n_in + n_out)])


def pillars(flags):
    return flags.index(True), flags.index(False)


def coarse(flags):
    return [g for g in range(len(flags)) if g not in pillars(flags)]


def window(key):
    """a key (prefix | diagnostic base << 8) -> the codes of its window in text order: left, diagnostic base, right"""
    b = [(int(key) >> (62 - 2 * j)) & 3 for j in range(L + R + D)]
    return np.array(b[:L] + b[L + R:] + b[L:L + R], dtype=np.uint8)


def key_of(win):
    """the key of a window given in text order (the forward strand's)"""
    b = list(win[:L]) + list(win[L + D:]) + list(win[L:L + D])
    k = 0
    for j, c in enumerate(b):
        k |= int(c) << (62 - 2 * j)
    return k


# ----------------------------------------------------------------------------
# a. crowded buckets
# ----------------------------------------------------------------------------
SKEW_SEED = 0


@functools.lru_cache(maxsize=None)
def skew(seed=SKEW_SEED):
    """2 in / 2 out of 600 kbp; the ancestor is 70 % A, so top bytes 0 (AAAA...) and 255 (the other strand's TTTT...)
    hold about 0.7^4 of the keys each: several chunks of CO_CHUNK keys, the last one partial"""
    n, mu, every = 600_000, 0.002, 1500
    rng = _rng(f"skew {seed}")
    anc = rng.choice(4, size=n, p=[0.7, 0.1, 0.1, 0.1]).astype(np.uint8)
    sites = np.arange(every // 2, n, every)
    b1 = rng.integers(0, 4, size=len(sites), dtype=np.uint8)
    b2 = (b1 + rng.integers(1, 4, size=len(sites), dtype=np.uint8)) & 3
    codes, flags = [], [True, True, False, False]
    for f in flags:
        c = anc.copy()
        _mutate(rng, c, mu)
        c[sites] = b1 if f else b2
        codes.append(c)
    return _texts(codes), flags


# ----------------------------------------------------------------------------
# b. dense hits in one top byte
# ----------------------------------------------------------------------------
DENSE = [("AAAA", 4000), ("TTTT", 4000), ("AAAA", 7000), ("TTTT", 7000)]


@functools.lru_cache(maxsize=None)
def dense(head, blocks):
    """2 in / 2 out of 300 kbp, uniform; from base 20 000 on `blocks` blocks of 28 bases = `head` + 24 random bases whose base
    25 is an ingroup / outgroup site: every block-aligned window starts with `head` and its diagnostic column is a site"""
    n, mu, at = 300_000, 0.001, 20_000
    rng = _rng(f"dense {head} {blocks}")
    anc = rng.integers(0, 4, size=n, dtype=np.uint8)
    body = rng.integers(0, 4, size=(blocks, 28), dtype=np.uint8)
    body[:, :4] = _codes(head)
    anc[at:at + 28 * blocks] = body.reshape(-1)
    sites = at + 28 * np.arange(blocks) + L
    b1 = rng.integers(0, 4, size=blocks, dtype=np.uint8)
    b2 = (b1 + rng.integers(1, 4, size=blocks, dtype=np.uint8)) & 3
    codes, flags = [], [True, True, False, False]
    for f in flags:
        c = anc.copy()
        _mutate(rng, c, mu)
        c[sites] = b1 if f else b2
        codes.append(c)
    return _texts(codes), flags


# ----------------------------------------------------------------------------
# c. the arena-row boundary
# ----------------------------------------------------------------------------
ROWS = (7, 8, 9)
SAT_LEFT, SAT_RIGHT, SAT_TAIL = "ACGTTGCAAGCTTAGGCATCGATCA", "GT", "CCTGACTG"
SAT_AT, SAT_GAP = 10_000, 36


@functools.lru_cache(maxsize=None)
def rows(copies):
    """the satellite of test_gpu_coarse.py -- a unit of 36 bases whose diagnostic base differs between the sides, in tandem --
    `copies` times in the coarse genomes and once in the pillars: a coarse genome holds `copies` keys under one candidate"""
    codes, flags = _family_codes(38, 2, 2, 300_000, 0.01)
    for g, (c, f) in enumerate(zip(codes, flags)):
        unit = _codes(SAT_LEFT + ("A" if f else "C") + SAT_RIGHT + SAT_TAIL)
        assert len(unit) == SAT_GAP
        for i in range(1 if g in pillars(flags) else copies):
            _put(c, SAT_AT + i * SAT_GAP, unit)
    return _texts(codes), flags


# ----------------------------------------------------------------------------
# plants: windows written by hand, 96 bases apart, clear of the family's own sites and of the record separators
# ----------------------------------------------------------------------------
def _slots(first=0):
    """positions of hand-written windows: eight per 2000 bases, behind the family's site at 1000 (mod 2000)"""
    k = first
    while True:
        yield 2000 * (k // 8) + 1100 + 96 * (k % 8)
        k += 1


def _other(rng, *bases):
    return int(rng.choice([b for b in range(4) if b not in bases]))


# ----------------------------------------------------------------------------
# d. equal hashes
# ----------------------------------------------------------------------------
HASH_C1, HASH_C2 = 0x9E3779B1, 0x85EBCA6B


def co_hash(prefix):
    """co_hash of k_coarse.inc: the table's slot is its top 13 bits, the tag its low 19, the prefilter's bit its top 17"""
    p = np.asarray(prefix, dtype=np.uint64)
    lo = p & np.uint64(0xFFFFFFFF)
    hi = p >> np.uint64(32)
    y = (lo * np.uint64(HASH_C1)) & np.uint64(0xFFFFFFFF)
    return (((hi ^ y) * np.uint64(HASH_C2)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def twin(rng, prefix):
    """another prefix with the same top byte and the same 32-bit hash: (hi, lo) -> (hi ^ lo c ^ lo' c, lo') for a lo' whose
    product with c agrees with lo's in its top byte"""
    hi, lo = prefix >> 32, prefix & 0xFFFFFFFF
    while True:
        lo2 = int(rng.integers(0, 1 << 22)) << 10
        x = ((lo * HASH_C1) ^ (lo2 * HASH_C1)) & 0xFFFFFFFF
        if lo2 != lo and x >> 24 == 0:
            return ((hi ^ x) << 32) | lo2


COLLIDE_PAIRS = 8


@functools.lru_cache(maxsize=None)
def collide():
    """-> texts, flags, plants: plants[kind] = list of (P, P') for the kinds
    "both":   P and P' are candidates (in A / out C and in G / out T), held by every genome
    "lacked": P is a candidate the coarse genomes lack; P' is in every coarse genome and in no pillar
    "alone":  P is a candidate every genome holds (in A / out C); P' is in the coarse genomes only, with the bases exchanged
              (ingroup C, outgroup A): taken for P it would fail P's filter"""
    rng = _rng("collide")
    codes, flags = _family_codes(51, 2, 2, 300_000, 0.001)
    pin, pout = pillars(flags)
    slot = _slots()
    plants = {"both": [], "lacked": [], "alone": []}
    A, C, G, T = 0, 1, 2, 3
    for kind in plants:
        for _ in range(COLLIDE_PAIRS):
            p = (int(rng.integers(0, 1 << 54, dtype=np.uint64)) << 10)
            q = twin(rng, p)
            plants[kind].append((p, q))
            at_p, at_q = next(slot), next(slot)
            for g, (c, f) in enumerate(zip(codes, flags)):
                pillar = g in (pin, pout)
                if kind == "both":
                    _put(c, at_p, window(p | (A if f else C) << DIAG_SHIFT))
                    _put(c, at_q, window(q | (G if f else T) << DIAG_SHIFT))
                elif kind == "lacked":
                    if pillar:
                        _put(c, at_p, window(p | (A if f else C) << DIAG_SHIFT))
                    else:
                        _put(c, at_q, window(q | (A if f else C) << DIAG_SHIFT))
                else:
                    _put(c, at_p, window(p | (A if f else C) << DIAG_SHIFT))
                    if not pillar:
                        _put(c, at_q, window(q | (C if f else A) << DIAG_SHIFT))
    return _texts(codes), flags, plants


# ----------------------------------------------------------------------------
# e. the genome-count boundary
# ----------------------------------------------------------------------------
MANY = (CO_MAXG, CO_MAXG + 1)


@functools.lru_cache(maxsize=None)
def many(n):
    """n genomes of 300 kbp, n // 2 ingroup.  mu = 0.001: a planted site's window survives in all of 25 genomes with
    probability 0.999^(27 x 25) = 0.51, and there are 150 sites (at mu = 0.01 it would be 0.001: an empty list)"""
    codes, flags = _family_codes(52, n // 2, n - n // 2, 300_000, 0.001)
    return _texts(codes), flags


# ----------------------------------------------------------------------------
# f. hand-planted outcomes
# ----------------------------------------------------------------------------
SIDES_KINDS = ("in_shows_out", "in_shows_third", "out_shows_in", "twice", "lacks")
SIDES_EACH = 4


@functools.lru_cache(maxsize=None)
def sides():
    """-> texts, flags, plants: plants[kind] = prefixes of windows every pillar holds, the ingroup pillar with base b1 and the
    outgroup pillar with b2 in the diagnostic column.  What the coarse genomes hold there:
    "in_shows_out":   the ingroup one b2, the outgroup one b2
    "in_shows_third": the ingroup one a third base, the outgroup one b2
    "out_shows_in":   the ingroup one b1, the outgroup one b1
    "twice":          the ingroup one the window twice, with b1 and with a third base (odd plants) or b2 (even plants)
    "lacks":          the ingroup one a substitution inside the left flank"""
    rng = _rng("sides")
    codes, flags = _family_codes(53, 2, 2, 300_000, 0.001)
    pin, pout = pillars(flags)
    cin, cout = coarse(flags)
    assert flags[cin] and not flags[cout]
    slot = _slots()
    plants = {k: [] for k in SIDES_KINDS}
    for kind in SIDES_KINDS:
        for i in range(SIDES_EACH):
            p = int(rng.integers(0, 1 << 54, dtype=np.uint64)) << 10
            plants[kind].append(p)
            b1 = int(rng.integers(0, 4))
            b2 = _other(rng, b1)
            b3 = _other(rng, b1, b2)
            at, at2 = next(slot), next(slot)
            show = {pin: b1, pout: b2, cin: b1, cout: b2}
            if kind == "in_shows_out":
                show[cin] = b2
            elif kind == "in_shows_third":
                show[cin] = b3
            elif kind == "out_shows_in":
                show[cout] = b1
            for g, b in show.items():
                _put(codes[g], at, window(p | b << DIAG_SHIFT))
            if kind == "twice":
                _put(codes[cin], at2, window(p | (b3 if i & 1 else b2) << DIAG_SHIFT))
            elif kind == "lacks":
                codes[cin][at + 11] = (codes[cin][at + 11] + 1) & 3
    return _texts(codes), flags, plants


# ----------------------------------------------------------------------------
# the oracle's view of a case, once per case
# ----------------------------------------------------------------------------
_CENSUS = {}


def census(K, name, texts, flags):
    """-> dict: keys (sorted, per genome), C (the pillars' filtered list), cands / recs (the final list and its records, sorted by
    key and genome), row (the largest multiplicity), hits[g] (the keys of coarse genome g under a prefix of C, sorted)"""
    if name not in _CENSUS:
        keys = [K.sorted_keys(t.tobytes(), L, D, R) for t in texts]
        pin, pout = pillars(flags)
        C = K.intersect([keys[pin], keys[pout]], [True, False], L, D, R, apply_filter=True)
        cands = K.intersect(keys, flags, L, D, R, apply_filter=True)
        recs = np.sort(K.collect(keys, cands, L, D, R), order=["key", "genome"])
        hits = {g: keys[g][np.isin(keys[g] & PMASK, C["prefix"])] for g in coarse(flags)}
        out = dict(keys=keys, C=C, cands=cands, recs=recs, row=int(recs["count"].max()) if len(recs) else 0, hits=hits)
        for a in keys + [C, cands, recs] + list(hits.values()):
            a.setflags(write=False)
        _CENSUS[name] = out
    return _CENSUS[name]


def held(arr, prefixes):
    """per prefix: is it in arr?"""
    return np.isin(np.array(prefixes, dtype=np.uint64), arr)


def sides_kept(K):
    """per kind, per plant of sides(): does the oracle's final list keep the planted prefix?  Recorded, not prescribed: this
    is what the device's list is held to"""
    texts, flags, plants = sides()
    c = census(K, "sides", texts, flags)
    return {kind: [bool(x) for x in held(c["cands"]["prefix"], ps)] for kind, ps in plants.items()}


def buckets(keys):
    """keys per top byte (the 256 buckets pass 1 leaves)"""
    return np.bincount((keys >> np.uint64(56)).astype(np.int64), minlength=256)

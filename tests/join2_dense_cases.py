"""Pairs of genomes for the dense join of k_join2 (k_join2<true>, csrc/j2_queue.inc; DESIGN §3 "k_join2", §10b): one item in
which EVERY key is live, at the sizes where a wave's queue fills, drains at exactly 64, drains twice, and takes a key slot on
top of drained ones.  The helpers are tests/join2_cases.py's, (25, 1, 2) on pairs of 800 kbp; every case returns (texts,
flags, plants).  tests/test_join2_dense_cases.py holds each case to what it claims with the oracle alone,
tests/test_gpu_join2_dense.py runs them on the device.

The item HEAD is scrubbed from both genomes and then holds planted windows only.  Element e of thread t of a workgroup of T
threads is key 2 (t + (e >> 1) T) + (e & 1) of a batch, whatever the order inside the bucket: with every key live the number
of live lanes per wave and key slot follows from the key count alone.  T is the call's, not the item's: PLANT_GEO["T"] = 512
(a batch is 2048 keys), which the device tests read back.

A planted window must bring no second key of the item: no window of either strand that overlaps a plant may start with HEAD's
five bases.  The gaps between the plants are written with a base that can neither begin nor end HEAD or its reverse complement,
so such a window lies inside one plant, whose prefix is drawn again."""
import functools

import numpy as np

import join2_cases as J

A_, C_, G_, T_ = J.A_, J.C_, J.G_, J.T_
HEAD = 0b0100101101                 # CAGTC: first base = last base, so one base (A) fits no end of it or of GACTG
GAP = A_
START, STRIDE = 410_000, 32
T = J.PLANT_GEO["T"]
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 65)
LONG = (500, 700)                   # prefixes of all_live_long: 1500 keys of the other genome are one batch at T = 512, 2100 are two
TWO_BASES = 550                     # prefixes of all_live_two_bases: 1100 anchor keys reach key slots 2 and 3, 550 prefixes fit the table


def _pats(head):
    pat = np.array([(head >> (8 - 2 * j)) & 3 for j in range(5)], dtype=np.uint8)
    return pat, (3 - pat)[::-1]


def heads_at(codes, head):
    """-> (forward, reverse): the positions where HEAD's five bases / their reverse complement stand"""
    out = []
    n = len(codes) - 4
    for p in _pats(head):
        m = np.ones(n, dtype=bool)
        for j in range(5):
            m &= codes[j:n + j] == p[j]
        out.append(np.flatnonzero(m))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _base():
    codes, flags = J._pair(67)
    for c in codes:
        J._scrub(c, HEAD)
    for c in codes:
        c.setflags(write=False)
    return codes, flags


def _plant_exact(rng, codes, count, shows):
    """`count` prefixes under HEAD; genome g shows prefix i with the bases shows[g], one window each, STRIDE apart from START on.
    Nothing else of either strand falls into the item -> the prefixes"""
    pat, rpat = _pats(HEAD)
    assert pat[0] == pat[4] and GAP not in (pat[0], 3 - pat[0])
    wl = J.L + J.D + J.R
    for g in (0, 1):
        nw = count * len(shows[g])
        for k in range(-1, nw):
            codes[g][START + k * STRIDE + wl:START + (k + 1) * STRIDE] = GAP
    ps = [J._prefix(rng, HEAD) for _ in range(count)]
    todo = range(count)
    for _ in range(64):
        for i in todo:
            for g in (0, 1):
                for j, b in enumerate(shows[g]):
                    J._plant(codes[g], START + (i * len(shows[g]) + j) * STRIDE, ps[i], b)
        bad = set()
        for g in (0, 1):
            m = len(shows[g])
            fwd, rev = heads_at(codes[g], HEAD)
            for at, forward in [(int(x), True) for x in fwd] + [(int(x), False) for x in rev]:
                k, off = divmod(at - START, STRIDE)
                assert 0 <= k < count * m and off + 5 <= wl, "a window of the item outside the plants"
                if not (forward and off == 0):
                    bad.add(k // m)
        if not bad:
            return ps
        for i in bad:
            ps[i] = J._prefix(rng, HEAD)
        todo = sorted(bad)
    raise AssertionError("the plants keep bringing stray windows")


@functools.lru_cache(maxsize=None)
def all_live(n):
    """the item HEAD holds exactly n keys of either genome: the same n prefixes, genome 0 (ingroup, the anchor) with a, genome 1
    with g.  Every key of the item is live, every prefix a candidate"""
    base, flags = _base()
    codes = [c.copy() for c in base]
    plants = {"all": _plant_exact(J._rng(f"all live {n}"), codes, n, ((A_,), (G_,)))}
    return J._finish(codes, 0), flags, plants


@functools.lru_cache(maxsize=None)
def all_live_long(count=LONG[0]):
    """the anchor shows `count` prefixes of the item with a, the other genome the same prefixes with c, g and t each: its run is
    3 * count keys, all live; every prefix is a candidate with out_mask {c, g, t}.  With more than 4 T keys the other genome's
    run is walked twice and queued on the second walk, batch after batch"""
    base, flags = _base()
    codes = [c.copy() for c in base]
    plants = {"all": _plant_exact(J._rng(f"all live long {count}"), codes, count, ((A_,), (C_, G_, T_)))}
    return J._finish(codes, 0), flags, plants


@functools.lru_cache(maxsize=None)
def all_live_two_bases(count=TWO_BASES):
    """the anchor shows `count` prefixes of the item with a AND with c, the other genome the same prefixes with g: 2 * count live
    anchor keys -- more than 2 T, so the anchor's key slots 2 and 3 are queued and inserted on top of drained ones -- of `count`
    distinct prefixes, which the exact table (1024 slots) holds with room to spare: the item is joined, not handed on.  Every
    prefix is a candidate with in_mask {a, c}, out_mask {g}"""
    base, flags = _base()
    codes = [c.copy() for c in base]
    plants = {"all": _plant_exact(J._rng(f"all live two bases {count}"), codes, count, ((A_, C_), (G_,)))}
    return J._finish(codes, 0), flags, plants

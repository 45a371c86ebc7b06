"""Seeded candidate sets of the panel pass: (templates, pairs, size, max_sec) per set, small enough that the
reference (panel_reference.select) takes well under a second a set and the device a few seconds for all of them.
test_panel_cases.py holds the conditions the sets must keep (every fate in several sets, a full panel, a short one, a late
member dropping for either cause, the planted verdicts); test_gpu_panel.py runs every set on the device.

A set's primers lie at the template's two ends unless it says otherwise: left = template[0, ln), right = the reverse
complement of template[W - rn, W).  Random sets draw a share of their middles from a small pool of 16-base cores, read on
either strand, so that same-locus drops are frequent; each set's max_sec (thermo.options(max_sec_tm=...)["max_sec"]) lies
inside the spread of its cross figures, so that clashes are frequent too.
"""
import functools
import random

from krisp_amd import thermo

import panel_reference as ref

_COMP = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s[::-1].translate(_COMP)


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _max_sec(celsius):
    return thermo.options(max_sec_tm=celsius)["max_sec"]


def _ends(W, ln, rn):
    return (0, ln, W - rn, rn)


def _random_set(seed, n, size, celsius, W=40, cores=6, share=0.35, lengths=(10, 13)):
    """n candidates of W random bases; a share of them carries one of `cores` 16-base cores in its middle, on either strand"""
    rng = random.Random(seed)
    pool = [_rand(rng, 16) for _ in range(cores)]
    templates, pairs = [], []
    for _ in range(n):
        t = _rand(rng, W)
        if W >= 36 and rng.random() < share:
            core = rng.choice(pool)
            core = _rc(core) if rng.random() < 0.5 else core
            at = rng.randrange(10, W - 10 - 16 + 1)
            t = t[:at] + core + t[at + 16:]
        templates.append(t)
        pairs.append(_ends(W, rng.randint(*lengths), rng.randint(*lengths)))
    return dict(templates=templates, pairs=pairs, size=size, max_sec=_max_sec(celsius))


def _pooled_set(seed, n, size, celsius, W=40, primers=14, cores=5, share=0.5):
    """the set of thousands: primers of 10 bases from a pool (the reference meets few distinct duplexes), middles random or
    around a core"""
    rng = random.Random(seed)
    left = [_rand(rng, 10) for _ in range(primers)]
    right = [_rand(rng, 10) for _ in range(primers)]
    pool = [_rand(rng, 16) for _ in range(cores)]
    templates, pairs = [], []
    for _ in range(n):
        mid = _rand(rng, W - 20)
        if rng.random() < share:
            core = rng.choice(pool)
            core = _rc(core) if rng.random() < 0.5 else core
            at = rng.randrange(0, W - 20 - 16 + 1)
            mid = mid[:at] + core + mid[at + 16:]
        templates.append(rng.choice(left) + mid + _rc(rng.choice(right)))
        pairs.append(_ends(W, 10, 10))
    return dict(templates=templates, pairs=pairs, size=size, max_sec=_max_sec(celsius))


def _w16(seed):
    """W = 16: exactly one window.  Candidates 2 and 5 are candidate 0 as written and reverse-complemented"""
    rng = random.Random(seed)
    t = [_rand(rng, 16) for _ in range(8)]
    t[2] = t[0]
    t[5] = _rc(t[0])
    return dict(templates=t, pairs=[(0, 10, 6, 10)] * 8, size=4, max_sec=_max_sec(-60), plant=[(2, (2, 1)), (5, (2, 1))])


def _w15(seed):
    """W = 15: no window.  Equal templates are not the same locus: they meet as primers only"""
    rng = random.Random(seed)
    t = [_rand(rng, 15) for _ in range(6)]
    t[1] = t[0]
    t[4] = _rc(t[0])
    return dict(templates=t, pairs=[(0, 10, 5, 10)] * 6, size=3, max_sec=_max_sec(-60), never_same=True)


def _w2047(seed):
    """W = 2047: 2032 windows a strand.  Candidate 2 shares candidate 0's LAST window in its own first; candidate 3 shares
    a window of the middle on the reverse strand"""
    rng = random.Random(seed)
    W = 2047
    t = [_rand(rng, W) for _ in range(5)]
    t[2] = t[0][W - 16:] + t[2][16:]
    t[3] = t[3][:1000] + _rc(t[0][500:516]) + t[3][1016:]
    return dict(templates=t, pairs=[_ends(W, 20, 22)] * 5, size=3, max_sec=_max_sec(-20), plant=[(2, (2, 1)), (3, (2, 1))])


def _long_primers(seed):
    """primers of 10 and of 60 bases in one set: 60 x 60 is 119 alignments, a second round of lanes"""
    rng = random.Random(seed)
    W = 130
    shapes = [(60, 60), (10, 60), (60, 10), (10, 10), (60, 60), (35, 60), (60, 60), (10, 60)]
    return dict(templates=[_rand(rng, W) for _ in shapes], pairs=[_ends(W, a, b) for a, b in shapes], size=4, max_sec=_max_sec(-15))


def _locus_plant(seed, kind):
    """[member, the planted candidate, a control] at W = 40 with a max_sec no random pair reaches: what happens to candidate
    1 is the locus rule's doing"""
    rng = random.Random(seed)
    W = 40
    m, c, control = _rand(rng, W), _rand(rng, W), _rand(rng, W)
    want = (2, 1)
    if kind == "first_window":          # the candidate's first window is the member's last
        c = m[W - 16:] + c[16:]
    elif kind == "last_window":         # the candidate's last window is the member's first
        c = c[:W - 16] + m[:16]
    elif kind == "reverse_only":
        c = c[:7] + _rc(m[11:27]) + c[23:]
    elif kind == "fifteen":             # 15 shared bases, the neighbours on both sides differ
        other = {"A": "C", "C": "G", "G": "T", "T": "A"}
        c = c[:11] + other[m[11]] + m[12:27] + other[m[27]] + c[28:]
        want = None
    elif kind == "broken_n":            # the same 16 letters in both, an N among them
        shared = m[12:19] + "N" + m[20:28]
        m = m[:12] + shared + m[28:]
        c = c[:12] + shared + c[28:]
        want = None
    elif kind == "poly":                # a poly-A member, a poly-T candidate: one key, 25 times, and its reverse complement
        m, c = "A" * W, "T" * W
    return dict(templates=[m, c, control], pairs=[_ends(W, 10, 10)] * 3, size=3, max_sec=_max_sec(60), plant=[(1, want)])


def _clash_plant(seed, kind):
    """a candidate whose left primer's 3' end is the reverse complement of a member's left primer's 3' end (8 GC-rich bases),
    under a max_sec between the random pairs' figures and that duplex's"""
    rng = random.Random(seed)
    W = 40
    end = "GCCGTGCC"                    # (its reverse complement GGCACGGC)
    if kind == "end3":                  # [member, clashing, control]
        t = [_rand(rng, W) for _ in range(3)]
        t[0] = t[0][:4] + end + t[0][12:]
        t[1] = t[1][:4] + _rc(end) + t[1][12:]
        plant = [(1, (3, 1))]
    elif kind == "by2":                 # [member 1, member 2, clashing with member 2 only, control]
        t = [_rand(rng, W) for _ in range(4)]
        t[1] = t[1][:4] + end + t[1][12:]
        t[2] = t[2][:4] + _rc(end) + t[2][12:]
        plant = [(1, (1, 2)), (2, (3, 2))]
    else:                               # both the same locus and clashing: the locus rule is asked first
        t = [_rand(rng, W) for _ in range(3)]
        t[0] = t[0][:4] + end + t[0][12:]
        t[1] = t[1][:4] + _rc(end) + t[0][12:28] + t[1][28:]
        plant = [(1, (2, 1))]
    return dict(templates=t, pairs=[_ends(W, 12, 12)] * len(t), size=len(t), max_sec=_max_sec(-30), plant=plant)


def _one_locus(seed):
    rng = random.Random(seed)
    core = _rand(rng, 16)
    t = []
    for i in range(20):
        x = _rand(rng, 40)
        at = rng.randrange(0, 25)
        t.append(x[:at] + (core if i % 3 else _rc(core)) + x[at + 16:])
    return dict(templates=t, pairs=[_ends(40, 10, 11)] * 20, size=8, max_sec=_max_sec(60))


SETS = {
    "random_1": lambda: _random_set(11, 1, 4, -50),
    "random_2": lambda: _random_set(12, 2, 4, -50),
    "random_65": lambda: _random_set(13, 65, 3, -50),
    "random_300": lambda: _random_set(14, 300, 5, -50),
    "pooled_5000": lambda: _pooled_set(15, 5000, 4, -50),
    "w16": lambda: _w16(16),
    "w15": lambda: _w15(17),
    "w2047": lambda: _w2047(18),
    "primers_10_and_60": lambda: _long_primers(19),
    "locus_first_window": lambda: _locus_plant(20, "first_window"),
    "locus_last_window": lambda: _locus_plant(21, "last_window"),
    "locus_reverse_only": lambda: _locus_plant(22, "reverse_only"),
    "locus_fifteen": lambda: _locus_plant(23, "fifteen"),
    "locus_broken_n": lambda: _locus_plant(24, "broken_n"),
    "locus_poly": lambda: _locus_plant(25, "poly"),
    "clash_end3": lambda: _clash_plant(26, "end3"),
    "clash_by2": lambda: _clash_plant(27, "by2"),
    "clash_and_locus": lambda: _clash_plant(28, "both"),
    "size_1": lambda: _random_set(29, 40, 1, -50),
    "size_64_filled": lambda: _pooled_set(30, 220, 64, 0, primers=24, cores=12, share=0.2),
    "size_above_survivors": lambda: _random_set(31, 10, 64, -50),
    "one_locus": lambda: _one_locus(32),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = SETS[name]()
    W = len(c["templates"][0])
    assert all(len(t) == W for t in c["templates"]) and len(c["pairs"]) == len(c["templates"])
    assert all(10 <= n <= 60 and s + n <= W for ls, ln, rs, rn in c["pairs"] for s, n in ((ls, ln), (rs, rn)))
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """the reference's (members, fates) of a set, computed once and shared"""
    c = case(name)
    return ref.select(c["templates"], c["pairs"], c["size"], c["max_sec"])

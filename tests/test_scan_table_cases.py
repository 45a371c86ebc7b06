"""scan_table_cases.py on the CPU: the references against scan_reference and guide_hits_reference on a sub-sample, and a
census of the tables the library builds from the cases -- the layout of seed_table_build and kr_locate_table
(csrc/h_scan.inc, csrc/h_locate.inc) restated in plain Python: that the generators' seeds still give what they were
searched for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_hits_reference as href                                        # noqa: E402
import scan_table_cases as TC                                              # noqa: E402
from scan_reference import ref_locate, ref_near                            # noqa: E402

MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF
LOC_HB = 0x9E3779B1
LOC_BM_LOG = 18


def loc_hash(s):
    h = 0
    for b in bytes(s):
        h = (h * LOC_HB + b) & MASK32
    return h


def loc_mix(hl, hr):
    x = (hl << 32) | hr
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def near_key(piece, h):
    return loc_mix((piece * 0x85EBCA6B + 1) & MASK32, h)


def slots_for(distinct):
    """the least power of two >= max(1024, 2 x distinct keys)"""
    slots = 1024
    while slots < 2 * distinct:
        slots <<= 1
    return slots


def insert(keys, slots):
    """linear probing in the given order -> per key (the slots a probe for it reads, did its chain pass the last slot)"""
    taken = [False] * slots
    out = []
    for key in keys:
        s = key & (slots - 1)
        steps = 1
        while taken[s]:
            s = (s + 1) & (slots - 1)
            steps += 1
        taken[s] = True
        out.append((steps, (key & (slots - 1)) + steps - 1 >= slots))
    return out


def bits_shared(keys):
    """the most keys under one bit of the membership bitmap"""
    return int(np.bincount(np.array([k >> (64 - LOC_BM_LOG) for k in keys], dtype=np.int64)).max())


def near_census(targets, M):
    """the seed table of kr_near_table / kr_guide_hits_table: entry 2 t = target t, 2 t + 1 = its reverse complement; piece j =
    columns [j k / (M + 1), (j + 1) k / (M + 1)); a slot per distinct key, inserted in ascending order
    -> dict(slots, chain, wraps, crowd, bits)"""
    k = targets.shape[1]
    off = [j * k // (M + 1) for j in range(M + 2)]
    under, piece = {}, {}
    for t, row in enumerate(targets):
        for e, x in ((2 * t, row), (2 * t + 1, TC.rc(row))):
            for j in range(M + 1):
                key = near_key(j, loc_hash(x[off[j]:off[j + 1]]))
                under.setdefault(key, []).append(e)
                piece[key] = j
    keys = sorted(under)
    slots = slots_for(len(keys))
    probes = insert(keys, slots)
    return dict(slots=slots, chain=max(s for s, _ in probes), wraps=sum(w for _, w in probes),
                crowd=max(len({e // 2 for e in es}) for es in under.values()), bits=bits_shared(keys), keys=len(keys),
                wrapped=[(e, piece[key]) for key, (_, w) in zip(keys, probes) if w for e in under[key]])


def locate_census(flanks, L):
    """kr_locate_table: a slot per group, inserted in index order, 2 x groups slots at least"""
    keys = [loc_mix(loc_hash(f[:L]), loc_hash(f[L:])) for f in flanks]
    slots = slots_for(len(keys))
    probes = insert(keys, slots)
    return dict(slots=slots, chain=max(s for s, _ in probes), wraps=sum(w for _, w in probes), bits=bits_shared(keys), keys=len(keys),
                wrapped=[g for g, (_, w) in enumerate(probes) if w])


def test_the_hashes_restated_here_on_values_worked_by_hand():
    assert loc_hash(b"") == 0 and loc_hash(b"A") == 65 and loc_hash(b"AC") == (65 * LOC_HB + 67) & MASK32
    assert loc_mix(0, 0) == 0
    # (splitmix64's finalizer of 1)
    assert loc_mix(0, 1) == 0x5692161D100B05E5
    assert near_key(0, 7) == loc_mix(1, 7) and near_key(2, 7) == loc_mix((2 * 0x85EBCA6B + 1) & MASK32, 7)
    assert insert([5, 5, 1023, 1023, 0], 1024) == [(1, False), (2, False), (1, False), (2, True), (2, False)]


@pytest.mark.parametrize("name", list(TC.NEAR_CASES))
def test_census_of_the_near_tables(name):
    M, n, _ = TC.NEAR_CASES[name]
    c = TC.near_case(name)
    assert c["M"] == M and c["targets"].shape == (n, TC.K) and len(c["text"]) == TC.N_TEXT <= TC.TILE + 1000
    s = near_census(c["targets"], M)
    print(name, s)
    assert s["slots"] > 1024
    assert s["chain"] >= 4
    assert s["crowd"] >= 8
    assert s["bits"] >= 2
    if name == "m3":
        # thousands of targets with seed pieces of five letters: nearly every key there is, and the set of all of them has
        # no chain that wraps (no seed gives one); every window of a text finds its bit set
        assert TC.K // (M + 1) == 5 and s["keys"] > 4000 and near_census_of_every_key(5, 4)["wraps"] == 0
    else:
        # a chain that wraps, and a hit that is found through it or not at all: the entry's text planted with a substitution
        # in every piece but the one under the wrapping key
        assert s["wraps"] >= 1 and TC.NEAR_WRAPS[name] in s["wrapped"]
        e, _ = TC.NEAR_WRAPS[name]
        L, D, R = TC.GEOMETRY
        at = slice(TC.PLANT_POS, TC.PLANT_POS + TC.K)
        hits, _ = TC.near_by_packed_words(c["text"][at], L, D, R, c["targets"][e // 2:e // 2 + 1], M)
        assert [tuple(h)[:4] for h in hits.tolist()] == [(0, e & 1, 0, M)]
    assert {m for m, _, _ in TC.NEAR_CASES.values()} == {0, 1, 2, 3}


def near_census_of_every_key(letters, pieces):
    import itertools
    keys = sorted({near_key(j, loc_hash(bytes(p))) for j in range(pieces) for p in itertools.product(b"ACGT", repeat=letters)})
    probes = insert(keys, slots_for(len(keys)))
    return dict(keys=len(keys), wraps=sum(w for _, w in probes))


def test_census_of_the_locate_table():
    c = TC.locate_case()
    L, D, R = TC.GEOMETRY
    assert c["flanks"].shape == (TC.N_GROUPS, L + R) and len(np.unique(c["flanks"], axis=0)) == TC.N_GROUPS
    s = locate_census(c["flanks"], L)
    print(s)
    assert s["slots"] > 1024
    assert s["chain"] >= 4
    assert s["wraps"] >= 1 and TC.LOCATE_WRAPS in s["wrapped"]
    assert s["bits"] >= 2
    at = slice(TC.PLANT_POS, TC.PLANT_POS + TC.K)
    hits = TC.locate_by_dictionary(c["text"][at], L, D, R, c["flanks"])
    assert (0, 0, TC.LOCATE_WRAPS) in [tuple(h) for h in hits.tolist()]


@pytest.mark.parametrize("name", ["m0", "m1", "m2", "m3"])
def test_the_packed_reference_equals_the_definitions_on_a_sub_sample(name):
    """the text's first 9000 bytes and every eighth target: scan_reference.ref_near's list, and
    guide_hits_reference.ref_hits' columns"""
    L, D, R = TC.GEOMETRY
    c = TC.near_case(name)
    M = c["M"]
    text = c["text"][:9000]
    targets = c["targets"][::8]
    want = ref_near(text, L, D, R, False, targets, M)
    got, columns = TC.near_by_packed_words(text, L, D, R, targets, M)
    assert len(want) >= 30 and got.dtype == want.dtype and np.array_equal(got, want)
    hits = href.ref_hits(text.tobytes(), False, [bytes(t).decode("ascii") for t in targets], M)
    assert len(hits) == len(got)
    assert np.array_equal(hits["pos"], got["pos"]) and np.array_equal(hits["guide"], got["target"])
    assert np.array_equal(hits["columns"], columns) and (hits["pam"] == 3).all()
    assert {0, 1} == set(got["strand"].tolist()) and got["flank_mismatches"].max() <= M


def test_the_dictionary_reference_equals_the_definition_on_a_sub_sample():
    L, D, R = TC.GEOMETRY
    c = TC.locate_case()
    text = c["text"][:8000]
    flanks = c["flanks"][::10]
    want = ref_locate(text, L, D, R, False, flanks)
    got = TC.locate_by_dictionary(text, L, D, R, flanks)
    assert len(want) >= 30 and np.array_equal(got, want) and {0, 1} == set(got["strand"].tolist())

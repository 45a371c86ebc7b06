"""A seeded input for k_gather_items: two genomes whose filtered candidate list holds a CHOSEN number of entries in
chosen items of the pipelined intersection.  No code of krisp_amd/ but synth, through the generators of coarse_cases.py.

2 in / 2 out of 300 kbp: 6e5 keys per genome, 512 fine buckets, one bucket per item -- an item is the keys with one value of
their top 9 bits.  All four genomes are one random sequence (no mutation: nothing but the plants survives the filter) with,
from base 20 000 on, blocks of 28 bases as coarse_cases.dense plants them: 8 bases of a group's head, 17 more bases of `left`,
the diagnostic base -- an ingroup / outgroup site --, 2 bases of `right`.  The forward window of a block is a candidate in the
item of its head.  The window of the other strand over the same site starts 22 bases into the NEXT block and reads backwards:
bases 15 .. 22 of every block are T, so that all those candidates begin with AAAAAAAA and fall into item 0.

GROUPS: head -> blocks.  Expected survivors per item: the group's count in the item of its head, all blocks in item 0 (the
first), five in item 511 (the last), every other item none."""
import functools

import numpy as np

import coarse_cases as CC

N_BASES = 300_000
ITEM_BITS = 9
AT = 20_000
GROUPS = (("CCCCAAAA", 63), ("GGGGAAAA", 64), ("CGCGAAAA", 65), ("GCGCAAAA", 1), ("ACACAAAA", 400), ("TTTTTTTT", 5))


def item_of_head(head):
    v = 0
    for c in head[:5]:
        v = v * 4 + "ACGT".index(c)
    return v >> 1                      # the top 9 of the first five bases' 10 bits


def expected_items():
    """item -> survivors: the groups' forward windows, and every block's window of the other strand in item 0"""
    want = {item_of_head(h): n for h, n in GROUPS}
    want[0] = sum(n for _, n in GROUPS)
    return want


def item_histogram(cands, item_bits=ITEM_BITS):
    """survivors per item of a candidate list (the field `prefix`: MSB-aligned)"""
    return np.bincount((cands["prefix"] >> np.uint64(64 - item_bits)).astype(np.int64), minlength=1 << item_bits)


@functools.lru_cache(maxsize=None)
def planted():
    rng = CC._rng("gather planted")
    anc = rng.integers(0, 4, size=N_BASES, dtype=np.uint8)
    heads = [h for h, n in GROUPS for _ in range(n)]
    blocks = len(heads)
    body = rng.integers(0, 4, size=(blocks + 1, 28), dtype=np.uint8)        # (+ 1: what the last block's other strand reads)
    for i, h in enumerate(heads):
        body[i, :8] = CC._codes(h)
    body[:, 15:23] = 3
    assert AT + 28 * (blocks + 1) < N_BASES // CC.RECORDS                   # (inside the first record)
    anc[AT:AT + 28 * (blocks + 1)] = body.reshape(-1)
    sites = AT + 28 * np.arange(blocks) + CC.L
    b1 = rng.integers(0, 4, size=blocks, dtype=np.uint8)
    b2 = (b1 + rng.integers(1, 4, size=blocks, dtype=np.uint8)) & 3
    codes, flags = [], [True, True, False, False]
    for f in flags:
        c = anc.copy()
        c[sites] = b1 if f else b2
        codes.append(c)
    return CC._texts(codes), flags

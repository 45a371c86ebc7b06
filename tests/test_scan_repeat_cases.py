"""scan_repeat_cases.py on the CPU: the identity the long GPU runs rest on -- every list of U * R is the list of the case
text, repeated with the positions shifted by i * len(U) -- asserted with the brute-force references themselves at R = 3, and
what the long cases were chosen for: 1100 tiles, and sites and seed pairs for more than 1024 blocks of the joins and the
extend step."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_bulge_cases as BC                                             # noqa: E402
import guide_bulges_reference as bref                                      # noqa: E402
import scan_repeat_cases as RC                                             # noqa: E402


def identity(lists, text):
    """lists(text) -> name: list; at R = 3"""
    one = lists(text)
    three = lists(RC.long_text(text, 3))
    period = len(RC.unit(text))
    for name, rows in one.items():
        if name == "seps":
            want = RC.repeated_positions(np.concatenate([rows.astype(np.int64), [period - 1]]), 3, period)
        else:
            want = RC.repeated(rows, 3, period)
        assert len(rows) > 0 and three[name].dtype == want.dtype and np.array_equal(three[name], want), name
    return one


def test_the_locate_and_near_lists_of_three_copies():
    c = RC.locate_case()
    assert len(c["text"]) > 3 * RC.TILE and (len(c["text"]) + 1) % 64 != 0
    one = identity(RC.locate_lists, c["text"])
    # the windows' text of the long run passes the million bytes up to which an element-stride launch has a thread per byte
    R = RC.count(c["text"])
    assert R * len(RC.unit(c["text"])) >= RC.MIN_TILES * RC.TILE > (R - 1) * len(RC.unit(c["text"]))
    assert min(len(one["locate"]), len(one["near"])) * c["k"] * R > 4 << 20


def test_the_product_lists_of_three_copies():
    for kind in ("flank", "primer"):
        c = RC.product_case(kind)
        assert (len(c["text"]) + 1) % 64 != 0
        one = identity(lambda text: RC.product_lists(kind, text), c["text"])
        # the join has a block per BLOCK sites: more blocks than k_loc_offsets has threads
        assert len(one["sites"]) * RC.count(c["text"]) > RC.OFFSET_THREADS * RC.BLOCK, kind
        assert len(one["products"]) > 100


def test_the_guide_lists_of_three_copies():
    c = RC.bulge_case()
    assert (c["B"], c["M"]) == (2, 2) and (len(c["text"]) + 1) % 64 != 0
    # the bulged reference over two of the guides (a call is held to MAX_COMPARISONS byte comparisons); the other two lists
    # over all of them
    part = c["guides"][:2]
    assert bref.comparisons(3 * (len(c["text"]) + 1), part, c["B"]) < BC.MAX_COMPARISONS
    identity(lambda text: {"bulges": RC.bulge_lists(text, part)["bulges"]}, c["text"])
    identity(lambda text: RC.bulge_lists(text, bulges=False), c["text"])
    # the extend step has a block per BLOCK seed pairs
    pairs = BC.seed_pairs(c["text"], False, c["guides"], c["M"], c["B"])
    assert pairs * RC.count(c["text"]) > RC.OFFSET_THREADS * RC.BLOCK
    assert len(BC.reference(RC.BULGE_CASE, 0)) > 500

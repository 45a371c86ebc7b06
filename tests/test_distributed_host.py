"""CPU tests of the multi-GPU flow's host pieces (krisp_fasta._distributed_rank and the helpers it shares with the
streaming flow): the batch plan, the touched pairs' candidate list, and the two exchanges every phase goes through --
over two threads whose "communicator" is a barrier in memory.  No GPU."""
import threading

import numpy as np
import pytest

from krisp_amd import _native
from krisp_amd import krisp_fasta as KF


def test_interleave_keeps_both_orders_and_mixes_from_the_start():
    for la in range(5):
        for lb in range(5):
            a, b = [("a", i) for i in range(la)], [("b", i) for i in range(lb)]
            out = KF._interleave(a, b)
            assert sorted(out) == sorted(a + b), (la, lb)
            assert [x for x in out if x[0] == "a"] == a and [x for x in out if x[0] == "b"] == b, (la, lb)
            for p in range(2, len(out) + 1):
                na = sum(1 for x in out[:p] if x[0] == "a")
                if la and lb:
                    assert 0 < na < p, (la, lb, p)                  # one of each in every prefix
                if p <= 2 * min(la, lb):
                    assert abs(2 * na - p) <= 1, (la, lb, p)        # ... in turn while both lists last


def test_batches_cover_the_list_and_the_first_holds_first_min():
    for n in range(1, 8):
        for bsz in range(1, 5):
            for first_min in (1, 2):
                order = list(range(100, 100 + n))
                got = list(KF._batches(order, bsz, first_min))
                assert [g for b in got for g in b] == order, (n, bsz, first_min)
                assert len(got[0]) == min(n, max(bsz, first_min)), (n, bsz, first_min)
                assert all(1 <= len(b) <= bsz for b in got[1:]), (n, bsz, first_min)


def test_first_min_is_two_only_with_both_sides_and_the_filter():
    assert KF._first_min([True, False, True], True) == 2
    assert KF._first_min([True, False], False) == 1
    assert KF._first_min([True, True], True) == 1
    assert KF._first_min([False, False], True) == 1


def test_touched_prefix_cands():
    specials = [[("TTTT", "N", "GG"), ("ACGT", "N", "GG"), ("ACGT", "R", "GG")],      # a plain pair, twice
                [("ARGT", "A", "GG")],                                                # an IUPAC letter in a flank
                [],
                [("AAAA", "Y", "CC"), ("TTTT", "A", "GN")]]
    touched, cands = KF._touched_prefix_cands(specials)
    assert touched == {("TTTT", "GG"), ("ACGT", "GG"), ("ARGT", "GG"), ("AAAA", "CC"), ("TTTT", "GN")}
    assert cands.dtype == _native.CAND
    want = sorted(KF._prefix_key(l, r) for l, r in (("TTTT", "GG"), ("ACGT", "GG"), ("AAAA", "CC")))
    assert cands["prefix"].tolist() == want
    assert want[0] == (1 << 54) | (1 << 52)             # AAAACC: two bits a base from the top, A C G T = 0 1 2 3
    assert not cands["in_mask"].any() and not cands["out_mask"].any()
    for none_plain in ([[("ARGT", "A", "GG")], [("ACGT", "C", "NN")]], [[], []], []):
        touched, cands = KF._touched_prefix_cands(none_plain)
        assert touched == {(l, r) for sp in none_plain for l, _, r in sp}
        assert cands.dtype == _native.CAND and len(cands) == 0


class _Rank:
    """one of two ranks in one process: the collectives meet at a barrier and read each other's slot"""

    def __init__(self, shared, rank):
        self.shared, self.rank = shared, rank
        self.allreduces = self.allgathers = 0

    def _exchange(self, mine):
        barrier, slots = self.shared
        slots[self.rank] = mine
        barrier.wait(timeout=10)
        got = list(slots)
        barrier.wait(timeout=10)                # (nobody writes its next value before all have read this one)
        return got

    def comm_allreduce(self, values, op):
        assert op == "max"
        self.allreduces += 1
        return [max(col) for col in zip(*self._exchange([float(v) for v in values]))]

    def comm_allgather(self, blob):
        self.allgathers += 1
        return self._exchange(bytes(blob))


def _on_two_ranks(body):
    """body(engine, rank) on two threads -> (engines, what each returned or raised)"""
    shared = (threading.Barrier(2), [None, None])
    engines = [_Rank(shared, r) for r in range(2)]
    out = [None, None]

    def work(r):
        try:
            out[r] = body(engines[r], r)
        except BaseException as e:  # noqa: BLE001
            out[r] = e
    threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return engines, out


def test_together_returns_each_ranks_own_value():
    engines, out = _on_two_ranks(lambda eng, r: KF._together(eng, r, lambda: ("value of", r)))
    assert out == [("value of", 0), ("value of", 1)]
    assert [e.allreduces for e in engines] == [1, 1] and [e.allgathers for e in engines] == [0, 0]


def test_together_stops_every_rank_when_one_raises():
    boom = ValueError("rank 1 cannot read its file")

    def fn(r):
        if r == 1:
            raise boom
        return r
    engines, out = _on_two_ranks(lambda eng, r: KF._together(eng, r, lambda: fn(r)))
    assert out[1] is boom
    assert type(out[0]) is KF.PeerFailed
    assert [e.allreduces for e in engines] == [1, 1] and [e.allgathers for e in engines] == [0, 0]


# what each of two ranks sends in the flow's three exchanges, and what the call site rebuilds from all of them
_ALPHABETS = [{0: False, 2: True}, {1: True, 3: False}]
_SPECIALS = [{0: [("ACGR", "A", "TT"), ("AC", "", "N")], 2: []}, {1: [("NNNN", "ACGT", "GG")], 3: []}]
_MEMBERS = [[[["ACGT", "GG"], ["ACGT", "A", "GG"], 0, 2], [["ACGT", "GG"], ["ACGT", "C", "GG"], 2, 1]],
            [[["ACGT", "GG"], ["ACGT", "A", "GG"], 1, 1]]]


@pytest.mark.parametrize("sent, rebuilt", [
    (_ALPHABETS, lambda parts: {int(g): r for part in parts for g, r in part.items()}
        == {0: False, 1: True, 2: True, 3: False}),
    (_SPECIALS, lambda parts: {int(g): [tuple(w) for w in sp] for part in parts for g, sp in part.items()}
        == {**_SPECIALS[0], **_SPECIALS[1]}),
    (_MEMBERS, lambda parts: [[(tuple(P), tuple(seq), g, cnt) for P, seq, g, cnt in part] for part in parts]
        == [[(tuple(P), tuple(seq), g, cnt) for P, seq, g, cnt in part] for part in _MEMBERS]),
], ids=["alphabets", "specials", "wide probe members"])
def test_allgather_json_gives_every_rank_every_payload_in_rank_order(sent, rebuilt):
    engines, out = _on_two_ranks(lambda eng, r: KF._allgather_json(eng, sent[r]))
    assert out[0] == out[1] and len(out[0]) == 2
    assert rebuilt(out[0])
    for part in out[0]:         # plain data came back: bools stay bools, numbers stay ints
        flat = part.values() if isinstance(part, dict) else [x for row in part for x in row[2:]]
        assert all(type(v) in (bool, int, list) for v in flat)
    assert [e.allgathers for e in engines] == [1, 1] and [e.allreduces for e in engines] == [0, 0]

"""The dense join of the two-genome kernel (k_join2<true>, KR_OPT_JOIN2_DENSE; csrc/j2_queue.inc): the screen slots kept in
registers, the live keys queued per wave and joined with full lanes.

The rule of every test: candidates (prefix, in_mask, out_mask) in order and the records of kr_collect are equal to
oracle/kmer_oracle.c and BIT-IDENTICAL between KR_OPT_JOIN2_DENSE = 1, = 0 and KR_JOIN2 = 0, with the grid capped at 1 and 3
workgroups (one workgroup walks item after item) and over three calls on one engine.  The cases are tests/join2_dense_cases.py's
(every key of one item live, at the sizes where a wave's queue fills and drains; tests/test_join2_dense_cases.py holds them
without a GPU) and tests/join2_cases.py's.  A few seconds per test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join2_cases as J                                                    # noqa: E402
import join2_dense_cases as JD                                             # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


@pytest.fixture(autouse=True)
def _one_sort_unit(monkeypatch):
    """the route's geometry is that of ONE sort unit; the switches of the route are each test's own"""
    for v in ("KR_SLICE_BASES", "KR_JOIN2", "KR_JOIN2_DENSE", "KR_JOIN2_GRID", "KR_ISECT_FMT", "KR_ISECT_KERNEL", "KR_FUSE_ANCHOR"):
        monkeypatch.delenv(v, raising=False)


def _run(N, monkeypatch, texts, flags, join2=1, dense=None, dense_env=None, grid=None, calls=1):
    """one engine made under KR_JOIN2 = join2 (and KR_JOIN2_GRID, KR_JOIN2_DENSE = dense_env), KR_OPT_JOIN2_DENSE set to `dense`
    where given -> dict(cands, recs, isect)"""
    monkeypatch.setenv("KR_JOIN2", str(join2))
    for name, v in (("KR_JOIN2_GRID", grid), ("KR_JOIN2_DENSE", dense_env)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    ids = list(range(len(texts)))
    out = dict(cands=[], recs=[])
    with N.Engine() as e:
        if dense is not None:
            e.set_option(N.OPT_JOIN2_DENSE, dense)
        e.set_params(*J.LDR, max_bases=max(len(t) for t in texts))
        for g, t in zip(ids, texts):
            e.upload(g, t)
        for _ in range(calls):
            for g in ids:
                e.sort(g)
            n = e.intersect(ids, flags, apply_filter=True)
            recs = e.collect(ids)
            out["cands"].append(e.cands().copy())
            out["recs"].append(np.sort(recs, order=["key", "genome"]))
            assert n == len(out["cands"][-1])
        out["isect"] = e.debug_isect()
    return out


def _same(ref, x, y, what):
    for a, b in zip(x["cands"], y["cands"] * len(x["cands"])):
        assert np.array_equal(a, b), "candidates differ: " + what
    for a, b in zip(x["recs"], y["recs"] * len(x["recs"])):
        assert np.array_equal(a, b), "records differ: " + what
    if ref is not None:
        for a in x["cands"]:
            assert len(a) == len(ref["cands"])
            for f in ("prefix", "in_mask", "out_mask"):
                assert np.array_equal(a[f], ref["cands"][f]), (what, f)
        for a in x["recs"]:
            assert np.array_equal(a, ref["recs"]), what


def _all_ways(N, K, monkeypatch, name, texts, flags, handed_on=None):
    """the default, three calls, against the oracle; the switch at 0, the n-way kernel, grids of 1 and 3 against the default
    -> the default's run"""
    ref = J.census(K, name, texts, flags)
    on = _run(N, monkeypatch, texts, flags, calls=3)
    _same(ref, on, on, "the default against the oracle")
    assert on["isect"]["join2_launches"] >= 3 and on["isect"]["heads32"] == 1 and on["isect"]["threads"] == JD.T, on["isect"]
    off = _run(N, monkeypatch, texts, flags, dense=0)
    assert off["isect"]["join2_launches"] >= 1
    _same(ref, off, on, "KR_OPT_JOIN2_DENSE = 0")
    nway = _run(N, monkeypatch, texts, flags, join2=0)
    assert nway["isect"]["join2_launches"] == 0 and nway["isect"]["join2_handed_on"] == 0
    _same(ref, nway, on, "KR_JOIN2 = 0")
    for grid in (1, 3):
        few = _run(N, monkeypatch, texts, flags, grid=grid)
        assert few["isect"]["join2_launches"] >= 1
        _same(ref, few, on, f"KR_JOIN2_GRID = {grid}")
    print(name, "handed on:", on["isect"]["join2_handed_on"], off["isect"]["join2_handed_on"])
    if handed_on is not None:
        for r in (on, off):
            assert (r["isect"]["join2_handed_on"] > 0) == handed_on, r["isect"]
    return on


@pytest.mark.parametrize("n", JD.SIZES)
def test_every_key_of_an_item_live(N, K, monkeypatch, n):
    """fills of 1, 2, 63; a drain at exactly 64 with nothing and with one key left; two drains; a second wave; with 2 T keys and
    more the key slots 2 and 3 -- and more distinct live prefixes than the exact table has slots (n > 1024): the drain flags the
    item, the redo answers (1023 and 1024 fill the table to the brim: either way is right, the result is the oracle's)"""
    texts, flags, plants = JD.all_live(n)
    handed_on = False if n <= 129 else (True if n > (1 << J.J2_TAB_LOG) else None)
    on = _all_ways(N, K, monkeypatch, f"all live {n}", texts, flags, handed_on)
    assert np.isin(np.array(plants["all"], dtype=np.uint64), on["cands"][0]["prefix"]).all()


@pytest.mark.parametrize("count", JD.LONG)
def test_every_key_live_in_a_long_run_of_the_other_genome(N, K, monkeypatch, count):
    """500 prefixes: the other genome's 1500 keys fill key slots 0 to 2 of one batch, every wave drains again and again;
    700: 2100 keys, more than a batch -- walked twice, queued and joined on the second walk, batch after batch"""
    texts, flags, plants = JD.all_live_long(count)
    on = _all_ways(N, K, monkeypatch, f"all live long {count}", texts, flags, False if count == JD.LONG[0] else None)
    c = on["cands"][0]
    row = c[np.isin(c["prefix"], np.array(plants["all"], dtype=np.uint64))]
    assert len(row) == count and np.all(row["in_mask"] == 1) and np.all(row["out_mask"] == 0b1110)


def test_the_anchors_key_slots_2_and_3_are_joined(N, K, monkeypatch):
    """1100 live anchor keys of 550 prefixes (each with a and c; the other genome shows g): the anchor's key slots 2 and 3 come in
    on top of drained slots, pass through the drain and the insert and reach the survivors -- the table holds 550 prefixes at a
    load of 0.54, far from a run of 64 taken slots, so the item is NOT handed on and the result is the kernel's own"""
    texts, flags, plants = JD.all_live_two_bases()
    on = _all_ways(N, K, monkeypatch, "all live two bases", texts, flags, False)
    c = on["cands"][0]
    row = c[np.isin(c["prefix"], np.array(plants["all"], dtype=np.uint64))]
    assert len(row) == JD.TWO_BASES and np.all(row["in_mask"] == 0b0011) and np.all(row["out_mask"] == 0b0100)


@pytest.mark.parametrize("dense", [1, 0])
def test_a_full_table_hands_the_item_on(N, K, monkeypatch, dense):
    """more live prefixes than the exact table holds: the drain (the key slot's own insert with the switch at 0) sets the full
    flag, the item is handed on and counted, the redo answers"""
    texts, flags, plants = J.many_survivors(J.FULL)
    ref = J.census(K, f"survivors {J.FULL}", texts, flags)
    r = _run(N, monkeypatch, texts, flags, dense=dense)
    _same(ref, r, r, f"KR_OPT_JOIN2_DENSE = {dense}")
    assert r["isect"]["join2_launches"] >= 1 and r["isect"]["join2_handed_on"] > 0, r["isect"]
    assert np.isin(np.array(plants["all"], dtype=np.uint64), r["cands"][0]["prefix"]).sum() > J.FULL * 0.9


@pytest.mark.parametrize("case", ["trap", "screen_collide", "table_collide"])
def test_the_switch_at_zero_keeps_the_old_path(N, K, monkeypatch, case):
    """the overlap trap, two prefixes in one screen slot and two in one table slot through k_join2<false> (with the default
    tests/test_gpu_join2.py runs them), by the environment as a user would set it"""
    texts, flags, _ = {"trap": lambda: J.trap(0), "screen_collide": J.screen_collide, "table_collide": J.table_collide}[case]()
    name = {"trap": "trap 0", "screen_collide": "screen collide", "table_collide": "table collide"}[case]
    ref = J.census(K, name, texts, flags)
    off = _run(N, monkeypatch, texts, flags, dense_env=0)
    on = _run(N, monkeypatch, texts, flags, dense_env=1)
    _same(ref, off, on, "KR_JOIN2_DENSE = 0")
    assert off["isect"]["join2_launches"] >= 1 and off["isect"]["join2_handed_on"] == 0, off["isect"]


def test_the_option_takes_0_and_1_only(N):
    with N.Engine() as e:
        e.set_option(N.OPT_JOIN2_DENSE, 0)
        e.set_option(N.OPT_JOIN2_DENSE, 1)
        with pytest.raises(Exception):
            e.set_option(N.OPT_JOIN2_DENSE, 2)

"""k_coarse_probe at the shapes where its loops and seams run: the cases of coarse_cases.py, whose census
test_coarse_cases.py counts on the host.  test_gpu_coarse.py asks which calls take the route; its uniform genomes of 300 kbp
give the probe one work unit and one key-loop iteration per top byte and fewer units than workgroups.  Here a top byte has
several chunks (skew), a unit more hits than the queue and the hit buffer hold and a table its full fill (dense), a workgroup
many units over several tables (KR_COARSE_GRID), a hash chain equal tags (collide), and the limits -- hit list, arena row,
genome count -- are tried from both sides.

The rule of every test is coarse_run.py's: candidates in order, records in kr_fetch order and counts bit-identical between
KR_OPT_COARSE_REST = 1 and 0 and equal to the oracle; and debug_lazy()'s `coarse` / `coarse_promoted` as the case says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import coarse_run                                                           # noqa: E402
from coarse_run import _ab                                                  # noqa: E402

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


@pytest.fixture(scope="module")
def D():
    from krisp_amd import distributed
    return distributed


def _case(K, name, texts, flags):
    """the case's census; its final list and records are the reference of coarse_run._ab under the same name"""
    c = CC.census(K, name, texts, flags)
    coarse_run._REF.setdefault(name, (c["keys"], c["cands"], c["recs"]))
    return c


def _knobs(monkeypatch, grid=None, tcap=None, hitcap=None):
    for name, v in (("KR_COARSE_GRID", grid), ("KR_COARSE_TCAP", tcap), ("KR_COARSE_HITCAP", hitcap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


# ----------------------------------------------------------------------------
# skew: several chunks per top byte
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid,tcap,lanes", [(None, None, None), (1, None, None), (3, None, None), (7, None, None),
                                             (None, 50, None), (3, 50, None), (None, 1, None),
                                             (None, None, 1), (None, None, 3)])
def test_skew(N, K, D, monkeypatch, grid, tcap, lanes):
    """two top bytes of five chunks, the last partial, one bucket at an odd and one at an even base.  Grid 1 / 3 / 7: one
    workgroup walks all units, or a third or a seventh of them -- across top bytes, through every chunk of one table, with the
    seams between workgroups inside a top byte.  KR_COARSE_TCAP = 50: rounds x chunks, one table over a byte's chunks and the
    next round's table behind it; = 1: thousands of units, many per workgroup at the full grid."""
    texts, flags = CC.skew()
    _case(K, "skew", texts, flags)
    _knobs(monkeypatch, grid=grid, tcap=tcap)
    plain = (grid, tcap, lanes) == (None, None, None)
    on = _ab(N, K, "skew", texts, flags, step=D.sharded_step, lanes=lanes, coarse_expected=2, promoted_expected=0,
             keys_of=(3,) if plain else ())
    assert len(on["cands"][0]) > 100
    if plain:
        assert on["lazy_after_keys"]["coarse_promoted"] == 1


# ----------------------------------------------------------------------------
# dense: the queue, the hit buffer and the table past their capacities
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("head,blocks,grid", [(h, b, None) for h, b in CC.DENSE] + [("AAAA", 7000, 1), ("TTTT", 7000, 1)])
def test_dense(N, K, D, monkeypatch, head, blocks, grid):
    """4000 blocks: the bucket's first iteration holds more than CO_QCAP keys that pass the prefilter (looked up in place) and
    the unit more than CO_HB hits (straight to the list).  7000: more than CO_TCAP candidates in the byte -- two rounds, the
    first at the table's full fill -- and two iterations per unit; with one workgroup both rounds' tables are built by it.
    Top byte 255 ends the key array: the unit's aligned loads read up to a key behind the genome's last."""
    texts, flags = CC.dense(head, blocks)
    name = f"dense_{head}_{blocks}"
    _case(K, name, texts, flags)
    _knobs(monkeypatch, grid=grid)
    _ab(N, K, name, texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)


@pytest.mark.parametrize("short", [0, 1])
def test_hit_list_boundary(N, K, D, monkeypatch, short):
    """H = the longest hit list of the case: the keys of a coarse genome under a prefix of the pillars' list.  A list of H keys
    holds them; one of H - 1 overflows, and the genomes are sorted fine"""
    texts, flags = CC.dense("AAAA", 4000)
    c = _case(K, "dense_AAAA_4000", texts, flags)
    H = max(len(h) for h in c["hits"].values())
    assert H > CC.CO_HB
    _knobs(monkeypatch, hitcap=H - short)
    _ab(N, K, "dense_AAAA_4000", texts, flags, step=D.sharded_step, coarse_expected=0 if short else 2,
        promoted_expected=2 if short else 0)


# ----------------------------------------------------------------------------
# rows: an arena row of 7, 8 and 9 keys
# ----------------------------------------------------------------------------
def test_rows_boundary(N, K, D):
    """COL_CAPM = 8 keys fit an arena row: 7 and 8 copies come from the hit lists, 9 promote the coarse genomes"""
    got = {}
    for copies in CC.ROWS:
        texts, flags = CC.rows(copies)
        c = _case(K, f"rows_{copies}", texts, flags)
        assert c["row"] == copies
        on = _ab(N, K, f"rows_{copies}", texts, flags, step=D.sharded_step, coarse_expected=2,
                 promoted_expected=2 if copies > CC.COL_CAPM else 0)
        assert int(on["recs"][0]["count"].max()) == copies
        got[copies] = on
    first = got[CC.ROWS[0]]
    for copies in CC.ROWS[1:]:
        assert np.array_equal(got[copies]["cands"][0], first["cands"][0])
        assert np.array_equal(got[copies]["recs"][0]["key"], first["recs"][0]["key"])
        assert np.array_equal(got[copies]["recs"][0]["genome"], first["recs"][0]["genome"])


# ----------------------------------------------------------------------------
# collide: equal tags in one hash chain
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [None, 1])
def test_collide(N, K, D, monkeypatch, grid):
    """pairs of prefixes with one top byte and one 32-bit co_hash: a look-up that stopped at the tag would take one for the other"""
    texts, flags, plants = CC.collide()
    _case(K, "collide", texts, flags)
    _knobs(monkeypatch, grid=grid)
    on = _ab(N, K, "collide", texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)
    cands, recs = on["cands"][0], on["recs"][0]
    assert CC.held(cands["prefix"], [x for pq in plants["both"] for x in pq]).all()
    # a candidate the coarse genomes lack, its twin in all of them: it falls
    assert not CC.held(cands["prefix"], [p for p, _ in plants["lacked"]]).any()
    # a candidate all hold, its twin in the coarse genomes with the sides' bases exchanged: it stays, with its own masks
    mine = cands[np.isin(cands["prefix"], np.array([p for p, _ in plants["alone"]], dtype=np.uint64))]
    assert len(mine) == len(plants["alone"])
    assert np.all(mine["in_mask"] == 1) and np.all(mine["out_mask"] == 2)
    # ... and no record of a twin that is no candidate
    twins = [q for kind in ("lacked", "alone") for _, q in plants[kind]]
    assert not CC.held(recs["key"] & CC.PMASK, twins).any()


# ----------------------------------------------------------------------------
# many: 24 genomes take the route, 25 do not
# ----------------------------------------------------------------------------
def test_24_genomes_take_the_route(N, K, D):
    texts, flags = CC.many(CC.CO_MAXG)
    _case(K, f"many_{CC.CO_MAXG}", texts, flags)
    on = _ab(N, K, f"many_{CC.CO_MAXG}", texts, flags, step=D.sharded_step, coarse_expected=CC.CO_MAXG - 2, promoted_expected=0)
    assert len(on["cands"][0]) > 0


def test_25_genomes_promote(N, K):
    texts, flags = CC.many(CC.CO_MAXG + 1)
    _case(K, f"many_{CC.CO_MAXG + 1}", texts, flags)
    on = _ab(N, K, f"many_{CC.CO_MAXG + 1}", texts, flags, coarse_ids=set(CC.coarse(flags)), coarse_expected=0,
             promoted_expected=CC.CO_MAXG - 1)
    assert len(on["cands"][0]) > 0


# ----------------------------------------------------------------------------
# sides: what a coarse genome shows at a site the pillars disagree on
# ----------------------------------------------------------------------------
def _sides_check(K, cands):
    _, _, plants = CC.sides()
    kept = CC.sides_kept(K)
    for kind, ps in plants.items():
        assert [bool(x) for x in CC.held(cands["prefix"], ps)] == kept[kind], kind


def test_sides(N, K, D):
    texts, flags, _ = CC.sides()
    _case(K, "sides", texts, flags)
    on = _ab(N, K, "sides", texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)
    _sides_check(K, on["cands"][0])


def test_sides_coarse_genomes_first(N, K):
    """the coarse genomes in front of the pillars in `ids`: state bits, sides and the records' genome index follow the
    position in the call, not the state of the genome"""
    texts, flags, _ = CC.sides()
    order = CC.coarse(flags) + list(CC.pillars(flags))
    texts, flags = [texts[g] for g in order], [flags[g] for g in order]
    on = _ab(N, K, "sides_coarse_first", texts, flags, coarse_ids={0, 1}, coarse_expected=2, promoted_expected=0)
    _sides_check(K, on["cands"][0])
    keys, cands, recs = coarse_run._REF["sides_coarse_first"]
    assert np.array_equal(np.sort(on["recs"][0], order=["key", "genome"]),
                          np.sort(K.collect(keys, cands, *CC.LDR), order=["key", "genome"]))
    assert set(on["recs"][0]["genome"]) == {0, 1, 2, 3}


# ----------------------------------------------------------------------------
# one engine, several calls
# ----------------------------------------------------------------------------
def test_one_engine_several_calls(N, K):
    """genomes 1 and 3 of skew partitioned once; then three calls with no sort in between -- the flags as given, the sides
    exchanged, and genomes 0, 2, 3 only (genome 3 is coarse genome 0 of that call, not 1).  State words, hit counts and
    hits_valid belong to one call: each answer is its own oracle's.  No call promotes: every one has a sorted genome of each
    side, the filter, one diagnostic column"""
    texts, flags = CC.skew()
    keys = _case(K, "skew", texts, flags)["keys"]
    calls = [([0, 1, 2, 3], flags), ([0, 1, 2, 3], [not f for f in flags]), ([0, 2, 3], [True, False, False])]
    want = []
    for ids, fl in calls:
        ks = [keys[g] for g in ids]
        cands = K.intersect(ks, fl, *CC.LDR, apply_filter=True)
        recs = K.collect(ks, cands, *CC.LDR)
        recs["genome"] = np.array(ids, dtype=np.uint32)[recs["genome"]]             # (a record names its genome by id)
        want.append((cands, np.sort(recs, order=["key", "genome"])))
    assert len(want[0][0]) > 100 and len(want[2][0]) > len(want[0][0])
    assert not np.array_equal(want[0][0]["in_mask"], want[1][0]["in_mask"])
    got = {}
    for rest in (1, 0):
        with N.Engine() as e:
            e.set_option(N.OPT_COARSE_REST, rest)
            e.set_params(*CC.LDR, max_bases=max(len(t) for t in texts))
            for g, t in enumerate(texts):
                e.upload(g, t)
            for g in range(4):
                (e.partition if g in (1, 3) else e.sort)(g)
            for (ids, fl), (cands, recs) in zip(calls, want):
                assert e.intersect(ids, fl) == len(cands)
                c = e.cands().copy()
                for f in ("prefix", "in_mask", "out_mask"):
                    assert np.array_equal(c[f], cands[f]), (ids, fl, f)
                r = e.collect(ids).copy()
                assert np.array_equal(np.sort(r, order=["key", "genome"]), recs), (ids, fl)
                got.setdefault(rest, []).append((c, r))
            lazy = e.debug_lazy()
            assert (lazy["coarse"], lazy["coarse_promoted"]) == ((5, 0) if rest else (0, 0)), lazy
    for (c1, r1), (c0, r0) in zip(got[1], got[0]):
        assert np.array_equal(c1, c0) and np.array_equal(r1, r0)

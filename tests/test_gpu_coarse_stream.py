"""k_coarse_probe as ONE launch over all coarse genomes of a call, its key loop software-pipelined: the cases of
coarse_stream_cases.py, whose census test_coarse_stream_cases.py counts on the host.  Several genomes of different lengths
share a table; buckets sit at the edges of the loop's iteration and a genome's last bucket ends on one; a unit's hits sit at
the edges of the queue; different coarse genomes of one call show different outcomes for one candidate; one of three hit
lists overflows; one engine runs three steps.

The rule of every test is coarse_run.py's: candidates in order, records in kr_fetch order and counts bit-identical between
KR_OPT_COARSE_REST = 1 and 0 and equal to the oracle; and debug_lazy()'s `coarse` / `coarse_promoted` as the case says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import coarse_run                                                           # noqa: E402
import coarse_stream_cases as SC                                            # noqa: E402
from coarse_run import _ab                                                  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [None, 1, 3]


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
# several genomes per table
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("tcap", [None, 50])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ncoarse", SC.MULTI)
def test_multi(N, K, D, monkeypatch, ncoarse, grid, tcap):
    """3 and 5 coarse genomes of 4, 2, (5, 3,) 1 chunks in top byte 0, the last a mini genome shorter than one iteration and
    without a key in most top bytes that have candidates.  KR_COARSE_TCAP = 50: rounds x genomes x chunks all vary.  Grid 1 /
    3: one workgroup walks every genome's units of every table, or a third of them with the seams inside a table"""
    texts, flags, plants = SC.multi(ncoarse)
    name = f"multi_{ncoarse}"
    _case(K, name, texts, flags)
    _knobs(monkeypatch, grid=grid, tcap=tcap)
    on = _ab(N, K, name, texts, flags, step=D.sharded_step, coarse_expected=ncoarse, promoted_expected=0,
             keys_of=(1,) if (grid, tcap) == (None, None) else ())
    assert np.array_equal(np.sort(on["cands"][0]["prefix"]), np.sort(SC.prefixes(plants)))


# ----------------------------------------------------------------------------
# prefetch edges
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_edges(N, K, D, monkeypatch, grid):
    """genome 1's buckets of 1, one iteration - 1, one iteration + 1, two iterations + 1 and -- the last of its key array --
    exactly one iteration; odd and even bases; every unit of genome 1 is followed by a unit of genome 3"""
    texts, flags, plants = SC.edges()
    _case(K, "edges", texts, flags)
    _knobs(monkeypatch, grid=grid)
    on = _ab(N, K, "edges", texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0,
             keys_of=(1,) if grid is None else ())
    assert np.array_equal(np.sort(on["cands"][0]["prefix"]), np.sort(SC.prefixes(plants)))


# ----------------------------------------------------------------------------
# the queue
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("hits", SC.QUEUE)
def test_queue(N, K, D, monkeypatch, hits, grid):
    """a unit of the queue's capacity - 1, = and + 1 keys, every one a true hit: the last overruns the queue, and the unit is
    read again and looked up in place"""
    texts, flags, plants = SC.queue(hits)
    name = f"queue_{hits}"
    _case(K, name, texts, flags)
    _knobs(monkeypatch, grid=grid)
    on = _ab(N, K, name, texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)
    assert len(on["cands"][0]) == hits


# ----------------------------------------------------------------------------
# sides across genomes
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_spread(N, K, D, monkeypatch, grid):
    """four coarse genomes; each planted candidate deviates in ONE of them.  A presence bit or a side written to a neighbour's
    bits of the state word changes which candidates stay"""
    texts, flags, plants = SC.spread()
    _case(K, "spread", texts, flags)
    _knobs(monkeypatch, grid=grid)
    on = _ab(N, K, "spread", texts, flags, step=D.sharded_step, coarse_expected=4, promoted_expected=0)
    kept = SC.spread_kept(K)
    for kind, ps in plants.items():
        assert [bool(x) for x in CC.held(on["cands"][0]["prefix"], [p for p, _ in ps])] == kept[kind], kind


# ----------------------------------------------------------------------------
# one list overflows
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_one_list_overflows(N, K, D, monkeypatch, grid):
    """KR_COARSE_HITCAP = the second longest hit list of three: the longest alone overflows, and the whole call promotes"""
    texts, flags, _ = SC.multi(3)
    c = _case(K, "multi_3", texts, flags)
    nh = sorted(len(h) for h in c["hits"].values())
    assert nh[-1] > nh[-2]
    _knobs(monkeypatch, grid=grid, hitcap=nh[-2])
    _ab(N, K, "multi_3", texts, flags, step=D.sharded_step, coarse_expected=0, promoted_expected=3)


def test_no_list_overflows_at_the_longest(N, K, D, monkeypatch):
    texts, flags, _ = SC.multi(3)
    c = _case(K, "multi_3", texts, flags)
    _knobs(monkeypatch, hitcap=max(len(h) for h in c["hits"].values()))
    _ab(N, K, "multi_3", texts, flags, step=D.sharded_step, coarse_expected=3, promoted_expected=0)


# ----------------------------------------------------------------------------
# three steps on one engine
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 3])
def test_three_steps(N, K, D, monkeypatch, lanes):
    """the second and third steps partition the coarse genomes again into the arrays the first step left them"""
    texts, flags, _ = SC.multi(3)
    _case(K, "multi_3", texts, flags)
    _knobs(monkeypatch)
    on = _ab(N, K, "multi_3", texts, flags, step=D.sharded_step, lanes=lanes, steps=3, coarse_expected=9, promoted_expected=0)
    assert len(on["cands"]) == 3
    for c, r in zip(on["cands"][1:], on["recs"][1:]):
        assert np.array_equal(c, on["cands"][0]) and np.array_equal(r, on["recs"][0])

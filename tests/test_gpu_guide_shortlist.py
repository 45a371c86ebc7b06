"""The shortlist of --guide-candidates on the GPU (kr_guides_run_top, csrc/k_guides.inc: k_guides_top): the device's
[regions, N] records equal the reference's (guide_shortlist_reference.py) field for field over the sets of
guide_shortlist_cases.py -- guide_cases' and the planted lane set -- for N = 1, 2 and 8; rank 1 is kr_guides_run's record;
two runs give the same bytes; a run cut into batches equals the single run; the library's refusals and its two states."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_cases                                                         # noqa: E402
import guide_shortlist_cases as SC                                         # noqa: E402
import guide_shortlist_reference as ref                                    # noqa: E402
from guides_reference import FIELDS                                        # noqa: E402

pytestmark = pytest.mark.gpu


def _pack(regs):
    rows, off, bounds = guide_cases.pack(regs)
    k = len(rows[0])
    return (np.frombuffer("".join(rows).encode("ascii"), dtype=np.uint8).reshape(len(rows), k), np.array(off, dtype=np.uint64),
            np.array(bounds, dtype=np.uint32).reshape(-1, 2))


@functools.lru_cache(maxsize=None)
def _case(name):
    """the set's regions, packed, and the reference's shortlists of 8: computed once, shared, never written to (the shortlist
    of N is its first N columns)"""
    from krisp_amd import _native
    s = SC.SETS[name]
    regs = SC.regions(name)
    lists = ref.shortlists(regs, s["geo"][0], s["geo"][1], top=8, **SC.options(name))
    want = np.zeros((len(regs), 8), dtype=_native.GUIDE_RECORD)
    for i, slots in enumerate(lists):
        for j, r in enumerate(slots):
            for f in FIELDS:
                want[f][i, j] = r[f]
    want.setflags(write=False)
    return _pack(regs) + (want,)


def _table(eng, name):
    o = SC.options(name)
    eng.guides_table(o["g"], KF.motif_masks(o["pam5"]), KF.motif_masks(o["pam3"]), o["gc"], o["min_mismatches"])


@pytest.mark.parametrize("name", list(SC.SETS))
def test_every_shortlist_equals_the_reference(name):
    """all fields of all slots for N = 1, 2, 8 (the k2047 set among them), the padding and the empty slots zero; slot 0 is
    Engine.guides' record byte for byte; a second run gives the same bytes"""
    from krisp_amd import _native
    L, D, _ = SC.SETS[name]["geo"]
    rows, off, bounds, want8 = _case(name)
    with _native.Engine() as eng:
        _table(eng, name)
        one = eng.guides(rows, off, bounds, L, D)
        for top in SC.TOPS:
            want = np.ascontiguousarray(want8[:, :top])
            got = eng.guides_top(rows, off, bounds, L, D, top)
            again = eng.guides_top(rows, off, bounds, L, D, top)
            print(name, "top", top, "regions", len(want), "filled", int(want["found"].sum()), "device", int(got["found"].sum()))
            assert got.dtype.itemsize == 32 and got.shape == want.shape
            assert got.tobytes() == again.tobytes()
            for f in FIELDS + ("pad",):
                bad = np.argwhere(got[f] != want[f])
                assert len(bad) == 0, (f, top, bad[:5].tolist(), got[f][got[f] != want[f]][:5].tolist(), want[f][got[f] != want[f]][:5].tolist())
            assert got.tobytes() == want.tobytes()
            assert np.ascontiguousarray(got[:, 0]).tobytes() == one.tobytes()
    assert one.tobytes() == np.ascontiguousarray(want8[:, 0]).tobytes()


def test_the_batches_of_a_long_list_join_up():
    """more regions than one batch takes (2^18) at N = 2: the records are those of the same regions alone, over and over"""
    from krisp_amd import _native
    name, top = "12_4_12_g12", 2
    L, D, _ = SC.SETS[name]["geo"]
    rows, off, bounds, want8 = _case(name)
    want = np.ascontiguousarray(want8[:, :top])
    n, nrows = len(want), int(off[-1])
    reps = (1 << 18) // n + 2
    many_off = np.concatenate([(off[:-1][None, :] + (np.arange(reps, dtype=np.uint64) * np.uint64(nrows))[:, None]).ravel(),
                               np.array([reps * nrows], dtype=np.uint64)])
    with _native.Engine() as eng:
        _table(eng, name)
        one = eng.guides_top(rows, off, bounds, L, D, top)
        got = eng.guides_top(np.tile(rows, (reps, 1)), many_off, np.tile(bounds, (reps, 1)), L, D, top)
    assert reps * n > 1 << 18 and got.shape == (reps * n, top)
    assert one.tobytes() == want.tobytes()
    assert got.tobytes() == np.tile(one, (reps, 1)).tobytes()


def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    P, CAP, STATE = -2, -3, -4
    # (test_gpu_guides.py's region: with the motif T the one guide is the window [0, 12) on '-')
    rows = np.frombuffer(b"ACGTACGTACGTAC" + b"ACGTACGTCCGTAC", dtype=np.uint8).reshape(2, 14)
    off = np.array([0, 2], dtype=np.uint64)
    bnd = np.array([0, 14], dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731

    def code(f):
        with pytest.raises(_native.KrispHipError) as e:
            f()
        return e.value.code, str(e.value)

    with _native.Engine() as eng:
        out = np.zeros(16, dtype=_native.GUIDE_RECORD)
        run_top = lambda top: eng.lib.kr_guides_run_top(eng.ctx, ptr(rows), ptr(off), ptr(bnd), 1, 14, 5, 4, top)   # noqa: E731
        fetch = lambda cap: eng.lib.kr_guides_fetch(eng.ctx, ptr(out), cap)                                         # noqa: E731
        fetch_top = lambda cap: eng.lib.kr_guides_fetch_top(eng.ctx, ptr(out), cap)                                 # noqa: E731
        c, msg = code(lambda: eng.guides_top(rows, off, [[0, 14]], 5, 4, 2))
        assert c == STATE and "kr_guides_table first" in msg
        assert fetch_top(16) == STATE
        eng.guides_table(12, pam5=[8])
        for top in (0, 9, -1, 64):
            assert run_top(top) == P and b"top" in eng.lib.kr_last_error(eng.ctx)
            assert fetch_top(16) == STATE
        # the two states: a top run does not satisfy kr_guides_fetch, nor kr_guides_run the top fetch
        assert run_top(3) == 1
        assert fetch(16) == STATE
        assert fetch_top(2) == CAP and fetch_top(3) == 3
        assert [int(out[0][f]) for f in FIELDS] == [1, 1, 0, 1, 1, 6, 1]
        assert [[int(out[j][f]) for f in FIELDS] for j in (1, 2)] == [[0, 0, 0, 0, 0, 0, 1]] * 2 and not out["pad"].any()
        top_bytes = out[:3].tobytes()
        single = eng.guides(rows, off, [[0, 14]], 5, 4)
        assert single.tobytes() == out[:1].tobytes()
        assert fetch_top(16) == 3 and out[:3].tobytes() == top_bytes             # (the top records outlive a plain run)
        assert run_top(9) == P and fetch_top(16) == STATE and fetch(16) == 1     # (a refused top run drops its own records only)
        assert run_top(8) == 1 and fetch_top(7) == CAP and fetch_top(8) == 8
        # the run's own refusals are kr_guides_run's; none leaves top records behind
        assert code(lambda: eng.guides_top(rows[:, :11], off, [[0, 11]], 5, 4, 2))[0] == P                     # K < guide_size
        assert fetch_top(16) == STATE and fetch(16) == 1
        assert code(lambda: eng.guides_top(rows, off, [[9, 8]], 5, 4, 2))[0] == P                              # lo > hi
        assert code(lambda: eng.guides_top(rows, off, [[0, 15]], 5, 4, 2))[0] == P                             # hi > K
        assert code(lambda: eng.guides_top(rows, [0, 1, 1], [[0, 14], [0, 14]], 5, 4, 2))[0] == P              # no template
        assert eng.lib.kr_guides_run_top(eng.ctx, None, ptr(off), ptr(bnd), 1, 14, 5, 4, 2) == P               # null pointers
        # a new table drops both
        assert run_top(2) == 1 and fetch_top(16) == 2
        eng.guides_table(12)
        assert fetch_top(16) == STATE and fetch(16) == STATE
        # no region: no record
        assert eng.guides_top(np.empty((0, 14), dtype=np.uint8), [0], np.empty((0, 2), dtype=np.uint32), 5, 4, 8).shape == (0, 8)

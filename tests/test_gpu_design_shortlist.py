"""--primer-candidates' shortlist on the GPU (kr_design_run_top, csrc/k_design.inc: k_design_top): every slot of every region
equals the brute-force shortlist (design_shortlist_reference.py) field for field, over the templates and option sets of
design_cases.py at N = 1, 2 and 8, with and without the hairpin check; slot 0 is kr_design_run's record byte for byte; two
runs give the same bytes; the batches join up; the library's refusals and the two runs' separate states."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import thermo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_cases                                                        # noqa: E402
import design_shortlist_reference as SR                                    # noqa: E402

pytestmark = pytest.mark.gpu

KR_ERR_PARAM, KR_ERR_CAPACITY, KR_ERR_STATE = -2, -3, -4        # include/krisp_hip.h
TOPS = (1, 2, 8)


def _rows(templates):
    return np.frombuffer("".join(templates).encode("ascii"), dtype=np.uint8).reshape(len(templates), -1)


def _equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    for name in want.dtype.names:
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, (what, name, bad[:5].tolist(), got[name][tuple(bad[:5].T)].tolist(), want[name][tuple(bad[:5].T)].tolist())
    assert got.tobytes() == want.tobytes(), what


def _check_geometry(geo, hairpins):
    """every option set of the geometry at every N of TOPS against the reference, whose passing pairs are computed once per
    set and sliced; -> the numbers of passing pairs met"""
    from krisp_amd import _native
    L, D, R = geo
    ts = design_cases.templates(L, D, R, design_cases.GEOMETRIES[geo]["n_random"])
    rows = _rows(ts)
    counts = set()
    for opts in design_cases.option_sets(geo):
        passed = SR.passing_all(ts, L, D, R, hairpins=hairpins, **opts)
        n = [len(p[2]) for p in passed]
        counts |= set(n)
        with _native.Engine() as eng:
            eng.design_table(thermo.params(**opts))
            if hairpins:
                eng.design_hairpins(thermo.hairpin_params())
            one = eng.design(rows, L, D, R)
            for top in TOPS:
                got = eng.design_top(rows, L, D, R, top)
                again = eng.design_top(rows, L, D, R, top)
                assert got.tobytes() == again.tobytes()
                _equal(got, SR.shortlist(passed, top, hairpins), (geo, opts, top))
                assert got[:, 0].tobytes() == one.tobytes()
                assert ((got["found"] != 0).sum(axis=1) == np.minimum(n, top)).all()
            # (the plain run's records stand beside the shortlist's)
            assert eng.design(rows, L, D, R).tobytes() == one.tobytes()
        print(geo, opts, "hairpins", hairpins, "regions", len(ts), "pairs a region", sorted(set(n)))
        assert 0 < sum(1 for x in n if x) < len(ts)
    return counts


@pytest.mark.parametrize("geo", list(design_cases.GEOMETRIES))
def test_every_slot_equals_the_brute_force_shortlist(geo):
    counts = _check_geometry(geo, False)
    # the list's edges occur: no pair, fewer than N, exactly N, more than N (test_design_shortlist_host.py pins the counts)
    assert 0 in counts and max(counts) > 8
    if geo == (12, 4, 12):
        assert {1, 2, 8} <= counts


@pytest.mark.parametrize("geo", [(30, 40, 30), (12, 4, 12)])
def test_with_the_hairpin_check_every_slot_carries_its_figures(geo):
    counts = _check_geometry(geo, True)
    assert 0 in counts and max(counts) > 8


def test_the_batches_of_a_long_list_join_up():
    """more regions than one batch holds at N = 8 (2^20 records): the records are those of the same templates alone"""
    from krisp_amd import _native
    L, D, R = 12, 4, 12
    ts = design_cases.templates(L, D, R, 30)
    rows = _rows(ts)
    opts = design_cases.option_sets((L, D, R))[0]
    reps = ((1 << 20) // 8) // len(ts) + 2
    many = np.tile(rows, (reps, 1))
    with _native.Engine() as eng:
        eng.design_table(thermo.params(**opts))
        eng.design_hairpins(thermo.hairpin_params())
        one = eng.design_top(rows, L, D, R, 8)
        got = eng.design_top(many, L, D, R, 8)
    assert len(many) * 8 > 1 << 20 and got.shape == (reps * len(ts), 8)
    assert got.tobytes() == np.tile(one, (reps, 1)).tobytes()
    assert (one["found"] != 0).sum() > len(ts) and (one["left_hairpin"] != 0).any()


def test_the_library_says_what_it_does_not_take_and_keeps_two_states():
    from krisp_amd import _native
    L, D, R = 12, 4, 12
    rows = _rows(design_cases.templates(L, D, R, 30))
    opts = design_cases.option_sets((L, D, R))[0]
    buf = np.zeros((len(rows), 8), dtype=_native.DESIGN_RECORD)
    hp = np.zeros((len(rows), 8, 2), dtype=np.int32)

    def code(fn, *a):
        return int(fn(eng.ctx, *a))

    with _native.Engine() as eng:
        with pytest.raises(Exception, match="kr_design_table first"):
            eng.design_top(rows, L, D, R, 4)
        eng.design_table(thermo.params(**opts))
        for top in (0, 9, -1):
            with pytest.raises(Exception, match="1 <= top <= 8") as e:
                eng.design_top(rows, L, D, R, top)
            assert e.value.code == KR_ERR_PARAM
        with pytest.raises(Exception, match="flanks of at most"):
            eng.design_top(np.zeros((1, 1030), dtype=np.uint8), 1024, 3, 3, 2)
        assert eng.design_top(np.empty((0, 28), dtype=np.uint8), L, D, R, 3).shape == (0, 3)
        # a plain run does not satisfy the shortlist's fetches ...
        eng.design_table(thermo.params(**opts))
        plain = eng.design(rows, L, D, R)
        assert code(eng.lib.kr_design_fetch_top, _native._ptr(buf), buf.size) == KR_ERR_STATE
        assert code(eng.lib.kr_design_fetch_top_hairpins, _native._ptr(hp), hp.size) == KR_ERR_STATE
        # ... nor a shortlist run the plain ones, and kr_design_table drops both
        eng.design_table(thermo.params(**opts))
        short = eng.design_top(rows, L, D, R, 8)
        assert code(eng.lib.kr_design_fetch, _native._ptr(buf), buf.size) == KR_ERR_STATE
        assert code(eng.lib.kr_design_fetch_top_hairpins, _native._ptr(hp), hp.size) == KR_ERR_STATE     # (the check was off)
        assert code(eng.lib.kr_design_fetch_top, _native._ptr(buf), buf.size - 1) == KR_ERR_CAPACITY     # (a short buffer)
        assert code(eng.lib.kr_design_fetch_top, _native._ptr(buf), buf.size) == buf.size
        assert buf.tobytes() == short.tobytes() and short[:, 0].tobytes() == plain.tobytes()
        # a refused top leaves no shortlist standing
        with pytest.raises(Exception, match="1 <= top <= 8"):
            eng.design_top(rows, L, D, R, 9)
        assert code(eng.lib.kr_design_fetch_top, _native._ptr(buf), buf.size) == KR_ERR_STATE
        eng.design_hairpins(thermo.hairpin_params())
        eng.design_top(rows, L, D, R, 8)
        assert code(eng.lib.kr_design_fetch_top_hairpins, _native._ptr(hp), hp.size) == hp.size
        eng.design_table(thermo.params(**opts))
        assert code(eng.lib.kr_design_fetch_top, _native._ptr(buf), buf.size) == KR_ERR_STATE
        assert code(eng.lib.kr_design_fetch, _native._ptr(buf), buf.size) == KR_ERR_STATE

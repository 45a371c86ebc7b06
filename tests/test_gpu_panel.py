"""--panel on the GPU (kr_panel_*, csrc/k_panel.inc): over every set of panel_cases.py the device's members, running
figures, drop counts and the fate of every candidate equal the reference's (panel_reference.py) field for field; two runs
give the same bytes; a run after a run of another size gives that size's answer; the library's refusals."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import thermo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_cases as PC                                                    # noqa: E402
import panel_reference as ref                                               # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(templates):
    return np.frombuffer("".join(templates).encode("ascii"), dtype=np.uint8).reshape(len(templates), -1)


def _params(max_sec):
    """the model with this max_sec in mK (a set's max_sec comes from thermo.options)"""
    p = thermo.params()
    p.max_sec = max_sec
    return p


def _compare(got, want, what):
    members, fates = got
    wm, wf = want
    assert fates.tolist() == [tuple(f) for f in wf], (what, [i for i, (a, b) in enumerate(zip(fates.tolist(), wf)) if tuple(a) != tuple(b)][:5])
    assert members["position"].tolist() == [m["position"] for m in wm], what
    assert members["cross_any"].tolist() == [m["cross_any"] for m in wm], what
    assert members["cross_end"].tolist() == [m["cross_end"] for m in wm], what
    assert members["dropped"].tolist() == [m["dropped"] for m in wm], what


@pytest.mark.parametrize("name", list(PC.SETS))
def test_every_set_equals_the_reference(name):
    from krisp_amd import _native
    c = PC.case(name)
    rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)
    with _native.Engine() as eng:
        eng.design_table(_params(c["max_sec"]))
        got = eng.panel(rows, pairs, c["size"])
        again = eng.panel(rows, pairs, c["size"])
    want = PC.expected(name)
    print(name, "candidates", len(rows), "members", len(got[0]), "of", c["size"], "fates", np.bincount(got[1]["fate"], minlength=4).tolist())
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    _compare(got, want, name)


def test_a_run_after_a_run_of_another_size():
    """one context: N = 5, then N = 2, then N = 5 again, then another set: each answer is that run's own"""
    from krisp_amd import _native
    c = PC.case("random_300")
    rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)
    small = ref.select(c["templates"], c["pairs"], 2, c["max_sec"])
    assert len(small[0]) == 2 and len(PC.expected("random_300")[0]) == 5
    with _native.Engine() as eng:
        eng.design_table(_params(c["max_sec"]))
        _compare(eng.panel(rows, pairs, 5), PC.expected("random_300"), "5")
        _compare(eng.panel(rows, pairs, 2), small, "2 after 5")
        _compare(eng.panel(rows, pairs, 5), PC.expected("random_300"), "5 after 2")
        d = PC.case("w16")
        eng.design_table(_params(d["max_sec"]))
        _compare(eng.panel(_rows(d["templates"]), np.array(d["pairs"], dtype=np.uint16), d["size"]), PC.expected("w16"), "w16 after")
        members, fates = eng.panel(np.empty((0, 40), dtype=np.uint8), np.empty((0, 4), dtype=np.uint16), 8)
        assert len(members) == 0 and len(fates) == 0


def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    c = PC.case("random_65")
    rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)

    def code(eng, *a):
        with pytest.raises(_native.KrispHipError) as e:
            eng.panel(*a)
        return e.value.code

    with _native.Engine() as eng:
        assert code(eng, rows, pairs, 3) == -4                                 # KR_ERR_STATE: no kr_design_table yet
        out = np.zeros(4, dtype=_native.PANEL_MEMBER)
        assert eng.lib.kr_panel_fetch(eng.ctx, out.ctypes.data, 4) == -4       # ... and no run yet
        assert eng.lib.kr_panel_fates(eng.ctx, out.ctypes.data, 4) == -4
        eng.design_table(_params(c["max_sec"]))
        assert code(eng, rows, pairs, 0) == -2 and code(eng, rows, pairs, 65) == -2
        assert code(eng, np.zeros((2, 2048), dtype=np.uint8), pairs[:2], 3) == -2
        for bad in ((0, 9, 30, 10), (0, 61, 30, 10), (0, 10, 31, 10), (35, 10, 30, 10), (0, 10, 30, 9)):
            q = pairs.copy()
            q[40] = bad
            assert code(eng, rows, q, 3) == -2, bad
        assert eng.lib.kr_panel_run(eng.ctx, None, pairs.ctypes.data, 5, 40, 3) == -2
        assert eng.lib.kr_panel_run(eng.ctx, rows.ctypes.data, None, 5, 40, 3) == -2
        assert eng.lib.kr_panel_run(eng.ctx, None, None, 0, 40, 3) == 0
        # a refused run leaves nothing to fetch; a good one does
        assert eng.lib.kr_panel_fetch(eng.ctx, out.ctypes.data, 4) == 0
        assert code(eng, rows, pairs, 0) == -2
        assert eng.lib.kr_panel_fetch(eng.ctx, out.ctypes.data, 4) == -4
        members, _ = eng.panel(rows, pairs, 3)
        assert len(members) == 3 and eng.lib.kr_panel_fetch(eng.ctx, out.ctypes.data, 2) == -3        # KR_ERR_CAPACITY
    # all candidates are resident: a context whose budget cannot hold them says so
    big = np.tile(rows, (400, 1))
    with _native.Engine(hbm_budget=1 << 20) as eng:
        eng.design_table(_params(c["max_sec"]))
        assert code(eng, big, np.tile(pairs, (400, 1)), 3) == -3

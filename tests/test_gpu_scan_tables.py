"""The seed passes and the locate pass with tables past 1024 slots (scan_table_cases.py): thousands of targets, guides and
groups over a text of a tile and a tail.  The tables test_scan_table_cases.py's census describes -- probe chains of ten slots
and more, a chain that wraps from the last slot to slot 0, a slot that lists the entries of ten targets and more, list
indexes in the thousands, shared bitmap bits -- against references without seeds, hashes or tables: the complete hit
lists, the windows' text, and the table's size as the library returns it against the census's.  Once without the grid cap
and once with KR_SCAN_GRID = 1 (one workgroup takes both tiles)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_hits_reference as href                                        # noqa: E402
import scan_table_cases as TC                                              # noqa: E402
import test_gpu_guide_hits as GH                                           # noqa: E402
import test_gpu_scan_properties as SP                                      # noqa: E402
from test_gpu_scan_grid import digest, geometry, set_cap                   # noqa: E402
from test_scan_table_cases import locate_census, near_census              # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(TC.NEAR_CASES))
def test_near_matches_and_guide_hits_of_thousands_of_targets(name, monkeypatch):
    L, D, R = TC.GEOMETRY
    c = TC.near_case(name)
    text, targets, M = c["text"], c["targets"], c["M"]
    want, columns = TC.near_by_packed_words(text, L, D, R, targets, M)
    guide_want = np.zeros(len(want), dtype=href.HIT)
    for f, g in (("pos", "pos"), ("strand", "strand"), ("guide", "target"), ("mismatches", "mismatches")):
        guide_want[f] = want[g]
    guide_want["columns"], guide_want["pam"] = columns, 3       # (no motifs: both match)
    census = near_census(targets, M)
    print(name, "hits", len(want), "by distance", np.bincount(want["mismatches"], minlength=M + 1).tolist(), census)
    assert len(want) >= len(targets) // 4 and (np.bincount(want["mismatches"], minlength=M + 1) > 0).all()
    assert {0, 1} == set(want["strand"].tolist()) and (want["pos"] < TC.TILE).any()
    assert (want["pos"] >= TC.TILE).any() or len(targets) < 1000
    runs = {}
    for cap in (None, 1):
        set_cap(monkeypatch, cap)
        with SP.engine(L, D, R, False, len(text)) as eng:
            eng.upload(0, text)
            assert eng.near_table(targets, M) == census["slots"] > 1024
            SP.check_near(eng, text, L, D, R, False, targets, M, want)
            assert geometry(eng, cap, len(text), TC.K) == (1 if cap else 0)
            runs[cap] = [digest(eng.near(0), eng.near_windows(TC.K))]
            assert eng.guide_hits_table(targets, M) == census["slots"]
            got, _ = GH._check(eng, text, TC.K, guide_want)
            assert geometry(eng, cap, len(text), TC.K) == (1 if cap else 0)
            runs[cap].append(digest(got, eng.guide_hit_windows(TC.K)))
    assert runs[1] == runs[None]


def test_locate_with_thousands_of_groups(monkeypatch):
    L, D, R = TC.GEOMETRY
    c = TC.locate_case()
    text, flanks = c["text"], c["flanks"]
    want = TC.locate_by_dictionary(text, L, D, R, flanks)
    census = locate_census(flanks, L)
    print("hits", len(want), census)
    assert len(want) >= 2000 and {0, 1} == set(want["strand"].tolist()) and len(set(want["group"].tolist())) >= 2000
    runs = {}
    for cap in (None, 1):
        set_cap(monkeypatch, cap)
        with SP.engine(L, D, R, False, len(text)) as eng:
            eng.upload(0, text)
            assert eng.locate_table(flanks) == census["slots"] > 1024
            SP.check_locate(eng, text, L, D, R, False, flanks, want)
            assert geometry(eng, cap, len(text), TC.K) == (1 if cap else 0)
            runs[cap] = digest(eng.locate(0), eng.locate_windows(TC.K))
    assert runs[1] == runs[None]

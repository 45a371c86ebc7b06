"""--design-primers on the GPU (kr_design_*, csrc/k_design.inc): the device's record of every region equals the brute-force
reference's (design_reference.py) field for field, over random templates and templates with planted structure
(design_cases.py), four geometries, option sets that make each filter bind; two runs give the same bytes; the library's
refusals; the command line end to end on the golden cases whose flanks are primers."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import codec, primers, thermo
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_cases                                                        # noqa: E402
from design_reference import design as ref_design                          # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(templates):
    return np.frombuffer("".join(templates).encode("ascii"), dtype=np.uint8).reshape(len(templates), -1)


@pytest.mark.parametrize("geo", list(design_cases.GEOMETRIES))
def test_every_record_equals_the_brute_force_record(geo):
    """every option set of the geometry: all 19 fields of all regions; regions with and without a pair both occur; every
    set that moves one figure of the base set changes an answer (its filter binds); a second run gives the same bytes"""
    from krisp_amd import _native
    L, D, R = geo
    ts = design_cases.templates(L, D, R, design_cases.GEOMETRIES[geo]["n_random"])
    rows = _rows(ts)
    base = None
    for opts in design_cases.option_sets(geo):
        with _native.Engine() as eng:
            eng.design_table(thermo.params(**opts))
            got = eng.design(rows, L, D, R)
            again = eng.design(rows, L, D, R)
        want = ref_design(ts, L, D, R, **opts)
        nfound = int(want["found"].sum())
        print(geo, opts, "regions", len(ts), "with a pair", nfound, "device", int(got["found"].sum()))
        assert got.tobytes() == again.tobytes()
        for name in want.dtype.names:
            bad = np.flatnonzero(got[name] != want[name])
            assert len(bad) == 0, (name, bad[:5].tolist(), got[name][bad[:5]].tolist(), want[name][bad[:5]].tolist())
        assert got.tobytes() == want.tobytes()
        assert 0 < nfound < len(ts)
        if base is None:
            base = want
        else:
            assert (want != base).any(), opts


def test_the_batches_of_a_long_list_join_up():
    """more regions than one batch of templates holds (64 MiB): the records are those of the same templates alone"""
    from krisp_amd import _native
    L, D, R = 12, 4, 12
    ts = design_cases.templates(L, D, R, 30)
    rows = _rows(ts)
    opts = design_cases.option_sets((L, D, R))[0]
    reps = (64 << 20) // (len(ts) * (L + D + R)) + 2
    many = np.tile(rows, (reps, 1))
    with _native.Engine() as eng:
        eng.design_table(thermo.params(**opts))
        one = eng.design(rows, L, D, R)
        got = eng.design(many, L, D, R)
    assert len(got) == reps * len(ts) and got.tobytes() == np.tile(one, reps).tobytes()
    assert one.tobytes() == ref_design(ts, L, D, R, **opts).tobytes()


def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    rows = _rows(["ACGT" * 7])
    with _native.Engine() as eng:
        with pytest.raises(Exception, match="kr_design_table first"):
            eng.design(rows, 12, 4, 12)
        for bad, msg in ((dict(primer_size=(9, 20)), "size_lo"), (dict(primer_size=(20, 61)), "size_lo"),
                         (dict(tm=(60, 50)), "upper bound"), (dict(gc_clamp=30), "gc_clamp")):
            with pytest.raises(Exception, match=msg):
                eng.design_table(thermo.params(**bad))
        p = thermo.params()
        p.conc_ds = 0
        with pytest.raises(Exception, match="model"):
            eng.design_table(p)
        eng.design_table(thermo.params(primer_size=(10, 12)))
        with pytest.raises(Exception, match="flanks of at most"):
            eng.design(np.zeros((1, 1030), dtype=np.uint8), 1024, 3, 3)
        assert len(eng.design(np.empty((0, 28), dtype=np.uint8), 12, 4, 12)) == 0


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def _primer_case(case):
    k = _amplicon(case)
    Le, De, Re = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
    return min(Le, Re) >= 10


E2E_CASES = [c for c in FC if "csv" in c and _primer_case(c)]


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def test_the_command_line_writes_what_the_reference_records_render_to(tmp_path):
    """every golden case with a CSV whose effective flanks are both >= 10 bases: with --design-primers the CSV and the
    alignment file are the reference's records through primers.render_designed; with no primer option they are today's"""
    names = [c["name"] for c in E2E_CASES]
    assert "c1_30_40_30" in names and "rand6_12_4_12" in names and "long_130_60_129" in names and len(names) >= 12
    found = missing = complete = 0
    for n, case in enumerate(E2E_CASES):
        d = tmp_path / str(n)
        d.mkdir()
        ing, out = _files(case, d)
        argv = _argv(case, d, ing, out)
        k = _amplicon(case)
        Le, De, Re = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
        h = min(Le, Re, 20)
        opts = dict(tm=(30, 75), gc=(20, 80), amp_size=(Le + De + Re - 4, Le + De + Re), primer_size=(h - 1, h), max_sec_tm=35,
                    gc_clamp=0, max_end_gc=5)
        flags = []
        for name, v in opts.items():
            flags += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
        dot = ["--dot-alignment"] if "--dot-alignment" in argv else []
        plain_csv = _main(argv + ["-o", str(d / "plain.align")])
        csv = _main(argv + flags + ["--design-primers", "-o", str(d / "design.align")])
        assert plain_csv == case["csv"]
        assert _main(argv + flags + ["-o", str(d / "flags.align")]) == case["csv"]
        assert open(d / "flags.align", "rb").read() == open(d / "plain.align", "rb").read()
        groups, _ = KF.find_regions(ing, out, case["L"], case["R"], k, omit_soft=case["omit_soft"])
        ingroup = [KF.simplename(f) for f in ing] if out else None
        rows, L, D, R = KF.design_templates(groups, ingroup)
        want = ref_design([bytes(r) for r in rows], L, D, R, **opts) if len(rows) else []
        assert KF.design_primers(groups, ingroup, **opts).tobytes() == (want.tobytes() if len(rows) else b"")
        want_csv, want_align = primers.render_designed(groups, ingroup, want, dot=bool(dot))
        print(case["name"], "regions", len(rows), "with a pair", int(sum(int(r["found"]) for r in want)))
        assert csv == want_csv
        assert open(d / "design.align").read() == want_align
        assert csv.split("\n")[0] == "left_seq,diag_seq,right_seq," + ",".join(primers.DESIGN_COLUMNS)
        nf = int(sum(int(r["found"]) for r in want))
        written = csv.count("\n") - 1
        # (a consensus column holding U stops the renderer, with the option as without it: rows are lost there)
        assert written == nf if plain_csv.count("\n") - 1 == len(rows) else written <= nf
        assert want_align.count("Forward") == 2 * written
        assert all(ln.count(",") == 2 + len(primers.DESIGN_COLUMNS) for ln in csv.split("\n")[1:-1])
        complete += written == nf
        found += nf
        missing += len(rows) - nf
    assert found > 0 and missing > 0 and complete >= len(E2E_CASES) - 2

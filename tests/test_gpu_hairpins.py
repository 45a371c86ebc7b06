"""--design-primers --hairpins on the GPU (kr_design_hairpins, kr_design_fetch_hairpins, k_design<true> of csrc/k_design.inc):
the device's records and hairpin figures equal the brute-force reference's (hairpin_reference.py) field for field over the
cases of hairpin_cases.py; a limit that cannot bite and a limit the plain winner keeps leave the plain bytes; the states of
the library; the command line."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import primers, thermo
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hairpin_cases as HC                                                 # noqa: E402
import hairpin_reference as HR                                             # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(templates):
    return np.frombuffer("".join(templates).encode("ascii"), dtype=np.uint8).reshape(len(templates), -1)


def _device(name, max_sec_tm, hairpins=True):
    from krisp_amd import _native
    L, D, R = HC.CASES[name]["geo"]
    with _native.Engine() as eng:
        eng.design_table(thermo.params(**HC.options(name, max_sec_tm)))
        if hairpins:
            eng.design_hairpins(thermo.hairpin_params())
        return eng.design(_rows(HC.templates(name)), L, D, R)


@pytest.mark.parametrize("name", list(HC.CASES))
def test_every_record_and_hairpin_figure_equals_the_brute_force_one(name):
    """every option set of the case: the 19 fields of the record and the two hairpin figures of every region"""
    for sec in HC.CASES[name]["sets"]:
        got, want = _device(name, sec), HC.reference(name, sec)
        print(name, sec, "regions", len(want), "with a pair", int(want["found"].sum()), "device", int(got["found"].sum()))
        assert got.dtype == want.dtype
        for field in want.dtype.names:
            bad = np.flatnonzero(got[field] != want[field])
            assert len(bad) == 0, (sec, field, bad[:5].tolist(), got[field][bad[:5]].tolist(), want[field][bad[:5]].tolist())
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", list(HC.CASES))
def test_a_limit_that_cannot_bite_leaves_the_plain_bytes(name):
    """differential A: --max_sec_tm 1000: the 64-byte records of the hairpin run are the plain run's"""
    hp, plain = _device(name, 1000), _device(name, 1000, hairpins=False)
    assert hp.dtype.itemsize == 72 and plain.dtype.itemsize == 64
    assert HR.plain(hp).tobytes() == plain.tobytes()
    assert int(plain["found"].sum()) > 0


@pytest.mark.parametrize("name", list(HC.CASES))
def test_a_plain_winner_within_the_limit_stays_and_no_other_is_better(name):
    """differential B: where the plain winner's two reference figures are at most max_sec the record is the plain one;
    elsewhere the pair penalty is not lower, or there is no pair"""
    for sec in HC.CASES[name]["sets"]:
        hp, plain = _device(name, sec), _device(name, sec, hairpins=False)
        same = other = 0
        for i, (t, b) in enumerate(zip(HC.templates(name), plain)):
            a = hp[i:i + 1]
            if not int(b["found"]):
                assert not int(a["found"][0])
                continue
            if max(HR.hairpin_figure(x) for x in HR.winner_sequences(t, b)) <= thermo.mk(sec):
                assert HR.plain(a).tobytes() == b.tobytes()
                same += 1
            else:
                assert not int(a["found"][0]) or int(a["pair_penalty"][0]) >= int(b["pair_penalty"])
                assert HR.plain(a).tobytes() != b.tobytes()
                other += 1
        print(name, sec, "the plain winner stays", same, "goes", other)
        assert same > 0


def test_the_states_of_the_library():
    from krisp_amd import _native
    name, sec = "30_40_30", 20
    L, D, R = HC.CASES[name]["geo"]
    rows = _rows(HC.templates(name))
    with _native.Engine() as eng:
        with pytest.raises(Exception, match="kr_design_table first"):
            eng.design_hairpins(thermo.hairpin_params())
        eng.design_table(thermo.params(**HC.options(name, sec)))
        plain = eng.design(rows, L, D, R)
        out = np.zeros(2 * len(rows), dtype=np.int32)
        assert eng.lib.kr_design_fetch_hairpins(eng.ctx, out.ctypes.data, len(out)) == -4          # KR_ERR_STATE
        bad = thermo.hairpin_params()
        bad.loop_ds[3] = 20000
        with pytest.raises(Exception, match="loop_ds\\[3\\]"):
            eng.design_hairpins(bad)
        assert eng.design(rows, L, D, R).tobytes() == plain.tobytes()                                # (a refused table: off)
        eng.design_hairpins(thermo.hairpin_params())
        hp = eng.design(rows, L, D, R)
        assert hp.dtype == _native.DESIGN_RECORD_HP and hp.tobytes() == HC.reference(name, sec).tobytes()
        assert eng.design(rows, L, D, R).tobytes() == hp.tobytes()                                   # a second batch
        assert HR.plain(hp).tobytes() != plain.tobytes()
        eng.design_hairpins(None)
        assert eng.design(rows, L, D, R).tobytes() == plain.tobytes()
        eng.design_hairpins(thermo.hairpin_params())
        assert eng.design(rows, L, D, R).tobytes() == hp.tobytes()
        eng.design_table(thermo.params(**HC.options(name, sec)))
        assert eng.design(rows, L, D, R).tobytes() == plain.tobytes()
        assert eng.lib.kr_design_fetch_hairpins(eng.ctx, out.ctypes.data, len(out)) == -4
        eng.design_hairpins(thermo.hairpin_params())
        eng.design(rows, L, D, R)
        assert eng.lib.kr_design_fetch_hairpins(eng.ctx, out.ctypes.data, len(out) - 1) < 0         # too small a buffer
        assert eng.lib.kr_design_fetch_hairpins(eng.ctx, out.ctypes.data, len(out)) == len(out)
        assert out.reshape(-1, 2).tolist() == np.stack([hp["left_hairpin"], hp["right_hairpin"]], axis=1).tolist()


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def test_the_command_line_on_c1_30_40_30(tmp_path):
    """--hairpins: the two columns behind the designer's, every figure within --max_sec_tm, the reference's records
    rendered; with --out_primer_products every location of a region with a pair is still an exact product; without
    --hairpins the CSV is the plain designer's"""
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    sec = 25
    opts = dict(tm=(30, 75), gc=(20, 80), amp_size=(96, 100), primer_size=(19, 20), max_sec_tm=sec, gc_clamp=0, max_end_gc=5)
    flags = []
    for name, v in opts.items():
        flags += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], _amplicon(case), omit_soft=case["omit_soft"])
    ingroup = [KF.simplename(f) for f in ing] if out else None
    rows, L, D, R = KF.design_templates(groups, ingroup)
    ts = [bytes(r).decode("ascii") for r in rows]
    plain_csv = _main(argv + flags + ["--design-primers", "-o", str(tmp_path / "plain.align")])
    want_plain = HR.design(ts, L, D, R, hairpins=False, **opts)
    assert plain_csv == primers.render_designed(groups, ingroup, want_plain)[0]
    assert plain_csv.split("\n")[0] == "left_seq,diag_seq,right_seq," + ",".join(primers.DESIGN_COLUMNS)

    csv = _main(argv + flags + ["--design-primers", "--hairpins", "-o", str(tmp_path / "hp.align"),
                                "--out_primer_products", str(tmp_path / "pp.tsv"), "--primer-mismatches", "0"])
    want = HR.design(ts, L, D, R, **opts)
    assert KF.design_primers(groups, ingroup, hairpins=True, **opts).tobytes() == want.tobytes()
    want_csv, want_align = primers.render_designed(groups, ingroup, want)
    assert csv == want_csv and open(tmp_path / "hp.align").read() == want_align
    lines = csv.split("\n")[:-1]
    assert lines[0] == "left_seq,diag_seq,right_seq," + ",".join(primers.DESIGN_COLUMNS + primers.HAIRPIN_COLUMNS)
    nf = int(want["found"].sum())
    assert len(lines) - 1 == nf > 0
    for ln in lines[1:]:
        cells = ln.split(",")
        assert len(cells) == 3 + len(primers.DESIGN_COLUMNS) + 2
        assert all(float(x) <= sec for x in cells[-2:])
    assert "Hairpin" in want_align and "Hairpin" not in open(tmp_path / "plain.align").read()
    # every data row of the CSV has its designed product in the ingroup: its product_size, no mismatches
    tsv = open(tmp_path / "pp.tsv").read().split("\n")
    assert tsv[0] == KF.PRODUCT_HEADER and tsv[-1] == ""
    sizes = [ln.split(",")[lines[0].split(",").index("product_size")] for ln in lines[1:]]
    exact = [ln.split("\t") for ln in tsv[1:-1] if ln.split("\t")[8:] == ["0", "0", "0", "0"]]
    for region, size in enumerate(sizes):
        assert any(r[0] == str(region) and r[7] == size for r in exact), region

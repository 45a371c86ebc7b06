"""--panel / --out_panel on the command line without a GPU: every new refusal exits 2 before a file is opened, in the order
DESIGN §23 gives, and the refusals that stood before still win over the new ones."""
import os

import pytest

from krisp_amd import krisp_fasta as KF

NOWHERE = ["/nonexistent/in0.fa", "/nonexistent/in1.fa", "--outgroup", "/nonexistent/out0.fa", "-c", "30", "-d", "40"]
DESIGN = ["--design-primers", "--primer_size", "18", "24", "--amp_size", "70", "100"]


def _refused(argv, tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        KF.main(NOWHERE + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("ERROR: ") and err.count("\n") == 1
    assert os.listdir(tmp_path) == []
    return err


@pytest.mark.parametrize("flags, word", [
    (["--panel", "8", "--out_panel", "p.tsv"], "--panel needs --design-primers"),
    (["--panel", "8"], "--panel needs --design-primers"),
    (DESIGN + ["--panel", "0", "--out_panel", "p.tsv"], "--panel must lie between 1 and 64 (got 0)"),
    (DESIGN + ["--panel", "65", "--out_panel", "p.tsv"], "--panel must lie between 1 and 64 (got 65)"),
    (DESIGN + ["--panel", "-3", "--out_panel", "p.tsv"], "--panel must lie between 1 and 64 (got -3)"),
    (DESIGN + ["--out_panel", "p.tsv"], "--out_panel needs --panel"),
    (["--out_panel", "p.tsv"], "--out_panel needs --panel"),
    (DESIGN + ["--panel", "8"], "--panel needs --out_panel"),
    (DESIGN + ["--out_guides", "g.tsv", "--panel", "64"], "--panel needs --out_panel"),
])
def test_the_new_refusals(flags, word, tmp_path, capsys, monkeypatch):
    assert word in _refused(flags, tmp_path, capsys, monkeypatch)


def test_primer3_with_panel_is_refused(tmp_path, capsys, monkeypatch):
    """(--panel needs --design-primers, which --primer3 excludes: whichever of the refusals speaks, the run ends before a file
    is read; panel_refusal's own line for --primer3 is pinned in test_panel_host.py)"""
    err = _refused(["--primer3", "--panel", "8", "--out_panel", "p.tsv"], tmp_path, capsys, monkeypatch)
    assert "--primer3" in err or "--panel needs --design-primers" in err
    err = _refused(DESIGN + ["--primer3", "--panel", "8", "--out_panel", "p.tsv"], tmp_path, capsys, monkeypatch)
    assert "--design-primers cannot be combined with --primer3" in err


@pytest.mark.parametrize("flags, word", [
    # the designer's own figures are checked before the panel's
    (["--design-primers", "--primer_size", "5", "35", "--panel", "0"], "--primer_size within 10 .. 60"),
    # an output that needs another one
    (DESIGN + ["--out_guide_hits", "h.tsv", "--panel", "8"], "--out_guide_hits needs --out_guides"),
    (["--out_primer_products", "x.tsv", "--panel", "8", "--out_panel", "p.tsv"], "--out_primer_products needs --design-primers"),
])
def test_existing_refusals_still_win(flags, word, tmp_path, capsys, monkeypatch):
    assert word in _refused(flags, tmp_path, capsys, monkeypatch)


def test_the_options_parse():
    a = KF.build_parser().parse_args(NOWHERE + DESIGN + ["--panel", "8", "--out_panel", "p.tsv"])
    assert a.panel == 8 and a.out_panel == "p.tsv"
    a = KF.build_parser().parse_args(NOWHERE)
    assert a.panel is None and a.out_panel is None

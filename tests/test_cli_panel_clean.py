"""The command line's checks of --panel-clean (krisp_fasta._check_options, reports.panel_clean_refusal) without a GPU: every
new refusal, exit status 2 and one line on stderr before a genome is read, their place behind every existing check --
panel_products_refusal among them --, and the runs that reach the discovery.  (tests/test_cli_refusals.py holds the existing
checks to their golden; the new option is in none of its cases.)"""
import io
from contextlib import redirect_stderr
from unittest import mock

from krisp_amd import krisp_fasta as KF

BASE = ["no_such_file.fa", "-c", "30", "-a", "100"]
PANEL = ["--design-primers", "--panel", "8", "--out_panel", "p"]
CLEAN = ["--panel-clean"]
ROWS = ["--out_panel_products", "x"]


class _Started(Exception):
    pass


def _start(*a, **k):
    raise _Started()


def run(argv):
    """-> "started" for a run that reaches the discovery, else (exit status, stderr)"""
    err = io.StringIO()
    with mock.patch.object(KF, "find_regions", _start), mock.patch.object(KF, "find_regions_multi_device", _start), \
            mock.patch.object(KF, "find_regions_distributed", _start):
        try:
            with redirect_stderr(err):
                KF.main(BASE + argv)
        except _Started:
            return "started"
        except SystemExit as e:
            return e.code, err.getvalue()
    raise AssertionError("main() came back")


def refused(argv, piece):
    got = run(argv)
    assert got != "started", argv
    code, text = got
    assert code == 2 and text.startswith("ERROR: ") and text.endswith("\n") and text.count("\n") == 1, (argv, got)
    assert piece in text, (argv, text)
    return text


def test_the_runs_that_start():
    assert run(PANEL + CLEAN) == "started"
    assert run(PANEL + CLEAN + ["--primer-mismatches", "0"]) == "started"         # (the two figures count with the option alone)
    assert run(PANEL + CLEAN + ["--max-product", "500"]) == "started"
    assert run(PANEL + CLEAN + ["--primer-mismatches", "3", "--max-product", "150", "--omit-soft"]) == "started"
    assert run(PANEL + CLEAN + ROWS + ["--out_panel_summary", "y"]) == "started"
    assert run(PANEL + CLEAN + ["--amp_size", "70", "100", "--primer_size", "25", "60", "--max-product", "120"]) == "started"
    assert run(PANEL) == "started"                                                  # (and without it, as before)


def test_the_new_refusals():
    assert refused(CLEAN, "needs --panel") == "ERROR: --panel-clean needs --panel (the selection it keeps clean)\n"
    refused(CLEAN + ["--design-primers"], "--panel-clean needs --panel")
    for m in ("4", "-1"):
        refused(PANEL + CLEAN + ["--primer-mismatches", m], f"--primer-mismatches must lie between 0 and 3 (got {m})")
    refused(PANEL + CLEAN + ["--max-product", "149"], "the upper bound of --amp_size, 150 bases (got 149)")
    refused(PANEL + CLEAN + ["--amp_size", "70", "100", "--primer_size", "25", "60", "--max-product", "119"],
            "twice the upper bound of --primer_size, 120 bases (got 119)")
    refused(PANEL + CLEAN + ["--max-product", "2147483648"], "smaller than 2^31")


def test_the_order_among_the_new_refusals():
    bad = ["--primer-mismatches", "4", "--max-product", "10"]
    refused(CLEAN + bad, "needs --panel")                                           # the panel first
    refused(PANEL + CLEAN + bad, "--primer-mismatches must lie")                    # then the distance
    refused(PANEL + CLEAN + ["--max-product", "10"], "--amp_size")                  # the designed product before two primers


def test_every_existing_check_comes_first():
    # the golden text of the figures without an output does not name the new option, and stands without it
    for fig in (["--primer-mismatches", "2"], ["--max-product", "500"]):
        refused(PANEL + fig, fig[0] + " needs --out_products or --out_primer_products or --out_assay_hits\n")
    # panel_products_refusal is tried before panel_clean_refusal: its wording names the oligos, the new one the primers
    refused(CLEAN + ROWS, "--out_panel_products needs --panel")
    text = refused(PANEL + CLEAN + ROWS + ["--amp_size", "70", "100", "--primer_size", "25", "60", "--max-product", "119"], "120 bases")
    assert "two oligos of the panel" in text
    text = refused(PANEL + CLEAN + ["--amp_size", "70", "100", "--primer_size", "25", "60", "--max-product", "119"], "120 bases")
    assert "two primers of the candidates" in text
    # the designer's own, the other outputs' and the panel's refusals win over the new one
    refused(CLEAN + ["--primer3", "--design-primers"], "--design-primers cannot be combined with --primer3")
    refused(PANEL + CLEAN + ["--primer-mismatches", "4", "--primer_size", "5", "35"], "--primer_size")
    refused(CLEAN + ["--near-mismatches", "2"], "--near-mismatches needs --out_near")
    refused(CLEAN + ["--hairpins"], "--hairpins needs --design-primers")
    refused(CLEAN + ["--out_guide_hits", "h"], "--out_guide_hits needs --out_guides")
    refused(CLEAN + ["--out_panel", "p"], "--out_panel needs --panel")
    refused(CLEAN + ["--panel", "8", "--out_panel", "p"], "--panel needs --design-primers")
    refused(CLEAN + ["--design-primers", "--panel", "65", "--out_panel", "p", "--primer-mismatches", "4"], "between 1 and 64")
    refused(CLEAN + ["--design-primers", "--panel", "8", "--primer-mismatches", "4"], "--panel needs --out_panel")


def test_the_help_names_the_option():
    text = KF.build_parser().format_help()
    assert "--panel-clean" in text and "dropped_cross" in text

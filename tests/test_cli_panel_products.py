"""The command line's checks of --out_panel_products and --out_panel_summary (krisp_fasta._check_options, reports.
panel_products_refusal) without a GPU: every new refusal, exit status 2 and one line on stderr, their place behind every
existing check, and the runs that reach the discovery.  (tests/test_cli_refusals.py holds the existing checks to their
golden; the new options are in none of its cases.)"""
import io
from contextlib import redirect_stderr
from unittest import mock

import pytest

from krisp_amd import krisp_fasta as KF

BASE = ["no_such_file.fa", "-c", "30", "-a", "100"]
PANEL = ["--design-primers", "--panel", "8", "--out_panel", "p"]
ROWS, SUMMARY = ["--out_panel_products", "x"], ["--out_panel_summary", "y"]


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


@pytest.mark.parametrize("out", [ROWS, SUMMARY, ROWS + SUMMARY])
def test_the_runs_that_start(out):
    assert run(PANEL + out) == "started"
    assert run(PANEL + out + ["--primer-mismatches", "0"]) == "started"           # (the two figures also alone)
    assert run(PANEL + out + ["--max-product", "500"]) == "started"
    assert run(PANEL + out + ["--primer-mismatches", "3", "--max-product", "150", "--omit-soft"]) == "started"
    assert run(PANEL + out + ["--primer_size", "20", "30", "--max-product", "150"]) == "started"
    assert run(PANEL) == "started"                                                  # (and without them, as before)


def test_the_new_refusals():
    assert refused(ROWS, "needs --panel") == "ERROR: --out_panel_products needs --panel (the oligos it searches for)\n"
    assert refused(SUMMARY, "needs --panel") == "ERROR: --out_panel_summary needs --panel (the oligos it searches for)\n"
    refused(ROWS + SUMMARY, "--out_panel_products needs --panel")
    refused(ROWS + ["--design-primers"], "--out_panel_products needs --panel")
    for out in (ROWS, SUMMARY):
        for m in ("4", "-1"):
            refused(PANEL + out + ["--primer-mismatches", m], f"--primer-mismatches must lie between 0 and 3 (got {m})")
        refused(PANEL + out + ["--max-product", "149"], "the upper bound of --amp_size, 150 bases (got 149)")
        refused(PANEL + out + ["--amp_size", "70", "100", "--primer_size", "25", "60", "--max-product", "119"],
                "twice the upper bound of --primer_size, 120 bases (got 119)")
        assert run(PANEL + out + ["--amp_size", "70", "100", "--primer_size", "25", "60", "--max-product", "120"]) == "started"
        refused(PANEL + out + ["--max-product", "2147483648"], "smaller than 2^31")


def test_the_order_among_the_new_refusals():
    bad = ["--primer-mismatches", "4", "--max-product", "10"]
    refused(ROWS + bad, "needs --panel")                                            # the panel first
    refused(PANEL + ROWS + bad, "--primer-mismatches must lie")                     # then the distance
    refused(PANEL + ROWS + ["--max-product", "10"], "--amp_size")                   # the designed product before two oligos


def test_every_existing_check_comes_first():
    # the golden text of the figures without an output does not name the new options, and stands without them
    for fig in (["--primer-mismatches", "2"], ["--max-product", "500"]):
        refused(PANEL + fig, fig[0] + " needs --out_products or --out_primer_products or --out_assay_hits\n")
        refused(fig, fig[0] + " needs --out_products or --out_primer_products or --out_assay_hits\n")
    # the designer's own, the other outputs' and the panel's refusals win over the new ones
    refused(ROWS + ["--primer3", "--design-primers"], "--design-primers cannot be combined with --primer3")
    refused(PANEL + ROWS + ["--primer-mismatches", "4", "--primer_size", "5", "35"], "--primer_size")
    refused(ROWS + ["--near-mismatches", "2"], "--near-mismatches needs --out_near")
    refused(ROWS + ["--hairpins"], "--hairpins needs --design-primers")
    refused(ROWS + ["--out_primer_products", "z"], "--out_primer_products needs --design-primers")
    refused(PANEL + ROWS + ["--out_primer_products", "z", "--max-product", "2147483648"], "smaller than 2^31")
    refused(ROWS + ["--out_guide_hits", "h"], "--out_guide_hits needs --out_guides")
    refused(ROWS + ["--guide-candidates", "4"], "--guide-candidates")
    refused(ROWS + ["--out_panel", "p"], "--out_panel needs --panel")
    refused(ROWS + ["--panel", "8", "--out_panel", "p"], "--panel needs --design-primers")
    refused(ROWS + ["--design-primers", "--panel", "65", "--out_panel", "p", "--primer-mismatches", "4"], "between 1 and 64")
    refused(ROWS + ["--design-primers", "--panel", "8", "--primer-mismatches", "4"], "--panel needs --out_panel")


def test_the_help_names_both_options():
    text = KF.build_parser().format_help()
    assert "--out_panel_products PATH" in text and "--out_panel_summary PATH" in text

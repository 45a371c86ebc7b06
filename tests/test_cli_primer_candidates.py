"""The refusals of --primer-candidates and --out_primer_candidates (krisp_fasta._check_options), in the manner of
test_cli_guide_candidates.py: the run itself is stubbed, no input file exists; a case either exits 2 with one line on stderr,
before a file is opened, or reaches the discovery.  The existing primer refusals still win where both apply."""
import io
from contextlib import redirect_stderr
from unittest import mock

import pytest

from krisp_amd import krisp_fasta as KF

BASE = ["no_such_file.fa", "-c", "30", "-a", "100"]
OUT = ["--outgroup", "no_such_outgroup.fa"]
DESIGN = ["--design-primers"]


class _Started(Exception):
    pass


def _start(*a, **k):
    raise _Started()


def _run(argv):
    """"started", or the one line a refusal wrote"""
    err = io.StringIO()
    with mock.patch.object(KF, "find_regions", _start), mock.patch.object(KF, "find_regions_multi_device", _start), \
            mock.patch.object(KF, "find_regions_distributed", _start), mock.patch("builtins.open", side_effect=AssertionError("a file is opened")):
        try:
            with redirect_stderr(err):
                KF.main(BASE + argv)
        except _Started:
            return "started"
        except SystemExit as e:
            text = err.getvalue()
            assert e.code == 2 and text.startswith("ERROR: ") and text.count("\n") == 1 and text.endswith("\n"), (e.code, text)
            return text[len("ERROR: "):-1]
    raise AssertionError("main() came back")


@pytest.mark.parametrize("argv, why", [
    (OUT + ["--primer-candidates", "4"], "--primer-candidates needs --design-primers (the pairs it picks)"),
    (["--primer-candidates", "4"], "--primer-candidates needs --design-primers (the pairs it picks)"),
    (OUT + ["--primer-candidates", "4", "--primer3"],
     "--primer-candidates cannot be combined with --primer3 (the pairs Primer3 designs are not re-ranked)"),
    (OUT + DESIGN + ["--primer-candidates", "0"], "--primer-candidates must lie between 1 and 8 (got 0)"),
    (OUT + DESIGN + ["--primer-candidates", "9"], "--primer-candidates must lie between 1 and 8 (got 9)"),
    (OUT + DESIGN + ["--primer-candidates", "-2"], "--primer-candidates must lie between 1 and 8 (got -2)"),
    (OUT + DESIGN + ["--out_primer_candidates", "c"], "--out_primer_candidates needs --primer-candidates"),
    (OUT + ["--out_primer_candidates", "c"], "--out_primer_candidates needs --primer-candidates"),
    # needs --design-primers comes before the value
    (OUT + ["--primer-candidates", "9"], "--primer-candidates needs --design-primers (the pairs it picks)"),
    # the search's own figures, checked as --out_primer_products checks them, in its words
    (OUT + DESIGN + ["--primer-candidates", "4", "--primer-mismatches", "4"], "--primer-mismatches must lie between 0 and 3 (got 4)"),
    (OUT + DESIGN + ["--primer-candidates", "4", "--primer-mismatches", "-1"], "--primer-mismatches must lie between 0 and 3 (got -1)"),
    (OUT + DESIGN + ["--primer-candidates", "4", "--max-product", "149"],
     "--max-product must be at least the upper bound of --amp_size, 150 bases (got 149): the designed product itself would not be found"),
    (OUT + DESIGN + ["--primer-candidates", "4", "--amp_size", "70", "1200"],
     "--max-product must be at least the upper bound of --amp_size, 1200 bases (got 1000): the designed product itself would not be found"),
    (OUT + DESIGN + ["--primer-candidates", "4", "--max-product", str(1 << 31)],
     f"--max-product must be smaller than 2^31 bases (got {1 << 31})"),
])
def test_every_new_refusal(argv, why):
    assert _run(argv) == why


@pytest.mark.parametrize("argv", [
    OUT + DESIGN + ["--primer-candidates", "1"],
    DESIGN + ["--primer-candidates", "4"],                                   # (all files are searched: no outgroup is needed)
    OUT + DESIGN + ["--primer-candidates", "8", "--out_primer_candidates", "c"],
    OUT + DESIGN + ["--primer-candidates", "4", "--primer-mismatches", "3", "--max-product", "150"],
    OUT + DESIGN + ["--primer-candidates", "4", "--primer-mismatches", "0", "--omit-soft"],
    OUT + DESIGN + ["--primer-candidates", "4", "--hairpins"],
    OUT + DESIGN + ["--primer-candidates", "4", "--out_primer_products", "p", "--out_guides", "g", "--out_assay_hits", "a"],
    OUT + DESIGN + ["--primer-candidates", "4", "--out_guides", "g", "--guide-candidates", "4"],
    OUT + DESIGN + ["--primer-candidates", "4", "--panel", "3", "--out_panel", "q", "--out_panel_products", "r"],
])
def test_what_the_checks_take(argv):
    assert _run(argv) == "started"


@pytest.mark.parametrize("argv, why", [
    # the existing refusals keep their place and their words when a new one applies too
    (OUT + DESIGN + ["--primer-candidates", "9", "--primer3"], "--design-primers cannot be combined with --primer3 (one designer at a time)"),
    (OUT + DESIGN + ["--primer-candidates", "9", "--out_products", "p"],
     "--out_products cannot be combined with --design-primers (the regions the designer keeps are not searched)"),
    (OUT + DESIGN + ["--primer-candidates", "0", "--primer_size", "9", "20"], None),
    (OUT + ["--primer-candidates", "4", "--hairpins"], "--hairpins needs --design-primers (it is the designer's own check; Primer3 has PRIMER_MAX_HAIRPIN_TH)"),
    (OUT + ["--primer-candidates", "4", "--out_primer_products", "p"], "--out_primer_products needs --design-primers"),
    (OUT + DESIGN + ["--out_primer_candidates", "c", "--primer-mismatches", "1"],
     "--primer-mismatches needs --out_products or --out_primer_products or --out_assay_hits"),
    (OUT + DESIGN + ["--out_primer_candidates", "c", "--max-product", "500"],
     "--max-product needs --out_products or --out_primer_products or --out_assay_hits"),
    (OUT + DESIGN + ["--primer-candidates", "0", "--out_primer_products", "p", "--primer-mismatches", "4"],
     "--primer-mismatches must lie between 0 and 3 (got 4)"),
    (OUT + DESIGN + ["--primer-candidates", "0", "--out_near", "n"],
     "--out_near cannot be combined with --design-primers (the regions the designer keeps are not searched)"),
])
def test_an_existing_refusal_still_wins(argv, why):
    got = _run(argv)
    if why is None:
        # (the designer's own refusal, whatever its words: the same as without the new option)
        assert got == _run([a for a in argv if a not in ("--primer-candidates", "0")]) != "started"
    else:
        assert got == why

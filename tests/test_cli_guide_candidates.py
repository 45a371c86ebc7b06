"""The refusals of --guide-candidates and --out_guide_candidates (krisp_fasta._check_options), in the manner of
test_cli_refusals.py: the run itself is stubbed, no input file exists; a case either exits 2 with one line on stderr, before
a file is opened, or reaches the discovery.  The existing guide refusals still win where both apply."""
import io
from contextlib import redirect_stderr
from unittest import mock

import pytest

from krisp_amd import krisp_fasta as KF

BASE = ["no_such_file.fa", "-c", "30", "-a", "100"]
OUT = ["--outgroup", "no_such_outgroup.fa"]
GUIDES = ["--out_guides", "g"]


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
    (OUT + ["--guide-candidates", "4"], "--guide-candidates needs --out_guides (the guides it picks)"),
    (OUT + GUIDES + ["--guide-candidates", "0"], "--guide-candidates must lie between 1 and 8 (got 0)"),
    (OUT + GUIDES + ["--guide-candidates", "9"], "--guide-candidates must lie between 1 and 8 (got 9)"),
    (OUT + GUIDES + ["--guide-candidates", "-2"], "--guide-candidates must lie between 1 and 8 (got -2)"),
    (GUIDES + ["--guide-candidates", "4"], "--guide-candidates needs an --outgroup file (the genomes its candidates are searched in)"),
    (OUT + GUIDES + ["--out_guide_candidates", "c"], "--out_guide_candidates needs --guide-candidates"),
    (OUT + ["--out_guide_candidates", "c"], "--out_guide_candidates needs --guide-candidates"),
    # needs --out_guides comes before the value and the outgroup
    (["--guide-candidates", "9"], "--guide-candidates needs --out_guides (the guides it picks)"),
    (GUIDES + ["--guide-candidates", "9"], "--guide-candidates must lie between 1 and 8 (got 9)"),
    # the search's own figures, checked as --out_guide_hits checks them, in today's words
    (OUT + GUIDES + ["--guide-candidates", "4", "--guide-hit-mismatches", "4"], "--guide-hit-mismatches must lie between 0 and 3 (got 4)"),
    (OUT + GUIDES + ["--guide-candidates", "4", "--guide-hits-need-pam"], "--guide-hits-need-pam needs a motif: --pam5 or --pam3"),
])
def test_every_new_refusal(argv, why):
    assert _run(argv) == why


@pytest.mark.parametrize("argv", [
    OUT + GUIDES + ["--guide-candidates", "1"],
    OUT + GUIDES + ["--guide-candidates", "8", "--out_guide_candidates", "c"],
    OUT + GUIDES + ["--guide-candidates", "4", "--guide-hit-mismatches", "3"],
    OUT + GUIDES + ["--guide-candidates", "4", "--guide-hit-mismatches", "0", "--guide-hits-need-pam", "--pam5", "TTTV"],
    OUT + GUIDES + ["--guide-candidates", "4", "--out_guide_hits", "h", "--guide-hit-bulges", "1"],
    OUT + GUIDES + ["--guide-candidates", "4", "--design-primers", "--out_assay_hits", "a"],
])
def test_what_the_checks_take(argv):
    assert _run(argv) == "started"


@pytest.mark.parametrize("argv, why", [
    # the existing refusals keep their place and their words when a new one applies too
    (OUT + ["--guide-candidates", "9", "--guide-size", "20"], "--guide-size needs --out_guides"),
    (OUT + GUIDES + ["--guide-candidates", "9", "--guide-size", "11"], "--guide-size must lie between 12 and 40 (got 11)"),
    (OUT + GUIDES + ["--guide-candidates", "9", "--primer3"], "--out_guides cannot be combined with --primer3 (the regions Primer3 keeps get no guide)"),
    (OUT + ["--guide-candidates", "4", "--out_guide_hits", "h"], "--out_guide_hits needs --out_guides (the guides it searches for)"),
    (OUT + GUIDES + ["--out_guide_candidates", "c", "--guide-hit-mismatches", "1"], "--guide-hit-mismatches needs --out_guide_hits or --out_assay_hits"),
    (OUT + GUIDES + ["--out_guide_candidates", "c", "--guide-hits-need-pam"], "--guide-hits-need-pam needs --out_guide_hits or --out_assay_hits"),
    (OUT + GUIDES + ["--guide-candidates", "4", "--guide-hit-bulges", "1"], "--guide-hit-bulges needs --out_guide_hits"),
    (OUT + GUIDES + ["--guide-candidates", "0", "--out_guide_hits", "h", "--guide-hit-mismatches", "4"],
     "--guide-hit-mismatches must lie between 0 and 3 (got 4)"),
    (OUT + GUIDES + ["--guide-candidates", "0", "--out_assay_hits", "a"], None),
])
def test_an_existing_refusal_still_wins(argv, why):
    got = _run(argv)
    if why is None:
        # (the assay join's own refusal, whatever its words: the same as without the new option)
        assert got == _run([a for a in argv if a not in ("--guide-candidates", "0")]) != "started"
    else:
        assert got == why

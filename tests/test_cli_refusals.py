"""Which refusal wins: the command line's option checks (krisp_fasta._check_options) against a golden recorded from the
commit before main() was split into steps (tests/golden/cli_refusals.json).  Every fragment below alone and every
unordered pair of them, over a packed and a wide geometry; the run itself is stubbed: a case either exits 2 with one
line on stderr or reaches the discovery.  `python tests/test_cli_refusals.py` prints the golden of the checked-out code."""
import ast
import inspect
import io
import itertools
import json
import os
import sys
import textwrap
from contextlib import redirect_stderr
from unittest import mock

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from krisp_amd import krisp_fasta as KF
from krisp_amd import primers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_refusals.json")
BASES = [["-c", "12", "-a", "28"], ["-c", "30", "-a", "100"]]
GUIDE_HITS = ["--out_guides", "g", "--out_guide_hits", "h"]
ASSAY = ["--design-primers", "--out_guides", "g", "--out_assay_hits", "a"]
# one fragment or more for every option the checks read, at a value they take and at one they refuse; the longer ones
# reach the checks that stand behind two or three options
FRAGMENTS = [
    ["--primer3"], ["--no-primer3"], ["--design-primers"], ["--hairpins"],
    ["--tm", "55", "65"], ["--tm", "68", "53"], ["--tm", "53", "2000"], ["--gc", "45", "65"], ["--gc", "70", "40"],
    ["--amp_size", "80", "140"], ["--amp_size", "150", "70"], ["--amp_size", "70", "2000"],
    ["--primer_size", "20", "30"], ["--primer_size", "5", "35"], ["--primer_size", "35", "25"],
    ["--max_sec_tm", "45"], ["--max_sec_tm", "2000"], ["--gc_clamp", "2"], ["--gc_clamp", "99"],
    ["--max_end_gc", "3"], ["--max_end_gc", "-1"],
    ["--out_locations", "x"],
    ["--out_near", "x"], ["--near-mismatches", "2"], ["--near-mismatches", "4"], ["--near-mismatches", "-1"],
    ["--out_products", "x"], ["--out_primer_products", "x"],
    ["--primer-mismatches", "2"], ["--primer-mismatches", "4"],
    ["--max-product", "500"], ["--max-product", "10"], ["--max-product", "100"], ["--max-product", "2147483648"],
    ["--out_guides", "x"],
    ["--guide-size", "20"], ["--guide-size", "16"], ["--guide-size", "11"], ["--guide-size", "29"], ["--guide-size", "41"],
    ["--pam5", "TTTV"], ["--pam5", "Z"], ["--pam3", "H"], ["--pam3", "ACGTACGTA"],
    ["--guide-gc", "20", "80"], ["--guide-gc", "70", "30"],
    ["--guide-min-mismatches", "2"], ["--guide-min-mismatches", "99"],
    ["--out_guide_hits", "x"], GUIDE_HITS,
    ["--guide-hit-mismatches", "1"], ["--guide-hit-mismatches", "3"], ["--guide-hit-mismatches", "4"],
    ["--guide-hit-bulges", "0"], ["--guide-hit-bulges", "1"], ["--guide-hit-bulges", "3"],
    ["--guide-hits-need-pam"],
    GUIDE_HITS + ["--guide-hit-bulges", "1"], GUIDE_HITS + ["--guide-hits-need-pam"],
    ["--out_assay_hits", "x"], ["--design-primers", "--out_assay_hits", "a"], ["--out_guides", "g", "--out_assay_hits", "a"],
    ASSAY, ASSAY + ["--guide-hits-need-pam"],
]


class _Started(Exception):
    pass


def _start(*a, **k):
    raise _Started()


def cases():
    """(name, argv) of every run: a base, then one fragment or two"""
    picks = [(f,) for f in FRAGMENTS] + list(itertools.combinations(FRAGMENTS, 2))
    for base in BASES:
        for pick in picks:
            argv = base + [tok for f in pick for tok in f]
            yield " | ".join(" ".join(f) for f in (base,) + pick), ["no_such_file.fa"] + argv


ABSENT = " | primer3-py absent"


def record():
    """{case: [2, stderr text] for a refusal, "started" for a run that reaches the discovery}.  primer3-py counts as
    installed, whatever the machine holds, but for --primer3 alone, recorded once more as if it were not"""
    out = {}
    with mock.patch.object(KF, "find_regions", _start), mock.patch.object(KF, "find_regions_multi_device", _start), \
            mock.patch.object(KF, "find_regions_distributed", _start):
        out.update(_record(cases(), True))
        out.update(_record(((" ".join(b) + " | --primer3" + ABSENT, ["no_such_file.fa"] + b + ["--primer3"]) for b in BASES), False))
    return out


def _record(runs, primer3_installed):
    out = {}
    with mock.patch.object(primers, "available", lambda: primer3_installed):
        for name, argv in runs:
            err = io.StringIO()
            try:
                with redirect_stderr(err):
                    KF.main(argv)
                raise AssertionError(f"{name}: main() came back")
            except _Started:
                out[name] = "started"
            except SystemExit as e:
                out[name] = [e.code, err.getvalue()]
    return out


@pytest.fixture(scope="module")
def recorded():
    return record()


def compact(recorded):
    """the golden's form: the distinct records once, then their index for every case, in record()'s order"""
    outcomes = []
    for v in recorded.values():
        if v not in outcomes:
            outcomes.append(v)
    return {"bases": BASES, "fragments": FRAGMENTS, "outcomes": outcomes, "cases": [outcomes.index(v) for v in recorded.values()]}


def dump(golden, f, per_line=60):
    """compact()'s result as JSON, a line per record and per `per_line` cases"""
    def rows(items):
        return ",\n".join("  " + json.dumps(x) for x in items)
    idx = golden["cases"]
    f.write('{"bases": ' + json.dumps(golden["bases"]) + ',\n "fragments": [\n' + rows(golden["fragments"]) + '],\n "outcomes": [\n'
            + rows(golden["outcomes"]) + '],\n "cases": [\n'
            + ",\n".join("  " + json.dumps(idx[i:i + per_line])[1:-1] for i in range(0, len(idx), per_line)) + "]}\n")


@pytest.fixture(scope="module")
def golden():
    """the golden file as record() would give it: {case: record}"""
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["bases"] == BASES and g["fragments"] == FRAGMENTS, "the golden was recorded for another list of cases"
    names = [name for name, _ in cases()] + [" ".join(b) + " | --primer3" + ABSENT for b in BASES]
    assert len(names) == len(g["cases"])
    return {name: g["outcomes"][i] for name, i in zip(names, g["cases"])}


def test_every_case_gives_what_the_parent_gave(recorded, golden):
    n = len(FRAGMENTS)
    assert len(recorded) == len(BASES) * (n + n * (n - 1) // 2 + 1)        # (no case skipped, none named twice)
    assert set(recorded) == set(golden)
    wrong = {k: (recorded[k], golden[k]) for k in golden if recorded[k] != golden[k]}
    assert not wrong, f"{len(wrong)} cases differ, the first: {sorted(wrong.items())[0]}"


def test_a_refusal_is_exit_2_and_one_line(golden):
    for name, got in golden.items():
        if got != "started":
            code, err = got
            assert code == 2 and err.startswith("ERROR: ") and err.count("\n") == 1 and err.endswith("\n"), name


def test_the_golden_holds_enough_of_both(golden):
    refused = sum(1 for v in golden.values() if v != "started")
    assert 3 * refused >= len(golden)
    assert 10 * (len(golden) - refused) >= len(golden)


def _message_literals(fn):
    """the pieces of message text in fn's source: every string constant with a blank in it (f-strings give their constant
    pieces), the docstrings left out"""
    tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
    docs = {id(node.body[0].value) for node in ast.walk(tree)
            if isinstance(node, (ast.FunctionDef, ast.Module)) and node.body and isinstance(node.body[0], ast.Expr)
            and isinstance(node.body[0].value, ast.Constant)}
    return sorted({node.value for node in ast.walk(tree)
                   if isinstance(node, ast.Constant) and isinstance(node.value, str) and " " in node.value.strip()
                   and id(node) not in docs})


def test_every_message_of_the_checks_is_in_the_golden(golden):
    texts = [v[1] for v in golden.values() if v != "started"]
    literals = _message_literals(KF._check_options)
    assert len(literals) >= 10
    for piece in literals:
        assert any(piece in t for t in texts), f"no case is refused with {piece!r}"


if __name__ == "__main__":
    dump(compact(record()), sys.stdout)

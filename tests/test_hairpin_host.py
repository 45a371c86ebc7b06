"""The hairpin figure of --design-primers --hairpins without a GPU: the loop table and the known answers of the
definition, stems counted by hand against the brute-force reference (hairpin_reference.py), what the filter does to a
region's answer, the refusals, the rendered texts, and the census of the GPU test's cases (hairpin_cases.py)."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import primers, thermo
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_reference as DR                                              # noqa: E402
import hairpin_cases as HC                                                 # noqa: E402
import hairpin_reference as HR                                             # noqa: E402


def test_the_known_answers_of_the_definition():
    assert HR.hairpin_figure("GGGGCCAAAAGGCCCC") == 329126
    assert HR.hairpin_figure("GCAAAGC") == 226484
    assert HR.hairpin_figure("GCAAGC") == 0                 # its only stem would have a loop of 2


def test_the_loop_table():
    want = {3: -11285, 4: -11285, 5: -10640, 6: -12897, 11: -15476, 30: -20313, 56: -23666}
    assert {l: thermo.LOOP_DS[l] for l in want} == want
    assert thermo.HAIRPIN_MIN_LOOP == 3 and len(thermo.LOOP_DS) == 64
    assert thermo.LOOP_DG37[3] == 3500 and thermo.LOOP_DG37[30] == 6300 and thermo.loop_dg37(11) == 4800
    assert all(v < 0 for v in thermo.LOOP_DS[3:57]) and not any(thermo.LOOP_DS[:3]) and not any(thermo.LOOP_DS[57:])
    h = thermo.hairpin_params()
    assert list(h.loop_ds) == thermo.LOOP_DS and isinstance(h, thermo.HairpinParams)


def _shape(x):
    return [s[:4] for s in HR.stems(x)]


def test_stems_counted_by_hand():
    # a stem that holds the oligo's first and its last base: GC....GC on fold 7
    assert _shape("GCAAAAGC") == [(7, 0, 1, 4)]
    # one at the first base only, one at the last base only (T tails do not pair with anything here)
    assert _shape("GCTTTTGCTT") == [(7, 0, 1, 4)]
    assert _shape("TTGCTTTTGC") == [(11, 2, 3, 4)]
    # two stems on one fold, split by the mismatch A/A: two runs, valued apart
    x = "GGCACCGTTTTCGGAGCC"
    st = HR.stems(x)
    assert [s[:4] for s in st if s[0] == 17] == [(17, 0, 2, 12), (17, 4, 6, 4)]
    assert st[[s[:2] for s in st].index((17, 0))][4] == HR.stem_tm(x, 0, 2, 12)
    assert st[[s[:2] for s in st].index((17, 4))][4] == HR.stem_tm(x, 4, 6, 4)
    assert HR.stem_tm(x, 0, 2, 12) != HR.stem_tm(x, 4, 6, 4) and HR.hairpin_figure(x) == max(s[4] for s in st)
    # its own reverse complement: the pairs run inwards, the run is cut where 3 bases are left, not dropped
    assert _shape("GGCATGCC") == [(7, 0, 1, 4)]
    assert _shape("GGCCATGGCC")[0] == (9, 0, 2, 4)
    # a loop of 2 is no stem, and neither is a single pair
    assert _shape("GCAAGC") == [] and _shape("GAAAAC") == [] and _shape("GTTTTTTC") == []
    # the figure is the stem's Tm with the loop's dS: by hand for GCAAAGC (step GC, two terminals G and C, loop 3)
    dh = thermo.NN_DH[4 * 2 + 1] + thermo.TERM_DH[2] + thermo.TERM_DH[1]
    ds = thermo.NN_DS[4 * 2 + 1] + thermo.TERM_DS[2] + thermo.TERM_DS[1] + thermo.SALT_DS + thermo.LOOP_DS[3]
    assert HR.hairpin_figure("GCAAAGC") == (dh * 10 ** 6) // ds == 226484


def test_the_filter_changes_a_winner_and_takes_a_regions_only_pair():
    """from the cases' census set: a region whose plain winner falls to its hairpin alone, and one left without a pair"""
    name, sec = "30_40_30", 20
    hp, pl = HC.reference(name, sec), HC.reference(name, sec, hairpins=False)
    changed = [i for i in range(len(hp)) if hp["found"][i] and HR.plain(hp[i:i + 1]).tobytes() != pl[i:i + 1].tobytes()]
    lost = [i for i in range(len(hp)) if pl["found"][i] and not hp["found"][i]]
    assert changed and lost
    for i in changed + lost:
        # the plain winner passed every other filter, so its hairpin figure alone removed it
        assert max(HR.hairpin_figure(x) for x in HR.winner_sequences(HC.templates(name)[i], pl[i])) > thermo.mk(sec)
    for i in changed:
        assert hp["pair_penalty"][i] >= pl["pair_penalty"][i]
        assert max(hp["left_hairpin"][i], hp["right_hairpin"][i]) <= thermo.mk(sec)
    assert not hp[lost].tobytes().strip(b"\0")
    assert HR.design(HC.templates(name)[:2], 30, 40, 30, hairpins=False, **HC.options(name, sec)).dtype.itemsize == 64


def test_hairpins_alone_is_refused_before_a_genome_is_read(capsys):
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_file.fasta", "--conserved", "30", "--amplicon", "100", "--hairpins"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("ERROR: --hairpins needs --design-primers") and err.count("\n") == 1
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_file.fasta", "--conserved", "30", "--amplicon", "100", "--hairpins", "--primer3"])
    assert e.value.code == 2 and "--hairpins needs --design-primers" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:          # the designer's own refusals hold with the option
        KF.main(["no_such_file.fasta", "--conserved", "30", "--amplicon", "100", "--design-primers", "--hairpins",
                 "--primer_size", "5", "20"])
    assert e.value.code == 2 and "--primer_size" in capsys.readouterr().err


def test_the_texts_with_and_without_the_figures():
    from krisp_amd import _native
    t = "ACGTTGCAAGGCTAGCTAGGATCCATGCAAGT" * 4
    rec = {"found": 1, "product_size": 100, "pair_penalty": 1500, "left_start": 2, "left_len": 20, "right_start": 82, "right_len": 20,
           "left_tm": 330000, "right_tm": 331250, "left_gc": 10, "right_gc": 11, "left_penalty": 700, "right_penalty": 800,
           "left_self_any": 0, "left_self_end": 0, "right_self_any": 280000, "right_self_end": 0, "pair_any": 0, "pair_end": 0}
    plain = primers.design_fields(t, rec)
    assert "left_hairpin" not in plain and "Hairpin" not in primers.design_stats_text(plain)
    with_hp = primers.design_fields(t, dict(rec, left_hairpin=0, right_hairpin=299126))
    assert {k: v for k, v in with_hp.items() if k not in primers.HAIRPIN_COLUMNS} == plain
    assert with_hp["left_hairpin"] == thermo.celsius(0) == "-273.150" and with_hp["right_hairpin"] == "25.976"
    text = primers.design_stats_text(with_hp)
    head = text.split("\n")[2].split()
    assert head[head.index("End") + 1] == "Hairpin" and head[-1] == "Penalty" and "25.976" in text
    assert text.replace("  Hairpin ", "").count("\n") == primers.design_stats_text(plain).count("\n")
    assert primers.HAIRPIN_COLUMNS == ["left_hairpin", "right_hairpin"] and primers.DESIGN_COLUMNS[-1] == "pair_compl_end"
    # a structured row of either dtype
    a = np.zeros(1, dtype=_native.DESIGN_RECORD_HP)
    for k, v in dict(rec, left_hairpin=0, right_hairpin=299126).items():
        a[k] = v
    assert primers.design_fields(t, a[0]) == with_hp and primers.design_fields(t, HR.plain(a)[0]) == plain
    assert _native.DESIGN_RECORD_HP.itemsize == 72 and _native.DESIGN_RECORD_HP.names[:19] == _native.DESIGN_RECORD.names
    assert primers.render_designed([], None, a[:0])[0] == \
        "left_seq,diag_seq,right_seq," + ",".join(primers.DESIGN_COLUMNS + primers.HAIRPIN_COLUMNS) + "\n"
    assert primers.render_designed([], None, HR.plain(a)[:0])[0] == "left_seq,diag_seq,right_seq," + ",".join(primers.DESIGN_COLUMNS) + "\n"


@pytest.mark.parametrize("name", [n for n in HC.CASES if n != "256_60_256"])
def test_the_census_of_the_gpu_cases(name):
    """from the reference alone: every option set holds at least one region of each kind it is meant to show"""
    for sec, kinds in HC.CASES[name]["sets"].items():
        c = HC.census(name, sec)
        print(name, sec, c)
        assert 0 < c["found"] and all(c[k] > 0 for k in kinds), (sec, c)
    assert any("round2" in k for n in HC.CASES for k in HC.CASES[n]["sets"].values())

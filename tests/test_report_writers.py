"""The TSV writers of the report passes, byte for byte: for every row dtype two rows -- one with an empty record ID, one of
an RNA genome (U in the sequence), one on the '-' strand -- against the text the hand-written writers gave before they
became calls of one generic writer."""
import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

SHARED = [("a.fa", "", 0, 5, "+"), ("dir/b.fna.gz", "chr 2|x", 3, 1234567890123, "-")]      # file, record, index, start, strand


def _rows(dtype, extra):
    """two rows of `dtype`: region 7 and 4000000000, SHARED's columns, `extra` = the other columns of each row"""
    rows = np.empty(2, dtype=dtype)
    for i, (region, more) in enumerate(zip((7, 4000000000), extra)):
        rows[i]["region"] = region
        rows[i]["file"], rows[i]["record"], rows[i]["record_index"], rows[i]["start"], rows[i]["strand"] = SHARED[i]
        for name, v in more.items():
            rows[i][name] = v
    return rows


LOCATION = _rows(KF.LOCATION, [dict(end=9, sequence="ACGU"), dict(end=1234567890127, sequence="ugca")])
NEAR = _rows(KF.NEAR, [dict(target="ACGT", end=9, mismatches=0, flank_mismatches=0, sequence="ACGU"),
                       dict(target="TGCA", end=1234567890127, mismatches=3, flank_mismatches=2, sequence="UGGG")])
PRODUCT = _rows(KF.PRODUCT, [dict(end=105, length=100, left_mismatches=0, right_mismatches=1, left_end_mismatches=0,
                                  right_end_mismatches=1),
                             dict(end=1234567891123, length=1000, left_mismatches=3, right_mismatches=2, left_end_mismatches=2,
                                  right_end_mismatches=0)])
GUIDE_HIT = _rows(KF.GUIDE_HIT, [dict(end=9, mismatches=0, mismatch_columns="-", pam5_match=1, pam3_match=0, sequence="ACGU"),
                                 dict(end=1234567890127, mismatches=2, mismatch_columns="1,4", pam5_match=0, pam3_match=1,
                                      sequence="UGCA")])
GUIDE_BULGE_HIT = _rows(KF.GUIDE_BULGE_HIT, [
    dict(end=10, mismatches=1, mismatch_columns="2", pam5_match=1, pam3_match=1, sequence="ACGUA", bulge="DNA", bulge_size=1,
         bulge_column="3"),
    dict(end=1234567890126, mismatches=0, mismatch_columns="-", pam5_match=0, pam3_match=1, sequence="UGC", bulge="RNA", bulge_size=1,
         bulge_column="2")])
ASSAY_HIT = _rows(KF.ASSAY_HIT, [
    dict(end=105, length=100, left_mismatches=0, right_mismatches=1, left_end_mismatches=0, right_end_mismatches=1, guide_start=40,
         guide_end=44, guide_strand="-", guide_mismatches=0, mismatch_columns="-", pam5_match=1, pam3_match=0, orientation="reverse",
         sequence="ACGU"),
    dict(end=1234567891123, length=1000, left_mismatches=3, right_mismatches=2, left_end_mismatches=2, right_end_mismatches=0,
         guide_start=1234567890200, guide_end=1234567890204, guide_strand="+", guide_mismatches=2, mismatch_columns="1,4",
         pam5_match=0, pam3_match=1, orientation="design", sequence="UGCA")])

A = "7\ta.fa\t\t0\t5\t"                                                 # region, file, record, record_index, start of row 0
B = "4000000000\tdir/b.fna.gz\tchr 2|x\t3\t1234567890123\t"            # ... and of row 1
WANT = {
    "LOCATION": "region\tfile\trecord\trecord_index\tstart\tend\tstrand\tsequence\n"
                + A + "9\t+\tACGU\n"
                + B + "1234567890127\t-\tugca\n",
    "NEAR": "region\ttarget\tfile\trecord\trecord_index\tstart\tend\tstrand\tmismatches\tflank_mismatches\tsequence\n"
            "7\tACGT\ta.fa\t\t0\t5\t9\t+\t0\t0\tACGU\n"
            "4000000000\tTGCA\tdir/b.fna.gz\tchr 2|x\t3\t1234567890123\t1234567890127\t-\t3\t2\tUGGG\n",
    "PRODUCT": "region\tfile\trecord\trecord_index\tstart\tend\tstrand\tlength\tleft_mismatches\tright_mismatches\t"
               "left_end_mismatches\tright_end_mismatches\n"
               + A + "105\t+\t100\t0\t1\t0\t1\n"
               + B + "1234567891123\t-\t1000\t3\t2\t2\t0\n",
    "GUIDE_HIT": "region\tfile\trecord\trecord_index\tstart\tend\tstrand\tmismatches\tmismatch_columns\tpam5_match\tpam3_match\t"
                 "sequence\n"
                 + A + "9\t+\t0\t-\t1\t0\tACGU\n"
                 + B + "1234567890127\t-\t2\t1,4\t0\t1\tUGCA\n",
    "GUIDE_BULGE_HIT": "region\tfile\trecord\trecord_index\tstart\tend\tstrand\tmismatches\tmismatch_columns\tpam5_match\t"
                       "pam3_match\tsequence\tbulge\tbulge_size\tbulge_column\n"
                       + A + "9\t+\t0\t-\t1\t0\tACGU\t-\t0\t-\n"
                       + A + "10\t+\t1\t2\t1\t1\tACGUA\tDNA\t1\t3\n"
                       + B + "1234567890126\t-\t0\t-\t0\t1\tUGC\tRNA\t1\t2\n"
                       + B + "1234567890127\t-\t2\t1,4\t0\t1\tUGCA\t-\t0\t-\n",
    "ASSAY_HIT": "region\tfile\trecord\trecord_index\tproduct_start\tproduct_end\tproduct_strand\tlength\tleft_mismatches\t"
                 "right_mismatches\tleft_end_mismatches\tright_end_mismatches\tguide_start\tguide_end\tguide_strand\t"
                 "guide_mismatches\tmismatch_columns\tpam5_match\tpam3_match\torientation\tsequence\n"
                 + A + "105\t+\t100\t0\t1\t0\t1\t40\t44\t-\t0\t-\t1\t0\treverse\tACGU\n"
                 + B + "1234567891123\t-\t1000\t3\t2\t2\t0\t1234567890200\t1234567890204\t+\t2\t1,4\t0\t1\tdesign\tUGCA\n",
}


def _written(tmp_path, write, *args):
    path = tmp_path / "out.tsv"
    write(str(path), *args)
    with open(path, newline="") as f:
        return f.read()


CASES = {
    "LOCATION": (KF.write_locations, (LOCATION,)),
    "NEAR": (KF.write_near, (NEAR,)),
    "PRODUCT": (KF.write_products, (PRODUCT,)),
    "GUIDE_HIT": (KF.write_guide_hits, (GUIDE_HIT,)),
    # (the unbulged rows take -, 0, - in the bulge columns and merge with the bulged ones by region, file, ...)
    "GUIDE_BULGE_HIT": (KF.write_guide_bulge_hits, (GUIDE_HIT, GUIDE_BULGE_HIT, ["a.fa", "dir/b.fna.gz"])),
    "ASSAY_HIT": (KF.write_assay_hits, (ASSAY_HIT,)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_written_file_is_the_text_the_earlier_writers_gave(name, tmp_path):
    write, args = CASES[name]
    assert _written(tmp_path, write, *args) == WANT[name]

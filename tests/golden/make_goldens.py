#!/usr/bin/env python3
"""Generate golden vectors by RUNNING the reference (grunwaldlab/krisp) in the
build container.  This script is the only place that imports /root/reference;
it is never executed on the GPU box (the reference tree does not travel) and
nothing else in the repo imports it.  Its outputs -- the *.json / *.gz data
files next to it -- are plain input/expected-output vectors.

How the reference is imported:
  * krisp.kstream imports as-is (stdlib only).
  * krisp.krisp_fasta.* import colorama, primer3, prettytable and
    Bio.Data.IUPACData at module top; none is installed (no network).  They are
    registered as in-memory placeholder modules: colours -> '', primer3 /
    PrettyTable -> never called (no --primer3 case is generated), and
    IUPACData.ambiguous_dna_values -> the standard IUPAC DNA table.  Only that
    table influences output (the CSV consensus letter, Amplicon.py:10-12,65);
    README.md:121-123 pins AC->M and GT->K of it.

Usage:  python3 tests/golden/make_goldens.py        (from the repo root)
"""
import gzip
import hashlib
import io
import json
import os
import random
import shutil
import sys
import tempfile
import types
from contextlib import redirect_stdout
from pathlib import Path

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, f"{REF}/src")


def _install_placeholders():
    col = types.ModuleType("colorama")

    class _Blank:
        def __getattr__(self, name):
            return ""
    col.Fore = col.Back = col.Style = _Blank()
    sys.modules["colorama"] = col
    p3 = types.ModuleType("primer3")
    sys.modules["primer3"] = p3
    pt = types.ModuleType("prettytable")
    pt.PrettyTable = object
    sys.modules["prettytable"] = pt
    bio = types.ModuleType("Bio")
    data = types.ModuleType("Bio.Data")
    iu = types.ModuleType("Bio.Data.IUPACData")
    iu.ambiguous_dna_values = {
        "A": "A", "C": "C", "G": "G", "T": "T", "M": "AC", "R": "AG",
        "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG", "H": "ACT",
        "D": "AGT", "B": "CGT", "X": "GATC", "N": "GATC"}
    bio.Data = data
    data.IUPACData = iu
    sys.modules["Bio"] = bio
    sys.modules["Bio.Data"] = data
    sys.modules["Bio.Data.IUPACData"] = iu


_install_placeholders()
from krisp.kstream import kstream  # noqa: E402
from krisp.krisp_fasta import krisp_fasta as KF  # noqa: E402
from krisp.krisp_fasta.intersectAmplicons import mergeFiles  # noqa: E402
from krisp.krisp_fasta.filterAlignments import filterAlignments  # noqa: E402
from krisp.krisp_fasta.shared import simplename  # noqa: E402
from krisp.krisp_fasta.Amplicon import ConservedEndAmplicons  # noqa: E402


def sha(b):
    return hashlib.sha256(b).hexdigest()


# --------------------------------------------------------------------------
# 1. kstream-level cases
# --------------------------------------------------------------------------
def run_kstream(kwargs, seqs=None, file_text=None, fname="in.fa", use_write=False):
    """Returns {'out': [...]} or {'raises': 'KeyError'}"""
    with tempfile.TemporaryDirectory() as td:
        src = seqs
        if file_text is not None:
            src = os.path.join(td, fname)
            if fname.endswith(".gz"):
                with gzip.open(src, "wt") as f:
                    f.write(file_text)
            else:
                with open(src, "w") as f:
                    f.write(file_text)
        try:
            ks = kstream(**kwargs)
            if use_write:
                outp = os.path.join(td, "out.txt")
                n = ks.write(outp, src)
                with open(outp) as f:
                    lines = f.read().split("\n")
                assert lines[-1] == ""
                return {"out": lines[:-1], "count": n}
            return {"out": list(ks(src))}
        except Exception as e:  # noqa: BLE001
            return {"raises": type(e).__name__, "msg": str(e)}


def kstream_cases():
    cases = []

    def add(name, kwargs, seqs=None, file_text=None, fname="in.fa", use_write=False):
        res = run_kstream(kwargs, seqs, file_text, fname, use_write)
        cases.append({"name": name, "kwargs": kwargs, "seqs": seqs,
                      "file_text": file_text, "fname": fname,
                      "use_write": use_write, **res})

    kf = dict(kmers=6, complements=True, disallow="Nn", split=[3, -1],
              sort=True, sortcols=[0, 2])
    adv = "ACGTacgtNACGTTRACGTA"
    add("adv_mapsoft", dict(kf, mapsoft=True), [adv])
    add("adv_omitsoft", dict(kf, omitsoft=True), [adv])
    add("adv_mapsoft_write", dict(kf, mapsoft=True), [adv], use_write=True)
    add("palindrome", dict(kmers=4, complements=True), ["ACGT"])
    add("split_R0", dict(kmers=6, split=[3, 0]), ["ACGTAC"])
    add("split_L0", dict(kmers=6, split=[0, -2]), ["ACGTAC"])
    add("split_int", dict(kmers=6, split=2), ["ACGTAC"])
    add("rna", dict(kmers=4, complements=True), ["ACGUAC"])
    add("rna_sorted_write", dict(kmers=4, complements=True, sort=True), ["ACGUAC", "UUGCA"], use_write=True)
    add("illegal_X", dict(kmers=4, complements=True), ["ACGXAC"])
    add("illegal_X_omit_lower", dict(kmers=4, complements=True, omitsoft=True), ["ACGxAC"])
    add("illegal_dash_omit", dict(kmers=4, complements=True, omitsoft=True), ["ACG-AC"])
    add("nonletter_only_omit", dict(kmers=3, complements=True, omitsoft=True), ["ACG123TT"])
    add("omit_and_map", dict(kmers=4, omitsoft=True, mapsoft=True), ["ACGT"])
    add("canon_and_comp", dict(kmers=4, canonicals=True, complements=True), ["ACGT"])
    add("canonicals", dict(kmers=5, canonicals=True), ["ACGTTGCAAT", "TTTTTAAAAA"])
    add("allow", dict(kmers=3, allow="ACGT"), ["ACGTNACGRT"])
    add("disallow", dict(kmers=3, disallow="Nn"), ["ACGTNACnGT"])
    add("expandiupac", dict(kmers=3, expandiupac=True), ["ARGNT"])
    add("multi_k", dict(kmers=[3, 5]), ["ACGTAC", "GG", "TTTTT"])
    add("no_k_passthrough", dict(complements=True), ["ACG", "TTA"])
    add("sorted_plain", dict(kmers=3, sort=True), ["GATTACA"])
    add("too_short", dict(kmers=8, complements=True), ["ACGT", "ACGTACGTA"])
    fasta = ">r1 desc\nACGTAC\n  GTTA  \n\n>r2\n>r3\nAC\n>r4\nTTGACCA\nGG\n"
    add("fasta_basic", dict(kmers=5, complements=True, disallow="Nn", mapsoft=True,
                            split=[2, -2], sort=True, sortcols=[0, 2]),
        file_text=fasta, fname="x.fasta")
    add("fasta_gz_write", dict(kmers=5, complements=True, disallow="Nn", mapsoft=True,
                               split=[2, -2], sort=True, sortcols=[0, 2]),
        file_text=fasta, fname="x.fasta.gz", use_write=True)
    nonfasta = "ACGTAC\n>notheader\nGGTTAA\n"
    add("nonfasta_later_gt", dict(kmers=4), file_text=nonfasta, fname="x.txt")
    add("fasta_header_midline", dict(kmers=4), file_text="AC>GT\nACGTA\n", fname="y.txt")
    add("fasta_rna_file", dict(kmers=4, complements=True, sort=True),
        file_text=">a\nACGUACGU\n>b\nGGUUAACC\n", fname="r.fa", use_write=True)
    # random soft-masked / N / IUPAC genomes through the krisp_fasta combination
    rng = random.Random(7)
    for i, (L, D, R) in enumerate([(3, 1, 2), (4, 2, 3), (5, 0, 5), (2, 3, 0), (0, 2, 3), (7, 1, 2)]):
        recs = []
        for r in range(3):
            n = rng.randint(5, 60)
            s = "".join(rng.choice("ACGT" * 10 + "acgt" * 2 + "NnRYK") for _ in range(n))
            recs.append(s)
        text = "".join(f">rec{j}\n{s}\n" for j, s in enumerate(recs))
        for mode in ("mapsoft", "omitsoft"):
            kw = dict(kmers=L + D + R, complements=True, disallow="Nn",
                      split=[L, -R], sort=True, sortcols=[0, 2])
            kw[mode] = True
            add(f"rand{i}_{mode}_{L}_{D}_{R}", kw, file_text=text, fname=f"g{i}.fa", use_write=True)
    return cases


def kstream_cases_more():
    """kstream option combinations beyond the krisp_fasta one that the device path also serves
    (strand mode x soft-mask rule x split x sort columns); written to kstream_cases_more.json."""
    cases = []

    def add(name, kwargs, seqs=None, file_text=None, fname="in.fa", use_write=False):
        res = run_kstream(kwargs, seqs, file_text, fname, use_write)
        cases.append({"name": name, "kwargs": kwargs, "seqs": seqs,
                      "file_text": file_text, "fname": fname,
                      "use_write": use_write, **res})

    rng = random.Random(11)
    texts = []
    for i in range(3):
        recs = []
        for r in range(3):
            n = rng.randint(8, 90)
            recs.append("".join(rng.choice("ACGT" * 12 + "acgt" * 2 + "Nn") for _ in range(n)))
        texts.append("".join(f">rec{j} x\n{s}\n" for j, s in enumerate(recs)))
    strands = {"comp": dict(complements=True), "canon": dict(canonicals=True), "fwd": {}}
    n = 0
    for sname, skw in strands.items():
        for mode in ("mapsoft", "omitsoft"):
            for split, cols in ((None, None), ([3, -2], None), ([3, -2], [0, 2]), ([4], None), ([2, -3], [0]),
                                ([0, -3], [0, 2]), ([5, 0], [0, 2])):
                kw = dict(kmers=7, disallow="Nn", sort=True, **skw)
                kw[mode] = True
                if split is not None:
                    kw["split"] = split
                if cols is not None:
                    kw["sortcols"] = cols
                text = texts[n % len(texts)]
                add(f"more{n}_{sname}_{mode}_{split}_{cols}", kw, file_text=text, fname=f"m{n % 3}.fa",
                    use_write=bool(n % 2))
                n += 1
    add("more_canon_palindromes", dict(kmers=4, canonicals=True, disallow="Nn", mapsoft=True, sort=True),
        ["ACGTACGTTTAAACGCGT", "aattAATTGGCC"])
    add("more_fwd_rna", dict(kmers=5, disallow="Nn", mapsoft=True, sort=True, split=[2, -1]),
        ["ACGUUGCAUUAG", "GGGuuuACG"], use_write=True)
    add("more_canon_k32", dict(kmers=32, canonicals=True, disallow="Nn", mapsoft=True, sort=True),
        ["".join(rng.choice("ACGT") for _ in range(80))])
    return cases


def kstream_cases_routes():
    """Reference vectors for every kstream route the device serves beyond kstream_cases_more() (round 5):
    every --sort-cols list over 2- and 3-field splits (all permutations, partial and repeated lists, empty fields,
    split=[a, 0]), --expand-iupac / --allow / kept lower case under --sort, several k with sort columns, k > 32 through
    kstream -- on inputs with N, lower case, IUPAC letters, RNA and several records -- plus the option sets that stay on
    the host chain (other disallow sets, N windows surviving, unsorted streams with IUPAC letters, the (last, middle,
    first) order with unequal outer widths), so that the chain itself is pinned there.  Written to
    kstream_cases_routes.json.  sort semantics pinned: kstream.py:83-119 runs GNU `sort -t, -kN,N ...`."""
    import itertools
    cases = []

    def add(name, kwargs, seqs=None, file_text=None, fname="in.fa", use_write=False):
        res = run_kstream(kwargs, seqs, file_text, fname, use_write)
        cases.append({"name": name, "kwargs": kwargs, "seqs": seqs,
                      "file_text": file_text, "fname": fname,
                      "use_write": use_write, **res})

    rng = random.Random(505)
    plain = "ACGT" * 12 + "acgt" * 3 + "Nn"
    iupac = "ACGT" * 14 + "acgt" * 2 + "Nn" + "RYKMSWBDHVry"

    def fasta(alphabet, nrec, lo, hi):
        recs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(nrec)]
        return "".join(f">rec{j} d\n{s}\n" for j, s in enumerate(recs))

    texts = [fasta(plain, 3, 8, 36), fasta(iupac, 4, 8, 36), fasta(plain, 2, 20, 44),
             fasta(iupac, 3, 10, 40).replace("T", "U").replace("t", "u")]
    strands = [("comp", dict(complements=True)), ("canon", dict(canonicals=True)), ("fwd", {})]
    softs = [("map", dict(mapsoft=True)), ("omit", dict(omitsoft=True)), ("keep", {})]
    # ---- A. every column list over 2- and 3-field lines
    k = 7
    n = 0
    for split in ([3], [0], [7], [3, -2], [2, -2], [0, -3], [5, 0], [3, -4]):
        nf = len(split) + 1
        lists = [list(p) for r in range(1, nf + 1) for p in itertools.permutations(range(nf), r)]
        lists += [[0, 0], [1, 0, 1]] if nf == 2 else [[2, 2, 1], [1, 1], [0, 2, 0]]
        for cols in lists:
            sname, skw = strands[n % 3]
            mname, mkw = softs[(n // 3) % 3]
            kw = dict(kmers=k, disallow="Nn", sort=True, split=split, sortcols=cols, **skw, **mkw)
            add(f"cols{n}_{sname}_{mname}_{split}_{cols}", kw, file_text=texts[n % len(texts)],
                fname=f"c{n % len(texts)}.fa", use_write=bool((n // 2) % 2))
            n += 1
    # ---- B. --expand-iupac under --sort
    n = 0
    for (sname, skw), (mname, mkw) in itertools.product(strands, softs):
        for split, cols in (((None, None), ([3, -2], [0, 2])) if n % 2 else (([4], [1]), ([2, -3], [2, 1]))):
            kw = dict(kmers=7, disallow="Nn", sort=True, expandiupac=True, **skw, **mkw)
            if split is not None:
                kw["split"] = split
            if cols is not None:
                kw["sortcols"] = cols
            add(f"expand{n}_{sname}_{mname}_{split}_{cols}", kw, file_text=texts[1 + 2 * (n % 2)],
                fname="e.fa", use_write=bool(n % 3 == 0))
            n += 1
    add("expand_no_disallow_sorted", dict(kmers=4, sort=True, expandiupac=True, mapsoft=True), ["ACGNTRAC", "nnAC"])
    add("expand_unsorted_comp", dict(kmers=5, complements=True, disallow="Nn", expandiupac=True), ["ACGRTYACGT", "ACnGTAACGW"])
    # ---- C. --allow under --sort
    n = 0
    for allow in ("ACGT", "ACGTacgt", "ACGTN", "AC", "ACGTRY", "ATat", "CGNn"):
        for (sname, skw) in strands:
            mname, mkw = softs[n % 3]
            split, cols = [(None, None), ([3, -2], [0, 2]), ([3], [1]), ([2, -3], [1, 0])][n % 4]
            kw = dict(kmers=5, allow=allow, sort=True, **skw, **mkw)
            if n % 2:
                kw["disallow"] = "Nn"
            if split is not None:
                kw["split"] = split
            if cols is not None:
                kw["sortcols"] = cols
            add(f"allow{n}_{allow}_{sname}_{mname}_{split}_{cols}", kw, file_text=texts[n % len(texts)],
                fname="a.fa", use_write=bool(n % 2))
            n += 1
    # ---- D. lower case kept (no soft-mask rule) under --sort, heavy lower case
    lower = "ACGT" * 4 + "acgt" * 4 + "NnRy"
    ltext = fasta(lower, 3, 12, 40)
    n = 0
    for (sname, skw) in strands:
        for split, cols in ((None, None), ([3, -2], [0, 2]), ([3, -2], [1]), ([2], [1, 0])):
            kw = dict(kmers=6, disallow="Nn", sort=True, **skw)
            if split is not None:
                kw["split"] = split
            if cols is not None:
                kw["sortcols"] = cols
            add(f"keepcase{n}_{sname}_{split}_{cols}", kw, file_text=ltext, fname="l.fa", use_write=bool(n % 2))
            n += 1
    # ---- E. several k with sort columns
    n = 0
    for ks in ([3, 5], [7, 4, 6], [5, 5], [8, 6]):
        for split, cols in ((None, None), ([2, -1], [0, 2]), ([3], [1]), ([2, -1], [2, 1, 0]), ([1, -2], [1])):
            sname, skw = strands[n % 3]
            mname, mkw = softs[(n // 2) % 3]
            kw = dict(kmers=ks, disallow="Nn", sort=True, **skw, **mkw)
            if split is not None:
                kw["split"] = split
            if cols is not None:
                kw["sortcols"] = cols
            add(f"multik{n}_{ks}_{sname}_{mname}_{split}_{cols}", kw, file_text=texts[n % len(texts)],
                fname="k.fa", use_write=bool(n % 2))
            n += 1
    add("multik_unsorted", dict(kmers=[4, 6], complements=True, disallow="Nn", mapsoft=True, split=[2, -1]),
        file_text=texts[0], fname="k.fa")
    # ---- F. k > 32 through kstream (the krisp_fasta combination and its neighbours)
    longalpha = "ACGT" * 40 + "acgt" * 2 + "N" + "R"
    for n, (kk, L, R, mname, nrec, lo, hi) in enumerate([(33, 30, 2, "mapsoft", 3, 40, 120), (40, 16, 16, "omitsoft", 3, 50, 140),
                                                        (100, 30, 30, "mapsoft", 2, 110, 170), (36, 30, 6, "mapsoft", 4, 30, 90),
                                                        (70, 33, 20, "omitsoft", 2, 80, 150)]):
        recs = ["".join(rng.choice(longalpha) for _ in range(rng.randint(lo, hi))) for _ in range(nrec)]
        recs.append(recs[0][5:5 + kk + 6])                      # repeated windows: equal lines
        text = "".join(f">r{j}\n{s}\n" for j, s in enumerate(recs))
        if n == 3:
            text = text.replace("T", "U").replace("t", "u")
        kw = dict(kmers=kk, complements=True, disallow="Nn", split=[L, -R], sort=True, sortcols=[0, 2])
        kw[mname] = True
        add(f"longk{n}_{kk}_{L}_{R}_{mname}", kw, file_text=text, fname="w.fa", use_write=bool(n % 2))
    lt = "".join(rng.choice("ACGT" * 30 + "N" + "acgt") for _ in range(120))
    add("longk_fwd_nosplit", dict(kmers=40, disallow="Nn", mapsoft=True, sort=True), [lt])
    add("longk_canon_split", dict(kmers=35, canonicals=True, disallow="Nn", mapsoft=True, sort=True, split=[10, -10],
                                  sortcols=[0, 2]), [lt])
    add("longk_unsorted", dict(kmers=34, complements=True, disallow="Nn", omitsoft=True, split=[12, -12]), [lt])
    # ---- G. option sets that stay on the host chain
    t = texts[1]
    add("host_disallow_other", dict(kmers=5, complements=True, disallow="RrN", mapsoft=True, sort=True), file_text=t, fname="h.fa")
    add("host_disallow_N_only", dict(kmers=5, disallow="N", sort=True, split=[2, -1], sortcols=[0, 2]), file_text=t, fname="h.fa")
    add("host_no_disallow_sorted", dict(kmers=5, complements=True, mapsoft=True, sort=True, split=[2, -1], sortcols=[0, 2]),
        file_text=t, fname="h.fa", use_write=True)
    add("host_unsorted_iupac", dict(kmers=6, complements=True, disallow="Nn", mapsoft=True, split=[2, -2]), file_text=t, fname="h.fa")
    add("host_unsorted_keepcase", dict(kmers=6, canonicals=True, disallow="Nn"), file_text=ltext, fname="h.fa")
    add("host_order_210_unequal", dict(kmers=7, complements=True, disallow="Nn", mapsoft=True, split=[3, -2], sort=True,
                                        sortcols=[2, 1, 0]), file_text=texts[0], fname="h.fa")
    add("host_cols_beyond_fields", dict(kmers=6, disallow="Nn", mapsoft=True, split=[3], sort=True, sortcols=[2, 0]),
        file_text=texts[0], fname="h.fa")
    add("host_three_splits", dict(kmers=8, disallow="Nn", mapsoft=True, split=[2, 2, -2], sort=True, sortcols=[1, 3]),
        file_text=texts[0], fname="h.fa")
    return cases


def kstream_cases_r6():
    """round 6 (VERDICT r5 missing #5): split lists of any length (kstream.py:805-832 takes any) -- sorted in line order, by
    column lists that cut the window into at most three blocks (device) or more (host chain), unsorted, with several k --
    and the sets that stay on the host chain (two sizes counted from the end).  Written to kstream_cases_r6.json."""
    cases = []

    def add(name, kwargs, seqs=None, file_text=None, fname="in.fa", use_write=False):
        res = run_kstream(kwargs, seqs, file_text, fname, use_write)
        cases.append({"name": name, "kwargs": kwargs, "seqs": seqs,
                      "file_text": file_text, "fname": fname,
                      "use_write": use_write, **res})

    rng = random.Random(606)
    plain = "ACGT" * 12 + "acgt" * 3 + "Nn"
    iupac = "ACGT" * 14 + "acgt" * 2 + "Nn" + "RYKMSWry"

    def fasta(alphabet, nrec, lo, hi):
        recs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(nrec)]
        return "".join(f">rec{j} d\n{s}\n" for j, s in enumerate(recs))

    texts = [fasta(plain, 3, 10, 40), fasta(iupac, 4, 10, 40), fasta(plain, 2, 24, 50),
             fasta(iupac, 3, 12, 40).replace("T", "U").replace("t", "u")]
    strands = [("comp", dict(complements=True)), ("canon", dict(canonicals=True)), ("fwd", {})]
    softs = [("map", dict(mapsoft=True)), ("omit", dict(omitsoft=True)), ("keep", {})]
    n = 0
    for k, split, collists in [
            (9, [2, 3, -2], [None, [0], [3], [2, 3], [3, 0], [1, 2], [0, 1, 2, 3], [3, 2], [1, 3], [2, 0]]),
            (8, [1, 2, 3], [None, [3], [1, 2], [2, 3, 0], [3, 1]]),
            (8, [2, -3, 1], [None, [3], [1], [2, 3]]),
            (9, [2, 2, 2, -2], [None, [4], [3, 4], [1, 2, 3], [4, 0, 1], [2, 0]]),
            (7, [-2], [None, [1], [1, 0]]),
            (7, [-3, 2], [None, [2], [1, 2], [2, 0]]),
            (8, [0, 3, -0], [None, [2], [3, 1]]),
            (8, [3, -2, -1], [None, [3], [2, 3]]),              # two sizes from the end: host chain
            (8, [8, 0, -0], [None]),
    ]:
        for cols in collists:
            sname, skw = strands[n % 3]
            mname, mkw = softs[(n // 3) % 3]
            kw = dict(kmers=k, disallow="Nn", sort=True, split=split, **skw, **mkw)
            if cols is not None:
                kw["sortcols"] = cols
            add(f"msplit{n}_{sname}_{mname}_{split}_{cols}", kw, file_text=texts[n % len(texts)],
                fname=f"m{n % len(texts)}.fa", use_write=bool((n // 2) % 2))
            n += 1
    # unsorted streams and several k
    for j, (k, split) in enumerate([(9, [2, 3, -2]), (8, [1, 2, 3]), (7, [-2]), (9, [2, 2, 2, -2]), (8, [3, -2, -1])]):
        sname, skw = strands[j % 3]
        mname, mkw = softs[(j + 1) % 3]
        add(f"msplit_unsorted{j}_{sname}_{mname}_{split}", dict(kmers=k, disallow="Nn", split=split, **skw, **mkw),
            file_text=texts[j % len(texts)], fname="u.fa", use_write=bool(j % 2))
    add("msplit_multik_sorted", dict(kmers=[7, 9], complements=True, disallow="Nn", mapsoft=True, sort=True, split=[2, 2, -2],
                                     sortcols=[2, 3]), file_text=texts[0], fname="k.fa")
    add("msplit_multik_unsorted", dict(kmers=[6, 8], disallow="Nn", omitsoft=True, split=[1, 2, -1]), file_text=texts[2], fname="k.fa")
    add("msplit_expand", dict(kmers=8, complements=True, disallow="Nn", mapsoft=True, sort=True, expandiupac=True, split=[2, 2, -2],
                              sortcols=[3, 0]), file_text=texts[1], fname="e.fa")
    add("msplit_allow", dict(kmers=8, allow="ACGT", sort=True, split=[3, 2, -1], sortcols=[2]), file_text=texts[1], fname="a.fa")
    # --allow / --disallow sets that leave bases the two strands do not share, sorted: a window and its reverse complement
    # are filtered each by itself (kstream.py:696-766 -- the complements are formed first)
    low_t = fasta("ACG" * 10 + "T" + "acg" + "N", 4, 30, 80)
    for j, (kw, text) in enumerate([
            (dict(kmers=5, complements=True, allow="ACG", sort=True, mapsoft=True), low_t),
            (dict(kmers=4, complements=True, disallow="TtNn", sort=True, mapsoft=True, split=[1, -1], sortcols=[2, 0]), low_t),
            (dict(kmers=6, complements=True, allow="ACGacg", sort=True, split=[2, 2]), low_t),
            (dict(kmers=5, complements=True, disallow="A", sort=True, omitsoft=True, split=[2]), texts[0]),
            (dict(kmers=4, complements=True, allow="CGT", disallow="Nn", sort=True, mapsoft=True, split=[1, 1, -1], sortcols=[3]), texts[1]),
            (dict(kmers=[4, 5], complements=True, allow="AG", sort=True, mapsoft=True), low_t),
    ]):
        add(f"strandsplit{j}", kw, file_text=text, fname="s.fa", use_write=bool(j % 2))
    # ... and in stream order: a window, then its reverse complement, each kept or dropped by itself
    rna_t = fasta("ACG" * 8 + "T" * 2 + "acg" + "N" + "RY", 3, 20, 60).replace("T", "U").replace("t", "u")
    for j, (kw, text) in enumerate([
            (dict(kmers=5, complements=True, allow="ACG", mapsoft=True), low_t),
            (dict(kmers=4, complements=True, disallow="TtNn", mapsoft=True, split=[1, -1]), low_t),
            (dict(kmers=6, complements=True, allow="ACGacg", split=[2, 2]), low_t),
            (dict(kmers=5, complements=True, disallow="A", omitsoft=True, split=[2]), texts[0]),
            (dict(kmers=4, complements=True, allow="CGT", disallow="Nn", mapsoft=True, split=[1, 1, -1]), texts[1]),
            (dict(kmers=5, complements=True, disallow="GgNn", mapsoft=True), texts[1]),
            (dict(kmers=4, complements=True, disallow="AaNn", omitsoft=True, split=[-2]), rna_t),
            (dict(kmers=[4, 5], complements=True, allow="AG", mapsoft=True), low_t),              # several k: host chain
    ]):
        add(f"strandsplit_unsorted{j}", kw, file_text=text, fname="s.fa", use_write=bool(j % 2))
    return cases


# --------------------------------------------------------------------------
# 2. krisp_fasta-level cases (stages + final text)
# --------------------------------------------------------------------------
def canon_lines(path):
    with open(path) as f:
        lines = [ln for ln in f.read().split("\n") if ln]
    return sorted(lines)


def _maybe_hashed(lines, hash_big):
    """canonicalised lines as they are, or -- long amplicons: megabytes of text -- their count and the sha256 of
    '\\n'.join(lines) (tests/ compare through the same function)"""
    if hash_big and sum(len(x) + 1 for x in lines) > 65536:
        return {"lines": len(lines), "sha256": sha("\n".join(lines).encode())}
    return lines


def run_fasta_case(name, files, ingroup, outgroup, L, D, R, omit=False, dot=False,
                   keep_sorted=False, main_args=None, run_main=True, hash_big=False):
    """files: {filename: bytes}.  Runs stages (for intermediates) and main()
    (for the final text), both with cores=1."""
    k = L + D + R
    out = {"name": name, "ingroup": ingroup, "outgroup": outgroup, "L": L, "D": D,
           "R": R, "omit_soft": omit, "dot": dot}
    with tempfile.TemporaryDirectory() as td:
        paths = {}
        for fn, content in files.items():
            p = os.path.join(td, fn)
            with open(p, "wb") as f:
                f.write(content)
            paths[fn] = p
        work = os.path.join(td, "work")
        os.mkdir(work)
        # ---- stages
        kfiles = []
        sorted_info = {}
        for fn in ingroup + outgroup:
            kf = f"{work}/{KF.basename(Path(fn).name)}.{k}mers"
            KF.extractSortedKmers(paths[fn], L, R, k, kf, "80%", 1, False, omit)
            data = open(kf, "rb").read()
            sorted_info[fn] = {"sha256": sha(data), "lines": data.count(b"\n"),
                               "bytes": len(data)}
            if keep_sorted and fn == ingroup[0]:
                with gzip.GzipFile(HERE / f"{name}.{fn}.{k}mers.gz", "wb", mtime=0) as g:
                    g.write(data)
            kfiles.append(kf)
        out["sorted"] = sorted_info
        merged = f"{work}/merged_file.txt"
        mergeFiles(list(kfiles), merged, 1, work, False)
        out["merged_canon"] = _maybe_hashed(canon_lines(merged), hash_big)
        if k > L + R:
            filt = f"{work}/filtered.txt"
            filterAlignments(merged, filt, frozenset(simplename(f) for f in ingroup))
            out["filtered_canon"] = _maybe_hashed(canon_lines(filt), hash_big)
        if not run_main:
            # the reference's renderer dies with KeyError when a column holds a
            # lone IUPAC letter (Amplicon.py:65); only the stages are pinned
            return out
        # ---- main()
        csvp = os.path.join(td, "out.csv")
        alnp = os.path.join(td, "out.txt")
        argv = ["krisp_fasta"] + [paths[f] for f in ingroup]
        if outgroup:
            argv += ["--outgroup"] + [paths[f] for f in outgroup]
        if main_args is None:
            main_args = ["--conserved-left", str(L), "--conserved-right", str(R),
                         "--diagnostic", str(D)]
        argv += main_args
        if omit:
            argv += ["--omit-soft"]
        if dot:
            argv += ["--dot-alignment"]
        argv += ["--cores", "1", "--workdir", work, "--out_csv", csvp, "--out_align", alnp]
        out["main_args"] = main_args
        old = sys.argv
        ConservedEndAmplicons.ENABLE_DOT = False
        try:
            sys.argv = argv
            KF.main()
        finally:
            sys.argv = old
        out["csv"] = open(csvp).read()
        out["align"] = open(alnp).read() if os.path.exists(alnp) else ""
    return out


def mutate(rng, s, rate):
    o = []
    for c in s:
        if rng.random() < rate:
            c = rng.choice([b for b in "ACGT" if b != c])
        o.append(c)
    return "".join(o)


def fasta_text(records, width=60):
    o = []
    for i, s in enumerate(records):
        o.append(f">rec{i}")
        for j in range(0, len(s), width):
            o.append(s[j:j + width])
    return ("\n".join(o) + "\n").encode()


def fasta_cases():
    cases = []
    # ---- C1: the reference's own test data
    c1 = {}
    names = ["ingroup0", "ingroup1", "outgroup0", "outgroup1", "outgroup2"]
    os.makedirs(HERE / "c1", exist_ok=True)
    for n in names:
        fn = f"{n}.fasta.gz"
        src = f"{REF}/test_data/krisp_fasta/{fn}"
        shutil.copyfile(src, HERE / "c1" / fn)
        os.chmod(HERE / "c1" / fn, 0o644)
        c1[fn] = open(src, "rb").read()
    ing = [f"{n}.fasta.gz" for n in names[:2]]
    outg = [f"{n}.fasta.gz" for n in names[2:]]
    cases.append(run_fasta_case("c1_25_1_2", c1, ing, outg, 25, 1, 2, keep_sorted=True))
    cases.append(run_fasta_case("c1_25_1_2_dot", c1, ing, outg, 25, 1, 2, dot=True))
    cases.append(run_fasta_case("c1_28_1_2", c1, ing, outg, 28, 1, 2))
    cases.append(run_fasta_case("c1_30_40_30", c1, ing, outg, 30, 40, 30,
                                main_args=["--conserved", "30", "--amplicon", "100"]))
    cases.append(run_fasta_case("c1_30_40_30_dot", c1, ing, outg, 30, 40, 30, dot=True,
                                main_args=["--conserved", "30", "--amplicon", "100"]))
    cases.append(run_fasta_case("c1_30_0_30_all_ingroup", c1, ing + outg, [], 30, 0, 30,
                                main_args=["--conserved", "30", "--diagnostic", "0"]))
    cases.append(run_fasta_case("c1_32_60_32", c1, ing, outg, 32, 60, 32))
    cases.append(run_fasta_case("c1_10_2_4_amplicon_diag", c1, ing, outg, 7, 2, 7,
                                main_args=["--amplicon", "16", "--diagnostic", "2"]))
    # ---- four-genome label case
    Lq, Rq = "ACGTTGCA", "GGATC"
    lab = {
        "inA.fa": fasta_text([Lq + "T" + Rq, Lq + "T" + Rq, Lq + "G" + Rq]),
        "inB.fasta": fasta_text([Lq + "T" + Rq]),
        "outX.v1.fna": fasta_text([Lq + "C" + Rq]),
        "outY.fa": fasta_text([Lq + "A" + Rq + "NN" + Lq + "C" + Rq]),
    }
    cases.append(run_fasta_case("labels_8_1_5", lab, ["inA.fa", "inB.fasta"],
                                ["outX.v1.fna", "outY.fa"], 8, 1, 5))
    cases.append(run_fasta_case("labels_8_1_5_noout", lab,
                                ["inA.fa", "inB.fasta", "outX.v1.fna", "outY.fa"], [], 8, 1, 5))
    cases.append(run_fasta_case("labels_8_1_5_dot", lab, ["inA.fa", "inB.fasta"],
                                ["outX.v1.fna", "outY.fa"], 8, 1, 5, dot=True))
    cases.append(run_fasta_case("labels_swapped_order", lab, ["inB.fasta", "inA.fa"],
                                ["outY.fa", "outX.v1.fna"], 8, 1, 5))
    # ---- related random genomes (seeded) -- many groups, repeats, soft mask, N
    rng = random.Random(20241008)
    for ci, (n_in, n_out, glen, L, D, R, omit, rate, iupac) in enumerate([
            (2, 2, 600, 6, 1, 2, False, 0.02, False),
            (2, 3, 900, 5, 2, 4, False, 0.03, False),
            (3, 2, 700, 7, 1, 3, True, 0.02, False),
            (1, 1, 500, 4, 3, 4, False, 0.05, False),
            (2, 1, 800, 9, 0, 9, False, 0.01, False),
            (3, 0, 500, 5, 1, 5, False, 0.04, False),
            (2, 2, 1200, 12, 4, 12, False, 0.01, False),
            (2, 2, 1500, 16, 1, 15, False, 0.005, False),
            (2, 2, 600, 3, 1, 0, False, 0.02, False),      # R = 0 quirk
            (2, 2, 2000, 20, 10, 20, False, 0.004, False),  # k = 50 > 32
            (2, 2, 3000, 32, 6, 32, True, 0.003, False),   # k = 70 > 32, omit-soft
            (2, 2, 600, 5, 1, 3, False, 0.02, True),        # IUPAC letters kept
            (4, 5, 900, 8, 1, 4, False, 0.01, False),       # 9 genomes, odd tree
            (2, 2, 1500, 14, 2, 14, False, 0.004, False),   # k = 30
            (1, 2, 1200, 15, 2, 15, False, 0.004, False),   # k = 32
    ]):
        anc_recs = []
        for r in range(3):
            s = "".join(rng.choice("ACGT") for _ in range(glen // 3))
            # plant a tandem repeat and a palindrome so duplicates / (2) labels occur
            if r == 0:
                unit = "".join(rng.choice("ACGT") for _ in range(L + D + R + 3))
                s = s[:50] + unit * 3 + s[50:]
            anc_recs.append(s)
        files = {}
        ing, outg = [], []
        # planted ingroup-specific SNPs: (record, position, ingroup base, outgroup base)
        plants = []
        for r in range(3):
            for _ in range(3):
                pos = rng.randrange(L + D + R, len(anc_recs[r]) - (L + D + R))
                b1, b2 = rng.sample("ACGT", 2)
                plants.append((r, pos, b1, b2))
        for gi in range(n_in + n_out):
            recs = []
            for r, s in enumerate(anc_recs):
                m = mutate(rng, s, rate)
                m = list(m)
                for (pr, pos, b1, b2) in plants:
                    if pr == r:
                        m[pos] = b1 if gi < n_in else b2
                # soft-mask a stretch and drop in a few N / IUPAC letters
                a = rng.randrange(0, max(1, len(m) - 40))
                for j in range(a, min(len(m), a + rng.randint(0, 30))):
                    m[j] = m[j].lower()
                for _ in range(rng.randint(0, 2)):
                    m[rng.randrange(len(m))] = rng.choice("NnRYKM" if iupac else "Nn")
                recs.append("".join(m))
            fn = (f"in{gi}.fa" if gi < n_in else f"out{gi - n_in}.fasta")
            files[fn] = fasta_text(recs)
            (ing if gi < n_in else outg).append(fn)
        cases.append(run_fasta_case(f"rand{ci}_{L}_{D}_{R}", files, ing, outg, L, D, R, omit=omit,
                                    run_main=not iupac))
        cases[-1]["files"] = {fn: c.decode() for fn, c in files.items()}
    for c in cases:
        if c["name"].startswith("labels"):
            c["files"] = {fn: v.decode() for fn, v in lab.items()}
    return cases


def fasta_cases_r6():
    """round 6 (VERDICT r5 'lift the input limits'): runs that mix DNA and RNA genomes, flanks longer than 64 bases,
    amplicons longer than 256 -- what the earlier builds refused and the reference simply runs"""
    cases = []
    rng = random.Random(20261005)

    def family(n, glen, rate, L, D, R, nrec=3, plants_per_rec=3, t_frac=0.25):
        k = L + D + R
        w = [(1 - t_frac) / 3] * 3 + [t_frac]
        anc = ["".join(rng.choices("ACGT", weights=w, k=glen // nrec)) for _ in range(nrec)]
        plants = []
        for r in range(nrec):
            for _ in range(plants_per_rec):
                pos = rng.randrange(k, len(anc[r]) - k)
                b1, b2 = rng.sample("ACGT", 2)
                plants.append((r, pos, b1, b2))
        return anc, plants

    def genome(anc, plants, rate, ingroup, rna, extra=None):
        recs = []
        for r, s in enumerate(anc):
            m = list(mutate(rng, s, rate))
            for (pr, pos, b1, b2) in plants + (extra or []):
                if pr == r:
                    m[pos] = b1 if ingroup else b2
            a = rng.randrange(0, max(1, len(m) - 40))
            for j in range(a, min(len(m), a + rng.randint(0, 20))):
                m[j] = m[j].lower()
            if rng.random() < 0.5:
                m[rng.randrange(len(m))] = "N"
            recs.append("".join(m))
        text = fasta_text(recs)
        if rna:
            text = text.replace(b"T", b"U").replace(b"t", b"u")
        return text

    # ---- DNA + RNA genomes in one run
    for name, kinds_in, kinds_out, (L, D, R), glen, rate, tf in [
            ("mixed_in_dna_out_rna_6_1_3", [False, False], [True, True], (6, 1, 3), 900, 0.01, 0.25),
            ("mixed_both_sides_8_2_4", [False, True], [False, True], (8, 2, 4), 1200, 0.01, 0.15),
            ("mixed_in_rna_out_dna_5_1_5", [True, True], [False], (5, 1, 5), 800, 0.02, 0.25),
            ("mixed_no_outgroup_7_1_3", [False, True, False], [], (7, 1, 3), 700, 0.01, 0.2),
            ("mixed_wide_20_10_20", [False, True], [True], (20, 10, 20), 1800, 0.003, 0.02),
            ("mixed_wide_in_dna_out_rna_18_6_18", [False, False], [True, True], (18, 6, 18), 1800, 0.003, 0.03),
            ("all_rna_6_1_3", [True, True], [True], (6, 1, 3), 600, 0.01, 0.25),
    ]:
        anc, plants = family(len(kinds_in) + len(kinds_out), glen, rate, L, D, R, t_frac=tf)
        # (a column that is T in every ingroup genome and T / U in every outgroup genome: diagnostic to the reference only
        # when the sides' alphabets differ -- it compares letters)
        extra = []
        for r in range(len(anc)):
            pos = rng.randrange(L + D + R, len(anc[r]) - (L + D + R))
            extra.append((r, pos, "T", "T"))
        files, ing, outg = {}, [], []
        for i, rna in enumerate(kinds_in):
            fn = f"in{i}.fa"
            files[fn] = genome(anc, plants, rate, True, rna, extra)
            ing.append(fn)
        for i, rna in enumerate(kinds_out):
            fn = f"out{i}.fasta"
            files[fn] = genome(anc, plants, rate, False, rna, extra)
            outg.append(fn)
        c = run_fasta_case(name, files, ing, outg, L, D, R)
        c["files"] = {fn: v.decode() for fn, v in files.items()}
        cases.append(c)
    # ---- flanks longer than 64 bases, amplicons longer than 256
    for name, n_in, n_out, (L, D, R), glen, rate, omit in [
            ("long_70_10_70", 2, 2, (70, 10, 70), 2400, 0.0015, False),
            ("long_100_5_90", 2, 1, (100, 5, 90), 2400, 0.001, False),
            ("long_40_220_40", 2, 2, (40, 220, 40), 2700, 0.001, False),
            ("long_65_1_2", 1, 2, (65, 1, 2), 1800, 0.002, True),
            ("long_130_60_129", 2, 2, (130, 60, 129), 3000, 0.0007, False),
    ]:
        anc, plants = family(n_in + n_out, glen, rate, L, D, R, plants_per_rec=4)
        files, ing, outg = {}, [], []
        for i in range(n_in):
            fn = f"in{i}.fa"
            files[fn] = genome(anc, plants, rate, True, False)
            ing.append(fn)
        for i in range(n_out):
            fn = f"out{i}.fasta"
            files[fn] = genome(anc, plants, rate, False, False)
            outg.append(fn)
        c = run_fasta_case(name, files, ing, outg, L, D, R, omit=omit, hash_big=True)
        c["files"] = {fn: v.decode() for fn, v in files.items()}
        cases.append(c)
    # ---- amplicons longer than one key whose k-mer files hold IUPAC ambiguity letters (kept by the reference, kstream.py:11-18):
    # the stage functions on such files (VERDICT r5 missing #6).  The renderer dies on a lone ambiguity letter: stages only.
    for name, n_in, n_out, (L, D, R), glen, rate in [
            ("long_iupac_20_10_20", 2, 2, (20, 10, 20), 900, 0.004),
            ("long_iupac_40_4_33", 2, 1, (40, 4, 33), 1200, 0.002),
    ]:
        anc, plants = family(n_in + n_out, glen, rate, L, D, R)
        files, ing, outg = {}, [], []
        for i in range(n_in + n_out):
            text = genome(anc, plants, rate, i < n_in, False).decode()
            m = list(text)
            body = [j for j, ch in enumerate(m) if ch in "ACGT"]
            for j in rng.sample(body, 4):
                m[j] = rng.choice("RYKMSW")
            fn = f"in{i}.fa" if i < n_in else f"out{i - n_in}.fasta"
            files[fn] = "".join(m).encode()
            (ing if i < n_in else outg).append(fn)
        c = run_fasta_case(name, files, ing, outg, L, D, R, hash_big=True, run_main=False)
        c["files"] = {fn: v.decode() for fn, v in files.items()}
        cases.append(c)
    # ---- DNA + RNA genomes AND IUPAC ambiguity letters in one run (stages only: the renderer dies on U / lone letters)
    for name, kinds_in, kinds_out, (L, D, R), glen, rate, tf in [
            ("mixed_iupac_6_1_3", [False, True], [True, False], (6, 1, 3), 900, 0.01, 0.2),
            ("mixed_iupac_in_dna_out_rna_5_2_4", [False, False], [True], (5, 2, 4), 800, 0.01, 0.25),
            ("mixed_iupac_wide_18_6_18", [False, True], [True], (18, 6, 18), 1500, 0.003, 0.03),
    ]:
        anc, plants = family(len(kinds_in) + len(kinds_out), glen, rate, L, D, R, t_frac=tf)
        files, ing, outg = {}, [], []
        for i, rna in enumerate(kinds_in + kinds_out):
            is_in = i < len(kinds_in)
            text = genome(anc, plants, rate, is_in, False).decode()
            m = list(text)
            body = [j for j, ch in enumerate(m) if ch in "ACGT"]
            for j in rng.sample(body, 5):
                m[j] = rng.choice("RYKMSW")
            text = "".join(m)
            if rna:
                text = text.replace("T", "U").replace("t", "u")
            fn = f"in{i}.fa" if is_in else f"out{i - len(kinds_in)}.fasta"
            files[fn] = text.encode()
            (ing if is_in else outg).append(fn)
        c = run_fasta_case(name, files, ing, outg, L, D, R, hash_big=True, run_main=False)
        c["files"] = {fn: v.decode() for fn, v in files.items()}
        cases.append(c)
    return cases


# --------------------------------------------------------------------------
# 3. the reader alone: file / list -> records, FASTA and RNA verdicts
# --------------------------------------------------------------------------
# the 29 code points str.strip() removes (str.isspace())
WHITE = [chr(c) for c in range(0x110000) if chr(c).isspace()]


def run_reader(text, source):
    """the reference's reader chain as kstream.__call__ runs it (kstream.py:444-456) and the RNA detection
    (kstream.py:481-508) over its records.  source: 'in.fa' (text mode, universal newlines), 'in.fa.gz' (a gzip file --
    see reader_cases for the texts it leaves out) or 'list' (the text's lines, '\\n'-split, as an in-memory list of str)"""
    ks = kstream()
    with tempfile.TemporaryDirectory() as td:
        if source == "list":
            sequences = text.split("\n")
        else:
            path = os.path.join(td, source)
            with (gzip.GzipFile(path, "wb", mtime=0) if source.endswith(".gz") else open(path, "wb")) as f:
                f.write(text.encode())
            sequences = ks._read_file(path)
        is_fasta, _ = ks._detect_FASTA(sequences)
        recs = list(ks._parse_FASTA(sequences) if is_fasta else ks._parse_seqs(sequences))
    rna, _ = ks._detect_RNA(iter(recs))
    return {"records": recs, "fasta": is_fasta, "rna": rna}


def reader_cases():
    """white space as str.strip() sees it, around and inside sequence lines, header lines and otherwise empty lines,
    FASTA and not, from a plain file, a gzip file and a list; written to reader_cases.json"""
    texts = []
    for i, w in enumerate(WHITE):
        v = WHITE[(i * 7 + 3) % len(WHITE)]
        texts.append((f"fasta_{ord(w):04x}",
                      f">h{w}\n{w}ACGT{w}\n{w} AC{w}GT\t{v}\n{w}\n{v}{w} {w}\n{w}>x{w}\n{w}TTU{w}{v}\n{w}{w}\n"
                      f">y\nGG{w}\n>z\n{w}\n>u\n{v}UUCA\n"))
        texts.append((f"plain_{ord(w):04x}", f"{w}first{w}\n{w}ACGT{w}\nAC{w}GT\n{w}\n\t{w}{v}UU{w}\n{w}TT"))
        texts.append((f"rna_{ord(w):04x}", f">a{w}\n{w}\n{w}UUAC{w}\n>b\n{w}GGT{w}\n"))
    # next to real line breaks (text mode splits on \n, \r and \r\n only; the binary lines on \n)
    for w in ("\x85", "\u2028", "\u2029", "\x1c", "\x1d", "\x1e", "\x0b", "\x0c"):
        texts.append((f"breaks_{ord(w):04x}", f">h\nAC{w}\nGT{w}\r\n{w}\rAA{w}\r{w}CC\n{w}\n\r\nGG{w}\n>x{w}\r\n{w}TT\r"))
        texts.append((f"breaks_plain_{ord(w):04x}", f"x{w}\r\n{w}AC{w}\rGT\n{w}{w}\r\nTT{w}"))
    # the issue's text: a record of white space only, a no-break space after the sequence
    texts.append(("issue_example", ">h\n\x1cACGT\x1f\nAC\xa0\n\x0bGG\n>x\n\x1d\n>y\nTT\n"))
    rng = random.Random(20261015)
    ascii_ws = [w for w in WHITE if ord(w) < 128]
    for i in range(160):
        lines = []
        for _ in range(rng.randint(0, 14)):
            pre = "".join(rng.choice(WHITE) for _ in range(rng.choice([0, 0, 1, 2, 3])))
            post = "".join(rng.choice(WHITE) for _ in range(rng.choice([0, 0, 1, 2, 3])))
            kind = rng.random()
            if kind < 0.25:
                body = ">" + "".join(rng.choice(["a", "b", " ", ">"] + WHITE) for _ in range(rng.randint(0, 5)))
            elif kind < 0.4:
                body = ""
            else:
                body = "".join(rng.choice(["A", "C", "G", "T", "U", "a", "u", "N", ">"] + WHITE[:3] + WHITE[-3:])
                               for _ in range(rng.randint(0, 20)))
            lines.append(pre + body + post)
        nl = rng.choice(["\n", "\r\n", "\r", "\n"])
        text = nl.join(lines) + rng.choice(["", nl, nl + rng.choice(ascii_ws)])
        texts.append((f"random{i}", text))
    cases = []
    for name, text in texts:
        for source in ("in.fa", "in.fa.gz", "list"):
            # (a '\r' that is not part of a '\r\n': a line break in a .gz file where fileinput wraps the stream in text
            # mode -- Python >= 3.10 --, inside the line where it hands over binary lines; the readers here take the
            # binary lines.  Such texts are pinned for plain files and lists only.)
            if source.endswith(".gz") and "\r" in text.replace("\r\n", ""):
                continue
            cases.append({"name": f"{name}_{source.replace('.', '_')}", "text": text, "source": source,
                          **run_reader(text, source)})
    return cases


def white_fasta_text(rng, records, width=60):
    """fasta_text with white space of every kind (str.strip()'s) at the ends of the lines, and lines of white space only"""
    def pad():
        return "".join(rng.choice(WHITE) for _ in range(rng.choice([0, 1, 1, 2, 3])))
    o = []
    for i, s in enumerate(records):
        o.append(f"{pad()}>rec{i}{pad()}")
        for j in range(0, len(s), width):
            o.append(pad() + s[j:j + width] + pad())
            if rng.random() < 0.1:
                o.append(pad())
    return ("\n".join(o) + "\n").encode()


def white_fasta_case():
    """krisp_fasta over genomes whose lines carry white space of every kind: two in-group and one out-group genome"""
    rng = random.Random(20261016)
    L, D, R = 8, 1, 6
    anc = ["".join(rng.choice("ACGT") for _ in range(400)) for _ in range(2)]
    plants = [(r, rng.randrange(20, 380)) for r in range(2) for _ in range(3)]
    files = {}
    for gi, fn in enumerate(["inW0.fa", "inW1.fasta", "outW.fa"]):
        recs = []
        for r, s in enumerate(anc):
            m = list(mutate(rng, s, 0.01))
            for pr, pos in plants:
                if pr == r:
                    m[pos] = "G" if gi < 2 else "T"
            recs.append("".join(m))
        files[fn] = white_fasta_text(rng, recs)
    c = run_fasta_case("white_space_8_1_6", files, ["inW0.fa", "inW1.fasta"], ["outW.fa"], L, D, R)
    c["files"] = {fn: v.decode() for fn, v in files.items()}
    return c


def main():
    if "--reader-only" in sys.argv:
        rc = reader_cases()
        with open(HERE / "reader_cases.json", "w") as f:
            json.dump(rc, f, indent=1)
        print(f"reader cases: {len(rc)}")
        return
    if "--ks6-only" in sys.argv:
        k6 = kstream_cases_r6()
        with open(HERE / "kstream_cases_r6.json", "w") as f:
            json.dump(k6, f, indent=1)
        print(f"kstream cases (round 6): {len(k6)}; raised: {sorted(c['name'] for c in k6 if 'raises' in c)}")
        return
    if "--r6-only" in sys.argv:
        fc = fasta_cases_r6()
        with open(HERE / "fasta_cases_r6.json", "w") as f:
            json.dump(fc, f, indent=1)
        for c in fc:
            print(c["name"], "merged", len(c["merged_canon"]), "filtered",
                  len(c.get("filtered_canon", [])), "csv bytes", len(c.get("csv", "")))
        return
    k6 = kstream_cases_r6()
    with open(HERE / "kstream_cases_r6.json", "w") as f:
        json.dump(k6, f, indent=1)
    kr = kstream_cases_routes()
    with open(HERE / "kstream_cases_routes.json", "w") as f:
        json.dump(kr, f, indent=1)
    print(f"kstream cases (routes): {len(kr)}; raised: {sorted(c['name'] for c in kr if 'raises' in c)}")
    if "--routes-only" in sys.argv:
        return
    km = kstream_cases_more()
    with open(HERE / "kstream_cases_more.json", "w") as f:
        json.dump(km, f, indent=1)
    print(f"kstream cases (more): {len(km)}")
    if "--more-only" in sys.argv:
        return
    ks = kstream_cases()
    with open(HERE / "kstream_cases.json", "w") as f:
        json.dump(ks, f, indent=1)
    print(f"kstream cases: {len(ks)}")
    rc = reader_cases()
    with open(HERE / "reader_cases.json", "w") as f:
        json.dump(rc, f, indent=1)
    print(f"reader cases: {len(rc)}")
    fc = fasta_cases() + [white_fasta_case()]
    with open(HERE / "fasta_cases.json", "w") as f:
        json.dump(fc, f, indent=1)
    print(f"krisp_fasta cases: {len(fc)}")
    fc6 = fasta_cases_r6()
    with open(HERE / "fasta_cases_r6.json", "w") as f:
        json.dump(fc6, f, indent=1)
    fc = fc + fc6
    for c in fc:
        print(c["name"], "merged", len(c["merged_canon"]), "filtered",
              len(c.get("filtered_canon", [])), "csv bytes", len(c.get("csv", "")))


if __name__ == "__main__":
    main()

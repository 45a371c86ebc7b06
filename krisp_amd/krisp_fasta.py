"""`krisp_fasta` -- same command line and stage functions as the reference
(krisp_fasta/krisp_fasta.py), with the k-mer generation / sort / multi-genome
intersection / diagnostic filter running on the MI355X through libkrisp_hip.so.

Seams kept:
  extractSortedKmers(fasta, primer_left, primer_right, ampl_len, output, sortmem,
                     parallel=1, verbose=True, omit=True)      krisp_fasta.py:16-66
  mergeFiles(files, output, parallel=1, workdir=None, verbose=True)
                                                               intersectAmplicons.py:232-310
  filterAlignments(kmerfile, output, ingroup)                  filterAlignments.py:31-40
  main()                                                       krisp_fasta.py:126-298
main() does not round-trip through text files: genomes are sorted once on the
device and intersected there (find_regions); the stage functions exist for
interoperability with the reference's intermediate files and for stage-level
parity tests.  There is no CPU implementation of the hot path behind any of them.
"""
import argparse
import json
import math
import os
import sys
import time
from collections import namedtuple
from typing import NamedTuple

import numpy as np

from . import _native, amplicon, codec, distributed, fasta
from .codec import _is_wide
from .fasta import _FASTA_EXT, basename, simplename                          # noqa: F401
from .kstream import kstream
# the report passes (reports.py): every name resolves here as before; main() calls the passes through these globals
from .reports import (                                                        # noqa: F401
    ASSAY_HIT, ASSAY_HIT_HEADER, GUIDE_BULGE_HIT, GUIDE_BULGE_HIT_HEADER, GUIDE_BULGE_MAX_MISMATCHES, GUIDE_BULGE_MIN_SIZE,
    GUIDE_HEADER, GUIDE_HIT, GUIDE_HIT_HEADER, GUIDE_HIT_MAX_BULGES, GUIDE_HIT_MAX_MISMATCHES, GUIDE_MAX_MOTIF, GUIDE_MAX_SIZE,
    GUIDE_MIN_SIZE, IUPAC_MASK, LOCATE_MAX_BASES, LOCATION, LOCATION_HEADER, NEAR, NEAR_HEADER, NEAR_MAX_MISMATCHES, PRODUCT,
    PRODUCT_END, PRODUCT_HEADER, PRODUCT_MAX_MISMATCHES, PRODUCT_MIN_PRIMER, _GUIDE_COMPLEMENT, _check_max_product, _engine,
    _fan_out, _fill_guide_hit, _fill_product, _fill_shared, _group_flanks, _guide_rc, _mask_columns, _record_coords, _rows_text,
    _scan_genomes, _sorted_parts, _text_matrix, _write_tsv, assay_hits, assay_hits_refusal, assay_links, assay_orientation,
    design_guide_shortlist, design_guides, design_primers, design_templates, guide_bulge_hits, guide_candidates_refusal, guide_hits,
    guide_hits_refusal, guide_rows, guide_tallies, guide_texts, guides_refusal, locate_regions, motif_masks, near_matches,
    near_refusal, near_targets, pick_guides, predict_products, primer_pairs, primer_products, primer_products_refusal,
    products_refusal, shortlist_texts, write_assay_hits, write_guide_bulge_hits, write_guide_candidates, write_guide_hits,
    write_guides, write_locations, write_near, write_products,
    PRIMER_CANDIDATE_HEADER, PRIMER_MAX_CANDIDATES, design_primer_shortlist, pick_pairs, primer_candidates_refusal,
    primer_tallies, shortlist_pairs, write_primer_candidates,
    PANEL_HEADER, PANEL_MAX_SIZE, panel_candidates, panel_refusal, select_panel, write_panel,
    panel_candidate_texts, panel_clean_refusal, select_panel_clean,
    PANEL_PRODUCT, PANEL_PRODUCT_HEADER, PANEL_SUMMARY, PANEL_SUMMARY_HEADER, panel_kind, panel_oligos, panel_products,
    panel_products_refusal, panel_texts, write_panel_products, write_panel_summary)

def prettyTime(t):
    """shared.py:8-31."""
    if t < 60:
        return f"{t:.2f} seconds"
    minutes = int(t / 60)
    seconds = math.ceil(t - 60 * minutes)
    return (f"{minutes} minute{'s' if minutes > 1 else ''} and "
            f"{seconds} second{'s' if seconds > 1 else ''}")


class UnsupportedGeometry(NotImplementedError):
    pass


class MixedAlphabet(NotImplementedError):
    """DNA and RNA genomes in one run: the reference compares their k-mers as text ('T' never
    equals 'U', kstream.py:481-508, 599), which the 2-bit device alphabet cannot express."""


def _to_rna(groups):
    """kstream writes an RNA genome's k-mers back with U (kstream.py:297, 599)"""
    for g in groups:
        for a in g:
            a.left, a.diag, a.right = (x.replace("T", "U") for x in (a.left, a.diag, a.right))
    return groups


def _mixed_prefix_filter(eng, L, R):
    """DNA and RNA genomes in one run: the reference compares text, and 'T' never equals 'U' (kstream.py:481-508, 599 writes
    an RNA genome's k-mers with U; shared.py:321-347 merges on the (left,right) strings) -- a (left,right) pair that holds
    code 3 is in no DNA genome AND RNA genome alike.  The device matched them (one code for both letters): those candidates
    go.  Returns the number left (the list is replaced on the device when any went)."""
    cands = eng.cands()
    if not len(cands):
        return 0
    p = cands["prefix"]
    threes = (p >> np.uint64(1)) & p & np.uint64(0x5555555555555555) & codec.prefix_mask(L, R)
    keep = threes == 0
    if not keep.all():
        cands = cands[keep]
        eng.load_cands(cands)
    return len(cands)


def _mixed_finish(records, labels, geo, rna, ingroup_labels, do_filter):
    """... and the exact filter on the survivors of the device's mode-2 filter (k_intersect.inc: passes_filter -- a column
    whose ingroup and outgroup sets share nothing but code 3 passed there): here each genome's alphabet is known, the
    groups are text, and the reference's own predicate decides (Amplicon.py:495-521 via filterAlignments.py:4-40)"""
    Le, De, Re = geo
    groups = amplicon.groups_from_records_mixed(records, labels, Le, De, Re, rna)
    if do_filter and len(ingroup_labels):
        ing = frozenset(ingroup_labels)
        groups = [g for g in groups if amplicon.ingroup_unique_columns(g, ing)]
    return groups


def _check_geometry(L, D, R):
    """geometries of the packed path: the whole amplicon in one 64-bit key"""
    k = L + D + R
    if k > 32:
        raise UnsupportedGeometry(
            f"amplicon length {k} > 32: only the fused flow (find_regions / the command line) "
            "carries amplicons longer than one 64-bit key")
    if D > 16:
        raise UnsupportedGeometry(f"diagnostic length {D} > 16 exceeds the device mask format")


def _check_wide(L, D, R):
    """geometries of the wide path (kr_wide_run): flanks of up to WIDE_MAX_FLANK bases (one key each, or -- longer than 32
    bases -- ranked piece by piece through up to eight keys), amplicons of up to WIDE_MAX_K"""
    if not (1 <= L <= _native.WIDE_MAX_FLANK and 1 <= R <= _native.WIDE_MAX_FLANK and L + D + R <= _native.WIDE_MAX_K):
        raise UnsupportedGeometry(
            f"{L}/{D}/{R}: amplicons longer than 32 bases need 1 <= conserved-left, conserved-right "
            f"<= {_native.WIDE_MAX_FLANK} and a length <= {_native.WIDE_MAX_K}")


_COMP_U8 = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP_U8[_a] = _b


def _hit_windows(sel, text, k):
    """member windows of kr_wide_run hits of ONE genome as an (n, k) byte matrix: cut from the text
    the host holds, soft-mask mapped, reverse complemented for strand 1"""
    t = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    W = t[sel["pos"].astype(np.int64)[:, None] + np.arange(k, dtype=np.int64)] & np.uint8(0xDF)
    rc = sel["strand"] == 1
    W[rc] = _COMP_U8[W[rc][:, ::-1]]
    return W


def _groups_from_hits(hits, texts, labels, L, D, R, rna_genomes=None):
    """kr_wide_run hits (group, genome, position, strand) -> groups of amplicon.Amplicon in the reference's order: groups
    by (left,right), sequences by diag; the window text is cut from the genome the host already holds (_hit_windows:
    soft-mask mapped, kstream.py:622-642; reverse complemented for strand 1, kstream.py:644-659)."""
    if len(hits) == 0:
        return []
    windows, genomes = [], []
    for gi, text in enumerate(texts):
        sel = hits[hits["genome"] == gi]
        if len(sel) == 0:
            continue
        W = _hit_windows(sel, text, L + D + R)
        if rna_genomes is not None and rna_genomes[gi]:
            W[W == ord("T")] = ord("U")                 # (an RNA genome's k-mers are written with U: kstream.py:599)
        windows.append(W)
        genomes.append(np.full(len(sel), gi, dtype=np.uint32))
    # (ordered as the reference's merged file is, not by the device's group numbers, which need not ascend with
    # (left, right): KR_OPT_WIDE_ORDERED)
    return amplicon.groups_from_windows(np.concatenate(windows), np.concatenate(genomes), labels, L, D, R)


# ----------------------------------------------------------------------------
# groups touched by k-mers that hold IUPAC ambiguity letters
# ----------------------------------------------------------------------------
_ACGT = frozenset("ACGT")


def _pure(s):
    return _ACGT.issuperset(s)


def _prefix_key(left, right):
    key = 0
    for i, ch in enumerate(left + right):
        key |= "ACGT".index(ch) << (62 - 2 * i)
    return key


def _touched_prefix_cands(specials):
    """the (left,right) pairs IUPAC windows touch, and those of them with plain flanks as a candidate list (their
    _prefix_key once each, ascending; empty when no pair is plain): the device looks their ACGT members up from it"""
    touched = {(l, r) for sp in specials for (l, d, r) in sp}
    pure = sorted({_prefix_key(l, r) for (l, r) in touched if _pure(l) and _pure(r)})
    cands = np.zeros(len(pure), dtype=_native.CAND)
    cands["prefix"] = np.array(pure, dtype=np.uint64)
    return touched, cands


def _special_groups(eng, ids, labels, specials, geo, ingroup, do_filter, rna_genomes=None):
    """The reference keeps k-mers with IUPAC letters (kstream.py:11-18); the device cannot pack them, so they arrive here
    as strings: specials[g] = [(left, diag, right), ...] of genome g.  Every (left,right) group they touch is rebuilt
    exactly: its ACGT members are looked up on the device (kr_cands_load + kr_collect), the IUPAC members added, then the
    reference's rules applied (_touched_groups).  Rare by nature; everything else stays on the device.
    Returns (set of touched (left,right), list of surviving groups)."""
    touched, cands = _touched_prefix_cands(specials)
    if not touched:
        return touched, []
    recs = None
    if len(cands):
        eng.load_cands(cands)
        recs = eng.collect(ids)
    return touched, _special_groups_from(recs, ids, labels, specials, geo, ingroup, do_filter, rna_genomes)


def _special_groups_from(recs, ids, labels, specials, geo, ingroup, do_filter, rna_genomes=None):
    """the groups IUPAC windows touch, from the device records of their ACGT members (`recs`: of one context, or
    gathered from every rank of a multi-GPU run) and the IUPAC members themselves (specials[g] of genome ids[g]).
    rna_genomes (a run that mixes DNA and RNA genomes): the text of an RNA genome's members carries U -- the reference
    compares text, so a group is a (left,right) pair every genome holds letter for letter"""
    members = {}            # (left,right) -> {(left,diag,right) -> {genome index -> count}}
    for rec in (recs if recs is not None else ()):
        l, d, r = codec.key_columns(rec["key"], *geo)
        m = members.setdefault((l, r), {}).setdefault((l, d, r), {})
        gi = ids.index(int(rec["genome"]))
        m[gi] = m.get(gi, 0) + int(rec["count"])
    touched = {(l, r) for sp in specials for (l, d, r) in sp}
    return _touched_groups(members, len(ids), labels, specials, touched, ingroup, do_filter, rna_genomes)


def _wide_probe_members(eng, texts, gis, probes, probe_text, geo, pid):
    """the ACGT members of the touched (left,right) pairs with plain flanks in the genomes gis (texts[i] = genome gis[i]):
    one kr_wide_run per genome against a probe genome made of the pairs (left + A..A + right) returns every window of
    that genome whose flanks are one of them.  -> {(left,right): {(left,diag,right): {genome: count}}}"""
    L, D, R = geo
    members = {}
    if not probes:
        return members
    wanted = set(probes)
    eng.upload(pid, probe_text)
    for gi, text in zip(gis, texts):
        nh = eng.wide_run([pid, gi], [True, True], apply_filter=False)
        if not nh:
            continue
        hits = eng.wide_fetch(_native.WIDE_HITS)
        hits = hits[hits["genome"] == 1].copy()
        hits["genome"] = 0
        for g in _groups_from_hits(hits, [text], ["x"], L, D, R):
            for a in g:
                if (a.left, a.right) in wanted:
                    m = members.setdefault((a.left, a.right), {}).setdefault((a.left, a.diag, a.right), {})
                    m[gi] = m.get(gi, 0) + len(a.labels)
    return members


def _touched_groups(members, n, labels, specials, touched, ingroup, do_filter, rna_genomes=None):
    """the groups IUPAC windows touch, from the ACGT members the device found (_special_groups_from's records or
    _wide_probe_members, of one context or merged over the ranks) and the IUPAC members themselves (specials[g] of genome
    g), under the reference's rules: present in every one of the n genomes (intersectAmplicons.py:232-310), an
    ingroup-unique column (Amplicon.py:495-521)"""
    for gi, sp in enumerate(specials):
        for (l, d, r) in sp:
            m = members.setdefault((l, r), {}).setdefault((l, d, r), {})
            m[gi] = m.get(gi, 0) + 1
    if rna_genomes is not None:
        # (a run that mixes DNA and RNA genomes: every member as the text its genome's file holds -- U for an RNA genome --,
        # grouped again on that text; pairs that hold T / U then lack the genomes of the other alphabet)
        conv = {}
        for P, seqs in members.items():
            if P not in touched:
                continue
            for seq, m in seqs.items():
                for gi, cnt in m.items():
                    l, d, r = ((x.replace("T", "U") for x in seq) if rna_genomes[gi] else seq)
                    mm = conv.setdefault((l, r), {}).setdefault((l, d, r), {})
                    mm[gi] = mm.get(gi, 0) + cnt
        members = conv
        touched = set(conv)
    groups = []
    for P in sorted(touched.intersection(members)):
        seqs = members[P]
        if len(set().union(*seqs.values())) != n:
            continue
        group = [amplicon.Amplicon(*seq, [labels[gi] for gi, cnt in seqs[seq].items() for _ in range(cnt)])
                 for seq in sorted(seqs, key=lambda t: t[1])]
        if not do_filter or amplicon.ingroup_unique_columns(group, ingroup):
            groups.append(group)
    return groups


def _special_groups_wide(eng, texts, labels, specials, touched, probes, probe_text, geo, ingroup, do_filter, rna_genomes=None):
    """Wide-path twin of _special_groups.  A touched (left,right) pair with an IUPAC letter in a flank can only hold IUPAC
    k-mers (the host has them all); a pair with plain flanks also holds ACGT windows, which the device locates."""
    n = len(texts)
    members = _wide_probe_members(eng, texts, list(range(n)), probes, probe_text, geo, pid=n)
    return _touched_groups(members, n, labels, specials, touched, ingroup, do_filter, rna_genomes)


def _merge_groups(device_groups, touched, special_groups):
    """device groups minus the ones re-evaluated on the host, plus those; (left,right) byte order"""
    out = [g for g in device_groups if (g[0].left, g[0].right) not in touched] + special_groups
    out.sort(key=lambda g: (g[0].left, g[0].right))
    return out


RESERVE_MIN = 128 << 20      # bytes of file text from which the context's memory is made ahead of the uploads (kr_reserve)
STREAM_MIN = 1 << 30         # ... and from which the files are read one after the other, each on all host threads


class _Run(NamedTuple):
    """one find_regions run (or one rank's share of a distributed run) as its flows see it"""
    geo: tuple                  # (L, D, R) after codec.effective_geometry
    k: int
    do_filter: bool
    quirk_all_fail: bool
    wide: bool                  # amplicons longer than one key: kr_wide_run
    labels: list                # one per genome, in the flow's file order
    ingroup_labels: frozenset
    flags: list                 # ingroup or not, per genome
    omit_soft: bool
    device: int
    verbose: bool
    workers: int                # host threads that read the files
    t0: float


def _describe_run(labels, ingroup_files, L, R, k, omit_soft, device, verbose, wide=None):
    """the run's description; a geometry no flow carries raises UnsupportedGeometry here, before a file is read"""
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    # the reference filters whenever k > L + R (krisp_fasta.py:265); with R == 0 the
    # diagnostic column is empty (kstream.py:824-830) and every group fails the filter
    do_filter = k > L + R
    quirk_all_fail = do_filter and De == 0
    if wide is None:                 # (tests force the wide path on packable geometries)
        wide = _is_wide(Le, De, Re)
    if wide and not quirk_all_fail:
        _check_wide(Le, De, Re)
    elif not wide:
        _check_geometry(Le, De, Re)
    # ingroup / outgroup by LABEL, as the reference classifies (Amplicon.py:495-521): an outgroup file whose label
    # equals an ingroup label counts as ingroup
    ingroup_labels = frozenset(simplename(f) for f in ingroup_files)
    return _Run((Le, De, Re), k, do_filter, quirk_all_fail, wide, labels, ingroup_labels,
                [lab in ingroup_labels for lab in labels], omit_soft, device, verbose,
                max(1, min(len(labels), os.cpu_count() or 1, 16)), time.time())


def _ingest_genome(eng, g, text, universal, run):
    """the text of one file -> genome g of `eng`, parsed on the device (fasta.ingest_on_device).  A packed run sorts it
    at once, while the files behind it still inflate (kr_wide_run sorts inside).
    -> (bases on the device, is RNA, its IUPAC windows as (left, diag, right))"""
    n, rna, sp = fasta.ingest_on_device(eng, g, text, universal, run.k, run.omit_soft)
    specials = [codec.split_window(w, *run.geo) for w in sp]
    if not run.wide:
        eng.sort(g)
    return n, rna, specials


def _packed_result(records, run, rna, touched, sgroups, stats):
    """a packed run's records (collected in label order) and the groups IUPAC windows touch (rebuilt on the host:
    sgroups) -> (groups, stats).  rna: the reader's verdict per genome (the streaming flow's fasta.sniff_rna gives the
    same: tests/test_host_glue.py)"""
    if run.quirk_all_fail:
        return [], stats
    if not touched and not any(rna):
        # (plain records: the renderer works from them directly, the list of groups is built only if someone walks it)
        return amplicon.RecordGroups(records, run.labels, *run.geo), stats
    if _mixed(rna):
        groups = _mixed_finish(records, run.labels, run.geo, rna, run.ingroup_labels, run.do_filter)
    else:
        groups = amplicon.groups_from_records(records, run.labels, *run.geo)
    if touched:
        groups = _merge_groups(groups, touched, sgroups)
    if _mixed(rna):
        stats["candidates"] = len(groups)
    return (_to_rna(groups) if all(rna) else groups), stats


def _touched_pairs(specials, D):
    """the (left,right) pairs IUPAC windows touch, those of them with plain flanks, and the probe genome made of these
    (left + A..A + right, a record each: _wide_probe_members)"""
    touched = {(l, r) for sp in specials for (l, d, r) in sp}
    probes = sorted(p for p in touched if _pure(p[0]) and _pure(p[1]))
    return touched, probes, np.frombuffer("\n".join(l + "A" * D + r for l, r in probes).encode(), dtype=np.uint8)


def _mixed_wide_groups(groups, run):
    """wide groups of a run that mixes DNA and RNA genomes: text decides -- flank pairs that hold T / U are in no DNA
    genome and RNA genome alike, and the filter's columns are compared letter by letter (_mixed_finish's rule on member
    windows)"""
    groups = [g for g in groups if not (set(g[0].left + g[0].right) & set("TU"))]
    if run.do_filter and run.ingroup_labels:
        groups = [g for g in groups if amplicon.ingroup_unique_columns(g, run.ingroup_labels)]
    return groups


def _mixed(flags):
    """some of them and not all: DNA and RNA genomes in one run, ingroup and outgroup genomes in one batch"""
    return any(flags) and not all(flags)


def _say_counts(files, counts, run):
    if run.verbose:
        for f, cnt in zip(files, counts):
            print(f"=> Extracted and sorted {cnt:,} {run.k}-kmers from {f}", file=sys.stderr)


def _free_quietly(eng, ids):
    for g in ids:
        try:
            eng.free(g)
        except _native.KrispHipError:
            pass


def _forced_batch():
    """KRISP_STREAM_BATCH=n: batches of n genomes whatever the device holds (tests); None when not set"""
    forced = os.environ.get("KRISP_STREAM_BATCH")
    return int(forced) if forced else None


class _Stages:
    """a flow's stage_s: stamp(name) books the time since the stamp before it (since `start`, for the first) under name"""

    def __init__(self):
        self.start = self.last = time.time()
        self.s = {}

    def stamp(self, name):
        now = time.time()
        self.s[name], self.last = now - self.last, now


def _find_regions_device_ingest(files, run):
    """find_regions' packed path; a genome set the plan thought would fit and the device then could not hold (the plan
    is an estimate: candidate lists, slices of a skewed genome, another process on the device) is run again in batches"""
    try:
        return _device_ingest_flow(files, run, None)
    except _native.KrispHipError as e:
        if e.code != _native.ERR_CAPACITY or len(files) < 2 or _forced_batch() is not None:
            raise
        if run.verbose:
            print(f"=> the genome set does not fit the device at once ({e}): in batches", file=sys.stderr)
    return _device_ingest_flow(files, run, (len(files) + 1) // 2)


def _ingest_plan(files, run):
    """what the files' sizes say before one is read (no device involved) -> (est: the longest text in bytes, from above,
    0 if a file cannot be asked; whether the context's memory is reserved ahead of the texts; reader threads)"""
    try:
        est = max(fasta.estimate_text_bytes(f) for f in files)
    except OSError:
        est = 0
    ahead = int(os.environ.get("KRISP_RESERVE_MIN", RESERVE_MIN)) <= est < (1 << 32) - 128 and os.environ.get("KRISP_RESERVE") != "0"
    # files whose inflate takes every host thread by itself (one large gzip member, a bz2 stream of many blocks) are read
    # one after the other: the first genome is parsed and sorted on the device while the second still inflates
    # (plain text files use no inflate threads: they keep their readers side by side -- ADVICE r4)
    alone = ahead and est >= int(os.environ.get("KRISP_STREAM_MIN", STREAM_MIN)) and \
        any(str(f).lower().endswith((".gz", ".bz2", ".bgz")) for f in files)
    return est, ahead, 1 if alone else run.workers


def _reserve_ahead(eng, nfiles, est, run):
    """large genomes: the context gets its memory (device memory another process has just given back takes the driver
    15-40 ms per GB to hand over: seconds at 3 Gbp) while the host threads read and inflate -- planned from the files'
    sizes, planned again by _texts_to_device if they said too little.  -> planned bases per genome, 0: not taken"""
    # kr_reserve is an optimisation (include/krisp_hip.h), and the plan is an ESTIMATE from the files' sizes (5 x
    # the compressed bytes where real sequence text is 3.3-4.5 x): a reservation that does not fit says nothing
    # about the run itself -- the reserved buffers go back and the unplanned route sizes the context from the
    # texts once they are read
    try:
        eng.set_params(*run.geo, omit_soft=run.omit_soft, max_bases=est)
        eng.reserve(list(range(nfiles)), est, with_text=True)
    except _native.KrispHipError as e:
        if run.verbose:
            print(f"=> memory plan for {est:,} bases per genome not taken ({e}): sizing from the texts instead", file=sys.stderr)
        _free_quietly(eng, range(nfiles))
        return 0
    return est


def _texts_to_device(eng, futures, files, planned, run):
    """every file's text -> its genome on the device, parsed and sorted (_ingest_genome).  While the plan stands
    (`planned` bases per genome reserved, no text longer than that so far) a genome goes as its text arrives, the files
    behind it still being read; the first text longer than the plan -- or no plan -- makes the texts wait for all sizes,
    and everything goes under max(len).  Each future is dropped as its result is taken (a Future keeps its result): a
    text handed over is unreferenced from then on.  -> (RNA per genome, IUPAC windows per genome, read_s, _Stages begun
    when the first text arrived and stamped to where the waiting texts are freed)"""
    got, waiting, stages = [], [], None
    for i in range(len(files)):
        text, universal = futures[i].result()
        futures[i] = None
        if stages is None:
            read_s = time.time() - run.t0       # (until the first text is there: from then on the device has work)
            stages = _Stages()
        if planned and len(text) <= planned and not waiting:
            got.append(_ingest_genome(eng, i, text, universal, run))
        else:
            waiting.append((text, universal))   # (no plan, or a file larger than planned: all sizes first)
        del text
    if waiting:
        if len(waiting) < len(files):
            # (a later file said too little about itself: everything again under a plan that holds them all -- the
            # texts already handed over are read once more)
            waiting = [fasta.read_text(f) for f in files[:len(files) - len(waiting)]] + waiting
        true_max = max(max(len(t) for t, _ in waiting), 1)
        for i in (range(len(files)) if planned else ()):
            eng.free(i)
        eng.set_params(*run.geo, omit_soft=run.omit_soft, max_bases=true_max)
        got = [_ingest_genome(eng, i, text, universal, run) for i, (text, universal) in enumerate(waiting)]
    stages.stamp("texts arrive, parse + sort launches")
    del waiting
    stages.stamp("texts freed")
    return [r for _, r, _ in got], [sp for _, _, sp in got], read_s, stages


def _intersect_packed(eng, ids, rna, run):
    """one n-way intersection of the sorted genomes -- of DNA and RNA genomes in the filter's mode 2 (set before it), less
    the candidates text tells apart --, and the counts behind it, which resolve the sorts.  -> (candidates, k-mers per genome)"""
    if _mixed(rna):
        eng.set_mixed_alphabets(True)
    ncand = eng.intersect(ids, run.flags, apply_filter=run.do_filter and not run.quirk_all_fail)
    if _mixed(rna) and ncand:
        ncand = _mixed_prefix_filter(eng, run.geo[0], run.geo[2])
    return ncand, [eng.count(i) for i in ids]


def _collect_packed(eng, ids, ncand, rna, specials, run):
    """the candidates' records, then the groups IUPAC windows touch.  -> (records, touched pairs, their groups)"""
    # (genomes listed by label: kr_collect's (key, position in the call) order is then the renderer's)
    by_label = sorted(ids, key=lambda i: run.labels[i])
    records = eng.collect(by_label) if (ncand and not run.quirk_all_fail) else np.empty(0, dtype=_native.RECORD)
    touched, sgroups = set(), []
    if any(specials) and not run.quirk_all_fail:
        touched, sgroups = _special_groups(eng, ids, run.labels, specials, run.geo, run.ingroup_labels, run.do_filter,
                                           rna_genomes=rna if _mixed(rna) else None)
    return records, touched, sgroups


def _device_ingest_flow(files, run, force_batch):
    """find_regions' packed path with the reader on the device: the host threads read and inflate, the main thread
    hands each text to the GPU (parse -> sort) as it arrives (the device reader equals kr_fasta_to_bases byte for byte:
    tests/test_gpu_kernels.py).  The phases and the device calls they make, in order: DESIGN.md section 1."""
    from concurrent.futures import ThreadPoolExecutor
    est, ahead, workers = _ingest_plan(files, run)
    ids = list(range(len(files)))
    with ThreadPoolExecutor(max_workers=workers) as pool, _engine(run.device) as eng:
        # a genome set the device cannot hold sorted at once goes through it in batches (the streaming flow below)
        batch = force_batch or (_plan_batch(eng, len(files), est) if len(files) > 1 else None)
        if batch is not None:
            return _find_regions_streaming(eng, pool, files, run, batch, max(est, 1))
        futures = [pool.submit(fasta.read_text, f) for f in files]
        planned = _reserve_ahead(eng, len(files), est, run) if ahead else 0
        rna, specials, read_s, stages = _texts_to_device(eng, futures, files, planned, run)
        ncand, counts = _intersect_packed(eng, ids, rna, run)
        stages.stamp("sorts + intersect")
        _say_counts(files, counts, run)
        records, touched, sgroups = _collect_packed(eng, ids, ncand, rna, specials, run)
        stages.stamp("collect")
    # (device_s ends where the context is gone: its buffers freed, the reader threads joined)
    stages.stamp("context freed")
    stats = {"read_s": read_s, "device_s": stages.last - stages.start,
             "kmers": int(sum(counts)) + sum(len(sp) for sp in specials), "candidates": int(ncand), "stage_s": stages.s}
    return _packed_result(records, run, rna, touched, sgroups, stats)


# ----------------------------------------------------------------------------
# genome sets larger than one GPU's memory: the streaming flow (SURVEY section 7 "HBM sizing")
# ----------------------------------------------------------------------------
STREAM_EAGER_MAX = 4_000_000     # running candidates up to which a batch's records are collected at once (64 MB per genome)


def _plan_batch(eng, nfiles, est_bases):
    """How many genomes of ~est_bases the context can hold sorted at once beside its scratch (None: all of them).  Per
    genome: the bases and two 8-byte keys per base (+ 2 % slack for key-space slices); scratch: codes + pass-1 output
    per sort lane (three at most), the pass-0 array of two genome lanes when the genome is sorted in slices (> 2^28
    bases), the text buffer of the device reader, candidate buffers.  KRISP_STREAM_BATCH=n forces batches of n."""
    forced = _forced_batch()
    if forced is not None:
        return max(1, forced) if forced < nfiles else None
    if est_bases <= 0:
        return None
    per_genome = 17.4 * est_bases
    sliced = est_bases > (1 << 28)
    scratch = (2 * 16.2 * est_bases + 3 * 17.0 * est_bases / 16) if sliced else 3 * 17.0 * est_bases
    scratch += est_bases + (2 << 30)
    avail = eng.mem_info()["avail"]
    fit = int((avail - scratch) // per_genome)
    if fit >= nfiles:
        return None
    return max(1, fit)


def _interleave(a, b):
    """a[0], b[0], a[1], b[1], ... and the longer list's tail: a first batch, a round-robin shard holds both kinds"""
    n = min(len(a), len(b))
    return [x for pair in zip(a, b) for x in pair] + a[n:] + b[n:]


def _first_min(flags, apply_f):
    """the least size of the first batch of genomes with these ingroup flags: it must hold both sides when there are two
    and the filter applies -- with one side only nothing prunes, and its candidate list is every (left,right) pair of its
    genomes (more than 2^32 entries at 3 Gbp -- the library refuses such a list, kr_intersect: KR_ERR_CAPACITY)"""
    return 2 if (_mixed(flags) and apply_f) else 1


def _batches(order, bsz, first_min):
    """`order` in slices of bsz, the first of max(bsz, first_min) (_first_min; `order` is interleaved: _interleave)"""
    a = 0
    while a < len(order):
        m = max(bsz, first_min) if a == 0 else bsz
        yield order[a:a + m]
        a += m


def _intersect_or_probe(eng, running, ids_b, flags, filt):
    """the batch ids_b against the running candidates (`running` of them, None before the first batch): the first batch
    is intersected; a later one looks the running candidates up in its genomes -- kr_cands_probe: presence in every
    genome, their diagnostic bases into the masks, the filter -- instead of being intersected whole: the candidate list
    of a batch that holds one side only is every prefix of its genomes, 24 bytes each.  -> the number left"""
    fl = [flags[g] for g in ids_b]
    if running is None:
        return eng.intersect(ids_b, fl, apply_filter=filt)
    return eng.probe_cands(ids_b, fl, apply_filter=filt)


class _Stream:
    """the streaming flow's state: what its passes work from and what they have learnt so far"""

    def __init__(self, eng, pool, files, run, batch, max_bases):
        n = len(files)
        self.eng, self.pool, self.files, self.run = eng, pool, files, run
        self.max_bases = max_bases      # what the context is sized for: raised when a text is longer than its file said
        self.order = _interleave([i for i in range(n) if run.flags[i]], [i for i in range(n) if not run.flags[i]])
        self.apply_f = run.do_filter and not run.quirk_all_fail
        self.first_min = _first_min(run.flags, self.apply_f)
        self.rank_of = {g: r for r, g in enumerate(sorted(range(n), key=lambda i: run.labels[i]))}
        self.rna, self.specials, self.counts = [None] * n, [None] * n, [0] * n     # per genome (pass 1 fills them)
        self.read_s = None              # until the first batch's texts were there
        # number of running candidates; the list itself stays on the device between the batches of pass 1 (kr_genome_free
        self.running = None             # does not touch it: no copy to the host and back per batch -- ADVICE r5)
        self.eager = True               # the running set is small enough to collect every batch's records of it at once
        self.kept = []                  # those records (pass 1), or the final candidates' (pass 2): a part per batch
        # after pass 1: the candidates it leaves, _touched_prefix_cands of the IUPAC windows
        self.final, self.touched, self.tc = None, set(), None
        self.srecs = []                 # pass 2: the records of `tc`, a part per batch
        self.stats = {"streamed": True, "batch": batch, "passes": 1, "batches": 0}


def _stream_load(st, ids_b, futs, first_pass):
    """texts -> device, sorted; a batch that does not fit after all is given back whole (KrispHipError, code capacity)"""
    eng, run, done = st.eng, st.run, []
    texts = {g: futs[g].result() for g in ids_b}
    if st.read_s is None:
        st.read_s = time.time() - run.t0
    biggest = max(len(t) for t, _ in texts.values())
    if biggest > st.max_bases:
        # (the plan came from the files' sizes: a text longer than it said -- nothing is resident between batches)
        st.max_bases = biggest
        eng.set_params(*run.geo, omit_soft=run.omit_soft, max_bases=biggest)
    try:
        for g in ids_b:
            text, universal = texts.pop(g)
            done.append(g)          # (before the ingest: a genome that fails half way holds buffers, too -- ADVICE r5)
            _n, r, sp = _ingest_genome(eng, g, text, universal, run)
            del text
            if first_pass:
                st.rna[g], st.specials[g] = r, sp
        for g in ids_b:
            st.counts[g] = eng.count(g)
    except _native.KrispHipError:
        _free_quietly(eng, done)
        raise


def _halve_batch(ids_b, first_min, first, e):
    """a batch the device could not hold (e: the capacity error) -> its two halves; `first`: it is the first batch of
    the first pass, which keeps first_min genomes (_first_min).  What cannot be halved raises: one genome e itself, a
    first batch of first_min the error that says why it must stay whole"""
    if len(ids_b) == 1:
        raise e
    if first and len(ids_b) <= first_min:
        err = _native.KrispHipError(
            f"the device cannot hold one ingroup and one outgroup genome sorted at once ({e}); the first batch "
            "needs both sides for the diagnostic filter to prune")
        err.code = e.code
        raise err from e
    half = max((len(ids_b) + 1) // 2, first_min if first else 1)
    return ids_b[:half], ids_b[half:]


def _stream_pass(st, bsz, first_pass, work):
    """every batch through _stream_load + work(st, ids_b); the next batch's files are read while this one is on the
    device; a batch the device cannot hold is halved and tried again (the plan is an estimate)"""
    todo = list(_batches(st.order, bsz, st.first_min))
    futs = {}
    while todo:
        ids_b = todo.pop(0)
        for g in ids_b + (todo[0] if todo else []):
            if g not in futs:
                futs[g] = st.pool.submit(fasta.read_text, st.files[g])
        try:
            _stream_load(st, ids_b, futs, first_pass)
        except _native.KrispHipError as e:
            if e.code != _native.ERR_CAPACITY:
                raise
            halves = _halve_batch(ids_b, st.first_min, first_pass and st.running is None, e)
            todo = list(halves) + todo
            for g in ids_b:
                futs[g] = st.pool.submit(fasta.read_text, st.files[g])
            st.stats["batch"] = min(st.stats["batch"], len(halves[0]))
            continue
        work(st, ids_b)
        for g in ids_b:
            st.eng.free(g)
            del futs[g]
        st.stats["batches"] += 1


def _stream_pass1(st, ids_b):
    """the batch prunes the running candidates; its records of them are kept while that set is small"""
    st.running = _intersect_or_probe(st.eng, st.running, ids_b, st.run.flags, st.apply_f)
    _say_counts([st.files[g] for g in ids_b], [st.counts[g] for g in ids_b], st.run)
    if st.run.quirk_all_fail or not st.running:
        return
    if st.eager and st.running <= STREAM_EAGER_MAX:
        st.kept.append(st.eng.collect(sorted(ids_b, key=lambda g: st.rank_of[g])))
    else:
        st.eager = False
        st.kept.clear()


def _stream_pass2(st, ids_b):
    """the batch's records of the final candidates (if pass 1 could not keep them) and of the touched pairs"""
    by = sorted(ids_b, key=lambda g: st.rank_of[g])
    if len(st.final) and not st.eager:
        st.eng.load_cands(st.final)
        st.kept.append(st.eng.collect(by))
    if len(st.tc):
        st.eng.load_cands(st.tc)
        st.srecs.append(st.eng.collect(by))


def _stream_assemble(st, mixed):
    """the end of the flow: the kept records of the final candidates' prefixes in (key, label rank) order -- what one
    collect in label order gives the in-core flow --, and the touched groups from the second pass's records.
    -> (records, the touched pairs' groups)"""
    run, n = st.run, len(st.files)
    records = np.empty(0, dtype=_native.RECORD)
    if st.kept and len(st.final):
        records = np.concatenate(st.kept)
        records = records[np.isin(records["key"] & codec.prefix_mask(run.geo[0], run.geo[2]), st.final["prefix"])]
        ranks = np.array([st.rank_of[g] for g in range(n)], dtype=np.int64)[records["genome"]]
        records = records[np.lexsort((ranks, records["key"]))]
    sgroups = []
    if st.touched:
        recs = np.concatenate(st.srecs) if st.srecs else None
        sgroups = _special_groups_from(recs, list(range(n)), run.labels, st.specials, run.geo, run.ingroup_labels,
                                       run.do_filter, rna_genomes=[bool(r) for r in st.rna] if mixed else None)
    return records, sgroups


def _find_regions_streaming(eng, pool, files, run, batch, max_bases):
    """find_regions for a genome set that does not fit the GPU at once (the reference has no such limit: it sorts in
    external memory, kstream.py:108-119, and merges files pairwise, intersectAmplicons.py:232-310): the genomes go through
    the device in batches of `batch`.  Pass 1 sorts a batch, prunes the running candidates with it (the filter's predicate
    is monotone, so partial masks may prune -- in and out genomes are interleaved so that the first batch holds both),
    keeps the batch's records of them (a superset of the final ones') and frees it.  Only when the running set was too
    large to collect from (no outgroup, no filter: every conserved pair is a candidate) or IUPAC windows touch groups
    whose ACGT members must be looked up, pass 2 sorts every batch again and collects then.  Same records, same order, same
    text as the in-core flow (tests/test_gpu_cli.py); the phases and their device calls: DESIGN.md section 8.  -> (groups, stats)"""
    t1 = time.time()
    eng.set_params(*run.geo, omit_soft=run.omit_soft, max_bases=max_bases)
    st = _Stream(eng, pool, files, run, batch, max_bases)
    # every genome's alphabet before the first batch (fasta.sniff_rna reads the head of a file): a run that mixes DNA and
    # RNA genomes filters in mode 2 from the first batch on (kr_set_mixed_alphabets)
    mixed = _mixed([bool(fasta.sniff_rna(f)) for f in files])
    if mixed:
        eng.set_mixed_alphabets(True)
    _stream_pass(st, batch, True, _stream_pass1)
    if mixed and st.running:
        st.running = _mixed_prefix_filter(eng, run.geo[0], run.geo[2])
    st.final = eng.cands().copy() if st.running else np.empty(0, dtype=_native.CAND)
    st.touched, st.tc = _touched_prefix_cands([] if run.quirk_all_fail else st.specials)
    if (len(st.final) and not st.eager and not run.quirk_all_fail) or len(st.tc):
        st.stats["passes"] = 2
        _stream_pass(st, max(1, st.stats["batch"]), False, _stream_pass2)
    records, sgroups = _stream_assemble(st, mixed)
    rna = [bool(r) for r in st.rna]
    st.stats.update(mixed_rna=rna if mixed else None, read_s=st.read_s or 0.0, candidates=int(len(st.final)),
                    kmers=int(sum(st.counts)) + sum(len(sp) for sp in st.specials), device_s=time.time() - t1)
    return _packed_result(records, run, rna, st.touched, sgroups, st.stats)


# what the host keeps of a wide run's genomes once they are on the device: their bases (None where the device parsed the
# files); per genome the number of bases, RNA or not, the IUPAC windows as (left, diag, right); _touched_pairs of those
_WideSetup = namedtuple("_WideSetup", "texts nb rna specials touched probes probe_text")


def _wide_setup_host(eng, loaded, run):
    """loaded: fasta.ingest of every file.  The bases are uploaded; the context also holds the probe text.  -> _WideSetup"""
    texts = [b for b, _, _ in loaded]
    specials = [[codec.split_window(w, *run.geo) for w in sp] for _, _, sp in loaded]
    touched, probes, probe_text = _touched_pairs(specials, run.geo[1])
    eng.set_params_wide(*run.geo, omit_soft=run.omit_soft, max_bases=max(max(len(t) for t in texts), len(probe_text)))
    for i, t in enumerate(texts):
        eng.upload(i, t)
    return _WideSetup(texts, [len(t) for t in texts], [bool(r) for _, r, _ in loaded], specials, touched, probes, probe_text)


def _wide_setup_device(eng, loaded, run):
    """loaded: fasta.read_text of every file, each let go once the device has parsed it (_ingest_genome).
    -> _WideSetup without texts, or None: the probe text is longer than the context was sized for -- the host parse"""
    maxb = max(max(len(t) for t, _ in loaded), 64)
    eng.set_params_wide(*run.geo, omit_soft=run.omit_soft, max_bases=maxb)
    got = []
    for i, (text, universal) in enumerate(loaded):
        got.append(_ingest_genome(eng, i, text, universal, run))
        loaded[i] = None
    nb, rna, specials = [n for n, _, _ in got], [bool(r) for _, r, _ in got], [sp for _, _, sp in got]
    touched, probes, probe_text = _touched_pairs(specials, run.geo[1])
    return None if len(probe_text) > maxb else _WideSetup(None, nb, rna, specials, touched, probes, probe_text)


def _wide_text_groups(hits, texts, run, rna, touched, sgroups):
    """the groups of a wide run where text decides (one GPU's and rank 0's): a run that mixes DNA and RNA genomes goes
    through _mixed_wide_groups, the groups IUPAC windows touch are replaced by `sgroups` (rebuilt by the caller from its
    own look-ups), an all-RNA run is written with U"""
    mixed = _mixed(rna)
    groups = _groups_from_hits(hits, texts, run.labels, *run.geo, rna_genomes=rna if mixed else None)
    if mixed:
        groups = _mixed_wide_groups(groups, run)
        touched = touched | {(g[0].left, g[0].right) for g in sgroups}
    if touched:
        groups = _merge_groups(groups, touched, sgroups)
    return _to_rna(groups) if all(rna) else groups


def _wide_result(eng, run, su, nhits, hits, ngroups):
    """the hits of one GPU's kr_wide_run -> (groups, their number)"""
    mixed = _mixed(su.rna)
    if not mixed and not su.touched:
        # the member windows are cut on the device (kr_wide_fetch_windows) and rendered from their rows in the library
        # (amplicon.WindowGroups: no object per window; the list of groups only if someone walks it; the RNA letters are its)
        rows = eng.wide_windows(run.k) if nhits else np.empty((0, run.k), dtype=np.uint8)
        return amplicon.WindowGroups(rows, hits["cand"], hits["genome"], run.labels, *run.geo, rna=all(su.rna)), ngroups
    # (the device parsed the files: their bases come back now that text decides)
    texts = su.texts if su.texts is not None else [eng.fetch_bases(i, n).copy() for i, n in enumerate(su.nb)]
    sgroups = _special_groups_wide(eng, texts, run.labels, su.specials, su.touched, su.probes, su.probe_text, run.geo, run.ingroup_labels,
                                   run.do_filter, rna_genomes=su.rna if mixed else None) if su.touched else []
    groups = _wide_text_groups(hits, texts, run, su.rna, su.touched, sgroups)
    return groups, (len(groups) if mixed else ngroups)


def _find_regions_wide(files, run, host_parse):
    """find_regions for amplicons longer than one key (kr_wide_run).  The files are read (and inflated) on host threads,
    every text goes to the device as it is (fasta.ingest_on_device: kr_genome_upload_text, or kr_genome_upload_bgzf for a
    BGZF file), and the host sees a genome's bases again only where it needs them -- IUPAC windows (scan_special), mixed
    DNA / RNA runs, the groups IUPAC windows touch -- through kr_genome_fetch_bases.  host_parse: the files are parsed on
    the host threads (fasta.ingest) and their bases uploaded -- for a run whose groups all fail the filter, and for one
    whose probe text is longer than its genomes: without host_parse that one returns None.  -> (groups, stats)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=run.workers) as pool:
        loaded = list(pool.map((lambda f: fasta.ingest(f, run.k, run.omit_soft)) if host_parse else fasta.read_text, files))
    stats = {"read_s": time.time() - run.t0}
    t1 = time.time()
    if run.quirk_all_fail:
        stats.update(device_s=0.0, kmers=0, candidates=0)
        return [], stats
    with _engine(run.device) as eng:
        # k-mers holding IUPAC letters (kept by the reference): the (left,right) groups they touch are rebuilt on the host;
        # those with plain flanks need their ACGT members from every genome, found through a probe "genome" of these pairs
        su = (_wide_setup_host if host_parse else _wide_setup_device)(eng, loaded, run)
        if su is None:
            return None
        if _mixed(su.rna):
            eng.set_mixed_alphabets(True)
        nhits = eng.wide_run(list(range(len(files))), run.flags, apply_filter=run.do_filter)
        hits = eng.wide_fetch(_native.WIDE_HITS) if nhits else np.empty(0, dtype=_native.WIDE_HIT)
        ngroups = int(eng.wide_fetch(_native.WIDE_NGROUPS)[0])
        counts = eng.wide_fetch(_native.WIDE_COUNTS).tolist()
        stats["wide_batch"] = int(eng.wide_fetch(_native.WIDE_BATCH_USED)[0])       # (0: every genome sorted at once)
        _say_counts(files, counts, run)
        groups, ngroups = _wide_result(eng, run, su, nhits, hits, ngroups)
    stats.update(device_s=time.time() - t1, kmers=int(sum(counts)) + sum(len(sp) for sp in su.specials), candidates=ngroups)
    return groups, stats


# ----------------------------------------------------------------------------
# the fused device flow used by main()
# ----------------------------------------------------------------------------
def find_regions(ingroup_files, outgroup_files, L, R, amplicon_len, omit_soft=False,
                 device=0, verbose=False, keep_merged=False, wide=None):
    """FASTA files -> list of surviving groups (amplicon.Amplicon lists).

    = extractSortedKmers per file + mergeFiles + filterAlignments of the reference (krisp_fasta.py:237-272), on the GPU:
    one sort per genome, one n-way intersection with the diagnostic filter fused in, one collect.  Returns (groups, stats)."""
    files = list(ingroup_files) + list(outgroup_files)
    # mergeFiles moves the lone k-mer file; its lines carry no label, so later stages
    # label them with the file they read: simplename('merged_file.txt') (shared.py:373)
    labels = ["merged_file"] if len(files) == 1 else [simplename(f) for f in files]
    run = _describe_run(labels, ingroup_files, L, R, amplicon_len, omit_soft, device, verbose, wide)
    if run.wide and run.quirk_all_fail:
        return _find_regions_wide(files, run, host_parse=True)
    # files are read and inflated concurrently on the host (the library releases the GIL); the PARSE runs on the device,
    # genome by genome as the texts arrive (fasta.ingest_on_device), each followed at once by its sort -- round 6: amplicons
    # longer than one key, too (the host's parser was the larger half of such a run from files: 1.8 of 2.4 s at 8 x 500 Mbp,
    # tools/e2e_profile.py)
    while True:
        try:
            got = _find_regions_wide(files, run, host_parse=False) if run.wide else _find_regions_device_ingest(files, run)
            break
        except fasta.GzipTextLonger as e:
            # (a `.gz` file of several members handed to the device inflate: the run's plan came from its last member's
            # length -- again from the start, that file read on the host: each round takes one more file off the device)
            if verbose:
                print(f"=> {e}: again, that file inflated on the host", file=sys.stderr)
    if got is None:
        # (a genome set whose IUPAC windows make a probe text longer than its genomes -- tiny inputs: the host parse)
        got = _find_regions_wide(files, run, host_parse=True)
    return got


class PeerFailed(RuntimeError):
    """another rank of a multi-GPU run raised; this rank stops with it instead of waiting in a collective"""


class _Rank(NamedTuple):
    """one rank of a multi-GPU run as its phases see it (_rank_read_and_agree fills it)"""
    eng: object                 # its context, connected to the other ranks'
    rank: int
    world: int
    order: list                 # the run's files, ingroup and outgroup interleaved: a genome's number is its place here
    mine: list                  # the genomes this rank holds (distributed.shard)
    loaded: list                # fasta.ingest of each of them: (bases, is RNA, windows with IUPAC letters)
    run: _Run
    max_bases: int              # the longest genome of any rank
    mixed: bool                 # DNA and RNA genomes in one run
    all_rna: bool
    rna_all: list               # a mixed run: RNA or not, per genome of the run (else None)
    specials_all: list          # every genome's IUPAC windows as (left, diag, right) when any rank has one (else None)


def _together(eng, rank, fn):
    """run fn() on this rank; every rank learns whether all succeeded before anyone goes on (one all-reduce per call)"""
    err, out = None, None
    try:
        out = fn()
    except BaseException as e:  # noqa: BLE001
        err = e
    failed = eng.comm_allreduce([1.0 if err is not None else 0.0], "max")[0] > 0
    if err is not None:
        raise err
    if failed:
        raise PeerFailed(f"rank {rank}: another rank failed")
    return out


def _allgather_json(eng, obj):
    """every rank's `obj`, in rank order, on every rank (one kr_comm_allgather).  Plain data only -- numbers, strings,
    lists, dicts (whose keys come back as strings) --: nothing executable crosses ranks"""
    return [json.loads(blob.decode()) for blob in eng.comm_allgather(json.dumps(obj).encode())]


def _rank_read_and_agree(eng, rank, world, order, run):
    """phase 1: the rank reads its files (distributed.shard), and the ranks agree on what the run holds: the longest
    genome, the alphabets, every window with IUPAC letters.  -> _Rank"""
    mine = distributed.shard(list(range(len(order))), rank, world)
    loaded = _together(eng, rank, lambda: [fasta.ingest(order[g], run.k, run.omit_soft) for g in mine])
    kinds = eng.comm_allreduce([1.0 if any(sp for _, _, sp in loaded) else 0.0,
                                1.0 if any(r for _, r, _ in loaded) else 0.0,
                                float(max(len(b) for b, _, _ in loaded)),
                                1.0 if any(not r for _, r, _ in loaded) else 0.0], "max")
    mixed = bool(kinds[1] and kinds[3])
    rna_all = None
    if mixed:
        # DNA and RNA genomes in one run (find_regions has the rules): every rank learns every genome's alphabet, every
        # context filters in mode 2, the candidates whose (left,right) pair holds T / U go, rank 0 decides the rest on text
        if kinds[0]:
            raise MixedAlphabet("some genomes are RNA (U) and some DNA (T), and windows hold IUPAC letters")
        mine_rna = {g: bool(r) for g, (_, r, _) in zip(mine, loaded)}
        got = {int(g): r for part in _allgather_json(eng, mine_rna) for g, r in part.items()}
        rna_all = [got[g] for g in range(len(order))]
        eng.set_mixed_alphabets(True)
    # windows with IUPAC letters (kept by the reference, kstream.py:11-18; the device alphabet cannot carry them):
    # every rank learns all of them -- they are rare --, the groups they touch are rebuilt on rank 0 from the
    # ranks' device look-ups of the ACGT members, as find_regions does on one GPU
    specials_all = None
    if kinds[0]:
        mine_sp = {g: [codec.split_window(w, *run.geo) for w in sp] for g, (_, _, sp) in zip(mine, loaded)}
        got = {int(g): sp for part in _allgather_json(eng, mine_sp) for g, sp in part.items()}
        specials_all = [[tuple(w) for w in got[g]] for g in range(len(order))]
    return _Rank(eng, rank, world, order, mine, loaded, run, int(kinds[2]), mixed, bool(kinds[1]) and not mixed,
                 rna_all, specials_all)


def _wide_shard_run(rk):
    """the rank's genomes through kr_wide_run, which exchanges the spectra lists, the group list and the kept groups'
    masks itself (the same calls in the same order on every rank).  -> (hits: genomes by their global number, k-mers, groups)"""
    eng, run = rk.eng, rk.run
    eng.set_params_wide(*run.geo, omit_soft=run.omit_soft, max_bases=rk.max_bases)
    for g, (bases, _, _) in zip(rk.mine, rk.loaded):
        eng.upload(g, bases)
    nh = eng.wide_run(rk.mine, [run.flags[g] for g in rk.mine], apply_filter=run.do_filter)
    return nh, int(sum(eng.wide_fetch(_native.WIDE_COUNTS).tolist())), int(eng.wide_fetch(_native.WIDE_NGROUPS)[0])


def _wide_shard_probe(rk, probes, probe_text):
    """the ACGT members of the touched pairs with plain flanks in THIS rank's genomes -- in a context of its own without
    a communicator: the look-ups are local, one kr_wide_run per genome.  -> _wide_probe_members' dict"""
    if not probes:
        return {}
    with _native.Engine(device=rk.run.device) as e2:
        e2.set_params_wide(*rk.run.geo, omit_soft=rk.run.omit_soft, max_bases=max(rk.max_bases, len(probe_text)))
        for g, (bases, _, _) in zip(rk.mine, rk.loaded):
            e2.upload(g, bases)
        return _wide_probe_members(e2, [b for b, _, _ in rk.loaded], list(rk.mine), probes, probe_text, rk.run.geo,
                                   pid=len(rk.order))


def _rank_wide(rk, stats):
    """phase 2 of a run whose amplicons are longer than one key: kr_wide_run, the IUPAC windows' probe look-ups, rank
    0's text cutting.  -> (groups on rank 0, None elsewhere; stats)"""
    eng, rank, run = rk.eng, rk.rank, rk.run
    t1 = time.time()
    if run.quirk_all_fail:
        eng.comm_barrier()
        stats.update(device_s=0.0, kmers=0, candidates=0, records=0)
        return ([] if rank == 0 else None), stats
    nh, counts, ngroups = _together(eng, rank, lambda: _wide_shard_run(rk))
    hits = eng.wide_fetch(_native.WIDE_HITS) if (rank == 0 and nh) else np.empty(0, dtype=_native.WIDE_HIT)
    # windows with IUPAC letters: every rank knows all of them (specials_all), so every rank derives the same touched
    # (left,right) pairs and the same probe genome and looks the pairs' ACGT members up in ITS genomes; rank 0 gets
    # everybody's findings and rebuilds the touched groups
    touched, members = set(), {}
    if rk.specials_all is not None:
        touched, probes, probe_text = _touched_pairs(rk.specials_all, run.geo[1])
        local = _together(eng, rank, lambda: _wide_shard_probe(rk, probes, probe_text))
        flat = [[list(P), list(seq), int(g), int(cnt)] for P, seqs in local.items() for seq, m in seqs.items()
                for g, cnt in m.items()]
        for part in _allgather_json(eng, flat):
            for P, seq, g, cnt in part:
                m = members.setdefault(tuple(P), {}).setdefault(tuple(seq), {})
                m[g] = m.get(g, 0) + cnt
    eng.comm_barrier()
    stats.update(device_s=time.time() - t1, kmers=counts, candidates=ngroups, records=int(len(hits)))
    if rank != 0:
        return None, stats
    # rank 0 cuts the windows' text: its own genomes are in memory, the others' files are read here
    texts = {g: bases for g, (bases, _, _) in zip(rk.mine, rk.loaded)}
    for g in sorted(set(hits["genome"].tolist()) - set(texts)):
        texts[g] = fasta.ingest(rk.order[g], run.k, run.omit_soft)[0]
    # (a mixed run holds no IUPAC windows: MixedAlphabet in _rank_read_and_agree)
    sg = _touched_groups(members, len(rk.order), run.labels, rk.specials_all, touched, run.ingroup_labels,
                         run.do_filter) if rk.specials_all is not None else []
    wg = _wide_text_groups(hits, [texts.get(g) for g in range(len(rk.order))], run,
                           rk.rna_all if rk.mixed else [rk.all_rna] * len(rk.order), touched, sg)
    if rk.mixed:
        stats["candidates"] = len(wg)
    return wg, stats


def _shard_batches(rk, bsz):
    """the rank's genomes through its device, bsz at a time: upload and sort a batch, hand it to the caller's loop body,
    free it.  bsz None: the whole shard at once, and it stays on the device"""
    eng, run = rk.eng, rk.run
    bases_of = {g: b for g, (b, _, _) in zip(rk.mine, rk.loaded)}
    first_min = _first_min([run.flags[g] for g in rk.mine], run.do_filter and not run.quirk_all_fail)
    for ids_b in ([rk.mine] if bsz is None else _batches(rk.mine, bsz, first_min)):
        for g in ids_b:
            eng.upload(g, bases_of[g])
            eng.sort(g)
        yield ids_b
        if bsz is not None:
            for g in ids_b:
                eng.free(g)


def _shard_intersect(rk, filt):
    """the rank's candidates from its own genomes (safe local pruning).  A shard that does not fit its GPU sorted at once
    goes through it in batches, as find_regions does on one GPU (_find_regions_streaming): the first intersected, the
    later ones probed; KRISP_STREAM_BATCH=n forces batches of n per rank (tests).  -> (batch size or None, k-mers)"""
    eng, run = rk.eng, rk.run
    eng.set_params(*run.geo, omit_soft=run.omit_soft, max_bases=rk.max_bases)
    bsz = _plan_batch(eng, len(rk.mine), rk.max_bases) if len(rk.mine) > 1 else None
    total, running = 0, None
    for ids_b in _shard_batches(rk, bsz):
        running = _intersect_or_probe(eng, running, ids_b, run.flags, filt)
        total += sum(eng.count(g) for g in ids_b)
    return bsz, total


def _shard_collect(rk, bsz, cands=None):
    """the rank's records of the candidates on the device (of `cands`, loaded first, if given).  bsz None: the shard is
    there -- one kr_collect, the records stay in its buffer -> their number; else a pass over the batches -> the records"""
    eng = rk.eng
    if cands is not None:
        eng.load_cands(cands)
    if bsz is None:
        return eng.collect(rk.mine, fetch=False)
    cands = eng.cands().copy()
    parts = []
    for ids_b in _shard_batches(rk, bsz):
        eng.load_cands(cands)
        if len(cands):
            parts.append(eng.collect(ids_b))
    return np.concatenate(parts) if parts else np.empty(0, dtype=_native.RECORD)


def _records_to_rank0(rk, any_batched, bsz, cands=None, wanted=True):
    """every rank's records of the candidates (of `cands`) -> rank 0: one _together (_shard_collect; no work in it if not
    wanted), then, if wanted, their way there -- as bytes (kr_comm_allgather) when any rank took its shard in batches,
    else from the device buffers (kr_records_gather).  -> (this rank's number of records, all records on rank 0)"""
    eng = rk.eng
    local = _together(eng, rk.rank, lambda: _shard_collect(rk, bsz, cands) if wanted else 0)
    if not wanted:
        return 0, None
    if not any_batched:
        total = eng.records_gather()
        return local, (eng.fetch_records(total) if rk.rank == 0 else None)
    got = eng.comm_allgather(np.ascontiguousarray(local).tobytes())
    if rk.rank != 0:
        return len(local), None
    parts = [np.frombuffer(b, dtype=_native.RECORD) for b in got if len(b)]
    return len(local), (np.concatenate(parts) if parts else np.empty(0, dtype=_native.RECORD))


def _rank_packed(rk, stats):
    """phase 2 of a run of packed keys: local candidates, their reduction over the ranks, the survivors' records and the
    IUPAC look-ups' records to rank 0.  -> (records, touched pairs, the look-ups' records)"""
    eng, rank, run = rk.eng, rk.rank, rk.run
    t1 = time.time()
    filt = run.do_filter and not run.quirk_all_fail
    bsz, counts = _together(eng, rank, lambda: _shard_intersect(rk, filt))
    # every rank learns whether ANY rank took its shard in batches: the records are then collected in a second pass over
    # the shard and travel to rank 0 as bytes on all of them, instead of from the device buffer of ONE kr_collect
    any_batched = eng.comm_allreduce([1.0 if bsz is not None else 0.0], "max")[0] > 0
    if any_batched and bsz is None:
        bsz = len(rk.mine)
    ncand = eng.cands_reduce(apply_filter=filt)
    eng.cands_bcast()
    if rk.mixed:                # (the same list on every rank: the same cut)
        _together(eng, rank, lambda: _mixed_prefix_filter(eng, run.geo[0], run.geo[2]))
    nrec, allrec = _records_to_rank0(rk, any_batched, bsz, wanted=not run.quirk_all_fail)
    sprec, touched = None, set()
    if rk.specials_all is not None and not run.quirk_all_fail:
        # the ACGT members of every (left,right) group an IUPAC window touches: each rank looks them up in ITS
        # genomes (the touched prefixes as a candidate list), rank 0 gets all the records
        touched, tc = _touched_prefix_cands(rk.specials_all)
        _, sprec = _records_to_rank0(rk, any_batched, bsz, cands=tc, wanted=len(tc) > 0)
    eng.comm_barrier()
    stats.update(device_s=time.time() - t1, kmers=int(counts) + sum(len(sp) for sp in rk.specials_all or []),
                 candidates=int(max(ncand, 0)), records=int(nrec))
    return allrec, touched, sprec


def _distributed_rank(rank, world, device, connect, ingroup_files, outgroup_files, L, R, amplicon_len, omit_soft):
    """one rank of the multi-GPU flow (see find_regions_distributed); `connect(engine)` gives the
    engine its communicator.  Returns (groups, stats) on rank 0 and (None, stats) elsewhere.  Every rank issues the same
    collectives in the same order (DESIGN.md section 8 lists them): the phases below, read top to bottom."""
    # (interleaved so that a round-robin shard holds both kinds; a lone genome is labelled by its file here)
    order = _interleave(list(ingroup_files), list(outgroup_files))
    run = _describe_run([simplename(f) for f in order], list(ingroup_files), L, R, amplicon_len, omit_soft, device, False)
    if len(order) < world:
        raise ValueError(f"{len(order)} genomes cannot be sharded over {world} GPUs")
    with _native.Engine(device=device) as eng:
        connect(eng)
        run = run._replace(t0=time.time())          # (the clock starts once the rank is connected)
        rk = _rank_read_and_agree(eng, rank, world, order, run)
        stats = {"read_s": time.time() - run.t0}
        if run.wide:                                # (amplicons longer than one key: kr_wide_run)
            return _rank_wide(rk, stats)
        allrec, touched, sprec = _rank_packed(rk, stats)
    if rank != 0:
        return None, stats
    sgroups = _special_groups_from(sprec, list(range(len(order))), run.labels, rk.specials_all, run.geo,
                                   run.ingroup_labels, run.do_filter) if touched else []
    # (a mixed run holds no IUPAC windows: MixedAlphabet in _rank_read_and_agree)
    return _packed_result(allrec, run, rk.rna_all if rk.mixed else [rk.all_rna] * len(order), touched, sgroups, stats)


def find_regions_distributed(ingroup_files, outgroup_files, L, R, amplicon_len, omit_soft=False,
                             transport="rccl", verbose=False):
    """find_regions over several GPUs: one process per GPU (started by torch.distributed.run, mpirun, srun ...: RANK /
    LOCAL_RANK / WORLD_SIZE in the environment; no PyTorch involved).  Genomes are sharded round-robin over the ranks
    (ingroup and outgroup files interleaved so that every rank can prune with the monotone filter); each rank sorts and
    intersects its own -- in batches when its shard does not fit its GPU sorted at once --, the candidate lists are
    tree-reduced between the GPUs (kr_cands_reduce: RCCL, device to device), the survivors broadcast, every rank collects
    its genomes' records and rank 0 gathers them.  Amplicons longer than one key take kr_wide_run, which exchanges the
    flank spectra, the group list and the kept groups' masks between the ranks itself.  Windows with IUPAC letters go to
    every rank; each looks the ACGT members of the groups they touch up in its genomes, rank 0 rebuilds those groups.  An
    all-RNA run is written with U; one that mixes DNA and RNA genomes filters in the mixed mode and rank 0 decides on text
    (MixedAlphabet if it holds IUPAC windows too).  A rank that fails (missing file, illegal character, out of memory)
    makes every rank raise before the next collective.  Returns (groups, stats) on rank 0 and (None, stats) elsewhere."""
    rank, local_rank, world = distributed.env_rank_world()
    if transport == "dir":                 # rehearsal: the ranks share the visible GPU(s)
        local_rank %= max(1, int(os.environ.get("KRISP_VISIBLE_GPUS", "1")))
    return _distributed_rank(rank, world, local_rank, lambda eng: distributed.connect(eng, rank, world, transport=transport),
                             ingroup_files, outgroup_files, L, R, amplicon_len, omit_soft)


def find_regions_multi_device(ingroup_files, outgroup_files, L, R, amplicon_len, devices, omit_soft=False,
                              verbose=False):
    """The same flow inside ONE process: a thread per listed device (the library calls release the
    GIL), each with its own context and communicator -- the fallback for hosts where a launcher
    is not at hand.  Distinct devices talk over RCCL (the unique id is passed between
    the threads); a device listed twice makes the exchange go through files instead (RCCL refuses
    duplicate devices): that is how a one-GPU box rehearses it.  Returns (groups, stats)."""
    import tempfile
    import threading
    world = len(devices)
    if world < 1:
        raise ValueError("find_regions_multi_device: no device listed")
    use_rccl = len(set(devices)) == world
    cid = _native.comm_unique_id() if use_rccl else None
    results, errors = [None] * world, [None] * world
    with tempfile.TemporaryDirectory(prefix="krisp_comm_") as td:
        def work(rank):
            connect = (lambda eng: eng.comm_init(rank, world, cid)) if use_rccl else \
                (lambda eng: eng.comm_init_dir(rank, world, td))
            try:
                results[rank] = _distributed_rank(rank, world, devices[rank], connect, ingroup_files, outgroup_files,
                                                  L, R, amplicon_len, omit_soft)
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e
        threads = [threading.Thread(target=work, args=(r,), name=f"krisp-gpu{devices[r]}") for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    real = [e for e in errors if e is not None and not isinstance(e, PeerFailed)]
    if real or any(errors):
        raise (real or [e for e in errors if e is not None])[0]
    groups, stats = results[0]
    stats["kmers"] = int(sum(r[1]["kmers"] for r in results))
    return groups, stats


# ----------------------------------------------------------------------------
# stage functions (reference signatures)
# ----------------------------------------------------------------------------
def _extract_sorted_wide(fasta_file, L, R, k, output, omit, device, verbose):
    """extractSortedKmers for amplicons longer than one key (krisp_fasta.py:16-66 takes any k):
    the genome alone through kr_wide_run without a filter -- every window then belongs to a
    (left,right) group, the groups come in (left,right) order -- and the members of a group put in
    diag order here; lines 'left,diag,right' as kstream.py:832 writes them."""
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    _check_wide(Le, De, Re)
    bases, rna, special = fasta.ingest(fasta_file, k, omit)
    lut = np.arange(256, dtype=np.uint8)
    if rna:
        lut[ord("T")] = ord("U")
    with _native.Engine(device=device) as eng:
        eng.set_option(_native.OPT_WIDE_ORDERED, 1)       # (the chunks below rely on hits in (left, right) group order)
        eng.set_params_wide(Le, De, Re, omit_soft=omit, max_bases=max(len(bases), 1))
        eng.upload(0, bases)
        nhits = eng.wide_run([0], [True], apply_filter=False)
        hits = eng.wide_fetch(_native.WIDE_HITS) if nhits else np.empty(0, dtype=_native.WIDE_HIT)
    # IUPAC k-mers (kept by the reference, resolved on the host) join by a merge of sorted lines
    sp_lines = sorted(",".join(codec.split_window(w, Le, De, Re)).encode() for w in special)

    def key(ln):
        f = ln.split(b",")
        return (f[0], f[2], f[1])

    def chunks():
        """the hits cut at group boundaries (members of one group are ordered together), each chunk as
        its window matrix in (group, diag) order"""
        pos = 0
        while pos < len(hits):
            b = min(len(hits), pos + (1 << 20))
            while b < len(hits) and hits["cand"][b] == hits["cand"][b - 1]:
                b += 1
            sel = hits[pos:b]
            W = _hit_windows(sel, bases, k)
            rec = np.empty(len(sel), dtype=[("c", ">u4"), ("d", f"S{max(De, 1)}")])
            rec["c"] = sel["cand"]
            rec["d"] = W[:, Le:Le + De].copy().view(f"S{De}").ravel() if De else b""
            yield W[np.argsort(rec, order=["c", "d"], kind="stable")]
            pos = b

    n = 0
    with open(output, "wb") as f:
        if not sp_lines:
            for W in chunks():
                W = lut[W]
                out = np.empty((len(W), k + 3), dtype=np.uint8)
                out[:, :Le] = W[:, :Le]
                out[:, Le] = ord(",")
                out[:, Le + 1:Le + 1 + De] = W[:, Le:Le + De]
                out[:, Le + 1 + De] = ord(",")
                out[:, Le + 2 + De:k + 2] = W[:, Le + De:]
                out[:, k + 2] = ord("\n")
                f.write(out.tobytes())
                n += len(out)
        else:
            import heapq
            dev = []
            for W in chunks():
                for row in W:
                    s = bytes(row)
                    dev.append(s[:Le] + b"," + s[Le:Le + De] + b"," + s[Le + De:])
            tr = bytes.maketrans(b"T", b"U") if rna else None
            for ln in heapq.merge(dev, sp_lines, key=key):
                f.write((ln.translate(tr) if tr else ln) + b"\n")
                n += 1
    return n


def extractSortedKmers(fasta_file, primer_left, primer_right, ampl_len, output,
                       sortmem, parallel=1, verbose=True, omit=True, device=0):
    """Fasta file -> sorted 'left,diag,right' k-mer file (krisp_fasta.py:16-66)."""
    kw = dict(kmers=ampl_len, disallow="Nn", complements=True,
              split=[primer_left, -primer_right], sort=True, sortmem=sortmem,
              sortcols=[0, 2], sortnp=parallel, parallel=parallel, device=device)
    kw["omitsoft" if omit else "mapsoft"] = True
    ks = kstream(fasta_file, **kw)
    t0 = time.time()
    if verbose:
        print(f"Extracting {ampl_len}-mers from {fasta_file} and saving to {output}", file=sys.stderr)
    if ks.device_geometry() is not None:
        found = ks.write(output)
    else:
        # amplicons longer than one key: the wide path (raises UnsupportedGeometry beyond it)
        found = _extract_sorted_wide(fasta_file, primer_left, primer_right, ampl_len, output, omit, device, verbose)
    if verbose:
        print(f"=> Extracted and sorted {found:,} {ampl_len}-kmers from {fasta_file} in "
              f"{prettyTime(time.time() - t0)}", file=sys.stderr)


def sortedKmersSerial(files, outputs, ampl_len, primer_left, primer_right, verbose=True,
                      omit=True, device=0):
    for f, o in zip(files, outputs):
        extractSortedKmers(f, primer_left, primer_right, ampl_len, o, "80%", 1, verbose, omit, device)


def sortedKmersParallel(files, outputs, ampl_len, primer_left, primer_right, parallel=1,
                        verbose=True, omit=True, device=0):
    """krisp_fasta.py:86-123.  One GPU sorts a genome in milliseconds; the reference's
    process-per-genome fan-out has nothing left to hide, so this is the serial loop."""
    sortedKmersSerial(files, outputs, ampl_len, primer_left, primer_right, verbose, omit, device)


def _read_lines(path):
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def mergeFiles(files, output, parallel=1, workdir=None, verbose=True, device=0):
    """Sorted 3-column k-mer files -> merged alignment file
    (intersectAmplicons.py:232-310): every (left,right) pair present in ALL files,
    one line 'left,diag,right,labels' per distinct sequence.  The keys of each file
    are packed on the host and adopted by the device as a sorted genome
    (kr_genome_load_sorted); the intersection and the collect run there."""
    files = list(files)
    t0 = time.time()
    if len(files) == 1:
        os.replace(files[0], output)              # shutil.move(files[0], output)
        return
    contents = [_read_lines(f) for f in files]
    geo = None
    for lines in contents:
        if lines:
            f3 = lines[0].split(b",")
            if len(f3) != 3:
                raise ValueError("mergeFiles on the device takes the 3-column sorted k-mer files "
                                 "extractSortedKmers writes")
            geo = (len(f3[0]), len(f3[1]), len(f3[2]))
            break
    if geo is None:
        open(output, "w").close()
        return
    L, D, R = geo
    labels = [simplename(f) for f in files]
    if _is_wide(L, D, R):
        groups = _merge_files_wide(contents, labels, L, D, R, device)
        with open(output, "w") as f:
            for ln in amplicon.merged_lines(groups):
                f.write(ln + "\n")
        if verbose:
            print(f"=> Merged {len(files)} files -> {output} in {prettyTime(time.time() - t0)}", file=sys.stderr)
        return
    _check_geometry(L, D, R)
    keysets, specials = [], []
    for lines in contents:
        flat = b"".join(lines)
        if flat.translate(None, b"ACGT,"):       # some line holds an IUPAC letter: split them off
            sp = [ln for ln in lines if ln.translate(None, b"ACGT,")]
            lines = [ln for ln in lines if not ln.translate(None, b"ACGT,")]
            specials.append([tuple(x.decode() for x in ln.split(b",")) for ln in sp])
        else:
            specials.append([])
        keys = codec.lines_to_keys(lines, L, D, R)
        if len(keys) > 1 and not np.all(keys[1:] >= keys[:-1]):
            raise ValueError("k-mer file is not sorted by (left, right, diag)")
        keysets.append(keys)
    with _native.Engine(device=device) as eng:
        eng.set_params(L, D, R, max_bases=max(1, max(len(k) for k in keysets)))
        for i, keys in enumerate(keysets):
            eng.load_sorted(i, keys)
        ids = list(range(len(files)))
        ncand = eng.intersect(ids, [True] * len(ids), apply_filter=False)
        by_label = sorted(ids, key=lambda i: labels[i])
        records = eng.collect(by_label) if ncand else np.empty(0, dtype=_native.RECORD)
        touched, sgroups = set(), []
        if any(specials):
            touched, sgroups = _special_groups(eng, ids, labels, specials, (L, D, R), frozenset(), False)
    groups = amplicon.groups_from_records(records, labels, L, D, R)
    if touched:
        groups = _merge_groups(groups, touched, sgroups)
    with open(output, "w") as f:
        for ln in amplicon.merged_lines(groups):
            f.write(ln + "\n")
    if verbose:
        print(f"=> Merged {len(files)} files -> {output} in {prettyTime(time.time() - t0)}", file=sys.stderr)


def _merge_files_wide(contents, labels, L, D, R, device):
    """mergeFiles for k-mer files of amplicons longer than one key: every file becomes a "genome"
    whose records are its lines (one window each, forward strand only: the file already holds both
    strands), kr_wide_run finds the (left,right) pairs present in all files and where their members lie."""
    _check_wide(L, D, R)
    k = L + D + R
    texts, rnas, specials = [], [], []
    for lines in contents:
        flat = b"".join(lines)
        rna = b"U" in flat and b"T" not in flat
        rnas.append(rna)
        plain = b"ACGU," if rna else b"ACGT,"
        if flat.translate(None, plain):
            # lines that hold IUPAC ambiguity letters (the reference keeps such k-mers: kstream.py:11-18, Amplicon.py:298-348
            # reads them like any line): they stay text -- the groups they touch are rebuilt on the host from them and from
            # the plain members the device finds for their (left,right) pairs, as find_regions does (round 6: refused before)
            sp = [ln for ln in lines if ln.translate(None, plain)]
            lines = [ln for ln in lines if not ln.translate(None, plain)]
            # (inside, an RNA file's lines are handled with T like its plain lines; they get their U back at the end)
            specials.append([tuple(x.decode().replace("U", "T") if rna else x.decode() for x in ln.split(b",")) for ln in sp])
        else:
            specials.append([])
        rec = [ln.replace(b",", b"") for ln in lines]
        if any(len(r) != k for r in rec):
            raise ValueError("k-mer file with lines of different lengths")
        t = b"\n".join(rec)
        texts.append(np.frombuffer(t.replace(b"U", b"T") if rna else t, dtype=np.uint8))
    ids = list(range(len(texts)))
    mixed = _mixed(rnas)
    touched, probes, probe_text = _touched_pairs(specials, D)
    with _native.Engine(device=device) as eng:
        eng.set_params_wide(L, D, R, omit_soft=False, max_bases=max(1, max(len(t) for t in texts), len(probe_text)))
        eng.set_strands(_native.STRANDS_FORWARD)
        for i, t in enumerate(texts):
            eng.upload(i, t)
        nhits = eng.wide_run(ids, [True] * len(ids), apply_filter=False)
        hits = eng.wide_fetch(_native.WIDE_HITS) if nhits else np.empty(0, dtype=_native.WIDE_HIT)
        # (an RNA genome's file holds U: its lines come back with U; a (left,right) pair that holds T / U is text no DNA file
        # and RNA file share -- shared.py:321-347 merges on the strings)
        groups = _groups_from_hits(hits, texts, labels, L, D, R, rna_genomes=rnas if any(rnas) else None)
        if mixed:
            groups = [g for g in groups if not (set(g[0].left + g[0].right) & set("TU"))]
        if touched:
            sgroups = _special_groups_wide(eng, texts, labels, specials, touched, probes, probe_text, (L, D, R), frozenset(), False,
                                           rna_genomes=rnas if any(rnas) else None)
            if any(rnas):       # (the device's groups of the touched pairs carry U where their files do)
                touched = touched | {(l.replace("T", "U"), r.replace("T", "U")) for l, r in touched}
            groups = _merge_groups(groups, touched, sgroups)
    return groups


def _parse_merged(path):
    """merged-file lines -> groups of amplicon.Amplicon (Amplicon.py:298-328,
    shared.py:350-398, 442-475)."""
    tag = simplename(path)
    groups = []
    for raw in _read_lines(path):
        f = raw.decode().strip().split(",")
        if len(f) not in (3, 4):
            raise ValueError(f"Unrecognised string format : {raw.decode()}")
        labels = [tag]
        if len(f) == 4:
            labels = []
            for item in f[3].split(";"):
                item = item.strip()
                if "(" in item:
                    name, mult = item.split("(")
                    labels += [name] * int(mult.strip(")"))
                else:
                    labels.append(item)
        amp = amplicon.Amplicon(f[0], f[1], f[2], labels)
        if groups and (groups[-1][0].left, groups[-1][0].right) == (amp.left, amp.right):
            for a in groups[-1]:
                if a.sequence == amp.sequence:
                    a.labels = sorted(a.labels + amp.labels)
                    break
            else:
                groups[-1].append(amp)
        else:
            groups.append([amp])
    return groups


_BASE_BIT = {"A": 0, "C": 1, "G": 2, "T": 3}


def filterAlignments(kmerfile, output, ingroup, device=0):
    """filterAlignments.py:31-40: keep the groups that have a diagnostic column whose
    ingroup and outgroup base sets are disjoint (Amplicon.py:495-521).  The host only
    re-encodes the text (one (in, out) base-set mask pair per group, include/krisp_hip.h
    kr_cand); the predicate itself is evaluated on the device (kr_cands_merge)."""
    groups = _parse_merged(kmerfile)
    ingroup = frozenset(ingroup)
    keep = list(range(len(groups)))
    if len(ingroup) and groups:
        D = len(groups[0][0].diag)
        if D == 0:
            keep = []                               # diagnosticLength() == 0: no column can pass
        else:
            # the device's mask pair carries 16 columns: a group passes when ANY column separates the
            # groups, so longer diagnostic regions are filtered 16 columns at a time and the kept sets united
            host_keep, pure = [], []
            for gi, g in enumerate(groups):
                if not all(_pure(a.diag) for a in g):
                    # IUPAC letters in a diagnostic column: base sets are sets of letters
                    # (Amplicon.py:514-520); rare, evaluated here
                    if amplicon.ingroup_unique_columns(g, ingroup):
                        host_keep.append(gi)
                else:
                    pure.append(gi)
            kept = set()
            with _native.Engine(device=device) as eng:
                for c0 in range(0, D, 16):
                    Dc = min(16, D - c0)
                    rows = []
                    for gi in pure:
                        if gi in kept:
                            continue
                        im = om = 0
                        for a in groups[gi]:
                            m = 0
                            for c, ch in enumerate(a.diag[c0:c0 + Dc]):
                                m |= 1 << (4 * c + _BASE_BIT[ch])
                            for lab in set(a.labels):
                                if lab in ingroup:
                                    im |= m
                                else:
                                    om |= m
                        rows.append((gi, im, om))           # prefix = group index: sorted, unique
                    if not rows:
                        break
                    eng.set_params(1, Dc, 0, max_bases=64)
                    eng.load_cands(np.array(rows, dtype=_native.CAND))
                    eng.merge_cands(None, apply_filter=True)
                    kept.update(int(p) for p in eng.cands()["prefix"])
            keep = sorted(kept)
            keep = sorted(keep + host_keep)
    with open(output, "w") as f:
        for gi in keep:
            for a in groups[gi]:
                f.write(a.line() + "\n")


# ----------------------------------------------------------------------------
# command line (krisp_fasta.py:126-298)
# ----------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(description="Find diagnostic alignments for a set of fasta files",
                                prog="krisp", formatter_class=argparse.RawTextHelpFormatter,
                                epilog="Limits of the GPU path, none of which the reference has (it works on text of any length;\n"
                                       "kstream.py:617-642) -- each is refused with a message, never answered wrongly:\n"
                                       "  * a sequence file of 2^33 bases or more (8.6 Gbp: the sorted k-mers of one such genome are what one GPU's\n"
                                       "    memory holds at all); with amplicons longer than 32 bases, 2^32 bases;\n"
                                       "  * amplicons longer than 32 bases (or more than 16 diagnostic bases): conserved flanks of 1 .. 256\n"
                                       "    bases each, amplicons of at most 1024;\n"
                                       "  * DNA and RNA genomes in one run together with IUPAC ambiguity letters over several ranks.\n"
                                       "A genome set that does not fit the GPU's memory sorted at once goes through it in batches\n"
                                       "(same result; KRISP_STREAM_BATCH=n forces batches of n genomes).")
    p.add_argument("files", nargs="+", type=str, metavar="PATH", help="Fasta file to read. .gz, .bz2")
    p.add_argument("--outgroup", nargs="*", type=str, default=[], metavar="PATH",
                   help="Outgroup Fasta files. To be amplified, but not detected")
    p.add_argument("-c", "--conserved", type=int, metavar="INT",
                   help="Length of conserved regions on ends of amplicon")
    p.add_argument("--conserved-left", type=int, metavar="INT",
                   help="Length of conserved region on left of amplicon")
    p.add_argument("--conserved-right", type=int, metavar="INT",
                   help="Length of conserved region on right of amplicon")
    p.add_argument("-d", "--diagnostic", type=int, metavar="INT", help="Diagnostic region length for amplicon")
    p.add_argument("-a", "--amplicon", type=int, metavar="INT", help="Total amplicon length")
    p.add_argument("--omit-soft", action="store_true", help="Omit softmasked nucleotides")
    p.add_argument("--cores", type=int, default=1, metavar="INT",
                   help="Total number of processors to utilize. (default: %(default)s)")
    p.add_argument("--dot-alignment", action="store_true", help="Output as dot-based alignments")
    p.add_argument("-o", "--out_align", type=str, metavar="PATH",
                   help="Write results as human-readable alignments to a file. (default: do not write alignment output)")
    p.add_argument("-s", "--out_csv", type=str, metavar="PATH",
                   help="Write results to as a CSV (comma-separated value) file. (default: print to screen (stdout))")
    p.add_argument("--out_locations", type=str, metavar="PATH",
                   help="Also write where every diagnostic region lies in every genome, as a tab-separated file:\n"
                        "region, file, record, record_index, start, end (0-based, half-open), strand, sequence.\n"
                        "A separate pass that reads every input again (and inflates again a file the GPU inflated);\n"
                        "not with --primer3. (default: no locations, no extra pass)")
    p.add_argument("--out_near", type=str, metavar="PATH",
                   help="Also write every window of every genome within --near-mismatches substitutions of an ingroup window\n"
                        "of a diagnostic region (both strands, wherever it lies), as a tab-separated file: region, target, file,\n"
                        "record, record_index, start, end, strand, mismatches, flank_mismatches, sequence.  A separate pass that\n"
                        "reads every input again; amplicons of at most 32 bases; not with --primer3.\n"
                        "(default: no near matches, no extra pass)")
    p.add_argument("--near-mismatches", type=int, default=None, metavar="INT",
                   help="Hamming distance of --out_near: 0 .. 3, smaller than the amplicon length (default: 1)")
    p.add_argument("--out_products", type=str, metavar="PATH",
                   help="Also write the predicted PCR products of every region's conserved flanks in every genome: a window\n"
                        "within --primer-mismatches substitutions of the left flank and one of the right flank on one record,\n"
                        "facing each other, at most --max-product bases from end to end (either strand), as a tab-separated\n"
                        "file: region, file, record, record_index, start, end, strand, length, left_mismatches,\n"
                        "right_mismatches, left_end_mismatches, right_end_mismatches (those in the five 3' bases).  A separate\n"
                        "pass that reads every input again; flanks of at least 10 bases; not with --primer3.\n"
                        "(default: no products, no extra pass)")
    p.add_argument("--out_primer_products", type=str, metavar="PATH",
                   help="With --design-primers: also write the predicted PCR products of the designed primer pairs in every\n"
                        "genome, the outgroups included: a window within --primer-mismatches substitutions of the left primer\n"
                        "and one of the right primer on one record, facing each other, at most --max-product bases from end to\n"
                        "end (either strand), as a tab-separated file with the columns of --out_products; region = the pair's\n"
                        "data row in the CSV, the end mismatches are those in the primer's own five 3' bases.  A separate pass\n"
                        "that reads every input again.  (default: no products, no extra pass)")
    p.add_argument("--primer-mismatches", type=int, default=None, metavar="INT",
                   help="substitutions allowed in each flank of --out_products, in each primer of --out_primer_products:\n"
                        "0 .. 3 (default: 1)")
    p.add_argument("--max-product", type=int, default=None, metavar="INT",
                   help="longest product of --out_products / --out_primer_products in bases, at least the two flanks together /\n"
                        "the upper bound of --amp_size (default: 1000)")
    p.add_argument("--primer-candidates", type=int, default=None, metavar="INT",
                   help="--design-primers picks a region's pair among its INT best passing pairs (1 .. 8, by penalty, then\n"
                        "position) by what they amplify: every shortlisted pair is searched in every input genome, ingroup and\n"
                        "outgroup, as --out_primer_products searches (--primer-mismatches, --max-product, --omit-soft), and the\n"
                        "pair with the fewest products without a mismatch in either primer's five 3' bases wins, then the fewest\n"
                        "with 0 mismatches in all, with 1, and so on; ties go to the better pair.  The picked pair takes the\n"
                        "place of the best one in the CSV and in every output that reads the pairs.  One more pass over the\n"
                        "inputs; not with --primer3.  (default: the best pair, no search)")
    p.add_argument("--out_primer_candidates", type=str, metavar="PATH",
                   help="With --primer-candidates: also write every searched pair of every region as a tab-separated file:\n"
                        "region, rank, shortlisted, pair_penalty, product_size, left_sequence, right_sequence, left_start,\n"
                        "left_length, right_start, right_length, products (the counts clean,t0,t1,...: clean 3' ends, then by the\n"
                        "two primers' mismatches together), picked (0/1), by region and rank")
    p.add_argument("--out_guides", type=str, metavar="PATH",
                   help="Also write a CRISPR guide for every region that can carry one, as a tab-separated file: region, strand,\n"
                        "start, end (template columns, 0-based, half-open), pam5, pam3, protospacer (as read 5'->3' on the guide's\n"
                        "strand), gc_percent, min_mismatches, sum_mismatches, candidates.  The guide is the window of --guide-size\n"
                        "columns of the ingroup's consensus, next to --pam5 / --pam3, within --guide-gc and without a run of five\n"
                        "equal bases, that differs most from the region's outgroup sequences; with --design-primers it lies\n"
                        "between the designed primers and region = the pair's data row in the CSV.  No extra pass over the\n"
                        "inputs; not with --primer3.  (default: no guides)")
    p.add_argument("--guide-size", type=int, default=None, metavar="INT",
                   help="protospacer length of --out_guides: 12 .. 40, at most the amplicon length (default: 28)")
    p.add_argument("--pam5", type=str, default=None, metavar="MOTIF",
                   help="motif 5' of the protospacer in IUPAC letters, at most 8, e.g. TTTV for Cas12a (default: none)")
    p.add_argument("--pam3", type=str, default=None, metavar="MOTIF",
                   help="motif 3' of the protospacer in IUPAC letters, at most 8, e.g. H for LwaCas13a's PFS (default: none)")
    p.add_argument("--guide-gc", type=int, nargs=2, default=None, metavar="INT",
                   help="GC percent of the protospacer, lower and upper bound (default: 30 70)")
    p.add_argument("--guide-min-mismatches", type=int, default=None, metavar="INT",
                   help="columns in which the protospacer differs from EVERY outgroup sequence of its region at least:\n"
                        "0 .. --guide-size (default: 1)")
    p.add_argument("--guide-candidates", type=int, default=None, metavar="INT",
                   help="--out_guides picks a region's guide among its INT best candidates (1 .. 8, in the order above) by their\n"
                        "off-targets: every candidate's protospacer is searched in every --outgroup genome, on both strands,\n"
                        "within --guide-hit-mismatches substitutions (--guide-hits-need-pam applies), and the candidate with the\n"
                        "fewest exact hits wins, then the fewest with 1 mismatch, and so on; ties go to the better candidate.  Every\n"
                        "row gains the columns rank, shortlisted and outgroup_hits (the hits with 0, 1, ... mismatches).  Needs an\n"
                        "--outgroup file; one more pass over the outgroup files.  (default: the best candidate, no search)")
    p.add_argument("--out_guide_candidates", type=str, metavar="PATH",
                   help="With --guide-candidates: also write every searched candidate of every region, as --out_guides writes the\n"
                        "picked one, with the column picked (0/1), by region and rank")
    p.add_argument("--out_guide_hits", type=str, metavar="PATH",
                   help="Also search every genome for the guides --out_guides picked, and write every window within\n"
                        "--guide-hit-mismatches substitutions of a protospacer, on both strands, as a tab-separated file: region,\n"
                        "file, record, record_index, start, end, strand, mismatches, mismatch_columns (1-based, 5'->3' on the\n"
                        "guide), pam5_match, pam3_match (1: --pam5 / --pam3 lies beside the window), sequence.  A guide's own\n"
                        "locus in its ingroup genomes is a row with 0 mismatches.  One more pass over the inputs; needs\n"
                        "--out_guides.  (default: no search)")
    p.add_argument("--guide-hit-mismatches", type=int, default=None, metavar="INT",
                   help="Hamming distance of --out_guide_hits: 0 .. 3 (default: 2)")
    p.add_argument("--guide-hit-bulges", type=int, default=None, metavar="INT",
                   help="--out_guide_hits also lists the windows that match a protospacer once one bulge of up to INT bases is\n"
                        "allowed for: a DNA bulge (bases of the genome without a partner in the guide) or an RNA bulge (guide\n"
                        "letters without a partner), 0 .. 2.  The file gains the columns bulge (-, DNA, RNA), bulge_size and\n"
                        "bulge_column (the 1-based guide column after which the bulge lies).  Needs --guide-size >= 20 and\n"
                        "--guide-hit-mismatches <= 2; one more pass over the inputs.  (default: 0, no bulges)")
    p.add_argument("--guide-hits-need-pam", action="store_true",
                   help="--out_guide_hits lists a window only where --pam5 and --pam3 lie beside it (needs one of the two)")
    p.add_argument("--out_assay_hits", type=str, metavar="PATH",
                   help="With --design-primers and --out_guides: also write where a region's assay would give a signal, in every\n"
                        "genome, the outgroups included: every product of the region's primer pair (as --out_primer_products\n"
                        "lists them: --primer-mismatches, --max-product) that carries a window within --guide-hit-mismatches\n"
                        "substitutions of the region's protospacer (as --out_guide_hits lists them: --guide-hits-need-pam)\n"
                        "wholly between its two primer sites.  A tab-separated file: region, file, record, record_index,\n"
                        "product_start, product_end, product_strand, length, the four primer mismatch columns, guide_start,\n"
                        "guide_end, guide_strand, guide_mismatches, mismatch_columns, pam5_match, pam3_match, orientation (design:\n"
                        "the guide lies on the strand of the product the design put it on; reverse otherwise), sequence.  The\n"
                        "designed locus of an ingroup genome is a row without mismatches; the rows to look at are the others.\n"
                        "Both searches and their join run on the device over one read of every input.  Bulged hits\n"
                        "(--guide-hit-bulges) take no part: the unbulged hits alone are joined.  (default: no join)")
    p.add_argument("--panel", type=int, default=None, metavar="INT",
                   help="With --design-primers and --out_panel: pick INT (1 .. 64) of the designed assays that can share a tube.\n"
                        "The regions with a pair (with --out_guides: and a guide) go by ascending pair_penalty (with\n"
                        "--out_guides: the greater min_mismatches first), then region; the first is a member, and after every\n"
                        "member a later candidate is dropped when it is the same locus (its template shares 16 bases with the\n"
                        "member's, on either strand) or clashes (a duplex figure of one of its primers with one of the member's\n"
                        "lies above --max_sec_tm); the next member is the first still alive.  The selection runs on the device;\n"
                        "no pass over the inputs.  (default: no panel)")
    p.add_argument("--out_panel", type=str, metavar="PATH",
                   help="The file of --panel, tab-separated, a row per member in order of acceptance: member, region (the pair's\n"
                        "data row in the CSV), pair_penalty, product_size, left_sequence, right_sequence, cross_any, cross_end (the\n"
                        "greatest duplex figures of its primers with the primers of the members before it), dropped_same_locus,\n"
                        "dropped_clash (the candidates this member dropped, by cause)")
    p.add_argument("--panel-clean", action="store_true",
                   help="With --panel: keep cross and single products out of the panel.  One pass over the inputs keeps the\n"
                        "sites of every candidate's primers on the device (--primer-mismatches, --max-product and --omit-soft as\n"
                        "--out_panel_products reads them); a candidate one of whose primers forms a product with itself is never\n"
                        "a member, and after every member a later candidate is also dropped when one of its primers forms a\n"
                        "product with one of the member's, in either order, in any genome, the outgroups included.  With the\n"
                        "same three figures --out_panel_products then holds pair rows only.  --out_panel gains the column\n"
                        "dropped_cross.  (default: the panel is picked without a look at the genomes)")
    p.add_argument("--out_panel_products", type=str, metavar="PATH",
                   help="With --panel: multiplex in-silico PCR.  With all the panel's primers in one tube, every product they\n"
                        "amplify in every genome, the outgroups included: any primer may open a product and any primer may close\n"
                        "one (--primer-mismatches, --max-product and --omit-soft as --out_primer_products reads them).  A\n"
                        "tab-separated file, a row per product: file, record, record_index, start, end, length, forward, reverse\n"
                        "(the primers' names: 1L and 1R are member 1's), kind (pair: the two primers of one member; single: one\n"
                        "primer with itself; cross: everything else), forward_mismatches, reverse_mismatches,\n"
                        "forward_end_mismatches, reverse_end_mismatches.  One more pass over the inputs.  (default: no search)")
    p.add_argument("--out_panel_summary", type=str, metavar="PATH",
                   help="With --panel: the products of --out_panel_products counted on the device, a row per file and ordered\n"
                        "primer pair with at least one: file, forward, reverse, kind, products, clean_end_products (those without\n"
                        "a mismatch in the five 3' bases of either primer).  Alone it brings no product to the host.")
    p.add_argument("-w", "--workdir", type=str, metavar="PATH", help="Work directory to place temporary files")
    p.add_argument("-p", "--primer3", action=argparse.BooleanOptionalAction,
                   help="Design primers with Primer3 for every region found (needs the primer3-py package)")
    p.add_argument("--design-primers", action="store_true",
                   help="Design a primer pair for every region found on the GPU, with the options below (no third-party\n"
                        "package): an integer nearest-neighbour model, ungapped duplex figures in the place of Primer3's\n"
                        "thermodynamic alignments, hairpins with --hairpins. Regions without a pair are left out; --primer_size within\n"
                        "10 .. 60; not with --primer3, --out_locations, --out_near or --out_products (the designed pairs are\n"
                        "searched by --out_primer_products).")
    p.add_argument("--hairpins", action="store_true",
                   help="With --design-primers: hold every primer to --max_sec_tm for hairpins too (the highest melting\n"
                        "temperature of a stem of two or more pairs around a loop of three or more bases, the project's own\n"
                        "integer model) and append left_hairpin and right_hairpin to the CSV. (default: hairpins are not looked at)")
    p.add_argument("--tm", type=int, nargs=2, metavar="INT", default=[53, 68])
    p.add_argument("--gc", type=int, nargs=2, metavar="INT", default=[40, 70])
    p.add_argument("--amp_size", type=int, nargs=2, metavar="INT", default=[70, 150])
    p.add_argument("--primer_size", type=int, nargs=2, metavar="INT", default=[25, 35])
    p.add_argument("--max_sec_tm", type=int, default=40, metavar="INT")
    p.add_argument("--gc_clamp", type=int, default=1, metavar="INT")
    p.add_argument("--max_end_gc", type=int, default=4, metavar="INT")
    p.add_argument("--verbose", action="store_true", help="Print runtime information to sys.stderr")
    p.add_argument("--device", type=int, default=0, metavar="INT", help="GPU to run on (default: 0)")
    p.add_argument("--devices", type=str, default=None, metavar="LIST",
                   help="several GPUs from ONE process, e.g. 0,1,2,3: genomes sharded over them, candidate lists "
                        "tree-reduced over RCCL (or start one process per GPU with torch.distributed.run / mpirun)")
    return p


def deduce_geometry(args, parser):
    """krisp_fasta.py:179-213, same precedence; exits 1 with the same message."""
    def fail():
        print("ERROR: Could not deduce input parameters", file=sys.stderr)
        parser.print_help(sys.stderr)
        sys.exit(1)

    if args.amplicon is not None:
        if args.diagnostic is not None:
            args.conserved = (args.amplicon - args.diagnostic) // 2
            args.conserved_left = args.conserved_right = args.conserved
        elif args.conserved is not None:
            args.diagnostic = args.amplicon - 2 * args.conserved
            args.conserved_left = args.conserved_right = args.conserved
        elif args.conserved_left is not None and args.conserved_right is not None:
            args.diagnostic = args.amplicon - args.conserved_left - args.conserved_right
        else:
            fail()
    elif args.diagnostic is not None:
        if args.conserved is not None:
            args.amplicon = args.diagnostic + 2 * args.conserved
            args.conserved_left = args.conserved_right = args.conserved
        elif args.conserved_left is not None and args.conserved_right is not None:
            args.amplicon = args.diagnostic + args.conserved_left + args.conserved_right
        else:
            fail()
    else:
        fail()
    return args


# what an option is when the command line does not give it -- filled in only where an output asks for it
_DEFAULTS = {"near_mismatches": 1, "primer_mismatches": 1, "max_product": 1000, "guide_size": 28, "guide_gc": [30, 70],
             "guide_min_mismatches": 1, "guide_hit_mismatches": 2, "guide_hit_bulges": 0}
_PRODUCT_OUTPUTS = ("--out_products", "--out_primer_products", "--out_assay_hits")
_GUIDE_HIT_OUTPUTS = ("--out_guide_hits", "--out_assay_hits")
# an option that only means something with one of these outputs, by the step of _check_options that looks at it
_NEEDS = {
    "near": (("--near-mismatches", ("--out_near",)),),
    "products": (("--primer-mismatches", _PRODUCT_OUTPUTS), ("--max-product", _PRODUCT_OUTPUTS)),
    "guides": tuple((opt, ("--out_guides",)) for opt in ("--guide-size", "--pam5", "--pam3", "--guide-gc", "--guide-min-mismatches")),
    # (the assay join takes the two figures of the guide hits; bulged hits take no part in it)
    "guide_hits": (("--guide-hit-mismatches", _GUIDE_HIT_OUTPUTS), ("--guide-hits-need-pam", _GUIDE_HIT_OUTPUTS),
                   ("--guide-hit-bulges", ("--out_guide_hits",))),
}
# ... or with one of these options, which the refusal does not name: --guide-candidates searches with the guide hits' two figures,
# and the panel's products and --primer-candidates read the product passes' two figures
_PANEL_PRODUCT_OUTPUTS = ("--out_panel_products", "--out_panel_summary")
_ALSO_WITH = {"--guide-hit-mismatches": ("--guide-candidates",), "--guide-hits-need-pam": ("--guide-candidates",),
              "--primer-mismatches": _PANEL_PRODUCT_OUTPUTS + ("--primer-candidates", "--panel-clean"),
              "--max-product": _PANEL_PRODUCT_OUTPUTS + ("--primer-candidates", "--panel-clean")}
_PRIMER_OPTIONS = ("tm", "gc", "amp_size", "primer_size", "max_sec_tm", "gc_clamp", "max_end_gc")


def _refuse(why):
    """the one way an option check ends the run: the reason on one line, exit status 2"""
    print("ERROR: " + why, file=sys.stderr)
    sys.exit(2)


def _check_options(args, parser):
    """Every check of the options against each other and against the geometry, and the defaults (_DEFAULTS) of the options
    that count only with an output, before a file is read.  The reasons are tried in a fixed order and the first one
    refuses (tests/test_cli_refusals.py pins the order).  args: after deduce_geometry; parser: as deduce_geometry takes it."""
    def given(opt):
        v = getattr(args, opt.lstrip("-").replace("-", "_"))
        return v is not None and v is not False

    def needs(step):
        for opt, outputs in _NEEDS[step]:
            if given(opt) and not any(given(out) for out in outputs) and not any(given(o) for o in _ALSO_WITH.get(opt, ())):
                _refuse(f"{opt} needs " + " or ".join(outputs))

    def fill(*names):
        for name in names:
            if getattr(args, name) is None:
                setattr(args, name, _DEFAULTS[name])

    def check(why):
        if why is not None:
            _refuse(why)

    L, R, k = args.conserved_left, args.conserved_right, args.amplicon
    if args.design_primers:
        from . import thermo
        if args.primer3:
            _refuse("--design-primers cannot be combined with --primer3 (one designer at a time)")
        for opt, verb in (("--out_locations", "located"), ("--out_near", "searched"), ("--out_products", "searched")):
            if given(opt):
                _refuse(f"{opt} cannot be combined with --design-primers (the regions the designer keeps are not {verb})")
        check(thermo.refusal(*(getattr(args, name) for name in _PRIMER_OPTIONS)))
    if args.hairpins and not args.design_primers:
        _refuse("--hairpins needs --design-primers (it is the designer's own check; Primer3 has PRIMER_MAX_HAIRPIN_TH)")
    if args.out_locations is not None and args.primer3:
        _refuse("--out_locations cannot be combined with --primer3 (the regions Primer3 keeps are not located)")
    if args.out_near is not None and args.primer3:
        _refuse("--out_near cannot be combined with --primer3 (the regions Primer3 keeps are not searched)")
    needs("near")
    if args.out_near is not None:
        fill("near_mismatches")
        check(near_refusal(L, R, k, args.near_mismatches))
    if args.out_products is not None and args.primer3:
        _refuse("--out_products cannot be combined with --primer3 (the primers Primer3 designs are not searched)")
    if args.out_primer_products is not None and not args.design_primers:
        _refuse("--out_primer_products needs --design-primers")
    needs("products")
    if args.out_primer_products is not None:
        fill("primer_mismatches", "max_product")
        check(primer_products_refusal(args.amp_size, args.primer_mismatches, args.max_product))
    check(primer_candidates_refusal(args.design_primers, args.primer_candidates, args.out_primer_candidates is not None,
                                    bool(args.primer3)))
    if args.primer_candidates is not None:
        fill("primer_mismatches", "max_product")
        check(primer_products_refusal(args.amp_size, args.primer_mismatches, args.max_product))
    if args.out_products is not None:
        fill("primer_mismatches", "max_product")
        check(products_refusal(L, R, k, args.primer_mismatches, args.max_product))
    needs("guides")
    if args.out_guides is not None:
        fill("guide_size", "guide_gc", "guide_min_mismatches")
        args.pam5, args.pam3 = args.pam5 or "", args.pam3 or ""
        if args.primer3:
            _refuse("--out_guides cannot be combined with --primer3 (the regions Primer3 keeps get no guide)")
        check(guides_refusal(k, args.guide_size, args.pam5, args.pam3, args.guide_gc, args.guide_min_mismatches))
    if args.out_guide_hits is not None and args.out_guides is None:
        _refuse("--out_guide_hits needs --out_guides (the guides it searches for)")
    needs("guide_hits")
    if args.out_guide_hits is not None:
        fill("guide_hit_mismatches", "guide_hit_bulges")
        check(guide_hits_refusal(args.guide_size, args.guide_hit_mismatches, args.pam5, args.pam3, args.guide_hits_need_pam,
                                 bulges=args.guide_hit_bulges))
    if args.out_assay_hits is not None:
        fill("primer_mismatches", "max_product", "guide_hit_mismatches")
        check(assay_hits_refusal(args.design_primers, args.out_guides is not None, args.amp_size, args.primer_mismatches,
                                 args.max_product, args.guide_size, args.guide_hit_mismatches, args.pam5, args.pam3,
                                 args.guide_hits_need_pam))
    check(guide_candidates_refusal(args.out_guides is not None, args.guide_candidates, args.outgroup,
                                   args.out_guide_candidates is not None))
    if args.guide_candidates is not None and args.out_guide_hits is None:
        fill("guide_hit_mismatches")
        check(guide_hits_refusal(args.guide_size, args.guide_hit_mismatches, args.pam5, args.pam3, args.guide_hits_need_pam))
    if args.primer3:
        from . import primers
        if not primers.available():
            _refuse("--primer3 needs the primer3-py package, which is not installed here (the k-mer path itself does not use it)")
    check(panel_refusal(args.design_primers, args.panel, args.out_panel is not None, bool(args.primer3)))
    if any(given(out) for out in _PANEL_PRODUCT_OUTPUTS):
        fill("primer_mismatches", "max_product")
        check(panel_products_refusal(args.panel, args.out_panel_products is not None, args.out_panel_summary is not None,
                                     args.amp_size, args.primer_size, args.primer_mismatches, args.max_product))
    if args.panel_clean:
        fill("primer_mismatches", "max_product")
        check(panel_clean_refusal(args.panel, True, args.amp_size, args.primer_size, args.primer_mismatches, args.max_product))
    return args


def _discover(args):
    """the regions, by the route the launch asks for: a thread per listed device, a process per GPU, or one device
    -> (groups, stats, the device the report passes run on); None on a rank that writes no output"""
    devices = [int(x) for x in str(args.devices).split(",")] if getattr(args, "devices", None) else None
    _rank, local_rank, launch_world = distributed.env_rank_world()   # torchrun / mpirun / srun alike (one place decides: distributed.py)
    L, R, k = args.conserved_left, args.conserved_right, args.amplicon
    if devices and len(devices) > 1 and launch_world == 1:
        # one process, a thread per device
        groups, stats = find_regions_multi_device(args.files, args.outgroup, L, R, k, devices, omit_soft=args.omit_soft,
                                                  verbose=args.verbose)
        return groups, stats, devices[0]
    if launch_world > 1:
        # one process per GPU (python -m torch.distributed.run ... -m krisp_amd.krisp_fasta ...)
        transport = os.environ.get("KRISP_COMM_TRANSPORT", "rccl")
        groups, stats = find_regions_distributed(args.files, args.outgroup, L, R, k, omit_soft=args.omit_soft, transport=transport,
                                                 verbose=args.verbose)
        if groups is None:
            return None                  # rank 0 writes the output
        if transport == "dir":
            local_rank %= max(1, int(os.environ.get("KRISP_VISIBLE_GPUS", "1")))
        return groups, stats, local_rank
    groups, stats = find_regions(args.files, args.outgroup, L, R, k, omit_soft=args.omit_soft, device=args.device,
                                 verbose=args.verbose)
    return groups, stats, args.device


def _render(args, groups, ingroup, device):
    """the CSV and the alignments, through the designer the options name -> (csv text, alignment text, the designed pairs'
    records or None, the templates where the guide pass takes them too or None)"""
    records = templates = None
    design = {name: getattr(args, name) for name in _PRIMER_OPTIONS}
    if args.primer3:
        from . import primers
        csv_text, align_text = primers.render(groups, ingroup, primers.settings(**design), dot=args.dot_alignment)
    elif args.design_primers:
        from . import primers
        if args.verbose:
            print("Designing a primer pair for every region ... ", file=sys.stderr)
        # (the templates are built once: the guide pass takes them too)
        shortlisting = args.primer_candidates is not None
        templates = design_templates(groups, ingroup) if args.out_guides is not None or args.panel is not None or shortlisting else None
        if not shortlisting:
            records = design_primers(groups, ingroup, device=device, hairpins=args.hairpins, templates=templates, **design)
        else:
            # (the picked records take the place of design_primers': every consumer below reads the same array)
            M = args.primer_mismatches
            shortlist = design_primer_shortlist(groups, ingroup, device=device, hairpins=args.hairpins, templates=templates,
                                                top=args.primer_candidates, **design)
            left, right, pairs, index = shortlist_pairs(templates[0], shortlist)
            if args.verbose:
                print(f"Searching every genome for {len(pairs):,} candidate primer pairs with up to {M} mismatches each ... ",
                      file=sys.stderr)
            tallies = primer_tallies(left, right, pairs, args.files, args.outgroup, args.conserved_left, args.conserved_right,
                                     args.amplicon, mismatches=M, max_product=args.max_product, omit_soft=args.omit_soft,
                                     device=device)
            records, ranks, _ = pick_pairs(shortlist, index, tallies, M)
            if args.out_primer_candidates is not None:
                write_primer_candidates(args.out_primer_candidates, templates[0], shortlist, index, tallies, ranks, M)
        csv_text, align_text = primers.render_designed(groups, ingroup, records, dot=args.dot_alignment)
    else:
        csv_text, align_text = amplicon.render(groups, ingroup, dot=args.dot_alignment)
    return csv_text, align_text, records, templates


def _run_reports(args, groups, ingroup, device, records, templates):
    """the --out_* passes, each on `device`, one genome at a time, written by rank 0 -- for every group, also those a
    stopped renderer left out of the CSV (amplicon.RendererStopped); with --design-primers for every group with a pair.
    records, templates: _render's"""
    def say(text):
        if args.verbose:
            print(text, file=sys.stderr)

    files = (args.files, args.outgroup)
    geometry = (args.conserved_left, args.conserved_right, args.amplicon)
    where = dict(omit_soft=args.omit_soft, device=device)
    if args.out_locations is not None:
        say("Locating the regions in every genome ... ")
        write_locations(args.out_locations, locate_regions(groups, *files, *geometry, **where))
    if args.out_near is not None:
        say(f"Searching every genome for windows within {args.near_mismatches} mismatches of the ingroup's ... ")
        write_near(args.out_near, near_matches(groups, *files, *geometry, mismatches=args.near_mismatches, **where))
    if args.out_products is not None:
        say(f"Predicting the products of the flanks with up to {args.primer_mismatches} mismatches each ... ")
        write_products(args.out_products, predict_products(groups, *files, *geometry, mismatches=args.primer_mismatches,
                                                           max_product=args.max_product, **where))
    if args.out_primer_products is not None:
        say(f"Predicting the products of the designed primers with up to {args.primer_mismatches} mismatches each ... ")
        write_products(args.out_primer_products,
                       primer_products(groups, records, ingroup, *files, *geometry, mismatches=args.primer_mismatches,
                                       max_product=args.max_product, **where))
    guides = None
    if args.out_guides is not None:
        guides = _run_guide_reports(args, groups, ingroup, device, records, templates, say)
    if args.panel is not None:
        say(f"Picking a panel of {args.panel} assays ... ")
        order = panel_candidates(records, guides)
        design = {name: getattr(args, name) for name in _PRIMER_OPTIONS}
        drops = None
        if args.panel_clean:
            say(f"Searching every genome for the primers of {len(order):,} candidates with up to {args.primer_mismatches} mismatches each ... ")
            members, _fates, drops = select_panel_clean(templates[0], records, order, args.panel, *files, *geometry,
                                                        mismatches=args.primer_mismatches, max_product=args.max_product, **where,
                                                        **design)
            print(f"--panel-clean: {int(drops[0])} of {len(order)} candidates prime with themselves and are left out",
                  file=sys.stderr)
        else:
            members, _fates = select_panel(templates[0], records, order, args.panel, device=device, **design)
        write_panel(args.out_panel, templates[0], records, order, members, drops)
        if args.out_panel_products is not None or args.out_panel_summary is not None:
            say(f"Predicting what the panel's primers amplify together, with up to {args.primer_mismatches} mismatches each ... ")
            rows, summary = panel_products(panel_oligos(templates[0], records, order, members), *files, *geometry,
                                           mismatches=args.primer_mismatches, max_product=args.max_product,
                                           rows=args.out_panel_products is not None, **where)
            if args.out_panel_products is not None:
                write_panel_products(args.out_panel_products, rows)
            if args.out_panel_summary is not None:
                write_panel_summary(args.out_panel_summary, summary)


def _run_guide_reports(args, groups, ingroup, device, records, templates, say):
    """_run_reports' passes of --out_guides: the guides, their hits, the assay hits -> the guides' records"""
    files = (args.files, args.outgroup)
    where = dict(omit_soft=args.omit_soft, device=device)
    say("Picking a guide for every region ... ")
    bounds = regions = None
    if args.design_primers:
        found = records["found"] != 0
        lo = records["left_start"].astype(np.int64) + records["left_len"]
        # (a region without a pair gets the empty bounds [0, 0): it takes no part)
        bounds = np.where(found[:, None], np.stack([lo, records["right_start"].astype(np.int64)], axis=1), 0).astype(np.uint32)
        regions = np.cumsum(found) - 1
    else:
        templates = design_templates(groups, ingroup)
    options = (args.guide_size, args.pam5, args.pam3, tuple(args.guide_gc), args.guide_min_mismatches)
    lengths = dict(pam5_len=len(args.pam5), pam3_len=len(args.pam3), regions=regions)
    motifs = dict(pam5=args.pam5, pam3=args.pam3, need_pam=args.guide_hits_need_pam)
    if args.guide_candidates is None:
        guides = design_guides(groups, ingroup, *options, bounds=bounds, device=device, templates=templates)
        write_guides(args.out_guides, templates[0], guides, args.guide_size, **lengths)
    else:
        M = args.guide_hit_mismatches
        shortlist = design_guide_shortlist(groups, ingroup, *options, bounds=bounds, device=device, templates=templates,
                                           top=args.guide_candidates)
        texts, index = shortlist_texts(templates[0], shortlist, args.guide_size)
        say(f"Searching the outgroup genomes for {len(texts):,} candidate guides with up to {M} mismatches ... ")
        tallies = guide_tallies(texts, args.outgroup, args.guide_size, mismatches=M, **motifs, **where)
        guides, ranks, picked = pick_guides(shortlist, index, tallies, M)
        write_guides(args.out_guides, templates[0], guides, args.guide_size, **lengths, ranks=ranks,
                     shortlisted=(index >= 0).sum(axis=1), outgroup_hits=picked[:, :M + 1])
        if args.out_guide_candidates is not None:
            write_guide_candidates(args.out_guide_candidates, templates[0], shortlist, index, tallies, ranks, args.guide_size, M,
                                   **lengths)
    if args.out_guide_hits is not None:
        say(f"Searching every genome for the guides with up to {args.guide_hit_mismatches} mismatches ... ")
        texts, text_regions = guide_texts(templates[0], guides, args.guide_size, regions=regions)
        how = dict(mismatches=args.guide_hit_mismatches, **motifs, **where)
        rows = guide_hits(texts, text_regions, *files, args.guide_size, **how)
        if not args.guide_hit_bulges:
            write_guide_hits(args.out_guide_hits, rows)
        else:
            say(f"... and once more with bulges of up to {args.guide_hit_bulges} ... ")
            bulged = guide_bulge_hits(texts, text_regions, *files, args.guide_size, bulges=args.guide_hit_bulges, **how)
            write_guide_bulge_hits(args.out_guide_hits, rows, bulged, list(args.files) + list(args.outgroup))
    if args.out_assay_hits is not None:
        # (both scans and their join over one read of each file)
        say("Searching every genome for the guides' hits inside the designed primers' products ... ")
        left, right, pairs, pairs_regions = primer_pairs(templates[0], records)
        texts, text_regions = guide_texts(templates[0], guides, args.guide_size, regions=regions)
        # the guide strand of every region with a pair and a guide, under the region's number in both files
        region_strand = np.full(int(found.sum()), -1, dtype=np.int64)
        picked = found & (guides["found"] != 0)
        region_strand[regions[picked]] = guides["strand"][picked]
        write_assay_hits(args.out_assay_hits,
                         assay_hits(left, right, pairs, pairs_regions, texts, text_regions, region_strand, *files, args.guide_size,
                                    primer_mismatches=args.primer_mismatches, max_product=args.max_product,
                                    guide_mismatches=args.guide_hit_mismatches, **motifs, **where))
    return guides


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    args = _check_options(deduce_geometry(args, parser), parser)
    t0 = time.time()
    if args.verbose:
        print("Finding kmer-based diagnostic regions for:", file=sys.stderr)
        for i, f in enumerate(args.files):
            print(f"({i}) {f}", file=sys.stderr)
        print("With this as an outgroup:", file=sys.stderr)
        for i, f in enumerate(args.outgroup):
            print(f"({i}) {f}", file=sys.stderr)
        print(file=sys.stderr)
    found = _discover(args)
    if found is None:
        return 0
    groups, stats, device = found
    if args.verbose:
        print("\nRendering output ... ", file=sys.stderr)
    ingroup = [simplename(f) for f in args.files] if len(args.outgroup) else None
    csv_text, align_text, records, templates = _render(args, groups, ingroup, device)
    if args.out_csv is not None:
        with open(args.out_csv, "w") as f:
            f.write(csv_text)
    else:
        sys.stdout.write(csv_text)
    if args.out_align is not None:
        with open(args.out_align, "w") as f:
            f.write(align_text)
    _run_reports(args, groups, ingroup, device, records, templates)
    if args.verbose:
        print(f"=> Found {len(groups):,} regions in {prettyTime(time.time() - t0)} "
              f"({stats['kmers']:,} k-mers, device {stats['device_s']:.3f} s)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())

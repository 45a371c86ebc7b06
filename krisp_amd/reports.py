"""The report passes of `krisp_fasta`: what runs after the diagnostic regions are found, on one device, one genome at a
time -- where the regions lie (--out_locations), their near matches (--out_near), the products of their flanks
(--out_products), a primer pair per region, picked among its best pairs by their products where asked, and its products
(--design-primers, --primer-candidates, --out_primer_products), a guide per
region, picked among its best candidates by their outgroup hits where asked (--out_guides, --guide-candidates), and its
hits (--out_guide_hits, --guide-hit-bulges), the guide hits inside the primers' products (--out_assay_hits) and N mutually
compatible assays of the designed pairs (--panel) and what their oligos amplify together (--out_panel_products) -- with their refusals, table builders and TSV writers.  krisp_fasta imports every name back: its
command line and its callers reach the passes there."""
import os

import numpy as np

from . import amplicon, codec, fasta
from .codec import _is_wide
from .fasta import simplename


def _engine(device):
    """a context under KRISP_HBM_BUDGET (bytes; tests and shared devices: kr_create's HBM budget)"""
    from . import _native
    return _native.Engine(device=device, hbm_budget=int(os.environ.get("KRISP_HBM_BUDGET", "0")))


# ----------------------------------------------------------------------------
# locations of the surviving groups' windows (--out_locations)
# ----------------------------------------------------------------------------
LOCATION_HEADER = "region\tfile\trecord\trecord_index\tstart\tend\tstrand\tsequence"
LOCATION = np.dtype([("region", "<u4"), ("file", "O"), ("record", "O"), ("record_index", "<i8"), ("start", "<i8"),
                     ("end", "<i8"), ("strand", "U1"), ("sequence", "O")])


def _group_flanks(groups, L, R):
    """the (left, right) flank text of every group, in the groups' order -> uint8 [groups, L + R], upper case, T for U.
    RecordGroups and WindowGroups give theirs from the device's records / windows: no Amplicon is made."""
    if isinstance(groups, amplicon.RecordGroups):
        keys = groups.records["key"]
        if len(keys) == 0:
            return np.empty((0, L + R), dtype=np.uint8)
        pre = keys & codec.prefix_mask(L, R)
        first = np.flatnonzero(np.concatenate([[True], pre[1:] != pre[:-1]]))
        return np.ascontiguousarray(codec.keys_to_matrix(keys[first], groups.L, groups.D, groups.R)[:, :L + R])
    if isinstance(groups, amplicon.WindowGroups):
        rows = groups.rows
        if len(rows) == 0:
            return np.empty((0, L + R), dtype=np.uint8)
        fl = np.concatenate([rows[:, :L], rows[:, rows.shape[1] - R:]], axis=1)
        return np.ascontiguousarray(np.unique(fl, axis=0))      # (groups_from_windows orders groups by these bytes)
    text = "".join(g[0].left + g[0].right for g in groups).replace("U", "T").encode("ascii")
    return np.frombuffer(text, dtype=np.uint8).reshape(-1, L + R)


LOCATE_MAX_BASES = (1 << 33) - 65     # the packed path's limit (KR_MAX_BASES)


def _scan_genomes(files, Le, De, Re, k, omit_soft, device, table, last=None):
    """The per-file loop of the passes that scan one genome at a time (locate_regions, near_matches, predict_products,
    primer_products): a locate context on `device`, table(eng) once, then every file uploaded alone as genome 0.
    Yields (eng, file index, path, RNA, names): names() -> (the record separators, the record IDs), their count checked.
    (The next file is read and inflated on a host thread while the device holds the current one: two texts at most.)
    last: called as last(eng) behind the last file, before the engine closes (select_panel_clean's selection)."""
    from concurrent.futures import ThreadPoolExecutor
    with _engine(device) as eng, ThreadPoolExecutor(max_workers=1) as pool:
        eng.set_params_locate(Le, De, Re, omit_soft, max_bases=LOCATE_MAX_BASES)
        table(eng)
        ahead = pool.submit(fasta.read_text, files[0]) if files else None
        for fi, path in enumerate(files):
            text, universal = ahead.result()
            ahead = pool.submit(fasta.read_text, files[fi + 1]) if fi + 1 < len(files) else None
            while True:
                try:
                    n, rna, _ = fasta.ingest_on_device(eng, 0, text, universal, k, omit_soft)
                    break
                except fasta.GzipTextLonger:
                    text, universal = fasta.read_text(path)     # (that file is read on the host from now on: read_text knows it)

            def names():
                seps = eng.locate_seps(0).astype(np.int64)
                # the record IDs: from the text the host holds, or -- a file the device inflated -- from the file read again
                ids = fasta.record_ids(path) if isinstance(text, fasta.BgzfFile) else fasta.record_ids_text(text, universal)
                nrec = len(seps) + 1 if n else 0
                if n and len(ids) != nrec:
                    raise RuntimeError(f"{path}: {len(ids)} record IDs, but the device's bases hold {nrec} records")
                return seps, ids

            yield eng, fi, path, rna, names
            del text, names
        if last is not None:
            last(eng)


def _record_coords(seps, pos):
    """positions in the device's bases -> (index of the record, 0-based start in it); seps = the separators, ascending"""
    ri = np.searchsorted(seps, pos)
    rec_start = np.where(ri > 0, seps[np.maximum(ri - 1, 0)] + 1, 0) if len(seps) else 0
    return ri, pos - rec_start


def _fill_shared(part, path, seps, ids, pos, strand):
    """the columns every pass's dtype has: file, record, record_index, start, strand ('end' is the pass's own)"""
    ri, start = _record_coords(seps, pos)
    part["file"] = path
    part["record"] = np.asarray(ids, dtype=object)[ri]
    part["record_index"] = ri
    part["start"] = start
    part["strand"] = np.where(strand == 0, "+", "-")


def _rows_text(rows, k, rna):
    """(n, k) window bytes -> the n texts as objects, U for T in an RNA genome"""
    if rna:
        rows = np.where(rows == ord("T"), np.uint8(ord("U")), rows)
    return np.ascontiguousarray(rows).view(f"S{k}").ravel().astype(f"U{k}").astype(object)


def _sorted_parts(parts, dtype):
    """parts = [(file index, the file's rows, their sort key)] -> one array ordered by the key, then the file's index
    (stable: a file's rows of one key keep their order)"""
    if not parts:
        return np.empty(0, dtype=dtype)
    out = np.concatenate([p for _, p, _ in parts])
    fidx = np.concatenate([np.full(len(p), fi, dtype=np.int64) for fi, p, _ in parts])
    return out[np.lexsort((fidx, np.concatenate([key for _, _, key in parts])))]


def _fan_out(index, regions):
    """A hit of table row t is a row for every region that owns t.  index: the table row of every hit, regions[t]: the
    regions of row t (a list of lists) -> (rep, region): output row j repeats hit rep[j] for region[j]; a hit's rows
    stand together, in the order of its table row's list"""
    count = np.array([len(r) for r in regions], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(count)])
    flat = np.array([x for r in regions for x in r], dtype=np.uint32)
    each = count[index]
    rep = np.repeat(np.arange(len(index)), each)
    within = np.arange(len(rep)) - np.repeat(np.cumsum(each) - each, each)
    return rep, flat[first[index[rep]] + within]


def _fill_product(part, hits):
    """the product's columns from PRODUCT_HIT-shaped hits, after _fill_shared: length, end and the four mismatch figures"""
    part["length"] = hits["length"]
    part["end"] = part["start"] + part["length"]
    part["left_mismatches"] = hits["left_mm"]
    part["right_mismatches"] = hits["right_mm"]
    part["left_end_mismatches"] = hits["left_end_mm"]
    part["right_end_mismatches"] = hits["right_end_mm"]


def _mask_columns(mask):
    """a column mask -> the 1-based columns that differ, ascending and comma-separated; '-' for none"""
    return ",".join(str(c + 1) for c in range(64) if (mask >> c) & 1) or "-"


def _fill_guide_hit(part, hits, count="mismatches", src_count="mismatches", src_pam="pam"):
    """a guide hit's columns: the mismatch count (part[count] from hits[src_count]), the columns that differ and the two
    motif bits of hits[src_pam]"""
    part[count] = hits[src_count]
    part["mismatch_columns"] = [_mask_columns(m) for m in hits["columns"].tolist()]
    part["pam5_match"] = hits[src_pam] & 1
    part["pam3_match"] = (hits[src_pam] >> 1) & 1


def _text_matrix(texts, G, who):
    """the guide texts of pass `who` -> uint8 [texts, G]; ValueError unless every text has G letters"""
    if any(len(t) != G for t in texts):
        raise ValueError(f"{who}: every text has --guide-size = {G} letters")
    return np.frombuffer(b"".join(bytes(t) for t in texts), dtype=np.uint8).reshape(-1, G)


def _check_max_product(max_product, left, right, pairs):
    """ValueError unless max_product holds the two primers of every pair"""
    for i, j in pairs.tolist():
        if max_product < len(left[i]) + len(right[j]):
            raise ValueError(f"--max-product must be at least a pair's two primers together, {len(left[i]) + len(right[j])} "
                             f"bases (got {max_product})")


def _write_tsv(path, header, rows, names=None):
    """`header`, then a line per row of the structured array `rows`: its fields `names` (default: all, in the dtype's
    order), each an int or a str, tab-separated"""
    names = rows.dtype.names if names is None else names
    with open(path, "w") as f:
        f.write(header + "\n")
        f.writelines("\t".join(str(v) for v in row) + "\n" for row in zip(*(rows[n].tolist() for n in names)))


def locate_regions(groups, ingroup_files, outgroup_files, L, R, amplicon_len, omit_soft=False, device=0):
    """Where every window of every group lies: `groups` as find_regions / find_regions_multi_device /
    find_regions_distributed returned them (lists, amplicon.RecordGroups, amplicon.WindowGroups), the same files and
    geometry.  A separate pass over the inputs on one device (kr_locate_*): each genome is uploaded alone and scanned
    against a hash table of the groups' (left, right) flanks.  Returns a LOCATION array, one row per window and strand:
    region = the group's index, file = the path as given, record / record_index = the record's ID and its index among
    the records the reader yields (fasta.read_records), start / end = 0-based half-open coordinates on the record's
    forward strand, strand '+' (the window as written) or '-' (its reverse complement), sequence = the k-mer as the
    alignment lists it for that genome.  Rows in (region, file in command-line order, record_index, start, strand) order.
    For every group, genome label and sequence there are as many rows as the label occurs in that Amplicon's labels."""
    files = list(ingroup_files) + list(outgroup_files)
    k = amplicon_len
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    flanks = _group_flanks(groups, Le, Re)
    if len(flanks) == 0:
        return np.empty(0, dtype=LOCATION)
    parts = []
    for eng, fi, path, rna, names in _scan_genomes(files, Le, De, Re, k, omit_soft, device, lambda eng: eng.locate_table(flanks)):
        hits = eng.locate(0)
        rows = eng.locate_windows(k)
        seps, ids = names()             # (checked for a genome without hits too)
        if len(hits) == 0:
            continue
        part = np.empty(len(hits), dtype=LOCATION)
        _fill_shared(part, path, seps, ids, hits["pos"].astype(np.int64), hits["strand"])
        part["region"] = hits["group"]
        part["end"] = part["start"] + k
        part["sequence"] = _rows_text(rows, k, rna)
        parts.append((fi, part, part["region"]))       # (a file's rows are in (position, strand) order already)
    return _sorted_parts(parts, LOCATION)


def write_locations(path, locs):
    """the TSV of --out_locations: LOCATION_HEADER, then a line per row"""
    _write_tsv(path, LOCATION_HEADER, locs, LOCATION.names)


# ----------------------------------------------------------------------------
# near matches of the ingroup windows in every genome (--out_near)
# ----------------------------------------------------------------------------
NEAR_HEADER = "region\ttarget\tfile\trecord\trecord_index\tstart\tend\tstrand\tmismatches\tflank_mismatches\tsequence"
NEAR = np.dtype([("region", "<u4"), ("target", "O"), ("file", "O"), ("record", "O"), ("record_index", "<i8"),
                 ("start", "<i8"), ("end", "<i8"), ("strand", "U1"), ("mismatches", "<u4"), ("flank_mismatches", "<u4"),
                 ("sequence", "O")])
NEAR_MAX_MISMATCHES = 3


def near_refusal(L, R, amplicon_len, mismatches):
    """why the near-match pass does not take this geometry and distance (one line), or None"""
    k = amplicon_len
    if mismatches < 0 or mismatches > NEAR_MAX_MISMATCHES:
        return f"--near-mismatches must lie between 0 and {NEAR_MAX_MISMATCHES} (got {mismatches})"
    if mismatches >= k:
        return f"--near-mismatches must be smaller than the amplicon length {k} (got {mismatches})"
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    if _is_wide(Le, De, Re):
        return (f"--out_near takes amplicons of at most 32 bases with at most 16 diagnostic bases (got {Le}/{De}/{Re}): for "
                "longer amplicons near matches are a question of primers, not of Hamming distance")
    return None


def near_targets(groups, ingroup_labels):
    """The targets of the near-match pass: for group i, the sequence (U written as T) of every Amplicon that has at least
    one ingroup label -- of every Amplicon when ingroup_labels is None (a run without outgroup) --, equal texts once,
    ordered by their bytes.  `groups` in any form find_regions* returns.  -> list of (i, text), ordered by (i, text)."""
    ingroup = None if ingroup_labels is None else frozenset(ingroup_labels)
    out = []
    for i, g in enumerate(groups):
        texts = {a.sequence.replace("U", "T").replace("u", "t") for a in g
                 if ingroup is None or not ingroup.isdisjoint(a.labels)}
        out.extend((i, t) for t in sorted(texts, key=lambda t: t.encode("ascii")))
    return out


def near_matches(groups, ingroup_files, outgroup_files, L, R, amplicon_len, mismatches=1, omit_soft=False, device=0):
    """Every window of every input genome within Hamming distance `mismatches` of a target (near_targets: the ingroup
    windows of the diagnostic regions), on both strands, wherever it lies -- what the exact k-mer intersection cannot
    see: a window whose conserved FLANK differs by a substitution or two.  `groups` as find_regions* returned them, the
    same files and geometry.  A separate pass over the inputs on one device in the manner of locate_regions
    (kr_near_*: pigeonhole seeds filter, a byte comparison decides).  Returns a NEAR array: region, target (DNA letters),
    file, record, record_index, start, end, strand, sequence as in LOCATION; mismatches = the differing columns,
    flank_mismatches = those of them in the conserved flanks.  Rows in (region, target, file in command-line order,
    record_index, start, '+' before '-') order.  Packed geometries only, 0 <= mismatches <= 3 (ValueError otherwise)."""
    why = near_refusal(L, R, amplicon_len, mismatches)
    if why is not None:
        raise ValueError(why)
    files = list(ingroup_files) + list(outgroup_files)
    k = amplicon_len
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    ingroup = [simplename(f) for f in ingroup_files] if len(outgroup_files) else None
    targets = near_targets(groups, ingroup)
    if not targets:
        return np.empty(0, dtype=NEAR)
    t_region = np.array([i for i, _ in targets], dtype=np.uint32)
    t_text = np.array([t for _, t in targets], dtype=object)
    t_bytes = np.frombuffer("".join(t for _, t in targets).encode("ascii"), dtype=np.uint8).reshape(-1, k)
    parts = []
    for eng, fi, path, rna, names in _scan_genomes(files, Le, De, Re, k, omit_soft, device,
                                                   lambda eng: eng.near_table(t_bytes, mismatches)):
        hits = eng.near(0)
        if len(hits) == 0:
            continue
        rows = eng.near_windows(k)
        seps, ids = names()
        pos = hits["pos"].astype(np.int64)
        tg = hits["target"].astype(np.int64)
        part = np.empty(len(hits), dtype=NEAR)
        _fill_shared(part, path, seps, ids, pos, hits["strand"])
        part["region"] = t_region[tg]
        part["target"] = t_text[tg]
        part["end"] = part["start"] + k
        part["mismatches"] = hits["mismatches"]
        part["flank_mismatches"] = hits["flank_mismatches"]
        part["sequence"] = _rows_text(rows, k, rna)
        # (a file's hits come in position order; within the table they go by target, then position, then strand)
        order = np.lexsort((hits["strand"], pos, tg))
        parts.append((fi, part[order], tg[order]))
    return _sorted_parts(parts, NEAR)


def write_near(path, rows):
    """the TSV of --out_near: NEAR_HEADER, then a line per row"""
    _write_tsv(path, NEAR_HEADER, rows, NEAR.names)


# ----------------------------------------------------------------------------
# predicted PCR products of the regions' flanks in every genome (--out_products)
# ----------------------------------------------------------------------------
PRODUCT_HEADER = ("region\tfile\trecord\trecord_index\tstart\tend\tstrand\tlength\tleft_mismatches\tright_mismatches\t"
                  "left_end_mismatches\tright_end_mismatches")
PRODUCT = np.dtype([("region", "<u4"), ("file", "O"), ("record", "O"), ("record_index", "<i8"), ("start", "<i8"),
                    ("end", "<i8"), ("strand", "U1"), ("length", "<i8"), ("left_mismatches", "<u4"), ("right_mismatches", "<u4"),
                    ("left_end_mismatches", "<u4"), ("right_end_mismatches", "<u4")])
PRODUCT_MAX_MISMATCHES = 3
PRODUCT_MIN_PRIMER = 10      # bases of a flank from which it is searched as a primer (a condition, not a measurement)
PRODUCT_END = 5              # the "last five 3' bases" of --max_end_gc: where the end mismatches are counted


def products_refusal(L, R, amplicon_len, mismatches, max_product):
    """why the product pass does not take this geometry, distance and product length (one line), or None"""
    k = amplicon_len
    if mismatches < 0 or mismatches > PRODUCT_MAX_MISMATCHES:
        return f"--primer-mismatches must lie between 0 and {PRODUCT_MAX_MISMATCHES} (got {mismatches})"
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    if min(Le, Re) < PRODUCT_MIN_PRIMER:
        return (f"--out_products takes conserved flanks of at least {PRODUCT_MIN_PRIMER} bases each (got {Le}/{De}/{Re}): a "
                "shorter text with a mismatch or two binds nearly everywhere")
    if max_product < Le + Re:
        return f"--max-product must be at least the two flanks together, {Le + Re} bases (got {max_product})"
    if max_product >= 1 << 31:
        return f"--max-product must be smaller than 2^31 bases (got {max_product})"
    return None


def predict_products(groups, ingroup_files, outgroup_files, L, R, amplicon_len, mismatches=1, max_product=1000,
                     omit_soft=False, device=0):
    """In-silico PCR of every region's conserved flanks against every input genome: a product is a window within
    `mismatches` substitutions of the left flank and one within as many of the right flank on ONE record, facing each
    other ('+': left ... right as written; '-': rc(right) ... rc(left)), not overlapping, at most `max_product` bases
    from the first base of the first to the last base of the second -- whatever lies between them.  What the exact
    k-mer intersection cannot see: a genome whose flank differs by a substitution, or whose diagnostic stretch is longer
    or shorter, still amplifies.  `groups` as find_regions* returned them, the same files and geometry.  A separate pass
    over the inputs on one device in the manner of locate_regions (kr_products_*).  Returns a PRODUCT array: region, file,
    record, record_index, start, end, strand as in LOCATION (end - start = length); left / right_mismatches = the distance
    of the left flank's and the right flank's window, left / right_end_mismatches = those of them in the PRODUCT_END
    columns at the primer's 3' end (the last of the left flank, the first of the right).  Rows in (region, file in
    command-line order, record_index, start, end, '+' before '-') order.  Flanks of at least PRODUCT_MIN_PRIMER bases,
    0 <= mismatches <= 3 (ValueError otherwise)."""
    why = products_refusal(L, R, amplicon_len, mismatches, max_product)
    if why is not None:
        raise ValueError(why)
    files = list(ingroup_files) + list(outgroup_files)
    k = amplicon_len
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    flanks = _group_flanks(groups, Le, Re)
    if len(flanks) == 0:
        return np.empty(0, dtype=PRODUCT)
    # (distinct texts once: regions that overlap share a flank; region i is pair i)
    left, li = np.unique(flanks[:, :Le], axis=0, return_inverse=True)
    right, ri_ = np.unique(flanks[:, Le:], axis=0, return_inverse=True)
    pairs = np.stack([li.ravel(), ri_.ravel()], axis=1).astype(np.uint32)
    parts = []
    for eng, fi, path, _rna, names in _scan_genomes(files, Le, De, Re, k, omit_soft, device,
                                                    lambda eng: eng.products_table(left, right, pairs, mismatches, max_product)):
        hits = eng.products(0)
        if len(hits) == 0:
            continue
        seps, ids = names()
        part = np.empty(len(hits), dtype=PRODUCT)
        _fill_shared(part, path, seps, ids, hits["pos"].astype(np.int64), hits["strand"])
        part["region"] = hits["pair"]
        _fill_product(part, hits)
        # (a file's rows are in (position, length, strand) order already -- positions ascend with (record_index, start))
        parts.append((fi, part, part["region"]))
    return _sorted_parts(parts, PRODUCT)


def write_products(path, rows):
    """the TSV of --out_products and of --out_primer_products: PRODUCT_HEADER, then a line per row"""
    _write_tsv(path, PRODUCT_HEADER, rows, PRODUCT.names)


# ----------------------------------------------------------------------------
# a primer pair per region, designed on the device (--design-primers)
# ----------------------------------------------------------------------------
def design_templates(groups, ingroup_labels):
    """the templates of the groups (primers.design_template) -> (uint8 [groups, L + D + R], L, D, R)"""
    from . import primers
    ingroup = None if ingroup_labels is None else frozenset(ingroup_labels)
    texts, geo = [], (0, 0, 0)
    for g in groups:
        geo = (len(g[0].left), len(g[0].diag), len(g[0].right))
        texts.append(primers.design_template(g, ingroup))
    k = sum(geo)
    if any(len(t) != k for t in texts):
        raise ValueError("design_templates: groups of more than one geometry")
    rows = np.frombuffer("".join(texts).encode("ascii"), dtype=np.uint8).reshape(len(texts), k) if texts else \
        np.empty((0, max(k, 1)), dtype=np.uint8)
    return (rows,) + geo


def design_primers(groups, ingroup_labels, tm=(53, 68), gc=(40, 70), amp_size=(70, 150), primer_size=(25, 35), max_sec_tm=40,
                   gc_clamp=1, max_end_gc=4, device=0, hairpins=False, templates=None):
    """A primer pair for every region, on the device (kr_design_*): on the consensus of the region's ingroup
    Amplicons -- the template --primer3 designs on -- a left primer inside the left flank and a right primer inside the
    right flank, lengths within `primer_size`; nearest-neighbour Tm within `tm` (degrees Celsius), GC percent within `gc`,
    no run of five equal bases, the last `gc_clamp` 3' bases G or C, at most `max_end_gc` G or C among the last five; the
    duplex figures (the highest Tm of a run of Watson-Crick pairs in an ungapped antiparallel alignment: self_any, self_end,
    pair_any, pair_end) at most `max_sec_tm`; the product within `amp_size`; of the passing pairs the one of least
    penalty, ties to the smallest (left_start, left_len, right_start, right_len).  Every figure is an integer
    (krisp_amd/thermo.py holds the model); no gapped or mismatched duplexes: this is not Primer3.  hairpins=True holds
    every primer to `max_sec_tm` for its hairpin figure too (the highest Tm of a stem of two or more pairs
    around a loop of three or more bases) and returns it.
    `groups` as find_regions* returned them.  Returns a _native.DESIGN_RECORD array, one row per group (found = 0: no
    pair); with hairpins a DESIGN_RECORD_HP array, the same fields and left_hairpin, right_hairpin.  ValueError for figures
    the pass does not take (thermo.refusal).  templates = design_templates(groups, ingroup_labels) where the caller has them
    already."""
    from . import thermo
    opts = dict(tm=tuple(tm), gc=tuple(gc), amp_size=tuple(amp_size), primer_size=tuple(primer_size), max_sec_tm=max_sec_tm,
                gc_clamp=gc_clamp, max_end_gc=max_end_gc)
    why = thermo.refusal(**opts)
    if why is not None:
        raise ValueError(why)
    rows, L, D, R = design_templates(groups, ingroup_labels) if templates is None else templates
    if len(rows) == 0:
        from . import _native
        return np.empty(0, dtype=_native.DESIGN_RECORD_HP if hairpins else _native.DESIGN_RECORD)
    with _engine(device) as eng:
        eng.design_table(thermo.params(**opts))
        if hairpins:
            eng.design_hairpins(thermo.hairpin_params())
        return eng.design(rows, L, D, R)


# ----------------------------------------------------------------------------
# predicted PCR products of the designed primer pairs in every genome (--design-primers --out_primer_products)
# ----------------------------------------------------------------------------
def primer_products_refusal(amp_size, mismatches, max_product):
    """why the primer-product pass does not take this distance and product length (one line), or None"""
    if mismatches < 0 or mismatches > PRODUCT_MAX_MISMATCHES:
        return f"--primer-mismatches must lie between 0 and {PRODUCT_MAX_MISMATCHES} (got {mismatches})"
    if amp_size is not None and max_product < amp_size[1]:
        return (f"--max-product must be at least the upper bound of --amp_size, {amp_size[1]} bases (got {max_product}): the "
                "designed product itself would not be found")
    if max_product >= 1 << 31:
        return f"--max-product must be smaller than 2^31 bases (got {max_product})"
    return None


def primer_pairs(rows, records):
    """The table of the primer-product pass from the templates (design_templates) and design_primers' records: the
    regions with found = 0 take no part, a region's left text is template[left_start, left_start + left_len) and its
    right text template[right_start, right_start + right_len) (the template's text under the right primer), equal texts
    are listed once (ordered by their bytes), equal (left, right) pairs of different regions once.  -> (left texts, right
    texts, pairs [np, 2], regions of pair p as a list of lists): a region is named by its rank among the regions with
    a pair."""
    lt, rt = [], []
    for row, r in zip(rows, records):
        if not int(r["found"]):
            continue
        ls, ll, rs, rl = (int(r[f]) for f in ("left_start", "left_len", "right_start", "right_len"))
        lt.append(bytes(row[ls:ls + ll]))
        rt.append(bytes(row[rs:rs + rl]))
    left, right = sorted(set(lt)), sorted(set(rt))
    li = {t: i for i, t in enumerate(left)}
    ri = {t: i for i, t in enumerate(right)}
    regions = {}
    for rank, (a, b) in enumerate(zip(lt, rt)):
        regions.setdefault((li[a], ri[b]), []).append(rank)
    keys = sorted(regions)
    return left, right, np.array(keys, dtype=np.uint32).reshape(-1, 2), [regions[k] for k in keys]


def primer_products(groups, records, ingroup_labels, ingroup_files, outgroup_files, L, R, amplicon_len, mismatches=1,
                    max_product=1000, omit_soft=False, device=0):
    """In-silico PCR of the primer pairs design_primers picked (`records`, one per group) against every input genome:
    predict_products with the designed primers in the place of the flanks.  A primer lies anywhere inside its flank, has a
    length of its own within --primer_size and its own 3' end: a site is a window of the PRIMER'S length within
    `mismatches` substitutions of it, left / right_end_mismatches count the PRODUCT_END columns at the primer's own 3' end,
    and a product is a left primer's site and a right primer's on one record, facing each other, not overlapping, at most
    `max_product` bases from end to end.  The texts are cut from design_templates(groups, ingroup_labels); regions without
    a pair take no part.  A separate pass over the inputs on one device in the manner of locate_regions (kr_primers_*).
    Returns a PRODUCT array whose `region` is the region's rank among the regions with a pair -- its data row in the CSV
    of --design-primers when the renderer was not stopped --, the other columns and the rows' order as predict_products
    gives them.  Neighbouring regions that get the same pair each have their rows.  ValueError for figures the pass does
    not take."""
    why = primer_products_refusal(None, mismatches, max_product)
    if why is None and len(records) != len(groups):
        why = f"primer_products: {len(records)} records for {len(groups)} groups"
    if why is not None:
        raise ValueError(why)
    files = list(ingroup_files) + list(outgroup_files)
    k = amplicon_len
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    rows, _, _, _ = design_templates(groups, ingroup_labels)
    left, right, pairs, regions = primer_pairs(rows, records)
    if len(pairs) == 0:
        return np.empty(0, dtype=PRODUCT)
    _check_max_product(max_product, left, right, pairs)
    parts = []
    for eng, fi, path, _rna, names in _scan_genomes(files, Le, De, Re, k, omit_soft, device,
                                                    lambda eng: eng.primers_table(left + right, len(left), pairs, mismatches,
                                                                                  max_product)):
        hits = eng.primer_products(0)
        if len(hits) == 0:
            continue
        seps, ids = names()
        # a hit of pair p is a row for every region of p
        rep, region = _fan_out(hits["pair"].astype(np.int64), regions)
        hits = hits[rep]
        part = np.empty(len(hits), dtype=PRODUCT)
        _fill_shared(part, path, seps, ids, hits["pos"].astype(np.int64), hits["strand"])
        part["region"] = region
        _fill_product(part, hits)
        # (a file's rows are in (position, length, strand) order already -- positions ascend with (record_index, start))
        parts.append((fi, part, part["region"]))
    return _sorted_parts(parts, PRODUCT)


# ----------------------------------------------------------------------------
# the primer pair picked among a region's best pairs by its products in every genome (--primer-candidates)
# ----------------------------------------------------------------------------
PRIMER_MAX_CANDIDATES = 8
PRIMER_CANDIDATE_HEADER = ("region\trank\tshortlisted\tpair_penalty\tproduct_size\tleft_sequence\tright_sequence\tleft_start\t"
                           "left_length\tright_start\tright_length\tproducts\tpicked")
PRIMER_TALLY_COLUMNS = 8            # kr_primers_tally: t0 .. t6, then the clean-end products


def primer_candidates_refusal(design_primers, candidates, out_primer_candidates, primer3):
    """why --primer-candidates / --out_primer_candidates are not taken (one line), or None.  design_primers, primer3,
    out_primer_candidates: whether they are asked for; candidates: the option's value or None"""
    if candidates is None:
        return "--out_primer_candidates needs --primer-candidates" if out_primer_candidates else None
    if primer3:
        return "--primer-candidates cannot be combined with --primer3 (the pairs Primer3 designs are not re-ranked)"
    if not design_primers:
        return "--primer-candidates needs --design-primers (the pairs it picks)"
    if candidates < 1 or candidates > PRIMER_MAX_CANDIDATES:
        return f"--primer-candidates must lie between 1 and {PRIMER_MAX_CANDIDATES} (got {candidates})"
    return None


def design_primer_shortlist(groups, ingroup_labels, tm=(53, 68), gc=(40, 70), amp_size=(70, 150), primer_size=(25, 35), max_sec_tm=40,
                            gc_clamp=1, max_end_gc=4, device=0, hairpins=False, templates=None, top=PRIMER_MAX_CANDIDATES):
    """design_primers' passing pairs of every region in design_primers' order -- ascending (pair_penalty, left_start,
    left_len, right_start, right_len) --, the first `top` (1 .. 8) of them, on the device (kr_design_run_top).
    Returns a _native.DESIGN_RECORD array [groups, top], with hairpins DESIGN_RECORD_HP: column j = the pair of rank j + 1
    with all its figures, column 0 = design_primers' record; found = 0 where the region has fewer.  ValueError for figures
    the pass does not take"""
    from . import _native, thermo
    if top < 1 or top > PRIMER_MAX_CANDIDATES:
        raise ValueError(f"--primer-candidates must lie between 1 and {PRIMER_MAX_CANDIDATES} (got {top})")
    opts = dict(tm=tuple(tm), gc=tuple(gc), amp_size=tuple(amp_size), primer_size=tuple(primer_size), max_sec_tm=max_sec_tm,
                gc_clamp=gc_clamp, max_end_gc=max_end_gc)
    why = thermo.refusal(**opts)
    if why is not None:
        raise ValueError(why)
    rows, L, D, R = design_templates(groups, ingroup_labels) if templates is None else templates
    if len(rows) == 0:
        return np.empty((0, top), dtype=_native.DESIGN_RECORD_HP if hairpins else _native.DESIGN_RECORD)
    with _engine(device) as eng:
        eng.design_table(thermo.params(**opts))
        if hairpins:
            eng.design_hairpins(thermo.hairpin_params())
        return eng.design_top(rows, L, D, R, top)


_BASE_CODE = np.full(256, 255, dtype=np.uint8)
_BASE_CODE[[ord(x) for x in "ACGT"]] = [0, 1, 2, 3]


def _distinct_texts(flat, at, length):
    """The texts flat[at[i], at[i] + length[i]) of 10 .. 60 letters A, C, G, T, equal texts once, ordered by their bytes ->
    (the distinct texts as bytes, int64: the text of every i).  No loop over i: a text is packed, two bits a letter, into
    two uint64 -- 32 letters, then 28 and the length --, whose order is the order of the bytes (A < C < G < T as 0 .. 3; a
    text sorts behind its prefixes as the padding is A's code and the length breaks the tie)"""
    key = at.astype(np.int64) * 64 + length.astype(np.int64)
    ukey, slot = np.unique(key, return_inverse=True)           # (neighbouring ranks often share a primer)
    uat, ulen = ukey // 64, ukey % 64
    width = int(ulen.max())
    hi = np.zeros(len(ukey), dtype=np.uint64)
    lo = ulen.astype(np.uint64)
    last = len(flat) - 1
    for c in range(width):                                      # (the letters' columns, 60 at most)
        code = _BASE_CODE[flat[np.minimum(uat + c, last)]]
        inside = c < ulen
        if (code[inside] > 3).any():
            raise ValueError("shortlist_pairs: a primer holds a letter other than A, C, G, T")
        v = np.where(inside, code, 0).astype(np.uint64)
        if c < 32:
            hi |= v << np.uint64(62 - 2 * c)
        else:
            lo |= v << np.uint64(62 - 2 * (c - 32))
    order = np.lexsort((lo, hi))
    hs, ls = hi[order], lo[order]
    new = np.concatenate([[True], (hs[1:] != hs[:-1]) | (ls[1:] != ls[:-1])])
    text_of = np.empty(len(ukey), dtype=np.int64)
    text_of[order] = np.cumsum(new) - 1
    first = order[new]
    letters = flat[np.minimum(uat[first][:, None] + np.arange(width)[None, :], last)].tobytes()
    texts = [letters[i * width:i * width + n] for i, n in enumerate(ulen[first].tolist())]
    return texts, text_of[np.asarray(slot).ravel()]


def shortlist_pairs(templates, shortlist):
    """The table of the shortlist's search: every filled slot's left text template[left_start, left_start + left_len) and
    right text template[right_start, right_start + right_len), as primer_pairs cuts them; equal texts are listed once,
    ordered by their bytes, equal (left, right) pairs of different slots or regions once, ordered by (left, right).
    -> (left texts, right texts, pairs uint32 [np, 2], int64 [regions, top]: the pair of every slot, -1 for an empty
    one).  Array indexing and np.unique throughout: no loop over the regions"""
    index = np.full(shortlist.shape, -1, dtype=np.int64)
    ri, si = np.nonzero(shortlist["found"])
    if len(ri) == 0:
        return [], [], np.empty((0, 2), dtype=np.uint32), index
    t = np.ascontiguousarray(templates, dtype=np.uint8).reshape(len(shortlist), -1)
    flat, base = t.ravel(), ri.astype(np.int64) * t.shape[1]
    s = shortlist[ri, si]
    left, li = _distinct_texts(flat, base + s["left_start"], s["left_len"])
    right, rj = _distinct_texts(flat, base + s["right_start"], s["right_len"])
    upair, inverse = np.unique(li * len(right) + rj, return_inverse=True)
    index[ri, si] = np.asarray(inverse).ravel()
    pairs = np.stack([upair // len(right), upair % len(right)], axis=1).astype(np.uint32)
    return left, right, pairs, index


def primer_tallies(left, right, pairs, ingroup_files, outgroup_files, L, R, amplicon_len, mismatches=1, max_product=1000,
                   omit_soft=False, device=0):
    """How often every pair (shortlist_pairs) amplifies in the input genomes: the search of primer_products over
    all files, ingroup and outgroup, and per file the device's count of the products by pair (kr_primers_tally) -- no
    product comes to the host.  Returns uint64 [pairs, 8]: column m = the products with left_mismatches +
    right_mismatches = m (0 .. 6; above 2 `mismatches` there is none), column 7 = those without a mismatch at either 3'
    end, summed over the files.  ValueError for figures the search does not take (primer_products_refusal)"""
    why = primer_products_refusal(None, mismatches, max_product)
    if why is not None:
        raise ValueError(why)
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    total = np.zeros((len(pairs), PRIMER_TALLY_COLUMNS), dtype=np.uint64)
    if len(pairs) == 0:
        return total
    both = np.array([len(x) for x in left], dtype=np.int64)[pairs[:, 0]] + np.array([len(x) for x in right], dtype=np.int64)[pairs[:, 1]]
    if max_product < int(both.max()):
        raise ValueError(f"--max-product must be at least a pair's two primers together, {int(both.max())} bases (got {max_product})")
    Le, De, Re = codec.effective_geometry(L, amplicon_len - L - R, R)
    files = list(ingroup_files) + list(outgroup_files)
    for eng, _, _, _, _ in _scan_genomes(files, Le, De, Re, amplicon_len, omit_soft, device,
                                         lambda eng: eng.primers_table(list(left) + list(right), len(left), pairs, mismatches,
                                                                       max_product)):
        if eng.primers_scan(0):
            total += eng.primers_tally()
    return total


def _tally_keys(tallies, mismatches):
    """kr_primers_tally's columns -> the tally the pick compares, (clean, t0, ..., t2M): uint64 [..., 2 M + 2]"""
    t = np.asarray(tallies, dtype=np.uint64)
    return np.concatenate([t[..., 7:8], t[..., :2 * int(mismatches) + 1]], axis=-1)


def pick_pairs(shortlist, index, tallies, mismatches):
    """The pick of --primer-candidates: per region the shortlisted pair whose tally (clean, t0, ..., t2M), M = `mismatches`,
    is lexicographically smallest, the lower rank where tallies tie.  shortlist: DESIGN_RECORD [regions, top]
    (design_primer_shortlist), index: [regions, top] rows of `tallies` (shortlist_pairs; -1: an empty slot), tallies: uint64
    [pairs, 8] (primer_tallies; the columns 2M + 1 .. 6 are not looked at).  -> (the picked records, [regions] of the
    shortlist's dtype -- a region without a pair keeps its record of rank 1, found = 0 --, their 0-based ranks, their
    tallies as uint64 [regions, 2 M + 2], zeros for a region without a pair).  Masked row minima: no loop over the regions"""
    n, top = shortlist.shape
    width = 2 * int(mismatches) + 2
    alive = index >= 0
    t = np.zeros((n, top, width), dtype=np.uint64)
    t[alive] = _tally_keys(tallies, mismatches).reshape(-1, width)[index[alive]]
    worst = np.uint64(np.iinfo(np.uint64).max)
    for m in range(width):
        col = np.where(alive, t[:, :, m], worst)
        alive &= col == col.min(axis=1, keepdims=True)
    ranks = np.argmax(alive, axis=1) if n else np.zeros(0, dtype=np.int64)      # (the first slot still alive; 0 where the region has none)
    rows = np.arange(n)
    return shortlist[rows, ranks], ranks.astype(np.int64), t[rows, ranks]


def write_primer_candidates(path, templates, shortlist, index, tallies, ranks, mismatches):
    """the TSV of --out_primer_candidates: PRIMER_CANDIDATE_HEADER, then a line per searched pair, by region, then rank.
    region: the region's rank among the regions with a pair, as --out_primer_products numbers them; rank from 1;
    shortlisted: the region's searched pairs; the sequences 5'->3' as the CSV shows them (the right primer is the reverse
    complement of the template under it), starts and lengths on the template; products: the pair's tally clean,t0,...,t2M
    (primer_tallies); picked = 1 for the region's pick (ranks: pick_pairs')"""
    keys = _tally_keys(tallies, mismatches)
    shortlisted = (index >= 0).sum(axis=1)
    region = np.cumsum(shortlisted > 0) - 1
    with open(path, "w") as f:
        f.write(PRIMER_CANDIDATE_HEADER + "\n")
        for i in np.flatnonzero(shortlisted).tolist():
            row = bytes(templates[i])
            for j in range(int(shortlisted[i])):
                r = shortlist[i, j]
                ls, ln, rs, rn = (int(r[k]) for k in ("left_start", "left_len", "right_start", "right_len"))
                right = row[rs:rs + rn].translate(bytes(_COMPLEMENT_BYTES))[::-1]
                f.write(f"{int(region[i])}\t{j + 1}\t{int(shortlisted[i])}\t{int(r['pair_penalty'])}\t{int(r['product_size'])}\t"
                        f"{row[ls:ls + ln].decode('ascii')}\t{right.decode('ascii')}\t{ls}\t{ln}\t{rs}\t{rn}\t"
                        f"{_tally_text(keys[index[i, j]])}\t{int(ranks[i] == j)}\n")


# ----------------------------------------------------------------------------
# a CRISPR guide per region, picked on the device (--out_guides)
# ----------------------------------------------------------------------------
GUIDE_HEADER = "region\tstrand\tstart\tend\tpam5\tpam3\tprotospacer\tgc_percent\tmin_mismatches\tsum_mismatches\tcandidates"
GUIDE_MIN_SIZE, GUIDE_MAX_SIZE, GUIDE_MAX_MOTIF = 12, 40, 8
# the IUPAC code as 4-bit sets: A = 1, C = 2, G = 4, T = 8
IUPAC_MASK = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11,
              "V": 7, "N": 15}
_GUIDE_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def motif_masks(motif):
    """a PAM / PFS motif in IUPAC letters (either case, U as T) -> its 4-bit masks, one per letter; ValueError for a
    letter outside the code"""
    out = []
    for ch in motif.upper():
        if ch not in IUPAC_MASK:
            raise ValueError(f"{ch!r} in the motif {motif!r} is no letter of the IUPAC code")
        out.append(IUPAC_MASK[ch])
    return out


def guides_refusal(amplicon_len, guide_size, pam5, pam3, gc, min_mismatches):
    """why the guide pass does not take these figures (one line), or None"""
    if guide_size < GUIDE_MIN_SIZE or guide_size > GUIDE_MAX_SIZE:
        return f"--guide-size must lie between {GUIDE_MIN_SIZE} and {GUIDE_MAX_SIZE} (got {guide_size})"
    if amplicon_len is not None and guide_size > amplicon_len:
        return f"--guide-size must not exceed the amplicon length {amplicon_len} (got {guide_size})"
    for opt, motif in (("--pam5", pam5), ("--pam3", pam3)):
        if len(motif) > GUIDE_MAX_MOTIF:
            return f"{opt} takes at most {GUIDE_MAX_MOTIF} letters (got {motif!r})"
        try:
            motif_masks(motif)
        except ValueError as e:
            return f"{opt}: {e}"
    if gc[0] > gc[1]:
        return f"--guide-gc: the upper bound lies below the lower ({gc[0]} .. {gc[1]})"
    if min_mismatches < 0 or min_mismatches > guide_size:
        return f"--guide-min-mismatches must lie between 0 and --guide-size, {guide_size} (got {min_mismatches})"
    return None


def guide_rows(groups, ingroup_labels, templates=None):
    """The rows of the guide pass: per group its template (primers.design_template), then one row per
    Amplicon of the group the template leaves out -- the outgroup rows, left + diag + right, upper case, U written as T.
    No ingroup_labels (a run without --outgroup): no outgroup rows.  templates = design_templates(groups, ingroup_labels)
    where the caller has them already.  -> (uint8 [rows, L + D + R], uint64 [groups + 1] row offsets, L, D, R)"""
    trows, L, D, R = design_templates(groups, ingroup_labels) if templates is None else templates
    ingroup = None if ingroup_labels is None else frozenset(ingroup_labels)
    k = L + D + R
    parts, off = [], [0]
    for gi, g in enumerate(groups):
        texts = []
        if ingroup is not None and len(g) > 1:
            texts = [(a.left + a.diag + a.right).upper().replace("U", "T") for a in g if not set(a.labels) <= ingroup]
        if any(len(t) != k for t in texts):
            raise ValueError("guide_rows: groups of more than one geometry")
        parts.append(bytes(trows[gi]))
        parts.extend(t.encode("ascii") for t in texts)
        off.append(off[-1] + 1 + len(texts))
    if len(off) - 1 != len(trows):
        raise ValueError(f"guide_rows: {len(trows)} templates for {len(off) - 1} groups")
    rows = np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(off[-1], k) if parts else np.empty((0, max(k, 1)), dtype=np.uint8)
    return rows, np.array(off, dtype=np.uint64), L, D, R


def design_guides(groups, ingroup_labels, guide_size=28, pam5="", pam3="", gc=(30, 70), min_mismatches=1, bounds=None, device=0,
                  templates=None):
    """A CRISPR guide for every region, on the device (kr_guides_*): the window of `guide_size` columns of the
    region's template -- on either strand -- whose 5' neighbours match the motif `pam5` and whose 3' neighbours match `pam3`
    (IUPAC letters, read 5'->3' on the guide's strand; "" = none), that holds only bases, has a GC percent within `gc` and
    no run of five equal bases, and that differs from every outgroup row of the region (guide_rows) in at least
    `min_mismatches` columns; of those the one whose least number of differences to an outgroup row is greatest, then
    whose sum over the outgroup rows is greatest, then the best centred on the diagnostic stretch, '+' before '-', the
    leftmost.  bounds: [groups, 2] columns [lo, hi) that window and motifs must lie in (default: the whole template).
    Every figure is an integer: no seed weights, no folding of the guide, no gapped matches, no off-target search
    (--guide-candidates weighs the best of these candidates by one: design_guide_shortlist, pick_guides).
    Returns a _native.GUIDE_RECORD array, one row per group (found = 0: no guide).  ValueError for figures the pass does
    not take (guides_refusal)."""
    return _guide_pass(groups, ingroup_labels, guide_size, pam5, pam3, gc, min_mismatches, bounds, device, templates, None)


def _guide_pass(groups, ingroup_labels, guide_size, pam5, pam3, gc, min_mismatches, bounds, device, templates, top):
    """design_guides (top = None: a record per group) and design_guide_shortlist (`top` records per group) on the device"""
    from . import _native
    why = guides_refusal(None, guide_size, pam5, pam3, tuple(gc), min_mismatches)
    if why is not None:
        raise ValueError(why)
    rows, off, L, D, R = guide_rows(groups, ingroup_labels, templates)
    n = len(off) - 1
    if n == 0:
        return np.empty(0 if top is None else (0, top), dtype=_native.GUIDE_RECORD)
    k = L + D + R
    if guide_size > k:
        raise ValueError(f"--guide-size must not exceed the amplicon length {k} (got {guide_size})")
    if bounds is None:
        bounds = np.tile(np.array([0, k], dtype=np.uint32), (n, 1))
    with _engine(device) as eng:
        eng.guides_table(guide_size, motif_masks(pam5), motif_masks(pam3), tuple(gc), min_mismatches)
        return eng.guides(rows, off, bounds, L, D) if top is None else eng.guides_top(rows, off, bounds, L, D, top)


def _guide_rc(text):
    return text[::-1].translate(_GUIDE_COMPLEMENT)


def _guide_line(template, r, guide_size, pam5_len, pam3_len, region):
    """the eleven columns of GUIDE_HEADER for the record r (found = 1) of a region with this template row"""
    from . import thermo
    g, a, b = guide_size, pam5_len, pam3_len
    t = bytes(template).decode("ascii")
    p = int(r["start"])
    if int(r["strand"]) == 0:
        strand, proto, m5, m3 = "+", t[p:p + g], t[p - a:p], t[p + g:p + g + b]
    else:
        strand, proto, m5, m3 = "-", _guide_rc(t[p:p + g]), _guide_rc(t[p + g:p + g + a]), _guide_rc(t[p - b:p])
    return (f"{region}\t{strand}\t{p}\t{p + g}\t{m5}\t{m3}\t{proto}\t{thermo.gc_percent(int(r['gc']), g)}\t"
            f"{int(r['min_mismatches'])}\t{int(r['sum_mismatches'])}\t{int(r['candidates'])}")


def _tally_text(tally):
    return ",".join(str(int(x)) for x in tally)


def write_guides(path, templates, records, guide_size, pam5_len=0, pam3_len=0, regions=None, ranks=None, shortlisted=None,
                 outgroup_hits=None):
    """the TSV of --out_guides: GUIDE_HEADER, then a line per region with a guide.  templates: the regions' template rows
    (design_templates), records: theirs (design_guides, or any array with GUIDE_RECORD's fields), regions: the number each
    region is listed under (default: its index).  start / end = the window's template columns, 0-based and half-open;
    pam5, pam3 and protospacer as read 5'->3' on the guide's strand.  With --guide-candidates the three columns of
    GUIDE_PICK_HEADER behind them, all three or none: ranks (pick_guides', 0-based; written 1-based), shortlisted (the
    region's searched candidates) and outgroup_hits ([regions, M + 1] counts, written t0,...,tM)"""
    picked = ranks is not None
    if picked != (shortlisted is not None) or picked != (outgroup_hits is not None):
        raise ValueError("write_guides: ranks, shortlisted and outgroup_hits come together")
    with open(path, "w") as f:
        f.write(GUIDE_HEADER + (GUIDE_PICK_HEADER if picked else "") + "\n")
        for i, (row, r) in enumerate(zip(templates, records)):
            if not int(r["found"]):
                continue
            line = _guide_line(row, r, guide_size, pam5_len, pam3_len, i if regions is None else int(regions[i]))
            if picked:
                line += f"\t{int(ranks[i]) + 1}\t{int(shortlisted[i])}\t{_tally_text(outgroup_hits[i])}"
            f.write(line + "\n")


# ----------------------------------------------------------------------------
# the guide picked among a region's best candidates by its outgroup off-targets (--guide-candidates)
# ----------------------------------------------------------------------------
GUIDE_MAX_CANDIDATES = 8
GUIDE_PICK_HEADER = "\trank\tshortlisted\toutgroup_hits"
GUIDE_CANDIDATE_HEADER = GUIDE_HEADER + GUIDE_PICK_HEADER + "\tpicked"


def guide_candidates_refusal(out_guides, candidates, outgroup_files, out_guide_candidates):
    """why --guide-candidates / --out_guide_candidates are not taken (one line), or None.  out_guides, out_guide_candidates:
    whether the outputs are asked for; candidates: the option's value or None"""
    if candidates is None:
        return "--out_guide_candidates needs --guide-candidates" if out_guide_candidates else None
    if not out_guides:
        return "--guide-candidates needs --out_guides (the guides it picks)"
    if candidates < 1 or candidates > GUIDE_MAX_CANDIDATES:
        return f"--guide-candidates must lie between 1 and {GUIDE_MAX_CANDIDATES} (got {candidates})"
    if len(outgroup_files) == 0:
        return "--guide-candidates needs an --outgroup file (the genomes its candidates are searched in)"
    return None


def design_guide_shortlist(groups, ingroup_labels, guide_size=28, pam5="", pam3="", gc=(30, 70), min_mismatches=1, bounds=None,
                           device=0, templates=None, top=GUIDE_MAX_CANDIDATES):
    """design_guides' candidates of every region in design_guides' order, the first `top` (1 .. 8) of them, on the device
    (kr_guides_run_top).  Returns a _native.GUIDE_RECORD array [groups, top]: column j = the candidate of rank
    j + 1, column 0 = design_guides' record; found = 0 where the region has fewer (`candidates` is the region's count in
    every column).  ValueError for figures the pass does not take"""
    if top < 1 or top > GUIDE_MAX_CANDIDATES:
        raise ValueError(f"--guide-candidates must lie between 1 and {GUIDE_MAX_CANDIDATES} (got {top})")
    return _guide_pass(groups, ingroup_labels, guide_size, pam5, pam3, gc, min_mismatches, bounds, device, templates, top)


_COMPLEMENT_BYTES = np.arange(256, dtype=np.uint8)
_COMPLEMENT_BYTES[[ord(x) for x in "ACGT"]] = [ord(x) for x in "TGCA"]


def shortlist_texts(templates, shortlist, guide_size):
    """The table of the shortlist's search: every filled slot's protospacer as read 5'->3' on its strand (as guide_texts:
    template[start, start + guide_size), its reverse complement for strand 1), equal texts listed once, ordered by their
    bytes.  -> (the distinct texts as bytes, int64 [regions, top]: the text of every slot, -1 for an empty one)"""
    g = guide_size
    index = np.full(shortlist.shape, -1, dtype=np.int64)
    ri, si = np.nonzero(shortlist["found"])
    if len(ri) == 0:
        return [], index
    t = np.ascontiguousarray(templates, dtype=np.uint8).reshape(len(shortlist), -1)
    start = shortlist["start"][ri, si].astype(np.int64)
    minus = shortlist["strand"][ri, si] != 0
    # column c of a text: template column start + c on '+', the complement of column start + g - 1 - c on '-'
    cols = np.where(minus[:, None], start[:, None] + (g - 1 - np.arange(g))[None, :], start[:, None] + np.arange(g)[None, :])
    text = t[ri[:, None], cols]
    text = np.where(minus[:, None], _COMPLEMENT_BYTES[text], text)
    uniq, inverse = np.unique(text, axis=0, return_inverse=True)
    index[ri, si] = np.asarray(inverse).ravel()
    return [bytes(u) for u in uniq], index


def guide_tallies(texts, outgroup_files, guide_size, mismatches=2, pam5="", pam3="", need_pam=False, omit_soft=False, device=0):
    """How often every text (shortlist_texts) hits the outgroup genomes: the guide-hit search of guide_hits over
    the outgroup files only, both strands, and per file the device's count of the hits by text and distance
    (kr_guide_hits_tally) -- no hit and no window comes to the host.  Returns uint64 [texts, 4]: column m = the windows with
    exactly m mismatches, summed over the files; the columns above `mismatches` are 0.  ValueError for figures the search
    does not take (guide_hits_refusal)"""
    why = guide_hits_refusal(guide_size, mismatches, pam5, pam3, need_pam)
    if why is not None:
        raise ValueError(why)
    G = guide_size
    total = np.zeros((len(texts), 4), dtype=np.uint64)
    if len(texts) == 0:
        return total
    t_bytes = _text_matrix(texts, G, "guide_tallies")
    for eng, _, _, _, _ in _scan_genomes(list(outgroup_files), 0, G, 0, G, omit_soft, device,
                                         lambda eng: eng.guide_hits_table(t_bytes, mismatches, pam5, pam3, need_pam)):
        if eng.guide_hits_scan(0):
            total += eng.guide_hits_tally()
    return total


def pick_guides(shortlist, index, tallies, mismatches):
    """The pick of --guide-candidates: per region the shortlisted candidate whose tally (t0, ..., tM), M = `mismatches`, is
    lexicographically smallest, the lower rank where tallies tie.  shortlist: GUIDE_RECORD [regions, top]
    (design_guide_shortlist), index: [regions, top] rows of `tallies` (shortlist_texts; -1: an empty slot), tallies:
    uint64 [texts, 4] (guide_tallies; the columns above M are not looked at).  -> (the picked records, GUIDE_RECORD
    [regions] -- a region without a candidate keeps its record of rank 1, found = 0 --, their 0-based ranks, their tallies
    as uint64 [regions, 4] with zeros above M)"""
    n, top = shortlist.shape
    M = int(mismatches)
    alive = index >= 0
    t = np.zeros((n, top, 4), dtype=np.uint64)
    t[alive, :M + 1] = np.asarray(tallies, dtype=np.uint64)[index[alive], :M + 1]
    worst = np.uint64(np.iinfo(np.uint64).max)
    for m in range(M + 1):
        col = np.where(alive, t[:, :, m], worst)
        alive &= col == col.min(axis=1, keepdims=True)
    ranks = np.argmax(alive, axis=1)               # (the first slot still alive; 0 where the region has none)
    rows = np.arange(n)
    return shortlist[rows, ranks], ranks.astype(np.int64), t[rows, ranks]


def write_guide_candidates(path, templates, shortlist, index, tallies, ranks, guide_size, mismatches, pam5_len=0, pam3_len=0,
                           regions=None):
    """the TSV of --out_guide_candidates: GUIDE_CANDIDATE_HEADER, then a line per shortlisted candidate -- write_guides'
    columns with the candidate's own rank and tally, and picked = 1 for the region's pick (ranks: pick_guides') --, by
    region, then rank"""
    M = int(mismatches)
    shortlisted = (index >= 0).sum(axis=1)
    with open(path, "w") as f:
        f.write(GUIDE_CANDIDATE_HEADER + "\n")
        for i, (row, slots) in enumerate(zip(templates, shortlist)):
            region = i if regions is None else int(regions[i])
            for j in range(int(shortlisted[i])):
                f.write(_guide_line(row, slots[j], guide_size, pam5_len, pam3_len, region) +
                        f"\t{j + 1}\t{int(shortlisted[i])}\t{_tally_text(tallies[index[i, j], :M + 1])}\t{int(ranks[i] == j)}\n")


# ----------------------------------------------------------------------------
# the picked guides searched in every genome (--out_guide_hits)
# ----------------------------------------------------------------------------
GUIDE_HIT_HEADER = ("region\tfile\trecord\trecord_index\tstart\tend\tstrand\tmismatches\tmismatch_columns\tpam5_match\t"
                    "pam3_match\tsequence")
GUIDE_HIT = np.dtype([("region", "<u4"), ("file", "O"), ("record", "O"), ("record_index", "<i8"), ("start", "<i8"),
                      ("end", "<i8"), ("strand", "U1"), ("mismatches", "<u4"), ("mismatch_columns", "O"), ("pam5_match", "<u4"),
                      ("pam3_match", "<u4"), ("sequence", "O")])


def guide_texts(templates, records, guide_size, regions=None):
    """The table of a guide-hit pass from the regions' template rows (design_templates) and design_guides' records: the
    regions with found = 0 take no part; a region's text is its protospacer as read 5'->3' on the guide's strand
    (template[start, start + guide_size), its reverse complement for strand 1); equal texts are listed once, ordered by
    their bytes.  regions: the number each region is listed under in the --out_guides file (default: its index).
    -> (the distinct texts as bytes, the regions of text t as a list of lists, ascending)"""
    g = guide_size
    by_text = {}
    for i, (row, r) in enumerate(zip(templates, records)):
        if not int(r["found"]):
            continue
        p = int(r["start"])
        t = bytes(row[p:p + g]).decode("ascii")
        if int(r["strand"]):
            t = _guide_rc(t)
        by_text.setdefault(t.encode("ascii"), []).append(i if regions is None else int(regions[i]))
    texts = sorted(by_text)
    return texts, [sorted(by_text[t]) for t in texts]


GUIDE_HIT_MAX_MISMATCHES = 3


GUIDE_HIT_MAX_BULGES = 2
GUIDE_BULGE_MIN_SIZE = 20           # with --guide-hit-bulges: the seeds are the guides' halves, (guide size - bulges) / 2 letters
GUIDE_BULGE_MAX_MISMATCHES = 2      # ... and each is searched within the mismatches: shorter or looser, nearly every window is a seed


def guide_hits_refusal(guide_size, mismatches, pam5, pam3, need_pam, bulges=0):
    """why the guide-hit pass does not take these figures (one line), or None.  bulges: --guide-hit-bulges"""
    if bulges < 0 or bulges > GUIDE_HIT_MAX_BULGES:
        return f"--guide-hit-bulges must lie between 0 and {GUIDE_HIT_MAX_BULGES} (got {bulges})"
    if bulges and guide_size < GUIDE_BULGE_MIN_SIZE:
        return (f"--guide-hit-bulges needs --guide-size >= {GUIDE_BULGE_MIN_SIZE} (got {guide_size}): the bulged search seeds with "
                "half-guides, and halves of fewer than 9 letters lie within the mismatches of nearly every window (DESIGN §20, cost)")
    if bulges and mismatches > GUIDE_BULGE_MAX_MISMATCHES:
        return (f"--guide-hit-bulges needs --guide-hit-mismatches <= {GUIDE_BULGE_MAX_MISMATCHES} (got {mismatches}): a half-guide "
                "within 3 mismatches seeds millions of windows per guide and genome (DESIGN §20, cost)")
    if guide_size < GUIDE_MIN_SIZE or guide_size > GUIDE_MAX_SIZE:
        return f"--guide-size must lie between {GUIDE_MIN_SIZE} and {GUIDE_MAX_SIZE} (got {guide_size})"
    if mismatches < 0 or mismatches > GUIDE_HIT_MAX_MISMATCHES:
        return f"--guide-hit-mismatches must lie between 0 and {GUIDE_HIT_MAX_MISMATCHES} (got {mismatches})"
    for opt, motif in (("--pam5", pam5), ("--pam3", pam3)):
        if len(motif) > GUIDE_MAX_MOTIF:
            return f"{opt} takes at most {GUIDE_MAX_MOTIF} letters (got {motif!r})"
        try:
            motif_masks(motif)
        except ValueError as e:
            return f"{opt}: {e}"
    if need_pam and not pam5 and not pam3:
        return "--guide-hits-need-pam needs a motif: --pam5 or --pam3"
    return None


def guide_hits(texts, text_regions, ingroup_files, outgroup_files, guide_size, mismatches=2, pam5="", pam3="", need_pam=False,
               omit_soft=False, device=0):
    """Every window of every input genome within Hamming distance `mismatches` of a picked guide's protospacer, on both
    strands, wherever it lies: the specificity pass of --out_guides.  texts, text_regions = guide_texts(...):
    the distinct protospacers and the regions that carry each.  A separate pass over the inputs on one device in the manner
    of near_matches (kr_guide_hits_*: the near pass's scan, a per-hit step for the column mask and the motifs).  Returns a
    GUIDE_HIT array: region, file, record, record_index, start, strand as in LOCATION, end = start + guide_size,
    mismatches, mismatch_columns (the 1-based columns that differ, 5'->3' on the guide), pam5_match / pam3_match = 1 where
    the motif lies beside the window as read on the guide's strand (an empty motif matches), sequence = the window on the
    guide's strand.  With need_pam a window counts only where both motifs match.  A hit of a text that several regions
    share is a row for each of them.  Rows in (region, file in command-line order, record_index, start, '+' before '-')
    order.  ValueError for figures the pass does not take (guide_hits_refusal)."""
    why = guide_hits_refusal(guide_size, mismatches, pam5, pam3, need_pam)
    if why is not None:
        raise ValueError(why)
    if len(texts) != len(text_regions):
        raise ValueError(f"guide_hits: {len(texts)} texts, the regions of {len(text_regions)}")
    files = list(ingroup_files) + list(outgroup_files)
    G = guide_size
    if len(texts) == 0:
        return np.empty(0, dtype=GUIDE_HIT)
    t_bytes = _text_matrix(texts, G, "guide_hits")
    parts = []
    for eng, fi, path, rna, names in _scan_genomes(files, 0, G, 0, G, omit_soft, device,
                                                   lambda eng: eng.guide_hits_table(t_bytes, mismatches, pam5, pam3, need_pam)):
        hits = eng.guide_hits(0)
        if len(hits) == 0:
            continue
        rows = eng.guide_hit_windows(G)
        seps, ids = names()
        shared = np.empty(len(hits), dtype=GUIDE_HIT)
        _fill_shared(shared, path, seps, ids, hits["pos"].astype(np.int64), hits["strand"])
        shared["end"] = shared["start"] + G
        _fill_guide_hit(shared, hits)
        shared["sequence"] = _rows_text(rows, G, rna)
        # a hit of text t is a row for every region of t
        rep, region = _fan_out(hits["guide"].astype(np.int64), text_regions)
        part = shared[rep]
        part["region"] = region
        order = np.lexsort((part["strand"] == "-", part["start"], part["record_index"], part["region"]))
        parts.append((fi, part[order], part["region"][order]))
    return _sorted_parts(parts, GUIDE_HIT)


def write_guide_hits(path, rows):
    """the TSV of the guide hits: GUIDE_HIT_HEADER, then a line per row"""
    _write_tsv(path, GUIDE_HIT_HEADER, rows, GUIDE_HIT.names)


GUIDE_BULGE_HIT_HEADER = GUIDE_HIT_HEADER + "\tbulge\tbulge_size\tbulge_column"
GUIDE_BULGE_HIT = np.dtype(GUIDE_HIT.descr + [("bulge", "O"), ("bulge_size", "<u4"), ("bulge_column", "O")])


def guide_bulge_hits(texts, text_regions, ingroup_files, outgroup_files, guide_size, mismatches=2, bulges=1, pam5="", pam3="",
                     need_pam=False, omit_soft=False, device=0):
    """Every window of every input genome that lies within `mismatches` substitutions of a picked guide's protospacer once
    one bulge of 1 .. `bulges` bases is allowed for, on both strands (--guide-hit-bulges): a DNA bulge (the
    genome holds bases the guide has no partner for: the window has guide_size + b bases) or an RNA bulge (guide letters
    have no partner: guide_size - b bases).  One contiguous bulge, never at a guide end; a window's row carries the least
    number of mismatches over the places of the bulge and, of those that reach it, the one nearest the guide's 5' end.
    The arguments and the rows' order are guide_hits'; the unbulged hits are guide_hits' own and no part of the result.
    (kr_guide_bulges_*: the near pass's scan over the guides' halves, a per-pair step that extends each seed.)  Returns a
    GUIDE_BULGE_HIT array: GUIDE_HIT's fields -- end = start + guide_size +- b, mismatch_columns of the aligned columns
    only, sequence = the window on the guide's strand -- and bulge ("DNA" / "RNA"), bulge_size, bulge_column (the
    1-based guide column after which the bulge lies).  Rows in (region, file in command-line order, record_index, start,
    '+' before '-', end) order.  ValueError for figures the pass does not take (guide_hits_refusal)."""
    why = guide_hits_refusal(guide_size, mismatches, pam5, pam3, need_pam, bulges=bulges)
    if why is None and bulges < 1:
        why = f"guide_bulge_hits: bulges is 1 or 2 (got {bulges})"
    if why is not None:
        raise ValueError(why)
    if len(texts) != len(text_regions):
        raise ValueError(f"guide_bulge_hits: {len(texts)} texts, the regions of {len(text_regions)}")
    files = list(ingroup_files) + list(outgroup_files)
    G, W = guide_size, guide_size + bulges
    if len(texts) == 0:
        return np.empty(0, dtype=GUIDE_BULGE_HIT)
    t_bytes = _text_matrix(texts, G, "guide_bulge_hits")
    parts = []
    for eng, fi, path, rna, names in _scan_genomes(files, 0, G, 0, G, omit_soft, device,
                                                   lambda eng: eng.guide_bulges_table(t_bytes, mismatches, bulges, pam5, pam3, need_pam)):
        hits = eng.guide_bulges(0)
        if len(hits) == 0:
            continue
        rows = eng.guide_bulge_windows(W)
        seps, ids = names()
        shared = np.empty(len(hits), dtype=GUIDE_BULGE_HIT)
        _fill_shared(shared, path, seps, ids, hits["pos"].astype(np.int64), hits["strand"])
        length = hits["length"].astype(np.int64)
        shared["end"] = shared["start"] + length
        _fill_guide_hit(shared, hits)
        padded = _rows_text(np.where(rows == 0, np.uint8(ord(" ")), rows), W, rna)
        shared["sequence"] = [t[:n] for t, n in zip(padded, length.tolist())]
        shared["bulge"] = np.where(hits["bulge"] > 0, "DNA", "RNA").astype(object)
        shared["bulge_size"] = np.abs(hits["bulge"].astype(np.int64))
        shared["bulge_column"] = [str(c) for c in hits["bulge_column"].tolist()]
        # a hit of text t is a row for every region of t
        rep, region = _fan_out(hits["guide"].astype(np.int64), text_regions)
        part = shared[rep]
        part["region"] = region
        # (a region's rows at one start and strand differ in their end: G + 1, G - 1, G + 2, G - 2)
        order = np.lexsort((part["end"], part["strand"] == "-", part["start"], part["record_index"], part["region"]))
        parts.append((fi, part[order], part["region"][order]))
    return _sorted_parts(parts, GUIDE_BULGE_HIT)


def write_guide_bulge_hits(path, rows, bulged, files):
    """the TSV of the guide hits under --guide-hit-bulges: GUIDE_BULGE_HIT_HEADER, then guide_hits' rows (with -, 0, - in the
    three bulge columns) and guide_bulge_hits' rows, merged by (region, file in the order of `files`, record_index, start,
    '+' before '-', end)"""
    both = np.empty(len(rows) + len(bulged), dtype=GUIDE_BULGE_HIT)
    head = both[:len(rows)]
    for name in GUIDE_HIT.names:
        head[name] = rows[name]
    head["bulge"] = "-"
    head["bulge_size"] = 0
    head["bulge_column"] = "-"
    both[len(rows):] = bulged
    index = {}
    for i, f_ in enumerate(files):
        index.setdefault(f_, i)
    fidx = np.array([index[f_] for f_ in both["file"]], dtype=np.int64)
    both = both[np.lexsort((both["end"], both["strand"] == "-", both["start"], both["record_index"], fidx, both["region"]))]
    _write_tsv(path, GUIDE_BULGE_HIT_HEADER, both)


# ----------------------------------------------------------------------------
# the guide hits inside the designed primers' products (--out_assay_hits)
# ----------------------------------------------------------------------------
ASSAY_HIT_HEADER = ("region\tfile\trecord\trecord_index\tproduct_start\tproduct_end\tproduct_strand\tlength\tleft_mismatches\t"
                    "right_mismatches\tleft_end_mismatches\tright_end_mismatches\tguide_start\tguide_end\tguide_strand\t"
                    "guide_mismatches\tmismatch_columns\tpam5_match\tpam3_match\torientation\tsequence")
# (start, end, strand: the product's -- the names _fill_shared writes)
ASSAY_HIT = np.dtype([("region", "<u4"), ("file", "O"), ("record", "O"), ("record_index", "<i8"), ("start", "<i8"), ("end", "<i8"),
                      ("strand", "U1"), ("length", "<u4"), ("left_mismatches", "<u4"), ("right_mismatches", "<u4"),
                      ("left_end_mismatches", "<u4"), ("right_end_mismatches", "<u4"), ("guide_start", "<i8"), ("guide_end", "<i8"),
                      ("guide_strand", "U1"), ("guide_mismatches", "<u4"), ("mismatch_columns", "O"), ("pam5_match", "<u4"),
                      ("pam3_match", "<u4"), ("orientation", "O"), ("sequence", "O")])


def assay_links(pairs_regions, text_regions):
    """The links of the assay join: pairs_regions[p] = the regions of primer pair p (primer_pairs), text_regions[t] = the
    regions of guide text t (guide_texts), both in one numbering.  A link is a (p, t) that some region has both of; a
    region with a pair and no guide, or a guide and no pair, makes none.  -> (the links as uint32 [n, 2], strictly
    ascending, the regions of link i as a list of ascending lists)"""
    pair_of = {int(r): p for p, rs in enumerate(pairs_regions) for r in rs}
    by_link = {}
    for t, rs in enumerate(text_regions):
        for r in rs:
            if int(r) in pair_of:
                by_link.setdefault((pair_of[int(r)], t), []).append(int(r))
    keys = sorted(by_link)
    return np.array(keys, dtype=np.uint32).reshape(-1, 2), [sorted(by_link[k]) for k in keys]


def assay_orientation(s_d, s_p, s_h):
    """'design' when a hit on strand s_h of a product on strand s_p lies on the strand of the product that the design put
    the guide on (s_d = the region's guide strand in the --out_guides record), 'reverse' otherwise"""
    return "design" if (int(s_h) ^ int(s_p)) == int(s_d) else "reverse"


def assay_hits_refusal(design_primers, out_guides, amp_size, primer_mismatches, max_product, guide_size, guide_mismatches, pam5, pam3,
                       need_pam):
    """why --out_assay_hits does not run with these options and figures (one line), or None: it needs --design-primers and
    --out_guides, and takes what primer_products_refusal and guide_hits_refusal take"""
    if not design_primers:
        return "--out_assay_hits needs --design-primers (the primer pairs whose products it looks into)"
    if not out_guides:
        return "--out_assay_hits needs --out_guides (the guides it looks for inside the products)"
    why = primer_products_refusal(amp_size, primer_mismatches, max_product)
    if why is None:
        why = guide_hits_refusal(guide_size, guide_mismatches, pam5, pam3, need_pam)
    return why


def assay_hits(left, right, pairs, pairs_regions, texts, text_regions, region_strand, ingroup_files, outgroup_files, guide_size,
               primer_mismatches=1, max_product=1000, guide_mismatches=2, pam5="", pam3="", need_pam=False, omit_soft=False,
               device=0):
    """Where the assay of a region gives a signal: every product of the region's primer pair, in every input
    genome, that carries a window within `guide_mismatches` substitutions of the region's protospacer between its two
    primer sites.  left, right, pairs, pairs_regions = primer_pairs(...); texts, text_regions = guide_texts(...) with the
    regions numbered alike; region_strand[r] = the guide strand of region r in the --out_guides record.  One pass over the
    inputs on one device: the primer table, the guide-hit table and the links stand in ONE locate context, every file is
    uploaded once, scanned by both passes (kr_primers_scan, kr_guide_hits_scan) and their lists are joined by position on
    the device (kr_assay_join); only the assay hits and the windows' text come back.  A product is exactly a product of
    primer_products, a hit exactly a hit of guide_hits (need_pam's selection included; bulged hits take no part).  Returns
    an ASSAY_HIT array: start / end / strand / length and the four mismatch figures are the product's, guide_* and
    mismatch_columns, pam5_match, pam3_match, sequence the hit's, orientation = assay_orientation.  An assay hit of a link
    that several regions share is a row for each.  Rows in (region, file in command-line order, record_index, start, end,
    '+' before '-' for the product, guide_start, '+' before '-' for the guide) order.  ValueError for figures the passes
    do not take."""
    why = primer_products_refusal(None, primer_mismatches, max_product)
    if why is None:
        why = guide_hits_refusal(guide_size, guide_mismatches, pam5, pam3, need_pam)
    if why is None and len(texts) != len(text_regions):
        why = f"assay_hits: {len(texts)} texts, the regions of {len(text_regions)}"
    if why is None and len(pairs) != len(pairs_regions):
        why = f"assay_hits: {len(pairs)} pairs, the regions of {len(pairs_regions)}"
    if why is not None:
        raise ValueError(why)
    G = guide_size
    t_bytes = _text_matrix(texts, G, "assay_hits")
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    _check_max_product(max_product, left, right, pairs)
    links, link_regions = assay_links(pairs_regions, text_regions)
    if len(links) == 0:
        return np.empty(0, dtype=ASSAY_HIT)
    files = list(ingroup_files) + list(outgroup_files)
    link_key = (links[:, 0].astype(np.int64) << 32) | links[:, 1]
    region_strand = np.asarray(region_strand, dtype=np.int64)

    def table(eng):
        eng.primers_table(list(left) + list(right), len(left), pairs, primer_mismatches, max_product)
        eng.guide_hits_table(t_bytes, guide_mismatches, pam5, pam3, need_pam)
        eng.assay_table(links)

    parts = []
    for eng, fi, path, rna, names in _scan_genomes(files, 0, G, 0, G, omit_soft, device, table):
        eng.primers_scan(0)
        eng.guide_hits_scan(0)
        if eng.assay_join(0) == 0:
            continue
        hits = eng.assay_hits()
        text = _rows_text(eng.guide_hit_windows(G)[hits["hit"].astype(np.int64)], G, rna)
        seps, ids = names()
        # an assay hit of link i is a row for every region of i
        li = np.searchsorted(link_key, (hits["pair"].astype(np.int64) << 32) | hits["guide"])
        rep, region = _fan_out(li, link_regions)
        h = hits[rep]
        part = np.empty(len(h), dtype=ASSAY_HIT)
        _fill_shared(part, path, seps, ids, h["pos"].astype(np.int64), h["strand"])
        part["region"] = region
        _fill_product(part, h)
        # (the window lies inside the product: on its record)
        part["guide_start"] = part["start"] + (h["hit_pos"].astype(np.int64) - h["pos"].astype(np.int64))
        part["guide_end"] = part["guide_start"] + G
        part["guide_strand"] = np.where(h["hit_strand"] == 0, "+", "-")
        _fill_guide_hit(part, h, "guide_mismatches", "hit_mismatches", "hit_pam")
        design = (h["hit_strand"].astype(np.int64) ^ h["strand"]) == region_strand[part["region"].astype(np.int64)]
        part["orientation"] = np.where(design, "design", "reverse").astype(object)
        part["sequence"] = text[rep]
        order = np.lexsort((part["guide_strand"] == "-", part["guide_start"], part["strand"] == "-", part["end"], part["start"],
                            part["record_index"], part["region"]))
        parts.append((fi, part[order], part["region"][order]))
    return _sorted_parts(parts, ASSAY_HIT)


def write_assay_hits(path, rows):
    """the TSV of --out_assay_hits: ASSAY_HIT_HEADER, then a line per row"""
    _write_tsv(path, ASSAY_HIT_HEADER, rows, ASSAY_HIT.names)


# ----------------------------------------------------------------------------
# N mutually compatible assays of the designed pairs (--panel)
# ----------------------------------------------------------------------------
PANEL_HEADER = ("member\tregion\tpair_penalty\tproduct_size\tleft_sequence\tright_sequence\tcross_any\tcross_end\t"
                "dropped_same_locus\tdropped_clash")
PANEL_MAX_SIZE = 64


def panel_refusal(design_primers, panel, out_panel, primer3):
    """why --panel / --out_panel are not taken (one line), or None.  panel: the option's value or None; design_primers,
    out_panel, primer3: whether the options are given"""
    if panel is None:
        return "--out_panel needs --panel (the number of assays to pick)" if out_panel else None
    if not design_primers:
        return "--panel needs --design-primers (the primer pairs it picks among)"
    if panel < 1 or panel > PANEL_MAX_SIZE:
        return f"--panel must lie between 1 and {PANEL_MAX_SIZE} (got {panel})"
    if not out_panel:
        return "--panel needs --out_panel (the file the panel is written to)"
    if primer3:
        return "--panel cannot be combined with --primer3 (the pairs Primer3 designs are not compared)"
    return None


def panel_candidates(records, guides=None):
    """The candidates of the panel pass in the order the selection goes by: the regions with a pair (records: design_primers')
    by ascending pair_penalty, then region; with `guides` (a GUIDE_RECORD per region: design_guides' or pick_guides') only
    those that have a guide too, the greater min_mismatches first, then pair_penalty, then region.  -> int64 region indexes"""
    ok = records["found"] != 0
    if guides is not None:
        if len(guides) != len(records):
            raise ValueError(f"panel_candidates: {len(guides)} guides for {len(records)} records")
        ok = ok & (guides["found"] != 0)
    idx = np.flatnonzero(ok).astype(np.int64)
    keys = (idx, records["pair_penalty"][idx].astype(np.int64))
    if guides is not None:
        keys += (-guides["min_mismatches"][idx].astype(np.int64),)
    return idx[np.lexsort(keys)]


def select_panel(templates, records, order, size, device=0, tm=(53, 68), gc=(40, 70), amp_size=(70, 150), primer_size=(25, 35),
                 max_sec_tm=40, gc_clamp=1, max_end_gc=4):
    """The panel of --panel on the device (kr_panel_*): of the candidates `order` (panel_candidates: region
    indexes into the template rows `templates` and design_primers' `records`) the first `size` (1 .. 64) that are different
    loci -- no window of 16 bases shared between two templates, on either strand -- and whose primers' duplex figures with
    the primers of every earlier member stay at `max_sec_tm` or below: member 1 is the first candidate; after every member
    each later candidate still alive is dropped if it is the same locus, else if it clashes; the next member is the first
    still alive.  The primer options are design_primers' (the model's integers and max_sec_tm are what the pass reads).
    -> (_native.PANEL_MEMBER array, in order of acceptance: `position` indexes `order`; _native.PANEL_FATE array, one per
    candidate of `order`).  ValueError for a size outside 1 .. 64 or figures the designer does not take"""
    from . import _native, thermo
    if size < 1 or size > PANEL_MAX_SIZE:
        raise ValueError(f"--panel must lie between 1 and {PANEL_MAX_SIZE} (got {size})")
    opts = dict(tm=tuple(tm), gc=tuple(gc), amp_size=tuple(amp_size), primer_size=tuple(primer_size), max_sec_tm=max_sec_tm,
                gc_clamp=gc_clamp, max_end_gc=max_end_gc)
    why = thermo.refusal(**opts)
    if why is not None:
        raise ValueError(why)
    order = np.asarray(order, dtype=np.int64)
    if len(order) == 0:
        return np.empty(0, dtype=_native.PANEL_MEMBER), np.empty(0, dtype=_native.PANEL_FATE)
    rows = np.ascontiguousarray(templates, dtype=np.uint8)[order]
    pairs = np.stack([records[f][order] for f in ("left_start", "left_len", "right_start", "right_len")], axis=1).astype(np.uint16)
    with _engine(device) as eng:
        eng.design_table(thermo.params(**opts))
        return eng.panel(rows, pairs, size)


def write_panel(path, templates, records, order, members, drops=None):
    """the TSV of --out_panel: PANEL_HEADER, then a line per member in order of acceptance.  templates, records, order as
    select_panel takes them, members: its.  region = the pair's data row in the CSV of --design-primers (the region's rank
    among the regions with a pair); penalty and figures as the CSV prints its own, from the integers.  drops
    (select_panel_clean's): one more column, dropped_cross, behind dropped_clash"""
    from . import thermo
    rank = np.cumsum(records["found"] != 0) - 1
    with open(path, "w") as f:
        f.write(PANEL_HEADER + ("\tdropped_cross" if drops is not None else "") + "\n")
        for j, m in enumerate(members):
            i = int(order[int(m["position"])])
            r = records[i]
            t = bytes(templates[i]).decode("ascii")
            ls, ln, rs, rn = (int(r[k]) for k in ("left_start", "left_len", "right_start", "right_len"))
            f.write(f"{j + 1}\t{int(rank[i])}\t{thermo.milli(int(r['pair_penalty']))}\t{int(r['product_size'])}\t{t[ls:ls + ln]}\t"
                    f"{_guide_rc(t[rs:rs + rn])}\t{thermo.celsius(int(m['cross_any']))}\t{thermo.celsius(int(m['cross_end']))}\t"
                    f"{int(m['dropped'][0])}\t{int(m['dropped'][1])}" + (f"\t{int(drops[1 + j])}" if drops is not None else "") + "\n")


# ----------------------------------------------------------------------------
# a panel without cross and single products in any input genome (--panel-clean)
# ----------------------------------------------------------------------------
def panel_clean_refusal(panel, panel_clean, amp_size, primer_size, mismatches, max_product):
    """why --panel-clean is not taken (one line), or None.  panel: --panel's value or None; panel_clean: whether the option
    is given; mismatches, max_product: the figures after the defaults"""
    if not panel_clean:
        return None
    if panel is None:
        return "--panel-clean needs --panel (the selection it keeps clean)"
    if mismatches < 0 or mismatches > PRODUCT_MAX_MISMATCHES:
        return f"--primer-mismatches must lie between 0 and {PRODUCT_MAX_MISMATCHES} (got {mismatches})"
    if max_product < amp_size[1]:
        return (f"--max-product must be at least the upper bound of --amp_size, {amp_size[1]} bases (got {max_product}): a "
                "member's designed product itself would not be found")
    if max_product < 2 * primer_size[1]:
        return (f"--max-product must be at least twice the upper bound of --primer_size, {2 * primer_size[1]} bases (got "
                f"{max_product}): two primers of the candidates would not fit one product")
    if max_product >= 1 << 31:
        return f"--max-product must be smaller than 2^31 bases (got {max_product})"
    return None


def panel_candidate_texts(templates, records, order):
    """The table of the clean selection: the primer texts of ALL candidates `order`, 5'->3' exactly as write_panel prints
    left_sequence and right_sequence, equal texts once, ordered by their bytes (as panel_texts orders a panel's)
    -> (texts: a list of bytes, rows: uint32 [candidates, 2], the table rows of each candidate's left and right primer)"""
    both = []
    for i in np.asarray(order, dtype=np.int64).tolist():
        r = records[i]
        t = bytes(templates[i]).decode("ascii")
        ls, ln, rs, rn = (int(r[k]) for k in ("left_start", "left_len", "right_start", "right_len"))
        both.append((t[ls:ls + ln].encode("ascii"), _guide_rc(t[rs:rs + rn]).encode("ascii")))
    texts = sorted({x for pair in both for x in pair})
    at = {t: n for n, t in enumerate(texts)}
    rows = np.array([[at[a], at[b]] for a, b in both], dtype=np.uint32).reshape(-1, 2)
    return texts, rows


def select_panel_clean(templates, records, order, size, ingroup_files, outgroup_files, L, R, amplicon_len, mismatches=1,
                       max_product=1000, omit_soft=False, device=0, tm=(53, 68), gc=(40, 70), amp_size=(70, 150),
                       primer_size=(25, 35), max_sec_tm=40, gc_clamp=1, max_end_gc=4):
    """select_panel that reads the genomes (kr_panel_sites_*, kr_panel_run_clean): one pass over the input files
    keeps the sites of ALL candidates' primers (within `mismatches` substitutions, as primer_products finds them) on the
    device, and the selection in the same engine also drops a candidate one of whose primers forms a product of at most
    `max_product` bases with itself (fate 5, before the first round) or, in either order, with a primer of a member (fate 4,
    tested behind same locus and clash).  With the same three figures the --out_panel_products of the result holds `pair`
    rows only.  -> (members, fates, drops): select_panel's two and uint32 [1 + members]: the self-priming candidates, then
    what each member dropped as cross.  ValueError for figures the passes do not take"""
    from . import _native, thermo
    if size < 1 or size > PANEL_MAX_SIZE:
        raise ValueError(f"--panel must lie between 1 and {PANEL_MAX_SIZE} (got {size})")
    opts = dict(tm=tuple(tm), gc=tuple(gc), amp_size=tuple(amp_size), primer_size=tuple(primer_size), max_sec_tm=max_sec_tm,
                gc_clamp=gc_clamp, max_end_gc=max_end_gc)
    why = thermo.refusal(**opts)
    if why is None and (mismatches < 0 or mismatches > PRODUCT_MAX_MISMATCHES):
        why = f"--primer-mismatches must lie between 0 and {PRODUCT_MAX_MISMATCHES} (got {mismatches})"
    if why is None and max_product >= 1 << 31:
        why = f"--max-product must be smaller than 2^31 bases (got {max_product})"
    order = np.asarray(order, dtype=np.int64)
    texts, rows = panel_candidate_texts(templates, records, order)
    if why is None and texts and max_product < 2 * max(len(t) for t in texts):
        why = f"--max-product must be at least twice the longest primer, {2 * max(len(t) for t in texts)} bases (got {max_product})"
    if why is not None:
        raise ValueError(why)
    if len(order) == 0:
        return np.empty(0, dtype=_native.PANEL_MEMBER), np.empty(0, dtype=_native.PANEL_FATE), np.zeros(1, dtype=np.uint32)
    trows = np.ascontiguousarray(templates, dtype=np.uint8)[order]
    pairs = np.stack([records[f][order] for f in ("left_start", "left_len", "right_start", "right_len")], axis=1).astype(np.uint16)
    k = amplicon_len
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    out = []

    def select(eng):
        eng.design_table(thermo.params(**opts))     # (kr_design_table touches no scan state: the store stands)
        out.append(eng.panel_clean(trows, pairs, rows, size))

    for eng, _fi, _path, _rna, _recs in _scan_genomes(list(ingroup_files) + list(outgroup_files), Le, De, Re, k, omit_soft, device,
                                                      lambda eng: eng.panel_sites_table(texts, mismatches, max_product), last=select):
        eng.panel_sites_scan(0)
    return out[0]


# ----------------------------------------------------------------------------
# multiplex in-silico PCR of the panel's oligos in every genome (--out_panel_products, --out_panel_summary)
# ----------------------------------------------------------------------------
PANEL_PRODUCT_HEADER = ("file\trecord\trecord_index\tstart\tend\tlength\tforward\treverse\tkind\tforward_mismatches\t"
                        "reverse_mismatches\tforward_end_mismatches\treverse_end_mismatches")
PANEL_SUMMARY_HEADER = "file\tforward\treverse\tkind\tproducts\tclean_end_products"
# (forward_index, reverse_index: the oligos' indexes, which order the rows; the files do not print them)
PANEL_PRODUCT = np.dtype([("file", "O"), ("record", "O"), ("record_index", "<i8"), ("start", "<i8"), ("end", "<i8"), ("length", "<i8"),
                          ("forward", "O"), ("reverse", "O"), ("kind", "O"), ("forward_mismatches", "u1"), ("reverse_mismatches", "u1"),
                          ("forward_end_mismatches", "u1"), ("reverse_end_mismatches", "u1"), ("forward_index", "<i8"),
                          ("reverse_index", "<i8")])
PANEL_SUMMARY = np.dtype([("file", "O"), ("forward", "O"), ("reverse", "O"), ("kind", "O"), ("products", "<i8"),
                          ("clean_end_products", "<i8"), ("forward_index", "<i8"), ("reverse_index", "<i8")])
PANEL_MAX_OLIGO_TEXTS = 128         # kr_multiplex_table's limit: the distinct texts of 64 members at most
PANEL_MIN_OLIGO, PANEL_MAX_OLIGO = 10, 60


def panel_products_refusal(panel, out_products, out_summary, amp_size, primer_size, mismatches, max_product):
    """why --out_panel_products / --out_panel_summary are not taken (one line), or None.  panel: --panel's value or None;
    out_products, out_summary: whether the options are given; mismatches, max_product: the figures after the defaults"""
    if not (out_products or out_summary):
        return None
    if panel is None:
        return f"{'--out_panel_products' if out_products else '--out_panel_summary'} needs --panel (the oligos it searches for)"
    if mismatches < 0 or mismatches > PRODUCT_MAX_MISMATCHES:
        return f"--primer-mismatches must lie between 0 and {PRODUCT_MAX_MISMATCHES} (got {mismatches})"
    if max_product < amp_size[1]:
        return (f"--max-product must be at least the upper bound of --amp_size, {amp_size[1]} bases (got {max_product}): a "
                "member's designed product itself would not be found")
    if max_product < 2 * primer_size[1]:
        return (f"--max-product must be at least twice the upper bound of --primer_size, {2 * primer_size[1]} bases (got "
                f"{max_product}): two oligos of the panel would not fit one product")
    if max_product >= 1 << 31:
        return f"--max-product must be smaller than 2^31 bases (got {max_product})"
    return None


def panel_oligos(templates, records, order, members):
    """The oligos of a panel in index order, 2 (member - 1) + side with L = 0 and R = 1 -> a list of (name, text): the names
    1L, 1R, 2L, ..., the texts 5'->3' exactly as write_panel prints left_sequence and right_sequence.  templates, records,
    order, members: as write_panel takes them"""
    out = []
    for j, m in enumerate(members):
        i = int(order[int(m["position"])])
        r = records[i]
        t = bytes(templates[i]).decode("ascii")
        ls, ln, rs, rn = (int(r[k]) for k in ("left_start", "left_len", "right_start", "right_len"))
        out.append((f"{j + 1}L", t[ls:ls + ln]))
        out.append((f"{j + 1}R", _guide_rc(t[rs:rs + rn])))
    return out


def panel_kind(i, j):
    """what the product of oligo i (forward) and oligo j (reverse) is: `single` the same oligo twice, `pair` the two oligos
    of one member in either order, `cross` everything else -- an oligo with its twin in another member too"""
    return "single" if i == j else "pair" if i // 2 == j // 2 else "cross"


def panel_texts(oligos):
    """the table of the multiplex pass: equal texts once, ordered by their bytes -> (texts, owners): owners[t] = the indexes
    of the oligos whose text is texts[t], ascending"""
    texts = sorted({text.encode("ascii") for _, text in oligos})
    at = {t: n for n, t in enumerate(texts)}
    owners = [[] for _ in texts]
    for i, (_, text) in enumerate(oligos):
        owners[at[text.encode("ascii")]].append(i)
    return texts, owners


def _panel_fan_out(fwd, rev, owners):
    """a product of the texts (fwd, rev) is a row for every oligo of fwd with every oligo of rev -> (rep, forward oligo,
    reverse oligo): output row j repeats product rep[j]"""
    rep, fi = _fan_out(fwd, owners)
    rep2, ri = _fan_out(rev[rep], owners)
    return rep[rep2], fi[rep2].astype(np.int64), ri.astype(np.int64)


def panel_products(oligos, ingroup_files, outgroup_files, L, R, amplicon_len, mismatches=1, max_product=1000, omit_soft=False,
                   device=0, rows=True):
    """Multiplex in-silico PCR: with all the oligos of a panel (panel_oligos) in one tube, what do they amplify
    in every input genome?  Every oligo can open a product and every oligo can close one: a site is primer_products' site, a
    product is a site of the forward oligo as written and, downstream on the same record and not overlapping it, a site of
    the reverse oligo's reverse complement, at most `max_product` bases from end to end.  One pass over the inputs on one
    device (kr_multiplex_*).  -> (PANEL_PRODUCT array, PANEL_SUMMARY array): the rows by file in the order given,
    record_index, start, end, forward oligo, reverse oligo; the summary -- a row per file and ordered oligo pair with a
    product, from the device's tally -- by file, forward, reverse.  An oligo's text that several oligos share gives a row
    for each of them.  rows=False: no product comes to the host, the first array is empty.  ValueError for figures the pass
    does not take"""
    why = None
    if mismatches < 0 or mismatches > PRODUCT_MAX_MISMATCHES:
        why = f"--primer-mismatches must lie between 0 and {PRODUCT_MAX_MISMATCHES} (got {mismatches})"
    elif max_product >= 1 << 31:
        why = f"--max-product must be smaller than 2^31 bases (got {max_product})"
    for name, text in oligos:
        if why is None and not (PANEL_MIN_OLIGO <= len(text) <= PANEL_MAX_OLIGO and set(text) <= set("ACGT")):
            why = f"panel_products: oligo {name} is not {PANEL_MIN_OLIGO} .. {PANEL_MAX_OLIGO} letters of A, C, G, T"
        elif why is None and max_product < 2 * len(text):
            why = f"--max-product must be at least twice the longest oligo, {2 * len(text)} bases (got {max_product})"
    texts, owners = panel_texts(oligos)
    if why is None and len(texts) > PANEL_MAX_OLIGO_TEXTS:
        why = f"panel_products: {len(texts)} distinct oligos (the limit is {PANEL_MAX_OLIGO_TEXTS})"
    if why is not None:
        raise ValueError(why)
    if not texts:
        return np.empty(0, dtype=PANEL_PRODUCT), np.empty(0, dtype=PANEL_SUMMARY)
    files = list(ingroup_files) + list(outgroup_files)
    k = amplicon_len
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    names = np.array([name for name, _ in oligos], dtype=object)
    kinds = np.array([[panel_kind(i, j) for j in range(len(oligos))] for i in range(len(oligos))], dtype=object)
    parts, sums = [], []
    for eng, fi, path, _rna, recs in _scan_genomes(files, Le, De, Re, k, omit_soft, device,
                                                   lambda eng: eng.multiplex_table(texts, mismatches, max_product)):
        hits = eng.multiplex_products(0) if rows else None
        if (len(hits) if rows else eng.multiplex_scan(0)) == 0:
            continue
        tally = eng.multiplex_tally()
        a, b = np.nonzero(tally.sum(axis=2))
        rep, fo, ro = _panel_fan_out(a.astype(np.int64), b.astype(np.int64), owners)
        part = np.empty(len(rep), dtype=PANEL_SUMMARY)
        part["file"] = path
        part["forward_index"], part["reverse_index"] = fo, ro
        part["forward"], part["reverse"], part["kind"] = names[fo], names[ro], kinds[fo, ro]
        part["products"] = tally[a, b].sum(axis=1)[rep]
        part["clean_end_products"] = tally[a, b, 1][rep]
        sums.append(part[np.lexsort((ro, fo))])
        if not rows:
            continue
        seps, ids = recs()
        rep, fo, ro = _panel_fan_out(hits["fwd"].astype(np.int64), hits["rev"].astype(np.int64), owners)
        hits = hits[rep]
        part = np.empty(len(hits), dtype=PANEL_PRODUCT)
        ri, start = _record_coords(seps, hits["pos"].astype(np.int64))
        part["file"] = path
        part["record"] = np.asarray(ids, dtype=object)[ri]
        part["record_index"], part["start"], part["length"] = ri, start, hits["length"]
        part["end"] = part["start"] + part["length"]
        part["forward_index"], part["reverse_index"] = fo, ro
        part["forward"], part["reverse"], part["kind"] = names[fo], names[ro], kinds[fo, ro]
        for side, src in (("forward", "fwd"), ("reverse", "rev")):
            part[side + "_mismatches"] = hits[src + "_mm"]
            part[side + "_end_mismatches"] = hits[src + "_end_mm"]
        # (positions ascend with (record_index, start); a position's rows by end, then by the oligos)
        parts.append(part[np.lexsort((ro, fo, hits["length"], hits["pos"]))])
    return (np.concatenate(parts) if parts else np.empty(0, dtype=PANEL_PRODUCT),
            np.concatenate(sums) if sums else np.empty(0, dtype=PANEL_SUMMARY))


def write_panel_products(path, rows):
    """the TSV of --out_panel_products: PANEL_PRODUCT_HEADER, then panel_products' rows"""
    _write_tsv(path, PANEL_PRODUCT_HEADER, rows, PANEL_PRODUCT_HEADER.split("\t"))


def write_panel_summary(path, summary):
    """the TSV of --out_panel_summary: PANEL_SUMMARY_HEADER, then panel_products' summary"""
    _write_tsv(path, PANEL_SUMMARY_HEADER, summary, PANEL_SUMMARY_HEADER.split("\t"))

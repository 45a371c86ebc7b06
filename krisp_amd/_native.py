"""ctypes binding of libkrisp_hip.so (include/krisp_hip.h).

There is NO fallback: if the shared library is missing or a call fails this
module raises.  The host layer never computes k-mers, sorts or intersects on
the CPU.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# KRISP_HIP_LIB: another build of the same library (A/B variants of tools/ab.sh); the product file
# is never overwritten by a variant
LIB_PATH = os.environ.get("KRISP_HIP_LIB") or os.path.join(HERE, "libkrisp_hip.so")

CAND = np.dtype([("prefix", "<u8"), ("in_mask", "<u8"), ("out_mask", "<u8")])
RECORD = np.dtype([("key", "<u8"), ("genome", "<u4"), ("count", "<u4")])
WIDE_HIT = np.dtype([("cand", "<u4"), ("genome", "<u4"), ("pos", "<u4"), ("strand", "<u4")])
LOC_HIT = np.dtype([("group", "<u4"), ("strand", "<u4"), ("pos", "<u8")])     # kr_loc_hit
NEAR_HIT = np.dtype([("target", "<u4"), ("strand", "u1"), ("mismatches", "u1"), ("flank_mismatches", "u1"), ("pad", "u1"),
                     ("pos", "<u8")])                                          # kr_near_hit
PRODUCT_SITE = np.dtype([("pos", "<u8"), ("entry", "<u4"), ("mismatches", "u1"), ("end_mismatches", "u1"),
                         ("pad", "<u2")])                                      # kr_product_site
PRODUCT_HIT = np.dtype([("pos", "<u8"), ("length", "<u4"), ("pair", "<u4"), ("strand", "u1"), ("left_mm", "u1"),
                        ("right_mm", "u1"), ("left_end_mm", "u1"), ("right_end_mm", "u1"), ("pad", "u1", (3,))])   # kr_product_hit
MULTIPLEX_HIT = np.dtype([("pos", "<u8"), ("length", "<u4"), ("fwd", "<u2"), ("rev", "<u2"), ("fwd_mm", "u1"), ("rev_mm", "u1"),
                          ("fwd_end_mm", "u1"), ("rev_end_mm", "u1"), ("pad", "u1", (4,))])                 # kr_multiplex_hit
DESIGN_RECORD = np.dtype([("found", "<u4"), ("product_size", "<u4"), ("pair_penalty", "<u4"), ("left_start", "<u2"),
                          ("left_len", "<u2"), ("right_start", "<u2"), ("right_len", "<u2"), ("left_tm", "<i4"), ("right_tm", "<i4"),
                          ("left_gc", "<u2"), ("right_gc", "<u2"), ("left_penalty", "<u4"), ("right_penalty", "<u4"),
                          ("left_self_any", "<i4"), ("left_self_end", "<i4"), ("right_self_any", "<i4"),
                          ("right_self_end", "<i4"), ("pair_any", "<i4"), ("pair_end", "<i4")])             # kr_design_record
# ... and, behind it, the pair's two figures of kr_design_fetch_hairpins: what Engine.design returns with the check on
DESIGN_RECORD_HP = np.dtype(DESIGN_RECORD.descr + [("left_hairpin", "<i4"), ("right_hairpin", "<i4")])
PANEL_MEMBER = np.dtype([("position", "<u4"), ("cross_any", "<i4"), ("cross_end", "<i4"), ("dropped", "<u4", (2,))])  # kr_panel_member
PANEL_FATE = np.dtype([("fate", "u1"), ("by", "u1")])                         # kr_panel_fates: two bytes a candidate
GUIDE_RECORD = np.dtype([("found", "<u4"), ("strand", "<u4"), ("start", "<u4"), ("min_mismatches", "<u4"),
                         ("sum_mismatches", "<u4"), ("gc", "<u4"), ("candidates", "<u4"), ("pad", "<u4")])    # kr_guide_record
GUIDE_HIT_RAW = np.dtype([("guide", "<u4"), ("strand", "u1"), ("mismatches", "u1"), ("pam", "u1"), ("pad", "u1"), ("pos", "<u8"),
                          ("columns", "<u8")])                                 # kr_guide_hit
ASSAY_HIT_RAW = np.dtype([("pos", "<u8"), ("length", "<u4"), ("pair", "<u4"), ("strand", "u1"), ("left_mm", "u1"), ("right_mm", "u1"),
                          ("left_end_mm", "u1"), ("right_end_mm", "u1"), ("hit_strand", "u1"), ("hit_mismatches", "u1"),
                          ("hit_pam", "u1"), ("hit_pos", "<u8"), ("columns", "<u8"), ("guide", "<u4"), ("hit", "<u4")])   # kr_assay_hit
GUIDE_BULGE_HIT_RAW = np.dtype([("guide", "<u4"), ("strand", "u1"), ("mismatches", "u1"), ("pam", "u1"), ("bulge", "i1"),
                                ("pos", "<u8"), ("columns", "<u8"), ("bulge_column", "<u4"), ("length", "<u4")])   # kr_guide_bulge_hit
WIDE_DICT_LEFT, WIDE_DICT_RIGHT, WIDE_GROUPS, WIDE_HITS, WIDE_COUNTS, WIDE_SLOT_BITS, WIDE_NGROUPS, WIDE_BATCH_USED, WIDE_LOCATED, WIDE_KEYS_LISTED = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
WIDE_MAX_K = 1024
WIDE_MAX_FLANK = 256
COMM_ID_BYTES = 128

SOFT_MAP, SOFT_OMIT = 0, 1
OPT_SLICE_BASES, OPT_GENERIC_INTERSECT, OPT_ISECT_FORMAT, OPT_ABLATE, OPT_WIDE_SLOTS, OPT_WIDE_ORDERED, OPT_PLACE_TRIES = 1, 2, 3, 4, 5, 6, 7
OPT_ISECT_KERNEL = 8
OPT_LANES = 9
OPT_LAZY_ORDER = 10
OPT_COARSE_REST = 11
OPT_COARSE_POOL = 12
OPT_JOIN2 = 13
OPT_COARSE_ONE_STRAND = 14
OPT_COARSE_ONE_PASS = 15
OPT_JOIN2_DENSE = 16
ERR_KEY, ERR_HOST = -5, -6
STRANDS_BOTH, STRANDS_FORWARD, STRANDS_CANONICAL = 0, 1, 2
STAGES = ["pack", "hist8", "reduce8", "scatter1", "hist2", "scan2", "scatter2", "chunks", "localsort",
          "fallback", "intersect", "compact", "collect", "merge", "locate"]
# stage -> the kernel(s) it times (names as rocprofv3 prints them)
STAGE_KERNELS = {"pack": "k_pack", "hist8": "k_hist8 (wide path: k_hist8w, slices: k_hist8k)", "reduce8": "k_reduce8a+k_reduce8b",
                 "scatter1": "k_scatter1p (wide path: k_scatter1w, slices: k_scatter1kp)",
                 "hist2": "k_hist16 (or k_hist2)", "scan2": "k_hist16_off (or k_scan2)", "scatter2": "k_scatter2",
                 "chunks": "k_chunk_table", "localsort": "k_localsort2",
                 "fallback": "k_seg_merge", "intersect": "k_intersect3 (+ k_intersect for oversized items)",
                 "compact": "k_scan+k_publish_reset+k_gather_items",
                 "collect": "k_collect_count+k_tile_sums+k_scan+k_tile_apply+k_publish+k_collect_emit",
                 "merge": "k_cands_flag+k_scan+k_cands_compact", "locate": "k_wide_locate"}

# every symbol include/krisp_hip.h declares: (name, restype, argtypes)
_c = ctypes
_P = _c.c_void_p
SYMBOLS = [
    ("kr_create", _P, [_c.c_int, _c.c_size_t]),
    ("kr_destroy", None, [_P]),
    ("kr_last_error", _c.c_char_p, [_P]),
    ("kr_set_params", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_size_t]),
    ("kr_set_strands", _c.c_int, [_P, _c.c_int]),
    ("kr_genome_upload", _c.c_int, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_genome_sort", _c.c_int, [_P, _c.c_int]),
    ("kr_genome_partition", _c.c_int, [_P, _c.c_int]),
    ("kr_genome_add", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_genome_count", _c.c_int64, [_P, _c.c_int]),
    ("kr_genome_load_sorted", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_genome_fetch_keys", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_genome_keys_in_order", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_set_allow", _c.c_int, [_P, _c.c_uint]),
    ("kr_set_field_order", _c.c_int, [_P, _P, _P]),
    ("kr_set_field_pieces", _c.c_int, [_P, _c.c_int, _P, _P]),
    ("kr_genome_free", _c.c_int, [_P, _c.c_int]),
    ("kr_intersect", _c.c_int64, [_P, _P, _c.c_int, _P, _c.c_int]),
    ("kr_cands_count", _c.c_int64, [_P]),
    ("kr_cands_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_cands_load", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_cands_merge", _c.c_int64, [_P, _P, _c.c_size_t, _c.c_int, _c.c_int]),
    ("kr_cands_probe", _c.c_int64, [_P, _P, _c.c_int, _P, _c.c_int]),
    ("kr_comm_unique_id", _c.c_int, [_P]),
    ("kr_comm_init", _c.c_int, [_P, _c.c_int, _c.c_int, _P]),
    ("kr_comm_init_dir", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_char_p]),
    ("kr_comm_destroy", _c.c_int, [_P]),
    ("kr_comm_rank", _c.c_int, [_P]),
    ("kr_comm_world", _c.c_int, [_P]),
    ("kr_comm_rccl_ranks", _c.c_int, [_P]),
    ("kr_comm_barrier", _c.c_int, [_P]),
    ("kr_comm_allreduce", _c.c_int, [_P, _P, _c.c_int, _c.c_int]),
    ("kr_comm_allgather", _c.c_int, [_P, _P, _c.c_size_t, _P]),
    ("kr_cands_reduce", _c.c_int64, [_P, _c.c_int]),
    ("kr_cands_bcast", _c.c_int64, [_P]),
    ("kr_records_gather", _c.c_int64, [_P]),
    ("kr_collect", _c.c_int64, [_P, _P, _c.c_int]),
    ("kr_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_set_params_wide", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_size_t]),
    ("kr_wide_run", _c.c_int64, [_P, _P, _c.c_int, _P, _c.c_int]),
    ("kr_wide_fetch", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_wide_fetch_windows", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_set_params_locate", _c.c_int, [_P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_size_t]),
    ("kr_locate_table", _c.c_int64, [_P, _P, _c.c_uint64]),
    ("kr_locate_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_locate_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_locate_windows", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_locate_seps", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_near_table", _c.c_int64, [_P, _P, _c.c_uint64, _c.c_int]),
    ("kr_near_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_near_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_near_windows", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_products_table", _c.c_int64, [_P, _P, _c.c_uint64, _P, _c.c_uint64, _P, _c.c_uint64, _c.c_int, _c.c_uint32]),
    ("kr_products_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_products_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_products_sites", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_primers_table", _c.c_int64, [_P, _P, _P, _c.c_uint64, _c.c_uint64, _P, _c.c_uint64, _c.c_int, _c.c_uint32]),
    ("kr_primers_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_primers_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_primers_sites", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_design_table", _c.c_int, [_P, _P]),
    ("kr_design_run", _c.c_int64, [_P, _P, _c.c_uint64, _c.c_int, _c.c_int, _c.c_int]),
    ("kr_design_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_design_hairpins", _c.c_int, [_P, _P]),
    ("kr_design_fetch_hairpins", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_design_run_top", _c.c_int64, [_P, _P, _c.c_uint64, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    ("kr_design_fetch_top", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_design_fetch_top_hairpins", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_primers_tally", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_panel_run", _c.c_int64, [_P, _P, _P, _c.c_uint64, _c.c_int, _c.c_int]),
    ("kr_panel_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_panel_fates", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_panel_sites_table", _c.c_int64, [_P, _P, _P, _c.c_uint64, _c.c_int, _c.c_uint32]),
    ("kr_panel_sites_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_panel_sites_fetch", _c.c_int64, [_P, _P, _P, _c.c_size_t]),
    ("kr_panel_run_clean", _c.c_int64, [_P, _P, _P, _P, _c.c_uint64, _c.c_int, _c.c_int]),
    ("kr_panel_clean_drops", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guides_table", _c.c_int, [_P, _P]),
    ("kr_guides_run", _c.c_int64, [_P, _P, _P, _P, _c.c_uint64, _c.c_int, _c.c_int, _c.c_int]),
    ("kr_guides_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guides_run_top", _c.c_int64, [_P, _P, _P, _P, _c.c_uint64, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    ("kr_guides_fetch_top", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guide_hits_table", _c.c_int64, [_P, _P, _c.c_uint64, _c.c_int, _c.c_char_p, _c.c_char_p, _c.c_int]),
    ("kr_guide_hits_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_guide_hits_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guide_hits_windows", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guide_hits_tally", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_multiplex_table", _c.c_int64, [_P, _P, _P, _c.c_uint64, _c.c_int, _c.c_uint32]),
    ("kr_multiplex_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_multiplex_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_multiplex_sites", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_multiplex_tally", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guide_bulges_table", _c.c_int64, [_P, _P, _c.c_uint64, _c.c_int, _c.c_int, _c.c_char_p, _c.c_char_p, _c.c_int]),
    ("kr_guide_bulges_scan", _c.c_int64, [_P, _c.c_int]),
    ("kr_guide_bulges_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_guide_bulges_windows", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_assay_table", _c.c_int64, [_P, _P, _c.c_uint64]),
    ("kr_assay_join", _c.c_int64, [_P, _c.c_int]),
    ("kr_assay_fetch", _c.c_int64, [_P, _P, _c.c_size_t]),
    ("kr_render_windows", _c.c_int64, [_P, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _P, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P,
                                       _c.c_int, _c.c_int, _P, _P, _P, _P]),
    ("kr_fasta_to_bases", _c.c_int64, [_P, _c.c_size_t, _c.c_int, _c.c_int, _P, _c.c_size_t, _P]),
    ("kr_ingest_file", _c.c_int64, [_c.c_char_p, _P, _P]),
    ("kr_read_file", _c.c_int64, [_c.c_char_p, _P, _P]),
    ("kr_genome_upload_text", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t, _c.c_int, _c.c_int, _P]),
    ("kr_genome_upload_bgzf", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t, _c.c_int, _P]),
    ("kr_genome_upload_gzip", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t, _c.c_size_t, _c.c_int, _P]),
    ("kr_reserve", _c.c_int, [_P, _P, _c.c_int, _c.c_size_t, _c.c_int]),
    ("kr_genome_fetch_bases", _c.c_int64, [_P, _c.c_int, _P, _c.c_size_t]),
    ("kr_host_free", None, [_P]),
    ("kr_scan_special", _c.c_int64, [_P, _c.c_size_t, _c.c_int, _c.c_int, _P, _c.c_size_t, _P]),
    ("kr_set_option", _c.c_int, [_P, _c.c_int, _c.c_int64]),
    ("kr_sync", _c.c_int, [_P]),
    ("kr_timer_begin", _c.c_int, [_P]),
    ("kr_timer_end_ms", _c.c_double, [_P]),
    ("kr_stage_enable", _c.c_int, [_P, _c.c_int]),
    ("kr_stage_select", _c.c_int, [_P, _c.c_uint]),
    ("kr_stage_reset", _c.c_int, [_P]),
    ("kr_stage_ms", _c.c_double, [_P, _c.c_int]),
    ("kr_stage_launches", _c.c_int64, [_P, _c.c_int]),
    ("kr_debug_fetch", _c.c_int64, [_P, _c.c_int, _c.c_int, _P, _c.c_size_t]),
    ("kr_debug_inversions", _c.c_int64, [_P, _c.c_int]),
    ("kr_debug_localsort", _c.c_double, [_P, _c.c_int, _c.c_int, _c.c_int]),
    ("kr_debug_intersect", _c.c_double, [_P, _P, _c.c_int, _P, _c.c_int, _c.c_int]),
    ("kr_debug_copy_gbps", _c.c_double, [_P, _c.c_size_t, _c.c_int]),
    ("kr_debug_copy_which", _c.c_char_p, [_P]),
    ("kr_mem_info", _c.c_int, [_P, _P]),
    ("kr_debug_comm", _c.c_int, [_P, _P]),
    ("kr_debug_place", _c.c_int, [_P, _P]),
    ("kr_debug_coarse_pool", _c.c_int, [_P, _P]),
    ("kr_debug_coarse_strand", _c.c_int, [_P, _P]),
    ("kr_debug_comm_probe", _c.c_int, [_P, _c.c_size_t, _c.c_int, _P]),
    ("kr_debug_cands_selfexchange", _c.c_int64, [_P, _c.c_int]),
    ("kr_debug_info", _c.c_int, [_P, _P]),
    ("kr_render_records", _c.c_int64, [_P, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_size_t, _P, _c.c_size_t, _P,
                                       _c.c_int, _P, _P, _P, _P]),
    ("kr_text_free", None, [_P]),
    ("kr_debug_isect", _c.c_int, [_P, _P]),
    ("kr_debug_lazy", _c.c_int, [_P, _P]),
    ("kr_debug_scan", _c.c_int, [_P, _P]),
    ("kr_set_mixed_alphabets", _c.c_int, [_P, _c.c_int]),
    ("kr_build_experiments", _c.c_int, []),
    ("kr_comm_set_timeout", _c.c_int, [_P, _c.c_int]),
    ("kr_debug_comm_hang", _c.c_int, [_P]),
    ("kr_debug_budget_left", _c.c_int64, [_P]),
    ("kr_debug_budget_set", _c.c_int, [_P, _c.c_int64]),
]


class GuideParams(ctypes.Structure):
    """kr_guide_params: pam5 / pam3 hold a 4-bit IUPAC mask per motif letter (A = 1, C = 2, G = 4, T = 8)"""
    _fields_ = [("guide_size", _c.c_int32), ("pam5_len", _c.c_int32), ("pam3_len", _c.c_int32), ("pam5", _c.c_uint8 * 8),
                ("pam3", _c.c_uint8 * 8), ("gc_lo", _c.c_int32), ("gc_hi", _c.c_int32), ("min_mismatches", _c.c_int32)]


class KrispHipError(RuntimeError):
    """a negative return code of the library with kr_last_error's text; `.code` = the KR_ERR_* value (-3 = capacity:
    a caller buffer, the context's HBM budget or the device's memory does not hold what was asked for)"""
    code = None


ERR_CAPACITY = -3


_lib = None


def load():
    """Load the HIP library; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KrispHipError(
            f"{LIB_PATH} is missing: build it with `python -m krisp_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _motif_bytes(m):
    """a PAM / PFS motif as the guide tables take it"""
    return m if isinstance(m, bytes) else str(m).encode("ascii", "replace")


def fasta_to_bases(data, universal_newlines, one_shot=True):
    """bytes of a FASTA / sequence file -> (uint8 upload buffer, records, special chars, rna, fasta)
    through the library's one-pass host parser (GIL released: callers may use threads)."""
    lib = load()
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(len(src) + 1, dtype=np.uint8)
    stats = np.zeros(4, dtype=np.int64)
    n = lib.kr_fasta_to_bases(_ptr(src) if len(src) else None, len(src), 1 if universal_newlines else 0,
                              1 if one_shot else 0, _ptr(out), len(out), _ptr(stats))
    if n < 0:
        raise KrispHipError(f"kr_fasta_to_bases: [{n}]")
    return out[:n], int(stats[0]), int(stats[1]), stats[2] == 1, bool(stats[3])


class _HostBlock:
    """a buffer the library owns (kr_ingest_file: pinned host memory on a GPU box); freed with the last view"""

    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def __del__(self):
        try:
            if self.ptr:
                self.lib.kr_host_free(self.ptr)
                self.ptr = None
        except Exception:  # noqa: BLE001
            pass


def ingest_file(path):
    """file -> (uint8 upload buffer in library-owned, pinned memory; records; special chars; rna; fasta;
    timings dict) through kr_ingest_file: read + inflate + parse inside the library, GIL released.
    Returns None for files the library leaves to the host layer (.bz2)."""
    lib = load()
    out = ctypes.c_void_p(0)
    stats = np.zeros(8, dtype=np.int64)
    n = lib.kr_ingest_file(os.fsencode(path), ctypes.byref(out), _ptr(stats))
    if n == ERR_HOST:
        return None
    if n < 0:
        msg = lib.kr_last_error(None).decode()
        if "cannot open" in msg:
            raise FileNotFoundError(msg)
        raise KrispHipError(f"kr_ingest_file({path}): [{n}] {msg}")
    block = _HostBlock(lib, out.value)
    raw = (ctypes.c_uint8 * max(int(n), 1)).from_address(out.value)
    raw._owner = block                       # the view keeps the block alive
    arr = np.frombuffer(raw, dtype=np.uint8)[:n]
    timings = dict(read_s=stats[4] / 1e6, inflate_s=stats[5] / 1e6, parse_s=stats[6] / 1e6,
                   members=int(stats[7] & 0xFFFFFFFF), libdeflate=bool(stats[7] >> 32))
    return arr, int(stats[0]), int(stats[1]), stats[2] == 1, bool(stats[3]), timings


def read_file(path):
    """file -> (its text as a uint8 view of library-owned, pinned memory; universal_newlines; timings) through
    kr_read_file: read + inflate inside the library, GIL released; the parse is left to the device
    (Engine.upload_text).  None for files the library leaves to the host layer (.bz2)."""
    lib = load()
    out = ctypes.c_void_p(0)
    stats = np.zeros(8, dtype=np.int64)
    n = lib.kr_read_file(os.fsencode(path), ctypes.byref(out), _ptr(stats))
    if n == ERR_HOST:
        return None
    if n < 0:
        msg = lib.kr_last_error(None).decode()
        if "cannot open" in msg:
            raise FileNotFoundError(msg)
        raise KrispHipError(f"kr_read_file({path}): [{n}] {msg}")
    block = _HostBlock(lib, out.value)
    raw = (ctypes.c_uint8 * max(int(n), 1)).from_address(out.value)
    raw._owner = block
    arr = np.frombuffer(raw, dtype=np.uint8)[:n]
    timings = dict(read_s=stats[4] / 1e6, inflate_s=stats[5] / 1e6, copy_s=stats[6] / 1e6,
                   members=int(stats[7] & 0xFFFFFFFF), libdeflate=bool(stats[7] >> 32))
    return arr, bool(stats[3]), timings


def render_records(records, label_of, label_text, label_in, L, D, R, dot=False):
    """kr_render_records: (csv_text, alignment_text, number of groups), or None when the library leaves a group to
    the general path.  records: RECORD array ordered by (key, label id); label_of: genome id -> label id;
    label_text: the distinct labels in string order; label_in: per label 1 / 0, or None (no outgroup given)."""
    lib = load()
    recs = np.ascontiguousarray(records, dtype=RECORD)
    lof = np.ascontiguousarray(label_of, dtype=np.uint32)
    texts = [t.encode("utf-8", "surrogateescape") for t in label_text]     # (labels come from file names)
    arr = (_c.c_char_p * max(len(texts), 1))(*texts)
    lin = None if label_in is None else np.ascontiguousarray(label_in, dtype=np.uint8)
    csv, align = _c.c_void_p(), _c.c_void_p()
    ncsv, nalign = _c.c_size_t(), _c.c_size_t()
    rc = lib.kr_render_records(_ptr(recs), len(recs), L, D, R, _ptr(lof), len(lof), arr, len(texts),
                               None if lin is None else _ptr(lin), 1 if dot else 0, _c.byref(csv), _c.byref(ncsv),
                               _c.byref(align), _c.byref(nalign))
    if rc == ERR_HOST:
        return None
    if rc < 0:
        raise KrispHipError(f"kr_render_records: [{rc}]")
    try:
        return (_c.string_at(csv, ncsv.value).decode("utf-8", "surrogateescape"),
                _c.string_at(align, nalign.value).decode("utf-8", "surrogateescape"), int(rc))
    finally:
        lib.kr_text_free(csv)
        lib.kr_text_free(align)


def render_windows(rows, cand, genome, label_of, label_text, label_in, L, D, R, dot=False, rna=False):
    """kr_render_windows: (csv_text, alignment_text, number of groups) from the member windows of long amplicons (rows:
    uint8 [n, L+D+R] in line order, cand / genome per row as kr_wide_fetch(HITS) gives them), or None when the library
    leaves a group to the general path"""
    lib = load()
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    cand = np.ascontiguousarray(cand, dtype=np.uint32)
    gen = np.ascontiguousarray(genome, dtype=np.uint32)
    lof = np.ascontiguousarray(label_of, dtype=np.uint32)
    texts = [t.encode("utf-8", "surrogateescape") for t in label_text]
    arr = (_c.c_char_p * max(len(texts), 1))(*texts)
    lin = None if label_in is None else np.ascontiguousarray(label_in, dtype=np.uint8)
    csv, align = _c.c_void_p(), _c.c_void_p()
    ncsv, nalign = _c.c_size_t(), _c.c_size_t()
    rc = lib.kr_render_windows(_ptr(rows) if len(rows) else None, len(rows), L, D, R, _ptr(cand) if len(rows) else None,
                               _ptr(gen) if len(rows) else None, _ptr(lof), len(lof), arr, len(texts),
                               None if lin is None else _ptr(lin), 1 if dot else 0, 1 if rna else 0, _c.byref(csv),
                               _c.byref(ncsv), _c.byref(align), _c.byref(nalign))
    if rc == ERR_HOST:
        return None
    if rc < 0:
        raise KrispHipError(f"kr_render_windows: [{rc}]")
    try:
        return (_c.string_at(csv, ncsv.value).decode("utf-8", "surrogateescape"),
                _c.string_at(align, nalign.value).decode("utf-8", "surrogateescape"), int(rc))
    finally:
        lib.kr_text_free(csv)
        lib.kr_text_free(align)


def _quiet_rccl():
    """RCCL prints its version banner (NCCL_DEBUG=VERSION, what some boxes export) and its warnings on STDOUT -- where the
    command line writes its CSV and bench.py its one JSON line: errors only, unless the caller asked for more than the banner"""
    if os.environ.get("NCCL_DEBUG", "VERSION").upper() == "VERSION":
        os.environ["NCCL_DEBUG"] = "ERROR"


def comm_unique_id():
    """the RCCL unique id (rank 0 makes it, every rank passes it to Engine.comm_init)"""
    _quiet_rccl()
    lib = load()
    buf = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
    rc = lib.kr_comm_unique_id(_ptr(buf))
    if rc < 0:
        raise KrispHipError(f"kr_comm_unique_id: [{rc}] " + lib.kr_last_error(None).decode())
    return buf.tobytes()


def scan_special_starts(bases, k, omit_soft):
    """Window starts (ascending) of the surviving, N-free windows that hold an IUPAC ambiguity letter
    (kr_scan_special).  Raises KeyError(char) exactly where the reference does; returns None when the
    library leaves the case to the host (bytes >= 0x80 near a special character)."""
    lib = load()
    buf = np.ascontiguousarray(bases, dtype=np.uint8)
    bad = ctypes.c_int(0)
    n = lib.kr_scan_special(_ptr(buf) if len(buf) else None, len(buf), k, 1 if omit_soft else 0, None, 0,
                            ctypes.byref(bad))
    if n == ERR_KEY:
        raise KeyError(chr(bad.value))
    if n == ERR_HOST:
        return None
    if n < 0:
        raise KrispHipError(f"kr_scan_special: [{n}]")
    out = np.empty(max(n, 1), dtype=np.uint64)
    lib.kr_scan_special(_ptr(buf) if len(buf) else None, len(buf), k, 1 if omit_soft else 0, _ptr(out), n,
                        ctypes.byref(bad))
    return out[:n]


class Engine:
    """One GPU context (one HIP stream) -- thin object face of the C ABI."""

    def __init__(self, device=0, hbm_budget=0):
        self.lib = load()
        self.ctx = self.lib.kr_create(device, hbm_budget)
        if not self.ctx:
            raise KrispHipError("kr_create failed: " + self.lib.kr_last_error(None).decode())
        self.params = None
        self._guide_hit_texts = 0
        self._multiplex_texts = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.kr_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            e = KrispHipError(f"{what}: [{rc}] " + self.lib.kr_last_error(self.ctx).decode())
            e.code = int(rc)
            raise e
        return rc

    def _scan_fetch(self, scan, fetch, gid, dtype):
        """scan(ctx, gid) -> the number of records n the scan left on the device, fetch(ctx, out, n) -> `dtype`[n]"""
        n = self._check(getattr(self.lib, scan)(self.ctx, gid), scan)
        out = np.empty(max(n, 1), dtype=dtype)
        self._check(getattr(self.lib, fetch)(self.ctx, _ptr(out), n), fetch)
        return out[:n]

    def _sized_fetch(self, fn, dtype_or_width, *lead):
        """a list whose length the library tells: fn(ctx, *lead, NULL, 0) -> the number of entries n, then
        fn(ctx, *lead, out, size) fills them.  dtype_or_width: the entries' dtype (size = n) -> dtype[n], or the width
        of text rows (size = the bytes) -> uint8 [n, width]"""
        call = getattr(self.lib, fn)
        n = self._check(call(self.ctx, *lead, None, 0), fn)
        rows = isinstance(dtype_or_width, (int, np.integer))
        out = np.empty((max(n, 1), dtype_or_width), dtype=np.uint8) if rows else np.empty(max(n, 1), dtype=dtype_or_width)
        if n:
            self._check(call(self.ctx, *lead, _ptr(out), out.nbytes if rows else n), fn)
        return out[:n]

    def _guide_texts(self, texts, who):
        """texts -> uint8 [n, L+D+R] as the guide tables of method `who` read it; ValueError for another shape"""
        t = np.ascontiguousarray(texts, dtype=np.uint8)
        # (the library reads len(t) rows of L+D+R bytes: another shape would be read past its end)
        k = sum(self.params) if self.params is not None else None
        if t.size and (t.ndim != 2 or (k is not None and t.shape[1] != k)):
            raise ValueError(f"{who}: texts is a matrix with a row of L+D+R = {k} letters per guide (got shape {t.shape})")
        return t

    # ---- configuration
    def upload_text(self, gid, text, universal_newlines, one_shot=True):
        """file text -> genome gid, parsed on the device with the reference reader's semantics (kr_genome_upload_text).
        Returns (bases, records, special characters, rna, fasta)."""
        t = np.ascontiguousarray(text, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.int64)
        n = self._check(self.lib.kr_genome_upload_text(self.ctx, gid, _ptr(t), len(t), 1 if universal_newlines else 0,
                                                       1 if one_shot else 0, _ptr(stats)), "kr_genome_upload_text")
        return n, int(stats[0]), int(stats[1]), stats[2] == 1, bool(stats[3])

    def upload_bgzf(self, gid, raw, one_shot=True):
        """the bytes of a BGZF file -> genome gid: inflated on the device, a lane per member, every member checked against
        its CRC-32 and length, then parsed there (kr_genome_upload_bgzf).  Returns (bases, records, special characters, rna,
        fasta, members, microseconds of the inflate kernels), or None when the file is not BGZF all the way or a member
        does not inflate to its trailer: nothing is uploaded then, the caller reads the file as any other .gz."""
        t = np.ascontiguousarray(raw, dtype=np.uint8)
        stats = np.zeros(8, dtype=np.int64)
        n = self.lib.kr_genome_upload_bgzf(self.ctx, gid, _ptr(t), len(t), 1 if one_shot else 0, _ptr(stats))
        if n == ERR_HOST:
            self.last_bgzf = (int(stats[4]), int(stats[5]), int(stats[6]), self.lib.kr_last_error(self.ctx).decode())
            return None
        n = self._check(n, "kr_genome_upload_bgzf")
        return n, int(stats[0]), int(stats[1]), stats[2] == 1, bool(stats[3]), int(stats[4]), int(stats[7])

    def upload_gzip(self, gid, raw, chunk=None, one_shot=True):
        """the bytes of a `.gz` file of one plain gzip member -> genome gid: inflated on the device (chunks of `chunk`
        compressed bytes, None: the library's choice; block starts found by trial, windows handed down the line, CRC-32 and
        ISIZE checked), then parsed there (kr_genome_upload_gzip).  Returns (bases, records, special characters, rna, fasta,
        chunks, microseconds of the inflate (wall time: kernels and the host steps between them), chunks joined, longest window run), or None -- nothing uploaded, the
        reason in `last_gzip` -- when the device path does not take the file: the caller reads it as any other .gz."""
        t = np.ascontiguousarray(raw, dtype=np.uint8)
        stats = np.zeros(8, dtype=np.int64)
        n = self.lib.kr_genome_upload_gzip(self.ctx, gid, _ptr(t), len(t), int(chunk or 0), 1 if one_shot else 0, _ptr(stats))
        if n == ERR_HOST:
            self.last_gzip = (int(stats[4]), int(stats[5]), int(stats[6]), self.lib.kr_last_error(self.ctx).decode())
            return None
        n = self._check(n, "kr_genome_upload_gzip")
        return (n, int(stats[0]), int(stats[1]), stats[2] == 1, bool(stats[3]), int(stats[4]), int(stats[7]), int(stats[5]),
                int(stats[6]))

    def reserve(self, ids, n_bases, with_text=False):
        """the large device buffers of genomes `ids` of up to n_bases bases, ahead of their uploads (kr_reserve)"""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        self._check(self.lib.kr_reserve(self.ctx, _ptr(a), len(a), int(n_bases), 1 if with_text else 0), "kr_reserve")

    def fetch_bases(self, gid, n):
        out = np.empty(max(n, 1), dtype=np.uint8)
        m = self._check(self.lib.kr_genome_fetch_bases(self.ctx, gid, _ptr(out), n), "kr_genome_fetch_bases")
        return out[:m]

    def set_option(self, option, value):
        """result-neutral options (OPT_SLICE_BASES, OPT_GENERIC_INTERSECT, OPT_ISECT_FORMAT, OPT_ISECT_KERNEL, OPT_WIDE_SLOTS, OPT_LANES); before set_params (OPT_LANES: any time)"""
        self._check(self.lib.kr_set_option(self.ctx, option, int(value)), "kr_set_option")

    def set_params(self, L, D, R, omit_soft=False, max_bases=0):
        self._check(self.lib.kr_set_params(self.ctx, L, D, R, SOFT_OMIT if omit_soft else SOFT_MAP,
                                           max_bases), "kr_set_params")
        self.params = (L, D, R)

    def set_mixed_alphabets(self, on=True):
        """DNA and RNA genomes in one run: the filter in its mode 2 (kr_set_mixed_alphabets)"""
        self._check(self.lib.kr_set_mixed_alphabets(self.ctx, 1 if on else 0), "kr_set_mixed_alphabets")

    def set_strands(self, mode):
        """STRANDS_BOTH (complements), STRANDS_FORWARD, STRANDS_CANONICAL (kstream canonicals)"""
        self._check(self.lib.kr_set_strands(self.ctx, mode), "kr_set_strands")

    # ---- genomes
    def upload(self, gid, bases):
        buf = np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases
        self._check(self.lib.kr_genome_upload(self.ctx, gid, _ptr(buf) if len(buf) else None, len(buf)),
                    "kr_genome_upload")

    def sort(self, gid, coarse=False):
        """kr_genome_sort; coarse=True: the sort may stop behind its first pass (kr_genome_partition) -- enough for a genome
        that joins an intersection beside a sorted ingroup and a sorted outgroup genome with the filter on; any other
        reader sorts it fine by itself"""
        if coarse:
            self._check(self.lib.kr_genome_partition(self.ctx, gid), "kr_genome_partition")
        else:
            self._check(self.lib.kr_genome_sort(self.ctx, gid), "kr_genome_sort")

    def partition(self, gid):
        """sort(gid, coarse=True)"""
        self.sort(gid, coarse=True)

    def add(self, gid, bases):
        self.upload(gid, bases)
        self.sort(gid)
        return self.count(gid)

    def load_sorted(self, gid, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        return self._check(self.lib.kr_genome_load_sorted(self.ctx, gid, _ptr(keys) if len(keys) else None,
                                                          len(keys)), "kr_genome_load_sorted")

    def count(self, gid):
        return self._check(self.lib.kr_genome_count(self.ctx, gid), "kr_genome_count")

    def keys(self, gid):
        n = self.count(gid)
        out = np.empty(max(n, 1), dtype=np.uint64)
        self._check(self.lib.kr_genome_fetch_keys(self.ctx, gid, _ptr(out), n), "kr_genome_fetch_keys")
        return out[:n]

    def set_allow(self, bases):
        """kstream --allow on the device alphabet: an iterable of the bases (of ACGT) a k-mer may hold"""
        mask = sum(1 << "ACGT".index(b) for b in set(bases))
        self._check(self.lib.kr_set_allow(self.ctx, mask), "kr_set_allow")

    def set_field_order(self, widths, order):
        """kstream --sort-cols as a key layout: the window's fields (widths in line order) held in `order`; after
        set_params(k, 0, 0).  Raises for the one order a layout cannot express (see include/krisp_hip.h)."""
        w = np.asarray(list(widths) + [0] * (3 - len(widths)), dtype=np.int32)
        o = np.asarray(order, dtype=np.int32)
        self._check(self.lib.kr_set_field_order(self.ctx, _ptr(w), _ptr(o)), "kr_set_field_order")

    def set_field_pieces(self, pieces):
        """the key = the window's pieces [(offset, width)] one after the other (kr_set_field_pieces); after set_params(k, 0, 0)"""
        o = np.asarray([p[0] for p in pieces], dtype=np.int32)
        w = np.asarray([p[1] for p in pieces], dtype=np.int32)
        self._check(self.lib.kr_set_field_pieces(self.ctx, len(pieces), _ptr(o), _ptr(w)), "kr_set_field_pieces")

    def keys_in_order(self, gid, n_bases):
        """keys of an uploaded genome in stream order (no sort)"""
        out = np.empty(max(2 * n_bases, 1), dtype=np.uint64)
        n = self._check(self.lib.kr_genome_keys_in_order(self.ctx, gid, _ptr(out), len(out)), "kr_genome_keys_in_order")
        return out[:n]

    def free(self, gid):
        self._check(self.lib.kr_genome_free(self.ctx, gid), "kr_genome_free")

    # ---- intersection
    MAX_GENOMES_PER_CALL = 32      # MAXG of kr_intersect

    def intersect(self, gids, is_ingroup, apply_filter=True):
        ids = np.asarray(gids, dtype=np.int32)
        flags = np.asarray([1 if f else 0 for f in is_ingroup], dtype=np.uint8)
        # (more than 32 genomes: the library intersects them in batches and keeps the running list on the device)
        return self._check(self.lib.kr_intersect(self.ctx, _ptr(ids), len(ids), _ptr(flags),
                                                 1 if apply_filter else 0), "kr_intersect")

    def cands(self):
        n = self._check(self.lib.kr_cands_count(self.ctx), "kr_cands_count")
        out = np.empty(max(n, 1), dtype=CAND)
        self._check(self.lib.kr_cands_fetch(self.ctx, _ptr(out), n), "kr_cands_fetch")
        return out[:n]

    def load_cands(self, cands):
        cands = np.ascontiguousarray(cands, dtype=CAND)
        return self._check(self.lib.kr_cands_load(self.ctx, _ptr(cands) if len(cands) else None, len(cands)),
                           "kr_cands_load")

    def merge_cands(self, other=None, apply_filter=False):
        if other is None:
            return self._check(self.lib.kr_cands_merge(self.ctx, None, 0, 0, 1 if apply_filter else 0),
                               "kr_cands_merge")
        other = np.ascontiguousarray(other, dtype=CAND)
        return self._check(self.lib.kr_cands_merge(self.ctx, _ptr(other) if len(other) else None,
                                                   len(other), 1, 1 if apply_filter else 0),
                           "kr_cands_merge")

    def probe_cands(self, gids, is_ingroup, apply_filter=True):
        """candidates := those every listed genome holds, masks OR-ed by side, filter (kr_cands_probe)"""
        ids = np.asarray(gids, dtype=np.int32)
        flags = np.asarray([1 if f else 0 for f in is_ingroup], dtype=np.uint8)
        return self._check(self.lib.kr_cands_probe(self.ctx, _ptr(ids), len(ids), _ptr(flags), 1 if apply_filter else 0),
                           "kr_cands_probe")

    def collect(self, gids, fetch=True):
        ids = np.asarray(gids, dtype=np.int32)
        n = self._check(self.lib.kr_collect(self.ctx, _ptr(ids), len(ids)), "kr_collect")
        return self.fetch_records(n) if fetch else n

    def fetch_records(self, n):
        out = np.empty(max(n, 1), dtype=RECORD)
        self._check(self.lib.kr_fetch(self.ctx, _ptr(out), n), "kr_fetch")
        return out[:n]

    # ---- multi-GPU exchange (one process / context per GPU; krisp_amd/distributed.py does the rendezvous)
    def comm_init(self, rank, world, comm_id):
        """RCCL communicator from the unique id rank 0 made (comm_unique_id)"""
        _quiet_rccl()
        buf = np.frombuffer(comm_id, dtype=np.uint8)
        assert len(buf) == COMM_ID_BYTES
        self._check(self.lib.kr_comm_init(self.ctx, rank, world, _ptr(buf)), "kr_comm_init")

    def comm_init_dir(self, rank, world, directory):
        """rehearsal transport: the same messages through files (ranks may share a GPU)"""
        self._check(self.lib.kr_comm_init_dir(self.ctx, rank, world, os.fsencode(directory)), "kr_comm_init_dir")

    def comm_rccl_ranks(self):
        """ranks of the RCCL communicator as ncclCommCount reports them; 0 without one (file transport, no communicator)"""
        return int(self.lib.kr_comm_rccl_ranks(self.ctx))

    def comm_barrier(self):
        self._check(self.lib.kr_comm_barrier(self.ctx), "kr_comm_barrier")

    def comm_allreduce(self, values, op="sum"):
        v = np.asarray(values, dtype=np.float64).copy()
        self._check(self.lib.kr_comm_allreduce(self.ctx, _ptr(v), len(v), 1 if op == "max" else 0), "kr_comm_allreduce")
        return v

    def comm_allgather(self, data):
        """bytes of every rank (any length) -> list of bytes by rank"""
        world = self.lib.kr_comm_world(self.ctx)
        if world == 1:
            return [bytes(data)]
        n = int(self.comm_allreduce([float(len(data))], "max")[0]) + 8
        mine = np.zeros(n, dtype=np.uint8)
        mine[:8] = np.frombuffer(np.uint64(len(data)).tobytes(), dtype=np.uint8)
        mine[8:8 + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
        out = np.empty(n * world, dtype=np.uint8)
        self._check(self.lib.kr_comm_allgather(self.ctx, _ptr(mine), n, _ptr(out)), "kr_comm_allgather")
        res = []
        for r in range(world):
            ln = int(np.frombuffer(out[r * n:r * n + 8].tobytes(), dtype=np.uint64)[0])
            res.append(out[r * n + 8:r * n + 8 + ln].tobytes())
        return res

    def cands_reduce(self, apply_filter):
        """tree reduction of every rank's candidates onto rank 0 (the count there, 0 elsewhere)"""
        return self._check(self.lib.kr_cands_reduce(self.ctx, 1 if apply_filter else 0), "kr_cands_reduce")

    def cands_bcast(self):
        return self._check(self.lib.kr_cands_bcast(self.ctx), "kr_cands_bcast")

    def records_gather(self):
        return self._check(self.lib.kr_records_gather(self.ctx), "kr_records_gather")

    # ---- wide windows (k > 32 or D > 16)
    def set_params_wide(self, L, D, R, omit_soft=False, max_bases=0):
        self._check(self.lib.kr_set_params_wide(self.ctx, L, D, R, SOFT_OMIT if omit_soft else SOFT_MAP,
                                                max_bases), "kr_set_params_wide")
        self.params = (L, D, R)

    def wide_run(self, gids, is_ingroup, apply_filter=True):
        ids = np.asarray(gids, dtype=np.int32)
        flags = np.asarray([1 if f else 0 for f in is_ingroup], dtype=np.uint8)
        return self._check(self.lib.kr_wide_run(self.ctx, _ptr(ids), len(ids), _ptr(flags),
                                                1 if apply_filter else 0), "kr_wide_run")

    def wide_count(self, what):
        """number of entries kr_wide_fetch(what) would return"""
        return self._check(self.lib.kr_wide_fetch(self.ctx, what, None, 0), "kr_wide_fetch")

    def wide_fetch(self, what):
        n = self._check(self.lib.kr_wide_fetch(self.ctx, what, None, 0), "kr_wide_fetch")
        out = np.empty(max(n, 1), dtype=WIDE_HIT if what == WIDE_HITS else np.uint64)
        self._check(self.lib.kr_wide_fetch(self.ctx, what, _ptr(out), out.nbytes), "kr_wide_fetch")
        return out[:n]

    def wide_windows(self, k):
        """the member windows of the latest wide_run as text, cut on the device (kr_wide_fetch_windows): uint8 [nhits, k]"""
        return self._sized_fetch("kr_wide_fetch_windows", k)

    # ---- locations (krisp_fasta --out_locations)
    def set_params_locate(self, L, D, R, omit_soft=False, max_bases=0):
        """a context for the locate pass only: genomes go up with no sort plan (kr_set_params_locate)"""
        self._check(self.lib.kr_set_params_locate(self.ctx, L, D, R, SOFT_OMIT if omit_soft else SOFT_MAP, max_bases),
                    "kr_set_params_locate")
        self.params = (L, D, R)

    def locate_table(self, flanks):
        """flanks: uint8 [ngroups, L+R] (left then right, upper case, T for U) -> slots of the table (kr_locate_table)"""
        f = np.ascontiguousarray(flanks, dtype=np.uint8)
        return self._check(self.lib.kr_locate_table(self.ctx, _ptr(f) if f.size else None, len(f)), "kr_locate_table")

    def locate(self, gid):
        """LOC_HIT array of uploaded genome gid against the table: position order, strand 0 before 1 (kr_locate_scan)"""
        return self._scan_fetch("kr_locate_scan", "kr_locate_fetch", gid, LOC_HIT)

    def locate_windows(self, k):
        """the latest locate()'s windows as text, cut on the device: uint8 [nhits, k] (kr_locate_windows)"""
        return self._sized_fetch("kr_locate_windows", k)

    def locate_seps(self, gid):
        """the positions of genome gid's record separators, ascending (kr_locate_seps)"""
        return self._sized_fetch("kr_locate_seps", np.uint64, gid)

    def near_table(self, targets, mismatches):
        """targets: uint8 [n, L+D+R] (upper case, T for U), in a locate context -> slots of the seed table (kr_near_table)"""
        t = np.ascontiguousarray(targets, dtype=np.uint8)
        return self._check(self.lib.kr_near_table(self.ctx, _ptr(t) if t.size else None, len(t), mismatches), "kr_near_table")

    def near(self, gid):
        """NEAR_HIT array of uploaded genome gid against the seed table, in position order (kr_near_scan)"""
        return self._scan_fetch("kr_near_scan", "kr_near_fetch", gid, NEAR_HIT)

    def near_windows(self, k):
        """the latest near()'s windows as text, cut on the device: uint8 [nhits, k] (kr_near_windows)"""
        return self._sized_fetch("kr_near_windows", k)

    def guide_hits_table(self, texts, mismatches, pam5="", pam3="", need_pam=False):
        """texts: uint8 [n, G] protospacers in A, C, G, T, in a locate context with L+D+R = G; pam5 / pam3: the motifs in
        IUPAC letters, read 5'->3' on the guide's strand -> slots of the seed table (kr_guide_hits_table)"""
        t = self._guide_texts(texts, "guide_hits_table")
        slots = self._check(self.lib.kr_guide_hits_table(self.ctx, _ptr(t) if t.size else None, len(t), mismatches, _motif_bytes(pam5),
                                                         _motif_bytes(pam3), 1 if need_pam else 0), "kr_guide_hits_table")
        self._guide_hit_texts = len(t)                # (guide_hits_tally's rows; a refused table leaves the earlier one)
        return slots

    def guide_hits(self, gid):
        """GUIDE_HIT_RAW array of uploaded genome gid against the guides' table, in position order (kr_guide_hits_scan)"""
        return self._scan_fetch("kr_guide_hits_scan", "kr_guide_hits_fetch", gid, GUIDE_HIT_RAW)

    def guide_hit_windows(self, G):
        """the latest guide_hits()'s windows as the guide's strand reads them, cut on the device: uint8 [nhits, G]
        (kr_guide_hits_windows)"""
        return self._sized_fetch("kr_guide_hits_windows", G)

    def guide_hits_tally(self):
        """the hits of the latest guide_hits() / guide_hits_scan() counted on the device: uint32 [nguides, 4], column m = the
        guide's hits with m mismatches (kr_guide_hits_tally)"""
        out = np.zeros((max(self._guide_hit_texts, 1), 4), dtype=np.uint32)
        n = self._check(self.lib.kr_guide_hits_tally(self.ctx, _ptr(out), out.size), "kr_guide_hits_tally")
        return out[:n // 4]

    def guide_bulges_table(self, texts, mismatches, bulges, pam5="", pam3="", need_pam=False):
        """as guide_hits_table, for the bulged search with bulges of 1 .. `bulges` bases (1 or 2): the seed table of the
        guides' halves -> its slots (kr_guide_bulges_table).  A state of its own beside guide_hits_table's"""
        t = self._guide_texts(texts, "guide_bulges_table")
        return self._check(self.lib.kr_guide_bulges_table(self.ctx, _ptr(t) if t.size else None, len(t), mismatches, bulges,
                                                          _motif_bytes(pam5), _motif_bytes(pam3), 1 if need_pam else 0), "kr_guide_bulges_table")

    def guide_bulges(self, gid):
        """GUIDE_BULGE_HIT_RAW array of uploaded genome gid against the guides' table: the bulged hits, in the order of the
        seed pairs that own them (kr_guide_bulges_scan)"""
        return self._scan_fetch("kr_guide_bulges_scan", "kr_guide_bulges_fetch", gid, GUIDE_BULGE_HIT_RAW)

    def guide_bulge_windows(self, width):
        """the latest guide_bulges()'s windows as the guide's strand reads them, cut on the device: uint8 [nhits, width],
        width = G + bulges; row i holds hit i's `length` letters, then 0 (kr_guide_bulges_windows)"""
        return self._sized_fetch("kr_guide_bulges_windows", width)

    def products_table(self, left, right, pairs, mismatches, max_product):
        """left: uint8 [nl, L], right: uint8 [nr, R] (upper case, T for U), pairs: [np, 2] rows of (left, right), in a
        locate context whose L and R are the texts' lengths -> slots of the seed table (kr_products_table)"""
        lf = np.ascontiguousarray(left, dtype=np.uint8)
        rt = np.ascontiguousarray(right, dtype=np.uint8)
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        return self._check(self.lib.kr_products_table(self.ctx, _ptr(lf) if lf.size else None, len(lf),
                                                      _ptr(rt) if rt.size else None, len(rt), _ptr(pr) if pr.size else None,
                                                      len(pr), mismatches, max_product), "kr_products_table")

    def products(self, gid):
        """PRODUCT_HIT array of uploaded genome gid in (pos, length, strand, pair) order (kr_products_scan)"""
        return self._scan_fetch("kr_products_scan", "kr_products_fetch", gid, PRODUCT_HIT)

    def product_sites(self):
        """the latest products()'s primer sites as the device lists them: PRODUCT_SITE, position order (kr_products_sites)"""
        return self._sized_fetch("kr_products_sites", PRODUCT_SITE)

    def primers_table(self, texts, nleft, pairs, mismatches, max_product):
        """texts: a list of bytes (upper case, T for U), each of its own length 10 .. 60, the first nleft of them left
        texts, the others right texts (the template's text under the right primer); pairs: [np, 2] rows of (left, right)
        -> slots of the seed table (kr_primers_table)"""
        texts = [bytes(t) for t in texts]
        offsets = np.zeros(len(texts) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([len(t) for t in texts], dtype=np.int64)
        text = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8)      # (never empty: a pointer to pass)
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        slots = self._check(self.lib.kr_primers_table(self.ctx, _ptr(text), _ptr(offsets), nleft, len(texts) - nleft,
                                                      _ptr(pr) if pr.size else None, len(pr), mismatches, max_product),
                            "kr_primers_table")
        self._primer_pairs = len(pr)                  # (primers_tally's rows; a refused table leaves no table)
        return slots

    def primer_products(self, gid):
        """PRODUCT_HIT array of uploaded genome gid in (pos, length, strand, pair) order (kr_primers_scan)"""
        return self._scan_fetch("kr_primers_scan", "kr_primers_fetch", gid, PRODUCT_HIT)

    def primer_sites(self):
        """the latest primer_products()'s primer sites as the device lists them: PRODUCT_SITE, position order
        (kr_primers_sites)"""
        return self._sized_fetch("kr_primers_sites", PRODUCT_SITE)

    def primers_scan(self, gid):
        """scans uploaded genome gid against the primer table and leaves the products on the device -> their number
        (kr_primers_scan)"""
        return self._check(self.lib.kr_primers_scan(self.ctx, gid), "kr_primers_scan")

    def primers_tally(self):
        """the products of the latest primers_scan() / primer_products() counted on the device: uint32 [pairs, 8], column m
        = the pair's products with left_mm + right_mm = m (0 .. 6), column 7 = those without a mismatch at either 3' end
        (kr_primers_tally)"""
        out = np.zeros((max(getattr(self, "_primer_pairs", 0), 1), 8), dtype=np.uint32)
        n = self._check(self.lib.kr_primers_tally(self.ctx, _ptr(out), out.size), "kr_primers_tally")
        return out[:n // 8]

    def guide_hits_scan(self, gid):
        """scans uploaded genome gid against the guides' table and leaves the hits on the device -> their number
        (kr_guide_hits_scan)"""
        return self._check(self.lib.kr_guide_hits_scan(self.ctx, gid), "kr_guide_hits_scan")

    def assay_table(self, links):
        """links: [n, 2] rows of (row of primers_table's pairs, row of guide_hits_table's texts), strictly ascending; both
        tables stand in this context -> n (kr_assay_table)"""
        lk = np.ascontiguousarray(links, dtype=np.uint32).reshape(-1, 2)
        return self._check(self.lib.kr_assay_table(self.ctx, _ptr(lk) if lk.size else None, len(lk)), "kr_assay_table")

    def assay_join(self, gid):
        """joins the products of the latest primers scan with the hits of the latest guide-hit scan, both of genome gid, on
        the device -> the number of assay hits (kr_assay_join)"""
        return self._check(self.lib.kr_assay_join(self.ctx, gid), "kr_assay_join")

    def assay_hits(self):
        """ASSAY_HIT_RAW array of the latest assay_join() in (pos, length, strand, pair, hit_pos, hit_strand, guide) order
        (kr_assay_fetch)"""
        return self._sized_fetch("kr_assay_fetch", ASSAY_HIT_RAW)

    def multiplex_table(self, texts, mismatches, max_product):
        """texts: a list of 1 .. 128 bytes (upper case, T for U, 5'->3'), each of its own length 10 .. 60: the oligos of one
        tube.  Text t opens a product as written and closes one as its reverse complement -> slots of the seed table
        (kr_multiplex_table).  A state of its own beside primers_table's"""
        texts = [bytes(t) for t in texts]
        offsets = np.zeros(len(texts) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([len(t) for t in texts], dtype=np.int64)
        text = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8)      # (never empty: a pointer to pass)
        slots = self._check(self.lib.kr_multiplex_table(self.ctx, _ptr(text), _ptr(offsets), len(texts), mismatches, max_product),
                            "kr_multiplex_table")
        self._multiplex_texts = len(texts)            # (multiplex_tally's side; a refused table leaves no table)
        return slots

    def multiplex_scan(self, gid):
        """scans uploaded genome gid against the oligos' table and leaves the products on the device -> their number
        (kr_multiplex_scan)"""
        return self._check(self.lib.kr_multiplex_scan(self.ctx, gid), "kr_multiplex_scan")

    def multiplex_products(self, gid):
        """MULTIPLEX_HIT array of uploaded genome gid in (pos, length, fwd, rev) order (kr_multiplex_scan)"""
        return self._scan_fetch("kr_multiplex_scan", "kr_multiplex_fetch", gid, MULTIPLEX_HIT)

    def multiplex_sites(self):
        """the latest multiplex scan's primer sites as the device lists them: PRODUCT_SITE, position order
        (kr_multiplex_sites)"""
        return self._sized_fetch("kr_multiplex_sites", PRODUCT_SITE)

    def multiplex_tally(self):
        """the products of the latest multiplex scan counted on the device: uint32 [T, T, 2], [a, b, clean] = the products
        that text a opens and text b closes, clean = 1 where neither 3' end holds a mismatch (kr_multiplex_tally)"""
        T = max(self._multiplex_texts, 1)
        out = np.zeros((T, T, 2), dtype=np.uint32)
        self._check(self.lib.kr_multiplex_tally(self.ctx, _ptr(out), out.size), "kr_multiplex_tally")
        return out

    def design_table(self, params):
        """params: thermo.Params, the model's integers and the primer options (kr_design_table)"""
        self._design_hairpins = False             # (kr_design_table switches the check off, whatever it returns)
        self._check(self.lib.kr_design_table(self.ctx, ctypes.byref(params)), "kr_design_table")

    def design_hairpins(self, params):
        """params: thermo.HairpinParams -- hold every candidate of design() to max_sec for its hairpin figure too -- or
        None: the check off again (kr_design_hairpins).  After design_table; the next design_table switches it off"""
        self._design_hairpins = False
        self._check(self.lib.kr_design_hairpins(self.ctx, None if params is None else ctypes.byref(params)), "kr_design_hairpins")
        self._design_hairpins = params is not None

    def design(self, templates, L, D, R):
        """templates: uint8 [regions, L + D + R] (upper case, T for U) -> DESIGN_RECORD array, one per region
        (kr_design_run, kr_design_fetch); after design_hairpins(params) a DESIGN_RECORD_HP array: the same fields and
        the pair's two hairpin figures (kr_design_fetch_hairpins)"""
        t = np.ascontiguousarray(templates, dtype=np.uint8).reshape(-1, L + D + R)
        self._check(self.lib.kr_design_run(self.ctx, _ptr(t) if t.size else None, len(t), L, D, R), "kr_design_run")
        out = np.empty(max(len(t), 1), dtype=DESIGN_RECORD)
        self._check(self.lib.kr_design_fetch(self.ctx, _ptr(out), len(t)), "kr_design_fetch")
        if not getattr(self, "_design_hairpins", False):
            return out[:len(t)]
        hp = np.empty((max(len(t), 1), 2), dtype=np.int32)
        self._check(self.lib.kr_design_fetch_hairpins(self.ctx, _ptr(hp), 2 * len(t)), "kr_design_fetch_hairpins")
        both = np.empty(len(t), dtype=DESIGN_RECORD_HP)
        for name in DESIGN_RECORD.names:
            both[name] = out[name][:len(t)]
        both["left_hairpin"], both["right_hairpin"] = hp[:len(t), 0], hp[:len(t), 1]
        return both

    def design_top(self, templates, L, D, R, top):
        """as design(), for the `top` (1 .. 8) passing pairs of least (penalty, left_start, left_len, right_start, right_len)
        of every region -> DESIGN_RECORD [regions, top]: column j is the pair of rank j + 1, column 0 design()'s record, all
        zero where the region has fewer (kr_design_run_top, kr_design_fetch_top); after design_hairpins(params)
        DESIGN_RECORD_HP [regions, top] with every slot's two hairpin figures (kr_design_fetch_top_hairpins)"""
        t = np.ascontiguousarray(templates, dtype=np.uint8).reshape(-1, L + D + R)
        self._check(self.lib.kr_design_run_top(self.ctx, _ptr(t) if t.size else None, len(t), L, D, R, top), "kr_design_run_top")
        n = len(t)
        out = np.empty((max(n, 1), top), dtype=DESIGN_RECORD)
        self._check(self.lib.kr_design_fetch_top(self.ctx, _ptr(out), n * top), "kr_design_fetch_top")
        if not getattr(self, "_design_hairpins", False):
            return out[:n]
        hp = np.empty((max(n, 1), top, 2), dtype=np.int32)
        self._check(self.lib.kr_design_fetch_top_hairpins(self.ctx, _ptr(hp), 2 * n * top), "kr_design_fetch_top_hairpins")
        both = np.empty((n, top), dtype=DESIGN_RECORD_HP)
        for name in DESIGN_RECORD.names:
            both[name] = out[name][:n]
        both["left_hairpin"], both["right_hairpin"] = hp[:n, :, 0], hp[:n, :, 1]
        return both

    def panel(self, templates, pairs, size, texts=None):
        """templates: uint8 [candidates, W], pairs: uint16 [candidates, 4] (left_start, left_len, right_start, right_len), in
        the order the selection goes by; after design_table (the model and max_sec) -> (PANEL_MEMBER array of at most
        `size` members in order of acceptance, PANEL_FATE array, one per candidate) (kr_panel_run, kr_panel_fetch,
        kr_panel_fates).  (texts: panel_clean's)"""
        t = np.ascontiguousarray(templates, dtype=np.uint8)
        if t.ndim != 2:
            raise ValueError("panel: templates is a matrix, a row of W letters each")
        q = np.ascontiguousarray(pairs, dtype=np.uint16).reshape(-1, 4)
        if len(q) != len(t):
            raise ValueError(f"panel: {len(t)} templates, {len(q)} pairs")
        n = len(t)
        if texts is None:
            members = self._check(self.lib.kr_panel_run(self.ctx, _ptr(t) if n else None, _ptr(q) if n else None, n, t.shape[1], size),
                                  "kr_panel_run")
        else:
            x = np.ascontiguousarray(texts, dtype=np.uint32).reshape(-1, 2)
            if len(x) != n:
                raise ValueError(f"panel_clean: {n} templates, {len(x)} rows of texts")
            members = self._check(self.lib.kr_panel_run_clean(self.ctx, _ptr(t) if n else None, _ptr(q) if n else None,
                                                              _ptr(x) if n else None, n, t.shape[1], size), "kr_panel_run_clean")
        out = np.zeros(max(members, 1), dtype=PANEL_MEMBER)
        self._check(self.lib.kr_panel_fetch(self.ctx, _ptr(out), members), "kr_panel_fetch")
        fates = np.zeros(max(n, 1), dtype=PANEL_FATE)
        self._check(self.lib.kr_panel_fates(self.ctx, _ptr(fates), 2 * n), "kr_panel_fates")
        return out[:members], fates[:n]

    def panel_sites_table(self, texts, mismatches, max_product):
        """texts: a list of 1 .. 2^24 - 1 bytes (upper case, T for U, 5'->3'), each of its own length 10 .. 60: the distinct
        primer texts of all candidates of panel_clean.  Empties the site store -> slots of the seed table
        (kr_panel_sites_table).  A state of its own beside multiplex_table's and primers_table's"""
        texts = [bytes(t) for t in texts]
        offsets = np.zeros(len(texts) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([len(t) for t in texts], dtype=np.int64)
        text = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8)      # (never empty: a pointer to pass)
        return self._check(self.lib.kr_panel_sites_table(self.ctx, _ptr(text), _ptr(offsets), len(texts), mismatches, max_product),
                           "kr_panel_sites_table")

    def panel_sites_scan(self, gid):
        """appends the primer sites of uploaded genome gid to the store -> that genome's site count (kr_panel_sites_scan)"""
        return self._check(self.lib.kr_panel_sites_scan(self.ctx, gid), "kr_panel_sites_scan")

    def panel_sites(self):
        """the store as the device holds it -> (PRODUCT_SITE array, uint32 array of the sites' record numbers)
        (kr_panel_sites_fetch)"""
        n = self._check(self.lib.kr_panel_sites_fetch(self.ctx, None, None, 0), "kr_panel_sites_fetch")
        sites, unit = np.empty(max(n, 1), dtype=PRODUCT_SITE), np.empty(max(n, 1), dtype=np.uint32)
        self._check(self.lib.kr_panel_sites_fetch(self.ctx, _ptr(sites), _ptr(unit), n), "kr_panel_sites_fetch")
        return sites[:n], unit[:n]

    def panel_clean(self, templates, pairs, texts, size):
        """panel() with the site store: texts = uint32 [candidates, 2], the rows of panel_sites_table's texts that are the
        candidate's left and right primer -> (members, fates, drops): fates 4 (a product with a member's primer in some
        scanned genome) and 5 (a primer that forms a product with itself) beside panel()'s; drops = uint32 [1 + members]:
        the self-priming candidates, then what each member dropped as cross (kr_panel_run_clean, kr_panel_clean_drops)"""
        members, fates = self.panel(templates, pairs, size, texts=texts)
        drops = np.zeros(1 + len(members), dtype=np.uint32)
        self._check(self.lib.kr_panel_clean_drops(self.ctx, _ptr(drops), len(drops)), "kr_panel_clean_drops")
        return members, fates, drops

    def guides_table(self, guide_size, pam5=(), pam3=(), gc=(30, 70), min_mismatches=1):
        """the options of guides(): pam5 / pam3 = the motifs as sequences of 4-bit IUPAC masks, read 5'->3' on the guide's
        strand (kr_guides_table)"""
        p = GuideParams(guide_size=guide_size, pam5_len=len(pam5), pam3_len=len(pam3), gc_lo=gc[0], gc_hi=gc[1],
                        min_mismatches=min_mismatches)
        for j, m in enumerate(pam5[:8]):
            p.pam5[j] = m
        for j, m in enumerate(pam3[:8]):
            p.pam3[j] = m
        self._check(self.lib.kr_guides_table(self.ctx, ctypes.byref(p)), "kr_guides_table")

    def _guide_regions(self, rows, row_off, bounds, who):
        """the arguments of guides() and guides_top() as the library reads them -> (rows, row_off, bounds, regions)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        if rows.ndim != 2:
            raise ValueError(f"{who}: rows is a matrix, a row of K letters each")
        off = np.ascontiguousarray(row_off, dtype=np.uint64).ravel()
        bnd = np.ascontiguousarray(bounds, dtype=np.uint32).reshape(-1, 2)
        n = len(off) - 1
        if n < 0 or len(bnd) != n or (n and int(off[-1]) > len(rows)):
            raise ValueError(f"{who}: {len(off)} row offsets up to {int(off[-1]) if len(off) else 0}, {len(bnd)} bounds, {len(rows)} rows")
        return rows, off, bnd, n

    def guides(self, rows, row_off, bounds, L, D):
        """rows: uint8 [n, K] (upper case, T for U), row_off: [regions + 1] counted in rows -- a region's first row is its
        template, the others its outgroup rows --, bounds: [regions, 2] columns [lo, hi) -> GUIDE_RECORD array, one per
        region (kr_guides_run, kr_guides_fetch)"""
        rows, off, bnd, n = self._guide_regions(rows, row_off, bounds, "guides")
        self._check(self.lib.kr_guides_run(self.ctx, _ptr(rows) if rows.size else None, _ptr(off), _ptr(bnd) if n else None, n,
                                           rows.shape[1], L, D), "kr_guides_run")
        out = np.empty(max(n, 1), dtype=GUIDE_RECORD)
        self._check(self.lib.kr_guides_fetch(self.ctx, _ptr(out), n), "kr_guides_fetch")
        return out[:n]

    def guides_top(self, rows, row_off, bounds, L, D, top):
        """as guides(), for the `top` (1 .. 8) best candidates of every region -> GUIDE_RECORD [regions, top]: column j is the
        candidate of rank j + 1, all zero but `candidates` where the region has fewer (kr_guides_run_top,
        kr_guides_fetch_top)"""
        rows, off, bnd, n = self._guide_regions(rows, row_off, bounds, "guides_top")
        self._check(self.lib.kr_guides_run_top(self.ctx, _ptr(rows) if rows.size else None, _ptr(off), _ptr(bnd) if n else None, n,
                                               rows.shape[1], L, D, top), "kr_guides_run_top")
        out = np.empty((max(n, 1), top), dtype=GUIDE_RECORD)
        self._check(self.lib.kr_guides_fetch_top(self.ctx, _ptr(out), n * top), "kr_guides_fetch_top")
        return out[:n]

    # ---- timing
    def sync(self):
        self._check(self.lib.kr_sync(self.ctx), "kr_sync")

    def timer_begin(self):
        self._check(self.lib.kr_timer_begin(self.ctx), "kr_timer_begin")

    def timer_end_ms(self):
        ms = self.lib.kr_timer_end_ms(self.ctx)
        if ms < 0:
            raise KrispHipError("kr_timer_end_ms failed")
        return ms

    def stage_enable(self, on=True):
        self.lib.kr_stage_enable(self.ctx, 1 if on else 0)

    def stage_select(self, names):
        """time only the named stages (event pairs around their launches)"""
        mask = 0
        for n in names:
            mask |= 1 << STAGES.index(n)
        self.lib.kr_stage_select(self.ctx, mask)

    def stage_reset(self):
        self.lib.kr_stage_reset(self.ctx)

    def stage_times(self):
        return {name: (self.lib.kr_stage_ms(self.ctx, i), self.lib.kr_stage_launches(self.ctx, i))
                for i, name in enumerate(STAGES)}

    # ---- introspection (stage-level parity tests)
    def debug_info(self):
        o = np.zeros(8, dtype=np.int64)
        self.lib.kr_debug_info(self.ctx, _ptr(o))
        return dict(b=int(o[0]), nbuckets=int(o[1]), T=int(o[2]), CAP=int(o[3]), nwg=int(o[4]),
                    overflow_segments=int(o[5]), fallback_launches=int(o[6]), nslices=int(o[7]))

    def debug_isect(self):
        o = np.zeros(8, dtype=np.int64)
        self.lib.kr_debug_isect(self.ctx, _ptr(o))
        return dict(chunk_kernel_items=int(o[0]), slices_redone=int(o[1]), threads=int(o[2]), buckets_per_item_log2=int(o[3]),
                    heads32=int(o[4]), sort_lanes=int(o[5]), join2_launches=int(o[6]), join2_handed_on=int(o[7]))

    def debug_lazy(self):
        """KR_OPT_LAZY_ORDER's counters (kr_debug_lazy): LDS sorts of whole slices the sorts left out, made later, collects
        that sorted the touched buckets only, the option's value"""
        o = np.zeros(8, dtype=np.int64)
        self.lib.kr_debug_lazy(self.ctx, _ptr(o))
        return dict(skipped=int(o[0]), ordered_later=int(o[1]), touch_collects=int(o[2]), on=int(o[3]),
                    anchor_in_bucket_order=int(o[4]), fuse_anchor=int(o[5]), coarse=int(o[6]), coarse_promoted=int(o[7]))

    def debug_scan(self):
        """the latest tile scan's geometry (kr_debug_scan): tiles, workgroups launched and the KR_SCAN_GRID cap in force (0:
        none) of the latest scan, the tiles or blocks of the latest two-pass list"""
        o = np.zeros(8, dtype=np.int64)
        self.lib.kr_debug_scan(self.ctx, _ptr(o))
        return dict(tiles=int(o[0]), grid=int(o[1]), cap=int(o[2]), blocks=int(o[3]))

    def copy_gbps(self, nbytes=1 << 30, reps=10):
        v = self.lib.kr_debug_copy_gbps(self.ctx, nbytes, reps)
        if v < 0:
            raise KrispHipError("kr_debug_copy_gbps failed")
        return v

    def mem_info(self):
        """bytes this context may still allocate (device free memory / rest of its budget), device total, held, budget"""
        o = np.zeros(4, dtype=np.int64)
        self._check(self.lib.kr_mem_info(self.ctx, _ptr(o)), "kr_mem_info")
        return dict(avail=int(o[0]), total=int(o[1]), used=int(o[2]), budget=int(o[3]))

    def debug_comm(self):
        """what the multi-GPU exchange has cost so far (kr_debug_comm)"""
        o = np.zeros(8, dtype=np.int64)
        self._check(self.lib.kr_debug_comm(self.ctx, _ptr(o)), "kr_debug_comm")
        return dict(syncs=int(o[0]), p2p=int(o[1]), collectives=int(o[2]), exchange_us=int(o[3]), reduces=int(o[4]),
                    message_entries=int(o[5]))

    def debug_place(self):
        """the latest placement search of the pass-1 output buffers (kr_debug_place)"""
        o = np.zeros(8, dtype=np.float64)
        self._check(self.lib.kr_debug_place(self.ctx, _ptr(o)), "kr_debug_place")
        return dict(candidates=int(o[0]), taken=int(o[1]), fastest_ms=[round(float(x), 4) for x in o[2:6]],
                    median_ms=round(float(o[6]), 4), slowest_ms=round(float(o[7]), 4))

    def debug_coarse_strand(self):
        """KR_OPT_COARSE_ONE_STRAND's counters (kr_debug_coarse_strand): partitions that wrote one strand, intersections that
        probed such genomes, their forward / reverse rounds in all and of the latest call, the option's value, the passes of the
        latest call (KR_OPT_COARSE_ONE_PASS)"""
        o = np.zeros(8, dtype=np.int64)
        self._check(self.lib.kr_debug_coarse_strand(self.ctx, _ptr(o)), "kr_debug_coarse_strand")
        return dict(partitions=int(o[0]), calls=int(o[1]), rounds_forward=int(o[2]), rounds_reverse=int(o[3]),
                    last_forward=int(o[4]), last_reverse=int(o[5]), on=int(o[6]), last_passes=int(o[7]))

    def debug_coarse_pool(self):
        """the pool of placed pass-1 targets of coarse genomes (kr_debug_coarse_pool)"""
        o = np.zeros(8, dtype=np.float64)
        self._check(self.lib.kr_debug_coarse_pool(self.ctx, _ptr(o)), "kr_debug_coarse_pool")
        return dict(total=int(o[0]), free=int(o[1]), held=int(o[2]), partitions=int(o[3]), searches=int(o[4]),
                    held_ms=[round(float(o[5]), 4), round(float(o[6]), 4)], on=int(o[7]))

    def comm_set_timeout(self, seconds):
        """the exchange's deadline: the watchdog aborts the communicator `seconds` after an exchange call began (kr_comm_set_timeout)"""
        self._check(self.lib.kr_comm_set_timeout(self.ctx, int(seconds)), "kr_comm_set_timeout")

    def debug_comm_hang(self):
        """test aid: a receive without a sender; raises once the watchdog has aborted the communicator (kr_debug_comm_hang)"""
        return self._check(self.lib.kr_debug_comm_hang(self.ctx), "kr_debug_comm_hang")

    def cands_selfexchange(self, apply_filter=False):
        """one round of the tree with the rank itself as partner, over RCCL (kr_debug_cands_selfexchange)"""
        return self._check(self.lib.kr_debug_cands_selfexchange(self.ctx, 1 if apply_filter else 0), "kr_debug_cands_selfexchange")

    def comm_probe(self, nbytes=64 << 10, reps=50):
        """microseconds per blocking call of the exchange (kr_debug_comm_probe; RCCL communicators only)"""
        o = np.zeros(3, dtype=np.float64)
        self._check(self.lib.kr_debug_comm_probe(self.ctx, nbytes, reps, _ptr(o)), "kr_debug_comm_probe")
        return dict(allreduce_sync_us=round(float(o[0]), 2), sendrecv_self_sync_us=round(float(o[1]), 2),
                    bcast_sync_us=round(float(o[2]), 2), message_bytes=int(nbytes))

    def copy_which(self):
        """the copy form and grid the latest copy_gbps() found fastest"""
        return (self.lib.kr_debug_copy_which(self.ctx) or b"").decode()

    def inversions(self, gid):
        return self._check(self.lib.kr_debug_inversions(self.ctx, gid), "kr_debug_inversions")

    def debug_fetch(self, gid, what, n_max):
        dt = {0: np.uint64, 1: np.uint32, 2: np.uint32, 3: np.uint32, 4: np.uint64, 5: np.uint64}[what]
        out = np.empty(max(n_max, 1), dtype=dt)
        n = self._check(self.lib.kr_debug_fetch(self.ctx, gid, what, _ptr(out), out.nbytes), "kr_debug_fetch")
        return out[:n]

// krisp_hip.hip -- hand-written HIP (gfx950 / MI355X) for krisp_fasta's hot path:
// 2-bit pack -> both-strand keys -> MSD radix partition (LDS digit histograms,
// per-workgroup private cursors) -> LDS bucket sort -> n-way intersection with
// diagnostic-column masks -> candidate compaction -> record collection.
// C ABI: include/krisp_hip.h (each entry point cites the reference seam it replaces).
//
// Integer / byte work, HBM-bound: no MFMA anywhere (DESIGN.md "kernels").
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>       // the one exchange step of the multi-GPU flow (h_comm.inc)
#include <dlfcn.h>
#include <sys/stat.h>
#include <zlib.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <condition_variable>
#include <cerrno>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "krisp_hip.h"

// One translation unit, cut into parts by subject (kernels k_*, host code h_*):
#include "k_keys.inc"        // typedefs, key geometry, tunables, key generators
#include "co_strand.inc"     // one strand of a coarse genome answers for both: digit, classes, patterns (shared with a host check)
#include "k_sort.inc"        // pack, histograms, pass 0 / 1 / 2, chunk table, LDS sort, merge fallback
#include "k_sort2.inc"       // pass 1 / pass 2 / LDS sort as persistent, software-pipelined kernels (buffer loads, counted waits)
#include "k_intersect.inc"   // n-way intersection, candidate compaction, collection, list merge
#include "k_intersect3.inc"  // the same intersection as a persistent, software-pipelined kernel (items of whole buckets)
#include "k_intersect3t.inc" // ... with 32-bit heads where the geometry allows
#include "k_join2.inc"       // two genomes, one of each side: a byte screen in LDS, an exact join of the live keys only
#include "k_text.inc"        // the reference reader on the device: file text -> upload buffer
#include "k_inflate.inc"     // BGZF members inflated on the device, a lane per member (round 6)
#include "k_gunzip.inc"      // one plain gzip member inflated on the device: chunks, block starts found by trial, windows
#include "k_wide.inc"        // wide path kernels, copy kernel
#include "k_scan.inc"        // what the six one-genome scans share: tile staging, block scan, two-pass epilogue, seed probe, separators
#include "k_locate.inc"      // the locate pass: flank-table scan of a genome's bases
#include "k_near.inc"        // the near-match pass: pigeonhole seeds of the targets, scan within Hamming distance M
#include "k_guide_hits.inc"  // the guide-hit pass: behind the near pass's scan a per-hit step (ghit_step.inc: column mask, PAM motifs), need_pam's selection
#include "k_guide_bulges.inc" // the bulged guide-hit pass: the near scan over the guides' halves, a per-pair step (gbulge_step.inc) for DNA / RNA bulges

#include "k_products.inc"    // the product pass: sites of the flanks within M substitutions, joined into PCR products
#include "k_primers.inc"     // the primer-product pass: sites of primer texts of mixed lengths, joined into PCR products
#include "k_assay.inc"       // the assay join: the guide hits inside the primer products' interiors, a thread per product
#include "k_multiplex.inc"   // the multiplex pass: every opening site of a panel's oligos joined with every closing site, and its tally
#include "k_design.inc"      // the primer design pass: a wavefront per region, integer thermodynamics, the best pair
#include "panel_step.inc"    // what the panel pass does per window, table slot and primer base, in plain C++ (shared with a host check)
#include "k_panel.inc"       // the panel pass: a launch per round, the member's windows in an LDS table, a wavefront per candidate
#include "pclean_step.inc"   // what the clean panel selection does per stored site and owner, in plain C++ (shared with a host check)
#include "k_panel_clean.inc" // the clean panel selection: the site store, self-priming, a member's cross products, the next member
#include "k_coarse.inc"      // a genome that stopped behind pass 1 against a short candidate list: LDS table per top byte, hit list
#include "k_guides.inc"      // the guide pass: a wavefront per region, the window next to a PAM that differs most from the outgroup rows
#include "h_core.inc"        // context, buffers, parameters, upload, sort, finalize   (opens extern "C")
#include "h_intersect.inc"   // kr_intersect, candidate lists, kr_collect
#include "h_wide.inc"        // kr_wide_run
#include "h_scan.inc"        // ... and on the host: two-pass driver, separator list, launch geometry, fetches; for the five seed passes the
                             // pieces, entries and keys, the seed table, the near-scan launcher, the pair list (its header: which helper serves which)
#include "h_locate.inc"      // kr_set_params_locate, kr_locate_*: where the surviving groups' windows lie
#include "h_near.inc"        // kr_near_*: the windows of a genome within M substitutions of an ingroup window
#include "h_guide_hits.inc"  // kr_guide_hits_*: the windows of a genome within M substitutions of a picked guide, with their motifs
#include "h_guide_bulges.inc" // kr_guide_bulges_*: the windows of a genome within M substitutions and one bulge of a picked guide
#include "h_products.inc"    // kr_products_*: in-silico PCR of the regions' flanks against a genome; the scan, join, fetch and sites of both product passes
#include "h_primers.inc"     // kr_primers_*: in-silico PCR of designed primer pairs against a genome
#include "h_assay.inc"       // kr_assay_*: the link table, the join of the two lists on the device, its rows
#include "h_multiplex.inc"   // kr_multiplex_*: in-silico PCR with all the oligos of a panel in one tube
#include "h_design.inc"      // kr_design_*: a primer pair per region from the model's integers and the primer options
#include "h_panel.inc"       // kr_panel_*: N mutually compatible assays of the designed pairs, selected on the device
#include "h_panel_clean.inc" // kr_panel_sites_*, kr_panel_run_clean: the panel kept free of cross and single products in every genome
#include "h_guides.inc"      // kr_guides_*: a CRISPR guide per region from its template, its outgroup rows and the guide options
#include "h_pgzip.inc"       // one gzip member inflated on several threads (host only)
#include "h_ingest.inc"      // file -> inflate -> parse -> pinned upload buffer (host side)
#include "h_gunzip.inc"      // kr_genome_upload_gzip: the host side of k_gunzip.inc
#include "h_comm.inc"        // multi-GPU exchange: RCCL (or files, for rehearsal) tree reduction of candidates, gather of records
#include "h_text.inc"        // FASTA text parser, IUPAC side-channel scan (host only, no HIP)
#include "h_misc.inc"        // timers, debug entries, FASTA text parser

}  // extern "C"

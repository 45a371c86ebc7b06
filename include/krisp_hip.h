/* krisp_hip.h -- C ABI of libkrisp_hip.so: the MI355X (gfx950) replacement for
 * krisp_fasta's k-mer generation / sort / multi-genome intersection hot path.
 *
 * The reference (grunwaldlab/krisp @ 2024_10_08) is pure Python and has no FFI
 * layer; the seams these entry points replace are (file:line into
 * /root/reference/src/krisp):
 *
 *   kr_genome_upload + kr_genome_sort   krisp_fasta/krisp_fasta.py:16-66 extractSortedKmers
 *        = kstream(...).write():        kstream/kstream.py:250-325 (generate: 617-677, 715-766,
 *                                       805-832) + sortInPlace kstream/kstream.py:83-119 (GNU sort)
 *   kr_genome_fetch_keys                the sorted "{left},{diag},{right}" k-mer file
 *                                       (krisp_fasta.py:241-243), as packed integers
 *   kr_intersect                        krisp_fasta/intersectAmplicons.py:232-310 mergeFiles
 *                                       (pairwise tree of shared.py:321-347 intersectSortedStreams)
 *                                       + filterAlignments.py:31-40 / Amplicon.py:495-521
 *   kr_cands_merge                      the same intersect applied to candidate lists that were
 *                                       produced on other GPUs (no reference counterpart: the
 *                                       reference is single-host)
 *   kr_collect + kr_fetch               the merged / filtered file: one (sequence, genome,
 *                                       multiplicity) triple per label of each line
 *                                       (Amplicon.py:170-187, 330-348)
 *
 * Conventions: plain C, no exceptions cross the boundary, every host buffer is
 * caller-allocated and caller-owned, a negative return value is an error code
 * (text via kr_last_error).  One context = one GPU = one HIP stream; a context
 * is not thread-safe, distinct contexts may be driven from distinct threads.
 * ctypes releases the GIL around each call.
 *
 * KEY FORMAT.  A window w of k = L+D+R bases (k <= 32) is split as
 * left = w[0:L], diag = w[L:L+D], right = w[L+D:k] (kstream.py:805-832 with
 * split=[L,-R]).  Its key is the string left|right|diag, 2 bits per base
 * (A=0 C=1 G=2 T=3), base j in bits 63-2j..62-2j, low bits zero.  Unsigned
 * integer order of keys == the reference's sort order (left, right, diag)
 * (GNU sort -t, -k1,1 -k3,3 with its whole-line last-resort compare).
 *
 * INPUT FORMAT.  `bases` is the ASCII text of the FASTA records of one genome,
 * records separated by ONE '\n' byte (no headers).  Windows never span a
 * separator.  Upper/lower-case ACGT, N/n are handled on the device; IUPAC
 * ambiguity letters and characters outside the reference's COMP_MAP
 * (kstream.py:11-18) must be resolved by the host before upload (the Python
 * host layer does so) -- on the device they simply invalidate their windows.
 */
#ifndef KRISP_HIP_H
#define KRISP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kr_ctx kr_ctx;

/* candidate window: (left,right) prefix present in every genome, plus, per
 * diagnostic column c (c < D <= 16) the set of bases seen at that column in
 * ingroup / outgroup genomes (bit 4c+b). */
typedef struct { uint64_t prefix, in_mask, out_mask; } kr_cand;

/* one distinct k-mer of one genome under a candidate prefix, with its multiplicity */
typedef struct { uint64_t key; uint32_t genome; uint32_t count; } kr_record;

enum {
    KR_OK = 0,
    KR_ERR_HIP = -1,       /* a HIP runtime call failed */
    KR_ERR_PARAM = -2,     /* bad argument (k > 32, D > 16, unknown genome id ...) */
    KR_ERR_CAPACITY = -3,  /* caller buffer too small / hbm budget exceeded */
    KR_ERR_STATE = -4,     /* call sequence error (e.g. intersect before sort) */
    KR_ERR_KEY = -5,       /* kr_scan_special: a surviving window holds a character outside the reference's
                              COMP_MAP -- the reference raises KeyError there (kstream.py:658) */
    KR_ERR_HOST = -6       /* kr_scan_special: bytes >= 0x80 in a candidate window, left to the host layer */
};

enum { KR_SOFT_MAP = 0,    /* lower case -> upper case (krisp_fasta default, krisp_fasta.py:33-43) */
       KR_SOFT_OMIT = 1 }; /* drop windows holding lower case (--omit-soft, krisp_fasta.py:21-31) */

/* stages with device timers (kr_stage_ms) */
enum { KR_ST_PACK = 0, KR_ST_HIST8, KR_ST_REDUCE8, KR_ST_SCATTER1, KR_ST_HIST2, KR_ST_SCAN2, KR_ST_SCATTER2,
       KR_ST_CHUNKS, KR_ST_LOCALSORT, KR_ST_FALLBACK, KR_ST_INTERSECT, KR_ST_COMPACT, KR_ST_COLLECT,
       KR_ST_MERGE, KR_ST_LOCATE, KR_ST_COUNT };   /* one kernel per stage (CHUNKS / COMPACT: two tiny ones) */

kr_ctx*     kr_create(int device, size_t hbm_budget_bytes);   /* budget 0 = no limit */
void        kr_destroy(kr_ctx*);
const char* kr_last_error(kr_ctx*);                            /* ctx may be NULL */

/* Key geometry + soft-mask rule for every genome of this context.
 * max_bases = length of the largest genome that will be uploaded (sizes the
 * radix fan-out so that all genomes share one bucket grid). */
int kr_set_params(kr_ctx*, int L, int D, int R, int softmask_mode, size_t max_bases);

/* Which strands of a window become keys (after kr_set_params, before the first upload).  BOTH is
 * kstream(complements=True), what krisp_fasta uses (krisp_fasta.py:21-43); FORWARD is neither
 * option; CANONICAL is kstream(canonicals=True): min(window, reverse complement) compared as
 * plain strings before the column split (kstream.py:679-694).  One key per window for the latter two. */
enum { KR_STRANDS_BOTH = 0, KR_STRANDS_FORWARD = 1, KR_STRANDS_CANONICAL = 2 };
int kr_set_strands(kr_ctx*, int mode);

/* kstream's --allow (kstream.py:696-713) on the device alphabet: only k-mers made of the bases whose bit
 * is set (A = 1, C = 2, G = 4, T = 8) are kept -- a generalised bad-base mask in the pack kernel.  The host
 * layer uses it when the allowed set holds no letter beyond ACGT(N) and, where both strands are emitted, is
 * closed under complement.  After kr_set_params, before the first upload. */
int kr_set_allow(kr_ctx*, unsigned base_mask);

/* kstream's --sort-cols (kstream.py:83-119: `sort -t, -kN,N ...`, then GNU sort's whole-line compare) as a key layout:
 * the window is cut into fields of widths[0..2] bases in line order (kstream.py:805-832; an empty field has width 0)
 * and the key holds them in the order order[0], order[1], order[2] (a permutation of 0 1 2), so that the unsigned
 * order of the keys is the order of that column list.  After kr_set_params(k, 0, 0, ...) with k = the sum of the
 * widths (the window as ONE field), before the first upload.  A layout moves every field by one shift, at most one
 * distinct left and one distinct right shift; the one order that needs two of a direction (2 1 0 with widths[0] !=
 * widths[2]) is served by rotating the window by a field boundary first (round 5): every permutation is taken.  Such a
 * context sorts and returns keys (kr_genome_sort, kr_genome_fetch_keys); kr_intersect and kr_collect -- whose
 * prefix is the krisp_fasta layout's -- refuse it. */
int kr_set_field_order(kr_ctx*, const int widths[3], const int order[3]);

/* ... and the column orders kr_set_field_order cannot hold (round 6): the key = the n <= 8 listed pieces of the window one after the
 * other, piece i = the widths[i] >= 1 bases at window offset offsets[i]; the pieces partition the window.  For split lists
 * with two or more sizes counted from the end (kstream.py:805-832: the line's columns then leave window order) and column
 * lists that cut the window into more than three blocks.  Same preconditions and the same sort-only context. */
int kr_set_field_pieces(kr_ctx*, int n, const int* offsets, const int* widths);

/* H2D copy of one genome's text + all device allocations it needs. */
int kr_genome_upload(kr_ctx*, int genome_id, const uint8_t* bases, size_t n_bases);
/* pack -> both-strand keys -> MSD radix partition -> LDS sort.  Asynchronous.  Under KR_OPT_LAZY_ORDER (the default) the
 * call ends behind the partition into fine buckets (<= 1600 keys on average, the bucket grid all genomes of a context
 * share); the order INSIDE the buckets -- the reference's `sort` has no such half-way state, kstream.py:83-119 -- is made
 * by the first reader that needs it: kr_genome_fetch_keys / kr_cands_probe for the whole genome, kr_intersect for its
 * anchor genome only (the other genomes' keys are looked up by hashing inside a bucket, in whatever order they lie),
 * kr_collect for the buckets its candidates touch.  Every call returns what it returns with the option off. */
int kr_genome_sort(kr_ctx*, int genome_id);
/* The sort up to its first partition pass only (256 buckets by the key's top byte).  Asynchronous, on a sort lane like a
 * sort.  Such a "coarse" genome can be counted and be an argument of kr_intersect / kr_collect beside at least one sorted ingroup
 * and one sorted outgroup genome with the filter on (one diagnostic column, at most 24 genomes): it then answers
 * the short filtered list of the sorted genomes in one streaming read instead of being partitioned fine and hashed whole.
 * Every other reader of the genome (its keys, the candidate probe, an intersection the route does not take) sorts it fine
 * first, from its resident bases.  Contexts the route does not serve (wide windows, single strands, a custom field order,
 * key-space slices, at most 256 fine buckets) and KR_OPT_COARSE_REST = 0: the call is the full sort. */
int kr_genome_partition(kr_ctx*, int genome_id);
/* upload + sort + sync; returns the number of k-mer records (>= 0). */
int64_t kr_genome_add(kr_ctx*, int genome_id, const uint8_t* bases, size_t n_bases);
int64_t kr_genome_count(kr_ctx*, int genome_id);               /* syncs */
/* Adopt an already sorted key array (the content of a sorted k-mer file the reference or
 * extractSortedKmers wrote, kstream.py:832 lines packed by the host): builds the bucket grid
 * only.  Lets mergeFiles (intersectAmplicons.py:232) run on files.  Returns n. */
int64_t kr_genome_load_sorted(kr_ctx*, int genome_id, const uint64_t* keys, size_t n);
int64_t kr_genome_fetch_keys(kr_ctx*, int genome_id, uint64_t* out, size_t cap);
/* kstream WITHOUT --sort (kstream.py:327-405): the keys of an uploaded genome in stream order -- window
 * by window, a window's reverse complement right after it (KR_STRANDS_BOTH) -- no sort involved.
 * Returns the number of keys (<= 2 n_bases). */
int64_t kr_genome_keys_in_order(kr_ctx*, int genome_id, uint64_t* out, size_t cap);
int     kr_genome_free(kr_ctx*, int genome_id);

/* n-way intersection on the (left,right) prefix over sorted genomes.
 * is_ingroup[i] != 0 marks genome_ids[i] as ingroup.  apply_filter != 0 keeps
 * only candidates with a column whose ingroup and outgroup base sets are
 * disjoint (skipped when D == 0, krisp_fasta.py:265).  Returns #candidates. */
int64_t kr_intersect(kr_ctx*, const int* genome_ids, int n, const uint8_t* is_ingroup,
                     int apply_filter);
/* DNA and RNA genomes in ONE run.  The reference compares k-mers as text, and an RNA genome's are written with U
 * (kstream.py:481-508, 599): 'T' never equals 'U'.  The device alphabet has one code for both, so after this call (on != 0)
 * the diagnostic filter of every call of this context runs in its mode 2 -- a column also passes when its ingroup and
 * outgroup sets share nothing but that code (a superset of the reference's survivors, monotone like the filter itself) --
 * and the host layer, which knows each genome's alphabet, drops the (left,right) pairs that hold the code (no DNA genome
 * and RNA genome share such a pair as text) and decides the passed columns from the survivors' records
 * (krisp_amd/krisp_fasta.py: _mixed_prefix_filter, _mixed_finish).  Any time. */
int     kr_set_mixed_alphabets(kr_ctx*, int on);
int64_t kr_cands_count(kr_ctx*);
int64_t kr_cands_fetch(kr_ctx*, kr_cand* out, size_t cap);
/* Replace the candidate set (sorted by prefix, unique). */
int64_t kr_cands_load(kr_ctx*, const kr_cand* cands, size_t n);
/* candidates := candidates INTERSECT other (sorted, unique), masks OR-ed;
 * other == NULL / n == 0 with apply_filter just filters.  Returns the new count. */
int64_t kr_cands_merge(kr_ctx*, const kr_cand* other, size_t n, int have_other, int apply_filter);
/* candidates := those whose (left,right) prefix EVERY listed (sorted) genome holds, the genomes' diagnostic bases OR-ed into
 * the masks of their side (is_ingroup), the diagnostic filter applied when asked for -- what kr_intersect over these genomes
 * followed by kr_cands_merge would leave, without the genomes' own candidate list in between (for genomes of one side only
 * that list is every prefix they hold).  One step of the reference's merge tree (intersectAmplicons.py:256-307: a merged
 * file against the next genome's file) on candidate lists; the streaming flow of genome sets beyond the GPU's memory uses it
 * for every batch after the first.  Returns the count. */
int64_t kr_cands_probe(kr_ctx*, const int* genome_ids, int n, const uint8_t* is_ingroup, int apply_filter);

/* ---- multi-GPU: one process (one context) per GPU, genomes sharded over the ranks.  Sort and
 * local intersect need no communication; the ONE exchange step is a binary-tree reduction of the
 * candidate lists -- the reference's merge tree (krisp_fasta/intersectAmplicons.py:256-307: pairs of
 * sorted files merged level by level) with GPUs in place of files -- then a broadcast of the
 * survivors for the local kr_collect and a gather of the records on rank 0.  RCCL point-to-point on
 * the context's stream, device buffer to device buffer (xGMI inside a node).  Rendezvous: rank 0
 * calls kr_comm_unique_id and hands the KR_COMM_ID_BYTES bytes to the other ranks any way it likes
 * (a file, an environment variable, MPI, torch.distributed); every rank then calls kr_comm_init.
 * kr_comm_init_dir is the rehearsal transport (the same bytes through files in `dir`) for ranks
 * that share one GPU, where RCCL refuses duplicate devices: tests on a one-GPU box use it. */
#define KR_COMM_ID_BYTES 128
int     kr_comm_unique_id(uint8_t* id);
int     kr_comm_init(kr_ctx*, int rank, int world, const uint8_t* id);
int     kr_comm_init_dir(kr_ctx*, int rank, int world, const char* dir);
int     kr_comm_destroy(kr_ctx*);
int     kr_comm_rank(kr_ctx*);
int     kr_comm_world(kr_ctx*);
/* ranks of the RCCL communicator as RCCL itself counts them (ncclCommCount); 0 without one (no communicator, or
 * the file transport): bench.py prints it, so a line says whether xGMI carried the exchange */
int     kr_comm_rccl_ranks(kr_ctx*);
/* The exchange's deadline.  RCCL's calls have no timeout; every communicator of this library has a watchdog thread
 * (csrc/h_comm.inc): while an exchange call is in progress it polls ncclCommGetAsyncError, and on an asynchronous error or
 * `seconds` after the call began it aborts the communicator (ncclCommAbort) -- the call returns KR_ERR_STATE / KR_ERR_HIP,
 * later exchange calls KR_ERR_STATE; a call that still does not return ends the process with status 124.  The file
 * transport waits `seconds` for a message.  Default: the environment's KRISP_COMM_TIMEOUT, else 600.  (The reference's tree
 * runs inside one multiprocessing pool, intersectAmplicons.py:256-307: a dead worker raises there.) */
int     kr_comm_set_timeout(kr_ctx*, int seconds);
int     kr_comm_barrier(kr_ctx*);                               /* syncs the stream, then all ranks meet */
/* vals[0..n) reduced over all ranks, n <= 8: op 0 = sum, 1 = max; the result on every rank */
int     kr_comm_allreduce(kr_ctx*, double* vals, int n, int op);
/* n bytes of every rank -> every rank: out[r * n .. (r + 1) * n) = rank r's (the same n on every rank); small side
 * data of the flow (windows with IUPAC letters, krisp_fasta.py), not candidate lists */
int     kr_comm_allgather(kr_ctx*, const void* mine, size_t n, void* out);
/* candidates := those present on EVERY rank, masks OR-ed (filtered when apply_filter), on rank 0;
 * returns the count on rank 0, 0 elsewhere (the other ranks' sets are spent) */
int64_t kr_cands_reduce(kr_ctx*, int apply_filter);
int64_t kr_cands_bcast(kr_ctx*);                                /* rank 0's candidates -> every rank */
int64_t kr_records_gather(kr_ctx*);                             /* every rank's kr_collect records -> rank 0 (kr_fetch) */

/* For every candidate and every listed genome: its distinct keys + multiplicities.
 * Returns #records; kr_fetch returns them ordered by (key, position of the genome in genome_ids). */
int64_t kr_collect(kr_ctx*, const int* genome_ids, int n);
int64_t kr_fetch(kr_ctx*, kr_record* out, size_t cap);

/* ---- wide windows: amplicons longer than one 64-bit key (L+D+R > 32, or D > 16) ------------
 * The reference has no length limit (its k-mers are text: krisp_fasta.py:21-43 passes any
 * kmers= / split= to kstream, README.md:201-232 runs --conserved 30 --amplicon 100).  Here 1 <= L, R <=
 * KR_WIDE_MAX_FLANK and L+D+R <= KR_WIDE_MAX_K.  The library sorts and intersects with the 64-bit
 * pipeline the `left` spectrum, the `right` spectrum, then exact composite keys
 * rank(left):rank(right) (a flank longer than 32 bases is itself ranked through two spectra and
 * their combinations: three more sorts), applies the diagnostic filter
 * (Amplicon.py:495-521) and returns, for every surviving (left,right) group, where its member
 * windows lie; the host cuts the text of those windows out of the genomes it already holds.
 * Replaces, for such geometries, the same calls as kr_genome_sort + kr_intersect + kr_collect:
 * extractSortedKmers + mergeFiles + filterAlignments (krisp_fasta.py:237-272). */
#define KR_WIDE_MAX_K 1024
#define KR_WIDE_MAX_FLANK 256
/* one member window of a surviving group: cand = the group's number (its rank in (left,right) order
 * under KR_OPT_WIDE_ORDERED = 1; else any number, the same for all members of a group),
 * genome = index into the genome_ids of kr_wide_run, pos = base offset of the window in the
 * uploaded text, strand = 1 when the member is the reverse complement of that window */
typedef struct { uint32_t cand, genome, pos, strand; } kr_wide_hit;
int     kr_set_params_wide(kr_ctx*, int L, int D, int R, int softmask_mode, size_t max_bases);
/* genomes: kr_genome_upload.  Returns the number of hits (grouped by cand, ascending).
 * With a communicator (kr_comm_init*) the call is collective: every rank passes ITS genomes (ids unique over
 * the ranks), the flank spectra, the group list and the kept groups' mask words are exchanged inside;
 * rank 0 ends with the hits of all ranks (genome = the caller's id, not an index; no order), the others with their own. */
int64_t kr_wide_run(kr_ctx*, const int* genome_ids, int n, const uint8_t* is_ingroup, int apply_filter);
enum { KR_WIDE_DICT_LEFT = 0,   /* u64: lefts present in all genomes, sorted (L > 32: their rank:rank combinations) */
       KR_WIDE_DICT_RIGHT = 1,  /* u64: rights present in all genomes, sorted (R > 32: likewise) */
       KR_WIDE_GROUPS = 2,      /* u64: composite keys of the groups present in all genomes (before the filter) */
       KR_WIDE_HITS = 3,        /* kr_wide_hit */
       KR_WIDE_COUNTS = 4,      /* u64 per genome of the last run: its k-mer records (2 x valid windows) */
       KR_WIDE_NGROUPS = 6,     /* u64 x 1: the (left,right) groups present in all genomes (before the filter).  With L = R
                                   (and KR_OPT_WIDE_ORDERED = 0) KR_WIDE_GROUPS lists one group of every mirror pair
                                   (a:b) / (b:a) only -- the two are decided alike -- and a hit of the unlisted one
                                   carries the listed one's number with bit 31 set */
       KR_WIDE_BATCH_USED = 7,  /* u64 x 1: genomes per batch of the sort + intersect phases of the last run (0 = all at once): a genome set
                                   whose sorted keys do not fit the device goes through the phases in batches (kr_wide_run) */
       KR_WIDE_LOCATED = 8,     /* u64 x 1: member windows the locate pass of the last run LISTED (round 6: a 16-byte entry per member
                                   window instead of a group number per window start, when the members are few); 0 = the dense form ran */
       KR_WIDE_KEYS_LISTED = 9, /* u64 x 1: composite keys the last run kept as per-genome LISTS (round 6: 16 bytes per window that has a key --
                                   both flanks in the dictionaries -- instead of 16 bytes per window start, when such windows are few); 0 = dense */
       KR_WIDE_SLOT_BITS = 5 }; /* u64 x 7 (left pieces 0..2, right pieces 0..2, groups): bucket bits of the dictionary's
                                   one-sector slot table in the last run, 0 = looked up through index + sorted keys,
                                   255 = through minimizer buckets (KR_OPT_WIDE_ORDERED = 0), 254 = not built: with L = R the
                                   rights present in every genome are the reverse complements of the lefts, and a right
                                   takes the number of that left */
int64_t kr_wide_fetch(kr_ctx*, int what, void* out, size_t cap_bytes);   /* returns #elements; out == NULL: size query */
/* The member windows of the latest kr_wide_run as text, cut on the device from the genomes' uploaded bases: row i = the
 * L+D+R letters of hit i (KR_WIDE_HITS order) in line order left|diag|right, upper case, the reverse complement for a
 * strand-1 member -- what the reference writes as one line of its merged file (Amplicon.py:330-348), so the host needs no
 * copy of the genomes to render long amplicons (kr_render_windows).  One context (no communicator of more than one
 * rank: the hits of other ranks' genomes have no bases here).  Returns the number of rows; rows == NULL: size query. */
int64_t kr_wide_fetch_windows(kr_ctx*, uint8_t* rows, size_t cap_bytes);

/* ---- locations: where the windows of the surviving groups lie (krisp_fasta --out_locations) ------------------------
 * No seam inside krisp_fasta: the upstream project's misc_scripts/grepFastaSequence.py re-reads the FASTA files and
 * str.find()s every sequence and its reverse complement, record by record.  Here each genome is scanned once on the
 * device (csrc/k_locate.inc) against a hash table of the groups' (left, right) flank texts, with the window rules of
 * kstream.py:617-677 (no N / n, no separator, no lower case under omit-soft, upper case otherwise; the reverse strand by
 * COMP_MAP, kstream.py:11-18), for packed and wide geometries alike.
 *
 * kr_set_params_locate: a context for this pass only -- genomes go up through kr_genome_upload / _upload_text /
 * _upload_bgzf / _upload_gzip with no sort plan (kr_genome_sort refuses them); 0 <= L, R <= KR_WIDE_MAX_FLANK,
 * 1 <= L+D+R <= KR_WIDE_MAX_K, max_bases < 2^33. */
int     kr_set_params_locate(kr_ctx*, int L, int D, int R, int softmask_mode, size_t max_bases);
/* the groups' flanks: ngroups rows of L+R bytes (left then right, upper case, U written as T), row i = group i.  Builds the
 * open-addressing table (a power of two >= 2 ngroups slots) and the membership bitmap the scan keeps in LDS.  Returns the
 * number of slots; KR_ERR_PARAM when two rows are equal, KR_ERR_CAPACITY when the table does not fit. */
int64_t kr_locate_table(kr_ctx*, const uint8_t* flanks, uint64_t ngroups);
/* one hit: the group (row of kr_locate_table), strand 0 = the window as written ('+'), 1 = its reverse complement ('-'),
 * pos = the window's first base in the uploaded bases (separators counted) */
typedef struct { uint32_t group, strand; uint64_t pos; } kr_loc_hit;
/* scans uploaded genome `id` against the table: returns the number of hits, kept on the device for kr_locate_fetch, in
 * position order, '+' before '-' at one position (counted, scanned, written: the same order on every run) */
int64_t kr_locate_scan(kr_ctx*, int id);
int64_t kr_locate_fetch(kr_ctx*, kr_loc_hit* out, size_t cap);
/* the hits' windows as text, cut on the device from the scanned genome (still uploaded): row i = the L+D+R letters of hit
 * i, upper case, the reverse complement for strand 1 -- the k-mer the alignment lists (kstream.py:622-659).  Returns the
 * number of rows; rows == NULL: size query */
int64_t kr_locate_windows(kr_ctx*, uint8_t* rows, size_t cap_bytes);
/* the positions of the record separators ('\n') of uploaded genome `id`, ascending: the host maps a position to (record,
 * offset) with them without fetching the bases.  Returns their number; out == NULL: the number only */
int64_t kr_locate_seps(kr_ctx*, int id, uint64_t* out, size_t cap);

/* ---- near matches: the windows within Hamming distance M of an ingroup window (krisp_fasta --out_near) ---------------
 * No seam in the reference: its k-mer intersection sees a window only where both conserved flanks are equal base for
 * base.  This pass reports, for every genome, every window (kstream.py:617-677's window rules, both strands through
 * COMP_MAP, as the locate pass) that differs from a target -- the L+D+R letters of an ingroup window of a diagnostic
 * region -- in at most M columns, wherever it lies.  It runs in the locate context (kr_set_params_locate; the genome is
 * uploaded by the same entry points, kr_locate_seps lists its records), on the device in csrc/k_near.inc: pigeonhole
 * seeds (the columns cut into M + 1 pieces; a near window equals the target in one of them) filter, a byte-by-byte
 * comparison decides.
 *
 * kr_near_table: ntargets rows of L+D+R bytes (upper case, U written as T), row i = target i; 0 <= mismatches <= 3 and
 * mismatches < L+D+R (KR_ERR_PARAM otherwise).  Builds the text of every target and its reverse complement, the table of
 * (piece, hash of the piece's bytes) -> the range of the entry list with that piece, and the membership bitmap the scan
 * keeps in LDS.  Equal rows are not refused (kr_locate_table refuses equal flank pairs): each stays a target of its own,
 * and a window near one is a hit of each.  Returns the number of slots; KR_ERR_CAPACITY for 2^24 targets or more, or a
 * table that does not fit. */
int64_t kr_near_table(kr_ctx*, const uint8_t* targets, uint64_t ntargets, int mismatches);
/* one hit: the target (row of kr_near_table), strand 0 = the window as written ('+'), 1 = its reverse complement ('-'),
 * the columns in which the strand's window differs from the target, those of them in the conserved flanks (the first L
 * and the last R columns of the target), pos = the window's first base in the uploaded bases (separators counted) */
typedef struct { uint32_t target; uint8_t strand, mismatches, flank_mismatches, pad; uint64_t pos; } kr_near_hit;
/* scans uploaded genome `id` against the table: returns the number of hits, kept on the device for kr_near_fetch, in
 * position order (at one position: by seed piece, then by the table's entry order; a (target, strand, pos) occurs once).
 * Counted, scanned, written: the same bytes on every run.  KR_ERR_CAPACITY for 2^32 hits or more, or hits that do not fit. */
int64_t kr_near_scan(kr_ctx*, int id);
int64_t kr_near_fetch(kr_ctx*, kr_near_hit* out, size_t cap);
/* the hits' windows as text, as kr_locate_windows gives the locate pass's: row i = the L+D+R letters of hit i, upper
 * case, the reverse complement for strand 1.  Returns the number of rows; rows == NULL: size query */
int64_t kr_near_windows(kr_ctx*, uint8_t* rows, size_t cap_bytes);

/* ---- predicted PCR products of the regions' flanks (krisp_fasta --out_products) ---------------------------------------
 * No seam in the reference.  The conserved flanks of a long amplicon are primer regions; this pass reports, for every
 * genome, every pair of SITES that would amplify: a site of a text X is a window of len(X) bases (the locate pass's window
 * rules) within Hamming distance M of X.  A product of the pair (A, B) on one record is a site of A at s1 and a site of B
 * at s2 (strand 0), or a site of rc(B) at s1 and a site of rc(A) at s2 (strand 1, rc through COMP_MAP), with
 * s2 >= s1 + the first site's length and s2 + the second site's length - s1 <= max_product; whatever lies between the
 * sites is not looked at.  It runs in the locate context (kr_set_params_locate: its L and R are the lengths of the left
 * and right texts, D plays no part), on the device in csrc/k_products.inc: pigeonhole seeds per text length filter, a
 * byte comparison decides, the sites of one genome are joined in position order.
 *
 * kr_products_table: nleft rows of L bytes and nright rows of R bytes (upper case, U written as T; equal rows are not
 * refused, each stays a text of its own), npairs rows of two u32 (row of left, row of right): pair p is what a product's
 * `pair` names.  0 <= mismatches <= 3 and mismatches < min(L, R), max_product >= L + R, indices in range and no pair
 * twice (KR_ERR_PARAM otherwise).  Returns the number of slots of the seed table; KR_ERR_CAPACITY for 2^24 texts or
 * more, or a table that does not fit. */
int64_t kr_products_table(kr_ctx*, const uint8_t* left, uint64_t nleft, const uint8_t* right, uint64_t nright,
                          const uint32_t* pairs, uint64_t npairs, int mismatches, uint32_t max_product);
/* one site: entry 2 i = left text i as written, 2 i + 1 = its reverse complement, 2 nleft + 2 j = right text j,
 * 2 nleft + 2 j + 1 = its reverse complement; the columns in which the window differs from the entry's text, those of
 * them in the min(5, length) columns at the primer's 3' end (the last columns of a left text and the first of a right
 * one, as the amplicon's strand reads them); pos = the window's first base in the uploaded bases */
typedef struct { uint64_t pos; uint32_t entry; uint8_t mismatches, end_mismatches; uint16_t pad; } kr_product_site;
/* one product: pos = the first base of its first site, length = to the last base of its second site, pair = row of
 * `pairs`, strand 0 / 1 as above, the mismatches of the left text's site (A or rc(A)) and the right text's, and those of
 * them at the 3' ends */
typedef struct { uint64_t pos; uint32_t length, pair; uint8_t strand, left_mm, right_mm, left_end_mm, right_end_mm, pad[3]; } kr_product_hit;
/* scans uploaded genome `id`: lists its separators, its sites (position order; at one position by text length, seed
 * piece and the table's entry order; an (entry, pos) occurs once), their records, and joins them.  Returns the number of
 * products, kept on the device with the sites.  Counted, scanned, written: the same bytes on every run.
 * KR_ERR_CAPACITY for 2^32 sites or products or more, or lists that do not fit. */
int64_t kr_products_scan(kr_ctx*, int id);
/* the products of the latest scan in (pos, length, strand, pair) order */
int64_t kr_products_fetch(kr_ctx*, kr_product_hit* out, size_t cap);
/* the sites of the latest scan, as the device lists them.  Returns their number; out == NULL: the number only */
int64_t kr_products_sites(kr_ctx*, kr_product_site* out, size_t cap);

/* ---- predicted PCR products of designed primer pairs (krisp_fasta --out_primer_products) ------------------------------
 * The product pass above for texts that each have a length of their own, 10 .. 60 letters: the primers kr_design_run
 * picks lie anywhere inside their flanks and are of every length in --primer_size.  The definition is the product pass's
 * with the entry's own length in the place of L and R: a site of entry e is a window of len(e) bases (the locate pass's
 * window rules) within Hamming distance M of its text, the end mismatches are counted in the 5 columns at the primer's
 * 3' end, and a product of the pair (A, B) is a site of A at s1 and of B at s2 (strand 0) or of rc(B) at s1 and of rc(A)
 * at s2 (strand 1) on one record with s2 >= s1 + len(first) and s2 + len(second) - s1 <= max_product.  With all left
 * texts of one length and all right texts of one length the sites and products are kr_products_*'s, byte for byte.  It
 * runs in the locate context (kr_set_params_locate: only the soft-mask mode plays a part), on the device in
 * csrc/k_primers.inc: every entry is seeded by the first smin columns of its text as it reads on the forward strand
 * (smin = the shortest text of the table), a byte comparison over the entry's whole length decides.
 *
 * kr_primers_table: the texts one after the other (upper case, U written as T; left texts first; a left text is the
 * primer as it reads on the template, a right text the template's text under the right primer), text t =
 * text[offsets[t] - offsets[0], offsets[t + 1] - offsets[0]), nleft + nright + 1 ascending offsets; npairs rows of two
 * u32 (row of left, row of right).  KR_ERR_PARAM for a length outside 10 .. 60, mismatches outside 0 .. 3, a pair index
 * out of range, a pair twice, a max_product shorter than some pair's two texts together, a null table.  Returns the
 * number of slots of the seed table; KR_ERR_CAPACITY for 2^24 texts or more, or a table that does not fit. */
int64_t kr_primers_table(kr_ctx*, const uint8_t* text, const uint32_t* offsets, uint64_t nleft, uint64_t nright,
                         const uint32_t* pairs, uint64_t npairs, int mismatches, uint32_t max_product);
/* scans uploaded genome `id` as kr_products_scan does: its separators, its sites (position order; at one position by
 * seed piece and the table's entry order; an (entry, pos) occurs once), their records, the join.  Returns the number of
 * products.  Counted, scanned, written: the same bytes on every run.  KR_ERR_STATE "kr_primers_table first" without a
 * table; KR_ERR_CAPACITY for 2^32 sites or products or more, or lists that do not fit. */
int64_t kr_primers_scan(kr_ctx*, int id);
/* the products of the latest scan in (pos, length, strand, pair) order */
int64_t kr_primers_fetch(kr_ctx*, kr_product_hit* out, size_t cap);
/* the sites of the latest scan, as the device lists them.  Returns their number; out == NULL: the number only */
int64_t kr_primers_sites(kr_ctx*, kr_product_site* out, size_t cap);
/* the products of the latest scan counted on the device (krisp_fasta --primer-candidates; csrc/k_primers.inc:
 * k_prim_tally), eight uint32 per pair of the table: out[8 p + m] = pair p's products with left_mm + right_mm = m, m = 0 ..
 * 6, out[8 p + 7] = those with left_end_mm = right_end_mm = 0.  The list on the device is only read: no product comes to
 * the host.  Integer adds: the same bytes on every run.  cap counts uint32; returns 8 npairs.  Zeros without a launch where
 * the table has no pair or the scan found no product; KR_ERR_STATE "kr_primers_scan first" before a scan of the standing
 * table, KR_ERR_CAPACITY for a buffer below 8 npairs. */
int64_t kr_primers_tally(kr_ctx*, uint32_t* out, size_t cap);

/* ---- a primer pair per region (krisp_fasta --design-primers) -----------------------------------------------------------
 * Replaces no seam of the reference: it designs with the third-party Primer3.  This is a small designer of its own whose
 * every figure is an integer (DESIGN §15 has the definition): nearest-neighbour melting temperatures in mK, the filters of
 * the command line's primer options, a duplex figure over ungapped antiparallel alignments in the place of Primer3's *_TH
 * values, the passing pair of least penalty with a fixed tie rule.  It runs on the device in csrc/k_design.inc, a
 * wavefront per region, in any context (no genome, no parameters of another pass are needed).
 *
 * kr_design_table: the model's integers (krisp_amd/thermo.py holds them; the library has no copy) and the options.
 * Bases are coded A C G T = 0 1 2 3; nn_*[4 x + y] is the step xy read 5'->3', term_*[x] a terminal base; dh in cal/mol,
 * ds in 0.001 cal/(mol K), temperatures in mK, gc_lo / gc_hi in percent.  KR_ERR_PARAM unless 10 <= size_lo <= size_hi
 * <= 60, every range is ordered, 0 <= gc_clamp <= size_lo, max_end_gc >= 0, and the model keeps every duplex's dH and dS
 * negative (every step's dH + two terminals < 0, conc + two terminals <= -4000). */
typedef struct {
    int32_t nn_dh[16], nn_ds[16], term_dh[4], term_ds[4];
    int32_t sym_ds, salt_ds, conc_ds, conc_self_ds;
    int32_t size_lo, size_hi, tm_lo, tm_hi, tm_opt, gc_lo, gc_hi, amp_lo, amp_hi, max_sec, gc_clamp, max_end_gc;
} kr_design_params;
int kr_design_table(kr_ctx*, const kr_design_params* params);
/* one region's answer, 64 bytes: found = 1 and the pair, or all zero.  Starts are template indices of the leftmost base
 * (the right primer is the reverse complement of template[right_start, right_start + right_len)); temperatures and
 * duplex figures in mK (0: no run of two pairs); *_gc = the number of G and C; penalties in 1/1000 */
typedef struct {
    uint32_t found, product_size, pair_penalty;
    uint16_t left_start, left_len, right_start, right_len;
    int32_t left_tm, right_tm;
    uint16_t left_gc, right_gc;
    uint32_t left_penalty, right_penalty;
    int32_t left_self_any, left_self_end, right_self_any, right_self_end, pair_any, pair_end;
} kr_design_record;
/* nregions templates of L + D + R bytes each (upper case, U written as T; any other letter than A C G T removes the
 * candidates that cover it), in batches so that any count fits.  Returns the number of regions with a pair.
 * KR_ERR_PARAM for a flank above 1023 or a template above 2047 bytes; KR_ERR_CAPACITY when the candidate tables of one
 * region (4 bytes per start and length of either flank) exceed the LDS of a workgroup. */
int64_t kr_design_run(kr_ctx*, const uint8_t* templates, uint64_t nregions, int L, int D, int R);
/* the records of the latest run, one per region in the order given */
int64_t kr_design_fetch(kr_ctx*, kr_design_record* out, size_t cap);
/* The hairpin check (krisp_fasta --design-primers --hairpins): with it a candidate whose hairpin figure lies
 * above max_sec is no candidate, as one whose self_any does.  The figure: over every fold c = i + j of the primer read
 * 5'->3' and every maximal run of at least two Watson-Crick pairs (i, c - i) with j - i >= 4, the Tm of the run's bases on
 * the 5' arm as a duplex's -- steps, both terminals, salt per step -- with loop_ds[l] in the place of the concentration
 * term and no symmetry term, l = the bases the innermost pair encloses, 3 .. 56; 0 without such a run.  loop_ds is indexed
 * by l (krisp_amd/thermo.py holds the values; the library has no copy); the entries 3 .. 56 are read.
 * kr_design_hairpins: after kr_design_table (KR_ERR_STATE before one); NULL switches the check off again, and so does every
 * later kr_design_table.  KR_ERR_PARAM unless for every l in 3 .. 56 |loop_ds[l]| < 100000 and
 * max(nn_ds) + salt_ds + 2 max(term_ds) + loop_ds[l] <= -4000 (the table's own: every stem's dS stays at -4000 or below). */
typedef struct {
    int32_t loop_ds[64];
} kr_hairpin_params;
int kr_design_hairpins(kr_ctx*, const kr_hairpin_params* params);
/* the hairpin figures of the latest run's pairs in mK: out[2 r] the left and out[2 r + 1] the right primer's of region r,
 * 0 and 0 for a region without a pair; cap counts int32.  Returns the number of int32 written, two per region.
 * KR_ERR_STATE when that run had the check off.  kr_design_record does not change with the check. */
int64_t kr_design_fetch_hairpins(kr_ctx*, int32_t* out, size_t cap);
/* The shortlist (krisp_fasta --primer-candidates): a region's passing pairs are kr_design_run's, under the
 * hairpin check too; in ascending (pair_penalty, left_start, left_len, right_start, right_len) order -- a total order, the
 * key holds the positions -- the first `top` of them are the region's shortlist, rank 1 the pair kr_design_run picks.  It
 * runs in csrc/k_design.inc (k_design_top): k_design's branch-and-bound with the top-th least accepted key as the bound.
 * kr_design_run_top: kr_design_run's arguments, checks and batches, 1 <= top <= 8 (KR_ERR_PARAM otherwise).  Returns the
 * number of regions with a pair.  The records and the state are its own: a kr_design_run neither changes nor satisfies
 * them, and the other way round; kr_design_table drops both. */
int64_t kr_design_run_top(kr_ctx*, const uint8_t* templates, uint64_t nregions, int L, int D, int R, int top);
/* the records of the latest kr_design_run_top, region-major: out[r top + j] = the pair of rank j + 1 of region r, with every
 * figure of a kr_design_record; all zero where the region has fewer pairs.  Returns nregions * top */
int64_t kr_design_fetch_top(kr_ctx*, kr_design_record* out, size_t cap);
/* ... and their hairpin figures: out[2 (r top + j)] the left and out[2 (r top + j) + 1] the right primer's; KR_ERR_STATE
 * when that run had the check off */
int64_t kr_design_fetch_top_hairpins(kr_ctx*, int32_t* out, size_t cap);

/* ---- N mutually compatible assays of the designed pairs (krisp_fasta --panel) -------------------------------------------
 * Replaces no seam of the reference, which selects nothing.  Of ncand candidates in the caller's order -- a template of W
 * bytes and a primer pair each, the pair as four uint16: left_start, left_len, right_start, right_len, as kr_design_record
 * names them -- the first `size` that are different loci (no window of 16 bases A C G T shared with an earlier member's
 * template, on either strand) and do not clash (every duplex figure of a candidate's primer, in the left role, with a
 * member's primer at most max_sec): DESIGN §23 has the definition.  It runs on the device in csrc/k_panel.inc, a launch per
 * round and one synchronise, with the model and max_sec of the latest kr_design_table (KR_ERR_STATE before one).  All
 * candidates are resident at once: KR_ERR_CAPACITY when templates and state (W + 18 bytes a candidate) do not fit.
 * KR_ERR_PARAM for W outside 1 .. 2047, a primer outside 10 .. 60 bases or outside its template, size outside 1 .. 64, a
 * null pointer with ncand > 0.  Returns the number of members, 0 .. size; ncand = 0: 0 without a launch. */
int64_t kr_panel_run(kr_ctx*, const uint8_t* templates, const uint16_t* pairs, uint64_t ncand, int W, int size);
/* a member, in order of acceptance: its position among the candidates, the greatest figures of its primers against the
 * primers of the members before it in mK (0 and 0 for the first), and how many candidates it dropped as the same locus
 * ([0]) and for a clash ([1]) */
typedef struct { uint32_t position; int32_t cross_any, cross_end; uint32_t dropped[2]; } kr_panel_member;
/* the members of the latest run (KR_ERR_STATE before one) */
int64_t kr_panel_fetch(kr_ctx*, kr_panel_member* out, size_t cap);
/* two bytes per candidate of the latest run: fate (1 member, 2 dropped as the same locus, 3 dropped for a clash, 0 still
 * alive when the panel was full; after kr_panel_run_clean also 4 dropped for a cross product with a member, 5 a primer
 * that primes with itself) and by (the 1-based member that dropped it, a member's own number, 0 for fates 0 and 5); cap
 * counts bytes.  Returns the number of bytes written (KR_ERR_STATE before a run) */
int64_t kr_panel_fates(kr_ctx*, uint8_t* out, size_t cap);

/* ---- a CRISPR guide per region (krisp_fasta --out_guides) ---------------------------------------------------------------
 * Replaces no seam of the reference, which picks no guide.  For every region the protospacer window of guide_size columns
 * of the region's template that lies next to the enzyme's PAM / PFS, passes the GC and poly-X filters and differs most
 * from the region's outgroup rows (DESIGN §18 has the definition, every figure an integer).  It runs on the device in
 * csrc/k_guides.inc, a wavefront per region, in any context (no genome, no parameters of another pass are needed).
 *
 * kr_guides_table: the options.  pam5 / pam3 hold one 4-bit IUPAC mask per motif letter, read 5'->3' on the guide's
 * strand (A = 1, C = 2, G = 4, T = 8; N = 15), pam5_len / pam3_len letters of them count (0: no motif on that side);
 * gc_lo / gc_hi in percent.  KR_ERR_PARAM unless 12 <= guide_size <= 40, both lengths lie in 0 .. 8 and every mask that
 * counts in 1 .. 15. */
typedef struct {
    int32_t guide_size, pam5_len, pam3_len;
    uint8_t pam5[8], pam3[8];
    int32_t gc_lo, gc_hi, min_mismatches;
} kr_guide_params;
int kr_guides_table(kr_ctx*, const kr_guide_params* params);
/* one region's answer, 32 bytes: found = 1 and the guide, or all zero but `candidates`.  strand 0: the protospacer reads
 * template[start, start + guide_size), 1: its reverse complement; min / sum_mismatches = the least and the total number of
 * protospacer columns at which an outgroup row holds another of A C G T than the template (guide_size and 0 without
 * outgroup rows); gc = the number of G and C; candidates = the windows and strands that passed every filter */
typedef struct {
    uint32_t found, strand, start, min_mismatches, sum_mismatches, gc, candidates, pad;
} kr_guide_record;
/* rows: byte rows of K letters each (upper case, U written as T); the rows row_off[r] .. row_off[r + 1] - 1 are region r's,
 * the first of them its template and the others its outgroup rows (any number, none included); bounds[2 r], bounds[2 r + 1]
 * = the columns [lo, hi) the guide with its PAM must lie in; L, D = the template's left flank and diagnostic stretch (the
 * tie rule prefers the window centred on column L + D / 2).  In batches so that any count fits.  Returns the number of
 * regions with a guide.  KR_ERR_STATE before kr_guides_table; KR_ERR_PARAM for K < guide_size, K > 2047, L + D > K, a null
 * pointer, lo > hi, hi > K, row_off[0] != 0, a region without a row or with more than 2^26 of them; KR_ERR_CAPACITY when
 * one region's tables exceed the LDS of a workgroup. */
int64_t kr_guides_run(kr_ctx*, const uint8_t* rows, const uint64_t* row_off, const uint32_t* bounds, uint64_t nregions, int K,
                      int L, int D);
/* the records of the latest run, one per region in the order given (KR_ERR_STATE before a run) */
int64_t kr_guides_fetch(kr_ctx*, kr_guide_record* out, size_t cap);
/* the shortlist of krisp_fasta --guide-candidates: as kr_guides_run -- the same arguments, checks and batches --
 * for the `top` best candidates of every region in the order of the definition, 1 <= top <= 8 (KR_ERR_PARAM otherwise), on
 * the device in k_guides_top.  Returns the number of filled slots.  kr_guides_fetch_top gives nregions * top records,
 * region-major: slot j of a region is its candidate of rank j + 1, and equals kr_guides_run's record for j = 0; a slot
 * beyond the region's candidates is zero but `candidates`, which in every slot is the region's full count.  A state of its
 * own: kr_guides_fetch is not satisfied by a top run, nor kr_guides_fetch_top by kr_guides_run (KR_ERR_STATE). */
int64_t kr_guides_run_top(kr_ctx*, const uint8_t* rows, const uint64_t* row_off, const uint32_t* bounds, uint64_t nregions, int K,
                          int L, int D, int top);
int64_t kr_guides_fetch_top(kr_ctx*, kr_guide_record* out, size_t cap);

/* ---- the picked guides searched in every genome (krisp_fasta --out_guide_hits) -----------------------------------------
 * No seam in the reference.  The specificity pass of the guides: for every genome, every window (the locate pass's window
 * rules, both strands) that differs from a guide's protospacer in at most M columns, with the columns that differ and
 * whether the PAM / PFS motifs lie beside it.  DESIGN §19 holds the definition (entries, staging, the column mask's
 * orientation, the motifs' index rules on both strands, need_pam); tests/guide_hits_reference.py restates it.  It runs in
 * the locate context (kr_set_params_locate with L+D+R = the protospacer length G: only the sum and the soft-mask mode play
 * a part; the genome is uploaded by the same entry points, kr_locate_seps lists its records), with a state of its own:
 * a near-match table of the same context is not disturbed.  On the device it is the near pass's scan itself (k_near_scan
 * over the guides' table: pigeonhole seeds filter, a byte comparison decides), then csrc/k_guide_hits.inc: a per-hit step
 * (csrc/ghit_step.inc), a thread per hit, that reads the window and the motifs' neighbours from the genome's bytes, every
 * index bounds-checked, and under need_pam an order-keeping selection of the hits with both motifs.
 *
 * The table: nguides rows of G bytes, each of A, C, G, T, row i = guide i (equal rows stay guides of their own);
 * 0 <= mismatches <= 3; pam5 / pam3 = the motifs in IUPAC letters (either case, U as T), read 5'->3' on the guide's strand,
 * at most 8 letters, NULL or "" = none; need_pam != 0: a hit counts only where both motifs match.  Returns the number of
 * slots of the seed table.  KR_ERR_PARAM for G outside 12 .. 40, mismatches outside 0 .. 3, a text byte other than A, C,
 * G, T, a motif of more than 8 letters or with a letter outside the IUPAC code, null texts with nguides != 0 (an earlier
 * table stays as it was); KR_ERR_CAPACITY for 2^24 guides or more, or a table that does not fit. */
int64_t kr_guide_hits_table(kr_ctx*, const uint8_t* texts, uint64_t nguides, int mismatches, const char* pam5, const char* pam3,
                            int need_pam);
/* one hit, 24 bytes: the guide (row of the table), strand 0 = the window as written ('+'), 1 = its reverse complement
 * ('-'), the number of columns that differ, pam bit 0 = the 5' motif matches and bit 1 = the 3' motif (an empty motif
 * matches), pos = the window's first base in the uploaded bases (separators counted), columns bit c = guide column c
 * differs, counted 5'->3' on the protospacer (window column G - 1 - c on '-') */
typedef struct { uint32_t guide; uint8_t strand, mismatches, pam, pad; uint64_t pos; uint64_t columns; } kr_guide_hit;
/* scans uploaded genome `id` against the table: returns the number of hits, kept on the device for the fetch, in position
 * order (at one position: by seed piece, then by the table's entry order; a (guide, strand, pos) occurs once).  Counted,
 * scanned, written: the same bytes on every run.  No guides, or a genome shorter than G: 0 without a launch.  KR_ERR_PARAM
 * before a table; KR_ERR_CAPACITY for 2^32 hits or more (counted before need_pam's selection), or hits that do not fit. */
int64_t kr_guide_hits_scan(kr_ctx*, int id);
int64_t kr_guide_hits_fetch(kr_ctx*, kr_guide_hit* out, size_t cap);
/* the hits' windows as text, as kr_near_windows gives the near pass's: row i = the G letters of hit i, upper case, the
 * reverse complement for strand 1 -- the window as the guide's strand reads it.  Returns the number of rows; rows == NULL:
 * size query */
int64_t kr_guide_hits_windows(kr_ctx*, uint8_t* rows, size_t cap_bytes);
/* the hits of the latest kr_guide_hits_scan (after need_pam's selection) counted on the device, for a caller that wants the
 * counts and not the hits: out[4 * guide + mismatches] = the number of such hits, 4 * nguides counters (a scan holds fewer
 * than 2^32 hits).  Returns 4 * nguides.  The list is only read: the fetch, the windows and kr_assay_join give the same
 * bytes after it as before it.  No guides or no hits: zeros without a launch.  KR_ERR_STATE before a scan or after a new
 * table; KR_ERR_CAPACITY for cap < 4 * nguides. */
int64_t kr_guide_hits_tally(kr_ctx*, uint32_t* out, size_t cap);

/* ---- guide hits with a bulge: in the locate context of kr_guide_hits_*, with a state of its own (a table and
 * a scan of either pass do not disturb the other's).  A bulged hit of size b is a window of G + b bases (a DNA bulge: b
 * bases of the genome have no partner) or G - b bases (an RNA bulge: b letters of the guide have none) that lies within
 * `mismatches` columns of a guide's protospacer, or of its reverse complement, when cut at one place inside the guide:
 * one contiguous bulge, never at an end.
 * kr_guide_bulges_table: as kr_guide_hits_table, with bulges = the largest b (1 or 2).  The seeds are the guides' halves of
 * (G - bulges) / 2 letters, searched by the near-match scan.  Returns the number of slots of the seed table.  KR_ERR_PARAM
 * as kr_guide_hits_table, and for bulges outside 1 .. 2, G below 20 or mismatches above 2 (shorter or looser halves seed
 * nearly every window); KR_ERR_CAPACITY for 2^23 guides or more, or a table that does not fit.  kr_set_params_locate drops
 * the table (its texts are rows of G letters): a scan after it, before a new table, is KR_ERR_PARAM. */
int64_t kr_guide_bulges_table(kr_ctx*, const uint8_t* texts, uint64_t nguides, int mismatches, int bulges, const char* pam5,
                              const char* pam3, int need_pam);
/* one bulged hit, 32 bytes: guide, strand, pam as in kr_guide_hit; mismatches = the least number of aligned columns that
 * differ over the cuts; bulge = +b for a DNA bulge, -b for an RNA bulge; pos = the window's first base, length = G + bulge
 * its bases; bulge_column = the guide columns that lie 5' of the bulge on the guide's strand (of the cuts with the least
 * mismatches the smallest); columns bit c = aligned guide column c differs, 5'->3' on the protospacer (a column without a
 * partner is never set).  One row per (guide, strand, bulge, pos). */
typedef struct { uint32_t guide; uint8_t strand, mismatches, pam; int8_t bulge; uint64_t pos; uint64_t columns;
                 uint32_t bulge_column, length; } kr_guide_bulge_hit;
/* scans uploaded genome `id`: returns the number of bulged hits, kept on the device for the fetch, in the order of the seed
 * pairs that own them (position of the seed, seed piece, the table's entry order), a pair's rows by DNA 1, RNA 1, DNA 2,
 * RNA 2.  Counted, scanned, written: the same bytes on every run.  KR_ERR_PARAM before a table; KR_ERR_CAPACITY for 2^32
 * seed pairs or hits or more, or lists that do not fit. */
int64_t kr_guide_bulges_scan(kr_ctx*, int id);
int64_t kr_guide_bulges_fetch(kr_ctx*, kr_guide_bulge_hit* out, size_t cap);
/* the hits' windows as the guide's strand reads them: row i = G + bulges bytes, the `length` letters of hit i (upper case,
 * the reverse complement for strand 1), then 0.  Returns the number of rows; rows == NULL: size query */
int64_t kr_guide_bulges_windows(kr_ctx*, uint8_t* rows, size_t cap_bytes);

/* ---- guide hits inside the designed primers' products (krisp_fasta --out_assay_hits) -----------------------------------
 * No seam in the reference.  An amplification-plus-Cas assay gives a signal where a region's primers amplify a product
 * AND that region's guide binds between the two primer sites.  DESIGN §21 holds the definition; tests/assay_reference.py
 * restates it.  A product P is a product of kr_primers_scan, a hit H a hit of kr_guide_hits_scan (after need_pam's
 * selection), both of one genome in one locate context (kr_set_params_locate with L+D+R = the protospacer length G; the
 * primer pass reads only the soft-mask mode).  P's interior is [P.pos + len(first), P.pos + P.length - len(second)), with
 * first = the left text on strand 0 and the right text on strand 1: the bases between the two primer sites.  An assay hit
 * is a (P, H) with interior.lo <= H.pos, H.pos + G <= interior.hi and (P.pair, H.guide) a link.  On the device it is
 * csrc/k_assay.inc: a thread per product, a binary search into the position-ordered hit list, a walk over the hits of the
 * interior, a binary search into the links; counted, scanned, written: no atomics, the same bytes on every run.
 *
 * kr_assay_table: n rows of two u32 (row of the primer table's `pairs`, row of the guide-hit table), strictly ascending
 * as 64-bit keys (pair << 32 | guide).  KR_ERR_STATE without both tables; KR_ERR_PARAM for an index out of range, rows
 * that are not ascending and unique, null links with n != 0.  kr_primers_table, kr_guide_hits_table and
 * kr_set_params_locate drop it.  Returns n. */
int64_t kr_assay_table(kr_ctx*, const uint32_t* links, uint64_t n);
/* one assay hit, 48 bytes: the product's pos, length, pair, strand and four mismatch figures as kr_product_hit holds
 * them, then the hit's hit_strand, hit_mismatches, hit_pam, hit_pos, columns, guide as kr_guide_hit holds them; hit = the
 * hit's index in the list of kr_guide_hits_fetch / row of kr_guide_hits_windows */
typedef struct { uint64_t pos; uint32_t length, pair; uint8_t strand, left_mm, right_mm, left_end_mm, right_end_mm, hit_strand,
                 hit_mismatches, hit_pam; uint64_t hit_pos; uint64_t columns; uint32_t guide, hit; } kr_assay_hit;
/* joins the products of the latest kr_primers_scan with the hits of the latest kr_guide_hits_scan.  KR_ERR_STATE without
 * a link table, unless both scans were of genome `id`, or when either table changed since its scan.  Returns the number
 * of assay hits, kept on the device; no products, no hits or no links: 0 without a launch.  Neither list is written: the
 * fetches, sites and windows of both passes give the same bytes after it as before it.  A thread walks the hits of its
 * product's interior alone: the cost is products x hits in range (limits).  KR_ERR_CAPACITY for 2^32 assay
 * hits or more, or a list that does not fit. */
int64_t kr_assay_join(kr_ctx*, int id);
/* the assay hits of the latest join in (pos, length, strand, pair, hit_pos, hit_strand, guide) order: the device lists
 * them by product as it lists the products, a product's by hit as it lists the hits; the rows of one product position
 * are ordered here.  Returns their number; out == NULL: the number only.  KR_ERR_STATE before a join */
int64_t kr_assay_fetch(kr_ctx*, kr_assay_hit* out, size_t cap);

/* ---- multiplex in-silico PCR of a panel's oligos (krisp_fasta --out_panel_products) -----------------------------------
 * No seam in the reference.  With all the primers of a panel in one tube every oligo can open a product and every oligo
 * can close one: DESIGN §24 holds the definition, tests/multiplex_reference.py restates it.  There are T distinct texts
 * of 10 .. 60 letters, written 5'->3'.  Entry 2 t is text t as written: it OPENS a product, its 3' end lies in its last
 * columns.  Entry 2 t + 1 is its reverse complement: it CLOSES a product, its 3' end lies in its first columns (the primer
 * pass's numbering with nleft = T, nright = 0).  A site is the primer pass's site.  A product (a, b) is an opening site of
 * entry 2 a at s1 and a closing site of entry 2 b + 1 at s2 on one record with s2 >= s1 + len(a) and
 * s2 + len(b) - s1 <= max_product; a == b is the product of one primer with itself.  There is no strand: a designed pair
 * (L, R) amplifies (L, R) on '+' and (R, L) on '-'.  It runs in the locate context (only the soft-mask mode plays a part)
 * with a state of its own: a kr_primers_* table, its lists and the assay links beside it are not touched.  On the device
 * the sites are csrc/k_primers.inc's scan, the join and the tally csrc/k_multiplex.inc.
 *
 * kr_multiplex_table: the texts as kr_primers_table takes them, ntexts + 1 ascending offsets.  KR_ERR_PARAM for ntexts
 * outside 1 .. 128, a length outside 10 .. 60, mismatches outside 0 .. 3, max_product < 2 * the longest text (with that
 * bound every ordered pair can form a product), a null table.  Returns the number of slots of the seed table;
 * KR_ERR_CAPACITY for a table that does not fit.  kr_set_params_locate drops the table. */
int64_t kr_multiplex_table(kr_ctx*, const uint8_t* text, const uint32_t* offsets, uint64_t ntexts, int mismatches,
                           uint32_t max_product);
/* one product, 24 bytes: pos = the first base of the opening site, length = to the last base of the closing site, fwd =
 * the text that opens, rev = the text that closes, their sites' mismatches and those in the 5 columns at the 3' ends; the
 * pad is zero */
typedef struct { uint64_t pos; uint32_t length; uint16_t fwd, rev; uint8_t fwd_mm, rev_mm, fwd_end_mm, rev_end_mm, pad[4]; } kr_multiplex_hit;
/* scans uploaded genome `id` as kr_primers_scan does: its separators, its sites, their records, then the join of every
 * opening site with every closing site in reach.  Returns the number of products.  Counted, scanned, written: no atomics,
 * the same bytes on every run.  KR_ERR_STATE "kr_multiplex_table first" without a table; KR_ERR_CAPACITY for 2^32 sites
 * or products or more, or lists that do not fit. */
int64_t kr_multiplex_scan(kr_ctx*, int id);
/* the products of the latest scan in (pos, length, fwd, rev) order.  KR_ERR_STATE before a scan */
int64_t kr_multiplex_fetch(kr_ctx*, kr_multiplex_hit* out, size_t cap);
/* the sites of the latest scan, as the device lists them.  Returns their number; out == NULL: the number only */
int64_t kr_multiplex_sites(kr_ctx*, kr_product_site* out, size_t cap);
/* the products of the latest scan counted on the device, for a caller that wants the counts and not the rows:
 * out[2 * (a * T + b) + clean] = the number of products (a, b), clean = 1 where both end-mismatch figures are 0; 2 T^2
 * counters.  Returns 2 T^2.  The list is only read: a fetch gives the same bytes after it as before it.  No products:
 * zeros without a launch.  KR_ERR_STATE before a scan or after a new table; KR_ERR_CAPACITY for cap < 2 T^2. */
int64_t kr_multiplex_tally(kr_ctx*, uint32_t* out, size_t cap);

/* ---- a panel without cross and single products in any input genome (krisp_fasta --panel-clean) ------------------------
 * No seam in the reference.  kr_panel_run decides by a shared window and four duplex figures and never looks at a genome;
 * here the primer sites of ALL candidates in every input genome are kept on the device, and the selection also drops a
 * candidate one of whose primers forms a product with itself (fate 5, by 0: before the first round, never alive) or with a
 * primer of a member, in either order (fate 4, by = the member; tested behind same locus and clash).  DESIGN §26 holds the
 * definition, tests/panel_clean_reference.py restates it; the kernels are csrc/k_panel_clean.inc.  The state lives in a
 * locate context beside the other passes' (kr_set_params_locate drops it) and touches none of theirs.
 *
 * kr_panel_sites_table: kr_multiplex_table for 1 <= ntexts < 2^24 texts, with its errors for the lengths (10 .. 60), the
 * mismatches (0 .. 3) and max_product (>= twice the longest text).  Empties the store.  Returns the table's slots.
 * kr_panel_sites_scan: the sites of uploaded genome `id` (kr_multiplex_scan's, no join) appended to the store, each with
 * its unit: the genome's record index plus the records of the scans before it (a scan counts separators + 1), so no two
 * records share a unit.  Returns the genome's site count.  KR_ERR_STATE "kr_panel_sites_table first"; KR_ERR_CAPACITY,
 * naming the count, when the store (16 + 4 bytes a site) does not fit or would reach 2^32 sites; the earlier content
 * survives growth.
 * kr_panel_sites_fetch: the whole store as the device holds it (a genome's sites in position order, genomes in scan
 * order) and the units beside it; out == NULL: the count only. */
int64_t kr_panel_sites_table(kr_ctx*, const uint8_t* text, const uint32_t* offsets, uint64_t ntexts, int mismatches,
                             uint32_t max_product);
int64_t kr_panel_sites_scan(kr_ctx*, int id);
int64_t kr_panel_sites_fetch(kr_ctx*, kr_product_site* out, uint32_t* unit, size_t cap);
/* kr_panel_run with the store: its arguments and checks, and texts = two table rows a candidate (left primer, right primer
 * as 5'->3' texts; KR_ERR_PARAM for a row >= ntexts).  KR_ERR_STATE "kr_panel_sites_table first" without a table; with an
 * empty store the members and fates are kr_panel_run's byte for byte.  Three launches a round on the context's stream, one
 * synchronise behind them all; the same bytes on every run.  kr_panel_fetch and kr_panel_fates serve either run.
 * Returns the members. */
int64_t kr_panel_run_clean(kr_ctx*, const uint8_t* templates, const uint16_t* pairs, const uint32_t* texts, uint64_t ncand,
                           int W, int size);
/* out[0] = the self-priming candidates of the latest run, out[1 + j] = the candidates member j + 1 dropped as cross;
 * 1 + members counters, counted from the fates.  Returns their number. */
int64_t kr_panel_clean_drops(kr_ctx*, uint32_t* out, size_t cap);

/* Host-side ingest (no GPU involved): the text of a FASTA / sequence-per-line file -> the
 * upload buffer of kr_genome_upload, with the reference reader's semantics
 * (kstream/kstream.py:458-479 file lines, 510-537 FASTA iff the first line holds '>', 450 that line is
 * consumed when one_shot, 556-583 strip + concatenate between headers, 481-508 + 599 RNA detection and
 * U->T mapping).  universal_newlines != 0 splits on \n, \r, \r\n (plain files), else on \n
 * (gz / bz2 streams).  out needs n + 1 bytes.  stats[4] = records, characters outside
 * ACGTNacgtn (the host resolves those), is_rna (-1 undecided, 0, 1), is_fasta.  Returns the
 * number of bytes written. */
int64_t kr_fasta_to_bases(const uint8_t* text, size_t n, int universal_newlines, int one_shot, uint8_t* out,
                          size_t cap, int64_t* stats);

/* Host-side ingest of one FILE: read -> inflate (.gz: libdeflate when the box
 * has it, else zlib; every member of a multi-member file, BGZF members side by side on host threads,
 * one large member cut into chunks that decode side by side -- csrc/h_pgzip.inc; .bz2: libbz2,
 * block by block on host threads) -> kr_fasta_to_bases, with the reference
 * reader's semantics for files (kstream.py:458-479: .gz by extension; 510-583).  *bases = a buffer
 * the library owns -- pinned host memory when a GPU is present, so that kr_genome_upload copies
 * from it by DMA -- until kr_host_free.  stats[8] = records, characters outside ACGTNacgtn, is_rna,
 * is_fasta, read us, inflate us, parse us, gzip members | used_libdeflate << 32.  Returns the
 * number of bytes; a .bz2 file on a box without libbz2 returns KR_ERR_HOST (the host layer inflates it). */
int64_t kr_ingest_file(const char* path, uint8_t** bases, int64_t* stats);
/* The same ingest with the PARSE on the device (the host reads and inflates only):
 *   kr_read_file            the file's text in pinned host memory (free with kr_host_free); stats[8]: [3] = 1 when the
 *                           text wants universal newlines (a plain file), [4] read us, [5] inflate us, [6] copy us,
 *                           [7] gzip members | used_libdeflate << 32.  Returns the number of bytes (.bz2 without libbz2: KR_ERR_HOST).
 *   kr_genome_upload_text   text -> genome `id`'s upload buffer, parsed on the device (csrc/k_text.inc) with exactly
 *                           kr_fasta_to_bases' result (the tests compare them byte for byte), then as
 *                           kr_genome_upload.  stats[4] = records, characters outside ACGTNacgtn, is_rna, is_fasta.
 *                           Returns the number of bases (separators included).
 *   kr_genome_fetch_bases   an uploaded genome's bases back to the host (the IUPAC side channel, text cutting) */
int64_t kr_read_file(const char* path, uint8_t** text, int64_t* stats);
/* Round 6 -- a BGZF file (bgzip: a chain of gzip members of <= 64 KB of text that say
 * how long they are) inflated ON THE DEVICE, a lane per member (csrc/k_inflate.inc), then parsed there as
 * kr_genome_upload_text parses a text (.gz streams: no universal newlines): `file` = the bytes of the file as they lie on
 * disk.  Every member's CRC-32 and ISIZE are checked on the device.  Returns the number of bases; KR_ERR_HOST -- nothing
 * uploaded -- when the file is not BGZF all the way (plain gzip, other extra fields, >= 2^32 bytes) or a member does not
 * inflate to its trailer: the caller then reads the file as any other `.gz` (kr_read_file), and that path's verdict on it
 * stands (the reference: kstream.py:458-479, gzip.open).  stats[8]: [0..3] as kr_genome_upload_text, [4] members,
 * [5] first bad member, [6] its status, [7] microseconds of the inflate + CRC kernels. */
int64_t kr_genome_upload_bgzf(kr_ctx*, int id, const uint8_t* file, size_t n, int one_shot, int64_t* stats);
/* A `.gz` file of ONE plain gzip member (what `gzip` writes; csrc/k_gunzip.inc) inflated ON THE DEVICE, then parsed there as
 * kr_genome_upload_bgzf parses its text: `file` = the bytes as they lie on disk (header with any of FEXTRA / FNAME /
 * FCOMMENT / FHCRC, deflate data, trailer, zero padding behind it).  The deflate data is cut into chunks of `chunk`
 * compressed bytes (0: the library's choice); every chunk after the first finds a block start by trial, the chunks decode
 * side by side into 16-bit symbols (a byte, or a place in the unknown 32 KB in front of the chunk), the windows are handed
 * down the line, CRC-32 and ISIZE checked against the trailer.  Returns the number of bases; KR_ERR_HOST -- nothing
 * uploaded -- for a BGZF file, a second member or other data behind the trailer, a file or text of >= 2^32 - 64 bytes, a
 * CRC or ISIZE that differs, anything that does not decode, or scratch (about 2 bytes per byte of text + the file) that
 * does not fit: the caller then reads the file through kr_read_file, whose verdict stands.  The scratch is given back
 * before the call returns.  stats[8]: [0..3] as kr_genome_upload_text, [4] chunks, [5] chunks joined (their block start
 * was real), [6] the longest run of windows resolved one after the other, [7] microseconds of the inflate's wall time (the
 * kernels, the host's walk along the chunks between them, the small copies of their results).  Tuning: KRISP_GZ_CHUNK =
 * the chunk size when `chunk` is 0 (default 256 KB), KRISP_GZ_LANES = active lanes per wave of the decode (1 .. 64,
 * default 64); KRISP_PGZIP_DEBUG=1 prints the chunks, starts found, line and window runs of every call. */
int64_t kr_genome_upload_gzip(kr_ctx*, int id, const uint8_t* file, size_t n, size_t chunk, int one_shot, int64_t* stats);
/* The large device buffers of `n` genomes (ids[]) of up to n_bases bases each -- upload buffer, sorted-key arrays, sort
 * lanes; with_text: the device reader's copy of the file text as well -- made ahead of the uploads, while host threads
 * still read and inflate the files (krisp_fasta.py:86-123 starts a process per genome; here the one context gets its
 * memory while the files inflate: memory another process has just given back costs 15-40 ms per GB to obtain, seconds at 3 Gbp).  After kr_set_params;
 * purely an optimisation: the uploads and sorts make or grow whatever is missing. */
int kr_reserve(kr_ctx*, const int* ids, int n, size_t n_bases, int with_text);
/* out4[0] = bytes this context may still allocate (the device's free memory, or the rest of its HBM budget when that is
 * less), [1] = the device's total, [2] = bytes the context holds, [3] = its budget (0 = none).  The command line sizes its
 * genome batches with it when a genome set does not fit one GPU (krisp_amd/krisp_fasta.py: the streaming flow -- the
 * reference has no such limit: kstream.py:108-119 sorts in external memory, intersectAmplicons.py:232-310 merges files) */
int kr_mem_info(kr_ctx*, int64_t* out4);
int64_t kr_genome_upload_text(kr_ctx*, int id, const uint8_t* text, size_t n, int universal_newlines, int one_shot,
                              int64_t* stats);
int64_t kr_genome_fetch_bases(kr_ctx*, int id, uint8_t* out, size_t cap);
void    kr_host_free(void* p);

/* Host-side (no GPU involved): the side channel of SURVEY 8(b) -- the windows the device's 2-bit
 * alphabet cannot carry.  `bases` is an upload buffer (kr_fasta_to_bases).  Returns the number of
 * window starts (ascending) of windows of k characters that survive the soft-mask rule, hold no
 * N/n and hold an IUPAC ambiguity letter: the reference keeps those k-mers and complements them
 * letter by letter (COMP_MAP kstream.py:11-18, _complements 644-677); the binder cuts them out
 * of its text and joins them with the device results.  KR_ERR_KEY (+ *bad_char) where the
 * reference raises KeyError (kstream.py:658).  starts may be NULL (count only). */
int64_t kr_scan_special(const uint8_t* bases, size_t n, int k, int omit_soft, uint64_t* starts, size_t cap,
                        int* bad_char);

/* Final text from survivor records of packed keys -- replaces Amplicon.py:523-671 (render_alignment, render_csv,
 * makeBracket, consensus) and outputAlignments.py:26-162 at --cores 1 for large results: the CSV and the alignment
 * blocks as bytes, one pass, no object per Amplicon (krisp_amd/amplicon.py keeps the general path; the tests run
 * both and compare byte for byte).  recs ordered by (key, label id); label_of[genome] = rank of the genome's label
 * among the distinct labels in string order; label_in[label] = 1 for ingroup labels, NULL when no outgroup was
 * given.  Host only.  Returns the number of groups, KR_ERR_HOST for a group this code leaves to the general path
 * (no all-ingroup row for the CSV consensus: the reference raises there).  Free the texts with kr_text_free. */
int64_t kr_render_records(const kr_record* recs, size_t n, int L, int D, int R, const uint32_t* label_of,
                          size_t n_genomes, const char* const* label_text, size_t n_labels, const uint8_t* label_in,
                          int dot, char** csv, size_t* csv_len, char** align, size_t* align_len);
/* ... and from member windows of long amplicons (kr_wide_fetch_windows; Amplicon.py:598-671 on text the reference holds as
 * strings anyway): rows = n windows of L+D+R letters in line order, cand[i] = group number of row i (the rows of a group
 * adjacent: KR_WIDE_HITS order), genome[i] = index into label_of.  Groups are ordered by (left, right), members by (diag,
 * label) here.  rna: write T as U.  KR_ERR_HOST also when one (left,right) arrives under two group numbers. */
int64_t kr_render_windows(const uint8_t* rows, size_t n, int L, int D, int R, const uint32_t* cand, const uint32_t* genome,
                          const uint32_t* label_of, size_t n_genomes, const char* const* label_text, size_t n_labels,
                          const uint8_t* label_in, int dot, int rna, char** csv, size_t* csv_len, char** align,
                          size_t* align_len);
void    kr_text_free(void* p);

/* Options that change HOW (never what) the library computes; results are identical for every
 * value (tests run the suite under each).  Set after kr_create, before kr_set_params. */
enum { KR_OPT_SLICE_BASES = 1,       /* -1 automatic; 0..4: sort every genome in 4^n key-space slices (the
                                        large-genome path, pass 0 + per-slice pass 1) */
       KR_OPT_GENERIC_INTERSECT = 2, /* 1: every intersect sub-tile takes the generic path (key-count
                                        splits, ranges from the prefixes) instead of whole-bucket sub-tiles */
       KR_OPT_ISECT_FORMAT = 3,      /* 0 automatic; 1: the narrow per-prefix state also for D <= 4; 2: automatic, but never the
                                        32-bit word per prefix that one diagnostic column and <= 24 genomes otherwise get */
       KR_OPT_ABLATE = 4,            /* timing aids of kr_debug_*; refused unless built with -DKR_ABLATE */
       KR_OPT_WIDE_SLOTS = 5,        /* wide path: 1 (default) dictionaries also as one-sector slot tables, 0 index + sorted keys only */
       KR_OPT_PLACE_TRIES = 7,       /* 1 .. 16 (default 8): candidate allocations of the pass-1 output buffer (>= 256 MB), each timed under
                                        pass 1's write pattern, the fastest kept: physical placement moves pass 1 / pass 2 by up to 15 %
                                        from one allocation to the next; worth its ~5 ms per candidate for contexts that sort many genomes */
       KR_OPT_ISECT_KERNEL = 8,      /* 0 (default) the persistent, pipelined intersect kernels over items of whole buckets wherever a
                                        (left,right) group lies inside one fine bucket (with 32-bit heads where the geometry allows);
                                        1: one workgroup per chunk everywhere; 2: pipelined with 64-bit heads only */
       KR_OPT_LANES = 9,             /* sort lanes, 1 .. 8: consecutive kr_genome_sort calls go to consecutive lanes (own stream, own
                                        scratch: 16 bytes per base each) and overlap on the device (3 lanes: -7 % per step on 4 x 50
                                        Mbp); kr_intersect and every call that reads a sorted genome join them.  0 (default):
                                        automatic -- one lane until the context has sorted 16 genomes (a lane costs ~10 ms to set
                                        up, more than a one-shot run gets back), 3 from then on.  Key-space slices use one lane
                                        whatever the setting, kr_wide_run two when more than one is asked for.  May be set at any time */
       KR_OPT_LAZY_ORDER = 10,       /* 1 (default): kr_genome_sort stops at the fine buckets, the LDS sort runs where a reader needs
                                        the order (see kr_genome_sort); 0: every sort ends with it (rounds 1-5) */
       KR_OPT_COARSE_REST = 11,      /* 1 (default; KR_COARSE_REST in the environment): kr_genome_partition stops behind pass 1; 0: it is the full sort */
       KR_OPT_COARSE_POOL = 12,      /* 1 (default; KR_COARSE_POOL in the environment): a genome that kr_genome_partition takes again and again
                                        writes its pass 1 into a buffer the placement search chose (a pool of them, made behind the
                                        kr_intersect that sees such a genome for the second time; the gates of KR_OPT_PLACE_TRIES); 0: always into its own key array */
       KR_OPT_JOIN2 = 13,            /* 1 (default; KR_JOIN2 in the environment): an intersection of two genomes, one of each side, with one
                                        diagnostic column and the filter on screens its keys in LDS and joins only the live ones
                                        (k_join2); 0: the n-way kernel as for every other call.  KR_JOIN2_GRID in the environment caps its grid (tests) */
       KR_OPT_COARSE_ONE_STRAND = 14, /* 1 (default; KR_COARSE_ONE_STRAND in the environment): where one diagnostic column, `left` filling the
                                        key's high word, L >= 5 and R < L allow it, kr_genome_partition writes the forward record of every
                                        window only and kr_intersect asks each key both ways (the same candidates, records and counts);
                                        0: both strands are partitioned */
       KR_OPT_COARSE_ONE_PASS = 15,  /* 1 (default; KR_COARSE_ONE_PASS in the environment): the probe of one-strand genomes streams a bucket
                                        past the forward AND the reverse candidates of its digit in one pass, each key tested once for
                                        both readings; 0: one reading after the other (the same kernel, the same results) */
       KR_OPT_JOIN2_DENSE = 16,      /* 1 (default; KR_JOIN2_DENSE in the environment): k_join2 keeps each key's screen slot in a register and
                                        queues the live keys per wave, so the exact join runs with full lanes; 0: every key slot joins its
                                        own live keys, the slot computed again (the same kernel source, the same results) */
       KR_OPT_WIDE_ORDERED = 6 };    /* wide path: 0 (default) flanks of >= 20 bases are numbered through minimizer buckets (look-ups
                                        of neighbouring windows share memory sectors): the same groups and hits, but `cand` no longer
                                        ascends with (left, right); 1: order-preserving ranks, groups in the reference's order */
int     kr_set_option(kr_ctx*, int option, int64_t value);

int     kr_sync(kr_ctx*);
/* HIP-event timers on the context's stream */
int     kr_timer_begin(kr_ctx*);
double  kr_timer_end_ms(kr_ctx*);                              /* syncs */
/* accumulated device time of one stage since the last kr_stage_reset (syncs);
 * only collected after kr_stage_enable(ctx, 1) (it serialises launches). */
int     kr_stage_enable(kr_ctx*, int on);
/* time only the stages whose bit (1 << KR_ST_x) is set: the event pairs around every launch
 * cost ~4 % of a C2 step when all stages are timed; bench.py times the dominant kernel only
 * inside its timed region (the full table comes from a calibration pass before it) */
int     kr_stage_select(kr_ctx*, unsigned stage_mask);
int     kr_stage_reset(kr_ctx*);
double  kr_stage_ms(kr_ctx*, int stage);
int64_t kr_stage_launches(kr_ctx*, int stage);

/* introspection for stage-level parity tests: 0 codes(u64) 1 bad(u32) 2 hist(u32)
 * 3 bucket offsets(u32) 4 keys after pass 1 5 keys after pass 2.  Returns the
 * number of ELEMENTS copied (of the element type above). */
int64_t kr_debug_fetch(kr_ctx*, int genome_id, int what, void* out, size_t cap_bytes);
/* property check for sizes no oracle reaches: adjacent key pairs out of order (0 = sorted) */
int64_t kr_debug_inversions(kr_ctx*, int genome_id);
/* timing aid: the LDS sort re-run `reps` times over a sorted genome (mode must be 0).  Average ms per launch. */
double  kr_debug_localsort(kr_ctx*, int genome_id, int reps, int mode);
/* timing aid: the intersect kernel `reps` times (mode 0 as shipped; a -DKR_ABLATE build also
 * takes 64 keys streamed but not probed, 128 probed without the LDS update, ...: k_intersect.inc);
 * leaves the candidate set invalid */
double  kr_debug_intersect(kr_ctx*, const int* genome_ids, int n, const uint8_t* is_ingroup, int reps, int mode);
/* measured streaming-copy rate of this device (read + write GB/s): bench.py reports the roofline
 * fraction against it beside the 8 TB/s specification figure */
double  kr_debug_copy_gbps(kr_ctx*, size_t bytes, int reps);
/* which copy form and grid gave that figure (1 / 2 / 4 loads in flight per lane, plain or non-temporal, 2 .. 32 workgroups
 * per CU are all timed; the best is reported): a string owned by the context, valid until the next probe */
const char* kr_debug_copy_which(kr_ctx*);
/* the pipelined intersect kernels: items that went to the chunk kernel (oversized), slices redone by chunks,
 * threads per workgroup, log2(buckets per item) and 1 = 32-bit heads of the latest launch; out[5] = sort lanes in use
 * now; out[6..7] = intersections that left their late genomes to the probe, candidates the latest of them probed */
/* 0 for a product build; else the result-changing experiment switches the library was compiled with (bit 0 -DKR_EXPERIMENTS,
 * 1 KR_ABLATE, 2 I3_ABL, 3 P2_ABL, 4 LS2_NORANK, 5 KR_EXP_NOLOOKUP, 6 KR_EXP_MZONLY: csrc/k_keys.inc).  No context, no GPU needed. */
int     kr_build_experiments(void);
/* KR_OPT_LAZY_ORDER's counters: out[0] LDS sorts of whole slices kr_genome_sort left out, [1] made later (anchor, fetch, probe),
 * [2] kr_collect calls that read only the buckets their candidates touch, [3] the option's value, [4] intersection launches whose
 * anchor genome stayed in bucket order as well (k_intersect3t<., UA>), [5] 1 unless KR_FUSE_ANCHOR=0,
 * [6] genomes an intersection took in the coarse state (kr_genome_partition), [7] coarse genomes sorted fine after all */
int     kr_debug_lazy(kr_ctx*, int64_t* out8);
/* the intersection's counters: out8[0] items the chunk kernel took, [1] slices redone by chunks, [2] threads and [3] log2 buckets of
 * the latest call's items, [4] 1 where it took the kernels with 32-bit heads, [5] the sort lanes in use, [6] launches that took
 * k_join2 (KR_OPT_JOIN2), [7] items it handed to the redo path because their live keys found no room in its table */
int     kr_debug_isect(kr_ctx*, int64_t* out8);
/* the latest tile scan's geometry (locate, near-match, product, primer and guide-hit passes): out8[0] tiles, [1] workgroups launched
 * and [2] the cap in force (KR_SCAN_GRID in the environment when the context is made, 1 .. 65 536: the scans' persistent grids and
 * their element-stride launches take at most that many workgroups; 0 = none) of the latest scan, [3] the tiles or blocks of the
 * latest two-pass list (a join's or an extend step's blocks), [4..7] 0 */
int     kr_debug_scan(kr_ctx*, int64_t* out8);
/* the latest placement search of the pass-1 output buffers: out8[0] candidates probed, [1] buffers handed to the sort lanes,
 * [2..5] probe milliseconds of the four fastest candidates, [6] the median, [7] the slowest (bench.py prints them: which
 * placement class a line ran in) */
int     kr_debug_place(kr_ctx*, double* out8);
/* the pool of placed pass-1 targets of coarse genomes (KR_OPT_COARSE_POOL): out8[0] buffers in all, [1] free, [2] held by genomes,
 * [3] partitions that wrote into a pooled buffer, [4] searches run, [5] / [6] the fastest / slowest probe milliseconds among the
 * buffers held, [7] the option's value */
int     kr_debug_coarse_pool(kr_ctx*, double* out8);
/* KR_OPT_COARSE_ONE_STRAND's counters: out8[0] partitions that wrote one strand, [1] intersections that probed one-strand genomes,
 * [2] / [3] the forward / reverse rounds of all of them, [4] / [5] of the latest, [6] the option's value, [7] the passes of the
 * latest call (KR_OPT_COARSE_ONE_PASS: a pass holds a forward and a reverse round) */
int     kr_debug_coarse_strand(kr_ctx*, int64_t* out8);
/* what the multi-GPU exchange has cost this context so far: out[0] host synchronisations, [1] point-to-point calls,
 * [2] collectives, [3] microseconds inside kr_cands_reduce / kr_cands_bcast, [4] kr_cands_reduce calls, [5] entries of the
 * agreed message size */
int     kr_debug_comm(kr_ctx*, int64_t* out8);
/* microseconds per blocking call of the exchange on this box (host clock, RCCL communicator of any world size, every rank
 * calls it): out3[0] all-reduce of three doubles + synchronisation, [1] a send / receive pair of `bytes` to the rank itself
 * + synchronisation, [2] a broadcast of `bytes` + synchronisation */
int     kr_debug_comm_probe(kr_ctx*, size_t bytes, int reps, double* out3);
/* one round of the tree with the rank itself as its partner over RCCL: the candidate list + header sent to and received from
 * itself, merged as a received list is (count read on the device).  What a one-GPU box can show of the exchange on the real
 * transport; returns the count (unchanged for an unfiltered list) */
int64_t kr_debug_cands_selfexchange(kr_ctx*, int apply_filter);
/* test aid for the communicator's watchdog: a receive nobody sends to + the synchronisation behind it; returns when the
 * watchdog has aborted the communicator (KR_ERR_STATE) or RCCL has refused the call (KR_ERR_HIP); the communicator is spent */
int     kr_debug_comm_hang(kr_ctx*);
/* test aids: bytes left of the context's HBM budget (-1 = no budget); make `left` bytes remain from now on */
int64_t kr_debug_budget_left(kr_ctx*);
int     kr_debug_budget_set(kr_ctx*, int64_t left);
int     kr_debug_info(kr_ctx*, int64_t* out8);  /* b, nbuckets, T, CAP, nwg, overflow segments, fallback launches, 0 */

#ifdef __cplusplus
}
#endif
#endif

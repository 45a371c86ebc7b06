// h_core.inc -- part of krisp_hip.hip (one translation unit): host: context, buffers, stage timers, parameters, upload, sort, finalize, sorted-file adoption
static thread_local std::string g_last_error;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// one key-space slice of a genome (the whole genome when the context has a single slice)
struct Slice {
    DevBuf keys, off, chunkstart, chunkdesc, ovf;   // ovf: u32 count @0, uint2 segments @16
    u64 nmax = 0;            // exact key count of the slice (known after upload)
    u32 nchunks = 0;
    int64_t count = -1;      // key count confirmed by the sort
    int res = -1;            // this slice's pair of words {oversized buckets, key count} in the host mailbox
};

struct Genome {
    int id = -1;
    size_t n_bases = 0;
    u64 nwords = 0;          // ceil(n/32)
    u64 nmax = 0;            // sum of the slice counts
    DevBuf bases, wkeys;     // wkeys: wide path, this genome's composite keys (then its windows' groups)
    DevBuf wlcnt;            // wide path, key LIST form (Geom.wlcnt): entries per workgroup segment of wkeys
    bool wlist = false;      // wkeys holds the list form (last wide run)
    u32 wlcap = 0;           // ... of so many entries per segment
    std::vector<Slice> sl;
    bool uploaded = false, sorted = false, finalized = false;
    bool ordered = false;    // the keys are in order INSIDE their fine buckets too (k_localsort2 has run): what kr_genome_sort leaves
                             // undone under KR_OPT_LAZY_ORDER until somebody needs it (order_genome)
    bool coarse = false;     // kr_genome_partition: the sort stopped behind pass 1 -- sl[0].keys holds the keys in 256 buckets by their top byte,
                             // sl[0].off[0 .. 256] the buckets' bases, sl[0].off[2^b] the key count; `sorted` is false: whoever needs the fine
                             // buckets calls ensure_fine() first.  kr_intersect takes such a genome by k_coarse_probe (h_intersect.inc)
    bool one_strand = false; // ... the forward record of every window only, in buckets by cs_digit (co_strand.inc): a key stands for two
                             // records (sl[0].off[2^b] counts both), the probe asks it both ways
    DevBuf ckeys;            // ... out of this array when the genome holds one: a pass-1 target of the context's pool of PLACED
                             // buffers (coarse_pool_*); without one pass 1 writes sl[0].keys, which no placement search chose
    double ckeys_ms = 0;     // ... its probe time
    hipStream_t ckeys_busy = nullptr;  // ... the stream of the last kernel that touched it, until the host has waited for that stream
    hipEvent_t ckeys_ev = nullptr;     // ... recorded behind that kernel when the buffer changes hands (coarse_pool_handover)
    bool ckeys_wait = false;           // ... and not waited for yet: whoever writes the buffer next waits for it first
    int64_t partitions = 0;  // coarse sorts of this genome in this context (the pool grows for genomes that come back)
    DevBuf hits;             // ... and leaves its keys under the candidates' prefixes here (u32 count, keys from byte 16) for kr_collect
    u32 hitcap = 0;
    bool hits_valid = false; // `hits` belongs to the context's current candidate list (or to a list the current one is a part of)
    bool was_anchor = false; // the latest kr_intersect over this genome took it as its anchor: its next sort ends with the LDS sort
                             // on its own lane, beside the other genomes' passes, instead of in front of the intersection
    int64_t count = -1;
    hipEvent_t up_done = nullptr;      // the H2D copy of `bases` (copy stream); sorts wait for it
};

// one sort "lane" = a stream + the scratch one genome sort needs; consecutive genome sorts
// go to different lanes so that their (latency / barrier bound) kernels overlap on the GPU
struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false;
    DevBuf codes, bad, partial8, base1, tmpkeys, tp, tiledesc, tilehist, wkeys;
    DevBuf partial16, cursor, h16exc;   // fine histogram from the codes (k_hist16), pass-2 reservation cursors, counts beyond 16 bits
    DevBuf pass0, base64;    // sliced genomes: all keys partitioned by their top byte, the 64-bit bucket bases
    DevBuf slt, offa, cura;  // ... and their pass 1 by k_scatter2: small tables, offsets / cursors of the (slice, top byte) bins
    // the lane's device buffers, named here alone (kr_destroy, and take_lane's retreat to one lane, release them)
    void bufs(std::vector<DevBuf*>& v) {
        v.insert(v.end(), {&codes, &bad, &partial8, &base1, &tmpkeys, &tp, &tiledesc, &tilehist, &wkeys, &pass0, &base64,
                           &partial16, &cursor, &h16exc, &slt, &offa, &cura});
    }
};
#define MAX_LANES 8

struct kr_comm;

struct kr_ctx {
    int device = 0;
    kr_comm* comm = nullptr;          // multi-GPU exchange (h_comm.inc)
    hipStream_t stream = nullptr;     // main stream = lanes[0].stream
    hipStream_t copy_stream = nullptr;   // H2D of genomes from pinned buffers (kr_ingest_file), beside the sorts
    Lane lanes[MAX_LANES];
    int nlanes = 0, next_lane = 0;    // sort lanes (KR_OPT_LANES / KR_LANES env; 0 = automatic): lanes_used() of them take the sorts in turn
    int lanes_ready = 0;              // lanes whose scratch fits lane_maxcount
    int64_t sorts_done = 0;
    int place_n = 0, place_taken = 0;  // the latest placement search (ensure_placed): candidates probed, buffers handed out,
    double place_ms[6] = {0, 0, 0, 0, 0, 0};    // probe times: the four fastest, the median, the slowest; of buffers of place_bytes
    size_t place_bytes = 0;
    u64 ex_cap = 0;                   // multi-GPU exchange (h_comm.inc): entries of the message size the ranks agreed on last (exchange_prepare)
    char copy_which[160] = {0};       // the form of k_copy16 that kr_debug_copy_gbps found fastest (kr_debug_copy_which)
    u64 lane_maxcount = 0;            // keys the lanes' scratch is sized for
    int last_lane = 0;                // the lane of the latest sort (kr_debug_fetch looks into its scratch)
    int sb = 0, nslices = 1;          // key-space slices: 4^sb
    size_t budget = 0, used = 0;
    bool have_params = false;
    Geom g{};
    size_t max_bases = 0;
    std::map<int, Genome> genomes;
    int ls_grid = 768;     // resident k_localsort2 workgroups (set from the occupancy query)
    int place_tries = 8;   // KR_OPT_PLACE_TRIES / KR_PLACE_TRIES env: candidate allocations of the pass-1 output buffer (buffers >= 256 MB)
    bool place_tries_set = false;   // asked for by the caller (option / environment): else contexts with an HBM budget, or that share
    bool shared_gpu = false;        // their GPU with other ranks (file transport), take the buffer as allocated
    // candidates / records
    DevBuf candP;      // kr_intersect over more than 32 genomes: the running list while the next batch is intersected
    DevBuf candA, candB, chunkcnt, chunkpos, flags, blockcnt, blockpos, other, records, nrec, fbdesc, fbsegs;
    DevBuf coltab, collo, colcnt, colpos, coltsum, coltpos, colfirst, colfm;     // kr_collect: pointer tables, run starts, counts, places, first keys + their multiplicities
    int64_t ncand = -1;
    int64_t nrecords = 0;
    std::string err;
    // timers
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool stage_on = false;
    unsigned stage_mask = ~0u;      // stages whose launches are bracketed by events while stage_on
    struct Pair { hipEvent_t a, b; int stage; };
    std::vector<Pair> pending;
    std::vector<hipEvent_t> pool;
    double stage_ms[KR_ST_COUNT] = {0};
    int64_t stage_n[KR_ST_COUNT] = {0};
    int64_t fallback_launches = 0, overflow_segments = 0;
    int dbg = 0;   // 32 = generic intersect sub-tile path (KR_OPT_GENERIC_INTERSECT, or KR_DBG=32 in the environment);
                   // other bits: timing aids of a -DKR_ABLATE build, set by kr_debug_* / KR_OPT_ABLATE only
    int isect_kernel = 0;   // KR_OPT_ISECT_KERNEL / KR_ISECT_KERNEL env: 0 = the pipelined kernels where they apply (32-bit heads, k_intersect3t, where the geometry allows), 1 = one workgroup per chunk (k_intersect) everywhere, 2 = pipelined with 64-bit heads only (k_intersect3)
    int ncu = 256;
    // host mailbox: pinned, device-visible words that kernels (k_publish) write and the host reads after ONE stream
    // synchronisation -- [0, MB_SLICE0): scalars of kr_intersect / kr_collect, then two words per slice
    DevBuf bgz_in, bgz_tab, bgz_stat;        // kr_genome_upload_bgzf: the compressed file, its member table (+ CRCs), the members' status
    DevBuf tx_scan;                          // kr_genome_upload_text: the line scan's per-thread / per-workgroup partials
    DevBuf tx_text, tx_tile, tx_tilepos, tx_lines, tx_ls, tx_ll, tx_op, tx_outpos, tx_state, tx_tsum, tx_tpos;   // kr_genome_upload_text: the device reader's scratch
    u32* mbox = nullptr;
    std::vector<uint64_t> coltab_host;     // kr_collect: the pointer table as last uploaded
    std::vector<int> mb_free;
    int mb_next = 0;
    int i3_occ[3][4][9] = {{{0}}};      // ([2]: k_intersect3t<FMT, UA = true>)      // resident k_intersect3<FMT> ([1]: k_intersect3t<FMT>) workgroups per CU by threads / 64 (occupancy query, cached)
    DevBuf isovf;                   // k_intersect3: oversized items
    int join2 = 1;                  // KR_OPT_JOIN2 / KR_JOIN2 env (A/B, tests): 1 = two genomes, one of each side, one diagnostic column, filter on take k_join2; 0 = k_intersect3t as every other call
    u32 j2_grid = 0;                // KR_JOIN2_GRID env (tests: a few workgroups walk many items; 0 = the occupancy x the CUs)
    int join2_dense = 1;            // KR_OPT_JOIN2_DENSE / KR_JOIN2_DENSE env (A/B, tests): 1 = k_join2<true>: slots kept, live keys queued per wave and joined with full lanes; 0 = k_join2<false>
    int j2_occ[2][9] = {{0}};       // resident k_join2<dense> workgroups per CU by threads / 64 (occupancy query, cached)
    int64_t j2_launches = 0, j2_full = 0;    // launches that took k_join2; items it handed on because their live keys found no room
    bool j2_full_counted = false;   // (the redo of a call counts its handed-on items once)
    int64_t isect_ovf_items = 0, isect_refall = 0;
    int i3_last_T = 0, i3_last_mlog = 0, i3_last_tags = 0, i3_last_ua = 0;
    int64_t isect_ua = 0;            // intersections whose anchor stayed in bucket order (k_intersect3t<., true>)
    int fuse_anchor = 1;             // KR_FUSE_ANCHOR env (A/B, tests): 0 = the anchor genome is sorted by k_localsort2 before every intersection
    u32 i3_ovf_cap = I3_OVF_CAP;    // KR_ISECT_OVF_CAP env (tests: the redo-by-chunks path at small sizes)   // items that took the chunk kernel; slices redone by chunks
    int isect_fmt = 0;   // KR_OPT_ISECT_FORMAT / KR_ISECT_FMT env (A/B switch): 1 = narrow mask format also for D <= 4
    int opt_slice_bases = -1;   // KR_OPT_SLICE_BASES / KR_SLICE_BASES env: -1 = automatic
    hipEvent_t slice_ready[2] = {nullptr, nullptr};   // a sliced genome's pass 0 is done (per genome lane): its slices may start on the helper lane
    bool custom_layout = false; // kr_set_field_order moved fields: a sort-only context (no (left,right) prefix to intersect on)
    bool mixed_alphabets = false;   // kr_set_mixed_alphabets: the diagnostic filter in its mode 2 (k_intersect.inc: passes_filter)
    int lazy_order = 1;         // KR_OPT_LAZY_ORDER / KR_LAZY_ORDER env: 1 = a sort stops at the fine buckets (two partition passes); the order
                                // inside the buckets is made when somebody reads it: the anchor of an intersection, the buckets a candidate
                                // list touches (kr_collect), a whole genome for kr_genome_fetch_keys / the probes.  0 = every sort ends with k_localsort2
    bool order_wanted = false;  // the latest kr_collect had to sort its genomes whole (a candidate list too long to read bucket by bucket:
                                // configs[4]'s 6.5e7): until a collect gets by without, the sorts of this context end with the LDS sort
                                // again -- on their lanes, beside each other -- instead of in front of the collect
    int64_t lazy_skipped = 0, lazy_ordered = 0, lazy_touch = 0;    // LDS sorts of whole slices left out / made later; bucket lists sorted for kr_collect
    DevBuf touchdesc, touchovf;   // kr_collect over genomes in bucket order: chunk descriptors of the touched buckets, their oversized list
    int coarse_rest = 1;        // KR_OPT_COARSE_REST / KR_COARSE_REST env: 1 = kr_genome_partition stops behind pass 1 where the context is
                                // eligible; 0 = it is kr_genome_sort
    int64_t coarse_done = 0, coarse_promoted = 0;   // genomes kr_intersect took in the coarse state; coarse genomes sorted fine after all
    int coarse_one = 1;         // KR_OPT_COARSE_ONE_STRAND / KR_COARSE_ONE_STRAND env: 1 = a coarse partition writes one strand where one_strand_form() holds
    int64_t one_partitions = 0, one_calls = 0, one_rounds[2] = {0, 0}, one_last[2] = {0, 0};   // ... its counters (kr_debug_coarse_strand)
    int coarse_pass = 1;        // KR_OPT_COARSE_ONE_PASS / KR_COARSE_ONE_PASS env: 1 = a pass of the one-strand probe holds a forward AND a
                                // reverse round of its digit (co_pass.inc); 0 = one round after the other
    int64_t one_last_passes = 0;    // ... the passes of the latest call
    DevBuf co_ent;              // ... the candidates' entries by class, behind them the class counts, bounds and cursors (k_strand_*)
    int coarse_pool = 1;        // KR_OPT_COARSE_POOL / KR_COARSE_POOL env: 1 = coarse genomes that are partitioned again and again write
                                // their pass 1 into placed buffers (coarse_pool_grow); 0 = always into their own key arrays
    struct PoolBuf { DevBuf buf; double ms; hipEvent_t ev; bool wait; };
    std::vector<PoolBuf> cpool_free;    // placed pass-1 targets nobody holds, the fastest first
    int cpool_total = 0;                // ... and in all: free + held by genomes (Genome.ckeys)
    int64_t cpool_partitions = 0;       // coarse sorts that wrote into a pooled buffer
    int64_t cpool_searches = 0;         // placement searches the pool has run
    size_t place_min_bytes = (size_t)256 << 20;     // KR_PLACE_MIN_BYTES env (tests): buffers below this size are taken as allocated
    DevBuf co_state, co_tab;    // k_coarse_probe: the candidates' state words; cb[257], ust[257] and the 256 rows of a call
    u32 co_tcap = CO_TCAP;      // KR_COARSE_TCAP env (tests: several rounds per top byte at small sizes)
    u32 co_hitcap = 0;          // KR_COARSE_HITCAP env (tests: a hit list that overflows; 0 = sized from the candidate list)
    int co_occ = 0;             // resident k_coarse_probe workgroups per CU (occupancy query, cached)
    u32 co_grid = 0;            // KR_COARSE_GRID env (tests: a few workgroups walk many work units; 0 = co_occ x the CUs)
    u32 scan_cap = 0;           // KR_SCAN_GRID env (tests: a few workgroups walk many tiles of a scan; 0 = scan_grid()'s occupancy x the CUs)
    int64_t scan_dbg[3] = {0, 0, 0};      // kr_debug_scan: tiles and grid of the latest scan_grid(), blocks of the latest scan_two_pass
    int slice_route = 1;        // KR_SLICE_ROUTE env (A/B, tests): 0 = every slice counts its keys again before its pass 1 (k_hist8k / k_scatter1kp)
    typedef std::vector<DevBuf*> Bufs;      // bufs(): a state's device buffers, named there alone (kr_destroy releases them)
    // wide windows (kr_set_params_wide / kr_wide_run)
    struct Wide {
        bool on = false;
        int L = 0, D = 0, R = 0, k = 0, omit = 0, W = 0, strands = 0;
        // per flank (0 `left`, 1 `right`) up to three dictionaries: [0] the flank (<= 32 bases) or its
        // first 32 bases, [1] the rest of a longer flank, [2] the combinations rank:rank of a longer flank
        struct DictBufs {               // a sorted dictionary on the device: keys, then ONE look-up form: minimizer
            DevBuf keys, idx, slots;    // buckets (mzlen > 0), or top-bits index (+ one-sector slots when sb > 0)
            DevBuf mzT, mzB;
            int ib = 1, sb = 0, mzlen = 0;
            u32 n = 0, mznb = 0;
            bool canon = false;         // Dict.canon: n canonical keys stand for nfull flanks (their reverse complements included)
            u32 nfull = 0;
            void bufs(Bufs& v) { v.insert(v.end(), {&keys, &idx, &slots, &mzT, &mzB}); }
            Dict view() const {
                Dict d{};
                d.keys = (const u64*)keys.p;
                d.idx = (const u32*)idx.p;
                d.slots = sb && slots.p ? (const uint4*)slots.p : nullptr;
                d.ib = ib;
                d.sb = sb;
                d.mzT = mzlen && mzT.p ? (const u64*)mzT.p : nullptr;
                d.mzB = (const u32*)mzB.p;
                d.mznb = mznb;
                d.mzlen = mzlen;
                d.canon = canon ? 1 : 0;
                return d;
            }
        };
        // per flank: piece 0 at [0], then for piece j >= 1 its own dictionary at [2 j - 1] and the combinations (pieces 0 .. j) at
        // [2 j] -- the flank's final dictionary is at [fd_last(len)]
        DictBufs fd[2][2 * FR_MAXP - 1], fin;         // fin: the composite keys of the groups present in all genomes
        static int fd_pieces(int len) { return (len + 31) / 32; }
        static int fd_plen(int len, int j) { const int np = fd_pieces(len); return len / np + (j < len % np ? 1 : 0); }
        static int fd_poff(int len, int j) { int o = 0; for (int q = 0; q < j; q++) o += fd_plen(len, q); return o; }
        static int fd_last(int len) { return fd_pieces(len) > 1 ? 2 * (fd_pieces(len) - 1) : 0; }
        FlankRank fr[2];
        // Geom.wfl lives in device memory: WFL_SLOTS pairs, one per composite geometry of a run (the kernels of two lanes
        // may still read the pair before), and their host mirror
        DevBuf flbuf;
        FlankRank flhost[8][2];
        int flslot = 0;
        std::vector<int> run_ids;       // genome ids of the latest kr_wide_run (a hit names its genome by its place here)
        DevBuf rows, rowtab;            // kr_wide_fetch_windows: the hits' windows as text, the genomes' base pointers
        DevBuf masks, keep, cnt, hitoff, cursor, hits, cibuf, tsum, tpos;
        DevBuf loc, loccur;             // round 6: the located member windows as a list (k_wide_locate), its cursor
        u64 located = 0;                // entries of that list in the last run (0: the dense form ran -- a group number per window start)
        bool use_slots = true;          // KR_OPT_WIDE_SLOTS
        bool ordered = false;           // KR_OPT_WIDE_ORDERED: order-preserving ranks (groups in the reference's order)
        bool use_share = true;          // KR_WIDE_SHARE env (A/B, tests): 0 = build the right spectrum even where it mirrors the left
        int lanes = 0;                  // sort lanes of kr_wide_run, forced by the run itself (1 while one cache of composite keys is shared); 0 = by KR_OPT_LANES
        bool packed_spectrum = true;    // KR_WIDE_SPECTRUM env (A/B, tests): 0 = the flank spectra from amplicon-long windows only (k_hist8w<1> / k_scatter1w<1>)
        DevBuf wcount;                  // valid windows per genome (k_count_windows) when the spectra are taken with the packed kernels
        bool share = false;             // last run: the right flank took the left dictionary (Geom.wshare)
        bool genome_cache = false;
        bool key_list = false;          // round 6: this run's composite keys as a list per genome (Geom.wlcnt) instead of 16 bytes per window start
        bool key_list_failed = false;   // a segment of such a list was too short in this call: the dense form from here on
        double key_list_frac = 0;       // the share of window starts the list was sized for
        u64 keys_listed = 0;            // entries of the genomes' key lists in the last run (0: dense)
        int batch = 0;                  // > 0: the sort + intersect phases of this run take the genomes in batches of so many (round 6: the
                                        // streaming form of kr_wide_run -- the sorted keys of ONE batch are resident, the dictionary of a
                                        // phase is the running intersection); 0 = all genomes at once
        std::vector<u64> nkeys;     // per genome of the last kr_wide_run: k-mer records (2 x valid windows)
        u32 nfin = 0;
        u64 ngroups = 0;                // (left,right) groups present in all genomes (= nfin unless the list is canonical)
        int64_t nhits = -1;
        // what the locate, count and emit passes of a run allocate: the first to go when memory is short (wide_make_room)
        void locate_bufs(Bufs& v) { v.insert(v.end(), {&masks, &keep, &cnt, &hitoff, &cursor, &hits, &cibuf, &loc}); }
        void bufs(Bufs& v) {
            fin.bufs(v);
            locate_bufs(v);
            v.insert(v.end(), {&loccur, &tsum, &tpos, &wcount, &flbuf, &rows, &rowtab});
            for (auto& flank : fd)
                for (DictBufs& d : flank) d.bufs(v);
        }
    } wide;
    // the one-genome scans (h_scan.inc), all in the locate context.  bufs(): a pass's device buffers, named here alone
    // (kr_destroy releases them); reset(): what another geometry leaves of a pass (kr_set_params_locate: no table, no result)
    // the seed table of a seed pass on the device (seed_table_build): the entries' text, the slots, the entry list, the
    // membership bitmap; slots = 0: no table
    struct SeedTable {
        DevBuf arena, table, list, bitmap;
        u64 slots = 0;
        void bufs(Bufs& v) { v.insert(v.end(), {&arena, &table, &list, &bitmap}); }
    };
    // the pair list of a product pass (pair_list_sort, pair_list_upload): (left << 32 | right) ascending, the pairs' rows
    struct PairList {
        DevBuf pairkeys, pairidx;
        u64 npairs = 0;
        void bufs(Bufs& v) { v.insert(v.end(), {&pairkeys, &pairidx}); }
    };
    // the locate pass (kr_set_params_locate / kr_locate_*: h_locate.inc)
    struct Loc {
        bool on = false;
        int L = 0, D = 0, R = 0, k = 0, omit = 0;
        u64 ngroups = 0, slots = 0;
        int64_t nhits = -1;
        int gid = -1;                   // the genome of the latest kr_locate_scan
        DevBuf arena, table, bitmap, hits, seps, rows;
        DevBuf tcount, toff, flag;      // the two-pass scratch of all six passes (h_scan.inc: scan_two_pass)
        void bufs(Bufs& v) { v.insert(v.end(), {&arena, &table, &bitmap, &tcount, &toff, &flag, &hits, &seps, &rows}); }
    } loc;
    // the near-match pass (kr_near_*: h_near.inc), in the locate context: it shares loc's geometry and scratch
    struct Near {
        int M = 0;
        u64 ntargets = 0;
        int64_t nhits = -1;
        int gid = -1;                   // the genome of the latest kr_near_scan
        SeedTable seed;
        DevBuf hits, rows;
        void bufs(Bufs& v) { seed.bufs(v); v.insert(v.end(), {&hits, &rows}); }
        void reset() { seed.slots = ntargets = 0; nhits = -1; }
    } near;
    // the guide-hit pass (kr_guide_hits_*: h_guide_hits.inc), in the locate context with loc.k = the protospacer length:
    // a state of its own beside the near pass's, loc's scratch
    struct Ghit {
        int M = 0;
        GhitMotifs gm = {0, 0, 0, 0};
        u32 need = 0;                   // need_pam
        u64 nguides = 0;
        int64_t nhits = -1;
        int gid = -1;                   // the genome of the latest kr_guide_hits_scan
        SeedTable seed;
        DevBuf pairs, hits, kept, rows; // pairs: the scan's list; kept: what need_pam leaves (it changes places with hits)
        DevBuf tally;                   // kr_guide_hits_tally's counters
        void bufs(Bufs& v) { seed.bufs(v); v.insert(v.end(), {&pairs, &hits, &kept, &rows, &tally}); }
        void reset() { seed.slots = nguides = 0; nhits = -1; }
    } ghit;
    // the bulged guide-hit pass (kr_guide_bulges_*: h_guide_bulges.inc), in the same context: a state of its own beside ghit.
    // seed: the table of the guides' halves of h letters; texts: the entries' whole text
    struct Gbulge {
        int M = 0, B = 0;
        u32 h = 0, need = 0;
        GhitMotifs gm = {0, 0, 0, 0};
        u64 nguides = 0;
        int64_t nhits = -1;
        int gid = -1;                   // the genome of the latest kr_guide_bulges_scan
        SeedTable seed;
        DevBuf texts, pairs, hits, rows;
        void bufs(Bufs& v) { seed.bufs(v); v.insert(v.end(), {&texts, &pairs, &hits, &rows}); }
        void reset() { seed.slots = nguides = 0; nhits = -1; }
    } gbulge;
    // the product pass (kr_products_*: h_products.inc), in the locate context: loc.L / loc.R are the texts' lengths
    struct Prod {
        int M = 0;
        u32 max_product = 0;
        u64 nleft = 0, nright = 0;
        int64_t nsites = -1, nhits = -1;
        SeedTable seed;
        PairList plist;
        DevBuf seps, sites, rec, hits;
        void bufs(Bufs& v) { seed.bufs(v); plist.bufs(v); v.insert(v.end(), {&seps, &sites, &rec, &hits}); }
        void reset() { seed.slots = 0; nsites = nhits = -1; }
    } prod;
    // the primer-product pass (kr_primers_*: h_primers.inc), in the locate context: the product pass's state for texts of
    // mixed lengths, smin .. maxlen, entry e's text at eoff[e]
    struct Prim : Prod {
        u32 smin = 0, maxlen = 0;
        int gid = -1;                   // the genome of the latest kr_primers_scan
        DevBuf eoff, plen;              // plen: pair p's two text lengths (left | right << 16), what the assay join reads
        DevBuf pair_tally;              // kr_primers_tally's counters
        void bufs(Bufs& v) { Prod::bufs(v); v.insert(v.end(), {&eoff, &plen, &pair_tally}); }
    } prim;
    // the assay join (kr_assay_*: h_assay.inc), in the same context: the links (primer pair << 32 | guide, ascending) and the
    // assay hits of the latest join of prim's products with ghit's hits.  on: a link table stands (it may be empty)
    struct Assay {
        bool on = false;
        u64 nlinks = 0;
        int64_t nhits = -1;
        DevBuf links, hits;
        void bufs(Bufs& v) { v.insert(v.end(), {&links, &hits}); }
        void reset() { on = false; nlinks = 0; nhits = -1; }
    } assay;
    // the multiplex pass (kr_multiplex_*: h_multiplex.inc), in the same context: the primer pass's state once more, a table
    // of its own with nleft = the texts and nright = 0 and no pair list; hits holds kr_multiplex_hit
    struct Mux : Prim {
        DevBuf tally;                   // kr_multiplex_tally's counters
        void bufs(Bufs& v) { Prim::bufs(v); v.push_back(&tally); }
    } mux;
    // the clean panel selection's site store (kr_panel_sites_*, kr_panel_run_clean: h_panel_clean.inc), in the same context:
    // tab = the primer pass's state a third time (a table of all candidates' texts, nright = 0, no pair list; its sites and
    // rec are the latest scan's); sites / unit = the store of every scan since the table, nstore sites, units records
    struct Pclean {
        Prim tab;
        u64 nstore = 0, units = 0, nown = 0;   // (nown: the owners' list of the latest run)
        DevBuf sites, unit;
        DevBuf rows, ooff, own;         // a run's: the candidates' table rows, the texts' owners
        void bufs(Bufs& v) { tab.bufs(v); v.insert(v.end(), {&sites, &unit, &rows, &ooff, &own}); }
        void reset() { tab.reset(); nstore = units = 0; }
    } pclean;
    // the primer design pass (kr_design_*: h_design.inc): no genome, no geometry of another pass
    struct Design {
        bool on = false;
        kr_design_params params{};
        int64_t nrec = -1;
        bool hp = false, hp_ran = false;        // kr_design_hairpins is on; the latest run had it on
        DevBuf par, tmpl, rec, hprec;           // (tmpl, rec, hprec: a batch's; kr_design_run and kr_design_run_top take turns on them)
        std::vector<kr_design_record> out;      // the records of the latest run, all batches
        std::vector<int32_t> hp_out;            // ... and, with the hairpin check, its two figures a region
        // kr_design_run_top's own list and state: regions * top records, region-major, and two figures a record
        int64_t top_nrec = -1;
        bool top_hp_ran = false;
        std::vector<kr_design_record> top_out;
        std::vector<int32_t> top_hp_out;
    } design;
    // the panel pass (kr_panel_*: h_panel.inc): all candidates resident, the model and max_sec are design's
    struct Panel {
        int64_t nmem = -1;                      // members of the latest run
        u64 ncand = 0;
        DevBuf tmpl, pairs, state, cross, pick;
        std::vector<kr_panel_member> members;   // the latest run's, in order of acceptance
        std::vector<uint8_t> fates;             // ... and (fate, by) per candidate
    } panel;
    // the guide pass (kr_guides_*: h_guides.inc): no genome, no geometry of another pass
    struct Guides {
        bool on = false;
        kr_guide_params params{};
        int64_t nrec = -1;
        DevBuf rows, off, bnd, rec;             // (a batch's: kr_guides_run and kr_guides_run_top take turns on them)
        std::vector<kr_guide_record> out;       // the records of the latest run, all batches
        int64_t top_nrec = -1;                  // kr_guides_run_top's own: regions * top records, region-major
        std::vector<kr_guide_record> top_out;
    } guides;
};

static int fail(kr_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(c, call)                                                                       \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail((c), KR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

static int ensure(kr_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes < 16) bytes = 16;
    if (b.bytes >= bytes) return KR_OK;
    if (b.p) {
        (void)hipDeviceSynchronize();
        (void)hipFree(b.p);
        c->used -= b.bytes;
        b.p = nullptr;
        b.bytes = 0;
    }
    if (c->budget && c->used + bytes > c->budget)
        return fail(c, KR_ERR_CAPACITY, "hbm budget exceeded: need %zu more bytes, %zu of %zu in use", bytes,
                    c->used, c->budget);
    {
        // (a device without room is a CAPACITY answer, as an exhausted budget is: the callers that can work in smaller
        // pieces -- the streaming flow of the command line -- take it as "does not fit", not as a failure of the device)
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            b.p = nullptr;
            return fail(c, KR_ERR_CAPACITY, "device memory exhausted: %zu more bytes wanted, %zu in use by this context", bytes, c->used);
        }
        HIPCHK(c, e);
    }
    b.bytes = bytes;
    c->used += bytes;
    static const bool trace = getenv("KR_TRACE_ALLOC") != nullptr;      // (debug aid: where the big buffers land)
    if (trace && bytes >= ((size_t)64 << 20)) fprintf(stderr, "[krisp_hip] alloc %p + %zu MB\n", b.p, bytes >> 20);
    return KR_OK;
}

// grow a buffer that holds live data: contents are preserved
static int ensure_keep(kr_ctx* c, DevBuf& b, size_t bytes, size_t live_bytes) {
    if (b.bytes >= bytes) return KR_OK;
    size_t want = std::max(bytes, b.bytes * 2);
    DevBuf nb;
    int rc = ensure(c, nb, want);
    if (rc) return rc;
    if (b.p && live_bytes) {
        hipError_t e = hipMemcpy(nb.p, b.p, live_bytes, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(c, KR_ERR_HIP, "hipMemcpy D2D failed: %s", hipGetErrorString(e));
    }
    if (b.p) {
        (void)hipFree(b.p);
        c->used -= b.bytes;
    }
    b = nb;
    return KR_OK;
}

static void release(kr_ctx* c, DevBuf& b) {
    if (b.p) {
        (void)hipFree(b.p);
        c->used -= b.bytes;
    }
    b.p = nullptr;
    b.bytes = 0;
}

#define MB_WORDS 65536
#define MB_SLICE0 64
#define PUB_CAP 4096        // slices one k_publish_slices launch takes (its table follows the mailbox words)
static int mbox_slot(kr_ctx* c) {
    if (!c->mb_free.empty()) { const int s = c->mb_free.back(); c->mb_free.pop_back(); return s; }
    if (MB_SLICE0 + 2 * (c->mb_next + 1) > MB_WORDS) return -1;
    return c->mb_next++;
}

// The pool of placed pass-1 targets for coarse genomes (coarse_pool_grow, behind ensure_placed, makes them).  A buffer is
// either in the free list or held by one genome (Genome.ckeys).  A genome that leaves the coarse state gives its buffer
// back; the buffers are freed with the context or its parameters.
// The hazard between owners: a buffer carries an event behind the last kernel that touched it -- the pass 1 that wrote
// it, the probe that read it -- and the lane that writes it next waits for that event.  The event is recorded where the
// buffer changes hands (a return, a sort on another stream), not behind every kernel: in the steady state -- the same
// genome on the same buffer step after step, kr_intersect's closing synchronisation behind every probe -- no event call
// is made at all (an event behind each pass 1 and each probe, and a wait in front of each pass 1, cost a one-lane step
// 45 us of idle device between its kernels: profiles/r13/README.md).
static void coarse_pool_handover(kr_ctx* c, Genome& G) {
    if (!G.ckeys.p || !G.ckeys_busy) return;
    if (!G.ckeys_ev && hipEventCreateWithFlags(&G.ckeys_ev, hipEventDisableTiming) != hipSuccess) G.ckeys_ev = nullptr;
    if (G.ckeys_ev && hipEventRecord(G.ckeys_ev, G.ckeys_busy) == hipSuccess) G.ckeys_wait = true;
    else (void)hipStreamSynchronize(G.ckeys_busy);          // (no event to be had: the host waits instead)
    G.ckeys_busy = nullptr;
    (void)c;
}
static void coarse_pool_return(kr_ctx* c, Genome& G) {
    if (!G.ckeys.p) return;
    coarse_pool_handover(c, G);
    kr_ctx::PoolBuf pb{G.ckeys, G.ckeys_ms, G.ckeys_ev, G.ckeys_wait};
    auto at = c->cpool_free.begin();
    while (at != c->cpool_free.end() && at->ms <= pb.ms) ++at;
    c->cpool_free.insert(at, pb);
    G.ckeys = DevBuf();
    G.ckeys_ms = 0;
    G.ckeys_ev = nullptr;
    G.ckeys_wait = false;
}
// free buffers shorter than `bytes` (the lanes' scratch has grown since they were made) leave the pool
static void coarse_pool_purge(kr_ctx* c, size_t bytes) {
    for (size_t i = c->cpool_free.size(); i-- > 0;) {
        kr_ctx::PoolBuf& pb = c->cpool_free[i];
        if (pb.buf.bytes >= bytes) continue;
        if (pb.ev) { if (pb.wait) (void)hipEventSynchronize(pb.ev); (void)hipEventDestroy(pb.ev); }
        release(c, pb.buf);
        c->cpool_free.erase(c->cpool_free.begin() + (long)i);
        c->cpool_total--;
    }
}
// the fastest free buffer of at least `bytes`, if there is one
static bool coarse_pool_take(kr_ctx* c, Genome& G, size_t bytes) {
    for (auto at = c->cpool_free.begin(); at != c->cpool_free.end(); ++at)
        if (at->buf.bytes >= bytes) {
            G.ckeys = at->buf;
            G.ckeys_ms = at->ms;
            G.ckeys_ev = at->ev;
            G.ckeys_wait = at->wait;
            G.ckeys_busy = nullptr;
            c->cpool_free.erase(at);
            return true;
        }
    return false;
}
// (the caller has returned every genome's buffer, or there are no genomes: kr_destroy, kr_set_params*)
static void coarse_pool_release(kr_ctx* c) {
    if (c->cpool_free.empty()) return;
    (void)hipDeviceSynchronize();
    for (auto& pb : c->cpool_free) {
        release(c, pb.buf);
        if (pb.ev) (void)hipEventDestroy(pb.ev);
    }
    c->cpool_total -= (int)c->cpool_free.size();
    c->cpool_free.clear();
}

// a slice's arrays and its pair of mailbox words
static void release_slice(kr_ctx* c, Slice& S) {
    release(c, S.keys);
    release(c, S.off);
    release(c, S.chunkstart);
    release(c, S.chunkdesc);
    release(c, S.ovf);
    if (S.res >= 0) c->mb_free.push_back(S.res);
}
// a genome's sorted keys go back (its slice plan with them: kr_wide_run makes one per phase)
static void genome_drop_sorted(kr_ctx* c, Genome& G) {
    for (Slice& S : G.sl) release_slice(c, S);
    G.sl.clear();
    G.sorted = G.finalized = G.ordered = false;
}
// a genome whose slices were planned for another slice count starts over with the context's
static void reset_slices(kr_ctx* c, Genome& G) {
    if ((int)G.sl.size() == c->nslices) return;
    for (Slice& S : G.sl) release_slice(c, S);
    G.sl.assign(c->nslices, Slice());
}
// what every new upload and every new sort makes of a genome's state
static void genome_unsorted(Genome& G) {
    G.sorted = G.finalized = G.ordered = G.coarse = G.one_strand = G.hits_valid = false;
    G.count = -1;
}

static void release_genome(kr_ctx* c, Genome& G) {
    coarse_pool_return(c, G);
    if (G.up_done) { (void)hipEventDestroy(G.up_done); G.up_done = nullptr; }
    release(c, G.bases);
    release(c, G.wkeys);
    release(c, G.wlcnt);
    release(c, G.hits);
    for (Slice& S : G.sl) release_slice(c, S);
    G.sl.clear();
}

struct StageScope {
    kr_ctx* c;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t stream;
    StageScope(kr_ctx* c_, int st, hipStream_t s_ = nullptr) : c(c_), stage(st), stream(s_ ? s_ : c_->stream) {
        c->stage_n[st]++;
        if (!c->stage_on || !((c->stage_mask >> st) & 1u)) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!c->pool.empty()) { e = c->pool.back(); c->pool.pop_back(); }
            else (void)hipEventCreate(&e);
            return e;
        };
        a = get();
        b = get();
        (void)hipEventRecord(a, stream);
    }
    ~StageScope() {
        if (!a) return;
        (void)hipEventRecord(b, stream);
        c->pending.push_back({a, b, stage});
    }
};

static void resolve_stages(kr_ctx* c) {
    for (auto& p : c->pending) {
        float ms = 0;
        (void)hipEventSynchronize(p.b);
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) c->stage_ms[p.stage] += ms;
        c->pool.push_back(p.a);
        c->pool.push_back(p.b);
    }
    c->pending.clear();
}

// Lanes in use: consecutive genome sorts go to consecutive lanes (own stream, own scratch) and overlap on the device --
// the small histogram / table kernels of one genome run beside the streaming passes of another, and the passes, each
// bound by something else (pass 1: instructions and writes, pass 2: scatter latency, LDS sort: instructions), fill
// each other's gaps: 3 lanes -7 % per step on 4 x 50 Mbp (profiles/r03/README.md).  One lane for wide windows (the
// per-genome key caches assume it) and for key-space slices (a lane then holds a pass-0 array of the whole genome).
// Automatic (the default): one lane until the context has sorted LANES_AFTER genomes, LANES_AUTO from then on -- a
// lane's scratch costs ~10 ms to set up (allocation, the placement probes of KR_OPT_PLACE_TRIES), more than a
// one-shot run over a handful of genomes gets back (tools/e2e_check.py: 0.165 s with one lane, 0.191 s with three).
#define LANES_AUTO 3
#define LANES_AFTER 16
static inline int lanes_used(const kr_ctx* c) {
    // kr_wide_run: two lanes when the caller asked for several (KR_OPT_LANES > 1) -- a genome's look-up-bound key
    // generation then runs beside the streaming passes of the genome before it (configs[2], round 3: 355 -> 334 ms with
    // two, 345 with three) --, one otherwise: a second lane's scratch (a pass-0 array of the whole
    // genome) costs a one-shot run more than it returns
    if (c->wide.on) return c->wide.lanes > 0 ? c->wide.lanes : (c->nlanes > 1 ? 2 : 1);
    if (c->g.wmode) return 1;
    // key-space slices (round 4): two genome lanes -- a lane holds a pass-0 array of the whole genome, made when the
    // lane first sorts one --, each with a helper lane its slices alternate with (genome_sort); KR_OPT_LANES = 1: one
    // (automatic: the second genome lane -- another pass-0 array of a whole genome, seconds of hipMalloc at 3 Gbp -- when
    // the context has sorted two sliced genomes and goes on: a one-shot run over two genomes does not get it back)
    if (c->nslices > 1) return c->nlanes == 1 || (c->nlanes == 0 && c->sorts_done < 2) ? 1 : 2;
    return c->nlanes > 0 ? c->nlanes : (c->sorts_done >= LANES_AFTER ? LANES_AUTO : 1);
}

// make the main stream wait for every lane that has sorts in flight
static int join_lanes(kr_ctx* c) {
    for (int i = 1; i < MAX_LANES; i++) {
        Lane& ln = c->lanes[i];
        if (!ln.pending) continue;
        HIPCHK(c, hipEventRecord(ln.done, ln.stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, ln.done, 0));
        ln.pending = false;
    }
    return KR_OK;
}

// a lane's stream and `done` event, made when the lane is first used
static int lane_open(kr_ctx* c, Lane& ln) {
    if (ln.stream) return KR_OK;
    HIPCHK(c, hipStreamCreate(&ln.stream));
    HIPCHK(c, hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
    return KR_OK;
}
// the scratch of lanes first .. MAX_LANES - 1 goes back
static void release_lanes(kr_ctx* c, int first) {
    std::vector<DevBuf*> lb;
    for (int i = first; i < MAX_LANES; i++) c->lanes[i].bufs(lb);
    for (DevBuf* b : lb) release(c, *b);
}
// k_hist16's list of counts beyond 16 bits: its count is cleared once, on `st` (k_chunk_table clears it after every use)
static int ensure_h16exc(kr_ctx* c, Lane& ln, hipStream_t st) {
    if (ln.h16exc.p) return KR_OK;
    int rc;
    if ((rc = ensure(c, ln.h16exc, (1 + 3 * (size_t)H16_EXC_CAP) * 4))) return rc;
    HIPCHK(c, hipMemsetAsync(ln.h16exc.p, 0, 16, st));
    return KR_OK;
}

// the exclusive scan of n counts, tiled: sums of tiles of 2048 into tsum, their scan into tpos (a word per tile and
// four more each), the positions into out -- out[n] is the total; out may be `in`
static void launch_excl_scan(hipStream_t st, const u32* in, u32 n, u32* tsum, u32* tpos, u32* out) {
    const u32 ntiles = (n + 2047) / 2048;
    hipLaunchKernelGGL(k_tile_sums, dim3(ntiles), dim3(256), 0, st, in, n, tsum);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)tsum, tpos, ntiles);
    hipLaunchKernelGGL(k_tile_apply, dim3(ntiles), dim3(256), 0, st, in, n, (const u32*)tpos, ntiles, out);
}

extern "C" {

const char* kr_last_error(kr_ctx* c) { return c ? c->err.c_str() : g_last_error.c_str(); }

kr_ctx* kr_create(int device, size_t hbm_budget_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_last_error = "no HIP device visible";
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        g_last_error = "device index out of range";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_last_error = "hipSetDevice failed";
        return nullptr;
    }
    kr_ctx* c = new kr_ctx();
    c->device = device;
    c->budget = hbm_budget_bytes;
    {
        // environment defaults of the result-neutral options (kr_set_option overrides them); KR_DBG
        // is masked to its one documented bit: the ablation switches change results
        const char* e = getenv("KR_DBG");
        c->dbg = e ? (atoi(e) & 32) : 0;
        const char* e2 = getenv("KR_ISECT_FMT");
        c->isect_fmt = e2 ? (atoi(e2) == 1 ? 1 : (atoi(e2) == 2 ? 2 : 0)) : 0;
        const char* e3 = getenv("KR_SLICE_BASES");
        c->opt_slice_bases = e3 ? std::max(0, std::min(4, atoi(e3))) : -1;
        const char* e16 = getenv("KR_FUSE_ANCHOR");
        c->fuse_anchor = e16 ? atoi(e16) != 0 : 1;
        const char* e15 = getenv("KR_LAZY_ORDER");
        c->lazy_order = e15 ? atoi(e15) != 0 : 1;
        const char* e17 = getenv("KR_COARSE_REST");
        c->coarse_rest = e17 ? atoi(e17) != 0 : 1;
        const char* e21 = getenv("KR_COARSE_POOL");
        c->coarse_pool = e21 ? atoi(e21) != 0 : 1;
        const char* e26 = getenv("KR_COARSE_ONE_STRAND");
        c->coarse_one = e26 ? atoi(e26) != 0 : 1;
        const char* e27 = getenv("KR_COARSE_ONE_PASS");
        c->coarse_pass = e27 ? atoi(e27) != 0 : 1;
        const char* e22 = getenv("KR_PLACE_MIN_BYTES");
        if (e22) c->place_min_bytes = (size_t)std::max(0ll, atoll(e22));
        const char* e18 = getenv("KR_COARSE_TCAP");
        if (e18) c->co_tcap = (u32)std::max(1, std::min((int)CO_TCAP, atoi(e18)));
        const char* e19 = getenv("KR_COARSE_HITCAP");
        if (e19) c->co_hitcap = (u32)std::max(1, atoi(e19));
        const char* e20 = getenv("KR_COARSE_GRID");
        if (e20) c->co_grid = (u32)std::max(0, std::min(65536, atoi(e20)));
        const char* e24 = getenv("KR_JOIN2");
        c->join2 = e24 ? atoi(e24) != 0 : 1;
        const char* e28 = getenv("KR_JOIN2_DENSE");
        c->join2_dense = e28 ? atoi(e28) != 0 : 1;
        const char* e25 = getenv("KR_JOIN2_GRID");
        if (e25) c->j2_grid = (u32)std::max(0, std::min(65536, atoi(e25)));
        const char* e23 = getenv("KR_SCAN_GRID");
        if (e23) c->scan_cap = (u32)std::max(0, std::min(65536, atoi(e23)));
        const char* e13 = getenv("KR_SLICE_ROUTE");
        c->slice_route = e13 ? atoi(e13) != 0 : 1;
        const char* e8 = getenv("KR_PLACE_TRIES");
        c->place_tries = e8 ? std::max(1, std::min(16, atoi(e8))) : 8;
        c->place_tries_set = e8 != nullptr;
        const char* e4 = getenv("KR_WIDE_SLOTS");
        c->wide.use_slots = e4 ? atoi(e4) != 0 : true;
        const char* e7 = getenv("KR_WIDE_SHARE");
        c->wide.use_share = e7 ? atoi(e7) != 0 : true;
        const char* e11 = getenv("KR_WIDE_SPECTRUM");
        c->wide.packed_spectrum = e11 ? atoi(e11) != 0 : true;
        const char* e5 = getenv("KR_WIDE_ORDERED");
        c->wide.ordered = e5 ? atoi(e5) != 0 : false;
        int ncu = 256, per = 3;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_localsort2, LS_THREADS, 0) != hipSuccess || per < 1)
            per = 2;
        c->ls_grid = ncu * per;
        c->ncu = ncu;
        const char* e9 = getenv("KR_ISECT_KERNEL");
        c->isect_kernel = e9 ? (atoi(e9) == 1 ? 1 : (atoi(e9) == 2 ? 2 : 0)) : 0;
        const char* e10 = getenv("KR_ISECT_OVF_CAP");
        if (e10) c->i3_ovf_cap = (u32)std::max(0, std::min((int)I3_OVF_CAP, atoi(e10)));
    }
    {
        const char* e = getenv("KR_LANES");
        int nl = e ? atoi(e) : 0;
        c->nlanes = nl < 0 ? 0 : (nl > MAX_LANES ? MAX_LANES : nl);
    }
    bool ok = hipHostMalloc((void**)&c->mbox, MB_WORDS * 4 + PUB_CAP * sizeof(PubEnt), hipHostMallocMapped) == hipSuccess &&
              hipEventCreate(&c->t0) == hipSuccess && hipEventCreate(&c->t1) == hipSuccess &&
              hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && lane_open(c, c->lanes[0]) == KR_OK;      // (the other lanes get their streams when they are first used: ensure_lanes)
    if (!ok) {
        g_last_error = "stream / event creation failed";
        delete c;
        return nullptr;
    }
    c->stream = c->lanes[0].stream;
    return c;
}

int kr_comm_destroy(kr_ctx* c);

void kr_destroy(kr_ctx* c) {
    if (!c) return;
    (void)kr_comm_destroy(c);
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    resolve_stages(c);
    release_lanes(c, 0);
    for (auto& kv : c->genomes) release_genome(c, kv.second);
    coarse_pool_release(c);
    DevBuf* all[] = {&c->candA, &c->candB, &c->chunkcnt,
                     &c->chunkpos, &c->flags, &c->blockcnt, &c->blockpos, &c->other, &c->records, &c->nrec, &c->fbdesc, &c->fbsegs,
                     &c->coltab, &c->collo, &c->colcnt, &c->colpos, &c->coltsum, &c->coltpos, &c->colfirst, &c->colfm, &c->isovf,
                     &c->bgz_in, &c->bgz_tab, &c->bgz_stat, &c->tx_scan, &c->tx_text, &c->tx_tile, &c->tx_tilepos, &c->tx_lines, &c->tx_ls, &c->tx_ll, &c->tx_op, &c->tx_outpos, &c->tx_state,
                     &c->tx_tsum, &c->tx_tpos, &c->candP, &c->touchdesc, &c->touchovf, &c->co_state, &c->co_tab, &c->co_ent};
    for (DevBuf* b : all) release(c, *b);
    {
        kr_ctx::Bufs sb;                // the wide path's and the one-genome scans': every pass hands over its own
        c->wide.bufs(sb);
        c->loc.bufs(sb); c->near.bufs(sb); c->ghit.bufs(sb); c->gbulge.bufs(sb); c->prod.bufs(sb); c->prim.bufs(sb); c->assay.bufs(sb); c->mux.bufs(sb); c->pclean.bufs(sb);
        for (DevBuf* b : sb) release(c, *b);
        auto& ds = c->design;
        DevBuf* db[] = {&ds.par, &ds.tmpl, &ds.rec, &ds.hprec};
        for (DevBuf* b : db) release(c, *b);
        auto& gu = c->guides;
        DevBuf* gb[] = {&gu.rows, &gu.off, &gu.bnd, &gu.rec};
        for (DevBuf* b : gb) release(c, *b);
        auto& pn = c->panel;
        DevBuf* pb[] = {&pn.tmpl, &pn.pairs, &pn.state, &pn.cross, &pn.pick};
        for (DevBuf* b : pb) release(c, *b);
    }
    if (c->mbox) (void)hipHostFree(c->mbox);
    for (auto e : c->pool) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (hipEvent_t e : c->slice_ready) if (e) (void)hipEventDestroy(e);
    (void)hipEventDestroy(c->t0);
    (void)hipEventDestroy(c->t1);
    for (int i = 0; i < MAX_LANES; i++) {
        if (c->lanes[i].done) (void)hipEventDestroy(c->lanes[i].done);
        if (c->lanes[i].stream) (void)hipStreamDestroy(c->lanes[i].stream);
    }
    delete c;
}

static u64 topbits(int nbits) { return nbits <= 0 ? 0ull : (nbits >= 64 ? ~0ull : (~0ull << (64 - nbits))); }

// geometry of slice `slice` (relative part) on top of the context's absolute geometry
static Geom slice_geom(const kr_ctx* c, u32 slice) {
    Geom g = c->g;
    g.slice = slice;
    return g;
}

// absolute + relative geometry of (L, D, R) windows sorted in 4^sb slices with fan-out 2^b
#define KR_RETRY_DENSE (-1000)       // internal (count_slices -> phase_sort_intersect): a key-list segment was too short, take the dense form
static Geom make_geom(int L, int D, int R, int omit, int sb, int b) {
    Geom g{};
    const int k = L + D + R;
    g.k = k; g.L = L; g.D = D; g.R = R;
    g.sR = 2 * D;
    g.sD = 2 * R;
    g.topmask = topbits(2 * k);
    g.mL = topbits(2 * L);
    g.mR = topbits(2 * (L + R)) & ~g.mL;
    g.mD = topbits(2 * k) & ~topbits(2 * (L + R));
    g.omit = omit;
    g.allow = 15;
    g.sbits = 2 * sb;
    g.slice = 0;
    g.LRrel = L - sb + R;
    g.pmask = topbits(2 * g.LRrel);
    g.b = b;
    g.rb = 64 - b;
    return g;
}

// key-space slices: one sort unit holds at most ~4.2e8 keys (fine buckets of <= 1600 keys at the
// largest fan-out b = 18); larger genomes are sorted in 4^sb slices by the first sb bases of `left`.
// fan-out: average fine bucket of ~1600 keys or fewer (limit LS_CAP - LS_T = 2048), 8 <= b <= 18
static int plan_sort(kr_ctx* c, size_t max_bases, int Lmin, int& sb, int& b) {
    const u64 nmax = 2 * (u64)max_bases;
    sb = 0;
    while (sb < 4 && (nmax >> (2 * sb)) > (BUCKET_AVG << 18)) sb++;
    // once slices are needed, finer ones pay: a slice of <= 1e8 keys sorts with fan-out 2^16, whose
    // pass-2 runs are 256 bytes instead of 64 (C5: 33.0 -> 36.4 G k-mers/s with 64 instead of 16 slices)
    if (sb > 0)
        while (sb < 4 && sb < Lmin && (nmax >> (2 * sb)) > (BUCKET_AVG << 16)) sb++;
    const bool forced = c->opt_slice_bases >= 0;
    if (forced) sb = c->opt_slice_bases;
    if (sb > Lmin) {
        if (forced) sb = Lmin;
        else return fail(c, KR_ERR_PARAM, "a genome of %zu bases needs %d slice bases but conserved-left is %d", max_bases, sb, Lmin);
    }
    if ((nmax >> (2 * sb)) > (BUCKET_AVG << 18) * 4)
        return fail(c, KR_ERR_PARAM, "genome of %zu bases is too large for %d slice bases", max_bases, sb);
    if (sb == 0 && nmax >= KR_MAX_SLICE_KEYS)
        return fail(c, KR_ERR_CAPACITY, "a genome of %zu bases gives up to %llu keys in one sort unit (the limit is %llu, "
                    "the 4 GiB a buffer descriptor spans): use key-space slices (KR_OPT_SLICE_BASES >= 1)", max_bases,
                    (unsigned long long)nmax, (unsigned long long)KR_MAX_SLICE_KEYS);
    const u64 per_slice = nmax >> (2 * sb);
    b = 8;
    while (b < 18 && (per_slice >> b) > BUCKET_AVG) b++;
    return KR_OK;
}

int kr_set_params(kr_ctx* c, int L, int D, int R, int softmask_mode, size_t max_bases) {
    if (!c) return KR_ERR_PARAM;
    const int k = L + D + R;
    if (L < 0 || D < 0 || R < 0 || k < 1 || k > 32)
        return fail(c, KR_ERR_PARAM, "need 1 <= L+D+R <= 32 on the packed path (got %d/%d/%d)", L, D, R);
    if (D > 16) return fail(c, KR_ERR_PARAM, "diagnostic length %d > 16 unsupported by the mask format", D);
    if (softmask_mode != KR_SOFT_MAP && softmask_mode != KR_SOFT_OMIT)
        return fail(c, KR_ERR_PARAM, "unknown softmask mode %d", softmask_mode);
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_params after genomes were uploaded");
    coarse_pool_release(c);
    // (round 6: base positions, word indexes and key counts of the packed path are 64 bits throughout -- k_pack, k_hist8,
    // k_scatter1p<., BIG>, k_hist16, the pass-0 array; the code words of a genome stay below the 4 GiB a buffer descriptor
    // spans up to 2^34 bases.  KR_MAX_BASES = 2^33: 1.7e10 keys of 8 bytes twice -- pass 0 and the slices -- are what one
    // GPU's 288 GB hold of ONE genome at all.  The device's text reader indexes 32 bits: longer texts are parsed on the host.)
    if (max_bases >= KR_MAX_BASES) return fail(c, KR_ERR_PARAM, "genomes of >= 2^33 bases are not supported");
    int sb, b, rc;
    if ((rc = plan_sort(c, max_bases, L, sb, b))) return rc;
    c->sb = sb;
    c->nslices = 1 << (2 * sb);
    c->g = make_geom(L, D, R, softmask_mode == KR_SOFT_OMIT, sb, b);
    c->max_bases = max_bases;
    c->have_params = true;
    c->wide.on = false;
    c->custom_layout = false;
    return KR_OK;
}

static int ensure_lanes(kr_ctx* c, u64 maxcount);

int kr_set_option(kr_ctx* c, int option, int64_t value) {
    if (!c) return KR_ERR_PARAM;
    switch (option) {
    case KR_OPT_SLICE_BASES:
        if (value < -1 || value > 4) return fail(c, KR_ERR_PARAM, "KR_OPT_SLICE_BASES: -1 .. 4");
        if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "KR_OPT_SLICE_BASES after genomes were uploaded");
        c->opt_slice_bases = (int)value;
        return KR_OK;
    case KR_OPT_GENERIC_INTERSECT:
        c->dbg = (c->dbg & ~32) | (value ? 32 : 0);
        return KR_OK;
    case KR_OPT_ISECT_FORMAT:
        if (value < 0 || value > 2) return fail(c, KR_ERR_PARAM, "KR_OPT_ISECT_FORMAT: 0, 1 or 2");
        c->isect_fmt = (int)value;
        return KR_OK;
    case KR_OPT_ISECT_KERNEL:
        if (value < 0 || value > 2) return fail(c, KR_ERR_PARAM, "KR_OPT_ISECT_KERNEL: 0, 1 or 2");
        c->isect_kernel = (int)value;
        return KR_OK;
    case KR_OPT_WIDE_SLOTS:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_WIDE_SLOTS: 0 or 1");
        c->wide.use_slots = value != 0;
        return KR_OK;
    case KR_OPT_LANES:
        if (value < 0 || value > MAX_LANES) return fail(c, KR_ERR_PARAM, "KR_OPT_LANES: 0 (automatic), 1 .. %d", MAX_LANES);
        // (any time: the sorts in flight are joined first, a lane that has no scratch yet gets it now)
        HIPCHK(c, hipSetDevice(c->device));
        { int rcj = join_lanes(c); if (rcj) return rcj; }
        HIPCHK(c, hipDeviceSynchronize());
        c->nlanes = (int)value;
        c->next_lane = 0;
        return (c->have_params && c->lane_maxcount) ? ensure_lanes(c, c->lane_maxcount) : KR_OK;
    case KR_OPT_PLACE_TRIES:
        if (value < 1 || value > 16) return fail(c, KR_ERR_PARAM, "KR_OPT_PLACE_TRIES: 1 .. 16");
        c->place_tries = (int)value;
        c->place_tries_set = true;
        return KR_OK;
    case KR_OPT_WIDE_ORDERED:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_WIDE_ORDERED: 0 or 1");
        c->wide.ordered = value != 0;
        return KR_OK;
    case KR_OPT_LAZY_ORDER:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_LAZY_ORDER: 0 or 1");
        c->lazy_order = (int)value;
        return KR_OK;
    case KR_OPT_COARSE_REST:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_COARSE_REST: 0 or 1");
        c->coarse_rest = (int)value;
        return KR_OK;
    case KR_OPT_COARSE_POOL:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_COARSE_POOL: 0 or 1");
        c->coarse_pool = (int)value;
        return KR_OK;
    case KR_OPT_COARSE_ONE_STRAND:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_COARSE_ONE_STRAND: 0 or 1");
        c->coarse_one = (int)value;
        return KR_OK;
    case KR_OPT_COARSE_ONE_PASS:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_COARSE_ONE_PASS: 0 or 1");
        c->coarse_pass = (int)value;
        return KR_OK;
    case KR_OPT_JOIN2:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_JOIN2: 0 or 1");
        c->join2 = (int)value;
        return KR_OK;
    case KR_OPT_JOIN2_DENSE:
        if (value != 0 && value != 1) return fail(c, KR_ERR_PARAM, "KR_OPT_JOIN2_DENSE: 0 or 1");
        c->join2_dense = (int)value;
        return KR_OK;
    case KR_OPT_ABLATE:
#ifdef KR_ABLATE
        c->dbg = (c->dbg & 32) | ((int)value & ~32);
        return KR_OK;
#else
        return fail(c, KR_ERR_PARAM, "KR_OPT_ABLATE needs a -DKR_ABLATE build");
#endif
    default:
        return fail(c, KR_ERR_PARAM, "unknown option %d", option);
    }
}

int kr_set_strands(kr_ctx* c, int mode) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (mode < KR_STRANDS_BOTH || mode > KR_STRANDS_CANONICAL) return fail(c, KR_ERR_PARAM, "unknown strand mode %d", mode);
    if (c->wide.on && mode == KR_STRANDS_CANONICAL) return fail(c, KR_ERR_PARAM, "the wide path emits both strands or the forward one");
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_strands after genomes were uploaded");
    c->g.strands = mode;
    c->wide.strands = mode;
    return KR_OK;
}

int kr_set_allow(kr_ctx* c, unsigned base_mask) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (base_mask > 15) return fail(c, KR_ERR_PARAM, "kr_set_allow: a mask of the four bases A C G T (bits 0..3)");
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_allow after genomes were uploaded");
    c->g.allow = base_mask;
    return KR_OK;
}

int kr_set_field_order(kr_ctx* c, const int* widths, const int* order) {
    if (!c || !c->have_params || c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (!widths || !order) return KR_ERR_PARAM;
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_field_order after genomes were uploaded");
    const int k = c->g.k;
    // (key-space slices -- genomes of more than 2^28 bases -- go by the top bits of the ORDERED key: the generic generators, the
    // pass 0 by the key's top bits and the slices' own histograms take any layout; round 6: no longer refused)
    if (c->g.D != 0 || c->g.R != 0 || c->g.L != k)
        return fail(c, KR_ERR_STATE, "kr_set_field_order: after kr_set_params(k, 0, 0, ...)");
    int seen = 0, sum = 0;
    for (int i = 0; i < 3; i++) {
        if (widths[i] < 0 || order[i] < 0 || order[i] > 2) return fail(c, KR_ERR_PARAM, "kr_set_field_order: widths >= 0, order a permutation of 0 1 2");
        seen |= 1 << order[i];
        sum += widths[i];
    }
    if (seen != 7 || sum != k) return fail(c, KR_ERR_PARAM, "kr_set_field_order: order must be a permutation of 0 1 2 and the widths add up to k = %d", k);
    // every field moves by dst - src bases: none (stays), towards the top of the key (left shift) or away from it.  One
    // left and one right shift are what layout_key has; an order that needs two of one direction -- (last, middle, first)
    // with outer fields of different widths -- is tried again behind a rotation of the window by a field boundary (the
    // fields stay whole, their sources move: rot = widths[0] or widths[0] + widths[1] bases)
    int src0[3], dst[3];
    src0[0] = 0; src0[1] = widths[0]; src0[2] = widths[0] + widths[1];
    for (int i = 0, at = 0; i < 3; i++) { dst[order[i]] = at; at += widths[order[i]]; }
    u64 mS = 0, mLf = 0, mRt = 0;
    int sLf = 0, sRt = 0, rot = -1;
    for (int r : {0, src0[1], src0[2]}) {
        if (r >= k) continue;
        mS = mLf = mRt = 0;
        sLf = sRt = 0;
        bool ok = true;
        for (int f = 0; f < 3 && ok; f++) {
            if (!widths[f]) continue;
            const int src = (src0[f] - r + k) % k;                  // where the field starts after the rotation
            if (src + widths[f] > k) { ok = false; break; }         // (the rotation would cut it: r is not one of its boundaries)
            const u64 m = topbits(2 * (dst[f] + widths[f])) & ~topbits(2 * dst[f]);       // where the field lies in the key
            const int mv = dst[f] - src;
            if (mv == 0) mS |= m;
            else if (mv < 0) {
                if (sLf && sLf != -2 * mv) ok = false;
                sLf = -2 * mv; mLf |= m;
            } else {
                if (sRt && sRt != 2 * mv) ok = false;
                sRt = 2 * mv; mRt |= m;
            }
        }
        if (ok) { rot = 2 * r; break; }
    }
    if (rot < 0) return fail(c, KR_ERR_PARAM, "kr_set_field_order: this order needs two different shifts of one direction");
    c->g.rot = rot;
    // layout_key (k_keys.inc): (w & mL) | ((w << sR) & mR) | ((w >> sD) & mD)
    c->g.mL = mS;
    c->g.sR = sLf; c->g.mR = mLf;
    c->g.sD = sRt; c->g.mD = mRt;
    // the kernels that read a key's top bits off the window's first bases (k_hist8's cheap path, k_hist16) are for
    // layouts that keep `left` in place: L = 0 sends this context through the generic generators
    const bool moved = (mS & topbits(2)) == 0 || mLf || mRt || rot;
    if (moved) { c->g.L = 0; c->g.LRrel = 0; c->g.pmask = 0; }
    c->custom_layout = moved;
    return KR_OK;
}

// kstream's column orders in general (round 6): the key = the listed pieces of the window one after the other.  What
// kr_set_field_order cannot hold -- more than three blocks, pieces out of window order (two split sizes counted from the end)
int kr_set_field_pieces(kr_ctx* c, int n, const int* offsets, const int* widths) {
    if (!c || !c->have_params || c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (!offsets || !widths || n < 1 || n > 8) return fail(c, KR_ERR_PARAM, "kr_set_field_pieces: 1 .. 8 pieces");
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_field_pieces after genomes were uploaded");
    const int k = c->g.k;
    if (c->g.D != 0 || c->g.R != 0 || c->g.L != k)
        return fail(c, KR_ERR_STATE, "kr_set_field_pieces: after kr_set_params(k, 0, 0, ...)");
    u64 seen = 0;
    int sum = 0;
    for (int i = 0; i < n; i++) {
        if (widths[i] < 1 || offsets[i] < 0 || offsets[i] + widths[i] > k) return fail(c, KR_ERR_PARAM, "kr_set_field_pieces: a piece outside the window (or empty)");
        const u64 m = ((widths[i] >= 64 ? ~0ull : ((1ull << widths[i]) - 1)) << offsets[i]);
        if (seen & m) return fail(c, KR_ERR_PARAM, "kr_set_field_pieces: pieces overlap");
        seen |= m;
        sum += widths[i];
    }
    if (sum != k) return fail(c, KR_ERR_PARAM, "kr_set_field_pieces: the pieces must cover the k = %d bases of the window", k);
    c->g.npc = n;
    for (int i = 0; i < n; i++) { c->g.pco[i] = (unsigned char)offsets[i]; c->g.pcl[i] = (unsigned char)widths[i]; }
    // (as kr_set_field_order for layouts that move `left`: L = 0 sends the context through the generic key generators)
    c->g.L = 0; c->g.LRrel = 0; c->g.pmask = 0;
    c->custom_layout = true;
    return KR_OK;
}

int kr_set_params_wide(kr_ctx* c, int L, int D, int R, int softmask_mode, size_t max_bases) {
    if (!c) return KR_ERR_PARAM;
    const int k = L + D + R;
    if (L < 1 || L > KR_WIDE_MAX_FLANK || R < 1 || R > KR_WIDE_MAX_FLANK || D < 0 || k > KR_WIDE_MAX_K)
        return fail(c, KR_ERR_PARAM, "wide path needs 1 <= L, R <= %d and L+D+R <= %d (got %d/%d/%d)", KR_WIDE_MAX_FLANK,
                    KR_WIDE_MAX_K, L, D, R);
    if (softmask_mode != KR_SOFT_MAP && softmask_mode != KR_SOFT_OMIT)
        return fail(c, KR_ERR_PARAM, "unknown softmask mode %d", softmask_mode);
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_params_wide after genomes were uploaded");
    coarse_pool_release(c);
    if (max_bases >= (1ull << 32) - 256) return fail(c, KR_ERR_PARAM, "genomes of >= 2^32 bases are not supported");
    int sb, b, rc;
    // (every sorted spectrum / composite must carry the slice digits: the shortest piece decides)
    const int shortest = std::min(std::min(L, 32), std::min(R, 32));
    // (the shortest piece of a flank longer than 32 bases: floor(len / pieces))
    const int restL = L > 32 ? L / kr_ctx::Wide::fd_pieces(L) : 32, restR = R > 32 ? R / kr_ctx::Wide::fd_pieces(R) : 32;
    if ((rc = plan_sort(c, max_bases, std::min(shortest, std::min(restL, restR)), sb, b))) return rc;
    c->sb = sb;
    c->nslices = 1 << (2 * sb);
    auto& w = c->wide;
    w.on = true;
    w.L = L; w.D = D; w.R = R; w.k = k;
    w.omit = softmask_mode == KR_SOFT_OMIT;
    w.W = (D + 15) / 16;
    w.strands = 0;
    w.nhits = -1;
    c->g = make_geom(L, 0, 0, w.omit, sb, b);    // placeholder until kr_wide_run picks a phase
    c->max_bases = max_bases;
    c->have_params = true;
    return KR_OK;
}

static int alloc_slice(kr_ctx* c, Slice& S, u64 count) {
    const u32 nb = 1u << c->g.b;
    S.nmax = count;
    S.nchunks = (u32)(count / LS_T) + 1;
    S.count = -1;
    int rc;
    if ((rc = ensure(c, S.keys, (count + 2) * 8))) return rc;
    if ((rc = ensure(c, S.off, ((size_t)nb + 2) * 4))) return rc;
    if ((rc = ensure(c, S.chunkdesc, ((size_t)S.nchunks + 2) * 16))) return rc;
    if ((rc = ensure(c, S.ovf, 16 + (size_t)OVF_MAX * 16))) return rc;
    if (S.res < 0 && (S.res = mbox_slot(c)) < 0)
        return fail(c, KR_ERR_CAPACITY, "more than %d key-space slices alive in one context", (MB_WORDS - MB_SLICE0) / 2);
    return KR_OK;
}

// per-lane scratch for sorting slices of up to `maxcount` keys from genomes of up to max_bases
// The pass-1 output buffer.  The same binary on the same box runs pass 1 and pass 2 up to 15 % faster or slower from
// one allocation of this buffer to the next (same virtual address, other physical pages:
// tools/placement_check.py).  KR_OPT_PLACE_TRIES = n > 1 (a caller that will sort many genomes with one
// context: bench.py): for a buffer of >= 256 MB n candidates are allocated, each is timed under pass 1's write
// pattern (k_probe_scatter, ~0.3 ms), the fastest is kept and the others are freed.  Over 8 processes per setting
// on two boxes (tools/ab_place.sh): 59.4-60.7 G k-mers/s as allocated, 60.0-63.1 (mean +3.3 %) with the best of 8.
// (Choosing the sorted-key arrays the same way helped on one box and hurt on the other: not done.)
static double probe_scatter_ms(kr_ctx* c, void* p, size_t bytes) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    const u64 nkeys = bytes / 8 > 64 ? bytes / 8 - 64 : 0;      // (a buffer too small for the kernel's loop is not written at all)
    hipLaunchKernelGGL(k_probe_scatter, dim3(NWG), dim3(512), 0, c->stream, (u64*)p, nkeys);      // warm-up (first touch)
    (void)hipEventRecord(e0, c->stream);
    for (int r = 0; r < 2; r++) hipLaunchKernelGGL(k_probe_scatter, dim3(NWG), dim3(512), 0, c->stream, (u64*)p, nkeys);
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float ms = -1.0f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms / 2;
}
// What a search saw: candidates probed, buffers handed out, the probe times of the four fastest, the median, the slowest.
struct PlaceStats {
    int n = 0, taken = 0;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    size_t bytes = 0;
};
// the gates of a search, for buffers of `bytes`: candidates per buffer (<= 1: the buffers are taken as allocated)
static int place_tries_for(const kr_ctx* c, size_t bytes) {
    // the search transiently holds place_tries x lanes buffers: not for a context that was given an HBM budget or that
    // shares its GPU with other ranks, unless the caller asked for it
    const int tries = (!c->place_tries_set && (c->budget || c->shared_gpu)) ? 1 : c->place_tries;
    if (tries <= 1 || bytes < c->place_min_bytes) return 1;
    // ... nor for a context that has not shown yet that it will sort many genomes (KR_OPT_LANES set, the automatic
    // switch after LANES_AFTER sorts, or KR_OPT_PLACE_TRIES set): the candidates are device memory the driver may have to clear first, 15-40 ms per GB
    // to obtain (tools/allocbench.hip) -- 7 ms of a 100 ms run over four 50 Mbp files, half a second of one over two
    // 3 Gbp genomes, for a few per cent of sort time that a one-shot run does not have
    if (!c->place_tries_set && c->nlanes == 0 && c->sorts_done < LANES_AFTER) return 1;
    return tries;
}
// The search: todo = allocated buffers of `bytes`; `tries` candidates per buffer are allocated and probed, the fastest go to
// todo (in order: todo[0] the fastest, its time in ms_out[0]), the rest is freed.
static void place_search(kr_ctx* c, const std::vector<DevBuf*>& todo, size_t bytes, int tries, PlaceStats& ps,
                         std::vector<double>* ms_out = nullptr) {
    static const bool trace = getenv("KR_TRACE_ALLOC") != nullptr;
    struct Cand { DevBuf buf; double ms; };
    std::vector<Cand> pool;            // (candidates stay allocated until the choice is made: a freed one would come back)
    for (DevBuf* b : todo) {
        pool.push_back({*b, probe_scatter_ms(c, b->p, b->bytes)});
        *b = DevBuf();
    }
    // place_tries candidates per buffer; when fewer candidates than buffers are near the best probe seen -- the fast class
    // is scarce at times: 1 of 48 in one process, 9 of 48 in the next on the same box, and a lane in the slow class costs
    // 5-8 % of the step -- the search goes on, up to four times as far and a third of the device's free memory
    const size_t want = (size_t)tries * todo.size();
    // the extended search (beyond `want`) only for a context that sorts many genomes (several lanes: asked for, or the
    // automatic switch after LANES_AFTER sorts); the whole pool within 48 GB (or the `want` candidates when they are more)
    const bool extended = lanes_used(c) > 1;
    const size_t pool_cap = std::max<size_t>(want, ((size_t)48 << 30) / bytes);
    size_t fr0 = 0, tot0 = 0;
    (void)hipMemGetInfo(&fr0, &tot0);
    auto near_best = [&]() {
        double best = 1e30;
        for (const Cand& k : pool) if (k.ms > 0 && k.ms < best) best = k.ms;
        size_t n = 0;
        for (const Cand& k : pool) n += k.ms > 0 && k.ms <= best * 1.04;
        return n;
    };
    while (pool.size() < std::min(want, pool_cap) ||
           (extended && pool.size() < std::min(4 * want, pool_cap) && near_best() < todo.size())) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < 2 * bytes + ((size_t)4 << 30)) break;
        if (pool.size() >= want && fr0 && fr < fr0 - fr0 / 3) break;
        if (c->budget && c->used + bytes > c->budget) break;
        DevBuf cand;
        if (ensure(c, cand, bytes)) break;
        pool.push_back({cand, probe_scatter_ms(c, cand.p, cand.bytes)});
    }
    if (trace)
        for (const Cand& k : pool) fprintf(stderr, "[krisp_hip] pass-1 buffer %p: probe %.3f ms\n", k.buf.p, k.ms);
    // (a failed probe, ms <= 0, sorts last)
    std::stable_sort(pool.begin(), pool.end(), [](const Cand& a, const Cand& b2) {
        return (a.ms > 0 ? a.ms : 1e30) < (b2.ms > 0 ? b2.ms : 1e30);
    });
    ps.n = (int)pool.size();
    ps.taken = (int)todo.size();
    for (int i = 0; i < 4; i++) ps.ms[i] = (size_t)i < pool.size() ? pool[i].ms : 0.0;
    ps.ms[4] = pool.empty() ? 0.0 : pool[pool.size() / 2].ms;
    ps.ms[5] = pool.empty() ? 0.0 : pool.back().ms;
    ps.bytes = bytes;
    for (size_t i = 0; i < pool.size(); i++) {
        if (i < todo.size()) {
            *todo[i] = pool[i].buf;
            if (ms_out) ms_out->push_back(pool[i].ms);
        } else release(c, pool[i].buf);
    }
}
// bufs = the pass-1 output buffers of the lanes that need (more) room: ONE pool of place_tries candidates per buffer
// is allocated and probed, the fastest go to the lanes, the rest is freed -- a lane-by-lane search sees the pages the
// lane before it gave back, and the probe classes (0.19 / 0.22 / 0.255 ms for 800 MB) come in streaks: three lanes
// with 8 candidates each ended at 0.22 / 0.19 / 0.22, a pool of 24 gives every lane one of the best.
static int ensure_placed(kr_ctx* c, DevBuf* const* bufs, int nbuf, size_t bytes) {
    std::vector<DevBuf*> todo;
    for (int i = 0; i < nbuf; i++)
        if (bufs[i]->bytes < bytes) todo.push_back(bufs[i]);
    if (todo.empty()) return KR_OK;
    int rc;
    for (DevBuf* b : todo)
        if ((rc = ensure(c, *b, bytes))) return rc;
    const int tries = place_tries_for(c, bytes);
    if (tries <= 1) return KR_OK;
    // (what the search saw, for kr_debug_place: bench.py prints it, so that a line says which placement class it ran in)
    PlaceStats ps;
    place_search(c, todo, bytes, tries, ps);
    c->place_n = ps.n;
    c->place_taken = ps.taken;
    for (int i = 0; i < 6; i++) c->place_ms[i] = ps.ms[i];
    c->place_bytes = ps.bytes;
    return KR_OK;
}

// The pool grows: one search for `want` more buffers (intersect_coarse calls this behind its closing synchronisation, for the
// coarse genomes of a call that hold no pooled buffer and have been partitioned at least twice -- a run that partitions each
// genome once never comes here).  The gates are ensure_placed's; the statistics are the pool's own (kr_debug_coarse_pool):
// c->place_* go on describing the lanes' buffers.  A device without room for a buffer ends the growth, not the call.
static void coarse_pool_grow(kr_ctx* c, int want) {
    const size_t bytes = ((size_t)c->lane_maxcount + 2) * 8;
    if (want <= 0 || !c->coarse_pool || !c->lane_maxcount) return;
    coarse_pool_purge(c, bytes);
    want -= (int)c->cpool_free.size();
    if (want <= 0) return;
    const int tries = place_tries_for(c, bytes);
    if (tries <= 1) return;
    std::vector<DevBuf> fresh((size_t)want);
    std::vector<DevBuf*> todo;
    for (DevBuf& b : fresh) {
        if (ensure(c, b, bytes)) break;
        todo.push_back(&b);
    }
    c->err.clear();
    if (todo.empty()) return;
    PlaceStats ps;
    std::vector<double> ms;
    place_search(c, todo, bytes, tries, ps, &ms);
    c->err.clear();        // (a candidate the device had no room for ended the search: not an error of the call)
    c->cpool_searches++;
    for (size_t i = 0; i < todo.size(); i++) {
        if (!todo[i]->p) continue;
        c->cpool_free.push_back({*todo[i], ms[i] > 0 ? ms[i] : 1e30, nullptr, false});      // (a failed probe sorts last)
        c->cpool_total++;
    }
    std::stable_sort(c->cpool_free.begin(), c->cpool_free.end(),
                     [](const kr_ctx::PoolBuf& a, const kr_ctx::PoolBuf& b2) { return a.ms < b2.ms; });
}

static int ensure_lanes(kr_ctx* c, u64 maxcount) {
    const u32 nb = 1u << c->g.b;
    const u64 mw = (c->max_bases + 31) / 32 + PAD_WORDS + 2;
    const u64 ntmax = maxcount / P2_TILE + 260;
    int rc;
    c->lane_maxcount = std::max(c->lane_maxcount, maxcount);
    maxcount = c->lane_maxcount;
    c->lanes_ready = lanes_used(c);
    for (int i = 0; i < lanes_used(c); i++) {
        Lane& ln = c->lanes[i];
        if ((rc = lane_open(c, ln))) return rc;
        if ((rc = ensure(c, ln.codes, mw * 8))) return rc;
        if ((rc = ensure(c, ln.bad, mw * 4))) return rc;
        if ((rc = ensure(c, ln.partial8, (size_t)NWG * 256 * 4))) return rc;
        if ((rc = ensure(c, ln.base1, (260 + 256) * 4))) return rc;     // bases[257] | column totals[256]
        if ((rc = ensure(c, ln.tp, 260 * 4))) return rc;
        if ((rc = ensure(c, ln.base64, 260 * 8))) return rc;
        if ((rc = ensure(c, ln.tiledesc, ntmax * 8))) return rc;
        if ((rc = ensure(c, ln.tilehist, ntmax * (nb >> 8) * 4))) return rc;
        if (USE_HIST16 && nb > 256) {
            if ((rc = ensure(c, ln.partial16, (size_t)H16_RANGES * nb * 2 + 64))) return rc;
            if ((rc = ensure_h16exc(c, ln, ln.stream))) return rc;
            if ((rc = ensure(c, ln.cursor, ((size_t)nb + 4) * 4))) return rc;
        }
    }
    DevBuf* tk[MAX_LANES];
    for (int i = 0; i < lanes_used(c); i++) tk[i] = &c->lanes[i].tmpkeys;
    return ensure_placed(c, tk, lanes_used(c), (maxcount + 2) * 8);
}

static void launch_pack(kr_ctx* c, Genome& G, Lane& ln, hipStream_t st) {
    const u64 nwp = G.nwords + PAD_WORDS;   // pad words (all bad): a window may read past the last base
    u32 grid = (u32)std::min<u64>((nwp + 255) / 256, 4096);
    hipLaunchKernelGGL(k_pack, dim3(grid), dim3(256), 0, st, (const uint8_t*)G.bases.p, (u64)G.n_bases,
                       (u64*)ln.codes.p, (u32*)ln.bad.p, nwp, c->g.omit, c->g.allow);
}

// dst_keys = keys the destination array holds (it has two more of slack).  The wide path's key
// generator reads dictionaries and caches from global memory inside the tile (data-dependent
// loads): it keeps the first form of the kernel; packed windows take the pipelined one -- BIG
// for the pass 0 of sliced genomes, whose output can exceed what a buffer descriptor spans.
static bool p1_fast_on() {
    static const bool on = [] { const char* e = getenv("KR_P1_FAST"); return e ? atoi(e) != 0 : true; }();
    return on;
}
static bool p1_fast_form(const Geom& g) {
    return p1_fast_on() && g.wmode == 0 && g.strands == 0 && g.rot == 0 && g.npc == 0 && (u32)((g.mR | g.mD) >> 32) == 0u;
}
// `one`: the forward record of every window only, by co_strand.inc's digit (a coarse genome, SortPlan.one)
static void launch_scatter1(const Geom& g, hipStream_t st, const u64* codes, const u32* bad, u64 nwords,
                            const u32* base1, const u64* base64, const u32* rowoff, u64* dst, u64 dst_keys, bool one = false) {
    const bool big = base64 != nullptr;
    // both strands, no rotation, the fields that move inside the low word: the generator that shifts the word string once
    // per thread (p1_fast_keys; KR_P1_FAST=0: the general one, A/B and tests)
    const bool fast = p1_fast_form(g);
    if (one) {
        hipLaunchKernelGGL((k_scatter1p<0, 0, 1, 1>), dim3(NWG), dim3(P1_T), 0, st, codes, bad, nwords, base1, base64, rowoff, dst, dst_keys, g);
    } else if (g.wmode && g.wmode != 1 && g.wcmode == 4) {
        hipLaunchKernelGGL(k_scatter1l, dim3(NWG), dim3(P1_T), 0, st, base1, base64, rowoff, dst, g);
    } else if (g.wmode) {
        const auto kw = g.wmode == 1 ? k_scatter1w<1> : g.wcmode == 2 ? k_scatter1w<3> : k_scatter1w<2>;
        hipLaunchKernelGGL(kw, dim3(NWG), dim3(P1_T), 0, st, codes, bad, nwords, base1, base64, rowoff, dst, g);
    } else {
        const auto kp = fast ? (big ? k_scatter1p<0, 1, 1> : k_scatter1p<0, 0, 1>)
                             : g.strands ? (big ? k_scatter1p<2, 1> : k_scatter1p<2, 0>) : (big ? k_scatter1p<0, 1> : k_scatter1p<0, 0>);
        hipLaunchKernelGGL(kp, dim3(NWG), dim3(P1_T), 0, st, codes, bad, nwords, base1, base64, rowoff, dst, dst_keys, g);
    }
}

// pass 2: tiles of 2 * P2_TILE keys, one per workgroup of 2 * P2_T threads (512-byte runs at fan-out
// 2^16); a persistent, prefetching form of the same kernel was 7 % slower (k_sort2.inc header)
static void launch_scatter2(hipStream_t st, const u64* src, u64* dst, const uint2* tiledesc, u32 ntmax,
                            const u32* tilehist, u32* cursor, int b, int shl = 0, u32 region_n = 0) {
    hipLaunchKernelGGL(k_scatter2<2 * P2_T>, dim3(ntmax), dim3(2 * P2_T), 0, st, src, dst, tiledesc, tilehist, cursor, b, shl, region_n);
}

static void launch_hist8(kr_ctx* c, Genome& G, Lane& ln, hipStream_t st, const Geom& g, bool one = false) {
    const auto kh = one ? k_hist8<3> : g.wmode == 1 ? k_hist8w<1> : g.wmode ? (g.wcmode == 2 ? k_hist8w<3> : k_hist8w<2>) : g.strands ? k_hist8<2> : k_hist8<0>;
    hipLaunchKernelGGL(kh, dim3(NWG), dim3(P1_T), 0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p, G.nwords,
                       (u32*)ln.partial8.p, g);
}

// the pass-2 tile: 16 keys per thread; 1024-thread workgroups (16384-key tiles, one per CU) keep a tile's runs at 512 bytes
// for fan-out 2^16 and 256 / 128 bytes for 2^17 / 2^18.  p2_tiles: the tiles of a slice of nmax keys at most, whose 256
// top-byte buckets each end in a tile of their own
static constexpr u32 P2_KEYS = 2 * P2_TILE;
static u32 p2_tiles(u64 nmax) { return (u32)(nmax / P2_KEYS) + 257; }

// the lane the next sort takes: count_slices looks at it, take_lane takes it -- the same one (genome_sort(., reuse_count)
// finds count_slices' codes, bad bits and reduced histogram in its scratch)
static Lane& peek_lane(kr_ctx* c) {
    if (c->next_lane >= lanes_used(c)) c->next_lane = 0;
    return c->lanes[c->next_lane];
}

// the context's geometry without slices: what pass 0, and the count in front of it, see of a key.  counting: the wide
// path's cached composite keys are WRITTEN by this histogram (as a list, Geom.wlcnt, or 16 bytes per window start)
static Geom pass0_geom(const kr_ctx* c, bool counting = false) {
    Geom g0 = c->g;
    g0.sbits = 0;
    g0.slice = 0;
    if (counting && g0.wmode == 2 && g0.wcache) g0.wcmode = g0.wlcnt ? 3 : 1;
    return g0;
}

// exact key count of every slice under the current geometry (sizes the slice arrays):
// pack + top-byte histogram on the main stream
static int count_slices(kr_ctx* c, Genome& G) {
    int rc;
    if ((rc = ensure_lanes(c, 16))) return rc;
    // the lane the genome's sort will take (genome_sort, right behind this call, finds the counts and the packed
    // codes in its scratch)
    Lane& ln = peek_lane(c);
    hipStream_t st = ln.stream;
    ln.pending = true;
    if (G.up_done && st != c->stream) HIPCHK(c, hipStreamWaitEvent(st, G.up_done, 0));
    launch_pack(c, G, ln, st);
    reset_slices(c, G);
    std::vector<u32> tot(256);
    u64 maxcount = 0;
    G.nmax = 0;
    genome_unsorted(G);
    coarse_pool_return(c, G);
    // ONE histogram of the top byte of the absolute keys: a slice is 2^(8 - sbits) of its buckets
    const Geom g0 = pass0_geom(c, true);
    {
        StageScope sc(c, KR_ST_HIST8, st);
        launch_hist8(c, G, ln, st, g0);
    }
    hipLaunchKernelGGL(k_reduce8a, dim3(256), dim3(256), 0, st, (u32*)ln.partial8.p, (u32*)ln.base1.p + 260);
    HIPCHK(c, hipMemcpyAsync(tot.data(), (u32*)ln.base1.p + 260, 256 * 4, hipMemcpyDeviceToHost, st));
    std::vector<u32> seglen;
    if (g0.wcmode == 3) {
        seglen.resize(NWG);
        HIPCHK(c, hipMemcpyAsync(seglen.data(), g0.wlcnt, NWG * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    if (g0.wcmode == 3) {
        u64 listed = 0;
        for (u32 v : seglen) {
            if (v > g0.wlcap) return KR_RETRY_DENSE;      // (a segment too short for its workgroup's keys: phase_sort_intersect takes the dense form)
            listed += v;
        }
        c->wide.keys_listed += listed;
    }
    const int per = 256 >> c->g.sbits;          // buckets per slice
    for (int s = 0; s < c->nslices; s++) {
        u64 cnt = 0;
        for (int d = s * per; d < (s + 1) * per; d++) cnt += tot[d];
        if (cnt >= KR_MAX_SLICE_KEYS)
            return fail(c, KR_ERR_CAPACITY, "slice %d of genome %d holds %llu keys (the limit is %llu, the 4 GiB a buffer "
                        "descriptor spans): raise KR_SLICE_BASES", s, G.id, (unsigned long long)cnt,
                        (unsigned long long)KR_MAX_SLICE_KEYS);
        if ((rc = alloc_slice(c, G.sl[s], cnt))) return rc;
        G.nmax += cnt;
        maxcount = std::max(maxcount, cnt);
    }
    if (c->nslices > 1 && (rc = ensure(c, ln.pass0, (G.nmax + 2) * 8))) return rc;      // (another lane makes its own when it first sorts a genome)
    HIPCHK(c, hipGetLastError());
    return ensure_lanes(c, maxcount);
}

// is `p` inside a pinned block of kr_ingest_file? (h_ingest.inc)
static bool host_is_pinned(const void* p, int device);

static int upload_finish(kr_ctx* c, Genome& G, int id, size_t n);

int kr_genome_upload(kr_ctx* c, int id, const uint8_t* bases, size_t n) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (n > c->max_bases) return fail(c, KR_ERR_PARAM, "genome of %zu bases exceeds max_bases %zu", n, c->max_bases);
    HIPCHK(c, hipSetDevice(c->device));
    const auto seen = c->genomes.find(id);
    const bool known = seen != c->genomes.end() && (seen->second.uploaded || seen->second.n_bases);     // (kr_reserve makes entries that were never uploaded)
    if (known) HIPCHK(c, hipDeviceSynchronize());     // re-upload under an id whose sort may still be running
    Genome& G = c->genomes[id];
    G.id = id;
    G.n_bases = n;
    G.nwords = (n + 31) / 32;
    genome_unsorted(G);
    coarse_pool_return(c, G);
    int rc;
    if ((rc = ensure(c, G.bases, n + 64))) return rc;
    if (!G.up_done) HIPCHK(c, hipEventCreateWithFlags(&G.up_done, hipEventDisableTiming));
    // no device-wide synchronisation: a pinned source (kr_ingest_file) is copied by DMA on the
    // copy stream while earlier genomes are being sorted; the context's stream (and any sort lane,
    // genome_sort) waits for the copy on the device, not the host
    hipStream_t cs = host_is_pinned(bases, c->device) ? c->copy_stream : c->stream;
    if (n) HIPCHK(c, hipMemcpyAsync(G.bases.p, bases, n, hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipEventRecord(G.up_done, cs));
    if (cs != c->stream) HIPCHK(c, hipStreamWaitEvent(c->stream, G.up_done, 0));
    return upload_finish(c, G, id, n);
}

// the genome's bookkeeping once its n bases are (being copied) on the device: slice plan, sort scratch
static int upload_finish(kr_ctx* c, Genome& G, int id, size_t n) {
    int rc;
    if (c->wide.on || c->loc.on) {   // the slices are counted per phase by kr_wide_run; a locate context sorts nothing
        G.uploaded = true;
        return KR_OK;
    }
    if (c->nslices == 1) {
        // one sort unit: its arrays are sized by the bound 2 n (exact unless the genome holds N /
        // soft-masked windows); no counting pass, no device -> host copy, no wait
        reset_slices(c, G);
        const u64 bound = 2 * (u64)n;
        if (bound >= KR_MAX_SLICE_KEYS)
            return fail(c, KR_ERR_CAPACITY, "genome %d: %llu keys in one sort unit (the limit is %llu)", id,
                        (unsigned long long)bound, (unsigned long long)KR_MAX_SLICE_KEYS);
        if ((rc = alloc_slice(c, G.sl[0], bound))) return rc;
        G.nmax = bound;
        if ((rc = ensure_lanes(c, bound))) return rc;
    } else if ((rc = count_slices(c, G))) {
        return rc;
    }
    G.uploaded = true;
    return KR_OK;
}

// lanes the slices of ONE genome take turns on: its own and a helper (KR_OPT_LANES = 1 keeps one: every kernel alone on
// the device); the helper of genome lane i is lane SLICE_HELPER + i
#define SLICE_HELPER 2
#define SLICE_HELPERS 2         // helper lanes per genome lane: the slices take turns on 1 + SLICE_HELPERS streams
static inline int slice_lanes(const kr_ctx* c) { return c->nlanes == 1 ? 1 : 1 + SLICE_HELPERS; }

// scratch of a helper lane: what a slice's pass 1, pass 2 and chunk table write
static int ensure_slice_lanes(kr_ctx* c, int helper) {
    const u32 nb = 1u << c->g.b;
    const u64 maxcount = c->lane_maxcount;
    const u64 ntmax = maxcount / P2_TILE + 260;
    int rc;
    Lane& ln = c->lanes[helper];
    if ((rc = lane_open(c, ln))) return rc;
    if ((rc = ensure(c, ln.base1, (260 + 256) * 4))) return rc;
    if ((rc = ensure(c, ln.tp, 260 * 4))) return rc;
    if ((rc = ensure(c, ln.slt, 1024 * 4))) return rc;
    if ((rc = ensure(c, ln.tiledesc, ntmax * 8))) return rc;
    if ((rc = ensure(c, ln.tilehist, ntmax * (nb >> 8) * 4))) return rc;
    return ensure(c, ln.tmpkeys, (maxcount + 2) * 8);
}

// The large buffers of `n` genomes of up to n_bases bases (or bytes of file text), made AHEAD of the uploads -- while host
// threads still read and inflate the files.  Device memory that another process has just given back costs 15-40 ms per GB
// to obtain on these boxes (the driver clears it: tools/allocbench.hip, 4 x 48 GB in 1 ms on a clean box, 3.7 s behind another process): the 250 GB two 3 Gbp genomes take come to 3-5 s, as long as the
// inflate of their files.  Nothing depends on this call: what it does not make, or makes too small (the slices of a
// skewed genome), the uploads and sorts make or grow as before.
int kr_reserve(kr_ctx* c, const int* ids, int n, size_t n_bases, int with_text) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (n < 0 || (n && !ids)) return fail(c, KR_ERR_PARAM, "kr_reserve: bad argument");
    if (n_bases > c->max_bases) return fail(c, KR_ERR_PARAM, "kr_reserve: %zu bases exceed max_bases %zu", n_bases, c->max_bases);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const u64 bound = 2 * (u64)n_bases;
    const u64 per_slice = c->nslices > 1 ? bound / (u64)c->nslices + bound / (u64)c->nslices / 50 + 4096 : bound;
    if (with_text && (rc = ensure(c, c->tx_text, n_bases + 64))) return rc;      // (kr_genome_upload_text's copy of the file)
    for (int i = 0; i < n; i++) {
        Genome& G = c->genomes[ids[i]];
        G.id = ids[i];
        if ((rc = ensure(c, G.bases, n_bases + 64))) return rc;
        if (c->wide.on || c->g.wmode) continue;
        reset_slices(c, G);
        if (per_slice >= KR_MAX_SLICE_KEYS) continue;           // (the upload will say so)
        for (Slice& S : G.sl)
            if ((rc = ensure(c, S.keys, (per_slice + 2) * 8))) return rc;
    }
    if (c->wide.on || c->g.wmode || !n || per_slice >= KR_MAX_SLICE_KEYS) return KR_OK;
    if ((rc = ensure_lanes(c, per_slice))) return rc;
    if (c->nslices > 1)
        for (int l = 0; l < std::min(n, lanes_used(c)); l++)
            if ((rc = ensure(c, c->lanes[l].pass0, (bound + 2) * 8))) return rc;
    return KR_OK;
}

static int genome_sort(kr_ctx* c, int id, bool reuse_count, bool coarse = false);
int kr_genome_sort(kr_ctx* c, int id) { return genome_sort(c, id, false); }

// The sort up to pass 1 only (pack, top-byte histogram, its reduction, k_scatter1p -- on a sort lane, as a sort): what a
// genome needs to answer a short candidate list (k_coarse.inc).  For the contexts the coarse route of kr_intersect takes:
// packed windows of both strands, one sort unit, the standard field order, more than 256 fine buckets; any other
// context, or KR_OPT_COARSE_REST = 0: kr_genome_sort.
static bool coarse_eligible(const kr_ctx* c) {
    return c->coarse_rest && c->have_params && !c->wide.on && c->g.wmode == 0 && c->g.strands == 0 && !c->custom_layout &&
           c->nslices == 1 && c->g.b > 8;
}
int kr_genome_partition(kr_ctx* c, int id) {
    if (!c) return KR_ERR_PARAM;
    return genome_sort(c, id, false, coarse_eligible(c));
}

// What one sort does: decided once (sort_plan), read by every pass.
struct SortPlan {
    bool reuse_count;   // count_slices(G) has just run on this lane (single lane): the codes, the bad bits and the workgroup
                        // histograms of the absolute top byte (already prefix-summed by k_reduce8a) are still in the lane's scratch
    bool coarse;        // kr_genome_partition on an eligible context: the sort stops behind pass 1
    bool one;           // ... and pass 1 writes the forward record of every window only (one_strand_form)
    bool lazy;          // ... or at the fine buckets: no LDS sort
    bool sliced, route2, fine16;
    bool cached_keys;   // the wide path's composite keys are read back from the genome's cache
    int cached_mode;    // ... (the key list, Geom.wlcnt, or 16 bytes per window start)
    int nba;            // absolute top bits: (slice, top byte of the relative key)
    u32 h16_ranges;
    int nsl, helper;    // lanes the genome's slices take turns on: the genome's own, and nsl - 1 from lane `helper` on
};

// A coarse genome's forward strand answers for both (co_strand.inc, k_coarse.inc) where the context is coarse_eligible and:
// one diagnostic column; pass 1's FAST key path (`left` fills the key's high word); L >= 5 -- the digit's four positions
// lie in `left` --; R < L -- so does window position R.  KR_OPT_COARSE_ONE_STRAND = 0: never.
static bool one_strand_form(const kr_ctx* c) {
    return c->coarse_one && c->g.D == 1 && p1_fast_form(c->g) && c->g.L >= 5 && c->g.R < c->g.L && c->g.sbits == 0;
}

static SortPlan sort_plan(const kr_ctx* c, const Genome& G, const Lane& ln, bool reuse_count, bool coarse) {
    SortPlan p{};
    p.reuse_count = reuse_count;
    p.coarse = coarse;
    p.one = coarse && !reuse_count && one_strand_form(c);
    p.cached_keys = reuse_count && c->g.wmode == 2 && c->g.wcache;
    p.cached_mode = c->g.wlcnt ? 4 : 2;
    p.sliced = c->nslices > 1;
    // KR_OPT_LAZY_ORDER: keys of both strands -- the packed path's (left,right,diag) keys, the wide path's spectra and
    // composite keys: what kr_intersect / kr_collect work on -- stop at the fine buckets; single-strand and custom-layout
    // (kstream) sorts are read in order right away and end with the LDS sort as before.  KR_LAZY_WIDE=0: the wide path eager (A/B)
    static const bool lazy_wide = [] { const char* e = getenv("KR_LAZY_WIDE"); return e ? atoi(e) != 0 : true; }();
    p.lazy = c->lazy_order && (lazy_wide || (!c->wide.on && c->g.wmode == 0)) && !c->custom_layout && c->g.strands == 0 &&
             !c->order_wanted && !(G.was_anchor && !c->i3_last_ua);       // (an anchor the fused kernel takes needs no order either)
    // sliced, packed windows of both strands whose top 8 + 2 sb bits lie inside `left`: every slice's pass 1 is a
    // k_scatter2 over its pass-0 buckets, counted from the codes once per genome (k_sort.inc, "Round 4"); else (the wide
    // path's generators, single-strand modes, KR_SLICE_ROUTE=0) a slice counts its top byte per workgroup (k_hist8k)
    // and scatters with private cursors (k_scatter1kp)
    p.nba = 8 + c->g.sbits;
    p.route2 = p.sliced && USE_HIST16 && c->slice_route && c->g.wmode == 0 && c->g.strands == 0 && 2 * c->g.L >= p.nba && p.nba <= 16;
    // k_hist16's ranges: 16-bit counters need < 65536 keys per (range, top byte); 256 .. NWG ranges
    p.h16_ranges = H16_RANGES;
    if (p.route2)
        while (p.h16_ranges < NWG && G.nmax / ((u64)p.h16_ranges * 256) > 30000) p.h16_ranges *= 2;
    // fine offsets straight from the codes when the top b bits of a key lie inside `left`
    p.fine16 = USE_HIST16 && c->g.b > 8 && !p.sliced && c->g.wmode == 0 && c->g.strands == 0 && 2 * c->g.L >= c->g.b;
    // Round 4: the slices of a genome take turns on up to three lanes (their own stream and pass-1 / pass-2 scratch; the
    // pass-0 array, the codes and the (slice, top byte) offsets are the genome's and only read), so the kernels of
    // consecutive slices overlap on the device as the sorts of consecutive genomes do in the unsliced case.
    p.nsl = p.route2 ? slice_lanes(c) : 1;
    p.helper = SLICE_HELPER + SLICE_HELPERS * (int)(&ln - c->lanes);
    return p;
}

// The sort's lane: more lanes first when the automatic count has grown, then the next in turn, marked busy and ordered
// behind the genome's upload.
static int take_lane(kr_ctx* c, Genome& G, Lane*& taken) {
    if (lanes_used(c) > c->lanes_ready) {         // (automatic lanes: the context has sorted enough genomes for more than one)
        int rcl = ensure_lanes(c, c->lane_maxcount);
        if (rcl && c->nlanes == 0) {
            // no room for the scratch of more lanes (HBM budget, a nearly full device): one lane it stays
            release_lanes(c, 1);
            c->nlanes = 1;
            c->lanes_ready = 1;
            c->next_lane = 0;
            c->err.clear();
            rcl = KR_OK;
        }
        if (rcl) return rcl;
    }
    Lane& ln = peek_lane(c);
    c->last_lane = c->next_lane;
    c->next_lane = (c->next_lane + 1) % lanes_used(c);
    ln.pending = true;
    hipStream_t st = ln.stream;
    if (G.up_done && st != c->stream) HIPCHK(c, hipStreamWaitEvent(st, G.up_done, 0));
    taken = &ln;
    return KR_OK;
}

// The pool of placed pass-1 targets at the head of a sort: a buffer this sort cannot write goes back, a coarse sort
// without one takes the fastest free one.
static void coarse_pool_step(kr_ctx* c, Genome& G, bool coarse) {
    const size_t cbytes = ((size_t)c->lane_maxcount + 2) * 8;       // (a pooled buffer has the size of a lane's tmpkeys)
    if (G.ckeys.p && (!coarse || !c->coarse_pool || G.ckeys.bytes < cbytes)) coarse_pool_return(c, G);
    if (coarse) {
        G.partitions++;
        if (c->coarse_pool && !G.ckeys.p) (void)coarse_pool_take(c, G, cbytes);
    }
}

static void pass_pack(kr_ctx* c, Genome& G, Lane& ln) {
    StageScope sc(c, KR_ST_PACK, ln.stream);
    launch_pack(c, G, ln, ln.stream);
}

// Pass 0 of a sliced genome: all its keys, generated once, partitioned by their top byte; slice s is the contiguous
// run of its 2^(8 - sbits) buckets.  route2: also the (slice, top byte) bins every slice's pass 1 will scatter by.
static int pass0(kr_ctx* c, Genome& G, const SortPlan& p, Lane& ln) {
    hipStream_t st = ln.stream;
    int rc;
    // the slices of the genome this lane sorted before may still run on its helper lane, out of this lane's arrays
    for (int h = 0; h < SLICE_HELPERS; h++) {
        Lane& hp = c->lanes[p.helper + h];
        if (hp.stream && hp.pending) {
            HIPCHK(c, hipEventRecord(hp.done, hp.stream));
            HIPCHK(c, hipStreamWaitEvent(st, hp.done, 0));
        }
    }
    if (p.route2) {
        if ((rc = ensure(c, ln.partial16, ((size_t)p.h16_ranges << p.nba) * 2 + 64))) return rc;
        if ((rc = ensure_h16exc(c, ln, st))) return rc;
        if ((rc = ensure(c, ln.slt, 1024 * 4))) return rc;
        if ((rc = ensure(c, ln.offa, (((size_t)1 << p.nba) + 4) * 4))) return rc;
        if ((rc = ensure(c, ln.cura, (((size_t)1 << p.nba) + 4) * 4))) return rc;
    }
    if (!p.reuse_count) pass_pack(c, G, ln);
    if ((rc = ensure(c, ln.pass0, (G.nmax + 2) * 8))) return rc;
    if (!p.reuse_count) {
        StageScope sc(c, KR_ST_HIST8, st);
        launch_hist8(c, G, ln, st, pass0_geom(c, true));
    }
    {
        StageScope sc(c, KR_ST_REDUCE8, st);
        if (!p.reuse_count)
            hipLaunchKernelGGL(k_reduce8a, dim3(256), dim3(256), 0, st, (u32*)ln.partial8.p, (u32*)ln.base1.p + 260);
        hipLaunchKernelGGL(k_bases64, dim3(1), dim3(64), 0, st, (const u32*)ln.base1.p + 260, (u64*)ln.base64.p);
    }
    Geom g0 = pass0_geom(c);
    g0.wcmode = (g0.wmode == 2 && g0.wcache) ? p.cached_mode : 0;
    g0.slice = (u32)c->g.sbits;          // (P0_DIGIT_BITS of k_scatter1p<., 1>: pass 0 partitions by the slice alone)
    {
        StageScope sc(c, KR_ST_SCATTER1, st);
        launch_scatter1(g0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p, G.nwords, (const u32*)nullptr,
                        (const u64*)ln.base64.p, (const u32*)ln.partial8.p, (u64*)ln.pass0.p, G.nmax);
    }
    if (!p.route2) return KR_OK;
    // the (slice, top byte) bins of the whole genome from the codes: offsets relative to each slice's start
    {
        StageScope sc(c, KR_ST_HIST2, st);
        hipLaunchKernelGGL(k_hist16, dim3(p.h16_ranges, 1), dim3(H16_T), 0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p,
                           G.nwords, (const u32*)ln.partial8.p, (const u32*)ln.base1.p + 260,
                           (unsigned short*)ln.partial16.p, (u32*)ln.h16exc.p, c->g.k, p.nba);
    }
    StageScope sc(c, KR_ST_SCAN2, st);
    hipLaunchKernelGGL(k_bases_rel, dim3(1), dim3(256), 0, st, (const u32*)ln.base1.p + 260, 256u >> c->g.sbits,
                       (u32*)ln.slt.p);
    hipLaunchKernelGGL(k_hist16_off, dim3(256), dim3(1024), 0, st, (const unsigned short*)ln.partial16.p, p.h16_ranges,
                       p.nba, (const u32*)ln.h16exc.p, (const u32*)ln.slt.p, (u32*)ln.offa.p, (u32*)ln.cura.p);
    return KR_OK;
}

// The slices go to their lanes: pass 0 and the offsets are behind `slice_ready`, the helper lanes (made here when they
// are first needed) wait for it.
static int slice_lanes_start(kr_ctx* c, const SortPlan& p, Lane& ln) {
    int rcs;
    hipStream_t st = ln.stream;
    hipEvent_t& ready = c->slice_ready[(int)(&ln - c->lanes)];
    if (!ready) HIPCHK(c, hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(ready, st));
    for (int h = p.helper; h < p.helper + SLICE_HELPERS; h++) {
        if ((rcs = ensure_slice_lanes(c, h))) return rcs;
        HIPCHK(c, hipStreamWaitEvent(c->lanes[h].stream, ready, 0));
        c->lanes[h].pending = true;
    }
    return KR_OK;
}

// Where a slice's pass 1 writes: the lane's scratch when a pass 2 follows, else the slice's keys -- or, for a coarse genome
// that holds one, its placed buffer of the pool, whose last owner's kernels may still be at it on another stream.
static int pass1_target(kr_ctx* c, Genome& G, const SortPlan& p, Lane& ls, Slice& S, u64*& pass1_dst) {
    hipStream_t ss = ls.stream;
    pass1_dst = (c->g.b > 8 && !p.coarse) ? (u64*)ls.tmpkeys.p : (u64*)S.keys.p;
    if (!p.coarse || !G.ckeys.p) return KR_OK;
    pass1_dst = (u64*)G.ckeys.p;
    if (G.ckeys_busy && G.ckeys_busy != ss) coarse_pool_handover(c, G);      // (its own last pass 1, on another lane)
    if (G.ckeys_wait) {
        HIPCHK(c, hipStreamWaitEvent(ss, G.ckeys_ev, 0));
        G.ckeys_wait = false;
    }
    G.ckeys_busy = ss;
    c->cpool_partitions++;
    return KR_OK;
}

// Pass 1 of slice s, route2: a k_scatter2 over the slice's pass-0 buckets by the bins pass0() counted.
// (ln: the genome's lane, whose scratch holds what belongs to the genome; ls: the slice's lane and stream)
static void pass1_route2(kr_ctx* c, const SortPlan& p, Lane& ln, Lane& ls, Slice& S, int s, const u64* src, u64* pass1_dst) {
    hipStream_t ss = ls.stream;
    const int b = c->g.b;
    const u32 ntA = (u32)((S.nmax + P2_KEYS - 1) / P2_KEYS);
    if (ntA) {
        StageScope sc(c, KR_ST_SCATTER1, ss);
        launch_scatter2(ss, src, pass1_dst, (const uint2*)nullptr, ntA, (const u32*)nullptr, (u32*)ln.cura.p, p.nba, c->g.sbits,
                        (u32)S.nmax);
    }
    StageScope sc(c, KR_ST_REDUCE8, ss);
    const u32 ntmax = b > 8 ? p2_tiles(S.nmax) : 0u;
    hipLaunchKernelGGL(k_reduce8b, dim3(std::max(1u, (ntmax + 255) / 256)), dim3(256), 0, ss, (const u32*)nullptr,
                       (u32*)ls.base1.p, (u32*)ls.tp.p, b > 8 ? P2_KEYS : 0u, ntmax, (uint2*)ls.tiledesc.p,
                       (const u32*)ln.offa.p + (size_t)s * 256, (u32)S.nmax);
}

// Pass 1 of slice s, counted: the top byte's histogram per workgroup (of the slice's pass-0 run, or of the codes; not
// after count_slices, whose histogram is still there), its reduction, the scatter with private cursors.
static void pass1_counted(kr_ctx* c, Genome& G, const SortPlan& p, Lane& ln, Lane& ls, Slice& S, int s, const u64* src,
                          u64* pass1_dst) {
    hipStream_t ss = ls.stream;
    Geom g = slice_geom(c, (u32)s);
    if (p.cached_keys) g.wcmode = p.cached_mode;
    if (p.sliced) {
        StageScope sc(c, KR_ST_HIST8, ss);
        hipLaunchKernelGGL(k_hist8k, dim3(NWG), dim3(P1_T), 0, ss, src, (u64)S.nmax, g.sbits, (u32*)ln.partial8.p);
    } else if (!p.reuse_count) {
        StageScope sc(c, KR_ST_HIST8, ss);
        launch_hist8(c, G, ln, ss, g, p.one);
    }
    {
        StageScope sc(c, KR_ST_REDUCE8, ss);
        if (p.sliced || !p.reuse_count)
            hipLaunchKernelGGL(k_reduce8a, dim3(256), dim3(256), 0, ss, (u32*)ln.partial8.p, (u32*)ls.base1.p + 260);
        const u32 ntmax = (g.b > 8 && !p.coarse) ? p2_tiles(S.nmax) : 0u;
        hipLaunchKernelGGL(k_reduce8b, dim3(std::max(1u, (ntmax + 255) / 256)), dim3(256), 0, ss,
                           (const u32*)ls.base1.p + 260, (u32*)ls.base1.p, (u32*)ls.tp.p, ntmax ? P2_KEYS : 0u, ntmax,
                           (uint2*)ls.tiledesc.p, (const u32*)nullptr, 0u);
    }
    StageScope sc(c, KR_ST_SCATTER1, ss);
    if (p.sliced)
        hipLaunchKernelGGL(k_scatter1kp, dim3(NWG), dim3(P1_T), 0, ss, src, (u64)S.nmax, g.sbits,
                           (const u32*)ls.base1.p, (const u32*)ln.partial8.p, pass1_dst, (u32)S.nmax);
    else
        launch_scatter1(g, ss, (const u64*)ln.codes.p, (const u32*)ln.bad.p, G.nwords, (const u32*)ls.base1.p,
                        (const u64*)nullptr, (const u32*)ln.partial8.p, pass1_dst, S.nmax, p.one);
}

// The coarse exit: the buckets' bases leave the lane's scratch; the words finalize() reads: no oversized bucket, the key count.
static void coarse_exit(kr_ctx* c, Lane& ls, Slice& S, bool one) {
    StageScope sc(c, KR_ST_REDUCE8, ls.stream);
    hipLaunchKernelGGL(k_coarse_keep, dim3(1), dim3(320), 0, ls.stream, (const u32*)ls.base1.p, (u32*)S.off.p, 1u << c->g.b,
                       (u32*)S.ovf.p, one ? 2u : 1u);
}

// Pass 2 of a slice, from the lane's pass-1 array into the slice's keys: by fine offsets counted from the codes
// (fine16), or from the pass-1 keys (k_hist2 / k_scan2); at fan-out 2^8 pass 1 was the whole partition and its bases
// are the offsets.
static int pass2(kr_ctx* c, Genome& G, const SortPlan& p, Lane& ln, Lane& ls, Slice& S) {
    hipStream_t ss = ls.stream;
    const int b = c->g.b;
    const u32 nb = 1u << b;
    if (b <= 8) {
        HIPCHK(c, hipMemcpyAsync(S.off.p, ls.base1.p, 257 * 4, hipMemcpyDeviceToDevice, ss));
        return KR_OK;
    }
    const u32 ntmax = p2_tiles(S.nmax);
    if (p.fine16) {
        {
            StageScope sc(c, KR_ST_HIST2, ss);
            const u32 parts = nb > H16_BINS ? nb / H16_BINS : 1;
            hipLaunchKernelGGL(k_hist16, dim3(H16_RANGES, parts), dim3(H16_T), 0, ss, (const u64*)ln.codes.p,
                               (const u32*)ln.bad.p, G.nwords, (const u32*)ln.partial8.p, (const u32*)ls.base1.p + 260,
                               (unsigned short*)ln.partial16.p, (u32*)ln.h16exc.p, c->g.k, b);
        }
        {
            StageScope sc(c, KR_ST_SCAN2, ss);
            hipLaunchKernelGGL(k_hist16_off, dim3(256), dim3(1024), 0, ss, (const unsigned short*)ln.partial16.p,
                               (u32)H16_RANGES, b, (const u32*)ln.h16exc.p, (const u32*)ls.base1.p, (u32*)S.off.p,
                               (u32*)ls.cursor.p);
        }
        StageScope sc(c, KR_ST_SCATTER2, ss);
        launch_scatter2(ss, (const u64*)ls.tmpkeys.p, (u64*)S.keys.p, (const uint2*)ls.tiledesc.p, ntmax, (const u32*)nullptr,
                        (u32*)ls.cursor.p, b);
        return KR_OK;
    }
    {
        StageScope sc(c, KR_ST_HIST2, ss);
        hipLaunchKernelGGL(k_hist2<2 * P2_T>, dim3(ntmax), dim3(2 * P2_T), 0, ss, (const u64*)ls.tmpkeys.p,
                           (const uint2*)ls.tiledesc.p, (u32*)ls.tilehist.p, b);
    }
    {
        StageScope sc(c, KR_ST_SCAN2, ss);
        hipLaunchKernelGGL(k_scan2, dim3(256), dim3(1024), 0, ss, (u32*)ls.tilehist.p, (const u32*)ls.base1.p,
                           (const u32*)ls.tp.p, (u32*)S.off.p, b);
    }
    StageScope sc(c, KR_ST_SCATTER2, ss);
    launch_scatter2(ss, (const u64*)ls.tmpkeys.p, (u64*)S.keys.p, (const uint2*)ls.tiledesc.p, ntmax, (const u32*)ls.tilehist.p,
                    (u32*)nullptr, b);
    return KR_OK;
}

// k_localsort2 over `ntiles` descriptors of S's keys: what it cannot take it lists in S.ovf (segments from byte 16)
static void launch_localsort(kr_ctx* c, Slice& S, const DevBuf& desc, u32 ntiles, hipStream_t st) {
    hipLaunchKernelGGL(k_localsort2, dim3(std::min<u32>(ntiles, (u32)c->ls_grid)), dim3(LS_THREADS), 0, st, (u64*)S.keys.p,
                       (const u32*)S.off.p, (const uint4*)desc.p, ntiles, c->g.b, (u32*)S.ovf.p, (uint4*)((char*)S.ovf.p + 16));
}

// The chunk table of a slice's fine buckets, and -- unless the order is left for later -- the LDS sort inside them.
static void chunks_and_order(kr_ctx* c, const SortPlan& p, Lane& ln, Lane& ls, Slice& S) {
    hipStream_t ss = ls.stream;
    {
        StageScope sc(c, KR_ST_CHUNKS, ss);
        hipLaunchKernelGGL(k_chunk_table, dim3((S.nchunks + 255) / 256), dim3(256), 0, ss, (const u32*)S.off.p, 1u << c->g.b,
                           S.nchunks, (uint4*)S.chunkdesc.p, (u32*)S.ovf.p, (p.fine16 || p.route2) ? (u32*)ln.h16exc.p : (u32*)nullptr);
    }
    if (p.lazy) {
        c->lazy_skipped++;
        return;
    }
    // (what finalize() will want to know -- S.ovf[0], S.off[nb] -- goes to the host mailbox when somebody asks:
    // publish_slices, one launch for all slices asked about)
    StageScope sc(c, KR_ST_LOCALSORT, ss);
    launch_localsort(c, S, S.chunkdesc, S.nchunks, ss);
}

// The sort of one genome, enqueued on its lane(s): the table of contents of the passes above.
static int genome_sort(kr_ctx* c, int id, bool reuse_count, bool coarse) {
    if (!c) return KR_ERR_PARAM;
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    if (it->second.sl.empty()) return fail(c, KR_ERR_STATE, "genome %d has no slice plan (wide windows: use kr_wide_run)", id);
    HIPCHK(c, hipSetDevice(c->device));
    Genome& G = it->second;
    c->sorts_done++;
    int rc;
    Lane* lane;
    if ((rc = take_lane(c, G, lane))) return rc;
    Lane& ln = *lane;
    genome_unsorted(G);
    coarse_pool_step(c, G, coarse);
    const SortPlan p = sort_plan(c, G, ln, reuse_count, coarse);
    if (p.sliced) {
        if ((rc = pass0(c, G, p, ln))) return rc;
    } else if (!reuse_count) {
        pass_pack(c, G, ln);
    }
    if (p.nsl > 1 && (rc = slice_lanes_start(c, p, ln))) return rc;
    u64 region = 0;       // start of the current slice inside the pass-0 array
    for (int s = 0; s < c->nslices; s++) {
        Slice& S = G.sl[s];
        Lane& ls = (p.nsl > 1 && s % p.nsl) ? c->lanes[p.helper + s % p.nsl - 1] : ln;       // the slice's scratch and stream
        const u64* src = (const u64*)ln.pass0.p + region;
        region += S.nmax;
        S.count = -1;
        u64* pass1_dst;
        if ((rc = pass1_target(c, G, p, ls, S, pass1_dst))) return rc;
        if (p.route2) pass1_route2(c, p, ln, ls, S, s, src, pass1_dst);
        else pass1_counted(c, G, p, ln, ls, S, s, src, pass1_dst);
        if (coarse) {
            coarse_exit(c, ls, S, p.one);
            continue;
        }
        if ((rc = pass2(c, G, p, ln, ls, S))) return rc;
        chunks_and_order(c, p, ln, ls, S);
    }
    G.ordered = !p.lazy && !coarse;
    G.sorted = !coarse;   // enqueued; oversized buckets (if any) are resolved by finalize()
    G.coarse = coarse;
    G.one_strand = p.one;
    if (p.one) c->one_partitions++;
    return KR_OK;
}

// The two words finalize() reads of each listed slice, into the host mailbox (n <= PUB_CAP; the caller synchronises
// `st` before the next call of this function: the table is one).
// a coarse genome (kr_genome_partition) sorted whole after all, from its resident bases: pass 1 runs again -- the price of
// the rare path (a reader of its keys, a candidate list the coarse route does not take)
static int ensure_fine(kr_ctx* c, Genome& G) {
    if (!G.coarse) return KR_OK;
    c->coarse_promoted++;
    return genome_sort(c, G.id, false);
}
static int ensure_fine_id(kr_ctx* c, int id) {
    auto it = c->genomes.find(id);
    return (it == c->genomes.end()) ? KR_OK : ensure_fine(c, it->second);
}

static void publish_slices(kr_ctx* c, Slice* const* sl, size_t n, hipStream_t st) {
    PubEnt* tab = (PubEnt*)(c->mbox + MB_WORDS);
    const u32 nb = 1u << c->g.b;
    for (size_t i = 0; i < n; i++) {
        tab[i].ovf = (const u32*)sl[i]->ovf.p;
        tab[i].tot = (const u32*)sl[i]->off.p + nb;
        tab[i].res = (u32)sl[i]->res;
        tab[i].pad = 0;
    }
    if (n) hipLaunchKernelGGL(k_publish_slices, dim3((u32)(n + 63) / 64), dim3(64), 0, st, (const PubEnt*)tab, (u32)n, c->mbox + MB_SLICE0);
}

// KR_OPT_LAZY_ORDER: the LDS sort of a genome whose sort stopped at the fine buckets, on stream `st` (the caller has ordered
// `st` behind the genome's partition passes: join_lanes).  The genome counts as not finalized again: the oversized buckets
// this launch may list are finalize()'s to resolve, as after an eager sort.
static int order_genome(kr_ctx* c, Genome& G, hipStream_t st) {
    if (!G.sorted || G.ordered) return KR_OK;
    for (Slice& S : G.sl) {
        HIPCHK(c, hipMemsetAsync(S.ovf.p, 0, 16, st));
        StageScope sc(c, KR_ST_LOCALSORT, st);
        launch_localsort(c, S, S.chunkdesc, S.nchunks, st);
        c->lazy_ordered++;
    }
    G.ordered = true;
    G.finalized = false;
    return KR_OK;
}

// every listed genome in full order (the readers that walk or search a genome's keys: fetch, the candidate probes, the
// chunk kernel of the intersection, a collect over many candidates); the caller calls finalize() behind it
static int ensure_ordered(kr_ctx* c, const std::vector<Genome*>& gs) {
    bool any = false;
    for (Genome* G : gs) any = any || (G->sorted && !G->ordered);
    if (!any) return KR_OK;
    int rc = join_lanes(c);
    if (rc) return rc;
    for (Genome* G : gs)
        if ((rc = order_genome(c, *G, c->stream))) return rc;
    return KR_OK;
}

// The merge fallback of finalize(): slice S of `total` keys has `novf` buckets the LDS sort could not take (listed in
// S.ovf; more than OVF_MAX: the whole slice counts as one).  Their 4096-key tiles are sorted by the LDS sorter and merged
// in global memory, through lane 0's pass-1 array, on stream `st`.
static int repair_slice(kr_ctx* c, Slice& S, u32 novf, u32 total, hipStream_t st) {
    StageScope sc(c, KR_ST_FALLBACK);
    const u32 nb = 1u << c->g.b;
    std::vector<uint4> segs;
    uint4* dsegs = (uint4*)((char*)S.ovf.p + 16);
    if (novf > OVF_MAX) {
        segs.push_back(make_uint4(0, total, 0, nb));      // everything: bucket range [0, nb)
    } else {
        segs.resize(novf);
        HIPCHK(c, hipMemcpy(segs.data(), dsegs, (size_t)novf * 16, hipMemcpyDeviceToHost));
        for (auto& sg : segs) sg.w = sg.z + 1;               // bucket range [f, f + 1)
    }
    c->overflow_segments += (int64_t)segs.size();
    // (1) sort the 4096-key tiles of every segment with the LDS sorter
    std::vector<uint4> tiles;
    u32 maxlen = 0;
    for (auto& sg : segs) {
        maxlen = std::max(maxlen, sg.y - sg.x);
        for (u32 t = sg.x; t < sg.y; t += LS_CAP) tiles.push_back(make_uint4(t, std::min(t + LS_CAP, sg.y), sg.z, sg.w));
    }
    int rc;
    if ((rc = ensure(c, c->fbdesc, tiles.size() * 16 + 16))) return rc;
    if ((rc = ensure(c, c->fbsegs, (segs.size() + 1) * 16))) return rc;
    HIPCHK(c, hipMemcpy(c->fbdesc.p, tiles.data(), tiles.size() * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(S.ovf.p, 0, 16, st));
    launch_localsort(c, S, c->fbdesc, (u32)tiles.size(), st);
    c->fallback_launches++;
    // (2) merge rounds: runs of `run` keys -> 2 * run, through the lane scratch and back
    Lane& ln = c->lanes[0];
    if ((rc = ensure(c, ln.tmpkeys, ((size_t)total + 2) * 8))) return rc;
    for (u64 run = LS_CAP; run < maxlen; run *= 2) {
        std::vector<uint4> act;
        u32 ntiles = 0;
        for (auto& sg : segs) {
            u32 len = sg.y - sg.x;
            if (len <= run) continue;
            act.push_back(make_uint4(sg.x, sg.y, ntiles, 0));
            ntiles += (len + MG_TILE - 1) / MG_TILE;
        }
        if (act.empty()) break;
        HIPCHK(c, hipMemcpy(c->fbsegs.p, act.data(), act.size() * 16, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_seg_merge, dim3(ntiles), dim3(MG_T), 0, st, (const u64*)S.keys.p,
                           (u64*)ln.tmpkeys.p, (const uint4*)c->fbsegs.p, (u32)act.size(), (u32)run);
        hipLaunchKernelGGL(k_seg_copy, dim3(ntiles), dim3(256), 0, st, (const u64*)ln.tmpkeys.p,
                           (u64*)S.keys.p, (const uint4*)c->fbsegs.p, (u32)act.size());
        HIPCHK(c, hipStreamSynchronize(st));      // fbsegs is rewritten next round
        c->fallback_launches += 2;
    }
    HIPCHK(c, hipGetLastError());
    return KR_OK;
}

// Resolve what the asynchronous sort left open: the key counts and -- rarely -- the
// oversized buckets the LDS sort could not take (bitonic fallback in global memory).
// One small D2H + sync for ALL listed genomes.
// already_synced: the caller has published the slices' words (publish_slices) and waited for the stream since
// (kr_intersect launches its kernels over the freshly sorted genomes and looks at the sorts' words after its own
// synchronisation);
// *repaired = some slice went through the merge fallback (what was computed from it meanwhile is void)
static int finalize(kr_ctx* c, const std::vector<Genome*>& gs, bool already_synced = false, bool* repaired = nullptr) {
    if (repaired) *repaired = false;
    std::vector<Slice*> todo;
    std::vector<Genome*> tg;
    for (Genome* G : gs)
        if ((G->sorted || G->coarse) && !G->finalized) {
            tg.push_back(G);
            for (Slice& S : G->sl) todo.push_back(&S);
        }
    if (tg.empty()) return KR_OK;
    hipStream_t st = c->stream;
    if (!already_synced) {
        int rcj = join_lanes(c);
        if (rcj) return rcj;
    }
    std::vector<u32> novf(todo.size()), total(todo.size());
    if (!already_synced) {
        for (size_t i0 = 0; i0 < todo.size(); i0 += PUB_CAP) {
            publish_slices(c, todo.data() + i0, std::min<size_t>(PUB_CAP, todo.size() - i0), st);
            HIPCHK(c, hipStreamSynchronize(st));         // (two words per slice in the host mailbox: no copies)
        }
        HIPCHK(c, hipGetLastError());
    }
    for (size_t i = 0; i < todo.size(); i++) {
        const volatile u32* w = c->mbox + MB_SLICE0 + 2 * todo[i]->res;
        novf[i] = w[0];
        total[i] = w[1];
    }
    for (size_t i = 0; i < todo.size(); i++) {
        Slice& S = *todo[i];
        S.count = total[i];
        if (novf[i]) {
            if (repaired) *repaired = true;
            int rc = repair_slice(c, S, novf[i], total[i], st);
            if (rc) return rc;
        }
    }
    for (Genome* G : tg) {
        G->count = 0;
        for (Slice& S : G->sl) G->count += S.count;
        G->finalized = true;
    }
    return KR_OK;
}

int64_t kr_genome_load_sorted(kr_ctx* c, int id, const uint64_t* keys, size_t n) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (n > 2 * c->max_bases) return fail(c, KR_ERR_PARAM, "%zu keys exceed 2 * max_bases", n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    Genome& G = c->genomes[id];
    G.id = id;
    G.n_bases = 0;
    G.nwords = 0;
    G.nmax = n;
    for (Slice& S : G.sl) release_slice(c, S);         // (whatever their number: the arrays are sized anew below)
    G.sl.assign(c->nslices, Slice());
    const u32 nb = 1u << c->g.b;
    const int sbits = c->g.sbits;
    hipStream_t st = c->stream;
    size_t pos = 0;
    std::vector<u64> rel;
    for (int s = 0; s < c->nslices; s++) {
        // the slice's keys are a contiguous run of the sorted input; store them relative
        size_t end = n;
        if (sbits && s + 1 < c->nslices) {
            const u64 bound = (u64)(s + 1) << (64 - sbits);
            end = std::lower_bound(keys + pos, keys + n, (uint64_t)bound) - keys;
        }
        const size_t cnt = end - pos;
        Slice& S = G.sl[s];
        int rc = alloc_slice(c, S, cnt);
        if (rc) return rc;
        if (cnt) {
            const void* src = keys + pos;
            if (sbits) {
                rel.resize(cnt);
                for (size_t i = 0; i < cnt; i++) rel[i] = (u64)keys[pos + i] << sbits;
                src = rel.data();
            }
            HIPCHK(c, hipMemcpy(S.keys.p, src, cnt * 8, hipMemcpyHostToDevice));
        }
        hipLaunchKernelGGL(k_offsets_from_sorted, dim3((nb + 1 + 255) / 256), dim3(256), 0, st, (const u64*)S.keys.p,
                           (u32)cnt, nb, c->g.rb, (u32*)S.off.p);
        hipLaunchKernelGGL(k_chunk_table, dim3((S.nchunks + 255) / 256), dim3(256), 0, st, (const u32*)S.off.p, nb,
                           S.nchunks, (uint4*)S.chunkdesc.p, (u32*)S.ovf.p, (u32*)nullptr);
        S.count = (int64_t)cnt;
        pos = end;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    G.uploaded = false;
    G.coarse = G.hits_valid = false;
    coarse_pool_return(c, G);
    G.sorted = true;
    G.ordered = true;
    G.finalized = true;
    G.count = (int64_t)n;
    return (int64_t)n;
}

int64_t kr_genome_count(kr_ctx* c, int id) {
    if (!c) return KR_ERR_PARAM;
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !(it->second.sorted || it->second.coarse)) return fail(c, KR_ERR_STATE, "genome %d not sorted", id);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = finalize(c, {&it->second});          // (a coarse genome stays coarse: its count comes from pass 1's histogram)
    if (rc) return rc;
    return it->second.count;
}

int64_t kr_genome_add(kr_ctx* c, int id, const uint8_t* bases, size_t n) {
    int rc = kr_genome_upload(c, id, bases, n);
    if (rc) return rc;
    rc = kr_genome_sort(c, id);
    if (rc) return rc;
    return kr_genome_count(c, id);
}

int64_t kr_genome_fetch_keys(kr_ctx* c, int id, uint64_t* out, size_t cap) {
    if (!c) return KR_ERR_PARAM;
    {
        auto it = c->genomes.find(id);
        if (it != c->genomes.end() && it->second.coarse) {
            HIPCHK(c, hipSetDevice(c->device));
            int rcf = ensure_fine(c, it->second);
            if (rcf) return rcf;
        }
        if (it != c->genomes.end() && it->second.sorted) {
            HIPCHK(c, hipSetDevice(c->device));
            int rco = ensure_ordered(c, {&it->second});
            if (rco) return rco;
        }
    }
    int64_t n = kr_genome_count(c, id);
    if (n < 0) return n;
    if ((size_t)n > cap) return fail(c, KR_ERR_CAPACITY, "key buffer too small: %lld > %zu", (long long)n, cap);
    Genome& G = c->genomes[id];
    HIPCHK(c, hipDeviceSynchronize());
    const int sbits = c->g.sbits;
    size_t pos = 0;
    for (int s = 0; s < c->nslices; s++) {
        Slice& S = G.sl[s];
        const size_t cnt = (size_t)S.count;
        if (cnt) HIPCHK(c, hipMemcpy(out + pos, S.keys.p, cnt * 8, hipMemcpyDeviceToHost));
        if (sbits) {      // relative -> absolute
            const u64 top = (u64)s << (64 - sbits);
            for (size_t i = 0; i < cnt; i++) out[pos + i] = top | (out[pos + i] >> sbits);
        }
        pos += cnt;
    }
    return n;
}

// keys of a genome in STREAM order (no sort): the windows as they come, both strands of a window
// one after the other (or the single key of kr_set_strands' other modes)
int64_t kr_genome_keys_in_order(kr_ctx* c, int id, uint64_t* out, size_t cap) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (c->wide.on) return fail(c, KR_ERR_PARAM, "kr_genome_keys_in_order: packed windows only");
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    HIPCHK(c, hipSetDevice(c->device));
    Genome& G = it->second;
    Lane& ln = c->lanes[0];
    hipStream_t st = c->stream;
    int rc;
    if ((rc = join_lanes(c))) return rc;
    launch_pack(c, G, ln, st);
    const u64 npos = G.n_bases;
    if (npos == 0) return 0;
    const u32 ntiles = (u32)((npos + 2047) / 2048);
    DevBuf tsum, tpos, keys;
    if ((rc = ensure(c, tsum, ((size_t)ntiles + 4) * 4)) || (rc = ensure(c, tpos, ((size_t)ntiles + 4) * 8))) {
        release(c, tsum); release(c, tpos);
        return rc;
    }
    const Geom g = pass0_geom(c);
    hipLaunchKernelGGL(k_order_count, dim3(ntiles), dim3(256), 0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p, npos, g,
                       (u32*)tsum.p);
    hipLaunchKernelGGL(k_scan64, dim3(1), dim3(1024), 0, st, (const u32*)tsum.p, (u64*)tpos.p, ntiles);
    u64 total = 0;
    hipError_t e = hipMemcpyAsync(&total, (u64*)tpos.p + ntiles, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || total > cap) {
        release(c, tsum); release(c, tpos);
        if (e != hipSuccess) return fail(c, KR_ERR_HIP, "kr_genome_keys_in_order: %s", hipGetErrorString(e));
        return fail(c, KR_ERR_CAPACITY, "key buffer too small: %llu > %zu", (unsigned long long)total, cap);
    }
    if (total) {
        if ((rc = ensure(c, keys, (size_t)total * 8))) { release(c, tsum); release(c, tpos); return rc; }
        hipLaunchKernelGGL(k_order_emit, dim3(ntiles), dim3(256), 0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p, npos,
                           g, (const u64*)tpos.p, (u64*)keys.p);
        e = hipMemcpy(out, keys.p, (size_t)total * 8, hipMemcpyDeviceToHost);
    }
    release(c, tsum); release(c, tpos); release(c, keys);
    if (e != hipSuccess) return fail(c, KR_ERR_HIP, "kr_genome_keys_in_order: %s", hipGetErrorString(e));
    HIPCHK(c, hipGetLastError());
    return (int64_t)total;
}

int kr_genome_free(kr_ctx* c, int id) {
    if (!c) return KR_ERR_PARAM;
    auto it = c->genomes.find(id);
    if (it == c->genomes.end()) return fail(c, KR_ERR_PARAM, "unknown genome %d", id);
    (void)hipDeviceSynchronize();
    release_genome(c, it->second);
    c->genomes.erase(it);
    return KR_OK;
}

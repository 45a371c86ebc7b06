// h_wide.inc -- part of krisp_hip.hip (one translation unit): host: wide path driver (kr_wide_run, kr_wide_fetch)
// ----------------------------------------------------------------------------
// wide path driver
// ----------------------------------------------------------------------------
// kr_wide_run is wide_run_once, again in smaller batches while a phase runs out of memory.  wide_run_once is a sequence
// of named passes over one WideRun (the call's arguments, the environment, the locate pass's decisions); every sort +
// intersect phase is wide_phase: phase_sort_intersect, then the dictionary (dict_canonical, dict_minimizer or
// dict_index_slots).  The passes' header comments say what each reads and leaves behind.
static int ceil_log2(u64 n) { int b = 0; while ((1ull << b) < n) b++; return b; }
static size_t free_bytes() { size_t fr = 0, tot = 0; return hipMemGetInfo(&fr, &tot) == hipSuccess ? fr : 0; }
// what n buffers of have[] bytes must still allocate to hold want[] bytes each (a buffer that grows is allocated whole)
static size_t bytes_missing(const size_t* want, const size_t* have, int n) {
    size_t need = 0;
    for (int q = 0; q < n; q++) need += want[q] > have[q] ? want[q] : 0;
    return need;
}

// The wide path's environment (A/B, tests), read by kr_wide_run at the start of every call; KR_WIDE_CANON once per process.
struct WideEnv {
    int batch;              // KR_WIDE_BATCH: genomes per batch of the sort + intersect phases to start with (0: all at once)
    bool canon;             // KR_WIDE_CANON=0: the full list of a shared spectrum, not its canonical flanks
    bool has_keyfrac;       // KR_WIDE_KEYFRAC: the share of window starts a key list's segments are sized for
    double keyfrac;
    bool keylist;           // KR_WIDE_KEYLIST=0: composite keys per window start, never as lists
    int cache;              // KR_WIDE_CACHE: 1 / 0 = a cache of composite keys per genome / one for all; -1 = by the memory
    bool loclist;           // KR_WIDE_LOCLIST=0: the member windows per window start, never as a list
    u64 loccap;             // KR_WIDE_LOCCAP: that list's room in entries (0: by the groups)
};
static WideEnv wide_env() {
    static const bool canon_on = [] { const char* e = getenv("KR_WIDE_CANON"); return e ? atoi(e) != 0 : true; }();
    const char *b = getenv("KR_WIDE_BATCH"), *kf = getenv("KR_WIDE_KEYFRAC"), *kl = getenv("KR_WIDE_KEYLIST"),
               *ca = getenv("KR_WIDE_CACHE"), *ll = getenv("KR_WIDE_LOCLIST"), *lc = getenv("KR_WIDE_LOCCAP");
    WideEnv e;
    e.batch = b ? atoi(b) : 0;
    e.canon = canon_on;
    e.has_keyfrac = kf != nullptr;
    e.keyfrac = kf ? atof(kf) : 0.0;
    e.keylist = kl ? atoi(kl) != 0 : true;
    e.cache = ca ? (atoi(ca) != 0 ? 1 : 0) : -1;
    e.loclist = ll ? atoi(ll) != 0 : true;
    e.loccap = lc ? (u64)atoll(lc) : 0ull;
    return e;
}

// several ranks: every rank learns whether all of them got through the local work before the next exchange
// (a rank that failed returns its own error; the others return KR_ERR_STATE instead of waiting for it)
static int wide_agree(kr_ctx* c, int rc) {
    if (kr_comm_world(c) <= 1) return rc;
    double bad = rc < 0 ? 1.0 : 0.0;
    const std::string mine = rc < 0 ? c->err : std::string();
    const int rca = kr_comm_allreduce(c, &bad, 1, 1);
    if (rc < 0) { c->err = mine; g_last_error = mine; return rc; }
    if (rca) return rca;
    if (bad > 0) return fail(c, KR_ERR_STATE, "kr_wide_run: another rank failed");
    return KR_OK;
}
// Memory is given back only when the next allocations would not fit (a repeated run finds every buffer of
// the previous one and allocates nothing: hipMalloc / hipFree of tens of GB cost more than the kernels).
// Before the locate pass its buffers of the previous run are the first to go.
static int wide_make_room(kr_ctx* c, size_t need) {
    if (free_bytes() >= need + ((size_t)1 << 30)) return KR_OK;
    HIPCHK(c, hipDeviceSynchronize());
    kr_ctx::Bufs lb;
    c->wide.locate_bufs(lb);
    for (DevBuf* b : lb) release(c, *b);
    return KR_OK;
}
// the candidate buffers go back (the next intersection or exchange sizes its own)
static void cands_drop(kr_ctx* c) {
    release(c, c->candA);
    release(c, c->candB);
    c->ncand = -1;
}
// the exclusive scan of n counts on `st` through the wide path's tile scratch: out[n] = the total; out may be `in`
static int excl_scan_tiles(kr_ctx* c, hipStream_t st, const u32* in, u32 n, u32* out) {
    auto& w = c->wide;
    const size_t ntiles = (n + 2047) / 2048;
    int rc;
    if ((rc = ensure(c, w.tsum, (ntiles + 4) * 4))) return rc;
    if ((rc = ensure(c, w.tpos, (ntiles + 4) * 4))) return rc;
    launch_excl_scan(st, in, n, (u32*)w.tsum.p, (u32*)w.tpos.p, out);
    return KR_OK;
}

// ---- a genome's cache of composite keys (Geom.wcache), made before its count_slices
// a key list's segment (Geom.wlcnt: one per workgroup of k_hist8w) in entries, sized for `frac` of the workgroup's window
// starts; the bytes of a list of such segments
static u32 key_list_cap(const Genome& G, double frac) {
    const u64 per_wg = (G.nwords + NWG - 1) / NWG * 32;
    return (u32)std::min<double>(4.0e9, (double)per_wg * frac + 256.0);
}
static size_t key_list_bytes(u32 cap) { return (size_t)NWG * cap * 16 + 64; }
static size_t key_dense_bytes(const Genome& G) { return (G.nwords + PAD_WORDS) * 32 * 16; }
// 16 bytes per window start; leaves c->g naming it
static int key_cache_dense(kr_ctx* c, Genome& G) {
    int rc;
    if ((rc = ensure(c, G.wkeys, key_dense_bytes(G)))) return rc;
    c->g.wcache = (u64*)G.wkeys.p;
    c->g.wlcnt = nullptr;
    c->g.wlcap = 0;
    G.wlist = false;
    return KR_OK;
}
// a list sized for w.key_list_frac; leaves c->g and the genome naming it
static int key_cache_list(kr_ctx* c, Genome& G) {
    const u32 cap = key_list_cap(G, c->wide.key_list_frac);
    int rc;
    if ((rc = ensure(c, G.wkeys, key_list_bytes(cap)))) return rc;
    if ((rc = ensure(c, G.wlcnt, (size_t)NWG * 4))) return rc;
    c->g.wcache = (u64*)G.wkeys.p;
    c->g.wlcnt = (u32*)G.wlcnt.p;
    c->g.wlcap = cap;
    G.wlist = true;
    G.wlcap = cap;
    return KR_OK;
}

// ---- one sort + intersect phase (wide_phase)
// Sorts the n listed genomes under the current c->g and intersects them, no filter: the values present in every genome
// are in c->candB, their number is returned.  Reads w.batch, w.genome_cache and w.key_list; a key list that overflows
// clears w.key_list for the rest of the call (w.key_list_failed).  count_windows_wk > 0: the genomes' amplicon-long
// windows are counted into w.wcount on the way.  No collective.
// The streaming form (w.batch): the values present in EVERY genome are a running intersection -- monotone, like the masks
// of the packed path's candidates --, so the genomes may go through the sort in batches: the first batch is intersected,
// every later batch looks the running list up in its sorted genomes (kr_cands_probe: one step of the reference's merge
// tree, intersectAmplicons.py:256-307, on lists), and a batch's sorted keys -- 16 bytes per base, the bulk of what a
// genome holds during a phase -- go back before the next batch is sorted.  Same list as the one-shot intersection.
static int64_t phase_sort_intersect(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int count_windows_wk) {
    int rc;
    const int B = (c->wide.batch > 0 && c->wide.batch < n) ? c->wide.batch : n;
    int64_t cur = -1;
    for (int b0 = 0; b0 < n; b0 += B) {
        const int b1 = std::min(n, b0 + B);
        for (int i = b0; i < b1; i++) {
            Genome& G = c->genomes[ids[i]];
            if (c->g.wmode == 2 && c->wide.genome_cache && (rc = c->wide.key_list ? key_cache_list(c, G) : key_cache_dense(c, G)))
                return rc;
            rc = count_slices(c, G);
            if (rc == KR_RETRY_DENSE) {
                // a workgroup found more keys than its segment holds (the estimate was for unrelated flanks): this genome
                // and the ones behind it take 16 bytes per window start as before
                c->wide.key_list = false;
                c->wide.key_list_failed = true;
                if ((rc = key_cache_dense(c, G))) return rc;
                rc = count_slices(c, G);
            }
            if (rc) return rc;
            if (count_windows_wk) {       // (the genome's bad bits are in its lane now: its amplicon-long windows, for the record count)
                Lane& ln = c->lanes[c->next_lane];
                hipLaunchKernelGGL(k_count_windows, dim3(1024), dim3(256), 0, ln.stream, (const u32*)ln.bad.p, G.nwords,
                                   count_windows_wk, (unsigned long long*)c->wide.wcount.p + i);
            }
            if ((rc = genome_sort(c, ids[i], true))) return rc;
        }
        if (b0 == 0) cur = kr_intersect(c, ids, b1, is_in, 0);          // (more than 32 genomes: cascaded inside, on the device)
        else if (cur > 0) cur = cands_probe_impl(c, ids + b0, b1 - b0, is_in + b0, 0, true);
        if (cur < 0) return cur;
        if (B < n) {
            HIPCHK(c, hipDeviceSynchronize());
            for (int i = b0; i < b1; i++) genome_drop_sorted(c, c->genomes[ids[i]]);
        }
    }
    return cur;
}

// Dict.canon: of a spectrum closed under reverse complement only the canonical flanks are kept (the list stays sorted).
// Reads the nc candidates in c->candB; returns how many stay there (all of them, d.canon unset, where the list is not
// closed -- the packed spectra are) or an error.
static int64_t dict_canonical(kr_ctx* c, kr_ctx::Wide::DictBufs& d, int64_t nc, int flank_len) {
    hipStream_t st = c->stream;
    const u32 n0 = (u32)nc, nblk = (n0 + 255) / 256;
    int rc;
    if ((rc = cands_compact_room(c, n0))) return rc;
    if ((rc = ensure(c, c->wide.tsum, 64))) return rc;
    HIPCHK(c, hipMemsetAsync(c->wide.tsum.p, 0, 4, st));
    hipLaunchKernelGGL(k_flag_canonical, dim3(nblk), dim3(256), 0, st, (const kr_cand*)c->candB.p, n0, flank_len,
                       (u32*)c->flags.p, (u32*)c->blockcnt.p, (u32*)c->wide.tsum.p);
    const u32* dkept = cands_compact_enqueue(c, n0, st, false);
    u32 kept = 0, npal = 0;
    HIPCHK(c, hipMemcpyAsync(&kept, dkept, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&npal, c->wide.tsum.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (2ull * kept - npal != n0) return nc;
    d.canon = true;
    return cands_compact_adopt(c, kept);
}

// The minimizer form (see Dict) of the nc sorted keys in d.keys: a minimizer is shared by ~9 consecutive windows, so
// occupied buckets hold ~9 keys or a multiple; ~4 keys per bucket overall; counting sort by bucket, every bucket sorted
// by value.  took: d.mzT / d.mzB / d.mzlen / d.mznb are the look-up form; not taken (more crowded buckets than the list
// holds: a degenerate spectrum), dict_index_slots takes the dictionary.
static int dict_minimizer(kr_ctx* c, kr_ctx::Wide::DictBufs& d, int64_t nc, int flank_len, bool& took) {
    hipStream_t st = c->stream;
    const u32 nb = (u32)std::max<int64_t>(1, nc / 4), bigcap = 1u << 16;
    int rc;
    took = false;
    const size_t want[] = {((size_t)nc + 2) * 8, ((size_t)nb + 4) * 4, ((size_t)nc + 4 + bigcap) * 4};     // (d.idx as scratch: places inside the buckets, list of big buckets)
    const size_t have[] = {d.mzT.bytes, d.mzB.bytes, d.idx.bytes};
    const size_t need = bytes_missing(want, have, 3);
    if (need && (rc = wide_make_room(c, need))) return rc;
    if ((rc = ensure(c, d.mzT, want[0]))) return rc;
    if ((rc = ensure(c, d.mzB, want[1]))) return rc;
    if ((rc = ensure(c, d.idx, want[2]))) return rc;
    u32 *B = (u32*)d.mzB.p, *within = (u32*)d.idx.p, *big = (u32*)d.idx.p + nc + 2;
    HIPCHK(c, hipMemsetAsync(B, 0, want[1], st));
    HIPCHK(c, hipMemsetAsync(big, 0, 4, st));
    const u32 grid = ((u32)nc + 255) / 256;
    hipLaunchKernelGGL(k_mz_count, dim3(grid), dim3(256), 0, st, (const u64*)d.keys.p, (u32)nc, flank_len, nb, B, within);
    if ((rc = excl_scan_tiles(c, st, B, nb, B))) return rc;
    hipLaunchKernelGGL(k_mz_scatter, dim3(grid), dim3(256), 0, st, (const u64*)d.keys.p, (u32)nc, flank_len, nb,
                       (const u32*)B, (const u32*)within, (u64*)d.mzT.p);
    hipLaunchKernelGGL(k_mz_sort, dim3((nb + 255) / 256), dim3(256), 0, st, (u64*)d.mzT.p, (const u32*)B, nb, big, bigcap);
    u32 nbig = 0;
    HIPCHK(c, hipMemcpyAsync(&nbig, big, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (nbig > bigcap) return KR_OK;
    if (nbig)
        hipLaunchKernelGGL(k_mz_sort_big, dim3(nbig), dim3(256), 0, st, (u64*)d.mzT.p, (const u32*)B, (const u32*)big);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    d.mzlen = flank_len;
    d.mznb = nb;
    took = true;
    return KR_OK;
}

// The top-bits index of the nc sorted keys in d.keys (d.idx, d.ib: ~1 entry per bucket) and, when it pays and fits a
// third of the free memory, the one-sector slot form (d.slots, d.sb: see Dict in k_keys.inc).
static int dict_index_slots(kr_ctx* c, kr_ctx::Wide::DictBufs& d, int64_t nc, int keybits) {
    hipStream_t st = c->stream;
    int rc;
    int ib = std::max(1, std::min(std::min(27, keybits), ceil_log2((u64)nc + 1)));
    // slots: 0.75 .. 1.5 keys per 32-byte slot when the 40 bits of an entry hold the rest of the key and the
    // table fits; the index is then built at the slot resolution (it also serves the crowded slots)
    int sb = std::max(1, std::min(std::min(31, keybits), ceil_log2((2 * (u64)nc + 2) / 3)));
    if (keybits - sb > 40 && (keybits - 40 <= 23 || keybits - 40 <= sb + 3))
        sb = keybits - 40;     // (few long keys: a sparser table, if it is small or at most 8 x the policy's)
    bool slots = c->wide.use_slots && nc > 0 && keybits - sb <= 40;
    if (slots) {
        const size_t want = ((size_t)32 << sb) + ((size_t)4 << sb), have = d.slots.bytes + d.idx.bytes;
        if (want > have && (rc = wide_make_room(c, want))) return rc;
        slots = want <= free_bytes() / 3 + have;
    }
    if (slots) ib = sb;
    d.ib = ib;
    if ((rc = ensure(c, d.idx, (((size_t)1 << ib) + 2) * 4))) return rc;
    if (slots && (rc = ensure(c, d.slots, (size_t)32 << sb))) return rc;
    HIPCHK(c, hipMemsetAsync(d.idx.p, 0xFF, (((size_t)1 << ib) + 1) * 4, st));
    if (nc)
        hipLaunchKernelGGL(k_index_sorted, dim3((u32)(((u64)nc + 255) / 256)), dim3(256), 0, st, (const u64*)d.keys.p,
                           (u32)nc, ib, (u32*)d.idx.p);
    hipLaunchKernelGGL(k_index_fill, dim3((u32)((((u64)1 << ib) + 1 + 255) / 256)), dim3(256), 0, st,
                       (const u64*)d.keys.p, (u32)nc, ib, (u32*)d.idx.p);
    if (slots) {
        hipLaunchKernelGGL(k_slot_build, dim3((u32)((((u64)1 << sb) + 255) / 256)), dim3(256), 0, st, (const u64*)d.keys.p,
                           (const u32*)d.idx.p, sb, (uint4*)d.slots.p);
        d.sb = sb;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return KR_OK;
}

// Sort every listed genome under the current c->g and intersect them (no filter): the candidates' prefixes, dense and
// sorted, go to d.keys with ONE look-up form -- minimizer buckets (flank_len >= MZ_MINLEN: the keys are flanks of that
// many bases) or a top-bits index, with slots when it pays.  Returns the dictionary's size; 0 leaves an empty one.
// Collectives, on every rank alike: wide_agree behind the local phase, then (several ranks, each with its own genomes)
// kr_cands_reduce and kr_cands_bcast -- the lists are intersected over the ranks by the packed path's tree reduction and
// the result returns to every rank; every rank then builds the same dictionary (the tables are deterministic), so ranks
// and composite keys agree everywhere.  A failure behind the broadcast is the rank's own: the next wide_agree tells.
static int64_t wide_phase(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, kr_ctx::Wide::DictBufs& d, int keybits,
                          int flank_len = 0, int count_windows_wk = 0, bool canonical = false) {
    d.sb = 0;
    d.mzlen = 0;
    d.canon = false;
    int rc;
    int64_t nc = phase_sort_intersect(c, ids, n, is_in, count_windows_wk);
    if ((rc = wide_agree(c, nc < 0 ? (int)nc : KR_OK))) return rc;
    if (kr_comm_world(c) > 1) {
        if ((nc = kr_cands_reduce(c, 0)) < 0) return nc;
        if ((nc = kr_cands_bcast(c)) < 0) return nc;
    }
    if (nc >= (1ll << 32) - 1) return fail(c, KR_ERR_CAPACITY, "wide path: %lld dictionary entries (>= 2^32)", (long long)nc);
    d.nfull = (u32)nc;
    if (canonical && nc > 0 && (nc = dict_canonical(c, d, nc, flank_len)) < 0) return nc;
    if ((rc = ensure(c, d.keys, ((size_t)nc + 2) * 8))) return rc;
    if (nc)
        hipLaunchKernelGGL(k_cand_prefixes, dim3(((u32)nc + 255) / 256), dim3(256), 0, c->stream, (const kr_cand*)c->candB.p,
                           (u32)nc, (u64*)d.keys.p);
    d.n = (u32)nc;
    if (flank_len >= MZ_MINLEN && !c->wide.ordered && nc > 0) {
        bool took = false;
        if ((rc = dict_minimizer(c, d, nc, flank_len, took))) return rc;
        if (took) return nc;
    }
    if ((rc = dict_index_slots(c, d, nc, keybits))) return rc;
    return nc;
}

struct WideRun;
static int64_t wide_run_once(kr_ctx* c, WideRun& r);

// What one attempt of kr_wide_run works on: the call, the environment, and -- from locate_plan on -- every decision of
// the locate / count / emit passes.  The run's results live in c->wide.
struct WideRun {
    const int* ids;
    int n;
    const uint8_t* is_in;
    int apply_filter;
    WideEnv env;
    bool counted = false;           // flank_ranks: the genomes' record counts came from k_count_windows
    // locate_plan
    u32 nf = 0;                     // groups in w.fin
    int W = 1;                      // mask words of 16 columns per group and side
    size_t kwords = 0, ksum_off = 0;    // w.keep: the keep bits' words, then (from ksum_off on) their summary bits
    std::vector<u64> cioff;         // the dense form's place of genome i in w.cibuf, in window starts; cioff[n]: all of them
    bool any_wlist = false;         // a genome's cached keys are a list: the dense form needs w.cibuf for it
    bool use_list = false;          // the member windows as a list (k_wide_locate) instead of a group number per window start
    u64 loc_cap = 0;                // ... its room in entries, WIDE_SEGS segments of seg_cap()
    DevBuf* loc_borrow = nullptr;   // ... kept in this idle sort scratch instead of w.loc
    size_t loc_need = 0;            // bytes the passes still have to allocate
    u32 nloc = 0;                   // locate_overflow: entries listed (0: the dense form ran)

    uint4* list(const kr_ctx::Wide& w) const { return (uint4*)(loc_borrow ? loc_borrow->p : w.loc.p); }
    u32 seg_cap() const { return (u32)(loc_cap / WIDE_SEGS); }
    size_t list_bytes() const { return (size_t)loc_cap * 16 + 64; }
    size_t cibuf_bytes() const { return (cioff[n] + 2) * sizeof(uint2); }
    size_t keep_bytes() const { return (ksum_off + kwords / 64 + 2) * 8; }
    // what w.masks, w.keep, w.cnt, w.hitoff and w.cursor must hold
    void sizes(size_t want[5]) const {
        want[0] = (size_t)nf * 2 * W * 8;
        want[1] = keep_bytes();
        want[2] = want[3] = want[4] = ((size_t)nf + 4) * 4;
    }
    // where the dense form keeps genome i's group numbers: in place of its per-window cache (stride 2), or -- no such cache,
    // or the genome's keys are a list -- in the run's own buffer
    uint2* dense_ci(kr_ctx* c, int i, u32& stride) const {
        Genome& G = c->genomes[ids[i]];
        if (c->wide.genome_cache && !G.wlist) { stride = 2u; return (uint2*)G.wkeys.p; }
        stride = 1u;
        return (uint2*)c->wide.cibuf.p + cioff[i];
    }
};

// A genome set whose sorted keys do not fit the device at once (KR_ERR_CAPACITY from a phase) is run again with the sort +
// intersect phases in batches of half as many genomes, and again, down to one genome per batch (KR_WIDE_BATCH=n in the
// environment starts there: tests) -- with the per-window cache of composite keys in one lane buffer instead of one per
// genome.  What must stay resident for the locate pass -- the genomes' bases (1 byte per base) and the group of every
// window (8 bytes per base) -- still bounds a run: beyond that the call fails with KR_ERR_CAPACITY, as before round 6.
// Several ranks retry together (one all-reduce behind every attempt: a rank must not enter the next attempt's exchanges alone).
int64_t kr_wide_run(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    if (!c || !c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params_wide first");
    const WideEnv env = wide_env();
    int B = (env.batch > 0 && env.batch < n) ? env.batch : n;
    c->wide.key_list_failed = false;
    for (;;) {
        c->wide.batch = B < n ? B : 0;
        WideRun run{ids, n, is_in, apply_filter, env};
        int64_t r = wide_run_once(c, run);
        double flag[2] = {r == KR_ERR_CAPACITY ? 1.0 : 0.0, (r < 0 && r != KR_ERR_CAPACITY && r != KR_ERR_STATE) ? 1.0 : 0.0};
        if (kr_comm_world(c) > 1) {
            const std::string mine = c->err;
            const int rca = kr_comm_allreduce(c, flag, 2, 1);
            c->err = mine;
            if (rca) return r < 0 ? r : rca;
        }
        if (flag[0] == 0.0 || flag[1] != 0.0 || B <= 1) return r;
        // (what the failed attempt holds goes back first: the genomes' sorted keys and per-window caches, the candidate buffers)
        (void)hipDeviceSynchronize();
        for (int i = 0; i < n; i++) {
            auto it = c->genomes.find(ids[i]);
            if (it == c->genomes.end()) continue;
            release(c, it->second.wkeys);
            genome_drop_sorted(c, it->second);
        }
        cands_drop(c);
        release(c, c->candP);
        release(c, c->other);
        c->err.clear();
        B = (B + 1) / 2;
    }
}

// the argument and state checks of an attempt
static int wide_check(kr_ctx* c, const int* ids, int n) {
    if (!c || !c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params_wide first");
    if (n < 1) return fail(c, KR_ERR_PARAM, "kr_wide_run: need at least one genome");
    for (int i = 0; i < n; i++) {
        auto it = c->genomes.find(ids[i]);
        if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", ids[i]);
    }
    return KR_OK;
}
// no result yet, no cache and no key list decided (the flank phases keep no per-window cache); the device table of
// flank dictionaries (Geom.wfl) exists
static int wide_run_begin(kr_ctx* c, const WideRun& r) {
    HIPCHK(c, hipSetDevice(c->device));
    auto& w = c->wide;
    w.nhits = -1;
    w.nfin = 0;
    w.run_ids.assign(r.ids, r.ids + r.n);
    w.genome_cache = false;
    w.key_list = false;
    w.keys_listed = 0;
    return ensure(c, w.flbuf, 8 * 2 * sizeof(FlankRank));
}

// ---- phases 1 / 2: the flanks ranked
// A spectrum phase: the `len` bases at forward offset fo (reverse strand: the reverse complement of the bases at
// k - fo - len) of every valid window -> the values present in all genomes, in w.fd[f][q]; returns their number.
// With both strands in play the spectrum is taken over EVERY valid flank-long window of the genome with the packed
// path's kernels (k_hist8 / k_scatter1p: 2.5 x the rate of the window-by-window generator): a superset of the
// flanks of the valid amplicon-long windows, closed under reverse complement.  The groups do not change -- a
// composite key present in every genome has its flanks at the ends of a valid window in every genome, so they
// are in the narrower dictionary as well -- and the ranks stay order-preserving.  The genomes' record counts
// (amplicon-long windows) then come from k_count_windows: the first such phase leaves them in w.nkeys (r.counted).
// Collectives: wide_phase's.
static int64_t spectrum_phase(kr_ctx* c, WideRun& r, int f, int q, int fo, int len) {
    auto& w = c->wide;
    Geom g = make_geom(len, 0, 0, w.omit, c->sb, c->g.b);
    const bool packed = w.packed_spectrum && w.strands == 0;
    g.wmode = packed ? 0 : 1;
    g.wk = w.k;
    g.wlen = len;
    g.wfo = fo;
    g.wro = w.k - fo - len;
    g.strands = w.strands;
    c->g = g;
    int cw = 0;
    if (packed && !r.counted) {
        int rcw = ensure(c, w.wcount, (size_t)r.n * 8 + 8);
        if (rcw) return rcw;
        HIPCHK(c, hipMemset(w.wcount.p, 0, (size_t)r.n * 8));
        cw = w.k;
    }
    // one spectrum for both flanks (w.share), taken over every flank-long window of both strands, one piece: the
    // dictionary keeps the canonical flanks only (Dict.canon; KR_WIDE_CANON=0: the full list, A/B and tests)
    const bool canon = r.env.canon && packed && w.share && kr_ctx::Wide::fd_pieces(f == 0 ? w.L : w.R) == 1;
    const int64_t nd = wide_phase(c, r.ids, r.n, r.is_in, w.fd[f][q], 2 * len, len, cw, canon);
    if (cw && nd >= 0) {
        std::vector<unsigned long long> wc(r.n);
        HIPCHK(c, hipMemcpy(wc.data(), w.wcount.p, (size_t)r.n * 8, hipMemcpyDeviceToHost));
        w.nkeys.clear();
        for (int i = 0; i < r.n; i++) w.nkeys.push_back(2ull * wc[i]);
        r.counted = true;
    }
    return nd;
}
// the rank of a flank (or piece) of one key through its dictionary w.fd[f][q]
static FlankRank one_level(const kr_ctx::Wide& w, int f, int q, int len) {
    FlankRank F{};
    F.len = F.plen[0] = len;
    F.poff[0] = 0;
    F.np = 1;
    F.d[0] = w.fd[f][q].view();
    return F;
}
// Composite geometry over two ranked parts: bit widths from the dictionary sizes, room for the slice digits.  The two
// parts' dictionaries go to the next pair of the device table (w.flslot; synchronous copy: the pair is in place before
// any launch that names it; the pair before stays for the kernels still reading it).
static Geom composite_geom(kr_ctx* c, const FlankRank& P0, u32 n0, int off0, const FlankRank& P1, u32 n1, int off1, int& bits) {
    auto& w = c->wide;
    int bits0 = std::max(1, ceil_log2((u64)n0 + 1)), bits1 = std::max(1, ceil_log2(n1));
    if ((bits0 + bits1) & 1) bits1++;
    while (bits0 + bits1 < 2 * c->sb + 2) bits1 += 2;
    bits = bits0 + bits1;
    Geom g = make_geom(bits / 2, 0, 0, w.omit, c->sb, c->g.b);
    g.wmode = 2;
    g.wk = w.k;
    g.wshL = 64 - bits0;
    g.wshR = 64 - bits0 - bits1;
    g.woff[0] = off0;
    g.woff[1] = off1;
    w.flslot = (w.flslot + 1) % 8;
    w.flhost[w.flslot][0] = P0;
    w.flhost[w.flslot][1] = P1;
    g.wfl = (const FlankRank*)w.flbuf.p + 2 * w.flslot;
    (void)hipMemcpy((void*)g.wfl, w.flhost[w.flslot], 2 * sizeof(FlankRank), hipMemcpyHostToDevice);
    g.strands = w.strands;
    return g;
}
// `left` and `right` ranked -- one spectrum each, or (longer than 32 bases) the spectrum of the first piece, the spectrum
// of the next and the combinations of their ranks, piece by piece (two sort + intersect phases per further piece); one
// spectrum serves both flanks where w.share says so (see Geom.wshare).  Leaves w.share, w.fd, w.fr and w.nkeys.
// Returns 1, an error, or 0 with w.nhits = 0: a dictionary is empty, so is the result.  Collectives: a wide_phase's per
// phase -- an empty dictionary is empty on every rank.
static int64_t flank_ranks(kr_ctx* c, WideRun& r) {
    auto& w = c->wide;
    typedef kr_ctx::Wide Wd;
    // (mixed DNA / RNA runs: a group and its mirror are no longer decided alike -- the column where one holds T against U holds
    // A against A in the other, the complement of both -- so every group is located and filtered by itself)
    w.share = !w.ordered && w.use_share && w.L == w.R && w.strands == 0 && !c->mixed_alphabets;
    for (int f = 0; f < (w.share ? 1 : 2); f++) {
        const int len = f == 0 ? w.L : w.R;
        const int fo = f == 0 ? 0 : w.k - w.R;              // forward offset of the flank in the window
        const int len1 = Wd::fd_plen(len, 0);
        int64_t nd = spectrum_phase(c, r, f, 0, fo, len1);
        if (nd < 0) return nd;
        if (f == 0 && !r.counted) {          // one key per strand of every valid window = the genome's k-mer records
            w.nkeys.clear();
            for (int i = 0; i < r.n; i++) w.nkeys.push_back(c->genomes[r.ids[i]].nmax);
        }
        if (nd == 0) { w.nhits = 0; return 0; }
        w.fr[f] = one_level(w, f, 0, len1);
        // longer than 32 bases: piece by piece -- the spectrum of piece j, then the combinations (rank of pieces 0 .. j - 1,
        // rank of piece j) present in every genome, ranked again
        u32 nsofar = w.fd[f][0].n;
        for (int j = 1; j < Wd::fd_pieces(len); j++) {
            const int lj = Wd::fd_plen(len, j), oj = Wd::fd_poff(len, j);
            if ((nd = spectrum_phase(c, r, f, 2 * j - 1, fo + oj, lj)) < 0) return nd;
            if (nd == 0) { w.nhits = 0; return 0; }
            int bits = 0;
            Geom g = composite_geom(c, w.fr[f], nsofar, fo, one_level(w, f, 2 * j - 1, lj), w.fd[f][2 * j - 1].n, fo + oj, bits);
            g.wcache = nullptr;
            c->g = g;
            if ((nd = wide_phase(c, r.ids, r.n, r.is_in, w.fd[f][2 * j], bits)) < 0) return nd;
            if (nd == 0) { w.nhits = 0; return 0; }
            FlankRank F = w.fr[f];
            F.len = oj + lj;
            F.np = j + 1;
            F.plen[j] = lj;
            F.poff[j] = oj;
            F.d[j] = w.fd[f][2 * j - 1].view();
            F.dc[j - 1] = w.fd[f][2 * j].view();
            F.sh1[j - 1] = g.wshL;
            F.sh2[j - 1] = g.wshR;
            w.fr[f] = F;
            nsofar = w.fd[f][2 * j].n;
        }
    }
    return 1;
}

// ---- phase 3: composite keys rank(left) : rank(right)
// Composite keys are generated once per genome and phase.  The keys as a LIST per genome (Geom.wlcnt) where few window
// starts have one -- both flanks in the dictionaries.  The canonical dictionary holds nfull flanks (both orientations) of
// a genome's 2 x bases flank occurrences: a share f of the starts has its left flank there, f^2 both if flanks went
// independently; conserved stretches cluster (2.2 x f^2 at configs[2]), so the segments are sized for 6 f^2 + 0.2 % --
// and a run whose genomes are close relatives (f -> 1) keeps 16 bytes per start: there most starts have a key.  A segment
// that turns out too short makes the run fall back by itself (phase_sort_intersect).  KR_WIDE_KEYLIST=0: dense (A/B,
// tests); KR_WIDE_KEYFRAC: the share to size for (tests: the fall-back).  Returns whether lists are meant; frac: the share.
static bool key_list_plan(kr_ctx* c, const WideRun& r, double& frac) {
    auto& w = c->wide;
    const FlankRank& F0 = w.fr[0];
    const bool canon_form = w.share && F0.np == 1 && F0.d[0].canon && w.k - F0.len <= H8W_HALO;     // (what k_hist8w's tiled form takes)
    u64 minb = ~0ull;
    for (int i = 0; i < r.n; i++) minb = std::min<u64>(minb, c->genomes[r.ids[i]].n_bases);
    const double f = std::min(1.0, (double)w.fd[0][kr_ctx::Wide::fd_last(w.L)].nfull / (2.0 * (double)std::max<u64>(minb, 1)));
    frac = r.env.has_keyfrac ? r.env.keyfrac : std::min(1.0, 6.0 * f * f + 0.002);
    return r.env.keylist && canon_form && !w.key_list_failed && frac <= 0.125;
}
// The keys are kept per genome (16 bytes per window start, or a list) when that fits comfortably -- the locate pass then
// reads them too and leaves each window's group in their place -- else in one lane buffer (sort passes only).  Reads
// w.key_list / w.key_list_frac; cache: whether per genome.  Where caches are still to be allocated (a first run) the
// candidate buffers of the flank phases go back -- they are dictionary-sized and the group phase sizes its own -- and,
// memory being short, the locate buffers of an earlier run.
static int key_cache_plan(kr_ctx* c, const WideRun& r, bool& cache) {
    auto& w = c->wide;
    size_t need = 0, slotbytes = 0;
    for (auto& flank : w.fd)
        for (auto& d : flank)      // (released once the composite keys exist)
            slotbytes += d.slots.bytes + (d.mzlen ? d.mzT.bytes + d.mzB.bytes : 0);
    for (int i = 0; i < r.n; i++) {       // what is still to be allocated (a repeated run has its caches)
        const Genome& G = c->genomes[r.ids[i]];
        const size_t want = w.key_list ? key_list_bytes(key_list_cap(G, w.key_list_frac)) : key_dense_bytes(G);
        need += bytes_missing(&want, &G.wkeys.bytes, 1);
    }
    if (need) {
        HIPCHK(c, hipDeviceSynchronize());
        cands_drop(c);
        int rc = wide_make_room(c, need * 5 / 2);
        if (rc) return rc;
    }
    const size_t fr = free_bytes();
    if (r.env.cache >= 0) cache = r.env.cache != 0;
    else cache = (!w.batch || w.key_list) && (need == 0 || need <= (fr + slotbytes) / 5 * 2);      // (batches: memory is short -- a list is small)
    return KR_OK;
}
// The list holds one group of every mirror pair (Geom.wshare): the (left,right) groups present in all genomes are twice
// as many, less the groups that mirror themselves -> w.ngroups
static int mirror_groups(kr_ctx* c, int64_t nf, const Geom& g) {
    auto& w = c->wide;
    if (nf >= (1ll << 31)) return fail(c, KR_ERR_CAPACITY, "wide path: %lld canonical groups (>= 2^31)", (long long)nf);
    u32 npal = 0;
    int rc = ensure(c, w.tsum, 64);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(w.tsum.p, 0, 4, c->stream));
    hipLaunchKernelGGL(k_count_selfmirror, dim3(((u32)nf + 255) / 256), dim3(256), 0, c->stream, (const u64*)w.fin.keys.p,
                       (u32)nf, g.wshL, g.wshR, g.wshL - g.wshR, (u32*)w.tsum.p);
    HIPCHK(c, hipMemcpyAsync(&npal, w.tsum.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    w.ngroups = 2 * (u64)nf - npal;
    return KR_OK;
}
// Reads w.fr / w.fd of flank_ranks; leaves the groups present in all genomes in w.fin (w.nfin, w.ngroups), c->g the
// composite geometry, and the run's two memory decisions: w.key_list (+ w.key_list_frac) and w.genome_cache (one cache
// for all genomes: one sort lane for the rest of the run, w.lanes).  Returns the groups' number, an error, or 0 with
// w.nhits = 0.  Collectives: one wide_phase's.
static int64_t group_phase(kr_ctx* c, WideRun& r) {
    auto& w = c->wide;
    int rc;
    // (a canonical dictionary of n keys hands out ids below 2 n)
    auto ids_of = [](const kr_ctx::Wide::DictBufs& dd) { return dd.canon ? 2u * dd.n : dd.n; };
    const u32 nL = ids_of(w.fd[0][kr_ctx::Wide::fd_last(w.L)]), nR = w.share ? nL : ids_of(w.fd[1][kr_ctx::Wide::fd_last(w.R)]);
    int bits = 0;
    Geom g = composite_geom(c, w.fr[0], nL, 0, w.share ? w.fr[0] : w.fr[1], nR, w.k - w.R, bits);
    g.wshare = w.share ? 1 : 0;
    w.genome_cache = false;
    w.key_list = key_list_plan(c, r, w.key_list_frac);
    bool cache = false;
    if ((rc = key_cache_plan(c, r, cache))) return rc;
    w.genome_cache = cache;
    if (!w.genome_cache) {
        w.key_list = false;            // (ONE cache for all genomes: the dense form)
        w.lanes = 1;          // (ONE cache of composite keys, in lane 0's scratch: one lane for the rest of this run)
        if ((rc = ensure(c, c->lanes[0].wkeys, ((c->max_bases + 31) / 32 + PAD_WORDS) * 32 * 16))) return rc;
        g.wcache = (u64*)c->lanes[0].wkeys.p;
    }
    c->g = g;
    const int64_t nf = wide_phase(c, r.ids, r.n, r.is_in, w.fin, bits);
    if (nf < 0) return nf;
    w.nfin = (u32)nf;
    w.ngroups = (u64)nf;
    if (w.share && nf && (rc = mirror_groups(c, nf, g))) return rc;
    if (nf == 0) w.nhits = 0;
    return nf;
}

// ---- members of the groups: masks + counts, filter, hits
// What the locate / count / emit passes need and what of it is still to be allocated -> r (see WideRun).  The member
// windows as a LIST when that is the smaller thing to write and read (k_wide_locate): room for two members per group and
// genome (more -- repeats -- : the dense form runs after all, locate_overflow); KR_WIDE_LOCLIST=0: dense (A/B, tests),
// KR_WIDE_LOCCAP: the list's room in entries (tests: the overflow).
static void locate_plan(kr_ctx* c, WideRun& r) {
    auto& w = c->wide;
    const int n = r.n;
    r.nf = w.nfin;
    r.W = std::max(1, w.W);
    r.kwords = (size_t)r.nf / 64 + 2;
    r.ksum_off = (r.kwords + 63) / 64 * 64;
    // the group of every window of every genome (8 bytes per base): written by the locate pass,
    // streamed by the emit pass once the filter has decided
    r.cioff.assign(n + 1, 0);
    for (int i = 0; i < n; i++) r.cioff[i + 1] = r.cioff[i] + c->genomes[r.ids[i]].n_bases;
    for (int i = 0; i < n; i++) r.any_wlist = r.any_wlist || (w.genome_cache && c->genomes[r.ids[i]].wlist);
    size_t want[5];
    r.sizes(want);
    const size_t have[] = {w.masks.bytes, w.keep.bytes, w.cnt.bytes, w.hitoff.bytes, w.cursor.bytes};
    size_t need = bytes_missing(want, have, 5);
    const u64 npos_all = r.cioff[n];
    r.loc_cap = r.env.loccap ? r.env.loccap : 2 * (u64)r.nf * (u64)n + (1u << 20);
    r.loc_cap = r.loc_cap / WIDE_SEGS * WIDE_SEGS;                  // (WIDE_SEGS lists of loc_cap / WIDE_SEGS entries)
    r.use_list = r.env.loclist && r.loc_cap < (1ull << 31) && (r.env.loccap || r.loc_cap * 16 <= npos_all * 4 + ((u64)64 << 20));
    if (r.use_list) {
        // the list lives for the locate / count / emit passes only, when every sort of the run is over: the first sort
        // lane's pass-0 or pass-1 scratch holds it when large enough (configs[2]: 0.8 GB in an idle 8 GB array -- a
        // buffer of its own would push a run planned to the device's last GB into giving memory back every time)
        Lane& l0 = c->lanes[0];
        const size_t lb = r.list_bytes();
        r.loc_borrow = l0.pass0.bytes >= lb ? &l0.pass0 : (l0.tmpkeys.bytes >= lb ? &l0.tmpkeys : nullptr);
        if (!r.loc_borrow) need += bytes_missing(&lb, &w.loc.bytes, 1);
    }
    if (!w.genome_cache && !r.use_list) {
        const size_t ci = r.cibuf_bytes();
        need += bytes_missing(&ci, &w.cibuf.bytes, 1);
    }
    r.loc_need = need;
}
// When r.loc_need does not fit beside a margin, memory goes back in three steps, each only if the one before was not
// enough: the flank dictionaries' look-up tables (with the composite keys of every window cached they have done their
// work; the device pair of Geom.wfl forgets them), then the candidate buffers, then the genomes' sorted composite keys.
static int locate_make_room(kr_ctx* c, const WideRun& r) {
    auto& w = c->wide;
    const size_t need = r.loc_need, margin = (size_t)2 << 30;
    if (!need || free_bytes() >= need + margin) return KR_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (w.genome_cache) {
        for (int f = 0; f < 2; f++) {
            for (auto& d : w.fd[f]) {
                release(c, d.slots);
                if (d.mzlen) { release(c, d.mzT); release(c, d.mzB); release(c, d.idx); }
            }
            if (c->g.wfl) {
                FlankRank* hf = &w.flhost[w.flslot][f];
                for (int q = 0; q < FR_MAXP; q++) hf->d[q].slots = nullptr, hf->d[q].mzT = nullptr;
                for (int q = 0; q < FR_MAXP - 1; q++) hf->dc[q].slots = nullptr, hf->dc[q].mzT = nullptr;
            }
        }
        if (c->g.wfl)       // (the device was synchronised above: nobody reads the pair)
            HIPCHK(c, hipMemcpy((void*)c->g.wfl, w.flhost[w.flslot], 2 * sizeof(FlankRank), hipMemcpyHostToDevice));
    }
    if (free_bytes() < need + margin) cands_drop(c);
    if (free_bytes() < need + margin)
        for (int i = 0; i < r.n; i++) genome_drop_sorted(c, c->genomes[r.ids[i]]);
    return KR_OK;
}
// The passes' buffers exist and are cleared on c->stream, which waits for the sort lanes.  The caller puts the answer to
// wide_agree: all ranks or none go on to the exchange.
static int locate_buffers(kr_ctx* c, const WideRun& r) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    int rc;
    size_t want[5];
    r.sizes(want);
    DevBuf* bufs[5] = {&w.masks, &w.keep, &w.cnt, &w.hitoff, &w.cursor};
    for (int q = 0; q < 5; q++)
        if ((rc = ensure(c, *bufs[q], want[q]))) return rc;
    if ((rc = join_lanes(c))) return rc;
    HIPCHK(c, hipMemsetAsync(w.masks.p, 0, want[0], st));
    HIPCHK(c, hipMemsetAsync(w.cnt.p, 0, want[2], st));
    HIPCHK(c, hipMemsetAsync((u64*)w.keep.p + r.ksum_off, 0, (r.kwords / 64 + 2) * 8, st));
    HIPCHK(c, hipMemsetAsync(w.cursor.p, 0, want[4], st));
    if (r.use_list) {
        if (!r.loc_borrow && (rc = ensure(c, w.loc, r.list_bytes()))) return rc;
        if ((rc = ensure(c, w.loccur, WIDE_SEGS * WIDE_SEG_STRIDE * 4))) return rc;
        HIPCHK(c, hipMemsetAsync(w.loccur.p, 0, WIDE_SEGS * WIDE_SEG_STRIDE * 4, st));
    } else if ((!w.genome_cache || r.any_wlist) && (rc = ensure(c, w.cibuf, r.cibuf_bytes()))) return rc;
    return KR_OK;
}
static u32 wide_grid(const Genome& G) { return (u32)std::min<u64>((G.n_bases + 255) / 256, 16384); }
// k_wide_locate over genome G, its codes in lane ln: the member windows to the list (list) or their groups to ci
static void launch_wide_locate(bool list, kr_ctx* c, const WideRun& r, const Genome& G, const Lane& ln, const Geom& g, u32 side,
                               uint2* ci, u32 stride, uint4* locp, u32 gidx) {
    auto& w = c->wide;
    auto kernel = list ? k_wide_locate<true> : k_wide_locate<false>;
    hipLaunchKernelGGL(kernel, dim3(wide_grid(G)), dim3(256), 0, c->stream, (const u64*)ln.codes.p, (const u32*)ln.bad.p,
                       (u64)G.n_bases, g, w.fin.view(), w.D, r.W, side, (u64*)w.masks.p, ci, stride, locp, (u32*)w.loccur.p,
                       r.seg_cap(), gidx);
}
// The locate pass over every genome, in the form r.use_list says: the groups' masks gain the genomes' columns (w.masks)
// and the member windows go to the list, or the group of every window start to dense_ci().
static void locate_all(kr_ctx* c, const WideRun& r) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    Lane& ln = c->lanes[0];
    const int world = kr_comm_world(c);
    for (int i = 0; i < r.n; i++) {
        Genome& G = c->genomes[r.ids[i]];
        if (G.n_bases == 0) continue;
        launch_pack(c, G, ln, st);
        Geom g = c->g;
        g.wcmode = 0;
        g.wcache = nullptr;
        g.wlcnt = nullptr;
        g.wlcap = 0;
        u32 stride = 1;
        uint2* ci = r.dense_ci(c, i, stride);
        if (w.genome_cache && !G.wlist) {
            g.wcache = (u64*)G.wkeys.p;
            g.wcmode = 2;
        }
        uint4* locp = r.use_list ? r.list(w) : (uint4*)nullptr;
        const u32 side = r.is_in[i] ? 0u : 1u;
        const u32 gidx = world > 1 ? (u32)r.ids[i] : (u32)i;      // (several ranks: a hit names its genome by the caller's id, the lists of all ranks meet on rank 0)
        StageScope sc(c, KR_ST_LOCATE, st);
        if (G.wlist && r.use_list) {
            // the genome's keys are a list (Geom.wlcnt): the locate pass walks it
            g.wcache = (u64*)G.wkeys.p;
            g.wlcnt = (u32*)G.wlcnt.p;
            g.wlcap = G.wlcap;
            g.wcmode = 4;
            hipLaunchKernelGGL(k_wide_locate_list, dim3(NWG), dim3(256), 0, st, (const u64*)ln.codes.p, g, w.fin.view(), w.D, r.W,
                               side, (u64*)w.masks.p, locp, (u32*)w.loccur.p, r.seg_cap(), gidx);
            continue;
        }
        // (a key-list genome in a run whose members are too many to list: its keys are made again, window by window)
        launch_wide_locate(r.use_list, c, r, G, ln, g, side, ci, stride, locp, gidx);
    }
}
// How many members were listed -> r.nloc, w.located.  More than the list holds (a genome set full of repeats): the dense
// form, from the start (the masks only gain bits they already have) -- r.use_list is cleared.  rcd: whether the dense
// form's buffer could be had, for the caller's wide_agree (several ranks: every rank comes there once, whichever form
// its own genomes took -- the forms are chosen rank by rank); the return value: a failure of the device.
static int locate_overflow(kr_ctx* c, WideRun& r, int& rcd) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    rcd = KR_OK;
    r.nloc = 0;
    w.located = 0;
    if (!r.use_list) return KR_OK;
    std::vector<u32> cur(WIDE_SEGS * WIDE_SEG_STRIDE);
    HIPCHK(c, hipMemcpyAsync(cur.data(), w.loccur.p, cur.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    bool over = false;
    u64 sum = 0;
    for (u32 sg = 0; sg < WIDE_SEGS; sg++) {
        over = over || cur[sg * WIDE_SEG_STRIDE] > r.loc_cap / WIDE_SEGS;
        sum += cur[sg * WIDE_SEG_STRIDE];
    }
    r.nloc = (u32)std::min<u64>(sum, 0xFFFFFFFFu);
    if (over) {
        r.use_list = false;
        r.nloc = 0;
        if (!w.genome_cache || r.any_wlist) rcd = ensure(c, w.cibuf, r.cibuf_bytes());
        if (!rcd) locate_all(c, r);
    }
    w.located = r.nloc;
    return KR_OK;
}

// the kept groups of this rank (w.keep) -> candidate records in c->candB with mask word wd; returns their number
// (w.hitoff is scratch here: free until the scan of the member counts)
static int64_t pack_list(kr_ctx* c, const WideRun& r, int wd) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    const u32 nwords = (r.nf + 63) / 64;
    u32* po = (u32*)w.hitoff.p;
    int rc;
    hipLaunchKernelGGL(k_keep_popc, dim3((nwords + 255) / 256), dim3(256), 0, st, (const u64*)w.keep.p, nwords, po);
    if ((rc = excl_scan_tiles(c, st, po, nwords, po))) return rc;
    u32 ns = 0;
    HIPCHK(c, hipMemcpyAsync(&ns, po + nwords, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if ((rc = ensure(c, c->candB, ((size_t)ns + 2) * sizeof(kr_cand)))) return rc;
    if ((rc = ensure(c, c->candA, ((size_t)ns + 2) * sizeof(kr_cand)))) return rc;
    hipLaunchKernelGGL(k_wide_pack, dim3((nwords + 255) / 256), dim3(256), 0, st, (const u64*)w.keep.p, (const u32*)po,
                       nwords, (const u64*)w.masks.p, r.W, wd, (kr_cand*)c->candB.p);
    c->ncand = ns;
    return ns;
}
// Several ranks, filtered: the masks hold this rank's genomes only.  The filter is monotone (masks only grow), so a
// group this rank drops is dropped for good; the groups it keeps travel with their mask words, one 16-column word per
// round, through the candidate tree reduction (intersection of the ranks' kept sets, masks OR-ed); rank 0 then filters
// on the complete masks and broadcasts the survivors -> w.keep on every rank.
// Collectives: per mask word wide_agree (all ranks enter the reduction, or none) and kr_cands_reduce; then kr_cands_bcast.
static int wide_filter_ranks(kr_ctx* c, const WideRun& r) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    const int rank = kr_comm_rank(c);
    int rc;
    int64_t ns = 0;
    for (int wd = 0; wd < r.W; wd++) {
        ns = pack_list(c, r, wd);
        if ((rc = wide_agree(c, ns < 0 ? (int)ns : KR_OK))) return rc;
        if ((ns = kr_cands_reduce(c, 0)) < 0) return (int)ns;
        if (rank == 0 && ns)
            hipLaunchKernelGGL(k_wide_unpack, dim3(((u32)ns + 255) / 256), dim3(256), 0, st, (const kr_cand*)c->candB.p,
                               (u32)ns, (u64*)w.masks.p, r.W, wd);
    }
    // the survivors in c->candB -> keep bits: rank 0 filters them on the complete masks, the others take its list
    auto relist = [&](int mode) -> int {
        HIPCHK(c, hipMemsetAsync(w.keep.p, 0, r.keep_bytes(), st));
        if (ns)
            hipLaunchKernelGGL(k_wide_relist, dim3(((u32)ns + 255) / 256), dim3(256), 0, st, (const kr_cand*)c->candB.p,
                               (u32)ns, (const u64*)w.masks.p, w.D, r.W, mode, (u64*)w.keep.p, (u64*)w.keep.p + r.ksum_off);
        return KR_OK;
    };
    if (rank == 0) {
        if ((rc = relist(fmode(c, 1)))) return rc;
        if ((ns = pack_list(c, r, 0)) < 0) c->ncand = -1;                         // (the broadcast's agreement tells the others)
    }
    if ((ns = kr_cands_bcast(c)) < 0) return (int)ns;
    if (rank != 0 && (rc = relist(0))) return rc;
    return KR_OK;
}
// the filter over the groups' masks -> the keep bits and their summary (w.keep); several ranks: over all ranks' genomes
static int wide_filter(kr_ctx* c, const WideRun& r) {
    auto& w = c->wide;
    hipLaunchKernelGGL(k_wide_filter, dim3((r.nf + 255) / 256), dim3(256), 0, c->stream, (const u64*)w.masks.p, (u64*)w.keep.p,
                       (u64*)w.keep.p + r.ksum_off, r.nf, w.D, r.W, fmode(c, r.apply_filter));
    return kr_comm_world(c) > 1 && r.apply_filter ? wide_filter_ranks(c, r) : KR_OK;
}
// Members per kept group (the list, or the windows' groups, streamed again; only kept groups are counted) -> w.cnt, their
// exclusive scan -> w.hitoff, the total -> w.nhits and `total`.
static int count_members(kr_ctx* c, const WideRun& r, u32& total) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    const u64 *keep = (const u64*)w.keep.p, *ksum = keep + r.ksum_off;
    int rc;
    if (r.use_list && r.nloc)
        hipLaunchKernelGGL(k_wide_count_list, dim3((r.seg_cap() + 255) / 256, WIDE_SEGS), dim3(256), 0, st, (const uint4*)r.list(w),
                           (const u32*)w.loccur.p, r.seg_cap(), keep, ksum, (u32*)w.cnt.p, w.share ? 1 : 0);
    for (int i = 0; i < r.n && !r.use_list; i++) {
        Genome& G = c->genomes[r.ids[i]];
        if (G.n_bases == 0) continue;
        u32 stride = 1;
        const uint2* ci = r.dense_ci(c, i, stride);
        hipLaunchKernelGGL(k_wide_count, dim3(wide_grid(G)), dim3(256), 0, st, ci, stride, (u64)G.n_bases, keep, ksum,
                           (u32*)w.cnt.p, w.share ? 1 : 0);
    }
    if ((rc = excl_scan_tiles(c, st, (const u32*)w.cnt.p, r.nf, (u32*)w.hitoff.p))) return rc;
    total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, (u32*)w.hitoff.p + r.nf, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    w.nhits = total;
    return KR_OK;
}
// the members of the kept groups -> w.hits, `total` of them, each group's together (w.hitoff, w.cursor)
static int emit_members(kr_ctx* c, const WideRun& r, u32 total) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    const u64 *keep = (const u64*)w.keep.p, *ksum = keep + r.ksum_off;
    const int world = kr_comm_world(c);
    int rc;
    if ((rc = ensure(c, w.hits, ((size_t)total + 2) * sizeof(wide_hit)))) return rc;
    if (r.use_list && r.nloc && total)
        hipLaunchKernelGGL(k_wide_emit_list, dim3((r.seg_cap() + 255) / 256, WIDE_SEGS), dim3(256), 0, st, (const uint4*)r.list(w),
                           (const u32*)w.loccur.p, r.seg_cap(), keep, ksum, (const u32*)w.hitoff.p, (u32*)w.cursor.p,
                           (wide_hit*)w.hits.p, w.share ? 1 : 0);
    for (int i = 0; i < r.n && total && !r.use_list; i++) {
        Genome& G = c->genomes[r.ids[i]];
        if (G.n_bases == 0) continue;
        u32 stride = 1;
        const uint2* ci = r.dense_ci(c, i, stride);
        // (several ranks: a hit names its genome by the caller's id, the lists of all ranks meet on rank 0)
        hipLaunchKernelGGL(k_wide_emit, dim3(wide_grid(G)), dim3(256), 0, st, ci, stride, (u64)G.n_bases,
                           world > 1 ? (u32)r.ids[i] : (u32)i, keep, ksum, (const u32*)w.hitoff.p, (u32*)w.cursor.p,
                           (wide_hit*)w.hits.p, w.share ? 1 : 0);
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return KR_OK;
}
// Several ranks: the hits of every rank -> rank 0's w.hits / w.nhits, through the record gather (a hit is 16 bytes, as a
// record is).  Collective: kr_records_gather.  Returns this rank's w.nhits.
static int64_t gather_hits(kr_ctx* c, u32 total) {
    auto& w = c->wide;
    hipStream_t st = c->stream;
    int rc;
    static_assert(sizeof(wide_hit) == sizeof(kr_record), "hits travel as records");
    if ((rc = ensure(c, c->records, ((size_t)total + 2) * sizeof(kr_record)))) return rc;
    if (total) HIPCHK(c, hipMemcpyAsync(c->records.p, w.hits.p, (size_t)total * sizeof(wide_hit), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->nrecords = total;
    const int64_t all = kr_records_gather(c);
    if (all < 0) return all;
    if (kr_comm_rank(c) == 0) {
        if ((rc = ensure(c, w.hits, ((size_t)all + 2) * sizeof(wide_hit)))) return rc;
        if (all) HIPCHK(c, hipMemcpy(w.hits.p, c->records.p, (size_t)all * sizeof(wide_hit), hipMemcpyDeviceToDevice));
        w.nhits = all;
    }
    c->nrecords = 0;
    return w.nhits;
}

// One attempt of kr_wide_run with the sort + intersect phases in batches of w.batch genomes: returns the number of hits
// (w.nhits; the results in c->wide) or an error.
// The collectives, in order, which every rank reaches alike or not at all -- a return between two of them is either
// behind a wide_agree that told all ranks, or the same on all ranks (an empty dictionary), or a failure of this rank's
// device or allocator that the peers learn at the next agreement:
//   per sort + intersect phase (flank_ranks: one per spectrum, one per combination; group_phase: one):
//       wide_agree, then with several ranks kr_cands_reduce, kr_cands_bcast
//   wide_agree on locate_buffers; wide_agree on locate_overflow's dense buffer
//   several ranks, filtered (wide_filter_ranks): per mask word wide_agree, kr_cands_reduce; then kr_cands_bcast
//   several ranks (gather_hits): kr_records_gather -- also with no hits on this rank
//   kr_wide_run: the retry all-reduce behind every attempt
static int64_t wide_run_once(kr_ctx* c, WideRun& r) {
    int rc;
    if ((rc = wide_check(c, r.ids, r.n))) return rc;
    auto& w = c->wide;
    struct LanesBack { kr_ctx::Wide& w; int lanes; ~LanesBack() { w.lanes = lanes; } } lanes_back{w, w.lanes};
    if ((rc = wide_run_begin(c, r))) return rc;
    int64_t nd;
    if ((nd = flank_ranks(c, r)) <= 0) return nd;           // (an error, or no flank in all genomes: no hits)
    if ((nd = group_phase(c, r)) <= 0) return nd;           // (an error, or no group in all genomes: no hits)
    locate_plan(c, r);
    if ((rc = locate_make_room(c, r))) return rc;
    if ((rc = wide_agree(c, locate_buffers(c, r)))) return rc;      // (several ranks: all or none go on to the exchange)
    locate_all(c, r);
    int rcd = KR_OK;
    if ((rc = locate_overflow(c, r, rcd))) return rc;
    if ((rc = wide_agree(c, rcd))) return rc;
    if ((rc = wide_filter(c, r))) return rc;
    u32 total = 0;
    if ((rc = count_members(c, r, total))) return rc;
    if (total == 0 && kr_comm_world(c) == 1) return 0;
    if ((rc = emit_members(c, r, total))) return rc;
    return kr_comm_world(c) > 1 ? gather_hits(c, total) : w.nhits;
}

int64_t kr_wide_fetch_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    if (!c || !c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params_wide first");
    auto& w = c->wide;
    if (w.nhits < 0) return fail(c, KR_ERR_STATE, "kr_wide_run first");
    if (kr_comm_world(c) > 1) return fail(c, KR_ERR_STATE, "kr_wide_fetch_windows: hits of other ranks' genomes have no bases here");
    const u64 nh = (u64)w.nhits, k = (u64)w.k, total = nh * k;
    if (!rows) return (int64_t)nh;
    if (total > cap_bytes) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch_windows: buffer too small (%llu bytes needed)", (unsigned long long)total);
    if (nh == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    std::vector<const uint8_t*> tab;
    for (int id : w.run_ids) {
        auto it = c->genomes.find(id);
        if (it == c->genomes.end() || !it->second.bases.p) return fail(c, KR_ERR_STATE, "kr_wide_fetch_windows: genome %d was freed", id);
        tab.push_back((const uint8_t*)it->second.bases.p);
    }
    if ((rc = ensure(c, w.rowtab, tab.size() * 8 + 16))) return rc;
    // (rows in pieces of <= 1 GiB: the text of 10^7 windows of 124 letters need not sit in HBM at once)
    const u64 piece = std::max<u64>(1, ((u64)1 << 30) / k);
    if ((rc = ensure(c, w.rows, std::min(nh, piece) * k))) return rc;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(w.rowtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
    for (u64 h0 = 0; h0 < nh; h0 += piece) {
        const u64 m = std::min(piece, nh - h0), bytes = m * k;
        hipLaunchKernelGGL(k_wide_cut, dim3((u32)((bytes + 255) / 256)), dim3(256), 0, st, (const wide_hit*)w.hits.p + h0, bytes,
                           (u32)k, (const uint8_t* const*)w.rowtab.p, (u32)tab.size(), (uint8_t*)w.rows.p);
        HIPCHK(c, hipMemcpyAsync(rows + h0 * k, w.rows.p, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    HIPCHK(c, hipGetLastError());
    return (int64_t)nh;
}

// the reverse complement of a flank of `len` bases held in the top 2 len bits: complement, then reverse the 2-bit groups
static u64 flank_revcomp(u64 x, int len) {
    u64 y = ~x;
    y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
    y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(y) << (64 - 2 * len);
}
// kr_wide_fetch of one number
static int64_t fetch_u64(kr_ctx* c, void* out, size_t cap_bytes, u64 v) {
    if (!out) return 1;
    if (cap_bytes < 8) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (8 bytes needed)");
    memcpy(out, &v, 8);
    return 1;
}

int64_t kr_wide_fetch(kr_ctx* c, int what, void* out, size_t cap_bytes) {
    if (!c || !c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params_wide first");
    HIPCHK(c, hipSetDevice(c->device));
    auto& w = c->wide;
    const void* src = nullptr;
    size_t n = 0, esz = 8;
    // a canonical dictionary (Dict.canon) stands for its keys AND their reverse complements: the full list is made here on
    // request (the spectrum is closed under reverse complement, so `left` and the mirrored `right` are the same set)
    auto full_of_canonical = [&](const kr_ctx::Wide::DictBufs& d, int len) -> int64_t {
        const size_t nf = d.nfull;
        if (!out) return (int64_t)nf;
        if (nf * 8 > cap_bytes) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (%zu bytes needed)", nf * 8);
        std::vector<u64> v(d.n);
        HIPCHK(c, hipDeviceSynchronize());
        if (d.n) HIPCHK(c, hipMemcpy(v.data(), d.keys.p, (size_t)d.n * 8, hipMemcpyDeviceToHost));
        std::vector<u64> all(v);
        for (u64 x : v)
            if (flank_revcomp(x, len) != x) all.push_back(flank_revcomp(x, len));
        std::sort(all.begin(), all.end());
        if (all.size() != nf) return fail(c, KR_ERR_STATE, "kr_wide_fetch: canonical dictionary of %u keys expands to %zu, not %zu", d.n, all.size(), nf);
        memcpy(out, all.data(), nf * 8);
        return (int64_t)nf;
    };
    if ((what == KR_WIDE_DICT_LEFT || (what == KR_WIDE_DICT_RIGHT && w.share)) && w.fd[0][0].canon && kr_ctx::Wide::fd_pieces(w.L) == 1)
        return full_of_canonical(w.fd[0][0], w.L);
    switch (what) {
    case KR_WIDE_DICT_LEFT: src = w.fd[0][kr_ctx::Wide::fd_last(w.L)].keys.p; n = w.fd[0][kr_ctx::Wide::fd_last(w.L)].n; break;
    case KR_WIDE_DICT_RIGHT:
        if (w.share) {
            // never built (Geom.wshare): for flanks of one key it is the reverse complement of the left
            // dictionary, made here on request; for longer flanks only its size is reported
            n = w.fd[0][kr_ctx::Wide::fd_last(w.L)].n;
            if (!out) return (int64_t)n;
            if (w.L > 32) return fail(c, KR_ERR_STATE, "kr_wide_fetch: the right dictionary of flanks longer than 32 bases is not "
                                                        "materialised when it mirrors the left one (KR_OPT_WIDE_ORDERED = 1 builds it)");
            if (n * 8 > cap_bytes) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (%zu bytes needed)", n * 8);
            HIPCHK(c, hipDeviceSynchronize());
            u64* o = (u64*)out;
            if (n) HIPCHK(c, hipMemcpy(o, w.fd[0][0].keys.p, n * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) o[i] = flank_revcomp(o[i], w.L);
            std::sort(o, o + n);
            return (int64_t)n;
        }
        src = w.fd[1][kr_ctx::Wide::fd_last(w.R)].keys.p; n = w.fd[1][kr_ctx::Wide::fd_last(w.R)].n; break;
    case KR_WIDE_GROUPS: src = w.fin.keys.p; n = w.nfin; break;
    case KR_WIDE_HITS: src = w.hits.p; n = w.nhits > 0 ? (size_t)w.nhits : 0; esz = sizeof(wide_hit); break;
    case KR_WIDE_COUNTS:
        n = w.nkeys.size();
        if (!out) return (int64_t)n;
        if (n * 8 > cap_bytes) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (%zu bytes needed)", n * 8);
        memcpy(out, w.nkeys.data(), n * 8);
        return (int64_t)n;
    case KR_WIDE_BATCH_USED: return fetch_u64(c, out, cap_bytes, (u64)w.batch);
    case KR_WIDE_KEYS_LISTED: return fetch_u64(c, out, cap_bytes, w.keys_listed);
    case KR_WIDE_LOCATED: return fetch_u64(c, out, cap_bytes, w.located);
    case KR_WIDE_NGROUPS: return fetch_u64(c, out, cap_bytes, w.ngroups);
    case KR_WIDE_SLOT_BITS: {
        u64 v[7];
        for (int f = 0; f < 2; f++)
            for (int q = 0; q < 3; q++) v[3 * f + q] = (f == 1 && w.share) ? 254u : (w.fd[f][q].mzlen ? 255u : (u64)w.fd[f][q].sb);
        v[6] = (u64)w.fin.sb;
        if (!out) return 7;
        if (cap_bytes < sizeof v) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (%zu bytes needed)", sizeof v);
        memcpy(out, v, sizeof v);
        return 7;
    }
    default: return fail(c, KR_ERR_PARAM, "kr_wide_fetch: unknown selector %d", what);
    }
    if (!out) return (int64_t)n;       // size query
    if (n * esz > cap_bytes) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (%zu bytes needed)", n * esz);
    HIPCHK(c, hipDeviceSynchronize());
    if (n) HIPCHK(c, hipMemcpy(out, src, n * esz, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

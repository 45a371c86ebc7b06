// h_intersect.inc -- part of krisp_hip.hip (one translation unit): host: kr_intersect, candidate lists, kr_collect / kr_fetch
static int64_t intersect_once(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter, bool* redo);

static int64_t cands_merge_device(kr_ctx* c, size_t m, int have_other, int apply_filter);

// candidate lists are indexed with 32 bits on the device (flags, block scans, the pair index of kr_collect): a longer list --
// possible where nothing prunes: one side only, no filter, genomes of > 2e9 bases -- is refused, never truncated (ADVICE r5)
// the filter argument of the kernels: 0 none, 1 the reference's, 2 its superset for runs that mix DNA and RNA genomes
static inline int fmode(const kr_ctx* c, int apply_filter) { return apply_filter ? (c->mixed_alphabets ? 2 : 1) : 0; }

int kr_set_mixed_alphabets(kr_ctx* c, int on) {
    if (!c) return KR_ERR_PARAM;
    c->mixed_alphabets = on != 0;
    return KR_OK;
}

#define KR_MAX_CANDS 0xFFFFFF00ull
static int cands_fit(kr_ctx* c, uint64_t n, const char* who) {
    if (n < KR_MAX_CANDS) return KR_OK;
    return fail(c, KR_ERR_CAPACITY, "%s: a candidate list of %llu entries exceeds the %llu a list may hold (an intersection that "
                "nothing prunes: give both ingroup and outgroup genomes to one call, or fewer genomes per call)", who,
                (unsigned long long)n, (unsigned long long)KR_MAX_CANDS);
}

// The compaction of the live list (the n candidates in candB), shared by every site that prunes it.  The site's own flag
// kernel leaves a keep flag per candidate in `flags` and the count of each block of 256 in `blockcnt`; k_scan places the
// blocks, k_cands_compact writes the kept candidates to candA, and the site adopts candA once its own synchronisation has
// brought the total to the host.  cands_compact_room: the scratch and the target for n candidates.
static int cands_compact_room(kr_ctx* c, u32 n) {
    const size_t nblk = ((size_t)n + 255) / 256;
    int rc;
    if ((rc = ensure(c, c->flags, (size_t)n * 4))) return rc;
    if ((rc = ensure(c, c->blockcnt, (nblk + 2) * 4))) return rc;
    if ((rc = ensure(c, c->blockpos, (nblk + 2) * 4))) return rc;
    return ensure(c, c->candA, ((size_t)n + 2) * sizeof(kr_cand));
}
// behind the flag kernel on `st`; returns where the total lies on the device (publish: also sent to mbox[16])
static const u32* cands_compact_enqueue(kr_ctx* c, u32 n, hipStream_t st, bool publish) {
    const u32 nblk = (n + 255) / 256;
    const u32* total = (const u32*)c->blockpos.p + nblk;
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)c->blockcnt.p, (u32*)c->blockpos.p, nblk);
    hipLaunchKernelGGL(k_cands_compact, dim3(nblk), dim3(256), 0, st, (const kr_cand*)c->candB.p, n,
                       (const u32*)c->flags.p, (const u32*)c->blockpos.p, (kr_cand*)c->candA.p);
    if (publish)
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, total, (const u32*)nullptr, (const u32*)nullptr, c->mbox + 16);
    return total;
}
static int64_t cands_compact_adopt(kr_ctx* c, u32 total) {
    std::swap(c->candA, c->candB);
    c->ncand = total;
    return total;
}

static int64_t intersect_batch(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    bool redo = false;
    int64_t r = intersect_once(c, ids, n, is_in, apply_filter, &redo);
    if (r >= 0 && redo) r = intersect_once(c, ids, n, is_in, apply_filter, &redo);     // (the sorts are final now)
    return r;
}

// More than MAXG genomes (the presence word of a prefix has 32 bits): batches of MAXG, each batch's candidates
// intersected with the running list ON THE DEVICE (k_cands_flag / k_cands_compact: list (x) list, masks OR-ed) -- the
// running list never leaves HBM --, the diagnostic filter once at the end (it needs every genome's masks).
// Coarse genomes among the arguments (kr_genome_partition).  The sorted genomes of the call -- the "pillars": at least one
// ingroup and one outgroup genome -- are intersected as ever, filter on: the list C, about 1 % of a genome's prefixes (those
// the pillars share and whose diagnostic base differs; the filter is monotone on partial masks, DESIGN 2).  Every coarse
// genome then streams its pass-1 output past C once (k_coarse_probe): presence and diagnostic bases into a state word per
// candidate, its keys under a candidate's prefix into its hit list; k_coarse_flag applies the presence test and the filter
// to the completed masks.  Needs filter mode 1, one diagnostic column, at most CO_MAXG genomes; else, or when a hit list
// overflows, the coarse genomes are sorted fine and the call is today's.  Returns KR_COARSE_PASS for "not taken".
#define KR_COARSE_PASS (-1001)       // internal
static int64_t intersect_coarse(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    std::vector<Genome*> cg;
    std::vector<int> pid, cpos;
    std::vector<uint8_t> pin;
    bool has_in = false, has_out = false;
    for (int i = 0; i < n; i++) {
        auto it = c->genomes.find(ids[i]);
        if (it == c->genomes.end()) return KR_COARSE_PASS;          // (the usual path reports it)
        if (it->second.coarse) { cg.push_back(&it->second); cpos.push_back(i); }
        else {
            pid.push_back(ids[i]);
            pin.push_back(is_in[i]);
            (is_in[i] ? has_in : has_out) = true;
        }
    }
    if (cg.empty()) return KR_COARSE_PASS;
    // all coarse genomes of the call hold one strand (co_strand.inc): each key is asked both ways; none does: today's probe;
    // a mix (the option changed between their partitions): they are sorted fine
    size_t n_one = 0;
    for (Genome* G : cg) n_one += G->one_strand;
    if (n_one != 0 && n_one != cg.size()) return KR_COARSE_PASS;
    const bool one = n_one != 0;
    const bool ok = apply_filter && fmode(c, apply_filter) == 1 && c->g.D == 1 && n <= CO_MAXG && has_in && has_out &&
                    c->nslices == 1 && !c->wide.on && !c->custom_layout;
    if (!ok) return KR_COARSE_PASS;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t nC64 = intersect_batch(c, pid.data(), (int)pid.size(), pin.data(), 1);
    if (nC64 <= 0) {
        if (nC64 == 0) c->coarse_done += (int64_t)cg.size();
        return nC64;
    }
    int rc;
    if ((rc = cands_fit(c, (uint64_t)nC64, "kr_intersect"))) return rc;
    const u32 nC = (u32)nC64, nblk = (nC + 255) / 256;
    const Geom g = slice_geom(c, 0);
    hipStream_t st = c->stream;
    // (a hit list holds the genome's keys under ANY candidate of C: at the reference's divergences about 0.8 per candidate)
    const u32 hitcap = c->co_hitcap ? c->co_hitcap : (u32)std::min<u64>(2ull * nC + 65536, 0x7FFFFFF0ull);
    if ((rc = ensure(c, c->co_state, (size_t)nC * 4))) return rc;
    if ((rc = ensure(c, c->co_tab, (size_t)(2 * 260 + 256 * CO_ROW) * 4))) return rc;
    if ((rc = cands_compact_room(c, nC))) return rc;
    // one-strand form: two entries per candidate, then the class counts, bounds (+ 1) and cursors
    const size_t ent_bytes = (size_t)2 * nC * sizeof(CoEnt);
    if (one && (rc = ensure(c, c->co_ent, ent_bytes + (size_t)(3 * CS_CLS + 8) * 4))) return rc;
    for (Genome* G : cg) {
        if (G->hitcap < hitcap || !G->hits.p) {
            if ((rc = ensure(c, G->hits, (size_t)hitcap * 8 + 16))) return rc;
        }
        G->hitcap = hitcap;
        G->hits_valid = false;
    }
    if (c->co_occ == 0) {
        int per = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_coarse_probe<0>, CO_T, 0);
        c->co_occ = (e == hipSuccess && per >= 1) ? per : 1;
        // (one grid for both forms: the one-strand form holds the same LDS and is compiled for the same occupancy)
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_coarse_probe<1>, CO_T, 0) == hipSuccess && per >= 1)
            c->co_occ = std::min(c->co_occ, per);
    }
    const u32 grid = c->co_grid ? c->co_grid : (u32)(c->co_occ * c->ncu);
    if ((rc = join_lanes(c))) return rc;                // (the partitions ran on the sort lanes)
    HIPCHK(c, hipMemsetAsync(c->co_state.p, 0, (size_t)nC * 4, st));
    u32 *cb = (u32*)c->co_tab.p, *ust = cb + 260, *rows = cb + 520;
    u32 need = 0;
    CoarsePub pub{};
    pub.n = (int)cg.size();
    CoarseArgs ca{};
    ca.n = (u32)cg.size();
    for (size_t j = 0; j < cg.size(); j++) {
        Genome& G = *cg[j];
        ca.keys[j] = (const u64*)(G.ckeys.p ? G.ckeys.p : G.sl[0].keys.p);       // (pass 1 wrote the pooled buffer where the genome holds one)
        ca.off[j] = (const u32*)G.sl[0].off.p;
        ca.hits[j] = (u32*)G.hits.p;
        ca.hitcap[j] = hitcap;
        ca.bit[j] = 8u + (u32)j;
        ca.side[j] = is_in[cpos[j]] ? 0u : 4u;
        need |= 1u << (8 + j);
        pub.cnt[j] = (const u32*)G.hits.p;
    }
    {
        // one launch each for all coarse genomes of the call (k_coarse_tables also clears their hit counts)
        StageScope sc(c, KR_ST_INTERSECT, st);
        if (one) {
            const CoStrand S = cs_make(g.L, g.R);
            CoEnt* ents = (CoEnt*)c->co_ent.p;
            u32 *cnt = (u32*)((char*)c->co_ent.p + ent_bytes), *cls = cnt + CS_CLS, *cursor = cls + CS_CLS + 4;
            const u32 cgrid = std::min<u32>((nC + CS_T - 1) / CS_T, (u32)c->ncu);
            HIPCHK(c, hipMemsetAsync(cnt, 0, CS_CLS * 4, st));
            hipLaunchKernelGGL(k_strand_count, dim3(cgrid), dim3(CS_T), 0, st, (const kr_cand*)c->candB.p, nC, S, cnt);
            hipLaunchKernelGGL(k_strand_tables, dim3(1), dim3(CS_CLS), 0, st, (const u32*)cnt, ca, c->co_tcap, cls, cursor, ust, rows,
                               c->mbox + 56, (u32)c->coarse_pass);
            hipLaunchKernelGGL(k_strand_fill, dim3(cgrid), dim3(CS_T), 0, st, (const kr_cand*)c->candB.p, nC, S, cursor, ents);
            hipLaunchKernelGGL(k_coarse_probe<1>, dim3(grid), dim3(CO_T), 0, st, ca, (const u32*)cls, (const u32*)ust, (const u32*)rows,
                               (const kr_cand*)c->candB.p, (u32*)c->co_state.p, c->co_tcap, g.pmask, g.LRrel, (const CoEnt*)ents, S,
                               (u32)c->coarse_pass);
        } else {
            hipLaunchKernelGGL(k_coarse_tables, dim3(1), dim3(256), 0, st, (const kr_cand*)c->candB.p, nC, ca, c->co_tcap, cb, ust, rows);
            hipLaunchKernelGGL(k_coarse_probe<0>, dim3(grid), dim3(CO_T), 0, st, ca, (const u32*)cb, (const u32*)ust, (const u32*)rows,
                               (const kr_cand*)c->candB.p, (u32*)c->co_state.p, c->co_tcap, g.pmask, g.LRrel, (const CoEnt*)nullptr,
                               CoStrand{}, 0u);
        }
    }
    for (Genome* G : cg)
        if (G->ckeys.p) G->ckeys_busy = st;             // (the probe is the last reader of a pooled buffer)
    {
        StageScope sc(c, KR_ST_MERGE, st);
        hipLaunchKernelGGL(k_coarse_flag, dim3(nblk), dim3(256), 0, st, (kr_cand*)c->candB.p, nC, (const u32*)c->co_state.p, need,
                           fmode(c, 1), (u32*)c->flags.p, (u32*)c->blockcnt.p);
        cands_compact_enqueue(c, nC, st, true);
        hipLaunchKernelGGL(k_coarse_publish, dim3(1), dim3(64), 0, st, pub, c->mbox + 32);
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    for (Genome* G : cg) G->ckeys_busy = nullptr;       // (the host has waited: nothing is at the pooled buffers)
    if (one) {
        c->one_calls++;
        for (int q = 0; q < 2; q++) {
            c->one_last[q] = ((volatile u32*)c->mbox)[56 + q];
            c->one_rounds[q] += c->one_last[q];
        }
        c->one_last_passes = ((volatile u32*)c->mbox)[58];
    }
    for (size_t j = 0; j < cg.size(); j++)
        if (((volatile u32*)c->mbox)[32 + j] > hitcap) {
            // a hit list that overflowed (a genome that repeats the candidates' prefixes many times over): nothing is
            // truncated -- the coarse genomes are sorted fine and the caller runs the call over all of them
            c->ncand = -1;
            return KR_COARSE_PASS;
        }
    const u32 total = ((volatile u32*)c->mbox)[16];
    cands_compact_adopt(c, total);
    for (Genome* G : cg) G->hits_valid = true;
    c->coarse_done += (int64_t)cg.size();
    {
        // the stream is idle: placed pass-1 targets for the genomes that came back without one (from their next partition on)
        int want = 0;
        for (Genome* G : cg) want += !G->ckeys.p && G->partitions >= 2;
        if (want > 0) coarse_pool_grow(c, want);      // (less what lies in the free list)
    }
    return total;
}

int64_t kr_intersect(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    if (!c || n < 1) return fail(c, KR_ERR_PARAM, "kr_intersect: need at least one genome");
    if (c->custom_layout) return fail(c, KR_ERR_STATE, "kr_intersect: this context sorts by a custom field order (kr_set_field_order)");
    {
        bool any_coarse = false;
        for (auto& kv : c->genomes) kv.second.hits_valid = false;      // (hit lists belong to ONE candidate list: the one made below)
        for (int i = 0; i < n; i++) {
            auto it = c->genomes.find(ids[i]);
            any_coarse = any_coarse || (it != c->genomes.end() && it->second.coarse);
        }
        if (any_coarse) {
            const int64_t r = intersect_coarse(c, ids, n, is_in, apply_filter);
            if (r != KR_COARSE_PASS) return r;
            int rcf;
            for (int i = 0; i < n; i++)
                if ((rcf = ensure_fine_id(c, ids[i]))) return rcf;
        }
    }
    if (n <= MAXG) return intersect_batch(c, ids, n, is_in, apply_filter);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t cur = -1, nprev = 0;
    int rc;
    for (int o = 0; o < n; o += MAXG) {
        const int m = std::min(MAXG, n - o);
        if ((cur = intersect_batch(c, ids + o, m, is_in + o, 0)) < 0) return cur;
        if (o > 0) {
            if ((rc = ensure(c, c->other, ((size_t)nprev + 2) * sizeof(kr_cand)))) return rc;
            if (nprev) HIPCHK(c, hipMemcpyAsync(c->other.p, c->candP.p, (size_t)nprev * sizeof(kr_cand), hipMemcpyDeviceToDevice, c->stream));
            if ((cur = cands_merge_device(c, (size_t)nprev, 1, 0)) < 0) return cur;
        }
        if (o + MAXG < n) {
            if ((rc = ensure(c, c->candP, ((size_t)cur + 2) * sizeof(kr_cand)))) return rc;
            if (cur) HIPCHK(c, hipMemcpyAsync(c->candP.p, c->candB.p, (size_t)cur * sizeof(kr_cand), hipMemcpyDeviceToDevice, c->stream));
            nprev = cur;
        }
    }
    if (apply_filter) cur = cands_merge_device(c, 0, 0, 1);
    return cur;
}

// the pipelined kernels' items over one slice of the anchor: items of 2^mlog buckets that hold, with all but vanishing
// probability for evenly filled buckets, at most 4 T anchor keys (T = 256 .. 512 threads); fuller ones are listed and go
// through k_intersect.  tagk: 32-bit heads (k_intersect3t.inc) where the sub-bin field starts in the key's high word and at
// most 32 bits above the prefix's lowest bit
struct ItemPlan {
    int mlog;       // an item is 2^mlog buckets
    u32 T;          // threads of its workgroup
    bool tagk;      // the kernels with 32-bit heads apply
    int p0, sht;    // the prefix's lowest bit; the shift to the sub-bin field of the 32-bit heads
};
static ItemPlan item_plan(const kr_ctx* c, const Slice& AS, const Geom& g) {
    const u32 nbk = 1u << c->g.b;
    const double avg = (double)std::max<int64_t>(AS.count >= 0 ? AS.count : (int64_t)AS.nmax, 1) / nbk;   // (nmax: the bound 2 n, exact but for N / masked windows)
    auto need = [](double mean) { return mean + 6.0 * std::sqrt(mean) + 8.0; };
    ItemPlan p;
    p.mlog = 0;
    while ((2u << p.mlog) <= nbk && need(avg * (2u << p.mlog)) <= (double)I3_SLOTS) p.mlog++;
    p.T = (u32)std::min(512.0, std::max(256.0, 64.0 * std::ceil(need(avg * (1u << p.mlog)) / 256.0)));
    p.p0 = 64 - 2 * g.LRrel;
    p.sht = g.rb + p.mlog - (int)I3T_NB_LOG;
    p.tagk = c->isect_kernel != 2 && p.p0 >= 0 && p.p0 < 32 && p.sht >= 32 && p.sht <= p.p0 + 32;
    return p;
}

// the pipelined kernels by [anchor in bucket order: k_intersect3t<., true>][mask format; 3 = one 32-bit state word] for the
// 32-bit heads, by [mask format] for the 64-bit ones; the chunk kernel by [mask format]
typedef void (*Isect3Kernel)(Isect3Args, Geom);
static Isect3Kernel isect3_kernel(bool ua, bool tagk, bool st32, int fmt) {
    static const Isect3Kernel heads32[2][4] = {
        {k_intersect3t<0>, k_intersect3t<1>, k_intersect3t<2>, k_intersect3t<3>},
        {k_intersect3t<0, true>, k_intersect3t<1, true>, k_intersect3t<2, true>, k_intersect3t<3, true>}};
    static const Isect3Kernel heads64[3] = {k_intersect3<0>, k_intersect3<1>, k_intersect3<2>};
    return tagk ? heads32[ua ? 1 : 0][st32 ? 3 : fmt] : heads64[fmt];
}
typedef void (*IsectKernel)(IsectArgs, Geom);
static const IsectKernel isect_chunk_kernel[3] = {k_intersect<0>, k_intersect<1>, k_intersect<2>};

// The genomes' sorts may still be running: their kernels are ordered before the intersection on the device, the
// host does not wait for them.  What a sort leaves open (its key count; rarely oversized buckets for the merge
// fallback) is looked at after the intersection's own synchronisation: *redo = a fallback ran, so the result just
// computed is void (once per such genome).
static int64_t intersect_once(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter, bool* redo) {
    *redo = false;
    if (!c || n < 1 || n > MAXG) return fail(c, KR_ERR_PARAM, "kr_intersect: 1 .. %d genomes per batch", MAXG);
    HIPCHK(c, hipSetDevice(c->device));
    int anchor = 0;
    u64 best = ~0ull;
    u32 ingroup_bits = 0;
    std::vector<Genome*> gs;
    for (int i = 0; i < n; i++) {
        auto it = c->genomes.find(ids[i]);
        if (it == c->genomes.end() || !it->second.sorted) return fail(c, KR_ERR_STATE, "genome %d not sorted", ids[i]);
        Genome& G = it->second;
        if (is_in[i]) ingroup_bits |= 1u << i;
        if (G.nmax < best) { best = G.nmax; anchor = i; }
        gs.push_back(&G);
    }
    int rc;
    // the pipelined kernel (k_intersect3.inc) wherever a (left,right) group lies inside one fine bucket
    const bool use3 = n >= 2 && 2 * c->g.LRrel >= c->g.b && !(c->dbg & 32) && c->isect_kernel != 1;
    // KR_OPT_LAZY_ORDER: genomes whose sort stopped at the fine buckets.  The pipelined kernels hash every streamed key
    // into the sub-bins of the item's anchor run -- they never look at a streamed genome's order inside a bucket --, so
    // only the ANCHOR's buckets are sorted now (its run of an item is the slot array: equal prefixes adjacent, survivors
    // in order); the chunk kernel (k_intersect: merges of sorted runs) needs every genome in order.
    bool all_ordered = true;
    for (Genome* G : gs) all_ordered = all_ordered && G->ordered;
    for (int q = 0; q < n; q++) gs[q]->was_anchor = use3 && q == anchor;
    if (!all_ordered) {
        if (use3) {
            // (the anchor, too, may stay as it is where the kernel with 32-bit heads applies to EVERY slice -- the item
            // geometry below decides that, k_intersect3t<., UA> then makes the item's slots itself; else its LDS sort runs now)
            bool ua_ok = c->fuse_anchor && c->isect_kernel != 2;
            for (int s = 0; ua_ok && s < c->nslices; s++) ua_ok = item_plan(c, gs[anchor]->sl[s], slice_geom(c, (u32)s)).tagk;
            if (!gs[anchor]->ordered && !ua_ok) {
                if ((rc = join_lanes(c))) return rc;
                if ((rc = order_genome(c, *gs[anchor], c->stream))) return rc;
            }
            all_ordered = true;
            for (Genome* G : gs) all_ordered = all_ordered && G->ordered;
        } else {
            if ((rc = ensure_ordered(c, gs))) return rc;
            all_ordered = true;
        }
    }
    bool pending = false;
    for (Genome* G : gs) pending = pending || !G->finalized;
    std::vector<Slice*> open_slices;
    if (pending) {
        // the words finalize() reads arrive with this call's first synchronisation behind their publication
        for (Genome* G : gs)
            if (!G->finalized)
                for (Slice& S : G->sl) open_slices.push_back(&S);
        if (open_slices.size() > PUB_CAP) {
            if ((rc = finalize(c, gs))) return rc;
            pending = false;
        } else {
            if ((rc = join_lanes(c))) return rc;
            publish_slices(c, open_slices.data(), open_slices.size(), c->stream);
        }
    }
    Genome& A = *gs[anchor];
    u64 amax = 0;
    u32 cmax = 0;
    for (Slice& S : A.sl) { amax = std::max(amax, S.nmax); cmax = std::max(cmax, S.nchunks); }
    if ((rc = ensure(c, c->candA, (amax + 2) * sizeof(kr_cand)))) return rc;      // per-slice sparse runs
    if ((rc = ensure(c, c->candB, 4096 * sizeof(kr_cand)))) return rc;            // dense result: grows as needed
    if ((rc = ensure(c, c->chunkcnt, ((size_t)cmax + 2) * 4))) return rc;
    if ((rc = ensure(c, c->chunkpos, ((size_t)cmax + 2) * 4))) return rc;
    {
        const size_t nt = ((size_t)std::max(cmax, 1u << c->g.b) + 2047) / 2048 + 8;       // (the scan of the unit counts, in tiles)
        if ((rc = ensure(c, c->coltsum, nt * 4))) return rc;
        if ((rc = ensure(c, c->coltpos, nt * 4))) return rc;
    }
    hipStream_t st = c->stream;
    u64 running = 0;
    const u32 nbk = 1u << c->g.b;
    if (use3) {
        if ((rc = ensure(c, c->chunkcnt, ((size_t)std::max(cmax, nbk) + 2) * 4))) return rc;
        if ((rc = ensure(c, c->chunkpos, ((size_t)std::max(cmax, nbk) + 2) * 4))) return rc;
        if (!c->isovf.p) {
            if ((rc = ensure(c, c->isovf, ((size_t)I3_OVF_CAP + 4) * 4))) return rc;
            HIPCHK(c, hipMemsetAsync(c->isovf.p, 0, ((size_t)I3_OVF_CAP + 4) * 4, st));      // (once: k_publish_reset reads the count and clears it)
        }
    }
    for (int s = 0; s < c->nslices; s++) {
        const Geom g = slice_geom(c, (u32)s);
        Slice& AS = A.sl[s];
        const int fmt = g.D > 8 ? 2 : ((g.D > 4 || c->isect_fmt == 1) ? 1 : 0);
        IsectArgs a{};
        a.n = n;
        a.ingroup_bits = ingroup_bits;
        a.apply_filter = fmode(c, apply_filter);
        a.dbg = c->dbg;
        a.anchor = anchor;
        for (int i = 0; i < n; i++) {
            a.keys[i] = (const u64*)gs[i]->sl[s].keys.p;
            a.off[i] = (const u32*)gs[i]->sl[s].off.p;
        }
        a.chunkdesc = (const uint4*)AS.chunkdesc.p;
        a.tmp = (kr_cand*)c->candA.p;
        a.chunkcnt = (u32*)c->chunkcnt.p;
        auto launch_chunks = [&](u32 grid) {
            hipLaunchKernelGGL(isect_chunk_kernel[fmt], dim3(grid), dim3(IS_THREADS), 0, st, a, g);
        };
        bool by_items = use3;
        u32 nunits = AS.nchunks;          // runs of survivors: per chunk, or per item
        Isect3Args a3{};
        if (by_items) {
            // items of 2^mlog buckets that hold, with all but vanishing probability for evenly filled buckets, at most
            // 4 T anchor keys (T = 256 .. 512 threads); fuller ones are listed and go through k_intersect below
            const ItemPlan ip = item_plan(c, AS, g);
            const int mlog = ip.mlog;
            const u32 T = ip.T;
            const bool tagk = ip.tagk;
            const bool ua = tagk && !gs[anchor]->ordered;        // (an anchor in bucket order: every slice's kernel has 32-bit heads -- checked above)
            a3.n = n;
            a3.ingroup_bits = ingroup_bits;
            a3.anchor = anchor;
            a3.apply_filter = a.apply_filter;
            for (int i = 0; i < n; i++) { a3.keys[i] = a.keys[i]; a3.off[i] = a.off[i]; }
            a3.nb = nbk;
            a3.mlog = mlog;
            a3.nitems = (nbk + (1u << mlog) - 1) >> mlog;
            a3.sh = tagk ? ip.sht : std::max(g.rb + mlog - (int)I3_NB_LOG, ip.p0);
            a3.p0 = ip.p0;
            a3.tmp = (kr_cand*)c->candA.p;
            a3.itemcnt = (u32*)c->chunkcnt.p;
            a3.ovf = (u32*)c->isovf.p;
            a3.ovf_cap = c->i3_ovf_cap;
            c->i3_last_T = (int)T;
            c->i3_last_mlog = mlog;
            nunits = a3.nitems;
            c->i3_last_tags = tagk ? 1 : 0;
            // (one diagnostic column, at most 24 genomes: the slot's state is one 32-bit word)
            const bool st32 = tagk && fmt == 0 && g.D == 1 && n <= 24 && c->isect_fmt == 0;
            // two genomes, one of each side, one diagnostic column, filter on: the screen and the small exact join
            // (k_join2.inc) -- it never looks at the order inside a bucket, of either genome
            const bool join2 = c->join2 && n == 2 && (ingroup_bits == 1u || ingroup_bits == 2u) && a.apply_filter == 1 &&
                               g.D == 1 && tagk && ip.p0 >= 2 && c->isect_fmt == 0 && c->isect_kernel == 0 && c->fuse_anchor != 0;
            const bool dense2 = c->join2_dense != 0;
            const Isect3Kernel kern = join2 ? (dense2 ? k_join2<true> : k_join2<false>) : isect3_kernel(ua, tagk, st32, fmt);
            int& occ = join2 ? c->j2_occ[dense2 ? 1 : 0][T / 64] : c->i3_occ[ua ? 2 : (tagk ? 1 : 0)][st32 ? 3 : fmt][T / 64];
            if (occ == 0) {
                int per = 0;
                const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, (int)T, 0);
                occ = (e == hipSuccess && per >= 1) ? per : 1;
            }
            u32 grid = std::min<u32>(a3.nitems, (u32)(occ * c->ncu));
            if (join2 && c->j2_grid) grid = std::min(grid, c->j2_grid);
            {
                StageScope sc(c, KR_ST_INTERSECT, st);
                c->i3_last_ua = ua ? 1 : 0;
                if (ua) c->isect_ua++;
                if (join2) c->j2_launches++;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(T), 0, st, a3, g);
                a.ovf = (const u32*)c->isovf.p;
                a.ovf_cap = c->i3_ovf_cap;
                a.mlog = mlog;
                a.nb = nbk;
                // (oversized items: the chunk kernel over the listed ones -- it walks sorted runs; with a genome still in
                // bucket order the count alone is looked at below)
                if (all_ordered) launch_chunks(I3_OVF_LAUNCH);
            }
        } else {
            StageScope sc(c, KR_ST_INTERSECT, st);
            launch_chunks(AS.nchunks);
        }
        u32 total = 0;
        // one synchronisation per slice: the scan's total and the count of oversized items arrive in the host
        // mailbox (k_publish), and the gather is launched BEFORE the host knows the total, against the room the
        // dense list has (the kernel writes nothing when the total exceeds it; the host then grows the list and
        // launches it again)
        auto gather = [&](u32 cap) {
            if (by_items)
                hipLaunchKernelGGL(k_gather_items, dim3((nunits + GI_ITEMS - 1) / GI_ITEMS), dim3(GI_T), 0, st, g.sbits, g.slice,
                                   (const kr_cand*)c->candA.p, (const u32*)AS.off.p, a3.mlog, nbk,
                                   (const u32*)c->chunkcnt.p, (const u32*)c->chunkpos.p, (kr_cand*)c->candB.p + running,
                                   nunits, cap);
            else
                hipLaunchKernelGGL(k_gather_cands, dim3(AS.nchunks), dim3(64), 0, st, g.sbits, g.slice,
                                   (const kr_cand*)c->candA.p, (const uint4*)AS.chunkdesc.p,
                                   (const u32*)c->chunkcnt.p, (const u32*)c->chunkpos.p,
                                   (kr_cand*)c->candB.p + running, nunits, cap);
        };
        for (;;) {
            u32 novf = 0, cap = 0;
            {
                StageScope sc(c, KR_ST_COMPACT, st);
                if (nunits > 8192) {
                    // (one workgroup walks 65536 counts in 36 us; tiles of 2048 in three short launches take 14)
                    const u32 nt = (nunits + 2047) / 2048;
                    hipLaunchKernelGGL(k_tile_sums, dim3(nt), dim3(256), 0, st, (const u32*)c->chunkcnt.p, nunits, (u32*)c->coltsum.p);
                    if (nt <= TA2_MAX) {
                        hipLaunchKernelGGL(k_tile_apply2, dim3(nt), dim3(256), 0, st, (const u32*)c->chunkcnt.p, nunits,
                                           (const u32*)c->coltsum.p, nt, (u32*)c->chunkpos.p, c->mbox,
                                           by_items ? (u32*)c->isovf.p : (u32*)nullptr);
                    } else {
                        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)c->coltsum.p, (u32*)c->coltpos.p, nt);
                        hipLaunchKernelGGL(k_tile_apply, dim3(nt), dim3(256), 0, st, (const u32*)c->chunkcnt.p, nunits,
                                           (const u32*)c->coltpos.p, nt, (u32*)c->chunkpos.p);
                        hipLaunchKernelGGL(k_publish_reset, dim3(1), dim3(64), 0, st, (const u32*)c->chunkpos.p + nunits,
                                           by_items ? (u32*)c->isovf.p : (u32*)nullptr, c->mbox);
                    }
                } else {
                    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)c->chunkcnt.p, (u32*)c->chunkpos.p, nunits);
                    hipLaunchKernelGGL(k_publish_reset, dim3(1), dim3(64), 0, st, (const u32*)c->chunkpos.p + nunits,
                                       by_items ? (u32*)c->isovf.p : (u32*)nullptr, c->mbox);
                }
                const size_t room = c->candB.bytes / sizeof(kr_cand);
                cap = room > running + 2 ? (u32)std::min<size_t>(room - running - 2, 0xFFFFFFFFu) : 0u;
                gather(cap);
            }
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            total = ((volatile u32*)c->mbox)[0];
            novf = by_items ? ((volatile u32*)c->mbox)[1] : 0u;
            if (by_items && novf > 0 && c->j2_launches) {
                // (rare) items k_join2 handed on because their live keys found no room in its table: counted once per call
                u32 nfull = 0;
                HIPCHK(c, hipMemcpy(&nfull, (const u32*)c->isovf.p + J2_FULL_WORD, 4, hipMemcpyDeviceToHost));
                if (nfull) HIPCHK(c, hipMemset((u32*)c->isovf.p + J2_FULL_WORD, 0, 4));
                if (!c->j2_full_counted) c->j2_full += nfull;
                c->j2_full_counted = !all_ordered && !c->j2_full_counted;
            }
            if (by_items && novf > 0 && !all_ordered) {
                // an item whose anchor run exceeds the slot array (skew): its turn is the chunk kernel's -- every genome
                // in order first, then the whole call once more (rare: satellites, low-complexity runs)
                if ((rc = ensure_ordered(c, gs))) return rc;
                if ((rc = finalize(c, gs))) return rc;
                *redo = true;
                return 0;
            }
            if (by_items && novf > c->i3_ovf_cap) {
                // more oversized items than the second launch took (heavy skew): all of the slice by chunks
                by_items = false;
                nunits = AS.nchunks;
                a.ovf = nullptr;
                c->isect_refall++;
                StageScope sc2(c, KR_ST_INTERSECT, st);
                launch_chunks(AS.nchunks);
                continue;
            }
            c->isect_ovf_items += novf;
            if (total > cap) {
                StageScope sc(c, KR_ST_COMPACT, st);
                size_t want = running + total + 2;
                if (s == 0 && c->nslices > 1)       // size for all slices at once instead of doubling through them
                    want = (size_t)((double)total * c->nslices * 1.15) + 4096;
                if ((rc = ensure_keep(c, c->candB, want * sizeof(kr_cand), running * sizeof(kr_cand))))
                    return rc;
                gather(0xFFFFFFFFu);
                // (rare path: this gather reads the anchor's offsets and nobody waits for it below -- a sort of the same
                // genome on another lane must not overwrite them under it)
                HIPCHK(c, hipStreamSynchronize(st));
            }
            break;
        }
        running += total;
        if ((rc = cands_fit(c, running, "kr_intersect"))) return rc;
    }
    HIPCHK(c, hipGetLastError());        // (no wait for the last gather: everything that reads the list is ordered behind it)
    if (pending) {
        if ((rc = finalize(c, gs, true, redo))) return rc;
        if (*redo) return 0;
    }
    c->ncand = (int64_t)running;
    return c->ncand;
}

int64_t kr_cands_count(kr_ctx* c) { return c ? c->ncand : KR_ERR_PARAM; }

int64_t kr_cands_fetch(kr_ctx* c, kr_cand* out, size_t cap) {
    if (!c || c->ncand < 0) return fail(c, KR_ERR_STATE, "no candidate set");
    if ((size_t)c->ncand > cap) return fail(c, KR_ERR_CAPACITY, "candidate buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->ncand) HIPCHK(c, hipMemcpy(out, c->candB.p, (size_t)c->ncand * sizeof(kr_cand), hipMemcpyDeviceToHost));
    return c->ncand;
}

int64_t kr_cands_load(kr_ctx* c, const kr_cand* cands, size_t n) {
    if (!c) return KR_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = cands_fit(c, n, "kr_cands_load"))) return rc;
    if ((rc = ensure(c, c->candB, (n + 2) * sizeof(kr_cand)))) return rc;
    if ((rc = ensure(c, c->candA, (n + 2) * sizeof(kr_cand)))) return rc;
    if (n) HIPCHK(c, hipMemcpy(c->candB.p, cands, n * sizeof(kr_cand), hipMemcpyHostToDevice));
    for (auto& kv : c->genomes) kv.second.hits_valid = false;      // (a list from outside: no coarse genome has its hits)
    c->ncand = (int64_t)n;
    return c->ncand;
}

// candidates := candidates INTERSECT the m candidates already in c->other (device memory), masks
// OR-ed, and / or the diagnostic filter
static int64_t cands_merge_device(kr_ctx* c, size_t m, int have_other, int apply_filter) {
    if (cands_fit(c, (uint64_t)c->ncand, "kr_cands_merge") || cands_fit(c, m, "kr_cands_merge")) return KR_ERR_CAPACITY;
    const u32 n = (u32)c->ncand;
    if (n == 0) return 0;
    if (have_other && m == 0) { c->ncand = 0; return 0; }
    hipStream_t st = c->stream;
    int rc;
    const u32 nblk = (n + 255) / 256;
    if ((rc = cands_compact_room(c, n))) return rc;
    if ((rc = ensure(c, c->other, 64))) return rc;
    const u32* dtotal;
    {
        StageScope sc(c, KR_ST_MERGE);
        hipLaunchKernelGGL(k_cands_flag, dim3(nblk), dim3(256), 0, st, (kr_cand*)c->candB.p, n,
                           (const kr_cand*)c->other.p, (u32)m, have_other ? 1 : 0, fmode(c, apply_filter), c->g.D,
                           (u32*)c->flags.p, (u32*)c->blockcnt.p, (const u64*)nullptr);
        dtotal = cands_compact_enqueue(c, n, st, false);
    }
    u32 total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, dtotal, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return cands_compact_adopt(c, total);
}

// candidates := those whose (left,right) prefix EVERY listed genome holds, the genomes' diagnostic bases OR-ed into the
// masks of their side, the filter applied.  What kr_intersect + kr_cands_merge would leave for the same genomes, without
// building the genomes' own candidate list first -- which, for genomes of one side only, is every prefix they hold
// (the streaming flow's later batches: krisp_fasta.py, _find_regions_streaming).  Batches of 32 genomes (the side bits).
static int64_t cands_probe_impl(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter, bool from_wide);
int64_t kr_cands_probe(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    return cands_probe_impl(c, ids, n, is_in, apply_filter, false);
}
// (from_wide: a phase of kr_wide_run in batches -- the context's geometry is that phase's: h_wide.inc)
static int64_t cands_probe_impl(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter, bool from_wide) {
    if (!c || c->ncand < 0) return fail(c, KR_ERR_STATE, "no candidate set");
    if (!c->have_params || (c->wide.on && !from_wide)) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (c->custom_layout) return fail(c, KR_ERR_STATE, "kr_cands_probe: this context sorts by a custom field order (kr_set_field_order)");
    if (n < 1 || !ids || !is_in) return fail(c, KR_ERR_PARAM, "kr_cands_probe: need at least one genome");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->ncand == 0) return 0;
    if (cands_fit(c, (uint64_t)c->ncand, "kr_cands_probe")) return KR_ERR_CAPACITY;
    hipStream_t st = c->stream;
    int rc;
    for (int o = 0; o < n; o += 32) {
        const int m = std::min(32, n - o);
        std::vector<Genome*> gs;
        u32 bits = 0;
        for (int i = 0; i < m; i++) {
            if ((rc = ensure_fine_id(c, ids[o + i]))) return rc;
            auto it = c->genomes.find(ids[o + i]);
            if (it == c->genomes.end() || !it->second.sorted) return fail(c, KR_ERR_STATE, "genome %d not sorted", ids[o + i]);
            gs.push_back(&it->second);
            if (is_in[o + i]) bits |= 1u << i;
        }
        if ((rc = ensure_ordered(c, gs))) return rc;          // (the probe searches sorted runs)
        if ((rc = finalize(c, gs))) return rc;
        const size_t np = (size_t)m * c->nslices;
        std::vector<uint64_t> tab(2 * np + 1);
        for (int i = 0; i < m; i++)
            for (int s = 0; s < c->nslices; s++) {
                tab[(size_t)i * c->nslices + s] = (uint64_t)gs[i]->sl[s].keys.p;
                tab[np + (size_t)i * c->nslices + s] = (uint64_t)gs[i]->sl[s].off.p;
            }
        c->coltab_host.clear();                 // (kr_collect's cached table: this one takes its place)
        if ((rc = ensure(c, c->coltab, tab.size() * 8))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->coltab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
        CollectArgs a;
        a.keys = (const u64* const*)c->coltab.p;
        a.off = (const u32* const*)((uint64_t*)c->coltab.p + np);
        a.gid = nullptr;
        a.n = m;
        a.nslices = c->nslices;
        a.ibo = nullptr;
        a.arena = nullptr;
        a.mcnt = nullptr;
        const u32 nc = (u32)c->ncand, nblk = (nc + 255) / 256;
        if ((rc = cands_compact_room(c, nc))) return rc;
        {
            StageScope sc(c, KR_ST_MERGE);
            // (the filter with the last batch of 32 only: before it the masks are not complete -- but partial masks may prune, it is monotone)
            hipLaunchKernelGGL(k_cands_probe_tab, dim3(nblk), dim3(256), 0, st, (kr_cand*)c->candB.p, nc, a, bits, fmode(c, apply_filter),
                               slice_geom(c, 0), (u32*)c->flags.p, (u32*)c->blockcnt.p);
            cands_compact_enqueue(c, nc, st, true);
        }
        HIPCHK(c, hipStreamSynchronize(st));        // (also: `tab` may go out of scope now)
        HIPCHK(c, hipGetLastError());
        if (cands_compact_adopt(c, ((volatile u32*)c->mbox)[16]) == 0) break;
    }
    return c->ncand;
}

int64_t kr_cands_merge(kr_ctx* c, const kr_cand* other, size_t m, int have_other, int apply_filter) {
    if (!c || c->ncand < 0) return fail(c, KR_ERR_STATE, "no candidate set");
    if (!c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->ncand == 0) return 0;
    int rc;
    if (have_other) {
        if ((rc = ensure(c, c->other, (m + 2) * sizeof(kr_cand)))) return rc;
        if (m) HIPCHK(c, hipMemcpyAsync(c->other.p, other, m * sizeof(kr_cand), hipMemcpyHostToDevice, c->stream));
    }
    return cands_merge_device(c, m, have_other, apply_filter);
}

static int64_t collect_impl(kr_ctx* c, const int* ids, int n, bool force_order);
int64_t kr_collect(kr_ctx* c, const int* ids, int n) { return collect_impl(c, ids, n, false); }

static int64_t collect_impl(kr_ctx* c, const int* ids, int n, bool force_order) {
    if (!c || c->ncand < 0) return fail(c, KR_ERR_STATE, "no candidate set");
    if (c->custom_layout) return fail(c, KR_ERR_STATE, "kr_collect: this context sorts by a custom field order (kr_set_field_order)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc;
    if ((rc = cands_fit(c, (uint64_t)c->ncand, "kr_collect"))) return rc;
    const u32 nc = (u32)c->ncand;
    c->nrecords = 0;
    if (nc == 0 || n == 0) return 0;
    // coarse genomes (kr_genome_partition): the rows of their (candidate, genome) pairs come from the hit lists the coarse
    // route of kr_intersect left -- where the list is short enough for the arena (a row per pair) and every such genome's
    // hits belong to this list; else they are sorted fine first
    bool any_coarse = false;
    {
        bool hits_ok = !force_order && (u64)nc * (u64)n <= ((u64)1 << 22);
        for (int i = 0; i < n; i++) {
            auto it = c->genomes.find(ids[i]);
            if (it == c->genomes.end() || !it->second.coarse) continue;
            any_coarse = true;
            hits_ok = hits_ok && it->second.hits_valid;
        }
        if (any_coarse && !hits_ok) {
            for (int i = 0; i < n; i++)
                if ((rc = ensure_fine_id(c, ids[i]))) return rc;
            any_coarse = false;
        }
    }
    std::vector<Genome*> gs;
    for (int i = 0; i < n; i++) {
        auto it = c->genomes.find(ids[i]);
        if (it == c->genomes.end() || !(it->second.sorted || it->second.coarse))
            return fail(c, KR_ERR_STATE, "genome %d not sorted", ids[i]);
        gs.push_back(&it->second);
    }
    // KR_OPT_LAZY_ORDER: genomes still in bucket order.  For a short candidate list (the usual one behind the diagnostic
    // filter) the bucket of every (candidate, such genome) pair is read once and the pair's keys kept (k_collect_scan:
    // some 10^4 x 1500 keys instead of the genomes' 10^8 each); a long one (no filter, no outgroup), or a geometry whose
    // (left,right) groups span buckets, has the genomes sorted whole first.
    bool touch = false;
    {
        bool any = false;
        for (Genome* G : gs) any = any || !G->ordered;
        if (any) {
            const u64 nbk = (u64)1 << c->g.b;
            touch = !force_order && 2 * c->g.LRrel >= c->g.b && (u64)nc * 4 <= nbk * (u64)c->nslices &&
                    (u64)nc * (u64)n <= ((u64)1 << 22);
            if (!touch && (rc = ensure_ordered(c, gs))) return rc;          // (a coarse genome is left as it is)
            c->order_wanted = !touch;
        }
    }
    const bool arena_on = touch || any_coarse;          // (rows of the pairs: read from buckets, or filled from hit lists)
    if ((rc = finalize(c, gs))) return rc;
    // pointer tables [genome][slice] + the genome ids (+ which genomes lie in bucket order), one upload
    const size_t np = (size_t)n * c->nslices;
    std::vector<uint64_t> tab(2 * np + 2 * ((n + 1) / 2) + 1);
    for (int i = 0; i < n; i++)
        for (int s = 0; s < c->nslices; s++) {
            tab[(size_t)i * c->nslices + s] = (uint64_t)gs[i]->sl[s].keys.p;
            tab[np + (size_t)i * c->nslices + s] = (uint64_t)gs[i]->sl[s].off.p;
        }
    u32* gid_host = (u32*)&tab[2 * np];
    for (int i = 0; i < n; i++) gid_host[i] = (u32)ids[i];
    u32* ibo_host = (u32*)&tab[2 * np + (n + 1) / 2];
    for (int i = 0; i < n; i++) ibo_host[i] = gs[i]->coarse ? 2u : ((touch && !gs[i]->ordered) ? 1u : 0u);   // (2: the row from the hit list)
    if (c->coltab.bytes < tab.size() * 8) c->coltab_host.clear();
    if ((rc = ensure(c, c->coltab, tab.size() * 8))) return rc;
    // a thread, a count and a place per (candidate, genome) pair -- in chunks of candidates, so that neither the pair
    // index (32 bits) nor the scratch (24 bytes per pair) bounds what one call can take (ADVICE r4: 7e7 candidates x 64
    // genomes used to be refused); the records of a chunk follow those of the chunks before it: the order of the
    // whole is (candidate, genome position), as one launch over all pairs would leave it
    const u64 chunk_pairs = []() {
        const char* e = getenv("KR_COLLECT_PAIRS");             // (tests: small chunks on small inputs)
        const u64 v = e ? (u64)atoll(e) : 0;
        return v >= 1 ? std::min<u64>(v, 0xFFFFFF00ull) : ((u64)1 << 28);
    }();
    const u32 per = (u32)std::max<u64>(1, std::min<u64>(nc, chunk_pairs / (u64)n));
    {
        const u32 np2max = per * (u32)n;
        if ((rc = ensure(c, c->collo, (size_t)np2max * 4 + 16))) return rc;
        if ((rc = ensure(c, c->colcnt, ((size_t)np2max + 4) * 4))) return rc;
        if ((rc = ensure(c, c->colpos, ((size_t)np2max + 4) * 4))) return rc;
        if ((rc = ensure(c, c->colfirst, ((size_t)np2max + 2) * 8))) return rc;
        if ((rc = ensure(c, c->colfm, ((size_t)np2max + 4) * 4))) return rc;
        const u32 ntmax = (np2max + 2047) / 2048;
        if ((rc = ensure(c, c->coltsum, ((size_t)ntmax + 4) * 4))) return rc;
        if ((rc = ensure(c, c->coltpos, ((size_t)ntmax + 4) * 4))) return rc;
    }
    if (tab != c->coltab_host) {           // (the same genomes as last time: the table is on the device already)
        HIPCHK(c, hipMemcpyAsync(c->coltab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
        c->coltab_host = tab;
    }
    CollectArgs a;
    a.keys = (const u64* const*)c->coltab.p;
    a.off = (const u32* const*)((uint64_t*)c->coltab.p + np);
    a.gid = (const u32*)((uint64_t*)c->coltab.p + 2 * np);
    a.n = n;
    a.nslices = c->nslices;
    a.ibo = nullptr;
    a.arena = nullptr;
    a.mcnt = nullptr;
    const Geom g = slice_geom(c, 0);
    if (arena_on) {
        // (the arena rows and counts of the pairs; ordered genomes' rows stay unused)
        const size_t npairs = (size_t)nc * (size_t)n;
        if ((rc = ensure(c, c->touchdesc, npairs * COL_CAPM * 8 + npairs * 4 + 64))) return rc;
        if ((rc = ensure(c, c->touchovf, 64))) return rc;
        u64* arena = (u64*)c->touchdesc.p;
        u32* mcnt = (u32*)(arena + npairs * COL_CAPM);
        HIPCHK(c, hipMemsetAsync(c->touchovf.p, 0, 16, st));
        a.ibo = (const u32*)((uint64_t*)c->coltab.p + 2 * np + (n + 1) / 2);
        a.arena = arena;
        a.mcnt = mcnt;
        StageScope sc(c, KR_ST_COLLECT);
        if (any_coarse) HIPCHK(c, hipMemsetAsync(mcnt, 0, npairs * 4, st));      // (the hits take their places in a row by counting)
        if (touch)
            hipLaunchKernelGGL(k_collect_scan, dim3((u32)((npairs + 3) / 4)), dim3(256), 0, st, (const kr_cand*)c->candB.p, (u32)npairs, a, g,
                               arena, mcnt, (u32*)c->touchovf.p);
        if (any_coarse) {
            for (int i = 0; i < n; i++)
                if (gs[i]->coarse)
                    hipLaunchKernelGGL(k_coarse_rows, dim3(1024), dim3(256), 0, st, (const u32*)gs[i]->hits.p, gs[i]->hitcap,
                                       (const kr_cand*)c->candB.p, nc, (u32)n, (u32)i, g.pmask, arena, mcnt);
            hipLaunchKernelGGL(k_coarse_rowsort, dim3((u32)((npairs + 255) / 256)), dim3(256), 0, st, (u32)npairs, (u32)n, a.ibo, arena,
                               mcnt, (u32*)c->touchovf.p);
        }
        // (a pair with more keys than an arena row holds: looked at behind the first synchronisation below)
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, (const u32*)c->touchovf.p, (const u32*)nullptr,
                           (const u32*)nullptr, c->mbox + 20);
        if (touch) c->lazy_touch++;
    }
    u64 done = 0;                           // records of the chunks so far
    for (u32 c0 = 0; c0 < nc; c0 += per) {
        const u32 cc = std::min(per, nc - c0), np2 = cc * (u32)n;
        const kr_cand* cand = (const kr_cand*)c->candB.p + c0;
        CollectArgs ac = a;             // (this chunk's rows of the arena: the kernels index pairs from the chunk's first)
        if (arena_on) {
            ac.arena = a.arena + (size_t)c0 * n * COL_CAPM;
            ac.mcnt = a.mcnt + (size_t)c0 * n;
        }
        const u32 ntiles = (np2 + 2047) / 2048;
        u32 total = 0;
        {
            StageScope sc(c, KR_ST_COLLECT);
            hipLaunchKernelGGL(k_collect_count, dim3((np2 + 255) / 256), dim3(256), 0, st, cand, np2, ac, g,
                               (u32*)c->collo.p, (u32*)c->colcnt.p, (u64*)c->colfirst.p, (u32*)c->colfm.p);
            hipLaunchKernelGGL(k_tile_sums, dim3(ntiles), dim3(256), 0, st, (const u32*)c->colcnt.p, np2, (u32*)c->coltsum.p);
            if (ntiles <= TA2_MAX) {
                hipLaunchKernelGGL(k_tile_apply2, dim3(ntiles), dim3(256), 0, st, (const u32*)c->colcnt.p, np2,
                                   (const u32*)c->coltsum.p, ntiles, (u32*)c->colpos.p, c->mbox + 4, (u32*)nullptr);
            } else {
                hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)c->coltsum.p, (u32*)c->coltpos.p, ntiles);
                hipLaunchKernelGGL(k_tile_apply, dim3(ntiles), dim3(256), 0, st, (const u32*)c->colcnt.p, np2,
                                   (const u32*)c->coltpos.p, ntiles, (u32*)c->colpos.p);
            }
        }
        // the records are emitted before the host knows how many there are, against the room their buffer has (as the
        // gather of kr_intersect): one synchronisation per chunk, the total arrives in the host mailbox
        const size_t room = c->records.bytes / sizeof(kr_record);
        const u32 cap = room > done + 2 ? (u32)std::min<size_t>(room - done - 2, 0xFFFFFFFFu) : 0u;
        {
            StageScope sc(c, KR_ST_COLLECT);
            if (ntiles > TA2_MAX)
                hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, (const u32*)c->colpos.p + np2, (const u32*)nullptr,
                                   (const u32*)nullptr, c->mbox + 4);
            if (cap)
                hipLaunchKernelGGL(k_collect_emit, dim3((np2 + 255) / 256), dim3(256), 0, st, cand, np2, ac, g,
                                   (const u32*)c->collo.p, (const u32*)c->colpos.p, (const u64*)c->colfirst.p, (const u32*)c->colfm.p,
                                   (kr_record*)c->records.p + done, cap);
        }
        HIPCHK(c, hipStreamSynchronize(st));         // (also: `tab` may go out of scope now)
        HIPCHK(c, hipGetLastError());
        if (arena_on && ((volatile u32*)c->mbox)[20] != 0)     // a pair with more keys than its arena row: the genomes sorted
            return collect_impl(c, ids, n, true);           // whole, and once more
        total = ((volatile u32*)c->mbox)[4];
        if (total > cap) {
            if ((rc = ensure_keep(c, c->records, (size_t)(done + total + 2) * sizeof(kr_record) * 5 / 4, (size_t)done * sizeof(kr_record))))
                return rc;
            StageScope sc(c, KR_ST_COLLECT);
            hipLaunchKernelGGL(k_collect_emit, dim3((np2 + 255) / 256), dim3(256), 0, st, cand, np2, ac, g,
                               (const u32*)c->collo.p, (const u32*)c->colpos.p, (const u64*)c->colfirst.p, (const u32*)c->colfm.p,
                               (kr_record*)c->records.p + done, 0xFFFFFFFFu);
            HIPCHK(c, hipStreamSynchronize(st));     // (rare path; it reads every genome's keys: a later sort on a lane must come behind it)
            HIPCHK(c, hipGetLastError());
        }
        done += total;
    }
    c->nrecords = (int64_t)done;
    return c->nrecords;
}

int64_t kr_fetch(kr_ctx* c, kr_record* out, size_t cap) {
    if (!c) return KR_ERR_PARAM;
    if ((size_t)c->nrecords > cap) return fail(c, KR_ERR_CAPACITY, "record buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->nrecords)
        HIPCHK(c, hipMemcpy(out, c->records.p, (size_t)c->nrecords * sizeof(kr_record), hipMemcpyDeviceToHost));
    return c->nrecords;
}

// h_wide.inc -- part of krisp_hip.hip (one translation unit): host: wide path driver (kr_wide_run, kr_wide_fetch)
// ----------------------------------------------------------------------------
// wide path driver
// ----------------------------------------------------------------------------
static int ceil_log2(u64 n) { int b = 0; while ((1ull << b) < n) b++; return b; }
static size_t free_bytes() { size_t fr = 0, tot = 0; return hipMemGetInfo(&fr, &tot) == hipSuccess ? fr : 0; }
// Memory is given back only when the next allocations would not fit (a repeated run finds every buffer of
// the previous one and allocates nothing: hipMalloc / hipFree of tens of GB cost more than the kernels).
// Before the locate pass its buffers of the previous run are the first to go.
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
static int wide_make_room(kr_ctx* c, size_t need) {
    if (free_bytes() >= need + ((size_t)1 << 30)) return KR_OK;
    auto& w = c->wide;
    HIPCHK(c, hipDeviceSynchronize());
    DevBuf* lb[] = {&w.masks, &w.keep, &w.cnt, &w.hitoff, &w.cursor, &w.hits, &w.cibuf, &w.loc};
    for (DevBuf* b : lb) release(c, *b);
    return KR_OK;
}

// sort every listed genome under the current c->g and intersect them (no filter): the
// candidates' prefixes, dense and sorted, go to `out` with a top-bits index
// (+ the one-sector slot form when it pays: see Dict in k_keys.inc)
// flank_len > 0: the keys are flanks of that many bases -- they may take the minimizer form instead.
static int64_t wide_phase(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, kr_ctx::Wide::DictBufs& d, int keybits,
                          int flank_len = 0, int count_windows_wk = 0, bool canonical = false) {
    DevBuf &out = d.keys, &idx = d.idx;
    int& ib = d.ib;
    d.sb = 0;
    d.mzlen = 0;
    d.canon = false;
    int rc;
    int64_t nc = -1;
    auto local = [&]() -> int64_t {
        int r2;
        // Round 6 (VERDICT r5 item 6): the streaming form.  The values present in EVERY genome are a running intersection --
        // monotone, like the masks of the packed path's candidates --, so the genomes may go through the sort in batches:
        // the first batch is intersected, every later batch looks the running list up in its sorted genomes
        // (kr_cands_probe: one step of the reference's merge tree, intersectAmplicons.py:256-307, on lists), and a batch's
        // sorted keys -- 16 bytes per base, the bulk of what a genome holds during a phase -- go back before the next
        // batch is sorted.  Same list as the one-shot intersection.
        const int B = (c->wide.batch > 0 && c->wide.batch < n) ? c->wide.batch : n;
        int64_t cur = -1;
        for (int b0 = 0; b0 < n; b0 += B) {
            const int b1 = std::min(n, b0 + B);
            for (int i = b0; i < b1; i++) {
                Genome& G = c->genomes[ids[i]];
                auto dense_cache = [&]() -> int {
                    int r3;
                    if ((r3 = ensure(c, G.wkeys, (G.nwords + PAD_WORDS) * 32 * 16))) return r3;
                    c->g.wcache = (u64*)G.wkeys.p;
                    c->g.wlcnt = nullptr;
                    c->g.wlcap = 0;
                    G.wlist = false;
                    return KR_OK;
                };
                if (c->g.wmode == 2 && c->wide.genome_cache) {
                    if (c->wide.key_list) {
                        // (Geom.wlcnt: a segment per workgroup of k_hist8w, sized for key_list_frac of its window starts)
                        const u64 per_wg = (G.nwords + NWG - 1) / NWG * 32;
                        const u32 cap = (u32)std::min<double>(4.0e9, (double)per_wg * c->wide.key_list_frac + 256.0);
                        if ((r2 = ensure(c, G.wkeys, (size_t)NWG * cap * 16 + 64))) return r2;
                        if ((r2 = ensure(c, G.wlcnt, (size_t)NWG * 4))) return r2;
                        c->g.wcache = (u64*)G.wkeys.p;
                        c->g.wlcnt = (u32*)G.wlcnt.p;
                        c->g.wlcap = cap;
                        G.wlist = true;
                        G.wlcap = cap;
                    } else if ((r2 = dense_cache())) return r2;
                }
                r2 = count_slices(c, G);
                if (r2 == KR_RETRY_DENSE) {
                    // a workgroup found more keys than its segment holds (the estimate was for unrelated flanks): this genome
                    // and the ones behind it take 16 bytes per window start as before
                    c->wide.key_list = false;
                    c->wide.key_list_failed = true;
                    if ((r2 = dense_cache())) return r2;
                    r2 = count_slices(c, G);
                }
                if (r2) return r2;
                if (count_windows_wk) {       // (the genome's bad bits are in its lane now: its amplicon-long windows, for the record count)
                    Lane& ln = c->lanes[c->next_lane];
                    hipLaunchKernelGGL(k_count_windows, dim3(1024), dim3(256), 0, ln.stream, (const u32*)ln.bad.p, G.nwords,
                                       count_windows_wk, (unsigned long long*)c->wide.wcount.p + i);
                }
                if ((r2 = genome_sort(c, ids[i], true))) return r2;
            }
            if (b0 == 0) cur = kr_intersect(c, ids, b1, is_in, 0);          // (more than 32 genomes: cascaded inside, on the device)
            else if (cur > 0) cur = cands_probe_impl(c, ids + b0, b1 - b0, is_in + b0, 0, true);
            if (cur < 0) return cur;
            if (B < n) {
                HIPCHK(c, hipDeviceSynchronize());
                for (int i = b0; i < b1; i++) {
                    Genome& G = c->genomes[ids[i]];
                    for (Slice& S : G.sl) {
                        release(c, S.keys); release(c, S.off); release(c, S.chunkstart); release(c, S.chunkdesc); release(c, S.ovf);
                        if (S.res >= 0) c->mb_free.push_back(S.res);
                    }
                    G.sl.clear();
                    G.sorted = G.finalized = G.ordered = false;
                }
            }
        }
        return cur;
    };
    nc = local();
    if ((rc = wide_agree(c, nc < 0 ? (int)nc : KR_OK))) return rc;
    if (kr_comm_world(c) > 1) {
        // several ranks, each with its own genomes: the lists are intersected over the ranks by the packed
        // path's tree reduction and the result returns to every rank -- every rank then builds the
        // same dictionary (the tables are deterministic), so ranks and composite keys agree everywhere
        if ((nc = kr_cands_reduce(c, 0)) < 0) return nc;
        if ((nc = kr_cands_bcast(c)) < 0) return nc;
    }
    if (nc >= (1ll << 32) - 1) return fail(c, KR_ERR_CAPACITY, "wide path: %lld dictionary entries (>= 2^32)", (long long)nc);
    hipStream_t st = c->stream;
    d.nfull = (u32)nc;
    if (canonical && nc > 0) {
        // Dict.canon: of a spectrum closed under reverse complement only the canonical flanks are kept (the list stays sorted)
        const u32 n0 = (u32)nc, nblk = (n0 + 255) / 256;
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
        if (2ull * kept - npal == n0) {      // (closed under reverse complement, as the packed spectra are: else the full list stays)
            nc = cands_compact_adopt(c, kept);
            d.canon = true;
        }
    }
    if ((rc = ensure(c, out, ((size_t)nc + 2) * 8))) return rc;
    if (nc)
        hipLaunchKernelGGL(k_cand_prefixes, dim3(((u32)nc + 255) / 256), dim3(256), 0, st, (const kr_cand*)c->candB.p,
                           (u32)nc, (u64*)out.p);
    d.n = (u32)nc;
    // minimizer form (see Dict): a minimizer is shared by ~9 consecutive windows, so occupied buckets hold ~9 keys or a
    // multiple; ~4 keys per bucket overall; counting sort by bucket, every bucket sorted by value
    if (flank_len >= MZ_MINLEN && !c->wide.ordered && nc > 0) {
        const u32 nb = (u32)std::max<int64_t>(1, nc / 4), bigcap = 1u << 16;
        const u32 ntiles = (nb + 2047) / 2048;
        auto& w = c->wide;
        {
            const size_t want[] = {((size_t)nc + 2) * 8, ((size_t)nb + 4) * 4, ((size_t)nc + 4 + bigcap) * 4};
            const size_t have[] = {d.mzT.bytes, d.mzB.bytes, idx.bytes};
            size_t need = 0;
            for (int q = 0; q < 3; q++) need += want[q] > have[q] ? want[q] : 0;
            if (need && (rc = wide_make_room(c, need))) return rc;
        }
        if ((rc = ensure(c, d.mzT, ((size_t)nc + 2) * 8))) return rc;
        if ((rc = ensure(c, d.mzB, ((size_t)nb + 4) * 4))) return rc;
        if ((rc = ensure(c, idx, ((size_t)nc + 4 + bigcap) * 4))) return rc;         // (scratch: places inside the buckets, list of big buckets)
        if ((rc = ensure(c, w.tsum, ((size_t)ntiles + 4) * 4))) return rc;
        if ((rc = ensure(c, w.tpos, ((size_t)ntiles + 4) * 4))) return rc;
        u32 *B = (u32*)d.mzB.p, *within = (u32*)idx.p, *big = (u32*)idx.p + nc + 2;
        HIPCHK(c, hipMemsetAsync(B, 0, ((size_t)nb + 4) * 4, st));
        HIPCHK(c, hipMemsetAsync(big, 0, 4, st));
        const u32 grid = ((u32)nc + 255) / 256;
        hipLaunchKernelGGL(k_mz_count, dim3(grid), dim3(256), 0, st, (const u64*)out.p, (u32)nc, flank_len, nb, B, within);
        hipLaunchKernelGGL(k_tile_sums, dim3(ntiles), dim3(256), 0, st, (const u32*)B, nb, (u32*)w.tsum.p);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)w.tsum.p, (u32*)w.tpos.p, ntiles);
        hipLaunchKernelGGL(k_tile_apply, dim3(ntiles), dim3(256), 0, st, (const u32*)B, nb, (const u32*)w.tpos.p, ntiles, B);
        hipLaunchKernelGGL(k_mz_scatter, dim3(grid), dim3(256), 0, st, (const u64*)out.p, (u32)nc, flank_len, nb,
                           (const u32*)B, (const u32*)within, (u64*)d.mzT.p);
        hipLaunchKernelGGL(k_mz_sort, dim3((nb + 255) / 256), dim3(256), 0, st, (u64*)d.mzT.p, (const u32*)B, nb, big, bigcap);
        u32 nbig = 0;
        HIPCHK(c, hipMemcpyAsync(&nbig, big, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (nbig <= bigcap) {
            if (nbig)
                hipLaunchKernelGGL(k_mz_sort_big, dim3(nbig), dim3(256), 0, st, (u64*)d.mzT.p, (const u32*)B, (const u32*)big);
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            d.mzlen = flank_len;
            d.mznb = nb;
            return nc;
        }
        // (more crowded buckets than the list holds: a degenerate spectrum; the forms below take it)
    }
    ib = std::max(1, std::min(std::min(27, keybits), ceil_log2((u64)nc + 1)));     // ~1 entry per index bucket
    // slots: 0.75 .. 1.5 keys per 32-byte slot when the 40 bits of an entry hold the rest of the key and the
    // table fits; the index is then built at the slot resolution (it also serves the crowded slots)
    int sb = std::max(1, std::min(std::min(31, keybits), ceil_log2((2 * (u64)nc + 2) / 3)));
    if (keybits - sb > 40 && (keybits - 40 <= 23 || keybits - 40 <= sb + 3))
        sb = keybits - 40;     // (few long keys: a sparser table, if it is small or at most 8 x the policy's)
    bool slots = c->wide.use_slots && nc > 0 && keybits - sb <= 40;
    if (slots) {
        const size_t want = ((size_t)32 << sb) + ((size_t)4 << sb), have = d.slots.bytes + idx.bytes;
        if (want > have && (rc = wide_make_room(c, want))) return rc;
        slots = want <= free_bytes() / 3 + have;
    }
    if (slots) ib = sb;
    if ((rc = ensure(c, idx, (((size_t)1 << ib) + 2) * 4))) return rc;
    if (slots && (rc = ensure(c, d.slots, (size_t)32 << sb))) return rc;
    HIPCHK(c, hipMemsetAsync(idx.p, 0xFF, (((size_t)1 << ib) + 1) * 4, st));
    if (nc)
        hipLaunchKernelGGL(k_index_sorted, dim3((u32)(((u64)nc + 255) / 256)), dim3(256), 0, st, (const u64*)out.p,
                           (u32)nc, ib, (u32*)idx.p);
    hipLaunchKernelGGL(k_index_fill, dim3((u32)((((u64)1 << ib) + 1 + 255) / 256)), dim3(256), 0, st,
                       (const u64*)out.p, (u32)nc, ib, (u32*)idx.p);
    if (slots) {
        hipLaunchKernelGGL(k_slot_build, dim3((u32)((((u64)1 << sb) + 255) / 256)), dim3(256), 0, st, (const u64*)out.p,
                           (const u32*)idx.p, sb, (uint4*)d.slots.p);
        d.sb = sb;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return nc;
}

static int64_t wide_run_once(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter);

// A genome set whose sorted keys do not fit the device at once (KR_ERR_CAPACITY from a phase) is run again with the sort +
// intersect phases in batches of half as many genomes, and again, down to one genome per batch (KR_WIDE_BATCH=n in the
// environment starts there: tests) -- with the per-window cache of composite keys in one lane buffer instead of one per
// genome.  What must stay resident for the locate pass -- the genomes' bases (1 byte per base) and the group of every
// window (8 bytes per base) -- still bounds a run: beyond that the call fails with KR_ERR_CAPACITY, as before round 6.
// Several ranks retry together (one all-reduce behind every attempt: a rank must not enter the next attempt's exchanges alone).
int64_t kr_wide_run(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    if (!c || !c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params_wide first");
    const char* eb = getenv("KR_WIDE_BATCH");
    const int env_batch = eb ? atoi(eb) : 0;
    int B = (env_batch > 0 && env_batch < n) ? env_batch : n;
    c->wide.key_list_failed = false;
    for (;;) {
        c->wide.batch = B < n ? B : 0;
        int64_t r = wide_run_once(c, ids, n, is_in, apply_filter);
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
            Genome& G = it->second;
            release(c, G.wkeys);
            for (Slice& S : G.sl) {
                release(c, S.keys); release(c, S.off); release(c, S.chunkstart); release(c, S.chunkdesc); release(c, S.ovf);
                if (S.res >= 0) c->mb_free.push_back(S.res);
            }
            G.sl.clear();
            G.sorted = G.finalized = G.ordered = false;
        }
        release(c, c->candA); release(c, c->candB); release(c, c->candP); release(c, c->other);
        c->ncand = -1;
        c->err.clear();
        B = (B + 1) / 2;
    }
}

static int64_t wide_run_once(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int apply_filter) {
    if (!c || !c->wide.on) return fail(c, KR_ERR_STATE, "kr_set_params_wide first");
    if (n < 1) return fail(c, KR_ERR_PARAM, "kr_wide_run: need at least one genome");
    for (int i = 0; i < n; i++) {
        auto it = c->genomes.find(ids[i]);
        if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", ids[i]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    auto& w = c->wide;
    struct LanesBack { kr_ctx::Wide& w; int lanes; ~LanesBack() { w.lanes = lanes; } } lanes_back{w, w.lanes};
    w.nhits = -1;
    w.nfin = 0;
    w.run_ids.assign(ids, ids + n);
    w.genome_cache = false;        // (decided for the final phase below; the flank phases keep no per-window cache)
    w.key_list = false;
    w.keys_listed = 0;
    const int sb = c->sb, b = c->g.b;
    {
        int rcf = ensure(c, w.flbuf, 8 * 2 * sizeof(FlankRank));
        if (rcf) return rcf;
    }
    // a spectrum phase: the `len` bases at forward offset fo (reverse strand: the reverse complement of
    // the bases at k - fo - len) of every valid window -> the values present in all genomes
    // With both strands in play the spectrum is taken over EVERY valid flank-long window of the genome with the packed
    // path's kernels (k_hist8 / k_scatter1p: 2.5 x the rate of the window-by-window generator): a superset of the
    // flanks of the valid amplicon-long windows, closed under reverse complement.  The groups do not change -- a
    // composite key present in every genome has its flanks at the ends of a valid window in every genome, so they
    // are in the narrower dictionary as well -- and the ranks stay order-preserving.  The genomes' record counts
    // (amplicon-long windows) then come from k_count_windows.
    bool counted = false;
    auto spectrum = [&](int f, int q, int fo, int len) -> int64_t {
        Geom g = make_geom(len, 0, 0, w.omit, sb, b);
        const bool packed = w.packed_spectrum && w.strands == 0;
        g.wmode = packed ? 0 : 1;
        g.wk = w.k;
        g.wlen = len;
        g.wfo = fo;
        g.wro = w.k - fo - len;
        g.strands = w.strands;
        c->g = g;
        int cw = 0;
        if (packed && !counted) {
            int rcw = ensure(c, w.wcount, (size_t)n * 8 + 8);
            if (rcw) return rcw;
            HIPCHK(c, hipMemset(w.wcount.p, 0, (size_t)n * 8));
            cw = w.k;
        }
        // one spectrum for both flanks (w.share), taken over every flank-long window of both strands, one piece: the
        // dictionary keeps the canonical flanks only (Dict.canon; KR_WIDE_CANON=0: the full list, A/B and tests)
        static const bool canon_on = [] { const char* e = getenv("KR_WIDE_CANON"); return e ? atoi(e) != 0 : true; }();
        const bool canon = canon_on && packed && w.share && kr_ctx::Wide::fd_pieces(f == 0 ? w.L : w.R) == 1;
        const int64_t r = wide_phase(c, ids, n, is_in, w.fd[f][q], 2 * len, len, cw, canon);
        if (cw && r >= 0) {
            std::vector<unsigned long long> wc(n);
            HIPCHK(c, hipMemcpy(wc.data(), w.wcount.p, (size_t)n * 8, hipMemcpyDeviceToHost));
            w.nkeys.clear();
            for (int i = 0; i < n; i++) w.nkeys.push_back(2ull * wc[i]);
            counted = true;
        }
        return r;
    };
    auto one_level = [&](int f, int q, int len) {
        FlankRank F{};
        F.len = F.plen[0] = len;
        F.poff[0] = 0;
        F.np = 1;
        F.d[0] = w.fd[f][q].view();
        return F;
    };
    // composite geometry over two ranked parts: bit widths from the dictionary sizes, room for the slice digits
    auto composite = [&](const FlankRank& P0, u32 n0, int off0, const FlankRank& P1, u32 n1, int off1, int& bits) {
        int bits0 = std::max(1, ceil_log2((u64)n0 + 1)), bits1 = std::max(1, ceil_log2(n1));
        if ((bits0 + bits1) & 1) bits1++;
        while (bits0 + bits1 < 2 * sb + 2) bits1 += 2;
        bits = bits0 + bits1;
        Geom g = make_geom(bits / 2, 0, 0, w.omit, sb, b);
        g.wmode = 2;
        g.wk = w.k;
        g.wshL = 64 - bits0;
        g.wshR = 64 - bits0 - bits1;
        g.woff[0] = off0;
        g.woff[1] = off1;
        // the two parts' dictionaries go to the next pair of the device table (synchronous copy: the pair is in place
        // before any launch that names it; the pair before stays for the kernels still reading it)
        w.flslot = (w.flslot + 1) % 8;
        w.flhost[w.flslot][0] = P0;
        w.flhost[w.flslot][1] = P1;
        g.wfl = (const FlankRank*)w.flbuf.p + 2 * w.flslot;
        (void)hipMemcpy((void*)g.wfl, w.flhost[w.flslot], 2 * sizeof(FlankRank), hipMemcpyHostToDevice);
        g.strands = w.strands;
        return g;
    };
    // phases 1 / 2: `left` and `right` ranked -- one spectrum each, or (longer than 32 bases) the
    // spectrum of the first 32 bases, the spectrum of the rest and the combinations of their ranks
    // (see Geom.wshare) one spectrum serves both flanks
    // (mixed DNA / RNA runs: a group and its mirror are no longer decided alike -- the column where one holds T against U holds
    // A against A in the other, the complement of both -- so every group is located and filtered by itself)
    w.share = !w.ordered && w.use_share && w.L == w.R && w.strands == 0 && !c->mixed_alphabets;
    for (int f = 0; f < (w.share ? 1 : 2); f++) {
        const int len = f == 0 ? w.L : w.R;
        const int fo = f == 0 ? 0 : w.k - w.R;              // forward offset of the flank in the window
        const int len1 = kr_ctx::Wide::fd_plen(len, 0);
        int64_t nd = spectrum(f, 0, fo, len1);
        if (nd < 0) return nd;
        if (f == 0 && !counted) {          // one key per strand of every valid window = the genome's k-mer records
            w.nkeys.clear();
            for (int i = 0; i < n; i++) w.nkeys.push_back(c->genomes[ids[i]].nmax);
        }
        if (nd == 0) { w.nhits = 0; return 0; }
        w.fr[f] = one_level(f, 0, len1);
        // longer than 32 bases: piece by piece -- the spectrum of piece j, then the combinations (rank of pieces 0 .. j - 1,
        // rank of piece j) present in every genome, ranked again (two sort + intersect phases per further piece)
        u32 nsofar = w.fd[f][0].n;
        for (int j = 1; j < kr_ctx::Wide::fd_pieces(len); j++) {
            const int lj = kr_ctx::Wide::fd_plen(len, j), oj = kr_ctx::Wide::fd_poff(len, j);
            if ((nd = spectrum(f, 2 * j - 1, fo + oj, lj)) < 0) return nd;
            if (nd == 0) { w.nhits = 0; return 0; }
            int bits = 0;
            Geom g = composite(w.fr[f], nsofar, fo, one_level(f, 2 * j - 1, lj), w.fd[f][2 * j - 1].n, fo + oj, bits);
            g.wcache = nullptr;
            c->g = g;
            if ((nd = wide_phase(c, ids, n, is_in, w.fd[f][2 * j], bits)) < 0) return nd;
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
    // phase 3: composite keys rank(left) : rank(right)
    {
        // (a canonical dictionary of n keys hands out ids below 2 n)
        auto ids_of = [](const kr_ctx::Wide::DictBufs& dd) { return dd.canon ? 2u * dd.n : dd.n; };
        const u32 nL = ids_of(w.fd[0][kr_ctx::Wide::fd_last(w.L)]), nR = w.share ? nL : ids_of(w.fd[1][kr_ctx::Wide::fd_last(w.R)]);
        int bits = 0;
        Geom g = composite(w.fr[0], nL, 0, w.share ? w.fr[0] : w.fr[1], nR, w.k - w.R, bits);
        g.wshare = w.share ? 1 : 0;
        // composite keys are generated once per genome and phase (16 bytes per window start).
        // Kept per genome when that fits comfortably -- the locate pass then reads them too and
        // leaves each window's group in their place -- else in one lane buffer (sort passes only)
        w.genome_cache = false;
        // Round 6: the composite keys as a LIST per genome (Geom.wlcnt) where few window starts have one -- both flanks in the
        // dictionaries.  The canonical dictionary holds nfull flanks (both orientations) of a genome's 2 x bases flank
        // occurrences: a share f of the starts has its left flank there, f^2 both if flanks went independently; conserved
        // stretches cluster (2.2 x f^2 at configs[2]), so the segments are sized for 6 f^2 + 0.2 % -- and a run whose
        // genomes are close relatives (f -> 1) keeps 16 bytes per start: there most starts have a key.  A segment that
        // turns out too short makes the run fall back by itself (count_slices).  KR_WIDE_KEYLIST=0: dense (A/B, tests);
        // KR_WIDE_KEYFRAC: the share to size for (tests: the fall-back)
        {
            const FlankRank& F0 = w.fr[0];
            const bool canon_form = w.share && F0.np == 1 && F0.d[0].canon && w.k - F0.len <= H8W_HALO;     // (what k_hist8w's tiled form takes)
            u64 minb = ~0ull;
            for (int i = 0; i < n; i++) minb = std::min<u64>(minb, c->genomes[ids[i]].n_bases);
            const double f = std::min(1.0, (double)w.fd[0][kr_ctx::Wide::fd_last(w.L)].nfull / (2.0 * (double)std::max<u64>(minb, 1)));
            double frac = std::min(1.0, 6.0 * f * f + 0.002);
            if (getenv("KR_WIDE_KEYFRAC")) frac = atof(getenv("KR_WIDE_KEYFRAC"));
            const bool on = getenv("KR_WIDE_KEYLIST") ? atoi(getenv("KR_WIDE_KEYLIST")) != 0 : true;
            w.key_list = on && canon_form && !w.key_list_failed && frac <= 0.125;
            w.key_list_frac = frac;
        }
        {
            size_t need = 0, fr = 0, tot = 0, slotbytes = 0;
            for (int f = 0; f < 2; f++)
                for (int q = 0; q < 2 * FR_MAXP - 1; q++)      // (released once the composite keys exist)
                    slotbytes += w.fd[f][q].slots.bytes + (w.fd[f][q].mzlen ? w.fd[f][q].mzT.bytes + w.fd[f][q].mzB.bytes : 0);
            for (int i = 0; i < n; i++) {       // what is still to be allocated (a repeated run has its caches)
                const Genome& G = c->genomes[ids[i]];
                const size_t want = w.key_list ? (size_t)NWG * (size_t)((double)((G.nwords + NWG - 1) / NWG * 32) * w.key_list_frac + 256.0) * 16 + 64
                                               : (G.nwords + PAD_WORDS) * 32 * 16;
                if (want > G.wkeys.bytes) need += want;
            }
            if (need) {
                // first run: the candidate buffers of the flank phases are dictionary-sized and the group
                // phase sizes its own; the locate buffers of an earlier run with other sizes go too
                HIPCHK(c, hipDeviceSynchronize());
                release(c, c->candA);
                release(c, c->candB);
                c->ncand = -1;
                int rcm = wide_make_room(c, need * 5 / 2);
                if (rcm) return rcm;
            }
            (void)tot;
            fr = free_bytes();
            if (getenv("KR_WIDE_CACHE")) w.genome_cache = atoi(getenv("KR_WIDE_CACHE")) != 0;
            else w.genome_cache = (!w.batch || w.key_list) && (need == 0 || need <= (fr + slotbytes) / 5 * 2);      // (batches: memory is short -- a list is small)
            if (!w.genome_cache) w.key_list = false;            // (ONE cache for all genomes: the dense form)
            if (!w.genome_cache) {
                w.lanes = 1;          // (ONE cache of composite keys, in lane 0's scratch: one lane for the rest of this run)
                int rcw = ensure(c, c->lanes[0].wkeys, ((c->max_bases + 31) / 32 + PAD_WORDS) * 32 * 16);
                if (rcw) return rcw;
                g.wcache = (u64*)c->lanes[0].wkeys.p;
            }
        }
        c->g = g;
        int64_t nf = wide_phase(c, ids, n, is_in, w.fin, bits);
        if (nf < 0) return nf;
        w.nfin = (u32)nf;
        w.ngroups = (u64)nf;
        if (w.share && nf) {
            // the list holds one group of every mirror pair (Geom.wshare): the (left,right) groups present in all
            // genomes are twice as many, less the groups that mirror themselves
            if (nf >= (1ll << 31)) return fail(c, KR_ERR_CAPACITY, "wide path: %lld canonical groups (>= 2^31)", (long long)nf);
            u32 npal = 0;
            int rcp = ensure(c, w.tsum, 64);
            if (rcp) return rcp;
            HIPCHK(c, hipMemsetAsync(w.tsum.p, 0, 4, c->stream));
            hipLaunchKernelGGL(k_count_selfmirror, dim3(((u32)nf + 255) / 256), dim3(256), 0, c->stream, (const u64*)w.fin.keys.p,
                               (u32)nf, g.wshL, g.wshR, g.wshL - g.wshR, (u32*)w.tsum.p);
            HIPCHK(c, hipMemcpyAsync(&npal, w.tsum.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            w.ngroups = 2 * (u64)nf - npal;
        }
        if (nf == 0) { w.nhits = 0; return 0; }
    }
    // members of the groups: masks + counts, filter, hits
    int rc;
    const u32 nf = w.nfin;
    const int W = std::max(1, w.W);
    bool use_list = false;
    u64 loc_cap = 0;
    DevBuf* loc_borrow = nullptr;
    {
        // what the locate pass still has to allocate; when that does not fit: the flank dictionaries' tables
        // first (with the composite keys of every window cached they have done their work), then the
        // candidate buffers, then the sorted composite keys
        const size_t kw = (size_t)nf / 64 + 2;
        const size_t want[] = {(size_t)nf * 2 * W * 8, ((kw + 63) / 64 * 64 + kw / 64 + 2) * 8, ((size_t)nf + 4) * 4,
                               ((size_t)nf + 4) * 4, ((size_t)nf + 4) * 4};
        const size_t have[] = {w.masks.bytes, w.keep.bytes, w.cnt.bytes, w.hitoff.bytes, w.cursor.bytes};
        size_t need = 0;
        for (int q = 0; q < 5; q++) need += want[q] > have[q] ? want[q] : 0;
        u64 npos_all = 0;
        for (int i = 0; i < n; i++) npos_all += c->genomes[ids[i]].n_bases;
        // round 6: the member windows as a LIST when that is the smaller thing to write and read (k_wide_locate): room for
        // two members per group and genome (more -- repeats -- : the dense form runs after all); KR_WIDE_LOCLIST=0: dense
        // (A/B, tests), KR_WIDE_LOCCAP: the list's room in entries (tests: the overflow)
        const int loclist = getenv("KR_WIDE_LOCLIST") ? atoi(getenv("KR_WIDE_LOCLIST")) : 1;
        const u64 loccap_env = getenv("KR_WIDE_LOCCAP") ? (u64)atoll(getenv("KR_WIDE_LOCCAP")) : 0ull;
        loc_cap = loccap_env ? loccap_env : 2 * (u64)nf * (u64)n + (1u << 20);
        loc_cap = loc_cap / WIDE_SEGS * WIDE_SEGS;                  // (WIDE_SEGS lists of loc_cap / WIDE_SEGS entries)
        use_list = loclist != 0 && loc_cap < (1ull << 31) && (loccap_env || loc_cap * 16 <= npos_all * 4 + ((u64)64 << 20));
        if (use_list) {
            // the list lives for the locate / count / emit passes only, when every sort of the run is over: the first sort
            // lane's pass-0 or pass-1 scratch holds it when large enough (configs[2]: 0.8 GB in an idle 8 GB array -- a
            // buffer of its own would push a run planned to the device's last GB into giving memory back every time)
            Lane& l0 = c->lanes[0];
            const size_t lb = (size_t)loc_cap * 16 + 64;
            loc_borrow = l0.pass0.bytes >= lb ? &l0.pass0 : (l0.tmpkeys.bytes >= lb ? &l0.tmpkeys : nullptr);
            if (!loc_borrow) need += lb > w.loc.bytes ? lb : 0;
        }
        if (!w.genome_cache && !use_list) {
            size_t ci = 2 * sizeof(uint2);
            for (int i = 0; i < n; i++) ci += c->genomes[ids[i]].n_bases * sizeof(uint2);
            need += ci > w.cibuf.bytes ? ci : 0;
        }
        const size_t margin = (size_t)2 << 30;
        if (need && free_bytes() < need + margin) {
            HIPCHK(c, hipDeviceSynchronize());
            if (w.genome_cache) {
                for (int f = 0; f < 2; f++) {
                    for (int q = 0; q < 2 * FR_MAXP - 1; q++) {
                        auto& d = w.fd[f][q];
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
            if (free_bytes() < need + margin) {
                release(c, c->candA);
                release(c, c->candB);
                c->ncand = -1;
            }
            if (free_bytes() < need + margin) {
                for (int i = 0; i < n; i++) {
                    Genome& G = c->genomes[ids[i]];
                    for (Slice& S : G.sl) {
                        release(c, S.keys); release(c, S.off); release(c, S.chunkstart); release(c, S.chunkdesc); release(c, S.ovf);
                        if (S.res >= 0) c->mb_free.push_back(S.res);
                    }
                    G.sl.clear();
                    G.sorted = G.finalized = G.ordered = false;
                }
            }
        }
    }
    const size_t kwords = (size_t)nf / 64 + 2, ksum_off = (kwords + 63) / 64 * 64;     // keep bits, then their summary bits
    hipStream_t st = c->stream;
    Lane& ln = c->lanes[0];
    // the group of every window of every genome (8 bytes per base): written by the locate pass,
    // streamed by the emit pass once the filter has decided
    std::vector<u64> cioff(n + 1, 0);
    for (int i = 0; i < n; i++) cioff[i + 1] = cioff[i] + c->genomes[ids[i]].n_bases;
    bool any_wlist = false;
    for (int i = 0; i < n; i++) any_wlist = any_wlist || (w.genome_cache && c->genomes[ids[i]].wlist);
    auto locate_buffers = [&]() -> int {
        int r2;
        if ((r2 = ensure(c, w.masks, (size_t)nf * 2 * W * 8))) return r2;
        if ((r2 = ensure(c, w.keep, (ksum_off + kwords / 64 + 2) * 8))) return r2;
        if ((r2 = ensure(c, w.cnt, ((size_t)nf + 4) * 4))) return r2;
        if ((r2 = ensure(c, w.hitoff, ((size_t)nf + 4) * 4))) return r2;
        if ((r2 = ensure(c, w.cursor, ((size_t)nf + 4) * 4))) return r2;
        if ((r2 = join_lanes(c))) return r2;
        HIPCHK(c, hipMemsetAsync(w.masks.p, 0, (size_t)nf * 2 * W * 8, st));
        HIPCHK(c, hipMemsetAsync(w.cnt.p, 0, ((size_t)nf + 4) * 4, st));
        HIPCHK(c, hipMemsetAsync((u64*)w.keep.p + ksum_off, 0, (kwords / 64 + 2) * 8, st));
        HIPCHK(c, hipMemsetAsync(w.cursor.p, 0, ((size_t)nf + 4) * 4, st));
        if (use_list) {
            if (!loc_borrow && (r2 = ensure(c, w.loc, (size_t)loc_cap * 16 + 64))) return r2;
            if ((r2 = ensure(c, w.loccur, WIDE_SEGS * WIDE_SEG_STRIDE * 4))) return r2;
            HIPCHK(c, hipMemsetAsync(w.loccur.p, 0, WIDE_SEGS * WIDE_SEG_STRIDE * 4, st));
        } else if ((!w.genome_cache || any_wlist) && (r2 = ensure(c, w.cibuf, (cioff[n] + 2) * sizeof(uint2)))) return r2;
        return KR_OK;
    };
    // where the dense form keeps genome i's group numbers: in place of its per-window cache (stride 2), or -- no such cache,
    // or the genome's keys are a list -- in the run's own buffer
    auto dense_ci = [&](int i, u32& stride) -> uint2* {
        Genome& G = c->genomes[ids[i]];
        if (w.genome_cache && !G.wlist) { stride = 2u; return (uint2*)G.wkeys.p; }
        stride = 1u;
        return (uint2*)w.cibuf.p + cioff[i];
    };
    const int world = kr_comm_world(c), rank = kr_comm_rank(c);
    auto locate_all = [&]() {
        for (int i = 0; i < n; i++) {
            Genome& G = c->genomes[ids[i]];
            if (G.n_bases == 0) continue;
            launch_pack(c, G, ln, st);
            const u32 grid = (u32)std::min<u64>((G.n_bases + 255) / 256, 16384);
            Geom g = c->g;
            g.wcmode = 0;
            g.wcache = nullptr;
            g.wlcnt = nullptr;
            g.wlcap = 0;
            u32 stride = 1;
            uint2* ci = dense_ci(i, stride);
            if (w.genome_cache && !G.wlist) {
                g.wcache = (u64*)G.wkeys.p;
                g.wcmode = 2;
            }
            uint4* locp = use_list ? (uint4*)(loc_borrow ? loc_borrow->p : w.loc.p) : (uint4*)nullptr;
            const u32 gidx = world > 1 ? (u32)ids[i] : (u32)i;      // (several ranks: a hit names its genome by the caller's id, the lists of all ranks meet on rank 0)
            StageScope sc(c, KR_ST_LOCATE, st);
            if (G.wlist && use_list) {
                // the genome's keys are a list (Geom.wlcnt): the locate pass walks it
                g.wcache = (u64*)G.wkeys.p;
                g.wlcnt = (u32*)G.wlcnt.p;
                g.wlcap = G.wlcap;
                g.wcmode = 4;
                hipLaunchKernelGGL(k_wide_locate_list, dim3(NWG), dim3(256), 0, st, (const u64*)ln.codes.p, g, w.fin.view(), w.D, W,
                                   is_in[i] ? 0u : 1u, (u64*)w.masks.p, locp, (u32*)w.loccur.p, (u32)(loc_cap / WIDE_SEGS), gidx);
                continue;
            }
            // (a key-list genome in a run whose members are too many to list: its keys are made again, window by window)
            if (use_list)
                hipLaunchKernelGGL(k_wide_locate<true>, dim3(grid), dim3(256), 0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p,
                                   (u64)G.n_bases, g, w.fin.view(), w.D, W, is_in[i] ? 0u : 1u, (u64*)w.masks.p, ci,
                                   stride, locp, (u32*)w.loccur.p, (u32)(loc_cap / WIDE_SEGS), gidx);
            else
                hipLaunchKernelGGL(k_wide_locate<false>, dim3(grid), dim3(256), 0, st, (const u64*)ln.codes.p, (const u32*)ln.bad.p,
                                   (u64)G.n_bases, g, w.fin.view(), w.D, W, is_in[i] ? 0u : 1u, (u64*)w.masks.p, ci,
                                   stride, locp, (u32*)w.loccur.p, (u32)(loc_cap / WIDE_SEGS), gidx);
        }
    };
    if ((rc = wide_agree(c, locate_buffers()))) return rc;      // (several ranks: all or none go on to the exchange)
    locate_all();
    u32 nloc = 0;
    w.located = 0;
    int rcd = KR_OK;
    if (use_list) {
        // how many were listed: more than the list holds (a genome set full of repeats) -> the dense form, from the start
        // (the masks only gain bits they already have)
        std::vector<u32> cur(WIDE_SEGS * WIDE_SEG_STRIDE);
        HIPCHK(c, hipMemcpyAsync(cur.data(), w.loccur.p, cur.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        bool over = false;
        u64 sum = 0;
        for (u32 sg = 0; sg < WIDE_SEGS; sg++) {
            over = over || cur[sg * WIDE_SEG_STRIDE] > loc_cap / WIDE_SEGS;
            sum += cur[sg * WIDE_SEG_STRIDE];
        }
        nloc = (u32)std::min<u64>(sum, 0xFFFFFFFFu);
        if (over) {
            use_list = false;
            nloc = 0;
            if (!w.genome_cache || any_wlist) rcd = ensure(c, w.cibuf, (cioff[n] + 2) * sizeof(uint2));
            if (!rcd) locate_all();
        }
        w.located = nloc;
    }
    // (several ranks: every rank comes here once, whichever form its own genomes took -- the forms are chosen rank by rank)
    if ((rc = wide_agree(c, rcd))) return rc;
    hipLaunchKernelGGL(k_wide_filter, dim3((nf + 255) / 256), dim3(256), 0, st, (const u64*)w.masks.p, (u64*)w.keep.p,
                       (u64*)w.keep.p + ksum_off, nf, w.D, W, fmode(c, apply_filter));
    if (world > 1 && apply_filter) {
        // the masks above hold this rank's genomes only.  The filter is monotone (masks only grow), so a
        // group this rank drops is dropped for good; the groups it keeps travel with their mask words,
        // one 16-column word per round, through the candidate tree reduction (intersection of the ranks'
        // kept sets, masks OR-ed); rank 0 then filters on the complete masks and broadcasts the survivors
        const u32 nwords = (nf + 63) / 64, ntl = (nwords + 2047) / 2048;
        u32* po = (u32*)w.hitoff.p;        // (free until the scan of the member counts)
        if ((rc = ensure(c, w.tsum, ((size_t)ntl + 4) * 4))) return rc;
        if ((rc = ensure(c, w.tpos, ((size_t)ntl + 4) * 4))) return rc;
        auto pack_list = [&](int wd) -> int64_t {          // kept groups of this rank -> candidate records in c->candB
            hipLaunchKernelGGL(k_keep_popc, dim3((nwords + 255) / 256), dim3(256), 0, st, (const u64*)w.keep.p, nwords, po);
            hipLaunchKernelGGL(k_tile_sums, dim3(ntl), dim3(256), 0, st, (const u32*)po, nwords, (u32*)w.tsum.p);
            hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)w.tsum.p, (u32*)w.tpos.p, ntl);
            hipLaunchKernelGGL(k_tile_apply, dim3(ntl), dim3(256), 0, st, (const u32*)po, nwords, (const u32*)w.tpos.p, ntl, po);
            u32 ns = 0;
            HIPCHK(c, hipMemcpyAsync(&ns, po + nwords, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            int r2;
            if ((r2 = ensure(c, c->candB, ((size_t)ns + 2) * sizeof(kr_cand)))) return r2;
            if ((r2 = ensure(c, c->candA, ((size_t)ns + 2) * sizeof(kr_cand)))) return r2;
            hipLaunchKernelGGL(k_wide_pack, dim3((nwords + 255) / 256), dim3(256), 0, st, (const u64*)w.keep.p, (const u32*)po,
                               nwords, (const u64*)w.masks.p, W, wd, (kr_cand*)c->candB.p);
            c->ncand = ns;
            return ns;
        };
        int64_t ns = 0;
        for (int wd = 0; wd < W; wd++) {
            ns = pack_list(wd);
            if ((rc = wide_agree(c, ns < 0 ? (int)ns : KR_OK))) return rc;      // (all ranks enter the reduction, or none)
            if ((ns = kr_cands_reduce(c, 0)) < 0) return ns;
            if (rank == 0 && ns)
                hipLaunchKernelGGL(k_wide_unpack, dim3(((u32)ns + 255) / 256), dim3(256), 0, st, (const kr_cand*)c->candB.p,
                                   (u32)ns, (u64*)w.masks.p, W, wd);
        }
        const size_t keep_bytes = (ksum_off + kwords / 64 + 2) * 8;
        if (rank == 0) {
            HIPCHK(c, hipMemsetAsync(w.keep.p, 0, keep_bytes, st));
            if (ns)
                hipLaunchKernelGGL(k_wide_relist, dim3(((u32)ns + 255) / 256), dim3(256), 0, st, (const kr_cand*)c->candB.p,
                                   (u32)ns, (const u64*)w.masks.p, w.D, W, fmode(c, 1), (u64*)w.keep.p, (u64*)w.keep.p + ksum_off);
            if ((ns = pack_list(0)) < 0) c->ncand = -1;                         // (the broadcast's agreement tells the others)
        }
        if ((ns = kr_cands_bcast(c)) < 0) return ns;
        if (rank != 0) {
            HIPCHK(c, hipMemsetAsync(w.keep.p, 0, keep_bytes, st));
            if (ns)
                hipLaunchKernelGGL(k_wide_relist, dim3(((u32)ns + 255) / 256), dim3(256), 0, st, (const kr_cand*)c->candB.p,
                                   (u32)ns, (const u64*)w.masks.p, w.D, W, 0, (u64*)w.keep.p, (u64*)w.keep.p + ksum_off);
        }
    }
    // members per kept group (the windows' groups are streamed again; only kept groups are counted)
    if (use_list && nloc)
        hipLaunchKernelGGL(k_wide_count_list, dim3((u32)((loc_cap / WIDE_SEGS + 255) / 256), WIDE_SEGS), dim3(256), 0, st,
                           (const uint4*)(loc_borrow ? loc_borrow->p : w.loc.p), (const u32*)w.loccur.p, (u32)(loc_cap / WIDE_SEGS),
                           (const u64*)w.keep.p, (const u64*)w.keep.p + ksum_off, (u32*)w.cnt.p, w.share ? 1 : 0);
    for (int i = 0; i < n && !use_list; i++) {
        Genome& G = c->genomes[ids[i]];
        if (G.n_bases == 0) continue;
        const u32 grid = (u32)std::min<u64>((G.n_bases + 255) / 256, 16384);
        u32 stride = 1;
        const uint2* ci = dense_ci(i, stride);
        hipLaunchKernelGGL(k_wide_count, dim3(grid), dim3(256), 0, st, ci, stride, (u64)G.n_bases,
                           (const u64*)w.keep.p, (const u64*)w.keep.p + ksum_off, (u32*)w.cnt.p, w.share ? 1 : 0);
    }
    {
        const u32 ntiles = (nf + 2047) / 2048;
        if ((rc = ensure(c, w.tsum, ((size_t)ntiles + 4) * 4))) return rc;
        if ((rc = ensure(c, w.tpos, ((size_t)ntiles + 4) * 4))) return rc;
        hipLaunchKernelGGL(k_tile_sums, dim3(ntiles), dim3(256), 0, st, (const u32*)w.cnt.p, nf, (u32*)w.tsum.p);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, (const u32*)w.tsum.p, (u32*)w.tpos.p, ntiles);
        hipLaunchKernelGGL(k_tile_apply, dim3(ntiles), dim3(256), 0, st, (const u32*)w.cnt.p, nf, (const u32*)w.tpos.p,
                           ntiles, (u32*)w.hitoff.p);
    }
    u32 total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, (u32*)w.hitoff.p + nf, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    w.nhits = total;
    if (total == 0 && world == 1) return 0;
    if ((rc = ensure(c, w.hits, ((size_t)total + 2) * sizeof(wide_hit)))) return rc;
    if (use_list && nloc && total)
        hipLaunchKernelGGL(k_wide_emit_list, dim3((u32)((loc_cap / WIDE_SEGS + 255) / 256), WIDE_SEGS), dim3(256), 0, st,
                           (const uint4*)(loc_borrow ? loc_borrow->p : w.loc.p), (const u32*)w.loccur.p, (u32)(loc_cap / WIDE_SEGS),
                           (const u64*)w.keep.p, (const u64*)w.keep.p + ksum_off, (const u32*)w.hitoff.p, (u32*)w.cursor.p,
                           (wide_hit*)w.hits.p, w.share ? 1 : 0);
    for (int i = 0; i < n && total && !use_list; i++) {
        Genome& G = c->genomes[ids[i]];
        if (G.n_bases == 0) continue;
        const u32 grid = (u32)std::min<u64>((G.n_bases + 255) / 256, 16384);
        u32 stride = 1;
        const uint2* ci = dense_ci(i, stride);
        // (several ranks: a hit names its genome by the caller's id, the lists of all ranks meet on rank 0)
        hipLaunchKernelGGL(k_wide_emit, dim3(grid), dim3(256), 0, st, ci, stride, (u64)G.n_bases,
                           world > 1 ? (u32)ids[i] : (u32)i, (const u64*)w.keep.p, (const u64*)w.keep.p + ksum_off,
                           (const u32*)w.hitoff.p, (u32*)w.cursor.p, (wide_hit*)w.hits.p, w.share ? 1 : 0);
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (world > 1) {
        // the hits of every rank -> rank 0, through the record gather (a hit is 16 bytes, as a record is)
        static_assert(sizeof(wide_hit) == sizeof(kr_record), "hits travel as records");
        if ((rc = ensure(c, c->records, ((size_t)total + 2) * sizeof(kr_record)))) return rc;
        if (total) HIPCHK(c, hipMemcpyAsync(c->records.p, w.hits.p, (size_t)total * sizeof(wide_hit), hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->nrecords = total;
        const int64_t all = kr_records_gather(c);
        if (all < 0) return all;
        if (rank == 0) {
            if ((rc = ensure(c, w.hits, ((size_t)all + 2) * sizeof(wide_hit)))) return rc;
            if (all) HIPCHK(c, hipMemcpy(w.hits.p, c->records.p, (size_t)all * sizeof(wide_hit), hipMemcpyDeviceToDevice));
            w.nhits = all;
        }
        c->nrecords = 0;
    }
    return w.nhits;
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
        const int sh = 64 - 2 * len;
        for (u64 x : v) {
            u64 y = ~x;                                     // complement, then reverse the 2-bit groups
            y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
            y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
            y = __builtin_bswap64(y) << sh;
            if (y != x) all.push_back(y);
        }
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
            const int sh = 64 - 2 * w.L;
            for (size_t i = 0; i < n; i++) {
                u64 y = ~o[i];                                  // complement, then reverse the 2-bit groups
                y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
                y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
                y = __builtin_bswap64(y);
                o[i] = (y << sh);                               // (the flank's bases were the top 2 L bits)
            }
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
    case KR_WIDE_BATCH_USED: {
        const u64 v = (u64)w.batch;
        if (!out) return 1;
        if (cap_bytes < 8) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (8 bytes needed)");
        memcpy(out, &v, 8);
        return 1;
    }
    case KR_WIDE_KEYS_LISTED: {
        const u64 v = w.keys_listed;
        if (!out) return 1;
        if (cap_bytes < 8) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (8 bytes needed)");
        memcpy(out, &v, 8);
        return 1;
    }
    case KR_WIDE_LOCATED: {
        const u64 v = w.located;
        if (!out) return 1;
        if (cap_bytes < 8) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (8 bytes needed)");
        memcpy(out, &v, 8);
        return 1;
    }
    case KR_WIDE_NGROUPS: {
        const u64 v = w.ngroups;
        if (!out) return 1;
        if (cap_bytes < 8) return fail(c, KR_ERR_CAPACITY, "kr_wide_fetch: buffer too small (8 bytes needed)");
        memcpy(out, &v, 8);
        return 1;
    }
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

// h_misc.inc -- part of krisp_hip.hip (one translation unit): host: timing aids, sync, timers, stage timers, debug fetch, FASTA text parser
// timing aid: run the LDS sort `reps` times over the (already sorted) slice 0 of a genome;
// returns the average milliseconds per launch (mode must be 0: the kernel as shipped).
double kr_debug_localsort(kr_ctx* c, int id, int reps, int mode) {
    if (!c || mode != 0) return -1.0;
    auto it = c->genomes.find(id);
    if (it != c->genomes.end() && ensure_fine(c, it->second)) return -1.0;
    if (it == c->genomes.end() || !it->second.sorted || it->second.sl.empty()) return -1.0;
    if (ensure_ordered(c, {&it->second}) || finalize(c, {&it->second})) return -1.0;
    Slice& S = it->second.sl[0];
    hipStream_t st = c->stream;
    const u32 grid = std::min<u32>(S.nchunks, (u32)c->ls_grid);
    auto launch = [&]() {
        hipLaunchKernelGGL(k_localsort2, dim3(grid), dim3(LS_THREADS), 0, st, (u64*)S.keys.p, (const u32*)S.off.p,
                           (const uint4*)S.chunkdesc.p, S.nchunks, c->g.b, (u32*)S.ovf.p,
                           (uint4*)((char*)S.ovf.p + 16));
    };
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    launch();       // warm-up
    (void)hipEventRecord(a, st);
    for (int r = 0; r < reps; r++) launch();
    (void)hipEventRecord(b, st);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return reps > 0 ? (double)ms / reps : 0.0;
}

// timing aid (tools/isect_ablate.py): kr_intersect's kernel `reps` times over sorted genomes with
// parts switched off: mode 0 = as it is, 64 = keys streamed but not probed, 128 = probed without
// the LDS update.  The candidate set is left invalid.  Average milliseconds per call.
double kr_debug_intersect(kr_ctx* c, const int* ids, int n, const uint8_t* is_in, int reps, int mode) {
    if (!c || reps < 1) return -1.0;
#ifndef KR_ABLATE
    if (mode & ~32) return -1.0;        // the ablation switches change results: -DKR_ABLATE builds only
#endif
    const int saved = c->dbg;
    if (kr_intersect(c, ids, n, is_in, 1) < 0) return -1.0;          // warm-up, allocations
    c->dbg = saved | mode;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    for (int r = 0; r < reps; r++) (void)kr_intersect(c, ids, n, is_in, 1);
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    c->dbg = saved;
    c->ncand = -1;
    return (double)ms / reps;
}

// measured HBM copy rate on this device: GB/s of read + write traffic of a streaming copy kernel (16 bytes per lane).
// The rate depends on how many workgroups stream at once and on how many loads a lane keeps in flight -- and the best
// combination differs from box to box (tools/membench.hip) --, so every form of k_copy16 (1, 2, 4 loads in flight; plain and
// non-temporal) is timed over several grid sizes and the best is the box's figure; kr_debug_copy_which names it.
extern "C++" {
template <int U, int NT>
static double copy_probe(hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* a, void* b, u64 n16, int grid, int reps) {
    hipLaunchKernelGGL((k_copy16<U, NT>), dim3((unsigned)grid), dim3(256), 0, st, (const u32x4*)a, (u32x4*)b, n16);   // warm-up
    (void)hipEventRecord(e0, st);
    for (int r = 0; r < reps; r++)
        hipLaunchKernelGGL((k_copy16<U, NT>), dim3((unsigned)grid), dim3(256), 0, st, (const u32x4*)a, (u32x4*)b, n16);
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms > 0 ? 2.0 * (double)(n16 * 16) * reps / (ms * 1e-3) / 1e9 : -1.0;
}
}
double kr_debug_copy_gbps(kr_ctx* c, size_t bytes, int reps) {
    if (!c || bytes < 4096 || reps < 1) return -1.0;
    if (hipSetDevice(c->device) != hipSuccess) return -1.0;
    DevBuf a, b;
    if (ensure(c, a, bytes) || ensure(c, b, bytes)) { release(c, a); release(c, b); return -1.0; }
    hipStream_t st = c->stream;
    (void)hipMemsetAsync(a.p, 1, bytes, st);
    (void)hipMemsetAsync(b.p, 2, bytes, st);
    const u64 n16 = bytes / 16;
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    double best = -1.0;
    c->copy_which[0] = 0;
    for (int per_cu : {2, 4, 8, 16, 32}) {
        const int grid = ncu * per_cu;
        const double r[6] = {copy_probe<1, 0>(st, e0, e1, a.p, b.p, n16, grid, reps), copy_probe<2, 0>(st, e0, e1, a.p, b.p, n16, grid, reps),
                             copy_probe<4, 0>(st, e0, e1, a.p, b.p, n16, grid, reps), copy_probe<1, 1>(st, e0, e1, a.p, b.p, n16, grid, reps),
                             copy_probe<2, 1>(st, e0, e1, a.p, b.p, n16, grid, reps), copy_probe<4, 1>(st, e0, e1, a.p, b.p, n16, grid, reps)};
        static const int un[6] = {1, 2, 4, 1, 2, 4};
        for (int i = 0; i < 6; i++)
            if (r[i] > best) {
                best = r[i];
                snprintf(c->copy_which, sizeof c->copy_which, "%d load(s) in flight per lane, %s, %d workgroups of 256 per CU, %.0f MB per array",
                         un[i], i >= 3 ? "non-temporal" : "plain", per_cu, (double)bytes / 1e6);
            }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    release(c, a);
    release(c, b);
    return best;
}
const char* kr_debug_copy_which(kr_ctx* c) { return c ? c->copy_which : ""; }

int kr_sync(kr_ctx* c) {
    if (!c) return KR_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    {
        int rcj = join_lanes(c);
        if (rcj) return rcj;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return KR_OK;
}

int kr_timer_begin(kr_ctx* c) {
    if (!c) return KR_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventRecord(c->t0, c->stream));
    return KR_OK;
}

double kr_timer_end_ms(kr_ctx* c) {
    if (!c) return -1.0;
    float ms = 0;
    if (hipEventRecord(c->t1, c->stream) != hipSuccess) return -1.0;
    if (hipEventSynchronize(c->t1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, c->t0, c->t1) != hipSuccess) return -1.0;
    return (double)ms;
}

int kr_stage_enable(kr_ctx* c, int on) {
    if (!c) return KR_ERR_PARAM;
    c->stage_on = on != 0;
    c->stage_mask = ~0u;
    return KR_OK;
}

int kr_stage_select(kr_ctx* c, unsigned mask) {
    if (!c) return KR_ERR_PARAM;
    c->stage_on = mask != 0;
    c->stage_mask = mask;
    return KR_OK;
}

int kr_stage_reset(kr_ctx* c) {
    if (!c) return KR_ERR_PARAM;
    (void)hipDeviceSynchronize();
    resolve_stages(c);
    for (int i = 0; i < KR_ST_COUNT; i++) { c->stage_ms[i] = 0; c->stage_n[i] = 0; }
    return KR_OK;
}

double kr_stage_ms(kr_ctx* c, int stage) {
    if (!c || stage < 0 || stage >= KR_ST_COUNT) return -1.0;
    (void)hipDeviceSynchronize();
    resolve_stages(c);
    return c->stage_ms[stage];
}

int64_t kr_stage_launches(kr_ctx* c, int stage) {
    if (!c || stage < 0 || stage >= KR_ST_COUNT) return -1;
    return c->stage_n[stage];
}

int64_t kr_debug_fetch(kr_ctx* c, int id, int what, void* out, size_t cap_bytes) {
    if (!c) return KR_ERR_PARAM;
    auto it = c->genomes.find(id);
    if (it == c->genomes.end()) return fail(c, KR_ERR_PARAM, "unknown genome %d", id);
    Genome& G = it->second;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcf = ensure_fine(c, G); if (rcf) return rcf; }
    if (what == 5 && G.sorted && !G.ordered) {      // (KR_OPT_LAZY_ORDER: selector 5 has always meant the sorted keys)
        int rco = ensure_ordered(c, {&G});
        if (!rco) rco = finalize(c, {&G});
        if (rco) return rco;
    }
    HIPCHK(c, hipDeviceSynchronize());
    Lane& ln = c->lanes[c->last_lane];   // the lane of the latest sort
    const u32 nb = 1u << c->g.b;
    const void* src = nullptr;
    size_t esz = 8, n = 0;
    if (G.sl.empty()) return fail(c, KR_ERR_STATE, "genome %d has no slices", id);
    Slice& S0 = G.sl[c->nslices - 1];      // the slice sorted last (its scratch is still in the lane)
    u32 total = 0;
    HIPCHK(c, hipMemcpy(&total, (u32*)S0.off.p + nb, 4, hipMemcpyDeviceToHost));
    switch (what) {
    case 0: src = ln.codes.p; esz = 8; n = G.nwords + 2; break;
    case 1: src = ln.bad.p; esz = 4; n = G.nwords + 2; break;
    case 2: src = ln.base1.p; esz = 4; n = 257; break;
    case 3: src = S0.off.p; esz = 4; n = nb + 1; break;
    case 4: src = c->g.b > 8 ? ln.tmpkeys.p : S0.keys.p; esz = 8; n = total; break;
    case 5: src = S0.keys.p; esz = 8; n = total; break;
    default: return fail(c, KR_ERR_PARAM, "kr_debug_fetch: unknown selector %d", what);
    }
    if (n * esz > cap_bytes) return fail(c, KR_ERR_CAPACITY, "debug buffer too small");
    if (n) HIPCHK(c, hipMemcpy(out, src, n * esz, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

int64_t kr_debug_inversions(kr_ctx* c, int id) {
    if (!c) return KR_ERR_PARAM;
    auto it = c->genomes.find(id);
    if (it != c->genomes.end()) { int rcf = ensure_fine(c, it->second); if (rcf) return rcf; }
    if (it == c->genomes.end() || !it->second.sorted) return fail(c, KR_ERR_STATE, "genome %d not sorted", id);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_ordered(c, {&it->second});
    if (rc) return rc;
    if ((rc = finalize(c, {&it->second}))) return rc;
    if ((rc = ensure(c, c->nrec, 16))) return rc;
    HIPCHK(c, hipMemset(c->nrec.p, 0, 16));
    for (Slice& S : it->second.sl)
        if (S.count > 1)
            hipLaunchKernelGGL(k_count_inversions, dim3(4096), dim3(256), 0, c->stream, (const u64*)S.keys.p,
                               (u64)S.count, (u64*)c->nrec.p);
    u64 bad = 0;
    HIPCHK(c, hipMemcpy(&bad, c->nrec.p, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipGetLastError());
    return (int64_t)bad;
}

// test aids: what is left of the context's HBM budget (-1: no budget set); set the budget so that `left` bytes remain
// what this context may still allocate: the device's free memory, or what is left of the context's HBM budget when
// that is less; out[1] = the device's total, out[2] = bytes this context holds, out[3] = its budget (0: none)
int kr_mem_info(kr_ctx* c, int64_t* out4) {
    if (!c || !out4) return KR_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    int64_t avail = (int64_t)fr;
    if (c->budget) avail = std::min<int64_t>(avail, (int64_t)c->budget - (int64_t)c->used);
    out4[0] = std::max<int64_t>(avail, 0);
    out4[1] = (int64_t)tot;
    out4[2] = (int64_t)c->used;
    out4[3] = (int64_t)c->budget;
    return KR_OK;
}
int64_t kr_debug_budget_left(kr_ctx* c) { return !c ? KR_ERR_PARAM : (c->budget ? (int64_t)c->budget - (int64_t)c->used : -1); }
int kr_debug_budget_set(kr_ctx* c, int64_t left) {
    if (!c || left < 0) return KR_ERR_PARAM;
    c->budget = c->used + (size_t)left;
    return KR_OK;
}

// the latest placement search of the pass-1 output buffers (h_core.inc: ensure_placed): out[0] candidates probed, [1] buffers
// handed to the sort lanes (the fastest), [2..5] probe milliseconds of the four fastest candidates, [6] the median, [7] the
// slowest; 800 MB buffers probe at ~0.19 ms in the fast class, ~0.22 and ~0.25 in the others (DESIGN.md, placement classes)
int kr_debug_place(kr_ctx* c, double* out8) {
    if (!c || !out8) return KR_ERR_PARAM;
    out8[0] = c->place_n;
    out8[1] = c->place_taken;
    for (int i = 0; i < 6; i++) out8[2 + i] = c->place_ms[i];
    return KR_OK;
}

// the pool of placed pass-1 targets for coarse genomes (h_core.inc: coarse_pool_*): out[0] buffers in all, [1] free, [2] held by
// genomes, [3] coarse sorts that wrote into a pooled buffer, [4] placement searches the pool has run, [5] / [6] the fastest and
// the slowest probe milliseconds among the buffers held (0 when none is), [7] KR_OPT_COARSE_POOL
int kr_debug_coarse_pool(kr_ctx* c, double* out8) {
    if (!c || !out8) return KR_ERR_PARAM;
    int held = 0;
    double lo = 0, hi = 0;
    for (auto& kv : c->genomes) {
        const Genome& G = kv.second;
        if (!G.ckeys.p) continue;
        lo = held ? std::min(lo, G.ckeys_ms) : G.ckeys_ms;
        hi = held ? std::max(hi, G.ckeys_ms) : G.ckeys_ms;
        held++;
    }
    out8[0] = c->cpool_total;
    out8[1] = (double)c->cpool_free.size();
    out8[2] = held;
    out8[3] = (double)c->cpool_partitions;
    out8[4] = (double)c->cpool_searches;
    out8[5] = lo;
    out8[6] = hi;
    out8[7] = c->coarse_pool;
    return KR_OK;
}

// KR_OPT_COARSE_ONE_STRAND (h_core.inc: one_strand_form; k_coarse.inc): out[0] partitions that wrote one strand, [1] intersections
// that probed one-strand genomes, [2] / [3] the forward / reverse rounds of all of them, [4] / [5] of the latest, [6] the option,
// [7] the passes of the latest call (KR_OPT_COARSE_ONE_PASS, co_pass.inc)
int kr_debug_coarse_strand(kr_ctx* c, int64_t* o) {
    if (!c || !o) return KR_ERR_PARAM;
    o[0] = c->one_partitions;
    o[1] = c->one_calls;
    o[2] = c->one_rounds[0];
    o[3] = c->one_rounds[1];
    o[4] = c->one_last[0];
    o[5] = c->one_last[1];
    o[6] = c->coarse_one;
    o[7] = c->one_last_passes;
    return KR_OK;
}

int kr_debug_isect(kr_ctx* c, int64_t* o) {
    if (!c || !o) return KR_ERR_PARAM;
    o[0] = c->isect_ovf_items;
    o[1] = c->isect_refall;
    o[2] = c->i3_last_T;
    o[3] = c->i3_last_mlog;
    o[4] = c->i3_last_tags;
    o[5] = lanes_used(c);
    o[6] = c->j2_launches;
    o[7] = c->j2_full;
    return KR_OK;
}

// the latest tile scan's geometry (h_scan.inc): o[0] tiles, [1] workgroups and [2] the KR_SCAN_GRID cap (0: none) of the latest
// scan_grid(), [3] the tiles or blocks of the latest scan_two_pass, [4..7] 0
int kr_debug_scan(kr_ctx* c, int64_t* o) {
    if (!c || !o) return KR_ERR_PARAM;
    o[0] = c->scan_dbg[0];
    o[1] = c->scan_dbg[1];
    o[2] = c->scan_cap;
    o[3] = c->scan_dbg[2];
    o[4] = o[5] = o[6] = o[7] = 0;
    return KR_OK;
}

// which result-changing experiment switches this library was compiled with (k_keys.inc): 0 for a product build
int kr_build_experiments(void) {
    int bits = 0;
#ifdef KR_EXPERIMENTS
    bits |= 1;
#endif
#ifdef KR_ABLATE
    bits |= 2;
#endif
#if defined(I3_ABL) && I3_ABL
    bits |= 4;
#endif
#if defined(P2_ABL) && P2_ABL
    bits |= 8;
#endif
#ifdef LS2_NORANK
    bits |= 16;
#endif
#ifdef KR_EXP_NOLOOKUP
    bits |= 32;
#endif
#ifdef KR_EXP_MZONLY
    bits |= 64;
#endif
    return bits;
}

int kr_debug_lazy(kr_ctx* c, int64_t* o) {
    if (!c || !o) return KR_ERR_PARAM;
    o[0] = c->lazy_skipped;
    o[1] = c->lazy_ordered;
    o[2] = c->lazy_touch;
    o[3] = c->lazy_order;
    o[4] = c->isect_ua;
    o[5] = c->fuse_anchor;
    o[6] = c->coarse_done;
    o[7] = c->coarse_promoted;
    return KR_OK;
}

int kr_debug_info(kr_ctx* c, int64_t* o) {
    if (!c || !o) return KR_ERR_PARAM;
    o[0] = c->g.b;
    o[1] = 1ll << c->g.b;
    o[2] = LS_T;
    o[3] = LS_CAP;
    o[4] = NWG;
    o[5] = c->overflow_segments;
    o[6] = c->fallback_launches;
    o[7] = (int64_t)c->nslices;
    return KR_OK;
}

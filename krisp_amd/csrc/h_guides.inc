// h_guides.inc -- part of krisp_hip.hip (one translation unit): host side of the guide pass (k_guides.inc): the check of the
// options, the run over the regions' rows in batches, the records.  The pass needs no genome and no parameters of another
// pass: any context takes it.  The options travel with every launch; on the device live, per batch, the rows (K bytes
// each), the regions' row offsets (8 bytes a region and 8 more) and bounds (8 bytes a region) and the records (32 bytes a
// region); the records of all batches are kept on the host.
#define GUI_BATCH_BYTES ((size_t)32 << 20)      // row bytes of one batch (a region's rows stay together: one region may exceed it)
#define GUI_BATCH_REGIONS ((u64)1 << 18)        // ... and its regions at most (a workgroup each)

int kr_guides_table(kr_ctx* c, const kr_guide_params* p) {
    if (!c || !p) return fail(c, KR_ERR_PARAM, "kr_guides_table: null argument");
    auto& u = c->guides;
    u.on = false;
    u.nrec = u.top_nrec = -1;
    if (p->guide_size < GUI_MIN_SIZE || p->guide_size > GUI_MAX_SIZE)
        return fail(c, KR_ERR_PARAM, "kr_guides_table: %d <= guide_size <= %d (got %d)", GUI_MIN_SIZE, GUI_MAX_SIZE, p->guide_size);
    if (p->pam5_len < 0 || p->pam5_len > GUI_MAX_PAM || p->pam3_len < 0 || p->pam3_len > GUI_MAX_PAM)
        return fail(c, KR_ERR_PARAM, "kr_guides_table: a motif has 0 .. %d letters (got %d and %d)", GUI_MAX_PAM, p->pam5_len, p->pam3_len);
    for (int j = 0; j < p->pam5_len; j++)
        if (p->pam5[j] < 1 || p->pam5[j] > 15) return fail(c, KR_ERR_PARAM, "kr_guides_table: pam5[%d] = %d is no IUPAC mask (1 .. 15)", j, p->pam5[j]);
    for (int j = 0; j < p->pam3_len; j++)
        if (p->pam3[j] < 1 || p->pam3[j] > 15) return fail(c, KR_ERR_PARAM, "kr_guides_table: pam3[%d] = %d is no IUPAC mask (1 .. 15)", j, p->pam3[j]);
    u.params = *p;
    u.on = true;
    return KR_OK;
}

// what kr_guides_run (`who`, top = 0: k_guides, a record a region into u.out) and kr_guides_run_top (1 <= top: k_guides_top,
// `top` records a region into u.top_out) share: the checks, the batches, the records kept on the host.  Each leaves the
// other's records alone
static int64_t guides_run(kr_ctx* c, const char* who, const uint8_t* rows, const uint64_t* row_off, const uint32_t* bounds,
                          uint64_t nregions, int K, int L, int D, int top) {
    if (!c || !c->guides.on) return fail(c, KR_ERR_STATE, "kr_guides_table first");
    auto& u = c->guides;
    const u64 per = top ? (u64)top : 1;             // records of a region
    std::vector<kr_guide_record>& out = top ? u.top_out : u.out;
    int64_t& nrec = top ? u.top_nrec : u.nrec;
    nrec = -1;
    const kr_guide_params& p = u.params;
    if (K < p.guide_size || K > GUI_MAX_TEMPLATE)
        return fail(c, KR_ERR_PARAM, "%s: rows of guide_size = %d .. %d letters (got %d)", who, p.guide_size, GUI_MAX_TEMPLATE, K);
    if (L < 0 || D < 0 || L + D > K) return fail(c, KR_ERR_PARAM, "%s: L + D within the %d letters of a row (got %d + %d)", who, K, L, D);
    if (nregions && (!rows || !row_off || !bounds)) return fail(c, KR_ERR_PARAM, "%s: null argument", who);
    if (nregions && row_off[0] != 0) return fail(c, KR_ERR_PARAM, "%s: row_off[0] = %llu (0 is meant)", who, (unsigned long long)row_off[0]);
    for (u64 r = 0; r < nregions; r++) {
        if (row_off[r + 1] <= row_off[r])
            return fail(c, KR_ERR_PARAM, "%s: region %llu has no template (row_off %llu, then %llu)", who, (unsigned long long)r,
                        (unsigned long long)row_off[r], (unsigned long long)row_off[r + 1]);
        if (row_off[r + 1] - row_off[r] > GUI_MAX_ROWS)
            return fail(c, KR_ERR_PARAM, "%s: region %llu has %llu rows (at most 2^26)", who, (unsigned long long)r,
                        (unsigned long long)(row_off[r + 1] - row_off[r]));
        if (bounds[2 * r] > bounds[2 * r + 1] || bounds[2 * r + 1] > (u32)K)
            return fail(c, KR_ERR_PARAM, "%s: region %llu: bounds [%u, %u) do not lie in order within the %d columns", who,
                        (unsigned long long)r, bounds[2 * r], bounds[2 * r + 1], K);
    }
    HIPCHK(c, hipSetDevice(c->device));
    GuideGeom g;
    guide_geom(K, L, D, &g);
    int lds_max = 65536;
    (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device);
    if ((size_t)g.lds_bytes > (size_t)lds_max)
        return fail(c, KR_ERR_CAPACITY, "%s: the tables of a region of %d columns take %u bytes of LDS (a workgroup has %d)", who, K,
                    g.lds_bytes, lds_max);
    HIPCHK(c, hipFuncSetAttribute(top ? (const void*)k_guides_top : (const void*)k_guides, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)g.lds_bytes));
    GuideArgs a{};
    a.g = (u32)p.guide_size; a.a = (u32)p.pam5_len; a.b = (u32)p.pam3_len;
    for (int j = 0; j < p.pam5_len; j++) a.pam5 |= (u32)p.pam5[j] << (4 * j);
    for (int j = 0; j < p.pam3_len; j++) a.pam3 |= (u32)p.pam3[j] << (4 * j);
    a.gc_lo = p.gc_lo; a.gc_hi = p.gc_hi; a.min_mm = p.min_mismatches;
    std::vector<u64> off;
    try {
        out.assign(nregions * per, kr_guide_record{});
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "%s: no host memory for %llu records", who, (unsigned long long)(nregions * per));
    }
    const u64 batch_rows = std::max<u64>(1, GUI_BATCH_BYTES / (size_t)K);
    int64_t found = 0;
    for (u64 at = 0; at < nregions;) {
        // the regions of this batch: at least one, then as many as keep the rows and the regions within a batch
        u64 to = at + 1;
        while (to < nregions && to - at < GUI_BATCH_REGIONS && row_off[to + 1] - row_off[at] <= batch_rows) to++;
        const u64 nb = to - at, r0 = row_off[at], nrows = row_off[to] - r0;
        off.resize(nb + 1);
        for (u64 i = 0; i <= nb; i++) off[i] = row_off[at + i] - r0;
        int rc;
        if ((rc = ensure(c, u.rows, nrows * (size_t)K)) || (rc = ensure(c, u.off, (nb + 1) * sizeof(u64))) ||
            (rc = ensure(c, u.bnd, nb * 2 * sizeof(u32))) || (rc = ensure(c, u.rec, nb * per * sizeof(kr_guide_record))))
            return rc;
        HIPCHK(c, hipMemcpy(u.rows.p, rows + r0 * (size_t)K, nrows * (size_t)K, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(u.off.p, off.data(), (nb + 1) * sizeof(u64), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(u.bnd.p, bounds + 2 * at, nb * 2 * sizeof(u32), hipMemcpyHostToDevice));
        if (top)
            hipLaunchKernelGGL(k_guides_top, dim3((u32)nb), dim3(GUI_T), g.lds_bytes, c->stream, (const uint8_t*)u.rows.p,
                               (const u64*)u.off.p, (const u32*)u.bnd.p, (u32)nb, g, a, (u32)top, (kr_guide_record*)u.rec.p);
        else
            hipLaunchKernelGGL(k_guides, dim3((u32)nb), dim3(GUI_T), g.lds_bytes, c->stream, (const uint8_t*)u.rows.p, (const u64*)u.off.p,
                               (const u32*)u.bnd.p, (u32)nb, g, a, (kr_guide_record*)u.rec.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(out.data() + at * per, u.rec.p, nb * per * sizeof(kr_guide_record), hipMemcpyDeviceToHost));
        for (u64 i = 0; i < nb * per; i++) found += out[at * per + i].found;
        at = to;
    }
    nrec = (int64_t)(nregions * per);
    return found;
}

int64_t kr_guides_run(kr_ctx* c, const uint8_t* rows, const uint64_t* row_off, const uint32_t* bounds, uint64_t nregions, int K,
                      int L, int D) {
    return guides_run(c, "kr_guides_run", rows, row_off, bounds, nregions, K, L, D, 0);
}

int64_t kr_guides_run_top(kr_ctx* c, const uint8_t* rows, const uint64_t* row_off, const uint32_t* bounds, uint64_t nregions, int K,
                          int L, int D, int top) {
    if (c && c->guides.on && (top < 1 || top > GUI_MAX_TOP)) {
        c->guides.top_nrec = -1;
        return fail(c, KR_ERR_PARAM, "kr_guides_run_top: 1 <= top <= %d (got %d)", GUI_MAX_TOP, top);
    }
    return guides_run(c, "kr_guides_run_top", rows, row_off, bounds, nregions, K, L, D, top);
}

int64_t kr_guides_fetch(kr_ctx* c, kr_guide_record* out, size_t cap) {
    if (!c || c->guides.nrec < 0) return fail(c, KR_ERR_STATE, "kr_guides_run first");
    const auto& u = c->guides;
    if ((size_t)u.nrec > cap) return fail(c, KR_ERR_CAPACITY, "record buffer too small: %lld > %zu", (long long)u.nrec, cap);
    if (u.nrec) {
        if (!out) return fail(c, KR_ERR_PARAM, "kr_guides_fetch: null argument");
        memcpy(out, u.out.data(), (size_t)u.nrec * sizeof(kr_guide_record));
    }
    return u.nrec;
}

int64_t kr_guides_fetch_top(kr_ctx* c, kr_guide_record* out, size_t cap) {
    if (!c || c->guides.top_nrec < 0) return fail(c, KR_ERR_STATE, "kr_guides_run_top first");
    const auto& u = c->guides;
    if ((size_t)u.top_nrec > cap) return fail(c, KR_ERR_CAPACITY, "record buffer too small: %lld > %zu", (long long)u.top_nrec, cap);
    if (u.top_nrec) {
        if (!out) return fail(c, KR_ERR_PARAM, "kr_guides_fetch_top: null argument");
        memcpy(out, u.top_out.data(), (size_t)u.top_nrec * sizeof(kr_guide_record));
    }
    return u.top_nrec;
}

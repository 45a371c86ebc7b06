// h_design.inc -- part of krisp_hip.hip (one translation unit): host side of the primer design pass (k_design.inc): the
// check and upload of the model and options, the run over the regions' templates in batches, the records.  The pass needs
// no genome and no parameters of another pass: any context takes it.  On the device live the 224 bytes of the parameters,
// behind them the 256 bytes of the hairpin check's loop table (kr_design_hairpins), and, per batch, the templates (L + D + R
// bytes a region), the records (64 bytes a region) and, with the hairpin check, the hairpin figures (8 bytes a region); the
// records and figures of all batches are kept on the host.  kr_design_run_top (--primer-candidates, DESIGN §25) has `top`
// records and figures a region, in a list and with a state of its own.
#define DES_BATCH_BYTES ((size_t)64 << 20)      // template bytes of one batch
#define DES_BATCH_REGIONS ((u64)1 << 20)        // ... and its records at most (a workgroup a region)

int kr_design_table(kr_ctx* c, const kr_design_params* p) {
    if (!c || !p) return fail(c, KR_ERR_PARAM, "kr_design_table: null argument");
    auto& d = c->design;
    d.on = false;
    d.hp = d.hp_ran = d.top_hp_ran = false;
    d.nrec = d.top_nrec = -1;
    if (p->size_lo < 10 || p->size_hi > 60 || p->size_hi < p->size_lo)
        return fail(c, KR_ERR_PARAM, "kr_design_table: 10 <= size_lo <= size_hi <= 60 (got %d .. %d)", p->size_lo, p->size_hi);
    if (p->tm_hi < p->tm_lo || p->gc_hi < p->gc_lo || p->amp_hi < p->amp_lo)
        return fail(c, KR_ERR_PARAM, "kr_design_table: a range whose upper bound lies below its lower (tm %d .. %d, gc %d .. %d, product %d .. %d)",
                    p->tm_lo, p->tm_hi, p->gc_lo, p->gc_hi, p->amp_lo, p->amp_hi);
    if (p->gc_clamp < 0 || p->gc_clamp > p->size_lo || p->max_end_gc < 0)
        return fail(c, KR_ERR_PARAM, "kr_design_table: 0 <= gc_clamp <= size_lo and max_end_gc >= 0 (got %d, %d)", p->gc_clamp, p->max_end_gc);
    // the kernel divides -dH 10^6 by -dS as unsigned numbers and keeps a Tm in an int: every duplex of two pairs or more has
    // dH < 0 and dS <= -4000, and no entry is beyond 16 bits and a half
    int max_term_dh = 0, max_term_ds = 0, max_nn_dh = INT32_MIN, max_nn_ds = INT32_MIN;
    bool small = true;
    for (int i = 0; i < 4; i++) {
        max_term_dh = std::max(max_term_dh, p->term_dh[i]);
        max_term_ds = std::max(max_term_ds, p->term_ds[i]);
        small = small && std::abs((long long)p->term_dh[i]) < 100000 && std::abs((long long)p->term_ds[i]) < 100000;
    }
    for (int i = 0; i < 16; i++) {
        max_nn_dh = std::max(max_nn_dh, p->nn_dh[i]);
        max_nn_ds = std::max(max_nn_ds, p->nn_ds[i]);
        small = small && std::abs((long long)p->nn_dh[i]) < 100000 && std::abs((long long)p->nn_ds[i]) < 100000;
    }
    const long long worst_ds = (long long)std::max(p->conc_ds, p->conc_self_ds + p->sym_ds) + 2ll * max_term_ds;
    if (!small || (long long)max_nn_dh + 2ll * max_term_dh >= 0 || max_nn_ds > 0 || p->salt_ds > 0 || worst_ds > -4000)
        return fail(c, KR_ERR_PARAM, "kr_design_table: the model does not keep every duplex's dH below 0 and dS at -4000 or below");
    const long long worst_pen = 2 * (std::max(std::abs((long long)p->tm_lo - p->tm_opt), std::abs((long long)p->tm_hi - p->tm_opt)) +
                                     500ll * (p->size_hi - p->size_lo));
    if (worst_pen >= (1ll << 30) - 1)
        return fail(c, KR_ERR_PARAM, "kr_design_table: a pair's penalty may reach %lld (the limit is 2^30 - 2)", worst_pen);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, d.par, sizeof *p + sizeof(kr_hairpin_params)))) return rc;
    HIPCHK(c, hipMemcpy(d.par.p, p, sizeof *p, hipMemcpyHostToDevice));
    d.params = *p;
    d.on = true;
    return KR_OK;
}

int kr_design_hairpins(kr_ctx* c, const kr_hairpin_params* h) {
    if (!c || !c->design.on) return fail(c, KR_ERR_STATE, "kr_design_table first");
    auto& d = c->design;
    d.hp = false;
    if (!h) return KR_OK;
    // a stem has a step at least and two terminal bases: as in kr_design_table, its dS stays at -4000 or below (its dH is
    // a duplex's, the loop's is 0)
    const kr_design_params& p = d.params;
    const long long stem_ds = (long long)*std::max_element(p.nn_ds, p.nn_ds + 16) + p.salt_ds +
                              2ll * *std::max_element(p.term_ds, p.term_ds + 4);
    for (int l = DES_MIN_LOOP; l <= DES_MAX_LOOP; l++)
        if (std::abs((long long)h->loop_ds[l]) >= 100000 || stem_ds + h->loop_ds[l] > -4000)
            return fail(c, KR_ERR_PARAM, "kr_design_hairpins: loop_ds[%d] = %d does not keep every stem's dS at -4000 or below "
                        "(the least negative step with its salt and two terminals come to %lld), or lies beyond +-99999", l,
                        h->loop_ds[l], stem_ds);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy((char*)d.par.p + sizeof p, h, sizeof *h, hipMemcpyHostToDevice));
    d.hp = true;
    return KR_OK;
}

// what kr_design_run (`who`, top = 0: k_design, a record a region into d.out) and kr_design_run_top (1 <= top: k_design_top,
// `top` records a region into d.top_out) share: the checks, the batches, the records and figures kept on the host.  Each
// leaves the other's list and state alone
static int64_t design_run(kr_ctx* c, const char* who, const uint8_t* templates, uint64_t nregions, int L, int D, int R, int top) {
    if (!c || !c->design.on) return fail(c, KR_ERR_STATE, "kr_design_table first");
    auto& d = c->design;
    const u64 per = top ? (u64)top : 1;             // records of a region
    std::vector<kr_design_record>& out = top ? d.top_out : d.out;
    std::vector<int32_t>& hp_out = top ? d.top_hp_out : d.hp_out;
    int64_t& nrec = top ? d.top_nrec : d.nrec;
    bool& hp_ran = top ? d.top_hp_ran : d.hp_ran;
    nrec = -1;
    hp_ran = false;
    const bool hp = d.hp;
    const void* const kernel = top ? (hp ? (const void*)k_design_top<true> : (const void*)k_design_top<false>)
                                   : (hp ? (const void*)k_design<true> : (const void*)k_design<false>);
    if (L < 0 || D < 0 || R < 0 || L > DES_MAX_FLANK || R > DES_MAX_FLANK || L + D + R > DES_MAX_TEMPLATE || L + D + R < 1)
        return fail(c, KR_ERR_PARAM, "%s: flanks of at most %d and a template of 1 .. %d bytes (got %d/%d/%d)", who, DES_MAX_FLANK,
                    DES_MAX_TEMPLATE, L, D, R);
    if (!templates && nregions) return fail(c, KR_ERR_PARAM, "%s: null templates", who);
    HIPCHK(c, hipSetDevice(c->device));
    DesignGeom g;
    design_geom(L, D, R, d.params.size_lo, d.params.size_hi, hp, &g);
    int lds_max = 65536;
    (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device);
    if ((size_t)g.lds_bytes > (size_t)lds_max)
        return fail(c, KR_ERR_CAPACITY, "%s: the candidate tables of a %d/%d/%d region with primers of %d .. %d bases take %u "
                    "bytes of LDS (a workgroup has %d): a narrower --primer_size", who, L, D, R, d.params.size_lo, d.params.size_hi,
                    g.lds_bytes, lds_max);
    HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes));
    try {
        out.assign(nregions * per, kr_design_record{});
        hp_out.assign(hp ? 2 * nregions * per : 0, 0);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "%s: no host memory for %llu records", who, (unsigned long long)(nregions * per));
    }
    // (a batch's records stay within DES_BATCH_REGIONS, whatever a region has of them)
    const u64 batch = std::max<u64>(1, std::min<u64>(DES_BATCH_REGIONS / per, DES_BATCH_BYTES / g.W));
    int64_t found = 0;
    for (u64 at = 0; at < nregions; at += batch) {
        const u64 nb = std::min<u64>(batch, nregions - at);
        int rc;
        if ((rc = ensure(c, d.tmpl, nb * g.W)) || (rc = ensure(c, d.rec, nb * per * sizeof(kr_design_record)))) return rc;
        if (hp && (rc = ensure(c, d.hprec, nb * per * sizeof(int2)))) return rc;
        HIPCHK(c, hipMemcpy(d.tmpl.p, templates + at * g.W, nb * g.W, hipMemcpyHostToDevice));
        const uint8_t* const tm = (const uint8_t*)d.tmpl.p;
        const kr_design_params* const par = (const kr_design_params*)d.par.p;
        kr_design_record* const rec = (kr_design_record*)d.rec.p;
        int2* const hprec = hp ? (int2*)d.hprec.p : nullptr;
        const dim3 grid((u32)nb), block(DES_T);
        if (top && hp) hipLaunchKernelGGL(k_design_top<true>, grid, block, g.lds_bytes, c->stream, tm, (u32)nb, g, par, (u32)top, rec, hprec);
        else if (top) hipLaunchKernelGGL(k_design_top<false>, grid, block, g.lds_bytes, c->stream, tm, (u32)nb, g, par, (u32)top, rec, hprec);
        else if (hp) hipLaunchKernelGGL(k_design<true>, grid, block, g.lds_bytes, c->stream, tm, (u32)nb, g, par, rec, hprec);
        else hipLaunchKernelGGL(k_design<false>, grid, block, g.lds_bytes, c->stream, tm, (u32)nb, g, par, rec, hprec);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(out.data() + at * per, d.rec.p, nb * per * sizeof(kr_design_record), hipMemcpyDeviceToHost));
        if (hp) HIPCHK(c, hipMemcpy(hp_out.data() + 2 * at * per, d.hprec.p, nb * per * sizeof(int2), hipMemcpyDeviceToHost));
        for (u64 i = 0; i < nb; i++) found += out[(at + i) * per].found;
    }
    nrec = (int64_t)(nregions * per);
    hp_ran = hp;
    return found;
}

int64_t kr_design_run(kr_ctx* c, const uint8_t* templates, uint64_t nregions, int L, int D, int R) {
    return design_run(c, "kr_design_run", templates, nregions, L, D, R, 0);
}

int64_t kr_design_run_top(kr_ctx* c, const uint8_t* templates, uint64_t nregions, int L, int D, int R, int top) {
    if (c && c->design.on && (top < 1 || top > DES_MAX_TOP)) {
        c->design.top_nrec = -1;
        c->design.top_hp_ran = false;
        return fail(c, KR_ERR_PARAM, "kr_design_run_top: 1 <= top <= %d (got %d)", DES_MAX_TOP, top);
    }
    return design_run(c, "kr_design_run_top", templates, nregions, L, D, R, top);
}

// the records of a run (nrec < 0: none stands, `first` says which to call)
static int64_t design_fetch(kr_ctx* c, const char* first, int64_t nrec, const std::vector<kr_design_record>& list, kr_design_record* out,
                            size_t cap) {
    if (nrec < 0) return fail(c, KR_ERR_STATE, "%s", first);
    if ((size_t)nrec > cap) return fail(c, KR_ERR_CAPACITY, "record buffer too small: %lld > %zu", (long long)nrec, cap);
    if (nrec) memcpy(out, list.data(), (size_t)nrec * sizeof(kr_design_record));
    return nrec;
}

// ... and its hairpin figures, two int32 a record
static int64_t design_fetch_hairpins(kr_ctx* c, const char* who, const char* first, int64_t nrec, bool hp_ran, const std::vector<int32_t>& list,
                                     int32_t* out, size_t cap) {
    if (nrec < 0) return fail(c, KR_ERR_STATE, "%s", first);
    if (!hp_ran) return fail(c, KR_ERR_STATE, "%s: the latest run had the hairpin check off (kr_design_hairpins)", who);
    const size_t n = 2 * (size_t)nrec;
    if (n > cap) return fail(c, KR_ERR_CAPACITY, "hairpin buffer too small: %zu > %zu", n, cap);
    if (n) memcpy(out, list.data(), n * sizeof(int32_t));
    return (int64_t)n;
}

int64_t kr_design_fetch(kr_ctx* c, kr_design_record* out, size_t cap) {
    if (!c) return fail(c, KR_ERR_STATE, "kr_design_run first");
    return design_fetch(c, "kr_design_run first", c->design.nrec, c->design.out, out, cap);
}

int64_t kr_design_fetch_hairpins(kr_ctx* c, int32_t* out, size_t cap) {
    if (!c) return fail(c, KR_ERR_STATE, "kr_design_run first");
    const auto& d = c->design;
    return design_fetch_hairpins(c, "kr_design_fetch_hairpins", "kr_design_run first", d.nrec, d.hp_ran, d.hp_out, out, cap);
}

int64_t kr_design_fetch_top(kr_ctx* c, kr_design_record* out, size_t cap) {
    if (!c) return fail(c, KR_ERR_STATE, "kr_design_run_top first");
    return design_fetch(c, "kr_design_run_top first", c->design.top_nrec, c->design.top_out, out, cap);
}

int64_t kr_design_fetch_top_hairpins(kr_ctx* c, int32_t* out, size_t cap) {
    if (!c) return fail(c, KR_ERR_STATE, "kr_design_run_top first");
    const auto& d = c->design;
    return design_fetch_hairpins(c, "kr_design_fetch_top_hairpins", "kr_design_run_top first", d.top_nrec, d.top_hp_ran, d.top_hp_out, out, cap);
}

// h_panel.inc -- part of krisp_hip.hip (one translation unit): host side of the panel pass (k_panel.inc, DESIGN §23): the
// checks, the upload of all candidates (the selection needs every one resident: no batches), N launches on the context's
// stream with one synchronise behind them, the members and the fates.  The model and max_sec are those kr_design_table left
// on the device.  On the device: the templates (W bytes a candidate), the pairs (8 bytes), fate and by (2 bytes), the
// running figures (8 bytes), and pick[0 .. size].
#define PAN_MAX_SIZE 64

// what kr_panel_run_clean adds to the launches (h_panel_clean.inc): before round 0, and behind every round's k_panel_round
static int pclean_before(kr_ctx* c, const uint32_t* texts, u64 ncand);
static void pclean_round(kr_ctx* c, u32 r, u64 ncand);

// kr_panel_run (texts == nullptr) and kr_panel_run_clean (texts: two table rows a candidate, checked by the caller)
static int64_t panel_run(kr_ctx* c, const char* who, const uint8_t* templates, const uint16_t* pairs, uint64_t ncand, int W, int size,
                         const uint32_t* texts) {
    auto& p = c->panel;
    if (W < 1 || W > (int)PANEL_MAX_TEMPLATE) return fail(c, KR_ERR_PARAM, "%s: a template of 1 .. %u bytes (got %d)", who, PANEL_MAX_TEMPLATE, W);
    if (size < 1 || size > PAN_MAX_SIZE) return fail(c, KR_ERR_PARAM, "%s: a panel of 1 .. %d members (got %d)", who, PAN_MAX_SIZE, size);
    if (ncand && (!templates || !pairs)) return fail(c, KR_ERR_PARAM, "%s: null argument", who);
    if (ncand >= (uint64_t)PAN_NONE) return fail(c, KR_ERR_CAPACITY, "%s: fewer than 2^32 - 1 candidates (got %llu)", who, (unsigned long long)ncand);
    for (u64 i = 0; i < ncand; i++) {
        const uint16_t* q = pairs + 4 * i;
        for (int s = 0; s < 2; s++)
            if (q[2 * s + 1] < 10 || q[2 * s + 1] > 60 || (int)q[2 * s] + (int)q[2 * s + 1] > W)
                return fail(c, KR_ERR_PARAM, "%s: candidate %llu: a primer of 10 .. 60 bases inside the template of %d (got start %u, "
                            "length %u)", who, (unsigned long long)i, W, (unsigned)q[2 * s], (unsigned)q[2 * s + 1]);
    }
    try {
        p.members.assign((size_t)size, kr_panel_member{});
        p.fates.assign(2 * (size_t)ncand, 0);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "%s: no host memory for %llu fates", who, (unsigned long long)ncand);
    }
    p.members.clear();
    p.ncand = ncand;
    if (!ncand) return p.nmem = 0;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t npick = (size_t)size + 1;
    if ((rc = ensure(c, p.tmpl, (size_t)ncand * (size_t)W)) || (rc = ensure(c, p.pairs, (size_t)ncand * 8)) ||
        (rc = ensure(c, p.state, (size_t)ncand * 2)) || (rc = ensure(c, p.cross, (size_t)ncand * 8)) || (rc = ensure(c, p.pick, npick * 4)))
        return rc;
    std::vector<u32> pick(npick, PAN_NONE);
    pick[0] = 0;
    HIPCHK(c, hipMemcpyAsync(p.tmpl.p, templates, (size_t)ncand * (size_t)W, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.pairs.p, pairs, (size_t)ncand * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.pick.p, pick.data(), npick * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(p.state.p, 0, (size_t)ncand * 2, c->stream));
    HIPCHK(c, hipMemsetAsync(p.cross.p, 0, (size_t)ncand * 8, c->stream));
    // (persistent workgroups: four a CU, a wave per candidate at a time)
    const u32 grid = (u32)std::max<u64>(1, std::min<u64>((u64)c->ncu * 4, (ncand + PAN_WAVES - 1) / PAN_WAVES));
    if (texts && (rc = pclean_before(c, texts, ncand))) return rc;
    for (int r = 0; r < size; r++) {
        hipLaunchKernelGGL(k_panel_round, dim3(grid), dim3(PAN_T), 0, c->stream, (const uint8_t*)p.tmpl.p, (const ushort4*)p.pairs.p,
                           (u32)ncand, (u32)W, (u32)r, (const kr_design_params*)c->design.par.p, (u32*)p.pick.p, (uint8_t*)p.state.p,
                           (int2*)p.cross.p);
        if (texts) pclean_round(c, (u32)r, ncand);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(pick.data(), p.pick.p, npick * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.fates.data(), p.state.p, (size_t)ncand * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the members: their running figures, and what each dropped by either cause
    for (int r = 0; r < size && pick[r] < ncand; r++) {
        kr_panel_member mb{};
        mb.position = pick[r];
        int cr[2];
        HIPCHK(c, hipMemcpy(cr, (const char*)p.cross.p + (size_t)pick[r] * 8, 8, hipMemcpyDeviceToHost));
        mb.cross_any = cr[0];
        mb.cross_end = cr[1];
        p.members.push_back(mb);
    }
    for (u64 i = 0; i < ncand; i++) {
        const unsigned fate = p.fates[2 * i], by = p.fates[2 * i + 1];
        if ((fate == 2 || fate == 3) && by >= 1 && by <= p.members.size()) p.members[by - 1].dropped[fate - 2]++;
    }
    return p.nmem = (int64_t)p.members.size();
}

int64_t kr_panel_run(kr_ctx* c, const uint8_t* templates, const uint16_t* pairs, uint64_t ncand, int W, int size) {
    if (!c || !c->design.on) return fail(c, KR_ERR_STATE, "kr_design_table first");
    c->panel.nmem = -1;
    return panel_run(c, "kr_panel_run", templates, pairs, ncand, W, size, nullptr);
}

int64_t kr_panel_fetch(kr_ctx* c, kr_panel_member* out, size_t cap) {
    if (!c || c->panel.nmem < 0) return fail(c, KR_ERR_STATE, "kr_panel_run first");
    const auto& p = c->panel;
    if ((size_t)p.nmem > cap) return fail(c, KR_ERR_CAPACITY, "member buffer too small: %lld > %zu", (long long)p.nmem, cap);
    if (p.nmem) memcpy(out, p.members.data(), (size_t)p.nmem * sizeof(kr_panel_member));
    return p.nmem;
}

int64_t kr_panel_fates(kr_ctx* c, uint8_t* out, size_t cap) {
    if (!c || c->panel.nmem < 0) return fail(c, KR_ERR_STATE, "kr_panel_run first");
    const auto& p = c->panel;
    if (p.fates.size() > cap) return fail(c, KR_ERR_CAPACITY, "fate buffer too small: %zu > %zu", p.fates.size(), cap);
    if (!p.fates.empty()) memcpy(out, p.fates.data(), p.fates.size());
    return (int64_t)p.fates.size();
}

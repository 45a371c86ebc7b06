// k_multiplex.inc -- part of krisp_hip.hip (one translation unit): the multiplex pass (--out_panel_products, DESIGN §24):
// in-silico PCR with all the oligos of a panel in one tube.  The host driver is h_multiplex.inc.  The table is the primer
// pass's with nleft = T texts and nright = 0: entry 2 t = text t as written, an OPENING site, its 3' end in its last
// columns; entry 2 t + 1 = its reverse complement, a CLOSING site, its 3' end in its first columns -- what prim_end_last
// (2 T, e) says.  The sites are k_prim_scan's (k_primers.inc), their records k_prod_rec's (k_products.inc); here are the
// join, in which any text opens and any text closes, and its tally.
//
// k_mux_join: a thread per site, a workgroup per LOC_T sites.  An opening site walks the following sites of its record
// up to pos + max_product - smin and takes every closing site that starts behind its own last base and ends within
// max_product: there is no pair list, every combination is a product (a == b: one primer with itself).  Count per block,
// k_loc_offsets, emit on a second visit: the products in the opening sites' order, a site's in its closing sites' order.
// No atomics: the same bytes on every run.  k_mux_tally counts the list per (fwd, rev, clean) with integer adds.

// the products of opening site i: on_hit(the closing site, its entry's length)
template <typename F>
__device__ inline void mux_walk(const PrimGeom& pg, const kr_product_site* __restrict__ sites, u64 ns, const u32* __restrict__ rec,
                                const u32* __restrict__ eoff, u32 max_product, u64 i, F&& on_hit) {
    const kr_product_site a = sites[i];
    if (a.entry >= pg.nleft2 || !prim_end_last(pg.nleft2, a.entry)) return;     // (a closing site)
    const u32 n1 = eoff[a.entry + 1] - eoff[a.entry];
    // (max_product >= 2 maxlen >= n1 + smin: the host refuses less, so first <= last and nothing wraps)
    const u64 first = a.pos + n1, last = a.pos + max_product - pg.smin;
    const u32 r = rec[i];
    for (u64 j = i + 1; j < ns; j++) {
        const kr_product_site b = sites[j];
        if (b.pos > last || rec[j] != r) break;
        if (b.pos < first) continue;
        if (b.entry >= pg.nleft2 || prim_end_last(pg.nleft2, b.entry)) continue;    // (an opening site)
        const u32 n2 = eoff[b.entry + 1] - eoff[b.entry];
        if (b.pos + n2 - a.pos > (u64)max_product) continue;
        on_hit(b, n2);
    }
}

// the join.  EMIT = false: bcount[block] = products (2^32 or more in a block set *overflow); EMIT = true: the products of
// the blocks with any, at boff[block]
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_mux_join(const kr_product_site* __restrict__ sites, u64 ns, const u32* __restrict__ rec,
                                                    PrimGeom pg, const u32* __restrict__ eoff, u32 max_product, u32* __restrict__ bcount,
                                                    const u64* __restrict__ boff, kr_multiplex_hit* __restrict__ out,
                                                    u32* __restrict__ overflow) {
    __shared__ u64 scan[LOC_T];
    const u64 bl = blockIdx.x;
    if (EMIT && bcount[bl] == 0) return;                          // (workgroup-uniform)
    const u64 i = bl * LOC_T + threadIdx.x;
    u64 cnt = 0;
    if (i < ns) mux_walk(pg, sites, ns, rec, eoff, max_product, i, [&](const kr_product_site&, u32) { cnt++; });
    kr_multiplex_hit* o = out + scan_epilogue<EMIT>(cnt, scan, bl, bcount, boff, overflow);
    if (!EMIT || i >= ns) return;
    const kr_product_site a = sites[i];
    mux_walk(pg, sites, ns, rec, eoff, max_product, i, [&](const kr_product_site& b, u32 n2) {
        kr_multiplex_hit hit;
        hit.pos = a.pos;
        hit.length = (u32)(b.pos + n2 - a.pos);
        hit.fwd = (uint16_t)(a.entry >> 1);
        hit.rev = (uint16_t)(b.entry >> 1);
        hit.fwd_mm = a.mismatches;
        hit.rev_mm = b.mismatches;
        hit.fwd_end_mm = a.end_mismatches;
        hit.rev_end_mm = b.end_mismatches;
        hit.pad[0] = hit.pad[1] = hit.pad[2] = hit.pad[3] = 0;
        *o++ = hit;
    });
}

// tally[2 (fwd T + rev) + clean] += the products of that ordered pair, clean = both 3' ends without a mismatch; the list is
// only read.  A wavefront takes 64 neighbouring products; a run of equal keys among them -- a repeat sends most of a
// genome's products to one pair -- is one add of its length (tally_runs).  A product that names a text >= T (there is none
// unless the join is broken) is not counted: no add outside the 2 T^2 counters
__global__ __launch_bounds__(256) void k_mux_tally(const kr_multiplex_hit* __restrict__ hits, u64 nhits, u32 T, u32* __restrict__ tally) {
    const u32 lane = threadIdx.x & 63u;
    // (the loop's bounds are the wavefront's: every lane of it takes every turn)
    for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < nhits; base += (u64)gridDim.x * 256) {
        const u64 i = base + lane;
        u32 key = ~0u;
        if (i < nhits) {
            const kr_multiplex_hit h = hits[i];
            const u32 clean = (h.fwd_end_mm == 0 && h.rev_end_mm == 0) ? 1u : 0u;
            if (h.fwd < T && h.rev < T) key = 2u * ((u32)h.fwd * T + h.rev) + clean;
        }
        tally_runs(key, lane, tally);
    }
}

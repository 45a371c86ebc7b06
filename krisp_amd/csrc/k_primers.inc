// k_primers.inc -- part of krisp_hip.hip (one translation unit): the primer-product pass (--out_primer_products): in-silico
// PCR of designed primer pairs, whose texts have every length in 10 .. 60, against a genome.  The host driver is
// h_primers.inc; the context and the genome on the device are the locate pass's; the tile layout, the staging, the seed
// table's slots and probe, the count / emit epilogue and the separator kernels are k_scan.inc's; the sites, the products,
// their records (k_prod_rec) and the pair lookup (prod_pair) are k_products.inc's.
//
// Entries are numbered as there: 2 i = left text i (A), 2 i + 1 = rc(A), nleft2 + 2 j = right text j (B), nleft2 + 2 j + 1
// = rc(B); entry e's text is arena[eoff[e], eoff[e + 1]).  A SITE is a valid window of the ENTRY'S OWN length within
// Hamming distance M of its text.  One length class of smin = the shortest text: every entry is seeded by the first smin
// columns of its text as it reads on the forward strand, cut into NP = M + 1 pieces.  A window within M of the whole text
// is within M on those columns, so one piece is equal (pigeonhole): the rolled window start is the site's position, and
// position order needs no sort.
//
// k_prim_scan stages a tile with maxlen - 1 bytes of overhang; a thread owns LOC_S starts of the smin-window and rolls
// the last bad byte and NP hashes.  prim_check compares the entry's whole length: the seeded columns, whose FIRST equal
// piece emits, and the tail, where a staged bad byte ('\n': a separator, N, lower case under omit, the genome's
// end) ends the window -- it is no mismatch.  Count per tile, k_loc_offsets, emit on a second visit: sites in position
// order, at one position by piece and list order.  k_prim_join: a thread per OPENING site walks the following sites of
// its record up to pos + max_product - smin and tests every CLOSING site with the two entries' own lengths.  No atomics:
// the same bytes on every run.  k_prim_tally (at the end) counts the product list per pair with integer adds.

struct PrimGeom {
    u32 smin, maxlen;               // the shortest and the longest text
    u32 omit, M, nleft2;
    u32 off[NEAR_MAXP + 1];         // piece j = columns [off[j], off[j + 1]) of the first smin
    u32 pw[NEAR_MAXP];              // LOC_HB^(length of the piece - 1)
};

// the 3' end of the primer lies in the LAST columns of A and of rc(B) as the text reads, in the FIRST of B and of rc(A);
// those entries open a product, the others close one
__host__ __device__ inline bool prim_end_last(u32 nleft2, u32 e) { return ((e < nleft2) ? 1u : 0u) != (e & 1u); }

// window p of the tile against entry e, found through piece `via`: on_hit(entry, mismatches, end mismatches)
template <u32 NP, typename F>
__device__ inline void prim_check(const PrimGeom& pg, const uint8_t* tile, const uint8_t* __restrict__ arena,
                                  const u32* __restrict__ eoff, u32 p, u32 e, u32 via, F&& on_hit) {
    const u32 t0 = eoff[e], n = eoff[e + 1] - t0;
    const uint8_t* f = arena + t0;
    const bool last = prim_end_last(pg.nleft2, e);
    const u32 elo = last ? n - PROD_END : 0u, ehi = last ? n : PROD_END;    // (n >= 10 > PROD_END: the host refuses less)
    // one walk over the entry's whole length (a single loop keeps the kernel's scalar registers in bounds): pmask's bit j =
    // piece j of the seeded columns differs.  The seeded columns hold no bad byte (the caller's `bad`); in the tail beyond
    // them (p + n - 1 <= LOC_T * LOC_S + maxlen - 2: staged) a staged bad byte ends the window -- it is no mismatch
    u32 mm = 0, em = 0, pmask = 0;
    #pragma unroll 1
    for (u32 q = 0; q < n; q++) {
        const u32 b = tile[loc_at(p + q)];
        if (b == '\n') return;                      // the window is no window of this length
        const u32 ne = b != f[q];
        u32 j = 0;
#pragma unroll
        for (u32 t = 1; t < NP; t++) j += q >= pg.off[t];
        pmask |= (ne & (u32)(q < pg.smin)) << j;
        mm += ne;
        em += ne & (u32)(q >= elo && q < ehi);
        if (mm > pg.M) return;
    }
    // the FIRST equal piece emits the pair: the pieces before `via` differ, piece `via` is equal (else: a hash collision)
    if ((pmask & ((2u << via) - 1u)) != (1u << via) - 1u) return;
    on_hit(e, mm, em);
}

// one thread's window starts [s, e) of the staged tile: on_hit(p, entry, mismatches, end mismatches), position order
template <u32 NP, typename F>
__device__ inline void prim_roll(const PrimGeom& pg, const uint8_t* tile, const u32* bm, const NearSlot* __restrict__ table, u64 tmask,
                                 const u32* __restrict__ list, const uint8_t* __restrict__ arena, const u32* __restrict__ eoff,
                                 u32 s, u32 e, F&& on_hit) {
    if (s >= e) return;
    u32 h[NP];
    int bad = -1;                   // the last bad byte in [s, s + smin)
#pragma unroll
    for (u32 j = 0; j < NP; j++) {
        u32 x = 0;
        #pragma unroll 1
        for (u32 q = pg.off[j]; q < pg.off[j + 1]; q++) x = x * LOC_HB + tile[loc_at(s + q)];
        h[j] = x;
    }
    #pragma unroll 1
    for (u32 j = pg.smin; j-- > 0;)
        if (tile[loc_at(s + j)] == '\n') { bad = (int)(s + j); break; }
    for (u32 p = s;; p++) {
        if (bad < (int)p) {
#pragma unroll
            for (u32 j = 0; j < NP; j++)
                seed_probe(bm, table, tmask, list, near_key(j, h[j]), [&](u32 en) {
                    prim_check<NP>(pg, tile, arena, eoff, p, en, j, [&](u32 en, u32 mm, u32 em) { on_hit(p, en, mm, em); });
                });
        }
        if (p + 1 >= e) break;
        // slide to p + 1: the byte that leaves piece j + 1 enters piece j
        u32 out = tile[loc_at(p)];
#pragma unroll
        for (u32 j = 0; j < NP; j++) {
            const u32 in = tile[loc_at(p + pg.off[j + 1])];
            h[j] = (h[j] - out * pg.pw[j]) * LOC_HB + in;
            out = in;
        }
        if (out == '\n') bad = (int)(p + pg.smin);  // (the last piece's new byte is byte p + smin)
    }
}

// the site scan: persistent workgroups over tiles of LOC_T * LOC_S window starts of the smin-window.  EMIT = false:
// tcount[tile] = sites (a tile with 2^32 or more sets *overflow); EMIT = true: the sites of the tiles with any, at
// toff[tile] (k_loc_offsets)
template <u32 NP, bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_prim_scan(const uint8_t* __restrict__ bases, u64 n, PrimGeom pg,
                                                     const u32* __restrict__ bitmap, const NearSlot* __restrict__ table, u64 tmask,
                                                     const u32* __restrict__ list, const uint8_t* __restrict__ arena,
                                                     const u32* __restrict__ eoff, u64 nw, u64 ntiles, u32* __restrict__ tcount,
                                                     const u64* __restrict__ toff, kr_product_site* __restrict__ out,
                                                     u32* __restrict__ overflow) {
    extern __shared__ __align__(16) u32 prim_lds[];
    u32* bm = prim_lds;                                           // LOC_BM_WORDS
    u64* scan = (u64*)(bm + LOC_BM_WORDS);                        // LOC_T
    uint8_t* tile = (uint8_t*)(scan + LOC_T);                     // loc_at(LOC_T * LOC_S + maxlen - 1) bytes
    scan_load_bitmap(bm, bitmap);
    const u32 TP = LOC_T * LOC_S;
    for (u64 tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        if (EMIT && tcount[tl] == 0) continue;                    // (workgroup-uniform)
        const u64 t0 = tl * TP;
        scan_stage_tile(bases, n, t0, TP + pg.maxlen - 1, pg.omit, tile);
        u32 s, e;
        scan_lane_starts(nw, t0, &s, &e);
        u64 cnt = 0;
        prim_roll<NP>(pg, tile, bm, table, tmask, list, arena, eoff, s, e, [&](u32, u32, u32, u32) { cnt++; });
        kr_product_site* o = out + scan_epilogue<EMIT>(cnt, scan, tl, tcount, toff, overflow);
        if (!EMIT) continue;
        prim_roll<NP>(pg, tile, bm, table, tmask, list, arena, eoff, s, e, [&](u32 p, u32 en, u32 mm, u32 em) {
            kr_product_site site;
            site.pos = t0 + p;
            site.entry = en;
            site.mismatches = (uint8_t)mm;
            site.end_mismatches = (uint8_t)em;
            site.pad = 0;
            *o++ = site;
        });
    }
}

// the products of opening site i: on_hit(the closing site, pair, plus strand, the closing entry's length)
template <typename F>
__device__ inline void prim_walk(const PrimGeom& pg, const kr_product_site* __restrict__ sites, u64 ns, const u32* __restrict__ rec,
                                 const u32* __restrict__ eoff, const u64* __restrict__ keys, const u32* __restrict__ idx, u32 npairs,
                                 u32 max_product, u64 i, F&& on_hit) {
    const kr_product_site a = sites[i];
    if (!prim_end_last(pg.nleft2, a.entry)) return;               // (a closing site)
    const bool plus = a.entry < pg.nleft2;                        // A ... B; otherwise rc(B) ... rc(A)
    const u32 n1 = eoff[a.entry + 1] - eoff[a.entry];
    // (max_product >= smin + smin: the host refuses a max_product below a pair's two texts, and there is a pair.  A text that
    // no pair names may give first > last: the walk then ends at its first step)
    const u64 first = a.pos + n1, last = a.pos + max_product - pg.smin;
    const u32 r = rec[i];
    for (u64 j = i + 1; j < ns; j++) {
        const kr_product_site b = sites[j];
        if (b.pos > last || rec[j] != r) break;
        if (b.pos < first) continue;
        // the closing site on this strand: B as written after A, rc(A) after rc(B)
        if ((b.entry < pg.nleft2) == plus || (b.entry & 1u) == (plus ? 1u : 0u)) continue;
        const u32 n2 = eoff[b.entry + 1] - eoff[b.entry];
        if (b.pos + n2 - a.pos > (u64)max_product) continue;
        const u32 li = (plus ? a.entry : b.entry) >> 1, rj = ((plus ? b.entry : a.entry) - pg.nleft2) >> 1;
        const u32 pr = prod_pair(keys, idx, npairs, li, rj);
        if (pr != LOC_EMPTY) on_hit(b, pr, plus, n2);
    }
}

// the join: a thread per site, a workgroup per LOC_T sites.  EMIT = false: bcount[block] = products (2^32 or more in a
// block set *overflow); EMIT = true: the products of the blocks with any, at boff[block], in the opening sites' order
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_prim_join(const kr_product_site* __restrict__ sites, u64 ns, const u32* __restrict__ rec,
                                                     PrimGeom pg, const u32* __restrict__ eoff, const u64* __restrict__ keys,
                                                     const u32* __restrict__ idx, u32 npairs, u32 max_product, u32* __restrict__ bcount,
                                                     const u64* __restrict__ boff, kr_product_hit* __restrict__ out,
                                                     u32* __restrict__ overflow) {
    __shared__ u64 scan[LOC_T];
    const u64 bl = blockIdx.x;
    if (EMIT && bcount[bl] == 0) return;                          // (workgroup-uniform)
    const u64 i = bl * LOC_T + threadIdx.x;
    u64 cnt = 0;
    if (i < ns)
        prim_walk(pg, sites, ns, rec, eoff, keys, idx, npairs, max_product, i, [&](const kr_product_site&, u32, bool, u32) { cnt++; });
    kr_product_hit* o = out + scan_epilogue<EMIT>(cnt, scan, bl, bcount, boff, overflow);
    if (!EMIT || i >= ns) return;
    const kr_product_site a = sites[i];
    prim_walk(pg, sites, ns, rec, eoff, keys, idx, npairs, max_product, i, [&](const kr_product_site& b, u32 pr, bool plus, u32 n2) {
        const kr_product_site& lf = plus ? a : b;                 // the site of the left text (A or rc(A))
        const kr_product_site& rt = plus ? b : a;
        kr_product_hit hit;
        hit.pos = a.pos;
        hit.length = (u32)(b.pos + n2 - a.pos);
        hit.pair = pr;
        hit.strand = plus ? 0 : 1;
        hit.left_mm = lf.mismatches;
        hit.right_mm = rt.mismatches;
        hit.left_end_mm = lf.end_mismatches;
        hit.right_end_mm = rt.end_mismatches;
        hit.pad[0] = hit.pad[1] = hit.pad[2] = 0;
        *o++ = hit;
    });
}

// k_prim_tally (--primer-candidates, DESIGN §25): tally[8 pair + m] += the products of that pair whose two sites hold m
// mismatches together, m = 0 .. 6, and tally[8 pair + 7] += those of them without a mismatch at either 3' end; the list is
// only read.  A wavefront takes 64 neighbouring products, in two turns of tally_runs (k_scan.inc): a run of equal keys among
// them -- a repeat sends most of a genome's products to one pair -- is one integer add of its length.  A product that names
// no pair of the table or a site with more than 3 mismatches (there is none unless the join is broken) is not counted: no
// add outside the 8 npairs counters
__global__ __launch_bounds__(256) void k_prim_tally(const kr_product_hit* __restrict__ hits, u64 nhits, u32 npairs, u32* __restrict__ tally) {
    const u32 lane = threadIdx.x & 63u;
    // (the loop's bounds are the wavefront's: every lane of it takes every turn, the shuffle and the ballot are whole)
    for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < nhits; base += (u64)gridDim.x * 256) {
        const u64 i = base + lane;
        u32 key = ~0u, clean = ~0u;
        if (i < nhits) {
            const kr_product_hit h = hits[i];
            if (h.pair < npairs && h.left_mm < 4u && h.right_mm < 4u) {
                key = 8u * h.pair + h.left_mm + h.right_mm;
                if (h.left_end_mm == 0 && h.right_end_mm == 0) clean = 8u * h.pair + 7u;
            }
        }
        tally_runs(key, lane, tally);
        tally_runs(clean, lane, tally);
    }
}

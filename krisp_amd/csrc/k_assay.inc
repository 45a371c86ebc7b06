// k_assay.inc -- part of krisp_hip.hip (one translation unit): the assay join (--out_assay_hits, DESIGN §21): the guide hits
// that lie inside the interiors of the primer products of one genome.  The host driver is h_assay.inc; the products are
// the primer pass's list (k_primers.inc: kr_product_hit, in the opening sites' order: positions ascend), the hits the
// guide-hit pass's (k_guide_hits.inc: kr_guide_hit, positions ascend), both on the device behind their scans; the count /
// emit epilogue is k_scan.inc's.
//
// A product of pair p on strand s has its FIRST site's text length -- the left text's on strand 0, the right text's on
// strand 1 -- and its SECOND site's; its interior is [pos + first, pos + length - second).  An assay hit is a product and a
// hit whose window of G bases lies inside the interior, with (pair, guide) a LINK: a row of the ascending list of 64-bit
// keys pair << 32 | guide.  k_assay_join: a thread per product, a workgroup per LOC_T products.  The thread loads its
// pair's two lengths (plen[pair] = left | right << 16), finds the first hit at or behind interior.lo by binary search,
// walks forward while the window ends inside the interior and looks every (pair, guide) up in the links by binary search.
// Products ascend by position, so neighbouring lanes search neighbouring ranges.  The walk reads a hit's pos and guide
// alone, the emit the rest.  Count per block, k_loc_offsets, emit on a second visit: no atomics, plain stores, the same
// bytes on every run.  Neither list is written.  A thread walks alone: a product whose interior holds very many hits costs
// products x hits in range (as k_prod_join's walk does, DESIGN §13).

struct AssayLists {
    const kr_product_hit* prods;    // np products
    const kr_guide_hit* hits;       // nh hits, positions ascending
    const u32* plen;                // npairs rows: the pair's left | right << 16 text lengths
    const u64* links;               // nl keys, strictly ascending
    u64 np, nh, nl;
    u32 npairs, G;
};

// the interior [*lo, *hi) of product p with its pair's lengths pl; false: it holds no window of G bases
__host__ __device__ inline bool assay_interior(const kr_product_hit& p, u32 pl, u32 G, u64* lo, u64* hi) {
    const u32 nl = pl & 0xFFFFu, nr = pl >> 16;
    const u32 first = p.strand ? nr : nl, second = p.strand ? nl : nr;
    if ((u64)first + second + G > (u64)p.length) return false;
    *lo = p.pos + first;
    *hi = p.pos + p.length - second;
    return true;
}

// whether `key` is one of the nl ascending keys
__host__ __device__ inline bool assay_linked(const u64* __restrict__ links, u64 nl, u64 key) {
    u64 b = 0, e = nl;
    while (b < e) {
        const u64 m = b + ((e - b) >> 1);           // (b <= m < e <= nl)
        const u64 v = links[m];
        if (v == key) return true;
        if (v < key) b = m + 1; else e = m;
    }
    return false;
}

// the assay hits of product i: on_hit(the product, the hit's index)
template <typename F>
__device__ inline void assay_walk(const AssayLists& a, u64 i, F&& on_hit) {
    const kr_product_hit p = a.prods[i];            // (i < np: the caller's)
    if (p.pair >= a.npairs) return;                 // (no product names such a pair: the bound of plen)
    u64 lo, hi;
    if (!assay_interior(p, a.plen[p.pair], a.G, &lo, &hi)) return;
    u64 b = 0, e = a.nh;                            // the first hit with pos >= lo
    while (b < e) {
        const u64 m = b + ((e - b) >> 1);           // (b <= m < e <= nh)
        if (a.hits[m].pos < lo) b = m + 1; else e = m;
    }
    for (u64 j = b; j < a.nh; j++) {
        if (a.hits[j].pos + a.G > hi) break;
        if (assay_linked(a.links, a.nl, ((u64)p.pair << 32) | a.hits[j].guide)) on_hit(p, j);
    }
}

// EMIT = false: bcount[block] = assay hits (2^32 or more in a block set *overflow); EMIT = true: the assay hits of the
// blocks with any, at boff[block], in the products' order, a product's in the hits' order
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_assay_join(AssayLists a, u32* __restrict__ bcount, const u64* __restrict__ boff,
                                                      kr_assay_hit* __restrict__ out, u32* __restrict__ overflow) {
    __shared__ u64 scan[LOC_T];
    const u64 bl = blockIdx.x;
    if (EMIT && bcount[bl] == 0) return;                          // (workgroup-uniform)
    const u64 i = bl * LOC_T + threadIdx.x;
    u64 cnt = 0;
    if (i < a.np) assay_walk(a, i, [&](const kr_product_hit&, u64) { cnt++; });
    kr_assay_hit* o = out + scan_epilogue<EMIT>(cnt, scan, bl, bcount, boff, overflow);
    if (!EMIT || i >= a.np) return;
    assay_walk(a, i, [&](const kr_product_hit& p, u64 j) {
        const kr_guide_hit h = a.hits[j];
        kr_assay_hit r;
        r.pos = p.pos;
        r.length = p.length;
        r.pair = p.pair;
        r.strand = p.strand;
        r.left_mm = p.left_mm;
        r.right_mm = p.right_mm;
        r.left_end_mm = p.left_end_mm;
        r.right_end_mm = p.right_end_mm;
        r.hit_strand = h.strand;
        r.hit_mismatches = h.mismatches;
        r.hit_pam = h.pam;
        r.hit_pos = h.pos;
        r.columns = h.columns;
        r.guide = h.guide;
        r.hit = (u32)j;                             // (nh < 2^32)
        *o++ = r;
    });
}

// k_guide_bulges.inc -- part of krisp_hip.hip (one translation unit): the bulged guide-hit pass (--guide-hit-bulges): every
// window of a genome that lies within M columns of a picked guide's protospacer once b = 1 .. B bases of the genome (a DNA
// bulge) or b letters of the guide (an RNA bulge) are left without a partner, on both strands (DESIGN §20).  The host
// driver is h_guide_bulges.inc.
//
// The seeds are the near-match pass's scan (k_near.inc), launched by the host unchanged over the guides' HALVES: texts of
// h = (G - B) / 2 letters, T[0, h) and T[G - h, G) of every guide, with a NearGeom of k = h.  Whatever the cut, one half
// lies whole on its side of the bulge and within M of its end of the window.  The scan leaves kr_near_hit pairs (half text,
// strand, distance, position).
//
// k_gbulge_extend then runs the per-pair step (gbulge_step.inc), a thread per pair: for each of the 2 B bulges the window
// that the half fixes, read from the genome's bytes in global memory with every index bounds-checked -- a right half's
// window starts LEFT of its seed, in the tile before or before the text --, its least distance over the cuts, the canonical
// cut, the column mask and the motifs.  A pair writes the rows it owns (the step's rule: a row has one owner), 0 to 2 B of
// them, through the scaffold's two passes over blocks of LOC_T pairs.  No atomics: the same bytes on every run.
//
// k_gbulge_cut cuts the rows' windows, each of its own length, into rows of G + B bytes padded with 0.
#include "gbulge_step.inc"

struct GbulgeGeom {
    u32 G, h, B, M, omit, need;
    u32 nhalves;                    // texts of the seed table: 2 * guides
    GhitMotifs gm;
};

// EMIT = false: cnt[block] = the rows of the block's pairs; EMIT = true: the rows at off[block], pair after pair, a pair's
// in the order DNA 1, RNA 1, DNA 2, RNA 2.  A pair that names no half of the table -- there is none unless the scan is
// broken -- indexes nothing and writes nothing
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_gbulge_extend(const uint8_t* __restrict__ bases, u64 n, const uint8_t* __restrict__ texts,
                                                         GbulgeGeom gg, const kr_near_hit* __restrict__ pairs, u64 npairs,
                                                         u32* __restrict__ cnt, const u64* __restrict__ off,
                                                         kr_guide_bulge_hit* __restrict__ out) {
    __shared__ u32 scan[LOC_T];
    const u64 tl = blockIdx.x;
    if (EMIT && cnt[tl] == 0) return;                             // (workgroup-uniform)
    const u64 i = tl * LOC_T + threadIdx.x;
    kr_near_hit e;
    e.target = 0xFFFFFFFFu; e.strand = 0; e.pos = 0;
    if (i < npairs) e = pairs[i];
    const bool live = i < npairs && e.target < gg.nhalves;
    const u32 strand = e.strand & 1u, guide = e.target >> 1;
    const u32 half = strand ? 1u - (e.target & 1u) : (e.target & 1u);      // the half in the entry's orientation
    const uint8_t* text = texts + (u64)(2 * guide + strand) * gg.G;
    auto step = [&](u32 j, int64_t* start, u32* pam) {
        return gbulge_pair(bases, n, e.pos, half, gg.h, text, gg.G, strand, gbulge_of(j), gg.M, gg.omit, gg.gm.sets5, gg.gm.a,
                           gg.gm.sets3, gg.gm.b, gg.need, start, pam);
    };
    u32 c = 0, owned = 0;                                         // owned bit j: bulge j is a row of this pair
    if (live)
        for (u32 j = 0; j < 2 * gg.B; j++) {
            int64_t start;
            u32 pam;
            const u32 hit = step(j, &start, &pam).hit;
            c += hit;
            owned |= hit << j;
        }
    kr_guide_bulge_hit* o = out + scan_epilogue<EMIT>(c, scan, tl, cnt, off, nullptr);
    if (!EMIT || !c) return;
    u32 w = 0;
    for (u32 j = 0; j < 2 * gg.B; j++) {
        if (!((owned >> j) & 1u)) continue;                       // (the step again only for the rows: it is not kept per bulge)
        int64_t start;
        u32 pam;
        const GbulgeStep r = step(j, &start, &pam);
        if (!r.hit || w >= c) continue;
        kr_guide_bulge_hit h;
        h.guide = guide;
        h.strand = (uint8_t)strand;
        h.mismatches = (uint8_t)r.mismatches;
        h.pam = (uint8_t)pam;
        h.bulge = (int8_t)gbulge_of(j);
        h.pos = (u64)start;
        h.columns = r.columns;
        h.bulge_column = r.bulge_column;
        h.length = r.length;
        o[w] = h;
        w++;
    }
}

// the text of the rows' windows, a row of W = G + B bytes per hit: the hit's `length` letters, upper case, the reverse
// complement over that length for strand 1, then 0.  A hit whose window does not lie in the n bases -- there is none -- is
// a row of 0
__global__ __launch_bounds__(256) void k_gbulge_cut(const uint8_t* __restrict__ bases, u64 n, const kr_guide_bulge_hit* __restrict__ hits,
                                                    u64 nhits, u32 W, uint8_t* __restrict__ rows) {
    const u64 total = nhits * W;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
        const u64 h = i / W;
        const u32 j = (u32)(i - h * W);
        const kr_guide_bulge_hit e = hits[h];
        uint8_t out = 0;
        if (e.length <= W && j < e.length && e.pos <= n && (u64)e.length <= n - e.pos) {
            u32 b = bases[e.pos + (e.strand ? e.length - 1 - j : j)];
            if (b >= 'a' && b <= 'z') b -= 32;
            out = e.strand ? loc_comp((uint8_t)b) : (uint8_t)b;
        }
        rows[i] = out;
    }
}

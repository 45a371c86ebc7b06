// k_guide_hits.inc -- part of krisp_hip.hip (one translation unit): the guide-hit pass (--out_guide_hits): every window of a
// genome within Hamming distance M of a picked guide's protospacer, on both strands, with the columns that differ and
// whether the PAM / PFS motifs lie beside it (DESIGN §19).  The host driver is h_guide_hits.inc.
//
// The scan IS the near-match pass's (k_near.inc): the host launches k_near_scan<NP, EMIT> itself, unchanged -- the tile, its
// staging, the pigeonhole seeds, near_roll and near_check (a NearGeom with lo = 0 and hi = k = G: no flank, the flank
// count is 0 and ignored), the seed table's probe, the count / emit epilogue -- over the guides' table; it leaves a list
// of kr_near_hit (target = guide, strand, distance, position) in position order, then piece, then the entry list's order.
//
// k_ghit_finish then runs the per-hit step (ghit_step.inc), a thread per pair, and writes the kr_guide_hit: the column
// mask and the motif bits, read from the genome's bytes in global memory with every index bounds-checked -- the 5' motif
// of a '+' hit lies LEFT of its window, and nothing left of a window is ever read from a tile.  (DESIGN §19 has why the
// step is no part of the scan: called from near_roll's on_hit it made the scan park up to 118 scalar registers in vector
// lanes, over the library's bound; hits are rare, so a second touch of each costs nothing.)
//
// With need_pam, k_ghit_keep keeps the hits whose motif bits are 3, in their order (count, k_loc_offsets, emit: the
// scaffold's two passes over blocks of LOC_T hits).  No atomics in the scan or the selection: the same bytes on every run.
//
// k_ghit_tally (--guide-candidates, DESIGN §22) counts the list per (guide, mismatches) for callers that want the counts and
// not the hits: integer atomic adds, so its sums too are the same on every run.
#include "ghit_step.inc"

struct GhitMotifs {
    u32 sets5, a, sets3, b;         // the motifs as 4-bit base sets, letter j in bits [4 j, 4 j + 4), and their lengths
};

// the per-hit step over the scan's pairs: hit i = pair i with its column mask and motif bits.  The step counts the distance
// again and finds every window free of bad bytes: the scan reports no other pair, so r.mismatches == e.mismatches and
// r.ok == 1 (the GPU tests hold both through the reference).  A pair that names no guide of the table -- there is none
// unless the scan is broken -- indexes nothing: it becomes a hit with pam = 0 and 255 mismatches, a wrong row instead of
// a read outside the entries' text
__global__ __launch_bounds__(256) void k_ghit_finish(const uint8_t* __restrict__ bases, u64 n, const uint8_t* __restrict__ arena, u32 G,
                                                     u32 omit, GhitMotifs gm, u32 nguides,
                                                     const kr_near_hit* __restrict__ pairs, kr_guide_hit* __restrict__ hits,
                                                     u64 nhits) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < nhits; i += (u64)gridDim.x * 256) {
        const kr_near_hit e = pairs[i];
        const u32 strand = e.strand & 1u;
        GhitStep r;
        r.ok = 0u; r.mismatches = 255u; r.pam = 0u; r.columns = 0ull;
        if (e.target < nguides)
            r = ghit_finish(bases, n, e.pos, arena + (u64)(2 * e.target + strand) * G, G, strand, omit, gm.sets5, gm.a, gm.sets3, gm.b);
        kr_guide_hit h;
        h.guide = e.target;
        h.strand = (uint8_t)strand;
        h.mismatches = (uint8_t)r.mismatches;
        h.pam = (uint8_t)r.pam;
        h.pad = 0;
        h.pos = e.pos;
        h.columns = r.columns;
        hits[i] = h;
    }
}

// need_pam: the hits with both motifs beside them, in their order; a workgroup per LOC_T hits.  EMIT = false: cnt[block];
// EMIT = true: the kept hits at off[block]
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_ghit_keep(const kr_guide_hit* __restrict__ hits, u64 nhits, u32* __restrict__ cnt,
                                                     const u64* __restrict__ off, kr_guide_hit* __restrict__ out) {
    __shared__ u32 scan[LOC_T];
    const u64 tl = blockIdx.x;
    if (EMIT && cnt[tl] == 0) return;                             // (workgroup-uniform)
    const u64 i = tl * LOC_T + threadIdx.x;
    const bool keep = i < nhits && hits[i].pam == 3;
    kr_guide_hit* o = out + scan_epilogue<EMIT>((u32)keep, scan, tl, cnt, off, nullptr);
    if (EMIT && keep) *o = hits[i];
}

// tally[4 guide + mismatches] += the hits of that guide at that distance; the list is only read.  A wavefront takes 64
// neighbouring hits; a run of equal (guide, mismatches) among them -- a repeat sends most of a genome's hits to one guide --
// is one add of its length by its first lane (k_scan.inc: tally_runs).  A hit that names no guide of the table or a distance above 3 (there is none
// unless the scan is broken) is not counted: no add outside the 4 nguides counters
__global__ __launch_bounds__(256) void k_ghit_tally(const kr_guide_hit* __restrict__ hits, u64 nhits, u32 nguides, u32* __restrict__ tally) {
    const u32 lane = threadIdx.x & 63u;
    // (the loop's bounds are the wavefront's: every lane of it takes every turn, the shuffle and the ballot are whole)
    for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < nhits; base += (u64)gridDim.x * 256) {
        const u64 i = base + lane;
        u32 key = ~0u;
        if (i < nhits) {
            const kr_guide_hit h = hits[i];
            if (h.guide < nguides && h.mismatches < 4u) key = 4u * h.guide + h.mismatches;
        }
        tally_runs(key, lane, tally);
    }
}

// gbulge_step.inc -- part of krisp_hip.hip, and of tests/gbulge_step_check.cpp: what the bulged guide-hit pass
// (k_guide_bulges.inc) does for ONE seed pair and one bulge, in plain C++ for host and device: no HIP call, no LDS, no
// thread index.  A translation unit without HIP defines __host__ and __device__ empty before it includes this file, and
// includes ghit_step.inc first (ghit_byte, ghit_pam).
//
// A bulged hit is a window of Lw = G + b bases (a DNA bulge: b bases of the genome have no partner in the guide) or
// Lw = G - b bases (an RNA bulge: b letters of the guide have no partner in the genome) that, cut at q, lies within M
// columns of an entry's text (DESIGN §20).  The seeds are the entries' two halves of h letters; a seed pair names where one
// half lies.  A left half's window starts at the seed, a right half's ENDS with it: that start lies LEFT of the seed, so
// the step reads the genome's bytes as uploaded -- never a tile -- and every index is tested against 0 <= i < n.
#include <stdint.h>

struct GbulgeStep {
    uint32_t hit;                   // the window lies in the text, holds no bad byte and is within M at some cut
    uint32_t mismatches;            // the least mm(q)
    uint32_t q;                     // the canonical cut, in the entry's orientation
    uint32_t bulge_column;          // the guide columns 5' of the bulge on the guide's strand
    uint32_t length;                // Lw
    uint64_t columns;               // bit c: aligned guide column c differs, 5'->3' on the protospacer
};

// the window [start, start + G + bulge) against an entry's text of G letters; bulge = +b (DNA) or -b (RNA), b = 1 or 2.
// mm(q) = the columns below q that differ with the window aligned at its start + the columns from q (DNA) or q + b (RNA)
// that differ with it aligned at its end: two masks, two popcounts a cut.  Of the cuts with the least mm the one with the
// smallest bulge_column: the smallest q of an even entry, the largest of an odd one
__host__ __device__ inline GbulgeStep gbulge_window(const uint8_t* bases, uint64_t n, int64_t start, const uint8_t* text, uint32_t G,
                                                    uint32_t strand, int32_t bulge, uint32_t M, uint32_t omit) {
    GbulgeStep r;
    r.hit = 0u; r.mismatches = 255u; r.q = 0u; r.bulge_column = 0u; r.columns = 0ull;
    const uint32_t Lw = (uint32_t)((int32_t)G + bulge);
    r.length = Lw;
    if (start < 0 || (uint64_t)start + Lw > n) return r;
    uint64_t head = 0, tail = 0;    // bit c: text column c differs from window byte c / from window byte c + bulge
    bool ok = true;
    for (uint32_t i = 0; i < Lw; i++) {
        const uint32_t w = ghit_byte(bases, n, start + (int64_t)i, omit);
        if (w == '\n') ok = false;
        if (i < G && w != text[i]) head |= 1ull << i;
        const int32_t c = (int32_t)i - bulge;
        if (c >= 0 && c < (int32_t)G && w != text[c]) tail |= 1ull << c;
    }
    if (!ok) return r;
    const uint32_t skip = bulge < 0 ? (uint32_t)-bulge : 0u;      // the guide letters without a partner
    uint32_t best = 255u, bq = 0u;
    for (uint32_t q = 1; q + skip < G; q++) {
        const uint32_t mm = (uint32_t)__builtin_popcountll(head & ((1ull << q) - 1)) + (uint32_t)__builtin_popcountll(tail >> (q + skip));
        if (mm < best || (strand && mm == best)) { best = mm; bq = q; }
    }
    if (best > M) return r;
    const uint64_t m = (head & ((1ull << bq) - 1)) | (tail >> (bq + skip) << (bq + skip));
    r.hit = 1u;
    r.mismatches = best;
    r.q = bq;
    if (!strand) {
        r.bulge_column = bq;
        r.columns = m;
    } else {
        r.bulge_column = G - bq - skip;
        for (uint32_t c = 0; c < G; c++)
            if ((m >> c) & 1ull) r.columns |= 1ull << (G - 1u - c);
    }
    return r;
}

// bulge number j of a pair's 2 B: DNA 1, RNA 1, DNA 2, RNA 2
__host__ __device__ inline int32_t gbulge_of(uint32_t j) {
    const int32_t b = (int32_t)(j >> 1) + 1;
    return (j & 1u) ? -b : b;
}

// the seed pair (half `half` of the entry -- 0 = text[0, h), 1 = text[G - h, G) -- lies at seed) and one bulge: the row the
// pair OWNS, if any.  The left half owns the rows whose canonical cut is >= h, the right half the others: every row has a
// half that its cut leaves whole (2 h <= G - b + 1), that half is within M, so its pair exists, and exactly one of a row's
// pairs owns it.  *pam = ghit_pam over the window's real ends; need != 0: a row whose pam != 3 is no row
__host__ __device__ inline GbulgeStep gbulge_pair(const uint8_t* bases, uint64_t n, uint64_t seed, uint32_t half, uint32_t h,
                                                  const uint8_t* text, uint32_t G, uint32_t strand, int32_t bulge, uint32_t M,
                                                  uint32_t omit, uint32_t sets5, uint32_t a, uint32_t sets3, uint32_t b, uint32_t need,
                                                  int64_t* start_out, uint32_t* pam) {
    const int64_t Lw = (int64_t)G + bulge;
    const int64_t start = half ? (int64_t)seed + (int64_t)h - Lw : (int64_t)seed;
    GbulgeStep r = gbulge_window(bases, n, start, text, G, strand, bulge, M, omit);
    *start_out = start;
    *pam = 0u;
    if (!r.hit) return r;
    if ((r.q >= h) != (half == 0u)) {
        r.hit = 0u;
        return r;
    }
    *pam = ghit_pam(bases, n, (uint64_t)start, (uint32_t)Lw, strand, omit, sets5, a, sets3, b);
    if (need && *pam != 3u) r.hit = 0u;
    return r;
}

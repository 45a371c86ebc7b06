// ghit_step.inc -- part of krisp_hip.hip, and of tests/ghit_step_check.cpp: what the guide-hit scan (k_guide_hits.inc) does
// for ONE hit, in plain C++ for host and device: no HIP call, no LDS, no thread index.  A translation unit without HIP
// defines __host__ and __device__ empty before it includes this file.
//
// A hit is a window [pos, pos + G) of the genome within M columns of an entry's text (DESIGN §19).  The step reads the
// window and the motifs' neighbours from the genome's bytes as uploaded -- never from a tile -- and every index is tested
// against 0 <= i < n before the load: an index outside is a bad byte, never a read.  So the 5' motif of a '+' hit, which
// lies LEFT of the window, needs no halo in the scan's tile.
#include <stdint.h>

// loc_stage_byte (k_scan.inc), restated: tests/test_guide_hits_step.py holds the two bodies to each other
__host__ __device__ inline uint32_t ghit_stage_byte(uint32_t b, uint32_t omit) {
    const bool lower = b >= 'a' && b <= 'z';
    if (b == '\n' || b == 'N' || b == 'n' || (omit && lower)) return '\n';
    return lower ? b - 32 : b;
}

// staged byte i of the n bases; an index outside the text is a bad byte
__host__ __device__ inline uint32_t ghit_byte(const uint8_t* bases, uint64_t n, int64_t i, uint32_t omit) {
    if (i < 0 || (uint64_t)i >= n) return '\n';
    return ghit_stage_byte(bases[i], omit);
}

// a staged byte as a 4-bit base set (A = 1, C = 2, G = 4, T = 8); 0 for a bad byte and for every other letter
__host__ __device__ inline uint32_t ghit_base_set(uint32_t b) {
    return b == 'A' ? 1u : b == 'C' ? 2u : b == 'G' ? 4u : b == 'T' ? 8u : 0u;
}

// ... and the set of its complement: A <-> T, C <-> G
__host__ __device__ inline uint32_t ghit_comp_set(uint32_t s) {
    return ((s & 1u) << 3) | ((s & 2u) << 1) | ((s & 4u) >> 1) | ((s & 8u) >> 3);
}

// does the motif -- len letters, letter j the 4-bit set in bits [4 j, 4 j + 4) of `sets`, read 5'->3' on the guide's strand
// -- match the neighbours first, first + step, ...?  strand 1 complements each neighbour
__host__ __device__ inline bool ghit_motif(const uint8_t* bases, uint64_t n, int64_t first, int64_t step, uint32_t strand,
                                           uint32_t omit, uint32_t sets, uint32_t len) {
    for (uint32_t j = 0; j < len; j++) {
        uint32_t s = ghit_base_set(ghit_byte(bases, n, first + (int64_t)j * step, omit));
        if (strand) s = ghit_comp_set(s);
        if (!(s & (sets >> (4 * j)) & 15u)) return false;
    }
    return true;
}

// the motif bits of the window at pos: bit 0 = the 5' motif (a letters), bit 1 = the 3' motif (b letters).  '+': the 5'
// motif reads [pos - a, pos), the 3' motif [pos + G, pos + G + b); '-': the 5' motif reads rc([pos + G, pos + G + a)), the
// 3' motif rc([pos - b, pos))
__host__ __device__ inline uint32_t ghit_pam(const uint8_t* bases, uint64_t n, uint64_t pos, uint32_t G, uint32_t strand,
                                             uint32_t omit, uint32_t sets5, uint32_t a, uint32_t sets3, uint32_t b) {
    const int64_t p = (int64_t)pos, e = p + (int64_t)G;
    bool m5, m3;
    if (!strand) {
        m5 = ghit_motif(bases, n, p - (int64_t)a, 1, 0u, omit, sets5, a);
        m3 = ghit_motif(bases, n, e, 1, 0u, omit, sets3, b);
    } else {
        m5 = ghit_motif(bases, n, e + (int64_t)a - 1, -1, 1u, omit, sets5, a);
        m3 = ghit_motif(bases, n, p - 1, -1, 1u, omit, sets3, b);
    }
    return (m5 ? 1u : 0u) | (m3 ? 2u : 0u);
}

struct GhitStep {
    uint32_t ok;                    // the window holds no bad byte
    uint32_t mismatches;            // the columns in which it differs from the text
    uint32_t pam;                   // ghit_pam
    uint64_t columns;               // bit c: guide column c differs, 5'->3' on the protospacer (window column G - 1 - c on '-')
};

// the window at pos against an entry's text of G letters (the reverse complement's for strand 1: window column c is
// compared with text[c] on both strands)
__host__ __device__ inline GhitStep ghit_finish(const uint8_t* bases, uint64_t n, uint64_t pos, const uint8_t* text, uint32_t G,
                                                uint32_t strand, uint32_t omit, uint32_t sets5, uint32_t a, uint32_t sets3,
                                                uint32_t b) {
    GhitStep r;
    r.ok = 1u;
    r.mismatches = 0u;
    r.columns = 0ull;
    for (uint32_t c = 0; c < G; c++) {
        const uint32_t w = ghit_byte(bases, n, (int64_t)pos + (int64_t)c, omit);
        if (w == '\n') r.ok = 0u;
        if (w != text[c]) {
            r.mismatches++;
            r.columns |= 1ull << (strand ? G - 1u - c : c);
        }
    }
    r.pam = ghit_pam(bases, n, pos, G, strand, omit, sets5, a, sets3, b);
    return r;
}

// co_pass.inc -- part of krisp_hip.hip, and of tests/co_pass_check.cpp: one prefilter test per key and one pass per pair of
// rounds of the coarse probe (k_coarse.inc, DESIGN §10b "One test, one pass") in plain C++ for host and device: no HIP call,
// no LDS, no thread index.  A translation unit without HIP defines __host__ and __device__ empty before it includes this file.
//
// A forward key K of a one-strand genome (co_strand.inc) lies under a candidate's forward entry when K & pmask == P and under
// its reverse entry when K & mask_rc == Q(P).  M = pmask & mask_rc -- the key's bits without window position L and without
// window position R -- is part of both masks, so pat & M == K & M for every entry K lies under, of either reading: ONE hash,
// of K & M, finds the prefilter bits and the table slots of both.  Entries that differ at position R (forward) or L
// (reverse) only share their hash: they are neighbours in the table, and a look-up walks on to the first empty slot.
#include <stdint.h>

#define CO_BM_LOG 17            // bits of the prefilter in front of the table: 2^17, as 4096 words of 32
#define CO_SLOT16_LOG 14        // 16-bit slots of a pass's table (the one-strand form): 2^14 of them in the 32 KB of 2^13 words
#define CO_SLOT16_EMPTY 0xFFFFu // a free slot: never an encoded one, whose entry number stays below 2 * 6144
#define CO_SLOT16_IDX 0x3FFFu

__host__ __device__ inline uint32_t co_hash(uint64_t pre) {
    const uint32_t y = (uint32_t)pre * 0x9E3779B1u;
    return ((uint32_t)(pre >> 32) ^ y) * 0x85EBCA6Bu;
}

__host__ __device__ inline uint64_t co_pass_mask(uint64_t pmask, uint64_t mask_rc) { return pmask & mask_rc; }

// the prefilter is a blocked Bloom filter: both bits of a hash lie in one word (one LDS read per key)
__host__ __device__ inline uint32_t co_bloom_word(uint32_t h) { return h >> (37 - CO_BM_LOG); }
__host__ __device__ inline uint32_t co_bloom_bits(uint32_t h) {
    return (1u << ((h >> (32 - CO_BM_LOG)) & 31u)) | (1u << ((h >> (27 - CO_BM_LOG)) & 31u));
}

// a 16-bit slot: the entry's number within the pass (14 bits) under two tag bits of its hash, which gate the read of the
// entry's pattern; the walk starts at the hash's top bits
__host__ __device__ inline uint32_t co_slot16_home(uint32_t h) { return h >> (32 - CO_SLOT16_LOG); }
__host__ __device__ inline uint32_t co_slot16_tag(uint32_t h) { return (h >> 8) & 3u; }
__host__ __device__ inline uint32_t co_slot16(uint32_t idx, uint32_t tag) { return (tag << 14) | idx; }
__host__ __device__ inline uint32_t co_slot16_idx(uint32_t slot) { return slot & CO_SLOT16_IDX; }
__host__ __device__ inline uint32_t co_slot16_tagof(uint32_t slot) { return slot >> 14; }

__host__ __device__ inline uint32_t co_rounds(uint32_t nc, uint32_t tcap) { return nc / tcap + (nc % tcap ? 1u : 0u); }

// the passes of a digit with nfc forward and nrc reverse entries.  A round is up to tcap entries of ONE reading; one_pass:
// pass p holds forward round p beside reverse round p; else a pass is one round, the forward rounds first
__host__ __device__ inline uint32_t co_pass_count(uint32_t nfc, uint32_t nrc, uint32_t tcap, uint32_t one_pass) {
    const uint32_t rf = co_rounds(nfc, tcap), rr = co_rounds(nrc, tcap);
    return one_pass ? (rf > rr ? rf : rr) : rf + rr;
}

// pass p of the digit whose forward entries are [f0, f1) and whose reverse entries are [f1, r1) of the entry array: entry
// number i < nf of the pass is the forward entry c0f + i, the others are the reverse entries c0r + i - nf
struct CoPass { uint32_t c0f, nf, c0r, nr; };
__host__ __device__ inline CoPass co_pass_decode(uint32_t f0, uint32_t f1, uint32_t r1, uint32_t tcap, uint32_t p, uint32_t one_pass) {
    const uint32_t rf = co_rounds(f1 - f0, tcap), rr = co_rounds(r1 - f1, tcap);
    CoPass P = {f0, 0u, f1, 0u};
    const uint32_t pf = p, pr = one_pass ? p : p - rf;              // (pr: used where p >= rf only)
    if (pf < rf) {
        P.c0f = f0 + pf * tcap;
        P.nf = f1 - P.c0f > tcap ? tcap : f1 - P.c0f;
    }
    if ((one_pass || p >= rf) && pr < rr) {
        P.c0r = f1 + pr * tcap;
        P.nr = r1 - P.c0r > tcap ? tcap : r1 - P.c0r;
    }
    return P;
}

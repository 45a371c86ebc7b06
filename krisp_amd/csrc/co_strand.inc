// co_strand.inc -- part of krisp_hip.hip, and of tests/co_strand_check.cpp: one strand of a coarse genome answers for both
// (k_coarse.inc, DESIGN §10b) in plain C++ for host and device: no HIP call, no LDS, no thread index.  A translation unit
// without HIP defines __host__ and __device__ empty before it includes this file.
//
// A window w of k = L + 1 + R bases (positions from 0) leaves two records: the key of w and the key of rc(w).  A key is
// [left | right | diag]: window positions 0 .. L-1, L+1 .. k-1, then L.  The forward record's prefix is w without position L;
// the reverse record's prefix, read in w's coordinates, is w without position R (rc(w)[L] = comp(w[R])).  With R < L both
// can be asked of the forward key K alone:
//   forward reading   K & pmask   == P           for a candidate prefix P,
//   reverse reading   K & mask_rc == Q(P),       Q(P) = the key of the reverse complement of P's sequence, laid out as a
//                                                window with position R left open; mask_rc = the key's 2k bits without the
//                                                two of position R (which lies in `left`, at key base R).
// The bucket digit of a key uses neither position: the first four window positions other than R (all below L: L >= 5), so
// one bucket serves both readings.
#include <stdint.h>

struct CoStrand {
    int L, R, k;
    uint64_t mL, mR, mD;        // the layout: (w & mL) | ((w << sR) & mR) | ((w >> sD) & mD)
    int sR, sD;
    uint64_t pmask, mask_rc;
    int dhi, dlo;               // the digit: the top 10 - dhi bits of the key's high word in front of position R, shifted up
    uint32_t dlow;              // by dlo, and the low dlo bits of its top 10
};

__host__ __device__ inline uint64_t cs_topbits(int n) { return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ~0ull << (64 - n)); }

// (L, 1, R) at the MSB-aligned layout of the packed path; needs L >= 5, R < L, k <= 32
__host__ __device__ inline CoStrand cs_make(int L, int R) {
    CoStrand S;
    S.L = L; S.R = R; S.k = L + 1 + R;
    S.mL = cs_topbits(2 * L);
    S.mR = cs_topbits(2 * (L + R)) & ~S.mL;
    S.mD = cs_topbits(2 * S.k) & ~cs_topbits(2 * (L + R));
    S.sR = 2;
    S.sD = 2 * R;
    S.pmask = cs_topbits(2 * (L + R));
    S.mask_rc = cs_topbits(2 * S.k) & ~(3ull << (62 - 2 * R));
    const int rc = R < 4 ? R : 4;
    S.dhi = 32 - 2 * rc;
    S.dlo = 8 - 2 * rc;
    S.dlow = (1u << S.dlo) - 1u;
    return S;
}

// the bucket digit of a forward key, and of a candidate prefix read forward: the bases at the first four window positions
// other than R
__host__ __device__ inline uint32_t cs_digit(const CoStrand& S, uint64_t key) {
    const uint32_t hi = (uint32_t)(key >> 32);
    const uint32_t front = S.dhi >= 32 ? 0u : (hi >> S.dhi) << S.dlo;       // (R = 0: no base in front of it)
    return front | ((hi >> 22) & S.dlow);
}
__host__ __device__ inline uint32_t cs_class_fwd(const CoStrand& S, uint64_t prefix) { return cs_digit(S, prefix); }

// reverse complement of all 32 bases of x (base 0 in the top two bits)
__host__ __device__ inline uint64_t cs_revcomp32(uint64_t x) {
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}
// ... of the top `len` bases of x (1 .. 32), MSB aligned again
__host__ __device__ inline uint64_t cs_revcomp(uint64_t x, int len) { return cs_revcomp32(x) << (64 - 2 * len); }

__host__ __device__ inline uint64_t cs_layout(const CoStrand& S, uint64_t w) {
    return (w & S.mL) | ((w << S.sR) & S.mR) | ((w >> S.sD) & S.mD);
}
__host__ __device__ inline uint64_t cs_unlayout(const CoStrand& S, uint64_t key) {
    return (key & S.mL) | ((key & S.mR) >> S.sR) | ((key & S.mD) << S.sD);
}

// the digit of the windows that meet prefix P through their reverse record: P's lowest four bases, complemented, reversed
__host__ __device__ inline uint32_t cs_class_rev(const CoStrand& S, uint64_t prefix) {
    return (uint32_t)(cs_revcomp(prefix, S.L + S.R) >> 56);
}

// Q(P): a forward key K has its reverse record under P iff (K & mask_rc) == Q(P)
__host__ __device__ inline uint64_t cs_pattern_rev(const CoStrand& S, uint64_t prefix) {
    const uint64_t s = cs_revcomp(prefix, S.L + S.R);       // w without position R
    const uint64_t front = cs_topbits(2 * S.R);
    return cs_layout(S, (s & front) | ((s & ~front) >> 2));
}

// the reverse record of the window whose forward key is K: inverse layout, reverse complement, layout.  Its diagnostic
// base is read off the key as off any other: (key >> (62 - 2 (L + R))) & 3
__host__ __device__ inline uint64_t cs_rev_key(const CoStrand& S, uint64_t key) {
    return cs_layout(S, cs_revcomp(cs_unlayout(S, key), S.k));
}

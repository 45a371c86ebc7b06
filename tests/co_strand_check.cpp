// co_strand_check.cpp -- one strand answering for both (krisp_amd/csrc/co_strand.inc) against a character-level reverse
// complement, on the host.  tests/test_co_strand.py builds this file with -fsanitize=address,undefined and runs it; it prints
// one line per geometry and "ok <geometries>" at the end, and exits with 1 at the first difference.
//
// A window is an array of k base codes (A C G T = 0 1 2 3, complement = 3 - code); its key is packed here base by base --
// window positions 0 .. L-1, L+1 .. k-1, then L -- with no use of the file under test.  For every window w, K = key(w),
// K' = key(rc(w)):
//   cs_rev_key(K) == K', and its diagnostic base is comp(w[R]);
//   cs_pattern_rev(K' & pmask) == K & mask_rc;
//   cs_class_fwd(K & pmask) == cs_class_rev(K' & pmask) == cs_digit(K) == the bases at the first four positions other than R;
//   cs_digit does not move when the bits of position R or of position L do.
#define __host__
#define __device__
#include "../krisp_amd/csrc/co_strand.inc"

#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t rng_state;
static uint64_t rnd64() {                    // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define FAIL(...) do { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); std::exit(1); } while (0)

// the key of a window, base by base
static uint64_t key_of(const std::vector<int>& w, int L, int R) {
    const int k = L + 1 + R;
    uint64_t key = 0;
    int j = 0;
    for (int i = 0; i < L; i++, j++) key |= (uint64_t)w[i] << (62 - 2 * j);
    for (int i = L + 1; i < k; i++, j++) key |= (uint64_t)w[i] << (62 - 2 * j);
    return key | (uint64_t)w[L] << (62 - 2 * j);
}

static uint64_t top_bases(int n) { return n >= 32 ? ~0ull : (n <= 0 ? 0ull : ~0ull << (64 - 2 * n)); }

static void one_window(const CoStrand& S, const std::vector<int>& w, std::vector<int>& r) {
    const int L = S.L, R = S.R, k = S.k;
    for (int i = 0; i < k; i++) r[i] = 3 - w[k - 1 - i];
    const uint64_t K = key_of(w, L, R), Kr = key_of(r, L, R);
    const uint64_t pmask = top_bases(L + R);
    const uint64_t got = cs_rev_key(S, K);
    if (got != Kr) FAIL("(%d,1,%d) rev key of %016llx: %016llx, want %016llx", L, R, (unsigned long long)K, (unsigned long long)got, (unsigned long long)Kr);
    const int base = (int)((got >> (62 - 2 * (L + R))) & 3u);
    if (base != r[L] || base != 3 - w[R]) FAIL("(%d,1,%d) rev base of %016llx: %d", L, R, (unsigned long long)K, base);
    const uint64_t mask_rc = top_bases(k) & ~(3ull << (62 - 2 * R));
    if (S.pmask != pmask || S.mask_rc != mask_rc) FAIL("(%d,1,%d) masks", L, R);
    const uint64_t Q = cs_pattern_rev(S, Kr & pmask);
    if (Q != (K & mask_rc)) FAIL("(%d,1,%d) Q of %016llx: %016llx, want %016llx", L, R, (unsigned long long)K, (unsigned long long)Q, (unsigned long long)(K & mask_rc));
    uint32_t want = 0;
    for (int i = 0, n = 0; n < 4; i++)
        if (i != R) { want = (want << 2) | (uint32_t)w[i]; n++; }
    const uint32_t d = cs_digit(S, K);
    if (d != want) FAIL("(%d,1,%d) digit of %016llx: %u, want %u", L, R, (unsigned long long)K, d, want);
    if (cs_class_fwd(S, K & pmask) != d) FAIL("(%d,1,%d) forward class of %016llx", L, R, (unsigned long long)K);
    if (cs_class_rev(S, Kr & pmask) != d) FAIL("(%d,1,%d) reverse class of %016llx", L, R, (unsigned long long)K);
    for (uint64_t f = 1; f <= 3; f++) {
        if (cs_digit(S, K ^ (f << (62 - 2 * R))) != d) FAIL("(%d,1,%d) position R reaches the digit", L, R);
        if (cs_digit(S, K ^ (f << (62 - 2 * (L + R)))) != d) FAIL("(%d,1,%d) position L reaches the digit", L, R);
    }
}

// all 4^k windows (sample = 0), or `sample` seeded random ones
static void geometry(int L, int R, uint64_t sample, int& done) {
    const CoStrand S = cs_make(L, R);
    const int k = L + 1 + R;
    std::vector<int> w(k), r(k);
    const uint64_t n = sample ? sample : 1ull << (2 * k);
    rng_state = 0x5EEDull * 1000003ull + (uint64_t)L * 101ull + (uint64_t)R;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t x = sample ? rnd64() : i;
        for (int j = 0; j < k; j++) { w[j] = (int)(x & 3u); x >>= 2; }
        one_window(S, w, r);
    }
    std::printf("L %d R %d k %d %s: %llu windows\n", L, R, k, sample ? "sampled" : "all", (unsigned long long)n);
    done++;
}

int main() {
    int done = 0;
    // every (L, 1, R) the one-strand form takes (L >= 5, R < L) with k <= 9: R = 0 .. 3, all windows
    for (int R = 0; R <= 3; R++)
        for (int L = 5; L + 1 + R <= 9; L++) geometry(L, R, 0, done);
    // R = 4 and R = 6 need L > R: their smallest k is 10 and 14.  k = 10 in full; k = 14 (2.7e8 windows) sampled
    geometry(5, 4, 0, done);
    geometry(7, 6, 1u << 20, done);
    // the two geometries the device tests run at
    geometry(25, 2, 1u << 18, done);
    geometry(20, 6, 1u << 18, done);
    std::printf("ok %d\n", done);
    return 0;
}

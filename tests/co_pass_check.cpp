// co_pass_check.cpp -- one prefilter test per key and one pass per pair of rounds (krisp_amd/csrc/co_pass.inc), on the host.
// tests/test_co_pass.py builds this file with -fsanitize=address,undefined and runs it; it prints one line per geometry, one
// for the slots, one per (tcap, switch) of the passes and "ok <lines>" at the end, and exits with 1 at the first difference.
//
// A window is an array of k base codes (A C G T = 0 1 2 3, complement = 3 - code); its key is packed here base by base --
// window positions 0 .. L-1, L+1 .. k-1, then L.  For every window w, K = key(w), K' = key(rc(w)), M = co_pass_mask:
//   M is the key's 2k bits without the two of window position L and the two of window position R, built here base by base;
//   the forward entry over w has the pattern P = K & pmask, the reverse entry the pattern Q = cs_pattern_rev(K' & pmask):
//   P & M == Q & M == K & M, so the prefilter word, its bit pair, the home slot and the tag of the key are the entries'
//   (no false negative, and one walk meets both entries).
#define __host__
#define __device__
#include "../krisp_amd/csrc/co_strand.inc"
#include "../krisp_amd/csrc/co_pass.inc"

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

// where window position i lies in the key: its base number, counted from the top
static int key_base(int i, int L, int R) { return i < L ? i : (i == L ? L + R : i - 1); }

static uint64_t key_of(const std::vector<int>& w, int L, int R) {
    uint64_t key = 0;
    for (int i = 0; i < L + 1 + R; i++) key |= (uint64_t)w[i] << (62 - 2 * key_base(i, L, R));
    return key;
}

static void same_place(int L, int R, const char* what, uint32_t hk, uint32_t he) {
    if (co_bloom_word(hk) != co_bloom_word(he) || co_bloom_bits(hk) != co_bloom_bits(he))
        FAIL("(%d,1,%d) the key's prefilter bits are not its %s entry's", L, R, what);
    if (co_slot16_home(hk) != co_slot16_home(he) || co_slot16_tag(hk) != co_slot16_tag(he))
        FAIL("(%d,1,%d) the key's slot or tag is not its %s entry's", L, R, what);
}

static void geometry(int L, int R, uint64_t sample, int& done) {
    const CoStrand S = cs_make(L, R);
    const int k = L + 1 + R;
    uint64_t want_m = 0;
    for (int i = 0; i < k; i++)
        if (i != L && i != R) want_m |= 3ull << (62 - 2 * key_base(i, L, R));
    const uint64_t M = co_pass_mask(S.pmask, S.mask_rc);
    if (M != want_m) FAIL("(%d,1,%d) M = %016llx, want %016llx", L, R, (unsigned long long)M, (unsigned long long)want_m);
    if (M & (3ull << (62 - 2 * key_base(L, L, R)))) FAIL("(%d,1,%d) M holds position L", L, R);
    if (M & (3ull << (62 - 2 * key_base(R, L, R)))) FAIL("(%d,1,%d) M holds position R", L, R);
    std::vector<int> w(k), r(k);
    const uint64_t n = sample ? sample : 1ull << (2 * k);
    rng_state = 0x9A55ull * 1000003ull + (uint64_t)L * 101ull + (uint64_t)R;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t x = sample ? rnd64() : i;
        for (int j = 0; j < k; j++) { w[j] = (int)(x & 3u); x >>= 2; }
        for (int j = 0; j < k; j++) r[j] = 3 - w[k - 1 - j];
        const uint64_t K = key_of(w, L, R), Kr = key_of(r, L, R);
        const uint64_t P = K & S.pmask, Q = cs_pattern_rev(S, Kr & S.pmask);
        if (Q != (K & S.mask_rc)) FAIL("(%d,1,%d) Q of %016llx", L, R, (unsigned long long)K);
        if ((P & M) != (K & M) || (Q & M) != (K & M)) FAIL("(%d,1,%d) pattern & M of %016llx", L, R, (unsigned long long)K);
        const uint32_t hk = co_hash(K & M);
        same_place(L, R, "forward", hk, co_hash(P & M));
        same_place(L, R, "reverse", hk, co_hash(Q & M));
        const uint32_t bits = co_bloom_bits(hk);
        if (__builtin_popcount(bits) < 1 || __builtin_popcount(bits) > 2)
            FAIL("(%d,1,%d) a hash sets one or two bits of its word", L, R);
        if (co_bloom_word(hk) >= (1u << (CO_BM_LOG - 5))) FAIL("(%d,1,%d) prefilter word out of range", L, R);
        if (co_slot16_home(hk) >= (1u << CO_SLOT16_LOG)) FAIL("(%d,1,%d) home slot out of range", L, R);
    }
    std::printf("L %d R %d k %d %s: %llu windows\n", L, R, k, sample ? "sampled" : "all", (unsigned long long)n);
    done++;
}

// every entry number a pass can hold (two rounds of 6144) under every tag: 16 bits, never EMPTY, decoded as encoded
static void slots(int& done) {
    uint32_t n = 0;
    for (uint32_t idx = 0; idx < 2 * 6144; idx++)
        for (uint32_t tag = 0; tag < 4; tag++, n++) {
            const uint32_t s = co_slot16(idx, tag);
            if (s > 0xFFFFu || s == CO_SLOT16_EMPTY) FAIL("slot of entry %u tag %u: %x", idx, tag, s);
            if (co_slot16_idx(s) != idx || co_slot16_tagof(s) != tag) FAIL("slot of entry %u tag %u decodes as %u, %u", idx, tag,
                                                                           co_slot16_idx(s), co_slot16_tagof(s));
        }
    // the corners: the largest entry number under the tag of all ones, and the pattern of a free slot
    if (co_slot16(2 * 6144 - 1, 3) != 0xEFFFu) FAIL("corner slot");
    if (co_slot16_idx(CO_SLOT16_EMPTY) < 2 * 6144) FAIL("EMPTY decodes as an entry number a pass can hold");
    for (uint32_t h = 0; h < 1024; h++)
        if (co_slot16_tag(h << 8) != (h & 3u)) FAIL("tag bits");
    if ((1u << CO_SLOT16_LOG) * 2u != 8192u * 4u) FAIL("the 16-bit slots do not fill the table's 32 KB");
    std::printf("slots: %u round trips\n", n);
    done++;
}

// seeded class sizes: every entry of the digit in exactly one pass, at most tcap of each reading per pass, the pass count
static void passes(uint32_t tcap, uint32_t one_pass, int& done) {
    rng_state = 0xC1A55ull + tcap * 7ull + one_pass;
    uint64_t digits = 0, npass = 0;
    for (int rep = 0; rep < 400; rep++) {
        const uint32_t span = tcap == 6144 ? 20000u : 12u * tcap + 3u;
        uint32_t nfc = (uint32_t)(rnd64() % span), nrc = (uint32_t)(rnd64() % span);
        // (the edges: a class without entries, a class of whole rounds, equal and unequal round counts)
        if (rep % 7 == 0) nfc = 0;
        if (rep % 11 == 0) nrc = 0;
        if (rep % 13 == 0) nfc = 3 * tcap;
        if (rep % 17 == 0) nrc = tcap;
        const uint32_t f0 = (uint32_t)(rnd64() % 100000u), f1 = f0 + nfc, r1 = f1 + nrc;
        const uint32_t rf = co_rounds(nfc, tcap), rr = co_rounds(nrc, tcap);
        const uint32_t np = co_pass_count(nfc, nrc, tcap, one_pass);
        if (np != (one_pass ? (rf > rr ? rf : rr) : rf + rr)) FAIL("tcap %u switch %u: %u passes for %u + %u rounds", tcap, one_pass, np, rf, rr);
        if (rf != (nfc + tcap - 1) / tcap || rr != (nrc + tcap - 1) / tcap) FAIL("tcap %u: rounds", tcap);
        std::vector<uint8_t> seen(nfc + nrc, 0);
        for (uint32_t p = 0; p < np; p++) {
            const CoPass P = co_pass_decode(f0, f1, r1, tcap, p, one_pass);
            if (P.nf > tcap || P.nr > tcap) FAIL("tcap %u switch %u: pass %u holds %u + %u", tcap, one_pass, p, P.nf, P.nr);
            if (P.nf + P.nr == 0) FAIL("tcap %u switch %u: pass %u is empty", tcap, one_pass, p);
            if (!one_pass && P.nf != 0 && P.nr != 0) FAIL("tcap %u switch 0: pass %u holds both readings", tcap, p);
            if (!one_pass && (P.nf != 0) != (p < rf)) FAIL("tcap %u switch 0: pass %u is not in today's order", tcap, p);
            if (P.nf && (P.c0f < f0 || P.c0f + P.nf > f1)) FAIL("tcap %u: forward entries outside their class", tcap);
            if (P.nr && (P.c0r < f1 || P.c0r + P.nr > r1)) FAIL("tcap %u: reverse entries outside their class", tcap);
            for (uint32_t i = 0; i < P.nf; i++) seen[P.c0f + i - f0]++;
            for (uint32_t i = 0; i < P.nr; i++) seen[P.c0r + i - f0]++;
        }
        for (size_t i = 0; i < seen.size(); i++)
            if (seen[i] != 1) FAIL("tcap %u switch %u: entry %zu of %u + %u lies in %d passes", tcap, one_pass, i, nfc, nrc, (int)seen[i]);
        digits++;
        npass += np;
    }
    std::printf("passes tcap %u switch %u: %llu digits, %llu passes\n", tcap, one_pass, (unsigned long long)digits, (unsigned long long)npass);
    done++;
}

int main() {
    int done = 0;
    // every (L, 1, R) the one-strand form takes (L >= 5, R < L) with k <= 9, all windows
    for (int R = 0; R <= 3; R++)
        for (int L = 5; L + 1 + R <= 9; L++) geometry(L, R, 0, done);
    // the two geometries the device tests run at
    geometry(25, 2, 1u << 18, done);
    geometry(20, 6, 1u << 18, done);
    slots(done);
    const uint32_t tcaps[4] = {1, 10, 50, 6144};
    for (uint32_t tcap : tcaps)
        for (uint32_t one_pass = 0; one_pass < 2; one_pass++) passes(tcap, one_pass, done);
    std::printf("ok %d\n", done);
    return 0;
}

// join2_screen_check.cpp -- krisp_amd/csrc/j2_screen.inc (the screen of k_join2) on the host, a stand-alone program:
//   * the live rule is necessary for a candidate: for all SA, SB, extraA, extraB in 0..15 with SA != 0, SB != 0 and
//     SA & SB == 0, live(SA | extraA, SB | extraB) holds (65 536 combinations), and bits added never turn a live slot dead;
//   * the slot and the table hash stay inside the screen and the table for random and extreme keys at every (p0, sh, mlog)
//     the item plan can produce with 32-bit heads;
//   * the slot depends on nothing below the prefix's lowest bit, and on nothing above the item's bits;
//   * the bit a key sets lands in its slot's byte, in its side's nibble.
// Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define __host__
#define __device__
#include "../krisp_amd/csrc/j2_screen.inc"

static uint64_t rnd(uint64_t& s) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return s;
}

#define CHECK(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

int main(int argc, char** argv) {
    // with arguments: the slot and the table hash of each item key (hexadecimal), for the numpy restatement
    for (int i = 1; i < argc; i++) {
        const uint64_t ik = std::strtoull(argv[i], nullptr, 16);
        std::printf("%u %u\n", j2_slot(ik), j2_tab_hash(ik));
    }
    if (argc > 1) return 0;
    long checks = 0;
    for (uint32_t sa = 0; sa < 16; sa++)
        for (uint32_t sb = 0; sb < 16; sb++)
            for (uint32_t xa = 0; xa < 16; xa++)
                for (uint32_t xb = 0; xb < 16; xb++) {
                    const bool cand = sa != 0 && sb != 0 && (sa & sb) == 0;
                    if (cand) CHECK(j2_live(sa | xa, sb | xb), "live rule: SA %u SB %u extra %u %u", sa, sb, xa, xb);
                    if (j2_live(sa, sb)) CHECK(j2_live(sa | xa, sb | xb), "a live slot turned dead: %u %u + %u %u", sa, sb, xa, xb);
                    CHECK(j2_live_byte((sa | xa) | (sb | xb) << 4) == j2_live(sa | xa, sb | xb), "byte form");
                    checks++;
                }
    // what a per-key rule would get wrong: SA = {a, c}, SB = {c} is no candidate, and its slot is live all the same
    CHECK(j2_live(0x3, 0x2), "overlap trap");
    CHECK(!j2_live(0x1, 0x1) && !j2_live(0x0, 0xF) && !j2_live(0xF, 0x0), "dead slots");

    uint64_t seed = 0x9E3779B97F4A7C15ull;
    // item plan with 32-bit heads: p0 = 64 - 2 LRrel in [2, 32) (a diagnostic base below it), sh = rb + mlog - 12 in
    // [32, p0 + 32], rb = 64 - b, b in 8 .. 18, mlog in 0 .. b
    for (int p0 = 2; p0 < 32; p0 += 2)
        for (int b = 8; b <= 18; b++)
            for (int mlog = 0; mlog <= b; mlog++) {
                const int sh = 64 - b + mlog - 12;
                if (sh < 32 || sh > p0 + 32) continue;
                const int w = sh + 12 - p0;
                CHECK(w >= 1 && w <= 44, "item key of %d bits", w);
                for (int i = 0; i < 2000; i++) {
                    uint64_t key = rnd(seed);
                    if (i == 0) key = 0;
                    if (i == 1) key = ~0ull;
                    if (i == 2) key = 1ull << p0;
                    if (i == 3) key = (1ull << p0) - 1;
                    if (i == 4) key = 1ull << (p0 + w - 1);
                    const uint64_t ik = j2_item_key(key, p0, w);
                    CHECK(ik < (1ull << w), "item key outside its bits");
                    const uint32_t slot = j2_slot(ik), h = j2_tab_hash(ik);
                    CHECK(slot < J2_SCREEN && h < J2_TAB, "slot %u hash %u outside", slot, h);
                    // nothing below the prefix's lowest bit, nothing above the item's bits
                    const uint64_t low = rnd(seed) & ((1ull << p0) - 1), high = p0 + w < 64 ? rnd(seed) << (p0 + w) : 0;
                    const uint64_t other = (key & ~((1ull << p0) - 1) & (p0 + w < 64 ? (1ull << (p0 + w)) - 1 : ~0ull)) | low | high;
                    CHECK(j2_slot(j2_item_key(other, p0, w)) == slot && j2_tab_hash(j2_item_key(other, p0, w)) == h,
                          "slot depends on bits outside the item key: p0 %d w %d", p0, w);
                    for (uint32_t base = 0; base < 4; base++)
                        for (int side = 0; side < 2; side++) {
                            const uint32_t word = j2_bit(slot, base, side != 0);
                            CHECK(j2_byte(word, slot) == (1u << (base + 4 * side)), "bit outside its nibble");
                            for (uint32_t o = 0; o < 4; o++)
                                if (o != (slot & 3)) CHECK(j2_byte(word, o) == 0, "bit in a neighbour's byte");
                        }
                    checks++;
                }
            }
    // the slots spread: 4096 consecutive item keys do not crowd a few slots (a bound far from the expected 0.25 per slot)
    {
        static uint16_t cnt[J2_SCREEN];
        for (uint64_t ik = 0; ik < 4096; ik++) cnt[j2_slot((ik << 20) | (rnd(seed) & 0xFFFFF))]++;
        uint32_t mx = 0;
        for (uint32_t i = 0; i < J2_SCREEN; i++) mx = cnt[i] > mx ? cnt[i] : mx;
        CHECK(mx <= 8, "slots crowd: %u keys in one", mx);
        checks++;
    }
    std::printf("ok %ld\n", checks);
    return 0;
}

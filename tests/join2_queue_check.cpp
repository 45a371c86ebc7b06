// join2_queue_check.cpp -- krisp_amd/csrc/j2_queue.inc (the per-wave queue of live keys of k_join2<true>) on the host, a
// stand-alone program.  A wave is modelled as 64 lanes over an array of J2Q_CAP entries and held to a plain loop:
//   * ballots of 0, 1, 63 and 64 lanes, every single-lane ballot and seeded random ballots, each from the starting fills 0, 1,
//     63, 64 and 127 (64 and 127 only through the drain in front of the append, as the kernel has it): the places of the live
//     lanes are distinct and dense from the fill on, in lane order; the fill never exceeds J2Q_CAP; a drain takes J2Q_DRAIN
//     entries nobody took before and leaves fill - J2Q_DRAIN;
//   * long seeded runs of appends and drains: every entry written is taken exactly once, the rest by the drain at the end;
//   * an entry gives back the item key and the diagnostic base of its key, for item keys of 1 to 44 bits, all four bases, the
//     lowest and highest p0 of the route, and whatever stands above the item key and below the base;
//   * the live rule as one comparison (j2_screen.inc: j2_live_byte_min) is the rule, for all 256 bytes.
// Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __host__
#define __device__
#include "../krisp_amd/csrc/j2_screen.inc"
#include "../krisp_amd/csrc/j2_queue.inc"

static uint64_t rnd(uint64_t& s) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return s;
}

#define CHECK(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

struct Wave {
    std::vector<uint64_t> q;        // the queue: entry = ticket + 1, 0 = never written
    uint32_t fill = 0;
    uint64_t written = 0;           // tickets handed out
    std::vector<int> taken;         // per ticket: times a drain took it
    Wave() : q(J2Q_CAP, 0) {}
};

// one key slot: the ballot's live lanes append, as the kernel does; returns 0 or says what failed
static int append(Wave& w, uint64_t ballot) {
    CHECK(!j2q_drains(w.fill), "append at fill %u: the drain was due", w.fill);
    // the plain loop: lane by lane, the next free place
    uint32_t next = w.fill;
    bool used[J2Q_CAP] = {false};
    for (uint32_t lane = 0; lane < 64; lane++) {
        if (!((ballot >> lane) & 1)) continue;
        const uint32_t place = j2q_place(w.fill, j2q_below(ballot, lane));
        CHECK(place == next, "lane %u of ballot %016llx at fill %u: place %u, the loop says %u", lane, (unsigned long long)ballot, w.fill, place, next);
        CHECK(place < J2Q_CAP, "place %u outside the queue", place);
        CHECK(!used[place], "place %u twice", place);
        used[place] = true;
        w.q[place] = ++w.written;
        w.taken.push_back(0);
        next++;
    }
    const uint32_t after = j2q_fill_after(w.fill, ballot);
    CHECK(after == next, "fill after ballot %016llx: %u, the loop says %u", (unsigned long long)ballot, after, next);
    CHECK(after <= J2Q_CAP, "fill %u exceeds the queue", after);
    w.fill = after;
    return 0;
}

// a join of n entries: lane l takes entry j2q_first(fill, n) + l
static int drain(Wave& w, uint32_t n) {
    CHECK(n >= 1 && n <= J2Q_DRAIN && n <= w.fill, "a drain of %u at fill %u", n, w.fill);
    const uint32_t first = j2q_first(w.fill, n);
    for (uint32_t lane = 0; lane < n; lane++) {
        CHECK(first + lane < w.fill, "lane %u reads past the fill", lane);
        const uint64_t t = w.q[first + lane];
        CHECK(t != 0, "entry %u never written", first + lane);
        CHECK(w.taken[t - 1] == 0, "ticket %llu taken twice", (unsigned long long)t);
        w.taken[t - 1]++;
        w.q[first + lane] = 0;
    }
    const uint32_t before = w.fill;
    w.fill = first;
    CHECK(w.fill == before - n, "a drain of %u leaves %u of %u", n, w.fill, before);
    return 0;
}

// what the kernel does with one key slot, and with the end of a visit
static int slot(Wave& w, uint64_t ballot) {
    if (append(w, ballot)) return 1;
    if (j2q_drains(w.fill)) {
        const uint32_t before = w.fill;
        if (drain(w, J2Q_DRAIN)) return 1;
        CHECK(w.fill == before - 64, "a drain leaves fill - 64");
    }
    CHECK(!j2q_drains(w.fill), "fill %u behind a slot", w.fill);
    return 0;
}
static int finish(Wave& w) {
    if (w.fill && drain(w, w.fill)) return 1;
    CHECK(w.fill == 0, "the end of a visit leaves %u", w.fill);
    for (size_t t = 0; t < w.taken.size(); t++) CHECK(w.taken[t] == 1, "ticket %zu taken %d times", t + 1, w.taken[t]);
    return 0;
}

// a wave whose queue holds `fill` entries (64 and 127: as the append of a full ballot leaves it, in front of its drain)
static int wave_at(Wave& w, uint32_t fill) {
    const uint32_t base = fill >= 64 ? fill - 64 : fill;
    if (base && append(w, base == 64 ? ~0ull : (1ull << base) - 1)) return 1;
    if (fill >= 64 && append(w, ~0ull)) return 1;
    CHECK(w.fill == fill, "starting fill %u, got %u", fill, w.fill);
    return 0;
}

int main() {
    long checks = 0;
    uint64_t seed = 0xD1B54A32D192ED03ull;
    std::vector<uint64_t> ballots = {0ull, 1ull, 1ull << 63, ~0ull, ~0ull >> 1, ~0ull << 1, ~(1ull << 31)};
    for (int l = 0; l < 64; l++) ballots.push_back(1ull << l);
    for (int i = 0; i < 400; i++) {
        uint64_t b = rnd(seed);
        if (i % 4 == 1) b &= rnd(seed) & rnd(seed);         // (about one lane in eight: the kernel's usual ballot)
        if (i % 4 == 2) b |= rnd(seed) | rnd(seed);
        ballots.push_back(b);
    }
    const uint32_t fills[] = {0, 1, 63, 64, 127};
    for (const uint32_t f : fills)
        for (const uint64_t b : ballots) {
            Wave w;
            if (wave_at(w, f)) return 1;
            if (j2q_drains(w.fill)) {
                if (drain(w, J2Q_DRAIN)) return 1;
                CHECK(w.fill == f - 64, "a drain leaves fill - 64");
            }
            if (slot(w, b) || finish(w)) return 1;
            checks++;
        }
    // long runs: visits of four slots, dense and sparse, each ended as the kernel ends it
    for (int run = 0; run < 200; run++) {
        Wave w;
        const int visits = 1 + (int)(rnd(seed) % 6);
        for (int v = 0; v < visits; v++) {
            for (int e = 0; e < 4; e++) {
                uint64_t b = rnd(seed);
                if (run % 3 == 0) b &= rnd(seed) & rnd(seed);
                if (run % 3 == 1) b |= rnd(seed);
                if (slot(w, b)) return 1;
            }
            if (finish(w)) return 1;
        }
        checks++;
    }
    // entries: the key = (item number) | item key << p0 | base << (p0 - 2) | the rest of the window
    const int p0s[] = {2, 10, 12, 20, 31};
    for (int bits = 1; bits <= J2Q_KEY_BITS; bits++)
        for (uint32_t base = 0; base < 4; base++)
            for (const int p0 : p0s) {
                if (p0 + bits > 64) continue;
                const uint64_t top = 1ull << (bits - 1), all = (top << 1) - 1;
                uint64_t iks[6] = {top, all, top | 1, top | (rnd(seed) & all), top | (rnd(seed) & all), top | (all >> 1)};
                for (const uint64_t ik : iks) {
                    const uint64_t above = p0 + bits < 64 ? rnd(seed) << (p0 + bits) : 0;
                    const uint64_t below = p0 > 2 ? rnd(seed) & ((1ull << (p0 - 2)) - 1) : 0;
                    const uint64_t key = above | ik << p0 | (uint64_t)base << (p0 - 2) | below;
                    const uint64_t en = j2q_entry((uint32_t)key, (uint32_t)(key >> 32), p0);
                    CHECK(j2q_key(en, bits) == ik && j2q_base(en) == base, "entry of key %llx base %u p0 %d: %llx", (unsigned long long)ik, base,
                          p0, (unsigned long long)en);
                    CHECK(j2q_key(en, bits) == j2_item_key(key, p0, bits), "entry and j2_item_key");
                    checks++;
                }
            }
    for (uint32_t b = 0; b < 256; b++) {
        CHECK(j2_live_byte_min(b) == j2_live_byte(b), "live rule of byte %u", b);
        checks++;
    }
    CHECK(J2Q_CAP == 2 * J2Q_DRAIN && J2Q_DRAIN == 64, "a drain is one wave, the queue two");
    std::printf("ok %ld\n", checks);
    return 0;
}

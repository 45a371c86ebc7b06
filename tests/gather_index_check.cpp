// gather_index_check.cpp -- the output -> (item, offset) arithmetic of k_gather_items (krisp_amd/csrc/gi_index.inc) on the
// host.  tests/test_gather_index.py builds this file with -fsanitize=address,undefined and runs it; it prints one line per
// count vector and "ok <vectors>" at the end, and exits with 1 at the first difference.
//
// A vector: the survivor counts of the GI_ITEMS items of one workgroup.  Its prefix sums are built as the kernel builds them
// (pre[0] = 0, pre[j + 1] = pre[j] + count[j]); every output o < pre[GI_ITEMS] is mapped with gi_slot.  Walking o upwards,
// the (item, offset) pairs must be exactly the enumeration "item by item, entry by entry": every entry once, in order,
// no entry of an empty item, none outside an item.
#define __host__
#define __device__
#include "../krisp_amd/csrc/gi_index.inc"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

static uint64_t rng_state;
static uint32_t rnd() {                      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

#define FAIL(...) do { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); std::exit(1); } while (0)

static int vectors = 0;

static void check(const char* kind, uint64_t seed, const std::vector<uint32_t>& count) {
    // exact-size heap arrays: an index one past an end is a report
    std::vector<uint32_t> pre(GI_ITEMS + 1);
    pre[0] = 0;
    for (uint32_t j = 0; j < GI_ITEMS; j++) pre[j + 1] = pre[j] + count[j];
    const uint32_t total = pre[GI_ITEMS];
    uint32_t item = 0, offset = 0, nonempty = 0;
    for (uint32_t j = 0; j < GI_ITEMS; j++) nonempty += count[j] != 0;
    for (uint32_t o = 0; o < total; o++) {
        while (offset == count[item]) { item++; offset = 0; }          // (the enumeration skips empty items)
        const GiSlot s = gi_slot(pre.data(), o);
        if (s.item != item || s.offset != offset)
            FAIL("%s seed %llu: output %u is (%u, %u), expected (%u, %u)", kind, (unsigned long long)seed, o, s.item, s.offset, item, offset);
        offset++;
    }
    if (total) {
        while (item < GI_ITEMS && offset == count[item]) { item++; offset = 0; }
        if (item != GI_ITEMS) FAIL("%s seed %llu: the outputs end inside item %u", kind, (unsigned long long)seed, item);
    }
    std::printf("%s seed %llu: %u outputs in %u items\n", kind, (unsigned long long)seed, total, nonempty);
    vectors++;
}

int main() {
    for (uint64_t seed = 0; seed < 4; seed++) {
        rng_state = seed * 1000003ull + 17;
        std::vector<uint32_t> c(GI_ITEMS);
        // nothing at all
        std::fill(c.begin(), c.end(), 0u);
        check("zero", seed, c);
        // one full item, anywhere (the first and the last among the seeds), the rest empty
        std::fill(c.begin(), c.end(), 0u);
        c[seed == 0 ? 0 : seed == 1 ? GI_ITEMS - 1 : rnd() % GI_ITEMS] = 1 + rnd() % 700;
        check("one", seed, c);
        // sparse: one item in eight holds one or two entries
        for (uint32_t j = 0; j < GI_ITEMS; j++) c[j] = (rnd() % 8u) ? 0u : 1u + rnd() % 2u;
        check("sparse", seed, c);
        // dense: about 24 entries per item, a few empty
        for (uint32_t j = 0; j < GI_ITEMS; j++) c[j] = (rnd() % 16u) ? 8u + rnd() % 33u : 0u;
        check("dense", seed, c);
        // every item holds exactly one entry
        std::fill(c.begin(), c.end(), 1u);
        check("ones", seed, c);
        // the counts the device cases plant: 0, 1, 63, 64, 65 and several hundred
        const uint32_t edge[6] = {0u, 1u, 63u, 64u, 65u, 300u + rnd() % 400u};
        for (uint32_t j = 0; j < GI_ITEMS; j++) c[j] = edge[rnd() % 6u];
        c[0] = edge[1 + seed % 5];
        c[GI_ITEMS - 1] = edge[1 + (seed + 2) % 5];
        check("edge", seed, c);
        // totals above 2^16: items of up to 4 T = 2048 survivors
        for (uint32_t j = 0; j < GI_ITEMS; j++) c[j] = (rnd() % 8u) ? 1024u + rnd() % 1025u : 0u;
        c[rnd() % GI_ITEMS] = 2048u;
        uint64_t sum = 0;
        for (uint32_t j = 0; j < GI_ITEMS; j++) sum += c[j];
        if (sum <= 65536) FAIL("large seed %llu: a total of %llu does not pass 2^16", (unsigned long long)seed, (unsigned long long)sum);
        check("large", seed, c);
    }
    std::printf("ok %d\n", vectors);
    return 0;
}

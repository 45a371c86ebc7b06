// coarse_units_check.cpp -- the work-unit arithmetic of the coarse route (krisp_amd/csrc/co_units.inc) against a brute-force
// enumeration, on the host.  tests/test_coarse_units.py builds this file with -fsanitize=address,undefined and runs it; it
// prints one line per table and "ok <tables>" at the end, and exits with 1 at the first difference.
//
// A table: G genomes, per (genome, top byte) a bucket whose length is drawn from {0, 1, CO_CHUNK - 1, CO_CHUNK, CO_CHUNK + 1,
// 3 CO_CHUNK + 7}, per top byte a candidate count from {0, 1, tcap, tcap + 1}.  ust[] is built as k_coarse_tables builds
// it (co_byte_units over the byte's row), every unit number is decoded as k_coarse_probe decodes it (co_unit_byte, then
// co_unit_decode on the byte's row).
#define __host__
#define __device__
#include "../krisp_amd/csrc/co_units.inc"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define MAXG 5

static uint64_t rng_state;
static uint32_t rnd() {                      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

#define FAIL(...) do { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); std::exit(1); } while (0)

struct Unit { uint32_t t, r, g, ch, k0, k1; };
static uint32_t used_len[6], used_nc[4];      // how often each length met a byte with candidates, each count a populated byte

static void one_table(uint32_t G, uint32_t tcap, uint64_t seed) {
    rng_state = seed * 1000003ull + G * 101ull + tcap;
    const uint32_t lens[6] = {0u, 1u, CO_CHUNK - 1u, CO_CHUNK, CO_CHUNK + 1u, 3u * CO_CHUNK + 7u};
    const uint32_t ncs[4] = {0u, 1u, tcap, tcap + 1u};
    // exact-size heap arrays: an index one past an end is a report
    std::vector<std::vector<uint32_t>> off(G, std::vector<uint32_t>(257));
    std::vector<uint32_t> nc(256);
    for (uint32_t t = 0; t < 256; t++) nc[t] = (rnd() % 3u) ? ncs[rnd() % 4u] : 0u;
    for (uint32_t j = 0; j < G; j++) {
        off[j][0] = rnd() % 5u;                                     // an odd or an even base
        for (uint32_t t = 0; t < 256; t++) {
            // one top byte in eight is populated (the first and the last always); the others are empty buckets
            const bool on = t == 0 || t == 255 || rnd() % 8u == 0;
            const uint32_t li = on ? rnd() % 6u : 0u;
            off[j][t + 1] = off[j][t] + lens[li];
            if (nc[t]) used_len[li]++;
            if (li) for (uint32_t i = 0; i < 4; i++) if (nc[t] == ncs[i]) used_nc[i]++;
        }
    }
    // the rows and ust[], as k_coarse_tables writes them
    std::vector<std::vector<uint32_t>> rows(256, std::vector<uint32_t>(2 * G));
    std::vector<uint32_t> ust(257);
    uint32_t total = 0;
    for (uint32_t t = 0; t < 256; t++) {
        for (uint32_t j = 0; j < G; j++) { rows[t][2 * j] = off[j][t]; rows[t][2 * j + 1] = off[j][t + 1]; }
        ust[t] = total;
        total += co_byte_units(nc[t], tcap, rows[t].data(), G);
    }
    ust[256] = total;
    // brute force: top byte -> round -> genome -> chunk
    std::vector<Unit> want;
    for (uint32_t t = 0; t < 256; t++) {
        uint32_t rounds = 0;
        for (uint32_t c = 0; c < nc[t]; c += tcap) rounds++;
        for (uint32_t r = 0; r < rounds; r++)
            for (uint32_t j = 0; j < G; j++) {
                uint32_t ch = 0;
                for (uint32_t k = off[j][t]; k < off[j][t + 1]; k += CO_CHUNK, ch++) {
                    const uint32_t e = off[j][t + 1] - k > CO_CHUNK ? k + CO_CHUNK : off[j][t + 1];
                    want.push_back(Unit{t, r, j, ch, k, e});
                }
            }
    }
    if (want.size() != total) FAIL("G %u tcap %u seed %llu: %u units, brute force %zu", G, tcap, (unsigned long long)seed, total, want.size());
    // every (round, genome, key) of a byte with candidates exactly once: counted per key
    std::vector<std::vector<std::vector<uint8_t>>> seen(2);
    for (uint32_t r = 0; r < 2; r++) {
        seen[r].resize(G);
        for (uint32_t j = 0; j < G; j++) seen[r][j].assign(off[j][256] - off[j][0], 0);
    }
    std::vector<Unit> got(total);
    for (uint32_t u = 0; u < total; u++) {
        const uint32_t t = co_unit_byte(ust.data(), u);
        if (t > 255 || ust[t] > u || ust[t + 1] <= u) FAIL("unit %u: top byte %u", u, t);
        if (nc[t] == 0) FAIL("unit %u lies in top byte %u, which has no candidate", u, t);
        const CoUnit un = co_unit_decode(u - ust[t], rows[t].data(), G);
        got[u] = Unit{t, un.round, un.genome, un.chunk, un.k0, un.k1};
        const Unit& w = want[u];
        if (t != w.t || un.round != w.r || un.genome != w.g || un.chunk != w.ch || un.k0 != w.k0 || un.k1 != w.k1)
            FAIL("unit %u: (%u %u %u %u [%u %u)), brute force (%u %u %u %u [%u %u))", u, t, un.round, un.genome, un.chunk, un.k0,
                 un.k1, w.t, w.r, w.g, w.ch, w.k0, w.k1);
        if (un.genome >= G || un.round >= 2) FAIL("unit %u: genome %u round %u", u, un.genome, un.round);
        if (un.k0 >= un.k1 || un.k1 - un.k0 > CO_CHUNK || un.k0 < off[un.genome][t] || un.k1 > off[un.genome][t + 1])
            FAIL("unit %u: keys [%u, %u) outside bucket [%u, %u)", u, un.k0, un.k1, off[un.genome][t], off[un.genome][t + 1]);
        std::vector<uint8_t>& s = seen[un.round][un.genome];
        for (uint32_t k = un.k0; k < un.k1; k++) {
            if (s[k - off[un.genome][0]]) FAIL("unit %u: key %u of genome %u twice in round %u", u, k, un.genome, un.round);
            s[k - off[un.genome][0]] = 1;
        }
    }
    for (uint32_t t = 0; t < 256; t++) {
        uint32_t rounds = 0;
        for (uint32_t c = 0; c < nc[t]; c += tcap) rounds++;
        for (uint32_t r = 0; r < 2; r++)
            for (uint32_t j = 0; j < G; j++)
                for (uint32_t k = off[j][t]; k < off[j][t + 1]; k++)
                    if (seen[r][j][k - off[j][0]] != (r < rounds ? 1 : 0))
                        FAIL("top byte %u round %u genome %u key %u: covered %u times, %u rounds", t, r, j, k,
                             seen[r][j][k - off[j][0]], rounds);
    }
    // a contiguous slice changes (top byte, round) monotonically: a workgroup never goes back to a table
    const uint32_t splits[3] = {1, 3, 7};
    for (uint32_t W : splits)
        for (uint32_t w = 0; w < W; w++) {
            const uint32_t u0 = (uint32_t)(((uint64_t)w * total) / W), u1 = (uint32_t)(((uint64_t)(w + 1) * total) / W);
            for (uint32_t u = u0 + 1; u < u1; u++) {
                const Unit &a = got[u - 1], &b = got[u];
                if (b.t < a.t || (b.t == a.t && b.r < a.r)) FAIL("split %u/%u: unit %u goes back to table (%u, %u)", w, W, u, b.t, b.r);
            }
        }
    std::printf("G %u tcap %u seed %llu: %u units\n", G, tcap, (unsigned long long)seed, total);
}

int main() {
    uint32_t tables = 0;
    const uint32_t tcaps[2] = {1, 50};
    for (uint32_t G = 1; G <= MAXG; G++)
        for (uint32_t tcap : tcaps)
            for (uint64_t seed = 0; seed < 2; seed++) {
                one_table(G, tcap, seed);
                tables++;
            }
    for (uint32_t i = 0; i < 6; i++) if (!used_len[i]) FAIL("bucket length %u of the list never met candidates", i);
    for (uint32_t i = 0; i < 4; i++) if (!used_nc[i]) FAIL("candidate count %u of the list never met keys", i);
    std::printf("ok %u\n", tables);
    return 0;
}

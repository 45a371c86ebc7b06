// gbulge_step_check.cpp -- a stand-alone program around krisp_amd/csrc/gbulge_step.inc, the per-pair step of the bulged
// guide-hit scan, for tests/test_guide_bulges_step.py: built with -fsanitize=address,undefined and run on its own (never
// loaded into Python).
//
// Input (argv[1]), any number of cases one after the other:
//   a line "G omit nguides n M B need pam5 pam3" (a motif in IUPAC letters, "-" for none), then nguides * G bytes of guides
//   and n bytes of text, raw, then a '\n'.
// The text goes into a heap buffer of exactly n bytes, so that a read at -1 or n is reported.  The program plays the scan:
// EVERY position 0 .. n - h, every entry (2 i = guide i, 2 i + 1 = its reverse complement) and either half of h = (G - B) / 2
// letters is a seed pair when the h staged bytes there hold no bad byte and differ from the half in at most M columns;
// every pair goes through the step with each of the 2 B bulges, and a row the pair owns is printed:
// "pos strand guide bulge mismatches columns pam bulge_column length".  A case ends with a line "end <case number>".
#define __host__
#define __device__
#include "../krisp_amd/csrc/ghit_step.inc"
#include "../krisp_amd/csrc/gbulge_step.inc"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint32_t motif_sets(const char* motif, uint32_t* len) {
    static const char letters[] = "ACGTURYSWKMBDHVN";
    static const uint32_t set_of[] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    uint32_t sets = 0;
    *len = 0;
    if (!strcmp(motif, "-")) return 0;
    for (size_t j = 0; motif[j]; j++) {
        const char* at = strchr(letters, motif[j]);
        if (!at || j >= 8) {
            fprintf(stderr, "bad motif %s\n", motif);
            exit(2);
        }
        sets |= set_of[at - letters] << (4 * j);
        *len = (uint32_t)j + 1;
    }
    return sets;
}

static uint8_t comp(uint8_t b) { return b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A'; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned G, omit, nguides, M, B, need;
    unsigned long long n;
    char pam5[16], pam3[16];
    for (int ncase = 0;; ncase++) {
        const int got = fscanf(f, "%u %u %u %llu %u %u %u %15s %15s", &G, &omit, &nguides, &n, &M, &B, &need, pam5, pam3);
        if (got == EOF) break;
        if (got != 9 || fgetc(f) != '\n' || B < 1 || B > 2 || G < 12 || G > 40) return 2;
        uint32_t a, b;
        const uint32_t sets5 = motif_sets(pam5, &a), sets3 = motif_sets(pam3, &b);
        const uint32_t h = (G - B) / 2;
        // entries: exact heap buffers, one per entry
        std::vector<uint8_t*> entry(2 * (size_t)nguides);
        for (unsigned i = 0; i < nguides; i++) {
            uint8_t* t = new uint8_t[G];
            uint8_t* r = new uint8_t[G];
            if (fread(t, 1, G, f) != G) return 2;
            for (unsigned c = 0; c < G; c++) r[c] = comp(t[G - 1 - c]);
            entry[2 * i] = t;
            entry[2 * i + 1] = r;
        }
        uint8_t* text = new uint8_t[n];                 // exactly n bytes: the sanitizer sees index -1 and index n
        if (n && fread(text, 1, n, f) != n) return 2;
        if (fgetc(f) != '\n') return 2;
        for (unsigned long long pos = 0; pos + h <= n; pos++)
            for (size_t e = 0; e < entry.size(); e++)
                for (uint32_t half = 0; half < 2; half++) {
                    // the scan's part: is the half at pos a seed pair?
                    const uint8_t* ht = entry[e] + (half ? G - h : 0);
                    uint32_t d = 0;
                    bool ok = true;
                    for (uint32_t c = 0; c < h; c++) {
                        const uint32_t w = ghit_byte(text, n, (int64_t)(pos + c), omit);
                        ok = ok && w != '\n';
                        d += w != ht[c];
                    }
                    if (!ok || d > M) continue;
                    for (uint32_t j = 0; j < 2 * B; j++) {
                        int64_t start;
                        uint32_t pam;
                        const GbulgeStep r = gbulge_pair(text, n, pos, half, h, entry[e], G, (uint32_t)(e & 1), gbulge_of(j), M, omit, sets5,
                                                         a, sets3, b, need, &start, &pam);
                        if (r.hit)
                            printf("%lld %u %zu %d %u %llu %u %u %u\n", (long long)start, (unsigned)(e & 1), e >> 1, (int)gbulge_of(j),
                                   r.mismatches, (unsigned long long)r.columns, pam, r.bulge_column, r.length);
                    }
                }
        printf("end %d\n", ncase);
        delete[] text;
        for (uint8_t* p : entry) delete[] p;
    }
    fclose(f);
    return 0;
}

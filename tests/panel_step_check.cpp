// panel_step_check.cpp -- krisp_amd/csrc/panel_step.inc as a stand-alone host program (tests/test_panel_step.py builds it
// with -fsanitize=address,undefined): the window keys, the table's insert and probe, the primer codes, over heap buffers of
// the exact size, so that an index outside a template or the table is a report.
//
//   panel_step_check FILE        FILE holds lines
//     locus MEMBER CANDIDATE             -> "locus V K": V = 1 where the two templates are the same locus, K = the slots in use
//     primer TEMPLATE START N RC         -> "primer" and the primer's N codes, then the codes at N and N + 5 (4: outside)
//     keys TEMPLATE I                    -> "keys OK FWD REV" of the window at I
#define __host__
#define __device__
#include "../krisp_amd/csrc/panel_step.inc"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint8_t* exact(const std::string& s) {
    uint8_t* p = (uint8_t*)malloc(s.size() ? s.size() : 1);
    if (s.size()) memcpy(p, s.data(), s.size());
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<char> line(1 << 16);
    while (fgets(line.data(), (int)line.size(), f)) {
        std::vector<std::string> w;
        for (char* tok = strtok(line.data(), " \n"); tok; tok = strtok(nullptr, " \n")) w.push_back(tok);
        if (w.empty()) continue;
        if (w[0] == "locus" && w.size() == 3) {
            const uint32_t Wm = (uint32_t)w[1].size(), Wc = (uint32_t)w[2].size();
            uint8_t* m = exact(w[1]);
            uint8_t* c = exact(w[2]);
            uint32_t* table = (uint32_t*)malloc(PANEL_SLOTS * sizeof(uint32_t));
            uint32_t* poly_t = (uint32_t*)malloc(sizeof(uint32_t));
            for (uint32_t i = 0; i < PANEL_SLOTS; i++) table[i] = PANEL_EMPTY;
            *poly_t = 0;
            bool ok = true;
            // (the loop runs past the last window on purpose: the step answers "no window" there)
            for (uint32_t i = 0; i < Wm + 2; i++) {
                uint32_t kf, kr;
                if (panel_window_keys(m, Wm, i, &kf, &kr)) ok = ok && panel_insert(table, poly_t, kf) && panel_insert(table, poly_t, kr);
            }
            bool same = false;
            for (uint32_t i = 0; i < Wc + 2; i++) {
                uint32_t kf, kr;
                if (panel_window_keys(c, Wc, i, &kf, &kr) && panel_probe(table, *poly_t, kf)) same = true;
            }
            uint32_t used = *poly_t;
            for (uint32_t i = 0; i < PANEL_SLOTS; i++) used += table[i] != PANEL_EMPTY;
            if (!ok) return 3;
            printf("locus %d %u\n", same ? 1 : 0, used);
            free(m); free(c); free(table); free(poly_t);
        } else if (w[0] == "primer" && w.size() == 5) {
            const uint32_t W = (uint32_t)w[1].size(), start = (uint32_t)atoi(w[2].c_str()), n = (uint32_t)atoi(w[3].c_str());
            const bool rc = atoi(w[4].c_str()) != 0;
            uint8_t* t = exact(w[1]);
            printf("primer ");
            for (uint32_t i = 0; i < n; i++) printf("%u", panel_primer_code(t, W, start, n, i, rc));
            printf(" %u %u\n", panel_primer_code(t, W, start, n, n, rc), panel_primer_code(t, W, start, n, n + 5, rc));
            free(t);
        } else if (w[0] == "keys" && w.size() == 3) {
            const uint32_t W = (uint32_t)w[1].size();
            uint8_t* t = exact(w[1]);
            uint32_t kf = 0, kr = 0;
            const bool ok = panel_window_keys(t, W, (uint32_t)atoi(w[2].c_str()), &kf, &kr);
            printf("keys %d %u %u\n", ok ? 1 : 0, ok ? kf : 0u, ok ? kr : 0u);
            free(t);
        } else {
            return 4;
        }
    }
    fclose(f);
    return 0;
}

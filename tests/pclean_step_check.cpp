// pclean_step_check.cpp -- krisp_amd/csrc/pclean_step.inc as a stand-alone host program (tests/test_pclean_step.py builds it
// with -fsanitize=address,undefined): the forward and backward walks over the site store, the owners' lookups and the fate
// words, over heap buffers of the exact size, so that an index outside the store, the offsets, the owners or the fates is a
// report.
//
//   pclean_step_check FILE       FILE holds whitespace-separated integers:
//     T smin max_product ncand, eoff[0 .. 2 T], ns, ns x (pos entry unit), nown, ooff[0 .. T], own[0 .. nown), ncand x (left
//     row, right row), then commands until the end:
//       1                         -> per site i = 0 .. ns + 1 a line "f i j ..." (the closing sites of i's products) and a
//                                    line "b i j ..." (the opening sites of the products i closes)
//       2                         -> "self w ...": the fate words after every site's pclean_self_site over fates of 0
//       3 m number w[0 .. ncand)  -> "cross w ...": the fate words w after every site's pclean_cross_site for member m
//       4 t                       -> "own c ...": the owners of text t
//       5 c                       -> "fate v": pclean_fate of candidate c over fates of 7
#define __host__
#define __device__
#include "../include/krisp_hip.h"
#include "../krisp_amd/csrc/pclean_step.inc"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool next(FILE* f, unsigned long long* v) { return fscanf(f, "%llu", v) == 1; }

template <typename X>
static X* exact(size_t n) { return (X*)malloc(n ? n * sizeof(X) : 1); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long v, T, smin, mp, ncand, ns, nown;
    if (!next(f, &T) || !next(f, &smin) || !next(f, &mp) || !next(f, &ncand)) return 2;
    uint32_t* eoff = exact<uint32_t>(2 * T + 1);
    for (size_t i = 0; i <= 2 * T; i++) { if (!next(f, &v)) return 2; eoff[i] = (uint32_t)v; }
    if (!next(f, &ns)) return 2;
    kr_product_site* sites = exact<kr_product_site>(ns);
    uint32_t* unit = exact<uint32_t>(ns);
    for (size_t i = 0; i < ns; i++) {
        unsigned long long pos, e, u;
        if (!next(f, &pos) || !next(f, &e) || !next(f, &u)) return 2;
        sites[i].pos = pos; sites[i].entry = (uint32_t)e; sites[i].mismatches = sites[i].end_mismatches = 0; sites[i].pad = 0;
        unit[i] = (uint32_t)u;
    }
    if (!next(f, &nown)) return 2;
    uint32_t* ooff = exact<uint32_t>(T + 1);
    uint32_t* own = exact<uint32_t>(nown);
    for (size_t i = 0; i <= T; i++) { if (!next(f, &v)) return 2; ooff[i] = (uint32_t)v; }
    for (size_t i = 0; i < nown; i++) { if (!next(f, &v)) return 2; own[i] = (uint32_t)v; }
    uint32_t* rows = exact<uint32_t>(2 * ncand);
    for (size_t i = 0; i < 2 * ncand; i++) { if (!next(f, &v)) return 2; rows[i] = (uint32_t)v; }
    uint16_t* state = exact<uint16_t>(ncand);

    PcleanStore S;
    S.sites = sites; S.unit = unit; S.ns = ns; S.eoff = eoff; S.ne = (uint32_t)(2 * T); S.smin = (uint32_t)smin; S.max_product = (uint32_t)mp;
    PcleanOwners O;
    O.ooff = ooff; O.own = own; O.T = (uint32_t)T; O.nown = (uint32_t)nown;
    const uint32_t nc = (uint32_t)ncand;

    unsigned long long cmd;
    while (next(f, &cmd)) {
        if (cmd == 1) {
            // (the loop runs past the last site on purpose: the step answers nothing there)
            for (uint64_t i = 0; i < ns + 2; i++) {
                printf("f %llu", (unsigned long long)i);
                pclean_forward(S, i, [&](uint64_t j, uint32_t) { printf(" %llu", (unsigned long long)j); return true; });
                printf("\nb %llu", (unsigned long long)i);
                pclean_backward(S, i, [&](uint64_t j, uint32_t) { printf(" %llu", (unsigned long long)j); return true; });
                printf("\n");
            }
        } else if (cmd == 2) {
            for (uint32_t c = 0; c < nc; c++) state[c] = 0;
            for (uint64_t i = 0; i < ns + 2; i++) pclean_self_site(S, O, i, state, nc);
            printf("self");
            for (uint32_t c = 0; c < nc; c++) printf(" %u", (unsigned)state[c]);
            printf("\n");
        } else if (cmd == 3) {
            unsigned long long m, number;
            if (!next(f, &m) || !next(f, &number)) return 2;
            for (uint32_t c = 0; c < nc; c++) { if (!next(f, &v)) return 2; state[c] = (uint16_t)v; }
            if (m < ncand)
                for (uint64_t i = 0; i < ns + 2; i++)
                    pclean_cross_site(S, O, i, rows[2 * m], rows[2 * m + 1], (uint32_t)m, (uint32_t)number, state, nc);
            printf("cross");
            for (uint32_t c = 0; c < nc; c++) printf(" %u", (unsigned)state[c]);
            printf("\n");
        } else if (cmd == 4) {
            if (!next(f, &v)) return 2;
            uint32_t lo, hi;
            pclean_owner_range(O, (uint32_t)v, &lo, &hi);
            printf("own");
            for (uint32_t k = lo; k < hi; k++) printf(" %u", own[k]);
            printf("\n");
        } else if (cmd == 5) {
            if (!next(f, &v)) return 2;
            for (uint32_t c = 0; c < nc; c++) state[c] = 7;
            printf("fate %u\n", pclean_fate(state, nc, (uint32_t)v));
        } else {
            return 2;
        }
    }
    free(eoff); free(sites); free(unit); free(ooff); free(own); free(rows); free(state);
    fclose(f);
    return 0;
}

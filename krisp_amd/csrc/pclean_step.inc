// pclean_step.inc -- part of krisp_hip.hip, and of tests/pclean_step_check.cpp: the pieces of the clean panel selection
// (k_panel_clean.inc, DESIGN §26) that index memory, in plain C++ for host and device: no LDS, no thread index.  A translation
// unit without HIP defines __host__ and __device__ empty and includes krisp_hip.h (kr_product_site) before this file.
//
// The store: ns sites of all scanned genomes, a genome's in position order, and beside every site its unit, a record number
// that no two records of the scans share -- so two neighbours of one unit lie in one record of one genome.  The table has
// ne = 2 T entries: entry 2 t = text t as written, an OPENING site; entry 2 t + 1 = its reverse complement, a CLOSING site;
// eoff[0 .. ne] = the entries' offsets, so entry e has eoff[e + 1] - eoff[e] letters.  A product (DESIGN §24): an opening site
// a and a closing site b of one unit with a.pos + n_a <= b.pos and b.pos + n_b - a.pos <= max_product.  The host refuses a
// max_product below twice the longest text, so max_product - smin and max_product - n do not wrap.
// The owners: a CSR over the texts, ooff[0 .. T] ascending into own[0 .. nown), candidate positions ascending per text.
// Every index is tested against its bound before the load or store.
#include <stdint.h>

#define PCLEAN_NONE 0xffffffffu
#define PCLEAN_FATE_CROSS 4u
#define PCLEAN_FATE_SELF 5u

struct PcleanStore {
    const kr_product_site* sites;
    const uint32_t* unit;
    uint64_t ns;
    const uint32_t* eoff;
    uint32_t ne;                    // 2 T
    uint32_t smin;                  // letters of the shortest text
    uint32_t max_product;
};

__host__ __device__ inline bool pclean_opening(uint32_t e) { return (e & 1u) == 0u; }

// letters of entry e; 0 for an entry the table does not have
__host__ __device__ inline uint32_t pclean_len(const PcleanStore& S, uint32_t e) { return e < S.ne ? S.eoff[e + 1u] - S.eoff[e] : 0u; }

// site i (i < ns) is a site of the table: its entry, else PCLEAN_NONE
__host__ __device__ inline uint32_t pclean_entry(const PcleanStore& S, uint64_t i) {
    if (i >= S.ns) return PCLEAN_NONE;
    const uint32_t e = S.sites[i].entry;
    return e < S.ne ? e : PCLEAN_NONE;
}

// the products the opening site i opens: on_hit(j, entry of the closing site j) in store order; on_hit returns false to
// end the walk.  Nothing for a closing site or an index outside the store
template <typename F>
__host__ __device__ inline void pclean_forward(const PcleanStore& S, uint64_t i, F&& on_hit) {
    const uint32_t ea = pclean_entry(S, i);
    if (ea == PCLEAN_NONE || !pclean_opening(ea)) return;
    const uint64_t apos = S.sites[i].pos;
    const uint64_t first = apos + pclean_len(S, ea), last = apos + (uint64_t)(S.max_product - S.smin);
    const uint32_t u = S.unit[i];
    for (uint64_t j = i + 1u; j < S.ns; j++) {
        const uint64_t bpos = S.sites[j].pos;
        if (S.unit[j] != u || bpos > last) break;
        if (bpos < first) continue;
        const uint32_t eb = pclean_entry(S, j);
        if (eb == PCLEAN_NONE || pclean_opening(eb)) continue;
        if (bpos + pclean_len(S, eb) - apos > (uint64_t)S.max_product) continue;
        if (!on_hit(j, eb)) return;
    }
}

// the products the closing site i closes: on_hit(j, entry of the opening site j), the store read backwards from i down to
// the position b.pos + n_b - max_product, saturated at 0
template <typename F>
__host__ __device__ inline void pclean_backward(const PcleanStore& S, uint64_t i, F&& on_hit) {
    const uint32_t eb = pclean_entry(S, i);
    if (eb == PCLEAN_NONE || pclean_opening(eb)) return;
    const uint64_t bpos = S.sites[i].pos, bend = bpos + pclean_len(S, eb);
    const uint64_t lower = bend > (uint64_t)S.max_product ? bend - (uint64_t)S.max_product : 0u;
    const uint32_t u = S.unit[i];
    for (uint64_t j = i; j-- > 0u;) {
        const uint64_t apos = S.sites[j].pos;
        if (S.unit[j] != u || apos < lower) break;
        const uint32_t ea = pclean_entry(S, j);
        if (ea == PCLEAN_NONE || !pclean_opening(ea)) continue;
        if (apos + pclean_len(S, ea) > bpos) continue;
        if (!on_hit(j, ea)) return;
    }
}

struct PcleanOwners {
    const uint32_t* ooff;           // T + 1
    const uint32_t* own;            // nown
    uint32_t T, nown;
};

// the owners of text t are own[*lo .. *hi); an empty range for a text outside the table or offsets outside the list
__host__ __device__ inline void pclean_owner_range(const PcleanOwners& O, uint32_t t, uint32_t* lo, uint32_t* hi) {
    *lo = *hi = 0u;
    if (t >= O.T) return;
    const uint32_t a = O.ooff[t], b = O.ooff[t + 1u];
    if (a > b || b > O.nown) return;
    *lo = a;
    *hi = b;
}

// fate and by are two bytes a candidate, written and read as one 16-bit word: fate in the low byte, by in the high one
__host__ __device__ inline uint32_t pclean_fate(const uint16_t* state, uint32_t ncand, uint32_t c) {
    return c < ncand ? (uint32_t)(state[c] & 0xffu) : PCLEAN_NONE;
}

// every owner of text t: (5, 0).  Several threads may store the same word
__host__ __device__ inline void pclean_mark_self(const PcleanOwners& O, uint32_t t, uint16_t* state, uint32_t ncand) {
    uint32_t lo, hi;
    pclean_owner_range(O, t, &lo, &hi);
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t c = O.own[k];
        if (c < ncand) state[c] = (uint16_t)PCLEAN_FATE_SELF;
    }
}

// every owner of text t above the member's position m that is still alive: (4, number).  Several threads may store the same
// word; a candidate another thread has just marked reads 4 and is left alone
__host__ __device__ inline void pclean_mark_cross(const PcleanOwners& O, uint32_t t, uint32_t m, uint32_t number, uint16_t* state,
                                                  uint32_t ncand) {
    uint32_t lo, hi;
    pclean_owner_range(O, t, &lo, &hi);
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t c = O.own[k];
        if (c > m && c < ncand && (state[c] & 0xffu) == 0u) state[c] = (uint16_t)(PCLEAN_FATE_CROSS | (number << 8));
    }
}

// what a thread of k_pclean_self does for site i
__host__ __device__ inline void pclean_self_site(const PcleanStore& S, const PcleanOwners& O, uint64_t i, uint16_t* state, uint32_t ncand) {
    pclean_forward(S, i, [&](uint64_t j, uint32_t eb) {
        const uint32_t ea = pclean_entry(S, i);
        (void)j;
        if ((eb >> 1) != (ea >> 1)) return true;
        pclean_mark_self(O, ea >> 1, state, ncand);
        return false;
    });
}

// what a thread of k_pclean_cross does for site i: tx, ty = the member's two texts, m its position, number = its 1-based number
__host__ __device__ inline void pclean_cross_site(const PcleanStore& S, const PcleanOwners& O, uint64_t i, uint32_t tx, uint32_t ty,
                                                  uint32_t m, uint32_t number, uint16_t* state, uint32_t ncand) {
    const uint32_t e = pclean_entry(S, i);
    if (e == PCLEAN_NONE || ((e >> 1) != tx && (e >> 1) != ty)) return;
    auto mark = [&](uint64_t j, uint32_t partner) {
        (void)j;
        pclean_mark_cross(O, partner >> 1, m, number, state, ncand);
        return true;
    };
    if (pclean_opening(e)) pclean_forward(S, i, mark);
    else pclean_backward(S, i, mark);
}

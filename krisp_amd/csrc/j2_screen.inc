// j2_screen.inc -- part of krisp_hip.hip, and of tests/join2_screen_check.cpp: the screen of the two-genome join
// (k_join2.inc) in plain C++ for host and device: no HIP call, no LDS, no thread index.  A translation unit without HIP
// defines __host__ and __device__ empty before it includes this file.
//
// Inside one item all prefixes share the key's bits from rb + mlog upwards; what tells two of them apart are the bits
// [p0, rb + mlog) -- the item key, at most 44 bits wherever the kernels with 32-bit heads apply (sh = rb + mlog - 12 <=
// p0 + 32).  Screen slot and table hash are functions of the item key alone, so of the PREFIX alone: nothing below bit
// p0 (the diagnostic base, the rest of the window) reaches them, and all keys of one prefix, of both genomes, share a slot.
//
// A screen slot is one byte: the low nibble collects the diagnostic bases the ANCHOR shows in the slot (bit = base),
// the high nibble the other genome's.  A candidate prefix has bases SA != 0 in the anchor, SB != 0 in the other genome
// and SA & SB == 0, so its slot holds both nibbles non-zero and at least two different bases in all; bits that other
// prefixes of the slot add never take that away.  The rule is per slot, never per key: either every key of a prefix
// goes on to the exact join or none does.
#include <stdint.h>

#ifndef J2_SCREEN_LOG
#define J2_SCREEN_LOG 14        // slots of the screen (one byte each: 16 KB)
#endif
#define J2_SCREEN (1u << J2_SCREEN_LOG)
#ifndef J2_TAB_LOG
#define J2_TAB_LOG 10           // slots of the exact table
#endif
#define J2_TAB (1u << J2_TAB_LOG)
#ifndef J2_PROBES
#define J2_PROBES 64u           // slots a key is looked for in: a live key that finds no room in them hands its item on
#endif

// the item key of a key: bits [p0, p0 + w) of it, w = rb + mlog - p0 (1 .. 63)
__host__ __device__ inline uint64_t j2_item_key(uint64_t key, int p0, int w) { return (key >> p0) & ((1ull << w) - 1); }

__host__ __device__ inline uint32_t j2_mix(uint64_t ik, uint32_t k0, uint32_t k1) {
    return (uint32_t)ik * k0 + (uint32_t)(ik >> 32) * k1;
}
__host__ __device__ inline uint32_t j2_slot(uint64_t ik) { return j2_mix(ik, 0x9E3779B1u, 0x85EBCA77u) >> (32 - J2_SCREEN_LOG); }
__host__ __device__ inline uint32_t j2_tab_hash(uint64_t ik) { return j2_mix(ik, 0xC2B2AE3Du, 0x27D4EB2Fu) >> (32 - J2_TAB_LOG); }

// the bit a key ORs into the screen's word slot >> 2
__host__ __device__ inline uint32_t j2_bit(uint32_t slot, uint32_t base, bool other) {
    return 1u << (8u * (slot & 3u) + base + (other ? 4u : 0u));
}
__host__ __device__ inline uint32_t j2_byte(uint32_t word, uint32_t slot) { return (word >> (8u * (slot & 3u))) & 255u; }

// anchor's bases a, the other genome's b (four bits each)
__host__ __device__ inline bool j2_live(uint32_t a, uint32_t b) {
    const uint32_t u = (a | b) & 15u;
    return (a & 15u) != 0 && (b & 15u) != 0 && (u & (u - 1)) != 0;
}
__host__ __device__ inline bool j2_live_byte(uint32_t byte) { return j2_live(byte & 15u, byte >> 4); }
// the same rule as one comparison: the smallest of a, b and (a | b) without its lowest bit is not zero
__host__ __device__ inline bool j2_live_byte_min(uint32_t byte) {
    const uint32_t a = byte & 15u, b = (byte >> 4) & 15u, u = a | b, two = u & (u - 1u);
    const uint32_t m = a < b ? a : b;
    return (m < two ? m : two) != 0;
}

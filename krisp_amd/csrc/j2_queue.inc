// j2_queue.inc -- part of krisp_hip.hip, and of tests/join2_queue_check.cpp: the arithmetic of the per-wave queue of live
// keys in the two-genome join (k_join2.inc, k_join2<true>) in plain C++ for host and device: no HIP call, no LDS, no thread
// index.  A translation unit without HIP defines __host__ and __device__ empty before it includes this file.
//
// A wave of 64 lanes owns J2Q_CAP entries of 8 bytes.  Per key slot it takes a ballot of "my key is live"; a live lane's
// entry goes to place fill + (live lanes below it), the fill grows by the ballot's population.  The fill is below J2Q_DRAIN
// in front of every append, so it stays below J2Q_CAP behind it.  Whenever it reaches J2Q_DRAIN the wave joins the
// J2Q_DRAIN entries on top, [fill - J2Q_DRAIN, fill), lane l taking entry fill - J2Q_DRAIN + l, and the fill falls by
// J2Q_DRAIN: nothing is moved, the order of the join is free.  What is left at the end of a visit is joined the same way
// from place 0 with the lanes below the fill.
//
// An entry is the key from its diagnostic base upwards, key >> (p0 - 2): the base in bits 0 and 1, the item key
// (j2_screen.inc: w bits, at most 44 on this route) from bit 2 on, the item's number -- the same in all its keys -- above.
// A live lane pays one funnel shift and one shift for it; the masks are the join's, where every lane has an entry.
#include <stdint.h>

#define J2Q_DRAIN 64u           // entries one join takes: a full wave
#define J2Q_CAP 128u            // entries of one wave's queue
#define J2Q_KEY_BITS 44

// the live lanes below `lane` in the ballot (the device's mbcnt of the ballot)
__host__ __device__ inline uint32_t j2q_below(uint64_t ballot, uint32_t lane) {
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}
// where a live lane writes, `below` = j2q_below(ballot, lane)
__host__ __device__ inline uint32_t j2q_place(uint32_t fill, uint32_t below) { return fill + below; }
__host__ __device__ inline uint32_t j2q_fill_after(uint32_t fill, uint64_t ballot) { return fill + (uint32_t)__builtin_popcountll(ballot); }
__host__ __device__ inline bool j2q_drains(uint32_t fill) { return fill >= J2Q_DRAIN; }
// a join of n entries (n = J2Q_DRAIN, or the rest at the end of a visit) reads from here on; fill - n are left
__host__ __device__ inline uint32_t j2q_first(uint32_t fill, uint32_t n) { return fill - n; }

// the entry of key hi:lo, p0 = the prefix's lowest bit (2 .. 31 on this route: the base lies right below it)
__host__ __device__ inline uint64_t j2q_entry(uint32_t lo, uint32_t hi, int p0) {
    const uint32_t s = (uint32_t)(p0 - 2);
#if defined(__HIP_DEVICE_COMPILE__)
    return ((uint64_t)(hi >> s) << 32) | __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (((uint64_t)hi << 32) | lo) >> s;
#endif
}
// = j2_item_key(key, p0, w) and the key's diagnostic base
__host__ __device__ inline uint64_t j2q_key(uint64_t entry, int w) { return (entry >> 2) & ((1ull << w) - 1ull); }
__host__ __device__ inline uint32_t j2q_base(uint64_t entry) { return (uint32_t)entry & 3u; }

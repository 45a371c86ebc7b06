// k_gunzip.inc -- part of krisp_hip.hip (one translation unit): ONE plain gzip member (what `gzip genome.fa` writes)
// inflated on the device -- the scheme of h_pgzip.inc (pugz / rapidgzip) with the decoder of k_inflate.inc.
//
// The deflate data is cut into chunks of C compressed bytes, and:
//   k_gz_find    a wave per chunk after the first finds the chunk's first block start, its lanes on consecutive bits:
//                cheap filters in registers (BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29, a complete precode), then on the
//                survivors pgz_is_block_start's rule -- strict header, the block decodes, a well-formed header follows;
//   k_gz_decode  a lane per chunk decodes from its start to the first found start it meets on a block boundary (a start
//                inside a block is stepped over, as pgz_at_join does) or to the end of the final block.  Pass 1 counts
//                (output length, stop bit); the host lines the chunks up from the first and places them (a scan of their
//                lengths); pass 2 decodes the chunks of that line again and writes 16-bit symbols at their places: a byte,
//                or 0x8000 + the place in the 32 KB in front of the chunk, copied along like any other symbol.  Two passes
//                instead of slots: a run of Ns inflates 1000:1, no slot size fits it, and the pass that only counts writes
//                nothing;
//   k_gz_window  the 32 KB in front of every chunk, as bytes: a workgroup per run of chunks whose windows need the window
//                before theirs (markers in the 32 KB in front), walked in order; the other runs side by side;
//   k_gz_emit    symbols -> bytes of c->tx_text, markers looked up in their chunk's window, coalesced;
//   k_gz_crc     CRC-32 of every 64 KB of the text, combined on the host against the trailer.
// Every read is bounded by the deflate data (+ 64 zero bytes of padding), every write by the chunk's length from pass 1
// or the text's; anything irregular stops the lane with a status and the host falls back (h_gunzip.inc).
// ----------------------------------------------------------------------------
#define GZ_NONE 0xFFFFFFFFFFFFFFFFull
#define GZ_SEG 65536u                   // bytes of text per CRC segment
#define GZ_WIN 32768u
#define GZ_TRIAL_OUT (16u << 20)        // a trial block may decode to this much (pgz_is_block_start's limit)
enum { GZ_E_NOSTART = 20 };            // (a chunk whose range holds no block start: not decoded)
struct GzRes { u64 end; u32 len, status, final_, lastmark; };      // lastmark: 1 + the chunk's last marker (0: none; pass 2)

// the code lengths of the fixed block -> the two codes (RFC 1951 3.2.6)
__device__ __forceinline__ void gz_fixed(unsigned short* t16, uint8_t* lens, u32 lane) {
    for (int s = 0; s < 144; s++) lens[s * BGZ_T + lane] = 8;
    for (int s = 144; s < 256; s++) lens[s * BGZ_T + lane] = 9;
    for (int s = 256; s < 280; s++) lens[s * BGZ_T + lane] = 7;
    for (int s = 280; s < 288; s++) lens[s * BGZ_T + lane] = 8;
    for (int s = 288; s < 318; s++) lens[s * BGZ_T + lane] = 5;
    unsigned short* const offs = t16 + BGZ_OFFS * BGZ_T;
    (void)bgz_construct(t16 + BGZ_LCNT * BGZ_T, t16 + BGZ_LSYMO * BGZ_T, offs, lens, 288, lane);
    (void)bgz_construct(t16 + BGZ_DCNT * BGZ_T, t16 + BGZ_DSYMO * BGZ_T, offs, lens + 288 * BGZ_T, 30, lane);
}

// the header of a dynamic block behind its type bits -> the two codes.  strict: an incomplete literal / length code is
// refused too (pgz_dynamic_header's trial rule); otherwise zlib's rule (incomplete only as a single code of length one)
__device__ int gz_dyn_header(BgzBits& b, unsigned short* t16, uint8_t* lens, u32 lane, bool strict) {
    unsigned short* const lcnt = t16 + BGZ_LCNT * BGZ_T;
    unsigned short* const lsym = t16 + BGZ_LSYMO * BGZ_T;
    unsigned short* const dcnt = t16 + BGZ_DCNT * BGZ_T;
    unsigned short* const dsym = t16 + BGZ_DSYMO * BGZ_T;
    unsigned short* const offs = t16 + BGZ_OFFS * BGZ_T;
    const int nl = (int)b.bits(5) + 257, nd = (int)b.bits(5) + 1, nc = (int)b.bits(4) + 4;
    if (nl > 286 || nd > 30) return BGZ_E_HEADER;
    for (int s = 0; s < 19; s++) lens[s * BGZ_T + lane] = 0;
    const u64 order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                         10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const u64 order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    int any = 0;
    for (int i = 0; i < nc; i++) {
        const u32 which = i < 12 ? (u32)(order_lo >> (5 * i)) & 31u : (u32)(order_hi >> (5 * (i - 12))) & 31u;
        const u32 l = b.bits(3);
        any |= (int)l;
        lens[which * BGZ_T + lane] = (uint8_t)l;
    }
    if (!any || bgz_construct(lcnt, lsym, offs, lens, 19, lane) != 0) return BGZ_E_CODE;
    const u64 pkc = bgz_pack(lcnt, lane);
    int index = 0;
    while (index < nl + nd) {
        const int s = bgz_decode(b, lcnt, lsym, lane, pkc);
        if (s < 0) return BGZ_E_SYMBOL;
        if (s < 16) {
            lens[index * BGZ_T + lane] = (uint8_t)s;
            index++;
            continue;
        }
        int len = 0, rep;
        if (s == 16) {
            if (index == 0) return BGZ_E_HEADER;
            len = lens[(index - 1) * BGZ_T + lane];
            rep = 3 + (int)b.bits(2);
        } else if (s == 17) {
            rep = 3 + (int)b.bits(3);
        } else {
            rep = 11 + (int)b.bits(7);
        }
        if (index + rep > nl + nd) return BGZ_E_HEADER;
        while (rep--) lens[index++ * BGZ_T + lane] = (uint8_t)len;
    }
    if (lens[256 * BGZ_T + lane] == 0) return BGZ_E_HEADER;
    // (the literal / length code's lengths stay where they are; the distance code's follow them at nl)
    int e = bgz_construct(lcnt, lsym, offs, lens, nl, lane);
    if (e < 0 || (e > 0 && (strict || nl != (int)lcnt[lane] + (int)lcnt[1 * BGZ_T + lane]))) return BGZ_E_CODE;
    e = bgz_construct(dcnt, dsym, offs, lens + nl * BGZ_T, nd, lane);
    if (e < 0 || (e > 0 && nd != (int)dcnt[lane] + (int)dcnt[1 * BGZ_T + lane])) return BGZ_E_CODE;
    return BGZ_OK;
}

// the data of a Huffman-coded block up to its end-of-block code.  MODE 0 counts (trial), 1 counts (pass 1), 2 writes the
// symbols to out[0 .. cap).  first: the chunk at the member's start -- nothing lies in front of it
template <int MODE>
__device__ int gz_block_data(BgzBits& b, const unsigned short* t16, u32 lane, u64 in_bits, unsigned short* __restrict__ out,
                             u32& o, u32 cap, bool first, u32& lastmark) {
    const unsigned short* const lcnt = t16 + BGZ_LCNT * BGZ_T;
    const unsigned short* const lsym = t16 + BGZ_LSYMO * BGZ_T;
    const unsigned short* const dcnt = t16 + BGZ_DCNT * BGZ_T;
    const unsigned short* const dsym = t16 + BGZ_DSYMO * BGZ_T;
    const u64 pkl = bgz_pack(lcnt, lane), pkd = bgz_pack(dcnt, lane);
    for (;;) {
        // (every symbol uses at least one bit: the loop ends with the data at the latest -- zeros behind it decode, too)
        if (b.used() > in_bits) return BGZ_E_IN;
        int s = bgz_decode(b, lcnt, lsym, lane, pkl);
        if (s < 0) return BGZ_E_SYMBOL;
        if (s < 256) {
            if (o >= cap) return BGZ_E_OUT;
            if (MODE == 2) out[o] = (unsigned short)s;
            o++;
            continue;
        }
        if (s == 256) return b.used() > in_bits ? BGZ_E_IN : BGZ_OK;
        s -= 257;
        if (s >= 29) return BGZ_E_SYMBOL;
        u32 len;
        if (s < 8) len = 3u + (u32)s;
        else if (s == 28) len = 258u;
        else {
            const int e = (s - 4) >> 2;
            len = 3u + ((4u + ((u32)s & 3u)) << e) + b.bits(e);
        }
        const int d = bgz_decode(b, dcnt, dsym, lane, pkd);
        if (d < 0 || d >= 30) return BGZ_E_SYMBOL;
        u32 dist;
        if (d < 4) dist = 1u + (u32)d;
        else {
            const int e = (d >> 1) - 1;
            dist = 1u + ((2u + ((u32)d & 1u)) << e) + b.bits(e);
        }
        if (o > cap || len > cap - o) return BGZ_E_OUT;
        if (dist > o && first) return BGZ_E_DIST;
        if (MODE == 2) {
            u32 any = 0;
            if (dist > o) {
                // (reaches into the unknown window: markers for those places, what the chunk wrote for the rest)
                for (u32 k = 0; k < len; k++) {
                    const u32 at = o + k;
                    const u32 v = at >= dist ? out[at - dist] : 0x8000u | (GZ_WIN + at - dist);
                    out[at] = (unsigned short)v;
                    any |= v;
                }
            } else if (dist >= 4) {
                u64 w8 = 0;
                u32 k = 0;
                for (; k + 4 <= len; k += 4) {
                    u64 v;
                    __builtin_memcpy(&v, out + o + k - dist, 8);
                    __builtin_memcpy(out + o + k, &v, 8);
                    w8 |= v;
                }
                for (; k < len; k++) {
                    const u32 v = out[o + k - dist];
                    out[o + k] = (unsigned short)v;
                    any |= v;
                }
                any |= (u32)(w8 | (w8 >> 16) | (w8 >> 32) | (w8 >> 48));
            } else {
                for (u32 k = 0; k < len; k++) {
                    const u32 v = out[o + k - dist];
                    out[o + k] = (unsigned short)v;
                    any |= v;
                }
            }
            if (any & 0x8000u) lastmark = o + len;
        }
        o += len;
    }
}

// cheap filters on the 74 bits from `bit` on: BFINAL 0 + BTYPE 2, HLIT <= 29, HDIST <= 29, a complete precode
__device__ __forceinline__ bool gz_maybe_start(const uint8_t* __restrict__ d, u64 bit) {
    u64 w0, w1;
    __builtin_memcpy(&w0, d + (bit >> 3), 8);
    __builtin_memcpy(&w1, d + (bit >> 3) + 8, 8);
    const unsigned __int128 v = (((unsigned __int128)w1 << 64) | w0) >> (bit & 7);
    if (((u32)v & 7u) != 4u || ((u32)(v >> 3) & 31u) > 29u || ((u32)(v >> 8) & 31u) > 29u) return false;
    const int nc = (int)((u32)(v >> 13) & 15u) + 4;
    u32 kraft = 0;
    for (int i = 0; i < nc; i++) {
        const u32 l = (u32)(v >> (17 + 3 * i)) & 7u;       // (bits <= 73 of the 121 loaded)
        if (l) kraft += 128u >> l;
    }
    return kraft == 128u;
}

// pgz_is_block_start on the device: the lane's tables in LDS
__device__ bool gz_is_block_start(const uint8_t* __restrict__ d, u32 dn, u64 bit, unsigned short* t16, uint8_t* lens, u32 lane) {
    BgzBits b{d, dn, (u32)(bit >> 3), 0ull, 0};
    b.bits((int)(bit & 7));
    const u64 in_bits = (u64)dn * 8ull;
    if (b.bits(3) != 4u) return false;
    if (gz_dyn_header(b, t16, lens, lane, true) != BGZ_OK) return false;
    u32 o = 0, lm = 0;
    if (gz_block_data<0>(b, t16, lane, in_bits, nullptr, o, GZ_TRIAL_OUT, false, lm) != BGZ_OK) return false;
    const u32 type = b.bits(3) >> 1;
    if (type == 3) return false;
    if (type == 2) return gz_dyn_header(b, t16, lens, lane, true) == BGZ_OK && b.used() <= in_bits;
    if (type == 0) {
        b.bits(b.cnt & 7);
        const u64 at = b.used() >> 3;
        if (at + 4 > dn) return false;
        const u32 len = d[at] | ((u32)d[at + 1] << 8), nlen = d[at + 2] | ((u32)d[at + 3] << 8);
        return (len ^ nlen) == 0xFFFFu;
    }
    return b.used() <= in_bits;
}

// a wave per chunk i >= 1: the first bit of [i cb, min((i + 1) cb, i cb + 512 KB)) bytes where a block starts -> start[i]
__global__ __launch_bounds__(BGZ_T) void k_gz_find(const uint8_t* __restrict__ d, u32 dn, u32 nch, u32 cb, u64* __restrict__ start) {
    __shared__ unsigned short t16[BGZ_U16 * BGZ_T];
    __shared__ uint8_t lens[BGZ_NLEN * BGZ_T];
    const u32 lane = threadIdx.x, i = blockIdx.x + 1;
    if (i >= nch) return;
    const u64 from = (u64)i * cb * 8ull;
    const u64 to_byte = i + 1 == nch ? (u64)dn : (u64)(i + 1) * cb;
    const u64 to = (to_byte < (u64)i * cb + (512u << 10) ? to_byte : (u64)i * cb + (512u << 10)) * 8ull;
    for (u64 base = from; base < to; base += BGZ_T) {
        const u64 bit = base + lane;
        const bool ok = bit < to && gz_maybe_start(d, bit) && gz_is_block_start(d, dn, bit, t16, lens, lane);
        const u64 m = __ballot(ok);
        if (m) {
            if (lane == 0) start[i] = base + (u64)__builtin_ctzll(m);
            return;
        }
    }
    if (lane == 0) start[i] = GZ_NONE;
}

// a lane per chunk (`act` lanes of every wave; the others idle -- the lanes of a wave serialise where they diverge).
// MODE 1: chunk idx of all nch, its length and stop; MODE 2: chunk list[idx] of the line, written at sym + off[idx]
template <int MODE>
__global__ __launch_bounds__(BGZ_T) void k_gz_decode(const uint8_t* __restrict__ d, u32 dn, const u64* __restrict__ start, u32 nch,
                                                     u32 act, const u32* __restrict__ list, u32 nlist, const u64* __restrict__ off,
                                                     GzRes* __restrict__ res, unsigned short* __restrict__ sym, u32 cap) {
    __shared__ unsigned short t16[BGZ_U16 * BGZ_T];
    __shared__ uint8_t lens[BGZ_NLEN * BGZ_T];
    const u32 lane = threadIdx.x;
    if (lane >= act) return;
    const u32 idx = blockIdx.x * act + lane;
    if (idx >= (MODE == 1 ? nch : nlist)) return;
    const u32 ci = MODE == 1 ? idx : list[idx];
    GzRes R{0ull, 0u, BGZ_OK, 0u, 0u};
    const u64 st = start[ci];
    if (st == GZ_NONE) {
        R.status = GZ_E_NOSTART;
        res[ci] = R;
        return;
    }
    unsigned short* const out = MODE == 2 ? sym + off[idx] : nullptr;
    const u32 lim = MODE == 2 ? res[ci].len : cap;
    const bool first = ci == 0;
    const u64 in_bits = (u64)dn * 8ull;
    BgzBits b{d, dn, (u32)(st >> 3), 0ull, 0};
    b.bits((int)(st & 7));
    u32 o = 0, lm = 0, nxt = ci + 1;
    int err = BGZ_OK;
    for (;;) {
        const bool last = b.bits(1) != 0;
        const u32 type = b.bits(2);
        if (type == 0) {
            b.bits(b.cnt & 7);
            const u32 len = b.bits(16), nlen = b.bits(16);
            if ((len ^ 0xFFFFu) != nlen) { err = BGZ_E_STORED; break; }
            if (b.used() + 8ull * len > in_bits) { err = BGZ_E_IN; break; }
            if (o > lim || len > lim - o) { err = BGZ_E_OUT; break; }
            for (u32 k = 0; k < len; k++) {
                const u32 v = b.bits(8);
                if (MODE == 2) out[o + k] = (unsigned short)v;
            }
            o += len;
        } else if (type == 3) {
            err = BGZ_E_BTYPE;
            break;
        } else {
            if (type == 1) gz_fixed(t16, lens, lane);
            else if ((err = gz_dyn_header(b, t16, lens, lane, false)) != BGZ_OK) break;
            if ((err = gz_block_data<MODE>(b, t16, lane, in_bits, out, o, lim, first, lm)) != BGZ_OK) break;
        }
        const u64 p = b.used();
        if (p > in_bits) { err = BGZ_E_IN; break; }
        if (last) {
            R.final_ = 1u;
            R.end = p;
            break;
        }
        // a found start on this block boundary: the next chunk goes on from here (a start behind it was none)
        while (nxt < nch && (start[nxt] == GZ_NONE || start[nxt] < p)) nxt++;
        if (nxt < nch && start[nxt] == p) {
            R.end = p;
            break;
        }
    }
    if (MODE == 2 && err == BGZ_OK && o != lim) err = BGZ_E_LEN;
    R.status = (u32)err;
    R.len = o;
    R.lastmark = lm;
    if (MODE == 1) res[ci] = R;
    else res[ci + nch] = R;             // (pass 2 beside pass 1: lengths and stops must agree)
}

// index of the chunk of the line that holds text byte g: the last k with off[k] <= g
__device__ __forceinline__ u32 gz_chunk_of(const u64* __restrict__ off, u32 npath, u64 g) {
    u32 lo = 0, hi = npath;         // off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// a workgroup per run of the line's chunks (chain[2 r], chain[2 r + 1]: first chunk, count), windows in order: window k =
// the text's 32 KB in front of off[k], markers looked up in the window of the chunk that holds them (one of this run's,
// earlier: h_gunzip.inc draws the runs so)
__global__ __launch_bounds__(256) void k_gz_window(const unsigned short* __restrict__ sym, const u64* __restrict__ off, u32 npath,
                                                   const u32* __restrict__ chain, uint8_t* __restrict__ win, u32* __restrict__ nbad) {
    const u32 k0 = chain[2 * blockIdx.x], nk = chain[2 * blockIdx.x + 1];
    u32 bad = 0;
    for (u32 k = k0; k < k0 + nk; k++) {
        uint8_t* const w = win + (u64)k * GZ_WIN;
        const long long lo = (long long)off[k] - (long long)GZ_WIN;
        for (u32 t = threadIdx.x; t < GZ_WIN; t += 256) {
            const long long g = lo + (long long)t;
            uint8_t v = 0;
            if (g >= 0) {
                const u32 s = sym[g];
                if (!(s & 0x8000u)) v = (uint8_t)s;
                else {
                    const u32 j = gz_chunk_of(off, npath, (u64)g);
                    const u32 m = s & 0x7FFFu;
                    if ((long long)off[j] - (long long)GZ_WIN + (long long)m < 0 || j >= k) bad = 1;
                    else v = win[(u64)j * GZ_WIN + m];
                }
            }
            w[t] = v;
        }
        __syncthreads();            // (the next window may read this one: same workgroup, same CU)
    }
    if (bad) atomicAdd(nbad, 1u);
}

// symbols -> bytes, eight per thread: text[g] = sym[g], or the byte of its chunk's window a marker names
__global__ __launch_bounds__(256) void k_gz_emit(const unsigned short* __restrict__ sym, const u64* __restrict__ off, u32 npath,
                                                 const uint8_t* __restrict__ win, u64 total, uint8_t* __restrict__ text,
                                                 u32* __restrict__ nbad) {
    const u64 g0 = ((u64)blockIdx.x * 256u + threadIdx.x) * 8ull;
    if (g0 >= total) return;
    u32 k = gz_chunk_of(off, npath, g0);
    u32 bad = 0;
    uint8_t b8[8];
    const u32 nn = total - g0 < 8 ? (u32)(total - g0) : 8u;
    for (u32 e = 0; e < nn; e++) {
        const u64 g = g0 + e;
        while (k + 1 < npath && off[k + 1] <= g) k++;
        const u32 s = sym[g];
        if (!(s & 0x8000u)) b8[e] = (uint8_t)s;
        else {
            const u32 m = s & 0x7FFFu;
            if (k == 0 || (long long)off[k] - (long long)GZ_WIN + (long long)m < 0) { bad = 1; b8[e] = 0; }
            else b8[e] = win[(u64)k * GZ_WIN + m];
        }
    }
    if (nn == 8) __builtin_memcpy(text + g0, b8, 8);
    else for (u32 e = 0; e < nn; e++) text[g0 + e] = b8[e];
    if (bad) atomicAdd(nbad, 1u);
}

// CRC-32 (reflected 0xEDB88320, initial and final xor) of every GZ_SEG bytes of the text, a lane per segment
__global__ __launch_bounds__(BGZ_T) void k_gz_crc(const uint8_t* __restrict__ text, u64 total, u32 nseg, u32* __restrict__ crcs) {
    __shared__ u32 T[256];
    for (u32 i = threadIdx.x; i < 256; i += BGZ_T) {
        u32 c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        T[i] = c;
    }
    __syncthreads();
    const u32 sgi = blockIdx.x * BGZ_T + threadIdx.x;
    if (sgi >= nseg) return;
    const u64 a = (u64)sgi * GZ_SEG;
    const u32 n = total - a < GZ_SEG ? (u32)(total - a) : GZ_SEG;
    const uint8_t* __restrict__ p = text + a;
    u32 c = 0xFFFFFFFFu, i = 0;
    for (; i + 8 <= n; i += 8) {
        u64 v;
        __builtin_memcpy(&v, p + i, 8);
#pragma unroll
        for (int q = 0; q < 8; q++) c = T[(c ^ (u32)(v >> (8 * q))) & 0xFFu] ^ (c >> 8);
    }
    for (; i < n; i++) c = T[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    crcs[sgi] = c ^ 0xFFFFFFFFu;
}

// k_text.inc -- part of krisp_hip.hip (one translation unit): the reference reader on the device (SURVEY 8f rank 1).
// File text (FASTA, or one sequence per line) -> the upload buffer: record bodies joined by one '\n', with exactly the
// semantics of kr_fasta_to_bases (h_text.inc; kstream.py:458-583): the first line decides FASTA mode (and is consumed
// when the text comes from a file), lines are stripped of white space at both ends (str.strip()'s, in UTF-8), header lines
// start a record, empty lines and empty records vanish (FASTA) / every line is a record (plain).  The host then only reads
// and inflates.
//   k_tx_firstline     FASTA mode: a '>' anywhere in the first line
//   k_tx_starts_*      line starts (p = 0, after '\n', after a lone '\r' under universal newlines) -> linestart[]
//   k_tx_lineinfo      per line: stripped body [s, s + len), what the line does to the record state
//   k_tx_scan1/2/3     a scan over the lines: which lines open a record, where every line's bytes go
//   k_tx_copy          output-driven: 16 KB of output per workgroup (long single-line records copy as fast as short ones)
//   k_tx_stats1/2, k_tx_finish   characters outside ACGTNacgtn, RNA detection (first record holding T or U), U -> T
// ----------------------------------------------------------------------------
struct TxState {           // device words of one parse (read back through the host mailbox)
    u32 fasta, nlines, nout, nrec, special, pT, pU, q, rna, ucount;
};

// white space as the reference's str.strip() sees it (is_space / space_head / space_tail of h_text.inc): ASCII 9-13, 28-31,
// ' ', and the UTF-8 forms of U+0085, U+00A0, U+1680, U+2000-U+200A, U+2028, U+2029, U+202F, U+205F, U+3000
__device__ __forceinline__ bool tx_space(u32 c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }
__device__ __forceinline__ bool tx_space2(u32 a, u32 b) { return a == 0xc2 && (b == 0x85 || b == 0xa0); }
__device__ __forceinline__ bool tx_space3(u32 a, u32 b, u32 c) {
    if (a == 0xe2) return (b == 0x80 && (c <= 0x8a || c == 0xa8 || c == 0xa9 || c == 0xaf)) || (b == 0x81 && c == 0x9f);
    return (a == 0xe1 && b == 0x9a && c == 0x80) || (a == 0xe3 && b == 0x80 && c == 0x80);
}
// bytes of the white space character at the start / end of [s, e) (s < e); 0: none
__device__ __forceinline__ u32 tx_space_head(const uint8_t* __restrict__ t, u32 s, u32 e) {
    const u32 c = t[s];
    if (c < 0x80) return tx_space(c) ? 1u : 0u;
    if (e - s >= 2 && tx_space2(c, t[s + 1])) return 2;
    return e - s >= 3 && tx_space3(c, t[s + 1], t[s + 2]) ? 3u : 0u;
}
__device__ __forceinline__ u32 tx_space_tail(const uint8_t* __restrict__ t, u32 s, u32 e) {
    const u32 c = t[e - 1];
    if (c < 0x80) return tx_space(c) ? 1u : 0u;
    if (e - s >= 2 && tx_space2(t[e - 2], c)) return 2;
    return e - s >= 3 && tx_space3(t[e - 3], t[e - 2], c) ? 3u : 0u;
}
// is byte position p the start of a line?  (universal newlines: '\n', '\r' and "\r\n" all end a line)
__device__ __forceinline__ bool tx_is_start(const uint8_t* __restrict__ t, u64 p, int universal) {
    if (p == 0) return true;
    const u32 prev = t[p - 1];
    if (prev == '\n') return true;
    return universal && prev == '\r' && t[p] != '\n';
}

__global__ __launch_bounds__(1024) void k_tx_firstline(const uint8_t* __restrict__ t, u32 n, int universal, TxState* st) {
    __shared__ u32 s_end, s_gt;
    if (threadIdx.x == 0) { s_end = n; s_gt = 0; }
    __syncthreads();
    // end of the first line: the first break character
    for (u32 base = 0; base < n; base += 1024 * 16) {
        u32 found = 0xFFFFFFFFu;
        for (u32 q = 0; q < 16; q++) {
            const u32 i = base + threadIdx.x * 16 + q;
            if (i < n && found == 0xFFFFFFFFu && (t[i] == '\n' || (universal && t[i] == '\r'))) found = i;
        }
        if (found != 0xFFFFFFFFu) atomicMin(&s_end, found);
        __syncthreads();
        if (s_end < n) break;           // (uniform: read after the barrier)
        __syncthreads();
    }
    __syncthreads();
    const u32 e = s_end;
    u32 gt = 0;
    for (u32 i = threadIdx.x; i < e; i += 1024) gt |= t[i] == '>' ? 1u : 0u;
    if (gt) atomicOr(&s_gt, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        st->fasta = s_gt;
        st->special = 0;
        st->pT = 0xFFFFFFFFu;
        st->pU = 0xFFFFFFFFu;
        st->q = 0xFFFFFFFFu;
        st->rna = 0;
        st->ucount = 0;
    }
}

#define TX_TILE 4096u
__global__ __launch_bounds__(256) void k_tx_starts_count(const uint8_t* __restrict__ t, u32 n, int universal,
                                                         u32* __restrict__ tilecnt) {
    __shared__ u32 waves[17];
    const u32 base = blockIdx.x * TX_TILE + threadIdx.x * 16;
    u32 cnt = 0;
    for (u32 q = 0; q < 16; q++) {
        const u32 p = base + q;
        if (p < n && tx_is_start(t, p, universal)) cnt++;
    }
    u32 total;
    (void)block_excl_scan(cnt, waves, total);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_tx_starts_write(const uint8_t* __restrict__ t, u32 n, int universal,
                                                         const u32* __restrict__ tilepos, u32* __restrict__ linestart) {
    __shared__ u32 waves[17];
    const u32 base = blockIdx.x * TX_TILE + threadIdx.x * 16;
    u32 mask = 0;
    for (u32 q = 0; q < 16; q++) {
        const u32 p = base + q;
        if (p < n && tx_is_start(t, p, universal)) mask |= 1u << q;
    }
    u32 total;
    u32 o = tilepos[blockIdx.x] + block_excl_scan((u32)__popc(mask), waves, total);
    for (u32 q = 0; q < 16; q++)
        if ((mask >> q) & 1u) linestart[o++] = base + q;
}

// per line: body after stripping, and its effect on the record state -- 0 nothing (empty line; the consumed first
// line), 1 header (closes the record), 2 sequence line (opens a record unless one is open), 3 plain mode: a record
__global__ __launch_bounds__(256) void k_tx_lineinfo(const uint8_t* __restrict__ t, u32 n, const u32* __restrict__ linestart,
                                                     u32 nlines, const TxState* __restrict__ st, int one_shot,
                                                     u32* __restrict__ ls, u32* __restrict__ ll, uint8_t* __restrict__ op) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nlines) return;
    u32 s = linestart[j], e = j + 1 < nlines ? linestart[j + 1] : n;
    for (u32 k; s < e && (k = tx_space_head(t, s, e));) s += k;
    for (u32 k; e > s && (k = tx_space_tail(t, s, e));) e -= k;
    u32 o;
    if (j == 0 && one_shot) { o = 0; e = s; }
    else if (!st->fasta) o = 3;
    else if (e > s && t[s] == '>') { o = 1; e = s; }
    else o = e > s ? 2u : 0u;
    ls[j] = s;
    ll[j] = e - s;
    op[j] = (uint8_t)o;
}

// Which lines open a record (a separator goes in front of them, except in front of the first record), where every line's
// bytes go: a scan over the lines with three carried quantities -- the record state (the last header / sequence line
// decides it), the separators, the bytes.  Thread t of TXS_T x G takes a contiguous run of `per` lines; three kernels,
// each a walk over the thread's run:  k_tx_scan1 the runs' effect on the record state (per workgroup: the last one that
// has any);  k_tx_scan2 the state in front of every run (the workgroups before it, the threads before it), its
// separators and bytes, scanned inside the workgroup;  k_tx_scan3 the places (the workgroups before it summed).
// (Round 6: these replace ONE workgroup of 1024 threads walking all lines -- 85 ms per GB of 80-column text, 0.25 s of a
// 3 Gbp genome's ingest, the largest single item of the device's reader; tools/inflate_check.py under rocprofv3.)
#define TXS_T 256
#define TXS_GMAX 1024
__device__ __forceinline__ void txs_run(u32 nlines, u32 per, u32& j0, u32& j1) {
    const u64 t = (u64)blockIdx.x * TXS_T + threadIdx.x;
    const u64 a = t * per;
    j0 = (u32)(a < nlines ? a : nlines);
    j1 = (u32)(a + per < nlines ? a + per : nlines);
}
__global__ __launch_bounds__(TXS_T) void k_tx_scan1(const uint8_t* __restrict__ op, u32 nlines, u32 per, u32* __restrict__ wg_f) {
    __shared__ u32 s_f[TXS_T];
    u32 j0, j1;
    txs_run(nlines, per, j0, j1);
    u32 f = 0;
    for (u32 j = j0; j < j1; j++) {
        const u32 o = op[j] & 3u;
        if (o == 1 || o == 2) f = o;
    }
    s_f[threadIdx.x] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 w = 0;
        for (int q = TXS_T - 1; q >= 0; q--)
            if (s_f[q]) { w = s_f[q]; break; }
        wg_f[blockIdx.x] = w;
    }
}
// thr: per thread (state in front of its run, separators before it inside the workgroup, bytes before it inside the workgroup)
__global__ __launch_bounds__(TXS_T) void k_tx_scan2(const u32* __restrict__ ll, const uint8_t* __restrict__ op, u32 nlines, u32 per,
                                                    const u32* __restrict__ wg_f, u32* __restrict__ thr, u32* __restrict__ wg_sep,
                                                    u32* __restrict__ wg_bytes) {
    __shared__ u32 s_f[TXS_T];
    __shared__ u32 waves[17];
    __shared__ u32 s_wg;
    u32 j0, j1;
    txs_run(nlines, per, j0, j1);
    u32 f = 0;
    for (u32 j = j0; j < j1; j++) {
        const u32 o = op[j] & 3u;
        if (o == 1 || o == 2) f = o;
    }
    s_f[threadIdx.x] = f;
    if (threadIdx.x == 0) {
        u32 w = 1;                      // state before the first line: 1 = no record open, 2 = open
        for (int q = (int)blockIdx.x - 1; q >= 0; q--)
            if (wg_f[q]) { w = wg_f[q]; break; }
        s_wg = w;
    }
    __syncthreads();
    u32 state = s_wg;
    for (int q = (int)threadIdx.x - 1; q >= 0; q--)
        if (s_f[q]) { state = s_f[q]; break; }
    u32 nsep = 0, bytes = 0, s2 = state;
    for (u32 j = j0; j < j1; j++) {
        const u32 o = op[j] & 3u;
        const u32 sep = (o == 3 || (o == 2 && s2 != 2)) ? 1u : 0u;
        if (o == 1 || o == 2) s2 = o;
        nsep += sep;
        bytes += ll[j] + sep;
    }
    u32 tsep, tbytes;
    const u32 sep_before = block_excl_scan(nsep, waves, tsep);
    const u32 bytes_before = block_excl_scan(bytes, waves, tbytes);
    const u64 t = (u64)blockIdx.x * TXS_T + threadIdx.x;
    thr[3 * t] = state;
    thr[3 * t + 1] = sep_before;
    thr[3 * t + 2] = bytes_before;
    if (threadIdx.x == 0) {
        wg_sep[blockIdx.x] = tsep;
        wg_bytes[blockIdx.x] = tbytes;
    }
}
__global__ __launch_bounds__(TXS_T) void k_tx_scan3(const u32* __restrict__ ll, uint8_t* __restrict__ op, u32 nlines, u32 per,
                                                    const u32* __restrict__ thr, const u32* __restrict__ wg_sep,
                                                    const u32* __restrict__ wg_bytes, u32* __restrict__ outpos, TxState* st) {
    __shared__ u32 waves[17];
    // separators and bytes of the workgroups in front of this one (<= TXS_GMAX of them)
    u32 a = 0, b = 0;
    for (u32 q = threadIdx.x; q < blockIdx.x; q += TXS_T) {
        a += wg_sep[q];
        b += wg_bytes[q];
    }
    u32 base_sep, base_bytes;
    (void)block_excl_scan(a, waves, base_sep);
    (void)block_excl_scan(b, waves, base_bytes);
    u32 j0, j1;
    txs_run(nlines, per, j0, j1);
    const u64 t = (u64)blockIdx.x * TXS_T + threadIdx.x;
    u32 s2 = thr[3 * t], ns = base_sep + thr[3 * t + 1], nb = base_bytes + thr[3 * t + 2];
    // places; the first record has no separator in front of it
    for (u32 j = j0; j < j1; j++) {
        const u32 o = op[j] & 3u;
        const u32 sep = (o == 3 || (o == 2 && s2 != 2)) ? 1u : 0u;
        if (o == 1 || o == 2) s2 = o;
        outpos[j] = nb - (ns > 0 ? 1u : 0u);
        op[j] = (uint8_t)(o | ((sep && ns > 0) ? 0x80u : 0u));       // bit 7: this line writes a separator byte first
        ns += sep;
        nb += ll[j] + sep;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const u32 tsep = base_sep + wg_sep[blockIdx.x], tbytes = base_bytes + wg_bytes[blockIdx.x];
        st->nrec = tsep;
        st->nout = tbytes - (tsep > 0 ? 1u : 0u);
        outpos[nlines] = st->nout;
    }
}

#define TX_OUT 16384u
__global__ __launch_bounds__(256) void k_tx_copy(const uint8_t* __restrict__ t, const u32* __restrict__ ls,
                                                 const u32* __restrict__ ll, const uint8_t* __restrict__ op,
                                                 const u32* __restrict__ outpos, u32 nlines, const TxState* __restrict__ st,
                                                 uint8_t* __restrict__ out) {
    __shared__ u32 m_s[256], m_l[256], m_o[256], m_sep[256];
    const u32 nout = st->nout;
    const u32 o0 = blockIdx.x * TX_OUT;
    if (o0 >= nout) return;
    const u32 o1 = min(o0 + TX_OUT, nout);
    // the line that holds output byte o0: the last one whose place is <= o0 (empty lines share places: any of them)
    u32 lo = 0, hi = nlines;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (outpos[mid] <= o0) lo = mid; else hi = mid;
    }
    for (u32 jb = lo; jb < nlines; jb += 256) {
        const u32 j = jb + threadIdx.x;
        __syncthreads();
        if (j < nlines) {
            m_s[threadIdx.x] = ls[j];
            m_l[threadIdx.x] = ll[j];
            m_o[threadIdx.x] = outpos[j];
            m_sep[threadIdx.x] = op[j] >> 7;
        }
        __syncthreads();
        const u32 cntl = min(256u, nlines - jb);
        if (m_o[0] >= o1) break;
        for (u32 q = 0; q < cntl; q++) {
            const u32 start = m_o[q], sep = m_sep[q], len = m_l[q], src = m_s[q];
            if (start >= o1) break;
            const u32 end = start + sep + len;
            const u32 a = max(start, o0), b = min(end, o1);
            for (u32 o = a + threadIdx.x; o < b; o += 256)
                out[o] = (sep && o == start) ? (uint8_t)'\n' : t[src + (o - start - sep)];
        }
        if (m_o[cntl - 1] >= o1) break;
    }
}

// characters outside ACGTNacgtn (and the separator); first T / t and first U / u
__global__ __launch_bounds__(256) void k_tx_stats1(const uint8_t* __restrict__ out, TxState* st) {
    __shared__ u32 waves[17];
    const u32 nout = st->nout;
    u32 special = 0, nu = 0, pT = 0xFFFFFFFFu, pU = 0xFFFFFFFFu;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += (u64)gridDim.x * blockDim.x) {
        const u32 c = out[i], m = c | 0x20u;
        // (U / u counted apart: plain letters when the text turns out to be RNA and they become T / t)
        special += (m == 'a' || m == 'c' || m == 'g' || m == 't' || m == 'n' || m == 'u' || c == '\n') ? 0u : 1u;
        nu += m == 'u' ? 1u : 0u;
        if (m == 't') pT = min(pT, (u32)i);
        if (m == 'u') pU = min(pU, (u32)i);
    }
    u32 total, totu;
    (void)block_excl_scan(special, waves, total);
    (void)block_excl_scan(nu, waves, totu);
    if (threadIdx.x == 0 && total) atomicAdd(&st->special, total);
    if (threadIdx.x == 0 && totu) atomicAdd(&st->ucount, totu);
    if (pT != 0xFFFFFFFFu) atomicMin(&st->pT, pT);
    if (pU != 0xFFFFFFFFu) atomicMin(&st->pU, pU);
}
// end of the record that holds the first U (when it comes before every T)
__global__ __launch_bounds__(256) void k_tx_stats2(const uint8_t* __restrict__ out, TxState* st) {
    const u32 nout = st->nout, pT = st->pT, pU = st->pU;
    if (pU >= pT) return;
    u32 q = 0xFFFFFFFFu;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += (u64)gridDim.x * blockDim.x)
        if (i > pU && out[i] == '\n') q = min(q, (u32)i);
    if (q != 0xFFFFFFFFu) atomicMin(&st->q, q);
}
// RNA iff the first record holding T / t / U / u holds U / u and no T / t (kstream.py:481-508): then U -> T.
// Every workgroup decides alike from the finished words; workgroup 0 records the verdict.
__global__ __launch_bounds__(256) void k_tx_finish(uint8_t* __restrict__ out, TxState* st) {
    const u32 nout = st->nout, pT = st->pT, pU = st->pU, q = st->q;
    // (pT = ~0: no T at all; q = ~0: the record with the first U runs to the end of the text)
    const bool rna = pU < pT && (pT == 0xFFFFFFFFu || (q != 0xFFFFFFFFu && pT > q));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->rna = rna ? 1u : 0u;
        if (!rna) st->special += st->ucount;
    }
    if (!rna) return;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += (u64)gridDim.x * blockDim.x) {
        const u32 c = out[i];
        if (c == 'U') out[i] = 'T';
        else if (c == 'u') out[i] = 't';
    }
}
__global__ void k_tx_publish(const TxState* __restrict__ st, u32* __restrict__ host) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        host[0] = st->nlines; host[1] = st->nout; host[2] = st->nrec; host[3] = st->special;
        host[4] = st->rna; host[5] = st->fasta;
    }
}

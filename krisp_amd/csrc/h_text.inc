// h_text.inc -- part of krisp_hip.hip (one translation unit): host-only text code -- the FASTA parser and the
// scan for windows the device alphabet cannot carry.  No HIP call in this file: tests/native/asan_host.cpp
// builds it alone with g++ -fsanitize=address,undefined and fuzzes it (SURVEY section 5).
// ----------------------------------------------------------------------------
// host side: FASTA / sequence text -> upload buffer, one pass, reference reader semantics
// (kstream.py:458-583; see include/krisp_hip.h).  Pure CPU code; ctypes releases the GIL, so
// the Python layer ingests several files concurrently.
// ----------------------------------------------------------------------------
#ifndef KR_SPAWN_DEFINED
#define KR_SPAWN_DEFINED
// start a host thread; false (nothing started) when the system has none to give (std::system_error: EAGAIN under a
// container's pid / thread limit).  The callers then do that thread's share themselves -- nothing may unwind through the
// extern "C" boundary, and a vector of joinable threads must not be destroyed by an exception (ADVICE r4).
extern "C++" {
template <class... A>
static bool kr_spawn(std::vector<std::thread>& th, A&&... a) {
    try {
        th.emplace_back(std::forward<A>(a)...);
        return true;
    } catch (const std::system_error&) {
        return false;
    } catch (const std::bad_alloc&) {
        return false;
    }
}
}   // extern "C++"
#endif
// White space as the reference's str.strip() sees it on its decoded (UTF-8) lines: the ASCII bytes 9-13, 28-31 and ' ',
// and 19 characters above U+007F -- U+0085, U+00A0 (two bytes), U+1680, U+2000-U+200A, U+2028, U+2029, U+202F, U+205F,
// U+3000 (three).  Matched as byte sequences: in UTF-8 a lead byte is never a continuation byte, so a match at either end
// of a line is a whole character.  (Text that is not UTF-8 makes the reference fail; nothing here decodes.)
static inline bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }
static inline bool is_space2(uint8_t a, uint8_t b) { return a == 0xc2 && (b == 0x85 || b == 0xa0); }
static inline bool is_space3(uint8_t a, uint8_t b, uint8_t c) {
    if (a == 0xe2) return (b == 0x80 && (c <= 0x8a || c == 0xa8 || c == 0xa9 || c == 0xaf)) || (b == 0x81 && c == 0x9f);
    return (a == 0xe1 && b == 0x9a && c == 0x80) || (a == 0xe3 && b == 0x80 && c == 0x80);
}
// bytes of the white space character at the start / end of [p, p + len); 0: none
static inline size_t space_head(const uint8_t* p, size_t len) {
    if (p[0] < 0x80) return is_space(p[0]) ? 1 : 0;
    if (len >= 2 && is_space2(p[0], p[1])) return 2;
    return len >= 3 && is_space3(p[0], p[1], p[2]) ? 3 : 0;
}
static inline size_t space_tail(const uint8_t* p, size_t len) {
    const uint8_t* e = p + len;
    if (e[-1] < 0x80) return is_space(e[-1]) ? 1 : 0;
    if (len >= 2 && is_space2(e[-2], e[-1])) return 2;
    return len >= 3 && is_space3(e[-3], e[-2], e[-1]) ? 3 : 0;
}

int64_t kr_fasta_to_bases(const uint8_t* text, size_t n, int universal_newlines, int one_shot, uint8_t* out,
                          size_t cap, int64_t* stats) {
    if (!text && n) return KR_ERR_PARAM;
    if (cap < n + 1) return KR_ERR_CAPACITY;
    size_t pos = 0, o = 0;
    int64_t nrec = 0;
    bool first_line = true, fasta = false, in_record = false, any_record = false;
    auto emit_separator = [&]() {
        if (any_record) out[o++] = '\n';
        any_record = true;
        nrec++;
    };
    while (pos < n) {
        // one line: [pos, eol)
        // (memchr scans 16+ bytes per step; a byte loop here was half of the parse time)
        size_t eol;
        {
            const void* q = memchr(text + pos, '\n', n - pos);
            eol = q ? (size_t)((const uint8_t*)q - text) : n;
            if (universal_newlines) {
                const void* r = memchr(text + pos, '\r', eol - pos);
                if (r) eol = (size_t)((const uint8_t*)r - text);
            }
        }
        size_t next = eol;
        if (next < n) {
            if (universal_newlines && text[next] == '\r' && next + 1 < n && text[next + 1] == '\n') next += 2;
            else next += 1;
        }
        const uint8_t* ln = text + pos;
        size_t len = eol - pos;
        pos = next;
        if (first_line) {
            first_line = false;
            fasta = memchr(ln, '>', len) != nullptr;         // decided on the first line only
            if (one_shot) continue;                          // ... which the detection consumed
        }
        for (size_t k; len && (k = space_head(ln, len));) { ln += k; len -= k; }
        for (size_t k; len && (k = space_tail(ln, len));) len -= k;
        if (!fasta) {                                        // every stripped line is a record
            emit_separator();
            memcpy(out + o, ln, len);
            o += len;
            continue;
        }
        if (len && ln[0] == '>') { in_record = false; continue; }
        if (!len) continue;
        if (!in_record) { emit_separator(); in_record = true; }
        memcpy(out + o, ln, len);
        o += len;
    }
    // RNA iff the first record holding T/t/U/u holds U/u and no T/t (kstream.py:481-508)
    int rna = -1;
    for (size_t i = 0, rs = 0; i <= o && rna < 0; i++) {
        if (i == o || out[i] == '\n') {
            bool t = false, u = false;
            for (size_t j = rs; j < i; j++) {
                uint8_t c = out[j];
                t |= (c == 'T' || c == 't');
                u |= (c == 'U' || c == 'u');
            }
            if (t) rna = 0; else if (u) rna = 1;
            rs = i + 1;
        }
    }
    if (rna == 1)
        for (size_t i = 0; i < o; i++) {
            if (out[i] == 'U') out[i] = 'T';
            else if (out[i] == 'u') out[i] = 't';
        }
    // characters outside ACGTNacgtn (and the separator), in a form the compiler vectorises
    int64_t special = 0;
    for (size_t i0 = 0; i0 < o; i0 += 1 << 16) {
        const size_t i1 = std::min(o, i0 + ((size_t)1 << 16));
        uint32_t plain = 0;
        for (size_t i = i0; i < i1; i++) {
            const uint8_t c = out[i], m = (uint8_t)(c | 0x20);
            plain += (uint32_t)((m == 'a') | (m == 'c') | (m == 'g') | (m == 't') | (m == 'n') | (c == '\n'));
        }
        special += (int64_t)(i1 - i0) - plain;
    }
    if (stats) { stats[0] = nrec; stats[1] = special; stats[2] = rna; stats[3] = fasta ? 1 : 0; }
    return (int64_t)o;
}

// ----------------------------------------------------------------------------
// host side: the windows the 2-bit device alphabet cannot carry (SURVEY 8b "side channel").
// The device keeps A/C/G/T windows and drops windows holding N, lower case under --omit-soft, or
// any other character.  The reference differs for two rare kinds of character: IUPAC ambiguity
// letters are KEPT (COMP_MAP, kstream.py:11-18: a surviving, N-free window holding one yields
// itself and its letter-wise reverse complement, kstream.py:644-677), and a character outside
// COMP_MAP raises KeyError in _get_complement for the first surviving window that holds one
// (kstream.py:658; the window is walked from its END, so the last such character of that
// window is the one reported).  Returns the number of window STARTS (ascending = stream order)
// of surviving, N-free windows with an ambiguity letter; writes up to cap of them.  A KeyError
// situation returns KR_ERR_KEY with *bad_char = the character as the reference would report it
// (after the soft-mask mapping).  A byte >= 0x80 inside a candidate window returns
// KR_ERR_HOST: Python's str.upper() / isupper() semantics for Latin-1 letters are left to the
// host layer (krisp_amd/fasta.py does the same scan in Python then).
// ----------------------------------------------------------------------------
static inline bool comp_key(uint8_t c) {
    switch (c) {
    case 'A': case 'T': case 'a': case 't': case 'G': case 'C': case 'g': case 'c': case 'R': case 'Y': case 'r':
    case 'y': case 'M': case 'K': case 'm': case 'k': case 'S': case 'W': case 's': case 'w': case 'B': case 'V':
    case 'b': case 'v': case 'D': case 'H': case 'd': case 'h': case 'N': case 'n': return true;
    default: return false;
    }
}
static inline bool iupac_letter(uint8_t c) {
    switch (c) {
    case 'R': case 'Y': case 'M': case 'K': case 'S': case 'W': case 'B': case 'V': case 'D': case 'H':
    case 'r': case 'y': case 'm': case 'k': case 's': case 'w': case 'b': case 'v': case 'd': case 'h': return true;
    default: return false;
    }
}

int64_t kr_scan_special(const uint8_t* bases, size_t n, int k, int omit_soft, uint64_t* starts, size_t cap,
                        int* bad_char) {
    if ((!bases && n) || k < 1) return KR_ERR_PARAM;
    if (bad_char) *bad_char = 0;
    int64_t nout = 0;
    size_t rec_lo = 0;
    while (rec_lo <= n) {
        size_t rec_hi = rec_lo;
        while (rec_hi < n && bases[rec_hi] != '\n') rec_hi++;
        // windows of this record that hold a character outside ACGTNacgtn
        size_t next_ok = rec_lo;            // first start not yet examined
        for (size_t p = rec_lo; p < rec_hi; p++) {
            const uint8_t c = bases[p];
            if (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N' || c == 'a' || c == 'c' || c == 'g' ||
                c == 't' || c == 'n')
                continue;
            if (rec_hi - rec_lo < (size_t)k) break;
            size_t s0 = p + 1 >= (size_t)k ? p + 1 - (size_t)k : 0;
            if (s0 < rec_lo) s0 = rec_lo;
            if (s0 < next_ok) s0 = next_ok;
            const size_t s1 = std::min(p, rec_hi - (size_t)k);
            for (size_t s = s0; s <= s1; s++) {
                const uint8_t* w = bases + s;
                bool lower = false, upper = false, has_n = false, iupac = false;
                for (int i = 0; i < k; i++) {
                    const uint8_t ch = w[i];
                    if (ch >= 0x80) return KR_ERR_HOST;
                    lower |= (ch >= 'a' && ch <= 'z');
                    upper |= (ch >= 'A' && ch <= 'Z');
                }
                if (omit_soft && (lower || !upper)) continue;       // str.isupper() is false (kstream.py:749)
                for (int i = k - 1; i >= 0; i--) {                   // reversed(w), after w.upper() when mapping
                    uint8_t ch = w[i];
                    if (!omit_soft && ch >= 'a' && ch <= 'z') ch -= 32;
                    if (!comp_key(ch)) {
                        if (bad_char) *bad_char = ch;
                        return KR_ERR_KEY;
                    }
                    has_n |= (ch == 'N' || ch == 'n');
                    iupac |= iupac_letter(ch);
                }
                if (has_n || !iupac) continue;
                if (starts && (size_t)nout < cap) starts[nout] = (uint64_t)s;
                nout++;
            }
            next_ok = s1 + 1;
        }
        rec_lo = rec_hi + 1;
    }
    return nout;
}


// ----------------------------------------------------------------------------
// host side: the final text from survivor records (SURVEY 8f rank 2; Amplicon.py:523-671 and
// outputAlignments.py:26-162 at --cores 1) -- the CSV and the alignment blocks of every group, written as bytes in
// one pass over the records: no object per Amplicon, no string per label list.  krisp_amd/amplicon.py holds the
// restatement of the reference (groups_from_records + render) this must equal byte for byte; the tests run both.
// Scope: records of packed keys (plain ACGT), DNA.  Anything else (IUPAC members, RNA, long amplicons cut from the
// genomes' text) stays with the general path; KR_ERR_HOST = "a group this code does not take" (the caller falls back).
//   recs       (key, genome, count), ordered by (key, label id of the genome)
//   label_of   genome id -> label id = rank of the genome's label among the DISTINCT labels in string order
//              (genomes whose file names collapse to one label share an id, as they share the label in the reference)
//   label_in   per label id: 1 = ingroup; NULL = no outgroup was given (krisp_fasta.py:284: ingroup = None)
// The two texts are malloc'ed; free them with kr_text_free.  Returns the number of groups.
// ----------------------------------------------------------------------------
void kr_text_free(void* p) { free(p); }

// The renderer proper, over any source of members in (group, sequence, label id) order -- packed records
// (kr_render_records) or window texts cut from the genomes (kr_render_windows: amplicons longer than one key):
//   src.n                      members
//   src.same_group(i, j)       members i and j share (left,right)
//   src.same_seq(i, j)         ... and the diagnostic part
//   src.load(i, out)           the base codes 0..3 of member i, position by position of the line left|diag|right
//   src.genome(i), src.count(i)
extern "C++" {
// the groups of the members [m0, m1) (m0 and m1 at group boundaries) appended to C (CSV rows) and A (alignment blocks);
// returns the number of groups or a negative code
template <class Src>
static int64_t render_range(const Src& src, size_t m0, size_t m1, int L, int D, int R, const uint32_t* label_of, size_t n_genomes,
                            const char* const* label_text, size_t n_labels, const uint8_t* label_in, int dot, char rna_t,
                            std::string& C, std::string& A) {
    const int k = L + D + R;
    const size_t n = m1;
    const char ACGT[5] = {'A', 'C', 'G', rna_t, 0};
    // 4-bit base set -> IUPAC letter (Amplicon.py:10-12 over Biopython's table; the full set reads N)
    static const char IUPAC[] = "?ACMGRSVTWYHKDBN";
    struct Pair { uint32_t lab, cnt; };
    struct Amp { size_t rep, p0, p1; bool has_in, has_out; };
    {
        C.reserve(C.size() + 64 + ((n - m0) / 2) * (size_t)(k + 3));
        A.reserve(A.size() + (n - m0) * (size_t)(k + 24));
        std::vector<Pair> pairs;
        std::vector<Amp> amps;
        std::vector<uint8_t> codes;         // the base codes of the group's sequences, k per Amplicon (loaded once: every loop below walks them)
        std::vector<uint32_t> rows;
        std::vector<std::string> lines;
        std::string br, field[3];
        // the Amplicon's label list as Python compares it: a list of names with multiplicity, element by element,
        // the shorter list first when it is a prefix of the other (Amplicon.py:605 sorts rows by this)
        auto less_labels = [&](const Amp& a, const Amp& b) {
            size_t i = a.p0, j = b.p0;
            uint32_t ca = i < a.p1 ? pairs[i].cnt : 0, cb = j < b.p1 ? pairs[j].cnt : 0;
            for (;;) {
                if (i == a.p1 || j == b.p1) return i == a.p1 && j != b.p1;
                if (pairs[i].lab != pairs[j].lab) return pairs[i].lab < pairs[j].lab;
                const uint32_t m = std::min(ca, cb);
                ca -= m;
                cb -= m;
                if (ca == 0 && ++i < a.p1) ca = pairs[i].cnt;
                if (cb == 0 && ++j < b.p1) cb = pairs[j].cnt;
            }
        };
        int64_t ngroups = 0;
        size_t i = m0;
        while (i < n) {
            // ---- one group: the members that share the (left,right) prefix
            const size_t g0 = i;
            pairs.clear();
            amps.clear();
            size_t j = i;
            while (j < n && src.same_group(g0, j)) {
                Amp a{j, pairs.size(), 0, false, false};
                uint32_t prev = 0;
                bool first = true;
                while (j < n && src.same_group(g0, j) && src.same_seq(a.rep, j)) {
                    if (src.genome(j) >= n_genomes) return KR_ERR_PARAM;
                    const uint32_t lab = label_of[src.genome(j)];
                    if (lab >= n_labels || (!first && lab < prev)) return KR_ERR_PARAM;        // (not in (sequence, label) order)
                    if (!first && lab == prev) pairs.back().cnt += src.count(j);
                    else pairs.push_back(Pair{lab, src.count(j)});
                    if (label_in) { if (label_in[lab]) a.has_in = true; else a.has_out = true; }
                    prev = lab;
                    first = false;
                    j++;
                }
                a.p1 = pairs.size();
                if (!amps.empty() && src.seq_less(a.rep, amps.back().rep)) return KR_ERR_PARAM;
                amps.push_back(a);
            }
            i = j;
            ngroups++;
            const size_t na = amps.size();
            codes.resize(na * (size_t)k);
            for (size_t q = 0; q < na; q++) src.load(amps[q].rep, codes.data() + q * (size_t)k);
            // ---- rows: stable by label list, then the ingroup-carrying ones first (Amplicon.py:602-612)
            rows.resize(na);
            for (size_t q = 0; q < na; q++) rows[q] = (uint32_t)q;
            if (na > 1) {
                std::stable_sort(rows.begin(), rows.end(), [&](uint32_t x, uint32_t y) { return less_labels(amps[x], amps[y]); });
                if (label_in) std::stable_partition(rows.begin(), rows.end(), [&](uint32_t x) { return amps[x].has_in; });
            }
            lines.resize(na);
            for (size_t q = 0; q < na; q++) {
                const Amp& a = amps[rows[q]];
                std::string& s = lines[q];
                s.clear();
                {
                    const uint8_t* cq = codes.data() + (size_t)rows[q] * (size_t)k;
                    s.resize((size_t)k);
                    for (int b = 0; b < k; b++) s[(size_t)b] = ACGT[cq[b]];
                }
                s += " : ";
                for (size_t p = a.p0; p < a.p1; p++) {          // Amplicon.py:170-187: name or name(count), ';' joined
                    if (p > a.p0) s.push_back(';');
                    s += label_text[pairs[p].lab];
                    if (pairs[p].cnt != 1) { s.push_back('('); s += std::to_string(pairs[p].cnt); s.push_back(')'); }
                }
            }
            if (dot) {
                // Amplicon.py:616-628: below the top row a character equal to the top row's, inside the sequence, is a dot
                A += lines[0];
                for (size_t q = 1; q < na; q++) {
                    A.push_back('\n');
                    const std::string &t = lines[q], &top = lines[0];
                    for (size_t x = 0; x < t.size(); x++) A.push_back((x < (size_t)k && x < top.size() && t[x] == top[x]) ? '.' : t[x]);
                }
            } else {
                for (size_t q = 0; q < na; q++) { A += lines[q]; A.push_back('\n'); }
                // the bracket line (Amplicon.py:523-540): '*' where the sequences differ, '#' where no ingroup base is an outgroup base
                br.assign(L > 0 ? (size_t)(L - 1) : 0, ' ');
                br.push_back('{');
                br.append((size_t)D, '-');
                br.push_back('}');
                for (int col = 0; col < D; col++) {
                    unsigned all = 0, ins = 0, outs = 0;
                    for (size_t q = 0; q < na; q++) {
                        const Amp& a = amps[q];
                        const unsigned bit = 1u << codes[q * (size_t)k + (size_t)(L + col)];
                        all |= bit;
                        if (a.has_in) ins |= bit;
                        if (a.has_out) outs |= bit;
                    }
                    if (all & (all - 1)) br[(size_t)(L + col)] = '*';
                    if (label_in && !(ins & outs)) br[(size_t)(L + col)] = '#';
                }
                A += br;
            }
            A += "\n\n";
            // ---- the CSV row: IUPAC consensus of the Amplicons whose labels are all ingroup (of all of them when there
            //      is one, or no ingroup was given; Amplicon.py:550-558, 663-671)
            for (int f = 0; f < 3; f++) field[f].clear();
            const bool take_all = na == 1 || !label_in;
            size_t nq = 0;
            for (const Amp& a : amps) nq += (take_all || !a.has_out) ? 1 : 0;
            if (nq == 0) return KR_ERR_HOST;        // (no row qualifies: the reference raises here; the general path reproduces that)
            for (int f = 0; f < 3; f++) {
                const int len = f == 0 ? L : (f == 1 ? D : R), off = f == 0 ? 0 : (f == 1 ? L : L + D);
                bool varies = false, has_t = false;
                for (int col = 0; col < len; col++) {
                    unsigned set = 0;
                    for (size_t q = 0; q < na; q++)
                        if (take_all || !amps[q].has_out) set |= 1u << codes[q * (size_t)k + (size_t)(off + col)];
                    varies = varies || (set & (set - 1));
                    has_t = has_t || (set & 8u);
                    char ch = IUPAC[set & 15u];
                    if (ch == 'T') ch = rna_t;
                    field[f].push_back(ch);
                }
                // (RNA: the reference's consensus table has no U -- a field whose sequences differ and hold one raises
                // KeyError there, Amplicon.py:65; the general path reproduces that)
                if (rna_t != 'T' && varies && has_t) return KR_ERR_HOST;
            }
            C += field[0]; C.push_back(','); C += field[1]; C.push_back(','); C += field[2]; C.push_back('\n');
        }
        return ngroups;
    }
}

// all members: large results are cut at group boundaries into pieces rendered side by side on host threads (the text of
// 10^6 groups is hundreds of megabytes), the pieces' texts joined in order
template <class Src>
static int64_t render_core(const Src& src, int L, int D, int R, const uint32_t* label_of, size_t n_genomes,
                           const char* const* label_text, size_t n_labels, const uint8_t* label_in, int dot, char rna_t,
                           char** csv, size_t* csv_len, char** align, size_t* align_len) {
    *csv = *align = nullptr;
    *csv_len = *align_len = 0;
    const size_t n = src.n;
    try {
        const char* e = getenv("KRISP_RENDER_THREADS");
        size_t nt = e ? (size_t)std::max(1, atoi(e)) : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
        nt = std::max<size_t>(1, std::min(nt, n / 20000));
        std::vector<size_t> cut(nt + 1, n);
        cut[0] = 0;
        for (size_t t = 1; t < nt; t++) {
            size_t b = std::max(cut[t - 1], t * n / nt);
            while (b > 0 && b < n && src.same_group(b - 1, b)) b++;
            cut[t] = b;
        }
        std::vector<std::string> Cs(nt), As(nt);
        std::vector<int64_t> res(nt, 0);
        auto work = [&](size_t t) {
            try {
                res[t] = cut[t] < cut[t + 1] ? render_range(src, cut[t], cut[t + 1], L, D, R, label_of, n_genomes, label_text, n_labels,
                                                            label_in, dot, rna_t, Cs[t], As[t]) : 0;
            } catch (const std::bad_alloc&) {
                res[t] = KR_ERR_CAPACITY;
            }
        };
        if (nt == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (size_t t = 0; t < nt; t++)
                if (!kr_spawn(th, work, t)) work(t);        // (no thread to be had: this one does the piece)
            for (auto& x : th) x.join();
        }
        int64_t ngroups = 0;
        static const char HEADER[] = "left_seq,diag_seq,right_seq\n";
        size_t cl = sizeof HEADER - 1, al = 0;
        for (size_t t = 0; t < nt; t++) {
            if (res[t] < 0) return res[t];
            ngroups += res[t];
            cl += Cs[t].size();
            al += As[t].size();
        }
        *csv = (char*)malloc(cl + 1);
        *align = (char*)malloc(al + 1);
        if (!*csv || !*align) { free(*csv); free(*align); *csv = *align = nullptr; return KR_ERR_CAPACITY; }
        memcpy(*csv, HEADER, sizeof HEADER - 1);
        size_t co = sizeof HEADER - 1, ao = 0;
        for (size_t t = 0; t < nt; t++) {
            memcpy(*csv + co, Cs[t].data(), Cs[t].size());
            co += Cs[t].size();
            memcpy(*align + ao, As[t].data(), As[t].size());
            ao += As[t].size();
        }
        *csv_len = cl;
        *align_len = al;
        return ngroups;
    } catch (const std::bad_alloc&) {
        return KR_ERR_CAPACITY;
    }
}

// members = packed records, key = left|right|diag
struct RecordSrc {
    const kr_record* recs;
    size_t n;
    int L, D, R;
    uint64_t pmask;
    bool same_group(size_t i, size_t j) const { return ((recs[i].key ^ recs[j].key) & pmask) == 0; }
    bool same_seq(size_t i, size_t j) const { return recs[i].key == recs[j].key; }
    bool seq_less(size_t i, size_t j) const { return recs[i].key < recs[j].key; }
    int code(size_t i, int pos) const {           // line position -> base of the key
        const int b = pos < L ? pos : (pos < L + D ? L + R + (pos - L) : L + (pos - L - D));
        return (int)((recs[i].key >> (62 - 2 * b)) & 3u);
    }
    void load(size_t i, uint8_t* out) const {
        for (int pos = 0; pos < L + D + R; pos++) out[pos] = (uint8_t)code(i, pos);
    }
    uint32_t genome(size_t i) const { return recs[i].genome; }
    uint32_t count(size_t i) const { return recs[i].count; }
};

// members = window texts (k letters of ACGT each, line order), walked through `order`
struct WindowSrc {
    const uint8_t* rows;
    const uint32_t* gen;
    const uint32_t* order;
    size_t n;
    int L, D, R, k;
    const uint8_t* row(size_t i) const { return rows + (size_t)order[i] * (size_t)k; }
    bool same_group(size_t i, size_t j) const {
        const uint8_t *a = row(i), *b = row(j);
        return memcmp(a, b, (size_t)L) == 0 && memcmp(a + L + D, b + L + D, (size_t)R) == 0;
    }
    bool same_seq(size_t i, size_t j) const { return memcmp(row(i) + L, row(j) + L, (size_t)D) == 0; }
    bool seq_less(size_t i, size_t j) const { return memcmp(row(i) + L, row(j) + L, (size_t)D) < 0; }
    int code(size_t i, int pos) const {
        const uint8_t ch = row(i)[pos];
        return ch == 'A' ? 0 : (ch == 'C' ? 1 : (ch == 'G' ? 2 : 3));
    }
    void load(size_t i, uint8_t* out) const {     // (A C G T differ in bits 1-2 of their ASCII codes: 0 1 3 2 -> 0 1 2 3)
        const uint8_t* r = row(i);
        for (int pos = 0; pos < k; pos++) { const uint8_t x = (uint8_t)((r[pos] >> 1) & 3u); out[pos] = (uint8_t)(x ^ (x >> 1)); }
    }
    uint32_t genome(size_t i) const { return gen[order[i]]; }
    uint32_t count(size_t) const { return 1; }
};
}   // extern "C++"

int64_t kr_render_records(const kr_record* recs, size_t n, int L, int D, int R, const uint32_t* label_of,
                          size_t n_genomes, const char* const* label_text, size_t n_labels, const uint8_t* label_in,
                          int dot, char** csv, size_t* csv_len, char** align, size_t* align_len) {
    if (!csv || !csv_len || !align || !align_len || (n && (!recs || !label_of || !label_text))) return KR_ERR_PARAM;
    const int k = L + D + R;
    if (L < 0 || D < 0 || R < 0 || k < 1 || k > 32) return KR_ERR_PARAM;
    const uint64_t pmask = (L + R) >= 32 ? ~0ull : ((L + R) == 0 ? 0ull : (~0ull << (64 - 2 * (L + R))));
    const RecordSrc src{recs, n, L, D, R, pmask};
    return render_core(src, L, D, R, label_of, n_genomes, label_text, n_labels, label_in, dot, 'T', csv, csv_len, align, align_len);
}

// The same text from the member windows of long amplicons (kr_wide_run's hits cut by kr_wide_fetch_windows): rows = n
// windows of k = L + D + R letters (ACGT, line order left|diag|right), cand[i] = the group number of row i (rows of a
// group adjacent, as kr_wide_fetch returns the hits), genome[i] = its genome's index into label_of.  Orders the groups
// by (left, right), the members of a group by (diag, label) -- the order of the reference's merged file -- and
// renders as kr_render_records does.  rna != 0: T is written as U (kstream.py:585-615 maps the output back).
int64_t kr_render_windows(const uint8_t* rows, size_t n, int L, int D, int R, const uint32_t* cand, const uint32_t* genome,
                          const uint32_t* label_of, size_t n_genomes, const char* const* label_text, size_t n_labels,
                          const uint8_t* label_in, int dot, int rna, char** csv, size_t* csv_len, char** align,
                          size_t* align_len) {
    if (!csv || !csv_len || !align || !align_len || (n && (!rows || !cand || !genome || !label_of || !label_text))) return KR_ERR_PARAM;
    const int k = L + D + R;
    if (L < 0 || D < 0 || R < 0 || k < 1 || n >= 0xFFFFFFFFull) return KR_ERR_PARAM;
    try {
        // rows by group number.  KR_WIDE_HITS order keeps a group and its mirror (bit 31) in one region and the regions in
        // ascending number: then a region is split by that bit in place; any other order takes a stable LSD radix sort of
        // the row indices (two 16-bit digits)
        std::vector<uint32_t> idx(n), tmp;
        bool regions = true;
        for (size_t i = 1; i < n && regions; i++) regions = (cand[i] & 0x7FFFFFFFu) >= (cand[i - 1] & 0x7FFFFFFFu);
        if (regions) {
            for (size_t i = 0; i < n;) {
                size_t j = i + 1;
                const uint32_t c0 = cand[i] & 0x7FFFFFFFu;
                while (j < n && (cand[j] & 0x7FFFFFFFu) == c0) j++;
                size_t at = i;
                for (size_t q = i; q < j; q++) if (!(cand[q] >> 31)) idx[at++] = (uint32_t)q;
                for (size_t q = i; q < j; q++) if (cand[q] >> 31) idx[at++] = (uint32_t)q;
                i = j;
            }
        } else {
            tmp.resize(n);
            for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
            for (int pass = 0; pass < 2; pass++) {
                std::vector<size_t> cnt(65537, 0);
                const int sh = 16 * pass;
                for (size_t i = 0; i < n; i++) cnt[((cand[idx[i]] >> sh) & 0xFFFFu) + 1]++;
                for (size_t d = 0; d < 65536; d++) cnt[d + 1] += cnt[d];
                for (size_t i = 0; i < n; i++) tmp[cnt[(cand[idx[i]] >> sh) & 0xFFFFu]++] = idx[i];
                idx.swap(tmp);
            }
        }
        // groups = runs of equal cand, ordered by (left, right): a packed prefix of the flanks decides most compares
        struct Grp { uint64_t pre; uint32_t lo, hi; };
        std::vector<Grp> grp;
        for (size_t i = 0; i < n;) {
            size_t j = i + 1;
            while (j < n && cand[idx[j]] == cand[idx[i]]) j++;
            grp.push_back(Grp{0, (uint32_t)i, (uint32_t)j});
            i = j;
        }
        {
            const char* e = getenv("KRISP_RENDER_THREADS");
            size_t nt = e ? (size_t)std::max(1, atoi(e)) : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
            nt = std::max<size_t>(1, std::min(nt, grp.size() / 4096));
            auto work = [&](size_t t) {
                for (size_t g = t * grp.size() / nt; g < (t + 1) * grp.size() / nt; g++) {
                    const uint8_t* x = rows + (size_t)idx[grp[g].lo] * k;
                    uint64_t pre = 0;
                    int nb = 0;
                    for (int q = 0; q < L && nb < 32; q++, nb++) { const uint64_t c2 = (x[q] >> 1) & 3u; pre = (pre << 2) | (c2 ^ (c2 >> 1)); }
                    for (int q = 0; q < R && nb < 32; q++, nb++) { const uint64_t c2 = (x[L + D + q] >> 1) & 3u; pre = (pre << 2) | (c2 ^ (c2 >> 1)); }
                    grp[g].pre = pre << (2 * (32 - nb));
                }
            };
            if (nt == 1) work(0);
            else {
                std::vector<std::thread> th;
                for (size_t t = 0; t < nt; t++)
                    if (!kr_spawn(th, work, t)) work(t);    // (no thread to be had: this one does the piece)
                for (auto& x : th) x.join();
            }
        }
        auto flank_cmp = [&](const Grp& a, const Grp& b) {
            if (a.pre != b.pre) return a.pre < b.pre ? -1 : 1;
            const uint8_t *x = rows + (size_t)idx[a.lo] * k, *y = rows + (size_t)idx[b.lo] * k;
            const int c1 = memcmp(x, y, (size_t)L);
            return c1 ? c1 : memcmp(x + L + D, y + L + D, (size_t)R);
        };
        std::sort(grp.begin(), grp.end(), [&](const Grp& a, const Grp& b) { return flank_cmp(a, b) < 0; });
        for (size_t g = 1; g < grp.size(); g++)
            if (flank_cmp(grp[g - 1], grp[g]) == 0) return KR_ERR_HOST;      // (one (left,right) under two group numbers)
        // the members of every group in (diag, label) order, the groups in their sorted order: filled and sorted side by
        // side on host threads (10^7 members in 10^6 groups: the one-threaded form took as long as the rendering)
        std::vector<size_t> goff(grp.size() + 1, 0);
        for (size_t g = 0; g < grp.size(); g++) goff[g + 1] = goff[g] + (grp[g].hi - grp[g].lo);
        std::vector<uint32_t> order(n);
        std::atomic<bool> bad_genome{false};
        {
            const char* e = getenv("KRISP_RENDER_THREADS");
            size_t nt = e ? (size_t)std::max(1, atoi(e)) : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
            nt = std::max<size_t>(1, std::min(nt, grp.size() / 4096));
            auto work = [&](size_t t) {
                for (size_t g = t * grp.size() / nt; g < (t + 1) * grp.size() / nt; g++) {
                    uint32_t* o = order.data() + goff[g];
                    const uint32_t m = grp[g].hi - grp[g].lo;
                    for (uint32_t i = 0; i < m; i++) {
                        o[i] = idx[grp[g].lo + i];
                        if (genome[o[i]] >= n_genomes) { bad_genome = true; return; }
                    }
                    std::sort(o, o + m, [&](uint32_t x, uint32_t y) {
                        const int c1 = memcmp(rows + (size_t)x * k + L, rows + (size_t)y * k + L, (size_t)D);
                        if (c1) return c1 < 0;
                        const uint32_t lx = label_of[genome[x]], ly = label_of[genome[y]];
                        return lx != ly ? lx < ly : x < y;
                    });
                }
            };
            if (nt == 1) work(0);
            else {
                std::vector<std::thread> th;
                for (size_t t = 0; t < nt; t++)
                    if (!kr_spawn(th, work, t)) work(t);    // (no thread to be had: this one does the piece)
                for (auto& x : th) x.join();
            }
        }
        if (bad_genome) return KR_ERR_PARAM;
        const WindowSrc src{rows, genome, order.data(), n, L, D, R, k};
        return render_core(src, L, D, R, label_of, n_genomes, label_text, n_labels, label_in, dot, rna ? 'U' : 'T', csv, csv_len,
                           align, align_len);
    } catch (const std::bad_alloc&) {
        return KR_ERR_CAPACITY;
    }
}

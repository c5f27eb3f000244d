// fastx_parse.cpp — the record parser of the host readers (fastx_read.cpp, fastx_index.cpp, fastx_stream.cpp): a range of
// text into an FxChunk, a text in pieces side by side, the name hash, kseq's stale comment / quality buffers over pieces.
#include "host_ingest_internal.h"

#include <immintrin.h>

using namespace crass;

// ---- FASTA/FASTQ reader: kseq_read record semantics (kseq.cpp:171-226) as driven by
// searchFile (libcrispr.cpp:96-131).  The whole (decompressed) file is parsed from memory, in parallel:
// the buffer is cut at guessed record starts, every piece is parsed by the same byte-exact state machine, and
// the pieces are accepted only if each one ends exactly where the next one began (otherwise — odd layouts,
// truncated files — the file is parsed again in one piece).  The reference's reader is single-threaded and
// byte-at-a-time; on the 800 MB / 5 M-read FASTA of tools/e2e_cli.sh it was 99 % of the wall time.
static bool is_space(int c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// L bases -> ceil(L/16) words (A0 C1 G2 T3, base i in bits 2(i%16) of word i/16); true when a byte outside ACGT was met (it
// packs as A: the read is an exception read and its slot's content is ignored).  Eight bases per step: the code of a letter is
// ((c >> 1) & 3) with the two upper values exchanged, the letter a code stands for is rebuilt (0x41 + 2 b0 + 6 b1 + 11 b0 b1)
// and compared with what was read
// 32 bases per step (AVX2, where the CPU has it): the code as above, checked by looking the letter up again (pshufb) and comparing;
// four codes become a byte through two multiply-adds (t0 + 4 t1, then + 16 (t2 + 4 t3)), the bytes of a 128-bit half are its word.
// The parsers of an index are bound by CPU seconds, not threads (a 16-CPU quota on a 256-thread host): packing was a quarter of
// the 130 ns they spent per 150-base record.
__attribute__((target("avx2"))) static inline uint32_t pack_bases_avx2(const uint8_t *s, uint32_t L, uint32_t *w, uint64_t &bad)
{
    const __m256i three = _mm256_set1_epi8(3), one = _mm256_set1_epi8(1);
    const __m256i letters = _mm256_setr_epi8('A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    const __m256i pick = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    __m256i ok = _mm256_set1_epi8(-1);
    uint32_t k = 0;
    for (; k + 32 <= L; k += 32) {
        const __m256i x = _mm256_loadu_si256((const __m256i *)(s + k));
        __m256i t = _mm256_and_si256(_mm256_srli_epi16(x, 1), three);
        t = _mm256_xor_si256(t, _mm256_and_si256(_mm256_srli_epi16(t, 1), one));
        ok = _mm256_and_si256(ok, _mm256_cmpeq_epi8(_mm256_shuffle_epi8(letters, t), x));
        const __m256i p2 = _mm256_maddubs_epi16(t, _mm256_set1_epi16(0x0401));            // t0 + 4 t1 per 16-bit lane
        const __m256i p4 = _mm256_madd_epi16(p2, _mm256_set1_epi32(0x00100001));           // + 16 (t2 + 4 t3) per 32-bit lane
        const __m256i by = _mm256_shuffle_epi8(p4, pick);
        w[k >> 4] = (uint32_t)_mm256_cvtsi256_si32(by);
        w[(k >> 4) + 1] = (uint32_t)_mm256_extract_epi32(by, 4);
    }
    if (_mm256_movemask_epi8(ok) != -1) bad |= 1;
    return k;
}

// The common record's sequence line in ONE pass: 32 bytes are loaded, looked at for the line's end and packed (the line's length
// comes out of the same loads memchr would have made).  true: the line was pure ACGT up to a '\n' at p[*len] and its words have
// been appended to `words` (the tail past the last base is zero); false: anything else — a byte outside ACGT, no line end within
// `avail - 32` bytes — with `words` as it was: the caller's general path takes the record.
__attribute__((target("avx2"))) static inline bool pack_line_avx2(const uint8_t *p, size_t avail, GrowBuf<uint32_t> &words, size_t *len)
{
    alignas(32) static const uint8_t lane_mask[64] = {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
                                                      255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const __m256i three = _mm256_set1_epi8(3), one = _mm256_set1_epi8(1), nl = _mm256_set1_epi8('\n');
    const __m256i letters = _mm256_setr_epi8('A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    const __m256i pick = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    const size_t w0 = words.size();
    size_t k = 0;
    for (;; k += 32) {
        if (k + 32 > avail || k >= (1u << 30)) { words.resize(w0); return false; }
        const size_t wi = w0 + (k >> 4);
        if (wi + 2 > words.cap) { words.n = wi; words.grow(wi + 2); }
        const __m256i x = _mm256_loadu_si256((const __m256i *)(p + k));
        const uint32_t nlm = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(x, nl));
        __m256i t = _mm256_and_si256(_mm256_srli_epi16(x, 1), three);
        t = _mm256_xor_si256(t, _mm256_and_si256(_mm256_srli_epi16(t, 1), one));
        const uint32_t okm = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_shuffle_epi8(letters, t), x));
        uint32_t rem = 32;
        if (nlm) {
            rem = (uint32_t)__builtin_ctz(nlm);
            const uint32_t lm = (1u << rem) - 1u;
            if ((okm & lm) != lm) { words.resize(w0); return false; }
            t = _mm256_and_si256(t, _mm256_loadu_si256((const __m256i *)(lane_mask + 32 - rem)));
        } else if (okm != 0xFFFFFFFFu) { words.resize(w0); return false; }
        const __m256i p2 = _mm256_maddubs_epi16(t, _mm256_set1_epi16(0x0401));
        const __m256i p4 = _mm256_madd_epi16(p2, _mm256_set1_epi32(0x00100001));
        const __m256i by = _mm256_shuffle_epi8(p4, pick);
        words.p[wi] = (uint32_t)_mm256_cvtsi256_si32(by);
        words.p[wi + 1] = (uint32_t)_mm256_extract_epi32(by, 4);
        if (nlm) { *len = k + rem; words.n = w0 + (k + rem + 15) / 16; return true; }
    }
}

static inline bool pack_bases(const uint8_t *s, uint32_t L, uint32_t *w)
{
    uint64_t bad = 0;
    uint32_t k = 0;
    static const bool have_avx2 = __builtin_cpu_supports("avx2") && !getenv("CRASS_NO_AVX2");
    if (have_avx2 && L >= 32) k = pack_bases_avx2(s, L, w, bad);
    for (; k + 16 <= L; k += 16) {
        uint32_t word = 0;
        for (int half = 0; half < 2; half++) {
            uint64_t x;
            memcpy(&x, s + k + 8 * half, 8);
            uint64_t t = (x >> 1) & 0x0303030303030303ull;
            t ^= (t >> 1) & 0x0101010101010101ull;
            const uint64_t b0 = t & 0x0101010101010101ull, b1 = (t >> 1) & 0x0101010101010101ull, b01 = b0 & b1;
            const uint64_t recon = 0x4141414141414141ull + 2 * b0 + 6 * b1 + 11 * b01;
            bad |= recon ^ x;
            t = (t | (t >> 6)) & 0x000F000F000F000Full;
            t = (t | (t >> 12)) & 0x000000FF000000FFull;
            t = (t | (t >> 24)) & 0xFFFFull;
            word |= (uint32_t)t << (16 * half);
        }
        w[k >> 4] = word;
    }
    if (k < L) {
        const uint8_t *const lut = base_lut();
        uint32_t acc = 0, b = 0;
        for (uint32_t q = 0; k + q < L; q++) { const uint32_t cc = lut[s[k + q]]; b |= cc; acc |= (cc & 3u) << (2 * q); }
        w[k >> 4] = acc;
        if (b & 0x80u) bad |= 1;
    }
    return bad != 0;
}

// Parses the records whose header character ('>' / '@') lies in [start, limit).  `start` indexes a header
// character unless scan_first (then the parser looks for the first one, as kseq_read does at the beginning).
void crass::parse_range(const uint8_t *data, size_t n, size_t start, size_t limit, bool scan_first, FxChunk &o)
{
    size_t pos = start;
    int last_char = 0;
    if (!scan_first) { last_char = data[start]; pos = start + 1; }
    for (;;) {
        size_t hdr;
        if (last_char == 0) {
            while (pos < n && data[pos] != '>' && data[pos] != '@') pos++;
            if (pos >= n) { o.ended = true; o.last_ret = -1; o.next_start = n; return; }
            hdr = pos;
            if (hdr >= limit) { o.next_start = hdr; return; }
            last_char = data[pos++];
        } else {
            hdr = pos - 1;
            if (hdr >= limit) { o.next_start = hdr; return; }
        }
        if (pos >= n) { o.ended = true; o.last_ret = -1; o.next_start = n; return; }      // ks_getuntil < 0 at EOF
        size_t st = pos;
        if (pos + 16 <= n) {                              // (the name's end — the first isspace() byte — sixteen bytes at a look)
            const __m128i x = _mm_loadu_si128((const __m128i *)(data + pos));
            const __m128i sp = _mm_or_si128(_mm_cmpeq_epi8(x, _mm_set1_epi8(' ')),
                                            _mm_cmpeq_epi8(_mm_min_epu8(_mm_sub_epi8(x, _mm_set1_epi8('\t')), _mm_set1_epi8(4)), _mm_sub_epi8(x, _mm_set1_epi8('\t'))));
            const unsigned m = (unsigned)_mm_movemask_epi8(sp);
            pos += m ? (size_t)__builtin_ctz(m) : 16;
        }
        while (pos < n && !is_space(data[pos])) pos++;
        const size_t name_st = st, name_len = pos - st;
        int c = pos < n ? data[pos] : -1;
        pos++;
        bool own_c = false;
        size_t com_st = 0, com_len = 0;
        if (c != -1 && c != '\n') {
            st = pos;
            const void *nl = pos < n ? memchr(data + pos, '\n', n - pos) : nullptr;
            pos = nl ? (size_t)((const uint8_t *)nl - data) : n;
            com_st = st; com_len = std::min(pos, n) - st;
            own_c = true;
            pos++;
        }
        const size_t seq_base = o.seq.size();
        c = -1;
        // pack mode, the common record: the sequence on ONE line of pure ACGT with the next header (or the '+' line) right behind
        // it — packed straight from the mapping (pack_bases also tells whether a byte was anything else: then the general
        // path below takes the record from the same position, as it does for wrapped lines, the last record and odd spacing)
        bool packed_in_place = false;
        size_t fast_len = 0;
        const size_t words_base = o.words.size();       // (a record that turns out truncated takes its words back)
        static const bool line_avx2 = __builtin_cpu_supports("avx2") && !getenv("CRASS_NO_AVX2");
        if (o.pack && pos < n && line_avx2) {
            size_t len = 0;
            if (pack_line_avx2(data + pos, n - pos, o.words, &len)) {
                const size_t nx = pos + len + 1;
                if (len && nx < n && (data[nx] == '>' || data[nx] == '@' || data[nx] == '+')) { packed_in_place = true; fast_len = len; c = data[nx]; pos = nx + 1; }
                else o.words.resize(words_base);
            }
        } else if (o.pack && pos < n) {
            const uint8_t *p = data + pos;
            const void *nlp = memchr(p, '\n', n - pos);
            if (nlp) {
                const size_t len = (size_t)((const uint8_t *)nlp - p), nx = pos + len + 1;
                if (len && len < (1u << 30) && nx < n && (data[nx] == '>' || data[nx] == '@' || data[nx] == '+')) {
                    const size_t w0 = o.words.size(), nw = (len + 15) / 16;
                    o.words.resize(w0 + nw);
                    if (!pack_bases(p, (uint32_t)len, o.words.data() + w0)) { packed_in_place = true; fast_len = len; c = data[nx]; pos = nx + 1; }
                    else o.words.resize(w0);
                }
            }
        }
        while (!packed_in_place && pos < n) {
            // fast path: a run of sequence bytes up to the end of the line.  The line's end comes from memchr; the bytes before
            // it are then checked eight at a time against a table of the bytes that END such a run ('>', '+', '@', anything
            // outside 33..126) — a sequence line has none, and one that does is walked byte by byte as before
            const uint8_t *p = data + pos, *e = data + n;
            const uint8_t *q = p;
            {
                static const struct Stop { uint8_t t[256]; Stop() { for (int i = 0; i < 256; i++) t[i] = (i < 33 || i > 126 || i == '>' || i == '+' || i == '@') ? 1 : 0; } } stop;
                const void *nlp = memchr(p, '\n', (size_t)(e - p));
                const uint8_t *le = nlp ? (const uint8_t *)nlp : e;
                const uint8_t *x = p;
                uint32_t bad = 0;
                for (; x + 8 <= le; x += 8)
                    bad |= stop.t[x[0]] | stop.t[x[1]] | stop.t[x[2]] | stop.t[x[3]] | stop.t[x[4]] | stop.t[x[5]] | stop.t[x[6]] | stop.t[x[7]];
                for (; x < le; x++) bad |= stop.t[*x];
                if (!bad) q = le;
            }
            while (q < e && *q != '\n' && *q != '>' && *q != '+' && *q != '@' && *q >= 33 && *q <= 126) q++;
            if (q > p) { o.seq.insert(o.seq.end(), p, q); pos += (size_t)(q - p); if (pos >= n) break; }
            c = data[pos++];
            if (c == '>' || c == '+' || c == '@') break;
            if (c >= 33 && c <= 126) o.seq.push_back((uint8_t)c);       // isgraph
            c = -1;
        }
        const size_t sq_len = packed_in_place ? fast_len : o.seq.size() - seq_base;
        if (c == '>' || c == '@') last_char = c;
        bool own_q = false;
        const size_t qual_base = o.qual.size();
        if (c == '+') {
            const void *nl = pos < n ? memchr(data + pos, '\n', n - pos) : nullptr;
            if (!nl) { o.seq.resize(seq_base); o.words.resize(words_base); o.ended = true; o.last_ret = -2; o.next_start = n; return; }
            pos = (size_t)((const uint8_t *)nl - data) + 1;
            // `while ((c = ks_getc(ks)) != -1 && seq->qual.l < seq->seq.l)`: consumes one byte past the quality
            size_t ql = 0;
            // the common record: the quality string on ONE line, as long as the sequence, every byte in 33 .. 127 — checked eight
            // bytes at a time and taken as a block (pack mode: not taken at all); the byte behind it is the one kseq's loop consumes
            if (sq_len && pos + sq_len < n && data[pos + sq_len] == '\n') {
                const uint8_t *q = data + pos;
                const uint64_t H = 0x8080808080808080ull, L21 = 0x2121212121212121ull;
                uint64_t bad = 0;
                size_t i = 0;
                for (; i + 8 <= sq_len; i += 8) { uint64_t x; memcpy(&x, q + i, 8); bad |= (~((x | H) - L21) | x) & H; }
                for (; i < sq_len; i++) bad |= (uint64_t)(q[i] < 33 || q[i] > 127);
                if (!bad) {
                    if (!o.pack) o.qual.insert(o.qual.end(), q, q + sq_len);
                    ql = sq_len;
                    pos += sq_len + 1;
                }
            }
            if (sq_len == 0 && pos < n) pos++;                           // (an empty sequence: the loop's one look still consumes a byte)
            while (ql < sq_len && pos < n) {
                const int ch = data[pos++];
                if (ch >= 33 && ch <= 127) { o.qual.push_back((uint8_t)ch); ql++; }
                if (!(ql < sq_len)) { if (pos < n) pos++; break; }       // (... and one byte past the quality)
            }
            last_char = 0;
            if (ql != sq_len) { o.seq.resize(seq_base); o.qual.resize(qual_base); o.words.resize(words_base); o.ended = true; o.last_ret = -2; o.next_start = n; return; }
            own_q = true;
        }
        o.last_hdr = hdr;
        if (o.pack) {
            o.hdr_pos.push_back(hdr);                     // (the index's: the whole-file and streamed readers never read it — 8 bytes per record)
            if (!packed_in_place) {
                const size_t w0 = o.words.size(), nw = (sq_len + 15) / 16;
                o.words.resize(w0 + nw);
                if (pack_bases(o.seq.data() + seq_base, (uint32_t)sq_len, o.words.data() + w0)) {
                    o.exc_rec.push_back(o.len32.size());
                    o.exc_bytes.insert(o.exc_bytes.end(), o.seq.begin() + seq_base, o.seq.end());
                    o.exc_off.push_back(o.exc_bytes.size());
                }
                o.seq.resize(seq_base);
            }
            o.qual.resize(qual_base);
            o.v_seq += sq_len; o.v_name += name_len;
            o.name_h.push_back(name_hash(data + name_st, name_len));
            o.len32.push_back((uint32_t)sq_len); o.nlen32.push_back((uint32_t)name_len);
            if (own_c) o.pk_flags |= 1; else o.pk_flags &= (uint8_t)~4;
            if (own_q) o.pk_flags |= 2; else o.pk_flags &= (uint8_t)~8;
            o.pk_min_len = std::min<uint32_t>(o.pk_min_len, (uint32_t)sq_len);
        } else {
            o.name.insert(o.name.end(), data + name_st, data + name_st + name_len); o.name_end.push_back(o.name.size());
            o.seq_end.push_back(o.seq.size());
            if (own_c) o.comment.insert(o.comment.end(), data + com_st, data + com_st + com_len);
            o.comment_end.push_back(o.comment.size());
            o.qual_end.push_back(o.qual.size());
        }
        if (!o.pack) { o.own_c.push_back(own_c ? 1 : 0); o.own_q.push_back(own_q ? 1 : 0); }
        o.max_len = std::max<uint32_t>(o.max_len, (uint32_t)sq_len);
        if (c == -1 && pos >= n) { o.ended = true; o.last_ret = -1; o.next_start = n; return; }
    }
}

// first plausible record start at or after `from`: a line that starts with the file's header character
// (FASTQ: and whose line after next starts with '+', which tells a header from a quality line)
static size_t guess_start(const uint8_t *data, size_t n, size_t from, bool fastq)
{
    size_t p = from;
    while (p < n) {
        const void *nl = memchr(data + p, '\n', n - p);
        if (!nl) return n;
        const size_t cand = (size_t)((const uint8_t *)nl - data) + 1;
        if (cand >= n) return n;
        if (!fastq) { if (data[cand] == '>') return cand; }
        else if (data[cand] == '@') {
            const void *l1 = memchr(data + cand, '\n', n - cand);
            if (l1) {
                const size_t s2 = (size_t)((const uint8_t *)l1 - data) + 1;
                const void *l2 = s2 < n ? memchr(data + s2, '\n', n - s2) : nullptr;
                if (l2) { const size_t s3 = (size_t)((const uint8_t *)l2 - data) + 1; if (s3 < n && data[s3] == '+') return cand; }
            }
        }
        p = cand;
    }
    return n;
}

uint64_t crass::name_hash(const uint8_t *p, size_t n)
{
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (n * 0xD6E8FEB86659FD93ull);
    while (n >= 8) { uint64_t v; memcpy(&v, p, 8); h = (h ^ v) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; p += 8; n -= 8; }
    if (n) { uint64_t v = 0; memcpy(&v, p, n); h = (h ^ v) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 29; }
    return h ^ (h >> 31);
}

// the (decompressed) text d[0, n) cut into pieces at guessed record starts, every piece parsed by parse_range on its own thread;
// accepted only if each piece ends exactly where the next one began, else parsed again in one piece (exact by construction)
void crass::parse_pieces(const uint8_t *d, size_t n, std::vector<FxChunk> &ch, size_t piece_bytes, bool pack)
{
    size_t chunk_bytes = piece_bytes;
    if (const char *e = getenv("CRASS_FASTX_CHUNK")) chunk_bytes = (size_t)std::max(64ll, atoll(e));     // tests: force small pieces
    unsigned nt = (unsigned)std::min<size_t>(std::min<unsigned>(hw_threads(), 64u), n / chunk_bytes);
    if (getenv("CRASS_FASTX_SERIAL")) nt = 1;
    std::vector<size_t> starts{0};
    if (nt > 1) {
        size_t first = 0;
        while (first < n && d[first] != '>' && d[first] != '@') first++;
        const bool fastq = first < n && d[first] == '@';
        for (unsigned k = 1; k < nt; k++) {
            const size_t g = guess_start(d, n, std::max(starts.back(), (size_t)((unsigned __int128)n * k / nt)), fastq);
            if (g >= n) break;
            if (g > starts.back()) starts.push_back(g);
        }
    }
    ch.resize(starts.size());
    for (auto &c : ch) c.reset(pack);
    run_side_by_side(starts.size(), [&](size_t k) { parse_range(d, n, starts[k], k + 1 < starts.size() ? starts[k + 1] : n, k == 0, ch[k]); });
    if (starts.size() > 1) {
        bool ok = true;
        for (size_t k = 0; k + 1 < starts.size() && ok; k++) ok = !ch[k].ended && ch[k].next_start == starts[k + 1];
        if (!ok) {                                       // a guess was wrong or the stream ended early: one piece, exact
            ch.assign(1, FxChunk());
            ch[0].pack = pack;
            parse_range(d, n, 0, n, true, ch[0]);
        }
    }
}

// kseq's stale comment (or quality) buffers over the first n_rec records of the pieces ch[0 .. n_pieces), in order: a record that
// carries its own string replaces `stale`, and from the first such record on every record is handed the string last seen
// (libcrispr.cpp:124-131).  has[r] and off[r + 1] per record, the strings appended to `bytes`; (any, stale) come in as the records
// before these left them — empty at the start of a file — and go out for the records behind
void crass::stale_walk(const FxChunk *ch, size_t n_pieces, uint64_t n_rec, bool comment, bool &any, std::string &stale, uint8_t *has, uint64_t *off, std::vector<uint8_t> &bytes)
{
    uint64_t r = 0;
    for (size_t k = 0; k < n_pieces && r < n_rec; k++) {
        const FxChunk &c = ch[k];
        const std::vector<uint8_t> &src = comment ? c.comment : c.qual;
        const std::vector<uint64_t> &end = comment ? c.comment_end : c.qual_end;
        const std::vector<uint8_t> &own = comment ? c.own_c : c.own_q;
        for (size_t i = 0; i < c.n_rec() && r < n_rec; i++, r++) {
            if (own[i]) { const uint64_t b0 = i ? end[i - 1] : 0; stale.assign((const char *)src.data() + b0, end[i] - b0); any = true; }
            has[r] = any ? 1 : 0;
            if (any) bytes.insert(bytes.end(), stale.begin(), stale.end());
            off[r + 1] = bytes.size();
        }
    }
}

// gunzip_core.h — what the host function (gunzip.cpp), the kernels (gunzip.hip) and the engine (engine.cpp) share about inflating
// ONE plain gzip member (RFC 1952) chunk by chunk: pgzip.cpp's technique (one deflate stream entered at block starts found in
// its middle, bytes copied from the unknown 32 KB in front of a chunk carried as 16-bit markers and resolved afterwards, the
// result accepted only with the trailer's length and CRC-32), made wait-free: no chunk ever waits for another, every step is a
// pass of its own over all chunks.  Plain C++ with CRASS_HD, on top of inflate_core.h's tables, bit reader and CRC; every
// statement below runs on host and device alike.  Not part of the public ABI.
//
// The rule, over the deflate data d[0, dn) between header and trailer, cut into nc = max(1, dn / chunk_bytes) chunks with
// nominal bit starts nominal[k] = (dn k / nc) 8:
//   find     start[0] = 0; start[k] is the first bit p in [nominal[k], nominal[k+1]) with p + 64 < 8 dn that passes the test:
//            BFINAL 0, BTYPE 2, a dynamic header that parses completely, that block decodes, and the next block (of any type)
//            decodes too, both before nominal[k + kGzMaxSpan].  gz_survives is the cheap part of the test, a position at a time
//            (a lane each on the device); it never rejects what the whole test accepts
//   count    every chunk with a start decodes block by block, storing nothing; at each block boundary at bit `pos` it looks at
//            the one chunk j > k whose nominal range holds pos: start[j] == pos and text produced -> link j.  It also stops at
//            the final block's end (link END), and as UNFINISHED once it stands at or beyond nominal[k + kGzMaxSpan]
//   chain    (host) from chunk 0 along link; the prefix sum of the chain's text lengths is every chunk's place in the text
//   decode   the same bits again into 16-bit symbols: a byte, or 0x8000 | index into the 32 KB in front of the chunk
//   windows  the 32 KB in front of chain element i from element i - 1's last symbols and its window, in chain order
//   narrow   symbols to bytes through each element's window; per-element CRC-32 parts, combined with bz_crc_shift
//
// kGzMaxSpan = 32: a chunk gives up when it has gone through 32 chunks' worth of input without meeting a later chunk's start.
// zlib ends a block after at most 32 767 symbols (memLevel 9; 16 383 at the default 8), which for FASTA / FASTQ text is 30 to
// 50 KB of input and at most ~120 KB for text of any kind: 32 chunks of the smallest size (4096 bytes: 128 KB) get through such a
// block and reach the next one's start, so reason 12 is left to input without dynamic block starts (stored or fixed blocks
// throughout) and to blocks much longer than zlib writes.  With the default chunk a block is a fraction of one chunk.  The span
// also bounds what one wave decodes (nothing runs away on a pathological input) and keeps a run's bit offsets inside 32 bits:
// 32 chunks of less than 2 kGzMaxChunk bytes are less than 2^31 bits.
//
// Bounds: a run reads d[b0, b0 + n_in) only (in() answers 0 beyond, every taker checks over()); every loop iteration takes at
// least one input bit or ends; a decode run writes symbols [0, counted length) of its chunk only (put() checks).
#pragma once
#include "inflate_core.h"

namespace crass {

static const uint32_t kGzMaxSpan = 32;
static const uint64_t kGzMinChunk = 4096, kGzMaxChunk = 4ull << 20;
static const uint64_t kGzDefaultChunk = 256 * 1024;      // (see profiles/NOTES_r16.md)
static const uint32_t kGzWindow = 32768;
static const uint32_t kGzSlack = 1024;                    // input a run may read beyond its stop: a dynamic header is at most 563 bytes
static const uint64_t kGzNoStart = ~0ull;
// link[k]: a chunk index, or
enum GzLink : uint32_t { GZ_LINK_END = 0xFFFFFFFFu, GZ_LINK_UNFINISHED = 0xFFFFFFFEu, GZ_LINK_BAD = 0xFFFFFFFDu, GZ_LINK_NONE = 0xFFFFFFFCu };

struct GzGeom { uint64_t d_off, dn, nc; };               // the deflate data: file bytes [d_off, d_off + dn), nc chunks

CRASS_HD inline uint64_t gz_chunk_bytes(uint64_t c)
{
    if (c == 0) c = kGzDefaultChunk;
    return c < kGzMinChunk ? kGzMinChunk : c > kGzMaxChunk ? kGzMaxChunk : c;
}
CRASS_HD inline uint64_t gz_n_chunks(uint64_t dn, uint64_t chunk_bytes) { const uint64_t n = dn / gz_chunk_bytes(chunk_bytes); return n ? n : 1; }
CRASS_HD inline uint64_t gz_nominal(const GzGeom &G, uint64_t k) { return k >= G.nc ? G.dn * 8 : (G.dn * k / G.nc) * 8; }
// the chunk whose nominal range holds bit pos < 8 dn
CRASS_HD inline uint64_t gz_chunk_of(const GzGeom &G, uint64_t pos)
{
    uint64_t j = (pos >> 3) * G.nc / G.dn;
    if (j >= G.nc) j = G.nc - 1;
    while (j + 1 < G.nc && gz_nominal(G, j + 1) <= pos) j++;
    while (j > 0 && gz_nominal(G, j) > pos) j--;
    return j;
}

// ---- the gzip header and trailer (host only: a few bytes) ----
struct GzMember { GzGeom G; uint32_t crc, isize; };
// b[0, n_head) are the first bytes of the n the file has (all of them on the host; the engine fetches a piece from the device
// and comes again with more when the answer is -1), t its last 8.  BZ_OK, or BZ_NOT_GZIP: the magic, the method, a reserved
// flag, the header CRC, or a header that leaves no room for the trailer
inline int32_t gz_parse_member(const uint8_t *b, uint64_t n_head, const uint8_t *t, uint64_t n, uint64_t chunk_bytes, GzMember *M)
{
    if (n < 18) return BZ_NOT_GZIP;
    const uint64_t end = n - 8;
    if (n_head > end) n_head = end;
    if (n_head < 10) return -1;
    if (b[0] != 0x1F || b[1] != 0x8B || b[2] != 8 || (b[3] & 0xE0)) return BZ_NOT_GZIP;
    const uint32_t flg = b[3];
    uint64_t d = 10;
    if (flg & 4) {
        if (d + 2 > end) return BZ_NOT_GZIP;
        if (d + 2 > n_head) return -1;
        d += 2 + ((uint64_t)b[10] | (uint64_t)b[11] << 8);
        if (d > end) return BZ_NOT_GZIP;
    }
    for (int bit = 3; bit <= 4; bit++)
        if (flg & (1u << bit)) {
            for (; d < end; d++) {
                if (d >= n_head) return -1;
                if (!b[d]) break;
            }
            if (d >= end) return BZ_NOT_GZIP;
            d++;
        }
    if (flg & 2) {
        if (d + 2 > end) return BZ_NOT_GZIP;
        if (d + 2 > n_head) return -1;
        uint32_t c = 0xFFFFFFFFu;
        for (uint64_t i = 0; i < d; i++) c = bz_crc_entry((c ^ b[i]) & 0xFFu) ^ (c >> 8);
        c = ~c;
        if ((c & 0xFFFFu) != ((uint32_t)b[d] | (uint32_t)b[d + 1] << 8)) return BZ_NOT_GZIP;
        d += 2;
    }
    M->G.d_off = d; M->G.dn = end - d; M->G.nc = gz_n_chunks(M->G.dn, chunk_bytes);
    M->crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    M->isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    return BZ_OK;
}

// crc(A B) from crc(A) and crc(B), B of any length
CRASS_HD inline uint32_t gz_crc_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    while (len_b > 0x40000000ull) { crc_a = bz_crc_shift(crc_a, 0x40000000u); len_b -= 0x40000000ull; }
    return bz_crc_shift(crc_a, (uint32_t)len_b) ^ crc_b;
}

// ---- find: the part of the test that takes one position and no table ----
// bits p .. p + 127 of d[0, dn) (0 beyond the data) say: BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29 and a code-length code whose
// HCLEN 3-bit lengths make a complete code (Kraft sum 1: what bz_build calls BZ_COMPLETE for lengths of at most 7)
CRASS_HD inline bool gz_prefilter(uint64_t lo, uint64_t hi)
{
    if ((lo & 7u) != 4u) return false;
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = (uint32_t)((lo >> 13) & 15u) + 4u;
    const uint64_t w = (lo >> 17) | (hi << 47);           // 19 lengths of 3 bits: 57 bits
    uint32_t kraft = 0;
    for (uint32_t k = 0; k < hclen; k++) {
        const uint32_t v = (uint32_t)(w >> (3 * k)) & 7u;
        kraft += v ? 128u >> v : 0u;
    }
    return kraft == 128u;
}
// position p of chunk range [.., hi) may be a start
CRASS_HD inline bool gz_survives(const uint8_t *d, uint64_t dn, uint64_t p, uint64_t hi, uint64_t limit)
{
    if (p >= hi || p + 64 >= limit) return false;
    const uint64_t b = p >> 3;
    const uint32_t sh = (uint32_t)(p & 7u);
    uint64_t a = 0, c = 0;
    for (uint32_t i = 0; i < 8; i++) a |= (uint64_t)(b + i < dn ? d[b + i] : 0) << (8 * i);
    for (uint32_t i = 0; i < 3; i++) c |= (uint64_t)(b + 8 + i < dn ? d[b + 8 + i] : 0) << (8 * i);
    const uint64_t lo = sh ? (a >> sh) | (c << (64 - sh)) : a;
    return gz_prefilter(lo, c >> sh);
}

// ---- a run: blocks decoded from a bit position, in one of three ways ----
// The IO of inflate_core.h, with 16-bit symbols as text and a movable input:
//   void     at(uint64_t b0, uint32_t n) in(i) is byte b0 + i of the deflate data for i < n, else 0
//   void     put(uint64_t p, uint32_t s) symbol p of the chunk (p below the counted length, else nothing)
//   uint32_t get(uint64_t p)             ... read back
//   uint64_t survivors(d.., base, hi, limit) bit l: gz_survives(base + l)
enum GzMode : int { GZ_TRIAL = 0, GZ_COUNT = 1, GZ_DECODE = 2 };
struct GzRun { int32_t reason; uint32_t link; uint64_t text, end_bit; };

template <class IO> CRASS_HD inline uint64_t gz_at(const BzBits<IO> &B, uint64_t b0) { return b0 * 8 + (uint64_t)(8u * B.ip - B.nb); }

// TRIAL   two blocks from start_bit, the first one BFINAL 0 / BTYPE 2: reason BZ_OK when both decode
// COUNT   until a link (start[] are all chunks' starts), the final block's end, the span's end or a fault
// DECODE  the blocks COUNT went through (it ended at bit end_bit), as symbols
template <int MODE, class IO>
CRASS_HD inline GzRun gz_run(IO &io, BzTables &T, const GzGeom &G, uint64_t k, uint64_t start_bit, const uint64_t *start, uint64_t end_bit)
{
    const uint64_t b0 = start_bit >> 3, limit = G.dn * 8;
    const uint64_t stop_bit = gz_nominal(G, k + kGzMaxSpan);
    const bool to_end = stop_bit >= limit;
    uint64_t n64 = G.dn - b0;
    if (!to_end && (stop_bit >> 3) - b0 + kGzSlack < n64) n64 = (stop_bit >> 3) - b0 + kGzSlack;
    const uint32_t n_in = (uint32_t)n64;                  // (< 2^28 + kGzSlack: see kGzMaxSpan)
    const bool sees_end = b0 + n_in == G.dn;
    io.at(b0, n_in);
    BzBits<IO> B(io, n_in);
    B.refill();
    B.drop((uint32_t)(start_bit & 7u));
    uint64_t pos = 0;
    uint32_t blocks = 0;
    GzRun R{BZ_OK, GZ_LINK_BAD, 0, 0};
#define GZ_STOP(why_)                                                                                                     \
    {                                                                                                                     \
        int32_t w_ = (why_);                                                                                              \
        if (w_ == BZ_INPUT_END && !sees_end) w_ = BZ_NO_START;                                                            \
        R.reason = w_; R.link = w_ == BZ_NO_START ? GZ_LINK_UNFINISHED : GZ_LINK_BAD; R.text = pos; R.end_bit = gz_at(B, b0); \
        return R;                                                                                                         \
    }
    for (;;) {                                            // a block: at least its 3 header bits
        const uint64_t here = gz_at(B, b0);
        if (MODE == GZ_COUNT && pos > 0 && here < limit) {
            const uint64_t j = gz_chunk_of(G, here);
            if (j > k && start[j] == here) { R.link = (uint32_t)j; break; }
        }
        if (MODE == GZ_DECODE && here == end_bit) break;
        if (MODE == GZ_TRIAL && blocks == 2) break;
        if (!to_end && here >= stop_bit) GZ_STOP(BZ_NO_START);
        B.refill();
        const uint32_t hdr = B.take(3);
        if (B.over()) GZ_STOP(BZ_INPUT_END);
        const uint32_t final_block = hdr & 1u, type = hdr >> 1;
        if (MODE == GZ_TRIAL && blocks == 0 && hdr != 4u) GZ_STOP(BZ_BLOCK_TYPE);
        if (type == 3) GZ_STOP(BZ_BLOCK_TYPE);
        if (type == 0) {
            B.drop(B.nb & 7u);                            // to the byte edge
            B.refill();
            const uint32_t len = B.take(16), nlen = B.take(16);
            if (B.over()) GZ_STOP(BZ_INPUT_END);
            if (len != (~nlen & 0xFFFFu)) GZ_STOP(BZ_STORED_LEN);
            const uint32_t from = B.ip - B.nb / 8;        // (<= n_in: not over)
            if (len > n_in - from) GZ_STOP(BZ_INPUT_END);
            if (MODE == GZ_DECODE) {
                io.par(len, [&](uint32_t i) { io.put(pos + i, io.in(from + i)); });
                io.sync();
            }
            pos += len;
            B.ip = from + len; B.hold = 0; B.nb = 0;
        } else {
            { const int32_t why = bz_block_tables(io, T, B, type); if (why != BZ_OK) GZ_STOP(why); }
            for (;;) {                                    // a literal / length symbol: at least one bit
                if (!to_end && gz_at(B, b0) >= stop_bit) GZ_STOP(BZ_NO_START);
                B.refill();
                int32_t why = 0;
                const int32_t s = bz_symbol(B, T.lit, &why);
                if (s < 0) GZ_STOP(why);
                if (s < 256) {
                    if (MODE == GZ_DECODE && io.lead()) io.put(pos, (uint32_t)s);
                    pos++;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) GZ_STOP(BZ_BAD_SYMBOL);
                const uint32_t li = (uint32_t)s - 257;
                uint32_t len;
                if (li < 8) len = 3 + li;
                else if (li == 28) len = 258;
                else { const uint32_t e = (li >> 2) - 1; len = 3 + ((4 + (li & 3u)) << e) + B.take(e); }
                if (B.over()) GZ_STOP(BZ_INPUT_END);
                B.refill();
                const int32_t d = bz_symbol(B, T.dist, &why);
                if (d < 0) GZ_STOP(why);
                if (d > 29) GZ_STOP(BZ_BAD_SYMBOL);
                uint32_t dist;
                if (d < 4) dist = 1 + (uint32_t)d;
                else { const uint32_t e = ((uint32_t)d >> 1) - 1; dist = 1 + ((2 + ((uint32_t)d & 1u)) << e) + B.take(e); }
                if (B.over()) GZ_STOP(BZ_INPUT_END);
                // (dist <= 32768: it reaches the chunk's own symbols or the window in front of it, nothing else)
                if (MODE == GZ_DECODE) {
                    // symbol i comes from pos - dist + (i mod dist): all of them were there before this match, or lie in the window
                    io.sync();
                    io.par(len, [&](uint32_t i) {
                        const uint64_t q = pos + (dist >= len ? i : i % dist);
                        io.put(pos + i, q >= dist ? io.get(q - dist) : 0x8000u | (kGzWindow - dist + (uint32_t)q));
                    });
                    io.sync();
                }
                pos += len;
            }
        }
        blocks++;
        if (final_block) { R.link = GZ_LINK_END; break; }
    }
#undef GZ_STOP
    R.text = pos; R.end_bit = gz_at(B, b0);
    return R;
}

// start[k] for k >= 1: positions in ascending order, 64 at a time through gz_survives, the survivors through the trial
template <class IO> CRASS_HD inline uint64_t gz_find(IO &io, BzTables &T, const GzGeom &G, uint64_t k)
{
    const uint64_t lo = gz_nominal(G, k), hi = gz_nominal(G, k + 1), limit = G.dn * 8;
    for (uint64_t base = lo; base < hi && base + 64 < limit; base += 64) {
        uint64_t mask = io.survivors(base, hi, limit);
        while (mask) {
            const uint32_t l = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1;
            const GzRun R = gz_run<GZ_TRIAL>(io, T, G, k, base + l, nullptr, 0);
            if (R.reason == BZ_OK) return base + l;
        }
    }
    return kGzNoStart;
}

// ---- windows and narrowing ----
// entry w of the 32 KB in front of a chain element, from the element before it: its L symbols sp and its own window wp (NULL:
// it is the chain's first).  Entries in front of the text's first byte read 0; gz_narrow refuses a marker that points there
CRASS_HD inline uint8_t gz_window_entry(const uint16_t *sp, uint64_t L, const uint8_t *wp, uint32_t w)
{
    const uint64_t back = kGzWindow - w;                  // this entry lies `back` bytes in front of the element
    if (back <= L) {
        const uint32_t s = sp[L - back];
        return (uint8_t)(s < 0x8000u ? s : wp ? wp[s & 0x7FFFu] : 0u);
    }
    return wp ? wp[w + L] : (uint8_t)0;
}
// a symbol of the element whose text starts at byte t0, through its window: the byte, or 0x100 for a marker that points in front
// of the text
CRASS_HD inline uint32_t gz_narrow(uint32_t s, const uint8_t *win, uint64_t t0)
{
    if (s < 0x8000u) return s & 0xFFu;
    const uint32_t w = s & 0x7FFFu;
    if (!win || t0 + w < kGzWindow) return 0x100u;
    return win[w];
}

// ---- the chain (host: a few hundred entries) ----
struct GzVerdict { int32_t reason; uint64_t member, in_pos; };
// from chunk 0 along link: chain[] gets the chunks in order (at most nc), *n_chain their number, *n_text the text's length.
// BZ_OK or the decline (reasons 1 .. 6, 12, 13, 7 / 8)
inline int32_t gz_chain(const GzMember &M, const uint64_t *start, const uint32_t *link, const uint64_t *text_len, const uint64_t *end_bit,
                        const int32_t *reason, uint32_t *chain, uint64_t *n_chain, uint64_t *n_text, GzVerdict *v)
{
    const GzGeom &G = M.G;
    uint64_t n = 0, total = 0, k = 0;
    for (;;) {
        chain[n++] = (uint32_t)k;
        total += text_len[k];
        if (link[k] == GZ_LINK_END) break;
        if (link[k] >= GZ_LINK_NONE || link[k] <= k) {      // bad or unfinished (a link never points back)
            *n_chain = n; *n_text = total;
            v->reason = reason[k] ? reason[k] : BZ_NO_START; v->member = k; v->in_pos = G.d_off + (start[k] >> 3);
            return v->reason;
        }
        k = link[k];
    }
    *n_chain = n; *n_text = total;
    if ((end_bit[k] + 7) / 8 != G.dn) { v->reason = BZ_TRAILING; v->member = k; v->in_pos = G.d_off + (start[k] >> 3); return v->reason; }
    if ((uint32_t)total != M.isize) { v->reason = (uint32_t)total > M.isize ? BZ_OUTPUT_LONG : BZ_OUTPUT_SHORT; v->member = 0; v->in_pos = 0; return v->reason; }
    return BZ_OK;
}

} // namespace crass

// gunzip_core.h — what the host function (gunzip.cpp), the kernels (gunzip.hip) and the engine (engine_ingest.cpp) share about inflating
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
// Ranges (a group's ranks, crass_hip_group_inflate_gzip; serially crass_gzip_inflate_ranges_host): chunk k is rank k N / nc's for
// find and count, a rank holds only d[nominal[k0] / 8, gz_input_end(k1 - 1)) for them; the chain's text offsets are then what a
// BGZF index is to the shard code: rank r takes the elements that hold its range of the text (gz_elements_for, gz_ranges), and
//   windows  a rank cannot know the 32 KB in front of its first element before the rank in front has finished, so it walks its
//            elements from an IDENTITY entry window: gz_window_entry_sym, entries are bytes or 0x8000 | index into that window
//   compose  (host) entry(r + 1) = gz_window_resolve(the symbolic window rank r holds in front of rank r + 1's first element,
//            entry(r)), in rank order; a rank that starts in the same element, or holds none, passes its entry on
//   resolve  every symbolic window through the rank's entry window: the bytes `windows` would have made; narrow as above.  An
//            element's text and CRC-32 part are taken from the first rank that holds it
//
// Members mode by ranges (crass_hip_group_inflate_gzip_members; serially crass_gzip_inflate_members_ranges_host): the two together.
// The rank whose find runs see the region's end also stages the 8 bytes behind it (io.tail()); a decode over the elements
// [e0, e1) writes its GzEnd records at slots relative to slot[e0], the member table is made from the records of each element's
// FIRST holder; the symbolic walk writes dead entries as 0 (gz_entry_dead, below); the CRC pieces are cut also where a range's own
// text begins (gz_crc_pieces), every range runs its own; the verdict comes behind all narrowing: 14 in chain order, then the
// first offending member (gz_member_verdict)
//
// kGzMaxSpan = 32: a chunk gives up when it has gone through 32 chunks' worth of input without meeting a later chunk's start.
// zlib ends a block after at most 32 767 symbols (memLevel 9; 16 383 at the default 8), which for FASTA / FASTQ text is 30 to
// 50 KB of input and at most ~120 KB for text of any kind: 32 chunks of the smallest size (4096 bytes: 128 KB) get through such a
// block and reach the next one's start, so reason 12 is left to input without dynamic block starts (stored or fixed blocks
// throughout) and to blocks much longer than zlib writes.  With the default chunk a block is a fraction of one chunk.  The span
// also bounds what one wave decodes (nothing runs away on a pathological input) and keeps a run's bit offsets inside 32 bits:
// 32 chunks of less than 2 kGzMaxChunk bytes are less than 2^31 bits.
//
// Members mode (the MEM template parameter; off, every statement above is what it was): a file of SEVERAL plain members (cat of
// .gz files, gzip's >>, a compressor that starts a member every N records), which zlib's gzread reads as one stream.  The region
// d[0, dn) is still what lies between the FIRST header and the file's LAST 8 bytes (the last member's trailer); inner trailers and
// inner headers are bytes of the region, chunks and nominal[] are cut over all of it.
//   a run    goes on past a final block: to the byte edge; at the region's end it ends with GZ_LINK_END; otherwise 8 trailer
//            bytes, then at byte H a gzip header (the fields gz_parse_member checks), then the next member's first block.  Bytes at
//            H without the magic, or fewer than 18 bytes up to the file's end: reason 13; the magic but a header the rule does not
//            take, or one that runs into the file's last 8 bytes: 11; a header (or inner trailer) the run cannot read inside its
//            input bound n_in (kGzSlack behind the span) surfaces as the span reason, 12 — accepted: such a run would have given
//            up a few bytes further on anyway, and a larger chunk takes the file.  n_ends counts the final blocks a run passed,
//            last_end is the text position of the last of them
//   window   a match that stands p text bytes behind the last member boundary the run passed, with a distance > p, is a fault
//            (14) in TRIAL, COUNT and DECODE alike; before a run's first boundary references in front of the run stay markers
//   find     position p also passes when it is byte-aligned, the bytes there are a gzip header the rule takes, the member's first
//            block (of any type) decodes and a second one too if there is one, and, where the first block is final, the ISIZE
//            behind it equals the text produced (so a file of many members of one final block each has starts).  Such a start
//            is the bit of the header's FIRST byte.  A byte-aligned 1F reads as BFINAL 1 / BTYPE 3, so the two kinds of start
//            cannot be confused: a run that begins on the magic parses the header first, knows that its member begins there and
//            emits no markers (14 instead).  gz_survives_header is the cheap part, as gz_survives
//   links    COUNT's link test and DECODE's end test run at H as at a block boundary (start[j] == 8 H and text produced), behind
//            the check of the magic at H.  A link goes only to a start of the kind the run arrives as: at H to a member's start,
//            at a block boundary never to one (there the byte-aligned magic is BTYPE 3, as for zlib)
//   narrow   gz_narrow gets m0, the text offset of the start of the member that holds the element's first byte (the host derives
//            it from the chain's n_ends / last_end): a marker w with t0 - m0 + w < kGzWindow points in front of the member (14)
//   ends     DECODE writes a GzEnd per final block it passes into the element's slots (base: the prefix sum of n_ends over the
//            chain); from them the host gets every member's place in file and text and checks every member's ISIZE (7 / 8) and,
//            from k_gz_member_crc's pieces joined with gz_crc_join, its CRC-32 (9).  Unlike the single-member rule, which knows
//            the one ISIZE before it decodes, this happens AFTER the decode step: inner trailers are only met by the runs
// Three deliberate differences from gzread: bytes behind the last member that are no gzip header (zero padding included) are
// declined (13) where zlib ignores them; stored-only or fixed-only data needs a start every kGzMaxSpan chunks (12) where zlib
// takes any size; an inner header beyond a run's input bound is declined (12).
//
// Bounds: a run reads d[b0, b0 + n_in) only, and in members mode the 8 bytes behind the region through io.tail() (in() answers 0
// beyond, every taker checks over()); every loop iteration takes at least one input bit or ends; a decode run writes symbols
// [0, counted length) of its chunk only (put() checks) and its own GzEnd slots only (end() checks).
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
// position p of chunk range [.., hi) may be a start.  d[d_lo, dn) is read, bytes beyond read 0 (a job that holds a part of the
// file passes the end of what it holds as dn: 11 bytes from p on, all inside what a chunk's runs may read)
CRASS_HD inline bool gz_survives(const uint8_t *d, uint64_t dn, uint64_t p, uint64_t hi, uint64_t limit, uint64_t d_lo = 0)
{
    if (p >= hi || p + 64 >= limit || (p >> 3) < d_lo) return false;
    const uint64_t b = p >> 3;
    const uint32_t sh = (uint32_t)(p & 7u);
    uint64_t a = 0, c = 0;
    for (uint32_t i = 0; i < 8; i++) a |= (uint64_t)(b + i < dn ? d[b + i] : 0) << (8 * i);
    for (uint32_t i = 0; i < 3; i++) c |= (uint64_t)(b + 8 + i < dn ? d[b + 8 + i] : 0) << (8 * i);
    const uint64_t lo = sh ? (a >> sh) | (c << (64 - sh)) : a;
    return gz_prefilter(lo, c >> sh);
}

// members mode: position p may be a member's start: byte-aligned, the magic, method 8, no reserved flag
// (d[d_lo, dn) is read, as in gz_survives)
CRASS_HD inline bool gz_survives_header(const uint8_t *d, uint64_t dn, uint64_t p, uint64_t hi, uint64_t limit, uint64_t d_lo = 0)
{
    if (p >= hi || p + 64 >= limit || (p & 7u) || (p >> 3) < d_lo) return false;
    const uint64_t b = p >> 3;                            // (b + 8 < dn)
    return b + 3 < dn && d[b] == 0x1Fu && d[b + 1] == 0x8Bu && d[b + 2] == 8u && !(d[b + 3] & 0xE0u);
}

// ---- a run: blocks decoded from a bit position, in one of three ways ----
// The IO of inflate_core.h, with 16-bit symbols as text and a movable input:
//   void     at(uint64_t b0, uint32_t n) in(i) is byte b0 + i of the deflate data for i < n, else 0
//   void     put(uint64_t p, uint32_t s) symbol p of the chunk (p below the counted length, else nothing)
//   uint32_t get(uint64_t p)             ... read back
//   uint64_t survivors(d.., base, hi, limit) bit l: gz_survives(base + l)
// and in members mode:
//   uint64_t header_survivors(base, hi, limit) bit l: gz_survives_header(base + l)
//   uint32_t tail(uint32_t i)            byte i < 8 behind the region: the file's last trailer
//   void     end(uint32_t e, GzEnd r)    the record of the e-th final block this run passed (e below the counted n_ends, else nothing)
enum GzMode : int { GZ_TRIAL = 0, GZ_COUNT = 1, GZ_DECODE = 2 };
struct GzRun { int32_t reason; uint32_t link; uint64_t text, end_bit; uint32_t n_ends; uint64_t last_end; };
// a member's end as DECODE met it: the text position in the element, the file byte of the next member's header (the file's size
// behind the last member), the trailer's CRC-32 and ISIZE (0 for the last member: the host holds that trailer)
struct GzEnd { uint64_t pos, next; uint32_t crc, isize; };

// members mode: the gzip header at byte h <= n_in of the run's input, of which `room` bytes lie in front of the region's end: its
// length, or minus the reason — 13 without the magic, 11 for a header the rule does not take or that runs into the file's last 8
// bytes, 6 for one the run may not read to its end (gz_run turns that into 12 where the run does not see the region's end)
template <class IO> CRASS_HD inline int32_t gz_header_at(IO &io, const BzTables &T, uint32_t h, uint32_t n_in, uint64_t room)
{
    const uint64_t avail = n_in - h;
    if (avail < 2) return -BZ_INPUT_END;
    if (io.in(h) != 0x1Fu || io.in(h + 1) != 0x8Bu) return -BZ_TRAILING;
    if (avail < 10) return -BZ_INPUT_END;
    if (io.in(h + 2) != 8u || (io.in(h + 3) & 0xE0u)) return -BZ_NOT_GZIP;
    const uint32_t flg = io.in(h + 3);
    uint64_t d = 10;
    if (flg & 4u) {
        if (d + 2 > room) return -BZ_NOT_GZIP;
        if (d + 2 > avail) return -BZ_INPUT_END;
        d += 2 + (uint64_t)(io.in(h + 10) | io.in(h + 11) << 8);
        if (d > room) return -BZ_NOT_GZIP;
        if (d > avail) return -BZ_INPUT_END;
    }
    for (uint32_t bit = 3; bit <= 4; bit++)
        if (flg & (1u << bit)) {
            for (;; d++) {                                // (ends: d reaches room or avail)
                if (d >= room) return -BZ_NOT_GZIP;
                if (d >= avail) return -BZ_INPUT_END;
                if (!io.in(h + (uint32_t)d)) break;
            }
            d++;
        }
    if (flg & 2u) {
        if (d + 2 > room) return -BZ_NOT_GZIP;
        if (d + 2 > avail) return -BZ_INPUT_END;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < (uint32_t)d; i++) c = T.crc_tab[(c ^ io.in(h + i)) & 0xFFu] ^ (c >> 8);
        c = ~c;
        if ((c & 0xFFFFu) != (io.in(h + (uint32_t)d) | io.in(h + (uint32_t)d + 1) << 8)) return -BZ_NOT_GZIP;
        d += 2;
    }
    return (int32_t)d;                                    // (<= n_in < 2^29)
}

template <class IO> CRASS_HD inline uint64_t gz_at(const BzBits<IO> &B, uint64_t b0) { return b0 * 8 + (uint64_t)(8u * B.ip - B.nb); }

// TRIAL   two blocks from start_bit, the first one BFINAL 0 / BTYPE 2: reason BZ_OK when both decode
// COUNT   until a link (start[] are all chunks' starts), the final block's end, the span's end or a fault
// DECODE  the blocks COUNT went through (it ended at bit end_bit), as symbols
// MEM: members mode; header_trial: the TRIAL is that of a member's start (COUNT and DECODE see what their start is by its bytes)
template <int MODE, bool MEM = false, class IO>
CRASS_HD inline GzRun gz_run(IO &io, BzTables &T, const GzGeom &G, uint64_t k, uint64_t start_bit, const uint64_t *start, uint64_t end_bit,
                             bool header_trial = false)
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
    uint64_t pos = 0;
    uint32_t blocks = 0;
    GzRun R{BZ_OK, GZ_LINK_BAD, 0, 0, 0, 0};
    // members mode: the text position of the last member boundary passed, once there is one
    bool bounded = false;
    uint64_t mb = 0;
    const bool at_header = MEM && k > 0 && !(start_bit & 7u) && (MODE != GZ_TRIAL || header_trial) && io.in(0) == 0x1Fu && io.in(1) == 0x8Bu;
    if (MEM && MODE == GZ_TRIAL && header_trial && !at_header) { R.reason = BZ_NOT_GZIP; return R; }
    if (!at_header) {
        B.refill();
        B.drop((uint32_t)(start_bit & 7u));
    }
#define GZ_STOP(why_)                                                                                                     \
    {                                                                                                                     \
        int32_t w_ = (why_);                                                                                              \
        if (w_ == BZ_INPUT_END && !sees_end) w_ = BZ_NO_START;                                                            \
        R.reason = w_; R.link = w_ == BZ_NO_START ? GZ_LINK_UNFINISHED : GZ_LINK_BAD; R.text = pos; R.end_bit = gz_at(B, b0); \
        return R;                                                                                                         \
    }
    if (at_header) {
        const int32_t hl = gz_header_at(io, T, 0, n_in, G.dn - b0);
        if (hl < 0) GZ_STOP(-hl);
        B.ip = (uint32_t)hl;
        bounded = true;
    }
    for (;;) {                                            // a block: at least its 3 header bits
        const uint64_t here = gz_at(B, b0);
        if (MODE == GZ_COUNT && pos > 0 && here < limit) {
            const uint64_t j = gz_chunk_of(G, here);
            // (members mode: a byte-aligned start on the magic is a MEMBER's start; a run that arrives at it at a block boundary
            // stands in the middle of a member, where 1F is BFINAL 1 / BTYPE 3: no link, the block header below faults.  Where the
            // two bytes lie beyond the run's input the kind is unknown: no link either, the run ends at its bound)
            bool member_start = false;
            if (MEM && !(here & 7u)) {
                const uint64_t r = (here >> 3) - b0;
                member_start = r + 2 > n_in || (io.in((uint32_t)r) == 0x1Fu && io.in((uint32_t)r + 1) == 0x8Bu);
            }
            if (j > k && start[j] == here && !member_start) { R.link = (uint32_t)j; break; }
        }
        if (MODE == GZ_DECODE && here == end_bit) break;
        if (MODE == GZ_TRIAL && blocks == 2) break;
        if (!to_end && here >= stop_bit) GZ_STOP(BZ_NO_START);
        B.refill();
        const uint32_t hdr = B.take(3);
        if (B.over()) GZ_STOP(BZ_INPUT_END);
        const uint32_t final_block = hdr & 1u, type = hdr >> 1;
        if (MODE == GZ_TRIAL && blocks == 0 && !at_header && hdr != 4u) GZ_STOP(BZ_BLOCK_TYPE);
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
                if (MEM && bounded && dist > pos - mb) GZ_STOP(BZ_MARKER);      // ... or, behind a boundary, the member's own text
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
        if (!MEM) {
            if (final_block) { R.link = GZ_LINK_END; break; }
            continue;
        }
        if (MODE == GZ_TRIAL && blocks == 2) break;
        if (!final_block) continue;
        // a member's end: the byte edge, the trailer, and unless the region ends here the next member's header
        B.drop(B.nb & 7u);
        const uint32_t from = B.ip - B.nb / 8;            // (<= n_in: not over)
        const uint64_t edge = b0 + from;
        if (MODE == GZ_TRIAL) {                           // (a member's start whose first block is final: its ISIZE)
            uint32_t isz = 0;
            if (edge == G.dn) { for (uint32_t i = 0; i < 4; i++) isz |= io.tail(4 + i) << (8 * i); }
            else {
                if ((uint64_t)from + 8 > n_in) GZ_STOP(BZ_INPUT_END);
                for (uint32_t i = 0; i < 4; i++) isz |= io.in(from + 4 + i) << (8 * i);
            }
            if (isz != (uint32_t)pos) GZ_STOP(BZ_OUTPUT_SHORT);
            break;
        }
        R.n_ends++; R.last_end = pos;
        if (edge == G.dn) {
            if (MODE == GZ_DECODE && io.lead()) io.end(R.n_ends - 1, GzEnd{pos, G.d_off + G.dn + 8, 0, 0});
            R.link = GZ_LINK_END;
            break;
        }
        B.ip = from; B.hold = 0; B.nb = 0;
        if (edge + 8 + 18 > G.dn + 8) GZ_STOP(BZ_TRAILING);
        if ((uint64_t)from + 8 > n_in) GZ_STOP(BZ_INPUT_END);
        if (MODE == GZ_DECODE && io.lead()) {
            uint32_t crc = 0, isz = 0;
            for (uint32_t i = 0; i < 4; i++) { crc |= io.in(from + i) << (8 * i); isz |= io.in(from + 4 + i) << (8 * i); }
            io.end(R.n_ends - 1, GzEnd{pos, G.d_off + edge + 8, crc, isz});
        }
        B.ip = from + 8;
        const uint64_t hbit = (edge + 8) * 8;             // (< limit: 18 bytes follow)
        // the magic before the link and end tests: a link at H goes to a member's start only, never to a block start that
        // happens to stand where a header should (a byte-aligned start on the magic is a member's start: 1F is no BFINAL 0)
        if ((uint64_t)from + 10 > n_in) GZ_STOP(BZ_INPUT_END);
        if (io.in(from + 8) != 0x1Fu || io.in(from + 9) != 0x8Bu) GZ_STOP(BZ_TRAILING);
        if (MODE == GZ_COUNT && pos > 0) {
            const uint64_t j = gz_chunk_of(G, hbit);
            if (j > k && start[j] == hbit) { R.link = (uint32_t)j; break; }
        }
        if (MODE == GZ_DECODE && hbit == end_bit) break;
        if (!to_end && hbit >= stop_bit) GZ_STOP(BZ_NO_START);
        const int32_t hl = gz_header_at(io, T, from + 8, n_in, G.dn - (edge + 8));
        if (hl < 0) GZ_STOP(-hl);
        B.ip = from + 8 + (uint32_t)hl;
        bounded = true; mb = pos;
    }
#undef GZ_STOP
    R.text = pos; R.end_bit = gz_at(B, b0);
    return R;
}

// the end of the input a run of chunk k may read (gz_run's b0 + n_in): d[.., gz_input_end) is what a job stages for its last chunk
CRASS_HD inline uint64_t gz_input_end(const GzGeom &G, uint64_t k)
{
    const uint64_t stop_bit = gz_nominal(G, k + kGzMaxSpan);
    if (stop_bit >= G.dn * 8) return G.dn;
    const uint64_t e = (stop_bit >> 3) + kGzSlack;
    return e < G.dn ? e : G.dn;
}

// start[k] for k >= 1: positions in ascending order, 64 at a time through gz_survives, the survivors through the trial
// (members mode: block starts and member starts alike, whichever comes first)
template <bool MEM = false, class IO> CRASS_HD inline uint64_t gz_find(IO &io, BzTables &T, const GzGeom &G, uint64_t k)
{
    const uint64_t lo = gz_nominal(G, k), hi = gz_nominal(G, k + 1), limit = G.dn * 8;
    for (uint64_t base = lo; base < hi && base + 64 < limit; base += 64) {
        uint64_t heads = 0;
        if (MEM) heads = io.header_survivors(base, hi, limit);
        uint64_t mask = io.survivors(base, hi, limit) | heads;
        while (mask) {
            const uint32_t l = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1;
            const GzRun R = gz_run<GZ_TRIAL, MEM>(io, T, G, k, base + l, nullptr, 0, MEM && ((heads >> l) & 1u));
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
// ---- a RANGE of the chain (a rank of a group): symbolic windows, composed afterwards ----
// A range walks its elements [e0, e1) without knowing the 32 KB in front of element e0 (its ENTRY window: the range before has
// not finished).  Its windows are symbolic: an entry is a byte (< 0x100) or 0x8000 | index into the entry window.
// gz_window_entry_sym is gz_window_entry in that form: entry w of the window in front of an element, from the element before it
// (its L symbols sp, its own symbolic window wp_sym; NULL: that element is the range's first, its window is the identity, so a
// marker of its symbols and an entry that lies in front of it, w + L, stay markers)
CRASS_HD inline uint16_t gz_window_entry_sym(const uint16_t *sp, uint64_t L, const uint16_t *wp_sym, uint32_t w)
{
    const uint64_t back = kGzWindow - w;
    uint32_t idx = (uint32_t)(w + L);                     // (< kGzWindow where it is used: back > L)
    if (back <= L) {
        const uint32_t s = sp[L - back];
        if (s < 0x8000u) return (uint16_t)(s & 0xFFu);
        idx = s & 0x7FFFu;
    }
    return wp_sym ? wp_sym[idx] : (uint16_t)(0x8000u | idx);
}
// Members mode by ranges, DEAD entries: entry w of the window in front of an element whose text starts at t0 lies at text
// position t0 - (kGzWindow - w).  Where that lies in front of m0, the start of the member that holds the element's first byte,
// no symbol may ever read it into the output: gz_narrow refuses such a marker by its position (14) before it looks at the window,
// and a window further on holds the entry only at a position in front of its own m0 >= m0, dead again.  The symbolic walk writes
// such an entry as the byte 0, not as a reference.  So the window behind a member boundary refers to nothing in front of that
// boundary: a range that holds a boundary exports a window without references, and the range behind it needs nothing from it
CRASS_HD inline bool gz_entry_dead(uint64_t t0, uint64_t m0, uint32_t w) { return t0 - m0 + w < kGzWindow; }
CRASS_HD inline uint16_t gz_window_entry_sym_members(const uint16_t *sp, uint64_t L, const uint16_t *wp_sym, uint32_t w, uint64_t t0, uint64_t m0)
{
    return gz_entry_dead(t0, m0, w) ? (uint16_t)0 : gz_window_entry_sym(sp, L, wp_sym, w);
}
// a symbolic entry through the range's entry window (NULL: the range starts at the file's element 0, entries in front of the
// text read 0 as in gz_window_entry).  Also the composition step: the entry window of the next range is the resolve of the
// symbolic window this range holds in front of that range's first element
CRASS_HD inline uint8_t gz_window_resolve(uint16_t sym_entry, const uint8_t *entry_bytes)
{
    return sym_entry < 0x8000u ? (uint8_t)sym_entry : entry_bytes ? entry_bytes[sym_entry & 0x7FFFu] : (uint8_t)0;
}
// the elements that hold the text range [a, b), off[n + 1] the chain's text offsets: [*e0, *e1).  bgzf_members_for's rule
// (fastx_shards.h) with elements in place of members: an element cut by a position is both neighbours', elements without text
// are taken where they lie at b and from element 0 when a is 0, so ranges that tile the text leave no element out, and for
// consecutive ranges e0 <= e0' <= e1
inline void gz_elements_for(const uint64_t *off, uint64_t n, uint64_t a, uint64_t b, uint64_t *e0, uint64_t *e1)
{
    auto ends_behind = [&](uint64_t x) {                  // the first element that ends behind x, or n
        uint64_t lo = 0, hi = n;
        while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (off[mid + 1] > x) hi = mid; else lo = mid + 1; }
        return lo;
    };
    *e0 = a == 0 ? 0 : ends_behind(a);
    uint64_t e = ends_behind(b);
    if (e < n && off[e] < b) e++;
    *e1 = e;
}
// the element ranges of n_ranges >= 1 text ranges that tile [0, T = off[n]), cut at nominal[n_ranges - 1] (NULL: T k / n_ranges):
// e0 / e1 [n_ranges].  false: cuts that decrease or lie beyond T
inline bool gz_ranges(const uint64_t *off, uint64_t n, uint32_t n_ranges, const uint64_t *nominal, uint64_t *e0, uint64_t *e1)
{
    const uint64_t T = off[n];
    uint64_t a = 0;
    for (uint32_t r = 0; r < n_ranges; r++) {
        const uint64_t b = r + 1 == n_ranges ? T : nominal ? nominal[r] : T / n_ranges * (r + 1) + T % n_ranges * (r + 1) / n_ranges;
        if (b < a || b > T) return false;
        gz_elements_for(off, n, a, b, &e0[r], &e1[r]);
        a = b;
    }
    return true;
}

// a symbol of the element whose text starts at byte t0, through its window: the byte, or 0x100 for a marker that points in front
// of the text — in members mode in front of the member that holds the element's first byte, whose text starts at m0 <= t0
CRASS_HD inline uint32_t gz_narrow(uint32_t s, const uint8_t *win, uint64_t t0, uint64_t m0 = 0)
{
    if (s < 0x8000u) return s & 0xFFu;
    const uint32_t w = s & 0x7FFFu;
    if (!win || t0 - m0 + w < kGzWindow) return 0x100u;
    return win[w];
}

// ---- the chain (host: a few hundred entries) ----
struct GzVerdict { int32_t reason; uint64_t member, in_pos; };
// from chunk 0 along link: chain[] gets the chunks in order (at most nc), *n_chain their number, *n_text the text's length.
// BZ_OK or the decline (reasons 1 .. 6, 12, 13, 7 / 8; members: 1 .. 6, 11 .. 14 as the runs met them — every member's ISIZE is
// checked behind the decode step, gz_member_verdict)
inline int32_t gz_chain(const GzMember &M, const uint64_t *start, const uint32_t *link, const uint64_t *text_len, const uint64_t *end_bit,
                        const int32_t *reason, uint32_t *chain, uint64_t *n_chain, uint64_t *n_text, GzVerdict *v, bool members = false)
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
    if (members) return BZ_OK;
    if ((uint32_t)total != M.isize) { v->reason = (uint32_t)total > M.isize ? BZ_OUTPUT_LONG : BZ_OUTPUT_SHORT; v->member = 0; v->in_pos = 0; return v->reason; }
    return BZ_OK;
}

// ---- members mode: places and the member table (host) ----
static const uint64_t kGzCrcPiece = 65536;                // k_gz_member_crc: a member's text is cut into pieces of at most this
// the chain's places from what COUNT reported per chunk: off[i] (text), slot[i] (GzEnd records), both [n + 1], and m0[i] [n]: the
// text offset of the start of the member that holds element i's first byte
inline void gz_places(const uint32_t *chain, uint64_t n, const uint64_t *text_len, const uint32_t *n_ends, const uint64_t *last_end, uint64_t *off,
                      uint64_t *slot, uint64_t *m0)
{
    uint64_t m = 0;
    off[0] = 0; slot[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t k = chain[i];
        m0[i] = m;
        off[i + 1] = off[i] + text_len[k]; slot[i + 1] = slot[i] + n_ends[k];
        if (n_ends[k]) m = off[i] + last_end[k];
    }
}
// the member table from DECODE's records, slot[n] = nm >= 1 of them: in_off / text_off [nm + 1], crc / isize [nm] (the last
// member's from the file's last 8 bytes)
inline void gz_member_table(const GzMember &M, uint64_t n_file, const uint64_t *off, const uint64_t *slot, uint64_t n, const GzEnd *ends,
                            uint64_t *in_off, uint64_t *text_off, uint32_t *crc, uint32_t *isize)
{
    in_off[0] = 0; text_off[0] = 0;
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t e = slot[i]; e < slot[i + 1]; e++) {
            text_off[e + 1] = off[i] + ends[e].pos; in_off[e + 1] = ends[e].next;
            crc[e] = ends[e].crc; isize[e] = ends[e].isize;
        }
    const uint64_t nm = slot[n];
    in_off[nm] = n_file; crc[nm - 1] = M.crc; isize[nm - 1] = M.isize;
}
// the text cuts of the CRC pieces: every member's text from its start in steps of at most kGzCrcPiece, cut again at base[0, nb)
// (ascending text positions: where the text a range holds FIRST begins, so that every piece is one range's).  piece[] has room for
// nm + T / kGzCrcPiece + nb + 2 entries; piece[0, np] are set, piece[np] = T = text_off[nm]; returns np.  An empty member has no piece
inline uint64_t gz_crc_pieces(const uint64_t *text_off, uint64_t nm, const uint64_t *base, uint64_t nb, uint64_t *piece)
{
    uint64_t np = 0, q = 0;
    for (uint64_t m = 0; m < nm; m++)
        for (uint64_t p = text_off[m]; p < text_off[m + 1];) {
            while (q < nb && base[q] <= p) q++;
            piece[np++] = p;
            uint64_t nx = text_off[m + 1] - p > kGzCrcPiece ? p + kGzCrcPiece : text_off[m + 1];
            if (q < nb && base[q] < nx) nx = base[q];
            p = nx;
        }
    piece[np] = text_off[nm];
    return np;
}
// the first offending member, ISIZE (7 / 8) before CRC-32 (9) within a member; crc_got[m]: the CRC-32 of member m's text
inline int32_t gz_member_verdict(uint64_t nm, const uint64_t *in_off, const uint64_t *text_off, const uint32_t *crc, const uint32_t *isize,
                                 const uint32_t *crc_got, GzVerdict *v)
{
    for (uint64_t m = 0; m < nm; m++) {
        const uint32_t len = (uint32_t)(text_off[m + 1] - text_off[m]);
        const int32_t why = len > isize[m] ? BZ_OUTPUT_LONG : len < isize[m] ? BZ_OUTPUT_SHORT : crc_got[m] != crc[m] ? BZ_CRC : BZ_OK;
        if (why != BZ_OK) { v->reason = why; v->member = m; v->in_pos = in_off[m]; return why; }
    }
    return BZ_OK;
}

} // namespace crass

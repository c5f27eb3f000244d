// inflate_core.h — what the host function (bgzf.cpp), the kernel (inflate.hip) and the engine (engine_ingest.cpp) share about inflating
// ONE member of a BGZF file (SAM spec 4.1: a gzip member of at most 64 KB of text that names its own size): the DEFLATE decoder
// (RFC 1951: stored, fixed and dynamic blocks, any number per member), the CRC-32 of RFC 1952, the decline reasons and the order
// in which they are reported.  Plain C++ with CRASS_HD (pack_text.h), so the rule exists once for host and device, like
// fastx_scan.h.  Not part of the public ABI (the reasons' VALUES are: include/crass_hip.h names them).
//
// The decoder is written against an IO type that says how input bytes are read, how text bytes are written and read back, and
// how an index range is worked through: one after the other on the host, 64 lanes side by side in a wave.  Every statement below
// runs in both places; on the device all lanes of the wave run the serial parts with the same values.
//   uint32_t in(uint32_t i)              byte i of the member's deflate data, 0 for i >= n_in (never a read outside the data)
//   void     put(uint32_t p, uint32_t b) byte p of the member's text (p < isize is the core's duty: see the bounds below)
//   uint32_t get(uint32_t p)             ... read back (p below the bytes produced)
//   void     par(uint32_t n, F f)        f(i) for every i in [0, n), in any order, none depending on another
//   bool     lead()                      true for the one executor that writes the tables' single entries
//   void     sync()                      what par() or lead() wrote is visible to everybody afterwards
//
// Bounds, all from the member's own two sizes (n_in bytes of deflate data, isize bytes of text):
//   * the bit reader hands out zeros beyond n_in and every taker checks over() before it believes them: BZ_INPUT_END
//   * a literal, a stored run or a match that would pass isize ends the member BEFORE anything of it is written: BZ_OUTPUT_LONG
//   * a match reaches back over bytes this member produced, or ends it: BZ_DISTANCE
//   * every loop iteration takes at least one bit (a code has at least one) or ends the member; every code table is indexed by
//     at most 15 bits of a walk that ends by itself
// The member's verdict is the first reason its decoder meets; the file's is the smallest bz_offence over its members.
#pragma once
#include <stdint.h>
#include "pack_text.h"

namespace crass {

// decline reasons (crass_bgzf_verdict.reason), in the order a decoder meets them; 0: accepted
enum BzReason : int32_t {
    BZ_OK = 0,
    BZ_BLOCK_TYPE = 1,       // BTYPE 3
    BZ_STORED_LEN = 2,       // stored block: LEN != ~NLEN
    BZ_CODE_LENGTHS = 3,     // dynamic block: HLIT > 286 or HDIST > 30; an over-subscribed or incomplete code (but a single distance
                             // code of one bit, and no distance code at all); repeat code 16 first; a repeat past HLIT + HDIST; no
                             // end-of-block code
    BZ_BAD_SYMBOL = 4,       // a bit pattern that is no code; length symbol 286 / 287; distance symbol 30 / 31
    BZ_DISTANCE = 5,         // a distance beyond the bytes this member has produced
    BZ_INPUT_END = 6,        // the data ends before the final block's end-of-block
    BZ_OUTPUT_LONG = 7,      // more text than ISIZE
    BZ_OUTPUT_SHORT = 8,     // the final block ends before ISIZE bytes
    BZ_CRC = 9,              // the text's CRC-32 is not the trailer's
    BZ_NOT_BGZF = 10,        // the index: a member that does not parse as BGZF (a plain .gz); position: that member's first byte
    // plain gzip, one member inflated chunk by chunk (gunzip_core.h); `member` is the chunk there
    BZ_NOT_GZIP = 11,        // not a gzip header (magic, method, reserved flags, header CRC), or a header that runs into the trailer
    BZ_NO_START = 12,        // a chunk on the chain met no block start of a later chunk within kGzMaxSpan chunks
    BZ_TRAILING = 13,        // the final block ends before the deflate data does (further members, trailing bytes)
    BZ_MARKER = 14           // a distance that reaches in front of the text's first byte
};

static const uint32_t kBzMaxText = 65536;        // ISIZE of a member (bgzf_walk's limit)
static const uint64_t kBzNoOffence = ~0ull;
// one member's offence as a sortable word: the smallest over all members is the file's verdict
CRASS_HD inline uint64_t bz_offence(uint64_t member, uint32_t reason) { return (member << 8) | reason; }

// ---- CRC-32, polynomial 0xEDB88320 (RFC 1952, bit-reflected: x^0 is bit 31) ----
CRASS_HD inline uint32_t bz_crc_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    return c;
}
// a(x) b(x) mod P
CRASS_HD inline uint32_t bz_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; k++) {
        p ^= b & (0u - ((a >> 31) & 1u));
        a <<= 1;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));      // b x
    }
    return p;
}
// x^(8 n) mod P
CRASS_HD inline uint32_t bz_gf_xpow8(uint32_t n)
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;               // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1u) r = bz_gf_mul(r, sq);
        sq = bz_gf_mul(sq, sq);
    }
    return r;
}
// crc(A B) from crc(A), crc(B) and the length of B: crc(A) x^(8 |B|) + crc(B)
CRASS_HD inline uint32_t bz_crc_shift(uint32_t crc_a, uint32_t len_b) { return bz_gf_mul(bz_gf_xpow8(len_b), crc_a); }

// ---- code tables ----
static const int kBzLitFast = 9, kBzDistFast = 8, kBzSlices = 64;
// a canonical prefix code: codes per length, where each length's symbols start in sym[] (sorted by length, then symbol), and a
// table over the next `fast` bits: (symbol << 4) | length, 0: longer than `fast` bits or no code
// (arrays, not pointers: on the device the tables are in LDS, and an address the compiler can follow stays an LDS access)
struct BzCode { uint16_t count[16], offs[16]; uint32_t fast_bits; uint16_t sym[288], fast[1 << kBzLitFast]; };
// what one member's decoder needs beside its text: 7 KB, a wave's share of LDS on the device
struct BzTables {
    uint32_t crc_tab[256];
    uint32_t crc_part[kBzSlices];
    uint8_t lens[288 + 32];
    BzCode lit, dist, cl;                  // literal / length, distance, code length
};

// the walk of a canonical code over `bits` (bit 0 first), at most maxlen of them: (symbol << 4) | length, 0: no code that short
CRASS_HD inline uint32_t bz_walk(const BzCode &C, uint32_t bits, uint32_t maxlen)
{
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= maxlen; len++) {
        code |= bits & 1u; bits >>= 1;
        const uint32_t cnt = C.count[len];
        if (code < first + cnt) return ((uint32_t)C.sym[index + (code - first)] << 4) | len;
        index += cnt; first = (first + cnt) << 1; code <<= 1;
    }
    return 0;
}

// what the lengths of a code say: complete (every bit pattern is a code), no symbol at all, a single code of one bit, or refused
enum BzShape : uint32_t { BZ_COMPLETE = 0, BZ_NO_CODE = 1, BZ_ONE_BIT = 2, BZ_REFUSED = 3 };

// the tables of the code whose symbol s has lens[s] bits (0: unused), s < n <= 288
template <class IO> CRASS_HD inline uint32_t bz_build(IO &io, BzCode &C, const uint8_t *lens, uint32_t n)
{
    io.sync();
    io.par(16, [&](uint32_t l) {
        uint32_t c = 0;
        for (uint32_t s = 0; s < n; s++) c += lens[s] == l ? 1u : 0u;
        C.count[l] = (uint16_t)(l ? c : 0);
    });
    io.sync();
    int32_t left = 1;
    uint32_t at = 0, used = 0;
    for (uint32_t l = 1; l < 16; l++) {
        const uint32_t cnt = C.count[l];
        if (io.lead()) C.offs[l] = (uint16_t)at;
        at += cnt; used += cnt;
        left = 2 * left - (int32_t)cnt;
        if (left < 0) return BZ_REFUSED;                      // over-subscribed
    }
    uint32_t shape = BZ_COMPLETE;
    if (used == 0) shape = BZ_NO_CODE;
    else if (left > 0) shape = (used == 1 && C.count[1] == 1) ? BZ_ONE_BIT : BZ_REFUSED;
    if (shape == BZ_REFUSED) return shape;
    io.sync();
    io.par(16, [&](uint32_t l) {
        if (l == 0) return;
        uint32_t k = C.offs[l];
        for (uint32_t s = 0; s < n; s++) if (lens[s] == l) C.sym[k++] = (uint16_t)s;
    });
    io.sync();
    const uint32_t fb = C.fast_bits;
    io.par(1u << fb, [&](uint32_t e) { C.fast[e] = (uint16_t)bz_walk(C, e, fb); });
    io.sync();
    return shape;
}

// ---- the bit reader: bits come lowest first out of bytes in ascending order (RFC 1951 3.1.1) ----
template <class IO> struct BzBits {
    IO &io; uint32_t n_in, ip; uint64_t hold; uint32_t nb;
    CRASS_HD BzBits(IO &io_, uint32_t n) : io(io_), n_in(n), ip(0), hold(0), nb(0) {}
    CRASS_HD void refill() { while (nb <= 56) { hold |= (uint64_t)io.in(ip) << nb; ip++; nb += 8; } }      // (ip <= n_in + 8: in() answers 0 there)
    CRASS_HD uint32_t peek(uint32_t k) const { return (uint32_t)hold & ((1u << k) - 1u); }                   // k <= 16, after refill()
    CRASS_HD void drop(uint32_t k) { hold >>= k; nb -= k; }
    CRASS_HD uint32_t take(uint32_t k) { const uint32_t v = peek(k); drop(k); return v; }
    CRASS_HD bool over() const { return 8u * ip - nb > 8u * n_in; }                                          // bits were taken that the data does not have
    CRASS_HD uint32_t left() const { const uint32_t used = 8u * ip - nb; return used < 8u * n_in ? 8u * n_in - used : 0u; }
};

// one symbol of code C off the reader (refilled by the caller): the symbol, or -1 no code (*why says which reason)
template <class IO> CRASS_HD inline int32_t bz_symbol(BzBits<IO> &B, const BzCode &C, int32_t *why)
{
    const uint32_t bits = B.peek(15);
    uint32_t e = C.fast[bits & ((1u << C.fast_bits) - 1u)];
    if (!e) e = bz_walk(C, bits, 15);
    if (!e) { *why = B.left() == 0 ? BZ_INPUT_END : BZ_BAD_SYMBOL; return -1; }
    B.drop(e & 15u);
    if (B.over()) { *why = BZ_INPUT_END; return -1; }
    return (int32_t)(e >> 4);
}

// the tables that do not depend on the member: once per executor (a host call, a wave)
template <class IO> CRASS_HD inline void bz_prepare(IO &io, BzTables &T)
{
    io.par(256, [&](uint32_t i) { T.crc_tab[i] = bz_crc_entry(i); });
    if (io.lead()) { T.lit.fast_bits = kBzLitFast; T.dist.fast_bits = kBzDistFast; T.cl.fast_bits = 7; }
    io.sync();
}

// the literal / length and distance codes of a block of type 1 (fixed) or 2 (dynamic: its header comes off the reader): BZ_OK or
// the reason
template <class IO> CRASS_HD inline int32_t bz_block_tables(IO &io, BzTables &T, BzBits<IO> &B, uint32_t type)
{
    if (type == 1) {
        io.par(288, [&](uint32_t s) { T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8); });
        io.par(32, [&](uint32_t s) { T.lens[288 + s] = 5; });
        (void)bz_build(io, T.lit, T.lens, 288);
        (void)bz_build(io, T.dist, T.lens + 288, 32);
    } else {
        B.refill();
        const uint32_t hlit = B.take(5) + 257, hdist = B.take(5) + 1, hclen = B.take(4) + 4;
        if (B.over()) return BZ_INPUT_END;
        if (hlit > 286 || hdist > 30) return BZ_CODE_LENGTHS;
        const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                                  5ull << 45 | 11ull << 50 | 4ull << 55;
        const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        io.par(19, [&](uint32_t s) { T.lens[s] = 0; });
        io.sync();
        for (uint32_t k = 0; k < hclen; k++) {
            B.refill();
            const uint32_t v = B.take(3);
            if (B.over()) return BZ_INPUT_END;
            const uint32_t s = (uint32_t)((k < 12 ? order_lo >> (5 * k) : order_hi >> (5 * (k - 12))) & 31u);
            if (io.lead()) T.lens[s] = (uint8_t)v;
        }
        BzCode &CL = T.cl;
        if (bz_build(io, CL, T.lens, 19) != BZ_COMPLETE) return BZ_CODE_LENGTHS;
        const uint32_t total = hlit + hdist;
        for (uint32_t i = 0; i < total;) {            // a code-length symbol: at least one bit
            B.refill();
            int32_t why = 0;
            const int32_t s = bz_symbol(B, CL, &why);
            if (s < 0) return why;
            if (s < 16) {
                if (io.lead()) T.lens[i] = (uint8_t)s;
                i++;
                io.sync();
                continue;
            }
            uint32_t rep, val = 0;
            if (s == 16) { rep = 3 + B.take(2); }
            else if (s == 17) rep = 3 + B.take(3);
            else rep = 11 + B.take(7);
            if (B.over()) return BZ_INPUT_END;
            if (s == 16) {
                if (i == 0) return BZ_CODE_LENGTHS;
                val = T.lens[i - 1];
            }
            if (rep > total - i) return BZ_CODE_LENGTHS;
            io.par(rep, [&](uint32_t k) { T.lens[i + k] = (uint8_t)val; });
            io.sync();
            i += rep;
        }
        if (T.lens[256] == 0) return BZ_CODE_LENGTHS;
        if (bz_build(io, T.lit, T.lens, hlit) != BZ_COMPLETE) return BZ_CODE_LENGTHS;
        if (bz_build(io, T.dist, T.lens + hlit, hdist) == BZ_REFUSED) return BZ_CODE_LENGTHS;
    }
    return BZ_OK;
}

// the deflate data of one member -> its text.  BZ_OK: exactly isize bytes were put
template <class IO> CRASS_HD inline int32_t bz_inflate_member(IO &io, BzTables &T, uint32_t n_in, uint32_t isize)
{
    BzBits<IO> B(io, n_in);
    uint32_t pos = 0;
    for (;;) {                                                // a block: at least its 3 header bits
        B.refill();
        const uint32_t hdr = B.take(3);
        if (B.over()) return BZ_INPUT_END;
        const uint32_t final_block = hdr & 1u, type = hdr >> 1;
        if (type == 3) return BZ_BLOCK_TYPE;
        if (type == 0) {
            B.drop(B.nb & 7u);                                // to the byte edge
            B.refill();
            const uint32_t len = B.take(16), nlen = B.take(16);
            if (B.over()) return BZ_INPUT_END;
            if (len != (~nlen & 0xFFFFu)) return BZ_STORED_LEN;
            const uint32_t from = B.ip - B.nb / 8;            // (<= n_in: not over)
            const uint32_t have = n_in - from, room = isize - pos;
            if (len > have && have <= room) return BZ_INPUT_END;
            if (len > room) return BZ_OUTPUT_LONG;
            io.par(len, [&](uint32_t i) { io.put(pos + i, io.in(from + i)); });
            io.sync();
            pos += len;
            B.ip = from + len; B.hold = 0; B.nb = 0;
        } else {
            { const int32_t why = bz_block_tables(io, T, B, type); if (why != BZ_OK) return why; }
            for (;;) {                                        // a literal / length symbol: at least one bit
                B.refill();
                int32_t why = 0;
                const int32_t s = bz_symbol(B, T.lit, &why);
                if (s < 0) return why;
                if (s < 256) {
                    if (pos >= isize) return BZ_OUTPUT_LONG;
                    if (io.lead()) io.put(pos, (uint32_t)s);
                    pos++;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return BZ_BAD_SYMBOL;
                const uint32_t li = (uint32_t)s - 257;
                uint32_t len;
                if (li < 8) len = 3 + li;
                else if (li == 28) len = 258;
                else { const uint32_t e = (li >> 2) - 1; len = 3 + ((4 + (li & 3u)) << e) + B.take(e); }
                if (B.over()) return BZ_INPUT_END;
                B.refill();
                const int32_t d = bz_symbol(B, T.dist, &why);
                if (d < 0) return why;
                if (d > 29) return BZ_BAD_SYMBOL;
                uint32_t dist;
                if (d < 4) dist = 1 + (uint32_t)d;
                else { const uint32_t e = ((uint32_t)d >> 1) - 1; dist = 1 + ((2 + ((uint32_t)d & 1u)) << e) + B.take(e); }
                if (B.over()) return BZ_INPUT_END;
                if (dist > pos) return BZ_DISTANCE;
                if (len > isize - pos) return BZ_OUTPUT_LONG;
                // byte i comes from pos - dist + (i mod dist): all of them were there before this match
                io.sync();
                const uint32_t src = pos - dist;
                if (dist >= len) io.par(len, [&](uint32_t i) { io.put(pos + i, io.get(src + i)); });
                else io.par(len, [&](uint32_t i) { io.put(pos + i, io.get(src + i % dist)); });
                io.sync();
                pos += len;
            }
        }
        if (final_block) break;
    }
    // (bits between the final block's end and the trailer are nobody's: a member of known length, as zlib treats it)
    if (pos < isize) return BZ_OUTPUT_SHORT;
    return BZ_OK;
}

// CRC-32 of the isize bytes of text: kBzSlices slices, each one's CRC moved to its place by x^(8 bytes behind it), summed
template <class IO> CRASS_HD inline uint32_t bz_text_crc(IO &io, BzTables &T, uint32_t isize)
{
    const uint32_t per = (isize + kBzSlices - 1) / kBzSlices;
    io.sync();
    io.par(kBzSlices, [&](uint32_t k) {
        const uint32_t a = k * per < isize ? k * per : isize, b = a + per < isize ? a + per : isize;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t p = a; p < b; p++) c = T.crc_tab[(c ^ io.get(p)) & 0xFFu] ^ (c >> 8);
        c = b > a ? ~c : 0u;                                  // (an empty slice adds nothing)
        T.crc_part[k] = b > a ? bz_crc_shift(c, isize - b) : 0u;
    });
    io.sync();
    uint32_t crc = 0;
    for (int k = 0; k < kBzSlices; k++) crc ^= T.crc_part[k];
    return crc;
}

} // namespace crass

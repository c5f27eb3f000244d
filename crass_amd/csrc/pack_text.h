// pack_text.h — what the host packer (ingest.cpp), the device packer (pack.hip) and the engine (engine_ingest.cpp) share about
// turning sequence text into the 2-bit layout of include/crass_hip.h: the byte -> code function and the layout decision
// (stride / uniform length).  Plain C++: ingest.cpp stays host-only code that any compiler builds (tools/sanitize); under
// hipcc the code function is a __host__ __device__ one.  The kernel's job description and launch wrappers: pack_launch.h.
// Not part of the public ABI.
#pragma once
#include <stdint.h>
#include "../../include/crass_hip.h"

#ifdef __HIPCC__
#define CRASS_HD __host__ __device__
#else
#define CRASS_HD
#endif

namespace crass {

// Four sequence bytes (byte 0 = the first base, little endian) -> their four 2-bit codes in bits [2 i, 2 i + 2) and, in
// *bad, bit i set when byte i is not one of 'A' 'C' 'G' 'T' (its code is then 0).  Exact for all 256 byte values: the code
// of a letter is bits 1..2 of its ASCII value with the two upper values exchanged (A 0x41 -> 0, C 0x43 -> 1, T 0x54 -> 2,
// G 0x47 -> 3, then x ^ (x >> 1)); the letter that code stands for is built again (0x41 + 2 b0 + 6 b1 + 11 b0 b1) and
// compared with the byte that was read, so anything else — lower case, 'N', 'U', 0x00, 0xFF — differs somewhere.
CRASS_HD inline uint32_t pack_code4(uint32_t v, uint32_t *bad)
{
    const uint32_t x = (v >> 1) & 0x03030303u;
    uint32_t code = x ^ ((x >> 1) & 0x01010101u);
    const uint32_t b0 = code & 0x01010101u, b1 = (code >> 1) & 0x01010101u;
    const uint32_t letter = 0x41414141u + 2u * b0 + 6u * b1 + 11u * (b0 & b1);      // (at most 0x54 per byte: no carry)
    const uint32_t diff = v ^ letter;
    const uint32_t nz = ((((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u) >> 7;      // bit 8 i: byte i differs
    code &= ~(nz * 3u);
    code = (code | (code >> 6)) & 0x000F000Fu;
    code = (code | (code >> 12)) & 0xFFu;
    *bad = (nz * 0x10204080u) >> 28;                   // bits 0, 8, 16, 24 -> 0 .. 3 (the partial products meet in no bit)
    return code;
}

// The layout crass_pack_reads gives a read set (ingest.cpp; the one rule for the host and the device packer).
// pad_uniform: 0 per-read word offsets, 1 one stride, 2 one stride when the reads are short and padding is cheap.
struct PackLayout {
    uint32_t max_len = 0;
    uint32_t stride_words = 0;      // > 0: read i starts at word i * stride_words
    uint32_t uniform_len = 0;       // > 0: every read has this length
    uint64_t total_words = 0;       // words of the set (four zero words follow)
};
// CRASS_ERR_UNSUPPORTED: a read beyond CRASS_HIP_MAX_READ_LEN; CRASS_ERR_INVALID_ARG: off decreases somewhere
int pack_layout(const uint64_t *off, uint64_t n, int pad_uniform, PackLayout *out);
void pack_layout_core(uint64_t n, uint32_t max_len, uint32_t min_len, uint64_t tight_words, int pad_uniform, PackLayout *out);

// a crass_packed (free with crass_free_packed) whose arrays have the given element counts and are filled by the caller;
// a count of 0 leaves the array NULL
struct PackedArrays { uint32_t *packed; uint64_t *word_off; uint32_t *lengths; uint64_t *exc_read, *exc_off; uint8_t *exc_bytes; uint64_t *header_id; };
int packed_alloc(uint64_t n_words, uint64_t n_word_off, uint64_t n_lengths, uint64_t n_exc_read, uint64_t n_exc_off, uint64_t n_exc_bytes,
                 uint64_t n_header_id, crass_packed *out, PackedArrays *arrays);

} // namespace crass

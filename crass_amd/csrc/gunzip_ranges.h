// gunzip_ranges.h — what the group (group_gzip.cpp) and the device gunzip (engine_inflate.cpp) share about inflating ONE plain gzip
// file across the ranks of a group (crass_hip_group_inflate_gzip): the file's state, which the group owns and the ranks fill
// between barriers, and one rank's four steps.  The rule is gunzip_core.h's (chunks dealt over the ranks, symbolic windows,
// composition); its serial restatement is crass_gzip_inflate_ranges_host.  Not part of the public ABI.
#pragma once
#include "../../include/crass_hip.h"
#include "gunzip_core.h"

#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)
namespace crass {

struct GzRangesFile {
    const uint8_t *bytes = nullptr; uint64_t n_bytes = 0;      // the file, host memory
    uint32_t n_ranks = 0;
    GzMember M{};
    // per chunk [M.G.nc]: rank r writes the entries of its chunks (chunk k is rank k n_ranks / nc's), everybody reads behind a barrier
    std::vector<uint64_t> start, text_len, end_bit;
    std::vector<uint32_t> link;
    std::vector<int32_t> reason;
    // rank 0, from gz_chain and gz_ranges: the chain, its text offsets [n_chain + 1], every rank's elements [e0[r], e1[r]) and the
    // elements [0, first[r]) that a rank in front of r holds (e0 / e1 / first have an entry behind the last rank: no elements)
    std::vector<uint32_t> chain;
    uint64_t n_chain = 0, n_text = 0;
    std::vector<uint64_t> off, e0, e1, first;
    // per rank: the symbolic window in front of the next rank's first element (empty: the identity), then from rank 0's
    // composition the entry window (rank 0's and every rank's that starts at element 0: empty, entries read 0)
    std::vector<std::vector<uint16_t>> exported;
    std::vector<std::vector<uint8_t>> entry;
    // per element, from the first rank that holds it; per rank the smallest element with an unresolved marker (~0: none)
    std::vector<uint32_t> crc_part;
    std::vector<uint64_t> bad;
    // members mode (gunzip_core.h; off, nothing below is touched): per chunk n_ends / last_end from count; rank 0 behind the count
    // step: gz_places' slot [n_chain + 1] and m0 [n_chain]; the GzEnd records [slot[n_chain]], every element's from its FIRST
    // holder (a rank writes the records of the elements no rank in front of it holds: ranges apart); rank 0 behind the decode
    // step: the member table (gz_member_table; table_ok false: a record nobody wrote) and the text cuts of the CRC pieces
    // (gz_crc_pieces, cut also where a rank's own text begins: a piece is one rank's); every rank the CRC-32 of its pieces
    bool members = false, table_ok = false;
    std::vector<uint32_t> n_ends;
    std::vector<uint64_t> last_end, slot, m0;
    std::vector<GzEnd> ends;
    std::vector<uint64_t> in_off, text_off, piece;
    std::vector<uint32_t> mcrc, misz, crc_piece;
    uint64_t n_pieces = 0, exported_plain = 0;      // exported_plain: exported windows without a reference
    // the chunks of rank r: [k_lo(r), k_lo(r + 1))
    uint64_t k_lo(uint32_t r) const { return (M.G.nc * r + n_ranks - 1) / n_ranks; }
};

} // namespace crass

// One rank's steps; the group's threads meet at a barrier behind each.  CRASS_OK or a HIP / memory error; declines are the
// host's to find (gz_chain behind step 2, crc_part / bad behind step 4).
// Members mode (F.members): the members kernels; find also stages the file's last 8 bytes on a rank whose runs see the region's
// end, count brings n_ends / last_end, decode the rank's GzEnd records (slots relative to its first element's) and the symbolic
// walk writes dead entries as 0, finish narrows with m0 and runs k_gz_member_crc over the rank's own pieces into F.crc_piece.
// 1. stages the compressed bytes its chunks' runs may read and finds its chunks' starts (k_gz_find) into F.start
int gzip_rank_find(crass_hip_ctx *c, crass::GzRangesFile &F, uint32_t r);
// 2. with every rank's starts: counts its chunks (k_gz_count) into F.link / text_len / end_bit / reason
int gzip_rank_count(crass_hip_ctx *c, crass::GzRangesFile &F, uint32_t r);
// 3. with the chain and the ranges: fetches what its elements' runs still need, decodes them (k_gz_decode), walks the symbolic
//    windows (k_gz_windows_sym) and exports the one in front of the next rank's first element into F.exported[r]
int gzip_rank_decode(crass_hip_ctx *c, crass::GzRangesFile &F, uint32_t r);
// 4. with its entry window F.entry[r]: resolves (k_gz_window_resolve), narrows (k_gz_narrow) and copies the text of the elements no
//    rank in front of it holds to out[off[i] ..), their CRC parts into F.crc_part, its verdict into F.bad[r]
//    keep (a group's files load, out NULL): nothing goes to the host but the CRC parts; the text stays on the rank's device with the
//    resolved window behind its last element, for gzip_kept_inflate
int gzip_rank_finish(crass_hip_ctx *c, crass::GzRangesFile &F, uint32_t r, uint8_t *out, bool keep);
// the elements [m0, m1) of a file of a group's files load as text, text position t at text0 + t (a DEVICE pointer): copied from
// what the rank keeps of the file; elements behind it are inflated first — decoded, their windows walked by k_gz_windows from
// the kept window (a seeded walk), narrowed — and kept too.  CRASS_ERR_UNSUPPORTED with *bv: an unresolved marker there
int gzip_kept_inflate(crass_hip_ctx *c, const crass::GzRangesFile &F, uint64_t m0, uint64_t m1, uint8_t *text0, crass_bgzf_verdict *bv);
// what a rank keeps goes back (the load's end); the seeded walks since the last reset: HIP-event milliseconds (stage timing >= 1), elements;
// reset also empties the list of uploads (host address ranges of the files' deflate bytes, gzip_rank_report)
void gzip_kept_release(crass_hip_ctx *c);
void gzip_kept_report(crass_hip_ctx *c, float *tail_ms, uint64_t *tail_elements, bool reset);
// the scratch goes back; ms[6]: HIP-event milliseconds of find, count, decode, symbolic windows, resolve, narrow (stage timing
// >= 1, else 0); uploads: the host address ranges of deflate bytes this rank sent to its device since the last reset
void gzip_rank_release(crass_hip_ctx *c);
void gzip_rank_report(const crass_hip_ctx *c, float ms[6], std::vector<std::pair<uint64_t, uint64_t>> *uploads);
// members mode: HIP-event milliseconds of k_gz_member_crc in the rank's last finish step (stage timing >= 1, else 0)
float gzip_rank_member_crc_ms(const crass_hip_ctx *c);
#pragma GCC visibility pop

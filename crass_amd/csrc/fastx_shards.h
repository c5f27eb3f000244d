// fastx_shards.h — what the group (group_files.cpp) and the device ingest (engine_shards.cpp) share about loading record-aligned
// shards of a job's files (crass_hip_group_load_fastx_files): one rank's three steps, between which the group's threads meet
// at barriers and rank 0 combines, and the host arithmetic of a shard (fastx_scan.cpp).  The cut rule is fastx_scan.h's.  Not
// part of the public ABI.
#pragma once
#include "../../include/crass_hip.h"
#include "fastx_scan.h"

#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)
namespace crass {

// what the host knows of a file before a byte goes up
struct ShardFile {
    const uint8_t *bytes; uint64_t n_bytes;
    uint64_t n_text;                       // the text's size (BGZF: the members' ISIZE summed)
    const crass_bgzf_index *ix;            // nullptr: plain text
    // a plain gzip file a group takes (crass_hip_group_set_gzip_on_device): its chain's ELEMENTS in place of BGZF members — ix
    // then holds their text offsets (out_off; in_off / data_off unused) and gz what inflates them (gunzip_ranges.h); else nullptr
    const struct GzRangesFile *gz;
    int32_t format;                        // the text's byte 0; a BGZF file's is known once a rank has inflated its first member
};
struct ShardPos { uint32_t file; uint64_t pos; };      // a position of the text space: (n_files, 0) is its end
// a rank's part of one file before the cuts are known, and its probe
struct ShardPiece {
    uint32_t file; uint64_t a, b;          // the text range [a, b) of that file
    bool left_is_ls;                       // a is a line start
    int32_t first_byte;                    // a == 0: the text's byte 0
    FxProbe probe;
};
// a decline: file -1 is none.  Order: the first file wins; in a file a compression decline comes before a FASTA / FASTQ one
// (the host inflates a file before it scans it), then the smallest (member | line position, reason)
struct ShardVerdict { int32_t file = -1, reason = 0; uint64_t pos = 0; crass_bgzf_verdict bgzf{}; };
inline bool shard_verdict_before(const ShardVerdict &x, const ShardVerdict &y)
{
    if (x.file < 0 || y.file < 0) return y.file < 0 && x.file >= 0;
    if (x.file != y.file) return x.file < y.file;
    const bool xz = x.bgzf.reason != 0, yz = y.bgzf.reason != 0;
    if (xz != yz) return xz;
    if (xz) return x.bgzf.member != y.bgzf.member ? x.bgzf.member < y.bgzf.member : x.bgzf.reason < y.bgzf.reason;
    return x.pos != y.pos ? x.pos < y.pos : x.reason < y.reason;
}

// ---- host arithmetic of a shard, no device byte read (fastx_scan.cpp; tools/sanitize/shards_main.cpp checks both) ----
// The members of a BGZF index (out_off[n_members + 1], non-decreasing from 0) that hold the text range [a, b): [*m0, *m1).
// Members without text are taken where they lie at b, and from member 0 when a is 0 (in front of a > 0 they are the range
// before's), so that a file cut into ranges that tile its text has every member inflated by somebody, the 28-byte end-of-file
// member included.
void bgzf_members_for(const uint64_t *out_off, uint64_t n_members, uint64_t a, uint64_t b, uint64_t *m0, uint64_t *m1);
// Where n pieces of text, piece k the range [sa[k], sb[k]) of its file, lie in one staging buffer: each at the next multiple of
// 16 plus its text position modulo 16, off[k] = ((cursor + 15) & ~15) + (sa[k] & 15), so that a piece is aligned as its text is.
// Returns the buffer's size: the last piece's end and 32 bytes of room behind it.
uint64_t shard_stage_place(const uint64_t *sa, const uint64_t *sb, uint64_t n, uint64_t *off);

} // namespace crass

// 1. Opens a load (no reads resident from here on), stages the text of [lo, hi) into scratch — plain bytes from the host, of a
//    BGZF file the members that overlap the range, inflated — and probes every piece.  A decline met here (a member that does
//    not inflate, a BGZF text whose byte 0 is neither '>' nor '@') goes into *v with CRASS_OK: the pieces in front of that
//    file are staged and probed all the same, the ones behind it are not.
//    wrapped (the second attempt of a class-1 group, fastx_scan.h): a piece [a, b) of a file whose format is '@' is staged up to
//    min(n_text, b + margin) and is not probed: its line table and its chain are built (k_fw_cut_*) and stay for shard_cut_exit.
int shard_stage_probe(crass_hip_ctx *c, const crass::ShardFile *files, uint32_t n_files, crass::ShardPos lo, crass::ShardPos hi,
                      std::vector<crass::ShardPiece> *pieces, crass::ShardVerdict *v, bool wrapped = false, uint64_t margin = 0);
// 1b. Between the barriers, on rank 0's thread while the rank's own waits: where the chain that enters the rank's wrapped-mode
//    piece of the file at record start e (a <= e < b) leaves it.  *kind FW_CUT_LANDED: *pos is the first record start at or behind
//    b, or n_text; FW_CUT_OFFENCE: *off is the offending record's word, in the file's positions.  A chain that is unresolved at
//    the staged end has the piece staged again with twice the margin, as often as it takes (bounded by the file's size).
int shard_cut_exit(crass_hip_ctx *c, const crass::ShardFile *files, uint32_t file, uint64_t e, uint32_t *kind, uint64_t *pos, uint64_t *off);
// the look-ups and margin doublings of the rank since its last shard_stage_probe, and (timed contexts) its cut kernels' event time
void shard_cut_counters(const crass_hip_ctx *c, uint64_t *lookups, uint64_t *doublings, float *ms);
// 2. The actual range [lo, hi) as slices on the rank's arena (the staged bytes device to device, the tail behind them from the
//    host or from further BGZF members), each followed by a '\n', scanned by the three scan kernels — with wrapped, a FASTQ
//    slice that the four-line scan declines for its shape by the wrapped scan (launch_fw_*), as a single context's class 1.  file_reads: (file, records)
//    per slice.  Declines go into *v with CRASS_OK; n_reads is then not to be used.
int shard_scan(crass_hip_ctx *c, const crass::ShardFile *files, uint32_t n_files, crass::ShardPos lo, crass::ShardPos hi,
               std::vector<std::pair<uint32_t, uint64_t>> *file_reads, uint64_t *n_reads, uint32_t *max_len, crass::ShardVerdict *v,
               bool wrapped = false);
// 3. One pack launch over the scanned text, the header ids and the name table on the arena; every scratch goes back.
int shard_pack(crass_hip_ctx *c, int pad_uniform, uint64_t read_index_base);
// ... or nothing: the scratch goes back, no reads, no arena
void shard_abort(crass_hip_ctx *c);
// the arena and the records of the last shard_pack (CRASS_ERR_STATE: there is none)
int shard_records(const crass_hip_ctx *c, const uint8_t **arena, uint64_t *n_bytes, const uint64_t **rec_pos, uint64_t *n_reads);
// how many answers of the last crass_hip_fastx_names_find_device named a record (counted on the device: the answers stay there)
uint64_t names_find_device_found(const crass_hip_ctx *c);
#pragma GCC visibility pop

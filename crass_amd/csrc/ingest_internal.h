// ingest_internal.h — what crosses the files of the device ingest, each declared once: engine_ingest.cpp (the scratch given
// back, packed reads and text in, text out), engine_fastx.cpp (the scan and the FASTA / FASTQ loaders), engine_inflate.cpp
// (BGZF and gzip inflate), engine_names.cpp (header ids, the name table, header lines, quality, comments) and engine_shards.cpp (one
// rank's steps of a group's files load, declared in fastx_shards.h).  The context and its Ingest member are engine_ctx.h.
// Host only: no .hip file includes this.
#pragma once
#include "engine_ctx.h"
#include "pack_launch.h"
#include "fastx_names_launch.h"
#include "inflate_launch.h"
#include "gunzip_launch.h"
#include "fastx_shards.h"

#include <new>

#pragma GCC visibility push(hidden)
namespace crass {

// what the gzip count step and the chain walk decided about one file: all the decode step needs beside the bytes
struct GzState {
    GzMember M{};
    std::vector<uint64_t> start, text_len, end_bit;
    std::vector<uint32_t> link, chain;
    std::vector<int32_t> reason;
    uint64_t n_chain = 0, n_text = 0;
    // members mode (gunzip_core.h): what count reported about member ends, and after the decode step the member table
    bool members = false;
    uint64_t n_file = 0;
    std::vector<uint32_t> n_ends;
    std::vector<uint64_t> last_end, in_off, text_off;
};

struct ScanResult {
    std::vector<uint64_t> rbase;                        // piece i's records are [rbase[i], rbase[i + 1])
    uint64_t n_reads = 0, total_seq = 0, max_len = 0;
    // CRASS_ERR_UNSUPPORTED with decline_file >= 0: the input is declined, the position counts from that piece's first byte
    int32_t decline_file = -1, decline_reason = 0; uint64_t decline_pos = 0;
};

// The scan of an arena of pieces (engine_fastx.cpp): one file or several, or the slices of a shard, whose text lies on the
// device, piece i at arena + base[i] with a byte of room behind it: base[i + 1] = base[i] + its size + 1 (a file on its own:
// base = {0, n + 1}).  x_tot / x_h_tot hold 5 words per piece PLANNED: [4 i ..) piece i's totals, [4 n_planned + i] its verdict.
//   open   the tile bases; x_tiles / x_base sized for all tiles, x_tot / x_h_tot for the planned pieces; tm_scan's first mark
//   queue  piece i's first two kernels, as soon as its text is there; newline: the '\n' into the byte of room behind it
//          (the one caller whose bytes are not its own stores none)
//   emit   the totals of the n_kept first pieces back, every one of them emits into one text and one pair of per-record
//          arrays, tm_scan's second mark, the verdict: the first piece in order that offends.  max_reads: a set of that many
//          records or more is CRASS_ERR_UNSUPPORTED (the files' name table holds 32-bit indices)
//   wrapped  set between open and emit by the callers that honour crass_hip_set_fastq_class (a shard's slices: in the wrapped
//          pass of a class-1 group only): emit
//          hands the FASTQ pieces the four-line scan declined for their shape to emit_wrapped, whose verdict is theirs
struct ArenaScan {
    const uint8_t *arena = nullptr; const uint64_t *base = nullptr;
    bool wrapped = false;
    int emit_wrapped(crass_hip_ctx *c, uint32_t n_kept, uint64_t max_reads, const std::vector<int32_t> &w_of, uint32_t n_w,
                     std::vector<uint64_t> &tbase, ScanResult &R);
    std::vector<uint64_t> tile0; std::vector<FxJob> jobs;      // (jobs.size(): the pieces planned)
    int open(crass_hip_ctx *c, const uint8_t *arena_, const uint64_t *base_, uint32_t n_pieces);
    int queue(crass_hip_ctx *c, uint32_t i, int32_t format, bool newline);
    int emit(crass_hip_ctx *c, uint32_t n_kept, uint64_t max_reads, ScanResult &R);
};

} // namespace crass

// (C linkage and hidden, as the block at the end of engine_ctx.h)
extern "C" {
// engine_ingest.cpp: the name table, the comment structure and the arena go; each stage's scratch goes back, after a wait for the streams that may
// still use it; what opens a load; packed text in
void names_drop(crass_hip_ctx *c);
void comments_drop(crass_hip_ctx *c);
void drop_arena(crass_hip_ctx *c);
void wait_main(crass_hip_ctx *c);
void release_text(crass_hip_ctx *c);
void release_scan(crass_hip_ctx *c);
void release_bgzf(crass_hip_ctx *c);
void release_gzip(crass_hip_ctx *c);
void release_header_ids(crass_hip_ctx *c);
void release_names_find(crass_hip_ctx *c);
void release_names_of(crass_hip_ctx *c);
void release_lines(crass_hip_ctx *c, LineFetch &B);
void release_comments_build(crass_hip_ctx *c);
void release_shard(crass_hip_ctx *c);
void begin_fastx_load(crass_hip_ctx *c);
void reset_results_keep_set(crass_hip_ctx *c);
int load_text_impl(crass_hip_ctx *c, const uint8_t *h_seqs, const uint8_t *d_seqs, const uint64_t *off, uint64_t n, int pad_uniform,
                   const uint64_t *header_id, uint64_t read_index_base);
int upload_staged(crass_hip_ctx *c, const uint8_t *h_bytes, uint64_t n, uint8_t *dst);
// engine_fastx.cpp: what makes a scanned arena the resident set
int arena_finish(crass_hip_ctx *c, const uint8_t *arena, uint64_t n_arena_bytes, uint64_t n_reads, int pad_uniform, uint64_t read_index_base);
// engine_inflate.cpp
int inflate_bgzf_members(crass_hip_ctx *c, const uint8_t *d_in, const crass_bgzf_index *ix, uint64_t m0, uint64_t n, uint8_t *d_out,
                         crass_bgzf_verdict *v);
int gzip_count_impl(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, GzState &S, crass_gzip_plan *plan,
                    crass_bgzf_verdict *v, bool members = false);
int gzip_decode_impl(crass_hip_ctx *c, const uint8_t *d_in, GzState &S, uint8_t *d_out, crass_bgzf_verdict *v);
// engine_names.cpp
int header_ids_device_impl(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n,
                           uint64_t *header_id_out, int install, uint64_t *n_repeated_out);
} // extern "C"
#pragma GCC visibility pop

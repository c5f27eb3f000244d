// fastx_names_launch.h — the job descriptions and launch wrappers of fastx_hid.hip (the name table: header ids, name lookups) and
// fastx_lines.hip (names, header lines, quality strings and handed comments of listed records) over the raw bytes of a FASTA /
// FASTQ file on the device, for the engine.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace crass {

static constexpr unsigned long long kHidEmpty = ~0ull;      // a free slot of the name table
static constexpr uint64_t kHidNotFound = ~0ull;             // CRASS_NAME_NOT_FOUND

// k_hid_insert / k_hid_insert_long / k_hid_lookup
struct HidJob {
    const uint8_t *bytes;            // device pointer, any alignment; [bytes, bytes + n_bytes) is all that is ever read
    uint64_t n_bytes;
    const uint64_t *rec_pos;         // [n_reads] position of every record's header character
    uint64_t n_reads;                // < 2^32 - 1
    unsigned long long *table;       // [mask + 1] {hash tag : 32 | read index : 32}, kHidEmpty before the insert launch
    uint64_t mask;                   // slots - 1, slots a power of two >= 2 n_reads
    uint32_t hash_bits;              // 64, or fewer: only that many low bits of the hash are kept (tests)
    uint64_t *ids;                   // [n_reads] insert: the record's slot; lookup: its header id
    uint32_t *long_list;             // [n_reads] the records whose name is beyond kHidLaneMax bytes (k_hid_insert -> k_hid_insert_long)
    uint32_t *ctl;                   // [4] 0: entries of long_list, 1: a rec_pos at or beyond n_bytes was seen
    unsigned long long *n_repeated;  // reads with ids[r] != r (k_hid_lookup)
};
uint32_t hid_lane_max();
hipError_t launch_hid_insert(const HidJob &J, hipStream_t st);
hipError_t launch_hid_insert_long(const HidJob &J, uint32_t n_long, hipStream_t st);
hipError_t launch_hid_lookup(const HidJob &J, hipStream_t st);

// k_hid_find / k_hid_find_long: queries against a table k_hid_insert(_long) filled; everything is read but first_out
struct HidFindJob {
    const uint8_t *bytes; uint64_t n_bytes;      // the file the table was built on
    const uint64_t *rec_pos;                     // [n_reads] as at the insert: every entry < n_bytes
    const unsigned long long *table; uint64_t mask; uint32_t hash_bits;
    const uint8_t *names;                        // device copy of the queries, any alignment; query k is [name_off[k], name_off[k + 1])
    const uint64_t *name_off;                    // [n_names + 1], not decreasing
    uint64_t n_names;
    const uint32_t *long_list;                   // the queries of hid_lane_end() bytes or more, listed by the host
    uint64_t *first_out;                         // [n_names] the smallest record index with that name, or kHidNotFound
};
uint32_t hid_lane_end();                         // names of this many bytes or more are hashed and compared by the wave kernels
hipError_t launch_hid_find(const HidFindJob &J, hipStream_t st);
hipError_t launch_hid_find_long(const HidFindJob &J, uint32_t n_long, hipStream_t st);
// k_hid_find_dev: k_hid_find for queries whose offsets nobody on the host has seen.  J.names, J.name_off and J.first_out are the
// caller's device memory; the kernel checks every offset pair against n_name_bytes, answers the short queries and lists the
// long ones itself (long_app, the J.long_list of the launch_hid_find_long that follows once the host has read ctl[0])
struct HidFindDev {
    uint64_t n_name_bytes;                       // name_off[k] <= name_off[k + 1] <= this, else the query is bad
    uint32_t *long_app;                          // [n_names] the queries of hid_lane_end() bytes or more, in any order
    uint32_t *ctl;                               // [2] 0: entries of long_app, 1: a bad offset pair was seen; both 0 before the launch
};
hipError_t launch_hid_find_dev(const HidFindJob &J, const HidFindDev &D, hipStream_t st);
// *count += the answers of first[0, n) that are not kHidNotFound
hipError_t launch_hid_count_found(const uint64_t *first, uint64_t n, unsigned long long *count, hipStream_t st);

// k_nm_measure_idx / k_nm_scan_* / k_nm_copy: the names of listed records of a built table, back to back, all in device memory
struct NmOfJob {
    const uint8_t *bytes; uint64_t n_bytes;      // the file the table was built on
    const uint64_t *rec_pos; uint64_t n_reads;   // [n_reads] as at the insert: every entry < n_bytes
    const uint64_t *idx; uint64_t n;             // [n] entry k is record idx[k] - idx_base, any order, repeats allowed
    uint64_t idx_base;
    uint32_t *len;                               // [n] k_nm_measure_idx: the name's bytes; 0 for an entry outside [0, n_reads)
    uint32_t *flag;                              // set to 1 by such an entry; 0 before the launch
    uint64_t *tile_sum;                          // [tiles + 1] k_nm_scan_tiles: a tile's bytes; k_nm_scan_top: the bytes in front of it
    uint64_t *off;                               // [n + 1] k_nm_scan_apply: where the names lie in out; off[n] the total
    uint8_t *out; uint64_t limit;                // k_nm_copy: min(off[n], the capacity of out) — nothing at or beyond out + limit is written
};
uint32_t nm_scan_tile();                         // entries per tile of the prefix sum
hipError_t launch_nm_measure_idx(const NmOfJob &J, hipStream_t st);
hipError_t launch_nm_scan(const NmOfJob &J, hipStream_t st);        // the three launches: tile sums, one block over them, apply
hipError_t launch_nm_copy(const NmOfJob &J, hipStream_t st);

// k_span_copy: entry a's bytes are bytes[start[a] ...), as many as off[a + 1] - off[a], and go to out + off[a] (header lines,
// handed comments)
struct SpanCopyJob {
    const uint8_t *bytes; uint64_t n_bytes;      // no byte at or beyond n_bytes is read
    const uint64_t *start;           // [n]
    const uint64_t *off;             // [n + 1] not decreasing from 0
    uint64_t n;                      // >= 1
    uint64_t total;                  // off[n]
    uint8_t *out;                    // [total], any alignment
};
hipError_t launch_span_copy(const SpanCopyJob &J, hipStream_t st);

// k_hl_measure; the copy is k_span_copy from src
struct HlJob {
    const uint8_t *bytes; uint64_t n_bytes;
    const uint64_t *src;             // [n] position of the first byte behind the record's header character (<= n_bytes)
    uint64_t n;
    uint32_t *line_len, *name_len;   // [n] k_hl_measure
};
hipError_t launch_hl_measure(const HlJob &J, hipStream_t st);

// k_ql_measure / k_ql_copy: the quality strings of selected records
struct QlJob {
    const uint8_t *bytes; uint64_t n_bytes;
    const uint64_t *src;             // [n] position of the record's header character (< n_bytes)
    const uint64_t *lim;             // [n] where the record ends: the next record's header character, or the end of the last file
    uint64_t n;
    uint64_t *start;                 // [n] k_ql_measure: position of the first byte of the record's fourth line
    uint32_t *len, *flags;           // [n] its bytes 33..126; bit 0: a FASTQ record, bit 1: those bytes lie back to back at start
    const uint64_t *off;             // [n + 1] k_ql_copy: where the records lie in out
    uint64_t total;                  // off[n]
    uint8_t *out;                    // [total], any alignment
};
hipError_t launch_ql_measure(const QlJob &J, hipStream_t st);
hipError_t launch_qw_measure(const QlJob &J, hipStream_t st);      // FASTQ class 1: start / len by the wrapped rule, the same copy
hipError_t launch_ql_copy(const QlJob &J, hipStream_t st);

// k_cm_bits / k_cm_tiles / k_cm_top: the own-comment bitmap of a file's records and the carry of every tile of kFxCmTile
// (fastx_scan.h) records
struct CmBuildJob {
    const uint8_t *bytes; uint64_t n_bytes;
    const uint64_t *rec_pos; uint64_t n_reads;   // [n_reads] position of every record's header character (scratch of the build)
    uint64_t *bits;                              // [(n_reads + 63) / 64] bit r & 63 of word r >> 6: record r has a comment of its own
    uint64_t *carry;                             // [tiles] 1 + the last such record in the tiles up to and including this one, 0: none
    uint64_t *tile_cnt;                          // [tiles + 1] scratch: such records per tile, [tiles] their total
    uint32_t *flag;                              // set to 1 by a rec_pos at or beyond n_bytes; 0 before the launch
};
hipError_t launch_cm_build(const CmBuildJob &J, hipStream_t st);      // the three launches

// k_cm_source / k_cm_measure: the comments handed to listed records; the copy is k_span_copy from start
struct CmFetchJob {
    const uint8_t *bytes; uint64_t n_bytes;
    const uint64_t *bits, *carry; uint64_t n_reads;      // as built
    const uint64_t *file_read_base; uint32_t n_files;    // [n_files + 1] from 0 to n_reads, not decreasing
    const uint64_t *idx; uint64_t n;             // [n] local record numbers, any order, repeats allowed
    uint64_t *src;                               // [n] k_cm_source: the record whose own comment entry k is handed, ~0: none
    const uint64_t *pos;                         // [n] k_cm_measure: the first byte behind that record's header character, ~0: none
    uint64_t *start; uint32_t *len;              // [n] k_cm_measure: where the comment starts and its bytes
};
hipError_t launch_cm_source(const CmFetchJob &J, hipStream_t st);
hipError_t launch_cm_measure(const CmFetchJob &J, hipStream_t st);

} // namespace crass

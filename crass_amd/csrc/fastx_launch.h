// fastx_launch.h — the device record scan's job description and launch wrappers (fastx_scan.hip), for the engine.  Not part
// of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "fastx_scan.h"

namespace crass {

// Positions are counted twice: FILE positions 0 .. n (64-bit), and positions in "aligned space", which starts at the 16-byte
// aligned address at or below the bytes: aligned position = lead + file position, lead = address of byte 0 modulo 16.  A tile is
// kFxTileBytes of aligned space, so every lane's vector is an aligned 16-byte load whatever the bytes' own alignment.

// what a tile knows about itself without its neighbours (k_fx_summary)
struct FxTile {
    uint32_t n_ls;          // line starts in the tile
    uint32_t lls;           // the last of them: ((offset in the tile + 1) << 1) | (its first byte is '>'); 0: the tile starts no line
    uint32_t lead_g;        // bytes 33..126 in front of the tile's first line start (the tail of a line of an earlier tile)
    uint32_t n_hdr;         // FASTA: line starts whose byte is '>'
    uint32_t c01, c23;      // bytes 33..126 in the lines that start in the tile; FASTA: c0 = those of sequence lines;
                            // FASTQ: c_r = those of the lines whose index AMONG THE TILE'S OWN is r modulo 4 (16 bits each)
};
// what the scan over the tiles adds (k_fx_tile_scan): everything in front of the tile
struct FxBase {
    uint64_t ls_before;     // line starts = index of the first line that starts in the tile
    uint64_t carry_ls;      // file position of the last of them (the line the tile's first bytes belong to)
    uint64_t rec_before, seq_before, qual_before;      // records, sequence bytes, quality bytes (FASTQ)
    uint32_t carry_kind;    // FxKind of that line
    uint32_t pad;
};

struct FxJob {
    const uint8_t *bytes;   // device pointer, any alignment
    uint64_t n;             // > 0
    uint32_t lead;          // address of bytes modulo 16
    int32_t format;         // '>' | '@' (byte 0)
    uint64_t n_tiles;
    FxTile *tiles; FxBase *base;
    uint64_t *tot;          // [4] lines, records, sequence bytes, quality bytes (k_fx_tile_scan)
    // k_fx_emit
    uint64_t n_lines, n_reads, text_cap;
    uint8_t *text;          // [text_cap] the reads' bytes back to back (16-byte aligned)
    uint64_t *rec_pos, *seq_off;      // [n_reads]
    unsigned long long *verdict;      // the smallest fx_offence, kFxNoOffence before the launch
    // several files into one set (crass_hip_load_fastx_files; all 0 for a file on its own): this file's record r is entry
    // read_base + r of rec_pos / seq_off, its sequence bytes start at text[text_base] (text_cap: where they end), and rec_pos holds
    // arena_base + the file position.  Offences stay in file positions.
    uint64_t text_base, read_base, arena_base;
};
// k_fx_cut_probe: the probe of fastx_scan.h over bytes[0, n) (device pointer, any alignment).  fx_probe_plan fills everything
// but part, which the caller points at n_blocks FxProbe of device memory; fx_probe_fold folds their host copy.
static constexpr uint32_t kFxProbeMaxBlocks = 1024;
struct FxProbeJob {
    const uint8_t *bytes; uint64_t n;
    uint32_t lead, left_is_ls;      // address of bytes modulo 16; whether position 0 is a line start
    uint64_t n_tiles, tiles_per_block;
    uint32_t n_blocks;
    FxProbe *part;
};
void fx_probe_plan(const uint8_t *bytes, uint64_t n, uint32_t left_is_ls, FxProbeJob *P);
void fx_probe_fold(const FxProbe *part, uint32_t n_blocks, FxProbe *out);
hipError_t launch_fx_cut_probe(const FxProbeJob &P, hipStream_t st);
uint32_t fastx_tile_bytes();
uint64_t fastx_n_tiles(const uint8_t *bytes, uint64_t n);
hipError_t launch_fx_summary(const FxJob &J, hipStream_t st);
hipError_t launch_fx_tile_scan(const FxJob &J, hipStream_t st);
hipError_t launch_fx_emit(const FxJob &J, hipStream_t st);

// ---- the wrapped FASTQ scan (fastx_wrapped.hip; fastx_scan.h states the rule) ----
// A table of the LINES (where each starts, its first byte, and how many bytes 33..126, bytes 127 and bytes '>' '@' '+' lie in
// front of it), every '@' line's successor under the rule, the lines reachable from line 0 by pointer doubling, their ranks and
// text offsets, then the sequence bytes out.  Line indices are 32-bit; END is n_lines.
struct FwTile { uint32_t n_ls, n_pl, g, d, f; };        // a tile's line starts, those whose byte is '+', bytes 33..126, 127, forbidden
struct FwBase { uint64_t ls, pl, g, d, f; };            // the same in front of the tile
static constexpr uint32_t kFwRankTile = 1024;            // lines per block of the rank scan
static constexpr uint32_t kFwTot = 8;                    // words of FwJob::tot
struct FwJob {
    const uint8_t *bytes; uint64_t n;                   // device pointer of any alignment, n > 0
    uint32_t lead, ends_nl;                             // address modulo 16; the last byte is a '\n'
    uint64_t n_tiles;
    FwTile *tiles; FwBase *base;                        // [n_tiles]
    uint64_t *tot;          // [kFwTot] lines, '+' lines, bytes 33..126, 127, forbidden (k_fw_tile_scan); records, sequence bytes
                            // (k_fw_rank_top); the verdict (kFxNoOffence before k_fw_rank_apply)
    uint32_t n_lines;       // tot[0], read back: the arrays below are sized by it
    uint64_t *pos, *G, *D, *F;        // [n_lines + 1] the line's first byte; the three counts in front of it (entry n_lines: n, the totals)
    uint8_t *first;         // [n_lines] the line's first byte
    uint32_t *plus;         // [n_lines] the lines that start with '+', in order (tot[1] of them)
    uint32_t *nxt[2];       // [n_lines + 1] the successor arrays of the doubling, in turns
    uint32_t *mark;         // [n_lines + 1] the line is a header reachable from line 0
    uint32_t *plus_of;      // [n_lines] a header candidate's '+' line
    uint64_t *seqlen, *off; // [n_lines] a candidate's sequence bytes and its offence word (kFxNoOffence: none)
    uint32_t *rank;         // [n_lines] marked lines in front
    uint64_t *seqpre;       // [n_lines] their sequence bytes
    uint64_t *tile_cnt, *tile_len;    // [n_rank_tiles + 1] the rank scan's tiles
    uint32_t *hdr;          // [n_lines] record r's header line
    uint64_t *delta;        // [n_lines] a sequence line of a marked record: where in the text its first byte 33..126 goes; else kFxNone
    // k_fw_place / k_fw_emit: as FxJob's
    uint64_t n_reads, text_cap, text_base, read_base, arena_base;
    uint8_t *text; uint64_t *rec_pos, *seq_off;
};
// the scratch of one piece in 64-bit words (everything above but the bytes), and the job's pointers laid into it
uint64_t fw_scratch_words(uint64_t n_tiles, uint64_t n_lines);
void fw_lay_out(FwJob &J, uint64_t *scratch);
hipError_t launch_fw_tiles(const FwJob &J, hipStream_t st);      // k_fw_summary, k_fw_tile_scan: tot[0 .. 5)
hipError_t launch_fw_analyse(const FwJob &J, hipStream_t st);    // k_fw_lines, k_fw_next, k_fw_jump rounds, the rank scan: tot[5 .. 8)
hipError_t launch_fw_emit(const FwJob &J, hipStream_t st);       // k_fw_place, k_fw_emit
// the cut of a group's files load: the job is a piece [a, b) of a wrapped file with a margin staged behind it, positions counted
// from a.  What a look-up says of the chain that starts at a record start of the piece:
// (FwCutKind, fastx_scan.h)
struct FwCut { uint64_t b; uint32_t at_eof, first_cand; };      // the piece's end; the staged bytes end the file; 1: position 0 is no line start
// k_fw_lines, k_fw_cut_next, the k_fw_cut_jump rounds (after launch_fw_tiles and with n_lines read back); *which: the nxt array that holds the terminals
hipError_t launch_fw_cut(const FwJob &J, const FwCut &K, hipStream_t st, uint32_t *which);
// k_fw_cut_lookup: d_out[3] = kind, the terminal's position, its offence word
hipError_t launch_fw_cut_lookup(const FwJob &J, uint32_t which, uint64_t p, uint64_t *d_out, hipStream_t st);

} // namespace crass

// fastx_scan.h — what the host restatement (fastx_scan.cpp), the device scan (fastx_scan.hip) and the engine (engine_fastx.cpp)
// share about finding the records of a FASTA / FASTQ file by LINES: the byte classes, the line kinds, the decline reasons and
// the order in which offences are reported.  Plain C++ with CRASS_HD (pack_text.h), so the rule exists once for host and
// device.  Not part of the public ABI (the reasons' VALUES are: include/crass_hip.h names them).
//
// kseq (kseq.cpp:171-226) is a byte-stream parser: '>', '@' or '+' ANYWHERE in a sequence ends it.  A scan by lines agrees with
// it on the regular class only, and declines everything else:
//   regular FASTA   byte 0 is '>'; a line whose first byte is '>' is a header line; every other line is a sequence line and
//                   holds none of '>' '@' '+'; the file does not end with a '>' that is the first byte of its line.
//   regular FASTQ   byte 0 is '@'; the number of lines is a multiple of 4; line 4k starts with '@', line 4k+1 holds none of
//                   '>' '@' '+', line 4k+2 starts with '+', line 4k+3 holds no byte 127 and as many bytes in 33..126 as line 4k+1.
// Lines are the pieces between '\n' bytes (the last may lack its '\n'; an empty piece after a final '\n' is no line).  A read is
// the bytes 33..126 of its record's sequence lines.
//
// The verdict of a declined input is the SMALLEST (position of the line, reason) pair over all offences of all lines: both
// scans evaluate every offence of a line, so the first offending line and, within it, the smallest reason value win.
#pragma once
#include <stdint.h>
#include "pack_text.h"

namespace crass {

// decline reasons (crass_fastx_layout.decline_reason); 0: accepted
enum FxReason : int32_t {
    FX_OK = 0,
    FX_EMPTY = 1,            // n_bytes == 0: no format to report
    FX_FIRST_BYTE = 2,       // byte 0 is neither '>' nor '@' (junk in front)
    FX_LINE_COUNT = 3,       // FASTQ: the lines are no multiple of 4; position: the first line of the incomplete record
    FX_FQ_HEADER = 4,        // FASTQ: line 4k does not start with '@' (a '>' record, a trailing blank line, multi-line records)
    FX_SEQ_CHAR = 5,         // '>' '@' or '+' in a sequence line (FASTA: a line that does not start with '>'; FASTQ: line 4k+1)
    FX_FQ_PLUS = 6,          // FASTQ: line 4k+2 does not start with '+'
    FX_QUAL_DEL = 7,         // FASTQ: byte 127 in a quality line (kseq counts it as a quality byte)
    FX_QUAL_SHORT = 8,       // FASTQ: the quality line holds fewer bytes in 33..126 than the sequence line
    FX_QUAL_LONG = 9,        // FASTQ: ... more
    FX_LONE_HEADER = 10,     // FASTA: the last byte is a '>' that starts its line (kseq finds no record there)
    FX_READ_TOO_LONG = 11,   // accepted by the scan, refused by the layout: a read beyond CRASS_HIP_MAX_READ_LEN (the load calls only)
    FX_FQ_EMPTY_SEQ = 12     // wrapped FASTQ: an empty sequence whose '+' line is followed by a line that starts with '@' (kseq.cpp:217 consumes that byte)
};

// ---- wrapped FASTQ (class 1: crass_fastx_scan_host_class, crass_hip_set_fastq_class) ----
// Byte 0 is '@'; lines as above.  A VOID line holds no byte in 33..127.  A record is
//   a header line, whose first byte is '@';
//   zero or more sequence lines, none holding '>' '@' or '+';
//   the first following line whose first byte is '+' (the rest of it is ignored); it ends with a '\n';
//   quality lines: with L the record's sequence bytes, the lines behind the '+' line up to the first line END at which their
//   bytes 33..126 are L or more (L == 0: none) — and there they must be exactly L;
//   any number of void lines;
//   the next record's header line, or the end of the input.
// This is what kseq_read (kseq.cpp:171-226) reads record by record without losing a byte: its quality loop counts the bytes
// 33..127 and swallows ONE byte behind the last one — a '\n' here, or the end of the input.
// Offences of ONE record in the order they are looked for; the first found is the record's, the position is the first byte of
// the line named:
//    3  no line behind the header starts with '+'                                   the header line
//    5  '>' '@' or '+' in a sequence line                                           the first such line
//   12  L == 0 and the line behind the '+' line starts with '@'                     that line
//    7  byte 127 in a quality line (the one the count passes L in included)         the first such line
//    9  the count passes L inside a line                                            that line
//    8  the input ends before the count is L, or inside the '+' line                the header line
//    4  the first line behind the quality that is not void does not start with '@'   that line
// Only the records REACHABLE from line 0 are judged, each from where the one before ended: a quality line that starts with
// '@' is no header, and what it would offend as one is nobody's business.  The verdict is the first reachable record's that
// offends.  Every regular (four-line) FASTQ is in this class, with the same records.
enum FxFastqClass : int32_t { FX_CLASS_FOUR_LINE = 0, FX_CLASS_WRAPPED = 1 };
CRASS_HD inline bool fx_is_void_byte(uint8_t b) { return b < 33 || b > 127; }                       // a void line holds only these
// the four-line scan's declines that the wrapped scan takes up: every one a FASTQ earns by its shape.  (Not only 3, 4, 6, 8
// and 9: "@r\n+\n\n" puts a '+' line where line 4k+1 should be, reason 5, and a header line of a later record may lie where
// a quality line should and hold a byte 127, reason 7 — both are wrapped FASTQ.)
CRASS_HD inline bool fx_wrapped_takes(int32_t reason) { return reason >= FX_LINE_COUNT && reason <= FX_QUAL_LONG; }

// the kind of a line.  FASTA: header or sequence; FASTQ: the line's index modulo 4 — so 0 is a header and 1 a sequence line in both
enum FxKind : uint32_t { FX_HEADER = 0, FX_SEQ = 1, FX_PLUS = 2, FX_QUAL = 3 };

// ---- byte classes ----
CRASS_HD inline bool fx_is_nl(uint8_t b) { return b == 0x0A; }
CRASS_HD inline bool fx_is_hdr_char(uint8_t b) { return b == 0x3E || b == 0x40; }                  // '>' '@'
CRASS_HD inline bool fx_is_forbidden(uint8_t b) { return b == 0x3E || b == 0x40 || b == 0x2B; }      // '>' '@' '+': ends kseq's sequence
CRASS_HD inline bool fx_is_seq_byte(uint8_t b) { return b >= 33 && b <= 126; }                       // isgraph(): what kseq keeps
CRASS_HD inline bool fx_is_del(uint8_t b) { return b == 127; }

// the same classes for four bytes at once (byte 0 = bits 0..7): bit i of a result says byte i is in the class
struct FxClass4 { uint32_t nl, gt, at, plus, del, graph; };
CRASS_HD inline uint32_t fx_gather4(uint32_t high_bits)      // bits 7, 15, 23, 31 -> bits 0 .. 3
{
    return ((high_bits >> 7) * 0x10204080u) >> 28;           // (the partial products meet in no bit: pack_code4)
}
CRASS_HD inline uint32_t fx_eq4(uint32_t v, uint32_t c)     // bytes equal to c, exact for all 256 values
{
    const uint32_t z = v ^ (c * 0x01010101u);
    const uint32_t nz = (((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
    return fx_gather4(nz ^ 0x80808080u);
}
CRASS_HD inline FxClass4 fx_class4(uint32_t v)
{
    FxClass4 c;
    c.nl = fx_eq4(v, 0x0Au); c.gt = fx_eq4(v, 0x3Eu); c.at = fx_eq4(v, 0x40u); c.plus = fx_eq4(v, 0x2Bu); c.del = fx_eq4(v, 0x7Fu);
    const uint32_t low = v & 0x7F7F7F7Fu;
    const uint32_t ge33 = (low + 0x5F5F5F5Fu) & 0x80808080u;               // low 7 bits >= 33 (at most 127 + 95: no carry into the next byte)
    const uint32_t is127 = (low + 0x01010101u) & 0x80808080u;              // low 7 bits == 127
    c.graph = fx_gather4(ge33 & ~is127 & ~(v & 0x80808080u));
    return c;
}

// one offence as a sortable word: the smallest over all offences is the verdict
CRASS_HD inline uint64_t fx_offence(uint64_t line_pos, uint32_t reason) { return (line_pos << 8) | reason; }
static const uint64_t kFxNoOffence = ~0ull;

// ---- cutting a job's files into record-aligned shards (crass_fastx_files_shards_host, crass_hip_group_load_fastx_files) ----
// TEXT SPACE: the files' texts back to back in file order, no byte between them (a BGZF file's text is its inflated text); T is
// its size.  NOMINAL cuts: n_ranks - 1 non-decreasing positions in [0, T] (by default T g / n_ranks); cut 0 is 0, cut n_ranks is T.
// A RECORD START is defined by lines alone, whether or not the file will be accepted: every file's position 0; in a file whose
// byte 0 is '>' every line start whose byte is '>'; in a file whose byte 0 is '@' every line start whose line index (the '\n' bytes
// in front of it in that file) is 0 modulo 4 — a quality line may start with '@', so nothing near the cut can tell.  A line start
// is position 0 or a position behind a '\n', and it is smaller than the file's text length.  A file of another first byte has no
// record start but 0 (the scan declines it with FX_FIRST_BYTE anyway).
// The ACTUAL cut c_g is the smallest record start at or after nominal cut g, or T: c_g <= c_{g+1}, a rank may be empty, rank g
// owns [c_g, c_{g+1}) — a tail of one file, whole files, a head of one file, each slice beginning at a record start.
//
// CLASS 1 (crass_fastx_files_shards_host_class, crass_hip_group_set_fastq_class): the record starts of a file whose byte 0 is '@'
// are the header-line positions of the records the wrapped rule above walks from line 0 (fastx_scan_class_serial's walk), and
// nothing else: a quality line may start with '@' and the lines behind it may parse as a complete record, which is not one of the
// file's.  FASTA files and files of another first byte keep the definition above, the actual cut stays "the smallest record
// start at or after the nominal cut, or T", and the verdict is crass_fastx_files_scan_host_class(.., 1, ..)'s whatever the cuts.
// So the cut cannot be made by looking near it.  Each rank builds, for its piece [a, b) of the file and a margin staged behind
// it, every '@' line's successor under the rule and doubles the pointers to where the chain leaves the piece (k_fw_cut_*,
// fastx_wrapped.hip); the host then walks the ranks in piece order: the entry e of the file's first piece is 0, a piece with
// e >= b is passed through (a record longer than the range), else the terminal of e's chain is looked up:
enum FwCutKind : uint32_t {
    FW_CUT_PASS = 0,        // (a line on the way: never a look-up's answer)
    FW_CUT_LANDED = 1,      // the chain's first record start at or beyond b, or the file's end: the piece's exit, the next one's entry
    FW_CUT_OFFENCE = 2,     // a record of the chain offends: the file's verdict, nothing behind it in the file is cut
    FW_CUT_UNRESOLVED = 3,  // a record's outcome depends on bytes beyond the staged end: the rank doubles its margin and builds again
    FW_CUT_NONE = 4         // the position starts no header line of the piece (never expected)
};
// c_g is the first exit at or after nominal cut g; an exit at the file's end is the next file's 0, or T.
//
// What a probe of a byte range [a, b) of ONE file's text reports (k_fx_cut_probe, and fx_probe_serial on the host), positions
// counted from a; kFxNone: there is none.  left_is_ls says whether position a is itself a line start (a == 0, or byte a - 1 is '\n').
static const uint64_t kFxNone = ~0ull;
struct FxProbe {
    uint64_t n_nl;           // '\n' bytes in the range
    uint64_t n_ls;           // how many of ls[] are there: min(4, line starts in the range)
    uint64_t ls[4];          // the range's first four line starts, ascending
    uint64_t gt;             // its first line start whose byte is '>'
};
// the first record start in the range from its probe: format is the file's byte 0, nl_before the '\n' bytes of the file in
// front of a (FASTQ: the k-th line start of the range is line nl_before + k, one more when a is no line start itself)
CRASS_HD inline uint64_t fx_probe_pick(const FxProbe &P, int32_t format, uint64_t nl_before, bool left_is_ls)
{
    if (format == 0x3E) return P.gt;
    if (format != 0x40) return kFxNone;
    const uint64_t first_idx = nl_before + (left_is_ls ? 0u : 1u);
    const uint64_t k = (0u - first_idx) & 3u;
    return k < P.n_ls ? P.ls[k] : kFxNone;
}
int fx_probe_serial(const uint8_t *bytes, uint64_t n, bool left_is_ls, FxProbe *out);      // the host restatement (fastx_scan.cpp)

// ---- the serial host restatement of the whole scan (fastx_scan.cpp) ----
// rec_pos / seq_off: malloc'd arrays of n_reads + 1 entries (free()), nullptr when the input is declined
struct FxHostScan {
    uint64_t n_reads = 0; int32_t format = 0, reason = 0; uint64_t decline_pos = 0; uint32_t max_len = 0;
    uint64_t *rec_pos = nullptr, *seq_off = nullptr;
};
int fastx_scan_serial(const uint8_t *bytes, uint64_t n_bytes, FxHostScan *out);      // CRASS_OK, CRASS_ERR_UNSUPPORTED (declined), CRASS_ERR_OOM
// the same for a FASTQ class: FX_CLASS_FOUR_LINE is fastx_scan_serial; FX_CLASS_WRAPPED walks a file whose byte 0 is '@' record
// by record under the wrapped rule (anything else, FASTA included, is fastx_scan_serial's)
int fastx_scan_class_serial(const uint8_t *bytes, uint64_t n_bytes, int32_t fastq_class, FxHostScan *out);

CRASS_HD inline bool fx_is_space(uint8_t b) { return b == 0x20 || (b >= 0x09 && b <= 0x0D); }       // isspace(): ends kseq's name

// ---- the comment kseq hands on (crass_fastx_comments_of, the k_cm_* kernels of fastx_lines.hip) ----
// A record's NAME is the bytes behind its header character up to the first fx_is_space() byte or the end of the file's text.
// The record has an OWN comment iff its name ends at a byte that exists and is not '\n' (kseq.cpp:179-186: the delimiter that
// ended the name decides whether the rest of the line is read).  The own comment is the bytes behind that delimiter up to, not
// including, the line's '\n' or the end of the text; it may be empty, and a '\r' in front of the '\n' stays in it.
// kseq never clears comment.s, so the comment HANDED to record r is the own comment of the last record r' <= r of the SAME
// file that has one; a record in front of its file's first comment is handed none.
// name_end: the position of the byte that ended the name, n_bytes: the end of the text, end_byte: that byte where it exists
CRASS_HD inline bool fx_own_comment(uint64_t name_end, uint64_t n_bytes, uint8_t end_byte) { return name_end < n_bytes && !fx_is_nl(end_byte); }

// the structure both sides look a record's source up in: one bit per record (bit r & 63 of word r >> 6: record r has an own
// comment) and one CARRY word per tile of kFxCmTile records: 1 + the last own-comment record in all tiles up to and including
// that one, 0 where there is none.  File boundaries are not in it: whoever looks up drops a source in front of the file's first
// record.  The last own-comment record at or in front of r, or kFxNone: r's own word masked to the bits at or below its
// position, then the earlier words of its tile (at most 63), then the carry of the tile in front.
static const uint64_t kFxCmTile = 4096;
CRASS_HD inline uint64_t fx_comment_source(const uint64_t *bits, const uint64_t *carry, uint64_t r)
{
    uint64_t w = r >> 6;
    const uint64_t tile = r / kFxCmTile, w0 = tile * (kFxCmTile / 64);
    uint64_t m = bits[w] & (~0ull >> (63u - (uint32_t)(r & 63u)));
    while (!m && w > w0) m = bits[--w];
    if (m) return w * 64 + (63u - (uint32_t)__builtin_clzll(m));
    if (tile == 0) return kFxNone;
    const uint64_t c = carry[tile - 1];
    return c ? c - 1 : kFxNone;
}
// the first record of the file that holds record r: file_read_base[0] == 0 <= r < file_read_base[n_files], not decreasing
// (files of no records share their base with the next)
CRASS_HD inline uint64_t fx_file_first_read(const uint64_t *file_read_base, uint32_t n_files, uint64_t r)
{
    uint32_t a = 0, b = n_files;                        // the last f with file_read_base[f] <= r
    while (a < b) {
        const uint32_t mid = (a + b + 1) >> 1;
        if (file_read_base[mid] <= r) a = mid; else b = mid - 1;
    }
    return file_read_base[a];
}
// what r is handed: its source unless that lies in front of its file's first record
CRASS_HD inline uint64_t fx_comment_handed_from(const uint64_t *bits, const uint64_t *carry, const uint64_t *file_read_base, uint32_t n_files, uint64_t r)
{
    const uint64_t src = fx_comment_source(bits, carry, r);
    return src != kFxNone && src >= fx_file_first_read(file_read_base, n_files, r) ? src : kFxNone;
}

} // namespace crass

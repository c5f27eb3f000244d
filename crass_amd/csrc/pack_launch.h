// pack_launch.h — the device packer's job description and launch wrappers (pack.hip), for the engine.  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "pack_text.h"
#include "engine_internal.h"

namespace crass {

// ---- the device packer (pack.hip) ----
// One launch packs the words [w_begin, w_end) of the set, which belong to the reads [r_begin, r_end) (a chunk boundary falls
// between reads); words of that range that belong to no read — the padding of a stride, the four tail words — are written as
// zero.  Read r's text is text[off(r) - bias .. off(r + 1) - bias).
struct PackJob {
    const uint8_t *text;            // device pointer, any alignment
    uint64_t bias;                  // offset (in the caller's numbering) of text[0]
    const uint64_t *off;            // device, [n_reads + 1] offsets in the caller's numbering; nullptr: off(r) = uni_base + r * uni_len
    uint64_t uni_base;
    uint32_t uni_len;
    uint32_t stride_words;          // > 0: read r starts at word r * stride_words; 0: at word_off[r]
    const uint64_t *word_off;       // device, [n_reads + 1] (stride_words == 0)
    uint64_t r_begin, r_end;
    uint64_t w_begin, w_end;
    uint32_t *out;                  // the set's word 0 (16-byte aligned; w_end rounded up to 4 words is inside the buffer)
    uint32_t *exc_mask;             // bit per read, cleared by the caller: set for every read with a byte outside ACGT
};
hipError_t launch_pack_text(const PackJob &J, hipStream_t st);
// exc_bytes[exc_off[e] .. exc_off[e + 1]) = the text of read exc_read[e]; off / uni_*: as in PackJob
hipError_t launch_gather_exc_text(const uint8_t *text, uint64_t bias, const uint64_t *off, uint64_t uni_base, uint32_t uni_len,
                                  const uint64_t *exc_read, const uint64_t *exc_off, uint64_t n_exc, uint8_t *exc_bytes, hipStream_t st);

// ---- the way back (pack.hip): records of the resident set as text ----
// Record k is the read idx[k] (LOCAL index) of R, reverse-complemented when rc && rc[k]; its text goes to
// out[out_off[k] .. out_off[k + 1]).  out_off is the exclusive prefix sum of the records' lengths (the caller computes it: it
// sizes the output from it), total = out_off[n].  out may have any alignment; no byte outside out[0 .. total) is written.
struct FetchJob {
    DevReads R;
    const uint64_t *idx;            // device, [n]
    const uint8_t *rc;              // device, [n], or nullptr: every record forward
    const uint64_t *out_off;        // device, [n + 1]
    uint64_t n, total;
    uint8_t *out;
};
hipError_t launch_fetch_text(const FetchJob &J, hipStream_t st);

} // namespace crass

// gunzip_launch.h — the device gunzip's job description and launch wrappers (gunzip.hip), for the engine.  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/crass_hip.h"
#include "gunzip_core.h"

namespace crass {

struct GzJob {
    const uint8_t *d;       // the deflate data (the file's bytes + G.d_off), device pointer, any alignment
    GzGeom G;
    // per chunk [G.nc]: find writes start (start[0] = 0 too), count the rest
    uint64_t *start; uint32_t *link; uint64_t *text_len, *end_bit; int32_t *reason;
    // per chain element, after the host's chain walk
    uint64_t n_chain;
    const uint32_t *chain;  // [n_chain] its chunk
    const uint64_t *off;    // [n_chain + 1] where its text starts
    uint16_t *sym;          // [off[n_chain]] the text as symbols
    uint8_t *win;           // [n_chain * 32768] the 32 KB in front of every element (element 0's is unused)
    uint8_t *out;           // the text, device pointer, any alignment
    uint32_t *crc_part;     // [n_chain] every element's own CRC-32
    unsigned long long *verdict;      // the first chain element that holds an unresolved marker, kBzNoOffence before the launch
    // members mode (NULL / 0 otherwise)
    uint32_t *n_ends; uint64_t *last_end;      // per chunk [G.nc], from count
    const uint64_t *slot;   // [n_chain + 1] where an element's GzEnd records start
    const uint64_t *m0;     // [n_chain] the text offset of the start of the member that holds the element's first byte
    GzEnd *ends;            // [slot[n_chain]]
    uint64_t n_pieces;
    const uint64_t *piece;  // [n_pieces + 1] the text cut at member boundaries and every kGzCrcPiece bytes inside a member
    uint32_t *crc_piece;    // [n_pieces]
};
// members: the kernels of members mode (k_gz_*_members)
hipError_t launch_gz_find(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_count(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_decode(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_windows(const GzJob &J, hipStream_t st);
hipError_t launch_gz_narrow(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_member_crc(const GzJob &J, hipStream_t st);
// gunzip.cpp: what the rule decided, for the caller
int gz_plan_fill(crass_gzip_plan *plan, uint64_t nc, const uint64_t *start, const uint32_t *link, const uint64_t *text_len, uint64_t n_chain);
int gz_members_fill(crass_gzip_members *m, uint64_t nm, const uint64_t *in_off, const uint64_t *text_off);

} // namespace crass

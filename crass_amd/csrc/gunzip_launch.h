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
    // what this job is of the file (gz_job_whole: all of it).  Only d[in_lo, in_hi) is staged: no kernel reads outside it (d itself
    // may lie in front of the allocation); find / count run over the chunks [k0, k1); the chain arrays below hold the elements
    // [e0, e0 + n_chain) of the file's chain, off[] their places in the FILE's text (sym and out are the places of text byte 0).
    // d, sym and out of such a job are BIASED pointers that may lie in front of their allocations: nothing is wrong as long as every
    // access stays inside [in_lo, in_hi) and [off[0], off[n_chain]) — at(), gz_survives, put() / get() and narrow's bounds see to that
    uint64_t in_lo, in_hi, k0, k1, e0;
    uint32_t in_tail;       // members mode: the 8 bytes behind the region, d[G.dn, G.dn + 8), are staged too (io.tail())
    // per chunk [G.nc]: find writes start (start[0] = 0 too), count the rest
    uint64_t *start; uint32_t *link; uint64_t *text_len, *end_bit; int32_t *reason;
    // per chain element, after the host's chain walk
    uint64_t n_chain;
    const uint32_t *chain;  // [n_chain] its chunk
    const uint64_t *off;    // [n_chain + 1] where its text starts
    uint16_t *sym;          // [off[n_chain]] the text as symbols
    uint8_t *win;           // [n_chain * 32768] the 32 KB in front of every element (the file's element 0 has none: its slot is unused)
    // a range of the chain whose entry window (in front of element e0) is not known yet: k_gz_windows_sym makes the symbolic
    // windows of its elements 1 .. n_win (n_win = n_chain where the next range starts behind this one's last element, else
    // n_chain - 1), k_gz_window_resolve makes win[1 .. n_win] from them once win[0] holds the entry window
    uint16_t *wsym;         // [(n_win + 1) * 32768] slot 0 is unused (the identity)
    uint64_t n_win;         // (0: a whole file, k_gz_windows makes win[1, n_chain)); win then has max(n_chain, n_win + 1) slots
    uint8_t *out;           // the text, device pointer, any alignment
    uint32_t *crc_part;     // [n_chain] every element's own CRC-32
    unsigned long long *verdict;      // the first chain element that holds an unresolved marker, kBzNoOffence before the launch
    // members mode (NULL / 0 otherwise)
    uint32_t *n_ends; uint64_t *last_end;      // per chunk [G.nc], from count
    const uint64_t *slot;   // [n_chain + 1] where an element's GzEnd records start (NULL: the decode keeps no records)
    const uint64_t *m0;     // [n_chain] the text offset of the start of the member that holds the element's first byte ([n_win + 1] where
                            // k_gz_windows_sym_members makes the window behind the last element)
    GzEnd *ends;            // [slot[n_chain] - slot[0]] the job's records, relative to its first element's slot
    uint64_t n_pieces;
    const uint64_t *piece;  // [n_pieces + 1] the text cut at member boundaries and every kGzCrcPiece bytes inside a member
    uint32_t *crc_piece;    // [n_pieces]
};
inline void gz_job_whole(GzJob &J) { J.in_lo = 0; J.in_hi = J.G.dn; J.k0 = 0; J.k1 = J.G.nc; J.e0 = 0; J.in_tail = 1; }      // (behind J.G)
// members: the kernels of members mode (k_gz_*_members)
hipError_t launch_gz_find(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_count(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_decode(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_windows(const GzJob &J, hipStream_t st);
hipError_t launch_gz_windows_sym(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_window_resolve(const GzJob &J, hipStream_t st);
hipError_t launch_gz_narrow(const GzJob &J, hipStream_t st, bool members = false);
hipError_t launch_gz_member_crc(const GzJob &J, hipStream_t st);
// gunzip.cpp: what the rule decided, for the caller
int gz_plan_fill(crass_gzip_plan *plan, uint64_t nc, const uint64_t *start, const uint32_t *link, const uint64_t *text_len, uint64_t n_chain);
int gz_members_fill(crass_gzip_members *m, uint64_t nm, const uint64_t *in_off, const uint64_t *text_off);

} // namespace crass

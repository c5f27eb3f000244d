// inflate_launch.h — the device inflate's job description and launch wrapper (inflate.hip), for the engine.  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "inflate_core.h"

namespace crass {

struct BzJob {
    const uint8_t *in;      // the file's bytes, device pointer, any alignment
    uint8_t *out;           // the text, device pointer, any alignment
    const uint64_t *in_off, *out_off, *data_off;      // device copies of the index: [n + 1], [n + 1], [n]
    uint64_t n_members;
    uint32_t *reason;       // [n] every member's BzReason
    unsigned long long *verdict;      // the smallest bz_offence, kBzNoOffence before the launch
    int hbm_window;         // 0: the text is decoded in the wave's LDS window; 1: in the member's range of out (inflate.hip)
};
// what both inflate calls check on the host before a byte is touched (bgzf.cpp): CRASS_OK or CRASS_ERR_INVALID_ARG
int bgzf_index_check(const crass_bgzf_index *ix, uint64_t n_bytes, uint64_t out_cap);
hipError_t launch_bgzf_inflate(const BzJob &J, hipStream_t st);

} // namespace crass

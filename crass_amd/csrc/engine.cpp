// engine.cpp — the context behind include/crass_hip.h: its creation and destruction, what every call that makes a read set
// resident ends with (scratch, position hints, first-call bounds), the install of a pattern set, Levenshtein, counters.
// The stages are files of their own: engine_pass1.cpp (seed scan), engine_merge.cpp (merge, exchange), engine_pass2.cpp (recruit),
// engine_ingest.cpp, engine_fastx.cpp, engine_inflate.cpp, engine_names.cpp, engine_shards.cpp (device ingest).  The context itself
// is engine_ctx.h, which also declares what crosses these files.
//
// There is no CPU fallback anywhere in these files: every search decision is made by the HIP kernels in kernels.hip, survivors.hip (survivor_wave.hip,
// long_light.hip, survivor_lanes.hip), pass2.hip and sinks.hip; the host only orders, tokenises and clusters their output ("stays on host").
#include "engine_ctx.h"

#include <cstdio>
#include <new>
#include <string>

// crass_candidates' arrays from the compact hand-off blob (and the distinct-string list for the DR strings)
void crass_hip_ctx::widen_p1() const
{
    P1Dense &D = dense;
    if (D.wide_ready) return;
    (void)wait_bulk();                  // (callers have checked its status)
    const uint64_t n = D.n;
    const uint32_t ss_cap = D.pack_ss_cap, stride = dr_stride;
    const uint8_t *hb = D.h_blob.p;
    const uint16_t *b_replen = (const uint16_t *)(hb + D.lay.replen), *b_ss = (const uint16_t *)(hb + D.lay.ss);
    const uint8_t *b_nss = hb + D.lay.nss, *b_ss8 = hb + D.lay.ss;
    D.w_replen.resize(n); D.w_nss.resize(n); D.w_ss_off.resize(n); D.w_ss.resize(n * (size_t)ss_cap);
    D.w_dr_len.resize(n); D.w_dr.resize(n * (size_t)stride);
    if (D.dr_fallback) (void)hipStreamSynchronize(copy_stream);
    else (void)wait_dx();               // (the distinct list the candidates' strings are read from)
    // ~150 bytes per candidate (564 k candidates at 100 M reads: 85 MB, 4.5 ms on one thread): ranges of candidates on the host pool
    const size_t per_task = 16384;
    host_parallel_for((size_t)((n + per_task - 1) / per_task), 16, [&](size_t t) {
        const uint64_t k0 = t * per_task, k1 = std::min<uint64_t>(n, k0 + per_task);
        for (uint64_t k = k0; k < k1; k++) { D.w_replen[k] = b_replen[k]; D.w_nss[k] = b_nss[k]; D.w_ss_off[k] = k * (uint64_t)ss_cap; }
        if (D.lay.ss_elem == 1) for (uint64_t i = k0 * ss_cap; i < k1 * (uint64_t)ss_cap; i++) D.w_ss[i] = b_ss8[i];
        else for (uint64_t i = k0 * ss_cap; i < k1 * (uint64_t)ss_cap; i++) D.w_ss[i] = b_ss[i];
        if (D.dr_fallback) {
            memcpy(D.w_dr.data() + k0 * (size_t)stride, D.h_dr_fb.p + k0 * (size_t)stride, (size_t)(k1 - k0) * stride);
            memcpy(D.w_dr_len.data() + k0, D.h_dr_len_fb.p + k0, (size_t)(k1 - k0) * 2);
        } else {
            for (uint64_t k = k0; k < k1; k++) {
                const uint32_t j = h_dmap.p[k];
                memcpy(D.w_dr.data() + k * (size_t)stride, h_dx_chars.p + j * (size_t)stride, stride);
                D.w_dr_len[k] = h_dx_len.p[j];
            }
        }
    });
    D.wide_ready = true;
}

// the helper thread owns c->merge while a host-view build is in flight: wait for it before touching that state
void quiesce_worker(crass_hip_ctx *c)
{
    if (c->dm.build_pending) {
        if (!c->worker.run_here_if_not_started()) c->worker.wait();
        c->dm.build_pending = false;
        (void)c->worker.take_failed();
        c->dm.br.valid = false;                         // (results of a build nobody asked for any more)
        if (c->dm.br.hip) { c->last_hip = c->dm.br.hip; c->dm.br.hip = 0; }
    }
}

extern "C" {

int crass_hip_abi_version(void) { return CRASS_HIP_ABI_VERSION; }

// Test seam, not part of include/crass_hip.h: the anchor keys' shape the device path selects for a lowDRsize (dm_anchor_shape,
// engine_internal.h) — bases per key and the windows' alignment in bases; 0 when the device path does not take that lowDRsize.
int crassi_anchor_shape(uint32_t low_dr, uint32_t *key_bases, uint32_t *align_bases)
{
    uint32_t kb = 0, ash = 0;
    const bool ok = dm_anchor_shape(low_dr, kb, ash);
    if (key_bases) *key_bases = ok ? kb : 0u;
    if (align_bases) *align_bases = ok ? 1u << ash : 0u;
    return ok ? 1 : 0;
}

// Test seam, not part of include/crass_hip.h: the device bytes this library holds right now, over every context of the
// process (DevBuf's counter) — what tests/test_gpu_ingest_scratch.py compares before and after a call.
uint64_t crassi_dev_bytes_live(void) { return g_dev_bytes.load(std::memory_order_relaxed); }

void crass_default_params(crass_params *p)
{
    p->lowDRsize = 23; p->highDRsize = 47; p->lowSpacerSize = 26; p->highSpacerSize = 50;
    p->searchWindowLength = 8; p->minNumRepeats = 2; p->kmer_clust_size = 6;
}

const char *crass_hip_strerror(int s)
{
    switch (s) {
        case CRASS_OK: return "ok";
        case CRASS_ERR_INVALID_ARG: return "invalid argument";
        case CRASS_ERR_UNSUPPORTED: return "parameter outside the device path's implementation limits";
        case CRASS_ERR_NO_DEVICE: return "no usable HIP device";
        case CRASS_ERR_HIP: return "HIP runtime call failed";
        case CRASS_ERR_OOM: return "out of memory";
        case CRASS_ERR_STATE: return "call order violated";
        case CRASS_ERR_SEARCH_FATAL: return "Fatal error in search algorithm!";
        case CRASS_ERR_OVERFLOW: return "device pool overflow";
        case CRASS_ERR_IO: return "I/O error";
        case CRASS_ERR_RCCL: return "RCCL call failed (crass_hip_group_last_error())";
        default: return "unknown status";
    }
}

int crass_hip_last_hip_error(const crass_hip_ctx *ctx) { return ctx ? ctx->last_hip : 0; }
void *crass_hip_stream(const crass_hip_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int crass_hip_create(const crass_params *p, int device, crass_hip_ctx **out)
{
    if (!p || !out) return CRASS_ERR_INVALID_ARG;
    *out = nullptr;
    // option validation as crass.cpp:264-271,316-324,351-358,366-374,388-400
    if (p->searchWindowLength < CRASS_HIP_MIN_WINDOW || p->searchWindowLength > CRASS_HIP_MAX_WINDOW) return CRASS_ERR_INVALID_ARG;
    if (p->lowDRsize < 8 || p->lowSpacerSize < 8) return CRASS_ERR_INVALID_ARG;
    if (p->lowDRsize >= p->highDRsize || p->lowSpacerSize >= p->highSpacerSize) return CRASS_ERR_INVALID_ARG;
    if (p->minNumRepeats < 2) return CRASS_ERR_INVALID_ARG;
    if (p->highDRsize > CRASS_HIP_MAX_DR) return CRASS_ERR_UNSUPPORTED;
    // lowDR < 2w-1 makes the reference's `unsigned skips = lowDR - (2w-1)` wrap to ~4e9
    // (libcrispr.cpp:281); its `j = j + skips` then walks BACKWARDS after a failed candidate and
    // need not terminate.  Ill-defined in the reference, refused here.
    if (p->lowDRsize < 2 * p->searchWindowLength - 1) return CRASS_ERR_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CRASS_ERR_NO_DEVICE;
    crass_hip_ctx *c = new (std::nothrow) crass_hip_ctx();
    if (!c) return CRASS_ERR_OOM;
    c->prm = *p;
    c->device = device;
    c->dp.lowDR = p->lowDRsize; c->dp.highDR = p->highDRsize; c->dp.lowSp = p->lowSpacerSize; c->dp.highSp = p->highSpacerSize;
    c->dp.window = p->searchWindowLength; c->dp.minRepeats = p->minNumRepeats;
    uint32_t skips = p->lowDRsize - (2 * p->searchWindowLength - 1);     // unsigned, libcrispr.cpp:281
    if (skips < 1) skips = 1;
    c->dp.skips = skips;
    c->env.read();
    g_dev_cap.store(c->env.pool_cap_bytes, std::memory_order_relaxed);
    c->dp.debug_stop = c->env.surv_debug;
    c->dp.find_serial = c->env.lane_find_serial ? 1u : 0u;
    if (c->env.stage_timing >= 0) c->timing_level = c->env.stage_timing;
    if (c->env.no_lookback) c->lb_on = false;                    // A/B switch: three-kernel compaction
    c->dr_stride = (p->highDRsize + 15u) & ~15u;
    { const hipError_t he = hipSetDevice(device);
      if (he != hipSuccess) { fprintf(stderr, "[crass_hip] hipSetDevice(%d): %s\n", device, hipGetErrorString(he)); delete c; return CRASS_ERR_NO_DEVICE; } }
    if (const char *e = getenv("CRASS_WAIT")) {           // A/B: how a host thread waits for the device (spin | yield | block)
        const unsigned f = !strcmp(e, "spin") ? hipDeviceScheduleSpin : !strcmp(e, "yield") ? hipDeviceScheduleYield : !strcmp(e, "block") ? hipDeviceScheduleBlockingSync : hipDeviceScheduleAuto;
        const hipError_t fe = hipSetDeviceFlags(f);
        if (fe != hipSuccess) fprintf(stderr, "[crass_hip] hipSetDeviceFlags(%s): %s\n", e, hipGetErrorString(fe));
    }
    if (getenv("CRASS_SURV_PROF")) {                    // diagnostics: phase cycles of the wave-per-read kernel (tools/longread_phases.py)
        void *pp = nullptr;
        if (hipMalloc(&pp, (192 + 2 * 16384) * 8) == hipSuccess && hipMemset(pp, 0, (192 + 2 * 16384) * 8) == hipSuccess) {
            c->dp.prof = (unsigned long long *)pp;
            const unsigned long long big = ~0ull;
            (void)hipMemcpy(c->dp.prof + 188, &big, 8, hipMemcpyHostToDevice);
        }
    }
    for (hipStream_t *sp : {&c->stream, &c->copy_stream}) {
        const hipError_t he = hipStreamCreateWithFlags(sp, hipStreamNonBlocking);
        if (he != hipSuccess) { fprintf(stderr, "[crass_hip] hipStreamCreateWithFlags on device %d: %s\n", device, hipGetErrorString(he)); delete c; return CRASS_ERR_NO_DEVICE; }
    }
    // (hint_stream and its events: created with the first long-read set, setup_pos_hints)
    for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) { delete c; return CRASS_ERR_HIP; }
    if (c->h_flags.ensure(8) != hipSuccess) { delete c; return CRASS_ERR_OOM; }
    memset(c->h_flags.p, 0, 32);
    c->poll_on = getenv("CRASS_NO_POLL") == nullptr;
    if (hipEventCreateWithFlags(&c->ev_gathered, hipEventDisableTiming) != hipSuccess) { delete c; return CRASS_ERR_HIP; }
    if (hipEventCreateWithFlags(&c->ev_premerge, hipEventDisableTiming) != hipSuccess) { delete c; return CRASS_ERR_HIP; }
    c->dma = sdma_create();                             // (nullptr: the copy kernel is used)
    if (c->dma && !getenv("CRASS_DX_PINNED")) {         // (A/B switch: the de-duplication kernel writes the distinct list to pinned memory itself)
        for (auto &d : c->dma_dx) d = sdma_create();
        c->dx_via_dma = c->dma_dx[0] && c->dma_dx[1] && c->dma_dx[2];
    }
    (void)warm_dmerge_module();                         // (code-object load: here, not inside the first merge)
    *out = c;
    return CRASS_OK;
}

int crass_hip_stream_wait_event(crass_hip_ctx *c, void *event)
{
    if (!c || !event) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamWaitEvent(c->stream, (hipEvent_t)event, 0));
    return CRASS_OK;
}

int crass_hip_reload_env(crass_hip_ctx *c)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    c->env.read();
    g_dev_cap.store(c->env.pool_cap_bytes, std::memory_order_relaxed);
    c->dp.debug_stop = c->env.surv_debug;
    c->dp.find_serial = c->env.lane_find_serial ? 1u : 0u;
    if (c->env.stage_timing >= 0) c->timing_level = c->env.stage_timing;
    c->lb_on = !c->env.no_lookback;
    return CRASS_OK;
}

int crass_hip_set_stage_timing(crass_hip_ctx *c, int level)
{
    if (!c || level < 0 || level > 2) return CRASS_ERR_INVALID_ARG;
    c->timing_level = level;
    return CRASS_OK;
}

int crass_hip_set_host_view(crass_hip_ctx *c, int light)
{
    if (!c || light < 0 || light > 1) return CRASS_ERR_INVALID_ARG;
    quiesce_worker(c);
    c->host_view_light = light != 0;
    // a merge prepared before this call (crass_hip_exchange_setup sizes one at load) would still export the view nobody reads:
    // a light context's merges skip the k_dmx_* kernels (the next prepare decides again)
    if (c->host_view_light) c->dm.M.x_on = 0;
    return CRASS_OK;
}

int crass_hip_set_timing_focus(crass_hip_ctx *c, unsigned kernels)
{
    if (!c || kernels > 7u) return CRASS_ERR_INVALID_ARG;
    c->timing_focus = kernels;
    return CRASS_OK;
}

void crass_hip_destroy(crass_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    quiesce_worker(c);
    c->worker.stop();
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->hint_stream) (void)hipStreamSynchronize(c->hint_stream);
    (void)sdma_wait(c->dma);                            // (before any buffer goes)
    (void)c->wait_dx();
    ingest_free_all(c);                                 // (while the streams its release functions wait for are alive)
    if (getenv("CRASS_POLL_REPORT")) fprintf(stderr, "[crass_hip] stage-flag polls that ran out of their budget: %u (of %u flags)\n", c->n_poll_timeouts.load(), c->flag_seq);
    c->lb_status.release(); c->lb_ticket.release(); c->h_lb_fail.release(); c->h_flags.release();
    if (c->xchg.ev_counts) (void)hipEventDestroy(c->xchg.ev_counts);
    c->dm.release(); c->h_qblob.release(); c->xchg.send.release(); c->xchg.xinfo.release(); c->xchg.h_xinfo.release();
    c->dd_map.release(); c->dd_dx_chars.release(); c->dd_dx_len.release(); c->dd_dx_hash.release();
    c->h_dmap.release(); c->h_dx_chars.release(); c->h_dx_len.release(); c->h_dx_hash.release();
    if (c->ev_gathered) (void)hipEventDestroy(c->ev_gathered);
    if (c->ev_sink_copies) (void)hipEventDestroy(c->ev_sink_copies);
    for (int q = 0; q < crass_hip_ctx::kHintParts; q++) if (c->ev_hint[q]) (void)hipEventDestroy(c->ev_hint[q]);
    if (c->ev_hint_go) (void)hipEventDestroy(c->ev_hint_go);
    if (c->hint_stream) (void)hipStreamDestroy(c->hint_stream);
    sdma_destroy(c->dma); c->dma = nullptr;
    for (auto &d : c->dma_sink) { sdma_destroy(d); d = nullptr; }
    for (auto &d : c->dma_dx) { sdma_destroy(d); d = nullptr; }
    if (c->ev_premerge) (void)hipEventDestroy(c->ev_premerge);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    c->r_packed.release(); c->r_word_off.release(); c->r_lengths.release(); c->r_header_id.release();
    c->r_exc_mask.release(); c->r_exc_read.release(); c->r_exc_off.release(); c->r_exc_bytes.release();
    c->d_mask.release(); c->d_word_prefix.release(); c->d_block_sums.release(); c->d_idx.release(); c->d_count.release();
    c->d_found.release(); c->d_hit_info.release(); c->d_surv.release(); c->d_dr.release(); c->d_ss_pool.release();
    c->d_ss_used.release(); c->d_rec.release(); c->d_exc_hit.release(); c->d_extra.release(); c->d_extra_bad.release(); c->h_extra_bad.release();
    c->g_surv.release(); c->g_dr.release(); c->g_ss.release(); c->g_fidx.release(); c->h_count.release(); c->h_surv.release(); c->h_dr.release(); c->h_ss.release(); c->h_idx.release(); c->h_rec.release();
    c->a_go4w.release(); c->a_go16.release(); c->a_go32.release(); c->a_out.release(); c->a_go4.release(); c->dense.release(); c->d_fidx.release(); c->d_pos_hint.release(); c->d_pos_hint_off.release(); c->d_pos_hint_blk.release(); c->d_punt.release(); c->d_redo.release(); c->dd_keys.release(); c->dd_first.release(); c->dd_slot.release(); c->dd_rep.release(); c->dd_hash.release(); c->h_rep.release(); c->h_hash.release(); c->a_anchor.release(); c->d_slot_info.release(); c->d_slot_pid.release(); c->a_out_pid.release(); c->a_pat_token.release();
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int validate_reads(const crass_reads *r)
{
    if (!r) return CRASS_ERR_INVALID_ARG;
    if (r->n_reads && !r->packed) return CRASS_ERR_INVALID_ARG;
    if (!r->stride_words && r->n_reads && !r->word_off) return CRASS_ERR_INVALID_ARG;
    if (!r->uniform_len && r->n_reads && !r->lengths) return CRASS_ERR_INVALID_ARG;
    if (r->n_exceptions && (!r->exc_read || !r->exc_off || !r->exc_bytes)) return CRASS_ERR_INVALID_ARG;
    if (r->uniform_len > CRASS_HIP_MAX_READ_LEN) return CRASS_ERR_UNSUPPORTED;
    return CRASS_OK;
}

int alloc_scratch(crass_hip_ctx *c)
{
    const uint64_t n = c->R.n_reads;
    // (the mask / prefix scratch also serves compactions over survivor and hit SLOTS, whose launches are sized by bounds of
    // at least 65 536 / 4 096 slots whatever the read count: never smaller than that many bits)
    const uint64_t n_words = std::max<uint64_t>((n + 63) / 64, 1024);
    HIPCHK(c, c->d_mask.ensure(n_words + 1));
    HIPCHK(c, c->d_word_prefix.ensure(n_words + 1));
    HIPCHK(c, c->d_block_sums.ensure((n_words + 255) / 256 + 2));
    HIPCHK(c, c->d_idx.ensure(n + 1));
    HIPCHK(c, c->d_count.ensure(8));
    HIPCHK(c, c->d_found.ensure(n + 1));
    HIPCHK(c, c->d_hit_info.ensure(n + 1));
    HIPCHK(c, c->d_ss_used.ensure(4));
    HIPCHK(c, c->h_count.ensure(32));      // [0..8) the stage counters, [16..24) those of a deferred pass 1 (p1d)
    HIPCHK(c, hipMemsetAsync(c->d_found.p, 0, n + 1, c->stream));
    return CRASS_OK;
}

// long reads skip the per-read filter; with the default window and DR/spacer bounds they get one seed-hint bit
// per base position instead (k_hint_positions).  lengths == nullptr: uniform length.
static int setup_pos_hints(crass_hip_ctx *c, const uint32_t *lengths, uint32_t uniform_len, uint64_t n)
{
    c->n_pos_hint_words = 0;
    c->R.pos_hint = nullptr; c->R.pos_hint_off = nullptr; c->R.wave_walk = 0; c->R.hint_all = 0;
    const DevParams &P = c->dp;
    // (skips == 8: the hints are kept per residue class mod 8 — k_hint_positions fills the lattice class, the walking wave the others)
    // (... and any shift range the hint tile's halo covers: -s / -S / -D keep the hints, launch_hint_positions)
    // (... and sets that stay on the filtered path but have no lane-per-read filter — reads of 257 .. 2 048 bases, strides that differ:
    // the hint bits are their filter, crass_hip_seed_scan; CRASS_NO_HINT_FILTER: the A/B switch, back to k_filter_general)
    const bool lane_filter = c->R.stride_words >= 4 && c->R.stride_words <= 16;
    c->hint_filter = c->max_len <= c->env.long_min && !lane_filter && !c->env.no_hint_filter;
    c->hint_filter_any = false;
    const bool shifts_ok = P.lowDR + P.lowSp >= 17 && P.highDR + P.highSp <= 127 && P.highDR + P.highSp >= P.lowDR + P.lowSp;
    const bool lattice_hints = P.window == 8 && P.skips == 8 && shifts_ok;
    // (... under another window or seed lattice those sets get the every-position form of the bits as their filter, nothing kept:
    // launch_hint_filter_any; the tiles' read index is all that is set up for it)
    const bool any_filter = c->hint_filter && !lattice_hints && shifts_ok && P.window >= 6 && P.window <= 9 && P.skips >= 1;
    if ((c->max_len <= c->env.long_min && !c->hint_filter) || n == 0 || !(lattice_hints || any_filter)) return CRASS_OK;
    if (c->env.no_pos_hints) return CRASS_OK;             // A/B switch
    std::vector<uint64_t> off(n + 1);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; i++) { off[i] = at; at += ((uint64_t)(lengths ? lengths[i] : uniform_len) + 63) / 64; }
    off[n] = at;
    HIPCHK(c, c->d_pos_hint_off.ensure(n + 1)); HIPCHK(c, c->d_pos_hint.ensure(at + 1));
    HIPCHK(c, hipMemcpy(c->d_pos_hint_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    c->n_pos_hint_words = at;
    c->hint_filter_any = any_filter;
    c->R.pos_hint = c->d_pos_hint.p; c->R.pos_hint_off = c->d_pos_hint_off.p;
    c->R.hint_all = any_filter ? 1u : 0u;               // (every position's bit, written by the filter launch itself)
    c->R.wave_walk = c->max_len > std::min<uint32_t>(c->env.long_min, c->env.wave_walk_min) ? 1u : 0u;
    c->pos_hint_blk = false;
    // slices: read boundaries n i / K; slice i covers the hint words [roundup256(off[r_i]), roundup256(off[r_i+1])), so every word
    // of a read below r_i+1 belongs to a slice <= i (CRASS_HINT_PARTS=1: the A/B switch)
    { const char *hp = getenv("CRASS_HINT_PARTS");       // (A/B: 1 = one launch on the main stream)
      const int want = hp ? atoi(hp) : 2;
      // (two: each slice's walk is its own launch with its own ramp and tail — four slices were slower than none, 15.5 vs 14.3 ms
      // per step on configs[3], two are 14.0; an explicit CRASS_HINT_PARTS also slices small sets: the tests)
      const bool big = hp ? (n >= 64 && at >= 2048) : (n >= 4096 && at >= (1u << 20));
      c->hint_parts = (big && !c->hint_filter) ? std::min(std::max(want, 1), (int)crass_hip_ctx::kHintParts) : 1; }
    if (c->hint_parts > 1 && !c->hint_stream) {
        // lowest priority: its blocks fill what the walking kernel (two waves per SIMD: its LDS) leaves free, not the other way
        // round.  Created with the first long-read set only: a second low-priority stream in every context changed how the
        // runtime spreads streams over its hardware queues, and the merge's view export (its own low-priority stream) then
        // cost a short-read step 0.5 ms instead of 0.1
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        HIPCHK(c, hipStreamCreateWithPriority(&c->hint_stream, hipStreamNonBlocking, getenv("CRASS_HINT_SAME_PRIORITY") ? 0 : prio_lo));
        for (int q = 0; q < crass_hip_ctx::kHintParts; q++) HIPCHK(c, hipEventCreateWithFlags(&c->ev_hint[q], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_hint_go, hipEventDisableTiming));
    }
    for (int q = 0; q <= c->hint_parts; q++) {
        const uint64_t r = q == c->hint_parts ? n : n * (uint64_t)q / (uint64_t)c->hint_parts;
        c->hint_read_split[q] = r;
        c->hint_word_split[q] = q == c->hint_parts ? at : ((off[r] + 255) & ~255ull);
    }
    if (lengths && n <= 0xFFFFFFFFull) {                // ragged: the read of every block's first hint word (k_hint_positions)
        std::vector<uint32_t> blk((at + 255) / 256 + 1, 0);
        uint64_t r = 0;
        for (uint64_t b = 0; b * 256 < at; b++) {
            while (r + 1 < n && off[r + 1] <= b * 256) r++;
            blk[b] = (uint32_t)r;
        }
        blk.back() = (uint32_t)(n - 1);                  // (the bisection's upper end for the last block)
        HIPCHK(c, c->d_pos_hint_blk.ensure(blk.size()));
        HIPCHK(c, hipMemcpy(c->d_pos_hint_blk.p, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
        c->pos_hint_blk = true;
    }
    return CRASS_OK;
}

void reset_results(crass_hip_ctx *c)
{
    quiesce_worker(c);
    if (c->p1d.active) { (void)hipStreamSynchronize(c->stream); c->p1d.active = false; }      // (a deferred pass 1 nobody finished)
    (void)c->wait_bulk();               // (a hand-off copy still on its DMA engine: the buffers may be re-sized next, and a
                                        // free only waits for the device's queues)
    c->have_pass1 = c->have_merge = c->have_pass2 = c->have_patterns = false;
    c->dm.active = false;
    memset(&c->cnt, 0, sizeof(c->cnt));
}

// what every call that makes a read set resident ends with, once the set's arrays are on their way to the device: the
// scratch sized by the read count, the long reads' position hints, the first call's speculation bounds and pools, counters.
// lengths: host array, nullptr for a uniform length.
int finish_load(crass_hip_ctx *c, const DevReads &R, uint64_t read_index_base, uint32_t max_len, const uint32_t *lengths, uint64_t total_words)
{
    c->R = R;
    c->read_base = read_index_base;
    c->max_len = max_len;
    c->uniform = R.uniform_len != 0;
    c->have_reads = true;
    int s = alloc_scratch(c);
    if (s) return s;
    s = setup_pos_hints(c, R.uniform_len ? nullptr : lengths, R.uniform_len, R.n_reads);
    if (s) return s;
    s = first_call_bounds(c);
    if (s) return s;
    presize_hostloop(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cnt.n_reads = R.n_reads; c->cnt.n_exceptions = R.n_exc; c->cnt.bytes_reads_device = total_words * 4;
    return CRASS_OK;
}

int crass_hip_get_candidates(const crass_hip_ctx *c, crass_candidates *o)
{
    if (!c || !o) return CRASS_ERR_INVALID_ARG;
    if (c->p1d.active) { const int ds = settle_p1(const_cast<crass_hip_ctx *>(c)); if (ds) return ds; }
    if (!c->have_pass1) return CRASS_ERR_STATE;
    if (const int bs = c->wait_bulk()) return bs;
    if (c->dense.active) {
        const crass_hip_ctx::P1Dense &D = c->dense;
        c->widen_p1();
        const uint8_t *hb = D.h_blob.p;
        o->n = D.n; o->read_idx = (const uint64_t *)(hb + D.lay.read); o->low_lexi = hb + D.lay.low; o->repeat_len = D.w_replen.data();
        o->n_ss = D.w_nss.data(); o->ss_off = D.w_ss_off.data(); o->ss_pool = D.w_ss.data();
        o->dr_stride = c->dr_stride; o->dr_len = D.w_dr_len.data(); o->dr_chars = D.w_dr.data();
    } else {
        c->materialize_cand();
        o->n = c->cand.size();
        o->read_idx = c->cand.read.data(); o->low_lexi = c->cand.low.data(); o->repeat_len = c->cand.replen.data();
        o->n_ss = c->cand.nss.data(); o->ss_off = c->cand.ss_off.data(); o->ss_pool = c->cand.ss.data();
        o->dr_stride = c->dr_stride; o->dr_len = c->cand.dr_len.data(); o->dr_chars = c->cand.dr.data();
    }
    o->max_read_len = c->max_len;
    return CRASS_OK;
}

// the pattern set pass 2 searches for: the merge's (engine_merge.cpp) or a caller's (crass_hip_set_patterns)
int install_patterns(crass_hip_ctx *c, const StringArena &pats)
{
    c->n_installed_patterns = (uint32_t)pats.size();
    c->have_patterns = false;
    quiesce_worker(c);
    c->dm.active = false;                               // the installed set is the host-built one from here on
    c->cnt.n_patterns = (uint32_t)pats.size();
    if (pats.empty()) { c->cnt.ac_states = 0; return CRASS_OK; }
    // a recruit's DR string lives in a slot of dr_stride bytes (d_dr, h_dr, q_dr: ensure_recruit_buffers, k_recruit_finish, the
    // host sink), so a longer pattern is declined here, before anything is uploaded; have_patterns stays false and a recruit
    // that follows returns CRASS_ERR_STATE
    for (size_t i = 0; i < pats.size(); i++)
        if (pats.len(i) == 0 || pats.len(i) > 255 || pats.len(i) > c->dr_stride) return CRASS_ERR_UNSUPPORTED;
    HostAutomaton &H = c->H;
    HostAnchors HK;
    const bool prof = c->env.merge_profile;
    const double tb0 = now_ms();
    build_automaton_and_anchors(H, HK, pats);
    const double tb2 = now_ms();
    DevAutomaton A{};
    A.n_states = H.n_states; A.n_sym1 = H.n_sym1;
    A.max_pat_len = 0;
    for (size_t i = 0; i < pats.size(); i++) A.max_pat_len = std::max<uint32_t>(A.max_pat_len, (uint32_t)pats.len(i));
    memcpy(A.sym, H.sym, 256);
    (void)hipSetDevice(c->device);
    // the packed-read scans need the 4-column table only; the full byte-symbol table goes up on demand
    // (ensure_full_automaton: full scans without anchors, exception reads)
    c->full_automaton_uploaded = false;
    if (H.n_states <= 65535) {
        HIPCHK(c, c->a_go4.ensure(H.go4.size()));
        HIPCHK(c, hipMemcpyAsync(c->a_go4.p, H.go4.data(), H.go4.size() * 2, hipMemcpyHostToDevice, c->stream));
        A.go4 = c->a_go4.p; A.acgt_ok = 1;
    } else {
        HIPCHK(c, c->a_go4w.ensure(H.go4w.size()));
        HIPCHK(c, hipMemcpyAsync(c->a_go4w.p, H.go4w.data(), H.go4w.size() * 4, hipMemcpyHostToDevice, c->stream));
        A.go4w = c->a_go4w.p; A.acgt_ok = 0;
    }
    HIPCHK(c, c->a_out.ensure(H.out_len.size()));
    HIPCHK(c, hipMemcpyAsync(c->a_out.p, H.out_len.data(), H.out_len.size() * 2, hipMemcpyHostToDevice, c->stream));
    A.out_len = c->a_out.p;
    HIPCHK(c, c->a_out_pid.ensure(H.out_pid.size()));
    HIPCHK(c, hipMemcpyAsync(c->a_out_pid.p, H.out_pid.data(), H.out_pid.size() * 4, hipMemcpyHostToDevice, c->stream));
    A.out_pid = c->a_out_pid.p;
    c->have_pat_token = false;
    c->A = A;
    // anchor keys for the pass-2 fast path
    c->have_anchors = false;
    if (HK.ok) {
        HIPCHK(c, c->a_anchor.ensure(HK.table.size()));
        HIPCHK(c, hipMemcpyAsync(c->a_anchor.p, HK.table.data(), HK.table.size() * 4, hipMemcpyHostToDevice, c->stream));
        c->K.table = c->a_anchor.p; c->K.log_size = HK.log_size; c->K.mode = HK.mode; c->K.m1 = HK.m1;
        c->K.m2 = HK.m2; c->K.n_keys = HK.n_keys;
        c->have_anchors = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));        // HK's table is a local
    c->have_patterns = true;
    c->cnt.ac_states = H.n_states;
    if (prof) fprintf(stderr, "[crass_merge] automaton + anchors %.3f ms, uploads %.3f ms\n", tb2 - tb0, now_ms() - tb2);
    return CRASS_OK;
}

// full byte-symbol transition table: only the scans that cannot use the 4-column table need it
int ensure_full_automaton(crass_hip_ctx *c)
{
    if (c->full_automaton_uploaded) return CRASS_OK;
    const HostAutomaton &H = c->H;
    if (H.n_states <= 65535) {
        std::vector<uint16_t> g16(H.go.size());
        for (size_t i = 0; i < H.go.size(); i++) g16[i] = (uint16_t)H.go[i];
        HIPCHK(c, c->a_go16.ensure(g16.size()));
        HIPCHK(c, hipMemcpyAsync(c->a_go16.p, g16.data(), g16.size() * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));     // g16 is a local
        c->A.go16 = c->a_go16.p;
    } else {
        HIPCHK(c, c->a_go32.ensure(H.go.size()));
        HIPCHK(c, hipMemcpyAsync(c->a_go32.p, H.go.data(), H.go.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->A.go32 = c->a_go32.p;
    }
    c->full_automaton_uploaded = true;
    return CRASS_OK;
}

int crass_hip_levenshtein_batch(crass_hip_ctx *c, const char *chars, uint64_t n_chars, const uint64_t *a_off,
                                const uint32_t *a_len, const uint64_t *b_off, const uint32_t *b_len, uint64_t n_pairs,
                                int32_t *dist_out, float *sim_out)
{
    if (!c || (n_pairs && (!chars || !a_off || !a_len || !b_off || !b_len))) return CRASS_ERR_INVALID_ARG;
    if (n_pairs == 0) return CRASS_OK;
    (void)hipSetDevice(c->device);
    uint32_t max_len = 1;
    for (uint64_t k = 0; k < n_pairs; k++) {
        if (a_off[k] + a_len[k] > n_chars || b_off[k] + b_len[k] > n_chars) return CRASS_ERR_INVALID_ARG;
        max_len = std::max(max_len, std::max(a_len[k], b_len[k]));
    }
    if (max_len > 30000) return CRASS_ERR_UNSUPPORTED;
    DevBuf<uint8_t> d_chars; DevBuf<uint64_t> d_ao, d_bo; DevBuf<uint32_t> d_al, d_bl; DevBuf<int32_t> d_dist; DevBuf<float> d_sim;
    int rc = CRASS_OK;
    auto body = [&]() -> int {
        HIPCHK(c, d_chars.ensure(n_chars + 1)); HIPCHK(c, d_ao.ensure(n_pairs)); HIPCHK(c, d_bo.ensure(n_pairs));
        HIPCHK(c, d_al.ensure(n_pairs)); HIPCHK(c, d_bl.ensure(n_pairs)); HIPCHK(c, d_dist.ensure(n_pairs)); HIPCHK(c, d_sim.ensure(n_pairs));
        HIPCHK(c, hipMemcpyAsync(d_chars.p, chars, n_chars, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_ao.p, a_off, n_pairs * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_bo.p, b_off, n_pairs * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_al.p, a_len, n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_bl.p, b_len, n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_levenshtein_batch(d_chars.p, d_ao.p, d_al.p, d_bo.p, d_bl.p, n_pairs, d_dist.p, sim_out ? d_sim.p : nullptr, max_len, c->stream));
        if (dist_out) HIPCHK(c, hipMemcpyAsync(dist_out, d_dist.p, n_pairs * 4, hipMemcpyDeviceToHost, c->stream));
        if (sim_out) HIPCHK(c, hipMemcpyAsync(sim_out, d_sim.p, n_pairs * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CRASS_OK;
    };
    rc = body();
    d_chars.release(); d_ao.release(); d_bo.release(); d_al.release(); d_bl.release(); d_dist.release(); d_sim.release();
    return rc;
}

int crass_hip_get_counters(const crass_hip_ctx *c, crass_counters *o)
{
    if (!c || !o) return CRASS_ERR_INVALID_ARG;
    crass_hip_ctx *m = const_cast<crass_hip_ctx *>(c);
    if (m->p1d.active) { const int ds = settle_p1(m); if (ds) return ds; }
    if (m->spans_p1) {
        m->spans_p1 = false;
        m->cnt.ms_filter = c->span(0, 1, 1);
        m->cnt.ms_compact = c->span(1, 2, 2);
        m->cnt.ms_survivor = c->span_survivors ? c->span(8, 9, 1) : 0.f;      // first chunk's kernel only (D2H excluded)
        m->cnt.ms_pass1_total = c->span(0, 4, 2);
    }
    if (m->spans_p2) {
        m->spans_p2 = false;
        m->cnt.ms_recruit = c->span(5, 6, 1);
        m->cnt.ms_recruit_finish = c->span(6, 7, 2);
        m->cnt.ms_pass2_total = c->span(5, 7, 2);
    }
    *o = c->cnt;
    o->n_merge_fallbacks = c->n_merge_fallbacks;
    o->last_fallback_bits = c->last_fallback_bits;
    for (int k = 0; k < 4; k++) o->n_bound_overflows[k] = c->n_bound_overflows[k];
    o->used_device_view = (c->dm.active && c->dm.view_ready) ? 1u : 0u;
    o->n_view_fallbacks = c->n_view_fallbacks.load();
    return CRASS_OK;
}

} // extern "C"

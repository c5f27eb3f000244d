// engine_pass1.cpp — pass 1 of the context behind include/crass_hip.h: the seed filter, the ordered compaction of its
// survivors, the survivor kernels and their two sinks (the dense one, whose tail stays on the device, and the host loop),
// the speculation bounds and pools of a context's first call, and a deferred pass 1's settling.  The merge a seed scan
// queues behind itself is engine_merge.cpp's (device_merge_prepare / device_merge_enqueue, declared in engine_ctx.h).
#include "engine_ctx.h"

#include <cstdio>

extern "C" {

// the main stream waits for every slice of the position hints (whoever reads them without slicing its own launches)
static int hint_wait_all(crass_hip_ctx *c)
{
    if (!c->hint_pending) return CRASS_OK;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_hint[c->hint_parts - 1], 0));
    c->hint_pending = false;
    return CRASS_OK;
}

static bool getenv_once_hl_host() { static const bool v = getenv("CRASS_HL_HOST_DEDUPE") != nullptr; return v; }      // A/B switch: the round-3 host de-duplication + merge for long reads
static bool getenv_once_copy_early() { static const bool on = getenv("CRASS_COPY_EARLY") != nullptr; return on; }      // A/B switch: the hand-off copy starts beside the merge (the old order)

// CRASS_SURV_PROF: one line per category of reads (0 skipped without a hinted seed, 1 walked / nothing found, 2 found, 3 handed
// over) with the summed cycles of the kernel's phases, then a histogram of cycles per read; the counters are cleared
static void dump_surv_prof(crass_hip_ctx *c)
{
    if (!c->dp.prof) return;
    unsigned long long v[192];
    if (hipMemcpy(v, c->dp.prof, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return;
    (void)hipMemset(c->dp.prof, 0, sizeof v);
    { const unsigned long long big = ~0ull; (void)hipMemcpy(c->dp.prof + 188, &big, 8, hipMemcpyHostToDevice); }
    if (v[191]) fprintf(stderr, "[surv_prof] %llu waves; first start .. last start %.1f us, first start .. last end %.1f us\n", v[186], (double)(v[187] - v[188]) / 100.0, (double)(v[189] - v[188]) / 100.0);
    if (v[186] && v[186] <= 16384) {
        // per-wave start / end (10 ns ticks): when did the waves of the launch start, how long did they live
        std::vector<unsigned long long> se(2 * v[186]);
        if (hipMemcpy(se.data(), c->dp.prof + 192, se.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            std::vector<double> st, life, en;
            for (size_t k = 0; k < v[186]; k++) if (se[2 * k] && se[2 * k + 1]) { st.push_back((double)(se[2 * k] - v[188]) / 100.0); en.push_back((double)(se[2 * k + 1] - v[188]) / 100.0); life.push_back((double)(se[2 * k + 1] - se[2 * k]) / 100.0); }
            auto pct = [](std::vector<double> &a, double q) { if (a.empty()) return 0.0; std::sort(a.begin(), a.end()); return a[(size_t)(q * (a.size() - 1))]; };
            fprintf(stderr, "[surv_prof] per wave (us): start p10 %.0f p50 %.0f p90 %.0f max %.0f | life p10 %.0f p50 %.0f p90 %.0f max %.0f | end p10 %.0f p50 %.0f p90 %.0f max %.0f\n",
                    pct(st, .1), pct(st, .5), pct(st, .9), pct(st, 1.), pct(life, .1), pct(life, .5), pct(life, .9), pct(life, 1.), pct(en, .1), pct(en, .5), pct(en, .9), pct(en, 1.));
        }
        (void)hipMemset(c->dp.prof + 192, 0, 2 * 16384 * 8);
    }
    if (v[185]) fprintf(stderr, "[surv_prof] slowest read: slot %llu, %llu cycles\n", v[185] & 0xFFFFFFull, v[185] >> 24);
    if (v[191]) fprintf(stderr, "[surv_prof] waves' lifetimes: %llu shader cycles in %llu ticks of 10 ns: %.3f GHz\n", v[190], v[191], (double)v[190] / (10.0 * (double)v[191]));
    static const char *nm[] = {"total", "stage", "find", "scan", "extend", "qc", "hints", "out", "n_cand", "n_scanfind", "n_switch", "n_qc", "loop", "n_iter", "max", "reads"};
    for (int cat = 0; cat < 4; cat++) {
        const unsigned long long n = v[cat * 16 + 15];
        if (!n) continue;
        fprintf(stderr, "[surv_prof] cat %d", cat);
        for (int k = 0; k < 16; k++) fprintf(stderr, " %s %llu", nm[k], v[cat * 16 + k]);
        fprintf(stderr, "\n[surv_prof] cat %d hist(log2 cycles):", cat);
        for (int b = 0; b < 24; b++) if (v[64 + cat * 24 + b]) fprintf(stderr, " %d:%llu", b + 8, v[64 + cat * 24 + b]);
        fprintf(stderr, "\n");
    }
}

// The mask / prefix / block-sum scratch is sized for the READ count at load; the three-kernel compactions over survivor and
// hit SLOTS (CRASS_NO_LOOKBACK, or after a look-back give-up) write (bound + 63) / 64 words of it, and a slot bound is not
// bounded by the read count (70 000 reads with 50 000 survivors: bound 131 072 = 2 048 words into 1 095).  Whoever sizes
// slot buffers for a bound grows the scratch with them.  (Its contents are dead between stages: a stage's mask is consumed by
// the compaction queued right behind it, and the release inside ensure() waits for the device.)
static int ensure_mask_scratch(crass_hip_ctx *c, uint64_t n_bits)
{
    const uint64_t n_words = (n_bits + 63) / 64;
    if (c->d_mask.n >= n_words + 1 && c->d_word_prefix.n >= n_words + 1 && c->d_block_sums.n >= (n_words + 255) / 256 + 2) return CRASS_OK;
    HIPCHK(c, c->d_mask.ensure(n_words + 1));
    HIPCHK(c, c->d_word_prefix.ensure(n_words + 1));
    HIPCHK(c, c->d_block_sums.ensure((n_words + 255) / 256 + 2));
    return CRASS_OK;
}

// the host-loop sink: runs the survivor kernel over `n_total` survivors (packed list in d_idx, or the exception
// list) in chunks and appends every found record, in order, to `L`
static int run_survivors(crass_hip_ctx *c, bool exc, uint64_t n_total, crass_hip_ctx::P1List &L,
                         const uint64_t *surv_idx_host)
{
    if (n_total == 0) return hint_wait_all(c);
    // Long reads: the Levenshtein fallback rows are sized for 256-base strings (spacers are a few dozen bases), which
    // is what lets several waves share a CU's LDS; a read that needs longer rows comes back with err == 6 and is
    // redone by a second launch with the full layout.  That layout's own rows are sized by the set's longest read as long as
    // it then fits a CU's 160 KB (reads up to ~28 kbp under the defaults) and by the longest string the QC can compare,
    // max(highDR, highSp) bases, beyond that (survivor_lds_last_resort: every read the library loads, up to 60 000 bases,
    // is searched); only options under which even that layout passes 160 KB (an extreme -S) are refused.  A read the full
    // layout answers err 6 for is an error status of the scan (the sink's worst-error word), never a dropped read.
    const SurvLds lds_full = survivor_lds_last_resort(c->max_len, c->dp);
    if (lds_full.total_bytes > 160 * 1024) return CRASS_ERR_UNSUPPORTED;
    const bool rows_bounded = lds_full.row_elems < survivor_lds_layout(c->max_len, c->dp).row_elems;
    // (tests: CRASS_ROW_CAP forces the second launch; no launch of a set asks for longer rows than its last resort has)
    const uint32_t row_cap = rows_bounded ? std::min(c->env.row_cap, std::max(c->dp.highDR, c->dp.highSp)) : c->env.row_cap;
    // Reads beyond 2 048 bases also get an ASCII WINDOW instead of room for the whole read (the byte-wise consumers only ever
    // read around the repeats of the candidate in hand: rh_ascii) and a start/stop list of 256 entries: 11.5 instead of 19.7 KB
    // of LDS per wave at 10 kbp — three waves per SIMD (with 168 registers) instead of two.  An array longer than the window
    // (> ~4.2 kbp), a 129th repeat or a string beyond the rows: the second launch.  CRASS_LONG_FULL_LAYOUT: the A/B switch.
    // (both read per call — once per seed scan of a long-read set —, so that a test can change them inside one process)
    const bool long_full = getenv("CRASS_LONG_FULL_LAYOUT") != nullptr;
    const uint32_t win_env = getenv("CRASS_SEQ_WINDOW") ? (uint32_t)atoi(getenv("CRASS_SEQ_WINDOW")) : 0u;      // (tests: a tiny window)
    const bool windowed = !exc && (win_env || (c->max_len > c->env.long_min && !long_full));
    const SurvLds lds = windowed ? survivor_lds_layout(c->max_len, c->dp, row_cap, win_env ? win_env : 4608u, 256u)
                                 : survivor_lds_layout(c->max_len, c->dp, row_cap);
    const bool capped = lds.row_elems != lds_full.row_elems || lds.seq_window != 0 || lds.ss_cap != lds_full.ss_cap;
    const uint64_t chunk_cap = std::min<uint64_t>(n_total, 1u << 20);
    const uint64_t ss_per = std::min<uint64_t>(lds_full.ss_cap, 64);
    const uint64_t pool_cap = std::min<uint64_t>(std::max<uint64_t>(chunk_cap * ss_per, 1u << 16), 1ull << 28);
    HIPCHK(c, c->d_surv.ensure(chunk_cap));
    HIPCHK(c, c->d_dr.ensure(chunk_cap * c->dr_stride));
    HIPCHK(c, c->d_ss_pool.ensure(pool_cap));
    HIPCHK(c, c->h_surv.ensure(chunk_cap));
    HIPCHK(c, c->h_dr.ensure(chunk_cap * c->dr_stride));
    // the survivor list on the device is 0, 1, 2, ... (no filter, no exception read, one chunk): the kernel is told so and needs no
    // look-up per read
    const bool ident_list = !exc && !surv_idx_host && c->R.n_exc == 0 && n_total <= chunk_cap;
    // ... and with position hints on top the walk is split: k_long_light for every read, the full kernel for what it hands over
    // (CRASS_NO_LIGHT: the A/B switch; the cut-short walks of CRASS_SURV_DEBUG belong to the full kernel)
    // ... or without position hints, for another window or seed lattice (-w / -d): k_long_light_any computes every position's bit itself
    const uint32_t sh0 = c->dp.lowDR + c->dp.lowSp, sh1 = c->dp.highDR + c->dp.highSp;
    const bool light_any = !c->R.pos_hint && c->max_len > c->env.long_min && !(c->dp.window == 8 && c->dp.skips == 8) && c->dp.window >= 6 && c->dp.window <= 9 &&
                           sh0 >= 17 && sh1 <= 127 && sh1 >= sh0 && !c->env.no_pos_hints;
    const bool use_light = ident_list && ((c->R.pos_hint && c->dp.skips == 8 && c->dp.window == 8) || light_any) && c->dp.debug_stop == 0 && !getenv("CRASS_NO_LIGHT");
    const int grid = 256 * 64;      // waves striding over the reads: 6 resident per CU at 10 kbp; 1 536 / 8 192 / 16 384 / 65 536 blocks: 11.5 / 8.6 / 8.2 / 9.1 ms
    const uint32_t stride = c->dr_stride;
    L.reserve(L.size() + n_total / 2 + 16, stride);
    for (uint64_t off = 0; off < n_total; off += chunk_cap) {
        const uint64_t nchunk = std::min(chunk_cap, n_total - off);
        HIPCHK(c, hipMemsetAsync(c->d_ss_used.p, 0, 4, c->stream));
        DevReads R = c->R;
        if (exc) {      // shift the exception window
            R.exc_read = c->R.exc_read + off; R.exc_off = c->R.exc_off + off; R.n_exc = nchunk;
        }
        // for the non-exception path the count lives on the device; chunking uses a host-known bound
        if (use_light) {
            HIPCHK(c, c->d_punt.ensure(nchunk + 1)); HIPCHK(c, hipMemsetAsync(c->d_punt.p, 0, 4, c->stream));
            HIPCHK(c, c->d_redo.ensure(nchunk + 1)); HIPCHK(c, hipMemsetAsync(c->d_redo.p, 0, 4, c->stream));
        }
        if (!exc && off == 0) HIPCHK(c, c->stamp(8, 1));
        if (!exc && c->hint_pending && off == 0 && nchunk == n_total) {
            // the walk, slice by slice behind the slice's hints (slot boundaries: the survivors with a read below the slice's end;
            // the list is ascending, and 0, 1, 2, ... when no host copy of it was made)
            uint64_t s0 = 0;
            for (int q = 0; q < c->hint_parts; q++) {
                const uint64_t r1 = c->hint_read_split[q + 1];
                uint64_t s1 = q + 1 == c->hint_parts ? nchunk
                            : (surv_idx_host ? (uint64_t)(std::lower_bound(surv_idx_host, surv_idx_host + nchunk, r1) - surv_idx_host) : std::min<uint64_t>(r1, nchunk));
                if (q > 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_hint[q], 0));
                if (s1 > s0 && use_light)
                    HIPCHK(c, launch_long_light(R, c->dp, c->d_count.p + 1, s1 - s0, c->d_surv.p + s0, s0, c->max_len, c->stream, c->d_punt.p + 1, c->d_punt.p));
                else if (s1 > s0)
                    HIPCHK(c, launch_survivor(R, c->dp, false, ident_list ? nullptr : c->d_idx.p + s0, c->d_count.p + 1, s1 - s0,
                                              c->d_surv.p + s0, c->d_dr.p + s0 * (size_t)stride, stride, c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p,
                                              c->d_found.p, c->hints_valid ? c->d_hit_info.p : nullptr, lds,
                                              (int)std::min<uint64_t>(grid, s1 - s0), c->stream, 0, s0, nchunk));
                s0 = s1;
            }
            c->hint_pending = false;
        } else if (use_light) {
            { const int hw = hint_wait_all(c); if (hw) return hw; }
            HIPCHK(c, launch_long_light(R, c->dp, c->d_count.p + 1, nchunk, c->d_surv.p, 0, c->max_len, c->stream, c->d_punt.p + 1, c->d_punt.p));
        } else {
            { const int hw = hint_wait_all(c); if (hw) return hw; }
            HIPCHK(c, launch_survivor(R, c->dp, exc, (exc || ident_list) ? nullptr : c->d_idx.p + off, c->d_count.p + (exc ? 0 : 1), nchunk,
                                      c->d_surv.p, c->d_dr.p, stride, c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p,
                                      c->d_found.p, (!exc && c->hints_valid) ? c->d_hit_info.p : nullptr, lds,
                                      (int)std::min<uint64_t>(grid, nchunk), c->stream));
        }
        // the reads the light walk handed over (an array, a candidate due for the QC: one read in 17 at 10 kbp): the full kernel
        if (use_light)
            HIPCHK(c, launch_survivor(R, c->dp, false, nullptr, c->d_count.p + 1, nchunk,
                                      c->d_surv.p, c->d_dr.p, stride, c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p,
                                      c->d_found.p, nullptr, lds, (int)std::min<uint64_t>(256 * 12, nchunk), c->stream, 7, 0, nchunk, c->d_punt.p + 1, c->d_punt.p,
                                      capped ? c->d_redo.p : nullptr));
        if (use_light && c->dp.prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); dump_surv_prof(c); }      // (diagnostics: this launch's counters alone)
        if (capped && use_light)                    // (only the full kernel can have met such a read: its list)
            HIPCHK(c, launch_survivor(R, c->dp, false, nullptr, c->d_count.p + 1, nchunk,
                                      c->d_surv.p, c->d_dr.p, stride, c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p,
                                      c->d_found.p, nullptr, lds_full, (int)std::min<uint64_t>(256 * 2, nchunk), c->stream, 6, 0, nchunk, c->d_redo.p + 1, c->d_redo.p));
        else if (capped)
            HIPCHK(c, launch_survivor(R, c->dp, exc, (exc || ident_list) ? nullptr : c->d_idx.p + off, c->d_count.p + (exc ? 0 : 1), nchunk,
                                      c->d_surv.p, c->d_dr.p, stride, c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p,
                                      c->d_found.p, (!exc && c->hints_valid) ? c->d_hit_info.p : nullptr, lds_full,
                                      (int)std::min<uint64_t>(grid, nchunk), c->stream, 6));
        if (!exc && off == 0) HIPCHK(c, c->stamp(9, 1));
        // only the FOUND records travel (all 1 M reads of a 10 kbp set are survivors, 5 % are found; copying every slot
        // and every start/stop slot area was 340 MB and 10 of 39 ms per step): select -> ordered index list -> gather
        // into dense arrays with the start/stops packed -> three counters -> exact-size copies
        const uint64_t n_words = (nchunk + 63) / 64;
        HIPCHK(c, c->d_fidx.ensure(nchunk)); HIPCHK(c, c->g_surv.ensure(nchunk)); HIPCHK(c, c->g_dr.ensure(nchunk * (size_t)stride + 16));
        HIPCHK(c, c->g_ss.ensure(pool_cap)); HIPCHK(c, c->g_fidx.ensure(nchunk));
        HIPCHK(c, c->d_mask.ensure(n_words + 1)); HIPCHK(c, c->d_word_prefix.ensure(n_words + 1)); HIPCHK(c, c->d_block_sums.ensure((n_words + 255) / 256 + 2));
        HIPCHK(c, hipMemsetAsync(c->d_count.p + 2, 0, 8, c->stream));            // [2] found, [3] worst error
        HIPCHK(c, hipMemsetAsync(c->d_ss_used.p, 0, 4, c->stream));              // (reused: words of packed start/stops)
        HIPCHK(c, launch_select_found(c->d_surv.p, nchunk, c->d_mask.p, c->d_count.p + 3, c->stream));
        HIPCHK(c, launch_compact(c->d_mask.p, n_words, nchunk, c->d_word_prefix.p, c->d_block_sums.p, c->d_fidx.p, nchunk, c->d_count.p + 2, c->stream));
        // One chunk of a set without exception reads: the found records' strings are de-duplicated on the device as well (the
        // kernels of the dense sink's tail, queued behind the first wait with the exact count, beside the copies and the host
        // loop below) — the distinct list in token order + every candidate's index in it are what the DEVICE merge takes, so a
        // long-read set no longer hashes 50 k strings and clusters them on the host (1.3 ms per step at 1 M x 10 kbp)
        const bool ss16 = c->max_len < 65536;           // start/stops travel as 16-bit values
        const bool hl_dedupe = !exc && off == 0 && nchunk == n_total && c->R.n_exc == 0 && !c->xchg.active && !c->env.host_merge &&
                               c->prm.lowDRsize >= (int)kDevMinDR && stride <= 64 && (stride & 15u) == 0 && nchunk < (1u << 24) && !getenv_once_hl_host();
        if (hl_dedupe) HIPCHK(c, c->g_dr_len.ensure(nchunk));
        HIPCHK(c, launch_gather_sparse(c->d_fidx.p, c->d_count.p + 2, nchunk, c->d_surv.p, c->d_dr.p, stride, c->d_ss_pool.p, c->g_surv.p,
                                       c->g_fidx.p, c->g_dr.p, c->g_ss.p, (uint32_t)pool_cap, c->d_ss_used.p, c->stream,
                                       hl_dedupe ? c->g_dr_len.p : nullptr, ss16 ? 1 : 0));
        HIPCHK(c, hipMemcpyAsync(c->h_count.p + 2, c->d_count.p + 2, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_count.p + 6, c->d_ss_used.p, 4, hipMemcpyDeviceToHost, c->stream));
        const double tq0 = now_ms();
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const double tq1 = now_ms();
        dump_surv_prof(c);
        if (c->h_count.p[3] == 2) return CRASS_ERR_SEARCH_FATAL;
        if (c->h_count.p[3]) return CRASS_ERR_OVERFLOW;
        const uint64_t nf = c->h_count.p[2];
        const uint32_t used = c->h_count.p[6];
        if (nf > nchunk || used > pool_cap) return CRASS_ERR_OVERFLOW;
        HIPCHK(c, c->h_ss.ensure(used + 1)); HIPCHK(c, c->h_idx.ensure(nf + 1));
        // the copies: on the copy stream when the records' consumers can wait (one chunk, no exception list to merge with, slots =
        // reads: `cand` is then filled on request, materialize_cand) — the main stream goes on with the de-duplication, the
        // merge and pass 2 —, else on the main stream with the host loop right behind them
        static const bool sink_eager = getenv("CRASS_SINK_EAGER") != nullptr;      // A/B switch
        const bool lazy = !sink_eager && !exc && off == 0 && nchunk == n_total && c->R.n_exc == 0 && !surv_idx_host && &L == &c->cand && L.read.empty();
        if (nf) {
            hipStream_t cs = lazy ? c->copy_stream : c->stream;      // (the main stream is idle: it was waited for above)
            // lazy: on DMA engines where the runtime offers them — as blit kernels these 12 MB of PCIe stores stretched whatever
            // ran beside them (k_block_scan of the de-duplication: 138 us instead of 5, profiles/r05_timeline_c3.txt)
            // (the records' slots are gathered into a buffer of their own, g_fidx: d_fidx is written again by pass 2, and the copies
            // below may still be reading when it is queued — crass_hip_recruit used to wait for them, 0.5 ms of a long-read step)
            const void *srcs[4] = {c->g_surv.p, c->g_dr.p, c->g_fidx.p, c->g_ss.p};
            void *dsts[4] = {c->h_surv.p, c->h_dr.p, c->h_idx.p, c->h_ss.p};
            const size_t nbs[4] = {nf * sizeof(SurvOut), nf * (size_t)stride, nf * 8, used ? (size_t)used * (ss16 ? 2 : 4) : 0};
            static const bool sink_blit = getenv("CRASS_COPY_BLIT") != nullptr;
            for (int q = 0; q < 4; q++) {
                if (!nbs[q]) continue;
                if (lazy && !sink_blit) {
                    if (!c->dma_sink[q]) c->dma_sink[q] = sdma_create();
                    if (sdma_start(c->dma_sink[q], srcs[q], dsts[q], nbs[q])) continue;
                }
                HIPCHK(c, hipMemcpyAsync(dsts[q], srcs[q], nbs[q], hipMemcpyDeviceToHost, cs));
            }
            if (lazy) {
                if (!c->ev_sink_copies) HIPCHK(c, hipEventCreateWithFlags(&c->ev_sink_copies, hipEventDisableTiming));
                HIPCHK(c, hipEventRecord(c->ev_sink_copies, c->copy_stream));
                c->bulk_pending = true;
            }
            else HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        bool hl_queued = false, hl_premerge = false;
        if (nf && hl_dedupe) {
            // (behind the copies above; the host loop below runs beside these kernels; their small outputs land in pinned memory)
            uint32_t tsize = 1024;
            while (tsize < nf * 2) tsize <<= 1;
            HIPCHK(c, c->dd_keys.ensure(tsize)); HIPCHK(c, c->dd_first.ensure(tsize)); HIPCHK(c, c->dd_slot.ensure(nf)); HIPCHK(c, c->dd_rep.ensure(nf));
            HIPCHK(c, c->dd_hash.ensure(nf)); HIPCHK(c, c->hl_dx_idx.ensure(nf));
            HIPCHK(c, c->dd_dx_chars.ensure(nf * (size_t)stride + 16)); HIPCHK(c, c->dd_dx_len.ensure(nf));
            HIPCHK(c, c->h_dmap.ensure(nf)); HIPCHK(c, c->h_dx_chars.ensure(nf * (size_t)stride + 16)); HIPCHK(c, c->h_dx_len.ensure(nf)); HIPCHK(c, c->h_dx_hash.ensure(nf));
            { const int ms = ensure_mask_scratch(c, nf); if (ms) return ms; }
            HIPCHK(c, hipMemsetAsync(c->d_count.p + 4, 0, 8, c->stream));            // [4] distinct strings, [5] mismatch flag
            HIPCHK(c, launch_dr_dedupe(c->g_dr.p, c->g_dr_len.p, stride, c->d_count.p + 2, (uint32_t)nf, c->dd_keys.p, c->dd_first.p, tsize, c->dd_hash.p,
                                       c->dd_slot.p, c->dd_rep.p, c->stream, false));
            HIPCHK(c, launch_dx_tokens(c->g_dr.p, c->g_dr_len.p, c->dd_hash.p, stride, c->d_count.p + 2, (uint32_t)nf, c->dd_rep.p, c->dd_slot.p, c->dd_first.p,
                                       c->d_mask.p, c->d_word_prefix.p, c->d_block_sums.p, c->hl_dx_idx.p, c->d_count.p + 4, c->d_count.p + 5, c->h_dmap.p,
                                       c->h_dx_chars.p, c->h_dx_len.p, c->h_dx_hash.p, c->dd_dx_chars.p, c->dd_dx_len.p, c->stream,
                                       c->d_count.p, c->h_count.p, 8, nullptr));
            hl_queued = true;
            // the merge itself right behind (its kernels read the token count from the device and are sized for nf, a bound on
            // it): it runs while the host returns from this call and enters crass_hip_merge, which adopts it
            HIPCHK(c, hipEventRecord(c->ev_gathered, c->stream));
            c->premerge = 0; c->premerge_inflight = false;
            if (!c->env.no_speculation && nf <= (1u << 18)) {
                const int ps = device_merge_enqueue(c, c->dd_dx_chars.p, c->dd_dx_len.p, nf, c->d_count.p + 4, false);
                if (ps) return ps;
                HIPCHK(c, hipEventRecord(c->ev_premerge, c->stream));
                hl_premerge = true;
            }
        }
        const double tq2 = now_ms();
        auto fill = [c, nf, ss16, stride, exc, off, surv_idx_host, &L]() {
        if (c->wait_bulk()) return;                         // (the copies; a failed one is reported by whoever asks for the records)
        const SurvOut *so = c->h_surv.p;
        const char *drs = c->h_dr.p;
        const uint32_t *pool = c->h_ss.p;
        // append the chunk's records: offsets first (one pass), then every array filled in place by the host pool
        // (50 k records with 80 start/stops each at 10 kbp: 20 MB, 4 ms on one thread)
        const size_t base = L.read.size();
        L.read.resize(base + nf); L.low.resize(base + nf); L.replen.resize(base + nf); L.nss.resize(base + nf);
        L.ss_off.resize(base + nf); L.dr_len.resize(base + nf); L.dr.resize((base + nf) * (size_t)stride);
        uint64_t at = L.ss.size();
        for (uint64_t q = 0; q < nf; q++) { L.ss_off[base + q] = at; at += so[q].n_ss; }
        L.ss.resize(at);
        const size_t per_task = 2048;
        host_parallel_for((nf + per_task - 1) / per_task, 16, [&](size_t t) {
            const uint64_t q1 = std::min<uint64_t>(nf, (t + 1) * per_task);
            for (uint64_t q = t * per_task; q < q1; q++) {
                const SurvOut &o = so[q];
                const uint64_t k = c->h_idx.p[q];                // the record's slot in the chunk
                L.read[base + q] = c->read_base + (exc ? c->h_exc_read[off + k] : (surv_idx_host ? surv_idx_host[off + k] : off + k));
                L.low[base + q] = o.low_lexi;
                L.replen[base + q] = o.repeat_len;
                L.nss[base + q] = o.n_ss;
                if (ss16) { const uint16_t *p16 = reinterpret_cast<const uint16_t *>(pool) + o.ss_off; uint32_t *d = L.ss.data() + L.ss_off[base + q]; for (uint32_t i = 0; i < o.n_ss; i++) d[i] = p16[i]; }
                else memcpy(L.ss.data() + L.ss_off[base + q], pool + o.ss_off, (size_t)o.n_ss * 4);
                L.dr_len[base + q] = o.dr_len;
                memcpy(L.dr.data() + (base + q) * (size_t)stride, drs + q * stride, stride);
            }
        });
        };
        if (lazy && nf) { c->cand_fill = fill; c->cand_pending_n = nf; }      // (L is c->cand: it outlives this call)
        else fill();
        if (hl_queued) {
            HIPCHK(c, hipEventSynchronize(c->ev_gathered));      // (the de-duplication's counters; the merge behind it may still run)
            c->premerge_inflight = hl_premerge;
            if (c->h_count.p[5] == 0 && c->h_count.p[2] == nf && c->h_count.p[4] > 0) {
                c->n_dx = c->h_count.p[4];
                c->have_dev_tokens = true; c->hl_tokens = true;
                c->dx_hash_valid = true;
                if (hl_premerge) c->premerge = 2;
            }
        }
        if (c->env.merge_profile)
            fprintf(stderr, "[crass_sink] survivors %llu: kernel+D2H wait %.3f ms, pool D2H %.3f ms, host loop %.3f ms\n",
                    (unsigned long long)nchunk, tq1 - tq0, tq2 - tq1, now_ms() - tq2);
    }
    return CRASS_OK;
}

// A long-read set (position hints: no per-read filter, every read is a survivor) takes the host-loop sink; crass scans a read
// set ONCE, so what that sink and the stages behind it allocate on their first call is allocated with the reads — best effort:
// whatever cannot be had now is had then, as before (the first step of a 1 M x 10 kbp set: 17.4 ms against 10.3 in steady
// state; the guesses: one found read in eight, 128 start/stops per found read)
void presize_hostloop(crass_hip_ctx *c)
{
    if (!c->R.pos_hint || c->max_len <= c->env.long_min || c->env.no_presize || c->R.n_reads == 0) return;
    const SurvLds lds_full = survivor_lds_last_resort(c->max_len, c->dp);      // (run_survivors' test: what it refuses is not sized)
    if (lds_full.total_bytes > 160 * 1024) return;
    for (auto &d : c->dma_sink) if (!d) d = sdma_create();      // (an engine's queue is created by its first copy, ~6 ms: here)
    const uint64_t chunk_cap = std::min<uint64_t>(c->R.n_reads, 1u << 20);
    const uint64_t ss_per = std::min<uint64_t>(lds_full.ss_cap, 64);
    const uint64_t pool_cap = std::min<uint64_t>(std::max<uint64_t>(chunk_cap * ss_per, 1u << 16), 1ull << 28);
    const uint32_t stride = c->dr_stride;
    const uint64_t nf = std::min<uint64_t>(chunk_cap, std::max<uint64_t>(65536, chunk_cap / 8));
    const uint64_t n_words = (chunk_cap + 63) / 64;
    const uint32_t tsize = dedupe_table_size(nf);
    bool ok = true;
    auto need = [&](hipError_t e) { if (e != hipSuccess) ok = false; };
    need(c->d_punt.ensure(chunk_cap + 1)); need(c->d_redo.ensure(chunk_cap + 1));
    need(c->d_surv.ensure(chunk_cap)); need(c->d_dr.ensure(chunk_cap * stride)); need(c->d_ss_pool.ensure(pool_cap));
    need(c->h_surv.ensure(chunk_cap)); need(c->h_dr.ensure(chunk_cap * stride));
    need(c->d_fidx.ensure(chunk_cap)); need(c->g_surv.ensure(chunk_cap)); need(c->g_dr.ensure(chunk_cap * (size_t)stride + 16)); need(c->g_ss.ensure(pool_cap));
    need(c->g_fidx.ensure(chunk_cap));
    need(c->d_mask.ensure(n_words + 1)); need(c->d_word_prefix.ensure(n_words + 1)); need(c->d_block_sums.ensure((n_words + 255) / 256 + 2));
    need(c->g_dr_len.ensure(chunk_cap)); need(c->h_ss.ensure(nf * 128 + 1)); need(c->h_idx.ensure(nf + 1));
    need(c->dd_keys.ensure(tsize)); need(c->dd_first.ensure(tsize)); need(c->dd_slot.ensure(nf)); need(c->dd_rep.ensure(nf));
    need(c->dd_hash.ensure(nf)); need(c->hl_dx_idx.ensure(nf)); need(c->dd_dx_chars.ensure(nf * (size_t)stride + 16)); need(c->dd_dx_len.ensure(nf));
    need(c->h_dmap.ensure(nf)); need(c->h_dx_chars.ensure(nf * (size_t)stride + 16)); need(c->h_dx_len.ensure(nf)); need(c->h_dx_hash.ensure(nf));
    if (ok && c->prm.lowDRsize >= (int)kDevMinDR && stride <= 64 && !c->env.host_merge && !c->xchg.active)
        (void)device_merge_prepare(c, c->dd_dx_chars.p, c->dd_dx_len.p, std::min<uint64_t>(nf, 1u << 18), nullptr);      // (the merge's tables: buffers only, nothing is launched)
    c->last_hip = 0;
}

// 2^26 survivors = 100 M+ read shards at the ~2 % filter pass rate; the slot pool stays below 2^31 words
static const uint64_t kDenseMaxSurvivors = 1ull << 26;

// every buffer the dense pass-1 sink touches for up to n_alloc survivors (crass_hip_load_reads sizes them for the first
// call's bound, so that the first seed scan of a context does not allocate; ensure() is a no-op when a buffer is large enough)
static int ensure_dense_buffers(crass_hip_ctx *c, uint64_t n_alloc, uint64_t pool_cap, const SurvLds &lds, bool dedupe)
{
    crass_hip_ctx::P1Dense &D = c->dense;
    const uint32_t stride = c->dr_stride;
    { const int ms = ensure_mask_scratch(c, n_alloc); if (ms) return ms; }
    HIPCHK(c, c->d_surv.ensure(n_alloc));
    HIPCHK(c, c->d_dr.ensure(n_alloc * stride));
    HIPCHK(c, c->d_ss_pool.ensure(std::max<uint64_t>(pool_cap, n_alloc * (uint64_t)lds.ss_cap)));
    HIPCHK(c, c->d_fidx.ensure(n_alloc));
    HIPCHK(c, D.d_dr_len.ensure(n_alloc + 8)); HIPCHK(c, D.d_dr.ensure(n_alloc * stride + 16));
    const uint32_t ss_elem = c->max_len <= 256 ? 1u : 2u;            // read positions fit a byte
    HIPCHK(c, D.h_blob.ensure(p1_blob_layout(n_alloc, lds.ss_cap, ss_elem).total + 64));
    HIPCHK(c, D.d_blob.ensure(D.h_blob.n));
    if (dedupe) {
        const uint32_t tsize_alloc = dedupe_table_size(n_alloc);
        HIPCHK(c, c->dd_keys.ensure(tsize_alloc)); HIPCHK(c, c->dd_first.ensure(tsize_alloc));
        HIPCHK(c, c->dd_slot.ensure(n_alloc)); HIPCHK(c, c->dd_hash.ensure(n_alloc));
        HIPCHK(c, c->dd_rep.ensure(n_alloc)); HIPCHK(c, c->h_rep.ensure(n_alloc)); HIPCHK(c, c->h_hash.ensure(n_alloc));
        HIPCHK(c, c->h_dmap.ensure(n_alloc)); HIPCHK(c, c->h_dx_chars.ensure(n_alloc * stride + 16)); HIPCHK(c, c->h_dx_len.ensure(n_alloc));
        HIPCHK(c, c->h_dx_hash.ensure(n_alloc));
        HIPCHK(c, c->dd_dx_chars.ensure(n_alloc * stride + 16)); HIPCHK(c, c->dd_dx_len.ensure(n_alloc));
        if (c->dx_via_dma) HIPCHK(c, c->dd_map.ensure(n_alloc));
    }
    return CRASS_OK;
}

// the host's half of the dense pass-1 tail: waits for the kernels queued by run_survivors_dense, reads the counters they left in
// pinned memory, starts the hand-off copies
static int dense_after_sync(crass_hip_ctx *c, uint64_t n_surv, uint32_t ss_cap, uint32_t ss_elem, bool dedupe, bool premerge_queued, bool *overflow)
{
    crass_hip_ctx::P1Dense &D = c->dense;
    const uint32_t stride = c->dr_stride;
    // (with the merge queued behind it, the host waits for pass 1 only — the event recorded above — and goes on to
    // adopt the merge and queue pass 2 while the merge kernels run)
    if (premerge_queued || c->p1d.finishing) {
        if (!c->poll_on) HIPCHK(c, hipEventSynchronize(c->ev_gathered));
        else if (!c->poll_flag(c->p1d.finishing ? 0 : 1, c->p1d.finishing ? c->want_p1 : c->want_pre, 200.0)) HIPCHK(c, hipStreamSynchronize(c->stream));
    } else HIPCHK(c, hipStreamSynchronize(c->stream));
    c->premerge_inflight = premerge_queued;
    c->t_p1_sync = now_ms();
    const uint32_t *hc = c->p1_counts();
    if (hc[0] > n_surv) { *overflow = true; return CRASS_OK; }
    const uint64_t nf = hc[2];
    const uint32_t err = hc[3];
    if (err == 1) return CRASS_ERR_SEARCH_FATAL;
    if (err) return CRASS_ERR_OVERFLOW;
    D.lay = p1_blob_layout(nf, ss_cap, ss_elem);
    if (nf) {
        // the hand-off records: the host has waited for the gather, the copy runs beside what follows.  As PCIe stores from
        // shader waves (the runtime's blit kernel or ours) it cost the kernels beside it its own 0.2-0.3 ms wherever it was
        // placed — k_dm_pack_codes 0.29 instead of 0.02 ms, or k_dm_greedy 0.27 instead of 0.06, or pass 2's filter 1.32
        // instead of 1.11 (profiles/NOTES_r03.md).  The fall-back order keeps it away from the merge, whose kernels are
        // short dependent chains of agent-scope loads and atomics.
        static const bool blit = getenv("CRASS_COPY_BLIT") != nullptr;      // A/B switch: the runtime's copy (a blit kernel over every CU)
        if (!blit && sdma_start(c->dma, D.d_blob.p, D.h_blob.p, D.lay.total)) {
            // (a DMA engine: nothing of it runs on the CUs, it starts now)
        } else {
            if (premerge_queued && !getenv_once_copy_early()) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_premerge, 0));
            if (blit) HIPCHK(c, hipMemcpyAsync(D.h_blob.p, D.d_blob.p, D.lay.total, hipMemcpyDeviceToHost, c->copy_stream));
            else HIPCHK(c, launch_copy_to_host(D.d_blob.p, D.h_blob.p, D.lay.total, c->copy_stream));
        }
        c->bulk_pending = true;
    }
    if (nf && !dedupe) {                                // no distinct list: the candidates' own strings travel
        HIPCHK(c, D.h_dr_fb.ensure(nf * stride + 16)); HIPCHK(c, D.h_dr_len_fb.ensure(nf + 8));
        HIPCHK(c, hipMemcpyAsync(D.h_dr_fb.p, D.d_dr.p, nf * stride, hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(c, hipMemcpyAsync(D.h_dr_len_fb.p, D.d_dr_len.p, nf * 2, hipMemcpyDeviceToHost, c->copy_stream));
        D.dr_fallback = true;
        c->bulk_pending = true;
    }
    if (nf) {
        if (dedupe) {
            if (hc[5] == 0) {
                c->n_dx = hc[4];
                c->have_dev_tokens = true;
                c->dx_hash_valid = !c->dx_via_dma;
                if (c->dx_via_dma) {
                    // (the host has waited for the kernels that wrote these: the engines start at once, beside the merge)
                    std::lock_guard<std::mutex> lk(c->dx_mu);
                    const void *src[3] = {c->dd_map.p, c->dd_dx_chars.p, c->dd_dx_len.p};
                    void *dst[3] = {c->h_dmap.p, c->h_dx_chars.p, c->h_dx_len.p};
                    const size_t bytes[3] = {(size_t)nf * 4, (size_t)c->n_dx * stride, (size_t)c->n_dx * 2};
                    for (int q = 0; q < 3; q++) {
                        if (!bytes[q] || sdma_start(c->dma_dx[q], src[q], dst[q], bytes[q])) continue;
                        HIPCHK(c, hipMemcpyAsync(dst[q], src[q], bytes[q], hipMemcpyDeviceToHost, c->copy_stream));
                        c->dx_stream_copy = true;
                    }
                    c->dx_pending = true;
                }
                if (premerge_queued && c->n_dx > 0 && c->n_dx <= c->dx_cap_hint) c->premerge = 2;
                else if (premerge_queued && c->n_dx > c->dx_cap_hint) c->n_bound_overflows[1]++;     // (crass_hip_merge launches its own)
            } else if (hc[5] & 2u) {
                // the de-duplication table was sized for fewer distinct strings than there are: nothing of it is usable.  The
                // candidates' own strings travel, the host de-duplicates them, and later calls size the table for the slots.
                c->dd_full_table = true;
                c->n_bound_overflows[1]++;
                HIPCHK(c, D.h_dr_fb.ensure(nf * stride + 16)); HIPCHK(c, D.h_dr_len_fb.ensure(nf + 8));
                HIPCHK(c, hipMemcpyAsync(D.h_dr_fb.p, D.d_dr.p, nf * stride, hipMemcpyDeviceToHost, c->copy_stream));
                HIPCHK(c, hipMemcpyAsync(D.h_dr_len_fb.p, D.d_dr_len.p, nf * 2, hipMemcpyDeviceToHost, c->copy_stream));
                D.dr_fallback = true;
                c->bulk_pending = true;
            } else {
                // (hash collision among the candidates: the host merge wants the first-occurrence map)
                HIPCHK(c, D.h_dr_fb.ensure(nf * stride + 16)); HIPCHK(c, D.h_dr_len_fb.ensure(nf + 8));
                HIPCHK(c, hipMemcpyAsync(D.h_dr_fb.p, D.d_dr.p, nf * stride, hipMemcpyDeviceToHost, c->copy_stream));
                HIPCHK(c, hipMemcpyAsync(D.h_dr_len_fb.p, D.d_dr_len.p, nf * 2, hipMemcpyDeviceToHost, c->copy_stream));
                D.dr_fallback = true;
                HIPCHK(c, hipMemcpyAsync(c->h_rep.p, c->dd_rep.p, nf * 4, hipMemcpyDeviceToHost, c->copy_stream));
                HIPCHK(c, hipMemcpyAsync(c->h_hash.p, c->dd_hash.p, nf * 8, hipMemcpyDeviceToHost, c->copy_stream));
                c->bulk_pending = true;
                c->have_rep = true;
            }
        }
    } else D.lay.total = 0;
    D.n = nf;
    D.active = true;
    return CRASS_OK;
}

// Fast path of the pass-1 sink: one chunk, fixed start/stop slots, no exception reads.  Returns
// CRASS_ERR_STATE when it does not apply (the caller then uses the host-loop path).
// n_surv: number of filter survivors, or (speculative mode: d_nsurv = the compaction's device-side count, no host
// round trip before this call) an upper bound for it.  The exact count then arrives with the final copy of
// the counters; *overflow is set when it exceeds the bound (nothing of this call is valid then).
// defer: the launch is queued and the function returns WITHOUT waiting for it (c->p1d holds what dense_after_sync needs) — a rank
// of a multi-rank job, whose exchange and merge can be queued behind pass 1 before the host has seen a count (p1_finish)
static int run_survivors_dense(crass_hip_ctx *c, uint64_t n_surv, const uint32_t *d_nsurv, bool *overflow, bool defer = false)
{
    *overflow = false;
    { const int hw = hint_wait_all(c); if (hw) return hw; }
    const SurvLds lds = survivor_lds_layout(c->max_len, c->dp);
    if (lds.total_bytes > 160 * 1024) return CRASS_ERR_UNSUPPORTED;
    const uint32_t stride = c->dr_stride;
    const uint64_t pool_cap = std::max<uint64_t>(n_surv * (uint64_t)lds.ss_cap, 1u << 16);
    if (n_surv == 0 || n_surv > kDenseMaxSurvivors || pool_cap >= (1ull << 31) || lds.ss_cap > 128 || (stride & 15)) return CRASS_ERR_STATE;
    crass_hip_ctx::P1Dense &D = c->dense;
    // buffers are sized for the bound the NEXT call will speculate with (1.5 x this call's count, see
    // crass_hip_seed_scan), so that the second call of a context does not re-allocate everything
    const bool speculative = (d_nsurv == c->d_count.p);          // n_surv is already such a bound
    const uint64_t n_alloc = speculative ? n_surv : std::max<uint64_t>(n_surv, survivor_bound(n_surv));
    const uint32_t ss_elem = c->max_len <= 256 ? 1u : 2u;            // read positions fit a byte
    const bool dedupe = n_surv < (1u << 24);
    const bool defer_ok = defer && dedupe && speculative && c->xchg.active;
    { const int as = ensure_dense_buffers(c, n_alloc, pool_cap, lds, dedupe); if (as) return as; }
    // [2] = found count, [3] = worst error, [4] = n distinct, [5] = de-duplication mismatch flag
    if (!speculative) {                                 // (speculative launch: cleared by the filter's compaction, see seed scan)
        HIPCHK(c, hipMemsetAsync(c->d_count.p + 2, 0, 20, c->stream));      // ([6]: the lane kernel's punt count)
        HIPCHK(c, hipMemsetAsync(c->d_ss_used.p, 0, 4, c->stream));
    }
    // The merge that will follow this stage is sized here already when the previous call's merge ran on the device (its
    // kernels read the token count from the device and are sized by a bound): the survivor kernel then clears the
    // merge's tables on its way, and the merge is queued right behind pass 1's tail further down.
    c->dm_prepared_n = 0; c->dm_prepared_src = nullptr;
    const DevMerge *init_merge = nullptr;
    if (speculative && dedupe && c->prm.lowDRsize >= (int)kDevMinDR && stride <= 64 && !c->env.host_merge && !c->env.no_speculation && !c->env.dm_init_late) {
        const char *src = nullptr; const uint16_t *src_len = nullptr; uint64_t bound = 0;
        if (!c->xchg.active && c->dm_prev_local && c->dx_cap_hint) {
            HIPCHK(c, c->dd_dx_chars.ensure(n_alloc * stride + 16)); HIPCHK(c, c->dd_dx_len.ensure(n_alloc));
            src = c->dd_dx_chars.p; src_len = c->dd_dx_len.p; bound = c->dx_cap_hint;
        } else if (c->xchg.active && c->xchg.gx_cap_hint && c->xchg.gx_cap_hint <= c->xchg.world * c->xchg.cap) {
            const uint64_t n_max = c->xchg.world * c->xchg.cap;
            HIPCHK(c, c->dm.gx_chars.ensure((size_t)n_max * stride + 16)); HIPCHK(c, c->dm.gx_len.ensure(n_max));
            src = c->dm.gx_chars.p; src_len = c->dm.gx_len.p; bound = c->xchg.gx_cap_hint;
        }
        if (src) {
            const int ps = device_merge_prepare(c, src, src_len, bound, c->d_count.p + 4);
            if (ps) return ps;
            init_merge = &c->dm.M;
        }
    }
    HIPCHK(c, c->stamp(8, 1));
    // lane-per-read kernel for uniform short reads; whatever it punts (err == 4) and every other
    // layout goes through the wave-per-read kernel
    static const bool no_hints_dbg = getenv("CRASS_SURV_NO_HINTS") != nullptr;      // (timing experiments only: the lanes walk every lattice seed)
    const uint32_t *hints = (c->hints_valid && !no_hints_dbg) ? c->d_hit_info.p : nullptr;
    const bool no_lanes = c->env.no_lane_kernel;
    hipError_t le = no_lanes ? hipErrorNotSupported
                             : launch_survivor_lanes(c->R, c->dp, c->d_idx.p, d_nsurv, n_surv, c->d_surv.p, c->d_dr.p, stride,
                                                     c->d_ss_pool.p, lds.ss_cap, c->d_found.p, hints, c->stream, init_merge, c->max_len, c->d_count.p + 6);
    if (le != hipSuccess && le != hipErrorNotSupported) { c->last_hip = (int)le; return CRASS_ERR_HIP; }
    if (le == hipSuccess && init_merge) { c->dm_prepared_n = init_merge->n_tok; c->dm_prepared_src = init_merge->dx_chars; }
    // Reads the lane kernel does not take (513 .. 2 048 bases): the long reads' LIGHT walk over the survivor list first — nearly every
    // survivor of such a set is a chance seed hit that ends without a candidate (a quarter of 1 000-base reads pass a 7-base window's
    // filter) — and the full wave kernel only for what it hands over, from the seed it stopped at.  Position hints of the default
    // lattice: k_long_light on them; another window or lattice: k_long_light_any, which works the bits out as it walks.
    bool light_done = false;
    if (le == hipErrorNotSupported && !no_lanes && c->dp.debug_stop == 0 && !c->env.no_dense_light && c->max_len <= 12288 && c->dp.window >= 6 && c->dp.window <= 9) {
        DevReads RL = c->R;
        const bool lattice = c->R.pos_hint && !c->R.hint_all && c->dp.skips == 8 && c->dp.window == 8;
        if (!lattice && !c->R.hint_all) RL.pos_hint = nullptr;
        HIPCHK(c, c->d_punt.ensure(n_surv + 1)); HIPCHK(c, hipMemsetAsync(c->d_punt.p, 0, 4, c->stream));
        const hipError_t ll = launch_long_light(RL, c->dp, d_nsurv, n_surv, c->d_surv.p, 0, c->max_len, c->stream, c->d_punt.p + 1, c->d_punt.p, c->d_idx.p);
        if (ll == hipSuccess) {
            light_done = true;
            HIPCHK(c, launch_survivor(c->R, c->dp, false, c->d_idx.p, d_nsurv, n_surv, c->d_surv.p, c->d_dr.p, stride,
                                      c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p, c->d_found.p, hints, lds,
                                      (int)std::min<uint64_t>(256 * 12, n_surv), c->stream, 7, 0, 0, c->d_punt.p + 1, c->d_punt.p));
        } else if (ll != hipErrorNotSupported) { c->last_hip = (int)ll; return CRASS_ERR_HIP; }
    }
    if (!light_done)
    HIPCHK(c, launch_survivor(c->R, c->dp, false, c->d_idx.p, d_nsurv, n_surv, c->d_surv.p, c->d_dr.p, stride,
                              c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p, c->d_found.p, hints, lds,
                              (int)std::min<uint64_t>(256 * 32, n_surv), c->stream, le == hipSuccess ? 4 : 0, 0, 0, nullptr,
                              le == hipSuccess ? c->d_count.p + 6 : nullptr));      // (the lane kernel's punt count: none -> the launch leaves at once)
    if (c->R.n_exc)                                     // exception reads in the list (err == 5): raw bytes, same slots
        HIPCHK(c, launch_survivor(c->R, c->dp, true, c->d_idx.p, d_nsurv, n_surv, c->d_surv.p, c->d_dr.p, stride,
                                  c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p, c->d_found.p, nullptr, lds,
                                  (int)std::min<uint64_t>(256 * 32, n_surv), c->stream, 5));
    HIPCHK(c, c->stamp(9, 1));
    const uint64_t n_words = (n_surv + 63) / 64;
    uint32_t tsize = 1024;
    if (dedupe) while (tsize < n_surv * 2) tsize <<= 1;
    // The table holds the DISTINCT strings.  Sized for the survivor slots (the only bound that cannot fail) it is 200 MB of
    // clearing per step at 100 M reads for 42 k strings; a speculative launch sizes it from the bound on the distinct
    // strings the merge is sized with, and an insert that runs out of probes reports the miss (h_count[5] bit 2): the host
    // de-duplicates that call itself and the context goes back to the full-size table.
    if (dedupe && speculative && c->dx_cap_hint && !c->dd_full_table && !c->env.dd_full_table) {
        uint32_t small = c->env.test_bounds[1] ? 64u : 4096u;          // (tests: a table that does overflow)
        while (small < c->dx_cap_hint * 4ull && small < tsize) small <<= 1;
        tsize = std::min(tsize, small);
    }
    Lookback lbf;
    if (const Lookback *lb = c->next_lookback_elems(n_surv, &lbf)) {
        // found flags -> ranks in one pass (also clears the de-duplication table)
        HIPCHK(c, launch_found_compact(c->d_surv.p, d_nsurv, n_surv, c->d_count.p + 3, dedupe ? c->dd_keys.p : nullptr,
                                       dedupe ? c->dd_first.p : nullptr, tsize, c->d_fidx.p, c->d_count.p + 2, *lb, c->stream));
    } else {
        HIPCHK(c, launch_found_mask(c->d_surv.p, d_nsurv, n_surv, c->d_mask.p, c->d_count.p + 3, c->stream,
                                    dedupe ? c->dd_keys.p : nullptr, dedupe ? c->dd_first.p : nullptr, tsize));
        HIPCHK(c, launch_compact(c->d_mask.p, n_words, n_surv, c->d_word_prefix.p, c->d_block_sums.p, c->d_fidx.p, n_surv, c->d_count.p + 2, c->stream));
    }
    // the gather assembles the hand-off blob and inserts every candidate's DR string into the de-duplication table
    HIPCHK(c, launch_gather_found(c->d_fidx.p, c->d_count.p + 2, n_surv, c->d_surv.p, c->d_idx.p, c->read_base, c->d_dr.p, stride,
                                  c->d_ss_pool.p, lds.ss_cap, ss_elem, D.d_blob.p, D.d_dr_len.p, D.d_dr.p, c->stream,
                                  dedupe ? c->dd_keys.p : nullptr, dedupe ? c->dd_first.p : nullptr, tsize, c->dd_hash.p, c->dd_slot.p,
                                  c->d_count.p + 5));
    // de-duplication and token ranks follow without a host round trip (the found count stays on the device);
    // their small outputs — all the merge needs — are written straight into pinned host memory
    c->have_rep = false;
    c->have_dev_tokens = false;
    if (dedupe) {
        // distinct strings in first-occurrence order and every candidate's rank among them, exact
        Lookback lbd;
        const bool dxd = c->dx_via_dma;                 // the list stays on the device; DMA engines bring it over (below)
        HIPCHK(c, launch_dx_tokens(D.d_dr.p, D.d_dr_len.p, c->dd_hash.p, stride, c->d_count.p + 2, (uint32_t)n_surv, c->dd_rep.p, c->dd_slot.p, c->dd_first.p, c->d_mask.p,
                                   c->d_word_prefix.p, c->d_block_sums.p, c->d_fidx.p, c->d_count.p + 4, c->d_count.p + 5, dxd ? c->dd_map.p : c->h_dmap.p,
                                   dxd ? nullptr : c->h_dx_chars.p, dxd ? nullptr : c->h_dx_len.p, dxd ? nullptr : c->h_dx_hash.p, c->dd_dx_chars.p, c->dd_dx_len.p, c->stream,
                                   c->d_count.p, defer_ok ? c->h_count.p + 16 : c->h_count.p, 8,           // (the counters leave with the last kernel: no copy call)
                                   c->next_lookback_tiles((n_surv + 1023) / 1024, &lbd)));
        if (c->xchg.active)                             // multi-rank: the list goes straight into the collective's send buffer
            HIPCHK(c, launch_xg_fill(c->dd_dx_chars.p, c->dd_dx_len.p, c->d_count.p + 4, stride, c->xchg.cap, c->xchg.slot, c->xchg.send.p, c->stream,
                                     defer_ok ? c->d_count.p : nullptr, n_surv,
                                     (defer_ok && c->poll_on) ? c->h_flags.p : nullptr, (defer_ok && c->poll_on) ? (c->want_p1 = ++c->flag_seq) : 0u));
    }
    if (!dedupe) HIPCHK(c, hipMemcpyAsync(c->h_count.p, c->d_count.p, 32, hipMemcpyDeviceToHost, c->stream));
    bool premerge_queued = false;
    c->premerge = 0;
    D.wide_ready = false; D.dr_fallback = false;
    D.pack_ss_cap = lds.ss_cap;
    // The merge itself is queued here too when the previous call's merge ran on the device: its kernels read the token
    // count from the device (d_count[4]) and are sized by a bound; crass_hip_merge adopts the result if the counts fit.
    const bool will_premerge = speculative && dedupe && !c->xchg.active && c->dm_prev_local && c->dx_cap_hint && c->prm.lowDRsize >= (int)kDevMinDR && stride <= 64 &&
                               !c->env.host_merge && !c->env.no_speculation;
    // (what the host waits for when the merge is queued behind pass 1, or pass 1 deferred: a stage flag — else this event)
    if (!c->poll_on && (will_premerge || defer_ok)) HIPCHK(c, hipEventRecord(c->ev_gathered, c->stream));
    if (will_premerge) {
        const bool prepared = c->dm_prepared_n == c->dx_cap_hint && c->dm_prepared_src == c->dd_dx_chars.p;
        const int ps = device_merge_enqueue(c, c->dd_dx_chars.p, c->dd_dx_len.p, c->dx_cap_hint, c->d_count.p + 4, prepared);
        if (ps) return ps;
        premerge_queued = true;
        // (only the fall-back order of the hand-off copy — no DMA engine — waits for this event)
        if (!c->poll_on || !c->dma) HIPCHK(c, hipEventRecord(c->ev_premerge, c->stream));
    }
    host_pool_warm();                                   // the merge follows: wake the host workers while the device finishes
    if (defer_ok) {
        c->p1d.active = true; c->p1d.n_bound = n_surv; c->p1d.ss_cap = lds.ss_cap; c->p1d.ss_elem = ss_elem;
        return CRASS_OK;
    }
    return dense_after_sync(c, n_surv, lds.ss_cap, ss_elem, dedupe, premerge_queued, overflow);
}

// every buffer pass 2's tail touches for up to h_alloc flagged reads (+ n_exc exception reads scanned byte-wise)
int ensure_recruit_buffers(crass_hip_ctx *c, uint64_t h_alloc, uint64_t n_exc, bool dev_sink, bool anchors)
{
    const uint64_t s_alloc = h_alloc + n_exc;
    { const int ms = ensure_mask_scratch(c, h_alloc); if (ms) return ms; }
    HIPCHK(c, c->d_rec.ensure(s_alloc + 1));
    HIPCHK(c, c->d_dr.ensure((s_alloc + 1) * c->dr_stride));
    if (!dev_sink) {                           // host sink only
        HIPCHK(c, c->h_rec.ensure(s_alloc + 1));
        HIPCHK(c, c->h_dr.ensure((s_alloc + 1) * c->dr_stride));
        HIPCHK(c, c->h_idx.ensure(h_alloc + 1));
    }
    if (anchors) {
        HIPCHK(c, c->d_slot_info.ensure(h_alloc + 1));
        HIPCHK(c, c->d_slot_pid.ensure(h_alloc + 1));
    }
    if (dev_sink) {
        HIPCHK(c, c->h_qblob.ensure(p2_blob_layout(h_alloc).total + 64));
        HIPCHK(c, c->d_fidx.ensure(h_alloc + 1));
    }
    return CRASS_OK;
}

// ------------------------------------------------------------------------------------------
// The first call of a context.  The three speculation bounds (survivors, distinct DR strings, flagged reads) are
// normally learnt from the previous call; a crass run scans each read set ONCE, so crass_hip_load_reads sets them from
// the read set itself — the expected pass rate of the seed filter on random sequence plus an allowance for real
// arrays — and sizes every pool for them.  The first seed scan / merge / recruit then neither allocates nor waits
// for a count before queueing the next stage; a bound that turns out too small repeats the stage with the exact
// count, exactly like a learnt one.  CRASS_NO_PRESIZE / CRASS_NO_SPECULATION switch this off.
// ------------------------------------------------------------------------------------------
static int first_call_bounds_impl(crass_hip_ctx *c)
{
    c->surv_cap_hint = 0; c->hit_cap_hint = 0; c->dx_cap_hint = 0; c->dm_prev_local = false; c->premerge = 0;
    c->recruit_exact = false;
    const uint64_t n = c->R.n_reads;
    if (c->env.no_presize || c->env.no_speculation || n == 0 || c->max_len > c->env.long_min) return CRASS_OK;
    if (c->R.n_exc && c->env.exc_separate) return CRASS_OK;
    const DevParams &P = c->dp;
    const SurvLds lds = survivor_lds_layout(c->max_len, P);
    if (lds.total_bytes > 160 * 1024 || lds.ss_cap > 128 || (c->dr_stride & 15)) return CRASS_OK;
    // seed filter on random sequence: every lattice seed has ~(highDR+highSp-lowDR-lowSp+1) candidate positions, each
    // an equal w-mer with probability 4^-w (libcrispr.cpp:295-339); + 2 % of the reads for real arrays; x 1.5
    const uint32_t min_len = P.lowDR + P.lowSp + P.window + 1;
    const double seeds = c->max_len > min_len ? (double)(c->max_len - min_len) / P.skips + 1.0 : 1.0;
    const double cand = (double)(P.highDR + P.highSp - P.lowDR - P.lowSp + 1);
    double rate = seeds * cand / (double)(1ull << (2 * P.window)) + 0.02;
    if (rate > 1.0) rate = 1.0;
    uint64_t surv = survivor_bound((uint64_t)((double)n * rate));
    if (surv > n + 65536) surv = survivor_bound(n * 2 / 3);       // (1.5 x inside: the bound never needs to exceed n)
    if (c->env.test_bounds[0]) surv = std::max<uint64_t>(64, c->env.test_bounds[0]);
    const uint64_t pool_cap = std::max<uint64_t>(surv * (uint64_t)lds.ss_cap, 1u << 16);
    if (surv > kDenseMaxSurvivors || pool_cap >= (1ull << 31)) return CRASS_OK;
    // keep the pools a small part of the device: ~(20 + 2*stride + 4*ss_cap + 100) bytes per survivor slot
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return CRASS_OK;
    const uint64_t per = 140ull + 3ull * c->dr_stride + 6ull * lds.ss_cap;
    if (surv * per > free_b / 4) return CRASS_OK;
    const bool dedupe = surv < (1u << 24);
    int s = ensure_dense_buffers(c, surv, pool_cap, lds, dedupe);
    if (s) return s;
    c->surv_cap_hint = surv;
    // look-back status words for the largest launch of a step (the masks over all reads), cleared once
    { const uint64_t nw = (n + 63) / 64; c->prealloc_lookback(std::max<uint64_t>((nw + lookback_tile_words(nw) - 1) / lookback_tile_words(nw), (surv + 1023) / 1024)); }
    // distinct DR strings: a few hundred per million reads on metagenome-like input; the device merge is queued
    // behind pass 1 for this many
    if (dedupe && c->prm.lowDRsize >= (int)kDevMinDR && c->dr_stride <= 64 && !c->env.host_merge) {
        uint64_t dx = crass_hip_exchange_rows_for(n);
        if (c->env.test_bounds[1]) dx = std::max<uint64_t>(16, c->env.test_bounds[1]);
        s = device_merge_prepare(c, c->dd_dx_chars.p, c->dd_dx_len.p, dx, c->d_count.p + 4);
        if (s) return s;
        c->dx_cap_hint = (uint32_t)dx;
        c->dm_prev_local = true;
        // the host view of that merge (token arena, per-candidate tokens, pattern list, flat groups) is built by the helper thread
        // while pass 2 runs; on a context's first call its containers grew and faulted their pages in there — 2.2 ms instead of
        // 1.1 at 100 M reads, 0.5 ms of it past the end of pass 2.  They are grown and touched here, with the reads
        // (MergeResult::clear keeps the capacity).
        try {
            auto touch = [](auto &v, size_t k) { v.resize(k); v.clear(); };
            MergeResult &m = c->merge;
            touch(m.cand_token, (size_t)(n / 128 + 4096));
            touch(m.tokens.strings.chars, (size_t)dx * 48); touch(m.tokens.strings.off, (size_t)dx + 2); m.tokens.strings.clear();
            touch(m.patterns.chars, (size_t)dx * 24); touch(m.patterns.off, (size_t)dx + 2); m.patterns.clear();
            touch(m.pat_group, (size_t)dx); touch(m.pat_token, (size_t)dx); touch(m.grp_tokens, (size_t)dx); touch(m.grp_off, (size_t)dx / 4 + 16);
        } catch (const std::bad_alloc &) { }
    }
    // reads flagged by the anchor probe: reads of arrays that pass 1 did not find (+ ~0 false positives)
    uint64_t hits = hit_bound(n / 64);
    if (c->env.test_bounds[2]) hits = std::max<uint64_t>(16, c->env.test_bounds[2]);
    s = ensure_recruit_buffers(c, hits, 0, true, true);
    if (s) return s;
    c->hit_cap_hint = hits;
    // The wave-per-read survivor kernel spills a few registers, i.e. needs scratch memory: the runtime sets a queue's scratch up
    // at the first dispatch that asks for it — the device sat idle for ~160 us in front of that launch and the launch itself
    // took 130 us instead of 20 (a fresh context's step at 100 M reads: 4.77-4.87 ms against 4.45-4.55 for its later steps,
    // profiles/r06_single_shot_timeline.txt).  An empty launch of the same shape here, with the reads, takes that off the step.
    if (!c->env.no_warm_launch) {
        HIPCHK(c, hipMemsetAsync(c->d_count.p, 0, 32, c->stream));
        HIPCHK(c, launch_survivor(c->R, c->dp, false, c->d_idx.p, c->d_count.p + 1, surv, c->d_surv.p, c->d_dr.p, c->dr_stride,
                                  c->d_ss_pool.p, (uint32_t)pool_cap, c->d_ss_used.p, c->d_found.p, nullptr, lds,
                                  (int)std::min<uint64_t>(256 * 32, surv), c->stream, 4));
    }
    host_pool_warm();
    return CRASS_OK;
}

// best effort: a pool that cannot be sized now (out of memory, a cap) just means the first call sizes things itself, as
// every call did before — the load itself has succeeded
int first_call_bounds(crass_hip_ctx *c)
{
    const int s = first_call_bounds_impl(c);
    if (s == CRASS_ERR_OOM) {
        c->surv_cap_hint = 0; c->hit_cap_hint = 0; c->dx_cap_hint = 0; c->dm_prev_local = false; c->premerge = 0;
        c->last_hip = 0;
        c->dm.release();                                // (the merge tables sized for the bound: the first call sizes them exactly)
        c->dm_prepared_n = 0; c->dm_prepared_src = nullptr;
        return CRASS_OK;
    }
    return s;
}

// the seed scan's filter: which kernel filled the mask (fast: the lane filter, whose seed hints the survivor kernels use;
// hint_filtered: the position hints stood in for it), and whether it cleared the found flags on its way
struct FilterRoute { bool fast = false, hint_filtered = false, found_cleared = false; };

// step 1 for reads up to env.long_min bases: one of four kernels sets a read's mask bit when it holds a lattice seed hit
static int launch_filter(crass_hip_ctx *c, uint64_t n_words, FilterRoute &fr)
{
    hipError_t fe = hipErrorNotSupported;
    // (uniform STRIDE is what the bit-parallel kernel needs; the lengths may differ — trimmed reads padded to one stride)
    static const bool found_memset = getenv("CRASS_FOUND_MEMSET") != nullptr;      // A/B switch: the fill kernel in front of the scan
    if (c->R.stride_words >= 4 && c->R.stride_words <= 16)
        fe = launch_filter_fast(c->R, c->dp, c->d_mask.p, c->d_hit_info.p, c->stream, found_memset ? nullptr : c->d_found.p, &fr.found_cleared);
    if (fe != hipSuccess) fr.found_cleared = false;
    const bool lattice_hints = c->hint_filter && c->R.pos_hint && !c->hint_filter_any;
    if (fe == hipSuccess) fr.fast = true;
    else if (fe == hipErrorNotSupported && (lattice_hints || (c->hint_filter_any && c->n_pos_hint_words))) {
        // no lane-per-read filter for this layout: one hint bit per lattice position (the long reads' kernel), which also flags the reads that have one —
        // the survivor kernel walks on the same bits —, or under another window or lattice the every-position form of the bits
        HIPCHK(c, hipMemsetAsync(c->d_mask.p, 0, n_words * 8, c->stream));
        const uint32_t *blk = c->pos_hint_blk ? c->d_pos_hint_blk.p : nullptr;
        const hipError_t he = lattice_hints ? launch_hint_positions(c->R, c->dp, c->d_pos_hint_off.p, blk, c->n_pos_hint_words, c->d_pos_hint.p, c->stream, 0, c->n_pos_hint_words, c->d_mask.p)
                                            : launch_hint_filter_any(c->R, c->dp, c->d_pos_hint_off.p, blk, c->n_pos_hint_words, c->d_mask.p, c->d_pos_hint.p, c->stream);
        c->hint_pending = false;
        if (he != hipSuccess) { c->last_hip = (int)he; return CRASS_ERR_HIP; }
        fr.hint_filtered = true;
    }
    else if (fe == hipErrorNotSupported) { HIPCHK(c, launch_filter_general(c->R, c->dp, c->d_mask.p, c->max_len, c->stream)); }
    else { c->last_hip = (int)fe; return CRASS_ERR_HIP; }
    return CRASS_OK;
}

// step 1 for longer reads: they almost surely contain a spurious lattice hit (P ~ seeds*49/4^w), so nothing filters — all
// non-exception reads survive: mask = ~exc_mask (exc_mask is 32-bit words of the same bit order) — and the position hints the
// survivor kernel walks on are computed, slice by slice
static int launch_unfiltered(crass_hip_ctx *c, uint64_t n_words)
{
    HIPCHK(c, hipMemsetAsync(c->d_mask.p, 0xFF, n_words * 8, c->stream));
    if (!c->R.pos_hint) return CRASS_OK;
    const uint32_t *blk = c->pos_hint_blk ? c->d_pos_hint_blk.p : nullptr;
    if (c->hint_parts > 1) { HIPCHK(c, hipEventRecord(c->ev_hint_go, c->stream)); HIPCHK(c, hipStreamWaitEvent(c->hint_stream, c->ev_hint_go, 0)); }
    for (int q = 0; q < c->hint_parts; q++) {
        hipStream_t hs = q == 0 ? c->stream : c->hint_stream;
        hipError_t he = launch_hint_positions(c->R, c->dp, c->d_pos_hint_off.p, blk, c->n_pos_hint_words, c->d_pos_hint.p, hs,
                                              c->hint_word_split[q], c->hint_word_split[q + 1]);
        if (he != hipSuccess) { c->last_hip = (int)he; return CRASS_ERR_HIP; }
        if (q > 0) HIPCHK(c, hipEventRecord(c->ev_hint[q], c->hint_stream));
    }
    c->hint_pending = c->hint_parts > 1;
    return CRASS_OK;
}

// the compaction's count, d_count[0], in h_count[0]: a host round trip
int read_count(crass_hip_ctx *c)
{
    HIPCHK(c, hipMemcpyAsync(c->h_count.p, c->d_count.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRASS_OK;
}

// host-loop path: a host copy of the n_surv survivors' read indices, which the sink labels its records with
static int host_survivor_list(crass_hip_ctx *c, bool use_filter, uint64_t &n_surv, std::vector<uint64_t> &surv_idx)
{
    surv_idx.resize(n_surv);
    if (n_surv && use_filter) {
        HIPCHK(c, c->h_idx.ensure(n_surv));
        HIPCHK(c, hipMemcpyAsync(c->h_idx.p, c->d_idx.p, n_surv * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        memcpy(surv_idx.data(), c->h_idx.p, n_surv * 8);
    } else if (n_surv) {
        // no filter: every non-exception read survives, in order
        const uint64_t n = c->R.n_reads;
        size_t e = 0, w = 0;
        for (uint64_t r = 0; r < n; r++) {
            while (e < c->h_exc_read.size() && c->h_exc_read[e] < r) e++;
            if (e < c->h_exc_read.size() && c->h_exc_read[e] == r) continue;
            surv_idx[w++] = r;
        }
        surv_idx.resize(w);
        n_surv = w;
        if (n_surv) HIPCHK(c, hipMemcpyAsync(c->d_idx.p, surv_idx.data(), n_surv * 8, hipMemcpyHostToDevice, c->stream));
    }
    return CRASS_OK;
}

// two lists, each ascending by read index, as one (exception reads are rare)
static crass_hip_ctx::P1List merge_p1_lists(const crass_hip_ctx::P1List &a, const crass_hip_ctx::P1List &el, uint32_t stride)
{
    crass_hip_ctx::P1List m;
    m.reserve(a.size() + el.size(), stride);
    size_t ia = 0, ib = 0;
    while (ia < a.size() || ib < el.size()) {
        const bool takeA = ib >= el.size() || (ia < a.size() && a.read[ia] < el.read[ib]);
        const crass_hip_ctx::P1List &src = takeA ? a : el;
        const size_t k = takeA ? ia++ : ib++;
        m.read.push_back(src.read[k]); m.low.push_back(src.low[k]); m.replen.push_back(src.replen[k]);
        m.nss.push_back(src.nss[k]); m.ss_off.push_back(m.ss.size());
        m.ss.insert(m.ss.end(), src.ss.begin() + src.ss_off[k], src.ss.begin() + src.ss_off[k] + src.nss[k]);
        m.dr_len.push_back(src.dr_len[k]);
        m.dr.insert(m.dr.end(), src.dr.begin() + k * stride, src.dr.begin() + (k + 1) * stride);
    }
    return m;
}

// no device-resident distinct list (exception reads, no candidates, ...): the exchange's send buffer is filled from the host's
static int fill_send_from_host(crass_hip_ctx *c)
{
    ensure_distinct(c);
    const uint64_t nd = c->dx_len.size();
    std::vector<uint8_t> buf(c->xchg.send_bytes(), 0);
    reinterpret_cast<uint64_t *>(buf.data())[0] = nd;
    reinterpret_cast<uint32_t *>(buf.data())[2] = c->dr_stride;
    reinterpret_cast<uint32_t *>(buf.data())[3] = (uint32_t)c->xchg.cap;
    for (uint64_t j = 0; j < nd && j < c->xchg.cap; j++) {
        uint8_t *row = buf.data() + (j + 1) * (size_t)c->xchg.slot;
        memcpy(row, c->dx_chars.data() + j * (size_t)c->dr_stride, c->dr_stride);
        const uint32_t l = c->dx_len[j];
        memcpy(row + c->dr_stride, &l, 4);
    }
    HIPCHK(c, hipMemcpy(c->xchg.send.p, buf.data(), buf.size(), hipMemcpyHostToDevice));
    return CRASS_OK;
}

// what a finished pass 1 reports (the event spans are evaluated when the counters are fetched: each query costs
// microseconds of host time between two stages)
static void publish_p1_counters(crass_hip_ctx *c, uint64_t n_surv, bool fast, bool hint_filtered, float ms_sink_host)
{
    c->cnt.ms_sink_host = ms_sink_host;
    c->cnt.n_filter_survivors = n_surv + (c->dp.exc_survive ? 0 : c->R.n_exc);
    c->cnt.n_pass1_found = c->n_cand();
    c->cnt.used_fast_filter = fast ? 1 : (hint_filtered ? 2 : 0);
    c->spans_p1 = true; c->span_survivors = n_surv != 0;
}

int crass_hip_seed_scan(crass_hip_ctx *c)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    if (!c->have_reads) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    (void)c->wait_bulk();               // (copies of the previous step: their records are dropped below)
    (void)c->wait_dx();                 // (... and the distinct list's: the engines read buffers this scan rewrites)
    c->bulk_status = CRASS_OK; c->dx_status = CRASS_OK;
    quiesce_worker(c);
    c->have_pass1 = c->have_merge = c->have_pass2 = false;
    c->dm.active = false;
    c->premerge_inflight = false;
    c->p1d.active = false;                  // (a deferred pass 1 nobody finished: its kernels are ahead of this scan's on the stream, its results dropped)
    const bool defer_p1 = c->p1d.enabled && !c->p1d.force_sync && c->xchg.active;
    c->p1d.force_sync = false;
    // (the survivor kernel clears the merge's words, x_* included: behind whatever export of a merge nobody adopted)
    if (c->dm.view_launched) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->dm.ev_view, 0)); c->dm.view_launched = false; }
    const uint64_t n = c->R.n_reads;
    const uint64_t n_words = (n + 63) / 64;
    HIPCHK(c, c->stamp(0, 1));
    // step 1: filter, or for reads longer than 2 kbp none: every read goes to the survivor kernel
    FilterRoute fr;
    const bool use_filter = c->max_len <= c->env.long_min;
    // exception reads (a byte outside ACGT) join the survivor list and are evaluated byte-wise in place, so that
    // the dense pass-1 path also holds for inputs with a few N reads
    c->dp.exc_survive = (use_filter && c->R.n_exc > 0 && !c->env.exc_separate) ? 1u : 0u;
    if (const int fs = use_filter ? launch_filter(c, n_words, fr) : launch_unfiltered(c, n_words)) return fs;
    c->hints_valid = fr.fast;
    if (!fr.found_cleared) HIPCHK(c, hipMemsetAsync(c->d_found.p, 0, n + 1, c->stream));      // (in front of the survivor kernels, which set them)
    HIPCHK(c, c->stamp(1, 1));
    // step 2: ordered compaction
    // (the scan kernel also clears the survivor stage's counters: d_count[2..6) and the start/stop pool cursor)
    Lookback lbs;
    HIPCHK(c, launch_compact(c->d_mask.p, n_words, n, c->d_word_prefix.p, c->d_block_sums.p, c->d_idx.p, n, c->d_count.p, c->stream,
                             c->d_count.p + 2, 5, c->d_ss_used.p, 1, c->next_lookback(n_words, &lbs)));      // ([2..6) + [6], the lane kernel's punt count)
    HIPCHK(c, c->stamp(2, 2));
    c->dense.active = false; c->have_rep = false; c->have_distinct = false;
    c->have_dev_tokens = false; c->hl_tokens = false;
    c->cand_fill = nullptr; c->cand_pending_n = 0;      // (a fill nobody asked for: its records are dropped)
    c->cand.clear();
    const double t_sink0 = now_ms();
    uint64_t n_surv = 0;
    int s = CRASS_ERR_STATE;
    // Speculative fast path: the survivor stage is launched right behind the compaction with the survivor
    // count still on the device, sized by a bound learnt from the previous call (1.5 x its count).  If the
    // bound turns out too small the stage is simply redone below with the exact count.
    const bool exc_ok = c->R.n_exc == 0 || c->dp.exc_survive;
    if (use_filter && exc_ok && c->surv_cap_hint && !c->env.no_speculation) {
        bool overflow = false;
        HIPCHK(c, c->stamp(3, 2));
        s = run_survivors_dense(c, c->surv_cap_hint, c->d_count.p, &overflow, defer_p1);
        if (s != CRASS_OK && s != CRASS_ERR_STATE) return s;
        if (s == CRASS_OK && c->p1d.active) {
            // queued up to the send buffer's fill kernel, not waited for: p1_finish does the rest when the caller has queued the
            // exchange and crass_hip_merge_gathered its kernels (or when anybody asks for pass 1's results)
            c->p1d.fast = fr.fast; c->p1d.hint_filtered = fr.hint_filtered;
            HIPCHK(c, c->stamp(4, 2));
            return CRASS_OK;
        }
        if (s == CRASS_OK) {
            n_surv = c->h_count.p[0];
            if (overflow) c->n_bound_overflows[0]++;
            if (overflow || n_surv == 0) {              // redo below with the exact count; undo the attempt's found flags
                c->dense.active = false;
                s = CRASS_ERR_STATE;
                HIPCHK(c, hipMemsetAsync(c->d_found.p, 0, n + 1, c->stream));
            }
        } else {                                        // nothing was launched (layout limits): plain path
            if (const int rs = read_count(c)) return rs;
            n_surv = c->h_count.p[0];
        }
    } else if (!use_filter && c->R.n_exc == 0) {
        // nothing filters and no read is an exception: every read survives and the compaction's list is 0, 1, 2, ... —
        // the survivor kernel is queued right behind it, no host round trip (0.7 ms of an idle device at 1 M x 10 kbp:
        // the wait, a host-built copy of the list and its 8 MB upload)
        n_surv = n;
    } else {
        if (const int rs = read_count(c)) return rs;
        n_surv = c->h_count.p[0];
    }
    const bool spec_done = (s == CRASS_OK);
    const bool try_dense = !spec_done && use_filter && exc_ok && n_surv > 0 && n_surv <= kDenseMaxSurvivors;
    if (!spec_done) {
        // the survivor kernel reads its count from d_count[1] (chunk-local bound is passed separately)
        c->h_count.p[1] = 0xFFFFFFFFu;
        HIPCHK(c, hipMemcpyAsync(c->d_count.p + 1, c->h_count.p + 1, 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, c->stamp(3, 2));
        bool overflow = false;
        s = try_dense ? run_survivors_dense(c, n_surv, c->d_count.p + 1, &overflow) : CRASS_ERR_STATE;
        if (s != CRASS_OK && s != CRASS_ERR_STATE) return s;
    }
    if (use_filter && exc_ok) c->surv_cap_hint = survivor_bound(n_surv);       // bound for the next call: 1.5 x this call's count
    if (s == CRASS_ERR_STATE) {
        // host-loop path: label records with their read index from a host copy of the survivor list
        const bool identity = !use_filter && c->R.n_exc == 0;      // (see above: the list on the device is 0, 1, 2, ...)
        std::vector<uint64_t> surv_idx;
        if (!identity) { const int ls = host_survivor_list(c, use_filter, n_surv, surv_idx); if (ls) return ls; }
        s = run_survivors(c, false, n_surv, c->cand, identity ? nullptr : surv_idx.data());
        if (s) return s;
    }
    if (c->R.n_exc && !c->dense.active) {               // (the dense path evaluated them in place)
        crass_hip_ctx::P1List el;
        s = run_survivors(c, true, c->R.n_exc, el, nullptr);
        if (s) return s;
        if (el.size()) c->cand = merge_p1_lists(c->cand, el, c->dr_stride);
    }
    HIPCHK(c, c->stamp(4, 2));
    if (!(c->premerge_inflight && (c->dense.active || c->hl_tokens))) HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_pass1 = true;
    if (c->xchg.active && !(c->dense.active && c->have_dev_tokens)) { const int xs = fill_send_from_host(c); if (xs) return xs; }
    publish_p1_counters(c, n_surv, fr.fast, fr.hint_filtered, (float)(now_ms() - t_sink0));     // (ms_sink_host includes the survivor kernel + D2H it waits for)
    return c->lookback_ok();
}

// The host's half of a deferred pass 1 (p1d).  CRASS_OK: the context is where a synchronous crass_hip_seed_scan leaves it.
// kP1Redo (engine_ctx.h): the speculative launch cannot be used.
int p1_finish(crass_hip_ctx *c)
{
    if (!c->p1d.active) return CRASS_OK;
    c->p1d.active = false;
    c->p1d.finishing = true;
    bool overflow = false;
    const int s = dense_after_sync(c, c->p1d.n_bound, c->p1d.ss_cap, c->p1d.ss_elem, true, false, &overflow);
    const uint64_t n_surv = c->h_count.p[16];
    c->p1d.finishing = false;
    if (s != CRASS_OK) { c->p1d.force_sync = true; (void)hipStreamSynchronize(c->stream); return s; }
    if (overflow) c->n_bound_overflows[0]++;
    c->surv_cap_hint = survivor_bound(n_surv);
    const bool usable = !overflow && n_surv != 0 && c->dense.active && (c->dense.n == 0 || c->have_dev_tokens);
    if (!usable) {
        c->dense.active = false; c->have_dev_tokens = false;
        c->p1d.force_sync = true;
        HIPCHK(c, hipStreamSynchronize(c->stream));       // (whatever was queued behind the launch worked on nothing usable)
        return kP1Redo;
    }
    c->have_pass1 = true;
    publish_p1_counters(c, n_surv, c->p1d.fast, c->p1d.hint_filtered, 0.f);
    return c->lookback_ok();
}

// every entry point that reads pass 1's results, other than crass_hip_merge_gathered: a launch that cannot be used is repeated
// here, synchronously (the send buffer is refilled; a caller that had already gathered it sees the redo mark in what it gathered)
int settle_p1(crass_hip_ctx *c)
{
    if (!c->p1d.active) return CRASS_OK;
    const int s = p1_finish(c);
    if (s == kP1Redo) return crass_hip_seed_scan(c);
    return s;
}

int crass_hip_exchange_set_deferred(crass_hip_ctx *c, int on)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    if (!on) { const int s = settle_p1(c); if (s) return s; }
    c->p1d.enabled = on != 0 && !c->env.no_speculation && getenv("CRASS_NO_DEFER_P1") == nullptr;
    return CRASS_OK;
}

} // extern "C"

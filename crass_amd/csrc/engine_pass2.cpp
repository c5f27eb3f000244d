// engine_pass2.cpp — pass 2 of the context behind include/crass_hip.h: crass_hip_set_patterns, crass_hip_recruit (mark extra
// found, probe or automaton, compact, size, verify / finish, then the device sink or the host sink) and crass_hip_get_recruits.
// The pattern set's install is engine.cpp's (install_patterns), the fall-back to the host merge engine_merge.cpp's.
#include "engine_ctx.h"

#include <cstdio>

extern "C" {

int crass_hip_set_patterns(crass_hip_ctx *c, const char *const *patterns, const uint32_t *lengths, uint32_t n)
{
    if (!c || (n && (!patterns || !lengths))) return CRASS_ERR_INVALID_ARG;
    StringArena pats;
    for (uint32_t i = 0; i < n; i++) pats.push(patterns[i], lengths[i]);
    c->have_pass2 = false;
    return install_patterns(c, pats);
}

// ------------------------------------------------------------------------------------------
// pass 2
// ------------------------------------------------------------------------------------------
// the device merge gave up (or its results do not add up): host merge, then pass 2 again
// (the two lists of found reads a recruit call was given, the host's and the device's: every repeat carries both along)
struct ExtraFound { const uint64_t *host; uint64_t n_host; const uint64_t *dev; uint64_t n_dev; };
static int recruit_impl(crass_hip_ctx *c, const ExtraFound &x);

static int recruit_after_host_merge(crass_hip_ctx *c, const ExtraFound &x)
{
    if (const int fs = host_merge_fallback(c)) return fs;
    return recruit_impl(c, x);
}

// additional found headers (local read indices, e.g. every header another input file found): one upload, one kernel
static int mark_extra_found(crass_hip_ctx *c, const uint64_t *extra_found, uint64_t n_extra)
{
    for (uint64_t i = 0; i < n_extra; i++) if (extra_found[i] >= c->R.n_reads) return CRASS_ERR_INVALID_ARG;
    HIPCHK(c, c->d_extra.ensure(n_extra));
    HIPCHK(c, hipMemcpyAsync(c->d_extra.p, extra_found, n_extra * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_mark_found(c->d_extra.p, n_extra, c->R.header_id, c->d_found.p, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));        // (the caller's array may go away)
    return CRASS_OK;
}

// the same for a list that lies in device memory and may hold CRASS_NAME_NOT_FOUND (the answers of
// crass_hip_fastx_names_find_device as they are): nothing is uploaded.  Two launches of k_mark_found_skip: the first only
// checks, so that a list with an entry out of range marks nothing; the host reads the one word between them
static int mark_extra_found_device(crass_hip_ctx *c, const uint64_t *d_extra_found, uint64_t n_d_extra)
{
    HIPCHK(c, c->d_extra_bad.ensure(1)); HIPCHK(c, c->h_extra_bad.ensure(1));
    HIPCHK(c, hipMemsetAsync(c->d_extra_bad.p, 0, 4, c->stream));
    HIPCHK(c, launch_mark_found_skip(d_extra_found, n_d_extra, c->R.n_reads, c->R.header_id, nullptr, c->d_extra_bad.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_extra_bad.p, c->d_extra_bad.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (*c->h_extra_bad.p) return CRASS_ERR_INVALID_ARG;
    HIPCHK(c, launch_mark_found_skip(d_extra_found, n_d_extra, c->R.n_reads, c->R.header_id, c->d_found.p, c->d_extra_bad.p, c->stream));
    return CRASS_OK;
}

// which reads may hold a pattern, as mask bits.  Fast path: the anchor filter (an exact superset; anchors = true), the flagged
// reads alone are scanned exactly later; otherwise the automaton scans every read (lds: its table fitted the LDS).  The n_exc
// exception reads of a host-built pattern set are scanned byte-wise on the side.
static int launch_probe(crass_hip_ctx *c, bool dmp, uint64_t n_exc, bool &anchors, bool &lds)
{
    anchors = lds = false;
    if (dmp) {
        HIPCHK(c, launch_anchor_filter_dev(c->R, c->dm.M, c->d_found.p, c->d_mask.p, c->stream, c->env.probe_blocks));
        anchors = true;
    } else if (c->have_anchors) {
        hipError_t ae = launch_anchor_filter(c->R, c->K, c->d_found.p, c->d_mask.p, c->stream, c->env.probe_blocks);
        if (ae == hipSuccess) anchors = true;
        else if (ae != hipErrorNotSupported) { c->last_hip = (int)ae; return CRASS_ERR_HIP; }
    }
    if (!anchors || n_exc) { int fs = ensure_full_automaton(c); if (fs) return fs; }
    if (!anchors) {
        hipError_t re = launch_recruit_lds(c->R, c->A, c->d_found.p, c->d_mask.p, c->d_hit_info.p, c->stream);
        lds = (re == hipSuccess);
        if (re == hipErrorNotSupported) { HIPCHK(c, launch_recruit_general(c->R, c->A, c->d_found.p, c->d_mask.p, c->d_hit_info.p, c->stream)); }
        else if (re != hipSuccess) { c->last_hip = (int)re; return CRASS_ERR_HIP; }
    }
    if (n_exc) {
        HIPCHK(c, c->d_exc_hit.ensure(n_exc));
        HIPCHK(c, launch_recruit_exceptions(c->R, c->A, c->d_found.p, c->d_exc_hit.p, c->stream));
    }
    return CRASS_OK;
}

// device merge path: the sink runs on the device too (drop the slots without a match, pack the records in
// read order) and ONE copy brings the hand-off arrays to pinned host memory
static int recruit_device_sink(crass_hip_ctx *c, bool spec, uint64_t n_hits, const ExtraFound &x)
{
    static const bool blob12 = getenv("CRASS_P2_BLOB12") != nullptr;      // A/B switch: the 12-byte form of round 3
    // (the 9-byte form needs the token strings when the records are widened: a context whose host view is the light one —
    // the ranks of a group other than the first — keeps the 12-byte form)
    const uint32_t narrow = (c->max_len <= 255 && c->R.n_reads < (1ull << 32)) ? ((blob12 || c->host_view_light) ? 1u : 2u) : 0u;
    c->q_lay = p2_blob_layout(n_hits, narrow);
    c->q_wide_ready = false;
    Lookback lbq;
    if (n_hits) {
        HIPCHK(c, launch_pack_p2_blob(c->d_rec.p, c->d_idx.p, c->read_base, c->d_count.p, n_hits, c->d_mask.p,
                                      c->d_word_prefix.p, c->d_block_sums.p, c->d_fidx.p, c->d_count.p + 6, c->h_qblob.p, c->stream,
                                      spec ? c->h_count.p : nullptr, c->next_lookback_elems(n_hits, &lbq), narrow));
    } else memset(c->h_qblob.p, 0, 16);
    const double th0 = now_ms();
    const int hs = ensure_host_merge(c);            // host view of the merge, rebuilt while the device verifies
    c->cnt.ms_merge_host += (float)(now_ms() - th0);
    if (c->env.merge_profile)
        fprintf(stderr, "[crass_dm] recruit: tail queued %.1f us after the pass-1 sync, then blocked %.1f us on the host view\n",
                1e3 * (th0 - c->t_p1_sync), 1e3 * (now_ms() - th0));
    if (hs == CRASS_ERR_STATE) {                    // inconsistent device results: never expected
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return recruit_after_host_merge(c, x);
    }
    if (hs) return hs;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->env.merge_profile)
        fprintf(stderr, "[crass_dm] recruit: final synchronisation returned %.1f us after the pass-1 sync\n", 1e3 * (now_ms() - c->t_p1_sync));
    if (spec) {
        if (c->dm.h_st.p->fail) return recruit_after_host_merge(c, x);
        if (c->h_count.p[0] > n_hits) {             // bound too small: repeat with the exact count
            c->n_bound_overflows[2]++;
            c->hit_cap_hint = 0;
            c->recruit_exact = true;
            return recruit_impl(c, x);
        }
    }
    c->hit_cap_hint = hit_bound(c->h_count.p[0]);
    // (the probe's selectivity — 12-base keys flag some per cent of the reads, 16-base keys 0.4 % —: CRASS_MERGE_PROFILE=1)
    if (c->env.merge_profile)
        fprintf(stderr, "[crass_dm] recruit: anchor probe flagged %u of %llu reads (%u keys of %u bases, windows every %u)\n", c->h_count.p[0],
                (unsigned long long)c->R.n_reads, c->dm.h_st.p->n_keys, c->dm.M.akey_bases, 1u << c->dm.M.akey_shift);
    if (const int bs = c->wait_bulk()) return bs;   // the step ends with the pass-1 hand-off records in host memory too
    c->q_n = *reinterpret_cast<const uint64_t *>(c->h_qblob.p);
    c->q_blob_active = true;
    c->have_pass2 = true;
    c->cnt.n_pass2_found = c->q_n;
    c->cnt.used_lds_automaton = 2;
    c->cnt.anchor_keys = c->dm.h_st.p->n_keys;
    c->cnt.anchor_table_kind = c->dm.h_st.p->tab_mode == 3 ? 1 : c->dm.h_st.p->tab_mode;
    c->spans_p2 = true;
    return c->lookback_ok();
}

// host-built pattern set: the records come back slot by slot; packed hits and exception hits are merged by read index here,
// token = existing or new (addReadHolder)
static int recruit_host_sink(crass_hip_ctx *c, uint64_t n_hits, uint64_t n_exc, bool anchors, bool lds)
{
    const uint64_t n_slots = n_hits + n_exc;
    if (n_slots) {
        HIPCHK(c, hipMemcpyAsync(c->h_rec.p, c->d_rec.p, n_slots * sizeof(RecruitOut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_dr.p, c->d_dr.p, n_slots * c->dr_stride, hipMemcpyDeviceToHost, c->stream));
    }
    if (n_hits) HIPCHK(c, hipMemcpyAsync(c->h_idx.p, c->d_idx.p, n_hits * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t0 = now_ms();
    size_t ia = 0, ib = 0;
    const size_t nb = n_exc;
    auto exc_valid = [&](size_t b) { return c->h_rec.p[n_hits + b].dr_len != 0; };
    while (ib < nb && !exc_valid(ib)) ib++;
    auto hit_valid = [&](size_t a) { return c->h_rec.p[a].dr_len != 0; };
    while (ia < n_hits && !hit_valid(ia)) ia++;                  // anchor false positives carry no match
    c->q_dr.reserve(n_slots * c->dr_stride);
    c->q_read.reserve(n_slots); c->q_low.reserve(n_slots); c->q_start.reserve(n_slots); c->q_end.reserve(n_slots);
    c->q_dr_len.reserve(n_slots); c->q_token.reserve(n_slots);
    while (ia < n_hits || ib < nb) {
        const bool takeA = ib >= nb || (ia < n_hits && c->h_idx.p[ia] < c->h_exc_read[ib]);
        const size_t slot = takeA ? ia : n_hits + ib;
        const RecruitOut &o = c->h_rec.p[slot];
        const uint64_t r = takeA ? c->h_idx.p[ia] : c->h_exc_read[ib];
        c->q_read.push_back(c->read_base + r); c->q_low.push_back(o.low_lexi);
        c->q_start.push_back(o.start); c->q_end.push_back(o.end); c->q_dr_len.push_back(o.dr_len);
        const char *dr = c->h_dr.p + slot * c->dr_stride;
        const size_t at = c->q_dr.size();
        c->q_dr.resize(at + c->dr_stride);
        memset(c->q_dr.data() + at, 0, c->dr_stride);
        memcpy(c->q_dr.data() + at, dr, o.dr_len);
        uint32_t tok = o.token;
        if (!tok && c->have_merge) {
            tok = c->merge.tokens.get(dr, o.dr_len);
            if (!tok) tok = c->merge.tokens.add(dr, o.dr_len);
        }
        c->q_token.push_back(tok);
        if (takeA) { ia++; while (ia < n_hits && !hit_valid(ia)) ia++; }
        else { ib++; while (ib < nb && !exc_valid(ib)) ib++; }
    }
    c->have_pass2 = true;
    c->cnt.ms_sink_host += (float)(now_ms() - t0);
    c->cnt.n_pass2_found = c->q_read.size();
    c->cnt.used_lds_automaton = anchors ? 2 : (lds ? 1 : 0);     // 2 = anchor filter + exact list scan
    c->cnt.anchor_keys = anchors ? c->K.n_keys : 0;
    c->cnt.anchor_table_kind = anchors ? (c->K.log_size > 15 ? 2 : c->K.mode) : 0;
    c->spans_p2 = true;
    return c->lookback_ok();
}

static int recruit_impl(crass_hip_ctx *c, const ExtraFound &x)
{
    if (!c->have_reads) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    if (c->p1d.active) { const int ds = settle_p1(c); if (ds) return ds; }
    c->q_read.clear(); c->q_low.clear(); c->q_start.clear(); c->q_end.clear(); c->q_token.clear(); c->q_dr_len.clear(); c->q_dr.clear();
    c->have_pass2 = false;
    c->q_blob_active = false;
    c->cnt.n_pass2_found = 0;
    // (the host-loop sink's copies — over copy_stream or on DMA engines — may still be running: their sources, g_surv / g_dr /
    // g_fidx / g_ss, are the sink's own and nothing in this pass writes them, so nobody waits here.  Round 5 gathered the slots
    // in place in d_fidx, which this pass writes near its end, and the wait that needed was 0.5 ms of a 1 M x 10 kbp step)
    // findSingletons is only called when the non-redundant set is non-empty (WorkHorse.cpp:373)
    if (c->n_installed_patterns == 0) { c->have_pass2 = true; return CRASS_OK; }
    if (!c->have_patterns) return CRASS_ERR_STATE;
    const uint64_t n = c->R.n_reads;
    const uint64_t n_words = (n + 63) / 64;
    if (x.n_host) { const int ms = mark_extra_found(c, x.host, x.n_host); if (ms) return ms; }
    if (x.n_dev) { const int ms = mark_extra_found_device(c, x.dev, x.n_dev); if (ms) return ms; }
    HIPCHK(c, c->stamp(5, 1));
    const bool dmp = c->dm.active;                  // pattern set built on the device (dmerge.hip)
    // exception reads: with a device-built (pure ACGT) pattern set they go through the anchor filter and the exact
    // verification on their packed words like every other read (k_dm_verify checks the bytes of a candidate);
    // otherwise the byte-wise automaton scans them separately
    const uint64_t n_exc = dmp ? 0 : c->R.n_exc;    // (so dmp implies no exception list: every slot below is a flagged read's)
    bool anchors = false, lds = false;
    if (const int ps = launch_probe(c, dmp, n_exc, anchors, lds)) return ps;
    HIPCHK(c, c->stamp(6, 1));
    Lookback lbr;
    HIPCHK(c, launch_compact(c->d_mask.p, n_words, n, c->d_word_prefix.p, c->d_block_sums.p, c->d_idx.p, n, c->d_count.p, c->stream,
                             nullptr, 0, nullptr, 0, c->next_lookback(n_words, &lbr)));
    // Speculative tail (device merge path): verification, finish and the hand-off pack are launched with the hit
    // count still on the device, sized by a bound learnt from the previous call; the exact count arrives with the
    // final synchronisation, and a bound that was too small repeats the tail with the exact count.
    const bool spec = dmp && c->hit_cap_hint && !c->env.no_speculation && !c->recruit_exact;
    c->recruit_exact = false;
    // (speculative: the count reaches the host with the last kernel of the tail, k_pack_p2_blob)
    if (!spec) { const int rs = read_count(c); if (rs) return rs; }
    if (!spec && dmp && c->dm.h_st.p->fail) return recruit_after_host_merge(c, x);
    const uint64_t n_hits = spec ? c->hit_cap_hint : c->h_count.p[0];
    // (sized for the bound the next call will speculate with, so that it does not re-allocate)
    const uint64_t h_alloc = spec ? n_hits : std::max<uint64_t>(n_hits, hit_bound(n_hits));
    { const int as = ensure_recruit_buffers(c, h_alloc, n_exc, dmp, anchors); if (as) return as; }
    if (anchors) {
        if (dmp) HIPCHK(c, launch_dm_verify(c->R, c->dm.M, c->d_idx.p, c->d_count.p, n_hits, c->d_slot_info.p, c->d_slot_pid.p, c->stream));
        else HIPCHK(c, launch_recruit_list(c->R, c->A, c->d_idx.p, c->d_count.p, n_hits, c->d_slot_info.p, c->d_slot_pid.p, c->stream));
    }
    const bool dev_tokens = dmp || (anchors && c->have_pat_token && c->have_merge);
    HIPCHK(c, launch_recruit_finish(c->R, c->d_idx.p, c->d_count.p, n_hits, anchors ? c->d_slot_info.p : c->d_hit_info.p, anchors, false,
                                    dev_tokens ? c->d_slot_pid.p : nullptr, dev_tokens ? (dmp ? c->dm.M.pat_token : c->a_pat_token.p) : nullptr,
                                    c->d_rec.p, dmp ? nullptr : c->d_dr.p, c->dr_stride, c->stream, dmp ? c->dm.M.pat_mask : nullptr));
    if (n_exc)
        HIPCHK(c, launch_recruit_finish(c->R, nullptr, nullptr, n_exc, c->d_exc_hit.p, true, true, nullptr, nullptr, c->d_rec.p + n_hits,
                                        c->d_dr.p + n_hits * c->dr_stride, c->dr_stride, c->stream));
    HIPCHK(c, c->stamp(7, 2));
    if (dmp) return recruit_device_sink(c, spec, n_hits, x);
    return recruit_host_sink(c, n_hits, n_exc, anchors, lds);
}

int crass_hip_recruit(crass_hip_ctx *c, const uint64_t *extra_found, uint64_t n_extra)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    return recruit_impl(c, ExtraFound{extra_found, n_extra, nullptr, 0});
}

int crass_hip_recruit_found(crass_hip_ctx *c, const uint64_t *extra_found, uint64_t n_extra, const uint64_t *d_extra_found, uint64_t n_d_extra)
{
    if (!c || (n_d_extra && !d_extra_found)) return CRASS_ERR_INVALID_ARG;
    return recruit_impl(c, ExtraFound{extra_found, n_extra, d_extra_found, n_d_extra});
}

int crass_hip_get_recruits(const crass_hip_ctx *c, crass_recruits *o)
{
    if (!c || !o) return CRASS_ERR_INVALID_ARG;
    if (!c->have_pass2) return CRASS_ERR_STATE;
    if (c->q_blob_active && !c->q_wide_ready) {
        // crass_recruits' arrays from the compact blob; the DR string of a recruit is its token's string
        crass_hip_ctx *mc = const_cast<crass_hip_ctx *>(c);
        const uint8_t *hb = c->h_qblob.p;
        const P2Blob &b = c->q_lay;
        const uint64_t n = c->q_n;
        const uint32_t *b_tok = (const uint32_t *)(hb + b.token);
        const uint16_t *b_start = (const uint16_t *)(hb + b.start), *b_end = (const uint16_t *)(hb + b.end);
        mc->q_read.resize(n); mc->q_token.resize(n); mc->q_low.resize(n);
        mc->q_start.resize(n); mc->q_end.resize(n); mc->q_dr_len.resize(n); mc->q_dr.resize(n * (size_t)c->dr_stride);
        // token strings: the device-built view (h_view) or the host-built arena
        const bool dv = c->dm.active && c->dm.view_ready;
        const uint8_t *vb = c->dm.h_view.p;
        const uint64_t *v_off = dv ? (const uint64_t *)(vb + c->dm.view_tot.lay.tok_off) : nullptr;
        const char *v_chars = dv ? (const char *)(vb + c->dm.view_tot.lay.tok_chars) : nullptr;
        const uint32_t n_tok = dv ? c->dm.view_tot.n_tok : c->merge.tokens.size();
        // ~100 bytes per recruit (436 k at 100 M reads): ranges of recruits on the host pool
        const size_t per_task = 16384;
        const size_t stride = c->dr_stride;
        host_parallel_for((size_t)((n + per_task - 1) / per_task), 16, [&](size_t task) {
            const uint64_t k0 = task * per_task, k1 = std::min<uint64_t>(n, k0 + per_task);
            memset(mc->q_dr.data() + k0 * stride, 0, (size_t)(k1 - k0) * stride);
            for (uint64_t k = k0; k < k1; k++) {
                mc->q_read[k] = b.narrow ? c->read_base + ((const uint32_t *)(hb + b.read))[k] : ((const uint64_t *)(hb + b.read))[k];
                const uint32_t t = b.narrow == 2 ? (b_tok[k] & 0x7FFFFFFFu) : b_tok[k];
                mc->q_token[k] = t;
                size_t tlen = 0;
                if (t >= 2 && t - 2 < n_tok) {
                    tlen = dv ? (size_t)(v_off[t - 1] - v_off[t - 2]) : (size_t)c->merge.tokens.strings.len(t - 2);
                    if (dv) memcpy(mc->q_dr.data() + k * stride, v_chars + v_off[t - 2], tlen);
                    else memcpy(mc->q_dr.data() + k * stride, c->merge.tokens.strings.data(t - 2), tlen);
                }
                if (b.narrow == 2) {
                    // the 9-byte form: orientation in the token's top bit; the repeat is as long as its token's string and ends
                    // at start + length - 1 in either orientation (k_recruit_finish)
                    mc->q_low[k] = (uint8_t)(b_tok[k] >> 31);
                    mc->q_start[k] = (hb + b.start)[k];
                    mc->q_dr_len[k] = (uint16_t)tlen;
                    mc->q_end[k] = mc->q_start[k] + (tlen ? (uint32_t)tlen - 1u : 0u);
                    continue;
                }
                mc->q_low[k] = (hb + b.low)[k];
                if (b.narrow) { mc->q_start[k] = (hb + b.start)[k]; mc->q_end[k] = (hb + b.end)[k]; }
                else { mc->q_start[k] = b_start[k]; mc->q_end[k] = b_end[k]; }
                mc->q_dr_len[k] = (hb + b.dr_len)[k];
            }
        });
        mc->q_wide_ready = true;
    }
    o->n = c->q_read.size(); o->read_idx = c->q_read.data(); o->low_lexi = c->q_low.data();
    o->start = c->q_start.data(); o->end = c->q_end.data(); o->dr_stride = c->dr_stride;
    o->dr_len = c->q_dr_len.data(); o->dr_chars = c->q_dr.data(); o->token = c->q_token.data();
    return CRASS_OK;
}

} // extern "C"

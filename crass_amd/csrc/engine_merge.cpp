// engine_merge.cpp — the merge of the context behind include/crass_hip.h: the merge on the device (dmerge.hip: prepare /
// enqueue / commit) and the host view built from it, the host merge (merge.cpp) and the fall-back to it, every
// crass_hip_merge* entry point, the distinct list, the exchange's set-up and crass_hip_get_merge.
#include "engine_ctx.h"

#include <cstdio>
#include <new>

extern "C" {

// ---- the merge on the device (dmerge.hip).  dx_*: distinct strings in token order on the device; hx_*: the same list in pinned
// host memory; n_tok: the token count, or — with d_ntok — the bound the launch is sized for while the count is still on the device ----
static bool device_merge_applies(const crass_hip_ctx *c)
{
    if (c->env.host_merge) return false;                 // A/B switch: force the host merge (merge.cpp)
    return c->have_pass1 && c->dev_tokens() && c->prm.lowDRsize >= (int)kDevMinDR &&
           c->dr_stride <= 64 && c->n_dx <= (1u << 20);
}

// buffers + the kernels' argument block for a merge over (up to) n_tok tokens; nothing is launched
int device_merge_prepare(crass_hip_ctx *c, const char *dx_chars, const uint16_t *dx_len, uint64_t n_tok, const uint32_t *d_ntok)
{
    crass_hip_ctx::DM &d = c->dm;
    const uint32_t n = (uint32_t)n_tok, stride = c->dr_stride;
    if (!d.ev_done) {
        HIPCHK(c, hipEventCreateWithFlags(&d.ev_done, hipEventDisableTiming));
        HIPCHK(c, hipEventCreate(&d.ev_t0)); HIPCHK(c, hipEventCreate(&d.ev_t1));
    }
    DevMerge M{};
    M.dx_chars = dx_chars; M.dx_len = dx_len; M.stride = stride; M.n_tok = n; M.d_ntok = d_ntok;
    M.thr = (uint32_t)std::max(c->prm.kmer_clust_size, 2); M.kmax = stride - 10;
    M.min_len = (uint32_t)c->prm.lowDRsize;
    if (!dm_anchor_shape(M.min_len, M.akey_bases, M.akey_shift)) return CRASS_ERR_STATE;      // (every caller checked lowDRsize >= kDevMinDR)
    { const char *ab = getenv("CRASS_DM_ABLATE"); M.ablate = ab ? (uint32_t)strtoul(ab, nullptr, 0) : 0u; }      // (profiling aid, read per merge)
    M.kset_log = 10; while ((1ull << M.kset_log) < 32ull * n) M.kset_log++;
    M.tab_log_alloc = 16; while (M.tab_log_alloc < 24 && (1ull << M.tab_log_alloc) < 48ull * n) M.tab_log_alloc++;
    HIPCHK(c, d.packed.ensure((size_t)n * 4)); HIPCHK(c, d.codes.ensure((size_t)n * M.kmax)); HIPCHK(c, d.owner.ensure((1u << 22) + kDmBadSlots));
    HIPCHK(c, d.tmask.ensure((size_t)n * 2)); HIPCHK(c, d.bk_key.ensure(kDmBadSlots));
    HIPCHK(c, d.root_of.ensure(n)); HIPCHK(c, d.blank.ensure(n)); HIPCHK(c, d.pat_token.ensure((size_t)n * 2));
    HIPCHK(c, d.kset_key.ensure((size_t)1 << M.kset_log)); HIPCHK(c, d.kset_u32.ensure((size_t)3 << M.kset_log));
    HIPCHK(c, d.ent_slot.ensure((size_t)n * 16)); HIPCHK(c, d.ents.ensure((size_t)n * 64));
    M.rset_log = 10; while ((1ull << M.rset_log) < 4ull * n) M.rset_log++;
    HIPCHK(c, d.rset_key.ensure((size_t)1 << M.rset_log)); HIPCHK(c, d.rset_u32.ensure((size_t)3 << M.rset_log));
    HIPCHK(c, d.rd_slot.ensure(n)); HIPCHK(c, d.rents.ensure((size_t)n * 4));
    HIPCHK(c, d.anchor_tab.ensure((size_t)1 << M.tab_log_alloc)); HIPCHK(c, d.st.ensure(1)); HIPCHK(c, d.hot.ensure(kDmHotWords)); HIPCHK(c, d.anchor_fp.ensure(1u << 15));
    HIPCHK(c, d.h_st.ensure(1)); HIPCHK(c, d.h_root.ensure(n)); HIPCHK(c, d.h_blank.ensure(n));
    M.packed = d.packed.p; M.codes = d.codes.p; M.owner = d.owner.p; M.bk_key = d.bk_key.p; M.root_of = d.root_of.p;
    M.tmask = d.tmask.p; M.pat_mask = d.tmask.p; M.blank = d.blank.p; M.pat_token = d.pat_token.p;
    M.kset_key = d.kset_key.p; M.kset_cnt = d.kset_u32.p; M.kset_base = d.kset_u32.p + ((size_t)1 << M.kset_log);
    M.kset_fill = d.kset_u32.p + ((size_t)2 << M.kset_log); M.ent_slot = d.ent_slot.p; M.ents = d.ents.p; M.ent_cap = 16u * n;
    M.rset_key = d.rset_key.p; M.rset_cnt = d.rset_u32.p; M.rset_base = d.rset_u32.p + ((size_t)1 << M.rset_log);
    M.rset_fill = d.rset_u32.p + ((size_t)2 << M.rset_log); M.rd_slot = d.rd_slot.p; M.rents = d.rents.p;
    if (!c->n_cu) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || v <= 0) v = 64;
        c->n_cu = (uint32_t)v;
    }
    M.n_cu = c->n_cu;
    M.h_st = d.h_st.p; M.h_root = d.h_root.p; M.h_blank = d.h_blank.p;
    // the host view of this merge is assembled on the device too (k_dmx_*), unless this context only reports its own
    // candidates' tokens (ranks > 0 of a group)
    // — and only where the host's build would be on the critical path: a rank of a multi-rank job (its shard's pass 2 is shorter
    // than the 0.6 ms the host needs for 42 k tokens).  A single context hides the host's build behind its own pass 2 (1.5 ms of
    // device work at 100 M reads), and there the export's kernels, running beside pass 2's probe, cost the step 0.08-0.1 ms
    // (4.65 vs 4.73-4.77 ms, same box, profiles/NOTES_r04.md): CRASS_DEVICE_VIEW=1 forces the export there (tests, A/B).
    M.x_on = (!c->env.no_device_view && !c->host_view_light && n <= (1u << 20) && (c->xchg.active || c->env.force_device_view)) ? 1u : 0u;
    if (M.x_on) {
        if (!d.view_stream) {
            // lowest priority: the export fills whatever the merge's own kernels and pass 2's probe leave idle (at equal priority
            // its 1 024-thread blocks kept the probe kernel's blocks off the CUs: 144 -> 216 us for an eighth of the 100 M reads)
            int prio_lo = 0, prio_hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
            static const bool view_same_prio = getenv("CRASS_VIEW_SAME_PRIORITY") != nullptr;      // A/B switch
            HIPCHK(c, hipStreamCreateWithPriority(&d.view_stream, hipStreamNonBlocking, view_same_prio ? 0 : prio_lo));
            HIPCHK(c, hipEventCreateWithFlags(&d.ev_fork, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&d.ev_view, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&d.ev_apply, hipEventDisableTiming));
            d.dma_view = sdma_create();                 // (nullptr: the runtime's copy is used)
            d.dma_view2 = sdma_create();
            d.dma_view3 = sdma_create();
        }
        const uint64_t cap = view_layout(n, n, 2ull * n, (uint64_t)n * stride, 2ull * n * stride).total;
        HIPCHK(c, d.x_u32.ensure((size_t)n * 8)); HIPCHK(c, d.x_members.ensure(n)); HIPCHK(c, d.x_tile.ensure(kDmxTiles * kDmxVals + 4));
        HIPCHK(c, d.x_blob.ensure(cap + 64)); HIPCHK(c, d.x_tot.ensure(1)); HIPCHK(c, d.x_htot.ensure(2));      // (x_htot[1]: the totals as k_dmx_apply published them)
        if (!d.h_view.p) HIPCHK(c, d.h_view.ensure(std::max<uint64_t>(cap / 4, 1u << 16)));      // (grown by the build if a merge needs more)
        uint32_t *x = d.x_u32.p;
        M.x_size = x; M.x_kept = x + n; M.x_kchars = x + 2ull * n; M.x_fill = x + 3ull * n;
        M.x_gid = x + 4ull * n; M.x_goff = x + 5ull * n; M.x_pat0 = x + 6ull * n; M.x_pch0 = x + 7ull * n;
        M.x_members = d.x_members.p; M.x_tile = d.x_tile.p; M.x_blob = d.x_blob.p; M.x_tot = d.x_tot.p; M.x_htot = d.x_htot.p;
        M.x_group_cap = c->env.view_group_cap;
        M.x_sort_max = c->env.view_sort_max;
    }
    M.inject_fail = c->env.dm_inject_fail ? 1u : 0u;
    M.group_cap = c->env.dm_group_cap;
    M.anchor_tab = d.anchor_tab.p; M.anchor_fp = d.anchor_fp.p; M.m1 = 0x9E3779u; M.m2 = 0x85EBCBu; M.st = d.st.p; M.hot = d.hot.p;
    d.M = M;
    return CRASS_OK;
}

// the kernels only; the context's state is untouched until device_merge_commit.  prepared: device_merge_prepare
// ran for exactly these arguments and an earlier kernel of the step cleared the tables (dm_init_slice)
int device_merge_enqueue(crass_hip_ctx *c, const char *dx_chars, const uint16_t *dx_len, uint64_t n_tok, const uint32_t *d_ntok,
                                bool prepared)
{
    crass_hip_ctx::DM &d = c->dm;
    if (!prepared) { const int ps = device_merge_prepare(c, dx_chars, dx_len, n_tok, d_ntok); if (ps) return ps; }
    const double tl0 = now_ms();
    if (d.view_launched) HIPCHK(c, hipStreamWaitEvent(c->stream, d.ev_view, 0));     // (an abandoned merge's export still owns the x_* words)
    if (c->timing_level >= 2) HIPCHK(c, hipEventRecord(d.ev_t0, c->stream));
    d.M.flag_pre = c->poll_on ? c->h_flags.p + 1 : nullptr; d.M.flag_pre_val = c->want_pre = ++c->flag_seq;
    d.M.flag_post = c->poll_on ? c->h_flags.p + 2 : nullptr; d.M.flag_post_val = d.want_post = ++c->flag_seq;
    d.M.flag_blank = c->poll_on ? c->h_flags.p + 3 : nullptr; d.M.flag_blank_val = d.want_blank = ++c->flag_seq;
    static const bool view_inline = getenv("CRASS_VIEW_INLINE") != nullptr;      // A/B switch: the export on the merge's own stream
    HIPCHK(c, launch_device_merge(d.M, c->stream, prepared, d.M.x_on ? (view_inline ? c->stream : d.view_stream) : nullptr, d.ev_fork, d.ev_view,
                                  view_inline ? nullptr : d.ev_apply));
    d.apply_recorded = d.M.x_on && !view_inline;
    d.view_launched = d.M.x_on != 0;
    if (c->timing_level >= 2) HIPCHK(c, hipEventRecord(d.ev_t1, c->stream));
    if (c->env.merge_profile)
        fprintf(stderr, "[crass_dm] host: pass-1 sync -> merge launch start %.1f us, launching the merge kernels %.1f us\n",
                1e3 * (tl0 - c->t_p1_sync), 1e3 * (now_ms() - tl0));
    // the per-token results the host view is rebuilt from (a few 10 KB): the helper thread polls the stage flag that pass 2's
    // probe stores, or waits for this event
    if (!c->poll_on) HIPCHK(c, hipEventRecord(d.ev_done, c->stream));
    return CRASS_OK;
}

static void apply_build_result(crass_hip_ctx *c)
{
    crass_hip_ctx::DM::BuildResult &b = c->dm.br;
    if (b.hip) { c->last_hip = b.hip; b.hip = 0; }
    if (!b.valid) return;
    b.valid = false;
    c->n_installed_patterns = b.n_patterns;
    c->cnt.n_patterns = b.n_patterns;
    c->cnt.ac_states = 0;
    c->cnt.anchor_keys = b.n_keys;
    c->cnt.ms_merge_device = b.ms_device;
}

// The host view of a merge that ran on the device, down to build_host_merge: runs on the helper thread OR on the caller's (never
// both at once), touches c->merge and dm.br only.  Here: the merge's kernels are through (the probe of pass 2 is normally queued
// right behind the merge; a caller that asks for the merge's view without running pass 2 gets it after the poll's budget)
static int dm_wait_done(crass_hip_ctx *c)
{
    crass_hip_ctx::DM &d = c->dm;
    if (c->poll_on && c->poll_flag(2, d.want_post, 1.0)) return CRASS_OK;
    const hipError_t e = c->poll_on ? hipStreamSynchronize(c->stream) : hipEventSynchronize(d.ev_done);
    if (e != hipSuccess) { d.br.hip = (int)e; return e == hipErrorOutOfMemory ? CRASS_ERR_OOM : CRASS_ERR_HIP; }
    return CRASS_OK;
}

static void dm_publish(crass_hip_ctx *c)
{
    crass_hip_ctx::DM &d = c->dm;
    d.br.n_patterns = d.h_st.p->n_patterns; d.br.n_keys = d.h_st.p->n_keys;
    float ms = 0;
    if (c->timing_level >= 2) (void)hipEventElapsedTime(&ms, d.ev_t0, d.ev_t1);
    d.br.ms_device = ms;
    d.br.valid = true;
}

// this context's own candidates' tokens through cmap, their distinct strings' ranks in the merged list; false: a rank out of range
static bool own_cand_tokens(crass_hip_ctx *c, const uint32_t *cmap)
{
    const crass_hip_ctx::DM &d = c->dm;
    c->merge.clear();
    c->merge.cand_token.resize(d.n_cand);
    for (uint64_t k = 0; k < d.n_cand; k++) {
        if (cmap[k] >= d.n_tok) { c->merge.clear(); return false; }
        c->merge.cand_token[k] = cmap[k] + 2;
    }
    return true;
}

// The view itself comes from the device (k_dmx_*).  CRASS_OK: adopted, the view is built; kHostBuildsView: not usable (a group
// beyond x_group_cap, totals that do not add up, no DMA engine for it), the merge is through and the host builds the view
// from the per-token results; anything else: a failure
constexpr int kHostBuildsView = 1001;
static int adopt_device_view(crass_hip_ctx *c, const uint32_t *cmap, double tb00)
{
    crass_hip_ctx::DM &d = c->dm;
    // what is left for the host are its own candidates' tokens (pass 1's outputs, done while the merge kernels run), one DMA
    // copy of the blob, and pointers
    if (!own_cand_tokens(c, cmap)) return CRASS_ERR_STATE;
    const double tv0 = now_ms();
    // The device's part of the view (k_dmx_*, forked behind k_dm_greedy): tok_off, the token strings, grp_off — complete
    // behind k_dmx_apply, copied first, beside the kernels that order the members — and grp_tokens, complete behind the
    // export's last kernel.  The PATTERN LIST (per group the survivors by length then token, then their reverse
    // complements: WorkHorse.cpp:690-697, remove_redundant's order) is put together here, from that view and blank[],
    // which k_dm_redundant has finished when k_dm_keys' stage flag shows — while the device builds pass 2's index and
    // runs pass 2.  (Until round 6 the export ran behind k_dm_redundant and ranked the patterns too: its last kernels
    // shared the CUs with pass 2's probe and verification, and the view was ready ~20 us after the step's last kernel.)
    auto hipfail = [&](hipError_t e) { d.br.hip = (int)e; return e == hipErrorOutOfMemory ? CRASS_ERR_OOM : CRASS_ERR_HIP; };
    bool usable = d.apply_recorded && d.dma_view && d.dma_view2 && d.dma_view3;
    DevViewTotals E{};
    if (usable) {
        const hipError_t e = hipEventSynchronize(d.ev_apply);
        if (e != hipSuccess) return hipfail(e);
        E = d.x_htot.p[1];
        usable = E.ok && E.n_tok == d.n_tok && E.n_groups >= 1 && E.lay.total <= d.x_blob.n && E.lay.grp_tokens <= E.lay.pat_off && E.lay.pat_off <= E.lay.total;
    }
    if (usable) {
        // room for the whole view whatever survives (every token a pattern, twice): grown before the first copy lands
        const uint64_t room = view_layout(E.n_tok, E.n_groups, 2ull * E.n_tok, E.tok_chars, 2ull * E.tok_chars).total;
        if (d.h_view.n < room) { const hipError_t e2 = d.h_view.ensure(room + room / 4); if (e2 != hipSuccess) return hipfail(e2); }
        bool ok = sdma_start(d.dma_view2, d.x_blob.p, d.h_view.p, E.lay.grp_tokens);
        struct Guard { SdmaCopy *s; bool on; ~Guard() { if (on) (void)sdma_wait(s); } } g2{d.dma_view2, ok}, g1{d.dma_view, false}, g3{d.dma_view3, false};
        // blank[]: final when k_dm_redundant is through (the flag is k_dm_keys'); a poll that runs out waits for the merge
        if (!(c->poll_on && c->poll_flag(3, d.want_blank, 2.0))) { if (const int ws = dm_wait_done(c)) return ws; }
        g3.on = ok && sdma_start(d.dma_view3, d.blank.p, d.h_blank.p, d.n_tok);
        ok = ok && g3.on;
        { const hipError_t e = hipEventSynchronize(d.ev_view); if (e != hipSuccess) return hipfail(e); }
        const DevViewTotals T0 = *d.x_htot.p;
        usable = T0.ok && T0.n_tok == d.n_tok && T0.n_groups == E.n_groups && T0.lay.grp_tokens == E.lay.grp_tokens && T0.lay.pat_off == E.lay.pat_off;
        if (usable) {
            g1.on = ok && sdma_start(d.dma_view, d.x_blob.p + E.lay.grp_tokens, d.h_view.p + E.lay.grp_tokens, E.lay.pat_off - E.lay.grp_tokens);
            ok = ok && g1.on;
            if (g1.on) { g1.on = false; ok = sdma_wait(d.dma_view) == 0 && ok; }
            if (g2.on) { g2.on = false; ok = sdma_wait(d.dma_view2) == 0 && ok; }
            if (g3.on) { g3.on = false; ok = sdma_wait(d.dma_view3) == 0 && ok; }
            if (!ok) {                              // (no engine: the runtime's copies, behind the export on its stream)
                hipError_t e = hipMemcpyAsync(d.h_view.p, d.x_blob.p, E.lay.pat_off, hipMemcpyDeviceToHost, d.view_stream);
                if (e == hipSuccess) e = hipMemcpyAsync(d.h_blank.p, d.blank.p, d.n_tok, hipMemcpyDeviceToHost, d.view_stream);
                if (e == hipSuccess) e = hipStreamSynchronize(d.view_stream);
                if (e != hipSuccess) return hipfail(e);
            }
            const double tv1 = now_ms();
            // ---- the pattern list ----
            uint8_t *hb = d.h_view.p;
            const uint64_t *tok_off = reinterpret_cast<const uint64_t *>(hb + E.lay.tok_off), *grp_off = reinterpret_cast<const uint64_t *>(hb + E.lay.grp_off);
            const char *tok_chars = reinterpret_cast<const char *>(hb + E.lay.tok_chars);
            const uint32_t *grp_tokens = reinterpret_cast<const uint32_t *>(hb + E.lay.grp_tokens);
            const uint8_t *blank = d.h_blank.p;
            // (over the host pool: a group's part of the list depends on the groups in front of it only through two offsets —
            // one thread took 1.1 ms for 13 k patterns of 42 k tokens; chunks of groups of ~equal member counts)
            const uint32_t NG = E.n_groups;
            const size_t n_chunks = std::min<size_t>(64, NG);
            std::vector<uint32_t> chunk_g0(n_chunks + 1, NG);
            {
                size_t cidx = 0;
                for (uint32_t g = 0; g < NG && cidx < n_chunks; g++)
                    if (grp_off[g] * n_chunks >= (uint64_t)cidx * E.n_tok) chunk_g0[cidx++] = g;
                for (; cidx < n_chunks; cidx++) chunk_g0[cidx] = NG;
                chunk_g0[n_chunks] = NG;
            }
            std::vector<uint64_t> ck(n_chunks + 1, 0), cc(n_chunks + 1, 0);     // kept tokens / their characters per chunk
            std::atomic<int> bad{0};
            bool sane = grp_off[NG] == E.n_tok;
            if (sane) host_parallel_for(n_chunks, 64, [&](size_t ci) {
                uint64_t k = 0, chs = 0;
                for (uint64_t i = grp_off[chunk_g0[ci]], e = chunk_g0[ci + 1] < NG ? grp_off[chunk_g0[ci + 1]] : E.n_tok; i < e; i++) {
                    const uint32_t t = grp_tokens[i] - 2u;
                    if (t >= E.n_tok) { bad = 1; return; }
                    const uint64_t len = tok_off[t + 1] - tok_off[t];
                    if (len > 64) { bad = 1; return; }
                    if (!blank[t]) { k++; chs += len; }
                }
                ck[ci + 1] = k; cc[ci + 1] = chs;
            });
            sane = sane && !bad.load();
            for (size_t ci = 0; ci < n_chunks; ci++) { ck[ci + 1] += ck[ci]; cc[ci + 1] += cc[ci]; }
            const uint64_t n_kept = ck[n_chunks], kept_chars = cc[n_chunks];
            if (sane) {
                DevViewTotals T = T0;
                T.n_kept = (uint32_t)n_kept; T.kept_chars = (uint32_t)kept_chars;
                T.lay = view_layout(E.n_tok, E.n_groups, 2ull * n_kept, E.tok_chars, 2ull * kept_chars);
                uint64_t *pat_off = reinterpret_cast<uint64_t *>(hb + T.lay.pat_off);
                char *pat_chars = reinterpret_cast<char *>(hb + T.lay.pat_chars);
                uint32_t *pat_group = reinterpret_cast<uint32_t *>(hb + T.lay.pat_group);
                host_parallel_for(n_chunks, 64, [&](size_t ci) {
                    static thread_local std::vector<uint32_t> order;        // a group's survivors by length, then token
                    static const struct Comp { char t[256]; Comp() { for (int i = 0; i < 256; i++) t[i] = (char)i; t['A'] = 'T'; t['C'] = 'G'; t['G'] = 'C'; t['T'] = 'A'; } } comp;   // SeqUtils.cpp:50-59 over the device merge's alphabet
                    uint64_t p = 2ull * ck[ci], ch = 2ull * cc[ci];
                    for (uint32_t g = chunk_g0[ci]; g < chunk_g0[ci + 1]; g++) {
                        const uint64_t m0 = grp_off[g], m1 = grp_off[g + 1];
                        uint32_t cnt[66] = {0};
                        uint32_t kg = 0;
                        for (uint64_t i = m0; i < m1; i++) {
                            const uint32_t t = grp_tokens[i] - 2u;
                            if (blank[t]) continue;
                            cnt[tok_off[t + 1] - tok_off[t] + 1]++; kg++;
                        }
                        for (int l = 1; l < 66; l++) cnt[l] += cnt[l - 1];
                        order.resize(kg);
                        for (uint64_t i = m0; i < m1; i++) {             // (token order inside a length: the list is sorted by token)
                            const uint32_t t = grp_tokens[i] - 2u;
                            if (!blank[t]) order[cnt[tok_off[t + 1] - tok_off[t]]++] = t;
                        }
                        uint64_t chr = ch;
                        for (uint32_t j = 0; j < kg; j++) chr += tok_off[order[j] + 1] - tok_off[order[j]];
                        for (uint32_t j = 0; j < kg; j++) {
                            const uint32_t t = order[j];
                            const uint64_t len = tok_off[t + 1] - tok_off[t];
                            const char *src = tok_chars + tok_off[t];
                            pat_off[p + j] = ch; pat_group[p + j] = g + 1u;
                            pat_off[p + kg + j] = chr; pat_group[p + kg + j] = g + 1u;
                            memcpy(pat_chars + ch, src, len);
                            char *dst = pat_chars + chr;
                            for (uint64_t q = 0; q < len; q++) dst[q] = comp.t[(unsigned char)src[len - 1 - q]];      // reverseComplement
                            ch += len; chr += len;
                        }
                        p += 2ull * kg; ch = chr;
                    }
                });
                pat_off[2ull * n_kept] = 2ull * kept_chars;
                const double tv2 = now_ms();
                if (const int ws = dm_wait_done(c)) return ws;
                if (d.h_st.p->fail) return CRASS_ERR_STATE;
                if (sane && 2u * T.n_kept == d.h_st.p->n_patterns) {
                    d.view_tot = T;
                    d.view_ready = true;
                    d.host_built = true;
                    if (c->env.merge_profile)
                        fprintf(stderr, "[crass_dm] helper: candidates' tokens %.1f us, the device's part of the view in host memory %.1f us later, pattern list %.1f us (done %.1f us after the pass-1 sync; the merge's state %.1f us after that)\n",
                                1e3 * (tv0 - tb00), 1e3 * (tv1 - tv0), 1e3 * (tv2 - tv1), 1e3 * (tv2 - c->t_p1_sync), 1e3 * (now_ms() - tv2));
                    dm_publish(c);
                    return CRASS_OK;
                }
            }
        }
    }
    if (const int ws = dm_wait_done(c)) return ws;
    if (d.h_st.p->fail) return CRASS_ERR_STATE;
    // (a group beyond x_group_cap, or totals that do not add up: the host builds the view from the per-token results)
    c->n_view_fallbacks++;
    return kHostBuildsView;
}

static int build_host_merge(crass_hip_ctx *c)
{
    crass_hip_ctx::DM &d = c->dm;
    if (!d.active || d.host_built) return CRASS_OK;
    {   // once per thread and device: the helper thread runs this for every step
        static thread_local int tl_device = -1;
        if (tl_device != c->device) { (void)hipSetDevice(c->device); tl_device = c->device; }
    }
    // every exit waits for the view export (a few small kernels on view_stream): whoever re-uses the x_* words or the blob
    // next must find them idle
    struct DrainView {
        crass_hip_ctx::DM &d;
        ~DrainView() { if (d.view_launched && d.ev_view) (void)hipEventSynchronize(d.ev_view); }
    } drain{d};
    // local merge: the token strings and the candidates' tokens only need pass 1's outputs, which the host has
    // already waited for — that half of the host view is built while the merge kernels are still running
    // (the gathered form too: the global distinct list and every gathered row's rank in it were written to pinned memory
    // by the de-duplication kernels, which the host has waited for before it committed the merge)
    const double tb00 = now_ms();
    if (const int ws = c->wait_dx()) { d.br.hip = c->last_hip; return ws; }      // (the candidates' indices and the distinct strings: DMA copies)
    const uint32_t *cmap = c->h_dmap.p;
    if (d.global) {                                     // own candidate -> own distinct string -> its rank in the global list
        d.cand_map.resize(d.n_cand);
        for (uint64_t k = 0; k < d.n_cand; k++) d.cand_map[k] = d.h_gmap.p[d.my_off + c->h_dmap.p[k]];
        cmap = d.cand_map.data();
    }
    if (c->host_view_light) {
        // a rank of a group other than rank 0: tokens, groups and patterns are read from rank 0's view (they are identical on
        // every rank); what is this rank's own are its candidates' tokens
        if (!own_cand_tokens(c, cmap)) return CRASS_ERR_STATE;
        if (const int ws = dm_wait_done(c)) return ws;
        if (d.h_st.p->fail) return CRASS_ERR_STATE;
        d.host_built = true;
        dm_publish(c);
        d.br.ms_device = 0;
        return CRASS_OK;
    }
    if (d.M.x_on && d.view_launched) {
        const int vs = adopt_device_view(c, cmap, tb00);
        if (vs != kHostBuildsView) return vs;
    }
    if (d.global && !d.hx_on_host) {                    // the gathered list stayed on the device: fetch it now
        hipError_t e = hipMemcpyAsync(d.h_gx_chars.p, d.gx_chars.p, d.n_tok * (size_t)c->dr_stride, hipMemcpyDeviceToHost, d.view_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d.h_gx_len.p, d.gx_len.p, d.n_tok * 2, hipMemcpyDeviceToHost, d.view_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d.view_stream);
        if (e != hipSuccess) { d.br.hip = (int)e; return CRASS_ERR_HIP; }
        d.hx_on_host = true;
    }
    if (!merge_from_device_begin(c->merge, d.hx_chars, d.hx_len, c->dr_stride, d.n_tok, cmap, d.n_cand)) return CRASS_ERR_STATE;
    host_pool_warm();                                   // the second half fans out over the pool: wake it while the device is busy
    const double tb0 = now_ms();
    if (const int ws = dm_wait_done(c)) return ws;
    const double tb1 = now_ms();
    if (d.h_st.p->fail) return CRASS_ERR_STATE;
    if (d.M.x_on) {                                     // (k_dm_fill_finish left the per-token results on the device)
        hipError_t e = hipMemcpyAsync(d.h_root.p, d.root_of.p, d.n_tok * 4, hipMemcpyDeviceToHost, d.view_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d.h_blank.p, d.blank.p, d.n_tok, hipMemcpyDeviceToHost, d.view_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d.view_stream);
        if (e != hipSuccess) { d.br.hip = (int)e; return CRASS_ERR_HIP; }
    }
    if (!merge_from_device_finish_roots(c->merge, d.h_root.p, d.h_blank.p, d.gid_tmp) ||
        c->merge.patterns.size() != d.h_st.p->n_patterns)
        return CRASS_ERR_STATE;
    d.host_built = true;
    if (c->env.merge_profile)
        fprintf(stderr, "[crass_dm] helper: first half %.1f us, waited %.1f us for the merge kernels, second half %.1f us (done %.1f us after the pass-1 sync)\n",
                1e3 * (tb0 - tb00), 1e3 * (tb1 - tb0), 1e3 * (now_ms() - tb1), 1e3 * (now_ms() - c->t_p1_sync));
    dm_publish(c);
    return CRASS_OK;
}

// the merge just queued becomes the context's merge: hx_*: the distinct list in pinned host memory
static int device_merge_commit(crass_hip_ctx *c, uint64_t n_tok, const char *hx_chars, const uint16_t *hx_len)
{
    crass_hip_ctx::DM &d = c->dm;
    d.hx_chars = hx_chars; d.hx_len = hx_len; d.n_tok = n_tok;
    d.active = true; d.host_built = false; d.view_ready = false; d.n_cand = c->n_cand();
    // the host view (tokens, groups, pattern list) is rebuilt by the helper thread as soon as the kernels are through
    // every field of the caller's side is set BEFORE the job is handed over: from submit() on, the helper thread owns
    // c->merge and dm.br until ensure_host_merge / quiesce_worker has waited for it
    c->have_merge = true; c->have_pass2 = false;
    c->have_patterns = true; c->have_anchors = false; c->have_pat_token = false;
    c->n_installed_patterns = 2;                                  // >= 1 survivor exists; the exact count arrives with h_st
    d.br = crass_hip_ctx::DM::BuildResult();
    d.build_status = CRASS_OK;
    d.build_pending = true;
    c->worker.submit([c] {
        int st;
        try { st = build_host_merge(c); } catch (const std::bad_alloc &) { st = CRASS_ERR_OOM; } catch (...) { st = CRASS_ERR_STATE; }
        c->dm.build_status = st;
    });
    return CRASS_OK;
}

// enqueue + commit
static int device_merge(crass_hip_ctx *c, const char *dx_chars, const uint16_t *dx_len, uint64_t n_tok, const char *hx_chars,
                        const uint16_t *hx_len)
{
    const int s = device_merge_enqueue(c, dx_chars, dx_len, n_tok, nullptr, false);
    if (s) return s;
    return device_merge_commit(c, n_tok, hx_chars, hx_len);
}

// c->merge for a merge that ran on the device: 0 ok, CRASS_ERR_STATE = the device path failed (the caller falls back)
int ensure_host_merge(crass_hip_ctx *c)
{
    crass_hip_ctx::DM &d = c->dm;
    if (d.build_pending) {                              // started by the merge call on the helper thread
        if (!c->worker.run_here_if_not_started()) c->worker.wait();
        d.build_pending = false;
        if (c->worker.take_failed()) d.build_status = CRASS_ERR_OOM;        // (the job threw: std::bad_alloc is the one thing it can throw)
        apply_build_result(c);
        if (d.build_status == CRASS_ERR_HIP || d.build_status == CRASS_ERR_OOM || d.build_status == CRASS_ERR_STATE) return d.build_status;
    }
    const int s = build_host_merge(c);
    apply_build_result(c);
    return s;
}

// the distinct list on the host, complete: the engine copies have landed and the strings' hashes are there (the host-merge
// forms want them; with the list brought over by DMA they are computed here, on the rare paths that need them)
static int ensure_host_distinct(crass_hip_ctx *c, bool want_hash)
{
    if (const int ws = c->wait_dx()) return ws;
    if (want_hash && !c->dx_hash_valid) {
        for (uint64_t j = 0; j < c->n_dx; j++) c->h_dx_hash.p[j] = TokenTable::hash(c->h_dx_chars.p + j * (size_t)c->dr_stride, c->h_dx_len.p[j]);
        c->dx_hash_valid = true;
    }
    return CRASS_OK;
}

// shared tail of the merge entry points: automaton/anchors/pattern tokens for pass 2
static int finish_merge(crass_hip_ctx *c, double t0)
{
    c->have_merge = true;
    c->have_pass2 = false;
    int s = install_patterns(c, c->merge.patterns);
    if (s == CRASS_OK && c->have_patterns) {
        // token of every pattern's low-lexi form, resolved once per pattern (merge.cpp) instead of once per
        // recruited read
        const std::vector<uint32_t> &pt = c->merge.pat_token;
        HIPCHK(c, c->a_pat_token.ensure(pt.size()));
        HIPCHK(c, hipMemcpyAsync(c->a_pat_token.p, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->have_pat_token = true;
    }
    if (const int bs = c->wait_bulk()) return bs;            // the per-candidate records are in host memory when the merge returns
    c->cnt.ms_merge_host = (float)(now_ms() - t0);
    return s;
}

// the distinct list of pass 1's candidates: the device's, or built here from the candidates' own strings
void ensure_distinct(crass_hip_ctx *c)
{
    if (c->have_distinct) return;
    if (c->dev_tokens()) { c->have_distinct = true; return; }   // straight from the device
    const uint64_t n = c->n_cand();
    const char *dr = c->cand_dr();
    const uint16_t *len = c->cand_dr_len();
    const uint32_t stride = c->dr_stride;
    c->dx_chars.clear(); c->dx_len.clear(); c->dx_map.assign(n, 0);
    if (c->have_rep && c->dense.active) {
        // the device already knows every candidate's first occurrence
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t f = c->h_rep.p[k];
            if (f == k) {
                c->dx_map[k] = (uint32_t)c->dx_len.size();
                c->dx_len.push_back(len[k]);
                c->dx_chars.insert(c->dx_chars.end(), dr + k * (uint64_t)stride, dr + (k + 1) * (uint64_t)stride);
            } else c->dx_map[k] = c->dx_map[f];
        }
    } else {
        TokenTable t;
        for (uint64_t k = 0; k < n; k++) {
            const char *p = dr + k * (uint64_t)stride;
            uint32_t tok = t.get(p, len[k]);
            if (!tok) {
                tok = t.add(p, len[k]);
                c->dx_len.push_back(len[k]);
                c->dx_chars.insert(c->dx_chars.end(), p, p + stride);
            }
            c->dx_map[k] = tok - 2;
        }
    }
    c->have_distinct = true;
}

// host merge over the concatenation of every rank's distinct list: the caller's, in host memory, or — on_device — the
// engine-owned copy (dm.g_chars / dm.g_len), copied back first
static int merge_global_host(crass_hip_ctx *c, const char *dr_chars, const uint16_t *dr_len, bool on_device, uint32_t dr_stride,
                             uint64_t n_global, uint64_t my_offset, double t0)
{
    std::vector<char> gc; std::vector<uint16_t> gl;
    if (on_device) {
        gc.resize(n_global * (size_t)dr_stride); gl.resize(n_global);
        if (n_global) {
            HIPCHK(c, hipMemcpy(gc.data(), dr_chars, gc.size(), hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(gl.data(), dr_len, gl.size() * 2, hipMemcpyDeviceToHost));
        }
        dr_chars = gc.data(); dr_len = gl.data();
    }
    c->premerge = 0; c->dm_prev_local = false;          // (multi-rank: nothing is queued ahead of the exchange)
    ensure_distinct(c);
    const bool dev = c->dev_tokens();
    const uint64_t my_nd = dev ? c->n_dx : c->dx_len.size();
    if (dev) { if (const int ds = c->wait_dx()) return ds; }
    const uint32_t *my_map = dev ? c->h_dmap.p : c->dx_map.data();
    const size_t my_n = dev ? (size_t)c->n_cand() : c->dx_map.size();
    if (my_offset + my_nd > n_global) {
        if (getenv("CRASS_GROUP_DEBUG")) fprintf(stderr, "[crass_xchg] merge_global_host: offset %llu + own %llu > global %llu (dev %d)\n",
                                                 (unsigned long long)my_offset, (unsigned long long)my_nd, (unsigned long long)n_global, (int)dev);
        return CRASS_ERR_INVALID_ARG;
    }
    merge_candidates(c->merge, dr_chars, dr_len, dr_stride, n_global, c->prm.kmer_clust_size);
    // tokens of this context's own candidates through their distinct index
    std::vector<uint32_t> own(my_n);
    for (size_t k = 0; k < own.size(); k++) own[k] = c->merge.cand_token[my_offset + my_map[k]];
    c->merge.cand_token.swap(own);
    return finish_merge(c, t0);
}

// host merge after all (the device path reported a condition it does not handle)
int host_merge_fallback(crass_hip_ctx *c)
{
    quiesce_worker(c);
    c->n_merge_fallbacks++;                             // (reported by crass_hip_get_counters: a silent latency cliff otherwise)
    c->last_fallback_bits = c->dm.h_st.p ? c->dm.h_st.p->fail : 0u;
    c->dm.active = false;
    c->cnt.used_device_merge = 0;
    c->dm_prev_local = false;                           // (no merge is queued ahead of time after a device-side failure)
    const double t0 = now_ms();
    if (c->dm.global)                                   // (the concatenated list is still on the device)
        return merge_global_host(c, c->dm.g_chars.p, c->dm.g_len.p, true, c->dr_stride, c->dm.n_global, c->dm.my_off, t0);
    if (const int ds = ensure_host_distinct(c, true)) return ds;
    if (!merge_from_distinct(c->merge, c->h_dx_chars.p, c->h_dx_len.p, c->h_dx_hash.p, c->dr_stride, c->n_dx, c->h_dmap.p, c->n_cand(),
                             c->prm.kmer_clust_size))
        merge_candidates(c->merge, c->cand_dr(), c->cand_dr_len(), c->dr_stride, c->n_cand(), c->prm.kmer_clust_size);
    return finish_merge(c, t0);
}

// what every merge entry point opens with: a deferred pass 1 settled (crass_hip_merge_gathered finishes one itself, behind what
// it queues), its results there where the call needs them, the helper thread idle, no device merge adopted.  *t0: ms_merge_host's start
static int open_merge(crass_hip_ctx *c, bool settle, bool need_pass1, double *t0)
{
    if (settle && c->p1d.active) { const int ds = settle_p1(c); if (ds) return ds; }
    if (need_pass1 && !c->have_pass1) return CRASS_ERR_STATE;
    *t0 = now_ms();
    quiesce_worker(c);
    c->dm.active = false;
    c->cnt.used_device_merge = 0; c->cnt.ms_merge_device = 0;
    (void)hipSetDevice(c->device);
    return CRASS_OK;
}

// ... and ends with when the merge runs on the device
static int merged_on_device(crass_hip_ctx *c, double t0) { c->cnt.used_device_merge = 1; c->cnt.ms_merge_host = (float)(now_ms() - t0); return CRASS_OK; }

int crass_hip_merge(crass_hip_ctx *c, const char *dr_chars, const uint16_t *dr_len, uint32_t dr_stride, uint64_t n)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    double t0 = 0;
    if (const int os = open_merge(c, true, false, &t0)) return os;
    const bool adopt = !dr_chars && c->premerge == 2;
    c->premerge = 0;
    if (!dr_chars && device_merge_applies(c)) {
        c->dm.global = false;
        int s = !c->n_dx ? CRASS_ERR_STATE
                : adopt  ? device_merge_commit(c, c->n_dx, c->h_dx_chars.p, c->h_dx_len.p)        // queued by the seed scan
                         : device_merge(c, c->dd_dx_chars.p, c->dd_dx_len.p, c->n_dx, c->h_dx_chars.p, c->h_dx_len.p);
        if (s == CRASS_ERR_STATE) goto host_path;
        if (s == CRASS_OK) {
            // the merge kernels are already running: the pass-1 hand-off pack (PCIe bound) goes beside them — small,
            // latency-bound kernels — rather than beside the pass-2 filter, which it would slow down
            c->dm_prev_local = true;
            c->dx_cap_hint = (uint32_t)distinct_bound(c->n_dx);
            return merged_on_device(c, t0);
        }
        return s;
    }
host_path:
    c->dm_prev_local = false;
    if (!dr_chars && c->have_pass1 && c->dev_tokens()) { if (const int ds = ensure_host_distinct(c, true)) return ds; }
    if (!dr_chars && c->have_pass1 && c->dev_tokens() &&
        merge_from_distinct(c->merge, c->h_dx_chars.p, c->h_dx_len.p, c->h_dx_hash.p, c->dr_stride, c->n_dx, c->h_dmap.p, c->n_cand(),
                            c->prm.kmer_clust_size))
        return finish_merge(c, t0);
    if (!dr_chars) {
        if (!c->have_pass1) return CRASS_ERR_STATE;
        dr_chars = c->cand_dr(); dr_len = c->cand_dr_len(); dr_stride = c->dr_stride; n = c->n_cand();
    } else if (!dr_len || !dr_stride) return CRASS_ERR_INVALID_ARG;
    const bool own = (dr_chars == c->cand_dr());
    merge_candidates(c->merge, dr_chars, dr_len, dr_stride, n, c->prm.kmer_clust_size,
                     (own && c->have_rep && c->dense.active) ? c->h_rep.p : nullptr,
                     (own && c->have_rep && c->dense.active) ? c->h_hash.p : nullptr);
    return finish_merge(c, t0);
}

int crass_hip_get_distinct(crass_hip_ctx *c, crass_distinct *o)
{
    if (!c || !o) return CRASS_ERR_INVALID_ARG;
    if (c->p1d.active) { const int ds = settle_p1(c); if (ds) return ds; }
    if (!c->have_pass1) return CRASS_ERR_STATE;
    ensure_distinct(c);
    o->dr_stride = c->dr_stride;
    if (c->dev_tokens()) {
        if (const int ds = c->wait_dx()) return ds;
        o->n_distinct = c->n_dx; o->dr_len = c->h_dx_len.p; o->dr_chars = c->h_dx_chars.p;
        o->n_candidates = c->n_cand(); o->cand_distinct = c->h_dmap.p;
    } else {
        o->n_distinct = c->dx_len.size(); o->dr_len = c->dx_len.data(); o->dr_chars = c->dx_chars.data();
        o->n_candidates = c->dx_map.size(); o->cand_distinct = c->dx_map.data();
    }
    return CRASS_OK;
}

// every buffer a global merge touches for a concatenation of up to n_max rows (the callers of merge_global_device have sized
// g_chars / g_len for theirs already: nothing moves under the copies they queued)
static int ensure_gathered_buffers(crass_hip_ctx *c, uint64_t n_max)
{
    crass_hip_ctx::DM &d = c->dm;
    const uint32_t stride = c->dr_stride, n = (uint32_t)n_max, tsize = dedupe_table_size(n);
    const uint64_t n_words = (n_max + 63) / 64;
    HIPCHK(c, d.g_chars.ensure(n_max * (size_t)stride + 16)); HIPCHK(c, d.g_len.ensure(n_max + 1));
    HIPCHK(c, d.g_keys.ensure(tsize)); HIPCHK(c, d.g_first.ensure(tsize)); HIPCHK(c, d.g_slot.ensure(n)); HIPCHK(c, d.g_rep.ensure(n));
    HIPCHK(c, d.g_hash.ensure(n)); HIPCHK(c, d.g_mask.ensure(n_words + 1)); HIPCHK(c, d.g_prefix.ensure(n_words + 1));
    HIPCHK(c, d.g_bsum.ensure((n_words + 255) / 256 + 2)); HIPCHK(c, d.g_idx.ensure(n));
    HIPCHK(c, d.gx_chars.ensure((size_t)n * stride + 16)); HIPCHK(c, d.gx_len.ensure(n));
    HIPCHK(c, d.h_gmap.ensure(n)); HIPCHK(c, d.h_gx_chars.ensure((size_t)n * stride + 16)); HIPCHK(c, d.h_gx_len.ensure(n)); HIPCHK(c, d.h_gx_hash.ensure(n));
    return CRASS_OK;
}

// The same on the device: de-duplicate the concatenation (first occurrence in rank order = global token order,
// the kernels of the single-GPU pass-1 tail), then the device merge over the global distinct list.  d_chars /
// d_len are device pointers owned by the engine (dm.g_chars / dm.g_len).  CRASS_ERR_STATE: not applicable,
// the caller merges on the host.
static int merge_global_device(crass_hip_ctx *c, uint64_t n_global, uint64_t my_offset)
{
    crass_hip_ctx::DM &d = c->dm;
    const uint32_t stride = c->dr_stride;
    c->premerge = 0; c->dm_prev_local = false;          // (multi-rank: nothing is queued ahead of the exchange)
    if (!device_merge_applies(c) || n_global == 0 || n_global > (1u << 22) || my_offset + c->n_dx > n_global) return CRASS_ERR_STATE;
    const uint32_t n = (uint32_t)n_global, tsize = dedupe_table_size(n);
    { const int as = ensure_gathered_buffers(c, n_global); if (as) return as; }
    // d_count[7] = n_global, [4] = distinct count, [5] = hash-collision flag
    c->h_count.p[7] = n;
    HIPCHK(c, hipMemcpyAsync(c->d_count.p + 7, c->h_count.p + 7, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_count.p + 4, 0, 8, c->stream));
    HIPCHK(c, launch_dr_dedupe(d.g_chars.p, d.g_len.p, stride, c->d_count.p + 7, n, d.g_keys.p, d.g_first.p, tsize, d.g_hash.p, d.g_slot.p,
                               d.g_rep.p, c->stream));
    HIPCHK(c, launch_dx_tokens(d.g_chars.p, d.g_len.p, d.g_hash.p, stride, c->d_count.p + 7, n, d.g_rep.p, d.g_slot.p, d.g_first.p, d.g_mask.p, d.g_prefix.p, d.g_bsum.p,
                               d.g_idx.p, c->d_count.p + 4, c->d_count.p + 5, d.h_gmap.p, d.h_gx_chars.p, d.h_gx_len.p, d.h_gx_hash.p,
                               d.gx_chars.p, d.gx_len.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_count.p + 4, c->d_count.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->h_count.p[5] != 0 || c->h_count.p[4] == 0 || c->h_count.p[4] > (1u << 20)) return CRASS_ERR_STATE;
    d.global = true; d.my_off = my_offset; d.n_global = n_global; d.hx_on_host = true;
    return device_merge(c, d.gx_chars.p, d.gx_len.p, c->h_count.p[4], d.h_gx_chars.p, d.h_gx_len.p);
}

int crass_hip_merge_distinct(crass_hip_ctx *c, const char *dr_chars, const uint16_t *dr_len, uint32_t dr_stride,
                             uint64_t n_global, uint64_t my_offset)
{
    if (!c || (n_global && (!dr_chars || !dr_len || !dr_stride))) return CRASS_ERR_INVALID_ARG;
    double t0 = 0;
    if (const int os = open_merge(c, true, true, &t0)) return os;
    if (dr_stride == c->dr_stride && n_global && n_global <= (1u << 22) && device_merge_applies(c)) {
        crass_hip_ctx::DM &d = c->dm;
        HIPCHK(c, d.g_chars.ensure(n_global * (size_t)dr_stride + 16)); HIPCHK(c, d.g_len.ensure(n_global + 1));
        HIPCHK(c, hipMemcpyAsync(d.g_chars.p, dr_chars, n_global * (size_t)dr_stride, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d.g_len.p, dr_len, n_global * 2, hipMemcpyHostToDevice, c->stream));
        const int s = merge_global_device(c, n_global, my_offset);
        if (s == CRASS_OK) return merged_on_device(c, t0);
        if (s != CRASS_ERR_STATE) return s;
        HIPCHK(c, hipStreamSynchronize(c->stream));                 // (the uploads read the caller's buffers)
        c->dm.global = false;
    }
    return merge_global_host(c, dr_chars, dr_len, false, dr_stride, n_global, my_offset, t0);
}

int crass_hip_exchange_setup(crass_hip_ctx *c, uint32_t world, uint32_t rank, uint64_t cap_rows, crass_exchange *o)
{
    if (!c || !o || world == 0 || rank >= world || cap_rows == 0 || cap_rows > (1u << 22)) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    crass_hip_ctx::Xchg &X = c->xchg;
    static const bool dbg = getenv("CRASS_GROUP_DEBUG") != nullptr;
#define XDBG(msg) do { if (dbg) { fprintf(stderr, "[crass_xchg] rank %u: %s\n", rank, msg); fflush(stderr); } } while (0)
    XDBG("setup: quiesce");
    quiesce_worker(c);
    c->p1d.active = false;                              // (a deferred pass 1 nobody finished: dropped; the stream is waited for below)
    XDBG("setup: stream sync");
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (kernels of an abandoned queued merge may still be running on the old buffers)
    X.world = world; X.rank = rank; X.cap = cap_rows; X.slot = c->dr_stride + 16; X.needed = 0;
    XDBG("setup: send buffer");
    HIPCHK(c, X.send.ensure(X.send_bytes())); HIPCHK(c, X.xinfo.ensure(8)); HIPCHK(c, X.h_xinfo.ensure(8));
    XDBG("setup: memset");
    HIPCHK(c, hipMemsetAsync(X.send.p, 0, X.send_bytes(), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    XDBG("setup: send buffer ready");
    X.active = true;
    X.gx_cap_hint = 0;
    // first call (see first_call_bounds): a bound for the GLOBAL distinct list from the job's size (every rank holds ~1/world
    // of the reads), and the buffers of crass_hip_merge_gathered sized now rather than inside the first step
    if (c->have_reads && c->surv_cap_hint && c->dx_cap_hint && !c->env.no_presize && !c->env.no_speculation) {
        const uint64_t n_max = (uint64_t)world * cap_rows;
        const uint64_t n_job = (uint64_t)world * c->R.n_reads;
        uint64_t gx = std::min<uint64_t>(std::min<uint64_t>(n_max, 1u << 20), std::max<uint64_t>(16384, (n_job / 1024 + 4095) & ~4095ull));
        if (c->env.test_bounds[3]) gx = std::min<uint64_t>(n_max, std::max<uint64_t>(16, c->env.test_bounds[3]));
        if (n_max <= (1u << 22)) {
            int s = ensure_gathered_buffers(c, n_max);
            if (s) return s;
            s = device_merge_prepare(c, c->dm.gx_chars.p, c->dm.gx_len.p, gx, c->d_count.p + 4);
            if (s) return s;
            X.gx_cap_hint = (uint32_t)gx;
        }
    }
    XDBG("setup: done");
#undef XDBG
    o->d_send = X.send.p; o->send_bytes = X.send_bytes(); o->slot_bytes = X.slot; o->cap_rows = X.cap;
    return CRASS_OK;
}

uint64_t crass_hip_exchange_needed_rows(const crass_hip_ctx *c) { return c ? c->xchg.needed : 0; }

// first-call bound for a shard's distinct DR strings (first_call_bounds_impl uses the same one for the queued merge)
static uint64_t distinct_bound_for(uint64_t n_reads)
{
    return std::min<uint64_t>(1u << 20, std::max<uint64_t>(16384, (n_reads / 1024 + 4095) & ~4095ull));
}
uint64_t crass_hip_exchange_rows_for(uint64_t n_reads) { return distinct_bound_for(n_reads); }

int crass_hip_merge_gathered(crass_hip_ctx *c, const void *d_recv)
{
    if (!c || !d_recv) return CRASS_ERR_INVALID_ARG;
    const bool deferred = c->p1d.active;                // pass 1 is still running (or its counters unread): p1_finish below
    if ((!c->have_pass1 && !deferred) || !c->xchg.active) return CRASS_ERR_STATE;
    double t0 = 0;
    auto lap = [&](const char *what) { if (c->env.merge_profile) fprintf(stderr, "[crass_xg] %-28s +%.1f us\n", what, 1e3 * (now_ms() - t0)); };
    crass_hip_ctx::Xchg &X = c->xchg;
    crass_hip_ctx::DM &d = c->dm;
    (void)open_merge(c, false, false, &t0);             // (nothing to settle: it cannot fail)
    lap("quiesced");
    const uint32_t stride = c->dr_stride;
    const uint64_t n_max = X.world * X.cap;
    const uint32_t n = (uint32_t)n_max;
    HIPCHK(c, d.g_chars.ensure(n_max * (size_t)stride + 16)); HIPCHK(c, d.g_len.ensure(n_max + 1));
    // (deferred: what device_merge_applies asks of pass 1's results is checked once they are known)
    bool dev = (deferred ? (!c->env.host_merge && c->prm.lowDRsize >= (int)kDevMinDR && c->dr_stride <= 64) : device_merge_applies(c)) && n_max <= (1u << 22);
    const uint32_t tsize = dedupe_table_size(n);
    if (dev) { const int as = ensure_gathered_buffers(c, n_max); if (as) return as; }
    lap("buffers ensured");
    HIPCHK(c, launch_xg_unpack((const uint8_t *)d_recv, X.world, X.rank, stride, X.cap, X.slot, d.g_chars.p, d.g_len.p, X.xinfo.p, c->stream,
                               X.h_xinfo.p, c->d_count.p + 4,        // (the four counters also land in pinned host memory: no copy call;
                                                                     //  d_count[4..5] = the de-duplication's counters, cleared on the way)
                               dev ? d.g_keys.p : nullptr, dev ? d.g_first.p : nullptr, tsize));      // (... and its table)
    lap("unpack queued");
    if (dev) {
        // the global count lives on the device (xinfo[0]); n_max bounds it
        HIPCHK(c, launch_dr_dedupe(d.g_chars.p, d.g_len.p, stride, X.xinfo.p, n, d.g_keys.p, d.g_first.p, tsize, d.g_hash.p, d.g_slot.p, d.g_rep.p,
                                   c->stream, true));
        Lookback lbg;
        // the global list's pinned copy is only read by the host-built view (3.7 MB of PCIe stores from the gather kernel at
        // 42 k tokens: 53 us); with the view exported by the device, or a light view, it stays on the device (fetch_host_list)
        d.hx_on_host = c->env.no_device_view && !c->host_view_light;
        HIPCHK(c, launch_dx_tokens(d.g_chars.p, d.g_len.p, d.g_hash.p, stride, X.xinfo.p, n, d.g_rep.p, d.g_slot.p, d.g_first.p, d.g_mask.p, d.g_prefix.p, d.g_bsum.p,
                                   d.g_idx.p, c->d_count.p + 4, c->d_count.p + 5, d.h_gmap.p, d.hx_on_host ? d.h_gx_chars.p : nullptr,
                                   d.hx_on_host ? d.h_gx_len.p : nullptr, d.hx_on_host ? d.h_gx_hash.p : nullptr,
                                   d.gx_chars.p, d.gx_len.p, c->stream,
                                   c->d_count.p, c->h_count.p, 8, c->next_lookback_tiles(((uint64_t)n + 1023) / 1024, &lbg)));   // counters leave with the last kernel
    }
    // As in the seed scan of the one-GPU path: when the previous step's merge ran on the device, this step's merge is
    // queued right here (token count read on the device, sized by a bound) and the host only waits for the counters.
    lap("de-duplication queued");
    bool queued = false;
    if (dev && X.gx_cap_hint && X.gx_cap_hint <= n_max && !c->env.no_speculation) {
        if (!c->poll_on) {
            if (!X.ev_counts) HIPCHK(c, hipEventCreateWithFlags(&X.ev_counts, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(X.ev_counts, c->stream));
        }
        const bool prepared = c->dm_prepared_n == X.gx_cap_hint && c->dm_prepared_src == d.gx_chars.p;
        c->dm_prepared_n = 0;                               // (a repeated exchange after an overflow starts from scratch)
        const int qs = device_merge_enqueue(c, d.gx_chars.p, d.gx_len.p, X.gx_cap_hint, c->d_count.p + 4, prepared);
        if (qs) return qs;
        queued = true;
        lap("merge queued");
    }
    if (deferred) {
        // everything of this step up to the merge is queued: now the host looks at pass 1
        const int fs = p1_finish(c);
        lap("pass 1 finished");
        if (fs == kP1Redo) { X.needed = 1; X.gx_cap_hint = 0; return CRASS_ERR_OVERFLOW; }      // (every rank finds the mark in what it gathered)
        if (fs) return fs;
        if (dev && !device_merge_applies(c)) {          // (no device-resident distinct list after all, e.g. no candidate in this shard)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            dev = false; queued = false;
        }
    }
    if (queued && !c->poll_on) HIPCHK(c, hipEventSynchronize(X.ev_counts));
    else if (!(queued && c->poll_flag(1, c->want_pre, 200.0))) HIPCHK(c, hipStreamSynchronize(c->stream));      // (the merge's first kernel stores the flag)
    lap("counts on the host");
    const uint64_t n_global = X.h_xinfo.p[0], my_off = X.h_xinfo.p[1];
    if (X.h_xinfo.p[2]) { X.needed = X.h_xinfo.p[3]; X.gx_cap_hint = 0; return CRASS_ERR_OVERFLOW; }
    if (dev && n_global && c->h_count.p[5] == 0 && c->h_count.p[4] != 0 && c->h_count.p[4] <= (1u << 20) && my_off + c->n_dx <= n_global) {
        d.global = true; d.my_off = my_off; d.n_global = n_global;
        const uint32_t n_tok = c->h_count.p[4];
        if (queued && n_tok > X.gx_cap_hint) c->n_bound_overflows[3]++;
        const int s = (queued && n_tok <= X.gx_cap_hint) ? device_merge_commit(c, n_tok, d.h_gx_chars.p, d.h_gx_len.p)
                                                         : device_merge(c, d.gx_chars.p, d.gx_len.p, n_tok, d.h_gx_chars.p, d.h_gx_len.p);
        lap("committed");
        if (s == CRASS_OK) {
            X.gx_cap_hint = (uint32_t)std::min<uint64_t>(n_max, distinct_bound(n_tok));
            return merged_on_device(c, t0);
        }
        if (s != CRASS_ERR_STATE) return s;
    }
    X.gx_cap_hint = 0;
    d.global = false;
    return merge_global_host(c, d.g_chars.p, d.g_len.p, true, stride, n_global, my_off, t0);
}

int crass_hip_get_distinct_device(crass_hip_ctx *c, crass_distinct_dev *o)
{
    if (!c || !o) return CRASS_ERR_INVALID_ARG;
    if (c->p1d.active) { const int ds = settle_p1(c); if (ds) return ds; }
    if (!c->have_pass1 || !c->dev_tokens()) return CRASS_ERR_STATE;
    o->n_distinct = c->n_dx; o->dr_stride = c->dr_stride; o->d_chars = c->dd_dx_chars.p; o->d_len = c->dd_dx_len.p;
    return CRASS_OK;
}

int crass_hip_merge_distinct_device(crass_hip_ctx *c, const char *d_chars, const uint16_t *d_len, uint32_t dr_stride,
                                    uint64_t n_global, uint64_t my_offset)
{
    if (!c || (n_global && (!d_chars || !d_len || !dr_stride))) return CRASS_ERR_INVALID_ARG;
    if (dr_stride != c->dr_stride) return CRASS_ERR_INVALID_ARG;
    double t0 = 0;
    if (const int os = open_merge(c, true, true, &t0)) return os;
    crass_hip_ctx::DM &d = c->dm;
    // engine-owned copy of the concatenation (the caller's buffers belong to its own stream and allocator)
    HIPCHK(c, d.g_chars.ensure(n_global * (size_t)dr_stride + 16)); HIPCHK(c, d.g_len.ensure(n_global + 1));
    if (n_global) {
        HIPCHK(c, hipMemcpyAsync(d.g_chars.p, d_chars, n_global * (size_t)dr_stride, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d.g_len.p, d_len, n_global * 2, hipMemcpyDeviceToDevice, c->stream));
    }
    int s = merge_global_device(c, n_global, my_offset);
    if (s == CRASS_OK) return merged_on_device(c, t0);
    if (s != CRASS_ERR_STATE) return s;
    // host merge after all
    c->dm.global = false;
    if (n_global) HIPCHK(c, hipStreamSynchronize(c->stream));       // (the engine's copy was queued on the stream)
    return merge_global_host(c, d.g_chars.p, d.g_len.p, true, dr_stride, n_global, my_offset, t0);
}

int crass_hip_get_merge(const crass_hip_ctx *c, crass_merge_view *o)
{
    if (!c || !o) return CRASS_ERR_INVALID_ARG;
    if (!c->have_merge) return CRASS_ERR_STATE;
    if (c->dm.active && !c->dm.host_built) {
        crass_hip_ctx *mc = const_cast<crass_hip_ctx *>(c);
        int s = ensure_host_merge(mc);
        if (s == CRASS_ERR_STATE) s = host_merge_fallback(mc);
        if (s) return s;
    }
    if (c->dm.active && c->dm.view_ready) {
        // the arrays the device assembled (k_dmx_*), where the DMA engine put them; the candidates' tokens are the host's
        const DevViewTotals &T = c->dm.view_tot;
        const uint8_t *b = c->dm.h_view.p;
        o->n_tokens = T.n_tok; o->tok_chars = (const char *)(b + T.lay.tok_chars); o->tok_off = (const uint64_t *)(b + T.lay.tok_off);
        o->n_candidates = c->merge.cand_token.size(); o->cand_token = c->merge.cand_token.data();
        o->n_groups = T.n_groups; o->grp_tokens = (const uint32_t *)(b + T.lay.grp_tokens); o->grp_off = (const uint64_t *)(b + T.lay.grp_off);
        o->n_patterns = 2u * T.n_kept; o->pat_chars = (const char *)(b + T.lay.pat_chars); o->pat_off = (const uint64_t *)(b + T.lay.pat_off);
        o->pat_group = (const uint32_t *)(b + T.lay.pat_group); o->next_free_gid = (int32_t)T.n_groups + 1;
        return CRASS_OK;
    }
    const MergeResult &m = c->merge;
    o->n_tokens = m.tokens.size(); o->tok_chars = m.tokens.strings.chars.data(); o->tok_off = m.tokens.strings.off.data();
    o->n_candidates = m.cand_token.size(); o->cand_token = m.cand_token.data();
    o->n_groups = (uint32_t)m.groups.size(); o->grp_tokens = m.grp_tokens.data(); o->grp_off = m.grp_off.data();
    o->n_patterns = (uint32_t)m.patterns.size(); o->pat_chars = m.patterns.chars.data(); o->pat_off = m.patterns.off.data();
    o->pat_group = m.pat_group.data(); o->next_free_gid = m.next_free_gid;
    return CRASS_OK;
}

} // extern "C"

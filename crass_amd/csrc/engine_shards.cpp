// engine_shards.cpp — one rank's shard of a group's files load (fastx_shards.h; the group's threads and barriers are
// group.cpp's, the load's steps group_files.cpp's): the cut probe, then the three steps stage and probe, complete and scan, pack; for a class-1 group's wrapped pass
// the chain of a piece in place of its probe (k_fw_cut_*, fastx_wrapped.hip) and what the host's walk over the ranks asks of it.  The scan and what makes its
// arena the resident set are engine_fastx.cpp's (ArenaScan, arena_finish), the members of a text range and the staging
// placement fastx_scan.cpp's.
#include "ingest_internal.h"
#include "gunzip_ranges.h"

// the probe of a range that lies on the device: launch, the blocks' parts back, folded in block order
static int probe_impl(crass_hip_ctx *c, const uint8_t *d, uint64_t n, bool left_is_ls, FxProbe *out)
{
    Ingest &I = c->in;
    FxProbe none{};
    none.gt = kFxNone;
    for (auto &x : none.ls) x = kFxNone;
    *out = none;
    I.last_probe_ms = 0;
    if (!n) return CRASS_OK;
    FxProbeJob P;
    fx_probe_plan(d, n, left_is_ls ? 1u : 0u, &P);
    HIPCHK(c, I.sh_part.ensure(P.n_blocks)); HIPCHK(c, I.sh_h_part.ensure(P.n_blocks));
    P.part = I.sh_part.p;
    HIPCHK(c, I.tm_probe.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_fx_cut_probe(P, c->stream));
    HIPCHK(c, I.tm_probe.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(I.sh_h_part.p, I.sh_part.p, P.n_blocks * sizeof(FxProbe), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_probe.elapsed(0, 1, &I.last_probe_ms));
    fx_probe_fold(I.sh_h_part.p, P.n_blocks, out);
    return CRASS_OK;
}

extern "C" int crass_hip_fastx_cut_probe_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, int left_is_ls, uint64_t out[7])
{
    if (!c || !out || (n_bytes && !d_bytes)) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    FxProbe P;
    const int s = probe_impl(c, d_bytes, n_bytes, left_is_ls != 0, &P);
    wait_main(c); c->in.sh_part.release();
    if (s) return s;
    out[0] = P.n_nl; out[1] = P.n_ls; for (int k = 0; k < 4; k++) out[2 + k] = P.ls[k]; out[6] = P.gt;
    return CRASS_OK;
}

extern "C" float crass_hip_last_cut_probe_ms(const crass_hip_ctx *c) { return c ? c->in.last_probe_ms : 0.0f; }
extern "C" float crass_hip_last_cut_chain_ms(const crass_hip_ctx *c) { return c ? c->in.cut_ms : 0.0f; }

// the parts of files that the range [lo, hi) of the text space holds, in order: (file, [a, b)), none of them empty
namespace {
struct Slice { uint32_t f; uint64_t a, b; };
}
static std::vector<Slice> shard_slices(const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi)
{
    std::vector<Slice> sl;
    for (uint32_t f = lo.file; f <= hi.file && f < n_files; f++) {
        const uint64_t a = f == lo.file ? lo.pos : 0, b = f == hi.file ? hi.pos : files[f].n_text;
        if (a < b) sl.push_back(Slice{f, a, b});
    }
    return sl;
}

// the members [m0, m1) of a host file inflated so that text position t lies at text0 + t: the compressed bytes up into z_raw
// (a plain gzip file: its elements, from what the rank keeps of the file and a seeded window walk behind it, gzip_kept_inflate)
static int shard_inflate(crass_hip_ctx *c, const ShardFile &F, uint64_t m0, uint64_t m1, uint8_t *text0, crass_bgzf_verdict *bv)
{
    if (F.gz) return gzip_kept_inflate(c, *F.gz, m0, m1, text0, bv);
    c->in.gzr_file = nullptr;                           // (z_raw is this inflate's now)
    const uint64_t z0 = F.ix->in_off[m0], z1 = F.ix->in_off[m1];
    HIPCHK(c, c->in.z_raw.ensure(z1 - z0 + 16));
    const int up = upload_staged(c, F.bytes + z0, z1 - z0, c->in.z_raw.p);
    if (up) return up;
    // (waits for the stream before it returns: z_raw may be used again)
    return inflate_bgzf_members(c, reinterpret_cast<const uint8_t *>((uintptr_t)c->in.z_raw.p - z0), F.ix, m0, m1 - m0, text0, bv);
}

// the line table and the chain of a wrapped-mode piece whose bytes [a, se) lie at K.bytes: k_fw_summary / k_fw_tile_scan, the line
// count back, then k_fw_lines / k_fw_cut_next / the k_fw_cut_jump rounds.  Look-ups follow on the same stream
static int shard_cut_build(crass_hip_ctx *c, Ingest::ShardCut &K, uint64_t n_text)
{
    Ingest &I = c->in;
    FwJob &J = K.J;
    J = FwJob{};
    J.bytes = K.bytes; J.n = K.se - K.a; J.lead = (uint32_t)((uintptr_t)K.bytes & 15u);
    J.n_tiles = fastx_n_tiles(J.bytes, J.n);
    uint8_t last = 0;
    HIPCHK(c, hipMemcpyAsync(&last, K.bytes + J.n - 1, 1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    J.ends_nl = fx_is_nl(last) ? 1u : 0u;
    const bool timed = c->timing_level >= 1;
    for (hipEvent_t &e : I.ev_cut) if (timed && !e) HIPCHK(c, hipEventCreate(&e));
    if (timed) HIPCHK(c, hipEventRecord(I.ev_cut[0], c->stream));
    // the tiles first, in a scratch without lines: their count sizes the rest, and what the tiles left moves over
    DevBuf<uint64_t> head;
    const uint64_t head_words = fw_scratch_words(J.n_tiles, 0);
    HIPCHK(c, head.ensure(head_words));
    fw_lay_out(J, head.p);
    uint64_t n_lines = 0;
    hipError_t e = launch_fw_tiles(J, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_lines, J.tot, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && n_lines < 0xFFFFFFFFull) {
        J.n_lines = (uint32_t)n_lines;
        e = K.scratch.ensure(fw_scratch_words(J.n_tiles, n_lines));
        if (e == hipSuccess) e = hipMemcpyAsync(K.scratch.p, head.p, head_words * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    head.release();
    HIPCHK(c, e);
    if (n_lines >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (line indices are 32-bit, END is one of them)
    fw_lay_out(J, K.scratch.p);
    FwCut Q{K.b - K.a, K.se == n_text ? 1u : 0u, K.left_is_ls ? 0u : 1u};
    HIPCHK(c, launch_fw_cut(J, Q, c->stream, &K.which));
    if (timed) {
        float ms = 0;
        HIPCHK(c, hipEventRecord(I.ev_cut[1], c->stream));
        HIPCHK(c, hipEventSynchronize(I.ev_cut[1]));
        HIPCHK(c, hipEventElapsedTime(&ms, I.ev_cut[0], I.ev_cut[1]));
        I.cut_ms += ms;
    }
    return CRASS_OK;
}

// the piece with twice the margin (more where whole BGZF members had brought more already): what is staged of it moves device to
// device into a buffer of its own, only the extra bytes [se, se') come up — plain bytes from the host, of a BGZF file the
// further members —, then its table and chain anew.  K.se < the file's text length
static int shard_cut_grow(crass_hip_ctx *c, const ShardFile &F, Ingest::ShardCut &K)
{
    Ingest &I = c->in;
    do K.margin *= 2; while (K.b + K.margin > K.b && K.b + K.margin <= K.se);
    const uint64_t want = K.b + K.margin < K.b ? F.n_text : std::min(F.n_text, K.b + K.margin);
    K.scratch.release();
    DevBuf<uint8_t> grown;
    auto run = [&]() -> int {
        uint64_t t0 = K.se, t1 = want;                  // the extra text; of a BGZF file whole members: [t0, t1) with t0 <= se
        uint64_t m0 = 0, m1 = 0;
        if (F.ix) { bgzf_members_for(F.ix->out_off, F.ix->n_members, K.se, want, &m0, &m1); t0 = F.ix->out_off[m0]; t1 = F.ix->out_off[m1]; }
        HIPCHK(c, grown.ensure(t1 - K.a + 48));
        uint8_t *dst = grown.p + (K.a & 15u);           // (aligned as its text is, as shard_stage_place puts it)
        HIPCHK(c, hipMemcpyAsync(dst, K.bytes, K.se - K.a, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));      // (the pinned staging buffers are the upload before's until its last copy is done)
        if (F.ix) {
            HIPCHK(c, I.sh_tail.ensure(t1 - t0 + 16));
            crass_bgzf_verdict bv{};
            const int s = shard_inflate(c, F, m0, m1, reinterpret_cast<uint8_t *>((uintptr_t)I.sh_tail.p - t0), &bv);
            // (never expected: every member of the file inflated in step 1.  A gzip file's grown elements were narrowed before the
            // load's steps by the rank whose piece holds them; a marker there is the file's pending decline, and a declined file
            // is not chained)
            if (s) return s == CRASS_ERR_UNSUPPORTED ? CRASS_ERR_STATE : s;
            HIPCHK(c, hipMemcpyAsync(dst + (K.se - K.a), I.sh_tail.p + (K.se - t0), t1 - K.se, hipMemcpyDeviceToDevice, c->stream));
        } else {
            const int up = upload_staged(c, F.bytes + K.se, t1 - K.se, dst + (K.se - K.a));
            if (up) return up;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));     // (the bytes moved: their old place and sh_tail may be used again)
        K.text.release();
        K.text = grown; grown = DevBuf<uint8_t>();
        K.bytes = dst; K.se = t1;
        return CRASS_OK;
    };
    const int s = run();
    grown.release();
    if (s) return s;
    I.cut_doublings++;
    return shard_cut_build(c, K, F.n_text);
}

int shard_cut_exit(crass_hip_ctx *c, const ShardFile *files, uint32_t file, uint64_t e, uint32_t *kind, uint64_t *pos, uint64_t *off)
{
    if (!c || !files || !kind || !pos || !off) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    Ingest::ShardCut *K = nullptr;
    for (auto &k : I.sh_cut) if (k.file == file && e >= k.a && e < k.b) K = &k;
    if (!K) return CRASS_ERR_STATE;
    HIPCHK(c, I.sh_cut_out.ensure(3)); HIPCHK(c, I.sh_h_cut_out.ensure(3));
    for (;;) {
        HIPCHK(c, launch_fw_cut_lookup(K->J, K->which, e - K->a, I.sh_cut_out.p, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.sh_h_cut_out.p, I.sh_cut_out.p, 24, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        I.cut_lookups++;
        const uint64_t *h = I.sh_h_cut_out.p;
        if (h[0] != FW_CUT_UNRESOLVED) {
            *kind = (uint32_t)h[0];
            *pos = h[0] == FW_CUT_LANDED ? K->a + h[1] : 0;
            *off = h[0] == FW_CUT_OFFENCE ? fx_offence((h[2] >> 8) + K->a, (uint32_t)(h[2] & 0xFF)) : kFxNoOffence;
            return h[0] == FW_CUT_LANDED || h[0] == FW_CUT_OFFENCE ? CRASS_OK : CRASS_ERR_STATE;
        }
        if (K->se >= files[file].n_text) return CRASS_ERR_STATE;      // (never expected: at the file's end nothing is open)
        try {
            const int s = shard_cut_grow(c, files[file], *K);
            if (s) return s;
        } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    }
}

void shard_cut_counters(const crass_hip_ctx *c, uint64_t *lookups, uint64_t *doublings, float *ms)
{
    if (lookups) *lookups = c ? c->in.cut_lookups : 0;
    if (doublings) *doublings = c ? c->in.cut_doublings : 0;
    if (ms) *ms = c ? c->in.cut_ms : 0.0f;
}

int shard_stage_probe(crass_hip_ctx *c, const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi, std::vector<ShardPiece> *pieces,
                      ShardVerdict *v, bool wrapped, uint64_t margin)
{
    if (!c || !files || !pieces || !v) return CRASS_ERR_INVALID_ARG;
    pieces->clear();
    *v = ShardVerdict();
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    release_shard(c);
    Ingest &I = c->in;
    I.cut_lookups = I.cut_doublings = 0; I.cut_ms = 0;
    if (margin == 0) margin = 1;
    try {
        // the pieces, the text each one stages ([sa, sb): of a BGZF file whole members) and their places in the staging buffer
        struct Plan { uint32_t f; uint64_t a, b, m0, m1; };
        std::vector<Plan> plan;
        std::vector<uint64_t> sas, sbs;
        for (const Slice &S : shard_slices(files, n_files, lo, hi)) {
            Plan p{S.f, S.a, S.b, 0, 0};
            // (a wrapped-mode piece: with the margin behind it, where a record that begins in the piece may end)
            const bool cut = wrapped && files[S.f].format == 0x40;
            uint64_t sa = S.a, sb = !cut ? S.b : S.b + margin < S.b ? files[S.f].n_text : std::min(files[S.f].n_text, S.b + margin);
            if (const crass_bgzf_index *ix = files[S.f].ix) {      // (with the byte in front of a: it says whether a is a line start)
                bgzf_members_for(ix->out_off, ix->n_members, S.a ? S.a - 1 : 0, sb, &p.m0, &p.m1);
                sa = ix->out_off[p.m0]; sb = ix->out_off[p.m1];
            }
            plan.push_back(p); sas.push_back(sa); sbs.push_back(sb);
        }
        std::vector<uint64_t> off(plan.size());
        HIPCHK(c, I.sh_stage.ensure(shard_stage_place(sas.data(), sbs.data(), plan.size(), off.data())));
        for (size_t k = 0; k < plan.size(); k++) {
            const Plan &p = plan[k];
            const uint64_t sa = sas[k], sb = sbs[k];
            const ShardFile &F = files[p.f];
            uint8_t *dst = I.sh_stage.p + off[k];       // text position sa
            if (k) HIPCHK(c, hipStreamSynchronize(c->copy_stream));      // (the staged buffers are the piece before's until its last copy is done)
            ShardPiece pc{};
            pc.file = p.f; pc.a = p.a; pc.b = p.b;
            if (F.ix) {
                crass_bgzf_verdict bv{};
                const int s = shard_inflate(c, F, p.m0, p.m1, reinterpret_cast<uint8_t *>((uintptr_t)dst - sa), &bv);
                if (s == CRASS_ERR_UNSUPPORTED) { v->file = (int32_t)p.f; v->bgzf = bv; break; }
                if (s) return s;
                uint8_t one = 0;
                HIPCHK(c, hipMemcpy(&one, dst + ((p.a ? p.a - 1 : 0) - sa), 1, hipMemcpyDeviceToHost));
                if (p.a == 0) {
                    pc.first_byte = one;
                    if (!fx_is_hdr_char(one)) { v->file = (int32_t)p.f; v->reason = FX_FIRST_BYTE; break; }
                }
                pc.left_is_ls = p.a == 0 || fx_is_nl(one);
            } else {
                const int up = upload_staged(c, F.bytes + p.a, sb - p.a, dst);
                if (up) return up;
                pc.left_is_ls = p.a == 0 || fx_is_nl(F.bytes[p.a - 1]);
                if (p.a == 0) pc.first_byte = F.bytes[0];
            }
            if (wrapped && F.format == 0x40) {
                Ingest::ShardCut K{};
                K.file = p.f; K.a = p.a; K.b = p.b; K.se = sb; K.margin = margin; K.left_is_ls = pc.left_is_ls; K.bytes = dst + (p.a - sa);
                I.sh_cut.push_back(K);
                const int cs = shard_cut_build(c, I.sh_cut.back(), F.n_text);
                if (cs) return cs;
            } else {
                const int ps = probe_impl(c, dst + (p.a - sa), p.b - p.a, pc.left_is_ls, &pc.probe);
                if (ps) return ps;
            }
            I.sh_staged.push_back(Ingest::ShardStaged{p.f, sa, sb, off[k]});
            pieces->push_back(pc);
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int shard_scan(crass_hip_ctx *c, const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi,
               std::vector<std::pair<uint32_t, uint64_t>> *file_reads, uint64_t *n_reads, uint32_t *max_len, ShardVerdict *v, bool wrapped)
{
    if (!c || !files || !file_reads || !n_reads || !max_len || !v) return CRASS_ERR_INVALID_ARG;
    *n_reads = 0; *max_len = 0; *v = ShardVerdict();
    file_reads->clear();
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    for (auto &k : I.sh_cut) { k.scratch.release(); k.text.release(); }      // (the chain is done: every look-up was waited for)
    I.sh_cut.clear();
    try {
        const std::vector<Slice> sl = shard_slices(files, n_files, lo, hi);
        // the arena: the slices in order, a byte of room behind each
        std::vector<uint64_t> &base = I.sh_base;
        base.assign(1, 0);
        for (const Slice &S : sl) base.push_back(base.back() + (S.b - S.a) + 1);
        HIPCHK(c, I.fa_arena.ensure(base.back() + 16));
        uint8_t *arena = I.fa_arena.p;
        uint32_t ns = (uint32_t)sl.size();
        for (uint32_t i = 0; i < ns; i++) {
            const Slice &S = sl[i];
            const ShardFile &F = files[S.f];
            uint8_t *dst = arena + base[i];
            // what was staged of it comes device to device ...
            uint64_t have = S.a;                        // [S.a, have) is in place
            for (const Ingest::ShardStaged &st : I.sh_staged) {
                if (st.file != S.f || S.a < st.a || S.a >= st.b) continue;
                have = std::min(S.b, st.b);
                HIPCHK(c, hipMemcpyAsync(dst, I.sh_stage.p + st.off + (S.a - st.a), have - S.a, hipMemcpyDeviceToDevice, c->stream));
            }
            if (have == S.b) continue;
            // ... and the tail behind it from the host: plain bytes, or the further members
            HIPCHK(c, hipStreamSynchronize(c->copy_stream));
            if (F.ix) {
                uint64_t m0, m1;
                bgzf_members_for(F.ix->out_off, F.ix->n_members, have, S.b, &m0, &m1);
                const uint64_t t0 = F.ix->out_off[m0], t1 = F.ix->out_off[m1];
                HIPCHK(c, I.sh_tail.ensure(t1 - t0 + 16));
                crass_bgzf_verdict bv{};
                const int s = shard_inflate(c, F, m0, m1, reinterpret_cast<uint8_t *>((uintptr_t)I.sh_tail.p - t0), &bv);
                if (s == CRASS_ERR_UNSUPPORTED) { v->file = (int32_t)S.f; v->bgzf = bv; ns = i; break; }      // (the slices in front of it are still scanned)
                if (s) return s;
                HIPCHK(c, hipMemcpyAsync(dst + (have - S.a), I.sh_tail.p + (have - t0), S.b - have, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));      // (sh_tail may be used again)
            } else {
                const int up = upload_staged(c, F.bytes + have, S.b - have, dst + (have - S.a));
                if (up) return up;
            }
        }
        base.resize((size_t)ns + 1);
        I.sh_n_reads = 0;
        I.fa_read_base.assign(1, 0);
        if (ns == 0) { I.sh_scanned = v->file < 0; return CRASS_OK; }
        ArenaScan A;
        const int os = A.open(c, arena, base.data(), ns);
        if (os) return os;
        A.wrapped = wrapped;                            // (a wrapped-mode slice begins at a reachable record: the wrapped rule walks it from there)
        for (uint32_t i = 0; i < ns; i++) {
            // a slice is scanned as a file of its file's format: it begins at a record start, so its lines count from 0
            const int qs = A.queue(c, i, files[sl[i].f].format, true);
            if (qs) return qs;
        }
        ScanResult R;
        const int es = A.emit(c, ns, 0xFFFFFFFFull, R);
        if (es == CRASS_ERR_UNSUPPORTED && R.decline_file >= 0) {      // (in the FILE's positions)
            ShardVerdict sv;
            sv.file = (int32_t)sl[R.decline_file].f; sv.reason = R.decline_reason; sv.pos = R.decline_pos + sl[R.decline_file].a;
            if (shard_verdict_before(sv, *v)) *v = sv;
            return CRASS_OK;
        }
        if (es) return es;
        if (v->file >= 0) return CRASS_OK;
        for (uint32_t i = 0; i < ns; i++) file_reads->push_back(std::make_pair(sl[i].f, R.rbase[i + 1] - R.rbase[i]));
        *n_reads = R.n_reads; *max_len = (uint32_t)R.max_len;
        I.sh_n_reads = R.n_reads; I.sh_scanned = true;
        I.fa_read_base.assign(R.rbase.begin(), R.rbase.begin() + ns + 1);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

static void shard_release_all(crass_hip_ctx *c)
{
    release_gzip(c); release_bgzf(c); release_scan(c); release_text(c); release_header_ids(c); release_shard(c);
}

int shard_pack(crass_hip_ctx *c, int pad_uniform, uint64_t read_index_base)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    if (!I.sh_scanned) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    auto run = [&]() -> int {
        const uint64_t nr = I.sh_n_reads, n_arena = I.sh_base.empty() ? 0 : I.sh_base.back();
        HIPCHK(c, I.x_h_seq_off.ensure(1)); HIPCHK(c, I.x_h_rec_pos.ensure(1)); HIPCHK(c, I.fa_arena.ensure(16));
        if (!nr) { I.x_h_seq_off.p[0] = 0; I.x_h_rec_pos.p[0] = 0; }      // (an empty shard: no slice was scanned)
        const int s = arena_finish(c, I.fa_arena.p, n_arena, nr, pad_uniform, read_index_base);
        if (s) return s;
        return crass_hip_fastx_names_build_device(c, nullptr, 0, nullptr, 0);
    };
    const int s = run();
    shard_release_all(c);
    if (s) { c->have_reads = false; drop_arena(c); }
    else I.sh_loaded = true;
    return s;
}

void shard_abort(crass_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    shard_release_all(c);
    c->have_reads = false;
    drop_arena(c);
}

int shard_records(const crass_hip_ctx *c, const uint8_t **arena, uint64_t *n_bytes, const uint64_t **rec_pos, uint64_t *n_reads)
{
    if (!c || !arena || !n_bytes || !rec_pos || !n_reads) return CRASS_ERR_INVALID_ARG;
    if (!c->in.sh_loaded || !c->in.have_arena || !c->have_reads) return CRASS_ERR_STATE;
    *arena = c->in.fa_arena.p; *n_bytes = c->in.fa_bytes; *rec_pos = c->in.x_h_rec_pos.p; *n_reads = c->R.n_reads;
    return CRASS_OK;
}

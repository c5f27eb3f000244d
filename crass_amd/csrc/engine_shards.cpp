// engine_shards.cpp — one rank's shard of a group's files load (fastx_shards.h; the group's threads and barriers are
// group.cpp's): the cut probe, then the three steps stage and probe, complete and scan, pack.  The scan and what makes its
// arena the resident set are engine_fastx.cpp's (ArenaScan, arena_finish), the members of a text range and the staging
// placement fastx_scan.cpp's.
#include "ingest_internal.h"

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
static int shard_inflate(crass_hip_ctx *c, const ShardFile &F, uint64_t m0, uint64_t m1, uint8_t *text0, crass_bgzf_verdict *bv)
{
    const uint64_t z0 = F.ix->in_off[m0], z1 = F.ix->in_off[m1];
    HIPCHK(c, c->in.z_raw.ensure(z1 - z0 + 16));
    const int up = upload_staged(c, F.bytes + z0, z1 - z0, c->in.z_raw.p);
    if (up) return up;
    // (waits for the stream before it returns: z_raw may be used again)
    return inflate_bgzf_members(c, reinterpret_cast<const uint8_t *>((uintptr_t)c->in.z_raw.p - z0), F.ix, m0, m1 - m0, text0, bv);
}

int shard_stage_probe(crass_hip_ctx *c, const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi, std::vector<ShardPiece> *pieces,
                      ShardVerdict *v)
{
    if (!c || !files || !pieces || !v) return CRASS_ERR_INVALID_ARG;
    pieces->clear();
    *v = ShardVerdict();
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    release_shard(c);
    Ingest &I = c->in;
    try {
        // the pieces, the text each one stages ([sa, sb): of a BGZF file whole members) and their places in the staging buffer
        struct Plan { uint32_t f; uint64_t a, b, m0, m1; };
        std::vector<Plan> plan;
        std::vector<uint64_t> sas, sbs;
        for (const Slice &S : shard_slices(files, n_files, lo, hi)) {
            Plan p{S.f, S.a, S.b, 0, 0};
            uint64_t sa = S.a, sb = S.b;
            if (const crass_bgzf_index *ix = files[S.f].ix) {      // (with the byte in front of a: it says whether a is a line start)
                bgzf_members_for(ix->out_off, ix->n_members, S.a ? S.a - 1 : 0, S.b, &p.m0, &p.m1);
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
                const int up = upload_staged(c, F.bytes + p.a, p.b - p.a, dst);
                if (up) return up;
                pc.left_is_ls = p.a == 0 || fx_is_nl(F.bytes[p.a - 1]);
                if (p.a == 0) pc.first_byte = F.bytes[0];
            }
            const int ps = probe_impl(c, dst + (p.a - sa), p.b - p.a, pc.left_is_ls, &pc.probe);
            if (ps) return ps;
            I.sh_staged.push_back(Ingest::ShardStaged{p.f, sa, sb, off[k]});
            pieces->push_back(pc);
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int shard_scan(crass_hip_ctx *c, const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi,
               std::vector<std::pair<uint32_t, uint64_t>> *file_reads, uint64_t *n_reads, uint32_t *max_len, ShardVerdict *v)
{
    if (!c || !files || !file_reads || !n_reads || !max_len || !v) return CRASS_ERR_INVALID_ARG;
    *n_reads = 0; *max_len = 0; *v = ShardVerdict();
    file_reads->clear();
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
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

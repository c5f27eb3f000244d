// group_files.cpp — a files load of a group (crass_hip_group_load_fastx_files): the files of a job as record-aligned shards, one
// per rank.  One rank's three steps are fastx_shards.h's; here is what rank 0 combines between their barriers (the actual cuts,
// the verdict, whether a class-1 load runs once more by the wrapped rule), one rank's part of the job, and the call as its
// steps: classify the files and index the gzip ones, the nominal cuts, every gzip file inflated (group_gzip.cpp), the dispatch,
// the counters, the shards.
#include "group_internal.h"

using namespace grp;

namespace {

// the file and the position inside it of text-space position x, over the first nf files
crass::ShardPos locate(const std::vector<uint64_t> &tb, uint32_t nf, uint64_t x)
{
    if (x >= tb[nf]) return crass::ShardPos{nf, 0};
    const uint32_t f = (uint32_t)(std::upper_bound(tb.begin(), tb.begin() + nf + 1, x) - tb.begin()) - 1;
    return crass::ShardPos{f, x - tb[f]};
}

// rank 0, between two barriers: every rank's pieces are probed.  The actual cuts by the rule of fastx_scan.h: a nominal cut at a
// file's position 0 is a record start; else the cut's rank has probed the range that begins there — the '\n' bytes of that
// file in front of it are the sum over the ranks before —, and "none in my range" is the next file's position 0 where the
// range reaches its file's end, else the next rank's cut: resolved from the last rank down.
int combine_cuts(crass_hip_group *g)
{
    auto &J = g->F;
    const int N = g->n;
    // a decline that a rank met while staging: the files in front of it go on, it waits for their verdict
    for (int r = 0; r < N; r++) if (crass::shard_verdict_before(J.v_stage[r], J.pend)) J.pend = J.v_stage[r];
    if (crass::shard_verdict_before(g->GZ.v_gz, J.pend)) J.pend = g->GZ.v_gz;      // (a gzip file whose CRC-32 or markers failed before the load's steps)
    J.nf_eff = J.pend.file >= 0 ? (uint32_t)J.pend.file : J.nf;
    for (int r = 0; r < N; r++) for (const crass::ShardPiece &pc : J.pieces[r]) if (pc.a == 0 && J.files[pc.file].ix) J.files[pc.file].format = pc.first_byte;
    // the wrapped pass: every '@' file's chain over the ranks, in piece order.  A piece is entered at e, the exit of the one before
    // (0 for the file's first); a record longer than the piece passes through it.  exits[f]: the pieces' exits, not decreasing
    std::vector<std::vector<uint64_t>> exits(J.nf_eff);
    J.n_chained = 0;
    for (uint32_t f = 0; J.wrapped_pass && f < J.nf_eff; f++) {
        if (J.files[f].format != 0x40) continue;
        J.n_chained++;
        uint64_t e = 0;
        bool offended = false;
        for (int r = 0; r < N && !offended; r++) for (const crass::ShardPiece &pc : J.pieces[r]) {
            if (pc.file != f) continue;
            if (e < pc.b) {
                uint32_t kind = 0; uint64_t pos = 0, off = 0;
                const int s = shard_cut_exit(g->ctx[r], J.files.data(), f, e, &kind, &pos, &off);
                if (s) return s;
                if (kind == crass::FW_CUT_OFFENCE) {    // the file's verdict: nothing behind it in this file is cut
                    crass::ShardVerdict sv;
                    sv.file = (int32_t)f; sv.reason = (int32_t)(off & 0xFF); sv.pos = off >> 8;
                    if (crass::shard_verdict_before(sv, J.pend)) J.pend = sv;
                    offended = true;
                    break;
                }
                e = pos;
            }
            exits[f].push_back(e);
        }
        if (offended) break;                            // (the files behind it are out of the set)
    }
    J.nf_eff = J.pend.file >= 0 ? (uint32_t)J.pend.file : J.nf;
    const uint32_t nf = J.nf_eff;
    J.cut.assign(N + 1, crass::ShardPos{nf, 0});
    J.cut[0] = crass::ShardPos{0, 0};
    for (int k = N - 1; k >= 1; k--) {
        const crass::ShardPos x = locate(J.tb, nf, J.nom_x[k]);
        if (x.file >= nf || x.pos == 0) { J.cut[k] = x; continue; }
        if (J.wrapped_pass && J.files[x.file].format == 0x40) {      // the first exit at or after the nominal cut; the file's end: the next file's 0
            const std::vector<uint64_t> &ex = exits[x.file];
            const auto it = std::lower_bound(ex.begin(), ex.end(), x.pos);
            if (it == ex.end()) return CRASS_ERR_STATE;
            J.cut[k] = *it < J.files[x.file].n_text ? crass::ShardPos{x.file, *it} : crass::ShardPos{x.file + 1, 0};
            continue;
        }
        J.cut[k] = J.cut[k + 1];
        if (J.pieces[k].empty()) continue;              // (an empty nominal range: the next rank's cut)
        const crass::ShardPiece &pc = J.pieces[k][0];
        if (pc.file != x.file || pc.a != x.pos) return CRASS_ERR_STATE;
        uint64_t nl_before = 0;
        for (int q = 0; q < k; q++) for (const crass::ShardPiece &o : J.pieces[q]) if (o.file == x.file) nl_before += o.probe.n_nl;
        const uint64_t pick = crass::fx_probe_pick(pc.probe, J.files[x.file].format, nl_before, pc.left_is_ls);
        if (pick != crass::kFxNone) J.cut[k] = crass::ShardPos{x.file, x.pos + pick};
        else if (pc.b == J.files[x.file].n_text) J.cut[k] = crass::ShardPos{x.file + 1, 0};
    }
    return CRASS_OK;
}

// rank 0, between two barriers: every rank's slices are scanned.  The job's verdict, or every rank's first read and the
// exchange's row capacity from the largest shard (every rank must use the same one)
void finish_scan(crass_hip_group *g)
{
    auto &J = g->F;
    J.verdict = J.pend;
    for (int r = 0; r < g->n; r++) if (crass::shard_verdict_before(J.v_scan[r], J.verdict)) J.verdict = J.v_scan[r];
    J.declined = J.verdict.file >= 0;
    if (J.declined) return;
    J.rank_base.assign(g->n + 1, 0);
    uint64_t largest = 0;
    for (int r = 0; r < g->n; r++) { J.rank_base[r + 1] = J.rank_base[r] + J.n_reads[r]; largest = std::max(largest, J.n_reads[r]); }
    if (!g->cap_rows_forced) g->cap_rows = crass_hip_exchange_rows_for(largest);
}

// rank 0, behind finish_scan of a class-1 group's first attempt: a file whose format is '@', declined for its shape, is what
// the wrapped rule takes up — the load runs once more with every '@' file cut and scanned by that rule.  Any other decline is final
void decide_second_attempt(crass_hip_group *g)
{
    auto &J = g->F;
    if (g->fastq_class != crass::FX_CLASS_WRAPPED || !J.declined || J.verdict.bgzf.reason != 0) return;
    if (J.files[J.verdict.file].format != 0x40 || !crass::fx_wrapped_takes(J.verdict.reason)) return;
    J.attempts = 2; J.wrapped_pass = true;
    J.pend = J.pend0; J.verdict = crass::ShardVerdict(); J.declined = false;
}

// 1. what every file is and how much text it holds (host: first bytes, BGZF index; ixs[f]: a BGZF file's).  The first file that
// cannot be taken waits with its decline (J.pend, J.nf): a file in front of it may still offend in the scan.  Plain gzip with
// the switch on, the index step: every rank finds and counts its share of the chunks, rank 0 walks the chain.  The text's size
// and the element index (start bit, end bit, text offset of every chain element) are known before any cut; the index takes a
// BGZF index's place, elements for members
int files_classify(crass_hip_group *g, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, std::vector<crass_bgzf_index> &ixs)
{
    auto &J = g->F;
    auto &GJ = g->GZ;
    J.files.assign(n_files, crass::ShardFile{});
    J.nf = n_files;
    GJ.files.clear(); GJ.ix.clear(); GJ.ix_zero.clear(); GJ.ix.reserve(n_files);
    GJ.v_gz = crass::ShardVerdict();
    for (uint32_t f = 0; f < n_files; f++) {
        crass::ShardFile &F = J.files[f];
        F.bytes = bytes[f]; F.n_bytes = n_bytes[f];
        auto pend = [&](int32_t reason) { J.pend.file = (int32_t)f; J.pend.reason = reason; J.nf = f; };
        if (F.n_bytes >= 2 && F.bytes[0] == 0x1F && F.bytes[1] == 0x8B) {
            const int s = crass_bgzf_index_host(F.bytes, F.n_bytes, &ixs[f]);
            if (s == CRASS_ERR_UNSUPPORTED && g->gzip_mode && ixs[f].decline.reason == crass::BZ_NOT_BGZF) {
                GJ.files.emplace_back(new crass::GzRangesFile());
                crass::GzRangesFile &Z = *GJ.files.back();
                if (!gzip_file_init(Z, F.bytes, F.n_bytes, (uint32_t)g->n, g->gzip_chunk, g->gzip_mode == CRASS_GZIP_ON_DEVICE_MEMBERS)) { pend(0); J.pend.bgzf.reason = crass::BZ_NOT_GZIP; break; }
                const int zs = gzip_job_run(g, Z, true, false);
                if (zs) return zs;
                if (GJ.status == CRASS_ERR_UNSUPPORTED) { pend(0); J.pend.bgzf.reason = GJ.v.reason; J.pend.bgzf.member = GJ.v.member; J.pend.bgzf.in_pos = GJ.v.in_pos; break; }
                GJ.ix_zero.emplace_back(Z.n_chain + 1, 0);
                crass_bgzf_index X{};
                X.n_members = Z.n_chain; X.out_off = Z.off.data(); X.in_off = X.data_off = GJ.ix_zero.back().data();
                GJ.ix.push_back(X);                     // (reserved for n_files: the pointers below stay)
                F.ix = &GJ.ix.back(); F.gz = &Z; F.n_text = Z.n_text;
                if (F.n_text == 0) { pend(crass::FX_EMPTY); break; }
                continue;
            }
            if (s == CRASS_ERR_UNSUPPORTED) { pend(0); J.pend.bgzf = ixs[f].decline; break; }      // (plain gzip with the switch off: declined)
            if (s) return s;
            F.ix = &ixs[f]; F.n_text = ixs[f].out_off[ixs[f].n_members];
            if (F.n_text == 0) { pend(crass::FX_EMPTY); break; }
        } else {
            if (F.n_bytes == 0) { pend(crass::FX_EMPTY); break; }
            if (!crass::fx_is_hdr_char(F.bytes[0])) { pend(crass::FX_FIRST_BYTE); break; }
            F.n_text = F.n_bytes; F.format = F.bytes[0];
        }
    }
    return CRASS_OK;
}

// 2. the job's text space over the files that were taken, and the nominal cuts in it: the caller's, else even ones
int files_nominal_cuts(crass_hip_group *g, const uint64_t *nominal, uint32_t n_files, int pad_uniform)
{
    auto &J = g->F;
    const int N = g->n;
    const uint32_t nf = J.nf;
    J.tb.assign(nf + 1, 0);
    for (uint32_t f = 0; f < nf; f++) J.tb[f + 1] = J.tb[f] + J.files[f].n_text;
    const uint64_t T = J.tb[nf];
    if (nominal && nf == n_files) for (int k = 0; k + 1 < N; k++) if (nominal[k] > T) return CRASS_ERR_INVALID_ARG;
    J.nom_x.assign(N + 1, T);
    J.nom_x[0] = 0;
    for (int k = 1; k < N; k++) J.nom_x[k] = nominal ? std::min(nominal[k - 1], T) : (uint64_t)((unsigned __int128)T * (unsigned)k / (unsigned)N);
    J.nom.resize(N + 1);
    for (int k = 0; k <= N; k++) J.nom[k] = locate(J.tb, nf, J.nom_x[k]);
    J.pad_uniform = pad_uniform;
    J.pieces.assign(N, {}); J.v_stage.assign(N, crass::ShardVerdict()); J.v_scan.assign(N, crass::ShardVerdict());
    J.file_reads.assign(N, {}); J.n_reads.assign(N, 0); J.max_len.assign(N, 0);
    J.cut.assign(N + 1, crass::ShardPos{nf, 0});
    return CRASS_OK;
}

// 3. the gzip files, now that the nominal cuts are known: every rank inflates the elements that hold its pieces (with the byte in
// front of a piece, as a BGZF file's members are taken) in two halves with the composition of the entry windows between them,
// and keeps their text on its device; rank 0 joins the CRC-32 parts.  The first file that does not inflate waits with its
// decline (GZ.v_gz) as a rank's staging decline does; the files behind it are inflated all the same
int files_inflate_gzip(crass_hip_group *g)
{
    auto &J = g->F;
    const int N = g->n;
    for (uint32_t f = 0; f < J.nf; f++) {
        if (!J.files[f].gz) continue;
        crass::GzRangesFile &Z = *const_cast<crass::GzRangesFile *>(J.files[f].gz);
        const uint64_t n = Z.n_chain;
        Z.e0.assign(N + 1, n); Z.e1.assign(N + 1, n); Z.first.assign(N + 1, 0);
        std::vector<uint8_t> holds(N + 1, 0);
        for (int r = 0; r < N; r++) {
            const crass::ShardPos lo = J.nom[r], hi = J.nom[r + 1];
            if (f < lo.file || f > hi.file) continue;
            const uint64_t a = f == lo.file ? lo.pos : 0, b = f == hi.file ? hi.pos : Z.n_text;
            if (a >= b) continue;
            crass::bgzf_members_for(Z.off.data(), n, a ? a - 1 : 0, b, &Z.e0[r], &Z.e1[r]);
            holds[r] = 1;
        }
        for (int r = N - 1; r >= 0; r--) if (!holds[r]) Z.e0[r] = Z.e1[r] = Z.e0[r + 1];      // (passes the window on to the next rank that holds some)
        for (int r = 0; r < N; r++) Z.first[r + 1] = std::max(Z.first[r], Z.e1[r]);
        int s = gzip_job_run(g, Z, false, true);
        if (s) return s;
        gzip_count_file(g, Z);
        crass::GzVerdict v{};
        if ((s = gzip_file_verdict(Z, &v))) return s;
        crass::ShardVerdict sv;
        sv.file = (int32_t)f; sv.bgzf.reason = v.reason; sv.bgzf.member = v.member; sv.bgzf.in_pos = v.in_pos;
        if (v.reason && crass::shard_verdict_before(sv, g->GZ.v_gz)) g->GZ.v_gz = sv;
    }
    return CRASS_OK;
}

// 5. the load's counters.  Of its gzip files: the elements the seeded walks added count as inflated by a further rank
void files_sum_counters(crass_hip_group *g)
{
    auto &J = g->F;
    if (!g->GZ.files.empty()) {
        for (uint64_t el : g->GZ.tail_el) g->GZ.cnt[3] += el;
        gzip_count_uploads(g);
    }
    g->load_cnt[0] = (uint64_t)J.attempts; g->load_cnt[1] = J.wrapped_pass ? J.n_chained : 0;
    for (int r = 0; J.wrapped_pass && r < g->n; r++) {
        uint64_t lk = 0, db = 0;
        shard_cut_counters(g->ctx[r], &lk, &db, nullptr);
        g->load_cnt[2] += db; g->load_cnt[3] += lk;
    }
}

// 6. the accepted load: every rank's first read, and crass_fastx_shards' arrays
void files_publish(crass_hip_group *g, uint32_t n_files, crass_fastx_shards *out)
{
    auto &J = g->F;
    auto &S = g->S;
    const int N = g->n;
    g->first = J.rank_base; g->n_reads = J.rank_base[N];
    S.cut_file.assign(N + 1, 0); S.cut_pos.assign(N + 1, 0); S.file_read_base.assign(n_files + 1, 0); S.format.assign(n_files, 0);
    for (int k = 0; k <= N; k++) { S.cut_file[k] = J.cut[k].file; S.cut_pos[k] = J.cut[k].pos; }
    for (int r = 0; r < N; r++) for (const auto &fr : J.file_reads[r]) S.file_read_base[fr.first + 1] += fr.second;
    for (uint32_t f = 0; f < n_files; f++) { S.file_read_base[f + 1] += S.file_read_base[f]; S.format[f] = J.files[f].format; }
    uint32_t max_len = 0;
    for (int r = 0; r < N; r++) max_len = std::max(max_len, J.max_len[r]);
    if (!out) return;
    out->n_reads = g->n_reads; out->max_len = max_len;
    out->rank_read_base = g->first.data(); out->cut_file = S.cut_file.data(); out->cut_pos = S.cut_pos.data();
    out->file_read_base = S.file_read_base.data(); out->format = S.format.data();
}

} // namespace

void grp::load_files_rank(crass_hip_group *g, int r)
{
    auto &J = g->F;
    crass_hip_ctx *c = g->ctx[r];
    for (int attempt = 1;; attempt++) {                 // (at most two: the second is decided once, behind the first)
        const bool w = attempt == 2;                    // (J.wrapped_pass, as every rank knows it)
        if (job_ok(g)) note(g, r, shard_stage_probe(c, J.files.data(), J.nf, J.nom[r], J.nom[r + 1], &J.pieces[r], &J.v_stage[r], w, g->shard_margin));
        g->bar->wait();                                 // every rank's probes (chains) are there
        rank0_step(g, r, [&] { return combine_cuts(g); });
        g->bar->wait();                                 // the actual cuts are known
        if (job_ok(g)) note(g, r, shard_scan(c, J.files.data(), J.nf_eff, J.cut[r], J.cut[r + 1], &J.file_reads[r], &J.n_reads[r], &J.max_len[r], &J.v_scan[r], w));
        g->bar->wait();                                 // every rank's records are counted
        rank0_step(g, r, [&] { finish_scan(g); if (attempt == 1) decide_second_attempt(g); return CRASS_OK; });
        g->bar->wait();                                 // the verdict, or every rank's first read — or one more attempt
        if (J.attempts <= attempt) break;
        shard_abort(c);
    }
    if (job_ok(g) && !J.declined) {
        int s = shard_pack(c, J.pad_uniform, J.rank_base[r]);
        if (!s) s = setup_exchange(g, r);
        note(g, r, s);
    } else shard_abort(c);
    if (!g->GZ.files.empty()) {                          // what the rank kept of the gzip files, and what its seeded walks took
        gzip_kept_report(c, &g->GZ.tail_ms[r], &g->GZ.tail_el[r], false);
        gzip_rank_report(c, g->GZ.ms[r].data(), &g->GZ.up[r]);
        gzip_kept_release(c);
    }
}

extern "C" {

int crass_hip_group_load_fastx_files(crass_hip_group *g, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                                     const uint64_t *nominal, crass_fastx_shards *out)
{
    if (out) { memset(out, 0, sizeof(*out)); out->decline_file = -1; out->n_files = n_files; out->n_ranks = g ? (uint32_t)g->n : 0; }
    if (!g || !n_files || !bytes || !n_bytes || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (n_bytes[f] && !bytes[f]) return CRASS_ERR_INVALID_ARG;
    const int N = g->n;
    for (int k = 1; nominal && k + 1 < N; k++) if (nominal[k] < nominal[k - 1]) return CRASS_ERR_INVALID_ARG;
    reset_for_load(g, 0, 0);
    auto &J = g->F;
    std::vector<crass_bgzf_index> ixs;
    struct FreeIx { std::vector<crass_bgzf_index> &v; ~FreeIx() { for (auto &x : v) crass_bgzf_index_free(&x); } } free_ix{ixs};
    // the caller's bytes and this call's indexes are used inside this call only: forgotten on every way out (host pointers; what a
    // rank keeps of the gzip files on its device goes back at the end of load_files_rank and at the start of the next load)
    struct Forget { crass_hip_group::FilesJob &J; ~Forget() { for (auto &F : J.files) { F.ix = nullptr; F.gz = nullptr; F.bytes = nullptr; } } } forget{J};
    try {
        J = crass_hip_group::FilesJob();
        g->names.assign(N, crass_hip_group::Text());
        ixs.assign(n_files, crass_bgzf_index{});
        for (uint64_t &x : g->GZ.cnt) x = 0;
        for (uint64_t &x : g->GZ.cnt_members) x = 0;
        for (crass_hip_ctx *c : g->ctx) gzip_kept_release(c);      // (what a failed load left)
        gzip_reset_reports(g);
        int st = files_classify(g, bytes, n_bytes, n_files, ixs);
        if (!st) st = files_nominal_cuts(g, nominal, n_files, pad_uniform);
        if (!st) st = files_inflate_gzip(g);
        if (st) return st;
        J.pend0 = J.pend;
        for (uint64_t &x : g->load_cnt) x = 0;
        st = dispatch(g, PH_LOAD_FILES);                // 4. every rank stages, probes, scans and packs its shard (load_files_rank)
        files_sum_counters(g);
        if (st) return st;
        if (J.declined) {
            if (out) { out->decline_file = J.verdict.file; out->decline_reason = J.verdict.reason; out->decline_pos = J.verdict.pos; out->bgzf = J.verdict.bgzf; }
            return CRASS_ERR_UNSUPPORTED;
        }
        files_publish(g, n_files, out);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    g->loaded = true; g->files_load = true; g->CM.ready = false;
    return CRASS_OK;
}

int crass_hip_group_load_counters(const crass_hip_group *g, uint64_t out[4])
{
    if (!g || !out) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = g->load_cnt[k];
    return CRASS_OK;
}

int crass_hip_group_set_fastq_class(crass_hip_group *g, int fastq_class)
{
    if (!g || fastq_class < 0 || fastq_class > 1) return CRASS_ERR_INVALID_ARG;
    for (crass_hip_ctx *c : g->ctx) { const int s = crass_hip_set_fastq_class(c, fastq_class); if (s) return s; }      // (fetch_quality reads by the context's class)
    g->fastq_class = fastq_class;
    return CRASS_OK;
}

} // extern "C"

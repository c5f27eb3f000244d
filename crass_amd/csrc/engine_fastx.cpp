// engine_fastx.cpp — the raw bytes of FASTA / FASTQ files in, parsed on the device (fastx_scan.hip): the scan of an arena of
// pieces (ArenaScan, ingest_internal.h) and what makes a scanned arena the resident set (arena_finish), both shared with
// engine_shards.cpp; one file in, as text, BGZF (inflate.hip) or plain gzip (gunzip.hip); several files as one set.
#include "ingest_internal.h"

// ---- the scan of an arena of pieces (ingest_internal.h says what the three steps promise) ----
int ArenaScan::open(crass_hip_ctx *c, const uint8_t *arena_, const uint64_t *base_, uint32_t n_pieces)
{
    Ingest &I = c->in;
    arena = arena_; base = base_;
    tile0.assign((size_t)n_pieces + 1, 0);
    for (uint32_t i = 0; i < n_pieces; i++) tile0[i + 1] = tile0[i] + fastx_n_tiles(arena + base[i], base[i + 1] - base[i] - 1);
    if (tile0[n_pieces] > 0x7FFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (beyond 8 TB)
    HIPCHK(c, I.x_tiles.ensure(tile0[n_pieces])); HIPCHK(c, I.x_base.ensure(tile0[n_pieces]));
    HIPCHK(c, I.x_tot.ensure(5 * (uint64_t)n_pieces)); HIPCHK(c, I.x_h_tot.ensure(5 * (uint64_t)n_pieces));
    jobs.assign(n_pieces, FxJob{});
    HIPCHK(c, I.tm_scan.begin(c->timing_level >= 1, c->stream));
    return CRASS_OK;
}

int ArenaScan::queue(crass_hip_ctx *c, uint32_t i, int32_t format, bool newline)
{
    const uint8_t *bytes = arena + base[i];
    FxJob &J = jobs[i];
    J = FxJob{};
    J.bytes = bytes; J.n = base[i + 1] - base[i] - 1; J.lead = (uint32_t)((uintptr_t)bytes & 15u); J.format = format;
    J.n_tiles = tile0[i + 1] - tile0[i];
    J.tiles = c->in.x_tiles.p + tile0[i]; J.base = c->in.x_base.p + tile0[i]; J.tot = c->in.x_tot.p + 4 * (uint64_t)i;
    HIPCHK(c, launch_fx_summary(J, c->stream));
    HIPCHK(c, launch_fx_tile_scan(J, c->stream));
    if (newline) HIPCHK(c, hipMemsetAsync(const_cast<uint8_t *>(arena) + base[i + 1] - 1, 0x0A, 1, c->stream));
    return CRASS_OK;
}

// FASTQ class 1 (fastx_wrapped.hip): the pieces f with w_of[f] >= 0 are read again under the wrapped rule of fastx_scan.h.  Each
// gets scratch of its own (Ingest::w_scratch, given back by release_scan), its line table, successors, reachable records and
// their ranks; the totals and verdicts come back in one wait.  The first piece in order that offends — under the wrapped rule,
// or the piece the four-line scan declined for good — is the verdict.  Otherwise every piece emits again with the bases the new
// totals give: the four-line pieces by k_fx_emit, the wrapped ones by k_fw_place / k_fw_emit.
int ArenaScan::emit_wrapped(crass_hip_ctx *c, uint32_t nf, uint64_t max_reads, const std::vector<int32_t> &w_of, uint32_t n_w,
                            std::vector<uint64_t> &tbase, ScanResult &R)
{
    Ingest &I = c->in;
    std::vector<uint64_t> &rbase = R.rbase;
    const uint64_t *h_verdict = I.x_h_tot.p + 4 * (uint64_t)jobs.size();
    std::vector<FwJob> wj(n_w);
    I.w_scratch.resize(n_w);
    HIPCHK(c, I.x_h_wtot.ensure((uint64_t)kFwTot * n_w));
    for (uint32_t f = 0; f < nf; f++) {
        if (w_of[f] < 0) continue;
        const FxJob &X = jobs[f];
        FwJob &J = wj[w_of[f]];
        J = FwJob{};
        if (I.x_h_tot.p[4 * f] >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (line indices are 32-bit, END is one of them)
        J.bytes = X.bytes; J.n = X.n; J.lead = X.lead; J.n_tiles = X.n_tiles; J.n_lines = (uint32_t)I.x_h_tot.p[4 * f];
        uint8_t last = 0;
        HIPCHK(c, hipMemcpy(&last, X.bytes + X.n - 1, 1, hipMemcpyDeviceToHost));
        J.ends_nl = fx_is_nl(last) ? 1u : 0u;
        DevBuf<uint64_t> &S = I.w_scratch[w_of[f]];
        HIPCHK(c, S.ensure(fw_scratch_words(J.n_tiles, J.n_lines)));
        fw_lay_out(J, S.p);
        HIPCHK(c, hipMemsetAsync(J.tot + 7, 0xFF, 8, c->stream));
        HIPCHK(c, launch_fw_tiles(J, c->stream));
        HIPCHK(c, launch_fw_analyse(J, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.x_h_wtot.p + (uint64_t)kFwTot * w_of[f], J.tot, 8 * kFwTot, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t f = 0; f < nf; f++) {
        uint64_t verdict = h_verdict[f];
        if (w_of[f] >= 0) {
            const uint64_t *t = I.x_h_wtot.p + (uint64_t)kFwTot * w_of[f];
            if (t[0] != wj[w_of[f]].n_lines) return CRASS_ERR_STATE;      // (never expected: both scans count the same line starts)
            verdict = t[7];
        }
        if (verdict != kFxNoOffence) { R.decline_file = (int32_t)f; R.decline_reason = (int32_t)(verdict & 0xFF); R.decline_pos = verdict >> 8; return CRASS_ERR_UNSUPPORTED; }
    }
    for (uint32_t f = 0; f < nf; f++) {
        const uint64_t *t = w_of[f] >= 0 ? I.x_h_wtot.p + (uint64_t)kFwTot * w_of[f] : nullptr;
        rbase[f + 1] = rbase[f] + (t ? t[5] : I.x_h_tot.p[4 * f + 1]);
        tbase[f + 1] = tbase[f] + (t ? t[6] : I.x_h_tot.p[4 * f + 2]);
    }
    const uint64_t nr = rbase[nf], total_seq = tbase[nf];
    if (nr >= max_reads) return CRASS_ERR_UNSUPPORTED;
    HIPCHK(c, I.x_text.ensure(total_seq + 32));
    HIPCHK(c, I.x_rec_pos.ensure(nr + 1)); HIPCHK(c, I.x_seq_off.ensure(nr + 1));
    HIPCHK(c, I.x_h_rec_pos.ensure(nr + 1)); HIPCHK(c, I.x_h_seq_off.ensure(nr + 1));
    for (uint32_t f = 0; f < nf; f++) {
        if (w_of[f] >= 0) {
            FwJob &J = wj[w_of[f]];
            J.n_reads = rbase[f + 1] - rbase[f];
            J.text = I.x_text.p; J.text_base = tbase[f]; J.text_cap = tbase[f + 1];
            J.rec_pos = I.x_rec_pos.p; J.seq_off = I.x_seq_off.p; J.read_base = rbase[f]; J.arena_base = base[f];
            HIPCHK(c, launch_fw_emit(J, c->stream));
        } else {
            FxJob &J = jobs[f];
            J.text = I.x_text.p; J.text_base = tbase[f]; J.text_cap = tbase[f + 1];
            J.rec_pos = I.x_rec_pos.p; J.seq_off = I.x_seq_off.p; J.read_base = rbase[f];
            HIPCHK(c, launch_fx_emit(J, c->stream));
        }
    }
    if (nr) {
        HIPCHK(c, hipMemcpyAsync(I.x_h_rec_pos.p, I.x_rec_pos.p, nr * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.x_h_seq_off.p, I.x_seq_off.p, nr * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRASS_OK;
}

int ArenaScan::emit(crass_hip_ctx *c, uint32_t nf, uint64_t max_reads, ScanResult &R)
{
    Ingest &I = c->in;
    const uint64_t n_planned = jobs.size();
    HIPCHK(c, hipMemcpyAsync(I.x_h_tot.p, I.x_tot.p, 4 * (uint64_t)nf * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (the record counts size the next kernels' arrays)
    std::vector<uint64_t> &rbase = R.rbase, tbase(nf + 1, 0);
    rbase.assign(nf + 1, 0);
    for (uint32_t f = 0; f < nf; f++) { rbase[f + 1] = rbase[f] + I.x_h_tot.p[4 * f + 1]; tbase[f + 1] = tbase[f] + I.x_h_tot.p[4 * f + 2]; }
    const uint64_t nr4 = rbase[nf], total_seq4 = tbase[nf];      // (as the four-line scan counts them)
    if (nr4 >= max_reads) return CRASS_ERR_UNSUPPORTED;
    HIPCHK(c, I.x_text.ensure(total_seq4 + 32));
    HIPCHK(c, I.x_rec_pos.ensure(nr4 + 1)); HIPCHK(c, I.x_seq_off.ensure(nr4 + 1));
    HIPCHK(c, I.x_h_rec_pos.ensure(nr4 + 1)); HIPCHK(c, I.x_h_seq_off.ensure(nr4 + 1));
    unsigned long long *d_verdict = reinterpret_cast<unsigned long long *>(I.x_tot.p + 4 * n_planned);
    HIPCHK(c, hipMemsetAsync(d_verdict, 0xFF, 8 * (uint64_t)nf, c->stream));
    for (uint32_t f = 0; f < nf; f++) {
        FxJob &J = jobs[f];
        J.n_lines = I.x_h_tot.p[4 * f]; J.n_reads = rbase[f + 1] - rbase[f];
        J.text = I.x_text.p; J.text_base = tbase[f]; J.text_cap = tbase[f + 1];
        J.rec_pos = I.x_rec_pos.p; J.seq_off = I.x_seq_off.p; J.read_base = rbase[f]; J.arena_base = base[f];
        J.verdict = d_verdict + f;
        HIPCHK(c, launch_fx_emit(J, c->stream));
    }
    HIPCHK(c, I.tm_scan.mark(c->stream));
    uint64_t *h_verdict = I.x_h_tot.p + 4 * n_planned;
    HIPCHK(c, hipMemcpyAsync(h_verdict, d_verdict, 8 * (uint64_t)nf, hipMemcpyDeviceToHost, c->stream));
    if (nr4) {
        HIPCHK(c, hipMemcpyAsync(I.x_h_rec_pos.p, I.x_rec_pos.p, nr4 * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.x_h_seq_off.p, I.x_seq_off.p, nr4 * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_scan.elapsed(0, 1, &I.last_scan_ms));
    auto decline = [&](uint32_t f, int32_t reason, uint64_t pos) {
        R.decline_file = (int32_t)f; R.decline_reason = reason; R.decline_pos = pos;
        return CRASS_ERR_UNSUPPORTED;
    };
    // FASTQ class 1: the pieces the four-line scan declined for their shape, up to the first piece declined for good
    std::vector<int32_t> w_of(nf, -1);
    uint32_t n_w = 0;
    for (uint32_t f = 0; wrapped && f < nf; f++) {
        if (h_verdict[f] == kFxNoOffence) continue;
        if (jobs[f].format != 0x40 || !fx_wrapped_takes((int32_t)(h_verdict[f] & 0xFF))) break;
        w_of[f] = (int32_t)n_w++;
    }
    I.scan_classes[0] = nf - n_w; I.scan_classes[1] = n_w;
    uint64_t nr = nr4, total_seq = total_seq4;
    if (n_w) {
        const int ws = emit_wrapped(c, nf, max_reads, w_of, n_w, tbase, R);
        if (ws) return ws;
        nr = rbase[nf]; total_seq = tbase[nf];
    }
    uint64_t *rec_pos = I.x_h_rec_pos.p, *seq_off = I.x_h_seq_off.p;
    rec_pos[nr] = base[nf] - 1; seq_off[nr] = total_seq;
    R.n_reads = nr; R.total_seq = total_seq; R.max_len = 0;
    for (uint32_t f = 0; f < nf; f++) {
        const uint64_t verdict = h_verdict[f];
        if (w_of[f] < 0 && verdict != kFxNoOffence) return decline(f, (int32_t)(verdict & 0xFF), verdict >> 8);
        const uint64_t seq_f = tbase[f + 1] - tbase[f];
        // (never expected: an accepted file has a record and as many quality as sequence bytes)
        if (rbase[f + 1] == rbase[f] || (w_of[f] < 0 && I.x_h_tot.p[4 * f + 3] != (jobs[f].format == 0x40 ? seq_f : 0))) return CRASS_ERR_STATE;
        for (uint64_t r = rbase[f]; r < rbase[f + 1]; r++) {
            const uint64_t l = (r + 1 < rbase[f + 1] ? seq_off[r + 1] : tbase[f + 1]) - seq_off[r];
            if (l > CRASS_HIP_MAX_READ_LEN) return decline(f, FX_READ_TOO_LONG, rec_pos[r] - base[f]);
            R.max_len = std::max(R.max_len, l);
        }
    }
    return CRASS_OK;
}

extern "C" {

// One file: h_bytes (host) or d_bytes (device), in a load the caller has opened (begin_fastx_load).  Accepted: the state is that
// of crass_hip_load_text on the reads' text; declined: no reads.
static int load_fastx_impl(crass_hip_ctx *c, const uint8_t *h_bytes, const uint8_t *d_bytes, uint64_t n, int pad_uniform,
                           uint64_t read_index_base, crass_fastx_layout *out)
{
    auto decline = [&](int32_t format, uint64_t pos, int32_t reason) {
        if (out) { out->format = format; out->decline_pos = pos; out->decline_reason = reason; }
        return CRASS_ERR_UNSUPPORTED;
    };
    if (n == 0) return decline(0, 0, FX_EMPTY);
    uint8_t b0 = 0;
    if (h_bytes) b0 = h_bytes[0];
    else HIPCHK(c, hipMemcpy(&b0, d_bytes, 1, hipMemcpyDeviceToHost));
    if (!fx_is_hdr_char(b0)) return decline(0, 0, FX_FIRST_BYTE);
    Ingest &I = c->in;
    if (h_bytes) {
        HIPCHK(c, I.x_raw.ensure(n + 16));
        const int up = upload_staged(c, h_bytes, n, I.x_raw.p);
        if (up) return up;
        d_bytes = I.x_raw.p;
    }
    const uint64_t base[2] = {0, n + 1};                // (rec_pos[n_reads] = n, and no '\n' is stored behind the bytes: they may be the caller's)
    ArenaScan A;
    int s = A.open(c, d_bytes, base, 1);
    if (s) return s;
    A.wrapped = I.fastq_class == FX_CLASS_WRAPPED;
    s = A.queue(c, 0, b0, false);
    if (s) return s;
    ScanResult R;
    s = A.emit(c, 1, ~0ull, R);
    if (s == CRASS_ERR_UNSUPPORTED && R.decline_file >= 0) return decline(b0, R.decline_pos, R.decline_reason);
    if (s) return s;
    s = load_text_impl(c, nullptr, I.x_text.p, I.x_h_seq_off.p, R.n_reads, pad_uniform, nullptr, read_index_base);
    if (s) return s;
    if (out) { out->n_reads = R.n_reads; out->format = b0; out->max_len = (uint32_t)R.max_len; out->rec_pos = I.x_h_rec_pos.p; out->seq_off = I.x_h_seq_off.p; }
    return CRASS_OK;
}

static int load_fastx_common(crass_hip_ctx *c, const uint8_t *h_bytes, const uint8_t *d_bytes, uint64_t n, int pad_uniform,
                             uint64_t read_index_base, crass_fastx_layout *out)
{
    if (out) memset(out, 0, sizeof(*out));
    if (!c || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    if (n && !h_bytes && !d_bytes) return CRASS_ERR_INVALID_ARG;
    begin_fastx_load(c);
    const int s = load_fastx_impl(c, h_bytes, d_bytes, n, pad_uniform, read_index_base, out);
    release_scan(c); release_text(c);                   // the scratch goes back on every way out, load_text_impl's part too
    return s;
}

int crass_hip_load_fastx_bytes(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                               crass_fastx_layout *out)
{
    return load_fastx_common(c, bytes, nullptr, n_bytes, pad_uniform, read_index_base, out);
}

int crass_hip_attach_device_fastx(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                  crass_fastx_layout *out)
{
    return load_fastx_common(c, nullptr, d_bytes, n_bytes, pad_uniform, read_index_base, out);
}

uint32_t crass_hip_fastx_tile_bytes(void) { return fastx_tile_bytes(); }

int crass_hip_set_fastq_class(crass_hip_ctx *c, int fastq_class)
{
    if (!c || (fastq_class != FX_CLASS_FOUR_LINE && fastq_class != FX_CLASS_WRAPPED)) return CRASS_ERR_INVALID_ARG;
    c->in.fastq_class = fastq_class;
    return CRASS_OK;
}

int crass_hip_last_scan_classes(const crass_hip_ctx *c, uint64_t out[2])
{
    if (!c || !out) return CRASS_ERR_INVALID_ARG;
    out[0] = c->in.scan_classes[0]; out[1] = c->in.scan_classes[1];
    return CRASS_OK;
}
float crass_hip_last_scan_ms(const crass_hip_ctx *c) { return c ? c->in.last_scan_ms : 0.0f; }

static int load_fastx_bgzf_impl(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, const crass_bgzf_index *ix, int pad_uniform,
                                uint64_t read_index_base, uint8_t *d_text, crass_fastx_layout *out, crass_bgzf_verdict *v)
{
    const uint64_t n_text = ix->out_off[ix->n_members];
    HIPCHK(c, c->in.z_raw.ensure(n_bytes + 16));
    const int up = upload_staged(c, bytes, n_bytes, c->in.z_raw.p);
    if (up) return up;
    if (!d_text) { HIPCHK(c, c->in.z_text.ensure(n_text + 16)); d_text = c->in.z_text.p; }
    const int s = inflate_bgzf_members(c, c->in.z_raw.p, ix, 0, ix->n_members, d_text, v);
    if (s) return s;
    c->in.z_raw.release();                                 // (the compressed bytes are done with: the scan's arrays may have their room)
    return load_fastx_impl(c, nullptr, d_text, n_text, pad_uniform, read_index_base, out);
}

int crass_hip_load_fastx_bgzf(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base, uint8_t *d_text,
                              uint64_t d_text_cap, crass_fastx_layout *out, crass_bgzf_verdict *v)
{
    if (out) memset(out, 0, sizeof(*out));
    if (v) memset(v, 0, sizeof(*v));
    if (!c || pad_uniform < 0 || pad_uniform > 2 || (n_bytes && !bytes)) return CRASS_ERR_INVALID_ARG;
    crass_bgzf_index ix;
    int s = crass_bgzf_index_host(bytes, n_bytes, &ix);
    if (s == CRASS_OK && d_text && d_text_cap < ix.out_off[ix.n_members]) s = CRASS_ERR_INVALID_ARG;
    if (s == CRASS_ERR_INVALID_ARG || s == CRASS_ERR_OOM) { crass_bgzf_index_free(&ix); return s; }
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    if (s == CRASS_ERR_UNSUPPORTED) { if (v) *v = ix.decline; return s; }
    s = load_fastx_bgzf_impl(c, bytes, n_bytes, &ix, pad_uniform, read_index_base, d_text, out, v);
    release_bgzf(c); release_scan(c); release_text(c);  // the scratch goes back on every way out, as in load_fastx_common
    crass_bgzf_index_free(&ix);
    return s;
}

static int load_fastx_gzip_impl(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base, uint8_t *d_text,
                                uint64_t d_text_cap, crass_fastx_layout *out, crass_gzip_members *members, bool mode, crass_bgzf_verdict *v)
{
    if (out) memset(out, 0, sizeof(*out));
    if (v) memset(v, 0, sizeof(*v));
    if (members) memset(members, 0, sizeof(*members));
    if (!c || pad_uniform < 0 || pad_uniform > 2 || (n_bytes && !bytes)) return CRASS_ERR_INVALID_ARG;
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    auto run = [&]() -> int {
        HIPCHK(c, c->in.z_raw.ensure(n_bytes + 16));
        const int up = upload_staged(c, bytes, n_bytes, c->in.z_raw.p);
        if (up) return up;
        HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        GzState S;
        int s = gzip_count_impl(c, c->in.z_raw.p, n_bytes, 0, S, nullptr, v, mode);
        if (s) return s;
        if (d_text && d_text_cap < S.n_text) return CRASS_ERR_INVALID_ARG;
        if (!d_text) { HIPCHK(c, c->in.z_text.ensure(S.n_text + 16)); d_text = c->in.z_text.p; }
        s = gzip_decode_impl(c, c->in.z_raw.p, S, d_text, v);
        if (s) return s;
        if (mode) { s = gz_members_fill(members, S.in_off.size() - 1, S.in_off.data(), S.text_off.data()); if (s) return s; }
        release_gzip(c);
        c->in.z_raw.release();                             // (the compressed bytes are done with: the scan's arrays may have their room)
        return load_fastx_impl(c, nullptr, d_text, S.n_text, pad_uniform, read_index_base, out);
    };
    const int s = run();
    release_gzip(c); release_bgzf(c); release_scan(c); release_text(c);      // the scratch goes back on every way out
    if (s && members) crass_gzip_members_free(members);      // (a scan decline behind an accepted inflate: no table without reads)
    return s;
}

int crass_hip_load_fastx_gzip(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base, uint8_t *d_text,
                              uint64_t d_text_cap, crass_fastx_layout *out, crass_bgzf_verdict *v)
{
    return load_fastx_gzip_impl(c, bytes, n_bytes, pad_uniform, read_index_base, d_text, d_text_cap, out, nullptr, false, v);
}

int crass_hip_load_fastx_gzip_members(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                      uint8_t *d_text, uint64_t d_text_cap, crass_fastx_layout *out, crass_gzip_members *members,
                                      crass_bgzf_verdict *v)
{
    return load_fastx_gzip_impl(c, bytes, n_bytes, pad_uniform, read_index_base, d_text, d_text_cap, out, members, true, v);
}

int crass_hip_set_gzip_on_device(crass_hip_ctx *c, int on)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    c->in.gzip_on_device = on == CRASS_GZIP_ON_DEVICE_MEMBERS ? CRASS_GZIP_ON_DEVICE_MEMBERS : on != 0 ? CRASS_GZIP_ON_DEVICE_ONE_MEMBER : CRASS_GZIP_ON_DEVICE_OFF;
    return CRASS_OK;
}

// ---- what makes a scanned arena the resident set ----
// One pack launch over the scan's text (x_text / x_h_seq_off), then the header ids of the records at x_h_rec_pos on the arena,
// installed from where they are, and the arena is the resident set's.  A set of no reads (an empty shard) has no header ids.
int arena_finish(crass_hip_ctx *c, const uint8_t *arena, uint64_t n_arena_bytes, uint64_t n_reads, int pad_uniform, uint64_t read_index_base)
{
    Ingest &I = c->in;
    const int s = load_text_impl(c, nullptr, I.x_text.p, I.x_h_seq_off.p, n_reads, pad_uniform, nullptr, read_index_base);
    if (s) return s;
    if (n_reads) {
        uint64_t n_rep = 0;
        const int hs = header_ids_device_impl(c, arena, n_arena_bytes, I.x_h_rec_pos.p, n_reads, nullptr, 1, &n_rep);
        if (hs) return hs;
        if (n_rep == 0) c->R.header_id = nullptr;       // (all names unique: as a load without header ids)
    }
    I.fa_bytes = n_arena_bytes; I.have_arena = true;
    return CRASS_OK;
}

// ---- several files into one resident set (fastx_scan.hip, inflate.hip, fastx_hid.hip) ----
namespace {
struct FilesPlan {
    struct File { bool bgzf = false, gz = false; crass_bgzf_index ix{}; GzState gzs; uint64_t n_text = 0; int32_t format = 0; };
    std::vector<File> f;
    ~FilesPlan() { for (auto &x : f) if (x.bgzf) crass_bgzf_index_free(&x.ix); }
};
}

static int load_fastx_files_impl(crass_hip_ctx *c, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                                 crass_fastx_files_layout *out)
{
    // a decline found before the scan (format, compression) waits here: a file in front of it may still offend in the scan
    int32_t pend_file = -1, pend_reason = 0; crass_bgzf_verdict pend_v{};
    auto decline = [&](uint32_t file, int32_t reason, uint64_t pos, const crass_bgzf_verdict *v) {
        if (out) { out->decline_file = (int32_t)file; out->decline_reason = reason; out->decline_pos = pos; if (v) out->bgzf = *v; }
        return CRASS_ERR_UNSUPPORTED;
    };
    // 1. what every file is, and how much text it holds (host: first bytes, BGZF index)
    FilesPlan P;
    P.f.resize(n_files);
    uint32_t nf = n_files;
    // (file f and the files behind it are out of the set: the caller leaves its loop)
    auto pend = [&](uint32_t f, int32_t reason, const crass_bgzf_verdict &v = crass_bgzf_verdict{}) { pend_file = (int32_t)f; pend_reason = reason; pend_v = v; nf = f; };
    for (uint32_t f = 0; f < nf; f++) {
        FilesPlan::File &F = P.f[f];
        const uint8_t *b = bytes[f];
        const uint64_t n = n_bytes[f];
        if (n >= 2 && b[0] == 0x1F && b[1] == 0x8B) {
            const int s = crass_bgzf_index_host(b, n, &F.ix);
            if (s == CRASS_ERR_UNSUPPORTED && c->in.gzip_on_device) {
                // plain gzip (crass_hip_set_gzip_on_device; of any number of members with CRASS_GZIP_ON_DEVICE_MEMBERS): its bytes go up once for the count step, which sizes its share of the arena
                HIPCHK(c, c->in.z_raw.ensure(n + 16));
                const int up = upload_staged(c, b, n, c->in.z_raw.p);
                if (up) return up;
                HIPCHK(c, hipStreamSynchronize(c->copy_stream));
                crass_bgzf_verdict v{};
                const int gs = gzip_count_impl(c, c->in.z_raw.p, n, 0, F.gzs, nullptr, &v, c->in.gzip_on_device == CRASS_GZIP_ON_DEVICE_MEMBERS);
                if (gs == CRASS_ERR_UNSUPPORTED) { pend(f, 0, v); break; }
                if (gs) return gs;
                F.gz = true; F.n_text = F.gzs.n_text;
                if (F.n_text == 0) { pend(f, FX_EMPTY); break; }
                continue;
            }
            if (s == CRASS_ERR_UNSUPPORTED) { pend(f, 0, F.ix.decline); break; }
            if (s) return s;
            F.bgzf = true; F.n_text = F.ix.out_off[F.ix.n_members];
            if (F.n_text == 0) { pend(f, FX_EMPTY); break; }
        } else {
            if (n == 0) { pend(f, FX_EMPTY); break; }
            if (!fx_is_hdr_char(b[0])) { pend(f, FX_FIRST_BYTE); break; }
            F.n_text = n; F.format = b[0];
        }
    }
    auto pending = [&]() { return decline((uint32_t)pend_file, pend_reason, 0, pend_v.reason ? &pend_v : nullptr); };
    if (nf == 0) return pending();
    // 2. the arena; every file's bytes up, a BGZF file inflated into its place; the first two scan kernels of file f are queued
    //    before file f + 1 is staged
    std::vector<uint64_t> base(nf + 1, 0);
    for (uint32_t f = 0; f < nf; f++) base[f + 1] = base[f] + P.f[f].n_text + 1;
    HIPCHK(c, c->in.fa_arena.ensure(base[nf] + 16));
    uint8_t *arena = c->in.fa_arena.p;
    ArenaScan A;
    const int os = A.open(c, arena, base.data(), nf);
    if (os) return os;
    A.wrapped = c->in.fastq_class == FX_CLASS_WRAPPED;
    for (uint32_t f = 0; f < nf; f++) {
        FilesPlan::File &F = P.f[f];
        if (f) HIPCHK(c, hipStreamSynchronize(c->copy_stream));      // (the staged buffers are the file before's until its last copy is done)
        if (F.bgzf || F.gz) {
            HIPCHK(c, c->in.z_raw.ensure(n_bytes[f] + 16));
            const int up = upload_staged(c, bytes[f], n_bytes[f], c->in.z_raw.p);
            if (up) return up;
            crass_bgzf_verdict v{};
            // (both wait for the stream: z_raw may be used again)
            const int s = F.gz ? gzip_decode_impl(c, c->in.z_raw.p, F.gzs, arena + base[f], &v) : inflate_bgzf_members(c, c->in.z_raw.p, &F.ix, 0, F.ix.n_members, arena + base[f], &v);
            if (s == CRASS_ERR_UNSUPPORTED) { pend(f, 0, v); break; }
            if (s) return s;
            HIPCHK(c, hipMemcpy(&F.format, arena + base[f], 1, hipMemcpyDeviceToHost));
            F.format &= 0xFF;
            if (!fx_is_hdr_char((uint8_t)F.format)) { pend(f, FX_FIRST_BYTE); break; }
        } else {
            const int up = upload_staged(c, bytes[f], n_bytes[f], arena + base[f]);
            if (up) return up;
        }
        const int qs = A.queue(c, f, F.format, true);      // (and the '\n' behind the file)
        if (qs) return qs;
    }
    if (nf == 0) return pending();
    // 3. every file emits into one text and one pair of per-record arrays; 4. the verdict: the first file in order that offends
    ScanResult R;
    const int es = A.emit(c, nf, 0xFFFFFFFFull, R);
    if (es == CRASS_ERR_UNSUPPORTED && R.decline_file >= 0) return decline((uint32_t)R.decline_file, R.decline_reason, R.decline_pos, nullptr);
    if (es) return es;
    const std::vector<uint64_t> &rbase = R.rbase;
    const uint64_t nr = R.n_reads, max_len = R.max_len;
    uint64_t *rec_pos = c->in.x_h_rec_pos.p, *seq_off = c->in.x_h_seq_off.p;
    if (pend_file >= 0) return pending();
    // 5. one pack launch over the joined text, then the header ids on the arena, installed from where they are
    const int s = arena_finish(c, arena, base[nf], nr, pad_uniform, 0);
    if (s) { c->have_reads = false; return s; }
    HIPCHK(c, c->in.fa_h_base.ensure(2 * ((uint64_t)nf + 1))); HIPCHK(c, c->in.fa_h_format.ensure(nf));
    for (uint32_t f = 0; f <= nf; f++) { c->in.fa_h_base.p[f] = rbase[f]; c->in.fa_h_base.p[nf + 1 + f] = base[f]; }
    for (uint32_t f = 0; f < nf; f++) c->in.fa_h_format.p[f] = P.f[f].format;
    c->in.fa_read_base.assign(rbase.begin(), rbase.begin() + nf + 1);
    if (out) {
        out->n_reads = nr; out->max_len = (uint32_t)max_len; out->rec_pos = rec_pos; out->seq_off = seq_off;
        out->file_read_base = c->in.fa_h_base.p; out->file_byte_base = c->in.fa_h_base.p + nf + 1; out->format = c->in.fa_h_format.p;
    }
    return CRASS_OK;
}

int crass_hip_load_fastx_files(crass_hip_ctx *c, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                               crass_fastx_files_layout *out)
{
    if (out) { memset(out, 0, sizeof(*out)); out->decline_file = -1; out->n_files = n_files; }
    if (!c || !n_files || !bytes || !n_bytes || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (n_bytes[f] && !bytes[f]) return CRASS_ERR_INVALID_ARG;
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    const int s = load_fastx_files_impl(c, bytes, n_bytes, n_files, pad_uniform, out);
    // the scratch goes back on every way out, as in load_fastx_common; the arena stays only with an accepted set
    release_gzip(c); release_bgzf(c); release_scan(c); release_text(c); release_header_ids(c);
    if (s) { c->have_reads = false; drop_arena(c); }
    return s;
}

int crass_hip_resident_fastx(const crass_hip_ctx *c, const uint8_t **d_bytes, uint64_t *n_bytes)
{
    if (!c || !d_bytes || !n_bytes) return CRASS_ERR_INVALID_ARG;
    *d_bytes = nullptr; *n_bytes = 0;
    if (!c->in.have_arena || !c->have_reads) return CRASS_ERR_STATE;
    *d_bytes = c->in.fa_arena.p; *n_bytes = c->in.fa_bytes;
    return CRASS_OK;
}

} // extern "C"

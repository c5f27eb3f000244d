// engine_inflate.cpp — compressed bytes inflated on the device: the members of a BGZF file (inflate.hip, inflate_core.h) and
// plain gzip of one member or several, chunk by chunk (gunzip.hip, gunzip_core.h).  The loaders that scan what is inflated
// here are engine_fastx.cpp and engine_shards.cpp; what they call is declared in ingest_internal.h.
#include "ingest_internal.h"
#include "gunzip_ranges.h"

extern "C" {

// ---- BGZF members inflated on the device (inflate.hip) ----
// a compressed input is declined: the verdict, where the caller wants one
static int bz_decline(crass_bgzf_verdict *v, int32_t reason, uint64_t member, uint64_t in_pos)
{
    if (v) { v->reason = reason; v->member = member; v->in_pos = in_pos; }
    return CRASS_ERR_UNSUPPORTED;
}

// the index is checked, d_in / d_out are device pointers: upload the offsets, launch, read the verdict
// (the members [m0, m0 + n) of the index alone: d_in and d_out stay the places of the FILE's byte 0 and the TEXT's byte 0, which
// may lie outside what the caller holds — a member's bytes are read and written inside its own ranges only, inflate.hip)
int inflate_bgzf_members(crass_hip_ctx *c, const uint8_t *d_in, const crass_bgzf_index *ix, uint64_t m0, uint64_t n, uint8_t *d_out,
                         crass_bgzf_verdict *v)
{
    c->in.last_inflate_ms = 0;
    if (n == 0) return CRASS_OK;
    HIPCHK(c, c->in.z_idx.ensure(3 * n + 2)); HIPCHK(c, c->in.z_reason.ensure(n)); HIPCHK(c, c->in.z_verdict.ensure(1)); HIPCHK(c, c->in.z_h_verdict.ensure(1));
    BzJob J{};
    J.in = d_in; J.out = d_out; J.n_members = n;
    J.in_off = c->in.z_idx.p; J.out_off = c->in.z_idx.p + (n + 1); J.data_off = c->in.z_idx.p + 2 * (n + 1);
    J.reason = c->in.z_reason.p; J.verdict = c->in.z_verdict.p; J.hbm_window = c->env.inflate_hbm_window ? 1 : 0;
    HIPCHK(c, hipMemcpyAsync(c->in.z_idx.p, ix->in_off + m0, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.z_idx.p + (n + 1), ix->out_off + m0, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.z_idx.p + 2 * (n + 1), ix->data_off + m0, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(J.verdict, 0xFF, 8, c->stream));
    HIPCHK(c, c->in.tm_inflate.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_bgzf_inflate(J, c->stream));
    HIPCHK(c, c->in.tm_inflate.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.z_h_verdict.p, J.verdict, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (the index's host arrays are the caller's: nothing reads them after this)
    HIPCHK(c, c->in.tm_inflate.elapsed(0, 1, &c->in.last_inflate_ms));
    const uint64_t w = c->in.z_h_verdict.p[0];
    if (w == kBzNoOffence) return CRASS_OK;
    return bz_decline(v, (int32_t)(w & 0xFF), m0 + (w >> 8), ix->in_off[m0 + (w >> 8)]);
}


int crass_hip_inflate_bgzf_device(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, const crass_bgzf_index *ix, uint8_t *d_out, uint64_t out_cap,
                                  crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    if (!c) return CRASS_ERR_INVALID_ARG;
    const int chk = bgzf_index_check(ix, n_in, out_cap);
    if (chk) return chk;
    if (ix->n_members && (!d_in || (ix->out_off[ix->n_members] && !d_out))) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const int s = inflate_bgzf_members(c, d_in, ix, 0, ix->n_members, d_out, v);
    release_bgzf(c);
    return s;
}

// ---- one plain gzip member inflated on the device chunk by chunk (gunzip.hip, gunzip_core.h) ----
// header and trailer (host), find and count (device), the chain (host): CRASS_OK with S.n_text known, or the decline
// (members: the rule's members mode, kept in S for the decode step)
int gzip_count_impl(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, GzState &S, crass_gzip_plan *plan,
                    crass_bgzf_verdict *v, bool members)
{
    S.members = members; S.n_file = n_in;
    c->in.last_inflate_ms = 0;
    for (auto &m : c->in.last_gzip_ms) m = 0;
    try {
        // the header's bytes come down in a piece that grows until the header ends inside it
        std::vector<uint8_t> head;
        uint8_t trailer[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n_in >= 18) HIPCHK(c, hipMemcpy(trailer, d_in + n_in - 8, 8, hipMemcpyDeviceToHost));
        int32_t why = BZ_NOT_GZIP;
        for (uint64_t h = std::min<uint64_t>(n_in, 65536);; h = std::min<uint64_t>(n_in, h * 4)) {
            head.resize(h ? h : 1);
            if (h) HIPCHK(c, hipMemcpy(head.data(), d_in, h, hipMemcpyDeviceToHost));
            why = gz_parse_member(head.data(), h, trailer, n_in, chunk_bytes, &S.M);
            if (why != -1 || h == n_in) break;
        }
        if (why != BZ_OK) return bz_decline(v, BZ_NOT_GZIP, 0, 0);
        const GzGeom &G = S.M.G;
        const uint64_t nc = G.nc;
        HIPCHK(c, c->in.gz_a64.ensure((members ? 4 : 3) * nc)); HIPCHK(c, c->in.gz_a32.ensure((members ? 3 : 2) * nc));
        GzJob J{};
        J.d = d_in + G.d_off; J.G = G; gz_job_whole(J);
        J.start = c->in.gz_a64.p; J.text_len = c->in.gz_a64.p + nc; J.end_bit = c->in.gz_a64.p + 2 * nc;
        J.link = c->in.gz_a32.p; J.reason = reinterpret_cast<int32_t *>(c->in.gz_a32.p + nc);
        if (members) { J.last_end = c->in.gz_a64.p + 3 * nc; J.n_ends = c->in.gz_a32.p + 2 * nc; }
        StageTimer<6> &T = c->in.tm_gzip;
        HIPCHK(c, T.begin(c->timing_level >= 1, c->stream));
        HIPCHK(c, launch_gz_find(J, c->stream, members));
        HIPCHK(c, T.mark(c->stream));
        HIPCHK(c, launch_gz_count(J, c->stream, members));      // (a launch of its own: every start is final before a chunk counts)
        HIPCHK(c, T.mark(c->stream));
        S.start.resize(nc); S.text_len.resize(nc); S.end_bit.resize(nc); S.link.resize(nc); S.reason.resize(nc); S.chain.assign(nc, 0);
        HIPCHK(c, hipMemcpyAsync(S.start.data(), J.start, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.text_len.data(), J.text_len, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.end_bit.data(), J.end_bit, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.link.data(), J.link, nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.reason.data(), J.reason, nc * 4, hipMemcpyDeviceToHost, c->stream));
        if (members) {
            S.n_ends.resize(nc); S.last_end.resize(nc);
            HIPCHK(c, hipMemcpyAsync(S.n_ends.data(), J.n_ends, nc * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(S.last_end.data(), J.last_end, nc * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 2; k++) HIPCHK(c, T.elapsed(k, k + 1, &c->in.last_gzip_ms[k]));
        c->in.last_inflate_ms = c->in.last_gzip_ms[0] + c->in.last_gzip_ms[1];
        GzVerdict gv{};
        const int32_t bad = gz_chain(S.M, S.start.data(), S.link.data(), S.text_len.data(), S.end_bit.data(), S.reason.data(), S.chain.data(),
                                     &S.n_chain, &S.n_text, &gv, members);
        const int ps = gz_plan_fill(plan, nc, S.start.data(), S.link.data(), S.text_len.data(), S.n_chain);
        if (ps) return ps;
        if (bad != BZ_OK) return bz_decline(v, gv.reason, gv.member, gv.in_pos);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

// decode, windows, narrow: the text of an accepted count into d_out[0, S.n_text)
// (members mode: every member's ISIZE and CRC-32 are checked here, behind the kernels; S gets the member table)
int gzip_decode_impl(crass_hip_ctx *c, const uint8_t *d_in, GzState &S, uint8_t *d_out, crass_bgzf_verdict *v)
{
    const bool members = S.members;
    const GzGeom &G = S.M.G;
    const uint64_t nc = G.nc, n = S.n_chain;
    try {
        std::vector<uint64_t> off(n + 1, 0);
        for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + S.text_len[S.chain[i]];
        std::vector<uint32_t> crc_part(n, 0);
        // members mode: [slot (n + 1) | m0 (n)] go up behind off; the pieces' bounds follow once the member table is known
        std::vector<uint64_t> places(2 * n + 1, 0);
        if (members) {
            std::vector<uint64_t> off2(n + 1, 0);
            gz_places(S.chain.data(), n, S.text_len.data(), S.n_ends.data(), S.last_end.data(), off2.data(), places.data(), places.data() + n + 1);
        }
        const uint64_t nm = members ? places[n] : 0;
        const uint64_t max_pieces = members ? nm + S.n_text / kGzCrcPiece + 1 : 0;
        HIPCHK(c, c->in.gz_b64.ensure(2 * nc + n + 1 + (members ? 2 * n + 1 + max_pieces + 1 : 0))); HIPCHK(c, c->in.gz_b32.ensure(2 * n + max_pieces));
        if (members) HIPCHK(c, c->in.gz_ends.ensure(3 * (nm ? nm : 1)));
        HIPCHK(c, c->in.gz_sym.ensure(S.n_text)); HIPCHK(c, c->in.gz_win.ensure(n * (uint64_t)kGzWindow));
        HIPCHK(c, c->in.z_verdict.ensure(1)); HIPCHK(c, c->in.z_h_verdict.ensure(1));
        GzJob J{};
        J.d = d_in + G.d_off; J.G = G; gz_job_whole(J);
        J.start = c->in.gz_b64.p; J.end_bit = c->in.gz_b64.p + nc;
        J.n_chain = n; J.off = c->in.gz_b64.p + 2 * nc; J.chain = c->in.gz_b32.p; J.crc_part = c->in.gz_b32.p + n;
        J.sym = c->in.gz_sym.p; J.win = c->in.gz_win.p; J.out = d_out; J.verdict = c->in.z_verdict.p;
        if (members) {
            static_assert(sizeof(GzEnd) == 24 && alignof(GzEnd) == 8, "GzEnd is three words");
            uint64_t *pl = c->in.gz_b64.p + 2 * nc + n + 1;
            J.slot = pl; J.m0 = pl + n + 1; J.piece = pl + 2 * n + 1; J.crc_piece = c->in.gz_b32.p + 2 * n;
            J.ends = reinterpret_cast<GzEnd *>(c->in.gz_ends.p);
            HIPCHK(c, hipMemcpyAsync(pl, places.data(), (2 * n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(J.start, S.start.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(J.end_bit, S.end_bit.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.gz_b64.p + 2 * nc, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.gz_b32.p, S.chain.data(), n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(J.verdict, 0xFF, 8, c->stream));
        StageTimer<6> &T = c->in.tm_gzip;
        HIPCHK(c, T.begin(c->timing_level >= 1, c->stream, 2));      // (the count step's last mark again: the uploads above are not decode's)
        HIPCHK(c, launch_gz_decode(J, c->stream, members));
        HIPCHK(c, T.mark(c->stream));
        HIPCHK(c, launch_gz_windows(J, c->stream));
        HIPCHK(c, T.mark(c->stream));
        HIPCHK(c, launch_gz_narrow(J, c->stream, members));
        std::vector<uint64_t> piece;
        std::vector<uint32_t> mcrc, misz;
        if (members) {
            // the records come down (the stream is waited for: decode is done, narrow may still run), the member table and the
            // pieces are made, the pieces' bounds go up for k_gz_member_crc; narrow's time then includes that round trip
            std::vector<GzEnd> ends(nm ? nm : 1);
            HIPCHK(c, hipMemcpyAsync(ends.data(), J.ends, nm * sizeof(GzEnd), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            S.in_off.assign(nm + 1, 0); S.text_off.assign(nm + 1, 0); mcrc.assign(nm, 0); misz.assign(nm, 0);
            gz_member_table(S.M, S.n_file, off.data(), places.data(), n, ends.data(), S.in_off.data(), S.text_off.data(), mcrc.data(), misz.data());
            for (uint64_t m = 0; m < nm; m++) {
                if (S.text_off[m + 1] < S.text_off[m] || S.text_off[m + 1] > S.n_text) return CRASS_ERR_STATE;      // (a record nobody wrote)
                for (uint64_t p = S.text_off[m]; p < S.text_off[m + 1]; p += kGzCrcPiece) piece.push_back(p);
            }
            piece.push_back(S.n_text);
            if (piece.size() - 1 > max_pieces) return CRASS_ERR_STATE;
            J.n_pieces = piece.size() - 1;
            HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t *>(J.piece), piece.data(), piece.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, launch_gz_member_crc(J, c->stream));
        }
        HIPCHK(c, T.mark(c->stream));
        std::vector<uint32_t> crc_piece(members ? piece.size() : 1, 0);
        if (members && J.n_pieces) HIPCHK(c, hipMemcpyAsync(crc_piece.data(), J.crc_piece, J.n_pieces * 4, hipMemcpyDeviceToHost, c->stream));
        if (!members) HIPCHK(c, hipMemcpyAsync(crc_part.data(), J.crc_part, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.z_h_verdict.p, J.verdict, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int k = 2; k < 5; k++) {
            HIPCHK(c, T.elapsed(k, k + 1, &c->in.last_gzip_ms[k]));
            c->in.last_inflate_ms += c->in.last_gzip_ms[k];
        }
        const uint64_t w = c->in.z_h_verdict.p[0];
        if (w != kBzNoOffence) {
            const uint64_t k = S.chain[w];
            return bz_decline(v, BZ_MARKER, k, G.d_off + (S.start[k] >> 3));
        }
        if (members) {
            // a member's pieces joined in text order (an empty member has none: CRC 0)
            std::vector<uint32_t> got(nm, 0);
            uint64_t q = 0;
            for (uint64_t m = 0; m < nm; m++)
                for (; q + 1 < piece.size() && piece[q] < S.text_off[m + 1]; q++) got[m] = gz_crc_join(got[m], crc_piece[q], piece[q + 1] - piece[q]);
            GzVerdict mv{};
            if (gz_member_verdict(nm, S.in_off.data(), S.text_off.data(), mcrc.data(), misz.data(), got.data(), &mv) != BZ_OK)
                return bz_decline(v, mv.reason, mv.member, mv.in_pos);
            return CRASS_OK;
        }
        uint32_t crc = 0;
        for (uint64_t i = 0; i < n; i++) crc = gz_crc_join(crc, crc_part[i], off[i + 1] - off[i]);
        if (crc != S.M.crc) return bz_decline(v, BZ_CRC, 0, 0);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

static int inflate_gzip_device_impl(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                    uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, bool mode, crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    if (plan) memset(plan, 0, sizeof(*plan));
    if (members) memset(members, 0, sizeof(*members));
    if (n_text) *n_text = 0;
    if (!c || !n_text || (n_in && !d_in) || (out_cap && !d_out)) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    GzState S;
    int s = gzip_count_impl(c, d_in, n_in, chunk_bytes, S, plan, v, mode);
    if (s == CRASS_OK) {
        *n_text = S.n_text;
        if (out_cap < S.n_text) s = CRASS_ERR_OVERFLOW;       // (known before anything is stored)
        else s = gzip_decode_impl(c, d_in, S, d_out, v);
        if (s == CRASS_OK && mode) s = gz_members_fill(members, S.in_off.size() - 1, S.in_off.data(), S.text_off.data());
    }
    release_gzip(c); release_bgzf(c);                   // (the verdict word is the BGZF inflate's)
    return s;
}

int crass_hip_inflate_gzip_device(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                  uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v)
{
    return inflate_gzip_device_impl(c, d_in, n_in, chunk_bytes, d_out, out_cap, n_text, plan, nullptr, false, v);
}

int crass_hip_inflate_gzip_members_device(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                          uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v)
{
    return inflate_gzip_device_impl(c, d_in, n_in, chunk_bytes, d_out, out_cap, n_text, plan, members, true, v);
}

int crass_hip_last_gzip_ms(const crass_hip_ctx *c, float *ms)
{
    if (!c || !ms) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 5; k++) ms[k] = c->in.last_gzip_ms[k];
    return CRASS_OK;
}

float crass_hip_last_inflate_ms(const crass_hip_ctx *c) { return c ? c->in.last_inflate_ms : 0.0f; }

} // extern "C"

// ---- one plain gzip file inflated across the ranks of a group (gunzip_ranges.h): one rank's steps ----
namespace {

// the deflate bytes [lo, hi) of the file in z_raw.  What z_raw holds of this file stays: the new range is taken as the hull of
// both, what is kept moves device to device, only the missing ends come up.  z_raw may have gone back in between (release_bgzf)
int gzr_stage(crass_hip_ctx *c, const GzRangesFile &F, uint64_t lo, uint64_t hi)
{
    Ingest &I = c->in;
    const bool kept = I.z_raw.p && I.gzr_file == F.bytes && I.gzr_hi > I.gzr_lo && I.z_raw.n >= I.gzr_hi - I.gzr_lo;
    const uint64_t klo = kept ? I.gzr_lo : 0, khi = kept ? I.gzr_hi : 0;
    if (kept && lo >= klo && hi <= khi) return CRASS_OK;
    if (kept && lo <= khi && hi >= klo) { lo = std::min(lo, klo); hi = std::max(hi, khi); }      // (the hull, where they touch)
    const uint8_t *src = F.bytes + F.M.G.d_off;
    I.gzr_uploads.reserve(I.gzr_uploads.size() + 2);    // (nothing below throws)
    DevBuf<uint8_t> fresh;
    auto run = [&]() -> int {
        HIPCHK(c, fresh.ensure(hi - lo + 16));
        const uint64_t a = std::max(lo, klo), b = std::min(hi, khi);      // what is kept of [lo, hi): [a, b)
        const bool some = kept && a < b;
        if (some) HIPCHK(c, hipMemcpyAsync(fresh.p + (a - lo), I.z_raw.p + (a - klo), b - a, hipMemcpyDeviceToDevice, c->stream));
        const uint64_t parts[2][2] = {{lo, some ? a : hi}, {some ? b : hi, hi}};
        for (const auto &q : parts) {
            if (q[0] >= q[1]) continue;
            const int s = upload_staged(c, src + q[0], q[1] - q[0], fresh.p + (q[0] - lo));
            if (s) return s;
            I.gzr_uploads.push_back(std::make_pair((uint64_t)(uintptr_t)(src + q[0]), (uint64_t)(uintptr_t)(src + q[1])));      // (host addresses: files apart)
            // (upload_staged begins with its first pinned buffer whatever the upload before left in flight: at most two uploads here)
            HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CRASS_OK;
    };
    const int s = run();
    if (s) { fresh.release(); return s; }
    I.z_raw.release();
    I.z_raw = fresh;
    I.gzr_file = F.bytes; I.gzr_lo = lo; I.gzr_hi = hi;
    return CRASS_OK;
}

// a job over the staged bytes and the per-chunk arrays of gz_a64 / gz_a32
GzJob gzr_job(crass_hip_ctx *c, const GzRangesFile &F)
{
    Ingest &I = c->in;
    const uint64_t nc = F.M.G.nc;
    GzJob J{};
    J.d = reinterpret_cast<const uint8_t *>((uintptr_t)I.z_raw.p - I.gzr_lo); J.G = F.M.G;
    // (members mode: a rank whose find runs see the region's end stages the 8 bytes behind it too; they are no part of the region)
    J.in_lo = I.gzr_lo; J.in_hi = std::min(I.gzr_hi, F.M.G.dn); J.in_tail = I.gzr_hi >= F.M.G.dn + 8 ? 1u : 0u;
    J.start = I.gz_a64.p; J.text_len = I.gz_a64.p + nc; J.end_bit = I.gz_a64.p + 2 * nc;
    J.link = I.gz_a32.p; J.reason = reinterpret_cast<int32_t *>(I.gz_a32.p + nc);
    if (F.members) { J.last_end = I.gz_a64.p + 3 * nc; J.n_ends = I.gz_a32.p + 2 * nc; }
    return J;
}

} // namespace

int gzip_rank_find(crass_hip_ctx *c, GzRangesFile &F, uint32_t r)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    I.gzr_lo = I.gzr_hi = 0; I.gzr_file = nullptr;
    for (float &m : I.gzr_ms) m = 0;
    I.gzr_crc_ms = 0;
    const GzGeom &G = F.M.G;
    const uint64_t nc = G.nc, k0 = F.k_lo(r), k1 = F.k_lo(r + 1);
    try {
        HIPCHK(c, I.gz_a64.ensure(4 * nc)); HIPCHK(c, I.gz_a32.ensure(3 * nc));
        if (k0 >= k1) return CRASS_OK;
        uint64_t in_end = gz_input_end(G, k1 - 1);
        if (F.members && in_end == G.dn) in_end += 8;       // (io.tail(): a member's start whose first block is final and ends the region)
        const int ss = gzr_stage(c, F, gz_nominal(G, k0) >> 3, in_end);
        if (ss) return ss;
        GzJob J = gzr_job(c, F);
        J.k0 = k0; J.k1 = k1;
        HIPCHK(c, I.tm_gzr.begin(c->timing_level >= 1, c->stream, 0));
        HIPCHK(c, launch_gz_find(J, c->stream, F.members));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        HIPCHK(c, hipMemcpyAsync(F.start.data() + k0, J.start + k0, (k1 - k0) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, I.tm_gzr.elapsed(0, 1, &I.gzr_ms[0]));
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int gzip_rank_count(crass_hip_ctx *c, GzRangesFile &F, uint32_t r)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    const uint64_t nc = F.M.G.nc, k0 = F.k_lo(r), k1 = F.k_lo(r + 1);
    if (k0 >= k1) return CRASS_OK;
    GzJob J = gzr_job(c, F);
    J.k0 = k0; J.k1 = k1;
    HIPCHK(c, hipMemcpyAsync(J.start, F.start.data(), nc * 8, hipMemcpyHostToDevice, c->stream));      // (every rank's starts: a run links to any later chunk)
    HIPCHK(c, I.tm_gzr.begin(c->timing_level >= 1, c->stream, 2));
    HIPCHK(c, launch_gz_count(J, c->stream, F.members));
    HIPCHK(c, I.tm_gzr.mark(c->stream));
    const uint64_t n = k1 - k0;
    if (F.members) {
        HIPCHK(c, hipMemcpyAsync(F.n_ends.data() + k0, J.n_ends + k0, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(F.last_end.data() + k0, J.last_end + k0, n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(F.text_len.data() + k0, J.text_len + k0, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(F.end_bit.data() + k0, J.end_bit + k0, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(F.link.data() + k0, J.link + k0, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(F.reason.data() + k0, J.reason + k0, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_gzr.elapsed(2, 3, &I.gzr_ms[1]));
    return CRASS_OK;
}

static uint64_t gzr_max_pieces(const GzRangesFile &F, uint64_t a, uint64_t b) { return (F.off[b] - F.off[a]) / kGzCrcPiece + (F.slot[b] - F.slot[a]) + 3; }

// the job of the rank's elements [a, b): the chain arrays of gz_b64 / gz_b32, sym and out as the places of text byte 0
static GzJob gzr_element_job(crass_hip_ctx *c, const GzRangesFile &F, uint64_t a, uint64_t b)
{
    Ingest &I = c->in;
    GzJob J = gzr_job(c, F);
    const uint64_t ne = b - a, last = std::min(b, F.n_chain - 1);
    J.e0 = a; J.n_chain = ne; J.n_win = last - a;
    J.off = I.gz_b64.p; J.chain = I.gz_b32.p; J.crc_part = I.gz_b32.p + ne;
    J.sym = reinterpret_cast<uint16_t *>((uintptr_t)I.gz_sym.p - 2 * F.off[a]);
    J.win = I.gz_win.p; J.wsym = I.gz_wsym.p;
    if (F.members) {                                    // [off (ne + 1) | slot (ne + 1) | m0 (ne + 1) | the rank's pieces]
        J.slot = I.gz_b64.p + (ne + 1); J.m0 = I.gz_b64.p + 2 * (ne + 1);
        J.ends = reinterpret_cast<GzEnd *>(I.gz_ends.p);
    }
    return J;
}

int gzip_rank_decode(crass_hip_ctx *c, GzRangesFile &F, uint32_t r)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    const GzGeom &G = F.M.G;
    const uint64_t nc = G.nc, a = F.e0[r], b = F.e1[r], ne = b - a;
    F.exported[r].clear();
    if (ne == 0) return CRASS_OK;
    try {
        const int ss = gzr_stage(c, F, F.start[F.chain[a]] >> 3, gz_input_end(G, F.chain[b - 1]));
        if (ss) return ss;
        const uint64_t n_win = std::min(b, F.n_chain - 1) - a;
        // (members mode: room for the rank's pieces too, which the finish step uploads behind what this step leaves here: at most
        // one per 64 KB of its text, one per member it touches and one where its own text begins)
        const uint64_t n_rec = F.members ? F.slot[b] - F.slot[a] : 0, max_p = F.members ? gzr_max_pieces(F, a, b) : 0;
        HIPCHK(c, I.gz_a64.ensure(4 * nc)); HIPCHK(c, I.gz_b64.ensure(ne + 1 + (F.members ? 2 * (ne + 1) + max_p + 1 : 0))); HIPCHK(c, I.gz_b32.ensure(2 * ne + max_p));
        HIPCHK(c, I.gz_sym.ensure(F.off[b] - F.off[a] + 1)); HIPCHK(c, I.gz_win.ensure(std::max(ne, n_win + 1) * (uint64_t)kGzWindow));
        HIPCHK(c, I.gz_wsym.ensure((n_win + 1) * (uint64_t)kGzWindow));
        if (F.members) HIPCHK(c, I.gz_ends.ensure(3 * (n_rec ? n_rec : 1)));
        GzJob J = gzr_element_job(c, F, a, b);
        if (F.members) {
            // (m0 also of the element behind the last one where the walk makes its window: a + n_win <= n_chain - 1)
            HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t *>(J.slot), F.slot.data() + a, (ne + 1) * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t *>(J.m0), F.m0.data() + a, (n_win + 1) * 8, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(J.start, F.start.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(J.end_bit, F.end_bit.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.gz_b64.p, F.off.data() + a, (ne + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.gz_b32.p, F.chain.data() + a, ne * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, I.tm_gzr.begin(c->timing_level >= 1, c->stream, 4));
        HIPCHK(c, launch_gz_decode(J, c->stream, F.members));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        HIPCHK(c, launch_gz_windows_sym(J, c->stream, F.members));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        // members mode: the records of the elements no rank in front holds, into the file's table (ranges of F.ends apart)
        const uint64_t f = std::max(a, F.first[r]);
        if (F.members && f < b && F.slot[b] > F.slot[f]) {
            static_assert(sizeof(GzEnd) == 24 && alignof(GzEnd) == 8, "GzEnd is three words");
            if (F.ends.size() < F.slot[b]) return CRASS_ERR_STATE;
            HIPCHK(c, hipMemcpyAsync(F.ends.data() + F.slot[f], J.ends + (F.slot[f] - F.slot[a]), (F.slot[b] - F.slot[f]) * sizeof(GzEnd), hipMemcpyDeviceToHost,
                                     c->stream));
        }
        // the window in front of the next rank's first element: this range's where that element lies behind its first one
        const uint64_t next = F.e0[r + 1];
        if (next > a && next < F.n_chain) {
            if (next - a > n_win) return CRASS_ERR_STATE;      // (never expected: e0 <= e0' <= e1)
            F.exported[r].resize(kGzWindow);
            HIPCHK(c, hipMemcpyAsync(F.exported[r].data(), J.wsym + (next - a) * (uint64_t)kGzWindow, kGzWindow * 2, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, I.tm_gzr.elapsed(4, 5, &I.gzr_ms[2])); HIPCHK(c, I.tm_gzr.elapsed(6, 7, &I.gzr_ms[3]));
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int gzip_rank_finish(crass_hip_ctx *c, GzRangesFile &F, uint32_t r, uint8_t *out, bool keep)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    const uint64_t a = F.e0[r], b = F.e1[r], ne = b - a;
    F.bad[r] = ~0ull;
    if (ne == 0) return CRASS_OK;
    try {
        if (a && F.entry[r].size() != kGzWindow) return CRASS_ERR_STATE;
        HIPCHK(c, I.z_text.ensure(F.off[b] - F.off[a] + 32)); HIPCHK(c, I.z_verdict.ensure(1)); HIPCHK(c, I.z_h_verdict.ensure(1));
        GzJob J = gzr_element_job(c, F, a, b);
        J.out = reinterpret_cast<uint8_t *>((uintptr_t)I.z_text.p + 16 - F.off[a]);
        J.verdict = I.z_verdict.p;
        if (a) HIPCHK(c, hipMemcpyAsync(J.win, F.entry[r].data(), kGzWindow, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(J.verdict, 0xFF, 8, c->stream));
        HIPCHK(c, I.tm_gzr.begin(c->timing_level >= 1, c->stream, 8));
        HIPCHK(c, launch_gz_window_resolve(J, c->stream));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        HIPCHK(c, launch_gz_narrow(J, c->stream, F.members));
        HIPCHK(c, I.tm_gzr.mark(c->stream));
        const uint64_t f = std::max(a, F.first[r]);
        // members mode: the CRC-32 of the pieces of the text this rank holds first, [q0, q1) of the file's pieces, their cuts
        // relative to the rank's text base (a rank that holds nothing first, or a table that is no table: none)
        uint64_t q0 = 0, q1 = 0;
        if (F.members && F.table_ok && f < b) {
            q0 = std::lower_bound(F.piece.begin(), F.piece.begin() + F.n_pieces, F.off[f]) - F.piece.begin();
            q1 = std::lower_bound(F.piece.begin(), F.piece.begin() + F.n_pieces, F.off[b]) - F.piece.begin();
        }
        std::vector<uint64_t> rel;                      // (read by an upload: lives until the stream is waited for below)
        I.gzr_crc_ms = 0;
        if (q1 > q0) {
            // (never expected: a piece is one rank's, and the decode step left room for them)
            if (F.piece[q1] > F.off[b] || F.crc_piece.size() < q1 || q1 - q0 > gzr_max_pieces(F, a, b)) return CRASS_ERR_STATE;
            rel.resize(q1 - q0 + 1);
            for (uint64_t q = q0; q <= q1; q++) rel[q - q0] = F.piece[q] - F.off[a];
            GzJob P = J;
            P.out = I.z_text.p + 16; P.n_pieces = q1 - q0;
            P.piece = I.gz_b64.p + 3 * (ne + 1); P.crc_piece = I.gz_b32.p + 2 * ne;
            HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t *>(P.piece), rel.data(), rel.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, I.tm_gzr.mark(c->stream));
            HIPCHK(c, launch_gz_member_crc(P, c->stream));
            HIPCHK(c, I.tm_gzr.mark(c->stream));
            HIPCHK(c, hipMemcpyAsync(F.crc_piece.data() + q0, P.crc_piece, (q1 - q0) * 4, hipMemcpyDeviceToHost, c->stream));
        }
        // what no rank in front holds: its text to the caller, its CRC parts to the host
        if (f < b) {
            if (out && F.off[b] > F.off[f]) HIPCHK(c, hipMemcpyAsync(out + F.off[f], J.out + F.off[f], F.off[b] - F.off[f], hipMemcpyDeviceToHost, c->stream));
            if (!F.members) HIPCHK(c, hipMemcpyAsync(F.crc_part.data() + f, J.crc_part + (f - a), (b - f) * 4, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(I.z_h_verdict.p, J.verdict, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, I.tm_gzr.elapsed(8, 9, &I.gzr_ms[4])); HIPCHK(c, I.tm_gzr.elapsed(10, 11, &I.gzr_ms[5]));
        if (q1 > q0) HIPCHK(c, I.tm_gzr.elapsed(12, 13, &I.gzr_crc_ms));
        const uint64_t w = I.z_h_verdict.p[0];
        if (w != kBzNoOffence) F.bad[r] = a + w;
        if (keep) {
            // a files load: the text stays on this rank's device until the load ends, with the resolved window behind its last
            // element, from which further elements are walked (gzip_kept_inflate)
            I.gz_kept.emplace_back();
            Ingest::GzKept &K = I.gz_kept.back();
            K.file = F.bytes; K.e0 = a; K.e1 = b;
            K.text = I.z_text; I.z_text = DevBuf<uint8_t>();
            HIPCHK(c, K.seed.ensure(kGzWindow));
            if (b < F.n_chain) HIPCHK(c, hipMemcpyAsync(K.seed.p, J.win + ne * (uint64_t)kGzWindow, kGzWindow, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

// further elements [K.e1, m1) of a kept range: decoded, their windows walked by k_gz_windows from the kept seed, narrowed behind the
// text that is there; the seed moves on.  An unresolved marker: CRASS_ERR_UNSUPPORTED with *bv
static int gzip_kept_grow(crass_hip_ctx *c, const GzRangesFile &F, Ingest::GzKept &K, uint64_t m1, crass_bgzf_verdict *bv)
{
    Ingest &I = c->in;
    const GzGeom &G = F.M.G;
    const uint64_t nc = G.nc, a = K.e1, b = m1, ne = b - a, n_win = std::min(b, F.n_chain - 1) - a;
    const int ss = gzr_stage(c, F, F.start[F.chain[a]] >> 3, gz_input_end(G, F.chain[b - 1]));
    if (ss) return ss;
    DevBuf<uint8_t> grown;
    auto run = [&]() -> int {
        HIPCHK(c, grown.ensure(F.off[b] - F.off[K.e0] + 32));
        HIPCHK(c, I.gz_a64.ensure(4 * nc)); HIPCHK(c, I.gz_b64.ensure(ne + 1 + (F.members ? 2 * (ne + 1) : 0))); HIPCHK(c, I.gz_b32.ensure(2 * ne));
        HIPCHK(c, I.gz_sym.ensure(F.off[b] - F.off[a] + 1)); HIPCHK(c, I.gz_win.ensure(std::max(ne, n_win + 1) * (uint64_t)kGzWindow));
        HIPCHK(c, I.z_verdict.ensure(1)); HIPCHK(c, I.z_h_verdict.ensure(1));
        GzJob J = gzr_element_job(c, F, a, b);
        if (F.members) {
            // the members rule with the elements' m0; the GzEnd records these runs meet again are in the table already: no slots
            J.slot = nullptr; J.ends = nullptr;
            HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t *>(J.m0), F.m0.data() + a, ne * 8, hipMemcpyHostToDevice, c->stream));
        }
        J.out = reinterpret_cast<uint8_t *>((uintptr_t)grown.p + 16 - F.off[K.e0]);
        J.verdict = I.z_verdict.p;
        if (F.off[a] > F.off[K.e0]) HIPCHK(c, hipMemcpyAsync(grown.p + 16, K.text.p + 16, F.off[a] - F.off[K.e0], hipMemcpyDeviceToDevice, c->stream));
        if (a) HIPCHK(c, hipMemcpyAsync(J.win, K.seed.p, kGzWindow, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(J.start, F.start.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(J.end_bit, F.end_bit.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.gz_b64.p, F.off.data() + a, (ne + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.gz_b32.p, F.chain.data() + a, ne * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(J.verdict, 0xFF, 8, c->stream));
        HIPCHK(c, launch_gz_decode(J, c->stream, F.members));
        HIPCHK(c, I.tm_gzt.begin(c->timing_level >= 1, c->stream));
        HIPCHK(c, launch_gz_windows(J, c->stream));
        HIPCHK(c, I.tm_gzt.mark(c->stream));
        HIPCHK(c, launch_gz_narrow(J, c->stream, F.members));
        if (b < F.n_chain) HIPCHK(c, hipMemcpyAsync(K.seed.p, J.win + ne * (uint64_t)kGzWindow, kGzWindow, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.z_h_verdict.p, J.verdict, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        HIPCHK(c, I.tm_gzt.elapsed(0, 1, &ms));
        I.gzr_tail_ms += ms; I.gzr_tail_elements += ne;
        const uint64_t w = I.z_h_verdict.p[0];
        if (w != kBzNoOffence) {
            const uint64_t k = F.chain[a + w];
            if (bv) { bv->reason = BZ_MARKER; bv->member = k; bv->in_pos = G.d_off + (F.start[k] >> 3); }
            return CRASS_ERR_UNSUPPORTED;
        }
        return CRASS_OK;
    };
    const int s = run();
    if (s) { grown.release(); return s; }
    K.text.release();
    K.text = grown; K.e1 = b;
    return CRASS_OK;
}

int gzip_kept_inflate(crass_hip_ctx *c, const GzRangesFile &F, uint64_t m0, uint64_t m1, uint8_t *text0, crass_bgzf_verdict *bv)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    if (m0 >= m1) return CRASS_OK;
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    try {
        Ingest::GzKept *K = nullptr;
        for (auto &k : I.gz_kept) if (k.file == F.bytes) K = &k;
        // a rank whose nominal range held nothing of the file (a cut that moved into a file the range did not touch: the file's
        // position 0, when no record starts between the nominal cut and the end of the file before): from element 0, which has no
        // window — correct, and serial over everything in front of m1, which there is what the rank needs anyway (its range
        // begins at the file's first byte)
        if (!K) {
            I.gz_kept.emplace_back();
            K = &I.gz_kept.back();
            K->file = F.bytes;
            HIPCHK(c, K->seed.ensure(kGzWindow)); HIPCHK(c, K->text.ensure(32));
        }
        if (m0 < K->e0) return CRASS_ERR_STATE;         // (never expected: a rank's later needs lie behind its nominal range's first element)
        if (m1 > K->e1) { const int s = gzip_kept_grow(c, F, *K, m1, bv); if (s) return s; }
        HIPCHK(c, hipMemcpyAsync(text0 + F.off[m0], K->text.p + 16 + (F.off[m0] - F.off[K->e0]), F.off[m1] - F.off[m0], hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

void gzip_kept_release(crass_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    wait_main(c);
    for (auto &k : c->in.gz_kept) { k.text.release(); k.seed.release(); }
    c->in.gz_kept.clear();
}

void gzip_kept_report(crass_hip_ctx *c, float *tail_ms, uint64_t *tail_elements, bool reset)
{
    if (tail_ms) *tail_ms = c ? c->in.gzr_tail_ms : 0.0f;
    if (tail_elements) *tail_elements = c ? c->in.gzr_tail_elements : 0;
    if (c && reset) { c->in.gzr_tail_ms = 0; c->in.gzr_tail_elements = 0; c->in.gzr_uploads.clear(); }
}

void gzip_rank_release(crass_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    release_gzip(c); release_bgzf(c);                   // (the staged bytes, the text and the verdict word are the BGZF inflate's)
    c->in.gzr_lo = c->in.gzr_hi = 0; c->in.gzr_file = nullptr;
}

float gzip_rank_member_crc_ms(const crass_hip_ctx *c) { return c ? c->in.gzr_crc_ms : 0.0f; }

void gzip_rank_report(const crass_hip_ctx *c, float ms[6], std::vector<std::pair<uint64_t, uint64_t>> *uploads)
{
    for (int k = 0; k < 6; k++) ms[k] = c ? c->in.gzr_ms[k] : 0.0f;
    if (uploads) { uploads->clear(); if (c) *uploads = c->in.gzr_uploads; }
}

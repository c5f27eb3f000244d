// engine_inflate.cpp — compressed bytes inflated on the device: the members of a BGZF file (inflate.hip, inflate_core.h) and
// plain gzip of one member or several, chunk by chunk (gunzip.hip, gunzip_core.h).  The loaders that scan what is inflated
// here are engine_fastx.cpp and engine_shards.cpp; what they call is declared in ingest_internal.h.
#include "ingest_internal.h"

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
        J.d = d_in + G.d_off; J.G = G;
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
        J.d = d_in + G.d_off; J.G = G;
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

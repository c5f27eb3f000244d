// gunzip.cpp — plain gzip on the host: a serial run of gunzip_core.h's rule (find, count, chain, decode, windows, narrow), one
// chunk after the other.  It needs no GPU; it is what the kernels (gunzip.hip) are tested against, itself tested against zlib.
// crass_gzip_inflate_members_host is the same run in members mode (a file of several members); crass_gzip_inflate_ranges_host and
// crass_gzip_inflate_members_ranges_host are both rules as the ranks of a group run them, range after range.
// Host-only C++17 that any compiler builds (tools/sanitize).  Scratch: 2 bytes per text byte and 32 KB per chain element.
#include "../../include/crass_hip.h"
#include "gunzip_core.h"

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace crass {

// the host's way through the core: one executor, one index after the other
struct GzHostIO {
    const uint8_t *d; uint64_t dn; const uint8_t *src; uint32_t n_in; uint16_t *sym; uint64_t cap;
    GzEnd *ends = nullptr; uint32_t ends_cap = 0;         // (members mode)
    void at(uint64_t b0, uint32_t n) { src = d + b0; n_in = n; }
    uint32_t in(uint32_t i) const { return i < n_in ? src[i] : 0u; }
    void put(uint64_t p, uint32_t s) { if (p < cap) sym[p] = (uint16_t)s; }
    uint32_t get(uint64_t p) const { return p < cap ? sym[p] : 0u; }
    template <class F> void par(uint32_t n, F f) { for (uint32_t i = 0; i < n; i++) f(i); }
    bool lead() const { return true; }
    void sync() {}
    uint64_t survivors(uint64_t base, uint64_t hi, uint64_t limit) const
    {
        uint64_t m = 0;
        for (uint32_t l = 0; l < 64; l++) m |= (uint64_t)gz_survives(d, dn, base + l, hi, limit) << l;
        return m;
    }
    uint64_t header_survivors(uint64_t base, uint64_t hi, uint64_t limit) const
    {
        uint64_t m = 0;
        for (uint32_t l = 0; l < 64; l += 8) m |= (uint64_t)gz_survives_header(d, dn, base + l, hi, limit) << l;      // (base is a multiple of 8)
        return m;
    }
    uint32_t tail(uint32_t i) const { return i < 8 ? d[dn + i] : 0u; }
    void end(uint32_t e, const GzEnd &r) { if (e < ends_cap) ends[e] = r; }
};

// what the rule decided, for the caller (malloc'd: crass_gzip_plan_free)
int gz_plan_fill(crass_gzip_plan *plan, uint64_t nc, const uint64_t *start, const uint32_t *link, const uint64_t *text_len, uint64_t n_chain)
{
    if (!plan) return CRASS_OK;
    crass_gzip_plan_free(plan);
    plan->start_bit = (uint64_t *)malloc(nc * 8); plan->link = (uint32_t *)malloc(nc * 4); plan->text_len = (uint64_t *)malloc(nc * 8);
    if (!plan->start_bit || !plan->link || !plan->text_len) { crass_gzip_plan_free(plan); return CRASS_ERR_OOM; }
    memcpy(plan->start_bit, start, nc * 8); memcpy(plan->link, link, nc * 4); memcpy(plan->text_len, text_len, nc * 8);
    plan->n_chunks = nc; plan->n_chain = n_chain;
    return CRASS_OK;
}

int gz_members_fill(crass_gzip_members *m, uint64_t nm, const uint64_t *in_off, const uint64_t *text_off)
{
    if (!m) return CRASS_OK;
    crass_gzip_members_free(m);
    m->in_off = (uint64_t *)malloc((nm + 1) * 8); m->text_off = (uint64_t *)malloc((nm + 1) * 8);
    if (!m->in_off || !m->text_off) { crass_gzip_members_free(m); return CRASS_ERR_OOM; }
    memcpy(m->in_off, in_off, (nm + 1) * 8); memcpy(m->text_off, text_off, (nm + 1) * 8);
    m->n_members = nm;
    return CRASS_OK;
}

} // namespace crass

using namespace crass;

// what find, count and the chain leave on the host
struct GzHostCount {
    GzMember M{};
    std::vector<uint64_t> start, text_len, end_bit, last_end;
    std::vector<uint32_t> link, chain, n_ends;
    std::vector<int32_t> reason;
    uint64_t n_chain = 0, total = 0;
};

static int gz_decline(crass_bgzf_verdict *v, int32_t reason, uint64_t member, uint64_t in_pos)
{
    if (v) { v->reason = reason; v->member = member; v->in_pos = in_pos; }
    return CRASS_ERR_UNSUPPORTED;
}

// the arguments, the header, find, count, the chain and the plan: -1 when the text is to be made (P filled, *n_text set, out_cap
// large enough), else what the caller returns
template <bool MEM>
static int gz_front_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_text,
                         crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v, GzHostIO &io, BzTables &T, GzHostCount &P)
{
    if (v) memset(v, 0, sizeof(*v));
    if (plan) memset(plan, 0, sizeof(*plan));
    if (members) memset(members, 0, sizeof(*members));
    if (n_text) *n_text = 0;
    if (!n_text || (n_bytes && !bytes) || (out_cap && !out)) return CRASS_ERR_INVALID_ARG;
    if (gz_parse_member(bytes, n_bytes, n_bytes >= 8 ? bytes + n_bytes - 8 : nullptr, n_bytes, chunk_bytes, &P.M) != BZ_OK) return gz_decline(v, BZ_NOT_GZIP, 0, 0);
    const GzGeom &G = P.M.G;
    const uint64_t nc = G.nc;
    P.start.assign(nc, kGzNoStart); P.text_len.assign(nc, 0); P.end_bit.assign(nc, 0); P.last_end.assign(nc, 0);
    P.link.assign(nc, GZ_LINK_NONE); P.chain.assign(nc, 0); P.n_ends.assign(nc, 0); P.reason.assign(nc, 0);
    io = GzHostIO{bytes + G.d_off, G.dn, nullptr, 0, nullptr, 0};
    bz_prepare(io, T);
    // find
    P.start[0] = 0;
    for (uint64_t k = 1; k < nc; k++) P.start[k] = gz_find<MEM>(io, T, G, k);
    // count
    for (uint64_t k = 0; k < nc; k++) {
        if (P.start[k] == kGzNoStart) continue;
        const GzRun R = gz_run<GZ_COUNT, MEM>(io, T, G, k, P.start[k], P.start.data(), 0);
        P.link[k] = R.link; P.text_len[k] = R.text; P.end_bit[k] = R.end_bit; P.reason[k] = R.reason; P.n_ends[k] = R.n_ends; P.last_end[k] = R.last_end;
    }
    // chain
    GzVerdict gv{};
    const int32_t why = gz_chain(P.M, P.start.data(), P.link.data(), P.text_len.data(), P.end_bit.data(), P.reason.data(), P.chain.data(), &P.n_chain,
                                 &P.total, &gv, MEM);
    const int status = gz_plan_fill(plan, nc, P.start.data(), P.link.data(), P.text_len.data(), P.n_chain);
    if (status) return status;
    if (why != BZ_OK) return gz_decline(v, gv.reason, gv.member, gv.in_pos);
    *n_text = P.total;
    if (out_cap < P.total) return CRASS_ERR_OVERFLOW;
    return -1;
}

// the serial run; MEM: members mode (gunzip_core.h), `members` (may be NULL) gets the member table
template <bool MEM>
static int gz_inflate_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_text,
                           crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v)
{
    auto decline = [&](int32_t reason, uint64_t member, uint64_t in_pos) { return gz_decline(v, reason, member, in_pos); };
    BzTables *T = new (std::nothrow) BzTables;
    if (!T) return CRASS_ERR_OOM;
    int status = CRASS_OK;
    try {
        GzHostIO io{};
        GzHostCount P;
        status = gz_front_host<MEM>(bytes, n_bytes, chunk_bytes, out, out_cap, n_text, plan, members, v, io, *T, P);
        if (status >= 0) { delete T; return status; }
        status = CRASS_OK;
        const GzMember &M = P.M;
        const GzGeom &G = M.G;
        const uint64_t nc = G.nc, n_chain = P.n_chain, total = P.total;
        const std::vector<uint64_t> &start = P.start, &text_len = P.text_len, &end_bit = P.end_bit, &last_end = P.last_end;
        const std::vector<uint32_t> &chain = P.chain, &n_ends = P.n_ends;
        std::vector<uint64_t> off(nc, 0);
        // decode
        std::vector<uint16_t> sym(total ? total : 1);
        std::vector<uint8_t> win(n_chain * (uint64_t)kGzWindow);
        uint64_t t = 0;
        for (uint64_t i = 0; i < n_chain; i++) { off[chain[i]] = t; t += text_len[chain[i]]; }
        // (members mode: the chain's places by element, every element's GzEnd slots)
        std::vector<uint64_t> eoff(n_chain + 1, 0), slot(n_chain + 1, 0), m0(n_chain, 0);
        if (MEM) gz_places(chain.data(), n_chain, text_len.data(), n_ends.data(), last_end.data(), eoff.data(), slot.data(), m0.data());
        std::vector<GzEnd> ends(slot[n_chain] ? slot[n_chain] : 1);
        for (uint64_t i = 0; i < n_chain; i++) {
            const uint64_t k = chain[i];
            io.sym = sym.data() + off[k]; io.cap = text_len[k];
            io.ends = ends.data() + slot[i]; io.ends_cap = (uint32_t)(slot[i + 1] - slot[i]);
            (void)gz_run<GZ_DECODE, MEM>(io, *T, G, k, start[k], nullptr, end_bit[k]);
        }
        // windows, in chain order
        for (uint64_t i = 1; i < n_chain; i++) {
            const uint64_t kp = chain[i - 1];
            const uint8_t *wp = i > 1 ? win.data() + (i - 1) * (uint64_t)kGzWindow : nullptr;
            uint8_t *w = win.data() + i * (uint64_t)kGzWindow;
            for (uint32_t e = 0; e < kGzWindow; e++) w[e] = gz_window_entry(sym.data() + off[kp], text_len[kp], wp, e);
        }
        // narrow, the CRC-32 element by element
        uint32_t crc = 0;
        for (uint64_t i = 0; i < n_chain && status == CRASS_OK; i++) {
            const uint64_t k = chain[i];
            const uint8_t *w = i ? win.data() + i * (uint64_t)kGzWindow : nullptr;
            uint32_t c = 0xFFFFFFFFu;
            for (uint64_t p = 0; p < text_len[k]; p++) {
                const uint32_t b = gz_narrow(sym[off[k] + p], w, off[k], m0[i]);
                if (b > 0xFFu) { status = decline(BZ_MARKER, k, G.d_off + (start[k] >> 3)); break; }
                out[off[k] + p] = (uint8_t)b;
                c = T->crc_tab[(c ^ b) & 0xFFu] ^ (c >> 8);
            }
            crc = gz_crc_join(crc, text_len[k] ? ~c : 0u, text_len[k]);
        }
        if (!MEM && status == CRASS_OK && crc != M.crc) status = decline(BZ_CRC, 0, 0);
        if (MEM && status == CRASS_OK) {
            // every member's place, ISIZE and CRC-32: behind the decode step, from the records the runs left
            const uint64_t nm = slot[n_chain];
            std::vector<uint64_t> in_off(nm + 1, 0), text_off(nm + 1, 0);
            std::vector<uint32_t> mcrc(nm, 0), misz(nm, 0), got(nm, 0);
            gz_member_table(M, n_bytes, eoff.data(), slot.data(), n_chain, ends.data(), in_off.data(), text_off.data(), mcrc.data(), misz.data());
            for (uint64_t m = 0; m < nm; m++) {
                uint32_t c = 0xFFFFFFFFu;
                for (uint64_t p = text_off[m]; p < text_off[m + 1]; p++) c = T->crc_tab[(c ^ out[p]) & 0xFFu] ^ (c >> 8);
                got[m] = text_off[m + 1] > text_off[m] ? ~c : 0u;
            }
            GzVerdict mv{};
            if (gz_member_verdict(nm, in_off.data(), text_off.data(), mcrc.data(), misz.data(), got.data(), &mv) != BZ_OK)
                status = decline(mv.reason, mv.member, mv.in_pos);
            else status = gz_members_fill(members, nm, in_off.data(), text_off.data());
        }
    } catch (const std::bad_alloc &) { status = CRASS_ERR_OOM; }
    delete T;
    return status;
}

// the distributed rule (a group's ranks) as a serial run: range after range, each one its own symbols and symbolic windows from
// an identity entry; the entry window of a range is composed from the range before it, which on the host has just finished.
// MEM: the members rule by ranges (gunzip_core.h): every range's GzEnd records in slots of its own, the table from each element's
// first holder; dead window entries read 0; the members' CRC-32 from pieces, the verdict behind all narrowing
template <bool MEM>
static int gz_inflate_ranges_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint32_t n_ranges, const uint64_t *nominal, uint8_t *out,
                                  uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v)
{
    BzTables *T = new (std::nothrow) BzTables;
    if (!T) return CRASS_ERR_OOM;
    int status = CRASS_OK;
    try {
        GzHostIO io{};
        GzHostCount P;
        status = gz_front_host<MEM>(bytes, n_bytes, chunk_bytes, out, out_cap, n_text, plan, members, v, io, *T, P);
        if (status >= 0) { delete T; return status; }
        status = CRASS_OK;
        const GzGeom &G = P.M.G;
        const uint64_t n = P.n_chain;
        std::vector<uint64_t> off(n + 1, 0), e0(n_ranges + 1, n), e1(n_ranges + 1, n);      // (a range behind the last: no elements)
        std::vector<uint64_t> slot(n + 1, 0), m0(n, 0);
        if (MEM) gz_places(P.chain.data(), n, P.text_len.data(), P.n_ends.data(), P.last_end.data(), off.data(), slot.data(), m0.data());
        else for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + P.text_len[P.chain[i]];
        if (!gz_ranges(off.data(), n, n_ranges, nominal, e0.data(), e1.data())) { delete T; *n_text = 0; return CRASS_ERR_INVALID_ARG; }
        std::vector<uint32_t> crc_part(n, 0);
        std::vector<uint8_t> entry(kGzWindow, 0), next_entry(kGzWindow, 0), win(kGzWindow, 0);
        std::vector<uint16_t> sym, wsym(kGzWindow), wsym_before(kGzWindow);
        std::vector<GzEnd> ends(slot[n] ? slot[n] : 1), own;      // (members mode: the table's records, a range's own)
        std::vector<uint64_t> base;                     // (members mode: where the text a range holds first begins)
        uint64_t done = 0;                              // elements [0, done) have their text: every part from the first range that holds it
        for (uint32_t r = 0; r < n_ranges && status == CRASS_OK; r++) {
            const uint64_t a = e0[r], b = e1[r];
            // decode: the range's elements as symbols, element i at sym[off[i] - off[a]]
            sym.assign(off[b] - off[a] + 1, 0);
            if (MEM) own.assign(slot[b] - slot[a] + 1, GzEnd{0, 0, 0, 0});
            for (uint64_t i = a; i < b; i++) {
                const uint64_t k = P.chain[i];
                io.sym = sym.data() + (off[i] - off[a]); io.cap = P.text_len[k];
                if (MEM) { io.ends = own.data() + (slot[i] - slot[a]); io.ends_cap = (uint32_t)(slot[i + 1] - slot[i]); }
                (void)gz_run<GZ_DECODE, MEM>(io, *T, G, k, P.start[k], nullptr, P.end_bit[k]);
            }
            if (MEM && b > std::max(a, done)) {
                const uint64_t f = std::max(a, done);
                for (uint64_t e = slot[f]; e < slot[b]; e++) ends[e] = own[e - slot[a]];
                base.push_back(off[f]);
            }
            // element after element: the symbolic window in front of it (of a, the identity), resolved through the entry window; its
            // text.  The window in front of b is made too where the next range starts there
            const uint64_t last = std::min(b, n - 1);
            for (uint64_t i = a; i <= last && status == CRASS_OK; i++) {
                if (i > a) {
                    wsym.swap(wsym_before);
                    const uint16_t *sp = sym.data() + (off[i - 1] - off[a]);
                    const uint16_t *wp = i > a + 1 ? wsym_before.data() : nullptr;
                    for (uint32_t e = 0; e < kGzWindow; e++)
                        wsym[e] = MEM ? gz_window_entry_sym_members(sp, off[i] - off[i - 1], wp, e, off[i], m0[i]) : gz_window_entry_sym(sp, off[i] - off[i - 1], wp, e);
                    for (uint32_t e = 0; e < kGzWindow; e++) win[e] = gz_window_resolve(wsym[e], a ? entry.data() : nullptr);
                }
                const std::vector<uint8_t> &w = i > a ? win : entry;
                if (i == e0[r + 1]) next_entry = w;
                if (i >= b || i < done) continue;
                const uint64_t k = P.chain[i];
                uint32_t c = 0xFFFFFFFFu;
                for (uint64_t p = off[i]; p < off[i + 1]; p++) {
                    const uint32_t x = gz_narrow(sym[p - off[a]], i ? w.data() : nullptr, off[i], MEM ? m0[i] : 0);
                    if (x > 0xFFu) { status = gz_decline(v, BZ_MARKER, k, G.d_off + (P.start[k] >> 3)); break; }
                    out[p] = (uint8_t)x;
                    c = T->crc_tab[(c ^ x) & 0xFFu] ^ (c >> 8);
                }
                crc_part[i] = off[i + 1] > off[i] ? ~c : 0u;
            }
            done = std::max(done, b);
            entry.swap(next_entry);
        }
        if (status == CRASS_OK && done != n) status = CRASS_ERR_STATE;      // (never expected: tiling ranges leave no element out)
        if (!MEM) {
            uint32_t crc = 0;
            for (uint64_t i = 0; i < n; i++) crc = gz_crc_join(crc, crc_part[i], off[i + 1] - off[i]);
            if (status == CRASS_OK && crc != P.M.crc) status = gz_decline(v, BZ_CRC, 0, 0);
        } else if (status == CRASS_OK) {
            // the member table, the pieces (cut also where a range's own text begins), every member's CRC-32 joined from them
            const uint64_t nm = slot[n], total = off[n];
            std::vector<uint64_t> in_off(nm + 1, 0), text_off(nm + 1, 0), piece(nm + total / kGzCrcPiece + base.size() + 2, 0);
            std::vector<uint32_t> mcrc(nm, 0), misz(nm, 0), got(nm, 0);
            gz_member_table(P.M, n_bytes, off.data(), slot.data(), n, ends.data(), in_off.data(), text_off.data(), mcrc.data(), misz.data());
            for (uint64_t m = 0; m < nm && status == CRASS_OK; m++)
                if (text_off[m + 1] < text_off[m] || text_off[m + 1] > total) status = CRASS_ERR_STATE;      // (a record nobody wrote)
            if (status == CRASS_OK) {
                const uint64_t np = gz_crc_pieces(text_off.data(), nm, base.data(), base.size(), piece.data());
                uint64_t q = 0;
                for (uint64_t m = 0; m < nm; m++)
                    for (; q < np && piece[q] < text_off[m + 1]; q++) {
                        uint32_t c = 0xFFFFFFFFu;
                        for (uint64_t p = piece[q]; p < piece[q + 1]; p++) c = T->crc_tab[(c ^ out[p]) & 0xFFu] ^ (c >> 8);
                        got[m] = gz_crc_join(got[m], ~c, piece[q + 1] - piece[q]);
                    }
                GzVerdict mv{};
                if (gz_member_verdict(nm, in_off.data(), text_off.data(), mcrc.data(), misz.data(), got.data(), &mv) != BZ_OK)
                    status = gz_decline(v, mv.reason, mv.member, mv.in_pos);
                else status = gz_members_fill(members, nm, in_off.data(), text_off.data());
            }
        }
    } catch (const std::bad_alloc &) { status = CRASS_ERR_OOM; }
    delete T;
    return status;
}

extern "C" {

int crass_gzip_inflate_ranges_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint32_t n_ranges, const uint64_t *nominal, uint8_t *out,
                                   uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v)
{
    if (n_ranges < 1 || n_ranges > 64) {
        if (v) memset(v, 0, sizeof(*v));
        if (plan) memset(plan, 0, sizeof(*plan));
        if (n_text) *n_text = 0;
        return CRASS_ERR_INVALID_ARG;
    }
    return gz_inflate_ranges_host<false>(bytes, n_bytes, chunk_bytes, n_ranges, nominal, out, out_cap, n_text, plan, nullptr, v);
}

int crass_gzip_inflate_members_ranges_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint32_t n_ranges, const uint64_t *nominal,
                                           uint8_t *out, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members,
                                           crass_bgzf_verdict *v)
{
    if (n_ranges < 1 || n_ranges > 64) {
        if (v) memset(v, 0, sizeof(*v));
        if (plan) memset(plan, 0, sizeof(*plan));
        if (members) memset(members, 0, sizeof(*members));
        if (n_text) *n_text = 0;
        return CRASS_ERR_INVALID_ARG;
    }
    return gz_inflate_ranges_host<true>(bytes, n_bytes, chunk_bytes, n_ranges, nominal, out, out_cap, n_text, plan, members, v);
}

void crass_gzip_plan_free(crass_gzip_plan *p)
{
    if (!p) return;
    free(p->start_bit); free(p->link); free(p->text_len);
    p->start_bit = nullptr; p->link = nullptr; p->text_len = nullptr; p->n_chunks = 0; p->n_chain = 0;
}

int crass_gzip_inflate_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_text,
                            crass_gzip_plan *plan, crass_bgzf_verdict *v)
{
    return gz_inflate_host<false>(bytes, n_bytes, chunk_bytes, out, out_cap, n_text, plan, nullptr, v);
}

void crass_gzip_members_free(crass_gzip_members *m)
{
    if (!m) return;
    free(m->in_off); free(m->text_off);
    m->in_off = nullptr; m->text_off = nullptr; m->n_members = 0;
}

int crass_gzip_inflate_members_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_text,
                                    crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v)
{
    return gz_inflate_host<true>(bytes, n_bytes, chunk_bytes, out, out_cap, n_text, plan, members, v);
}

} // extern "C"

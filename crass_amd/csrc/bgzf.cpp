// bgzf.cpp — BGZF on the host: the walk over the members' headers and trailers (the restatement of bgzf_walk, host_inflate.cpp, that
// also notes where every member's deflate data starts), and the inflate of inflate_core.h member after member: what the kernel
// (inflate.hip) is tested against, itself tested against zlib.  Host-only C++17 that any compiler builds (tools/sanitize).
#include "../../include/crass_hip.h"
#include "inflate_core.h"

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace crass {

// the host's way through the core: one executor, one index after the other
struct BzHostIO {
    const uint8_t *src; uint32_t n_in; uint8_t *dst; uint32_t isize;
    uint32_t in(uint32_t i) const { return i < n_in ? src[i] : 0u; }
    void put(uint32_t p, uint32_t b) { if (p < isize) dst[p] = (uint8_t)b; }
    uint32_t get(uint32_t p) const { return p < isize ? dst[p] : 0u; }
    template <class F> void par(uint32_t n, F f) { for (uint32_t i = 0; i < n; i++) f(i); }
    bool lead() const { return true; }
    void sync() {}
};

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// what both inflate calls check before they touch a byte: ascending offsets inside the input, deflate data between a member's
// start and its trailer, at most 64 KB of text per member, room for the text
int bgzf_index_check(const crass_bgzf_index *ix, uint64_t n_bytes, uint64_t out_cap)
{
    if (!ix) return CRASS_ERR_INVALID_ARG;
    const uint64_t n = ix->n_members;
    if (n == 0) return CRASS_OK;
    if (!ix->in_off || !ix->out_off || !ix->data_off) return CRASS_ERR_INVALID_ARG;
    if (ix->in_off[n] > n_bytes || ix->out_off[n] > out_cap) return CRASS_ERR_INVALID_ARG;
    for (uint64_t m = 0; m < n; m++) {
        const uint64_t a = ix->in_off[m], b = ix->in_off[m + 1], d = ix->data_off[m];
        if (a > b || b > n_bytes || d < a || b - a < 8 || d > b - 8 || b - d > 65536 + 8) return CRASS_ERR_INVALID_ARG;
        if (ix->out_off[m] > ix->out_off[m + 1] || ix->out_off[m + 1] - ix->out_off[m] > kBzMaxText) return CRASS_ERR_INVALID_ARG;
    }
    return CRASS_OK;
}

} // namespace crass

using namespace crass;

extern "C" {

int crass_bgzf_index_host(const uint8_t *in, uint64_t csz, crass_bgzf_index *out)
{
    if (!out || (csz && !in)) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    std::vector<uint64_t> ioff, ooff, doff;
    auto decline = [&](uint64_t pos) {
        out->decline.reason = BZ_NOT_BGZF; out->decline.member = ioff.size(); out->decline.in_pos = pos;
        return CRASS_ERR_UNSUPPORTED;
    };
    try {
        uint64_t p = 0, o = 0;
        if (csz == 0) return decline(0);                      // (no member at all)
        while (p < csz) {
            if (csz - p < 28) return decline(p);              // 12 + 6 header bytes, at least 2 of deflate data, 8 of trailer
            if (in[p] != 0x1f || in[p + 1] != 0x8b || in[p + 2] != 8 || !(in[p + 3] & 4)) return decline(p);
            const uint64_t xlen = (uint64_t)in[p + 10] | ((uint64_t)in[p + 11] << 8);
            if (p + 12 + xlen > csz) return decline(p);
            uint64_t total = 0;
            for (uint64_t q = p + 12; q + 4 <= p + 12 + xlen;) {
                const uint64_t slen = (uint64_t)in[q + 2] | ((uint64_t)in[q + 3] << 8);
                if (in[q] == 'B' && in[q + 1] == 'C' && slen == 2 && q + 6 <= p + 12 + xlen) total = ((uint64_t)in[q + 4] | ((uint64_t)in[q + 5] << 8)) + 1;
                q += 4 + slen;
            }
            if (total < 12 + xlen + 10 || p + total > csz) return decline(p);
            const uint32_t isz = le32(in + p + total - 4);
            if (isz > kBzMaxText) return decline(p);
            // where the deflate data starts: behind the extra field and whatever else the flags announce (RFC 1952 2.3: a file
            // name, a comment, a header CRC), all of it inside the member.  This is the one place where the index is STRICTER
            // than bgzf_walk, which never looks at these flags (its inflate parses the header again): a member whose name,
            // comment or header CRC run into the trailer is accepted there and declined here, because the device needs data_off
            uint64_t d = p + 12 + xlen;
            const uint64_t end = p + total - 8;
            for (int bit = 3; bit <= 4; bit++)
                if (in[p + 3] & (1 << bit)) {
                    while (d < end && in[d]) d++;
                    if (d >= end) return decline(p);
                    d++;
                }
            if (in[p + 3] & 2) d += 2;
            if (d > end) return decline(p);
            ioff.push_back(p); ooff.push_back(o); doff.push_back(d);
            p += total; o += isz;
        }
        ioff.push_back(p); ooff.push_back(o);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    const uint64_t n = doff.size();
    out->in_off = (uint64_t *)malloc((n + 1) * 8); out->out_off = (uint64_t *)malloc((n + 1) * 8); out->data_off = (uint64_t *)malloc((n ? n : 1) * 8);
    if (!out->in_off || !out->out_off || !out->data_off) { crass_bgzf_index_free(out); return CRASS_ERR_OOM; }
    memcpy(out->in_off, ioff.data(), (n + 1) * 8); memcpy(out->out_off, ooff.data(), (n + 1) * 8); memcpy(out->data_off, doff.data(), n * 8);
    out->n_members = n;
    return CRASS_OK;
}

void crass_bgzf_index_free(crass_bgzf_index *ix)
{
    if (!ix) return;
    free(ix->in_off); free(ix->out_off); free(ix->data_off);
    ix->in_off = ix->out_off = ix->data_off = nullptr; ix->n_members = 0;
}

int crass_bgzf_inflate_host(const uint8_t *bytes, uint64_t n_bytes, const crass_bgzf_index *ix, uint8_t *out, uint64_t out_cap, crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    const int chk = bgzf_index_check(ix, n_bytes, out_cap);
    if (chk) return chk;
    const uint64_t n = ix->n_members;
    if (n && (!bytes || (ix->out_off[n] && !out))) return CRASS_ERR_INVALID_ARG;
    BzTables *T = new (std::nothrow) BzTables;
    if (!T) return CRASS_ERR_OOM;
    BzHostIO io0{nullptr, 0, nullptr, 0};
    bz_prepare(io0, *T);
    int status = CRASS_OK;
    for (uint64_t m = 0; m < n; m++) {
        const uint64_t trailer = ix->in_off[m + 1] - 8;
        const uint32_t isize = (uint32_t)(ix->out_off[m + 1] - ix->out_off[m]);
        BzHostIO io{bytes + ix->data_off[m], (uint32_t)(trailer - ix->data_off[m]), isize ? out + ix->out_off[m] : nullptr, isize};
        int32_t why = bz_inflate_member(io, *T, io.n_in, isize);
        if (why == BZ_OK && bz_text_crc(io, *T, isize) != le32(bytes + trailer)) why = BZ_CRC;
        if (why != BZ_OK) {                                   // (the first offending member: the smallest offence)
            if (v) { v->reason = why; v->member = m; v->in_pos = ix->in_off[m]; }
            status = CRASS_ERR_UNSUPPORTED;
            break;
        }
    }
    delete T;
    return status;
}

} // extern "C"

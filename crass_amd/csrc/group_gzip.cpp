// group_gzip.cpp — one plain gzip file inflated across the ranks of a group (crass_hip_group_inflate_gzip and its members form;
// gunzip_ranges.h has one rank's steps): rank 0's steps between the barriers, one rank's part of the job, the job as a files
// load runs it on each of its gzip files (group_files.cpp), and a file's verdict and counters, stated once for both.
#include "group_internal.h"

using namespace grp;

namespace {

// rank 0 behind the count step: the chain, the text's size, every rank's elements.  A decline or a text that does not fit ends
// the job there (J.go stays false, J.status says why)
int gzip_chain_host(crass_hip_group *g)
{
    auto &J = g->GZ;
    crass::GzRangesFile &Z = *J.zp;
    const uint64_t nc = Z.M.G.nc;
    Z.chain.assign(nc, 0);
    const int32_t bad = crass::gz_chain(Z.M, Z.start.data(), Z.link.data(), Z.text_len.data(), Z.end_bit.data(), Z.reason.data(), Z.chain.data(),
                                        &Z.n_chain, &Z.n_text, &J.v, Z.members);
    if (bad != crass::BZ_OK) { J.status = CRASS_ERR_UNSUPPORTED; return CRASS_OK; }
    if (J.do_inflate && J.out_cap < Z.n_text) { J.status = CRASS_ERR_OVERFLOW; return CRASS_OK; }
    const uint64_t n = Z.n_chain;
    Z.off.assign(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) Z.off[i + 1] = Z.off[i] + Z.text_len[Z.chain[i]];
    Z.crc_part.assign(n, 0);
    if (Z.members) {                                    // the places of the GzEnd records and every element's member start
        Z.slot.assign(n + 1, 0); Z.m0.assign(n, 0);
        crass::gz_places(Z.chain.data(), n, Z.text_len.data(), Z.n_ends.data(), Z.last_end.data(), Z.off.data(), Z.slot.data(), Z.m0.data());
        Z.ends.assign(Z.slot[n], crass::GzEnd{0, 0, 0, 0});
        Z.table_ok = false; Z.n_pieces = 0;
    }
    if (!J.do_inflate) return CRASS_OK;                 // (a files load: the ranges follow once the cuts are known)
    const uint32_t N = (uint32_t)g->n;
    Z.e0.assign(N + 1, n); Z.e1.assign(N + 1, n); Z.first.assign(N + 1, 0);
    if (!crass::gz_ranges(Z.off.data(), n, N, J.nominal, Z.e0.data(), Z.e1.data())) { J.status = CRASS_ERR_INVALID_ARG; return CRASS_OK; }
    for (uint32_t r = 0; r < N; r++) Z.first[r + 1] = std::max(Z.first[r], Z.e1[r]);
    J.go = true;
    return CRASS_OK;
}

// ... behind the decode step: every rank's entry window, composed in rank order from what the rank in front exported (a rank
// without elements of its own, or one that starts in the same element, passes its entry window on)
void gzip_compose_host(crass_hip_group *g)
{
    crass::GzRangesFile &Z = *g->GZ.zp;
    Z.entry[0].clear();
    for (int r = 0; r + 1 < g->n; r++) {
        if (Z.e0[r + 1] >= Z.n_chain) { Z.entry[r + 1].clear(); continue; }      // (no elements: nothing to enter)
        if (Z.exported[r].empty()) { Z.entry[r + 1] = Z.entry[r]; continue; }
        const uint8_t *in = Z.entry[r].empty() ? nullptr : Z.entry[r].data();
        Z.entry[r + 1].resize(crass::kGzWindow);
        for (uint32_t w = 0; w < crass::kGzWindow; w++) Z.entry[r + 1][w] = crass::gz_window_resolve(Z.exported[r][w], in);
    }
}

// ... in members mode, behind the composition: the member table from the gathered GzEnd records (every element's from its first
// holder) and the text cuts of the CRC pieces, cut also where a rank's own text begins; the exported windows that held no
// reference are counted (a range that holds a member boundary exports such a window: its dead entries read 0)
void gzip_members_host(crass_hip_group *g)
{
    crass::GzRangesFile &Z = *g->GZ.zp;
    const uint64_t n = Z.n_chain, nm = Z.slot[n];
    Z.exported_plain = 0;
    for (int r = 0; r + 1 < g->n; r++) {
        if (Z.exported[r].empty()) continue;
        bool plain = true;
        for (uint16_t w : Z.exported[r]) if (w >= 0x8000u) { plain = false; break; }
        Z.exported_plain += plain;
    }
    Z.table_ok = false; Z.n_pieces = 0;
    if (nm == 0) return;                                // (never expected: the chain ends behind a final block)
    Z.in_off.assign(nm + 1, 0); Z.text_off.assign(nm + 1, 0); Z.mcrc.assign(nm, 0); Z.misz.assign(nm, 0);
    crass::gz_member_table(Z.M, Z.n_bytes, Z.off.data(), Z.slot.data(), n, Z.ends.data(), Z.in_off.data(), Z.text_off.data(), Z.mcrc.data(), Z.misz.data());
    for (uint64_t m = 0; m < nm; m++) if (Z.text_off[m + 1] < Z.text_off[m] || Z.text_off[m + 1] > Z.n_text) return;      // (a record nobody wrote)
    if (Z.text_off[nm] != Z.n_text) return;
    std::vector<uint64_t> base;
    for (int r = 0; r < g->n; r++) {
        const uint64_t f = std::max(Z.e0[r], Z.first[r]);
        if (f < Z.e1[r]) base.push_back(Z.off[f]);
    }
    Z.piece.assign(nm + Z.n_text / crass::kGzCrcPiece + base.size() + 2, 0);
    Z.n_pieces = crass::gz_crc_pieces(Z.text_off.data(), nm, base.data(), base.size(), Z.piece.data());
    Z.crc_piece.assign(Z.n_pieces ? Z.n_pieces : 1, 0);
    Z.table_ok = true;
}

// ... at the end: every member's CRC-32 joined from its pieces, the first offending member (7 / 8 before 9)
int32_t gzip_members_verdict(const crass::GzRangesFile &Z, crass::GzVerdict *v)
{
    const uint64_t nm = Z.in_off.size() - 1;
    std::vector<uint32_t> got(nm, 0);
    uint64_t q = 0;
    for (uint64_t m = 0; m < nm; m++)
        for (; q < Z.n_pieces && Z.piece[q] < Z.text_off[m + 1]; q++) got[m] = crass::gz_crc_join(got[m], Z.crc_piece[q], Z.piece[q + 1] - Z.piece[q]);
    return crass::gz_member_verdict(nm, Z.in_off.data(), Z.text_off.data(), Z.mcrc.data(), Z.misz.data(), got.data(), v);
}

// the smallest element with an unresolved marker over the ranks (~0: none)
uint64_t gzip_first_marker(const crass::GzRangesFile &Z)
{
    uint64_t bad = ~0ull;
    for (uint64_t b : Z.bad) bad = std::min(bad, b);
    return bad;
}

} // namespace

int grp::gzip_file_verdict(const crass::GzRangesFile &Z, crass::GzVerdict *v)
{
    *v = crass::GzVerdict{};
    const uint64_t bad = gzip_first_marker(Z);
    if (bad != ~0ull) { const uint64_t k = Z.chain[bad]; *v = crass::GzVerdict{crass::BZ_MARKER, k, Z.M.G.d_off + (Z.start[k] >> 3)}; return CRASS_OK; }
    if (Z.members) {
        if (!Z.table_ok) return CRASS_ERR_STATE;
        crass::GzVerdict mv{};
        if (gzip_members_verdict(Z, &mv) != crass::BZ_OK) *v = mv;
        return CRASS_OK;
    }
    uint32_t crc = 0;                                   // every part from the first rank that holds it
    for (uint64_t i = 0; i < Z.n_chain; i++) crc = crass::gz_crc_join(crc, Z.crc_part[i], Z.off[i + 1] - Z.off[i]);
    if (crc != Z.M.crc) v->reason = crass::BZ_CRC;
    return CRASS_OK;
}

void grp::gzip_count_file(crass_hip_group *g, const crass::GzRangesFile &Z)
{
    auto &J = g->GZ;
    uint64_t held = 0;
    for (int r = 0; r < g->n; r++) held += Z.e1[r] - Z.e0[r];
    J.cnt[0] += 1; J.cnt[1] += Z.M.G.nc; J.cnt[2] += Z.n_chain; J.cnt[3] += held - Z.n_chain;
    if (!Z.members || !Z.table_ok || gzip_first_marker(Z) != ~0ull) return;      // (the verdict did not reach the member table)
    J.cnt_members[0] += 1; J.cnt_members[1] += Z.in_off.size() - 1; J.cnt_members[2] += Z.n_pieces; J.cnt_members[3] += Z.exported_plain;
}

void grp::gzip_count_uploads(crass_hip_group *g)
{
    auto &J = g->GZ;
    std::vector<std::pair<uint64_t, uint64_t>> all;
    uint64_t sent = 0, distinct = 0, reach = 0;
    for (const auto &up : J.up) for (const auto &u : up) { sent += u.second - u.first; all.push_back(u); }
    std::sort(all.begin(), all.end());
    for (const auto &u : all) { if (u.second > reach) { distinct += u.second - std::max(u.first, reach); reach = u.second; } }
    J.cnt[4] = sent; J.cnt[5] = sent - distinct;
}

void grp::gzip_reset_reports(crass_hip_group *g)
{
    auto &J = g->GZ;
    const size_t N = (size_t)g->n;
    for (crass_hip_ctx *c : g->ctx) gzip_kept_report(c, nullptr, nullptr, true);
    J.ms.assign(N, std::array<float, 6>{}); J.up.assign(N, {}); J.tail_ms.assign(N, 0.0f); J.tail_el.assign(N, 0); J.crc_ms.assign(N, 0.0f);
}

bool grp::gzip_file_init(crass::GzRangesFile &Z, const uint8_t *bytes, uint64_t n_bytes, uint32_t n_ranks, uint64_t chunk_bytes, bool members)
{
    Z = crass::GzRangesFile();
    Z.bytes = bytes; Z.n_bytes = n_bytes; Z.n_ranks = n_ranks; Z.members = members;
    if (crass::gz_parse_member(bytes, n_bytes, n_bytes >= 8 ? bytes + n_bytes - 8 : nullptr, n_bytes, chunk_bytes, &Z.M) != crass::BZ_OK) return false;
    const uint64_t nc = Z.M.G.nc;
    Z.start.assign(nc, crass::kGzNoStart); Z.text_len.assign(nc, 0); Z.end_bit.assign(nc, 0);
    Z.link.assign(nc, crass::GZ_LINK_NONE); Z.reason.assign(nc, 0);
    if (members) { Z.n_ends.assign(nc, 0); Z.last_end.assign(nc, 0); }
    return true;
}

void grp::gzip_inflate_rank(crass_hip_group *g, int r)
{
    auto &J = g->GZ;
    crass_hip_ctx *c = g->ctx[r];
    crass::GzRangesFile &Z = *J.zp;
    if (J.do_index) {
        if (job_ok(g)) note(g, r, gzip_rank_find(c, Z, (uint32_t)r));
        g->bar->wait();                                 // every chunk's start is there
        if (job_ok(g)) note(g, r, gzip_rank_count(c, Z, (uint32_t)r));
        g->bar->wait();                                 // ... and what its run counted
        rank0_step(g, r, [&] { return gzip_chain_host(g); });
        g->bar->wait();                                 // the chain and the ranges, or the end of the job
    }
    if (J.do_inflate) {
        if (job_ok(g) && J.go) note(g, r, gzip_rank_decode(c, Z, (uint32_t)r));
        g->bar->wait();                                 // every rank's exported window
        if (J.go) rank0_step(g, r, [&] { gzip_compose_host(g); if (Z.members) gzip_members_host(g); return CRASS_OK; });
        g->bar->wait();                                 // every rank's entry window
        if (job_ok(g) && J.go) note(g, r, gzip_rank_finish(c, Z, (uint32_t)r, J.out, !J.do_index));
    }
    gzip_rank_report(c, J.ms[r].data(), &J.up[r]);
    if (J.do_inflate && (size_t)r < J.crc_ms.size()) J.crc_ms[r] = gzip_rank_member_crc_ms(c);
    if (J.do_index && J.do_inflate) gzip_rank_release(c);      // (a files load keeps the staged bytes and gives all scratch back at its end)
}

int grp::gzip_job_run(crass_hip_group *g, crass::GzRangesFile &Z, bool index, bool inflate, uint8_t *out, uint64_t out_cap, const uint64_t *nominal)
{
    auto &J = g->GZ;
    const size_t N = (size_t)g->n;
    J.zp = &Z; J.do_index = index; J.do_inflate = inflate;
    J.out = out; J.out_cap = out_cap; J.nominal = nominal; J.status = CRASS_OK;
    if (index) J.v = crass::GzVerdict{};
    if (inflate) { Z.exported.assign(N, {}); Z.entry.assign(N, {}); Z.bad.assign(N, ~0ull); }
    J.go = !index;                                      // (behind an index step rank 0 decides: gzip_chain_host)
    return dispatch(g, PH_INFLATE_GZIP);
}

static int group_inflate_gzip(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal, uint8_t *out_host,
                              uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, bool mem, crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    if (plan) memset(plan, 0, sizeof(*plan));
    if (members) memset(members, 0, sizeof(*members));
    if (n_text) *n_text = 0;
    if (!g || !n_text || (n_bytes && !bytes) || (out_cap && !out_host)) return CRASS_ERR_INVALID_ARG;
    auto &J = g->GZ;
    for (auto &x : J.cnt) x = 0;
    for (auto &x : J.cnt_members) x = 0;
    auto decline = [&](const crass::GzVerdict &d) {
        if (v) { v->reason = d.reason; v->member = d.member; v->in_pos = d.in_pos; }
        return CRASS_ERR_UNSUPPORTED;
    };
    try {
        crass::GzRangesFile &Z = J.Z;
        gzip_reset_reports(g);
        if (!gzip_file_init(Z, bytes, n_bytes, (uint32_t)g->n, chunk_bytes, mem)) return decline(crass::GzVerdict{crass::BZ_NOT_GZIP, 0, 0});
        const int st = gzip_job_run(g, Z, true, true, out_host, out_cap, nominal);
        if (st) return st;
        const int ps = crass::gz_plan_fill(plan, Z.M.G.nc, Z.start.data(), Z.link.data(), Z.text_len.data(), Z.n_chain);
        if (ps) return ps;
        if (J.status == CRASS_ERR_UNSUPPORTED) return decline(J.v);
        if (J.status == CRASS_ERR_INVALID_ARG) return J.status;
        *n_text = Z.n_text;
        if (J.status) return J.status;                  // (the text does not fit: known before anything is stored)
        gzip_count_file(g, Z);
        gzip_count_uploads(g);
        crass::GzVerdict fv{};
        const int vs = gzip_file_verdict(Z, &fv);
        if (vs) return vs;
        if (fv.reason) return decline(fv);
        if (mem) return crass::gz_members_fill(members, Z.in_off.size() - 1, Z.in_off.data(), Z.text_off.data());
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

extern "C" {

int crass_hip_group_inflate_gzip(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal,
                                 uint8_t *out_host, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v)
{
    return group_inflate_gzip(g, bytes, n_bytes, chunk_bytes, nominal, out_host, out_cap, n_text, plan, nullptr, false, v);
}

int crass_hip_group_inflate_gzip_members(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal,
                                         uint8_t *out_host, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members,
                                         crass_bgzf_verdict *v)
{
    return group_inflate_gzip(g, bytes, n_bytes, chunk_bytes, nominal, out_host, out_cap, n_text, plan, members, true, v);
}

int crass_hip_group_gzip_members_counters(const crass_hip_group *g, uint64_t out[4])
{
    if (!g || !out) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = g->GZ.cnt_members[k];
    return CRASS_OK;
}

int crass_hip_group_gzip_members_ms(const crass_hip_group *g, int rank, float out[1])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    out[0] = (size_t)rank < g->GZ.crc_ms.size() ? g->GZ.crc_ms[rank] : 0.0f;
    return CRASS_OK;
}

int crass_hip_group_set_gzip_on_device(crass_hip_group *g, int mode, uint64_t chunk_bytes)
{
    if (!g || mode < 0) return CRASS_ERR_INVALID_ARG;
    g->gzip_mode = mode == CRASS_GZIP_ON_DEVICE_MEMBERS ? CRASS_GZIP_ON_DEVICE_MEMBERS : mode ? CRASS_GZIP_ON_DEVICE_ONE_MEMBER : CRASS_GZIP_ON_DEVICE_OFF;
    g->gzip_chunk = chunk_bytes ? crass::gz_chunk_bytes(chunk_bytes) : 0;
    return CRASS_OK;
}

int crass_hip_group_gzip_counters(const crass_hip_group *g, uint64_t out[6])
{
    if (!g || !out) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 6; k++) out[k] = g->GZ.cnt[k];
    return CRASS_OK;
}

int crass_hip_group_gzip_ms(const crass_hip_group *g, int rank, float out[7])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 6; k++) out[k] = (size_t)rank < g->GZ.ms.size() ? g->GZ.ms[rank][k] : 0.0f;
    out[6] = (size_t)rank < g->GZ.tail_ms.size() ? g->GZ.tail_ms[rank] : 0.0f;
    return CRASS_OK;
}

} // extern "C"

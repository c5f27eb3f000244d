// group_fetch.cpp — text, header lines, quality strings and handed comments of reads of the whole job: every index goes to the
// rank whose shard holds it, one fetch per rank that has any, and the records are put back in the caller's order (group_route.h
// has the routing and the gathering; the fetches differ in the index base and in where one record's bytes come from).
#include "group_internal.h"

using namespace grp;

namespace {

Span span_of(const crass_text &t, size_t q) { return Span{t.chars + t.off[q], t.off[q + 1] - t.off[q]}; }

// what every fetch begins with: the arguments, the load it needs, every index inside the job
int check_fetch(const crass_hip_group *g, const crass_text *o, const uint64_t *read_idx, uint64_t n, bool files, uint64_t base)
{
    if (!g || !o || (n && !read_idx)) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded || (files && !g->files_load)) return CRASS_ERR_STATE;
    for (uint64_t k = 0; k < n; k++) if (read_idx[k] < base || read_idx[k] - base >= g->n_reads) return CRASS_ERR_INVALID_ARG;
    return CRASS_OK;
}

// fetch(r, &part[r]) on every rank that has an index.  (A rank's result lives in its own context until that context's next
// fetch of the kind: all of them are there at once)
template <typename F> int fetch_per_rank(const Route &R, std::vector<crass_text> &part, F fetch)
{
    part.assign(R.idx.size(), crass_text{0, nullptr, nullptr});
    for (size_t r = 0; r < R.idx.size(); r++) {
        if (R.idx[r].empty()) continue;
        const int s = fetch((int)r, &part[r]);
        if (s) return s;
    }
    return CRASS_OK;
}

int give(const Text &T, uint64_t n, crass_text *o) { o->n = n; o->chars = T.chars.data(); o->off = T.off.data(); return CRASS_OK; }

// header lines (quality == false) or quality strings: each rank fetches from its own arena, by local indices
int group_fetch_lines(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, bool quality, crass_text *o, uint32_t *name_len_out, uint8_t *has_qual_out)
{
    int s = check_fetch(g, o, read_idx, n, true, 0);
    if (s) return s;
    Text &T = quality ? g->TQ : g->TH;
    try {
        Route R;
        route(g->first, 0, read_idx, n, true, &R);
        std::vector<crass_text> part;
        std::vector<uint32_t> nl;
        std::vector<uint8_t> hq;
        s = fetch_per_rank(R, part, [&](int r, crass_text *t) -> int {
            const uint64_t m = R.idx[r].size();
            const uint8_t *arena = nullptr; const uint64_t *rec_pos = nullptr; uint64_t nb = 0, nr = 0;
            int fs = shard_records(g->ctx[r], &arena, &nb, &rec_pos, &nr);
            if (fs) return fs;
            nl.resize(m); hq.resize(m);
            fs = quality ? crass_hip_fetch_quality_device(g->ctx[r], arena, nb, rec_pos, nr, R.idx[r].data(), m, t, hq.data())
                         : crass_hip_fetch_header_lines_device(g->ctx[r], arena, nb, rec_pos, nr, R.idx[r].data(), m, t, nl.data());
            if (fs) return fs;
            if (quality) scatter(R.at[r], hq.data(), has_qual_out); else scatter(R.at[r], nl.data(), name_len_out);
            return CRASS_OK;
        });
        if (s) return s;
        gather(R, n, [&](size_t r, size_t q) { return span_of(part[r], q); }, &T);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return give(T, n, o);
}

// what the cuts of a files load carry (include/crass_hip.h): rank after rank in file order, each rank "publishes" the comment handed
// to its LAST record — the own comment of the last own-comment record of the file part its shard ends in, a host string — and
// is handed what the ranks in front of it left for the file its shard begins in.  Empty ranks, and ranks that are one part of
// one file without a comment, pass it through; nothing crosses a file boundary.
int group_comments_resolve(crass_hip_group *g)
{
    auto &J = g->F;
    auto &CM = g->CM;
    const int N = g->n;
    CM.in.assign(N, std::string()); CM.has.assign(N, 0); CM.first_n.assign(N, 0);
    bool carried = false; std::string text; int64_t file = -1;      // what the ranks so far leave, and for which file
    for (int r = 0; r < N; r++) {
        const uint64_t nr = g->first[r + 1] - g->first[r];
        if (!nr) continue;
        int64_t f0 = -1, fl = -1; size_t parts = 0;
        for (const auto &fr : J.file_reads[r]) if (fr.second) { if (f0 < 0) { f0 = fr.first; CM.first_n[r] = fr.second; } fl = fr.first; parts++; }
        if (carried && file == f0) { CM.in[r] = text; CM.has[r] = 1; }
        const uint64_t last = nr - 1;
        crass_text t; uint8_t has = 0;
        const int s = crass_hip_fetch_comments_device(g->ctx[r], &last, 1, &t, &has);
        if (s) return s;
        if (has) { carried = true; text.assign((const char *)t.chars + t.off[0], (size_t)(t.off[1] - t.off[0])); }
        else if (!(parts == 1 && file == f0)) { carried = false; text.clear(); }      // (else: one part of the file the carry belongs to)
        file = fl;
    }
    CM.ready = true;
    return CRASS_OK;
}

} // namespace

extern "C" {

// (a shard's read_index_base is the job's plus its first read, so the global indices pass through as they are)
int crass_hip_group_fetch_text(crass_hip_group *g, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, crass_text *o)
{
    int s = check_fetch(g, o, read_idx, n, false, g ? g->base : 0);
    if (s) return s;
    try {
        Route R;
        route(g->first, g->base, read_idx, n, false, &R);
        std::vector<crass_text> part;
        std::vector<std::vector<uint8_t>> rc(g->n);
        s = fetch_per_rank(R, part, [&](int r, crass_text *t) -> int {
            for (uint64_t k : R.at[r]) if (revcomp) rc[r].push_back(revcomp[k]);
            return crass_hip_fetch_text(g->ctx[r], R.idx[r].data(), revcomp ? rc[r].data() : nullptr, R.idx[r].size(), t);
        });
        if (s) return s;
        gather(R, n, [&](size_t r, size_t q) { return span_of(part[r], q); }, &g->T);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return give(g->T, n, o);
}

int crass_hip_group_fetch_header_lines(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint32_t *name_len_out)
{
    return group_fetch_lines(g, read_idx, n, false, out, name_len_out, nullptr);
}

int crass_hip_group_fetch_quality(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint8_t *has_qual_out)
{
    return group_fetch_lines(g, read_idx, n, true, out, nullptr, has_qual_out);
}

int crass_hip_group_fetch_comments(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *o, uint8_t *has_out)
{
    int s = check_fetch(g, o, read_idx, n, true, 0);
    if (s) return s;
    try {
        if (!g->CM.ready && (s = group_comments_resolve(g))) return s;
        Route R;
        route(g->first, 0, read_idx, n, true, &R);
        std::vector<crass_text> part;
        std::vector<std::vector<uint8_t>> hc(g->n), carried(g->n);      // a comment is handed; ... and it is the carried string, not the rank's own text
        s = fetch_per_rank(R, part, [&](int r, crass_text *t) -> int {
            const uint64_t m = R.idx[r].size();
            hc[r].assign(m, 0); carried[r].assign(m, 0);
            const int fs = crass_hip_fetch_comments_device(g->ctx[r], R.idx[r].data(), m, t, hc[r].data());
            if (fs) return fs;
            for (uint64_t q = 0; q < m; q++) {
                if (!hc[r][q] && g->CM.has[r] && R.idx[r][q] < g->CM.first_n[r]) hc[r][q] = carried[r][q] = 1;
                else hc[r][q] = hc[r][q] ? 1 : 0;
            }
            scatter(R.at[r], hc[r].data(), has_out);
            return CRASS_OK;
        });
        if (s) return s;
        gather(R, n, [&](size_t r, size_t q) {
            const std::string &in = g->CM.in[r];
            return carried[r][q] ? Span{(const uint8_t *)in.data(), in.size()} : span_of(part[r], q);
        }, &g->TC);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return give(g->TC, n, o);
}

} // extern "C"

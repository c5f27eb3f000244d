// group_names.cpp — found headers across the ranks of a files load (readsFound is keyed by header, libcrispr.cpp:138,411):
// installed header ids are per rank, so behind a merge every rank publishes the names of its pass-1 records, the ranks meet at a
// barrier, and every rank looks the others' names up in its own table: its namesakes are marked found before pass 2.  Two
// routes: over the host, or (crass_hip_group_set_name_exchange) with every name, answer and index in device memory.
#include "group_internal.h"

#include <chrono>

using namespace grp;

namespace {

// the host route: every rank publishes the names of its pass-1 records (its header lines, cut at the name) ...
int names_publish(crass_hip_group *g, int r)
{
    crass_hip_group::Text &NM = g->names[r];
    NM.chars.clear(); NM.off.assign(1, 0);
    crass_candidates cd;
    int s = crass_hip_get_candidates(g->ctx[r], &cd);
    if (s || !cd.n) return s;
    const uint8_t *arena = nullptr; const uint64_t *rec_pos = nullptr; uint64_t nb = 0, nr = 0;
    if ((s = shard_records(g->ctx[r], &arena, &nb, &rec_pos, &nr))) return s;
    std::vector<uint64_t> idx(cd.n);
    std::vector<uint32_t> name_len(cd.n);
    for (uint64_t k = 0; k < cd.n; k++) idx[k] = cd.read_idx[k] - g->first[r];
    crass_text t;
    if ((s = crass_hip_fetch_header_lines_device(g->ctx[r], arena, nb, rec_pos, nr, idx.data(), cd.n, &t, name_len.data()))) return s;
    for (uint64_t k = 0; k < cd.n; k++) {
        NM.chars.insert(NM.chars.end(), t.chars + t.off[k], t.chars + t.off[k] + name_len[k]);
        NM.off.push_back(NM.chars.size());
    }
    return CRASS_OK;
}

// ... and looks the other ranks' names up in its own table
int names_lookup(crass_hip_group *g, int r)
{
    std::vector<uint64_t> &e = g->extra[r];
    e.clear();
    std::vector<uint64_t> first;
    uint64_t looked = 0;
    for (int q = 0; q < g->n; q++) {
        const crass_hip_group::Text &NM = g->names[q];
        const uint64_t nq = NM.off.size() - 1;
        if (q == r || !nq) continue;
        first.resize(nq);
        const int s = crass_hip_fastx_names_find(g->ctx[r], NM.chars.data(), NM.off.data(), nq, first.data());
        if (s) return s;
        for (uint64_t k = 0; k < nq; k++) if (first[k] != CRASS_NAME_NOT_FOUND) e.push_back(first[k]);
        looked += nq;
    }
    crass_hip_group::NameX &X = g->nx[r];
    X.n_first = 0; X.first_valid = false;
    X.cnt[0] = 0; X.cnt[1] = g->names[r].off.size() - 1; X.cnt[2] = looked; X.cnt[3] = e.size();
    return CRASS_OK;
}

// ---- the same exchange on the device route: no name, answer or index crosses to the host, only counts and totals ----
// a buffer of at least `want` elements (+ extra) on the rank's device (the current device); what it held is dropped
template <typename T> int nx_grow(T *&p, uint64_t &cap, uint64_t want, uint64_t extra)
{
    if (p && cap >= want) return CRASS_OK;
    if (p) { crass::dev_free(p); p = nullptr; cap = 0; }
    void *q = nullptr;
    if (crass::dev_alloc(&q, (size_t)((want + extra) * sizeof(T))) != hipSuccess) return CRASS_ERR_OOM;
    p = (T *)q; cap = want;
    return CRASS_OK;
}

// rank r's names into its own buffer, sized from the step before (the first step: from the candidate count); too small: regrown
// to the totals the call reported and the call repeated, once
int names_publish_device(crass_hip_group *g, int r)
{
    crass_hip_group::NameX &X = g->nx[r];
    X.n = X.total = 0;
    if (hipSetDevice(g->devices[r]) != hipSuccess) return CRASS_ERR_HIP;
    crass_counters k{};
    (void)crass_hip_get_counters(g->ctx[r], &k);
    const uint64_t want_n = std::max<uint64_t>(X.cap_names, k.n_pass1_found), want_b = std::max<uint64_t>(X.cap_chars, 32 * want_n);
    int s;
    if ((s = nx_grow(X.off, X.cap_names, want_n, 1)) || (s = nx_grow(X.chars, X.cap_chars, want_b, 0))) return s;
    uint64_t n = 0, total = 0;
    s = crass_hip_found_names_device(g->ctx[r], X.chars, X.cap_chars, X.off, X.cap_names, &n, &total);
    if (s == CRASS_ERR_OVERFLOW) {
        if ((s = nx_grow(X.off, X.cap_names, n + n / 4, 1)) || (s = nx_grow(X.chars, X.cap_chars, total + total / 4, 0))) return s;
        s = crass_hip_found_names_device(g->ctx[r], X.chars, X.cap_chars, X.off, X.cap_names, &n, &total);
    }
    if (s) return s;
    X.n = n; X.total = total;
    return CRASS_OK;
}

// behind the barrier: every other rank's names and offsets to this rank's device on its stream, looked up there; the answers of
// all sources back to back in X.first.  (A source's buffers are not written again before the next step's publish, which lies
// behind that step's barriers.)
int names_lookup_device(crass_hip_group *g, int r)
{
    crass_hip_group::NameX &X = g->nx[r];
    g->extra[r].clear();
    X.n_first = 0; X.first_valid = false;
    if (hipSetDevice(g->devices[r]) != hipSuccess) return CRASS_ERR_HIP;
    hipStream_t st = (hipStream_t)crass_hip_stream(g->ctx[r]);
    uint64_t n_all = 0, found = 0, at = 0;
    for (int q = 0; q < g->n; q++) if (q != r) n_all += g->nx[q].n;
    int s;
    if ((s = nx_grow(X.first, X.cap_first, n_all, 0))) return s;
    for (int q = 0; q < g->n; q++) {
        const crass_hip_group::NameX &Q = g->nx[q];
        if (q == r || !Q.n) continue;
        if ((s = nx_grow(X.q_off, X.cap_q_names, Q.n, 1)) || (s = nx_grow(X.q_chars, X.cap_q_chars, Q.total, 0))) return s;
        hipError_t e = hipSuccess;
        if (g->local_copies || g->devices[q] == g->devices[r]) {
            e = hipMemcpyAsync(X.q_off, Q.off, (Q.n + 1) * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && Q.total) e = hipMemcpyAsync(X.q_chars, Q.chars, Q.total, hipMemcpyDeviceToDevice, st);
        } else {
            e = hipMemcpyPeerAsync(X.q_off, g->devices[r], Q.off, g->devices[q], (Q.n + 1) * 8, st);
            if (e == hipSuccess && Q.total) e = hipMemcpyPeerAsync(X.q_chars, g->devices[r], Q.chars, g->devices[q], Q.total, st);
        }
        if (e != hipSuccess) { set_error(std::string("found-name exchange, copy of rank ") + std::to_string(q) + "'s names: " + hipGetErrorString(e)); return CRASS_ERR_HIP; }
        if ((s = crass_hip_fastx_names_find_device(g->ctx[r], X.q_chars, Q.total, X.q_off, Q.n, X.first + at))) return s;
        found += names_find_device_found(g->ctx[r]);
        at += Q.n;
    }
    X.n_first = at; X.first_valid = true;
    X.cnt[0] = 1; X.cnt[1] = X.n; X.cnt[2] = at; X.cnt[3] = found;
    return CRASS_OK;
}

} // namespace

void grp::nx_free(crass_hip_group *g, int r)
{
    crass_hip_group::NameX &X = g->nx[r];
    (void)hipSetDevice(g->devices[r]);
    for (void *p : {(void *)X.chars, (void *)X.q_chars, (void *)X.off, (void *)X.q_off, (void *)X.first}) if (p) crass::dev_free(p);
    for (hipEvent_t e : X.ev) if (e) (void)hipEventDestroy(e);
    X = crass_hip_group::NameX{};
}

void grp::clear_extra(crass_hip_group *g)
{
    for (auto &e : g->extra) e.clear();
    for (auto &X : g->nx) { X.n_first = 0; X.first_valid = false; }
}

// publish, the barrier every rank passes, lookup; timed from before the publish to behind the lookup, on the wall and (timed
// groups) by two events on the rank's stream
void grp::names_exchange_rank(crass_hip_group *g, int r)
{
    const bool dev = g->names_on_device;                // (set between jobs: the same on every rank of a job)
    crass_hip_group::NameX &X = g->nx[r];
    hipStream_t st = (hipStream_t)crass_hip_stream(g->ctx[r]);
    const auto t0 = std::chrono::steady_clock::now();
    bool timed = g->names_timed && job_ok(g) && hipSetDevice(g->devices[r]) == hipSuccess;
    for (hipEvent_t &e : X.ev) if (timed && !e) timed = hipEventCreate(&e) == hipSuccess;
    if (timed) timed = hipEventRecord(X.ev[0], st) == hipSuccess;
    rank_step(g, r, [&] { return dev ? names_publish_device(g, r) : names_publish(g, r); });
    g->bar->wait();                                     // every rank's names are there
    rank_step(g, r, [&] { return dev ? names_lookup_device(g, r) : names_lookup(g, r); });
    X.event_ms = 0;
    if (timed && hipSetDevice(g->devices[r]) == hipSuccess && hipEventRecord(X.ev[1], st) == hipSuccess && hipEventSynchronize(X.ev[1]) == hipSuccess)
        (void)hipEventElapsedTime(&X.event_ms, X.ev[0], X.ev[1]);
    X.wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" {

int crass_hip_group_set_name_exchange(crass_hip_group *g, int on_device)
{
    if (!g) return CRASS_ERR_INVALID_ARG;
    g->names_on_device = on_device != 0;
    return CRASS_OK;
}

int crass_hip_group_name_exchange_ms(const crass_hip_group *g, int rank, float out[2])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    out[0] = g->nx[rank].wall_ms; out[1] = g->nx[rank].event_ms;
    return CRASS_OK;
}

int crass_hip_group_name_exchange_counters(const crass_hip_group *g, int rank, uint64_t out[4])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = g->nx[rank].cnt[k];
    return CRASS_OK;
}

} // extern "C"

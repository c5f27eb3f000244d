// group_route.h — a group's fetches (group_fetch.cpp), as host arithmetic: read indices of the whole job routed to the ranks
// whose shards hold them, and the ranks' records put back in the caller's order.  No HIP and no crass_hip_group in here:
// tools/sanitize/group_route_main.cpp checks both against the per-index loop.  Not part of the public ABI.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#pragma GCC visibility push(hidden)
namespace grp {

struct Text { std::vector<uint8_t> chars; std::vector<uint64_t> off; };      // records back to back, off[n + 1], one spare byte
struct Span { const uint8_t *p; uint64_t n; };                               // one record's bytes

// per rank: the indices of its fetch, and the place of each in the caller's order
struct Route { std::vector<std::vector<uint64_t>> idx, at; };

// read_idx[k] - base is read first[r] + i of the job (first[N + 1], not decreasing; every index below first[N]): it goes to
// rank r as i (local), or as it came (a shard whose read_index_base is the job's plus its first read)
inline void route(const std::vector<uint64_t> &first, uint64_t base, const uint64_t *read_idx, uint64_t n, bool local, Route *R)
{
    const size_t N = first.size() - 1;
    R->idx.assign(N, {}); R->at.assign(N, {});
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t i = read_idx[k] - base;
        const size_t r = (size_t)(std::upper_bound(first.begin(), first.end(), i) - first.begin()) - 1;
        R->idx[r].push_back(local ? i - first[r] : read_idx[k]); R->at[r].push_back(k);
    }
}

// what rank r's fetch said of its record q, to the record's place in the caller's order (out NULL: not asked for)
template <typename V, typename U> void scatter(const std::vector<uint64_t> &at, const V *v, U *out)
{
    for (size_t q = 0; out && q < at.size(); q++) out[at[q]] = (U)v[q];
}

// rec(r, q): the Span of rank r's record q.  Lengths to their places, prefix sum, bytes to theirs
template <typename Rec> void gather(const Route &R, uint64_t n, Rec rec, Text *T)
{
    T->off.assign(n + 1, 0);
    for (size_t r = 0; r < R.at.size(); r++) for (size_t q = 0; q < R.at[r].size(); q++) T->off[R.at[r][q] + 1] = rec(r, q).n;
    for (uint64_t k = 0; k < n; k++) T->off[k + 1] += T->off[k];
    T->chars.resize(T->off[n] + 1);
    for (size_t r = 0; r < R.at.size(); r++) for (size_t q = 0; q < R.at[r].size(); q++) {
        const Span s = rec(r, q);
        if (s.n) memcpy(T->chars.data() + T->off[R.at[r][q]], s.p, s.n);
    }
}

} // namespace grp
#pragma GCC visibility pop

// group_route_main.cpp — the router and the gatherer of a group's fetches (crass_amd/csrc/group_route.h) against the obvious
// per-index loop, on the host: 1 to 5 ranks, shards of 0, 1 and a few records in every arrangement (so that empty first, middle
// and last ranks occur), no index at all, every index once in a random order, 300 random indices with repeats, an index base of 0
// and of 77, local and global indices, and a "carried string" that stands in for some records of a rank's first part.  Exits
// non-zero on the first difference.
//   g++ -std=c++17 -Icrass_amd/csrc tools/sanitize/group_route_main.cpp -o group_route && ./group_route
#include "group_route.h"

#include <cstdio>
#include <random>
#include <string>

using namespace grp;

static std::mt19937_64 rng(20240607);

// record i of the job: a text of i % 7 bytes that names i (so records of no bytes occur)
static std::string record(uint64_t i)
{
    std::string s = std::to_string(i * 2654435761u);
    return s.substr(0, i % 7);
}

struct Job {
    std::vector<uint64_t> first;                        // [N + 1]
    std::vector<std::string> carried;                   // per rank: the string handed to the first carried_n[r] records that have none
    std::vector<uint64_t> carried_n;
    // what the per-index loop says of record i: its bytes, and a flag of the rank's fetch (here: i is odd)
    std::string bytes(uint64_t i) const
    {
        const size_t r = rank_of(i);
        if (i - first[r] < carried_n[r] && record(i).empty()) return carried[r];
        return record(i);
    }
    size_t rank_of(uint64_t i) const { size_t r = 0; while (!(first[r] <= i && i < first[r + 1])) r++; return r; }
};

static int fail(const char *what, const Job &J, uint64_t base, bool local, size_t n)
{
    printf("DIFF %s: %zu ranks, base %llu, %s indices, n %zu\n", what, J.first.size() - 1, (unsigned long long)base, local ? "local" : "global", n);
    return 1;
}

// one fetch: route, "fetch" per rank (the rank sees what route gave it), scatter a flag, gather; against the loop
static int check(const Job &J, const std::vector<uint64_t> &pick, uint64_t base, bool local)
{
    const size_t N = J.first.size() - 1, n = pick.size();
    std::vector<uint64_t> idx(n);
    for (size_t k = 0; k < n; k++) idx[k] = pick[k] + base;
    Route R;
    route(J.first, base, idx.data(), n, local, &R);
    if (R.idx.size() != N || R.at.size() != N) return fail("ranks", J, base, local, n);
    std::vector<uint8_t> seen(n, 0), flag(n, 0xEE);
    std::vector<std::vector<std::string>> part(N);      // the ranks' answers, in the order of their indices
    for (size_t r = 0; r < N; r++) {
        if (R.idx[r].size() != R.at[r].size()) return fail("sizes", J, base, local, n);
        std::vector<uint8_t> odd;
        for (size_t q = 0; q < R.idx[r].size(); q++) {
            const uint64_t i = local ? R.idx[r][q] + J.first[r] : R.idx[r][q] - base;      // the job-level index the rank was given
            const uint64_t k = R.at[r][q];
            if (k >= n || seen[k]++ || i != pick[k] || i < J.first[r] || i >= J.first[r + 1]) return fail("route", J, base, local, n);
            if (q && R.at[r][q - 1] >= k) return fail("order within a rank", J, base, local, n);
            part[r].push_back(record(i));
            odd.push_back((uint8_t)(i & 1));
        }
        scatter(R.at[r], odd.data(), flag.data());
        scatter(R.at[r], odd.data(), (uint8_t *)nullptr);
    }
    for (size_t k = 0; k < n; k++) if (!seen[k]) return fail("an index went nowhere", J, base, local, n);
    Text T;
    T.chars.assign(5, 0x55); T.off.assign(3, 9);         // (what an earlier fetch left)
    gather(R, n, [&](size_t r, size_t q) {
        const std::string &own = part[r][q];
        const uint64_t i_local = local ? R.idx[r][q] : R.idx[r][q] - base - J.first[r];
        const std::string &s = own.empty() && i_local < J.carried_n[r] ? J.carried[r] : own;
        return Span{(const uint8_t *)s.data(), s.size()};
    }, &T);
    if (T.off.size() != n + 1 || T.off[0] != 0 || T.chars.size() != T.off[n] + 1) return fail("offsets", J, base, local, n);
    for (size_t k = 0; k < n; k++) {
        const std::string want = J.bytes(pick[k]);
        if (T.off[k + 1] - T.off[k] != want.size() || memcmp(T.chars.data() + T.off[k], want.data(), want.size())) return fail("bytes", J, base, local, n);
        if (flag[k] != (pick[k] & 1)) return fail("scatter", J, base, local, n);
    }
    return 0;
}

int main()
{
    const uint64_t sizes[] = {0, 1, 4};
    uint64_t n_jobs = 0, n_checks = 0;
    for (size_t N = 1; N <= 5; N++) {
        size_t combos = 1;
        for (size_t r = 0; r < N; r++) combos *= 3;
        for (size_t c = 0; c < combos; c++) {
            Job J;
            J.first.assign(1, 0);
            for (size_t r = 0, x = c; r < N; r++, x /= 3) J.first.push_back(J.first.back() + sizes[x % 3]);
            J.carried.resize(N); J.carried_n.assign(N, 0);
            for (size_t r = 0; r < N; r++) if ((c + r) % 2) { J.carried[r] = "carried by " + std::to_string(r); J.carried_n[r] = 1 + (c + r) % 3; }
            const uint64_t total = J.first[N];
            std::vector<std::vector<uint64_t>> picks(1);      // n = 0
            if (total) {
                std::vector<uint64_t> all(total);
                for (uint64_t i = 0; i < total; i++) all[i] = i;
                std::shuffle(all.begin(), all.end(), rng);
                picks.push_back(all);
                std::vector<uint64_t> rep(300);
                for (auto &i : rep) i = rng() % total;
                picks.push_back(rep);
            }
            for (const auto &pick : picks) for (uint64_t base : {0, 77}) for (bool local : {false, true}) {
                if (check(J, pick, base, local)) return 1;
                n_checks++;
            }
            n_jobs++;
        }
    }
    printf("group_route ok: %llu jobs, %llu fetches\n", (unsigned long long)n_jobs, (unsigned long long)n_checks);
    return 0;
}

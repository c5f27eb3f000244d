// AddressSanitizer / UBSan harness for the plain-gzip host code in members mode by ranges (crass_gzip_inflate_members_ranges_host:
// csrc/gunzip.cpp + csrc/gunzip_core.h + csrc/inflate_core.h), next to gzip_members_main.cpp and gzip_ranges_main.cpp: every file
// given — the sets of tests/gzip_member_sets.py, dumped by tools/sanitize/gzip_members_dump.py — goes through the function for 1, 2,
// 3 and 7 ranges with even cuts (and, accepted, with cuts on and beside its first member boundary) at the chunk size its name
// carries (X.c<chunk>.r<reason>.gz), from an exact-size heap copy into an exact-size heap buffer, so that a read or a store one
// byte outside either is the sanitizer's to report.  Text, member table and verdict must be crass_gzip_inflate_members_host's.
// CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/gunzip.cpp \
//       tools/sanitize/gzip_members_ranges_main.cpp -o gzip_members_ranges_asan && python3 tools/sanitize/gzip_members_dump.py DIR && \
//       ./gzip_members_ranges_asan DIR/*
#include "../../include/crass_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Answer { int rc; uint64_t n_text; crass_bgzf_verdict v; std::vector<uint8_t> text; std::vector<uint64_t> in_off, text_off; };

// n_ranges 0: crass_gzip_inflate_members_host
static Answer run(const uint8_t *in, uint64_t n, uint64_t chunk, uint32_t n_ranges, const std::vector<uint64_t> &nominal, uint64_t cap)
{
    Answer A;
    memset(&A.v, 0, sizeof(A.v));
    A.n_text = 0;
    uint64_t *nom = nominal.empty() ? nullptr : (uint64_t *)malloc(nominal.size() * 8);
    if (nom) memcpy(nom, nominal.data(), nominal.size() * 8);
    uint8_t *out = cap ? (uint8_t *)malloc(cap) : nullptr;
    crass_gzip_plan plan;
    crass_gzip_members mem;
    A.rc = n_ranges ? crass_gzip_inflate_members_ranges_host(in, n, chunk, n_ranges, nom, out, cap, &A.n_text, &plan, &mem, &A.v)
                    : crass_gzip_inflate_members_host(in, n, chunk, out, cap, &A.n_text, &plan, &mem, &A.v);
    if (A.rc == CRASS_OK) {
        A.text.assign(out, out + A.n_text);
        A.in_off.assign(mem.in_off, mem.in_off + mem.n_members + 1); A.text_off.assign(mem.text_off, mem.text_off + mem.n_members + 1);
    }
    crass_gzip_plan_free(&plan); crass_gzip_members_free(&mem);
    free(out); free(nom);
    return A;
}

static bool same(const Answer &a, const Answer &b)
{
    return a.rc == b.rc && a.n_text == b.n_text && a.v.reason == b.v.reason && a.v.member == b.v.member && a.v.in_pos == b.v.in_pos && a.text == b.text &&
           a.in_off == b.in_off && a.text_off == b.text_off;
}

int main(int argc, char **argv)
{
    int bad = 0, n_runs = 0, n_declined = 0;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { printf("DIFF %s: cannot open\n", argv[a]); bad++; continue; }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + k);
        fclose(f);
        uint8_t *exact = data.empty() ? nullptr : (uint8_t *)malloc(data.size());
        if (exact) memcpy(exact, data.data(), data.size());
        long chunk = 0, want_r = -1;
        if (const char *p = strstr(argv[a], ".c")) if (sscanf(p, ".c%ld.r%ld.", &chunk, &want_r) != 2) { chunk = 0; want_r = -1; }
        const Answer size = run(exact, data.size(), (uint64_t)chunk, 0, {}, 0);          // the size alone (or the decline)
        const uint64_t T = size.n_text;
        const Answer want = size.rc == CRASS_ERR_OVERFLOW ? run(exact, data.size(), (uint64_t)chunk, 0, {}, T) : size;
        n_declined += want.rc == CRASS_ERR_UNSUPPORTED;
        std::vector<std::pair<uint32_t, std::vector<uint64_t>>> cuts = {{1, {}}, {2, {}}, {3, {}}, {7, {}}};
        if (want.rc == CRASS_OK && want.text_off.size() > 2 && want.text_off[1] > 0 && want.text_off[1] < T) {
            const uint64_t b = want.text_off[1];
            cuts.push_back({2, {b}}); cuts.push_back({3, {b - 1, b + 1}}); cuts.push_back({4, {0, b, T}});
        }
        int diffs = 0;
        for (const auto &q : cuts) {
            // (a late decline — a marker, a member's CRC-32 — stores text first: it gets the room too)
            const Answer got = run(exact, data.size(), (uint64_t)chunk, q.first, q.second, T);
            n_runs++;
            if (!same(got, want)) {
                printf("DIFF %s ranges %u: rc %d / %d, text %llu / %llu, reason %d / %d, member %llu / %llu\n", argv[a], q.first, got.rc, want.rc,
                       (unsigned long long)got.n_text, (unsigned long long)want.n_text, got.v.reason, want.v.reason, (unsigned long long)got.v.member,
                       (unsigned long long)want.v.member);
                diffs++;
            }
        }
        if (T > 1 && run(exact, data.size(), (uint64_t)chunk, 3, {}, T - 1).rc != (size.rc == CRASS_ERR_OVERFLOW ? CRASS_ERR_OVERFLOW : want.rc)) {
            printf("DIFF %s: the overflow protocol\n", argv[a]);
            diffs++;
        }
        if (want_r >= 0 && want.v.reason != want_r) { printf("DIFF %s: reason %d, the name says %ld\n", argv[a], want.v.reason, want_r); diffs++; }
        if (!diffs) printf("ok   %s: rc %d, %llu bytes of text in %zu members\n", argv[a], want.rc, (unsigned long long)T, want.in_off.size() ? want.in_off.size() - 1 : 0);
        bad += diffs;
        free(exact);
    }
    printf("%d files, %d runs by ranges, %d files declined, %d differ\n", argc - 1, n_runs, n_declined, bad);
    return bad ? 1 : 0;
}

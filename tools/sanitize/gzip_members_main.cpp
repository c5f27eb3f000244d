// AddressSanitizer / UBSan harness for the plain-gzip host code in members mode (csrc/gunzip.cpp + csrc/gunzip_core.h +
// csrc/inflate_core.h), next to gzip_main.cpp: every file given — the sets of tests/gzip_member_sets.py, dumped by
// tools/sanitize/gzip_members_dump.py — goes through crass_gzip_inflate_members_host at the chunk size its name carries, from an
// exact-size heap copy into an exact-size heap buffer, so that a read or a store one byte outside either is the sanitizer's to
// report.  A name of the form X.c<chunk>.r<reason>.gz says what must come back (r-1: whatever comes, the seeded bit flips); an
// accepted file also goes through the overflow protocol, and its member table must end at the file's and the text's sizes.  CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/gunzip.cpp \
//       tools/sanitize/gzip_members_main.cpp -o gzip_members_asan && python3 tools/sanitize/gzip_members_dump.py DIR && ./gzip_members_asan DIR/*
#include "../../include/crass_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char **argv)
{
    int bad = 0, n_ok = 0, n_declined = 0;
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
        crass_bgzf_verdict v;
        crass_gzip_plan plan;
        crass_gzip_members mem;
        uint64_t n_text = 0;
        int rc = crass_gzip_inflate_members_host(exact, data.size(), (uint64_t)chunk, nullptr, 0, &n_text, &plan, &mem, &v);      // the size alone
        bool ok = mem.n_members == 0;
        if (rc == CRASS_ERR_OVERFLOW || (rc == CRASS_OK && n_text == 0)) {
            uint8_t *out = n_text ? (uint8_t *)malloc(n_text) : nullptr;
            uint64_t n2 = 0;
            if (n_text > 1 && crass_gzip_inflate_members_host(exact, data.size(), (uint64_t)chunk, out, n_text - 1, &n2, nullptr, nullptr, &v) != CRASS_ERR_OVERFLOW) ok = false;
            crass_gzip_members_free(&mem);
            rc = crass_gzip_inflate_members_host(exact, data.size(), (uint64_t)chunk, out, n_text, &n2, nullptr, &mem, &v);
            if (rc == CRASS_OK && (n2 != n_text || mem.n_members == 0 || mem.in_off[mem.n_members] != data.size() || mem.text_off[mem.n_members] != n_text)) ok = false;
            free(out);
        }
        ok = ok && (rc == CRASS_OK ? v.reason == 0 : (rc == CRASS_ERR_UNSUPPORTED && v.reason != 0));
        if (want_r >= 0) ok = ok && v.reason == want_r;
        printf("%s %s: rc %d, %llu bytes of text in %llu members, %llu of %llu chunks on the chain, reason %d, member %llu at %llu\n", ok ? "ok  " : "DIFF",
               argv[a], rc, (unsigned long long)n_text, (unsigned long long)mem.n_members, (unsigned long long)plan.n_chain,
               (unsigned long long)plan.n_chunks, v.reason, (unsigned long long)v.member, (unsigned long long)v.in_pos);
        bad += ok ? 0 : 1; n_ok += rc == CRASS_OK; n_declined += rc == CRASS_ERR_UNSUPPORTED;
        crass_gzip_plan_free(&plan);
        crass_gzip_members_free(&mem);
        free(exact);
    }
    printf("%d files: %d inflated, %d declined, %d DIFF\n", argc - 1, n_ok, n_declined, bad);
    return bad ? 1 : 0;
}

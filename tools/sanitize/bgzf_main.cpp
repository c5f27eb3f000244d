// AddressSanitizer / UBSan harness for the BGZF host code (csrc/bgzf.cpp + csrc/inflate_core.h), next to fastx_scan_main.cpp: every
// file given — the sets of tests/bgzf_sets.py, dumped by tools/sanitize/bgzf_dump.py — goes through crass_bgzf_index_host and
// crass_bgzf_inflate_host, from an exact-size heap copy into an exact-size heap buffer, so that a read or a store one byte outside
// either is the sanitizer's to report.  A name of the form X.m<member>.r<reason>.bgzf says what must come back.  CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -fno-omit-frame-pointer -Iinclude crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/bgzf_main.cpp -o bgzf_asan && python3 tools/sanitize/bgzf_dump.py DIR && ./bgzf_asan DIR/*
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
        long want_m = -1, want_r = -1;
        if (const char *p = strstr(argv[a], ".m")) if (sscanf(p, ".m%ld.r%ld.", &want_m, &want_r) != 2) want_m = want_r = -1;
        crass_bgzf_index ix;
        crass_bgzf_verdict v;
        memset(&v, 0, sizeof(v));
        int rc = crass_bgzf_index_host(exact, data.size(), &ix);
        uint64_t n_text = 0;
        if (rc == CRASS_OK) {
            n_text = ix.out_off[ix.n_members];
            uint8_t *out = n_text ? (uint8_t *)malloc(n_text) : nullptr;
            rc = crass_bgzf_inflate_host(exact, data.size(), &ix, out, n_text, &v);
            if (rc == CRASS_OK && n_text && crass_bgzf_inflate_host(exact, data.size(), &ix, out, n_text - 1, &v) != CRASS_ERR_INVALID_ARG) rc = -1;
            free(out);
        } else v = ix.decline;
        bool ok = rc == CRASS_OK ? v.reason == 0 : (rc == CRASS_ERR_UNSUPPORTED && v.reason != 0);
        if (want_r >= 0) ok = ok && v.reason == want_r && (want_r == 0 || (long)v.member == want_m);
        printf("%s %s: rc %d, %llu bytes of text, reason %d, member %llu at %llu\n", ok ? "ok  " : "DIFF", argv[a], rc, (unsigned long long)n_text,
               v.reason, (unsigned long long)v.member, (unsigned long long)v.in_pos);
        bad += ok ? 0 : 1; n_ok += rc == CRASS_OK; n_declined += rc == CRASS_ERR_UNSUPPORTED;
        crass_bgzf_index_free(&ix);
        free(exact);
    }
    printf("%d files: %d inflated, %d declined, %d DIFF\n", argc - 1, n_ok, n_declined, bad);
    return bad ? 1 : 0;
}

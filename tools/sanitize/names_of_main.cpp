// AddressSanitizer / UBSan harness for crass_fastx_names_of (csrc/fastx_scan.cpp), next to find_names_main.cpp: every file given —
// the sets of tests/fastx_sets.py, dumped by tools/sanitize/fastx_scan_dump.py — is scanned; where it is accepted, its records in
// reverse order with every third one twice go through crass_fastx_names_of with both index bases, from exact-size heap copies of
// the bytes, the indices, the offsets and an output of exactly the capacity: the capacity one byte short (CRASS_ERR_OVERFLOW,
// offsets complete), exact and one byte long; each name must be the bytes up to the first isspace() byte.  Then designed inputs
// of its own: a last header without a line end, an empty name at the input's end, n == 0, an index out of range on either side,
// NULL arrays.  CPU only.  Prints one line per file; any sanitizer report fails the run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/names_of_main.cpp -o names_of_asan -lz && python3 tools/sanitize/fastx_scan_dump.py DIR && ./names_of_asan DIR/*
#include "../../include/crass_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
static bool is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// one call on exact-size heap copies; true: the status, the offsets and the bytes in front of the capacity are as they must be
static bool one(const uint8_t *bytes, uint64_t nb, const uint64_t *rec_pos, uint64_t n_reads, const std::vector<uint64_t> &idx, uint64_t base, int64_t slack)
{
    std::string want;
    std::vector<uint64_t> woff(1, 0);
    for (uint64_t r : idx) {
        uint64_t s = rec_pos[r] + 1, e = s;
        while (e < nb && !is_space(bytes[e])) e++;
        want.append((const char *)bytes + s, e - s);
        woff.push_back(want.size());
    }
    if (slack < 0 && want.size() < (uint64_t)-slack) return true;
    const uint64_t cap = want.size() + slack, n = idx.size();
    uint64_t *ix = n ? (uint64_t *)malloc(n * 8) : nullptr;
    for (uint64_t k = 0; k < n; k++) ix[k] = idx[k] + base;
    uint64_t *off = (uint64_t *)malloc((n + 1) * 8);
    uint8_t *out = cap ? (uint8_t *)malloc(cap) : nullptr;
    const int st = crass_fastx_names_of(bytes, nb, rec_pos, n_reads, ix, n, base, out, cap, off);
    bool ok = st == (cap < want.size() ? CRASS_ERR_OVERFLOW : CRASS_OK);
    ok = ok && memcmp(off, woff.data(), (n + 1) * 8) == 0;
    const uint64_t m = cap < want.size() ? cap : want.size();
    ok = ok && (m == 0 || memcmp(out, want.data(), m) == 0);
    free(ix); free(off); free(out);
    return ok;
}

static bool designed()
{
    bool ok = true;
    const char *texts[] = {">a\nAC\n>tail", ">q\nA\n>", ">only", ">x y\nAC\n>\tz\nA\n", ">crlf c\r\nAC\r\n>n\r\nA\r\n"};
    for (const char *t : texts) {
        const uint64_t nb = strlen(t);
        uint8_t *exact = (uint8_t *)malloc(nb);
        memcpy(exact, t, nb);
        std::vector<uint64_t> rp;
        for (uint64_t p = 0; p < nb; p++) if (exact[p] == '>' && (p == 0 || exact[p - 1] == '\n')) rp.push_back(p);
        const uint64_t n = rp.size();
        rp.push_back(nb);
        uint64_t *rpx = (uint64_t *)malloc(rp.size() * 8);
        memcpy(rpx, rp.data(), rp.size() * 8);
        std::vector<uint64_t> all;
        for (uint64_t r = n; r-- > 0;) { all.push_back(r); all.push_back(r); }
        for (uint64_t base : {0ull, 7ull}) {
            for (int64_t slack : {-1, 0, 1}) ok = ok && one(exact, nb, rpx, n, all, base, slack);
            ok = ok && one(exact, nb, rpx, n, {}, base, 0);
            for (uint64_t r = 0; r < n; r++) ok = ok && one(exact, nb, rpx, n, {r}, base, 0);
            // an index out of range, below and above: nothing is written
            uint64_t off[3] = {5, 5, 5}, bad[2] = {base, base + n};
            uint8_t out[8] = {0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5};
            ok = ok && crass_fastx_names_of(exact, nb, rpx, n, bad, 2, base, out, 8, off) == CRASS_ERR_INVALID_ARG;
            if (base) { bad[1] = base - 1; ok = ok && crass_fastx_names_of(exact, nb, rpx, n, bad, 2, base, out, 8, off) == CRASS_ERR_INVALID_ARG; }
            for (uint8_t b : out) ok = ok && b == 0xA5;
        }
        uint64_t off[2], ix[1] = {0};
        ok = ok && crass_fastx_names_of(exact, nb, rpx, n, nullptr, 1, 0, nullptr, 0, off) == CRASS_ERR_INVALID_ARG;
        ok = ok && crass_fastx_names_of(exact, nb, rpx, n, ix, 1, 0, nullptr, 0, nullptr) == CRASS_ERR_INVALID_ARG;
        ok = ok && crass_fastx_names_of(nullptr, nb, rpx, n, ix, 1, 0, nullptr, 0, off) == CRASS_ERR_INVALID_ARG;
        ok = ok && crass_fastx_names_of(exact, nb, rpx, n, ix, 1, 0, nullptr, 3, off) == CRASS_ERR_INVALID_ARG;
        ok = ok && crass_fastx_names_of(nullptr, 0, nullptr, 0, ix, 1, 0, nullptr, 0, off) == CRASS_ERR_INVALID_ARG;      // (no records: every index is out of range)
        ok = ok && crass_fastx_names_of(nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, 0, off) == CRASS_OK && off[0] == 0;
        free(rpx); free(exact);
    }
    return ok;
}

int main(int argc, char **argv)
{
    int bad = 0;
    const bool d = designed();
    printf("%s designed inputs\n", d ? "ok  " : "DIFF");
    bad += d ? 0 : 1;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { printf("DIFF %s: cannot open\n", argv[a]); bad++; continue; }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + k);
        fclose(f);
        uint8_t *exact = data.empty() ? nullptr : (uint8_t *)malloc(data.size());
        if (exact) memcpy(exact, data.data(), data.size());
        crass_fastx_layout lay;
        if (crass_fastx_scan_host(exact, data.size(), &lay) != CRASS_OK) { printf("ok   %s: declined, no names\n", argv[a]); crass_fastx_layout_free(&lay); free(exact); continue; }
        const uint64_t n = lay.n_reads;
        std::vector<uint64_t> idx;
        for (uint64_t r = n; r-- > 0;) { idx.push_back(r); if (r % 3 == 0) idx.push_back(r); }
        bool ok = true;
        for (uint64_t base : {0ull, 7ull}) for (int64_t slack : {-1, 0, 1}) ok = ok && one(exact, data.size(), lay.rec_pos, n, idx, base, slack);
        printf("%s %s: %llu records, %zu names\n", ok ? "ok  " : "DIFF", argv[a], (unsigned long long)n, idx.size());
        bad += ok ? 0 : 1;
        free(exact);
        crass_fastx_layout_free(&lay);
    }
    return bad ? 1 : 0;
}

// AddressSanitizer / UBSan harness for the plain-gzip host code by ranges (crass_gzip_inflate_ranges_host: csrc/gunzip.cpp +
// csrc/gunzip_core.h + csrc/inflate_core.h), next to gzip_main.cpp: a few built-in streams (made here with zlib: FASTQ-like text
// in short blocks, text copied from 20 .. 32 KB back, a text shorter than a window, no text at all, and copies with one bit
// flipped) go through the function for 1 .. 7 ranges with even cuts and with cuts on, beside and between element boundaries,
// from an exact-size heap copy into an exact-size heap buffer, so that a read or a store one byte outside either is the
// sanitizer's to report.  Text and verdict must be crass_gzip_inflate_host's.  CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/gunzip.cpp \
//       tools/sanitize/gzip_ranges_main.cpp -o gzip_ranges_asan -lz && ./gzip_ranges_asan
#include "../../include/crass_hip.h"
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// text as one gzip member, a Z_BLOCK flush every `flush` bytes (0: none)
static std::vector<uint8_t> gz(const std::vector<uint8_t> &text, int level, size_t flush)
{
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, level, Z_DEFLATED, 31, 9, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    std::vector<uint8_t> out(deflateBound(&z, text.size()) + text.size() / 64 + 4096);
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    size_t at = 0;
    while (flush && at + flush < text.size()) {
        z.next_in = const_cast<uint8_t *>(text.data()) + at; z.avail_in = (uInt)flush;
        if (deflate(&z, Z_BLOCK) != Z_OK) abort();
        at += flush;
    }
    z.next_in = const_cast<uint8_t *>(text.data()) + at; z.avail_in = (uInt)(text.size() - at);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(out.size() - z.avail_out);
    deflateEnd(&z);
    return out;
}

static std::vector<uint8_t> fastq_like(size_t n)
{
    std::string t;
    for (int i = 0; t.size() < n; i++) {
        const int L = 100 + (int)(rnd() % 51);
        t += "@run." + std::to_string(i) + " lane=" + std::to_string(i % 4) + "\n";
        for (int k = 0; k < L; k++) t += "ACGT"[rnd() & 3];
        t += "\n+\n";
        for (int k = 0; k < L; k++) t += "FFFFFFFF:,#F"[rnd() % 12];
        t += "\n";
    }
    return std::vector<uint8_t>(t.begin(), t.end());
}

static std::vector<uint8_t> far_matches(size_t n)
{
    std::vector<uint8_t> t;
    for (int i = 0; i < 33000; i++) t.push_back("ACGTNacgtnRYKMSW"[rnd() & 15]);
    while (t.size() < n) {
        for (int i = 0; i < 2200; i++) t.push_back("ACGTNacgtnRYKMSW"[rnd() & 15]);
        for (int r = 0; r < 2; r++) {
            const size_t back = 20000 + rnd() % 12600, len = 100 + rnd() % 300, from = t.size() - back;
            for (size_t k = 0; k < len; k++) t.push_back(t[from + k]);
        }
    }
    return t;
}

struct Answer { int rc; uint64_t n_text; crass_bgzf_verdict v; std::vector<uint8_t> text; };

static uint8_t *exact_copy(const std::vector<uint8_t> &d)
{
    uint8_t *p = d.empty() ? nullptr : (uint8_t *)malloc(d.size());
    if (p) memcpy(p, d.data(), d.size());
    return p;
}

// n_ranges 0: crass_gzip_inflate_host
static Answer run(const std::vector<uint8_t> &file, uint64_t chunk, uint32_t n_ranges, const std::vector<uint64_t> &nominal, uint64_t cap)
{
    Answer A;
    memset(&A.v, 0, sizeof(A.v));
    A.n_text = 0;
    uint8_t *in = exact_copy(file);
    uint64_t *nom = nominal.empty() ? nullptr : (uint64_t *)malloc(nominal.size() * 8);
    if (nom) memcpy(nom, nominal.data(), nominal.size() * 8);
    uint8_t *out = cap ? (uint8_t *)malloc(cap) : nullptr;
    crass_gzip_plan plan;
    A.rc = n_ranges ? crass_gzip_inflate_ranges_host(in, file.size(), chunk, n_ranges, nom, out, cap, &A.n_text, &plan, &A.v)
                    : crass_gzip_inflate_host(in, file.size(), chunk, out, cap, &A.n_text, &plan, &A.v);
    if (A.rc == CRASS_OK) A.text.assign(out, out + A.n_text);
    crass_gzip_plan_free(&plan);
    free(out); free(nom); free(in);
    return A;
}

static bool same(const Answer &a, const Answer &b)
{
    return a.rc == b.rc && a.n_text == b.n_text && a.v.reason == b.v.reason && a.v.member == b.v.member && a.v.in_pos == b.v.in_pos && a.text == b.text;
}

int main()
{
    std::vector<std::pair<std::string, std::vector<uint8_t>>> files;
    const std::vector<uint8_t> fq = fastq_like(260000), far = far_matches(300000);
    files.push_back({"fastq_short_blocks", gz(fq, 6, 9000)});
    files.push_back({"far_matches_short_blocks", gz(far, 9, 3000)});
    files.push_back({"fastq_one_flush", gz(fq, 1, 0)});
    files.push_back({"shorter_than_a_window", gz(std::vector<uint8_t>(fq.begin(), fq.begin() + 20000), 6, 0)});
    files.push_back({"no_text", gz(std::vector<uint8_t>(), 6, 0)});
    const std::vector<uint8_t> good = files[1].second;
    for (int i = 0; i < 12; i++) {
        std::vector<uint8_t> bad = good;
        bad[(size_t)i * bad.size() / 12 + rnd() % (bad.size() / 12)] ^= (uint8_t)(1u << (rnd() & 7));
        files.push_back({"flip_" + std::to_string(i), bad});
    }
    int n_bad = 0, n_runs = 0, n_declined = 0;
    for (const auto &f : files) {
        const uint64_t chunk = 4096;
        const Answer size = run(f.second, chunk, 0, {}, 0);          // the size alone (or the decline)
        const uint64_t T = size.n_text;
        const Answer want = size.rc == CRASS_ERR_OVERFLOW ? run(f.second, chunk, 0, {}, T) : size;
        n_declined += want.rc == CRASS_ERR_UNSUPPORTED;
        const uint64_t room = T;                          // (a late decline — CRC, marker — stores text first: it gets the room too)
        std::vector<std::vector<uint64_t>> cuts;
        for (uint32_t n = 1; n <= 7; n++) cuts.push_back({});             // even cuts: the sizes follow below
        if (T > 70000) {
            cuts.push_back({T / 2}); cuts.push_back({T / 2 - 1, T / 2 + 1}); cuts.push_back({0, 0, T}); cuts.push_back({T, T});
            cuts.push_back({T / 3, T / 3, T / 3 + 1}); cuts.push_back({1, T - 1}); cuts.push_back({33000, 33001, 33002, 65536, 65537, 65538});
        }
        for (size_t q = 0; q < cuts.size(); q++) {
            const uint32_t n = q < 7 ? (uint32_t)q + 1 : (uint32_t)cuts[q].size() + 1;
            const Answer got = run(f.second, chunk, n, cuts[q], room);
            n_runs++;
            if (!same(got, want)) {
                printf("DIFF %s ranges %u cuts #%zu: rc %d / %d, text %llu / %llu, reason %d / %d\n", f.first.c_str(), n, q, got.rc, want.rc,
                       (unsigned long long)got.n_text, (unsigned long long)want.n_text, got.v.reason, want.v.reason);
                n_bad++;
            }
            if (T > 1 && run(f.second, chunk, n, cuts[q], T - 1).rc != (size.rc == CRASS_ERR_OVERFLOW ? CRASS_ERR_OVERFLOW : want.rc)) {
                printf("DIFF %s ranges %u cuts #%zu: one byte short\n", f.first.c_str(), n, q);
                n_bad++;
            }
        }
    }
    printf("%zu streams, %d runs, %d streams declined, %d DIFF\n", files.size(), n_runs, n_declined, n_bad);
    return n_bad ? 1 : 0;
}

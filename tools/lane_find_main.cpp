// lane_find_main.cpp — the packed seed find of the lane kernel (crass_amd/csrc/lane_find.h: find_packed) against the serial
// rule it replaces (bmpSearch's, one candidate at a time: a copy of ln_find_serial of survivor_lanes.hip on host words), on designed
// cases and on random draws.  Host only:  c++ -O2 -std=c++17 -I crass_amd/csrc tools/lane_find_main.cpp -o lane_find_main
// (tests/test_lane_find_host.py does that; with -fsanitize=address,undefined it is the sanitizer run of the header).
// Exit status 0: no difference; 1: the first difference is printed.     usage: lane_find_main [random draws, default 1000000]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lane_find.h"

using crass::find_packed;
using crass::find_packed_steps;

// a read as the lane kernel holds it: 16 bases per word, base p in bits 2 (p & 15) of word p >> 4, zero words behind
struct Text {
    std::vector<uint32_t> w;
    int L = 0;
    explicit Text(int len) : w((size_t)(len + 15) / 16 + 8, 0u), L(len) {}
    void set(int p, uint32_t b) { w[(size_t)p >> 4] = (w[(size_t)p >> 4] & ~(3u << ((p & 15) * 2))) | ((b & 3u) << ((p & 15) * 2)); }
    uint32_t word(int i) const { return (i >= 0 && (size_t)i < w.size()) ? w[(size_t)i] : 0u; }
    uint32_t code(int p, int plen) const
    {
        const int wi = p >> 4, sh = (p & 15) * 2;
        const uint64_t v = ((uint64_t)word(wi + 1) << 32) | word(wi);
        return (uint32_t)(v >> sh) & ((1u << (2 * plen)) - 1u);
    }
    void plant(int p, uint32_t c, int plen) { for (int i = 0; i < plen; i++) set(p + i, (c >> (2 * i)) & 3u); }
    // bases [start, start + 64) as two 64-bit words, base `start` in bits 0-1 (ln_load128)
    void load128(int start, uint64_t &lo, uint64_t &hi) const
    {
        const int wi = start >> 4;
        const uint32_t sh = (uint32_t)(start & 15) * 2u;
        uint32_t y[4];
        for (int k = 0; k < 4; k++) y[k] = crass::lf_alignbit(word(wi + k + 1), word(wi + k), sh);
        lo = (uint64_t)y[0] | ((uint64_t)y[1] << 32); hi = (uint64_t)y[2] | ((uint64_t)y[3] << 32);
    }
};

// the serial rule: bmpSearch's conditions (end - begin <= 0, plen > end - begin, last candidate at p + plen <= end)
static int find_serial(const Text &x, int begin, int end, uint32_t sj, int plen)
{
    if (end - begin <= 0 || plen <= 0 || plen > end - begin) return -1;
    uint32_t code = x.code(begin, plen);
    const int top = 2 * (plen - 1);
    int nb = begin + plen;
    uint64_t buf = 0; int left = 0;
    for (int p = begin;; p++) {
        if (code == sj) return p;
        if (p + 1 + plen > end) return -1;
        if (left == 0) {
            const int wi = nb >> 4;
            const uint32_t sh = (uint32_t)(nb & 15) * 2u;
            buf = (uint64_t)crass::lf_alignbit(x.word(wi + 1), x.word(wi), sh) | ((uint64_t)crass::lf_alignbit(x.word(wi + 2), x.word(wi + 1), sh) << 32);
            left = 32;
        }
        code = (code >> 2) | ((uint32_t)(buf & 3ull) << top);
        buf >>= 2; left--; nb++;
    }
}

// the packed route as ln_find takes it: chunks of 64 - plen + 1 candidates; short: the steps of a default window only, where
// the chunk allows it (on the device: where it does in every lane of the wave)
static int find_chunked(const Text &x, int begin, int end, uint32_t sj, int plen, bool short_steps)
{
    int left = (end - begin <= 0 || plen <= 0 || plen > end - begin) ? 0 : end - plen - begin + 1;
    const int chunk = 64 - plen + 1;
    while (left > 0) {
        uint64_t lo, hi;
        x.load128(begin, lo, hi);
        const int n = left < chunk ? left : chunk;
        const int t = find_packed_steps(lo, hi, sj, plen, n, !(short_steps && n <= crass::kLaneFindShortNpos));
        if (t >= 0) return begin + t;
        left -= chunk; begin += chunk;
    }
    return -1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

static long n_checked = 0, n_matched = 0;

static bool check(const char *what, const Text &x, int begin, int end, uint32_t sj, int plen)
{
    const int want = find_serial(x, begin, end, sj, plen);
    n_checked++; n_matched += want >= 0;
    for (int s = 0; s < 2; s++) {
        const int got = find_chunked(x, begin, end, sj, plen, s != 0);
        if (got != want) {
            fprintf(stderr, "%s: L %d begin %d end %d plen %d code %#x %s: packed %d, serial %d\n", what, x.L, begin, end, plen, sj, s ? "short steps" : "all steps", got, want);
            return false;
        }
    }
    const int npos = end - plen - begin + 1;
    if (npos >= 1 && npos <= 64 - plen + 1) {             // the header's own entry point, one chunk
        uint64_t lo, hi;
        x.load128(begin, lo, hi);
        const int t = find_packed(lo, hi, sj, plen, npos);
        if ((t < 0 ? -1 : begin + t) != want) { fprintf(stderr, "%s: find_packed %d, serial %d (begin %d npos %d plen %d)\n", what, t, want, begin, npos, plen); return false; }
    }
    return true;
}

static Text random_text(int L)
{
    Text x(L);
    for (int p = 0; p < L; p++) x.set(p, (uint32_t)(rnd() & 3u));
    return x;
}
// a code that occurs nowhere in x from `from` on
static uint32_t absent_code(const Text &x, int from, int plen)
{
    for (;;) {
        const uint32_t c = (uint32_t)rnd() & ((1u << (2 * plen)) - 1u);
        bool hit = false;
        for (int p = from; p + plen <= x.L + 32 && !hit; p++) hit = x.code(p, plen) == c;
        if (!hit) return c;
    }
}

static bool designed()
{
    for (int plen = 6; plen <= 8; plen++) {
        const int chunk = 64 - plen + 1;
        for (int npos : {1, 2, 8, 9, 16, 17, 25, 48, 49, 50, 56, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 3}) {
            for (int begin : {0, 5, 16, 31, 77}) {
                const int end = begin + npos + plen - 1, L = end + 40;
                Text base = random_text(L);
                const uint32_t c = absent_code(base, 0, plen);
                if (c == 0) continue;                      // (zero words behind the text: poly-A has its own cases)
                if (!check("no match", base, begin, end, c, plen)) return false;
                { Text x = base; x.plant(begin, c, plen); if (!check("match at offset 0", x, begin, end, c, plen)) return false; }
                { Text x = base; x.plant(begin + npos - 1, c, plen); if (!check("match at npos - 1", x, begin, end, c, plen)) return false; }
                { Text x = base; x.plant(begin + npos, c, plen); if (find_serial(x, begin, end, c, plen) != -1) { fprintf(stderr, "designed case broken\n"); return false; }
                  if (!check("match at npos only", x, begin, end, c, plen)) return false; }
                for (int t = 0; t + 8 < npos; t += 7) {
                    Text x = base;
                    x.plant(begin + t + 8, c, plen); x.plant(begin + t, c, plen);       // (the lower copy last: it may overlap the upper one)
                    if (find_serial(x, begin, end, c, plen) > begin + t) continue;      // (an overlap made an earlier one: still checked)
                    if (!check("matches at t and t + 8", x, begin, end, c, plen)) return false;
                }
                for (int t = 0; t < npos; t++) {            // a match at every single offset
                    Text x = base; x.plant(begin + t, c, plen);
                    if (!check("match at t", x, begin, end, c, plen)) return false;
                }
            }
        }
        // poly-A (code 0) against the zero bases past a read's end: a window clipped at L (end = L, and the reference's
        // end = L - 1), the read's last bases C so that the only A's in reach are the padding's
        for (int L : {60, 64, 100, 150}) {
            for (int back = plen; back <= 40; back += 3) {
                Text x = random_text(L);
                for (int p = L - back; p < L; p++) x.set(p, 1u);
                for (int end : {L, L - 1}) if (!check("poly-A at the read's end", x, L - back, end, 0u, plen)) return false;
                Text y = x;
                y.plant(L - plen, 0u, plen);               // ... and a real poly-A as the read's last bases
                for (int end : {L, L - 1}) if (!check("poly-A ends the read", y, L - back, end, 0u, plen)) return false;
            }
        }
        // bmpSearch's refusals
        { Text x = random_text(80); const uint32_t c = x.code(10, plen);
          if (!check("end == begin", x, 10, 10, c, plen) || !check("end < begin", x, 10, 4, c, plen) || !check("plen > end - begin", x, 10, 10 + plen - 1, c, plen)
              || !check("npos == 1, match", x, 10, 10 + plen, c, plen)) return false; }
    }
    return true;
}

int main(int argc, char **argv)
{
    const long draws = argc > 1 ? atol(argv[1]) : 1000000;
    if (!designed()) return 1;
    const long n_designed = n_checked;
    n_checked = 0; n_matched = 0;
    for (long i = 0; i < draws; i++) {
        const int plen = rnd_in(6, 8), chunk = 64 - plen + 1;
        // nine draws in ten are one chunk (find_packed's own domain), the others up to three
        const int npos = (i % 10) ? rnd_in(1, chunk) : rnd_in(1, 3 * chunk);
        const int begin = rnd_in(0, 40), end = begin + npos + plen - 1;
        const int L = (i % 7) ? end + rnd_in(0, 30) : end;                // (every seventh window ends with the text)
        Text x = random_text(L);
        uint32_t c = (uint32_t)rnd() & ((1u << (2 * plen)) - 1u);
        if (i % 13 == 0) c = 0;
        if (rnd() & 1u) {                                                  // planted: one to three copies, anywhere up to just past the window
            const int copies = rnd_in(1, 3);
            for (int k = 0; k < copies; k++) { const int at = begin + rnd_in(0, npos + 1); if (at + plen <= L) x.plant(at, c, plen); }
        }
        if (!check("random", x, begin, end, c, plen)) { fprintf(stderr, "draw %ld\n", i); return 1; }
    }
    printf("lane_find ok: %ld designed cases, %ld random draws (%ld with a match)\n", n_designed, n_checked, n_matched);
    return 0;
}

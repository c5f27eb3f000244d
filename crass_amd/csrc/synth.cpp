// synth.cpp — the deterministic synthetic metagenome generator used by bench.py and the parity tests, and packed words back
// to text.
#include "host_ingest_internal.h"

using namespace crass;

extern "C" {

// ---- synthetic metagenome, counter-based ----
static inline uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static inline uint64_t key3(uint64_t seed, uint64_t a, uint64_t b) { return mix64(seed ^ mix64(a * 0xD1342543DE82EF95ull + mix64(b))); }

void crass_synth_default(crass_synth_spec *s)
{
    s->seed = 42; s->read_len = 150; s->n_dr = 50; s->dr_len_min = 28; s->dr_len_max = 37;
    s->spacer_len_min = 30; s->spacer_len_max = 38; s->crispr_per_million = 10000; s->gc_classes = 0;
    s->array_min_repeats = 0; s->array_max_repeats = 0;
}

static inline uint32_t gc_word(uint64_t seed, uint64_t i, uint32_t w, uint32_t cls)
{
    // GC-content classes 30/45/55/70 %: 8-bit threshold draw + 1 bit to pick inside the pair
    static const uint32_t thr[4] = {77, 115, 141, 179};
    uint32_t out = 0;
    for (int q = 0; q < 2; q++) {
        uint64_t r0 = key3(seed ^ 0x6C62272E07BB0142ull, i, (uint64_t)w * 4 + q * 2);
        uint64_t r1 = key3(seed ^ 0x6C62272E07BB0142ull, i, (uint64_t)w * 4 + q * 2 + 1);
        for (int k = 0; k < 8; k++) {
            uint32_t u = (uint32_t)(r0 >> (8 * k)) & 0xFF;
            uint32_t pick = (uint32_t)(r1 >> k) & 1;
            uint32_t code = (u < thr[cls & 3]) ? (pick ? 1u : 2u) : (pick ? 0u : 3u);   // C/G vs A/T
            out |= code << (2 * (q * 8 + k));
        }
    }
    return out;
}

int crass_synth_packed(const crass_synth_spec *s, uint64_t first, uint64_t n, uint32_t *packed, int n_threads)
{
    if (!s || (n && !packed)) return CRASS_ERR_INVALID_ARG;
    if (s->read_len == 0 || s->read_len > CRASS_HIP_MAX_READ_LEN || s->n_dr == 0 || s->dr_len_max < s->dr_len_min ||
        s->spacer_len_max < s->spacer_len_min || s->dr_len_max > 200) return CRASS_ERR_INVALID_ARG;
    const bool arrays = s->array_max_repeats != 0;           // long-read mode: an array placed inside a random read
    if (arrays && (s->array_max_repeats < s->array_min_repeats || s->array_max_repeats > 1000 || s->spacer_len_max > 64)) return CRASS_ERR_INVALID_ARG;
    if (!arrays && s->read_len > 4096) return CRASS_ERR_INVALID_ARG;
    const uint32_t L = s->read_len, W = (L + 15) / 16;
    const uint64_t seed = s->seed;
    // DR table
    std::vector<std::vector<uint8_t>> drs(s->n_dr);
    for (uint32_t d = 0; d < s->n_dr; d++) {
        uint32_t len = s->dr_len_min + (uint32_t)(key3(seed, 1000, d) % (s->dr_len_max - s->dr_len_min + 1));
        drs[d].resize(len);
        for (uint32_t k = 0; k < len; k++) drs[d][k] = (uint8_t)((key3(seed, 2000 + d, k >> 5) >> (2 * (k & 31))) & 3);
    }
    unsigned nt = n_threads > 0 ? (unsigned)n_threads : hw_threads();
    nt = std::min<unsigned>(nt, 64);
    parallel_ranges(n, nt, [&](uint64_t a, uint64_t b, unsigned) {
        std::vector<uint8_t> sbuf;
        for (uint64_t k = a; k < b; k++) {
            const uint64_t i = first + k;
            uint32_t *w = packed + k * (uint64_t)W;
            const uint64_t h = key3(seed, 1, i);
            if (arrays) {
                // BASELINE configs[3] shape: random background, and in a CRISPR read an array of U[min,max] repeats
                // (DR + spacer units) written over it from a random offset (cut at the read end)
                const uint32_t cls = s->gc_classes > 1 ? (uint32_t)((h >> 40) % s->gc_classes) : 0;
                for (uint32_t q = 0; q < W; q++)
                    w[q] = s->gc_classes > 1 ? gc_word(seed, i, q, cls) : (uint32_t)key3(seed ^ 0xA24BAED4963EE407ull, i, q);
                if (L & 15) w[W - 1] &= (1u << ((L & 15) * 2)) - 1u;
                if ((h % 1000000ull) < s->crispr_per_million) {
                    const uint32_t d = (uint32_t)((h >> 24) % s->n_dr);
                    const uint32_t reps = s->array_min_repeats + (uint32_t)(key3(seed, 8, i) % (s->array_max_repeats - s->array_min_repeats + 1));
                    uint32_t pos = (uint32_t)(key3(seed, 3, i) % (L > 64 ? L * 2 / 5 : 1));
                    auto put = [&](uint32_t at, uint32_t code) { w[at >> 4] = (w[at >> 4] & ~(3u << ((at & 15) * 2))) | (code << ((at & 15) * 2)); };
                    for (uint32_t u = 0; u < reps; u++) {
                        const uint32_t sl = s->spacer_len_min + (uint32_t)(key3(seed, 6, i * 1024 + u) % (s->spacer_len_max - s->spacer_len_min + 1));
                        if (pos + drs[d].size() + sl > L) break;
                        for (size_t p = 0; p < drs[d].size(); p++) put(pos + (uint32_t)p, drs[d][p]);
                        pos += (uint32_t)drs[d].size();
                        for (uint32_t p = 0; p < sl; p++) put(pos + p, (uint32_t)((key3(seed, 7, i * 65536 + (uint64_t)u * 64 + p) >> 11) & 3));
                        pos += sl;
                    }
                }
            } else if ((h % 1000000ull) < s->crispr_per_million) {
                const uint32_t d = (uint32_t)((h >> 24) % s->n_dr);
                const uint32_t prefix = (uint32_t)(key3(seed, 3, i) % 41);
                const uint32_t cut = (uint32_t)(key3(seed, 4, i) % 41);
                sbuf.clear();
                for (uint32_t p = 0; p < prefix; p++) sbuf.push_back((uint8_t)((key3(seed, 5, i * 8192 + p) >> 7) & 3));
                uint32_t u = 0;
                while (sbuf.size() < (size_t)cut + L) {
                    sbuf.insert(sbuf.end(), drs[d].begin(), drs[d].end());
                    uint32_t sl = s->spacer_len_min + (uint32_t)(key3(seed, 6, i * 64 + u) % (s->spacer_len_max - s->spacer_len_min + 1));
                    for (uint32_t p = 0; p < sl; p++) sbuf.push_back((uint8_t)((key3(seed, 7, i * 8192 + (uint64_t)(u + 1) * 64 + p) >> 11) & 3));
                    u++;
                }
                for (uint32_t q = 0; q < W; q++) w[q] = 0;
                for (uint32_t q = 0; q < L; q++) w[q >> 4] |= (uint32_t)sbuf[cut + q] << ((q & 15) * 2);
            } else {
                const uint32_t cls = s->gc_classes > 1 ? (uint32_t)((h >> 40) % s->gc_classes) : 0;
                for (uint32_t q = 0; q < W; q++) {
                    uint32_t v = s->gc_classes > 1 ? gc_word(seed, i, q, cls) : (uint32_t)key3(seed ^ 0xA24BAED4963EE407ull, i, q);
                    w[q] = v;
                }
                if (L & 15) w[W - 1] &= (1u << ((L & 15) * 2)) - 1u;       // padding bases are zero
            }
        }
    });
    return CRASS_OK;
}

int crass_unpack_ascii(const uint32_t *packed, uint32_t stride_words, uint32_t read_len, uint64_t n, uint8_t *out)
{
    if (n && (!packed || !out || !stride_words)) return CRASS_ERR_INVALID_ARG;
    static const char acgt[4] = {'A', 'C', 'G', 'T'};
    parallel_ranges(n, std::min<unsigned>(hw_threads(), 32), [&](uint64_t a, uint64_t b, unsigned) {
        for (uint64_t i = a; i < b; i++) {
            const uint32_t *w = packed + i * (uint64_t)stride_words;
            uint8_t *o = out + i * (uint64_t)read_len;
            for (uint32_t q = 0; q < read_len; q++) o[q] = (uint8_t)acgt[(w[q >> 4] >> ((q & 15) * 2)) & 3];
        }
    });
    return CRASS_OK;
}

} // extern "C"

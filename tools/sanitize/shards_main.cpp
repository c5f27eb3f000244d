// AddressSanitizer / UBSan harness for the host side of the record-aligned shards (crass_fastx_files_shards_host and the serial
// probe, csrc/fastx_scan.cpp + csrc/fastx_scan.h), next to fastx_scan_main.cpp: every file given (the sets of
// tools/sanitize/fastx_scan_dump.py) alone and with its successor as a set of two, cut for 1 .. 7 ranks with even cuts and for two
// ranks at nominal cuts spread over the text; the cuts must be record positions of crass_fastx_files_scan_host, in order, and the
// verdict that scan's.  The probe of every tail of a small file is folded against the count of its line ends.  In front of the files,
// and with no file at all, a self-check of the host arithmetic of a rank's shard (csrc/fastx_shards.h): bgzf_members_for over the
// tilings of designed and drawn BGZF indices (fixed seed), shard_stage_place over designed pieces.  CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/shards_main.cpp -o shards_asan && python3 tools/sanitize/fastx_scan_dump.py DIR && ./shards_asan DIR/*
#include "../../include/crass_hip.h"
#include "../../crass_amd/csrc/fastx_scan.h"
#include "../../crass_amd/csrc/fastx_shards.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int check_set(const std::vector<uint8_t *> &ptr, const std::vector<uint64_t> &len, size_t a, size_t b)
{
    crass_fastx_files_layout lay;
    const int rc = crass_fastx_files_scan_host(ptr.data() + a, len.data() + a, (uint32_t)(b - a), &lay);
    const uint32_t nf = (uint32_t)(b - a);
    const uint64_t T = rc == CRASS_OK ? lay.file_byte_base[nf] - nf : 0;
    bool ok = true;
    unsigned tried = 0;
    for (uint32_t n = 1; n <= 7 && ok; n++) {
        for (uint64_t step = 0; step <= (n == 2 ? 40u : 0u) && ok; step++) {
            uint64_t nominal = T * step / 40;
            crass_fastx_shards sh;
            const int rs = crass_fastx_files_shards_host(ptr.data() + a, len.data() + a, nf, n, n == 2 && step ? &nominal : nullptr, &sh);
            tried++;
            ok = rs == rc && sh.decline_file == lay.decline_file && sh.decline_reason == lay.decline_reason && sh.decline_pos == lay.decline_pos &&
                 sh.bgzf.reason == lay.bgzf.reason && sh.bgzf.member == lay.bgzf.member;
            if (ok && rs == CRASS_OK) {
                ok = sh.n_reads == lay.n_reads && sh.rank_read_base[0] == 0 && sh.rank_read_base[n] == lay.n_reads && sh.cut_file[n] == nf && sh.cut_pos[n] == 0;
                for (uint32_t g = 0; ok && g < n; g++) {
                    const uint64_t r = sh.rank_read_base[g];
                    ok = r <= sh.rank_read_base[g + 1];
                    if (ok && r < lay.n_reads) ok = sh.cut_file[g] < nf && lay.rec_pos[r] == lay.file_byte_base[sh.cut_file[g]] + sh.cut_pos[g];
                }
            } else if (ok) ok = !sh.rank_read_base && !sh.cut_file && !sh.cut_pos && !sh.file_read_base && !sh.format;
            crass_fastx_shards_free(&sh);
        }
    }
    printf("%s shards of files %zu..%zu: rc %d, %u calls\n", ok ? "ok  " : "DIFF", a, b - 1, rc, tried);
    crass_fastx_files_layout_free(&lay);
    return ok ? 0 : 1;
}

static int check_probe(const uint8_t *p, uint64_t n)
{
    bool ok = true;
    for (uint64_t a = 0; a < n && ok; a++) {
        uint64_t out[7];
        const int left = a == 0 || p[a - 1] == 0x0A;
        ok = crass_fastx_cut_probe_host(p + a, n - a, left, out) == CRASS_OK;
        uint64_t nl = 0;
        for (uint64_t i = a; i < n; i++) nl += p[i] == 0x0A;
        ok = ok && out[0] == nl && out[1] <= 4 && (out[1] == 0 || out[2] == (left ? 0u : out[2])) && (out[6] == crass::kFxNone || p[a + out[6]] == 0x3E);
        for (uint64_t k = 0; ok && k < out[1]; k++) ok = out[2 + k] < n - a && (a + out[2 + k] == 0 || p[a + out[2 + k] - 1] == 0x0A);
    }
    return ok ? 0 : 1;
}

// ---- the member rule: which members of a BGZF index hold a text range, over ranges that tile the text ----
// one tiling {0 = cut[0] < ... < cut[k] = T} of the index out_off[n + 1]: every range's members enclose it, and together the
// ranges take EVERY member, those without text and the empty last one included
static bool check_tiling(const uint64_t *oo, uint64_t n, const uint64_t *cut, unsigned k, uint64_t *n_ranges)
{
    bool taken[8] = {false, false, false, false, false, false, false, false};
    for (unsigned g = 0; g < k; g++) {
        const uint64_t a = cut[g], b = cut[g + 1];
        uint64_t m0 = ~0ull, m1 = ~0ull;
        crass::bgzf_members_for(oo, n, a, b, &m0, &m1);
        ++*n_ranges;
        if (!(m0 <= m1 && m1 <= n && oo[m0] <= a && oo[m1] >= b)) return false;
        for (uint64_t m = m0; m < m1; m++) taken[m] = true;
    }
    for (uint64_t m = 0; m < n; m++) if (!taken[m]) return false;
    return true;
}

static int check_member_rule()
{
    static const uint64_t kSize[5] = {0, 1, 2, 5, 16};
    uint64_t rng = 0x9E3779B97F4A7C15ull;                 // a fixed seed: the same cases on every run
    auto draw = [&](uint64_t below) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (rng >> 33) % below; };
    uint64_t n_cases = 0, n_ranges = 0, n_bad = 0;
    auto tilings_of = [&](const uint64_t *oo, uint64_t n) {
        const uint64_t T = oo[n];
        if (T == 0) return;                               // (no text at all: nothing to cut)
        uint64_t cut[5];
        auto one = [&](unsigned inner) { cut[0] = 0; cut[inner + 1] = T; n_cases++; if (!check_tiling(oo, n, cut, inner + 1, &n_ranges)) n_bad++; };
        one(0);
        for (uint64_t x = 1; x < T; x++) { cut[1] = x; one(1); }      // every single inner cut
        if (T <= 10) {                                    // a small text: every pair and every triple of inner cuts
            for (uint64_t x = 1; x < T; x++) for (uint64_t y = x + 1; y < T; y++) {
                cut[1] = x; cut[2] = y; one(2);
                for (uint64_t z = y + 1; z < T; z++) { cut[1] = x; cut[2] = y; cut[3] = z; one(3); }
            }
        } else {                                          // else 12 drawn pairs and 12 drawn triples
            for (int rep = 0; rep < 24; rep++) {
                const unsigned inner = rep < 12 ? 2 : 3;
                if (T - 1 < inner) continue;
                uint64_t c[3];
                for (unsigned i = 0; i < inner;) {        // distinct positions in [1, T), then sorted
                    c[i] = 1 + draw(T - 1);
                    bool dup = false;
                    for (unsigned j = 0; j < i; j++) dup = dup || c[j] == c[i];
                    if (!dup) i++;
                }
                for (unsigned i = 0; i < inner; i++) for (unsigned j = i + 1; j < inner; j++) if (c[j] < c[i]) { const uint64_t t = c[i]; c[i] = c[j]; c[j] = t; }
                for (unsigned i = 0; i < inner; i++) cut[1 + i] = c[i];
                one(inner);
            }
        }
    };
    uint64_t oo[9];
    // every index of 1 .. 4 members ...
    for (uint64_t n = 1; n <= 4; n++) {
        uint64_t combos = 1;
        for (uint64_t m = 0; m < n; m++) combos *= 5;
        for (uint64_t code = 0; code < combos; code++) {
            oo[0] = 0;
            uint64_t q = code;
            for (uint64_t m = 0; m < n; m++) { oo[m + 1] = oo[m] + kSize[q % 5]; q /= 5; }
            tilings_of(oo, n);
        }
    }
    // ... and 3000 drawn ones of 5 .. 8, three in four with the empty last member a BGZF file ends with
    for (int k = 0; k < 3000; k++) {
        const uint64_t n = 5 + draw(4);
        const bool eof_member = draw(4) != 0;
        oo[0] = 0;
        for (uint64_t m = 0; m < n; m++) oo[m + 1] = oo[m] + (eof_member && m + 1 == n ? 0 : kSize[draw(5)]);
        tilings_of(oo, n);
    }
    printf("%s member rule: %llu tilings, %llu ranges, %llu fail\n", n_bad ? "DIFF" : "ok  ", (unsigned long long)n_cases, (unsigned long long)n_ranges,
           (unsigned long long)n_bad);
    return n_bad ? 1 : 0;
}

// ---- the staging placement: every piece at its text position modulo 16, none on another, the size the buffer is given ----
static int check_placement()
{
    struct List { std::vector<uint64_t> sa, sb; };
    std::vector<List> lists;
    lists.push_back(List{{}, {}});                                            // no piece
    lists.push_back(List{{0}, {1}});
    lists.push_back(List{{5}, {5}});                                          // an empty piece
    lists.push_back(List{{15, 0, 16, 17}, {16, 1, 32, 17}});                  // phases 15, 0, 0, 1; one byte, one byte, a full line, nothing
    lists.push_back(List{{3, 3, 3}, {4, 19, 35}});                            // the same phase thrice: 1, 16 and 32 bytes
    lists.push_back(List{{65535, 65536, 1ull << 32}, {131072, 65536 + 15, (1ull << 32) + 65280}});      // member-sized texts, a position beyond 2^32
    List every;                                                               // every phase against every phase of the cursor
    for (uint64_t p = 0; p < 16; p++) for (uint64_t l = 0; l < 18; l++) { every.sa.push_back(1000 * p + p); every.sb.push_back(1000 * p + p + l); }
    lists.push_back(every);
    int bad = 0;
    for (const List &L : lists) {
        const uint64_t n = L.sa.size();
        std::vector<uint64_t> off(n + 1, ~0ull);
        const uint64_t total = crass::shard_stage_place(L.sa.data(), L.sb.data(), n, off.data());
        bool ok = off[n] == ~0ull;                        // (nothing written behind the n places)
        uint64_t end = 0;
        for (uint64_t k = 0; ok && k < n; k++) {
            ok = off[k] % 16 == L.sa[k] % 16 && off[k] >= end && off[k] < end + 31;
            end = off[k] + (L.sb[k] - L.sa[k]);
        }
        ok = ok && total == end + 32;
        if (!ok) { printf("DIFF placement of %llu pieces\n", (unsigned long long)n); bad++; }
    }
    printf("%s placement: %zu lists, %d fail\n", bad ? "DIFF" : "ok  ", lists.size(), bad);
    return bad;
}

int main(int argc, char **argv)
{
    int bad = check_member_rule() + check_placement();
    std::vector<uint8_t *> ptr; std::vector<uint64_t> len;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { printf("DIFF %s: cannot open\n", argv[a]); bad++; continue; }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + k);
        fclose(f);
        // an exact-size heap copy: a read one byte past the input is the sanitizer's to report
        uint8_t *exact = data.empty() ? nullptr : (uint8_t *)malloc(data.size());
        if (exact) memcpy(exact, data.data(), data.size());
        ptr.push_back(exact); len.push_back(data.size());
        if (data.size() && data.size() < 3000) {
            const int pb = check_probe(exact, data.size());
            if (pb) printf("DIFF probe of %s\n", argv[a]);
            bad += pb;
        }
    }
    for (size_t f = 0; f < ptr.size(); f++) bad += check_set(ptr, len, f, f + 1);
    for (size_t f = 0; f + 1 < ptr.size(); f++) bad += check_set(ptr, len, f, f + 2);
    for (uint8_t *p : ptr) free(p);
    printf("%s: %d failures\n", bad ? "DIFF" : "ok  ", bad);
    return bad ? 1 : 0;
}

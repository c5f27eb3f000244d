// AddressSanitizer / UBSan harness for the host side of the record-aligned shards (crass_fastx_files_shards_host and the serial
// probe, csrc/fastx_scan.cpp + csrc/fastx_scan.h), next to fastx_scan_main.cpp: every file given (the sets of
// tools/sanitize/fastx_scan_dump.py) alone and with its successor as a set of two, cut for 1 .. 7 ranks with even cuts and for two
// ranks at nominal cuts spread over the text; the cuts must be record positions of crass_fastx_files_scan_host, in order, and the
// verdict that scan's.  The probe of every tail of a small file is folded against the count of its line ends.  CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/shards_main.cpp -o shards_asan && python3 tools/sanitize/fastx_scan_dump.py DIR && ./shards_asan DIR/*
#include "../../include/crass_hip.h"
#include "../../crass_amd/csrc/fastx_scan.h"
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

int main(int argc, char **argv)
{
    int bad = 0;
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

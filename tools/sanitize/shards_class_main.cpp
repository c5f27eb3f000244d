// AddressSanitizer / UBSan harness for the host cut rule of a FASTQ class (crass_fastx_files_shards_host_class, csrc/fastx_scan.cpp +
// csrc/fastx_scan.h), next to shards_main.cpp: the jobs of tools/sanitize/shards_class_dump.py (files jKKK_J.bin: job KKK's file
// J), each cut under class 1 for 1 .. 7 ranks with even cuts and for two ranks at nominal cuts spread over the text — every byte
// of a small job.  The cuts must be record positions of crass_fastx_files_scan_host_class(.., 1, ..), each the first at or after its
// nominal cut, and the verdict that scan's; class 0 must be crass_fastx_files_shards_host field for field.  CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/shards_class_main.cpp -o shards_class_asan && python3 tools/sanitize/shards_class_dump.py DIR && ./shards_class_asan DIR/*
#include "../../include/crass_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool same_verdict(const crass_fastx_shards &s, const crass_fastx_files_layout &l)
{
    return s.decline_file == l.decline_file && s.decline_reason == l.decline_reason && s.decline_pos == l.decline_pos && s.bgzf.reason == l.bgzf.reason &&
           s.bgzf.member == l.bgzf.member;
}

static int check_job(const uint8_t *const *ptr, const uint64_t *len, uint32_t nf, const char *name)
{
    bool ok = true;
    unsigned tried = 0;
    int rc1 = 0;
    for (int cls = 0; cls <= 1 && ok; cls++) {
        crass_fastx_files_layout lay;
        const int rc = crass_fastx_files_scan_host_class(ptr, len, nf, cls, &lay);
        if (cls) rc1 = rc;
        const uint64_t T = rc == CRASS_OK ? lay.file_byte_base[nf] - nf : 0;
        const uint64_t steps = T <= 400 ? T : 40;
        for (uint32_t n = 1; n <= 7 && ok; n++) {
            for (uint64_t step = 0; step <= (n == 2 ? steps : 0u) && ok; step++) {
                uint64_t nominal = steps ? T * step / steps : 0;
                const uint64_t *nom = n == 2 && step ? &nominal : nullptr;
                crass_fastx_shards sh;
                const int rs = crass_fastx_files_shards_host_class(ptr, len, nf, n, nom, cls, &sh);
                tried++;
                ok = rs == rc && same_verdict(sh, lay);
                if (ok && rs == CRASS_OK) {
                    ok = sh.n_reads == lay.n_reads && sh.rank_read_base[0] == 0 && sh.rank_read_base[n] == lay.n_reads && sh.cut_file[n] == nf && sh.cut_pos[n] == 0;
                    for (uint32_t g = 0; ok && g < n; g++) {
                        const uint64_t r = sh.rank_read_base[g];
                        ok = r <= sh.rank_read_base[g + 1];
                        if (ok && r < lay.n_reads) ok = sh.cut_file[g] < nf && lay.rec_pos[r] == lay.file_byte_base[sh.cut_file[g]] + sh.cut_pos[g];
                    }
                    if (ok && nom) {                      // the first record start at or after the nominal cut: the one before lies in front of it
                        const uint64_t r = sh.rank_read_base[1];
                        const uint32_t f = sh.cut_file[1];
                        const uint64_t at = f < nf ? lay.file_byte_base[f] - f + sh.cut_pos[1] : T;      // (text space: a byte less per file in front)
                        ok = at >= nominal;
                        if (ok && r > 0) {
                            uint32_t fb = 0;
                            while (fb + 1 < nf && lay.file_byte_base[fb + 1] <= lay.rec_pos[r - 1]) fb++;
                            ok = lay.rec_pos[r - 1] - fb < nominal;
                        }
                    }
                } else if (ok) ok = !sh.rank_read_base && !sh.cut_file && !sh.cut_pos && !sh.file_read_base && !sh.format;
                if (ok && cls == 0) {                     // class 0 is the four-line call
                    crass_fastx_shards s0;
                    const int r0 = crass_fastx_files_shards_host(ptr, len, nf, n, nom, &s0);
                    ok = r0 == rs && s0.decline_file == sh.decline_file && s0.decline_reason == sh.decline_reason && s0.decline_pos == sh.decline_pos && s0.n_reads == sh.n_reads;
                    for (uint32_t g = 0; ok && rs == CRASS_OK && g <= n; g++)
                        ok = s0.cut_file[g] == sh.cut_file[g] && s0.cut_pos[g] == sh.cut_pos[g] && s0.rank_read_base[g] == sh.rank_read_base[g];
                    crass_fastx_shards_free(&s0);
                }
                crass_fastx_shards_free(&sh);
            }
        }
        crass_fastx_files_layout_free(&lay);
    }
    crass_fastx_shards bad;
    ok = ok && crass_fastx_files_shards_host_class(ptr, len, nf, 2, nullptr, 2, &bad) == CRASS_ERR_INVALID_ARG && !bad.rank_read_base;
    printf("%s job %s, %u file(s): class 1 rc %d, %u calls\n", ok ? "ok  " : "DIFF", name, nf, rc1, tried);
    return ok ? 0 : 1;
}

int main(int argc, char **argv)
{
    int bad = 0;
    std::vector<uint8_t *> ptr; std::vector<uint64_t> len; std::vector<std::string> job;
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
        const char *base = strrchr(argv[a], '/');
        const std::string nm = base ? base + 1 : argv[a];
        job.push_back(nm.substr(0, nm.find('_')));
    }
    for (size_t a = 0; a < ptr.size();) {
        size_t b = a + 1;
        while (b < ptr.size() && job[b] == job[a]) b++;
        bad += check_job(ptr.data() + a, len.data() + a, (uint32_t)(b - a), job[a].c_str());
        a = b;
    }
    for (uint8_t *p : ptr) free(p);
    printf("%s: %d failures\n", bad ? "DIFF" : "ok  ", bad);
    return bad ? 1 : 0;
}

// AddressSanitizer / UBSan harness for the wrapped FASTQ rule on the host (csrc/fastx_scan.cpp: crass_fastx_scan_host_class,
// crass_fastx_files_scan_host_class), next to fastx_scan_main.cpp.  The inputs are built in: every one is copied to an exact-size
// heap block, so a read one byte past it is the sanitizer's to report; every PREFIX of every input goes through the rule as
// well (an input that ends anywhere).  Accepted inputs are checked for what the layout promises, declines for their stated
// (reason, position).  CPU only.  Prints one line per input; any DIFF or sanitizer report fails the run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/wrapped_scan_main.cpp -o wrapped_scan_asan -lz && ./wrapped_scan_asan
#include "../../include/crass_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct Case { const char *name; std::string data; int reason; uint64_t pos; uint64_t n_reads; uint64_t bases; };

static int scan(const std::string &d, int cls, crass_fastx_layout *lay)
{
    uint8_t *exact = d.empty() ? nullptr : (uint8_t *)malloc(d.size());
    if (exact) memcpy(exact, d.data(), d.size());
    const int rc = crass_fastx_scan_host_class(exact, d.size(), cls, lay);
    free(exact);
    return rc;
}

int main()
{
    std::string seq9000, q9000;
    for (int i = 0; i < 9000; i++) { seq9000 += "ACGT"[i & 3]; if (i % 60 == 59) seq9000 += '\n'; q9000 += (i % 60 == 0) ? '@' : 'I'; if (i % 60 == 59) q9000 += '\n'; }
    const std::vector<Case> cases = {
        {"four_line", "@a\nACGT\n+\nIIII\n@b\nAC\n+\nII\n", 0, 0, 2, 6},
        {"wrapped", "@a\nAC\nGT\n+a\nII\nII\n@b\nA\n+\nI\n", 0, 0, 2, 5},
        {"void_lines", "@a\nACGT\n+\nIIII\n\n\r\n  \n@b\nAC\n+\nII\n\n\n", 0, 0, 2, 6},
        {"quality_at_plus", "@a\nACGT\nACGT\n+\n@III\n+III\n@b\nA\n+\n@\n", 0, 0, 2, 9},
        {"crlf", "@a c\r\nAC\r\nGT\r\n+\r\nIIII\r\n", 0, 0, 1, 4},
        {"empty_then_void", "@e\n+\n\n@b\nA\n+\nI\n", 0, 0, 2, 1},
        {"empty_at_end", "@a\nA\n+\nI\n@e\n+\n", 0, 0, 2, 1},
        {"no_final_newline", "@a\nAC\nGT\n+\nII\nII", 0, 0, 1, 4},
        {"long_read", "@long\n" + seq9000 + "+\n" + q9000 + "@b\nA\n+\nI\n", 0, 0, 2, 9001},
        {"no_plus", "@a\nACGT\n@b\nAC\n", 3, 0, 0, 0},
        {"forbidden", "@a\nAC\nG>T\n+\nIIII\n", 5, 6, 0, 0},
        {"empty_then_at", "@a\nA\n+\nI\n@e\n+\n@b\nA\n+\nI\n", 12, 14, 0, 0},
        {"quality_del", "@a\nACGT\n+\nII\nI\x7fI\n", 7, 13, 0, 0},
        {"quality_passes", "@a\nACGT\n+\nII\nIII\n", 9, 13, 0, 0},
        {"quality_short", "@a\nA\n+\nI\n@b\nACGT\n+\nII\n", 8, 9, 0, 0},
        {"plus_ends_input", "@a\nA\n+\nI\n@e\n+", 8, 9, 0, 0},
        {"not_a_header", "@a\nACGT\n+\nIIII\n\nACGT\n", 4, 16, 0, 0},
        {"first_byte", "x@a\nA\n+\nI\n", 2, 0, 0, 0},
        {"empty", "", 1, 0, 0, 0},
    };
    int bad = 0;
    for (const Case &c : cases) {
        crass_fastx_layout lay;
        const int rc = scan(c.data, 1, &lay);
        bool ok;
        if (c.reason == 0) {
            ok = rc == CRASS_OK && lay.decline_reason == 0 && lay.n_reads == c.n_reads && lay.rec_pos && lay.seq_off && lay.rec_pos[lay.n_reads] == c.data.size() &&
                 lay.seq_off[lay.n_reads] == c.bases;
            for (uint64_t r = 0; ok && r < lay.n_reads; r++) ok = c.data[lay.rec_pos[r]] == '@' && lay.rec_pos[r] < lay.rec_pos[r + 1] && lay.seq_off[r] <= lay.seq_off[r + 1];
        } else ok = rc == CRASS_ERR_UNSUPPORTED && lay.decline_reason == c.reason && lay.decline_pos == c.pos && !lay.rec_pos && !lay.seq_off && lay.n_reads == 0;
        printf("%s %s: rc %d, %llu records, reason %d at %llu\n", ok ? "ok  " : "DIFF", c.name, rc, (unsigned long long)lay.n_reads, lay.decline_reason,
               (unsigned long long)lay.decline_pos);
        bad += ok ? 0 : 1;
        crass_fastx_layout_free(&lay);
        // every prefix: accepted or declined, and class 0 on the same bytes is crass_fastx_scan_host
        uint64_t accepted = 0;
        for (size_t k = 0; k <= c.data.size() && k <= 400; k++) {
            const std::string pre = c.data.substr(0, k);
            crass_fastx_layout a, b, b0;
            const int ra = scan(pre, 1, &a), rb = scan(pre, 0, &b);
            uint8_t *exact = pre.empty() ? nullptr : (uint8_t *)malloc(pre.size());
            if (exact) memcpy(exact, pre.data(), pre.size());
            const int r0 = crass_fastx_scan_host(exact, pre.size(), &b0);
            free(exact);
            const bool same0 = rb == r0 && b.n_reads == b0.n_reads && b.decline_reason == b0.decline_reason && b.decline_pos == b0.decline_pos;
            const bool sane = (ra == CRASS_OK && a.rec_pos[a.n_reads] == k) || (ra == CRASS_ERR_UNSUPPORTED && a.decline_reason > 0 && a.decline_pos <= k);
            // what four lines accept, the wrapped rule accepts with the same records
            const bool super = rb != CRASS_OK || (ra == CRASS_OK && a.n_reads == b.n_reads && !memcmp(a.rec_pos, b.rec_pos, (a.n_reads + 1) * 8) && !memcmp(a.seq_off, b.seq_off, (a.n_reads + 1) * 8));
            if (!same0 || !sane || !super) { printf("DIFF %s prefix %zu\n", c.name, k); bad++; }
            accepted += ra == CRASS_OK;
            crass_fastx_layout_free(&a); crass_fastx_layout_free(&b); crass_fastx_layout_free(&b0);
        }
        (void)accepted;
    }
    // the accepted inputs as one set, and a set whose second file is declined
    std::vector<const uint8_t *> ptr; std::vector<uint64_t> len;
    uint64_t reads = 0;
    for (const Case &c : cases) if (c.reason == 0) { ptr.push_back((const uint8_t *)c.data.data()); len.push_back(c.data.size()); reads += c.n_reads; }
    crass_fastx_files_layout fl;
    int rc = crass_fastx_files_scan_host_class(ptr.data(), len.data(), (uint32_t)ptr.size(), 1, &fl);
    bool ok = rc == CRASS_OK && fl.n_reads == reads && fl.decline_file == -1;
    crass_fastx_files_layout_free(&fl);
    ptr.resize(1); len.resize(1);
    for (const Case &c : cases) if (c.reason == 12) { ptr.push_back((const uint8_t *)c.data.data()); len.push_back(c.data.size()); }
    rc = crass_fastx_files_scan_host_class(ptr.data(), len.data(), (uint32_t)ptr.size(), 1, &fl);
    ok = ok && rc == CRASS_ERR_UNSUPPORTED && fl.decline_file == 1 && fl.decline_reason == 12 && !fl.rec_pos;
    crass_fastx_files_layout_free(&fl);
    crass_fastx_layout l;
    ok = ok && crass_fastx_scan_host_class((const uint8_t *)"@", 1, 2, &l) == CRASS_ERR_INVALID_ARG && crass_fastx_scan_host_class(nullptr, 1, 1, &l) == CRASS_ERR_INVALID_ARG;
    printf("%s sets and argument errors\n", ok ? "ok  " : "DIFF");
    bad += ok ? 0 : 1;
    printf("%s: %zu inputs, %d differ\n", bad ? "FAILED" : "passed", cases.size(), bad);
    return bad ? 1 : 0;
}

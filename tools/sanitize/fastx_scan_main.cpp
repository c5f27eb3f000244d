// AddressSanitizer / UBSan harness for the record scan's host code (csrc/fastx_scan.cpp + csrc/fastx_scan.h), next to ingest_main.cpp:
// every file given — the sets of tests/fastx_sets.py, dumped by tools/sanitize/fastx_scan_dump.py — goes through crass_fastx_scan_host
// and, where it is accepted, crass_fastx_header_ids; the four-bytes-at-once byte classes of fastx_scan.h are compared with the
// byte predicates for every byte value in every position.  CPU only.  Prints one line per file; any sanitizer report fails the run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp \
//       tools/sanitize/fastx_scan_main.cpp -o fastx_scan_asan && python3 tools/sanitize/fastx_scan_dump.py DIR && ./fastx_scan_asan DIR/*
#include "../../include/crass_hip.h"
#include "../../crass_amd/csrc/fastx_scan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
static int check_classes()
{
    int bad = 0;
    for (int pos = 0; pos < 4; pos++)
        for (int b = 0; b < 256; b++) {
            const uint32_t v = 0x41004100u ^ ((0x41004100u >> (8 * pos) & 0xFFu) << (8 * pos)) | ((uint32_t)b << (8 * pos));
            const crass::FxClass4 c = crass::fx_class4(v);
            const uint8_t x = (uint8_t)b;
            const bool ok = ((c.nl >> pos) & 1u) == (uint32_t)crass::fx_is_nl(x) && ((c.gt >> pos) & 1u) == (uint32_t)(x == '>') &&
                            ((c.at >> pos) & 1u) == (uint32_t)(x == '@') && ((c.plus >> pos) & 1u) == (uint32_t)(x == '+') &&
                            ((c.del >> pos) & 1u) == (uint32_t)crass::fx_is_del(x) && ((c.graph >> pos) & 1u) == (uint32_t)crass::fx_is_seq_byte(x) &&
                            (((c.gt | c.at | c.plus) >> pos) & 1u) == (uint32_t)crass::fx_is_forbidden(x) && (((c.gt | c.at) >> pos) & 1u) == (uint32_t)crass::fx_is_hdr_char(x);
            // the other three bytes are 'A' or 0: 'A' is a sequence byte and nothing else, 0 is in no class
            for (int q = 0; q < 4; q++) if (q != pos) {
                const uint32_t other = (v >> (8 * q)) & 0xFFu;
                if (((c.graph >> q) & 1u) != (other == 0x41u ? 1u : 0u) || (((c.nl | c.gt | c.at | c.plus | c.del) >> q) & 1u)) bad++;
            }
            if (!ok) { printf("DIFF class of byte %d at position %d\n", b, pos); bad++; }
        }
    printf("%s byte classes: 1024 cases\n", bad ? "DIFF" : "ok  ");
    return bad;
}
int main(int argc, char **argv)
{
    int bad = check_classes();
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
        crass_fastx_layout lay;
        const int rc = crass_fastx_scan_host(exact, data.size(), &lay);
        bool ok = rc == CRASS_OK ? (lay.decline_reason == 0 && lay.rec_pos && lay.seq_off && lay.rec_pos[lay.n_reads] == data.size())
                                 : (rc == CRASS_ERR_UNSUPPORTED && lay.decline_reason != 0 && !lay.rec_pos && !lay.seq_off);
        unsigned long long dup = 0;
        if (rc == CRASS_OK) {
            std::vector<uint64_t> hid(lay.n_reads);
            ok = ok && crass_fastx_header_ids(exact, data.size(), lay.rec_pos, lay.n_reads, hid.data()) == CRASS_OK;
            for (uint64_t r = 0; r < lay.n_reads; r++) { ok = ok && hid[r] <= r && hid[hid[r]] == hid[r]; dup += hid[r] != r; }
        }
        printf("%s %s: rc %d, %llu records, %llu bases, %llu repeated names, reason %d at %llu\n", ok ? "ok  " : "DIFF", argv[a], rc,
               (unsigned long long)lay.n_reads, (unsigned long long)(rc == CRASS_OK ? lay.seq_off[lay.n_reads] : 0), dup, lay.decline_reason,
               (unsigned long long)lay.decline_pos);
        bad += ok ? 0 : 1;
        crass_fastx_layout_free(&lay);
        free(exact);
    }
    return bad ? 1 : 0;
}

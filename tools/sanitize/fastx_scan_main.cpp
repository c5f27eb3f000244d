// AddressSanitizer / UBSan harness for the record scan's host code (csrc/fastx_scan.cpp + csrc/fastx_scan.h), next to ingest_main.cpp:
// every file given — the sets of tests/fastx_sets.py, dumped by tools/sanitize/fastx_scan_dump.py — goes through crass_fastx_scan_host
// and, where it is accepted, crass_fastx_header_ids; the four-bytes-at-once byte classes of fastx_scan.h are compared with the
// byte predicates for every byte value in every position.  Then all files given go through crass_fastx_files_scan_host as ONE set,
// and every file with its successor as a set of two (plain files; a BGZF file among them is inflated by the host decoder): the
// joined arrays are checked against the single-file scans.  CPU only.  Prints one line per file; any sanitizer report fails the run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
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
// files [a, b) as one set against their single-file scans (plain files: a BGZF one only has to come back accepted or declined)
static int check_set(const std::vector<uint8_t *> &ptr, const std::vector<uint64_t> &len, size_t a, size_t b)
{
    crass_fastx_files_layout lay;
    const int rc = crass_fastx_files_scan_host(ptr.data() + a, len.data() + a, (uint32_t)(b - a), &lay);
    bool ok = rc == CRASS_OK || rc == CRASS_ERR_UNSUPPORTED;
    uint64_t reads = 0, at = 0;
    for (size_t f = a; ok && f < b; f++) {
        crass_fastx_layout one;
        const int r1 = crass_fastx_scan_host(ptr[f], len[f], &one);
        const bool plain = !(len[f] >= 2 && ptr[f][0] == 0x1F && ptr[f][1] == 0x8B);
        if (rc == CRASS_ERR_UNSUPPORTED && (size_t)lay.decline_file == f - a) {
            ok = !lay.rec_pos && !lay.seq_off && !lay.file_read_base && (!plain || (r1 == CRASS_ERR_UNSUPPORTED && one.decline_reason == lay.decline_reason && one.decline_pos == lay.decline_pos));
            crass_fastx_layout_free(&one);
            break;
        }
        if (rc == CRASS_OK && plain) {
            ok = r1 == CRASS_OK && lay.file_read_base[f - a] == reads && lay.file_byte_base[f - a] == at && lay.format[f - a] == one.format;
            for (uint64_t r = 0; ok && r < one.n_reads; r++) ok = lay.rec_pos[reads + r] == at + one.rec_pos[r] && lay.seq_off[reads + r + 1] - lay.seq_off[reads + r] == one.seq_off[r + 1] - one.seq_off[r];
            reads += one.n_reads; at += len[f] + 1;
        } else if (rc == CRASS_OK) { reads = lay.file_read_base[f - a + 1]; at = lay.file_byte_base[f - a + 1]; }
        else if (plain) ok = r1 == CRASS_OK;             // (a file in front of the declined one)
        crass_fastx_layout_free(&one);
    }
    if (rc == CRASS_OK) ok = ok && lay.n_reads == reads && lay.file_byte_base[b - a] == at && lay.rec_pos[reads] == at - 1;
    printf("%s set of files %zu..%zu: rc %d, %llu records, declined file %d\n", ok ? "ok  " : "DIFF", a, b - 1, rc, (unsigned long long)lay.n_reads, lay.decline_file);
    crass_fastx_files_layout_free(&lay);
    return ok ? 0 : 1;
}
int main(int argc, char **argv)
{
    int bad = check_classes();
    std::vector<uint8_t *> all_ptr; std::vector<uint64_t> all_len;
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
        all_ptr.push_back(exact); all_len.push_back(data.size());
    }
    if (!all_ptr.empty()) {
        for (size_t f = 0; f + 1 < all_ptr.size(); f++) bad += check_set(all_ptr, all_len, f, f + 2);
        bad += check_set(all_ptr, all_len, 0, all_ptr.size());
        // the accepted files alone as one set: the joins of all of them
        std::vector<uint8_t *> ok_ptr; std::vector<uint64_t> ok_len;
        for (size_t f = 0; f < all_ptr.size(); f++) {
            crass_fastx_layout one;
            if (crass_fastx_scan_host(all_ptr[f], all_len[f], &one) == CRASS_OK) { ok_ptr.push_back(all_ptr[f]); ok_len.push_back(all_len[f]); }
            crass_fastx_layout_free(&one);
        }
        if (!ok_ptr.empty()) bad += check_set(ok_ptr, ok_len, 0, ok_ptr.size());
    }
    for (uint8_t *p : all_ptr) free(p);
    return bad ? 1 : 0;
}

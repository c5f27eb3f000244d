// AddressSanitizer / UBSan harness for crass_fastx_comments_of (csrc/fastx_scan.cpp, the rule of csrc/fastx_scan.h), next to
// names_of_main.cpp: designed jobs of one to three files made here — comments on every third record, on none and on all, records
// in front of a file's first comment, own empty comments ("name \n", "name\t\n", "name\r\n") behind a non-empty one, CRLF, a
// comment of 300 bytes, names of 259, 260 and 300 bytes, a last header line without its '\n', 1 .. 4 097 records, 12 300 records
// whose only comment sits on record 4 095, a commented file in front of an uncommented one — go through crass_fastx_comments_of
// from exact-size heap copies of the arena (every file's text, a '\n' behind it), the positions, the indices, the offsets, the
// flags and an output of exactly the capacity: the capacity one byte short (CRASS_ERR_OVERFLOW, offsets and flags complete),
// exact and one byte long, both index bases, all records in reverse order with every third one twice.  What it must give is
// restated here by ONE forward walk per file that carries the last comment along, as kseq's buffer does.  Then the argument
// errors: nothing is written.  CPU only.  Prints one line per job; any sanitizer report fails the run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude crass_amd/csrc/fastx_scan.cpp crass_amd/csrc/bgzf.cpp \
//       tools/sanitize/comments_of_main.cpp -o comments_of_asan -lz && ./comments_of_asan
#include "../../include/crass_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
static bool is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

struct Job {
    std::string arena;                                  // every file's text, a '\n' behind it
    std::vector<uint64_t> rec_pos, file_read_base;      // n_reads + 1 (the last: the arena's size), n_files + 1
    std::vector<int> has; std::vector<std::string> handed;      // per record: the forward walk's answer
};

// files of two-line FASTA records given as header lines (without '>'); line_end: "\n" or "\r\n"; open_end: the last file's last
// header line is the text's end (no line end, no sequence)
static Job make(const std::vector<std::vector<std::string>> &files, const char *line_end = "\n", bool open_end = false)
{
    Job J;
    J.file_read_base.push_back(0);
    for (size_t f = 0; f < files.size(); f++) {
        std::string text;
        bool have = false; std::string carried;           // kseq's comment buffer: one per file
        for (size_t i = 0; i < files[f].size(); i++) {
            const std::string &h = files[f][i];
            const bool last = open_end && f + 1 == files.size() && i + 1 == files[f].size();
            J.rec_pos.push_back(J.arena.size() + text.size());
            const std::string line = last ? h : h + (strcmp(line_end, "\n") ? "\r" : "");      // the line's bytes in front of its '\n'
            size_t e = 0;
            while (e < line.size() && !is_space((uint8_t)line[e])) e++;
            if (e < line.size()) { have = true; carried = line.substr(e + 1); }
            J.has.push_back(have ? 1 : 0); J.handed.push_back(have ? carried : std::string());
            text += ">" + h;
            if (!last) text += std::string(line_end) + "ACGT" + line_end;
        }
        J.arena += text + "\n";
        J.file_read_base.push_back(J.rec_pos.size());
    }
    J.rec_pos.push_back(J.arena.size());
    return J;
}

template <class T> static T *exact(const std::vector<T> &v) { T *p = v.empty() ? nullptr : (T *)malloc(v.size() * sizeof(T)); if (p) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

static bool one(const Job &J, const std::vector<uint64_t> &idx, uint64_t base, int64_t slack, bool one_file_null)
{
    std::string want; std::vector<uint64_t> woff(1, 0); std::vector<uint8_t> whas;
    for (uint64_t r : idx) { want += J.handed[r]; woff.push_back(want.size()); whas.push_back((uint8_t)J.has[r]); }
    if (slack < 0 && want.size() < (uint64_t)-slack) return true;
    const uint64_t cap = want.size() + slack, n = idx.size(), nr = J.rec_pos.size() - 1;
    uint8_t *bytes = (uint8_t *)malloc(J.arena.size());
    memcpy(bytes, J.arena.data(), J.arena.size());
    uint64_t *rp = exact(J.rec_pos), *fb = exact(J.file_read_base);
    std::vector<uint64_t> shifted(idx);
    for (auto &x : shifted) x += base;
    uint64_t *ix = exact(shifted), *off = (uint64_t *)malloc((n + 1) * 8);
    uint8_t *has = n ? (uint8_t *)malloc(n) : nullptr, *out = cap ? (uint8_t *)malloc(cap) : nullptr;
    const int st = crass_fastx_comments_of(bytes, J.arena.size(), rp, nr, one_file_null ? nullptr : fb, one_file_null ? 0 : (uint32_t)(J.file_read_base.size() - 1),
                                           ix, n, base, out, cap, off, has);
    bool ok = st == (cap < want.size() ? CRASS_ERR_OVERFLOW : CRASS_OK);
    ok = ok && memcmp(off, woff.data(), (n + 1) * 8) == 0 && (n == 0 || memcmp(has, whas.data(), n) == 0);
    const uint64_t m = cap < want.size() ? cap : want.size();
    ok = ok && (m == 0 || memcmp(out, want.data(), m) == 0);
    free(bytes); free(rp); free(fb); free(ix); free(off); free(has); free(out);
    return ok;
}

static bool check(const char *name, const Job &J)
{
    const uint64_t nr = J.rec_pos.size() - 1;
    std::vector<uint64_t> idx;
    for (uint64_t r = nr; r-- > 0;) { idx.push_back(r); if (r % 3 == 0) idx.push_back(r); }
    bool ok = true;
    uint64_t handed = 0;
    for (uint64_t r = 0; r < nr; r++) handed += J.has[r] ? 1 : 0;
    const bool single = J.file_read_base.size() == 2;
    for (uint64_t base : {0ull, 7ull}) for (int64_t slack : {-1, 0, 1}) ok = ok && one(J, idx, base, slack, false) && (!single || one(J, idx, base, slack, true));
    ok = ok && one(J, {}, 0, 0, false);
    for (uint64_t r = 0; r < nr && r < 70; r++) ok = ok && one(J, {r}, 0, 0, false);
    printf("%s %s: %llu records in %zu file(s), %llu are handed a comment\n", ok ? "ok  " : "DIFF", name, (unsigned long long)nr, J.file_read_base.size() - 1,
           (unsigned long long)handed);
    return ok;
}

static bool errors()
{
    const Job J = make({{"a c", "b", "c"}, {"d"}});
    const uint64_t nr = 4, nb = J.arena.size();
    const uint8_t *b = (const uint8_t *)J.arena.data();
    bool ok = true;
    for (uint64_t base : {0ull, 7ull}) {
        uint64_t off[3] = {5, 5, 5}, bad[2] = {base, base + nr};
        uint8_t has[2] = {9, 9}, out[8];
        memset(out, 0xA5, 8);
        ok = ok && crass_fastx_comments_of(b, nb, J.rec_pos.data(), nr, J.file_read_base.data(), 2, bad, 2, base, out, 8, off, has) == CRASS_ERR_INVALID_ARG;
        if (base) { bad[1] = base - 1; ok = ok && crass_fastx_comments_of(b, nb, J.rec_pos.data(), nr, J.file_read_base.data(), 2, bad, 2, base, out, 8, off, has) == CRASS_ERR_INVALID_ARG; }
        for (uint8_t x : out) ok = ok && x == 0xA5;
        ok = ok && off[0] == 5 && off[1] == 5 && off[2] == 5 && has[0] == 9 && has[1] == 9;
    }
    uint64_t off[2] = {5, 5}, ix[1] = {0};
    uint8_t has[1] = {9};
    const uint64_t *rp = J.rec_pos.data(), *fb = J.file_read_base.data();
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, fb, 2, nullptr, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, fb, 2, ix, 1, 0, nullptr, 0, nullptr, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(nullptr, nb, rp, nr, fb, 2, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(b, nb, nullptr, nr, fb, 2, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, fb, 2, ix, 1, 0, nullptr, 3, off, has) == CRASS_ERR_INVALID_ARG;
    const uint64_t short_fb[3] = {0, 3, 3}, down_fb[3] = {0, 4, 4}, late_fb[3] = {1, 3, 4}, back_fb[4] = {0, 3, 2, 4};
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, short_fb, 2, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, down_fb, 2, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_OVERFLOW;      // (a last file of no records is fine: "c" is handed)
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, late_fb, 2, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, back_fb, 3, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, fb, 0, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;
    const uint64_t far_rp[5] = {0, nb, 0, 0, nb};
    off[0] = off[1] = 5; has[0] = 9;
    ok = ok && crass_fastx_comments_of(b, nb, far_rp, nr, fb, 2, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG && off[0] == 5 && off[1] == 5 && has[0] == 9;
    ok = ok && crass_fastx_comments_of(nullptr, 0, nullptr, 0, nullptr, 0, ix, 1, 0, nullptr, 0, off, has) == CRASS_ERR_INVALID_ARG;      // (no records: every index is out of range)
    ok = ok && crass_fastx_comments_of(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, 0, off, nullptr) == CRASS_OK && off[0] == 0;
    ok = ok && crass_fastx_comments_of(b, nb, rp, nr, fb, 2, ix, 1, 0, nullptr, 0, off, nullptr) == CRASS_ERR_OVERFLOW && off[1] == 1;      // (has_out may be NULL)
    printf("%s argument errors\n", ok ? "ok  " : "DIFF");
    return ok;
}

static std::vector<std::string> headers(uint64_t n, uint64_t every, uint64_t first, const char *tag)
{
    std::vector<std::string> h;
    for (uint64_t r = 0; r < n; r++) {
        std::string s = std::string(tag) + std::to_string(r);
        if (every && r >= first && (r - first) % every == 0) s += " c" + std::to_string(r * 7);
        h.push_back(s);
    }
    return h;
}

int main()
{
    int bad = 0;
    auto run = [&](const char *name, const Job &J) { bad += check(name, J) ? 0 : 1; };
    run("every third", make({headers(30, 3, 0, "r")}));
    run("none", make({headers(30, 0, 0, "r")}));
    run("all", make({headers(30, 1, 0, "r")}));
    run("late first", make({headers(30, 4, 9, "r")}));
    run("empty own", make({{"a first", "b ", "c", "d\t", "e", "f second", "g\r", "h", "i\v", "j", "k \t ", "l"}}));
    run("crlf", make({headers(20, 2, 1, "r")}, "\r\n"));
    run("long comment", make({{"a", "b " + std::string(300, 'x'), "c", "d"}}));
    run("long names", make({{"z zero", std::string(259, 'a'), std::string(259, 'b') + " c259", std::string(260, 'c'), std::string(260, 'd') + "\tc260",
                             std::string(300, 'e'), std::string(300, 'f') + " c300", "y"}}));
    run("open end, comment", make({{"a", "b c", "c", "last tail comment"}}, "\n", true));
    run("open end, none", make({{"a", "b c", "c", "last"}}, "\n", true));
    run("open end, blank", make({{"a", "b c", "c", "last "}}, "\n", true));
    for (uint64_t n : {1, 63, 64, 65, 4095, 4096, 4097}) run(("count " + std::to_string(n)).c_str(), make({headers(n, 5, 2, "r")}));
    run("one record, comment", make({{"only one"}}));
    { std::vector<std::string> h = headers(12300, 0, 0, ""); for (auto &s : h) s = "r"; h[4095] = "r only"; run("sparse", make({h})); }
    run("two files", make({headers(10, 1, 0, "a"), headers(10, 0, 0, "b")}));
    run("three files", make({headers(100, 3, 2, "a"), headers(50, 0, 0, "b"), headers(70, 4, 5, "c")}));
    run("open end between files", make({{"a c", "b"}, {"d", "e f", "g"}}));
    bad += errors() ? 0 : 1;
    printf("%s: %d failures\n", bad ? "DIFF" : "ok  ", bad);
    return bad ? 1 : 0;
}

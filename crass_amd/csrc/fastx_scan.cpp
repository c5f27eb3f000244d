// fastx_scan.cpp — the record scan of fastx_scan.h on the host, one byte after the other: the restatement the device scan
// (fastx_scan.hip) is tested against, the header ids of a scanned file, and the host arithmetic of a rank's shard
// (fastx_shards.h: the BGZF members of a text range, the staging placement).  Host-only C++17 that any compiler builds
// (tools/sanitize).
#include "../../include/crass_hip.h"
#include "fastx_scan.h"
#include "fastx_shards.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace crass {

int fastx_scan_serial(const uint8_t *bytes, uint64_t n, FxHostScan *out)
{
    *out = FxHostScan();
    auto decline = [&](uint64_t pos, int32_t reason) { out->reason = reason; out->decline_pos = pos; out->n_reads = 0; out->max_len = 0; return CRASS_ERR_UNSUPPORTED; };
    if (n == 0) return decline(0, FX_EMPTY);
    if (!fx_is_hdr_char(bytes[0])) return decline(0, FX_FIRST_BYTE);
    out->format = bytes[0];
    const bool fastq = bytes[0] == 0x40;
    uint64_t n_lines = 0;
    if (fastq) {
        for (uint64_t i = 0; i < n; i++) n_lines += fx_is_nl(bytes[i]) ? 1 : 0;
        if (!fx_is_nl(bytes[n - 1])) n_lines++;
    }
    const uint64_t first_partial = n_lines & ~3ull;      // FASTQ: index of the first line of an incomplete record
    std::vector<uint64_t> rec_pos, seq_off;
    try {
        uint64_t seq = 0, qual = 0, idx = 0, max_len = 0;
        uint32_t kind = FX_QUAL;                          // (FASTQ: the kind of the line before line 0)
        for (uint64_t p = 0; p < n; idx++) {
            uint64_t e = p;
            while (e < n && !fx_is_nl(bytes[e])) e++;     // the line: [p, e), its '\n' (if any) at e
            uint64_t off = kFxNoOffence;
            auto offend = [&](uint32_t reason) { const uint64_t o = fx_offence(p, reason); if (o < off) off = o; };
            kind = fastq ? (kind + 1) & 3u : (bytes[p] == 0x3E ? FX_HEADER : FX_SEQ);
            uint64_t graph = 0;
            bool forbidden = false, del = false;
            for (uint64_t i = p; i < e; i++) { graph += fx_is_seq_byte(bytes[i]) ? 1 : 0; forbidden |= fx_is_forbidden(bytes[i]); del |= fx_is_del(bytes[i]); }
            if (kind == FX_HEADER) {
                if (fastq && (n_lines & 3) && idx == first_partial) offend(FX_LINE_COUNT);
                if (fastq && bytes[p] != 0x40) offend(FX_FQ_HEADER);
                if (!fastq && p == n - 1) offend(FX_LONE_HEADER);
                if (!rec_pos.empty()) max_len = std::max<uint64_t>(max_len, seq - seq_off.back());
                rec_pos.push_back(p); seq_off.push_back(seq);
            } else if (kind == FX_SEQ) {
                if (forbidden) offend(FX_SEQ_CHAR);
                seq += graph;
            } else if (kind == FX_PLUS) {
                if (bytes[p] != 0x2B) offend(FX_FQ_PLUS);
            } else {
                if (del) offend(FX_QUAL_DEL);
                qual += graph;
                if (seq > qual) offend(FX_QUAL_SHORT);
                if (seq < qual) offend(FX_QUAL_LONG);
            }
            if (off != kFxNoOffence) return decline(off >> 8, (int32_t)(off & 0xFF));
            p = e + 1;
        }
        max_len = std::max<uint64_t>(max_len, seq - seq_off.back());      // (byte 0 starts a header line: there is a record)
        rec_pos.push_back(n); seq_off.push_back(seq);
        out->n_reads = rec_pos.size() - 1;
        out->max_len = (uint32_t)std::min<uint64_t>(max_len, 0xFFFFFFFFull);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    const size_t bytes_arr = rec_pos.size() * sizeof(uint64_t);
    out->rec_pos = (uint64_t *)malloc(bytes_arr); out->seq_off = (uint64_t *)malloc(bytes_arr);
    if (!out->rec_pos || !out->seq_off) { free(out->rec_pos); free(out->seq_off); *out = FxHostScan(); return CRASS_ERR_OOM; }
    memcpy(out->rec_pos, rec_pos.data(), bytes_arr); memcpy(out->seq_off, seq_off.data(), bytes_arr);
    return CRASS_OK;
}

// the wrapped FASTQ rule of fastx_scan.h, record by record from line 0: each record is judged from where the one before ended
static int fastx_scan_wrapped_serial(const uint8_t *bytes, uint64_t n, FxHostScan *out)
{
    *out = FxHostScan();
    out->format = 0x40;
    auto decline = [&](uint64_t pos, int32_t reason) { out->reason = reason; out->decline_pos = pos; out->n_reads = 0; out->max_len = 0; return CRASS_ERR_UNSUPPORTED; };
    struct Line { uint64_t e, graph; bool forbidden, del, is_void; };
    auto line_at = [&](uint64_t p) {                     // the line that starts at p < n: [p, e), its '\n' (if any) at e
        Line l{p, 0, false, false, true};
        for (; l.e < n && !fx_is_nl(bytes[l.e]); l.e++) {
            const uint8_t b = bytes[l.e];
            l.graph += fx_is_seq_byte(b) ? 1 : 0; l.forbidden |= fx_is_forbidden(b); l.del |= fx_is_del(b); l.is_void &= fx_is_void_byte(b);
        }
        return l;
    };
    std::vector<uint64_t> rec_pos, seq_off;
    try {
        uint64_t seq = 0, max_len = 0;
        for (uint64_t hdr = 0; hdr < n;) {               // (byte hdr is '@')
            uint64_t p = line_at(hdr).e + 1, L = 0, first_forbidden = kFxNone;
            bool plus = false, plus_ended = false;
            while (p < n && !plus) {                     // the sequence lines, up to the first line that starts with '+'
                const Line l = line_at(p);
                if (bytes[p] == 0x2B) { plus = true; plus_ended = l.e < n; }
                else { L += l.graph; if (l.forbidden && first_forbidden == kFxNone) first_forbidden = p; }
                p = l.e + 1;
            }
            if (!plus) return decline(hdr, FX_LINE_COUNT);
            if (first_forbidden != kFxNone) return decline(first_forbidden, FX_SEQ_CHAR);
            if (L == 0 && p < n && bytes[p] == 0x40) return decline(p, FX_FQ_EMPTY_SEQ);
            uint64_t count = 0, first_del = kFxNone, passed = kFxNone;
            while (plus_ended && count < L && p < n) {   // the quality lines
                const Line l = line_at(p);
                if (l.del && first_del == kFxNone) first_del = p;
                count += l.graph;
                if (count > L) passed = p;
                p = l.e + 1;
            }
            if (first_del != kFxNone) return decline(first_del, FX_QUAL_DEL);
            if (passed != kFxNone) return decline(passed, FX_QUAL_LONG);
            if (!plus_ended || count < L) return decline(hdr, FX_QUAL_SHORT);
            while (p < n) {                              // void lines
                const Line l = line_at(p);
                if (!l.is_void) break;
                p = l.e + 1;
            }
            if (p < n && bytes[p] != 0x40) return decline(p, FX_FQ_HEADER);
            rec_pos.push_back(hdr); seq_off.push_back(seq);
            seq += L; max_len = std::max(max_len, L);
            hdr = p;
        }
        rec_pos.push_back(n); seq_off.push_back(seq);
        out->n_reads = rec_pos.size() - 1;
        out->max_len = (uint32_t)std::min<uint64_t>(max_len, 0xFFFFFFFFull);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    const size_t bytes_arr = rec_pos.size() * sizeof(uint64_t);
    out->rec_pos = (uint64_t *)malloc(bytes_arr); out->seq_off = (uint64_t *)malloc(bytes_arr);
    if (!out->rec_pos || !out->seq_off) { free(out->rec_pos); free(out->seq_off); *out = FxHostScan(); return CRASS_ERR_OOM; }
    memcpy(out->rec_pos, rec_pos.data(), bytes_arr); memcpy(out->seq_off, seq_off.data(), bytes_arr);
    return CRASS_OK;
}

int fastx_scan_class_serial(const uint8_t *bytes, uint64_t n, int32_t fastq_class, FxHostScan *out)
{
    if (fastq_class == FX_CLASS_WRAPPED && n && bytes[0] == 0x40) return fastx_scan_wrapped_serial(bytes, n, out);
    return fastx_scan_serial(bytes, n, out);
}

// the probe of fastx_scan.h, one byte after the other
int fx_probe_serial(const uint8_t *bytes, uint64_t n, bool left_is_ls, FxProbe *out)
{
    FxProbe P{};
    P.gt = kFxNone;
    for (int k = 0; k < 4; k++) P.ls[k] = kFxNone;
    bool ls = left_is_ls;
    for (uint64_t i = 0; i < n; i++) {
        if (ls) {
            if (P.n_ls < 4) P.ls[P.n_ls++] = i;
            if (bytes[i] == 0x3E && P.gt == kFxNone) P.gt = i;
        }
        ls = fx_is_nl(bytes[i]);
        P.n_nl += ls ? 1 : 0;
    }
    *out = P;
    return CRASS_OK;
}

// ---- the host arithmetic of a rank's shard (fastx_shards.h) ----
void bgzf_members_for(const uint64_t *oo, uint64_t n, uint64_t a, uint64_t b, uint64_t *m0, uint64_t *m1)
{
    *m0 = a == 0 ? 0 : (uint64_t)(std::upper_bound(oo + 1, oo + n + 1, a) - (oo + 1));      // the first member that ends behind a
    uint64_t e = (uint64_t)(std::upper_bound(oo + 1, oo + n + 1, b) - (oo + 1));            // ... behind b
    if (e < n && oo[e] < b) e++;
    *m1 = e;
}

uint64_t shard_stage_place(const uint64_t *sa, const uint64_t *sb, uint64_t n, uint64_t *off)
{
    uint64_t cursor = 0;
    for (uint64_t k = 0; k < n; k++) {
        off[k] = ((cursor + 15) & ~15ull) + (sa[k] & 15u);
        cursor = off[k] + (sb[k] - sa[k]);
    }
    return cursor + 32;
}

} // namespace crass

extern "C" {

int crass_fastx_cut_probe_host(const uint8_t *bytes, uint64_t n_bytes, int left_is_ls, uint64_t out[7])
{
    if (!out || (n_bytes && !bytes)) return CRASS_ERR_INVALID_ARG;
    crass::FxProbe P;
    crass::fx_probe_serial(bytes, n_bytes, left_is_ls != 0, &P);
    out[0] = P.n_nl; out[1] = P.n_ls; for (int k = 0; k < 4; k++) out[2 + k] = P.ls[k]; out[6] = P.gt;
    return CRASS_OK;
}

void crass_fastx_shards_free(crass_fastx_shards *s)
{
    if (!s) return;
    free((void *)s->rank_read_base); free((void *)s->cut_file); free((void *)s->cut_pos); free((void *)s->file_read_base); free((void *)s->format);
    s->rank_read_base = s->cut_pos = s->file_read_base = nullptr; s->cut_file = nullptr; s->format = nullptr;
}

// The cut rule of fastx_scan.h on the host.  The verdict is crass_fastx_files_scan_host's; an ACCEPTED file's record starts are
// that scan's rec_pos (regular FASTA: the line starts whose byte is '>'; regular FASTQ: the lines of index 0 modulo 4), so the
// actual cut is the first record position at or after the nominal one.
// Class 1: the same with crass_fastx_files_scan_host_class(.., 1, ..) — a wrapped file's rec_pos are the header lines of the
// records the wrapped rule walks from line 0, which is that class's definition of a record start.
int crass_fastx_files_shards_host_class(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, uint32_t n_ranks, const uint64_t *nominal,
                                        int fastq_class, crass_fastx_shards *out)
{
    if (!out) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->decline_file = -1; out->n_ranks = n_ranks; out->n_files = n_files;
    if (!n_ranks || n_ranks > 64 || fastq_class < 0 || fastq_class > 1) return CRASS_ERR_INVALID_ARG;
    crass_fastx_files_layout L;
    const int s = crass_fastx_files_scan_host_class(bytes, n_bytes, n_files, fastq_class, &L);
    out->decline_file = L.decline_file; out->decline_reason = L.decline_reason; out->decline_pos = L.decline_pos; out->bgzf = L.bgzf;
    if (s) return s;
    // text space: file f is [tb[f], tb[f + 1]); arena positions count one byte more per file in front
    std::vector<uint64_t> tb(n_files + 1);
    for (uint32_t f = 0; f <= n_files; f++) tb[f] = L.file_byte_base[f] - f;
    const uint64_t T = tb[n_files], nr = L.n_reads;
    for (uint32_t g = 1; nominal && g < n_ranks; g++)
        if (nominal[g - 1] > T || (g > 1 && nominal[g - 1] < nominal[g - 2])) { crass_fastx_files_layout_free(&L); return CRASS_ERR_INVALID_ARG; }
    uint64_t *rb = (uint64_t *)malloc((n_ranks + 1) * 8), *cp = (uint64_t *)malloc((n_ranks + 1) * 8), *fb = (uint64_t *)malloc((n_files + 1) * 8);
    uint32_t *cf = (uint32_t *)malloc((n_ranks + 1) * 4);
    int32_t *fm = (int32_t *)malloc(n_files * 4);
    if (!rb || !cp || !fb || !cf || !fm) { free(rb); free(cp); free(fb); free(cf); free(fm); crass_fastx_files_layout_free(&L); return CRASS_ERR_OOM; }
    for (uint32_t g = 0; g <= n_ranks; g++) {
        const uint64_t x = g == 0 ? 0 : g == n_ranks ? T : nominal ? nominal[g - 1] : (uint64_t)((unsigned __int128)T * g / n_ranks);
        // the file that holds text position x, and the first record of the set at or behind it
        const uint32_t f = (uint32_t)(std::upper_bound(tb.begin(), tb.end(), x) - tb.begin()) - 1;
        uint64_t r = nr;
        if (f < n_files) r = (uint64_t)(std::lower_bound(L.rec_pos, L.rec_pos + nr, x + f) - L.rec_pos);
        rb[g] = r;
        if (r == nr) { cf[g] = n_files; cp[g] = 0; }
        else {
            const uint32_t rf = (uint32_t)(std::upper_bound(L.file_read_base, L.file_read_base + n_files + 1, r) - L.file_read_base) - 1;
            cf[g] = rf; cp[g] = L.rec_pos[r] - L.file_byte_base[rf];
        }
    }
    memcpy(fb, L.file_read_base, (n_files + 1) * 8); memcpy(fm, L.format, n_files * 4);
    out->n_reads = nr; out->max_len = L.max_len;
    out->rank_read_base = rb; out->cut_file = cf; out->cut_pos = cp; out->file_read_base = fb; out->format = fm;
    crass_fastx_files_layout_free(&L);
    return CRASS_OK;
}

int crass_fastx_files_shards_host(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, uint32_t n_ranks, const uint64_t *nominal,
                                  crass_fastx_shards *out)
{
    return crass_fastx_files_shards_host_class(bytes, n_bytes, n_files, n_ranks, nominal, crass::FX_CLASS_FOUR_LINE, out);
}

int crass_fastx_scan_host_class(const uint8_t *bytes, uint64_t n_bytes, int fastq_class, crass_fastx_layout *out)
{
    if (!out || (n_bytes && !bytes) || fastq_class < 0 || fastq_class > 1) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    crass::FxHostScan h;
    const int s = crass::fastx_scan_class_serial(bytes, n_bytes, fastq_class, &h);
    out->n_reads = h.n_reads; out->format = h.format; out->decline_reason = h.reason; out->decline_pos = h.decline_pos; out->max_len = h.max_len;
    out->rec_pos = h.rec_pos; out->seq_off = h.seq_off;
    return s;
}

int crass_fastx_scan_host(const uint8_t *bytes, uint64_t n_bytes, crass_fastx_layout *out)
{
    return crass_fastx_scan_host_class(bytes, n_bytes, crass::FX_CLASS_FOUR_LINE, out);
}

void crass_fastx_layout_free(crass_fastx_layout *l)
{
    if (!l) return;
    free((void *)l->rec_pos); free((void *)l->seq_off);
    l->rec_pos = nullptr; l->seq_off = nullptr;
}

// several files as one set (crass_hip_load_fastx_files' restatement): file after file, the first that is declined ends the walk
int crass_fastx_files_scan_host_class(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int fastq_class,
                                      crass_fastx_files_layout *out)
{
    if (!out || fastq_class < 0 || fastq_class > 1) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->decline_file = -1;
    if (!n_files || !bytes || !n_bytes) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (n_bytes[f] && !bytes[f]) return CRASS_ERR_INVALID_ARG;
    out->n_files = n_files;
    std::vector<uint64_t> read_base(1, 0), byte_base(1, 0), rec_pos, seq_off;
    std::vector<int32_t> format;
    uint32_t max_len = 0;
    int status = CRASS_OK;
    try {
        std::vector<uint8_t> text;
        for (uint32_t f = 0; f < n_files && status == CRASS_OK; f++) {
            const uint8_t *b = bytes[f];
            uint64_t n = n_bytes[f];
            if (n >= 2 && b[0] == 0x1F && b[1] == 0x8B) {      // compressed: BGZF or nothing
                crass_bgzf_index ix;
                status = crass_bgzf_index_host(b, n, &ix);
                if (status == CRASS_ERR_UNSUPPORTED) { out->decline_file = (int32_t)f; out->bgzf = ix.decline; }
                if (status == CRASS_OK) {
                    text.resize(ix.out_off[ix.n_members] + 1);
                    crass_bgzf_verdict v;
                    memset(&v, 0, sizeof(v));
                    status = crass_bgzf_inflate_host(b, n, &ix, text.data(), text.size(), &v);
                    if (status == CRASS_ERR_UNSUPPORTED) { out->decline_file = (int32_t)f; out->bgzf = v; }
                    n = ix.out_off[ix.n_members]; b = text.data();
                }
                crass_bgzf_index_free(&ix);
                if (status != CRASS_OK) break;
            }
            crass::FxHostScan h;
            status = crass::fastx_scan_class_serial(b, n, fastq_class, &h);
            if (status == CRASS_ERR_UNSUPPORTED) { out->decline_file = (int32_t)f; out->decline_reason = h.reason; out->decline_pos = h.decline_pos; }
            if (status == CRASS_OK) {
                const uint64_t t0 = seq_off.empty() ? 0 : seq_off.back();
                if (!seq_off.empty()) { rec_pos.pop_back(); seq_off.pop_back(); }      // (the entry behind the file before)
                for (uint64_t r = 0; r <= h.n_reads; r++) { rec_pos.push_back(byte_base.back() + h.rec_pos[r]); seq_off.push_back(t0 + h.seq_off[r]); }
                read_base.push_back(read_base.back() + h.n_reads);
                byte_base.push_back(byte_base.back() + n + 1);      // (the '\n' behind the file)
                format.push_back(h.format);
                max_len = std::max(max_len, h.max_len);
            }
            free(h.rec_pos); free(h.seq_off);
        }
        if (status != CRASS_OK) return status;
        const uint64_t nr = read_base.back();
        uint64_t *a = (uint64_t *)malloc((n_files + 1) * 8), *bb = (uint64_t *)malloc((n_files + 1) * 8);
        uint64_t *rp = (uint64_t *)malloc((nr + 1) * 8), *so = (uint64_t *)malloc((nr + 1) * 8);
        int32_t *fm = (int32_t *)malloc(n_files * 4);
        if (!a || !bb || !rp || !so || !fm) { free(a); free(bb); free(rp); free(so); free(fm); return CRASS_ERR_OOM; }
        memcpy(a, read_base.data(), (n_files + 1) * 8); memcpy(bb, byte_base.data(), (n_files + 1) * 8);
        memcpy(rp, rec_pos.data(), (nr + 1) * 8); memcpy(so, seq_off.data(), (nr + 1) * 8); memcpy(fm, format.data(), n_files * 4);
        out->file_read_base = a; out->file_byte_base = bb; out->rec_pos = rp; out->seq_off = so; out->format = fm;
        out->n_reads = nr; out->max_len = max_len;
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int crass_fastx_files_scan_host(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, crass_fastx_files_layout *out)
{
    return crass_fastx_files_scan_host_class(bytes, n_bytes, n_files, crass::FX_CLASS_FOUR_LINE, out);
}

void crass_fastx_files_layout_free(crass_fastx_files_layout *l)
{
    if (!l) return;
    free((void *)l->file_read_base); free((void *)l->file_byte_base); free((void *)l->format); free((void *)l->rec_pos); free((void *)l->seq_off);
    l->file_read_base = l->file_byte_base = l->rec_pos = l->seq_off = nullptr; l->format = nullptr;
}

int crass_fastx_header_ids(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, uint64_t *header_id_out)
{
    if (n_reads && (!bytes || !rec_pos || !header_id_out)) return CRASS_ERR_INVALID_ARG;
    auto is_space = [](uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    try {
        std::unordered_map<std::string_view, uint64_t> first;
        first.reserve(n_reads * 2);
        for (uint64_t r = 0; r < n_reads; r++) {
            if (rec_pos[r] >= n_bytes) return CRASS_ERR_INVALID_ARG;
            uint64_t a = rec_pos[r] + 1, b = a;
            while (b < n_bytes && !is_space(bytes[b])) b++;      // the name: up to the first isspace() byte, as kseq cuts it
            header_id_out[r] = first.emplace(std::string_view((const char *)bytes + a, b - a), r).first->second;
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int crass_fastx_find_names(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, const uint8_t *names,
                           const uint64_t *name_off, uint64_t n_names, uint64_t *first_out)
{
    if ((n_reads && (!bytes || !rec_pos)) || (n_names && (!name_off || !first_out))) return CRASS_ERR_INVALID_ARG;
    for (uint64_t k = 0; k < n_names; k++) if (name_off[k + 1] < name_off[k]) return CRASS_ERR_INVALID_ARG;
    if (n_names && name_off[n_names] && !names) return CRASS_ERR_INVALID_ARG;
    auto is_space = [](uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    try {
        std::unordered_map<std::string_view, uint64_t> first;
        first.reserve(n_reads * 2);
        for (uint64_t r = 0; r < n_reads; r++) {
            if (rec_pos[r] >= n_bytes) return CRASS_ERR_INVALID_ARG;
            uint64_t a = rec_pos[r] + 1, b = a;
            while (b < n_bytes && !is_space(bytes[b])) b++;      // the name, as crass_fastx_header_ids cuts it
            first.emplace(std::string_view((const char *)bytes + a, b - a), r);
        }
        // (a query with an isspace() byte is looked up like any other: no name holds one, so it is not found)
        for (uint64_t k = 0; k < n_names; k++) {
            const uint64_t len = name_off[k + 1] - name_off[k];
            const auto it = first.find(std::string_view(len ? (const char *)names + name_off[k] : "", len));
            first_out[k] = it == first.end() ? CRASS_NAME_NOT_FOUND : it->second;
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int crass_fastx_names_of(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, const uint64_t *idx, uint64_t n,
                         uint64_t idx_base, uint8_t *out, uint64_t cap_bytes, uint64_t *off_out)
{
    if (!off_out || (n && !idx) || (n_reads && (!bytes || !rec_pos)) || (cap_bytes && !out)) return CRASS_ERR_INVALID_ARG;
    auto is_space = [](uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    off_out[0] = 0;
    // every index first: nothing is written to out by a call that fails with CRASS_ERR_INVALID_ARG
    for (uint64_t k = 0; k < n; k++) {
        if (idx[k] < idx_base || idx[k] - idx_base >= n_reads || rec_pos[idx[k] - idx_base] >= n_bytes) return CRASS_ERR_INVALID_ARG;
    }
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t a = rec_pos[idx[k] - idx_base] + 1;
        uint64_t b = a;
        while (b < n_bytes && !is_space(bytes[b])) b++;          // the name, as crass_fastx_header_ids cuts it
        const uint64_t at = off_out[k];
        if (at < cap_bytes) memcpy(out + at, bytes + a, (size_t)std::min(b - a, cap_bytes - at));      // (nothing at or beyond out + cap_bytes)
        off_out[k + 1] = at + (b - a);
    }
    return off_out[n] > cap_bytes ? CRASS_ERR_OVERFLOW : CRASS_OK;
}

// the comment kseq hands on (fastx_scan.h states the rule): the bitmap and the carries of ALL records first, serially — the
// structure the device builds with k_cm_bits / k_cm_tiles / k_cm_top —, then every listed record looks its source up in it
int crass_fastx_comments_of(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, const uint64_t *file_read_base,
                            uint32_t n_files, const uint64_t *idx, uint64_t n, uint64_t idx_base, uint8_t *out, uint64_t cap_bytes,
                            uint64_t *off_out, uint8_t *has_out)
{
    if (!off_out || (n && !idx) || (n_reads && (!bytes || !rec_pos)) || (cap_bytes && !out)) return CRASS_ERR_INVALID_ARG;
    const uint64_t one_file[2] = {0, n_reads};
    if (!file_read_base) { file_read_base = one_file; n_files = 1; }
    if (!n_files || file_read_base[0] != 0 || file_read_base[n_files] != n_reads) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (file_read_base[f + 1] < file_read_base[f]) return CRASS_ERR_INVALID_ARG;
    // every index and position first: nothing is written by a call that fails with CRASS_ERR_INVALID_ARG
    for (uint64_t r = 0; r < n_reads; r++) if (rec_pos[r] >= n_bytes) return CRASS_ERR_INVALID_ARG;
    for (uint64_t k = 0; k < n; k++) if (idx[k] < idx_base || idx[k] - idx_base >= n_reads) return CRASS_ERR_INVALID_ARG;
    off_out[0] = 0;
    if (n == 0) return CRASS_OK;
    // where record r's name ends: the position of the first isspace() byte behind the header character, or n_bytes
    auto name_end = [&](uint64_t r) { uint64_t e = rec_pos[r] + 1; while (e < n_bytes && !crass::fx_is_space(bytes[e])) e++; return e; };
    std::vector<uint64_t> bits, carry;
    try {
        bits.assign((n_reads + 63) / 64, 0); carry.assign((n_reads + crass::kFxCmTile - 1) / crass::kFxCmTile, 0);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    uint64_t last = 0;                                  // 1 + the last own-comment record so far
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t e = name_end(r);
        if (crass::fx_own_comment(e, n_bytes, e < n_bytes ? bytes[e] : 0)) { bits[r >> 6] |= 1ull << (r & 63); last = r + 1; }
        if ((r + 1) % crass::kFxCmTile == 0 || r + 1 == n_reads) carry[r / crass::kFxCmTile] = last;
    }
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t src = crass::fx_comment_handed_from(bits.data(), carry.data(), file_read_base, n_files, idx[k] - idx_base);
        const uint64_t at = off_out[k];
        uint64_t len = 0;
        if (src != crass::kFxNone) {
            const uint64_t a = name_end(src) + 1;       // (an own-comment record: its name ends in front of n_bytes)
            uint64_t b = a;
            while (b < n_bytes && !crass::fx_is_nl(bytes[b])) b++;
            len = b - a;
            if (at < cap_bytes) memcpy(out + at, bytes + a, (size_t)std::min(len, cap_bytes - at));      // (nothing at or beyond out + cap_bytes)
        }
        if (has_out) has_out[k] = src != crass::kFxNone ? 1 : 0;
        off_out[k + 1] = at + len;
    }
    return off_out[n] > cap_bytes ? CRASS_ERR_OVERFLOW : CRASS_OK;
}

} // extern "C"

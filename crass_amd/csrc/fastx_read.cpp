// fastx_read.cpp — the host reader of a WHOLE file: every record's text as the arrays of a crass_fastx, the first read of
// every name, and the table that finds a name again (crass_fastx_find).  The parser: fastx_parse.cpp.
#include "host_ingest_internal.h"

#include <memory>
#include <unistd.h>

using namespace crass;

// the eleven arrays of a crass_fastx of nrec records, a byte / an element more than asked for each; all of them or none
// (CRASS_ERR_OOM, *out empty again).  The four offset arrays start at 0.
int crass::fastx_alloc(crass_fastx *out, uint64_t nrec, uint64_t seq_b, uint64_t name_b, uint64_t com_b, uint64_t qual_b)
{
    auto alloc8 = [](uint64_t nb) { return (uint8_t *)malloc(nb + 1); };
    auto alloc64 = [](uint64_t ne) { return (uint64_t *)malloc((ne + 1) * 8); };
    out->n_reads = nrec;
    out->seq = alloc8(seq_b); out->seq_off = alloc64(nrec + 1); out->name = alloc8(name_b); out->name_off = alloc64(nrec + 1);
    out->comment = alloc8(com_b); out->comment_off = alloc64(nrec + 1); out->has_comment = alloc8(nrec);
    out->qual = alloc8(qual_b); out->qual_off = alloc64(nrec + 1); out->has_qual = alloc8(nrec);
    out->header_id = alloc64(nrec);
    if (!out->seq || !out->seq_off || !out->name || !out->name_off || !out->comment || !out->comment_off || !out->has_comment ||
        !out->qual || !out->qual_off || !out->has_qual || !out->header_id) { crass_free_fastx(out); return CRASS_ERR_OOM; }
    out->seq_off[0] = out->name_off[0] = out->comment_off[0] = out->qual_off[0] = 0;
    return CRASS_OK;
}

// ---- header_id: first read with the same name (readsFound is keyed by the header string) ----
static void header_ids(crass_fastx *out)
{
    const uint64_t nrec = out->n_reads;
    // one 64-bit word per slot: (32-bit hash tag | 1) << 32 | index of the first read with that name; a tag match
    // is confirmed by comparing the names, so two names never share a slot
    size_t cap = 1024;
    while (cap * 10 < nrec * 14) cap <<= 1;                  // load <= ~0.7
    std::unique_ptr<std::atomic<uint64_t>[]> tab(new std::atomic<uint64_t>[cap]);
    std::vector<uint64_t> slot_of(nrec);
    const unsigned ht = (unsigned)std::min<uint64_t>(hw_threads(), std::max<uint64_t>(1, nrec / 65536));
    parallel_ranges(cap, ht, [&](uint64_t a, uint64_t b2, unsigned) { for (uint64_t i = a; i < b2; i++) tab[i].store(0, std::memory_order_relaxed); });
    auto same_name = [&](uint64_t x, uint64_t y) {
        const uint64_t lx = out->name_off[x + 1] - out->name_off[x], ly = out->name_off[y + 1] - out->name_off[y];
        return lx == ly && memcmp(out->name + out->name_off[x], out->name + out->name_off[y], lx) == 0;
    };
    parallel_ranges(nrec, ht, [&](uint64_t a, uint64_t b2, unsigned) {
        for (uint64_t r = a; r < b2; r++) {
            const uint64_t h = name_hash(out->name + out->name_off[r], out->name_off[r + 1] - out->name_off[r]);
            const uint64_t tag = ((h >> 32) | 1ull) << 32;
            size_t i = (size_t)h & (cap - 1);
            for (;;) {
                uint64_t cur = tab[i].load(std::memory_order_acquire);
                if (cur == 0) {
                    if (tab[i].compare_exchange_strong(cur, tag | r, std::memory_order_acq_rel)) break;      // claimed
                }
                if ((cur & 0xFFFFFFFF00000000ull) == tag && same_name((uint64_t)(uint32_t)cur, r)) {
                    while ((uint32_t)cur > r && !tab[i].compare_exchange_weak(cur, tag | r, std::memory_order_acq_rel)) {}
                    break;
                }
                i = (i + 1) & (cap - 1);
            }
            slot_of[r] = i;
        }
    });
    parallel_ranges(nrec, ht, [&](uint64_t a, uint64_t b2, unsigned) {
        for (uint64_t r = a; r < b2; r++) out->header_id[r] = (uint32_t)tab[slot_of[r]].load(std::memory_order_relaxed);
    });
    // the table stays with the records: crass_fastx_find() resolves a header name without a second index
    out->name_index = (uint64_t *)malloc(cap * sizeof(uint64_t));
    out->name_index_cap = out->name_index ? cap : 0;
    if (out->name_index)
        parallel_ranges(cap, ht, [&](uint64_t a, uint64_t b2, unsigned) { for (uint64_t i = a; i < b2; i++) out->name_index[i] = tab[i].load(std::memory_order_relaxed); });
}

extern "C" {

int crass_read_fastx(const char *path, crass_fastx *out)
{
    if (!path || !out) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    const double tr0 = now_s();
    std::vector<uint8_t> data;
    InflatedBuf inflated;
    struct Mapping {                                     // plain text is parsed straight from the page cache
        void *p = nullptr; size_t n = 0;
        ~Mapping() { if (p && n) munmap(p, n); }
    } map;
    {
        FILE *f = fopen(path, "rb");
        if (!f) return CRASS_ERR_IO;
        unsigned char magic[2] = {0, 0};
        const size_t got2 = fread(magic, 1, 2, f);
        const bool gz = got2 == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        if (!gz) {
            fseek(f, 0, SEEK_END);
            const long sz = ftell(f);
            fseek(f, 0, SEEK_SET);
            if (sz < 0) { fclose(f); return CRASS_ERR_IO; }
            void *m = sz ? mmap(nullptr, (size_t)sz, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fileno(f), 0) : nullptr;
            if (sz && m != MAP_FAILED) { map.p = m; map.n = (size_t)sz; }
            else {                                       // (pipes, odd file systems): one read of the whole file
                data.resize((size_t)sz);
                if (sz && fread(data.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return CRASS_ERR_IO; }
            }
            fclose(f);
        } else if (inflate_with_libdeflate(path, inflated)) {
            fclose(f);
        } else {
            fclose(f);
            if (!inflate_with_zlib(path, data)) return CRASS_ERR_IO;
        }
    }
    const bool timing = getenv("CRASS_TIMING") != nullptr;
    const double tr1 = now_s();
    const size_t n = map.p ? map.n : inflated.p ? inflated.n : data.size();
    const uint8_t *d = map.p ? (const uint8_t *)map.p : inflated.p ? inflated.p : data.data();
    std::vector<FxChunk> ch;
    parse_pieces(d, n, ch);
    const double tr2 = now_s();
    // the pieces hold their own copies of everything: the file image goes before the record arrays are allocated
    // (peak host memory = pieces + record arrays, not file + pieces + record arrays)
    if (map.p && map.n) { munmap(map.p, map.n); map.p = nullptr; map.n = 0; }
    free(inflated.p); inflated.p = nullptr; inflated.n = 0;
    std::vector<uint8_t>().swap(data);
    // ---- assemble ----
    const size_t nc = ch.size();
    std::vector<uint64_t> rec0(nc + 1, 0), seq0(nc + 1, 0), name0(nc + 1, 0), com0(nc + 1, 0), qual0(nc + 1, 0);
    bool any_c = false, all_c = true, any_q = false, all_q = true;
    uint32_t max_len = 0;
    for (size_t k = 0; k < nc; k++) {
        rec0[k + 1] = rec0[k] + ch[k].n_rec(); seq0[k + 1] = seq0[k] + ch[k].seq.size(); name0[k + 1] = name0[k] + ch[k].name.size();
        com0[k + 1] = com0[k] + ch[k].comment.size(); qual0[k + 1] = qual0[k] + ch[k].qual.size();
        for (uint8_t v : ch[k].own_c) { any_c |= v != 0; all_c &= v != 0; }
        for (uint8_t v : ch[k].own_q) { any_q |= v != 0; all_q &= v != 0; }
        max_len = std::max(max_len, ch[k].max_len);
    }
    const uint64_t nrec = rec0[nc];
    // comments / qualities: every record its own, or none at all, is a plain concatenation; a mix follows the
    // reference's stale-buffer semantics (once allocated, comment.s / qual.s keep their old bytes and searchFile
    // passes them on, libcrispr.cpp:124-131) in one ordered pass
    const bool simple_c = !any_c || all_c, simple_q = !any_q || all_q;
    if (const int rc = fastx_alloc(out, nrec, seq0[nc], name0[nc], simple_c ? com0[nc] : 0, simple_q ? qual0[nc] : 0)) return rc;
    run_side_by_side(nc, [&](size_t k) {
        const FxChunk &c = ch[k];
        if (!c.seq.empty()) memcpy(out->seq + seq0[k], c.seq.data(), c.seq.size());
        if (!c.name.empty()) memcpy(out->name + name0[k], c.name.data(), c.name.size());
        if (simple_c && !c.comment.empty()) memcpy(out->comment + com0[k], c.comment.data(), c.comment.size());
        if (simple_q && !c.qual.empty()) memcpy(out->qual + qual0[k], c.qual.data(), c.qual.size());
        for (size_t i = 0; i < c.n_rec(); i++) {
            const uint64_t r = rec0[k] + i;
            out->seq_off[r + 1] = seq0[k] + c.seq_end[i];
            out->name_off[r + 1] = name0[k] + c.name_end[i];
            if (simple_c) { out->comment_off[r + 1] = com0[k] + c.comment_end[i]; out->has_comment[r] = any_c ? 1 : 0; }
            if (simple_q) { out->qual_off[r + 1] = qual0[k] + c.qual_end[i]; out->has_qual[r] = any_q ? 1 : 0; }
        }
    });
    for (int comment = 1; comment >= 0; comment--) {
        if (comment ? simple_c : simple_q) continue;
        std::vector<uint8_t> bytes;
        std::string stale;
        bool any = false;
        stale_walk(ch.data(), nc, nrec, comment != 0, any, stale, comment ? out->has_comment : out->has_qual, comment ? out->comment_off : out->qual_off, bytes);
        uint8_t *&dst = comment ? out->comment : out->qual;
        free(dst);
        dst = (uint8_t *)malloc(bytes.size() + 1);
        if (!dst) { crass_free_fastx(out); return CRASS_ERR_OOM; }
        if (!bytes.empty()) memcpy(dst, bytes.data(), bytes.size());
    }
    const int last_ret_of_stream = ch.back().last_ret;
    std::vector<FxChunk>().swap(ch);                    // (and the pieces before the header table is built)
    const double tr3 = now_s();
    header_ids(out);
    out->max_len = max_len;
    out->last_ret = last_ret_of_stream;
    if (timing)
        fprintf(stderr, "[crass_timing] fastx: %zu bytes, %zu pieces: read %.3f s, parse %.3f s, assemble %.3f s, header ids %.3f s\n", n, nc,
                tr1 - tr0, tr2 - tr1, tr3 - tr2, now_s() - tr3);
    return CRASS_OK;
}

void crass_free_fastx(crass_fastx *f)
{
    if (!f) return;
    free(f->seq); free(f->seq_off); free(f->name); free(f->name_off); free(f->comment); free(f->comment_off);
    free(f->has_comment); free(f->qual); free(f->qual_off); free(f->has_qual); free(f->header_id); free(f->name_index);
    memset(f, 0, sizeof(*f));
}

uint64_t crass_fastx_find(const crass_fastx *f, const char *name, uint64_t len)
{
    if (!f || !f->name_index || !f->name_index_cap) return UINT64_MAX;
    const uint64_t h = name_hash((const uint8_t *)name, (size_t)len);
    const uint64_t tag = ((h >> 32) | 1ull) << 32, cap = f->name_index_cap;
    for (uint64_t i = h & (cap - 1);; i = (i + 1) & (cap - 1)) {
        const uint64_t cur = f->name_index[i];
        if (cur == 0) return UINT64_MAX;
        if ((cur & 0xFFFFFFFF00000000ull) == tag) {
            const uint64_t r = (uint32_t)cur;
            if (f->name_off[r + 1] - f->name_off[r] == len && memcmp(f->name + f->name_off[r], name, (size_t)len) == 0) return r;
        }
    }
}

} // extern "C"

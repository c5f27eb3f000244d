// fastx_index.cpp — the host reader as an index over the inputs' text, the command line's default: built in steps (IndexBuild),
// its reads, the records that are handed on fetched from it, its text dropped.  The parser: fastx_parse.cpp.
#include "host_ingest_internal.h"

#include <memory>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace crass;

// ---- the same reader as an INDEX over the file image (plain-text inputs) ----
// What the device wants from an input is its reads as 2-bit words; what the hand-off wants is the TEXT of the ~1 % of reads that
// are handed on.  crass_read_fastx builds every record's text as arrays (3.6 bytes of host memory per byte of input while it
// assembles them, and a serial share — page faults of 1.6 GB of fresh arrays, the ordered header table — that is larger than the
// parallel parse).  The index keeps the file mapped and, per record, the position of its header character: the pieces are parsed
// by the same state machine, each piece packs its own records into the job's word array at once and drops its text, the header
// table compares names in the mapping itself, and crass_fastx_index_fetch parses the few records that are handed on, again with
// the same state machine, when they are asked for.  gzip'd inputs and files that mix records with and without a comment /
// quality line (kseq's stale-buffer semantics need the records in order) are left to the two readers above: CRASS_ERR_UNSUPPORTED.
struct __attribute__((visibility("hidden"))) crass_fastx_index {      // (as the types of host_ingest_internal.h it is made of)
    // the text: per input a mapped file or, for a gzip'd input, its inflated image.  A record's header position is kept as a position
    // in the inputs' concatenation (base = the bytes of the inputs before it)
    struct File {
        void *map = nullptr; size_t n = 0; uint8_t *own = nullptr;     // own: the inflated image (then map points at it)
        int fd = -1;                                                   // a plain file stays open: its mapping goes when the index is built, the
                                                                       // handed-on records are read from the file (crass_fastx_index_fetch)
        uint64_t base = 0;
        bool any_c = false, any_q = false;
        int last_ret = -1;
    };
    std::vector<File> files;
    const File &file_of(uint64_t pos) const
    {
        size_t f = files.size() - 1;
        while (f > 0 && files[f].base > pos) f--;
        return files[f];
    }
    const uint8_t *text(uint64_t pos) const { const File &f = file_of(pos); return (const uint8_t *)f.map + (pos - f.base); }
    RawBuf<uint64_t> hdr_pos;                          // [n]
    RawBuf<uint32_t> packed; RawBuf<uint64_t> word_off; RawBuf<uint32_t> lengths;
    PackedOwner pk;                                    // (the exception lists)
    RawBuf<uint64_t> header_id;                        // [n] or empty (all names unique)
    crass_reads reads{};
    uint32_t max_len = 0;
    int last_ret = -1;
    ~crass_fastx_index()
    {
        for (File &f : files) {
            if (f.own) { drop_pages(f.own, f.n); free(f.own); }
            else if (f.map && f.n) { drop_pages(f.map, f.n); munmap(f.map, f.n); }
            if (f.fd >= 0) close(f.fd);
        }
    }
};

namespace {
// The building of an index (crass_index_fastx_files), step by step; what one step hands to the next.  A non-zero return ends the
// building: the words' thread, once started, is waited for before anything it reads or writes goes.
struct IndexBuild {
    crass_fastx_index *ix;
    size_t n = 0;                                        // bytes of text, all inputs
    std::vector<FxChunk> ch;                             // the pieces of all inputs in (input, position) order
    std::vector<uint32_t> piece_file;
    std::vector<uint64_t> rec0, tight0;                  // the records / the tight words in front of piece k
    uint64_t nrec = 0;
    PackLayout lay;
    RawBuf<uint32_t> name_len;
    unsigned SH = 0, shard_shift = 0, low_shift = 0;     // the header table's shards
    std::vector<uint64_t> cnt;                           // [piece][shard]: records of the piece whose name hash starts with the shard's byte
    RawBuf<uint32_t> order, order_h;                     // (released behind the words' placement, with the pieces: not beside it)
    std::thread words_thread;
    double t_words = 0, th_ph[4] = {0, 0, 0, 0};
    explicit IndexBuild(crass_fastx_index *x) : ix(x) {}
    ~IndexBuild() { if (words_thread.joinable()) words_thread.join(); }
    int open_inputs(const char *const *paths, uint32_t n_paths);
    int parse_and_gate();
    int place_arrays();
    void place_words(size_t k);
    int header_ids(double t3);
    void release_pieces();
};

int IndexBuild::open_inputs(const char *const *paths, uint32_t n_paths)
{
    ix->files.resize(n_paths);
    // every input opened on its own thread: a gzip'd one is a single-threaded inflate (0.7 GB/s of text), and paired-end files are two
    std::vector<int> frc(n_paths, CRASS_OK);
    auto open_one = [&](uint32_t f) {
        crass_fastx_index::File &F = ix->files[f];
        const int fd = open(paths[f], O_RDONLY);
        if (fd < 0) { frc[f] = CRASS_ERR_IO; return; }
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); frc[f] = CRASS_ERR_UNSUPPORTED; return; }
        const size_t fn = (size_t)st.st_size;
        unsigned char magic[2] = {0, 0};
        const bool gz = fn >= 2 && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        if (gz) {
            // a gzip'd input: its inflated image takes the mapping's place (libdeflate, whole buffer; without the library the
            // whole-file reader's zlib path takes the input).  1 x the text + the packed reads instead of the whole-file reader's
            // ~3.6 x, and none of its assemble / pack passes
            // (only if the text — about four times the file — fits half of what this host has available: the bounded readers otherwise)
            const uint64_t avail = mem_available();
            close(fd);
            if (avail && (uint64_t)fn * 4 * n_paths > avail / 2) { frc[f] = CRASS_ERR_UNSUPPORTED; return; }
            InflatedBuf inflated;
            if (!inflate_with_libdeflate(paths[f], inflated)) { frc[f] = CRASS_ERR_UNSUPPORTED; return; }
            F.own = inflated.p; F.map = inflated.p; F.n = inflated.n;
            inflated.p = nullptr;
        } else {
            if (fn) {
                // (no MAP_POPULATE: one thread filling 2 M page-table entries was 0.25 s for 8 GB; the 64 piece parsers take the
                // faults of their own pieces)
                void *m = mmap(nullptr, fn, PROT_READ, MAP_PRIVATE, fd, 0);
                if (m == MAP_FAILED) { close(fd); frc[f] = CRASS_ERR_UNSUPPORTED; return; }
                (void)madvise(m, fn, MADV_WILLNEED);
                F.map = m; F.n = fn;
            }
            F.fd = fd;
        }
    };
    run_side_by_side(n_paths, open_one);
    for (uint32_t f = 0; f < n_paths; f++) if (frc[f] == CRASS_ERR_IO) return CRASS_ERR_IO;
    for (uint32_t f = 0; f < n_paths; f++) if (frc[f] != CRASS_OK) return frc[f];
    for (uint32_t f = 0; f < n_paths; f++) { ix->files[f].base = n; n += ix->files[f].n; }
    return CRASS_OK;
}

// every input parsed in pieces (pack mode: every record is packed as it is parsed, its text dropped); the pieces of all inputs in
// (input, position) order are the job's reads in (file, read) order.  Gated: the lengths, the stale comment / quality buffers
int IndexBuild::parse_and_gate()
{
    for (uint32_t f = 0; f < (uint32_t)ix->files.size(); f++) {
        crass_fastx_index::File &F = ix->files[f];
        std::vector<FxChunk> cf;
        parse_pieces((const uint8_t *)F.map, F.n, cf, 8u << 20, true);
        bool any_c = false, all_c = true, any_q = false, all_q = true;
        for (FxChunk &c : cf) {                         // (the pieces kept their own comment / quality flags)
            const uint8_t fl = c.pk_flags;
            if (c.n_rec()) { any_c |= (fl & 1) != 0; any_q |= (fl & 2) != 0; all_c &= (fl & 4) != 0; all_q &= (fl & 8) != 0; }
        }
        if ((any_c && !all_c) || (any_q && !all_q)) return CRASS_ERR_UNSUPPORTED;      // stale comment / quality buffers: ordered readers
        F.any_c = any_c; F.any_q = any_q; F.last_ret = cf.empty() ? -1 : cf.back().last_ret;
        for (FxChunk &c : cf) { ch.emplace_back(std::move(c)); piece_file.push_back(f); }
    }
    const size_t nc = ch.size();
    rec0.assign(nc + 1, 0); tight0.assign(nc + 1, 0);
    uint32_t max_len = 0, min_len = 0xFFFFFFFFu;
    for (size_t k = 0; k < nc; k++) {                    // (the pieces kept their own minimum length)
        rec0[k + 1] = rec0[k] + ch[k].n_rec(); tight0[k + 1] = tight0[k] + ch[k].words.size();
        max_len = std::max(max_len, ch[k].max_len); min_len = std::min(min_len, ch[k].pk_min_len);
    }
    if (max_len > CRASS_HIP_MAX_READ_LEN) return CRASS_ERR_UNSUPPORTED;
    nrec = rec0[nc];
    if (nrec == 0) min_len = 0;
    ix->max_len = max_len; ix->last_ret = ix->files.back().last_ret;
    // ---- layout: crass_pack_reads' rules (mode 2); the pieces' words are then copied into place ----
    pack_layout_core(nrec, max_len, min_len, tight0[nc], 2, &lay);
    return CRASS_OK;
}

// the per-record arrays first (the header table needs them), then the words — 2 GB for 50 M reads, most of this stage's time —
// on their own threads BESIDE the header table: both are bound by memory, neither by the other's data
int IndexBuild::place_arrays()
{
    const size_t nc = ch.size();
    const uint32_t stride = lay.stride_words;
    const bool uniform_len = lay.uniform_len != 0;
    PackedOwner &o = ix->pk;
    // shards of the header table (below): by the hash's top 12 bits — ~12 k names per shard for 50 M reads, a 256 KB table that
    // stays in the filling core's L2 (256 shards of 4 MB tables spent 0.12 s on L3 / memory latency; CRASS_HDR_SHARD_BITS: the A/B)
    unsigned shard_bits = nrec >= (1u << 22) ? 12 : 8;
    if (const char *e = getenv("CRASS_HDR_SHARD_BITS")) shard_bits = (unsigned)std::min(14, std::max(1, atoi(e)));
    SH = 1u << shard_bits; shard_shift = 64 - shard_bits; low_shift = shard_shift - 32;
    cnt.assign(nc * (size_t)SH, 0);
    const size_t n_words = (size_t)lay.total_words + 4;
    // (no zero fill: the pieces write every word they own, pad words included)
    if (!ix->packed.alloc(n_words) || (!stride && !ix->word_off.alloc(nrec + 1)) || (!uniform_len && !ix->lengths.alloc(nrec)) ||
        !ix->hdr_pos.alloc(nrec) || !name_len.alloc(nrec)) return CRASS_ERR_OOM;
    {
        run_side_by_side(nc, [&](size_t k) {
            FxChunk &c = ch[k];
            const size_t m = c.n_rec();
            if (m) {
                const uint64_t fb = ix->files[piece_file[k]].base;
                uint64_t *hp = ix->hdr_pos.data() + rec0[k];
                for (size_t i = 0; i < m; i++) hp[i] = fb + c.hdr_pos[i];
                uint64_t *cs = cnt.data() + k * SH;         // (the header table's counting pass: the hashes are read here anyway)
                const uint64_t *nhk = c.name_h.data();
                for (size_t i = 0; i < m; i++) cs[nhk[i] >> shard_shift]++;
            }
            uint64_t wat = 0;
            for (size_t i = 0; i < m; i++) {
                const uint64_t r = rec0[k] + i;
                const uint32_t L = c.len32[i];
                name_len[r] = c.nlen32[i];
                if (!uniform_len) ix->lengths[r] = L;
                if (!stride) ix->word_off[r] = tight0[k] + wat;
                wat += (L + 15) / 16;
            }
            // (the pieces' arrays go with the pieces, at the end: sixty-four threads unmapping at once, here, meet on the address
            // space's lock — 0.08 s; the name hashes are read once more, by the header table's scatter)
        });
        if (!stride) ix->word_off[nrec] = tight0[nc];
    }
    words_thread = std::thread([this, nc, n_words]() {
        const double tw0 = now_s();
        run_side_by_side(nc, [this](size_t k) { place_words(k); });
        for (size_t x = 0; x < 4; x++) ix->packed[n_words - 4 + x] = 0;
        t_words = now_s() - tw0;
    });
    o.exc_off.push_back(0);
    for (size_t k = 0; k < nc; k++) {
        const uint64_t base = o.exc_bytes.size();
        for (uint64_t e : ch[k].exc_rec) o.exc_read.push_back(rec0[k] + e);
        o.exc_bytes.insert(o.exc_bytes.end(), ch[k].exc_bytes.begin(), ch[k].exc_bytes.end());
        for (uint64_t e : ch[k].exc_off) o.exc_off.push_back(base + e);
    }
    return CRASS_OK;
}

// piece k's words into their place in the job's array
void IndexBuild::place_words(size_t k)
{
    const uint32_t stride = lay.stride_words;
    const bool uniform_len = lay.uniform_len != 0;
    uint32_t *packed = ix->packed.data();
    FxChunk &c = ch[k];
    if (uniform_len) { if (!c.words.empty()) memcpy(packed + rec0[k] * (uint64_t)stride, c.words.data(), c.words.size() * 4); }
    else if (!stride) { if (!c.words.empty()) memcpy(packed + tight0[k], c.words.data(), c.words.size() * 4); }
    else {                                           // padded to one stride
        uint64_t wat = 0;
        for (size_t i = 0; i < c.n_rec(); i++) {
            const uint32_t L = c.len32[i];
            const uint32_t nw = (L + 15) / 16;
            uint32_t *w = packed + (rec0[k] + i) * (uint64_t)stride;
            memcpy(w, c.words.data() + wat, (size_t)nw * 4);
            for (uint32_t x = nw; x < stride; x++) w[x] = 0;
            wat += nw;
        }
    }
}

// ---- header_id: first read with the same name, names compared in the mapping (exact) ----
// SHARDED by the hash's top byte: one table for 50 M names is 1 GB of random compare-and-swaps (0.7 s on the box's 16 CPUs);
// 256 shards of ~200 k names each fit a cache-resident table, are filled by ONE thread each — in read order, so the first
// occurrence is simply the first insert, no atomics — and are independent.  Records reach their shard by a stable counting
// sort of the record indices (two streaming passes over the hashes).  Runs beside the words' placement.
int IndexBuild::header_ids(double t3)
{
    const size_t nc = ch.size();
    for (double &t : th_ph) t = t3;
    if (nrec) {
        if (nrec >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;
        const unsigned ht = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<unsigned>(hw_threads(), 64u), nrec / 65536));
        // order_h: the hashes in shard order too — the 32 bits below the shard's — so that the shard's thread reads them in a stream
        // (looked up per record they were 50 M cache misses, most of this stage)
        if (!order.alloc(nrec) || !order_h.alloc(nrec)) return CRASS_ERR_OOM;
        th_ph[0] = now_s();
        // (counted per piece while the record arrays were placed, above: no pass of its own, and no job-wide copy of the hashes)
        th_ph[1] = now_s();
        std::vector<uint64_t> sh_begin(SH + 1, 0);
        {   // shard-major, piece-minor: a shard's records stay in read order
            uint64_t at = 0;
            for (unsigned sh = 0; sh < SH; sh++) {
                sh_begin[sh] = at;
                for (size_t k = 0; k < nc; k++) { const uint64_t c = cnt[k * SH + sh]; cnt[k * SH + sh] = at; at += c; }
            }
            sh_begin[SH] = at;
        }
        run_pulled(nc, (unsigned)std::min<size_t>(ht, nc), [&](size_t k, unsigned) {
            uint64_t *c = cnt.data() + k * SH;
            const uint64_t *nhk = ch[k].name_h.data();
            const size_t m = ch[k].n_rec();
            for (size_t i = 0; i < m; i++) { const uint64_t h = nhk[i], at = c[h >> shard_shift]++; order[at] = (uint32_t)(rec0[k] + i); order_h[at] = (uint32_t)(h >> low_shift); }
        });
        th_ph[2] = now_s();
        auto same_name = [&](uint64_t x, uint64_t y) {
            return name_len[x] == name_len[y] && memcmp(ix->text(ix->hdr_pos[x]) + 1, ix->text(ix->hdr_pos[y]) + 1, name_len[x]) == 0;
        };
        struct alignas(64) Worker {
            std::vector<uint64_t> tab;                    // (tag | record index + 1), 0 = empty
            std::vector<std::pair<uint32_t, uint32_t>> mine;          // (record, the first record of its name): the repeats only — a
                                                          // first[] entry written per record was 50 M scattered cache lines
        };
        std::vector<Worker> workers(ht);
        run_pulled(SH, ht, [&](size_t sh, unsigned t) {
            const uint64_t m = sh_begin[sh + 1] - sh_begin[sh];
            if (!m) return;
            std::vector<uint64_t> &tab = workers[t].tab;
            size_t cap = 1024;
            while (cap * 10 < m * 16) cap <<= 1;
            tab.assign(cap, 0);
            for (uint64_t q = sh_begin[sh]; q < sh_begin[sh + 1]; q++) {
                const uint64_t r = order[q];
                const uint64_t tag = (uint64_t)order_h[q] << 32;          // the 32 hash bits below the shard's
                size_t i = (size_t)order_h[q] & (cap - 1);
                for (;;) {
                    const uint64_t cur = tab[i];
                    if (cur == 0) { tab[i] = tag | (r + 1); break; }
                    if ((cur & 0xFFFFFFFF00000000ull) == tag && same_name((uint32_t)cur - 1u, r)) { workers[t].mine.emplace_back((uint32_t)r, (uint32_t)cur - 1u); break; }
                    i = (i + 1) & (cap - 1);
                }
            }
        });
        th_ph[3] = now_s();
        bool any_dup = false;
        for (const Worker &w : workers) any_dup |= !w.mine.empty();
        if (any_dup) {
            if (!ix->header_id.alloc(nrec)) return CRASS_ERR_OOM;
            parallel_ranges(nrec, ht, [&](uint64_t a2, uint64_t b2, unsigned) { for (uint64_t r = a2; r < b2; r++) ix->header_id[r] = r; });
            for (const Worker &w : workers) for (const auto &d : w.mine) ix->header_id[d.first] = d.second;
        }
    }
    return CRASS_OK;
}

void IndexBuild::release_pieces()
{
    order.release(); order_h.release();
    // (the pieces — 3.4 GB of per-record arrays and words for 50 M reads — are handed back here, over sixteen threads: their pages
    // dropped under the shared lock side by side, ~25 ms.  One thread doing it beside whatever the caller does next took 0.15 s and
    // the caller's host-to-device copy, which pins its source through the same address-space lock, waited for it)
    const size_t nc = ch.size();
    run_pulled(nc, (unsigned)std::min<size_t>(std::min<unsigned>(hw_threads(), 16u), nc), [&](size_t k, unsigned) {
        FxChunk &c = ch[k];
        c.words.drop(); c.hdr_pos.drop(); c.name_h.drop(); c.len32.drop(); c.nlen32.drop();
    });
    std::vector<FxChunk>().swap(ch);
}
} // namespace

extern "C" {

int crass_index_fastx(const char *path, crass_fastx_index **out) { return crass_index_fastx_files(&path, 1, out); }

int crass_index_fastx_files(const char *const *paths, uint32_t n_paths, crass_fastx_index **out)
{
    if (!paths || !n_paths || !out) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_paths; f++) if (!paths[f]) return CRASS_ERR_INVALID_ARG;
    *out = nullptr;
    const double t0 = now_s();
    std::unique_ptr<crass_fastx_index> ix(new (std::nothrow) crass_fastx_index());
    if (!ix) return CRASS_ERR_OOM;
    IndexBuild b(ix.get());
    if (const int rc = b.open_inputs(paths, n_paths)) return rc;
    const double t1 = now_s(), c1 = cpu_seconds();
    if (const int rc = b.parse_and_gate()) return rc;
    const double t2 = now_s(), c2 = cpu_seconds();
    if (const int rc = b.place_arrays()) return rc;      // (the words' thread runs from here on ...)
    const double t3 = now_s();
    if (const int rc = b.header_ids(t3)) return rc;
    const double t_hdr = now_s() - t3;
    b.words_thread.join();                               // (... to here: before the pieces go)
    const double t4 = now_s();
    const size_t nc = b.ch.size();
    b.release_pieces();
    fill_reads(ix->reads, b.nrec, b.lay, ix->packed.data(), ix->word_off.data(), ix->lengths.data(), ix->pk);
    ix->reads.header_id = ix->header_id.data();          // (NULL where no name was met twice)
    if (getenv("CRASS_TIMING"))
        fprintf(stderr, "[crass_timing] fastx index: %zu bytes, %zu pieces, %llu records: map %.3f s, parse + pack %.3f s (%.2f CPU s), record arrays %.3f s, header ids %.3f s (arrays %.3f, count %.3f, scatter %.3f, shards %.3f) beside the words' placement %.3f s: %.3f s, pieces freed %.3f s; %.2f CPU s behind the parse\n",
                b.n, nc, (unsigned long long)b.nrec, t1 - t0, t2 - t1, c2 - c1, t3 - t2, t_hdr, b.th_ph[0] - t3, b.th_ph[1] - b.th_ph[0], b.th_ph[2] - b.th_ph[1], b.th_ph[3] - b.th_ph[2], b.t_words, t4 - t3, now_s() - t4, cpu_seconds() - c2);
    *out = ix.release();
    return CRASS_OK;
}

int crass_fastx_index_reads(const crass_fastx_index *ix, crass_reads *reads, uint32_t *max_len, int *last_ret)
{
    if (!ix || !reads) return CRASS_ERR_INVALID_ARG;
    *reads = ix->reads;
    if (max_len) *max_len = ix->max_len;
    if (last_ret) *last_ret = ix->last_ret;
    return CRASS_OK;
}

// the records idx[0 .. n) (any order, repeats allowed) as a crass_fastx of n records in that order: parsed from the mapping by
// the reader's own state machine; header_id[k] = idx[k] (the caller knows the job-level ids)
int crass_fastx_index_fetch(const crass_fastx_index *ix, const uint64_t *idx, uint64_t n, crass_fastx *out)
{
    if (!ix || !out || (n && !idx)) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    const uint64_t nrec = ix->reads.n_reads;
    for (uint64_t k = 0; k < n; k++) if (idx[k] >= nrec) return CRASS_ERR_INVALID_ARG;
    const unsigned nt = (unsigned)std::min<uint64_t>(std::min<unsigned>(hw_threads(), 32u), std::max<uint64_t>(1, n / 2048));
    std::vector<FxChunk> parts(nt ? nt : 1);
    const uint64_t per = (n + parts.size() - 1) / parts.size();
    std::atomic<bool> io_fail{false};
    auto run = [&](size_t t) {
        const uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
        std::vector<uint8_t> rb;
        for (uint64_t k = a; k < b; k++) {
            const uint64_t h = ix->hdr_pos[idx[k]];
            const crass_fastx_index::File &F = ix->file_of(h);
            const size_t lh = (size_t)(h - F.base);
            if (F.map) { parse_range((const uint8_t *)F.map, F.n, lh, lh + 1, false, parts[t]); continue; }      // exactly the record whose header character is at h
            // (the mapping is gone: the record's bytes — from its header character to the next record's, or to the file's end — from the file)
            uint64_t e = F.base + F.n;
            if (idx[k] + 1 < nrec && ix->hdr_pos[idx[k] + 1] < e) e = ix->hdr_pos[idx[k] + 1];
            const size_t len = (size_t)(e - h);
            rb.resize(len);
            size_t got = 0;
            while (got < len) { const ssize_t g = pread(F.fd, rb.data() + got, len - got, (off_t)(lh + got)); if (g <= 0) break; got += (size_t)g; }
            if (got != len) { io_fail.store(true); return; }
            parse_range(rb.data(), len, 0, 1, false, parts[t]);
        }
    };
    run_side_by_side(parts.size(), run);
    if (io_fail.load()) return CRASS_ERR_IO;
    uint64_t got = 0, seq_b = 0, name_b = 0, com_b = 0, qual_b = 0;
    for (auto &c : parts) { got += c.n_rec(); seq_b += c.seq.size(); name_b += c.name.size(); com_b += c.comment.size(); qual_b += c.qual.size(); }
    if (got != n) return CRASS_ERR_STATE;
    if (const int rc = fastx_alloc(out, n, seq_b, name_b, com_b, qual_b)) return rc;
    uint64_t r = 0, sq = 0, nm = 0, cm = 0, ql = 0;
    uint32_t max_len = 0;
    for (auto &c : parts) {
        if (!c.seq.empty()) memcpy(out->seq + sq, c.seq.data(), c.seq.size());
        if (!c.name.empty()) memcpy(out->name + nm, c.name.data(), c.name.size());
        if (!c.comment.empty()) memcpy(out->comment + cm, c.comment.data(), c.comment.size());
        if (!c.qual.empty()) memcpy(out->qual + ql, c.qual.data(), c.qual.size());
        for (size_t i = 0; i < c.n_rec(); i++, r++) {
            out->seq_off[r + 1] = sq + c.seq_end[i]; out->name_off[r + 1] = nm + c.name_end[i];
            out->comment_off[r + 1] = cm + c.comment_end[i]; out->qual_off[r + 1] = ql + c.qual_end[i];
            { const crass_fastx_index::File &F = ix->file_of(ix->hdr_pos[idx[r]]); out->has_comment[r] = F.any_c ? 1 : 0; out->has_qual[r] = F.any_q ? 1 : 0; }
            out->header_id[r] = idx[r];
        }
        sq += c.seq.size(); nm += c.name.size(); cm += c.comment.size(); ql += c.qual.size();
        max_len = std::max(max_len, c.max_len);
    }
    out->max_len = max_len;
    out->last_ret = ix->last_ret;
    return CRASS_OK;
}

void crass_fastx_index_free(crass_fastx_index *ix) { delete ix; }

// A plain file's mapping has done most of its work once the hand-off has fetched its records: 2 M page-table entries for 8 GB, taken
// down side by side (the pages dropped under the shared lock by sixteen threads, then an unmapping that finds nothing) instead of by
// one thread beside a later stage, whose allocations waited for it a quarter of a second.  Records fetched after this are read from
// the file (pread: four times slower per record, which is why the hand-off fetches first).
void crass_fastx_index_drop_text(crass_fastx_index *ix)
{
    if (!ix) return;
    for (crass_fastx_index::File &F : ix->files) {
        if (F.own || !F.map || !F.n || F.fd < 0) continue;
        // (not drop_pages: it keeps a last page that is not whole — the mapping's last page goes here — and runs ns / 2 threads where
        // this site runs ns, up to sixteen: a file of 64 MB to 2 GB would be dropped by half as many)
        const size_t slice = 64u << 20, ns = (F.n + slice - 1) / slice;
        uint8_t *mp = (uint8_t *)F.map;
        const size_t fn = F.n;
        run_pulled(ns, (unsigned)std::min<size_t>(std::min<unsigned>(hw_threads(), 16u), ns),
                   [&](size_t q, unsigned) { (void)madvise(mp + q * slice, std::min<size_t>(slice, fn - q * slice), MADV_DONTNEED); });
        munmap(F.map, F.n);
        F.map = nullptr;
    }
}

} // extern "C"

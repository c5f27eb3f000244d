// host_ingest_internal.h — what crosses the files of the host reader, each declared once: ingest.cpp (the 2-bit packer),
// fastx_parse.cpp (the kseq-exact record parser), host_inflate.cpp (gzip / BGZF of a whole file), fastx_read.cpp (the whole
// file), fastx_index.cpp (the index), fastx_stream.cpp (the stream, the job's name table) and synth.cpp (the synthetic
// metagenome).  Host-only C++17 that any compiler builds (tools/sanitize): no .hip file includes this.
#pragma once
#include "../../include/crass_hip.h"
#include "pack_text.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include <sys/mman.h>
#include <sys/resource.h>

namespace crass { bool parallel_gunzip(const uint8_t *in, size_t n, uint8_t **out_p, size_t *out_n, unsigned threads); }      // pgzip.cpp
#pragma GCC visibility push(hidden)
namespace crass {

struct PackedOwner {
    std::vector<uint32_t> packed;
    std::vector<uint64_t> word_off;
    std::vector<uint32_t> lengths;
    std::vector<uint64_t> exc_read, exc_off;
    std::vector<uint8_t> exc_bytes;
    std::vector<uint64_t> header_id;                   // (crass_hip_get_packed only)
};

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

inline unsigned hw_threads()
{
    unsigned n = std::thread::hardware_concurrency();
    // (not limited to a cgroup CPU quota: the ingest is one short burst, and 64 threads for 70 ms beat 16 for 160 ms on
    // the GPU box even though the quota there is 16 CPUs — the host pool, which polls for as long as a search runs, does
    // follow the quota: merge.cpp)
    return n ? n : 1;
}

template <typename F> void parallel_ranges(uint64_t n, unsigned nt, F f)
{
    if (nt <= 1 || n < 4096) { f(0, n, 0u); return; }
    std::vector<std::thread> th;
    uint64_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
        if (a >= b) break;
        th.emplace_back([=]() { f(a, b, t); });
    }
    for (auto &x : th) x.join();
}

// f(0) .. f(n - 1) side by side: f(1) .. f(n - 1) on threads of their own, f(0) on the caller's, all joined
template <typename F> void run_side_by_side(size_t n, F &&f)
{
    std::vector<std::thread> th;
    for (size_t k = 1; k < n; k++) th.emplace_back([&f, k]() { f(k); });
    if (n) f(0);
    for (auto &x : th) x.join();
}

// f(k, t) for every k in [0, n), pulled from one counter by workers t = 0 .. nt - 1 (the caller is worker 0; nt <= 1: the caller alone)
template <typename F> void run_pulled(size_t n, unsigned nt, F &&f)
{
    std::atomic<size_t> next{0};
    run_side_by_side(std::max(1u, nt), [&](size_t t) { for (;;) { const size_t k = next.fetch_add(1, std::memory_order_relaxed); if (k >= n) break; f(k, (unsigned)t); } });
}

// CPU seconds of the process so far (user + system): under a cgroup CPU quota a stage's wall time is its CPU seconds over the quota
inline double cpu_seconds()
{
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    return ru.ru_utime.tv_sec + 1e-6 * ru.ru_utime.tv_usec + ru.ru_stime.tv_sec + 1e-6 * ru.ru_stime.tv_usec;
}

// A large array that is written in full by many threads right after it is allocated: no value-initialisation (a std::vector's
// resize() zero-fills — 2 GB of packed reads on ONE thread before the 64 that fill them start), 2 MB alignment and
// MADV_HUGEPAGE where the kernel takes the hint (a first touch per 2 MB instead of per 4 KB: the page faults of the 3.4 GB of
// arrays an index of 50 M reads allocates were most of its "words into place" second).
// Giving gigabytes back: one munmap of 8 GB holds the address space's lock for a quarter of a second, and every other thread of
// the process that touches a fresh page (the next stage's buffers) waits for it.  MADV_DONTNEED drops the pages under the SHARED
// lock, slice by slice; the unmapping that follows finds nothing left to do.
// Gigabytes at once go side by side: the kernel hands pages back (and clears them) at ~13 GB/s per thread in 4 KB pages, 27 GB/s in
// 2 MB pages — 6 GB were 0.46 s on one thread, 0.11 s on sixteen (profiles/r06_exit_cost.txt); more threads than that meet on the
// zone locks and are slower again.
inline void drop_pages(void *p, size_t bytes)
{
    const size_t page = 4096, slice = 64u << 20;
    const uintptr_t a0 = ((uintptr_t)p + page - 1) & ~(uintptr_t)(page - 1), e = ((uintptr_t)p + bytes) & ~(uintptr_t)(page - 1);
    if (e <= a0) return;
    const size_t ns = (e - a0 + slice - 1) / slice;
    const unsigned nt = (unsigned)std::min<size_t>(std::min<unsigned>(hw_threads(), 16u), ns / 2);
    run_pulled(ns, nt, [&](size_t q, unsigned) { const uintptr_t a = a0 + q * slice; (void)madvise((void *)a, std::min<size_t>(slice, e - a), MADV_DONTNEED); });
}

// an array that is asked for again and again with about the same size: grown, never shrunk, not initialised
template <typename T> struct KeepBuf {
    T *p = nullptr; size_t cap = 0;
    KeepBuf() = default;
    KeepBuf(const KeepBuf &) = delete;
    KeepBuf &operator=(const KeepBuf &) = delete;
    ~KeepBuf() { free(p); }
    T *ensure(size_t n) { if (n > cap) { free(p); cap = n + n / 8 + 64; p = (T *)malloc(cap * sizeof(T)); if (!p) cap = 0; } return p; }
};

template <typename T> struct RawBuf {
    T *p = nullptr; size_t n = 0;
    RawBuf() = default;
    RawBuf(const RawBuf &) = delete;
    RawBuf &operator=(const RawBuf &) = delete;
    void release() { if (p && n * sizeof(T) >= (8u << 20)) drop_pages(p, n * sizeof(T)); free(p); p = nullptr; n = 0; }
    ~RawBuf() { release(); }
    bool alloc(size_t count)
    {
        release();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        if (bytes >= (8u << 20)) {
            const size_t al = 2u << 20, rounded = (bytes + al - 1) / al * al;
            void *q = aligned_alloc(al, rounded);
            if (!q) return false;
            (void)madvise(q, rounded, MADV_HUGEPAGE);
            p = (T *)q;
        } else {
            p = (T *)malloc(bytes);
            if (!p) return false;
        }
        n = count;
        return true;
    }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

// A per-record array a parser appends to without knowing its final size (a piece of an input: ~10^6 records).  A std::vector doubles
// by allocate + copy + free: every doubling touches fresh pages, and what it frees stays in its thread's malloc arena (glibc's
// mmap threshold moves up to 32 MB with the first large free) — 64 parsers left 1.8 GB of such arenas behind, resident until the
// process's end.  This one is a mapping of its own from 1 MB on: grown by mremap (page tables move, no byte is copied or touched
// again), MADV_HUGEPAGE, handed back to the kernel the moment it is released; no value-initialisation.
template <typename T> struct GrowBuf {
    T *p = nullptr; size_t n = 0, cap = 0;
    bool mapped = false;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &o) { assign(o); }
    GrowBuf &operator=(const GrowBuf &o) { if (this != &o) { n = 0; assign(o); } return *this; }
    GrowBuf(GrowBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap), mapped(o.mapped) { o.p = nullptr; o.n = o.cap = 0; o.mapped = false; }
    GrowBuf &operator=(GrowBuf &&o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; cap = o.cap; mapped = o.mapped; o.p = nullptr; o.n = o.cap = 0; o.mapped = false; } return *this; }
    ~GrowBuf() { release(); }
    void release()
    {
        if (p) { if (mapped) munmap(p, cap * sizeof(T)); else free(p); }
        p = nullptr; n = cap = 0; mapped = false;
    }
    // the pages go back under the address space's SHARED lock (several threads side by side); release() then unmaps nothing but
    // page tables
    void drop() { if (p && mapped) (void)madvise(p, cap * sizeof(T), MADV_DONTNEED); release(); }
    void assign(const GrowBuf &o) { resize(o.n); if (o.n) memcpy(p, o.p, o.n * sizeof(T)); }
    void grow(size_t want)
    {
        static const size_t kMap = 1u << 20, kHuge = 2u << 20;
        size_t bytes = std::max<size_t>(std::max(want, cap * 2) * sizeof(T), 4096);
        if (bytes < kMap) {
            T *q = (T *)realloc(p, bytes);
            if (!q) throw std::bad_alloc();
            p = q; cap = bytes / sizeof(T);
            return;
        }
        bytes = (bytes + kHuge - 1) / kHuge * kHuge;
        void *q;
        if (mapped) q = mremap(p, cap * sizeof(T), bytes, MREMAP_MAYMOVE);
        else q = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (q == MAP_FAILED) throw std::bad_alloc();
        (void)madvise(q, bytes, MADV_HUGEPAGE);
        if (!mapped) { if (n) memcpy(q, p, n * sizeof(T)); free(p); mapped = true; }
        p = (T *)q; cap = bytes / sizeof(T);
    }
    void push_back(const T &v) { if (n == cap) grow(n + 1); p[n++] = v; }
    void resize(size_t m) { if (m > cap) grow(m); n = m; }           // (new elements are NOT initialised)
    void clear() { n = 0; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

struct FxChunk {
    std::vector<uint8_t> seq, name, comment, qual;                      // concatenated fields of the records parsed here
    std::vector<uint64_t> seq_end, name_end, comment_end, qual_end;     // local end offsets per record
    std::vector<uint8_t> own_c, own_q;                                  // the record carried its own comment / quality
    uint32_t max_len = 0;
    size_t next_start = 0;     // index of the header char of the first record NOT parsed here
    size_t last_hdr = 0;       // index of the header char of the LAST record parsed here (streaming: a chunk's last record is re-read)
    GrowBuf<uint64_t> hdr_pos;                                          // index of every record's header char (crass_index_fastx)
    // pack mode (crass_index_fastx): a record's sequence is 2-bit packed the moment it is complete — while its bytes are still in
    // the cache — and its text dropped; seq / name / comment / qual stay empty, seq_end / name_end count virtual bytes (the
    // lengths), the name is kept as a hash
    bool pack = false;
    GrowBuf<uint32_t> words;                                            // the records' words, tightly packed (ceil(L/16) each)
    GrowBuf<uint64_t> name_h;                                           // name_hash() of every record's name
    // (pack mode keeps 24 bytes per record beside its words — header position, name hash, the two lengths — and the comment /
    // quality flags per piece: the eight per-record vectors of the other mode were 50 bytes, 2.5 GB for 50 M reads, written by the
    // parsers and freed again — 0.4 s on one thread — before the reads had even been looked at)
    GrowBuf<uint32_t> len32, nlen32;                                    // sequence / name length of every record
    uint8_t pk_flags = 12;                                              // bit 0 any comment, 1 any quality, 2 all comment, 3 all quality
    uint32_t pk_min_len = 0xFFFFFFFFu;
    std::vector<uint64_t> exc_rec, exc_off;                             // local indices of reads with a byte outside ACGT, ends in exc_bytes
    std::vector<uint8_t> exc_bytes;
    uint64_t v_seq = 0, v_name = 0;
    bool ended = false;        // kseq_read returned < 0 inside this range
    int last_ret = -1;         // ... with this value
    size_t n_rec() const { return pack ? len32.size() : seq_end.size(); }
    // as new, with the vectors' memory kept (a stream parses chunk after chunk into the same pieces: 64 MB of vectors allocated and
    // given back per chunk were most of a chunk's time outside its parse)
    void reset(bool pk)
    {
        seq.clear(); name.clear(); comment.clear(); qual.clear(); seq_end.clear(); name_end.clear(); comment_end.clear(); qual_end.clear();
        own_c.clear(); own_q.clear(); hdr_pos.clear(); words.clear(); name_h.clear(); len32.clear(); nlen32.clear();
        exc_rec.clear(); exc_off.clear(); exc_bytes.clear();
        max_len = 0; next_start = 0; last_hdr = 0; pack = pk; pk_flags = 12; pk_min_len = 0xFFFFFFFFu; v_seq = 0; v_name = 0; ended = false; last_ret = -1;
    }
};

// byte -> 2-bit code, 0x80 for anything outside ACGT: the one table of crass_pack_reads and the parser's pack_bases
inline const uint8_t *base_lut()
{
    static const struct Lut { uint8_t t[256]; Lut() { memset(t, 0x80, sizeof(t)); t['A'] = 0; t['C'] = 1; t['G'] = 2; t['T'] = 3; } } lut;
    return lut.t;
}
// ingest.cpp: the crass_reads of a layout over arrays that are laid out by it (header_id NULL, read_index_base 0)
void fill_reads(crass_reads &r, uint64_t n, const PackLayout &lay, const uint32_t *packed, const uint64_t *word_off, const uint32_t *lengths, const PackedOwner &exc);

// fastx_parse.cpp
uint64_t name_hash(const uint8_t *p, size_t n);
void parse_range(const uint8_t *data, size_t n, size_t start, size_t limit, bool scan_first, FxChunk &o);
void parse_pieces(const uint8_t *d, size_t n, std::vector<FxChunk> &ch, size_t piece_bytes = 8u << 20, bool pack = false);
void stale_walk(const FxChunk *ch, size_t n_pieces, uint64_t n_rec, bool comment, bool &any, std::string &stale, uint8_t *has, uint64_t *off, std::vector<uint8_t> &bytes);

// host_inflate.cpp
struct InflatedBuf {
    uint8_t *p = nullptr; size_t n = 0;
    ~InflatedBuf() { free(p); }
};
uint64_t mem_available();
bool inflate_with_libdeflate(const char *path, InflatedBuf &out);
bool inflate_with_zlib(const char *path, std::vector<uint8_t> &data);

// fastx_read.cpp
int fastx_alloc(crass_fastx *out, uint64_t nrec, uint64_t seq_b, uint64_t name_b, uint64_t com_b, uint64_t qual_b);

} // namespace crass
#pragma GCC visibility pop

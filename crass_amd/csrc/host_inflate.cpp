// host_inflate.cpp — a gzip'd input of the host readers as its whole text: BGZF members side by side, one large member on
// several threads (pgzip.cpp), libdeflate member by member, zlib; and what this host has available for it.
#include "host_ingest_internal.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

using namespace crass;

// MemAvailable of /proc/meminfo in bytes; 0: not known
uint64_t crass::mem_available()
{
    uint64_t avail = 0;
    if (FILE *fp = fopen("/proc/meminfo", "r")) {
        char line[256];
        while (fgets(line, sizeof(line), fp)) if (!strncmp(line, "MemAvailable:", 13)) { avail = (uint64_t)atoll(line + 13) << 10; break; }
        fclose(fp);
    }
    return avail;
}

// Whole-buffer gzip inflate through libdeflate when the runtime library is present (no header in the image: the four
// entry points are bound by hand): about 3x zlib's streaming inflate, which is what bounds a .gz input end to end.
// Members are decompressed one after the other like gzread does (SeqUtils.cpp:100-126 opens every input through
// gzopen).  Any surprise — no library, damaged data, trailing garbage — returns false and the zlib path below decides.
// BGZF (bgzip; Illumina's bcl2fastq / BCL Convert write their .fastq.gz this way): a series of gzip members of at most 64 KB, each
// announcing its own compressed size in an extra field ('B' 'C', RFC 1952 2.3.1.1) and its text size in its last four bytes — the
// members' places in the input AND in the output are known without inflating anything, so they can be inflated side by side (a
// plain gzip stream is one member: 0.7 GB/s of text on one thread, which is what bounds a .gz input end to end).
// ioff / ooff: member b is in[ioff[b], ioff[b+1]) and inflates to out[ooff[b], ooff[b+1]).  false: not (entirely) BGZF.
static bool bgzf_walk(const uint8_t *in, size_t csz, std::vector<uint64_t> &ioff, std::vector<uint64_t> &ooff)
{
    size_t p = 0;
    uint64_t o = 0;
    while (p < csz) {
        if (csz - p < 28) return false;                   // 12 + 6 header bytes, at least 2 of deflate data, 8 of trailer
        if (in[p] != 0x1f || in[p + 1] != 0x8b || in[p + 2] != 8 || !(in[p + 3] & 4)) return false;
        const size_t xlen = (size_t)in[p + 10] | ((size_t)in[p + 11] << 8);
        if (p + 12 + xlen > csz) return false;
        size_t total = 0;
        for (size_t q = p + 12; q + 4 <= p + 12 + xlen;) {
            const size_t slen = (size_t)in[q + 2] | ((size_t)in[q + 3] << 8);
            if (in[q] == 'B' && in[q + 1] == 'C' && slen == 2 && q + 6 <= p + 12 + xlen) total = ((size_t)in[q + 4] | ((size_t)in[q + 5] << 8)) + 1;
            q += 4 + slen;
        }
        if (total < 12 + xlen + 10 || p + total > csz) return false;
        uint32_t isz;
        memcpy(&isz, in + p + total - 4, 4);
        if (isz > 65536u) return false;
        ioff.push_back(p); ooff.push_back(o);
        p += total; o += isz;
    }
    ioff.push_back(p); ooff.push_back(o);
    return ioff.size() > 1;
}

bool crass::inflate_with_libdeflate(const char *path, InflatedBuf &out)
{
    typedef void *(*alloc_fn)(void);
    typedef int (*gz_fn)(void *, const void *, size_t, void *, size_t, size_t *, size_t *);
    typedef void (*free_fn)(void *);
    static void *lib = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!lib || getenv("CRASS_NO_LIBDEFLATE")) return false;
    static const alloc_fn d_alloc = (alloc_fn)dlsym(lib, "libdeflate_alloc_decompressor");
    static const gz_fn d_gzip = (gz_fn)dlsym(lib, "libdeflate_gzip_decompress_ex");
    static const free_fn d_free = (free_fn)dlsym(lib, "libdeflate_free_decompressor");
    if (!d_alloc || !d_gzip || !d_free) return false;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 18) { close(fd); return false; }
    const size_t csz = (size_t)st.st_size;
    void *m = mmap(nullptr, csz, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return false;
    const uint8_t *in = (const uint8_t *)m;
    {
        std::vector<uint64_t> ioff, ooff;
        if (!getenv("CRASS_NO_BGZF") && bgzf_walk(in, csz, ioff, ooff) && ioff.size() > 64) {
            const size_t nb = ioff.size() - 1;
            // (2 MB-aligned, MADV_HUGEPAGE: a gigabyte of first touches in 4 KB pages is a good part of what is left)
            const size_t al = 2u << 20, bytes = ((size_t)ooff[nb] + 1 + al - 1) / al * al;
            uint8_t *buf = (uint8_t *)aligned_alloc(al, bytes);
            if (buf) (void)madvise(buf, bytes, MADV_HUGEPAGE);
            std::atomic<int> bad{buf ? 0 : 1};
            if (buf) {
                const unsigned nt = (unsigned)std::min<size_t>(std::min<unsigned>(hw_threads(), 32u), nb / 32);
                auto run = [&](unsigned t) {
                    void *dec = d_alloc();
                    if (!dec) { bad.store(1); return; }
                    for (size_t b = nb * t / nt; b < nb * (t + 1) / nt && !bad.load(std::memory_order_relaxed); b++) {
                        size_t ain = 0, aout = 0;
                        const size_t want = (size_t)(ooff[b + 1] - ooff[b]);
                        const int res = d_gzip(dec, in + ioff[b], (size_t)(ioff[b + 1] - ioff[b]), buf + ooff[b], want, &ain, &aout);
                        if (res != 0 || aout != want) bad.store(1);
                    }
                    d_free(dec);
                };
                run_side_by_side(nt, run);                // (more than 64 members: nt >= 2)
            }
            if (!bad.load()) {
                if (getenv("CRASS_TIMING")) fprintf(stderr, "[crass_timing] inflate: BGZF, %zu members (%zu -> %llu bytes) side by side\n", nb, csz, (unsigned long long)ooff[nb]);
                munmap(m, csz); out.p = buf; out.n = (size_t)ooff[nb]; return true;
            }
            free(buf);                                    // (a member that is not what its header says: the serial path decides)
        }
    }
    bool pg_fits = true;
    {
        // (its symbols are two bytes per byte of text, held beside the text: only where three times the text — about four times the
        // file each — fits half of the available memory)
        const uint64_t avail = mem_available();
        // (the text: the trailer's ISIZE where it can be believed — a single member below 4 GB of text —, else eight times the file:
        // FASTA and quality-binned FASTQ compress 6-8 x, and a guess of four let the several-thread inflate start on hosts where
        // three times the real text did not fit)
        uint32_t isz = 0;
        memcpy(&isz, in + csz - 4, 4);
        const uint64_t text = (csz < (1ull << 29) && (uint64_t)isz >= csz) ? (uint64_t)isz : (uint64_t)csz * 8;
        if (avail && text * 3 > avail / 2) pg_fits = false;
    }
    if (pg_fits && !getenv("CRASS_NO_PGZIP")) {
        // one member, large: inflated by several threads from block starts found in the middle of the stream (pgzip.cpp); its own
        // checks (length, CRC-32) decide, and anything it does not take comes back here
        uint8_t *pb = nullptr; size_t pn = 0;
        const double tp0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        if (crass::parallel_gunzip(in, csz, &pb, &pn, std::min<unsigned>(hw_threads(), 16u))) {
            if (getenv("CRASS_TIMING")) fprintf(stderr, "[crass_timing] inflate: one member, %zu -> %zu bytes on several threads, %.3f s\n", csz, pn,
                                                std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - tp0);
            munmap(m, csz);
            out.p = pb; out.n = pn;
            return true;
        }
    }
    uint32_t isize;                                       // size of the last member modulo 2^32: a first guess only
    memcpy(&isize, in + csz - 4, 4);
    size_t cap = std::max<size_t>((size_t)isize, csz * 3) + (1u << 20);
    uint8_t *buf = (uint8_t *)malloc(cap);
    // the output's pages are touched by other threads AHEAD of the one thread that inflates: first touches of a gigabyte (the kernel
    // clears every page) were a good part of the inflate's time on that thread
    std::atomic<bool> stop_touch{false};
    std::vector<std::thread> touchers;
    if (buf && cap >= (64u << 20) && !getenv("CRASS_NO_PREFAULT")) {
        const unsigned nt = std::min<unsigned>(std::max(1u, hw_threads() / 2), 8u);
        const size_t page = 4096;
        uint8_t *const base = (uint8_t *)(((uintptr_t)buf + page - 1) / page * page);
        const size_t span = (size_t)((buf + cap) - base) / page * page;
        for (unsigned t = 0; t < nt; t++)
            touchers.emplace_back([&, t, nt, base, span] {
                // (interleaved 64 MB stripes, in output order: whoever is ahead of the inflater is useful)
                // MADV_POPULATE_WRITE (Linux 5.14): the pages are made present and writable, their content is not touched — a page the
                // inflater got to first keeps what it wrote
                const size_t stripe = 16u << 20;
                for (size_t s0 = (size_t)t * stripe; s0 < span && !stop_touch.load(std::memory_order_relaxed); s0 += (size_t)nt * stripe)
                    if (madvise(base + s0, std::min(stripe, span - s0), 23 /* MADV_POPULATE_WRITE */) != 0) break;
            });
    }
    struct JoinTouch { std::atomic<bool> &stop; std::vector<std::thread> &th; ~JoinTouch() { stop.store(true); for (auto &x : th) x.join(); } } join_touch{stop_touch, touchers};
    void *dec = d_alloc();
    bool ok = buf && dec;
    size_t ipos = 0, opos = 0;
    while (ok && ipos < csz) {
        size_t ain = 0, aout = 0;
        const int res = d_gzip(dec, in + ipos, csz - ipos, buf + opos, cap - opos, &ain, &aout);
        if (res == 3) {                                   // LIBDEFLATE_INSUFFICIENT_SPACE: grow and repeat this member
            const size_t ncap = cap * 2;
            stop_touch.store(true);
            for (auto &x : touchers) x.join();
            touchers.clear();
            uint8_t *nb = (uint8_t *)realloc(buf, ncap);
            if (!nb) { ok = false; break; }
            buf = nb; cap = ncap;
            continue;
        }
        if (res != 0 || ain == 0) { ok = false; break; }
        ipos += ain; opos += aout;
    }
    if (dec) d_free(dec);
    munmap(m, csz);
    if (!ok) { free(buf); return false; }
    out.p = buf; out.n = opos;
    return true;
}

// ... and through zlib, as the reference reads every input (gzread); false: the file cannot be opened or its data is damaged
bool crass::inflate_with_zlib(const char *path, std::vector<uint8_t> &data)
{
    gzFile fp = gzopen(path, "r");
    if (!fp) return false;
    gzbuffer(fp, 1 << 20);
    std::vector<uint8_t> buf(4 << 20);
    int got;
    while ((got = gzread(fp, buf.data(), (unsigned)buf.size())) > 0) data.insert(data.end(), buf.begin(), buf.begin() + got);
    gzclose(fp);
    return got >= 0;
}

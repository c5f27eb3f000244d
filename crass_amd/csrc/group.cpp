// group.cpp — several GPUs from ONE process: crass_hip_group_* of include/crass_hip.h.
//
// A group is N contexts (engine.cpp and its engine_*.cpp stage files), one per device, driven by N host threads (the caller is rank 0's thread).  The
// path shards by contiguous read ranges; the only exchange is ONE all-gather per step of every rank's distinct
// candidate DR strings between pass 1 and the merge, issued by rank 0's thread for all ranks inside
// ncclGroupStart / ncclGroupEnd on the contexts' own streams — the canonical single-process form of RCCL
// (communicators from ncclCommInitAll).  RCCL is bound at run time (dlopen of librccl.so.1: the library stays loadable
// where RCCL is absent, and a process that already holds an RCCL — torch's — shares it); a failed RCCL call is
// reported as CRASS_ERR_RCCL with its error string, never retried by other means.
// Everything here goes through the public C ABI of the contexts — but for a files load (crass_hip_group_load_fastx_files), whose
// three steps per rank are fastx_shards.h's —; nothing computes a search result.
#include "../../include/crass_hip.h"

#include <hip/hip_runtime.h>
#include "devmem.h"
#include "fastx_shards.h"
#include "gunzip_launch.h"
#include "gunzip_ranges.h"
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

std::mutex g_err_mu;
std::string g_last_error;
void set_error(const std::string &s) { std::lock_guard<std::mutex> lk(g_err_mu); g_last_error = s; }

// the six RCCL entry points the group uses
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    // thread-safe and idempotent: groups may be created from several threads.  CRASS_RCCL_LIB names the library to bind
    // instead (tests: a name that does not exist must end in CRASS_ERR_RCCL, not in a crash)
    bool load()
    {
        std::lock_guard<std::mutex> lk(mu);
        if (lib) return true;
        const char *forced = getenv("CRASS_RCCL_LIB");
        const char *names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
        std::string why;
        if (forced && *forced) {
            lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
            if (!lib) { const char *e = dlerror(); why = e ? e : "dlopen failed"; }      // (dlerror() clears the state: read it ONCE)
        } else {
            // First the RCCL that lies beside the HIP runtime THIS library calls, by its full path.  A bare "librccl.so.1" is
            // answered with any loaded library of that soname — a torch wheel imported after this library brings its own RCCL
            // AND its own HIP runtime ($ORIGIN), and an ncclAllGather of that pair on a stream of ours (another runtime's
            // handle) aborts the process.  Where torch came first this library runs on torch's runtime, no RCCL lies beside
            // it under these names, and the soname below finds torch's: the matching pair again.
            Dl_info di{};
            if (dladdr((const void *)&hipGetDeviceCount, &di) && di.dli_fname) {
                std::string dir(di.dli_fname);
                const size_t cut = dir.rfind('/');
                if (cut != std::string::npos) {
                    dir.resize(cut + 1);
                    for (const char *n : {"librccl.so.1", "librccl.so"}) {
                        lib = dlopen((dir + n).c_str(), RTLD_NOW | RTLD_LOCAL);
                        if (lib) break;
                        (void)dlerror();
                    }
                }
            }
            for (const char *n : names) {
                if (lib) break;
                lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
                if (lib) break;
                const char *e = dlerror();
                if (why.empty()) why = e ? e : "dlopen(librccl.so.1) failed";
            }
        }
        if (!lib) { set_error("RCCL not found: " + why); return false; }
        bool missing = false;
        auto sym = [&](const char *n) { void *p = dlsym(lib, n); if (!p) { set_error(std::string("RCCL symbol missing: ") + n); missing = true; } return p; };
        CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        CommCount = (decltype(CommCount))sym("ncclCommCount");
        AllGather = (decltype(AllGather))sym("ncclAllGather");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (missing) { dlclose(lib); lib = nullptr; return false; }
        return true;
    }
    std::mutex mu;
};
Rccl g_rccl;

// sense-reversing barrier; waiters spin briefly (the ranks of a step normally arrive within microseconds of each other), then
// sleep on a condition variable: N - 1 cores at 100 % for as long as the slowest shard takes are not ours to burn
class Barrier {
public:
    explicit Barrier(int n) : n_(n) {}
    void wait()
    {
        const int gen = gen_.load(std::memory_order_acquire);
        if (count_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
            count_.store(0, std::memory_order_relaxed);
            { std::lock_guard<std::mutex> lk(m_); gen_.store(gen + 1, std::memory_order_release); }
            cv_.notify_all();
            return;
        }
        for (unsigned spin = 0; spin < 20000; spin++) {
            if (gen_.load(std::memory_order_acquire) != gen) return;
            if (spin > 2000) std::this_thread::yield();
        }
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != gen; });
    }
private:
    const int n_;
    std::atomic<int> count_{0}, gen_{0};
    std::mutex m_;
    std::condition_variable cv_;
};

enum Phase : unsigned { PH_SEED = 1, PH_MERGE = 2, PH_RECRUIT = 4, PH_LOAD = 8, PH_LOAD_FILES = 16, PH_INFLATE_GZIP = 32 };

const bool g_debug = getenv("CRASS_GROUP_DEBUG") != nullptr;           // stage trace on stderr
#define GDBG(...) do { if (g_debug) { fprintf(stderr, "[crass_group] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)

} // namespace

struct crass_hip_group {
    int n = 0;
    std::vector<int> devices;
    std::vector<crass_hip_ctx *> ctx;
    bool local_copies = false;
    std::vector<ncclComm_t> comms;
    int rccl_ranks = 0;
    // exchange buffers: rank r's send buffer belongs to its context (crass_hip_exchange_setup), recv[r] is ours
    std::vector<crass_exchange> xc;
    std::vector<void *> recv;
    std::vector<hipEvent_t> ev_send;            // local copies only: behind rank r's pass 1 on its stream (the seed scans return before their kernels end)
    uint64_t cap_rows = 16384;                  // rows per rank in the exchange; sized from the largest shard at load unless forced
    bool cap_rows_forced = false;               // CRASS_GROUP_CAP_ROWS (tests: the overflow path)
    // helper threads (ranks 1 .. n-1); the caller's thread is rank 0
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv, cv_done;
    uint64_t job_id = 0;
    unsigned job_phases = 0;
    bool quit = false;
    std::atomic<int> done{0};
    Barrier *bar = nullptr;
    std::vector<int> status;                    // per rank, of the current job
    std::atomic<int> failed{0};                 // some rank failed: the others skip their work but still meet at the barriers
    std::atomic<uint64_t> need_rows{0};
    // sharding
    uint64_t n_reads = 0, base = 0;                // base: the caller's read_index_base
    std::vector<uint64_t> first;                // [n+1] first global read of every shard
    std::vector<crass_reads> shard;             // per-rank views into the caller's / our rebased arrays (load only)
    std::vector<std::vector<uint64_t>> sh_word_off, sh_exc_read, sh_exc_off, sh_header_id;
    // duplicate headers across shards: global header id -> local index of the first read with it, per rank
    bool have_dups = false;
    std::vector<uint64_t> hid_global;           // [n_reads] copy of header_id (only when have_dups)
    std::vector<std::unordered_map<uint64_t, uint64_t>> dup_local;
    std::vector<std::vector<uint64_t>> extra;   // per rank: local read indices to mark found before pass 2 (other shards' pass-1 hits)
    std::vector<std::vector<uint64_t>> extra_user;   // per rank: the caller's extra_found, routed to the shards
    bool loaded = false, have_p1 = false, have_merge = false, have_p2 = false, explicit_patterns = false;
    // concatenated hand-off (group getters)
    struct {
        std::vector<uint64_t> read, ss_off; std::vector<uint8_t> low; std::vector<uint32_t> replen, nss, ss; std::vector<uint16_t> dr_len;
        std::vector<char> dr; uint32_t stride = 0, max_len = 0; bool ready = false;
    } C;
    struct { std::vector<uint32_t> cand_token; bool ready = false; } M;
    struct Text { std::vector<uint8_t> chars; std::vector<uint64_t> off; };
    Text T;                                     // crass_hip_group_fetch_text's result
    Text TH, TQ;                                // crass_hip_group_fetch_header_lines' and crass_hip_group_fetch_quality's
    // crass_hip_group_fetch_comments: its result, and what a files load's cuts carry — in[r] / has[r]: the comment handed to the
    // records of rank r's FIRST file part that have no source in that part (the own comment of the last own-comment record of
    // the same file on an earlier rank), first_n[r]: the records of that part; resolved at the first fetch after the load
    Text TC;
    struct { std::vector<std::string> in; std::vector<uint8_t> has; std::vector<uint64_t> first_n; bool ready = false; } CM;
    // a files load (crass_hip_group_load_fastx_files, fastx_shards.h): what the ranks share between its barriers.  Rank r writes
    // entry r of the per-rank vectors, rank 0 combines between two barriers, everybody reads behind the second
    bool files_load = false;                    // the last load was one, and was accepted
    struct FilesJob {
        std::vector<crass::ShardFile> files;
        uint32_t nf = 0, nf_eff = 0;            // the files in front of the first one the host declined; ... or a rank's staging did
        int pad_uniform = 0;
        std::vector<uint64_t> tb;               // [nf+1] text-space position of every file's byte 0
        std::vector<uint64_t> nom_x;            // [n+1] the nominal cuts in the text space
        std::vector<crass::ShardPos> nom, cut;  // [n+1] nominal and actual cuts
        std::vector<std::vector<crass::ShardPiece>> pieces;
        std::vector<crass::ShardVerdict> v_stage, v_scan;
        std::vector<std::vector<std::pair<uint32_t, uint64_t>>> file_reads;
        std::vector<uint64_t> n_reads, rank_base;
        std::vector<uint32_t> max_len;
        crass::ShardVerdict pend, verdict;      // the decline that waits for the files in front of it; the job's
        bool declined = false;
        // class 1 (crass_hip_group_set_fastq_class): the attempts the load takes — rank 0 decides on the second between two
        // barriers —, the pend the host left before the first, whether this attempt cuts and scans every '@' file by the wrapped
        // rule, and how many files the chain cut
        int attempts = 1;
        crass::ShardVerdict pend0;
        bool wrapped_pass = false;
        uint64_t n_chained = 0;
    } F;
    // crass_hip_group_inflate_gzip (gunzip_ranges.h): the file's state, which the ranks fill between barriers; where the text
    // goes; what rank 0 decided behind the count step (go on, or the call's status); the last call's counters and times
    struct GzipJob {
        crass::GzRangesFile Z;                  // crass_hip_group_inflate_gzip's file
        crass::GzRangesFile *zp = nullptr;      // the file of the running job: &Z, or one of a files load's
        // the steps of the running job: a files load indexes every gzip file first (find, count, chain: the text's size and the
        // element index, before any cut) and inflates it once the nominal cuts are known, each rank the elements of its pieces,
        // their text kept on its device (out NULL)
        bool do_index = true, do_inflate = true;
        std::vector<std::unique_ptr<crass::GzRangesFile>> files;      // a files load's, until it returns
        std::vector<crass_bgzf_index> ix;       // ... and their element indexes in a BGZF index's form (out_off: the text offsets)
        std::vector<std::vector<uint64_t>> ix_zero;
        crass::ShardVerdict v_gz;               // the first gzip file of the load that did not inflate (CRC-32, marker)
        std::vector<float> tail_ms;             // per rank: the seeded window walks of the last load, and the elements they added
        std::vector<uint64_t> tail_el;
        uint8_t *out = nullptr; uint64_t out_cap = 0;
        const uint64_t *nominal = nullptr;
        std::vector<std::vector<std::pair<uint64_t, uint64_t>>> up;      // per rank: the byte ranges of the deflate data it uploaded
        bool go = false;
        int status = 0;
        crass::GzVerdict v{};
        uint64_t cnt[6] = {0, 0, 0, 0, 0, 0};
        uint64_t cnt_members[4] = {0, 0, 0, 0};   // crass_hip_group_gzip_members_counters
        std::vector<std::array<float, 6>> ms;
        std::vector<float> crc_ms;              // per rank, members mode: k_gz_member_crc of the last finish step
    } GZ;
    int gzip_mode = 0;                          // crass_hip_group_set_gzip_on_device
    uint64_t gzip_chunk = 0;
    int fastq_class = 0;                        // crass_hip_group_set_fastq_class, CRASS_DEVICE_FASTQ at creation
    uint64_t shard_margin = 256u << 10;         // what a wrapped-mode piece stages behind its end at first (CRASS_SHARD_MARGIN at creation)
    uint64_t load_cnt[4] = {0, 0, 0, 0};        // crass_hip_group_load_counters
    struct { std::vector<uint64_t> cut_pos, file_read_base; std::vector<uint32_t> cut_file; std::vector<int32_t> format; } S;      // crass_fastx_shards' arrays
    // the names of every rank's pass-1 records, for the other ranks to look up (found headers across ranks)
    std::vector<Text> names;
    // ... or, on the device route (crass_hip_group_set_name_exchange), per rank in its device's memory: its own names and their
    // offsets (what the other ranks copy from, behind the barrier), the copy of ONE other rank's names at a time (the lookup of a
    // source has finished before the next one is copied over it), and the answers to all of them back to back — what pass 2
    // takes as its device list.  n / total: the last publish; cnt: crass_hip_group_name_exchange_counters
    struct NameX {
        uint8_t *chars = nullptr, *q_chars = nullptr; uint64_t *off = nullptr, *q_off = nullptr, *first = nullptr;
        uint64_t cap_chars = 0, cap_names = 0, cap_q_chars = 0, cap_q_names = 0, cap_first = 0;
        uint64_t n = 0, total = 0, n_first = 0;
        bool first_valid = false;               // the last merge's exchange took the device route: first[0, n_first) is pass 2's list
        uint64_t cnt[4] = {0, 0, 0, 0};
        // the last exchange on this rank, publish to lookup with the barrier between them: wall milliseconds, and (timed groups
        // only) HIP-event milliseconds on the rank's stream between the same two points
        float wall_ms = 0, event_ms = 0;
        hipEvent_t ev[2] = {nullptr, nullptr};
    };
    std::vector<NameX> nx;
    bool names_on_device = false;
    bool names_timed = false;                   // CRASS_GROUP_NAMES_TIMING at creation: the two events are recorded (tools/group_names_time.py)
    struct {
        std::vector<uint64_t> read; std::vector<uint8_t> low; std::vector<uint32_t> start, end, token; std::vector<uint16_t> dr_len;
        std::vector<char> dr; uint32_t stride = 0; bool ready = false;
    } Q;
};

namespace {

int rccl_fail(const char *what, ncclResult_t r)
{
    set_error(std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error") + " (" + std::to_string((int)r) + ")");
    return CRASS_ERR_RCCL;
}

int setup_exchange(crass_hip_group *g, int r)
{
    int s = crass_hip_exchange_setup(g->ctx[r], (uint32_t)g->n, (uint32_t)r, g->cap_rows, &g->xc[r]);
    if (s) return s;
    if (hipSetDevice(g->devices[r]) != hipSuccess) return CRASS_ERR_HIP;
    if (g->recv[r]) { crass::dev_free(g->recv[r]); g->recv[r] = nullptr; }
    if (crass::dev_alloc(&g->recv[r], (size_t)g->n * g->xc[r].send_bytes) != hipSuccess) return CRASS_ERR_OOM;
    // the seed scan returns with pass 1 queued; the collective and the merge's kernels are queued behind it before the host looks
    // at a counter (include/crass_hip.h).  CRASS_GROUP_SYNC_P1: the A/B switch (the round-5 order: wait, then exchange)
    const bool sync_p1 = getenv("CRASS_GROUP_SYNC_P1") != nullptr;        // (read per set-up: the tests flip it)
    return crass_hip_exchange_set_deferred(g->ctx[r], sync_p1 ? 0 : 1);
}

// rank 0's thread, between two barriers: every rank's send buffer is complete (its seed scan has returned)
int all_gather(crass_hip_group *g)
{
    const size_t bytes = (size_t)g->xc[0].send_bytes;
    if (g->local_copies) {
        // (every rank's stream reads every other rank's send buffer: ordered behind that rank's pass 1 by an event — a collective
        // orders this by itself)
        for (int s = 0; s < g->n; s++) {
            if (hipSetDevice(g->devices[s]) != hipSuccess) return CRASS_ERR_HIP;
            if (!g->ev_send[s] && hipEventCreateWithFlags(&g->ev_send[s], hipEventDisableTiming) != hipSuccess) return CRASS_ERR_HIP;
            if (hipEventRecord(g->ev_send[s], (hipStream_t)crass_hip_stream(g->ctx[s])) != hipSuccess) return CRASS_ERR_HIP;
        }
        for (int r = 0; r < g->n; r++) {
            if (hipSetDevice(g->devices[r]) != hipSuccess) return CRASS_ERR_HIP;
            hipStream_t st = (hipStream_t)crass_hip_stream(g->ctx[r]);
            for (int s = 0; s < g->n; s++)
                if (s != r && hipStreamWaitEvent(st, g->ev_send[s], 0) != hipSuccess) return CRASS_ERR_HIP;
            for (int s = 0; s < g->n; s++)
                if (hipMemcpyAsync((char *)g->recv[r] + (size_t)s * bytes, g->xc[s].d_send, bytes, hipMemcpyDefault, st) != hipSuccess) return CRASS_ERR_HIP;
        }
        return CRASS_OK;
    }
    ncclResult_t e = g_rccl.GroupStart();
    if (e != ncclSuccess) return rccl_fail("ncclGroupStart", e);
    for (int r = 0; r < g->n; r++) {
        e = g_rccl.AllGather(g->xc[r].d_send, g->recv[r], bytes, ncclChar, g->comms[r], (hipStream_t)crass_hip_stream(g->ctx[r]));
        if (e != ncclSuccess) { (void)g_rccl.GroupEnd(); return rccl_fail("ncclAllGather", e); }
    }
    e = g_rccl.GroupEnd();
    if (e != ncclSuccess) return rccl_fail("ncclGroupEnd", e);
    return CRASS_OK;
}

void note(crass_hip_group *g, int r, int s)
{
    if (s && !g->status[r]) g->status[r] = s;
    if (s) g->failed.store(1, std::memory_order_release);
}

// found headers that also occur in other shards: marked there before pass 2 (readsFound, libcrispr.cpp:138,411)
void collect_extra(crass_hip_group *g)
{
    for (auto &e : g->extra) e.clear();
    if (!g->have_dups) return;
    for (int r = 0; r < g->n; r++) {
        crass_candidates c;
        if (crass_hip_get_candidates(g->ctx[r], &c) != CRASS_OK) continue;
        for (uint64_t k = 0; k < c.n; k++) {
            const uint64_t h = g->hid_global[c.read_idx[k] - g->base];
            for (int q = 0; q < g->n; q++) {
                if (q == r) continue;
                auto it = g->dup_local[q].find(h);
                if (it != g->dup_local[q].end()) g->extra[q].push_back(it->second);
            }
        }
    }
}

// ---- a files load: record-aligned shards (fastx_shards.h) ----
// the file and the position inside it of text-space position x, over the first nf files
crass::ShardPos locate(const std::vector<uint64_t> &tb, uint32_t nf, uint64_t x)
{
    if (x >= tb[nf]) return crass::ShardPos{nf, 0};
    const uint32_t f = (uint32_t)(std::upper_bound(tb.begin(), tb.begin() + nf + 1, x) - tb.begin()) - 1;
    return crass::ShardPos{f, x - tb[f]};
}

// rank 0, between two barriers: every rank's pieces are probed.  The actual cuts by the rule of fastx_scan.h: a nominal cut at a
// file's position 0 is a record start; else the cut's rank has probed the range that begins there — the '\n' bytes of that
// file in front of it are the sum over the ranks before —, and "none in my range" is the next file's position 0 where the
// range reaches its file's end, else the next rank's cut: resolved from the last rank down.
int combine_cuts(crass_hip_group *g)
{
    auto &J = g->F;
    const int N = g->n;
    // a decline that a rank met while staging: the files in front of it go on, it waits for their verdict
    for (int r = 0; r < N; r++) if (crass::shard_verdict_before(J.v_stage[r], J.pend)) J.pend = J.v_stage[r];
    if (crass::shard_verdict_before(g->GZ.v_gz, J.pend)) J.pend = g->GZ.v_gz;      // (a gzip file whose CRC-32 or markers failed before the load's steps)
    J.nf_eff = J.pend.file >= 0 ? (uint32_t)J.pend.file : J.nf;
    for (int r = 0; r < N; r++) for (const crass::ShardPiece &pc : J.pieces[r]) if (pc.a == 0 && J.files[pc.file].ix) J.files[pc.file].format = pc.first_byte;
    // the wrapped pass: every '@' file's chain over the ranks, in piece order.  A piece is entered at e, the exit of the one before
    // (0 for the file's first); a record longer than the piece passes through it.  exits[f]: the pieces' exits, not decreasing
    std::vector<std::vector<uint64_t>> exits(J.nf_eff);
    J.n_chained = 0;
    for (uint32_t f = 0; J.wrapped_pass && f < J.nf_eff; f++) {
        if (J.files[f].format != 0x40) continue;
        J.n_chained++;
        uint64_t e = 0;
        bool offended = false;
        for (int r = 0; r < N && !offended; r++) for (const crass::ShardPiece &pc : J.pieces[r]) {
            if (pc.file != f) continue;
            if (e < pc.b) {
                uint32_t kind = 0; uint64_t pos = 0, off = 0;
                const int s = shard_cut_exit(g->ctx[r], J.files.data(), f, e, &kind, &pos, &off);
                if (s) return s;
                if (kind == crass::FW_CUT_OFFENCE) {    // the file's verdict: nothing behind it in this file is cut
                    crass::ShardVerdict sv;
                    sv.file = (int32_t)f; sv.reason = (int32_t)(off & 0xFF); sv.pos = off >> 8;
                    if (crass::shard_verdict_before(sv, J.pend)) J.pend = sv;
                    offended = true;
                    break;
                }
                e = pos;
            }
            exits[f].push_back(e);
        }
        if (offended) break;                            // (the files behind it are out of the set)
    }
    J.nf_eff = J.pend.file >= 0 ? (uint32_t)J.pend.file : J.nf;
    const uint32_t nf = J.nf_eff;
    J.cut.assign(N + 1, crass::ShardPos{nf, 0});
    J.cut[0] = crass::ShardPos{0, 0};
    for (int k = N - 1; k >= 1; k--) {
        const crass::ShardPos x = locate(J.tb, nf, J.nom_x[k]);
        if (x.file >= nf || x.pos == 0) { J.cut[k] = x; continue; }
        if (J.wrapped_pass && J.files[x.file].format == 0x40) {      // the first exit at or after the nominal cut; the file's end: the next file's 0
            const std::vector<uint64_t> &ex = exits[x.file];
            const auto it = std::lower_bound(ex.begin(), ex.end(), x.pos);
            if (it == ex.end()) return CRASS_ERR_STATE;
            J.cut[k] = *it < J.files[x.file].n_text ? crass::ShardPos{x.file, *it} : crass::ShardPos{x.file + 1, 0};
            continue;
        }
        J.cut[k] = J.cut[k + 1];
        if (J.pieces[k].empty()) continue;              // (an empty nominal range: the next rank's cut)
        const crass::ShardPiece &pc = J.pieces[k][0];
        if (pc.file != x.file || pc.a != x.pos) return CRASS_ERR_STATE;
        uint64_t nl_before = 0;
        for (int q = 0; q < k; q++) for (const crass::ShardPiece &o : J.pieces[q]) if (o.file == x.file) nl_before += o.probe.n_nl;
        const uint64_t pick = crass::fx_probe_pick(pc.probe, J.files[x.file].format, nl_before, pc.left_is_ls);
        if (pick != crass::kFxNone) J.cut[k] = crass::ShardPos{x.file, x.pos + pick};
        else if (pc.b == J.files[x.file].n_text) J.cut[k] = crass::ShardPos{x.file + 1, 0};
    }
    return CRASS_OK;
}

// rank 0, between two barriers: every rank's slices are scanned.  The job's verdict, or every rank's first read and the
// exchange's row capacity from the largest shard (every rank must use the same one)
void finish_scan(crass_hip_group *g)
{
    auto &J = g->F;
    J.verdict = J.pend;
    for (int r = 0; r < g->n; r++) if (crass::shard_verdict_before(J.v_scan[r], J.verdict)) J.verdict = J.v_scan[r];
    J.declined = J.verdict.file >= 0;
    if (J.declined) return;
    J.rank_base.assign(g->n + 1, 0);
    uint64_t largest = 0;
    for (int r = 0; r < g->n; r++) { J.rank_base[r + 1] = J.rank_base[r] + J.n_reads[r]; largest = std::max(largest, J.n_reads[r]); }
    if (!g->cap_rows_forced) g->cap_rows = crass_hip_exchange_rows_for(largest);
}

// rank 0, behind finish_scan of a class-1 group's first attempt: a file whose format is '@', declined for its shape, is what
// the wrapped rule takes up — the load runs once more with every '@' file cut and scanned by that rule.  Any other decline is final
void decide_second_attempt(crass_hip_group *g)
{
    auto &J = g->F;
    if (g->fastq_class != crass::FX_CLASS_WRAPPED || !J.declined || J.verdict.bgzf.reason != 0) return;
    if (J.files[J.verdict.file].format != 0x40 || !crass::fx_wrapped_takes(J.verdict.reason)) return;
    J.attempts = 2; J.wrapped_pass = true;
    J.pend = J.pend0; J.verdict = crass::ShardVerdict(); J.declined = false;
}

void load_files_rank(crass_hip_group *g, int r)
{
    auto &J = g->F;
    crass_hip_ctx *c = g->ctx[r];
    auto ok = [&] { return g->failed.load(std::memory_order_acquire) == 0; };
    for (int attempt = 1;; attempt++) {                 // (at most two: the second is decided once, behind the first)
        const bool w = attempt == 2;                    // (J.wrapped_pass, as every rank knows it)
        if (ok()) note(g, r, shard_stage_probe(c, J.files.data(), J.nf, J.nom[r], J.nom[r + 1], &J.pieces[r], &J.v_stage[r], w, g->shard_margin));
        g->bar->wait();                                 // every rank's probes (chains) are there
        if (r == 0 && ok()) { try { note(g, 0, combine_cuts(g)); } catch (const std::bad_alloc &) { note(g, 0, CRASS_ERR_OOM); } }
        g->bar->wait();                                 // the actual cuts are known
        if (ok()) note(g, r, shard_scan(c, J.files.data(), J.nf_eff, J.cut[r], J.cut[r + 1], &J.file_reads[r], &J.n_reads[r], &J.max_len[r], &J.v_scan[r], w));
        g->bar->wait();                                 // every rank's records are counted
        if (r == 0 && ok()) {
            try { finish_scan(g); if (attempt == 1) decide_second_attempt(g); } catch (const std::bad_alloc &) { note(g, 0, CRASS_ERR_OOM); }
        }
        g->bar->wait();                                 // the verdict, or every rank's first read — or one more attempt
        if (J.attempts <= attempt) break;
        shard_abort(c);
    }
    if (ok() && !J.declined) {
        int s = shard_pack(c, J.pad_uniform, J.rank_base[r]);
        if (!s) s = setup_exchange(g, r);
        note(g, r, s);
    } else shard_abort(c);
    if (!g->GZ.files.empty()) {                          // what the rank kept of the gzip files, and what its seeded walks took
        gzip_kept_report(c, &g->GZ.tail_ms[r], &g->GZ.tail_el[r], false);
        gzip_rank_report(c, g->GZ.ms[r].data(), &g->GZ.up[r]);
        gzip_kept_release(c);
    }
}

// found headers across the ranks of a files load (readsFound is keyed by header, libcrispr.cpp:138,411): installed header ids
// are per rank, so every rank publishes the names of its pass-1 records (its header lines, cut at the name) ...
int names_publish(crass_hip_group *g, int r)
{
    crass_hip_group::Text &NM = g->names[r];
    NM.chars.clear(); NM.off.assign(1, 0);
    crass_candidates cd;
    int s = crass_hip_get_candidates(g->ctx[r], &cd);
    if (s || !cd.n) return s;
    const uint8_t *arena = nullptr; const uint64_t *rec_pos = nullptr; uint64_t nb = 0, nr = 0;
    if ((s = shard_records(g->ctx[r], &arena, &nb, &rec_pos, &nr))) return s;
    std::vector<uint64_t> idx(cd.n);
    std::vector<uint32_t> name_len(cd.n);
    for (uint64_t k = 0; k < cd.n; k++) idx[k] = cd.read_idx[k] - g->first[r];
    crass_text t;
    if ((s = crass_hip_fetch_header_lines_device(g->ctx[r], arena, nb, rec_pos, nr, idx.data(), cd.n, &t, name_len.data()))) return s;
    for (uint64_t k = 0; k < cd.n; k++) {
        NM.chars.insert(NM.chars.end(), t.chars + t.off[k], t.chars + t.off[k] + name_len[k]);
        NM.off.push_back(NM.chars.size());
    }
    return CRASS_OK;
}

// ... and looks the other ranks' names up in its own table: its namesakes are marked found before pass 2
int names_lookup(crass_hip_group *g, int r)
{
    std::vector<uint64_t> &e = g->extra[r];
    e.clear();
    std::vector<uint64_t> first;
    uint64_t looked = 0;
    for (int q = 0; q < g->n; q++) {
        const crass_hip_group::Text &NM = g->names[q];
        const uint64_t nq = NM.off.size() - 1;
        if (q == r || !nq) continue;
        first.resize(nq);
        const int s = crass_hip_fastx_names_find(g->ctx[r], NM.chars.data(), NM.off.data(), nq, first.data());
        if (s) return s;
        for (uint64_t k = 0; k < nq; k++) if (first[k] != CRASS_NAME_NOT_FOUND) e.push_back(first[k]);
        looked += nq;
    }
    crass_hip_group::NameX &X = g->nx[r];
    X.n_first = 0; X.first_valid = false;
    X.cnt[0] = 0; X.cnt[1] = g->names[r].off.size() - 1; X.cnt[2] = looked; X.cnt[3] = e.size();
    return CRASS_OK;
}

// ---- the same exchange on the device route: no name, answer or index crosses to the host, only counts and totals ----
// a buffer of at least `want` elements (+ extra) on the rank's device (the current device); what it held is dropped
template <typename T> int nx_grow(T *&p, uint64_t &cap, uint64_t want, uint64_t extra)
{
    if (p && cap >= want) return CRASS_OK;
    if (p) { crass::dev_free(p); p = nullptr; cap = 0; }
    void *q = nullptr;
    if (crass::dev_alloc(&q, (size_t)((want + extra) * sizeof(T))) != hipSuccess) return CRASS_ERR_OOM;
    p = (T *)q; cap = want;
    return CRASS_OK;
}

void nx_free(crass_hip_group *g, int r)
{
    crass_hip_group::NameX &X = g->nx[r];
    (void)hipSetDevice(g->devices[r]);
    for (void *p : {(void *)X.chars, (void *)X.q_chars, (void *)X.off, (void *)X.q_off, (void *)X.first}) if (p) crass::dev_free(p);
    for (hipEvent_t e : X.ev) if (e) (void)hipEventDestroy(e);
    X = crass_hip_group::NameX{};
}

// no list of namesakes is left for pass 2, on either route (a load, an explicit pattern set)
void clear_extra(crass_hip_group *g)
{
    for (auto &e : g->extra) e.clear();
    for (auto &X : g->nx) { X.n_first = 0; X.first_valid = false; }
}

// rank r's names into its own buffer, sized from the step before (the first step: from the candidate count); too small: regrown
// to the totals the call reported and the call repeated, once
int names_publish_device(crass_hip_group *g, int r)
{
    crass_hip_group::NameX &X = g->nx[r];
    X.n = X.total = 0;
    if (hipSetDevice(g->devices[r]) != hipSuccess) return CRASS_ERR_HIP;
    crass_counters k{};
    (void)crass_hip_get_counters(g->ctx[r], &k);
    const uint64_t want_n = std::max<uint64_t>(X.cap_names, k.n_pass1_found), want_b = std::max<uint64_t>(X.cap_chars, 32 * want_n);
    int s;
    if ((s = nx_grow(X.off, X.cap_names, want_n, 1)) || (s = nx_grow(X.chars, X.cap_chars, want_b, 0))) return s;
    uint64_t n = 0, total = 0;
    s = crass_hip_found_names_device(g->ctx[r], X.chars, X.cap_chars, X.off, X.cap_names, &n, &total);
    if (s == CRASS_ERR_OVERFLOW) {
        if ((s = nx_grow(X.off, X.cap_names, n + n / 4, 1)) || (s = nx_grow(X.chars, X.cap_chars, total + total / 4, 0))) return s;
        s = crass_hip_found_names_device(g->ctx[r], X.chars, X.cap_chars, X.off, X.cap_names, &n, &total);
    }
    if (s) return s;
    X.n = n; X.total = total;
    return CRASS_OK;
}

// behind the barrier: every other rank's names and offsets to this rank's device on its stream, looked up there; the answers of
// all sources back to back in X.first.  (A source's buffers are not written again before the next step's publish, which lies
// behind that step's barriers.)
int names_lookup_device(crass_hip_group *g, int r)
{
    crass_hip_group::NameX &X = g->nx[r];
    g->extra[r].clear();
    X.n_first = 0; X.first_valid = false;
    if (hipSetDevice(g->devices[r]) != hipSuccess) return CRASS_ERR_HIP;
    hipStream_t st = (hipStream_t)crass_hip_stream(g->ctx[r]);
    uint64_t n_all = 0, found = 0, at = 0;
    for (int q = 0; q < g->n; q++) if (q != r) n_all += g->nx[q].n;
    int s;
    if ((s = nx_grow(X.first, X.cap_first, n_all, 0))) return s;
    for (int q = 0; q < g->n; q++) {
        const crass_hip_group::NameX &Q = g->nx[q];
        if (q == r || !Q.n) continue;
        if ((s = nx_grow(X.q_off, X.cap_q_names, Q.n, 1)) || (s = nx_grow(X.q_chars, X.cap_q_chars, Q.total, 0))) return s;
        hipError_t e = hipSuccess;
        if (g->local_copies || g->devices[q] == g->devices[r]) {
            e = hipMemcpyAsync(X.q_off, Q.off, (Q.n + 1) * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && Q.total) e = hipMemcpyAsync(X.q_chars, Q.chars, Q.total, hipMemcpyDeviceToDevice, st);
        } else {
            e = hipMemcpyPeerAsync(X.q_off, g->devices[r], Q.off, g->devices[q], (Q.n + 1) * 8, st);
            if (e == hipSuccess && Q.total) e = hipMemcpyPeerAsync(X.q_chars, g->devices[r], Q.chars, g->devices[q], Q.total, st);
        }
        if (e != hipSuccess) { set_error(std::string("found-name exchange, copy of rank ") + std::to_string(q) + "'s names: " + hipGetErrorString(e)); return CRASS_ERR_HIP; }
        if ((s = crass_hip_fastx_names_find_device(g->ctx[r], X.q_chars, Q.total, X.q_off, Q.n, X.first + at))) return s;
        found += names_find_device_found(g->ctx[r]);
        at += Q.n;
    }
    X.n_first = at; X.first_valid = true;
    X.cnt[0] = 1; X.cnt[1] = X.n; X.cnt[2] = at; X.cnt[3] = found;
    return CRASS_OK;
}

// crass_hip_group_inflate_gzip, rank 0 behind the count step: the chain, the text's size, every rank's elements.  A decline or a
// text that does not fit ends the job there (J.go stays false, J.status says why)
int gzip_chain_host(crass_hip_group *g)
{
    auto &J = g->GZ;
    crass::GzRangesFile &Z = *J.zp;
    const uint64_t nc = Z.M.G.nc;
    Z.chain.assign(nc, 0);
    const int32_t bad = crass::gz_chain(Z.M, Z.start.data(), Z.link.data(), Z.text_len.data(), Z.end_bit.data(), Z.reason.data(), Z.chain.data(),
                                        &Z.n_chain, &Z.n_text, &J.v, Z.members);
    if (bad != crass::BZ_OK) { J.status = CRASS_ERR_UNSUPPORTED; return CRASS_OK; }
    if (J.do_inflate && J.out_cap < Z.n_text) { J.status = CRASS_ERR_OVERFLOW; return CRASS_OK; }
    const uint64_t n = Z.n_chain;
    Z.off.assign(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) Z.off[i + 1] = Z.off[i] + Z.text_len[Z.chain[i]];
    Z.crc_part.assign(n, 0);
    if (Z.members) {                                    // the places of the GzEnd records and every element's member start
        Z.slot.assign(n + 1, 0); Z.m0.assign(n, 0);
        crass::gz_places(Z.chain.data(), n, Z.text_len.data(), Z.n_ends.data(), Z.last_end.data(), Z.off.data(), Z.slot.data(), Z.m0.data());
        Z.ends.assign(Z.slot[n], crass::GzEnd{0, 0, 0, 0});
        Z.table_ok = false; Z.n_pieces = 0;
    }
    if (!J.do_inflate) return CRASS_OK;                 // (a files load: the ranges follow once the cuts are known)
    const uint32_t N = (uint32_t)g->n;
    Z.e0.assign(N + 1, n); Z.e1.assign(N + 1, n); Z.first.assign(N + 1, 0);
    if (!crass::gz_ranges(Z.off.data(), n, N, J.nominal, Z.e0.data(), Z.e1.data())) { J.status = CRASS_ERR_INVALID_ARG; return CRASS_OK; }
    for (uint32_t r = 0; r < N; r++) Z.first[r + 1] = std::max(Z.first[r], Z.e1[r]);
    J.go = true;
    return CRASS_OK;
}

// ... behind the decode step: every rank's entry window, composed in rank order from what the rank in front exported (a rank
// without elements of its own, or one that starts in the same element, passes its entry window on)
void gzip_compose_host(crass_hip_group *g)
{
    crass::GzRangesFile &Z = *g->GZ.zp;
    Z.entry[0].clear();
    for (int r = 0; r + 1 < g->n; r++) {
        if (Z.e0[r + 1] >= Z.n_chain) { Z.entry[r + 1].clear(); continue; }      // (no elements: nothing to enter)
        if (Z.exported[r].empty()) { Z.entry[r + 1] = Z.entry[r]; continue; }
        const uint8_t *in = Z.entry[r].empty() ? nullptr : Z.entry[r].data();
        Z.entry[r + 1].resize(crass::kGzWindow);
        for (uint32_t w = 0; w < crass::kGzWindow; w++) Z.entry[r + 1][w] = crass::gz_window_resolve(Z.exported[r][w], in);
    }
}

// ... in members mode, behind the composition: the member table from the gathered GzEnd records (every element's from its first
// holder) and the text cuts of the CRC pieces, cut also where a rank's own text begins; the exported windows that held no
// reference are counted (a range that holds a member boundary exports such a window: its dead entries read 0)
void gzip_members_host(crass_hip_group *g)
{
    crass::GzRangesFile &Z = *g->GZ.zp;
    const uint64_t n = Z.n_chain, nm = Z.slot[n];
    Z.exported_plain = 0;
    for (int r = 0; r + 1 < g->n; r++) {
        if (Z.exported[r].empty()) continue;
        bool plain = true;
        for (uint16_t w : Z.exported[r]) if (w >= 0x8000u) { plain = false; break; }
        Z.exported_plain += plain;
    }
    Z.table_ok = false; Z.n_pieces = 0;
    if (nm == 0) return;                                // (never expected: the chain ends behind a final block)
    Z.in_off.assign(nm + 1, 0); Z.text_off.assign(nm + 1, 0); Z.mcrc.assign(nm, 0); Z.misz.assign(nm, 0);
    crass::gz_member_table(Z.M, Z.n_bytes, Z.off.data(), Z.slot.data(), n, Z.ends.data(), Z.in_off.data(), Z.text_off.data(), Z.mcrc.data(), Z.misz.data());
    for (uint64_t m = 0; m < nm; m++) if (Z.text_off[m + 1] < Z.text_off[m] || Z.text_off[m + 1] > Z.n_text) return;      // (a record nobody wrote)
    if (Z.text_off[nm] != Z.n_text) return;
    std::vector<uint64_t> base;
    for (int r = 0; r < g->n; r++) {
        const uint64_t f = std::max(Z.e0[r], Z.first[r]);
        if (f < Z.e1[r]) base.push_back(Z.off[f]);
    }
    Z.piece.assign(nm + Z.n_text / crass::kGzCrcPiece + base.size() + 2, 0);
    Z.n_pieces = crass::gz_crc_pieces(Z.text_off.data(), nm, base.data(), base.size(), Z.piece.data());
    Z.crc_piece.assign(Z.n_pieces ? Z.n_pieces : 1, 0);
    Z.table_ok = true;
}

// ... at the end: every member's CRC-32 joined from its pieces, the first offending member (7 / 8 before 9)
int32_t gzip_members_verdict(const crass::GzRangesFile &Z, crass::GzVerdict *v)
{
    const uint64_t nm = Z.in_off.size() - 1;
    std::vector<uint32_t> got(nm, 0);
    uint64_t q = 0;
    for (uint64_t m = 0; m < nm; m++)
        for (; q < Z.n_pieces && Z.piece[q] < Z.text_off[m + 1]; q++) got[m] = crass::gz_crc_join(got[m], Z.crc_piece[q], Z.piece[q + 1] - Z.piece[q]);
    return crass::gz_member_verdict(nm, Z.in_off.data(), Z.text_off.data(), Z.mcrc.data(), Z.misz.data(), got.data(), v);
}

// a file's state before the index step: the header and the trailer parsed (false: not a gzip member), the per-chunk arrays empty
bool gzip_file_init(crass::GzRangesFile &Z, const uint8_t *bytes, uint64_t n_bytes, uint32_t n_ranks, uint64_t chunk_bytes, bool members = false)
{
    Z = crass::GzRangesFile();
    Z.bytes = bytes; Z.n_bytes = n_bytes; Z.n_ranks = n_ranks; Z.members = members;
    if (crass::gz_parse_member(bytes, n_bytes, n_bytes >= 8 ? bytes + n_bytes - 8 : nullptr, n_bytes, chunk_bytes, &Z.M) != crass::BZ_OK) return false;
    const uint64_t nc = Z.M.G.nc;
    Z.start.assign(nc, crass::kGzNoStart); Z.text_len.assign(nc, 0); Z.end_bit.assign(nc, 0);
    Z.link.assign(nc, crass::GZ_LINK_NONE); Z.reason.assign(nc, 0);
    if (members) { Z.n_ends.assign(nc, 0); Z.last_end.assign(nc, 0); }
    return true;
}

void gzip_inflate_rank(crass_hip_group *g, int r)
{
    auto &J = g->GZ;
    crass_hip_ctx *c = g->ctx[r];
    auto ok = [&] { return g->failed.load(std::memory_order_acquire) == 0; };
    crass::GzRangesFile &Z = *J.zp;
    if (J.do_index) {
        if (ok()) note(g, r, gzip_rank_find(c, Z, (uint32_t)r));
        g->bar->wait();                                 // every chunk's start is there
        if (ok()) note(g, r, gzip_rank_count(c, Z, (uint32_t)r));
        g->bar->wait();                                 // ... and what its run counted
        if (r == 0 && ok()) { try { note(g, 0, gzip_chain_host(g)); } catch (const std::bad_alloc &) { note(g, 0, CRASS_ERR_OOM); } }
        g->bar->wait();                                 // the chain and the ranges, or the end of the job
    }
    if (J.do_inflate) {
        if (ok() && J.go) note(g, r, gzip_rank_decode(c, Z, (uint32_t)r));
        g->bar->wait();                                 // every rank's exported window
        if (r == 0 && ok() && J.go) { try { gzip_compose_host(g); if (Z.members) gzip_members_host(g); } catch (const std::bad_alloc &) { note(g, 0, CRASS_ERR_OOM); } }
        g->bar->wait();                                 // every rank's entry window
        if (ok() && J.go) note(g, r, gzip_rank_finish(c, Z, (uint32_t)r, J.out, !J.do_index));
    }
    gzip_rank_report(c, J.ms[r].data(), &J.up[r]);
    if (J.do_inflate && (size_t)r < J.crc_ms.size()) J.crc_ms[r] = gzip_rank_member_crc_ms(c);
    if (J.do_index && J.do_inflate) gzip_rank_release(c);      // (a files load keeps the staged bytes and gives all scratch back at its end)
}

// one rank's part of a job; every rank passes the same barriers whatever happens
void run_rank(crass_hip_group *g, int r, unsigned phases)
{
    crass_hip_ctx *c = g->ctx[r];
    auto ok = [&] { return g->failed.load(std::memory_order_acquire) == 0; };
    if (phases & PH_LOAD_FILES) { load_files_rank(g, r); return; }
    if (phases & PH_INFLATE_GZIP) { gzip_inflate_rank(g, r); return; }
    if (phases & PH_LOAD) {
        int s = crass_hip_load_reads(c, &g->shard[r]);
        if (!s) s = setup_exchange(g, r);
        note(g, r, s);
        return;
    }
    if ((phases & PH_SEED) && ok()) note(g, r, crass_hip_seed_scan(c));
    if (phases & PH_MERGE) {
        for (int attempt = 0; attempt < 6; attempt++) {
            GDBG("rank %d attempt %d: at barrier A", r, attempt);
            g->bar->wait();                                         // every send buffer is complete
            if (r == 0) { g->need_rows.store(0); if (ok()) note(g, 0, all_gather(g)); }
            g->bar->wait();                                         // the collective is queued on every rank's stream
            GDBG("rank %d attempt %d: merge_gathered", r, attempt);
            int s = ok() ? crass_hip_merge_gathered(c, g->recv[r]) : CRASS_OK;
            GDBG("rank %d attempt %d: merge_gathered -> %d", r, attempt, s);
            if (s == CRASS_ERR_OVERFLOW) {
                uint64_t need = crass_hip_exchange_needed_rows(c), cur = g->need_rows.load();
                while (need > cur && !g->need_rows.compare_exchange_weak(cur, need)) {}
                s = CRASS_OK;
            }
            note(g, r, s);
            g->bar->wait();                                         // every rank knows whether the lists fitted
            const uint64_t need = g->need_rows.load();
            if (!need || !ok()) break;
            if (attempt == 5) { note(g, r, CRASS_ERR_OVERFLOW); break; }
            // some rank's list did not fit: larger buffers everywhere, pass 1 again (its kernel fills the send buffer)
            if (r == 0) { uint64_t cap = g->cap_rows; while (cap < need * 2) cap *= 2; g->cap_rows = cap; }
            g->bar->wait();
            GDBG("rank %d attempt %d: %llu rows needed, exchange set up again with %llu", r, attempt, (unsigned long long)need, (unsigned long long)g->cap_rows);
            int t = setup_exchange(g, r);
            GDBG("rank %d attempt %d: setup -> %d, pass 1 again", r, attempt, t);
            if (!t) t = crass_hip_seed_scan(c);
            GDBG("rank %d attempt %d: pass 1 -> %d", r, attempt, t);
            note(g, r, t);
        }
        if (g->have_dups) {
            g->bar->wait();
            if (r == 0 && ok()) { try { collect_extra(g); } catch (const std::bad_alloc &) { note(g, 0, CRASS_ERR_OOM); } }
            g->bar->wait();
        }
        if (g->files_load && g->n > 1) {                            // (with one rank nothing is exchanged)
            const bool dev = g->names_on_device;                    // (set between jobs: the same on every rank of a job)
            crass_hip_group::NameX &X = g->nx[r];
            const auto t0 = std::chrono::steady_clock::now();
            bool timed = g->names_timed && ok() && hipSetDevice(g->devices[r]) == hipSuccess;
            for (hipEvent_t &e : X.ev) if (timed && !e) timed = hipEventCreate(&e) == hipSuccess;
            if (timed) timed = hipEventRecord(X.ev[0], (hipStream_t)crass_hip_stream(c)) == hipSuccess;
            try { if (ok()) note(g, r, dev ? names_publish_device(g, r) : names_publish(g, r)); } catch (const std::bad_alloc &) { note(g, r, CRASS_ERR_OOM); }
            g->bar->wait();                                         // every rank's names are there
            try { if (ok()) note(g, r, dev ? names_lookup_device(g, r) : names_lookup(g, r)); } catch (const std::bad_alloc &) { note(g, r, CRASS_ERR_OOM); }
            X.event_ms = 0;
            if (timed && hipSetDevice(g->devices[r]) == hipSuccess && hipEventRecord(X.ev[1], (hipStream_t)crass_hip_stream(c)) == hipSuccess &&
                hipEventSynchronize(X.ev[1]) == hipSuccess) (void)hipEventElapsedTime(&X.event_ms, X.ev[0], X.ev[1]);
            X.wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    }
    if ((phases & PH_RECRUIT) && ok()) {
        std::vector<uint64_t> &e = g->extra[r];
        const std::vector<uint64_t> &u = g->extra_user[r];
        // the device route's namesakes: the answers as the lookup left them on this rank's device, beside the host lists
        const crass_hip_group::NameX &X = g->nx[r];
        const uint64_t *d_first = X.first_valid && X.n_first ? X.first : nullptr;
        const uint64_t n_d = d_first ? X.n_first : 0;
        // (no barrier behind this point: an allocation failure here only ends this rank's part)
        try {
            if (!u.empty()) {                                       // (this call's; extra[r] is rebuilt by the next merge)
                std::vector<uint64_t> both(e);
                both.insert(both.end(), u.begin(), u.end());
                note(g, r, crass_hip_recruit_found(c, both.data(), both.size(), d_first, n_d));
            } else note(g, r, crass_hip_recruit_found(c, e.empty() ? nullptr : e.data(), e.size(), d_first, n_d));
        } catch (const std::bad_alloc &) { note(g, r, CRASS_ERR_OOM); }
    }
}

void helper_loop(crass_hip_group *g, int r)
{
    uint64_t seen = 0;
    (void)hipSetDevice(g->devices[r]);                  // this thread's current device (every context call sets it again)
    for (;;) {
        unsigned phases;
        {
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv.wait(lk, [&] { return g->quit || g->job_id != seen; });
            if (g->quit) return;
            seen = g->job_id; phases = g->job_phases;
        }
        run_rank(g, r, phases);
        g->done.fetch_add(1, std::memory_order_release);
        { std::lock_guard<std::mutex> lk(g->mu); }      // (the waiter is either before its check or asleep: no lost wake-up)
        g->cv_done.notify_one();
    }
}

int dispatch(crass_hip_group *g, unsigned phases)
{
    std::fill(g->status.begin(), g->status.end(), 0);
    g->failed.store(0);
    g->done.store(0);
    if (g->n > 1) {
        { std::lock_guard<std::mutex> lk(g->mu); g->job_id++; g->job_phases = phases; }
        g->cv.notify_all();
    }
    run_rank(g, 0, phases);
    for (unsigned spin = 0; g->done.load(std::memory_order_acquire) != g->n - 1; spin++) {
        if (spin > 20000) {                             // (rank 0 finished well ahead of the others: sleep until the last one reports)
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv_done.wait_for(lk, std::chrono::milliseconds(2), [&] { return g->done.load(std::memory_order_acquire) == g->n - 1; });
        } else if (spin > 2000) std::this_thread::yield();
    }
    for (int r = 0; r < g->n; r++) if (g->status[r]) return g->status[r];
    return CRASS_OK;
}

// a step of a files load on one of its gzip files: the index step, or — its ranges set — the inflate step whose text the ranks keep
int gzip_job_run(crass_hip_group *g, crass::GzRangesFile &Z, bool index, bool inflate)
{
    auto &J = g->GZ;
    const size_t N = (size_t)g->n;
    J.zp = &Z; J.do_index = index; J.do_inflate = inflate;
    J.out = nullptr; J.out_cap = 0; J.nominal = nullptr; J.status = CRASS_OK;
    if (index) { J.v = crass::GzVerdict{}; J.go = false; }
    else { Z.exported.assign(N, {}); Z.entry.assign(N, {}); Z.bad.assign(N, ~0ull); J.go = true; }
    return dispatch(g, PH_INFLATE_GZIP);
}

} // namespace

extern "C" {

const char *crass_hip_group_last_error(void)
{
    static thread_local std::string copy;
    std::lock_guard<std::mutex> lk(g_err_mu);
    copy = g_last_error;
    return copy.c_str();
}

int crass_hip_group_create(const crass_params *p, const int *devices, int n, unsigned flags, crass_hip_group **out)
{
    if (!p || !devices || !out || n <= 0 || n > 64 || (flags & ~CRASS_GROUP_LOCAL_COPIES)) return CRASS_ERR_INVALID_ARG;
    *out = nullptr;
    set_error("");
    bool dup = false;
    for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (devices[i] == devices[j]) dup = true;
    const bool local = (flags & CRASS_GROUP_LOCAL_COPIES) != 0;
    if (dup && !local) { set_error("a device is listed twice: RCCL needs one rank per device (CRASS_GROUP_LOCAL_COPIES for tests)"); return CRASS_ERR_INVALID_ARG; }
    if (!local && !g_rccl.load()) return CRASS_ERR_RCCL;            // (before any context: no RCCL, no group — text in crass_hip_group_last_error)
    if (!local && getenv("CRASS_GROUP_INJECT_RCCL_FAIL")) {         // tests: what a caller sees when ncclCommInitAll refuses (its fall-back path)
        set_error("ncclCommInitAll: injected failure (CRASS_GROUP_INJECT_RCCL_FAIL)");
        return CRASS_ERR_RCCL;
    }
    crass_hip_group *g = new (std::nothrow) crass_hip_group();
    if (!g) return CRASS_ERR_OOM;
    g->n = n; g->devices.assign(devices, devices + n); g->local_copies = local;
    g->ctx.assign(n, nullptr); g->xc.assign(n, crass_exchange{}); g->recv.assign(n, nullptr); g->status.assign(n, 0); g->ev_send.assign(n, nullptr);
    g->extra.resize(n); g->extra_user.resize(n); g->dup_local.resize(n); g->nx.resize(n);
    if (const char *e = getenv("CRASS_GROUP_NAMES")) g->names_on_device = strcmp(e, "device") == 0;      // (crass_hip_group_set_name_exchange)
    g->names_timed = getenv("CRASS_GROUP_NAMES_TIMING") != nullptr;
    if (const char *e = getenv("CRASS_DEVICE_FASTQ")) g->fastq_class = strcmp(e, "wrapped") == 0 ? 1 : 0;      // (crass_hip_group_set_fastq_class)
    if (const char *e = getenv("CRASS_SHARD_MARGIN")) g->shard_margin = std::max<uint64_t>(1, strtoull(e, nullptr, 10));      // (tests: a tiny margin forces the doublings)
    if (const char *e = getenv("CRASS_GROUP_CAP_ROWS")) { g->cap_rows = (uint64_t)std::max(1, atoi(e)); g->cap_rows_forced = true; }      // (tests: force the overflow path)
    for (int r = 0; r < n; r++) {
        const int s = crass_hip_create(p, devices[r], &g->ctx[r]);
        if (s) { crass_hip_group_destroy(g); return s; }
        if (r > 0) (void)crass_hip_set_host_view(g->ctx[r], 1);       // ONE host view for the group: rank 0's
        (void)crass_hip_set_fastq_class(g->ctx[r], g->fastq_class);
    }
    if (!local) {
        g->comms.assign(n, nullptr);
        const ncclResult_t e = g_rccl.CommInitAll(g->comms.data(), n, devices);
        if (e != ncclSuccess) { g->comms.clear(); crass_hip_group_destroy(g); return rccl_fail("ncclCommInitAll", e); }
        int cnt = 0;
        const ncclResult_t e2 = g_rccl.CommCount(g->comms[0], &cnt);
        if (e2 != ncclSuccess) { crass_hip_group_destroy(g); return rccl_fail("ncclCommCount", e2); }
        g->rccl_ranks = cnt;
    }
    g->bar = new Barrier(n);
    for (int r = 1; r < n; r++) g->threads.emplace_back(helper_loop, g, r);
    *out = g;
    return CRASS_OK;
}

void crass_hip_group_destroy(crass_hip_group *g)
{
    if (!g) return;
    { std::lock_guard<std::mutex> lk(g->mu); g->quit = true; }
    g->cv.notify_all();
    for (auto &t : g->threads) t.join();
    for (int r = 0; r < g->n; r++) {
        if (g->recv[r]) { (void)hipSetDevice(g->devices[r]); crass::dev_free(g->recv[r]); }
        if (g->ctx[r]) {
            (void)hipSetDevice(g->devices[r]);
            (void)hipStreamSynchronize((hipStream_t)crass_hip_stream(g->ctx[r]));
        }
    }
    for (int r = 0; r < (int)g->nx.size(); r++) nx_free(g, r);      // (behind every stream's wait: a lookup may have read another rank's names)
    for (int r = 0; r < g->n; r++) if (g->ev_send[r]) { (void)hipSetDevice(g->devices[r]); (void)hipEventDestroy(g->ev_send[r]); }
    for (auto cm : g->comms) if (cm) (void)g_rccl.CommDestroy(cm);
    for (auto c : g->ctx) if (c) crass_hip_destroy(c);
    delete g->bar;
    delete g;
}

int crass_hip_group_size(const crass_hip_group *g) { return g ? g->n : 0; }

int crass_hip_group_set_name_exchange(crass_hip_group *g, int on_device)
{
    if (!g) return CRASS_ERR_INVALID_ARG;
    g->names_on_device = on_device != 0;
    return CRASS_OK;
}

int crass_hip_group_set_fastq_class(crass_hip_group *g, int fastq_class)
{
    if (!g || fastq_class < 0 || fastq_class > 1) return CRASS_ERR_INVALID_ARG;
    for (crass_hip_ctx *c : g->ctx) { const int s = crass_hip_set_fastq_class(c, fastq_class); if (s) return s; }      // (fetch_quality reads by the context's class)
    g->fastq_class = fastq_class;
    return CRASS_OK;
}

int crass_hip_group_load_counters(const crass_hip_group *g, uint64_t out[4])
{
    if (!g || !out) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = g->load_cnt[k];
    return CRASS_OK;
}

static int group_inflate_gzip(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal, uint8_t *out_host,
                              uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, bool mem, crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    if (plan) memset(plan, 0, sizeof(*plan));
    if (members) memset(members, 0, sizeof(*members));
    if (n_text) *n_text = 0;
    if (!g || !n_text || (n_bytes && !bytes) || (out_cap && !out_host)) return CRASS_ERR_INVALID_ARG;
    auto &J = g->GZ;
    for (auto &x : J.cnt) x = 0;
    for (auto &x : J.cnt_members) x = 0;
    auto decline = [&](int32_t reason, uint64_t member, uint64_t in_pos) {
        if (v) { v->reason = reason; v->member = member; v->in_pos = in_pos; }
        return CRASS_ERR_UNSUPPORTED;
    };
    try {
        const uint32_t N = (uint32_t)g->n;
        crass::GzRangesFile &Z = J.Z;
        J.zp = &Z; J.do_index = J.do_inflate = true;
        for (int r = 0; r < g->n; r++) gzip_kept_report(g->ctx[r], nullptr, nullptr, true);
        J.ms.assign(N, std::array<float, 6>{}); J.up.assign(N, {}); J.tail_ms.assign(N, 0.0f); J.tail_el.assign(N, 0); J.crc_ms.assign(N, 0.0f);
        if (!gzip_file_init(Z, bytes, n_bytes, N, chunk_bytes, mem)) return decline(crass::BZ_NOT_GZIP, 0, 0);
        const uint64_t nc = Z.M.G.nc;
        Z.exported.assign(N, {}); Z.entry.assign(N, {}); Z.bad.assign(N, ~0ull);
        J.out = out_host; J.out_cap = out_cap; J.nominal = nominal; J.go = false; J.status = CRASS_OK; J.v = crass::GzVerdict{};
        const int st = dispatch(g, PH_INFLATE_GZIP);
        if (st) return st;
        const int ps = crass::gz_plan_fill(plan, nc, Z.start.data(), Z.link.data(), Z.text_len.data(), Z.n_chain);
        if (ps) return ps;
        if (J.status == CRASS_ERR_UNSUPPORTED) return decline(J.v.reason, J.v.member, J.v.in_pos);
        if (J.status == CRASS_ERR_INVALID_ARG) return J.status;
        *n_text = Z.n_text;
        if (J.status) return J.status;                  // (the text does not fit: known before anything is stored)
        // the counters: elements held by a further rank, bytes uploaded and those of them that some upload had brought already
        const uint64_t n = Z.n_chain;
        uint64_t held = 0, sent = 0, distinct = 0;
        std::vector<std::pair<uint64_t, uint64_t>> all;
        for (uint32_t r = 0; r < N; r++) {
            held += Z.e1[r] - Z.e0[r];
            for (const auto &u : J.up[r]) { sent += u.second - u.first; all.push_back(u); }
        }
        std::sort(all.begin(), all.end());
        uint64_t reach = 0;
        for (const auto &u : all) { if (u.second > reach) { distinct += u.second - std::max(u.first, reach); reach = u.second; } }
        J.cnt[0] = 1; J.cnt[1] = nc; J.cnt[2] = n; J.cnt[3] = held - n; J.cnt[4] = sent; J.cnt[5] = sent - distinct;
        // an unresolved marker: the smallest element over the ranks; then the CRC-32, every part from the first rank that holds it
        uint64_t bad = ~0ull;
        for (uint32_t r = 0; r < N; r++) bad = std::min(bad, Z.bad[r]);
        if (bad != ~0ull) { const uint64_t k = Z.chain[bad]; return decline(crass::BZ_MARKER, k, Z.M.G.d_off + (Z.start[k] >> 3)); }
        if (mem) {
            // the verdict in the host rule's order: 14 above, then the first offending member
            if (!Z.table_ok) return CRASS_ERR_STATE;
            J.cnt_members[0] = 1; J.cnt_members[1] = Z.in_off.size() - 1; J.cnt_members[2] = Z.n_pieces; J.cnt_members[3] = Z.exported_plain;
            crass::GzVerdict mv{};
            if (gzip_members_verdict(Z, &mv) != crass::BZ_OK) return decline(mv.reason, mv.member, mv.in_pos);
            return crass::gz_members_fill(members, Z.in_off.size() - 1, Z.in_off.data(), Z.text_off.data());
        }
        uint32_t crc = 0;
        for (uint64_t i = 0; i < n; i++) crc = crass::gz_crc_join(crc, Z.crc_part[i], Z.off[i + 1] - Z.off[i]);
        if (crc != Z.M.crc) return decline(crass::BZ_CRC, 0, 0);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int crass_hip_group_inflate_gzip(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal,
                                 uint8_t *out_host, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v)
{
    return group_inflate_gzip(g, bytes, n_bytes, chunk_bytes, nominal, out_host, out_cap, n_text, plan, nullptr, false, v);
}

int crass_hip_group_inflate_gzip_members(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal,
                                         uint8_t *out_host, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members,
                                         crass_bgzf_verdict *v)
{
    return group_inflate_gzip(g, bytes, n_bytes, chunk_bytes, nominal, out_host, out_cap, n_text, plan, members, true, v);
}

int crass_hip_group_gzip_members_counters(const crass_hip_group *g, uint64_t out[4])
{
    if (!g || !out) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = g->GZ.cnt_members[k];
    return CRASS_OK;
}

int crass_hip_group_gzip_members_ms(const crass_hip_group *g, int rank, float out[1])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    out[0] = (size_t)rank < g->GZ.crc_ms.size() ? g->GZ.crc_ms[rank] : 0.0f;
    return CRASS_OK;
}

int crass_hip_group_set_gzip_on_device(crass_hip_group *g, int mode, uint64_t chunk_bytes)
{
    if (!g || mode < 0) return CRASS_ERR_INVALID_ARG;
    g->gzip_mode = mode == CRASS_GZIP_ON_DEVICE_MEMBERS ? CRASS_GZIP_ON_DEVICE_MEMBERS : mode ? CRASS_GZIP_ON_DEVICE_ONE_MEMBER : CRASS_GZIP_ON_DEVICE_OFF;
    g->gzip_chunk = chunk_bytes ? crass::gz_chunk_bytes(chunk_bytes) : 0;
    return CRASS_OK;
}

int crass_hip_group_gzip_counters(const crass_hip_group *g, uint64_t out[6])
{
    if (!g || !out) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 6; k++) out[k] = g->GZ.cnt[k];
    return CRASS_OK;
}

int crass_hip_group_gzip_ms(const crass_hip_group *g, int rank, float out[7])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 6; k++) out[k] = (size_t)rank < g->GZ.ms.size() ? g->GZ.ms[rank][k] : 0.0f;
    out[6] = (size_t)rank < g->GZ.tail_ms.size() ? g->GZ.tail_ms[rank] : 0.0f;
    return CRASS_OK;
}

int crass_hip_group_name_exchange_ms(const crass_hip_group *g, int rank, float out[2])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    out[0] = g->nx[rank].wall_ms; out[1] = g->nx[rank].event_ms;
    return CRASS_OK;
}

int crass_hip_group_name_exchange_counters(const crass_hip_group *g, int rank, uint64_t out[4])
{
    if (!g || !out || rank < 0 || rank >= g->n) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) out[k] = g->nx[rank].cnt[k];
    return CRASS_OK;
}
int crass_hip_group_rccl_ranks(const crass_hip_group *g) { return g ? g->rccl_ranks : 0; }
crass_hip_ctx *crass_hip_group_ctx(crass_hip_group *g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->ctx[rank] : nullptr; }

int crass_hip_group_load_reads(crass_hip_group *g, const crass_reads *h)
{
    if (!g || !h) return CRASS_ERR_INVALID_ARG;
    if (h->n_reads && !h->packed) return CRASS_ERR_INVALID_ARG;
    if (!h->stride_words && h->n_reads && !h->word_off) return CRASS_ERR_INVALID_ARG;
    if (!h->uniform_len && h->n_reads && !h->lengths) return CRASS_ERR_INVALID_ARG;
    if (h->n_exceptions && (!h->exc_read || !h->exc_off || !h->exc_bytes)) return CRASS_ERR_INVALID_ARG;
    const int N = g->n;
    const uint64_t n = h->n_reads;
    g->loaded = g->have_p1 = g->have_merge = g->have_p2 = false;
    g->files_load = false;
    g->C.ready = g->M.ready = g->Q.ready = false;
    g->n_reads = n; g->base = h->read_index_base;
    g->first.assign(N + 1, 0);
    for (int r = 0; r <= N; r++) g->first[r] = n * (uint64_t)r / (uint64_t)N;
    g->shard.assign(N, crass_reads{});
    g->sh_word_off.assign(N, {}); g->sh_exc_read.assign(N, {}); g->sh_exc_off.assign(N, {}); g->sh_header_id.assign(N, {});
    for (auto &m : g->dup_local) m.clear();
    clear_extra(g);
    g->have_dups = false; g->hid_global.clear();
    // header ids that occur on more than one read (header_id[i] != i marks a repeat of read header_id[i]'s header)
    std::unordered_map<uint64_t, uint8_t> is_dup;
    if (h->header_id) {
        for (uint64_t i = 0; i < n; i++) if (h->header_id[i] != i) { if (h->header_id[i] > i) return CRASS_ERR_INVALID_ARG; is_dup[h->header_id[i]] = 1; }
        if (!is_dup.empty()) { g->have_dups = true; g->hid_global.assign(h->header_id, h->header_id + n); }
    }
    for (int r = 0; r < N; r++) {
        const uint64_t lo = g->first[r], hi = g->first[r + 1], m = hi - lo;
        crass_reads &s = g->shard[r];
        s.n_reads = m; s.stride_words = h->stride_words; s.uniform_len = h->uniform_len;
        s.read_index_base = h->read_index_base + lo;
        if (h->stride_words) s.packed = h->packed + lo * (uint64_t)h->stride_words;
        else if (m) {
            const uint64_t w0 = h->word_off[lo];
            std::vector<uint64_t> &wo = g->sh_word_off[r];
            wo.resize(m);
            for (uint64_t i = 0; i < m; i++) wo[i] = h->word_off[lo + i] - w0;
            s.packed = h->packed + w0; s.word_off = wo.data();
        } else s.packed = h->packed;
        if (!h->uniform_len) s.lengths = h->lengths + lo;
        if (h->n_exceptions) {
            const uint64_t *eb = std::lower_bound(h->exc_read, h->exc_read + h->n_exceptions, lo);
            const uint64_t *ee = std::lower_bound(h->exc_read, h->exc_read + h->n_exceptions, hi);
            const uint64_t e0 = (uint64_t)(eb - h->exc_read), ne = (uint64_t)(ee - eb);
            if (ne) {
                std::vector<uint64_t> &er = g->sh_exc_read[r], &eo = g->sh_exc_off[r];
                er.resize(ne); eo.resize(ne + 1);
                const uint64_t b0 = h->exc_off[e0];
                for (uint64_t i = 0; i < ne; i++) { er[i] = h->exc_read[e0 + i] - lo; eo[i] = h->exc_off[e0 + i] - b0; }
                eo[ne] = h->exc_off[e0 + ne] - b0;
                s.n_exceptions = ne; s.exc_read = er.data(); s.exc_off = eo.data(); s.exc_bytes = h->exc_bytes + b0;
            }
        }
        if (g->have_dups) {
            // local header ids: the first read OF THIS SHARD with the same header; headers that occur more than once anywhere
            // are remembered so that other shards' pass-1 hits can be marked here (collect_extra)
            std::vector<uint64_t> &hl = g->sh_header_id[r];
            hl.resize(m);
            std::unordered_map<uint64_t, uint64_t> &loc = g->dup_local[r];
            bool any_local_dup = false;
            for (uint64_t i = 0; i < m; i++) {
                const uint64_t gh = h->header_id[lo + i];
                if (gh == lo + i && !is_dup.count(gh)) { hl[i] = i; continue; }
                auto it = loc.find(gh);
                if (it == loc.end()) { loc.emplace(gh, i); hl[i] = i; }
                else { hl[i] = it->second; any_local_dup = true; }
            }
            if (any_local_dup) s.header_id = hl.data();
        }
    }
    // the exchange's row capacity from the largest shard (every rank must use the same one): the first step then neither
    // overflows nor repeats pass 1
    if (!g->cap_rows_forced) g->cap_rows = crass_hip_exchange_rows_for((n + (uint64_t)N - 1) / (uint64_t)N);
    const int st = dispatch(g, PH_LOAD);
    // (the shard views point into the caller's arrays: they are only used inside this call)
    g->sh_word_off.clear(); g->sh_exc_read.clear(); g->sh_exc_off.clear(); g->sh_header_id.clear();
    if (st) return st;
    g->loaded = true;
    return CRASS_OK;
}

static int run(crass_hip_group *g, unsigned phases)
{
    if (!g) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded) return CRASS_ERR_STATE;
    if ((phases & PH_MERGE) && !(phases & PH_SEED) && !g->have_p1) return CRASS_ERR_STATE;
    if ((phases & PH_RECRUIT) && !(phases & PH_MERGE) && !g->have_merge) return CRASS_ERR_STATE;
    g->C.ready = (phases & PH_SEED) ? false : g->C.ready;
    g->M.ready = false; g->Q.ready = false;
    if (phases & PH_SEED) g->have_p1 = g->have_merge = g->have_p2 = false;
    if (phases & PH_MERGE) { g->have_merge = g->have_p2 = false; g->C.ready = false; g->explicit_patterns = false; }      // (an overflow repeats pass 1)
    if (phases & PH_RECRUIT) g->have_p2 = false;
    const int s = dispatch(g, phases);
    if (s) return s;
    if (phases & PH_SEED) g->have_p1 = true;
    if (phases & PH_MERGE) g->have_merge = true;
    if (phases & PH_RECRUIT) g->have_p2 = true;
    return CRASS_OK;
}

// found headers named by the caller (job-level read indices) -> local read indices of every shard that holds the header
static int route_extra(crass_hip_group *g, const uint64_t *extra_found, uint64_t n_extra)
{
    for (auto &e : g->extra_user) e.clear();
    for (uint64_t k = 0; k < n_extra; k++) {
        const uint64_t i = extra_found[k];
        if (i >= g->n_reads) return CRASS_ERR_INVALID_ARG;
        const int r = (int)(std::upper_bound(g->first.begin(), g->first.end(), i) - g->first.begin()) - 1;
        bool routed = false;
        if (g->have_dups) {
            const uint64_t h = g->hid_global[i];
            for (int q = 0; q < g->n; q++) {
                auto it = g->dup_local[q].find(h);
                if (it != g->dup_local[q].end()) { g->extra_user[q].push_back(it->second); routed = routed || q == r; }
            }
        }
        if (!routed) g->extra_user[r].push_back(i - g->first[r]);
    }
    return CRASS_OK;
}

int crass_hip_group_seed_scan(crass_hip_group *g) { return run(g, PH_SEED); }
int crass_hip_group_merge(crass_hip_group *g) { return run(g, PH_MERGE); }
int crass_hip_group_recruit(crass_hip_group *g, const uint64_t *extra_found, uint64_t n_extra)
{
    if (!g || (n_extra && !extra_found)) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded) return CRASS_ERR_STATE;
    const int s = route_extra(g, extra_found, n_extra);
    if (s) return s;
    const int rs = run(g, PH_RECRUIT);
    for (auto &e : g->extra_user) e.clear();
    return rs;
}
int crass_hip_group_step(crass_hip_group *g)
{
    if (g) for (auto &e : g->extra_user) e.clear();
    return run(g, PH_SEED | PH_MERGE | PH_RECRUIT);
}

// an explicit pattern list on every rank (findSingletons' argument, libcrispr.h:86-92): the seam's form of pass 2, where
// createNonRedundantSet ran on the caller's side
int crass_hip_group_set_patterns(crass_hip_group *g, const char *const *patterns, const uint32_t *lengths, uint32_t n)
{
    if (!g || (n && (!patterns || !lengths))) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded) return CRASS_ERR_STATE;
    g->M.ready = g->Q.ready = false; g->have_p2 = false;
    for (int r = 0; r < g->n; r++) {
        const int s = crass_hip_set_patterns(g->ctx[r], patterns, lengths, n);
        if (s) return s;
    }
    clear_extra(g);                                     // (no device merge ran: cross-shard found headers come from the caller)
    g->have_merge = true; g->explicit_patterns = true;
    return CRASS_OK;
}

int crass_hip_group_get_candidates(crass_hip_group *g, crass_candidates *o)
{
    if (!g || !o) return CRASS_ERR_INVALID_ARG;
    if (!g->have_p1) return CRASS_ERR_STATE;
    auto &C = g->C;
    if (!C.ready) {
        C.read.clear(); C.ss_off.clear(); C.low.clear(); C.replen.clear(); C.nss.clear(); C.ss.clear(); C.dr_len.clear(); C.dr.clear();
        C.max_len = 0;
        for (int r = 0; r < g->n; r++) {
            crass_candidates c;
            const int s = crass_hip_get_candidates(g->ctx[r], &c);
            if (s) return s;
            C.stride = c.dr_stride; C.max_len = std::max(C.max_len, c.max_read_len);
            C.read.insert(C.read.end(), c.read_idx, c.read_idx + c.n);
            C.low.insert(C.low.end(), c.low_lexi, c.low_lexi + c.n);
            C.replen.insert(C.replen.end(), c.repeat_len, c.repeat_len + c.n);
            C.nss.insert(C.nss.end(), c.n_ss, c.n_ss + c.n);
            C.dr_len.insert(C.dr_len.end(), c.dr_len, c.dr_len + c.n);
            C.dr.insert(C.dr.end(), c.dr_chars, c.dr_chars + c.n * (size_t)c.dr_stride);
            for (uint64_t k = 0; k < c.n; k++) {                     // start/stops packed tightly
                C.ss_off.push_back(C.ss.size());
                C.ss.insert(C.ss.end(), c.ss_pool + c.ss_off[k], c.ss_pool + c.ss_off[k] + c.n_ss[k]);
            }
        }
        C.ready = true;
    }
    o->n = C.read.size(); o->read_idx = C.read.data(); o->low_lexi = C.low.data(); o->repeat_len = C.replen.data();
    o->n_ss = C.nss.data(); o->ss_off = C.ss_off.data(); o->ss_pool = C.ss.data(); o->dr_stride = C.stride;
    o->dr_len = C.dr_len.data(); o->dr_chars = C.dr.data(); o->max_read_len = C.max_len;
    return CRASS_OK;
}

// the text of reads of the whole job: every index goes to the rank whose shard holds it (a shard's read_index_base is the
// job's plus its first read, so the global indices pass through as they are), one crass_hip_fetch_text per rank that has any,
// and the records are put back in the caller's order
int crass_hip_group_fetch_text(crass_hip_group *g, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, crass_text *o)
{
    if (!g || !o || (n && !read_idx)) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded) return CRASS_ERR_STATE;
    for (uint64_t k = 0; k < n; k++) if (read_idx[k] < g->base || read_idx[k] - g->base >= g->n_reads) return CRASS_ERR_INVALID_ARG;
    try {
        std::vector<std::vector<uint64_t>> idx(g->n), at(g->n);
        std::vector<std::vector<uint8_t>> rc(g->n);
        for (uint64_t k = 0; k < n; k++) {
            const int r = (int)(std::upper_bound(g->first.begin(), g->first.end(), read_idx[k] - g->base) - g->first.begin()) - 1;
            idx[r].push_back(read_idx[k]); at[r].push_back(k);
            if (revcomp) rc[r].push_back(revcomp[k]);
        }
        // (a rank's result lives in its own context until that context's next fetch: all of them are there at once)
        std::vector<crass_text> part(g->n, crass_text{0, nullptr, nullptr});
        for (int r = 0; r < g->n; r++) {
            if (idx[r].empty()) continue;
            const int s = crass_hip_fetch_text(g->ctx[r], idx[r].data(), revcomp ? rc[r].data() : nullptr, idx[r].size(), &part[r]);
            if (s) return s;
        }
        auto &T = g->T;
        T.off.assign(n + 1, 0);
        for (int r = 0; r < g->n; r++) for (uint64_t q = 0; q < part[r].n; q++) T.off[at[r][q] + 1] = part[r].off[q + 1] - part[r].off[q];
        for (uint64_t k = 0; k < n; k++) T.off[k + 1] += T.off[k];
        T.chars.resize(T.off[n] + 1);
        for (int r = 0; r < g->n; r++) for (uint64_t q = 0; q < part[r].n; q++) {
            const uint64_t len = part[r].off[q + 1] - part[r].off[q];
            if (len) memcpy(T.chars.data() + T.off[at[r][q]], part[r].chars + part[r].off[q], len);
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    o->n = n; o->chars = g->T.chars.data(); o->off = g->T.off.data();
    return CRASS_OK;
}

// the files of a job as record-aligned shards, one per rank (include/crass_hip.h; the ranks' steps are load_files_rank's)
int crass_hip_group_load_fastx_files(crass_hip_group *g, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                                     const uint64_t *nominal, crass_fastx_shards *out)
{
    if (out) { memset(out, 0, sizeof(*out)); out->decline_file = -1; out->n_files = n_files; out->n_ranks = g ? (uint32_t)g->n : 0; }
    if (!g || !n_files || !bytes || !n_bytes || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (n_bytes[f] && !bytes[f]) return CRASS_ERR_INVALID_ARG;
    const int N = g->n;
    for (int k = 1; nominal && k + 1 < N; k++) if (nominal[k] < nominal[k - 1]) return CRASS_ERR_INVALID_ARG;
    g->loaded = g->have_p1 = g->have_merge = g->have_p2 = false;
    g->files_load = false;
    g->C.ready = g->M.ready = g->Q.ready = false;
    g->n_reads = 0; g->base = 0;
    g->first.assign(N + 1, 0);
    for (auto &m : g->dup_local) m.clear();
    clear_extra(g);
    g->have_dups = false; g->hid_global.clear();
    std::vector<crass_bgzf_index> ixs;
    struct FreeIx { std::vector<crass_bgzf_index> &v; ~FreeIx() { for (auto &x : v) crass_bgzf_index_free(&x); } } free_ix{ixs};
    int st = CRASS_OK;
    try {
        g->F = crass_hip_group::FilesJob();
        auto &J = g->F;
        g->names.assign(N, crass_hip_group::Text());
        ixs.assign(n_files, crass_bgzf_index{});
        // what every file is and how much text it holds (host: first bytes, BGZF index); the first file that cannot be taken
        // waits with its decline: a file in front of it may still offend in the scan
        J.files.assign(n_files, crass::ShardFile{});
        J.nf = n_files;
        for (uint64_t &x : g->GZ.cnt) x = 0;
        for (uint64_t &x : g->GZ.cnt_members) x = 0;
        g->GZ.files.clear(); g->GZ.ix.clear(); g->GZ.ix_zero.clear(); g->GZ.ix.reserve(n_files);
        g->GZ.v_gz = crass::ShardVerdict();
        g->GZ.ms.assign(N, std::array<float, 6>{}); g->GZ.up.assign(N, {}); g->GZ.tail_ms.assign(N, 0.0f); g->GZ.tail_el.assign(N, 0); g->GZ.crc_ms.assign(N, 0.0f);
        for (int r = 0; r < N; r++) { gzip_kept_release(g->ctx[r]); gzip_kept_report(g->ctx[r], nullptr, nullptr, true); }      // (what a failed load left)
        for (uint32_t f = 0; f < n_files; f++) {
            crass::ShardFile &F = J.files[f];
            F.bytes = bytes[f]; F.n_bytes = n_bytes[f];
            auto pend = [&](int32_t reason) { J.pend.file = (int32_t)f; J.pend.reason = reason; J.nf = f; };
            if (F.n_bytes >= 2 && F.bytes[0] == 0x1F && F.bytes[1] == 0x8B) {
                const int s = crass_bgzf_index_host(F.bytes, F.n_bytes, &ixs[f]);
                if (s == CRASS_ERR_UNSUPPORTED && g->gzip_mode && ixs[f].decline.reason == crass::BZ_NOT_BGZF) {
                    // plain gzip with the switch on, the index step: every rank finds and counts its share of the chunks, rank 0 walks
                    // the chain.  The text's size and the element index (start bit, end bit, text offset of every chain element) are
                    // known before any cut; the index takes a BGZF index's place, elements for members
                    auto &GJ = g->GZ;
                    GJ.files.emplace_back(new crass::GzRangesFile());
                    crass::GzRangesFile &Z = *GJ.files.back();
                    if (!gzip_file_init(Z, F.bytes, F.n_bytes, (uint32_t)N, g->gzip_chunk, g->gzip_mode == CRASS_GZIP_ON_DEVICE_MEMBERS)) { pend(0); J.pend.bgzf.reason = crass::BZ_NOT_GZIP; break; }
                    const int zs = gzip_job_run(g, Z, true, false);
                    if (zs) return zs;
                    if (GJ.status == CRASS_ERR_UNSUPPORTED) { pend(0); J.pend.bgzf.reason = GJ.v.reason; J.pend.bgzf.member = GJ.v.member; J.pend.bgzf.in_pos = GJ.v.in_pos; break; }
                    GJ.ix_zero.emplace_back(Z.n_chain + 1, 0);
                    crass_bgzf_index X{};
                    X.n_members = Z.n_chain; X.out_off = Z.off.data(); X.in_off = X.data_off = GJ.ix_zero.back().data();
                    GJ.ix.push_back(X);                     // (reserved for n_files: the pointers below stay)
                    F.ix = &GJ.ix.back(); F.gz = &Z; F.n_text = Z.n_text;
                    if (F.n_text == 0) { pend(crass::FX_EMPTY); break; }
                    continue;
                }
                if (s == CRASS_ERR_UNSUPPORTED) { pend(0); J.pend.bgzf = ixs[f].decline; break; }      // (plain gzip with the switch off: declined)
                if (s) return s;
                F.ix = &ixs[f]; F.n_text = ixs[f].out_off[ixs[f].n_members];
                if (F.n_text == 0) { pend(crass::FX_EMPTY); break; }
            } else {
                if (F.n_bytes == 0) { pend(crass::FX_EMPTY); break; }
                if (!crass::fx_is_hdr_char(F.bytes[0])) { pend(crass::FX_FIRST_BYTE); break; }
                F.n_text = F.n_bytes; F.format = F.bytes[0];
            }
        }
        const uint32_t nf = J.nf;
        J.tb.assign(nf + 1, 0);
        for (uint32_t f = 0; f < nf; f++) J.tb[f + 1] = J.tb[f] + J.files[f].n_text;
        const uint64_t T = J.tb[nf];
        if (nominal && nf == n_files) for (int k = 0; k + 1 < N; k++) if (nominal[k] > T) return CRASS_ERR_INVALID_ARG;
        J.nom_x.assign(N + 1, T);
        J.nom_x[0] = 0;
        for (int k = 1; k < N; k++) J.nom_x[k] = nominal ? std::min(nominal[k - 1], T) : (uint64_t)((unsigned __int128)T * (unsigned)k / (unsigned)N);
        J.nom.resize(N + 1);
        for (int k = 0; k <= N; k++) J.nom[k] = locate(J.tb, nf, J.nom_x[k]);
        J.pad_uniform = pad_uniform;
        J.pieces.assign(N, {}); J.v_stage.assign(N, crass::ShardVerdict()); J.v_scan.assign(N, crass::ShardVerdict());
        J.file_reads.assign(N, {}); J.n_reads.assign(N, 0); J.max_len.assign(N, 0);
        J.cut.assign(N + 1, crass::ShardPos{nf, 0});
        // the gzip files, now that the nominal cuts are known: every rank inflates the elements that hold its pieces (with the
        // byte in front of a piece, as a BGZF file's members are taken) in two halves with the composition of the entry windows
        // between them, and keeps their text on its device; rank 0 joins the CRC-32 parts.  The first file that does not inflate
        // waits with its decline as a rank's staging decline does; the files behind it are inflated all the same
        for (uint32_t f = 0; f < nf; f++) {
            if (!J.files[f].gz) continue;
            crass::GzRangesFile &Z = *const_cast<crass::GzRangesFile *>(J.files[f].gz);
            const uint64_t n = Z.n_chain;
            Z.e0.assign(N + 1, n); Z.e1.assign(N + 1, n); Z.first.assign(N + 1, 0);
            std::vector<uint8_t> holds(N + 1, 0);
            for (int r = 0; r < N; r++) {
                const crass::ShardPos lo = J.nom[r], hi = J.nom[r + 1];
                if (f < lo.file || f > hi.file) continue;
                const uint64_t a = f == lo.file ? lo.pos : 0, b = f == hi.file ? hi.pos : Z.n_text;
                if (a >= b) continue;
                crass::bgzf_members_for(Z.off.data(), n, a ? a - 1 : 0, b, &Z.e0[r], &Z.e1[r]);
                holds[r] = 1;
            }
            for (int r = N - 1; r >= 0; r--) if (!holds[r]) Z.e0[r] = Z.e1[r] = Z.e0[r + 1];      // (passes the window on to the next rank that holds some)
            for (int r = 0; r < N; r++) Z.first[r + 1] = std::max(Z.first[r], Z.e1[r]);
            const int zs = gzip_job_run(g, Z, false, true);
            if (zs) return zs;
            uint64_t bad = ~0ull;
            for (int r = 0; r < N; r++) { bad = std::min(bad, Z.bad[r]); g->GZ.cnt[3] += Z.e1[r] - Z.e0[r]; }
            g->GZ.cnt[0] += 1; g->GZ.cnt[1] += Z.M.G.nc; g->GZ.cnt[2] += n; g->GZ.cnt[3] -= n;
            uint32_t crc = 0;
            for (uint64_t i = 0; i < n; i++) crc = crass::gz_crc_join(crc, Z.crc_part[i], Z.off[i + 1] - Z.off[i]);
            crass::ShardVerdict sv;
            sv.file = (int32_t)f;
            if (bad != ~0ull) { const uint64_t k = Z.chain[bad]; sv.bgzf.reason = crass::BZ_MARKER; sv.bgzf.member = k; sv.bgzf.in_pos = Z.M.G.d_off + (Z.start[k] >> 3); }
            else if (Z.members) {
                // members mode: the member verdict (7 / 8 / 9 with the member and the file byte of its header) is the file's
                if (!Z.table_ok) return CRASS_ERR_STATE;
                g->GZ.cnt_members[0] += 1; g->GZ.cnt_members[1] += Z.in_off.size() - 1; g->GZ.cnt_members[2] += Z.n_pieces; g->GZ.cnt_members[3] += Z.exported_plain;
                crass::GzVerdict mv{};
                if (gzip_members_verdict(Z, &mv) != crass::BZ_OK) { sv.bgzf.reason = mv.reason; sv.bgzf.member = mv.member; sv.bgzf.in_pos = mv.in_pos; }
            }
            else if (crc != Z.M.crc) sv.bgzf.reason = crass::BZ_CRC;
            if (sv.bgzf.reason && crass::shard_verdict_before(sv, g->GZ.v_gz)) g->GZ.v_gz = sv;
        }
        J.pend0 = J.pend;
        for (uint64_t &x : g->load_cnt) x = 0;
        st = dispatch(g, PH_LOAD_FILES);
        // the gzip counters of the load: the elements the seeded walks added count as inflated by a further rank; the uploads
        // are ranges of host addresses, so bytes of different files never count as the same
        if (!g->GZ.files.empty()) {
            std::vector<std::pair<uint64_t, uint64_t>> all;
            uint64_t sent = 0, distinct = 0, reach = 0;
            for (int r = 0; r < N; r++) {
                g->GZ.cnt[3] += g->GZ.tail_el[r];
                for (const auto &u : g->GZ.up[r]) { sent += u.second - u.first; all.push_back(u); }
            }
            std::sort(all.begin(), all.end());
            for (const auto &u : all) { if (u.second > reach) { distinct += u.second - std::max(u.first, reach); reach = u.second; } }
            g->GZ.cnt[4] = sent; g->GZ.cnt[5] = sent - distinct;
        }
        g->load_cnt[0] = (uint64_t)J.attempts; g->load_cnt[1] = J.wrapped_pass ? J.n_chained : 0;
        for (int r = 0; J.wrapped_pass && r < N; r++) {
            uint64_t lk = 0, db = 0;
            shard_cut_counters(g->ctx[r], &lk, &db, nullptr);
            g->load_cnt[2] += db; g->load_cnt[3] += lk;
        }
        for (auto &F : J.files) { F.ix = nullptr; F.gz = nullptr; F.bytes = nullptr; }      // (the caller's bytes and this call's indexes: used inside this call only)
        if (st) return st;
        if (J.declined) {
            if (out) { out->decline_file = J.verdict.file; out->decline_reason = J.verdict.reason; out->decline_pos = J.verdict.pos; out->bgzf = J.verdict.bgzf; }
            return CRASS_ERR_UNSUPPORTED;
        }
        g->first = J.rank_base; g->n_reads = J.rank_base[N];
        auto &S = g->S;
        S.cut_file.assign(N + 1, 0); S.cut_pos.assign(N + 1, 0); S.file_read_base.assign(n_files + 1, 0); S.format.assign(n_files, 0);
        for (int k = 0; k <= N; k++) { S.cut_file[k] = J.cut[k].file; S.cut_pos[k] = J.cut[k].pos; }
        for (int r = 0; r < N; r++) for (const auto &fr : J.file_reads[r]) S.file_read_base[fr.first + 1] += fr.second;
        for (uint32_t f = 0; f < n_files; f++) { S.file_read_base[f + 1] += S.file_read_base[f]; S.format[f] = J.files[f].format; }
        uint32_t max_len = 0;
        for (int r = 0; r < N; r++) max_len = std::max(max_len, J.max_len[r]);
        if (out) {
            out->n_reads = g->n_reads; out->max_len = max_len;
            out->rank_read_base = g->first.data(); out->cut_file = S.cut_file.data(); out->cut_pos = S.cut_pos.data();
            out->file_read_base = S.file_read_base.data(); out->format = S.format.data();
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    g->loaded = true; g->files_load = true; g->CM.ready = false;
    return CRASS_OK;
}

// header lines (quality == false) or quality strings of reads of the whole job: routed like crass_hip_group_fetch_text, each
// rank fetches from its own arena, the records are put back in the caller's order
static int group_fetch_lines(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, bool quality, crass_text *o, uint32_t *name_len_out,
                             uint8_t *has_qual_out)
{
    if (!g || !o || (n && !read_idx)) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded || !g->files_load) return CRASS_ERR_STATE;
    for (uint64_t k = 0; k < n; k++) if (read_idx[k] >= g->n_reads) return CRASS_ERR_INVALID_ARG;
    crass_hip_group::Text &T = quality ? g->TQ : g->TH;
    try {
        std::vector<std::vector<uint64_t>> idx(g->n), at(g->n);
        for (uint64_t k = 0; k < n; k++) {
            const int r = (int)(std::upper_bound(g->first.begin(), g->first.end(), read_idx[k]) - g->first.begin()) - 1;
            idx[r].push_back(read_idx[k] - g->first[r]); at[r].push_back(k);
        }
        // (a rank's result lives in its own context until that context's next fetch of the kind: all of them are there at once)
        std::vector<crass_text> part(g->n, crass_text{0, nullptr, nullptr});
        std::vector<uint32_t> nl;
        std::vector<uint8_t> hq;
        for (int r = 0; r < g->n; r++) {
            const uint64_t m = idx[r].size();
            if (!m) continue;
            const uint8_t *arena = nullptr; const uint64_t *rec_pos = nullptr; uint64_t nb = 0, nr = 0;
            int s = shard_records(g->ctx[r], &arena, &nb, &rec_pos, &nr);
            if (s) return s;
            nl.resize(m); hq.resize(m);
            s = quality ? crass_hip_fetch_quality_device(g->ctx[r], arena, nb, rec_pos, nr, idx[r].data(), m, &part[r], hq.data())
                        : crass_hip_fetch_header_lines_device(g->ctx[r], arena, nb, rec_pos, nr, idx[r].data(), m, &part[r], nl.data());
            if (s) return s;
            for (uint64_t q = 0; q < m; q++) {
                if (quality && has_qual_out) has_qual_out[at[r][q]] = hq[q];
                if (!quality && name_len_out) name_len_out[at[r][q]] = nl[q];
            }
        }
        T.off.assign(n + 1, 0);
        for (int r = 0; r < g->n; r++) for (uint64_t q = 0; q < part[r].n; q++) T.off[at[r][q] + 1] = part[r].off[q + 1] - part[r].off[q];
        for (uint64_t k = 0; k < n; k++) T.off[k + 1] += T.off[k];
        T.chars.resize(T.off[n] + 1);
        for (int r = 0; r < g->n; r++) for (uint64_t q = 0; q < part[r].n; q++) {
            const uint64_t len = part[r].off[q + 1] - part[r].off[q];
            if (len) memcpy(T.chars.data() + T.off[at[r][q]], part[r].chars + part[r].off[q], len);
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    o->n = n; o->chars = T.chars.data(); o->off = T.off.data();
    return CRASS_OK;
}

int crass_hip_group_fetch_header_lines(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint32_t *name_len_out)
{
    return group_fetch_lines(g, read_idx, n, false, out, name_len_out, nullptr);
}

int crass_hip_group_fetch_quality(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint8_t *has_qual_out)
{
    return group_fetch_lines(g, read_idx, n, true, out, nullptr, has_qual_out);
}

// what the cuts of a files load carry (include/crass_hip.h): rank after rank in file order, each rank "publishes" the comment handed
// to its LAST record — the own comment of the last own-comment record of the file part its shard ends in, a host string — and
// is handed what the ranks in front of it left for the file its shard begins in.  Empty ranks, and ranks that are one part of
// one file without a comment, pass it through; nothing crosses a file boundary.
static int group_comments_resolve(crass_hip_group *g)
{
    auto &J = g->F;
    auto &CM = g->CM;
    const int N = g->n;
    CM.in.assign(N, std::string()); CM.has.assign(N, 0); CM.first_n.assign(N, 0);
    bool carried = false; std::string text; int64_t file = -1;      // what the ranks so far leave, and for which file
    for (int r = 0; r < N; r++) {
        const uint64_t nr = g->first[r + 1] - g->first[r];
        if (!nr) continue;
        int64_t f0 = -1, fl = -1; size_t parts = 0;
        for (const auto &fr : J.file_reads[r]) if (fr.second) { if (f0 < 0) { f0 = fr.first; CM.first_n[r] = fr.second; } fl = fr.first; parts++; }
        if (carried && file == f0) { CM.in[r] = text; CM.has[r] = 1; }
        const uint64_t last = nr - 1;
        crass_text t; uint8_t has = 0;
        const int s = crass_hip_fetch_comments_device(g->ctx[r], &last, 1, &t, &has);
        if (s) return s;
        if (has) { carried = true; text.assign((const char *)t.chars + t.off[0], (size_t)(t.off[1] - t.off[0])); }
        else if (!(parts == 1 && file == f0)) { carried = false; text.clear(); }      // (else: one part of the file the carry belongs to)
        file = fl;
    }
    CM.ready = true;
    return CRASS_OK;
}

int crass_hip_group_fetch_comments(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *o, uint8_t *has_out)
{
    if (!g || !o || (n && !read_idx)) return CRASS_ERR_INVALID_ARG;
    if (!g->loaded || !g->files_load) return CRASS_ERR_STATE;
    for (uint64_t k = 0; k < n; k++) if (read_idx[k] >= g->n_reads) return CRASS_ERR_INVALID_ARG;
    crass_hip_group::Text &T = g->TC;
    try {
        if (!g->CM.ready) { const int rs = group_comments_resolve(g); if (rs) return rs; }
        std::vector<std::vector<uint64_t>> idx(g->n), at(g->n);
        for (uint64_t k = 0; k < n; k++) {
            const int r = (int)(std::upper_bound(g->first.begin(), g->first.end(), read_idx[k]) - g->first.begin()) - 1;
            idx[r].push_back(read_idx[k] - g->first[r]); at[r].push_back(k);
        }
        // (a rank's result lives in its own context until that context's next fetch of the kind: all of them are there at once)
        std::vector<crass_text> part(g->n, crass_text{0, nullptr, nullptr});
        std::vector<std::vector<uint8_t>> hc(g->n);     // 0: nothing handed, 1: the rank's own text, 2: the carried string
        T.off.assign(n + 1, 0);
        for (int r = 0; r < g->n; r++) {
            const uint64_t m = idx[r].size();
            if (!m) continue;
            hc[r].assign(m, 0);
            const int s = crass_hip_fetch_comments_device(g->ctx[r], idx[r].data(), m, &part[r], hc[r].data());
            if (s) return s;
            for (uint64_t q = 0; q < m; q++) {
                if (!hc[r][q] && g->CM.has[r] && idx[r][q] < g->CM.first_n[r]) hc[r][q] = 2;
                T.off[at[r][q] + 1] = hc[r][q] == 2 ? g->CM.in[r].size() : part[r].off[q + 1] - part[r].off[q];
                if (has_out) has_out[at[r][q]] = hc[r][q] ? 1 : 0;
            }
        }
        for (uint64_t k = 0; k < n; k++) T.off[k + 1] += T.off[k];
        T.chars.resize(T.off[n] + 1);
        for (int r = 0; r < g->n; r++) for (uint64_t q = 0; q < part[r].n; q++) {
            const uint64_t len = T.off[at[r][q] + 1] - T.off[at[r][q]];
            if (len) memcpy(T.chars.data() + T.off[at[r][q]], hc[r][q] == 2 ? (const uint8_t *)g->CM.in[r].data() : part[r].chars + part[r].off[q], len);
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    o->n = n; o->chars = T.chars.data(); o->off = T.off.data();
    return CRASS_OK;
}

int crass_hip_group_get_merge(crass_hip_group *g, crass_merge_view *o)
{
    if (!g || !o) return CRASS_ERR_INVALID_ARG;
    if (!g->have_merge || g->explicit_patterns) return CRASS_ERR_STATE;
    int s = crass_hip_get_merge(g->ctx[0], o);
    if (s) return s;
    if (g->n == 1) return CRASS_OK;
    if (!g->M.ready) {
        g->M.cand_token.assign(o->cand_token, o->cand_token + o->n_candidates);
        for (int r = 1; r < g->n; r++) {
            crass_merge_view v;
            s = crass_hip_get_merge(g->ctx[r], &v);
            if (s) return s;
            g->M.cand_token.insert(g->M.cand_token.end(), v.cand_token, v.cand_token + v.n_candidates);
        }
        g->M.ready = true;
    }
    o->n_candidates = g->M.cand_token.size(); o->cand_token = g->M.cand_token.data();
    return CRASS_OK;
}

int crass_hip_group_get_recruits(crass_hip_group *g, crass_recruits *o)
{
    if (!g || !o) return CRASS_ERR_INVALID_ARG;
    if (!g->have_p2) return CRASS_ERR_STATE;
    auto &Q = g->Q;
    if (!Q.ready) {
        crass_merge_view mv{};
        int s = g->explicit_patterns ? CRASS_OK : crass_hip_get_merge(g->ctx[0], &mv);     // (explicit patterns: the host sink filled the strings)
        if (s) return s;
        Q.read.clear(); Q.low.clear(); Q.start.clear(); Q.end.clear(); Q.token.clear(); Q.dr_len.clear(); Q.dr.clear();
        for (int r = 0; r < g->n; r++) {
            crass_recruits q;
            s = crass_hip_get_recruits(g->ctx[r], &q);
            if (s) return s;
            Q.stride = q.dr_stride;
            const size_t base = Q.read.size();
            Q.read.insert(Q.read.end(), q.read_idx, q.read_idx + q.n);
            Q.low.insert(Q.low.end(), q.low_lexi, q.low_lexi + q.n);
            Q.start.insert(Q.start.end(), q.start, q.start + q.n);
            Q.end.insert(Q.end.end(), q.end, q.end + q.n);
            Q.token.insert(Q.token.end(), q.token, q.token + q.n);
            Q.dr_len.insert(Q.dr_len.end(), q.dr_len, q.dr_len + q.n);
            Q.dr.insert(Q.dr.end(), q.dr_chars, q.dr_chars + q.n * (size_t)q.dr_stride);
            // a recruit's DR string is its token's string: ranks with the light host view left it empty
            for (uint64_t k = 0; k < q.n; k++) {
                const uint32_t t = q.token[k];
                if (t >= 2 && t - 2 < mv.n_tokens) {
                    const uint64_t a = mv.tok_off[t - 2], len = mv.tok_off[t - 1] - a;
                    if (len <= q.dr_stride) memcpy(Q.dr.data() + (base + k) * (size_t)q.dr_stride, mv.tok_chars + a, len);
                }
            }
        }
        Q.ready = true;
    }
    o->n = Q.read.size(); o->read_idx = Q.read.data(); o->low_lexi = Q.low.data(); o->start = Q.start.data(); o->end = Q.end.data();
    o->dr_stride = Q.stride; o->dr_len = Q.dr_len.data(); o->dr_chars = Q.dr.data(); o->token = Q.token.data();
    return CRASS_OK;
}

} // extern "C"

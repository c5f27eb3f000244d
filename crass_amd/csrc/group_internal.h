// group_internal.h — the group behind crass_hip_group_* of include/crass_hip.h and what crosses the host files that implement
// it: group.cpp (create / destroy, the helper threads and a job's dispatch, the exchange, the reads load, the steps, the
// concatenating getters), group_files.cpp (a files load: record-aligned shards), group_gzip.cpp (one plain gzip file inflated
// across the ranks, and such files inside a files load), group_names.cpp (the found-name exchange, both routes) and
// group_fetch.cpp (text, header lines, quality and comments of reads of the whole job).  Host only.
#pragma once
#include "../../include/crass_hip.h"

#include <hip/hip_runtime.h>
#include "devmem.h"
#include "fastx_shards.h"
#include "gunzip_launch.h"
#include "gunzip_ranges.h"
#include "group_route.h"
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

// (what used to be file-local in group.cpp stays out of the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace grp {

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

} // namespace grp

struct crass_hip_group {
    // ---- the ranks: contexts, communicators, the exchange's buffers (group.cpp) ----
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
    // ---- a job and its threads (group.cpp): helper threads are ranks 1 .. n-1; the caller's thread is rank 0 ----
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv, cv_done;
    uint64_t job_id = 0;
    unsigned job_phases = 0;
    bool quit = false;
    std::atomic<int> done{0};
    grp::Barrier *bar = nullptr;
    std::vector<int> status;                    // per rank, of the current job
    std::atomic<int> failed{0};                 // some rank failed: the others skip their work but still meet at the barriers
    std::atomic<uint64_t> need_rows{0};
    // ---- sharding, and what the steps have reached (group.cpp) ----
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
    // ---- the concatenated hand-off (group.cpp's getters) ----
    struct {
        std::vector<uint64_t> read, ss_off; std::vector<uint8_t> low; std::vector<uint32_t> replen, nss, ss; std::vector<uint16_t> dr_len;
        std::vector<char> dr; uint32_t stride = 0, max_len = 0; bool ready = false;
    } C;
    struct { std::vector<uint32_t> cand_token; bool ready = false; } M;
    struct {
        std::vector<uint64_t> read; std::vector<uint8_t> low; std::vector<uint32_t> start, end, token; std::vector<uint16_t> dr_len;
        std::vector<char> dr; uint32_t stride = 0; bool ready = false;
    } Q;
    // ---- the fetches of the whole job (group_fetch.cpp) ----
    using Text = grp::Text;
    Text T;                                     // crass_hip_group_fetch_text's result
    Text TH, TQ;                                // crass_hip_group_fetch_header_lines' and crass_hip_group_fetch_quality's
    // crass_hip_group_fetch_comments: its result, and what a files load's cuts carry — in[r] / has[r]: the comment handed to the
    // records of rank r's FIRST file part that have no source in that part (the own comment of the last own-comment record of
    // the same file on an earlier rank), first_n[r]: the records of that part; resolved at the first fetch after the load
    Text TC;
    struct { std::vector<std::string> in; std::vector<uint8_t> has; std::vector<uint64_t> first_n; bool ready = false; } CM;
    // ---- a files load (group_files.cpp; crass_hip_group_load_fastx_files, fastx_shards.h): what the ranks share between its
    // barriers.  Rank r writes entry r of the per-rank vectors, rank 0 combines between two barriers, everybody reads behind
    // the second ----
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
    int fastq_class = 0;                        // crass_hip_group_set_fastq_class, CRASS_DEVICE_FASTQ at creation
    uint64_t shard_margin = 256u << 10;         // what a wrapped-mode piece stages behind its end at first (CRASS_SHARD_MARGIN at creation)
    uint64_t load_cnt[4] = {0, 0, 0, 0};        // crass_hip_group_load_counters
    struct { std::vector<uint64_t> cut_pos, file_read_base; std::vector<uint32_t> cut_file; std::vector<int32_t> format; } S;      // crass_fastx_shards' arrays
    // ---- a gzip job (group_gzip.cpp; crass_hip_group_inflate_gzip, gunzip_ranges.h): the file's state, which the ranks fill
    // between barriers; where the text goes; what rank 0 decided behind the count step (go on, or the call's status); the last
    // call's counters and times ----
    struct GzipJob {
        crass::GzRangesFile Z;                  // crass_hip_group_inflate_gzip's file
        crass::GzRangesFile *zp = nullptr;      // the file of the running job: &Z, or one of a files load's
        // the steps of the running job: a files load indexes every gzip file first (find, count, chain: the text's size and the
        // element index, before any cut) and inflates it once the nominal cuts are known, each rank the elements of its pieces,
        // their text kept on its device (out NULL)
        bool do_index = true, do_inflate = true;
        std::vector<std::unique_ptr<crass::GzRangesFile>> files;      // a files load's, until the next load
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
    // ---- found headers across the ranks of a files load (group_names.cpp): the names of every rank's pass-1 records, for the
    // other ranks to look up ----
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
};

namespace grp {

// ---- group.cpp ----
void set_error(const std::string &s);           // crass_hip_group_last_error's text
void note(crass_hip_group *g, int r, int s);    // rank r's status of the running job: the first one stays, any one fails the job
int dispatch(crass_hip_group *g, unsigned phases);      // one job on every rank; the first rank's status that is not CRASS_OK
int setup_exchange(crass_hip_group *g, int r);
// what a load clears before anything else: no reads, no step's result, no shard, no namesakes
void reset_for_load(crass_hip_group *g, uint64_t n_reads, uint64_t base);

inline bool job_ok(const crass_hip_group *g) { return g->failed.load(std::memory_order_acquire) == 0; }
// a rank's step that may allocate, run if nobody has failed: its status is noted, a bad_alloc is this rank's CRASS_ERR_OOM ...
template <typename F> void rank_step(crass_hip_group *g, int r, F f)
{
    if (!job_ok(g)) return;
    try { note(g, r, f()); } catch (const std::bad_alloc &) { note(g, r, CRASS_ERR_OOM); }
}
// ... and rank 0's step between two barriers, which every rank passes whatever happens
template <typename F> void rank0_step(crass_hip_group *g, int r, F f) { if (r == 0) rank_step(g, 0, f); }

// ---- group_files.cpp ----
void load_files_rank(crass_hip_group *g, int r);        // one rank's part of a PH_LOAD_FILES job

// ---- group_gzip.cpp ----
void gzip_inflate_rank(crass_hip_group *g, int r);      // one rank's part of a PH_INFLATE_GZIP job
// a file's state before the index step: the header and the trailer parsed (false: not a gzip member), the per-chunk arrays empty
bool gzip_file_init(crass::GzRangesFile &Z, const uint8_t *bytes, uint64_t n_bytes, uint32_t n_ranks, uint64_t chunk_bytes, bool members);
// a gzip job on a file: both steps with the text to out (crass_hip_group_inflate_gzip), or a step of a files load on one of its
// gzip files: the index step, or — its ranges set — the inflate step whose text the ranks keep
int gzip_job_run(crass_hip_group *g, crass::GzRangesFile &Z, bool index, bool inflate, uint8_t *out = nullptr, uint64_t out_cap = 0, const uint64_t *nominal = nullptr);
// a call's start: the per-rank times and upload lists empty, on the group and in the contexts
void gzip_reset_reports(crass_hip_group *g);
// an inflated file's part of GZ.cnt[0 .. 3] (files, chunks, elements, elements held by a further rank) and, where its member
// table was judged, of GZ.cnt_members; GZ.cnt[4 .. 5] from the ranks' upload lists: bytes uploaded, and those some upload had
// brought already (ranges of host addresses, so bytes of different files never count as the same)
void gzip_count_file(crass_hip_group *g, const crass::GzRangesFile &Z);
void gzip_count_uploads(crass_hip_group *g);
// the verdict of an inflated file in the host rule's order: the smallest unresolved marker over the ranks (14), then in members
// mode the first offending member (7 / 8 before 9; CRASS_ERR_STATE: no member table), else the joined CRC-32.  v->reason 0: none
int gzip_file_verdict(const crass::GzRangesFile &Z, crass::GzVerdict *v);

// ---- group_names.cpp ----
void names_exchange_rank(crass_hip_group *g, int r);    // behind a merge on a files load: publish, barrier, lookup
void nx_free(crass_hip_group *g, int r);
void clear_extra(crass_hip_group *g);           // no list of namesakes is left for pass 2, on either route (a load, an explicit pattern set)

} // namespace grp
#pragma GCC visibility pop

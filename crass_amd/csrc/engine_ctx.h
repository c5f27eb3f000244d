// engine_ctx.h — the context behind include/crass_hip.h and what its members are made of, shared by the host files that
// implement the ABI: engine.cpp (create / destroy, what every load ends with, pattern install, Levenshtein, counters),
// engine_pass1.cpp (the seed scan and its sinks), engine_merge.cpp (the merge on the device and on the host, the exchange),
// engine_pass2.cpp (set_patterns, recruit) and the device ingest: engine_ingest.cpp (load / attach, fetch text, the scratch
// given back), engine_fastx.cpp (FASTA / FASTQ scan), engine_inflate.cpp (BGZF and gzip inflate), engine_names.cpp (header ids,
// names, header lines, quality), engine_shards.cpp (a group's file shards).  What crosses these files is declared at the end;
// what crosses the ingest's five among themselves, in ingest_internal.h.
// Host only: no .hip file includes this.
#pragma once
#include "../../include/crass_hip.h"
#include "engine_internal.h"
#include "merge.h"
#include "fastx_launch.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

// (what used to be file-local in engine.cpp stays out of the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace crass {

inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One helper thread per context: rebuilds the host view of a device-side merge while the calling thread keeps
// the device fed (pass 2).  submit() hands over one job; wait() returns when it has finished.
class HostWorker {
public:
    ~HostWorker() { stop(); }
    void submit(std::function<void()> job)
    {
        wait();
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!started_) { th_ = std::thread([this] { loop(); }); started_ = true; }
            job_ = std::move(job); busy_ = true;
        }
        cv_.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return !busy_; });
    }
    // The caller is about to wait for the job: if the helper has not even picked it up yet (its wake-up is normally
    // ~50 us, but on a busy or CPU-limited host it was seen to take 4-14 ms — every slow step of tools/step_spikes.py was
    // this wait), the caller runs the job itself instead.  Returns false when the helper has it (then: wait()).
    bool run_here_if_not_started()
    {
        std::function<void()> job;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!(busy_ && job_)) return false;
            job = std::move(job_); job_ = nullptr;          // the helper's wait predicate (busy_ && job_) stays false: it sleeps on
        }
        try { job(); } catch (...) { failed_.store(true, std::memory_order_relaxed); }      // (the job records its own status; this only keeps busy_ honest)
        { std::lock_guard<std::mutex> lk(m_); busy_ = false; }
        cv_.notify_all();
        return true;
    }
    bool take_failed() { return failed_.exchange(false, std::memory_order_relaxed); }
    void stop()
    {
        if (!started_) return;
        wait();
        { std::lock_guard<std::mutex> lk(m_); quit_ = true; }
        cv_.notify_all();
        th_.join();
        started_ = false;
    }
private:
    void loop()
    {
        for (;;) {
            std::function<void()> job;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return quit_ || (busy_ && job_); });
                if (quit_) return;
                job = std::move(job_); job_ = nullptr;
            }
            try { job(); } catch (...) { failed_.store(true, std::memory_order_relaxed); }
            { std::lock_guard<std::mutex> lk(m_); busy_ = false; }
            cv_.notify_all();
        }
    }
    std::atomic<bool> failed_{false};
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool busy_ = false, quit_ = false, started_ = false;
};

// std::allocator whose resize() leaves trivially constructible elements uninitialised
template <typename T> struct NoInitAlloc : std::allocator<T> {
    template <typename U> struct rebind { typedef NoInitAlloc<U> other; };
    NoInitAlloc() = default;
    template <typename U> NoInitAlloc(const NoInitAlloc<U> &) {}
    template <typename U, typename... A> void construct(U *p, A &&...a)
    {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U;
        else ::new ((void *)p) U(std::forward<A>(a)...);
    }
};

// device allocations of this library, and an optional cap on them (tests: CRASS_POOL_CAP_MB makes an allocation beyond the
// cap fail with hipErrorOutOfMemory, so the error paths can be exercised without exhausting a 288 GB device)
inline std::atomic<uint64_t> g_dev_bytes{0};      // (inline variables: one definition for every file that includes this)
inline std::atomic<uint64_t> g_dev_cap{0};

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t want)
    {
        if (want <= n && p) return hipSuccess;
        release();
        if (want == 0) want = 1;
        const uint64_t cap = g_dev_cap.load(std::memory_order_relaxed);
        if (cap && g_dev_bytes.load(std::memory_order_relaxed) + want * sizeof(T) > cap) return hipErrorOutOfMemory;
        hipError_t e = crass::dev_alloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess) { n = want; g_dev_bytes.fetch_add(want * sizeof(T), std::memory_order_relaxed); }
        else p = nullptr;
        return e;
    }
    void release()
    {
        if (p) { crass::dev_free(p); g_dev_bytes.fetch_sub(n * sizeof(T), std::memory_order_relaxed); }
        p = nullptr; n = 0;
    }
};

template <typename T> struct PinBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t want)
    {
        if (want <= n && p) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
        if (want == 0) want = 1;
        hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
};

// The HIP-event times of one ingest stage.  begin() switches the timer on for this call only when the caller's timing level
// asks for it (else nothing is created and nothing recorded, as crass_hip_set_stage_timing promises) and records the stage's
// first mark, mark() the next one, elapsed() reads a span once the stream has been waited for (untimed: *ms stays as it is).
// The events are created on first use and go with destroy().
template <int N> struct StageTimer {
    hipEvent_t ev[N] = {};
    bool on = false;
    int at = 0;
    // first: the mark this part of the stage starts at (the gzip decode step goes on from the count step's last mark)
    hipError_t begin(bool timed, hipStream_t s, int first = 0) { on = timed; at = first; return mark(s); }
    hipError_t mark(hipStream_t s)
    {
        if (!on) return hipSuccess;
        if (at >= N) return hipErrorInvalidValue;
        if (!ev[at]) { const hipError_t e = hipEventCreate(&ev[at]); if (e != hipSuccess) return e; }
        return hipEventRecord(ev[at++], s);
    }
    hipError_t elapsed(int a, int b, float *ms) const { return on ? hipEventElapsedTime(ms, ev[a], ev[b]) : hipSuccess; }
    void destroy() { for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } on = false; }
};

// crass_hip_fetch_header_lines_device / crass_hip_fetch_quality_device: one word per record (a header line's first byte) or two
// (a record's position and end) and, for the quality, the lines' starts; the lengths (then the name lengths / the flags),
// offsets and the text on the device — given back before the call returns — and their pinned host sides, which stay: h_off and
// h_chars are what crass_text points at.  Each of the two results has pinned memory of its own.
struct LineFetch {
    DevBuf<uint64_t> src, start, off; DevBuf<uint32_t> len; DevBuf<uint8_t> chars;
    PinBuf<uint64_t> h_src, h_off; PinBuf<uint32_t> h_len; PinBuf<uint8_t> h_chars;
    void release_device() { src.release(); start.release(); off.release(); len.release(); chars.release(); }
    void free_all() { release_device(); h_src.release(); h_off.release(); h_len.release(); h_chars.release(); }
};

// ---- device ingest: everything the load / inflate / names / fetch calls keep in the context (engine_ingest.cpp, engine_fastx.cpp,
// engine_inflate.cpp, engine_names.cpp, engine_shards.cpp).  Each stage's device scratch goes back through ONE function of
// engine_ingest.cpp (release_*, declared in ingest_internal.h); ingest_free_all is made of those plus what is kept.
struct Ingest {
    // crass_hip_load_text / crass_hip_attach_device_text: the text's offsets on the device (lengths that differ), the two
    // staged chunks of a host text (pinned source of the copy, device destination) and the events that order their reuse
    DevBuf<uint64_t> t_off; DevBuf<uint8_t> t_dev[2]; PinBuf<uint8_t> t_pin[2];
    hipEvent_t ev_t_copy[2] = {nullptr, nullptr}, ev_t_pack[2] = {nullptr, nullptr};
    StageTimer<2> tm_pack;
    float last_pack_ms = 0;                  // HIP-event time of the last call's pack kernels (stage timing >= 1, else 0)
    // crass_hip_load_fastx_bytes / crass_hip_attach_device_fastx (fastx_scan.hip): the raw bytes of a host file, the tile arrays,
    // the totals ([0..4), then the verdict word), the reads' text and the two per-record arrays — all given back before the call
    // returns; the pinned copies crass_fastx_layout points at stay until the next such call or destroy
    DevBuf<uint8_t> x_raw, x_text; DevBuf<FxTile> x_tiles; DevBuf<FxBase> x_base; DevBuf<uint64_t> x_tot, x_rec_pos, x_seq_off;
    PinBuf<uint64_t> x_h_tot, x_h_rec_pos, x_h_seq_off;
    StageTimer<2> tm_scan;
    float last_scan_ms = 0;                  // HIP-event time of the last call's scan kernels (stage timing >= 1, else 0)
    // crass_hip_set_fastq_class (fastx_wrapped.hip): the class, the pieces the last load's four-line / wrapped scan decided, one
    // scratch buffer per wrapped piece (fw_scratch_words) — given back with the scan's — and the pinned copy of their totals
    int fastq_class = 0;
    uint64_t scan_classes[2] = {0, 0};
    std::vector<DevBuf<uint64_t>> w_scratch;
    PinBuf<uint64_t> x_h_wtot;
    // crass_hip_inflate_bgzf_device / crass_hip_load_fastx_bgzf (inflate.hip): the index's three arrays back to back, every
    // member's reason, the verdict word (the gzip decode step's too), the compressed bytes of a host file and the text that is
    // not the caller's — all given back before the call returns
    DevBuf<uint64_t> z_idx; DevBuf<uint32_t> z_reason; DevBuf<unsigned long long> z_verdict; DevBuf<uint8_t> z_raw, z_text;
    PinBuf<unsigned long long> z_h_verdict;
    StageTimer<2> tm_inflate;
    float last_inflate_ms = 0;               // HIP-event time of the last call's inflate kernel (stage timing >= 1, else 0)
    // crass_hip_inflate_gzip_device / crass_hip_load_fastx_gzip (gunzip.hip): per chunk start / text_len / end_bit and link / reason
    // (count step); per chain element start / end_bit of all chunks + the elements' offsets and chain / CRC parts, the text as
    // 16-bit symbols and the 32 KB windows (decode step) — all given back before the call returns
    DevBuf<uint64_t> gz_a64, gz_b64; DevBuf<uint32_t> gz_a32, gz_b32; DevBuf<uint16_t> gz_sym; DevBuf<uint8_t> gz_win;
    DevBuf<uint64_t> gz_ends;                // members mode: the GzEnd records (3 words each)
    StageTimer<6> tm_gzip;                   // marks around find, count (count step: 0 1 2), decode, windows, narrow (decode step: 2 .. 5)
    float last_gzip_ms[5] = {0, 0, 0, 0, 0};  // find, count, decode, windows, narrow of the last gzip inflate (stage timing >= 1, else 0)
    // a rank's part of crass_hip_group_inflate_gzip (gzip_rank_*, engine_inflate.cpp): the symbolic windows, the deflate bytes
    // [gzr_lo, gzr_hi) that z_raw holds, a pair of marks per step and their times (find, count, decode, symbolic windows,
    // resolve, narrow), the byte ranges this rank uploaded — all scratch given back by gzip_rank_release
    DevBuf<uint16_t> gz_wsym;
    const uint8_t *gzr_file = nullptr; uint64_t gzr_lo = 0, gzr_hi = 0;
    // ... and of a group's files load: per gzip file the text of the elements [e0, e1) this rank inflated (text byte p of the file at
    // text.p + 16 + p - off[e0]) and the resolved window in front of element e1, kept until the load ends (gzip_kept_release);
    // the seeded window walks that added elements later: their marks, milliseconds and elements
    struct GzKept { const uint8_t *file = nullptr; uint64_t e0 = 0, e1 = 0; DevBuf<uint8_t> text, seed; };
    std::vector<GzKept> gz_kept;
    StageTimer<2> tm_gzt;
    float gzr_tail_ms = 0; uint64_t gzr_tail_elements = 0;
    StageTimer<14> tm_gzr;
    float gzr_ms[6] = {0, 0, 0, 0, 0, 0};
    float gzr_crc_ms = 0;                    // members mode: k_gz_member_crc over the rank's pieces, marks 12 and 13
    std::vector<std::pair<uint64_t, uint64_t>> gzr_uploads;
    int gzip_on_device = 0;                  // crass_hip_set_gzip_on_device: crass_hip_load_fastx_files takes plain gzip (CRASS_GZIP_ON_DEVICE_*)
    // crass_hip_fetch_text (k_fetch_text, pack.hip): the records' indices / flags / offsets and the text on the device, kept from
    // call to call, their pinned host sides (f_h_off and f_h_chars are what crass_text points at), the flags of
    // crass_hip_fetch_record_text
    DevBuf<uint64_t> f_idx, f_off; DevBuf<uint8_t> f_rc, f_chars;
    PinBuf<uint64_t> f_h_idx, f_h_off; PinBuf<uint8_t> f_h_rc, f_h_chars;
    StageTimer<2> tm_fetch;
    float last_fetch_ms = 0;
    std::vector<uint8_t> f_flags;
    // crass_hip_fastx_header_ids_device (fastx_hid.hip): the name table, the uploaded record positions, the ids, the list of
    // long names and the control words ([0..4) 32-bit: long names, bad position; then the 64-bit count of repeats) — all given
    // back before the call returns; the marks around the insert launches and behind the lookup launch
    DevBuf<unsigned long long> n_table; DevBuf<uint64_t> n_rec_pos, n_ids, n_ctl; DevBuf<uint32_t> n_long;
    PinBuf<uint64_t> n_h_ctl;
    StageTimer<3> tm_names;
    float last_hid_ms[3] = {0, 0, 0};        // whole call's kernels, the insert launches, the lookup launch
    // crass_hip_fastx_names_build_device: the same table and record positions, KEPT until crass_hip_fastx_names_drop, the next
    // build or destroy (built on the arena: also until the next load or attach, drop_arena); the bytes are the caller's or the
    // arena's.  crass_hip_fastx_names_find: the queries, their offsets, the list of long ones and the answers on the device — given
    // back before the call returns
    DevBuf<unsigned long long> nt_table; DevBuf<uint64_t> nt_rec_pos;
    bool have_names = false, nt_on_arena = false;
    const uint8_t *nt_bytes = nullptr; uint64_t nt_n_bytes = 0, nt_n_reads = 0, nt_mask = 0;
    DevBuf<uint8_t> nq_names; DevBuf<uint64_t> nq_off, nq_out; DevBuf<uint32_t> nq_long;
    // crass_hip_fastx_names_find_device: the queries, offsets and answers are the caller's; the list of long queries (nq_long) and
    // the two control words (long queries, a bad offset pair) are ours.  crass_hip_fastx_names_of_device / crass_hip_found_names_device:
    // the lengths, the tile sums, the flag word, the record numbers of a step without a dense blob and the offsets of a caller
    // who gave too few words for them — all given back before the call returns; the pinned words the host reads (find: the two
    // control words; names of: the total, then the flag)
    DevBuf<uint32_t> nq_ctl, no_len, no_flag; DevBuf<uint64_t> no_tiles, no_idx, no_off;
    PinBuf<uint64_t> nq_h_ctl, no_h;
    uint64_t last_find_found = 0;            // answers of the last crass_hip_fastx_names_find_device that named a record
    StageTimer<2> tm_find;
    float last_names_ms[2] = {0, 0};         // the last build's insert launches, the last find's kernels
    LineFetch hl, ql;                        // header lines, quality strings
    // crass_hip_fastx_comments_build_device (k_cm_bits / _tiles / _top): the own-comment bitmap, the tiles' carries and the files'
    // read bases on the device, KEPT until crass_hip_fastx_comments_drop, the next build, any load or attach, or destroy; the bytes
    // are the caller's or the arena's; the record positions stay on the HOST (the layout's pinned array on the arena, else a copy
    // of the caller's) — the fetch turns the few sources into positions there.  The build's scratch (the uploaded positions, the
    // tiles' counts, the flag word) and the fetch's (cm: the indices then the positions, the sources behind them, the starts,
    // lengths, offsets and text) are given back before the call returns; cm's pinned sides stay, h_off and h_chars are what
    // crass_text points at
    DevBuf<uint64_t> ct_bits, ct_carry, ct_frb;
    bool have_comments = false, ct_on_arena = false;
    const uint8_t *ct_bytes = nullptr; uint64_t ct_n_bytes = 0, ct_n_reads = 0, ct_counts[2] = {0, 0}; uint32_t ct_n_files = 0;
    std::vector<uint64_t> ct_h_rec_pos;
    DevBuf<uint64_t> cb_rec_pos, cb_cnt; DevBuf<uint32_t> cb_flag; PinBuf<uint64_t> cb_h;
    LineFetch cm;
    StageTimer<2> tm_cm;
    float last_cm_ms[2] = {0, 0};            // the last build's three launches, the last fetch's kernels
    // crass_hip_load_fastx_files: the arena (every file's text, a '\n' behind each) stays until the next load, attach or destroy
    // (drop_arena); the pinned per-file arrays crass_fastx_files_layout points at (read bases, byte bases, formats)
    DevBuf<uint8_t> fa_arena; uint64_t fa_bytes = 0; bool have_arena = false;
    std::vector<uint64_t> fa_read_base;      // the records in front of every piece of the arena (files, or a shard's slices) and their total
    PinBuf<uint64_t> fa_h_base; PinBuf<int32_t> fa_h_format;
    // a shard of a group's files load (fastx_shards.h): the staged text of the nominal range and where each file's part lies in
    // it, a BGZF tail, the probe's per-block parts — all given back by shard_pack / shard_abort; what shard_scan found for
    // shard_pack (the slices' arena bases, the records); the marks around the last k_fx_cut_probe launch
    struct ShardStaged { uint32_t file; uint64_t a, b, off; };      // the text range [a, b) of the file lies at sh_stage + off
    DevBuf<uint8_t> sh_stage, sh_tail; DevBuf<FxProbe> sh_part; PinBuf<FxProbe> sh_h_part;
    std::vector<ShardStaged> sh_staged;
    std::vector<uint64_t> sh_base;
    uint64_t sh_n_reads = 0; bool sh_scanned = false, sh_loaded = false;
    StageTimer<2> tm_probe;
    float last_probe_ms = 0;
    // ... and of a wrapped-mode piece (fastx_shards.h): its line table and chain (k_fw_cut_*, scratch as fw_scratch_words), kept
    // from shard_stage_probe to the end of the chain over the ranks; text: the piece staged again with a larger margin, where the
    // chain asked for it.  Given back with the shard's.  The answer of a look-up, and the cut kernels' event times of the load
    struct ShardCut {
        uint32_t file; uint64_t a, b, se, margin;      // the piece [a, b) of the file, staged up to se
        bool left_is_ls; const uint8_t *bytes;          // a is a line start; the device bytes of position a
        FwJob J; uint32_t which;
        DevBuf<uint64_t> scratch; DevBuf<uint8_t> text;
    };
    std::vector<ShardCut> sh_cut;
    DevBuf<uint64_t> sh_cut_out; PinBuf<uint64_t> sh_h_cut_out;
    hipEvent_t ev_cut[2] = {nullptr, nullptr};
    float cut_ms = 0;
    uint64_t cut_lookups = 0, cut_doublings = 0;
};

} // namespace crass
#pragma GCC visibility pop

using namespace crass;

// A/B and test switches from the environment, read ONCE per context (crass_hip_create; crass_hip_reload_env re-reads
// them for a live context) — never on the per-call path
struct EnvSwitches {
    bool no_lookback = false, no_pos_hints = false, merge_profile = false, no_lane_kernel = false;
    bool host_merge = false, no_speculation = false, exc_separate = false, dm_inject_fail = false, dm_init_late = false;
    bool no_presize = false;                         // A/B switch: no first-call bounds / pool sizing at crass_hip_load_reads
    bool dd_full_table = false;                      // A/B switch: pass 1's de-duplication table sized for the survivor slots (the round-3 size)
    bool no_device_view = false;                     // A/B switch: the host rebuilds crass_merge_view from root_of / blank (the round-3 path)
    bool force_device_view = false;                  // CRASS_DEVICE_VIEW=1: the device assembles it for a single context too (default: multi-rank only)
    bool no_dense_light = false;                     // CRASS_NO_DENSE_LIGHT: the A/B switch of the light walk over the dense path's survivors
    bool no_warm_launch = false;                     // CRASS_NO_WARM_LAUNCH: the A/B switch of first_call_bounds' empty launch
    uint32_t view_group_cap = 32768;                 // groups beyond this many members are ranked by the host (CRASS_VIEW_GROUP_CAP)
    uint32_t view_sort_max = 2048;                   // groups of 65 .. this many members are ranked by a sort in LDS (k_dmx_sort; CRASS_VIEW_SORT_MAX: tests)
    uint64_t test_bounds[4] = {0, 0, 0, 0};          // tests: CRASS_TEST_BOUNDS="survivors,distinct,flagged,gathered" replaces the
                                                     // first-call bounds (0 = computed), so that every overflow path can be forced
    uint32_t row_cap = 256, dm_group_cap = 16384, surv_debug = 0;     // row_cap: Levenshtein fallback rows of the long-read layout (strings beyond it: second launch, full rows)
    int stage_timing = -1;
    uint64_t pool_cap_bytes = 0;                     // tests: device allocations beyond this total fail with hipErrorOutOfMemory
    bool no_hint_filter = false;                     // A/B switch: k_filter_general where the hint bits would be the filter
    uint32_t wave_walk_min = 800;                    // pass 2 walks a read per wave when the longest read is beyond this (CRASS_WAVE_WALK_MIN)
    uint32_t long_min = 2048;                        // read sets whose longest read is beyond this take the long-read path (CRASS_LONG_MIN: the A/B switch)
    uint64_t text_chunk_bytes = 64ull << 20;         // crass_hip_load_text: text bytes per staged chunk (CRASS_TEXT_CHUNK_BYTES: tests force many chunks)
    bool inflate_hbm_window = true;                  // CRASS_INFLATE_WINDOW=lds: k_bgzf_inflate decodes in the wave's LDS window, not in the output's own range (A/B switch, inflate.hip)
    uint32_t hid_hash_bits = 64;                     // tests: CRASS_HID_TEST_HASH_BITS keeps only that many low bits of a name's hash (fastx_hid.hip)
    bool lane_find_serial = false;                   // CRASS_LANE_FIND_SERIAL=1: the A/B switch of the lane kernel's packed seed find (lane_find.h)
    uint32_t probe_blocks = 0;                       // tests: CRASS_PROBE_BLOCKS caps the grid of pass 2's anchor probe, so that a few thousand reads are several tiles per wave (0: off)
    void read()
    {
        auto on = [](const char *n) { return getenv(n) != nullptr; };
        no_lookback = on("CRASS_NO_LOOKBACK"); no_pos_hints = on("CRASS_NO_POS_HINTS");
        merge_profile = on("CRASS_MERGE_PROFILE"); no_lane_kernel = on("CRASS_NO_LANE_KERNEL"); host_merge = on("CRASS_HOST_MERGE");
        no_speculation = on("CRASS_NO_SPECULATION"); exc_separate = on("CRASS_EXC_SEPARATE"); dm_init_late = on("CRASS_DM_INIT_LATE");
        dm_inject_fail = on("CRASS_DM_INJECT_FAIL"); no_presize = on("CRASS_NO_PRESIZE"); no_device_view = on("CRASS_NO_DEVICE_VIEW"); dd_full_table = on("CRASS_DD_FULL_TABLE"); force_device_view = on("CRASS_DEVICE_VIEW");
        view_group_cap = 32768; if (const char *e = getenv("CRASS_VIEW_GROUP_CAP")) view_group_cap = (uint32_t)std::max(1, atoi(e));
        view_sort_max = 2048; if (const char *e = getenv("CRASS_VIEW_SORT_MAX")) view_sort_max = (uint32_t)std::min(2048, std::max(64, atoi(e)));
        row_cap = 256; if (const char *e = getenv("CRASS_ROW_CAP")) row_cap = (uint32_t)std::max(1, atoi(e));
        dm_group_cap = 16384; if (const char *e = getenv("CRASS_DM_GROUP_CAP")) dm_group_cap = (uint32_t)std::max(1, atoi(e));
        surv_debug = 0; if (const char *e = getenv("CRASS_SURV_DEBUG")) surv_debug = (uint32_t)atoi(e);
        stage_timing = -1; if (const char *e = getenv("CRASS_STAGE_TIMING")) stage_timing = std::min(2, std::max(0, atoi(e)));
        for (auto &b : test_bounds) b = 0;
        if (const char *e = getenv("CRASS_TEST_BOUNDS")) { int k = 0; for (const char *q = e; *q && k < 4; k++) { test_bounds[k] = (uint64_t)atoll(q); while (*q && *q != ',') q++; if (*q == ',') q++; } }
        no_hint_filter = on("CRASS_NO_HINT_FILTER");
        wave_walk_min = 800; if (const char *e = getenv("CRASS_WAVE_WALK_MIN")) wave_walk_min = (uint32_t)std::max(0, atoi(e));
        long_min = 2048; if (const char *e = getenv("CRASS_LONG_MIN")) long_min = (uint32_t)std::max(0, atoi(e));
        no_warm_launch = getenv("CRASS_NO_WARM_LAUNCH") != nullptr;
        no_dense_light = getenv("CRASS_NO_DENSE_LIGHT") != nullptr;
        text_chunk_bytes = 64ull << 20; if (const char *e = getenv("CRASS_TEXT_CHUNK_BYTES")) text_chunk_bytes = (uint64_t)std::max(1ll, atoll(e));
        inflate_hbm_window = true; if (const char *e = getenv("CRASS_INFLATE_WINDOW")) inflate_hbm_window = strcmp(e, "lds") != 0;
        hid_hash_bits = 64; if (const char *e = getenv("CRASS_HID_TEST_HASH_BITS")) hid_hash_bits = (uint32_t)std::min(64, std::max(0, atoi(e)));
        lane_find_serial = false; if (const char *e = getenv("CRASS_LANE_FIND_SERIAL")) lane_find_serial = atoi(e) != 0;
        probe_blocks = 0; if (const char *e = getenv("CRASS_PROBE_BLOCKS")) probe_blocks = (uint32_t)std::max(0, atoi(e));
        pool_cap_bytes = 0; if (const char *e = getenv("CRASS_POOL_CAP_MB")) pool_cap_bytes = (uint64_t)std::max(1ll, atoll(e)) << 20;
    }
};

// ---- the context's state, in one place -----------------------------------------------------------------------------
// Results:      have_reads -> have_pass1 -> have_merge -> have_pass2 (each API call clears everything to its right and
//               refuses with CRASS_ERR_STATE if what it needs on its left is missing).  dense.active / q_blob_active say
//               which representation holds pass 1's / pass 2's records (compact pinned blob vs host vectors).
// Speculation:  five bounds learnt from the PREVIOUS call of the same stage, each 1.5 x the count seen then, each used to
//               size and queue the next stage before the host has seen the current count.  Every one of them has the same
//               three-step protocol: (1) the kernels read the real count on the device and never touch a slot beyond the
//               bound, (2) the real count reaches the host with the stage's final synchronisation, (3) count > bound =>
//               nothing of the speculative launch is used, the bound is dropped (set to 0) and the stage is repeated with
//               the exact count.  None is ever trusted for a result.
//                 surv_cap_hint     survivors of the seed scan        -> survivor kernels queued behind the compaction
//                 dx_cap_hint       distinct DR strings (one GPU)     -> the device merge queued behind pass 1 (premerge)
//                 xchg.gx_cap_hint  distinct DR strings (all ranks)   -> the same behind the exchange's de-duplication
//                 hit_cap_hint      reads flagged by the anchor probe -> verify / finish / pack queued behind it
//                 (recruit_exact    one-shot: the next recruit call must not speculate, it repeats an overflowed one)
// Queued merge: premerge 0 none / 2 queued by the seed scan and valid (count within the bound), premerge_inflight: its
//               kernels may still be running when the seed scan returns; dm_prepared_n / dm_prepared_src: the survivor
//               kernel already cleared the merge tables for that many tokens of that buffer.  crass_hip_merge ADOPTS a
//               queued merge iff no strings were passed in and premerge == 2, otherwise launches its own.  dm_prev_local: the previous merge ran on the device for this
//               context alone (only then is the next one queued ahead of time).  dm.active: the installed pattern set is
//               the device-built one (dm.M), not the host-built automaton / anchors; dm.host_built, dm.build_pending: the
//               host view (c->merge) of a device merge is being / has been rebuilt by the helper thread.
// Copies:       bulk_pending: exact-size copies of pass 1's hand-off records are in flight on copy_stream; wait_bulk()
//               before any getter reads them (a failed copy is reported there, bulk_status).
// Failure:      a device merge that gives up sets dm.h_st->fail; whoever sees it calls host_merge_fallback (counted in
//               n_merge_fallbacks) and repeats pass 2.  An allocation failure anywhere returns CRASS_ERR_OOM with the
//               context still usable (tests/test_gpu_device_merge.py::test_out_of_memory_is_reported_and_the_context_survives).
struct crass_hip_ctx {
    crass_params prm{};
    EnvSwitches env;
    DevParams dp{};
    int device = 0;
    hipStream_t stream = nullptr;
    mutable int last_hip = 0;

    // resident reads
    DevReads R{};
    bool have_reads = false;
    uint64_t read_base = 0;
    uint32_t max_len = 0;
    bool uniform = false;
    DevBuf<uint32_t> r_packed; DevBuf<uint64_t> r_word_off; DevBuf<uint32_t> r_lengths; DevBuf<uint64_t> r_header_id;
    DevBuf<uint32_t> r_exc_mask; DevBuf<uint64_t> r_exc_read; DevBuf<uint64_t> r_exc_off; DevBuf<uint8_t> r_exc_bytes;
    std::vector<uint64_t> h_exc_read;        // host copy of the exception read indices (local)
    std::vector<uint32_t> h_lengths;         // the lengths of a set whose reads differ in length, kept on the host (crass_hip_fetch_text sums a fetch's offsets from them)
    Ingest in;                               // device ingest: loaders, inflate, header ids, names, header lines, quality, fetch text (engine_ingest.cpp and the four files beside it)

    // scratch
    DevBuf<uint64_t> d_mask; DevBuf<uint32_t> d_word_prefix; DevBuf<uint32_t> d_block_sums;
    DevBuf<uint64_t> d_idx; DevBuf<uint32_t> d_count; DevBuf<uint8_t> d_found; DevBuf<uint32_t> d_hit_info;
    bool hints_valid = false;       // d_hit_info doubles as the pass-1 seed-hint array (pass 2 reuses it afterwards)
    DevBuf<SurvOut> d_surv; DevBuf<char> d_dr; DevBuf<uint32_t> d_ss_pool; DevBuf<uint32_t> d_ss_used;
    DevBuf<RecruitOut> d_rec; DevBuf<uint32_t> d_exc_hit; DevBuf<uint64_t> d_extra;
    DevBuf<uint32_t> d_extra_bad; PinBuf<uint32_t> h_extra_bad;      // crass_hip_recruit_found: the word k_mark_found_skip sets for an entry out of range
    PinBuf<uint32_t> h_count; PinBuf<SurvOut> h_surv; PinBuf<char> h_dr; PinBuf<uint32_t> h_ss; PinBuf<uint64_t> h_idx;
    DevBuf<SurvOut> g_surv; DevBuf<char> g_dr; DevBuf<uint32_t> g_ss;       // host-loop sink: the found records, dense
    PinBuf<RecruitOut> h_rec;
    // automaton
    DevBuf<uint16_t> a_go16; DevBuf<uint32_t> a_go32; DevBuf<uint16_t> a_out; DevBuf<uint16_t> a_go4;
    DevAutomaton A{};
    HostAutomaton H;
    bool full_automaton_uploaded = false;
    DevBuf<uint32_t> a_go4w;
    DevBuf<uint32_t> a_anchor; DevBuf<uint32_t> d_slot_info; DevBuf<uint32_t> d_slot_pid; DevBuf<uint32_t> a_out_pid; DevBuf<uint32_t> a_pat_token;
    bool have_pat_token = false;
    DevAnchors K{};
    bool have_anchors = false;
    bool have_patterns = false;
    uint32_t n_installed_patterns = 0;

    // pass-1 results (host), final hand-off layout
    bool have_pass1 = false;
    struct P1List {
        std::vector<uint64_t> read; std::vector<uint8_t> low; std::vector<uint32_t> replen, nss;
        // (the two large arrays are filled by the host pool right after resize(): no value-initialisation pass over them)
        std::vector<uint64_t> ss_off; std::vector<uint32_t, NoInitAlloc<uint32_t>> ss; std::vector<uint16_t> dr_len; std::vector<char, NoInitAlloc<char>> dr;
        void clear() { read.clear(); low.clear(); replen.clear(); nss.clear(); ss_off.clear(); ss.clear(); dr_len.clear(); dr.clear(); }
        void reserve(size_t n, uint32_t stride) { read.reserve(n); low.reserve(n); replen.reserve(n); nss.reserve(n); ss_off.reserve(n); ss.reserve(n * 6); dr_len.reserve(n); dr.reserve(n * stride); }
        size_t size() const { return read.size(); }
    } cand;
    // fast path: the found records are gathered on the device into dense arrays and land in pinned
    // host memory already in the hand-off layout (no per-record host work)
    mutable struct P1Dense {
        DevBuf<uint16_t> d_dr_len; DevBuf<char> d_dr;       // dense DR strings of the found records (input of the de-duplication)
        uint64_t n = 0;
        bool active = false;
        // everything else of the found records: the compact hand-off blob (p1_blob_layout), assembled by the gather kernel
        // in device memory; its used bytes are copied by the runtime on the copy stream once the host knows the record
        // count (beside the merge kernels; bulk_pending until wait_bulk())
        PinBuf<uint8_t> h_blob; DevBuf<uint8_t> d_blob;
        P1Blob lay{};
        uint32_t pack_ss_cap = 0;
        // the ABI's wide per-candidate arrays (crass_candidates), widened from the compact blob on first request
        bool wide_ready = false;
        // (the two large ones are filled by the host pool right after resize(): no value-initialisation pass over 85 MB)
        std::vector<uint32_t> w_replen, w_nss; std::vector<uint32_t, NoInitAlloc<uint32_t>> w_ss; std::vector<uint64_t> w_ss_off; std::vector<uint16_t> w_dr_len;
        std::vector<char, NoInitAlloc<char>> w_dr;
        PinBuf<char> h_dr_fb; PinBuf<uint16_t> h_dr_len_fb; bool dr_fallback = false;    // candidates' own strings (no distinct list)
        void release()
        {
            h_blob.release(); d_blob.release(); h_dr_fb.release(); h_dr_len_fb.release(); d_dr_len.release(); d_dr.release();
        }
    } dense;
    DevBuf<uint64_t> d_fidx;
    DevBuf<uint64_t> g_fidx;                        // host-loop sink: the found records' slots, gathered (a source of the sink's copies)
    DevBuf<uint64_t> d_pos_hint, d_pos_hint_off; uint64_t n_pos_hint_words = 0;     // long reads: per-position seed hints
    DevBuf<uint32_t> d_punt;                                                          // long reads: [0] count, [1 ..] slots the light walk handed over
    DevBuf<uint32_t> d_redo;                                                          // ... [0] count, [1 ..] slots the full kernel hands on to its full-layout launch
    SdmaCopy *dma_sink[4] = {nullptr, nullptr, nullptr, nullptr};                     // the long-read sink's four copies on DMA engines (created with the first long-read set)
    DevBuf<uint32_t> d_pos_hint_blk; bool pos_hint_blk = false;                       // ragged lengths: read of every 256th hint word
    // device-side DR de-duplication (single-GPU merge fast path)
    DevBuf<unsigned long long> dd_keys; DevBuf<uint32_t> dd_first, dd_slot, dd_rep; DevBuf<uint64_t> dd_hash;
    PinBuf<uint32_t> h_rep; PinBuf<uint64_t> h_hash;
    bool have_rep = false;
    // device-side token ranks: distinct strings (first-occurrence order) + every candidate's distinct index.
    // With these the host merge never touches the per-candidate strings.
    DevBuf<uint32_t> dd_map; DevBuf<char> dd_dx_chars; DevBuf<uint16_t> dd_dx_len; DevBuf<uint64_t> dd_dx_hash;
    PinBuf<uint32_t> h_dmap; PinBuf<char> h_dx_chars; PinBuf<uint16_t> h_dx_len; PinBuf<uint64_t> h_dx_hash;
    uint64_t n_dx = 0;
    bool have_dev_tokens = false;
    uint32_t n_cu = 0;
    bool host_view_light = false;              // crass_hip_set_host_view: a device merge's host view = the own candidates' tokens only
    HostWorker worker;
    uint64_t surv_cap_hint = 0;
    uint64_t hit_cap_hint = 0;                // speculative bound for pass 2's flagged reads (0: none yet)
    bool recruit_exact = false;               // the next recruit call must not speculate (it repeats an overflowed one)               // speculative survivor bound for the next seed scan (0: none yet)
    hipStream_t copy_stream = nullptr;
    // Long reads: k_hint_positions runs in kHintParts slices of the reads, the first on the main stream and the others on
    // hint_stream BESIDE the walking kernel, which is launched slice by slice behind the slice's hints (run_survivors): the
    // hint kernel is VALU-issue bound, the walk LDS-latency bound at two waves per SIMD.
    static constexpr int kHintParts = 4;     // (at most; the default is two — see setup_pos_hints)
    hipStream_t hint_stream = nullptr;
    hipEvent_t ev_hint[kHintParts] = {nullptr, nullptr, nullptr, nullptr}, ev_hint_go = nullptr;
    int hint_parts = 1;                         // slices of this read set (1: one launch on the main stream)
    bool hint_filter = false;                   // the hint bits are this set's seed-scan filter (no lane-per-read filter for its layout)
    bool hint_filter_any = false;               // ... in their every-position form (another window or seed lattice): computed for the filter, not kept
    uint64_t hint_read_split[kHintParts + 1] = {0, 0, 0, 0, 0}, hint_word_split[kHintParts + 1] = {0, 0, 0, 0, 0};
    DevBuf<uint16_t> g_dr_len; DevBuf<uint64_t> hl_dx_idx;      // host-loop sink: dense DR lengths, scratch of the device de-duplication
    bool hint_pending = false;                  // slices are in flight on hint_stream: the main stream has not waited for them yet
    hipEvent_t ev_gathered = nullptr;
    hipEvent_t ev_premerge = nullptr;           // recorded behind a merge queued in the seed scan: the hand-off copy waits for it
    mutable bool bulk_pending = false;          // rare paths only: D2H copies of the candidates' own strings in flight on copy_stream
    // CRASS_OK, or CRASS_ERR_HIP with last_hip set: a failed copy must not be mistaken for delivered records
    int wait_bulk() const
    {
        if (!bulk_pending) return bulk_status;
        const hipError_t e = hipStreamSynchronize(copy_stream);
        int de = sdma_wait(dma);
        for (SdmaCopy *s : dma_sink) de |= sdma_wait(s);
        bulk_pending = false;
        if (e != hipSuccess) { last_hip = (int)e; bulk_status = CRASS_ERR_HIP; }
        else if (de) { last_hip = (int)hipErrorUnknown; bulk_status = CRASS_ERR_HIP; }
        return bulk_status;
    }
    SdmaCopy *dma = nullptr;                    // the hand-off records travel on a DMA engine when the HSA runtime offers one (sdma.cpp)
    // The distinct list of pass 1 (every candidate's index in it, the strings, their lengths) reaches the host the same way:
    // the de-duplication kernel used to write it straight into pinned memory — 5 MB of PCIe stores at 100 M reads, 90 us of
    // the pass-1 tail — while its first reader (the helper thread's view build, get_candidates, the host-merge fall-backs) is
    // a millisecond away.  dx_via_dma: three engine copies started when the counts are known; wait_dx() before any read.
    SdmaCopy *dma_dx[3] = {nullptr, nullptr, nullptr};
    bool dx_via_dma = false;
    mutable std::mutex dx_mu;
    mutable bool dx_pending = false, dx_stream_copy = false;
    mutable int dx_status = CRASS_OK;
    mutable bool dx_hash_valid = true;          // h_dx_hash holds the strings' TokenTable hashes (else: computed on first use)
    int wait_dx() const
    {
        std::lock_guard<std::mutex> lk(dx_mu);
        if (!dx_pending) return dx_status;
        int bad = 0;
        for (SdmaCopy *s : dma_dx) bad |= sdma_wait(s);
        if (dx_stream_copy) { const hipError_t e = hipStreamSynchronize(copy_stream); if (e != hipSuccess) { last_hip = (int)e; bad = 1; } }
        dx_pending = false; dx_stream_copy = false;
        if (bad) { if (!last_hip) last_hip = (int)hipErrorUnknown; dx_status = CRASS_ERR_HIP; }
        return dx_status;
    }
    mutable int bulk_status = CRASS_OK;         // sticky until the next seed scan issues new copies
    // device-side merge (dmerge.hip): clustering, non-redundant set, anchor keys and the pass-2 verification
    // index are built on the device; the host view (c->merge) is rebuilt from its per-token results while
    // pass 2 runs.  dm.active: the installed pattern set lives in dm.M, not in the automaton/anchors above.
    struct DM {
        DevBuf<uint64_t> packed, tmask; DevBuf<uint32_t> codes, owner, root_of, pat_token;
        DevBuf<uint32_t> kset_u32, ent_slot, anchor_tab, anchor_fp; DevBuf<uint8_t> blank; DevBuf<uint64_t> ents, rents; DevBuf<uint32_t> rset_u32, rd_slot;
        DevBuf<unsigned long long> rset_key, bk_key;
        DevBuf<unsigned long long> kset_key; DevBuf<DevMergeState> st; DevBuf<uint32_t> hot;
        PinBuf<DevMergeState> h_st; PinBuf<uint32_t> h_root; PinBuf<uint8_t> h_blank;
        std::vector<uint32_t> gid_tmp;
        DevMerge M{};
        bool active = false, host_built = false;
        int build_status = 0;                       // result of the host-view build that runs on `worker`
        bool build_pending = false;
        // what the build found out, written by whichever thread runs it and copied into the context's own fields
        // (n_installed_patterns, cnt.*, last_hip) by the CALLING thread once the build is known to be over (apply_build_result):
        // the helper thread never writes a field the caller may read without waiting for it
        struct BuildResult { bool valid = false; uint32_t n_patterns = 0, n_keys = 0; float ms_device = 0; int hip = 0; } br;
        uint64_t n_cand = 0;
        // what the host view is rebuilt from: the distinct list (pinned host copy) and every own candidate's index in it
        const char *hx_chars = nullptr; const uint16_t *hx_len = nullptr; uint64_t n_tok = 0;
        // multi-rank: the merge runs over the de-duplicated concatenation of every rank's list
        bool global = false; uint64_t my_off = 0, n_global = 0;
        DevBuf<char> g_chars, gx_chars; DevBuf<uint16_t> g_len, gx_len; DevBuf<unsigned long long> g_keys;
        DevBuf<uint32_t> g_first, g_slot, g_rep, g_prefix, g_bsum; DevBuf<uint64_t> g_hash, g_mask, g_idx;
        PinBuf<uint32_t> h_gmap; PinBuf<char> h_gx_chars; PinBuf<uint16_t> h_gx_len; PinBuf<uint64_t> h_gx_hash;
        std::vector<uint32_t> cand_map;
        hipEvent_t ev_done = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
        uint32_t want_post = 0;                     // the stage flag value pass 2's probe stores for this merge (h_flags[2])
        // crass_merge_view assembled on the device (k_dmx_*, dmerge.hip): scratch, the dense blob, its totals; the blob
        // reaches h_view on a DMA engine (dma_view) started by the helper thread once ev_view has fired
        DevBuf<uint32_t> x_u32, x_members, x_tile; DevBuf<uint8_t> x_blob; DevBuf<DevViewTotals> x_tot;
        PinBuf<DevViewTotals> x_htot; PinBuf<uint8_t> h_view;
        hipStream_t view_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_view = nullptr, ev_apply = nullptr;
        SdmaCopy *dma_view = nullptr, *dma_view2 = nullptr, *dma_view3 = nullptr;
        uint32_t want_blank = 0;                    // the stage flag value k_dm_keys stores for this merge (h_flags[3]): blank[] is final      // (the blob travels in two pieces: the token half behind k_dmx_apply, the rest behind the last kernel)
        bool hx_on_host = true;                     // the gathered distinct list has a pinned host copy (else: on the device only)
        bool view_launched = false;                 // export kernels may be running on view_stream (ev_view orders after them)
        bool apply_recorded = false;                // ev_apply was recorded behind this merge's k_dmx_apply
        bool view_ready = false;                    // h_view holds the view of the current merge (crass_hip_get_merge reads it)
        DevViewTotals view_tot{};
        void release()
        {
            x_u32.release(); x_members.release(); x_tile.release(); x_blob.release(); x_tot.release(); x_htot.release(); h_view.release();
            packed.release(); tmask.release(); bk_key.release(); codes.release(); owner.release(); root_of.release();
            pat_token.release(); kset_u32.release(); ent_slot.release(); anchor_tab.release(); anchor_fp.release();
            blank.release(); ents.release(); rents.release(); rset_u32.release(); rd_slot.release(); rset_key.release(); kset_key.release(); st.release(); hot.release(); h_st.release(); h_root.release(); h_blank.release();
            g_chars.release(); gx_chars.release(); g_len.release(); gx_len.release(); g_keys.release(); g_first.release(); g_slot.release();
            g_rep.release(); g_prefix.release(); g_bsum.release(); g_hash.release(); g_mask.release(); g_idx.release();
            h_gmap.release(); h_gx_chars.release(); h_gx_len.release(); h_gx_hash.release();
            if (ev_done) (void)hipEventDestroy(ev_done);
            if (ev_t0) (void)hipEventDestroy(ev_t0);
            if (ev_t1) (void)hipEventDestroy(ev_t1);
            ev_done = ev_t0 = ev_t1 = nullptr;
            if (view_stream) (void)hipStreamSynchronize(view_stream);
            sdma_destroy(dma_view); dma_view = nullptr;
            sdma_destroy(dma_view2); dma_view2 = nullptr;
            sdma_destroy(dma_view3); dma_view3 = nullptr;
            if (ev_apply) (void)hipEventDestroy(ev_apply);
            ev_apply = nullptr;
            if (ev_fork) (void)hipEventDestroy(ev_fork);
            if (ev_view) (void)hipEventDestroy(ev_view);
            if (view_stream) (void)hipStreamDestroy(view_stream);
            ev_fork = ev_view = nullptr; view_stream = nullptr;
            view_launched = view_ready = false;
        }
    } dm;
    // one-collective exchange (crass_hip_exchange_setup): this rank's distinct list in a fixed-size device buffer
    struct Xchg {
        bool active = false;
        uint32_t world = 1, rank = 0, slot = 0;
        uint64_t cap = 0, needed = 0;
        uint32_t gx_cap_hint = 0;                   // bound for the merge queued ahead of the counters (previous global count x 1.5)
        hipEvent_t ev_counts = nullptr;
        DevBuf<uint8_t> send; DevBuf<uint32_t> xinfo; PinBuf<uint32_t> h_xinfo;
        uint64_t send_bytes() const { return (cap + 1) * (uint64_t)slot; }
    } xchg;
    // distinct candidate strings (multi-GPU exchange)
    std::vector<char> dx_chars; std::vector<uint16_t> dx_len; std::vector<uint32_t> dx_map; bool have_distinct = false;
    // host-loop sink, one chunk without exception reads: the found records reach pinned host memory on the copy stream (bulk_pending)
    // while the merge and pass 2 are queued; the ABI's per-candidate arrays (`cand`) are filled from them when somebody asks
    mutable std::function<void()> cand_fill;
    hipEvent_t ev_sink_copies = nullptr;        // behind those copies on the copy stream: pass 2 re-uses one of their source buffers (d_fidx)
    mutable uint64_t cand_pending_n = 0;
    void materialize_cand() const { if (cand_fill) { std::function<void()> f; f.swap(cand_fill); f(); } }
    uint64_t n_cand() const { return dense.active ? dense.n : (cand_fill ? cand_pending_n : cand.size()); }
    // the distinct DR strings (token order) and every candidate's index among them came from the DEVICE: the dense sink, or the
    // host-loop sink of a long-read set (hl_tokens: its gathered records were de-duplicated on the device beside the copies)
    bool hl_tokens = false;
    bool dev_tokens() const { return have_dev_tokens && (dense.active || hl_tokens); }
    void widen_p1() const;
    const char *cand_dr() const { if (dense.active) { widen_p1(); return dense.w_dr.data(); } materialize_cand(); return cand.dr.data(); }
    const uint16_t *cand_dr_len() const { if (dense.active) { widen_p1(); return dense.w_dr_len.data(); } materialize_cand(); return cand.dr_len.data(); }
    uint32_t dr_stride = 48;
    // merge
    MergeResult merge;
    bool have_merge = false;
    // pass-2 results
    bool have_pass2 = false;
    std::vector<uint64_t> q_read; std::vector<uint8_t> q_low; std::vector<uint32_t> q_start, q_end, q_token;
    std::vector<uint16_t> q_dr_len; std::vector<char, NoInitAlloc<char>> q_dr;      // (q_dr: whoever grows it fills the new bytes)
    // ... or, when the sink ran on the device, one pinned blob (p2_blob_layout)
    PinBuf<uint8_t> h_qblob; P2Blob q_lay{}; uint64_t q_n = 0; bool q_blob_active = false, q_wide_ready = false;

    crass_counters cnt{};
    uint32_t n_merge_fallbacks = 0, last_fallback_bits = 0;
    std::atomic<uint32_t> n_view_fallbacks{0};      // device merges whose host view was built by the host after all (a group beyond the export's cap)
    uint32_t n_bound_overflows[4] = {0, 0, 0, 0};   // speculation bounds that turned out too small (stage repeated): survivors, distinct, flagged, gathered
    hipEvent_t ev[12]{};
    // stage timing (crass_hip_set_stage_timing): an event record costs ~6 us of stream time, 14 of them 8 % of a 1 ms step.
    // 0 none (the default: a crass run reads no stage times), 1 the three large kernels only (seed scan, survivors, pass-2 scan), 2 every stage
    int timing_level = 0;
    // single-pass compaction (k_mask_compact_lb): status words + ticket counter shared by every launch of the context
    DevBuf<unsigned long long> lb_status; DevBuf<uint32_t> lb_ticket; PinBuf<uint32_t> h_lb_fail;
    uint32_t lb_epoch = 0;
    bool lb_on = true;
    // nullptr: use the three-kernel form (switched off, or allocation failed)
    const Lookback *next_lookback(uint64_t n_words, Lookback *out)
    {
        const uint32_t tw = lookback_tile_words(n_words);
        return next_lookback_tiles((n_words + tw - 1) / tw, out);
    }
    // element-wise kernels (k_found_compact, k_dx_flag_rank, k_valid_compact): tiles of 4096 elements
    const Lookback *next_lookback_elems(uint64_t n, Lookback *out) { return next_lookback_tiles((n + 4095) / 4096, out); }
    const Lookback *next_lookback_tiles(uint64_t n_tiles, Lookback *out)
    {
        if (!lb_on || n_tiles == 0) return nullptr;
        if (n_tiles > (1u << 24)) return nullptr;
        if (!lb_status.p || lb_status.n < n_tiles) {
            if (lb_status.ensure(std::max<uint64_t>(n_tiles * 2, 4096)) != hipSuccess) return nullptr;
            if (hipMemsetAsync(lb_status.p, 0, lb_status.n * 8, stream) != hipSuccess) return nullptr;
        }
        if (!lb_ticket.p) {
            if (lb_ticket.ensure(4) != hipSuccess || h_lb_fail.ensure(4) != hipSuccess) return nullptr;
            if (hipMemsetAsync(lb_ticket.p, 0, 16, stream) != hipSuccess) return nullptr;
            h_lb_fail.p[0] = 0;
        }
        lb_epoch = (lb_epoch + 1) & 0x3FFFFFFFu;
        if (lb_epoch == 0) lb_epoch = 1;
        out->status = lb_status.p; out->ticket = lb_ticket.p; out->epoch = lb_epoch; out->fail = h_lb_fail.p;
        return out;
    }
    // allocation only (crass_hip_load_reads): hands out no tickets — a launch that never runs must not move the ticket base
    void prealloc_lookback(uint64_t n_tiles)
    {
        if (!lb_on || n_tiles == 0 || n_tiles > (1u << 24)) return;
        if (!lb_status.p || lb_status.n < n_tiles) {
            if (lb_status.ensure(std::max<uint64_t>(n_tiles * 2, 4096)) != hipSuccess) return;
            if (hipMemsetAsync(lb_status.p, 0, lb_status.n * 8, stream) != hipSuccess) return;
            // (a re-allocated status array starts a new life: epochs of the old one mean nothing in it)
        }
        if (!lb_ticket.p) {
            if (lb_ticket.ensure(4) != hipSuccess || h_lb_fail.ensure(4) != hipSuccess) return;
            if (hipMemsetAsync(lb_ticket.p, 0, 16, stream) != hipSuccess) return;
            h_lb_fail.p[0] = 0;
        }
    }
    // after a synchronisation: a look-back spin that gave up invalidates the stage (never expected)
    int lookback_ok()
    {
        if (!h_lb_fail.p || !h_lb_fail.p[0]) return CRASS_OK;
        h_lb_fail.p[0] = 0; lb_on = false;
        last_hip = (int)hipErrorLaunchTimeOut;
        return CRASS_ERR_HIP;
    }
    // the device merge queued by the seed scan itself, right behind pass 1 (no host round trip in between): sized by a
    // bound learnt from the previous merge, adopted by crass_hip_merge when the counts turn out to fit
    bool dd_full_table = false;                         // a de-duplication table sized for the distinct strings overflowed once
    uint32_t dx_cap_hint = 0; bool dm_prev_local = false; int premerge = 0;      // premerge: 0 none, 2 queued and valid
    // a merge sized ahead of pass 1's survivor stage, whose kernel cleared the merge's tables (device_merge_prepare)
    uint64_t dm_prepared_n = 0; const char *dm_prepared_src = nullptr;
    bool premerge_inflight = false;                 // merge kernels may still be running when the seed scan returns
    double t_p1_sync = 0;                           // CRASS_MERGE_PROFILE: host time line between pass 1 and the merge
    bool spans_p1 = false, spans_p2 = false, span_survivors = false;     // spans to evaluate at the next counters fetch
    // Deferred pass-1 tail (crass_hip_exchange_set_deferred; a rank of a multi-rank job): crass_hip_seed_scan queues pass 1 up to the
    // kernel that fills the exchange's send buffer and RETURNS — the caller queues the collective and crass_hip_merge_gathered its
    // kernels behind it on the same stream, and only then does the host wait for pass 1's counters (p1_finish).  The ~60 us the
    // device idled between pass 1's last kernel and the exchange (host wake-up, the collective's and the unpack's launches) are
    // gone.  The counters of the deferred stage land in h_count[16..24) (the exchange's kernels rewrite h_count[0..8) meanwhile).
    // A launch that turns out unusable (bound too small, no device-resident distinct list) was marked by k_xg_fill in the send
    // buffer's header from the same counters: every rank then sees an exchange that "did not fit" and the step is repeated, this
    // context's next seed scan running synchronously (force_sync).
    // Stage flags (DevMerge::flag_pre, engine_internal.h): pinned words stored by the first kernel of a stage; the host polls them
    // where it used to wait for an event recorded between two kernels.  [0] pass 1 complete (k_xg_fill, deferred pass 1),
    // [1] everything in front of the merge complete (k_dm_pack_codes), [2] the merge complete (pass 2's probe).  A poll that runs
    // out of its budget falls back to a stream synchronisation (CRASS_NO_POLL: the events of round 5, the A/B switch).
    PinBuf<uint32_t> h_flags; uint32_t flag_seq = 0, want_p1 = 0, want_pre = 0, want_post = 0; bool poll_on = false;
    mutable std::atomic<uint32_t> n_poll_timeouts{0};
    bool poll_flag(int k, uint32_t want, double budget_ms) const
    {
        const volatile uint32_t *f = h_flags.p + k;
        const double t0 = now_ms();
        for (uint32_t it = 0;; it++) {
            if ((int32_t)(*f - want) >= 0) { std::atomic_thread_fence(std::memory_order_acquire); return true; }
            __builtin_ia32_pause();
            if ((it & 255u) == 255u && now_ms() - t0 > budget_ms) { n_poll_timeouts++; return false; }
        }
    }
    struct P1Deferred {
        bool enabled = false, active = false, finishing = false, force_sync = false;
        uint64_t n_bound = 0; uint32_t ss_cap = 0, ss_elem = 1;
        bool fast = false, hint_filtered = false;
    } p1d;
    const uint32_t *p1_counts() const { return p1d.finishing ? h_count.p + 16 : h_count.p; }
    // level 1 only: which of the three large kernels are bracketed (bit 0 seed scan, 1 survivors, 2 pass-2 scan)
    unsigned timing_focus = 7;
    bool timed(int i, int level) const
    {
        if (timing_level < level) return false;
        if (timing_level >= 2 || level != 1) return true;
        const unsigned bit = (i <= 1) ? 1u : (i == 8 || i == 9) ? 2u : 4u;
        return (timing_focus & bit) != 0;
    }
    hipError_t stamp(int i, int level) { return timed(i, level) ? hipEventRecord(ev[i], stream) : hipSuccess; }
    float span(int a, int b, int level) const
    {
        float ms = 0;
        if (!timed(a, level) || !timed(b, level) || hipEventElapsedTime(&ms, ev[a], ev[b]) != hipSuccess) ms = 0;
        return ms;
    }
};

#define HIPCHK(ctx, call)                                                       \
    do {                                                                        \
        hipError_t e__ = (call);                                                \
        if (e__ != hipSuccess) { (ctx)->last_hip = (int)e__; return e__ == hipErrorOutOfMemory ? CRASS_ERR_OOM : CRASS_ERR_HIP; } \
    } while (0)

// ---- the bounds a stage is sized with before the host knows its count: 1.5 x the count of the previous call, rounded up ---------
inline uint64_t hit_bound(uint64_t n_hits)              // pass 2's flagged reads
{
    return std::max<uint64_t>(4096, (n_hits + n_hits / 2 + 4095) & ~4095ull);
}
inline uint64_t survivor_bound(uint64_t n_surv)         // the seed filter's survivors
{
    return std::min<uint64_t>(std::max<uint64_t>(65536, (n_surv + n_surv / 2 + 65535) & ~65535ull), 1ull << 26);
}
inline uint64_t distinct_bound(uint64_t n_tok)          // distinct DR strings: a context's own, or the gathered list's
{
    return (n_tok * 3 / 2 + 4095) & ~4095ull;
}
// slots of the de-duplication table for up to n strings: a power of two, at most half full
inline uint32_t dedupe_table_size(uint64_t n)
{
    uint32_t tsize = 1024;
    while (tsize < n * 2) tsize <<= 1;
    return tsize;
}

// p1_finish: the speculative launch of a deferred pass 1 cannot be used — k_xg_fill marked the send buffer from the same counters,
// so every rank of the job sees an exchange that did not fit and repeats the step; this context's next seed scan runs synchronously
constexpr int kP1Redo = 1000;

// ---- what crosses the engine's files, each declared once ------------------------------------------------------------------------
// (C linkage like the ABI functions they are defined among; hidden: not part of the library's dynamic symbols)
#pragma GCC visibility push(hidden)
extern "C" {
// engine.cpp
int validate_reads(const crass_reads *r);
void reset_results(crass_hip_ctx *c);
int alloc_scratch(crass_hip_ctx *c);
int finish_load(crass_hip_ctx *c, const DevReads &R, uint64_t read_index_base, uint32_t max_len, const uint32_t *lengths, uint64_t total_words);
void quiesce_worker(crass_hip_ctx *c);
int install_patterns(crass_hip_ctx *c, const StringArena &pats);
int ensure_full_automaton(crass_hip_ctx *c);
// engine_pass1.cpp
int first_call_bounds(crass_hip_ctx *c);
void presize_hostloop(crass_hip_ctx *c);
int ensure_recruit_buffers(crass_hip_ctx *c, uint64_t h_alloc, uint64_t n_exc, bool dev_sink, bool anchors);
int read_count(crass_hip_ctx *c);
int p1_finish(crass_hip_ctx *c);
int settle_p1(crass_hip_ctx *c);
// engine_merge.cpp
int device_merge_prepare(crass_hip_ctx *c, const char *dx_chars, const uint16_t *dx_len, uint64_t n_tok, const uint32_t *d_ntok);
int device_merge_enqueue(crass_hip_ctx *c, const char *dx_chars, const uint16_t *dx_len, uint64_t n_tok, const uint32_t *d_ntok, bool prepared);
void ensure_distinct(crass_hip_ctx *c);
int ensure_host_merge(crass_hip_ctx *c);
int host_merge_fallback(crass_hip_ctx *c);
// engine_ingest.cpp: every device and pinned buffer and every event of c->in goes; crass_hip_destroy calls it with the
// context's streams still alive and waited for
void ingest_free_all(crass_hip_ctx *c);
} // extern "C"
#pragma GCC visibility pop

/*
 * crass_hip.h — C ABI of the MI355X-native crass search engine (libcrass_hip.so).
 *
 * This is the drop-in boundary for crass's WorkHorse search path.  The reference has no
 * FFI layer: the seam is three C++ free functions called from WorkHorse::parseSeqFiles
 * (reference paths are relative to the crass v1.0.1 tree):
 *
 *   searchFile()               src/crass/libcrispr.h:74-80   (call: WorkHorse.cpp:340-346)
 *   createNonRedundantSet()    src/crass/WorkHorse.h:111-112 (call: WorkHorse.cpp:370)
 *   findSingletons()           src/crass/libcrispr.h:86-92   (call: WorkHorse.cpp:386)
 *   sink: addReadHolder()      src/crass/libcrispr.h:123-125
 *
 * Each entry point below names the reference interface it replaces.  Plain pointers and
 * sizes only; caller-allocated/caller-freed flat buffers or views into context-owned
 * memory; no C++ objects or exceptions cross this boundary; every function returns an
 * int status (0 = CRASS_OK) and crass_hip_strerror() explains it.  One context per GPU,
 * one host thread per context (the reference is single-threaded).
 *
 * INTEGRATION.md shows the C++ adapter a crass maintainer would add on top of this.
 */
#ifndef CRASS_HIP_H
#define CRASS_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRASS_HIP_ABI_VERSION 3   /* 2: crass_counters, crass_fastx and crass_synth_spec grew (round 2); group API (round 3);
                                    3: crass_counters grew (used_device_view, n_view_fallbacks) (round 4) */

/* ---- status codes (reference: crispr::exception -> exit code) ---- */
enum {
    CRASS_OK = 0,
    CRASS_ERR_INVALID_ARG   = 1,   /* bad pointer / size / parameter combination             */
    CRASS_ERR_UNSUPPORTED   = 2,   /* parameter outside the engine's implementation limits   */
    CRASS_ERR_NO_DEVICE     = 3,   /* no HIP device / HIP runtime failure at init            */
    CRASS_ERR_HIP           = 4,   /* a HIP call failed (crass_hip_last_hip_error())         */
    CRASS_ERR_OOM           = 5,   /* host or device allocation failed                       */
    CRASS_ERR_STATE         = 6,   /* call order violated (e.g. recruit before patterns)     */
    CRASS_ERR_SEARCH_FATAL  = 7,   /* the reference would have thrown "Fatal error in search
                                      algorithm!" (libcrispr.cpp:141-149)                    */
    CRASS_ERR_OVERFLOW      = 8,   /* an internal device pool overflowed                     */
    CRASS_ERR_IO            = 9,   /* file could not be opened / parsed                      */
    CRASS_ERR_RCCL          = 10   /* an RCCL call failed (crass_hip_group_last_error())     */
};

/* implementation limits of the device path (checked by crass_hip_create) */
#define CRASS_HIP_MAX_WINDOW   9      /* CRASS_DEF_MAX_SEARCH_WINDOW_LENGTH, crassDefines.h:55 */
#define CRASS_HIP_MIN_WINDOW   6
#define CRASS_HIP_MAX_DR       240    /* highDRsize upper bound handled on device             */
#define CRASS_HIP_MAX_READ_LEN 60000  /* longest read the device path accepts                 */

/* ---- options: POD mirror of the hot-path fields of `options` (crassDefines.h:140-170) ---- */
typedef struct {
    uint32_t lowDRsize;          /* -d  default 23  (crassDefines.h:121) */
    uint32_t highDRsize;         /* -D  default 47  (:122)               */
    uint32_t lowSpacerSize;      /* -s  default 26  (:123)               */
    uint32_t highSpacerSize;     /* -S  default 50  (:124)               */
    uint32_t searchWindowLength; /* -w  default 8   (:56), 6..9          */
    uint32_t minNumRepeats;      /* -n  default 2   (:91)                */
    int32_t  kmer_clust_size;    /* -k  default 6   (:67)                */
} crass_params;

void crass_default_params(crass_params *p);       /* crass.cpp:430-460 */

typedef struct crass_hip_ctx crass_hip_ctx;

/* ---- reads: the device-resident replacement for "re-read every file twice" ---- *
 * 2-bit packed bases (A=0 C=1 G=2 T=3), 16 bases per uint32, base i of a read in bits
 * [2*(i%16), 2*(i%16)+2) of word i/16; every read starts on a word boundary.
 * A read containing any byte outside {A,C,G,T} is an *exception read*: it keeps its slot in
 * `packed` (content ignored) and is listed, as raw bytes, in the exception arrays, so that
 * the reference's raw-byte semantics (N matches N, lower case is not ACGT)
 * are kept on the device's byte-wise kernels.                                              */
typedef struct {
    uint64_t        n_reads;
    const uint32_t *packed;        /* all reads, word-aligned                                      */
    uint32_t        stride_words;  /* >0: read i starts at word i*stride_words; 0: use word_off    */
    const uint64_t *word_off;      /* [n_reads] start word of each read (stride_words == 0)        */
    uint32_t        uniform_len;   /* >0: every read has this length; 0: use lengths               */
    const uint32_t *lengths;       /* [n_reads] (uniform_len == 0)                                 */
    uint64_t        n_exceptions;
    const uint64_t *exc_read;      /* [n_exceptions] ascending read indices                        */
    const uint64_t *exc_off;       /* [n_exceptions+1] offsets into exc_bytes                      */
    const uint8_t  *exc_bytes;     /* raw sequence bytes of the exception reads                    */
    const uint64_t *header_id;     /* [n_reads] or NULL.  header_id[i] = index of the FIRST read
                                      with the same header (readsFound is keyed by header string,
                                      libcrispr.cpp:138,411); NULL = all headers unique            */
    uint64_t        read_index_base; /* global index of read 0 (multi-GPU shards)                  */
} crass_reads;

/* ---- lifecycle ---- */
/* replaces: the `options` argument of searchFile/findSingletons */
int  crass_hip_create(const crass_params *p, int device, crass_hip_ctx **out);
/* Stage timing with HIP events on the context's stream.  An event record costs ~6 us of stream time, so the
 * default (0) times nothing; 1 times the three large kernels (counters ms_filter, ms_survivor, ms_recruit); 2 adds every
 * stage (ms_compact, ms_pass1_total, ms_merge_device, ms_recruit_finish, ms_pass2_total).  (Until round 6 the default was 1:
 * six records = ~35 us of every step of every caller, 3.5 % of a rank's step at 100 M reads over 8 GPUs.)
 * Environment override at creation: CRASS_STAGE_TIMING=0|1|2.  (No reference counterpart: crass has no timers.) */
int  crass_hip_set_stage_timing(crass_hip_ctx *ctx, int level);
/* The A/B and test switches of the environment (CRASS_HOST_MERGE, CRASS_NO_SPECULATION, CRASS_DM_*, ...) are read once,
 * when the context is created — never on the per-call path.  This re-reads them for a live context (tests that flip
 * a switch between two runs of one context).  (No reference counterpart.) */
int  crass_hip_reload_env(crass_hip_ctx *ctx);
/* Level 1 only: which of the three large kernels are bracketed — bit 0 seed scan (ms_filter), bit 1 survivors
 * (ms_survivor), bit 2 pass-2 scan (ms_recruit); default 7.  A caller that reports one kernel's duration over many
 * calls (bench.py: the dominant one) times just that kernel: two event records per call instead of six. */
int  crass_hip_set_timing_focus(crass_hip_ctx *ctx, unsigned kernels);
/* Orders the context's stream behind a HIP event recorded on another stream (hipEvent_t passed as void*): lets the
 * caller's collective (RCCL all-gather on its own stream) feed crass_hip_merge_gathered without a host wait. */
int  crass_hip_stream_wait_event(crass_hip_ctx *ctx, void *event);
void crass_hip_destroy(crass_hip_ctx *ctx);
const char *crass_hip_strerror(int status);
int  crass_hip_last_hip_error(const crass_hip_ctx *ctx);

/* replaces: getFileHandle/kseq_read loops of searchFile+findSingletons (libcrispr.cpp:84-96,
 * 471-487): host buffers are copied to HBM once and stay resident for both passes. */
int crass_hip_load_reads(crass_hip_ctx *ctx, const crass_reads *host_reads);
/* same, but every pointer in `dev_reads` is a DEVICE pointer the caller owns (e.g. torch
 * tensors) and keeps alive until the context is destroyed or new reads are set. */
int crass_hip_attach_device_reads(crass_hip_ctx *ctx, const crass_reads *dev_reads);
/* replaces: crass_pack_reads + crass_hip_load_reads for a caller that holds sequence TEXT (one byte per base, read i =
 * seqs[off[i] .. off[i+1]), off[n_reads+1] a host array): the 2-bit packing runs on the device (pack.hip) with
 * crass_pack_reads' byte semantics and layout rules (pad_uniform 0 | 1 | 2 as there), and the resident set, the exception
 * list and the counters end up exactly as after the host route.  The text goes up in chunks of whole reads through two
 * pinned staging buffers, the copy of one chunk beside the pack kernel of the one before (CRASS_TEXT_CHUNK_BYTES, read at
 * crass_hip_create: bytes per chunk, default 64 MB); text in pinned memory is copied from where it is.
 * CRASS_ERR_INVALID_ARG: a NULL pointer with n_reads > 0, offsets that decrease; CRASS_ERR_UNSUPPORTED (nothing launched,
 * no reads resident): a read beyond CRASS_HIP_MAX_READ_LEN. */
int crass_hip_load_text(crass_hip_ctx *ctx, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads,
                        int pad_uniform, const uint64_t *header_id, uint64_t read_index_base);
/* same, but d_seqs is a DEVICE pointer (a torch uint8 tensor, the output of another GPU stage, a decompressor); off stays
 * a host array.  The text is only read during the call: the packed set belongs to the context, the caller may free the
 * text on return.  Any lengths and any bytes: the way to attach device-resident input that is ragged or holds an 'N'
 * (crass_hip_attach_device_reads takes packed words of one stride without exception reads). */
int crass_hip_attach_device_text(crass_hip_ctx *ctx, const uint8_t *d_seqs, const uint64_t *off, uint64_t n_reads,
                                 int pad_uniform, const uint64_t *header_id, uint64_t read_index_base);

/* ---- pass 1 : searchFile / searchCore (libcrispr.cpp:68-166, 265-395) ---- *
 * Runs the seed-scan filter, ordered compaction, and the survivor kernel (scanRight,
 * extendPreRepeat, qcFoundRepeats incl. Levenshtein, DRLowLexi) on the device.  Results are
 * kept in the context in read order.                                                       */
int crass_hip_seed_scan(crass_hip_ctx *ctx);

/* candidates found by pass 1, in read order (views into context memory, valid until the
 * next seed_scan/load).  One entry per read for which searchCore returned true.           */
typedef struct {
    uint64_t        n;
    const uint64_t *read_idx;     /* global read index (read_index_base + local)                  */
    const uint8_t  *low_lexi;     /* RH_WasLowLexi after DRLowLexi (ReadHolder.cpp:513-591)       */
    const uint32_t *repeat_len;   /* RH_RepeatLength                                              */
    const uint32_t *n_ss;         /* RH_StartStops.size()                                         */
    const uint64_t *ss_off;       /* offset of this read's start/stops in ss_pool                 */
    const uint32_t *ss_pool;      /* start/stop pairs AFTER DRLowLexi (mirrored if flipped)       */
    uint32_t        dr_stride;    /* bytes per DR slot                                            */
    const uint16_t *dr_len;
    const char     *dr_chars;     /* low-lexi representative DR of read k at dr_chars+k*dr_stride */
    uint32_t        max_read_len; /* searchFile's return value (libcrispr.cpp:98,165)             */
} crass_candidates;
int crass_hip_get_candidates(const crass_hip_ctx *ctx, crass_candidates *out);

/* ---- merge : addReadHolder token order + createNonRedundantSet (libcrispr.cpp:1119-1162,
 * StringCheck.cpp:46-81, WorkHorse.cpp:612-709, 1404-1637) ---- *
 * Input: the representative DR strings of ALL pass-1 candidates in global read order (for
 * one GPU: the context's own; for several GPUs: the all-gathered slots of every rank, rank
 * order == read order).  dr_chars == NULL means "use this context's candidates".
 * Deterministic: every rank that feeds the same list builds the same tokens, groups and
 * pattern list.  Also installs the pattern list for crass_hip_recruit().                   */
int crass_hip_merge(crass_hip_ctx *ctx, const char *dr_chars, const uint16_t *dr_len,
                    uint32_t dr_stride, uint64_t n_candidates);

/* Multi-GPU exchange in its compact form: only the DISTINCT representative DR strings of a rank's
 * candidates travel (first-occurrence order), not one string per candidate.  Scanning the ranks'
 * lists in rank order reproduces the global first-occurrence order, so tokens come out exactly
 * as if one process had seen every read (libcrispr.cpp:1137-1143).                            */
typedef struct {
    uint64_t        n_distinct;
    uint32_t        dr_stride;
    const uint16_t *dr_len;        /* [n_distinct]                                                */
    const char     *dr_chars;      /* string d at dr_chars + d*dr_stride                          */
    uint64_t        n_candidates;
    const uint32_t *cand_distinct; /* [n_candidates] index of each candidate's string in the list */
} crass_distinct;
int crass_hip_get_distinct(crass_hip_ctx *ctx, crass_distinct *out);
/* merge from the concatenation (rank order) of every rank's distinct list; `my_offset` is where this
 * context's own list starts in it.  crass_merge_view.cand_token then covers this context's candidates. */
int crass_hip_merge_distinct(crass_hip_ctx *ctx, const char *dr_chars, const uint16_t *dr_len, uint32_t dr_stride,
                             uint64_t n_global, uint64_t my_offset);

/* The same exchange with the lists left on the device (RCCL all-gather between device buffers): the device
 * addresses of this context's distinct list (CRASS_ERR_STATE when pass 1 did not produce it on the device,
 * use crass_hip_get_distinct then), and the merge from a device-resident concatenation.  The merge copies
 * the list, so the caller's buffers may be released as soon as the call returns.                          */
typedef struct {
    uint64_t        n_distinct;
    uint32_t        dr_stride;
    const char     *d_chars;       /* device pointer, n_distinct * dr_stride bytes                */
    const uint16_t *d_len;         /* device pointer                                              */
} crass_distinct_dev;
int crass_hip_get_distinct_device(crass_hip_ctx *ctx, crass_distinct_dev *out);
int crass_hip_merge_distinct_device(crass_hip_ctx *ctx, const char *d_chars, const uint16_t *d_len, uint32_t dr_stride,
                                    uint64_t n_global, uint64_t my_offset);

/* One-collective form of the exchange.  After crass_hip_exchange_setup every seed scan leaves this rank's
 * distinct list in a fixed-size device buffer: row 0 = header {uint64 n_distinct, uint32 stride, uint32
 * rows}, then `cap_rows` slots of `slot_bytes` (DR bytes, zero padded, then the uint16 length).  The caller
 * all-gathers that buffer (ncclAllGather / torch all_gather_into_tensor: world * send_bytes) and hands the
 * result to crass_hip_merge_gathered, which compacts, de-duplicates and merges on the device.
 * CRASS_ERR_OVERFLOW: some rank had more than cap_rows strings (every rank sees that in the headers) —
 * set up again with crass_hip_exchange_needed_rows() rows, repeat the seed scan and the collective.       */
typedef struct {
    void    *d_send;              /* device pointer, send_bytes bytes, owned by the context              */
    uint64_t send_bytes;          /* (cap_rows + 1) * slot_bytes                                          */
    uint32_t slot_bytes;
    uint64_t cap_rows;
} crass_exchange;
int crass_hip_exchange_setup(crass_hip_ctx *ctx, uint32_t world, uint32_t rank, uint64_t cap_rows, crass_exchange *out);
int crass_hip_merge_gathered(crass_hip_ctx *ctx, const void *d_recv);
uint64_t crass_hip_exchange_needed_rows(const crass_hip_ctx *ctx);
/* on != 0: from the next call on, crass_hip_seed_scan of a context with an exchange set up QUEUES pass 1 up to the kernel that
 * fills the send buffer and returns without waiting for it; the caller queues its collective on the context's stream
 * (crass_hip_stream) — or on a stream ordered behind it — and calls crass_hip_merge_gathered, which queues its own kernels behind
 * the collective and only then waits for pass 1's counters.  The device no longer idles between pass 1 and the exchange while
 * the host wakes up, launches the collective and the unpack (~60 us of a rank's ~1 ms step at 100 M reads over 8 GPUs).  Any
 * other call that reads pass 1's results settles the pending scan first.  A scan whose speculative launch turns out unusable
 * (more survivors than its bound, no device-resident distinct list) marks its send buffer on the device: every rank's
 * crass_hip_merge_gathered then returns CRASS_ERR_OVERFLOW exactly as for a list that did not fit (needed rows <= the capacity
 * in use), and the repeated seed scan of the marked rank runs synchronously.  Off by default; crass_hip_group_* and
 * crass_amd.distributed.GatheredExchange switch it on.  (No reference counterpart: crass is single-threaded, TODO.md:18.) */
int crass_hip_exchange_set_deferred(crass_hip_ctx *ctx, int on);
/* A row capacity for the first exchange of a job whose LARGEST shard holds n_reads reads: the bound the engine itself
 * speculates with for a shard's distinct DR strings (a few hundred per million reads on metagenome-like input, >= 16 384).
 * Every rank must use the same capacity; with this one the first step of a group neither overflows nor repeats pass 1
 * (16 384 rows, the round-3 default, did at 50 M reads per rank: 18.4 ms for the first step against 4.9 in steady state). */
uint64_t crass_hip_exchange_rows_for(uint64_t n_reads_of_largest_shard);

typedef struct {
    uint32_t        n_tokens;     /* StringCheck size; tokens are 2 .. n_tokens+1                 */
    const char     *tok_chars;    /* token t string = tok_chars[tok_off[t-2] .. tok_off[t-1])     */
    const uint64_t *tok_off;      /* [n_tokens+1]                                                 */
    uint64_t        n_candidates; /* length of cand_token                                         */
    const uint32_t *cand_token;   /* token of every candidate fed to merge, in the same order     */
    uint32_t        n_groups;     /* mDR2GIDMap size; GIDs are 1 .. n_groups                      */
    const uint32_t *grp_tokens;   /* group g (GID g+1) = grp_tokens[grp_off[g] .. grp_off[g+1])   */
    const uint64_t *grp_off;      /* [n_groups+1]                                                 */
    uint32_t        n_patterns;   /* Vecstr* returned by createNonRedundantSet                    */
    const char     *pat_chars;
    const uint64_t *pat_off;      /* [n_patterns+1]                                               */
    const uint32_t *pat_group;    /* GID of each pattern                                          */
    int32_t         next_free_gid;/* nextFreeGID after clustering (WorkHorse.cpp:369-370)         */
} crass_merge_view;
int crass_hip_get_merge(const crass_hip_ctx *ctx, crass_merge_view *out);

/* The same merge as a context-free host function (no GPU needed): used by the multi-rank
 * driver's CPU tests and by callers that only want createNonRedundantSet's result.        */
typedef struct crass_merge_handle crass_merge_handle;
int  crass_merge_create(const char *dr_chars, const uint16_t *dr_len, uint32_t dr_stride,
                        uint64_t n_candidates, int32_t kmer_clust_size, crass_merge_handle **out);
/* the host view of a merge whose per-token results (GID, dropped by removeRedundantRepeats) were computed
 * elsewhere — by the device merge in the engine; exported so that the rebuild can be tested without a GPU.
 * dx_*: the distinct DR strings in token order; cand_distinct[k] = index of candidate k's string.          */
int  crass_merge_rebuild(const char *dx_chars, const uint16_t *dx_len, uint32_t dr_stride, uint64_t n_distinct,
                         const uint32_t *cand_distinct, uint64_t n_candidates, const uint32_t *gid_of,
                         const uint8_t *dropped, uint32_t n_groups, crass_merge_handle **out);
int  crass_merge_get(const crass_merge_handle *h, crass_merge_view *out);
void crass_merge_destroy(crass_merge_handle *h);

/* ---- pass 2 : findSingletons / on_match (libcrispr.cpp:399-518) ---- */
/* replaces: refsplit + acism_create (libcrispr.cpp:452-469).  Optional: merge() already
 * installed the non-redundant set; use this to recruit with an explicit pattern list.
 * A pattern is 1 .. min(255, dr_stride) bytes long, dr_stride = highDRsize rounded up to a
 * multiple of 16 (crass_recruits.dr_stride: the slot a recruit's DR string is returned in;
 * 48 with the default parameters).  A set holding an empty or a longer pattern is declined
 * as a whole with CRASS_ERR_UNSUPPORTED before anything is installed: the context then has
 * no pattern set, and crass_hip_recruit returns CRASS_ERR_STATE until a valid one is given.
 * An empty list (n = 0) is valid: crass_hip_recruit then recruits nothing.                   */
int crass_hip_set_patterns(crass_hip_ctx *ctx, const char *const *patterns,
                           const uint32_t *lengths, uint32_t n);
/* replaces: the acism_scan loop.  Reads whose header was found in pass 1 (readsFound,
 * libcrispr.cpp:411) are skipped; `extra_found` (may be NULL) lists further header ids,
 * as global read indices, found by OTHER ranks' pass 1 (duplicate headers across shards).  */
int crass_hip_recruit(crass_hip_ctx *ctx, const uint64_t *extra_found, uint64_t n_extra);
/* replaces: the same, with a second list of found reads that lies in DEVICE memory and may hold CRASS_NAME_NOT_FOUND — the
 * answers of crass_hip_fastx_names_find_device as they are, no copy to the host and back (k_mark_found_skip passes those
 * entries over).  n_d_extra == 0: crass_hip_recruit, call for call.  CRASS_ERR_INVALID_ARG: a NULL d_extra_found with
 * n_d_extra > 0, or any other device entry >= the resident set's reads (seen on the device before anything of that list is
 * marked): no pass-2 result is left, crass_hip_get_recruits returns CRASS_ERR_STATE.  The repeats inside the call (host merge
 * fall-back, a bound that was too small) carry both lists along. */
int crass_hip_recruit_found(crass_hip_ctx *ctx, const uint64_t *extra_found, uint64_t n_extra, const uint64_t *d_extra_found, uint64_t n_d_extra);

typedef struct {
    uint64_t        n;
    const uint64_t *read_idx;     /* global read index, ascending                                 */
    const uint8_t  *low_lexi;     /* RH_WasLowLexi                                                */
    const uint32_t *start;        /* the single repeat [start, end] AFTER DRLowLexi               */
    const uint32_t *end;
    uint32_t        dr_stride;
    const uint16_t *dr_len;
    const char     *dr_chars;     /* low-lexi DR (== a stored token string)                       */
    const uint32_t *token;        /* StringToken (existing, or newly added like addReadHolder)    */
} crass_recruits;
int crass_hip_get_recruits(const crass_hip_ctx *ctx, crass_recruits *out);

/* ---- Levenshtein / similarity batch (PatternMatcher.cpp:111-204) on the device ---- *
 * pair k compares chars[a_off[k] .. a_off[k]+a_len[k]) with chars[b_off[k] ..)              */
int crass_hip_levenshtein_batch(crass_hip_ctx *ctx, const char *chars, uint64_t n_chars,
                                const uint64_t *a_off, const uint32_t *a_len,
                                const uint64_t *b_off, const uint32_t *b_len,
                                uint64_t n_pairs, int32_t *dist_out, float *sim_out);

/* ---- observability (the reference only has a wall-clock progress line) ---- */
typedef struct {
    uint64_t n_reads, n_exceptions;
    uint64_t n_filter_survivors;    /* reads with a lattice seed hit (superset allowed)           */
    uint64_t n_pass1_found, n_pass2_found;
    uint32_t n_patterns, ac_states;
    uint32_t used_fast_filter;      /* 1: bit-parallel lane-per-read kernel, 2: position hints (reads of 257 .. 2 048 bases, differing strides), 0: general */
    uint32_t used_lds_automaton;    /* pass 2: 2 = anchor filter + exact scan of flagged reads,
                                       1 = automaton in LDS over all reads, 0 = automaton in L2   */
    /* HIP-event timings of the last call, milliseconds, measured on the context's stream      */
    float ms_filter, ms_compact, ms_survivor, ms_pass1_total;
    float ms_recruit, ms_recruit_finish, ms_pass2_total;
    float ms_merge_host, ms_sink_host;
    uint64_t bytes_reads_device;    /* packed read bytes resident in HBM                          */
    uint32_t anchor_keys;           /* distinct anchor keys of the pattern set (pass 2): 16-mers;
                                       12-mers when lowDRsize is 15 .. 18 (device-built sets)     */
    uint32_t anchor_table_kind;     /* 0 exact keys in LDS, 1 fingerprint buckets in LDS,
                                       2 exact keys probed in L2 (key set beyond LDS)             */
    uint32_t used_device_merge;     /* 1: clustering / non-redundant set / pass-2 index built on the
                                       device (dmerge.hip), 0: host merge (merge.cpp)             */
    float ms_merge_device;          /* HIP-event time of the device merge kernels                 */
    uint32_t n_merge_fallbacks;     /* since crass_hip_create: device merges that gave up (key set beyond the table,
                                       cuckoo insertion, a wait that timed out, ...) and were redone on the host     */
    uint32_t last_fallback_bits;    /* the device merge's `fail` word of the last such case (0: none so far)         */
    uint32_t n_bound_overflows[4];  /* since crass_hip_create: stages repeated because a speculation bound (sized from the read
                                       set at load, or learnt from the previous call) was too small: [0] seed-scan survivors,
                                       [1] distinct DR strings (queued merge), [2] reads flagged in pass 2, [3] gathered
                                       distinct strings (multi-rank).  Results are unaffected; each is one repeated stage.  */
    uint32_t used_device_view;      /* 1: crass_merge_view's arrays (tokens, groups, pattern list) of the last merge were
                                       assembled on the device and copied by a DMA engine; 0: built by the host            */
    uint32_t n_view_fallbacks;      /* since crass_hip_create: device merges whose view the host built after all (a group
                                       with more members than the export ranks on the device)                              */
} crass_counters;
int crass_hip_get_counters(const crass_hip_ctx *ctx, crass_counters *out);

/* ---- several GPUs from ONE process (north_star: "C++ host code ... RCCL all-gather over xGMI") ----
 * A group owns one context per device.  The reads shard by contiguous ranges in input order (rank r holds reads
 * [r*n/N, (r+1)*n/N), WorkHorse.cpp:336-393: pass 1 covers every read before pass 2 starts), every rank runs pass 1 on its
 * shard, ONE collective — ncclAllGather inside ncclGroupStart/ncclGroupEnd on the contexts' streams, communicators from
 * ncclCommInitAll — moves every rank's distinct candidate DR strings to every rank (the fixed-size buffers of
 * crass_hip_exchange_setup), each rank merges the rank-ordered concatenation on its device (identical tokens, groups,
 * pattern set and pass-2 index everywhere: no broadcast of tables) and recruits on its shard.  The host view of the
 * merge (crass_merge_view) is built ONCE for the group, by rank 0.  There is no reference counterpart: crass is a
 * single-threaded program; what the group replaces is the same three calls of WorkHorse::parseSeqFiles
 * (searchFile / createNonRedundantSet / findSingletons, WorkHorse.cpp:340,370,386) over all reads.
 * flags: CRASS_GROUP_LOCAL_COPIES replaces the collective by plain device copies (required when a device is listed more
 * than once — RCCL refuses duplicate devices — which is how the group is tested on a one-GPU box).
 * Duplicate headers (readsFound is keyed by header, libcrispr.cpp:138,411) are honoured across shards: pass-1 hits of a
 * header that also occurs in another shard are marked found there before pass 2.
 * Call order as for a context: load_reads -> seed_scan -> merge -> recruit (or step = the three in one dispatch).
 * One host thread calls the group; the group runs one helper thread per additional rank.                              */
typedef struct crass_hip_group crass_hip_group;
#define CRASS_GROUP_LOCAL_COPIES 1u
int  crass_hip_group_create(const crass_params *p, const int *devices, int n_devices, unsigned flags, crass_hip_group **out);
void crass_hip_group_destroy(crass_hip_group *g);
int  crass_hip_group_size(const crass_hip_group *g);
/* ranks of the RCCL communicator (ncclCommCount), 0 when the collective is the local-copy stand-in */
int  crass_hip_group_rccl_ranks(const crass_hip_group *g);
/* text of the last RCCL / group error of this process ("" if none); valid until the next group call */
const char *crass_hip_group_last_error(void);
/* rank r's context, for the per-rank getters (crass_hip_get_counters, crass_hip_get_candidates, ...); owned by the group */
crass_hip_ctx *crass_hip_group_ctx(crass_hip_group *g, int rank);
int  crass_hip_group_load_reads(crass_hip_group *g, const crass_reads *host_reads);
int  crass_hip_group_seed_scan(crass_hip_group *g);
int  crass_hip_group_merge(crass_hip_group *g);
/* extra_found: further found headers as job-level read indices (crass_hip_recruit's argument), routed to the shards */
int  crass_hip_group_recruit(crass_hip_group *g, const uint64_t *extra_found, uint64_t n_extra);
/* an explicit pattern list on every rank instead of the group's own merge (the seam's findSingletons, whose pattern list
 * comes from the caller's createNonRedundantSet; crass_hip_set_patterns).  Found headers of OTHER shards are then the
 * caller's to pass (extra_found): it holds readsFound.                                                          */
int  crass_hip_group_set_patterns(crass_hip_group *g, const char *const *patterns, const uint32_t *lengths, uint32_t n);
int  crass_hip_group_step(crass_hip_group *g);         /* seed_scan + merge + recruit, one dispatch per rank */
/* the hand-off of the whole job, in global read order (rank order == read order): views into group-owned memory, valid
 * until the next group call.  get_merge: tokens / groups / patterns from rank 0's host view, cand_token for the
 * candidates of all ranks (the order of crass_hip_group_get_candidates).                                          */
int  crass_hip_group_get_candidates(crass_hip_group *g, crass_candidates *out);
int  crass_hip_group_get_merge(crass_hip_group *g, crass_merge_view *out);
int  crass_hip_group_get_recruits(crass_hip_group *g, crass_recruits *out);
/* Which host view a context builds after a device merge: 0 (default) the full one, 1 only its own candidates' tokens
 * (ranks other than 0 of a group: tokens, groups and patterns are identical on every rank and are read from rank 0). */
int  crass_hip_set_host_view(crass_hip_ctx *ctx, int light);

/* ---- the stage right behind the hot path: true-DR consensus + start/stop repair ----
 * replaces: int WorkHorse::findConsensusDRs(GroupKmerMap&, int& nextFreeGID)  (WorkHorse.cpp:578-611, called at :403), i.e.
 * per DR group parseGroupedDRs (:1135-1379): Aligner (Aligner.cpp:73-468 over ksw_align, ksw.c:330-360) -> consensus and
 * possible split of the group (calculateDRConsensus :801-938, splitGroupedDR :940-1132) -> ReadHolder::updateStartStops
 * for every read (ReadHolder.cpp:382-511: smithWaterman, SmithWaterman.cpp:151-308, with its Levenshtein filter :283),
 * and combineGroupsWithIdenticalDRs (:416-452) after every group.
 * Input = the hand-off of the search path as flat arrays; mReads[token] = the records of that token in record order
 * (pass-1 records of all files, then pass-2 records: the push order of addReadHolder, libcrispr.cpp:1161).           */
typedef struct {
    const char *seqs; const uint64_t *seq_off; uint64_t n_reads;     /* the input reads (as read from the files)        */
    uint64_t n_rec;                                                  /* records = ReadHolders                           */
    const uint64_t *rec_read;        /* index into seqs                                                                 */
    const uint8_t  *rec_lowlexi;     /* RH_WasLowLexi: 0 = the holder's RH_Seq is the reverse complement of the read    */
    const uint32_t *rec_token;       /* StringToken of the holder's ReadList                                            */
    const uint32_t *rec_nss; const uint64_t *rec_ss_off; const uint32_t *ss_pool;    /* RH_StartStops                   */
    uint32_t n_tokens; const char *tok_chars; const uint64_t *tok_off;               /* StringCheck: token t = entry t-2 */
    uint32_t n_groups; const uint32_t *grp_tokens; const uint64_t *grp_off;          /* mDR2GIDMap: GID g = entry g-1    */
    uint32_t max_read_len;                                                           /* mMaxReadLength                   */
} crass_cons_input;

typedef struct {
    uint64_t n_groups_parsed;        /* parseGroupedDRs calls that reached the coverage stage (incl. split sub-groups)  */
    uint64_t n_ksw_launches, n_ksw_alignments, n_placements, n_flips, n_true_drs, n_sw_tasks, n_partials_added;
} crass_counters_cons;

typedef struct {
    int32_t  error;                  /* != 0: the reference would have thrown / crashed / not terminated on this input  */
    int32_t  next_free_gid;
    uint32_t n_tokens;               /* StringCheck after the stage (reversed slaves and split forms add tokens)        */
    const char *tok_chars; const uint64_t *tok_off;
    uint32_t n_groups;               /* groups with a true DR (mTrueDRs), ascending GID                                 */
    const int32_t *grp_gid; const char *dr_chars; const uint64_t *dr_off;           /* GID, laurenized true DR          */
    const uint32_t *grp_tokens; const uint64_t *grp_off;                            /* mDR2GIDMap[GID], in order        */
    uint64_t n_rec;                  /* per input record:                                                               */
    const uint8_t  *rec_alive;       /* 0: the ReadHolder was deleted                                                   */
    const uint8_t  *rec_rc;          /* 1: RH_Seq is the reverse complement of the input read                           */
    const uint32_t *rec_token;       /* the token whose ReadList holds the record (0: none)                             */
    const uint32_t *rec_nss; const uint64_t *rec_ss_off; const uint32_t *ss_pool;   /* repaired RH_StartStops           */
    const uint64_t *tokread_off; const uint64_t *tokread_idx;                       /* mReads[token]: records in order  */
    const uint8_t  *tok_has_list;
    crass_counters_cons counters;
} crass_cons_view;

typedef struct crass_cons crass_cons;
/* runs the whole stage on `device`; CRASS_OK with view.error != 0 when the reference itself would not have survived the
 * input (the view is then incomplete)                                                                                  */
int  crass_hip_consensus(const crass_params *p, int device, const crass_cons_input *in, crass_cons **out);
int  crass_hip_consensus_view(const crass_cons *c, crass_cons_view *v);
void crass_hip_consensus_free(crass_cons *c);

/* ---- the consensus stage's two alignment kernels on their own (tests: against the compiled reference's answers) ----
 * crass_hip_ksw_batch: ksw_align (ksw.c:330-360) with the Aligner's scoring (Aligner.h:112-136) of query v (codes 0..4,
 * q_codes[q_off[v] .. + q_len[v])) against target q_tgt[v] (t_codes[t_off[t] .. + t_len[t])), and of its reverse
 * complement, through the consensus stage's own batch code.  out[2 v + o][3] = score, tb, qb (o = 1: the reverse
 * complement; tb = qb = -1 below minsc).  CRASS_ERR_UNSUPPORTED (nothing launched): a query longer than
 * CRASS_HIP_KSW_MAX_QLEN; CRASS_ERR_INVALID_ARG: an empty string, a code above 4, a target index out of range.          */
#define CRASS_HIP_KSW_MAX_QLEN 320
int crass_hip_ksw_batch(int device, const uint8_t *q_codes, const uint32_t *q_off, const uint32_t *q_len, const uint32_t *q_tgt,
                        uint32_t n, const uint8_t *t_codes, const uint32_t *t_off, const uint32_t *t_len, uint32_t n_targets,
                        int32_t *out);
/* crass_hip_smith_waterman_batch: smithWaterman(read, dr, &aStart, &aEnd, start[k], len[k], similarity)
 * (SmithWaterman.cpp:151-308) of task k, read = chars[read_off[k] .. + read_len[k]), dr = chars[dr_off[k] .. + dr_len[k]),
 * through the consensus stage's own updateStartStops code (scratch layout, k_cons_sw launches in scratch-bounded chunks,
 * Levenshtein batch, similarity decision).  a_ret = read[a_off .. + a_len), b_ret = dr[b_off .. + b_len); a rejected
 * alignment (similarity != 0) has aStart = aEnd = a_len = b_len = 0.  n_launches (may be NULL): k_cons_sw launches used.
 * CRASS_ERR_INVALID_ARG (nothing launched): len < 1, start < 0, start + len > read_len, an empty DR, chars out of range.
 * CRASS_CONS_SW_BUDGET (environment, bytes, read per call): the traceback scratch budget per launch (default 1 GB).        */
int crass_hip_smith_waterman_batch(int device, const char *chars, uint64_t n_chars, const uint64_t *read_off, const uint32_t *read_len,
                                   const uint64_t *dr_off, const uint32_t *dr_len, const int32_t *start, const int32_t *len, uint64_t n,
                                   double similarity, int32_t *a_start, int32_t *a_end, int32_t *a_off, int32_t *a_len, int32_t *b_off,
                                   int32_t *b_len, uint32_t *n_launches);

/* ---- the stages behind findConsensusDRs: spacer graph + crass's output files ----
 * replaces, for a caller that wants crass's outputs from the hand-off: WorkHorse::buildGraph / cleanGraph / makeSpacerGraphs /
 * cleanSpacerGraphs / splitIntoContigs / generateFlankers / removeLowConfidenceNodeManagers (WorkHorse.cpp:196-277 ->
 * NodeManager.cpp, CrisprNode.cpp, SpacerInstance.cpp) and WorkHorse::outputResults (WorkHorse.cpp:1900-2249: crass.crispr
 * through crispr::xml::writer, Group_<gid>_<DR>.fa through NodeManager::dumpReads, Spacers_<gid>_<DR>_spacers.gv and
 * crass.<timestamp>.keys.gv through printSpacerGraph / printSpacerKey).  Host code (<= 10^4 reads per group; serial graph
 * work), no GPU needed.  Input: the groups that have a true DR after crass_hip_consensus, ascending GID, and for each the
 * ReadHolders in buildGraph's order (WorkHorse.cpp:454-505: for every token of mDR2GIDMap[GID], mReads[token] in list
 * order) with RH_Seq as it stands after the consensus stage.
 * The reference's own output depends on heap addresses where a graph has forks or bubbles (edge maps keyed by CrisprNode*):
 * creation order is used there (oracle/crass_graph.py: parity unpinned for these two rows).            */
typedef struct {
    uint32_t n_groups; const int32_t *gid; const char *dr_chars; const uint64_t *dr_off;      /* true DR of group g            */
    const uint64_t *grp_rec_off;                                  /* [n_groups+1]: records of group g, in buildGraph's order  */
    uint64_t n_rec;
    const char *hdr_chars; const uint64_t *hdr_off;               /* RH_Header                                                  */
    const char *com_chars; const uint64_t *com_off;               /* RH_Comment (may be NULL: no comments)                      */
    const char *seq_chars; const uint64_t *seq_off;               /* RH_Seq                                                     */
    const uint32_t *rec_nss; const uint64_t *rec_ss_off; const uint32_t *ss_pool;              /* RH_StartStops                 */
} crass_graph_input;
typedef struct {
    const char *out_dir;          /* options::output_fastq as crass holds it (with the trailing '/'), only used in names/urls  */
    const char *timestamp;        /* mTimeStamp, crass.cpp:476-479 ("%d_%m_%Y_%H%M%S")                                          */
    const char *command_line;     /* mCommandLine, crass.cpp:508-512 (every argv followed by a blank)                           */
    const char *cwd;              /* getcwd() (WorkHorse.cpp:2104)                                                              */
    int32_t log_to_screen;        /* options::logToScreen: no <file type="log"> entry                                           */
    int32_t cov_cutoff;           /* options::covCutoff, default 3 (crassDefines.h:126); <= 0: default                         */
    int32_t node_kmer;            /* options::cNodeKmerLength, default 7 (crassDefines.h:111); <= 0: default                   */
    int32_t show_singles, long_description;                       /* options::showSingles / longDescription, default 0         */
} crass_output_opts;
typedef struct crass_outputs crass_outputs;
typedef struct {
    uint32_t n_files; const char *const *name; const char *const *data; const uint64_t *size;  /* file contents in memory      */
    uint32_t n_groups_kept; const int32_t *kept_gid;              /* the groups in crass.crispr                                 */
    const char *stdout_text;                                      /* what crass prints to stdout in these stages                */
} crass_outputs_view;
int  crass_build_outputs(const crass_graph_input *in, const crass_output_opts *opts, crass_outputs **out);
int  crass_outputs_get(const crass_outputs *o, crass_outputs_view *v);
int  crass_outputs_write(const crass_outputs *o, const char *dir);                              /* every file into dir          */
void crass_outputs_free(crass_outputs *o);

/* raw stream handle (hipStream_t) the context launches on, for callers that time with HIP
 * events or want to order their own work (torch.cuda.ExternalStream) */
void *crass_hip_stream(const crass_hip_ctx *ctx);

/* ---- host utilities: ingest side of the boundary ("next" row f-2) ---- */
/* 2-bit packer.  seqs: concatenated raw bytes, off[n+1].  Allocates the output arrays with
 * malloc (free with crass_free_packed).  pad_uniform: 0 = per-read word offsets, 1 = every
 * read padded to stride_words = ceil(max_len/16), 2 = pad when the reads are short (64..256
 * bases) and padding costs at most twice the words (trimmed reads of differing lengths then
 * take the uniform-stride kernels).                                                        */
typedef struct {
    crass_reads reads;              /* host pointers, owned by this struct                        */
    void *owner;
} crass_packed;
int  crass_pack_reads(const uint8_t *seqs, const uint64_t *off, uint64_t n_reads,
                      int pad_uniform, crass_packed *out);
void crass_free_packed(crass_packed *p);
/* HIP-event time, in milliseconds on the context's stream, of the pack kernels of the last crass_hip_load_text /
 * crass_hip_attach_device_text call; measured when the stage timing level is >= 1 (crass_hip_set_stage_timing), else 0.
 * Device text: the kernel alone.  Host text: first kernel to last, the waits for the chunks' copies included.
 * (No reference counterpart: crass has no timers.) */
float crass_hip_last_pack_ms(const crass_hip_ctx *ctx);
/* the context's resident read set copied back to the host as a crass_packed (malloc'd, free with crass_free_packed; arrays
 * the set does not have are NULL, as from crass_pack_reads; header_id and read_index_base as loaded): lets a caller cache
 * the packed form of text it loaded with crass_hip_load_text / crass_hip_attach_device_text.  CRASS_ERR_STATE: no reads.
 * (No reference counterpart: crass reads its input files again for every pass.) */
int  crass_hip_get_packed(const crass_hip_ctx *ctx, crass_packed *out);
/* ---- the raw bytes of a FASTA / FASTQ file in, parsed on the device (fastx_scan.hip) ----
 * replaces: crass_read_fastx + crass_pack_reads + crass_hip_load_reads (the kseq_read loop of libcrispr.cpp:96-131 and the
 * packer) for a caller that holds the FILE's bytes — in host memory, or in HBM as the output of another GPU stage: no host code
 * touches a sequence byte.  kseq is a byte-stream parser ('>' '@' '+' anywhere in a sequence end it); the device scans by LINES,
 * which agrees with kseq on the regular class below and on nothing else, so every input is either
 *   accepted (CRASS_OK): the resident set, the exception list, the counters and seq_off equal, bit for bit, what crass_read_fastx
 *     on the same bytes + crass_pack_reads (same pad_uniform) + crass_hip_load_reads give; or
 *   declined (CRASS_ERR_UNSUPPORTED): no reads are resident (as after a failed crass_hip_load_text), decline_reason / decline_pos
 *     say why, and the caller takes the host readers.  A different answer is never an outcome.
 * Lines are the pieces between '\n' bytes (the last may lack its '\n'; an empty piece after a final '\n' is no line).
 *   regular FASTA: byte 0 is '>'; every line whose first byte is '>' is a header line; every other line is a sequence line and
 *     holds none of '>' '@' '+' (empty lines, '\r', blanks, NUL, bytes >= 128 are fine); the file does not end with a '>' that is
 *     the first byte of its line.  A record may have no sequence line: an empty read.
 *   regular four-line FASTQ: byte 0 is '@'; the lines are a multiple of 4; line 4k starts with '@'; line 4k+1 holds none of
 *     '>' '@' '+'; line 4k+2 starts with '+'; line 4k+3 holds no byte 127 and as many bytes in 33..126 as line 4k+1.
 * A read is the bytes 33..126 of its record's sequence lines.  Reads beyond CRASS_HIP_MAX_READ_LEN: CRASS_ERR_UNSUPPORTED as from
 * crass_hip_load_text (decline_reason 11).  Other errors: CRASS_ERR_INVALID_ARG — a NULL pointer with n_bytes > 0, pad_uniform
 * outside 0..2; CRASS_ERR_UNSUPPORTED — n_bytes == 0 (an empty file has no format to report).
 * decline_reason: 1 empty input, 2 byte 0 is neither '>' nor '@', 3 FASTQ lines no multiple of 4 (position: the first line of the
 * incomplete record), 4 FASTQ line 4k does not start with '@', 5 '>' '@' '+' in a sequence line, 6 FASTQ line 4k+2 does not start
 * with '+', 7 byte 127 in a quality line, 8 / 9 quality line shorter / longer than its sequence line, 10 FASTA ends with a lone
 * '>', 11 a read beyond the length limit.  The verdict is the first offending line and, within it, the smallest reason. */
typedef struct {
    uint64_t n_reads; int32_t format;      /* '>' | '@' */
    int32_t decline_reason;                /* 0 when accepted */
    uint64_t decline_pos;                  /* byte position of the first offending line, when declined */
    uint32_t max_len;
    const uint64_t *rec_pos;               /* [n_reads+1] position of each record's header character; rec_pos[n] = n_bytes */
    const uint64_t *seq_off;               /* [n_reads+1] offsets in the concatenated sequence text */
} crass_fastx_layout;
/* the scan on the host, one byte after the other (no GPU needed): what the device scan is tested against.  rec_pos / seq_off are
 * malloc'd (crass_fastx_layout_free), NULL when the input is declined. */
int  crass_fastx_scan_host(const uint8_t *bytes, uint64_t n_bytes, crass_fastx_layout *out);
void crass_fastx_layout_free(crass_fastx_layout *l);
/* bytes in host memory: they go up through the two staged buffers of crass_hip_load_text (CRASS_TEXT_CHUNK_BYTES each) into one
 * device buffer of n_bytes, then the device route runs.  out may be NULL; its arrays are context-owned pinned memory, valid until
 * the next load, attach or destroy (NULL when declined).  header_id is left NULL (crass_hip_set_header_ids,
 * crass_hip_fastx_header_ids_device). */
int  crass_hip_load_fastx_bytes(crass_hip_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                crass_fastx_layout *out);
/* same, but d_bytes is a DEVICE pointer of any alignment (a torch uint8 tensor, a decompressor's output).  The bytes are read
 * only during the call: the caller may free them on return. */
int  crass_hip_attach_device_fastx(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                   crass_fastx_layout *out);
/* ---- wrapped FASTQ: records whose sequence or quality runs over several lines, blank lines between records and at the end ----
 * FASTQ class 1 (class 0, the default, is the four-line form above).  What kseq_read (kseq.cpp:171-226) reads record by record
 * without losing a byte: byte 0 is '@'; a VOID line holds no byte in 33..127; a record is a header line whose first byte is '@',
 * zero or more sequence lines holding none of '>' '@' '+', the first following line whose first byte is '+' (the rest of it is
 * ignored, it ends with a '\n'), quality lines — with L the record's bytes 33..126 of its sequence lines, the lines behind the '+'
 * line up to the first line END at which their bytes 33..126 are L or more (none when L is 0), and there they are exactly L —,
 * any number of void lines, then the next header line or the end of the input.  Every regular four-line FASTQ is in the class
 * with the same layout; FASTA is untouched by the class.
 * Declines, per record in this order, the position the first byte of the line named: 3 no line behind the header starts with '+'
 * (the header line), 5 '>' '@' '+' in a sequence line (the first such line), 12 CRASS_FX_FQ_EMPTY_SEQ: the sequence is empty and
 * the line behind the '+' line starts with '@' — kseq_read swallows that byte (kseq.cpp:217) — (that line), 7 byte 127 in a
 * quality line (the first such line), 9 the count passes L inside a line (that line), 8 the input ends before the count is L or
 * inside the '+' line (the header line), 4 the first line behind the quality that is not void does not start with '@' (that
 * line); 1, 2 and 11 as above.  Only the records reachable from line 0 are judged: a quality line that starts with '@' is no
 * header.  An '@' record without a '+' line (kseq reads it like FASTA) is declined with 3 or 5. */
#define CRASS_FX_FQ_EMPTY_SEQ 12
/* the host rule for a class (kseq.cpp:171-226): fastq_class 0 is crass_fastx_scan_host, byte for byte; 1 walks a file whose byte 0
 * is '@' record by record under the wrapped rule.  CRASS_ERR_INVALID_ARG: a class outside 0..1. */
int  crass_fastx_scan_host_class(const uint8_t *bytes, uint64_t n_bytes, int fastq_class, crass_fastx_layout *out);
/* the class the context's device ingest reads FASTQ by (kseq.cpp:171-226): crass_hip_load_fastx_bytes, crass_hip_attach_device_fastx,
 * crass_hip_load_fastx_bgzf / _gzip / _gzip_members and crass_hip_load_fastx_files.  0 (the default): every call as before.  1: a
 * FASTQ piece is scanned by four lines first; where that scan declines it for its shape (reasons 3 .. 9), the wrapped scan
 * (fastx_wrapped.hip) reads the piece again and its verdict is the call's: exactly crass_fastx_scan_host_class(.., 1, ..).  The
 * group load (crass_hip_group_load_fastx_files) has a switch of its own, crass_hip_group_set_fastq_class, which sets this one on
 * every rank's context.  With class 1 set, crass_hip_fetch_quality_device(_to) reads a record's quality by the wrapped rule (k_qw_measure):
 * behind the '+' line as many bytes 33..126 as the record has sequence bytes, over however many lines — on a four-line record
 * the same answer as with class 0.  Header lines, names, header ids and comments need the record positions alone.
 * crass_hip_last_scan_ms stays the four-line scan's kernels; the wrapped scan's are not in it.
 * CRASS_ERR_INVALID_ARG: a class outside 0..1. */
int  crass_hip_set_fastq_class(crass_hip_ctx *ctx, int fastq_class);
/* the pieces (files) of the context's last device load whose layout the four-line scan decided (FASTA counts here), out[0], and
 * the wrapped scan, out[1] (kseq.cpp:171-226 is what both agree with) */
int  crass_hip_last_scan_classes(const crass_hip_ctx *ctx, uint64_t out[2]);
/* replaces: the header_id argument of the load calls, for ANY resident set: header_id[n_reads] (host; NULL: all headers unique)
 * is copied to the device and the results of earlier passes are dropped, as by a load.  CRASS_ERR_STATE: no reads resident. */
int  crass_hip_set_header_ids(crass_hip_ctx *ctx, const uint64_t *header_id);
/* replaces: crass_fastx.header_id for a scanned file, on the host: header_id_out[r] = index of the first read with the same NAME,
 * the bytes behind the header character up to the first isspace() byte, compared exactly (readsFound's key, libcrispr.cpp:138,411). */
int  crass_fastx_header_ids(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, uint64_t *header_id_out);
/* replaces: the other direction of the same key, names in and first read index out — what findSingletons asks of readsFound
 * (libcrispr.cpp:411: a read whose NAME was found in pass 1 is not recruited) when the names come from somewhere else: a mate
 * file, another lane, another rank.  first_out[k] = the smallest r whose NAME (as crass_fastx_header_ids cuts it: the bytes behind
 * the header character at rec_pos[r] up to the first isspace() byte or the end of the bytes) equals the query
 * names[name_off[k] .. name_off[k+1]) byte for byte, CRASS_NAME_NOT_FOUND when no record has that name.  A query is raw bytes: an
 * empty one matches exactly the records with an empty name, one that holds an isspace() byte matches nothing.  On the host, no
 * GPU needed: what crass_hip_fastx_names_find is tested against.  CRASS_ERR_INVALID_ARG: NULL arrays with counts > 0, a
 * decreasing name_off, a rec_pos[r] >= n_bytes.  n_names == 0: CRASS_OK; n_reads == 0: every query is not found. */
#define CRASS_NAME_NOT_FOUND (~0ull)
int  crass_fastx_find_names(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                            const uint8_t *names, const uint64_t *name_off, uint64_t n_names, uint64_t *first_out);
/* replaces: the same (crass_fastx.header_id, readsFound's key) for a caller whose file bytes exist only on the DEVICE, which would
 * otherwise copy the file back to feed crass_fastx_header_ids: header_id_out[r] (host, [n_reads], may be NULL) is exactly that
 * function's result on the same bytes.  Names are hashed into a device table and compared byte for byte (fastx_hid.hip): no
 * answer rests on a hash.  d_bytes: a device pointer of any alignment, read only during the call; rec_pos: the HOST array of a
 * layout (the context's own pinned one is fine), uploaded into scratch that is given back with the table (8 bytes per slot,
 * the smallest power of two >= 2 n_reads slots) before the call returns.  install != 0: as crass_hip_set_header_ids(ctx, those
 * ids) — earlier results are dropped, the array (always one, never NULL) goes device to device; needs n_reads == the resident
 * set's (else CRASS_ERR_INVALID_ARG) and reads (CRASS_ERR_STATE).  *n_repeated_out (may be NULL): reads with header_id[r] != r.
 * Errors (the resident set is untouched): CRASS_ERR_INVALID_ARG — a NULL context, NULL d_bytes or rec_pos with n_reads > 0
 * (nothing launched), a rec_pos[r] >= n_bytes (seen on the device, reported before anything is installed or written to
 * header_id_out); CRASS_ERR_UNSUPPORTED — n_reads >= 2^32 - 1.  n_reads == 0: CRASS_OK.
 * CRASS_HID_TEST_HASH_BITS=b (read when the context is created): only the low b bits of a name's hash are kept, so that a few
 * names make long probe chains and equal tags (tests). */
int  crass_hip_fastx_header_ids_device(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                       uint64_t *header_id_out, int install, uint64_t *n_repeated_out);
/* HIP-event time, in milliseconds on the context's stream, of the last crass_hip_fastx_header_ids_device call's kernels: part 0
 * first to last, 1 the insert launches (the host's look at the count of long names included), 2 the lookup launch; measured when
 * the stage timing level is >= 1, else 0.  (No reference counterpart: crass has no timers.) */
float crass_hip_last_header_ids_ms(const crass_hip_ctx *ctx, int part);
/* replaces: crass_fastx_find_names (readsFound's lookup by NAME, libcrispr.cpp:411) for a caller whose file bytes exist only on
 * the DEVICE and whose names come from elsewhere (crass_amd/distributed.py: the found headers of other ranks), which would
 * otherwise copy the file back.  build: the insert step of crass_hip_fastx_header_ids_device (the same kernels, slots, table size
 * and CRASS_HID_TEST_HASH_BITS), but the table and the device copy of rec_pos (HOST array, [n_reads]) are KEPT by the context: 8
 * bytes per slot + 8 per record until crass_hip_fastx_names_drop, the next build, or destroy.  The table refers to d_bytes (names
 * are compared byte for byte): the caller keeps those bytes alive and unchanged for as long.  d_bytes == NULL && rec_pos == NULL:
 * the arena and layout of the last crass_hip_load_fastx_files (n_bytes and n_reads are ignored; CRASS_ERR_STATE if there is none);
 * any load or attach on the context drops a table built on the arena.
 * find: first_out[k] (host, [n_names]) is exactly crass_fastx_find_names' answer on the bytes and rec_pos of the build; names and
 * name_off ([n_names + 1]) are HOST arrays, uploaded into scratch that is given back before the call returns.  Nothing outside
 * [names, names + name_off[n_names]) and [d_bytes, d_bytes + n_bytes) is read; no answer rests on a hash, and none depends on
 * scheduling (the table is final: k_hid_find / k_hid_find_long only read).  Any number of find calls may follow one build.
 * Errors (the table before and the resident set are untouched): CRASS_ERR_INVALID_ARG — a NULL context, NULL arrays with counts
 * > 0, a decreasing name_off, a rec_pos[r] >= n_bytes (seen on the device, reported as crass_hip_fastx_header_ids_device reports
 * it; the build then keeps no table of its own); CRASS_ERR_STATE — find without a table; CRASS_ERR_UNSUPPORTED — n_reads or
 * n_names >= 2^32 - 1.  n_names == 0 (with a table): CRASS_OK.  n_reads == 0 (with a non-NULL pointer): build is CRASS_OK and every query is
 * CRASS_NAME_NOT_FOUND.  drop without a table: CRASS_OK.
 * Queries that are already in device memory: crass_hip_fastx_names_find_device, below. */
int  crass_hip_fastx_names_build_device(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads);
int  crass_hip_fastx_names_find(crass_hip_ctx *ctx, const uint8_t *names, const uint64_t *name_off, uint64_t n_names, uint64_t *first_out);
int  crass_hip_fastx_names_drop(crass_hip_ctx *ctx);
/* ---- the found-name exchange with everything in device memory: names out, looked up, marked ----
 * replaces: the name cut of kseq for listed records, on the host (no GPU): the statement of the rule the device call below is
 * tested against.  Entry k is record idx[k] - idx_base (any order, repeats allowed); its NAME, as crass_fastx_header_ids cuts it,
 * goes to out at off_out[k]; off_out ([n + 1], never NULL) holds the offsets and the total.  CRASS_ERR_OVERFLOW: cap_bytes <
 * off_out[n] — the offsets are complete, the first cap_bytes bytes are written and nothing at or beyond out + cap_bytes is.
 * CRASS_ERR_INVALID_ARG: a NULL off_out, NULL arrays with counts > 0, an index outside [idx_base, idx_base + n_reads), a
 * rec_pos >= n_bytes — nothing is written to out.  n == 0: CRASS_OK, off_out[0] = 0. */
int  crass_fastx_names_of(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, const uint64_t *idx, uint64_t n,
                          uint64_t idx_base, uint8_t *out, uint64_t cap_bytes, uint64_t *off_out);
/* replaces: crass_hip_fetch_header_lines_device plus the host's cut at the name, for a caller who hands the names to another
 * stream or device: the same names of records of the table crass_hip_fastx_names_build_device keeps (k_nm_measure_idx, a
 * three-launch prefix sum, k_nm_copy).  d_idx ([n]), d_chars ([cap_bytes], any alignment) and d_off ([n + 1], never NULL) are
 * DEVICE memory of the context's device; *total_out (host, may be NULL) is the call's one host read.  The call returns after its
 * kernels have finished.  CRASS_ERR_STATE: no table.  CRASS_ERR_OVERFLOW: cap_bytes < total — *total_out and d_off are complete,
 * the first cap_bytes bytes are written and nothing at or beyond d_chars + cap_bytes is (the rule of crass_hip_fetch_text_device).
 * CRASS_ERR_INVALID_ARG: a NULL context or d_off, NULL arrays with counts > 0 (nothing launched), an entry outside [idx_base,
 * idx_base + n_reads) (seen on the device: d_off holds length 0 for it, no byte is written).  CRASS_ERR_UNSUPPORTED: n >= 2^32 - 1.
 * n == 0: CRASS_OK, d_off[0] = 0. */
int  crass_hip_fastx_names_of_device(crass_hip_ctx *ctx, const uint64_t *d_idx, uint64_t n, uint64_t idx_base, uint8_t *d_chars, uint64_t cap_bytes,
                                     uint64_t *d_off, uint64_t *total_out);
/* replaces: crass_hip_get_candidates + crass_hip_fetch_header_lines_device + the cut at the name (what a rank publishes for the
 * found headers of other ranks): the names of this context's pass-1 records, in record order, without the caller holding their
 * indices — they are read where pass 1 left them on the device, with idx_base = the set's read_index_base.  A step without a
 * device copy of them (the long reads' host-loop sink) uploads the host list: the only host array this call may send.
 * d_off: DEVICE [cap_names + 1] (may be NULL with cap_names == 0); *n_out (never NULL) the records, *total_out the bytes.
 * CRASS_ERR_STATE: no table, or no pass 1.  CRASS_ERR_OVERFLOW: cap_names < *n_out (nothing of the caller's is written; both
 * counts are filled) or cap_bytes < *total_out (as above).  Other errors as crass_hip_fastx_names_of_device. */
int  crass_hip_found_names_device(crass_hip_ctx *ctx, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *d_off, uint64_t cap_names, uint64_t *n_out,
                                  uint64_t *total_out);
/* replaces: crass_hip_fastx_names_find for queries that are in DEVICE memory (another rank's crass_hip_found_names_device, copied
 * device to device): d_names ([n_name_bytes], any alignment), d_name_off ([n_names + 1]) and d_first_out ([n_names]) are device
 * memory of the context's device; the answers are crass_fastx_find_names' (the hash, probe and comparison of k_hid_find).  Nobody
 * on the host has seen the offsets: k_hid_find_dev checks them, and lists the queries of 260 bytes or more for k_hid_find_long
 * itself — the host reads that count and one flag.  The call returns after its kernels have finished.  CRASS_ERR_STATE: no table.
 * CRASS_ERR_INVALID_ARG: a NULL context, NULL arrays with counts > 0 (nothing launched), a decreasing offset pair or an offset
 * beyond n_name_bytes (seen on the device: such a query reads nothing and answers CRASS_NAME_NOT_FOUND, the others are answered).
 * CRASS_ERR_UNSUPPORTED: n_names >= 2^32 - 1.  n_names == 0: CRASS_OK.  A table of no records: every answer is
 * CRASS_NAME_NOT_FOUND. */
int  crass_hip_fastx_names_find_device(crass_hip_ctx *ctx, const uint8_t *d_names, uint64_t n_name_bytes, const uint64_t *d_name_off,
                                       uint64_t n_names, uint64_t *d_first_out);
/* entries per tile of the prefix sum of crass_hip_fastx_names_of_device (tests place n on its edges) */
uint32_t crass_hip_names_scan_tile(void);
/* HIP-event time, in milliseconds on the context's stream: part 0 the insert launches of the last crass_hip_fastx_names_build_device
 * (the host's look at the count of long names included), 1 the kernels of the last crass_hip_fastx_names_find; measured when the
 * stage timing level is >= 1, else 0.  (No reference counterpart: crass has no timers.) */
float crass_hip_last_names_ms(const crass_hip_ctx *ctx, int part);
/* bytes one workgroup of the device scan handles per tile; tiles start at multiples of it counted from the 16-byte aligned
 * address at or below the bytes (tests place line and record edges on tile edges) */
uint32_t crass_hip_fastx_tile_bytes(void);
/* HIP-event time, in milliseconds on the context's stream, of the scan kernels (first to last, the host's look at the totals
 * between them included) of the last crass_hip_load_fastx_bytes / crass_hip_attach_device_fastx call; measured when the stage timing
 * level is >= 1, else 0; crass_hip_last_pack_ms then holds the pack kernel's.  (No reference counterpart: crass has no timers.) */
float crass_hip_last_scan_ms(const crass_hip_ctx *ctx);
/* ---- BGZF-compressed input, inflated on the device (inflate.hip) ----
 * replaces: getFileHandle / gzopen (SeqUtils.cpp:100-126) for a .gz input written as BGZF (bgzip; Illumina's converters): a
 * series of gzip members of at most 64 KB of text, each naming its compressed size in a 'BC' extra subfield and its text size in
 * its trailer, so that the members' places in the input and in the output are known before anything is inflated and the members
 * inflate side by side.  A file is either inflated exactly (the bytes zlib gives) or declined with a verdict; plain single-member
 * gzip is declined (reason 10) and stays with the host readers.
 * reason: 0 accepted, 1 block type 3, 2 stored block LEN != ~NLEN, 3 code lengths (over-subscribed or incomplete code — but a
 * single distance code of one bit —, repeat code 16 first, a repeat past HLIT + HDIST, no end-of-block code, HLIT > 286, HDIST > 30),
 * 4 a bit pattern that is no code, length symbol 286 / 287, distance symbol 30 / 31, 5 a distance beyond the member's own text,
 * 6 the deflate data ends before the final block does, 7 / 8 more / less text than ISIZE, 9 CRC-32, 10 not BGZF (11 .. 14: plain
 * gzip on the device, below).
 * A member's verdict is the first reason its decoder meets; the file's is that of the first offending member; in_pos is the file
 * position of that member's first byte.  Bits between a member's final block and its trailer are ignored. */
typedef struct {
    int32_t reason; uint64_t member; uint64_t in_pos;
} crass_bgzf_verdict;
typedef struct {
    uint64_t n_members;
    uint64_t *in_off;                      /* [n_members+1] member m is bytes[in_off[m] .. in_off[m+1]) */
    uint64_t *out_off;                     /* [n_members+1] ... and inflates to text[out_off[m] .. out_off[m+1]) */
    uint64_t *data_off;                    /* [n_members] where member m's deflate data starts; it ends 8 bytes before in_off[m+1] */
    crass_bgzf_verdict decline;            /* reason 10 and the member that does not parse, when declined */
} crass_bgzf_index;
/* replaces: the same (gzopen's view of the file as one stream) — the walk over the members' headers and trailers, on the host: accepts
 * what the host readers' side-by-side inflate accepts (the 28-byte end-of-file member, empty members anywhere, further extra
 * subfields around 'BC'), with one difference: data_off honours FNAME / FCOMMENT / FHCRC, which that walk never looks at, so a
 * member in which those fields run into the trailer is declined here; everything else: CRASS_ERR_UNSUPPORTED, out->decline filled, arrays NULL.  The arrays are malloc'd:
 * crass_bgzf_index_free. */
int  crass_bgzf_index_host(const uint8_t *bytes, uint64_t n_bytes, crass_bgzf_index *out);
void crass_bgzf_index_free(crass_bgzf_index *ix);
/* replaces: gzread (SeqUtils.cpp:100-126) — member after member through the decoder the kernel runs (inflate_core.h), on the host, no
 * GPU needed: what the device is tested against.  CRASS_OK: out[0 .. out_off[n]) is the text.  CRASS_ERR_UNSUPPORTED: declined, *v
 * (may be NULL) says why; out's contents are unspecified, nothing outside [out, out + out_cap) is written.  CRASS_ERR_INVALID_ARG:
 * NULL pointers with work to do, out_cap < out_off[n], an index that is not ascending or reaches beyond n_bytes. */
int  crass_bgzf_inflate_host(const uint8_t *bytes, uint64_t n_bytes, const crass_bgzf_index *index, uint8_t *out, uint64_t out_cap,
                             crass_bgzf_verdict *v);
/* replaces: gzread (SeqUtils.cpp:100-126) for compressed bytes that are in HBM: d_in and d_out are caller-owned DEVICE pointers of any
 * alignment, index is the HOST index of the same bytes; its offsets go up into scratch that is given back before the call returns.
 * One wave inflates one member (k_bgzf_inflate).  CRASS_OK: d_out[0 .. out_off[n]) equals zlib's text.  CRASS_ERR_UNSUPPORTED:
 * declined, *v (may be NULL) equals crass_bgzf_inflate_host's verdict, d_out's contents are unspecified.  CRASS_ERR_INVALID_ARG (checked
 * on the host, nothing is launched): as crass_bgzf_inflate_host.  The resident set is untouched either way. */
int  crass_hip_inflate_bgzf_device(crass_hip_ctx *ctx, const uint8_t *d_in, uint64_t n_in, const crass_bgzf_index *index, uint8_t *d_out,
                                   uint64_t out_cap, crass_bgzf_verdict *v);
/* replaces: getFileHandle / gzopen + the kseq_read loop (SeqUtils.cpp:100-126, libcrispr.cpp:96-131) for a BGZF file's bytes in HOST
 * memory: index on the host, the compressed bytes up through the staged buffers of crass_hip_load_text, inflate, then the device scan
 * and pack of crass_hip_attach_device_fastx on the text — accepted means exactly what that call gives on the inflated bytes.
 * d_text == NULL: the text lives in context scratch that is given back before the call returns.  d_text (DEVICE, d_text_cap >= the
 * text's size, else CRASS_ERR_INVALID_ARG): the text stays there for crass_hip_fastx_header_ids_device /
 * crass_hip_fetch_header_lines_device; its size is out->rec_pos[n_reads].  CRASS_ERR_UNSUPPORTED: a compression decline fills *v
 * (may be NULL), a FASTA / FASTQ decline fills out->decline_reason (v->reason stays 0); no reads are resident either way. */
int  crass_hip_load_fastx_bgzf(crass_hip_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                               uint8_t *d_text, uint64_t d_text_cap, crass_fastx_layout *out, crass_bgzf_verdict *v);
/* HIP-event time, in milliseconds on the context's stream, of the inflate kernel of the last crass_hip_inflate_bgzf_device /
 * crass_hip_load_fastx_bgzf call; measured when the stage timing level is >= 1, else 0.  (No reference counterpart: crass has no
 * timers.) */
float crass_hip_last_inflate_ms(const crass_hip_ctx *ctx);
/* ---- plain gzip input, inflated on the device chunk by chunk (gunzip.hip) ----
 * replaces: getFileHandle / gzopen + gzread (SeqUtils.cpp:100-126) for a .gz input as gzip / pigz write it: ONE member, one deflate
 * stream.  The stream is cut into chunks of about chunk_bytes (0: the default, 256 KB; at least 4096, at most 4 MB); a chunk is entered at the
 * first dynamic block start found inside it, bytes copied from the unknown 32 KB in front of a chunk are carried as 16-bit
 * markers and resolved afterwards, and the result is accepted only with the trailer's length and CRC-32 (gunzip_core.h).  A file
 * is either inflated exactly (the bytes zlib gives) or declined with a crass_bgzf_verdict whose `member` is the offending CHUNK
 * (the first in text order) and whose in_pos is the file byte that holds that chunk's start bit (0 for header and trailer reasons).
 * reason: 1 .. 6 as above, 7 / 8 more / less text than ISIZE, 9 CRC-32, 11 not a gzip header (magic, method, reserved flags,
 * header CRC) or a header that runs into the trailer, 12 a chunk met no later chunk's block start within 32 chunks (stored or
 * fixed blocks throughout, blocks much longer than a chunk: take a larger chunk_bytes), 13 the member ends before the input does
 * (further members, trailing bytes), 14 a distance that reaches in front of the text's first byte. */
#define CRASS_GZIP_LINK_END        0xFFFFFFFFu   /* the chunk ran to the final block's end */
#define CRASS_GZIP_LINK_UNFINISHED 0xFFFFFFFEu   /* ... gave up at the span's end */
#define CRASS_GZIP_LINK_BAD        0xFFFFFFFDu   /* ... met a fault */
#define CRASS_GZIP_LINK_NONE       0xFFFFFFFCu   /* no start was found in the chunk */
typedef struct {
    uint64_t n_chunks, n_chain;            /* chunks of the deflate data; how many of them the text is made of */
    uint64_t *start_bit;                   /* [n_chunks] the bit of the deflate data where chunk k is entered, ~0: nowhere */
    uint32_t *link;                        /* [n_chunks] the chunk whose start this one ran into, or CRASS_GZIP_LINK_* */
    uint64_t *text_len;                    /* [n_chunks] the text between the chunk's start and its link */
} crass_gzip_plan;
void crass_gzip_plan_free(crass_gzip_plan *plan);
/* replaces: gzread (SeqUtils.cpp:100-126) — the rule above as a serial run on the host, no GPU needed: what the kernels are tested
 * against.  CRASS_OK: out[0 .. *n_text) is the text.  CRASS_ERR_OVERFLOW: out_cap < *n_text, *n_text is filled and nothing is
 * written (out NULL with out_cap 0 asks for the size).  CRASS_ERR_UNSUPPORTED: declined, *v (may be NULL) says why; out's contents
 * are unspecified.  plan (may be NULL) reports what the rule decided, whenever the header parsed; its arrays are malloc'd:
 * crass_gzip_plan_free.  CRASS_ERR_INVALID_ARG: NULL n_text, NULL bytes / out with a size. */
int  crass_gzip_inflate_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_text,
                             crass_gzip_plan *plan, crass_bgzf_verdict *v);
/* replaces: gzread (SeqUtils.cpp:100-126) — the rule as the ranks of a group run it (crass_hip_group_inflate_gzip), serially on the
 * host, no GPU needed: what that call is tested against.  The text [0, T) is cut into n_ranges (1 .. 64) ranges at nominal
 * (n_ranges - 1 non-decreasing text positions <= T; NULL: T k / n_ranges); a range takes the chain elements that hold its text (an
 * element cut by a position is both neighbours'), decodes them to symbols and walks their windows SYMBOLICALLY from an identity
 * entry window (an entry is a byte or a reference into the unknown 32 KB in front of the range's first element); the ranges'
 * entry windows are composed in order, each range resolves and narrows, and every element's text and CRC-32 part are taken from
 * the first range that holds it.  Text, plan, verdict and the overflow / argument protocol are crass_gzip_inflate_host's, field
 * for field, for every n_ranges and every cut.  Also CRASS_ERR_INVALID_ARG: n_ranges outside 1 .. 64, cuts that decrease or lie
 * beyond T (found once T is known: the plan is filled then). */
int  crass_gzip_inflate_ranges_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint32_t n_ranges, const uint64_t *nominal,
                                    uint8_t *out, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v);
/* replaces: gzread (SeqUtils.cpp:100-126) for compressed bytes that are in HBM: d_in and d_out are caller-owned DEVICE pointers of any
 * alignment.  k_gz_find (a lane per bit position), k_gz_count and k_gz_decode (a wave per chunk), k_gz_windows, k_gz_narrow.
 * Scratch: 2 bytes per text byte plus 32 KB per chain element, given back before the call returns.  Results as
 * crass_gzip_inflate_host, the verdict and the plan field for field; CRASS_ERR_OVERFLOW is known before anything is stored.  The
 * resident set is untouched. */
int  crass_hip_inflate_gzip_device(crass_hip_ctx *ctx, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                   uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v);
/* replaces: getFileHandle / gzopen + the kseq_read loop (SeqUtils.cpp:100-126, libcrispr.cpp:96-131) for a plain gzip file's bytes in
 * HOST memory: the mirror of crass_hip_load_fastx_bgzf (default chunk size).  d_text_cap smaller than the text: CRASS_ERR_INVALID_ARG,
 * found after the count step, nothing resident. */
int  crass_hip_load_fastx_gzip(crass_hip_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                               uint8_t *d_text, uint64_t d_text_cap, crass_fastx_layout *out, crass_bgzf_verdict *v);
/* ---- plain gzip of SEVERAL members (cat of .gz files, gzip's >>, a compressor that starts a member every N records) ----
 * replaces: gzread (SeqUtils.cpp:100-126), which reads such a file as one stream.  The rule above in members mode (gunzip_core.h):
 * chunks are cut over everything between the first header and the file's last 8 bytes, a run goes on past a final block through
 * the inner trailer and the next member's header, member starts are chunk starts too, no match reaches over a member boundary, and
 * every member is accepted only with its own ISIZE and CRC-32 (k_gz_member_crc) — checked behind the decode step, since inner
 * trailers are only met by the runs.  A single-member file gives the plan of the single-member calls; those calls are unchanged and
 * go on declining further members with reason 13.
 * Verdicts: reasons 1 .. 6 and 11 .. 14 met by a run or by narrowing name the CHUNK (the first in text order) and the file byte that
 * holds its start, as above; 7 / 8 / 9 name the gzip MEMBER (the first offending one, 7 / 8 before 9 within a member) and the file
 * byte of its header; 11 for the file's first header: member 0, in_pos 0.  At an inner header: 13 without the magic or with fewer
 * than 18 bytes up to the file's end; 11 for the magic with a header the rule does not take or that runs into the file's last 8
 * bytes; 14 for a distance that reaches in front of its own member.
 * Three deliberate differences from gzread: bytes behind the last member that are no gzip header (zero padding included) are
 * declined (13) where zlib ignores them; stored-only or fixed-only data needs a chunk start every 32 chunks (12: take a larger
 * chunk_bytes) where zlib takes any size; an inner header beyond the input a chunk's run may read is declined (12). */
typedef struct {
    uint64_t n_members;
    uint64_t *in_off;                      /* [n_members+1] file byte of each member's header, in_off[n_members] = n_bytes */
    uint64_t *text_off;                    /* [n_members+1] member m inflates to text[text_off[m] .. text_off[m+1]) */
} crass_gzip_members;
void crass_gzip_members_free(crass_gzip_members *m);
/* crass_gzip_inflate_host in members mode: the same overflow and argument protocol; members (may be NULL) is filled when the file is
 * accepted, its arrays are malloc'd: crass_gzip_members_free. */
int  crass_gzip_inflate_members_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint8_t *out, uint64_t out_cap,
                                     uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v);
/* crass_gzip_inflate_members_host by the rule the ranks of a group run (crass_hip_group_inflate_gzip_members), serially on the host,
 * no GPU needed: crass_gzip_inflate_ranges_host in members mode.  Every range decodes its elements with GzEnd records of its own
 * (the member table is made from each element's first holder) and walks symbolic windows from an identity entry; an entry of the
 * window in front of an element that lies in front of the member that holds the element's first byte is DEAD — nothing may read it
 * (14) — and is written as the byte 0, so a range that holds a member boundary exports a window without references; the members'
 * CRC-32 are joined from pieces cut at member boundaries, every 64 KB and where a range's own text begins; the verdict is given
 * behind all narrowing: 14 in chain order first, then the first offending member, 7 / 8 before 9.  Text, plan, member table,
 * verdict and the overflow / argument protocol are crass_gzip_inflate_members_host's, field for field, for every n_ranges in
 * 1 .. 64 and every cut.  Also CRASS_ERR_INVALID_ARG as crass_gzip_inflate_ranges_host. */
int  crass_gzip_inflate_members_ranges_host(const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint32_t n_ranges, const uint64_t *nominal,
                                            uint8_t *out, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members,
                                            crass_bgzf_verdict *v);
/* crass_hip_inflate_gzip_device in members mode: results as crass_gzip_inflate_members_host, text, plan, members and verdict field
 * for field.  Further scratch: 24 bytes per member and 4 per 64 KB piece of text. */
int  crass_hip_inflate_gzip_members_device(crass_hip_ctx *ctx, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out,
                                           uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members,
                                           crass_bgzf_verdict *v);
/* the mirror of crass_hip_load_fastx_gzip for a file of any number of members; members (may be NULL) as above.  Members may end
 * anywhere in the text (in the middle of a record): the text as a whole is what is scanned. */
int  crass_hip_load_fastx_gzip_members(crass_hip_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                       uint8_t *d_text, uint64_t d_text_cap, crass_fastx_layout *out, crass_gzip_members *members,
                                       crass_bgzf_verdict *v);
/* crass_hip_load_fastx_files takes a plain gzip file on the terms of a BGZF one (inflated on the device into the arena): OFF (the
 * default) such a file is declined with reason 10; ONE_MEMBER takes a single-member file and declines further members (13); MEMBERS
 * takes plain gzip of any number of members.  Any other non-zero value is ONE_MEMBER.  (No reference counterpart.) */
#define CRASS_GZIP_ON_DEVICE_OFF        0
#define CRASS_GZIP_ON_DEVICE_ONE_MEMBER 1
#define CRASS_GZIP_ON_DEVICE_MEMBERS    2
int  crass_hip_set_gzip_on_device(crass_hip_ctx *ctx, int on);
/* HIP-event milliseconds of the last gzip inflate's five steps, ms[0 .. 5): find, count, decode, windows, narrow; measured when the
 * stage timing level is >= 1, else 0.  crass_hip_last_inflate_ms holds their sum.  (No reference counterpart.) */
int  crass_hip_last_gzip_ms(const crass_hip_ctx *ctx, float *ms);
/* ---- the text of selected reads, out of the resident set ----
 * n records back to back: record k is chars[off[k] .. off[k+1]), off[n+1] the exclusive prefix sum of the records' lengths.
 * The gather and the unpacking run on the device (k_fetch_text, pack.hip), where the words are: only the selected reads'
 * bytes move.  Reads without an exception come back as A C G T from their codes; exception reads as the raw bytes they were
 * loaded with ('N', lower case, 0x00, 0xFF).  revcomp[k] != 0 (revcomp may be NULL: none) gives the reverse complement by
 * reverseComplement's table (SeqUtils.cpp:50-59): byte i = table[byte[len - 1 - i] & 127].  Works on every resident set,
 * however it was loaded or attached; a read may be listed more than once.
 * Errors (nothing is launched, the resident set is untouched): CRASS_ERR_INVALID_ARG — a NULL context or result pointer, a
 * NULL index array with n > 0, an index outside [read_index_base, read_index_base + n_reads), a pass other than 1 or 2;
 * CRASS_ERR_STATE — no reads resident, no results of that pass. */
typedef struct {
    uint64_t        n;
    const uint8_t  *chars;         /* off[n] bytes                                                   */
    const uint64_t *off;           /* [n+1]                                                          */
} crass_text;
/* replaces: the second reading of the input files in findSingletons (the getFileHandle / kseq_read loop of libcrispr.cpp:471-487)
 * and any host copy of the text a caller kept only to look up the reads the search returned.  read_idx: GLOBAL indices
 * (read_index_base + local) — crass_candidates.read_idx and crass_recruits.read_idx as they are.  The result lives in the
 * context's pinned memory, valid until the next fetch, load or destroy.  One copy up per array, an exact-size copy back, one
 * host wait; n == 0 (or empty reads only): an empty result, nothing launched, no wait. */
int crass_hip_fetch_text(crass_hip_ctx *ctx, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, crass_text *out);
/* replaces: the same loop (libcrispr.cpp:471-487) for a caller whose next stage is on the device: the text goes into the caller's
 * DEVICE buffer d_chars (cap_bytes bytes, any alignment; a torch uint8 tensor), the offsets into the host array off_out[n+1].
 * cap_bytes < off_out[n]: CRASS_ERR_OVERFLOW with off_out filled and nothing written to d_chars — size the buffer from off_out[n]
 * and call again (d_chars may be NULL when cap_bytes is 0).  No byte at or beyond d_chars + off_out[n] is written. */
int crass_hip_fetch_text_device(crass_hip_ctx *ctx, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n,
                                uint8_t *d_chars, uint64_t cap_bytes, uint64_t *off_out);
/* replaces: ReadHolder's RH_Seq (ReadHolder.h; filled from the kseq record at libcrispr.cpp:471-487 and reversed by DRLowLexi,
 * ReadHolder.cpp:513-591) for every record of the last pass 1 (pass == 1: the candidates, in crass_hip_get_candidates' order) or
 * pass 2 (pass == 2: the recruits, in crass_hip_get_recruits' order): record k = low_lexi[k] ? seq : revcomp(seq) of the read
 * read_idx[k] — what crass_graph_input.seq_chars takes. */
int crass_hip_fetch_record_text(crass_hip_ctx *ctx, int pass, crass_text *out);
/* HIP-event time, in milliseconds on the context's stream, of the fetch kernel of the last crass_hip_fetch_* call; measured
 * when the stage timing level is >= 1 (crass_hip_set_stage_timing), else 0.  (No reference counterpart: crass has no timers.) */
float crass_hip_last_fetch_ms(const crass_hip_ctx *ctx);
/* replaces: ReadHolder's RH_Header / RH_Comment (filled from the kseq record at libcrispr.cpp:471-487) for a caller whose file
 * bytes exist only on the device: the header LINES of the records idx[0..n) (LOCAL record numbers in [0, n_reads), any order,
 * repeats allowed) back to back — record k is the bytes from rec_pos[idx[k]] + 1 up to, not including, the '\n' that ends the
 * line, or up to n_bytes (a '\r' in front of the '\n' stays).  name_len_out[k] (host [n], may be NULL): the length of the NAME at
 * the line's start (the bytes up to the first isspace() byte, as above): the caller cuts header and comment there.  The result
 * follows crass_hip_fetch_text: a crass_text in the context's pinned memory (its own, not that of the text fetches), valid until
 * the next call of this function, or destroy.  Errors (nothing launched): CRASS_ERR_INVALID_ARG — a NULL context or result
 * pointer, NULL d_bytes or rec_pos with n_reads > 0, a NULL idx with n > 0, an idx[k] >= n_reads, a rec_pos[idx[k]] >= n_bytes;
 * CRASS_ERR_UNSUPPORTED — n_reads >= 2^32 - 1.  Needs no resident reads. */
int  crass_hip_fetch_header_lines_device(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                         const uint64_t *idx, uint64_t n, crass_text *out, uint32_t *name_len_out);
/* the same into the caller's DEVICE buffer d_chars (cap_bytes bytes, any alignment), the offsets into the host array off_out[n+1],
 * by the rules of crass_hip_fetch_text_device: cap_bytes < off_out[n] is CRASS_ERR_OVERFLOW with off_out and name_len_out filled
 * and nothing written; no byte at or beyond d_chars + off_out[n] is written. */
int  crass_hip_fetch_header_lines_device_to(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                            const uint64_t *idx, uint64_t n, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *off_out,
                                            uint32_t *name_len_out);
/* ---- several input files (paired-end files, lanes) as ONE resident set, parsed on the device ----
 * replaces: crass_index_fastx_files + crass_fastx_index_reads + crass_hip_load_reads, i.e. the kseq_read loop of libcrispr.cpp:96-131
 * over every file of parseSeqFiles (WorkHorse.cpp:336-393), for a caller that holds the files' bytes in HOST memory: the job's reads in
 * (file, read) order in one packed set, header ids across the files.  Each file is taken on its own terms: byte 0 '>' or '@' — plain
 * text (FASTA and FASTQ may be mixed in one call); bytes 1f 8b and a valid BGZF index — inflated on the device (k_bgzf_inflate);
 * anything else, plain single-member gzip included — declined.
 * The ARENA: every file's text (inflated where compressed) lies in one device buffer in file order, file f at
 * [file_byte_base[f], file_byte_base[f+1] - 1); the byte behind each file's last byte is a '\n' that belongs to no file, so nothing
 * that walks a line or a name runs into the next file.  The context keeps the arena until the next load, attach or destroy
 * (crass_hip_resident_fastx); rec_pos holds ARENA positions.
 * accepted (CRASS_OK): the resident packed words, stride / uniform length, exception list, counters and seq_off are bit for bit what
 *   the three calls above give on the same files (same pad_uniform; a set whose files differ in read length is ragged exactly as the
 *   host packer makes it) — with one exception: in the words of an EXCEPTION read, a byte that is not A C G T has crass_pack_reads'
 *   code 0 here (as after crass_hip_load_text), where the indexed reader's own packer leaves another code; the search reads such reads
 *   from the exception list, never from those words.  header_id is theirs: the index of the first read, over all files, with the same name (k_hid_insert /
 *   k_hid_lookup on the arena, installed device to device; none installed when no name repeats).
 * declined (CRASS_ERR_UNSUPPORTED): no reads are resident and no arena is kept; decline_file says which file, and either
 *   decline_reason / decline_pos (a FASTA / FASTQ decline: the reasons 1..11 of crass_fastx_layout, the position inside THAT file) or
 *   bgzf (a compression decline: bgzf.reason != 0, decline_reason 0).  When several files offend, the first file in order wins.
 *   A different answer is never an outcome.
 * Other errors: CRASS_ERR_INVALID_ARG — a NULL context, n_files == 0, NULL arrays, a NULL bytes[f] with n_bytes[f] > 0, pad_uniform
 * outside 0..2; CRASS_ERR_UNSUPPORTED without a verdict — 2^32 - 1 reads or more. */
typedef struct {
    uint32_t n_files;
    int32_t  decline_file;                 /* -1 when accepted */
    int32_t  decline_reason;               /* FASTA / FASTQ decline of that file, else 0 */
    uint32_t max_len;
    uint64_t decline_pos;                  /* position inside that file */
    crass_bgzf_verdict bgzf;               /* compression decline of that file (reason 0: none) */
    uint64_t n_reads;
    const uint64_t *file_read_base;        /* [n_files+1] first read of every file; [n_files] = n_reads */
    const uint64_t *file_byte_base;        /* [n_files+1] arena position of every file's byte 0; [n_files] = the arena's size */
    const int32_t  *format;                /* [n_files] '>' | '@' */
    const uint64_t *rec_pos;               /* [n_reads+1] arena position of each record's header character; [n_reads] = the end of the
                                              last file's text = the arena's size - 1 */
    const uint64_t *seq_off;               /* [n_reads+1] offsets in the concatenated sequence text */
} crass_fastx_files_layout;
/* the same layout on the host (no GPU needed): crass_fastx_scan_host per file, crass_bgzf_index_host + crass_bgzf_inflate_host for a
 * BGZF file — what the device call is tested against.  The arrays are malloc'd (crass_fastx_files_layout_free), NULL when declined
 * (n_files and the decline fields are always filled).  With one plain file: crass_fastx_scan_host's answer with bases 0. */
int  crass_fastx_files_scan_host(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, crass_fastx_files_layout *out);
/* the same with every FASTQ file read by a class (crass_fastx_scan_host_class; kseq.cpp:171-226): 0 is the call above */
int  crass_fastx_files_scan_host_class(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int fastq_class,
                                       crass_fastx_files_layout *out);
void crass_fastx_files_layout_free(crass_fastx_files_layout *l);
/* the device call.  Uploads go through the two staged buffers of crass_hip_load_text, file after file (a BGZF file's compressed bytes
 * into scratch, inflated from there into the arena); file f's two scan kernels are queued before file f+1 is staged, so they run
 * beside its upload.  Each file is scanned by k_fx_summary / k_fx_tile_scan / k_fx_emit with its own format and tile grid, all files
 * emit into one text and one seq_off, ONE k_pack_text launch packs the set.  out may be NULL; its arrays are context-owned pinned
 * memory, valid until the next load, attach or destroy (NULL when declined). */
int  crass_hip_load_fastx_files(crass_hip_ctx *ctx, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                                crass_fastx_files_layout *out);
/* the arena of the last crass_hip_load_fastx_files: a DEVICE pointer and its size (= file_byte_base[n_files]), for
 * crass_hip_fastx_header_ids_device, crass_hip_fetch_header_lines_device(_to) and crass_hip_fetch_quality_device(_to), which work on
 * it unchanged.  CRASS_ERR_STATE: the last load was not a files load (or was declined). */
int  crass_hip_resident_fastx(const crass_hip_ctx *ctx, const uint8_t **d_bytes, uint64_t *n_bytes);
/* replaces: ReadHolder's RH_Qual / RH_IsFasta (filled from the kseq record at libcrispr.cpp:471-487) for a caller whose file bytes
 * exist only on the device: the QUALITY strings of the records idx[0..n) (LOCAL record numbers in [0, n_reads), any order, repeats
 * allowed) back to back.  A record whose header character is '@' has its quality on its fourth line, found from rec_pos[idx[k]] by
 * three line ends and bounded by rec_pos[idx[k] + 1] (rec_pos has n_reads + 1 entries; entries beyond n_bytes count as n_bytes): the
 * string is that line's bytes 33..126 — for a regular four-line FASTQ record exactly crass_fastx_index_fetch's qual —, has_qual_out[k]
 * (host [n], may be NULL) is 1.  A '>' record gives an empty string and has_qual 0.  The result follows
 * crass_hip_fetch_header_lines_device: a crass_text in the context's pinned memory (its own), valid until the next call of this
 * function, or destroy.  Errors (nothing launched, nothing outside the bytes read): CRASS_ERR_INVALID_ARG — a NULL context or result
 * pointer, NULL d_bytes or rec_pos with n_reads > 0, a NULL idx with n > 0, an idx[k] >= n_reads, a rec_pos[idx[k]] >= n_bytes;
 * CRASS_ERR_UNSUPPORTED — n_reads >= 2^32 - 1.  n == 0: CRASS_OK, an empty result.  Needs no resident reads. */
int  crass_hip_fetch_quality_device(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                    const uint64_t *idx, uint64_t n, crass_text *out, uint8_t *has_qual_out);
/* the same into the caller's DEVICE buffer d_chars (cap_bytes bytes, any alignment), the offsets into the host array off_out[n+1], by
 * the rules of crass_hip_fetch_text_device: cap_bytes < off_out[n] is CRASS_ERR_OVERFLOW with off_out and has_qual_out filled and
 * nothing written; no byte outside [d_chars, d_chars + off_out[n]) is written. */
int  crass_hip_fetch_quality_device_to(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                       const uint64_t *idx, uint64_t n, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *off_out,
                                       uint8_t *has_qual_out);
/* replaces: the second reading of the input files (libcrispr.cpp:471-487) for a group (crass_hip_group_*): crass_hip_fetch_text
 * over the whole job.  Every global index is routed to the rank whose shard holds it; the records come back in the caller's
 * order in one crass_text owned by the group, valid until the next group fetch, load or destroy. */
int crass_hip_group_fetch_text(crass_hip_group *g, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, crass_text *out);
/* ---- the files of a job cut into record-aligned shards, one per rank of a group ----
 * replaces: nothing in crass, which reads its files in one thread; in this library it replaces the host's indexed reader
 * + crass_hip_group_load_reads in front of a group, the way crass_hip_load_fastx_files replaces it in front of one context.
 * The CUT RULE (csrc/fastx_scan.h states it once for host and device): the job's TEXT SPACE is the files' texts back to back in
 * file order (a BGZF file's text is its inflated text), T bytes in all.  nominal (may be NULL: T g / n_ranks) holds n_ranks - 1
 * non-decreasing positions in [0, T].  A record start is every file's position 0, every line start whose byte is '>' in a file
 * whose byte 0 is '>', and every line start of line index 0 modulo 4 in a file whose byte 0 is '@'.  The actual cut c_g is the
 * smallest record start at or after nominal cut g, or T; rank g owns [c_g, c_{g+1}) and may be empty.
 * cut_file / cut_pos [n_ranks+1]: the file and the text position inside it of every actual cut ([n_ranks] = (n_files, 0));
 * rank_read_base [n_ranks+1]: the records in front of every cut, rank g holds reads [rank_read_base[g], rank_read_base[g+1]);
 * file_read_base [n_files+1] and format [n_files] as in crass_fastx_files_layout.  The decline fields are that layout's. */
typedef struct {
    uint32_t n_ranks, n_files;
    int32_t  decline_file;                 /* -1 when accepted */
    int32_t  decline_reason;
    uint64_t decline_pos;
    crass_bgzf_verdict bgzf;
    uint64_t n_reads;
    uint32_t max_len;
    const uint64_t *rank_read_base;
    const uint32_t *cut_file;
    const uint64_t *cut_pos;
    const uint64_t *file_read_base;
    const int32_t  *format;
} crass_fastx_shards;
/* the shards on the host, no GPU needed: what the group's load is tested against.  Exact: the verdict is
 * crass_fastx_files_scan_host's, field for field, whatever the cuts (the first offending file wins, inside it the smallest
 * (line position, reason)); the cuts are the rule's.  The arrays are malloc'd (crass_fastx_shards_free), NULL when the input is
 * declined (n_ranks, n_files and the decline fields are always filled).  Errors: CRASS_ERR_INVALID_ARG — as
 * crass_fastx_files_scan_host, n_ranks outside 1..64, nominal cuts that decrease or lie beyond T; CRASS_ERR_UNSUPPORTED —
 * declined; CRASS_ERR_OOM. */
int  crass_fastx_files_shards_host(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, uint32_t n_ranks,
                                   const uint64_t *nominal, crass_fastx_shards *out);
void crass_fastx_shards_free(crass_fastx_shards *s);
/* the same for a FASTQ class (crass_hip_group_set_fastq_class).  0 is crass_fastx_files_shards_host, byte for byte.  1: the record
 * starts of a file whose byte 0 is '@' are the header-line positions of the records the wrapped rule walks from line 0
 * (crass_fastx_scan_host_class(.., 1, ..)) — a quality line that starts with '@' is none, whatever follows it; FASTA files keep
 * their definition; the verdict is crass_fastx_files_scan_host_class(.., 1, ..)'s, field for field, whatever the cuts.
 * CRASS_ERR_INVALID_ARG also for a class outside 0..1. */
int  crass_fastx_files_shards_host_class(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, uint32_t n_ranks,
                                         const uint64_t *nominal, int fastq_class, crass_fastx_shards *out);
/* replaces: the same, for a job whose plain gzip files are taken as their text.  gzip_mode 0 is
 * crass_fastx_files_shards_host_class, the decline of a plain gzip file (reason 10) included.  gzip_mode != 0: a file that starts
 * with the gzip magic and that crass_bgzf_index_host declines as not BGZF is replaced by crass_gzip_inflate_host's text
 * (chunk_bytes: 0 is the default chunk) and the job is then cut and judged like any other; a file that does not inflate is the
 * job's decline (decline_file, bgzf = that call's verdict; several members: 13) unless a file in front of it is declined.
 * gzip_mode == CRASS_GZIP_ON_DEVICE_MEMBERS: such a file is replaced by crass_gzip_inflate_members_host's text, a file of any
 * number of members; one that does not inflate gives that call's verdict. */
int  crass_fastx_files_shards_host_gzip(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, uint32_t n_ranks,
                                        const uint64_t *nominal, int fastq_class, int gzip_mode, uint64_t chunk_bytes,
                                        crass_fastx_shards *out);
/* what a rank knows about a byte range of one file's text before the cuts are known (the probe of csrc/fastx_scan.h), serially
 * on the host and by k_fx_cut_probe on bytes in HBM (d_bytes: a DEVICE pointer of any alignment; one aligned 16-byte load per 16
 * bytes, nothing outside the vectors that cover the range is read).  left_is_ls: position 0 of the range is a line start.
 * out: [0] the '\n' bytes, [1] how many line starts follow (at most 4), [2..6) the first four line starts, [6] the first line
 * start whose byte is '>'; positions count from the range's first byte, ~0 where there is none.  The two agree word for word.
 * Errors: CRASS_ERR_INVALID_ARG — NULL pointers with n_bytes > 0, a NULL out or context; CRASS_ERR_HIP. */
int  crass_fastx_cut_probe_host(const uint8_t *bytes, uint64_t n_bytes, int left_is_ls, uint64_t out[7]);
int  crass_hip_fastx_cut_probe_device(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, int left_is_ls, uint64_t out[7]);
/* HIP-event time, in milliseconds on the context's stream, of the last k_fx_cut_probe launch of that call; measured when the
 * stage timing level is >= 1, else 0. */
float crass_hip_last_cut_probe_ms(const crass_hip_ctx *ctx);
/* the same for the cut kernels of a wrapped-mode load of a group (k_fw_summary .. k_fw_cut_jump over the rank's pieces, every
 * rebuild after a margin doubling included), summed over the context's part of the last crass_hip_group_load_fastx_files */
float crass_hip_last_cut_chain_ms(const crass_hip_ctx *ctx);
/* the device call: every rank of the group parses its own shard of the files beside the others (the rank threads of
 * crass_hip_group_load_reads).  Each rank stages the bytes of its NOMINAL range (plain bytes from the caller's memory; of a BGZF
 * file the members that overlap the range, inflated by k_bgzf_inflate), probes them with k_fx_cut_probe, the host combines the
 * probes into the actual cuts, each rank drops the head in front of its cut and adds the tail behind its nominal end (the few
 * bytes up to the next rank's cut, or the further BGZF members), and then does on its slices what crass_hip_load_fastx_files does
 * on whole files: k_fx_summary / k_fx_tile_scan / k_fx_emit per slice, one k_pack_text, header ids by k_hid_insert /
 * k_hid_lookup, and a name table on its arena (crass_hip_fastx_names_build_device).  A file's bytes cross the bus once, apart
 * from those tails.  Rank r's read_index_base is rank_read_base[r]; the exchange's row capacity comes from the largest shard.
 * exact: out (may be NULL) equals crass_fastx_files_shards_host's, its arrays group-owned and valid until the next group load
 *   or destroy; the reads, their text, header lines and quality (crass_hip_group_fetch_*) are those of crass_hip_load_fastx_files
 *   on the same files.  A rank's packed layout (uniform or ragged) is its own; no result depends on it.
 *   Names that repeat across ranks: after the merge of a step every rank looks the names of the other ranks' pass-1 records up
 *   in its own table, and its namesakes are marked found before pass 2 (readsFound, libcrispr.cpp:138,411).
 * declined (CRASS_ERR_UNSUPPORTED): the verdict of crass_fastx_files_shards_host in out; no rank holds reads, and the group is as
 *   after a failed load (step: CRASS_ERR_STATE).  Plain gzip is declined unless crass_hip_group_set_gzip_on_device is on: then
 *   the ranks inflate such a file together first (one deflate stream IS cut: crass_hip_group_inflate_gzip).
 * FASTQ class 1 (crass_hip_group_set_fastq_class; default 0: everything above, unchanged): the load takes at most two attempts.
 *   Attempt 1 is the load above; accepted, it is the load (a four-line job takes the same kernels as with class 0).  Attempt 2
 *   runs only when attempt 1 declines a file whose format is '@' with one of the reasons 3 .. 9: every '@' file is then cut and
 *   scanned by the wrapped rule.  A rank stages its piece [a, b) of such a file with a margin behind it (256 KiB;
 *   CRASS_SHARD_MARGIN=<bytes> at group creation), builds the piece's line table (k_fw_summary / k_fw_tile_scan / k_fw_lines),
 *   every '@' line's successor up to where the chain leaves the piece (k_fw_cut_next) and doubles the pointers (k_fw_cut_jump);
 *   the host walks the ranks in piece order with one k_fw_cut_lookup per piece, a rank whose chain is unresolved at its staged
 *   end doubles its margin and builds again; the slices go through the wrapped scan as a single context's class 1 does.
 *   exact: out equals crass_fastx_files_shards_host_class(.., 1, ..)'s, accepted or declined, and the reads, header lines,
 *   quality and comments are those of crass_hip_load_fastx_files with class 1 on the same files.
 *   Line indices of a piece are 32-bit: a piece of more lines is CRASS_ERR_UNSUPPORTED.  A plain gzip file taken
 *   by crass_hip_group_set_gzip_on_device (the group's counterpart of crass_hip_set_gzip_on_device) is cut by its text like any other.
 * Other errors: CRASS_ERR_INVALID_ARG — a NULL group, n_files == 0, NULL arrays, a NULL bytes[f] with n_bytes[f] > 0, pad_uniform
 * outside 0..2, nominal cuts that decrease or lie beyond T; CRASS_ERR_HIP / CRASS_ERR_OOM from a rank. */
int  crass_hip_group_load_fastx_files(crass_hip_group *g, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files,
                                      int pad_uniform, const uint64_t *nominal, crass_fastx_shards *out);
/* the class the group's files load reads FASTQ by; also set on every rank's context (crass_hip_set_fastq_class), so
 * crass_hip_group_fetch_quality reads quality by the wrapped rule.  CRASS_DEVICE_FASTQ=wrapped|four-line at group creation does
 * the same.  CRASS_ERR_INVALID_ARG: a NULL group, a class outside 0..1. */
int  crass_hip_group_set_fastq_class(crass_hip_group *g, int fastq_class);
/* the last crass_hip_group_load_fastx_files: out[0] its attempts (1 or 2; 0: the call failed before the ranks ran), out[1] the
 * files cut by the wrapped rule (the '@' files in front of the first declined file, in attempt 2), out[2] margin doublings and
 * out[3] chain look-ups, both summed over the ranks. */
int  crass_hip_group_load_counters(const crass_hip_group *g, uint64_t out[4]);
/* ---- one plain gzip file inflated across the ranks of a group ----
 * replaces: gzread (SeqUtils.cpp:100-126) for a .gz input of ONE member whose bytes are in HOST memory; the text comes back to host
 * memory (out_host, out_cap bytes).  One deflate stream is cut without any rank waiting for the rank in front of it
 * (gunzip_core.h, crass_gzip_inflate_ranges_host): chunk k of the nc chunks is rank k N / nc's for k_gz_find and k_gz_count (a
 * rank stages only the compressed bytes its chunks' runs may read), the host gathers the starts between the two and walks the chain;
 * rank r then takes the chain elements that hold its range of the text (nominal: N - 1 text positions, NULL: T k / N), fetches
 * what their runs still need, decodes them (k_gz_decode) and walks their windows symbolically (k_gz_windows_sym); the host composes
 * the ranks' entry windows, 32 768 look-ups per rank; every rank resolves (k_gz_window_resolve) and narrows (k_gz_narrow).  An
 * element's text and CRC-32 part come from the first rank that holds it; the host joins the parts over the chain.
 * exact: text, plan and verdict are crass_gzip_inflate_ranges_host's with n_ranges = the group's size and the same cuts, which are
 * crass_gzip_inflate_host's; the overflow protocol is crass_hip_inflate_gzip_device's (CRASS_ERR_OVERFLOW with *n_text, known
 * before anything is stored).  A file of several members is declined (13).  Scratch goes back before the call returns; the
 * ranks' resident sets and the group's state are untouched.  Errors: CRASS_ERR_INVALID_ARG — a NULL group or n_text, NULL bytes /
 * out_host with a size, cuts that decrease or lie beyond the text; CRASS_ERR_HIP / CRASS_ERR_OOM from a rank. */
int  crass_hip_group_inflate_gzip(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal,
                                  uint8_t *out_host, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v);
/* crass_hip_group_inflate_gzip for a plain gzip file of ANY number of members (cat of .gz files, gzip's >>, a member every N
 * records): the members rule (gunzip_core.h) by ranges.  k_gz_find_members / k_gz_count_members over a rank's chunks (the rank whose
 * runs see the region's end also stages the file's last 8 bytes); rank 0 walks the chain and places the member-end records
 * (gz_places); k_gz_decode_members writes a rank's records at slots relative to its first element's, the records of every element
 * come from its first holder; k_gz_windows_sym_members writes DEAD window entries — those in front of the member that holds the
 * element's first byte, which nothing may read (14) — as the byte 0, so a rank whose range holds a member boundary exports a
 * window without references and the rank behind it needs nothing from the ranks in front; rank 0 builds the member table and
 * the text cuts of the CRC pieces (member boundaries, every 64 KB, where a rank's own text begins); every rank resolves, narrows
 * with its elements' member starts (k_gz_narrow_members) and runs k_gz_member_crc over its own pieces; rank 0 joins the pieces
 * per member.  exact: text, plan, member table and verdict are crass_gzip_inflate_members_ranges_host's with n_ranges = the
 * group's size and the same cuts, which are crass_gzip_inflate_members_host's: 14 in chain order first, then the first offending
 * member, 7 / 8 before 9.  members (may be NULL) as in crass_gzip_inflate_members_host.  Errors as crass_hip_group_inflate_gzip. */
int  crass_hip_group_inflate_gzip_members(crass_hip_group *g, const uint8_t *bytes, uint64_t n_bytes, uint64_t chunk_bytes, const uint64_t *nominal,
                                          uint8_t *out_host, uint64_t out_cap, uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members,
                                          crass_bgzf_verdict *v);
/* crass_hip_group_load_fastx_files takes a plain gzip file: mode 0 (the default) such a file is declined as before
 * (reason 10); CRASS_GZIP_ON_DEVICE_MEMBERS (2): plain gzip of any number of members — everything below in members mode
 * (crass_hip_group_inflate_gzip_members); members may end anywhere in the text, also inside a record: the cuts are by text; a
 * member's verdict (7 / 8 / 9 with the member and the file byte of its header) is the file's decline like 9 and 14 below; a
 * single-member file gives what mode 1 gives.  CRASS_GZIP_ON_DEVICE_ONE_MEMBER, or any other non-zero value, files of ONE member
 * (further members: 13): a file that starts with the gzip magic and that
 * crass_bgzf_index_host declines as not BGZF goes through an index step before the shards are cut (chunk_bytes: 0 the default
 * chunk, else clamped to 4096 .. 4 MB): every rank runs k_gz_find and k_gz_count on its share of the chunks, rank 0 walks the
 * chain.  The text's size and the element index (start bit, end bit and text offset of every chain element) are then known and
 * take a BGZF index's place, elements for members.  With the nominal cuts known every rank inflates the elements that hold its
 * pieces, in two halves: k_gz_decode and k_gz_windows_sym, then — the entry windows composed on the host in rank order —
 * k_gz_window_resolve and k_gz_narrow; the text stays on the rank's device, only compressed bytes cross the bus.  Elements a rank
 * needs later (the tail up to the next rank's cut, a wrapped-mode margin that doubles) are decoded and their windows walked by
 * k_gz_windows from the resolved window the rank keeps behind its last element (a seeded walk), through the one seam that inflates
 * BGZF members for the shard code.  Every element's CRC-32 part comes from the first rank that narrowed it, rank 0 joins them over
 * the chain.  A file that does not inflate — a chain decline (several members: 13), a wrong CRC-32 (9), an unresolved marker (14,
 * the smallest element over the ranks) — is the job's decline (bgzf: crass_gzip_inflate_host's verdict) unless a file in front
 * of it offends.  A rank keeps the compressed bytes it staged and fetches only what its elements still need, while the file is
 * the one it staged last: every file's index step runs before any file is inflated, so only the LAST gzip file of a job gains
 * from it (of a paired R1 / R2 job, R1's bytes go up twice).  Memory: a rank holds its text three times at the peak — what it
 * keeps of every gzip file until the load ends, the stage buffer, the arena — beside 2 bytes per text byte of symbols and 96 KB
 * per chain element of windows while a file is inflated.  exact: out equals crass_fastx_files_shards_host_gzip's with the same class,
 * mode and chunk.  (No reference counterpart.)  CRASS_ERR_INVALID_ARG: a NULL group, a negative mode. */
int  crass_hip_group_set_gzip_on_device(crass_hip_group *g, int mode, uint64_t chunk_bytes);
/* members mode, the last crass_hip_group_inflate_gzip_members that got to its end, or summed over the files the last
 * crass_hip_group_load_fastx_files took in members mode (else zeros): out[0] files taken in members mode, out[1] their members,
 * out[2] CRC pieces, summed over the ranks, out[3] exported windows that held no reference (a rank whose range holds a member
 * boundary exports such a window).  (No reference counterpart.) */
int  crass_hip_group_gzip_members_counters(const crass_hip_group *g, uint64_t out[4]);
/* members mode: HIP-event milliseconds on rank `rank`'s stream of k_gz_member_crc over its pieces, out[0], in the last
 * crass_hip_group_inflate_gzip_members (of a load: its last gzip file's); crass_hip_group_gzip_ms's narrow does not hold it.
 * Measured when that rank's stage timing level is >= 1, else 0.  (No reference counterpart.) */
int  crass_hip_group_gzip_members_ms(const crass_hip_group *g, int rank, float out[1]);
/* the last crass_hip_group_inflate_gzip that got as far as the decode step (else zeros), or summed over the gzip files the last
 * crass_hip_group_load_fastx_files took (a load that took none: zeros): out[0] gzip files taken, out[1] chunks,
 * out[2] chain elements, out[3] how many times an element was inflated by a further rank (the elements the ranks hold, summed,
 * minus out[2], plus in a load the elements its seeded walks added), out[4] compressed bytes uploaded, summed over the ranks, out[5] those of them that an upload had brought
 * already (to any rank).  (No reference counterpart.) */
int  crass_hip_group_gzip_counters(const crass_hip_group *g, uint64_t out[6]);
/* HIP-event milliseconds on rank `rank`'s stream of its kernels in the last crass_hip_group_inflate_gzip: out[0 .. 6) find, count,
 * decode, symbolic windows, resolve, narrow (of a load: its last gzip file's); out[6] the seeded window walks (k_gz_windows) of the
 * last files load, summed; measured when that rank's stage timing level is >= 1, else 0.  (No reference counterpart.) */
int  crass_hip_group_gzip_ms(const crass_hip_group *g, int rank, float out[7]);
/* replaces: ReadHolder's RH_Header / RH_Comment and RH_Qual / RH_IsFasta for a group loaded by crass_hip_group_load_fastx_files:
 * crass_hip_fetch_header_lines_device / crass_hip_fetch_quality_device on every rank's arena, over the whole job.  read_idx are
 * GLOBAL read indices (0 .. n_reads), routed to the rank that holds them; the records come back in the caller's order in one
 * crass_text owned by the group (each call its own), valid until the next call of the same function, group load or destroy.
 * name_len_out / has_qual_out (host [n], may be NULL) as in the single-context calls.  Errors: CRASS_ERR_STATE — the last group
 * load was not a files load (or was declined); CRASS_ERR_INVALID_ARG — NULL group or result, NULL read_idx with n > 0, an index
 * >= n_reads. */
int  crass_hip_group_fetch_header_lines(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint32_t *name_len_out);
int  crass_hip_group_fetch_quality(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint8_t *has_qual_out);
/* ---- the comment kseq hands on from record to record ----
 * replaces: ReadHolder's RH_Comment as searchFile / findSingletons fill it (libcrispr.cpp:124-127, :471-487).  kseq_read sets
 * comment.l = 0 for every record but never clears comment.s (kseq.cpp:182-186), and the callers test only comment.s: a record
 * whose header line has no comment of its own is handed the last comment seen earlier in the SAME file (the reference opens one
 * kseq per file), a record in front of its file's first comment is handed none.  The rule (csrc/fastx_scan.h states it once for
 * host and device): record r has an OWN comment iff its name — the bytes behind the header character up to the first isspace()
 * byte or the end of the text — ends at a byte that exists and is not '\n'; the own comment is the bytes behind that byte up to,
 * not including, the line's '\n' or the end of the text (it may be empty: ">a \n", ">a\r\n"; a '\r' in front of the '\n' stays).
 * The comment HANDED to r is the own comment of the last record r' <= r of r's file that has one.
 * the host rule, no GPU needed: the handed comments of the records idx[0..n) (idx[k] - idx_base in [0, n_reads), any order,
 * repeats allowed) back to back in out, off_out[n+1], has_out[n] (may be NULL): 1 where a comment is handed (it may be empty),
 * 0 where none is.  file_read_base[n_files+1] (file f holds records [file_read_base[f], file_read_base[f+1]); NULL: one file) as
 * in crass_fastx_files_layout, whose arena layout the bytes of several files have: a '\n' behind every file's text, so that no
 * name or comment runs into the next file (rec_pos has n_reads + 1 entries, the last is not read).
 * By the conventions of crass_fastx_names_of: CRASS_ERR_OVERFLOW — off_out[n] > cap_bytes: off_out and has_out complete, nothing
 * at or beyond out + cap_bytes written; CRASS_ERR_INVALID_ARG (nothing written) — NULL off_out, NULL idx with n > 0, NULL bytes or
 * rec_pos with n_reads > 0, NULL out with cap_bytes > 0, an index outside the records, a rec_pos at or beyond n_bytes, a
 * file_read_base that does not run from 0 to n_reads without decreasing.  n == 0: CRASS_OK. */
int  crass_fastx_comments_of(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads, const uint64_t *file_read_base,
                             uint32_t n_files, const uint64_t *idx, uint64_t n, uint64_t idx_base, uint8_t *out, uint64_t cap_bytes,
                             uint64_t *off_out, uint8_t *has_out);
/* the device side, for bytes that exist only in HBM (fastx_lines.hip).  BUILD: k_cm_bits — a lane per record walks its name, a
 * wave's ballot is one 64-bit word of the own-comment BITMAP; k_cm_tiles / k_cm_top — every tile of 4 096 records gets a carry
 * word, the last own-comment record in all tiles up to and including it (a maximum scan in launches of their own: no block
 * waits for another).  Kept in the context: one bit per record, 8 bytes per tile and file_read_base; the record positions are
 * scratch of the build.  d_bytes == NULL and rec_pos == NULL: on the arena and the layout of the last
 * crass_hip_load_fastx_files (the other arguments are ignored); else d_bytes is the caller's DEVICE memory, which must stay
 * valid and unchanged until the drop, and rec_pos (HOST, n_reads + 1 entries) is copied into the context's host memory.
 * Any load, attach or destroy drops a structure built on the arena.  Errors: CRASS_ERR_STATE — no arena; CRASS_ERR_INVALID_ARG —
 * as the host rule; CRASS_ERR_UNSUPPORTED — n_reads >= 2^32 - 1; a failed build leaves the context as it was. */
int  crass_hip_fastx_comments_build_device(crass_hip_ctx *ctx, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                           const uint64_t *file_read_base, uint32_t n_files);
int  crass_hip_fastx_comments_drop(crass_hip_ctx *ctx);
/* FETCH: the handed comments of the records idx[0..n) (HOST array, LOCAL record numbers, any order, repeats allowed) — k_cm_source:
 * a lane per listed record bisects file_read_base, finds its source in the bitmap (its own word, the earlier words of its tile,
 * the carry of the tile in front) and drops a source in front of its file's first record; k_cm_measure walks the source's name
 * and comment; k_span_copy, a lane per OUTPUT byte, copies.  The result is a crass_text in the context's pinned memory (its own),
 * valid until the next call of this function or destroy; has_out (host [n], may be NULL) as in the host rule.  Without a built
 * structure the first fetch after crass_hip_load_fastx_files builds it on the arena; else CRASS_ERR_STATE.  Exact:
 * crass_fastx_comments_of on the same bytes.  CRASS_ERR_INVALID_ARG — NULL context or result, NULL idx with n > 0, an idx[k] >= n_reads. */
int  crass_hip_fetch_comments_device(crass_hip_ctx *ctx, const uint64_t *idx, uint64_t n, crass_text *out, uint8_t *has_out);
/* the same into the caller's DEVICE buffer by the rules of crass_hip_fetch_header_lines_device_to: cap_bytes < off_out[n] is
 * CRASS_ERR_OVERFLOW with off_out and has_out filled and nothing written; no byte outside [d_chars, d_chars + off_out[n]) is
 * written; d_chars may be NULL with cap_bytes 0.  Without a built structure and without an arena: CRASS_ERR_STATE. */
int  crass_hip_fetch_comments_device_to(crass_hip_ctx *ctx, const uint64_t *idx, uint64_t n, uint8_t *d_chars, uint64_t cap_bytes,
                                        uint64_t *off_out, uint8_t *has_out);
/* out[0]: the records of the built structure that have a comment of their own, out[1]: its records.  CRASS_ERR_STATE without one. */
int  crass_hip_fastx_comments_counters(const crass_hip_ctx *ctx, uint64_t out[2]);
/* HIP-event times, in milliseconds on the context's stream: part 0 the three launches of the last build, part 1 the kernels of
 * the last fetch with the copies between them; measured when the stage timing level is >= 1, else 0. */
float crass_hip_last_comments_ms(const crass_hip_ctx *ctx, int part);
/* the same for a group loaded by crass_hip_group_load_fastx_files, routed and owned like crass_hip_group_fetch_header_lines.  A
 * rank's shard may begin in the middle of a file: every rank publishes the own comment of the last own-comment record of the
 * file part its shard ends in (a host string), the group resolves what is carried into every rank's first file part (empty
 * ranks and ranks whose part holds no comment pass it through), and a listed record with no source in its rank's part of its
 * file is handed that string.  Exact: crass_fastx_comments_of on the whole job. */
int  crass_hip_group_fetch_comments(crass_hip_group *g, const uint64_t *read_idx, uint64_t n, crass_text *out, uint8_t *has_out);
/* the route of the found-name exchange of a files load (names that repeat across ranks, above).  0, the default: through the host —
 * header lines back, cut at the name, every other rank's names up (crass_hip_fastx_names_find), the namesakes up again.
 * on_device != 0 (or CRASS_GROUP_NAMES=device in the environment when the group is created): rank r writes its names with
 * crass_hip_found_names_device into a device buffer of its own (sized from the step before; regrown once to the reported totals
 * on CRASS_ERR_OVERFLOW), copies every other rank's names and offsets to its device on its stream (hipMemcpyPeerAsync; with
 * CRASS_GROUP_LOCAL_COPIES a device-to-device copy), looks them up with crass_hip_fastx_names_find_device into one answer array
 * and hands that to crass_hip_recruit_found.  No name, answer or index crosses to the host, only counts and totals; a failed
 * copy is CRASS_ERR_HIP of the step, never a change of route.  Both routes give the same results.  CRASS_ERR_INVALID_ARG: a NULL
 * group. */
int  crass_hip_group_set_name_exchange(crass_hip_group *g, int on_device);
/* out: [0] the route of the last step's exchange on that rank (0 host, 1 device), [1] the names it published, [2] the queries
 * it looked up (the other ranks' names), [3] the namesakes it found; zeros before the first exchange.  CRASS_ERR_INVALID_ARG: a
 * NULL group or out, a rank outside the group. */
int  crass_hip_group_name_exchange_counters(const crass_hip_group *g, int rank, uint64_t out[4]);
/* what the last step's exchange took on that rank, from the publish to the end of the lookup, the barrier between them
 * included: out[0] wall milliseconds; out[1] HIP-event milliseconds on the rank's stream between the same two points, measured
 * only in a group created with CRASS_GROUP_NAMES_TIMING in the environment, else 0.  (No reference counterpart: crass has no
 * timers.)  CRASS_ERR_INVALID_ARG as above. */
int  crass_hip_group_name_exchange_ms(const crass_hip_group *g, int rank, float out[2]);
/* the two decisions of the packers on their own, for callers and tests without a GPU: the layout crass_pack_reads and
 * crass_hip_load_text give a set (stride_words / uniform_len as in crass_reads), and the byte -> code function both use —
 * four sequence bytes (byte 0 first) -> their 2-bit codes in bits [2i, 2i+2), *bad bit i set when byte i is not A C G T
 * (its code is then 0). */
int  crass_pack_layout(const uint64_t *off, uint64_t n_reads, int pad_uniform, uint32_t *stride_words, uint32_t *uniform_len);
uint32_t crass_pack_code4(uint32_t four_bytes, uint32_t *bad);

/* FASTA/FASTQ(.gz) reader with kseq_read record semantics (kseq.cpp:171-226).  Buffers are
 * malloc'd, free with crass_free_fastx.                                                    */
typedef struct {
    uint64_t  n_reads;
    uint8_t  *seq;   uint64_t *seq_off;     /* [n+1] */
    uint8_t  *name;  uint64_t *name_off;
    uint8_t  *comment; uint64_t *comment_off; uint8_t *has_comment; /* stale-pointer semantics,
                                                                       libcrispr.cpp:124-127 */
    uint8_t  *qual;  uint64_t *qual_off;   uint8_t *has_qual;
    uint64_t *header_id;                    /* first read with the same name                     */
    uint32_t  max_len;
    int32_t   last_ret;                     /* kseq_read's final return value (-1 EOF, -2 trunc) */
    uint64_t *name_index; uint64_t name_index_cap;   /* open-addressing table name -> first read (crass_fastx_find) */
} crass_fastx;
int  crass_read_fastx(const char *path, crass_fastx *out);
void crass_free_fastx(crass_fastx *f);
/* index of the FIRST read with this header name (the key of readsFound, libcrispr.cpp:138,411), UINT64_MAX if none */
uint64_t crass_fastx_find(const crass_fastx *f, const char *name, uint64_t len);

/* The same reader as an INDEX over an input kept mapped (plain text) or inflated once (gzip, through libdeflate when the runtime
 * library is there): the records are parsed by the same state machine, every read is
 * 2-bit packed at once (crass_pack_reads' layout rules, mode 2) and its text dropped; what stays is the packed reads, the
 * position of every record's header character, and header_id (first read with the same header, names compared in the mapping:
 * exact).  crass_fastx_index_fetch parses the records that are handed on (the ~1 % that pass 1 / pass 2 find) when they are
 * asked for.  replaces: the getFileHandle / kseq_read loops of searchFile + findSingletons (libcrispr.cpp:84-131, 471-487) and
 * the ReadHolder fields they fill (seq, header, comment, quality) for the reads that reach addReadHolder.  Host memory: 40 bytes
 * of words + 12 of bookkeeping per 150 bp read instead of ~330.  CRASS_ERR_UNSUPPORTED: a gzip'd input without libdeflate or whose text would not fit half the available memory, a file that mixes
 * records with and without a comment / quality line (kseq's stale buffers, libcrispr.cpp:124-131, need the records in order), a
 * file that cannot be mapped — the two readers around this one take those.                                                      */
typedef struct crass_fastx_index crass_fastx_index;
int  crass_index_fastx(const char *path, crass_fastx_index **out);
/* ... over SEVERAL inputs (paired-end files, lanes): the job's reads in (file, read) order in one packed set, header ids across the
 * inputs (the first read of the JOB with the same header: readsFound is keyed by the header string whatever file it came from,
 * libcrispr.cpp:138,411), every input plain text or gzip'd on its own.  max_len / last_ret of crass_fastx_index_reads: the longest
 * read of all inputs, kseq_read's final return value on the LAST one.                                                              */
int  crass_index_fastx_files(const char *const *paths, uint32_t n_paths, crass_fastx_index **out);
/* the packed reads (host pointers owned by the index), the longest read, kseq_read's final return value */
int  crass_fastx_index_reads(const crass_fastx_index *ix, crass_reads *reads, uint32_t *max_len, int *last_ret);
/* records idx[0 .. n) (any order) as a crass_fastx of n records in that order; header_id[k] = idx[k]; free with crass_free_fastx */
int  crass_fastx_index_fetch(const crass_fastx_index *ix, const uint64_t *idx, uint64_t n, crass_fastx *out);
void crass_fastx_index_free(crass_fastx_index *ix);
/* the mappings of the plain-text inputs given back now, over the cores (page tables of gigabytes are slow to take down and block the
 * process's other allocations meanwhile); records fetched afterwards are read from the files — a hand-off fetches what it needs first */
void crass_fastx_index_drop_text(crass_fastx_index *ix);

/* The same reader as a STREAM of chunks, for inputs that should not be held in host memory as a whole — the reference's own
 * memory model: kseq_read hands out one record at a time (kseq.cpp:171-226, libcrispr.cpp:96) and crass reads every input
 * twice, once per pass (WorkHorse.cpp:336-393).  A chunk holds the complete records of about `chunk_bytes` of decompressed text
 * (0: 64 MB; a record larger than a chunk grows it); the fields are those of crass_fastx, valid until the next call; n_reads == 0
 * marks the end of the file.  kseq's cross-record state travels with the stream (stale comment / quality buffers,
 * libcrispr.cpp:124-131).  With a name table, header_id[i] is the JOB-level index (index_base + records before it in this
 * stream) of the first read with the same header — across chunks and, with one table for several streams, across files
 * (readsFound is keyed by the header string, libcrispr.cpp:138,411); names are kept as 128-bit hashes only (two independent
 * 64-bit mixes, both stored and compared in full): two DIFFERENT headers of a job of n reads are taken for one with probability
 * ~ n^2 / 2^129 (1.5e-23 at n = 1e8) — the one place of the path that is exact with that probability rather than by
 * construction; crass_read_fastx (whole-file) compares the header strings themselves.                                       */
typedef struct crass_name_table crass_name_table;
typedef struct crass_fastx_stream crass_fastx_stream;
crass_name_table *crass_name_table_create(void);
void     crass_name_table_destroy(crass_name_table *t);
void     crass_name_table_reserve(crass_name_table *t, uint64_t n_names);    /* sized once for about n_names names (optional) */
uint64_t crass_name_table_first(crass_name_table *t, const char *name, uint64_t len, uint64_t index);
int      crass_fastx_stream_open(const char *path, uint64_t chunk_bytes, crass_name_table *names, uint64_t index_base,
                                 crass_fastx_stream **out);
int      crass_fastx_stream_next(crass_fastx_stream *s, crass_fastx *chunk);
uint64_t crass_fastx_stream_reads_done(const crass_fastx_stream *s);
uint32_t crass_fastx_stream_max_len(const crass_fastx_stream *s);
void     crass_fastx_stream_close(crass_fastx_stream *s);

/* deterministic synthetic metagenome: counter-based, so any shard can be
 * generated independently.  Writes 2-bit packed reads with uniform stride ceil(L/16).      */
typedef struct {
    uint64_t seed;
    uint32_t read_len;          /* 150                                                        */
    uint32_t n_dr;              /* 50 (config 2/3), 500 (config 5)                            */
    uint32_t dr_len_min, dr_len_max;       /* 28..37                                          */
    uint32_t spacer_len_min, spacer_len_max; /* 30..38                                        */
    uint32_t crispr_per_million; /* 10000 = 1 %                                               */
    uint32_t gc_classes;        /* 0/1 = uniform; 4 = GC 30/45/55/70 % background mix         */
    uint32_t array_min_repeats, array_max_repeats; /* 0,0 = short-read mode (the read is a cut
                                   from a tiled DR+spacer stream); else long-read mode (config 4:
                                   20..60): an array of that many units written into a random read */
} crass_synth_spec;
void crass_synth_default(crass_synth_spec *s);
int  crass_synth_packed(const crass_synth_spec *s, uint64_t first_read, uint64_t n_reads,
                        uint32_t *packed_out /* n_reads*ceil(L/16) words */, int n_threads);
/* unpack reads [first, first+n) of a uniform-stride packed buffer to ASCII (for the CPU baseline) */
int  crass_unpack_ascii(const uint32_t *packed, uint32_t stride_words, uint32_t read_len,
                        uint64_t n_reads, uint8_t *ascii_out /* n_reads*read_len */);

int crass_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CRASS_HIP_H */

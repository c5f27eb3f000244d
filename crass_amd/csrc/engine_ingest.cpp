// engine_ingest.cpp — the device ingest behind include/crass_hip.h: packed reads and sequence text in (pack.hip), the raw
// bytes of FASTA / FASTQ files parsed on the device (fastx_scan.hip), BGZF and plain gzip inflated there (inflate.hip,
// gunzip.hip), several files as one set, header ids, the name table, header lines and quality strings (fastx_names.hip), and
// the text of resident reads back out (k_fetch_text), and one rank's steps of a group's files load (fastx_shards.h: stage and
// probe, complete and scan, pack).  The context and its Ingest member are engine_ctx.h; what a load ends
// with (finish_load: scratch, position hints, first-call bounds) is engine.cpp's.
#include "engine_ctx.h"
#include "pack_launch.h"
#include "fastx_names_launch.h"
#include "inflate_launch.h"
#include "gunzip_launch.h"
#include "fastx_shards.h"

#include <new>

extern "C" {

// the file arena of crass_hip_load_fastx_files goes with the read set it belongs to: every public load and attach calls this
// (load_text_impl, the pack step those calls share with crass_hip_load_fastx_files itself, does not)
static void names_drop(crass_hip_ctx *c)
{
    if (c->in.nt_table.p || c->in.nt_rec_pos.p) { (void)hipStreamSynchronize(c->stream); c->in.nt_table.release(); c->in.nt_rec_pos.release(); }
    c->in.have_names = false; c->in.nt_on_arena = false; c->in.nt_bytes = nullptr; c->in.nt_n_bytes = c->in.nt_n_reads = c->in.nt_mask = 0;
}

static void drop_arena(crass_hip_ctx *c)
{
    if (c->in.have_names && c->in.nt_on_arena) names_drop(c);      // (a name table built on the arena refers to its bytes)
    if (c->in.fa_arena.p) { (void)hipStreamSynchronize(c->stream); c->in.fa_arena.release(); }
    c->in.have_arena = false; c->in.fa_bytes = 0; c->in.sh_loaded = false;
}

// ---- the scratch goes back: one function per stage, which first waits for the streams that may still use the stage's buffers ----
static void wait_main(crass_hip_ctx *c) { (void)hipStreamSynchronize(c->stream); }
static void wait_both(crass_hip_ctx *c) { wait_main(c); (void)hipStreamSynchronize(c->copy_stream); }
// crass_hip_load_text's own part: the text's offsets (8 bytes per read) and the two staged chunks, upload_staged's too (pinned and
// device memory of up to CRASS_TEXT_CHUNK_BYTES each) — a context loads a read set once
static void release_text(crass_hip_ctx *c)
{
    wait_both(c);
    c->in.t_off.release();
    for (int k = 0; k < 2; k++) { c->in.t_dev[k].release(); c->in.t_pin[k].release(); }
}

// the scan: the raw copy, the reads' text, the tile and per-record arrays
static void release_scan(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_both(c);
    I.x_raw.release(); I.x_text.release(); I.x_tiles.release(); I.x_base.release(); I.x_tot.release(); I.x_rec_pos.release(); I.x_seq_off.release();
}

// the BGZF inflate, and the verdict word the gzip decode step shares with it
static void release_bgzf(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_both(c);
    I.z_idx.release(); I.z_reason.release(); I.z_verdict.release(); I.z_raw.release(); I.z_text.release();
}

static void release_gzip(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.gz_a64.release(); I.gz_b64.release(); I.gz_a32.release(); I.gz_b32.release(); I.gz_sym.release(); I.gz_win.release(); I.gz_ends.release();
}

// the header ids, and what a names build needs beside the table it keeps
static void release_header_ids(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.n_table.release(); I.n_rec_pos.release(); I.n_ids.release(); I.n_long.release(); I.n_ctl.release();
}

static void release_names_find(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.nq_names.release(); I.nq_off.release(); I.nq_out.release(); I.nq_long.release(); I.nq_ctl.release();
}

static void release_names_of(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.no_len.release(); I.no_flag.release(); I.no_tiles.release(); I.no_idx.release(); I.no_off.release();
}

static void release_lines(crass_hip_ctx *c, LineFetch &B) { wait_main(c); B.release_device(); }

// a shard's staged text, its BGZF tail and the probe's parts (fastx_shards.h)
static void release_shard(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_both(c);
    I.sh_stage.release(); I.sh_tail.release(); I.sh_part.release();
    I.sh_staged.clear(); I.sh_scanned = false;
}

void ingest_free_all(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    release_text(c); release_scan(c); release_bgzf(c); release_gzip(c); release_header_ids(c); release_names_find(c); release_names_of(c);
    names_drop(c); drop_arena(c);
    release_shard(c); I.sh_h_part.release(); I.tm_probe.destroy();
    I.hl.free_all(); I.ql.free_all();
    // what is kept from call to call, and the pinned sides of the results
    I.f_idx.release(); I.f_off.release(); I.f_rc.release(); I.f_chars.release();
    I.f_h_idx.release(); I.f_h_off.release(); I.f_h_rc.release(); I.f_h_chars.release();
    I.x_h_tot.release(); I.x_h_rec_pos.release(); I.x_h_seq_off.release(); I.z_h_verdict.release(); I.n_h_ctl.release(); I.nq_h_ctl.release(); I.no_h.release();
    I.fa_h_base.release(); I.fa_h_format.release();
    for (hipEvent_t *e : {&I.ev_t_copy[0], &I.ev_t_copy[1], &I.ev_t_pack[0], &I.ev_t_pack[1]}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    I.tm_pack.destroy(); I.tm_scan.destroy(); I.tm_inflate.destroy(); I.tm_gzip.destroy(); I.tm_fetch.destroy(); I.tm_names.destroy(); I.tm_find.destroy();
}

// what opens every call that replaces the resident set: earlier results and the arena go, and a failure or a decline further
// down leaves no reads, never the previous ones half replaced
static void begin_load(crass_hip_ctx *c)
{
    (void)hipSetDevice(c->device);
    reset_results(c);
    c->have_reads = false;
    drop_arena(c);
}

// ... and the FASTA / FASTQ loaders' stage times start from zero (a compressed file's loader clears last_inflate_ms too)
static void begin_fastx_load(crass_hip_ctx *c)
{
    begin_load(c);
    c->in.last_scan_ms = 0; c->in.last_pack_ms = 0;
}

int crass_hip_load_reads(crass_hip_ctx *c, const crass_reads *h)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    int v = validate_reads(h);
    if (v) return v;
    begin_load(c);
    const uint64_t n = h->n_reads;
    // host-side scan for the total word count / max length
    uint64_t total_words = 0;
    uint32_t max_len = h->uniform_len;
    if (!h->uniform_len) for (uint64_t i = 0; i < n; i++) max_len = std::max(max_len, h->lengths[i]);
    if (max_len > CRASS_HIP_MAX_READ_LEN) return CRASS_ERR_UNSUPPORTED;
    if (h->stride_words) total_words = n * (uint64_t)h->stride_words;
    else if (n) {
        uint32_t lastL = h->uniform_len ? h->uniform_len : h->lengths[n - 1];
        total_words = h->word_off[n - 1] + (lastL + 15) / 16;
    }
    HIPCHK(c, c->r_packed.ensure(total_words + 4));
    HIPCHK(c, hipMemcpyAsync(c->r_packed.p, h->packed, total_words * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->r_packed.p + total_words, 0, 16, c->stream));
    DevReads R{};
    R.packed = c->r_packed.p; R.n_reads = n; R.stride_words = h->stride_words; R.uniform_len = h->uniform_len;
    if (!h->stride_words) {
        HIPCHK(c, c->r_word_off.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->r_word_off.p, h->word_off, n * 8, hipMemcpyHostToDevice, c->stream));
        R.word_off = c->r_word_off.p;
    }
    if (!h->uniform_len) {
        HIPCHK(c, c->r_lengths.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->r_lengths.p, h->lengths, n * 4, hipMemcpyHostToDevice, c->stream));
        R.lengths = c->r_lengths.p;
        c->h_lengths.assign(h->lengths, h->lengths + n);
    } else c->h_lengths.clear();
    if (h->header_id) {
        HIPCHK(c, c->r_header_id.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->r_header_id.p, h->header_id, n * 8, hipMemcpyHostToDevice, c->stream));
        R.header_id = c->r_header_id.p;
    }
    const uint64_t mask_words = (n + 31) / 32 + 1;
    HIPCHK(c, c->r_exc_mask.ensure(mask_words));
    HIPCHK(c, hipMemsetAsync(c->r_exc_mask.p, 0, mask_words * 4, c->stream));
    R.exc_mask = c->r_exc_mask.p;
    R.n_exc = h->n_exceptions;
    c->h_exc_read.assign(h->exc_read, h->exc_read + h->n_exceptions);
    if (h->n_exceptions) {
        const uint64_t ne = h->n_exceptions;
        for (uint64_t i = 0; i < ne; i++) {
            uint64_t l = h->exc_off[i + 1] - h->exc_off[i];
            if (l > CRASS_HIP_MAX_READ_LEN) return CRASS_ERR_UNSUPPORTED;
            max_len = std::max<uint32_t>(max_len, (uint32_t)l);
        }
        HIPCHK(c, c->r_exc_read.ensure(ne));
        HIPCHK(c, c->r_exc_off.ensure(ne + 1));
        HIPCHK(c, c->r_exc_bytes.ensure(h->exc_off[ne] + 16));
        HIPCHK(c, hipMemcpyAsync(c->r_exc_read.p, h->exc_read, ne * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->r_exc_off.p, h->exc_off, (ne + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->r_exc_bytes.p, h->exc_bytes, h->exc_off[ne], hipMemcpyHostToDevice, c->stream));
        R.exc_read = c->r_exc_read.p; R.exc_off = c->r_exc_off.p; R.exc_bytes = c->r_exc_bytes.p;
        HIPCHK(c, launch_build_exc_mask(R.exc_read, ne, c->r_exc_mask.p, c->stream));
    }
    return finish_load(c, R, h->read_index_base, max_len, h->uniform_len ? nullptr : h->lengths, total_words);
}

int crass_hip_attach_device_reads(crass_hip_ctx *c, const crass_reads *d)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    int v = validate_reads(d);
    if (v) return v;
    if (!d->uniform_len || !d->stride_words) return CRASS_ERR_UNSUPPORTED;   // attach mode: uniform shards only
    if (d->n_exceptions) return CRASS_ERR_UNSUPPORTED;
    begin_load(c);
    DevReads R{};
    R.packed = d->packed; R.n_reads = d->n_reads; R.stride_words = d->stride_words; R.uniform_len = d->uniform_len;
    R.header_id = d->header_id;
    const uint64_t mask_words = (d->n_reads + 31) / 32 + 1;
    HIPCHK(c, c->r_exc_mask.ensure(mask_words));
    HIPCHK(c, hipMemsetAsync(c->r_exc_mask.p, 0, mask_words * 4, c->stream));
    R.exc_mask = c->r_exc_mask.p;
    c->h_exc_read.clear();
    c->h_lengths.clear();
    return finish_load(c, R, d->read_index_base, d->uniform_len, nullptr, d->n_reads * (uint64_t)d->stride_words);
}

// ---- sequence text in, packed on the device (pack.hip) ----
// h_seqs (host text) or d_seqs (device text); off[n + 1] is a host array either way.  The resident set, the host mirrors and
// the counters end up as after crass_pack_reads + crass_hip_load_reads on the same bytes.
static int load_text_impl(crass_hip_ctx *c, const uint8_t *h_seqs, const uint8_t *d_seqs, const uint64_t *off, uint64_t n,
                            int pad_uniform, const uint64_t *header_id, uint64_t read_index_base)
{
    if (!c || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    if (n && ((!h_seqs && !d_seqs) || !off)) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    reset_results(c);
    c->have_reads = false;                              // (a failure below must not leave the previous reads half replaced)
    PackLayout lay;
    if (const int ls = pack_layout(off, n, pad_uniform, &lay)) return ls;      // (nothing launched)
    const uint64_t total_words = lay.total_words, out_words = (total_words + 4 + 3) & ~3ull;      // (the last vector store ends inside the buffer)
    HIPCHK(c, c->r_packed.ensure(out_words));
    DevReads R{};
    R.packed = c->r_packed.p; R.n_reads = n; R.stride_words = lay.stride_words; R.uniform_len = lay.uniform_len;
    std::vector<uint64_t> word_off;
    std::vector<uint32_t> lengths;
    if (!lay.stride_words && n) {
        word_off.resize(n + 1);
        uint64_t w = 0;
        for (uint64_t i = 0; i < n; i++) { word_off[i] = w; w += (off[i + 1] - off[i] + 15) / 16; }
        word_off[n] = w;
        HIPCHK(c, c->r_word_off.ensure(n + 1));
        HIPCHK(c, hipMemcpyAsync(c->r_word_off.p, word_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        R.word_off = c->r_word_off.p;
    }
    if (!lay.uniform_len && n) {
        lengths.resize(n);
        for (uint64_t i = 0; i < n; i++) lengths[i] = (uint32_t)(off[i + 1] - off[i]);
        HIPCHK(c, c->r_lengths.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->r_lengths.p, lengths.data(), n * 4, hipMemcpyHostToDevice, c->stream));
        R.lengths = c->r_lengths.p;
        HIPCHK(c, c->in.t_off.ensure(n + 1));              // (a uniform length needs no per-read array: off[i] = off[0] + i L)
        HIPCHK(c, hipMemcpyAsync(c->in.t_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (header_id && n) {
        HIPCHK(c, c->r_header_id.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->r_header_id.p, header_id, n * 8, hipMemcpyHostToDevice, c->stream));
        R.header_id = c->r_header_id.p;
    }
    const uint64_t mask_words = (n + 31) / 32 + 1;
    HIPCHK(c, c->r_exc_mask.ensure(mask_words));
    HIPCHK(c, hipMemsetAsync(c->r_exc_mask.p, 0, mask_words * 4, c->stream));
    R.exc_mask = c->r_exc_mask.p;
    c->h_exc_read.clear();

    PackJob J{};
    J.off = lay.uniform_len ? nullptr : c->in.t_off.p;
    J.uni_base = n ? off[0] : 0; J.uni_len = lay.uniform_len;
    J.stride_words = lay.stride_words; J.word_off = R.word_off;
    J.out = c->r_packed.p; J.exc_mask = c->r_exc_mask.p;
    auto word_start = [&](uint64_t r) { return lay.stride_words ? r * (uint64_t)lay.stride_words : word_off[r]; };
    // stage timing (crass_hip_set_stage_timing >= 1): the pack kernels between two events, crass_hip_last_pack_ms
    c->in.last_pack_ms = 0;
    HIPCHK(c, c->in.tm_pack.begin(c->timing_level >= 1 && n != 0, c->stream));
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(c->r_packed.p, 0, out_words * 4, c->stream));
    } else if (d_seqs) {
        J.text = d_seqs; J.bias = 0; J.r_begin = 0; J.r_end = n; J.w_begin = 0; J.w_end = out_words;
        HIPCHK(c, launch_pack_text(J, c->stream));
    } else {
        // chunks of whole reads through two staged buffers: the copy of chunk k + 1 (copy stream) runs beside the pack kernel of
        // chunk k (main stream).  Pageable text goes through the pinned buffers; text that is already pinned is copied from where it is.
        const uint64_t text_bytes = off[n] - off[0];
        const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(c->env.text_chunk_bytes, lay.max_len), std::max<uint64_t>(text_bytes, 1));
        hipPointerAttribute_t pa{};
        const bool src_pinned = hipPointerGetAttributes(&pa, h_seqs) == hipSuccess && pa.type == hipMemoryTypeHost;
        (void)hipGetLastError();                        // (pageable memory is reported as an invalid value: not an error of ours)
        for (int k = 0; k < 2; k++) {
            if (!c->in.ev_t_copy[k]) HIPCHK(c, hipEventCreateWithFlags(&c->in.ev_t_copy[k], hipEventDisableTiming));
            if (!c->in.ev_t_pack[k]) HIPCHK(c, hipEventCreateWithFlags(&c->in.ev_t_pack[k], hipEventDisableTiming));
        }
        uint64_t ra = 0;
        for (uint64_t k = 0; ra < n; k++) {
            const int b = (int)(k & 1);
            uint64_t rb;                                // the chunk: reads [ra, rb), at least one
            if (lay.uniform_len) rb = std::min<uint64_t>(n, ra + std::max<uint64_t>(1, cap / lay.uniform_len));
            else rb = std::max<uint64_t>(ra + 1, (uint64_t)(std::upper_bound(off + ra, off + n + 1, off[ra] + cap) - off) - 1);
            const uint64_t bytes = off[rb] - off[ra];
            const bool last = rb == n;
            if (bytes) {
                HIPCHK(c, c->in.t_dev[b].ensure(cap + 16));
                const uint8_t *from = h_seqs + off[ra];
                if (!src_pinned) {
                    HIPCHK(c, c->in.t_pin[b].ensure(cap));
                    if (k >= 2) HIPCHK(c, hipEventSynchronize(c->in.ev_t_copy[b]));      // (the copy that last read this pinned buffer)
                    memcpy(c->in.t_pin[b].p, from, bytes);
                    from = c->in.t_pin[b].p;
                }
                if (k >= 2) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->in.ev_t_pack[b], 0));      // (the kernel that last read this device buffer)
                HIPCHK(c, hipMemcpyAsync(c->in.t_dev[b].p, from, bytes, hipMemcpyHostToDevice, c->copy_stream));
                HIPCHK(c, hipEventRecord(c->in.ev_t_copy[b], c->copy_stream));
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->in.ev_t_copy[b], 0));
            }
            J.text = c->in.t_dev[b].p; J.bias = off[ra]; J.r_begin = ra; J.r_end = rb;
            J.w_begin = word_start(ra); J.w_end = last ? out_words : word_start(rb);
            HIPCHK(c, launch_pack_text(J, c->stream));
            if (bytes) HIPCHK(c, hipEventRecord(c->in.ev_t_pack[b], c->stream));
            ra = rb;
        }
    }
    HIPCHK(c, c->in.tm_pack.mark(c->stream));
    // the exception list: ascending read indices from the mask (ordered look-back compaction), their bytes from the text
    c->R = R;
    if (n) {
        int s = alloc_scratch(c);
        if (s) return s;
        const uint64_t n_words = (n + 63) / 64;
        Lookback lbs;
        const Lookback *lb = c->next_lookback(n_words, &lbs);
        HIPCHK(c, launch_compact(reinterpret_cast<const uint64_t *>(c->r_exc_mask.p), n_words, n, c->d_word_prefix.p, c->d_block_sums.p, c->d_idx.p, n,
                                 c->d_count.p, c->stream, nullptr, 0, nullptr, 0, lb));
        HIPCHK(c, hipMemcpyAsync(c->h_count.p, c->d_count.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((s = c->lookback_ok())) return s;
        const uint64_t ne = c->h_count.p[0];
        if (ne) {
            c->h_exc_read.resize(ne);
            HIPCHK(c, c->r_exc_read.ensure(ne));
            HIPCHK(c, hipMemcpyAsync(c->r_exc_read.p, c->d_idx.p, ne * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpy(c->h_exc_read.data(), c->d_idx.p, ne * 8, hipMemcpyDeviceToHost));
            std::vector<uint64_t> exc_off(ne + 1);
            exc_off[0] = 0;
            for (uint64_t e = 0; e < ne; e++) { const uint64_t r = c->h_exc_read[e]; exc_off[e + 1] = exc_off[e] + (off[r + 1] - off[r]); }
            HIPCHK(c, c->r_exc_off.ensure(ne + 1));
            HIPCHK(c, c->r_exc_bytes.ensure(exc_off[ne] + 16));
            HIPCHK(c, hipMemcpyAsync(c->r_exc_off.p, exc_off.data(), (ne + 1) * 8, hipMemcpyHostToDevice, c->stream));
            if (d_seqs) {
                HIPCHK(c, launch_gather_exc_text(d_seqs, 0, J.off, J.uni_base, J.uni_len, c->r_exc_read.p, c->r_exc_off.p, ne, c->r_exc_bytes.p, c->stream));
            } else {
                std::vector<uint8_t> bytes(exc_off[ne] + 1);
                for (uint64_t e = 0; e < ne; e++) { const uint64_t r = c->h_exc_read[e]; memcpy(bytes.data() + exc_off[e], h_seqs + off[r], off[r + 1] - off[r]); }
                HIPCHK(c, hipMemcpyAsync(c->r_exc_bytes.p, bytes.data(), exc_off[ne], hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));      // (bytes goes out of scope)
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));          // (exc_off goes out of scope; the caller's text may be freed on return)
            R.exc_read = c->r_exc_read.p; R.exc_off = c->r_exc_off.p; R.exc_bytes = c->r_exc_bytes.p; R.n_exc = ne;
        }
    }
    const int s = finish_load(c, R, read_index_base, lay.max_len, lay.uniform_len ? nullptr : lengths.data(), total_words);
    c->h_lengths.swap(lengths);                         // (empty for a uniform length)
    if (!s) HIPCHK(c, c->in.tm_pack.elapsed(0, 1, &c->in.last_pack_ms));
    return s;
}

static int load_text_common(crass_hip_ctx *c, const uint8_t *h_seqs, const uint8_t *d_seqs, const uint64_t *off, uint64_t n,
                            int pad_uniform, const uint64_t *header_id, uint64_t read_index_base)
{
    // (with arguments load_text_impl refuses, the resident set and its arena stay)
    if (c && pad_uniform >= 0 && pad_uniform <= 2 && !(n && ((!h_seqs && !d_seqs) || !off))) { (void)hipSetDevice(c->device); drop_arena(c); }
    const int s = load_text_impl(c, h_seqs, d_seqs, off, n, pad_uniform, header_id, read_index_base);
    if (c) release_text(c);                             // what only this call needed goes back, on every way out
    return s;
}

int crass_hip_load_text(crass_hip_ctx *c, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, int pad_uniform,
                        const uint64_t *header_id, uint64_t read_index_base)
{
    return load_text_common(c, seqs, nullptr, off, n_reads, pad_uniform, header_id, read_index_base);
}

int crass_hip_attach_device_text(crass_hip_ctx *c, const uint8_t *d_seqs, const uint64_t *off, uint64_t n_reads, int pad_uniform,
                                 const uint64_t *header_id, uint64_t read_index_base)
{
    return load_text_common(c, nullptr, d_seqs, off, n_reads, pad_uniform, header_id, read_index_base);
}

float crass_hip_last_pack_ms(const crass_hip_ctx *c) { return c ? c->in.last_pack_ms : 0.0f; }

// n host bytes up into dst (device) through the two pinned staging buffers of crass_hip_load_text; bytes that are already pinned are
// copied from where they are.  The context's stream waits for the last copy.
static int upload_staged(crass_hip_ctx *c, const uint8_t *h_bytes, uint64_t n, uint8_t *dst)
{
    if (n == 0) return CRASS_OK;
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(c->env.text_chunk_bytes, 1), n);
    hipPointerAttribute_t pa{};
    const bool src_pinned = hipPointerGetAttributes(&pa, h_bytes) == hipSuccess && pa.type == hipMemoryTypeHost;
    (void)hipGetLastError();                            // (pageable memory is reported as an invalid value: not an error of ours)
    for (int k = 0; k < 2; k++) if (!c->in.ev_t_copy[k]) HIPCHK(c, hipEventCreateWithFlags(&c->in.ev_t_copy[k], hipEventDisableTiming));
    int b = 0;
    uint64_t k = 0;
    for (uint64_t at = 0; at < n; at += cap, k++) {
        b = (int)(k & 1);
        const uint64_t bytes = std::min<uint64_t>(cap, n - at);
        const uint8_t *from = h_bytes + at;
        if (!src_pinned) {
            HIPCHK(c, c->in.t_pin[b].ensure(cap));
            if (k >= 2) HIPCHK(c, hipEventSynchronize(c->in.ev_t_copy[b]));      // (the copy that last read this pinned buffer)
            memcpy(c->in.t_pin[b].p, from, bytes);
            from = c->in.t_pin[b].p;
        }
        HIPCHK(c, hipMemcpyAsync(dst + at, from, bytes, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(c, hipEventRecord(c->in.ev_t_copy[b], c->copy_stream));
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->in.ev_t_copy[b], 0));      // (the last copy: the copy stream runs them in order)
    return CRASS_OK;
}

// ---- the raw bytes of FASTA / FASTQ files in, parsed on the device (fastx_scan.hip) ----
// The scan of one file or several whose text lies on the device, file f at base[f] of one range of bytes with a byte of room
// behind it: base[f + 1] = base[f] + its size + 1 (a file on its own: base = {0, n + 1}).  The caller sizes x_tiles / x_base
// for all tiles and x_tot / x_h_tot for 5 words per planned file ([4 f ..): file f's totals, [4 n_planned + f]: its verdict),
// starts tm_scan, and queues scan_queue for each file as soon as its text is there; scan_emit then brings the totals back, has
// every file emit into one text and one pair of per-record arrays, and gives the verdict: the first file in order that offends.
namespace {
struct ScanResult {
    std::vector<uint64_t> rbase;                        // file f's records are [rbase[f], rbase[f + 1])
    uint64_t n_reads = 0, total_seq = 0, max_len = 0;
    // CRASS_ERR_UNSUPPORTED with decline_file >= 0: the input is declined, the position counts from that file's first byte
    int32_t decline_file = -1, decline_reason = 0; uint64_t decline_pos = 0;
};
}

static int scan_queue(crass_hip_ctx *c, FxJob &J, uint32_t f, const uint8_t *bytes, uint64_t n, int32_t format, uint64_t tile0, uint64_t n_tiles)
{
    J = FxJob{};
    J.bytes = bytes; J.n = n; J.lead = (uint32_t)((uintptr_t)bytes & 15u); J.format = format;
    J.n_tiles = n_tiles;
    J.tiles = c->in.x_tiles.p + tile0; J.base = c->in.x_base.p + tile0; J.tot = c->in.x_tot.p + 4 * (uint64_t)f;
    HIPCHK(c, launch_fx_summary(J, c->stream));
    HIPCHK(c, launch_fx_tile_scan(J, c->stream));
    return CRASS_OK;
}

// max_reads: a set of that many records or more is CRASS_ERR_UNSUPPORTED (the files' name table holds 32-bit indices)
static int scan_emit(crass_hip_ctx *c, FxJob *jobs, uint32_t nf, uint32_t n_planned, const uint64_t *base, uint64_t max_reads, ScanResult &R)
{
    Ingest &I = c->in;
    HIPCHK(c, hipMemcpyAsync(I.x_h_tot.p, I.x_tot.p, 4 * (uint64_t)nf * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (the record counts size the next kernels' arrays)
    std::vector<uint64_t> &rbase = R.rbase, tbase(nf + 1, 0);
    rbase.assign(nf + 1, 0);
    for (uint32_t f = 0; f < nf; f++) { rbase[f + 1] = rbase[f] + I.x_h_tot.p[4 * f + 1]; tbase[f + 1] = tbase[f] + I.x_h_tot.p[4 * f + 2]; }
    const uint64_t nr = rbase[nf], total_seq = tbase[nf];
    if (nr >= max_reads) return CRASS_ERR_UNSUPPORTED;
    HIPCHK(c, I.x_text.ensure(total_seq + 32));
    HIPCHK(c, I.x_rec_pos.ensure(nr + 1)); HIPCHK(c, I.x_seq_off.ensure(nr + 1));
    HIPCHK(c, I.x_h_rec_pos.ensure(nr + 1)); HIPCHK(c, I.x_h_seq_off.ensure(nr + 1));
    unsigned long long *d_verdict = reinterpret_cast<unsigned long long *>(I.x_tot.p + 4 * (uint64_t)n_planned);
    HIPCHK(c, hipMemsetAsync(d_verdict, 0xFF, 8 * (uint64_t)nf, c->stream));
    for (uint32_t f = 0; f < nf; f++) {
        FxJob &J = jobs[f];
        J.n_lines = I.x_h_tot.p[4 * f]; J.n_reads = rbase[f + 1] - rbase[f];
        J.text = I.x_text.p; J.text_base = tbase[f]; J.text_cap = tbase[f + 1];
        J.rec_pos = I.x_rec_pos.p; J.seq_off = I.x_seq_off.p; J.read_base = rbase[f]; J.arena_base = base[f];
        J.verdict = d_verdict + f;
        HIPCHK(c, launch_fx_emit(J, c->stream));
    }
    HIPCHK(c, I.tm_scan.mark(c->stream));
    uint64_t *h_verdict = I.x_h_tot.p + 4 * (uint64_t)n_planned;
    HIPCHK(c, hipMemcpyAsync(h_verdict, d_verdict, 8 * (uint64_t)nf, hipMemcpyDeviceToHost, c->stream));
    if (nr) {
        HIPCHK(c, hipMemcpyAsync(I.x_h_rec_pos.p, I.x_rec_pos.p, nr * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(I.x_h_seq_off.p, I.x_seq_off.p, nr * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_scan.elapsed(0, 1, &I.last_scan_ms));
    uint64_t *rec_pos = I.x_h_rec_pos.p, *seq_off = I.x_h_seq_off.p;
    rec_pos[nr] = base[nf] - 1; seq_off[nr] = total_seq;
    R.n_reads = nr; R.total_seq = total_seq; R.max_len = 0;
    auto decline = [&](uint32_t f, int32_t reason, uint64_t pos) {
        R.decline_file = (int32_t)f; R.decline_reason = reason; R.decline_pos = pos;
        return CRASS_ERR_UNSUPPORTED;
    };
    for (uint32_t f = 0; f < nf; f++) {
        const uint64_t verdict = h_verdict[f];
        if (verdict != kFxNoOffence) return decline(f, (int32_t)(verdict & 0xFF), verdict >> 8);
        const uint64_t seq_f = tbase[f + 1] - tbase[f];
        // (never expected: an accepted file has a record and as many quality as sequence bytes)
        if (rbase[f + 1] == rbase[f] || I.x_h_tot.p[4 * f + 3] != (jobs[f].format == 0x40 ? seq_f : 0)) return CRASS_ERR_STATE;
        for (uint64_t r = rbase[f]; r < rbase[f + 1]; r++) {
            const uint64_t l = (r + 1 < rbase[f + 1] ? seq_off[r + 1] : tbase[f + 1]) - seq_off[r];
            if (l > CRASS_HIP_MAX_READ_LEN) return decline(f, FX_READ_TOO_LONG, rec_pos[r] - base[f]);
            R.max_len = std::max(R.max_len, l);
        }
    }
    return CRASS_OK;
}

// One file: h_bytes (host) or d_bytes (device), in a load the caller has opened (begin_fastx_load).  Accepted: the state is that
// of crass_hip_load_text on the reads' text; declined: no reads.
static int load_fastx_impl(crass_hip_ctx *c, const uint8_t *h_bytes, const uint8_t *d_bytes, uint64_t n, int pad_uniform,
                           uint64_t read_index_base, crass_fastx_layout *out)
{
    auto decline = [&](int32_t format, uint64_t pos, int32_t reason) {
        if (out) { out->format = format; out->decline_pos = pos; out->decline_reason = reason; }
        return CRASS_ERR_UNSUPPORTED;
    };
    if (n == 0) return decline(0, 0, FX_EMPTY);
    uint8_t b0 = 0;
    if (h_bytes) b0 = h_bytes[0];
    else HIPCHK(c, hipMemcpy(&b0, d_bytes, 1, hipMemcpyDeviceToHost));
    if (!fx_is_hdr_char(b0)) return decline(0, 0, FX_FIRST_BYTE);
    Ingest &I = c->in;
    if (h_bytes) {
        HIPCHK(c, I.x_raw.ensure(n + 16));
        const int up = upload_staged(c, h_bytes, n, I.x_raw.p);
        if (up) return up;
        d_bytes = I.x_raw.p;
    }
    const uint64_t n_tiles = fastx_n_tiles(d_bytes, n);
    if (n_tiles > 0x7FFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (beyond 8 TB)
    HIPCHK(c, I.x_tiles.ensure(n_tiles)); HIPCHK(c, I.x_base.ensure(n_tiles));
    HIPCHK(c, I.x_tot.ensure(8)); HIPCHK(c, I.x_h_tot.ensure(8));
    FxJob J{};
    HIPCHK(c, I.tm_scan.begin(c->timing_level >= 1, c->stream));
    int s = scan_queue(c, J, 0, d_bytes, n, b0, 0, n_tiles);
    if (s) return s;
    const uint64_t base[2] = {0, n + 1};                // (rec_pos[n_reads] = n, and no '\n' is stored behind the bytes)
    ScanResult R;
    s = scan_emit(c, &J, 1, 1, base, ~0ull, R);
    if (s == CRASS_ERR_UNSUPPORTED && R.decline_file >= 0) return decline(b0, R.decline_pos, R.decline_reason);
    if (s) return s;
    s = load_text_impl(c, nullptr, I.x_text.p, I.x_h_seq_off.p, R.n_reads, pad_uniform, nullptr, read_index_base);
    if (s) return s;
    if (out) { out->n_reads = R.n_reads; out->format = b0; out->max_len = (uint32_t)R.max_len; out->rec_pos = I.x_h_rec_pos.p; out->seq_off = I.x_h_seq_off.p; }
    return CRASS_OK;
}

static int load_fastx_common(crass_hip_ctx *c, const uint8_t *h_bytes, const uint8_t *d_bytes, uint64_t n, int pad_uniform,
                             uint64_t read_index_base, crass_fastx_layout *out)
{
    if (out) memset(out, 0, sizeof(*out));
    if (!c || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    if (n && !h_bytes && !d_bytes) return CRASS_ERR_INVALID_ARG;
    begin_fastx_load(c);
    const int s = load_fastx_impl(c, h_bytes, d_bytes, n, pad_uniform, read_index_base, out);
    release_scan(c); release_text(c);                   // the scratch goes back on every way out, load_text_impl's part too
    return s;
}

int crass_hip_load_fastx_bytes(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                               crass_fastx_layout *out)
{
    return load_fastx_common(c, bytes, nullptr, n_bytes, pad_uniform, read_index_base, out);
}

int crass_hip_attach_device_fastx(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                  crass_fastx_layout *out)
{
    return load_fastx_common(c, nullptr, d_bytes, n_bytes, pad_uniform, read_index_base, out);
}

uint32_t crass_hip_fastx_tile_bytes(void) { return fastx_tile_bytes(); }
float crass_hip_last_scan_ms(const crass_hip_ctx *c) { return c ? c->in.last_scan_ms : 0.0f; }

// ---- BGZF members inflated on the device (inflate.hip) ----
// a compressed input is declined: the verdict, where the caller wants one
static int bz_decline(crass_bgzf_verdict *v, int32_t reason, uint64_t member, uint64_t in_pos)
{
    if (v) { v->reason = reason; v->member = member; v->in_pos = in_pos; }
    return CRASS_ERR_UNSUPPORTED;
}

// the index is checked, d_in / d_out are device pointers: upload the offsets, launch, read the verdict
// (the members [m0, m0 + n) of the index alone: d_in and d_out stay the places of the FILE's byte 0 and the TEXT's byte 0, which
// may lie outside what the caller holds — a member's bytes are read and written inside its own ranges only, inflate.hip)
static int inflate_bgzf_members(crass_hip_ctx *c, const uint8_t *d_in, const crass_bgzf_index *ix, uint64_t m0, uint64_t n, uint8_t *d_out,
                                crass_bgzf_verdict *v)
{
    c->in.last_inflate_ms = 0;
    if (n == 0) return CRASS_OK;
    HIPCHK(c, c->in.z_idx.ensure(3 * n + 2)); HIPCHK(c, c->in.z_reason.ensure(n)); HIPCHK(c, c->in.z_verdict.ensure(1)); HIPCHK(c, c->in.z_h_verdict.ensure(1));
    BzJob J{};
    J.in = d_in; J.out = d_out; J.n_members = n;
    J.in_off = c->in.z_idx.p; J.out_off = c->in.z_idx.p + (n + 1); J.data_off = c->in.z_idx.p + 2 * (n + 1);
    J.reason = c->in.z_reason.p; J.verdict = c->in.z_verdict.p; J.hbm_window = c->env.inflate_hbm_window ? 1 : 0;
    HIPCHK(c, hipMemcpyAsync(c->in.z_idx.p, ix->in_off + m0, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.z_idx.p + (n + 1), ix->out_off + m0, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.z_idx.p + 2 * (n + 1), ix->data_off + m0, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(J.verdict, 0xFF, 8, c->stream));
    HIPCHK(c, c->in.tm_inflate.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_bgzf_inflate(J, c->stream));
    HIPCHK(c, c->in.tm_inflate.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.z_h_verdict.p, J.verdict, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (the index's host arrays are the caller's: nothing reads them after this)
    HIPCHK(c, c->in.tm_inflate.elapsed(0, 1, &c->in.last_inflate_ms));
    const uint64_t w = c->in.z_h_verdict.p[0];
    if (w == kBzNoOffence) return CRASS_OK;
    return bz_decline(v, (int32_t)(w & 0xFF), m0 + (w >> 8), ix->in_off[m0 + (w >> 8)]);
}

static int inflate_bgzf_impl(crass_hip_ctx *c, const uint8_t *d_in, const crass_bgzf_index *ix, uint8_t *d_out, crass_bgzf_verdict *v)
{
    return inflate_bgzf_members(c, d_in, ix, 0, ix->n_members, d_out, v);
}

int crass_hip_inflate_bgzf_device(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, const crass_bgzf_index *ix, uint8_t *d_out, uint64_t out_cap,
                                  crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    if (!c) return CRASS_ERR_INVALID_ARG;
    const int chk = bgzf_index_check(ix, n_in, out_cap);
    if (chk) return chk;
    if (ix->n_members && (!d_in || (ix->out_off[ix->n_members] && !d_out))) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const int s = inflate_bgzf_impl(c, d_in, ix, d_out, v);
    release_bgzf(c);
    return s;
}

static int load_fastx_bgzf_impl(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, const crass_bgzf_index *ix, int pad_uniform,
                                uint64_t read_index_base, uint8_t *d_text, crass_fastx_layout *out, crass_bgzf_verdict *v)
{
    const uint64_t n_text = ix->out_off[ix->n_members];
    HIPCHK(c, c->in.z_raw.ensure(n_bytes + 16));
    const int up = upload_staged(c, bytes, n_bytes, c->in.z_raw.p);
    if (up) return up;
    if (!d_text) { HIPCHK(c, c->in.z_text.ensure(n_text + 16)); d_text = c->in.z_text.p; }
    const int s = inflate_bgzf_impl(c, c->in.z_raw.p, ix, d_text, v);
    if (s) return s;
    c->in.z_raw.release();                                 // (the compressed bytes are done with: the scan's arrays may have their room)
    return load_fastx_impl(c, nullptr, d_text, n_text, pad_uniform, read_index_base, out);
}

int crass_hip_load_fastx_bgzf(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base, uint8_t *d_text,
                              uint64_t d_text_cap, crass_fastx_layout *out, crass_bgzf_verdict *v)
{
    if (out) memset(out, 0, sizeof(*out));
    if (v) memset(v, 0, sizeof(*v));
    if (!c || pad_uniform < 0 || pad_uniform > 2 || (n_bytes && !bytes)) return CRASS_ERR_INVALID_ARG;
    crass_bgzf_index ix;
    int s = crass_bgzf_index_host(bytes, n_bytes, &ix);
    if (s == CRASS_OK && d_text && d_text_cap < ix.out_off[ix.n_members]) s = CRASS_ERR_INVALID_ARG;
    if (s == CRASS_ERR_INVALID_ARG || s == CRASS_ERR_OOM) { crass_bgzf_index_free(&ix); return s; }
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    if (s == CRASS_ERR_UNSUPPORTED) { if (v) *v = ix.decline; return s; }
    s = load_fastx_bgzf_impl(c, bytes, n_bytes, &ix, pad_uniform, read_index_base, d_text, out, v);
    release_bgzf(c); release_scan(c); release_text(c);  // the scratch goes back on every way out, as in load_fastx_common
    crass_bgzf_index_free(&ix);
    return s;
}

// ---- one plain gzip member inflated on the device chunk by chunk (gunzip.hip, gunzip_core.h) ----
namespace {
// what the count step and the chain walk decided about one file: all the decode step needs beside the bytes
struct GzState {
    GzMember M{};
    std::vector<uint64_t> start, text_len, end_bit;
    std::vector<uint32_t> link, chain;
    std::vector<int32_t> reason;
    uint64_t n_chain = 0, n_text = 0;
    // members mode (gunzip_core.h): what count reported about member ends, and after the decode step the member table
    bool members = false;
    uint64_t n_file = 0;
    std::vector<uint32_t> n_ends;
    std::vector<uint64_t> last_end, in_off, text_off;
};
}

// header and trailer (host), find and count (device), the chain (host): CRASS_OK with S.n_text known, or the decline
// (members: the rule's members mode, kept in S for the decode step)
static int gzip_count_impl(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, GzState &S, crass_gzip_plan *plan,
                           crass_bgzf_verdict *v, bool members = false)
{
    S.members = members; S.n_file = n_in;
    c->in.last_inflate_ms = 0;
    for (auto &m : c->in.last_gzip_ms) m = 0;
    try {
        // the header's bytes come down in a piece that grows until the header ends inside it
        std::vector<uint8_t> head;
        uint8_t trailer[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n_in >= 18) HIPCHK(c, hipMemcpy(trailer, d_in + n_in - 8, 8, hipMemcpyDeviceToHost));
        int32_t why = BZ_NOT_GZIP;
        for (uint64_t h = std::min<uint64_t>(n_in, 65536);; h = std::min<uint64_t>(n_in, h * 4)) {
            head.resize(h ? h : 1);
            if (h) HIPCHK(c, hipMemcpy(head.data(), d_in, h, hipMemcpyDeviceToHost));
            why = gz_parse_member(head.data(), h, trailer, n_in, chunk_bytes, &S.M);
            if (why != -1 || h == n_in) break;
        }
        if (why != BZ_OK) return bz_decline(v, BZ_NOT_GZIP, 0, 0);
        const GzGeom &G = S.M.G;
        const uint64_t nc = G.nc;
        HIPCHK(c, c->in.gz_a64.ensure((members ? 4 : 3) * nc)); HIPCHK(c, c->in.gz_a32.ensure((members ? 3 : 2) * nc));
        GzJob J{};
        J.d = d_in + G.d_off; J.G = G;
        J.start = c->in.gz_a64.p; J.text_len = c->in.gz_a64.p + nc; J.end_bit = c->in.gz_a64.p + 2 * nc;
        J.link = c->in.gz_a32.p; J.reason = reinterpret_cast<int32_t *>(c->in.gz_a32.p + nc);
        if (members) { J.last_end = c->in.gz_a64.p + 3 * nc; J.n_ends = c->in.gz_a32.p + 2 * nc; }
        StageTimer<6> &T = c->in.tm_gzip;
        HIPCHK(c, T.begin(c->timing_level >= 1, c->stream));
        HIPCHK(c, launch_gz_find(J, c->stream, members));
        HIPCHK(c, T.mark(c->stream));
        HIPCHK(c, launch_gz_count(J, c->stream, members));      // (a launch of its own: every start is final before a chunk counts)
        HIPCHK(c, T.mark(c->stream));
        S.start.resize(nc); S.text_len.resize(nc); S.end_bit.resize(nc); S.link.resize(nc); S.reason.resize(nc); S.chain.assign(nc, 0);
        HIPCHK(c, hipMemcpyAsync(S.start.data(), J.start, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.text_len.data(), J.text_len, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.end_bit.data(), J.end_bit, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.link.data(), J.link, nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.reason.data(), J.reason, nc * 4, hipMemcpyDeviceToHost, c->stream));
        if (members) {
            S.n_ends.resize(nc); S.last_end.resize(nc);
            HIPCHK(c, hipMemcpyAsync(S.n_ends.data(), J.n_ends, nc * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(S.last_end.data(), J.last_end, nc * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 2; k++) HIPCHK(c, T.elapsed(k, k + 1, &c->in.last_gzip_ms[k]));
        c->in.last_inflate_ms = c->in.last_gzip_ms[0] + c->in.last_gzip_ms[1];
        GzVerdict gv{};
        const int32_t bad = gz_chain(S.M, S.start.data(), S.link.data(), S.text_len.data(), S.end_bit.data(), S.reason.data(), S.chain.data(),
                                     &S.n_chain, &S.n_text, &gv, members);
        const int ps = gz_plan_fill(plan, nc, S.start.data(), S.link.data(), S.text_len.data(), S.n_chain);
        if (ps) return ps;
        if (bad != BZ_OK) return bz_decline(v, gv.reason, gv.member, gv.in_pos);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

// decode, windows, narrow: the text of an accepted count into d_out[0, S.n_text)
// (members mode: every member's ISIZE and CRC-32 are checked here, behind the kernels; S gets the member table)
static int gzip_decode_impl(crass_hip_ctx *c, const uint8_t *d_in, GzState &S, uint8_t *d_out, crass_bgzf_verdict *v)
{
    const bool members = S.members;
    const GzGeom &G = S.M.G;
    const uint64_t nc = G.nc, n = S.n_chain;
    try {
        std::vector<uint64_t> off(n + 1, 0);
        for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + S.text_len[S.chain[i]];
        std::vector<uint32_t> crc_part(n, 0);
        // members mode: [slot (n + 1) | m0 (n)] go up behind off; the pieces' bounds follow once the member table is known
        std::vector<uint64_t> places(2 * n + 1, 0);
        if (members) {
            std::vector<uint64_t> off2(n + 1, 0);
            gz_places(S.chain.data(), n, S.text_len.data(), S.n_ends.data(), S.last_end.data(), off2.data(), places.data(), places.data() + n + 1);
        }
        const uint64_t nm = members ? places[n] : 0;
        const uint64_t max_pieces = members ? nm + S.n_text / kGzCrcPiece + 1 : 0;
        HIPCHK(c, c->in.gz_b64.ensure(2 * nc + n + 1 + (members ? 2 * n + 1 + max_pieces + 1 : 0))); HIPCHK(c, c->in.gz_b32.ensure(2 * n + max_pieces));
        if (members) HIPCHK(c, c->in.gz_ends.ensure(3 * (nm ? nm : 1)));
        HIPCHK(c, c->in.gz_sym.ensure(S.n_text)); HIPCHK(c, c->in.gz_win.ensure(n * (uint64_t)kGzWindow));
        HIPCHK(c, c->in.z_verdict.ensure(1)); HIPCHK(c, c->in.z_h_verdict.ensure(1));
        GzJob J{};
        J.d = d_in + G.d_off; J.G = G;
        J.start = c->in.gz_b64.p; J.end_bit = c->in.gz_b64.p + nc;
        J.n_chain = n; J.off = c->in.gz_b64.p + 2 * nc; J.chain = c->in.gz_b32.p; J.crc_part = c->in.gz_b32.p + n;
        J.sym = c->in.gz_sym.p; J.win = c->in.gz_win.p; J.out = d_out; J.verdict = c->in.z_verdict.p;
        if (members) {
            static_assert(sizeof(GzEnd) == 24 && alignof(GzEnd) == 8, "GzEnd is three words");
            uint64_t *pl = c->in.gz_b64.p + 2 * nc + n + 1;
            J.slot = pl; J.m0 = pl + n + 1; J.piece = pl + 2 * n + 1; J.crc_piece = c->in.gz_b32.p + 2 * n;
            J.ends = reinterpret_cast<GzEnd *>(c->in.gz_ends.p);
            HIPCHK(c, hipMemcpyAsync(pl, places.data(), (2 * n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(J.start, S.start.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(J.end_bit, S.end_bit.data(), nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.gz_b64.p + 2 * nc, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.gz_b32.p, S.chain.data(), n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(J.verdict, 0xFF, 8, c->stream));
        StageTimer<6> &T = c->in.tm_gzip;
        HIPCHK(c, T.begin(c->timing_level >= 1, c->stream, 2));      // (the count step's last mark again: the uploads above are not decode's)
        HIPCHK(c, launch_gz_decode(J, c->stream, members));
        HIPCHK(c, T.mark(c->stream));
        HIPCHK(c, launch_gz_windows(J, c->stream));
        HIPCHK(c, T.mark(c->stream));
        HIPCHK(c, launch_gz_narrow(J, c->stream, members));
        std::vector<uint64_t> piece;
        std::vector<uint32_t> mcrc, misz;
        if (members) {
            // the records come down (the stream is waited for: decode is done, narrow may still run), the member table and the
            // pieces are made, the pieces' bounds go up for k_gz_member_crc; narrow's time then includes that round trip
            std::vector<GzEnd> ends(nm ? nm : 1);
            HIPCHK(c, hipMemcpyAsync(ends.data(), J.ends, nm * sizeof(GzEnd), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            S.in_off.assign(nm + 1, 0); S.text_off.assign(nm + 1, 0); mcrc.assign(nm, 0); misz.assign(nm, 0);
            gz_member_table(S.M, S.n_file, off.data(), places.data(), n, ends.data(), S.in_off.data(), S.text_off.data(), mcrc.data(), misz.data());
            for (uint64_t m = 0; m < nm; m++) {
                if (S.text_off[m + 1] < S.text_off[m] || S.text_off[m + 1] > S.n_text) return CRASS_ERR_STATE;      // (a record nobody wrote)
                for (uint64_t p = S.text_off[m]; p < S.text_off[m + 1]; p += kGzCrcPiece) piece.push_back(p);
            }
            piece.push_back(S.n_text);
            if (piece.size() - 1 > max_pieces) return CRASS_ERR_STATE;
            J.n_pieces = piece.size() - 1;
            HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t *>(J.piece), piece.data(), piece.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, launch_gz_member_crc(J, c->stream));
        }
        HIPCHK(c, T.mark(c->stream));
        std::vector<uint32_t> crc_piece(members ? piece.size() : 1, 0);
        if (members && J.n_pieces) HIPCHK(c, hipMemcpyAsync(crc_piece.data(), J.crc_piece, J.n_pieces * 4, hipMemcpyDeviceToHost, c->stream));
        if (!members) HIPCHK(c, hipMemcpyAsync(crc_part.data(), J.crc_part, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.z_h_verdict.p, J.verdict, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int k = 2; k < 5; k++) {
            HIPCHK(c, T.elapsed(k, k + 1, &c->in.last_gzip_ms[k]));
            c->in.last_inflate_ms += c->in.last_gzip_ms[k];
        }
        const uint64_t w = c->in.z_h_verdict.p[0];
        if (w != kBzNoOffence) {
            const uint64_t k = S.chain[w];
            return bz_decline(v, BZ_MARKER, k, G.d_off + (S.start[k] >> 3));
        }
        if (members) {
            // a member's pieces joined in text order (an empty member has none: CRC 0)
            std::vector<uint32_t> got(nm, 0);
            uint64_t q = 0;
            for (uint64_t m = 0; m < nm; m++)
                for (; q + 1 < piece.size() && piece[q] < S.text_off[m + 1]; q++) got[m] = gz_crc_join(got[m], crc_piece[q], piece[q + 1] - piece[q]);
            GzVerdict mv{};
            if (gz_member_verdict(nm, S.in_off.data(), S.text_off.data(), mcrc.data(), misz.data(), got.data(), &mv) != BZ_OK)
                return bz_decline(v, mv.reason, mv.member, mv.in_pos);
            return CRASS_OK;
        }
        uint32_t crc = 0;
        for (uint64_t i = 0; i < n; i++) crc = gz_crc_join(crc, crc_part[i], off[i + 1] - off[i]);
        if (crc != S.M.crc) return bz_decline(v, BZ_CRC, 0, 0);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

static int inflate_gzip_device_impl(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                    uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, bool mode, crass_bgzf_verdict *v)
{
    if (v) memset(v, 0, sizeof(*v));
    if (plan) memset(plan, 0, sizeof(*plan));
    if (members) memset(members, 0, sizeof(*members));
    if (n_text) *n_text = 0;
    if (!c || !n_text || (n_in && !d_in) || (out_cap && !d_out)) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    GzState S;
    int s = gzip_count_impl(c, d_in, n_in, chunk_bytes, S, plan, v, mode);
    if (s == CRASS_OK) {
        *n_text = S.n_text;
        if (out_cap < S.n_text) s = CRASS_ERR_OVERFLOW;       // (known before anything is stored)
        else s = gzip_decode_impl(c, d_in, S, d_out, v);
        if (s == CRASS_OK && mode) s = gz_members_fill(members, S.in_off.size() - 1, S.in_off.data(), S.text_off.data());
    }
    release_gzip(c); release_bgzf(c);                   // (the verdict word is the BGZF inflate's)
    return s;
}

int crass_hip_inflate_gzip_device(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                  uint64_t *n_text, crass_gzip_plan *plan, crass_bgzf_verdict *v)
{
    return inflate_gzip_device_impl(c, d_in, n_in, chunk_bytes, d_out, out_cap, n_text, plan, nullptr, false, v);
}

int crass_hip_inflate_gzip_members_device(crass_hip_ctx *c, const uint8_t *d_in, uint64_t n_in, uint64_t chunk_bytes, uint8_t *d_out, uint64_t out_cap,
                                          uint64_t *n_text, crass_gzip_plan *plan, crass_gzip_members *members, crass_bgzf_verdict *v)
{
    return inflate_gzip_device_impl(c, d_in, n_in, chunk_bytes, d_out, out_cap, n_text, plan, members, true, v);
}

static int load_fastx_gzip_impl(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base, uint8_t *d_text,
                                uint64_t d_text_cap, crass_fastx_layout *out, crass_gzip_members *members, bool mode, crass_bgzf_verdict *v)
{
    if (out) memset(out, 0, sizeof(*out));
    if (v) memset(v, 0, sizeof(*v));
    if (members) memset(members, 0, sizeof(*members));
    if (!c || pad_uniform < 0 || pad_uniform > 2 || (n_bytes && !bytes)) return CRASS_ERR_INVALID_ARG;
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    auto run = [&]() -> int {
        HIPCHK(c, c->in.z_raw.ensure(n_bytes + 16));
        const int up = upload_staged(c, bytes, n_bytes, c->in.z_raw.p);
        if (up) return up;
        HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        GzState S;
        int s = gzip_count_impl(c, c->in.z_raw.p, n_bytes, 0, S, nullptr, v, mode);
        if (s) return s;
        if (d_text && d_text_cap < S.n_text) return CRASS_ERR_INVALID_ARG;
        if (!d_text) { HIPCHK(c, c->in.z_text.ensure(S.n_text + 16)); d_text = c->in.z_text.p; }
        s = gzip_decode_impl(c, c->in.z_raw.p, S, d_text, v);
        if (s) return s;
        if (mode) { s = gz_members_fill(members, S.in_off.size() - 1, S.in_off.data(), S.text_off.data()); if (s) return s; }
        release_gzip(c);
        c->in.z_raw.release();                             // (the compressed bytes are done with: the scan's arrays may have their room)
        return load_fastx_impl(c, nullptr, d_text, S.n_text, pad_uniform, read_index_base, out);
    };
    const int s = run();
    release_gzip(c); release_bgzf(c); release_scan(c); release_text(c);      // the scratch goes back on every way out
    if (s && members) crass_gzip_members_free(members);      // (a scan decline behind an accepted inflate: no table without reads)
    return s;
}

int crass_hip_load_fastx_gzip(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base, uint8_t *d_text,
                              uint64_t d_text_cap, crass_fastx_layout *out, crass_bgzf_verdict *v)
{
    return load_fastx_gzip_impl(c, bytes, n_bytes, pad_uniform, read_index_base, d_text, d_text_cap, out, nullptr, false, v);
}

int crass_hip_load_fastx_gzip_members(crass_hip_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int pad_uniform, uint64_t read_index_base,
                                      uint8_t *d_text, uint64_t d_text_cap, crass_fastx_layout *out, crass_gzip_members *members,
                                      crass_bgzf_verdict *v)
{
    return load_fastx_gzip_impl(c, bytes, n_bytes, pad_uniform, read_index_base, d_text, d_text_cap, out, members, true, v);
}

int crass_hip_set_gzip_on_device(crass_hip_ctx *c, int on)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    c->in.gzip_on_device = on == CRASS_GZIP_ON_DEVICE_MEMBERS ? CRASS_GZIP_ON_DEVICE_MEMBERS : on != 0 ? CRASS_GZIP_ON_DEVICE_ONE_MEMBER : CRASS_GZIP_ON_DEVICE_OFF;
    return CRASS_OK;
}

int crass_hip_last_gzip_ms(const crass_hip_ctx *c, float *ms)
{
    if (!c || !ms) return CRASS_ERR_INVALID_ARG;
    for (int k = 0; k < 5; k++) ms[k] = c->in.last_gzip_ms[k];
    return CRASS_OK;
}

float crass_hip_last_inflate_ms(const crass_hip_ctx *c) { return c ? c->in.last_inflate_ms : 0.0f; }

// new header ids: pass 1's found flags are keyed by them, so earlier results are void; the resident set's own counters stay
static void reset_results_keep_set(crass_hip_ctx *c)
{
    const uint64_t n_reads = c->cnt.n_reads, n_exc = c->cnt.n_exceptions, bytes_dev = c->cnt.bytes_reads_device;
    reset_results(c);
    c->cnt.n_reads = n_reads; c->cnt.n_exceptions = n_exc; c->cnt.bytes_reads_device = bytes_dev;
}

int crass_hip_set_header_ids(crass_hip_ctx *c, const uint64_t *header_id)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    if (!c->have_reads) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    reset_results_keep_set(c);
    const uint64_t n = c->R.n_reads;
    if (header_id && n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));     // (nothing may still read the array this replaces)
        HIPCHK(c, c->r_header_id.ensure(n));
        HIPCHK(c, hipMemcpy(c->r_header_id.p, header_id, n * 8, hipMemcpyHostToDevice));
        c->R.header_id = c->r_header_id.p;
    } else c->R.header_id = nullptr;
    return CRASS_OK;
}

// ---- header ids from a file's raw bytes on the device (fastx_names.hip) ----
// Every check that needs no byte of the file comes first; a record position outside the input is seen by the insert launch and
// reported before the lookup launch and before anything is installed.
// the insert step, shared by the header ids (the table is scratch) and crass_hip_fastx_names_build_device (the table is kept):
// table and d_rec_pos are the two arrays that make a table, the slots per record, the list of long names and the control words
// are the context's scratch.  Queued on return: both insert launches; tm_names' marks 0 and 1 lie around them when timed.
static int names_insert_impl(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n,
                             DevBuf<unsigned long long> &table, DevBuf<uint64_t> &d_rec_pos, HidJob &J)
{
    uint64_t slots = 2;
    while (slots < 2 * n) slots <<= 1;
    HIPCHK(c, d_rec_pos.ensure(n)); HIPCHK(c, c->in.n_ids.ensure(n)); HIPCHK(c, c->in.n_long.ensure(n));
    HIPCHK(c, c->in.n_ctl.ensure(4)); HIPCHK(c, c->in.n_h_ctl.ensure(4)); HIPCHK(c, table.ensure(slots));
    J = HidJob{};
    J.bytes = d_bytes; J.n_bytes = n_bytes; J.rec_pos = d_rec_pos.p; J.n_reads = n;
    J.table = table.p; J.mask = slots - 1; J.hash_bits = c->env.hid_hash_bits;
    J.ids = c->in.n_ids.p; J.long_list = c->in.n_long.p;
    J.ctl = reinterpret_cast<uint32_t *>(c->in.n_ctl.p); J.n_repeated = reinterpret_cast<unsigned long long *>(c->in.n_ctl.p + 2);
    HIPCHK(c, hipMemcpyAsync(d_rec_pos.p, rec_pos, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(table.p, 0xFF, slots * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->in.n_ctl.p, 0, 32, c->stream));
    HIPCHK(c, c->in.tm_names.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_hid_insert(J, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.n_h_ctl.p, c->in.n_ctl.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (how many long names there are sizes the wave kernel's launch)
    const uint32_t *h_ctl = reinterpret_cast<const uint32_t *>(c->in.n_h_ctl.p);
    if (h_ctl[1]) return CRASS_ERR_INVALID_ARG;         // a rec_pos[r] >= n_bytes
    if (h_ctl[0]) HIPCHK(c, launch_hid_insert_long(J, h_ctl[0], c->stream));
    HIPCHK(c, c->in.tm_names.mark(c->stream));
    return CRASS_OK;
}

static int header_ids_device_impl(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n,
                                  uint64_t *header_id_out, int install, uint64_t *n_repeated_out)
{
    (void)hipSetDevice(c->device);
    for (auto &m : c->in.last_hid_ms) m = 0;
    HidJob J{};
    const int ins = names_insert_impl(c, d_bytes, n_bytes, rec_pos, n, c->in.n_table, c->in.n_rec_pos, J);
    if (ins) return ins;
    StageTimer<3> &T = c->in.tm_names;
    HIPCHK(c, launch_hid_lookup(J, c->stream));
    HIPCHK(c, T.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.n_h_ctl.p + 2, c->in.n_ctl.p + 2, 8, hipMemcpyDeviceToHost, c->stream));
    if (header_id_out) HIPCHK(c, hipMemcpyAsync(header_id_out, c->in.n_ids.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, T.elapsed(0, 2, &c->in.last_hid_ms[0]));
    HIPCHK(c, T.elapsed(0, 1, &c->in.last_hid_ms[1]));
    HIPCHK(c, T.elapsed(1, 2, &c->in.last_hid_ms[2]));
    if (n_repeated_out) *n_repeated_out = c->in.n_h_ctl.p[2];
    if (install) {                                      // crass_hip_set_header_ids, the array from where it is
        reset_results_keep_set(c);
        HIPCHK(c, c->r_header_id.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->r_header_id.p, c->in.n_ids.p, n * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->R.header_id = c->r_header_id.p;
    }
    return CRASS_OK;
}

int crass_hip_fastx_header_ids_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                      uint64_t *header_id_out, int install, uint64_t *n_repeated_out)
{
    if (!c || (n_reads && (!d_bytes || !rec_pos))) return CRASS_ERR_INVALID_ARG;
    if (n_reads >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (a slot holds a 32-bit index, all-ones is the free slot's)
    if (install) {
        if (!c->have_reads) return CRASS_ERR_STATE;
        if (n_reads != c->R.n_reads) return CRASS_ERR_INVALID_ARG;
    }
    if (n_repeated_out) *n_repeated_out = 0;
    if (n_reads == 0) return install ? crass_hip_set_header_ids(c, nullptr) : CRASS_OK;
    (void)hipSetDevice(c->device);
    if (install) HIPCHK(c, hipStreamSynchronize(c->stream));      // (nothing may still read the array this replaces)
    const int s = header_ids_device_impl(c, d_bytes, n_bytes, rec_pos, n_reads, header_id_out, install, n_repeated_out);
    release_header_ids(c);                              // the scratch goes back on every way out
    return s;
}

float crass_hip_last_header_ids_ms(const crass_hip_ctx *c, int part) { return c && part >= 0 && part < 3 ? c->in.last_hid_ms[part] : 0.0f; }

// ---- the name table kept on the device: names in, first read index out (fastx_names.hip) ----
// The table is built aside and replaces the one before only when the insert step accepted every record position: a build that
// fails leaves the context as it was.
static int names_build_impl(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n,
                            DevBuf<unsigned long long> &table, DevBuf<uint64_t> &d_rec_pos, uint64_t *mask_out)
{
    HidJob J{};
    const int ins = names_insert_impl(c, d_bytes, n_bytes, rec_pos, n, table, d_rec_pos, J);
    if (ins) return ins;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->in.tm_names.elapsed(0, 1, &c->in.last_names_ms[0]));
    *mask_out = J.mask;
    return CRASS_OK;
}

int crass_hip_fastx_names_build_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    const bool on_arena = !d_bytes && !rec_pos;
    if (on_arena) {                                     // the arena and layout of the last crass_hip_load_fastx_files
        if (!c->in.have_arena || !c->have_reads) return CRASS_ERR_STATE;
        d_bytes = c->in.fa_arena.p; n_bytes = c->in.fa_bytes; rec_pos = c->in.x_h_rec_pos.p; n_reads = c->R.n_reads;
    }
    if (n_reads && (!d_bytes || !rec_pos)) return CRASS_ERR_INVALID_ARG;
    if (n_reads >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (a slot holds a 32-bit index, all-ones is the free slot's)
    (void)hipSetDevice(c->device);
    c->in.last_names_ms[0] = 0;
    DevBuf<unsigned long long> table; DevBuf<uint64_t> d_rec_pos;
    uint64_t mask = 0;
    const int s = n_reads ? names_build_impl(c, d_bytes, n_bytes, rec_pos, n_reads, table, d_rec_pos, &mask) : CRASS_OK;
    release_header_ids(c);                              // the scratch goes back on every way out (the table built here is a local)
    if (s) { table.release(); d_rec_pos.release(); return s; }
    names_drop(c);
    c->in.nt_table = table; c->in.nt_rec_pos = d_rec_pos;     // (DevBuf owns nothing by itself: the context's release gives them back)
    c->in.have_names = true; c->in.nt_on_arena = on_arena;
    c->in.nt_bytes = d_bytes; c->in.nt_n_bytes = n_bytes; c->in.nt_n_reads = n_reads; c->in.nt_mask = mask;
    return CRASS_OK;
}

static int names_find_impl(crass_hip_ctx *c, const uint8_t *names, const uint64_t *name_off, uint64_t n_names, const std::vector<uint32_t> &longs,
                           uint64_t *first_out)
{
    const uint64_t total = name_off[n_names];
    HIPCHK(c, c->in.nq_names.ensure(total)); HIPCHK(c, c->in.nq_off.ensure(n_names + 1)); HIPCHK(c, c->in.nq_out.ensure(n_names));
    HIPCHK(c, c->in.nq_long.ensure(longs.size()));
    HidFindJob J{};
    J.bytes = c->in.nt_bytes; J.n_bytes = c->in.nt_n_bytes; J.rec_pos = c->in.nt_rec_pos.p;
    J.table = c->in.nt_table.p; J.mask = c->in.nt_mask; J.hash_bits = c->env.hid_hash_bits;
    J.names = c->in.nq_names.p; J.name_off = c->in.nq_off.p; J.n_names = n_names; J.long_list = c->in.nq_long.p; J.first_out = c->in.nq_out.p;
    if (total) HIPCHK(c, hipMemcpyAsync(c->in.nq_names.p, names, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.nq_off.p, name_off, (n_names + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (!longs.empty()) HIPCHK(c, hipMemcpyAsync(c->in.nq_long.p, longs.data(), longs.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->in.tm_find.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_hid_find(J, c->stream));
    if (!longs.empty()) HIPCHK(c, launch_hid_find_long(J, (uint32_t)longs.size(), c->stream));
    HIPCHK(c, c->in.tm_find.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(first_out, c->in.nq_out.p, n_names * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->in.tm_find.elapsed(0, 1, &c->in.last_names_ms[1]));
    return CRASS_OK;
}

int crass_hip_fastx_names_find(crass_hip_ctx *c, const uint8_t *names, const uint64_t *name_off, uint64_t n_names, uint64_t *first_out)
{
    if (!c || (n_names && (!name_off || !first_out))) return CRASS_ERR_INVALID_ARG;
    for (uint64_t k = 0; k < n_names; k++) if (name_off[k + 1] < name_off[k]) return CRASS_ERR_INVALID_ARG;
    if (n_names && name_off[n_names] && !names) return CRASS_ERR_INVALID_ARG;
    if (n_names >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (the list of long queries holds 32-bit indices)
    if (!c->in.have_names) return CRASS_ERR_STATE;
    c->in.last_names_ms[1] = 0;
    if (n_names == 0) return CRASS_OK;
    if (c->in.nt_n_reads == 0) { for (uint64_t k = 0; k < n_names; k++) first_out[k] = CRASS_NAME_NOT_FOUND; return CRASS_OK; }
    std::vector<uint32_t> longs;
    try {
        const uint64_t lane_end = hid_lane_end();
        for (uint64_t k = 0; k < n_names; k++) if (name_off[k + 1] - name_off[k] >= lane_end) longs.push_back((uint32_t)k);
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    (void)hipSetDevice(c->device);
    const int s = names_find_impl(c, names, name_off, n_names, longs, first_out);
    release_names_find(c);                              // the scratch goes back on every way out; the table stays
    return s;
}

// ---- the same exchange with everything in device memory: names out (k_nm_*), names looked up (k_hid_find_dev) ----
// The host reads counts only: the total and the flag word of a names-of call, the two control words of a find.
static int names_find_device_impl(crass_hip_ctx *c, const uint8_t *d_names, uint64_t n_name_bytes, const uint64_t *d_name_off, uint64_t n_names,
                                  uint64_t *d_first_out)
{
    Ingest &I = c->in;
    HIPCHK(c, I.nq_long.ensure(n_names)); HIPCHK(c, I.nq_ctl.ensure(4)); HIPCHK(c, I.nq_h_ctl.ensure(2));      // (words 2 and 3: the 64-bit count of answers that name a record)
    HidFindJob J{};
    J.bytes = I.nt_bytes; J.n_bytes = I.nt_n_bytes; J.rec_pos = I.nt_rec_pos.p;
    J.table = I.nt_table.p; J.mask = I.nt_mask; J.hash_bits = c->env.hid_hash_bits;
    J.names = d_names; J.name_off = d_name_off; J.n_names = n_names; J.long_list = I.nq_long.p; J.first_out = d_first_out;
    HidFindDev D{};
    D.n_name_bytes = n_name_bytes; D.long_app = I.nq_long.p; D.ctl = I.nq_ctl.p;
    HIPCHK(c, hipMemsetAsync(I.nq_ctl.p, 0, 16, c->stream));
    HIPCHK(c, I.tm_find.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_hid_find_dev(J, D, c->stream));
    HIPCHK(c, hipMemcpyAsync(I.nq_h_ctl.p, I.nq_ctl.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (how many long queries there are sizes the wave kernel's launch)
    const uint32_t *h_ctl = reinterpret_cast<const uint32_t *>(I.nq_h_ctl.p);
    const uint32_t n_long = h_ctl[0], bad = h_ctl[1];
    if (n_long > n_names) return CRASS_ERR_STATE;       // (never expected: a lane appends at most once)
    if (n_long) HIPCHK(c, launch_hid_find_long(J, n_long, c->stream));
    HIPCHK(c, launch_hid_count_found(d_first_out, n_names, reinterpret_cast<unsigned long long *>(I.nq_ctl.p + 2), c->stream));
    HIPCHK(c, I.tm_find.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(I.nq_h_ctl.p + 1, I.nq_ctl.p + 2, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_find.elapsed(0, 1, &I.last_names_ms[1]));
    I.last_find_found = I.nq_h_ctl.p[1];
    return bad ? CRASS_ERR_INVALID_ARG : CRASS_OK;
}

int crass_hip_fastx_names_find_device(crass_hip_ctx *c, const uint8_t *d_names, uint64_t n_name_bytes, const uint64_t *d_name_off, uint64_t n_names,
                                      uint64_t *d_first_out)
{
    if (!c || (n_names && (!d_name_off || !d_first_out)) || (n_name_bytes && !d_names)) return CRASS_ERR_INVALID_ARG;
    if (n_names >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;      // (the list of long queries holds 32-bit indices)
    if (!c->in.have_names) return CRASS_ERR_STATE;
    c->in.last_names_ms[1] = 0; c->in.last_find_found = 0;
    if (n_names == 0) return CRASS_OK;
    (void)hipSetDevice(c->device);
    if (c->in.nt_n_reads == 0) {                        // a table of no records: every query is CRASS_NAME_NOT_FOUND (all bits set)
        HIPCHK(c, hipMemsetAsync(d_first_out, 0xFF, n_names * 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CRASS_OK;
    }
    const int s = names_find_device_impl(c, d_names, n_name_bytes, d_name_off, n_names, d_first_out);
    release_names_find(c);                              // the scratch goes back on every way out; the table stays
    return s;
}

static int names_of_device_impl(crass_hip_ctx *c, const uint64_t *d_idx, uint64_t n, uint64_t idx_base, uint8_t *d_chars, uint64_t cap_bytes,
                                uint64_t *d_off, uint64_t *total_out)
{
    Ingest &I = c->in;
    const uint64_t tiles = (n + nm_scan_tile() - 1) / nm_scan_tile();
    HIPCHK(c, I.no_len.ensure(n)); HIPCHK(c, I.no_flag.ensure(1)); HIPCHK(c, I.no_tiles.ensure(tiles + 1)); HIPCHK(c, I.no_h.ensure(2));
    NmOfJob J{};
    J.bytes = I.nt_bytes; J.n_bytes = I.nt_n_bytes; J.rec_pos = I.nt_rec_pos.p; J.n_reads = I.nt_n_reads;
    J.idx = d_idx; J.n = n; J.idx_base = idx_base;
    J.len = I.no_len.p; J.flag = I.no_flag.p; J.tile_sum = I.no_tiles.p; J.off = d_off; J.out = d_chars;
    HIPCHK(c, hipMemsetAsync(I.no_flag.p, 0, 4, c->stream));
    I.no_h.p[1] = 0;
    HIPCHK(c, launch_nm_measure_idx(J, c->stream));
    HIPCHK(c, launch_nm_scan(J, c->stream));
    HIPCHK(c, hipMemcpyAsync(I.no_h.p, d_off + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(I.no_h.p + 1, I.no_flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // (the total sizes the copy launch and is the caller's one host read)
    const uint64_t total = I.no_h.p[0];
    if (total_out) *total_out = total;
    if (I.no_h.p[1]) return CRASS_ERR_INVALID_ARG;      // an entry outside [0, n_reads): no byte is written
    J.limit = std::min(total, cap_bytes);
    if (J.limit) {
        HIPCHK(c, launch_nm_copy(J, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return total > cap_bytes ? CRASS_ERR_OVERFLOW : CRASS_OK;
}

int crass_hip_fastx_names_of_device(crass_hip_ctx *c, const uint64_t *d_idx, uint64_t n, uint64_t idx_base, uint8_t *d_chars, uint64_t cap_bytes,
                                    uint64_t *d_off, uint64_t *total_out)
{
    if (!c || !d_off || (n && !d_idx) || (cap_bytes && !d_chars)) return CRASS_ERR_INVALID_ARG;
    if (n >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;
    if (!c->in.have_names) return CRASS_ERR_STATE;
    if (total_out) *total_out = 0;
    (void)hipSetDevice(c->device);
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(d_off, 0, 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CRASS_OK;
    }
    const int s = names_of_device_impl(c, d_idx, n, idx_base, d_chars, cap_bytes, d_off, total_out);
    release_names_of(c);                                // the scratch goes back on every way out
    return s;
}

int crass_hip_found_names_device(crass_hip_ctx *c, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *d_off, uint64_t cap_names, uint64_t *n_out,
                                 uint64_t *total_out)
{
    if (!c || !n_out || (cap_bytes && !d_chars) || (cap_names && !d_off)) return CRASS_ERR_INVALID_ARG;
    *n_out = 0;
    if (total_out) *total_out = 0;
    if (!c->in.have_names) return CRASS_ERR_STATE;
    if (c->p1d.active) { const int ds = settle_p1(c); if (ds) return ds; }
    if (!c->have_pass1) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    const uint64_t n = c->n_cand();
    *n_out = n;
    if (n >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;
    if (n == 0) {
        if (d_off) { HIPCHK(c, hipMemsetAsync(d_off, 0, 8, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
        return CRASS_OK;
    }
    // too few offset words: the names are measured into scratch of ours, so that the caller learns n and the total at once
    const bool short_off = cap_names < n;
    if (short_off) { HIPCHK(c, c->in.no_off.ensure(n + 1)); d_off = c->in.no_off.p; cap_bytes = 0; }
    const uint64_t *d_idx;
    if (c->dense.active) d_idx = reinterpret_cast<const uint64_t *>(c->dense.d_blob.p + c->dense.lay.read);      // pass 1's records, where the gather kernel left them
    else {                                              // the host-loop sink (long reads): its list is the one host array this route sends
        crass_candidates cd;
        if (const int gs = crass_hip_get_candidates(c, &cd)) return gs;
        HIPCHK(c, c->in.no_idx.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->in.no_idx.p, cd.read_idx, n * 8, hipMemcpyHostToDevice, c->stream));
        d_idx = c->in.no_idx.p;
    }
    const int s = names_of_device_impl(c, d_idx, n, c->read_base, d_chars, cap_bytes, d_off, total_out);
    release_names_of(c);
    return (short_off && s == CRASS_OK) ? CRASS_ERR_OVERFLOW : s;
}

uint32_t crass_hip_names_scan_tile(void) { return nm_scan_tile(); }

int crass_hip_fastx_names_drop(crass_hip_ctx *c)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    names_drop(c);
    return CRASS_OK;
}

float crass_hip_last_names_ms(const crass_hip_ctx *c, int part) { return c && part >= 0 && part < 2 ? c->in.last_names_ms[part] : 0.0f; }

// ---- header lines and quality strings of selected records from a file's raw bytes on the device (fastx_names.hip) ----
// One routine for both: the records' source words up, the measure launch, the lengths back (they size the result), their prefix
// sum on the host, the copy launch, the text back.  d_user == nullptr: the host route (the text comes back into B's pinned
// memory, *out points at it); else the caller's device buffer of cap bytes, the offsets into off_user.  Every check comes
// before the first launch; the resident set is not involved; B's device side goes back on every way out, its pinned side stays.
namespace {
struct LineOps {
    int words;                                          // source words per record: one, or two (the second n behind the first n)
    std::function<void(uint64_t k, uint64_t r, uint64_t *src)> fill;      // the words of the k-th picked record, r
    std::function<hipError_t(LineFetch &B)> measure;    // -> B.len[0, n): the lengths, B.len[n, 2 n): the second half
    std::function<hipError_t(LineFetch &B, uint64_t total, uint8_t *dst)> copy;
    std::function<void(const uint32_t *half)> second;   // the caller's use of the second half (host copy)
};
}

static int fetch_lines(crass_hip_ctx *c, LineFetch Ingest::*which, const LineOps &ops, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos,
                       uint64_t n_reads, const uint64_t *idx, uint64_t n, uint8_t *d_user, uint64_t cap, uint64_t *off_user, crass_text *out)
{
    if (!c || (n && !idx) || (n_reads && (!d_bytes || !rec_pos))) return CRASS_ERR_INVALID_ARG;
    if (n_reads >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;
    LineFetch &B = c->in.*which;
    auto run = [&]() -> int {
        for (uint64_t k = 0; k < n; k++) if (idx[k] >= n_reads || rec_pos[idx[k]] >= n_bytes) return CRASS_ERR_INVALID_ARG;
        (void)hipSetDevice(c->device);
        HIPCHK(c, B.h_off.ensure(n + 1));
        uint64_t *off = B.h_off.p;
        off[0] = 0;
        if (n) {
            const uint64_t nw = (uint64_t)ops.words * n;
            HIPCHK(c, B.h_src.ensure(nw)); HIPCHK(c, B.h_len.ensure(2 * n));
            HIPCHK(c, B.src.ensure(nw)); HIPCHK(c, B.len.ensure(2 * n));
            for (uint64_t k = 0; k < n; k++) ops.fill(k, idx[k], B.h_src.p);
            HIPCHK(c, hipMemcpyAsync(B.src.p, B.h_src.p, nw * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, ops.measure(B));
            HIPCHK(c, hipMemcpyAsync(B.h_len.p, B.len.p, 2 * n * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream)); // (the lengths size the result)
            for (uint64_t k = 0; k < n; k++) off[k + 1] = off[k] + B.h_len.p[k];
            ops.second(B.h_len.p + n);
        }
        const uint64_t total = off[n];
        if (off_user) memcpy(off_user, off, (n + 1) * 8);
        if (d_user && cap < total) return CRASS_ERR_OVERFLOW;
        if (!d_user) HIPCHK(c, B.h_chars.ensure(total));
        if (out) { out->n = n; out->chars = B.h_chars.p; out->off = off; }
        if (!total) return CRASS_OK;
        HIPCHK(c, B.off.ensure(n + 1));
        if (!d_user) HIPCHK(c, B.chars.ensure(total));
        HIPCHK(c, hipMemcpyAsync(B.off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, ops.copy(B, total, d_user ? d_user : B.chars.p));
        if (!d_user) HIPCHK(c, hipMemcpyAsync(B.h_chars.p, B.chars.p, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CRASS_OK;
    };
    const int s = run();
    release_lines(c, B);
    return s;
}

// the header line: one word per record, its first byte behind the header character; the second half is the names' lengths
static int header_lines_common(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                               const uint64_t *idx, uint64_t n, uint8_t *d_user, uint64_t cap, uint64_t *off_user, crass_text *out,
                               uint32_t *name_len_out)
{
    HlJob J{};
    J.bytes = d_bytes; J.n_bytes = n_bytes; J.n = n;
    LineOps ops;
    ops.words = 1;
    ops.fill = [&](uint64_t k, uint64_t r, uint64_t *src) { src[k] = rec_pos[r] + 1; };
    ops.measure = [&](LineFetch &B) { J.src = B.src.p; J.line_len = B.len.p; J.name_len = B.len.p + n; return launch_hl_measure(J, c->stream); };
    ops.copy = [&](LineFetch &B, uint64_t total, uint8_t *dst) { J.off = B.off.p; J.total = total; J.out = dst; return launch_hl_copy(J, c->stream); };
    ops.second = [&](const uint32_t *half) { if (name_len_out) memcpy(name_len_out, half, n * 4); };
    return fetch_lines(c, &Ingest::hl, ops, d_bytes, n_bytes, rec_pos, n_reads, idx, n, d_user, cap, off_user, out);
}

int crass_hip_fetch_header_lines_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                        const uint64_t *idx, uint64_t n, crass_text *out, uint32_t *name_len_out)
{
    if (!out) return CRASS_ERR_INVALID_ARG;
    return header_lines_common(c, d_bytes, n_bytes, rec_pos, n_reads, idx, n, nullptr, 0, nullptr, out, name_len_out);
}

int crass_hip_fetch_header_lines_device_to(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                           const uint64_t *idx, uint64_t n, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *off_out,
                                           uint32_t *name_len_out)
{
    if (!off_out || (!d_chars && cap_bytes)) return CRASS_ERR_INVALID_ARG;
    static uint8_t nowhere;                             // (a NULL buffer of capacity 0 asks for the offsets alone, as in crass_hip_fetch_text_device)
    return header_lines_common(c, d_bytes, n_bytes, rec_pos, n_reads, idx, n, d_chars ? d_chars : &nowhere, cap_bytes, off_out, nullptr, name_len_out);
}

// ---- several files into one resident set (fastx_scan.hip, inflate.hip, fastx_names.hip) ----
namespace {
struct FilesPlan {
    struct File { bool bgzf = false, gz = false; crass_bgzf_index ix{}; GzState gzs; uint64_t n_text = 0; int32_t format = 0; };
    std::vector<File> f;
    ~FilesPlan() { for (auto &x : f) if (x.bgzf) crass_bgzf_index_free(&x.ix); }
};
}

static int load_fastx_files_impl(crass_hip_ctx *c, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                                 crass_fastx_files_layout *out)
{
    // a decline found before the scan (format, compression) waits here: a file in front of it may still offend in the scan
    int32_t pend_file = -1, pend_reason = 0; uint64_t pend_pos = 0; crass_bgzf_verdict pend_v{};
    auto decline = [&](uint32_t file, int32_t reason, uint64_t pos, const crass_bgzf_verdict *v) {
        if (out) { out->decline_file = (int32_t)file; out->decline_reason = reason; out->decline_pos = pos; if (v) out->bgzf = *v; }
        return CRASS_ERR_UNSUPPORTED;
    };
    // 1. what every file is, and how much text it holds (host: first bytes, BGZF index)
    FilesPlan P;
    P.f.resize(n_files);
    uint32_t nf = n_files;
    for (uint32_t f = 0; f < nf; f++) {
        FilesPlan::File &F = P.f[f];
        const uint8_t *b = bytes[f];
        const uint64_t n = n_bytes[f];
        if (n >= 2 && b[0] == 0x1F && b[1] == 0x8B) {
            const int s = crass_bgzf_index_host(b, n, &F.ix);
            if (s == CRASS_ERR_UNSUPPORTED && c->in.gzip_on_device) {
                // plain gzip (crass_hip_set_gzip_on_device; of any number of members with CRASS_GZIP_ON_DEVICE_MEMBERS): its bytes go up once for the count step, which sizes its share of the arena
                HIPCHK(c, c->in.z_raw.ensure(n + 16));
                const int up = upload_staged(c, b, n, c->in.z_raw.p);
                if (up) return up;
                HIPCHK(c, hipStreamSynchronize(c->copy_stream));
                crass_bgzf_verdict v{};
                const int gs = gzip_count_impl(c, c->in.z_raw.p, n, 0, F.gzs, nullptr, &v, c->in.gzip_on_device == CRASS_GZIP_ON_DEVICE_MEMBERS);
                if (gs == CRASS_ERR_UNSUPPORTED) { pend_file = (int32_t)f; pend_v = v; nf = f; break; }
                if (gs) return gs;
                F.gz = true; F.n_text = F.gzs.n_text;
                if (F.n_text == 0) { pend_file = (int32_t)f; pend_reason = FX_EMPTY; nf = f; break; }
                continue;
            }
            if (s == CRASS_ERR_UNSUPPORTED) { pend_file = (int32_t)f; pend_v = F.ix.decline; nf = f; break; }
            if (s) return s;
            F.bgzf = true; F.n_text = F.ix.out_off[F.ix.n_members];
            if (F.n_text == 0) { pend_file = (int32_t)f; pend_reason = FX_EMPTY; nf = f; break; }
        } else {
            if (n == 0) { pend_file = (int32_t)f; pend_reason = FX_EMPTY; nf = f; break; }
            if (!fx_is_hdr_char(b[0])) { pend_file = (int32_t)f; pend_reason = FX_FIRST_BYTE; nf = f; break; }
            F.n_text = n; F.format = b[0];
        }
    }
    auto pending = [&]() { return decline((uint32_t)pend_file, pend_reason, pend_pos, pend_v.reason ? &pend_v : nullptr); };
    if (nf == 0) return pending();
    // 2. the arena; every file's bytes up, a BGZF file inflated into its place; the first two scan kernels of file f are queued
    //    before file f + 1 is staged
    std::vector<uint64_t> base(nf + 1, 0), tile0(nf + 1, 0);
    for (uint32_t f = 0; f < nf; f++) base[f + 1] = base[f] + P.f[f].n_text + 1;
    HIPCHK(c, c->in.fa_arena.ensure(base[nf] + 16));
    uint8_t *arena = c->in.fa_arena.p;
    for (uint32_t f = 0; f < nf; f++) {
        tile0[f + 1] = tile0[f] + fastx_n_tiles(arena + base[f], P.f[f].n_text);
    }
    if (tile0[nf] > 0x7FFFFFFFull) return CRASS_ERR_UNSUPPORTED;
    HIPCHK(c, c->in.x_tiles.ensure(tile0[nf])); HIPCHK(c, c->in.x_base.ensure(tile0[nf]));
    HIPCHK(c, c->in.x_tot.ensure(5 * (uint64_t)nf)); HIPCHK(c, c->in.x_h_tot.ensure(5 * (uint64_t)nf));      // [4 f ..): the totals; [4 nf + f]: the verdict
    std::vector<FxJob> jobs(nf);
    HIPCHK(c, c->in.tm_scan.begin(c->timing_level >= 1, c->stream));
    for (uint32_t f = 0; f < nf; f++) {
        FilesPlan::File &F = P.f[f];
        if (f) HIPCHK(c, hipStreamSynchronize(c->copy_stream));      // (the staged buffers are the file before's until its last copy is done)
        if (F.bgzf || F.gz) {
            HIPCHK(c, c->in.z_raw.ensure(n_bytes[f] + 16));
            const int up = upload_staged(c, bytes[f], n_bytes[f], c->in.z_raw.p);
            if (up) return up;
            crass_bgzf_verdict v{};
            // (both wait for the stream: z_raw may be used again)
            const int s = F.gz ? gzip_decode_impl(c, c->in.z_raw.p, F.gzs, arena + base[f], &v) : inflate_bgzf_impl(c, c->in.z_raw.p, &F.ix, arena + base[f], &v);
            if (s == CRASS_ERR_UNSUPPORTED) { pend_file = (int32_t)f; pend_reason = 0; pend_v = v; nf = f; break; }
            if (s) return s;
            HIPCHK(c, hipMemcpy(&F.format, arena + base[f], 1, hipMemcpyDeviceToHost));
            F.format &= 0xFF;
            if (!fx_is_hdr_char((uint8_t)F.format)) { pend_file = (int32_t)f; pend_reason = FX_FIRST_BYTE; pend_v = crass_bgzf_verdict{}; nf = f; break; }
        } else {
            const int up = upload_staged(c, bytes[f], n_bytes[f], arena + base[f]);
            if (up) return up;
        }
        const int qs = scan_queue(c, jobs[f], f, arena + base[f], F.n_text, F.format, tile0[f], tile0[f + 1] - tile0[f]);
        if (qs) return qs;
    }
    if (nf == 0) return pending();
    for (uint32_t f = 0; f < nf; f++) HIPCHK(c, hipMemsetAsync(arena + base[f + 1] - 1, 0x0A, 1, c->stream));      // the '\n' behind every file
    // 3. every file emits into one text and one pair of per-record arrays; 4. the verdict: the first file in order that offends
    //    (the verdict words lie behind the totals of every file planned in step 2)
    ScanResult R;
    const int es = scan_emit(c, jobs.data(), nf, (uint32_t)jobs.size(), base.data(), 0xFFFFFFFFull, R);
    if (es == CRASS_ERR_UNSUPPORTED && R.decline_file >= 0) return decline((uint32_t)R.decline_file, R.decline_reason, R.decline_pos, nullptr);
    if (es) return es;
    const std::vector<uint64_t> &rbase = R.rbase;
    const uint64_t nr = R.n_reads, max_len = R.max_len;
    uint64_t *rec_pos = c->in.x_h_rec_pos.p, *seq_off = c->in.x_h_seq_off.p;
    if (pend_file >= 0) return pending();
    // 5. one pack launch over the joined text, then the header ids on the arena, installed from where they are
    const int s = load_text_impl(c, nullptr, c->in.x_text.p, seq_off, nr, pad_uniform, nullptr, 0);
    if (s) return s;
    uint64_t n_rep = 0;
    const int hs = header_ids_device_impl(c, arena, base[nf], rec_pos, nr, nullptr, 1, &n_rep);
    if (hs) { c->have_reads = false; return hs; }
    if (n_rep == 0) c->R.header_id = nullptr;           // (all names unique: as a load without header ids)
    HIPCHK(c, c->in.fa_h_base.ensure(2 * ((uint64_t)nf + 1))); HIPCHK(c, c->in.fa_h_format.ensure(nf));
    for (uint32_t f = 0; f <= nf; f++) { c->in.fa_h_base.p[f] = rbase[f]; c->in.fa_h_base.p[nf + 1 + f] = base[f]; }
    for (uint32_t f = 0; f < nf; f++) c->in.fa_h_format.p[f] = P.f[f].format;
    c->in.fa_bytes = base[nf]; c->in.have_arena = true;
    if (out) {
        out->n_reads = nr; out->max_len = (uint32_t)max_len; out->rec_pos = rec_pos; out->seq_off = seq_off;
        out->file_read_base = c->in.fa_h_base.p; out->file_byte_base = c->in.fa_h_base.p + nf + 1; out->format = c->in.fa_h_format.p;
    }
    return CRASS_OK;
}

int crass_hip_load_fastx_files(crass_hip_ctx *c, const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, int pad_uniform,
                               crass_fastx_files_layout *out)
{
    if (out) { memset(out, 0, sizeof(*out)); out->decline_file = -1; out->n_files = n_files; }
    if (!c || !n_files || !bytes || !n_bytes || pad_uniform < 0 || pad_uniform > 2) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (n_bytes[f] && !bytes[f]) return CRASS_ERR_INVALID_ARG;
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    const int s = load_fastx_files_impl(c, bytes, n_bytes, n_files, pad_uniform, out);
    // the scratch goes back on every way out, as in load_fastx_common; the arena stays only with an accepted set
    release_gzip(c); release_bgzf(c); release_scan(c); release_text(c); release_header_ids(c);
    if (s) { c->have_reads = false; drop_arena(c); }
    return s;
}

int crass_hip_resident_fastx(const crass_hip_ctx *c, const uint8_t **d_bytes, uint64_t *n_bytes)
{
    if (!c || !d_bytes || !n_bytes) return CRASS_ERR_INVALID_ARG;
    *d_bytes = nullptr; *n_bytes = 0;
    if (!c->in.have_arena || !c->have_reads) return CRASS_ERR_STATE;
    *d_bytes = c->in.fa_arena.p; *n_bytes = c->in.fa_bytes;
    return CRASS_OK;
}

// the quality string: two words per record, its position and its end; the starts of the quality lines stay on the device; the
// second half is the flags, bit 0: the record has a quality line
static int quality_common(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                          const uint64_t *idx, uint64_t n, uint8_t *d_user, uint64_t cap, uint64_t *off_user, crass_text *out, uint8_t *has_qual_out)
{
    QlJob J{};
    J.bytes = d_bytes; J.n_bytes = n_bytes; J.n = n;
    LineOps ops;
    ops.words = 2;
    ops.fill = [&](uint64_t k, uint64_t r, uint64_t *src) { src[k] = rec_pos[r]; src[n + k] = std::min(rec_pos[r + 1], n_bytes); };
    ops.measure = [&](LineFetch &B) {
        const hipError_t e = B.start.ensure(n);
        if (e != hipSuccess) return e;
        J.src = B.src.p; J.lim = B.src.p + n; J.start = B.start.p; J.len = B.len.p; J.flags = B.len.p + n;
        return launch_ql_measure(J, c->stream);
    };
    ops.copy = [&](LineFetch &B, uint64_t total, uint8_t *dst) { J.off = B.off.p; J.total = total; J.out = dst; return launch_ql_copy(J, c->stream); };
    ops.second = [&](const uint32_t *half) { if (has_qual_out) for (uint64_t k = 0; k < n; k++) has_qual_out[k] = (uint8_t)(half[k] & 1u); };
    return fetch_lines(c, &Ingest::ql, ops, d_bytes, n_bytes, rec_pos, n_reads, idx, n, d_user, cap, off_user, out);
}

int crass_hip_fetch_quality_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                   const uint64_t *idx, uint64_t n, crass_text *out, uint8_t *has_qual_out)
{
    if (!out) return CRASS_ERR_INVALID_ARG;
    return quality_common(c, d_bytes, n_bytes, rec_pos, n_reads, idx, n, nullptr, 0, nullptr, out, has_qual_out);
}

int crass_hip_fetch_quality_device_to(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                      const uint64_t *idx, uint64_t n, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *off_out, uint8_t *has_qual_out)
{
    if (!off_out || (!d_chars && cap_bytes)) return CRASS_ERR_INVALID_ARG;
    static uint8_t nowhere;                             // (a NULL buffer of capacity 0 asks for the offsets alone, as in crass_hip_fetch_text_device)
    return quality_common(c, d_bytes, n_bytes, rec_pos, n_reads, idx, n, d_chars ? d_chars : &nowhere, cap_bytes, off_out, nullptr, has_qual_out);
}

int crass_hip_get_packed(const crass_hip_ctx *c, crass_packed *out)
{
    if (!c || !out) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (!c->have_reads) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    const DevReads &R = c->R;
    const uint64_t n = R.n_reads, ne = R.n_exc;
    auto get = [&](void *dst, const void *src, uint64_t bytes) {
        if (!bytes) return CRASS_OK;
        const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { c->last_hip = (int)e; return CRASS_ERR_HIP; }
        return CRASS_OK;
    };
    // the word count: n strides, or the last read's first word and its own words
    uint64_t total_words = n * (uint64_t)R.stride_words;
    if (!R.stride_words && n) {
        uint64_t w_last = 0; uint32_t l_last = R.uniform_len;
        int s = get(&w_last, R.word_off + (n - 1), 8);
        if (!s && !R.uniform_len) s = get(&l_last, R.lengths + (n - 1), 4);
        if (s) return s;
        total_words = w_last + (l_last + 15) / 16;
    }
    uint64_t exc_total = 0;
    if (ne) { const int s = get(&exc_total, R.exc_off + ne, 8); if (s) return s; }
    crass_packed pk;
    PackedArrays a{};
    int s = packed_alloc(total_words + 4, R.stride_words ? 0 : n + 1, R.uniform_len ? 0 : n, ne, ne + 1, exc_total, R.header_id ? n : 0, &pk, &a);
    if (s) return s;
    s = get(a.packed, R.packed, total_words * 4);
    if (!s) memset(a.packed + total_words, 0, 16);
    if (!s && a.word_off) { s = get(a.word_off, R.word_off, n * 8); a.word_off[n] = total_words; }
    if (!s && a.lengths) s = get(a.lengths, R.lengths, n * 4);
    if (!s && ne) s = get(a.exc_read, R.exc_read, ne * 8);
    if (!s && ne) s = get(a.exc_off, R.exc_off, (ne + 1) * 8);
    if (!ne) a.exc_off[0] = 0;
    if (!s && exc_total) s = get(a.exc_bytes, R.exc_bytes, exc_total);
    if (!s && a.header_id) s = get(a.header_id, R.header_id, n * 8);
    if (s) { crass_free_packed(&pk); return s; }
    crass_reads &r = pk.reads;
    r.n_reads = n; r.packed = a.packed; r.stride_words = R.stride_words; r.word_off = a.word_off; r.uniform_len = R.uniform_len; r.lengths = a.lengths;
    r.n_exceptions = ne; r.exc_read = a.exc_read; r.exc_off = a.exc_off; r.exc_bytes = a.exc_bytes; r.header_id = a.header_id;
    r.read_index_base = c->read_base;
    *out = pk;
    return CRASS_OK;
}

// ---- text of selected reads out of the resident set (k_fetch_text, pack.hip) ----
// d_user == nullptr: the host route (the text comes back into pinned memory, *out points at it); else the caller's device
// buffer of cap bytes, the offsets into off_user.  Every check comes before the first launch; the resident set is only read.
static int fetch_text_impl(crass_hip_ctx *c, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, uint8_t *d_user, uint64_t cap,
                           uint64_t *off_user, crass_text *out)
{
    if (n && !read_idx) return CRASS_ERR_INVALID_ARG;
    if (!c->have_reads) return CRASS_ERR_STATE;
    const DevReads &R = c->R;
    for (uint64_t k = 0; k < n; k++) if (read_idx[k] < c->read_base || read_idx[k] - c->read_base >= R.n_reads) return CRASS_ERR_INVALID_ARG;
    if (!R.uniform_len && c->h_lengths.size() != R.n_reads) return CRASS_ERR_STATE;      // (never expected: every load keeps them)
    c->in.last_fetch_ms = 0;
    (void)hipSetDevice(c->device);
    HIPCHK(c, c->in.f_h_off.ensure(n + 1));
    uint64_t *off = c->in.f_h_off.p;
    off[0] = 0;
    if (n) {
        HIPCHK(c, c->in.f_h_idx.ensure(n));
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t r = read_idx[k] - c->read_base;
            c->in.f_h_idx.p[k] = r;
            off[k + 1] = off[k] + (R.uniform_len ? R.uniform_len : c->h_lengths[r]);
        }
    }
    const uint64_t total = off[n];
    if (off_user) memcpy(off_user, off, (n + 1) * 8);
    if (d_user && cap < total) return CRASS_ERR_OVERFLOW;
    if (!d_user) HIPCHK(c, c->in.f_h_chars.ensure(total));
    if (out) { out->n = n; out->chars = c->in.f_h_chars.p; out->off = off; }
    if (!total) return CRASS_OK;                        // (no record, or empty reads only: nothing to launch or wait for)
    HIPCHK(c, c->in.f_idx.ensure(n));
    HIPCHK(c, c->in.f_off.ensure(n + 1));
    HIPCHK(c, hipMemcpyAsync(c->in.f_idx.p, c->in.f_h_idx.p, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in.f_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (revcomp) {
        HIPCHK(c, c->in.f_h_rc.ensure(n));
        HIPCHK(c, c->in.f_rc.ensure(n));
        memcpy(c->in.f_h_rc.p, revcomp, n);
        HIPCHK(c, hipMemcpyAsync(c->in.f_rc.p, c->in.f_h_rc.p, n, hipMemcpyHostToDevice, c->stream));
    }
    if (!d_user) HIPCHK(c, c->in.f_chars.ensure(total));
    FetchJob J{};
    J.R = R; J.idx = c->in.f_idx.p; J.rc = revcomp ? c->in.f_rc.p : nullptr; J.out_off = c->in.f_off.p; J.n = n; J.total = total;
    J.out = d_user ? d_user : c->in.f_chars.p;
    HIPCHK(c, c->in.tm_fetch.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_fetch_text(J, c->stream));
    HIPCHK(c, c->in.tm_fetch.mark(c->stream));
    if (!d_user) HIPCHK(c, hipMemcpyAsync(c->in.f_h_chars.p, c->in.f_chars.p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the call's one wait (device route: the staged indices are free again, the text is written)
    HIPCHK(c, c->in.tm_fetch.elapsed(0, 1, &c->in.last_fetch_ms));
    return CRASS_OK;
}

int crass_hip_fetch_text(crass_hip_ctx *c, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, crass_text *out)
{
    if (!c || !out) return CRASS_ERR_INVALID_ARG;
    return fetch_text_impl(c, read_idx, revcomp, n, nullptr, 0, nullptr, out);
}

int crass_hip_fetch_text_device(crass_hip_ctx *c, const uint64_t *read_idx, const uint8_t *revcomp, uint64_t n, uint8_t *d_chars,
                                uint64_t cap_bytes, uint64_t *off_out)
{
    if (!c || !off_out || (!d_chars && cap_bytes)) return CRASS_ERR_INVALID_ARG;
    static uint8_t nowhere;                             // (a NULL buffer of capacity 0 asks for the offsets alone: the device route, which then overflows or writes nothing)
    return fetch_text_impl(c, read_idx, revcomp, n, d_chars ? d_chars : &nowhere, cap_bytes, off_out, nullptr);
}

int crass_hip_fetch_record_text(crass_hip_ctx *c, int pass, crass_text *out)
{
    if (!c || !out || (pass != 1 && pass != 2)) return CRASS_ERR_INVALID_ARG;
    const uint64_t *idx = nullptr; const uint8_t *low = nullptr; uint64_t n = 0;
    if (pass == 1) {
        crass_candidates v;
        if (const int s = crass_hip_get_candidates(c, &v)) return s;
        idx = v.read_idx; low = v.low_lexi; n = v.n;
    } else {
        crass_recruits v;
        if (const int s = crass_hip_get_recruits(c, &v)) return s;
        idx = v.read_idx; low = v.low_lexi; n = v.n;
    }
    // RH_Seq = low_lexi ? seq : revcomp(seq): the adapter's fill_holder, ReadHolder.cpp:513-591
    c->in.f_flags.resize(n);
    for (uint64_t k = 0; k < n; k++) c->in.f_flags[k] = low[k] ? 0 : 1;
    return fetch_text_impl(c, idx, c->in.f_flags.data(), n, nullptr, 0, nullptr, out);
}

float crass_hip_last_fetch_ms(const crass_hip_ctx *c) { return c ? c->in.last_fetch_ms : 0.0f; }

} // extern "C"

// ---- one rank's shard of a group's files load (fastx_shards.h; the group's threads and barriers are group.cpp's) ----
// the probe of a range that lies on the device: launch, the blocks' parts back, folded in block order
static int probe_impl(crass_hip_ctx *c, const uint8_t *d, uint64_t n, bool left_is_ls, FxProbe *out)
{
    Ingest &I = c->in;
    FxProbe none{};
    none.gt = kFxNone;
    for (auto &x : none.ls) x = kFxNone;
    *out = none;
    I.last_probe_ms = 0;
    if (!n) return CRASS_OK;
    FxProbeJob P;
    fx_probe_plan(d, n, left_is_ls ? 1u : 0u, &P);
    HIPCHK(c, I.sh_part.ensure(P.n_blocks)); HIPCHK(c, I.sh_h_part.ensure(P.n_blocks));
    P.part = I.sh_part.p;
    HIPCHK(c, I.tm_probe.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_fx_cut_probe(P, c->stream));
    HIPCHK(c, I.tm_probe.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(I.sh_h_part.p, I.sh_part.p, P.n_blocks * sizeof(FxProbe), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_probe.elapsed(0, 1, &I.last_probe_ms));
    fx_probe_fold(I.sh_h_part.p, P.n_blocks, out);
    return CRASS_OK;
}

extern "C" int crass_hip_fastx_cut_probe_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, int left_is_ls, uint64_t out[7])
{
    if (!c || !out || (n_bytes && !d_bytes)) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    FxProbe P;
    const int s = probe_impl(c, d_bytes, n_bytes, left_is_ls != 0, &P);
    wait_main(c); c->in.sh_part.release();
    if (s) return s;
    out[0] = P.n_nl; out[1] = P.n_ls; for (int k = 0; k < 4; k++) out[2 + k] = P.ls[k]; out[6] = P.gt;
    return CRASS_OK;
}

extern "C" float crass_hip_last_cut_probe_ms(const crass_hip_ctx *c) { return c ? c->in.last_probe_ms : 0.0f; }

// The members of a BGZF index that hold the text range [a, b): [*m0, *m1).  Members without text are taken where they lie at
// b, and from member 0 when a is 0 (in front of a > 0 they are the range before's), so that a file cut into ranges that tile
// its text has every member inflated by somebody, the 28-byte end-of-file member included.
static void bgzf_members_for(const crass_bgzf_index *ix, uint64_t a, uint64_t b, uint64_t *m0, uint64_t *m1)
{
    const uint64_t n = ix->n_members, *oo = ix->out_off;
    *m0 = a == 0 ? 0 : (uint64_t)(std::upper_bound(oo + 1, oo + n + 1, a) - (oo + 1));      // the first member that ends behind a
    uint64_t e = (uint64_t)(std::upper_bound(oo + 1, oo + n + 1, b) - (oo + 1));            // ... behind b
    if (e < n && oo[e] < b) e++;
    *m1 = e;
}

// the members [m0, m1) of a host file inflated so that text position t lies at text0 + t: the compressed bytes up into z_raw
static int shard_inflate(crass_hip_ctx *c, const ShardFile &F, uint64_t m0, uint64_t m1, uint8_t *text0, crass_bgzf_verdict *bv)
{
    const uint64_t z0 = F.ix->in_off[m0], z1 = F.ix->in_off[m1];
    HIPCHK(c, c->in.z_raw.ensure(z1 - z0 + 16));
    const int up = upload_staged(c, F.bytes + z0, z1 - z0, c->in.z_raw.p);
    if (up) return up;
    // (waits for the stream before it returns: z_raw may be used again)
    return inflate_bgzf_members(c, reinterpret_cast<const uint8_t *>((uintptr_t)c->in.z_raw.p - z0), F.ix, m0, m1 - m0, text0, bv);
}

int shard_stage_probe(crass_hip_ctx *c, const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi, std::vector<ShardPiece> *pieces,
                      ShardVerdict *v)
{
    if (!c || !files || !pieces || !v) return CRASS_ERR_INVALID_ARG;
    pieces->clear();
    *v = ShardVerdict();
    begin_fastx_load(c);
    c->in.last_inflate_ms = 0;
    release_shard(c);
    Ingest &I = c->in;
    try {
        // the pieces and their places in the staging buffer: every piece at its text position modulo 16
        struct Plan { uint32_t f; uint64_t a, b, sa, sb, off, m0, m1; };
        std::vector<Plan> plan;
        uint64_t cursor = 0;
        for (uint32_t f = lo.file; f <= hi.file && f < n_files; f++) {
            const uint64_t a = f == lo.file ? lo.pos : 0, b = f == hi.file ? hi.pos : files[f].n_text;
            if (a >= b) continue;
            Plan p{f, a, b, a, b, 0, 0, 0};
            if (files[f].ix) {                          // (with the byte in front of a: it says whether a is a line start)
                bgzf_members_for(files[f].ix, a ? a - 1 : 0, b, &p.m0, &p.m1);
                p.sa = files[f].ix->out_off[p.m0]; p.sb = files[f].ix->out_off[p.m1];
            }
            p.off = ((cursor + 15) & ~15ull) + (p.sa & 15u);
            cursor = p.off + (p.sb - p.sa);
            plan.push_back(p);
        }
        HIPCHK(c, I.sh_stage.ensure(cursor + 32));
        bool first = true;
        for (const Plan &p : plan) {
            const ShardFile &F = files[p.f];
            uint8_t *dst = I.sh_stage.p + p.off;        // text position p.sa
            if (!first) HIPCHK(c, hipStreamSynchronize(c->copy_stream));      // (the staged buffers are the piece before's until its last copy is done)
            first = false;
            ShardPiece pc{};
            pc.file = p.f; pc.a = p.a; pc.b = p.b;
            if (F.ix) {
                crass_bgzf_verdict bv{};
                const int s = shard_inflate(c, F, p.m0, p.m1, reinterpret_cast<uint8_t *>((uintptr_t)dst - p.sa), &bv);
                if (s == CRASS_ERR_UNSUPPORTED) { v->file = (int32_t)p.f; v->bgzf = bv; break; }
                if (s) return s;
                uint8_t one = 0;
                HIPCHK(c, hipMemcpy(&one, dst + ((p.a ? p.a - 1 : 0) - p.sa), 1, hipMemcpyDeviceToHost));
                if (p.a == 0) {
                    pc.first_byte = one;
                    if (!fx_is_hdr_char(one)) { v->file = (int32_t)p.f; v->reason = FX_FIRST_BYTE; break; }
                }
                pc.left_is_ls = p.a == 0 || fx_is_nl(one);
            } else {
                const int up = upload_staged(c, F.bytes + p.a, p.b - p.a, dst);
                if (up) return up;
                pc.left_is_ls = p.a == 0 || fx_is_nl(F.bytes[p.a - 1]);
                if (p.a == 0) pc.first_byte = F.bytes[0];
            }
            const int ps = probe_impl(c, dst + (p.a - p.sa), p.b - p.a, pc.left_is_ls, &pc.probe);
            if (ps) return ps;
            I.sh_staged.push_back(Ingest::ShardStaged{p.f, p.sa, p.sb, p.off});
            pieces->push_back(pc);
        }
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

int shard_scan(crass_hip_ctx *c, const ShardFile *files, uint32_t n_files, ShardPos lo, ShardPos hi,
               std::vector<std::pair<uint32_t, uint64_t>> *file_reads, uint64_t *n_reads, uint32_t *max_len, ShardVerdict *v)
{
    if (!c || !files || !file_reads || !n_reads || !max_len || !v) return CRASS_ERR_INVALID_ARG;
    *n_reads = 0; *max_len = 0; *v = ShardVerdict();
    file_reads->clear();
    Ingest &I = c->in;
    (void)hipSetDevice(c->device);
    try {
        struct Slice { uint32_t f; uint64_t a, b; };
        std::vector<Slice> sl;
        for (uint32_t f = lo.file; f <= hi.file && f < n_files; f++) {
            const uint64_t a = f == lo.file ? lo.pos : 0, b = f == hi.file ? hi.pos : files[f].n_text;
            if (a < b) sl.push_back(Slice{f, a, b});
        }
        // the arena: the slices in order, a byte of room behind each
        std::vector<uint64_t> &base = I.sh_base;
        base.assign(1, 0);
        for (const Slice &S : sl) base.push_back(base.back() + (S.b - S.a) + 1);
        HIPCHK(c, I.fa_arena.ensure(base.back() + 16));
        uint8_t *arena = I.fa_arena.p;
        uint32_t ns = (uint32_t)sl.size();
        for (uint32_t i = 0; i < ns; i++) {
            const Slice &S = sl[i];
            const ShardFile &F = files[S.f];
            uint8_t *dst = arena + base[i];
            // what was staged of it comes device to device ...
            uint64_t have = S.a;                        // [S.a, have) is in place
            for (const Ingest::ShardStaged &st : I.sh_staged) {
                if (st.file != S.f || S.a < st.a || S.a >= st.b) continue;
                have = std::min(S.b, st.b);
                HIPCHK(c, hipMemcpyAsync(dst, I.sh_stage.p + st.off + (S.a - st.a), have - S.a, hipMemcpyDeviceToDevice, c->stream));
            }
            if (have == S.b) continue;
            // ... and the tail behind it from the host: plain bytes, or the further members
            HIPCHK(c, hipStreamSynchronize(c->copy_stream));
            if (F.ix) {
                uint64_t m0, m1;
                bgzf_members_for(F.ix, have, S.b, &m0, &m1);
                const uint64_t t0 = F.ix->out_off[m0], t1 = F.ix->out_off[m1];
                HIPCHK(c, I.sh_tail.ensure(t1 - t0 + 16));
                crass_bgzf_verdict bv{};
                const int s = shard_inflate(c, F, m0, m1, reinterpret_cast<uint8_t *>((uintptr_t)I.sh_tail.p - t0), &bv);
                if (s == CRASS_ERR_UNSUPPORTED) { v->file = (int32_t)S.f; v->bgzf = bv; ns = i; break; }      // (the slices in front of it are still scanned)
                if (s) return s;
                HIPCHK(c, hipMemcpyAsync(dst + (have - S.a), I.sh_tail.p + (have - t0), S.b - have, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));      // (sh_tail may be used again)
            } else {
                const int up = upload_staged(c, F.bytes + have, S.b - have, dst + (have - S.a));
                if (up) return up;
            }
        }
        base.resize((size_t)ns + 1);
        I.sh_n_reads = 0;
        if (ns == 0) { I.sh_scanned = v->file < 0; return CRASS_OK; }
        std::vector<uint64_t> tile0(ns + 1, 0);
        for (uint32_t i = 0; i < ns; i++) tile0[i + 1] = tile0[i] + fastx_n_tiles(arena + base[i], sl[i].b - sl[i].a);
        if (tile0[ns] > 0x7FFFFFFFull) return CRASS_ERR_UNSUPPORTED;
        HIPCHK(c, I.x_tiles.ensure(tile0[ns])); HIPCHK(c, I.x_base.ensure(tile0[ns]));
        HIPCHK(c, I.x_tot.ensure(5 * (uint64_t)ns)); HIPCHK(c, I.x_h_tot.ensure(5 * (uint64_t)ns));
        std::vector<FxJob> jobs(ns);
        HIPCHK(c, I.tm_scan.begin(c->timing_level >= 1, c->stream));
        for (uint32_t i = 0; i < ns; i++) {
            // a slice is scanned as a file of its file's format: it begins at a record start, so its lines count from 0
            const int qs = scan_queue(c, jobs[i], i, arena + base[i], sl[i].b - sl[i].a, files[sl[i].f].format, tile0[i], tile0[i + 1] - tile0[i]);
            if (qs) return qs;
            HIPCHK(c, hipMemsetAsync(arena + base[i + 1] - 1, 0x0A, 1, c->stream));
        }
        ScanResult R;
        const int es = scan_emit(c, jobs.data(), ns, ns, base.data(), 0xFFFFFFFFull, R);
        if (es == CRASS_ERR_UNSUPPORTED && R.decline_file >= 0) {      // (in the FILE's positions)
            ShardVerdict sv;
            sv.file = (int32_t)sl[R.decline_file].f; sv.reason = R.decline_reason; sv.pos = R.decline_pos + sl[R.decline_file].a;
            if (shard_verdict_before(sv, *v)) *v = sv;
            return CRASS_OK;
        }
        if (es) return es;
        if (v->file >= 0) return CRASS_OK;
        for (uint32_t i = 0; i < ns; i++) file_reads->push_back(std::make_pair(sl[i].f, R.rbase[i + 1] - R.rbase[i]));
        *n_reads = R.n_reads; *max_len = (uint32_t)R.max_len;
        I.sh_n_reads = R.n_reads; I.sh_scanned = true;
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
    return CRASS_OK;
}

static void shard_release_all(crass_hip_ctx *c)
{
    release_gzip(c); release_bgzf(c); release_scan(c); release_text(c); release_header_ids(c); release_shard(c);
}

int shard_pack(crass_hip_ctx *c, int pad_uniform, uint64_t read_index_base)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    if (!I.sh_scanned) return CRASS_ERR_STATE;
    (void)hipSetDevice(c->device);
    auto run = [&]() -> int {
        const uint64_t nr = I.sh_n_reads, n_arena = I.sh_base.empty() ? 0 : I.sh_base.back();
        HIPCHK(c, I.x_h_seq_off.ensure(1)); HIPCHK(c, I.x_h_rec_pos.ensure(1)); HIPCHK(c, I.fa_arena.ensure(16));
        if (!nr) { I.x_h_seq_off.p[0] = 0; I.x_h_rec_pos.p[0] = 0; }      // (an empty shard: no slice was scanned)
        const int s = load_text_impl(c, nullptr, I.x_text.p, I.x_h_seq_off.p, nr, pad_uniform, nullptr, read_index_base);
        if (s) return s;
        if (nr) {
            uint64_t n_rep = 0;
            const int hs = header_ids_device_impl(c, I.fa_arena.p, n_arena, I.x_h_rec_pos.p, nr, nullptr, 1, &n_rep);
            if (hs) return hs;
            if (n_rep == 0) c->R.header_id = nullptr;   // (all names of the shard unique: as a load without header ids)
        }
        I.fa_bytes = n_arena; I.have_arena = true;
        return crass_hip_fastx_names_build_device(c, nullptr, 0, nullptr, 0);
    };
    const int s = run();
    shard_release_all(c);
    if (s) { c->have_reads = false; drop_arena(c); }
    else I.sh_loaded = true;
    return s;
}

void shard_abort(crass_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    shard_release_all(c);
    c->have_reads = false;
    drop_arena(c);
}

int shard_records(const crass_hip_ctx *c, const uint8_t **arena, uint64_t *n_bytes, const uint64_t **rec_pos, uint64_t *n_reads)
{
    if (!c || !arena || !n_bytes || !rec_pos || !n_reads) return CRASS_ERR_INVALID_ARG;
    if (!c->in.sh_loaded || !c->in.have_arena || !c->have_reads) return CRASS_ERR_STATE;
    *arena = c->in.fa_arena.p; *n_bytes = c->in.fa_bytes; *rec_pos = c->in.x_h_rec_pos.p; *n_reads = c->R.n_reads;
    return CRASS_OK;
}
uint64_t names_find_device_found(const crass_hip_ctx *c) { return c ? c->in.last_find_found : 0; }

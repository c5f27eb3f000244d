// engine_ingest.cpp — the device ingest behind include/crass_hip.h, its first file: the scratch of every ingest stage given back
// (one release_* per stage) and what opens a load; packed reads and sequence text in (pack.hip); the text of resident reads
// back out (k_fetch_text).  The FASTA / FASTQ scan and its loaders are engine_fastx.cpp, BGZF and gzip inflate
// engine_inflate.cpp, header ids, names, header lines and quality engine_names.cpp, one rank's steps of a group's files load
// engine_shards.cpp; what crosses them is ingest_internal.h.  The context and its Ingest member are engine_ctx.h; what a load
// ends with (finish_load: scratch, position hints, first-call bounds) is engine.cpp's.
#include "ingest_internal.h"

extern "C" {

// the file arena of crass_hip_load_fastx_files goes with the read set it belongs to: every public load and attach calls this
// (load_text_impl, the pack step those calls share with crass_hip_load_fastx_files itself, does not)
void names_drop(crass_hip_ctx *c)
{
    if (c->in.nt_table.p || c->in.nt_rec_pos.p) { (void)hipStreamSynchronize(c->stream); c->in.nt_table.release(); c->in.nt_rec_pos.release(); }
    c->in.have_names = false; c->in.nt_on_arena = false; c->in.nt_bytes = nullptr; c->in.nt_n_bytes = c->in.nt_n_reads = c->in.nt_mask = 0;
}

// the comment structure goes with every load and attach, whatever it was built on (crass_hip_fastx_comments_build_device)
void comments_drop(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    if (I.ct_bits.p || I.ct_carry.p || I.ct_frb.p) { (void)hipStreamSynchronize(c->stream); I.ct_bits.release(); I.ct_carry.release(); I.ct_frb.release(); }
    I.have_comments = false; I.ct_on_arena = false; I.ct_bytes = nullptr; I.ct_n_bytes = I.ct_n_reads = 0; I.ct_n_files = 0;
    I.ct_counts[0] = I.ct_counts[1] = 0;
    std::vector<uint64_t>().swap(I.ct_h_rec_pos);
}

void drop_arena(crass_hip_ctx *c)
{
    comments_drop(c);
    if (c->in.have_names && c->in.nt_on_arena) names_drop(c);      // (a name table built on the arena refers to its bytes)
    if (c->in.fa_arena.p) { (void)hipStreamSynchronize(c->stream); c->in.fa_arena.release(); }
    c->in.have_arena = false; c->in.fa_bytes = 0; c->in.sh_loaded = false;
}

// ---- the scratch goes back: one function per stage, which first waits for the streams that may still use the stage's buffers ----
void wait_main(crass_hip_ctx *c) { (void)hipStreamSynchronize(c->stream); }
static void wait_both(crass_hip_ctx *c) { wait_main(c); (void)hipStreamSynchronize(c->copy_stream); }
// crass_hip_load_text's own part: the text's offsets (8 bytes per read) and the two staged chunks, upload_staged's too (pinned and
// device memory of up to CRASS_TEXT_CHUNK_BYTES each) — a context loads a read set once
void release_text(crass_hip_ctx *c)
{
    wait_both(c);
    c->in.t_off.release();
    for (int k = 0; k < 2; k++) { c->in.t_dev[k].release(); c->in.t_pin[k].release(); }
}

// the scan: the raw copy, the reads' text, the tile and per-record arrays
void release_scan(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_both(c);
    I.x_raw.release(); I.x_text.release(); I.x_tiles.release(); I.x_base.release(); I.x_tot.release(); I.x_rec_pos.release(); I.x_seq_off.release();
    for (auto &w : I.w_scratch) w.release();
    I.w_scratch.clear();
}

// the BGZF inflate, and the verdict word the gzip decode step shares with it
void release_bgzf(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_both(c);
    I.z_idx.release(); I.z_reason.release(); I.z_verdict.release(); I.z_raw.release(); I.z_text.release();
}

void release_gzip(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.gz_a64.release(); I.gz_b64.release(); I.gz_a32.release(); I.gz_b32.release(); I.gz_sym.release(); I.gz_win.release(); I.gz_ends.release(); I.gz_wsym.release();
}

// the header ids, and what a names build needs beside the table it keeps
void release_header_ids(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.n_table.release(); I.n_rec_pos.release(); I.n_ids.release(); I.n_long.release(); I.n_ctl.release();
}

void release_names_find(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.nq_names.release(); I.nq_off.release(); I.nq_out.release(); I.nq_long.release(); I.nq_ctl.release();
}

void release_names_of(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.no_len.release(); I.no_flag.release(); I.no_tiles.release(); I.no_idx.release(); I.no_off.release();
}

void release_lines(crass_hip_ctx *c, LineFetch &B) { wait_main(c); B.release_device(); }

void release_comments_build(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_main(c);
    I.cb_rec_pos.release(); I.cb_cnt.release(); I.cb_flag.release();
}

// a shard's staged text, its BGZF tail, the probe's parts and the wrapped-mode pieces' chains (fastx_shards.h)
void release_shard(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    wait_both(c);
    I.sh_stage.release(); I.sh_tail.release(); I.sh_part.release();
    I.sh_staged.clear(); I.sh_scanned = false;
    for (auto &k : I.sh_cut) { k.scratch.release(); k.text.release(); }
    I.sh_cut.clear(); I.sh_cut_out.release();
}

void ingest_free_all(crass_hip_ctx *c)
{
    Ingest &I = c->in;
    for (auto &k : I.gz_kept) { k.text.release(); k.seed.release(); }
    I.gz_kept.clear();
    release_text(c); release_scan(c); release_bgzf(c); release_gzip(c); release_header_ids(c); release_names_find(c); release_names_of(c);
    release_comments_build(c); I.cb_h.release(); I.cm.free_all(); I.tm_cm.destroy();
    names_drop(c); drop_arena(c);
    release_shard(c); I.sh_h_part.release(); I.tm_probe.destroy(); I.sh_h_cut_out.release();
    for (hipEvent_t &e : I.ev_cut) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    I.hl.free_all(); I.ql.free_all();
    // what is kept from call to call, and the pinned sides of the results
    I.f_idx.release(); I.f_off.release(); I.f_rc.release(); I.f_chars.release();
    I.f_h_idx.release(); I.f_h_off.release(); I.f_h_rc.release(); I.f_h_chars.release();
    I.x_h_tot.release(); I.x_h_rec_pos.release(); I.x_h_seq_off.release(); I.z_h_verdict.release(); I.n_h_ctl.release(); I.nq_h_ctl.release(); I.no_h.release();
    I.fa_h_base.release(); I.fa_h_format.release();
    for (hipEvent_t *e : {&I.ev_t_copy[0], &I.ev_t_copy[1], &I.ev_t_pack[0], &I.ev_t_pack[1]}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    I.tm_pack.destroy(); I.tm_scan.destroy(); I.tm_inflate.destroy(); I.tm_gzip.destroy(); I.tm_gzr.destroy(); I.tm_gzt.destroy(); I.tm_fetch.destroy(); I.tm_names.destroy(); I.tm_find.destroy();
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
void begin_fastx_load(crass_hip_ctx *c)
{
    begin_load(c);
    c->in.last_scan_ms = 0; c->in.last_pack_ms = 0;
    c->in.scan_classes[0] = c->in.scan_classes[1] = 0;
}

// new header ids: pass 1's found flags are keyed by them, so earlier results are void; the resident set's own counters stay
void reset_results_keep_set(crass_hip_ctx *c)
{
    const uint64_t n_reads = c->cnt.n_reads, n_exc = c->cnt.n_exceptions, bytes_dev = c->cnt.bytes_reads_device;
    reset_results(c);
    c->cnt.n_reads = n_reads; c->cnt.n_exceptions = n_exc; c->cnt.bytes_reads_device = bytes_dev;
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
int load_text_impl(crass_hip_ctx *c, const uint8_t *h_seqs, const uint8_t *d_seqs, const uint64_t *off, uint64_t n,
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
int upload_staged(crass_hip_ctx *c, const uint8_t *h_bytes, uint64_t n, uint8_t *dst)
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

// ---- the resident set back out: its packed form, and the text of selected reads ----
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

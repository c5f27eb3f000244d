// engine_names.cpp — the names of device-resident FASTA / FASTQ records (fastx_hid.hip, fastx_lines.hip): header ids, given or computed from
// a file's raw bytes; the name table kept on the device, names looked up in it and names read out of it, from the host or with
// everything in device memory; header lines and quality strings of selected records; the comment kseq hands on from record to
// record (the own-comment bitmap and the tiles' carries kept on the device, the handed comments of listed records).
#include "ingest_internal.h"
#include "fastx_scan.h"

extern "C" {

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

// ---- header ids from a file's raw bytes on the device (fastx_hid.hip) ----
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

int header_ids_device_impl(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n,
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

// ---- the name table kept on the device: names in, first read index out (fastx_hid.hip) ----
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

// the table half of a find job: the kept table and the bytes its record positions point into
static HidFindJob names_table_job(const crass_hip_ctx *c)
{
    HidFindJob J{};
    J.bytes = c->in.nt_bytes; J.n_bytes = c->in.nt_n_bytes; J.rec_pos = c->in.nt_rec_pos.p;
    J.table = c->in.nt_table.p; J.mask = c->in.nt_mask; J.hash_bits = c->env.hid_hash_bits;
    return J;
}

static int names_find_impl(crass_hip_ctx *c, const uint8_t *names, const uint64_t *name_off, uint64_t n_names, const std::vector<uint32_t> &longs,
                           uint64_t *first_out)
{
    const uint64_t total = name_off[n_names];
    HIPCHK(c, c->in.nq_names.ensure(total)); HIPCHK(c, c->in.nq_off.ensure(n_names + 1)); HIPCHK(c, c->in.nq_out.ensure(n_names));
    HIPCHK(c, c->in.nq_long.ensure(longs.size()));
    HidFindJob J = names_table_job(c);
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
    HidFindJob J = names_table_job(c);
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

// ---- header lines and quality strings of selected records from a file's raw bytes on the device (fastx_lines.hip) ----
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
    ops.copy = [&](LineFetch &B, uint64_t total, uint8_t *dst) { return launch_span_copy(SpanCopyJob{d_bytes, n_bytes, B.src.p, B.off.p, n, total, dst}, c->stream); };
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

// the quality string: two words per record, its position and its end; the starts of the quality lines stay on the device; the
// second half is the flags, bit 0: the record has a quality line.  With FASTQ class 1 on the context the records are measured by
// the wrapped rule (k_qw_measure)
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
        return c->in.fastq_class == FX_CLASS_WRAPPED ? launch_qw_measure(J, c->stream) : launch_ql_measure(J, c->stream);
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

// ---- the comment kseq hands on from record to record (fastx_scan.h; k_cm_* of fastx_lines.hip) ----
// The structure is built aside and replaces the one before only when every record position was accepted: a build that fails
// leaves the context as it was.  Queued and waited for here: the positions up, the three launches, the flag and the total back.
static int comments_build_impl(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n,
                               const uint64_t *frb, uint32_t n_files, DevBuf<uint64_t> &bits, DevBuf<uint64_t> &carry, DevBuf<uint64_t> &d_frb,
                               uint64_t *n_own)
{
    Ingest &I = c->in;
    const uint64_t words = (n + 63) / 64, tiles = (n + kFxCmTile - 1) / kFxCmTile;
    HIPCHK(c, bits.ensure(words)); HIPCHK(c, carry.ensure(tiles)); HIPCHK(c, d_frb.ensure((uint64_t)n_files + 1));
    HIPCHK(c, I.cb_rec_pos.ensure(n)); HIPCHK(c, I.cb_cnt.ensure(tiles + 1)); HIPCHK(c, I.cb_flag.ensure(1)); HIPCHK(c, I.cb_h.ensure(2));
    CmBuildJob J{};
    J.bytes = d_bytes; J.n_bytes = n_bytes; J.rec_pos = I.cb_rec_pos.p; J.n_reads = n;
    J.bits = bits.p; J.carry = carry.p; J.tile_cnt = I.cb_cnt.p; J.flag = I.cb_flag.p;
    I.cb_h.p[1] = 0;
    HIPCHK(c, hipMemcpyAsync(I.cb_rec_pos.p, rec_pos, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_frb.p, frb, ((uint64_t)n_files + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(I.cb_flag.p, 0, 4, c->stream));
    HIPCHK(c, I.tm_cm.begin(c->timing_level >= 1, c->stream));
    HIPCHK(c, launch_cm_build(J, c->stream));
    HIPCHK(c, I.tm_cm.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(I.cb_h.p, I.cb_cnt.p + tiles, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(I.cb_h.p + 1, I.cb_flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, I.tm_cm.elapsed(0, 1, &I.last_cm_ms[0]));
    if (I.cb_h.p[1]) return CRASS_ERR_INVALID_ARG;      // a rec_pos[r] >= n_bytes
    *n_own = I.cb_h.p[0];
    return CRASS_OK;
}

int crass_hip_fastx_comments_build_device(crass_hip_ctx *c, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *rec_pos, uint64_t n_reads,
                                          const uint64_t *file_read_base, uint32_t n_files)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    const bool on_arena = !d_bytes && !rec_pos;
    const uint64_t one_file[2] = {0, n_reads};
    if (on_arena) {                                     // the arena and layout of the last crass_hip_load_fastx_files (or of a shard)
        if (!I.have_arena || !c->have_reads || I.fa_read_base.empty() || I.fa_read_base.back() != c->R.n_reads) return CRASS_ERR_STATE;
        d_bytes = I.fa_arena.p; n_bytes = I.fa_bytes; rec_pos = I.x_h_rec_pos.p; n_reads = c->R.n_reads;
        file_read_base = I.fa_read_base.data(); n_files = (uint32_t)(I.fa_read_base.size() - 1);
    } else if (!file_read_base) { file_read_base = one_file; n_files = 1; }
    if (n_reads && (!d_bytes || !rec_pos)) return CRASS_ERR_INVALID_ARG;
    if (n_reads >= 0xFFFFFFFFull) return CRASS_ERR_UNSUPPORTED;
    if (n_files == 0 ? n_reads != 0 : (file_read_base[0] != 0 || file_read_base[n_files] != n_reads)) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (file_read_base[f + 1] < file_read_base[f]) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    I.last_cm_ms[0] = 0;
    DevBuf<uint64_t> bits, carry, d_frb;
    std::vector<uint64_t> h_rec_pos;
    uint64_t n_own = 0;
    int s = CRASS_OK;
    if (n_reads) {
        if (!on_arena) { try { h_rec_pos.assign(rec_pos, rec_pos + n_reads); } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; } }
        s = comments_build_impl(c, d_bytes, n_bytes, rec_pos, n_reads, file_read_base, n_files, bits, carry, d_frb, &n_own);
    }
    release_comments_build(c);                          // the scratch goes back on every way out (the structure built here is a local)
    if (s) { bits.release(); carry.release(); d_frb.release(); return s; }
    comments_drop(c);
    I.ct_bits = bits; I.ct_carry = carry; I.ct_frb = d_frb;      // (DevBuf owns nothing by itself: comments_drop gives them back)
    I.ct_h_rec_pos.swap(h_rec_pos);
    I.have_comments = true; I.ct_on_arena = on_arena;
    I.ct_bytes = d_bytes; I.ct_n_bytes = n_bytes; I.ct_n_reads = n_reads; I.ct_n_files = n_files;
    I.ct_counts[0] = n_own; I.ct_counts[1] = n_reads;
    return CRASS_OK;
}

int crass_hip_fastx_comments_drop(crass_hip_ctx *c)
{
    if (!c) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    comments_drop(c);
    return CRASS_OK;
}

int crass_hip_fastx_comments_counters(const crass_hip_ctx *c, uint64_t out[2])
{
    if (!c || !out) return CRASS_ERR_INVALID_ARG;
    if (!c->in.have_comments) return CRASS_ERR_STATE;
    out[0] = c->in.ct_counts[0]; out[1] = c->in.ct_counts[1];
    return CRASS_OK;
}

float crass_hip_last_comments_ms(const crass_hip_ctx *c, int part) { return c && part >= 0 && part < 2 ? c->in.last_cm_ms[part] : 0.0f; }

// the fetch: the indices up, the sources back, their positions up (the host keeps the record positions), the lengths back (they
// size the result), their prefix sum on the host, the copy launch, the text back or into the caller's device buffer — the shape
// of fetch_lines with one step in front.  Every check comes before the first launch.
static int comments_fetch_impl(crass_hip_ctx *c, const uint64_t *idx, uint64_t n, uint8_t *d_user, uint64_t cap, uint64_t *off_user, crass_text *out,
                               uint8_t *has_out)
{
    Ingest &I = c->in;
    LineFetch &B = I.cm;
    const uint64_t *rec_pos = I.ct_on_arena ? I.x_h_rec_pos.p : I.ct_h_rec_pos.data();
    HIPCHK(c, B.h_off.ensure(n + 1));
    uint64_t *off = B.h_off.p;
    off[0] = 0;
    if (n) {
        HIPCHK(c, B.h_src.ensure(2 * n)); HIPCHK(c, B.h_len.ensure(n));
        HIPCHK(c, B.src.ensure(2 * n)); HIPCHK(c, B.start.ensure(n)); HIPCHK(c, B.len.ensure(n));
        CmFetchJob J{};
        J.bytes = I.ct_bytes; J.n_bytes = I.ct_n_bytes; J.bits = I.ct_bits.p; J.carry = I.ct_carry.p; J.n_reads = I.ct_n_reads;
        J.file_read_base = I.ct_frb.p; J.n_files = I.ct_n_files;
        J.idx = B.src.p; J.n = n; J.src = B.src.p + n; J.pos = B.src.p; J.start = B.start.p; J.len = B.len.p;
        memcpy(B.h_src.p, idx, n * 8);
        HIPCHK(c, hipMemcpyAsync(B.src.p, B.h_src.p, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, I.tm_cm.begin(c->timing_level >= 1, c->stream));
        HIPCHK(c, launch_cm_source(J, c->stream));
        HIPCHK(c, hipMemcpyAsync(B.h_src.p + n, B.src.p + n, n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));     // (the sources become positions on the host)
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t src = B.h_src.p[n + k];
            const bool has = src < I.ct_n_reads;
            if (has_out) has_out[k] = has ? 1 : 0;
            B.h_src.p[k] = has ? rec_pos[src] + 1 : kFxNone;
        }
        HIPCHK(c, hipMemcpyAsync(B.src.p, B.h_src.p, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_cm_measure(J, c->stream));
        HIPCHK(c, hipMemcpyAsync(B.h_len.p, B.len.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));     // (the lengths size the result)
        for (uint64_t k = 0; k < n; k++) off[k + 1] = off[k] + B.h_len.p[k];
        const uint64_t total = off[n];
        if (off_user) memcpy(off_user, off, (n + 1) * 8);
        if (d_user && cap < total) return CRASS_ERR_OVERFLOW;
        if (!d_user) HIPCHK(c, B.h_chars.ensure(total));
        if (out) { out->n = n; out->chars = B.h_chars.p; out->off = off; }
        if (total) {
            HIPCHK(c, B.off.ensure(n + 1));
            if (!d_user) HIPCHK(c, B.chars.ensure(total));
            HIPCHK(c, hipMemcpyAsync(B.off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, launch_span_copy(SpanCopyJob{J.bytes, J.n_bytes, J.start, B.off.p, n, total, d_user ? d_user : B.chars.p}, c->stream));
            if (!d_user) HIPCHK(c, hipMemcpyAsync(B.h_chars.p, B.chars.p, total, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, I.tm_cm.mark(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, I.tm_cm.elapsed(0, 1, &I.last_cm_ms[1]));
        return CRASS_OK;
    }
    if (off_user) off_user[0] = 0;
    if (!d_user) HIPCHK(c, B.h_chars.ensure(0));
    if (out) { out->n = 0; out->chars = B.h_chars.p; out->off = off; }
    return CRASS_OK;
}

static int comments_fetch_common(crass_hip_ctx *c, const uint64_t *idx, uint64_t n, uint8_t *d_user, uint64_t cap, uint64_t *off_user, crass_text *out,
                                 uint8_t *has_out)
{
    if (!c || (n && !idx)) return CRASS_ERR_INVALID_ARG;
    Ingest &I = c->in;
    if (!I.have_comments) {                             // the first fetch after a files load builds on the resident arena
        if (!I.have_arena || !c->have_reads) return CRASS_ERR_STATE;
        const int bs = crass_hip_fastx_comments_build_device(c, nullptr, 0, nullptr, 0, nullptr, 0);
        if (bs) return bs;
    }
    for (uint64_t k = 0; k < n; k++) if (idx[k] >= I.ct_n_reads) return CRASS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    I.last_cm_ms[1] = 0;
    const int s = comments_fetch_impl(c, idx, n, d_user, cap, off_user, out, has_out);
    release_lines(c, I.cm);                             // the scratch goes back on every way out; the structure and the pinned sides stay
    return s;
}

int crass_hip_fetch_comments_device(crass_hip_ctx *c, const uint64_t *idx, uint64_t n, crass_text *out, uint8_t *has_out)
{
    if (!out) return CRASS_ERR_INVALID_ARG;
    return comments_fetch_common(c, idx, n, nullptr, 0, nullptr, out, has_out);
}

int crass_hip_fetch_comments_device_to(crass_hip_ctx *c, const uint64_t *idx, uint64_t n, uint8_t *d_chars, uint64_t cap_bytes, uint64_t *off_out,
                                       uint8_t *has_out)
{
    if (!off_out || (!d_chars && cap_bytes)) return CRASS_ERR_INVALID_ARG;
    static uint8_t nowhere;                             // (a NULL buffer of capacity 0 asks for the offsets alone, as in crass_hip_fetch_text_device)
    return comments_fetch_common(c, idx, n, d_chars ? d_chars : &nowhere, cap_bytes, off_out, nullptr, has_out);
}

} // extern "C"

// (fastx_shards.h: the group's found-name exchange reads the count, the answers stay on the device)
uint64_t names_find_device_found(const crass_hip_ctx *c) { return c ? c->in.last_find_found : 0; }

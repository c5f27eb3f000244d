// ingest.cpp — the ingest side of the boundary, its first file: the 2-bit packer with an exception list.  The FASTA/FASTQ(.gz)
// reader with kseq_read record semantics is fastx_parse.cpp (the parser), host_inflate.cpp and the three readers built on them
// (fastx_read.cpp, fastx_index.cpp, fastx_stream.cpp); the synthetic metagenome of bench.py and the parity tests is synth.cpp.
// Host-only C++17 (+ zlib); what crosses these files: host_ingest_internal.h.
#include "host_ingest_internal.h"

using namespace crass;

// the layout of a packed set: crass_pack_reads and the device packer (crass_hip_load_text, crass_hip_attach_device_text) decide here
int crass::pack_layout(const uint64_t *off, uint64_t n, int pad_uniform, crass::PackLayout *out)
{
    *out = crass::PackLayout();
    uint32_t max_len = 0, min_len = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return CRASS_ERR_INVALID_ARG;
        uint64_t l = off[i + 1] - off[i];
        if (l > CRASS_HIP_MAX_READ_LEN) return CRASS_ERR_UNSUPPORTED;
        max_len = std::max<uint32_t>(max_len, (uint32_t)l);
        min_len = std::min<uint32_t>(min_len, (uint32_t)l);
    }
    if (n == 0) min_len = 0;
    uint64_t tight = 0;
    for (uint64_t i = 0; i < n; i++) tight += (off[i + 1] - off[i] + 15) / 16;
    crass::pack_layout_core(n, max_len, min_len, tight, pad_uniform, out);
    return CRASS_OK;
}

// ... from what the offsets say: n reads of min_len .. max_len bases (min_len 0 where n is 0) in `tight` words when none is padded
void crass::pack_layout_core(uint64_t n, uint32_t max_len, uint32_t min_len, uint64_t tight, int pad_uniform, crass::PackLayout *out)
{
    const bool uniform_len = (n > 0 && max_len == min_len && max_len > 0);       // (uniform_len == 0 says "lengths differ": a set of empty reads keeps its lengths array)
    uint32_t stride = 0;
    if (pad_uniform == 2) {
        // auto: short reads of differing lengths (trimmed Illumina data) are padded to one stride when that costs at
        // most twice the words — the bit-parallel filter and the lane-per-read kernels need a uniform stride
        const uint64_t padded = n * (uint64_t)((max_len + 15) / 16);
        pad_uniform = (max_len <= 256 && max_len >= 64 && padded <= 2 * tight) ? 1 : 0;
    }
    if (pad_uniform || uniform_len) stride = std::max<uint32_t>(1, (max_len + 15) / 16);
    out->max_len = max_len; out->stride_words = stride; out->uniform_len = uniform_len ? max_len : 0;
    out->total_words = stride ? n * (uint64_t)stride : tight;
}

void crass::fill_reads(crass_reads &r, uint64_t n, const crass::PackLayout &lay, const uint32_t *packed, const uint64_t *word_off, const uint32_t *lengths, const PackedOwner &exc)
{
    r.n_reads = n; r.packed = packed; r.stride_words = lay.stride_words;
    r.word_off = lay.stride_words ? nullptr : word_off;
    r.uniform_len = lay.uniform_len;
    r.lengths = lay.uniform_len ? nullptr : lengths;
    r.n_exceptions = exc.exc_read.size();
    r.exc_read = exc.exc_read.data(); r.exc_off = exc.exc_off.data(); r.exc_bytes = exc.exc_bytes.data();
    r.header_id = nullptr; r.read_index_base = 0;
}

int crass::packed_alloc(uint64_t n_words, uint64_t n_word_off, uint64_t n_lengths, uint64_t n_exc_read, uint64_t n_exc_off, uint64_t n_exc_bytes,
                        uint64_t n_header_id, crass_packed *out, crass::PackedArrays *a)
{
    memset(out, 0, sizeof(*out));
    PackedOwner *o = new (std::nothrow) PackedOwner();
    if (!o) return CRASS_ERR_OOM;
    try {
        o->packed.resize(n_words); o->word_off.resize(n_word_off); o->lengths.resize(n_lengths); o->exc_read.resize(n_exc_read);
        o->exc_off.resize(n_exc_off); o->exc_bytes.resize(n_exc_bytes); o->header_id.resize(n_header_id);
    } catch (const std::bad_alloc &) { delete o; return CRASS_ERR_OOM; }
    a->packed = n_words ? o->packed.data() : nullptr; a->word_off = n_word_off ? o->word_off.data() : nullptr;
    a->lengths = n_lengths ? o->lengths.data() : nullptr; a->exc_read = n_exc_read ? o->exc_read.data() : nullptr;
    a->exc_off = n_exc_off ? o->exc_off.data() : nullptr; a->exc_bytes = n_exc_bytes ? o->exc_bytes.data() : nullptr;
    a->header_id = n_header_id ? o->header_id.data() : nullptr;
    out->owner = o;
    return CRASS_OK;
}

extern "C" {

uint32_t crass_pack_code4(uint32_t four_bytes, uint32_t *bad)
{
    uint32_t b = 0;
    const uint32_t c = crass::pack_code4(four_bytes, &b);
    if (bad) *bad = b;
    return c;
}

int crass_pack_layout(const uint64_t *off, uint64_t n_reads, int pad_uniform, uint32_t *stride_words, uint32_t *uniform_len)
{
    if (n_reads && !off) return CRASS_ERR_INVALID_ARG;
    crass::PackLayout lay;
    const int s = crass::pack_layout(off, n_reads, pad_uniform, &lay);
    if (stride_words) *stride_words = lay.stride_words;
    if (uniform_len) *uniform_len = lay.uniform_len;
    return s;
}

int crass_pack_reads(const uint8_t *seqs, const uint64_t *off, uint64_t n, int pad_uniform, crass_packed *out)
{
    if (!out || (n && (!seqs || !off))) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    crass::PackLayout lay;
    // (offsets that decrease have always been reported here as a read beyond the length limit)
    if (const int ls = crass::pack_layout(off, n, pad_uniform, &lay)) return ls == CRASS_ERR_INVALID_ARG ? CRASS_ERR_UNSUPPORTED : ls;
    PackedOwner *o = new PackedOwner();
    const uint32_t stride = lay.stride_words;
    const bool uniform_len = lay.uniform_len != 0;
    if (!stride) {
        o->word_off.resize(n + 1);
        uint64_t w = 0;
        for (uint64_t i = 0; i < n; i++) { o->word_off[i] = w; w += (off[i + 1] - off[i] + 15) / 16; }
        o->word_off[n] = w;
        o->packed.assign(w + 4, 0);
    } else {
        o->packed.assign(n * (uint64_t)stride + 4, 0);
    }
    if (!uniform_len) { o->lengths.resize(n); for (uint64_t i = 0; i < n; i++) o->lengths[i] = (uint32_t)(off[i + 1] - off[i]); }
    const unsigned nt = std::min<unsigned>(hw_threads(), 64);
    std::vector<std::vector<uint64_t>> exc_parts(nt);
    uint32_t *packed = o->packed.data();
    // byte -> 2-bit code, 0x80 for anything outside ACGT; one output word is built in a register per 16 bases
    const uint8_t *const lut = base_lut();
    parallel_ranges(n, nt, [&](uint64_t a, uint64_t b, unsigned t) {
        for (uint64_t i = a; i < b; i++) {
            const uint8_t *s = seqs + off[i];
            const uint32_t L = (uint32_t)(off[i + 1] - off[i]);
            uint32_t *w = packed + (stride ? i * (uint64_t)stride : o->word_off[i]);
            uint32_t bad = 0;
            uint32_t k = 0;
            for (; k + 16 <= L; k += 16) {
                uint32_t acc = 0;
                for (int q = 0; q < 16; q++) { const uint32_t c = lut[s[k + q]]; bad |= c; acc |= (c & 3u) << (2 * q); }
                w[k >> 4] = acc;
            }
            if (k < L) {
                uint32_t acc = 0;
                for (uint32_t q = 0; k + q < L; q++) { const uint32_t c = lut[s[k + q]]; bad |= c; acc |= (c & 3u) << (2 * q); }
                w[k >> 4] = acc;
            }
            if (bad & 0x80u) exc_parts[t].push_back(i);
        }
    });
    for (auto &p : exc_parts) o->exc_read.insert(o->exc_read.end(), p.begin(), p.end());
    std::sort(o->exc_read.begin(), o->exc_read.end());
    o->exc_off.push_back(0);
    for (uint64_t r : o->exc_read) {
        o->exc_bytes.insert(o->exc_bytes.end(), seqs + off[r], seqs + off[r + 1]);
        o->exc_off.push_back(o->exc_bytes.size());
    }
    fill_reads(out->reads, n, lay, o->packed.data(), o->word_off.data(), o->lengths.data(), *o);
    out->owner = o;
    return CRASS_OK;
}

void crass_free_packed(crass_packed *p)
{
    if (!p) return;
    delete static_cast<PackedOwner *>(p->owner);
    memset(p, 0, sizeof(*p));
}

} // extern "C"

// fastx_shards_gzip.cpp — the record-aligned shards of a job on the host (fastx_scan.cpp) when plain gzip files are taken
// (crass_hip_group_set_gzip_on_device): such a file's text is crass_gzip_inflate_host's (gunzip.cpp; with
// CRASS_GZIP_ON_DEVICE_MEMBERS crass_gzip_inflate_members_host's, a file of any number of members), then the job is cut and judged
// as crass_fastx_files_shards_host_class does.  Host-only C++17, no GPU needed.
#include "../../include/crass_hip.h"
#include "gunzip_core.h"

#include <cstring>
#include <new>
#include <vector>

extern "C" int crass_fastx_files_shards_host_gzip(const uint8_t *const *bytes, const uint64_t *n_bytes, uint32_t n_files, uint32_t n_ranks,
                                                  const uint64_t *nominal, int fastq_class, int gzip_mode, uint64_t chunk_bytes, crass_fastx_shards *out)
{
    if (!gzip_mode) return crass_fastx_files_shards_host_class(bytes, n_bytes, n_files, n_ranks, nominal, fastq_class, out);
    if (!out) return CRASS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->decline_file = -1; out->n_ranks = n_ranks; out->n_files = n_files;
    if (!n_files || !bytes || !n_bytes) return CRASS_ERR_INVALID_ARG;
    for (uint32_t f = 0; f < n_files; f++) if (n_bytes[f] && !bytes[f]) return CRASS_ERR_INVALID_ARG;
    try {
        // the plain gzip files as their text, up to the first one that does not inflate
        std::vector<std::vector<uint8_t>> text(n_files);
        std::vector<const uint8_t *> b(bytes, bytes + n_files);
        std::vector<uint64_t> n(n_bytes, n_bytes + n_files);
        uint32_t nf = n_files;
        const bool members = gzip_mode == CRASS_GZIP_ON_DEVICE_MEMBERS;
        crass_bgzf_verdict bad;
        memset(&bad, 0, sizeof(bad));
        for (uint32_t f = 0; f < nf; f++) {
            if (n[f] < 2 || b[f][0] != 0x1F || b[f][1] != 0x8B) continue;
            crass_bgzf_index ix;
            const int is = crass_bgzf_index_host(b[f], n[f], &ix);
            const bool plain = is == CRASS_ERR_UNSUPPORTED && ix.decline.reason == crass::BZ_NOT_BGZF;
            crass_bgzf_index_free(&ix);
            if (!plain) continue;                         // (BGZF, or a decline that is the BGZF index's own)
            uint64_t nt = 0;
            // (CRASS_GZIP_ON_DEVICE_MEMBERS: a file of any number of members, crass_gzip_inflate_members_host's text and verdict)
            auto inflate = [&](uint8_t *o, uint64_t cap) {
                return members ? crass_gzip_inflate_members_host(b[f], n[f], chunk_bytes, o, cap, &nt, nullptr, nullptr, &bad)
                               : crass_gzip_inflate_host(b[f], n[f], chunk_bytes, o, cap, &nt, nullptr, &bad);
            };
            int s = inflate(nullptr, 0);
            if (s == CRASS_ERR_OVERFLOW || s == CRASS_OK) {
                text[f].resize(nt + 1);
                s = inflate(text[f].data(), nt);
            }
            if (s == CRASS_ERR_UNSUPPORTED) { nf = f; break; }
            if (s) return s;
            b[f] = text[f].data(); n[f] = nt;
        }
        if (nf == n_files) return crass_fastx_files_shards_host_class(b.data(), n.data(), n_files, n_ranks, nominal, fastq_class, out);
        // file nf does not inflate: that is the job's verdict unless a file in front of it is declined
        if (!n_ranks || n_ranks > 64 || fastq_class < 0 || fastq_class > 1) return CRASS_ERR_INVALID_ARG;
        if (nf) {
            crass_fastx_files_layout L;
            const int s = crass_fastx_files_scan_host_class(b.data(), n.data(), nf, fastq_class, &L);
            if (s == CRASS_OK) crass_fastx_files_layout_free(&L);
            else {
                out->decline_file = L.decline_file; out->decline_reason = L.decline_reason; out->decline_pos = L.decline_pos; out->bgzf = L.bgzf;
                return s;
            }
        }
        out->decline_file = (int32_t)nf; out->bgzf = bad;
        return CRASS_ERR_UNSUPPORTED;
    } catch (const std::bad_alloc &) { return CRASS_ERR_OOM; }
}

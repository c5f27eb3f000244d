// fastx_names.hip — what the header lines of a FASTA / FASTQ file's raw bytes hold, on the device, for a caller whose bytes
// exist only in HBM: header_id (the index of the first read with the same NAME: readsFound's key, libcrispr.cpp:138,411) and the
// header lines of selected records (RH_Header / RH_Comment).  The restatement both are tested against is the host's
// crass_fastx_header_ids (fastx_scan.cpp) and kseq's name cut.
//
// A NAME is the bytes behind the record's header character up to the first isspace() byte (' ', '\t' .. '\r') or the input's end.
// Names lie at any byte offset: they are read as ALIGNED dwords, funnel-shifted into name-relative dwords (v_alignbyte_b32), so a
// name's hash and the comparison of two names do not depend on where they lie.  No byte below bytes or at / beyond bytes + n_bytes
// is read: the one dword that holds the input's first byte and the one that holds its last are loaded byte by byte (nm_ld4).
//
// header ids — an open-addressing table of 2^k >= 2 n_reads slots of 64 bits, {hash tag : 32 | read index : 32}, all-ones = free:
//   k_hid_insert       a lane per record: hash the name, probe linearly.  Free slot: claim it by CAS.  Other tag: next slot.  Same
//                      tag: compare the names byte for byte, lengths included — equal: atomicMin on the slot (same tag, so the
//                      smaller index), different: next slot.  A slot's owner only ever changes to a read with the IDENTICAL name,
//                      so the comparison's outcome does not depend on when the slot was read; no lane waits for another.  The
//                      record's slot goes to ids[r].  Names beyond kHidLaneMax bytes are only listed ...
//   k_hid_insert_long  ... and inserted by a wave per record (a 12 KB name must not be one lane's tail): the wave finds the name's
//                      end 256 bytes a step, hashes and compares a dword per lane.  The two kernels hash differently, which is
//                      fine: equal names have equal lengths, so both are hashed by the same kernel.
//   k_hid_lookup       a launch of its own, so the table is final: ids[r] = the index in the record's slot — the smallest index
//                      with that name, whatever the scheduling.  (The slot was kept at insert, so no name is read twice.)
//   k_hid_find        names in, first index out, on a table that is kept (crass_hip_fastx_names_build_device): a lane per query.  The
//                      query is a name that ends with its own bytes: it is hashed by the function k_hid_insert hashes with
//                      (hid_hash_lane), then probed for linearly from the hash's slot — free slot: not found; other tag: next slot;
//                      same tag: the query against the slot owner's name, lengths included; equal: the slot's index.  The table is
//                      final and only read: no atomics, no waiting, and a probe that has seen every slot ends with not found.
//   k_hid_find_long    a wave per query of kHidLaneEnd bytes or more, hashed as k_hid_insert_long hashes (hid_hash_wave).
//   k_hid_find_dev     k_hid_find for queries made on the device (another rank's names): it checks the offsets nobody on the host
//                      has seen and lists the long queries itself, one add per wave; k_hid_find_long then runs over that list.
//   k_nm_measure_idx / k_nm_scan_tiles, _top, _apply / k_nm_copy   the names of listed records of the kept table, back to back in
//                      device memory with their offsets: lengths, a three-launch prefix sum, a lane per output byte.
// No answer rests on a hash: hash_bits (CRASS_HID_TEST_HASH_BITS) cuts the hash to its low bits, down to none, for the tests.
// Slot accesses are agent-scope atomics; the name bytes and rec_pos are read-only input.
//
// header lines — k_hl_measure: a lane per selected record walks its header line: bytes up to the '\n' (or the input's end) and the
// name's length.  The host sums the lengths.  k_hl_copy: driven by the OUTPUT, a lane per byte finds its record in the offsets;
// nothing outside [out, out + total) is stored.  Neither is hot: about one read in a hundred is handed on.
//
// handed comments (RH_Comment as kseq hands it on, fastx_scan.h) — build: k_cm_bits, a lane per record walks its name as
// k_hl_measure does, fx_own_comment decides, the wave's ballot is one word of the own-comment bitmap; k_cm_tiles, a wave per tile
// of kFxCmTile records: the tile's last own-comment record and their number; k_cm_top, one block: the running maximum over the
// tiles (the carries) and the total.  Three launches, no block waits for another, no atomics.  fetch: k_cm_source, a lane per
// listed record: fx_comment_handed_from, the statements the host runs; the host turns the sources into positions (it keeps the
// record positions, the device does not); k_cm_measure walks the source's name and comment, k_cm_copy is k_hl_copy from the
// comments' starts.  Names of any length take the lane walk.
//
// quality strings (RH_Qual) — the same shape.  k_ql_measure: a lane per selected record; a record whose header character is '@'
// has its quality on its fourth line, found by three line ends from the header character and bounded by the next record's header
// character: the string is the bytes 33..126 of that line, as kseq keeps them (a '\r' in front of the '\n' is none).  A '>'
// record has none.  k_ql_copy: a lane per output byte; where the line's first bytes are the string (every line but one with
// blanks inside) the byte is at start + k, else the lane walks the line to its k-th such byte.  No byte outside
// [src, min(lim, n_bytes)) of a record is read.
#include "fastx_names_launch.h"
#include "devmem.h"
#include "fastx_scan.h"

namespace crass {

static constexpr int kNmThreads = 256;
static constexpr uint32_t kHidLaneMax = 256;             // names beyond this many bytes go to the wave kernel
static constexpr uint32_t kHidLaneEnd = kHidLaneMax + 4; // ... seen a dword at a time: names of this many bytes or more are the wave kernels'

// the aligned dword at address q of the input [lo, hi); bytes outside the input read as 0 and are not touched
static __device__ __forceinline__ uint32_t nm_ld4(uintptr_t lo, uintptr_t hi, uintptr_t q)
{
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t *>(q);
    uint32_t w = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) { const uintptr_t a = q + j; if (a >= lo && a < hi) w |= (uint32_t)*reinterpret_cast<const uint8_t *>(a) << (8 * j); }
    return w;
}

// the input's bytes from a position on, four at a time (byte 0 lowest); one aligned load per step
struct NmCur {
    uintptr_t lo, hi, q;
    uint32_t w0, sh;
    uint64_t left;                   // bytes from here to the input's end
    __device__ __forceinline__ void init(uintptr_t lo_, uintptr_t hi_, uint64_t pos)      // pos <= hi - lo
    {
        lo = lo_; hi = hi_;
        const uintptr_t a = lo + pos;
        sh = (uint32_t)(a & 3u); q = a - sh; left = hi - a;
        w0 = left ? nm_ld4(lo, hi, q) : 0u;
    }
    __device__ __forceinline__ uint32_t next(uint32_t *avail)      // *avail: how many of the four bytes are inside the input
    {
        const uint32_t w1 = left > 4u - sh ? nm_ld4(lo, hi, q + 4) : 0u;
        const uint32_t w = __builtin_amdgcn_alignbyte(w1, w0, sh);
        *avail = left < 4 ? (uint32_t)left : 4u;
        w0 = w1; q += 4; left -= *avail;
        return w;
    }
};
// the four bytes at a position, without a cursor (the wave kernel: a dword per lane)
static __device__ __forceinline__ uint32_t nm_dword_at(uintptr_t lo, uintptr_t hi, uint64_t pos, uint32_t *avail)
{
    if (pos >= hi - lo) { *avail = 0; return 0u; }
    NmCur c;
    c.init(lo, hi, pos);
    return c.next(avail);
}

static __device__ __forceinline__ uint32_t nm_is_space(uint32_t c) { return (uint32_t)(c - 9u < 5u) | (uint32_t)(c == 32u); }
// how many of the first `avail` bytes of w come before the first isspace() byte / the first '\n'
static __device__ __forceinline__ uint32_t nm_name_bytes(uint32_t w, uint32_t avail)
{
    uint32_t stop = 1u << avail;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) stop |= nm_is_space((w >> (8 * j)) & 0xFFu) << j;
    return (uint32_t)__builtin_ctz(stop);
}
static __device__ __forceinline__ uint32_t nm_line_bytes(uint32_t w, uint32_t avail)
{
    uint32_t stop = 1u << avail;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) stop |= (uint32_t)(((w >> (8 * j)) & 0xFFu) == 10u) << j;
    return (uint32_t)__builtin_ctz(stop);
}
static __device__ __forceinline__ uint32_t nm_low_bytes(uint32_t cnt) { return cnt >= 4 ? 0xFFFFFFFFu : (1u << (8 * cnt)) - 1u; }

static __device__ __forceinline__ uint64_t nm_fmix(uint64_t h)      // (the 64-bit finaliser of MurmurHash3)
{
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
    return h;
}
static __device__ __forceinline__ uint64_t nm_cut(uint64_t h, uint32_t bits) { return bits >= 64 ? h : bits == 0 ? 0ull : h & ((1ull << bits) - 1ull); }

static __device__ __forceinline__ unsigned long long hid_load(unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// claims a free slot; true: it is ours, else *seen is what the slot holds
static __device__ __forceinline__ bool hid_claim(unsigned long long *p, unsigned long long mine, unsigned long long *seen)
{
    unsigned long long expected = kHidEmpty;
    const bool won = __hip_atomic_compare_exchange_strong(p, &expected, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *seen = expected;
    return won;
}
static __device__ __forceinline__ void hid_min(unsigned long long *p, unsigned long long mine) { (void)__hip_atomic_fetch_min(p, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one lane: is the name at a of the input [loa, hia) the name at b of [lob, hib)?  (Both end at their first isspace() byte or their
// input's end; the walk ends with the shorter of the two.)
static __device__ __forceinline__ bool hid_same_name_lane(uintptr_t loa, uintptr_t hia, uint64_t a, uintptr_t lob, uintptr_t hib, uint64_t b)
{
    NmCur ca, cb;
    ca.init(loa, hia, a); cb.init(lob, hib, b);
    for (;;) {
        uint32_t ava, avb;
        const uint32_t wa = ca.next(&ava), wb = cb.next(&avb);
        const uint32_t na = nm_name_bytes(wa, ava), nb = nm_name_bytes(wb, avb);
        if (na != nb || ((wa ^ wb) & nm_low_bytes(na))) return false;
        if (na < 4) return true;
    }
}

// one lane hashes the name at pos of the input [lo, hi): its length and its hash before the cut to hash_bits.  False: the name is
// of kHidLaneEnd bytes or more, the wave kernels'.  (k_hid_insert and k_hid_find: the one function, so the two cannot drift.)
static __device__ __forceinline__ bool hid_hash_lane(uintptr_t lo, uintptr_t hi, uint64_t pos, uint64_t *h_out, uint32_t *len_out)
{
    NmCur c;
    c.init(lo, hi, pos);
    uint64_t h = 0x9E3779B97F4A7C15ull;
    uint32_t len = 0;
    for (;;) {
        uint32_t avail;
        const uint32_t w = c.next(&avail);
        const uint32_t cnt = nm_name_bytes(w, avail);
        if (cnt) { h = (h ^ (w & nm_low_bytes(cnt))) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
        len += cnt;
        if (cnt < 4) break;
        if (len > kHidLaneMax) return false;
    }
    *h_out = nm_fmix(h ^ len); *len_out = len;
    return true;
}

__global__ __launch_bounds__(kNmThreads) void k_hid_insert(const HidJob J)
{
    const uint64_t r = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (r >= J.n_reads) return;
    const uint64_t pos = J.rec_pos[r];
    if (pos >= J.n_bytes) { J.ctl[1] = 1u; J.ids[r] = kHidEmpty; return; }
    const uintptr_t lo = (uintptr_t)J.bytes, hi = lo + J.n_bytes;
    uint64_t h;
    uint32_t len;
    if (!hid_hash_lane(lo, hi, pos + 1, &h, &len)) {    // the wave kernel's
        J.long_list[atomicAdd(&J.ctl[0], 1u)] = (uint32_t)r;
        return;
    }
    h = nm_cut(h, J.hash_bits);
    const unsigned long long tag = h >> 32, mine = (tag << 32) | r;
    uint64_t s = h & J.mask;
    for (;;) {                                          // (ends: the table has more slots than there are records)
        unsigned long long cur = hid_load(&J.table[s]);
        if (cur == kHidEmpty && hid_claim(&J.table[s], mine, &cur)) break;
        if ((cur >> 32) == tag) {
            const uint64_t owner = cur & 0xFFFFFFFFull;
            if (owner == r || hid_same_name_lane(lo, hi, pos + 1, lo, hi, J.rec_pos[owner] + 1)) {
                if (owner > r) hid_min(&J.table[s], mine);
                break;
            }
        }
        s = (s + 1) & J.mask;
    }
    J.ids[r] = s;
}

static __device__ __forceinline__ uint64_t nm_bcast64(uint64_t v, int src)
{
    const uint32_t a = (uint32_t)__shfl((int)(uint32_t)v, src), b = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)b << 32) | a;
}
static __device__ __forceinline__ uint64_t nm_wave_sum64(uint64_t v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)(uint32_t)v, s), b = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s);
        v += ((uint64_t)b << 32) | a;
    }
    return v;
}

// the wave: is the name of len bytes at a of the input [loa, hia) the name at b of [lob, hib)?  (The len bytes are equal and b's
// name ends behind them.)
static __device__ __forceinline__ bool hid_same_name_wave(uintptr_t loa, uintptr_t hia, uint64_t a, uint64_t len, uintptr_t lob, uintptr_t hib, uint64_t b,
                                                          uint32_t lane)
{
    const uint64_t n = hib - lob;
    if (b > n || n - b < len) return false;
    if (b + len < n && !nm_is_space(*reinterpret_cast<const uint8_t *>(lob + b + len))) return false;
    for (uint64_t k0 = 0; 4 * k0 < len; k0 += 64) {
        const uint64_t k = k0 + lane;
        uint32_t diff = 0;
        if (4 * k < len) {
            uint32_t ava, avb;
            const uint32_t wa = nm_dword_at(loa, hia, a + 4 * k, &ava), wb = nm_dword_at(lob, hib, b + 4 * k, &avb);
            const uint64_t rest = len - 4 * k;
            diff = (wa ^ wb) & nm_low_bytes(rest < 4 ? (uint32_t)rest : 4u);
        }
        if (__any(diff != 0)) return false;
    }
    return true;
}

// the wave hashes the name at a of the input [lo, hi): its length and its hash before the cut to hash_bits, the same in every lane.
// (k_hid_insert_long and k_hid_find_long: the one function.)
static __device__ __forceinline__ uint64_t hid_hash_wave(uintptr_t lo, uintptr_t hi, uint64_t a, uint32_t lane, uint64_t *len_out)
{
    // the name's end, 64 dwords a step; every dword of the name is mixed with its index, the sum is the hash
    uint64_t acc = 0, len = 0;
    for (uint64_t k0 = 0;; k0 += 64) {
        const uint64_t k = k0 + lane;
        uint32_t avail;
        const uint32_t w = nm_dword_at(lo, hi, a + 4 * k, &avail);
        const uint32_t cnt = nm_name_bytes(w, avail);
        const unsigned long long ended = __ballot(cnt < 4);
        const uint32_t first = ended ? (uint32_t)__builtin_ctzll(ended) : 64u;
        if (lane <= first && cnt) acc += nm_fmix(((k + 1) << 32) | (w & nm_low_bytes(cnt)));
        if (ended) { len = 4 * (k0 + first) + (uint32_t)__shfl((int)cnt, (int)first); break; }
    }
    *len_out = len;
    return nm_fmix(nm_wave_sum64(acc) ^ len);
}

__global__ __launch_bounds__(kNmThreads) void k_hid_insert_long(const HidJob J, const uint32_t n_long)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t li = (uint64_t)blockIdx.x * (kNmThreads / 64) + (threadIdx.x >> 6);
    if (li >= n_long) return;                           // (the whole wave)
    const uint64_t r = J.long_list[li];
    const uintptr_t lo = (uintptr_t)J.bytes, hi = lo + J.n_bytes;
    const uint64_t a = J.rec_pos[r] + 1;
    uint64_t len;
    const uint64_t h = nm_cut(hid_hash_wave(lo, hi, a, lane, &len), J.hash_bits);
    const unsigned long long tag = h >> 32, mine = (tag << 32) | r;
    uint64_t s = h & J.mask;
    for (;;) {                                          // (every lane takes the same way: lane 0's view of the slot decides)
        unsigned long long cur = 0;
        uint32_t won = 0;
        if (lane == 0) {
            cur = hid_load(&J.table[s]);
            if (cur == kHidEmpty) won = hid_claim(&J.table[s], mine, &cur) ? 1u : 0u;
        }
        if (__shfl((int)won, 0)) break;
        cur = nm_bcast64(cur, 0);
        if ((cur >> 32) == tag) {
            const uint64_t owner = cur & 0xFFFFFFFFull;
            if (owner == r || hid_same_name_wave(lo, hi, a, len, lo, hi, J.rec_pos[owner] + 1, lane)) {
                if (lane == 0 && owner > r) hid_min(&J.table[s], mine);
                break;
            }
        }
        s = (s + 1) & J.mask;
    }
    if (lane == 0) J.ids[r] = s;
}

__global__ __launch_bounds__(kNmThreads) void k_hid_lookup(const HidJob J)
{
    const uint64_t r = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    uint32_t rep = 0;
    if (r < J.n_reads) {
        const uint64_t s = J.ids[r];
        if (s <= J.mask) {                              // (not so behind a rec_pos beyond the input: the call fails, nothing is read)
            const uint64_t id = hid_load(&J.table[s]) & 0xFFFFFFFFull;
            J.ids[r] = id;
            rep = id != r ? 1u : 0u;
        }
    }
    const unsigned long long m = __ballot(rep);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(J.n_repeated, (unsigned long long)__builtin_popcountll(m));
}

// ---- names in, first index out: the table of crass_hip_fastx_names_build_device is final here and only read ----
// a query is an input of its own, [names + name_off[k], names + name_off[k + 1]): the name that starts with it ends with it, or
// before that at an isspace() byte — then no record's name equals the query

// the probe of one lane for a query of hash h (cut already): every step ends the loop or moves on a slot, mask + 1 steps at most
static __device__ __forceinline__ uint64_t hid_probe_lane(const HidFindJob &J, uintptr_t qlo, uintptr_t qhi, uint64_t h)
{
    const uintptr_t lo = (uintptr_t)J.bytes, hi = lo + J.n_bytes;
    const unsigned long long tag = h >> 32;
    uint64_t s = h & J.mask;
    for (uint64_t step = 0; step <= J.mask; step++) {
        const unsigned long long cur = J.table[s];
        if (cur == kHidEmpty) break;
        if ((cur >> 32) == tag) {
            const uint64_t owner = cur & 0xFFFFFFFFull;
            if (hid_same_name_lane(qlo, qhi, 0, lo, hi, J.rec_pos[owner] + 1)) return owner;
        }
        s = (s + 1) & J.mask;
    }
    return kHidNotFound;
}

__global__ __launch_bounds__(kNmThreads) void k_hid_find(const HidFindJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n_names) return;
    const uint64_t qa = J.name_off[k], qlen = J.name_off[k + 1] - qa;
    if (qlen >= kHidLaneEnd) return;                    // the wave kernel's (the host listed it)
    const uintptr_t qlo = (uintptr_t)J.names + qa, qhi = qlo + qlen;
    uint64_t h, found = kHidNotFound;
    uint32_t len;
    if (hid_hash_lane(qlo, qhi, 0, &h, &len) && len == qlen)      // (a shorter name: an isspace() byte inside the query)
        found = hid_probe_lane(J, qlo, qhi, nm_cut(h, J.hash_bits));
    J.first_out[k] = found;
}

__global__ __launch_bounds__(kNmThreads) void k_hid_find_long(const HidFindJob J, const uint32_t n_long)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t li = (uint64_t)blockIdx.x * (kNmThreads / 64) + (threadIdx.x >> 6);
    if (li >= n_long) return;                           // (the whole wave)
    const uint64_t k = J.long_list[li];
    const uint64_t qa = J.name_off[k], qlen = J.name_off[k + 1] - qa;
    const uintptr_t qlo = (uintptr_t)J.names + qa, qhi = qlo + qlen;
    const uintptr_t lo = (uintptr_t)J.bytes, hi = lo + J.n_bytes;
    uint64_t len, found = kHidNotFound;
    const uint64_t h = nm_cut(hid_hash_wave(qlo, qhi, 0, lane, &len), J.hash_bits);
    if (len == qlen) {                                  // (every lane takes the same way: the slot is the same word for all of them)
        const unsigned long long tag = h >> 32;
        uint64_t s = h & J.mask;
        for (uint64_t step = 0; step <= J.mask; step++) {
            const unsigned long long cur = J.table[s];
            if (cur == kHidEmpty) break;
            if ((cur >> 32) == tag) {
                const uint64_t owner = cur & 0xFFFFFFFFull;
                if (hid_same_name_wave(qlo, qhi, 0, len, lo, hi, J.rec_pos[owner] + 1, lane)) { found = owner; break; }
            }
            s = (s + 1) & J.mask;
        }
    }
    if (lane == 0) J.first_out[k] = found;
}

// k_hid_find for queries that were made on the device (crass_hip_fastx_names_find_device): nobody has seen their offsets, so the
// lane checks its pair — a decreasing pair or an end beyond n_name_bytes sets ctl[1], and that query reads nothing — and the
// queries of kHidLaneEnd bytes or more are listed here for k_hid_find_long: one add per wave (the ballot's first lane), every
// long lane stores behind the wave's base by its rank in the ballot.  The list's order depends on scheduling, no answer does.
__global__ __launch_bounds__(kNmThreads) void k_hid_find_dev(const HidFindJob J, const HidFindDev D)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool in = k < J.n_names;
    uint64_t qa = 0, qlen = 0;
    bool bad = false;
    if (in) {
        const uint64_t qb = J.name_off[k + 1];
        qa = J.name_off[k];
        bad = qb < qa || qb > D.n_name_bytes;
        qlen = bad ? 0 : qb - qa;
    }
    const bool is_long = in && qlen >= kHidLaneEnd;
    const unsigned long long m = __ballot(is_long);     // (no lane has left: the wave's 64 queries)
    if (m) {
        const int first = __builtin_ctzll(m);
        uint32_t base = 0;
        if (lane == (uint32_t)first) base = atomicAdd(&D.ctl[0], (uint32_t)__builtin_popcountll(m));
        base = (uint32_t)__shfl((int)base, first);
        if (is_long) D.long_app[base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint32_t)k;
    }
    if (!in || is_long) return;
    uint64_t h, found = kHidNotFound;
    uint32_t len;
    if (bad) D.ctl[1] = 1u;
    else {
        const uintptr_t qlo = (uintptr_t)J.names + qa, qhi = qlo + qlen;
        if (hid_hash_lane(qlo, qhi, 0, &h, &len) && len == qlen) found = hid_probe_lane(J, qlo, qhi, nm_cut(h, J.hash_bits));
    }
    J.first_out[k] = found;
}

// how many answers name a record: the one figure of them the host learns (one add per wave)
__global__ __launch_bounds__(kNmThreads) void k_hid_count_found(const uint64_t *first, const uint64_t n, unsigned long long *count)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    const unsigned long long m = __ballot(k < n && first[k] != kHidNotFound);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(count, (unsigned long long)__builtin_popcountll(m));
}

// ---- the names of listed records of a built table, back to back in device memory (crass_hip_fastx_names_of_device) ----
// k_nm_measure_idx: a lane per entry walks its record's name (nm_name_bytes, the rule of k_hl_measure).  The prefix sum of the
// lengths stays on the device, in three launches and without any block waiting for another: k_nm_scan_tiles sums kNmTile
// lengths per block, k_nm_scan_top turns the tile sums into the bytes in front of every tile (one block, 256 tiles a step, the
// total behind the last), k_nm_scan_apply writes every entry's offset and off[n].  k_nm_copy is k_hl_copy with the offsets and
// the records' numbers read from the device.
static constexpr uint32_t kNmTileItems = 4;                             // lengths per lane
static constexpr uint32_t kNmTile = kNmThreads * kNmTileItems;          // ... per block

__global__ __launch_bounds__(kNmThreads) void k_nm_measure_idx(const NmOfJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t g = J.idx[k];
    if (g < J.idx_base || g - J.idx_base >= J.n_reads) { *J.flag = 1u; J.len[k] = 0u; return; }
    const uintptr_t lo = (uintptr_t)J.bytes;
    NmCur c;
    c.init(lo, lo + J.n_bytes, J.rec_pos[g - J.idx_base] + 1);      // (rec_pos < n_bytes: the insert saw every one)
    uint64_t name = 0;
    for (;;) {
        uint32_t avail;
        const uint32_t w = c.next(&avail);
        const uint32_t nb = nm_name_bytes(w, avail);
        name += nb;
        if (nb < 4) break;
    }
    J.len[k] = name > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)name;
}

// the block's sum of v, in every lane (sh: one word per wave)
static __device__ __forceinline__ uint64_t nm_block_sum64(uint64_t v, uint64_t *sh)
{
    v = nm_wave_sum64(v);
    __syncthreads();                                    // (sh may still be read from the step before)
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t s = 0;
#pragma unroll
    for (int w = 0; w < kNmThreads / 64; w++) s += sh[w];
    return s;
}
// what the lanes in front of this one hold in v, summed (the exclusive prefix over the block); *total: the block's sum
static __device__ __forceinline__ uint64_t nm_block_prefix64(uint64_t v, uint64_t *sh, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t a = (uint32_t)__shfl_up((int)(uint32_t)inc, s), b = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), s);
        if (lane >= (uint32_t)s) inc += ((uint64_t)b << 32) | a;
    }
    __syncthreads();
    if (lane == 63u) sh[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kNmThreads / 64; w++) { const uint64_t s = sh[w]; if (w < wave) before += s; all += s; }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kNmThreads) void k_nm_scan_tiles(const NmOfJob J)
{
    __shared__ uint64_t sh[kNmThreads / 64];
    const uint64_t k0 = (uint64_t)blockIdx.x * kNmTile + (uint64_t)threadIdx.x * kNmTileItems;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kNmTileItems; j++) if (k0 + j < J.n) v += J.len[k0 + j];
    const uint64_t s = nm_block_sum64(v, sh);
    if (threadIdx.x == 0) J.tile_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kNmThreads) void k_nm_scan_top(const NmOfJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kNmThreads / 64];
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < n_tiles; t0 += kNmThreads) {      // (the same trip count in every lane)
        const uint64_t t = t0 + threadIdx.x;
        const uint64_t v = t < n_tiles ? J.tile_sum[t] : 0;
        uint64_t total;
        const uint64_t before = nm_block_prefix64(v, sh, &total);
        if (t < n_tiles) J.tile_sum[t] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) J.tile_sum[n_tiles] = carry;
}

__global__ __launch_bounds__(kNmThreads) void k_nm_scan_apply(const NmOfJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kNmThreads / 64];
    const uint64_t k0 = (uint64_t)blockIdx.x * kNmTile + (uint64_t)threadIdx.x * kNmTileItems;
    uint32_t l[kNmTileItems];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kNmTileItems; j++) { l[j] = k0 + j < J.n ? J.len[k0 + j] : 0u; v += l[j]; }
    uint64_t total;
    uint64_t at = J.tile_sum[blockIdx.x] + nm_block_prefix64(v, sh, &total);
#pragma unroll
    for (uint32_t j = 0; j < kNmTileItems; j++) { if (k0 + j < J.n) J.off[k0 + j] = at; at += l[j]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) J.off[J.n] = J.tile_sum[n_tiles];
}

__global__ __launch_bounds__(kNmThreads) void k_nm_copy(const NmOfJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.limit) return;
    uint64_t a = 0, b = J.n - 1;                        // the last entry whose offset is <= i, as in k_hl_copy
    while (a < b) {
        const uint64_t mid = (a + b + 1) >> 1;
        if (J.off[mid] <= i) a = mid; else b = mid - 1;
    }
    const uint64_t r = J.idx[a] - J.idx_base;           // (an entry out of range has no byte: the bisection never ends on one ...)
    if (r >= J.n_reads) return;                         // (... and this keeps a wrong offset array from reading rec_pos out of bounds)
    const uint64_t p = J.rec_pos[r] + 1 + (i - J.off[a]);
    if (p < J.n_bytes) J.out[i] = J.bytes[p];
}

__global__ __launch_bounds__(kNmThreads) void k_hl_measure(const HlJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uintptr_t lo = (uintptr_t)J.bytes;
    NmCur c;
    c.init(lo, lo + J.n_bytes, J.src[k]);
    uint64_t line = 0, name = 0;
    bool named = false;
    for (;;) {
        uint32_t avail;
        const uint32_t w = c.next(&avail);
        const uint32_t lb = nm_line_bytes(w, avail);
        if (!named) { const uint32_t nb = nm_name_bytes(w, avail); name += nb; named = nb < 4; }      // ('\n' is a space: nb <= lb)
        line += lb;
        if (lb < 4) break;
    }
    J.line_len[k] = line > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)line;
    J.name_len[k] = name > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)name;
}

__global__ __launch_bounds__(kNmThreads) void k_hl_copy(const HlJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.total) return;
    uint64_t a = 0, b = J.n - 1;                        // the last record whose offset is <= i (empty records in front of it share the offset)
    while (a < b) {
        const uint64_t mid = (a + b + 1) >> 1;
        if (J.off[mid] <= i) a = mid; else b = mid - 1;
    }
    const uint64_t p = J.src[a] + (i - J.off[a]);
    if (p < J.n_bytes) J.out[i] = J.bytes[p];
}

static __device__ __forceinline__ bool ql_is_graph(uint8_t b) { return b >= 33 && b <= 126; }

__global__ __launch_bounds__(kNmThreads) void k_ql_measure(const QlJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t p0 = J.src[k];
    const uint64_t end = J.lim[k] < J.n_bytes ? J.lim[k] : J.n_bytes;
    uint64_t start = p0;
    uint32_t len = 0, flags = 0;
    if (p0 < end && J.bytes[p0] == 0x40) {
        flags = 1u;
        uint64_t p = p0;
        for (uint32_t lines = 0; lines < 3 && p < end; p++) lines += J.bytes[p] == 0x0A ? 1u : 0u;      // behind the third line end
        start = p;
        bool gap = false, dense = true;
        for (; p < end; p++) {
            const uint8_t b = J.bytes[p];
            if (b == 0x0A) break;
            if (ql_is_graph(b)) { if (gap) dense = false; if (len != 0xFFFFFFFFu) len++; }
            else gap = true;
        }
        if (dense) flags |= 2u;
    }
    J.start[k] = start; J.len[k] = len; J.flags[k] = flags;
}

// the same for a record of the wrapped class (fastx_scan.h): behind the header line the sequence lines up to the first line that
// starts with '+', L their bytes 33..126; the quality is the first L bytes 33..126 behind the '+' line, over however many lines.
// On a four-line record the answer is k_ql_measure's.
__global__ __launch_bounds__(kNmThreads) void k_qw_measure(const QlJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t p0 = J.src[k];
    const uint64_t end = J.lim[k] < J.n_bytes ? J.lim[k] : J.n_bytes;
    uint64_t start = p0;
    uint32_t len = 0, flags = 0;
    if (p0 < end && J.bytes[p0] == 0x40) {
        flags = 1u;
        uint64_t p = p0, L = 0;
        while (p < end && J.bytes[p] != 0x0A) p++;      // the header line
        p++;
        while (p < end && J.bytes[p] != 0x2B) {         // sequence lines
            for (; p < end && J.bytes[p] != 0x0A; p++) L += ql_is_graph(J.bytes[p]) ? 1u : 0u;
            p++;
        }
        while (p < end && J.bytes[p] != 0x0A) p++;      // the '+' line
        p++;
        start = p < end ? p : end;
        bool gap = false, dense = true;
        for (p = start; p < end && len < L && len != 0xFFFFFFFFu; p++) {
            if (ql_is_graph(J.bytes[p])) { if (gap) dense = false; len++; }
            else gap = true;
        }
        if (dense) flags |= 2u;
    }
    J.start[k] = start; J.len[k] = len; J.flags[k] = flags;
}

// a lane per output byte; nothing is stored outside [out, out + total).  Wrapped records too (k_qw_measure): the walk to the
// k-th byte 33..126 goes over line ends up to the record's end
__global__ __launch_bounds__(kNmThreads) void k_ql_copy(const QlJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.total) return;
    uint64_t a = 0, b = J.n - 1;                        // the last record whose offset is <= i, as in k_hl_copy
    while (a < b) {
        const uint64_t mid = (a + b + 1) >> 1;
        if (J.off[mid] <= i) a = mid; else b = mid - 1;
    }
    const uint64_t k = i - J.off[a];
    const uint64_t end = J.lim[a] < J.n_bytes ? J.lim[a] : J.n_bytes;
    uint64_t p = J.start[a];
    if (J.flags[a] & 2u) p += k;
    else {                                              // the line's k-th byte in 33..126
        uint64_t seen = 0;
        for (; p < end; p++) if (ql_is_graph(J.bytes[p]) && seen++ == k) break;
    }
    if (p < end) J.out[i] = J.bytes[p];
}

// ---- the comment kseq hands on (fastx_scan.h: fx_own_comment, fx_comment_handed_from) ----
// where the name that starts at pos ends: the position of its first isspace() byte, or n_bytes (pos <= n_bytes)
static __device__ __forceinline__ uint64_t cm_name_end(uintptr_t lo, uint64_t n_bytes, uint64_t pos)
{
    NmCur c;
    c.init(lo, lo + n_bytes, pos);
    uint64_t name = 0;
    for (;;) {
        uint32_t avail;
        const uint32_t w = c.next(&avail);
        const uint32_t nb = nm_name_bytes(w, avail);
        name += nb;
        if (nb < 4) break;
    }
    return pos + name;
}

__global__ __launch_bounds__(kNmThreads) void k_cm_bits(const CmBuildJob J)
{
    const uint64_t r = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;      // (no lane leaves: the wave's 64 records are one word)
    bool own = false;
    if (r < J.n_reads) {
        const uint64_t pos = J.rec_pos[r];
        if (pos >= J.n_bytes) *J.flag = 1u;
        else {
            const uint64_t e = cm_name_end((uintptr_t)J.bytes, J.n_bytes, pos + 1);
            own = fx_own_comment(e, J.n_bytes, e < J.n_bytes ? J.bytes[e] : (uint8_t)0);
        }
    }
    const unsigned long long m = __ballot(own);
    if ((threadIdx.x & 63u) == 0 && r < J.n_reads) J.bits[r >> 6] = m;
}

static __device__ __forceinline__ uint64_t cm_wave_max64(uint64_t v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)(uint32_t)v, s), b = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s);
        const uint64_t o = ((uint64_t)b << 32) | a;
        v = o > v ? o : v;
    }
    return v;
}

// a wave per tile, a bitmap word per lane: 1 + the tile's last own-comment record (0: none) and how many it has
__global__ __launch_bounds__(kNmThreads) void k_cm_tiles(const CmBuildJob J, const uint64_t n_words, const uint64_t n_tiles)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * (kNmThreads / 64) + (threadIdx.x >> 6);
    if (t >= n_tiles) return;                           // (the whole wave)
    const uint64_t wi = t * (kFxCmTile / 64) + lane;
    const uint64_t v = wi < n_words ? J.bits[wi] : 0ull;
    const uint64_t last = cm_wave_max64(v ? wi * 64 + (63u - (uint32_t)__builtin_clzll(v)) + 1 : 0ull);
    const uint64_t cnt = nm_wave_sum64((uint64_t)__builtin_popcountll(v));
    if (lane == 0) { J.carry[t] = last; J.tile_cnt[t] = cnt; }
}

// one block, 256 tiles a step: carry[t] becomes the maximum over the tiles up to and including t, tile_cnt[n_tiles] the total
__global__ __launch_bounds__(kNmThreads) void k_cm_top(const CmBuildJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kNmThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t run = 0, cnt = 0;
    for (uint64_t t0 = 0; t0 < n_tiles; t0 += kNmThreads) {      // (the same trip count in every lane)
        const uint64_t t = t0 + threadIdx.x;
        uint64_t inc = t < n_tiles ? J.carry[t] : 0ull;
        cnt += t < n_tiles ? J.tile_cnt[t] : 0ull;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t a = (uint32_t)__shfl_up((int)(uint32_t)inc, s), b = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), s);
            const uint64_t o = ((uint64_t)b << 32) | a;
            if (lane >= (uint32_t)s && o > inc) inc = o;
        }
        __syncthreads();                                // (sh may still be read from the step before)
        if (lane == 63u) sh[wave] = inc;
        __syncthreads();
        uint64_t all = run;
#pragma unroll
        for (uint32_t w = 0; w < kNmThreads / 64; w++) { const uint64_t s = sh[w]; if (w < wave && s > inc) inc = s; if (s > all) all = s; }
        if (run > inc) inc = run;
        if (t < n_tiles) J.carry[t] = inc;
        run = all;
    }
    const uint64_t total = nm_block_sum64(cnt, sh);
    if (threadIdx.x == 0) J.tile_cnt[n_tiles] = total;
}

__global__ __launch_bounds__(kNmThreads) void k_cm_source(const CmFetchJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t r = J.idx[k];
    J.src[k] = r < J.n_reads ? fx_comment_handed_from(J.bits, J.carry, J.file_read_base, J.n_files, r) : kFxNone;
}

// pos[k]: the first byte behind the header character of entry k's source, kFxNone where nothing is handed
__global__ __launch_bounds__(kNmThreads) void k_cm_measure(const CmFetchJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t pos = J.pos[k];
    uint64_t start = 0, line = 0;
    if (pos <= J.n_bytes) {                             // (kFxNone is beyond every input)
        const uintptr_t lo = (uintptr_t)J.bytes;
        const uint64_t e = cm_name_end(lo, J.n_bytes, pos);
        if (fx_own_comment(e, J.n_bytes, e < J.n_bytes ? J.bytes[e] : (uint8_t)0)) {      // (so for every source: its bit says so)
            start = e + 1;
            NmCur c;
            c.init(lo, lo + J.n_bytes, start);
            for (;;) {
                uint32_t avail;
                const uint32_t w = c.next(&avail);
                const uint32_t lb = nm_line_bytes(w, avail);
                line += lb;
                if (lb < 4) break;
            }
        }
    }
    J.start[k] = start;
    J.len[k] = line > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)line;
}

__global__ __launch_bounds__(kNmThreads) void k_cm_copy(const CmFetchJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.total) return;
    uint64_t a = 0, b = J.n - 1;                        // the last entry whose offset is <= i, as in k_hl_copy
    while (a < b) {
        const uint64_t mid = (a + b + 1) >> 1;
        if (J.off[mid] <= i) a = mid; else b = mid - 1;
    }
    const uint64_t p = J.start[a] + (i - J.off[a]);
    if (p < J.n_bytes) J.out[i] = J.bytes[p];
}


uint32_t hid_lane_max() { return kHidLaneMax; }
uint32_t hid_lane_end() { return kHidLaneEnd; }

static bool nm_grid(uint64_t items, uint64_t per_block, unsigned *blocks)
{
    const uint64_t g = (items + per_block - 1) / per_block;
    if (!g || g > 0x7FFFFFFFull) return false;
    *blocks = (unsigned)g;
    return true;
}

hipError_t launch_hid_insert(const HidJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n_reads, kNmThreads, &g) || J.n_reads >= 0xFFFFFFFFull || J.mask + 1 < 2 * J.n_reads || (J.mask & (J.mask + 1))) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_insert, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_hid_insert_long(const HidJob &J, uint32_t n_long, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(n_long, kNmThreads / 64, &g) || n_long > J.n_reads) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_insert_long, dim3(g), dim3(kNmThreads), 0, st, J, n_long);
    return hipGetLastError();
}

hipError_t launch_hid_lookup(const HidJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n_reads, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_lookup, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_hid_find(const HidFindJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n_names, kNmThreads, &g) || (J.mask & (J.mask + 1))) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_find, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_hid_find_long(const HidFindJob &J, uint32_t n_long, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(n_long, kNmThreads / 64, &g) || n_long > J.n_names || (J.mask & (J.mask + 1))) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_find_long, dim3(g), dim3(kNmThreads), 0, st, J, n_long);
    return hipGetLastError();
}

hipError_t launch_hid_find_dev(const HidFindJob &J, const HidFindDev &D, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n_names, kNmThreads, &g) || J.n_names >= 0xFFFFFFFFull || (J.mask & (J.mask + 1)) || !D.long_app || !D.ctl) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_find_dev, dim3(g), dim3(kNmThreads), 0, st, J, D);
    return hipGetLastError();
}

hipError_t launch_hid_count_found(const uint64_t *first, uint64_t n, unsigned long long *count, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(n, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hid_count_found, dim3(g), dim3(kNmThreads), 0, st, first, n, count);
    return hipGetLastError();
}

uint32_t nm_scan_tile() { return kNmTile; }

hipError_t launch_nm_measure_idx(const NmOfJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_nm_measure_idx, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_nm_scan(const NmOfJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmTile, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_nm_scan_tiles, dim3(g), dim3(kNmThreads), 0, st, J);
    CRASS_LAUNCH(k_nm_scan_top, dim3(1), dim3(kNmThreads), 0, st, J, (uint64_t)g);
    CRASS_LAUNCH(k_nm_scan_apply, dim3(g), dim3(kNmThreads), 0, st, J, (uint64_t)g);
    return hipGetLastError();
}

hipError_t launch_nm_copy(const NmOfJob &J, hipStream_t st)
{
    unsigned g;
    if (!J.n || !nm_grid(J.limit, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_nm_copy, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_hl_measure(const HlJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hl_measure, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_hl_copy(const HlJob &J, hipStream_t st)
{
    unsigned g;
    if (!J.n || !nm_grid(J.total, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_hl_copy, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_ql_measure(const QlJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_ql_measure, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_qw_measure(const QlJob &J, hipStream_t st)
{
    unsigned blocks;
    if (!nm_grid(J.n, kNmThreads, &blocks)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_qw_measure, dim3(blocks), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_ql_copy(const QlJob &J, hipStream_t st)
{
    unsigned g;
    if (!J.n || !nm_grid(J.total, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_ql_copy, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_cm_build(const CmBuildJob &J, hipStream_t st)
{
    unsigned g, gt;
    const uint64_t n_words = (J.n_reads + 63) / 64, n_tiles = (J.n_reads + kFxCmTile - 1) / kFxCmTile;
    if (!nm_grid(J.n_reads, kNmThreads, &g) || !nm_grid(n_tiles, kNmThreads / 64, &gt) || !J.bits || !J.carry || !J.tile_cnt || !J.flag) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_cm_bits, dim3(g), dim3(kNmThreads), 0, st, J);
    CRASS_LAUNCH(k_cm_tiles, dim3(gt), dim3(kNmThreads), 0, st, J, n_words, n_tiles);
    CRASS_LAUNCH(k_cm_top, dim3(1), dim3(kNmThreads), 0, st, J, n_tiles);
    return hipGetLastError();
}

hipError_t launch_cm_source(const CmFetchJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmThreads, &g) || !J.n_files || !J.n_reads) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_cm_source, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_cm_measure(const CmFetchJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_cm_measure, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_cm_copy(const CmFetchJob &J, hipStream_t st)
{
    unsigned g;
    if (!J.n || !nm_grid(J.total, kNmThreads, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_cm_copy, dim3(g), dim3(kNmThreads), 0, st, J);
    return hipGetLastError();
}

} // namespace crass

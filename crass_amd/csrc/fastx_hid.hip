// fastx_hid.hip — the name table of a FASTA / FASTQ file's raw bytes on the device, for a caller whose bytes exist only in HBM:
// header_id (the index of the first read with the same NAME: readsFound's key, libcrispr.cpp:138,411) and names in, first index
// out.  The restatement both are tested against is the host's crass_fastx_header_ids / crass_fastx_find_names (fastx_scan.cpp)
// and kseq's name cut.  What a name is and how its bytes are read: fastx_walk.h.
//
// An open-addressing table of 2^k >= 2 n_reads slots of 64 bits, {hash tag : 32 | read index : 32}, all-ones = free:
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
//   k_hid_find         names in, first index out, on a table that is kept (crass_hip_fastx_names_build_device): a lane per query.  The
//                      query is a name that ends with its own bytes: it is hashed by the function k_hid_insert hashes with
//                      (hid_hash_lane), then probed for linearly from the hash's slot — free slot: not found; other tag: next slot;
//                      same tag: the query against the slot owner's name, lengths included; equal: the slot's index.  The table is
//                      final and only read: no atomics, no waiting, and a probe that has seen every slot ends with not found.
//   k_hid_find_long    a wave per query of kHidLaneEnd bytes or more, hashed as k_hid_insert_long hashes (hid_hash_wave).
//   k_hid_find_dev     k_hid_find for queries made on the device (another rank's names): it checks the offsets nobody on the host
//                      has seen and lists the long queries itself, one add per wave; k_hid_find_long then runs over that list.
//   k_hid_count_found  how many answers name a record.
// No answer rests on a hash: hash_bits (CRASS_HID_TEST_HASH_BITS) cuts the hash to its low bits, down to none, for the tests.
// Slot accesses are agent-scope atomics; the name bytes and rec_pos are read-only input.
#include "fastx_walk.h"
#include "fastx_vec.h"

namespace crass {

static constexpr uint32_t kHidLaneMax = 256;             // names beyond this many bytes go to the wave kernel
static constexpr uint32_t kHidLaneEnd = kHidLaneMax + 4; // ... seen a dword at a time: names of this many bytes or more are the wave kernels'

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
    return nm_fmix(fx_wave_sum64(acc) ^ len);
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

// the probe for a query of hash h (cut already): every step ends the loop or moves on a slot, mask + 1 steps at most.  same(owner):
// is the query the name of that record?
template <class Same> static __device__ __forceinline__ uint64_t hid_probe(const HidFindJob &J, uint64_t h, Same same)
{
    const unsigned long long tag = h >> 32;
    uint64_t s = h & J.mask;
    for (uint64_t step = 0; step <= J.mask; step++) {
        const unsigned long long cur = J.table[s];
        if (cur == kHidEmpty) break;
        if ((cur >> 32) == tag) {
            const uint64_t owner = cur & 0xFFFFFFFFull;
            if (same(owner)) return owner;
        }
        s = (s + 1) & J.mask;
    }
    return kHidNotFound;
}
// ... of one lane, for the query [qlo, qhi)
static __device__ __forceinline__ uint64_t hid_probe_lane(const HidFindJob &J, uintptr_t qlo, uintptr_t qhi, uint64_t h)
{
    const uintptr_t lo = (uintptr_t)J.bytes, hi = lo + J.n_bytes;
    return hid_probe(J, h, [&](uint64_t owner) { return hid_same_name_lane(qlo, qhi, 0, lo, hi, J.rec_pos[owner] + 1); });
}
// ... of a wave, for the query of len bytes (every lane takes the same way: the slot is the same word for all of them)
static __device__ __forceinline__ uint64_t hid_probe_wave(const HidFindJob &J, uintptr_t qlo, uintptr_t qhi, uint64_t len, uint64_t h, uint32_t lane)
{
    const uintptr_t lo = (uintptr_t)J.bytes, hi = lo + J.n_bytes;
    return hid_probe(J, h, [&](uint64_t owner) { return hid_same_name_wave(qlo, qhi, 0, len, lo, hi, J.rec_pos[owner] + 1, lane); });
}

// one lane's answer to the query of qlen < kHidLaneEnd bytes at qlo: hashed, its length checked (a shorter name: an isspace() byte
// inside the query), probed for
static __device__ __forceinline__ uint64_t hid_find_lane(const HidFindJob &J, uintptr_t qlo, uint64_t qlen)
{
    uint64_t h;
    uint32_t len;
    if (!hid_hash_lane(qlo, qlo + qlen, 0, &h, &len) || len != qlen) return kHidNotFound;
    return hid_probe_lane(J, qlo, qlo + qlen, nm_cut(h, J.hash_bits));
}

__global__ __launch_bounds__(kNmThreads) void k_hid_find(const HidFindJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n_names) return;
    const uint64_t qa = J.name_off[k], qlen = J.name_off[k + 1] - qa;
    if (qlen >= kHidLaneEnd) return;                    // the wave kernel's (the host listed it)
    J.first_out[k] = hid_find_lane(J, (uintptr_t)J.names + qa, qlen);
}

__global__ __launch_bounds__(kNmThreads) void k_hid_find_long(const HidFindJob J, const uint32_t n_long)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t li = (uint64_t)blockIdx.x * (kNmThreads / 64) + (threadIdx.x >> 6);
    if (li >= n_long) return;                           // (the whole wave)
    const uint64_t k = J.long_list[li];
    const uint64_t qa = J.name_off[k], qlen = J.name_off[k + 1] - qa;
    const uintptr_t qlo = (uintptr_t)J.names + qa, qhi = qlo + qlen;
    uint64_t len, found = kHidNotFound;
    const uint64_t h = nm_cut(hid_hash_wave(qlo, qhi, 0, lane, &len), J.hash_bits);
    if (len == qlen) found = hid_probe_wave(J, qlo, qhi, len, h, lane);
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
    if (bad) D.ctl[1] = 1u;
    J.first_out[k] = bad ? kHidNotFound : hid_find_lane(J, (uintptr_t)J.names + qa, qlen);
}

// how many answers name a record: the one figure of them the host learns (one add per wave)
__global__ __launch_bounds__(kNmThreads) void k_hid_count_found(const uint64_t *first, const uint64_t n, unsigned long long *count)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    const unsigned long long m = __ballot(k < n && first[k] != kHidNotFound);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(count, (unsigned long long)__builtin_popcountll(m));
}

// ---- host: the launches, each behind its own checks ----
uint32_t hid_lane_max() { return kHidLaneMax; }
uint32_t hid_lane_end() { return kHidLaneEnd; }

hipError_t launch_hid_insert(const HidJob &J, hipStream_t st)
{
    if (J.n_reads >= 0xFFFFFFFFull || J.mask + 1 < 2 * J.n_reads || (J.mask & (J.mask + 1))) return hipErrorInvalidValue;
    return NM_LAUNCH(k_hid_insert, J.n_reads, kNmThreads, st, J);
}

hipError_t launch_hid_insert_long(const HidJob &J, uint32_t n_long, hipStream_t st)
{
    if (n_long > J.n_reads) return hipErrorInvalidValue;
    return NM_LAUNCH(k_hid_insert_long, n_long, kNmThreads / 64, st, J, n_long);
}

hipError_t launch_hid_lookup(const HidJob &J, hipStream_t st) { return NM_LAUNCH(k_hid_lookup, J.n_reads, kNmThreads, st, J); }

hipError_t launch_hid_find(const HidFindJob &J, hipStream_t st)
{
    if (J.mask & (J.mask + 1)) return hipErrorInvalidValue;
    return NM_LAUNCH(k_hid_find, J.n_names, kNmThreads, st, J);
}

hipError_t launch_hid_find_long(const HidFindJob &J, uint32_t n_long, hipStream_t st)
{
    if (n_long > J.n_names || (J.mask & (J.mask + 1))) return hipErrorInvalidValue;
    return NM_LAUNCH(k_hid_find_long, n_long, kNmThreads / 64, st, J, n_long);
}

hipError_t launch_hid_find_dev(const HidFindJob &J, const HidFindDev &D, hipStream_t st)
{
    if (J.n_names >= 0xFFFFFFFFull || (J.mask & (J.mask + 1)) || !D.long_app || !D.ctl) return hipErrorInvalidValue;
    return NM_LAUNCH(k_hid_find_dev, J.n_names, kNmThreads, st, J, D);
}

hipError_t launch_hid_count_found(const uint64_t *first, uint64_t n, unsigned long long *count, hipStream_t st)
{
    return NM_LAUNCH(k_hid_count_found, n, kNmThreads, st, first, n, count);
}

} // namespace crass

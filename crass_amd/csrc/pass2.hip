// pass2.hip — pass 2 on gfx950: findSingletons / on_match (src/crass/libcrispr.cpp:399-518, src/aho-corasick/acism.c:25-106;
// citations are relative to the crass v1.0.1 tree).  The automaton kernels, the anchor probe that flags the reads worth
// scanning, and k_recruit_finish (on_match + DRLowLexi of the recruited repeat).  The hits are packed by sinks.hip.
#include "dev_common.h"
#include "comp_table.h"
#include <type_traits>
#include <utility>

namespace crass {

static __constant__ CompTable c_comp = make_comp_table();     // reverseComplement table, SeqUtils.cpp:50-59

// ------------------------------------------------------------------------------------
// pass 2: first-match multi-pattern scan (findSingletons/on_match semantics: the first ACISM
// callback = occurrence with the smallest end position, ties -> longest pattern;
// libcrispr.cpp:441, acism.c:73-102).  Lane per read, 64 consecutive reads per wave so the
// ballot is the mask word.  hit_info[r] = (end_exclusive << 8) | pattern_length.
// ------------------------------------------------------------------------------------
template <bool LDS_TABLE, int THREADS>
__global__ __launch_bounds__(THREADS) void k_recruit(DevReads R, DevAutomaton A, const uint8_t *found_flag,
                                                 uint64_t *hitmask, uint32_t *hit_info)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t rc_lds[];
    const uint16_t *go4 = A.go4;
    const uint16_t *outl = A.out_len;
    if (LDS_TABLE) {
        // stage [n_states][4] transitions + out_len in LDS
        uint16_t *l_go = rc_lds;
        uint16_t *l_out = rc_lds + (size_t)A.n_states * 4;
        for (uint32_t i = threadIdx.x; i < A.n_states * 4; i += blockDim.x) l_go[i] = A.go4[i];
        for (uint32_t i = threadIdx.x; i < A.n_states; i += blockDim.x) l_out[i] = A.out_len[i];
        __syncthreads();
        go4 = l_go; outl = l_out;
    }
    const uint64_t n_tiles = (R.n_reads + 63) / 64;
    const int lane = threadIdx.x & 63;
    const uint64_t wave_global = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t wave_total = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t tile = wave_global; tile < n_tiles; tile += wave_total) {
        const uint64_t r = tile * 64 + lane;
        bool hit = false;
        if (r < R.n_reads && !rd_is_exc(R, r) && !found_flag[rd_header_id(R, r)]) {
            const uint32_t L = rd_len(R, r);
            const uint32_t *g = R.packed + rd_word_off(R, r);
            uint32_t state = 0;
            uint32_t word = 0;
            for (uint32_t i = 0; i < L; i++) {
                if ((i & 15u) == 0) word = g[i >> 4];
                uint32_t c = word & 3u;
                word >>= 2;
                state = go4[state * 4 + c];
                uint32_t ol = outl[state];
                if (ol) { hit_info[r] = ((i + 1) << 8) | ol; hit = true; break; }
            }
        }
        uint64_t m = __ballot(hit);
        if (lane == 0) hitmask[tile] = m;
    }
}

// generic transition tables (any symbol count / state count), global memory
__global__ __launch_bounds__(256) void k_recruit_wide(DevReads R, DevAutomaton A, const uint8_t *found_flag,
                                                       uint64_t *hitmask, uint32_t *hit_info)
{
    const uint64_t n_tiles = (R.n_reads + 63) / 64;
    const int lane = threadIdx.x & 63;
    const uint64_t wave_global = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t wave_total = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t symA = A.sym['A'], symC = A.sym['C'], symG = A.sym['G'], symT = A.sym['T'];
    for (uint64_t tile = wave_global; tile < n_tiles; tile += wave_total) {
        const uint64_t r = tile * 64 + lane;
        bool hit = false;
        if (r < R.n_reads && !rd_is_exc(R, r) && !found_flag[rd_header_id(R, r)]) {
            const uint32_t L = rd_len(R, r);
            const uint32_t *g = R.packed + rd_word_off(R, r);
            uint32_t state = 0, word = 0;
            for (uint32_t i = 0; i < L; i++) {
                if ((i & 15u) == 0) word = g[i >> 4];
                uint32_t c = word & 3u;
                word >>= 2;
                uint32_t sy = c == 0 ? symA : c == 1 ? symC : c == 2 ? symG : symT;
                state = A.go16 ? (uint32_t)A.go16[(size_t)state * A.n_sym1 + sy] : A.go32[(size_t)state * A.n_sym1 + sy];
                uint32_t ol = A.out_len[state];
                if (ol) { hit_info[r] = ((i + 1) << 8) | ol; hit = true; break; }
            }
        }
        uint64_t m = __ballot(hit);
        if (lane == 0) hitmask[tile] = m;
    }
}

hipError_t launch_recruit_general(const DevReads &R, const DevAutomaton &A, const uint8_t *found_flag,
                                  uint64_t *hitmask, uint32_t *hit_info, hipStream_t st)
{
    if (R.n_reads == 0) return hipSuccess;
    uint64_t n_tiles = (R.n_reads + 63) / 64;
    uint64_t blocks = (n_tiles + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (A.acgt_ok && A.go4)
        CRASS_LAUNCH((k_recruit<false, 256>), dim3((unsigned)blocks), dim3(256), 0, st, R, A, found_flag, hitmask, hit_info);
    else
        CRASS_LAUNCH(k_recruit_wide, dim3((unsigned)blocks), dim3(256), 0, st, R, A, found_flag, hitmask, hit_info);
    return hipGetLastError();
}

hipError_t launch_recruit_lds(const DevReads &R, const DevAutomaton &A, const uint8_t *found_flag,
                              uint64_t *hitmask, uint32_t *hit_info, hipStream_t st)
{
    if (R.n_reads == 0) return hipSuccess;
    if (!A.acgt_ok || !A.go4) return hipErrorNotSupported;
    size_t lds = (size_t)A.n_states * 10;       // 4 x u16 transitions + u16 out_len
    if (lds > 160 * 1024) return hipErrorNotSupported;
    uint64_t n_tiles = (R.n_reads + 63) / 64;
    // one workgroup per CU-slot; the LDS footprint decides how many fit, so size the block to fill the CU
    const int threads = lds > 80 * 1024 ? 1024 : (lds > 40 * 1024 ? 512 : 256);
    uint64_t waves_per_block = threads / 64;
    uint64_t blocks = (n_tiles + waves_per_block - 1) / waves_per_block;
    uint64_t cap = lds > 80 * 1024 ? 256 : (lds > 40 * 1024 ? 512 : (lds > 20 * 1024 ? 1024 : 2048));
    if (blocks > cap) blocks = cap;
    hipError_t e;
#define RC_LAUNCH(T)                                                                                                   \
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_recruit<true, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return e;                                                                                     \
    CRASS_LAUNCH((k_recruit<true, T>), dim3((unsigned)blocks), dim3(T), lds, st, R, A, found_flag, hitmask, hit_info);
    if (threads == 1024) { RC_LAUNCH(1024) }
    else if (threads == 512) { RC_LAUNCH(512) }
    else { RC_LAUNCH(256) }
#undef RC_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// pass 2 fast path: anchor filter + exact verification of the flagged reads.
//
// Every pattern has length >= 23.  If pattern P occurs at offset o of a read, let a be the
// smallest multiple of 8 with a >= o (a <= o+7): bases [a, a+16) lie inside the occurrence
// (a+16 <= o+23 <= o+|P|) and equal P[a-o .. a-o+16).  So the halfword-aligned 32-bit window
// of the read at base a is one of the keys {P[r..r+16) : r = 0..7}.  The filter probes every
// aligned window (ceil(L/8)-1 per read, all independent) in an exact LDS hash set of the keys:
// no false negatives by construction; the rare false positives (a key occurring by chance,
// ~n_keys * L/8 / 4^16) are removed by the exact automaton scan of the flagged reads
// (k_recruit_list), which also yields ACISM's first-callback (end, length).
// ------------------------------------------------------------------------------------
// One probe for every table form.  `lds` is the staged table (MODE 2: the table in global memory itself).
// MODE 0: exact keys in LDS, 1: buckets of two 16-bit fingerprints in LDS, 2: exact keys in global memory; 3 and 4: see there
template <int MODE>
static __device__ __forceinline__ bool anchor_probe_any(const uint32_t *lds, uint32_t V, const DevAnchors &K, uint32_t rshift)
{
    if constexpr (MODE == 4) {
        // MODE 4 (device-built tables beyond the LDS tiers): 2^20-bit Bloom filter in LDS, exact keys in global memory
        const uint32_t h1 = ak_hash(V, K.m1);
        const uint32_t wd = lds[ak_bloom_word(h1)];
        bool hit = false;
        if (((wd >> ((h1 >> 12) & 31u)) & (wd >> ((h1 >> 7) & 31u)) & 1u) != 0u)          // ~7 % of the probes at 150 k keys
            hit = (K.table[h1 >> rshift] == V) | (K.table[ak_hash(V, K.m2) >> rshift] == V);
        return hit;
    } else if constexpr (MODE == 3) {
        // MODE 3 (device-built tables): 2^16 slots, 16 bits per slot in LDS — the OTHER slot index of the key that sits there
        // (partial-key cuckoo: slot h1(K) stores h2(K) and the other way round), so a window matches when one of its two slots
        // names the other.  Sixteen bits that depend on every base of the key through an independent hash; the low halfword of
        // h1 ^ h2 — the first form — only depends on the key's first eight bases, which the hundreds of variants of one repeat
        // share: every read carrying a near-copy of a repeat then met that value in ~30 slots instead of one (k_dm_verify
        // 364 -> 464 us at 100 M reads, profiles/NOTES_r03.md).
        const uint16_t *tab = reinterpret_cast<const uint16_t *>(lds);
        const uint32_t i1 = ak_hash(V, K.m1) >> 16, i2 = ak_hash(V, K.m2) >> 16;
        const uint32_t a = tab[i1], b = tab[i2];
        return (a == i2) | (b == i1);
    } else {
        const uint32_t h1 = ak_hash(V, K.m1);
        const uint32_t h2 = ak_hash(V, K.m2);
        const uint32_t a = lds[h1 >> rshift], b = lds[h2 >> rshift];   // both probes always issued: independent reads, no branches
        if (MODE == 1) {
            // fingerprint = HIGH halfword of h1 ^ h2 (the bits that depend on every base of the key; the low halfword only
            // sees the first eight, see MODE 3), replicated into both halves
            const uint32_t hx = h1 ^ h2;
            const uint32_t ff = __builtin_amdgcn_perm(hx, hx, 0x03020302u);
            // a halfword of (slot ^ ff) is zero <=> that fingerprint matches; min(x, 1) per halfword keeps 1 unless zero
            const uint32_t t = pk_min_u16(a ^ ff, 0x00010001u) & pk_min_u16(b ^ ff, 0x00010001u);
            return t != 0x00010001u;
        }
        return (a == V) | (b == V);
    }
}

// ASH: log2 of the windows' alignment — 3: every 8 bases (halfword positions; patterns of >= 23 bases), 2: every 4 bases (byte
// positions; patterns of 15 .. 22 bases, `-d 15` .. `-d 22`: twice the windows per read, see kDevMinDR)
// KL: bases per key — 16, or 12 (patterns of 15 .. 18 bases): the window's value is cut to 24 bits before it is hashed and
// compared (one v_and_b32, the one ak_hash needs anyway: its top-byte term is then zero), and a window only needs KL bases
// inside the read, so a read has one more of them at its end
template <int W, int THREADS, int MODE, int ASH = 3, int KL = 16>     // W = uniform stride in words (0: ragged / any stride)
static __device__ __forceinline__ void anchor_filter_body(const DevReads &R, const DevAnchors &K, const uint32_t *ak_lds,
                                                          const uint8_t *found_flag, uint64_t *hitmask)
{
    constexpr uint32_t PW = 16u >> ASH;              // windows per packed word (2 or 4)
    constexpr uint32_t WB = 32u / PW;                // bits between two windows (16 or 8)
    constexpr uint32_t KMASK = KL >= 16 ? 0xFFFFFFFFu : (1u << (2 * KL)) - 1u;
    constexpr int NWIN = W > 0 ? (16 * W - KL) / (1 << ASH) + 1 : 0;      // windows of a row of W words
    static_assert(KL == 16 || (KL == 12 && ASH == 2), "anchor key shapes: engine_internal.h, kDevMinDR");
    auto cut = [](uint32_t V) { return KL >= 16 ? V : (V & KMASK); };
    const uint32_t mask = 32u - K.log_size;          // right shift that keeps the top log_size bits
    const uint64_t n_tiles = (R.n_reads + 63) / 64;
    const int lane = threadIdx.x & 63;
    const uint64_t wave_global = (blockIdx.x * (uint64_t)THREADS + threadIdx.x) >> 6;
    const uint64_t wave_total = ((uint64_t)gridDim.x * THREADS) >> 6;
    if (W == 0 && R.wave_walk) {
        // long reads: a lane walking its own 10 kbp read
        // touches one word per 2.5 KB row, 258 GB/s; here the WAVE walks one read, lane = window, so the loads are
        // consecutive words, and a tile's 64 reads are taken one after the other (bit k of the mask word = read k)
        for (uint64_t tile = wave_global; tile < n_tiles; tile += wave_total) {
            uint64_t bits = 0;
            for (int k = 0; k < 64; k++) {
                const uint64_t r = tile * 64 + (uint64_t)k;                     // wave-uniform
                if (r >= R.n_reads) break;
                if (!(K.with_exc || !rd_is_exc(R, r)) || found_flag[rd_header_id(R, r)]) continue;
                const uint32_t L = rd_len(R, r);
                if (L < (uint32_t)KL) continue;
                const uint32_t *g = R.packed + rd_word_off(R, r);
                const uint32_t nw = (L + 15) >> 4, h_max = (L - (uint32_t)KL) >> ASH;
                // a lane takes FOUR consecutive windows (halfword positions 4q .. 4q+3 = words 2q, 2q+1 and the low half of
                // 2q+2): three loads serve four probes, one ballot decides 256 windows, and the words of the next round are
                // requested before this round is probed (one window per lane and round was 20 dependent round trips per
                // 10 kbp read: 3.3 ms for 1 M reads)
                auto fetch3 = [&](uint32_t q, uint32_t &a, uint32_t &b, uint32_t &c3) {
                    const uint32_t w0 = 2u * q;
                    a = w0 < nw ? g[w0] : 0u; b = w0 + 1u < nw ? g[w0 + 1u] : 0u; c3 = w0 + 2u < nw ? g[w0 + 2u] : 0u;
                };
                uint32_t na, nb, nc;
                fetch3((uint32_t)lane, na, nb, nc);
                // (windows every 4 bases: the same three words serve EIGHT probes per lane)
                constexpr uint32_t PL = 2u * PW;                                // windows per lane and round
                for (uint32_t h0 = 0; h0 <= h_max; h0 += 64u * PL) {
                    const uint32_t q = (h0 / PL) + (uint32_t)lane;
                    const uint32_t a = na, b = nb, c3 = nc;
                    if (h0 + 64u * PL <= h_max) fetch3(q + 64u, na, nb, nc);
                    const uint32_t h = PL * q;
                    bool f = false;
#pragma unroll
                    for (uint32_t i = 0; i < PL; i++) {
                        const uint32_t V = i < PW ? __builtin_amdgcn_alignbit(b, a, (i * WB) & 31u) : __builtin_amdgcn_alignbit(c3, b, ((i - PW) * WB) & 31u);
                        if (h + i <= h_max) f = f | anchor_probe_any<MODE>(ak_lds, cut(V), K, mask);
                    }
                    if (__ballot(f)) { bits |= 1ull << k; break; }              // one window is enough to flag the read
                }
            }
            if (lane == 0) hitmask[tile] = bits;
        }
        return;
    }
    if constexpr (W > 0) {
        // Uniform stride, a software pipeline one tile deep: EVERYTHING a tile's turn reads from global memory — the rows, the
        // found flag, the read's length (padded ragged sets) and its exception word (host-built tables) — is requested one
        // turn earlier, in one place, and carried in registers; where header ids exist a tile's ids are requested TWO turns
        // earlier, so that the flag's address is in a register when the flag is requested.  A turn then waits once, at its
        // top, for what the turn before it asked for, and asks for nothing it needs itself: between the requests and the next
        // top lie the tile's 2W-1 hashes and LDS probes.  (Until round 17 only the rows were requested ahead and the flag
        // was loaded — behind a wait that, vmcnt retiring in order, also covered the rows just requested — in front of the
        // probes: two serial HBM round trips per wave and tile, two thirds of the wave's time parked, NOTES r17.)
        // The loads are unconditional, from an index clamped to the last read, not loads under a lane predicate: behind the
        // join of a divergent branch the compiler's wait for an OLDER load comes out as vmcnt(0).  A clamped lane's values are
        // never used (r < n_reads is tested where they would be).  found_flag is read a tile early: nothing writes it while
        // the probe runs — the scan that cleared it and the kernels that set it are complete before the probe is launched,
        // and pass 2's own recruits are marked by a later kernel.  The mask word of a tile is stored in the NEXT turn, behind
        // that turn's requests: stored at the end of its own turn (or in front of the requests) the store is the newest
        // vector-memory operation when the wait comes, and the wave sits out the store's round trip instead.
        // (MODE 2 and 4 probe keys in global memory inside the turn; those loads wait where they are used, as before.)
        const uint64_t wave0 = uni64(wave_global), wave_step = uni64(wave_total);
        const uint64_t r_last = R.n_reads - 1;
        const bool ids = R.header_id != nullptr;         // (wave-uniform like uniform_len and with_exc: scalar branches)
        uint32_t pre[W], pre_len = 0, pre_exc = 0;
        uint32_t pre_found = 0;
        uint64_t pre_id = 0;                             // header ids of the tile BEHIND the one in pre[]
        auto clamped = [&](uint64_t tile) { const uint64_t rr = tile * 64 + lane; return rr < r_last ? rr : r_last; };
        auto request_ids = [&](uint64_t tile) { if (ids) pre_id = R.header_id[clamped(tile)]; };
        auto request = [&](uint64_t tile, uint64_t id) {
            const uint64_t rc = clamped(tile);
            const uint32_t *gp = R.packed + rc * (uint64_t)W;
#pragma unroll
            for (int i = 0; i < W; i++) pre[i] = gp[i];
            pre_found = found_flag[ids ? id : rc];
            if (!R.uniform_len) pre_len = R.lengths[rc];
            if (!K.with_exc) pre_exc = R.exc_mask[rc >> 5];
        };
        request_ids(wave0);
        const uint64_t id0 = pre_id;
        request_ids(wave0 + wave_step);
        request(wave0, id0);                             // (with header ids the one dependent round trip of a wave's life)
        uint64_t m_done = 0, tile_done = 0;
        bool have_done = false;
        for (uint64_t tile = wave0; tile < n_tiles; tile += wave_step) {
            const uint64_t r = tile * 64 + lane;
            uint32_t w[W + 1];
#pragma unroll
            for (int i = 0; i < W; i++) w[i] = pre[i];
            w[W] = 0;
            const uint32_t found = pre_found, L = R.uniform_len ? R.uniform_len : pre_len, excw = pre_exc;
            const uint64_t id_next = pre_id;
            request(tile + wave_step, id_next);
            request_ids(tile + 2 * wave_step);
            if (have_done && lane == 0) hitmask[tile_done] = m_done;
            bool flag = false;
            // with_exc: every pattern is pure ACGT, so an occurrence in an exception read lies in a stretch whose packed
            // codes are the real bases — the probe stays a superset filter; the verification checks the bytes
            if (r < R.n_reads && (K.with_exc || !((excw >> (r & 31)) & 1u)) && !found && L >= (uint32_t)KL) {
                const uint32_t h_max = (L - (uint32_t)KL) >> ASH;          // last window position (halfword, or byte) whose 16-mer is inside the read
                if (MODE == 4) {
                    // Bloom filter in LDS, exact keys in global memory.  ~7 % of the windows pass the Bloom filter, i.e.
                    // in nearly every one of the 2W-1 unrolled windows SOME lane of the wave does, and a conditional
                    // pair of global loads per window made the wave wait for 19 round trips.  So: all Bloom tests
                    // first (LDS only, a bit per window), then every lane resolves ITS positives one per round —
                    // the wave needs as many rounds as its busiest lane has positives (4-5).
                    typedef typename std::conditional<ASH == 3, uint32_t, uint64_t>::type pm_t;      // (up to 61 windows every 4 bases)
                    pm_t pm = 0;
#pragma unroll
                    for (int h = 0; h < NWIN; h++) {
                        const uint32_t V = cut(__builtin_amdgcn_alignbit(w[h / (int)PW + 1], w[h / (int)PW], ((uint32_t)h % PW) * WB));
                        // (blocked Bloom: ONE hash, one LDS word, both bits from it; a shift by a register takes the register's low
                        // five bits, so the two positions cost a shift each and the window's flag joins pm with one v_lshl_or)
                        const uint32_t h1 = ak_hash(V, K.m1);
                        const uint32_t wd = ak_lds[ak_bloom_word(h1)];
                        const uint32_t bit = (wd >> ((h1 >> 12) & 31u)) & (wd >> ((h1 >> 7) & 31u)) & 1u;
                        if ((uint32_t)h <= h_max) pm |= (pm_t)bit << h;
                    }
                    while (pm) {                                   // (divergent: lanes with fewer positives idle)
                        const uint32_t h = (uint32_t)(ASH == 3 ? __ffs((int)(uint32_t)pm) : __ffsll((unsigned long long)pm)) - 1u;
                        pm &= pm - 1u;
                        const uint32_t kk = h / PW;
                        uint32_t lo = 0, hi = 0;
#pragma unroll
                        for (int i = 0; i < W; i++) { lo = kk == (uint32_t)i ? w[i] : lo; hi = kk == (uint32_t)i ? w[i + 1] : hi; }
                        const uint32_t V = cut(__builtin_amdgcn_alignbit(hi, lo, (h % PW) * WB));
                        const uint32_t h1 = ak_hash(V, K.m1), h2 = ak_hash(V, K.m2);
                        if ((K.table[h1 >> mask] == V) | (K.table[h2 >> mask] == V)) { flag = true; pm = 0; }
                    }
                } else {
                    // Uniform read length: the last window hm is a scalar.  A read that needs all W words of its row has more
                    // than 16 (W-1) bases, so windows up to HS lie inside it whatever its length and "inside the read" is a
                    // scalar condition on the result, no vector compare; the few windows behind HS (two of 19 at 150 bases and
                    // W = 10) are hashed and probed only where hm reaches them — a scalar branch each.  (A uniform length
                    // shorter than that — a padded stride — masks the early windows and skips the late ones: still exact.)
                    // Per-read lengths keep the vector mask.
                    auto scan = [&](const uint32_t hm, auto uniform_c) {
                        constexpr int HS = decltype(uniform_c)::value ? (int)((16u * (uint32_t)(W - 1) + 1u - (uint32_t)KL) >> ASH) : NWIN - 1;
#pragma unroll
                        for (int h = 0; h < NWIN; h++) {
                            auto probe = [&]() {
                                const uint32_t V = cut(__builtin_amdgcn_alignbit(w[h / (int)PW + 1], w[h / (int)PW], ((uint32_t)h % PW) * WB));
                                return anchor_probe_any<MODE>(ak_lds, V, K, mask);
                            };
                            if (h > HS) { if ((uint32_t)h <= hm) flag = flag | probe(); }
                            else flag = flag | (probe() & ((uint32_t)h <= hm));
                            // (16 LDS reads in flight are plenty; left alone the scheduler hoists all 4W-2 of them and, from
                            // W = 12, spills)
                            if ((h & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                        }
                    };
                    if (R.uniform_len) scan((R.uniform_len - (uint32_t)KL) >> ASH, std::true_type{});
                    else scan(h_max, std::false_type{});
                }
            }
            m_done = __ballot(flag); tile_done = tile; have_done = true;
        }
        if (have_done && lane == 0) hitmask[tile_done] = m_done;
        return;
    }
    // any stride, lane per read
    for (uint64_t tile = wave_global; tile < n_tiles; tile += wave_total) {
        const uint64_t r = tile * 64 + lane;
        bool flag = false;
        if (r < R.n_reads && (K.with_exc || !rd_is_exc(R, r)) && !found_flag[rd_header_id(R, r)]) {
            const uint32_t L = rd_len(R, r);
            const uint32_t *g = R.packed + rd_word_off(R, r);
            if (L >= (uint32_t)KL) {
                const uint32_t h_max = (L - (uint32_t)KL) >> ASH;          // last window position (halfword, or byte) whose 16-mer is inside the read
                // (four words per round, requested together: one word per round was one dependent round trip per 16 bases — reads of
                // 300 .. 800 bases, lane per read, took twice the time of the register form per base)
                const uint32_t nw = (L + 15) >> 4;
                uint32_t lo = g[0];
                for (uint32_t h = 0; h <= h_max && !flag; h += 4u * PW) {
                    const uint32_t wi = (h / PW) + 1;
                    uint32_t x[4];
#pragma unroll
                    for (uint32_t q = 0; q < 4; q++) x[q] = wi + q < nw ? g[wi + q] : 0u;
#pragma unroll
                    for (uint32_t q = 0; q < 4; q++) {
#pragma unroll
                        for (uint32_t i = 0; i < PW; i++)
                            if (h + PW * q + i <= h_max && anchor_probe_any<MODE>(ak_lds, cut(__builtin_amdgcn_alignbit(x[q], lo, i * WB)), K, mask)) flag = true;
                        lo = x[q];
                    }
                }
            }
        }
        uint64_t m = __ballot(flag);
        if (lane == 0) hitmask[tile] = m;
    }
}

template <int W, int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void k_anchor_filter(DevReads R, DevAnchors K, const uint8_t *found_flag, uint64_t *hitmask)
{
    // (1 024 threads per block and, with its table in LDS, one block per CU.  Until round 4 a CRASS_VGPR_FLOOR(120) kept every
    // instantiation off a multiple of 8 registers: 4 waves x 128 allocated registers = a SIMD's whole file, so no wave of any
    // other kernel could share the CU — the view export beside it then cost the probe 144 -> 216 us.  The build's guard is exact
    // now, crass_amd/vgpr_guard.py, and these kernels hold no 64-bit shift by their last register.)
    extern __shared__ __attribute__((aligned(16))) uint32_t ak_lds_buf[];
    const uint32_t tsize = 1u << K.log_size;
    const uint32_t *ak_lds = K.table;                   // key sets too large for LDS are probed in global memory (L2)
    if (MODE != 2) {
        for (uint32_t i = threadIdx.x; i < tsize; i += THREADS) ak_lds_buf[i] = K.table[i];
        __syncthreads();
        ak_lds = ak_lds_buf;
    }
    anchor_filter_body<W, THREADS, MODE>(R, K, ak_lds, found_flag, hitmask);
}

// the same filter when the key table was built on the device (dmerge.hip): its size is only known there
// (ASH is a template parameter of the KERNEL: with both forms in one kernel the default one was allocated the other's registers —
// 99 instead of 56 — and no other kernel's waves fitted beside its four per SIMD any more)
template <int W, int THREADS, int ASH, int KL>
__global__ __launch_bounds__(THREADS) void k_anchor_filter_dev(DevReads R, DevMerge M, const uint8_t *found_flag, uint64_t *hitmask)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ak_lds_buf[];
    if (M.flag_post && blockIdx.x == 0 && threadIdx.x == 0) stage_flag_store(M.flag_post, M.flag_post_val);      // (the merge's kernels are complete)
    DevAnchors K;
    K.table = M.anchor_tab; K.log_size = M.st->log_size; K.mode = 0; K.m1 = M.m1; K.m2 = M.m2; K.n_keys = 0;
    K.with_exc = 1;
    if (M.st->fail != 0 || K.log_size == 0) {            // the host redoes the merge; flag nothing
        const uint64_t n_tiles = (R.n_reads + 63) / 64;
        for (uint64_t t = blockIdx.x * (uint64_t)THREADS + threadIdx.x; t < n_tiles; t += (uint64_t)gridDim.x * THREADS) hitmask[t] = 0ull;
        return;
    }
    if (K.log_size <= 15) {
        const uint32_t tsize = 1u << K.log_size;
        for (uint32_t i = threadIdx.x; i < tsize; i += THREADS) ak_lds_buf[i] = K.table[i];
        __syncthreads();
        anchor_filter_body<W, THREADS, 0, ASH, KL>(R, K, ak_lds_buf, found_flag, hitmask);
    } else if (M.st->tab_mode == 3) {
        for (uint32_t i = threadIdx.x; i < (1u << 15); i += THREADS) ak_lds_buf[i] = M.anchor_fp[i];
        __syncthreads();
        anchor_filter_body<W, THREADS, 3, ASH, KL>(R, K, ak_lds_buf, found_flag, hitmask);
    } else {
        for (uint32_t i = threadIdx.x; i < (1u << 15); i += THREADS) ak_lds_buf[i] = M.anchor_fp[i];
        __syncthreads();
        anchor_filter_body<W, THREADS, 4, ASH, KL>(R, K, ak_lds_buf, found_flag, hitmask);
    }
}

// The run-time stride as the kernels' compile-time W: a register form for rows of 4 .. 16 words, 0 for everything else.
// f is called once, with a std::integral_constant.
template <int N> using int_c = std::integral_constant<int, N>;
template <typename F>
static hipError_t with_row_words(uint32_t stride_words, F &&f)
{
    switch (stride_words) {
        case 4: return f(int_c<4>{});   case 5: return f(int_c<5>{});   case 6: return f(int_c<6>{});   case 7: return f(int_c<7>{});
        case 8: return f(int_c<8>{});   case 9: return f(int_c<9>{});   case 10: return f(int_c<10>{}); case 11: return f(int_c<11>{});
        case 12: return f(int_c<12>{}); case 13: return f(int_c<13>{}); case 14: return f(int_c<14>{}); case 15: return f(int_c<15>{});
        case 16: return f(int_c<16>{});
        default: return f(int_c<0>{});
    }
}

// max_blocks: 0, or a cap on the grid (CRASS_PROBE_BLOCKS: the tests make every wave walk several tiles of a small read set)
hipError_t launch_anchor_filter_dev(const DevReads &R, const DevMerge &M, const uint8_t *found_flag, uint64_t *hitmask, hipStream_t st, uint32_t max_blocks)
{
    if (R.n_reads == 0) return hipSuccess;
    if (!((M.akey_bases == 16u && (M.akey_shift == 3u || M.akey_shift == 2u)) || (M.akey_bases == 12u && M.akey_shift == 2u))) return hipErrorInvalidValue;
    const size_t lds = 128 * 1024;
    const uint64_t n_tiles = (R.n_reads + 63) / 64;
    constexpr int T = 1024;
    uint64_t blocks = (n_tiles + (T / 64) - 1) / (T / 64);
    if (blocks > 256) blocks = 256;
    if (max_blocks && blocks > max_blocks) blocks = max_blocks;
    return with_row_words(R.stride_words, [&](auto w) -> hipError_t {
        constexpr int W = decltype(w)::value;
#define AKD_LAUNCH(AA, KK)                                                                                                \
        {                                                                                                               \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_anchor_filter_dev<W, T, AA, KK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e;                                                                              \
            CRASS_LAUNCH((k_anchor_filter_dev<W, T, AA, KK>), dim3((unsigned)blocks), dim3(T), lds, st, R, M, found_flag, hitmask); \
        }
        if (M.akey_shift == 2u && M.akey_bases == 12u) AKD_LAUNCH(2, 12) else if (M.akey_shift == 2u) AKD_LAUNCH(2, 16) else AKD_LAUNCH(3, 16)
#undef AKD_LAUNCH
        return hipGetLastError();
    });
}

hipError_t launch_anchor_filter(const DevReads &R, const DevAnchors &K, const uint8_t *found_flag, uint64_t *hitmask, hipStream_t st, uint32_t max_blocks)
{
    if (R.n_reads == 0) return hipSuccess;
    const size_t tbytes = (size_t)4 << K.log_size;
    const bool in_lds = tbytes <= 128 * 1024;
    if (K.mode == 1 && !in_lds) return hipErrorInvalidValue;
    const size_t lds = in_lds ? tbytes : 0;
    const uint64_t n_tiles = (R.n_reads + 63) / 64;
    constexpr int T = 1024;
    uint64_t blocks = (n_tiles + (T / 64) - 1) / (T / 64);
    const uint64_t cap = lds > 80 * 1024 ? 256 : (lds > 40 * 1024 ? 512 : 1024);
    if (blocks > cap) blocks = cap;
    if (max_blocks && blocks > max_blocks) blocks = max_blocks;
    return with_row_words(R.stride_words, [&](auto w) -> hipError_t {
        constexpr int W = decltype(w)::value;
#define AK_LAUNCH(MM)                                                                                                     \
        {                                                                                                               \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_anchor_filter<W, T, MM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e;                                                                              \
            CRASS_LAUNCH((k_anchor_filter<W, T, MM>), dim3((unsigned)blocks), dim3(T), lds, st, R, K, found_flag, hitmask); \
        }
        if (!in_lds) AK_LAUNCH(2) else if (K.mode == 1) AK_LAUNCH(1) else AK_LAUNCH(0)
#undef AK_LAUNCH
        return hipGetLastError();
    });
}

// exact first-match scan of the flagged reads (lane per flagged read), transition table in global
// memory (L2-resident).  info_by_slot[k] = (end_exclusive << 8) | length, 0 = no pattern occurs.
__global__ __launch_bounds__(256) void k_recruit_list(DevReads R, DevAutomaton A, const uint64_t *idx, const uint32_t *d_n,
                                                       uint64_t n_max, uint32_t *info_by_slot, uint32_t *pid_by_slot)
{
    uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t n = *d_n;
    if (n > n_max) n = n_max;
    if (k >= n) return;
    const uint64_t r = idx[k];
    const uint32_t L = rd_len(R, r);
    const uint32_t *g = R.packed + rd_word_off(R, r);
    const uint32_t symA = A.sym['A'], symC = A.sym['C'], symG = A.sym['G'], symT = A.sym['T'];
    uint32_t state = 0, word = 0, info = 0, pid = 0;
    for (uint32_t i = 0; i < L; i++) {
        if ((i & 15u) == 0) word = g[i >> 4];
        uint32_t c = word & 3u;
        word >>= 2;
        if (A.go4) state = A.go4[state * 4 + c];
        else if (A.go4w) state = A.go4w[(size_t)state * 4 + c];
        else {
            uint32_t sy = c == 0 ? symA : c == 1 ? symC : c == 2 ? symG : symT;
            state = A.go16 ? (uint32_t)A.go16[(size_t)state * A.n_sym1 + sy] : A.go32[(size_t)state * A.n_sym1 + sy];
        }
        uint32_t ol = A.out_len[state];
        if (ol) { info = ((i + 1) << 8) | ol; pid = A.out_pid[state]; break; }
    }
    info_by_slot[k] = info;
    pid_by_slot[k] = pid;
}

// The same for long reads: one WAVE per flagged read.  The automaton's state at a position only depends on the last
// max_pat_len bases (the depth of the trie), so lane l scans its own slice [l * seg, (l + 1) * seg) after a warm-up of
// max_pat_len bases from the start state and is in the exact state for every position it reports; the first callback
// of the whole read is the smallest reported position over the lanes (a lane per 10 kbp read walked 10 000 dependent
// table look-ups: 2.8 ms for a few hundred reads).
__global__ __launch_bounds__(256) void k_recruit_list_wave(DevReads R, DevAutomaton A, const uint64_t *idx, const uint32_t *d_n,
                                                            uint64_t n_max, uint32_t *info_by_slot, uint32_t *pid_by_slot)
{
    const int lane = threadIdx.x & 63;
    const uint64_t k = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    uint64_t n = *d_n;
    if (n > n_max) n = n_max;
    if (k >= n) return;
    const uint64_t r = idx[k];
    const uint32_t L = rd_len(R, r);
    const uint32_t *g = R.packed + rd_word_off(R, r);
    const uint32_t symA = A.sym['A'], symC = A.sym['C'], symG = A.sym['G'], symT = A.sym['T'];
    const uint32_t seg = (L + 63u) / 64u;
    const uint32_t s0 = (uint32_t)lane * seg, e0 = min(L, s0 + seg);
    uint32_t first = 0xFFFFFFFFu, ol_found = 0, pid = 0;
    if (s0 < L) {
        const uint32_t p0 = s0 >= A.max_pat_len ? s0 - A.max_pat_len : 0u;        // warm-up (exact from the read start anyway)
        uint32_t state = 0, word = 0;
        for (uint32_t i = p0; i < e0; i++) {
            if ((i & 15u) == 0 || i == p0) word = g[i >> 4] >> ((i & 15u) * 2u);
            const uint32_t c = word & 3u;
            word >>= 2;
            if (A.go4) state = A.go4[state * 4 + c];
            else if (A.go4w) state = A.go4w[(size_t)state * 4 + c];
            else {
                const uint32_t sy = c == 0 ? symA : c == 1 ? symC : c == 2 ? symG : symT;
                state = A.go16 ? (uint32_t)A.go16[(size_t)state * A.n_sym1 + sy] : A.go32[(size_t)state * A.n_sym1 + sy];
            }
            if (i >= s0) {
                const uint32_t ol = A.out_len[state];
                if (ol) { first = i; ol_found = ol; pid = A.out_pid[state]; break; }
            }
        }
    }
    uint32_t best = first;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off));
    if (best == 0xFFFFFFFFu) { if (lane == 0) { info_by_slot[k] = 0; pid_by_slot[k] = 0; } return; }
    if (first == best) {                                  // exactly one lane owns that position
        info_by_slot[k] = ((best + 1) << 8) | ol_found;
        pid_by_slot[k] = pid;
    }
}

hipError_t launch_recruit_list(const DevReads &R, const DevAutomaton &A, const uint64_t *idx, const uint32_t *d_n,
                               uint64_t n_max, uint32_t *info_by_slot, uint32_t *pid_by_slot, hipStream_t st)
{
    if (n_max == 0) return hipSuccess;
    if (R.wave_walk && A.max_pat_len)                      // long reads
        CRASS_LAUNCH(k_recruit_list_wave, dim3((unsigned)((n_max + 3) / 4)), dim3(256), 0, st, R, A, idx, d_n, n_max, info_by_slot, pid_by_slot);
    else
        CRASS_LAUNCH(k_recruit_list, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, st, R, A, idx, d_n, n_max, info_by_slot, pid_by_slot);
    return hipGetLastError();
}

// exception reads: raw bytes through the byte-symbol automaton, lane per exception read
__global__ __launch_bounds__(256) void k_recruit_exc(DevReads R, DevAutomaton A, const uint8_t *found_flag, uint32_t *exc_hit_info)
{
    uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (s >= R.n_exc) return;
    uint64_t r = R.exc_read[s];
    uint32_t info = 0;
    if (!found_flag[rd_header_id(R, r)]) {
        uint64_t o0 = R.exc_off[s];
        uint32_t L = (uint32_t)(R.exc_off[s + 1] - o0);
        uint32_t state = 0;
        for (uint32_t i = 0; i < L; i++) {
            uint32_t sy = A.sym[R.exc_bytes[o0 + i]];
            state = A.go16 ? (uint32_t)A.go16[(size_t)state * A.n_sym1 + sy] : A.go32[(size_t)state * A.n_sym1 + sy];
            uint32_t ol = A.out_len[state];
            if (ol) { info = ((i + 1) << 8) | ol; break; }
        }
    }
    exc_hit_info[s] = info;
}

hipError_t launch_recruit_exceptions(const DevReads &R, const DevAutomaton &A, const uint8_t *found_flag,
                                     uint32_t *exc_hit_info, hipStream_t st)
{
    if (R.n_exc == 0) return hipSuccess;
    CRASS_LAUNCH(k_recruit_exc, dim3((unsigned)((R.n_exc + 255) / 256)), dim3(256), 0, st, R, A, found_flag, exc_hit_info);
    return hipGetLastError();
}

// on_match + addReadHolder's DRLowLexi for the single recruited repeat
// (libcrispr.cpp:408-442, ReadHolder.cpp:524-528,573-590).  Thread per hit.
template <bool EXC>
__global__ __launch_bounds__(256) void k_recruit_finish(DevReads R, const uint64_t *hit_idx, const uint32_t *d_n_hits,
                                                        uint64_t n_max, const uint32_t *hit_info, int info_by_slot,
                                                        const uint32_t *pid_by_slot, const uint32_t *pat_token,
                                                        RecruitOut *out, char *dr_chars, uint32_t dr_stride, const uint64_t *pat_mask)
{
    if constexpr (!EXC) CRASS_VGPR_FLOOR(24);      // 24 VGPRs with the 128-bit shift amount in v23: the kernel that exposed the erratum
    uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t n = EXC ? R.n_exc : (uint64_t)(*d_n_hits);
    if (n > n_max) n = n_max;
    if (k >= n) return;
    RecruitOut o; o.start = 0; o.end = 0; o.token = 0; o.dr_len = 0; o.low_lexi = 0; o.pad = 0;
    uint32_t info;
    uint32_t L;
    uint64_t r = 0, o0 = 0;
    const uint32_t *g = nullptr;
    if (EXC) {
        info = hit_info[k];
        o0 = R.exc_off[k];
        L = (uint32_t)(R.exc_off[k + 1] - o0);
    } else {
        r = hit_idx[k];
        info = info_by_slot ? hit_info[k] : hit_info[r];
        L = rd_len(R, r);
        g = R.packed + rd_word_off(R, r);
    }
    if (info == 0) { out[k] = o; return; }              // no match (exception read / anchor false positive)
    uint32_t textpos = info >> 8, len = info & 0xFFu;
    uint32_t DR_end = textpos - 1;
    if (DR_end >= L) DR_end = L - 1;
    uint32_t start = DR_end - (len - 1);
    // a pattern with an 'N' (device merge, dmerge.hip) matched an exception read: the packed words hold 'A' there,
    // so the repeat is read from the read's bytes
    const uint8_t *raw = nullptr;
    if (!EXC && pat_mask && pid_by_slot && pat_mask[pid_by_slot[k]] != 0ull && R.n_exc) {
        uint64_t lo = 0, hi = R.n_exc - 1;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (R.exc_read[mid] < r) lo = mid + 1; else hi = mid; }
        raw = R.exc_bytes + R.exc_off[lo];
    }
    if (!EXC && len <= 64 && !raw) {
        // packed reads: the repeat as a 128-bit value (base i in bits 2i..2i+1), its reverse complement by bit
        // reversal, and DRLowLexi's string comparison as "first differing base from the low end"
        const uint32_t nw = (L + 15) >> 4, w0 = start >> 4, sh = (start & 15u) * 2u;
        uint32_t x[5];
#pragma unroll
        for (int q = 0; q < 5; q++) x[q] = (w0 + q < nw) ? g[w0 + q] : 0u;
        uint32_t y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) y[q] = sh ? ((x[q] >> sh) | (x[q + 1] << (32 - sh))) : x[q];
        uint64_t v0 = (uint64_t)y[0] | ((uint64_t)y[1] << 32), v1 = (uint64_t)y[2] | ((uint64_t)y[3] << 32);
        const uint64_t m0 = len >= 32 ? ~0ull : ((1ull << (2 * len)) - 1ull);
        const uint64_t m1 = len >= 64 ? ~0ull : (len > 32 ? ((1ull << (2 * (len - 32))) - 1ull) : 0ull);
        v0 &= m0; v1 &= m1;
        auto rev2 = [](uint64_t t) -> uint64_t {          // reverse the order of the 32 two-bit groups
            t = __brevll(t);
            return ((t >> 1) & 0x5555555555555555ull) | ((t & 0x5555555555555555ull) << 1);
        };
        // complement, reverse all 64 groups of the 128-bit value, then shift the len groups down to bit 0
        const uint64_t c0 = rev2(~v1), c1 = rev2(~v0);     // (c1:c0) = reversed 128 bits
        const uint32_t drop = 128u - 2u * len;             // unused high groups became low groups
        uint64_t r0, r1;
        if (drop == 0) { r0 = c0; r1 = c1; }
        else if (drop < 64) { r0 = (c0 >> drop) | (c1 << (64 - drop)); r1 = c1 >> drop; }
        else { r0 = c1 >> (drop - 64); r1 = 0; }
        r0 &= m0; r1 &= m1;
        int less = 0;
        const uint64_t d0 = v0 ^ r0, d1 = v1 ^ r1;
        if (d0 | d1) {
            const uint64_t dv = d0 ? d0 : d1, av = d0 ? v0 : v1, bv = d0 ? r0 : r1;
            const int p = (__ffsll((unsigned long long)dv) - 1) & ~1;
            less = ((av >> p) & 3ull) < ((bv >> p) & 3ull);
        }
        const uint64_t s0 = less ? v0 : r0, s1 = less ? v1 : r1;
        if (dr_chars) {
            char *dr = dr_chars + k * (uint64_t)dr_stride;
            for (uint32_t i = 0; i < dr_stride; i++) {
                const uint32_t c = (uint32_t)(((i < 32 ? s0 : s1) >> (2 * (i & 31))) & 3ull);
                dr[i] = i < len ? "ACGT"[c] : (char)0;
            }
        }
        if (less) { o.start = start; o.end = DR_end; o.low_lexi = 1; }
        else { o.start = L - 1 - DR_end; o.end = L - 1 - start; o.low_lexi = 0; }
        o.dr_len = (uint16_t)len;
        if (pid_by_slot && pat_token) o.token = pat_token[pid_by_slot[k]];
        out[k] = o;
        return;
    }
    auto base_at = [&](uint32_t i) -> uint8_t {
        if (EXC) return R.exc_bytes[o0 + i];
        if (raw) return raw[i];
        uint32_t c = (g[i >> 4] >> ((i & 15u) * 2u)) & 3u;
        return (uint8_t)("ACGT"[c]);
    };
    int less = 0;
    for (uint32_t i = 0; i < len; i++) {
        uint8_t a = base_at(start + i);
        uint8_t b = c_comp.v[base_at(start + len - 1 - i) & 127];
        if (a != b) { less = a < b; break; }
    }
    char *dr = dr_chars ? dr_chars + k * (uint64_t)dr_stride : nullptr;
    if (less) {
        if (dr) for (uint32_t i = 0; i < len; i++) dr[i] = (char)base_at(start + i);
        o.start = start; o.end = DR_end; o.low_lexi = 1;
    } else {
        if (dr) for (uint32_t i = 0; i < len; i++) dr[i] = (char)c_comp.v[base_at(start + len - 1 - i) & 127];
        o.start = L - 1 - DR_end; o.end = L - 1 - start; o.low_lexi = 0;
    }
    if (dr) for (uint32_t i = len; i < dr_stride; i++) dr[i] = 0;
    o.dr_len = (uint16_t)len;
    // the matched pattern's low-lexi form is a stored DR variant: its token was resolved once per
    // pattern on the host (addReadHolder's lookup, libcrispr.cpp:1137)
    if (pid_by_slot && pat_token) o.token = pat_token[pid_by_slot[k]];
    out[k] = o;
}

hipError_t launch_recruit_finish(const DevReads &R, const uint64_t *hit_idx, const uint32_t *d_n_hits, uint64_t n_hits_max,
                                 const uint32_t *hit_info, bool info_by_slot, bool exceptions,
                                 const uint32_t *pid_by_slot, const uint32_t *pat_token, RecruitOut *out,
                                 char *dr_chars, uint32_t dr_stride, hipStream_t st, const uint64_t *pat_mask)
{
    if (n_hits_max == 0) return hipSuccess;
    unsigned nb = (unsigned)((n_hits_max + 255) / 256);
    if (exceptions)
        CRASS_LAUNCH(k_recruit_finish<true>, dim3(nb), dim3(256), 0, st, R, hit_idx, d_n_hits, n_hits_max, hit_info, 1, pid_by_slot, pat_token, out, dr_chars, dr_stride, (const uint64_t *)nullptr);
    else
        CRASS_LAUNCH(k_recruit_finish<false>, dim3(nb), dim3(256), 0, st, R, hit_idx, d_n_hits, n_hits_max, hit_info, info_by_slot ? 1 : 0, pid_by_slot, pat_token, out, dr_chars, dr_stride, pat_mask);
    return hipGetLastError();
}

} // namespace crass

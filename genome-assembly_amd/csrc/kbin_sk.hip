// kbin_sk.hip -- the binned engine's records: super-k-mer extraction (phase
// A), routing to owner ranks, and the receiver's conversion of routed records
// into binned ones (plain, or into the local bucket regions).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "kbin_internal.h"
#include "kbin_device.h"

namespace kb {

// ---------------------------------------------------------------------------
// phase A: super-k-mer extraction
// ---------------------------------------------------------------------------
// One segment of the sticky chain per call: leftmost strict argmax of the
// complement-canonical mmer score over [lo, lo + K - M]  (binning.c:922-988).
DEV void segment_at(const uint64_t* sw, int lo, int lane, int W, int M, uint32_t maskM,
                    uint32_t halfM, int& sig, uint32_t& canon) {
    const int d = (lane - lo) & 63;
    uint32_t key = 0;
    if (d < W) {
        const int p = lo + d;
        const uint32_t s = (uint32_t)(window64(sw, p) >> (64 - 2 * M));
        const uint32_t c = s >= halfM ? s : maskM - s;
        key = (c << 16) | (0xFFFFu - (uint32_t)p);
    }
    key = wave_max_u32(key);
    sig = rfl((int)(0xFFFFu - (key & 0xFFFFu)));
    canon = (uint32_t)rfl((int)(key >> 16));
}

// QK (K < 2M): the reference's per-k-mer signature state, binning.c:922-1021.
// The incremental branch (992-1021: j runs K-M .. M-1) is live: it appends
// bases to a score it never trims, in int arithmetic that wraps, so the
// signature can move to the k-mer's last M bases and is_rev follow the
// polluted scores.  One lane walks its read k-mer by k-mer with that state;
// a record is a run of k-mers with one signature position (`next`).
struct QWalk {
    int32_t s = 0, r = 0, m = 0;  // score, rev_score, max_score
    bool rev = false;
    int sig = -1, i = -1;         // signature position, last k-mer stepped
    DEV uint32_t code(const uint64_t* sw, int p, int M, uint32_t maskM) const {
        return (uint32_t)(window64(sw, p) >> (64 - 2 * M)) & maskM;
    }
    DEV void step(const uint64_t* sw, int k, int K, int M, uint32_t maskM) {
        if (k > sig) {  // a fresh window (binning.c:922-989): leftmost strict argmax
            uint32_t sm = code(sw, k, M, maskM);
            int32_t sc = (int32_t)sm, rv = (int32_t)(maskM - sm);
            m = sc > rv ? sc : rv;
            rev = !(sc > rv);
            sig = k;
            for (int p = k + 1; p <= k + K - M; p++) {
                sm = code(sw, p, M, maskM);
                sc = (int32_t)sm;
                rv = (int32_t)(maskM - sm);
                if ((sc > rv ? sc : rv) > m) {
                    m = sc > rv ? sc : rv;
                    rev = !(sc > rv);
                    sig = p;
                }
            }
            s = sc;
            r = rv;
        } else {  // the incremental branch (binning.c:992-1021)
            for (int j = K - M; j < M; j++) {
                const uint32_t v = (uint32_t)(window64(sw, k + j) >> 62);
                s = (int32_t)((uint32_t)s * 4u + v);
                r = (int32_t)((uint32_t)r * 4u + 3u - v);
            }
            if ((s > r ? s : r) > m) {
                m = s > r ? s : r;
                rev = !(s > r);
                sig = k + K - M;
            }
        }
        i = k;
    }
    // the record starting at k-mer lo: its signature and complement flag, and
    // the first k-mer of the next record
    DEV void next(const uint64_t* sw, int lo, int nK, int K, int M, uint32_t maskM, int& rsig, bool& rrev,
                  int& e) {
        if (i < lo) step(sw, lo, K, M, maskM);
        rsig = sig;
        rrev = rev;
        e = lo + 1;
        while (e < nK) {
            step(sw, e, K, M, maskM);
            if (sig != rsig) break;
            e++;
        }
    }
};

// CPU-callable check of bm_has_entry's guard (kbin_internal.h; tests/test_abi.py):
// the first destination of a depth-0 record of code `canon` on a bucketed pass
// with map `map` over NB buckets -- the map's bucket for a canonical code, the
// hash route for any other (never map[canon - half] with canon < half)
extern "C" uint32_t kb_internal_map_dest(const uint32_t* map, uint32_t canon, int M, uint32_t NB) {
    if (!map || !bm_has_entry(canon, M)) return dest_of(canon, NB, BUCKET_SALT);
    return map[canon - (1u << (2 * M - 1))] & 1023u;
}
DEV uint32_t owner_of_mmer(uint32_t mmer, uint32_t G) { return dest_of(mmer, G, OWNER_SALT); }

template <bool WRITE, bool QK = false>
__global__ __launch_bounds__(256) void sk_kernel(SkScanArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint64_t smem[];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int RW = A.RW, K = A.K, M = A.M;
    const int W = K - M + 1;
    const uint32_t maskM = (1u << (2 * M)) - 1u;
    const uint32_t halfM = 1u << (2 * M - 1);
    uint64_t* sw = smem + wid * (RW + 2);  // two zero words: span windows never leave the read
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    uint64_t kmers = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + wid; r < A.n_reads; r += nwaves) {
        const int L = rfl((int)A.lens[r]);
        const int nK = L - K + 1;
        uint32_t nseg = 0;
        if (nK > 0) {
            wave_sync();
            for (int w = lane; w < RW + 2; w += 64) sw[w] = w < RW ? A.words[r * RW + w] : 0ull;
            wave_sync();
            const uint64_t rbase = WRITE ? A.rec_base[r] : 0;
            const uint64_t ordv = (uint64_t)(A.ord_base + (uint32_t)r);
            int lo = 0;
            QWalk qw;  // (QK: lane 0's walk, its records broadcast to the wave)
            while (lo < nK) {
                int sig, nlo;
                uint32_t canon;
                bool qrev = false;
                if (QK) {
                    int rs = 0, e = 0;
                    bool rv = false;
                    if (lane == 0) qw.next(sw, lo, nK, K, M, maskM, rs, rv, e);
                    sig = __shfl(rs, 0, 64);
                    nlo = __shfl(e, 0, 64);
                    qrev = __shfl((int)rv, 0, 64) != 0;
                    const uint32_t sm = qw.code(sw, sig, M, maskM);
                    canon = qrev ? maskM - sm : sm;  // the bin's mmer code (not canonical)
                } else {
                    segment_at(sw, lo, lane, W, M, maskM, halfM, sig, canon);
                    nlo = sig + 1;
                }
                if (!in_part(canon, A.part, A.part_n)) {  // another pass's super-k-mer
                    lo = nlo;
                    continue;
                }
                const int n = QK ? nlo - lo : min(sig, nK - 1) - lo + 1;
                kmers += (uint64_t)n;
                if (WRITE && lane == 0) {
                    // one super-k-mer: k-mers lo..lo+n-1 share the signature at
                    // sig (binning.c:1004-1040 with the sticky window).  Span =
                    // bases lo .. lo+n+K-2 (<= 56 for K <= 31).
                    const uint64_t t = rbase + nseg;
                    const uint32_t sm = (uint32_t)(window64(sw, sig) >> (64 - 2 * M));
                    // complement wins (binning.c:1029-1040)
                    const uint64_t rev = QK ? (qrev ? 1ull : 0ull) : (sm < halfM ? 1ull : 0ull);
                    A.pay[3 * t + 0] = ordv | ((uint64_t)n << 32) | ((uint64_t)(sig - lo) << 38) | (rev << 44) |
                                       ((uint64_t)lo << 45);
                    A.pay[3 * t + 1] = window64(sw, lo);
                    A.pay[3 * t + 2] = window64(sw, lo + 32);
                    A.keys[t] = ((uint64_t)canon << 38) | ((uint64_t)(63 - n) << 32) | (uint32_t)t;
                }
                nseg++;
                lo = nlo;
            }
        }
        if (!WRITE && lane == 0) A.seg_count[r] = nseg;
    }
    if (!WRITE) {
        __shared__ uint64_t sh[4];
        const uint64_t tot = block_sum256((uint64_t)(lane == 0 ? kmers : 0), sh);
        if (threadIdx.x == 0) A.n_kmers[blockIdx.x] = tot;
    }
}

// one record into a destination region: the binned layout (ordinal) or the
// routed one (read id), see SkScanArgs; then rw - 1 span words from base lo
// (n + K - 1 <= 2K - M bases: 2 words for K <= 31, 4 for K <= 63)
DEV void put_record(const SkScanArgs& A, uint64_t* o, uint32_t ord, uint64_t lo, uint64_t n, uint64_t so,
                    uint64_t rev, const uint64_t* sw, uint32_t sub = 0) {
    if (A.binned_fmt) {
        o[0] = (uint64_t)ord | (n << 32) | (so << 38) | (rev << 44) | (lo << 45);
    } else {
        const uint32_t id = (uint32_t)id_of(ord, A.read_ids, A.id_off);
        o[0] = (uint64_t)id | (lo << 32) | (n << 48) | (so << 54) | (rev << ROUTED_REV_BIT);
    }
    for (int w = 1; w < A.rw; w++) {
        uint64_t x = window64(sw, (int)lo + 32 * (w - 1));
        if (A.sub_stamp && w + 1 == A.rw) x = (x & ~SUB_MASK) | sub;  // (a bucket record's sub-bin, sub_room)
        o[w] = x;
    }
}

// The pieces of one record bound for destination regions: its owner rank or
// local bucket, or -- a split mmer's record -- its context sub-bin's bucket,
// cut in two (the first ne k-mers, the edge, then the rest) when its first
// k-mers lie in the edge.  row: the read's LDS row (the context bases).
// Returns the number of pieces; d[] their regions.
DEV uint32_t record_pieces(const SkScanArgs& A, uint32_t canon, int lo, int n, int so, bool rev,
                           const uint64_t* row, uint32_t (&d)[2], uint32_t (&sub)[2], int& ne) {
    ne = 0;
    sub[0] = sub[1] = 0;
    if (!A.bucket_map || !bm_has_entry(canon, A.M)) {
        d[0] = A.owner_map && bm_has_entry(canon, A.M) ? (uint32_t)A.owner_map[canon - (1u << (2 * A.M - 1))]
                                                       : dest_of(canon, A.G, A.dest_salt);
        return 1;
    }
    const uint32_t me = A.bucket_map[canon - (1u << (2 * A.M - 1))];
    const uint32_t b = bm_depth(me);
    if (!b) {
        d[0] = me & 1023u;
        return 1;
    }
    const uint64_t w = window64(row, lo + so + A.M);  // the read's bases after the signature
    const int e = sub_edge(so, n, A.K, A.M, b);
    if (e > 0 && e < n) {
        ne = e;
        sub[1] = sub_ctx(so - e, A.K, A.M, b, w, rev);
        d[0] = bm_bucket(me, A.sub_map, 0u);
        d[1] = bm_bucket(me, A.sub_map, sub[1]);
        return 2;
    }
    sub[0] = sub_ctx(so, A.K, A.M, b, w, rev);
    d[0] = bm_bucket(me, A.sub_map, sub[0]);
    return 1;
}

// The record pass's count loop plans each staged record once -- its pieces'
// destinations from the map entry me (bucket_map[canon - 2^(2M-1)], loaded by
// the caller) -- and caches the plan in the staged entry, so the placement
// loop repeats no map lookups.  Staged entry bits: lo 0..15 (< 512 for the
// thread kernel's reads), n 16..21, so 22..27, rev 28, row 29..37, canon
// 38..63; planned: canon -> d0 | d1 << 10 | ne << 20 | (pieces - 1) << 25, and
// the sub-bin depth b in bits 9..11.
DEV uint64_t record_plan(const SkScanArgs& A, uint64_t e, uint32_t me, const uint64_t* row) {
    const uint32_t canon = (uint32_t)(e >> 38);
    const int lo = (int)(e & 0x1FFu), n = (int)((e >> 16) & 63u), so = (int)((e >> 22) & 63u);
    const bool rev = ((e >> 28) & 1u) != 0;
    uint32_t d0 = 0, d1 = 0, b = 0, two = 0;
    int ne = 0;
    if (!A.bucket_map || !bm_has_entry(canon, A.M)) {  // (me: not loaded for such a code)
        d0 = A.owner_map && bm_has_entry(canon, A.M) ? (uint32_t)A.owner_map[canon - (1u << (2 * A.M - 1))]
                                                     : dest_of(canon, A.G, A.dest_salt);
    } else if (!(b = bm_depth(me))) {
        d0 = me & 1023u;
    } else {
        const uint64_t w = window64(row, lo + so + A.M);  // the read's bases after the signature
        const int ec = sub_edge(so, n, A.K, A.M, b);
        if (ec > 0 && ec < n) {
            ne = ec;
            two = 1;
            d0 = bm_bucket(me, A.sub_map, 0u);
            d1 = bm_bucket(me, A.sub_map, sub_ctx(so - ec, A.K, A.M, b, w, rev));
        } else {
            d0 = bm_bucket(me, A.sub_map, sub_ctx(so, A.K, A.M, b, w, rev));
        }
    }
    const uint64_t pk = (uint64_t)d0 | ((uint64_t)d1 << 10) | ((uint64_t)ne << 20) | ((uint64_t)two << 25);
    return (e & 0x3FFFFF01FFull) | ((uint64_t)b << 9) | (pk << 38);
}

// Add one record to a packed 16-bit LDS destination count (two per word) and
// return the count before it, aggregated over the wave: lanes bound for the
// same destination share one atomic (the lowest lane's) and take their
// offsets from the ballot.  With few destinations (ranks) every lane of a wave
// would otherwise hit the same word and the LDS would serialise 64 returning
// atomics per instruction (1.97 ms vs 0.27 ms for the pass at one rank).
DEV uint32_t wave_dest_add(uint32_t* cnt2, uint32_t d) {
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t off = 0;
    bool pending = true;
    for (;;) {
        const uint64_t rem = __ballot(pending);
        if (!rem) break;
        const int leader = __builtin_ctzll(rem);
        const uint32_t ld = (uint32_t)__shfl((int)d, leader, 64);
        const bool mine = pending && d == ld;
        const uint64_t m = __ballot(mine);
        uint32_t b = 0;
        if (lane == leader) {
            const uint32_t sh = 16u * (ld & 1u);
            b = (atomicAdd(&cnt2[ld >> 1], (uint32_t)__popcll(m) << sh) >> sh) & 0xFFFFu;
        }
        b = (uint32_t)__shfl((int)b, leader, 64);
        if (mine) {
            off = b + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            pending = false;
        }
    }
    return off;
}

// LDS row of one read in sk_thread_kernel: the read's words, then zero words
// so that every span window (up to 4 words past the first base) stays inside
__device__ __host__ inline int sk_row_words(int RW, int rw) { return RW + (rw > 3 ? rw - 1 : 2); }

// Thread-per-read variant for short reads (RW <= SK_THREAD_RW): a block
// stages SKT reads in LDS rows and each lane walks its own read's sticky
// chain serially.  The wave-per-read kernel above keeps 64 lanes busy on a
// window of only K-M+1 positions; one lane per read does the same argmax
// with no cross-lane reduction and no idle lanes.  The window of mmer scores
// is walked with a 2-bit shift per position (two LDS reads per segment).
// The write pass stages each record as one u64 in LDS and the block then
// writes its (contiguous) record range with coalesced stores.
constexpr int SK_THREAD_RW = 16;
// staged records per block (8 B each): 256 reads of 150 bp make ~2.5 K; a
// block past it stores the rest directly.  With the per-destination arrays
// (16-bit counts, two per word) and the read rows the block fits four to a CU.
constexpr int SKT = 512;              // reads (lanes) per block
constexpr uint32_t SK_STAGE = 4992;   // (two blocks per CU)
static_assert(SKT <= 512, "a staged record keeps its row in 9 bits");
constexpr uint32_t SK_MAX_DEST = 1024;  // destination regions (ranks or buckets)

#ifdef KB_BIN_PROF
// record pass phases (thread 0's clock at the block's barriers, summed over
// blocks): row loads, walk, per-destination counts + reservations, placement
__device__ unsigned long long g_sk_prof[8];
#define SKPROF(ph)                                        \
    do {                                                  \
        if (tid == 0) {                                   \
            const unsigned long long t1_ = clock64();     \
            atomicAdd(&g_sk_prof[ph], t1_ - skt_);        \
            skt_ = t1_;                                   \
        }                                                 \
    } while (0)
#else
#define SKPROF(ph) do {} while (0)
#endif
// a value the compiler must keep in a VGPR and cannot see through
DEV uint32_t vreg(uint32_t v) {
    asm("" : "+v"(v));
    return v;
}

// QK (K < 2M): the reference's incremental branch is live (binning.c:992-1021:
// j runs K-M .. M-1, appending bases to a score it never trims, in int
// arithmetic that wraps).  Each lane then walks its read k-mer by k-mer with
// the reference's own state (score, rev_score, max_score, is_rev, signature),
// and a record is a run of k-mers with one signature position -- its so, rev
// and mmer are whatever that state says, not the window's leftmost argmax
template <bool WRITE, bool QK = false>
__global__ __launch_bounds__(SKT) void sk_thread_kernel(SkScanArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint64_t smem[];
    const int RW = A.RW, K = A.K, M = A.M;
    const int W = K - M + 1;  // <= 57 (K <= 63): mmer starts lo..lo+W-1 end inside one 64-base window pair
    const int RS = sk_row_words(RW, A.rw);  // row stride: zero words past the read
    const int sh = 64 - 2 * M;
    const uint32_t maskM = (1u << (2 * M)) - 1u;
    const uint32_t halfM = 1u << (2 * M - 1);
    const bool one_word = K <= 31 && M <= 12;  // (scores < 2^24 keep 8 bits for the offset)
    const uint32_t tid = threadIdx.x;
    uint64_t* stg = smem + SKT * RS;  // WRITE: [SK_STAGE] {lo, n, so, rev, row, canon}
    __shared__ uint32_t span_end;
    __shared__ unsigned long long s_base;
    __shared__ uint32_t dcnt2[SK_MAX_DEST / 2];  // per-destination counts, 16 bits each (< SK_STAGE)
    __shared__ uint32_t dbase[SK_MAX_DEST];  // reserved slot in the region (< region_cap < 2^32)
    const bool route = WRITE && A.regions;          // records to destination regions, any order
    const bool alloc = WRITE && (A.rec_ctr || route);  // records placed by block allocation
    const bool rounds = alloc && !(route && A.G > 64);  // see the walk below
    uint64_t kmers = 0;
#ifdef KB_BIN_PROF
    unsigned long long skt_ = clock64();
#endif
    for (uint64_t r0 = (uint64_t)blockIdx.x * SKT; r0 < A.n_reads; r0 += (uint64_t)gridDim.x * SKT) {
        const uint32_t nrows = (uint32_t)min<uint64_t>(SKT, A.n_reads - r0);
        __syncthreads();
        {
            // (the block's reads into LDS rows, eight loads in flight per lane)
            const uint32_t nw = nrows * (uint32_t)RW;
            for (uint32_t i0 = tid; i0 < nw; i0 += 8u * SKT) {
                uint64_t v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint32_t i = i0 + (uint32_t)u * SKT;
                    v[u] = i < nw ? A.words[r0 * RW + i] : 0ull;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint32_t i = i0 + (uint32_t)u * SKT;
                    if (i >= nw) break;
                    const uint32_t row = i / (uint32_t)RW, col = i - row * (uint32_t)RW;
                    smem[row * RS + col] = v[u];
                }
            }
        }
        if (tid < nrows)
            for (int w = RW; w < RS; w++) smem[tid * RS + w] = 0;
        if (tid == 0) span_end = 0;
        __syncthreads();
        SKPROF(0);
        const uint64_t bfirst = WRITE && !alloc ? A.rec_base[r0] : 0;
        // Block allocation onto few counters (ranks, or the one record counter)
        // runs in rounds: a walk whose record finds the stage full stops there
        // and resumes after the block has written the stage out.  (Writing such
        // records one by one took a global atomic per record on a few hot
        // counters -- 256 reads of 150 bp average ~2.5 K records, so about half
        // the blocks overflowed: 1.97 ms at one rank.)  With 1024 local buckets
        // the per-record atomics spread out and are cheaper than a round.
        const uint64_t r = r0 + tid;
        const uint64_t* sw = smem + tid * RS;
        const int nK = tid < nrows ? (int)A.lens[r] - K + 1 : 0;
        const uint64_t rbase = WRITE && !alloc && tid < nrows ? A.rec_base[r] : 0;
        uint32_t nseg = 0;
        int lo = 0;
        // (QK) the reference's walk state (QWalk), and the record it closed
        // (kept across a stage-full round: the walk does not repeat)
        QWalk qw;
        int q_lo = -1, q_e = 0, q_rsig = 0;
        bool q_rrev = false;
        for (;;) {
            while (lo < nK) {
                // leftmost strict argmax of the canonical score over the window
                int best = -1, sig = lo;
                uint32_t bsm = 0;
                int nlo = 0;  // the next record's first k-mer
                if (QK) {
                    if (q_lo != lo) {  // (a stage-full round keeps the record it closed)
                        qw.next(sw, lo, nK, K, M, maskM, q_rsig, q_rrev, q_e);
                        q_lo = lo;
                    }
                    sig = q_rsig;
                    const uint32_t sm = qw.code(sw, sig, M, maskM);
                    best = (int)(q_rrev ? maskM - sm : sm);  // the bin's mmer code
                    bsm = q_rrev ? 0u : halfM;               // (rev below: bsm < halfM)
                    nlo = q_e;
                } else if (one_word) {
                    // K <= 31: the window's W mmers all lie in the 64-bit word at
                    // lo, so each score is one shift of it (no shifting chain),
                    // and the argmax is a max over (score << 8 | 255 - offset):
                    // larger score first, then the leftmost position.  In
                    // 32-bit halves: position i's mmer sits at bit sh - 2i,
                    // inside the high half for i < 17 - M, across both for
                    // i < 16, in the low half after -- one bit-field extract
                    // (two across), and both orientations' keys in one max3
                    // (the complement's key is the forward key ^ maskM << 8)
                    const uint64_t x = window64(sw, lo);
                    const uint32_t xh = (uint32_t)(x >> 32), xl = (uint32_t)x;
                    // (loop constants held in VGPRs: a VOP3 reads one SGPR on gfx9)
                    const uint32_t xc = vreg(maskM << 8), w2 = vreg(2u * (uint32_t)M);
                    const int e1 = min(W, 17 - M), e2 = min(W, 16);
                    uint32_t bk = 0;
                    const auto hi_at = [&](int p) {
                        const uint32_t k =
                            vreg((__builtin_amdgcn_ubfe(xh, (uint32_t)(sh - 32 - 2 * p), w2) << 8) | (uint32_t)(255 - p));
                        bk = max(max(bk, k), k ^ xc);
                    };
                    const auto mid_at = [&](int p) {
                        const uint32_t k = vreg(((__builtin_amdgcn_alignbit(xh, xl, (uint32_t)(sh - 2 * p)) & maskM) << 8) |
                                                (uint32_t)(255 - p));
                        bk = max(max(bk, k), k ^ xc);
                    };
                    const auto lo_at = [&](int p) {
                        const uint32_t k =
                            vreg((__builtin_amdgcn_ubfe(xl, (uint32_t)(sh - 2 * p), w2) << 8) | (uint32_t)(255 - p));
                        bk = max(max(bk, k), k ^ xc);
                    };
                    // (unrolled by hand: the loop bounds are uniform but not constant)
                    int p = 0;
                    for (; p + 2 <= e1; p += 2) hi_at(p), hi_at(p + 1);
                    if (p < e1) hi_at(p++);
                    for (; p + 2 <= e2; p += 2) mid_at(p), mid_at(p + 1);
                    if (p < e2) mid_at(p++);
                    for (; p + 3 <= W; p += 3) lo_at(p), lo_at(p + 1), lo_at(p + 2);
                    for (; p < W; p++) lo_at(p);
                    const int i = 255 - (int)(bk & 255u);
                    sig = lo + i;
                    best = (int)(bk >> 8);
                    bsm = (uint32_t)(x >> (sh - 2 * i)) & maskM;
                } else {
                    uint64_t x = window64(sw, lo), y = window64(sw, lo + 32);
                    for (int p = lo; p < lo + W; p++) {
                        const uint32_t sm = (uint32_t)(x >> sh);
                        const int c = (int)(sm >= halfM ? sm : maskM - sm);
                        if (c > best) {
                            best = c;
                            sig = p;
                            bsm = sm;
                        }
                        x = (x << 2) | (y >> 62);
                        y <<= 2;
                    }
                }
                if (!QK) nlo = sig + 1;
                const uint64_t n = QK ? (uint64_t)(nlo - lo) : (uint64_t)(min(sig, nK - 1) - lo + 1);
                if (!in_part((uint32_t)best, A.part, A.part_n)) {  // another pass's super-k-mer
                    lo = nlo;
                    continue;
                }
                if (WRITE) {
                    const uint64_t rev = bsm < halfM ? 1ull : 0ull;  // complement wins (binning.c:1029-1040)
                    const uint64_t e = (uint64_t)lo | (n << 16) | ((uint64_t)(sig - lo) << 22) | (rev << 28) |
                                       ((uint64_t)tid << 29) | ((uint64_t)(uint32_t)best << 38);
                    // one stage slot per record: one atomic per wave (the lanes
                    // still walking take consecutive slots) -- 512 lanes' atomics
                    // on the one LDS word serialised every segment round
                    uint64_t loc;
                    if (alloc) {
                        const uint64_t am = __ballot(1);
                        const int lead = __builtin_ctzll(am);
                        uint32_t wb = 0;
                        if ((int)(tid & 63u) == lead) wb = atomicAdd(&span_end, (uint32_t)__popcll(am));
                        wb = (uint32_t)__shfl((int)wb, lead, 64);
                        loc = (uint64_t)wb + __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
                    } else {
                        loc = rbase + nseg - bfirst;
                    }
                    if (loc < SK_STAGE) {
                        stg[loc] = e;
                    } else if (rounds) {
                        break;  // stage full: resume at this record in the next round
                    } else if (route) {  // many destinations: each piece its own slot
                        uint32_t d[2], sub[2];
                        int ne;
                        const uint32_t np_ = record_pieces(A, (uint32_t)best, lo, (int)n, sig - lo, rev != 0, sw, d, sub, ne);
                        for (uint32_t q = 0; q < np_; q++) {
                            const int cut = q ? ne : 0;
                            const uint64_t pn = np_ == 2 && q == 0 ? (uint64_t)ne : n - (uint64_t)cut;
                            const uint64_t i = atomicAdd(&A.dest_ctr[d[q]], 1ull);
                            if (i < region_room(A.region_base, A.region_cap, d[q]))
                                put_record(A, A.regions + (region_off(A.region_base, A.region_cap, d[q]) + i) * (uint64_t)A.rw,
                                           A.ord_base + (uint32_t)r, (uint64_t)(lo + cut), pn,
                                           (uint64_t)(sig - lo - cut), rev, sw, sub[q]);
                        }
                    }
                    if (loc >= SK_STAGE && !route && !alloc) {  // ordered records beyond the staging area: direct (scattered) stores
                        const uint64_t t = rbase + nseg;
                        A.pay[3 * t + 0] = (uint64_t)(A.ord_base + (uint32_t)r) | (n << 32) |
                                           ((uint64_t)(sig - lo) << 38) | (rev << 44) | ((uint64_t)lo << 45);
                        A.pay[3 * t + 1] = window64(sw, lo);
                        A.pay[3 * t + 2] = window64(sw, lo + 32);
                        A.keys[t] = ((uint64_t)(uint32_t)best << 38) | ((63ull - n) << 32) | (uint32_t)t;
                    }
                }
                kmers += n;
                nseg++;
                lo = nlo;
            }
            if (!WRITE && tid < nrows) A.seg_count[r] = nseg;
            if (WRITE && !alloc && nseg)
                atomicMax(&span_end, (uint32_t)min<uint64_t>(rbase + nseg - bfirst, SK_STAGE));
            if (!WRITE) break;
            __syncthreads();
            SKPROF(1);
            const uint32_t span = min(span_end, SK_STAGE);
            if (route) {
                // per destination: count, reserve a range, place (LDS cursors)
                for (uint32_t d = tid; d < (A.G + 1) / 2; d += SKT) dcnt2[d] = 0;
                __syncthreads();
                const bool agg = A.G <= 64;  // ranks, not local buckets: aggregate per wave
                const uint32_t half = 1u << (2 * M - 1);
                // two records per trip: both map loads in flight together
                for (uint32_t i0 = tid; i0 < span; i0 += 2 * SKT) {
                    const uint32_t i1 = i0 + SKT;
                    const bool v1 = i1 < span;
                    const uint64_t e0 = stg[i0], e1 = v1 ? stg[i1] : e0;
                    uint32_t me0 = 0, me1 = 0;
                    if (A.bucket_map) {  // (codes below half: no entry, record_plan hashes them)
                        const uint32_t c0 = (uint32_t)(e0 >> 38), c1 = (uint32_t)(e1 >> 38);
                        me0 = c0 >= half ? A.bucket_map[c0 - half] : 0u;
                        me1 = c1 >= half ? A.bucket_map[c1 - half] : 0u;
                    }
                    const uint64_t p0 = record_plan(A, e0, me0, smem + ((e0 >> 29) & 0x1FFu) * RS);
                    const uint64_t p1 = record_plan(A, e1, me1, smem + ((e1 >> 29) & 0x1FFu) * RS);
                    stg[i0] = p0;
                    if (v1) stg[i1] = p1;
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const uint64_t pl = u ? p1 : p0;
                        if (u && !v1) break;
                        const uint32_t np_ = 1u + (uint32_t)((pl >> 63) & 1u);
                        for (uint32_t q = 0; q < np_; q++) {
                            const uint32_t dq = (uint32_t)(pl >> (38 + 10 * q)) & 1023u;
                            if (agg)
                                wave_dest_add(dcnt2, dq);
                            else
                                atomicAdd(&dcnt2[dq >> 1], 1u << (16 * (dq & 1)));
                        }
                    }
                }
                __syncthreads();
                for (uint32_t d = tid; d < A.G; d += SKT) {
                    const uint32_t nd = (dcnt2[d >> 1] >> (16 * (d & 1))) & 0xFFFFu;
                    dbase[d] = nd ? (uint32_t)min<unsigned long long>(
                                        atomicAdd(&A.dest_ctr[d], (unsigned long long)nd), 0xFFFFFFFFull)
                                  : 0u;
                }
                __syncthreads();
                for (uint32_t d = tid; d < (A.G + 1) / 2; d += SKT) dcnt2[d] = 0;
                __syncthreads();
                SKPROF(2);
                for (uint32_t i = tid; i < span; i += SKT) {
                    const uint64_t e = stg[i];  // (planned)
                    const uint32_t row = (uint32_t)((e >> 29) & 0x1FFu);
                    const int lo = (int)(e & 0x1FFu), n = (int)((e >> 16) & 63u), so = (int)((e >> 22) & 63u);
                    const bool rev = ((e >> 28) & 1u) != 0;
                    const uint32_t b = (uint32_t)((e >> 9) & 7u), np_ = 1u + (uint32_t)((e >> 63) & 1u);
                    const int ne = (int)((e >> 58) & 31u);
                    const uint64_t* rw_ = smem + row * RS;
                    // the pieces' sub-bins (the stamp), from the read's bases in LDS
                    uint32_t sub[2] = {0u, 0u};
                    if (A.sub_stamp && b) {
                        const uint64_t w = window64(rw_, lo + so + M);
                        if (np_ == 2) sub[1] = sub_ctx(so - ne, K, M, b, w, rev);
                        else sub[0] = sub_ctx(so, K, M, b, w, rev);
                    }
                    for (uint32_t q = 0; q < np_; q++) {
                        const uint32_t dq = (uint32_t)(e >> (38 + 10 * q)) & 1023u;
                        const uint64_t slot =
                            (uint64_t)dbase[dq] +
                            (agg ? wave_dest_add(dcnt2, dq)
                                 : ((atomicAdd(&dcnt2[dq >> 1], 1u << (16 * (dq & 1))) >> (16 * (dq & 1))) & 0xFFFFu));
                        if (slot >= region_room(A.region_base, A.region_cap, dq)) continue;  // counted: the caller retries bigger
                        const int cut = q ? ne : 0;
                        const int pn = np_ == 2 && q == 0 ? ne : n - cut;
                        put_record(A, A.regions + (region_off(A.region_base, A.region_cap, dq) + slot) * (uint64_t)A.rw,
                                   A.ord_base + (uint32_t)(r0 + row), (uint64_t)(lo + cut), (uint64_t)pn,
                                   (uint64_t)(so - cut), rev ? 1u : 0u, rw_, sub[q]);
                    }
                }
            } else {
                if (alloc) {  // the block's staged records get one contiguous range
                    if (tid == 0) s_base = span ? atomicAdd(A.rec_ctr, (unsigned long long)span) : 0ull;
                    __syncthreads();
                }
                const uint64_t tbase = alloc ? (uint64_t)s_base : bfirst;
                for (uint32_t i = tid; i < span; i += SKT) {
                    const uint64_t e = stg[i];
                    const uint32_t elo = (uint32_t)(e & 0xFFFFu), row = (uint32_t)((e >> 29) & 0x1FFu);
                    const uint64_t en = (e >> 16) & 63u, so = (e >> 22) & 63u, rev = (e >> 28) & 1u;
                    const uint64_t* rw_ = smem + row * RS;
                    const uint64_t t = tbase + i;
                    A.pay[3 * t + 0] = (uint64_t)(A.ord_base + (uint32_t)(r0 + row)) | (en << 32) | (so << 38) |
                                       (rev << 44) | ((uint64_t)elo << 45);
                    A.pay[3 * t + 1] = window64(rw_, (int)elo);
                    A.pay[3 * t + 2] = window64(rw_, (int)elo + 32);
                    A.keys[t] = ((e >> 38) << 38) | ((63ull - en) << 32) | (uint32_t)t;
                }
            }
            // another round while a walk stopped at the full stage
#ifdef KB_BIN_PROF
            __syncthreads();
            SKPROF(3);
#endif
            if (!rounds || !__syncthreads_or(lo < nK)) break;
            if (tid == 0) span_end = 0;
            __syncthreads();
        }
    }
    if (!WRITE || (alloc && (!route || A.binned_fmt))) {  // per-block k-mer sums (sk_kmers_total_kernel)
        __shared__ unsigned long long shs;
        if (tid == 0) shs = 0;
        __syncthreads();
        uint64_t w = kmers;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) w += (uint64_t)__shfl_xor((long long)w, off, 64);
        if ((tid & 63u) == 0 && w) atomicAdd(&shs, (unsigned long long)w);
        __syncthreads();
        if (tid == 0) A.n_kmers[blockIdx.x] = shs;
    }
}

uint64_t sk_blocks(uint64_t n_reads, int RW) {
    if (!n_reads) return 0;
    if (RW <= SK_THREAD_RW) return std::min<uint64_t>((n_reads + SKT - 1) / SKT, 8192);
    return std::min<uint64_t>((n_reads + 3) / 4, 4096);
}

__global__ void sk_kmers_total_kernel(const unsigned long long* part, uint64_t n, unsigned long long* out) {
    __shared__ uint64_t sh[4];
    uint64_t v = 0;
    for (uint64_t i = threadIdx.x; i < n; i += 256) v += part[i];
    v = block_sum256(v, sh);
    if (threadIdx.x == 0) *out += v;
}

hipError_t launch_sk_kmers_total(const unsigned long long* part, uint64_t n, unsigned long long* out,
                                 hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(sk_kmers_total_kernel, dim3(1), dim3(256), 0, s, part, n, out);
    return hipGetLastError();
}

hipError_t launch_sk(const SkScanArgs& a, bool write, hipStream_t s) {
    if (!a.n_reads) return hipSuccess;
    const uint64_t blocks = sk_blocks(a.n_reads, a.RW);
    if (a.RW <= SK_THREAD_RW) {
        const size_t lds = (size_t)SKT * sk_row_words(a.RW, a.rw) * sizeof(uint64_t) +
                           (write ? SK_STAGE * sizeof(uint64_t) : 0);
        if (a.K < 2 * a.M) {  // (QK: the reference's incremental branch is live)
            if (write)
                hipLaunchKernelGGL((sk_thread_kernel<true, true>), dim3((unsigned)blocks), dim3(SKT), lds, s, a);
            else
                hipLaunchKernelGGL((sk_thread_kernel<false, true>), dim3((unsigned)blocks), dim3(SKT), lds, s, a);
        } else if (write) {
            hipLaunchKernelGGL(sk_thread_kernel<true>, dim3((unsigned)blocks), dim3(SKT), lds, s, a);
        } else {
            hipLaunchKernelGGL(sk_thread_kernel<false>, dim3((unsigned)blocks), dim3(SKT), lds, s, a);
        }
        return hipGetLastError();
    }
    const size_t lds = (size_t)4 * (a.RW + 2) * sizeof(uint64_t);
    if (a.K < 2 * a.M) {  // (QK: a long read's walk on one lane of its wave)
        if (write)
            hipLaunchKernelGGL((sk_kernel<true, true>), dim3((unsigned)blocks), dim3(256), lds, s, a);
        else
            hipLaunchKernelGGL((sk_kernel<false, true>), dim3((unsigned)blocks), dim3(256), lds, s, a);
    } else if (write) {
        hipLaunchKernelGGL(sk_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, s, a);
    } else {
        hipLaunchKernelGGL(sk_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

// records into bin order, structure of arrays (the bin kernel streams them)
__global__ __launch_bounds__(256) void sk_gather_kernel(const uint64_t* __restrict__ keys,
                                                        const uint64_t* __restrict__ pay, uint64_t R,
                                                        uint64_t* __restrict__ srec) {
    for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < R; k += (uint64_t)gridDim.x * 256) {
        const uint64_t t = (uint32_t)keys[k];
        const uint64_t hd = pay[3 * t], w0 = pay[3 * t + 1];
        reinterpret_cast<uint4*>(srec)[k] = make_uint4((uint32_t)hd, (uint32_t)(hd >> 32), (uint32_t)w0,
                                                        (uint32_t)(w0 >> 32));  // (header, word 0) pairs
        srec[2 * R + k] = pay[3 * t + 2];
    }
}

hipError_t launch_sk_gather(const uint64_t* keys, const uint64_t* pay, uint64_t R, uint64_t* srec,
                            hipStream_t s) {
    if (!R) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((R + 255) / 256, 8192);
    hipLaunchKernelGGL(sk_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, keys, pay, R, srec);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// routing (one process per GPU): the sender's records go to
// owner(mmer) in the routed record format of route_kernel (kbin_kernels.hip)
// -- header {id | i0 << 32 | n << 48 | sig_off << 54 | rev << 60}, then the
// span words (rev: kbin_internal.h ROUTED_REV_BIT) --
// destination-major, read order within a destination; the receiver turns
// them back into binned records.
// ---------------------------------------------------------------------------


__global__ __launch_bounds__(256) void route_dest_kernel(const uint64_t* __restrict__ keys, uint64_t R,
                                                         uint32_t G, const uint8_t* __restrict__ owner_map, int M,
                                                         uint64_t* __restrict__ dkeys,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ uint32_t hist[64];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t t = blockIdx.x * 256ull + threadIdx.x; t < R; t += (uint64_t)gridDim.x * 256) {
        const uint32_t mm = (uint32_t)(keys[t] >> 38);
        const uint32_t d = owner_map && bm_has_entry(mm, M) ? (uint32_t)owner_map[mm - (1u << (2 * M - 1))]
                                                            : owner_of_mmer(mm, G);
        dkeys[t] = ((uint64_t)d << 32) | (uint32_t)t;
        atomicAdd(&hist[d], 1u);
    }
    __syncthreads();
    if (threadIdx.x < G && hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

hipError_t launch_route_dest(const uint64_t* keys, uint64_t R, uint32_t G, const uint8_t* owner_map, int M,
                             uint64_t* dkeys,
                             unsigned long long* counts, hipStream_t s) {
    if (!R) return hipSuccess;
    if (G < 1 || G > 64) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((R + 255) / 256, 2048);
    hipLaunchKernelGGL(route_dest_kernel, dim3((unsigned)blocks), dim3(256), 0, s, keys, R, G, owner_map, M, dkeys, counts);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void route_pack_binned_kernel(const uint64_t* __restrict__ sorted,
                                                                const uint64_t* __restrict__ pay, uint64_t R,
                                                                int rw, const int32_t* __restrict__ read_ids,
                                                                uint32_t id_off, uint64_t* __restrict__ out) {
    for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < R; k += (uint64_t)gridDim.x * 256) {
        const uint64_t t = (uint32_t)sorted[k];
        const uint64_t hd = pay[3 * t];
        const uint32_t id = (uint32_t)id_of((uint32_t)hd, read_ids, id_off);
        const uint64_t n = (hd >> 32) & 63u, so = (hd >> 38) & 63u, lo = (hd >> 45) & 0xFFFFu, rev = (hd >> 44) & 1u;
        uint64_t* o = out + k * (uint64_t)rw;
        o[0] = (uint64_t)id | (lo << 32) | (n << 48) | (so << 54) | (rev << ROUTED_REV_BIT);
        o[1] = pay[3 * t + 1];
        if (rw >= 3) o[2] = pay[3 * t + 2];
        for (int w = 3; w < rw; w++) o[w] = 0;  // (K <= 31 spans fit two words)
    }
}

hipError_t launch_route_pack_binned(const uint64_t* sorted, const uint64_t* pay, uint64_t R, int rw,
                                    const int32_t* read_ids, uint32_t id_off, uint64_t* out,
                                    hipStream_t s) {
    if (!R) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((R + 255) / 256, 8192);
    hipLaunchKernelGGL(route_pack_binned_kernel, dim3((unsigned)blocks), dim3(256), 0, s, sorted, pay, R, rw,
                       read_ids, id_off, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void sk_convert_kernel(const uint64_t* __restrict__ recs, uint64_t n_rec,
                                                         int rw, uint64_t off, int M, int K, uint64_t* __restrict__ pay,
                                                         uint64_t* __restrict__ keys, uint32_t* status,
                                                         unsigned long long* n_kmers) {
    const uint32_t maskM = (1u << (2 * M)) - 1u;
    bool neg = false;
    uint64_t kmers = 0;
    for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n_rec; k += (uint64_t)gridDim.x * 256) {
        const uint64_t* r = recs + k * (uint64_t)rw;
        const uint64_t h = r[0];
        const uint64_t w0 = r[1], w1 = rw >= 3 ? r[2] : 0ull;
        const uint32_t id = (uint32_t)h;
        const uint64_t lo = (h >> 32) & 0xFFFFu, n = (h >> 48) & 63u, so = (h >> 54) & 63u;
        const uint32_t sm = (uint32_t)(span_window(w0, w1, 0ull, 0ull, (int)so) >> (64 - 2 * M));
        const bool rev = routed_rev(h, sm, K, M);  // complement wins (binning.c:1029-1040)
        const uint32_t canon = rev ? maskM - sm : sm;
        neg |= (int32_t)id < 0;
        const uint64_t t = off + k;
        pay[3 * t + 0] = (uint64_t)id | (n << 32) | (so << 38) | ((uint64_t)rev << 44) | (lo << 45);
        pay[3 * t + 1] = w0;
        pay[3 * t + 2] = w1;
        keys[t] = ((uint64_t)canon << 38) | ((63ull - n) << 32) | (uint32_t)t;
        kmers += n;
    }
    if (neg) atomicOr(status, ST_NEG_ID);
    __shared__ uint64_t sh[4];
    kmers = block_sum256(kmers, sh);
    if (threadIdx.x == 0 && kmers) atomicAdd(n_kmers, (unsigned long long)kmers);
}

hipError_t launch_sk_convert(const uint64_t* recs, uint64_t n_rec, int rw, uint64_t off, int M, int K,
                             uint64_t* pay, uint64_t* keys, uint32_t* status, unsigned long long* n_kmers,
                             hipStream_t s) {
    if (!n_rec) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n_rec + 255) / 256, 8192);
    hipLaunchKernelGGL(sk_convert_kernel, dim3((unsigned)blocks), dim3(256), 0, s, recs, n_rec, rw, off, M, K, pay,
                       keys, status, n_kmers);
    return hipGetLastError();
}

// The receiver's plan for PERT records of a block trip (record k0 + j * 256 +
// tid): the destination of its (last) piece, and of its edge piece when it is
// cut (ne > 0 k-mers), its pay-layout header and span words.  In phases, so
// that the record loads, then the map lookups, then the sub-bin lookups of all
// PERT records are in flight together (one record's chain of dependent global
// loads at a time left the kernel latency-bound).
template <int SPW, int PERT>
DEV void convert_plan(const uint64_t* __restrict__ recs, uint64_t n_rec, int rw, int M, uint32_t NB, int K,
                      const uint32_t* __restrict__ bucket_map, const uint16_t* __restrict__ sub_map, uint64_t k0,
                      uint32_t (&dst)[PERT], uint32_t (&dst2)[PERT], uint32_t (&ne)[PERT], uint32_t (&sub1)[PERT],
                      uint64_t (&pay0)[PERT], uint64_t (&ps)[PERT][SPW], bool& neg, uint64_t& kmers) {
    const uint32_t maskM = (1u << (2 * M)) - 1u, halfM = 1u << (2 * M - 1);
    uint32_t canon[PERT], me[PERT];
#pragma unroll
    for (int j = 0; j < PERT; j++) {
        const uint64_t k = k0 + (uint64_t)j * 256 + threadIdx.x;
        dst[j] = 0xFFFFFFFFu;
        ne[j] = 0;
        sub1[j] = 0;
        me[j] = 0;
        if (k >= n_rec) continue;
        const uint64_t* r = recs + k * (uint64_t)rw;
        pay0[j] = r[0];
#pragma unroll
        for (int w = 0; w < SPW; w++) ps[j][w] = w + 1 < rw ? r[w + 1] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < PERT; j++) {
        if (k0 + (uint64_t)j * 256 + threadIdx.x >= n_rec) continue;
        const uint64_t h = pay0[j];
        const uint32_t id = (uint32_t)h;
        const uint64_t lo = (h >> 32) & 0xFFFFu, n = (h >> 48) & 63u, so = (h >> 54) & 63u;
        // the signature (so <= 56) ends inside the first two span words
        const uint32_t sm = (uint32_t)(span_window(ps[j][0], ps[j][1], 0ull, 0ull, (int)so) >> (64 - 2 * M));
        const bool rev = routed_rev(h, sm, K, M);  // complement wins (binning.c:1029-1040)
        canon[j] = rev ? maskM - sm : sm;
        neg |= (int32_t)id < 0;
        kmers += n;
        pay0[j] = (uint64_t)id | (n << 32) | (so << 38) | ((uint64_t)rev << 44) | (lo << 45);
        dst[j] = 0;
    }
    if (bucket_map) {
#pragma unroll
        for (int j = 0; j < PERT; j++)
            // (K >= 2M: canon >= halfM by construction, the larger of a code and
            // its complement; K < 2M passes run without a map.  The guard bounds
            // the index whatever a received record says)
            if (dst[j] != 0xFFFFFFFFu) me[j] = canon[j] >= halfM ? bucket_map[canon[j] - halfM] : 0u;
#pragma unroll
        for (int j = 0; j < PERT; j++) {
            if (dst[j] == 0xFFFFFFFFu) continue;
            const uint32_t b = bm_depth(me[j]);
            if (!b) {
                dst[j] = me[j] & 1023u;
                continue;
            }
            const uint64_t h = pay0[j];
            const int n = (int)((h >> 32) & 63u), so = (int)((h >> 38) & 63u);
            const bool rev = ((h >> 44) & 1u) != 0;
            const int e = sub_edge(so, n, K, M, b);
            // the context at so + M: past the first two span words
            // when a long (K > 31) record's first k-mers are its edge
            const uint64_t wc = span_window(ps[j][0], ps[j][1], SPW > 2 ? ps[j][SPW > 2 ? 2 : 0] : 0ull,
                                            SPW > 3 ? ps[j][SPW > 3 ? 3 : 0] : 0ull, so + M);
            if (e > 0 && e < n) ne[j] = (uint32_t)e;
            sub1[j] = sub_ctx(so - (int)ne[j], K, M, b, wc, rev);
        }
#pragma unroll
        for (int j = 0; j < PERT; j++) {
            if (dst[j] == 0xFFFFFFFFu || !(me[j] & BM_SPLIT)) continue;
            const uint32_t off = me[j] & 0x0FFFFFFFu;
            dst[j] = sub_map[off + sub1[j]];
            if (ne[j]) dst2[j] = sub_map[off];
        }
    } else {
#pragma unroll
        for (int j = 0; j < PERT; j++)
            if (dst[j] != 0xFFFFFFFFu) dst[j] = dest_of(canon[j], NB, BUCKET_SALT);
    }
}

// the 1 + SPW words of one piece of a planned record: the edge piece (its
// first ne k-mers, same span start, sub-bin 0) or the (last) piece (k-mers
// ne.., span from base ne, signature ne closer, its sub-bin stamped)
template <int SPW>
DEV void convert_piece(uint64_t h, const uint64_t (&ps)[SPW], uint32_t ne, uint32_t sub1, uint64_t stamp, bool edge,
                       uint64_t (&o)[1 + SPW]) {
    if (edge) {
        o[0] = (h & ~(63ull << 32)) | ((uint64_t)ne << 32);
#pragma unroll
        for (int w = 0; w < SPW; w++) o[1 + w] = w + 1 == SPW ? ps[w] & ~stamp : ps[w];
    } else if (ne) {
        const uint64_t c = ne;
        const uint64_t n = (h >> 32) & 63u, so = (h >> 38) & 63u, lo = (h >> 45) & 0xFFFFu;
        o[0] = (h & 0xFFFFFFFFull) | ((n - c) << 32) | ((so - c) << 38) | (h & (1ull << 44)) | ((lo + c) << 45);
        const uint64_t sw[4] = {ps[0], ps[1], SPW > 2 ? ps[SPW > 2 ? 2 : 0] : 0ull, SPW > 3 ? ps[SPW > 3 ? 3 : 0] : 0ull};
#pragma unroll
        for (int w = 0; w < SPW; w++) {
            const uint64_t x = span_window(sw[0], sw[1], sw[2], sw[3], (int)c + 32 * w);
            o[1 + w] = w + 1 == SPW ? (x & ~stamp) | (sub1 & stamp) : x;
        }
    } else {
        o[0] = h;
#pragma unroll
        for (int w = 0; w < SPW; w++) o[1 + w] = w + 1 == SPW ? (ps[w] & ~stamp) | (sub1 & stamp) : ps[w];
    }
}

// received routed records -> local bucket regions (pay layout, ordinal = id,
// 1 + spw words); a block reserves one range per bucket for its 256 x 8
// records.  A split mmer's record goes to its context sub-bin's bucket, cut in
// two (edge piece first) when its first k-mers lie in the edge.
template <int SPW>
__global__ __launch_bounds__(256) void sk_convert_buckets_kernel(const uint64_t* __restrict__ recs, uint64_t n_rec,
                                                                 int rw, int M, uint32_t NB, int K,
                                                                 const uint32_t* __restrict__ bucket_map,
                                                                 const uint16_t* __restrict__ sub_map, int sub_stamp,
                                                                 uint64_t* __restrict__ regions, uint64_t cap,
                                                                 const uint64_t* __restrict__ rbase,
                                                                 unsigned long long* bfill, uint32_t* status,
                                                                 unsigned long long* n_kmers, int diag_group) {
    constexpr int PERT = 8;
#ifdef KB_BIN_ABL
    // (diagnostic builds only, KB_DIAG_CONVERT_GROUP: only the blocks of one
    // XCD group b % 8 == 0 convert their records -- the rest are dropped,
    // results wrong by design -- so a WRITE_SIZE pass can price cross-XCD
    // line sharing; ADVICE r04: never in the product library)
    if (diag_group && (blockIdx.x & 7u)) return;
#else
    (void)diag_group;
#endif
    __shared__ uint32_t cnt[SK_MAX_DEST];
    __shared__ unsigned long long base[SK_MAX_DEST];
    bool neg = false;
    uint64_t kmers = 0;
    const uint64_t stamp = sub_stamp ? SUB_MASK : 0ull;  // (a bucket record's last span word carries its sub-bin)
    for (uint64_t k0 = (uint64_t)blockIdx.x * 256 * PERT; k0 < n_rec; k0 += (uint64_t)gridDim.x * 256 * PERT) {
        for (uint32_t d = threadIdx.x; d < NB; d += 256) cnt[d] = 0;
        __syncthreads();
        uint32_t dst[PERT], dst2[PERT], ne[PERT], sub1[PERT];
        uint64_t pay0[PERT], ps[PERT][SPW];
        convert_plan<SPW, PERT>(recs, n_rec, rw, M, NB, K, bucket_map, sub_map, k0, dst, dst2, ne, sub1, pay0, ps,
                                neg, kmers);
#pragma unroll
        for (int j = 0; j < PERT; j++) {
            if (dst[j] == 0xFFFFFFFFu) continue;
            atomicAdd(&cnt[dst[j]], 1u);
            if (ne[j]) atomicAdd(&cnt[dst2[j]], 1u);
        }
        __syncthreads();
        for (uint32_t d = threadIdx.x; d < NB; d += 256) {
            base[d] = cnt[d] ? atomicAdd(&bfill[d], (unsigned long long)cnt[d]) : 0ull;
            cnt[d] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PERT; j++) {
            if (dst[j] == 0xFFFFFFFFu) continue;
            uint64_t o[1 + SPW];
            if (ne[j]) {  // the edge piece first
                const uint64_t slot = base[dst2[j]] + atomicAdd(&cnt[dst2[j]], 1u);
                if (slot < region_room(rbase, cap, dst2[j])) {
                    convert_piece<SPW>(pay0[j], ps[j], ne[j], sub1[j], stamp, true, o);
                    uint64_t* op = regions + (region_off(rbase, cap, dst2[j]) + slot) * (1 + SPW);
#pragma unroll
                    for (int w = 0; w <= SPW; w++) op[w] = o[w];
                }
            }
            const uint64_t slot = base[dst[j]] + atomicAdd(&cnt[dst[j]], 1u);
            if (slot >= region_room(rbase, cap, dst[j])) continue;  // counted: the caller retries bigger
            convert_piece<SPW>(pay0[j], ps[j], ne[j], sub1[j], stamp, false, o);
            uint64_t* op = regions + (region_off(rbase, cap, dst[j]) + slot) * (1 + SPW);
#pragma unroll
            for (int w = 0; w <= SPW; w++) op[w] = o[w];
        }
        __syncthreads();
    }
    if (neg) atomicOr(status, ST_NEG_ID);
    __shared__ uint64_t sh[4];
    kmers = block_sum256(kmers, sh);
    if (threadIdx.x == 0 && kmers) atomicAdd(n_kmers, (unsigned long long)kmers);
}

hipError_t launch_sk_convert_buckets(const uint64_t* recs, uint64_t n_rec, int rw, int spw, int M, uint32_t NB,
                                     int K, const uint32_t* bucket_map, const uint16_t* sub_map, int sub_stamp,
                                     uint64_t* regions, uint64_t cap, const uint64_t* rbase, unsigned long long* bfill,
                                     uint32_t* status, unsigned long long* n_kmers, hipStream_t s) {
    if (!n_rec) return hipSuccess;
    if (NB < 1 || NB > SK_MAX_DEST || (spw != 2 && spw != 4)) return hipErrorInvalidValue;
#ifdef KB_BIN_ABL
    static const int diag = getenv("KB_DIAG_CONVERT_GROUP") ? atoi(getenv("KB_DIAG_CONVERT_GROUP")) : 0;
#else
    const int diag = 0;
#endif
    const uint64_t blocks = std::min<uint64_t>((n_rec + 2047) / 2048, 4096);
    if (spw == 2)
        hipLaunchKernelGGL(sk_convert_buckets_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, recs, n_rec, rw, M,
                           NB, K, bucket_map, sub_map, sub_stamp, regions, cap, rbase, bfill, status, n_kmers, diag);
    else
        hipLaunchKernelGGL(sk_convert_buckets_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, recs, n_rec, rw, M,
                           NB, K, bucket_map, sub_map, sub_stamp, regions, cap, rbase, bfill, status, n_kmers, diag);
    return hipGetLastError();
}

#ifdef KB_BIN_PROF
void sk_prof_report() {
    unsigned long long g[8];
    (void)hipMemcpyFromSymbol(g, HIP_SYMBOL(g_sk_prof), sizeof(g));
    fprintf(stderr, "[sk_prof] rows=%llu walk=%llu counts=%llu place=%llu\n", g[0], g[1], g[2], g[3]);
    unsigned long long z8[8] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sk_prof), z8, sizeof(z8));
}
#endif

hipError_t load_sk_kernels() {
    return resolve_kernels({(const void*)sk_thread_kernel<true>, (const void*)sk_thread_kernel<false>,
                            (const void*)sk_kmers_total_kernel, (const void*)sk_convert_buckets_kernel<2>,
                            (const void*)sk_convert_buckets_kernel<4>});
}

}  // namespace kb

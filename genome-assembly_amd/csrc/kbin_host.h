// kbin_host.h -- private to the host side of the C-ABI (kbin_api.hip,
// kbin_route.hip, kbin_bmap.hip, kbin_finalize.hip): the context, its buffer
// types, error plumbing and the functions those files call across.  Not
// installed.  (Never includes kbin_device.h: the host side must not see the
// PROF-implies-ABL define.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/kbin.h"
#include "kbin_internal.h"
#include "kbin_hash.h"

using namespace kb;

namespace kb {
extern thread_local std::string g_err;  // this thread's kb_last_error() message (kbin_api.hip)
int fail(int code, const char* fmt, ...);
// (KB_DEBUG) host time in DevBuf allocations since the last report; per host
// thread (a multi-GPU group drives its contexts from one thread each)
extern thread_local double g_alloc_ms;
}  // namespace kb

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(_e == hipErrorOutOfMemory ? KB_ENOMEM : KB_EDEVICE, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                \
    } while (0)

inline double now_ms() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    uint64_t cap = 0;
    // Data-sized buffers (slack, the default) take 1/8 headroom, so passes
    // whose sizes wander by a few percent (the partitioned passes of one job,
    // records cut into sub-bins) do not free and map them afresh each pass: a
    // re-mapped allocation is cleared by the driver at roughly 20-25 GB/s (a
    // C3-sized stage regrown per pass cost seconds).  When the headroom does
    // not fit, the allocation is exact (no KB_ENOMEM from the headroom).
    // Fixed-size buffers (exact) allocate what they ask.
    hipError_t ensure(uint64_t n, bool slack = true) {
        if (n <= cap && p) return hipSuccess;
        const double t0 = now_ms();
        uint64_t want = std::max<uint64_t>(n, 1);
        if (slack) want += want / 8;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess && want > n) {  // no room for the headroom: exactly n
            (void)hipGetLastError();
            want = std::max<uint64_t>(n, 1);
            e = hipMalloc((void**)&p, want * sizeof(T));
        }
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        const double dt = now_ms() - t0;
        g_alloc_ms += dt;
        static const bool dbg = getenv("KB_DEBUG") && atoi(getenv("KB_DEBUG")) != 0;
        if (dbg && want * sizeof(T) >= (64u << 20))
            fprintf(stderr, "[kb] alloc %.1f MB in %.2f ms\n", (double)(want * sizeof(T)) / 1e6, dt);
        return e;
    }
    hipError_t ensure_exact(uint64_t n) { return ensure(n, false); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// host buffer, grown on demand: page-locked (full-rate DMA both ways) up to
// PIN_MAX_BYTES, else -- or when the pinned allocation fails -- pageable
// malloc memory (hipMemcpyAsync into it then completes synchronously).  Pinning
// only affects the copy rate, never the result.
constexpr uint64_t PIN_MAX_BYTES = 8ull << 30;
template <typename T>
struct PinBuf {
    T* p = nullptr;
    uint64_t cap = 0;
    bool pinned = false;
    hipError_t ensure(uint64_t n) {
        if (n <= cap && p) return hipSuccess;
        release();
        const uint64_t want = std::max<uint64_t>(n, 1) + std::max<uint64_t>(n, 1) / 8;
        if (want * sizeof(T) <= PIN_MAX_BYTES &&
            hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault) == hipSuccess) {
            pinned = true;
            cap = want;
            return hipSuccess;
        }
        (void)hipGetLastError();  // (a failed pinned allocation is not sticky)
        p = static_cast<T*>(malloc(want * sizeof(T)));
        if (!p) return hipErrorOutOfMemory;
        pinned = false;
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) {
            if (pinned) (void)hipHostFree(p);
            else free(p);
        }
        p = nullptr;
        cap = 0;
        pinned = false;
    }
};

// Bump allocator over device chunks for the read batches of one context
// (packed words, lengths, ids, k-mer offsets): kb_reset rewinds it and keeps
// the chunks, so a streaming job submits batch after batch without a
// hipMalloc / hipFree per batch.
struct DevPool {
    struct Chunk {
        uint8_t* p;
        uint64_t cap;
    };
    std::vector<Chunk> chunks;
    size_t cur = 0;
    uint64_t off = 0;
    template <typename T>
    hipError_t alloc(uint64_t n, T** out) {
        const uint64_t bytes = (std::max<uint64_t>(n, 1) * sizeof(T) + 255) & ~255ull;
        for (; cur < chunks.size(); cur++, off = 0)
            if (off + bytes <= chunks[cur].cap) {
                *out = reinterpret_cast<T*>(chunks[cur].p + off);
                off += bytes;
                return hipSuccess;
            }
        Chunk ch{nullptr, std::max<uint64_t>(bytes, 64ull << 20)};
        hipError_t e = hipMalloc((void**)&ch.p, ch.cap);
        if (e != hipSuccess) return e;
        chunks.push_back(ch);
        cur = chunks.size() - 1;
        off = bytes;
        *out = reinterpret_cast<T*>(ch.p);
        return hipSuccess;
    }
    void reset() {
        cur = 0;
        off = 0;
    }
    void release() {
        for (auto& ch : chunks) (void)hipFree(ch.p);
        chunks.clear();
        reset();
    }
};

// Host ingest: two staging slots, each a pinned buffer and its device twin
// (bases | offsets | ids).  kb_submit fills one slot while the other's H2D
// copy and pack kernel run; `done` (recorded after the slot's pack) gates its
// reuse, two submits later.
struct IngestSlot {
    PinBuf<uint8_t> h;
    DevBuf<uint8_t> d;
    hipEvent_t done = nullptr;
    bool used = false;
};

struct Batch {
    const uint64_t* words = nullptr;  // adopted or owned
    const uint32_t* lens = nullptr;
    uint64_t* own_words = nullptr;
    uint32_t* own_lens = nullptr;
    uint64_t* kmer_base = nullptr;  // owned, n_reads+1
    int32_t* ids = nullptr;         // owned, n_reads
    uint64_t n_reads = 0;
    int RW = 0;
    uint64_t ord_base = 0;
    uint64_t occ_base = 0;
    uint64_t n_occ = 0;
    bool affine = false;              // ids = first_id + r (no ids array until needed)
    bool have_occ = false;            // kmer_base / n_occ computed (batch_offsets)
    int64_t first_id = 0;
    // multi-GPU routing
    bool superkmers = false;          // a batch of received super-k-mer records
    const uint64_t* recs = nullptr;   // (superkmers) caller's device records
    uint32_t* rec_base = nullptr;     // (superkmers) owned, per-record occurrence base
    bool routed = false;              // (reads) shipped by kb_route_pack: not scanned here
    uint32_t* route_offs = nullptr;   // (reads) owned [G][n_reads]
    std::vector<uint64_t> route_tot;  // (reads) records per destination
};

struct kb_ctx {
    kb_params p{};
    int KW = 1;
    int dev = 0;
    hipStream_t s = nullptr;
    std::vector<Batch> batches;
    uint64_t n_reads = 0, n_occ = 0;
    uint32_t route_G = 0;  // destinations of the last kb_route_plan
    bool route_binned = false;  // the plan came from the super-k-mer record pass
    uint64_t route_R = 0;
    bool route_affine = false;
    int64_t route_id_c = 0;
    DevBuf<unsigned long long> rcount;  // records per destination
    // owner ranks of the canonical mmers per (n_dest, part, part_n) (owner_map_dev):
    // host copy (the upload's source stays alive) and device table
    std::map<uint64_t, std::pair<std::vector<uint8_t>, DevBuf<uint8_t>>> owners;

    // host ingest (kb_submit): double-buffered pinned staging, pooled batches
    IngestSlot ring[2];
    int ring_next = 0;
    DevPool pool;
    uint32_t* h_alpha = nullptr;  // pinned: the pack status word after each slot's pack
    bool alpha_bad = false;       // a submitted read had a byte outside ACGT (sticky until kb_reset)
    bool ingest_unchecked = false;  // host batches whose alphabet status is not read yet

    // finalize working set
    DevBuf<uint64_t> table;
    uint64_t slots = 0, learned_slots = 0;
    DevBuf<uint64_t> occ_a, occ_b;  // occurrence records, radix ping-pong
    uint64_t* sorted = nullptr;
    DevBuf<uint64_t> os_flags;        // onesweep look-back words
    DevBuf<uint32_t> os_aux;          // histograms/bases, tickets, error word
    uint32_t os_epoch = 0;
    DevBuf<int32_t> read_ids;
    DevBuf<uint32_t> starts;
    DevBuf<uint32_t> e_mmer, e_cnt;
    DevBuf<uint64_t> e_hi, e_lo, e_off;
    const uint64_t* e_hi_zeroed = nullptr;  // e_hi is all zero (one-word keys: bin_kernel leaves it alone)
    uint64_t e_hi_zeroed_cap = 0;           // (an allocation may come back at the same address)
    DevBuf<uint64_t> first, e_first;  // KB_TRACK_FIRST
    DevBuf<int32_t> ids_out;
    DevBuf<uint64_t> scratch;
    DevBuf<uint32_t> misc;    // [KB_MISC] status words and small counters: the M_* words (kbin_words.h)
    DevBuf<uint64_t> totals;  // [KB_TOTALS] the finalize's counters: the T_* words (kbin_words.h)
    // binned engine
    DevBuf<uint32_t> seg;      // super-k-mers per read -> exclusive scan
    DevBuf<uint64_t> pay;      // super-k-mer records, call order (3 words each)
    DevBuf<uint64_t> srec;     // the same, bin order, structure of arrays
    DevBuf<uint64_t> stage;    // per-occurrence (slot, ordinal) staging
    DevBuf<uint32_t> stage_ord;   // light bins: the stage as ordinals ...
    DevBuf<uint16_t> stage_slot;  // ... and LDS slots (6 B per occurrence)
    DevBuf<uint64_t> kstage;   // heavy bins: per-occurrence k-mer code + 1
    DevBuf<uint32_t> rrank, rord;  // ranked bins: record -> rank, rank -> ordinal (BinArgs::rank_mode)
    DevBuf<BinArgs> bargs;         // the bin kernels' arguments (launch_bins)
    DevBuf<uint32_t> long_q;   // entries with 257..4096 ids (lists_long_kernel)
    DevBuf<uint64_t> lq;       // list items for lists_kernel (BinArgs::lq_items); [0] the counter
    DevBuf<uint32_t> border;   // bin processing order
    DevBuf<uint4> bdesc;       // [2 max_bins] per processing slot: bin descriptor + stage base
    DevBuf<uint32_t> bcount, bmmer, bocc;  // bin descriptors (with starts); bocc: k-mers
    DevBuf<uint32_t> flat_list, flat_next, flat_l0, flat_off, flat_cur, flat_chunk, pool_bin, chunk_bin;  // heavy bins published for phase 1
    DevBuf<unsigned long long> flat_sbase, flat_obase, flat_n;  // flat_n: [KB_FLAT_N], the FN_* words
    DevBuf<unsigned long long> pstat;  // [KB_PSTAT] path counters of the bin kernels (BinArgs::pstat)
    DevBuf<uint64_t> regions;  // local bucket regions (pay layout)
    DevBuf<unsigned long long> bfill;  // records per bucket
    DevBuf<uint64_t> bbase;  // [NB + 1] bucket output bases (bucket_bases_kernel)
    DevBuf<uint64_t> rbase;  // [NB + 1] exact region bases (a pass without a learned map)
    bool rexact = false;     // the regions of the last record pass use rbase
    uint64_t bucket_cap_used = 0;  // the region stride (records per bucket) the regions were written with
    DevBuf<uint64_t> kpart;    // per-block k-mer sums of the count pass
    int ocut_km = -1;          // (K << 8 | M) the offset cut table was made for
    uint8_t ocut[5][17] = {};  // offset partitions' ranges (offset_cuts)
    float rho = 0.f;           // learned distinct / occurrences
    float rho_tab = 0.f;       // learned table keys / occurrences under the singleton pre-filter
    bool pfl_regime = false;   // (sticky) a finalize ran light pre-filtered bins: sub-bins sized for the sketch
    bool rank_regime = false;  // (sticky) a finalize ranked bins (long lists): smaller sub-bins, so more get ranked
    DevBuf<uint32_t> hll;      // cold pass: HyperLogLog registers (launch_hll)
    bool bucket_failed = false;  // a bucket overflowed its mmer map: radix path from now on
    bool prior_off = false;      // a prior map overflowed a bucket: hash routing for first passes
    uint64_t n_occ_entries_hint = 0;  // entries of the last finalize (lists grid)
    uint64_t ecap_hint = 0;    // entry capacity for the next binned finalize
    uint32_t part = 0, part_n = 1;  // kb_set_partition: this pass's mmer partition
    // balanced local buckets: records per canonical mmer seen in earlier passes,
    // and one device map (mmer -> bucket) per (part, part_n) key
    std::vector<double> prior_p;   // bmap_prior's weight shape ((i + 1) / half)^(K - M) per canonical mmer
    std::vector<uint32_t> mmer_w;  // records per canonical mmer (all its sub-bins)
    std::vector<uint64_t> mmer_o;  // k-mer occurrences per canonical mmer
    std::unordered_map<uint64_t, uint32_t> sub_w;  // (mmer << 16 | sub-bin) -> records, split mmers of the last pass
    struct BucketMap {
        uint64_t key = 0;
        uint32_t nb = 0;
        bool stale = false;
        uint64_t want_max = 0;  // the largest bucket load the packing expects (records)
        uint64_t want_tot = 0;
        uint64_t cap = 0;       // region stride of this key's passes (records per bucket)
        uint32_t split = 0;     // mmers split into context sub-bins
        std::vector<uint32_t> h_map;  // host copy of map
        // a pass's descriptors waiting to rebuild this map (bmap_apply)
        bool pending = false;
        std::vector<uint32_t> p_mm, p_cnt, p_occ;
        double p_rho = 0;
        DevBuf<uint32_t> map;   // per canonical mmer (bm_* in kbin_internal.h)
        DevBuf<uint16_t> sub;   // buckets of the split mmers' sub-bins
    };
    std::vector<BucketMap> bmaps;
    uint64_t* h_totals = nullptr;  // pinned [KB_TOTALS]: totals read back (and HT_SCAN_R)
    uint32_t* h_misc = nullptr;    // pinned [KB_MISC]: misc read back (and HM_RADIX_ERR)

    // results
    bool finalized = false;
    uint64_t n_entries = 0, n_ids = 0, n_distinct = 0;
    PinBuf<uint32_t> h_mmer, h_cnt;  // pinned: kb_export's D2H at full rate
    PinBuf<uint64_t> h_hi, h_lo, h_off, h_first;
    PinBuf<int32_t> h_ids;
    PinBuf<uint32_t> h_bins;  // a pass's bin descriptors for map learning (mmer | sub, records, occurrences)
    PinBuf<uint8_t> map_stage;  // bucket map uploads (bmap_build)
    hipEvent_t map_done = nullptr;
    bool map_stage_used = false;
    // the bucket ordering launched before the mid-finalize wait (spec_bucket_phase)
    hipEvent_t ev_mid = nullptr;
    bool spec = false;
    uint64_t spec_rlay = 0, spec_bins = 0, prev_R = 0;
    bool exported = false;

    // timing
    int timing = 0;  // KB_TIMING_ALL / KB_TIMING_KERNEL (kb_set_timing)
    kb_timing tm{};
    uint32_t nbins_hint = 0;  // bins of the last binned finalize (flat-list threshold)
    // grid hints for kernels that usually have nothing to do (~0: not seen yet)
    uint64_t hint_heavy = ~0ull, hint_lq = ~0ull, hint_long[2] = {~0ull, ~0ull};
    uint64_t hint_entries = 0, hint_ids = 0;  // the last finalize's entries and ids (kb_reset keeps them)
    double t_fin = 0;  // (KB_DEBUG) host time the finalize started
    bool alpha_dirty = false;  // a pack kernel may have set the sticky alphabet status since it was cleared
    hipEvent_t ev[8] = {};
};

// phase events: every mode on the table engine; the binned engine's
// KB_TIMING_KERNEL records only the two events around bin_kernel (each event
// record leaves the GPU idle some 5 us: seven of them cost ~35 us per C2 step)
#define REC(i) \
    do {                                                                                     \
        if (c->timing == KB_TIMING_ALL || (c->timing && c->tm.engine == KB_ENG_TABLE))      \
            HIPCHK(hipEventRecord(c->ev[i], c->s));                                          \
    } while (0)

// words per routed super-k-mer record: header + span of n + K - 1 <= 2K - M bases
inline int rec_words(const kb_ctx* c) { return 1 + (2 * c->p.K - c->p.M + 31) / 32; }

inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// KB_DEBUG=1: one stderr line per host-side event of a finalize (diagnostics)
#define KB_DBG(...)                                             \
    do {                                                        \
        static const bool _on = env_int("KB_DEBUG", 0) != 0;    \
        if (_on) fprintf(stderr, "[kb] " __VA_ARGS__);          \
    } while (0)

// the binned engine (kbin_sk.hip, kbin_plan.hip, kbin_bins.hip, kbin_lists.hip) serves K <= 63 unless the table engine is
// forced (flag, or KB_ENGINE=table).  Two-word k-mers (K > 31) take only its
// bucketed record path: reads of <= 512 bp (or received super-k-mers), no
// forced radix path, and no bucket overflow so far -- elsewhere the table
// engine bins them.
inline bool binned_applies(const kb_ctx* c) {
    if (c->p.flags & KB_ENGINE_TABLE) return false;
    if (!(c->p.flags & KB_ENGINE_BINNED)) {
        const char* e = getenv("KB_ENGINE");
        if (e && strcmp(e, "table") == 0) return false;
    }
    if (c->KW == 1) return true;
    if (c->bucket_failed || env_int("KB_BIN_RADIX", 0)) return false;
    for (auto& b : c->batches)
        if (!b.routed && !b.superkmers && b.RW > 16) return false;
    return true;
}

namespace kb {
// kbin_api.hip
int set_device(kb_ctx* c);
int ingest_check(kb_ctx* c, bool sync);
int batch_ids(kb_ctx* c, Batch& b);
int read_id_map(kb_ctx* c, bool& affine, int64_t& id_c);
// kbin_bmap.hip
uint64_t bmap_key(const kb_ctx* c);
kb_ctx::BucketMap* bmap_find(kb_ctx* c, uint32_t NB);
uint64_t bin_budget(const kb_ctx* c, uint32_t NB);
bool bmap_wants(kb_ctx* c, uint32_t NB, uint64_t R);
int bmap_apply(kb_ctx* c, uint32_t NB, const uint32_t* mm, const uint32_t* cnt, const uint32_t* occ, uint64_t nbins,
               double rho);
int bmap_prior(kb_ctx* c, uint32_t NB);
// kbin_finalize.hip
int binned_read_records(kb_ctx* c, uint64_t& R, uint64_t& N, bool ordered);
int finalize_binned(kb_ctx* c, int prune, bool affine, int64_t id_c, bool received);
}  // namespace kb

// kbin_plan.hip -- around the bin kernels of the binned engine: the bucket
// ordering (records of the local buckets into bin order, the bin descriptors),
// the bins' processing order and plan, and the finalize's small bookkeeping
// kernels (bucket stats, totals, counter clears).
#include <algorithm>

#include "kbin_internal.h"
#include "kbin_device.h"

namespace kb {

// Bin processing order: descending records (longest-processing-time first
// for the persistent blocks; a bin's cost follows its super-k-mers).  One
// block; counting sort over 8 classes per power of two (class = log2 of the
// count with 3 fractional bits), largest class first.
DEV uint32_t order_class(uint32_t c) {
    if (c < 8) return c;
    const uint32_t msb = 31u - (uint32_t)__clz(c);
    return msb * 8u + ((c >> (msb - 3u)) & 7u);  // <= 255
}

__global__ __launch_bounds__(1024) void bins_order_kernel(const uint32_t* __restrict__ bcount,
                                                          const uint64_t* __restrict__ totals,
                                                          uint32_t* __restrict__ order, uint64_t max_bins) {
    constexpr uint32_t NC = 256;
    __shared__ uint32_t hist[NC];
    const uint32_t nbins = (uint32_t)min(totals[T_BINS], max_bins);
    for (uint32_t i = threadIdx.x; i < NC; i += 1024) hist[i] = 0;
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += 1024) atomicAdd(&hist[order_class(bcount[b])], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {  // exclusive offsets, largest class first
        uint32_t acc = 0;
        for (int c = NC - 1; c >= 0; c--) {
            const uint32_t h = hist[c];
            hist[c] = acc;
            acc += h;
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += 1024) order[atomicAdd(&hist[order_class(bcount[b])], 1u)] = b;
}

hipError_t launch_bins_order(const uint32_t* bcount, const uint64_t* totals, uint32_t* order, uint64_t max_bins,
                             hipStream_t s) {
    hipLaunchKernelGGL(bins_order_kernel, dim3(1), dim3(1024), 0, s, bcount, totals, order, max_bins);
    return hipGetLastError();
}

// one descriptor per processing slot: {bin, first record, records, mmer},
// {occurrences, stage base lo, hi, 0}; stage bases are the exclusive prefix of
// the occurrences in processing order (each bin's range, as the stage counter
// handed them out before)
__global__ __launch_bounds__(1024) void bins_desc_kernel(const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ bstart,
                                                         const uint32_t* __restrict__ bcount,
                                                         const uint32_t* __restrict__ bmmer,
                                                         const uint32_t* __restrict__ bocc,
                                                         const uint64_t* __restrict__ totals, uint64_t max_bins,
                                                         uint4* __restrict__ desc, unsigned long long* stage_ctr) {
    __shared__ uint64_t red[16];
    const uint32_t nbins = (uint32_t)min(totals[T_BINS], max_bins);
    const uint32_t per = (nbins + 1023u) / 1024u, i0 = threadIdx.x * per;
    uint64_t mine = 0;
    for (uint32_t k = 0; k < per; k++)
        if (i0 + k < nbins) mine += bocc[order[i0 + k]];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t inc = wave_incl_scan(mine, lane);
    if (lane == 63) red[wid] = inc;
    __syncthreads();
    uint64_t run = inc - mine;
    for (int w = 0; w < 16; w++)
        if (w < wid) run += red[w];
    for (uint32_t k = 0; k < per; k++) {
        const uint32_t i = i0 + k;
        if (i >= nbins) break;
        const uint32_t b = order[i];
        const uint32_t occ = bocc[b];
        desc[2 * (uint64_t)i] = make_uint4(b, bstart[b], bcount[b], bmmer[b]);
        desc[2 * (uint64_t)i + 1] = make_uint4(occ, (uint32_t)run, (uint32_t)(run >> 32), 0u);
        run += occ;
    }
    // bins without a count (spread runs: bocc 0) take their stage ranges from
    // the stage counter, after every described range
    if (threadIdx.x == 1023) *stage_ctr = run;
}

hipError_t launch_bins_desc(const uint32_t* order, const uint32_t* bstart, const uint32_t* bcount,
                            const uint32_t* bmmer, const uint32_t* bocc, const uint64_t* totals, uint64_t max_bins,
                            uint4* desc, unsigned long long* stage_ctr, hipStream_t s) {
    hipLaunchKernelGGL(bins_desc_kernel, dim3(1), dim3(1024), 0, s, order, bstart, bcount, bmmer, bocc, totals,
                       max_bins, desc, stage_ctr);
    return hipGetLastError();
}

// bins_order_kernel and bins_desc_kernel in one launch: the class histogram,
// the processing order (kept in LDS up to PLAN_LDS bins, else re-read from
// `order`), then the descriptors in rounds of 1024 processing slots (a block
// scan of the occurrences per round carries the stage base) -- coalesced
// descriptor stores and independent gathers, where bins_desc_kernel walked
// each thread's range of slots one dependent load after another
constexpr uint32_t PLAN_LDS = 8192;
__global__ __launch_bounds__(1024) void bins_plan_kernel(const uint32_t* __restrict__ bstart,
                                                         const uint32_t* __restrict__ bcount,
                                                         const uint32_t* __restrict__ bmmer,
                                                         const uint32_t* __restrict__ bocc,
                                                         const uint64_t* __restrict__ totals, uint64_t max_bins,
                                                         uint32_t* __restrict__ order, uint4* __restrict__ desc,
                                                         unsigned long long* stage_ctr) {
    constexpr uint32_t NC = 256;
    __shared__ uint32_t hist[NC];
    __shared__ uint32_t ordl[PLAN_LDS];
    __shared__ uint64_t red[16];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wid = (int)(t >> 6);
    const uint32_t nbins = (uint32_t)min(totals[T_BINS], max_bins);
    if (t < NC) hist[t] = 0;
    __syncthreads();
    for (uint32_t b = t; b < nbins; b += 1024) atomicAdd(&hist[order_class(bcount[b])], 1u);
    __syncthreads();
    // exclusive offsets, largest class first: thread t < 256 holds class 255 - t
    {
        const uint32_t h = t < NC ? hist[NC - 1u - t] : 0u;
        const uint64_t inc = wave_incl_scan((uint64_t)h, lane);
        if (lane == 63 && wid < 4) red[wid] = inc;
        __syncthreads();
        uint64_t wp = 0;
        for (int w = 0; w < wid && w < 4; w++) wp += red[w];
        if (t < NC) hist[NC - 1u - t] = (uint32_t)(wp + inc - h);
        __syncthreads();
    }
    const bool in_lds = nbins <= PLAN_LDS;
    for (uint32_t b = t; b < nbins; b += 1024) {
        const uint32_t pos = atomicAdd(&hist[order_class(bcount[b])], 1u);
        order[pos] = b;
        if (in_lds) ordl[pos] = b;
    }
    __threadfence_block();
    __syncthreads();
    uint64_t carry = 0;
    // (each round's four descriptor gathers are issued a round ahead: the
    // rounds' scans no longer wait for their loads one after another)
    auto gather = [&](uint32_t i, uint32_t& occ, uint4& d0) {
        const bool v = i < nbins;
        const uint32_t b = v ? (in_lds ? ordl[i] : order[i]) : 0u;
        occ = v ? bocc[b] : 0u;
        d0 = v ? make_uint4(b, bstart[b], bcount[b], bmmer[b]) : make_uint4(0u, 0u, 0u, 0u);
    };
    uint32_t occ_n = 0;
    uint4 d0_n = make_uint4(0u, 0u, 0u, 0u);
    gather(t, occ_n, d0_n);
    for (uint32_t base = 0; base < nbins; base += 1024) {
        const uint32_t i = base + t;
        const bool v = i < nbins;
        const uint32_t occ = occ_n;
        const uint4 d0 = d0_n;
        if (base + 1024 < nbins) gather(base + 1024 + t, occ_n, d0_n);
        const uint64_t inc = wave_incl_scan((uint64_t)occ, lane);
        if (lane == 63) red[wid] = inc;
        __syncthreads();
        uint64_t wp = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            if (w < wid) wp += red[w];
            tot += red[w];
        }
        const uint64_t run = carry + wp + inc - occ;
        if (v) {
            desc[2 * (uint64_t)i] = d0;
            desc[2 * (uint64_t)i + 1] = make_uint4(occ, (uint32_t)run, (uint32_t)(run >> 32), 0u);
        }
        carry += tot;
        __syncthreads();  // (red is the next round's)
    }
    // bins without a count (bocc 0) take their stage ranges from the stage
    // counter, after every described range
    if (t == 0) *stage_ctr = carry;
}

hipError_t launch_bins_plan(const uint32_t* bstart, const uint32_t* bcount, const uint32_t* bmmer,
                            const uint32_t* bocc, const uint64_t* totals, uint64_t max_bins, uint32_t* order,
                            uint4* desc, unsigned long long* stage_ctr, hipStream_t s) {
    hipLaunchKernelGGL(bins_plan_kernel, dim3(1), dim3(1024), 0, s, bstart, bcount, bmmer, bocc, totals, max_bins,
                       order, desc, stage_ctr);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void bins_describe_kernel(const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ starts,
                                                            const uint64_t* __restrict__ totals,
                                                            uint32_t* __restrict__ bcount,
                                                            uint32_t* __restrict__ bmmer, uint64_t max_bins) {
    const uint64_t nbins = min(totals[T_BINS], max_bins);
    for (uint64_t b = blockIdx.x * 256ull + threadIdx.x; b < nbins; b += (uint64_t)gridDim.x * 256) {
        bcount[b] = starts[b + 1] - starts[b];
        bmmer[b] = (uint32_t)(keys[starts[b]] >> 38);
    }
}

hipError_t launch_bins_describe(const uint64_t* keys, const uint32_t* starts, const uint64_t* totals,
                                uint32_t* bcount, uint32_t* bmmer, uint64_t max_bins, hipStream_t s) {
    const uint64_t blocks = std::min<uint64_t>((max_bins + 255) / 256, 1024);
    hipLaunchKernelGGL(bins_describe_kernel, dim3((unsigned)std::max<uint64_t>(blocks, 1)), dim3(256), 0, s, keys,
                       starts, totals, bcount, bmmer, max_bins);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// bucket_kernel: one workgroup per local bucket.  The bucket's records (pay
// layout, contiguous) are read twice: pass 1 maps each record's mmer to a
// slot of a small LDS table and counts (slot, 63 - n); a block scan turns the
// counts into positions; pass 2 places every record (SoA) so that each bin is
// contiguous with its longest records first.  Bins are appended to the bin
// descriptors.  Replaces a global radix sort + gather: no random reads, one
// bucket per workgroup.
// ---------------------------------------------------------------------------
#ifndef KB_BK_THREADS
#define KB_BK_THREADS 1024  // (C2 1.784 -> 1.752 ms, profiles/r06/ab_bkt/)
#endif
constexpr int BK_THREADS = KB_BK_THREADS;  // (A/B builds: -DKB_BK_THREADS)
constexpr uint32_t BK_SLOTS = 256;  // mmers per bucket (a bucket with more is reported)

// a bucket's bins: key (mmer << SUB_BITS | context sub-bin) + 1 in an LDS table
DEV int bk_slot(uint32_t* keys, uint32_t bkey, bool insert) {
    const uint32_t k = bkey + 1u;
    uint32_t i = (uint32_t)((mix64((uint64_t)bkey) >> 32) & (BK_SLOTS - 1));
    for (uint32_t p = 0; p < BK_SLOTS; p++) {
        const uint32_t v = keys[i];
        if (v == k) return (int)i;
        if (v == 0) {
            if (!insert) return -1;
            const uint32_t old = atomicCAS(&keys[i], 0u, k);
            if (old == 0 || old == k) return (int)i;
        }
        i = (i + 1) & (BK_SLOTS - 1);
    }
    return -1;
}

// ROWS = k-mers per record rounded up to a power of two: n <= K - M + 1
// (<= 31 for K <= 31, <= 57 for K <= 63); row ROWS - n puts longest first.
// The bin key: canonical mmer << SUB_BITS | the piece's context sub-bin (0
// unless the map splits the mmer; the record pass cut every piece to one side)
template <int ROWS>
DEV void bk_decode(uint64_t h, uint64_t a, uint64_t b, uint64_t last, const BucketArgs& A, uint32_t& bkey,
                   uint32_t& row) {
    const int M = A.M;
    const uint32_t maskM = (1u << (2 * M)) - 1u;
    const int so = (int)((h >> 38) & 63u);
    const uint32_t sm = (uint32_t)(span_window(a, b, 0ull, 0ull, so) >> (64 - 2 * M));
    const uint32_t canon = ((h >> 44) & 1u) ? maskM - sm : sm;
    const uint32_t sub = A.sub ? (uint32_t)(last & SUB_MASK) : 0u;  // (stamped by the record pass)
    bkey = (canon << SUB_BITS) | sub;
    row = (uint32_t)ROWS - (uint32_t)((h >> 32) & 63u);
}

// SPW span words per record (2: K <= 31, 4: K <= 63)
template <int SPW>
__global__ __launch_bounds__(BK_THREADS) void bucket_kernel(BucketArgs A) {
    constexpr uint32_t ROWS = SPW == 2 ? 32 : 64;
    __shared__ uint32_t keys[BK_SLOTS];
    __shared__ uint32_t hist[BK_SLOTS * ROWS];  // (slot, ROWS - n) counts, then cursors
    __shared__ uint64_t red[BK_THREADS / 64];
    __shared__ unsigned long long s_base, s_bin;
    __shared__ uint32_t s_full;
    __shared__ uint32_t socc[BK_SLOTS];  // occurrences (k-mers) per slot
    const uint32_t tid = threadIdx.x, bk = blockIdx.x;
    const uint64_t cnt = min<uint64_t>(A.bfill[bk], region_room(A.rbase, A.cap, bk));
    constexpr int RWD = 1 + SPW;  // record words
    const uint64_t* src = A.regions + region_off(A.rbase, A.cap, bk) * RWD;
    for (uint32_t i = tid; i < BK_SLOTS; i += BK_THREADS) keys[i] = 0;
    for (uint32_t i = tid; i < BK_SLOTS * ROWS; i += BK_THREADS) hist[i] = 0;
    if (tid == 0) s_full = 0;
    __syncthreads();
#ifndef KB_BK_U
#define KB_BK_U 12  // (records in flight: 4 -> 8 C2 1.809 -> 1.796 ms at 512 threads, profiles/r06/ab_bku/; 12 at 1024 threads, ab_bku3/)
#endif
#ifndef KB_BK_U4
#define KB_BK_U4 4  // (C5 share 491.6 -> 489.2 ms, profiles/r06/ab_rows/)
#endif
    constexpr int U = SPW == 2 ? KB_BK_U : KB_BK_U4;  // records in flight per thread (A/B builds: -DKB_BK_U, -DKB_BK_U4)
    for (uint64_t i0 = tid; i0 < cnt; i0 += U * BK_THREADS) {
        uint64_t h[U], a[U], b[U], z[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = i0 + (uint64_t)u * BK_THREADS;
            if (i < cnt) {
                h[u] = src[RWD * i];
                a[u] = src[RWD * i + 1];
                b[u] = src[RWD * i + 2];
                z[u] = SPW == 2 ? b[u] : (A.sub ? src[RWD * i + SPW] : 0ull);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (i0 + (uint64_t)u * BK_THREADS >= cnt) break;
            uint32_t bkey, row;
            bk_decode<ROWS>(h[u], a[u], b[u], z[u], A, bkey, row);
            const int sl = bk_slot(keys, bkey, true);
            if (sl < 0) s_full = 1;
            else atomicAdd(&hist[sl * ROWS + row], 1u);
        }
    }
    __syncthreads();
    if (s_full) {  // uniform
        if (tid == 0) atomicOr(A.status, ST_BUCKET_FULL);
        return;
    }
    // exclusive scan of the counters in (slot, row) order
    constexpr uint32_t PER = BK_SLOTS * ROWS / BK_THREADS;
    static_assert(ROWS % PER == 0, "a thread's counters lie in one slot");
    uint32_t loc[PER];
    uint64_t mine = 0;
    uint32_t kmers = 0;  // this thread's slot: k-mers = records x n, n = ROWS - row
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        loc[k] = hist[tid * PER + k];
        mine += loc[k];
        kmers += loc[k] * (ROWS - (tid * PER + k) % ROWS);
    }
    if (tid < BK_SLOTS) socc[tid] = 0;
    __syncthreads();
    if (kmers) atomicAdd(&socc[(tid * PER) / ROWS], kmers);
    const int lane = tid & 63, wid = tid >> 6;
    const uint64_t inc = wave_incl_scan(mine, lane);
    if (lane == 63) red[wid] = inc;
    __syncthreads();
    uint64_t wp = 0;
    for (int w = 0; w < wid; w++) wp += red[w];
    uint32_t run = (uint32_t)(wp + inc - mine);
    if (tid == 0) s_base = A.bbase[bk];  // exclusive prefix of the fills
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        const uint32_t c = loc[k];
        hist[tid * PER + k] = run;
        run += c;
    }
    __syncthreads();
    // count non-empty slots, reserve bin descriptors (one per bin key: an
    // mmer, or one context sub-bin of a split mmer)
    // (the dense index of a slot among the non-empty ones, from the waves'
    // ballots -- a thread counting the set slots below it walked up to 255
    // LDS words in series)
    const bool has = tid < BK_SLOTS && keys[tid] != 0;
    const uint64_t hb = __ballot(has);
    __shared__ uint32_t wset[BK_SLOTS / 64];
    if (tid < BK_SLOTS && lane == 0) wset[wid] = (uint32_t)__popcll(hb);
    __syncthreads();
    uint32_t nb = 0, below = (uint32_t)__popcll(hb & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < (int)(BK_SLOTS / 64); w++) {
        if (w < wid) below += wset[w];
        nb += wset[w];
    }
    if (tid == 0) s_bin = nb ? atomicAdd(A.bin_ctr, (unsigned long long)nb) : 0ull;
    __syncthreads();
    if (has) {
        const uint64_t bi = s_bin + below;
        const uint32_t first = hist[tid * ROWS];
        const uint32_t last = tid + 1 < BK_SLOTS ? hist[(tid + 1) * ROWS] : (uint32_t)cnt;
        if (bi < A.max_bins) {
            A.bstart[bi] = (uint32_t)s_base + first;
            A.bcount[bi] = last - first;
            // the mmer, and its context sub-bin above bit 16 (bin_kernel masks
            // it off; the host learns each sub-bin's records from it)
            A.bmmer[bi] = ((keys[tid] - 1u) >> SUB_BITS) | (((keys[tid] - 1u) & ((1u << SUB_BITS) - 1u)) << 16);
            if (A.bocc) A.bocc[bi] = socc[tid];
        }
    }
    __syncthreads();
    const uint64_t base = s_base;
#ifdef KB_BIN_ABL
    if (A.ablate == 2) return;
#endif
    for (uint64_t i0 = tid; i0 < cnt; i0 += U * BK_THREADS) {
        uint64_t h[U], a[U], b[U], c[U], d[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = i0 + (uint64_t)u * BK_THREADS;
            if (i < cnt) {
                h[u] = src[RWD * i];
                a[u] = src[RWD * i + 1];
                b[u] = src[RWD * i + 2];
                if constexpr (SPW == 4) {
                    c[u] = src[RWD * i + 3];
                    d[u] = src[RWD * i + 4];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (i0 + (uint64_t)u * BK_THREADS >= cnt) break;
            uint32_t bkey, row;
            bk_decode<ROWS>(h[u], a[u], b[u], SPW == 2 ? b[u] : d[u], A, bkey, row);
            const int sl = bk_slot(keys, bkey, false);
            const uint64_t pos = base + atomicAdd(&hist[sl * ROWS + row], 1u);
            if (A.rcap && pos >= A.rcap) continue;  // (a speculative launch's layout is too small: rerun)
#ifdef KB_BIN_ABL
            if (A.ablate == 1) {
                if (pos == ~0ull) A.hdr[0] = h[u] ^ a[u] ^ b[u];  // (keeps the loads alive)
                continue;
            }
#endif
            reinterpret_cast<uint4*>(A.hdr)[pos] = make_uint4((uint32_t)h[u], (uint32_t)(h[u] >> 32), (uint32_t)a[u],
                                                              (uint32_t)(a[u] >> 32));
            if constexpr (SPW == 2) {
                A.w1[pos] = b[u];
            } else {
                reinterpret_cast<uint4*>(A.w1)[pos] = make_uint4((uint32_t)b[u], (uint32_t)(b[u] >> 32), (uint32_t)c[u],
                                                                 (uint32_t)(c[u] >> 32));
                A.w3[pos] = d[u];
            }
        }
    }
}

// exclusive prefix of the bucket fills (clamped to the capacity) -> bbase[NB + 1]
__global__ __launch_bounds__(1024) void bucket_bases_kernel(const unsigned long long* __restrict__ bfill, uint64_t cap,
                                                          const uint64_t* __restrict__ rbase, uint32_t NB,
                                                          uint64_t* __restrict__ bbase) {
    __shared__ uint64_t red[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t v = threadIdx.x < NB ? min<uint64_t>(bfill[threadIdx.x], region_room(rbase, cap, threadIdx.x)) : 0ull;
    const uint64_t inc = wave_incl_scan(v, lane);
    if (lane == 63) red[wid] = inc;
    __syncthreads();
    uint64_t wp = 0, tot = 0;
    for (int w = 0; w < 16; w++) {
        if (w < wid) wp += red[w];
        tot += red[w];
    }
    if (threadIdx.x < NB) bbase[threadIdx.x] = wp + inc - v;
    if (threadIdx.x == 0) bbase[NB] = tot;
}

hipError_t launch_bucket_sort(const BucketArgs& a, uint32_t NB, hipStream_t s) {
    if (!NB) return hipSuccess;
    if (NB > 1024) return hipErrorInvalidValue;
    if (!a.bases_ready)
        hipLaunchKernelGGL(bucket_bases_kernel, dim3(1), dim3(1024), 0, s, a.bfill, a.cap, a.rbase, NB, a.bbase);
    if (a.spw == 2)
        hipLaunchKernelGGL(bucket_kernel<2>, dim3(NB), dim3(BK_THREADS), 0, s, a);
    else if (a.spw == 4)
        hipLaunchKernelGGL(bucket_kernel<4>, dim3(NB), dim3(BK_THREADS), 0, s, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

__global__ void bins_final_kernel(const unsigned long long* gcount, uint64_t* e_off, uint64_t* totals,
                                  uint64_t max_entries, const unsigned long long* flat_n,
                                  const unsigned long long* lq_n, const unsigned long long* pstat,
                                  const uint32_t* misc) {
    if (pstat)  // (the finalize's stats next to the totals: one copy, kbin_internal.h)
        for (int k = 0; k < KB_PSTAT; k++) totals[T_PSTAT + k] = pstat[k];
    if (misc)
        for (int k = 0; k < M_REPORTED / 2; k++)
            totals[T_MISC_PAIRS + k] = (uint64_t)misc[2 * k] | ((uint64_t)misc[2 * k + 1] << 32);
    // (the next finalize's grid hints: published heavy / split bins, queued list items)
    totals[T_HEAVY] = flat_n ? flat_n[FN_BINS] : 0ull;
    totals[T_QUEUED] = lq_n ? *lq_n : 0ull;
    // on overflow the counters ran past the capacity (status says so) and the
    // bins past it wrote nothing, so no entry range is whole: publish none (the
    // lists kernel then has no work and the host reruns at the exact need)
    const uint64_t ne0 = gcount[G_PACKED] >> 32, ni = gcount[G_PACKED] & 0xFFFFFFFFull;
    const uint64_t ne = ne0 <= max_entries ? ne0 : 0;
    totals[T_ENTRIES] = ne;
    totals[T_IDS] = ni;
    e_off[ne] = ni;
}

__global__ __launch_bounds__(1024) void clear_kernel(ClearList l) {
    for (int k = 0; k < l.n; k++)
        for (uint32_t i = threadIdx.x; i < l.words[k]; i += 1024) l.p[k][i] = 0u;
}

// After the record pass: R (records), the largest bucket and the status word
// next to N for the host's one mid-finalize copy, and the exclusive prefix of
// the bucket fills (clamped to the capacity) -> bbase[NB + 1], which the bucket
// ordering reads (one launch where a stats kernel and a bases kernel were two)
__global__ __launch_bounds__(1024) void bucket_stats_kernel(const unsigned long long* __restrict__ bfill, uint32_t NB,
                                                            const uint32_t* misc, uint64_t* totals, uint64_t cap,
                                                            const uint64_t* __restrict__ rbase,
                                                            uint64_t* __restrict__ bbase,
                                                            const unsigned long long* __restrict__ kpart, uint64_t nk) {
    __shared__ uint64_t red[16];
    __shared__ uint32_t mxw[16];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wid = (int)(t >> 6);
    // (the record pass's per-block k-mer sums: N, where a kernel of its own did it)
    uint64_t ks = 0;
    for (uint64_t i = t; i < nk; i += 1024) ks += kpart[i];
    const uint64_t f = t < NB ? bfill[t] : 0ull;  // (NB <= 1024)
    const uint64_t v = t < NB ? min<uint64_t>(f, region_room(rbase, cap, t)) : 0ull;
    const uint64_t inc = wave_incl_scan(v, lane);
    // fills < 2^32 (a region's capacity); a larger one is clamped for the max
    const uint32_t m = wave_max_u32((uint32_t)min<uint64_t>(f, 0xFFFFFFFFull));
    uint64_t fs = f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        fs += (uint64_t)__shfl_xor((long long)fs, off, 64);
        ks += (uint64_t)__shfl_xor((long long)ks, off, 64);
    }
    if (lane == 63) red[wid] = inc;
    if (lane == 0) mxw[wid] = m;
    __shared__ uint64_t fsum[16], ksum[16];
    if (lane == 0) {
        fsum[wid] = fs;
        ksum[wid] = ks;
    }
    __syncthreads();
    uint64_t wp = 0, tot = 0, sum = 0, kt = 0;
    uint32_t mx = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        if (w < wid) wp += red[w];
        tot += red[w];
        sum += fsum[w];
        kt += ksum[w];
        mx = max(mx, mxw[w]);
    }
    if (t < NB) bbase[t] = wp + inc - v;
    if (t == 0) {
        bbase[NB] = tot;
        totals[T_KMERS] += kt;
        totals[T_REC_SUM] = sum;
        totals[T_REC_MAX] = mx;
        totals[T_REC_STATUS] = misc[M_REC_STATUS];
    }
}

hipError_t launch_bucket_stats(const unsigned long long* bfill, uint32_t NB, const uint32_t* misc, uint64_t* totals,
                               uint64_t cap, const uint64_t* rbase, uint64_t* bbase, const unsigned long long* kpart,
                               uint64_t nk, hipStream_t s) {
    if (NB > 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bucket_stats_kernel, dim3(1), dim3(1024), 0, s, bfill, NB, misc, totals, cap, rbase, bbase,
                       kpart, nk);
    return hipGetLastError();
}

hipError_t launch_clear(const ClearList& l, hipStream_t s) {
    if (l.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(1024), 0, s, l);
    return hipGetLastError();
}

hipError_t launch_bins_final(const unsigned long long* gcount, uint64_t* e_off, uint64_t* totals,
                             uint64_t max_entries, const unsigned long long* flat_n, const unsigned long long* lq_n,
                             const unsigned long long* pstat, const uint32_t* report_misc, hipStream_t s) {
    hipLaunchKernelGGL(bins_final_kernel, dim3(1), dim3(1), 0, s, gcount, e_off, totals, max_entries, flat_n, lq_n,
                       pstat, report_misc);
    return hipGetLastError();
}

hipError_t load_plan_kernels() {
    return resolve_kernels({(const void*)bucket_kernel<2>, (const void*)bucket_kernel<4>,
                            (const void*)bucket_bases_kernel, (const void*)bucket_stats_kernel,
                            (const void*)bins_order_kernel, (const void*)bins_desc_kernel,
                            (const void*)bins_plan_kernel, (const void*)bins_final_kernel, (const void*)clear_kernel});
}

}  // namespace kb

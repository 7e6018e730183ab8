// kbin_lists.hip -- the binned engine's list kernels.
#include <algorithm>
#include <cstdio>

#include "kbin_internal.h"
#include "kbin_sort.h"

namespace kb {

// ---------------------------------------------------------------------------
// phase C: every list into reverse call order (binning.c:1061-1068 prepends,
// so a list reads newest call first = descending ordinal), ordinals -> ids.
// A block takes 256 consecutive entries: lists of <= 32 ids are sorted in the
// registers of one lane, 33..256 by one wavefront in LDS, longer ones by the
// whole block (LDS bitonic up to LIST_CAP, else chunks + merge passes).
// ---------------------------------------------------------------------------
constexpr int LIST_THREADS = 256;
constexpr uint32_t LIST_SPAN = 7168;  // ids staged in LDS at once (28 KiB: 5 blocks per CU)
constexpr uint32_t LIST_WIN = LIST_SPAN - 256 - 8;  // window of list starts: + one list <= 256, + alignment

#ifdef KB_BIN_PROF
__device__ unsigned long long g_list_prof[8];
#define LPROF(ph)                                                  \
    do {                                                           \
        if (tid == 0) {                                            \
            const unsigned long long _t = clock64();               \
            lacc[ph] += _t - lt;                                   \
            lt = _t;                                               \
        }                                                          \
    } while (0)
#else
#define LPROF(ph) do {} while (0)
#endif

__global__ __launch_bounds__(LIST_THREADS) __attribute__((amdgpu_waves_per_eu(5, 8))) void lists_kernel(ListArgs A) {
#ifdef KB_BIN_PROF
    unsigned long long lacc[8] = {};
    unsigned long long lt = clock64();
#endif
    // staged chunks: ibuf = the chunk's ids (ordinal + 1); other chunks: buf =
    // block sort space (LIST_CAP), wave windows inside
    __shared__ uint32_t lds[LIST_SPAN + LIST_READ_PAD];  // (the pad: sort_lists_lane's reads)
    static_assert(LIST_CAP <= LIST_SPAN, "block sort space aliases the staging area");
    uint32_t* const ibuf = lds;
    uint32_t* const buf = lds;
    __shared__ uint32_t big[LIST_THREADS], mid[LIST_THREADS];
    __shared__ uint32_t n_big, n_mid, s_long, w_lo[2], w_hi[2];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const uint64_t n_entries = A.totals[T_ENTRIES];
    // items: the bin kernels' queue (partitions whose ids took the global
    // path, and long lists of the LDS path), else every entry in chunks of 256
    // (an entry-capacity overflow publishes no entries, bins_final_kernel: the
    // queued items' neighbours then have unwritten offsets -- no work at all,
    // the host reruns the bin phase)
    const uint64_t n_items = !n_entries ? 0ull
                             : A.lq_items ? min<uint64_t>(*A.lq_n, A.lq_cap)
                                          : (n_entries + LIST_THREADS - 1) / LIST_THREADS;
    for (uint64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        uint64_t e0;
        uint32_t ne;
        if (A.lq_items) {
            const uint64_t x = A.lq_items[it];
            e0 = x >> 16;
            ne = (uint32_t)(x & 0xFFFFu);
        } else {
            e0 = it * LIST_THREADS;
            ne = (uint32_t)min<uint64_t>(LIST_THREADS, n_entries - e0);
        }
        const uint64_t ob = A.e_off[e0], span = A.e_off[e0 + ne] - ob;
        // (barriers in the staged path order LDS only: a full __syncthreads
        // also waits for the previous window's global stores to land)
        if (tid == 0) {
            n_big = 0;
            s_long = 0;
        }
        lds_barrier();
        // this thread's entry; lists > 256 leave the staged windows: up to
        // WAVE_LIST_MAX to lists_bucket_kernel, longer ones to this block below
        const uint32_t n_me = tid < ne ? A.e_cnt[e0 + tid] : 0u;
        const uint32_t rel = tid < ne ? (uint32_t)(A.e_off[e0 + tid] - ob) : 0u;  // < 2^32 ids per finalize
        const bool short_me = tid < ne && n_me <= 256;
        if (tid < ne && !short_me) {
            if (n_me <= WAVE_LIST_MAX) A.long_q[atomicAdd(A.long_n, 1u)] = (uint32_t)(e0 + tid);
            else big[atomicAdd(&n_big, 1u)] = tid;
            s_long = 1;
        }
        lds_barrier();
        // Staged windows: the chunk's id range cut every LIST_WIN ids; a short
        // list belongs to the window its first id falls in, and a window stages
        // [first start, last end) of its lists (<= LIST_WIN + 256 ids) with
        // coalesced 16-B loads, sorts each list in LDS (<= 32: one lane's
        // registers, 33..256: one wavefront) and writes the range back with 16-B
        // stores.  (Ids of a long list inside the range are written back
        // unsorted; its own kernel rewrites them later on the stream.)
        // (the common case -- every list short, the chunk fits -- is one window)
        const bool one = !s_long && span + 8 <= LIST_SPAN;
        const uint32_t nw = one ? 1u : (uint32_t)((span + LIST_WIN - 1) / LIST_WIN);
        const uint32_t wk = rel / LIST_WIN;
        for (uint32_t k = 0; k < nw; k++) {
            const uint32_t wb = k & 1u;  // double-buffered: a lane may still read the last window's range
            if (tid == 0) {
                w_lo[wb] = one ? 0u : 0xFFFFFFFFu;
                w_hi[wb] = one ? (uint32_t)span : 0u;
                n_mid = 0;
            }
            lds_barrier();
            const bool in_w = short_me && (one || wk == k);
            if (!one) {
                if (in_w) {
                    atomicMin(&w_lo[wb], rel);
                    atomicMax(&w_hi[wb], rel + n_me);
                }
                lds_barrier();
            }
            const uint32_t lo_w = w_lo[wb], hi_w = w_hi[wb];
            if (lo_w >= hi_w) continue;  // uniform: no short list starts here
            LPROF(0);
            const uint64_t base = (ob + lo_w) & ~3ull;   // staging is 16-B aligned
            const uint32_t sh = (uint32_t)(ob + lo_w - base);  // ibuf[j] holds id base + j
            const uint32_t nv = (sh + (hi_w - lo_w) + 3) >> 2;  // uint4 groups (<= LIST_SPAN / 4)
            const uint4* src4 = reinterpret_cast<const uint4*>(A.ids_ord + base);
            uint4* ib4 = reinterpret_cast<uint4*>(ibuf);
            for (uint32_t g0 = 0; g0 < nv; g0 += 4 * LIST_THREADS) {  // 4 x 16 B in flight
                uint4 v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t g = g0 + q * LIST_THREADS + tid;
                    if (g < nv) v[q] = src4[g];  // may read up to 3 ids past the range: same allocation
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t g = g0 + q * LIST_THREADS + tid;
                    if (g < nv) ib4[g] = make_uint4(v[q].x + 1u, v[q].y + 1u, v[q].z + 1u, v[q].w + 1u);
                }
            }
            lds_barrier();
            LPROF(1);
            sort_lists_lane(ibuf + sh + (rel - lo_w), in_w ? n_me : 0u);
            if (in_w && n_me > 32) mid[atomicAdd(&n_mid, 1u)] = tid;
            lds_barrier();
            LPROF(2);
            const uint32_t nmid = n_mid;
            for (uint32_t q = wid; q < nmid; q += LIST_THREADS / 64) {
                const uint32_t n = A.e_cnt[e0 + mid[q]];
                uint32_t* p = ibuf + sh + (uint32_t)(A.e_off[e0 + mid[q]] - ob - lo_w);
                if (n <= 64) wave_sort_desc<1>(p, n, lane);
                else if (n <= 128) wave_sort_desc<2>(p, n, lane);
                else wave_sort_desc<4>(p, n, lane);
                wave_sync();
            }
            lds_barrier();
            LPROF(3);
            {
                // full groups as 16-B stores, the partial first/last group per id
                const uint32_t end = sh + (hi_w - lo_w);  // ibuf index past the range
                int4* dst4 = reinterpret_cast<int4*>(A.ids_out + base);
                for (uint32_t g = tid; g < nv; g += LIST_THREADS) {
                    const uint32_t j0 = g * 4;
                    const uint4 v = ib4[g];
                    if (j0 >= sh && j0 + 4 <= end) {
                        dst4[g] = make_int4(id_of(v.x - 1u, A.read_ids, A.id_off), id_of(v.y - 1u, A.read_ids, A.id_off),
                                            id_of(v.z - 1u, A.read_ids, A.id_off), id_of(v.w - 1u, A.read_ids, A.id_off));
                    } else {
                        const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if (j0 + q >= sh && j0 + q < end)
                                A.ids_out[base + j0 + q] = id_of(vv[q] - 1u, A.read_ids, A.id_off);
                    }
                }
            }
            // the staging area is reused: every lane's LDS reads must be done (they
            // fed its stores), but its global stores need not have landed -- a
            // full __syncthreads() would wait for them (vmcnt), 36 % of the kernel
            lds_barrier();
            LPROF(4);
#ifdef KB_BIN_PROF
            if (tid == 0) lacc[5]++, lacc[6] += nmid;
#endif
        }
        const uint32_t nbig = n_big;  // lists > WAVE_LIST_MAX: the whole block
        if (nbig) {  // it rewrites ids the windows wrote: let those land first
            __threadfence_block();
            __syncthreads();
        }
        for (uint32_t q = 0; q < nbig; q++) {
            const uint64_t ge = e0 + big[q];
            const uint32_t n = A.e_cnt[ge];
            const uint64_t o = A.e_off[ge];
            if (n <= WAVE_LIST_MAX) continue;  // uniform
            if (n <= (uint32_t)LIST_CAP) {
                uint32_t Pw = 64;
                while (Pw < n) Pw <<= 1;
                for (uint32_t j = tid; j < Pw; j += LIST_THREADS) buf[j] = j < n ? A.ids_ord[o + j] + 1u : 0u;
                __syncthreads();
                for (uint32_t kk = 2; kk <= Pw; kk <<= 1) {
                    for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                        for (uint32_t i = tid; i < Pw; i += LIST_THREADS) {
                            const uint32_t l2 = i ^ jj;
                            if (l2 > i) {
                                const uint32_t x = buf[i], y = buf[l2];
                                const bool desc = (i & kk) == 0;
                                if (desc ? (x < y) : (x > y)) {
                                    buf[i] = y;
                                    buf[l2] = x;
                                }
                            }
                        }
                        __syncthreads();
                    }
                }
                for (uint32_t j = tid; j < n; j += LIST_THREADS)
                    A.ids_out[o + j] = id_of(buf[j] - 1u, A.read_ids, A.id_off);
                __syncthreads();
            } else {
                // very long list: sort LDS-sized chunks, then merge passes
                // through ids_out (as scratch) and ids_ord, ordinals + 1
                const uint32_t C = (uint32_t)LIST_CAP;
                uint32_t* src = A.ids_ord + o;
                uint32_t* dst = reinterpret_cast<uint32_t*>(A.ids_out + o);
                for (uint32_t c0 = 0; c0 < n; c0 += C) {
                    const uint32_t cn = min(C, n - c0);
                    for (uint32_t j = tid; j < C; j += LIST_THREADS) buf[j] = j < cn ? src[c0 + j] + 1u : 0u;
                    __syncthreads();
                    for (uint32_t kk = 2; kk <= C; kk <<= 1) {
                        for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                            for (uint32_t i = tid; i < C; i += LIST_THREADS) {
                                const uint32_t l2 = i ^ jj;
                                if (l2 > i) {
                                    const uint32_t x = buf[i], y = buf[l2];
                                    const bool desc = (i & kk) == 0;
                                    if (desc ? (x < y) : (x > y)) {
                                        buf[i] = y;
                                        buf[l2] = x;
                                    }
                                }
                            }
                            __syncthreads();
                        }
                    }
                    for (uint32_t j = tid; j < cn; j += LIST_THREADS) dst[c0 + j] = buf[j];
                    __syncthreads();
                }
                __threadfence_block();
                __syncthreads();
                // merge runs of width wd from dst into src, alternating
                uint32_t* a = dst;
                uint32_t* bb = src;
                for (uint32_t wd = C; wd < n; wd <<= 1) {
                    for (uint32_t t = tid; t < n; t += LIST_THREADS) {
                        const uint32_t pair0 = (t / (2 * wd)) * 2 * wd;
                        const uint32_t an = min(wd, n - pair0);
                        const uint32_t b0 = pair0 + an, bn = b0 < n ? min(wd, n - b0) : 0u;
                        const uint32_t d = t - pair0;
                        uint32_t l1 = d > bn ? d - bn : 0u, h1 = min(d, an);
                        while (l1 < h1) {
                            const uint32_t i = (l1 + h1) >> 1;
                            if (a[pair0 + i] >= a[b0 + d - i - 1]) l1 = i + 1; else h1 = i;
                        }
                        const uint32_t i = l1, j = d - l1;
                        bb[t] = (i < an && (j >= bn || a[pair0 + i] >= a[b0 + j])) ? a[pair0 + i] : a[b0 + j];
                    }
                    __threadfence_block();
                    __syncthreads();
                    uint32_t* tmp = a;
                    a = bb;
                    bb = tmp;
                }
                // a holds the merged ordinals + 1; map into ids_out
                if (a == dst) {  // ids_out holds them already: map in place
                    for (uint32_t t = tid; t < n; t += LIST_THREADS)
                        A.ids_out[o + t] = id_of(dst[t] - 1u, A.read_ids, A.id_off);
                } else {
                    for (uint32_t t = tid; t < n; t += LIST_THREADS)
                        A.ids_out[o + t] = id_of(a[t] - 1u, A.read_ids, A.id_off);
                }
                __threadfence_block();
                __syncthreads();
            }
        }
        lds_barrier();  // (LDS only: big[], n_big and the staging area are reused)
    }
#ifdef KB_BIN_PROF
    if (tid == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&g_list_prof[i], lacc[i]);
#endif
}

#ifdef KB_BIN_PROF
void lists_prof_report(hipStream_t s) {
    unsigned long long h[8];
    (void)hipStreamSynchronize(s);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_list_prof), sizeof(h));
    fprintf(stderr, "[list_prof] pre=%llu load=%llu small=%llu mid=%llu store=%llu chunks=%llu mid_lists=%llu\n",
            h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
    unsigned long long z[8] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_list_prof), z, sizeof(z));
}
#endif

// lists of 257..WAVE_LIST_MAX ids that lists_bucket_kernel passed on: one
// wavefront per list, a full bitonic network in its registers (kept out of the
// other list kernels, whose occupancy its 64-register lists would cap)
__global__ __launch_bounds__(256) void lists_long_kernel(ListArgs A) {
    const int lane = threadIdx.x & 63;
    const uint32_t nq = A.long_n[1];
    for (uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += gridDim.x * 4) {
        const uint32_t e = A.long_q[A.long_cap + q];
        const uint32_t n = A.e_cnt[e];
        const uint64_t o = A.e_off[e];
        const uint32_t* src = A.ids_ord + o;
        int32_t* dst = A.ids_out + o;
        if (n <= 512) wave_sort_list_long<8>(src, dst, n, lane, A.read_ids, A.id_off);
        else if (n <= 1024) wave_sort_list_long<16>(src, dst, n, lane, A.read_ids, A.id_off);
        else if (n <= 2048) wave_sort_list_long<32>(src, dst, n, lane, A.read_ids, A.id_off);
        else wave_sort_list_long<64>(src, dst, n, lane, A.read_ids, A.id_off);
    }
}

// Lists of 257..WAVE_LIST_MAX ids (high coverage: every true k-mer's list
// is this long) by bucketing rather than a full sorting network.  One
// wavefront per list: min/max of its ordinals, NB order-preserving buckets
// over that range (an LDS histogram, a wave scan, an LDS scatter), then every
// lane sorts its own bucket(s) of <= 64 ids in registers and writes them
// straight to their place in the list.  About n (log2(64) + 3) wave steps
// against the network's n log2^2(n) / 2; a list with a bucket past 64 ids
// (clustered ordinals) is queued for the network (lists_long_kernel).
constexpr uint32_t LB_WAVES = 4;
constexpr uint32_t LB_SPAN = WAVE_LIST_MAX;  // ids per wave in LDS
constexpr uint32_t LB_ILP = 16;              // loads in flight per lane

// n <= 64 values in registers, sorted descending (0 pads last)
template <int W>
DEV void lane_sort_desc(uint32_t (&v)[W]) {
#pragma unroll
    for (int kk = 2; kk <= W; kk <<= 1) {
#pragma unroll
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int l2 = i ^ jj;
                if (l2 > i) {
                    const uint32_t x = v[i], y = v[l2];
                    const bool desc = (i & kk) == 0;
                    const bool sw = desc ? (x < y) : (x > y);
                    v[i] = sw ? y : x;
                    v[l2] = sw ? x : y;
                }
            }
        }
    }
}


// one lane's bucket buf[off, off + c) sorted ascending in place (values >= 1)
template <int W>
DEV void lane_bucket_sort_asc(uint32_t* buf, uint32_t off, uint32_t c) {
    uint32_t v[W];
#pragma unroll
    for (int j = 0; j < W; j++) v[j] = (uint32_t)j < c ? buf[off + j] : 0u;
    lane_sort_desc<W>(v);  // the c values first, descending
#pragma unroll
    for (int j = 0; j < W; j++)
        if ((uint32_t)j < c) buf[off + c - 1u - (uint32_t)j] = v[j];
}

__global__ __launch_bounds__(LB_WAVES * 64) void lists_bucket_kernel(ListArgs A) {
    __shared__ uint32_t sbuf[LB_WAVES][LB_SPAN];
    __shared__ uint32_t scnt[LB_WAVES][256], scur[LB_WAVES][256];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t* buf = sbuf[wid];
    uint32_t* cnt = scnt[wid];
    uint32_t* cur = scur[wid];
    const uint32_t nq = *A.long_n;
    for (uint32_t q = blockIdx.x * LB_WAVES + wid; q < nq; q += gridDim.x * LB_WAVES) {
        const uint32_t e = A.long_q[q];
        const uint32_t n = A.e_cnt[e];
        const uint64_t o = A.e_off[e];
        const uint32_t* src = A.ids_ord + o;
        int32_t* dst = A.ids_out + o;
        // three passes over the list, each with LB_ILP loads in flight per lane
        // (one dependent load per iteration left every wave waiting on HBM)
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
        for (uint32_t i0 = lane; i0 < n; i0 += 64u * LB_ILP) {
            uint32_t x[LB_ILP];
#pragma unroll
            for (uint32_t k = 0; k < LB_ILP; k++) x[k] = i0 + 64u * k < n ? src[i0 + 64u * k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < LB_ILP; k++)
                if (i0 + 64u * k < n) {
                    mn = min(mn, x[k]);
                    mx = max(mx, x[k]);
                }
        }
        mx = wave_max_u32(mx);
        mn = ~wave_max_u32(~mn);
        // about 16 ids per bucket: each lane then sorts its buckets with
        // 16- or 32-input networks (64 buckets for 4096 ids took 64-input ones)
        const uint32_t nb = n <= 1024 ? 64u : n <= 2048 ? 128u : 256u;
        // order-preserving bucket of an ordinal: floor((x - mn) * nb / range)
        const float scale = (float)nb / ((float)(mx - mn) + 1.0f);
        for (uint32_t b = lane; b < nb; b += 64) cnt[b] = 0;
        wave_sync();
        for (uint32_t i0 = lane; i0 < n; i0 += 64u * LB_ILP) {
            uint32_t x[LB_ILP];
#pragma unroll
            for (uint32_t k = 0; k < LB_ILP; k++) x[k] = i0 + 64u * k < n ? src[i0 + 64u * k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < LB_ILP; k++)
                if (i0 + 64u * k < n) atomicAdd(&cnt[min(nb - 1u, (uint32_t)((float)(x[k] - mn) * scale))], 1u);
        }
        wave_sync();
        // lane l owns the npl = nb / 64 adjacent buckets from ba = npl l, so one
        // wave scan of the per-lane totals places them all
        const uint32_t npl = nb / 64u, ba = npl * (uint32_t)lane;
        uint32_t c[4], tot = 0, big = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            c[k] = k < npl ? cnt[ba + k] : 0u;
            tot += c[k];
            big = max(big, c[k]);
        }
        big = wave_max_u32(big);
        if (big > 64) {  // clustered ordinals: the sorting network takes the list
            if (lane == 0) A.long_q[A.long_cap + atomicAdd(A.long_n + 1, 1u)] = e;
            continue;
        }
        const uint32_t base = wave_incl_scan(tot, lane) - tot;  // ascending offsets
        wave_sync();
        {
            uint32_t run = base;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k < npl) {
                    cur[ba + k] = run;
                    run += c[k];
                }
        }
        wave_sync();
        for (uint32_t i0 = lane; i0 < n; i0 += 64u * LB_ILP) {
            uint32_t x[LB_ILP];
#pragma unroll
            for (uint32_t k = 0; k < LB_ILP; k++) x[k] = i0 + 64u * k < n ? src[i0 + 64u * k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < LB_ILP; k++)
                if (i0 + 64u * k < n) {
                    const uint32_t b = min(nb - 1u, (uint32_t)((float)(x[k] - mn) * scale));
                    buf[atomicAdd(&cur[b], 1u)] = x[k] + 1u;
                }
        }
        wave_sync();
        // each lane sorts its buckets in place (ascending), so buf holds the
        // whole list ascending; the wave then writes it reversed -- descending,
        // binning.c:1065-1068 -- with coalesced stores (lanes writing their own
        // buckets straight to HBM touched 64 lines per store instruction)
        uint32_t a0 = base;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (k >= npl) break;  // (wave-uniform)
            if (big <= 16)
                lane_bucket_sort_asc<16>(buf, a0, c[k]);
            else if (big <= 32)
                lane_bucket_sort_asc<32>(buf, a0, c[k]);
            else
                lane_bucket_sort_asc<64>(buf, a0, c[k]);
            a0 += c[k];
        }
        wave_sync();
        for (uint32_t j = lane; j < n; j += 64) dst[j] = id_of(buf[n - 1u - j] - 1u, A.read_ids, A.id_off);
        wave_sync();
    }
}

hipError_t launch_lists(const ListArgs& a, uint64_t max_entries, hipStream_t s) {
    uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>(1, (max_entries + LIST_THREADS - 1) / LIST_THREADS), 16384);
    // queued items / long lists of the last finalize (~0: none seen yet) size
    // the grids: every list kernel strides over its queue
    auto grid = [](uint64_t hint, uint64_t per_block, uint64_t full) {
        if (hint == ~0ull) return full;
        return std::min<uint64_t>(full, std::max<uint64_t>(16, (hint + hint / 2 + 64) / per_block));
    };
    if (a.lq_items) blocks = grid(a.lq_hint, 1, blocks);
    if (!a.long_n_zeroed) {
        hipError_t e = hipMemsetAsync(a.long_n, 0, 2 * sizeof(unsigned int), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lists_kernel, dim3((unsigned)blocks), dim3(LIST_THREADS), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lists_bucket_kernel, dim3((unsigned)grid(a.long_hint[0], LB_WAVES, 4096)), dim3(LB_WAVES * 64), 0,
                       s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lists_long_kernel, dim3((unsigned)grid(a.long_hint[1], 4, 1024)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t load_lists_kernels() {
    return resolve_kernels(
        {(const void*)lists_kernel, (const void*)lists_bucket_kernel, (const void*)lists_long_kernel});
}

}  // namespace kb

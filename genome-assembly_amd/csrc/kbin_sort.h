// kbin_sort.h -- the id lists' sorters (descending call ordinal: reverse call
// order), in registers and in LDS: the list kernels' (kbin_lists.hip), which
// the bin kernel's LDS id windows borrow (kbin_bins.hip).
#pragma once
#include "kbin_device.h"

namespace kb {

constexpr uint32_t LIST_CAP = 4096;   // longest list sorted in LDS in one piece (power of two)
constexpr uint32_t WAVE_LIST_MAX = 4096;  // longest list one wavefront sorts in its registers (64 x 64)
// words past a list window that sort_lists_lane may read (never write): the
// end of bin_kernel's LDS carve and lists_kernel's window are padded by it
constexpr uint32_t LIST_READ_PAD = 32;

// descending bitonic sort of Pw (power of two) values in LDS by a group of G
// lanes (G = 64: one wavefront, wave barriers; else the block)
template <int G>
DEV void bitonic_desc(uint32_t* a, uint32_t Pw, uint32_t r) {
    for (uint32_t kk = 2; kk <= Pw; kk <<= 1) {
        for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
            for (uint32_t i = r; i < Pw; i += G) {
                const uint32_t l2 = i ^ jj;
                if (l2 > i) {
                    const uint32_t x = a[i], y = a[l2];
                    const bool desc = (i & kk) == 0;
                    if (desc ? (x < y) : (x > y)) {
                        a[i] = y;
                        a[l2] = x;
                    }
                }
            }
            if (G == 64) wave_sync();
            else __syncthreads();
        }
    }
}

// up to 256 values sorted descending by one wavefront, in registers: element
// i = r * 64 + lane lives in v[r]; partners across lanes meet by xor-shuffle,
// partners 64 or 128 apart are in the same lane.  In place in LDS.
// Bitonic sort, descending, of R*64 values held by one wavefront in
// registers, striped (value i = v[i / 64] of lane i % 64): partner distances
// below 64 are lane shuffles, 64 and up are register pairs.  No LDS, no
// barriers -- a wavefront sorts a list of up to 64 R ids on its own.
template <int R>
DEV void wave_bitonic(uint32_t (&v)[R], int lane) {
#pragma unroll
    for (int kk = 2; kk <= R * 64; kk <<= 1) {
#pragma unroll
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            if (jj >= 64) {
                const int rj = jj >> 6;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int r2 = r ^ rj;
                    if (r2 > r) {
                        const uint32_t i = (uint32_t)(r * 64 + lane);
                        const bool desc = (i & kk) == 0;
                        const uint32_t x = v[r], y = v[r2];
                        const uint32_t hi = x > y ? x : y, lo = x > y ? y : x;
                        v[r] = desc ? hi : lo;
                        v[r2] = desc ? lo : hi;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const uint32_t i = (uint32_t)(r * 64 + lane);
                    const uint32_t y = (uint32_t)__shfl_xor((int)v[r], jj, 64);
                    const bool lower = (lane & jj) == 0;
                    const bool desc = (i & kk) == 0;
                    const uint32_t hi = v[r] > y ? v[r] : y, lo = v[r] > y ? y : v[r];
                    v[r] = (lower == desc) ? hi : lo;
                }
            }
        }
    }
}

// The same network for long lists with the stage loops left rolled: the
// register-pair stages are unrolled per distance (RJ), so the code and the
// register file stay at O(R), not O(R log^2 R).
template <int R, int RJ>
DEV void reg_stage(uint32_t (&v)[R], int lane, uint32_t kk) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int r2 = r ^ RJ;
        if (r2 > r) {
            const bool desc = ((uint32_t)(r * 64 + lane) & kk) == 0;
            const uint32_t x = v[r], y = v[r2];
            const uint32_t hi = x > y ? x : y, lo = x > y ? y : x;
            v[r] = desc ? hi : lo;
            v[r2] = desc ? lo : hi;
        }
    }
}

template <int R>
DEV void wave_bitonic_rolled(uint32_t (&v)[R], int lane) {
    for (uint32_t kk = 2; kk <= R * 64; kk <<= 1) {
        for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
            if (jj >= 64) {
                switch (jj >> 6) {
                    case 1: if constexpr (R > 1) reg_stage<R, 1>(v, lane, kk); break;
                    case 2: if constexpr (R > 2) reg_stage<R, 2>(v, lane, kk); break;
                    case 4: if constexpr (R > 4) reg_stage<R, 4>(v, lane, kk); break;
                    case 8: if constexpr (R > 8) reg_stage<R, 8>(v, lane, kk); break;
                    case 16: if constexpr (R > 16) reg_stage<R, 16>(v, lane, kk); break;
                    case 32: if constexpr (R > 32) reg_stage<R, 32>(v, lane, kk); break;
                    default: break;
                }
            } else {
                const bool lower = (lane & jj) == 0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const uint32_t y = (uint32_t)__shfl_xor((int)v[r], (int)jj, 64);
                    const bool desc = ((uint32_t)(r * 64 + lane) & kk) == 0;
                    const uint32_t hi = v[r] > y ? v[r] : y, lo = v[r] > y ? y : v[r];
                    v[r] = (lower == desc) ? hi : lo;
                }
            }
        }
    }
}

template <int R>
DEV void wave_sort_list_long(const uint32_t* __restrict__ src, int32_t* __restrict__ dst, uint32_t n, int lane,
                             const int32_t* read_ids, uint32_t id_off) {
    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t i = (uint32_t)(r * 64 + lane);
        v[r] = i < n ? src[i] + 1u : 0u;
    }
    wave_bitonic_rolled<R>(v, lane);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t i = (uint32_t)(r * 64 + lane);
        if (i < n) dst[i] = id_of(v[r] - 1u, read_ids, id_off);
    }
}

// n <= 64 R values (ordinal + 1) in LDS, sorted descending in place
template <int R>
DEV void wave_sort_desc(uint32_t* p, uint32_t n, int lane) {
    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t i = (uint32_t)(r * 64 + lane);
        v[r] = i < n ? p[i] : 0u;
    }
    wave_bitonic<R>(v, lane);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t i = (uint32_t)(r * 64 + lane);
        if (i < n) p[i] = v[r];
    }
}

// one list of n <= 64 R call ordinals from HBM to its ids, reverse call order
template <int R>
DEV void wave_sort_list(const uint32_t* __restrict__ src, int32_t* __restrict__ dst, uint32_t n, int lane,
                        const int32_t* read_ids, uint32_t id_off) {
    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t i = (uint32_t)(r * 64 + lane);
        v[r] = i < n ? src[i] + 1u : 0u;
    }
    wave_bitonic<R>(v, lane);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t i = (uint32_t)(r * 64 + lane);
        if (i < n) dst[i] = id_of(v[r] - 1u, read_ids, id_off);
    }
}

// up to 32 values (ordinal + 1) sorted descending in one lane's registers, in place
// Batcher's odd-even merge network on NP = 2^k inputs, descending (the larger
// of every pair to the lower index), keeping only the comparators whose upper
// index is < N: a list of n <= N ids padded with zeros (below every id + 1)
// keeps its pads in place, so the pruned network sorts it.  NP = 32: 191
// comparators (the bitonic network: 240); N = 24: 132; 16: 63; 8: 19
// (2 <= n <= N.  The loads and stores are branch-free -- a branch per
// position saved the exec mask in an SGPR pair, and in bin_kernel those were
// spilled to VGPR lanes: all N words are read (p[0 .. N) must lie inside the
// LDS allocation: both callers leave LIST_READ_PAD words after their windows)
// and the pads masked; position j >= n writes p[n - 1] instead, the stores
// going out from the last position down, so p[n - 1] ends with its own value)
template <int N, int NP>
DEV void sort_net_desc(uint32_t* p, uint32_t n) {
    uint32_t v[N];
    const uint32_t last = n - 1u;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t x = p[j];
        v[j] = (uint32_t)j < n ? x : 0u;
    }
#pragma unroll
    for (int q = 1; q < NP; q <<= 1)
#pragma unroll
        for (int k = q; k >= 1; k >>= 1)
#pragma unroll
            for (int j = k % q; j + k < NP; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; i++) {
                    const int a = i + j, b = i + j + k;
                    if (b < N && a / (2 * q) == b / (2 * q)) {
                        const uint32_t x = v[a], y = v[b < N ? b : 0];
                        v[a] = x > y ? x : y;
                        v[b < N ? b : 0] = x > y ? y : x;
                    }
                }
#pragma unroll
    for (int j = N - 1; j >= 0; j--) p[min((uint32_t)j, last)] = v[j];
}

// every lane's list of 2..32 ids (n outside that: nothing) in descending
// order in its registers, with the smallest network that holds the wave's
// longest such list (wave-uniform call)
DEV void sort_lists_lane(uint32_t* p, uint32_t n) {
    const bool me = n >= 2 && n <= 32;
    const uint32_t m = wave_max_u32(me ? n : 0u);
    if (m > 24) {
        if (me) sort_net_desc<32, 32>(p, n);
    } else if (m > 16) {
        if (me) sort_net_desc<24, 32>(p, n);
    } else if (m > 8) {
        if (me) sort_net_desc<16, 16>(p, n);
    } else if (m >= 2) {
        if (me) sort_net_desc<8, 8>(p, n);
    }
}

}  // namespace kb

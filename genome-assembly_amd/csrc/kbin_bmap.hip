// kbin_bmap.hip -- the bucket maps of the binned engine's bucketed record
// pass: which local bucket each canonical mmer (or context sub-bin) lands in.
#include <cmath>

#include "kbin_host.h"

// ---- balanced local buckets.  A bucket's records are ordered by ONE
// workgroup (bucket_kernel), so the largest bucket sets that kernel's time.
// The minimizer rule (leftmost max of the complement-canonical score) makes
// mmer frequencies very uneven: hashed into 1024 buckets the largest holds
// ~8x the mean.  After a pass the host learns the records per mmer from the
// bin descriptors and packs the mmers of each (part, part_n) key into buckets
// longest-processing-time first; later passes route records by that map.
uint64_t kb::bmap_key(const kb_ctx* c) { return ((uint64_t)c->part << 32) | c->part_n; }

kb_ctx::BucketMap* kb::bmap_find(kb_ctx* c, uint32_t NB) {
    for (auto& m : c->bmaps)
        if (m.key == bmap_key(c) && m.nb == NB) return &m;
    return nullptr;
}

// Context sub-bins (kbin_internal.h): an mmer whose expected distinct keys
// exceed one LDS table at the light load (few mmers per rank at N GPUs, high
// coverage), or whose records exceed 1.5 buckets' fair share, is split into
// 4^b + 1 sub-bins, b the smallest depth that brings each under both.  Each
// sub-bin is then an item of its own in the packing below, placed on any
// bucket -- a light bin of its own in bin_kernel: no flat lists, no
// re-expansion per partition, finer longest-first scheduling.
static uint32_t sub_depth(const kb_ctx* c, double w, double keys, double mean) {
    int bmax = std::min<int>((int)SUB_MAX_B, std::max(0, env_int("KB_BIN_SUB", (int)SUB_MAX_B)));
    if (!sub_room(c->p.K, c->p.M, 2 * c->KW)) bmax = 0;  // (no spare span bits for the stamp)
    if (c->p.K < 2 * c->p.M) bmax = 0;  // (K < 2M: a signature is no function of its key's k-mer)
    const double ts = c->KW == 1 ? 8192.0 : 4096.0;
    // (the long-list regime: sub-bins at 40 % of a table, so that they stay under
    // the ranking's LDS limit and their long lists take the bitmaps -- C3 261 ->
    // 247 ms per step, the list kernels 26 -> 4.5 ms)
    double cap = ts * std::min(4.0, std::max(0.2, env_int("KB_BIN_SUB_FILL_PCT", c->rank_regime ? 40 : 80) / 100.0));
    // light pre-filtered bins (two-word keys, singleton-heavy): a sub-bin's
    // distinct keys only have to load the bin's sketch lightly (PFL_LOAD of
    // its PFL_CELLS); the table holds the keys seen twice
    if (c->KW == 2 && c->pfl_regime) cap = std::max(cap, PFL_LOAD * (double)PFL_CELLS);
    uint32_t b = 0;
    while ((int)b < bmax && (keys / (double)(1u << (2 * b)) > cap || w / (double)(1u << (2 * b)) > 1.5 * mean)) b++;
    return b;
}

// bins one finalize may describe: every canonical mmer once, plus the extra
// sub-bins of the split ones (bmap_build keeps within it)
uint64_t kb::bin_budget(const kb_ctx* c, uint32_t NB) {
    const uint64_t half = 1ull << (2 * c->p.M - 1);
    // (at most 240: a bucket orders up to BK_SLOTS = 256 bins, one per mmer plus its extra sub-bins)
    // (the light pre-filtered regime splits every heavy mmer ~64 ways: a larger budget)
    const uint64_t per_bucket =
        (uint64_t)std::min(240, std::max(0, env_int("KB_BIN_SUB_EXTRA", c->rank_regime ? 240 : c->pfl_regime ? 160 : 48)));
    return half + (sub_room(c->p.K, c->p.M, 2 * c->KW) ? per_bucket * NB : 0ull);
}

// prior: a first pass's map from the prior weights (bmap_prior) -- packed in
// one serpentine sweep over the items in their generated order (heaviest mmers
// first) instead of sorted LPT: the prior only approximates the data, and the
// pass learns the real map (0.28 of the prior's 0.44 ms at C2 was the sort and
// the heap)
static int bmap_build(kb_ctx* c, uint32_t NB, double rho, bool prior = false) {
    const double tb0 = now_ms();
    const int M = c->p.M;
    const uint32_t half = 1u << (2 * M - 1);
    struct Item {
        double w;
        uint32_t mm, sub;  // sub: ~0 for an unsplit mmer
    };
    std::vector<uint32_t> h(half);
    uint64_t tot_w = 0;
    for (uint32_t i = 0; i < half && i < c->mmer_w.size(); i++) tot_w += c->mmer_w[i];
    const double mean = std::max(1.0, (double)tot_w / NB);
    // this pass's mmers, heaviest first: the split depths are handed out in
    // that order within the bin budget
    std::vector<std::pair<double, uint32_t>> seen;
    for (uint32_t i = 0; i < half; i++) {
        h[i] = (uint32_t)dest_of(half + i, NB, BUCKET_SALT);  // unseen (or another pass's): hash
        if (c->part_n > 1 && dest_of(half + i, c->part_n, PART_SALT) != c->part) continue;
        const double w = i < c->mmer_w.size() ? (double)c->mmer_w[i] : 0.0;
        // (a negligible mmer keeps its hash bucket: no packing item)
        if (w > 0 && w >= mean / 512.0) seen.push_back({w, i});
    }
    // (a prior's weights rise with the mmer score: ascending already)
    const auto desc = [](const std::pair<double, uint32_t>& a, const std::pair<double, uint32_t>& b) {
        return a.first > b.first;
    };
    if (std::is_sorted(seen.begin(), seen.end(), [&](const auto& a, const auto& b) { return desc(b, a); }))
        std::reverse(seen.begin(), seen.end());
    else if (!std::is_sorted(seen.begin(), seen.end(), desc))
        std::sort(seen.begin(), seen.end(), desc);
    uint64_t extra = bin_budget(c, NB) - half;  // sub-bins beyond one per mmer
    const kb_ctx::BucketMap* old = bmap_find(c, NB);
    std::vector<Item> items;
    std::vector<uint16_t> subs;
    uint32_t n_split = 0;
    for (const auto& sw : seen) {
        const uint32_t i = sw.second, mm = half + i;
        const double w = sw.first;
        const double occ = i < c->mmer_o.size() && c->mmer_o[i] ? (double)c->mmer_o[i] : 12.0 * w;
        uint32_t b = sub_depth(c, w, occ * rho, mean);
        while (b && sub_count(b) - 1 > extra) b--;
        if (!b) {
            items.push_back({w, mm, ~0u});
            continue;
        }
        extra -= sub_count(b) - 1;
        // sub-bin 0, the edge, holds a few percent; the contexts share the
        // rest -- or, when the last pass split this mmer as deep, as measured
        const uint32_t nsub = sub_count(b);
        const bool same = old && !old->h_map.empty() && (old->h_map[i] & BM_SPLIT) &&
                          ((old->h_map[i] >> 28) & 7u) == b;
        h[i] = BM_SPLIT | (b << 28) | (uint32_t)subs.size();
        for (uint32_t s2 = 0; s2 < nsub; s2++) {
            double ws = s2 ? w / (double)(nsub - 1) : 0.04 * w + 1.0;
            if (same) {
                auto f = c->sub_w.find(((uint64_t)mm << 16) | s2);
                ws = f != c->sub_w.end() ? (double)f->second : 1.0;
            }
            items.push_back({ws, mm, s2});
        }
        subs.resize(subs.size() + nsub, 0);
        n_split++;
    }
    const double tb1 = now_ms();
    if (!prior || env_int("KB_BIN_PRIOR_LPT", 0))
        std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.w > b.w; });
    const double tb2 = now_ms();
    // longest processing time first onto the least loaded bucket; at most 248
    // bins per bucket (bucket_kernel maps 256).  A binary min-heap of packed
    // (load in 1/16 records << 11 | bucket) words: one compare per level, the
    // top replaced in place (no pop + push)
    std::vector<uint64_t> heap(NB);
    std::vector<uint32_t> nm(NB, 0);
    for (uint32_t b = 0; b < NB; b++) heap[b] = b;  // (all loads 0: already a heap)
    uint32_t hn = NB;
    auto sift = [&](uint32_t i) {
        const uint64_t v = heap[i];
        for (;;) {
            uint32_t c2 = 2 * i + 1;
            if (c2 >= hn) break;
            if (c2 + 1 < hn && heap[c2 + 1] < heap[c2]) c2++;
            if (heap[c2] >= v) break;
            heap[i] = heap[c2];
            i = c2;
        }
        heap[i] = v;
    };
    const bool serp = prior && !env_int("KB_BIN_PRIOR_LPT", 0);
    for (size_t k = 0; serp && k < items.size(); k++) {
        const Item& it = items[k];
        const uint32_t r = (uint32_t)(k / NB), q = (uint32_t)(k % NB);
        const uint32_t b = (r & 1u) ? NB - 1u - q : q;  // (at most ceil(items / NB) <= 248 per bucket)
        if (it.sub == ~0u) h[it.mm - half] = b;
        else subs[(h[it.mm - half] & 0x0FFFFFFFu) + it.sub] = (uint16_t)b;
        nm[b]++;
        heap[b] += (uint64_t)std::llround(std::min(it.w, 1e12) * 16.0) << 11;  // (loads: heap[b] >> 11)
    }
    for (const Item& it : items) {
        if (serp) break;
        while (hn > 1 && nm[heap[0] & 2047u] >= 248) {  // full: retire it
            std::swap(heap[0], heap[--hn]);  // (kept past the heap: its load still counts)
            sift(0);
        }
        const uint32_t b = (uint32_t)(heap[0] & 2047u);
        if (it.sub == ~0u) h[it.mm - half] = b;
        else subs[(h[it.mm - half] & 0x0FFFFFFFu) + it.sub] = (uint16_t)b;
        nm[b]++;
        heap[0] += (uint64_t)std::llround(std::min(it.w, 1e12) * 16.0) << 11;
        sift(0);
    }
    double want_max = 0, want_tot = 0;
    for (uint32_t i = 0; i < NB; i++) {
        const double ld = (double)(heap[i] >> 11) / 16.0;
        want_max = std::max(want_max, ld);
        want_tot += ld;
    }
    const double tb3 = now_ms();
    kb_ctx::BucketMap* m = bmap_find(c, NB);
    if (!m) {
        c->bmaps.emplace_back();
        m = &c->bmaps.back();
        m->key = bmap_key(c);
        m->nb = NB;
    }
    HIPCHK(m->map.ensure_exact(half));
    HIPCHK(m->sub.ensure(std::max<size_t>(subs.size(), 1)));
    // uploaded from the context's pinned staging (a pageable copy stages
    // through the runtime's bounce buffers: milliseconds on a context's first
    // use); the last upload must have left it
    const uint64_t need = half * sizeof(uint32_t) + subs.size() * sizeof(uint16_t);
    if (c->map_stage_used) HIPCHK(hipEventSynchronize(c->map_done));
    HIPCHK(c->map_stage.ensure(need));
    memcpy(c->map_stage.p, h.data(), half * sizeof(uint32_t));
    if (!subs.empty()) memcpy(c->map_stage.p + half * sizeof(uint32_t), subs.data(), subs.size() * sizeof(uint16_t));
    HIPCHK(hipMemcpyAsync(m->map.p, c->map_stage.p, half * sizeof(uint32_t), hipMemcpyHostToDevice, c->s));
    if (!subs.empty())
        HIPCHK(hipMemcpyAsync(m->sub.p, c->map_stage.p + half * sizeof(uint32_t), subs.size() * sizeof(uint16_t),
                              hipMemcpyHostToDevice, c->s));
    HIPCHK(hipEventRecord(c->map_done, c->s));
    c->map_stage_used = true;
    KB_DBG("bmap_build: %zu items, setup %.3f sort %.3f pack %.3f upload %.3f ms\n", items.size(), tb1 - tb0,
           tb2 - tb1, tb3 - tb2, now_ms() - tb3);
    m->h_map = std::move(h);
    m->stale = false;
    m->pending = false;
    m->split = n_split;
    m->want_max = (uint64_t)want_max + 1;
    m->want_tot = (uint64_t)want_tot + 1;
    // the region stride (records per bucket) this key's next pass writes with:
    // the largest bucket the packing expects plus a fifth (dense regions: a
    // sparse stride spreads a block's scattered record stores over more
    // pages), a larger bucket reruns the pass bigger
    // (a rebuilt map keeps the stride its key's passes have needed so far:
    // the packing's expectation runs some 10-25 % under the fullest bucket)
    m->cap = std::max<uint64_t>(m->cap, m->want_max + m->want_max / 3 + 256);
    return KB_OK;
}

// Learning a key's map from a bucketed pass: its bins' descriptors (records,
// occurrences, mmer | sub-bin << 16) give the records and occurrences per
// mmer (a split mmer's sub-bins add up) and each sub-bin's own records.  The
// descriptors ride the finalize's last copy (bmap_stage); the map itself is
// rebuilt when the key is next binned (bmap_apply), so no finalize waits on
// the packing -- a one-shot caller never pays it.
bool kb::bmap_wants(kb_ctx* c, uint32_t NB, uint64_t R) {
    if (!env_int("KB_BIN_BALANCE", 1) || R < (uint64_t)std::max(0, env_int("KB_BIN_BALANCE_MIN", 1 << 18)))
        return false;
    if (c->p.K < 2 * c->p.M) return false;  // (K < 2M: no map, see binned_buckets)
    const kb_ctx::BucketMap* m = bmap_find(c, NB);
    return !m || m->stale;
}

int kb::bmap_apply(kb_ctx* c, uint32_t NB, const uint32_t* mm, const uint32_t* cnt, const uint32_t* occ,
                      uint64_t nbins, double rho) {
    const kb_ctx::BucketMap* m = bmap_find(c, NB);
    const uint32_t half = 1u << (2 * c->p.M - 1);
    c->mmer_w.assign(half, 0);
    c->mmer_o.assign(half, 0);
    c->sub_w.clear();
    for (uint64_t b = 0; b < nbins; b++) {
        const uint32_t mmer = mm[b] & 0xFFFFu, sub = mm[b] >> 16;
        if (mmer < half || mmer >= 2 * half) continue;
        c->mmer_w[mmer - half] += std::max(cnt[b], 1u);
        c->mmer_o[mmer - half] += occ[b];
        if (m && m->split && !m->h_map.empty() && (m->h_map[mmer - half] & BM_SPLIT))
            c->sub_w[((uint64_t)mmer << 16) | sub] += std::max(cnt[b], 1u);
    }
    return bmap_build(c, NB, rho);
}

// A context's first pass of a (part, part_n) key has no learned map.  Hashed
// into the buckets, the records would be very uneven (the minimizer rule
// makes mmer frequencies skewed: the largest hashed bucket holds ~8x the
// mean), which took a counting pass to lay the regions out exactly.  Instead
// the first pass packs the buckets by a PRIOR: on uniform sequence, a
// canonical mmer with canonical score c is a window's leftmost maximum
// (binning.c:972) about as often as all W - 1 other positions score below it,
// i.e. in proportion to ((c - 2^(2M-1)) / 2^(2M-1))^(W-1) (W = K - M + 1
// positions; each canonical score stands for two strings).  Packed by that
// weight, buckets come out as even as packed by the true counts (simulated
// at K31 M7: max/mean 1.85 either way, 6.4 hashed).  The records expected per
// read, 2 (L - K + 1) / (K - M + 2), scale it.  The prior map is marked stale,
// so the pass's own bins replace it.
int kb::bmap_prior(kb_ctx* c, uint32_t NB) {
    const int K = c->p.K, M = c->p.M;
    const uint32_t half = 1u << (2 * M - 1);
    double R_est = 0;
    for (auto& b : c->batches) {
        if (b.routed || !b.n_reads) continue;
        if (b.superkmers) {
            R_est += (double)b.n_reads;
        } else {
            const double L = std::min(b.RW * 32.0, (double)c->p.max_read_len);
            R_est += (double)b.n_reads * std::max(1.0, 2.0 * std::max(1.0, L - K + 1) / (K - M + 2));
        }
    }
    const bool reads_part = c->part_n > 1 && std::none_of(c->batches.begin(), c->batches.end(),
                                                          [](const Batch& b) { return b.superkmers; });
    const std::vector<double>& p = c->prior_p;  // (kb_create: the shape depends on K and M only)
    double tot = 0, mine = 0;
    for (uint32_t i = 0; i < half; i++) {
        tot += p[i];
        if (c->part_n <= 1 || dest_of(half + i, c->part_n, PART_SALT) == c->part) mine += p[i];
    }
    // reads scanned for one partition emit only its records; received ones are its own
    const double R_part = reads_part ? R_est * mine / std::max(tot, 1e-300) : R_est;
    c->mmer_w.assign(half, 0);
    c->mmer_o.assign(half, 0);
    for (uint32_t i = 0; i < half; i++) {
        const double w = R_part * p[i] / std::max(mine, 1e-300);
        c->mmer_w[i] = (uint32_t)std::min(4e9, std::ceil(w));
    }
    // (no density learned yet: a typical one -- splits then follow the keys as well as the loads)
    const int rc = bmap_build(c, NB, c->rho > 0.f ? (double)c->rho : 0.1, true);
    if (rc) return rc;
    kb_ctx::BucketMap* m = bmap_find(c, NB);
    m->stale = true;  // (the pass learns the real one)
    // a prior misses real data's skew more than a learned map: a wider stride
    // (an overflowing bucket reruns the pass bigger)
    m->cap = 3 * m->want_max + 1024;
    return KB_OK;
}

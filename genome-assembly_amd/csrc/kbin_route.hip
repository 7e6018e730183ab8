// kbin_route.hip -- multi-GPU routing on the host side: the owner table, the
// kb_route_* calls, kb_split_passes and the receiving end's submit.
#include <cmath>

#include "kbin_host.h"

// Owner ranks.  The owner of a canonical mmer had been a hash
// of it modulo the ranks; the minimizer rule skews the mmers' loads (bmap_prior),
// so at 8 ranks the busiest rank bound 1.19x the mean k-mers on C2's reads,
// and 1.4-1.7x inside one pass of C4's and C5's partitioned legs (the pass
// keeps a hashed fifth or quarter of the mmers).  Instead every pass packs
// its own canonical mmers onto the ranks, heaviest expected load first, each
// onto the least-loaded rank (ties: the lower rank) -- LPT over bmap_prior's
// weight shape ((i + 1) / half)^(K - M), the expected signature frequency on
// uniform sequence: C2 at 8 ranks 1.019x.  A function of (K, M, ranks, part,
// part_n) only, so every rank and process computes the same table; mmers of
// other passes keep the hash (never routed in this pass).  K < 2M codes are
// not canonical (binning.c:992-1021): the hash, as before.
static void owner_table_host(int K, int M, uint32_t n_dest, uint32_t part, uint32_t part_n, uint8_t* out) {
    const uint32_t half = 1u << (2 * M - 1);
    std::vector<double> load(n_dest, 0.0);
    for (uint32_t i = half; i-- > 0;) {  // the weight grows with i: heaviest first
        const uint32_t mm = half + i;
        if (part_n > 1 && dest_of(mm, part_n, PART_SALT) != part) {
            out[i] = (uint8_t)dest_of(mm, n_dest, OWNER_SALT);
            continue;
        }
        uint32_t r = 0;
        for (uint32_t d = 1; d < n_dest; d++)
            if (load[d] < load[r]) r = d;
        out[i] = (uint8_t)r;
        load[r] += std::pow((double)(i + 1) / half, K - M);
    }
}

extern "C" int kb_owner_table(int K, int M, uint32_t n_dest, uint32_t part, uint32_t n_parts, uint8_t* out) {
    if (!out) return fail(KB_EINVAL, "null argument");
    if (M < 1 || M > 8 || K < M || K > 63) return fail(KB_EINVAL, "K=%d, M=%d outside 1 <= M <= 8, M <= K <= 63", K, M);
    if (n_dest < 1 || n_dest > 64) return fail(KB_EINVAL, "n_dest=%u outside [1,64]", n_dest);
    if (n_parts < 1 || part >= n_parts) return fail(KB_EINVAL, "part %u of %u", part, n_parts);
    owner_table_host(K, M, n_dest, part, n_parts, out);
    return KB_OK;
}

// the context's owner table for n_dest ranks in its current pass, on the
// device (null for K < 2M: the hash)
static int owner_map_dev(kb_ctx* c, uint32_t n_dest, const uint8_t** out) {
    *out = nullptr;
    if (c->p.K < 2 * c->p.M) return KB_OK;
    const uint32_t pn = std::max(1u, c->part_n), pt = pn > 1 ? c->part : 0u;
    const uint64_t key = (uint64_t)n_dest | ((uint64_t)pt << 8) | ((uint64_t)pn << 36);
    const uint32_t half = 1u << (2 * c->p.M - 1);
    auto& t = c->owners[key];  // (a partitioned job's passes each keep theirs)
    if (!t.second.p) {
        t.first.resize(half);
        owner_table_host(c->p.K, c->p.M, n_dest, pt, pn, t.first.data());
        HIPCHK(t.second.ensure_exact(half));
        HIPCHK(hipMemcpyAsync(t.second.p, t.first.data(), half, hipMemcpyHostToDevice, c->s));
    }
    *out = t.second.p;
    return KB_OK;
}

// routing through the binned engine's record pass: records in read order,
// destination = owner(mmer); counts now, a stable sort by destination and
// the pack in kb_route_pack (same record format and order as route_kernel)
static int route_plan_binned(kb_ctx* c, uint32_t G, uint64_t* h_counts) {
    HIPCHK(c->totals.ensure(KB_TOTALS));
    uint64_t R = 0, N = 0;
    int rc = binned_read_records(c, R, N, true);  // routed records keep read order
    if (rc) return rc;
    rc = read_id_map(c, c->route_affine, c->route_id_c);
    if (rc) return rc;
    HIPCHK(c->rcount.ensure(64));
    HIPCHK(hipMemsetAsync(c->rcount.p, 0, 64 * sizeof(unsigned long long), c->s));
    const uint8_t* om = nullptr;
    rc = owner_map_dev(c, G, &om);
    if (rc) return rc;
    HIPCHK(launch_route_dest(c->occ_a.p, R, G, om, c->p.M, c->occ_b.p, c->rcount.p, c->s));
    std::vector<unsigned long long> cnt(G);
    HIPCHK(hipMemcpyAsync(cnt.data(), c->rcount.p, G * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    uint64_t tot = 0;
    for (uint32_t d = 0; d < G; d++) {
        h_counts[d] = cnt[d];
        tot += h_counts[d];
    }
    if (tot != R) return fail(KB_EDEVICE, "internal: routed %llu of %llu records", (unsigned long long)tot,
                              (unsigned long long)R);
    if (R > 0xFFFFFFFFull) return fail(KB_EOVERFLOW, "more than 2^32 routed records");
    c->route_binned = true;
    c->route_R = R;
    c->route_G = G;
    return KB_OK;
}

static int route_pack_binned(kb_ctx* c, uint64_t* d_send) {
    const uint64_t R = c->route_R;
    if (R && !d_send) return fail(KB_EINVAL, "null send buffer");
    int bits = 1;
    while ((1u << bits) < c->route_G) bits++;
    const uint64_t nflags = onesweep_flag_elems(R);
    if (c->os_flags.cap < nflags || c->os_epoch > (1u << 24) - 8) {
        HIPCHK(c->os_flags.ensure(nflags));
        HIPCHK(hipMemsetAsync(c->os_flags.p, 0, c->os_flags.cap * sizeof(uint64_t), c->s));
        c->os_epoch = 0;
    }
    HIPCHK(c->os_aux.ensure(OS_AUX_WORDS));
    uint64_t* sorted = nullptr;
    HIPCHK(launch_onesweep(c->occ_b.p, c->occ_a.p, R, bits, c->os_flags.p, c->os_aux.p, &c->os_epoch,
                           &sorted, c->s));
    HIPCHK(launch_route_pack_binned(sorted, c->pay.p, R, rec_words(c),
                                    c->route_affine ? nullptr : c->read_ids.p,
                                    (uint32_t)(c->route_affine ? c->route_id_c : 0), d_send, c->s));
    if (R) HIPCHK(hipMemcpyAsync(c->h_misc + HM_RADIX_ERR, c->os_aux.p + OS_AUX_ERR, sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
    else c->h_misc[HM_RADIX_ERR] = 0;
    HIPCHK(hipStreamSynchronize(c->s));
    if (c->h_misc[HM_RADIX_ERR]) return fail(KB_EDEVICE, "radix look-back timed out (device error word %u)", c->h_misc[HM_RADIX_ERR]);
    for (auto& b : c->batches)
        if (!b.superkmers) b.routed = true;
    c->route_G = 0;
    c->route_binned = false;
    return KB_OK;
}

extern "C" int kb_record_words(kb_ctx* c, uint32_t* out) {
    if (!c || !out) return fail(KB_EINVAL, "null argument");
    *out = (uint32_t)rec_words(c);
    return KB_OK;
}

extern "C" int kb_route_plan(kb_ctx* c, uint32_t n_dest, uint64_t* h_counts) {
    if (!c || !h_counts) return fail(KB_EINVAL, "null argument");
    // (K < 2M: routed records carry the complement flag, ROUTED_REV_BIT; the
    // binned engine's record pass walks the live incremental branch)
    if (c->p.K < 2 * c->p.M && !(binned_applies(c) && c->KW == 1))
        return fail(KB_EINVAL, "K=%d < 2M=%d routes through the binned engine only", c->p.K, 2 * c->p.M);
    if (n_dest < 1 || n_dest > 64) return fail(KB_EINVAL, "n_dest=%u outside [1,64]", n_dest);
    if (c->finalized) return fail(KB_ESTATE, "route after finalize (call kb_reset)");
    int rc = set_device(c);
    if (rc) return rc;
    // every host batch routed from here must be ACGT: records built from an
    // invalid read would otherwise reach the peers, whose finalize succeeds
    rc = ingest_check(c, true);
    if (rc) return rc;
    if (binned_applies(c) && c->KW == 1) return route_plan_binned(c, n_dest, h_counts);
    c->route_binned = false;
    std::vector<uint64_t> tot(n_dest, 0);
    for (auto& b : c->batches) {
        if (b.superkmers || b.routed) continue;
        const uint64_t cells = (uint64_t)n_dest * b.n_reads;
        rc = batch_ids(c, b);
        if (rc) return rc;
        if (b.route_offs) (void)hipFree(b.route_offs);
        b.route_offs = nullptr;
        HIPCHK(hipMalloc((void**)&b.route_offs, std::max<uint64_t>(cells, 1) * sizeof(uint32_t)));
        RouteArgs a{};
        a.words = b.words;
        a.lens = b.lens;
        a.ids = b.ids;
        a.n_reads = b.n_reads;
        a.offs = b.route_offs;
        a.G = n_dest;
        a.part = c->part;
        a.part_n = c->part_n;
        a.rec_words = rec_words(c);
        a.RW = b.RW;
        a.K = c->p.K;
        a.M = c->p.M;
        rc = owner_map_dev(c, n_dest, &a.owner_map);
        if (rc) return rc;
        HIPCHK(launch_route(a, false, c->s));
        // dest-major exclusive scan -> every (dest, read) slot in a dest-major buffer
        HIPCHK(c->scratch.ensure(std::max(scan_u32_scratch_elems(cells), c->scratch.cap)));
        std::vector<uint32_t> edge(n_dest + 1, 0);
        HIPCHK(launch_scan_u32(b.route_offs, cells, c->scratch.p, c->scratch.cap, c->s));
        uint64_t grand = 0;
        const uint64_t nb = scan_u32_scratch_elems(cells) - 2;
        HIPCHK(hipMemcpyAsync(&grand, c->scratch.p + nb, 8, hipMemcpyDeviceToHost, c->s));
        for (uint32_t d = 0; d < n_dest; d++)
            HIPCHK(hipMemcpyAsync(&edge[d], b.route_offs + (uint64_t)d * b.n_reads, 4,
                                  hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipStreamSynchronize(c->s));
        edge[n_dest] = (uint32_t)grand;
        b.route_tot.assign(n_dest, 0);
        for (uint32_t d = 0; d < n_dest; d++) {
            b.route_tot[d] = (uint64_t)edge[d + 1] - edge[d];
            tot[d] += b.route_tot[d];
        }
    }
    c->route_G = n_dest;
    for (uint32_t d = 0; d < n_dest; d++) h_counts[d] = tot[d];
    return KB_OK;
}

// kb_route_scatter (destinations = owner ranks) and kb_split_passes
// (destinations = kb_set_partition passes): one super-k-mer pass into
// per-destination regions, the destination a hash of the canonical mmer
static int scatter_regions(kb_ctx* c, uint32_t n_dest, uint64_t* d_regions, uint64_t region_cap,
                           uint64_t* h_counts, uint64_t salt, bool by_pass) {
    if (!c || !h_counts) return fail(KB_EINVAL, "null argument");
    if (n_dest < 1 || n_dest > 64) return fail(KB_EINVAL, "n_dest=%u outside [1,64]", n_dest);
    if (by_pass && c->part_n > 1) return fail(KB_ESTATE, "kb_split_passes on a partitioned context");
    if (c->finalized) return fail(KB_ESTATE, "route after finalize (call kb_reset)");
    if (!binned_applies(c)) return fail(KB_EINVAL, "kb_route_scatter needs the binned engine (use plan/pack)");
    for (auto& b : c->batches)
        if (!b.routed && !b.superkmers && b.RW > 16)
            return fail(KB_EINVAL, "kb_route_scatter serves reads of <= 512 bp (use plan/pack)");
    if (region_cap && !d_regions) return fail(KB_EINVAL, "null regions");
    if (region_cap >= 0xFFFFFFFFull) return fail(KB_EINVAL, "region_cap must be below 2^32 records");
    int rc = set_device(c);
    if (rc) return rc;
    rc = ingest_check(c, true);  // (as kb_route_plan: nothing invalid leaves this context)
    if (rc) return rc;
    bool affine = false;
    int64_t id_c = 0;
    rc = read_id_map(c, affine, id_c);
    if (rc) return rc;
    HIPCHK(c->rcount.ensure(64));
    HIPCHK(hipMemsetAsync(c->rcount.p, 0, 64 * sizeof(unsigned long long), c->s));
    for (auto& b : c->batches) {
        if (b.routed || b.superkmers || !b.n_reads) continue;
        SkScanArgs a{};
        a.part = c->part;
        a.part_n = c->part_n;
        a.words = b.words;
        a.lens = b.lens;
        a.n_reads = b.n_reads;
        a.ord_base = (uint32_t)b.ord_base;
        a.RW = b.RW;
        a.K = c->p.K;
        a.M = c->p.M;
        a.regions = d_regions;
        a.region_cap = region_cap;
        a.dest_ctr = c->rcount.p;
        (void)by_pass;
        a.read_ids = affine ? nullptr : c->read_ids.p;
        a.id_off = (uint32_t)(affine ? id_c : 0);
        a.G = n_dest;
        a.dest_salt = salt;  // OWNER_SALT or PART_SALT (kbin_hash.h)
        if (!by_pass) {  // ranks: the pass's owner table (passes: the partition hash)
            const int orc = owner_map_dev(c, n_dest, &a.owner_map);
            if (orc) return orc;
        }
        a.rw = rec_words(c);
        HIPCHK(launch_sk(a, true, c->s));
    }
    std::vector<unsigned long long> cnt(n_dest);
    HIPCHK(hipMemcpyAsync(cnt.data(), c->rcount.p, n_dest * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    bool over = false;
    for (uint32_t d = 0; d < n_dest; d++) {
        h_counts[d] = cnt[d];
        over |= cnt[d] > region_cap;
    }
    if (over) return fail(KB_EOVERFLOW, "a destination needs more than %llu records (see counts)",
                          (unsigned long long)region_cap);
    for (auto& b : c->batches)
        if (!b.superkmers) b.routed = true;
    return KB_OK;
}

extern "C" int kb_route_scatter(kb_ctx* c, uint32_t n_dest, uint64_t* d_regions, uint64_t region_cap,
                                uint64_t* h_counts) {
    return scatter_regions(c, n_dest, d_regions, region_cap, h_counts, OWNER_SALT, false);
}

extern "C" int kb_split_passes(kb_ctx* c, uint32_t n_parts, uint64_t* d_regions, uint64_t region_cap,
                               uint64_t* h_counts) {
    return scatter_regions(c, n_parts, d_regions, region_cap, h_counts, PART_SALT, true);
}

extern "C" int kb_route_pack(kb_ctx* c, uint64_t* d_send) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (!c->route_G) return fail(KB_ESTATE, "kb_route_pack before kb_route_plan");
    int rc = set_device(c);
    if (rc) return rc;
    if (c->route_binned) return route_pack_binned(c, d_send);
    const uint32_t G = c->route_G;
    // destination d's records start at sum_{d'<d} total(d'); inside it, batches in order
    std::vector<uint64_t> dest_base(G, 0), seen(G, 0);
    {
        std::vector<uint64_t> tot(G, 0);
        for (auto& b : c->batches)
            if (!b.superkmers && !b.routed && b.route_offs)
                for (uint32_t d = 0; d < G; d++) tot[d] += b.route_tot[d];
        uint64_t acc = 0;
        for (uint32_t d = 0; d < G; d++) {
            dest_base[d] = acc;
            acc += tot[d];
        }
        if (acc && !d_send) return fail(KB_EINVAL, "null send buffer");
        if (acc > 0xFFFFFFFFull) return fail(KB_EOVERFLOW, "more than 2^32 routed records");
    }
    DevBuf<uint64_t> adj;
    HIPCHK(adj.ensure(G));
    for (auto& b : c->batches) {
        if (b.superkmers || b.routed || !b.route_offs) continue;
        std::vector<uint64_t> h_adj(G);
        uint64_t below = 0;  // sum_{d'<d} total_b(d'): already inside the scanned offsets
        for (uint32_t d = 0; d < G; d++) {
            h_adj[d] = dest_base[d] + seen[d] - below;
            below += b.route_tot[d];
            seen[d] += b.route_tot[d];
        }
        HIPCHK(hipMemcpyAsync(adj.p, h_adj.data(), G * 8, hipMemcpyHostToDevice, c->s));
        RouteArgs a{};
        a.words = b.words;
        a.lens = b.lens;
        a.ids = b.ids;
        a.n_reads = b.n_reads;
        a.offs = b.route_offs;
        a.adj = adj.p;
        a.out = d_send;
        a.G = G;
        a.part = c->part;  // the same records the plan counted
        a.part_n = c->part_n;
        a.rec_words = rec_words(c);
        a.RW = b.RW;
        a.K = c->p.K;
        a.M = c->p.M;
        {
            const int orc = owner_map_dev(c, G, &a.owner_map);  // (the plan's table)
            if (orc) return orc;
        }
        HIPCHK(launch_route(a, true, c->s));
        HIPCHK(hipStreamSynchronize(c->s));  // h_adj / adj reuse
        b.routed = true;
    }
    adj.release();
    c->route_G = 0;
    return KB_OK;
}

extern "C" int kb_submit_superkmers_device(kb_ctx* c, const uint64_t* d_recs, uint64_t n_rec) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (c->finalized) return fail(KB_ESTATE, "submit after finalize (call kb_reset)");
    if (n_rec == 0) return KB_OK;
    if (!d_recs) return fail(KB_EINVAL, "null records");
    if (n_rec > 0xFFFFFFFFull) return fail(KB_EOVERFLOW, "more than 2^32 records");
    int rc = set_device(c);
    if (rc) return rc;
    Batch b;
    b.superkmers = true;
    b.recs = d_recs;
    b.n_reads = n_rec;
    c->batches.push_back(b);  // occurrence offsets are computed by the engine that bins them
    return KB_OK;
}

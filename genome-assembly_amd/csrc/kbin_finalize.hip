// kbin_finalize.hip -- the binned engine's finalize on the host side: the
// record passes, the bucket ordering, and finalize_binned in its steps.
#include <cmath>

#include "kbin_host.h"

// ---------------------------------------------------------------------------
// binned engine: super-k-mers (kbin_sk.hip) -> sort by mmer (kbin_plan.hip's
// bucket ordering, or onesweep) -> one LDS table per bin (kbin_bins.hip).  Eligible for K <= 31 reads binned here, no first-occurrence
// tracking.
// ---------------------------------------------------------------------------

// ---- phase A (reads): one record per super-k-mer of every unrouted read
// batch -- pay[3t..3t+2] and keys[t] in occ_a, t in read order; returns the
// record count R and the k-mer count N (one host sync)
int kb::binned_read_records(kb_ctx* c, uint64_t& R, uint64_t& N, bool ordered) {
    const int M = c->p.M;
    const uint64_t nr = c->n_reads;
    // one pass (records allocated per block, any order) when every batch takes
    // the thread-per-read kernel and the buffers sized by the k-mer bound fit
    uint64_t nb = 0;
    bool one_pass = !ordered;
    for (auto& b : c->batches) {
        if (b.routed || b.superkmers) continue;
        if (b.RW > 16) one_pass = false;
        nb += b.n_reads * (uint64_t)std::max(0, b.RW * 32 - c->p.K + 1);
    }
    if (one_pass && nb < 0xFFFFFFFFull && nb * 40 <= (32ull << 30)) {
        HIPCHK(c->pay.ensure(3 * nb + 3));
        HIPCHK(c->occ_a.ensure(nb + 4));
        HIPCHK(c->occ_b.ensure(nb + 4));  // radix ping-pong (R <= nb) and ids by ordinal
        HIPCHK(hipMemsetAsync(c->totals.p + T_KMERS, 0, (T_RECORDS + 1 - T_KMERS) * sizeof(uint64_t), c->s));
        uint64_t kp = 1;
        for (auto& b : c->batches) kp = std::max(kp, sk_blocks(b.n_reads, b.RW));
        HIPCHK(c->kpart.ensure(kp));
        for (auto& b : c->batches) {
            if (b.routed || b.superkmers) continue;
            SkScanArgs a{};
            a.part = c->part;
            a.part_n = c->part_n;
            a.words = b.words;
            a.lens = b.lens;
            a.n_reads = b.n_reads;
            a.rec_ctr = reinterpret_cast<unsigned long long*>(c->totals.p + T_RECORDS);
            a.n_kmers = reinterpret_cast<unsigned long long*>(c->kpart.p);
            a.pay = c->pay.p;
            a.keys = c->occ_a.p;
            a.ord_base = (uint32_t)b.ord_base;
            a.RW = b.RW;
            a.K = c->p.K;
            a.M = M;
            HIPCHK(launch_sk(a, true, c->s));
            HIPCHK(launch_sk_kmers_total(reinterpret_cast<unsigned long long*>(c->kpart.p),
                                         sk_blocks(b.n_reads, b.RW),
                                         reinterpret_cast<unsigned long long*>(c->totals.p + T_KMERS), c->s));
            c->tm.scan_insert_launches++;
        }
        HIPCHK(hipMemcpyAsync(c->h_totals + T_KMERS, c->totals.p + T_KMERS, (T_RECORDS + 1 - T_KMERS) * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipStreamSynchronize(c->s));  // the one mid-finalize sync: R and N size the rest
        N = c->h_totals[T_KMERS];
        R = c->h_totals[T_RECORDS];
        if (R > N || N > nb)
            return fail(KB_EDEVICE, "internal: %llu super-k-mers, %llu k-mers, bound %llu", (unsigned long long)R,
                        (unsigned long long)N, (unsigned long long)nb);
        HIPCHK(c->srec.ensure(3 * R));
        return KB_OK;
    }
    HIPCHK(c->seg.ensure(nr + 1));
    HIPCHK(hipMemsetAsync(c->seg.p, 0, (nr + 1) * sizeof(uint32_t), c->s));
    HIPCHK(c->scratch.ensure(std::max(scan_u32_scratch_elems(nr + 1), c->scratch.cap)));
    HIPCHK(hipMemsetAsync(c->totals.p + T_KMERS, 0, sizeof(uint64_t), c->s));
    {
        uint64_t kp = 1;
        for (auto& b : c->batches) kp = std::max(kp, sk_blocks(b.n_reads, b.RW));
        HIPCHK(c->kpart.ensure(kp));
    }
    for (auto& b : c->batches) {
        if (b.routed || b.superkmers) continue;
        SkScanArgs a{};
        a.part = c->part;
        a.part_n = c->part_n;
        a.words = b.words;
        a.lens = b.lens;
        a.n_reads = b.n_reads;
        a.seg_count = c->seg.p + b.ord_base;
        a.n_kmers = reinterpret_cast<unsigned long long*>(c->kpart.p);
        a.RW = b.RW;
        a.K = c->p.K;
        a.M = M;
        HIPCHK(launch_sk(a, false, c->s));
        HIPCHK(launch_sk_kmers_total(reinterpret_cast<unsigned long long*>(c->kpart.p), sk_blocks(b.n_reads, b.RW),
                                     reinterpret_cast<unsigned long long*>(c->totals.p + T_KMERS), c->s));
        c->tm.scan_insert_launches++;
    }
    HIPCHK(launch_scan_u32(c->seg.p, nr, c->scratch.p, c->scratch.cap, c->s));
    const uint64_t nbs = scan_u32_scratch_elems(nr) - 2;
    HIPCHK(hipMemcpyAsync(c->h_totals + HT_SCAN_R, c->scratch.p + nbs, 8, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipMemcpyAsync(c->h_totals + T_KMERS, c->totals.p + T_KMERS, 8, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));  // the one mid-finalize sync: R and N size the rest
    R = nr ? c->h_totals[HT_SCAN_R] : 0;
    N = nr ? c->h_totals[T_KMERS] : 0;
    if (N >= 0xFFFFFFFFull)
        return fail(KB_EOVERFLOW, "%llu k-mer occurrences in one context (limit 2^32-1)",
                    (unsigned long long)N);
    if (R > N) return fail(KB_EDEVICE, "internal: %llu super-k-mers > %llu k-mers", (unsigned long long)R,
                           (unsigned long long)N);
    HIPCHK(c->pay.ensure(3 * R));
    HIPCHK(c->srec.ensure(3 * R));
    HIPCHK(c->occ_a.ensure(std::max<uint64_t>(R, N / 2 + 4)));
    HIPCHK(c->occ_b.ensure(std::max<uint64_t>(R, N / 2 + 4))  /* ids (u32) + 16-B over-read */);
    for (auto& b : c->batches) {
        if (b.routed || b.superkmers) continue;
        SkScanArgs a{};
        a.part = c->part;
        a.part_n = c->part_n;
        a.words = b.words;
        a.lens = b.lens;
        a.n_reads = b.n_reads;
        a.rec_base = c->seg.p + b.ord_base;
        a.pay = c->pay.p;
        a.keys = c->occ_a.p;
        a.ord_base = (uint32_t)b.ord_base;
        a.RW = b.RW;
        a.K = c->p.K;
        a.M = M;
        HIPCHK(launch_sk(a, true, c->s));
        c->tm.scan_insert_launches++;
    }
    return KB_OK;
}

// ---- phase A, bucketed: records straight into NB local bucket regions
// (hash of the mmer); the learned capacity grows (and the pass reruns) when a
// bucket overflows.  Reads: the one-pass super-k-mer kernel in region mode;
// received: the block-aggregated converter.  Returns R and N (one sync per try).
// The bucket ordering and the bin plan of a bucketed pass: records in rlay
// slots (hdr pairs, then w1 / w3 at 2 rlay / 4 rlay), descriptors for
// max_bins bins.  rcap (speculative launches): records past it are not
// placed -- the layout was sized from the last pass, and the caller reruns.
static int bucket_phase(kb_ctx* c, uint32_t NB, uint64_t rlay, uint64_t max_bins, uint64_t cap, bool rexact,
                        uint64_t rcap, bool plan = true) {
    const int KW = c->KW;
    const uint64_t RWD = 1 + 2 * (uint64_t)KW;
    HIPCHK(c->starts.ensure(max_bins + 1));
    HIPCHK(c->bcount.ensure(max_bins));
    HIPCHK(c->bmmer.ensure(max_bins));
    HIPCHK(c->bocc.ensure(max_bins));
    HIPCHK(c->srec.ensure(RWD * rlay));
    BucketArgs ba{};
    ba.regions = c->regions.p;
    ba.cap = cap;
    ba.rbase = rexact ? c->rbase.p : nullptr;
    ba.bfill = c->bfill.p;
    ba.M = c->p.M;
    ba.hdr = c->srec.p;  // ((header, word 0) pairs, then word 1 / (word 1, word 2) pairs + word 3)
    ba.w1 = c->srec.p + 2 * rlay;
    ba.w3 = KW == 2 ? c->srec.p + 4 * rlay : nullptr;
    ba.spw = 2 * KW;
    HIPCHK(c->bbase.ensure(NB + 1));
    ba.bbase = c->bbase.p;
    ba.bases_ready = 1;  // (bucket_stats_kernel, after the record pass that made these regions)
    {
        // records written by a map-routed pass carry their sub-bin (zero
        // for an unsplit mmer); a hash-routed pass writes spans untouched
        kb_ctx::BucketMap* bm = bmap_find(c, NB);  // (the map the record pass used)
        ba.sub = bm && bm->split ? 1 : 0;
    }
    ba.bin_ctr = reinterpret_cast<unsigned long long*>(c->totals.p + T_BINS);
    ba.bstart = c->starts.p;
    ba.bcount = c->bcount.p;
    ba.bmmer = c->bmmer.p;
    ba.bocc = c->bocc.p;
    ba.max_bins = max_bins;
#ifdef KB_BIN_ABL
    {   // (diagnostic: from a context's third finalize on, so the records
        // the bin kernel reads are the last pass's -- replay input only)
        static int abl_calls = 0;
        ba.ablate = abl_calls++ >= 2 ? env_int("KB_BK_ABLATE", 0) : 0;
    }
#endif
    ba.status = c->misc.p + M_REC_STATUS;
    ba.rcap = rcap;
    HIPCHK(launch_bucket_sort(ba, NB, c->s));
    c->tm.sort_passes = 0;
    if (!plan) return KB_OK;  // (KB_BIN_DESC=0: the caller orders the bins by count)
    HIPCHK(c->border.ensure(max_bins));
    HIPCHK(c->bdesc.ensure(2 * max_bins));
    HIPCHK(launch_bins_plan(c->starts.p, c->bcount.p, c->bmmer.p, c->bocc.p, c->totals.p, max_bins, c->border.p,
                            c->bdesc.p, reinterpret_cast<unsigned long long*>(c->totals.p + T_STAGE), c->s));
    return KB_OK;
}

// What a bucketed record pass read back.  The counting pass copies every
// bucket's fill, N and the status word; a writing pass the record-pass trio
// that bucket_stats folded next to N (one copy).
struct RecRead {
    uint64_t R, mx, N;  // records, the largest bucket, k-mers
    uint32_t status;
};
static RecRead rec_decode(const kb_ctx* c, const std::vector<unsigned long long>& fill, bool counting) {
    RecRead r{};
    r.N = c->h_totals[T_KMERS];
    if (!counting) {
        r.R = c->h_totals[T_REC_SUM];
        r.mx = c->h_totals[T_REC_MAX];
        r.status = (uint32_t)c->h_totals[T_REC_STATUS];
        return r;
    }
    for (unsigned long long f : fill) {
        r.R += f;
        r.mx = std::max<uint64_t>(r.mx, f);
    }
    r.status = c->h_misc[M_REC_STATUS];
    return r;
}

static int binned_buckets(kb_ctx* c, uint32_t NB, bool received, bool zeroed, uint64_t& R, uint64_t& N) {
    const int M = c->p.M;
    c->spec = false;
    // K < 2M: a record's mmer code is the reference's complemented-or-not
    // signature, not the canonical (larger) one the bucket map is indexed by
    // (bucket_map[canon - 2^(2M-1)]): no map -- hash routing, exact regions
    const bool nomap = c->p.K < 2 * M;
    kb_ctx::BucketMap* bm = nomap ? nullptr : bmap_find(c, NB);
    if (bm && bm->pending) {  // the last pass of this key left its bins: rebuild the map from them
        const double t0 = now_ms();
        const int rc = bmap_apply(c, NB, bm->p_mm.data(), bm->p_cnt.data(), bm->p_occ.data(), bm->p_mm.size(),
                                  bm->p_rho);
        if (rc) return rc;
        bm = bmap_find(c, NB);
        KB_DBG("map rebuilt part %u/%u: %.3f ms, %u split\n", c->part, c->part_n, now_ms() - t0, bm->split);
    }
    if (!bm && !nomap && !c->prior_off && env_int("KB_BIN_PRIOR", 1) && env_int("KB_BIN_BALANCE", 1)) {
        const double t0 = now_ms();
        const int rc = bmap_prior(c, NB);
        if (rc) return rc;
        bm = bmap_find(c, NB);
        KB_DBG("prior map part %u/%u: %.3f ms (allocations %.3f), %u split, cap %llu\n", c->part, c->part_n,
               now_ms() - t0, g_alloc_ms, bm->split, (unsigned long long)bm->cap);
    }
    const uint32_t* bmap = bm ? bm->map.p : nullptr;
    const uint16_t* bsub = bm ? bm->sub.p : nullptr;
    // Without any map (KB_BIN_PRIOR=0) the records are routed by hash and the
    // buckets are uneven: a counting pass first (capacity 0: every record
    // counted, none written), then regions laid out exactly (rbase).  With a
    // map (learned, or the prior), one pass into regions of the learned
    // capacity (stride), rerun bigger on overflow.
    const bool exact = bmap == nullptr;
    HIPCHK(c->bfill.ensure(NB));
    // (every batch's per-block k-mer sums side by side: one sum at the end,
    // inside bucket_stats_kernel, where each batch launched a kernel for it)
    uint64_t kp = 1;
    for (auto& b : c->batches) kp += b.routed || b.superkmers ? 0 : sk_blocks(b.n_reads, b.RW);
    HIPCHK(c->kpart.ensure(kp));
    if (exact) HIPCHK(c->rbase.ensure(NB + 1));
    HIPCHK(c->regions.ensure(1));  // (non-null: the record kernel's region mode keys on it)
    const uint64_t RWD = 1 + 2 * (uint64_t)c->KW;
    for (int attempt = 0; attempt < 3; attempt++) {
        const bool counting = exact && attempt == 0;
        const bool use_base = exact && attempt > 0;
        const uint64_t cap = exact ? 0 : bm->cap;
        if (c->spec) HIPCHK(hipStreamSynchronize(c->s));  // (a rerun: nothing in flight reads what is regrown)
        if (attempt > 0 || !zeroed) {  // (the finalize's first clear zeroed them for attempt 0)
            ClearList cl{};
            cl.add(c->bfill.p, NB * sizeof(unsigned long long));
            cl.add(c->totals.p + T_KMERS, sizeof(uint64_t));
            cl.add(c->misc.p + M_REC_STATUS, sizeof(uint32_t));
            if (c->spec) cl.add(c->totals.p + T_BINS, sizeof(uint64_t));  // (the speculative ordering's bins)
            HIPCHK(launch_clear(cl, c->s));
        }
        c->spec = false;
        if (!counting && !use_base) HIPCHK(c->regions.ensure(NB * cap * RWD));
        uint64_t koff = 0;  // (kpart entries written by this attempt's record passes)
        for (auto& b : c->batches) {
            if (b.routed || !b.n_reads) continue;
            if (received) {
                if (!b.superkmers) continue;
                HIPCHK(launch_sk_convert_buckets(b.recs, b.n_reads, rec_words(c), 2 * c->KW, M, NB, c->p.K, bmap, bsub,
                                                 bm && bm->split ? 1 : 0, c->regions.p, cap,
                                                 use_base ? c->rbase.p : nullptr, c->bfill.p, c->misc.p + M_REC_STATUS,
                                                 reinterpret_cast<unsigned long long*>(c->totals.p + T_KMERS), c->s));
            } else {
                if (b.superkmers) continue;
                SkScanArgs a{};
                a.part = c->part;
                a.part_n = c->part_n;
                a.words = b.words;
                a.lens = b.lens;
                a.n_reads = b.n_reads;
                a.ord_base = (uint32_t)b.ord_base;
                a.RW = b.RW;
                a.K = c->p.K;
                a.M = M;
                a.regions = c->regions.p;
                a.region_cap = cap;
                a.region_base = use_base ? c->rbase.p : nullptr;
                a.dest_ctr = c->bfill.p;
                a.G = NB;
                a.dest_salt = BUCKET_SALT;
                a.rw = (int)RWD;  // header + span words
                a.bucket_map = bmap;
                a.sub_map = bsub;
                a.sub_stamp = bm && bm->split ? 1 : 0;
                a.binned_fmt = 1;
                a.n_kmers = reinterpret_cast<unsigned long long*>(c->kpart.p) + koff;
                HIPCHK(launch_sk(a, true, c->s));
                koff += sk_blocks(b.n_reads, b.RW);
            }
            c->tm.scan_insert_launches++;
        }
        if (counting && koff)
            HIPCHK(launch_sk_kmers_total(reinterpret_cast<unsigned long long*>(c->kpart.p), koff,
                                         reinterpret_cast<unsigned long long*>(c->totals.p + T_KMERS), c->s));
        std::vector<unsigned long long> fill(counting ? NB : 0);
        if (counting) {  // the exact layout needs every bucket's count
            HIPCHK(hipMemcpyAsync(fill.data(), c->bfill.p, NB * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                  c->s));
            HIPCHK(hipMemcpyAsync(c->h_totals + T_KMERS, c->totals.p + T_KMERS, sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  c->s));
            HIPCHK(hipMemcpyAsync(c->h_misc + M_REC_STATUS, c->misc.p + M_REC_STATUS, sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, c->s));
        } else {  // R, the largest bucket and the status word folded next to N: one copy
            HIPCHK(c->bbase.ensure(NB + 1));
            HIPCHK(launch_bucket_stats(c->bfill.p, NB, c->misc.p, c->totals.p, cap, use_base ? c->rbase.p : nullptr,
                                       c->bbase.p, reinterpret_cast<unsigned long long*>(c->kpart.p), koff, c->s));
            HIPCHK(hipMemcpyAsync(c->h_totals + T_KMERS, c->totals.p + T_KMERS,
                                  (T_REC_STATUS + 1 - T_KMERS) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
        }
        HIPCHK(hipEventRecord(c->ev_mid, c->s));
        // Speculation: the bucket ordering and the bin plan go out before the
        // host waits for R -- sized from the last pass's R with a quarter of
        // headroom -- so the GPU orders buckets while the host wakes, checks
        // and queues the bin kernel (the wait left it idle ~20 us per C2
        // step).  finalize_binned keeps the result when R fits the layout and
        // the bin count is the budget's, else reruns the phase exactly
        if (!counting && attempt == 0 && c->prev_R && c->rho > 0.f && env_int("KB_BIN_SPEC", 1) &&
            env_int("KB_BIN_DESC", 1)) {
            const uint64_t bk = bin_budget(c, NB);
            if (c->prev_R >= 2 * bk) {
                const uint64_t rl = c->prev_R + c->prev_R / 4 + 65536;
                const int rc = bucket_phase(c, NB, rl, bk, cap, use_base, rl);
                if (rc) return rc;
                c->spec = true;
                c->spec_rlay = rl;
                c->spec_bins = bk;
            }
        }
        HIPCHK(hipEventSynchronize(c->ev_mid));  // the one mid-finalize wait (two without a map): R and N size the rest
        KB_DBG("record pass attempt %d: %s cap %llu, %.3f ms since finalize (allocations %.3f ms)\n", attempt,
               counting ? "counting" : use_base ? "exact" : "stride", (unsigned long long)cap, now_ms() - c->t_fin,
               g_alloc_ms);
        const RecRead rr = rec_decode(c, fill, counting);
        if (rr.status & ST_NEG_ID)
            return fail(KB_EINVAL, "routed read ids must be non-negative (they order the id lists)");
        R = rr.R;
        N = rr.N;
        const uint64_t mx = rr.mx;
        if (counting) {  // exact bases for the writing pass
            std::vector<uint64_t> base(NB + 1, 0);
            for (uint32_t d = 0; d < NB; d++) base[d + 1] = base[d] + fill[d];
            HIPCHK(c->regions.ensure(std::max<uint64_t>(R, 1) * RWD));
            HIPCHK(hipMemcpyAsync(c->rbase.p, base.data(), (NB + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->s));
            HIPCHK(hipStreamSynchronize(c->s));  // (base is a local)
            continue;
        }
        // a map that no longer fits (largest bucket > 1.5x what the packing
        // expected, scaled to this pass's records): relearn it after this pass
        if (bm && R && bm->want_tot &&
            (double)mx > 1.5 * (double)bm->want_max * (double)R / (double)bm->want_tot + 64.0) {
            KB_DBG("map stale: bucket %llu vs expected %.0f (records %llu, k-mers %llu)\n", (unsigned long long)mx,
                   (double)bm->want_max * (double)R / (double)bm->want_tot, (unsigned long long)R,
                   (unsigned long long)N);
            bm->stale = true;
        }
        if (use_base || mx <= cap) {
            c->rexact = use_base;
            c->bucket_cap_used = cap;  // the region stride of this pass (0: exact bases)
            if (!use_base && mx + mx / 16 > cap) bm->cap = mx + mx / 5 + 256;  // (close to full: next passes wider)
            if (N >= 0xFFFFFFFFull)
                return fail(KB_EOVERFLOW, "%llu k-mer occurrences in one context (limit 2^32-1)",
                            (unsigned long long)N);
            if (R > N)
                return fail(KB_EDEVICE, "internal: %llu super-k-mers > %llu k-mers", (unsigned long long)R,
                            (unsigned long long)N);
            return KB_OK;
        }
        // grow and rerun the pass; with headroom, so a later pass's slightly
        // larger bucket does not regrow (each growth maps the regions afresh)
        KB_DBG("record pass rerun: bucket %llu > cap %llu\n", (unsigned long long)mx, (unsigned long long)cap);
        bm->cap = mx + mx / 4 + 1024;
    }
    return fail(KB_EDEVICE, "internal: bucket capacity did not converge");
}

// ---- phase A (received): the routed super-k-mer records of every
// kb_submit_superkmers_device batch, converted in place of phase A; the
// record's read id is its ordinal (ids increase with the global call order)
static int binned_sk_records(kb_ctx* c, uint64_t& R, uint64_t& N) {
    R = 0;
    for (auto& b : c->batches)
        if (b.superkmers) R += b.n_reads;
    if (R > 0xFFFFFFFFull) return fail(KB_EOVERFLOW, "more than 2^32 received records");
    // N <= 63 R; buffers that scale with N are sized after the count
    HIPCHK(c->pay.ensure(3 * R));
    HIPCHK(c->srec.ensure(3 * R));
    HIPCHK(c->occ_a.ensure(std::max<uint64_t>(R, 4)));
    HIPCHK(hipMemsetAsync(c->totals.p + T_KMERS, 0, sizeof(uint64_t), c->s));
    uint64_t off = 0;
    for (auto& b : c->batches) {
        if (!b.superkmers) continue;
        HIPCHK(launch_sk_convert(b.recs, b.n_reads, rec_words(c), off, c->p.M, c->p.K, c->pay.p, c->occ_a.p,
                                 c->misc.p + M_REC_STATUS, reinterpret_cast<unsigned long long*>(c->totals.p + T_KMERS), c->s));
        off += b.n_reads;
        c->tm.scan_insert_launches++;
    }
    HIPCHK(hipMemcpyAsync(c->h_totals + T_KMERS, c->totals.p + T_KMERS, sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    N = c->h_totals[T_KMERS];
    if (N >= 0xFFFFFFFFull)
        return fail(KB_EOVERFLOW, "%llu k-mer occurrences in one context (limit 2^32-1)",
                    (unsigned long long)N);
    HIPCHK(c->occ_b.ensure(std::max<uint64_t>(R, N / 2 + 4)));
    if (c->occ_a.cap < N / 2 + 4) {  // grow, keeping the R keys
        DevBuf<uint64_t> t;
        HIPCHK(t.ensure(std::max<uint64_t>(R, N / 2 + 4)));
        HIPCHK(hipMemcpyAsync(t.p, c->occ_a.p, R * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->s));
        HIPCHK(hipStreamSynchronize(c->s));
        c->occ_a.release();
        c->occ_a = t;
        t.p = nullptr;
        t.cap = 0;
    }
    return KB_OK;
}

// Offset partitions.  A light bin that needs 2^l tables is split by the
// minimizer's offset o inside the k-mer: o is the first occurrence of the
// (canonical) mmer string in the (complemented) k-mer, a function of the key
// (bin_body), so every key lands in exactly one range.  The ranges are chosen
// to hold equal shares of the occurrences, whose distribution over o is
// measured here once per (K, M) on seeded uniform random reads of the sticky
// signature walk (binning.c:922-989): roughly triangular, offset 0 most
// frequent (distinct keys per offset follow occurrences per offset).
static void offset_cuts(int K, int M, uint8_t (&cut)[5][17]) {
    const int W = K - M + 1, L = std::max(150, 4 * K);
    std::vector<double> h(W, 0.0);
    std::vector<uint8_t> r(L);
    std::vector<uint32_t> cs(L);
    const uint32_t full = (1u << (2 * M)) - 1u;
    uint64_t x = 0x243F6A8885A308D3ull;
    for (int read = 0; read < 400; read++) {  // (~50 K occurrences: once per context, in its first finalize)
        for (int i = 0; i < L; i++) {
            x += GOLDEN64;
            uint64_t z = x;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            r[i] = (uint8_t)((z ^ (z >> 31)) & 3u);
        }
        for (int p = 0; p + M <= L; p++) {
            uint32_t s = 0;
            for (int j = 0; j < M; j++) s = s * 4u + r[p + j];
            cs[p] = std::max(s, full - s);
        }
        int sig = -1;
        for (int i = 0; i + K <= L; i++) {
            if (i > sig) {  // leftmost strict argmax (binning.c:972)
                uint32_t best = 0;
                for (int p = i; p <= i + K - M; p++)
                    if (sig < i || cs[p] > best) {
                        best = cs[p];
                        sig = p;
                    }
            }
            h[sig - i] += 1.0;
        }
    }
    double tot = 0;
    for (double v : h) tot += v;
    for (int l = 0; l <= 4; l++) {
        const int R = 1 << l;
        cut[l][0] = 0;
        double acc = 0;
        int o = 0;
        for (int rr = 1; rr < R; rr++) {
            while (o < W && acc + h[o] * 0.5 < tot * rr / R) acc += h[o++];
            // non-empty ranges where W allows
            int c = std::max(o, (int)cut[l][rr - 1] + 1);
            cut[l][rr] = (uint8_t)std::min(c, 63);
        }
        for (int rr = R; rr <= 16; rr++) cut[l][rr] = 64;
    }
}

// ---- finalize_binned in its steps.  The plan of one binned finalize: its
// arguments, what the record pass found and what the knobs choose; fixed over
// the entry-capacity attempts.
struct FinPlan {
    int prune;  // finalize_binned's arguments
    bool affine;
    int64_t id_c;
    bool received;
    bool bucketed;  // fin_records
    uint32_t NB;
    int KW;
    uint64_t R, N;
    uint64_t max_bins, rlay;  // fin_plan
    bool use_desc, spec_ok, stage6, few_bins, learn;
    int opart, ts_log2;
    uint32_t flat_l;
    float* rho_dev;  // fin_order
};

// the finalize's first clear and the record pass: bucketed, NB, KW, R, N
static int fin_records(kb_ctx* c, FinPlan& pl) {
    // bucketed (default): records into local bucket regions, one workgroup
    // orders each bucket; radix: flat records, a global sort by (mmer, n)
    bool all_short = true;
    for (auto& b : c->batches)
        if (!b.routed && !b.superkmers && b.RW > 16) all_short = false;
    pl.bucketed = all_short && env_int("KB_BIN_RADIX", 0) == 0 && !c->bucket_failed;
    pl.KW = c->KW;
    if (pl.KW != 1 && !pl.bucketed) return fail(KB_EDEVICE, "internal: two-word k-mers off the bucketed path");
    // local buckets (power of two, <= 1024): more buckets, more workgroups in flight
    pl.NB = 1;
    while (pl.NB < (uint32_t)std::min(1024, std::max(64, env_int("KB_BIN_NB", 1024)))) pl.NB <<= 1;
    // every counter of this finalize's first attempt zeroed in one launch
    HIPCHK(c->flat_n.ensure_exact(KB_FLAT_N));
    HIPCHK(c->pstat.ensure_exact(KB_PSTAT));
    {
        ClearList cl{};
        cl.add(c->totals.p, T_REPORT * sizeof(uint64_t));
        cl.add(c->misc.p, M_REPORTED * sizeof(uint32_t));  // (status words, the list kernels' queue lengths)
        cl.add(c->flat_n.p, KB_FLAT_N * sizeof(unsigned long long));
        cl.add(c->pstat.p, KB_PSTAT * sizeof(unsigned long long));
        if (pl.bucketed) {
            HIPCHK(c->bfill.ensure(pl.NB));
            cl.add(c->bfill.p, pl.NB * sizeof(unsigned long long));
        }
        if (c->lq.p) cl.add(c->lq.p, sizeof(uint64_t));
        HIPCHK(launch_clear(cl, c->s));
    }
    REC(1);
    int rc = pl.bucketed ? binned_buckets(c, pl.NB, pl.received, true, pl.R, pl.N)
                         : (pl.received ? binned_sk_records(c, pl.R, pl.N) : binned_read_records(c, pl.R, pl.N, false));
    if (rc) return rc;
    c->n_occ = pl.N;
    return KB_OK;
}

// the rest of the plan, and the buffers sized by it
static int fin_plan(kb_ctx* c, FinPlan& pl) {
    const int M = c->p.M, RWD = 1 + 2 * pl.KW;  // record words: header + span words
    // bins: canonical mmers, or context sub-bins of the split ones (a fixed
    // budget: the buffers sized by it keep their size as maps change)
    // (the radix path's bins are mmer codes: canonical ones, 2^(2M-1) of them,
    // except for K < 2M signatures, which take any of the 4^M codes -- ADVICE r05)
    const uint64_t bin_keys = pl.bucketed ? bin_budget(c, pl.NB) : 1ull << (2 * M - (c->p.K < 2 * M ? 0 : 1));
    pl.max_bins = std::max<uint64_t>(1, std::min<uint64_t>(pl.R, bin_keys));
    pl.use_desc = pl.bucketed && env_int("KB_BIN_DESC", 1);
    // the speculative bucket ordering (binned_buckets) stands when R fitted
    // its layout and the bin count is the budget's; otherwise it is rerun
    // exactly, after its counter is zeroed
    pl.spec_ok = pl.use_desc && c->spec && pl.R <= c->spec_rlay && pl.max_bins == c->spec_bins;
    if (c->spec && !pl.spec_ok) {
        HIPCHK(hipStreamSynchronize(c->s));  // (nothing in flight reads what is regrown)
        HIPCHK(hipMemsetAsync(c->totals.p + T_BINS, 0, sizeof(uint64_t), c->s));
    }
    c->spec = false;
    KB_DBG("bucket ordering: %s (R %llu, layout %llu)\n", pl.spec_ok ? "speculative, kept" : "exact",
           (unsigned long long)pl.R, (unsigned long long)(pl.spec_ok ? c->spec_rlay : pl.R));
    pl.rlay = pl.spec_ok ? c->spec_rlay : pl.R;  // (the records' layout: hdr, w1 at 2 rlay, w3 at 4 rlay)
    c->prev_R = pl.R;
    HIPCHK(c->starts.ensure(pl.max_bins + 1));
    HIPCHK(c->bcount.ensure(pl.max_bins));
    HIPCHK(c->bmmer.ensure(pl.max_bins));
    if (pl.bucketed) HIPCHK(c->bocc.ensure(pl.max_bins));
    HIPCHK(c->srec.ensure(RWD * pl.rlay));
    HIPCHK(c->occ_b.ensure(std::max<uint64_t>(pl.R, pl.N / 2 + 4)));  // ids by ordinal (+ radix ping-pong)
    // the stage: 4-B ordinals + 2-B slots (KB_BIN_STAGE6, default), or 8-B
    // entries -- also with first-occurrence tracking, whose entries carry the
    // k-mer's position (the 8-B array is then the only one touched)
    pl.stage6 = env_int("KB_BIN_STAGE6", 1) != 0 && !(c->p.flags & KB_TRACK_FIRST);
    HIPCHK(c->stage.ensure(pl.stage6 ? 1 : std::max<uint64_t>(pl.N, 1)));
    if (pl.stage6) {
        HIPCHK(c->stage_ord.ensure(std::max<uint64_t>(pl.N, 1)));
        HIPCHK(c->stage_slot.ensure(std::max<uint64_t>(pl.N, 1)));
    }
    // heavy bins' flat k-mer lists (touched only when a bin needs many tables)
    // Few, large bins (the last finalize had fewer than three per CU: the
    // mmer-sharded receivers of N ranks, high coverage): bins above 1/32 of a
    // block's fair share are split (their partitions re-expanded by any block)
    // up to depth 3, deeper ones take the flat lists -- both spread over the
    // chip (bins 3.67 -> 2.70 ms per pass on the 8-rank share).  Otherwise
    // flat lists from depth 3 on and no splits (many bins keep the CUs busy).
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->dev));
    pl.few_bins = c->nbins_hint && c->nbins_hint < 3u * (uint32_t)std::max(1, cus);
    // offset partitions (bin_body) make a light bin of depth 3-4 cheaper than
    // flat lists for one-word keys
    // (one-word keys only: two-word bins expand through the ring, which
    // would still walk every k-mer of the bin per range)
    // (K < 2M: no offset partitions -- their exactness needs the leftmost-argmax signature)
    pl.opart = pl.KW == 1 && c->p.K >= 2 * M ? std::min(4, std::max(0, env_int("KB_BIN_OPART", 4))) : 0;
    pl.flat_l =
        (uint32_t)std::max(0, env_int("KB_BIN_FLAT_L", pl.few_bins ? 4 : (pl.KW == 1 && pl.opart >= 4) ? 5 : 3));
    if (pl.flat_l) HIPCHK(c->kstage.ensure(std::max<uint64_t>(pl.KW * pl.N, 1)));
    // LDS table slots: 8192 one-word keys, 4096 two-word keys (bins_lds_bytes <= 160 KiB)
    pl.ts_log2 = std::min(pl.KW == 1 ? 13 : 12, std::max(10, env_int("KB_BIN_TS_LOG2", pl.KW == 1 ? 13 : 12)));
    pl.learn = pl.bucketed && bmap_wants(c, pl.NB, pl.R);  // (before the record pass's map may be replaced)
    return KB_OK;
}

// records into bin order (the bucket ordering unless the speculative one
// stands, or the radix sort), the bins' processing order, and the cold pass's
// density estimate
static int fin_order(kb_ctx* c, FinPlan& pl) {
    const int M = c->p.M;
    if (pl.bucketed) {
        if (!pl.spec_ok) {
            const int rc2 = bucket_phase(c, pl.NB, pl.R, pl.max_bins, c->bucket_cap_used, c->rexact, 0, pl.use_desc);
            if (rc2) return rc2;
        }
    } else {
        // ---- stable sort of the records by (mmer, 63 - n), bin boundaries
        const int key_bits = 2 * M + 6;
        const uint64_t nflags = onesweep_flag_elems(pl.R);
        if (c->os_flags.cap < nflags || c->os_epoch > (1u << 24) - 8) {
            HIPCHK(c->os_flags.ensure(nflags));
            HIPCHK(hipMemsetAsync(c->os_flags.p, 0, c->os_flags.cap * sizeof(uint64_t), c->s));
            c->os_epoch = 0;
        }
        HIPCHK(c->os_aux.ensure(OS_AUX_WORDS));
        HIPCHK(hipMemsetAsync(c->os_aux.p + OS_AUX_ERR, 0, sizeof(uint32_t), c->s));
        HIPCHK(launch_onesweep(c->occ_a.p, c->occ_b.p, pl.R, key_bits, c->os_flags.p, c->os_aux.p,
                               &c->os_epoch, &c->sorted, c->s));
        c->tm.sort_passes = (uint32_t)((key_bits + 7) / 8);
        HIPCHK(c->scratch.ensure(std::max(runs_scratch_elems(pl.R, pl.max_bins), c->scratch.cap)));
        HIPCHK(launch_heads(c->sorted, pl.R, c->starts.p, pl.max_bins, c->scratch.p, c->scratch.cap,
                            c->totals.p, c->s, 38));
        HIPCHK(launch_bins_describe(c->sorted, c->starts.p, c->totals.p, c->bcount.p, c->bmmer.p, pl.max_bins,
                                    c->s));
        HIPCHK(launch_sk_gather(c->sorted, c->pay.p, pl.R, c->srec.p, c->s));
    }
    HIPCHK(c->border.ensure(pl.max_bins));
    if (!pl.use_desc)  // (bucketed: bucket_phase planned the bins from their descriptors; bocc counted by it)
        HIPCHK(launch_bins_order(c->bcount.p, c->totals.p, c->border.p, pl.max_bins, c->s));
    pl.rho_dev = nullptr;
    if (c->rho <= 0.f && pl.N && env_int("KB_BIN_HLL", 1)) {
        // the context's first finalize: distinct keys per occurrence from one
        // HyperLogLog over the records (no learned density yet)
        BinArgs h{};
        h.hdr = c->srec.p;  // ((header, word 0) pairs, then word 1 / (word 1, word 2) pairs + word 3)
        h.w1 = c->srec.p + 2 * pl.rlay;
        h.w3 = pl.KW == 2 ? c->srec.p + 4 * pl.rlay : nullptr;
        h.K = c->p.K;
        h.M = M;
        // large passes estimate from the bins of 1/8 of the mmers (whole bins:
        // the ratio of a sample of bins, 1/8 of the expansion work) -- when the
        // pass holds enough mmers for the sample to be a fair one: at least 64
        // sampled of the canonical mmers a partition expects; received records
        // (one rank's share of the mmers, unknown here) are never sampled
        const uint32_t sample_div = (uint32_t)std::max(1, env_int("KB_BIN_HLL_SAMPLE", 8));
        const uint64_t mm_expect = (1ull << (2 * M - 1)) / std::max<uint32_t>(1u, c->part_n);
        const uint32_t sample = pl.R >= (1u << 20) && !pl.received && mm_expect / sample_div >= 64 ? sample_div : 1u;
        // (registers, the u64 occurrence count, then the estimate: read by the
        // bin kernel from device memory -- the host never waits for it; the
        // finalize's own distinct count replaces it afterwards)
        HIPCHK(c->hll.ensure_exact(4096 + 3));
        HIPCHK(launch_hll(h, pl.R, pl.KW, c->hll.p, sample, c->s));
        pl.rho_dev = reinterpret_cast<float*>(c->hll.p + 4096 + 2);
        HIPCHK(launch_hll_finish(c->hll.p, pl.rho_dev, c->s));
        KB_DBG("hll (sample 1/%u) queued: %.3f ms since finalize\n", sample, now_ms() - c->t_fin);
    }
    return KB_OK;
}

// an attempt's entry arrays; a rerun's counters and status start again
static int fin_entries(kb_ctx* c, const FinPlan& pl, uint64_t ecap, int attempt) {
    HIPCHK(c->e_mmer.ensure(ecap));
    HIPCHK(c->e_cnt.ensure(ecap));
    HIPCHK(c->e_hi.ensure(ecap));
    if (pl.KW == 1 && (c->e_hi_zeroed != c->e_hi.p || c->e_hi_zeroed_cap != c->e_hi.cap)) {
        // K <= 31: every key's high code word is 0; zeroed once per
        // allocation instead of 8 B per entry from bin_kernel each finalize
        HIPCHK(hipMemsetAsync(c->e_hi.p, 0, c->e_hi.cap * sizeof(uint64_t), c->s));
        c->e_hi_zeroed = c->e_hi.p;
        c->e_hi_zeroed_cap = c->e_hi.cap;
    }
    HIPCHK(c->e_lo.ensure(ecap));
    HIPCHK(c->e_off.ensure(ecap));
    if (attempt) {  // the bin kernel's counters and status start again
        HIPCHK(hipMemsetAsync(c->totals.p + T_GCOUNT, 0, (T_WORK + 1 - T_GCOUNT) * sizeof(uint64_t), c->s));
        HIPCHK(hipMemsetAsync(c->totals.p + T_STAGE, 0, (T_TAB_KEYS + 1 - T_STAGE) * sizeof(uint64_t), c->s));
        HIPCHK(hipMemsetAsync(c->misc.p + M_BIN_STATUS, 0, sizeof(uint32_t), c->s));
        if (pl.use_desc)  // (the stage counter starts after the described ranges)
            HIPCHK(launch_bins_desc(c->border.p, c->starts.p, c->bcount.p, c->bmmer.p, c->bocc.p, c->totals.p,
                                    pl.max_bins, c->bdesc.p,
                                    reinterpret_cast<unsigned long long*>(c->totals.p + T_STAGE), c->s));
        REC(3);
    }
    return KB_OK;
}

// the heavy bins' flat-list buffers
static int flat_args(kb_ctx* c, const FinPlan& pl, int attempt, BinArgs& a) {
    HIPCHK(c->flat_list.ensure(pl.max_bins));
    HIPCHK(c->flat_next.ensure(pl.max_bins));
    HIPCHK(c->flat_l0.ensure(pl.max_bins));
    HIPCHK(c->flat_sbase.ensure(pl.max_bins));
    HIPCHK(c->flat_obase.ensure(pl.max_bins));
    // offsets: np + 1 per heavy bin, np < 2 x (expected keys / (fill x TS)) + 1,
    // expected keys <= occurrences, fill x TS >= 0.3 x 1024
    HIPCHK(c->flat_off.ensure(pl.N / 150 + 9 * pl.max_bins + KB_FLAT_MAX + 1));
    HIPCHK(c->flat_cur.ensure(c->flat_off.cap));
    HIPCHK(c->flat_chunk.ensure(pl.max_bins));
    HIPCHK(c->pool_bin.ensure(c->flat_off.cap));
    HIPCHK(c->chunk_bin.ensure(pl.R / 1024 + pl.max_bins + 1));
    if (attempt) HIPCHK(hipMemsetAsync(c->flat_n.p, 0, KB_FLAT_N * sizeof(unsigned long long), c->s));
    a.flat_list = c->flat_list.p;
    a.flat_next = c->flat_next.p;
    a.flat_l0 = c->flat_l0.p;
    a.flat_sbase = c->flat_sbase.p;
    a.flat_off = c->flat_off.p;
    a.flat_cur = c->flat_cur.p;
    a.flat_chunk = c->flat_chunk.p;
    a.pool_bin = c->pool_bin.p;
    a.chunk_bin = c->chunk_bin.p;
    a.flat_obase = c->flat_obase.p;
    a.flat_n = c->flat_n.p;
    a.flat_octr = c->flat_n.p + FN_POOL;
    return KB_OK;
}

static int fill_bin_args(kb_ctx* c, const FinPlan& pl, uint64_t ecap, int attempt, BinArgs& a) {
    const int M = c->p.M;
    a = BinArgs{};
    a.hdr = c->srec.p;  // ((header, word 0) pairs, then word 1 / (word 1, word 2) pairs + word 3)
    a.w1 = c->srec.p + 2 * pl.rlay;
    a.w3 = pl.KW == 2 ? c->srec.p + 4 * pl.rlay : nullptr;
    a.bstart = c->starts.p;
    a.bcount = c->bcount.p;
    a.bmmer = c->bmmer.p;
    a.bocc = pl.bucketed ? c->bocc.p : nullptr;
    a.max_bins = pl.max_bins;
    a.stage_ctr = reinterpret_cast<unsigned long long*>(c->totals.p + T_STAGE);
    a.order = c->border.p;
    a.bdesc = pl.use_desc ? c->bdesc.p : nullptr;
    a.work = reinterpret_cast<unsigned long long*>(c->totals.p + T_WORK);
    a.stage = c->stage.p;
    a.stage_ord = pl.stage6 ? c->stage_ord.p : nullptr;
    a.stage_slot = pl.stage6 ? c->stage_slot.p : nullptr;
    a.kstage = pl.flat_l ? c->kstage.p : nullptr;
    a.flat_l = pl.flat_l;
    a.n_occ = pl.N;
    a.split_div = (uint32_t)std::max(0, env_int("KB_BIN_SPLIT_DIV", pl.few_bins ? 32 : 0));
    a.big_div = (uint32_t)std::max(0, env_int("KB_BIN_BIG_DIV", 2));
    if (pl.flat_l) {
        const int rc = flat_args(c, pl, attempt, a);
        if (rc) return rc;
    }
    a.totals = c->totals.p;
    a.K = c->p.K;
    a.M = M;
    a.keep_gt = pl.prune ? (uint32_t)c->p.cutoff : 0u;
    a.ts_log2 = (uint32_t)pl.ts_log2;
    a.rho = c->rho > 0.f ? c->rho : 0.25f;
    a.rho_dev = pl.rho_dev;
    a.fill = (float)std::min(0.85, std::max(0.3, env_int("KB_BIN_FILL_PCT", 60) / 100.0));
    a.ablate = env_int("KB_BIN_ABLATE", 0);
    a.ringfree = (uint32_t)(env_int("KB_BIN_RINGFREE", 1) != 0);
    a.opart = (uint32_t)pl.opart;
    a.osplit = (uint32_t)(env_int("KB_BIN_OSPLIT", 0) != 0);
    a.fill_light = (float)std::min(0.85, std::max(0.3, env_int("KB_BIN_FILL_LIGHT_PCT", 50) / 100.0));
    if (a.opart) {
        if (c->ocut_km != (c->p.K << 8 | M)) {
            offset_cuts(c->p.K, M, c->ocut);
            c->ocut_km = c->p.K << 8 | M;
        }
        memcpy(a.ocut, c->ocut, sizeof(a.ocut));
    }
    a.heavy_hint = attempt ? ~0ull : c->hint_heavy;
    // LDS id windows in heavy-bin partitions where the last finalize's lists
    // were short on average (C4 share: 588 -> 502 ms per step; C3's lists of
    // ~2300 ids measured 342 -> 351 ms with them)
    a.win_heavy = (uint32_t)(env_int("KB_BIN_WIN_HEAVY", 1) != 0 &&
                             (c->hint_entries == 0 || c->hint_ids <= 128 * c->hint_entries));
    // (bit 1: two-word keys too -- KB_BIN_WIN_HEAVY2; C5 share 510 -> 482 ms
    // per step: its short lists no longer wait for the list kernels, emit
    // 32 -> 0.04 ms, the bin phase +4.5 ms; round 2 had measured 624 -> 641
    // before the pre-filter, r5g29)
    if (a.win_heavy && env_int("KB_BIN_WIN_HEAVY2", 1)) a.win_heavy |= 2u;
    a.gcount = reinterpret_cast<unsigned long long*>(c->totals.p + T_GCOUNT);
    a.status = c->misc.p + M_BIN_STATUS;  // the bin kernel's own status word
    a.e_mmer = c->e_mmer.p;
    a.e_hi = c->e_hi.p;
    a.e_lo = c->e_lo.p;
    a.e_cnt = c->e_cnt.p;
    a.e_off = c->e_off.p;
    a.e_first = nullptr;
    if (c->p.flags & KB_TRACK_FIRST) {
        HIPCHK(c->e_first.ensure(ecap));
        a.e_first = c->e_first.p;
    }
    a.ids_ord = reinterpret_cast<uint32_t*>(pl.bucketed || c->sorted == c->occ_a.p ? c->occ_b.p : c->occ_a.p);
    a.ids_out = c->ids_out.p;
    a.read_ids = pl.affine ? nullptr : c->read_ids.p;
    a.id_off = (uint32_t)(pl.affine ? pl.id_c : 0);
    a.max_entries = ecap - 1;
    a.max_ids = pl.N;
    // lists placed and ordered in LDS id windows by the bins (lists_kernel
    // then takes only the queued items: lists > 256 ids, partitions whose
    // ids took the global path)
    if (env_int("KB_BIN_LDS_LISTS", 1)) {
        // items <= entries (every item holds >= 1 entry): one slot per entry
        const uint64_t* lq_was = c->lq.p;
        HIPCHK(c->lq.ensure(ecap + 1));
        // (the first clear zeroed the head of the queue it saw; a queue
        // allocated since needs its own)
        if (attempt || c->lq.p != lq_was) HIPCHK(hipMemsetAsync(c->lq.p, 0, sizeof(uint64_t), c->s));
        a.lq_n = reinterpret_cast<unsigned long long*>(c->lq.p);
        a.lq_items = c->lq.p + 1;
        a.lq_cap = ecap;
    }
    a.fs_lds = (uint32_t)(env_int("KB_BIN_FSL", 1) != 0);
    a.fsl_run = (uint32_t)std::max(1, env_int("KB_BIN_FSL_RUN", 64));
    // singleton pre-filter for the heavy bins: where most distinct keys are
    // pruned singletons (high error rates, low coverage: C5), learned from
    // the last finalize; exact because a key seen once has count 1 <= cutoff
    {
        const int pf_env = env_int("KB_BIN_PF", -1);
        const bool pf_ok = pl.prune && c->p.cutoff >= 1 && !(c->p.flags & KB_TRACK_FIRST) && pl.flat_l;
        a.pf = pf_ok && (pf_env == 1 || (pf_env < 0 && c->rho >= 0.3f && c->rho_tab > 0.f)) ? 1u : 0u;
        a.rho_tab = c->rho_tab > 0.f ? c->rho_tab : a.rho;
        a.pf_light = a.pf && pl.KW == 2 && env_int("KB_BIN_PF_LIGHT", 1) != 0 ? 1u : 0u;
        if (a.pf_light) c->pfl_regime = true;  // (the next maps split for the sketch)
        a.tab_keys = reinterpret_cast<unsigned long long*>(c->totals.p + T_TAB_KEYS);
    }
    if (attempt) HIPCHK(hipMemsetAsync(c->pstat.p, 0, KB_PSTAT * sizeof(unsigned long long), c->s));
    a.pstat = c->pstat.p;
    a.ldsbar = (uint32_t)(env_int("KB_BIN_LDSBAR", 1) != 0);
    a.ts_adapt = (uint32_t)(env_int("KB_BIN_TS_ADAPT", 1) != 0);
    a.corrupt = (uint32_t)(env_int("KB_DIAG_CORRUPT", 0) != 0);
    a.skew = (uint32_t)std::max(0, env_int("KB_DIAG_SKEW", 0));
    a.diag_alloc = (uint32_t)(env_int("KB_DIAG_ALLOC", 0) != 0);
    // ranked bins where lists are long (the last finalize's mean list
    // length, C3: ~2200 ids): KB_BIN_RANK=0 off, 2 always
    {
        const int rk = env_int("KB_BIN_RANK", 1);
        const bool long_lists = c->hint_entries && c->hint_ids >= 64 * c->hint_entries;
        // (the bitmaps emit the long lists outside the list kernels, which
        // then must take only the queued items: no ranking without the
        // list queue, KB_BIN_LDS_LISTS=0)
        a.rank_mode = (rk == 2 || (rk == 1 && long_lists)) && pl.stage6 && !a.e_first && a.lq_items ? 1u : 0u;
        a.rank_merge = (uint32_t)(env_int("KB_BIN_RANK_MERGE", 1) != 0);
        if (a.rank_mode) c->rank_regime = true;  // (the next maps split finer)
        if (a.rank_mode) {
            HIPCHK(c->rrank.ensure(std::max<uint64_t>(pl.R, 1)));
            HIPCHK(c->rord.ensure(std::max<uint64_t>(pl.R, 1)));
            a.rrank = c->rrank.p;
            a.rord = c->rord.p;
        }
    }
    return KB_OK;
}

static int fill_list_args(kb_ctx* c, const FinPlan& pl, const BinArgs& a, int attempt, ListArgs& la) {
    la = ListArgs{};
    la.totals = c->totals.p;
    la.e_cnt = c->e_cnt.p;
    la.e_off = c->e_off.p;
    la.ids_ord = a.ids_ord;
    la.ids_out = c->ids_out.p;
    la.read_ids = a.read_ids;
    la.id_off = a.id_off;
    la.long_cap = pl.N / 256 + 2;  // lists of > 256 ids
    la.lq_items = a.lq_items;
    la.lq_n = a.lq_n;
    la.lq_cap = a.lq_cap;
    HIPCHK(c->long_q.ensure(2 * la.long_cap));
    la.long_q = c->long_q.p;
    la.long_n = c->misc.p + M_LONG_N;
    la.long_n_zeroed = attempt == 0;  // (the finalize's first clear)
    la.lq_hint = attempt ? ~0ull : c->hint_lq;
    la.long_hint[0] = attempt ? ~0ull : c->hint_long[0];
    la.long_hint[1] = attempt ? ~0ull : c->hint_long[1];
    return KB_OK;
}

// what an attempt read back (fin_readback)
struct FinRead {
    uint64_t entries, ids, bins, bin_over;
    uint64_t asked;  // entries asked of the packed counter (what a rerun must hold)
    uint64_t counted, distinct, tab_keys;
    uint64_t heavy, queued;  // the tail pair
    uint32_t rec_status, bin_status, long_n[2], radix_err;
    uint64_t pstat[KB_PSTAT];
};

// Queue an attempt's read-back, wait for it and decode it.  report: bins_final
// gathered pstat and misc next to the totals (the deferred tail: one copy of
// the low words and the report block); otherwise totals, pstat and misc are
// three copies.  first: the attempt's first wait, which also carries the
// bins' descriptors for the map and the radix sort's error word.
static int fin_readback(kb_ctx* c, const FinPlan& pl, bool report, bool first, FinRead& r) {
    if (report) {
        HIPCHK(hipMemcpyAsync(c->h_totals, c->totals.p, T_REPORT_END * sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
    } else {
        HIPCHK(hipMemcpyAsync(c->h_totals, c->totals.p, (T_QUEUED + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              c->s));
        HIPCHK(hipMemcpyAsync(c->h_totals + T_PSTAT, c->pstat.p, KB_PSTAT * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              c->s));
    }
    if (first && pl.learn) {  // the bins' descriptors for the map (bmap_apply), in the same copy batch
        const uint64_t mb = pl.max_bins;
        HIPCHK(c->h_bins.ensure(3 * mb));
        HIPCHK(hipMemcpyAsync(c->h_bins.p, c->bmmer.p, mb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipMemcpyAsync(c->h_bins.p + mb, c->bcount.p, mb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipMemcpyAsync(c->h_bins.p + 2 * mb, c->bocc.p, mb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
    }
    if (!report)
        HIPCHK(hipMemcpyAsync(c->h_misc, c->misc.p, M_REPORTED * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
    if (first) {
        if (pl.R && !pl.bucketed)
            HIPCHK(hipMemcpyAsync(c->h_misc + HM_RADIX_ERR, c->os_aux.p + OS_AUX_ERR, sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, c->s));
        else c->h_misc[HM_RADIX_ERR] = 0;
    }
    HIPCHK(hipStreamSynchronize(c->s));
    const uint64_t* t = c->h_totals;
    uint32_t m[M_REPORTED];
    for (int k = 0; k < M_REPORTED; k++)
        m[k] = report ? (uint32_t)(t[T_MISC_PAIRS + k / 2] >> (32 * (k & 1))) : c->h_misc[k];
    r.entries = t[T_ENTRIES];
    r.ids = t[T_IDS];
    r.bins = t[T_BINS];
    r.bin_over = t[T_BIN_OVER];
    r.asked = t[T_GCOUNT + G_PACKED] >> 32;
    r.counted = t[T_GCOUNT + G_COUNTED];
    r.distinct = t[T_GCOUNT + G_DISTINCT];
    r.tab_keys = t[T_TAB_KEYS];
    r.heavy = t[T_HEAVY];
    r.queued = t[T_QUEUED];
    r.rec_status = m[M_REC_STATUS];
    r.bin_status = m[M_BIN_STATUS];
    r.long_n[0] = m[M_LONG_N];
    r.long_n[1] = m[M_LONG_N + 1];
    r.radix_err = c->h_misc[HM_RADIX_ERR];
    for (int k = 0; k < KB_PSTAT; k++) r.pstat[k] = t[T_PSTAT + k];
    return KB_OK;
}

// ST_BUCKET_FULL: a bucket held too many mmers -- the finalize runs again on
// another path
static int fin_bucket_full(kb_ctx* c, const FinPlan& pl) {
    c->finalized = false;
    // a learned (or prior) map packed them: forget it and rerun on the
    // hash routing (no prior for this context from now on)
    for (size_t i = 0; i < c->bmaps.size(); i++)
        if (c->bmaps[i].key == bmap_key(c) && c->bmaps[i].nb == pl.NB) {
            c->prior_off = true;
            auto& m = c->bmaps[i];
            m.map.release(); m.sub.release();
            c->bmaps.erase(c->bmaps.begin() + (long)i);
            return finalize_binned(c, pl.prune, pl.affine, pl.id_c, pl.received);
        }
    // the hash itself overflowed: the radix path (K <= 31) or the
    // table engine (K > 31, which has no partitioned passes)
    if (pl.KW == 2 && c->part_n > 1)
        return fail(KB_EINVAL, "a local bucket overflowed with two-word k-mers in a partitioned "
                               "pass (M too large for %u buckets)", pl.NB);
    c->bucket_failed = true;  // until kb_reset
    if (pl.KW == 1) return finalize_binned(c, pl.prune, pl.affine, pl.id_c, pl.received);
    return kb_finalize(c, pl.prune);
}

// device errors and the result's invariants; the context's result counts
static int fin_check(kb_ctx* c, const FinPlan& pl, const FinRead& rb) {
    const uint32_t bst = rb.bin_status;
    if (rb.radix_err) return fail(KB_EDEVICE, "radix look-back timed out (device error word %u)", rb.radix_err);
    if (rb.bin_over) return fail(KB_EDEVICE, "internal: %llu bins > %llu", (unsigned long long)rb.bin_over,
                                    (unsigned long long)pl.max_bins);
    if (bst & ST_TABLE_FULL) return fail(KB_EDEVICE, "internal: CSR capacity exceeded");
    if (rb.rec_status & ST_NEG_ID)
        return fail(KB_EINVAL, "routed read ids must be non-negative (they order the id lists)");
    if (bst & ST_PROBE_LIMIT) return fail(KB_ENOMEM, "a bin exceeded the partition depth");
    // result invariants (a wrong result must not come back as KB_OK): every
    // k-mer of the pass counted exactly once before the prune, and kept
    // entries <= distinct keys <= k-mers
#ifdef KB_BIN_ABL
    static const bool abl_on = env_int("KB_BIN_ABLATE", 0) != 0;  // (phases switched off: wrong results by design)
#else
    constexpr bool abl_on = false;
#endif
    if (!abl_on && (rb.counted != pl.N || rb.entries > rb.distinct || rb.distinct > pl.N))
        return fail(KB_EDEVICE,
                    "internal: result invariant violated (counted %llu of %llu k-mers, %llu entries, %llu distinct)",
                    (unsigned long long)rb.counted, (unsigned long long)pl.N, (unsigned long long)rb.entries,
                    (unsigned long long)rb.distinct);
    c->n_entries = rb.entries;
    c->n_ids = rb.ids;
    c->n_distinct = rb.distinct;
    return KB_OK;
}

// what the next finalize learns from this one (bucket map, capacities,
// densities; pf: the pre-filter ran) and kb_timing
static int fin_publish(kb_ctx* c, const FinPlan& pl, const FinRead& rb, bool pf) {
    if (pl.bucketed) {
        const double rho_now = pl.N ? (double)rb.distinct / (double)pl.N : 0.1;
        KB_DBG("bins done: %.3f ms since finalize (allocations %.3f ms)\n", now_ms() - c->t_fin, g_alloc_ms);
        if (pl.learn) {
            const uint64_t nb = std::min<uint64_t>(rb.bins, pl.max_bins);
            const uint32_t* hb = c->h_bins.p;
            if (const char* dp = getenv("KB_DIAG_BINS")) {  // (diagnostic: this pass's bins, appended)
                if (FILE* f = fopen(dp, "a")) {
                    for (uint64_t i = 0; i < nb; i++)
                        fprintf(f, "%u %u %u %u %u\n", c->part, hb[i] & 0xFFFFu, hb[i] >> 16, hb[pl.max_bins + i],
                                hb[2 * pl.max_bins + i]);
                    fclose(f);
                }
            }
            kb_ctx::BucketMap* bm0 = bmap_find(c, pl.NB);
            if (bm0) {  // rebuilt when this key is next binned
                bm0->p_mm.assign(hb, hb + nb);
                bm0->p_cnt.assign(hb + pl.max_bins, hb + pl.max_bins + nb);
                bm0->p_occ.assign(hb + 2 * pl.max_bins, hb + 2 * pl.max_bins + nb);
                bm0->p_rho = rho_now;
                bm0->pending = true;
            } else {  // (no map at all: KB_BIN_PRIOR=0) the next pass needs one now
                const int rc2 = bmap_apply(c, pl.NB, hb, hb + pl.max_bins, hb + 2 * pl.max_bins, nb, rho_now);
                if (rc2) return rc2;
            }
            KB_DBG("learn part %u/%u: %s (bins %llu, R %llu)\n", c->part, c->part_n, bm0 ? "deferred" : "built",
                   (unsigned long long)nb, (unsigned long long)pl.R);
        }
    }
    c->n_occ_entries_hint = c->n_entries;
    c->ecap_hint = c->n_entries + c->n_entries / 4 + 1024;
    if (pl.N) c->rho = (float)((double)c->n_distinct / (double)pl.N);
    // keys the tables will hold under the pre-filter: measured when it ran,
    // else the kept keys plus a margin for sketch collisions and counts 2..cutoff
    if (pl.N) c->rho_tab = pf ? (float)((double)rb.tab_keys / (double)pl.N * 1.05)
                             : std::min(c->rho, (float)((double)c->n_entries / (double)pl.N * 1.3 + 0.01));
    if (c->timing == KB_TIMING_ALL) {
        HIPCHK(hipEventElapsedTime(&c->tm.scan_insert_ms, c->ev[1], c->ev[2]));
        HIPCHK(hipEventElapsedTime(&c->tm.sort_ms, c->ev[2], c->ev[3]));
        HIPCHK(hipEventElapsedTime(&c->tm.runs_ms, c->ev[3], c->ev[4]));
        HIPCHK(hipEventElapsedTime(&c->tm.emit_ms, c->ev[4], c->ev[5]));
        HIPCHK(hipEventElapsedTime(&c->tm.total_ms, c->ev[0], c->ev[5]));
    } else {
        c->tm.scan_insert_ms = c->tm.sort_ms = c->tm.runs_ms = c->tm.emit_ms = c->tm.total_ms = 0.f;
    }
    if (c->timing) HIPCHK(hipEventElapsedTime(&c->tm.bin_kernel_ms, c->ev[6], c->ev[7]));
    {
        const uint64_t* ps = rb.pstat;  // (BinArgs::pstat)
        c->tm.heavy_bins = (uint32_t)ps[PS_HEAVY];
        c->tm.split_bins = (uint32_t)ps[PS_SPLIT];
        c->tm.partitions = ps[PS_PARTS];
        c->tm.overflow_redos = (uint32_t)ps[PS_REDO];
        c->tm.max_depth = (uint32_t)ps[PS_DEPTH];
        c->tm.prefiltered = ps[PS_PREFILTERED];
        c->tm.offset_partitions = ps[PS_OFFSET];
        c->tm.flat_partitions = ps[PS_FLAT];
        c->tm.light_prefilter_bins = (uint32_t)ps[PS_PF_LIGHT];
        c->tm.ranked_bins = (uint32_t)ps[PS_RANKED];
        c->tm.bitmap_partitions = (uint32_t)ps[PS_BITMAP];
        c->tm.long_lists = rb.long_n[0];
        c->tm.clustered_lists = rb.long_n[1];
        const kb_ctx::BucketMap* bm = pl.bucketed ? bmap_find(c, pl.NB) : nullptr;  // (before this pass's learning)
        c->tm.split_mmers = bm ? bm->split : 0u;
    }
    c->tm.table_slots = 1ull << pl.ts_log2;
    c->tm.n_bins = (uint32_t)rb.bins;
    c->nbins_hint = c->tm.n_bins;
    c->tm.n_superkmers = pl.R;
    c->finalized = true;
    c->exported = false;
    return KB_OK;
}

int kb::finalize_binned(kb_ctx* c, int prune, bool affine, int64_t id_c, bool received) {
    c->t_fin = now_ms();
    g_alloc_ms = 0;
    c->tm.engine = KB_ENG_BINNED;
    REC(0);
    HIPCHK(c->totals.ensure(KB_TOTALS));
    c->tm.scan_insert_launches = 0;
    c->tm.tail_reruns = 0;
    FinPlan pl{};
    pl.prune = prune;
    pl.affine = affine;
    pl.id_c = id_c;
    pl.received = received;
    int rc = fin_records(c, pl);
    if (rc) return rc;
    REC(2);
    rc = fin_plan(c, pl);
    if (rc) return rc;
    rc = fin_order(c, pl);
    if (rc) return rc;
    REC(3);
    // ---- one workgroup per bin.  Entry capacity: learned (or N/8), rerun once
    // with the exact need when the packed counter says it was exceeded.
    HIPCHK(c->ids_out.ensure(std::max<uint64_t>(pl.N, 1)));
    uint64_t ecap = std::min<uint64_t>(pl.N + 1, c->ecap_hint ? c->ecap_hint : pl.N / 8 + 1024);
    if (const int forced = env_int("KB_BIN_ECAP0", 0)) ecap = (uint64_t)forced;  // tests: force the rerun
    BinArgs a{};
    FinRead rb{};
    for (int attempt = 0;; attempt++) {
        rc = fin_entries(c, pl, ecap, attempt);
        if (rc) return rc;
        rc = fill_bin_args(c, pl, ecap, attempt, a);
        if (rc) return rc;
        // The tail kernels -- the heavy bins' list builds and partitions, the
        // list kernels -- have work only when bin_kernel publishes a heavy bin
        // or queues a list, and cost ~4.5 us per empty launch (8 of them: 2 %
        // of a C2 step).  Where the last finalize needed none they are left
        // out, and launched after all (full grids) only if this finalize's
        // totals say bin_kernel published or queued something
        const bool defer = attempt == 0 && c->hint_heavy == 0 && c->hint_lq == 0 && a.lq_items &&
                           env_int("KB_BIN_DEFER_TAIL", 1) != 0;
        HIPCHK(c->bargs.ensure_exact(1));
        HIPCHK(launch_bins(a, pl.max_bins, pl.KW, c->s, c->timing ? &c->ev[6] : nullptr, !defer, c->bargs.p));
#ifdef KB_BIN_PROF
        bins_prof_report(c->s);
#endif
        // (deferred tail: nothing runs after bins_final, so it gathers the
        // finalize's stats next to the totals for one copy instead of three)
        HIPCHK(launch_bins_final(a.gcount, c->e_off.p, c->totals.p, a.max_entries, pl.flat_l ? c->flat_n.p : nullptr,
                                 a.lq_n, defer ? c->pstat.p : nullptr, defer ? c->misc.p : nullptr, c->s));
        REC(4);
        ListArgs la{};
        rc = fill_list_args(c, pl, a, attempt, la);
        if (rc) return rc;
        if (!defer) HIPCHK(launch_lists(la, c->n_occ_entries_hint ? c->n_occ_entries_hint : ecap, c->s));
#ifdef KB_BIN_PROF
        lists_prof_report(c->s);
#endif
        REC(5);
        rc = fin_readback(c, pl, defer, true, rb);
        if (rc) return rc;
        if (defer && (rb.heavy || rb.queued)) {
            // the tail after all (a heavy bin published, or lists queued):
            // full grids, then the totals again
            c->tm.tail_reruns++;
            a.heavy_hint = ~0ull;
            HIPCHK(launch_bins_heavy(a, pl.KW, c->s, c->bargs.p));
            HIPCHK(launch_bins_final(a.gcount, c->e_off.p, c->totals.p, a.max_entries,
                                     pl.flat_l ? c->flat_n.p : nullptr, a.lq_n, nullptr, nullptr, c->s));
            la.lq_hint = ~0ull;
            la.long_hint[0] = la.long_hint[1] = ~0ull;
            HIPCHK(launch_lists(la, c->n_occ_entries_hint ? c->n_occ_entries_hint : ecap, c->s));
            REC(5);
            rc = fin_readback(c, pl, false, false, rb);
            if (rc) return rc;
        }
        if (rb.rec_status & ST_BUCKET_FULL) return fin_bucket_full(c, pl);
        const uint64_t need = rb.asked + 1;  // entries asked of the packed counter
        if ((rb.bin_status & ST_TABLE_FULL) && attempt == 0 && need > ecap) {
            ecap = need + need / 16 + 1024;
            continue;
        }
        break;
    }
    c->hint_heavy = rb.heavy;
    c->hint_lq = rb.queued;
    c->hint_long[0] = rb.long_n[0];
    c->hint_long[1] = rb.long_n[1];
    c->hint_entries = rb.entries;
    c->hint_ids = rb.ids;
    rc = fin_check(c, pl, rb);
    if (rc) return rc;
    return fin_publish(c, pl, rb, a.pf != 0);
}

// kbin_api.hip -- host side of the C-ABI declared in include/kbin.h: a
// context's lifecycle, submit, timing, kb_finalize (the dispatch and the table
// engine), digest, export and the read generator.  Routing is in
// kbin_route.hip, the bucket maps in kbin_bmap.hip, the binned engine's
// finalize in kbin_finalize.hip; kbin_host.h is their shared header.
//
// Owns device memory and the HIP stream of a context, plans the table size,
// and sequences the kernels of kbin_kernels.hip:
//   submit   : H2D (pinned staging) + pack, or adopt device-packed reads;
//              per-read k-mer offsets (device scan)
//   finalize : zero table -> scan_insert per batch (records) -> [retry
//              bigger on overflow] -> radix sort by slot -> runs/prune/CSR ->
//              emit read ids
//   export   : D2H of the CSR
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>

#include "kbin_host.h"

thread_local std::string kb::g_err;
thread_local double kb::g_alloc_ms = 0;

int kb::fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int kb::set_device(kb_ctx* c) {
    HIPCHK(hipSetDevice(c->dev));
    return KB_OK;
}

extern "C" int kb_abi_version(void) { return 3; }  // 2: kb_timing path counters; 3: ranked-bin counters, kb_group_*

extern "C" const char* kb_last_error(void) { return g_err.c_str(); }
// (kbin_group.hip: a group call's failure is this thread's last error too)
void kb::set_last_error(const char* msg) { g_err = msg; }

extern "C" void* kb_stream(kb_ctx* ctx) { return ctx ? (void*)ctx->s : nullptr; }

extern "C" int kb_create(const kb_params* params, kb_ctx** out) {
    if (!params || !out) return fail(KB_EINVAL, "null argument");
    *out = nullptr;
    const kb_params& p = *params;
    if (p.M < 1 || p.M > 8)
        return fail(KB_EINVAL, "M=%d outside [1,8] (power_val, binning.c:17)", p.M);
    // (K < 2M: the reference's incremental branch, binning.c:992-1021, is
    // live -- the binned engine's record pass walks it, any read length; its
    // records are routable, the complement flag in bit 60 of their header
    // (ROUTED_REV_BIT); kb_finalize and the routing calls check the rest)
    if (p.K > 63) return fail(KB_EINVAL, "K=%d > 63 unsupported", p.K);
    // (a k-mer holds its signature mmer: K >= M, binning.c:931-936 reads M bases
    // of every k-mer; the incremental walk starts at K - M >= 0)
    if (p.K < 1 || p.K < p.M) return fail(KB_EINVAL, "K=%d outside [M=%d, 63]", p.K, p.M);
    if (p.cutoff < 0) return fail(KB_EINVAL, "cutoff < 0");
    if (p.max_read_len < 1 || p.max_read_len > 65535)
        return fail(KB_EINVAL, "max_read_len=%d outside [1,65535]", p.max_read_len);
    if (p.flags & ~(KB_TRACK_FIRST | KB_ENGINE_TABLE | KB_ENGINE_BINNED)) return fail(KB_EINVAL, "unknown flags 0x%x", p.flags);
    if (p.table_slots && (p.table_slots & (p.table_slots - 1)))
        return fail(KB_EINVAL, "table_slots must be a power of two");
    kb_ctx* c = new kb_ctx();
    c->p = p;
    c->KW = p.K <= 31 ? 1 : 2;
    c->dev = p.device;
    int rc = set_device(c);
    if (rc) { delete c; return rc; }
    hipError_t e = hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(KB_EDEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
    for (auto& ev : c->ev) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) { kb_destroy(c); return fail(KB_EDEVICE, "hipEventCreate"); }
    }
    e = hipHostMalloc((void**)&c->h_misc, KB_MISC * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) { kb_destroy(c); return fail(KB_ENOMEM, "hipHostMalloc"); }
    e = hipHostMalloc((void**)&c->h_totals, KB_TOTALS * sizeof(uint64_t), hipHostMallocDefault);
    if (e != hipSuccess) { kb_destroy(c); return fail(KB_ENOMEM, "hipHostMalloc"); }
    e = hipHostMalloc((void**)&c->h_alpha, 2 * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) { kb_destroy(c); return fail(KB_ENOMEM, "hipHostMalloc"); }
    c->h_alpha[0] = c->h_alpha[1] = 0;
    for (auto& sl : c->ring) {
        e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
        if (e != hipSuccess) { kb_destroy(c); return fail(KB_EDEVICE, "hipEventCreate"); }
    }
    e = hipEventCreateWithFlags(&c->map_done, hipEventDisableTiming);
    if (e != hipSuccess) { kb_destroy(c); return fail(KB_EDEVICE, "hipEventCreate"); }
    e = hipEventCreateWithFlags(&c->ev_mid, hipEventDisableTiming);
    if (e != hipSuccess) { kb_destroy(c); return fail(KB_EDEVICE, "hipEventCreate"); }
    {
        {
            const uint32_t hm = 1u << (2 * p.M - 1);
            c->prior_p.resize(hm);
            for (uint32_t i = 0; i < hm; i++) c->prior_p[i] = std::pow((double)(i + 1) / hm, p.K - p.M);
        }
        // the bucket maps' pinned staging (map upload, bin descriptors back):
        // page-locking takes milliseconds, so here rather than inside a finalize
        const uint64_t half = 1ull << (2 * p.M - 1), bins = bin_budget(c, 1024);
        if (c->map_stage.ensure(half * sizeof(uint32_t) + bins * sizeof(uint16_t)) != hipSuccess ||
            c->h_bins.ensure(3 * bins) != hipSuccess) {
            kb_destroy(c);
            return fail(KB_ENOMEM, "hipHostMalloc");
        }
        // The runtime sets up its host-to-device copy path for copies of this
        // size on first use (milliseconds, once per process and device): a
        // map-sized warm-up copy here keeps it out of the first finalize; so
        // does resolving the kernels (load_bin_kernels)
        static std::atomic<bool> warm[64] = {};  // (contexts of several devices may be created concurrently)
        if (p.device >= 0 && p.device < 64 && !warm[p.device].load(std::memory_order_acquire)) {
            DevBuf<uint8_t> t;
            const uint64_t nb = half * sizeof(uint32_t);
            if (t.ensure_exact(nb) == hipSuccess &&
                hipMemcpyAsync(t.p, c->map_stage.p, nb, hipMemcpyHostToDevice, c->s) == hipSuccess &&
                hipStreamSynchronize(c->s) == hipSuccess &&
                (getenv("KB_PRELOAD") && atoi(getenv("KB_PRELOAD")) == 0 ? true : load_bin_kernels() == hipSuccess))
                warm[p.device].store(true, std::memory_order_release);
            t.release();
        }
    }
    // (the zeroing goes up as a host-to-device copy: the context's first such
    // copy sets up the copy path, here rather than inside a first finalize)
    memset(c->h_totals, 0, KB_TOTALS * sizeof(uint64_t));
    if (c->misc.ensure_exact(KB_MISC) != hipSuccess || c->totals.ensure_exact(KB_TOTALS) != hipSuccess ||
        hipMemsetAsync(c->misc.p, 0, KB_MISC * sizeof(uint32_t), c->s) != hipSuccess ||
        hipMemcpyAsync(c->totals.p, c->h_totals, KB_TOTALS * sizeof(uint64_t), hipMemcpyHostToDevice, c->s) !=
            hipSuccess ||
        hipStreamSynchronize(c->s) != hipSuccess) {
        kb_destroy(c);
        return fail(KB_ENOMEM, "device alloc");
    }
    *out = c;
    return KB_OK;
}

// (a batch's words, lengths, ids and k-mer offsets live in c->pool: rewound here)
static void free_batches(kb_ctx* c) {
    for (auto& b : c->batches) {
        if (b.rec_base) (void)hipFree(b.rec_base);
        if (b.route_offs) (void)hipFree(b.route_offs);
    }
    c->pool.reset();
    c->route_G = 0;
    c->batches.clear();
    c->n_reads = 0;
    c->n_occ = 0;
}

extern "C" void kb_destroy(kb_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->dev);
    if (c->s) (void)hipStreamSynchronize(c->s);
    free_batches(c);
    for (auto& sl : c->ring) {
        sl.h.release();
        sl.d.release();
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    c->pool.release();
    c->h_mmer.release(); c->h_cnt.release(); c->h_hi.release(); c->h_lo.release(); c->h_off.release();
    c->h_first.release(); c->h_ids.release(); c->h_bins.release(); c->map_stage.release();
    if (c->map_done) (void)hipEventDestroy(c->map_done);
    if (c->ev_mid) (void)hipEventDestroy(c->ev_mid);
    if (c->h_alpha) (void)hipHostFree(c->h_alpha);
    c->table.release(); c->occ_a.release();
    c->seg.release(); c->pay.release(); c->srec.release(); c->stage.release(); c->stage_ord.release(); c->stage_slot.release(); c->kstage.release(); c->rrank.release(); c->rord.release(); c->bargs.release(); c->long_q.release(); c->border.release(); c->bdesc.release(); c->bcount.release(); c->bmmer.release(); c->bocc.release();
    c->regions.release(); c->bfill.release(); c->bbase.release(); c->rbase.release(); c->kpart.release(); c->rcount.release();
    c->occ_b.release(); c->os_flags.release(); c->os_aux.release(); c->read_ids.release(); c->starts.release();
    c->e_mmer.release(); c->e_cnt.release(); c->e_hi.release(); c->e_hi_zeroed = nullptr;
    c->e_lo.release(); c->e_off.release(); c->ids_out.release(); c->scratch.release();
    c->misc.release(); c->totals.release(); c->first.release(); c->e_first.release();
    for (auto& m : c->bmaps) { m.map.release(); m.sub.release(); }
    for (auto& o : c->owners) o.second.second.release();
    c->flat_list.release(); c->flat_next.release(); c->flat_l0.release(); c->flat_off.release();
    c->flat_cur.release(); c->flat_chunk.release(); c->pool_bin.release(); c->chunk_bin.release();
    c->flat_sbase.release(); c->flat_obase.release(); c->flat_n.release(); c->hll.release();
    if (c->h_totals) (void)hipHostFree(c->h_totals);
    if (c->h_misc) (void)hipHostFree(c->h_misc);
    for (auto& ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->s) (void)hipStreamDestroy(c->s);
    delete c;
}

extern "C" int kb_reset(kb_ctx* c) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->s));
    free_batches(c);
    c->finalized = false;
    c->exported = false;
    c->bucket_failed = false;  // a new input gets the bucketed path again
    c->alpha_bad = false;
    c->ingest_unchecked = false;
    c->h_alpha[0] = c->h_alpha[1] = 0;
    for (auto& sl : c->ring) sl.used = false;
    if (c->alpha_dirty) {  // (only a pack kernel sets the sticky status word)
        HIPCHK(hipMemsetAsync(c->misc.p + M_ALPHABET, 0, sizeof(uint32_t), c->s));
        c->alpha_dirty = false;
    }
    c->n_entries = c->n_ids = c->n_distinct = 0;
    c->part = 0;  // back to one full pass
    c->part_n = 1;
    return KB_OK;
}

// Partitioned passes: the next finalize (or route) covers only the mmers of
// one partition.  Received records and the result are dropped; read batches
// are kept and re-armed (a shipped batch can be routed again for this pass).
extern "C" int kb_set_partition(kb_ctx* c, uint32_t part, uint32_t n_parts) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (n_parts == 0 || part >= n_parts) return fail(KB_EINVAL, "partition %u of %u", part, n_parts);
    if (n_parts > 1 && !binned_applies(c))
        return fail(KB_EINVAL, "partitioned passes need the binned engine (K <= 63, reads <= 512 bp)");
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->s));
    std::vector<Batch> keep;
    for (auto& b : c->batches) {
        if (b.superkmers) {
            if (b.rec_base) (void)hipFree(b.rec_base);
            continue;
        }
        b.routed = false;
        keep.push_back(b);
    }
    c->batches.swap(keep);
    c->route_G = 0;
    c->part = part;
    c->part_n = n_parts;
    c->finalized = false;
    c->exported = false;
    c->n_entries = c->n_ids = c->n_distinct = 0;
    return KB_OK;
}

// k-mer offsets of a batch (device scan) and its occurrence total (host sync)
static int batch_offsets(kb_ctx* c, Batch& b) {
    HIPCHK(c->pool.alloc(b.n_reads + 1, &b.kmer_base));
    const uint64_t need = kmer_base_scratch_elems(b.n_reads);
    HIPCHK(c->scratch.ensure(std::max<uint64_t>(need, c->scratch.cap)));
    HIPCHK(launch_kmer_base(b.lens, b.n_reads, c->p.K, b.kmer_base, c->scratch.p, c->scratch.cap, c->s));
    uint64_t tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, b.kmer_base + b.n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    b.n_occ = tot;
    b.have_occ = true;
    return KB_OK;
}

// the ids array of an affine batch, materialised only where a path needs it
int kb::batch_ids(kb_ctx* c, Batch& b) {
    if (b.ids || b.superkmers) return KB_OK;
    HIPCHK(c->pool.alloc(b.n_reads, &b.ids));
    HIPCHK(launch_fill_ids(b.ids, b.n_reads, (int32_t)b.first_id, c->s));
    return KB_OK;
}

// The alphabet status of the host batches packed so far: the slot snapshot
// taken after each pack (no wait) or, with sync, the device word itself.
int kb::ingest_check(kb_ctx* c, bool sync) {
    if (!c->alpha_bad && c->ingest_unchecked && sync) {
        HIPCHK(hipMemcpyAsync(c->h_alpha, c->misc.p + M_ALPHABET, sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipStreamSynchronize(c->s));
        c->ingest_unchecked = false;
        if (c->h_alpha[0] & ST_ALPHABET) c->alpha_bad = true;
    }
    if (c->alpha_bad)
        return fail(KB_EALPHABET, "read byte outside {A,C,G,T} in a submitted batch (see DESIGN.md: alphabet)");
    return KB_OK;
}

// binning.c:1150-1166 feeds process_read one fgets line at a time; here the
// host hands over batches.  A batch is copied into a pinned staging slot (the
// caller may reuse its buffer on return, as binning.c:1154 does), sent H2D and
// packed to 2-bit words on the context's stream, and kb_submit returns
// without waiting: the next submit fills the other slot meanwhile.  The
// alphabet check rides along (the pack kernel's sticky status word, read back
// two submits later or by kb_finalize).
static int submit_common(kb_ctx* c, const char* bases, const uint32_t* lens, uint64_t n_reads,
                         const int32_t* ids, int32_t first_id) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (c->finalized) return fail(KB_ESTATE, "submit after finalize (call kb_reset)");
    if (n_reads == 0) return KB_OK;
    if (!bases || !lens) return fail(KB_EINVAL, "null bases/lens");
    if (c->n_reads + n_reads > 0xFFFFFFFFull)
        return fail(KB_EOVERFLOW, "more than 2^32 reads per context");
    int rc = set_device(c);
    if (rc) return rc;
    uint32_t maxlen = 0;
    uint64_t nb = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (lens[r] > (uint32_t)c->p.max_read_len)
            return fail(KB_ETOOLONG, "read %llu has %u bases > max_read_len %d",
                        (unsigned long long)r, lens[r], c->p.max_read_len);
        maxlen = std::max(maxlen, lens[r]);
        nb += lens[r];
    }
    const int RW = (int)((std::max<uint32_t>(maxlen, 1) + 31) / 32);
    // slot layout: bases | offsets (u64, 8-B aligned) | ids
    const uint64_t o_off = (nb + 7) & ~7ull;
    const uint64_t o_ids = o_off + (n_reads + 1) * sizeof(uint64_t);
    const uint64_t bytes = o_ids + (ids ? n_reads * sizeof(int32_t) : 0);
    const int si = c->ring_next;
    IngestSlot& sl = c->ring[si];
    if (sl.used) {  // its last H2D + pack (two submits ago) must be done
        HIPCHK(hipEventSynchronize(sl.done));
        if (c->h_alpha[si] & ST_ALPHABET) c->alpha_bad = true;
    }
    rc = ingest_check(c, false);
    if (rc) return rc;
    HIPCHK(sl.h.ensure(bytes));
    HIPCHK(sl.d.ensure(bytes));
    memcpy(sl.h.p, bases, nb);
    uint64_t* hoff = reinterpret_cast<uint64_t*>(sl.h.p + o_off);
    hoff[0] = 0;
    for (uint64_t r = 0; r < n_reads; r++) hoff[r + 1] = hoff[r] + lens[r];
    if (ids) memcpy(sl.h.p + o_ids, ids, n_reads * sizeof(int32_t));
    HIPCHK(hipMemcpyAsync(sl.d.p, sl.h.p, bytes, hipMemcpyHostToDevice, c->s));
    Batch b;
    b.n_reads = n_reads;
    b.RW = RW;
    b.ord_base = c->n_reads;
    HIPCHK(c->pool.alloc(n_reads * (uint64_t)RW, &b.own_words));
    HIPCHK(c->pool.alloc(n_reads, &b.own_lens));
    b.words = b.own_words;
    b.lens = b.own_lens;
    c->alpha_dirty = true;
    HIPCHK(launch_pack(sl.d.p, reinterpret_cast<const uint64_t*>(sl.d.p + o_off),
                       n_reads, RW, b.own_words, b.own_lens, c->misc.p + M_ALPHABET, c->s));
    if (ids) {
        HIPCHK(c->pool.alloc(n_reads, &b.ids));
        HIPCHK(hipMemcpyAsync(b.ids, sl.d.p + o_ids, n_reads * sizeof(int32_t), hipMemcpyDeviceToDevice, c->s));
    } else {
        b.affine = true;
        b.first_id = first_id;
    }
    HIPCHK(hipMemcpyAsync(c->h_alpha + si, c->misc.p + M_ALPHABET, sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipEventRecord(sl.done, c->s));
    sl.used = true;
    c->ring_next ^= 1;
    c->ingest_unchecked = true;
    c->n_reads += n_reads;
    c->batches.push_back(b);
    return KB_OK;
}

extern "C" int kb_submit(kb_ctx* c, const char* bases, const uint32_t* lens, uint64_t n_reads,
                         int32_t first_id) {
    return submit_common(c, bases, lens, n_reads, nullptr, first_id);
}

extern "C" int kb_submit_ids(kb_ctx* c, const char* bases, const uint32_t* lens, uint64_t n_reads,
                             const int32_t* ids) {
    if (n_reads && !ids) return fail(KB_EINVAL, "null ids");
    return submit_common(c, bases, lens, n_reads, ids, 0);
}

extern "C" int kb_submit_packed_device(kb_ctx* c, const uint64_t* d_words, const uint32_t* d_lens,
                                       uint64_t n_reads, uint32_t wpr, int32_t first_id) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (c->finalized) return fail(KB_ESTATE, "submit after finalize (call kb_reset)");
    if (n_reads == 0) return KB_OK;
    if (!d_words || !d_lens) return fail(KB_EINVAL, "null device pointers");
    if ((uint64_t)wpr * 32 < 1 || wpr > 2048) return fail(KB_EINVAL, "words_per_read=%u", wpr);
    if ((uint64_t)wpr * 32 > (uint64_t)c->p.max_read_len + 31)
        return fail(KB_ETOOLONG, "words_per_read=%u exceeds max_read_len %d", wpr, c->p.max_read_len);
    if (c->n_reads + n_reads > 0xFFFFFFFFull)
        return fail(KB_EOVERFLOW, "more than 2^32 reads per context");
    int rc = set_device(c);
    if (rc) return rc;
    Batch b;
    b.words = d_words;
    b.lens = d_lens;
    b.n_reads = n_reads;
    b.RW = (int)wpr;
    b.ord_base = c->n_reads;
    b.affine = true;
    b.first_id = first_id;
    c->n_reads += n_reads;
    c->batches.push_back(b);
    return KB_OK;
}

static uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

extern "C" int kb_set_timing(kb_ctx* c, int enable) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (enable < 0 || enable > KB_TIMING_KERNEL) return fail(KB_EINVAL, "timing mode %d", enable);
    c->timing = enable;
    return KB_OK;
}

extern "C" int kb_get_timing(kb_ctx* c, kb_timing* out) {
    if (!c || !out) return fail(KB_EINVAL, "null argument");
    *out = c->tm;
    return KB_OK;
}

// ordinal -> read id over the unrouted read batches: one affine map (id =
// ordinal + id_c) when every batch has affine ids that agree, else read_ids
int kb::read_id_map(kb_ctx* c, bool& affine, int64_t& id_c) {
    affine = true;
    id_c = 0;
    bool first_b = true;
    for (auto& b : c->batches) {
        if (b.routed || b.superkmers) continue;
        const int64_t cb = b.first_id - (int64_t)b.ord_base;
        if (!b.affine || (!first_b && cb != id_c)) affine = false;
        id_c = cb;
        first_b = false;
    }
    if (affine) return KB_OK;
    HIPCHK(c->read_ids.ensure(std::max<uint64_t>(c->n_reads, 1)));
    for (auto& b : c->batches) {
        if (b.routed || b.superkmers || !b.n_reads) continue;
        if (b.ids)
            HIPCHK(hipMemcpyAsync(c->read_ids.p + b.ord_base, b.ids, b.n_reads * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, c->s));
        else
            HIPCHK(launch_fill_ids(c->read_ids.p + b.ord_base, b.n_reads, (int32_t)b.first_id, c->s));
    }
    return KB_OK;
}

// the table engine's per-record occurrence offsets of a received batch
static int sk_batch_offsets(kb_ctx* c, Batch& b) {
    HIPCHK(hipMalloc((void**)&b.rec_base, std::max<uint64_t>(b.n_reads, 1) * sizeof(uint32_t)));
    HIPCHK(launch_sk_counts(b.recs, b.n_reads, rec_words(c), b.rec_base, c->s));
    HIPCHK(c->scratch.ensure(std::max(scan_u32_scratch_elems(b.n_reads), c->scratch.cap)));
    HIPCHK(launch_scan_u32(b.rec_base, b.n_reads, c->scratch.p, c->scratch.cap, c->s));
    uint64_t tot = 0;
    const uint64_t nb = scan_u32_scratch_elems(b.n_reads) - 2;
    HIPCHK(hipMemcpyAsync(&tot, c->scratch.p + nb, 8, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    b.n_occ = tot;
    b.have_occ = true;
    return KB_OK;
}

static int log2u(uint64_t x) {
    int b = 0;
    while ((1ull << b) < x) b++;
    return b;
}

extern "C" int kb_finalize(kb_ctx* c, int prune) {
    if (!c) return fail(KB_EINVAL, "null ctx");
    if (c->finalized) return fail(KB_ESTATE, "already finalized (call kb_reset)");
    int rc = set_device(c);
    if (rc) return rc;
    rc = ingest_check(c, true);  // every host batch packed so far was ACGT
    if (rc) return rc;
    // active batches: unrouted reads, or received super-k-mers (not both)
    bool any_reads = false, any_sk = false;
    for (auto& b : c->batches) {
        if (b.routed) continue;
        (b.superkmers ? any_sk : any_reads) = true;
    }
    if (any_reads && any_sk)
        return fail(KB_ESTATE, "a context bins either its own reads or received super-k-mers");
    // (K < 2M: the record pass walks the reference's live incremental branch,
    // one lane per read -- the thread-per-read kernel, or one lane of a wave
    // per longer read -- in the binned engine)
    if (c->p.K < 2 * c->p.M && !binned_applies(c))
        return fail(KB_EINVAL, "K=%d < 2M=%d needs the binned engine", c->p.K, 2 * c->p.M);
    memset(&c->tm, 0, sizeof(c->tm));
    const int SW = c->KW == 1 ? 2 : 4;
    const bool track_first = (c->p.flags & KB_TRACK_FIRST) != 0;
    bool affine = false;
    int64_t id_c = 0;
    if (any_sk) {
        affine = false;
    } else {
        rc = read_id_map(c, affine, id_c);
        if (rc) return rc;
    }
    if (binned_applies(c)) {
        if (any_sk) return finalize_binned(c, prune, true, 0, true);  // ordinal = read id
        return finalize_binned(c, prune, affine, id_c, false);
    }
    if (c->part_n > 1) return fail(KB_EINVAL, "partitioned passes need the binned engine (K <= 63, reads <= 512 bp)");
    c->tm.engine = KB_ENG_TABLE;
    // per-read occurrence offsets (the table engine's record slots)
    uint64_t N = 0;
    for (auto& b : c->batches) {
        if (b.routed) continue;
        if (!b.have_occ) {
            rc = b.superkmers ? sk_batch_offsets(c, b) : batch_offsets(c, b);
            if (rc) return rc;
        }
        b.occ_base = N;
        N += b.n_occ;
    }
    c->n_occ = N;
    if (N >= 0xFFFFFFFFull)
        return fail(KB_EOVERFLOW, "%llu k-mer occurrences in one context (limit 2^32-1)",
                    (unsigned long long)N);
    // ---- table plan: ~0.6 load for the expected distinct keys
    uint64_t slots = c->p.table_slots;
    if (!slots) slots = c->learned_slots;
    if (!slots) slots = next_pow2(std::max<uint64_t>(4096, N / 6));
    slots = std::max<uint64_t>(slots, 1024);
    HIPCHK(c->occ_a.ensure(N));
    HIPCHK(c->occ_b.ensure(N));
    HIPCHK(c->ids_out.ensure(N));
    uint32_t status = 0, ndist = 0;
    for (int attempt = 0;; attempt++) {
        if (slots > (1ull << 32) - 1)
            return fail(KB_ENOMEM, "table would need 2^32 slots or more");
        hipError_t e = c->table.ensure(slots * SW);
        if (e != hipSuccess)
            return fail(KB_ENOMEM, "table of %llu slots: %s", (unsigned long long)slots,
                        hipGetErrorString(e));
        c->slots = slots;
        REC(0);
        HIPCHK(hipMemsetAsync(c->table.p, 0, slots * SW * sizeof(uint64_t), c->s));
        HIPCHK(hipMemsetAsync(c->misc.p, 0, (M_DISTINCT + 1) * sizeof(uint32_t), c->s));
        if (track_first) {
            HIPCHK(c->first.ensure(slots));
            HIPCHK(hipMemsetAsync(c->first.p, 0xFF, slots * sizeof(uint64_t), c->s));
        }
        REC(1);
        c->tm.scan_insert_launches = 0;
        for (auto& b : c->batches) {
            if (b.routed) continue;
            if (b.superkmers) {
                SkArgs a{};
                a.recs = b.recs;
                a.rec_base = b.rec_base;
                a.n_rec = b.n_reads;
                a.rec_words = rec_words(c);
                a.table = c->table.p;
                a.mask = slots - 1;
                a.occ = c->occ_a.p;
                a.occ_base = b.occ_base;
                a.n_occ_total = N;
                a.first = track_first ? c->first.p : nullptr;
                a.n_distinct = c->misc.p + M_DISTINCT;
                a.status = c->misc.p + M_REC_STATUS;
                a.max_distinct = (uint32_t)std::min<uint64_t>(slots - slots / 8, 0xFFFFFFFFull);
                a.max_probe = (uint32_t)std::min<uint64_t>(slots, 1u << 14);  // past it: rerun bigger
                a.K = c->p.K;
                a.M = c->p.M;
                HIPCHK(launch_insert_sk(a, c->KW, c->s));
                c->tm.scan_insert_launches++;
                continue;
            }
            ScanArgs a{};
            a.words = b.words;
            a.lens = b.lens;
            a.kmer_base = b.kmer_base;
            a.n_reads = b.n_reads;
            a.table = c->table.p;
            a.mask = slots - 1;
            a.occ = c->occ_a.p;
            a.occ_base = b.occ_base;
            a.n_occ_total = N;
            a.ord_base = (uint32_t)b.ord_base;
            a.first = track_first ? c->first.p : nullptr;
            a.n_distinct = c->misc.p + M_DISTINCT;
            a.status = c->misc.p + M_REC_STATUS;
            a.max_distinct = (uint32_t)std::min<uint64_t>(slots - slots / 8, 0xFFFFFFFFull);
            a.max_probe = (uint32_t)std::min<uint64_t>(slots, 1u << 14);  // past it: rerun bigger
            a.RW = b.RW;
            a.K = c->p.K;
            a.M = c->p.M;
            HIPCHK(launch_scan_insert(a, c->KW, c->s));
            c->tm.scan_insert_launches++;
        }
        REC(2);
        HIPCHK(hipMemcpyAsync(c->h_misc, c->misc.p, (M_DISTINCT + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipStreamSynchronize(c->s));
        status = c->h_misc[M_REC_STATUS];
        ndist = c->h_misc[M_DISTINCT];
        if (!(status & (ST_TABLE_FULL | ST_PROBE_LIMIT))) break;
        if (attempt >= 6) return fail(KB_ENOMEM, "table retries exhausted (status %u)", status);
        slots *= 4;
    }
    c->n_distinct = ndist;
#ifdef KB_ABLATE_TABLE
    if (c->timing) HIPCHK(hipEventElapsedTime(&c->tm.scan_insert_ms, c->ev[1], c->ev[2]));
    c->n_entries = c->n_ids = 0;
    c->finalized = true;
    return KB_OK;
#endif
    // next finalize on this context: ~0.6 load for the distinct keys seen now
    if (!c->p.table_slots)
        c->learned_slots = std::max<uint64_t>(1024, next_pow2((uint64_t)ndist * 5 / 3 + 1));
    // ---- stable radix sort of the records by slot
    const int key_bits = log2u(slots);
    const uint64_t ne_cap = (uint64_t)ndist + 1;
    HIPCHK(c->scratch.ensure(std::max(runs_scratch_elems(N, ne_cap), c->scratch.cap)));
    const uint64_t nflags = onesweep_flag_elems(N);
    if (c->os_flags.cap < nflags || c->os_epoch > (1u << 24) - 8) {
        HIPCHK(c->os_flags.ensure(nflags));
        HIPCHK(hipMemsetAsync(c->os_flags.p, 0, c->os_flags.cap * sizeof(uint64_t), c->s));
        c->os_epoch = 0;
    }
    HIPCHK(c->os_aux.ensure(OS_AUX_WORDS));
    HIPCHK(launch_onesweep(c->occ_a.p, c->occ_b.p, N, key_bits, c->os_flags.p, c->os_aux.p,
                           &c->os_epoch, &c->sorted, c->s));
    c->tm.sort_passes = (uint32_t)((key_bits + 7) / 8);
    REC(3);
    // ---- runs -> counts -> prune -> CSR entries
    HIPCHK(c->starts.ensure(ne_cap + 1));
    HIPCHK(c->e_mmer.ensure(ne_cap));
    HIPCHK(c->e_cnt.ensure(ne_cap));
    HIPCHK(c->e_hi.ensure(ne_cap));
    c->e_hi_zeroed = nullptr;  // (the table engine writes it)
    HIPCHK(c->e_lo.ensure(ne_cap));
    HIPCHK(c->e_off.ensure(ne_cap));
    if (track_first) HIPCHK(c->e_first.ensure(ne_cap));
    const uint32_t keep_gt = prune ? (uint32_t)c->p.cutoff : 0u;
    // ids: affine fast path (id = ordinal + c for every batch) avoids the gather
    HIPCHK(launch_runs(c->sorted, N, c->table.p, c->KW, keep_gt, c->starts.p,
                       (any_sk || affine) ? nullptr : c->read_ids.p, (uint32_t)(affine ? id_c : 0),
                       c->ids_out.p, ne_cap, c->e_mmer.p, c->e_hi.p, c->e_lo.p, c->e_cnt.p,
                       c->e_off.p, track_first ? c->first.p : nullptr,
                       track_first ? c->e_first.p : nullptr, c->scratch.p, c->scratch.cap,
                       c->totals.p, c->s));
    REC(4);
    REC(5);
    HIPCHK(hipMemcpyAsync(c->h_totals, c->totals.p, (T_BIN_OVER + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
    if (N) HIPCHK(hipMemcpyAsync(c->h_misc + HM_RADIX_ERR, c->os_aux.p + OS_AUX_ERR, sizeof(uint32_t), hipMemcpyDeviceToHost, c->s));
    else c->h_misc[HM_RADIX_ERR] = 0;
    HIPCHK(hipStreamSynchronize(c->s));
    if (c->h_misc[HM_RADIX_ERR]) return fail(KB_EDEVICE, "radix look-back timed out (device error word %u)", c->h_misc[HM_RADIX_ERR]);
    if (c->h_totals[T_BIN_OVER])
        return fail(KB_EDEVICE, "internal: %llu runs > %llu distinct keys", (unsigned long long)c->h_totals[T_BIN_OVER],
                    (unsigned long long)ne_cap);
    // result invariants: kept entries <= distinct keys (runs) <= k-mers, ids <= k-mers
    if (c->h_totals[T_ENTRIES] > c->h_totals[T_BINS] || c->h_totals[T_BINS] > N || c->h_totals[T_IDS] > N)
        return fail(KB_EDEVICE, "internal: result invariant violated (%llu entries, %llu distinct, %llu ids, %llu k-mers)",
                    (unsigned long long)c->h_totals[T_ENTRIES], (unsigned long long)c->h_totals[T_BINS],
                    (unsigned long long)c->h_totals[T_IDS], (unsigned long long)N);
    c->n_entries = c->h_totals[T_ENTRIES];
    c->n_ids = c->h_totals[T_IDS];
    if (c->timing) {
        HIPCHK(hipEventElapsedTime(&c->tm.scan_insert_ms, c->ev[1], c->ev[2]));
        HIPCHK(hipEventElapsedTime(&c->tm.sort_ms, c->ev[2], c->ev[3]));
        HIPCHK(hipEventElapsedTime(&c->tm.runs_ms, c->ev[3], c->ev[4]));
        HIPCHK(hipEventElapsedTime(&c->tm.emit_ms, c->ev[4], c->ev[5]));
        HIPCHK(hipEventElapsedTime(&c->tm.total_ms, c->ev[0], c->ev[5]));
    }
    c->tm.table_slots = slots;
    c->finalized = true;
    c->exported = false;
    return KB_OK;
}

extern "C" int kb_digest(kb_ctx* c, uint64_t* out) {
    if (!c || !out) return fail(KB_EINVAL, "null argument");
    if (!c->finalized) return fail(KB_ESTATE, "digest before finalize");
    int rc = set_device(c);
    if (rc) return rc;
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c->totals.p + T_DIGEST);
    HIPCHK(launch_digest(c->e_mmer.p, c->e_hi.p, c->e_lo.p, c->e_cnt.p, c->e_off.p, c->ids_out.p, c->n_entries, d,
                         c->s));
    HIPCHK(hipMemcpyAsync(c->h_totals + T_DIGEST, d, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    out[0] = c->n_entries;
    out[1] = c->n_ids;
    out[2] = c->h_totals[T_DIGEST];
    out[3] = c->h_totals[T_DIGEST + 1];
    return KB_OK;
}

extern "C" int kb_export_device(kb_ctx* c, kb_csr* out) {
    if (!c || !out) return fail(KB_EINVAL, "null argument");
    if (!c->finalized) return fail(KB_ESTATE, "export before finalize");
    out->n_entries = c->n_entries;
    out->n_ids = c->n_ids;
    out->n_kmers = c->n_occ;
    out->n_distinct = c->n_distinct;
    out->mmer = c->e_mmer.p;
    out->kmer_hi = c->e_hi.p;
    out->kmer_lo = c->e_lo.p;
    out->count = c->e_cnt.p;
    out->offset = c->e_off.p;
    out->ids = c->ids_out.p;
    out->first = (c->p.flags & KB_TRACK_FIRST) ? c->e_first.p : nullptr;
    return KB_OK;
}

extern "C" int kb_export(kb_ctx* c, kb_csr* out) {
    if (!c || !out) return fail(KB_EINVAL, "null argument");
    if (!c->finalized) return fail(KB_ESTATE, "export before finalize");
    int rc = set_device(c);
    if (rc) return rc;
    if (!c->exported) {
        const uint64_t n = c->n_entries;
        const bool tf = (c->p.flags & KB_TRACK_FIRST) != 0;
        HIPCHK(c->h_mmer.ensure(n));
        HIPCHK(c->h_cnt.ensure(n));
        HIPCHK(c->h_hi.ensure(n));
        HIPCHK(c->h_lo.ensure(n));
        HIPCHK(c->h_off.ensure(n + 1));
        if (tf) HIPCHK(c->h_first.ensure(n));
        HIPCHK(c->h_ids.ensure(c->n_ids));
        if (n) {
            HIPCHK(hipMemcpyAsync(c->h_mmer.p, c->e_mmer.p, n * 4, hipMemcpyDeviceToHost, c->s));
            HIPCHK(hipMemcpyAsync(c->h_cnt.p, c->e_cnt.p, n * 4, hipMemcpyDeviceToHost, c->s));
            HIPCHK(hipMemcpyAsync(c->h_hi.p, c->e_hi.p, n * 8, hipMemcpyDeviceToHost, c->s));
            HIPCHK(hipMemcpyAsync(c->h_lo.p, c->e_lo.p, n * 8, hipMemcpyDeviceToHost, c->s));
            HIPCHK(hipMemcpyAsync(c->h_off.p, c->e_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, c->s));
            if (tf)
                HIPCHK(hipMemcpyAsync(c->h_first.p, c->e_first.p, n * 8, hipMemcpyDeviceToHost, c->s));
        } else {
            c->h_off.p[0] = 0;
        }
        if (c->n_ids)
            HIPCHK(hipMemcpyAsync(c->h_ids.p, c->ids_out.p, c->n_ids * 4, hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipStreamSynchronize(c->s));
        c->exported = true;
    }
    out->n_entries = c->n_entries;
    out->n_ids = c->n_ids;
    out->n_kmers = c->n_occ;
    out->n_distinct = c->n_distinct;
    out->mmer = c->h_mmer.p;
    out->kmer_hi = c->h_hi.p;
    out->kmer_lo = c->h_lo.p;
    out->count = c->h_cnt.p;
    out->offset = c->h_off.p;
    out->ids = c->h_ids.p;
    out->first = (c->p.flags & KB_TRACK_FIRST) ? c->h_first.p : nullptr;
    return KB_OK;
}

extern "C" int kb_generate_reads_device_at(int device, uint64_t* d_words, uint32_t* d_lens,
                                           uint64_t n_reads, uint32_t read_len, uint64_t genome_len,
                                           uint32_t err_ppm, uint64_t seed, uint64_t read_base) {
    if (!d_words || !d_lens) return fail(KB_EINVAL, "null device pointers");
    if (read_len < 1 || genome_len < read_len) return fail(KB_EINVAL, "bad read_len/genome_len");
    if (err_ppm > 1000000) return fail(KB_EINVAL, "err_per_million > 1e6");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_generate(d_words, d_lens, n_reads, read_len, genome_len, err_ppm, seed, read_base, 0));
    HIPCHK(hipStreamSynchronize(0));
    return KB_OK;
}

extern "C" int kb_generate_reads_device(int device, uint64_t* d_words, uint32_t* d_lens,
                                        uint64_t n_reads, uint32_t read_len, uint64_t genome_len,
                                        uint32_t err_ppm, uint64_t seed) {
    return kb_generate_reads_device_at(device, d_words, d_lens, n_reads, read_len, genome_len, err_ppm,
                                       seed, 0);
}

extern "C" int kb_unpack_reads_to_host(int device, const uint64_t* d_words, const uint32_t* d_lens,
                                       uint64_t n_reads, uint32_t wpr, char* h_bases,
                                       uint32_t* h_lens) {
    if (!d_words || !d_lens || !h_bases || !h_lens) return fail(KB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(device));
    if (!n_reads) return KB_OK;
    HIPCHK(hipMemcpy(h_lens, d_lens, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint64_t> off(n_reads + 1);
    off[0] = 0;
    for (uint64_t r = 0; r < n_reads; r++) off[r + 1] = off[r] + h_lens[r];
    uint64_t *d_off = nullptr;
    uint8_t* d_out = nullptr;
    HIPCHK(hipMalloc((void**)&d_off, (n_reads + 1) * 8));
    hipError_t e = hipMalloc((void**)&d_out, std::max<uint64_t>(off[n_reads], 1));
    if (e != hipSuccess) { (void)hipFree(d_off); return fail(KB_ENOMEM, "unpack alloc"); }
    e = hipMemcpy(d_off, off.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_unpack(d_words, d_lens, n_reads, (int)wpr, d_off, d_out, 0);
    if (e == hipSuccess) e = hipMemcpy(h_bases, d_out, off[n_reads], hipMemcpyDeviceToHost);
    (void)hipFree(d_off);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(KB_EDEVICE, "unpack: %s", hipGetErrorString(e));
    return KB_OK;
}

"""GPU parity: the HIP path (through the C-ABI, libkbin.so) against
  (1) the known-answer digests of the compiled reference (tests/golden), and
  (2) the CPU oracle (oracle/, clean-room restatement) on the same inputs,
bit-exact on every (mmer, kmer) key, count and read-id list."""
import hashlib
import os

import numpy as np
import pytest

import kbin
import oracle

# every case runs on both engines (conftest.engine)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("engine")]


def gpu_result(bases, lens, K, M, cutoff=1, prune=True, ids=None, batches=1, max_read_len=1024):
    with kbin.Engine(K, M, cutoff=cutoff, max_read_len=max_read_len) as eng:
        n = len(lens)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
        cuts = np.linspace(0, n, batches + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b <= a:
                continue
            sub = bases[off[a]:off[b]]
            if ids is None:
                eng.submit(bases=sub, lens=lens[a:b], first_id=int(a))
            else:
                eng.submit(bases=sub, lens=lens[a:b], ids=ids[a:b])
        eng.finalize(prune=prune)
        return eng.export()


def assert_csr(res):
    """CSR contract (kbin.h): offset[e + 1] ends entry e's list, lists tile ids"""
    off = np.asarray(res.offset, dtype=np.int64)
    assert off[0] == 0 and off[-1] == len(res.ids)
    np.testing.assert_array_equal(np.diff(off), np.asarray(res.count, dtype=np.int64))


def assert_same(res, ora):
    assert_csr(res)
    c = res.canonical()
    assert c.n_entries == ora.n_entries
    np.testing.assert_array_equal(c.mmer, ora.mmer)
    np.testing.assert_array_equal(c.kmer_hi, ora.kmer_hi)
    np.testing.assert_array_equal(c.kmer_lo, ora.kmer_lo)
    np.testing.assert_array_equal(c.count, ora.count)
    np.testing.assert_array_equal(c.offset, ora.offset)
    np.testing.assert_array_equal(c.ids, ora.ids)


def dump_sha(res, K, M):
    h = hashlib.sha256()
    for line in kbin.dump_lines(res, K, M):
        h.update(line.encode())
    return h.hexdigest()


def test_known_answer_digests(digests, golden_dir):
    for row in digests:
        bases, lens = oracle.read_fgets(golden_dir / row["input"], row["read_length"])
        res = gpu_result(bases, lens, row["K"], row["M"], row["cutoff"], row["prune"])
        assert res.n_entries == row["entries"], row
        assert int(res.count.sum()) == row["sum_count"], row
        assert len(set(res.mmer.tolist())) == row["mmers"], row
        assert dump_sha(res, row["K"], row["M"]) == row["sha256"], row


@pytest.mark.parametrize("K,M", [(31, 7), (6, 3), (21, 5), (32, 8), (33, 7), (63, 7), (40, 1), (2, 1)])
def test_random_vs_oracle(K, M):
    rng = np.random.default_rng(K * 100 + M)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3000)
    reads = []
    for _ in range(1500):
        L = int(rng.integers(0, 260))
        s = int(rng.integers(0, 3000 - L))
        r = genome[s:s + L].copy()
        m = rng.random(L) < 0.01
        r[m] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(m.sum()))
        reads.append(r.tobytes())
    bases, lens = kbin.pack_reads(reads)
    for prune in (False, True):
        ora = oracle.bin_reads(bases, lens, K, M, 1, prune)
        res = gpu_result(bases, lens, K, M, 1, prune, batches=3)
        assert res.n_kmers == ora.n_kmers
        assert_same(res, ora)


def test_result_invariant_fails_loudly(engine, monkeypatch):
    """a result whose pre-prune counts do not add up to the
    pass's k-mers (or entries > distinct > k-mers) is KB_EDEVICE, never KB_OK.
    KB_DIAG_CORRUPT=1 makes block 0 add one to a table count; the same input
    without it stays bit-exact."""
    rng = np.random.default_rng(11)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=4000)
    reads = [genome[s:s + 150].tobytes() for s in rng.integers(0, 3850, 2000)]
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, 31, 7, 1, True)
    assert_same(gpu_result(bases, lens, 31, 7), ora)
    if engine != "binned":
        pytest.skip("the corruption knob is the binned engine's")
    monkeypatch.setenv("KB_DIAG_CORRUPT", "1")
    with pytest.raises(kbin.KbError) as ei:
        gpu_result(bases, lens, 31, 7)
    assert ei.value.code == kbin.KB_EDEVICE and "invariant" in str(ei.value)


@pytest.mark.parametrize("knob", ["KB_BIN_LDSBAR", "KB_BIN_STAGE6", "KB_BIN_TS_ADAPT", "KB_BIN_DEFER_TAIL"])
@pytest.mark.parametrize("heavy", [False, True])
def test_default_knobs_off(knob, heavy, engine, monkeypatch):
    """the paths on by default (LDS-only barriers, the split 6-B
    stage, per-bin table sizes, the deferred tail) in their OTHER state stay
    bit-exact: a C2-like input, and one forced onto heavy bins (small tables,
    flat lists, the pre-filter)"""
    if engine != "binned":
        pytest.skip("binned engine knobs")
    rng = np.random.default_rng(5)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=20000)
    reads = []
    for s in rng.integers(0, 19850, 6000):
        r = genome[s:s + 150].copy()
        m = rng.random(150) < 0.002
        r[m] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(m.sum()))
        reads.append(r.tobytes())
    bases, lens = kbin.pack_reads(reads)
    monkeypatch.setenv(knob, "0")
    if heavy:
        monkeypatch.setenv("KB_BIN_TS_LOG2", "10")
        monkeypatch.setenv("KB_BIN_FLAT_L", "1")
        monkeypatch.setenv("KB_BIN_PF", "1")
    for prune in (True, False):
        ora = oracle.bin_reads(bases, lens, 31, 7, 1, prune)
        assert_same(gpu_result(bases, lens, 31, 7, 1, prune, batches=2), ora)


def test_binned_engine_selected(engine):
    """the engine the environment asks for is the one that runs (K <= 31)"""
    rng = np.random.default_rng(3)
    reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes() for _ in range(500)]
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, 31, 7, 1, True)
    with kbin.Engine(31, 7, cutoff=1, max_read_len=150) as eng:
        eng.set_timing(True)
        eng.submit(bases=bases, lens=lens, first_id=0)
        eng.finalize(prune=True)
        t = eng.timing()
        assert_same(eng.export(), ora)
    assert t["engine"] == (kbin.KB_ENG_BINNED if engine == "binned" else kbin.KB_ENG_TABLE)
    if engine == "binned":
        assert t["n_superkmers"] > 0 and t["n_bins"] > 0


def test_timing_modes(engine):
    """kb_set_timing: every phase (1), bin_kernel's two events only (2: the
    phase fields read 0 on the binned engine; the table engine keeps them), off
    (0); anything else is KB_EINVAL.  The result does not depend on it."""
    rng = np.random.default_rng(4)
    reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes() for _ in range(2000)]
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, 31, 7, 1, True)
    with kbin.Engine(31, 7, cutoff=1, max_read_len=150) as eng:
        with pytest.raises(kbin.KbError):
            kbin._check(eng.lib, eng.lib.kb_set_timing(eng._h, 3))
        for mode in (True, "kernel", False):
            eng.reset()
            eng.set_timing(mode)
            eng.submit(bases=bases, lens=lens, first_id=0)
            eng.finalize(prune=True)
            assert_same(eng.export(), ora)
            t = eng.timing()
            binned = t["engine"] == kbin.KB_ENG_BINNED
            if mode is True:
                assert t["total_ms"] > 0 and (t["bin_kernel_ms"] > 0 or not binned), t
            elif mode == "kernel":
                assert t["total_ms"] == 0 if binned else t["total_ms"] > 0, t
                if binned:
                    assert t["bin_kernel_ms"] > 0, t


@pytest.mark.parametrize("K,M", [(63, 7), (33, 7), (32, 8), (45, 1), (63, 1), (40, 6)])
def test_binned_two_word_kmers(K, M, engine, monkeypatch):
    """K > 31: the binned engine with two-word table keys (LDS claim word +
    published low word), 4-word super-k-mer spans and 64 length rows in the
    bucket ordering -- bit-exact against the oracle, with and without prune,
    first occurrences tracked; reads > 512 bp (or a forced radix path) hand
    two-word k-mers to the table engine"""
    rng = np.random.default_rng(K * 7 + M)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=4000)
    reads = []
    for _ in range(1200):
        L = int(rng.integers(K - 5, 300))
        s = int(rng.integers(0, 4000 - L))
        r = genome[s:s + L].copy()
        m = rng.random(L) < 0.01
        r[m] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(m.sum()))
        reads.append(r.tobytes())
    bases, lens = kbin.pack_reads(reads)
    for prune in (False, True):
        ora = oracle.bin_reads(bases, lens, K, M, 1, prune)
        with kbin.Engine(K, M, cutoff=1, max_read_len=300, flags=kbin.KB_TRACK_FIRST) as eng:
            eng.set_timing(True)
            eng.submit(bases=bases, lens=lens, first_id=0)
            eng.finalize(prune=prune)
            t = eng.timing()
            res = eng.export()
        assert t["engine"] == (kbin.KB_ENG_BINNED if engine == "binned" else kbin.KB_ENG_TABLE)
        assert_same(res, ora)
        last = res.ids[res.offset[1:].astype(np.int64) - 1]  # oldest id = first occurrence
        np.testing.assert_array_equal(res.first >> np.uint64(16), last.astype(np.uint64))
    if engine != "binned":
        return
    monkeypatch.setenv("KB_BIN_RADIX", "1")  # no radix path for two-word keys: table engine
    ora = oracle.bin_reads(bases, lens, K, M, 1, True)
    with kbin.Engine(K, M, cutoff=1, max_read_len=300) as eng:
        eng.set_timing(True)
        eng.submit(bases=bases, lens=lens, first_id=0)
        eng.finalize(prune=True)
        assert eng.timing()["engine"] == kbin.KB_ENG_TABLE
        assert_same(eng.export(), ora)


@pytest.mark.parametrize("K,M", [(31, 7), (6, 3), (21, 5), (2, 1)])
def test_binned_radix_path(K, M, engine, monkeypatch):
    """the binned engine's radix-sort record path (the fallback when a local
    bucket holds too many mmers, and the path for reads > 512 bp) matches the
    oracle as the default bucketed path does"""
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_RADIX", "1")
    rng = np.random.default_rng(K * 100 + M)
    reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(K, 300))).tobytes()
             for _ in range(400)]
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, K, M, 1, True)
    res = gpu_result(bases, lens, K, M, 1, True)
    assert_same(res, ora)


@pytest.mark.parametrize("prune", [False, True])
def test_binned_entry_capacity_rerun(prune, engine, monkeypatch):
    """the binned engine sizes its entry arrays from a learned estimate; when
    the estimate is too small the bin phase reruns at the exact need (forced
    here with a 64-entry first attempt)"""
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_ECAP0", "64")
    rng = np.random.default_rng(11)
    reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(31, 200))).tobytes()
             for _ in range(600)]
    reads += reads[:200]  # repeats survive the prune
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, 21, 6, 1, prune)
    assert len(ora.count) > 64
    res = gpu_result(bases, lens, 21, 6, 1, prune)
    assert_same(res, ora)


@pytest.mark.parametrize("P,radix,long_reads,K,M", [(1, False, False, 21, 5), (3, False, False, 21, 5),
                                                     (8, False, False, 21, 5), (4, True, False, 21, 5),
                                                     (3, False, True, 21, 5), (4, False, False, 63, 7)])
def test_partitioned_passes(P, radix, long_reads, K, M, engine, monkeypatch):
    """kb_set_partition: P passes over the same submitted reads bin disjoint
    mmer slices whose union is the single-pass result, list for list"""
    bases, lens = oracle.read_fgets(kbin.REPO_ROOT / "tests/golden/reads.txt", 101)
    rng = np.random.default_rng(P * 10 + radix)
    extra = [rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(0, 300))).tobytes()
             for _ in range(300)]
    if long_reads:  # > 512 bp: the wave-per-read scan and the radix record path
        extra += [rng.choice(np.frombuffer(b"ACGT", np.uint8), 700).tobytes() for _ in range(20)]
    off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    reads = [bases[off[i]:off[i + 1]] for i in range(3000)] + extra
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, K, M, 1, True)
    if radix:
        monkeypatch.setenv("KB_BIN_RADIX", "1")
    with kbin.Engine(K, M, cutoff=1, max_read_len=1024) as eng:
        eng.submit(bases=bases, lens=lens, first_id=0)
        if engine != "binned":
            with pytest.raises(kbin.KbError, match="KB_EINVAL"):
                eng.set_partition(0, 2)
            eng.set_partition(0, 1)
            return
        parts, dig = [], [0, 0, 0, 0]
        for p in range(P):
            eng.set_partition(p, P)
            eng.finalize(prune=True)
            parts.append(eng.export())
            d = eng.digest()
            assert d == kbin.result_digest(parts[-1])
            dig = [(a + b) % (1 << 64) for a, b in zip(dig, d)]
    seen = [set(np.unique(r.mmer).tolist()) for r in parts]
    for a in range(P):
        for b in range(a + 1, P):
            assert not seen[a] & seen[b], "a mmer in two partitions"
    if P > 1:
        assert sum(1 for r in parts if r.n_entries) > 1, "all keys in one partition"
    for r in parts:
        assert_csr(r)
    assert sum(r.n_kmers for r in parts) == ora.n_kmers
    assert_same(kbin.Result.concat(parts), ora)
    assert tuple(dig) == kbin.result_digest(ora)  # digests add over partitions


@pytest.mark.parametrize("K,M,sub,prior", [(21, 5, "4", "1"), (63, 7, "4", "1"), (21, 5, "0", "1"), (31, 7, "1", "1"),
                                           (31, 7, "4", "0"), (63, 7, "4", "0")])
def test_balanced_buckets(K, M, sub, prior, engine, monkeypatch):
    """after a pass the host packs the mmers into local buckets by their
    record counts (largest first, least-loaded bucket; an mmer above 1.5 x the
    mean load, or above one LDS table of keys, is split into context sub-bins,
    each an item of its own); later passes route records by that map, cutting
    a split mmer's records at the edge, per partition key -- every pass equals
    the oracle, and the split happened where allowed"""
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_BALANCE_MIN", "0")
    monkeypatch.setenv("KB_BIN_SUB", sub)
    monkeypatch.setenv("KB_BIN_PRIOR", prior)  # 0: a first pass without a map counts, then lays regions out exactly
    rng = np.random.default_rng(K)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=20000)
    reads = []
    for _ in range(3000):
        L = int(rng.integers(K, 260))
        s0 = int(rng.integers(0, 20000 - L))
        reads.append(genome[s0:s0 + L].tobytes())
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, K, M, 1, True)
    splits = []
    with kbin.Engine(K, M, cutoff=1, max_read_len=300) as eng:
        for P in (1, 3):
            for _ in range(3):  # the first pass of a key learns its map, the next ones use it
                parts = []
                for p in range(P):
                    eng.reset()
                    eng.submit(bases=bases, lens=lens, first_id=0)
                    eng.set_partition(p, P)
                    eng.finalize(prune=True)
                    parts.append(eng.export())
                    splits.append(eng.timing()["split_mmers"])
                assert_same(kbin.Result.concat(parts), ora)
        assert (max(splits) > 0) == (sub != "0"), splits


def test_explicit_ids_nonmonotone():
    """ids are caller-supplied (process_read's read_id): lists keep REVERSE CALL
    order, not id order (binning.c:1065-1068)."""
    rng = np.random.default_rng(7)
    reads = [b"ACGTACGTAC" * 5] * 20 + [rng.choice(np.frombuffer(b"ACGT", np.uint8), 60).tobytes() for _ in range(50)]
    bases, lens = kbin.pack_reads(reads)
    ids = rng.permutation(len(reads)).astype(np.int32) * 3 - 7
    ora = oracle.bin_reads(bases, lens, 11, 4, 1, True, ids=ids)
    res = gpu_result(bases, lens, 11, 4, 1, True, ids=ids, batches=2)
    assert_same(res, ora)


def test_large_lists():
    """a key seen > 4096 times takes the chunk-sort + merge path"""
    reads = [b"A" * 40] * 3000 + [b"ACGT" * 10] * 200
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, 9, 3, 1, True)
    res = gpu_result(bases, lens, 9, 3, 1, True)
    assert int(res.count.max()) > 4096 * 4
    assert_same(res, ora)


def test_clustered_long_lists():
    """lists of 257..4096 ids are bucketed by ordinal range; ordinals that
    cluster (300 copies of one read, then one far away) overflow a bucket and
    take the full sorting network instead"""
    rng = np.random.default_rng(5)
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), 120).tobytes()
    mid = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 120).tobytes() for _ in range(3000)]
    spread = [a if i % 7 == 0 else m for i, m in enumerate(mid)]  # uniform: bucketed
    b = rng.choice(np.frombuffer(b"ACGT", np.uint8), 90).tobytes()
    reads = [b] * 300 + spread + [b] + [a] * 5
    bases, lens = kbin.pack_reads(reads)
    ora = oracle.bin_reads(bases, lens, 25, 6, 1, True)
    assert int(ora.count.max()) > 256
    res = gpu_result(bases, lens, 25, 6, 1, True)
    assert_same(res, ora)


def test_cutoffs():
    bases, lens = oracle.read_fgets(kbin.REPO_ROOT / "tests/golden/reads.txt", 101)
    for cutoff in (0, 2, 5):
        ora = oracle.bin_reads(bases, lens, 15, 5, cutoff, True)
        res = gpu_result(bases, lens, 15, 5, cutoff, True)
        assert_same(res, ora)


def test_device_generator_roundtrip():
    import torch
    n, L = 20000, 150
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, 200000, 1000, 5)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    assert (hl == L).all() and len(bases) == n * L
    ora = oracle.bin_reads(bases, hl, 31, 7, 1, True)
    with kbin.Engine(31, 7, cutoff=1, max_read_len=L) as eng:
        eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
        eng.finalize(True)
        res = eng.export()
    assert_same(res, ora)


@pytest.mark.parametrize("ts_log2,flat_l,fill,K", [(13, 2, 60, 31), (10, 1, 60, 31), (10, 1, 30, 31),
                                                    (10, 0, 60, 31), (12, 2, 60, 63), (10, 1, 30, 63),
                                                    (10, 0, 60, 63)])
def test_heavy_bins_flat_lists(ts_log2, flat_l, fill, K, engine, monkeypatch):
    """high coverage (40K reads of a 3 kbp genome, 2000x): bins with far more
    distinct keys than one LDS table holds take the flat per-partition lists
    (KB_BIN_FLAT_L; small tables force it, low fill forces deeper first
    splits) -- and, with flat_l 0, the re-expansion path; lists run to
    thousands of ids"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_TS_LOG2", str(ts_log2))
    monkeypatch.setenv("KB_BIN_FLAT_L", str(flat_l))
    monkeypatch.setenv("KB_BIN_FILL_PCT", str(fill))
    n, L = 40000, 150
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, 3000, 5000, 9)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    ora = oracle.bin_reads(bases, hl, K, 7, 1, True)
    assert int(ora.count.max()) > (1000 if K <= 31 else 500)  # (fewer 63-mers per 150-bp read)
    with kbin.Engine(K, 7, cutoff=1, max_read_len=L, flags=kbin.KB_TRACK_FIRST) as eng:
        for _ in range(2):  # the second pass runs with the learned density
            eng.reset()
            eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
            eng.finalize(True)
            res = eng.export()
            assert_same(res, ora)
            # first occurrence: its call ordinal is the list's oldest id
            last = res.ids[res.offset[1:].astype(np.int64) - 1]
            np.testing.assert_array_equal(res.first >> np.uint64(16), last.astype(np.uint64))
            assert int((res.first & np.uint64(0xFFFF)).max()) <= L - K


@pytest.mark.parametrize("K,ts_log2,cutoff,parts,err", [(31, 10, 1, 1, 30000), (31, 12, 2, 3, 30000),
                                                        (63, 10, 1, 1, 20000), (63, 11, 1, 2, 50000),
                                                        (31, 13, 1, 1, 1000)])
def test_singleton_prefilter(K, ts_log2, cutoff, parts, err, engine, monkeypatch):
    """the heavy bins' singleton pre-filter (KB_BIN_PF=1; small tables force
    every bin onto the flat lists): reads with 2-5 % errors, so most distinct
    keys are seen once -- they go through the LDS sketch only, never the
    table; the result and the distinct count (before the prune) equal the
    oracle's, with cutoffs 1 and 2, partitioned passes, both key widths, and
    a low-error case where the sketch passes nearly everything"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_TS_LOG2", str(ts_log2))
    monkeypatch.setenv("KB_BIN_FLAT_L", "1")
    monkeypatch.setenv("KB_BIN_PF", "1")
    n, L = 30000, 150
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, 60000, err, 21)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    ora = oracle.bin_reads(bases, hl, K, 7, cutoff, True)
    distinct = oracle.bin_reads(bases, hl, K, 7, cutoff, False).n_entries
    if err >= 20000:
        assert distinct > 2 * ora.n_entries  # singleton-heavy
    with kbin.Engine(K, 7, cutoff=cutoff, max_read_len=L) as eng:
        for _ in range(2):  # the second run sizes the partitions from the learned densities
            eng.reset()
            eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
            got, nd = [], 0
            for p in range(parts):
                if parts > 1:
                    eng.set_partition(p, parts)
                eng.finalize(True)
                r = eng.export()
                nd += r.n_distinct
                got.append(r)
            assert_same(kbin.Result.concat(got) if parts > 1 else got[0], ora)
            assert nd == distinct


@pytest.mark.parametrize("ts_log2,flat_l,cutoff,parts,err", [(10, 2, 1, 1, 30000), (10, 1, 2, 2, 30000),
                                                             (10, 1, 1, 1, 20000), (10, 1, 1, 3, 50000)])
@pytest.mark.parametrize("light", ["1", "0"])
def test_light_prefilter_two_word(ts_log2, flat_l, cutoff, parts, err, light, engine, monkeypatch):
    """two-word keys (K63) with 2-5 % errors: bins that would go flat stay
    light when their keys seen twice fit under the flat depth -- a per-bin LDS
    sketch screens the singles out of every partition's sweep (KB_BIN_PF_LIGHT,
    on by default; 0 keeps the flat path).  Result and distinct count (before
    the prune) equal the oracle's, with cutoffs 1 and 2 and partitioned
    passes; the second run (learned densities) takes the light path"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_TS_LOG2", str(ts_log2))
    monkeypatch.setenv("KB_BIN_FLAT_L", str(flat_l))
    monkeypatch.setenv("KB_BIN_PF", "1")
    monkeypatch.setenv("KB_BIN_PF_LIGHT", light)
    n, L, K = 30000, 150, 63
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, 60000, err, 23)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    ora = oracle.bin_reads(bases, hl, K, 7, cutoff, True)
    distinct = oracle.bin_reads(bases, hl, K, 7, cutoff, False).n_entries
    with kbin.Engine(K, 7, cutoff=cutoff, max_read_len=L) as eng:
        eng.set_timing(True)
        for run in range(2):
            eng.reset()
            eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
            got, nd, lpb, pre = [], 0, 0, 0
            for p in range(parts):
                if parts > 1:
                    eng.set_partition(p, parts)
                eng.finalize(True)
                t = eng.timing()
                lpb += t["light_prefilter_bins"]
                pre += t["prefiltered"]
                r = eng.export()
                nd += r.n_distinct
                got.append(r)
            assert_same(kbin.Result.concat(got) if parts > 1 else got[0], ora)
            assert nd == distinct
            if run == 1:
                assert (lpb > 0) == (light == "1") and pre > 0, (lpb, pre)


@pytest.mark.parametrize("genome,n,err,parts,K,repeats", [(3000, 40000, 5000, 1, 31, 0), (20000, 60000, 1000, 2, 31, 0),
                                                          (3000, 40000, 5000, 1, 31, 300), (200000, 30000, 1000, 1, 31, 0),
                                                          (3000, 30000, 3000, 1, 63, 0), (8000, 40000, 2000, 3, 27, 50)])
def test_ranked_bins(genome, n, err, parts, K, repeats, engine, monkeypatch):
    """ranked bins (KB_BIN_RANK=2: every bin of >= 512 records ranks its
    records by call ordinal and stages ranks): high coverage -- lists of
    hundreds to thousands of ids emitted from per-key bitmaps over the ranks,
    no sort, no list kernels; low coverage -- short lists through the LDS
    windows, ranks mapped back to ordinals; low-complexity reads (a k-mer
    twice in one super-k-mer: a bitmap bit set twice) fall back to the
    cursor path.  Bit-exact against the oracle in every case"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_RANK", "2")
    L = 150
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, genome, err, 17)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    if repeats:  # tandem repeats: the same k-mer several times inside one super-k-mer
        rng = np.random.default_rng(5)
        b = bytearray(bases)
        for r in rng.choice(n, repeats, replace=False):
            unit = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(1, 4))))
            b[r * L:(r + 1) * L] = (unit * L)[:L]
        bases = bytes(b)
    ora = oracle.bin_reads(bases, hl, K, 7, 1, True)
    with kbin.Engine(K, 7, cutoff=1, max_read_len=L) as eng:
        eng.set_timing(True)
        got, rb, bp = [], 0, 0
        for p in range(parts):
            if parts > 1:
                eng.set_partition(p, parts)
            if p == 0:
                eng.submit(bases=bases, lens=hl, first_id=0)
            eng.finalize(True)
            t = eng.timing()
            rb += t["ranked_bins"]
            bp += t["bitmap_partitions"]
            got.append(eng.export())
    res = kbin.Result.concat(got) if parts > 1 else got[0]
    assert_same(res, ora)
    assert rb > 0
    if genome <= 8000:
        assert bp > 0 and int(ora.count.max()) > 256


@pytest.mark.parametrize("genome,flat_l,ts_log2,K", [(3000, 3, 13, 31), (3000, 2, 10, 31), (200000, 3, 13, 31),
                                                      (200000, 3, 11, 31), (3000, 3, 12, 63), (200000, 3, 11, 63)])
def test_split_bins(genome, flat_l, ts_log2, K, engine, monkeypatch):
    """split bins: a light bin above a fair share of one block is counted per
    hash partition in phase 0 and its partitions are binned by any block in
    phase 1 (KB_BIN_SPLIT_DIV forces it for nearly every bin); small tables
    add overflow re-splits inside a partition"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_SPLIT_DIV", "1000000")
    monkeypatch.setenv("KB_BIN_FLAT_L", str(flat_l))
    monkeypatch.setenv("KB_BIN_TS_LOG2", str(ts_log2))
    n, L = 40000, 150
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, genome, 5000, 11)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    ora = oracle.bin_reads(bases, hl, K, 7, 1, True)
    with kbin.Engine(K, 7, cutoff=1, max_read_len=L, flags=kbin.KB_TRACK_FIRST) as eng:
        for _ in range(2):  # the second pass runs with the learned density
            eng.reset()
            eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
            eng.finalize(True)
            res = eng.export()
            assert_same(res, ora)
            last = res.ids[res.offset[1:].astype(np.int64) - 1]
            np.testing.assert_array_equal(res.first >> np.uint64(16), last.astype(np.uint64))


@pytest.mark.parametrize("genome,ts_log2,fill,osplit,track", [(200000, 13, 50, 0, 0), (200000, 11, 50, 0, 1),
                                                               (200000, 10, 85, 0, 0), (3000, 11, 50, 0, 0),
                                                               (3000, 12, 85, 0, 1), (200000, 11, 50, 1, 0),
                                                               (3000, 11, 50, 1, 1)])
def test_offset_partitions(genome, ts_log2, fill, osplit, track, engine, monkeypatch):
    """light bins partitioned by the signature's offset inside the k-mer
    (bin_body): small tables push bins to depths 1-4, a
    high light-bin load (85 %) and high coverage (3 kbp genome) overfill
    ranges so they split by hash on top (the sweep stops inserting once past
    the key limit), and KB_BIN_OSPLIT=1 bins big ranges on any block; with
    and without first-occurrence tracking (the global sweep-2 path)"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    monkeypatch.setenv("KB_BIN_TS_LOG2", str(ts_log2))
    monkeypatch.setenv("KB_BIN_FILL_LIGHT_PCT", str(fill))
    monkeypatch.setenv("KB_BIN_OSPLIT", str(osplit))
    if osplit:
        monkeypatch.setenv("KB_BIN_SPLIT_DIV", "1000000")
    n, L, K = 40000, 150, 31
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, genome, 5000, 13)
    torch.cuda.synchronize()
    bases, hl = kbin.unpack_reads_to_host(words.data_ptr(), lens.data_ptr(), n, wpr, n * L)
    ora = oracle.bin_reads(bases, hl, K, 7, 1, True)
    flags = kbin.KB_TRACK_FIRST if track else 0
    with kbin.Engine(K, 7, cutoff=1, max_read_len=L, flags=flags) as eng:
        for _ in range(2):  # the second pass runs with the learned density
            eng.reset()
            eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
            eng.finalize(True)
            res = eng.export()
            assert_same(res, ora)
            if track:
                last = res.ids[res.offset[1:].astype(np.int64) - 1]
                np.testing.assert_array_equal(res.first >> np.uint64(16), last.astype(np.uint64))


@pytest.mark.parametrize("second", ["heavy", "lists"])
def test_deferred_tail_surprise(second, engine, monkeypatch):
    """a finalize after one that needed no tail kernels (no heavy bins, no
    queued lists) leaves them out; when its own bins publish a heavy bin
    (small forced tables) or queue long lists (2000x coverage) it runs them
    after all -- kb_timing.tail_reruns says so -- and the result still equals
    the oracle's"""
    import torch
    if engine != "binned":
        pytest.skip("binned engine only")
    L, K, M = 150, 31, 7
    wpr = (L + 31) // 32

    def reads(n, genome, seed):
        words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
        lens = torch.empty(n, dtype=torch.int32, device="cuda")
        kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, genome, 1000, seed)
        torch.cuda.synchronize()
        return words, lens

    w1, l1 = reads(20000, 2_000_000, 5)  # ~1.5x coverage: light bins, short lists
    w2, l2 = reads(40000, 3000, 9)       # ~2000x: lists of thousands of ids
    with kbin.Engine(K, M, cutoff=1, max_read_len=L) as eng:
        eng.submit_packed_device(w1.data_ptr(), l1.data_ptr(), 20000, wpr, 0)
        eng.finalize(True)
        t = eng.timing()
        assert t["heavy_bins"] == 0 and t["long_lists"] == 0 and t["tail_reruns"] == 0, t
        if second == "heavy":
            monkeypatch.setenv("KB_BIN_TS_LOG2", "10")
            monkeypatch.setenv("KB_BIN_FLAT_L", "1")
        eng.reset()
        eng.submit_packed_device(w2.data_ptr(), l2.data_ptr(), 40000, wpr, 0)
        eng.finalize(True)
        t = eng.timing()
        assert t["tail_reruns"] == 1, t
        if second == "heavy":
            assert t["heavy_bins"] > 0, t
        else:
            assert t["long_lists"] > 0, t
        res = eng.export()
    bases, hl = kbin.unpack_reads_to_host(w2.data_ptr(), l2.data_ptr(), 40000, wpr, 40000 * L)
    assert_same(res, oracle.bin_reads(bases, hl, K, M, 1, True))


def test_alphabet_rejected():
    """bytes outside ACGT are rejected loudly (alphabet): kb_submit
    returns before the pack kernel has run, so the error surfaces at the next
    submits or at the latest at kb_finalize, and sticks until kb_reset"""
    with kbin.Engine(11, 4) as eng:
        with pytest.raises(kbin.KbError) as ei:
            eng.submit([b"ACGTNACGTACGTACG"])
            for _ in range(3):
                eng.submit([b"ACGTACGTACGTACG"])
            eng.finalize(True)
        assert ei.value.code == kbin.KB_EALPHABET
        with pytest.raises(kbin.KbError) as ei:
            eng.finalize(True)
        assert ei.value.code == kbin.KB_EALPHABET
        eng.reset()  # a new input is clean again
        reads = [b"ACGTACGTTCGTACGTA", b"ACGTACGTTCGTACGTA", b"GGCATTACGAGGTTACA"]
        eng.submit(reads)
        eng.finalize(True)
        assert_same(eng.export(), oracle.bin_reads(b"".join(reads), [len(r) for r in reads], 11, 4, 1, True))


@pytest.mark.parametrize("how", ["scatter", "split", "plan"])
def test_alphabet_rejected_before_routing(how, engine):
    """a batch with a byte outside ACGT never leaves the context: kb_route_scatter,
    kb_split_passes and kb_route_plan check the pack status first (KB_EALPHABET),
    so no record built from the invalid read reaches a peer or a pass"""
    import torch
    if engine != "binned" and how != "plan":
        pytest.skip("the one-pass senders are the binned engine's")
    with kbin.Engine(31, 7, max_read_len=150) as eng:
        eng.submit([b"ACGT" * 20 + b"N" + b"ACGT" * 10])  # returns before the pack has run
        cap = 1024
        buf = torch.zeros(4 * cap * eng.record_words(), dtype=torch.int64, device="cuda")
        with pytest.raises(kbin.KbError) as ei:
            if how == "scatter":
                eng.route_scatter(4, buf.data_ptr(), cap)
            elif how == "split":
                eng.split_passes(4, buf.data_ptr(), cap)
            else:
                eng.route_plan(4)
        assert ei.value.code == kbin.KB_EALPHABET
        torch.cuda.synchronize()
        assert int(buf.abs().sum()) == 0  # nothing was written


def test_streaming_submits_reuse_buffer():
    """kb_submit copies in and returns without waiting (double-buffered pinned
    staging, pooled device batches): 40 batches of varying size, each written
    into ONE host buffer that is overwritten right after its submit, equal the
    oracle on the whole input; then again after kb_reset (pool and slots reused)"""
    import ctypes as C
    rng = np.random.default_rng(17)
    L, n = 150, 24_000
    genome = rng.integers(0, 4, 400_000)
    st = rng.integers(0, len(genome) - L + 1, n)
    raw = np.frombuffer(b"TGCA", dtype=np.uint8)[genome[st[:, None] + np.arange(L)]].reshape(-1)
    lens = np.full(n, L, dtype=np.uint32)
    ora = oracle.bin_reads(raw.tobytes(), lens, 31, 7, 1, True)
    cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n, 39)]))
    buf = C.create_string_buffer(len(raw))
    with kbin.Engine(31, 7, cutoff=1, max_read_len=L) as eng:
        for _ in range(2):
            for a, b in zip(cuts[:-1], cuts[1:]):
                C.memmove(buf, raw[a * L:b * L].tobytes(), int(b - a) * L)
                eng.submit(bases=buf, lens=lens[a:b], first_id=int(a))
                C.memset(buf, ord("N"), len(raw))  # the caller's buffer is free on return
            eng.finalize(True)
            assert_same(eng.export(), ora)
            eng.reset()


def test_host_cli_process_read_prune_data(digests, golden_dir):
    """The reference's C surface (process_read / prune_data over libkbin.so,
    then a walk of the MATERIALISED ZHashTable/ll_node tables) reproduces the
    known-answer digests: kbin_main = binning.c:1147-1169 up to the prune."""
    import subprocess
    exe = kbin.LIB_DIR / "kbin_main"
    for row in digests[:8]:
        out = subprocess.run([str(exe), str(golden_dir / row["input"]), str(row["K"]), str(row["M"]),
                              str(row["read_length"]), str(row["cutoff"]), "1" if row["prune"] else "0"],
                             check=True, capture_output=True, timeout=120).stdout
        assert hashlib.sha256(out).hexdigest() == row["sha256"], row


def test_kbin_main_unitigs(golden_dir, tmp_path):
    """kbin_main --unitigs: the rest of the reference's main (binning.c:1171-
    1180) after the GPU binning -- expand_read_id_list, the exact unitig
    replay forward and backward (host/unitig.c), print_kmers -- gives the
    reference program's stdout (sha256) on every unitigs.json row, without the
    reference linked: the replay's own print (kbh_print_kmers) reproduces
    print_kmers' resume from the iterator cursor the walk leaves."""
    import json
    import subprocess
    from conftest import golden_input_path
    exe = kbin.LIB_DIR / "kbin_main"
    for row in json.loads((golden_dir / "unitigs.json").read_text()):
        r = subprocess.run([str(exe), str(golden_input_path(row, tmp_path)), str(row["K"]), str(row["M"]),
                            str(row.get("read_length", 101)), str(row["cutoff"]), "1", "--unitigs"],
                           capture_output=True, timeout=300, env=dict(os.environ, KBH_TIMING="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count(b"\n") == row["lines"], row
        assert hashlib.sha256(r.stdout).hexdigest() == row["sha256"], row


def test_dropin_reference_program(golden_dir, tmp_path):
    """DROP-IN: the reference program itself (binning.c main + print_kmers,
    compiled from /root/reference into oracle/_ref in the build container)
    with process_read/prune_data/expand_read_id_list replaced by the GPU shim
    and find_kmer_extensions by the exact unitig replay (host/unitig.c) at
    link time.  Its stdout must equal the reference program's stdout byte for
    byte -- which requires the materialised ZHashTable layout (bucket chains,
    sizes, rehash history) to match the reference's exactly, and the replay to
    merge exactly the reference's pairs (reads.txt K31 M4 and K6 M3, the C2
    generator's first 20 K reads at M4: the extension is live)."""
    import json
    import subprocess
    from conftest import golden_input_path, ref_exe_name
    rows = json.loads((golden_dir / "unitigs.json").read_text())
    ran = 0
    for row in rows:
        exe = kbin.REPO_ROOT / "oracle" / "_ref" / ref_exe_name("dropin", row)
        if not exe.exists():
            continue
        out = subprocess.run([str(exe), str(golden_input_path(row, tmp_path))], check=True,
                             capture_output=True, timeout=300).stdout
        assert hashlib.sha256(out).hexdigest() == row["sha256"], row
        ran += 1
    if not ran:
        pytest.skip("drop-in binaries not built (needs the reference at build time)")


def test_host_cli_multi_gpu(digests, golden_dir):
    """kbin_main --gpus: the reference surface over a multi-GPU group (reads
    cut into contiguous per-rank ranges, mmer-sharded, records exchanged, the
    ranks' results merged and materialised) gives the known-answer digests.
    On one GPU the ranks are virtual shards ("0,0,0": the device-copy
    transport of the same C routing code)."""
    import subprocess
    exe = kbin.LIB_DIR / "kbin_main"
    for row in digests[:8]:
        out = subprocess.run([str(exe), str(golden_dir / row["input"]), str(row["K"]), str(row["M"]),
                              str(row["read_length"]), str(row["cutoff"]), "1" if row["prune"] else "0",
                              "--gpus", "0,0,0"], check=True, capture_output=True, timeout=120).stdout
        assert hashlib.sha256(out).hexdigest() == row["sha256"], row


def test_dropin_reference_program_multi_gpu(golden_dir, tmp_path):
    """the unchanged reference program on several GPUs (KBH_GPUS): its stdout
    (unitig extension and print_kmers over the materialised tables) stays
    byte-identical to the reference program's -- the merged multi-GPU result
    reproduces the exact zhash layout, first occurrences included"""
    import json
    import os
    import subprocess
    from conftest import golden_input_path, ref_exe_name
    rows = json.loads((golden_dir / "unitigs.json").read_text())
    ran = 0
    for row in rows:
        exe = kbin.REPO_ROOT / "oracle" / "_ref" / ref_exe_name("dropin", row)
        if not exe.exists():
            continue
        for gpus in ("0,0", "0,0,0,0"):
            out = subprocess.run([str(exe), str(golden_input_path(row, tmp_path))], check=True, capture_output=True,
                                 timeout=300, env=dict(os.environ, KBH_GPUS=gpus)).stdout
            assert hashlib.sha256(out).hexdigest() == row["sha256"], (row, gpus)
        ran += 1
    if not ran:
        pytest.skip("drop-in binaries not built (needs the reference at build time)")


@pytest.mark.parametrize("n,L,K,M", [(1_000_000, 150, 31, 7), (400_000, 250, 27, 6), (300_000, 250, 63, 7)])
def test_full_scale_engines_agree(engine, n, L, K, M):
    """BASELINE C2 size (1M x 150 bp, K31 M7, cutoff 1) and a longer-read
    variant: both engines produce the same canonical result; CSR contract,
    prune, list order by property (affine ids: every list non-increasing)"""
    if engine == "binned":
        pytest.skip("runs both engines itself")
    import torch
    wpr = (L + 31) // 32
    words = torch.empty(n * wpr, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    kbin.generate_reads_device(words.data_ptr(), lens.data_ptr(), n, L, 5_000_000, 1000, 2)
    torch.cuda.synchronize()
    out = {}
    for flag in (kbin.KB_ENGINE_TABLE, kbin.KB_ENGINE_BINNED):
        with kbin.Engine(K, M, cutoff=1, max_read_len=L, flags=flag) as eng:
            eng.set_timing(True)
            eng.submit_packed_device(words.data_ptr(), lens.data_ptr(), n, wpr, 0)
            eng.finalize(True)
            assert eng.timing()["engine"] == (1 if flag == kbin.KB_ENGINE_TABLE else 2)
            r = eng.export()
        assert_csr(r)
        assert int(np.asarray(r.count).min()) > 1
        ok = np.diff(np.asarray(r.ids, dtype=np.int64)) <= 0
        ok[np.asarray(r.offset[1:-1], dtype=np.int64) - 1] = True  # list boundaries
        assert bool(ok.all())
        out[flag] = r.canonical()
    a, b = out[kbin.KB_ENGINE_TABLE], out[kbin.KB_ENGINE_BINNED]
    assert a.n_entries == b.n_entries
    for f in ("mmer", "kmer_hi", "kmer_lo", "count", "offset", "ids"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))


def test_edge_inputs_and_context_reuse(engine):
    """empty input, reads shorter than K, one read, then a context reused
    across very different sizes (the binned engine's learned bucket capacity
    is exceeded and the record pass reruns)"""
    rng = np.random.default_rng(11)
    K, M = 31, 7
    with kbin.Engine(K, M, cutoff=1, max_read_len=300) as eng:
        eng.finalize(prune=True)  # nothing submitted
        assert eng.export().n_entries == 0
        eng.reset()
        eng.submit([b"ACGT" * 5, b"A" * 30])  # all shorter than K
        eng.finalize(prune=False)
        r = eng.export()
        assert r.n_entries == 0 and len(r.ids) == 0
        for n in (1, 40, 5000, 300):  # small -> large -> small
            reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(K, 300))).tobytes()
                     for _ in range(n)]
            reads += reads[: n // 3]  # repeats -> counts > 1 survive the prune
            bases, lens = kbin.pack_reads(reads)
            eng.reset()
            eng.submit(bases=bases, lens=lens, first_id=0)
            eng.finalize(prune=True)
            assert_same(eng.export(), oracle.bin_reads(bases, lens, K, M, 1, True))


def test_speculative_bucket_layout():
    """The bucket ordering goes out before the finalize's mid-way wait, in a
    layout sized from the last pass's records (kbin_finalize.hip bucket_phase).
    One context: a pass, then one with 3x the records (the layout is too
    small: the ordering reruns exactly), then the same again (the speculative
    ordering stands) -- each bit-exact against the oracle."""
    rng = np.random.default_rng(77)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=400_000)

    def reads(n, seed):
        r = np.random.default_rng(seed)
        starts = r.integers(0, len(genome) - 150, n)
        out = np.stack([genome[s:s + 150] for s in starts])
        flip = r.random(out.shape) < 0.001
        out[flip] = r.choice(np.frombuffer(b"ACGT", np.uint8), size=int(flip.sum()))
        return out.reshape(-1).tobytes(), np.full(n, 150, dtype=np.uint32)

    with kbin.Engine(31, 7, cutoff=1, max_read_len=150) as eng:
        for n, seed in ((20_000, 1), (60_000, 2), (60_000, 3)):
            bases, lens = reads(n, seed)
            eng.reset()
            eng.submit(bases=bases, lens=lens, first_id=0)
            eng.finalize(prune=True)
            assert_same(eng.export(), oracle.bin_reads(bases, lens, 31, 7, 1, True))


@pytest.mark.parametrize("K,M", [(10, 6), (5, 4), (5, 3), (7, 4), (3, 2), (13, 7), (15, 8), (1, 1)])
def test_k_below_2m_vs_oracle(K, M, engine):
    """K < 2M: the reference's incremental branch (binning.c:992-1021) is live
    -- the record pass walks the reference's own score state k-mer by k-mer
    (sk_thread_kernel QK); bit-exact against the oracle, which
    test_oracle_vs_reference_binary pins to the compiled reference at (10, 6)
    and (5, 4).  The table engine refuses these configurations."""
    rng = np.random.default_rng(K * 1000 + M)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3000)
    reads = []
    for _ in range(1500):
        L = int(rng.integers(0, 260))
        s = int(rng.integers(0, 3000 - L))
        r = genome[s:s + L].copy()
        m = rng.random(L) < 0.01
        r[m] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(m.sum()))
        reads.append(r.tobytes())
    bases, lens = kbin.pack_reads(reads)
    if engine != "binned":
        with pytest.raises(kbin.KbError):
            gpu_result(bases, lens, K, M, 1, True)
        return
    for prune in (False, True):
        ora = oracle.bin_reads(bases, lens, K, M, 1, prune)
        res = gpu_result(bases, lens, K, M, 1, prune, batches=3)
        assert res.n_kmers == ora.n_kmers
        assert_same(res, ora)


@pytest.mark.parametrize("K,M", [(10, 6), (5, 4), (13, 7), (15, 8)])
@pytest.mark.parametrize("radix", ["0", "1"])
def test_k_below_2m_long_reads(K, M, radix, engine, monkeypatch):
    """K < 2M on reads longer than 512 bp (VERDICT r05 missing #2: the
    reference's READ_LENGTH is a compile-time bound, binning.c:13): the
    long-read scan kernel walks the live incremental branch on one lane of the
    read's wave (QWalk, the same state as the thread-per-read kernel); with
    the forced radix path too (whose bins then span all 4^M codes: ADVICE
    r05).  Bit-exact against the oracle, and through route_plan/pack to three
    shards."""
    if engine != "binned":
        pytest.skip("K < 2M runs on the binned engine")
    monkeypatch.setenv("KB_BIN_RADIX", radix)
    rng = np.random.default_rng(K * 100 + M)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=20000)
    reads = []
    for _ in range(300):
        L = int(rng.integers(0, 3000)) if rng.random() < 0.7 else int(rng.integers(0, 300))
        s = int(rng.integers(0, 20000 - L))
        r = genome[s:s + L].copy()
        m = rng.random(L) < 0.01
        r[m] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(m.sum()))
        reads.append(r.tobytes())
    bases, lens = kbin.pack_reads(reads)
    for prune in (False, True):
        ora = oracle.bin_reads(bases, lens, K, M, 1, prune)
        res = gpu_result(bases, lens, K, M, 1, prune, batches=2, max_read_len=4096)
        assert res.n_kmers == ora.n_kmers
        assert_same(res, ora)
    # routed: plan/pack to three shards (kb_route_scatter serves reads <= 512 bp)
    import torch
    import skmer_ref
    rw = skmer_ref.rec_words(K, M)
    ids = np.arange(len(reads), dtype=np.int32)
    with kbin.Engine(K, M, cutoff=1, max_read_len=4096) as eng:
        eng.submit(bases=bases, lens=lens, ids=ids)
        counts = eng.route_plan(3)
        send = torch.zeros(max(1, int(counts.sum()) * rw), dtype=torch.int64, device="cuda")
        eng.route_pack(send.data_ptr())
    edges = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    union = {}
    for d in range(3):
        with kbin.Engine(K, M, cutoff=1, max_read_len=4096) as rx:
            rx.submit_superkmers_device(send[int(edges[d]) * rw:].data_ptr(), int(counts[d]))
            rx.finalize(prune=True)
            part = skmer_ref.oracle_dict(rx.export().canonical())
        assert not (set(part) & set(union))
        union.update(part)
    assert union == skmer_ref.oracle_dict(oracle.bin_reads(bases, lens, K, M, 1, True, ids=ids))

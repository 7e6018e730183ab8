"""bench.py's own contract: a plain run times --steps steps and prints the
headline line only (every other leg is behind --full), and --dump-outputs
writes the last timed step's result -- checked here against the CPU oracle
over the same reads (oracle.gen_reads: the bench generator's stream)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import kbin
import oracle

pytestmark = [pytest.mark.gpu]

N, L, GENOME, STEPS, WARMUP = 20_000, 150, 100_000, 2, 1


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """one plain run of a small C2-shaped workload (30x coverage): its line and its dump"""
    out = tmp_path_factory.mktemp("dump")
    env = dict(os.environ)
    env.pop("KB_ENGINE", None)
    r = subprocess.run([sys.executable, str(bench.REPO / "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--reads", str(N), "--genome", str(GENOME), "--input", "fresh",
                        "--dump-outputs", str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {p.stem: np.load(p) for p in out.glob("*.npy")}


def test_plain_run_line(plain_run):
    """the headline fields, --steps timed steps, and none of the --full legs"""
    line, _ = plain_run
    wl = bench.WORKLOADS["c2"]
    assert line["metric"] == bench.METRIC and line["unit"] == "k-mers/s" and line["dtype"] == "u64"
    assert line["higher_is_better"] is True and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0
    kmers = N * (L - wl["K"] + 1)
    assert line["value"] == pytest.approx(kmers / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["result"]["kmers_owned"] == kmers
    for leg in ("host_input", "capacity", "cpu_baseline", "dropin"):
        assert leg not in line
    assert "replay" not in line["input"]


def test_dump_outputs_vs_oracle(plain_run):
    """the dump is the last timed step's result: step i bins reads [i n, (i+1) n)
    of the workload's stream, so the last of WARMUP + STEPS steps binned set
    WARMUP + STEPS - 1 -- totals, digest and every sampled entry with its id
    list equal to the oracle's canonical result"""
    line, d = plain_run
    wl = bench.WORKLOADS["c2"]
    K, M = wl["K"], wl["M"]
    raw = oracle.gen_reads(N, L, GENOME, wl["err_ppm"], bench.gen_seed(wl["seed"]),
                           read_base=(WARMUP + STEPS - 1) * N)
    ora = oracle.bin_reads(raw, np.full(N, L, dtype=np.uint32), K, M, 1, True)
    assert set(d) == {"totals", "digest", "entry_index", "mmer", "kmer", "count", "offset", "ids"}
    assert all(a.dtype == np.float64 for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64_000_000
    assert d["totals"].tolist() == [ora.n_entries, len(ora.ids), ora.n_kmers, line["result"]["distinct"]]
    assert d["totals"][0] == line["result"]["entries"] and ora.n_entries > 50_000
    dig = [(int(h) << 32) | int(lo) for h, lo in d["digest"]]
    assert tuple(dig) == tuple(kbin.result_digest(ora))
    pick = d["entry_index"].astype(np.int64)
    assert len(pick) == min(ora.n_entries, bench.DUMP_ENTRIES) and (np.diff(pick) > 0).all()
    assert np.array_equal(d["mmer"], ora.mmer[pick])
    words = d["kmer"].astype(np.uint64)
    assert np.array_equal((words[:, 0] << np.uint64(32)) | words[:, 1], ora.kmer_hi[pick])
    assert np.array_equal((words[:, 2] << np.uint64(32)) | words[:, 3], ora.kmer_lo[pick])
    assert np.array_equal(d["count"], ora.count[pick])
    assert np.array_equal(d["offset"], ora.offset[:-1][pick])
    cnt = d["count"].astype(np.int64)
    j = int(np.searchsorted(np.cumsum(cnt), bench.DUMP_IDS, side="right"))
    assert j == len(pick)  # (this workload's sampled lists fit whole)
    want = np.concatenate([ora.ids[int(o):int(o) + int(c)] for o, c in zip(d["offset"], cnt)])
    assert np.array_equal(d["ids"], want)

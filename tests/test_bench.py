"""bench.py's launch contract (the driver's `python bench.py --gpus N`): without a launcher it
starts N rank processes itself; with one, WORLD_SIZE must equal --gpus."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(kw)
    return e


def test_world_size_must_match_gpus():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"], env=_env(WORLD_SIZE="2", RANK="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE 2" in r.stderr


@pytest.mark.gpu
def test_bench_spawns_two_ranks_gloo():
    """`bench.py --full --gpus 2` with no launcher: two ranks (gloo rehearsal, both on one GPU),
    one JSON line with n_gpus 2, every parity split bit-exact."""
    r = subprocess.run([sys.executable, BENCH, "--full", "--gpus", "2", "--size", "2e8", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--parity-splits", "4", "--sort-size", "2e8"],
                       env=_env(HBAM_BENCH_BACKEND="gloo"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["parallelism"] == "shard2"
    assert res["parity"]["mismatches"] == 0 and res["parity"]["splits"] == 4
    assert res["value"] > 0
    # every record of each rank's timed launch against the oracle
    assert len(res["parity"]["whole_launch"]) == 2
    for w in res["parity"]["whole_launch"]:
        assert w["mismatches"] == 0 and w["records_checked"] == w["shard_records"] > 0, w
    # config #5's leg across the ranks (tools/sort_leg.py), here over the host-staged gloo exchange
    srt = res["sort"]
    assert srt["parity"]["mismatches"] == 0, srt
    assert srt["parity"]["records_out"] == srt["parity"]["records_decoded"] > 100000
    assert srt["parity"]["oracle_sample"]["records"] > 0 and srt["records_per_s"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("gpus,extra", [(1, ["--c4-window", "2.5e8"]), (2, [])])
def test_bench_config4_windows(gpus, extra):
    """`bench.py --full --config4` (BASELINE config #4: one file sharded over the ranks, strong scaling) at a
    small total: several windows per step at N=1, two gloo ranks at N=2; every record of every window
    equals the body's resident decode, the body decode equals the oracle, the record count adds up."""
    r = subprocess.run([sys.executable, BENCH, "--full", "--gpus", str(gpus), "--config4", "--c4-total", "8e8",
                        "--c4-body", "2e8", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
                        "--parity-splits", "2"] + extra,
                       env=_env(HBAM_BENCH_BACKEND="gloo"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == gpus and res["scaling"] == "strong"
    p = res["parity"]
    assert p["mismatches"] == 0 and p["record_count_matches"], p
    assert p["records_checked_vs_body_decode"] == res["config"]["records_all_gpus"]
    if gpus == 1:
        assert res["config"]["windows_per_step_rank0"] > 1


def _bench_file(size, seed):
    """the file a one-GPU `bench.py --size --seed` run decodes, as host bytes (+ its record count)"""
    for d in ("oracle", "tools", ""):
        sys.path.insert(0, os.path.join(ROOT, d))
    import numpy as np
    import bench
    pieces, own_len, off, file_len, n_own = bench.make_shard(int(size), seed, 0, 1, 4, None, None)
    data = np.concatenate(pieces)
    assert off == 0 and own_len == file_len == len(data)
    return data, n_own


def test_bench_file_is_one_bam_of_repeated_bodies():
    """bench.make_shard: header, BODY_COPIES copies of one generated body, the unplaced tail, EOF --
    one BAM the oracle's reader reads to the end, with the record count the generator reports."""
    import bench
    import oracle
    data, n_own = _bench_file(3e8, 5)
    h = oracle.read_header(data)
    ref = oracle.read_split(data, h["first_voffset"], (len(data) << 16) | 0xffff)
    assert ref["status"] == 0 and ref["n"] == n_own
    # a body = whole generator segments (65536 records), more than one here; the tail is far shorter
    body = n_own // bench.BODY_COPIES // 65536 * 65536
    assert body > 65536 and 0 < n_own - bench.BODY_COPIES * body < 65536
    k = ref["key"]
    for c in range(1, bench.BODY_COPIES):
        assert (k[c * body:(c + 1) * body] == k[:body]).all()


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W`: the line has the headline and none of the
    --full legs; `--dump-outputs DIR` writes float32/float64 arrays of at most 64 MB whose sampled
    records equal the oracle's read of the same file (so any run with these arguments writes them)."""
    import numpy as np
    import oracle
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "1e8",
                        "--dump-outputs", out], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    a = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    U = line["config"]["uncompressed_bytes_per_gpu"]
    assert abs(line["value"] - U / (line["ms_per_step"] / 1e3) / 1e9) <= 0.01 * line["value"]
    assert line["parity"] is None and "cpu_baseline" not in line and "sort" not in line
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    data, n_own = _bench_file(1e8, 2)  # bench.py's default seed
    h = oracle.read_header(data)
    ref = oracle.read_split(data, h["first_voffset"], (len(data) << 16) | 0xffff)
    assert a["totals"][0] == ref["n"] == n_own == line["config"]["records_per_gpu"] and a["totals"][1] == 0
    idx = a["records"].astype(np.int64)
    assert len(idx) > 1000 and idx.max() > n_own // 2
    for k in ("voffset", "block_size", "ref_id", "pos", "flag", "l_seq", "tlen"):
        assert np.array_equal(a[k], ref[k][idx].astype(a[k].dtype)), k
    key = ref["key"][idx].astype(np.int64)
    assert np.array_equal(a["key_hi"], (key >> 32).astype(np.float64))
    assert np.array_equal(a["key_lo"], (key & 0xffffffff).astype(np.float64))
    # the sampled records' bytes (runs of consecutive records, concatenated) and their pools
    fb = oracle.record_fixed_bytes(ref, idx)
    vo = ref["var_off"].astype(np.int64)
    want = np.concatenate([np.concatenate([fb[j], ref["var"][vo[i]:vo[i + 1]]]) for j, i in enumerate(idx)])
    assert np.array_equal(a["ubuf"], want.astype(np.float32))
    sub = {k: (v[idx] if isinstance(v, np.ndarray) and len(v) == ref["n"] else v) for k, v in ref.items()}
    sub["n"] = len(idx)
    sub["var_off"] = np.concatenate([[0], np.cumsum(vo[idx + 1] - vo[idx])]).astype(ref["var_off"].dtype)
    sub["var"] = np.concatenate([ref["var"][vo[i]:vo[i + 1]] for i in idx])
    op = oracle.pools(sub)
    for k in ("names", "cigars", "seq", "qual", "aux"):
        assert np.array_equal(a[k], op[k].astype(a[k].dtype)), k


def test_sort_leg_budget_from_the_whole_run_deadline():
    """The Sort leg's watchdog counts from process start (--deadline), not from the leg's start,
    so a hung exchange ends while the driver's own limit still leaves time to print the line."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.sort_leg_budget(420.0, 100.0) == 320.0
    assert bench.sort_leg_budget(420.0, 420.0 - bench.SORT_LEG_MIN_S) == bench.SORT_LEG_MIN_S
    assert bench.sort_leg_budget(420.0, 400.0) == 0.0  # too little left: the leg is skipped
    assert bench.sort_leg_budget(420.0, 500.0) == 0.0


_HANG = r"""
import json, sys, time, types
sys.path.insert(0, %r)
import bench
bench.SORT_LEG_MIN_S = 0.5
fake = types.ModuleType("sort_leg")
fake.run = lambda *a, **k: time.sleep(600)  # an exchange that never returns
sys.modules["sort_leg"] = fake
args = types.SimpleNamespace(deadline=time.time() - bench.T_START + 1.5, sort_size=1, seed=0, sort_steps=1)
res = {"value": 1.0}
bench.guarded_sort_leg(None, None, 0, 2, args, 1, None, None, res)
print("not reached")
"""


def test_sort_leg_watchdog_prints_the_line_and_exits_nonzero():
    """A hung Sort leg: rank 0 prints the headline line carrying the leg's timeout, and the
    process exits with WATCHDOG_EXIT (3), so launchers see the failure."""
    r = subprocess.run([sys.executable, "-c", _HANG % ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and "not reached" not in r.stdout
    res = json.loads(lines[0])
    assert res["value"] == 1.0 and "timeout" in res["sort"]["error"]


def test_cpu_baseline_builds_the_same_pools_as_the_oracle_reader():
    """bench.py's cpu_baseline does the device decode's whole work on host cores: every record of
    its FileVirtualSplits with the lazy getters' pools built (or_read_split_pools), the same
    records and pool bytes as oracle.read_split + oracle.pools over those splits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in ("oracle", "tools", ""):
        sys.path.insert(0, os.path.join(root, d))
    import numpy as np
    import bench
    import genbam
    import oracle
    data = np.frombuffer(genbam.generate(records=20000, seed=11, odd_every=53), np.uint8)
    r = bench.cpu_baseline(data, 0.02, 3)
    assert r["status"] == [0] and r["kind"] == "port"
    sample = int(min(len(data), 0.02 * 3 * 0.06e9))
    block = int(np.ceil(sample / 3))
    begs = list(range(0, sample, block))
    ends = [min(b + block, sample) for b in begs]
    base = np.ascontiguousarray(data[:sample + (1 << 20) if sample < len(data) else len(data)])
    vs, ve = oracle.probabilistic_splits(base, np.array(begs, np.uint64), np.array(ends, np.uint64))
    n = pb = 0
    for a, b in zip(vs, ve):
        c = oracle.read_split(base, int(a), int(b))
        p = oracle.pools(c)
        n += c["n"]
        pb += sum(len(p[k]) * p[k].itemsize for k in ("names", "cigars", "seq", "qual", "aux"))
    assert n > 0 and r["records_per_s"] > 0
    assert r["pool_bytes"] == pb
    assert ("%d records" % n) in r["sample"]


def test_issue_roofline_reads_the_committed_sq_pass():
    """bench.py's roofline carries the instruction-issue view of the Huffman pass from the
    committed SQ counter pass (profiles/r06/closing/pmc_sq_3g.json)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    r = bench.issue_roofline("k_inflate_tokens")
    assert r is not None and r["waves_per_simd"] == 2
    assert 0.0 < r["simd_valu_pipe_frac"] <= 1.0 and 0.0 < r["wave_issue_frac"] <= 1.0
    assert abs(r["wave_issue_frac"] + r["wait_frac"] + r["dependency_stall_frac"] - 1.0) < 0.02
    assert bench.issue_roofline("k_no_such_kernel") is None

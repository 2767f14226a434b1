"""CPU: bench.py's host-side logic (no GPU): the workload chosen per GPU count, the shard layout of
config 4, and config 3's Zipf index."""
import numpy as np

import bench


def test_default_config_follows_gpu_count():
    # N = 1: BASELINE configs[1]; N > 1 (flag or torch.distributed.run's WORLD_SIZE): configs[3]'s shard
    assert bench.default_config(1, 1) == "uniform4k"
    for n in (2, 4, 8):
        assert bench.default_config(n, 1) == "shard8m"
        assert bench.default_config(1, n) == "shard8m"


def test_config4_shards_tile_the_global_stream():
    per, L = 8 << 20, 4096
    firsts = [bench.shard_first_word(r, per, L) for r in range(8)]
    assert firsts[0] == 0
    # consecutive shards are adjacent slices of one stream: 64M x 4 KiB in 8-byte words
    assert all(b - a == per * L // 8 for a, b in zip(firsts, firsts[1:]))
    assert firsts[-1] + per * L // 8 == (64 << 20) * L // 8


def test_zipf_index_matches_survey_shape():
    offs, lens = bench.zipf_index(1 << 16)
    assert lens.min() >= 64 and lens.max() <= 65536
    assert (offs[1:] == offs[:-1] + lens[:-1]).all()  # packed back to back
    assert 5000 < lens.mean() < 8000  # mean ~6 484 B on 1M entries
    o2, l2 = bench.zipf_index(1 << 16)
    assert np.array_equal(offs, o2) and np.array_equal(lens, l2)  # seeded


def test_dump_outputs_writes_float64_and_samples_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: u32 digests land exactly in float64; an array over its share of DUMP_LIMIT is cut
    to the same seeded sample on every call, its indices beside it; ranks write files of their own."""
    import os
    small = np.array([0, 1, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    assert bench.dump_outputs(str(tmp_path / "a"), {"digests": small}) == {"digests.npy": 4}
    got = np.load(tmp_path / "a" / "digests.npy")
    assert got.dtype == np.float64 and (got.astype(np.uint32) == small).all()
    monkeypatch.setattr(bench, "DUMP_LIMIT", 2 * 1600)  # two ranks' shares of 1600 B: 100 values + 100 indices
    big = np.arange(1000, dtype=np.int32) * 7
    for d in ("b", "c"):
        names = bench.dump_outputs(str(tmp_path / d), {"status": big}, rank=1, world=2)
        assert names == {"status_index_rank1.npy": 100, "status_rank1.npy": 100}
    idx = np.load(tmp_path / "b" / "status_index_rank1.npy")
    val = np.load(tmp_path / "b" / "status_rank1.npy")
    assert idx.dtype == val.dtype == np.float64 and (np.diff(idx) > 0).all() and idx.max() < 1000
    assert (val == big[idx.astype(np.int64)]).all()
    assert (idx == np.load(tmp_path / "c" / "status_index_rank1.npy")).all()  # a fixed sample
    total = sum(os.path.getsize(tmp_path / "b" / f) - 128 for f in os.listdir(tmp_path / "b"))
    assert total <= 1600


def test_crc32c_cpu_leg_without_the_reference_build_is_the_oracle(monkeypatch):
    """Where oracle/_ref was never built (no reference tree), --full's CPU leg for CRC32C digests the
    sample with the C oracle (it once fell through to the CRC-32 port, whose digests can never match)."""
    import oracle
    monkeypatch.setattr(oracle, "ref", lambda: None)
    n, L = 37, 4096
    data = oracle.fill_splitmix64(n * L, 42)
    cb, got = bench.cpu_baseline(data, L, oracle.CRC32C, budget_s=0.01)
    assert cb["kind"] == "oracle" and cb["cores"] == 1 and cb["value"] > 0
    assert (got == oracle.uniform(oracle.CRC32C, data, L, L, n)).all()
    offs, lens = bench.zipf_index(200)
    zdata = oracle.fill_splitmix64(int(offs[-1] + lens[-1]), 42)
    cb, got = bench.cpu_baseline_indexed(zdata, offs, lens, oracle.CRC32C, budget_s=0.01)
    assert cb["kind"] == "oracle" and (got == oracle.batch(oracle.CRC32C, zdata, offs, lens)).all()
    # CRC-32 keeps its own port either way
    cb, got = bench.cpu_baseline(data, L, oracle.CRC32, budget_s=0.01)
    assert cb["kind"] == "port" and (got == oracle.uniform(oracle.CRC32, data, L, L, n)).all()


def test_only_config2_carries_the_headline_metric():
    """BASELINE.json's metric names config 2 (1M x 4 KiB, CRC32C) only; every other
    workload's line names itself (Zipf, CRC32, config 4's shard), so none can be read as the headline."""
    import json
    import os
    base = json.load(open(os.path.join(os.path.dirname(bench.__file__), "BASELINE.json")))
    assert bench.metric_for("uniform4k", "crc32c") == base["metric"] == bench.METRIC
    others = [bench.metric_for(c, a) for c in ("uniform4k", "shard8m", "zipf", "zipf_split", "indexed4k")
              for a in ("crc32c", "crc32")
              if (c, a) != ("uniform4k", "crc32c")]
    assert len(set(others)) == len(others) and base["metric"] not in others
    assert "Zipf" in bench.metric_for("zipf", "crc32") and "CRC32 " in bench.metric_for("zipf", "crc32")
    assert "config 4" in bench.metric_for("shard8m", "crc32c")
    assert "split across the GPUs by bytes" in bench.metric_for("zipf_split", "crc32c")

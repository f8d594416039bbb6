"""bench/run.py helpers that decide what a multi-GPU run measures (CPU)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_module():
    spec = importlib.util.spec_from_file_location("bench_run", os.path.join(ROOT, "bench", "run.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_transcode_batch_sizes_from_the_rank_share():
    """Config 3 at world 8 (256 pieces -> 32 per rank) must not run one half-padded batch: the
    batch is sized from the share so every rank pipelines >= 3 equal batches."""
    tb = _run_module().transcode_batch
    for world in (1, 2, 4, 8):
        n = 256 // world
        b = tb(n, 64)
        assert n % b == 0 and n // b >= 3 and b <= 64, (world, b)
    assert tb(256, 64) == 64 and tb(32, 64) == 8
    assert tb(2, 64) == 2 and tb(1, 64) == 1        # fewer pieces than batches: one full batch
    assert tb(33, 64) == 11                          # an odd share still divides evenly


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_headline", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_arrays(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float arrays of fixed names; the same results give the same files,
    one changed byte shows in the segment's hash and (stream shorter than the sample) in the stream;
    a stream longer than the sample is cut to the sample size, in stream order and spread over it."""
    import numpy as np

    from govideocompressor_amd.models.h264_gpu import SegmentResult
    bench = _bench_module()
    rng = np.random.default_rng(5)

    def results():
        return [SegmentResult(3, nals=[rng.bytes(int(n)) for n in rng.integers(1, 400, 3 if b else 2)], header=b"\0\0\0\1gh")
                for b in range(4)]

    res = results()
    merged = np.frombuffer(b"".join(r.bitstream for r in res), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), res, merged)
    bench.dump_outputs(str(tmp_path / "b"), res, merged)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["merged_sample.npy", "nal_bytes.npy", "segment_sha48.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], np.load(tmp_path / "b" / n))
    assert a["nal_bytes.npy"].shape == (4, 4) and a["nal_bytes.npy"][0, 3] == 0     # 2 NALs, padded
    assert a["nal_bytes.npy"].sum() == len(merged) and a["nal_bytes.npy"][2, 0] == 6
    assert np.array_equal(a["merged_sample.npy"], merged.astype(np.float32))

    res[1].nals[0] = bytes([res[1].nals[0][0] ^ 1]) + res[1].nals[0][1:]
    res[1]._bs = None
    merged2 = np.frombuffer(b"".join(r.bitstream for r in res), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "c"), res, merged2)
    c = {n: np.load(tmp_path / "c" / n) for n in names}
    assert np.array_equal(c["nal_bytes.npy"], a["nal_bytes.npy"])
    assert list(np.nonzero(c["segment_sha48.npy"] != a["segment_sha48.npy"])[0]) == [1]
    assert np.count_nonzero(c["merged_sample.npy"] != a["merged_sample.npy"]) == 1

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    ramp = (np.arange(len(merged)) * 255 // len(merged)).astype(np.uint8)          # value = position
    bench.dump_outputs(str(tmp_path / "d"), res, ramp)
    d = np.load(tmp_path / "d" / "merged_sample.npy")
    assert d.shape == (64,) and d.dtype == np.float32
    assert np.all(np.diff(d) >= 0) and d[0] < 32 and d[-1] > 223 and len(np.unique(d)) > 32   # in order, spread out

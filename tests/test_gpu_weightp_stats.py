"""Weighted prediction outside the bitstream (csrc/kernels/weightp.hip): the source statistics
``wp_stats`` / ``wp_stats16``, the inverse-weighted search source ``wp_src`` and the weights the
two encoders derive from the statistics, against tests/ref_models.py.

The fade tests show that weighted pictures decode bit-exactly; a wrong sum or a wrong search
source would still decode, with worse weights or a worse search.  Here:

* the six sums per picture, exactly, at the sizes where the kernel changes path: 18x14 (63
  chroma bytes per picture: the planes of odd pictures start off a 4-byte boundary and are read
  byte by byte, and 3 bytes follow the last whole word), 16x16, 256x128 (two chunks), 1024x1024
  (64 chunks, the cap), with all-255 / all-1023 planes at the largest size;
* ``wp_src`` on every byte value for weights 0..127, offsets -128..127 and both denominators,
  exactly, in one launch with a slot per triple; planes long enough for the grid-stride loop;
* the (w, o) tables of ``GpuH264Encoder._weights`` and ``GpuHevcEncoder._weights`` (Main and
  Main 10) during an encode of a two-slot fade, against their documented formula evaluated from
  the model's sums.
"""
import numpy as np
import pytest

import ref_models as rm

pytestmark = pytest.mark.gpu

_SIZES = [(18, 14, 5), (16, 16, 3), (256, 128, 4), (1024, 1024, 3)]   # (w, h, pictures)


def _stats(planes, w, h):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
    n = planes[0].shape[0]
    out = torch.full((n, 6), -1, dtype=torch.int64).cuda()   # the launch clears it
    fn = hip.wp_stats if planes[0].dtype == np.uint8 else hip.wp_stats16
    fn(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), w, h, n, out.data_ptr(),
       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("bits", [8, 10], ids=["u8", "u16"])
@pytest.mark.parametrize("size", _SIZES, ids=["%dx%d" % s[:2] for s in _SIZES])
def test_wp_stats_equal_the_model(size, bits):
    w, h, n = size
    rng = np.random.default_rng(w + h + bits)
    dt = np.uint8 if bits == 8 else np.int16
    y = rng.integers(0, 1 << bits, (n, h, w)).astype(dt)
    u, v = (rng.integers(0, 1 << bits, (n, h // 2, w // 2)).astype(dt) for _ in range(2))
    # pictures that differ in level, so a sum taken from the neighbouring picture shows
    y[0] >>= 1
    u[n - 1] >>= 2
    got = _stats((y, u, v), w, h)
    want = rm.wp_stats(y, u, v)
    print(size, bits, got[0].tolist())
    assert np.array_equal(got, want)
    assert len({tuple(r) for r in want.tolist()}) == n


@pytest.mark.parametrize("bits", [8, 10], ids=["u8", "u16"])
def test_wp_stats_saturated_planes(bits):
    w, h, n = 1024, 1024, 3
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.int16
    y = np.full((n, h, w), top, dt)
    u = np.full((n, h // 2, w // 2), top, dt)
    got = _stats((y, u, u.copy()), w, h)
    ny, nc = w * h, w * h // 4
    assert got.tolist() == [[ny * top, ny * top * top, nc * top, nc * top * top, nc * top, nc * top * top]] * n
    assert np.array_equal(got, rm.wp_stats(y, u, u))


def test_wp_stats_refuse_odd_sizes():
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    buf = torch.zeros(4096, dtype=torch.int16).cuda()
    out = torch.zeros((1, 6), dtype=torch.int64).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for fn in (hip.wp_stats, hip.wp_stats16):
        for w, h in ((17, 14), (18, 13), (15, 15)):
            with pytest.raises(ValueError):
                fn(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), w, h, 1, out.data_ptr(), s)
    torch.cuda.synchronize()


def _triples():
    t = [(w, o, 6) for w in (0, 1, 31, 63, 64, 65, 127) for o in (-128, -1, 0, 1, 127)]
    t += [(32, 0, 5), (31, -1, 5), (1, 127, 5), (127, -128, 5), (33, 1, 5), (0, 0, 5)]
    return t


@pytest.mark.parametrize("repeat", [5, 1028], ids=["1280B", "263168B"])
def test_wp_src_equals_the_model(repeat):
    """Every byte value through every weight triple; 263168 bytes per slot are 65792 words, more
    than the 256 x 256 threads of a slot's grid, so the last words come from the stride loop."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    triples = _triples() if repeat == 5 else [(64, 0, 6), (65, -1, 6), (31, 127, 6), (127, 1, 5)]
    B = len(triples)
    row = np.tile(np.arange(256, dtype=np.uint8), repeat)
    row[-256:] = row[-256:][::-1]   # the tail differs from the head
    nbytes = row.size
    assert nbytes % 4 == 0
    src = torch.from_numpy(np.ascontiguousarray(np.repeat(row[None], B, axis=0))).cuda()
    dst = torch.full((B, nbytes), 0xA5, dtype=torch.uint8).cuda()
    wt = torch.tensor(triples, dtype=torch.int32).cuda()
    hip.wp_src(src.data_ptr(), dst.data_ptr(), wt.data_ptr(), B, nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for b, (w, o, d) in enumerate(triples):
        want = rm.wp_src(row, w, o, d)
        bad = np.flatnonzero(got[b] != want)
        assert bad.size == 0, f"(w, o, d) = {(w, o, d)}: byte {row[bad[0]]} -> {got[b][bad[0]]}, model {want[bad[0]]}"
        if w == 1 << d and o == 0:
            assert np.array_equal(got[b], row), "the identity weight copies its input"
    with pytest.raises(ValueError):
        hip.wp_src(src.data_ptr(), dst.data_ptr(), wt.data_ptr(), B, nbytes - 2, torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ host derivation
def _fade(bits, w=64, h=48, F=5, seed=5):
    """Two slots: slot 0 loses contrast frame by frame (the scale moves), slot 1 gets brighter
    over three frames (the offset moves) and then stands still (no weights)."""
    rng = np.random.default_rng(seed)

    def planes(ph, pw):
        tex = np.clip(128 + rng.normal(0, 40, (ph, pw)), 10, 245)
        out = np.zeros((2, F, ph, pw))
        for k in range(F):
            out[0, k] = 128 + (tex - 128) * (1 - 0.15 * k)
            out[1, k] = 0.6 * tex + 9 * min(k, 2)
        return out

    up = 1 << (bits - 8)
    dt = np.uint8 if bits == 8 else np.int16
    return [np.clip(np.rint(planes(ph, pw) * up), 0, (1 << bits) - 1).astype(dt) for ph, pw in
            ((h, w), (h // 2, w // 2), (h // 2, w // 2))]


def _expected(planes, b, cur, ref, unit, w_min, min_mean, min_scale):
    """The documented rule from the model's sums: scale = sqrt(var_cur / var_ref) (1 when the
    reference is flat), offset = mean_cur - w / 64 * mean_ref in 8-bit units; used when the luma
    mean moved by min_mean levels or the luma scale by min_scale.  -> [w, o] x 3, or None."""
    st = rm.wp_stats(*(p[b] for p in planes)).astype(np.float64)   # [F, 6]
    n = np.array([planes[0][b, 0].size, planes[1][b, 0].size, planes[2][b, 0].size], dtype=np.float64)
    mean = st[:, 0::2] / n / unit
    var = np.maximum(st[:, 1::2] / n / unit ** 2 - mean ** 2, 0.0)
    scale = np.array([np.sqrt(var[cur, c] / var[ref, c]) if var[ref, c] > 1e-3 else 1.0 for c in range(3)])
    if abs(mean[cur, 0] - mean[ref, 0]) < min_mean and abs(scale[0] - 1) < min_scale:
        return None
    wq = np.clip(np.rint(scale * 64), w_min, 127)
    oq = np.clip(np.rint(mean[cur] - wq / 64.0 * mean[ref]), -128, 127)
    return [int(x) for c in range(3) for x in (wq[c], oq[c])]


def test_h264_weights_follow_the_statistics():
    import torch
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params

    planes = _fade(8)
    B, F, h, w = planes[0].shape
    p = H264Params(width=w, height=h, crf=None, qp=28, bframes=0, lookahead=False, weightp=True)
    enc = GpuH264Encoder(p, slots=B)
    enc.encode(*(torch.from_numpy(q).cuda() for q in planes), metrics=False)
    table, plans = enc._wp, enc.last_plans
    enc.close()
    assert table is not None and table.shape == (F, B, 6)
    seen = {"weighted": 0, "plain": 0}
    for b in range(B):
        for t, pic in enumerate(plans[b]):
            if pic.kind != "P":
                assert table[t, b].tolist() == [64, 0, 64, 0, 64, 0]
                continue
            want = _expected(planes, b, pic.d, pic.l0, 1.0, 0, p.wp_min_mean, p.wp_min_scale)
            print("h264 slot", b, "picture", pic.d, "ref", pic.l0, table[t, b].tolist(), want)
            seen["plain" if want is None else "weighted"] += 1
            assert table[t, b].tolist() == (want or [64, 0, 64, 0, 64, 0])
    assert seen["weighted"] >= 4 and seen["plain"] >= 1, seen


@pytest.mark.parametrize("bd", [8, 10], ids=["main", "main10"])
def test_hevc_weights_follow_the_statistics(bd):
    import torch
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    planes = _fade(bd)
    B, F, h, w = planes[0].shape
    p = HevcParams(width=w, height=h, bit_depth=bd, crf=None, qp=30, bframes=0, lookahead=False, weightp=True)
    enc = GpuHevcEncoder(p, slots=B)
    seen_calls = []
    inner = enc._weights

    def spy(y, u, v, plan):
        out = inner(y, u, v, plan)
        seen_calls.append((plan, out))
        return out

    enc._weights = spy
    enc.encode(*(torch.from_numpy(q).cuda() for q in planes), metrics=False)
    enc.close()
    assert len(seen_calls) == 1
    plan, out = seen_calls[0]
    seen = {"weighted": 0, "plain": 0}
    for t, pic in enumerate(plan):
        if pic.kind != "P":
            assert t not in out
            continue
        rows = out[t][0] if t in out else [None] * B
        wsrc = out[t][2].cpu().numpy() if t in out else None
        for b in range(B):
            # weights are unit-free, offsets in 8-bit units: 10-bit statistics at 8-bit scale; a
            # weight of 0 would read as "not weighted", so the smallest is 1
            want = _expected(planes, b, pic.d, pic.l0, float(1 << (bd - 8)), 1, p.wp_min_mean, p.wp_min_scale)
            print("hevc", bd, "slot", b, "picture", pic.d, "ref", pic.l0, rows[b], want)
            seen["plain" if want is None else "weighted"] += 1
            assert rows[b] == want
            if wsrc is not None:
                assert wsrc[b].tolist() == ([want[0], want[1], 6] if want else [64, 0, 6])
    assert seen["weighted"] >= 4 and seen["plain"] >= 1, seen

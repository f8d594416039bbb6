"""GPU reconstruction of High 10 H.264 segments (decode.hip's 16-bit instantiation +
deblock16.hip, 9- and 10-bit samples in int16 planes) against the CPU decoder, bit-exact.

Every case decodes with ``GpuH264Decoder(high_depth="gpu")`` and compares every plane of every
picture with ``host.decode``.  The 8-bit twin of each random stream is ``gpu_ok`` on every
picture: nothing but the depth keeps these streams off the default GPU path.
"""
import numpy as np
import pytest
import torch

from govideocompressor_amd.utils.h264_synth import HDR_BYTES, P16x16, random_stream

pytestmark = pytest.mark.gpu

_KIND, _QP, _REF, _MV = 0, 2, 8, 16
IPCM = 4


def _planes(pic):
    w, h = pic["width"], pic["height"]
    b = pic["i420"]
    ys, cs = w * h, (w // 2) * (h // 2)
    return (b[:ys].reshape(h, w), b[ys:ys + cs].reshape(h // 2, w // 2), b[ys + cs:].reshape(h // 2, w // 2))


def _compare(host, stream, d, i=0):
    """Planes of decoded segment ``d`` against the CPU decoder's; returns the top sample."""
    ref = host.decode(stream)
    assert d.frames == len(ref)
    y, u, v = d.y.cpu().numpy(), d.u.cpu().numpy(), d.v.cpu().numpy()
    top = 0
    for t, p in enumerate(ref):
        for name, a, b in zip("yuv", (y[t], u[t], v[t]), _planes(p)):
            b = b.astype(a.dtype)
            top = max(top, int(b.max()))
            if not np.array_equal(a, b):
                diff = np.argwhere(a != b)
                raise AssertionError(f"segment {i} picture {t} plane {name}: {len(diff)} samples differ, "
                                     f"first at {diff[0].tolist()} (gpu {a[tuple(diff[0])]}, cpu {b[tuple(diff[0])]})")
    return top


def _check(host, dec, streams, bd):
    """Every segment on the GPU path, int16 planes of ``bd``-bit samples, equal to the CPU decoder's."""
    out = dec.decode(streams)
    assert dec.stats["segments_cpu"] == 0
    top = 0
    for i, (s, d) in enumerate(zip(streams, out)):
        assert d.path == "gpu", f"segment {i} fell back to the CPU decoder"
        assert d.bit_depth == bd
        assert d.y.dtype == torch.int16 and d.u.dtype == torch.int16 and d.v.dtype == torch.int16
        top = max(top, _compare(host, s, d, i))
    return top


@pytest.fixture(scope="module")
def dec():
    from govideocompressor_amd.models.h264_decode_gpu import GpuH264Decoder
    return GpuH264Decoder(high_depth="gpu")


def _cqm():
    rng = np.random.default_rng(5)
    cqm4 = rng.integers(6, 60, (6, 16)).astype(np.uint8)
    cqm8 = rng.integers(6, 60, (2, 64)).astype(np.uint8)
    return dict(cqm=3, cqm4=cqm4, cqm8=cqm8, cqm_coded=0x5A)


# (w, h, frames, seed, arguments, bit depth, top sample of the decoded planes: the depth's maximum where
# the stream reaches it, so that the clips are exercised, else None)
_CASES = {
    "cavlc_negative_qp_pcm": (96, 64, 5, 101, dict(qp=2, pcm=0.25, intra_in_p=0.3, t8x8=True), 10, 1023),
    "cabac_refs3_t8x8": (96, 64, 7, 102, dict(cabac=True, refs=3, t8x8=True, intra_in_p=0.3), 10, 1023),
    "cropped_9bit_keyint": (50, 34, 6, 103, dict(cabac=True, refs=2, t8x8=True, keyint=3, qp=8), 9, None),
    "clamped_windows": (96, 64, 5, 104, dict(density=0.4, mv_range=200), 10, 1023),
    "slices": (112, 80, 4, 105, dict(slice_rows=1, cabac=True, t8x8=True, intra_in_p=0.4), 10, 1023),
    "scaling_lists": (96, 64, 5, 106, dict(t8x8=True, cabac=True, intra_in_p=0.3, density=0.3, cqm="lists"), 10, 1023),
    "constrained_intra": (96, 64, 5, 107, dict(constrained_intra=True, intra_in_p=0.4, density=0.3), 10, 1023),
    "tall_35_mb_rows": (32, 560, 3, 108, dict(cabac=True, t8x8=True, intra_in_p=0.5, qp=20), 10, None),
    "wide_66_mb_columns": (1056, 32, 3, 109, dict(cabac=True, t8x8=True, intra_in_p=0.5, qp=20), 10, None),
}


def _stream(host, name, bit_depth=None):
    w, h, frames, seed, kw, bd, _ = _CASES[name]
    kw = dict(kw)
    if kw.get("cqm") == "lists":
        kw["cqm"] = _cqm()
    return random_stream(host, w, h, frames, seed=seed, bit_depth=bit_depth or bd, **kw)


@pytest.mark.parametrize("name", list(_CASES))
def test_gpu_decode_high10_random_records(host, dec, name):
    bd, want_top = _CASES[name][5], _CASES[name][6]
    top = _check(host, dec, [_stream(host, name)], bd)
    if want_top is not None:
        assert top == want_top


@pytest.mark.parametrize("name", list(_CASES))
def test_gpu_decode_8bit_twins_of_random_records(host, name):
    """The 8-bit twin of every case on the default decoder: both depths are instantiations of
    one kernel source, so each case guards the other depth's too.  Where the High 10 stream
    reaches its depth's maximum, the twin reaches 255.  The tall and the wide case have more MB
    rows than twice the waves of either wavefront workgroup, and a row longer than one 64-lane
    ballot of the P-picture intra scan."""
    from govideocompressor_amd.models.h264_decode_gpu import GpuH264Decoder
    d8 = GpuH264Decoder()
    s = _stream(host, name, bit_depth=8)
    out = d8.decode([s])
    assert d8.stats["segments_cpu"] == 0
    assert out[0].path == "gpu" and out[0].bit_depth == 8
    assert out[0].y.dtype == torch.uint8 and out[0].u.dtype == torch.uint8 and out[0].v.dtype == torch.uint8
    top = _compare(host, s, out[0])
    if _CASES[name][6] is not None:
        assert top == 255


class _Depth:
    """The host module with ``bit_depth`` added to the writer config of parameter_sets / write_slice."""

    def __init__(self, host, bd):
        self._host, self._bd = host, bd

    def parameter_sets(self, cfg):
        return self._host.parameter_sets(dict(cfg, bit_depth=self._bd))

    def write_slice(self, cfg, *a):
        return self._host.write_slice(dict(cfg, bit_depth=self._bd), *a)


@pytest.mark.parametrize("w,h,seed", [(64, 48, 1), (96, 80, 2)])
def test_gpu_decode_high10_b_picture(host, dec, w, h, seed):
    """I, P and a non-reference B picture (L0 / L1 / Bi / temporal direct) at 10 bits; the B
    picture's in-loop filter runs on the side stream."""
    from test_h264_bframes import _b_stream
    s, _ = _b_stream(_Depth(host, 10), w, h, seed)
    pics = host.decode(s)
    assert [p["poc"] for p in pics] == [0, 2, 4] and all(p["bit_depth"] == 10 for p in pics)
    _check(host, dec, [s], 10)


@pytest.mark.parametrize("bd", [9, 10])
def test_gpu_decode_high10_explicit_weighted_p(host, dec, bd):
    """A PCM picture, then P_L0_16x16 MBs at QP -QpBdOffset with explicit weights: offsets
    scaled by 1 << (bd - 8), clips at the depth's maximum."""
    rng = np.random.default_rng(bd)
    w, h, wmb, hmb = 64, 48, 4, 3
    nmb = wmb * hmb
    wp = [5, 4, 40, -7, 21, 3, 13, -2]
    cfg = dict(width=w, height=h, bit_depth=bd, weightp=1)
    qmin = -6 * (bd - 8)
    hdr0 = np.zeros((nmb, HDR_BYTES), np.uint8)
    hdr0[:, _KIND] = IPCM
    hdr0[:, _REF:_REF + 8] = 0xFF
    coef0 = np.zeros((nmb, 408), np.int16)
    coef0[:, :384] = rng.integers(0, 1 << bd, (nmb, 384))
    nal0, _ = host.write_slice(cfg, dict(idr=1, qp=qmin, frame_num=0), hdr0, coef0)
    hdr1 = np.zeros((nmb, HDR_BYTES), np.uint8)
    hdr1[:, _KIND] = P16x16
    hdr1[:, _QP] = qmin & 0xFF
    hdr1[:, _REF:_REF + 8] = 0xFF
    hdr1[:, _REF:_REF + 4] = 0
    mvs = rng.integers(-23, 24, (nmb, 2))
    mv4 = np.repeat(mvs[:, None, :], 4, axis=1).astype(np.int16)
    hdr1[:, _MV:_MV + 16] = np.frombuffer(mv4.tobytes(), np.uint8).reshape(nmb, 16)
    nal1, _ = host.write_slice(cfg, dict(idr=0, qp=qmin, frame_num=1, wp=wp), hdr1, np.zeros((nmb, 408), np.int16))
    s = host.parameter_sets(cfg) + nal0 + nal1
    assert _check(host, dec, [s], bd) == (1 << bd) - 1


def test_gpu_decode_mixed_depths_in_one_call(host, dec):
    """8-, 10- and 12-bit segments of one call: two GPU groups and one CPU fallback, all exact."""
    s8 = random_stream(host, 96, 64, 4, seed=121, intra_in_p=0.3)
    s10 = random_stream(host, 96, 64, 4, seed=122, intra_in_p=0.3, t8x8=True, cabac=True, bit_depth=10)
    s12 = random_stream(host, 96, 64, 3, seed=123, intra_in_p=0.3, cabac=True, bit_depth=12)
    streams = [s8, s10, s12]
    out = dec.decode(streams)
    assert [d.path for d in out] == ["gpu", "gpu", "cpu"]
    assert [d.bit_depth for d in out] == [8, 10, 12]
    assert [d.y.dtype for d in out] == [torch.uint8, torch.int16, torch.int16]
    assert dec.stats["segments_cpu"] == 1 and dec.stats["segments_gpu"] == 2
    for i, (s, d) in enumerate(zip(streams, out)):
        _compare(host, s, d, i)


def test_gpu_transcode_high10_gpu_equals_cpu_route(host):
    """Two 10-bit pieces through GpuTranscoder on either route: the decoded planes are identical,
    so the encoder's bytes are too."""
    from govideocompressor_amd.models.h264_gpu import H264Params
    from govideocompressor_amd.models.transcode import GpuTranscoder
    pieces = [random_stream(host, 96, 64, 4, seed=131, bit_depth=10, intra_in_p=0.3, t8x8=True, cabac=True),
              random_stream(host, 96, 64, 4, seed=132, bit_depth=10, intra_in_p=0.3)]
    outs = {}
    for route in ("cpu", "gpu"):
        tc = GpuTranscoder(H264Params(width=96, height=64, crf=20.0), slots=2, high_depth=route)
        outs[route] = tc.run(pieces, 30.0)
        assert tc.dec["h264"].stats["segments_cpu"] == (2 if route == "cpu" else 0)
        tc.close()
    assert [len(host.decode(o)) for o in outs["gpu"]] == [4, 4]
    assert outs["gpu"] == outs["cpu"]

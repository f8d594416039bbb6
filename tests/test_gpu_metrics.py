"""The quality metrics (csrc/kernels/metrics.hip ``sse_planes`` / ``ssim8`` and the host finish in
models/h264_gpu.py; ``GpuHevcEncoder.psnr_y``) against the numpy models of tests/ref_models.py.

Every BD-rate figure of the project rests on these numbers and nothing downstream checks them: a
wrong sum still gives a valid stream.

* direct ``hip.sse`` launches: the three sums of squared errors, exactly, at the sizes where the
  16-byte column chunks can go wrong (a chroma row that ends half way through a chunk, a display
  window inside the coded size, one chunk per row, sums above 2^32), unrouted and routed through
  a reconstruction pool in which every slot's current picture sits in another buffer and one slot
  is idle.  The padding outside the display window and the pool buffers that are not current
  hold bytes that would change the sums if they were read;
* SSIM per slot against the float64 model.  Tolerance on the mean over the windows, derived:
  (a) the float32 rounding of the kernel's formula, estimated on the test's own inputs as 4 x
  the mean absolute distance between a numpy float32 and the float64 evaluation of every
  window, plus (b) the float accumulation: one atomic add per wave of 64 windows, each within
  half an ulp (float32) of the final sum.  On the inputs below (a) + (b) comes to 1.7e-7 .. 1.3e-6
  (16x16, four windows), 1.3e-6 (180x100) and 2.1e-6 .. 2.2e-6 (176x144) of an SSIM mean of
  0.58 .. 0.77, and to 9.0e-11 on the constant 272x256 planes (SSIM 1.0e-4); on the encoded clips
  (SSIM 0.92 .. 0.94, where the variances cancel more) to 1.7e-5 .. 2.4e-5.  The kernel came
  within 2.3e-7 and 1.6e-6 of the model respectively (the tests print every figure);
* end to end: clips encoded with ``metrics=True``, every stream decoded by the CPU decoder, PSNR
  and SSIM computed by the models from the *decoder's* pictures against the source.

The two encoders define the PSNR of a segment differently, and published numbers depend on both:

* H.264 (``SegmentResult.psnr_y/u/v``): the mean over the frames of each frame's PSNR, 100 dB
  for a frame without error (``ref_models.psnr_h264``);
* HEVC (``HevcSegmentResult.psnr_y``): the PSNR of the mean squared error over all frames
  together, 99 dB without error, peak ``2^bit_depth - 1`` (``ref_models.psnr_hevc``).
"""
import math

import numpy as np
import pytest

import ref_models as rm

pytestmark = pytest.mark.gpu

# (W, H, w, h): coded and display size
_SHAPES = [(176, 144, 176, 144), (192, 112, 180, 100), (16, 16, 16, 16), (272, 256, 272, 256)]
_B, _NBUF = 3, 3
_CUR = [2, 1, 0]      # pool buffer of each slot's current picture
_KIND = [0, -1, 1]    # P, idle, B


def _ssim_tol(win64, win32):
    """-> (tolerance on the mean SSIM, its two terms): see the module text."""
    nwin = win64.size
    rounding = 4.0 * float(np.abs(win32.astype(np.float64) - win64).mean())
    waves = math.ceil(nwin / 64)
    accum = waves * 0.5 * float(np.spacing(np.float32(abs(win64.sum())))) / nwin
    return rounding + accum, (rounding, accum)


def _planes(W, H, w, h, seed):
    """Source and reconstruction of _B slots at the coded size.  Inside the display window the
    reconstruction is the source plus noise whose amplitude changes per 8x8 window (2^-2 .. 2^7),
    with some flat bright windows and some inverted ones; outside it both hold unrelated bytes.
    272x256: source 0, reconstruction 255 (4.5e9 of luma error: past 32 bits)."""
    rng = np.random.default_rng(seed)
    src, rec = [], []
    for c in range(3):
        ph, pw, dh, dw = (H, W, h, w) if c == 0 else (H // 2, W // 2, h // 2, w // 2)
        if (W, H) == (272, 256):
            src.append(np.zeros((_B, ph, pw), np.uint8))
            rec.append(np.full((_B, ph, pw), 255, np.uint8))
            continue
        yy, xx = np.mgrid[0:ph, 0:pw]
        base = 40 + 150 * (xx / max(1, pw - 1)) * (yy / max(1, ph - 1))
        s = np.clip(base[None] + rng.normal(0, 12, (_B, ph, pw)), 0, 255).astype(np.uint8)
        amp = 2.0 ** rng.uniform(-2, 7, (_B, (ph + 7) // 8, (pw + 7) // 8))
        amp = np.repeat(np.repeat(amp, 8, axis=1), 8, axis=2)[:, :ph, :pw]
        r = np.clip(np.rint(s + amp * rng.normal(0, 1, s.shape)), 0, 255).astype(np.uint8)
        for b in range(_B):
            for k in range(3):
                by, bx = rng.integers(0, max(1, ph // 8)), rng.integers(0, max(1, pw // 8))
                win = (b, slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
                if k == 0 and ph > 16:
                    s[win] = 250
                    r[win] = 249
                elif k == 1 and ph > 16:
                    r[win] = 255 - s[win]
        # outside the display window: bytes that differ a lot
        pad = np.ones((ph, pw), bool)
        pad[:dh, :dw] = False
        s[:, pad] = rng.integers(0, 64, (_B, int(pad.sum())), dtype=np.uint8)
        r[:, pad] = rng.integers(192, 256, (_B, int(pad.sum())), dtype=np.uint8)
        src.append(s)
        rec.append(r)
    return src, rec


def _route():
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE

    assert ROUTE_DTYPE.itemsize == 32
    rt = np.zeros(_B, dtype=ROUTE_DTYPE)
    rt["kind"], rt["cur"] = _KIND, _CUR
    rt["n0"] = 1
    rt["l0"][:, 0] = [(c + 1) % _NBUF for c in _CUR]   # the references are other buffers
    rt["l1"] = [(c + 2) % _NBUF for c in _CUR]
    return rt


@pytest.mark.parametrize("routed", [False, True], ids=["plain", "routed"])
@pytest.mark.parametrize("shape", _SHAPES, ids=["%dx%d-%dx%d" % s for s in _SHAPES])
def test_sse_and_ssim_against_the_models(shape, routed):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    W, H, w, h = shape
    src, rec = _planes(W, H, w, h, seed=W * 7 + h)
    dev_src = [torch.from_numpy(p).cuda() for p in src]
    if routed:
        # [B, NBUF, plane]: the current picture in its buffer, the inverted source in the others
        pools = []
        for c in range(3):
            pool = np.repeat((255 - src[c])[:, None], _NBUF, axis=1)
            for b in range(_B):
                pool[b, _CUR[b]] = rec[c][b]
            pools.append(np.ascontiguousarray(pool))
        dev_rec = [torch.from_numpy(p).cuda() for p in pools]
        rt = torch.from_numpy(_route().view(np.uint8).reshape(_B, 32).copy()).cuda()
        route, nbuf = rt.data_ptr(), _NBUF
    else:
        dev_rec = [torch.from_numpy(p).cuda() for p in rec]
        route, nbuf = 0, 0
    sse = torch.zeros((_B, 3), dtype=torch.int64).cuda()
    ssim = torch.zeros(_B, dtype=torch.float32).cuda()
    hip.sse(_B, W, H, w, h, *(t.data_ptr() for t in dev_src), *(t.data_ptr() for t in dev_rec), sse.data_ptr(),
            ssim.data_ptr(), torch.cuda.current_stream().cuda_stream, route, nbuf)
    torch.cuda.synchronize()
    got_sse, got_ssim = sse.cpu().numpy(), ssim.cpu().numpy().astype(np.float64)
    nwin = (w // 8) * (h // 8)
    for b in range(_B):
        if routed and _KIND[b] < 0:
            assert got_sse[b].tolist() == [0, 0, 0] and got_ssim[b] == 0.0, "an idle slot was measured"
            continue
        want = rm.sse_planes([p[b] for p in src], [p[b] for p in rec], w, h)
        print(shape, "slot", b, "sse", got_sse[b].tolist(), "model", want.tolist())
        assert got_sse[b].dtype == np.int64 and np.array_equal(got_sse[b], want), f"slot {b}"
        win64 = rm.ssim8_windows(src[0][b], rec[0][b], w, h)
        win32 = rm.ssim8_windows(src[0][b], rec[0][b], w, h, np.float32)
        tol, terms = _ssim_tol(win64, win32)
        print(shape, "slot", b, "ssim", got_ssim[b] / nwin, "model", win64.sum() / nwin, "tol", tol, terms)
        assert abs(got_ssim[b] / nwin - win64.sum() / nwin) <= tol, f"slot {b}"
    if (W, H) == (272, 256):
        assert int(got_sse[0, 0]) == 272 * 256 * 65025 > 2 ** 32


def test_sse_binding_refuses_bad_geometry():
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    y = torch.zeros((1, 32, 32), dtype=torch.uint8).cuda()
    c = torch.zeros((1, 16, 16), dtype=torch.uint8).cuda()
    sse = torch.zeros((1, 3), dtype=torch.int64).cuda()
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream

    def call(W, H, w, h):
        hip.sse(1, W, H, w, h, P(y), P(c), P(c), P(y), P(c), P(c), P(sse), 0, s, 0, 0)

    call(32, 32, 30, 18)
    for W, H, w, h in ((32, 32, 34, 32), (32, 32, 32, 34), (32, 32, 31, 32), (32, 32, 32, 31), (24, 32, 24, 32)):
        with pytest.raises(ValueError):
            call(W, H, w, h)
    torch.cuda.synchronize()
    assert sse.cpu().numpy().tolist() == [[0, 0, 0]]


# ------------------------------------------------------------------ end to end
_H264_CLIPS = [
    dict(id="176x144-p", w=176, h=144, slots=2, frames=6, seed=11, params=dict(bframes=0)),
    dict(id="180x100-b3", w=180, h=100, slots=2, frames=7, seed=12, params=dict(bframes=3)),
    # a forced anchor in slot 0 only: the slots follow different plans, so their current pictures
    # sit in different pool buffers at the same step
    dict(id="352x288-pyramid-spatial", w=352, h=288, slots=3, frames=9, seed=13,
         params=dict(bframes=3, pyramid=True, direct="spatial"), anchors_at=[[5], [], []]),
]


@pytest.mark.parametrize("clip", _H264_CLIPS, ids=[c["id"] for c in _H264_CLIPS])
def test_h264_metrics_equal_the_decoders_pictures(host, clip):
    """``psnr_y/u/v`` (mean of per-frame PSNRs, 100 dB at zero error) to 1e-9 dB -- the sums of
    squared errors are equal integers -- and ``ssim_y`` within the derived tolerance, from what the
    CPU decoder rebuilds from each slot's bytes."""
    from govideocompressor_amd.models.h264_gpu import GpuH264Encoder, H264Params, synth_clip

    w, h, B, F = clip["w"], clip["h"], clip["slots"], clip["frames"]
    y, u, v = synth_clip(B, F, w, h, seed=clip["seed"])
    enc = GpuH264Encoder(H264Params(width=w, height=h, **clip["params"]), slots=B)
    res = enc.encode(y, u, v, metrics=True, anchors_at=clip.get("anchors_at", ()))
    kinds = ["".join(p.kind for p in plan) for plan in enc.last_plans]
    enc.close()
    if "anchors_at" in clip:
        assert len(set(kinds)) > 1, f"the slots follow one plan: {kinds}"
    src = [p.cpu().numpy() for p in (y, u, v)]
    nwin = (w // 8) * (h // 8)
    for b, r in enumerate(res):
        pics = host.decode(r.bitstream)
        assert len(pics) == F
        sse = np.zeros((F, 3), np.int64)
        win64, win32 = [], []
        for d, pic in enumerate(pics):
            dec = [pic["y_coded"], pic["u_coded"], pic["v_coded"]]
            sse[d] = rm.sse_planes([p[b, d] for p in src], dec, w, h)
            win64.append(rm.ssim8_windows(src[0][b, d], dec[0], w, h))
            win32.append(rm.ssim8_windows(src[0][b, d], dec[0], w, h, np.float32))
        want = [rm.psnr_h264(sse[:, 0], w * h), rm.psnr_h264(sse[:, 1], w * h // 4), rm.psnr_h264(sse[:, 2], w * h // 4)]
        got = [r.psnr_y, r.psnr_u, r.psnr_v]
        print(clip["id"], "slot", b, kinds[b], "psnr", got, "model", want)
        assert sse[:, 0].min() > 0, "a lossless frame would hide the error sums behind the 100 dB cap"
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-9
        # one launch and one accumulator per frame: the mean over the frames of the per-frame
        # tolerances; the host then adds the F float32 sums (F - 1 additions, each within half an
        # ulp of the total)
        tols = [_ssim_tol(a, c) for a, c in zip(win64, win32)]
        total = float(sum(a.sum() for a in win64))
        tol = float(np.mean([t[0] for t in tols])) + (F - 1) * 0.5 * float(np.spacing(np.float32(total))) / (F * nwin)
        model = total / (F * nwin)
        print(clip["id"], "slot", b, "ssim", r.ssim_y, "model", model, "tol", tol)
        assert abs(r.ssim_y - model) <= tol


@pytest.mark.parametrize("bd", [8, 10], ids=["main", "main10"])
def test_hevc_psnr_equals_the_decoders_pictures(host, bd):
    """``psnr_y`` of the HEVC encoder (the PSNR of the mean squared error over all frames, 99 dB at
    zero error, peak 2^bd - 1; measured after deblocking and SAO) to 1e-9 dB from the CPU HEVC
    decoder's pictures."""
    from govideocompressor_amd.models.h264_gpu import synth_clip
    from govideocompressor_amd.models.hevc_gpu import GpuHevcEncoder, HevcParams

    w, h, B, F = 192, 128, 2, 5
    y, u, v = synth_clip(B, F, w, h, seed=17, bit_depth=bd)
    enc = GpuHevcEncoder(HevcParams(width=w, height=h, bit_depth=bd, sao=True, deblock=True), slots=B)
    res = enc.encode(y, u, v, metrics=True)
    enc.close()
    sy = y.cpu().numpy()
    for b, r in enumerate(res):
        pics = host.hevc_decode(r.bitstream)
        assert len(pics) == F
        per_frame = []
        for d, p in enumerate(pics):
            diff = sy[b, d].astype(np.int64) - p["y"][:h, :w].astype(np.int64)
            per_frame.append(int((diff * diff).sum()))
        want = rm.psnr_hevc(sum(per_frame), F * w * h, bd)
        other = float(np.mean([rm.psnr_hevc(s, w * h, bd) for s in per_frame]))
        print("hevc", bd, "slot", b, "psnr_y", r.psnr_y, "model", want, "mean of per-frame PSNRs", other)
        assert sum(per_frame) > 0
        assert abs(r.psnr_y - want) <= 1e-9

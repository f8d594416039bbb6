"""HEVC source preparation (csrc/kernels/hevc_filters.hip ``hevc_prep_frame``, ``hevc_proxy8``)
against tests/ref_models.py, exactly.

The encoder codes whatever source it was given and measures PSNR against that same prepared
source, so a wrong edge replication, a slip between the vector and the tail load path, a wrong
8 -> 10-bit shift or a wrong search proxy passes every decoder comparison.  Here the padded planes
and the 8-bit proxy of coded 96x64 pictures must equal ``hevc_prep`` for display sizes that end on
and off the 8-sample units (90: a luma tail, chroma 45; 66: chroma 33), for input rows that are and
are not 8- / 16-byte aligned, for three slots whose stride is larger than a frame, and for every
sample format the encoder feeds in.
"""
import numpy as np
import pytest

import ref_models as rm

pytestmark = pytest.mark.gpu

_W, _H, _B = 96, 64, 3
_SENTINEL16, _SENTINEL8 = 0x5A5A, 0xA5


def _input(w, h, bps, aligned, seed):
    """[B, rows, pitch] tensors on the device and their [B, h, w] views (chroma half size).
    aligned: pitch 112 / 64 from the allocation's start; otherwise the view starts one
    sample into a tensor of an odd pitch (rows of either alignment follow).  Either way a slot is more than a frame apart."""
    import torch

    rng = np.random.default_rng(seed)
    out = []
    for c in range(3):
        ph, pw = (h, w) if c == 0 else (h // 2, w // 2)
        pitch, x0, y0 = ((112 if c == 0 else 64), 0, 0) if aligned else (pw + 5 + (pw + 5 + 1) % 2, 1, 0)
        if bps == 1:
            a = rng.integers(0, 256, (_B, ph + 3, pitch), dtype=np.uint8)
            a[:, y0, x0:x0 + 4] = (0, 255, 1, 254)
        else:
            a = rng.integers(0, 1024, (_B, ph + 3, pitch)).astype(np.uint16)
            a[:, y0, x0:x0 + 5] = (0, 1020, 1021, 1022, 1023)
            a[:, y0 + ph - 1, x0 + pw - 5:x0 + pw] = (1023, 1022, 1021, 1020, 0)     # the replicated corner
        t = torch.from_numpy(a.view(np.int16) if bps == 2 else a).cuda()
        out.append((t, t[:, y0:y0 + ph, x0:x0 + pw], a[:, y0:y0 + ph, x0:x0 + pw].astype(np.int64)))
    return out


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("bps,bd", [(1, 8), (1, 10), (2, 10)], ids=["8to8", "8to10", "16to10"])
@pytest.mark.parametrize("w,h", [(96, 64), (90, 50), (66, 34)])
def test_prep_frame_equals_the_model(w, h, bps, bd, aligned):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    shift = bd - 8 if bps == 1 else 0
    planes = _input(w, h, bps, aligned, seed=w + bps)
    (ty, vy, hy), (tu, vu, hu), (tv, vv, hv) = planes
    assert vy.stride(2) == 1 and vu.stride(0) == vv.stride(0) and vy.stride(0) > h * vy.stride(1)
    if not aligned:
        assert vy.stride(1) % 8 and vu.stride(1) % 8 and vy.data_ptr() % (8 * bps)
    else:
        assert vy.data_ptr() % 16 == 0 and (vy.stride(1) * bps) % 16 == 0
    want = [rm.hevc_prep((hy[b], hu[b], hv[b]), w, h, _W, _H, shift, bd) for b in range(_B)]
    for with_proxy in (True, False):
        dst = [torch.full((_B, _H >> (c > 0), _W >> (c > 0)), _SENTINEL16, dtype=torch.int16).cuda() for c in range(3)]
        d8 = torch.full((_B, _H, _W), _SENTINEL8, dtype=torch.uint8).cuda()
        hip.hevc_prep_frame(_B, vy.data_ptr(), vu.data_ptr(), vv.data_ptr(), vy.stride(0) * bps, vu.stride(0) * bps,
                            vy.stride(1), vu.stride(1), bps, w, h, dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(),
                            d8.data_ptr() if with_proxy else 0, _W, _H, shift, bd, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = [p.cpu().numpy().view(np.uint16).astype(np.int64) for p in dst]
        got8 = d8.cpu().numpy().astype(np.int64)
        for b in range(_B):
            for c in range(3):
                bad = np.argwhere(got[c][b] != want[b][c])
                assert bad.size == 0, (f"slot {b} plane {c}: {len(bad)} samples differ, first {bad[0].tolist()}: "
                                       f"{got[c][b][tuple(bad[0])]} != {want[b][c][tuple(bad[0])]}")
            if with_proxy:
                assert np.array_equal(got8[b], want[b][3]) and np.array_equal(got8[b], got[0][b] >> (bd - 8))
        if not with_proxy:
            assert (got8 == _SENTINEL8).all()
    if bps == 2:
        assert want[0][0].max() == 1023 and want[0][0][_H - 1, _W - 1] == 0      # the display's last sample, replicated
    else:
        assert want[0][0].max() == 255 << shift


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("n", [8, 8 * 37, 8 * 301])
def test_proxy8_equals_the_model(n, shift):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    a = np.random.default_rng(n).integers(0, 1024, n).astype(np.uint16)
    a[:8] = (0, 255, 256, 1020, 1021, 1022, 1023, 3)
    src = torch.from_numpy(a.view(np.int16)).cuda()
    dst = torch.full((n + 16,), _SENTINEL8, dtype=torch.uint8).cuda()
    hip.hevc_proxy8(src.data_ptr(), dst.data_ptr(), n, shift, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[:n], rm.proxy8(a, shift))
    assert (got[n:] == _SENTINEL8).all()


def test_bad_geometry_is_refused():
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    src = torch.zeros((_H, _W), dtype=torch.uint8).cuda()
    dst = torch.zeros((_H, 128), dtype=torch.int16).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def prep(bps, w, W):
        hip.hevc_prep_frame(1, src.data_ptr(), src.data_ptr(), src.data_ptr(), _W * _H, _W * _H // 4, _W, _W // 2, bps, w, 32,
                            dst.data_ptr(), dst.data_ptr(), dst.data_ptr(), 0, W, 32, 0, 8, s)

    for bps, w, W in [(1, 64, 72), (1, 80, 64), (3, 64, 64)]:       # W % 16, w > W, three bytes per sample
        with pytest.raises(ValueError):
            prep(bps, w, W)
    with pytest.raises(ValueError):
        hip.hevc_proxy8(dst.data_ptr(), src.data_ptr(), 12, 0, s)
    torch.cuda.synchronize()

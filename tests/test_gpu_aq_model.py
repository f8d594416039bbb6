"""Adaptive quantisation against a model: H.264 variance AQ (csrc/kernels/aq.hip ``aq_offset``,
reached through ``aq_offsets`` and the fused ``prep_aq``) and the HEVC per-CTB AQ
(hevc_filters.hip ``hevc_aq_ctb``), against tests/ref_models.py.

tests/test_gpu_source_pass.py compares the two H.264 launches with each other, and both call the
same ``aq_offset``; the HEVC test reads back the QPs the GPU wrote.  A wrong constant, a wrong
shift or a wrap of the unsigned energy passes both.  Here the offsets of about 12k blocks --
per-block ``base + amp * noise`` with ``amp`` log-uniform in 2^-1 .. 2^7, plus planted flat 0,
flat 255 / 1023 and 0 / 255 checkerboard blocks -- must equal the float64 model.

The energy is an exact integer, so the only legitimate difference is the device's ``log2f`` and
float32 products next to a rounding boundary: a numpy float32 evaluation of the formula differs
from float64 by 1.3e-6 on these inputs.  Blocks whose float64 value lies within 1e-3 of a
half-integer (three orders above that) are allowed to differ by one; every other block must be
equal, and at most 1 % of the blocks may fall into the band (the tests print the share: 0.20 ..
0.28 % of the H.264 MBs, 0.10 .. 0.29 % of the HEVC CTBs; on an MI355X no block differed, inside
the band or outside).
"""
import numpy as np
import pytest

import ref_models as rm

pytestmark = pytest.mark.gpu

_B, _W, _H = 3, 1024, 1024
_WMB, _HMB = _W // 16, _H // 16
_NMB = _WMB * _HMB
_BAND, _BAND_CAP = 1e-3, 0.01
_cache = {}


def _planes(bits):
    """[_B, H, W] / [_B, H/2, W/2] x 2 with 0 .. 2^bits - 1 samples (uint8 / uint16).  The 10-bit
    planes are the 8-bit ones x 4 with random low bits; the planted blocks keep their meaning
    (flat 0, flat top, 0 / top checkerboard)."""
    if bits in _cache:
        return _cache[bits]
    rng = np.random.default_rng(2024)
    top = (1 << bits) - 1
    out = []
    base = rng.uniform(16, 235, (_B, _HMB, _WMB))
    amp = 2.0 ** rng.uniform(-1, 7, (_B, _HMB, _WMB))
    for n in (16, 8, 8):
        b_, a_ = (np.repeat(np.repeat(x, n, axis=1), n, axis=2) for x in (base, amp))
        p = np.clip(np.rint(b_ + a_ * rng.normal(0, 1, b_.shape)), 0, 255).astype(np.int64)
        if bits > 8:
            p = p * 4 + rng.integers(0, 4, p.shape)
        yy, xx = np.mgrid[0:n, 0:n]
        checker = ((yy + xx) & 1) * top
        for slot, (my, mx) in enumerate([(0, 0), (_HMB // 2, _WMB - 4), (_HMB - 1, _WMB - 3)]):
            for k, blk in enumerate((0, top, checker)):
                p[slot, my * n:(my + 1) * n, (mx + k) * n:(mx + k + 1) * n] = blk
        out.append(p.astype(np.uint8 if bits == 8 else np.uint16))
    _cache[bits] = out
    return out


def _energy(bits):
    key = ("e", bits)
    if key not in _cache:
        _cache[key] = rm.aq_energy(*rm.mb_blocks(*_planes(bits)))   # [_B, _NMB]
    return _cache[key]


def _check(got, want, adj, what):
    """Equality outside the band around the half-integers, at most one apart inside it, and the
    cap on the band's share."""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    band = np.abs(adj - np.floor(adj) - 0.5) < _BAND
    share = float(band.mean())
    diff = got - want
    print(what, "distinct", np.unique(want).size, "range", int(want.min()), int(want.max()), "band share", share,
          "differ inside the band", int((diff[band] != 0).sum()), "outside", int((diff[~band] != 0).sum()))
    assert share <= _BAND_CAP
    bad = np.argwhere((diff != 0) & ~band)
    assert bad.size == 0, f"{what}: {len(bad)} blocks differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert np.abs(diff).max() <= 1
    return share


def test_inputs_span_the_offsets():
    """The family covers what the kernel can get wrong: the planted blocks (energy 0 twice, once
    through the 32-bit unsigned product; the largest energy) and a wide range of offsets."""
    e = _energy(8)
    assert e[0, 0] == 0 and e[0, 1] == 0 and e[0, 2] == 6242400
    off = rm.aq_offset_h264(e, 1.0)
    assert off[0, :3].tolist() == [-15, -15, 8]
    assert np.unique(off).size >= 16 and off.max() == 8
    e10 = _energy(10)
    assert e10[0, 0] == 0 and e10[0, 1] == 0
    assert (_planes(10)[0].max(), _planes(8)[0].max()) == (1023, 255)


@pytest.mark.parametrize("use_extra", [False, True], ids=["noextra", "extra"])
@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("fused", [False, True], ids=["aq_offsets", "prep_aq"])
def test_h264_offsets_equal_the_model(fused, strength, use_extra):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    y, u, v = (torch.from_numpy(p).cuda() for p in _planes(8))
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    extra_h, extra, stride = None, 0, 0
    if use_extra:
        extra_h = np.random.default_rng(9).uniform(-30, 30, (_B, _NMB)).astype(np.float32)
        extra_d = torch.from_numpy(extra_h).cuda()
        extra, stride = P(extra_d), _NMB
    out = torch.full((_B, _NMB), 99, dtype=torch.int8).cuda()
    if fused:
        oy, ou, ov = (torch.zeros_like(t) for t in (y, u, v))
        took = hip.prep_aq(P(y), P(u), P(v), _W, _H, _W * _H, _W * _H // 4, _B, P(oy), P(ou), P(ov), _W, _H, strength,
                           P(out), s, 0, extra, stride, 0)
        assert took, "the fused launch takes 16-byte rows"
        torch.cuda.synchronize()
        assert torch.equal(oy, y) and torch.equal(ou, u) and torch.equal(ov, v)
    else:
        hip.aq_offsets(_B, _WMB, _HMB, P(y), P(u), P(v), strength, P(out), s, extra, stride, 0)
        torch.cuda.synchronize()
    e = _energy(8)
    adj = rm.aq_adj(e, strength, extra_h)
    want = rm.aq_offset_h264(e, strength, extra_h)
    if use_extra:
        assert np.rint(adj).max() > 24 and np.rint(adj).min() < -24, "the table pushes no MB past the clamp"
        assert want.max() == 24 and want.min() == -24
    _check(out.cpu().numpy(), want, adj, f"h264 fused={fused} strength={strength} extra={use_extra}")


@pytest.mark.parametrize("use_extra", [False, True], ids=["noextra", "extra"])
@pytest.mark.parametrize("bd", [8, 10])
def test_hevc_ctb_qps_equal_the_model(bd, use_extra):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    y, u, v = (torch.from_numpy(p.astype(np.int16)).cuda() for p in _planes(bd))
    P = lambda t: t.data_ptr()  # noqa: E731
    base = np.array([4, 30, 50], dtype=np.int32)   # per slot: the 0 .. 51 clamp from both sides
    qp = torch.from_numpy(base).cuda()
    wctb, hctb = _W // 32, _H // 32
    extra_h, extra, stride, rows = None, 0, 0, 0
    if use_extra:
        # the table ends three block rows above the picture's last: the CTB row it ends in has it
        # for its upper blocks only
        rows = _HMB - 3
        table = np.random.default_rng(10).uniform(-20, 20, (_B, rows, _WMB)).astype(np.float32)
        extra_d = torch.from_numpy(table).cuda()
        extra, stride = P(extra_d), rows * _WMB
        extra_h = np.zeros((_B, _HMB, _WMB), np.float32)
        extra_h[:, :rows] = table
    ctb_qp = torch.full((_B, wctb * hctb), -7, dtype=torch.int32).cuda()
    mb_aq = torch.full((_B, _NMB), 99, dtype=torch.int8).cuda()
    hip.hevc_aq(_B, _W, _H, bd, P(y), P(u), P(v), P(qp), 1.0, extra, stride, rows, P(ctb_qp), P(mb_aq),
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def quads(a):   # [_B, HMB, WMB] -> [_B, nctb, 4]: the blocks of a CTB in raster order
        return a.reshape(_B, hctb, 2, wctb, 2).transpose(0, 1, 3, 2, 4).reshape(_B, hctb * wctb, 4)

    e4 = quads(_energy(bd).reshape(_B, _HMB, _WMB))
    x4 = quads(extra_h) if use_extra else None
    mean = rm.aq_ctb_mean(e4, bd, 1.0, x4)
    want = rm.aq_ctb_hevc(e4, bd, 1.0, x4, base[:, None])
    if use_extra:
        assert np.rint(mean).max() > 12 and np.rint(mean).min() < -12, "the table pushes no CTB past the clamp"
    assert want.min() == 0 and want.max() == 51, "the base QPs do not reach the 0 .. 51 clamp"
    _check(ctb_qp.cpu().numpy(), want, mean, f"hevc bd={bd} extra={use_extra}")
    # the per-block table: the CTB's applied offset on its four blocks
    delta = (ctb_qp.cpu().numpy() - base[:, None]).reshape(_B, hctb, wctb)
    per_mb = np.repeat(np.repeat(delta, 2, axis=1), 2, axis=2).reshape(_B, _NMB)
    assert np.array_equal(mb_aq.cpu().numpy().astype(np.int64), per_mb)

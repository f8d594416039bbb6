"""Auto-variance adaptive quantisation (aq_mode 2 / 3) on the GPU against the float64 model
(tests/ref_models_aq_auto.py): the H.264 term passes (``aq_terms``, the fused ``prep_aq_terms``)
with ``aq_auto_finish``, and ``hevc_aq_terms`` with ``hevc_aq_auto_finish``.

The comparison is that of tests/test_gpu_aq_model.py: values must be equal outside a band of 1e-3
around the half-integers of the float64 ``adj`` (HEVC: of the CTB mean), may differ by one inside
it, and at most 1 % of the blocks may lie in the band.  The energies are exact integers; what
differs legitimately is the float32 term (three correctly rounded square roots, about one ulp),
the float32 products of the finish pass and the double sums, orders of magnitude below the band.

A block's offset depends on the statistics of its own slot's picture, so the three slots get
different noise amplitudes (``amp`` log-uniform in 2^-1 .. 2^3, 2^2 .. 2^7, 2^-1 .. 2^7) and
test_inputs_tell_the_slots_apart asserts on the CPU that evaluating a slot with its neighbour's
statistics (either neighbour's, at strength 1.0) changes more than 20 % of its results: a
cross-slot mix-up cannot pass.

Geometry: 1040 x 1008 for H.264 -- 65 MB columns (the fused kernel's second 64-column group has
one live lane) by 63 rows, 4095 MBs, a multiple of nothing the kernels stride by -- and
1056 x 992 for HEVC (33 x 31 CTBs).  Every finish launch runs twice into separate outputs, which
must be byte-identical (fixed summation order, no atomics).
"""
import numpy as np
import pytest

import ref_models as rm
import ref_models_aq_auto as am

pytestmark = pytest.mark.gpu

_B = 3
_AMP = ((-1, 3), (2, 7), (-1, 7))      # log2 of the noise amplitude, per slot
_H264 = (1040, 1008)
_HEVC = (1056, 992)
_MODES = [(2, 1.0), (3, 1.0), (2, 0.5), (3, 0.5)]
_MODE_IDS = [f"mode{m}-s{s}" for m, s in _MODES]
_TERM_RTOL = 4 * 2.0 ** -23            # float32 term against float64: about one ulp; four allowed
_cache = {}


def _planes(size, bits, seed=2024):
    """[_B, H, W] / [_B, H/2, W/2] x 2 of per-block ``base + amp * noise`` with 0 .. 2^bits - 1
    samples; the 10-bit planes are the 8-bit ones x 4 with random low bits.  Planted per slot:
    a flat 0, a flat top and a 0 / top checkerboard block."""
    key = (size, bits, seed)
    if key in _cache:
        return _cache[key]
    W, H = size
    wmb, hmb = W // 16, H // 16
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    base = rng.uniform(16, 235, (_B, hmb, wmb))
    amp = np.stack([2.0 ** rng.uniform(lo, hi, (hmb, wmb)) for lo, hi in _AMP])
    out = []
    for n in (16, 8, 8):
        b_, a_ = (np.repeat(np.repeat(x, n, axis=1), n, axis=2) for x in (base, amp))
        p = np.clip(np.rint(b_ + a_ * rng.normal(0, 1, b_.shape)), 0, 255).astype(np.int64)
        if bits > 8:
            p = p * 4 + rng.integers(0, 4, p.shape)
        yy, xx = np.mgrid[0:n, 0:n]
        checker = ((yy + xx) & 1) * top
        for slot, (my, mx) in enumerate([(0, 0), (hmb // 2, wmb - 4), (hmb - 1, wmb - 3)]):
            for k, blk in enumerate((0, top, checker)):
                p[slot, my * n:(my + 1) * n, (mx + k) * n:(mx + k + 1) * n] = blk
        out.append(p.astype(np.uint8 if bits == 8 else np.uint16))
    _cache[key] = out
    return out


def _energy(size, bits, seed=2024):
    key = ("e", size, bits, seed)
    if key not in _cache:
        _cache[key] = rm.aq_energy(*rm.mb_blocks(*_planes(size, bits, seed)))   # [_B, nmb]
    return _cache[key]


def _quads(a, size):
    """[_B, nmb] (raster) -> [_B, nctb, 4]: the blocks of a CTB in raster order."""
    wmb, hmb = size[0] // 16, size[1] // 16
    return a.reshape(_B, hmb // 2, 2, wmb // 2, 2).transpose(0, 1, 3, 2, 4).reshape(_B, (hmb // 2) * (wmb // 2), 4)


def test_inputs_tell_the_slots_apart():
    """(CPU) The planted blocks are there, the slots' means differ, the band holds few blocks and
    a slot evaluated with its neighbour's statistics gets other results."""
    for size, bits in ((_H264, 8), (_HEVC, 8), (_HEVC, 10)):
        e = _energy(size, bits)
        wmb = size[0] // 16
        assert e[0, 0] == 0 and e[0, 1] == 0 and e[0, 2] == 96 * ((1 << bits) - 1) ** 2   # 6242400 at 8 bits
        a = am.aq_auto_terms(e, bits)
        m, avg = am.aq_auto_stats(a)
        print(size, bits, "m", m.ravel().round(3).tolist(), "avg", avg.ravel().round(3).tolist(), "a max", float(a.max()))
        assert np.ptp(m) > 1.0 and a.min() == 1.0
        assert e.shape[1] % 64 and wmb % 2 == (1 if size == _H264 else 0)
        for mode, s in _MODES:
            own = am.aq_auto_adj(e, mode, s, bd=bits)
            q = own if size == _H264 else am.ctb_mean(_quads(own, size))
            band = np.abs(q - np.floor(q) - 0.5) < am.BAND
            print("  mode", mode, "strength", s, "band share", float(band.mean()))
            for shift in (1, -1):   # the statistics of either neighbour
                other = (np.roll(m, shift, axis=0), np.roll(avg, shift, axis=0))
                swapped = am.aq_auto_adj(e, mode, s, bd=bits, stats=other)
                if size == _H264:
                    changed = (am.offset_h264(own) != am.offset_h264(swapped)).mean(axis=1)
                else:
                    qs = am.ctb_mean(_quads(swapped, size))
                    changed = (am.ctb_qp_hevc(q, 26) != am.ctb_qp_hevc(qs, 26)).mean(axis=1)
                print("    results changed with the statistics of slot + %d:" % shift, changed.round(3).tolist())
                # (at strength 0.5 the offsets, and with them the shares, shrink: as low as 12 % of
                # the CTBs of one slot; a mix-up at one strength is one at the other)
                if s == 1.0:
                    assert (changed > 0.2).all()
            assert band.mean() <= am.BAND_CAP
            # float32 evaluation of the whole rule: far inside the band
            a32 = a.astype(np.float32)
            sm, av = (np.float32(s) * m).astype(np.float32), avg.astype(np.float32)
            adj32 = sm * (a32 - av)
            if mode == 3:
                adj32 = adj32 + np.float32(s) * (np.float32(1) - np.float32(14) / (a32 * a32))
            assert adj32.dtype == np.float32 and np.abs(adj32 - own).max() < 1e-5


def _route_tables(nmb, frames=3):
    """Slot 0 codes a reference picture (display index 1), slot 1 a non-reference picture, slot 2
    is idle: only slot 0 takes a row of the [B, F, nmb] MB-tree table."""
    from govideocompressor_amd.models.h264_gpu import ROUTE_DTYPE, SF_REF

    rt = np.zeros(_B, dtype=ROUTE_DTYPE)
    rt["kind"], rt["flags"], rt["disp"] = [0, 1, -1], [SF_REF, 0, 0], [1, 2, -1]
    table = np.random.default_rng(12).uniform(-8, 8, (_B, frames, nmb)).astype(np.float32)
    used = np.zeros((_B, nmb), np.float32)
    used[0] = table[0, 1]
    return rt, table, used


def _h264_finish_twice(hip, terms, nmb, mode, strength, extra=0, stride=0, rt=0):
    import torch

    s = torch.cuda.current_stream().cuda_stream
    outs = [torch.full((_B, nmb), 99, dtype=torch.int8).cuda() for _ in range(2)]
    for o in outs:
        hip.aq_auto_finish(_B, nmb, terms.data_ptr(), mode, strength, o.data_ptr(), s, extra, stride, rt)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "two finish launches on the same terms differ"
    return outs[0].cpu().numpy()


def _h264_terms(hip, planes, fused):
    """The term buffer of 8-bit coded-size planes [_B, H, W] by either launch."""
    import torch

    y, u, v = planes
    H, W = y.shape[1:]
    nmb = (W // 16) * (H // 16)
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731
    terms = torch.full((_B, nmb), -1.0, dtype=torch.float32).cuda()
    if fused:
        oy, ou, ov = (torch.zeros_like(t) for t in (y, u, v))
        took = hip.prep_aq_terms(P(y), P(u), P(v), W, H, W * H, W * H // 4, _B, P(oy), P(ou), P(ov), W, H, P(terms), s, 0)
        assert took, "the fused launch takes 16-byte rows"
        torch.cuda.synchronize()
        assert torch.equal(oy, y) and torch.equal(ou, u) and torch.equal(ov, v)
    else:
        hip.aq_terms(_B, W // 16, H // 16, P(y), P(u), P(v), P(terms), s)
        torch.cuda.synchronize()
    return terms


def test_h264_terms_fused_and_unfused():
    """Both term launches give the same float32 bits, one ulp or so from the float64 term."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    planes = [torch.from_numpy(p).cuda() for p in _planes(_H264, 8)]
    t0, t1 = _h264_terms(hip, planes, False), _h264_terms(hip, planes, True)
    assert torch.equal(t0, t1)
    got, want = t0.cpu().numpy().astype(np.float64), am.aq_auto_terms(_energy(_H264, 8))
    rel = np.abs(got - want) / want
    print("terms: largest relative difference", float(rel.max()), "of", _TERM_RTOL)
    assert rel.max() <= _TERM_RTOL
    assert got[0, 0] == 1.0 and got[0, 1] == 1.0 and got.min() == 1.0


@pytest.mark.parametrize("use_extra", [False, True], ids=["noextra", "extra"])
@pytest.mark.parametrize("mode,strength", _MODES, ids=_MODE_IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["aq_terms", "prep_aq_terms"])
def test_h264_offsets_equal_the_model(fused, mode, strength, use_extra):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    planes = [torch.from_numpy(p).cuda() for p in _planes(_H264, 8)]
    nmb = (_H264[0] // 16) * (_H264[1] // 16)
    extra_h, extra, stride = None, 0, 0
    if use_extra:
        extra_h = np.random.default_rng(9).uniform(-30, 30, (_B, nmb)).astype(np.float32)
        extra_d = torch.from_numpy(extra_h).cuda()
        extra, stride = extra_d.data_ptr(), nmb
    terms = _h264_terms(hip, planes, fused)
    got = _h264_finish_twice(hip, terms, nmb, mode, strength, extra, stride)
    adj = am.aq_auto_adj(_energy(_H264, 8), mode, strength, extra_h)
    want = am.offset_h264(adj)
    if use_extra:
        assert np.rint(adj).max() > 24 and np.rint(adj).min() < -24, "the table pushes no MB past the clamp"
        assert want.max() == 24 and want.min() == -24
    am.check_band(got, want, adj, f"h264 fused={fused} mode={mode} strength={strength} extra={use_extra}")


@pytest.mark.parametrize("mode", [2, 3])
def test_h264_routed_table(mode):
    """The batch's [B, F, nmb] MB-tree table with the step's routing: the slot coding a reference
    picture takes the row of its display index, the non-reference and the idle slot none (and
    all three get offsets from their own planes)."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    planes = [torch.from_numpy(p).cuda() for p in _planes(_H264, 8)]
    nmb = (_H264[0] // 16) * (_H264[1] // 16)
    rt, table, used = _route_tables(nmb)
    rt_d = torch.from_numpy(rt.view(np.uint8).reshape(_B, -1).copy()).cuda()
    table_d = torch.from_numpy(table).cuda()
    terms = _h264_terms(hip, planes, True)
    got = _h264_finish_twice(hip, terms, nmb, mode, 1.0, table_d.data_ptr(), table.shape[1] * nmb, rt_d.data_ptr())
    adj = am.aq_auto_adj(_energy(_H264, 8), mode, 1.0, used)
    am.check_band(got, am.offset_h264(adj), adj, f"h264 routed mode={mode}")


def test_h264_fused_replicated_rows():
    """Display height below the coded height: the fused launch replicates the last rows, and the
    statistics are those of the coded (padded) picture."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    W, H = _H264
    h = H - 10
    full = _planes(_H264, 8)
    shown = [full[0][:, :h], full[1][:, :h // 2], full[2][:, :h // 2]]
    padded = [np.pad(p, ((0, 0), (0, (H >> (c > 0)) - p.shape[1]), (0, 0)), mode="edge") for c, p in enumerate(shown)]
    y, u, v = (torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in shown)
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    nmb = (W // 16) * (H // 16)
    oy, ou, ov = (torch.full(p.shape, 99, dtype=torch.uint8).cuda() for p in padded)
    terms = torch.full((_B, nmb), -1.0, dtype=torch.float32).cuda()
    assert hip.prep_aq_terms(P(y), P(u), P(v), W, h, W * h, W * h // 4, _B, P(oy), P(ou), P(ov), W, H, P(terms), s, 0)
    torch.cuda.synchronize()
    for got, want in zip((oy, ou, ov), padded):
        assert np.array_equal(got.cpu().numpy(), want)
    e = rm.aq_energy(*rm.mb_blocks(*padded))
    assert (e[:, -_H264[0] // 16:] != _energy(_H264, 8)[:, -_H264[0] // 16:]).any()   # the last MB row changed
    for mode in (2, 3):
        adj = am.aq_auto_adj(e, mode, 1.0)
        am.check_band(_h264_finish_twice(hip, terms, nmb, mode, 1.0), am.offset_h264(adj), adj, f"h264 replicated rows mode={mode}")
    # the unfused launch on the padded planes: the same terms
    assert torch.equal(_h264_terms(hip, [oy, ou, ov], False), terms)


def test_h264_fused_frame_selection():
    """A 2-frame clip per slot and a per-slot frame selection: planes and terms of the chosen frames."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    W, H = _H264
    clips = [np.ascontiguousarray(np.stack([a, b], axis=1)) for a, b in zip(_planes(_H264, 8), _planes(_H264, 8, seed=77))]
    pick = [1, 0, 1]
    chosen = [np.stack([c[b, pick[b]] for b in range(_B)]) for c in clips]
    y, u, v = (torch.from_numpy(c).cuda() for c in clips)
    fsel = torch.tensor(pick, dtype=torch.int32).cuda()
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    nmb = (W // 16) * (H // 16)
    oy, ou, ov = (torch.full(p.shape, 99, dtype=torch.uint8).cuda() for p in chosen)
    terms = torch.full((_B, nmb), -1.0, dtype=torch.float32).cuda()
    assert hip.prep_aq_terms(P(y), P(u), P(v), W, H, 2 * W * H, 2 * W * H // 4, _B, P(oy), P(ou), P(ov), W, H, P(terms), s,
                             P(fsel))
    torch.cuda.synchronize()
    for got, want in zip((oy, ou, ov), chosen):
        assert np.array_equal(got.cpu().numpy(), want)
    e = rm.aq_energy(*rm.mb_blocks(*chosen))
    for mode in (2, 3):
        adj = am.aq_auto_adj(e, mode, 1.0)
        am.check_band(_h264_finish_twice(hip, terms, nmb, mode, 1.0), am.offset_h264(adj), adj, f"h264 fsel mode={mode}")
    assert torch.equal(_h264_terms(hip, [oy, ou, ov], False), terms)


def test_h264_fused_refuses_unaligned_width():
    """A display width off the coded width is not the fused launch's: nothing launched, nothing written."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    w, h, W, H = 40, 32, 48, 32
    y = torch.zeros((1, h, w), dtype=torch.uint8).cuda()
    u = torch.zeros((1, h // 2, w // 2), dtype=torch.uint8).cuda()
    oy = torch.full((1, H, W), 99, dtype=torch.uint8).cuda()
    ou, ov = (torch.full((1, H // 2, W // 2), 99, dtype=torch.uint8).cuda() for _ in range(2))
    terms = torch.full((1, 6), -1.0).cuda()
    P = lambda t: t.data_ptr()  # noqa: E731
    took = hip.prep_aq_terms(P(y), P(u), P(u), w, h, w * h, w * h // 4, 1, P(oy), P(ou), P(ov), W, H, P(terms),
                             torch.cuda.current_stream().cuda_stream, 0)
    torch.cuda.synchronize()
    assert not took and int((oy != 99).sum()) == 0 and float(terms.max()) == -1.0


@pytest.mark.parametrize("B,n", [(2, 138240), (256, 1023), (1, 1)], ids=["8k", "256slots", "oneblock"])
def test_finish_shapes(B, n):
    """The finish pass alone on given terms: 138240 blocks per slot (an 8192 x 4320 picture), 256
    slots, and a single block."""
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    rng = np.random.default_rng(B * 7 + n)
    e = (2.0 ** (rng.uniform(0, 1, (B, n)) * rng.uniform(8, 23, (B, 1)))).astype(np.int64)   # each slot its own range
    if n > 1:
        e[0, 0] = 0   # (alone in its picture a flat block sits on a half-integer: -19.5 in mode 3)
    a32 = am.aq_auto_terms(e).astype(np.float32)
    terms = torch.from_numpy(a32).cuda()
    s = torch.cuda.current_stream().cuda_stream
    outs = [torch.full((B, n), 99, dtype=torch.int8).cuda() for _ in range(2)]
    for o in outs:
        hip.aq_auto_finish(B, n, terms.data_ptr(), 3, 1.0, o.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    adj = am.aq_auto_adj(e, 3, 1.0)
    am.check_band(outs[0].cpu().numpy(), am.offset_h264(adj), adj, f"finish B={B} n={n}")


@pytest.mark.parametrize("use_extra", [False, True], ids=["noextra", "extra"])
@pytest.mark.parametrize("mode,strength", _MODES, ids=_MODE_IDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_hevc_ctb_qps_equal_the_model(bd, mode, strength, use_extra):
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    W, H = _HEVC
    wmb, hmb, wctb, hctb = W // 16, H // 16, W // 32, H // 32
    nmb = wmb * hmb
    y, u, v = (torch.from_numpy(p.astype(np.int16)).cuda() for p in _planes(_HEVC, bd))
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    base = np.array([4, 30, 50], dtype=np.int32)   # per slot: the 0 .. 51 clamp from both sides
    qp = torch.from_numpy(base).cuda()
    extra_h, extra, stride, rows = None, 0, 0, 0
    if use_extra:
        # the table ends three block rows above the picture's last, inside a CTB row: that row has
        # it for its upper blocks only
        rows = hmb - 3
        assert rows % 2 == 1
        table = np.random.default_rng(10).uniform(-20, 20, (_B, rows, wmb)).astype(np.float32)
        extra_d = torch.from_numpy(table).cuda()
        extra, stride = P(extra_d), rows * wmb
        extra_h = np.zeros((_B, hmb, wmb), np.float32)
        extra_h[:, :rows] = table
        extra_h = extra_h.reshape(_B, nmb)
    terms = torch.full((_B, nmb), -1.0, dtype=torch.float32).cuda()
    hip.hevc_aq_terms(_B, W, H, bd, P(y), P(u), P(v), P(terms), s)
    outs = []
    for _ in range(2):
        ctb_qp = torch.full((_B, wctb * hctb), -7, dtype=torch.int32).cuda()
        mb_aq = torch.full((_B, nmb), 99, dtype=torch.int8).cuda()
        hip.hevc_aq_auto_finish(_B, W, H, P(terms), P(qp), mode, strength, extra, stride, rows, P(ctb_qp), P(mb_aq), s)
        outs.append((ctb_qp, mb_aq))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    e = _energy(_HEVC, bd)
    got_t, want_t = terms.cpu().numpy().astype(np.float64), am.aq_auto_terms(e, bd)
    assert (np.abs(got_t - want_t) / want_t).max() <= _TERM_RTOL
    adj = am.aq_auto_adj(e, mode, strength, extra_h, bd=bd)
    mean = am.ctb_mean(_quads(adj, _HEVC))
    want = am.ctb_qp_hevc(mean, base[:, None])
    if use_extra:
        assert np.rint(mean).max() > 12 and np.rint(mean).min() < -12, "the table pushes no CTB past the clamp"
    # (mode 2 at strength 0.5 alone takes at most 2.7 off: base QP 4 stops at 1 there)
    low = 1 if (mode, strength, use_extra) == (2, 0.5, False) else 0
    assert want.min() == low and want.max() == 51, "the base QPs do not reach the 0 .. 51 clamp"
    got = outs[0][0].cpu().numpy()
    am.check_band(got, want, mean, f"hevc bd={bd} mode={mode} strength={strength} extra={use_extra}")
    # the per-block table: the CTB's applied offset on its four blocks
    delta = (got - base[:, None]).reshape(_B, hctb, wctb)
    per_mb = np.repeat(np.repeat(delta, 2, axis=1), 2, axis=2).reshape(_B, nmb)
    assert np.array_equal(outs[0][1].cpu().numpy().astype(np.int64), per_mb)


def test_bindings_validate_their_arguments():
    import torch
    from govideocompressor_amd.ops import native

    hip = native.hip()
    t = torch.ones((1, 4), dtype=torch.float32).cuda()
    o = torch.zeros((1, 4), dtype=torch.int8).cuda()
    q = torch.zeros((1,), dtype=torch.int32).cuda()
    c = torch.zeros((1, 1), dtype=torch.int32).cuda()
    for mode in (0, 1, 4):
        with pytest.raises(ValueError, match="mode"):
            hip.aq_auto_finish(1, 4, t.data_ptr(), mode, 1.0, o.data_ptr(), 0)
        with pytest.raises(ValueError, match="mode"):
            hip.hevc_aq_auto_finish(1, 32, 32, t.data_ptr(), q.data_ptr(), mode, 1.0, 0, 0, 0, c.data_ptr(), o.data_ptr(), 0)
    with pytest.raises(ValueError):
        hip.aq_auto_finish(1, 4, 0, 2, 1.0, o.data_ptr(), 0)
    with pytest.raises(ValueError):
        hip.aq_auto_finish(1, 0, t.data_ptr(), 2, 1.0, o.data_ptr(), 0)
    with pytest.raises(ValueError):
        hip.aq_terms(1, 1, 1, t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 0)
    with pytest.raises(ValueError):
        hip.prep_aq_terms(t.data_ptr(), t.data_ptr(), t.data_ptr(), 16, 16, 256, 64, 1, t.data_ptr(), t.data_ptr(),
                          t.data_ptr(), 16, 16, 0, 0)
    with pytest.raises(ValueError):
        hip.hevc_aq_terms(1, 48, 32, 8, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 0)
    with pytest.raises(ValueError, match="extra_rows"):
        hip.hevc_aq_auto_finish(1, 32, 32, t.data_ptr(), q.data_ptr(), 2, 1.0, t.data_ptr(), 4, 3, c.data_ptr(), o.data_ptr(), 0)
    with pytest.raises(ValueError):
        hip.hevc_aq_auto_finish(1, 32, 32, t.data_ptr(), 0, 2, 1.0, 0, 0, 0, c.data_ptr(), o.data_ptr(), 0)

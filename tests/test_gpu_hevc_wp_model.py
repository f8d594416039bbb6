"""The HEVC motion compensation and weighted sample prediction of hevc_inter_cu (mc_block,
csrc/kernels/hevc_mc.h) through its stand-alone probe launch ``hip.hevc_mc_probe``, and the
forward proxy weight ``hip.wp_ref8``, against the numpy model tests/ref_models_hevc_wp.py --
exactly.  The model itself is pinned by hand (tests/test_ref_models_hevc_wp.py) and against the
independent decoder (tests/test_hevc_weightb_codec.py).

Planes of 48x40 luma / 24x20 chroma samples; block sizes 8 / 16 / 32 with the 8-tap filter and
4 / 8 / 16 with the 4-tap filter; the three directions; 8 and 10 bit; all 16 luma and 24 of the 64
chroma phases; vectors past each of the four edges and a corner; no weight, one list, both, the
extreme values; random, all-zero and all-maximum reference planes; both LDS layouts.
"""
import numpy as np
import pytest

import ref_models_hevc_wp as wm

pytestmark = pytest.mark.gpu

# (ww, wo, ww1, wo1, wb, plane pair, lean): mc_block's arguments as hevc_inter_cu passes them -- in
# a weighted slot a list without weight enters as (64, 0)
WEIGHTS = [
    (0, 0, 0, 0, 0, 0, 1),          # the default instances, default weighting
    (0, 0, 0, 0, 1, 0, 0),          # a weightb instance on a slot without weights
    (96, -20, 0, 0, 0, 0, 1),       # weightp's uni-directional weight in the default instances
    (96, -20, 64, 0, 1, 0, 1),      # list 0 only
    (64, 0, 96, -20, 1, 1, 0),      # list 1 only
    (96, -20, 40, 33, 1, 0, 1),     # both
    (1, 127, 127, -128, 1, 2, 1),   # extremes, on all-zero / all-maximum planes too
    (127, -128, 1, 127, 1, 1, 0),
    (127, 127, 127, 127, 1, 2, 0),
    (64, 0, 64, 0, 1, 1, 1),        # identity written out
]


def _planes(bd, chroma):
    rng = np.random.default_rng(100 + bd + chroma)
    h, w = (20, 24) if chroma else (40, 48)
    mx = (1 << bd) - 1
    r = [rng.integers(0, mx + 1, (h, w)).astype(np.uint16) for _ in range(2)]
    zero, full = np.zeros((h, w), np.uint16), np.full((h, w), mx, np.uint16)
    return [(r[0], r[1]), (full, r[1]), (zero, full)]


def _cases(chroma, n):
    """int16 [ncase, 6]: block x, y, list-0 vector, list-1 vector"""
    fb = 3 if chroma else 2
    nph = 1 << fb
    pw, ph = (24, 20) if chroma else (48, 40)
    out = []
    if chroma:
        phases = [(fx, (3 * fx + 1) % 8) for fx in range(8)] + [(0, f) for f in range(8)] + [(f, 0) for f in range(8)]
    else:
        phases = [(fx, fy) for fy in range(4) for fx in range(4)]
    for k, (fx, fy) in enumerate(phases):
        gx, gy = phases[-1 - k]
        out.append((4, 4, ((k % 5 - 2) << fb) + fx, ((k % 3 - 1) << fb) + fy, ((1 - k % 4) << fb) + gx, ((k % 2) << fb) + gy))
    far = (pw + 8) << fb
    for (bx, by, mx, my) in ((0, 4, -(6 << fb) + 1, 2), (pw - n, 4, (6 << fb) + 3, 1), (4, 0, 1, -(5 << fb) + 1),
                             (4, ph - n, 2, (7 << fb) + 3), (0, 0, -far + 1, -far + 3), (pw - n, ph - n, far + 3, far + 1),
                             (0, ph - n, -(3 << fb), (4 << fb)), (pw - n, 0, (9 << fb) + nph - 1, -(9 << fb) - 1)):
        out.append((bx, by, mx, my, -my, mx))
        out.append((bx, by, my, -mx, mx, my))
    return np.array(out, dtype=np.int16)


def _model(cases, r0, r1, n, d, chroma, bd, wset):
    ww, wo, ww1, wo1, wb = wset[:5]
    out = np.empty((len(cases), n * n), np.uint16)
    for i, (bx, by, m0x, m0y, m1x, m1y) in enumerate(cases.tolist()):
        if wb:
            p = wm.predict(r0, r1, bx, by, n, n, d, (m0x, m0y), (m1x, m1y), chroma, bd, (ww, wo) if ww else None,
                           (ww1, wo1) if ww1 else None)
        elif ww and d != wm.DIR_BI:   # the default instances: one weight for the uni-directional block
            src, mv = (r0, (m0x, m0y)) if d == wm.DIR_L0 else (r1, (m1x, m1y))
            p = wm.weight_explicit(wm.interp(src, bx, by, n, n, mv[0], mv[1], chroma, bd), ww, wo, None, 0, 0, bd)
        else:
            p = wm.predict(r0, r1, bx, by, n, n, d, (m0x, m0y), (m1x, m1y), chroma, bd)
        out[i] = p.reshape(-1)
    return out


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("nt", [8, 4])
def test_mc_probe_equals_model(nt, bd):
    import torch

    from govideocompressor_amd.ops import native
    hip = native.hip()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev).cuda_stream
    chroma = nt == 4
    planes = _planes(bd, chroma)
    d_planes = [tuple(torch.from_numpy(p.view(np.int16)).to(dev) for p in pair) for pair in planes]
    ph, pw = planes[0][0].shape
    seen_weighted_diff = False
    for n in ((4, 8, 16) if chroma else (8, 16, 32)):
        cases = _cases(chroma, n)
        d_cases = torch.from_numpy(cases).to(dev)
        d_out = torch.empty((len(cases), n * n), dtype=torch.int16, device=dev)
        for d in (wm.DIR_L0, wm.DIR_L1, wm.DIR_BI):
            plain = None
            for wset in WEIGHTS:
                ww, wo, ww1, wo1, wb, pp, lean = wset
                d_out.fill_(-1)
                hip.hevc_mc_probe(len(cases), d_planes[pp][0].data_ptr(), d_planes[pp][1].data_ptr(), pw, ph,
                                  d_cases.data_ptr(), d_out.data_ptr(), nt, n, d, bd, ww, wo, ww1, wo1, wb, lean, stream)
                torch.cuda.synchronize(dev)
                got = d_out.cpu().numpy().view(np.uint16)
                want = _model(cases, planes[pp][0], planes[pp][1], n, d, chroma, bd, wset)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, (n, d, wset, bad[:6].tolist(), cases[bad[0]].tolist(),
                                       got[bad[0]][:8].tolist(), want[bad[0]][:8].tolist())
                if pp == 0 and not (ww or ww1):
                    plain = want
                elif pp == 0 and plain is not None and not np.array_equal(want, plain):
                    seen_weighted_diff = True
    assert seen_weighted_diff   # the weights change the prediction: the comparison is not vacuous


def test_mc_probe_refuses_parameters_outside_its_domain():
    import torch

    from govideocompressor_amd.ops import native
    hip = native.hip()
    t = torch.zeros(4096, dtype=torch.int16, device="cuda")
    ok = dict(ncase=1, ref0=t.data_ptr(), ref1=t.data_ptr(), pw=48, ph=40, cases=t.data_ptr(), out=t.data_ptr(), nt=8,
              n=16, dir=3, bd=8, ww=96, wo=-20, ww1=64, wo1=0, wb=1, lean=1, stream=0)
    for bad in (dict(n=64), dict(n=4), dict(nt=4, n=32), dict(nt=6), dict(dir=0), dict(dir=4), dict(bd=9), dict(ww=128),
                dict(ww1=-1), dict(wo=128), dict(wo1=-129), dict(wb=0), dict(ncase=0), dict(pw=0), dict(ref1=0)):
        with pytest.raises(ValueError):
            hip.hevc_mc_probe(**{**ok, **bad})


def test_wp_ref8_equals_the_model():
    """Three slots with their own weights, one of them identity (a slot read with its neighbour's
    weights fails); 300 words per slot: a multiple of 4 bytes but not of a block's 256 words."""
    import torch

    from govideocompressor_amd.ops import native
    hip = native.hip()
    B, nbytes = 3, 1200
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (B, nbytes), dtype=np.uint8)
    src[:, :256] = np.arange(256, dtype=np.uint8)        # every byte value in every slot
    wts = np.array([[96, -20], [64, 0], [40, 33]], dtype=np.int32)
    d_src, d_wt = torch.from_numpy(src).cuda(), torch.from_numpy(wts).cuda()
    guard = torch.full((B * nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = guard[:B * nbytes].view(B, nbytes)
    hip.wp_ref8(d_src.data_ptr(), out.data_ptr(), d_wt.data_ptr(), B, nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], wm.wp_ref8(src[b], int(wts[b, 0]), int(wts[b, 1]))), b
    assert np.array_equal(got[1], src[1])
    assert bool((guard[B * nbytes:] == 0xA5).all())      # nothing written past the last slot
    for bad in (nbytes - 2, 0):
        with pytest.raises(ValueError):
            hip.wp_ref8(d_src.data_ptr(), out.data_ptr(), d_wt.data_ptr(), B, bad, 0)
    with pytest.raises(ValueError):
        hip.wp_ref8(d_src.data_ptr(), out.data_ptr(), d_wt.data_ptr(), 0, nbytes, 0)

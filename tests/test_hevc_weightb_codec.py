"""x265 --weightb in the host writer, against the independent CPU decoder and the numpy model.

An I, P, B GOP from random records (utils/hevc_synth.py) whose B slice carries planted explicit
weights and no residual: the decoder's B picture must equal tests/ref_models_hevc_wp.py applied
to the decoder's own reference pictures, sample for sample.  That pins the slice header syntax
(weighted_bipred_flag, the two-list pred_weight_table) and validates the model against the
decoder before any GPU is involved (tests/test_gpu_hevc_wp_model.py then holds the kernels to it).
"""
import numpy as np
import pytest

import ref_models_hevc_wp as wm

from govideocompressor_amd.utils.hevc_synth import _cu_list, random_gop_stream, random_records

W0 = [96, -20, 70, 5, 50, -7]      # (w, o) of Y, Cb, Cr: every component its own row
W1 = [40, 33, 90, -12, 127, -128]
CASES = {"l0": dict(wp=W0), "l1": dict(wp1=W1), "both": dict(wp=W0, wp1=W1)}


def _model_b_picture(recs, ref0, ref1, bd, wts):
    """The B picture's three planes from its CU records and the two decoded references."""
    ctu, cu = recs[0], recs[1]
    H, W = ref0["y"].shape
    out = [np.zeros((H, W), np.uint16), np.zeros((H // 2, W // 2), np.uint16), np.zeros((H // 2, W // 2), np.uint16)]
    seen = {"dirs": set(), "int": 0, "frac": 0, "outside": 0}
    wc = W // 32
    for i in range(len(ctu)):
        rx, ry = i % wc, i // wc
        for (x, y, n) in _cu_list(int(ctu[i, 0])):
            gx, gy = x // 8, y // 8
            z = (gx & 1) | ((gy & 1) << 1) | ((gx & 2) << 1) | ((gy & 2) << 2)
            rec = cu[i * 16 + z]
            assert rec[0] == 1, "the B picture of this test holds inter CUs only"
            d = int(rec[12]) or 1
            mv0 = [int(t) for t in rec[4:8].view(np.int16)]
            mv1 = [int(t) for t in rec[8:12].view(np.int16)]
            X, Y = rx * 32 + x, ry * 32 + y
            seen["dirs"].add(d)
            for l, mv in ((1, mv0), (2, mv1)):
                if d & l:
                    seen["int" if (mv[0] % 4 == 0 and mv[1] % 4 == 0) else "frac"] += 1
                    x0, y0 = X + (mv[0] >> 2) - 3, Y + (mv[1] >> 2) - 3
                    seen["outside"] += x0 < 0 or y0 < 0 or x0 + n + 7 > W or y0 + n + 7 > H
            for c, name in enumerate("yuv"):
                s = 2 if c else 1
                wp0 = tuple(wts["wp"][2 * c:2 * c + 2]) if "wp" in wts else None
                wp1 = tuple(wts["wp1"][2 * c:2 * c + 2]) if "wp1" in wts else None
                p = wm.predict(ref0[name], ref1[name], X // s, Y // s, n // s, n // s, d, mv0, mv1, c > 0, bd, wp0, wp1)
                out[c][Y // s:(Y + n) // s, X // s:(X + n) // s] = p
    return out, seen


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("which", ["l0", "l1", "both"])
@pytest.mark.parametrize("w,h,seed", [(64, 64, 1), (96, 64, 2)])
def test_weighted_b_slice_decodes_to_the_model(host, w, h, seed, which, bd):
    wts = CASES[which]
    s, recs = random_gop_stream(host, w, h, 3, bframes=1, seed=seed, bit_depth=bd, tmvp=True, intra_in_p=0.0,
                                density=0.02, sao=False, host_cfg=dict(weightb=1, weightp=1, sao=0, deblock=0),
                                weights={1: wts}, b_residual=False, force_split=1 | (seed << 1))
    pics = host.hevc_decode(s, True)
    assert [p["slice_type"] for p in pics] == [2, 0, 1]
    want, seen = _model_b_picture(recs[1], pics[0], pics[2], bd, wts)
    # coverage: CUs of all three directions, integer and fractional vectors, windows past an edge
    assert seen["dirs"] == {1, 2, 3} and seen["int"] > 0 and seen["frac"] > 0 and seen["outside"] > 0, seen
    for c, name in enumerate("yuv"):
        assert np.array_equal(pics[1][name], want[c]), f"plane {name}: {np.argwhere(pics[1][name] != want[c])[:3].tolist()}"
    # the weights matter: the default prediction differs
    plain, _ = _model_b_picture(recs[1], pics[0], pics[2], bd, {})
    assert not np.array_equal(plain[0], want[0])


def test_unweighted_b_slice_of_a_weightb_stream_carries_the_table(host):
    """Flags 0 on both lists: the decoder must parse the (empty) table and predict by default."""
    s, recs = random_gop_stream(host, 64, 64, 3, bframes=1, seed=4, intra_in_p=0.0, density=0.02, sao=False,
                                host_cfg=dict(weightb=1, sao=0, deblock=0), b_residual=False)
    s0, _ = random_gop_stream(host, 64, 64, 3, bframes=1, seed=4, intra_in_p=0.0, density=0.02, sao=False,
                              host_cfg=dict(sao=0, deblock=0), b_residual=False)
    assert s != s0
    pics, pics0 = host.hevc_decode(s, True), host.hevc_decode(s0, True)
    want, _ = _model_b_picture(recs[1], pics[0], pics[2], 8, {})
    for c, name in enumerate("yuv"):
        assert np.array_equal(pics[1][name], want[c]) and np.array_equal(pics0[1][name], want[c])


def test_weightb_off_keeps_the_bytes(host):
    """weightb=0 in the config and no config key at all write the same B GOP."""
    kw = dict(bframes=3, seed=7, mv_pool=3, intra_in_p=0.05, density=0.02, pyramid=True)
    a, _ = random_gop_stream(host, 128, 96, 9, host_cfg=dict(max_merge=3, wpp=1, weightb=0), **kw)
    b, _ = random_gop_stream(host, 128, 96, 9, host_cfg=dict(max_merge=3, wpp=1), **kw)
    assert a == b
    assert host.hevc_parameter_sets(dict(width=128, height=96, bframes=3, weightb=0)) == \
        host.hevc_parameter_sets(dict(width=128, height=96, bframes=3))
    assert host.hevc_parameter_sets(dict(width=128, height=96, bframes=3, weightb=1)) != \
        host.hevc_parameter_sets(dict(width=128, height=96, bframes=3))


def test_writer_refuses_misplaced_weights(host):
    rng = np.random.default_rng(0)
    rb = random_records(rng, 64, 64, pslice=True, bslice=True, sao=False)
    rp = random_records(rng, 64, 64, pslice=True, sao=False)
    bfp = dict(idr=0, poc=1, qp=30, slice_type=0, ref_poc0=0, ref_poc1=2, nal_ref=0)
    on, off = dict(width=64, height=64, bframes=1, weightb=1, weightp=1), dict(width=64, height=64, bframes=1, weightp=1)
    host.hevc_write_slice(on, dict(bfp, wp=W0, wp1=W1), *rb)            # fine
    with pytest.raises(RuntimeError, match="wp1"):                      # list-1 weights in a P slice
        host.hevc_write_slice(on, dict(idr=0, poc=1, qp=30, slice_type=1, wp1=W1), *rp)
    with pytest.raises(RuntimeError, match="weightb"):                  # B weights without the PPS flag
        host.hevc_write_slice(off, dict(bfp, wp=W0), *rb)
    with pytest.raises(RuntimeError, match="weightb"):
        host.hevc_write_slice(off, dict(bfp, wp1=W1), *rb)
    for bad in ([192, 0, 64, 0, 64, 0], [64, 128, 64, 0, 64, 0], [64, 0, 64, 0, -65, 0], [64, 0, 64, 0]):
        with pytest.raises(RuntimeError, match="wp1"):                  # the range checks of wp
            host.hevc_write_slice(on, dict(bfp, wp1=bad), *rb)

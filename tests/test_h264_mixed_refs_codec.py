"""P macroblocks whose 8x8 partitions differ in reference, through the host CABAC writer and the
CPU decoder: hand-built records, the decoder's motion (vectors of every 4x4 block, and the
parsed records' kinds, references and vectors) must equal them.

The mixed-reference decision (csrc/kernels/h264_p_mixed.hip) writes such records; everything
after the record -- ref_idx per partition, the refIdx rules of the vector prediction (8.4.1.3:
a single neighbour on the partition's reference gives its vector, the directional rules of
16x8 / 8x16 apply only on a matching reference) -- is the shared coder's, pinned here without a
GPU.  Stream: I, then P pictures that fill the reference list, then the picture under test.
"""
import numpy as np
import pytest

from govideocompressor_amd.utils.h264_synth import HDR_BYTES, P8x8, P8x16, P16x8, P16x16, PSKIP, _intra_record

_KIND, _QP, _REF, _MV = 0, 2, 8, 16
W = H = 48  # 3 x 3 MBs
WMB, NMB = 3, 9


def _blank():
    hdr = np.zeros((NMB, HDR_BYTES), np.uint8)
    hdr[:, _REF:_REF + 8] = 0xFF
    return hdr, np.zeros((NMB, 408), np.int16)


def _put(hdr, mb, kind, refs, mvs, qp=28):
    hdr[mb, _KIND], hdr[mb, _QP] = kind, qp
    hdr[mb, _REF:_REF + 4] = np.asarray(refs, np.uint8)
    hdr[mb, _MV:_MV + 16] = np.frombuffer(np.asarray(mvs, np.int16).reshape(4, 2).tobytes(), np.uint8)


def _stream(host, nref, test_hdr):
    """I + nref P pictures (zero motion, reference 0) + the picture under test -> bytes"""
    rng = np.random.default_rng(9)
    cfg = dict(width=W, height=H, qp=28, cabac=1, refs=nref)
    out = [host.parameter_sets(cfg)]
    hdr, coef = _blank()
    for mb in range(NMB):
        _intra_record(rng, hdr[mb], coef[mb], mb % WMB, mb // WMB, 28, 0.1)
    out.append(host.write_slice(cfg, dict(idr=1, qp=28, frame_num=0), hdr, coef)[0])
    for t in range(1, nref):
        hdr, coef = _blank()
        for mb in range(NMB):
            _put(hdr, mb, P16x16, [0] * 4, [[4 * t, -4]] * 4)
        out.append(host.write_slice(cfg, dict(idr=0, qp=28, frame_num=t, num_ref_l0=min(t, nref)), hdr, coef)[0])
    _, coef = _blank()
    out.append(host.write_slice(cfg, dict(idr=0, qp=28, frame_num=nref, num_ref_l0=nref), test_hdr, coef)[0])
    return b"".join(out)


def _check(host, nref, hdr):
    s = _stream(host, nref, hdr)
    seg = host.parse([s], 1)[0]
    assert seg["error"] is None
    got = seg["hdr"][nref]
    pic = host.decode(s)[nref]
    dec_mv = np.asarray(pic["mv"]).reshape(NMB, 16, 2)
    for mb in range(NMB):
        want_mv = np.frombuffer(hdr[mb, _MV:_MV + 16].tobytes(), np.int16).reshape(4, 2)
        for blk in range(16):
            q = (blk // 4 // 2) * 2 + (blk % 4) // 2
            assert tuple(dec_mv[mb, blk]) == tuple(want_mv[q]), (mb, blk)
        if got[mb, _KIND] == PSKIP:  # the writer's own shorthand for an MB at the skip predictor on reference 0
            assert hdr[mb, _KIND] == P16x16 and not hdr[mb, _REF:_REF + 4].any()
        else:
            assert got[mb, _KIND] == hdr[mb, _KIND], mb
        assert np.array_equal(got[mb, _REF:_REF + 4], hdr[mb, _REF:_REF + 4]), mb
        assert np.array_equal(got[mb, _MV:_MV + 16], hdr[mb, _MV:_MV + 16]), mb
    return got


def _background(rng, nref):
    hdr, _ = _blank()
    for mb in range(NMB):
        r = int(rng.integers(0, nref))
        _put(hdr, mb, P16x16, [r] * 4, [list(rng.integers(-24, 25, 2))] * 4)
    return hdr


@pytest.mark.parametrize("seed", [1, 2])
def test_p8x8_with_four_different_references(host, seed):
    rng = np.random.default_rng(seed)
    hdr = _background(rng, 4)
    for mb, refs in ((4, [0, 1, 2, 3]), (5, [3, 2, 1, 0]), (0, [1, 0, 1, 0]), (8, [2, 2, 0, 1])):
        _put(hdr, mb, P8x8, refs, rng.integers(-30, 31, size=(4, 2)))
    # equal vectors in every quadrant: only the references make it P_8x8
    _put(hdr, 7, P8x8, [0, 1, 1, 0], [[6, -2]] * 4)
    _check(host, 4, hdr)


@pytest.mark.parametrize("seed", [3, 4])
def test_halves_that_differ_only_in_reference(host, seed):
    """P_16x8 / P_8x16 with one vector and two references: the directional predictor (B for the top
    half, A for the bottom; A for the left, C for the right) holds only on a matching reference"""
    rng = np.random.default_rng(seed)
    hdr = _background(rng, 3)
    v = [list(rng.integers(-20, 21, 2))] * 4
    _put(hdr, 4, P16x8, [0, 0, 1, 1], v)
    _put(hdr, 5, P8x16, [2, 0, 2, 0], v)
    _put(hdr, 1, P16x8, [1, 1, 0, 0], v)
    _put(hdr, 3, P8x16, [0, 1, 0, 1], v)
    _put(hdr, 8, P16x8, [2, 2, 1, 1], [[8, 8], [8, 8], [-12, 4], [-12, 4]])
    _check(host, 3, hdr)


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_exactly_one_neighbour_shares_the_reference(host, which):
    """MB 4 (centre) on reference 2; of A (MB 3), B (MB 1) and C (MB 2) exactly one is on reference
    2, with a vector far from the median of the three: the predictor is that neighbour's vector"""
    hdr = _background(np.random.default_rng(5), 1)
    vec = {"A": [36, -20], "B": [-40, 28], "C": [12, 44]}
    for name, mb in (("A", 3), ("B", 1), ("C", 2)):
        _put(hdr, mb, P16x16, [2 if name == which else (0 if name == "A" else 1)] * 4, [vec[name]] * 4)
    cur = [vec[which][0] + 1, vec[which][1] - 2]
    _put(hdr, 4, P16x16, [2] * 4, [cur] * 4)
    _check(host, 3, hdr)
    # the same inside an MB: quadrant 3 of a P_8x8 whose quadrants 1 (B) and 2 (A) are on other references
    _put(hdr, 4, P8x8, [2, 0, 1, 2], [vec[which], [-28, -28], [30, 30], [vec[which][0] + 3, vec[which][1] + 1]])
    _check(host, 3, hdr)

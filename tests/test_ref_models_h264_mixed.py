"""The numpy model of ``p_mixed_refs`` (tests/ref_models_h264_mixed.py) on cases worked by hand.

One macroblock, flat pictures, so every SATD is known without a transform: a flat difference d
over a 4x4 block has the one coefficient 16 d, SATD 8 |d|, and an 8x8 quadrant 32 |d|.  The source
is 80 on its left half and 120 on its right; picture 0 is flat 120 (matches the right quadrants),
picture 1 flat 80 (matches the left ones), so a quadrant on the wrong picture costs 32 * 40 = 1280.
On flat pictures every vector predicts the same, so the vector bits alone order the candidates.
QP 30: lambda 8.  overhead 8, min_satd 2000, all vectors and the predictor zero unless said.
"""
import numpy as np
import pytest

import ref_models_h264_mixed as mx

L = 8  # lambda at QP 30
KNO = mx.KNO


def _case(src_l=80, src_r=120, pics=(120, 80, 200), cost=3000, xcost=(3000, KNO), nref=3, n0=3, pm=(0, 0),
          xmv=((0, 0), (0, 0)), scale=(512, 768), min_satd=2000, kind=0, mv8=None):
    src = np.empty((1, 16, 16), dtype=np.uint8)
    src[:, :, :8], src[:, :, 8:] = src_l, src_r
    pool = np.stack([np.full((16, 16), v, dtype=np.uint8) for v in pics])[None]
    a = dict(mv=np.zeros((1, 1, 2), np.int16),
             mv8=np.zeros((1, 1, 4, 2), np.int16) if mv8 is None else np.array(mv8, np.int16).reshape(1, 1, 4, 2),
             cost=np.array([[cost]], np.int32), pred=np.full((1, 1, 256), 7, np.uint8),
             xmv=np.array(xmv, np.int16).reshape(2, 1, 1, 2), xcost=np.array(xcost, np.int32).reshape(2, 1, 1),
             xpred=np.stack([np.full((1, 1, 256), 11, np.uint8), np.full((1, 1, 256), 12, np.uint8)]),
             mref=np.full((1, 1), 99, np.int8), mref4=np.full((1, 1, 4), 99, np.int8))
    lam = np.zeros(52, dtype=np.int32)
    lam[30] = L
    out = mx.p_mixed_refs(lam, 1, 1, nref, [kind], [n0], [[0, 1, 2, -1]], np.array([30]), None, a["mv"], a["mv8"], a["cost"],
                          a["pred"], a["xmv"], a["xcost"], a["xpred"], a["mref"], a["mref4"], src, src, pool,
                          np.array(pm, np.int16).reshape(1, 1, 2), np.array(scale, np.int16).reshape(2, 1), 8, min_satd)
    return a, out


def test_mixed_wins_by_the_hand_computed_margin():
    # (a) 3000 + L = 3008.  (c): left quadrants on picture 1, SATD 0 + L * (1 + 1 + 3) = 40 (on picture 0:
    # 1280 + 24); right quadrants on picture 0, 0 + L * (1 + 1 + 1) = 24 (on picture 1: 1280 + 40);
    # MB: 40 + 24 + 40 + 24 + 8 L = 192.  Margin 3008 - 192 = 2816.
    a, o = _case()
    assert o["winner"][0, 0] == 3
    assert o["mref4"][0, 0].tolist() == [1, 0, 1, 0] and o["mref"][0, 0] == 1
    assert not o["mv8"].any() and not o["mv"].any()
    assert o["cost"][0, 0] == 3000 + 192 - 3008
    p = o["pred"][0, 0].reshape(16, 16)
    assert (p[:, :8] == 80).all() and (p[:, 8:] == 7).all()  # the quadrants left on picture 0 keep their prediction


def test_tie_between_c_and_a_keeps_a():
    a, o = _case(cost=192 - L)  # (a) = 192 = (c)
    assert o["winner"][0, 0] == 1 and o["mref4"][0, 0].tolist() == [0] * 4 and o["mref"][0, 0] == 0
    for k in ("mv", "mv8", "cost", "pred"):
        assert np.array_equal(o[k], a[k])
    assert _case(cost=192 - L + 1)[1]["winner"][0, 0] == 3  # one more and (c) is strictly cheaper


def test_tie_between_b_and_c_keeps_b():
    a, o = _case(xcost=(192 - 3 * L, KNO), xmv=((4, -8), (0, 0)))  # (b) = 168 + 3 L = 192 = (c), (a) = 3008
    # ((c)'s picture-1 quadrants now start from xmv = (4, -8): the zero candidate is cheaper in bits, same 40)
    assert o["winner"][0, 0] == 2 and o["mref"][0, 0] == 1 and o["mref4"][0, 0].tolist() == [1] * 4
    assert o["mv"][0, 0].tolist() == [4, -8] and (o["mv8"][0, 0] == [4, -8]).all()
    assert o["cost"][0, 0] == 168 and (o["pred"] == 11).all()
    assert _case(xcost=(192 - 3 * L + 1, KNO), xmv=((4, -8), (0, 0)))[1]["winner"][0, 0] == 3


def test_four_quadrants_on_one_farther_picture_are_not_mixed():
    # source flat 80: every quadrant takes picture 1 at (0, 0), 4 * 40 + 64 = 224 < (a) = 3008 -- yet
    # that is candidate (b)'s shape, and (b) at 3000 + 24 loses to (a)
    a, o = _case(src_r=80)
    assert o["winner"][0, 0] == 1 and o["mref4"][0, 0].tolist() == [0] * 4
    for k in ("mv", "mv8", "cost", "pred"):
        assert np.array_equal(o[k], a[k])


def test_four_quadrants_on_reference_zero_are_not_mixed():
    # the source is picture 0 everywhere and picture 1 (searched) matches nothing: every quadrant stays on
    # reference 0 with its own vector, 3 L + 9 L + 3 L + 3 L + 8 L = 208 < (a) = 3008 -- but a split on
    # reference 0 alone is p_part8x8's choice, priced there against another predictor: (a) stays
    a, o = _case(src_l=120, pics=(120, 200, 200), mv8=((0, 0), (4, 0), (0, 0), (0, 0)), min_satd=-1)
    assert mx.se_bits(4) == 7
    assert o["winner"][0, 0] == 1 and o["mref4"][0, 0].tolist() == [0] * 4
    for k in ("mv", "mv8", "cost", "pred"):
        assert np.array_equal(o[k], a[k])


def test_unsearched_picture_is_never_chosen():
    # picture 2 matches the left half exactly but was not searched; picture 1 (searched) matches nothing
    a, o = _case(pics=(120, 200, 80), xcost=(3000, KNO))
    assert o["winner"][0, 0] == 1 and not (o["mref4"] == 2).any()
    # searched, it takes the left quadrants: 2 * L * (1 + 1 + 4) + 2 * 24 + 64 = 208
    a, o = _case(pics=(120, 200, 80), xcost=(3000, 3000))
    assert o["winner"][0, 0] == 3 and o["mref4"][0, 0].tolist() == [2, 0, 2, 0]
    assert o["cost"][0, 0] == 3000 + 208 - 3008
    # a slot with two active pictures never looks at picture 2, whatever its cost says
    a, o = _case(pics=(120, 200, 80), xcost=(3000, 3000), n0=2)
    assert o["winner"][0, 0] == 1 and not (o["mref4"] == 2).any()


def test_below_min_satd_and_other_slots():
    a, o = _case(min_satd=2560)  # the list-0[0] SATD is 1280 + 0 + 1280 + 0: at the threshold, not priced
    assert o["winner"][0, 0] == 1
    assert _case(min_satd=2559)[1]["winner"][0, 0] == 3
    a, o = _case(kind=2)         # an I slot: untouched, sentinels included
    assert o["winner"][0, 0] == 0 and (o["mref"] == 99).all() and (o["mref4"] == 99).all()
    a, o = _case(n0=1)           # one active picture: reference 0, nothing else moves
    assert o["winner"][0, 0] == 1 and (o["mref"] == 0).all() and (o["mref4"] == 0).all()
    assert np.array_equal(o["cost"], a["cost"]) and np.array_equal(o["pred"], a["pred"])


def test_distance_scale_rounds_half_up_for_both_signs():
    assert mx.scale_mv(256, 37, *mx.MVX) == 37 and mx.scale_mv(256, -37, *mx.MVX) == -37
    assert mx.scale_mv(512, 3, *mx.MVX) == 6 and mx.scale_mv(512, -3, *mx.MVX) == -6
    assert mx.scale_mv(384, 5, *mx.MVX) == 8       # 7.5 -> 8
    assert mx.scale_mv(384, -5, *mx.MVX) == -7     # -7.5 -> -7: floor(x + 1/2), not away from zero
    assert mx.scale_mv(128, 1, *mx.MVX) == 1 and mx.scale_mv(128, -1, *mx.MVX) == 0
    assert mx.scale_mv(768, 2000, *mx.MVX) == 2047 and mx.scale_mv(768, -2000, *mx.MVX) == -2048
    assert mx.scale_mv(768, 400, *mx.MVY) == 511 and mx.scale_mv(768, -400, *mx.MVY) == -512


def test_vector_at_the_clamp_stays_inside():
    # predictor (2000, 500) scaled by 2 clamps to (2047, 511) = xmv: zero mvd, and the ring positions
    # beyond the range clamp back onto it (equal price: not taken).  The picture-0 quadrants keep the
    # zero vector at L * (23 + 19 + 1) = 344 against the predictor.  (c) = 2 * 40 + 2 * 344 + 64 = 832.
    a, o = _case(pm=(2000, 500), xmv=((2047, 511), (0, 0)))
    assert mx.se_bits(-2000) == 23 and mx.se_bits(-500) == 19
    assert o["winner"][0, 0] == 3 and o["mref4"][0, 0].tolist() == [1, 0, 1, 0]
    assert o["mv8"][0, 0].tolist() == [[2047, 511], [0, 0], [2047, 511], [0, 0]]
    assert o["cost"][0, 0] == 3000 + 832 - 3008
    # the same at the negative corner
    a, o = _case(pm=(-2000, -500), xmv=((-2048, -512), (0, 0)))
    assert o["mv8"][0, 0].tolist() == [[-2048, -512], [0, 0], [-2048, -512], [0, 0]]


@pytest.mark.parametrize("mv", [(0, 0), (5, -3), (-2046, 509), (2047, -512), (-9, 510)])
def test_fetch_equals_edge_extension(mv):
    """Pic.block (coordinates clamped like the kernels') against Planes.block (an edge-extended array)
    where the latter reaches, and far outside against the block at the last vector it reaches."""
    from ref_models_me import Planes
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 256, size=(32, 48)).astype(np.uint8)
    pic, pl = mx.Pic(ref), Planes(ref)
    near = (max(-600, min(600, mv[0])), max(-500, min(500, mv[1])))
    for x0, y0 in ((0, 0), (40, 24), (16, 8)):
        assert np.array_equal(pic.block(x0, y0, *near), pl.block(x0, y0, *near)[:8, :8])
    far = pic.block(8, 8, *mv)
    assert far.shape == (8, 8) and far.min() >= 0 and far.max() <= 255

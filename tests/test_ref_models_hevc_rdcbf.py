"""The numpy model of the rate-distortion check of inter residuals against none
(tests/ref_models_hevc_rdcbf.py) on cases computed by hand.

The block cases are flat 4x4 residuals r at 8 bits.  A flat residual has only a DC coefficient:
the row stage gives (4 * 64 r) >> 1 = 128 r, the column stage (4 * 64 * 128 r + 128) >> 8 = 128 r.
At Qp' 28 (qscale 2^14, qbits 23) a level is r / 4 coefficient-wise, and level 1 dequantises to
(16 * 64 << 4 + 16) >> 5 = 512, the inverse columns give (64 * 512 + 64) >> 7 = 256 and the rows
(64 * 256 + 2048) >> 12 = 4: r = 4 is reconstructed exactly.  At Qp' 27 (qscale 18396, qbits 23) a
step is 2^23 / (128 * 18396) = 3.5625 residual units and the inter dead zone adds 85 / 512, so
r = 3 quantises to floor(0.842 + 0.166) = 1, which reconstructs to (16 * 57 << 4 + 16) >> 5 = 456,
(64 * 456 + 64) >> 7 = 228, (64 * 228 + 2048) >> 12 = 4: one above the residual.  The DC level 1
alone costs rate(1, False, 0) = SIG1 + SIGN + GT1_NO + LAST_BASE = 72, so the check clears when
256 (D0 - D1) <= lamq * (72 + 18 - 8) = 82 lamq.
"""
import functools

import numpy as np
import pytest

import ref_models_hevc_rdcbf as rc
import ref_models_hevc_rdoq as rq


@functools.lru_cache(maxsize=1)
def _dct32():
    from govideocompressor_amd.ops import native
    return np.asarray(native.host().table("hevc_dct32"), dtype=np.int64).reshape(32, 32)


def _levels(log2n, placed):
    """level block with placed = {diagonal coder scan position: level}"""
    order, _ = rq.positions(0, log2n)
    lev = np.zeros((1 << log2n, 1 << log2n), dtype=np.int64)
    for p, v in placed.items():
        x, y = order[p]
        lev[y, x] = v
    return lev


def test_constants():
    assert (rc.CBF0, rc.CBF1) == (8, 18) == (rq.CSBF0, rq.CSBF1)


@pytest.mark.parametrize("sign", [1, -1])
def test_single_one_at_the_last_position_of_a_4x4(sign):
    # rate(1, False, 15) = 22 + 16 + 10 + 24 + 20 * floor(log2(16)) = 152 and the 15 zeros below it in
    # its group cost SIG0 = 9 each; a 4x4 TU has no group flags
    assert rc.tu_rate(_levels(2, {15: sign}), 2) == 152 + 135 == 287
    # alone at the first position it costs 72
    assert rc.tu_rate(_levels(2, {0: sign}), 2) == 72
    # the levels are kept only while 256 (D0 - D1) > lamq * (287 + 18 - 8) = 297 lamq
    assert rc.clears(397, 100, 287, 256) and rc.clears(397, 100, 287, 257)  # 76032 <= 76032: the tie clears
    assert not rc.clears(397, 100, 287, 255)


def test_no_levels_have_no_rate():
    for lg in (2, 3, 4, 5):
        assert rc.tu_rate(_levels(lg, {}), lg) == 0


def test_group_2_of_an_8x8_with_an_empty_group_1_prices_csbf0():
    # level 2 at p = 37 (group 2, q = 5), level -1 at p = 3 (group 0):
    #   pmax: rate(2, False, 37) = 22 + 16 + (24 + 11) + 24 + 20 * floor(log2(38)) = 197
    #   group 2 below pmax: 5 zeros * SIG0 = 45
    #   group 1 is empty: its zeros cost nothing, its flag CSBF0 = 8
    #   group 0: rate(1, True, 3) = 48 and 15 zeros * 9 = 135; group 0 and pmax's group have no flag
    assert rc.tu_rate(_levels(3, {37: 2, 3: -1}), 3) == 197 + 45 + 8 + 48 + 135 == 433
    # a level 1 at p = 20 fills group 1: CSBF1 = 18 instead of 8, 48 for the level, 15 zeros
    assert rc.tu_rate(_levels(3, {37: 2, 3: -1, 20: 1}), 3) == 433 - 8 + 18 + 48 + 135
    # group 0 empty too: its zeros cost nothing and it has no flag
    assert rc.tu_rate(_levels(3, {37: 2}), 3) == 197 + 45 + 8
    # pmax in group 3: groups 1 and 2 are both strictly between
    assert rc.tu_rate(_levels(3, {48: 1}), 3) == (22 + 16 + 10 + 24 + 20 * 5) + 8 + 8


def test_large_levels_and_a_32x32_last_position():
    # level 7 at p = 1023: 22 + 16 + (24 + 22 + 16 * (5 + 2 * 0)) + 24 + 20 * 10 = 388, 62 empty groups between
    assert rq.g_bits(7) == 126
    assert rc.tu_rate(_levels(5, {1023: -7}), 5) == 388 + 15 * 9 + 62 * 8


def test_exact_tie_clears():
    # lamq 256: 256 D0 + 256 * 8 <= 256 D1 + 256 (Rb + 18)  <=>  D0 - D1 <= Rb + 10
    assert rc.clears(1162, 1000, 152, 256)
    assert not rc.clears(1163, 1000, 152, 256)
    assert rc.clears(1 << 30, (1 << 30) - 10, 0, 256)  # 64-bit terms
    assert not rc.clears(1 << 30, 0, 1 << 15, 4781507)  # 2^38 = 2.75e11 > 4781507 * (2^15 + 10) = 1.57e11
    assert rc.clears(1 << 30, 0, 1 << 20, 4781507 // 16)


def test_flat_block_end_to_end():
    """r = 4 at Qp' 28: level 1 at the DC, D0 = 16 * 16 = 256, D1 = 0, Rb = 72; kept while
    65536 > 82 lamq, that is up to lamq 799"""
    pred = np.full((4, 4), 100, dtype=np.int64)
    src = pred + 4
    for lamq, keep in ((0, True), (799, True), (800, False), (5000, False)):
        lev, rec, flag, d0, d1, rb = rc.rd_cbf_tu(src, pred, _dct32(), 2, 8, 28, lamq)
        assert (d0, d1, rb) == (256, 0, 72)
        assert flag == int(keep)
        assert np.array_equal(lev, _levels(2, {0: 1} if keep else {}))
        assert np.array_equal(rec, src if keep else pred)
    # a block the quantiser empties is not examined: r = 1 is a quarter of a step
    lev, rec, flag, d0, d1, rb = rc.rd_cbf_tu(pred + 1, pred, _dct32(), 2, 8, 28, 0)
    assert not lev.any() and flag == 0 and (d0, d1, rb) == (16, 16, 0) and np.array_equal(rec, pred)


def test_flat_block_on_an_exact_tie():
    """r = 21 at Qp' 16 (qscale 2^14, qbits 21): the level is 128 * 21 * 2^14 >> 21 = 21, dequantised
    (16 * 64 * 21 << 2 + 16) >> 5 = 2688, inverse (64 * 2688 + 64) >> 7 = 1344, (64 * 1344 + 2048) >>
    12 = 21: exact.  D0 = 16 * 441 = 7056, D1 = 0, Rb = rate(21, False, 0) = 22 + 16 + (24 + 22 + 16 *
    (5 + 2 * 3)) + 24 = 284, and 256 * 7056 = 1806336 = 6144 * (284 + 10): the tie at lamq 6144 clears"""
    pred = np.full((4, 4), 100, dtype=np.int64)
    assert rq.g_bits(21) == 222
    for lamq, keep in ((6143, 1), (6144, 0), (6145, 0)):
        lev, rec, flag, d0, d1, rb = rc.rd_cbf_tu(pred + 21, pred, _dct32(), 2, 8, 16, lamq)
        assert (d0, d1, rb, flag) == (7056, 0, 284, keep)
        assert np.array_equal(rec, pred + 21 * keep) and int(np.abs(lev).sum()) == 21 * keep


@pytest.mark.parametrize("pred_v,src_v", [(252, 255), (3, 0)])
def test_clip_changes_d1(pred_v, src_v):
    """|r| = 3 at Qp' 27 reconstructs to 4 (-4 too: every shift floors from an exact half or
    below): pred + R' = 256 / -1 is clipped to the source sample, so D1 = 0, not 16.  D0 = 144:
    the levels are kept while 36864 > 82 lamq (up to 449); unclipped they would go from 400 on"""
    pred = np.full((4, 4), pred_v, dtype=np.int64)
    src = np.full((4, 4), src_v, dtype=np.int64)
    lev, rres, flag = rq.transform_quant_block(src - pred, _dct32(), 2, 8, 27, False)
    assert flag and np.array_equal(rres, np.full((4, 4), 4 if src_v > pred_v else -4))
    for lamq, keep in ((420, True), (449, True), (450, False)):
        lev, rec, flag, d0, d1, rb = rc.rd_cbf_tu(src, pred, _dct32(), 2, 8, 27, lamq)
        assert (d0, d1, rb) == (144, 0, 72) and flag == int(keep)
        assert np.array_equal(rec, src if keep else pred)
    # the same residual away from the range's ends: D1 = 16, cleared from lamq 400 on
    mid = np.full((4, 4), 100, dtype=np.int64)
    assert rc.rd_cbf_tu(mid + (src_v - pred_v), mid, _dct32(), 2, 8, 27, 420)[2:] == (0, 144, 16, 72)
    assert rc.rd_cbf_tu(mid + (src_v - pred_v), mid, _dct32(), 2, 8, 27, 399)[2:] == (1, 144, 16, 72)


def test_lamq_table():
    """0.57 * 16 * 2^((QpY - 12) / 3) = 0.57 at QpY 0, 9.12 * 10.0794 = 91.924 at 22 and
    9.12 * 8192 = 74711.04 at 51; 10 bits multiply by 16"""
    want = {
        (8, 0.5): (0, 46, 37356), (8, 1.0): (1, 92, 74711), (8, 4.0): (2, 368, 298844),
        (10, 0.5): (5, 735, 597688), (10, 1.0): (9, 1471, 1195377), (10, 4.0): (36, 5883, 4781507),
    }
    for (bd, lam), vals in want.items():
        t = rc.lamq_table(lam, bd)
        assert len(t) == 52 and (t[0], t[22], t[51]) == vals, (bd, lam)
        assert t == [rc.lamq_of(lam, q, bd) for q in range(52)]

"""Hand-worked pins of the transform skip decision's numpy model (tests/ref_models_hevc_tskip.py).

8-bit cases use Qp' 34 unless noted: qp % 6 = 4 (quantiser scale 16384, level scale 64),
qp // 6 = 5, so the quantiser step is 32 in sample units for a transform-skip block:
c = r << 5, qbits = 14 + 5 + 5 = 24, level = (|r| * 2^19 + (171 << 15)) >> 24 = (|r| + 10.69) // 32
(intra dead zone); a level l dequantises to d = (l * 1024 * 32 + 16) >> 5 = 1024 l and comes back as
r' = (1024 l * 128 + 2048) >> 12 = 32 l.  lamq of QpY 34 at tskip_lambda 1.0 is 1471.
"""
import numpy as np
import pytest

import ref_models_hevc_rdcbf as rc
import ref_models_hevc_rdoq as rq
import ref_models_hevc_tskip as ts


@pytest.fixture(scope="module")
def dct(host):
    return host.table("hevc_dct32")


def _tu(res, dct, bd=8, qp=34, lamq=1471, pred=None, intra=True, dst=True, scan=0, **kw):
    res = np.asarray(res, dtype=np.int64).reshape(4, 4)
    pred = np.full((4, 4), 1 << (bd - 1), dtype=np.int64) if pred is None else np.asarray(pred, dtype=np.int64).reshape(4, 4)
    out = ts.tskip_tu(pred + res, pred, dct, bd, qp, lamq, intra, dst, scan, **kw)
    return out, pred


def _impulse(a, y=1, x=1):
    r = np.zeros((4, 4), dtype=np.int64)
    r[y, x] = a
    return r


def test_lamq_is_the_rd_cbf_table():
    assert rc.lamq_table(1.0, 8)[34] == 1471 and rc.lamq_table(1.0, 8)[26] == 232
    assert ts.TSF == 16 and (ts.CBF0, ts.CBF1) == (8, 18)


def test_arithmetic_of_candidate_b():
    assert ts.ts_coef(np.array([[-3, 5]]), 8).tolist() == [[-96, 160]]
    assert ts.ts_coef(np.array([[-3, 5]]), 10).tolist() == [[-24, 40]]
    # 8.6.4.2 with transform_skip_flag: (d << 7 + 2^(19 - bd)) >> (20 - bd)
    assert ts.ts_inverse(np.array([1024, -1024, 15, -17]), 8).tolist() == [32, -32, 0, -1]
    assert ts.ts_inverse(np.array([1024, -1024, 3, -5]), 10).tolist() == [128, -128, 0, -1]
    assert ts.ts_residual(np.array([[1, -2]]), 8, 34).tolist() == [[32, -64]]


def test_lone_impulse_b_wins(dct):
    """r = 60 at (1, 1): B codes one level 2 ((60 + 10.69) // 32) -> r' = 64, D_B = 16; the DST spreads
    it over the block.  (1, 1) is diagonal scan position 4: R_B = rate(2, last at 4) + 4 zeros =
    (22 + 16 + 24 + 11 + 24 + 20 * 2) + 4 * 9 = 173."""
    (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(_impulse(60), dct)
    assert (tsf, cbf) == (1, 1)
    assert lev.tolist() == _impulse(2).tolist()
    assert (rec - pred).tolist() == _impulse(64).tolist()
    assert d_b == 16 and r_b == 173
    assert 256 * d_b + 1471 * (r_b + 34) < 256 * d_a + 1471 * (r_a + 34)
    assert np.count_nonzero(rq.transform_quant_block(_impulse(60), dct, 2, 8, 34, True, True)[0]) > 1


def test_flat_offset_a_wins(dct):
    """a flat +20 is one DC coefficient for the DCT and sixteen levels for B"""
    (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(np.full((4, 4), 40), dct, dst=False)
    assert (tsf, cbf) == (0, 1)
    assert np.count_nonzero(lev) == 1 and lev[0, 0] != 0
    assert r_b > r_a and d_b == 16 * 8 * 8       # B: sixteen levels 1 -> 32 each
    assert np.array_equal(rec - pred, rq.transform_quant_block(np.full((4, 4), 40), dct, 2, 8, 34, True, False)[1])


def test_exact_tie_keeps_a(dct):
    """r = 33 at (x 1, y 0), A without levels: D0 = 1089; B: level 1 -> 32, D_B = 1, R_B = (22 + 16 +
    10 + 24 + 20) + 2 * 9 = 110.  At lamq 2048: J_B = 256 + 2048 * 144 = 295168 = 256 * 1089 + 2048 * 8."""
    res = _impulse(33, 0, 1)
    (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(res, dct, lamq=2048)
    assert (d_a, r_a, d_b, r_b) == (1089, 0, 1, 110)
    assert 256 * d_b + 2048 * (r_b + 34) == 256 * d_a + 2048 * 8
    assert (tsf, cbf) == (0, 0) and not lev.any() and np.array_equal(rec, pred)
    (lev, rec, tsf, cbf, *_), _ = _tu(res, dct, lamq=2047)
    assert (tsf, cbf) == (1, 1) and lev[0, 1] == 1 and rec[0, 1] - pred[0, 1] == 32
    assert not ts.chooses_b(10, True, 5, 40, 5, 40, 100) and ts.chooses_b(10, True, 5, 41, 5, 40, 100)


def test_b_empty_keeps_a(dct):
    """|r| <= 21 quantises to nothing without a transform ((21 + 10.69) // 32 = 0), while the sum of
    sixteen such samples is a DC coefficient: A stands with its levels, B's terms read D0 and 0"""
    res = np.full((4, 4), 21)
    (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(res, dct, dst=False)
    assert (tsf, cbf) == (0, 1) and lev[0, 0] != 0
    assert (d_b, r_b) == (16 * 21 * 21, 0) and r_a > 0 and d_a < d_b
    # both empty
    (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(_impulse(3), dct)
    assert (tsf, cbf, d_a, d_b, r_a, r_b) == (0, 0, 9, 9, 0, 0) and np.array_equal(rec, pred)


def test_a_empty_against_b_uses_cbf0(dct):
    """impulse a at (1, 1), which the DST quantises to nothing: R_B = (22 + 16 + 10 + 24 + 40) + 4 * 9
    = 148, J_B = 256 (a - 32)^2 + 1471 * 182 against J_A = 256 a^2 + 1471 * 8: B from a = 32 on"""
    for a, want in ((30, 0), (31, 0), (32, 1), (38, 1)):
        (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(_impulse(a), dct)
        assert (d_a, r_a, d_b, r_b) == (a * a, 0, (a - 32) ** 2, 148)
        assert (256 * d_b + 1471 * 182 < 256 * a * a + 1471 * 8) == bool(want)
        assert (tsf, cbf) == (want, want)
    # with the flag costs on A's side instead (the branch for an A with levels) 30 would win too
    assert ts.chooses_b(900, True, 900, 0, 4, 148, 1471) and not ts.chooses_b(900, False, 900, 0, 4, 148, 1471)


@pytest.mark.parametrize("bd", [8, 10])
def test_clip_at_both_ends(dct, bd):
    """Qp' 22 + 6 (bd - 8): step 8 (32 at 10 bits).  A lone -6 / +6 (x 4 at 10 bits) codes level
    -1 / +1 -> -8 / +8, which leaves the sample range: D_B counts the clipped sample (lamq 1 lets
    the distortion decide: 256 * 0 + 182 against 256 * 36 k^2 + 8)"""
    maxv, k = (1 << bd) - 1, 1 << (bd - 8)
    qp = 22 + 6 * (bd - 8)
    lamq = 1
    for pv, sign, edge in ((maxv - 6 * k, 1, maxv), (6 * k, -1, 0)):
        pred = np.full((4, 4), pv)
        (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), _ = _tu(_impulse(sign * 6 * k), dct, bd=bd, qp=qp, lamq=lamq, pred=pred)
        assert ts.ts_residual(_impulse(sign), bd, qp)[1, 1] == sign * 8 * k
        assert d_b == 0 and (tsf, cbf) == (1, 1)           # unclipped it would be (2 k)^2
        assert rec[1, 1] == edge and rec.min() >= 0 and rec.max() <= maxv


def test_ten_bit_shift(dct):
    """10 bits at Qp' 46 (QpY 34): c = r << 3, qbits = 14 + 7 + 3 = 24, level = (|r| * 2^17 + (171 << 15))
    >> 24 = (|r| + 42.75) // 128; d = (l * 1024 * 128 + 64) >> 7 = 1024 l; r' = (1024 l * 128 + 512)
    >> 10 = 128 l: four times the 8-bit step, as four times the sample scale"""
    (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), pred = _tu(_impulse(240), dct, bd=10, qp=46, lamq=rc.lamq_table(1.0, 10)[34])
    assert rc.lamq_table(1.0, 10)[34] == 23533
    assert (tsf, cbf) == (1, 1) and lev.tolist() == _impulse(2).tolist()
    assert (rec - pred).tolist() == _impulse(256).tolist() and d_b == 16 * 16 and r_b == 173


def test_vertical_scan_rate_differs(dct):
    """a level at (x 1, y 0) is position 2 of the diagonal scan, 1 of the horizontal and 4 of the
    vertical one: R_B = 48 + 24 + 20 floor(log2(p + 1)) + 9 p"""
    res = _impulse(64, 0, 1)
    got = {}
    for scan in (0, 1, 2):
        (lev, rec, tsf, cbf, d_a, d_b, r_a, r_b), _ = _tu(res, dct, dst=False, scan=scan)
        assert tsf == 1 and lev.tolist() == _impulse(2, 0, 1).tolist() and d_b == 0
        got[scan] = r_b
    g2 = 24 + 11 - 10    # level 2 instead of 1: greater1 yes + greater2 no
    assert got == {0: 110 + g2, 1: 48 + 24 + 20 + 9 + g2, 2: 48 + 24 + 40 + 36 + g2}
    assert ts.tu_rate4(_impulse(2, 0, 1), 2) != ts.tu_rate4(_impulse(2, 0, 1), 0)


def test_sdh_and_rdoq_run_on_b_as_on_coefficients(dct):
    """the quantiser's options apply to B: its levels are the quantiser model's on r << (13 - bd)"""
    rng = np.random.default_rng(5)
    for sdh, rdoq in ((True, 0), (False, 1), (True, 2)):
        res = rng.integers(-90, 91, (4, 4)) * (rng.random((4, 4)) < 0.6)
        (lev, rec, tsf, cbf, *_), pred = _tu(res, dct, qp=22, lamq=rc.lamq_table(1.0, 8)[22], scan=2, sdh=sdh, rdoq=rdoq, lam=184)
        want = rq.quantise(ts.ts_coef(res, 8), 2, 8, 22, True, 2, sdh, rdoq, 184)
        if tsf:
            assert np.array_equal(lev, want) and np.array_equal(rec, np.clip(pred + ts.ts_residual(want, 8, 22), 0, 255))

"""The numpy models of tests/ref_models.py on cases small enough to compute by hand: the GPU
tests trust these models, so a slip in one of them must fail here, without a GPU."""
import numpy as np
import pytest

import ref_models as rm


def _mb(y, c=None):
    c = y if c is None else c
    return np.full((16, 16), y, np.uint8), np.full((8, 8), c, np.uint8), np.full((8, 8), c, np.uint8)


def test_flat_mb_has_no_energy_and_offset_minus_15():
    for level in (0, 1, 128, 200):
        assert rm.aq_energy(*_mb(level)) == 0
    # e = 0 counts as 1: 1.0397 * (0 - 14.427) = -14.9997... -> -15
    assert rm.aq_adj(0, 1.0) == pytest.approx(-1.0397 * 14.427, abs=1e-12)
    assert rm.aq_offset_h264(0, 1.0) == -15
    assert rm.aq_offset_h264(0, 0.5) == -7   # -7.49987
    assert rm.aq_offset_h264(np.array([0, 1]), 1.0).tolist() == [-15, -15]


def test_all_255_mb_matches_the_32_bit_unsigned_product():
    y, cb, cr = _mb(255)
    assert rm.aq_energy(y, cb, cr) == 0
    # the kernel's arithmetic: s = 65280, s * s = 4261478400 needs all 32 unsigned bits
    s, ss = np.uint32(256 * 255), np.uint32(256 * 255 * 255)
    assert int(s) * int(s) == 4261478400 > 2 ** 31
    with np.errstate(over="ignore"):
        assert int(ss - ((s * s) >> np.uint32(8))) == 0
        wrapped = int(np.int32(ss)) - (int(np.int32(s) * np.int32(s)) >> 8)  # what a signed product gives
    assert wrapped != 0


def test_checkerboard_mb():
    yy, xx = np.mgrid[0:16, 0:16]
    y = (((yy + xx) & 1) * 255).astype(np.uint8)
    c = y[:8, :8]
    # luma: s = 128 * 255 = 32640, ss = 128 * 65025 = 8323200, s^2 >> 8 = 4161600 -> 4161600
    # chroma: s = 8160, ss = 2080800, s^2 >> 6 = 1040400 -> 1040400 each
    assert rm.aq_energy(y, c, c) == 4161600 + 2 * 1040400 == 6242400
    # log2(6242400) = 22.57367; 1.0397 * (22.57367 - 14.427) = 8.4702
    assert rm.aq_adj(6242400, 1.0) == pytest.approx(8.4702, abs=1e-3)
    assert rm.aq_offset_h264(6242400, 1.0) == 8
    assert rm.aq_offset_h264(6242400, 1.0, extra=20.0) == 24      # clamp
    assert rm.aq_offset_h264(0, 1.0, extra=-20.0) == -24
    assert rm.aq_offset_h264(6242400, 1.0, extra=0.0298) == 8     # 8.4999
    assert rm.aq_offset_h264(6242400, 1.0, extra=1.03) == 10      # 9.5001
    assert rm.aq_offset_h264(0, 0.0, extra=np.array([0.5, 1.5, -2.5])).tolist() == [0, 2, -2]   # ties to even


def test_aq_energy_batched_equals_per_block():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 1024, (2, 32, 48), dtype=np.int64)
    u, v = rng.integers(0, 1024, (2, 2, 16, 24), dtype=np.int64)
    Y, U, V = rm.mb_blocks(y, u, v)
    e = rm.aq_energy(Y, U, V)
    assert e.shape == (2, 6)
    for b in range(2):
        for mb in range(6):
            my, mx = divmod(mb, 3)
            blk = y[b, my * 16:my * 16 + 16, mx * 16:mx * 16 + 16]
            want = int((blk * blk).sum()) - (int(blk.sum()) ** 2 >> 8)
            for p in (u, v):
                cb = p[b, my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]
                want += int((cb * cb).sum()) - (int(cb.sum()) ** 2 >> 6)
            assert e[b, mb] == want


def test_aq_ctb_hevc_clamps():
    e4 = np.array([[0, 0, 0, 0], [6242400] * 4, [1 << 14, 1 << 15, 1 << 14, 1 << 15]])
    # means at 8 bits: -14.9997, 8.4702, 1.0397 * (14.5 - 14.427) = 0.0759
    assert rm.aq_ctb_mean(e4, 8, 1.0) == pytest.approx([-14.9997, 8.4702, 0.0759], abs=1e-3)
    assert rm.aq_ctb_hevc(e4, 8, 1.0, None, 30).tolist() == [18, 38, 30]     # offset clamp -12
    assert rm.aq_ctb_hevc(e4, 8, 1.0, None, 4).tolist() == [0, 12, 4]        # QP clamp 0
    assert rm.aq_ctb_hevc(e4, 8, 1.0, None, 50).tolist() == [38, 51, 50]     # QP clamp 51
    # two more bits of depth: every block 1.0397 * 4 = 4.1588 lower
    assert rm.aq_ctb_mean(e4, 10, 1.0) == pytest.approx(np.array([-14.9997, 8.4702, 0.0759]) - 4.1588, abs=1e-3)
    assert rm.aq_ctb_hevc(e4, 10, 1.0, None, 30).tolist() == [18, 34, 26]
    # strength 0: the per-block table alone, averaged over the four blocks
    assert rm.aq_ctb_hevc(e4[:1], 8, 0.0, np.array([[1.0, 2.0, 3.0, 4.5]]), 30).tolist() == [33]   # 2.625


def test_wp_src_identity_and_rounding():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(rm.wp_src(b, 64, 0, 6), b)
    assert np.array_equal(rm.wp_src(b, 32, 0, 5), b)
    # w = 0 divides by 1; negative numerators round like positive ones (ties up)
    assert rm.wp_src(np.array([3]), 0, 0, 6)[0] == 192
    assert rm.wp_src(np.array([1, 2, 3]), 128, 2, 6).tolist() == [0, 0, 1]   # -0.5 -> 0, 0, 0.5 -> 1
    assert rm.wp_src(np.array([0, 200]), 64, 100, 6).tolist() == [0, 100]
    assert rm.wp_src(np.array([255]), 32, -10, 6)[0] == 255                 # clipped


@pytest.mark.parametrize("w,o,d", [(31, 5, 6), (63, -3, 6), (64, 17, 6), (65, -20, 6), (127, 10, 6), (40, 2, 5)])
def test_forward_weight_inverts_wp_src(w, o, d):
    one = 1 << d
    b = np.arange(256, dtype=np.int64)
    keep = ((b - o) * one / w >= 0) & ((b - o) * one / w <= 255)   # the inverse does not clip
    assert keep.sum() > 100
    back = rm.wp_forward(rm.wp_src(b[keep], w, o, d), w, o, d)
    # s' is off by at most half a level, which the weight scales by w / 2^d; the forward rounding
    # adds another half
    step = int(np.floor(0.5 * w / one + 0.5))
    assert np.abs(back - b[keep]).max() <= step


def test_wp_stats_any_integer_type():
    y = np.array([[[1, 2], [3, 4]], [[255, 255], [255, 255]]])
    u = np.array([[[5]], [[1023]]])
    v = np.array([[[7]], [[0]]])
    want = [[10, 30, 5, 25, 7, 49], [1020, 4 * 65025, 1023, 1023 * 1023, 0, 0]]
    for dt in (np.uint8, np.int16, np.uint16, np.int64):
        if dt == np.uint8:
            got = rm.wp_stats(y.astype(dt), (u % 256).astype(dt), v.astype(dt))
            w2 = [list(r) for r in want]
            w2[1][2], w2[1][3] = 255, 65025
            assert got.tolist() == w2
        else:
            assert rm.wp_stats(y.astype(dt), u.astype(dt), v.astype(dt)).tolist() == want


def test_sse_window_and_psnr_definitions():
    rng = np.random.default_rng(2)
    src = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((16, 32), (8, 16), (8, 16))]
    rec = [p.copy() for p in src]
    rec[0][0, 0] = src[0][0, 0] ^ 0xFF          # inside the window
    rec[0][15, 31] ^= 0xFF                      # outside (20 x 12)
    rec[1][5, 9] = (int(src[1][5, 9]) + 3) % 256
    rec[2][6, 0] ^= 0xFF                        # outside
    d0 = int(src[0][0, 0]) - int(rec[0][0, 0])
    d1 = int(src[1][5, 9]) - int(rec[1][5, 9])
    assert rm.sse_planes(src, rec, 20, 12).tolist() == [d0 * d0, d1 * d1, 0]
    # H.264: the mean of per-frame PSNRs; HEVC: the PSNR of the mean error
    assert rm.psnr_h264([0, 0], 100) == 100.0
    assert rm.psnr_hevc(0, 100, 8) == 99.0
    assert rm.psnr_h264([65025, 0], 100) == pytest.approx((20.0 + 100.0) / 2)
    assert rm.psnr_hevc(65025, 200, 8) == pytest.approx(10 * np.log10(200.0))
    assert rm.psnr_h264([100, 400], 100) == pytest.approx(10 * np.log10(65025.0) - 10 * np.log10(2.0), abs=1e-12)
    assert rm.psnr_hevc(500, 200, 8) == pytest.approx(10 * np.log10(65025.0 / 2.5))
    assert rm.psnr_hevc(1023 * 1023, 1, 10) == pytest.approx(0.0, abs=1e-12)


def test_ssim_of_identical_planes_is_the_window_count():
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    assert rm.ssim8(y, y, 50, 36) == 6 * 4      # whole windows only: 48 x 32
    assert rm.ssim8(y, y, 56, 40) == 7 * 5
    # one window by hand: a = 0 / 2 columns, b = its mirror: means 1, variances 1, covariance -1
    a = np.tile(np.array([0, 2] * 4, dtype=np.uint8), (8, 1))
    b = 2 - a
    want = ((2 + rm.SSIM_C1) * (-2 + rm.SSIM_C2)) / ((2 + rm.SSIM_C1) * (2 + rm.SSIM_C2))
    assert rm.ssim8(a, b, 8, 8) == pytest.approx(want, rel=1e-15)
    # the float32 evaluation stays close on ordinary content
    z = np.clip(y.astype(np.int64) + rng.integers(-9, 10, y.shape), 0, 255)
    d = rm.ssim8_windows(y, z, 56, 40, np.float32).astype(np.float64) - rm.ssim8_windows(y, z, 56, 40)
    assert np.abs(d).max() < 2e-4


# ------------------------------------------------------------------ HEVC SAO
@pytest.mark.parametrize("k", range(4))
def test_sao_edge_category_of_a_3x3_neighbourhood(k):
    """Centre 5 with the class's two neighbours set: both larger -> 1 (valley), one larger and
    one equal -> 2, one smaller and one equal -> 3, both smaller -> 4 (peak), otherwise none.
    Samples with a neighbour outside the picture have no category."""
    (ax, ay), (bx, by) = rm.SAO_EO_NEIGHBOURS[k]
    assert [(ax, ay), (bx, by)] == [[(-1, 0), (1, 0)], [(0, -1), (0, 1)], [(-1, -1), (1, 1)], [(1, -1), (-1, 1)]][k]
    for a, b, want in [(7, 7, 1), (7, 5, 2), (5, 9, 2), (5, 3, 3), (4, 5, 3), (3, 4, 4), (3, 7, 0), (9, 1, 0), (5, 5, 0)]:
        p = np.full((3, 3), 5)
        p[1 + ay, 1 + ax], p[1 + by, 1 + bx] = a, b
        cat = rm.sao_edge_category(p, k)
        assert cat[1, 1] == want
        assert cat[0, 0] == cat[0, 2] == cat[2, 0] == cat[2, 2] == 0          # picture corners
        if k != 0:
            assert cat[0, 1] == cat[2, 1] == 0      # top / bottom edge: only the horizontal class has both neighbours
        if k != 1:
            assert cat[1, 0] == cat[1, 2] == 0      # left / right edge: only the vertical class
    # an edge sample of the class that does have both neighbours: a peak on the top row, a valley in the left column
    p = np.full((3, 3), 5)
    p[0, 1], p[1, 0] = 9, 2
    assert rm.sao_edge_category(p, 0)[0, 1] == 4 and rm.sao_edge_category(p, 1)[1, 0] == 1


def _sao_4x4():
    deb = np.full((4, 4), 10)
    deb[1, 1], deb[1, 2] = 12, 8
    src = deb + 1
    src[1, 1], src[1, 2] = 9, 10     # differences -3 at the peak, +2 in the valley, +1 elsewhere
    flat = np.full((2, 2), 77)
    return (deb, flat, flat), (src, flat, flat)


def test_sao_stats_of_a_4x4_picture_by_hand():
    deb, src = _sao_4x4()
    s = rm.sao_stats(deb, src, 8, 0, 0, 32)      # the block reaches past the picture: only its inside counts
    # class 0: (1,1) is a peak, (2,1) a valley.  Class 1 adds (1,2) below the peak (cat 2) and (2,2) below
    # the valley (cat 3).  Class 2: (2,2) has the peak up-left (cat 2).  Class 3: (1,2) has the valley up-right (cat 3).
    assert s["eo_cnt"][0].tolist() == [[1, 0, 0, 1], [1, 1, 1, 1], [1, 1, 0, 1], [1, 0, 1, 1]]
    assert s["eo_sum"][0].tolist() == [[2, 0, 0, -3], [2, 1, 1, -3], [2, 1, 0, -3], [2, 0, 1, -3]]
    assert s["bo_cnt"][0].tolist() == [0, 16] + [0] * 30       # 8, 10, 12 >> 3 = 1
    assert s["bo_sum"][0].tolist() == [0, 14 - 3 + 2] + [0] * 30
    for c in (1, 2):
        assert not s["eo_cnt"][c].any() and not s["eo_sum"][c].any() and not s["bo_sum"][c].any()
        assert s["bo_cnt"][c].tolist() == [0] * 9 + [4] + [0] * 22      # 77 >> 3 = 9
    # the top-left 2x2 block: the peak's right neighbour lies in the next block and still counts
    q = rm.sao_stats(deb, src, 8, 0, 0, 2)
    assert q["eo_cnt"][0].tolist() == [[0, 0, 0, 1]] * 4 and q["eo_sum"][0].tolist() == [[0, 0, 0, -3]] * 4
    assert q["bo_cnt"][0][1] == 4 and q["bo_sum"][0][1] == 0 and q["bo_cnt"][1][9] == 1
    # the bottom-right 2x2 block
    r = rm.sao_stats(deb, src, 8, 2, 2, 2)
    assert r["eo_cnt"][0].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert r["bo_cnt"][0][1] == 4 and r["bo_sum"][0][1] == 4
    # 10 bits: the band is sample >> 5
    s10 = rm.sao_stats([p * 4 + 3 for p in deb], [p * 4 for p in src], 10, 0, 0, 4)
    assert s10["bo_cnt"][0][1] == 16 and s10["bo_sum"][0][1] == 4 * 13 - 3 * 16
    assert s10["eo_cnt"][0].tolist() == s["eo_cnt"][0].tolist()


def _empty_stats():
    return dict(eo_cnt=np.zeros((3, 4, 4), np.int64), eo_sum=np.zeros((3, 4, 4), np.int64),
                bo_cnt=np.zeros((3, 32), np.int64), bo_sum=np.zeros((3, 32), np.int64))


def test_sao_lambda_and_offset_range():
    assert rm.sao_lambda(12, 8) == 0.57
    assert rm.sao_lambda(15, 8) == pytest.approx(1.14, rel=1e-15)
    assert rm.sao_lambda(15, 10) == pytest.approx(1.14 * 16, rel=1e-15)
    assert [rm.sao_offset_max(bd) for bd in (8, 10, 12)] == [7, 31, 31]


def test_sao_band_window_wraps_31_to_0():
    s = _empty_stats()
    s["bo_cnt"][0, 31], s["bo_sum"][0, 31] = 100, 300       # mean 3: 900 - 1800 = -900
    s["bo_cnt"][0, 0], s["bo_sum"][0, 0] = 100, -200        # mean -2: 400 - 800 = -400
    s["bo_cnt"][0, 30], s["bo_sum"][0, 30] = 100, 100       # mean 1: 100 - 200 = -100
    s["bo_cnt"][0, 1], s["bo_sum"][0, 1] = 100, -100        # mean -1: -100
    s["bo_cnt"][0, 5], s["bo_sum"][0, 5] = 50, 20           # mean 0.4 -> 0
    d = rm.sao_decide(s, 22, 8)
    lam = rm.sao_lambda(22, 8)
    assert lam == pytest.approx(5.745, abs=1e-3)
    assert (d["type"][0], d["band"][0], d["off"][0]) == (1, 30, [1, 3, -2, -1])
    assert d["cost"][0] == pytest.approx(lam * (1 + 5 + 2 + 4 + 3 + 2) - 1500, rel=1e-12)
    assert d["near_tie"] == [False, False]
    assert d["type"][1] == 0 and d["off"][1] == d["off"][2] == [0] * 4       # chroma: nothing to gain
    assert rm.sao_sse_delta(s, d, 0) == -1500 and rm.sao_sse_delta(s, d, 1) == 0
    # without bands 30 and 1, windows 29 and 30 do the same to the picture at the same price up to
    # the rounding of the sums: either may win, and that is no near tie
    s["bo_cnt"][0, 30] = s["bo_sum"][0, 30] = s["bo_cnt"][0, 1] = s["bo_sum"][0, 1] = 0
    d = rm.sao_decide(s, 22, 8)
    assert (d["band"][0], d["off"][0]) in [(29, [0, 0, 3, -2]), (30, [0, 3, -2, 0])] and d["near_tie"] == [False, False]
    # a small gain is dropped: 50 samples, sum 60 -> offset 1 gains 70 < 2 lambda at QP 37
    t = _empty_stats()
    t["bo_cnt"][0, 5], t["bo_sum"][0, 5] = 50, 60           # 50 - 120 = -70
    assert rm.sao_decide(t, 37, 8)["type"][0] == 0          # lambda 183.8


def test_sao_edge_offset_shrinks_by_exactly_one_step():
    s = _empty_stats()
    s["eo_cnt"][0, 0, 0], s["eo_sum"][0, 0, 0] = 100, 240        # mean 2.4 -> 2
    s["eo_cnt"][0, 0, 3], s["eo_sum"][0, 0, 3] = 1000, -3000     # mean -3, gain 9000: stays
    lam = rm.sao_lambda(37, 8)
    assert lam == pytest.approx(183.84, abs=1e-2)
    # 2 -> 1 pays from lambda >= 180 (-380 + lam <= -560 + 2 lam), 1 -> 0 only from lambda >= 380
    d = rm.sao_decide(s, 37, 8)
    assert (d["type"][0], d["cls"][0], d["off"][0]) == (2, 0, [1, 0, 0, -3])
    assert d["cost"][0] == pytest.approx(lam * (3 + 2 + 1 + 1 + 4) - 380 - 9000, rel=1e-12)
    assert rm.sao_cost(s, lam, d, 0) == d["cost"][0] and rm.sao_sse_delta(s, d, 0) == -9380
    assert rm.sao_decide(s, 36, 8)["off"][0] == [2, 0, 0, -3]     # lambda 145.9: no step
    assert rm.sao_decide(s, 41, 8)["off"][0] == [0, 0, 0, -3]     # lambda 463.2: both steps
    # the sign constraint: a negative mean in a valley category gives no offset
    s["eo_sum"][0, 0, 0] = -240
    assert rm.sao_decide(s, 22, 8)["off"][0] == [0, 0, 0, -3]
    # the limit: mean 9 -> 7 at 8 bits, 9 at 10 bits
    s["eo_sum"][0, 0, 0] = 900
    assert rm.sao_decide(s, 22, 8)["off"][0][0] == 7 and rm.sao_decide(s, 22, 10)["off"][0][0] == 9
    # chroma shares type and class: Cb gains on class 1, Cr on class 3 and more -> both get class 3
    c = _empty_stats()
    c["eo_cnt"][1, 1, 0], c["eo_sum"][1, 1, 0] = 1000, 2000      # gain 4000
    c["eo_cnt"][2, 3, 3], c["eo_sum"][2, 3, 3] = 1000, -3000     # gain 9000
    c["eo_cnt"][1, 3, 1], c["eo_sum"][1, 3, 1] = 1000, 1000      # gain 1000
    d = rm.sao_decide(c, 22, 8)
    assert d["type"] == [0, 2] and d["cls"][1] == 3 and d["off"][1] == [0, 1, 0, 0] and d["off"][2] == [0, 0, 0, -3]


def test_sao_shrink_tie_shrinks_and_needs_an_integer_lambda():
    """Equal prices of o and the next smaller offset: the smaller one is taken.  The two differ by
    n (2 |o| - 1) - 2 |s| + lambda, an integer plus lambda, so they tie only at an integer lambda,
    and no QP at either bit depth comes closer to one than 0.003: the encoder never meets the tie."""
    s = _empty_stats()
    s["eo_cnt"][0, 0, 0], s["eo_sum"][0, 0, 0] = 100, 240
    s["eo_cnt"][0, 0, 3], s["eo_sum"][0, 0, 3] = 1000, -3000
    assert rm.sao_decide(s, 0, 8, lam=180.0)["off"][0] == [1, 0, 0, -3]      # -560 + 360 == -380 + 180
    assert rm.sao_decide(s, 0, 8, lam=179.999)["off"][0] == [2, 0, 0, -3]
    assert rm.sao_decide(s, 0, 8, lam=380.0)["off"][0] == [0, 0, 0, -3]      # then -380 + 380 == 0 as well
    gaps = [abs(lam - round(lam)) for qp in range(52) for bd in (8, 10) for lam in [rm.sao_lambda(qp, bd)]]
    assert min(gaps) > 0.003


def test_sao_equal_costs_take_the_first_and_close_ones_are_flagged():
    s = _empty_stats()
    for k in (1, 3):
        s["eo_cnt"][0, k, 0], s["eo_sum"][0, k, 0] = 1000, 3000
    d = rm.sao_decide(s, 22, 8)
    assert (d["type"][0], d["cls"][0], d["near_tie"][0]) == (2, 1, False)      # bitwise equal: the order decides
    # 9e9 against 9e9 + 6: apart by 6.7e-10 of the cost, and another picture
    s["eo_cnt"][0, 1, 0], s["eo_sum"][0, 1, 0] = 10 ** 9, 3 * 10 ** 9
    s["eo_cnt"][0, 3, 0], s["eo_sum"][0, 3, 0] = 10 ** 9, 3 * 10 ** 9 + 1
    d = rm.sao_decide(s, 22, 8)
    assert (d["type"][0], d["cls"][0], d["near_tie"][0]) == (2, 3, True)
    lam = rm.sao_lambda(22, 8)
    other = dict(type=[2, 0], cls=[1, 0], band=[0] * 3, off=[[3, 0, 0, 0]] + [[0] * 4] * 2)
    assert abs(rm.sao_cost(s, lam, other, 0) - d["cost"][0]) == pytest.approx(6, abs=1e-3)


def test_sao_all_equal_block_is_off():
    flat = [np.full((32, 32), 100), np.full((16, 16), 60), np.full((16, 16), 200)]
    s = rm.sao_stats(flat, flat, 8, 0, 0, 32)
    assert not s["eo_cnt"].any() and not s["bo_sum"].any() and s["bo_cnt"].sum(axis=1).tolist() == [1024, 256, 256]
    d = rm.sao_decide(s, 30, 8)
    assert d["type"] == [0, 0] and d["off"] == [[0] * 4] * 3 and d["near_tie"] == [False, False]
    assert d["cost"] == [rm.sao_lambda(30, 8)] * 2


def _one_block(typ, cls, band, off):
    return dict(type=np.array([[typ]]), cls=np.array([[cls]]), band=np.array([[band]]), off=np.array([[off]]))


def test_sao_apply_by_hand_and_clips_at_both_ends():
    deb, _ = _sao_4x4()
    no = [0] * 4
    # edge class 0: the peak 12 takes off[3], the valley 8 takes off[0]; class 1 also moves the row below
    out = rm.sao_apply(deb, _one_block([2, 0], [0, 0], [0, 0, 0], [[1, 5, 6, -2], no, no]), 8)
    want = deb[0].copy()
    want[1, 1], want[1, 2] = 10, 9
    assert np.array_equal(out[0], want) and np.array_equal(out[1], deb[1])
    out = rm.sao_apply(deb, _one_block([2, 0], [1, 0], [0, 0, 0], [[1, 5, 6, -2], no, no]), 8)
    want[2, 1], want[2, 2] = 15, 16
    assert np.array_equal(out[0], want)
    # band window 30 (bands 30, 31, 0, 1) at 10 bits: 32 samples per band
    y = np.array([[1023, 1022, 991, 959], [0, 2, 31, 32], [63, 64, 500, 960]])
    c = np.array([[0, 1023]])
    out = rm.sao_apply((y, c, c), _one_block([1, 1], [0, 0], [30, 31, 0], [[5, 3, -3, 7], [9, -9, 0, 0], [-1, 0, 0, 0]]), 10)
    assert out[0].tolist() == [[1023, 1023, 996, 959], [0, 0, 28, 39], [70, 64, 500, 965]]
    assert out[1].tolist() == [[0, 1023]] and out[2].tolist() == [[0, 1023]]
    # type 0 leaves the picture alone whatever the other fields hold
    out = rm.sao_apply((y, c, c), _one_block([0, 0], [3, 3], [30, 31, 0], [[5, 3, -3, 7]] * 3), 10)
    assert np.array_equal(out[0], y)
    # two blocks side by side: each sample takes its own block's parameters, neighbours across the border
    row = np.array([[10] * 31 + [12, 8] + [10] * 31] * 3)
    ch = np.full((2, 32), 50)
    two = dict(type=np.array([[[2, 0], [2, 0]]]), cls=np.array([[[0, 0], [0, 0]]]), band=np.zeros((1, 2, 3), int),
               off=np.array([[[[0, 0, 0, -1], no, no], [[4, 0, 0, 0], no, no]]]))
    out = rm.sao_apply((row, ch, ch), two, 8)
    assert out[0][:, 30:34].tolist() == [[10, 11, 12, 10]] * 3


# ------------------------------------------------------------------ HEVC source preparation
def test_hevc_prep_pads_by_replication_and_proxy8():
    y = np.array([[1, 2, 3, 99], [4, 5, 6, 99], [99] * 4])
    u = np.array([[7, 99], [99, 99]])
    v = np.array([[250, 99], [99, 99]])
    py, pu, pv, p8 = rm.hevc_prep((y, u, v), 3, 2, 8, 4, 2, 10)      # display 3x2 (chroma 1x1) -> coded 8x4
    assert py.tolist() == [[4, 8, 12, 12, 12, 12, 12, 12], [16, 20, 24, 24, 24, 24, 24, 24]] + [[16, 20] + [24] * 6] * 2
    assert pu.tolist() == [[28] * 4] * 2 and pv.tolist() == [[1000] * 4] * 2
    assert p8.tolist() == [[1, 2, 3, 3, 3, 3, 3, 3], [4, 5, 6, 6, 6, 6, 6, 6]] + [[4, 5] + [6] * 6] * 2
    py, _, _, p8 = rm.hevc_prep((y, u, v), 4, 2, 4, 2, 0, 8)
    assert py.tolist() == y[:2].tolist() == p8.tolist()
    assert rm.proxy8([1023, 1020, 255, 256, 3], 2).tolist() == [255, 255, 63, 64, 0]
    assert rm.proxy8([255, 254, 0, 256, 1023], 0).tolist() == [255, 254, 0, 0, 255]       # the low byte

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

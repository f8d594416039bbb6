"""Hand-computed pins of the HEVC inter prediction model (tests/ref_models_hevc_wp.py), on the
CPU: tests/test_hevc_weightb_codec.py validates it against the independent decoder and
tests/test_gpu_hevc_wp_model.py compares the kernels with it."""
import numpy as np
import pytest

import ref_models_hevc_wp as wm


def test_integer_vector_copies_the_block_at_14_bits():
    ref = np.arange(48 * 40).reshape(40, 48) % 251
    p = wm.interp(ref, 8, 4, 8, 8, 4 * 3, 4 * -2, False, 8)
    assert np.array_equal(p, ref[2:10, 11:19] << 6)
    p10 = wm.interp(ref, 8, 4, 8, 8, 4 * 3, 4 * -2, False, 10)
    assert np.array_equal(p10, ref[2:10, 11:19] << 4)
    c = wm.interp(ref, 4, 2, 4, 4, 8 * 1, 8 * 2, True, 8)   # chroma: eighth-sample units
    assert np.array_equal(c, ref[4:8, 5:9] << 6)


def test_flat_plane_interpolates_to_itself():
    """Every filter's taps sum to 64: a flat plane gives v * 64 >> shift1 (one pass) or
    (v * 64 >> shift1) * 64 >> 6 (two passes) = v << (14 - bd) at any phase."""
    for bd, v in ((8, 255), (8, 0), (10, 1023), (10, 513)):
        ref = np.full((20, 24), v)
        for fx in range(4):
            for fy in range(4):
                assert np.all(wm.interp(ref, 4, 4, 8, 8, fx - 9, fy + 5, False, bd) == v << (14 - bd))
        for fx in range(8):
            for fy in range(8):
                assert np.all(wm.interp(ref, 2, 2, 4, 4, fx + 16, fy - 24, True, bd) == v << (14 - bd))


def test_luma_half_sample_of_a_step_edge_by_hand():
    """Row 0 .. 0 100 .. 100 with the edge between x = 7 and 8; half-sample taps
    -1 4 -11 40 40 -11 4 -1 around position x + 1/2 (samples x - 3 .. x + 4)."""
    ref = np.zeros((8, 16), np.int64)
    ref[:, 8:] = 100
    p = wm.interp(ref, 4, 0, 4, 1, 2, 0, False, 8)[0]   # x = 4 .. 7, fx = 2
    # x = 4: samples 1..8 -> only the last tap (-1) sees 100
    # x = 5: samples 2..9 -> taps 4, -1;  x = 6: -11, 4, -1;  x = 7: 40, -11, 4, -1
    assert p.tolist() == [-100, 300, -800, 3200]
    q = wm.interp(ref.T, 0, 4, 1, 4, 0, 2, False, 8)[:, 0]   # the same edge, vertical filter
    assert q.tolist() == [-100, 300, -800, 3200]
    # quarter sample at x = 7: taps -1 4 -10 58 17 -5 1 0 on samples 4..11 -> (17 - 5 + 1) * 100
    assert wm.interp(ref, 7, 0, 1, 1, 1, 0, False, 8)[0, 0] == 1300
    # 10 bit: shift1 = 2
    assert wm.interp(ref, 7, 0, 1, 1, 1, 0, False, 10)[0, 0] == 1300 >> 2


def test_two_pass_uses_the_shifted_intermediate():
    """fx and fy both fractional: rows first (>> shift1), then columns (>> 6)."""
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 1024, (24, 24))
    bd = 10
    t = wm.LUMA_TAPS
    x0, y0 = 9, 8
    rows = [sum(int(t[1, k]) * int(ref[y0 - 3 + r, x0 - 3 + k]) for k in range(8)) >> 2 for r in range(8)]
    want = sum(int(t[3, k]) * rows[k] for k in range(8)) >> 6
    assert wm.interp(ref, x0, y0, 1, 1, 1, 3, False, bd)[0, 0] == want
    ct = wm.CHROMA_TAPS
    rows = [sum(int(ct[5, k]) * int(ref[y0 - 1 + r, x0 - 1 + k]) for k in range(4)) >> 2 for r in range(4)]
    want = sum(int(ct[2, k]) * rows[k] for k in range(4)) >> 6
    assert wm.interp(ref, x0, y0, 1, 1, 5, 2, True, bd)[0, 0] == want


def test_reference_coordinates_are_clamped():
    ref = np.arange(12 * 10).reshape(10, 12)
    # far outside the top-left corner: every sample is ref[0, 0]; bottom-right: ref[-1, -1]
    assert np.all(wm.interp(ref, 0, 0, 8, 8, -4 * 40 + 1, -4 * 40 + 3, False, 8) == ref[0, 0] << 6)
    assert np.all(wm.interp(ref, 4, 2, 8, 8, 4 * 40 + 2, 4 * 40 + 2, False, 8) == ref[-1, -1] << 6)
    # integer vector two columns past the left edge: columns -2, -1 repeat column 0
    p = wm.interp(ref, 0, 3, 4, 2, -8, 0, False, 8) >> 6
    assert np.array_equal(p, ref[3:5, [0, 0, 0, 1]])


def test_default_weighting_by_hand():
    assert wm.weight_default(np.array([0, 31, 32, 16320, 16383, -40]), None, 8).tolist() == [0, 0, 1, 255, 255, 0]
    assert wm.weight_default(np.array([7, 8, 16376]), None, 10).tolist() == [0, 1, 1023]
    # bi, 8 bit: (a + b + 64) >> 7
    assert wm.weight_default(np.array([64, 0, 16320]), np.array([0, 63, 16320]), 8).tolist() == [1, 0, 255]
    assert wm.weight_default(np.array([8, 7]), np.array([8, 8]), 10).tolist() == [1, 0]   # (a + b + 16) >> 5


def test_explicit_weighting_by_hand():
    p = np.array([6400])   # sample 100 at 8 bits
    # uni: ((6400 * 96 + 2048) >> 12) - 20 = 150 - 20
    assert wm.weight_explicit(p, 96, -20, None, 0, 0, 8)[0] == 130
    # 10 bit, sample 400 (<< 4): ((6400 * 96 + 512) >> 10) + (-20 << 2) = 600 - 80
    assert wm.weight_explicit(p, 96, -20, None, 0, 0, 10)[0] == 520
    # bi: (6400 * 96 + 3200 * 32 + ((-20 + 10 + 1) << 12)) >> 13 = (614400 + 102400 - 36864) >> 13
    assert wm.weight_explicit(p, 96, -20, np.array([3200]), 32, 10, 8)[0] == (614400 + 102400 - 36864) >> 13 == 83
    # extremes clip: weight 127 on the maximum, offset -128 on zero
    assert wm.weight_explicit(np.array([16320]), 127, 127, None, 0, 0, 8)[0] == 255
    assert wm.weight_explicit(np.array([0]), 1, -128, None, 0, 0, 8)[0] == 0
    assert wm.weight_explicit(np.array([16320]), 1, 127, None, 0, 0, 8)[0] == ((16320 + 2048) >> 12) + 127
    # a negative intermediate shifts arithmetically (floor)
    assert wm.weight_explicit(np.array([-100]), 127, 3, None, 0, 0, 8)[0] == ((-12700 + 2048) >> 12) + 3 == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_identity_weights_equal_the_default_formula(bd):
    """(64, 0) over 2^6 on random 14-bit inputs, uni and bi: both are the same shift of the same
    sum -- an unweighted slot of a weightb stream may keep the default path."""
    rng = np.random.default_rng(bd)
    p0 = rng.integers(-(1 << 13), 1 << 14, 4096)
    p1 = rng.integers(-(1 << 13), 1 << 14, 4096)
    assert np.array_equal(wm.weight_explicit(p0, 64, 0, None, 0, 0, bd), wm.weight_default(p0, None, bd))
    assert np.array_equal(wm.weight_explicit(p0, 64, 0, p1, 64, 0, bd), wm.weight_default(p0, p1, bd))


def test_predict_substitutes_identity_for_the_unweighted_list():
    rng = np.random.default_rng(5)
    r0, r1 = rng.integers(0, 256, (40, 48)), rng.integers(0, 256, (40, 48))
    a = wm.predict(r0, r1, 8, 8, 8, 8, wm.DIR_BI, (5, -3), (-2, 7), False, 8, wp0=(96, -20))
    b = wm.predict(r0, r1, 8, 8, 8, 8, wm.DIR_BI, (5, -3), (-2, 7), False, 8, wp0=(96, -20), wp1=(64, 0))
    assert np.array_equal(a, b)
    # list-1-only block of a slice weighted on list 0 only: the default prediction
    c = wm.predict(r0, r1, 8, 8, 8, 8, wm.DIR_L1, (5, -3), (-2, 7), False, 8, wp0=(96, -20))
    assert np.array_equal(c, wm.predict(r0, r1, 8, 8, 8, 8, wm.DIR_L1, (5, -3), (-2, 7), False, 8))
    # and a list-0 block of it is weighted
    d = wm.predict(r0, r1, 8, 8, 8, 8, wm.DIR_L0, (4, 0), (0, 0), False, 8, wp0=(96, -20))
    assert np.array_equal(d, np.clip(((r0[8:16, 9:17] * 64 * 96 + 2048) >> 12) - 20, 0, 255))


def test_wp_ref8_by_hand():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(wm.wp_ref8(b, 64, 0), b)
    assert wm.wp_ref8(np.array([0, 1, 2, 3, 200]), 32, 0).tolist() == [0, 1, 1, 2, 100]   # (r * 32 + 32) >> 6: halves round up
    assert wm.wp_ref8(np.array([100, 255, 0]), 96, -20).tolist() == [130, 255, 0]
    assert wm.wp_ref8(np.array([255]), 1, -128)[0] == 0 and wm.wp_ref8(np.array([255]), 127, 127)[0] == 255

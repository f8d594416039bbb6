"""The numpy model of the HEVC quantiser with RDOQ (tests/ref_models_hevc_rdoq.py) on cases
computed by hand, the lane-parallel form against the serial pass, and level 0 against the
dead-zone formula.

The hand cases use Qp' 28 at 8 bits: qscale = 2^14 and, at 4x4, qbits = 23, so a step is 512 in
coefficient units, lr = round(a / 512) and e(l) = (a - 512 l) / 2 for even a; at 8x8 qbits = 22,
a step is 256 and e(l) = a - 256 l.  lam = 368 unless stated.
"""
import numpy as np
import pytest

import ref_models_hevc_rdoq as rq

QP, BD = 28, 8
LAM = 368


def _block(log2n, scan, placed):
    """coefficient block with placed = {scan position: value}"""
    order, _ = rq.positions(scan, log2n)
    c = np.zeros((1 << log2n, 1 << log2n), dtype=np.int64)
    for p, v in placed.items():
        x, y = order[p]
        c[y, x] = v
    return c


def _levels(log2n, scan, placed, level=1, lam=LAM, qp=QP, bd=BD):
    order, _ = rq.positions(scan, log2n)
    lev = rq.quantise(_block(log2n, scan, placed), log2n, bd, qp, False, scan, False, level, lam)
    return {p: int(lev[y, x]) for p, (x, y) in enumerate(order) if lev[y, x]}


def test_scans_and_constants():
    assert rq.scan_order(0, 2)[:7] == [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0), (0, 3)]
    assert rq.scan_order(1, 1) == [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert rq.scan_order(2, 1) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for scan in range(3):
        for lg in range(2, 6):
            order, pos = rq.positions(scan, lg)
            assert order[0] == (0, 0) and sorted(order) == sorted((x, y) for x in range(1 << lg) for y in range(1 << lg))
            assert all(pos[y, x] == p for p, (x, y) in enumerate(order))
    # 8x8 diagonal: group 1 is the 4x4 block below the DC group (6.5.3 walks a diagonal upwards)
    assert rq.positions(0, 3)[0][16] == (0, 4) and rq.positions(1, 3)[0][16] == (4, 0)
    assert rq.qparams(2, 8, 28) == (23, 16384) and rq.qparams(3, 8, 28) == (22, 16384)
    assert [rq.g_bits(l) for l in (1, 2, 3, 4, 6, 7, 8, 9, 10)] == [10, 35, 62, 78, 110, 126, 158, 158, 190]
    assert all(rq.g_bits(l) <= rq.g_bits(l + 1) for l in range(1, 40000))
    assert rq.rate(0, False, 5) == 0 and rq.rate(0, True, 5) == 9
    assert rq.rate(1, True, 15) == 48 and rq.rate(1, False, 15) == 48 + 24 + 20 * 4 and rq.rate(1, False, 0) == 72
    assert rq.lam_of(1.0) == 368 and rq.lam_of(0.5) == 184 and rq.lam_of(1.5) == 552 and rq.lam_of(0.75) == 276


def test_trailing_one_dropped_but_kept_before_a_large_level():
    # a = 400 at p = 15: lr = 1, e(1) = -56, e(0) = 200.  Alone it would be the last position:
    # J(1) = 3136 + 368 * 152 = 59072 > J(0) = 40000 -> dropped, the block is empty
    assert rq.round_nearest(400, 16384, 23) == (1, -56)
    assert _levels(2, 0, {15: 400}) == {}
    assert _levels(2, 0, {15: -400}) == {}
    # at p = 14 before a = 5120 (level 10) at p = 15: seen, J(1) = 3136 + 368 * 48 = 20800 <
    # J(0) = 40000 + 368 * 9 = 43312 -> kept
    assert _levels(2, 0, {14: 400, 15: 5120}) == {14: 1, 15: 10}
    assert _levels(2, 0, {14: -400, 15: -5120}) == {14: -1, 15: -10}
    # and what follows a dropped trailing coefficient is judged as the last position again:
    # a = 400 at p = 3 (LAST = 24 + 20 * 2): J(1) = 3136 + 368 * 112 = 44352 > 40000 -> dropped too
    assert _levels(2, 0, {3: 400, 15: 400}) == {}
    # at p = 0 (LAST = 24): J(1) = 3136 + 368 * 72 = 29632 < 40000 -> kept
    assert _levels(2, 0, {0: 400, 3: 400, 15: 400}) == {0: 1}


def test_break_even_of_a_one():
    # seen, lr = 1: J(1) = e^2 + 17664, J(0) = (e + 256)^2 + 3312: the one stays for e >= -99
    # a = 314: e = -99, J(1) = 27465 < J(0) = 27961;  a = 312: e = -100, J(1) = 27664 > J(0) = 27648
    assert rq.choose(1, -99, LAM, 7, True) == 1 and rq.choose(1, -100, LAM, 7, True) == 0
    assert _levels(2, 0, {7: 314, 15: 5120}) == {7: 1, 15: 10}
    assert _levels(2, 0, {7: 312, 15: 5120}) == {15: 10}
    # lr = 3 (a = 1330: e(3) = -103, e(2) = 153), seen: J(3) = 10609 + 368 * 100 = 47409,
    # J(2) = 23409 + 368 * 73 = 50273 -> 3;  a = 1320: e(3) = -108, J(3) = 11664 + 36800 = 48464 <
    # J(2) = 148^2 + 26864 = 48768 -> 3;  a = 1310: e(3) = -113, J(3) = 12769 + 36800 = 49569 >
    # J(2) = 143^2 + 26864 = 47313 -> 2
    assert _levels(2, 0, {7: 1330, 15: 5120})[7] == 3
    assert _levels(2, 0, {7: 1320, 15: 5120})[7] == 3
    assert _levels(2, 0, {7: 1310, 15: 5120})[7] == 2


def test_tie_goes_to_the_smaller_level():
    # seen, lr = 1, e = -89 (a = 334): J(1) - J(0) = 39 lam - 512 (e + 128) = 39 (lam - 512)
    assert rq.round_nearest(334, 16384, 23) == (1, -89)
    assert 89 * 89 + 512 * 48 == 167 * 167 + 512 * 9
    assert _levels(2, 0, {7: 334, 15: 5120}, lam=512) == {15: 10}
    assert _levels(2, 0, {7: 334, 15: 5120}, lam=511) == {7: 1, 15: 10}


def test_level_clip():
    # 32x32 at 10 bits, Qp' 4: qbits = 14 and qscale = 2^14, so lr = a up to the clip
    assert rq.qparams(5, 10, 4) == (14, 16384)
    assert rq.round_nearest(32767, 16384, 14) == (32767, 0)
    assert rq.round_nearest(40000, 16384, 14) == (32767, 16383)  # e = 7233 * 256 before the bound
    assert _levels(5, 0, {0: 32767}, qp=4, bd=10) == {0: 32767}
    # behind the clip both candidates have the bounded error and the same rate: the tie goes down
    assert rq.g_bits(32767) == rq.g_bits(32766)
    assert _levels(5, 0, {0: -40000}, qp=4, bd=10) == {0: -32766}
    lev = rq.quantise(_block(5, 0, {0: 40000}), 5, 10, 4, True, 0, False, 0, 0)
    assert lev[0, 0] == 32767  # the dead-zone quantiser clips too


def test_group_zero_out():
    # 8x8: a step is 256.  Two coefficients a = 166 (lr = 1, e(1) = -90, e(0) = 166) in group 1 before
    # a = 2560 (level 10) in group 3.  Level 1 keeps them (J(1) = 8100 + 17664 < J(0) = 27556 + 3312).
    # Level 2: sum D(0) + lam * 8 = 55112 + 2944 < 2 * 25764 + 14 * 3312 + lam * 18 = 104520 -> cleared
    assert rq.round_nearest(166, 16384, 22) == (1, -90)
    placed = {17: 166, 26: -166, 50: 2560}
    assert _levels(3, 0, placed, level=1) == {17: 1, 26: -1, 50: 10}
    assert _levels(3, 0, placed, level=2) == {50: 10}
    # a full group of them pays for its flags: 16 * 27556 + 2944 > 16 * 25764 + 6624 -> stays
    full = {p: 166 for p in range(16, 32)}
    full[50] = 2560
    assert _levels(3, 0, full, level=2) == _levels(3, 0, full, level=1) == {**{p: 1 for p in range(16, 32)}, 50: 10}
    # a level above 2 in the group (lr = 3) keeps the group whatever the sums say
    assert _levels(3, 0, {17: 166, 26: 768, 50: 2560}, level=2) == {17: 1, 26: 3, 50: 10}
    # the same for the other scans and at 16x16 (a step is 128 there)
    for scan in (1, 2):
        assert _levels(3, scan, placed, level=2) == {50: 10} and len(_levels(3, scan, placed, level=1)) == 3
    assert _levels(4, 0, {17: 83, 26: -83, 200: 1280}, level=1) == {17: 1, 26: -1, 200: 10}
    assert _levels(4, 0, {17: 83, 26: -83, 200: 1280}, level=2) == {200: 10}


def test_group_zero_is_never_cleared():
    placed = {3: 166, 9: -166, 50: 2560}
    assert _levels(3, 0, placed, level=1) == _levels(3, 0, placed, level=2) == {3: 1, 9: -1, 50: 10}
    # a 4x4 TU has no other group: level 2 is level 1 there
    rng = np.random.default_rng(5)
    for _ in range(200):
        c = rng.integers(-1500, 1500, size=(4, 4))
        a = rq.quantise(c, 2, BD, QP, True, 0, False, 1, LAM)
        assert np.array_equal(a, rq.quantise(c, 2, BD, QP, True, 0, False, 2, LAM))


def _random_coefs(rng, log2n, bd, qp, count):
    """Laplacian coefficients whose scale falls with the frequency: levels 0..3 near the DC,
    mostly zero far from it, a few large ones"""
    n = 1 << log2n
    qbits, qscale = rq.qparams(log2n, bd, qp)
    step = (1 << qbits) / qscale
    f = np.add.outer(np.arange(n), np.arange(n)) / n
    c = rng.laplace(0.0, 1.0, size=(count, n, n)) * step * (1.6 / (1.0 + 6.0 * f))
    big = rng.random((count, n, n)) < 0.002
    return np.where(big, c * 40, c).round().astype(np.int64)


@pytest.mark.parametrize("log2n", [2, 3, 4, 5])
def test_parallel_form_equals_serial_pass(log2n):
    rng = np.random.default_rng(100 + log2n)
    differ = 0
    for k, coef in enumerate(_random_coefs(rng, log2n, 8 + 2 * (log2n & 1), 30, 2000)):
        bd, scan = 8 + 2 * (log2n & 1), (k % 3 if log2n <= 3 else 0)
        lam = (184, 368, 552)[k % 3]
        serial, _ = rq.rdoq_serial(coef, log2n, bd, 30, scan, 1, lam)
        assert np.array_equal(serial, rq.rdoq_parallel(coef, log2n, bd, 30, scan, lam)), k
        dz, _ = rq.quant_deadzone(coef, log2n, bd, 30, False)
        differ += not np.array_equal(serial, dz)
    assert differ > 1000  # the blocks are not ones every quantiser agrees on


def test_level_0_is_the_dead_zone_formula():
    rng = np.random.default_rng(9)
    for log2n, bd, qp, intra in ((2, 8, 4, True), (3, 10, 22, False), (4, 8, 37, True), (5, 10, 63, False), (5, 8, 51, True)):
        coef = rng.integers(-32768, 32768, size=(1 << log2n, 1 << log2n))
        qbits = 14 + qp // 6 + 15 - bd - log2n
        want = np.minimum(32767, (np.abs(coef) * rq.QUANT_SCALE[qp % 6] + ((171 if intra else 85) << (qbits - 9))) >> qbits)
        got = rq.quantise(coef, log2n, bd, qp, intra, 0, False, 0, 0)
        assert np.array_equal(got, np.where(coef < 0, -want, want))


def test_sign_data_hiding_parity_holds_after_rdoq():
    """the parity rule on RDOQ's levels: every group with a span above 3 hides its first sign"""
    rng = np.random.default_rng(21)
    changed = 0
    for k, coef in enumerate(_random_coefs(rng, 3, 8, 30, 300)):
        scan = k % 3
        order, _ = rq.positions(scan, 3)
        plain = rq.quantise(coef, 3, 8, 30, True, scan, False, 2, LAM)
        lev = rq.quantise(coef, 3, 8, 30, True, scan, True, 2, LAM)
        changed += not np.array_equal(plain, lev)
        assert np.abs(lev - plain).sum() <= 4  # at most one level per group moves, by one
        for g in range(4):
            lv = [int(lev[order[16 * g + q][1], order[16 * g + q][0]]) for q in range(16)]
            sig = [q for q in range(16) if lv[q]]
            if sig and sig[-1] - sig[0] > 3:
                assert (sum(abs(v) for v in lv) & 1) == (1 if lv[sig[0]] < 0 else 0)
    assert changed > 50

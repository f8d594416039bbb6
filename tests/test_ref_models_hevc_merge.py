"""Hand-computed pins of the HEVC merge model (tests/ref_models_hevc_merge.py), on the CPU: the
GPU tests of tests/test_gpu_hevc_merge_model.py rest on it."""
import numpy as np
import pytest

import ref_models_hevc_merge as hm
import ref_models_me as mm


def L0(x, y, r=0):
    return (1 | (r << 2), x, y, 0, 0)


def L1(x, y):
    return (2, 0, 0, x, y)


def BI(x0, y0, x1, y1):
    return (3, x0, y0, x1, y1)


ZP, ZB = L0(0, 0), BI(0, 0, 0, 0)


# ---------------------------------------------------------------------------- z-scan availability

def _morton(x, y):
    k = 0
    for b in range(4):
        k |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return k


def _explicit_order(wmb, hmb, sh):
    """coding order by sorting every block by (CTU row, CTU column, Morton index inside the CTU)"""
    n = 1 << sh
    keys = sorted((y >> sh, x >> sh, _morton(x & (n - 1), y & (n - 1)), x, y) for y in range(hmb) for x in range(wmb))
    return {(x, y): i for i, (_, _, _, x, y) in enumerate(keys)}


@pytest.mark.parametrize("sh", [1, 2])
@pytest.mark.parametrize("ctus", [(4, 4), None])
def test_availability_is_coding_order(sh, ctus):
    """a 4x4-CTU picture, and 10x6 blocks (partial CTUs at the right and bottom edges)"""
    wmb, hmb = (ctus[0] << sh, ctus[1] << sh) if ctus else (10, 6)
    order = hm.coding_order(wmb, hmb, sh)
    ex = _explicit_order(wmb, hmb, sh)
    assert sorted(order.reshape(-1).tolist()) == list(range(wmb * hmb))
    for (x, y), i in ex.items():
        assert order[y, x] == i
    later_ctu_in_picture = 0
    for my in range(hmb):
        for mx in range(wmb):
            for k, (nx, ny) in hm.neighbour_positions(mx, my).items():
                inside = 0 <= nx < wmb and 0 <= ny < hmb
                want = inside and ex[(nx, ny)] < ex[(mx, my)]
                assert hm.available(order, nx, ny, mx, my) == want, (k, mx, my)
                if inside and not want and (nx >> sh, ny >> sh) != (mx >> sh, my >> sh):
                    later_ctu_in_picture += 1
    assert later_ctu_in_picture > 0


def test_availability_in_a_32x32_ctb():
    """A0 is available for quadrant 0 only, B0 not for quadrant 3 (whose B0 lies in the next CTU)"""
    order = hm.coding_order(8, 8, 1)
    for my in range(1, 7):
        for mx in range(1, 7):
            quad = (mx & 1) | ((my & 1) << 1)
            assert hm.available(order, mx - 1, my + 1, mx, my) == (quad == 0)
            assert hm.available(order, mx + 1, my - 1, mx, my) == (quad != 3)
            assert hm.available(order, mx - 1, my, mx, my) and hm.available(order, mx, my - 1, mx, my)
            assert hm.available(order, mx - 1, my - 1, mx, my)
    # in the picture, but in a CTU that is coded later
    assert not hm.available(order, 4, 2, 3, 3) and not hm.available(order, 1, 4, 2, 3)
    # outside the picture
    assert not hm.available(order, 8, 1, 7, 2) and not hm.available(order, -1, 1, 0, 0) and not hm.available(order, 1, 8, 2, 7)


def test_availability_in_a_64x64_ctu():
    order = hm.coding_order(8, 8, 2)
    assert [int(order[y, x]) for y, x in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (3, 3), (0, 4))] == \
        [0, 1, 2, 3, 4, 8, 15, 16]
    # block (1, 2) (z 9): above-right (2, 1) has z 6; below-left (0, 3) has z 10
    assert hm.available(order, 2, 1, 1, 2) and not hm.available(order, 0, 3, 1, 2)
    # block (2, 2) (z 12): below-left (1, 3) has z 11; block (1, 1) (z 3): above-right (2, 0) has z 4
    assert hm.available(order, 1, 3, 2, 2) and not hm.available(order, 2, 0, 1, 1)
    # block (3, 1) (z 7): above-right (4, 0) is the next CTU; block (4, 1): below-left (3, 2) the previous one
    assert not hm.available(order, 4, 0, 3, 1) and hm.available(order, 3, 2, 4, 1)


# ---------------------------------------------------------------------------- pruning

a, b, c, d, e, t = L0(4, -8), L0(5, 0), L0(-3, 2), L0(40, 41), L0(-1, -1), L0(7, 7)


def _p(nb, temporal=None, max_merge=5, nref0=1):
    return hm.merge_list(nb, temporal, 0, max_merge, nref0)


def test_pruning_a1_b1():
    assert _p(dict(A1=a, B1=a)) == ([a, ZP, ZP, ZP, ZP], ["A1", "Z", "Z", "Z", "Z"], ["A1-B1"])
    assert _p(dict(A1=a, B1=b))[0] == [a, b, ZP, ZP, ZP]
    assert _p(dict(A1=a, B1=L0(4, -8, 1)), nref0=2)[2] == []  # the refIdx is part of a motion


def test_pruning_b1_b0():
    assert _p(dict(A1=b, B1=a, B0=a)) == ([b, a, ZP, ZP, ZP], ["A1", "B1", "Z", "Z", "Z"], ["B1-B0"])
    # B0 is compared with B1 only
    assert _p(dict(A1=a, B1=b, B0=a)) == ([a, b, a, ZP, ZP], ["A1", "B1", "B0", "Z", "Z"], [])
    # and with the neighbour B1 itself, whether or not B1 made it into the list
    assert _p(dict(A1=a, B1=a, B0=a)) == ([a, ZP, ZP, ZP, ZP], ["A1", "Z", "Z", "Z", "Z"], ["A1-B1", "B1-B0"])


def test_pruning_a1_a0():
    assert _p(dict(A1=a, A0=a)) == ([a, ZP, ZP, ZP, ZP], ["A1", "Z", "Z", "Z", "Z"], ["A1-A0"])
    assert _p(dict(B1=a, A0=a)) == ([a, a, ZP, ZP, ZP], ["B1", "A0", "Z", "Z", "Z"], [])  # A0 against A1 only


def test_pruning_b2():
    assert _p(dict(A1=a, B2=a)) == ([a, ZP, ZP, ZP, ZP], ["A1", "Z", "Z", "Z", "Z"], ["A1-B2"])
    assert _p(dict(B1=a, B2=a)) == ([a, ZP, ZP, ZP, ZP], ["B1", "Z", "Z", "Z", "Z"], ["B1-B2"])
    assert _p(dict(A1=b, B1=a, B2=a)) == ([b, a, ZP, ZP, ZP], ["A1", "B1", "Z", "Z", "Z"], ["B1-B2"])
    assert _p(dict(B0=a, A0=b, B2=a)) == ([a, b, a, ZP, ZP], ["B0", "A0", "B2", "Z", "Z"], [])  # not against B0 / A0


def test_four_present_so_no_b2():
    nb = dict(A1=a, B1=b, B0=c, A0=d, B2=e)
    assert _p(nb) == ([a, b, c, d, ZP], ["A1", "B1", "B0", "A0", "Z"], ["four-no-B2"])
    assert _p(nb, temporal=t) == ([a, b, c, d, t], ["A1", "B1", "B0", "A0", "T"], ["four-no-B2"])
    # one of the four pruned: B2 takes the fourth place
    nb["B0"] = b
    assert _p(nb, temporal=t) == ([a, b, d, e, t], ["A1", "B1", "A0", "B2", "T"], ["B1-B0"])


def test_temporal_refused_once_the_list_is_full():
    nb = dict(A1=a, B1=b)
    assert _p(nb, temporal=t, max_merge=2) == ([a, b], ["A1", "B1"], ["T-full"])
    assert _p(nb, temporal=t, max_merge=3) == ([a, b, t], ["A1", "B1", "T"], [])
    assert _p(dict(A1=a, B1=b, B0=c, A0=d), temporal=t, max_merge=3) == ([a, b, c], ["A1", "B1", "B0"], ["T-full"])
    # a P slice's temporal candidate is list 0, refIdx 0
    order = hm.coding_order(2, 2, 1)
    lst, src, _, _, _ = hm.block_merge_list(np.array([1, 1, 1, 1]), np.zeros((4, 4), dtype=np.int16), order, 0, 0, 2,
                                            np.array([9, -9, 5, 5]), 0, 2)
    assert lst == [L0(9, -9), ZP] and src == ["T", "Z"]
    lst, src, _, _, _ = hm.block_merge_list(np.array([1, 1, 1, 1]), np.zeros((4, 4), dtype=np.int16), order, 0, 0, 1,
                                            np.array([9, -9, 5, 5]), 1, 2)
    assert lst == [BI(9, -9, 5, 5), ZB] and src == ["T", "Z"]


# ---------------------------------------------------------------------------- combined, zero, truncation

# 8.5.3.2.4: combIdx -> l0CandIdx, l1CandIdx
_SPEC_COMB = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (0, 3), (3, 0), (1, 3), (3, 1), (2, 3), (3, 2)]


def test_combined_candidates_follow_the_table():
    assert list(zip(hm.COMB_L0, hm.COMB_L1)) == _SPEC_COMB
    # four bi candidates and (beyond any real MaxNumMergeCand) room for all twelve combinations
    k = [BI(10 * i + 1, 10 * i + 2, 10 * i + 3, 10 * i + 4) for i in range(4)]
    lst, src, _ = hm.merge_list(dict(A1=k[0], B1=k[1], B0=k[2], A0=k[3]), None, 1, 16)
    assert lst[:4] == k and src == ["A1", "B1", "B0", "A0"] + ["C"] * 12
    assert lst[4:] == [BI(k[i][1], k[i][2], k[j][3], k[j][4]) for i, j in _SPEC_COMB]
    # three originals: six combinations, then zero candidates
    lst, src, _ = hm.merge_list(dict(A1=k[0], B1=k[1], B0=k[2]), None, 1, 10)
    assert src == ["A1", "B1", "B0"] + ["C"] * 6 + ["Z"]
    assert lst[3:9] == [BI(k[i][1], k[i][2], k[j][3], k[j][4]) for i, j in _SPEC_COMB[:6]]


def test_combined_candidates_hand_built_list():
    """A1 L0, B1 L1, B0 bi, A0 L0: MaxNumMergeCand 5 leaves one place; combIdx 0 (A1's L0, B1's L1) takes it"""
    nb = dict(A1=L0(1, 2), B1=L1(3, 4), B0=BI(5, 6, 7, 8), A0=L0(9, 10))
    assert hm.merge_list(nb, None, 1, 5) == ([nb["A1"], nb["B1"], nb["B0"], nb["A0"], BI(1, 2, 3, 4)],
                                             ["A1", "B1", "B0", "A0", "C"], [])
    # A1 L1, B1 L0: combIdx 0 needs A1's L0 -- skipped; combIdx 1 is B1's L0 with A1's L1
    nb = dict(A1=L1(3, 4), B1=L0(1, 2))
    assert hm.merge_list(nb, None, 1, 5) == ([L1(3, 4), L0(1, 2), BI(1, 2, 3, 4), ZB, ZB], ["A1", "B1", "C", "Z", "Z"], [])
    # two L0 candidates: nothing combines; one candidate, or a P slice: no combined candidates at all
    assert hm.merge_list(dict(A1=L0(1, 2), B1=L0(2, 2)), None, 1, 4)[1] == ["A1", "B1", "Z", "Z"]
    assert hm.merge_list(dict(A1=BI(1, 2, 3, 4)), None, 1, 3)[1] == ["A1", "Z", "Z"]
    assert hm.merge_list(dict(A1=L0(1, 2), B1=L0(2, 2)), None, 0, 4)[1] == ["A1", "B1", "Z", "Z"]
    # the temporal candidate counts as an original: A1 L0 + temporal bi -> (A1's L0, T's L1), then (T's L0, ...) fails
    lst, src, _ = hm.merge_list(dict(A1=L0(1, 2)), BI(5, 6, 7, 8), 1, 5)
    assert (lst, src) == ([L0(1, 2), BI(5, 6, 7, 8), BI(1, 2, 7, 8), ZB, ZB], ["A1", "T", "C", "Z", "Z"])
    # a full list takes none (numOrig == MaxNumMergeCand)
    assert hm.merge_list(dict(A1=L0(1, 2), B1=L1(3, 4)), None, 1, 2)[1] == ["A1", "B1"]


def test_zero_fill_p_slice_three_refs():
    assert hm.merge_list(dict(A1=a), None, 0, 5, nref0=3) == (
        [a, L0(0, 0, 0), L0(0, 0, 1), L0(0, 0, 2), L0(0, 0, 0)], ["A1", "Z", "Z", "Z", "Z"], [])
    assert [m[0] for m in hm.merge_list({}, None, 0, 5, nref0=3)[0]] == [1, 5, 9, 1, 1]
    assert hm.merge_list({}, None, 1, 3)[0] == [ZB, ZB, ZB]


@pytest.mark.parametrize("max_merge,want", [(1, ["A1"]), (2, ["A1", "B1"]), (3, ["A1", "B1", "B0"]),
                                            (5, ["A1", "B1", "B0", "A0", "T"])])
def test_truncation(max_merge, want):
    nb = dict(A1=a, B1=b, B0=c, A0=d, B2=e)
    lst, src, _ = _p(nb, temporal=t, max_merge=max_merge)
    assert src == want and lst == [dict(nb, T=t)[k] for k in want]


# ---------------------------------------------------------------------------- prediction, SATD, prices

def _ref(seed=5, W=48, H=32):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H, W)).astype(np.float64)
    k = np.ones(3) / 3
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    return np.clip(base, 0, 255).astype(np.uint8)


def test_prediction_equals_planes_block():
    ref = _ref()
    p, q = hm.Pred(ref), mm.Planes(ref)
    assert hm.QTAP == mm._TAPS
    for X0, Y0 in ((0, 0), (32, 16), (16, 0)):
        for ph in range(16):
            for bx, by in ((0, 0), (-72, 40), (120, -100), (-300, -300), (400, 300)):
                mv = (bx + (ph & 3), by + (ph >> 2))
                assert np.array_equal(p.block(X0, Y0, *mv), q.block(X0, Y0, *mv)), (X0, Y0, mv)


def test_prediction_far_outside_is_the_replicated_edge():
    ref = _ref(6)
    H, W = ref.shape
    p = hm.Pred(ref)
    big = mm.Planes(np.pad(ref, 600, mode="edge"))  # the same picture with 600 more samples of edge
    for ph in range(16):
        fx, fy = ph & 3, ph >> 2
        for mv in ((2000 + fx, fy), (-2000 + fx, 8 + fy), (4 + fx, 2000 + fy), (fx, -2000 + fy), (2000 + fx, -2000 + fy),
                   (32767, -32768)):
            got = p.block(16, 16, *mv)
            assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 255
            if abs(mv[0]) < 2400 and abs(mv[1]) < 2400:
                assert np.array_equal(got, big.block(616, 616, *mv)), mv
    # integer positions: a column / the corner sample repeated
    assert np.array_equal(p.block(16, 16, 2000, 0), np.tile(ref[16:32, W - 1:W].astype(np.int64), (1, 16)))
    assert np.array_equal(p.block(16, 16, 0, -2000), np.tile(ref[0:1, 16:32].astype(np.int64), (16, 1)))
    assert (p.block(16, 16, 32767, -32768) == int(ref[0, W - 1])).all()


def test_bipred_rounds_up():
    assert hm.bipred(np.array([0, 1, 255, 7]), np.array([1, 1, 254, 10])).tolist() == [1, 1, 255, 9]


def test_satd_by_hand():
    r = np.zeros((16, 16), dtype=np.int64)
    assert hm.satd16(r, r) == 0
    r[5, 6] = 3          # one sample: all sixteen coefficients of its 4x4 block are +-3 -> 48
    r[8:12, 12:16] = -2  # a flat block: one coefficient, 16 * 2 -> 32
    r[0, 0:2] = (1, -1)  # (1, -1, 0, 0) in a row: rows of H4 give 0, 0, 2, 2; times four columns -> 16
    assert hm.satd16(r, np.zeros_like(r)) == (48 + 32 + 16) // 2
    assert hm.satd16(np.zeros_like(r), r) == 48
    src = np.full((16, 16), 200, dtype=np.uint8)
    assert hm.satd16(src, np.zeros((16, 16), dtype=np.uint8)) == 16 * 16 * 200 // 2


def test_prices():
    assert [hm.ref_bins(r, 1) for r in range(2)] == [0, 0]
    assert [hm.ref_bins(r, 2) for r in range(2)] == [1, 1]
    assert [hm.ref_bins(r, 3) for r in range(3)] == [1, 2, 2]
    assert [hm.ref_bins(r, 4) for r in range(4)] == [1, 2, 3, 3]
    assert [hm.merge_bins(j, 1) for j in range(1)] == [1]
    assert [hm.merge_bins(j, 2) for j in range(2)] == [2, 2]
    assert [hm.merge_bins(j, 3) for j in range(3)] == [2, 3, 3]
    assert [hm.merge_bins(j, 5) for j in range(5)] == [2, 3, 4, 5, 5]
    assert [hm.se_bits(v) for v in (0, 1, -1, 2, -2, 3, 4, -7, 8)] == [1, 3, 3, 5, 5, 5, 7, 7, 9]
    tab = np.arange(100, 152)
    assert hm.lambdas(tab, 22, np.array([-30, -22, 0, 29, 30, 127], dtype=np.int8)).tolist() == [100, 100, 122, 151, 151, 151]
    assert hm.motion(2, (5, 6, 7, 8)) == (2, 0, 0, 7, 8) and hm.motion(9, (5, 6, 7, 8)) == (9, 5, 6, 0, 0)


def test_chg_nearby_by_hand():
    """a flag at (2, 1) of a 5x3 picture reaches the block itself and the blocks it is A1, B1, B0, A0 or B2 of"""
    chg = np.zeros(15, dtype=np.uint8)
    chg[1 * 5 + 2] = 1
    near = hm.chg_nearby(chg, 5, 3).reshape(3, 5)
    want = np.zeros((3, 5), dtype=bool)
    want[1, 2] = want[1, 3] = want[2, 2] = want[2, 1] = want[0, 3] = want[2, 3] = True
    assert np.array_equal(near, want)


# ---------------------------------------------------------------------------- the passes, by hand

def test_b_init_p_by_hand():
    """lambda 10, three refs (bins 1, 2, 2): block 0 stays, block 1 goes to ref 1, block 2 has ref 1 cheaper before
    the bins only, block 3 skips the unsearched ref 1 and takes ref 2, block 4 ties and keeps the earlier ref"""
    lam = np.full(5, 10)
    mv0 = np.array([[4, 4]] * 5)
    pm0 = np.array([[4, 4], [4, 4], [4, 4], [4, 4], [0, 0]])
    cost0 = np.array([100, 100, 100, 100, 100])
    xmv = np.array([[[8, 0]] * 5, [[-8, 2]] * 5])
    xpm = np.array([[[8, 0]] * 5, [[-8, 1]] * 5])
    xcost = np.array([[200, 80, 95, hm.KNO, 90], [300, 95, 300, 70, 300]])
    out, rec = hm.b_init_p(mv0, cost0, pm0, lam, 3, xmv, xcost, xpm)
    assert out["dir"].tolist() == [1, 5, 1, 9, 1]
    assert out["cost"].tolist() == [110, 100, 110, 90, 110]
    assert out["bits"].tolist() == [2 + 1, 2 + 2, 2 + 1, (1 + 3) + 2, (7 + 7) + 1]
    assert out["mvb"].tolist() == [[4, 4, 0, 0], [8, 0, 0, 0], [4, 4, 0, 0], [-8, 2, 0, 0], [4, 4, 0, 0]]
    assert [r["lost_to_bins"] for r in rec] == [[], [], [1], [], [1]] and rec[3]["skipped"] == [1]
    out, _ = hm.b_init_p(mv0, cost0, pm0, lam)
    assert out["cost"].tolist() == cost0.tolist() and out["bits"].tolist() == [2, 2, 2, 2, 14] and (out["dir"] == 1).all()


def _flat_case():
    """a 3x2 picture whose reference is a horizontal ramp: a vector's SATD depends on its x alone"""
    ref = np.tile(np.arange(40, 40 + 48 * 2, 2, dtype=np.uint8), (32, 1))
    return ref, hm.Pred(ref)


def test_b_choose_by_hand():
    ref, p = _flat_case()
    ref1 = np.ascontiguousarray(ref[:, ::-1])
    p1 = hm.Pred(ref1)
    src = np.zeros((32, 48), dtype=np.uint8)
    mv0, mv1 = np.array([[8, 0]] * 6), np.array([[-4, 4]] * 6)
    pm0, pm1 = np.array([[8, 0]] * 6), np.array([[0, 4]] * 6)  # b0 = 2, b1 = 7 + 1
    for mb, plan in enumerate(("L0", "L1", "bi", "L0", "L1", "bi")):
        X0, Y0 = (mb % 3) * 16, (mb // 3) * 16
        a0, a1 = p.block(X0, Y0, 8, 0), p1.block(X0, Y0, -4, 4)
        src[Y0:Y0 + 16, X0:X0 + 16] = dict(L0=a0, L1=a1, bi=hm.bipred(a0, a1))[plan]
    lam = np.full(6, 3)
    sat = lambda mb, q, mv: hm.satd16(src[(mb // 3) * 16:(mb // 3) * 16 + 16, (mb % 3) * 16:(mb % 3) * 16 + 16],  # noqa: E731
                                      q.block((mb % 3) * 16, (mb // 3) * 16, *mv))
    cost0 = np.array([sat(mb, p, (8, 0)) + 3 * 2 for mb in range(6)])
    cost1 = np.array([sat(mb, p1, (-4, 4)) + 3 * 8 for mb in range(6)])
    out, rec = hm.b_choose(src, p, p1, mv0, mv1, cost0, cost1, pm0, pm1, lam, 3, 2)
    assert [r["choice"] for r in rec] == ["L0", "L1", "bi", "L0", "L1", "bi"]
    assert out["dir"].tolist() == [1, 2, 3, 1, 2, 3]
    assert out["cost"].tolist() == [3 * 4, 3 * 10, 3 * 11, 3 * 4, 3 * 10, 3 * 11]
    assert out["bits"].tolist() == [4, 10, 11, 4, 10, 11]
    assert out["mvb"].tolist() == [[8, 0, 0, 0], [0, 0, -4, 4], [8, 0, -4, 4]] * 2


def test_b_merge_pass_by_hand():
    """P slice, 3x2 blocks in 32x32 CTBs, MaxNumMergeCand 2, lambda 2.  The source is the reference moved by two
    samples, (8, 0); block 0 has that motion, every other block the zero vector, each at 6 bits."""
    ref, p = _flat_case()
    src = np.tile(np.arange(44, 44 + 96, 2), (32, 1)).astype(np.uint8)
    dirs = np.ones(6, dtype=np.int64)
    mvs = np.zeros((6, 4), dtype=np.int64)
    mvs[0, :2] = (8, 0)
    lam = np.full(6, 2)
    bits = np.full(6, 6)
    sat = np.array([0, 512, 512, 512, 512, 512])  # the zero vector is off by 4 on every sample
    cost = sat + lam * bits
    out, rec = hm.b_merge_pass(src, [p], None, dirs, mvs, cost, bits, lam, 3, 2, 0, 2, 1)
    # block 0: no neighbours, list (zero, zero): the repeat is skipped, zero loses -> kept
    assert rec[0]["sources"] == ["Z", "Z"] and rec[0]["dups"] == [1] and rec[0]["kept"] and out["cost"][0] == 12
    # block 1: A1 = (8, 0) wins with merge_flag + one merge_idx bin
    assert rec[1]["list"] == [L0(8, 0), ZP] and rec[1]["winner_source"] == "A1" and rec[1]["moved"]
    assert out["mvb"][1].tolist() == [8, 0, 0, 0] and out["cost"][1] == 2 * 2 and out["bits"][1] == 2
    # block 2 reads the input field (Jacobi): A1 is still zero.  Quadrant 0 of the second CTB: A0 (block 4) is
    # available, and pruned.  Its own motion at j 0: re-priced from 6 bits to 2, not moved
    assert rec[2]["avail"]["A0"] and rec[2]["fired"] == ["A1-A0"] and rec[2]["sources"] == ["A1", "Z"]
    assert rec[2]["list"] == [ZP, ZP] and rec[2]["repriced"] and not rec[2]["moved"] and not rec[2]["kept"]
    assert out["cost"][2] == 512 + 2 * 2 and out["bits"][2] == 2 and out["mvb"][2].tolist() == [0, 0, 0, 0]
    # block 3: B1 (block 0) and B0 (block 1); quadrant 2's A0 is outside the picture.  B1 wins
    assert rec[3]["sources"] == ["B1", "B0"] and rec[3]["winner_source"] == "B1" and out["cost"][3] == 4
    # block 4, quadrant 3: B0 (block 2) is in the picture, in the next CTB.  A1 zero, B1 zero pruned, B2 (8, 0) wins
    assert rec[4]["inpic"]["B0"] and not rec[4]["avail"]["B0"] and rec[4]["fired"] == ["A1-B1"]
    assert rec[4]["list"] == [ZP, L0(8, 0)] and rec[4]["winner_source"] == "B2"
    assert out["cost"][4] == 0 + 2 * 2 and out["dir"][4] == 1 and out["mvb"][4].tolist() == [8, 0, 0, 0]
    # block 5: A1, B1 and B2 all zero
    assert rec[5]["fired"] == ["A1-B1", "A1-B2"] and rec[5]["list"] == [ZP, ZP] and rec[5]["repriced"]
    assert out["chg"].tolist() == [0, 1, 0, 1, 1, 0]
    assert out["cost"].tolist() == [12, 4, 516, 4, 4, 516] and out["bits"].tolist() == [6, 2, 2, 2, 2, 2]


def test_merge_refine_pass_by_hand():
    ref, p = _flat_case()
    src = np.tile(np.arange(44, 44 + 96, 2), (32, 1)).astype(np.uint8)  # the reference moved by (8, 0)
    mv = np.zeros((6, 2), dtype=np.int64)
    mv[0] = (8, 0)
    mv[3] = (8, 0)
    mv[4] = (8, 0)
    pm = np.zeros((6, 2), dtype=np.int64)
    lam = np.full(6, 2)
    sat = np.array([0, 512, 512, 0, 0, 512])
    mvd = np.array([hm.mvd_bits(mv[i], pm[i]) for i in range(6)])
    assert mvd.tolist() == [10, 2, 2, 10, 10, 2]
    cost = sat + 2 * mvd
    out, rec = hm.merge_refine_pass(src, p, mv, cost, pm, lam, 3, 2)
    # block 0: only zero; kept.  block 1: A1 (8, 0) at j 0, A0 = block 3 is (8, 0) too (no repeat), then zero:
    # its own vector at j 1, re-priced 2 bits -> 2 bins: not cheaper; A1 wins at 0 + 2 * 1
    assert rec[0]["list"] == [(0, 0)] and rec[0]["kept"] and out["cost"][0] == 20
    assert rec[1]["list"] == [(8, 0), (0, 0)] and rec[1]["sources"] == ["A1", "Z"] and rec[1]["winner_source"] == "A1"
    assert out["mv"][1].tolist() == [8, 0] and out["cost"][1] == 2
    # block 3: B1 (8, 0) is its own vector at j 0: 10 mvd bits become 1 bin, the vector stays
    assert rec[3]["repriced"] and out["mv"][3].tolist() == [8, 0] and out["cost"][3] == 2
    # block 4: A1 = (8, 0) its own at j 0 (re-priced to 2), B1 zero at j 1
    assert rec[4]["list"] == [(8, 0), (0, 0)] and out["cost"][4] == 2 and rec[4]["repriced"]
    # block 5: A1 (8, 0), B1 zero (its own), B2 (0, 0) repeat: A1 wins
    assert rec[5]["list"] == [(8, 0), (0, 0)] and out["mv"][5].tolist() == [8, 0]
    # without a predictor the mvd bits are those of the vector itself: the same here
    out2, _ = hm.merge_refine_pass(src, p, mv, cost, None, lam, 3, 2)
    assert np.array_equal(out2["mv"], out["mv"]) and np.array_equal(out2["cost"], out["cost"])


def test_merge_refine_takes_the_searched_vector_back():
    """The searched vector later in the list than a candidate that beat the search: when the search
    re-priced as merge is cheaper still, the block keeps the searched vector *and* gets that price."""
    ref, p = _flat_case()
    src = np.tile(np.arange(44, 44 + 96, 2), (32, 1)).astype(np.uint8)
    mv = np.zeros((6, 2), dtype=np.int64)
    mv[0] = (4, 0)   # A1 of block 1: half of the true motion, every sample off by 2
    mv[1] = (8, 0)   # block 1 searched the true motion, at many mvd bits
    mv[3] = (8, 0)   # ... which its A0 (block 3) offers at j 1
    pm = np.zeros((6, 2), dtype=np.int64)
    pm[1] = (-200, 90)
    lam = np.full(6, 20)
    s4 = hm.satd16(src[0:16, 16:32], p.block(16, 0, 4, 0))
    nbits = hm.mvd_bits(mv[1], pm[1])
    # A1 at j 0 beats the search (256 + 20 < 0 + 20 * 32); the search as merge at j 1 (0 + 20 * 2) beats A1
    assert (s4, nbits) == (256, 17 + 15)
    cost = np.array([0, 20 * nbits, 0, 0, 0, 0]) + 10 ** 6 * (np.arange(6) != 1)
    out, rec = hm.merge_refine_pass(src, p, mv, cost, pm, lam, 3, 2)
    assert rec[1]["list"] == [(4, 0), (8, 0), (0, 0)] and rec[1]["took_back"] and rec[1]["repriced"]
    assert out["mv"][1].tolist() == [8, 0] and out["cost"][1] == 20 * 2

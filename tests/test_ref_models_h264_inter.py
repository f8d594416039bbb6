"""tests/ref_models_h264_inter.py against code that is independent of it (no GPU needed):

* the host decoder (written from the clauses, csrc/host/h264_decoder.cc): the model's records,
  written by the host CAVLC / CABAC writers and decoded, must reconstruct to the model's own
  reconstruction bit for bit -- chroma MC, explicit weights, dequantisation, both inverse
  transforms, the chroma DC path, the record and level layouts;
* x264's decimation scores worked by hand from its run tables;
* sa8d / satd against a brute-force Kronecker Hadamard in float64;
* the input families of tests/test_gpu_h264_inter_model.py: the model alone must find in each
  what the family is there for, and stay under the near-tie cap, so the GPU test cannot turn out
  vacuous.
"""
import numpy as np
import pytest

import ref_models_h264_inter as M
from ref_models_me import Planes


# ------------------------------------------------------------------ the decoder anchor
def _anchor_case(host, wmb, hmb, qp, cqo, cabac, t8, seed, wp=None, trellis=0):
    from govideocompressor_amd.utils.h264_synth import random_stream
    W, H, nmb = wmb * 16, hmb * 16, wmb * hmb
    rng = np.random.default_rng(seed)
    cfg1 = dict(width=W, height=H, qp=qp, cabac=int(cabac), t8x8=int(t8), refs=1, constrained_intra=0, bit_depth=8)
    s1 = random_stream(host, W, H, 1, seed=seed, qp=qp, cabac=bool(cabac), t8x8=bool(t8))
    ps1 = host.parameter_sets(cfg1)
    assert s1.startswith(ps1)
    cfg = dict(cfg1, deblock=0, chroma_qp_offset=cqo, weightp=int(wp is not None))
    head = host.parameter_sets(cfg) + s1[len(ps1):]
    ref = host.decode(head)[0]
    ry, ru, rv = (np.asarray(ref[k]) for k in ("y_coded", "u_coded", "v_coded"))
    assert ry.shape == (H, W)
    # vectors: 16x16 and four-quadrant MBs, far enough to leave the picture on every side
    mv8 = rng.integers(-100, 101, (nmb, 4, 2))
    shape = rng.integers(0, 4, nmb)
    for mb in range(nmb):
        if shape[mb] == 0:
            mv8[mb, :] = mv8[mb, 0]
        elif shape[mb] == 1:
            mv8[mb, 1], mv8[mb, 3] = mv8[mb, 0], mv8[mb, 2]
        elif shape[mb] == 2:
            mv8[mb, 2], mv8[mb, 3] = mv8[mb, 0], mv8[mb, 1]
    mv8[0] = (-37, -45)  # up and left of the first MB: outside
    mv8[nmb - 1] = (51, 62)
    pl = Planes(ry)
    pred = np.zeros((nmb, 16, 16), np.int64)
    for mb in range(nmb):
        for q in range(4):
            full = pl.block((mb % wmb) * 16, (mb // wmb) * 16, int(mv8[mb, q, 0]), int(mv8[mb, q, 1]))
            ys, xs = slice((q >> 1) * 8, (q >> 1) * 8 + 8), slice((q & 1) * 8, (q & 1) * 8 + 8)
            pred[mb, ys, xs] = full[ys, xs]
    amp = max(2.0, 0.8 * 0.625 * 2 ** (qp / 6))
    tile = pred.reshape(hmb, wmb, 16, 16).transpose(0, 2, 1, 3).reshape(H, W)
    # every other MB also gets a smooth 8x8-wide term (those prefer the 8x8 transform)
    smooth = np.kron(rng.normal(0, amp, (hmb * 2, wmb * 2)), np.ones((8, 8)))
    smooth *= np.kron((np.arange(nmb).reshape(hmb, wmb) % 2 == 0), np.ones((16, 16)))
    sy = np.clip(np.round(tile + rng.laplace(0, amp, (H, W)) + smooth), 0, 255).astype(np.uint8)
    su = np.clip(np.round(ru + rng.laplace(0, amp, ru.shape)), 0, 255).astype(np.uint8)
    sv = np.clip(np.round(rv + rng.laplace(0, amp, rv.shape)), 0, 255).astype(np.uint8)
    aq = rng.integers(-3, 4, nmb)
    big = np.full(nmb, 1 << 20)
    out = M.encode_inter_slot(wmb, hmb, sy, su, sv, pred.reshape(nmb, 256), [ru], [rv], np.zeros(nmb, np.int64), big, qp,
                              mv8=mv8, aq=aq, chroma_qp_offset=cqo, wp=wp, t8=int(t8), trellis=trellis)
    fp = dict(idr=0, qp=qp, frame_num=1)
    if wp is not None:
        fp["wp"] = [wp[2], wp[7], wp[0], wp[1], wp[3], wp[4], wp[5], wp[6]]
    nal, _ = host.write_slice(cfg, fp, out["hdr"], out["coef"])
    pics = host.decode(head + nal)
    assert len(pics) == 2
    return out, pics[1]


@pytest.mark.parametrize("wmb,hmb", [(3, 2), (5, 3)])
@pytest.mark.parametrize("qp,cqo", [(12, 0), (26, -3), (40, 4)])
@pytest.mark.parametrize("cabac,t8", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_model_reconstruction_is_the_decoders(host, wmb, hmb, qp, cqo, cabac, t8):
    out, pic = _anchor_case(host, wmb, hmb, qp, cqo, cabac, t8, seed=100 * qp + 10 * wmb + 2 * cabac + t8)
    assert out["work"].all()
    assert out["coef"].any(axis=1).sum() >= out["work"].sum() // 2, "too few MBs with levels to mean anything"
    if t8:
        assert (out["flags"] == M.MBF_T8x8).any() and (out["flags"] == 0).any()
    for k, name in (("rec_y", "y_coded"), ("rec_u", "u_coded"), ("rec_v", "v_coded")):
        np.testing.assert_array_equal(np.asarray(pic[name]), out[k], err_msg=name)


@pytest.mark.parametrize("trellis", [0, 2])
def test_model_reconstruction_with_weights_and_trellis(host, trellis):
    """explicit weights of list-0 entry 0 (luma and both chroma components, with offsets), and the
    trellis levels: whatever levels are chosen, the reconstruction is the decoder's"""
    wp = [37, -3, 5, 29, 2, 70, -4, 6]
    out, pic = _anchor_case(host, 5, 3, 30, 2, 1, 1, seed=77 + trellis, wp=wp, trellis=trellis)
    for k, name in (("rec_y", "y_coded"), ("rec_u", "u_coded"), ("rec_v", "v_coded")):
        np.testing.assert_array_equal(np.asarray(pic[name]), out[k], err_msg=name)


# ------------------------------------------------------------------ decimation scores by hand
def _lv(n, **at):
    v = [0] * n
    for k, x in at.items():
        v[int(k[1:])] = x
    return v


@pytest.mark.parametrize("levels,want", [
    # x264 ds_table4 = 3 2 2 1 1 1 0 ...: the price of a +-1 by the zeros between it and the level below
    (_lv(16), 0),
    (_lv(16, p0=1), 3),                      # run 0
    (_lv(16, p1=-1), 2),                     # one zero below it
    (_lv(16, p2=1), 2),
    (_lv(16, p3=1), 1), (_lv(16, p5=-1), 1),
    (_lv(16, p6=1), 0), (_lv(16, p15=1), 0),
    (_lv(16, p0=1, p1=1), 6),                # 3 + 3
    (_lv(16, p0=1, p2=-1), 5),               # 3 + (run 1) 2
    (_lv(16, p0=1, p4=1), 4),                # 3 + (run 3) 1
    (_lv(16, p0=-1, p7=1), 3),               # 3 + (run 6) 0
    (_lv(16, p2=1, p3=1, p9=-1), 2 + 3 + 1),  # runs 2, 0, 5
    (_lv(16, p0=2), 9), (_lv(16, p15=-2), 9), (_lv(16, p0=1, p1=1, p9=-2), 9),  # a single +-2 anywhere
])
def test_decimate_score_4x4_by_hand(levels, want):
    assert M.decimate_score(levels, M.DS4) == want


def test_decimate_score_chroma_ac_starts_at_scan_1():
    """decimate_score15: the DC is coded elsewhere, runs count from scan position 1"""
    ac = _lv(16, p0=5, p1=1, p3=-1)           # the DC level is not part of it
    assert M.decimate_score(ac[1:], M.DS4) == 3 + 2
    assert M.decimate_score(_lv(16, p4=1)[1:], M.DS4) == 1   # three zeros (1, 2, 3) below it


@pytest.mark.parametrize("levels,want", [
    # x264 ds_table8 = 3 x4, 2 x8, 1 x12, 0 ...
    (_lv(64), 0),
    (_lv(64, p0=1), 3), (_lv(64, p3=-1), 3), (_lv(64, p4=1), 2), (_lv(64, p11=1), 2), (_lv(64, p12=1), 1),
    (_lv(64, p23=-1), 1), (_lv(64, p24=1), 0), (_lv(64, p63=1), 0),
    (_lv(64, p15=1, p16=-1), 1 + 3),          # across 15 / 16: run 0, not a fresh start at 16
    (_lv(64, p14=1, p17=1), 1 + 3),           # run 2 across 15 / 16
    (_lv(64, p10=1, p20=-1), 2 + 2),          # run 9 across 15 / 16
    (_lv(64, p31=1, p32=1), 0 + 3),           # across 31 / 32
    (_lv(64, p28=-1, p36=1), 0 + 2),          # run 7 across 31 / 32
    (_lv(64, p47=1, p48=1), 0 + 3),           # across 47 / 48
    (_lv(64, p40=1, p60=1), 0 + 1),           # run 19 across 47 / 48
    (_lv(64, p0=1, p20=1, p40=-1, p60=1), 3 + 1 + 1 + 1),  # runs 0, 19, 19, 19: every boundary
    (_lv(64, p5=1, p50=-1), 2 + 0),           # run 44 over two boundaries
    (_lv(64, p33=2), 9), (_lv(64, p0=1, p63=-2), 9),
])
def test_decimate_score_64_by_hand(levels, want):
    assert M.decimate_score(levels, M.DS8) == want


def test_chunk_blind_score_differs_where_a_run_crosses():
    """the helper that finds inputs for the GPU test really is the wrong score there"""
    assert M.score64_chunk_blind(_lv(64, p15=1, p16=-1)) == 1 + 1
    assert M.score64_chunk_blind(_lv(64, p3=1, p9=1)) == M.decimate_score(_lv(64, p3=1, p9=1), M.DS8)


# ------------------------------------------------------------------ sa8d / satd
def _kron_hadamard_abs(block):
    n = block.shape[0]
    h = np.array([[1.0]])
    while h.shape[0] < n:
        h = np.kron(np.array([[1.0, 1.0], [1.0, -1.0]]), h)
    return np.abs(np.kron(h, h) @ block.astype(np.float64).reshape(-1)).sum()


def test_sa8d_and_satd_against_kronecker_hadamard():
    rng = np.random.default_rng(5)
    cases = [rng.integers(-255, 256, (16, 16)) for _ in range(20)] + [rng.integers(-3, 4, (16, 16)) for _ in range(10)]
    yy, xx = np.mgrid[0:16, 0:16]
    cases += [np.full((16, 16), 255), np.full((16, 16), -255), ((xx + yy) % 2 * 510 - 255), ((xx // 4 + yy // 8) % 2 * 510 - 255)]
    for res in cases:
        res = res.astype(np.int64)
        satd = sum(int(_kron_hadamard_abs(res[y:y + 4, x:x + 4])) // 2 for y in range(0, 16, 4) for x in range(0, 16, 4))
        sa8d = sum((int(_kron_hadamard_abs(res[y:y + 8, x:x + 8])) + 2) // 4 for y in range(0, 16, 8) for x in range(0, 16, 8))
        assert M.satd_mb(res) == satd
        assert M.sa8d_mb(res) == sa8d


def test_transforms_invert():
    """forward then the spec's inverse returns the residual (times the transform's gain, which the
    scaling removes): with all-pass scaling the 4x4 pair is exact on multiples of the gain"""
    rng = np.random.default_rng(6)
    x = rng.integers(-255, 256, (50, 4, 4))
    w = M.forward4(x)
    # Ci (W * [inverse norms]) : use the identity Cf^-1 via float to confirm the integer butterfly
    cf = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], np.float64)
    back = np.linalg.inv(cf) @ w.astype(np.float64) @ np.linalg.inv(cf.T)
    np.testing.assert_allclose(back, x, atol=1e-9)
    x8 = rng.integers(-32, 33, (50, 8, 8)) * 64     # multiples of 64: the shifts of both passes are exact
    t8 = np.array([[8, 8, 8, 8, 8, 8, 8, 8], [12, 10, 6, 3, -3, -6, -10, -12], [8, 4, -4, -8, -8, -4, 4, 8],
                   [10, -3, -12, -6, 6, 12, 3, -10], [8, -8, -8, 8, 8, -8, -8, 8], [6, -12, 3, 10, -10, -3, 12, -6],
                   [4, -8, 8, -4, -4, 8, -8, 4], [3, -6, 10, -12, 12, -10, 6, -3]], np.float64) / 8
    np.testing.assert_allclose(M.forward8(x8), t8 @ x8 @ t8.T, atol=1e-9)


# ------------------------------------------------------------------ the GPU test's inputs are not vacuous
@pytest.mark.parametrize("wmb,hmb,bmode,t8,trellis,aq", M.grid())
def test_families_hold_what_they_are_for(wmb, hmb, bmode, t8, trellis, aq):
    seed = M.SEEDS[(wmb, hmb, bmode, aq)]
    ties = work = 0
    for fam in M.families(bmode, trellis):
        c = M.cached_case(fam, wmb, hmb, bmode, seed, aq, trellis)
        outs = M.cached_model(fam, wmb, hmb, bmode, seed, aq, t8, trellis, 0xA5)
        n = M.family_counts(c, outs)
        assert M.missing_counts(fam, n, wmb * hmb, t8) == [], (fam, n)
        assert len(set(int(q) for q in c["qp"])) == 2
        if aq:
            q = c["mbqp"]
            assert all(len(set(q[b, i:i + 4])) == 4 for b in range(2) for i in range(0, 12, 4) if fam == "near")
            assert fam == "near" or ((q == 0).any() and (q == 51).any())
        ties += n["tie"]
        work += n["work"]
    if trellis:
        assert ties <= M.TIE_CAP * work, (ties, work)
    else:
        assert ties == 0

"""``hv::rd_cbf_tu`` (csrc/kernels/hevc_rdcbf.h) through its stand-alone probe launch
(``hip.hevc_rd_cbf_probe``) against the numpy model of tests/ref_models_hevc_rdcbf.py: levels,
reconstructed samples, flag, D0, D1 and Rb of every block must be equal, no tolerance, no block
left out.

One case per TU size (4 .. 32), bit depth (8 / 10) and QpY in {12, 27, 42} (Qp' = QpY + 6 (bit
depth - 8); lamq from the model's table at rd_cbf_lambda 1.0 unless the variant says otherwise).
In each case every variant -- the dead zone alone, with sign data hiding, RDOQ level 1 and 2 at
rdoq_lambda 0.5, and sign data hiding with RDOQ level 2 at rdoq_lambda 1.5 and rd_cbf_lambda 2.0
-- is one launch on the same blocks:

* source = prediction; the largest residual of both signs (source 2^bd - 1 against prediction 0
  and the reverse: D0 = n^2 (2^bd - 1)^2, at 32x32 and 10 bits 1,071,645,696, times 256 in the
  comparison); a full-range checkerboard against its inverse;
* single planted levels (the inverse transform of a one-hot level 1, -1, 2 and -5 on mid grey) at
  the first, a middle and the last scan position;
* 256 / 128 / 64 / 64 random blocks at 4x4 / 8x8 / 16x16 / 32x32: a textured source, the
  prediction off by a smooth error (a plane worth up to SMOOTH_STEPS quantiser steps of DC and
  first-order coefficients) plus white noise whose amplitude cycles over NOISE_STEPS quantiser
  steps from block to block.  The amplitudes are per size, found with the model (they scale with
  the step, so one set serves every Qp'): the check weighs about 0.09 step^2 per bit, so what it
  clears is a handful of lone +-1 levels; under 0.3 steps of noise the dead zone leaves none, above
  0.5 a 16x16 or 32x32 TU holds too many to go, and a 4x4 TU goes mostly on one high-frequency
  level (its share of cleared blocks peaks near 0.3 around 0.44 steps, hence the larger sample).
  Before the GPU is used each case asserts on the model alone that every variant at
  rd_cbf_lambda 1.0 clears between 20 % and 80 % of its random blocks (blocks without levels
  counted) -- a kernel that never or always clears cannot pass -- and that the last variant
  clears some.

The hand cases of tests/test_ref_models_hevc_rdcbf.py run through the probe in a test of their
own (their lamq values are not a table's).
"""
import functools

import numpy as np
import pytest

import ref_models_hevc_rdcbf as rc
import ref_models_hevc_rdoq as rq

pytestmark = pytest.mark.gpu

NRAND = {2: 256, 3: 128, 4: 64, 5: 64}  # random blocks of a case, per log2 of the TU size
# noise amplitudes of the random blocks in quantiser steps (cycled), per log2 of the TU size, and
# the smooth error's amplitude in coefficient steps
NOISE_STEPS = {2: (0.42, 0.46), 3: (0.3, 0.35, 0.4, 0.45), 4: (0.25, 0.3, 0.35, 0.4, 0.45, 0.5),
               5: (0.2, 0.25, 0.35, 0.4, 0.45, 0.5)}
SMOOTH_STEPS = {2: 0.3, 3: 0.6, 4: 1.0, 5: 1.0}
QPYS = (12, 27, 42)
CASES = [(lg, bd, qpy) for lg in (2, 3, 4, 5) for bd in (8, 10) for qpy in QPYS]
# (name, sdh, rdoq level, rdoq_lambda, rd_cbf_lambda)
VARIANTS = [("dz", False, 0, 0.5, 1.0), ("sdh", True, 0, 0.5, 1.0), ("rdoq1", False, 1, 0.5, 1.0),
            ("rdoq2", False, 2, 0.5, 1.0), ("sdh-rdoq2-l2", True, 2, 1.5, 2.0)]
POISON16, POISON32, POISON64 = -21846, -1431655766, -6148914691236517206


def _case_id(c):
    return f"{1 << c[0]}-bd{c[1]}-qpy{c[2]}"


@functools.lru_cache(maxsize=1)
def _dct32():
    from govideocompressor_amd.ops import native
    return np.asarray(native.host().table("hevc_dct32"), dtype=np.int64).reshape(32, 32)


def _qstep(qp):
    """quantiser step of Qp' in sample units at any TU size (the transforms are orthonormal up to
    the standard's scaling)"""
    return 2.0 ** ((qp - 4) / 6.0)


def _blocks(lg, bd, qpy):
    """(src, pred) uint16 [nblk, n, n] of a case and the index of its first random block"""
    n, maxv, qp = 1 << lg, (1 << bd) - 1, qpy + 6 * (bd - 8)
    rng = np.random.default_rng(10000 * lg + 100 * bd + qpy)
    C = rq.matrix(_dct32(), lg)
    order, _ = rq.positions(0, lg)
    mid = 1 << (bd - 1)
    full, zero = np.full((n, n), maxv, dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    chk = (np.add.outer(np.arange(n), np.arange(n)) & 1) * maxv
    src, pred = [np.full((n, n), mid), full, zero, chk], [np.full((n, n), mid), zero, full, maxv - chk]
    for p in (0, n * n // 2 - 3, n * n - 1):
        x, y = order[p]
        for l in (1, -1, 2, -5):
            one = np.zeros((n, n), dtype=np.int64)
            one[y, x] = l
            res = np.clip(rq.inverse(rq.dequant(one, lg, bd, qp), C, bd), -mid, mid - 1)
            pred.append(np.full((n, n), mid))
            src.append(mid + res)
    first = len(src)
    yy, xx = np.mgrid[0:n, 0:n] / float(n)
    step = _qstep(qp)
    for k in range(NRAND[lg]):
        tex = mid + 0.3 * mid * np.sin(2 * np.pi * (xx * rng.uniform(0.5, 3) + yy * rng.uniform(0.5, 3)) + rng.uniform(0, 6.28))
        s = np.clip(np.rint(tex + rng.normal(0.0, 0.02 * mid, size=(n, n))), 0, maxv).astype(np.int64)
        # (a flat error e gives a DC coefficient of n e: the plane is scaled in coefficient steps)
        smooth = SMOOTH_STEPS[lg] * step / n * (rng.uniform(-1, 1) + rng.uniform(-1, 1) * (xx - 0.5) + rng.uniform(-1, 1) * (yy - 0.5))
        noise = rng.normal(0.0, NOISE_STEPS[lg][k % len(NOISE_STEPS[lg])] * step, size=(n, n))
        src.append(s)
        pred.append(np.clip(np.rint(s - smooth - noise), 0, maxv).astype(np.int64))
    return np.stack(src).astype(np.uint16), np.stack(pred).astype(np.uint16), first


@functools.lru_cache(maxsize=2)
def expected(case):
    """(src, pred, first random block, {variant name: (levels, samples, flags, terms [nblk, 3])})"""
    lg, bd, qpy = case
    qp = qpy + 6 * (bd - 8)
    src, pred, first = _blocks(lg, bd, qpy)
    out = {}
    for name, sdh, rdoq, rlam, clam in VARIANTS:
        lamq = rc.lamq_table(clam, bd)[qpy]
        r = [rc.rd_cbf_tu(s, p, _dct32(), lg, bd, qp, lamq, sdh, rdoq, rq.lam_of(rlam) if rdoq else 0) for s, p in zip(src, pred)]
        out[name] = (np.stack([v[0] for v in r]), np.stack([v[1] for v in r]), np.array([v[2] for v in r]),
                     np.array([v[3:6] for v in r], dtype=np.int64))
    return src, pred, first, out


def cleared_fraction(case, name):
    """share of the case's random blocks the check cleared (blocks the quantiser itself emptied
    count as not cleared: terms D1 = D0 and Rb = 0 mark them)"""
    src, pred, first, out = expected(case)
    lev, _, flag, terms = out[name]
    had = terms[first:, 2] > 0
    return float((had & (flag[first:] == 0)).mean()), float(had.mean())


def assert_both_outcomes(case):
    for name, *_, clam in VARIANTS:
        frac, had = cleared_fraction(case, name)
        if clam == 1.0:
            assert 0.2 <= frac <= 0.8, (case, name, "share of random blocks cleared", frac, had)
        else:
            assert 0.0 < frac <= had, (case, name, frac, had)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_probe_equals_model(case):
    import torch

    from govideocompressor_amd.ops import native
    lg, bd, qpy = case
    n, qp = 1 << lg, qpy + 6 * (bd - 8)
    src, pred, first, out = expected(case)
    assert_both_outcomes(case)
    nblk = src.shape[0]
    hip = native.hip()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_src = torch.from_numpy(src.astype(np.int16)).to(dev)
    d_pred = torch.from_numpy(pred.astype(np.int16)).to(dev)
    d_lev = torch.empty((nblk, n, n), dtype=torch.int16, device=dev)
    d_rec = torch.empty((nblk, n, n), dtype=torch.int16, device=dev)
    d_flag = torch.empty((nblk,), dtype=torch.int32, device=dev)
    d_terms = torch.empty((nblk, 3), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, sdh, rdoq, rlam, clam in VARIANTS:
        d_lev.fill_(POISON16)
        d_rec.fill_(POISON16)
        d_flag.fill_(POISON32)
        d_terms.fill_(POISON64)
        hip.hevc_rd_cbf_probe(nblk, d_src.data_ptr(), d_pred.data_ptr(), d_lev.data_ptr(), d_rec.data_ptr(), d_flag.data_ptr(),
                              d_terms.data_ptr(), lg, bd, qp, int(sdh), rdoq, rq.lam_of(rlam) if rdoq else 0,
                              rc.lamq_table(clam, bd)[qpy], stream)
        torch.cuda.synchronize(dev)
        lev = d_lev.cpu().numpy().astype(np.int64)
        rec = d_rec.cpu().numpy().astype(np.int64) & 0xFFFF
        flag, terms = d_flag.cpu().numpy(), d_terms.cpu().numpy()
        wl, wr, wf, wt = out[name]
        for k, what in enumerate(("D0", "D1", "Rb")):
            bad = np.flatnonzero(terms[:, k] != wt[:, k])
            assert bad.size == 0, (name, what, bad[:8].tolist(), terms[bad[:4], k].tolist(), wt[bad[:4], k].tolist())
        assert np.array_equal(flag, wf), (name, "flag", np.flatnonzero(flag != wf)[:8].tolist())
        bad = np.flatnonzero((lev != wl).any(axis=(1, 2)))
        assert bad.size == 0, (name, "levels", bad[:8].tolist(), np.argwhere(lev[bad[0]] != wl[bad[0]])[:4].tolist())
        bad = np.flatnonzero((rec != wr).any(axis=(1, 2)))
        assert bad.size == 0, (name, "samples", bad[:8].tolist())


def _probe(src, pred, lg, bd, qp, lamq, sdh=0, rdoq=0, rdoq_lam=0):
    """the probe on blocks [nblk, n, n]: (levels, samples, flags, terms)"""
    import torch

    from govideocompressor_amd.ops import native
    n, nblk = 1 << lg, len(src)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_src = torch.from_numpy(np.asarray(src).astype(np.int16)).to(dev)
    d_pred = torch.from_numpy(np.asarray(pred).astype(np.int16)).to(dev)
    d_lev = torch.full((nblk, n, n), POISON16, dtype=torch.int16, device=dev)
    d_rec = torch.full((nblk, n, n), POISON16, dtype=torch.int16, device=dev)
    d_flag = torch.full((nblk,), POISON32, dtype=torch.int32, device=dev)
    d_terms = torch.full((nblk, 3), POISON64, dtype=torch.int64, device=dev)
    native.hip().hevc_rd_cbf_probe(nblk, d_src.data_ptr(), d_pred.data_ptr(), d_lev.data_ptr(), d_rec.data_ptr(),
                                   d_flag.data_ptr(), d_terms.data_ptr(), lg, bd, qp, sdh, rdoq, rdoq_lam, lamq,
                                   torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return (d_lev.cpu().numpy().astype(np.int64), d_rec.cpu().numpy().astype(np.int64) & 0xFFFF, d_flag.cpu().numpy(),
            d_terms.cpu().numpy())


def _planted(lg, bd, qp, placed):
    """(src, pred) on mid grey whose dead-zone levels are `placed` = {scan position: level}"""
    n, mid = 1 << lg, 1 << (bd - 1)
    order, _ = rq.positions(0, lg)
    lev = np.zeros((n, n), dtype=np.int64)
    for p, v in placed.items():
        x, y = order[p]
        lev[y, x] = v
    res = rq.inverse(rq.dequant(lev, lg, bd, qp), rq.matrix(_dct32(), lg), bd)
    pred = np.full((n, n), mid, dtype=np.int64)
    got = rq.transform_quant_block(res, _dct32(), lg, bd, qp, False)[0]
    assert np.array_equal(got, lev), "the planted levels do not survive the quantiser"
    return pred + res, pred


def test_probe_on_the_hand_cases():
    """the cases of tests/test_ref_models_hevc_rdcbf.py, the numbers computed there"""
    f4 = np.full((4, 4), 1, dtype=np.int64)
    # flat r = 4 at Qp' 28: D0 256, D1 0, Rb 72; kept up to lamq 799
    for lamq, keep in ((0, 1), (799, 1), (800, 0), (5000, 0)):
        lev, rec, flag, terms = _probe([104 * f4], [100 * f4], 2, 8, 28, lamq)
        assert terms.tolist() == [[256, 0, 72]] and flag.tolist() == [keep]
        assert lev[0, 0, 0] == keep and np.count_nonzero(lev) == keep and np.array_equal(rec[0], (104 if keep else 100) * f4)
    # |r| = 3 at Qp' 27 next to the range's ends: the clip makes D1 0; away from them it is 16
    for lamq, keep_edge, keep_mid in ((399, 1, 1), (420, 1, 0), (449, 1, 0), (450, 0, 0)):
        lev, rec, flag, terms = _probe([255 * f4, 0 * f4, 103 * f4, 97 * f4], [252 * f4, 3 * f4, 100 * f4, 100 * f4], 2, 8, 27, lamq)
        assert terms.tolist() == [[144, 0, 72], [144, 0, 72], [144, 16, 72], [144, 16, 72]]
        assert flag.tolist() == [keep_edge, keep_edge, keep_mid, keep_mid]
        want = [255 if keep_edge else 252, 0 if keep_edge else 3, 104 if keep_mid else 100, 96 if keep_mid else 100]
        assert [np.array_equal(rec[b], want[b] * f4) for b in range(4)] == [True] * 4
    # a single +-1 at the last position of a 4x4: Rb = 287; the tie 256 (D0 - D1) = 297 lamq cannot
    # be planted through the transform, the model's own terms place lamq on both sides of it
    for sign in (1, -1):
        src, pred = _planted(2, 8, 28, {15: sign})
        want = rc.rd_cbf_tu(src, pred, _dct32(), 2, 8, 28, 0)
        assert want[5] == 287 and want[2] == 1
        edge = 256 * (want[3] - want[4]) // 297  # the smallest lamq that clears, or one below it
        for lamq in (edge - 1, edge, edge + 1):
            w = rc.rd_cbf_tu(src, pred, _dct32(), 2, 8, 28, lamq)
            lev, rec, flag, terms = _probe([src], [pred], 2, 8, 28, lamq)
            assert terms.tolist() == [list(w[3:6])] and flag.tolist() == [w[2]]
            assert np.array_equal(lev[0], w[0]) and np.array_equal(rec[0], w[1])
        assert rc.rd_cbf_tu(src, pred, _dct32(), 2, 8, 28, edge - 1)[2] == 1 and rc.rd_cbf_tu(src, pred, _dct32(), 2, 8, 28, edge + 1)[2] == 0
    # group 2 of an 8x8 with an empty group 1 (Rb 433), with a filled one, and pmax in group 3
    for placed, rb in (({37: 2, 3: -1}, 433), ({37: 2, 3: -1, 20: 1}, 433 - 8 + 18 + 48 + 135), ({48: 1}, 188)):
        src, pred = _planted(3, 8, 28, placed)
        w = rc.rd_cbf_tu(src, pred, _dct32(), 3, 8, 28, 92)
        assert w[5] == rb
        lev, rec, flag, terms = _probe([src], [pred], 3, 8, 28, 92)
        assert terms.tolist() == [list(w[3:6])] and flag.tolist() == [w[2]] and np.array_equal(lev[0], w[0])


# flat residuals r on 100 that lie exactly on the tie 256 (D0 - D1) = lamq (Rb + 10):
# (log2n, bit depth, Qp', r, lamq).  The first by hand: at Qp' 16 a 4x4 level is 128 r 2^14 / 2^21
# = r, reconstructed exactly, so D0 = 16 * 441 = 7056, D1 = 0, Rb = rate(21, False, 0) = 22 + 16 +
# (24 + 22 + 16 * 11) + 24 = 284 and 256 * 7056 = 1806336 = 6144 * 294
TIES = [(2, 8, 16, 21, 6144), (2, 10, 16, 21, 6144), (2, 8, 24, 24, 10240), (2, 8, 43, 32, 47104), (3, 8, 22, 21, 24576),
        (3, 8, 30, 47, 122880)]


@pytest.mark.parametrize("lg,bd,qp,r,lamq", TIES)
def test_an_exact_tie_clears_on_the_gpu(lg, bd, qp, r, lamq):
    n = 1 << lg
    pred = np.full((n, n), 100, dtype=np.int64)
    src = pred + r
    for lq, keep in ((lamq - 1, 1), (lamq, 0)):
        w = rc.rd_cbf_tu(src, pred, _dct32(), lg, bd, qp, lq)
        assert w[2] == keep and w[5] > 0
        assert (256 * (w[3] - w[4]) == lamq * (w[5] + 10)), "not a tie"
        lev, rec, flag, terms = _probe([src], [pred], lg, bd, qp, lq)
        assert terms.tolist() == [list(w[3:6])] and flag.tolist() == [keep]
        assert np.array_equal(lev[0], w[0]) and np.array_equal(rec[0], w[1])
        assert np.array_equal(rec[0], pred if not keep else w[1]) and (lev[0] != 0).any() == bool(keep)


def test_probe_refuses_parameters_outside_its_domain():
    import torch

    from govideocompressor_amd.ops import native
    hip = native.hip()
    t = torch.zeros(4096, dtype=torch.int64, device="cuda")
    ok = dict(log2n=3, bd=8, qp=30, sdh=0, rdoq=1, rdoq_lam=368, lamq=92)
    for bad in (dict(log2n=6), dict(log2n=1), dict(bd=9), dict(qp=52), dict(qp=-1), dict(rdoq=3), dict(rdoq_lam=1473),
                dict(rdoq_lam=-1), dict(lamq=-1), dict(lamq=(1 << 23) + 1), dict(nblk=0)):
        kw = {**dict(nblk=1), **ok, **bad}
        with pytest.raises(ValueError):
            hip.hevc_rd_cbf_probe(kw.pop("nblk"), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                  t.data_ptr(), stream=0, **kw)

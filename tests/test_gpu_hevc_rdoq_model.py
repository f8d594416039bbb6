"""``hv::transform_quant_block`` (csrc/kernels/hevc_common.h, with the RDOQ passes of
hevc_rdoq.h) through its stand-alone probe launch (``hip.hevc_tq_probe``) against the numpy model
of tests/ref_models_hevc_rdoq.py: levels, reconstructed residual and flag of every block must be
equal, no tolerance, no block left out.

One case per TU size, legal mode (DST only at 4x4 intra; scans 1 / 2 only where 7.4.9.11 allows
them: intra 4x4 and 8x8), bit depth and Qp' in {4, 22, 37, 51 + 6 (bd - 8)}; in each case every
variant of rdoq 0 / 1 / 2, sign data hiding off / on, rdoq_lambda 0.5 / 1.5 and, at rdoq 0 and
sizes 16 / 32, both transform forms (matrix cores / LDS wave products: today's quantiser, pinned)
is one launch on the same 64 blocks:

* all zero; flat DC of both signs; a +-(2^bd - 1) checkerboard in both phases (the level and
  16-bit clips);
* single planted coefficients (the inverse transform of a one-hot level 1, 2 and -5) at the
  first, a middle and the last scan position;
* white noise at 0.35 / 0.6 / 1.0 / 1.6 quantiser steps (clipped to the sample range), so most
  levels fall in 0..3 at the case's QP.

Before the GPU is used each case asserts on the model alone that RDOQ changes something there:
level 1 against level 0 in some block, and level 2 against level 1 at sizes >= 8.
"""
import functools

import numpy as np
import pytest

import ref_models_hevc_rdoq as rq

pytestmark = pytest.mark.gpu

NBLK = 64
NOISE_STEPS = (0.35, 0.6, 1.0, 1.6)
POISON_LEV, POISON_REC, POISON_FLAG = -21846, -1431655766, -5


# (log2n, intra, dst, scan)
MODES = ([(2, True, True, s) for s in range(3)] + [(2, True, False, s) for s in range(3)] + [(2, False, False, 0)] +
         [(3, True, False, s) for s in range(3)] + [(3, False, False, 0)] +
         [(lg, intra, False, 0) for lg in (4, 5) for intra in (True, False)])
CASES = [(lg, intra, dst, scan, bd, qp) for lg, intra, dst, scan in MODES for bd in (8, 10)
         for qp in (4, 22, 37, 51 + 6 * (bd - 8))]


def _case_id(c):
    lg, intra, dst, scan, bd, qp = c
    return f"{1 << lg}-{'intra' if intra else 'inter'}{'-dst' if dst else ''}-scan{scan}-bd{bd}-qp{qp}"


def _variants(lg):
    out = []
    for sdh in (False, True):
        for mfma in ((True, False) if lg >= 4 else (True,)):
            out.append((0, sdh, 0.5, mfma))
        for rdoq in (1, 2):
            for lam in (0.5, 1.5):
                out.append((rdoq, sdh, lam, True))
    return out


def _blocks(dct32, lg, dst, scan, bd, qp):
    """the 64 residual blocks of a case, int32 [64, n, n]"""
    n, maxv = 1 << lg, (1 << bd) - 1
    rng = np.random.default_rng(1000 * lg + 100 * scan + 10 * bd + qp + (7 if dst else 0))
    qstep = (1 << (14 + qp // 6)) / rq.QUANT_SCALE[qp % 6]
    C = rq.matrix(dct32, lg, dst)
    order, _ = rq.positions(scan, lg)
    out = [np.zeros((n, n), dtype=np.int64)]
    dc = min(maxv, max(1, int(round(3.3 * qstep))))
    out += [np.full((n, n), dc), np.full((n, n), -dc)]
    chk = (np.add.outer(np.arange(n), np.arange(n)) & 1) * 2 - 1
    out += [chk * maxv, -chk * maxv]
    for p in (0, n * n // 2 - 3, n * n - 1):
        x, y = order[p]
        for l in (1, 2, -5):
            one = np.zeros((n, n), dtype=np.int64)
            one[y, x] = l
            out.append(np.clip(rq.inverse(rq.dequant(one, lg, bd, qp), C, bd), -maxv, maxv))
    k = 0
    while len(out) < NBLK:
        sigma = NOISE_STEPS[k % len(NOISE_STEPS)] * qstep
        out.append(np.clip(np.rint(rng.normal(0.0, sigma, size=(n, n))), -maxv, maxv).astype(np.int64))
        k += 1
    return np.stack(out).astype(np.int32)


@functools.lru_cache(maxsize=2)
def _dct32():
    from govideocompressor_amd.ops import native
    return np.asarray(native.host().table("hevc_dct32"), dtype=np.int64).reshape(32, 32)


def expected(case):
    """(blocks, {variant: (levels [64, n, n], reconstruction [64, n, n], flags [64])}) of the model;
    the transform form is no parameter of the model"""
    lg, intra, dst, scan, bd, qp = case
    dct32 = _dct32()
    res = _blocks(dct32, lg, dst, scan, bd, qp)
    C = rq.matrix(dct32, lg, dst)
    coefs = [rq.forward(r, C, lg, bd) for r in res]
    out = {}
    for rdoq, sdh, lam, mfma in _variants(lg):
        if not mfma:
            out[(rdoq, sdh, lam, mfma)] = out[(rdoq, sdh, lam, True)]
            continue
        levs, recs, flags = [], [], []
        for c in coefs:
            lev = rq.quantise(c, lg, bd, qp, intra, scan, sdh, rdoq, rq.lam_of(lam))
            nz = bool(lev.any())
            levs.append(lev)
            recs.append(rq.inverse(rq.dequant(lev, lg, bd, qp), C, bd) if nz else np.zeros_like(lev))
            flags.append(int(nz))
        out[(rdoq, sdh, lam, mfma)] = (np.stack(levs), np.stack(recs), np.array(flags))
    return res, out


def assert_rdoq_matters(case, out):
    """Level 1 differs from level 0 in some block and, at sizes >= 8, level 2 from level 1.

    One family of variants cannot: 16x16 and 32x32 at 10 bits and Qp' 4 have a quantiser step of 2
    and 1 coefficient units, so every coefficient is a whole or a half level.  At rdoq_lambda 0.5
    (lam 184) a whole level never moves (D grows by 65536, the dearest level-1 rate, 272 at the
    last position of a 32x32 TU, is worth 50048) and a half level goes where the dead zone sends
    it (both neighbours have D = 16384, the smaller one has the smaller rate), so level 1 *is*
    level 0 there whatever the blocks hold.  No group is cleared either: one level 1 cleared costs
    D >= 65536 - 16384 against at most 184 * (48 + 15 * 9 + 18 - 8) = 35512 of rate, so level 2 is
    level 1.  Sign data hiding then sees the same levels and the same remainders.  These equalities
    are what those variants assert."""
    lg, _, _, _, bd, qp = case
    qbits, qscale = rq.qparams(lg, bd, qp)
    halves = (1 << qbits) <= 2 * qscale  # a step of at most two coefficient units
    for sdh in (False, True):
        for lam in (0.5, 1.5):
            l0, l1, l2 = (out[(r, sdh, 0.5 if r == 0 else lam, True)][0] for r in (0, 1, 2))
            if halves and lam == 0.5:
                assert np.array_equal(l1, l0) and np.array_equal(l2, l1), (case, sdh, lam, "a whole or half level moved")
                continue
            assert (l1 != l0).any(), (case, sdh, lam, "level 1 equals level 0 everywhere")
            if lg >= 3:
                assert (l2 != l1).any(), (case, sdh, lam, "level 2 equals level 1 everywhere")


def test_model_block_function_is_the_composition_the_cases_use():
    """the model's own transform_quant_block is the composition the cases use"""
    case = (3, True, False, 1, 8, 22)
    res, out = expected(case)
    for b in (5, 20, 40):
        lev, rec, flag = rq.transform_quant_block(res[b], _dct32(), 3, 8, 22, True, False, 1, True, 2, rq.lam_of(1.5))
        want = out[(2, True, 1.5, True)]
        assert np.array_equal(lev, want[0][b]) and np.array_equal(rec, want[1][b]) and flag == want[2][b]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_probe_equals_model(case):
    import torch

    from govideocompressor_amd.ops import native
    lg, intra, dst, scan, bd, qp = case
    n = 1 << lg
    res, out = expected(case)
    assert_rdoq_matters(case, out)
    hip = native.hip()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_res = torch.from_numpy(res).to(dev)
    d_lev = torch.empty((NBLK, n, n), dtype=torch.int16, device=dev)
    d_rec = torch.empty((NBLK, n, n), dtype=torch.int32, device=dev)
    d_flag = torch.empty((NBLK,), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for var in _variants(lg):
        rdoq, sdh, lam, mfma = var
        d_lev.fill_(POISON_LEV)
        d_rec.fill_(POISON_REC)
        d_flag.fill_(POISON_FLAG)
        hip.hevc_tq_probe(NBLK, d_res.data_ptr(), d_lev.data_ptr(), d_rec.data_ptr(), d_flag.data_ptr(), lg, bd, qp,
                          int(intra), int(dst), scan, int(sdh), rdoq, rq.lam_of(lam) if rdoq else 0, int(mfma), stream)
        torch.cuda.synchronize(dev)
        lev, rec, flag = d_lev.cpu().numpy().astype(np.int64), d_rec.cpu().numpy().astype(np.int64), d_flag.cpu().numpy()
        wl, wr, wf = out[var]
        assert np.array_equal(flag, wf), (var, np.flatnonzero(flag != wf)[:8].tolist())
        bad = np.flatnonzero((lev != wl).any(axis=(1, 2)))
        assert bad.size == 0, (var, "levels", bad[:8].tolist(), np.argwhere(lev[bad[0]] != wl[bad[0]])[:4].tolist())
        bad = np.flatnonzero((rec != wr).any(axis=(1, 2)))
        assert bad.size == 0, (var, "reconstruction", bad[:8].tolist())


def test_probe_refuses_parameters_outside_its_domain():
    import torch

    from govideocompressor_amd.ops import native
    hip = native.hip()
    t = torch.zeros(1024, dtype=torch.int32, device="cuda")
    ok = dict(log2n=3, bd=8, qp=30, intra=1, dst=0, scan=0, sdh=0, rdoq=1, rdoq_lam=368, mfma=1)
    for bad in (dict(log2n=6), dict(log2n=1), dict(bd=9), dict(qp=52), dict(dst=1), dict(scan=3), dict(rdoq=3),
                dict(rdoq_lam=1473), dict(rdoq_lam=-1)):
        with pytest.raises(ValueError):
            hip.hevc_tq_probe(1, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), stream=0, **{**ok, **bad})
